"""Float64 NumPy restatement of the Gaussian-mixture prior (ct-vae_amd/latentprior.py, csrc/gmm.hip), written from the formulas of
include/ctvae_hip.h and of the issue: one E step, one M step (the centred single-pass form the kernel uses), the full EM loop,
``log_prob`` and ``sample``.  No GPU import and no scikit-learn import: tests/test_latent_prior_host.py pins it to scikit-learn's
recorded results (tests/golden/gmm_sklearn.npz), the GPU tests compare the kernels with it."""
import numpy as np

EPS10 = 10 * np.finfo(np.float64).eps
LOG_2PI = np.log(2.0 * np.pi)
GOLDEN_CASES = (("full_10", 700, 10, 3, "full"), ("diag_10", 700, 10, 3, "diag"), ("full_40", 640, 40, 4, "full"))
GOLDEN_SEEDS = {"full_10": (100, 200), "diag_10": (101, 201), "full_40": (102, 309)}      # (blobs, blob_start): starts that end
#                                                                                         # with every condition number below 1e4


def finite_rows(X):
    return np.isfinite(np.asarray(X, dtype=np.float64)).all(axis=1)


def factor(cov, covariance):
    """(L, P, log_det_half): the lower Cholesky factors of ``cov`` [K, D, D] (sqrt(var) [K, D] for diag), their inverses, and
    sum log diag(L_k)."""
    cov = np.asarray(cov, dtype=np.float64)
    if covariance == "full":
        L = np.linalg.cholesky(cov)
        eye = np.eye(cov.shape[1])
        P = np.stack([np.tril(np.linalg.solve(Lk, eye)) for Lk in L])
        ldh = np.log(np.diagonal(L, axis1=1, axis2=2)).sum(axis=1)
    else:
        L = np.sqrt(cov)
        P = 1.0 / L
        ldh = np.log(L).sum(axis=1)
    return L, P, ldh


def log_prob_parts(X, weights, means, cov, covariance):
    """lp [N, K] = log_w[k] - 0.5 |P_k (x_n - mu_k)|^2 - log_det_half[k] - 0.5 D log(2 pi), for the rows as given."""
    X = np.asarray(X, dtype=np.float64)
    _, P, ldh = factor(cov, covariance)
    N, D = X.shape
    K = len(weights)
    lp = np.empty((N, K))
    for k in range(K):
        xc = X - np.asarray(means, dtype=np.float64)[k]
        y = xc @ P[k].T if covariance == "full" else xc * P[k]
        lp[:, k] = np.log(weights[k]) - 0.5 * (y * y).sum(axis=1) - ldh[k] - 0.5 * D * LOG_2PI
    return lp


def estep(X, weights, means, cov, covariance):
    """(r [N, K], ll [N], nonfinite [N]): ll = logsumexp_k lp with the maximum subtracted, r = exp(lp - ll); a row with a
    non-finite value gets r = 0, ll = 0 and flag 1."""
    X = np.asarray(X, dtype=np.float64)
    ok = finite_rows(X)
    lp = log_prob_parts(np.where(ok[:, None], X, 0.0), weights, means, cov, covariance)
    m = lp.max(axis=1)
    ll = m + np.log(np.exp(lp - m[:, None]).sum(axis=1))
    r = np.exp(lp - ll[:, None])
    return np.where(ok[:, None], r, 0.0), np.where(ok, ll, 0.0), (~ok).astype(np.int32)


def msums(X, r, nonfinite, m, covariance):
    """The M step's sums centred at ``m`` [K, D]: Nk [K], S1 [K, D], S2 [K, D, D] (or its diagonal [K, D])."""
    X = np.asarray(X, dtype=np.float64)
    ok = np.asarray(nonfinite) == 0
    Xf, rf = X[ok], np.asarray(r, dtype=np.float64)[ok]
    K, D = np.asarray(m).shape
    Nk = rf.sum(axis=0)
    S1 = np.empty((K, D))
    S2 = np.empty((K, D, D) if covariance == "full" else (K, D))
    for k in range(K):
        xc = Xf - np.asarray(m, dtype=np.float64)[k]
        S1[k] = rf[:, k] @ xc
        S2[k] = (rf[:, k, None] * xc).T @ xc if covariance == "full" else rf[:, k] @ (xc * xc)
    return Nk, S1, S2


def mfinish(Nk, S1, S2, m, covariance, reg_covar):
    """The host's end of the M step: nk = Nk + 10 eps (scikit-learn's guard), w = nk / sum nk (= Nk / N_finite up to that guard),
    mu = m + S1 / nk, Sigma = S2 / nk - (mu - m)(mu - m)^T + reg_covar I."""
    m = np.asarray(m, dtype=np.float64)
    nk = np.asarray(Nk, dtype=np.float64) + EPS10
    d = np.asarray(S1, dtype=np.float64) / nk[:, None]
    if covariance == "full":
        cov = np.asarray(S2, dtype=np.float64) / nk[:, None, None] - d[:, :, None] * d[:, None, :] + reg_covar * np.eye(m.shape[1])
    else:
        cov = np.asarray(S2, dtype=np.float64) / nk[:, None] - d * d + reg_covar
    return nk / nk.sum(), m + d, cov


def mstep(X, r, nonfinite, m, covariance, reg_covar):
    return mfinish(*msums(X, r, nonfinite, m, covariance), m, covariance, reg_covar)


def fit(X, init, covariance, reg_covar=1e-6, max_iter=100, tol=1e-3):
    """scikit-learn's loop: E step, M step, stop when |delta mean ll| < tol.  Returns (weights, means, cov, info); info holds
    ``iterations``, ``converged``, ``loglik_trace``, ``rows``, ``nonfinite`` and ``states``, the parameters every iteration
    started from."""
    w, mu, cov = (np.asarray(a, dtype=np.float64).copy() for a in init)
    trace, states, prev, converged, it = [], [], None, False, 0
    ok = finite_rows(X)
    for it in range(1, max_iter + 1):
        states.append((w, mu, cov))
        r, ll, bad = estep(X, w, mu, cov, covariance)
        mean_ll = ll.sum() / ok.sum()
        trace.append(mean_ll)
        w, mu, cov = mstep(X, r, bad, mu, covariance, reg_covar)
        if prev is not None and abs(mean_ll - prev) < tol:
            converged = True
            break
        prev = mean_ll
    return w, mu, cov, {"iterations": it, "converged": converged, "loglik_trace": trace, "rows": int(ok.sum()),
                        "nonfinite": int((~ok).sum()), "states": states}


def mean_log_prob(X, weights, means, cov, covariance):
    """The mean of ll over the finite rows (scikit-learn's ``score``)."""
    _, ll, bad = estep(X, weights, means, cov, covariance)
    return ll.sum() / (bad == 0).sum()


def standard_log_prob(X):
    X = np.asarray(X, dtype=np.float64)
    return -0.5 * (X * X).sum(axis=1) - 0.5 * X.shape[1] * LOG_2PI


def component_of(u, weights):
    """The first index whose running sum of the weights exceeds u (K - 1 when none does)."""
    cdf = np.cumsum(np.asarray(weights, dtype=np.float64))
    k = (np.asarray(u, dtype=np.float64)[:, None] >= cdf[None, :]).sum(axis=1)
    return np.minimum(k, len(cdf) - 1).astype(np.int32)


def sample(u, eps, weights, means, cov, covariance):
    """(z [n, D], k [n]): z = mu_k + L_k eps."""
    L, _, _ = factor(cov, covariance)
    k = component_of(u, weights)
    eps = np.asarray(eps, dtype=np.float64)
    means = np.asarray(means, dtype=np.float64)
    if covariance == "full":
        z = means[k] + np.einsum("nij,nj->ni", L[k], eps)
    else:
        z = means[k] + L[k] * eps
    return z, k


def default_start(X, K, seed, covariance, reg_covar=1e-6):
    """The library's default start: K distinct finite rows (``torch.randperm`` of a CPU generator seeded with ``seed`` over the
    finite rows' indices), the data's biased covariance plus reg_covar for every component, uniform weights."""
    import torch
    X = np.asarray(X, dtype=np.float64)
    idx = np.nonzero(finite_rows(X))[0]
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    pick = idx[torch.randperm(len(idx), generator=g)[:K].numpy()]
    Xf = X[idx]
    xc = Xf - Xf.mean(axis=0)
    if covariance == "full":
        cov = xc.T @ xc / len(Xf) + reg_covar * np.eye(X.shape[1])
    else:
        cov = (xc * xc).mean(axis=0) + reg_covar
    return np.full(K, 1.0 / K), X[pick].copy(), np.repeat(cov[None], K, axis=0)


def blobs(seed, N, D, K, spread=2.0):
    """A seeded data set: K blobs with unequal scales and mixing matrices, stored as fp32; its condition numbers stay small."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(K, D)) * spread
    scales = 0.5 + 1.5 * rng.random(K)
    which = rng.integers(0, K, size=N)
    which[:K] = np.arange(K)
    X = np.empty((N, D))
    for k in range(K):
        A = np.eye(D) + 0.3 * rng.normal(size=(D, D)) / np.sqrt(D)
        n = int((which == k).sum())
        X[which == k] = centres[k] + scales[k] * rng.normal(size=(n, D)) @ A.T
    return X.astype(np.float32)


def blob_start(X, K, seed, covariance, reg_covar=1e-6):
    """A start for the comparisons: K rows of X drawn with ``default_rng(seed)`` as the means, the data's covariance, uniform
    weights."""
    rng = np.random.default_rng(seed)
    X = np.asarray(X, dtype=np.float64)
    pick = rng.choice(len(X), size=K, replace=False)
    xc = X - X.mean(axis=0)
    cov = xc.T @ xc / len(X) + reg_covar * np.eye(X.shape[1]) if covariance == "full" else (xc * xc).mean(axis=0) + reg_covar
    return np.full(K, 1.0 / K), X[pick].copy(), np.repeat(cov[None], K, axis=0)
