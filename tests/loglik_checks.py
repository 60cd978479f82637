"""Float64 NumPy restatement of csrc/loglik.hip and ctvae_amd/loglik.py's finish, written from the formulas of
include/ctvae_hip.h and of Burda et al. 2016, section 5.  No torch, no GPU import: tests/test_loglik_host.py pins it against
``np.logaddexp`` and a closed form, the GPU tests compare the kernels with it.

* ``latent_terms`` / ``latent_a``   the per-dimension terms z^2 - eps^2 - log_var and a = -0.5 * their sum (``math.fsum``)
* ``sse_rows`` / ``log_weights``    the squared error per decoder row (``math.fsum`` of exact float64 squares' roundings) and
                                    lw = -sse / (2 sigma^2) - (P / 2) log(2 pi sigma^2) + a
* ``merge`` / ``finish``            the sequential state (m, s, s2, t, n) and flag, operation by operation as the kernel does,
                                    and loglik = m + log s - log n, elbo = t / n, ess = s^2 / s2
* ``linear_gaussian``               decoder xhat = W z + b with the exact posterior q = p(z|x) and the exact log p(x)
"""
import math

import numpy as np

CUTS = ([24], [1, 7, 16], [1] * 24)          # three ways to cut 24 samples into chunks


def consts(sigma, P):
    s2 = float(sigma) * float(sigma)
    return 1.0 / (2.0 * s2), 0.5 * P * math.log(2.0 * math.pi * s2)


def latent_terms(z, eps, log_var, S):
    """[R, L] float64: z^2 - eps^2 - log_var, row r of z / eps against row r // S of log_var."""
    z, eps, lv = (np.asarray(t, dtype=np.float64) for t in (z, eps, log_var))
    R, L = z.shape
    return z * z - eps.reshape(R, L) ** 2 - np.repeat(lv, S, axis=0)


def latent_a(z, eps, log_var, S):
    """(a [R], sum_d |terms| [R]): a = log p(z) - log q(z|x) from the z given."""
    t = latent_terms(z, eps, log_var, S)
    return np.array([-0.5 * math.fsum(row) for row in t.tolist()]), np.abs(t).sum(1)


def reparameterize(mu, log_var, eps, S):
    """(z [R, L] float64, |mu| + |exp(0.5 lv) eps| [R, L]) from fp32 inputs, all in float64."""
    mu, lv = (np.repeat(np.asarray(t, dtype=np.float64), S, axis=0) for t in (mu, log_var))
    e = np.asarray(eps, dtype=np.float64).reshape(mu.shape)
    step = np.exp(0.5 * lv) * e
    return mu + step, np.abs(mu) + np.abs(step)


def sse_rows(xhat, x, S):
    """[R] float64: sum_i (xhat[r][i] - x[r // S][i])^2 over the flattened rows, by ``math.fsum``."""
    xhat = np.asarray(xhat, dtype=np.float64).reshape(len(xhat), -1)
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    assert len(xhat) == len(x) * S
    out = np.empty(len(xhat))
    for r in range(len(xhat)):
        d = xhat[r] - x[r // S]
        out[r] = math.fsum((d * d).tolist())
    return out


def log_weights(xhat, x, S, z, eps, log_var, sigma):
    """(lw [R], scale [R]): the log-weights and sse / (2 sigma^2) + |const| + sum_d |latent terms|, what their rounding error
    is measured against.  ``z`` None: a = 0."""
    P = int(np.asarray(x)[0].size)
    c0, c1 = consts(sigma, P)
    sse = sse_rows(xhat, x, S)
    if z is None:
        a, mag = np.zeros(len(sse)), np.zeros(len(sse))
    else:
        a, mag = latent_a(z, eps, log_var, S)
    return -sse * c0 - c1 + a, sse * c0 + abs(c1) + mag


def new_state(B):
    st = np.zeros((B, 5))
    st[:, 0] = -np.inf
    return st, np.zeros(B, dtype=np.int32)


def merge(state, flags, lw, S, row0=0):
    """The chunk's log-weights lw [B * S] into rows [row0, row0 + B) of (state, flags), in place, one at a time."""
    lw = np.asarray(lw, dtype=np.float64).reshape(-1, S)
    for b, row in enumerate(lw):
        m, s, s2, t, n = state[row0 + b]
        for v in row.tolist():
            if not math.isfinite(v):
                flags[row0 + b] = 1
                continue
            if v > m:
                c = math.exp(m - v)
                s = s * c + 1.0
                s2 = s2 * (c * c) + 1.0
                m = v
            else:
                e = math.exp(v - m)
                s = s + e
                s2 = s2 + e * e
            t = t + v
            n = n + 1.0
        state[row0 + b] = (m, s, s2, t, n)
    return state, flags


def merge_cut(lw, cut):
    """(state, flags) of lw [B, K] merged in chunks of the sizes in ``cut``."""
    lw = np.asarray(lw, dtype=np.float64)
    assert sum(cut) == lw.shape[1]
    state, flags = new_state(len(lw))
    at = 0
    for S in cut:
        merge(state, flags, np.ascontiguousarray(lw[:, at:at + S]).reshape(-1), S)
        at += S
    return state, flags


def finish(state):
    """(loglik, elbo, ess) [B] of a state whose rows hold at least one sample."""
    m, s, s2, t, n = (np.asarray(state, dtype=np.float64)[:, i] for i in range(5))
    return m + np.log(s) - np.log(n), t / n, s * s / s2


def estimate(lw):
    """(loglik, elbo, ess) of lw [B, K] in one chunk."""
    return finish(merge_cut(lw, [np.asarray(lw).shape[1]])[0])


def linear_gaussian(seed, P, L, sigma, B=3):
    """A model whose marginal is known: z ~ N(0, I), x = W z + b + sigma * noise, with orthogonal columns in W so that the exact
    posterior is diagonal -- the family ``ctvae_loglik_latent`` samples from: precision 1 + |w_d|^2 / sigma^2 per dimension.
    Returns float64 arrays: ``W`` [P, L], ``b`` [P], ``x`` [B, P], the exact posterior's ``mu`` and ``log_var`` [B, L], and the
    exact ``logpx`` [B] = log N(x; b, W W^T + sigma^2 I)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((P, L)))
    scale = 0.5 + rng.random(L)
    W = Q * scale
    b = 0.1 * rng.standard_normal(P)
    x = rng.standard_normal((B, L)) @ W.T + b + sigma * rng.standard_normal((B, P))
    s2 = sigma * sigma
    var = 1.0 / (1.0 + (W * W).sum(0) / s2)                      # [L]; W^T W is diagonal
    mu = ((x - b) @ W) * var / s2
    cov = W @ W.T + s2 * np.eye(P)
    _, logdet = np.linalg.slogdet(cov)
    d = x - b
    logpx = -0.5 * (np.einsum("bi,bi->b", d @ np.linalg.inv(cov), d) + logdet + P * math.log(2.0 * math.pi))
    return {"W": W, "b": b, "x": x, "mu": mu, "log_var": np.tile(np.log(var), (B, 1)), "logpx": logpx, "sigma": float(sigma)}


def linear_gaussian_log_weights(case, eps, dtype=np.float64):
    """(lw [B, K], z, xhat) of eps [B, K, L] under the exact posterior through ``log_weights``.  ``dtype``: the precision z and xhat
    are formed and stored in (float32: what a device decoder hands over); the log-weights are float64 over those values."""
    W, b, x, mu, lv = (case[k].astype(dtype) for k in ("W", "b", "x", "mu", "log_var"))
    B, K, L = eps.shape
    e = np.asarray(eps, dtype=dtype).reshape(B * K, L)
    z = (np.repeat(mu, K, axis=0) + np.exp(dtype(0.5) * np.repeat(lv, K, axis=0)) * e).astype(dtype)
    xhat = (z @ W.T + b).astype(dtype)
    lw, _ = log_weights(xhat, x, K, z, e, lv, case["sigma"])
    return lw.reshape(B, K), z, xhat
