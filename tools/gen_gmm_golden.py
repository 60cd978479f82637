"""Record tests/golden/gmm_sklearn.npz: what scikit-learn's ``GaussianMixture`` ends with on three seeded data sets.

    python tools/gen_gmm_golden.py            # needs scikit-learn (recorded with 1.7.2); no GPU

Per case of ``prior_checks.GOLDEN_CASES`` -- (N, D, K) = (700, 10, 3) full, (700, 10, 3) diag, (640, 40, 4) full -- the file holds
the fp32 data ``<case>_X`` (``prior_checks.blobs``), the start ``<case>_w0`` / ``_mu0`` / ``_cov0`` (``prior_checks.blob_start``) and
the ``weights_``, ``means_``, ``covariances_`` and ``score(X)`` of
``GaussianMixture(tol=0, max_iter=6, reg_covar=1e-6, weights_init, means_init, precisions_init)`` as ``<case>_w`` / ``_mu`` / ``_cov`` /
``_score``.  tests/test_latent_prior_host.py compares the float64 restatement (tests/prior_checks.py) with them.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import prior_checks as PC  # noqa: E402

REG_COVAR, MAX_ITER = 1e-6, 6


def sklearn_fit(X, init, covariance, max_iter=MAX_ITER, reg_covar=REG_COVAR):
    """(weights_, means_, covariances_, score(X)) of scikit-learn from the given start, ``tol=0``."""
    from sklearn.mixture import GaussianMixture
    w0, mu0, cov0 = init
    prec0 = np.linalg.inv(cov0) if covariance == "full" else 1.0 / cov0
    gm = GaussianMixture(n_components=len(w0), covariance_type=covariance, tol=0.0, max_iter=max_iter, reg_covar=reg_covar,
                         weights_init=w0, means_init=mu0, precisions_init=prec0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")           # (tol=0 never converges: that is the point)
        gm.fit(np.asarray(X, dtype=np.float64))
    return gm.weights_, gm.means_, gm.covariances_, gm.score(np.asarray(X, dtype=np.float64))


def main():
    out = {}
    for name, N, D, K, covariance in PC.GOLDEN_CASES:
        data_seed, start_seed = PC.GOLDEN_SEEDS[name]
        X = PC.blobs(data_seed, N, D, K)
        init = PC.blob_start(X, K, start_seed, covariance, REG_COVAR)
        w, mu, cov, score = sklearn_fit(X, init, covariance)
        out.update({f"{name}_X": X, f"{name}_w0": init[0], f"{name}_mu0": init[1], f"{name}_cov0": init[2], f"{name}_w": w,
                    f"{name}_mu": mu, f"{name}_cov": cov, f"{name}_score": np.asarray(score)})
    path = os.path.join(ROOT, "tests", "golden", "gmm_sklearn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
