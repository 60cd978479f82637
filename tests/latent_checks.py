"""Shared by the latent-statistics tests (no GPU, imported by nothing in the product): a float64 numpy restatement of
csrc/latentstat.hip -- ``ref_accumulate`` adds the rows of a batch one at a time in ascending order, which is the kernel's
contract: float32 -> float64 is exact, the product of two float32 values is exact in float64 and a float64 add rounds once, so
``mu_sum``, ``cov_sum`` and the counts must match to the bit; ``kl_sum`` and ``sig2_sum`` go through ``exp`` and match within
``kl_bound`` -- and seeded input builders."""
import numpy as np

KEYS = ("kl_sum", "mu_sum", "sig2_sum", "cov_sum", "nonfinite", "rows")


def new_state(L):
    """The accumulators of ctvae_latent_accumulate, zeroed."""
    return {"kl_sum": np.zeros(L, np.float64), "mu_sum": np.zeros(L, np.float64), "sig2_sum": np.zeros(L, np.float64),
            "cov_sum": np.zeros((L, L), np.float64), "nonfinite": np.zeros(L, np.int32), "rows": np.zeros(1, np.int32)}


def ref_accumulate(state, mu, logvar):
    """Adds mu, logvar [B, L] float32 into ``state`` IN PLACE, one row at a time in ascending row order; returns it."""
    mu, logvar = np.asarray(mu), np.asarray(logvar)
    assert mu.dtype == np.float32 and logvar.dtype == np.float32 and mu.ndim == 2 and mu.shape == logvar.shape
    with np.errstate(all="ignore"):
        for r in range(mu.shape[0]):
            m, lv = mu[r].astype(np.float64), logvar[r].astype(np.float64)
            s2 = np.exp(lv)
            state["kl_sum"] = state["kl_sum"] + 0.5 * (((m * m + s2) - lv) - 1.0)
            state["mu_sum"] = state["mu_sum"] + m
            state["sig2_sum"] = state["sig2_sum"] + s2
            state["cov_sum"] = state["cov_sum"] + np.outer(m, m)
            state["nonfinite"] += (~np.isfinite(mu[r]) | ~np.isfinite(logvar[r])).astype(np.int32)
            state["rows"][0] += 1
    return state


def kl_bound(mu, logvar):
    """Per column: 16 * 2^-53 * sum over rows of (mu^2 + exp(lv) + |lv| + 1).  Derived: the device's and numpy's double exp are
    each within 1 ulp of exp(lv), a term has three further roundings, and the adds run in the same order on both sides, so
    the two sums differ by a few ulps of the magnitudes that went in.  A dropped or doubled row, or an fp32 exp, is off by at
    least 2^-24 relative."""
    m, lv = np.asarray(mu, np.float64), np.asarray(logvar, np.float64)
    return 16.0 * 2.0 ** -53 * (m * m + np.exp(lv) + np.abs(lv) + 1.0).sum(axis=0)


def inputs(seed, B, L, constant_col=None):
    """mu ~ N(0, 1), logvar uniform in [-6, 2], float32 [B, L]; column ``constant_col`` is mu = 0, logvar = 0 (a collapsed
    dimension: KL 0, sigma^2 1)."""
    rng = np.random.default_rng(seed)
    mu = rng.standard_normal((B, L)).astype(np.float32)
    lv = rng.uniform(-6.0, 2.0, size=(B, L)).astype(np.float32)
    if constant_col is not None:
        mu[:, constant_col] = 0.0
        lv[:, constant_col] = 0.0
    return mu, lv
