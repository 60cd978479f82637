"""Shared by the EMA-codebook tests (tests/test_vq_ema_*.py): a float64 restatement of what csrc/vqema.hip computes -- the
window statistics with the slice quirk and the update of van den Oord et al. 2017, appendix A.1 -- and the error bounds the GPU
tests hold the kernels to.  The reference project has no EMA codebook: these formulas ARE the definition.

Layouts are the kernels': latents ``x`` [P = B*HW][D], indices [B][C][HW], codebooks / M / acc_s [C][K][Dc], N / acc_n [C][K].
"""
import struct

import torch

from tests.vq_checks import U32, rows_of


def fp32(v: float) -> float:
    return struct.unpack("f", struct.pack("f", v))[0]


def stats64(x, inds, K):
    """(counts int64 [C, K], sums float64 [C, K, Dc], abs-sums float64 [C, K, Dc], invalid) of latents x [P, D] (any float dtype,
    cast up here) under indices [B, C, HW]: codebook c reads columns c .. c + Dc - 1.  An index outside [0, K) counts in
    ``invalid`` and nowhere else."""
    rows = rows_of(inds)                                  # [P, C]
    P, C = rows.shape
    Dc = x.shape[1] // C
    x = x.double()
    counts = torch.zeros(C, K, dtype=torch.int64)
    sums = torch.zeros(C, K, Dc, dtype=torch.float64)
    asums = torch.zeros(C, K, Dc, dtype=torch.float64)
    invalid = 0
    for c in range(C):
        idx = rows[:, c]
        ok = (idx >= 0) & (idx < K)
        invalid += int((~ok).sum())
        xs = x[ok][:, c:c + Dc]
        counts[c] = torch.bincount(idx[ok], minlength=K)
        sums[c].index_add_(0, idx[ok], xs)
        asums[c].index_add_(0, idx[ok], xs.abs())
    return counts, sums, asums, invalid


def update64(N, M, acc_n, acc_s, decay, eps):
    """The update in float64 on the given (fp32 or float64) inputs; decay and eps are used as given (pass the fp32-rounded values).
    Returns dict(N, M, Nt, E, n) -- n per codebook."""
    N, M, acc_n, acc_s = N.double(), M.double(), acc_n.double(), acc_s.double()
    K = N.shape[1]
    N1 = decay * N + (1.0 - decay) * acc_n
    M1 = decay * M + (1.0 - decay) * acc_s
    n = N1.sum(dim=1, keepdim=True)
    Nt = (N1 + eps) / (n + K * eps) * n
    return dict(N=N1, M=M1, Nt=Nt, E=M1 / Nt[..., None], n=n[:, 0])


# The kernel forms N' = fma(g, N, fl32((1-g) * acc_n)) and M' likewise, 1 - g and the product in float64 (exact, or rounded far
# below fp32's unit): two fp32 roundings, of values no larger than |g old| + |(1-g) acc| (1 + u) -- the (1 + 2u) below covers the
# second-order terms.  E = M' / Nt: the two roundings of M', the two of N' inside Nt (N and acc_n are non-negative, so the
# magnitude is N' itself; n moves by less), the rounding of Nt (float64 -> fp32) and the division (at most 2.5 ulp were it not
# correctly rounded): 2 + 2 + 1 + 2.5 < 8, the constant the issue sets.
UPD_ROUNDINGS_NM = 2.0 * (1.0 + 2.0 * U32)
UPD_ROUNDINGS_E = 8.0


def update_bounds(N, M, acc_n, acc_s, decay, eps):
    """Element bounds of the update against ``update64`` on the same inputs: dict(N, M, E)."""
    ref = update64(N, M, acc_n, acc_s, decay, eps)
    mag_n = (decay * N.double()).abs() + ((1.0 - decay) * acc_n.double()).abs()
    mag_m = (decay * M.double()).abs() + ((1.0 - decay) * acc_s.double()).abs()
    return dict(N=UPD_ROUNDINGS_NM * U32 * mag_n, M=UPD_ROUNDINGS_NM * U32 * mag_m,
                E=UPD_ROUNDINGS_E * U32 * mag_m / ref["Nt"][..., None])


def stats_bound(counts, asums):
    """A fixed-order fp32 sum of n_k terms errs by at most (n_k - 1) u sum |x| to first order, whatever the order; n_k u sum |x|
    covers the second-order terms and the slice-wise regrouping."""
    return counts.double()[..., None] * U32 * asums
