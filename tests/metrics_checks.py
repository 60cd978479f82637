"""Shared by tests/test_metrics_host.py, tests/test_metrics_ops_gpu.py and tests/test_metrics_gpu.py: a numpy restatement of
the two disentanglement metrics of ctvae_amd/metrics.py (MIG, Chen et al. 2018; FactorVAE score, Kim & Mnih 2018, both as
disentanglement_lib implements them), of the three kernels of csrc/disent.hip they are built from, and the seeded input
generators of the kernel tests.  Sums run in float64; only the bin edges are float32, because the contract fixes them as
``lo + k * ((hi - lo) / 20)`` with every operation rounded to float32.

The restatement checks its own inputs: ``ref_bins`` asserts that no value sits within ``margin`` bin widths of an edge
(where float32 and float64 binning could differ), ``ref_group_argmin`` asserts a relative gap between the two smallest
ratios of every group (where the arg-min could flip).  Nothing in the product imports this module.
"""
from functools import lru_cache

import numpy as np

NUM_BINS = 20
ACTIVE_STD = 0.05
MARGIN = 1e-3
GAP = 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
def ref_moments(z):
    """z [N, L] float32 -> mean, var (ddof = 1) in float64; min, max in float32 (exact)."""
    z64 = np.asarray(z, dtype=np.float64)
    return z64.mean(axis=0), z64.var(axis=0, ddof=1), np.asarray(z).min(axis=0), np.asarray(z).max(axis=0)


def ref_edges(lo, hi):
    """edges [20, L] float32: lo + k * ((hi - lo) / 20), each operation rounded to float32; hi == lo -> lo - 0.5, hi + 0.5."""
    lo = np.asarray(lo, dtype=np.float32).copy()
    hi = np.asarray(hi, dtype=np.float32).copy()
    same = hi == lo
    lo[same] = lo[same] - np.float32(0.5)
    hi[same] = hi[same] + np.float32(0.5)
    w = ((hi - lo) / np.float32(NUM_BINS)).astype(np.float32)
    k = np.arange(NUM_BINS, dtype=np.float32)[:, None]
    kw = (k * w[None, :]).astype(np.float32)
    return (lo[None, :] + kw).astype(np.float32), w


def ref_bins(z, lo, hi, margin=MARGIN):
    """np.digitize(x, np.histogram(x, 20)[1][:-1]) per column: the number of edges <= x (1..20), uint8 [N, L].
    Input condition (asserted unless margin is None): every value is at least ``margin`` bin widths away from every edge, except
    a value that EQUALS the first edge (the column minimum, whose comparison is exact in any precision) and a constant column."""
    z = np.asarray(z, dtype=np.float32)
    edges, w = ref_edges(lo, hi)
    d = z[:, None, :].astype(np.float64) - edges[None, :, :].astype(np.float64)          # [N, 20, L]
    if margin is not None:
        near = np.abs(d) < margin * w.astype(np.float64)[None, None, :]
        near[:, 0, :] &= d[:, 0, :] != 0.0
        # a constant column sits in the middle of [x - 0.5, x + 0.5], i.e. ON edge 10 whatever its value: no margin exists, so
        # there the condition is that the float32 edge EQUALS the value (then the comparison is exact and the bin is 11)
        const = np.asarray(lo) == np.asarray(hi)
        assert (edges[10, const] == z[:, const]).all(), "a constant column whose float32 edge 10 misses its value"
        near[:, :, const] = False
        assert not near.any(), f"{int(near.sum())} values within {margin} bin widths of an edge"
    assert (d[:, 0, :] >= 0).all(), "a value below the first edge"
    return (d >= 0).sum(axis=1).astype(np.uint8)


def ref_mi(bins, factors, sizes, chunk=512):
    """Mutual information in nats [L, F] between the bin columns [N, L] (1..20) and the factor columns [N, F]."""
    bins = np.asarray(bins, dtype=np.int64)
    factors = np.asarray(factors, dtype=np.int64)
    N, L = bins.shape
    out = np.zeros((L, len(sizes)), dtype=np.float64)
    for f, S in enumerate(sizes):
        ps = np.bincount(factors[:, f], minlength=S) / N                                   # [S]
        for c0 in range(0, L, chunk):
            b = bins[:, c0:c0 + chunk] - 1
            C = b.shape[1]
            joint = np.zeros((C, NUM_BINS, S), dtype=np.float64)
            np.add.at(joint, (np.arange(C)[None, :].repeat(N, 0), b, factors[:, f][:, None].repeat(C, 1)), 1.0)
            joint /= N
            pb = joint.sum(axis=2, keepdims=True)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = joint * np.log(joint / (pb * ps[None, None, :]))
            out[c0:c0 + C, f] = np.where(joint > 0, t, 0.0).sum(axis=(1, 2))
    return out


def ref_entropy(values, S):
    """H = MI(f, f) of a factor column in nats."""
    p = np.bincount(np.asarray(values, dtype=np.int64), minlength=S) / float(len(values))
    p = p[p > 0]
    return float(-(p * np.log(p)).sum())


def ref_group_argmin(z, global_var, active, gap=GAP):
    """z [G, B, L] -> (arg [G], val [G]): arg-min over the active columns of var_B (ddof = 1) / global_var, lowest index on a
    tie.  Input condition (asserted unless gap is None): the two smallest ratios of every group differ by >= gap, relative."""
    z64 = np.asarray(z, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):          # an inactive column may have no variance at all
        ratio = z64.var(axis=1, ddof=1) / np.asarray(global_var, dtype=np.float64)[None, :]
    ratio[:, ~np.asarray(active, dtype=bool)] = np.inf
    arg = ratio.argmin(axis=1)
    val = ratio[np.arange(len(arg)), arg]
    if gap is not None and np.asarray(active, dtype=bool).sum() > 1:
        second = np.partition(ratio, 1, axis=1)[:, 1]
        rel = (second - val) / np.maximum(second, np.finfo(np.float64).tiny)
        assert (rel >= gap).all(), f"smallest relative gap {rel.min():.3e} < {gap}"
    return arg, val


# ---------------------------------------------------------------------------------------------------------------------
# metrics (fed the product's plan and the product's codes)
# ---------------------------------------------------------------------------------------------------------------------
def ref_mig(z, factors, sizes, margin=MARGIN):
    """z [N, L] codes of the factor rows [N, F] -> mig.discrete_score."""
    _, _, lo, hi = ref_moments(z)
    mi = ref_mi(ref_bins(z, lo, hi, margin), factors, sizes)                       # [L, F]
    top = np.sort(mi, axis=0)[::-1]
    factors = np.asarray(factors, dtype=np.int64)
    ent = np.array([ref_entropy(factors[:, f], S) for f, S in enumerate(sizes)])
    return float(np.mean((top[0] - top[1]) / ent))


def ref_factor_vae(z_var, z_train, fixed_train, z_eval, fixed_eval, num_factors, gap=GAP):
    """Codes of the variance items [V, L] and of the train / eval groups [G, B, L] with their fixed factors [G] -> the three
    factor_vae.* results."""
    gvar = np.asarray(z_var, dtype=np.float64).var(axis=0, ddof=1)
    active = np.sqrt(gvar) >= ACTIVE_STD
    if not active.any():
        return {"factor_vae.train_accuracy": 0.0, "factor_vae.eval_accuracy": 0.0, "factor_vae.num_active_dims": 0}
    L = gvar.shape[0]

    def votes(z, fixed):
        v = np.zeros((num_factors, L), dtype=np.int64)
        np.add.at(v, (np.asarray(fixed), ref_group_argmin(z, gvar, active, gap)[0]), 1)
        return v

    train, ev = votes(z_train, fixed_train), votes(z_eval, fixed_eval)
    classifier = train.argmax(axis=0)
    cols = np.arange(L)
    return {"factor_vae.train_accuracy": float(train[classifier, cols].sum() / train.sum()),
            "factor_vae.eval_accuracy": float(ev[classifier, cols].sum() / ev.sum()),
            "factor_vae.num_active_dims": int(active.sum())}


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs of the kernel tests
# ---------------------------------------------------------------------------------------------------------------------
MOMENT_SHAPES = [(2, 1), (63, 10), (512, 130), (64, 8192)]
MI_SIZES = (2, 15, 183)
MI_SHAPES = [(320, 10), (320, 130), (64, 8192)]
ARGMIN_SHAPES = [(1, 2, 3), (7, 16, 130), (40, 64, 8192)]


@lru_cache(maxsize=None)
def moment_inputs(N, L):
    """Columns with their own offset (|mean| ~ 0.5..3: a relative bound on the mean is meaningful) and scale; the last column
    is constant (var = 0)."""
    rng = np.random.default_rng(1000 + 7 * N + L)
    off = rng.uniform(0.5, 3.0, L) * rng.choice([-1.0, 1.0], L)
    z = (off[None, :] + rng.uniform(0.01, 1.0, L)[None, :] * rng.standard_normal((N, L))).astype(np.float32)
    z[:, L - 1] = np.float32(off[L - 1])
    z.setflags(write=False)
    return z


@lru_cache(maxsize=None)
def mi_inputs(N, L, sizes=MI_SIZES):
    """z = lo + (b + u) * w with b a random bin and u in [0.25, 0.75]; rows 0 / 1 hold each column's exact lo / hi; column
    min(3, L-1) is constant; columns l % 5 == 0 follow factor (l // 5) % F so that some MI entries are large.
    Returns (z, lo, hi, factors int32, reference bins, reference mi): computed once, read-only."""
    rng = np.random.default_rng(2000 + 7 * N + L)
    F = len(sizes)
    factors = np.stack([rng.integers(0, S, N) for S in sizes], axis=1).astype(np.int32)
    lo = rng.uniform(-2.0, 2.0, L)
    w = rng.uniform(0.01, 1.0, L)
    b = rng.integers(0, NUM_BINS, (N, L))
    for l in range(0, L, 5):
        f = (l // 5) % F
        b[:, l] = (factors[:, f].astype(np.int64) * NUM_BINS) // sizes[f]
    u = rng.uniform(0.25, 0.75, (N, L))
    z = (lo[None, :] + (b + u) * w[None, :]).astype(np.float32)
    z[0, :] = lo.astype(np.float32)
    z[1, :] = (lo + NUM_BINS * w).astype(np.float32)
    const = min(3, L - 1)
    z[:, const] = np.float32(0.75)
    lo32, hi32 = z.min(axis=0), z.max(axis=0)
    assert lo32[const] == hi32[const]
    bins = ref_bins(z, lo32, hi32)
    assert bins.min() == 1 and bins.max() == NUM_BINS and (bins[1, np.arange(L) != const] == NUM_BINS).all()
    mi = ref_mi(bins, factors, sizes)
    for a in (z, lo32, hi32, factors, bins, mi):
        a.setflags(write=False)
    return z, lo32, hi32, factors, bins, mi


@lru_cache(maxsize=None)
def argmin_inputs(G, B, L):
    """z [G, B, L] ~ N(0, 1) * column scale; inactive columns at the first index, the last index and at random (about a fifth);
    in every group one active column is scaled down until its ratio is 1/16 of the smallest other one (the asserted gap).
    Returns (z, global_var, active uint8, reference arg, reference val)."""
    rng = np.random.default_rng(3000 + 101 * G + 7 * B + L)
    scale = rng.uniform(0.5, 2.0, L)
    z = rng.standard_normal((G, B, L)) * scale[None, None, :]
    active = rng.uniform(size=L) > 0.2
    active[0] = False
    active[L - 1] = False
    if not active.any():
        active[L // 2] = True
    gvar = (scale ** 2 * rng.uniform(0.8, 1.25, L)).astype(np.float32)
    idx = np.flatnonzero(active)
    # the chosen column's ratio becomes the smallest by a wide margin: its rows shrink until the ratio is 1/16 of the group's
    # smallest other ratio (B = 2 leaves a chi-square with one degree of freedom, so a fixed factor would not do)
    for g in range(G):
        c = idx[rng.integers(len(idx))]
        ratio = z[g].var(axis=0, ddof=1) / gvar
        others = np.delete(idx, np.searchsorted(idx, c))
        target = (ratio[others].min() if len(others) else ratio[c]) / 16.0
        z[g, :, c] *= np.sqrt(target / ratio[c])
    z = z.astype(np.float32)
    arg, val = ref_group_argmin(z, gvar, active)
    act8 = active.astype(np.uint8)
    for a in (z, gvar, act8, arg, val):
        a.setflags(write=False)
    return z, gvar, act8, arg, val
