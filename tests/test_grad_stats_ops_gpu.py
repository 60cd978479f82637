"""GPU: the gradient-tracking kernels alone (csrc/gradstat.hip) -- ctvae_grad_segment_stats and ctvae_grad_segment_hist against
numpy on the same fp32 values.

One table holds every segment shape the kernels can go wrong on: widths 1 / 63 / 64 / 65, one chunk - 1 / + 0 / + 1, several
chunks, many rows with ``period > width`` and ``col_lo > 0``, two neighbouring column ranges of one block (whose chunk boundaries
fall inside rows), rows of width 1, a 32-float segment next to multi-chunk ones, bases at every offset from a 16-byte boundary,
and three special segments: all equal, all zero, no finite value.  Values: normal draws over sixty decades with +-0, denormals,
+-inf and NaN strewn in (every other segment stays finite, so that its norms are numbers).

Exact: the non-finite counts, the finite min / max as bits (-0 orders below +0), all 64 bin counts (``optim.histc_bins``, which
tests/test_grad_stats_host.py holds against torch.histc), the copied flag words.  Norms for p = 1, 2, 3.5 and inf: within relative
1e-6 of the float64 value.  That bound is derived, not measured: the squares of fp32 inputs are exact in double, a double sum of
n < 2^27 terms is off by less than 1e-8, what remains is one rounding of the result with a margin for pow / sqrt.  The gradient
buffer and the guard words around every output and every partial come back untouched."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 8
SPECIALS = [0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -5.877e-39, 1.0, -1.0]
NONFINITE = [float("inf"), float("-inf"), float("nan")]
SCALES = [1.0, 1.0 / 6.0]
FILL = -3.0                      # what the gradient buffer holds outside every segment


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _chunk():
    from ctvae_amd import native
    return int(native.load().ctvae_grad_segment_chunk_floats())


def _layout():
    """[(label, base, rows, period, col_lo, width)]; blocks are laid out back to back with gaps that walk base % 4 through 0..3."""
    C = _chunk()
    shapes = [("w1", 1, 1, [(0, 1)]), ("w63", 1, 63, [(0, 63)]), ("w64", 1, 64, [(0, 64)]), ("w65", 1, 65, [(0, 65)]),
              ("bias32", 1, 32, [(0, 32)]),
              ("chunk-1", 1, C - 1, [(0, C - 1)]), ("chunk", 1, C, [(0, C)]), ("chunk+1", 1, C + 1, [(0, C + 1)]),
              ("chunks", 1, 3 * C + 77, [(0, 3 * C + 77)]),
              ("rows", 37, 100, [(7, 63)]),                          # period > width, col_lo > 0
              ("heads", 130, 96, [(0, 40), (40, 56)]),               # two neighbouring column ranges, both longer than a chunk
              ("col", 300, 5, [(2, 1)]),                             # rows of width 1
              ("equal", 1, 100, [(0, 100)]), ("zero", 1, 70, [(0, 70)]), ("nofinite", 1, 50, [(0, 50)])]
    out, off = [], 0
    for i, (label, rows, period, cols) in enumerate(shapes):
        off += (i % 4 - off % 4) % 4 + (4 if i % 5 == 0 else 0)                 # base % 4 == i % 4
        for j, (col_lo, width) in enumerate(cols):
            out.append((label if len(cols) == 1 else f"{label}{j}", off, rows, period if rows > 1 else width, col_lo, width))
        off += rows * period if rows > 1 else cols[0][1]
    return out, off + 5


def _elements(seg):
    _, base, rows, period, col_lo, width = seg
    return (base + np.arange(rows)[:, None] * period + col_lo + np.arange(width)[None, :]).reshape(-1)


def _key(v):
    b = v.view(np.int32).astype(np.int64)
    return np.where(b < 0, b ^ 0x7fffffff, b)


@pytest.fixture(scope="module")
def case(dev):
    """The table, the gradient buffer between guard words, its host copy, and per scale the numpy reference of every segment."""
    from ctvae_amd import kernels as K
    from ctvae_amd.optim import histc_bins
    segs, n = _layout()
    assert sorted({s[1] % 4 for s in segs}) == [0, 1, 2, 3]
    gen = torch.Generator().manual_seed(99)
    host = torch.full((n,), FILL, dtype=torch.float32)
    for i, seg in enumerate(segs):
        idx = torch.from_numpy(_elements(seg))
        m = idx.numel()
        v = torch.randn(m, generator=gen) * torch.pow(10.0, torch.randint(-30, 30, (m,), generator=gen).float())
        pool = SPECIALS + (NONFINITE if i % 2 else [])
        where = torch.randperm(m, generator=gen)[:max(1, min(m, max(len(pool), m // 16)))]
        v[where] = torch.tensor(pool, dtype=torch.float32)[torch.randint(0, len(pool), (len(where),), generator=gen)]
        if seg[0] == "equal":
            v[:] = 0.375
        elif seg[0] == "zero":
            v[:] = 0.0
            v[::3] = -0.0
        elif seg[0] == "nofinite":
            v = torch.tensor(NONFINITE, dtype=torch.float32)[torch.randint(0, 3, (m,), generator=gen)]
        host[idx] = v
    buf = torch.full((GUARD + n + GUARD,), 7.0, dtype=torch.float32, device=dev)
    g = buf[GUARD:GUARD + n]
    g.copy_(host)
    table = K.GradSegmentTable([s[1:] for s in segs], n, dev, nflags=3, guard=GUARD)
    ref = {}
    hv = host.numpy()
    for scale in SCALES:
        rows = []
        for seg in segs:
            v = (hv[_elements(seg)] * np.float32(scale)).astype(np.float32)
            fin = v[np.isfinite(v)]
            r = {"v": v, "bad": int(v.size - fin.size), "fin": int(fin.size)}
            if fin.size:
                k = _key(fin)
                r["min"], r["max"] = fin[np.argmin(k)], fin[np.argmax(k)]
                r["hist"] = np.bincount(histc_bins(fin, r["min"], r["max"]), minlength=64)
            else:
                r["min"], r["max"], r["hist"] = np.float32(np.inf), np.float32(-np.inf), np.zeros(64, np.int64)
            rows.append(r)
        ref[scale] = rows
    return {"segs": segs, "n": n, "buf": buf, "g": g, "host": host, "table": table, "ref": ref}


def _norm64(v, p):
    a = np.abs(v.astype(np.float64))
    if np.isnan(a).any():
        return math.nan
    if math.isinf(p):
        return float(a.max())
    if np.isinf(a).any():
        return math.inf
    with np.errstate(all="ignore"):
        return math.fsum(a ** p) ** (1.0 / p) if p != 2 else math.sqrt(math.fsum(a * a))


def _bits(x):
    return np.asarray(x, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("p", [1.0, 2.0, 3.5, math.inf])
@pytest.mark.parametrize("scale", SCALES, ids=["scale1", "scale1/6"])
def test_stats_and_histograms_match_numpy(case, scale, p):
    from ctvae_amd import kernels as K
    table, g, segs, ref = case["table"], case["g"], case["segs"], case["ref"][scale]
    flags = torch.tensor([1, 0, 5], dtype=torch.int32, device=g.device)
    K.grad_segment_stats(table, g, scale, p, flags)
    sums0, rng0, bad0, hist0, flags0 = table.fetch()
    assert not bool(hist0.any()), "the stats pass leaves the bin counts zeroed"
    K.grad_segment_hist(table, g, scale)
    torch.cuda.synchronize()
    sums, rng, bad, hist, fl = table.fetch()
    assert torch.equal(sums.view(torch.int64), sums0.view(torch.int64)), "the histogram pass changed the sums"      # (as bits: NaN)
    assert torch.equal(rng.view(torch.int32), rng0.view(torch.int32)) and torch.equal(bad, bad0)
    assert fl.tolist() == [1, 0, 5] and flags0.tolist() == [1, 0, 5]
    saw = set()
    for i, (seg, r) in enumerate(zip(segs, ref)):
        label = seg[0]
        assert int(bad[i]) == r["bad"], label
        assert _bits(rng[i, 0].item()) == _bits(r["min"]) and _bits(rng[i, 1].item()) == _bits(r["max"]), (label, rng[i], r["min"], r["max"])
        got = hist[i].numpy().astype(np.int64)
        assert np.array_equal(got, r["hist"]), (label, np.nonzero(got != r["hist"])[0][:8])
        assert int(got.sum()) == r["fin"], label
        want = _norm64(r["v"], p)
        total, amax = float(sums[i, 0]), float(sums[i, 1])
        have = amax if math.isinf(p) else (math.sqrt(total) if p == 2 else total ** (1.0 / p))
        if math.isnan(want):
            assert math.isnan(have), label
            saw.add("nan")
        elif math.isinf(want):
            assert have == math.inf, label
            saw.add("inf")
        else:
            print(f"{label} p={p} scale={scale:.4f}: norm {have!r} float64 {want!r} rel {abs(have - want) / max(want, 1e-300):.2e}")
            assert abs(have - want) <= 1e-6 * want, (label, have, want)
            saw.add("finite")
        amax_want = _norm64(r["v"], math.inf)
        assert (math.isnan(amax) and math.isnan(amax_want)) or amax == amax_want, label
    assert {"nan", "finite"} <= saw
    assert torch.equal(case["g"].cpu().view(torch.int32), case["host"].view(torch.int32)), "the gradient buffer changed"
    b = case["buf"].cpu()
    assert bool((b[:GUARD] == 7.0).all()) and bool((b[GUARD + case["n"]:] == 7.0).all())
    assert table.guards_intact()


def test_the_inputs_exercise_what_they_claim(case):
    ref = case["ref"][1.0]
    by = {s[0]: r for s, r in zip(case["segs"], ref)}
    assert by["nofinite"]["fin"] == 0 and by["nofinite"]["bad"] == 50 and not by["nofinite"]["hist"].any()
    assert by["equal"]["hist"][32] == 100 and by["zero"]["hist"][32] == 70
    assert _bits(by["zero"]["min"]) == _bits(-0.0) and _bits(by["zero"]["max"]) == _bits(0.0)
    allv = np.concatenate([r["v"] for r in ref])
    assert np.isnan(allv).any() and (allv == np.inf).any() and (allv == -np.inf).any()
    a = np.abs(allv[np.isfinite(allv)])
    assert ((a > 0) & (a < 1.1754944e-38)).any(), "no denormal among the values"
    assert any(np.count_nonzero(r["hist"]) > 8 for r in ref), "every histogram is degenerate"
    assert by["heads0"]["v"].size > _chunk() and by["heads1"]["v"].size > _chunk()


def test_results_do_not_depend_on_the_run(case):
    """No floating-point atomics: two runs leave the same bits in every output."""
    from ctvae_amd import kernels as K
    table, g = case["table"], case["g"]
    runs = []
    for _ in range(2):
        K.grad_segment_stats(table, g, SCALES[1], 3.5, torch.zeros(3, dtype=torch.int32, device=g.device))
        K.grad_segment_hist(table, g, SCALES[1])
        runs.append(table.raw.cpu().clone())
    assert torch.equal(runs[0], runs[1])


def test_wrappers_refuse_bad_arguments(case, dev):
    from ctvae_amd import kernels as K
    table, g = case["table"], case["g"]
    flags = torch.zeros(3, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        K.grad_segment_stats(table, g[:-1], 1.0, 2.0, flags)
    with pytest.raises(ValueError):
        K.grad_segment_stats(table, g, 1.0, 2.0, None)
    with pytest.raises(ValueError):
        K.grad_segment_stats(table, g, 1.0, 0.0, flags)
    with pytest.raises(ValueError):
        K.grad_segment_hist(table, g.double())
