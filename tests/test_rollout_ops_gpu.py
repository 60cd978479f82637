"""GPU: csrc/acteval.hip (ctvae_action_hits) and the per-image grid (ctvae_image_grid_each_u8 through
imagegrid.make_grid_u8(scale_each=True)) against the numpy restatements of tests/rollout_checks.py.  Counts are integers and the
grid inputs keep every byte away from a rounding boundary (asserted by the restatement), so both comparisons are EXACT."""
import numpy as np
import pytest
import torch

from tests import grid_checks as G
from tests import rollout_checks as R

pytestmark = pytest.mark.gpu

FILL = 0xAA
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import imagegrid, native, rollout
    native.load()
    return imagegrid, native, rollout


def _hits(native, probas, action, counts=None):
    """One launch over numpy [N, A] inputs; counts: a device tensor to add into (default zeros).  Returns int64 numpy [A, 3]."""
    N, A = probas.shape
    p, a = torch.from_numpy(probas).cuda(), torch.from_numpy(action).cuda()
    if counts is None:
        counts = torch.zeros(A, 3, dtype=torch.int32, device="cuda")
    native.call("ctvae_action_hits", p.data_ptr(), a.data_ptr(), N, A, counts.data_ptr())
    torch.cuda.synchronize()
    return counts.cpu().numpy().astype(np.int64)


def hit_inputs(seed, N, A):
    """Random probability rows and one-hot actions, then as many crafted rows as fit (the row's action is a):
    p = a + V and p = a - V (direction-agnostic hit, directed miss), an all-equal row, NaN first, NaN later, an all -inf row,
    a tie of two maxima, and a soft action row that is not one-hot."""
    rng = np.random.default_rng(seed)
    V = A // 2
    probas = rng.random((N, A), dtype=np.float32)
    probas /= probas.sum(axis=1, keepdims=True)
    act_idx = rng.integers(0, A, size=N)
    hit = rng.random(N) < 0.4
    probas[np.arange(N)[hit], act_idx[hit]] = 2.0                 # a good share of directed hits
    action = np.zeros((N, A), dtype=np.float32)
    action[np.arange(N), act_idx] = 1.0

    def onehot(i, val=1.0):
        r = np.zeros(A, dtype=np.float32)
        r[i] = val
        return r

    a_lo, a_hi = V - 1, A - 1
    soft = rng.random(A, dtype=np.float32) * 0.1
    soft[a_hi] = 0.5
    tie = onehot(a_lo, 3.0)
    tie[a_hi] = 3.0                                              # the first maximum (a_lo) wins
    nan_later = onehot(0, 9.0)
    nan_later[a_hi] = NAN
    crafted = [(onehot(a_lo + V), onehot(a_lo)), (onehot(a_hi - V), onehot(a_hi)), (np.full(A, 0.25, np.float32), onehot(0)),
               (np.concatenate([[NAN], np.full(A - 1, 5.0)]).astype(np.float32), onehot(0)), (nan_later, onehot(a_hi)),
               (np.full(A, -INF, np.float32), onehot(0)), (tie, onehot(a_lo)), (onehot(a_hi), soft)]
    for r, (p, a) in enumerate(crafted[:max(N - 1, 0)]):         # (row 0 stays random)
        probas[N - 1 - r], action[N - 1 - r] = p, a
    return probas, action


HIT_CASES = [(1, 2), (3, 12), (64, 12), (65, 20), (130, 80), (257, 6), (5, 256)]


@pytest.mark.parametrize("N,A", HIT_CASES)
def test_action_hits_equal_the_restatement(mods, N, A):
    _, native, _ = mods
    probas, action = hit_inputs(100 + N, N, A)
    want = R.hits_ref(probas, action)
    got = _hits(native, probas, action)
    assert np.array_equal(got, want), (got - want)
    assert got[:, 0].sum() == N
    if N >= 9:                                                  # every crafted row is in: hits and misses of each kind exist
        assert 0 < got[:, 1].sum() < got[:, 2].sum() < N


def test_action_hits_crafted_rows_alone(mods):
    """The eight crafted rows by themselves, A = 12: each row's verdict is known without the restatement."""
    _, native, _ = mods
    probas, action = hit_inputs(5, 9, 12)
    probas, action = probas[1:][::-1].copy(), action[1:][::-1].copy()
    got = _hits(native, probas, action)
    want = np.zeros((12, 3), dtype=np.int64)
    # a = 5: p = 11 (nodir), tie -> 5 (both);  a = 11: p = 5 (nodir), NaN later -> p = 11 (both), soft action -> p = 11 (both)
    # a = 0: all-equal -> 0, NaN first -> 0, all -inf -> 0 (all directed hits)
    want[5], want[11], want[0] = [2, 1, 2], [3, 2, 3], [3, 3, 3]
    assert np.array_equal(got, want), got


def test_action_hits_accumulate(mods):
    """Two launches over the two halves equal one launch over the whole; a pre-filled counts is added to, not overwritten;
    N = 0 leaves it untouched."""
    _, native, _ = mods
    probas, action = hit_inputs(9, 130, 20)
    whole = _hits(native, probas, action)
    counts = torch.zeros(20, 3, dtype=torch.int32, device="cuda")
    _hits(native, probas[:67], action[:67], counts)
    assert np.array_equal(_hits(native, probas[67:], action[67:], counts), whole)
    pre = torch.arange(60, dtype=torch.int32, device="cuda").reshape(20, 3) * 1000
    assert np.array_equal(_hits(native, probas, action, pre.clone()), whole + pre.cpu().numpy())
    kept = pre.clone()
    p = torch.from_numpy(probas).cuda()
    native.call("ctvae_action_hits", p.data_ptr(), p.data_ptr(), 0, 20, kept.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(kept, pre)


def test_action_hits_bad_arguments(mods):
    _, native, rollout = mods
    p = torch.zeros(4 * 258, device="cuda")
    counts = torch.full((258 * 3,), 7, dtype=torch.int32, device="cuda")
    for A in (3, 13, 0, 1, 258, -2):
        with pytest.raises(RuntimeError, match="bad argument"):
            native.call("ctvae_action_hits", p.data_ptr(), p.data_ptr(), 4, A, counts.data_ptr())
    with pytest.raises(RuntimeError, match="bad argument"):
        native.call("ctvae_action_hits", p.data_ptr(), p.data_ptr(), -1, 12, counts.data_ptr())
    for args in ((None, p.data_ptr(), counts.data_ptr()), (p.data_ptr(), None, counts.data_ptr()), (p.data_ptr(), p.data_ptr(), None)):
        with pytest.raises(RuntimeError, match="bad argument"):
            native.call("ctvae_action_hits", args[0], args[1], 4, 12, args[2])
    with pytest.raises(RuntimeError, match="bad argument"):
        rollout.ActionHits(13, "cuda").update(torch.zeros(2, 13, device="cuda"), torch.zeros(2, 13, device="cuda"))
    torch.cuda.synchronize()
    assert bool((counts == 7).all())


def test_action_hits_class_reads_views_and_other_dtypes(mods):
    """ActionHits.update: a non-contiguous probas view and float64 inputs give the contiguous float32 result; counts() and
    result() agree with the restatement; an empty batch is a no-op."""
    _, _, rollout = mods
    probas, action = hit_inputs(13, 65, 12)
    want = R.hits_ref(probas, action)
    wide = torch.zeros(65, 24, device="cuda")
    wide[:, ::2] = torch.from_numpy(probas).cuda()
    view = wide[:, ::2]
    assert not view.is_contiguous()
    h = rollout.ActionHits(12, torch.device("cuda"))
    h.update(view, torch.from_numpy(action).cuda())
    h.update(torch.zeros(0, 12, device="cuda"), torch.zeros(0, 12, device="cuda"))
    assert np.array_equal(h.counts(), want)
    h.update(torch.from_numpy(probas).cuda().double(), torch.from_numpy(action).cuda().double())
    assert np.array_equal(h.counts(), 2 * want)
    assert h.result() == rollout.summarize(2 * want)
    with pytest.raises(ValueError, match=r"\[N, 12\]"):
        h.update(torch.zeros(3, 10, device="cuda"), torch.zeros(3, 10, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# make_grid_u8(normalize=True, scale_each=True)
# ---------------------------------------------------------------------------------------------------------------------
def _run(IG, xt, scanlines, **kw):
    """make_grid_u8 into a 0xAA buffer with 32 spare bytes -> (the stream as numpy [Hg, pitch], the spare bytes)."""
    N, _, H, W = xt.shape
    _, _, Hg, Wg = G.geometry(N, H, W, kw.get("nrow", 8), kw.get("padding", 2))
    total = Hg * ((1 if scanlines else 0) + 3 * Wg)
    buf = torch.full(((total + 3) // 4 * 4 + 32,), FILL, dtype=torch.uint8, device=xt.device)
    got = IG.make_grid_u8(xt, scanlines=scanlines, out=buf, **kw)
    assert got.data_ptr() == buf.data_ptr() and got.numel() == total
    torch.cuda.synchronize()
    return got.cpu().numpy().reshape(Hg, -1), buf[total:].cpu().numpy()


GRID_CASES = [(1, 3, 5, 7, 8), (3, 1, 4, 4, 2), (7, 3, 9, 6, 3), (13, 3, 64, 64, 12), (72, 3, 64, 64, 6)]
_want = {}


def _case(case):
    """(the case's input, its restatement as scanlines): made once, shared by the four variants, never written to."""
    if case not in _want:
        x = R.each_inputs(30 + case[0], case[:4])
        want = R.grid_each_ref(x, nrow=case[4], scanlines=True)
        x.setflags(write=False)
        want.setflags(write=False)
        _want[case] = (x, want)
    return _want[case]


@pytest.mark.parametrize("scanlines", [True, False])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
@pytest.mark.parametrize("case", GRID_CASES)
def test_scale_each_grid_equals_the_restatement(mods, case, layout, scanlines):
    IG = mods[0]
    x, want = _case(case)
    xt = torch.from_numpy(x.copy()).cuda()
    if layout == "channels_last":
        xt = xt.contiguous(memory_format=torch.channels_last)
        if case[0] > 1 and case[1] > 1:
            assert not xt.is_contiguous()
    got, spare = _run(IG, xt, scanlines, nrow=case[4], normalize=True, scale_each=True)
    want = want if scanlines else want[:, 1:]
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"
    assert (spare == FILL).all()


def test_scale_each_reads_a_strided_window_in_place(mods):
    """A window of a larger tensor (not dense, not 16-byte aligned: the range pass's element-wise path)."""
    IG = mods[0]
    x, want = _case((7, 3, 9, 6, 3))
    big = torch.full((7, 3, 12, 11), 99.0, device="cuda")          # 99 outside the window would wreck a range if it were read
    big[:, :, 2:11, 3:9] = torch.from_numpy(x.copy()).cuda()
    win = big[:, :, 2:11, 3:9]
    assert not win.is_contiguous() and win.data_ptr() % 16 != 0
    got, spare = _run(IG, win, True, nrow=3, normalize=True, scale_each=True)
    assert np.array_equal(got, want) and (spare == FILL).all()


def test_scale_each_identities(mods):
    """Byte-identical: one image with and without scale_each; a value_range given; normalize off; and scale_each=False is what
    the existing entry point returns."""
    IG, native, _ = mods
    one = torch.from_numpy(G.grid_inputs(41, (1, 3, 9, 6))).cuda()
    assert torch.equal(IG.make_grid_u8(one, normalize=True, scale_each=True), IG.make_grid_u8(one, normalize=True))
    x = torch.from_numpy(R.each_inputs(42, (7, 3, 9, 6))).cuda()
    kw = dict(nrow=3, padding=1, pad_value=0.5, scanlines=True)
    ranged = IG.make_grid_u8(x, normalize=True, value_range=(-1.0, 2.0), **kw)
    assert torch.equal(IG.make_grid_u8(x, normalize=True, value_range=(-1.0, 2.0), scale_each=True, **kw), ranged)
    assert torch.equal(IG.make_grid_u8(x, scale_each=True, **kw), IG.make_grid_u8(x, **kw))
    batch = IG.make_grid_u8(x, normalize=True, scale_each=False, **kw)
    assert not torch.equal(IG.make_grid_u8(x, normalize=True, scale_each=True, **kw), batch)
    Hg, pitch = batch.shape
    raw = torch.full(((Hg * pitch + 3) // 4 * 4,), FILL, dtype=torch.uint8, device="cuda")
    ws = native.workspace(x.device)
    native.call("ctvae_image_grid_u8", x.data_ptr(), *x.stride(), 7, 3, 9, 6, 3, 1, 1, 0, 0.0, 1.0, 0.5, 1, raw.data_ptr(), raw.numel(),
                ws.data_ptr(), ws.numel() * 4)
    assert torch.equal(raw[:Hg * pitch].view(Hg, pitch), batch)
    # the C entry itself: with a range, or without normalize, it IS the existing entry
    for normalize, has_range in ((1, 1), (0, 0)):
        outs = []
        for entry in ("ctvae_image_grid_u8", "ctvae_image_grid_each_u8"):
            o = torch.full_like(raw, FILL)
            native.call(entry, x.data_ptr(), *x.stride(), 7, 3, 9, 6, 3, 1, normalize, has_range, -1.0, 2.0, 0.5, 1, o.data_ptr(),
                        o.numel(), ws.data_ptr(), ws.numel() * 4)
            outs.append(o)
        assert torch.equal(outs[0], outs[1])


def test_scale_each_launch_shape_and_bad_arguments(mods):
    IG, native, _ = mods
    x = torch.from_numpy(R.each_inputs(43, (13, 3, 8, 8))).cuda()
    native.prof_report()
    native.prof_enable(True)
    try:
        IG.make_grid_u8(x, normalize=True, scale_each=True)
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    assert {k: v["count"] for k, v in native.prof_report().items()} == {"grid_range_each_kernel": 1, "grid_compose_each_kernel": 1}
    lib = native.load()
    out = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")
    ws = native.workspace(x.device)
    xp, op, wp, st = x.data_ptr(), out.data_ptr(), ws.data_ptr(), native.stream_ptr()

    def call(xp=xp, C=3, nrow=8, pad=2, op=op, ob=8192, wp=wp, wb=4096, N=4, H=8, W=8):
        return lib.ctvae_image_grid_each_u8(xp, C * H * W, H * W, W, 1, N, C, H, W, nrow, pad, 1, 0, 0.0, 1.0, 0.0, 1, op, ob, wp, wb, st)

    codes = {"C=2": call(C=2), "nrow=0": call(nrow=0), "pad=-1": call(pad=-1), "x NULL": call(xp=None), "out NULL": call(op=None),
             "workspace NULL": call(wp=None), "workspace too small": call(wb=4 * 8 - 1), "out too small": call(ob=12 * 127 - 1),
             "out misaligned": call(op=op + 4), "N=0": call(N=0), "H=0": call(H=0)}
    assert all(c == -22 for c in codes.values()), codes
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    assert call(ob=12 * 127, wb=4 * 8) == 0                 # the smallest buffers that pass: 4 images x 1 part x 8 bytes
    torch.cuda.synchronize()
