"""GPU: csrc/reconstat.hip through ``kernels.recon_record`` / ``kernels.recon_worst`` and ``reconstats.ReconStats``, against the
float64 numpy restatement tests/recon_checks.py (a direct 2-D windowed sum; the kernel is separable and banded).

Bounds.  Both sides are float64 over the same fp32 pictures and differ by summation order only: ``mse`` and ``mae`` agree to 1e-12
relative, ``max`` is EQUAL (a maximum has no order), ``ssim`` agrees to 1e-9 absolute -- 121-term sums of magnitudes <= R^2 at eps
1.1e-16, amplified by at most 1 / C2 ~ 1.1e3 / R^2, is about 1e-11, with two digits of margin.  Everything about batching, layout,
neighbours and the worst set's pictures is bit for bit."""
import numpy as np
import pytest
import torch

from tests import recon_checks as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _nhwc(x, dev):
    """A logical [B, C, S, S] device tensor over NHWC memory: the wrapper reads it where it lies."""
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).contiguous(memory_format=torch.channels_last)


SENTINEL = -7.5


def _records(a, b, dev, R=1.0, row0=0, cap=None, layout=_nhwc):
    """(records [B, 4], flags [B]) on the host; every row outside [row0, row0 + B) must keep its sentinel."""
    from ctvae_amd import kernels as K
    B = a.shape[0]
    cap = B + row0 if cap is None else cap
    rec = torch.full((cap, 4), SENTINEL, dtype=torch.float64, device=dev)
    flags = torch.full((cap,), 77, dtype=torch.int32, device=dev)
    K.recon_record(layout(a, dev), layout(b, dev), K.recon_consts(R), rec, flags, row0)
    rec, flags = rec.cpu().numpy(), flags.cpu().numpy()
    outside = np.ones(cap, bool)
    outside[row0:row0 + B] = False
    assert (rec[outside] == SENTINEL).all() and (flags[outside] == 77).all(), "rows outside [row0, row0 + B) were written"
    return rec[row0:row0 + B], flags[row0:row0 + B]


def _assert_close(got, want):
    for i, name in ((0, "mse"), (1, "mae")):
        err = np.abs(got[:, i] - want[:, i]) / want[:, i]
        print(name, "relative", err.max())
        assert err.max() <= 1e-12, (name, got[:, i], want[:, i])
    assert np.array_equal(got[:, 2], want[:, 2]), ("max", got[:, 2], want[:, 2])
    err = np.abs(got[:, 3] - want[:, 3])
    print("ssim absolute", err.max(), "ssim", got[:, 3])
    assert err.max() <= 1e-9, ("ssim", got[:, 3], want[:, 3])


# ---- 1. the record kernel against the restatement --------------------------------------------------------------
@pytest.mark.parametrize("kind", ["unit", "randn"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("S", [11, 12, 17, 64])
def test_records_match_the_reference(dev, S, C_, B, kind):
    a, b = C.pictures(1000 + 7 * S + C_ + 31 * B, B, C_, S, kind)
    got, flags = _records(a, b, dev)
    want, want_flags = C.ref_records(a, b)
    assert flags.tolist() == want_flags.tolist() == [0] * B
    _assert_close(got, want)


def test_data_range_enters_the_constants(dev):
    a, b = C.pictures(5, 2, 3, 20)
    a, b = (a * 255).astype(np.float32), (b * 255).astype(np.float32)
    got, _ = _records(a, b, dev, R=255.0)
    want, _ = C.ref_records(a, b, R=255.0)
    _assert_close(got, want)
    # the same pictures under R = 1: other constants, another number -- the reference's, and far outside the bound of the first
    other, _ = _records(a, b, dev, R=1.0)
    want1, _ = C.ref_records(a, b, R=1.0)
    _assert_close(other, want1)
    assert np.abs(want1[:, 3] - want[:, 3]).min() > 1e-6


def test_identical_pictures_are_exactly_one(dev):
    for S, C_, kind in ((11, 1, "unit"), (17, 3, "randn"), (64, 3, "unit")):
        a, _ = C.pictures(40 + S, 2, C_, S, kind)
        got, flags = _records(a, a.copy(), dev)
        assert got[:, 3].tolist() == [1.0, 1.0] and got[:, 0].tolist() == [0.0, 0.0], got
        assert got[:, 1].tolist() == [0.0, 0.0] and got[:, 2].tolist() == [0.0, 0.0] and flags.tolist() == [0, 0]


def test_records_do_not_depend_on_the_batching(dev):
    a, b = C.pictures(77, 5, 3, 23)
    whole, _ = _records(a, b, dev)
    first, _ = _records(a[:2], b[:2], dev, row0=7, cap=16)
    rest, _ = _records(a[2:], b[2:], dev, row0=9, cap=16)
    assert np.array_equal(np.concatenate([first, rest]).view(np.uint64), whole.view(np.uint64))
    alone, _ = _records(a[3:4], b[3:4], dev, row0=1, cap=3)
    assert np.array_equal(alone.view(np.uint64), whole[3:4].view(np.uint64))


def test_an_nchw_tensor_is_copied_and_gives_the_same_bits(dev):
    a, b = C.pictures(78, 3, 3, 19)
    nchw = lambda x, d: torch.from_numpy(x).to(d)                       # contiguous NCHW: the wrapper must copy
    assert nchw(a, dev).is_contiguous() and not nchw(a, dev).permute(0, 2, 3, 1).is_contiguous()
    got, _ = _records(a, b, dev, layout=nchw)
    want, _ = _records(a, b, dev)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # a strided view that is neither: three of four channels of a wider NHWC buffer (a pixel pitch of 4 floats)

    def padded(x, d):
        wide = torch.full(x.shape[:1] + x.shape[2:] + (x.shape[1] + 1,), 9.0, device=d)
        wide[..., :x.shape[1]] = torch.from_numpy(x).to(d).permute(0, 2, 3, 1)
        return wide[..., :x.shape[1]].permute(0, 3, 1, 2)
    assert not padded(a, dev).is_contiguous() and not padded(a, dev).permute(0, 2, 3, 1).is_contiguous()
    got, _ = _records(a, b, dev, layout=padded)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_nonfinite_rows_are_flagged_and_their_neighbours_unchanged(dev):
    a, b = C.pictures(79, 5, 3, 16)
    clean, flags = _records(a, b, dev)
    assert flags.tolist() == [0] * 5
    a2, b2 = a.copy(), b.copy()
    a2[1, 2, 15, 15] = np.nan              # the last element of the picture
    b2[3, 0, 0, 0] = np.inf                # the first, in the target
    got, flags = _records(a2, b2, dev)
    assert flags.tolist() == [0, 1, 0, 1, 0]
    keep = [0, 2, 4]
    assert np.array_equal(got[keep].view(np.uint64), clean[keep].view(np.uint64))
    a3 = a.copy()
    a3[4, 1, 7, 3] = -np.inf
    assert _records(a3, b, dev)[1].tolist() == [0, 0, 0, 0, 1]


def test_shapes_outside_the_limits_raise(dev):
    from ctvae_amd import kernels as K
    consts = K.recon_consts(1.0)
    rec, flags = torch.zeros(4, 4, dtype=torch.float64, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    for S in (10, 65):
        x = torch.zeros(1, 3, S, S, device=dev)
        with pytest.raises(ValueError, match="11 <= S <= 64"):
            K.recon_record(x, x, consts, rec, flags, 0)
    with pytest.raises(ValueError, match="one shape"):
        K.recon_record(torch.zeros(1, 3, 16, 16, device=dev), torch.zeros(1, 3, 17, 17, device=dev), consts, rec, flags, 0)
    with pytest.raises(ValueError, match="one shape"):
        K.recon_record(torch.zeros(2, 3, 16, 16, device=dev), torch.zeros(1, 3, 16, 16, device=dev), consts, rec, flags, 0)
    with pytest.raises(ValueError, match="leave the capacity 4"):
        K.recon_record(torch.zeros(3, 3, 16, 16, device=dev), torch.zeros(3, 3, 16, 16, device=dev), consts, rec, flags, 2)
    assert not rec.any().item() and not flags.any().item()              # nothing was launched
    K.recon_record(torch.zeros(0, 3, 16, 16, device=dev), torch.zeros(0, 3, 16, 16, device=dev), consts, rec, flags, 4)   # no rows: a no-op


# ---- 2. the worst set ------------------------------------------------------------------------------------------
def _stream(seed, sizes, S=12, C_=3, descending=False):
    """Batches of the given sizes.  ``descending``: the noise of batch i is three times that of batch i - 1 (0.1, 0.3, 0.9, 2.7 on
    a target of standard deviation 0.29: ssim about 0.94, 0.65, 0.17, 0.02), so every batch is worse than all before it and
    evicts.  Otherwise the stream holds an exact duplicate of image 0 at the last row (a tie in ssim), and a NaN image at row 2
    when it has one."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(sizes):
        b = rng.random((n, C_, S, S))
        if descending:
            a = b + 0.1 * 3.0 ** i * rng.standard_normal((n, C_, S, S))
        else:
            a = np.clip(b + (0.05 + 0.2 * rng.random((n, 1, 1, 1))) * rng.standard_normal((n, C_, S, S)), 0.0, 1.0)
        out.append([a.astype(np.float32), b.astype(np.float32)])
    if not descending:
        out[-1][0][-1], out[-1][1][-1] = out[0][0][0], out[0][1][0]
        flat = sum(sizes)
        if flat > 3:
            r, i = 2, 0
            while r >= sizes[i]:
                r, i = r - sizes[i], i + 1
            out[i][0][r, 0, 3, 3] = np.nan
    return [(a, b) for a, b in out]


def _recut(stream, sizes):
    a, b = np.concatenate([s[0] for s in stream]), np.concatenate([s[1] for s in stream])
    assert sum(sizes) == len(a)
    cuts = np.cumsum([0] + list(sizes))
    return [(a[lo:hi], b[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])]


def _run(stream, Kw, dev, R=1.0):
    from ctvae_amd.reconstats import ReconStats
    acc = ReconStats(dev, R, Kw)
    acc.reset()
    for a, b in stream:
        acc.observe(_nhwc(a, dev), _nhwc(b, dev))
    torch.cuda.synchronize()
    return acc, acc.result()


def _assert_worst_is(res, stream, Kw):
    rows, ssim, wa, wb = C.ref_worst(stream, Kw)
    k = int((rows >= 0).sum())
    print("worst rows", res["worst_rows"].tolist(), "reference", rows[:k].tolist())
    assert res["worst_rows"].tolist() == rows[:k].tolist()
    assert np.abs(res["worst_ssim"] - ssim[:k]).max() <= 1e-9 if k else True
    assert tuple(res["worst_recons"].shape) == (k,) + wa.shape[1:]
    assert np.array_equal(res["worst_recons"].cpu().numpy().view(np.uint32), wa[:k].view(np.uint32))      # bit for bit, NaN-safe
    assert np.array_equal(res["worst_target"].cpu().numpy().view(np.uint32), wb[:k].view(np.uint32))
    return k


@pytest.mark.parametrize("Kw", [1, 4, 32])
def test_worst_set_equals_a_sort_of_the_whole_stream(dev, Kw):
    sizes = [3, 1, 5, 3]
    stream = _stream(90 + Kw, sizes)
    acc, res = _run(stream, Kw, dev)
    k = _assert_worst_is(res, stream, Kw)
    assert k == min(Kw, 11) and res["flags"].tolist().count(1) == 1 and 2 not in res["worst_rows"].tolist()
    if Kw == 32:                       # K larger than the rows seen: the slots behind the last candidate are reported empty
        side = acc.sides[acc.cur]
        assert side["row"].cpu().tolist() == res["worst_rows"].tolist() + [-1] * (32 - k)
        assert not side["a"][k:].any().item() and not side["b"][k:].any().item()
        got = res["worst_rows"].tolist()
        assert got.index(0) + 1 == got.index(11), "the duplicate of image 0 at row 11 ties with it and goes right behind it"
    # another cut of the same stream: the same bits, records included
    for other in ([5, 3, 1, 3], [1] * 12, [12]):
        _, res2 = _run(_recut(stream, other), Kw, dev)
        for key in ("records", "flags", "worst_rows", "worst_ssim"):
            assert np.array_equal(res2[key].view(np.uint8), res[key].view(np.uint8)), (key, other)
        for key in ("worst_recons", "worst_target"):
            assert torch.equal(res2[key].view(torch.int32), res[key].view(torch.int32)), (key, other)


@pytest.mark.parametrize("Kw,sizes", [(1, [1, 1, 1]), (4, [5, 5, 5, 5]), (4, [3, 3, 3])])
def test_descending_quality_every_batch_evicts(dev, Kw, sizes):
    from ctvae_amd.reconstats import ReconStats
    stream = _stream(120 + Kw + len(sizes), sizes, S=17, descending=True)
    acc = ReconStats(dev, 1.0, Kw)
    acc.reset()
    lo = 0
    for a, b in stream:
        acc.observe(_nhwc(a, dev), _nhwc(b, dev))
        src = acc.sides[acc.cur]["source"].cpu().tolist()
        rows = acc.sides[acc.cur]["row"].cpu().tolist()
        take = min(Kw, len(a))
        assert sum(1 for s in src if s >= Kw) == take, ("every new slot that a batch can fill comes from the batch", src)
        assert sum(1 for r in rows if r >= lo) == take
        lo += len(a)
    _assert_worst_is(acc.result(), stream, Kw)


def test_worst_set_at_the_full_picture_size_and_one_channel(dev):
    for S, C_ in ((64, 3), (17, 1)):
        stream = _stream(130 + S, [3, 4, 3], S=S, C_=C_)
        _, res = _run(stream, 4, dev)
        _assert_worst_is(res, stream, 4)
        want, want_flags = C.ref_records(np.concatenate([s[0] for s in stream]), np.concatenate([s[1] for s in stream]))
        ok = want_flags == 0
        assert res["flags"].tolist() == want_flags.tolist()
        _assert_close(res["records"][ok], want[ok])


def test_accumulator_grows_resets_and_runs_without_a_worst_set(dev, monkeypatch):
    from ctvae_amd import reconstats as S
    monkeypatch.setattr(S, "FIRST_CAPACITY", 4)
    stream = _stream(140, [3, 1, 5, 3])
    acc, res = _run(stream, 0, dev)
    assert acc.flags.numel() == 16 and acc.sides is None and len(res["worst_rows"]) == 0 and res["worst_recons"] is None
    _, ref = _run(stream, 4, dev)
    assert np.array_equal(res["records"].view(np.uint8), ref["records"].view(np.uint8)), "growing the buffer moved a record"
    assert res["flags"].tolist() == ref["flags"].tolist()
    # reset: no rows, an empty set, and the next epoch is the first one again
    acc4, first = _run(stream, 4, dev)
    acc4.reset()
    assert acc4.rows == 0 and len(acc4.result()["flags"]) == 0
    for a, b in stream:
        acc4.observe(_nhwc(a, dev), _nhwc(b, dev))
    again = acc4.result()
    for key in ("records", "flags", "worst_rows", "worst_ssim"):
        assert np.array_equal(again[key].view(np.uint8), first[key].view(np.uint8)), key
    with pytest.raises(ValueError, match="pictures changed"):
        acc4.observe(torch.zeros(1, 3, 16, 16, device=dev), torch.zeros(1, 3, 16, 16, device=dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc4.observe(torch.zeros(1, 3, 12, 12), torch.zeros(1, 3, 12, 12))
