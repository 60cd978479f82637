"""GPU: csrc/imggrid.hip through imagegrid.make_grid_u8 against the float64 restatement of tests/grid_checks.py.  The inputs keep
every v*255 + 0.5 at least 0.05 from an integer (asserted there), so the comparison is exact byte equality over the WHOLE output:
the test pre-fills the buffer with 0xAA, so borders, empty cells and filter bytes count like pixels, and the bytes behind the
stream must still be 0xAA.  Shapes: the smallest at which each branch can break (module table in DESIGN.md 4.11)."""
import numpy as np
import pytest
import torch

from tests import grid_checks as G

pytestmark = pytest.mark.gpu

FILL = 0xAA


@pytest.fixture(scope="module")
def IG():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import imagegrid, native
    native.load()
    return imagegrid


def _run(IG, xt, scanlines=True, **kw):
    """make_grid_u8 into a 0xAA buffer with 32 spare bytes -> (the stream as numpy [Hg, pitch], the spare bytes)."""
    N, _, H, W = xt.shape
    _, _, Hg, Wg = G.geometry(N, H, W, kw.get("nrow", 8), kw.get("padding", 2))
    total = Hg * ((1 if scanlines else 0) + 3 * Wg)
    buf = torch.full(((total + 3) // 4 * 4 + 32,), FILL, dtype=torch.uint8, device=xt.device)
    got = IG.make_grid_u8(xt, scanlines=scanlines, out=buf, **kw)
    assert got.data_ptr() == buf.data_ptr() and got.numel() == total
    torch.cuda.synchronize()
    return got.cpu().numpy().reshape(Hg, -1), buf[total:].cpu().numpy()


def _check(IG, x, xt=None, **kw):
    """Both output forms of batch x (numpy) against the restatement; xt: the device tensor to read instead of a contiguous copy."""
    xt = torch.from_numpy(x).cuda() if xt is None else xt
    want = G.ref_grid_bytes(x, scanlines=True, **kw)
    got, spare = _run(IG, xt, scanlines=True, **kw)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"
    assert (spare == FILL).all()
    plain, spare = _run(IG, xt, scanlines=False, **kw)
    assert np.array_equal(plain, want[:, 1:]) and (spare == FILL).all()       # the scanline form minus the filter bytes
    return got


CASES = {
    "one image, pitch 34, dword tail": ((1, 3, 5, 7), dict(nrow=8, padding=2)),
    "one full row": ((12, 3, 8, 8), dict(nrow=12, padding=2)),
    "second row, 11 empty cells": ((13, 3, 8, 8), dict(nrow=12, padding=2)),
    "one channel, 3 rows, 4 empty": ((32, 1, 64, 64), dict(nrow=12, padding=2)),
    "no borders": ((5, 3, 6, 9), dict(nrow=8, padding=0)),
    "the validation batch, 794 x 794": ((144, 3, 64, 64), dict(nrow=12, padding=2)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_normalized_grid_equals_the_restatement(IG, name):
    shape, kw = CASES[name]
    got = _check(IG, G.grid_inputs(11, shape), normalize=True, **kw)
    N, _, H, W = shape
    _, _, Hg, Wg = G.geometry(N, H, W, kw["nrow"], kw["padding"])
    assert got.shape == (Hg, 1 + 3 * Wg)
    if N == 144:
        assert (Hg, Wg) == (794, 794)


def test_channels_last_and_strided_views_are_read_in_place(IG):
    """N=13, C=3, 64x64: channels_last memory (what the decoders return) and a window of a larger tensor (neither dense nor
    16-byte aligned: the range pass's element-wise path) give the bytes of the contiguous copy."""
    x = G.grid_inputs(12, (13, 3, 64, 64))
    xc = torch.from_numpy(x).cuda()
    xl = xc.contiguous(memory_format=torch.channels_last)
    assert xl.stride() == (64 * 64 * 3, 1, 64 * 3, 3)
    _check(IG, x, xt=xl, normalize=True, nrow=12)
    big = torch.full((13, 3, 70, 71), 99.0, device="cuda")            # 99 outside the window would wreck the range if it were read
    big[:, :, 3:67, 5:69] = xc
    win = big[:, :, 3:67, 5:69]
    assert not win.is_contiguous() and win.data_ptr() % 16 != 0
    _check(IG, x, xt=win, normalize=True, nrow=12)
    one = G.grid_inputs(13, (7, 1, 9, 10))
    _check(IG, one, xt=torch.from_numpy(one).cuda().expand(7, 3, 9, 10)[:, :1], normalize=True, nrow=3)


def test_value_range_and_unnormalized(IG):
    """value_range given: values below / above it clamp to 0 / 255.  normalize off: v = x, values outside [0, 1] clamp."""
    x = G.grid_inputs(14, (5, 3, 6, 9), lo=-0.5, hi=1.75, kmin=-30, kmax=290, pin=False)
    got = _check(IG, x, normalize=True, value_range=(-0.5, 1.75), nrow=3, padding=1)
    assert (got == 0).any() and (got == 255).any()
    y = G.grid_inputs(15, (5, 3, 6, 9), lo=0.0, hi=1.0, kmin=-40, kmax=300, pin=False)
    assert y.min() < -0.1 and y.max() > 1.1
    _check(IG, y, normalize=False, nrow=3, padding=1)
    _check(IG, y, normalize=False, value_range=(0.25, 0.5), nrow=3, padding=1)      # a range without normalize is not used


def test_pad_value_and_constant_batch(IG):
    """pad_value 0.5 -> 0.5*255 + 0.5 = 128 exactly (no rounding anywhere), un-normalised also under normalize; a constant
    batch (hi == lo) divides 0 by 1e-5: all image bytes 0."""
    x = G.grid_inputs(16, (13, 3, 8, 8))
    got = _check(IG, x, normalize=True, nrow=12, pad_value=0.5)
    assert got[0, 1] == 128 and got[-1, -1] == 128
    c = np.full((5, 3, 6, 9), 0.37, dtype=np.float32)
    got = _check(IG, c, normalize=True, nrow=4, padding=1, pad_value=1.0)
    img = got[:, 1:].reshape(got.shape[0], -1, 3)
    assert int((img == 0).sum()) == c.size and int((img == 255).sum()) == img.size - c.size


def test_nan_and_inf(IG):
    """One NaN and one +inf / -inf element: byte 0 / 255 / 0 at their places; the NaN does not enter the range (every other byte
    as without it).  An infinity DOES enter an automatic range, as in torch: with hi = inf every finite value lands on byte 0,
    and so does inf / inf."""
    x = G.grid_inputs(17, (3, 3, 6, 9))
    assert -1.25 < x[1, 2, 3, 4] < 2.5                      # not one of the two pinned elements
    clean = G.ref_grid_bytes(x, nrow=3, padding=1, normalize=True, scanlines=True)
    xn = x.copy()
    xn[1, 2, 3, 4] = np.nan
    got = _check(IG, xn, normalize=True, nrow=3, padding=1)
    row, byte = 1 + 3, 1 + 3 * (1 * (9 + 1) + 1 + 4) + 2
    assert got[row, byte] == 0
    diff = np.argwhere(got != clean)
    assert len(diff) <= 1 and all(tuple(d) == (row, byte) for d in diff)
    xi = G.grid_inputs(19, (3, 3, 6, 9), lo=0.0, hi=1.0, kmin=-40, kmax=300, pin=False)
    xi[1, 2, 3, 4], xi[0, 0, 0, 0], xi[2, 1, 5, 8] = np.inf, -np.inf, np.nan
    got = _check(IG, xi, normalize=False, nrow=3, padding=1)
    assert got[row, byte] == 255 and got[1, 1 + 3] == 0
    xr = xn.copy()
    xr[0, 0, 0, 0], xr[2, 1, 5, 8] = np.inf, -np.inf
    got = _check(IG, xr, normalize=True, value_range=(-1.25, 2.5), nrow=3, padding=1)
    assert got[row, byte] == 0 and got[1, 1 + 3] == 255
    xa = x.copy()
    xa[1, 2, 3, 4] = np.inf
    got = _check(IG, xa, normalize=True, nrow=3, padding=1, pad_value=1.0)
    assert int((got[:, 1:] != 255).sum()) == x.size and int((got[:, 1:] == 0).sum()) == x.size


def _launches(native, fn):
    native.prof_report()
    native.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    return out, {k: v["count"] for k, v in native.prof_report().items()}


def test_launch_shape(IG):
    """normalize without a range: the range pass and the compose pass; with value_range, or normalize off: compose only."""
    from ctvae_amd import native
    x = torch.from_numpy(G.grid_inputs(18, (13, 3, 8, 8))).cuda()
    _, log = _launches(native, lambda: IG.make_grid_u8(x, normalize=True))
    assert log == {"grid_range_kernel": 1, "grid_compose_kernel": 1}
    _, log = _launches(native, lambda: IG.make_grid_u8(x, normalize=True, value_range=(-1.0, 2.0)))
    assert log == {"grid_compose_kernel": 1}
    _, log = _launches(native, lambda: IG.make_grid_u8(x))
    assert log == {"grid_compose_kernel": 1}


def test_bad_arguments_return_the_error_code_and_launch_nothing(IG):
    from ctvae_amd import native
    lib = native.load()
    x = torch.zeros(4 * 3 * 8 * 8, device="cuda")
    out = torch.full((8192,), FILL, dtype=torch.uint8, device="cuda")
    ws = native.workspace(x.device)
    xp, op, wp, st = x.data_ptr(), out.data_ptr(), ws.data_ptr(), native.stream_ptr()

    def call(xp=xp, C=3, nrow=8, pad=2, op=op, ob=8192, wp=wp, wb=2048, N=4, H=8, W=8):
        return lib.ctvae_image_grid_u8(xp, C * H * W, H * W, W, 1, N, C, H, W, nrow, pad, 1, 0, 0.0, 1.0, 0.0, 1, op, ob, wp, wb, st)

    def all_bad():
        return {"C=2": call(C=2), "C=4": call(C=4), "nrow=0": call(nrow=0), "pad=-1": call(pad=-1), "x NULL": call(xp=None),
                "out NULL": call(op=None), "workspace NULL": call(wp=None), "workspace too small": call(wb=2040),
                "out too small": call(ob=12 * 127 - 1), "out misaligned": call(op=op + 4), "N=0": call(N=0), "H=0": call(H=0)}

    codes, log = _launches(native, all_bad)
    assert all(c == -22 for c in codes.values()), codes
    assert log == {} and bool((out == FILL).all())
    assert call(ob=12 * 127) == 0                       # 12 scanlines of 1 + 3*42 bytes: the smallest buffer that passes
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="bad argument"):
        IG.make_grid_u8(torch.zeros(2, 3, 4, 4, device="cuda"), nrow=0)
    with pytest.raises(ValueError, match="C = 1 or 3"):
        IG.make_grid_u8(torch.zeros(2, 2, 4, 4, device="cuda"))
