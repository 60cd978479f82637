"""GPU: the weight-average kernels alone (csrc/ema.hip), through the C ABI -- ctvae_ema_update against a float64 reference and
ctvae_buffer_swap bit for bit, on the smallest shapes where they can go wrong.

The update's bound is derived, not measured: ema' = fmaf(w, p - ema, ema) with w = 1 - decay in (0, 1).  The subtraction rounds
by at most 2^-24 * |p - ema| <= 2^-23 * max(|ema|, |p|), which w < 1 only shrinks, and the fma rounds once, by at most
2^-24 * |ema'| with |ema'| <= max(|ema|, |p|) (up to that same rounding): together below 2^-22 * max(|ema|, |p|) per element.  The
reference uses the fp32 value of w the kernel receives.  Shapes: n in {1, 3, 4, 5, 7, 1023, one full turn of the grid + 13}, the
slice starting at each of the four float offsets from a 16-byte boundary, the average once at the same phase (scalar head, 16-byte
loop, scalar tail) and once at another (float by float throughout).  Every buffer lies between guard words."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 8                      # floats on either side of a range
SMALL = [1, 3, 4, 5, 7, 1023]
W = 0.25 + 2.0 ** -20          # a 1 - decay that is exact in fp32 and is no power of two


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _wrap_n():
    from ctvae_amd import native
    return int(native.load().ctvae_grad_accumulate_pass_floats()) + 13


def _values(n, seed):
    """n finite, normal fp32 values over twenty orders of magnitude, both signs, no zero."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=gen) * torch.pow(10.0, torch.randint(-10, 10, (n,), generator=gen).float())
    return torch.where(v == 0, torch.ones(()), v)


def _placed(dev, vals, offset, fill):
    """vals on the device, ``offset`` floats behind a 16-byte boundary, between guard words of value ``fill``."""
    n = vals.numel()
    buf = torch.full((4 + GUARD + n + GUARD + 4,), fill, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    lo = GUARD + offset                         # GUARD % 4 == 0: at least GUARD guard words on either side
    view = buf[lo:lo + n]
    assert (view.data_ptr() // 4) % 4 == offset
    view.copy_(vals)
    return buf, view, lo


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _assert_guards(buf, lo, n, fill, what):
    b = buf.cpu()
    assert bool((b[:lo] == fill).all()) and bool((b[lo + n:] == fill).all()), what


def _update(ema, p, w, n=None):
    from ctvae_amd import native
    native.call("ctvae_ema_update", ema.data_ptr(), p.data_ptr(), ema.numel() if n is None else n, w)


def _swap(a, b, n=None):
    from ctvae_amd import native
    native.call("ctvae_buffer_swap", a.data_ptr(), b.data_ptr(), a.numel() if n is None else n)


def _update_case(dev, n, e_off, p_off, poison=False):
    e0, p0 = _values(n, 7 * n + 1), _values(n, 7 * n + 2)
    bad = torch.zeros(n, dtype=torch.bool)
    if poison:
        for j, v in enumerate((float("nan"), float("inf"), float("-inf"))):
            k = (j * (n // 3 + 1) + n // 5) % n
            p0[k], bad[k] = v, True
    e_buf, e, elo = _placed(dev, e0, e_off, 7.0)
    p_buf, p, plo = _placed(dev, p0, p_off, -3.0)
    assert ctypes.c_float(W).value == W
    _update(e, p, W)
    torch.cuda.synchronize()
    out = e.cpu()
    assert torch.equal(_bits(p), _bits(p0)), "the update changed p"
    _assert_guards(e_buf, elo, n, 7.0, "guard words of the average")
    _assert_guards(p_buf, plo, n, -3.0, "guard words of the parameters")
    assert torch.equal(~torch.isfinite(out), bad), "a non-finite average where p is finite, or a finite one where it is not"
    ok = ~bad
    ref = e0.double() + W * (p0.double() - e0.double())
    bound = 2.0 ** -22 * torch.maximum(e0.abs(), p0.abs()).double()
    err = (out.double() - ref).abs()
    worst = float((err[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0
    print(f"n {n} offsets {e_off}/{p_off}: max error / bound {worst:.3f}")
    assert bool((err[ok] <= bound[ok]).all()), worst
    if bool(ok.any()) and n > 1:
        assert not torch.equal(out[ok], e0[ok]), "the update did nothing"
    # ema == p stays p, bit for bit (finite values)
    e.copy_(p)
    _update(e, p, W)
    torch.cuda.synchronize()
    assert torch.equal(_bits(e)[ok], _bits(p0)[ok]), "ema == p moved"
    _assert_guards(e_buf, elo, n, 7.0, "guard words of the average")


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("n", SMALL)
def test_update_within_the_derived_bound(dev, n, offset):
    _update_case(dev, n, offset, offset)
    _update_case(dev, n, (offset + 1 + n % 3) % 4, offset)            # another phase: float by float


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_update_wraps_the_grid_stride_loop(dev, offset):
    """One turn of the full grid plus 13 floats: the loop's second turn, a lone first quad of a pair and a tail."""
    n = _wrap_n()
    _update_case(dev, n, offset, offset)
    _update_case(dev, n, (offset + 2) % 4, offset)


@pytest.mark.parametrize("n", [1, 3, 5, 1023])
def test_update_nonfinite_stays_in_its_element(dev, n):
    """NaN, +inf and -inf in p: a non-finite average at exactly those elements, the bound everywhere else."""
    _update_case(dev, n, 1, 1, poison=True)
    _update_case(dev, n, 3, 2, poison=True)


def _swap_values(n, seed):
    """Raw words: random bit patterns (NaN payloads, denormals, infinities among them) with -0, +0 and two NaNs of different
    payload put in by hand."""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32)
    special = torch.tensor([-2 ** 31, 0x7FC00001, 0x7F800123, 0, 0xFFC12345 - 2 ** 32, 0x7F800000], dtype=torch.int64).to(torch.int32)
    k = min(n, special.numel())
    w[torch.randperm(n, generator=gen)[:k]] = special[:k]
    return w


def _swap_case(dev, n, a_off, b_off):
    wa, wb = _swap_values(n, 3 * n + 1), _swap_values(n, 3 * n + 2)
    a_buf, a, alo = _placed(dev, torch.zeros(n), a_off, 7.0)
    b_buf, b, blo = _placed(dev, torch.zeros(n), b_off, -3.0)
    a.view(torch.int32).copy_(wa)
    b.view(torch.int32).copy_(wb)
    _swap(a, b)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), wb) and torch.equal(_bits(b), wa), "swap"
    _swap(a, b)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), wa) and torch.equal(_bits(b), wb), "the second swap did not restore"
    _assert_guards(a_buf, alo, n, 7.0, "guard words of a")
    _assert_guards(b_buf, blo, n, -3.0, "guard words of b")


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("n", SMALL)
def test_swap_exchanges_raw_words(dev, n, offset):
    _swap_case(dev, n, offset, offset)
    _swap_case(dev, n, (offset + 1 + n % 3) % 4, offset)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_swap_wraps_the_grid_stride_loop(dev, offset):
    n = _wrap_n()
    _swap_case(dev, n, offset, offset)
    _swap_case(dev, n, (offset + 2) % 4, offset)


def test_swap_values_hold_what_they_claim():
    w = _swap_values(1023, 5)
    f = w.view(torch.float32)
    assert bool((w == -2 ** 31).any()) and bool((w == 0).any()) and int(torch.isnan(f).sum()) >= 2
    nan_words = w[torch.isnan(f)]
    assert nan_words.unique().numel() >= 2, "one NaN payload only"


def test_refusals_leave_memory_untouched(dev):
    """Overlap, a null pointer, n = 0, a pointer off the 4-byte grid and one_minus_decay in {0, 1, nan} (and beyond): the bad-
    argument error, and no word of either buffer changes."""
    from ctvae_amd import native
    base = torch.arange(64, dtype=torch.float32, device=dev) + 1
    before = base.clone()
    a, b = base[:16], base[32:48]

    def refused(name, *args):
        with pytest.raises(RuntimeError, match="bad argument"):
            native.call(name, *args)

    for w in (0.0, 1.0, float("nan"), float("inf"), -0.25, 1.5):
        refused("ctvae_ema_update", a.data_ptr(), b.data_ptr(), 16, w)
    refused("ctvae_ema_update", a.data_ptr(), base[8:24].data_ptr(), 16, 0.5)             # overlapping ranges
    refused("ctvae_ema_update", base[8:24].data_ptr(), a.data_ptr(), 16, 0.5)
    refused("ctvae_ema_update", a.data_ptr(), a.data_ptr(), 16, 0.5)
    refused("ctvae_ema_update", None, b.data_ptr(), 16, 0.5)
    refused("ctvae_ema_update", a.data_ptr(), None, 16, 0.5)
    refused("ctvae_ema_update", a.data_ptr(), b.data_ptr(), 0, 0.5)
    refused("ctvae_ema_update", a.data_ptr(), b.data_ptr(), -4, 0.5)
    refused("ctvae_ema_update", a.data_ptr() + 2, b.data_ptr(), 8, 0.5)
    refused("ctvae_buffer_swap", a.data_ptr(), base[8:24].data_ptr(), 16)
    refused("ctvae_buffer_swap", a.data_ptr(), a.data_ptr(), 16)
    refused("ctvae_buffer_swap", None, b.data_ptr(), 16)
    refused("ctvae_buffer_swap", a.data_ptr(), None, 16)
    refused("ctvae_buffer_swap", a.data_ptr(), b.data_ptr(), 0)
    refused("ctvae_buffer_swap", a.data_ptr(), b.data_ptr() + 1, 8)
    torch.cuda.synchronize()
    assert torch.equal(_bits(base), _bits(before))
    _update(a, b, 0.5)                              # (adjacent ranges are no overlap: the same calls go through when legal)
    _swap(base[:16], base[16:32])
    torch.cuda.synchronize()
    assert not torch.equal(base[:32], before[:32]) and torch.equal(base[32:], before[32:])


def test_python_wrappers_check_their_tensors(dev):
    from ctvae_amd import kernels as K
    a = torch.zeros(16, device=dev)
    with pytest.raises(ValueError):
        K.ema_update(a[:8], a[8:15], 0.5)
    with pytest.raises(ValueError):
        K.buffer_swap(a[:8], a[8:].double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.ema_update(torch.zeros(4), torch.zeros(4), 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.buffer_swap(torch.zeros(4), torch.zeros(4))
