"""GPU: the gradient-accumulation kernels alone (csrc/gradaccum.hip) -- ctvae_grad_accumulate in its three modes against
torch's own fp32 ``a + b`` bit for bit, on the smallest shapes where the kernel can go wrong, and ctvae_adam_flags_window
against numpy.

fp32 addition is correctly rounded, so the comparison is exact (int32 views: +0 / -0 and NaN count as what they are).  The
inputs carry +-0, denormals, +-inf and NaN.  Every buffer has guard words in front of and behind the range; they, and the
accumulator in "finish" mode, must come back untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 8                      # floats on either side of a range
SPECIALS = [0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -5.877e-39, float("inf"), float("-inf"), float("nan"), 1.0, -1.0,
            3.4028235e38, -3.4028235e38]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _values(n, seed):
    """n fp32 values: normal draws over many magnitudes with the special values strewn in (every one of them at least once
    when n allows, and meeting each other across the three vectors of a case)."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=gen) * torch.pow(10.0, torch.randint(-30, 30, (n,), generator=gen).float())
    sp = torch.tensor(SPECIALS, dtype=torch.float32)
    where = torch.randperm(n, generator=gen)[:max(1, min(n, max(len(SPECIALS), n // 16)))]
    v[where] = sp[torch.randint(0, len(SPECIALS), (len(where),), generator=gen)]
    return v


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


def _wrap_n():
    from ctvae_amd import native
    return int(native.load().ctvae_grad_accumulate_pass_floats()) + 1027


def _case(dev, n, acc_off, g_off):
    from ctvae_amd import kernels as K
    g0, g1, g2 = (_values(n, 10 * n + s) for s in range(3))
    sp = torch.tensor(SPECIALS, dtype=torch.float32)
    m = min(n, len(SPECIALS) ** 2)                    # the head of the range: every special value meets every other one
    g0[:m] = sp.repeat_interleave(len(SPECIALS))[:m]
    g1[:m] = sp.repeat(len(SPECIALS))[:m]
    g2[:m] = -0.0                                     # x + -0 = x, also for x = -0
    acc_buf, acc, alo = _placed(dev, torch.zeros(n), acc_off, 7.0)
    g_buf, g, glo = _placed(dev, g0, g_off, -3.0)
    d0, d1, d2 = g0.to(dev), g1.to(dev), g2.to(dev)
    want1 = d0 + d1                                   # torch's fp32 add, the same operand order
    want2 = want1 + d2
    K.grad_accumulate(acc, g, "store")
    assert torch.equal(_bits(acc), _bits(d0)), "store"
    assert torch.equal(_bits(g), _bits(d0)), "store changed the gradients"
    g.copy_(d1)
    K.grad_accumulate(acc, g, "add")
    assert torch.equal(_bits(acc), _bits(want1)), "add"
    assert torch.equal(_bits(g), _bits(d1)), "add changed the gradients"
    g.copy_(d2)
    K.grad_accumulate(acc, g, "finish")
    torch.cuda.synchronize()
    assert torch.equal(_bits(g), _bits(want2)), "finish"
    assert torch.equal(_bits(acc), _bits(want1)), "finish changed the accumulator"
    _assert_guards(acc_buf, alo, n, 7.0, "guard words of the accumulator")
    _assert_guards(g_buf, glo, n, -3.0, "guard words of the gradient buffer")
    return want2


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1024, 1027])
def test_accumulate_modes_bit_equal_torch(dev, n, offset):
    """Slice start ``offset`` floats behind a 16-byte boundary, accumulator at the same phase (what FlatAdam allocates): the
    scalar head, the 16-byte loop and the scalar tail."""
    _case(dev, n, offset, offset)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_accumulate_wraps_the_grid_stride_loop(dev, offset):
    """One turn of the full grid plus 1027 floats: the loop's second turn, a lone first quad of a pair and a 3-float tail."""
    n = _wrap_n()
    assert n % 4 == 3
    _case(dev, n, offset, offset)


@pytest.mark.parametrize("n", [5, 1027])
@pytest.mark.parametrize("acc_off,g_off", [(0, 1), (2, 0), (3, 1)])
def test_accumulate_with_different_phases_runs_float_by_float(dev, n, acc_off, g_off):
    """Accumulator and gradients at different offsets from a 16-byte boundary: no 16-byte access is possible on both."""
    _case(dev, n, acc_off, g_off)


def test_special_values_meet(dev):
    """The inputs do exercise what they claim: the expected sums contain NaN, both infinities, denormals and both zeros."""
    want = _case(dev, 1027, 0, 0).cpu()
    bits = want.view(torch.int32)
    assert bool(torch.isnan(want).any()) and bool((want == float("inf")).any()) and bool((want == float("-inf")).any())
    assert bool((bits == 0).any()) and bool((bits == -2 ** 31).any())
    absw = want.abs()
    assert bool(((absw > 0) & (absw < 1.1754944e-38)).any()), "no denormal survived into a sum"


def test_accumulate_refuses_bad_arguments(dev):
    from ctvae_amd import kernels as K
    a = torch.zeros(16, device=dev)
    with pytest.raises(KeyError):
        K.grad_accumulate(a[:8], a[8:], "sum")
    with pytest.raises(ValueError):
        K.grad_accumulate(a[:8], a[8:15], "add")
    with pytest.raises(RuntimeError, match="bad argument"):
        K.grad_accumulate(a[:8], a[4:12], "add")                  # overlapping ranges
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.grad_accumulate(torch.zeros(4), torch.zeros(4), "add")


def test_accumulator_like_follows_the_slice_phase(dev):
    from ctvae_amd import kernels as K
    base = torch.zeros(64, device=dev)
    for off in range(4):
        g = base[off:off + 21]
        acc = K.grad_accumulator_like(g)
        assert acc.numel() == 21 and acc.data_ptr() % 16 == g.data_ptr() % 16 and not bool(acc.any())


@pytest.mark.parametrize("nb", [1, 63, 64, 65, 300])
def test_flag_window_modes_match_numpy(dev, nb):
    from ctvae_amd import kernels as K
    rng = np.random.default_rng(nb)
    table = K.AdamBlockTable([(4 * b, 4 * b + 3) for b in range(nb)], [-1] * nb, 4 * nb, 0, dev)
    # guard words around the window's flags; table.active is the table's own tensor
    wbuf = torch.full((nb + 2 * GUARD,), 5, dtype=torch.int32, device=dev)
    window = wbuf[GUARD:GUARD + nb]
    acts = [rng.integers(0, 2, nb).astype(np.int32) for _ in range(3)]
    acts[1][rng.integers(0, nb)] = 3                      # any non-zero word counts; MAX keeps it
    table.active.copy_(torch.from_numpy(acts[0]))
    K.adam_flags_window(window, table, "store")
    assert np.array_equal(window.cpu().numpy(), acts[0]) and np.array_equal(table.active.cpu().numpy(), acts[0])
    table.active.copy_(torch.from_numpy(acts[1]))
    K.adam_flags_window(window, table, "add")
    want = np.maximum(acts[0], acts[1])
    assert np.array_equal(window.cpu().numpy(), want) and np.array_equal(table.active.cpu().numpy(), acts[1])
    table.active.copy_(torch.from_numpy(acts[2]))
    K.adam_flags_window(window, table, "finish")
    torch.cuda.synchronize()
    assert np.array_equal(table.active.cpu().numpy(), np.maximum(want, acts[2]))
    assert np.array_equal(window.cpu().numpy(), want), "finish changed the window's flags"
    guards = wbuf.cpu().numpy()
    assert (guards[:GUARD] == 5).all() and (guards[GUARD + nb:] == 5).all()
    with pytest.raises(ValueError):
        K.adam_flags_window(window[:-1] if nb > 1 else wbuf, table, "add")
