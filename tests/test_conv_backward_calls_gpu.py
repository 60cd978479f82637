"""GPU: a paired backward call's result depends on its arguments only.

The five ctvae_conv_backward* entry points share one implementation, and three of them select a mode of it (no data
gradient tensor, dy formed in the kernel, data gradient left as split-K slices).  Whatever call came before -- a refused one, or
a valid one in another mode -- the same arguments must give the same bits and the same launches.

Shapes: the small-batch layers of test_pair_narrow_gpu.py (k 3, stride 2, pad 1).  The paired data gradient of the transposed
conv splits K there; that of Conv 32 -> 64 never does (the shortest parity class of its data gradient reduces over 2 chunks of
32, the plan wants 8), so Conv 128 -> 256 on 8 x 8 stands beside it for the calls that need slices.
"""
import pytest
import torch

from tests.test_ops_gpu import as_param, pack

pytestmark = pytest.mark.gpu

CASES = [
    # transposed, Ci, Co, H, B, paired data gradient splits K
    (False, 32, 64, 32, 5, False),
    (True, 64, 32, 16, 3, True),
    (False, 128, 256, 8, 5, True),
]
IDS = ["conv32-64", "convT64-32", "conv128-256"]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import kernels
    from ctvae_amd import native
    native.load()
    return kernels


class Layer:
    """Device operands of one case, and the three kinds of call made with them."""

    def __init__(self, K, case):
        from ctvae_amd import native
        self.K, self.N = K, native
        self.transposed, self.Ci, self.Co, self.H, self.B, self.split = case
        t = self.transposed
        g = torch.Generator().manual_seed(self.Ci * 31 + self.Co + self.B)
        self.spec = K.ConvSpec(K.CONVT if t else K.CONV, self.Ci, self.Co, 3, 2, 1, 1 if t else 0, K.ACT_NONE)
        ho, wo = self.spec.out_hw(self.H, self.H)
        self.x = torch.randn(self.B, self.H, self.H, self.Ci, generator=g).cuda()
        self.dy = torch.randn(self.B, ho, wo, self.Co, generator=g).cuda()
        self.w = pack(torch.randn((self.Ci, self.Co, 3, 3) if t else (self.Co, self.Ci, 3, 3), generator=g) * 0.05, t).cuda()
        self.geom = self.spec.geom(self.B, self.H, self.H)
        self.ws = native.workspace(self.x.device)

    def slices(self, for_bn):
        return self.N.load().ctvae_conv_backward_lazy_slices(*self.geom, for_bn, self.ws.numel() * 4)

    def logged(self, fn):
        """(fn(), {kernel name: launches}) of the launches fn makes."""
        self.N.prof_report()
        self.N.prof_enable(True)
        try:
            out = fn()
            torch.cuda.synchronize()
        finally:
            self.N.prof_enable(False)
        return out, {k: v["count"] for k, v in self.N.prof_report().items()}

    def plain(self):
        """K.conv_backward_raw on fresh parameters: ((dx, dw, db), launches)."""
        wp = as_param(self.w, self.transposed)
        bp = torch.nn.Parameter(torch.zeros(self.Co).cuda())
        dx, rep = self.logged(lambda: self.K.conv_backward_raw(self.x, self.dy, wp, bp, self.spec))
        return (dx, wp.grad, bp.grad), rep

    def lazy(self, pixel_major, x=True):
        """ctvae_conv_backward_lazy into fresh buffers: ((slices, dw, db), launches)."""
        n = self.slices(0 if pixel_major else 1)
        P = self.N.ptr
        sl = torch.zeros(max(n, 1) * self.x.numel()).cuda()
        dw, db = torch.zeros_like(self.w), torch.zeros(self.Co).cuda()
        _, rep = self.logged(lambda: self.N.call(
            "ctvae_conv_backward_lazy", self.geom[0], P(self.x) if x else None, P(self.dy), P(self.w), P(dw), P(db), P(sl),
            *self.geom[1:], 0, None, None, 0, pixel_major, P(self.ws), self.ws.numel() * 4))
        return (sl, dw, db), rep

    def nodx(self):
        """ctvae_conv_backward_nodx without a BatchNorm rider: planned like any paired call, then refused -- only the picture-side
        conv's fused kernel can do without the data gradient tensor."""
        P = self.N.ptr
        dw, db = torch.zeros_like(self.w), torch.zeros(self.Co).cuda()
        return self.logged(lambda: self.N.call(
            "ctvae_conv_backward_nodx", self.geom[0], P(self.x), P(self.dy), P(self.w), P(dw), P(db), *self.geom[1:], 0,
            None, None, None, None, None, 0, None, 0, None, None, None, 0, None, None, 0, P(self.ws), self.ws.numel() * 4))

    def recompute(self):
        """ctvae_conv_backward_recompute naming a 3 x 3 picture-side conv behind this layer, which only the 32 -> 32 transposed
        conv of the final block has."""
        conv2 = (self.K.CONV, 3, 3, 1, 1, 0)
        assert self.N.load().ctvae_conv_recompute_supported(*self.geom, *conv2) == 0
        P = self.N.ptr
        dw, db, dx = torch.zeros_like(self.w), torch.zeros(self.Co).cuda(), torch.zeros_like(self.x)
        g_pre, w2 = torch.zeros(self.dy.numel() // self.Co * 3).cuda(), torch.zeros(9 * self.Co * 3).cuda()
        coef, gy = torch.zeros(7 * self.Co).cuda(), torch.zeros_like(self.dy)
        return self.logged(lambda: self.N.call(
            "ctvae_conv_backward_recompute", self.geom[0], P(self.x), P(g_pre), P(w2), P(self.w), P(dw), P(db), P(dx),
            *self.geom[1:], 0, None, None, None, None, None, 0, None, 0, None, None, None, 0, None, None, 0,
            P(self.dy), P(coef), self.K.ACT_LRELU, P(gy), *conv2, P(self.ws), self.ws.numel() * 4))


def same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_data_gradient_splits_where_the_cases_say(K, case):
    L = Layer(K, case)
    for for_bn in (0, 1):
        assert (L.slices(for_bn) > 1) == L.split, (for_bn, L.slices(for_bn))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_state_after_a_refusal(K, case):
    L = Layer(K, case)
    base, base_rep = L.plain()
    assert base_rep, "the plain call launched nothing"
    for refused in (lambda: L.lazy(1, x=False), L.nodx, L.recompute):
        with pytest.raises(RuntimeError, match="code -22"):
            refused()
        assert L.N.prof_report() == {}          # refused before any launch
        again, rep = L.plain()
        assert same(again, base)
        assert rep == base_rep


@pytest.mark.parametrize("case", [c for c in CASES if c[5]], ids=[i for i, c in zip(IDS, CASES) if c[5]])
def test_calls_do_not_depend_on_their_order(K, case):
    L = Layer(K, case)
    assert L.slices(0) > 1 and L.slices(1) > 1
    calls = {"lazy pixel-major": lambda: L.lazy(1), "lazy channel-major": lambda: L.lazy(0), "plain": L.plain}
    first = {}
    for name in ("lazy pixel-major", "lazy channel-major", "plain"):
        first[name] = calls[name]()
    assert not torch.equal(first["lazy pixel-major"][0][0], first["lazy channel-major"][0][0])    # two layouts, not one
    for name in ("plain", "lazy channel-major", "lazy pixel-major", "plain", "lazy pixel-major", "lazy channel-major"):
        out, rep = calls[name]()
        assert same(out, first[name][0]), name
        assert rep == first[name][1], name
