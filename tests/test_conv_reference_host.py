"""CPU: the float64 references, the geometry port, the kernel-selection mirror, the exactness margins and the bounds of
tests/conv_checks.py, which tests/test_conv_ops_gpu.py holds ctvae_conv_forward / ctvae_conv_dgrad against.

Per case: the reference equals torch's float64 conv2d / conv_transpose2d plus the epilogue expressions (the data gradient:
torch's float64 autograd); the geometry port agrees with tests/host_emul/geom_emul.cpp (kinds 0..3, the refusals included); the
mirror predicts the kernel the case names in `expect`; the int regime's margin holds; float32 evaluations of the same sums in
three orders stay inside the randn bound; no tensor of a case is larger than 128 MB.  Run with -s to see, per case, the mirror's
prediction, the margin, the bound and the time of the reference."""
import ctypes
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import conv_checks as C
from tests import wgrad_checks as V

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_emul", "geom_emul.cpp")
SO = os.path.join(HERE, "host_emul", "_geom_emul.so")
EMUL_MAX_MACS = 3e8                     # the emulation is a naive loop nest: the large cases are left to the torch comparison
_REF = {}


def ref_of(c, regime):
    key = (c.id, regime)
    if key not in _REF:
        inp = C.make_inputs(c, regime)
        _REF[key] = (inp, C.reference(c, regime, inp))
    return _REF[key]


@pytest.fixture(scope="module")
def emul():
    hdr = os.path.join(os.path.dirname(HERE), "ct-vae_amd", "csrc", "geom.hpp")
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", SO, SRC])
    lib = ctypes.CDLL(SO)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.emul_tapgemm.argtypes = [ctypes.c_int, fp, fp, fp] + [ctypes.c_int] * 9
    return lib


def fptr(t):
    return ctypes.cast(t.data_ptr(), ctypes.POINTER(ctypes.c_float))


def gkind(c):
    return (0 if c.op == "fwd" else 2) + (0 if (c.kind & ~C.W_CI_TAP) == C.CONV else 1)


def torch_weight(c, W):
    """The library's weight block -> the torch parameter of the layer, float64."""
    W = W.double()
    if c.kind & C.W_CI_TAP:             # [Ci][tap][Co]: nn.Linear over torch.flatten(NCHW), read as a k x k convolution
        return W.view(c.Ci, c.k, c.k, c.Co).permute(3, 0, 1, 2).contiguous()
    W = W.view(c.k, c.k, c.Ci, c.Co)
    return (W.permute(2, 3, 0, 1) if (c.kind & ~C.W_CI_TAP) == C.CONVT else W.permute(3, 2, 0, 1)).contiguous()


def torch_layer(c, x, w):
    if (c.kind & ~C.W_CI_TAP) == C.CONVT:
        return F.conv_transpose2d(x, w, None, stride=c.s, padding=c.p, output_padding=c.opad)
    return F.conv2d(x, w, None, stride=c.s, padding=c.p)


def torch_reference(c, regime, inp):
    """pre-bias sum, pre and out from torch's own float64 ops; the epilogue written out once more, independently."""
    act, _, maska = c.acts(regime)
    w = torch_weight(c, inp["W"])
    G = inp["G"].double()
    if inp["xf"] is not None:
        sc, sh, a = inp["xf"]
        t = G * sc.double() + sh.double()
        G = t if a == C.ACT_NONE else torch.where(t > 0, t, t * (C.LEAKY if a == C.ACT_LRELU else 0.0))
    if c.op == "fwd":
        s = torch_layer(c, G.permute(0, 3, 1, 2), w).permute(0, 2, 3, 1)
    else:
        x = torch.zeros(c.B, c.Ci, c.H, c.W, dtype=torch.float64, requires_grad=True)
        torch_layer(c, x, w).backward(G.permute(0, 3, 1, 2))
        s = x.grad.permute(0, 2, 3, 1)
    pre = s
    if inp["bias"] is not None:
        pre = pre + inp["bias"].double()
    if inp["add"] is not None:
        pre = pre + inp["add"].double()
    if act == C.ACT_TANH:
        out = torch.tanh(pre)
    else:
        out = torch.where(pre > 0, pre, pre * {C.ACT_NONE: 1.0, C.ACT_LRELU: C.LEAKY, C.ACT_RELU: 0.0}[act])
    if inp["mask"] is not None:
        m = inp["mask"].double()
        out = out * (1 - m * m if maska == C.ACT_TANH else torch.where(m > 0, 1.0, {C.ACT_LRELU: C.LEAKY, C.ACT_RELU: 0.0}[maska]))
    return s, pre, out


def close(a, b, what):
    scale = max(1.0, float(b.abs().max()))
    err = float((a - b).abs().max())
    assert a.shape == b.shape and err <= 1e-11 * scale, f"{what}: {err:.3e} (scale {scale:.3e})"


@pytest.mark.parametrize("c", C.RUN_CASES, ids=lambda c: c.id)
def test_reference_matches_torch_float64(c):
    for regime in c.regimes:
        inp, ref = ref_of(c, regime)
        s, pre, out = torch_reference(c, regime, inp)
        close(ref["sum"], s, f"{c.id}/{regime}/sum")
        close(ref["pre"], pre, f"{c.id}/{regime}/pre")
        close(ref["out"], out, f"{c.id}/{regime}/out")
        print(f"{c.id}/{regime}: reference {ref['seconds']:.2f} s")


@pytest.mark.parametrize("c", C.ALL_CASES, ids=lambda c: c.id)
def test_geometry_port_matches_host_emulation(emul, c):
    """build_geom() kinds 0..3 against csrc/geom.hpp itself: the same refusals, and on integer data the same sums bit for bit."""
    g = c.geom()
    args = c.args()[1:]
    flag = 0x100 if c.kind & C.W_CI_TAP else 0
    if g is None:
        one = torch.zeros(1 << 16)
        assert emul.emul_tapgemm(gkind(c) | flag, fptr(one), fptr(one), fptr(one), *args) == -1
        return
    if gkind(c) < 2 and not flag:       # kinds 0 / 1: the port the weight-gradient suite already pins
        v = V.build_geom(c.kind, *args)
        assert (v.gH, v.gW, v.gC, v.sH, v.sW, v.sC, v.Qh, v.Qw, v.is_, v.os, v.py, v.px, v.taps) == \
               (g.gH, g.gW, g.gC, g.sH, g.sW, g.sC, g.Qh, g.Qw, g.is_, g.os, g.py, g.px, g.taps)
    assert g.wT == (0 if c.op == "fwd" else 1) and all(len(t) <= 16 for t in g.taps)
    macs = g.Mc * g.sC * sum(g.ntaps) * g.gC
    if macs > EMUL_MAX_MACS:            # its geometry kind and tap pattern are covered by the smaller cases
        return
    inp = C.make_inputs(c, "int")
    out = torch.full((g.B, g.sH, g.sW, g.sC), float("nan"))
    G, W = inp["G"].contiguous(), inp["W"].contiguous()
    assert emul.emul_tapgemm(gkind(c) | flag, fptr(G), fptr(W), fptr(out), *args) == 0
    want = C.gather_gemm(g, G.double(), C.wmat(g, W))
    assert torch.equal(out.double(), want)


def test_geometry_refusals():
    """sH % s, k*k > 16 on the conv-like kinds, more than 16 taps per class on the others, k*k > 64, a bad stride."""
    assert C.build_geom(2, 2, 15, 16, 8, 8, 3, 2, 1, 0) is None and C.build_geom(2, 2, 16, 15, 8, 8, 3, 2, 1, 0) is None
    assert C.build_geom(2, 2, 16, 16, 8, 8, 3, 2, 1, 0) is not None
    assert C.build_geom(0, 2, 16, 16, 8, 8, 5, 1, 2, 0) is None and C.build_geom(3, 2, 16, 16, 8, 8, 5, 1, 2, 0) is None
    assert C.build_geom(1, 2, 8, 8, 8, 8, 5, 1, 2, 0) is None            # 25 taps in the one class
    assert C.build_geom(1, 2, 8, 8, 8, 8, 5, 2, 2, 1) is not None        # at stride 2 at most 9 per class
    assert C.build_geom(1, 2, 8, 8, 8, 8, 9, 2, 4, 1) is None            # k*k > 64
    assert C.build_geom(0, 2, 8, 8, 8, 8, 3, 3, 1, 0) is None


@pytest.mark.parametrize("c", C.ALL_CASES, ids=lambda c: c.id)
def test_mirror_predicts_the_expected_kernel(c):
    sel = C.select(c)
    print(f"{c.id}: rc {sel.rc} {sel.labels} sk={sel.sk} cls_rot={sel.cls_rot} L={sel.L}  ({c.hits})")
    assert sel.rc == c.rc
    if c.rc:
        assert sel.labels == []
        return
    assert sel.labels == sorted(c.expect)
    if c.sk is not None:
        assert sel.sk == c.sk
    assert C.max_tensor_bytes(c) <= C.MAX_TENSOR_BYTES


def test_mirror_edges():
    """What the case list relies on without naming it in `expect`."""
    by = C.case_by_id
    assert C.select(by("tt-k3-clsrot")).cls_rot == 1 and C.select(by("d-s2-k4")).cls_rot == 1 and C.select(by("tt-k3-3x5")).cls_rot == 0
    assert C.tapgemm_plan(by("ft-up-add").geom(), C.WS_BYTES // 4).BM == 0          # the fall-through picks its tile without the plan
    assert C.tapgemm_plan(by("t-128x64").geom(), C.WS_BYTES // 4).BM == 128
    g = by("t-pf0").geom()
    assert ceil(g.Mc, 64) * ceil(g.sC, 64) > 1024
    # Winograd's floor of 64 workgroups and the switch to the 64 x 64 workgroups at 200
    assert C.wino_supported(by("w-fs-b16").geom(), C.WS_BYTES // 4) and not C.wino_supported(by("w-b15-direct").geom(), C.WS_BYTES // 4)
    assert [C.wino_block(by(i).geom())[2] for i in ("w-h4-b250", "w-h8-b62", "w-full-b50", "w-fs-b16")] == [16, 4, 1, 1]
    # the transform on load: refused where ctvae_conv_input_transform_supported says 0
    assert C.input_transform_supported(by("t-xf-lrelu"), False) and C.input_transform_supported(by("up-xf"), False)
    assert C.input_transform_supported(by("img-xf"), False) and C.input_transform_supported(by("thin-64-upimg-xf"), False)
    assert not C.input_transform_supported(by("enc-1tile"), False) and not C.input_transform_supported(by("w-fs-b16"), True)
    assert C.input_transform_supported(by("w-fs-b16"), False)
    # ctvae_conv_forward_lazy_slices
    assert [C.lazy_slices(c) for c, _ in C.LAZY_CASES] == [n for _, n in C.LAZY_CASES]
    assert all(C.lazy_slices(by(i), wino_on=by(i).wino) == 0 for i in C.LAZY_REFUSED)
    assert [C.linear_pixmajor_supported(B, Ci, Cc, P, ws) for B, Ci, Cc, P, ws, _ in C.PIXMAJOR] == [ok for *_, ok in C.PIXMAJOR]
    # the Winograd filter hand-over exists only where forward and data gradient both run Winograd
    assert C.wino_filter_floats(by("w-fs-b16"), True) == 16 * 64 * 64 and C.wino_filter_floats(by("t-64-128-sk4"), True) == 0
    assert C.select(by("w-fs-b16"), filters_out=True).labels == ["wino_conv_fs_kernel", "wino_weight2_kernel"]
    assert C.select(by("w-fs-b16"), filters_ready=True).labels == ["wino_conv_fs_kernel"]
    assert C.select(by("t-64-128-sk4"), filters_out=True).rc == C.ERR_BAD_ARG


def ceil(a, b):
    return -(-a // b)


@pytest.mark.parametrize("c", [c for c in C.RUN_CASES if "int" in c.regimes], ids=lambda c: c.id)
def test_int_regime_is_exact(c):
    inp, ref = ref_of(c, "int")
    sel = C.select(c)
    m = C.int_exact_margin(c, sel, ref, inp)
    print(f"{c.id}: int margin {m:.5f}")
    assert m < 1.0
    # integers in, integers out: the reference itself is free of rounding
    assert torch.equal(ref["out"], ref["out"].round()) and float(ref["out"].abs().max()) < 2 ** 24
    if sel.family == "wino":
        g = c.geom()
        assert torch.equal(C.wino_forward(g, inp["G"].double(), C.wmat(g, inp["W"])), ref["sum"])


@pytest.mark.parametrize("c", C.RUN_CASES, ids=lambda c: c.id)
def test_float32_orders_stay_inside_the_randn_bound(c):
    inp, ref = ref_of(c, "randn")
    sel = C.select(c)
    bnd = C.bounds(c, sel, ref, inp)
    worst = 0.0
    for order in ("taps", "reversed", "slices"):
        got = C.emulate32(c, sel, order, inp).double()
        worst = max(worst, float(((got - ref["pre"]).abs() / bnd["pre"]).max()))
    print(f"{c.id}: L = {bnd['L']}, median bound {float(bnd['out'].median()):.3e}, float32 orders: max err/bound = {worst:.4f}")
    assert worst < 1.0
    assert bool((bnd["out"] > 0).all()) and bool(torch.isfinite(bnd["out"]).all())
    if sel.family == "wino":            # the identity the absolute pipeline is taken from
        g = c.geom()
        w = C.wino_forward(g, inp["G"].double(), C.wmat(g, inp["W"]))
        close(w, ref["sum"], f"{c.id}/winograd identity")
        assert bool((C.wino_forward(g, inp["G"].double(), C.wmat(g, inp["W"]), absolute=True) >= ref["sum"].abs() * (1 - 1e-12)).all())


def test_pixmajor_and_lazy_references():
    """out_pix: column c*P + p of the Linear goes to pixel p, channel c; the lazy forward's slices sum to the pre-bias sum."""
    B, Ci, Cc, P = 3, 32, 8, 4
    gen = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(B, Ci, generator=gen), torch.randn(Ci, Cc * P, generator=gen), torch.randn(Cc * P, generator=gen)
    y = F.linear(x.double(), w.double().t(), b.double()).view(B, Cc, 2, 2)                  # .view(B, C, h, w): NCHW
    # not torch.equal: F.linear adds the bias inside the GEMM, the reference behind it, and whether the two float64 results agree to
    # the last bit depends on the host's BLAS path.  A wrong column-to-pixel map is off by O(1), not by 1e-12.
    want = y.permute(0, 2, 3, 1).reshape(B, P, Cc)
    assert float((C.pixmajor_ref(x, w, b, Cc, P) - want).abs().max()) <= 1e-12 * float(want.abs().max())
