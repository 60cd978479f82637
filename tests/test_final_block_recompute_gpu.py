"""GPU: the final block's backward without the tensor g_a between its two convolutions.

final_layer = ConvTranspose2d(32->32, s2) + BatchNorm2d + LeakyReLU + Conv2d(32->3) + Tanh (vanilla_vae.py:64-75).  Its backward
used to write g_a [B,2H,2W,32] (the picture-side conv's data gradient, image.hip img_bwd_fused_kernel) and read it back once
(upconv.hip up_wgrad_kernel, BatchNorm backward applied on load).  Now the picture-side kernel skips the store
(ctvae_conv_backward_nodx) and the transposed conv's weight-gradient kernel forms g_a again per tile from the 3-channel
gradient (ctvae_conv_backward_recompute / ctvae_conv_wgrad_recompute).

Every case drives the block's backward twice on identical inputs -- the two-tensor path and the new one -- and asserts
  * bitwise equality of g_y, dW1, db1, dW2, db2, d gamma, d beta and g_x (same dot products, same summation order), and
  * both against one float64 CPU reference of the block (torch conv_transpose2d / batch_norm / conv2d autograd) with the bound
    tests/test_bench_sizes_gpu.py uses for this model: absolute 1e-4 scaled by max(1, max|reference|), rtol 2e-3.
Shapes: one tile whose whole halo is outside the image; 2 x 2 tiles per image; 516 tiles on the 512-workgroup persistent grid.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
TOL = 1e-4          # tests/test_bench_sizes_gpu.py TOL / _assert_grads
NAMES = ("g_y", "dW1", "db1", "dW2", "db2", "dgamma", "dbeta", "g_x")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _slope(K, act):
    return {K.ACT_NONE: 1.0, K.ACT_LRELU: 0.01, K.ACT_RELU: 0.0}[act]


def _make(dev, B, H, W, seed, bn_act_name="lrelu", lazy_in=False):
    """Parameters and inputs of one case (seeded normal; g_pre has no zero anywhere, so none on a border pixel)."""
    from ctvae_amd import kernels as K
    from ctvae_amd.models.packing import PackedBN, PackedConv
    g = torch.Generator().manual_seed(seed)
    up, bn, conv = PackedConv(32, 32, 3, transposed=True, bias=True), PackedBN(32), PackedConv(32, 3, 3, bias=True)
    with torch.no_grad():
        for p, s in ((up.weight, 0.08), (up.bias, 0.1), (conv.weight, 0.08), (conv.bias, 0.1)):
            p.copy_(torch.randn(p.shape, generator=g) * s)
        bn.weight.copy_(1.0 + 0.2 * torch.randn(32, generator=g))
        bn.bias.copy_(0.2 * torch.randn(32, generator=g))
    x = torch.randn(B, H, W, 32, generator=g)
    # per-pixel magnitude P^-1/2 (P = B*2H*2W pixels): every reduced gradient (a sum over P pixels) is then O(1), the scale at which
    # the absolute bound bites, and the float32 rounding of a P-term sum whose exact value is 0 (db1: the gradient behind a
    # train-mode BatchNorm sums to zero per channel) stays a rounding error of O(1) terms, not of O(sqrt(P)) ones
    g_pre = torch.randn(B, 2 * H, 2 * W, 3, generator=g) / float(B * 2 * H * 2 * W) ** 0.5
    g_pre = torch.where(g_pre == 0, torch.ones_like(g_pre), g_pre)
    in_coef = None
    if lazy_in:   # the previous block's BatchNorm scale | shift [2][32], applied on load with LeakyReLU
        in_coef = torch.cat([1.0 + 0.3 * torch.randn(32, generator=g), 0.3 * torch.randn(32, generator=g)])
    case = dict(B=B, H=H, W=W, up=up.to(dev), bn=bn.to(dev), conv=conv.to(dev), x=x.to(dev), g_pre=g_pre.to(dev),
                in_coef=None if in_coef is None else in_coef.to(dev), in_act=K.ACT_LRELU if lazy_in else K.ACT_NONE,
                bn_act={"lrelu": K.ACT_LRELU, "none": K.ACT_NONE}[bn_act_name],
                spec1=K.ConvSpec(K.CONVT, 32, 32, 3, 2, 1, 1, K.ACT_NONE), spec2=K.ConvSpec(K.CONV, 32, 3, 3, 1, 1, 0, K.ACT_TANH))
    return case


def _gpu_backward(c, new):
    """The backward of ConvBNActConvAct's lazy form through the raw entry points: g_a written and read (new=False) or never made."""
    from ctvae_amd import kernels as K
    up, bn, conv = c["up"], c["bn"], c["conv"]
    params = (up.weight, up.bias, bn.weight, bn.bias, conv.weight, conv.bias)
    for p in params:
        p.grad = None
    x, g_pre, bn_act, spec1, spec2 = c["x"], c["g_pre"], c["bn_act"], c["spec1"], c["spec2"]
    lazy_in = (c["in_coef"], c["in_act"]) if c["in_coef"] is not None else None
    with torch.no_grad():
        y1, _, coef, mean, invstd = K._conv_bn_act_forward(x, params[:4], (bn.running_mean, bn.running_var, bn.num_batches_tracked),
                                                           True, spec1, bn_act, lazy_in, want_a=False, want_coef=True)
        link = K.BNLink(y1, mean, invstd, bn.weight, bn.bias, bn_act)
        grads = K._grad_targets(bn.weight, bn.bias)
        g_y = torch.full_like(y1, float("nan"))
        kw = dict(in_coef=c["in_coef"], in_act=c["in_act"])
        if new:
            assert K.conv_recompute_supported(spec1, spec2, c["B"], c["H"], c["W"])
            c7 = K.conv_backward_nodx_raw(y1, g_pre, conv.weight, conv.bias, spec2, link, coef, bn_act, grads)
            assert c7 is not None
            g_x = K.conv_backward_raw(x, g_pre, up.weight, up.bias, spec1, dy_bn=(y1, c7, bn_act, g_y), recompute=(conv.weight, spec2), **kw)
        else:
            g_a = K.conv_backward_raw(y1, g_pre, conv.weight, conv.bias, spec2, link=link, in_coef=coef, in_act=bn_act, bn_commit=grads)
            _, _, c7 = link.take(g_a)
            assert c7 is not None
            g_x = K.conv_backward_raw(x, g_a, up.weight, up.bias, spec1, dy_bn=(y1, c7, bn_act, g_y), **kw)
        torch.cuda.synchronize()
    out = (g_y, up.weight.grad, up.bias.grad, conv.weight.grad, conv.bias.grad, bn.weight.grad, bn.bias.grad, g_x)
    return dict(zip(NAMES, (t.detach().clone() for t in out)))


def _reference(c):
    """float64 CPU autograd of the same block; tensors in the layouts _gpu_backward returns (NHWC activations)."""
    from ctvae_amd import kernels as K
    d = torch.float64
    up, bn, conv = c["up"], c["bn"], c["conv"]
    w1, b1, gm, bt, w2, b2 = (p.detach().cpu().to(d).contiguous().requires_grad_(True)
                              for p in (up.weight, up.bias, bn.weight, bn.bias, conv.weight, conv.bias))
    xin = c["x"].cpu().to(d).permute(0, 3, 1, 2)
    if c["in_coef"] is not None:
        co = c["in_coef"].cpu().to(d)
        t = xin * co[:32].view(1, -1, 1, 1) + co[32:].view(1, -1, 1, 1)
        xin = torch.maximum(t, t * _slope(K, c["in_act"]))
    xin = xin.contiguous().requires_grad_(True)
    y = F.conv_transpose2d(xin, w1, b1, stride=2, padding=1, output_padding=1)
    y.retain_grad()
    t = F.batch_norm(y, None, None, gm, bt, True, 0.1, K.BN_EPS)
    a = torch.maximum(t, t * _slope(K, c["bn_act"])) if c["bn_act"] != K.ACT_NONE else t
    pre = F.conv2d(a, w2, b2, padding=1)
    pre.backward(c["g_pre"].cpu().to(d).permute(0, 3, 1, 2))
    out = (y.grad.permute(0, 2, 3, 1), w1.grad, b1.grad, w2.grad, b2.grad, gm.grad, bt.grad, xin.grad.permute(0, 2, 3, 1))
    return dict(zip(NAMES, out))


def _check(c):
    old, new, ref = _gpu_backward(c, False), _gpu_backward(c, True), _reference(c)
    for k in NAMES:
        r = ref[k].numpy()
        tol = TOL * max(1.0, float(np.abs(r).max()))
        for tag, got in (("two-tensor", old[k]), ("recompute", new[k])):
            e = float(np.abs(got.cpu().double().numpy() - r).max())
            print(f"{k} {tag}: max abs err {e:.3e} (bound {tol:.3e} + 2e-3 rel, max|ref| {float(np.abs(r).max()):.3e})")
    for k in NAMES:
        assert torch.equal(old[k], new[k]), f"{k}: recompute path differs from the two-tensor path"
    for k in NAMES:
        r = ref[k].numpy()
        tol = TOL * max(1.0, float(np.abs(r).max()))
        np.testing.assert_allclose(new[k].cpu().numpy(), r, atol=tol, rtol=2e-3, err_msg=k)
        np.testing.assert_allclose(old[k].cpu().numpy(), r, atol=tol, rtol=2e-3, err_msg=k)


@pytest.mark.parametrize("B,H,W", [(1, 8, 32), (3, 16, 64), (129, 32, 32)])
def test_recompute_matches_two_tensor_path_and_float64(dev, B, H, W):
    """One tile with every halo pixel outside the image; 2 x 2 tiles per image; 516 tiles on 512 persistent workgroups."""
    _check(_make(dev, B, H, W, seed=4100 + B))


def test_recompute_with_lazy_input_transform(dev):
    """The previous block's BatchNorm + LeakyReLU applied on load (in_scale / in_shift) next to the recompute."""
    _check(_make(dev, 3, 16, 64, seed=4201, lazy_in=True))


@pytest.mark.parametrize("bn_act_name", ["lrelu", "none"])
def test_recompute_bn_activation(dev, bn_act_name):
    """LeakyReLU and identity as the BatchNorm's activation."""
    _check(_make(dev, 2, 8, 64, seed=4301, bn_act_name=bn_act_name))


def _node_backward(dev, B, H, W):
    """ConvBNActConvAct forward + backward under the launch log; returns the report."""
    from ctvae_amd import kernels as K
    from ctvae_amd import native
    c = _make(dev, B, H, W, seed=4400 + H)
    up, bn, conv = c["up"], c["bn"], c["conv"]
    x = c["x"].clone().requires_grad_(True)
    native.prof_enable(True)
    r = K.ConvBNActConvAct.apply(x, up.weight, up.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                 conv.weight, conv.bias, True, c["spec1"], c["spec2"], K.ACT_LRELU)
    r.backward(c["g_pre"].reshape(r.shape) if r.shape == c["g_pre"].shape else c["g_pre"].permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    native.prof_enable(False)
    assert all(bool(torch.isfinite(p.grad).all()) for p in (up.weight, up.bias, bn.weight, bn.bias, conv.weight, conv.bias))
    assert bool(torch.isfinite(x.grad).all())
    return native.prof_report()


def test_unsupported_geometry_takes_the_old_path(dev):
    """Host side: the query says no for a 32 -> 3 conv with k != 3 and for H not a multiple of 8, and ConvBNActConvAct then runs
    the old launches -- the picture-side kernel's logged bytes include the g_a store (y read + g_a written: 2 x 32 channels)."""
    from ctvae_amd import kernels as K
    spec1 = K.ConvSpec(K.CONVT, 32, 32, 3, 2, 1, 1, K.ACT_NONE)
    assert K.conv_recompute_supported(spec1, K.ConvSpec(K.CONV, 32, 3, 3, 1, 1, 0, K.ACT_TANH), 2, 8, 32)
    assert not K.conv_recompute_supported(spec1, K.ConvSpec(K.CONV, 32, 3, 5, 1, 2, 0, K.ACT_TANH), 2, 8, 32)
    assert not K.conv_recompute_supported(spec1, K.ConvSpec(K.CONV, 32, 3, 3, 1, 1, 0, K.ACT_TANH), 2, 4, 32)
    px = lambda B, H, W: B * 2 * H * 2 * W
    rep = _node_backward(dev, 2, 4, 32)          # H % 8 != 0: the transposed conv runs its generic kernels
    assert "up_wgrad_kernel" not in rep, sorted(rep)
    assert rep["img_bwd_fused_kernel"]["bytes"] == 4.0 * px(2, 4, 32) * (2 * 32 + 3), rep["img_bwd_fused_kernel"]
    rep = _node_backward(dev, 2, 8, 32)          # supported: no g_a store, and the weight-gradient kernel reads the 3-channel gradient
    assert rep["img_bwd_fused_kernel"]["bytes"] == 4.0 * px(2, 8, 32) * (32 + 3), rep["img_bwd_fused_kernel"]
    assert rep["up_wgrad_kernel"]["count"] == 1 and rep["up_wgrad_kernel"]["bytes"] == 4.0 * 2 * 8 * 32 * (9 * 32 + 12), rep["up_wgrad_kernel"]
