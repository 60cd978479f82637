"""GPU: csrc/klfloor.hip through ``kernels.FreeBitsKL`` (``ctvae_freebits_kl_forward_grad``) against the float64 restatement of
tests/kl_checks.py.

Shapes: one row; L not a multiple of 4; the headline shape (one workgroup, one launch); ragged last tiles in both directions with
two workgroups and the finishing launch; and the largest L.  Bounds: those of tests/test_ops_gpu.py::test_reparam_and_loss
(kl_checks.VALUE_RTOL / GRAD_ATOL / GRAD_RTOL).  The floored count is exact and the floored columns' gradients are 0.0 bit for bit."""
import numpy as np
import pytest
import torch

from tests import kl_checks as C

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4), (3, 10), (64, 128), (257, 200), (2, 1024)]
FLOORS = (0.0, 0.05, 0.5)
WEIGHTS = ((0.37, 1.0), (1.0, 4.0))            # (device weight, scale)


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import kernels
    from ctvae_amd import native
    native.load()
    return kernels


def _device_inputs(B, L, sliced):
    """(mu, log_var) leaves on the device: column slices of one [B, 2L] tensor, or two contiguous tensors."""
    mu, lv = C.make_inputs(B, L)
    dev = torch.device("cuda")
    if sliced:
        heads = torch.cat([mu, lv], dim=1).to(dev).requires_grad_(True)
        return heads, heads[:, :L], heads[:, L:]
    md, ld = mu.to(dev).requires_grad_(True), lv.to(dev).requires_grad_(True)
    return (md, ld), md, ld


def _grads(leaf, L):
    if isinstance(leaf, tuple):
        return leaf[0].grad, leaf[1].grad
    return leaf.grad[:, :L], leaf.grad[:, L:]


def _run(K, B, L, sliced, weight, scale, lam, w_dev=None):
    leaf, md, ld = _device_inputs(B, L, sliced)
    if w_dev is None:
        w_dev = torch.full((1,), weight, dtype=torch.float32, device="cuda")
    out = K.FreeBitsKL.apply(md, ld, w_dev, scale, lam)
    K.backward(out[0])
    torch.cuda.synchronize()
    g_mu, g_lv = _grads(leaf, L)
    return [o.detach().clone() for o in out], g_mu.detach().clone(), g_lv.detach().clone()


def _close(got, want, what):
    print(f"  {what}: got {got!r} want {want!r}")
    assert abs(got - want) <= C.VALUE_RTOL * abs(want), what


@pytest.mark.parametrize("sliced", [True, False], ids=["slices", "contiguous"])
@pytest.mark.parametrize("B,L", SHAPES)
def test_op_against_float64(K, B, L, sliced):
    mu, lv = C.make_inputs(B, L)
    for lam in FLOORS:
        for weight, scale in WEIGHTS:
            print(f"B {B} L {L} lambda {lam} weight {weight} scale {scale}")
            ref = C.reference(mu, lv, weight, scale, lam)
            out, g_mu, g_lv = _run(K, B, L, sliced, weight, scale, lam)
            assert len(out) == 4 and all(o.dim() == 0 for o in out)
            assert float(out[3]) == ref["out"][3]
            for i, name in enumerate(("w * sum f", "sum m", "sum f")):
                _close(float(out[i]), ref["out"][i], name)
            floored = ~ref["active"]
            if lam > 0.0:
                assert int(floored.sum()) == (L + 1) // 2
                zeros = torch.zeros(B, int(floored.sum()), dtype=torch.int32)
                assert torch.equal(g_mu.cpu()[:, floored].contiguous().view(torch.int32), zeros), "floored g_mu is not +0.0"
                assert torch.equal(g_lv.cpu()[:, floored].contiguous().view(torch.int32), zeros), "floored g_lv is not +0.0"
            else:
                assert not bool(floored.any())
            np.testing.assert_allclose(g_mu.cpu().numpy(), ref["g_mu"].numpy(), atol=C.GRAD_ATOL, rtol=C.GRAD_RTOL)
            np.testing.assert_allclose(g_lv.cpu().numpy(), ref["g_lv"].numpy(), atol=C.GRAD_ATOL, rtol=C.GRAD_RTOL)


@pytest.mark.parametrize("B,L", SHAPES)
def test_no_floor_equals_the_loss_kernels(K, B, L):
    """lambda = 0: the value and the gradients of the existing ``VAELoss`` path with the same M_N (reconstruction operands of four
    zeros, as ``GaussKL`` calls it)."""
    weight, scale = 0.37, 1.0
    out, g_mu, g_lv = _run(K, B, L, True, weight, scale, 0.0)
    leaf, md, ld = _device_inputs(B, L, True)
    z4 = torch.zeros(4, device="cuda")
    old = K.VAELoss.apply(z4.clone().requires_grad_(True), z4, md, ld, None, weight * scale)
    K.backward(old[0])
    torch.cuda.synchronize()
    o_mu, o_lv = _grads(leaf, L)
    _close(float(out[0]), float(old[0].detach()), "loss")
    _close(float(out[1]), float(old[2]), "kld")
    assert float(out[2]) == float(out[1]) and float(out[3]) == 0.0
    np.testing.assert_allclose(g_mu.cpu().numpy(), o_mu.cpu().numpy(), atol=C.GRAD_ATOL, rtol=C.GRAD_RTOL)
    np.testing.assert_allclose(g_lv.cpu().numpy(), o_lv.cpu().numpy(), atol=C.GRAD_ATOL, rtol=C.GRAD_RTOL)


@pytest.mark.parametrize("B,L", [(64, 128), (257, 200)])
def test_repeatable_and_the_weight_is_read_from_the_device(K, B, L):
    w_dev = torch.full((1,), 0.37, dtype=torch.float32, device="cuda")
    a = _run(K, B, L, True, None, 1.0, 0.05, w_dev=w_dev)
    b = _run(K, B, L, True, None, 1.0, 0.05, w_dev=w_dev)
    for x, y in zip(a[0] + [a[1], a[2]], b[0] + [b[1], b[2]]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), "the same call gave other bits"
    w_dev.fill_(0.11)                                            # in place: the same address
    c = _run(K, B, L, True, None, 1.0, 0.05, w_dev=w_dev)
    assert float(c[0][0]) != float(a[0][0])
    for i in (1, 2, 3):
        assert torch.equal(c[0][i].view(torch.int32), a[0][i].view(torch.int32)), i
    assert not torch.equal(c[1], a[1]) and not torch.equal(c[2], a[2])
    mu, lv = C.make_inputs(B, L)
    ref = C.reference(mu, lv, 0.11, 1.0, 0.05)
    _close(float(c[0][0]), ref["out"][0], "w * sum f at the new weight")
    np.testing.assert_allclose(c[1].cpu().numpy(), ref["g_mu"].numpy(), atol=C.GRAD_ATOL, rtol=C.GRAD_RTOL)


def test_an_upstream_gradient_scales_the_precomputed_ones(K):
    """The rare path of ``backward``: the term is not the root of the pass."""
    B, L = 3, 10
    mu, lv = C.make_inputs(B, L)
    leaf, md, ld = _device_inputs(B, L, False)
    w_dev = torch.full((1,), 0.37, dtype=torch.float32, device="cuda")
    out = K.FreeBitsKL.apply(md, ld, w_dev, 1.0, 0.05)
    (out[0] * 2.0).backward()
    ref = C.reference(mu, lv, 0.37, 1.0, 0.05)
    np.testing.assert_allclose(leaf[0].grad.cpu().numpy(), 2.0 * ref["g_mu"].numpy(), atol=C.GRAD_ATOL, rtol=C.GRAD_RTOL)
    np.testing.assert_allclose(leaf[1].grad.cpu().numpy(), 2.0 * ref["g_lv"].numpy(), atol=C.GRAD_ATOL, rtol=C.GRAD_RTOL)
    assert not any(o.requires_grad for o in out[1:])


def test_nan_stays_visible_and_no_grad_writes_no_gradients(K):
    mu, lv = C.make_inputs(3, 10)
    mu[1, 0] = float("nan")                                      # a collapsed column: under the floor if it were finite
    w_dev = torch.full((1,), 0.37, dtype=torch.float32, device="cuda")
    with torch.no_grad():
        out = K.FreeBitsKL.apply(mu.cuda(), lv.cuda(), w_dev, 1.0, 0.05)
    assert float(out[3]) == 4.0                                  # the other four collapsed columns
    assert all(float(out[i]) != float(out[i]) for i in (0, 1, 2)), "the NaN column was floored away"


def test_refusals(K):
    from ctvae_amd import native
    w_dev = torch.full((1,), 1.0, dtype=torch.float32, device="cuda")
    z = torch.zeros(2, 8, device="cuda")
    with pytest.raises(RuntimeError, match="1 <= L <= 1024"):
        K.FreeBitsKL.apply(torch.zeros(1, 1025, device="cuda"), torch.zeros(1, 1025, device="cuda"), w_dev, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="one shape"):
        K.FreeBitsKL.apply(z, torch.zeros(2, 9, device="cuda"), w_dev, 1.0, 0.0)
    with pytest.raises(RuntimeError, match="one fp32 element"):
        K.FreeBitsKL.apply(z, z, torch.zeros(2, device="cuda"), 1.0, 0.0)
    with pytest.raises(RuntimeError, match="bad argument"):      # the library's own check: a negative floor launches nothing
        K.FreeBitsKL.apply(z, z, w_dev, 1.0, -1.0)
    assert native.load().ctvae_freebits_workspace_bytes(128) == 0 and native.load().ctvae_freebits_workspace_bytes(129) == 129 * 12
