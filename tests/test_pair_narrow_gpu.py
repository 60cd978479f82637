"""GPU: the paired backward launch (ctvae_conv_backward, conv_bwd_pair_kernel) for the layers with a 32-wide side.

VanillaVAE has two: encoder.1 (Conv 32 -> 64, stride 2: its data gradient has 32 output channels -> 128 x 32 tiles on the
data-gradient role) and decoder.3 (ConvTranspose 64 -> 32, stride 2: 128 x 32 tiles of dW on the weight-gradient role).  Both
read their X operand through the previous block's lazy BatchNorm + LeakyReLU (in_coef).  The paired call is checked against
the separate ctvae_conv_wgrad / ctvae_conv_dgrad calls (weight and bias gradients bit-identical: same kernel bodies, same
slices) and against torch in float64; the launch log of a bs = 64 step shows that neither layer runs its GEMMs stand-alone.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_ops_gpu import as_param, pack

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import kernels
    from ctvae_amd import native
    native.load()
    return kernels


@pytest.mark.parametrize("case", [
    # transposed, Ci, Co, H, B        (k 3, stride 2, pad 1; output padding 1 for the transposed conv)
    (False, 32, 64, 32, 64),          # encoder.1 at the bench batch: 128 x 32 data-gradient tiles
    (True, 64, 32, 16, 64),           # decoder.3 at the bench batch: 128 x 32 weight-gradient tiles
    (False, 32, 64, 32, 5),           # small batch: the data gradient is split over K slices
    (True, 64, 32, 16, 3),
])
@pytest.mark.parametrize("lazy", [True, False])
def test_narrow_pair_matches_separate_launches_and_torch(K, case, lazy):
    transposed, Ci, Co, H, B = case
    g = torch.Generator().manual_seed(Ci * 31 + Co + B)
    spec = K.ConvSpec(K.CONVT if transposed else K.CONV, Ci, Co, 3, 2, 1, 1 if transposed else 0, K.ACT_NONE)
    ho, wo = spec.out_hw(H, H)
    y = torch.randn(B, H, H, Ci, generator=g)                 # raw BatchNorm input of the previous block (NHWC)
    scale, shift = 0.5 + torch.rand(Ci, generator=g), 0.3 * torch.randn(Ci, generator=g)
    x = F.leaky_relu(y * scale + shift, 0.01) if lazy else y
    dy = torch.randn(B, ho, wo, Co, generator=g)
    w = torch.randn((Ci, Co, 3, 3) if transposed else (Co, Ci, 3, 3), generator=g) * 0.05
    coef = torch.cat([scale, shift]).cuda() if lazy else None
    act = K.ACT_LRELU if lazy else K.ACT_NONE

    res = []
    for paired in (True, False):
        wp = as_param(pack(w, transposed).cuda(), transposed)
        bp = torch.nn.Parameter(torch.zeros(Co).cuda())
        yd, dyd = y.cuda(), dy.cuda()
        if paired:
            dx = K.conv_backward_raw(yd, dyd, wp, bp, spec, in_coef=coef, in_act=act)
        else:
            K.conv_wgrad_raw(yd, dyd, wp, bp, spec, in_coef=coef, in_act=act)
            dx = K.conv_dgrad_raw(dyd, wp, spec, (H, H))
        torch.cuda.synchronize()
        res.append((dx.cpu(), wp.grad.cpu(), bp.grad.cpu()))
    assert torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2])
    np.testing.assert_allclose(res[0][0].numpy(), res[1][0].numpy(), rtol=2e-5, atol=2e-5 * float(res[1][0].abs().max()))

    xr = x.permute(0, 3, 1, 2).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = torch.zeros(Co, dtype=torch.float64, requires_grad=True)
    out = (F.conv_transpose2d(xr, wr, br, stride=2, padding=1, output_padding=1) if transposed
           else F.conv2d(xr, wr, br, stride=2, padding=1))
    out.backward(dy.permute(0, 3, 1, 2).double())
    for got, ref in ((res[0][0], xr.grad.permute(0, 2, 3, 1)), (res[0][1], wr.grad), (res[0][2], br.grad)):
        ref = ref.float().numpy()
        np.testing.assert_allclose(got.numpy(), ref, rtol=1e-4, atol=1e-4 * max(1.0, float(np.abs(ref).max())))


def test_vanilla_bs64_step_pairs_its_narrow_layers(K):
    """One VanillaVAE training step at the bench batch: ten paired launches, no stand-alone 128 x 32 weight gradient, and the
    only stand-alone 128 x 32 data gradient left is final_layer.0's (its weight gradient is the picture-side up_wgrad kernel)."""
    from ctvae_amd import filler, native
    from ctvae_amd.models import vae_models
    from tests import helpers as H
    seed, B = 1265, 64
    sd = filler.fill_state(H.vanilla_specs(), seed + 1)
    x, eps = filler.synthetic_batch(seed, B)
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
    m.load_state_dict(sd)
    m = m.to("cuda").train()
    native.prof_enable(True)
    out = m(x.cuda(), eps=eps.cuda())
    m.loss_function(*out, M_N=0.00025)["loss"].backward()
    torch.cuda.synchronize()
    native.prof_enable(False)
    rep = native.prof_report()
    assert not any(k.startswith("wgrad_kernel<4,1") for k in rep), sorted(rep)
    assert rep["tapgemm_fast_kernel<4,1,1,1,true,3>"]["count"] == 1, rep
    assert rep["conv_bwd_pair_kernel"]["count"] == 10, rep
