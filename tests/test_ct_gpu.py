"""GPU: CTMCQVAE modes, the Gumbel straight-through kernel, the training harness (VAEXperiment + FlatAdam)
and the YAML runner."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from ctvae_amd import filler
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def build_ct(dev, seed, **over):
    from ctvae_amd.models import vae_models
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
    cfg.update(over)
    torch.manual_seed(seed)
    m = vae_models["CTMCQVAE"](**cfg)
    conv = filler.fill_state(H.mcq_specs(H.CT_CONV_CFG), seed + 1)
    m.load_state_dict(conv, strict=False)
    return m.to(dev).train()


def test_gumbel_st_kernel(dev):
    from ctvae_amd import kernels as K
    g = torch.Generator().manual_seed(4)
    p = torch.rand(3, 64, 64, generator=g)
    p[0, 0, :4] = torch.tensor([0.0, 1.0, 5e-5, 1 - 5e-5])
    noise = -torch.empty(3, 64, 64, 2).exponential_(generator=g).log()
    pr = p.clone().requires_grad_(True)
    logits = torch.stack([1 - pr, pr], dim=-1).clamp(min=1e-4).log()
    y_soft = ((logits + noise) / 1.0).softmax(-1)
    idx = y_soft.max(-1, keepdim=True)[1]
    y_hard = torch.zeros_like(logits).scatter_(-1, idx, 1.0)
    ref = (y_hard - y_soft.detach() + y_soft)[..., 1]
    w = torch.randn(3, 64, 64, generator=g)
    (ref * w).sum().backward()
    pd = p.to(dev).requires_grad_(True)
    out = K.GumbelBernoulliST.apply(pd, noise.to(dev))
    (out * w.to(dev)).sum().backward()
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=1e-6)
    np.testing.assert_allclose(pd.grad.cpu().numpy(), pr.grad.numpy(), atol=1e-4, rtol=1e-3)


def test_ct_conv_path_matches_golden(dev, golden):
    """skip_transition=True decodes compute_latents(latents, argmin indices): the conv/VQ/decoder path of CT must equal
    the MCQVAE(codebooks=1, beta=0.1) golden vectors whatever the causal layer does."""
    g = golden("ctconv_b2")
    seed = int(g["seed"])
    m = build_ct(dev, seed, skip_transition=True)
    x, _ = filler.synthetic_batch(seed, 2)
    out = m(x.to(dev), mode="base")
    assert len(out) == 5 and out[4]["mode"] == "base"
    np.testing.assert_allclose(out[0].detach().cpu().numpy(), g["recons"], atol=TOL, rtol=0)
    assert abs(out[2].item() - float(g["loss.VQ_Loss"])) <= TOL
    losses = m.loss_function(*out)
    assert abs(losses["Reconstruction_Loss"].item() - float(g["loss.Reconstruction_Loss"])) <= TOL
    assert set(losses) >= {"loss", "Reconstruction_Loss", "VQ_Loss", "CT_Loss", "ct_adjacency", "mode"}
    losses["loss"].backward()
    conv_grads = {k: p.grad for k, p in m.named_parameters() if not k.startswith("ct_layer.")}
    for k in ("decoder.10.0.weight", "decoder.3.resblock.2.weight", "encoder.0.0.weight", "vq_layer.quantizers.0.embedding.weight"):
        np.testing.assert_allclose(conv_grads[k].cpu().numpy(), g["grad." + k], atol=TOL, rtol=2e-3, err_msg=k)
    ct_g = [p.grad for k, p in m.named_parameters() if k.startswith("ct_layer.graph_discovers.0")]
    assert all(torch.isfinite(t).all() for t in ct_g) and sum(float(t.abs().sum()) for t in ct_g) > 0


@pytest.mark.parametrize("mode", ["base", "action", "causal"])
def test_ct_modes_run_and_backprop(dev, mode):
    m = build_ct(dev, 11)
    x, y, a = filler.synthetic_pairs(11, 3, 12)
    kw = {"mode": [mode] * 3}
    if mode != "base":
        kw.update(input_y=y.to(dev), action=a.to(dev))
    out = m(x.to(dev), **kw)
    losses = m.loss_function(*out)
    assert torch.isfinite(losses["loss"])
    m.zero_grad()
    losses["loss"].backward()
    assert torch.isfinite(m.flat_grads).all()
    sl = m.flat_range("ct_layer")
    assert float(m.flat_grads[sl].abs().sum()) > 0
    if mode == "causal":
        assert out[0].shape == (3, 12) and abs(float(out[0].sum()) - 3.0) < 1e-4      # action probabilities
    else:
        assert out[0].shape == (3, 3, 64, 64)
    if mode == "action":
        assert float(out[2]) == 0.0 and out[1].data_ptr() == kw["input_y"].data_ptr()   # vq_loss forced 0, recon vs y


def test_harness_three_adam_steps_match_reference(dev, golden):
    """VAEXperiment.training_step + FlatAdam on one batch for 3 steps: the loss trajectory recorded from the reference's
    modules with torch.optim.Adam (oracle/gen_golden.py) must be reproduced (H1 in SURVEY §8a)."""
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    g = golden("vanilla_b2")
    seed = int(g["seed"])
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
    m.load_state_dict(filler.fill_state(H.vanilla_specs(), seed + 1))
    m = m.to(dev).train()
    exp = VAEXperiment(m, {"LR": float(g["lr"]), "weight_decay": 0.0, "scheduler_gamma": 0.95, "kld_weight": float(g["M_N"])})
    x, eps = filler.synthetic_batch(seed, 2)
    xd, ed = x.to(dev), eps.to(dev)
    got = []
    for step in range(3):
        m.zero_grad()
        out = m(xd, eps=ed)
        l = m.loss_function(*out, M_N=exp.params["kld_weight"])
        l["loss"].backward()
        exp.optimizer_step()
        got.append(l["loss"].item())
    np.testing.assert_allclose(got, g["adam_losses"], rtol=2e-3, atol=1e-4)
    # (a) checksums of every parameter after 3 steps against the reference's (the fixture holds checksums only);
    for k, p in m.named_parameters():
        if k.endswith(".0.bias") and not k.startswith("final_layer.3"):
            continue        # conv bias in front of a BatchNorm: its gradient is rounding noise, Adam turns noise into +-lr steps
        H.assert_cks_close(H.cks(p), g["adam3." + k], rtol=5e-3, atol=6 * float(g["lr"]), what=k)
    # (b) FULL tensors against the oracle's own 3-step torch.optim.Adam trajectory (tests/test_oracle_golden.py pins that
    # trajectory to the same fixture).  Adam normalises each element's step to ~lr: an element whose gradient is within rounding
    # of zero may step +-lr either way on either side ("flip"), everything else must agree to a small fraction of one step.
    from oracle import vae_cpu as O
    lr = float(g["lr"])
    cur = O.leafify(filler.fill_state(H.vanilla_specs(), seed + 1))
    names = [k for k, v in cur.items() if v.requires_grad]
    opt = torch.optim.Adam([cur[k] for k in names], lr=lr)
    for step in range(3):
        opt.zero_grad()
        nb = {}
        r = O.vanilla_forward(cur, x, eps, True, nb)
        O.vanilla_loss(*r, exp.params["kld_weight"])["loss"].backward()
        opt.step()
        for k, v in nb.items():
            cur[k] = v
    # B = 2 through ten BatchNorm layers is ill-conditioned: an element that flips in step 1 perturbs every gradient of steps 2
    # and 3.  Measured on MI355X (CTVAE_ADAM_STATS=1 prints it): median deviation 0.001-0.01 lr, 90th percentile <= 0.06 lr,
    # 98th <= 0.15 lr, largest 2.8 lr.  Bounds per tensor: 90 % of the elements within 0.15 lr, 98 % within 0.6 lr, all within 4 lr
    # (three steps of +-lr can separate two trajectories by at most 6 lr).
    for k, p in m.named_parameters():
        if k.endswith(".0.bias") and not k.startswith("final_layer.3"):
            continue        # BatchNorm-cancelled conv bias (see (a))
        want, got_p = cur[k].detach(), p.detach().cpu()
        d = ((got_p - want).abs().flatten() / lr)[:1000000]
        q = torch.quantile(d, torch.tensor([0.5, 0.9, 0.98, 1.0]))
        if os.environ.get("CTVAE_ADAM_STATS"):
            print(k, [round(float(v), 4) for v in q])
        assert float(q[1]) <= 0.15 and float(q[2]) <= 0.6 and float(q[3]) <= 4.0, (k, [float(v) for v in q])
    exp.scheduler.step()
    assert abs(exp.optimizer.state[1].item() - float(g["lr"]) * 0.95) < 1e-9


def test_runner_consumes_yaml(dev, tmp_path):
    from ctvae_amd import run
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "mcq_vae.yaml")))
    cfg["logging_params"]["save_dir"] = str(tmp_path)
    cfg["data_params"]["train_batch_size"] = 8
    cfg["data_params"]["val_batch_size"] = 8
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    hist = run.main(["-c", str(p), "--steps-per-epoch", "3", "--max-epochs", "2"])
    assert len(hist) == 2 and "val_Reconstruction_Loss" in hist[-1] and hist[-1]["train_images"] == 24
    ck = torch.load(tmp_path / "MCQVAE" / "checkpoints" / "last.ckpt", weights_only=True)
    assert all(k.startswith("model.") for k in ck["state_dict"])
    assert ck["state_dict"]["model.encoder.0.0.weight"].shape == (64, 3, 4, 4)


def test_runner_full_resume_continues_bit_exactly(dev, tmp_path):
    """trainer_params.resume_from_checkpoint WITHOUT load_weights_only (run.py:85-101: Lightning restores optimizer, scheduler,
    epoch): 2 epochs in one run == 1 epoch, then a second process-like run resumed from last.ckpt for the second epoch --
    parameters, Adam moments / step / lr and the global step bit for bit (MCQVAE: no random draws in the step).  5 batches per
    epoch, so the straight run replays its captured step in epoch 2 where the resumed run starts eagerly again."""
    from ctvae_amd import run

    def cfg_for(sub, **trainer):
        cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "mcq_vae.yaml")))
        cfg["logging_params"]["save_dir"] = str(tmp_path / sub)
        cfg["data_params"]["train_batch_size"] = 8
        cfg["data_params"]["val_batch_size"] = 8
        cfg["trainer_params"].update(trainer)
        p = tmp_path / f"{sub}.yaml"
        p.write_text(yaml.safe_dump(cfg))
        return str(p)

    last = lambda sub: tmp_path / sub / "MCQVAE" / "checkpoints" / "last.ckpt"
    h2 = run.main(["-c", cfg_for("straight"), "--steps-per-epoch", "5", "--max-epochs", "2"])
    h1 = run.main(["-c", cfg_for("first"), "--steps-per-epoch", "5", "--max-epochs", "1"])
    hr = run.main(["-c", cfg_for("resumed", resume_from_checkpoint=str(last("first"))), "--steps-per-epoch", "5", "--max-epochs", "2"])
    assert [r["epoch"] for r in h2] == [0, 1] and [r["epoch"] for r in h1] == [0] and [r["epoch"] for r in hr] == [1]
    a = torch.load(last("straight"), weights_only=True)
    b = torch.load(last("resumed"), weights_only=True)
    assert a["epoch"] == b["epoch"] == 1 and a["global_step"] == b["global_step"] == 10
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    for k in ("exp_avg", "exp_avg_sq", "state"):
        assert torch.equal(a["trainer"]["optimizer"][k], b["trainer"]["optimizer"][k]), k
    assert a["trainer"]["optimizer"]["lr"] == b["trainer"]["optimizer"]["lr"] == pytest.approx(0.0005 * 0.98 ** 2)
    assert a["trainer"]["scheduler"] == b["trainer"]["scheduler"]
    assert float(a["trainer"]["optimizer"]["state"][0]) == 10.0
    assert hr[0]["val_Reconstruction_Loss"] == h2[1]["val_Reconstruction_Loss"]
    # a checkpoint without the trainer entry (e.g. the reference's weights) is refused loudly unless load_weights_only is set
    torch.save({"state_dict": a["state_dict"], "epoch": 1}, tmp_path / "weights.ckpt")
    with pytest.raises(SystemExit):
        run.main(["-c", cfg_for("bad", resume_from_checkpoint=str(tmp_path / "weights.ckpt")), "--steps-per-epoch", "2", "--max-epochs", "2"])
    hw = run.main(["-c", cfg_for("wo", resume_from_checkpoint=str(tmp_path / "weights.ckpt"), load_weights_only=True),
                   "--steps-per-epoch", "2", "--max-epochs", "1"])
    assert [r["epoch"] for r in hw] == [0]


@pytest.mark.parametrize("B,N,H", [(3, 64, 800), (2, 37, 70)])
def test_pair_mlp_kernel(dev, B, N, H):
    """ctvae_pair_mlp_forward/backward against the torch expression of CausalTransition._pair_coeffs
    (ct_mcq_vae.py:86-95 on all ordered pairs): values and all four gradients."""
    import torch.nn.functional as F
    from ctvae_amd import kernels as K
    g = torch.Generator().manual_seed(B * 1000 + N)
    u = (0.5 * torch.randn(B, N, H, generator=g)).requires_grad_(True)
    v = (0.5 * torch.randn(B, N, H, generator=g)).requires_grad_(True)
    w2 = (torch.randn(H, generator=g) / H ** 0.5).requires_grad_(True)
    b2 = torch.randn(1, generator=g).requires_grad_(True)
    h = F.leaky_relu(u.unsqueeze(2) + v.unsqueeze(1))
    ref = torch.sigmoid(F.linear(h, w2.view(1, -1), b2)).squeeze(-1)
    go = torch.randn(B, N, N, generator=g)
    ref.backward(go)
    ud, vd, wd, bd = (t.detach().to(dev).requires_grad_(True) for t in (u, v, w2, b2))
    out = K.PairMLP.apply(ud, vd, wd, bd)
    out.backward(go.to(dev))
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=2e-6, rtol=1e-5)
    for got, want in ((ud.grad, u.grad), (vd.grad, v.grad), (wd.grad, w2.grad), (bd.grad, b2.grad)):
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=1e-5 * max(1.0, float(want.abs().max())), rtol=1e-4)


@pytest.mark.parametrize("scale", [1e-4, 1.0, 3e3])
def test_clamp_kernels_hold_over_input_magnitudes(dev, scale):
    """relu / step of the N = 64 pair kernels and of the fused GATv2 layer are the VOP3P clamp of packed adds / fmas on operands
    scaled by 2^-64 / 2^60 (csrc/satmath.hpp): exact while |t| < 2^64 and, for the step, t > 2^-60.  Values and every gradient
    must keep matching the torch expressions when the pre-activations are 1e-4 .. 3e3 times their usual size (relative
    tolerances: the references are float32 torch ops themselves)."""
    import torch.nn.functional as F
    from ctvae_amd import kernels as K
    from ctvae_amd.models.causal import DenseGATv2
    g = torch.Generator().manual_seed(777)
    B, N, H = 2, 64, 96
    u = (scale * torch.randn(B, N, H, generator=g)).requires_grad_(True)
    v = (scale * torch.randn(B, N, H, generator=g)).requires_grad_(True)
    w2 = (torch.randn(H, generator=g) / (scale * H ** 0.5)).requires_grad_(True)
    b2 = torch.randn(1, generator=g).requires_grad_(True)
    ref = torch.sigmoid(F.linear(F.leaky_relu(u.unsqueeze(2) + v.unsqueeze(1)), w2.view(1, -1), b2)).squeeze(-1)
    go = torch.randn(B, N, N, generator=g)
    ref.backward(go)
    ud, vd, wd, bd = (t.detach().to(dev).requires_grad_(True) for t in (u, v, w2, b2))
    out = K.PairMLP.apply(ud, vd, wd, bd)
    out.backward(go.to(dev))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=3e-6, rtol=1e-5)
    for name, got, want in (("dU", ud.grad, u.grad), ("dV", vd.grad, v.grad), ("dw2", wd.grad, w2.grad), ("db2", bd.grad, b2.grad)):
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=2e-5 * float(want.abs().max()), rtol=2e-4, err_msg=name)
    # the fused layer on the 64 latent nodes against the head-by-head torch expression of the same module
    torch.manual_seed(778)
    layer = DenseGATv2(24, 32, 3)
    with torch.no_grad():
        layer.bias.uniform_(-0.1, 0.1)
        layer.lin_l.weight.mul_(scale)
        layer.lin_r.weight.mul_(scale)
        layer.lin_edge.weight.mul_(scale)
        layer.att.div_(scale)
    x = torch.randn(B, 64, 24, requires_grad=True)
    adj = (torch.rand(B, 64, 64) * (torch.rand(B, 64, 64) > 0.4)).requires_grad_(True)
    ref = layer(x, adj)
    go = torch.randn_like(ref)
    ref.backward(go)
    want = {k: p.grad.clone() for k, p in layer.named_parameters()}
    layer_d = DenseGATv2(24, 32, 3).to(dev)
    layer_d.load_state_dict(layer.state_dict())
    xd, ad = x.detach().to(dev).requires_grad_(True), adj.detach().to(dev).requires_grad_(True)
    assert layer_d.fused_ok(xd)
    out = layer_d.forward_fused(xd, ad)
    out.backward(go.to(dev))
    torch.cuda.synchronize()
    tol = lambda t: 3e-4 * max(1e-30, float(t.detach().abs().max()))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=tol(ref), rtol=1e-3)
    np.testing.assert_allclose(xd.grad.cpu().numpy(), x.grad.numpy(), atol=tol(x.grad), rtol=2e-3)
    np.testing.assert_allclose(ad.grad.cpu().numpy(), adj.grad.numpy(), atol=tol(adj.grad), rtol=2e-3)
    for k, p in layer_d.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), want[k].numpy(), atol=tol(want[k]), rtol=2e-3, err_msg=k)


@pytest.mark.parametrize("B,N,Hh,C", [(2, 65, 13, 100), (3, 65, 13, 64), (2, 9, 3, 20)])
def test_gat_score_kernel_and_layer(dev, B, N, Hh, C):
    """DenseGATv2.forward (the head-by-head torch expression of the GATv2Conv attention, ct_mcq_vae.py:103-114; torch ops on
    either device -- it no longer calls ctvae_gat_score) on the GPU against the same module on the CPU: the whole layer output
    and the gradients of x, adj and every parameter must agree."""
    from ctvae_amd.models.causal import DenseGATv2
    torch.manual_seed(50 + N + C)
    layer = DenseGATv2(24, C, Hh)
    with torch.no_grad():
        layer.bias.uniform_(-0.1, 0.1)
    x = torch.randn(B, N, 24, requires_grad=True)
    adj = (torch.rand(B, N, N) * (torch.rand(B, N, N) > 0.3)).requires_grad_(True)
    ref = layer(x, adj)                                    # CPU tensors -> torch path
    go = torch.randn_like(ref)
    ref.backward(go)
    want = {k: p.grad.clone() for k, p in layer.named_parameters()}
    gx, gadj = x.grad.clone(), adj.grad.clone()
    layer_d = DenseGATv2(24, C, Hh).to(dev)
    layer_d.load_state_dict(layer.state_dict())
    xd, ad = x.detach().to(dev).requires_grad_(True), adj.detach().to(dev).requires_grad_(True)
    out = layer_d(xd, ad)                                  # CUDA tensors -> the same torch ops on the device
    out.backward(go.to(dev))
    torch.cuda.synchronize()
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=2e-5, rtol=1e-4)
    np.testing.assert_allclose(xd.grad.cpu().numpy(), gx.numpy(), atol=1e-4 * max(1.0, float(gx.abs().max())), rtol=1e-3)
    np.testing.assert_allclose(ad.grad.cpu().numpy(), gadj.numpy(), atol=1e-4 * max(1.0, float(gadj.abs().max())), rtol=1e-3)
    for k, p in layer_d.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), want[k].numpy(), atol=1e-4 * max(1.0, float(want[k].abs().max())),
                                   rtol=1e-3, err_msg=k)


def test_pair_mlp_per_sample_scorers_and_compute_adj(dev):
    """per_sample mode of ctvae_pair_mlp_* (every sample scored by its own w2/b2) and the batched per-action
    discoverer evaluation built on it (CausalTransition._compute_adj) against the reference-shaped loop on the CPU."""
    import torch.nn.functional as F
    from ctvae_amd import kernels as K
    from ctvae_amd.models.causal import CausalTransition
    g = torch.Generator().manual_seed(77)
    B, N, Hd = 5, 64, 96
    u = (0.5 * torch.randn(B, N, Hd, generator=g)).requires_grad_(True)
    v = (0.5 * torch.randn(B, N, Hd, generator=g)).requires_grad_(True)
    w2 = (torch.randn(B, Hd, generator=g) / Hd ** 0.5).requires_grad_(True)
    b2 = torch.randn(B, generator=g).requires_grad_(True)
    h = F.leaky_relu(u.unsqueeze(2) + v.unsqueeze(1))
    ref = torch.sigmoid((h * w2[:, None, None, :]).sum(-1) + b2[:, None, None])
    go = torch.randn(B, N, N, generator=g)
    ref.backward(go)
    ud, vd, wd, bd = (t.detach().to(dev).requires_grad_(True) for t in (u, v, w2, b2))
    out = K.PairMLP.apply(ud, vd, wd, bd)
    out.backward(go.to(dev))
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().numpy(), atol=2e-6, rtol=1e-5)
    for got, want in ((ud.grad, u.grad), (vd.grad, v.grad), (wd.grad, w2.grad), (bd.grad, b2.grad)):
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=1e-5 * max(1.0, float(want.abs().max())), rtol=1e-4)

    # whole _compute_adj: CPU = one masked call per distinct action (reference structure), GPU = one batched launch
    torch.manual_seed(3)
    ct = CausalTransition(64, 12, [48, 10])
    lat = torch.rand(7, 64, 64)
    act = F.one_hot(torch.tensor([0, 3, 3, 11, 5, 0, 7]), 12).float()
    mask = (torch.rand(7, 64, 1) > 0.5).float()
    a_ref = ct._compute_adj(lat, act, mask)
    a_ref.sum().backward()
    want = {k: p.grad.clone() for k, p in ct.named_parameters() if p.grad is not None}
    ct_d = CausalTransition(64, 12, [48, 10]).to(dev)
    ct_d.load_state_dict(ct.state_dict())
    a_gpu = ct_d._compute_adj(lat.to(dev), act.to(dev), mask.to(dev))
    a_gpu.sum().backward()
    np.testing.assert_allclose(a_gpu.detach().cpu().numpy(), a_ref.detach().numpy(), atol=2e-6, rtol=1e-5)
    for k, p in ct_d.named_parameters():
        if k in want:
            np.testing.assert_allclose(p.grad.cpu().numpy(), want[k].numpy(), atol=1e-5 * max(1.0, float(want[k].abs().max())),
                                       rtol=1e-3, err_msg=k)


class _FixedNoise:
    """Noise source with one cached device tensor per (tag, shape): deterministic and free of host-to-device copies once every
    tag has been drawn (so a captured step replays the same noise an eager step sees)."""

    def __init__(self, dev):
        self.dev, self.cache = dev, {}

    def draw(self, tag, shape, p=0.0):
        key = (tag, tuple(shape), p)
        if key not in self.cache:
            self.cache[key] = filler.ct_noise(77, tag, len(self.cache) % 5, shape, p).to(self.dev)
        return self.cache[key]


def test_harness_captures_ct_modes_as_hipgraphs(dev):
    """VAEXperiment.fit on transition batches: every CT-MCQ-VAE mode (one per batch, datasets/transition.py:128-190) is captured
    into its own hipGraph after three eager steps, and the parameter trajectory is bit-identical to the all-eager harness."""
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import causal
    B, A = 4, 12
    batches = []
    for i in range(18):
        x, y, a = filler.synthetic_pairs(100 + i, B, A)
        mode = ["base", "action", "causal"][i % 3]
        opts = {"mode": [mode] * B}
        if mode != "base":
            opts.update(input_y=y.to(dev), action=a.to(dev))
        batches.append((x.to(dev), torch.zeros(B, device=dev), opts))
    params = {"LR": 5e-4, "weight_decay": 0.0, "scheduler_gamma": 0.99, "kld_weight": 0.00025, "update_parameters": "ct_layer"}
    finals = {}
    prev = causal.set_noise_source(_FixedNoise(dev))
    try:
        for graphed in (False, True):
            m = build_ct(dev, 5)
            exp = VAEXperiment(m, dict(params, hipgraph=graphed))
            hist = exp.fit(lambda: iter(batches), None, max_epochs=1)
            torch.cuda.synchronize()
            assert hist[0]["train_images"] == 18 * B and exp.global_step == 18
            if graphed:
                assert len(exp._graphed) == 3 and all(g.graph is not None and g.seen == 6 for g in exp._graphed.values())
            else:
                assert not exp._graphed
            finals[graphed] = m.flat_params.clone()
    finally:
        causal.set_noise_source(prev)
    assert torch.isfinite(finals[True]).all()
    assert torch.equal(finals[True], finals[False]), float((finals[True] - finals[False]).abs().max())
