"""GPU: the HIP models behind the reference API against (a) the golden vectors produced by the reference's
own modules and (b) the CPU oracle on the same seeded inputs.  Everything goes through the C ABI."""
import numpy as np
import pytest
import torch

from ctvae_amd import filler
from tests import helpers as H

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import native
    native.load()
    return torch.device("cuda")


def build_vanilla(dev, seed):
    from ctvae_amd.models import vae_models
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
    m.load_state_dict(filler.fill_state(H.vanilla_specs(), seed + 1))
    return m.to(dev).train()


def build_mcq(dev, cfg, seed):
    from ctvae_amd.models import vae_models
    m = vae_models["MCQVAE"](**{**cfg, "hidden_dims": list(cfg["hidden_dims"])})
    m.load_state_dict(filler.fill_state(H.mcq_specs(cfg), seed + 1))
    return m.to(dev).train()


@pytest.mark.parametrize("B", [2, 4])
def test_vanilla_vs_golden(dev, golden, B):
    g = golden(f"vanilla_b{B}")
    seed = int(g["seed"])
    m = build_vanilla(dev, seed)
    x, eps = filler.synthetic_batch(seed, B)
    xd = x.to(dev)
    out = m(xd, eps=eps.to(dev))
    losses = m.loss_function(*out, M_N=float(g["M_N"]))
    losses["loss"].backward()
    torch.cuda.synchronize()
    recons, _, mu, log_var = out
    assert recons.shape == (B, 3, 64, 64)
    np.testing.assert_allclose(mu.detach().cpu().numpy(), g["mu"], atol=TOL, rtol=0)
    np.testing.assert_allclose(log_var.detach().cpu().numpy(), g["log_var"], atol=TOL, rtol=0)
    r = recons.detach().cpu()
    if B <= 2:
        np.testing.assert_allclose(r.numpy(), g["recons"], atol=TOL, rtol=0)
    else:
        np.testing.assert_allclose(r[:, :, ::4, ::4].numpy(), g["recons_strided"], atol=TOL, rtol=0)
    for k in ("loss", "Reconstruction_Loss", "KLD"):
        assert abs(losses[k].item() - float(g["loss." + k])) <= TOL * max(1.0, abs(float(g["loss." + k]))), k
    sd_grads = {k: p.grad for k, p in m.named_parameters()}
    for k, gr in sd_grads.items():
        H.assert_cks_close(H.cks(gr), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    for k in ("fc_mu.bias", "encoder.0.0.weight", "final_layer.3.weight", "decoder.3.1.weight", "encoder.4.1.bias"):
        np.testing.assert_allclose(sd_grads[k].cpu().numpy(), g["grad." + k], atol=TOL, rtol=2e-3)
    for k, b in m.named_buffers():
        np.testing.assert_allclose(b.cpu().numpy(), g["buf1." + k], atol=1e-5, rtol=1e-4)


def _placeholder_paths_are_live(m, B, dev):
    """The library's own plan for VanillaVAE(3, 128) at batch B: all three never-written placeholders are in play (B = 4 is the
    smallest such batch) -- heads (forward slices for GaussianLatent), the data gradients of decoder.0 and decoder_input
    (pixel-major slices for LinearToNHWC / GaussianLatent), the data gradient of the heads (channel-major, for encoder.4's BatchNorm)."""
    from ctvae_amd import kernels as K
    from ctvae_amd import native
    lib, ws = native.load(), native.workspace(dev).numel() * 4
    heads = K.ConvSpec(K.CONV_FLAT, 512, 2 * m.latent_dim, 2, 2, 0).geom(B, 2, 2)
    assert lib.ctvae_conv_forward_lazy_slices(*heads, ws) == 16
    assert lib.ctvae_conv_backward_lazy_slices(*m.decoder[0].spec.geom(B, 2, 2), 0, ws) == 16
    assert lib.ctvae_conv_backward_lazy_slices(*m._dec_in_spec.geom(B, 1, 1), 0, ws) == 16
    assert lib.ctvae_conv_backward_lazy_slices(*heads, 1, ws) == 2


def _vanilla_step_by_hand(m, xd, eps, second_consumer=False):
    """VanillaVAE.forward + loss + kernels.backward spelled out; second_consumer: z is also read by the loss directly."""
    from ctvae_amd import kernels as K
    m.zero_grad()
    heads, fwd_slices = m._encode_heads(xd, for_latent_node=True)
    mu, log_var, z = K.GaussianLatent.apply(heads, eps, None, fwd_slices)
    K.grad_slices_ok(z)
    recons = m.decode(z)
    loss = m.loss_function(recons, xd, mu, log_var, M_N=0.00025)["loss"]
    K.backward(loss + z.sum() if second_consumer else loss)
    torch.cuda.synchronize()
    return loss.detach().clone(), recons.detach().clone()


def test_vanilla_second_consumer_of_z_raises_and_leaves_nothing_behind(dev):
    """z is promised to decode alone (grad_slices_ok): decoder_input leaves its data gradient as slices behind a placeholder that is
    never written.  With a second consumer autograd hands GaussianLatent placeholder + the other gradient -- at another address, so
    nobody claims the slices: kernels.backward raises after the pass (every launch has completed; the kernels only read allocated
    memory).  The next ordinary step of the same model equals a fresh model's, bit for bit."""
    from ctvae_amd import kernels as K
    B, seed = 4, 41
    x, eps = filler.synthetic_batch(seed, B)
    xd, eps = x.to(dev), eps.to(dev)
    m, fresh = build_vanilla(dev, seed), build_vanilla(dev, seed)
    _placeholder_paths_are_live(m, B, dev)
    with pytest.raises(RuntimeError, match="never claimed"):
        _vanilla_step_by_hand(m, xd, eps, second_consumer=True)
    assert not K._lazy_grads
    _vanilla_step_by_hand(fresh, xd, eps)                   # the same forward passes on both sides: BatchNorm's running statistics
    got, want = _vanilla_step_by_hand(m, xd, eps), _vanilla_step_by_hand(fresh, xd, eps)
    assert torch.isfinite(want[0]) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.isfinite(fresh.flat_grads).all() and fresh.flat_grads.abs().max() > 0
    assert torch.equal(m.flat_grads, fresh.flat_grads)
    for (k, a), (_, b) in zip(m.named_buffers(), fresh.named_buffers()):
        assert torch.equal(a, b), k


def test_vanilla_b4_step_runs_the_placeholder_kernels(dev):
    """An ordinary B = 4 training step takes all three placeholder paths: the kernels that sum the slices ran."""
    from ctvae_amd import kernels as K
    from ctvae_amd import native
    B, seed = 4, 41
    x, eps = filler.synthetic_batch(seed, B)
    m = build_vanilla(dev, seed)
    _placeholder_paths_are_live(m, B, dev)
    native.prof_report()
    native.prof_enable(True)
    try:
        out = m(x.to(dev), eps=eps.to(dev))
        K.backward(m.loss_function(*out, M_N=0.00025)["loss"])
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    rep = native.prof_report()
    for name in ("gauss_latent_fwd_kernel", "gauss_latent_bwd_kernel", "splitk_permute_kernel", "bn_fused_bwd_kernel"):
        assert name in rep and rep[name]["count"] >= 1, (name, sorted(rep))
    assert not K._lazy_grads and torch.isfinite(m.flat_grads).all()


def test_vanilla_vs_oracle_b16(dev):
    from oracle import vae_cpu as O
    seed, B = 77, 16
    m = build_vanilla(dev, seed)
    sd = filler.fill_state(H.vanilla_specs(), seed + 1)
    x, eps = filler.synthetic_batch(seed, B)
    ref_losses, ref_grads, ref_nb, ref_out = O.vanilla_step(sd, x, eps, 0.00025)
    out = m(x.to(dev), eps=eps.to(dev))
    losses = m.loss_function(*out, M_N=0.00025)
    losses["loss"].backward()
    torch.cuda.synchronize()
    np.testing.assert_allclose(out[0].detach().cpu().numpy(), ref_out["recons"].numpy(), atol=TOL, rtol=0)
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), ref_out["mu"].numpy(), atol=TOL, rtol=0)
    for k in ("loss", "Reconstruction_Loss", "KLD"):
        assert abs(losses[k].item() - ref_losses[k].item()) <= TOL * max(1.0, abs(ref_losses[k].item()))
    for k, p in m.named_parameters():
        ref = ref_grads[k]
        tol = TOL * max(1.0, float(ref.abs().max()))
        np.testing.assert_allclose(p.grad.cpu().numpy(), ref.numpy(), atol=tol, rtol=2e-3, err_msg=k)
    # eval mode uses running statistics
    m.eval()
    with torch.no_grad():
        r_eval = m.generate(x.to(dev))
    nb = dict(sd)
    nb.update(ref_nb)
    with torch.no_grad():
        mu, lv = O.vanilla_encode(nb, x, training=False)
    # generate() draws its own eps: compare the deterministic part only
    mu_h, _ = m.encode(x.to(dev))
    np.testing.assert_allclose(mu_h.detach().cpu().numpy(), mu.numpy(), atol=TOL, rtol=0)
    assert r_eval.shape == (B, 3, 64, 64)


@pytest.mark.parametrize("tag,cfg", [("mcq", H.MCQ_CFG), ("ctconv", H.CT_CONV_CFG)])
@pytest.mark.parametrize("B", [2, 4])
def test_mcq_vs_golden(dev, golden, tag, cfg, B):
    g = golden(f"{tag}_b{B}")
    seed = int(g["seed"])
    m = build_mcq(dev, cfg, seed)
    x, _ = filler.synthetic_batch(seed, B)
    xd = x.to(dev)
    lat = m.encode(xd)[0]
    inds = m.vq_layer.compute_inds(lat)
    q, vq_loss = m.vq_layer.compute_latents(lat, inds)
    recons = m.decode(q)
    losses = m.loss_function(recons, xd, vq_loss)
    losses["loss"].backward()
    torch.cuda.synchronize()
    bad = inds.cpu().numpy() != g["inds"]
    assert not (bad & (g["margin"] > 1e-5)).any(), "index mismatch outside near-ties (SURVEY N2)"
    assert not bad.any(), "near-tie flip: downstream comparisons would be meaningless for this seed"
    if B <= 2:
        np.testing.assert_allclose(lat.detach().cpu().numpy(), g["latents"], atol=TOL, rtol=0)
        np.testing.assert_allclose(recons.detach().cpu().numpy(), g["recons"], atol=TOL, rtol=0)
    else:
        np.testing.assert_allclose(recons.detach().cpu()[:, :, ::4, ::4].numpy(), g["recons_strided"], atol=TOL, rtol=0)
    H.assert_cks_close(H.cks(q), g["quantized_cks"], rtol=1e-4, atol=1e-5, what="quantized")
    for k in ("loss", "Reconstruction_Loss", "VQ_Loss"):
        assert abs(losses[k].item() - float(g["loss." + k])) <= TOL, k
    grads = {k: p.grad for k, p in m.named_parameters()}
    for k, gr in grads.items():
        H.assert_cks_close(H.cks(gr), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    for k in [k[5:] for k in g if k.startswith("grad.")]:
        np.testing.assert_allclose(grads[k].cpu().numpy(), g["grad." + k], atol=TOL, rtol=2e-3, err_msg=k)


def test_mcq_forward_api(dev):
    m = build_mcq(dev, H.MCQ_CFG, 3)
    x, _ = filler.synthetic_batch(3, 3)
    out = m(x.to(dev))
    assert len(out) == 3 and out[0].shape == (3, 3, 64, 64) and out[2].dim() == 0
    l = m.loss_function(*out)
    assert set(l) == {"loss", "Reconstruction_Loss", "VQ_Loss"}
    assert m.sample(2, dev).shape == (2, 3, 64, 64)
    assert m.generate(x.to(dev)).shape == (3, 3, 64, 64)


def test_zero_grad_and_set_to_none(dev):
    m = build_vanilla(dev, 5)
    x, eps = filler.synthetic_batch(5, 2)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    for _ in range(2):
        opt.zero_grad()                      # set_to_none=True: the model re-attaches its flat gradient views
        out = m(x.to(dev), eps=eps.to(dev))
        m.loss_function(*out, M_N=0.00025)["loss"].backward()
        assert all(p.grad is not None for p in m.parameters())
        opt.step()
    g1 = m.flat_grads.clone()
    m.zero_grad()
    assert m.flat_grads.abs().max().item() == 0.0
    out = m(x.to(dev), eps=eps.to(dev))
    m.loss_function(*out, M_N=0.00025)["loss"].backward()
    assert torch.isfinite(m.flat_grads).all() and g1.abs().max().item() > 0


def test_split_backward_matches_single_backward():
    """ddp.SplitBackward (backward cut at the latent, used to overlap the decoder-side all-reduce with the encoder's
    backward) must leave exactly the gradients of the ordinary single backward pass."""
    import torch
    from ctvae_amd import filler
    from ctvae_amd.ddp import SplitBackward
    from ctvae_amd.models import vae_models
    from tests import helpers as H
    dev = torch.device("cuda")
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
    m.load_state_dict(filler.fill_state(filler.specs_of(m), 77))
    m = m.to(dev).train()
    x, eps = filler.synthetic_batch(76, 8)
    x, eps = x.to(dev), eps.to(dev)
    m.zero_grad()
    out = m(x, eps=eps)
    l1 = m.loss_function(*out, M_N=0.00025)
    l1["loss"].backward()
    g_ref = m.flat_grads.clone()
    rm_ref = m.encoder[0]._modules["1"].running_mean.clone()
    # same step again through the two-stage path (running stats move on, gradients must not care)
    sb = SplitBackward(m)
    assert 0 < sb.split < sb.total
    m.zero_grad()
    l2 = sb.stage1(x, eps=eps, M_N=0.00025)
    g_dec = m.flat_grads[sb.split:].clone()
    assert float(m.flat_grads[:sb.split].abs().max()) == 0.0, "stage 1 must not touch the encoder-side gradients"
    sb.stage2()
    torch.cuda.synchronize()
    assert abs(float(l1["loss"]) - float(l2["loss"])) < 1e-6
    assert torch.equal(m.flat_grads[sb.split:], g_dec), "stage 2 must not touch the decoder-side gradients"
    scale = float(g_ref.abs().max())
    assert float((m.flat_grads - g_ref).abs().max()) <= 1e-5 * max(1.0, scale)
    assert not torch.equal(rm_ref, torch.zeros_like(rm_ref))


def test_eval_mode_final_block_matches_unfused_path():
    """Eval mode (running statistics) through the fused final block (BatchNorm applied on load by the 3-channel conv)
    against the same model with the fusion switched off, and train-mode parity of both paths."""
    import torch
    from ctvae_amd import filler, kernels as K
    from ctvae_amd.models import vae_models
    dev = torch.device("cuda")
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
    m.load_state_dict(filler.fill_state(filler.specs_of(m), 91))
    m = m.to(dev)
    x, eps = filler.synthetic_batch(90, 4)
    x, eps = x.to(dev), eps.to(dev)
    m.train()
    for _ in range(2):                      # move the running statistics away from their init
        m(x, eps=eps)
    outs = {}
    real = K.input_transform_supported
    try:
        for fused in (True, False):
            K.input_transform_supported = real if fused else (lambda *a, **k: False)
            m.eval()
            with torch.no_grad():
                outs[("eval", fused)] = m(x, eps=eps)[0].clone()
            sample = m.sample(2, dev)
            assert sample.shape == (2, 3, 64, 64) and torch.isfinite(sample).all()
    finally:
        K.input_transform_supported = real
    assert float((outs[("eval", True)] - outs[("eval", False)]).abs().max()) < 1e-5


def test_harness_hipgraph_training_matches_eager():
    """VAEXperiment.fit with the hipGraph-captured training step (3 eager warm-up steps, then replays) must follow the
    eager trajectory exactly; MCQVAE has no random draw in its step, so parameters can be compared bit for bit."""
    import torch
    from ctvae_amd import filler
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    from tests import helpers as H
    dev = torch.device("cuda")
    batches = [(filler.synthetic_batch(500 + i, 8)[0].to(dev), torch.zeros(8, device=dev)) for i in range(7)]
    finals = []
    for use_graph in (False, True):
        cfg = {**H.MCQ_CFG, "hidden_dims": list(H.MCQ_CFG["hidden_dims"])}    # the constructor reverses the list in place
        sd = filler.fill_state(H.mcq_specs(cfg), 501)
        m = vae_models["MCQVAE"](**cfg)
        m.load_state_dict(sd)
        m = m.to(dev).train()
        exp = VAEXperiment(m, {"LR": 0.0005, "weight_decay": 0.0, "scheduler_gamma": 0.95, "kld_weight": 0.00025,
                               "hipgraph": use_graph})
        exp.fit(lambda: iter(batches), None, max_epochs=1)
        torch.cuda.synchronize()
        assert exp.global_step == len(batches)
        if use_graph:
            assert any(g.graph is not None for g in exp._graphed.values()), "no hipGraph was captured"
        finals.append(m.flat_params.clone())
    assert torch.equal(finals[0], finals[1])


def test_mcq_winograd_matches_direct_kernels(dev):
    """MCQ-VAE training step at a batch where the residual 3x3 layers run Winograd (wino.hip): encoder latents, the
    reconstruction, the losses and every parameter gradient agree with the same step on the direct tap-GEMM kernels
    (ctvae_winograd_enable(0)) -- the path that the golden vectors above pin -- within the 1e-4 parity bound."""
    from ctvae_amd import native
    B, seed = 128, 11
    x, _ = filler.synthetic_batch(seed, B)
    xd = x.to(dev)

    def step(wino, inds=None):
        prev = native.winograd_enable(wino)
        try:
            m = build_mcq(dev, H.MCQ_CFG, seed)
            native.prof_enable(True)
            lat = m.encode(xd)[0]
            if inds is None:
                inds = m.vq_layer.compute_inds(lat)
            q, vq_loss = m.vq_layer.compute_latents(lat, inds)      # same code indices on both sides: no near-tie flips
            recons = m.decode(q)
            losses = m.loss_function(recons, xd, vq_loss)
            losses["loss"].backward()
            torch.cuda.synchronize()
            native.prof_enable(False)
            rep = native.prof_report()
        finally:
            native.winograd_enable(prev)
        return m, lat.detach(), inds, recons.detach(), {k: float(v) for k, v in losses.items()}, rep

    m_d, lat_d, inds, rec_d, loss_d, rep_d = step(False)
    m_w, lat_w, _, rec_w, loss_w, rep_w = step(True, inds)
    assert ("wino_conv_kernel" in rep_w or "wino_conv_fs_kernel" in rep_w) and "wino_wgrad_kernel" in rep_w, sorted(rep_w)
    assert not any(k.startswith("wino_") for k in rep_d), sorted(rep_d)
    np.testing.assert_allclose(lat_w.cpu().numpy(), lat_d.cpu().numpy(), atol=TOL, rtol=0)
    np.testing.assert_allclose(rec_w.cpu().numpy(), rec_d.cpu().numpy(), atol=TOL, rtol=0)
    for k in loss_d:
        assert abs(loss_w[k] - loss_d[k]) <= TOL, (k, loss_w[k], loss_d[k])
    gd = {k: p.grad for k, p in m_d.named_parameters()}
    for k, p in m_w.named_parameters():
        a, b = p.grad.cpu().numpy(), gd[k].cpu().numpy()
        sc = max(1.0, float(np.abs(b).max()))
        np.testing.assert_allclose(a, b, atol=TOL * sc, rtol=2e-3, err_msg=k)


@pytest.mark.parametrize("tag,cfg", [("H", dict(loss_type="H", beta=10.0)),
                                     ("B", dict(loss_type="B", gamma=10.0, max_capacity=25, Capacity_max_iter=10000))])
def test_beta_vae_vs_golden(dev, golden, tag, cfg):
    """BetaVAE (VanillaVAE's network, beta / capacity objectives) against the reference's own beta_vae.py fixture: two
    consecutive loss calls (type 'B' depends on the call counter) and every parameter gradient of the first."""
    from ctvae_amd.models import vae_models
    g = golden(f"beta_{tag}_b2")
    seed = int(g["seed"])
    m = vae_models["BetaVAE"](in_channels=3, latent_dim=128, **cfg)
    m.load_state_dict(filler.fill_state(H.vanilla_specs(), seed + 1))
    m = m.to(dev).train()
    x, eps = filler.synthetic_batch(seed, 2)
    out = m(x.to(dev), eps=eps.to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["mu"], atol=TOL, rtol=0)
    l1 = m.loss_function(*out, M_N=float(g["M_N"]))
    l1["loss"].backward()
    with torch.no_grad():
        l2 = m.loss_function(*out, M_N=float(g["M_N"]))
    for call, l in (("call1", l1), ("call2", l2)):
        for k in ("loss", "Reconstruction_Loss", "KLD"):
            want = float(g[f"{call}.{k}"])
            assert abs(float(l[k].detach()) - want) <= TOL * max(1.0, abs(want)), (call, k, float(l[k].detach()), want)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)


def test_categorical_vae_vs_golden(dev, golden):
    """CategoricalVAE (cat_vae.py: VanillaVAE's stacks around a Gumbel-softmax categorical latent) against the reference's
    own fixture: logits, reconstruction, loss dict, temperature annealing, every parameter gradient."""
    from ctvae_amd.models import vae_models
    g = golden("cat_b2")
    seed = int(g["seed"])
    D, Q = 64, 40
    m = vae_models["CategoricalVAE"](in_channels=3, latent_dim=D, categorical_dim=Q, temperature=0.5, anneal_rate=0.00003,
                                     anneal_interval=100, alpha=1.0)
    m.load_state_dict(filler.fill_state(H.cat_specs(D, Q), seed + 1))
    m = m.to(dev).train()
    x, _ = filler.synthetic_batch(seed, 2)
    out = m(x.to(dev), u=H.cat_uniform(seed, 2, D, Q).to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["q"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out[0].detach()[:, :, ::8, ::8].cpu().numpy(), g["recons_slice"], atol=TOL, rtol=0)
    l1 = m.loss_function(*out, M_N=float(g["M_N"]), batch_idx=0)
    l1["loss"].backward()
    with torch.no_grad():
        l2 = m.loss_function(*out, M_N=float(g["M_N"]), batch_idx=100)
    assert float(m.temp) == float(g["temp_after"])
    for call, l in (("call1", l1), ("call2", l2)):
        for k in ("loss", "Reconstruction_Loss", "KLD"):
            want = float(g[f"{call}.{k}"])
            assert abs(float(l[k].detach()) - want) <= TOL * max(1.0, abs(want)), (call, k, float(l[k].detach()), want)
    np.testing.assert_allclose(m.fc_z.bias.grad.cpu().numpy(), g["grad.fc_z.bias"], atol=TOL, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    assert m.sample(3, dev).shape == (3, 3, 64, 64)


@pytest.mark.parametrize("tag", ["iwae", "miwae"])
def test_iwae_miwae_vs_golden(dev, golden, tag):
    """IWAE / MIWAE against the reference's own fixtures: repeated posterior parameters, reconstructions of all samples,
    the importance-weighted loss dict and every parameter gradient (weights not detached)."""
    from ctvae_amd.models import vae_models
    g = golden(f"{tag}_b2")
    seed = int(g["seed"])
    name, cfg, lead = H.IW_CASES[tag]
    m = vae_models[name](**cfg)
    m.load_state_dict(filler.fill_state(H.vanilla_specs(), seed + 1))
    m = m.to(dev).train()
    x, _ = filler.synthetic_batch(seed, 2)
    out = m(x.to(dev), eps=H.iw_noise(seed, (2,) + lead).to(dev))
    assert tuple(out[0].shape) == tuple(g["recons_shape"]) and tuple(out[2].shape) == g["mu"].shape
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["mu"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out[0].detach()[..., ::16, ::16].cpu().numpy(), g["recons_slice"], atol=TOL, rtol=0)
    H.assert_cks_close(H.cks(out[4]), g["z_cks"], rtol=1e-5, atol=1e-5, what="z")
    losses = m.loss_function(*out, M_N=float(g["M_N"]))
    losses["loss"].backward()
    for k in ("loss", "Reconstruction_Loss", "KLD"):
        want = float(g["loss." + k])
        assert abs(float(losses[k].detach()) - want) <= TOL * max(1.0, abs(want)), (k, float(losses[k].detach()), want)
    for k in ("fc_mu.bias", "fc_var.bias"):
        np.testing.assert_allclose(getattr(m, k.split(".")[0]).bias.grad.cpu().numpy(), g["grad." + k], atol=1e-6, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    assert m.sample(3, dev).shape == (3, 3, 64, 64) and m.generate(x.to(dev)).shape == (2, 3, 64, 64)


def test_logcosh_vae_vs_golden(dev, golden):
    """LogCoshVAE against the reference's own logcosh_vae.py fixture: loss dict and every parameter gradient."""
    from ctvae_amd.models import vae_models
    g = golden("logcosh_b2")
    seed = int(g["seed"])
    m = vae_models["LogCoshVAE"](in_channels=3, latent_dim=128, alpha=10.0, beta=1.0)
    m.load_state_dict(filler.fill_state(H.vanilla_specs(), seed + 1))
    m = m.to(dev).train()
    x, eps = filler.synthetic_batch(seed, 2)
    out = m(x.to(dev), eps=eps.to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["mu"], atol=TOL, rtol=0)
    losses = m.loss_function(*out, M_N=float(g["M_N"]))
    losses["loss"].backward()
    for k in ("loss", "Reconstruction_Loss", "KLD"):
        want = float(g["loss." + k])
        assert abs(float(losses[k].detach()) - want) <= TOL * max(1.0, abs(want)), (k, float(losses[k].detach()), want)
    np.testing.assert_allclose(m.fc_mu.bias.grad.cpu().numpy(), g["grad.fc_mu.bias"], atol=1e-5, rtol=2e-3)
    np.testing.assert_allclose(m.final_layer._modules["3"].weight.grad.cpu().numpy(), g["grad.final_layer.3.weight"], atol=1e-5, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)


def test_mssim_loss_kernel_vs_golden(dev, golden):
    """csrc/ssim.hip on its own against the pair recorded from the reference's MSSIM module: value and full gradient."""
    from ctvae_amd import kernels as K
    g = golden("mssim_b4")
    a = torch.from_numpy(g["pair.a"]).permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
    b = torch.from_numpy(g["pair.b"]).permute(0, 2, 3, 1).contiguous().to(dev)
    val = K.MSSIMLoss.apply(a, b)
    assert abs(float(val.detach()) - float(g["pair.loss"])) <= 2e-6, (float(val.detach()), float(g["pair.loss"]))
    (3.0 * val).backward()
    want = 3.0 * np.transpose(g["pair.grad_a"], (0, 2, 3, 1))
    np.testing.assert_allclose(a.grad.cpu().numpy(), want, atol=2e-7 * max(1.0, float(np.abs(want).max()) / 1e-3), rtol=2e-3)


def test_mssim_vae_vs_golden(dev, golden):
    """MSSIMVAE against the reference's own mssim_vae.py fixture: loss dict and every parameter gradient."""
    from ctvae_amd.models import vae_models
    g = golden("mssim_b4")
    seed = int(g["seed"])
    m = vae_models["MSSIMVAE"](in_channels=3, latent_dim=128)
    assert list(m.state_dict().keys()) == list(g["keys"])
    m.load_state_dict(filler.fill_state(H.vanilla_specs(), seed + 1))
    m = m.to(dev).train()
    x, eps = filler.synthetic_batch(seed, 4)
    out = m(x.to(dev), eps=eps.to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["mu"], atol=TOL, rtol=0)
    losses = m.loss_function(*out, M_N=float(g["M_N"]))
    losses["loss"].backward()
    for k in ("loss", "Reconstruction_Loss", "KLD"):
        want = float(g["loss." + k])
        assert abs(float(losses[k].detach()) - want) <= TOL * max(1.0, abs(want)), (k, float(losses[k].detach()), want)
    np.testing.assert_allclose(m.fc_mu.bias.grad.cpu().numpy(), g["grad.fc_mu.bias"], atol=1e-5, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)


@pytest.mark.parametrize("tag", ["wae_imq", "wae_rbf", "infovae"])
def test_mmd_models_vs_golden(dev, golden, tag):
    """WAE_MMD (imq / rbf) and InfoVAE against the reference's own fixtures: latent codes, loss dict (incl. the MMD term),
    every parameter gradient."""
    from ctvae_amd.models import vae_models
    g = golden(f"{tag}_b4")
    seed, B = int(g["seed"]), 4
    name, cfg = H.MMD_CASES[tag]
    gaussian = name == "InfoVAE"
    m = vae_models[name](**cfg)
    m.load_state_dict(filler.fill_state(H.vanilla_specs() if gaussian else H.wae_specs(), seed + 1))
    m = m.to(dev).train()
    x, eps = filler.synthetic_batch(seed, B)
    out = m(x.to(dev), eps=eps.to(dev)) if gaussian else m(x.to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["z"], atol=TOL, rtol=0)
    losses = m.loss_function(*out, M_N=float(g["M_N"]), prior_z=H.mmd_prior(seed, B).to(dev))
    losses["loss"].backward()
    for k, v in losses.items():
        want = float(g["loss." + k])
        assert abs(float(v.detach()) - want) <= TOL * max(1.0, abs(want)), (k, float(v.detach()), want)
    head = "fc_mu" if gaussian else "fc_z"
    np.testing.assert_allclose(getattr(m, head).bias.grad.cpu().numpy(), g[f"grad.{head}.bias"], atol=1e-5, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)


ZOO = [("VanillaVAE", dict(in_channels=3, latent_dim=128)),
       ("BetaVAE", dict(in_channels=3, latent_dim=128, loss_type="H", beta=10.0)),
       ("LogCoshVAE", dict(in_channels=3, latent_dim=128, alpha=10.0, beta=1.0)),
       ("IWAE", dict(in_channels=3, latent_dim=128, num_samples=5)),
       ("MIWAE", dict(in_channels=3, latent_dim=128, num_samples=5, num_estimates=3)),
       ("WAE_MMD", dict(in_channels=3, latent_dim=128, reg_weight=100, kernel_type="imq")),
       ("InfoVAE", dict(in_channels=3, latent_dim=128, reg_weight=110, kernel_type="imq", alpha=-9.0, beta=10.5)),
       ("DIPVAE", dict(in_channels=3, latent_dim=128, lambda_diag=0.05, lambda_offdiag=0.1)),
       ("JointVAE", dict(H.JOINT_CFG)),
       ("ConditionalVAE", dict(H.CVAE_CFG)),
       ("SWAE", dict(H.SWAE_CFG)),
       ("TwoStageVAE", dict(in_channels=3, latent_dim=128)),
       ("HVAE", dict(in_channels=3, latent1_dim=64, latent2_dim=64, pseudo_input_size=128)),
       ("VampVAE", dict(in_channels=3, latent_dim=128)),
       ("BetaTCVAE", dict(H.BETATC_CFG)),
       ("GammaVAE", dict(in_channels=3, latent_dim=128, gamma_shape=8., prior_shape=2., prior_rate=1.)),
       ("MSSIMVAE", dict(in_channels=3, latent_dim=128)),
       ("LVAE", dict(H.LVAE_CFG)),
       ("CategoricalVAE", dict(in_channels=3, latent_dim=64, categorical_dim=40, temperature=0.5, alpha=1.0)),
       ("VQVAE", dict(in_channels=3, embedding_dim=64, num_embeddings=512, img_size=64, beta=0.25)),
       ("MCQVAE", dict(in_channels=3, embedding_dim=128, hidden_dims=[64, 128, 256], num_embeddings=64, img_size=64, codebooks=4, beta=0.25))]


@pytest.mark.parametrize("name,cfg", ZOO, ids=[z[0] for z in ZOO])
def test_every_registered_model_trains_through_the_harness(dev, name, cfg):
    """run.py's training loop (VAEXperiment.fit: Adam, hipGraph-captured step after three eager ones, validation with
    M_N = 1) on every model of the registry: the loss stays finite, every parameter receives a gradient and moves, the
    captured step is the one that ran, sample() / generate() return pictures."""
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    torch.manual_seed(3)
    m = vae_models[name](**{k: (list(v) if isinstance(v, list) else v) for k, v in cfg.items()}, name=name).to(dev).train()
    labels = (lambda i: H.cvae_labels(900 + i, 8).to(dev)) if name == "ConditionalVAE" else (lambda i: torch.zeros(8, device=dev))
    batches = [(H.zoo_prepare(name, m, filler.synthetic_batch(900 + i, 8)[0].to(dev)), labels(i)) for i in range(6)]
    before = m.flat_params.clone()
    exp = VAEXperiment(m, {"LR": 0.0005, "weight_decay": 0.0, "scheduler_gamma": 0.95, "kld_weight": 0.00025, "hipgraph": True})
    exp.fit(lambda: iter(batches), lambda: iter(batches[:2]), max_epochs=1)
    torch.cuda.synchronize()
    assert exp.global_step == len(batches)
    if getattr(m, "graph_safe", True):
        assert any(g.graph is not None for g in exp._graphed.values()), "no hipGraph was captured"
    after = m.flat_params
    # TwoStageVAE: 40 % of its parameters are the second stage no step touches; VampVAE: pseudo-input weights behind the flat
    # sides of the Hardtanh (and the zero rows that pad 50 inputs to 64) keep a zero gradient
    moved = {"TwoStageVAE": 0.55, "VampVAE": 0.8}.get(name, 0.9)
    assert torch.isfinite(after).all() and (after != before).float().mean().item() > moved   # codebook rows no latent selected keep a zero gradient
    m.eval()
    with torch.no_grad():
        extra = {"labels": batches[0][1]} if name == "ConditionalVAE" else {}
        assert m.generate(batches[0][0], **extra).shape == (8, 3, 64, 64)
        try:
            assert m.sample(4, dev, **({"labels": batches[0][1][:4]} if extra else {})).shape == (4, 3, 64, 64)
        except Warning:        # the reference's "sampler is not implemented" for the quantised models (vq_vae.py, mcq_vae.py)
            assert name in ("VQVAE", "MCQVAE")


@pytest.mark.parametrize("name,cfg", ZOO, ids=[z[0] for z in ZOO])
def test_lazy_zero_grad_gives_the_same_gradient_buffer(dev, name, cfg):
    """zero_grad(lazy=True) (models/packing.py: no fill, first writers overwrite, settle_grads() fills the rest) against
    zero_grad(): the flat gradient buffer after one forward + backward is the same bit for bit, starting from a buffer
    full of NaN -- so every block is either overwritten completely by its first writer or zero-filled by the settle."""
    from ctvae_amd.models import vae_models
    torch.manual_seed(3)
    m = vae_models[name](**{k: (list(v) if isinstance(v, list) else v) for k, v in cfg.items()}, name=name).to(dev).train()
    x = H.zoo_prepare(name, m, filler.synthetic_batch(901, 8)[0].to(dev))
    labels = H.cvae_labels(901, 8).to(dev) if name == "ConditionalVAE" else torch.zeros(8, device=dev)

    def grads(lazy):
        torch.manual_seed(11)
        for mod in m.modules():                      # in-kernel noise: same Philox key and position in both runs
            if getattr(mod, "_rng_state", None) is not None:
                mod._rng_state = None
            if hasattr(mod, "num_iter"):             # annealed loss weights (betatc_vae.py:166, joint_vae.py:195): same step both times
                mod.num_iter = 0
        m.gather_torch_grads()
        for blk in m._grad_blocks:                   # (the alignment gaps between blocks hold zeros and are never written)
            m._flat_grads[blk.lo:blk.hi] = float("nan")
        for _, g in m._torch_grad_views:
            g.fill_(float("nan"))
        m.zero_grad(lazy=lazy)
        out = m(x, labels=labels)
        m.loss_function(*out, M_N=0.00025, optimizer_idx=0, batch_idx=0)["loss"].backward()
        return m.flat_grads.clone()                  # the property settles / gathers

    want = grads(False)
    got = grads(True)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {want.numel()} gradient elements differ"


@pytest.mark.parametrize("name", ["VanillaVAE", "MCQVAE", "VQVAE", "BetaTCVAE", "ConditionalVAE"])
def test_deferred_slab_reductions_give_the_same_gradients(dev, name):
    """kernels.backward (ctvae_defer_begin / _flush: the weight-gradient slabs go into an arena, ONE launch reduces all of
    them at the end of the pass) against loss.backward() (every reduction behind its kernel): the same bits."""
    from ctvae_amd import kernels as K
    from ctvae_amd.models import vae_models
    cfg = dict(next(c for n, c in ZOO if n == name))
    torch.manual_seed(3)
    m = vae_models[name](**{k: (list(v) if isinstance(v, list) else v) for k, v in cfg.items()}, name=name).to(dev).train()
    x = filler.synthetic_batch(902, 16)[0].to(dev)
    labels = H.cvae_labels(902, 16).to(dev) if name == "ConditionalVAE" else torch.zeros(16, device=dev)

    def grads(deferred):
        torch.manual_seed(11)
        for mod in m.modules():
            if getattr(mod, "_rng_state", None) is not None:
                mod._rng_state = None
            if hasattr(mod, "num_iter"):
                mod.num_iter = 0
        m.zero_grad()
        out = m(x, labels=labels)
        loss = m.loss_function(*out, M_N=0.00025, optimizer_idx=0, batch_idx=0)["loss"]
        if deferred:
            K.backward(loss)
        else:
            loss.backward()
        return m.flat_grads.clone()

    want = grads(False)
    got = grads(True)
    assert K._DEFER_REDUCE and torch.isfinite(want).all() and want.abs().max() > 0
    assert torch.equal(got, want), f"{(got != want).sum().item()} of {want.numel()} gradient elements differ"
    again = grads(True)                      # the arena and the job list are clean after a flush
    assert torch.equal(again, want)


def test_dip_vae_vs_golden(dev, golden):
    """DIPVAE against the reference's own dip_vae.py fixture: loss dict (sums + DIP term) and every parameter gradient."""
    from ctvae_amd.models import vae_models
    g = golden("dip_b4")
    seed = int(g["seed"])
    m = vae_models["DIPVAE"](in_channels=3, latent_dim=128, lambda_diag=0.05, lambda_offdiag=0.1)
    m.load_state_dict(filler.fill_state(H.vanilla_specs(), seed + 1))
    m = m.to(dev).train()
    x, eps = filler.synthetic_batch(seed, 4)
    out = m(x.to(dev), eps=eps.to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["mu"], atol=TOL, rtol=0)
    losses = m.loss_function(*out, M_N=float(g["M_N"]))
    losses["loss"].backward()
    for k, v in losses.items():
        want = float(g["loss." + k])
        assert abs(float(v.detach()) - want) <= TOL * max(1.0, abs(want)), (k, float(v.detach()), want)
    for k in ("fc_mu.bias", "fc_var.bias"):
        np.testing.assert_allclose(getattr(m, k.split(".")[0]).bias.grad.cpu().numpy(), g["grad." + k], atol=2e-3, rtol=2e-3)
    for k, p in m.named_parameters():
        if k.endswith(".0.bias") and not k.startswith("final_layer.3"):
            continue    # bias of a conv in front of a BatchNorm: analytically zero gradient, rounding noise x the sum-reduced loss scale
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-3, what=k)


def test_joint_vae_vs_golden(dev, golden):
    """JointVAE against the reference's own joint_vae.py fixture: logits, means, two consecutive loss dicts, every gradient."""
    from ctvae_amd.models import vae_models
    g = golden("joint_b4")
    seed = int(g["seed"])
    m = vae_models["JointVAE"](**H.JOINT_CFG)
    m.load_state_dict(filler.fill_state(H.joint_specs(), seed + 1))
    m = m.to(dev).train()
    x, e = filler.synthetic_batch(seed, 4)
    out = m(x.to(dev), eps=e.to(dev), u=H.joint_uniform(seed, 4).to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["q"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out[3].detach().cpu().numpy(), g["mu"], atol=TOL, rtol=0)
    l1 = m.loss_function(*out, M_N=float(g["M_N"]), batch_idx=0)
    l1["loss"].backward()
    with torch.no_grad():
        l2 = m.loss_function(*out, M_N=float(g["M_N"]), batch_idx=1)
    for call, l in (("call1", l1), ("call2", l2)):
        for k, v in l.items():
            want = float(g[f"{call}.{k}"])
            assert abs(float(v.detach()) - want) <= TOL * max(1.0, abs(want)), (call, k, float(v.detach()), want)
    for k in ("fc_z.bias", "fc_var.bias"):
        np.testing.assert_allclose(getattr(m, k.split(".")[0]).bias.grad.cpu().numpy(), g["grad." + k], atol=1e-6, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    assert m.sample(3, dev).shape == (3, 3, 64, 64)


def test_vqvae_vs_golden(dev, golden):
    """VQVAE (vq_vae.py: MCQ-VAE's conv stacks around one 512-entry codebook) against the reference's own fixture."""
    from ctvae_amd.models import vae_models
    g = golden("vqvae_b2")
    seed = int(g["seed"])
    cfg = {**H.VQVAE_CFG, "hidden_dims": list(H.VQVAE_CFG["hidden_dims"])}
    cfg.pop("codebooks")
    m = vae_models["VQVAE"](**cfg)
    m.load_state_dict(filler.fill_state(H.vqvae_specs(), seed + 1))
    m = m.to(dev).train()
    x, _ = filler.synthetic_batch(seed, 2)
    xd = x.to(dev)
    lat = m.encode(xd)[0]
    inds = m.vq_layer.compute_inds(lat)
    assert not ((inds.cpu().numpy() != g["inds"]) & (g["margin"] > 1e-5)).any()
    out = m(xd)
    losses = m.loss_function(*out)
    losses["loss"].backward()
    np.testing.assert_allclose(lat.detach().cpu().numpy(), g["latents"], atol=TOL, rtol=0)
    H.assert_cks_close(H.cks(out[0]), g["recons_cks"], rtol=1e-4, atol=1e-5, what="recons")
    for k in ("loss", "Reconstruction_Loss", "VQ_Loss"):
        assert abs(float(losses[k].detach()) - float(g["loss." + k])) <= TOL, k
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    with pytest.raises(Warning):
        m.sample(2, dev)


def test_conditional_vae_vs_golden(dev, golden):
    """ConditionalVAE against the reference's own cvae.py fixture: means, log-variances, reconstruction, loss dict, every
    gradient (the label embeddings, the 4-channel first conv and the widened decoder_input included)."""
    from ctvae_amd.models import vae_models
    g = golden("cvae_b4")
    seed = int(g["seed"])
    m = vae_models["ConditionalVAE"](**H.CVAE_CFG)
    m.load_state_dict(filler.fill_state(H.cvae_specs(), seed + 1))
    m = m.to(dev).train()
    x, e = filler.synthetic_batch(seed, 4)
    labels = H.cvae_labels(seed, 4).to(dev)
    out = m(x.to(dev), eps=e.to(dev), labels=labels)
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["mu"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out[3].detach().cpu().numpy(), g["log_var"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out[0].detach()[:, :, ::8, ::8].cpu().numpy(), g["recons_sub"], atol=TOL, rtol=0)
    losses = m.loss_function(*out, M_N=float(g["M_N"]))
    for k, v in losses.items():
        want = float(g["loss." + k])
        assert abs(float(v.detach()) - want) <= TOL * max(1.0, abs(want)), (k, float(v.detach()), want)
    m.zero_grad()
    losses["loss"].backward()
    # gradients that reach the image side pass back through five BatchNorm layers at B = 4: differently ordered fp32 sums are
    # amplified there (1.5e-5 on values of 1e-3); same absolute allowance as the checksums below
    np.testing.assert_allclose(m.embed_data.weight.grad.cpu().numpy(), g["grad.embed_data.weight"], atol=2e-5, rtol=2e-3)
    np.testing.assert_allclose(m.embed_data.bias.grad.cpu().numpy(), g["grad.embed_data.bias"], atol=2e-5, rtol=2e-3)
    np.testing.assert_allclose(m.embed_class.bias.grad[::16].cpu().numpy(), g["grad.embed_class.bias_sub"], atol=2e-6, rtol=2e-3)
    np.testing.assert_allclose(m.decoder_input.weight.grad[::64, 128:].cpu().numpy(), g["grad.decoder_input.weight_labelcols"],
                               atol=1e-6, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    for k, b in m.named_buffers():
        if "running" in k:
            H.assert_cks_close(H.cks(b), g["buf." + k], rtol=1e-4, atol=1e-5, what=k)
    assert m.sample(3, dev, labels=labels[:3]).shape == (3, 3, 64, 64)
    assert m.generate(x.to(dev), labels=labels).shape == (4, 3, 64, 64)


def test_swae_vs_golden(dev, golden):
    """SWAE against the reference's own swae.py fixture: codes, loss dict (mse + l1, SWD), every gradient; the SWD kernel
    (projections + per-direction sort + rank-wise power) against the torch expression at other batch sizes and exponents."""
    from ctvae_amd import kernels as K
    from ctvae_amd.models import vae_models
    g = golden("swae_b8")
    seed, B = int(g["seed"]), int(g["B"])
    m = vae_models["SWAE"](**H.SWAE_CFG)
    m.load_state_dict(filler.fill_state(H.wae_specs(), seed + 1))
    m = m.to(dev).train()
    x, _ = filler.synthetic_batch(seed, B)
    out = m(x.to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["z"], atol=TOL, rtol=0)
    prior, proj = H.swae_draws(seed, B)
    losses = m.loss_function(*out, M_N=0.00025, prior_z=prior.to(dev), proj=proj.to(dev))
    for k, v in losses.items():
        want = float(g["loss." + k])
        assert abs(float(v.detach()) - want) <= TOL * max(1.0, abs(want)), (k, float(v.detach()), want)
    m.zero_grad()
    losses["loss"].backward()
    np.testing.assert_allclose(m.fc_z.bias.grad.cpu().numpy(), g["grad.fc_z.bias"], atol=2e-6, rtol=2e-3)
    np.testing.assert_allclose(m.final_layer._modules["3"].bias.grad.cpu().numpy(), g["grad.final_layer.3.bias"], atol=2e-6, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    assert m.sample(3, dev).shape == (3, 3, 64, 64)
    # the distance kernel alone: odd batch sizes (padding of the bitonic network), p = 2 and p = 4, default draws run
    gen = torch.Generator().manual_seed(3)
    for N, S, p in ((37, 50, 2.0), (256, 200, 2.0), (64, 16, 4.0), (1000, 8, 2.0)):
        z = torch.randn(N, 128, generator=gen).to(dev).requires_grad_(True)
        pr = torch.randn(N, 128, generator=gen).to(dev)
        r = torch.randn(S, 128, generator=gen)
        pj = (r / r.norm(dim=1).view(-1, 1)).to(dev)
        got = K.SWD.apply(z, pr, pj, p, 0.7)
        got.backward()
        z2 = z.detach().clone().requires_grad_(True)
        wd = torch.sort(z2.matmul(pj.t()).t(), dim=1)[0] - torch.sort(pr.matmul(pj.t()).t(), dim=1)[0]
        ref = 0.7 * wd.pow(p).mean()
        ref.backward()
        assert abs(float(got) - float(ref)) <= 1e-5 * max(1.0, abs(float(ref))), (N, S, p, float(got), float(ref))
        # two samples whose projections on some direction agree to rounding may swap ranks between the two dot-product orders;
        # the swap moves their gradients by the gap of their rank partners: compare in the L2 sense, not element by element
        assert float((z.grad - z2.grad).norm() / z2.grad.norm()) <= 2e-3, (N, S, p)
    assert torch.isfinite(m.loss_function(*m(x.to(dev)), M_N=0.00025)["loss"])


def test_twostage_vae_vs_golden(dev, golden):
    """TwoStageVAE against the reference's own twostage_vae.py fixture: state_dict keys / shapes, the first-stage step, and the
    second-stage parameters receiving no gradient (they stay put through an optimizer step)."""
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    g = golden("twostage_b2")
    seed = int(g["seed"])
    m = vae_models["TwoStageVAE"](in_channels=3, latent_dim=128)
    assert [k for k in m.state_dict()] == list(g["keys"])
    assert [str(tuple(v.shape)) for v in m.state_dict().values()] == list(g["shapes"])
    m.load_state_dict(filler.fill_state(H.twostage_specs(), seed + 1))
    m = m.to(dev).train()
    x, e = filler.synthetic_batch(seed, 2)
    out = m(x.to(dev), eps=e.to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["mu"], atol=TOL, rtol=0)
    losses = m.loss_function(*out, M_N=float(g["M_N"]))
    for k, v in losses.items():
        want = float(g["loss." + k])
        assert abs(float(v.detach()) - want) <= TOL * max(1.0, abs(want)), (k, float(v.detach()), want)
    m.zero_grad()
    K_backward = __import__("ctvae_amd.kernels", fromlist=["backward"]).backward
    K_backward(losses["loss"])
    m.gather_torch_grads()
    no_grad = set(g["no_grad"])
    for k, p in m.named_parameters():
        if k in no_grad:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        elif not (k.startswith(("encoder.", "decoder.")) and k.endswith(".0.bias")) and k != "final_layer.0.bias":
            H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    before = {k: p.detach().clone() for k, p in m.named_parameters() if k in no_grad}
    exp = VAEXperiment(m, {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 0.00025, "hipgraph": False})
    exp.optimizer_step()
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        if k in no_grad:
            assert torch.equal(p.detach(), before[k]), k


def test_hvae_vs_golden(dev, golden):
    """HVAE against the reference's own hvae.py fixture: both levels' posterior means, z1, reconstruction, loss dict (the three
    Gaussian-KL terms through the KL kernels), every gradient."""
    from ctvae_amd.models import vae_models
    g = golden("hvae_b4")
    seed, B = int(g["seed"]), int(g["B"])
    m = vae_models["HVAE"](in_channels=3, latent1_dim=64, latent2_dim=64, pseudo_input_size=128)
    assert list(m.state_dict().keys()) == list(g["keys"])
    m.load_state_dict(filler.fill_state(H.hvae_specs(), seed + 1))
    m = m.to(dev).train()
    x, _ = filler.synthetic_batch(seed, B)
    e1, e2 = H.hvae_noise(seed, B)
    out = m(x.to(dev), eps=e1.to(dev), eps2=e2.to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["z1_mu"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out[4].detach().cpu().numpy(), g["z2_mu"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out[6].detach().cpu().numpy(), g["z1"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out[0].detach()[:, :, ::8, ::8].cpu().numpy(), g["recons_sub"], atol=TOL, rtol=0)
    losses = m.loss_function(*out, M_N=float(g["M_N"]))
    for k, v in losses.items():
        want = float(g["loss." + k])
        assert abs(float(v.detach()) - want) <= TOL * max(1.0, abs(want)), (k, float(v.detach()), want)
    m.zero_grad()
    losses["loss"].backward()
    np.testing.assert_allclose(m.recons_z1_mu.bias.grad.cpu().numpy(), g["grad.recons_z1_mu.bias"], atol=1e-7, rtol=2e-3)
    # z2's gradient arrives through encoder_z1's five BatchNorm layers at B = 4 (16 values per channel in the deepest one):
    # a different summation order in that BatchNorm backward moves these ~1e-3 entries by a few 1e-6
    np.testing.assert_allclose(m.fc_z2_var.bias.grad.cpu().numpy(), g["grad.fc_z2_var.bias"], atol=1e-5, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    assert m.sample(3, dev).shape == (3, 3, 64, 64)


def test_winograd_filter_cache_follows_the_parameters(dev, monkeypatch):
    """The per-step batched Winograd filter transform (kernels.wino_cache) must never serve filters of older weights: after
    optimizer steps (raw-pointer updates: parameter epoch), after an in-place edit through torch (tensor version) and after
    load_state_dict, a training-mode forward equals -- bit for bit -- the forward of a fresh model holding the same parameters
    with the cache switched off (one transform launch per layer, the round-1 path)."""
    from ctvae_amd import kernels as K
    from ctvae_amd.models import vae_models
    from ctvae_amd.optim import FlatAdam
    cfg = dict(in_channels=3, embedding_dim=128, hidden_dims=[64, 128, 256], num_embeddings=64, img_size=64, codebooks=4, beta=0.25)
    B = 128
    x = filler.synthetic_batch(31, B)[0].to(dev)

    def fresh_forward(src):
        monkeypatch.setattr(K, "_WINO_BATCH", False)
        m2 = vae_models["MCQVAE"](**{k: (list(v) if isinstance(v, list) else v) for k, v in cfg.items()}).to(dev).train()
        m2.load_state_dict(src.state_dict())
        out = m2(x)[0].detach().clone()
        monkeypatch.setattr(K, "_WINO_BATCH", True)
        return out

    torch.manual_seed(5)
    m = vae_models["MCQVAE"](**{k: (list(v) if isinstance(v, list) else v) for k, v in cfg.items()}).to(dev).train()
    opt = FlatAdam(m, lr=1e-3)
    for _ in range(2):
        m.zero_grad()
        out = m(x)
        K.backward(m.loss_function(*out, M_N=0.00025)["loss"])
        opt.step()
    w3 = m.encoder[4].resblock._modules["0"].weight
    e = K.wino_cache.entries.get(id(w3))
    assert e is not None and e["ref"]() is w3, "the Winograd layers did not register with the cache"
    assert torch.equal(m(x)[0].detach(), fresh_forward(m)), "stale filters after optimizer steps"
    with torch.no_grad():
        for p in m.encoder[4].resblock.parameters():
            p.mul_(1.25)
    assert torch.equal(m(x)[0].detach(), fresh_forward(m)), "stale filters after an in-place edit"
    sd = {k: (v * 0.9 if v.is_floating_point() and v.dim() == 4 else v) for k, v in m.state_dict().items()}
    m.load_state_dict(sd)
    assert torch.equal(m(x)[0].detach(), fresh_forward(m)), "stale filters after load_state_dict"


def test_vamp_vae_vs_golden(dev, golden):
    """VampVAE against the reference's own vampvae.py fixture: codes, loss dict (mixture-prior KL through csrc/vamp.hip), every
    gradient incl. the pseudo-input embedding, BatchNorm running statistics after the step's TWO encoder passes; the KL kernel
    against the torch expression on other shapes."""
    from ctvae_amd import kernels as K
    from ctvae_amd.models import vae_models
    g = golden("vamp_b4")
    seed, B = int(g["seed"]), int(g["B"])
    m = vae_models["VampVAE"](in_channels=3, latent_dim=128)
    assert list(m.state_dict().keys()) == list(g["keys"])
    sd = filler.fill_state(H.vamp_specs(), seed + 1)
    sd["embed_pseudo.0.bias"] = sd["embed_pseudo.0.bias"] + 0.5
    m.load_state_dict(sd)
    m = m.to(dev).train()
    x, e = filler.synthetic_batch(seed, B)
    out = m(x.to(dev), eps=e.to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["mu"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out[4].detach().cpu().numpy(), g["z"], atol=TOL, rtol=0)
    losses = m.loss_function(*out, M_N=float(g["M_N"]))
    for k, v in losses.items():
        want = float(g["loss." + k])
        assert abs(float(v.detach()) - want) <= TOL * max(1.0, abs(want)), (k, float(v.detach()), want)
    m.zero_grad()
    losses["loss"].backward()
    np.testing.assert_allclose(m.embed_pseudo._modules["0"].bias.grad[::64].cpu().numpy(), g["grad.embed_pseudo.0.bias_sub"],
                               atol=2e-8, rtol=5e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    for k, b in m.named_buffers():
        if "running" in k:
            H.assert_cks_close(H.cks(b), g["buf." + k], rtol=1e-4, atol=1e-5, what=k)
    assert m.sample(3, dev).shape == (3, 3, 64, 64)
    gen = torch.Generator().manual_seed(8)
    for Bk, D, Kc in ((7, 128, 50), (64, 10, 3), (33, 200, 300)):
        t = [torch.randn(Bk, D, generator=gen).to(dev).requires_grad_(True) for _ in range(3)]
        pr = [(0.5 * torch.randn(Kc, D, generator=gen)).to(dev).requires_grad_(True) for _ in range(2)]
        got = K.VampKL.apply(*t, *pr)
        (3.0 * got).backward()
        t2 = [v.detach().clone().requires_grad_(True) for v in t]
        p2 = [v.detach().clone().requires_grad_(True) for v in pr]
        zz, mm, ll = t2
        eq = torch.mean(torch.sum(-0.5 * (ll + (zz - mm) ** 2) / ll.exp(), dim=1), dim=0)
        ep = torch.sum(-0.5 * (p2[1].unsqueeze(0) + (zz.unsqueeze(1) - p2[0].unsqueeze(0)) ** 2) / p2[1].unsqueeze(0).exp(), dim=2) \
            - torch.log(torch.tensor(float(Kc)))
        ref = -(torch.mean(torch.logsumexp(ep, dim=1), dim=0) - eq)
        (3.0 * ref).backward()
        assert abs(float(got) - float(ref)) <= 2e-5 * max(1.0, abs(float(ref))), (Bk, D, Kc, float(got), float(ref))
        for a, b2 in zip(t + pr, t2 + p2):
            torch.testing.assert_close(a.grad, b2.grad, rtol=2e-4, atol=2e-5 * float(b2.grad.abs().max()))


def test_betatc_vae_vs_golden(dev, golden):
    """BetaTCVAE against the reference's own betatc_vae.py fixture: codes, reconstruction, two consecutive loss dicts (anneal
    counter), every gradient; the decomposition kernel against the torch expression on other shapes."""
    from ctvae_amd import kernels as K
    from ctvae_amd.models import vae_models
    g = golden("betatc_b8")
    seed, B = int(g["seed"]), int(g["B"])
    m = vae_models["BetaTCVAE"](**H.BETATC_CFG)
    assert list(m.state_dict().keys()) == list(g["keys"])
    m.load_state_dict(filler.fill_state(H.betatc_specs(), seed + 1))
    m = m.to(dev).train()
    x, e = filler.synthetic_batch(seed, B, latent_dim=10)
    out = m(x.to(dev), eps=e.to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["mu"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out[4].detach().cpu().numpy(), g["z"], atol=TOL, rtol=0)
    np.testing.assert_allclose(out[0].detach()[:, :, ::8, ::8].cpu().numpy(), g["recons_sub"], atol=TOL, rtol=0)
    l1 = m.loss_function(*out, M_N=float(g["M_N"]))
    m.zero_grad()
    l1["loss"].backward()
    with torch.no_grad():
        l2 = m.loss_function(*out, M_N=float(g["M_N"]))
    for call, l in (("call1", l1), ("call2", l2)):
        for k, v in l.items():
            want = float(g[f"{call}.{k}"])
            assert abs(float(v.detach()) - want) <= TOL * max(1.0, abs(want)), (call, k, float(v.detach()), want)
    np.testing.assert_allclose(m.fc_var.bias.grad.cpu().numpy(), g["grad.fc_var.bias"], atol=2e-4, rtol=2e-3)
    np.testing.assert_allclose(m.fc_mu.bias.grad.cpu().numpy(), g["grad.fc_mu.bias"], atol=2e-4, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-3, what=k)     # sum-reduced objective: gradients of O(1e2)
    assert m.sample(3, dev).shape == (3, 3, 64, 64)
    gen = torch.Generator().manual_seed(12)
    import math
    for Bk, D in ((8, 10), (64, 10), (300, 32), (5, 1)):
        t = [torch.randn(Bk, D, generator=gen).to(dev).requires_grad_(True) for _ in range(3)]
        liw = torch.log(torch.rand(Bk, Bk, generator=gen) * 0.1 + 1e-3).to(dev)
        mi, tc, kld = K.TCDecomp.apply(*t, liw)
        (1.5 * mi + 6.0 * tc + 0.3 * kld).backward()
        zz, mm, ll = [v.detach().clone().requires_grad_(True) for v in t]

        def logn(v, a, b):
            return -0.5 * (math.log(2 * math.pi) + b) - 0.5 * ((v - a) ** 2 * torch.exp(-b))
        mat = logn(zz.view(Bk, 1, D), mm.view(1, Bk, D), ll.view(1, Bk, D)) + liw.view(Bk, Bk, 1)
        lqz, lprod = torch.logsumexp(mat.sum(2), dim=1), torch.logsumexp(mat, dim=1).sum(1)
        lqzx, lpz = logn(zz, mm, ll).sum(1), logn(zz, torch.zeros_like(zz), torch.zeros_like(zz)).sum(1)
        r = ((lqzx - lqz).mean(), (lqz - lprod).mean(), (lprod - lpz).mean())
        (1.5 * r[0] + 6.0 * r[1] + 0.3 * r[2]).backward()
        for a, b2 in zip((mi, tc, kld), r):
            assert abs(float(a.detach()) - float(b2.detach())) <= 2e-5 * max(1.0, abs(float(b2.detach()))), (Bk, D)
        for a, b2 in zip(t, (zz, mm, ll)):
            torch.testing.assert_close(a.grad, b2.grad, rtol=3e-4, atol=3e-5 * float(b2.grad.abs().max()))


def test_gamma_vae_vs_golden(dev, golden):
    """GammaVAE against the reference's own gamma_vae.py fixture (Gamma draw injected): shape / rate heads, reconstruction, loss,
    every gradient; reparameterisation and KL kernels against torch's lgamma / digamma expressions."""
    from ctvae_amd import kernels as K
    from ctvae_amd.models import vae_models
    g = golden("gamma_b4")
    seed, B = int(g["seed"]), int(g["B"])
    m = vae_models["GammaVAE"](in_channels=3, latent_dim=128, gamma_shape=8., prior_shape=2., prior_rate=1.)
    assert list(m.state_dict().keys()) == list(g["keys"])
    m.load_state_dict(filler.fill_state(H.gamma_specs(), seed + 1))
    m = m.to(dev).train()
    x, _ = filler.synthetic_batch(seed, B)
    out = m(x.to(dev), zhat=torch.from_numpy(g["zhat"]).to(dev))
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["alpha"], atol=1e-6, rtol=2e-3)
    np.testing.assert_allclose(out[3].detach().cpu().numpy(), g["beta"], atol=1e-6, rtol=2e-3)
    np.testing.assert_allclose(out[0].detach()[:, :, ::8, ::8].cpu().numpy(), g["recons_sub"], atol=TOL, rtol=0)
    losses = m.loss_function(*out, M_N=0.00025)
    want = float(g["loss.loss"])
    assert abs(float(losses["loss"].detach()) - want) <= TOL * max(1.0, abs(want)), (float(losses["loss"].detach()), want)
    m.zero_grad()
    losses["loss"].backward()
    np.testing.assert_allclose(m.fc_var._modules["0"].bias.grad.cpu().numpy(), g["grad.fc_var.0.bias"], atol=2e-5, rtol=2e-3)
    np.testing.assert_allclose(m.fc_mu._modules["0"].bias.grad.cpu().numpy(), g["grad.fc_mu.0.bias"], atol=2e-5, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-4, what=k)
    assert m.sample(3, dev).shape == (3, 3, 64, 64)
    gen = torch.Generator().manual_seed(21)
    al = torch.softmax(torch.randn(6, 40, generator=gen), 1).to(dev).requires_grad_(True)
    be = torch.softmax(torch.randn(6, 40, generator=gen), 1).to(dev).requires_grad_(True)
    zh = torch.distributions.Gamma(al.detach().cpu() + 8.0, torch.ones(6, 40)).sample().to(dev)
    z = K.GammaReparam.apply(al, be, zh, 8.0)
    kl = K.GammaKL.apply(al, be, 2.0, 1.0)
    (z.sum() + 0.01 * kl).backward()
    a2, b2 = al.detach().clone().requires_grad_(True), be.detach().clone().requires_grad_(True)
    aa = a2 + 8.0
    eps = torch.sqrt(9. * aa - 3.) * ((zh / (aa - 1. / 3.)) ** (1. / 3.) - 1.)
    zr = (aa - 1. / 3.) * (1 + eps / torch.sqrt(9. * aa - 3.)) ** 3 / b2
    c, d = torch.tensor([0.5], device=dev), torch.tensor([1.0], device=dev)

    def I(a, b, c_, d_):
        return -c_ * d_ / a - b * torch.log(a) - torch.lgamma(b) + (b - 1) * (torch.digamma(d_) + torch.log(c_))
    klr = torch.sum(I(c, d, c, d) - I(1 / a2, b2, c, d), dim=1).mean()
    (zr.sum() + 0.01 * klr).backward()
    torch.testing.assert_close(z, zr, rtol=2e-5, atol=1e-5)
    assert abs(float(kl.detach()) - float(klr.detach())) <= 1e-4 * abs(float(klr.detach()))
    torch.testing.assert_close(be.grad, b2.grad, rtol=2e-4, atol=1e-4 * float(b2.grad.abs().max()))
    # d z / d alpha cancels analytically; what is left on both sides is rounding, compare through the KL part's scale
    assert float((al.grad - a2.grad).abs().max()) <= 1e-3 * max(1.0, float(a2.grad.abs().max()))


def test_lvae_vs_golden(dev, golden):
    """LVAE against the reference's own lvae.py fixture: per-sample KL of the four rungs, reconstruction, loss dict, every
    gradient, BatchNorm1d / BatchNorm2d running statistics; the rung kernel against the torch expressions."""
    from ctvae_amd import kernels as K
    from ctvae_amd.models import vae_models
    g = golden("lvae_b4")
    seed, B = int(g["seed"]), int(g["B"])
    m = vae_models["LVAE"](**{k: (list(v) if isinstance(v, list) else v) for k, v in H.LVAE_CFG.items()})
    assert list(m.state_dict().keys()) == list(g["keys"])
    m.load_state_dict(filler.fill_state(filler.specs_of(m), seed + 1))
    m = m.to(dev).train()
    x, _ = filler.synthetic_batch(seed, B)
    out = m(x.to(dev), eps=[e.to(dev) for e in H.lvae_noise(seed, B)])
    np.testing.assert_allclose(out[2].detach().cpu().numpy(), g["kl_div"], atol=2e-3, rtol=2e-4)
    np.testing.assert_allclose(out[0].detach()[:, :, ::8, ::8].cpu().numpy(), g["recons_sub"], atol=TOL, rtol=0)
    losses = m.loss_function(*out, M_N=float(g["M_N"]))
    for k, v in losses.items():
        want = float(g["loss." + k])
        assert abs(float(v.detach()) - want) <= TOL * max(1.0, abs(want)), (k, float(v.detach()), want)
    m.zero_grad()
    losses["loss"].backward()
    np.testing.assert_allclose(m.ladders[0].fc_var.bias.grad.cpu().numpy(), g["grad.ladders.0.fc_var.bias"], atol=2e-7, rtol=2e-3)
    np.testing.assert_allclose(m.encoders[2].encoder_mu.bias.grad.cpu().numpy(), g["grad.encoders.2.encoder_mu.bias"], atol=2e-7, rtol=2e-3)
    for k, p in m.named_parameters():
        H.assert_cks_close(H.cks(p.grad), g["gradcks." + k], rtol=2e-3, atol=2e-5, what=k)
    for k, b in m.named_buffers():
        if "running" in k:
            H.assert_cks_close(H.cks(b), g["buf." + k], rtol=1e-4, atol=1e-5, what=k)
    assert m.sample(3, dev).shape == (3, 3, 64, 64)
    gen = torch.Generator().manual_seed(2)
    t = [torch.randn(9, 20, generator=gen).to(dev).requires_grad_(True) for _ in range(4)]
    e = torch.randn(9, 20, generator=gen).to(dev)
    wz, wk = torch.randn(9, 20, generator=gen).to(dev), torch.randn(9, generator=gen).to(dev)
    z, kl = K.LadderMerge.apply(*t, e)
    ((z * wz).sum() + (kl * wk).sum()).backward()
    t2 = [v.detach().clone().requires_grad_(True) for v in t]
    mu_e, lv_e, mu_t, lv_t = t2
    p1, p2 = 1. / (lv_e.exp() + 1e-7), 1. / (lv_t.exp() + 1e-7)
    mu_m, lv_m = (mu_e * p1 + mu_t * p2) / (p1 + p2), torch.log(1. / (p1 + p2))
    zr = e * torch.exp(0.5 * lv_m) + mu_m
    klr = torch.sum((lv_e - lv_m) + (lv_m.exp() + (mu_m - mu_e) ** 2) / (2 * lv_e.exp()) - 0.5, dim=-1)
    ((zr * wz).sum() + (klr * wk).sum()).backward()
    torch.testing.assert_close(z, zr, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(kl, klr, rtol=1e-5, atol=1e-4)
    for a, b2 in zip(t, t2):
        torch.testing.assert_close(a.grad, b2.grad, rtol=2e-4, atol=2e-5 * float(b2.grad.abs().max()))
