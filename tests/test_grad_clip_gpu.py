"""GPU: gradient clipping in front of the fused Adam step (Lightning's gradient_clip_val / gradient_clip_algorithm, which the
reference's Trainer applies with torch.nn.utils.clip_grad_norm_ / clip_grad_value_ before torch.optim.Adam).

The torch side is fed the product's own gradients at every step (teacher forcing), so only the clip and the Adam arithmetic
are compared.  It runs in fp64 on CPU copies, with the hyper-parameters the device state holds (fp32 values): torch's own fp32
norm sums in another order and is itself ~1e-5 off on a few million elements, so the fp64 run is the yardstick, and the bounds
are fp32 rounding, not bit equality.  Where the clip must not change anything (off, c == 1), the comparison is bitwise."""
import os

import pytest
import torch
import yaml

from ctvae_amd import filler
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA_CFG = dict(in_channels=3, latent_dim=128, gamma_shape=8., prior_shape=2., prior_rate=1.)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _gamma(dev, seed=1265):
    from ctvae_amd.models import vae_models
    m = vae_models["GammaVAE"](**GAMMA_CFG)
    m.load_state_dict(filler.fill_state(H.gamma_specs(), seed))
    return m.to(dev).train()


def _mcq(dev, seed=1320):
    from ctvae_amd.models import vae_models
    cfg = {**H.MCQ_CFG, "hidden_dims": list(H.MCQ_CFG["hidden_dims"])}    # the constructor reverses the list in place
    sd = filler.fill_state(H.mcq_specs(cfg), seed)
    m = vae_models["MCQVAE"](**cfg)
    m.load_state_dict(sd)
    return m.to(dev).train()


def _batches(dev, seed, n, B=8):
    return [filler.synthetic_batch(seed + i, B)[0].to(dev) for i in range(n)]


def _flat_view(m, p, buf):
    """p's elements in a buffer laid out like the flat parameter buffer (p is a strided view into it: packed conv weights)."""
    off = (p.data_ptr() - m.flat_params.data_ptr()) // 4
    return buf.as_strided(p.size(), p.stride(), buf.storage_offset() + off)


def _backward(exp, x, i):
    from ctvae_amd import kernels as K
    exp.model.zero_grad(lazy=True)
    loss = exp.training_step((x, torch.zeros(x.size(0), device=x.device)), i)
    K.backward(loss)
    exp.model.gather_torch_grads()


def _grad_norm64(m, prefix=None):
    return float(torch.sqrt(sum((_flat_view(m, p, m.flat_grads).double() ** 2).sum() for k, p in m.named_parameters()
                                if prefix is None or k.startswith(prefix + "."))))


def _assert_close_ulp(got, want, lr, what):
    """Parameters: within 1e-3 * lr plus 2 ulp of |p|, elementwise."""
    a = want.abs().float()
    ulp = (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).to(want.dtype)      # fp32 ulp
    err = (got - want).abs()
    bad = err > 1e-3 * lr + 2 * ulp
    assert not bool(bad.any()), (what, float(err.max()), int(bad.sum()))


def _f32(x):
    """x as the fp32 device state holds it, back in a Python float."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _torch_adam64(params, lr, wd):
    return torch.optim.Adam(params, lr=_f32(lr), betas=(_f32(0.9), _f32(0.999)), eps=_f32(1e-8), weight_decay=_f32(wd))


def _assert_close_moment(got, want, what):
    scale = float(want.abs().max())
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6 * scale + 1e-30, msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("algorithm", ["norm", "value"])
def test_clip_matches_torch_over_three_steps(dev, algorithm):
    """GammaVAE at B = 8, three steps on different batches, clip active in every step: FlatAdam's pre-clip norm, moments and
    parameters against clip_grad_norm_ / clip_grad_value_ + torch.optim.Adam on CPU copies fed the same gradients."""
    from ctvae_amd.experiment import VAEXperiment
    lr, wd = 0.003, 5e-5
    xs = _batches(dev, 900, 3)
    probe = VAEXperiment(_gamma(dev), {"LR": lr, "weight_decay": wd, "kld_weight": 0.00025, "hipgraph": False})
    _backward(probe, xs[0], 0)
    if algorithm == "norm":
        clip = _f32(0.25 * _grad_norm64(probe.model))            # well below the norm of every step (asserted below)
    else:
        clip = _f32(torch.quantile(probe.model.flat_grads.abs()[:1 << 20].cpu(), 0.9))
    del probe
    m = _gamma(dev)
    exp = VAEXperiment(m, {"LR": lr, "weight_decay": wd, "kld_weight": 0.00025, "hipgraph": False},
                       gradient_clip_val=clip, gradient_clip_algorithm=algorithm)
    opt = exp.optimizer
    assert (opt.grad_norm is not None) == (algorithm == "norm")
    named = list(m.named_parameters())
    cpu = {k: torch.nn.Parameter(p.detach().cpu().double()) for k, p in named}
    topt = _torch_adam64(list(cpu.values()), lr, wd)
    for i, x in enumerate(xs):
        _backward(exp, x, i)
        for k, p in named:
            cpu[k].grad = _flat_view(m, p, m.flat_grads).detach().cpu().double()
        if algorithm == "norm":
            ref_norm = float(torch.nn.utils.clip_grad_norm_(list(cpu.values()), clip))
            assert ref_norm > clip, (ref_norm, clip)
        else:
            assert any(bool((g.grad.abs() > clip).any()) for g in cpu.values())
            torch.nn.utils.clip_grad_value_(list(cpu.values()), clip)
        topt.step()
        exp.optimizer_step()
        torch.cuda.synchronize()
        if algorithm == "norm":
            assert abs(float(opt.grad_norm) - ref_norm) <= 1e-5 * ref_norm, (float(opt.grad_norm), ref_norm)
        for k, p in named:
            st = topt.state[cpu[k]]
            _assert_close_moment(_flat_view(m, p, opt.exp_avg).cpu().double(), st["exp_avg"], f"step {i} exp_avg {k}")
            _assert_close_moment(_flat_view(m, p, opt.exp_avg_sq).cpu().double(), st["exp_avg_sq"], f"step {i} exp_avg_sq {k}")
            _assert_close_ulp(p.detach().cpu().double(), cpu[k].detach(), lr, f"step {i} param {k}")
    assert float(opt.state[0]) == 3.0


def test_clip_off_and_inactive_are_bit_identical(dev):
    """gradient_clip_val None / 0 runs today's single adam_kernel launch and nothing else; an inactive clip (c == 1, value
    far above every gradient) runs the clip kernels and still steps bit for bit like adam_kernel (weight decay on)."""
    from ctvae_amd import native
    from ctvae_amd.optim import FlatAdam
    from ctvae_amd.experiment import VAEXperiment
    m = _mcq(dev)
    exp = VAEXperiment(m, {"LR": 0.0005, "kld_weight": 0.00025, "hipgraph": False})
    grads = []
    for i, x in enumerate(_batches(dev, 300, 3)):
        _backward(exp, x, i)
        grads.append(m.flat_grads.clone())
    p0 = m.flat_params.clone()

    def run(record=False, **clip):
        m.flat_params.copy_(p0)
        opt = FlatAdam(m, lr=0.0005, weight_decay=1e-3, **clip)
        torch.cuda.synchronize()
        native.prof_enable(record)
        try:
            for g in grads:
                m.flat_grads.copy_(g)
                opt.step()
            torch.cuda.synchronize()
        finally:
            native.prof_enable(False)
        rep = native.prof_report() if record else {}
        return m.flat_params.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt, rep

    base = run(record=True)
    assert set(base[4]) == {"adam_kernel"}, sorted(base[4])
    for clip in ({"clip_val": None}, {"clip_val": 0}, {"clip_val": 0.0, "clip_algorithm": "value"}):
        got = run(record=True, **clip)
        assert set(got[4]) == {"adam_kernel"}, (clip, sorted(got[4]))
        for a, b in zip(got[:3], base[:3]):
            assert torch.equal(a, b), clip
    got = run(record=True, clip_val=1e30)
    assert set(got[4]) == {"grad_sqnorm_kernel", "adam_clip_kernel"}, sorted(got[4])
    for a, b in zip(got[:3], base[:3]):
        assert torch.equal(a, b)
    want = float(grads[-1].double().norm())
    assert abs(float(got[3].grad_norm) - want) <= 1e-5 * want, (float(got[3].grad_norm), want)
    assert set(run(record=True, clip_val=1e30, clip_algorithm="value")[4]) == {"adam_clip_kernel"}


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_inactive_norm_clip_reproduces_adam_kernel_on_every_path(dev, grad_scale):
    """c == 1: the 16-byte loop, its scalar tail (n % 4 == 3) and the unaligned kernel (offset 1) all step bit for bit like
    ctvae_adam_step, weight decay on, over three steps."""
    from ctvae_amd import kernels as K
    n = 10007
    gen = torch.Generator().manual_seed(11)
    p0 = torch.randn(n, generator=gen)
    gs = [torch.randn(n, generator=gen) * 1e-2 for _ in range(3)]
    for offset in (0, 1):
        out = []
        for clipped in (False, True):
            bufs = [torch.zeros(n + offset, device=dev) for _ in range(4)]
            p, g, mo, v = (b[offset:] for b in bufs)
            p.copy_(p0)
            state = K.adam_state([0.0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 1.0], dev)
            ws, norm = K.grad_clip_workspace(dev), torch.zeros((), device=dev)
            for gk in gs:
                g.copy_(gk)
                if clipped:
                    K.adam_step_clipped(p, g, mo, v, state, grad_scale, "norm", 1e30, ws, norm)
                else:
                    K.adam_step(p, g, mo, v, state, grad_scale)
            torch.cuda.synchronize()
            out.append([t.cpu() for t in (p, mo, v, state[:8])])
        for a, b in zip(*out):
            assert torch.equal(a, b), offset


def test_hipgraph_clipped_training_matches_eager(dev):
    """test_harness_hipgraph_training_matches_eager with an active norm clip: MCQVAE, 7 batches, 3 eager steps then graph
    replays that include the squared-norm pass -- bit-equal to the eager run, and different from the unclipped run."""
    from ctvae_amd.experiment import VAEXperiment
    batches = [(filler.synthetic_batch(500 + i, 8)[0].to(dev), torch.zeros(8, device=dev)) for i in range(7)]
    finals = {}
    for use_graph, clip in ((False, 1e-3), (True, 1e-3), (False, None)):
        m = _mcq(dev, 501)
        exp = VAEXperiment(m, {"LR": 0.0005, "weight_decay": 0.0, "scheduler_gamma": 0.95, "kld_weight": 0.00025,
                               "hipgraph": use_graph}, gradient_clip_val=clip)
        exp.fit(lambda: iter(batches), None, max_epochs=1)
        torch.cuda.synchronize()
        assert exp.global_step == len(batches)
        if use_graph:
            assert any(g.graph is not None for g in exp._graphed.values()), "no hipGraph was captured"
        if clip is not None:
            assert float(exp.optimizer.grad_norm) > clip, float(exp.optimizer.grad_norm)
        finals[(use_graph, clip)] = m.flat_params.clone()
    assert torch.equal(finals[(False, 1e-3)], finals[(True, 1e-3)])
    assert not torch.equal(finals[(False, 1e-3)], finals[(False, None)])


def test_update_parameters_clips_that_slice_only(dev):
    """exp_params.update_parameters (the optimizer covers one sub-module): the norm is torch's norm over that sub-module's
    gradients, and gradients outside the slice neither change the clip coefficient nor get stepped."""
    from ctvae_amd.experiment import VAEXperiment
    params = {"LR": 0.0005, "kld_weight": 0.00025, "update_parameters": "decoder", "hipgraph": False}
    m = _mcq(dev)
    p0 = m.flat_params.clone()
    exp = VAEXperiment(m, params, gradient_clip_val=1e-3)
    _backward(exp, _batches(dev, 77, 1)[0], 0)
    g = m.flat_grads.clone()
    sl = exp.optimizer.slice
    assert 0 < sl.start < sl.stop <= g.numel()
    dec = []
    for k, p in m.named_parameters():
        if k.startswith("decoder."):
            dec.append(torch.nn.Parameter(p.detach().cpu().double()))
            dec[-1].grad = _flat_view(m, p, g).cpu().double()
    ref_norm = float(torch.nn.utils.clip_grad_norm_(dec, 1e-3))
    whole = _grad_norm64(m)
    exp.optimizer_step()
    torch.cuda.synchronize()
    assert ref_norm > 1e-3
    assert abs(float(exp.optimizer.grad_norm) - ref_norm) <= 1e-5 * ref_norm, (float(exp.optimizer.grad_norm), ref_norm)
    assert abs(whole - ref_norm) > 1e-4 * whole, "the whole model's norm would not tell the slice's apart"
    first = m.flat_params.clone()
    assert torch.equal(first[:sl.start], p0[:sl.start]) and torch.equal(first[sl.stop:], p0[sl.stop:])
    # same slice gradients, huge gradients everywhere else: the same step, bit for bit
    m.flat_params.copy_(p0)
    exp2 = VAEXperiment(m, params, gradient_clip_val=1e-3)
    g2 = torch.randn(g.numel(), device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 1e3
    g2[sl] = g[sl]
    m.flat_grads.copy_(g2)
    exp2.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(m.flat_params, first)
    assert torch.equal(exp2.optimizer.grad_norm, exp.optimizer.grad_norm)


def _raw_step(dev, p, g, algorithm, clip, wd, offset=0):
    """One ctvae_adam_step_clipped on copies of p / g placed `offset` floats into fresh buffers (offset 1: the scalar paths)."""
    from ctvae_amd import kernels as K
    n = p.numel()
    bufs = [torch.zeros(n + offset, dtype=torch.float32, device=dev) for _ in range(4)]
    pd, gd, md, vd = (b[offset:] for b in bufs)
    pd.copy_(p)
    gd.copy_(g)
    state = K.adam_state([0.0, 1e-3, 0.9, 0.999, 1e-8, wd, 1.0, 1.0], dev)
    ws = K.grad_clip_workspace(dev)
    norm = torch.full((), -1.0, device=dev)
    K.adam_step_clipped(pd, gd, md, vd, state, 1.0, algorithm, clip, ws, norm)
    torch.cuda.synchronize()
    return pd.cpu(), md.cpu(), vd.cpu(), norm.cpu()


def _torch_step(p, g, algorithm, clip, wd):
    q = torch.nn.Parameter(p.clone())
    q.grad = g.clone()
    norm = None
    if algorithm == "norm":
        norm = torch.nn.utils.clip_grad_norm_([q], clip)
    else:
        torch.nn.utils.clip_grad_value_([q], clip)
    opt = torch.optim.Adam([q], lr=1e-3, weight_decay=wd)
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"], norm


@pytest.mark.parametrize("algorithm,bad", [("norm", float("nan")), ("value", float("nan")), ("norm", float("inf"))])
def test_nonfinite_gradient_matches_torch(dev, algorithm, bad):
    """A NaN in norm mode makes every updated element NaN; in value mode only that element.  An inf in norm mode gives
    c = 0: every other element steps with a zero gradient and the inf element becomes NaN (inf * 0).  As torch does."""
    n, j = 10007, 4321
    gen = torch.Generator().manual_seed(3)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    g[j] = bad
    want = _torch_step(p, g, algorithm, 0.5, 0.0)
    for offset in (0, 1):
        got = _raw_step(dev, p, g, algorithm, 0.5, 0.0, offset)
        for a, b, what in zip(got[:3], want[:3], ("param", "exp_avg", "exp_avg_sq")):
            assert torch.equal(torch.isnan(a), torch.isnan(b)), (what, offset, int(torch.isnan(a).sum()), int(torch.isnan(b).sum()))
            fin = ~torch.isnan(b)
            torch.testing.assert_close(a[fin], b[fin], rtol=1e-5, atol=1e-7)
        nan_count = int(torch.isnan(got[0]).sum())
        if algorithm == "norm" and bad != bad:
            assert nan_count == n
        else:
            assert nan_count == 1 and bool(torch.isnan(got[0][j]))
        if algorithm == "norm" and bad == float("inf"):
            keep = torch.ones(n, dtype=torch.bool)
            keep[j] = False
            assert torch.equal(got[0][keep], p[keep]) and float(got[3]) == float("inf")


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4097, (1 << 20) + 3, 3_900_001])
def test_grad_norm_matches_fp64_and_ignores_alignment(dev, n):
    """The pre-clip norm against an fp64 norm, and bit-identical whether the buffers are 16-byte aligned (vector paths) or
    not (scalar paths): the reduction order is a function of n alone.  (The update itself joins the weight decay with the
    roundings of adam_kernel's path, so aligned and unaligned steps agree to fp32 rounding.)"""
    gen = torch.Generator().manual_seed(n)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 3
    aligned = _raw_step(dev, p, g, "norm", 1e-3, 1e-2, 0)
    again = _raw_step(dev, p, g, "norm", 1e-3, 1e-2, 0)
    shifted = _raw_step(dev, p, g, "norm", 1e-3, 1e-2, 1)
    want = float(g.double().norm())
    assert abs(float(aligned[3]) - want) <= 1e-5 * want, (float(aligned[3]), want)
    assert torch.equal(aligned[3], again[3]) and torch.equal(aligned[3], shifted[3])
    for a, b in zip(aligned[:3], shifted[:3]):
        _assert_close_moment(a, b, "aligned against unaligned")
    ref = _torch_step(p, g, "norm", 1e-3, 1e-2)
    _assert_close_moment(aligned[1], ref[1], "exp_avg")


def _runner_cfg(tmp_path, sub, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "gammavae.yaml")))
    cfg["logging_params"]["save_dir"] = str(tmp_path / sub)
    cfg["data_params"]["train_batch_size"] = 8
    cfg["data_params"]["val_batch_size"] = 8
    for k, v in trainer.items():
        if v is None:
            cfg["trainer_params"].pop(k, None)
        else:
            cfg["trainer_params"][k] = v
    p = tmp_path / f"{sub}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_honours_gradient_clip_val(dev, tmp_path):
    """configs/gammavae.yaml carries gradient_clip_val: 0.8 (as the reference's does): run.main trains with it -- the
    parameters differ from the same run with the key removed -- and an unknown algorithm is refused before any step."""
    from ctvae_amd import run
    assert yaml.safe_load(open(os.path.join(ROOT, "configs", "gammavae.yaml")))["trainer_params"]["gradient_clip_val"] == 0.8
    last = lambda sub: tmp_path / sub / "GammaVAE" / "checkpoints" / "last.ckpt"
    args = ["--steps-per-epoch", "4", "--max-epochs", "1"]
    run.main(["-c", _runner_cfg(tmp_path, "clip")] + args)
    run.main(["-c", _runner_cfg(tmp_path, "plain", gradient_clip_val=None)] + args)
    a = torch.load(last("clip"), weights_only=True)["state_dict"]
    b = torch.load(last("plain"), weights_only=True)["state_dict"]
    assert any(not torch.equal(v, b[k]) for k, v in a.items() if k.endswith("weight"))
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        run.main(["-c", _runner_cfg(tmp_path, "bad", gradient_clip_algorithm="l1")] + args)
    assert not last("bad").exists()
