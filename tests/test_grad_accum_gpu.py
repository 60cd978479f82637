"""GPU: ``accumulate_grad_batches`` through the training harness (experiment.py, optim.py): a window of k micro-batches steps
once, on (sum of the micro-batches' gradients) / k.

VanillaVAE (latent_dim 128) at B = 4 unless stated.  The hand-made side of a comparison ("route B") runs the harness's own
backward pieces, sums the micro-batches' flat gradients with torch's fp32 add and calls ``FlatAdam.step(grad_scale=1 / k)``:
both sides run the same kernels on the same values in the same order, so the comparisons are bitwise.  The CT-MCQ-VAE case
compares with ``torch.optim.Adam`` under the bounds of tests/test_adam_blocks_ct_gpu.py."""
import os

import pytest
import torch
import yaml

from ctvae_amd import filler
from ctvae_amd import specs
from tests.test_adam_blocks_ct_gpu import A, LR, PARAMS, WD, _layout, _model as _ct_model, fixed_noise  # noqa: F401
from tests.test_adam_blocks_gpu import _assert_close_moment, _assert_close_ulp, _f32
from tests.test_adam_blocks_host import expected_active

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4
EXP = {"LR": 0.005, "weight_decay": 1e-4, "kld_weight": 0.00025}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _vanilla(dev, seed=1266):
    """The same weights, BatchNorm statistics and in-kernel noise state on every call."""
    from ctvae_amd.models import vae_models
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
    m.load_state_dict(filler.fill_state(specs.vanilla_specs(), seed))
    m = m.to(dev).train()
    m._rng_state = torch.tensor([987654321, 0], dtype=torch.int64, device=dev)
    return m


def _batches(dev, n, seed=4100):
    return [(filler.synthetic_batch(seed + i, B)[0].to(dev), torch.zeros(B, device=dev)) for i in range(n)]


def _backward(exp, batch, i):
    """One micro-batch's gradients into the flat buffer, by the eager branch's own pieces; returns a copy of the buffer."""
    from ctvae_amd import kernels as K
    exp.model.zero_grad(lazy=True)
    K.backward(exp.training_step(batch, i))
    exp.model.gather_torch_grads()
    return exp.model.flat_grads.clone()


def _snapshot(exp):
    torch.cuda.synchronize()
    m, opt = exp.model, exp.optimizer
    out = {"param": m.flat_params.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(),
           "state": opt.state[:8].clone()}
    for k, b in m.named_buffers():
        out["buffer " + k] = b.clone()
    return out


def _assert_same(a, b, what):
    assert sorted(a) == sorted(b)
    assert any(k.endswith("running_mean") for k in a) and any(k.endswith("num_batches_tracked") for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k, float((a[k].double() - b[k].double()).abs().max()))


def _hand_made_window(exp, batches, first_index, k):
    """Route B: the window's micro-batches one by one, the flat gradient buffer set to their sum, one step at 1 / k."""
    gs = [_backward(exp, b, first_index + j) for j, b in enumerate(batches)]
    total = gs[0]
    for g in gs[1:]:
        total = total + g
    exp.model.flat_grads.copy_(total)
    exp.optimizer.step(grad_scale=1.0 / k)
    exp.global_step += 1


@pytest.mark.parametrize("hipgraph", [False, True])
def test_window_equals_hand_made_step(dev, hipgraph):
    """fit() over (a, b) with k = 2 against: backward a, backward b, flat_grads = g_a + g_b, FlatAdam.step(grad_scale=0.5).
    Parameters, both moments, the step counter and the BatchNorm running statistics, bit for bit.  (With ``hipgraph`` on, the two
    batches are the signature's eager warm-up steps: the captured branch's code, nothing replayed yet.)"""
    from ctvae_amd.experiment import VAEXperiment
    ab = _batches(dev, 2)
    exp_a = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=hipgraph), accumulate_grad_batches=2)
    hist = exp_a.fit(lambda: iter(ab), None, max_epochs=1)
    assert exp_a.global_step == 1 and hist[0]["train_images"] == 2 * B
    exp_b = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False))
    p0 = exp_b.model.flat_params.clone()
    _hand_made_window(exp_b, ab, 0, 2)
    a, b = _snapshot(exp_a), _snapshot(exp_b)
    _assert_same(a, b, "k = 2 window")
    assert float(a["state"][0]) == 1.0 and not torch.equal(a["param"], p0)


def test_incomplete_last_window_steps_at_one_over_k(dev):
    """Five batches, k = 2: three optimizer steps, and the third is batch 5 alone at grad_scale 0.5 -- not 1."""
    from ctvae_amd.experiment import VAEXperiment
    five = _batches(dev, 5)
    exp_a = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False), accumulate_grad_batches=2)
    exp_a.fit(lambda: iter(five), None, max_epochs=1)
    assert exp_a.global_step == 3 and float(exp_a.optimizer.state[0]) == 3.0
    assert exp_a.optimizer.stashed == 0
    finals = {}
    for scale in (0.5, 1.0):
        exp_b = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False), accumulate_grad_batches=2)
        exp_b.fit(lambda: iter(five[:4]), None, max_epochs=1)
        assert exp_b.global_step == 2
        assert exp_b.scheduler is None           # (the epoch end behind the four batches did not move the learning rate)
        _backward(exp_b, five[4], 4)
        exp_b.optimizer.step(grad_scale=scale)
        finals[scale] = _snapshot(exp_b)
    a = _snapshot(exp_a)
    _assert_same(a, finals[0.5], "third step")
    assert not torch.equal(a["param"], finals[1.0]["param"]), "a step at grad_scale 1 would not tell the two apart"


@pytest.mark.parametrize("algorithm", ["norm", "value"])
def test_clipping_applies_once_to_the_window_gradient(dev, algorithm):
    """gradient_clip_val on (g_a + g_b) / 2: grad_norm and everything the step writes equal route B's under the same setting."""
    from ctvae_amd.experiment import VAEXperiment
    ab = _batches(dev, 2)
    probe = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False))
    g = (_backward(probe, ab[0], 0) + _backward(probe, ab[1], 1)) * 0.5
    if algorithm == "norm":
        clip = _f32(0.25 * float(g.double().norm()))
    else:
        clip = _f32(torch.quantile(g.abs()[:1 << 20].cpu(), 0.9))
    assert clip > 0
    del probe
    kw = dict(gradient_clip_val=clip, gradient_clip_algorithm=algorithm)
    exp_a = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False), accumulate_grad_batches=2, **kw)
    exp_a.fit(lambda: iter(ab), None, max_epochs=1)
    exp_b = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False), **kw)
    _hand_made_window(exp_b, ab, 0, 2)
    _assert_same(_snapshot(exp_a), _snapshot(exp_b), algorithm)
    g = exp_b.model.flat_grads * 0.5                   # what the clip saw
    if algorithm == "norm":
        assert torch.equal(exp_a.optimizer.grad_norm, exp_b.optimizer.grad_norm)
        want = float(g.double().norm())
        assert want > clip and abs(float(exp_a.optimizer.grad_norm) - want) <= 1e-5 * want
    else:
        assert bool((g.abs() > clip).any()) and bool((g.abs() < clip).any())
    plain = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False), accumulate_grad_batches=2)
    plain.fit(lambda: iter(ab), None, max_epochs=1)
    assert not torch.equal(plain.model.flat_params, exp_a.model.flat_params), "the clip did not act"


def test_captured_equals_eager(dev):
    """k = 2 over 2 * (WARM + 2) batches: the signature's graph (which ends behind gather_torch_grads) is captured at the
    fourth micro-batch and serves both positions of the later windows; the stash / step launches follow the replay eagerly."""
    from ctvae_amd.experiment import VAEXperiment, _GraphedTrainStep
    batches = _batches(dev, 2 * (_GraphedTrainStep.WARM + 2))
    finals = {}
    for hipgraph in (False, True):
        exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=hipgraph), accumulate_grad_batches=2)
        exp.fit(lambda: iter(batches), None, max_epochs=1)
        assert exp.global_step == len(batches) // 2
        if hipgraph:
            gs = list(exp._graphed.values())
            assert len(gs) == 1 and gs[0].graph is not None and gs[0].seen == len(batches)
        finals[hipgraph] = _snapshot(exp)
    _assert_same(finals[False], finals[True], "captured against eager")


def test_k1_is_the_unchanged_path(dev):
    """accumulate_grad_batches: 1 and no key at all: the same four steps bit for bit, no accumulator, and no accumulation
    launch in the library's launch log -- while k = 2 shows one "store" and one "finish" launch per window there."""
    from ctvae_amd import native
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, 4)
    finals, reports = {}, {}
    for name, kw in (("none", {}), ("one", {"accumulate_grad_batches": 1}), ("two", {"accumulate_grad_batches": 2})):
        exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False), **kw)
        torch.cuda.synchronize()
        native.prof_enable(True)
        try:
            exp.fit(lambda: iter(batches), None, max_epochs=1)
            torch.cuda.synchronize()
        finally:
            native.prof_enable(False)
        reports[name] = native.prof_report()
        finals[name] = _snapshot(exp)
        assert (exp.optimizer.acc is None) == (name != "two")
        assert exp.global_step == (2 if name == "two" else 4)
    _assert_same(finals["none"], finals["one"], "k = 1")
    for name in ("none", "one"):
        assert reports[name]["adam_kernel"]["count"] == 4
        assert not [k for k in reports[name] if k.startswith("grad_accumulate")], sorted(reports[name])
    assert sorted(reports["none"]) == sorted(reports["one"])
    assert {k: v["count"] for k, v in reports["none"].items()} == {k: v["count"] for k, v in reports["one"].items()}
    assert reports["two"]["grad_accumulate_kernel"]["count"] == 4 and reports["two"]["adam_kernel"]["count"] == 2


# ---- skip modes across the modes of CT-MCQ-VAE -----------------------------------------------------------
# (mode, action ids of the 4 pairs).  WITH_CAUSAL is the window the feature is for: one micro-batch of every mode.  A
# causal-mode micro-batch evaluates every scorer on every sample (tests/test_adam_blocks_host.expected_active), so in such a
# window no member of graph_discovers is left without a gradient; the only block that never steps there is a_dense.  The
# members whose action is absent from the action micro-batch (all but 0 and 3) are hit in ONE micro-batch per window, the
# causal one.  NO_CAUSAL (base + action + action) has what the first cannot have: members hit in no micro-batch (every scorer
# but 0, 1, 4 and 8), members hit in one micro-batch per window only (1: action 0, 8: action 7) and one hit in two (4: action 3).
WITH_CAUSAL = [("base", None), ("action", [0, 3, 0, 3]), ("causal", [1, 5, 2, 9])]
NO_CAUSAL = [("base", None), ("action", [0, 3, 0, 3]), ("action", [3, 7, 7, 3])]


def _ct_batches(dev, window, rounds=2):
    out = []
    for i, (mode, actions) in enumerate(window * rounds):
        x, y, _ = filler.synthetic_pairs(300 + i, B, A)
        opts = {"mode": [mode] * B}
        if mode != "base":
            opts.update(input_y=y.to(dev), action=torch.nn.functional.one_hot(torch.tensor(actions), A).float().to(dev))
        out.append((x.to(dev), torch.zeros(B, device=dev), opts))
    return out


def _ct_windows(dev, absent, window):
    """Two windows of k = 3 through the harness's own step pieces (window_step), keeping every micro-batch's slice gradients."""
    from ctvae_amd import kernels as K
    from ctvae_amd.experiment import VAEXperiment
    m = _ct_model(dev)
    exp = VAEXperiment(m, dict(PARAMS, hipgraph=False, adam_absent_grad=absent), accumulate_grad_batches=3)
    opt = exp.optimizer
    p0 = m.flat_params[opt.slice].clone()
    grads = []
    for i, batch in enumerate(_ct_batches(dev, window)):
        m.zero_grad(lazy=True)
        K.backward(exp.training_step(batch, i % 3))
        grads.append(m.flat_grads[opt.slice].clone())
        exp.window_step(i % 3 == 2)
    torch.cuda.synchronize()
    return m, opt, p0, grads


def _window_active(name, window):
    return any(expected_active(name, mode, actions or []) for mode, actions in window)


@pytest.mark.parametrize("window", [WITH_CAUSAL, NO_CAUSAL], ids=["base-action-causal", "base-action-action"])
def test_skip_steps_blocks_active_anywhere_in_the_window(dev, fixed_noise, window):
    """adam_absent_grad: skip, k = 3, two windows.  A block's counter is 2 iff some micro-batch of the window gave it a
    gradient, else 0; the trajectory is torch.optim.Adam's on clones whose .grad is (sum of the window's gradients) / 3 where a
    gradient is present and None where it is absent."""
    m, opt, p0, grads = _ct_windows(dev, "skip", window)
    spans, by_lo = _layout(m, opt)
    names = [by_lo[b[0]] for b in opt.blocks]
    active = {k: _window_active(k, window) for k in spans}
    steps = dict(zip(names, opt.block_steps().cpu().tolist()))
    assert steps == {k: 2.0 if active[k] else 0.0 for k in spans}, [k for k in spans if steps[k] != 2.0 * active[k]]
    assert steps["a_dense.weight"] == 0.0 and steps["graph_discovers.0.0.weight"] == 2.0 and steps["mask.0.weight"] == 2.0
    if window is NO_CAUSAL:
        assert steps["graph_discovers.2.0.weight"] == 0.0 and steps["graph_discovers.12.2.bias"] == 0.0      # never hit
        assert steps["graph_discovers.1.0.weight"] == 2.0 and steps["graph_discovers.8.2.bias"] == 2.0       # one micro-batch
        assert sum(1 for k in spans if k.startswith("graph_discovers.") and not active[k]) == 4 * (A + 1 - 4)
    else:
        assert steps["graph_discovers.8.2.bias"] == 2.0                    # the causal micro-batch alone
        assert all(active[k] for k in spans if k.startswith("graph_discovers."))
    ref = {k: torch.nn.Parameter(p0[lo:hi].cpu().double()) for k, (lo, hi) in spans.items()}
    topt = torch.optim.Adam(list(ref.values()), lr=_f32(LR), betas=(_f32(0.9), _f32(0.999)), eps=_f32(1e-8), weight_decay=_f32(WD))
    for w in range(2):
        total = sum(g.cpu().double() for g in grads[3 * w:3 * w + 3]) / 3
        for k, (lo, hi) in spans.items():
            if active[k]:
                ref[k].grad = total[lo:hi].clone()
            else:
                assert not bool(total[lo:hi].any()), f"window {w}: {k} should have no gradient"
                ref[k].grad = None
        topt.step()
    after = m.flat_params[opt.slice]
    for k, (lo, hi) in spans.items():
        if not active[k]:
            assert torch.equal(p0[lo:hi], after[lo:hi]) and not bool(opt.exp_avg[lo:hi].any()), k
            continue
        st = topt.state[ref[k]]
        _assert_close_moment(opt.exp_avg[lo:hi].cpu().double(), st["exp_avg"], k + " exp_avg")
        _assert_close_moment(opt.exp_avg_sq[lo:hi].cpu().double(), st["exp_avg_sq"], k + " exp_avg_sq")
        _assert_close_ulp(after[lo:hi].cpu().double(), ref[k].detach(), LR, k + " param")


@pytest.mark.parametrize("window", [WITH_CAUSAL, NO_CAUSAL], ids=["base-action-causal", "base-action-action"])
def test_skip_until_first_counters_over_two_windows(dev, fixed_noise, window):
    """Both windows have the same activity, so "has stepped before" adds nothing: the counters are skip's."""
    m, opt, _, _ = _ct_windows(dev, "skip_until_first", window)
    spans, by_lo = _layout(m, opt)
    steps = dict(zip([by_lo[b[0]] for b in opt.blocks], opt.block_steps().cpu().tolist()))
    assert steps == {k: 2.0 if _window_active(k, window) else 0.0 for k in spans}


def test_skip_until_first_keeps_stepping_after_the_merge(dev, fixed_noise):
    """Window 1 = NO_CAUSAL (scorers 1, 4, 8 and 0 step), window 2 = base x 3 (of the scorers only 0 has a gradient, the mask
    network none): under skip_until_first the blocks of window 1 step again -- the rule is applied behind the window's merge."""
    from ctvae_amd.experiment import VAEXperiment
    finals = {}
    for absent in ("skip", "skip_until_first"):
        m = _ct_model(dev)
        exp = VAEXperiment(m, dict(PARAMS, hipgraph=False, adam_absent_grad=absent), accumulate_grad_batches=3)
        batches = _ct_batches(dev, NO_CAUSAL, 1) + _ct_batches(dev, [("base", None)] * 3, 1)
        exp.fit(lambda: iter(batches), None, max_epochs=1)
        torch.cuda.synchronize()
        assert exp.global_step == 2
        spans, by_lo = _layout(m, exp.optimizer)
        finals[absent] = dict(zip([by_lo[b[0]] for b in exp.optimizer.blocks], exp.optimizer.block_steps().cpu().tolist()))
    for k, n in finals["skip"].items():
        first = _window_active(k, NO_CAUSAL)
        second = expected_active(k, "base", [])
        assert n == float(first) + float(second), k
        assert finals["skip_until_first"][k] == float(first) + float(first or second), k
    assert finals["skip"]["mask.0.weight"] == 1.0 and finals["skip_until_first"]["mask.0.weight"] == 2.0


# ---- the runner -------------------------------------------------------------------------------------------
def _runner_cfg(tmp_path, sub, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "vae.yaml")))
    cfg["logging_params"]["save_dir"] = str(tmp_path / sub)
    cfg["data_params"]["train_batch_size"] = B
    cfg["data_params"]["val_batch_size"] = B
    cfg["trainer_params"].update(trainer)
    p = tmp_path / f"{sub}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_honours_accumulate_grad_batches(dev, tmp_path):
    """run.main on synthetic data, 6 batches per epoch, accumulate_grad_batches: 2 -> 3 optimizer steps in the checkpoint's
    trainer entry (a runner that ignores the key leaves 6); a refused value is a SystemExit that names the key."""
    from ctvae_amd import run
    args = ["--steps-per-epoch", "6", "--max-epochs", "1"]
    run.main(["-c", _runner_cfg(tmp_path, "acc", accumulate_grad_batches=2)] + args)
    ckpt = torch.load(tmp_path / "acc" / "VanillaVAE" / "checkpoints" / "last.ckpt", weights_only=True)
    assert ckpt["trainer"]["global_step"] == 3 and ckpt["global_step"] == 3
    assert float(ckpt["trainer"]["optimizer"]["state"][0]) == 3.0
    for bad in (0, 2.0, True, {0: 2}):
        with pytest.raises(SystemExit, match="accumulate_grad_batches"):
            run.main(["-c", _runner_cfg(tmp_path, "bad", accumulate_grad_batches=bad)] + args)
    assert not (tmp_path / "bad" / "VanillaVAE" / "checkpoints" / "last.ckpt").exists()
