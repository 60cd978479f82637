"""GPU: gradient tracking through the training harness (experiment.py, optim.py: GradientTracker) -- ``track_grad_norm`` and
``watch_gradients`` measure the gradient an optimizer step was handed, and leave the run as it is.

VanillaVAE (latent_dim 128) at B = 4 as tests/test_grad_accum_gpu.py builds it, and the CT-MCQ-VAE of
tests/test_adam_blocks_ct_gpu.py (action_dim 12, ``update_parameters: ct_layer``).  The expected values come from ``.grad`` views
read by torch on the CPU in float64 and from ``torch.histc``; the norm bound is the kernels' own (relative 1e-6,
tests/test_grad_stats_ops_gpu.py) next to the 4 decimals the record is rounded to."""
import json
import math
import os

import pytest
import torch
import yaml

from ctvae_amd import filler
from tests.test_adam_blocks_ct_gpu import PARAMS, _batches as _ct_batches, _model as _ct_model, fixed_noise  # noqa: F401
from tests.test_adam_blocks_host import SEQUENCE, expected_active
from tests.test_grad_accum_gpu import B, EXP, _backward, _batches, _runner_cfg, _snapshot, _vanilla

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


def _want_norms(model, scale, p, names=None):
    """{name: float64 p-norm of fl32(.grad * scale)} from the parameters' own views of the flat gradient buffer."""
    out = {}
    for name, prm in model.named_parameters():
        if names is not None and name not in names:
            continue
        v = (prm.grad.detach().float() * torch.tensor(scale, dtype=torch.float32)).cpu().double().reshape(-1)
        out[name] = float(v.abs().max()) if math.isinf(p) else float(v.norm(p))
    return out


def _assert_norm_record(rec, want, p, step):
    stem = f"grad_{float(p)}_norm"
    assert rec["step"] == step
    keys = {k for k in rec if k.startswith(stem + "/")}
    assert keys == {f"{stem}/model.{k}" for k in want}, keys ^ {f"{stem}/model.{k}" for k in want}
    for k, w in want.items():
        got = rec[f"{stem}/model.{k}"]
        assert got == round(got, 4)
        assert abs(got - w) <= 0.5e-4 + 1e-6 * w, (k, got, w)
    vals = torch.tensor([rec[f"{stem}/model.{k}"] for k in want], dtype=torch.float64)
    total = float(vals.abs().max()) if math.isinf(p) else float(torch.tensor(list(want.values()), dtype=torch.float64).norm(p))
    assert abs(rec[f"{stem}_total"] - total) <= 0.5e-4 + 1e-6 * total, (rec[f"{stem}_total"], total)


# ---- the run is untouched ------------------------------------------------------------------------------------
@pytest.mark.parametrize("hipgraph", [False, True])
def test_tracking_on_equals_off(dev, hipgraph):
    """Six steps (three eager, three replayed when ``hipgraph`` is on), tracking every step against no tracking: parameters, both
    moments, Adam's state, the BatchNorm buffers, the in-kernel noise state and torch's generators, bit for bit."""
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, 6)
    finals = {}
    for on in (False, True):
        torch.manual_seed(5)
        kw = dict(track_grad_norm=2, watch_gradients=True, watch_log_freq=2, log_every=1) if on else dict(log_every=1)
        exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=hipgraph), **kw)
        exp.fit(lambda: iter(batches), None, max_epochs=1)
        assert exp.global_step == 6
        if hipgraph:
            gs = list(exp._graphed.values())
            assert len(gs) == 1 and gs[0].graph is not None and gs[0].seen == 6
        snap = _snapshot(exp)
        snap["model_rng"] = exp.model._rng_state.clone()
        snap["torch_rng"] = torch.get_rng_state()
        snap["device_rng"] = torch.cuda.get_rng_state(dev)
        finals[on] = snap
        assert (exp.grad_tracker is not None) == on
        if on:
            assert exp.last_grad_norms["step"] == 5 and exp.last_grad_hists["step"] == 4
    assert sorted(finals[True]) == sorted(finals[False])
    for k in finals[True]:
        assert torch.equal(finals[True][k], finals[False][k]), k


# ---- what is measured ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [2, 1, 3.5, "inf"])
def test_norms_equal_the_gradients(dev, p):
    """One eager step at k = 1: Python still sees the gradients, and every recorded norm is the float64 norm of that
    parameter's ``.grad`` to 4 decimals; the total is the norm of the norms."""
    from ctvae_amd.experiment import VAEXperiment
    exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False), track_grad_norm=p, log_every=1)
    exp.fit(lambda: iter(_batches(dev, 1)), None, max_epochs=1)
    pf = float(p)
    rec = exp.last_grad_norms
    assert rec["lr-Adam"] == EXP["LR"]
    _assert_norm_record(rec, _want_norms(exp.model, 1.0, pf), pf, 0)
    assert exp.last_grad_hists is None


def test_total_equals_the_clip_norm(dev):
    """gradient_clip_val with track_grad_norm 2: the tracker's total before rounding against the optimizer's device ``grad_norm``
    (the pre-clip norm of the clipped step): two independent kernels agree within relative 1e-6."""
    from ctvae_amd.experiment import VAEXperiment
    probe = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False))
    clip = 0.25 * float(_backward(probe, _batches(dev, 1)[0], 0).double().norm())
    exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False), track_grad_norm=2, log_every=1, gradient_clip_val=clip)
    exp.fit(lambda: iter(_batches(dev, 1)), None, max_epochs=1)
    clip_norm = float(exp.optimizer.grad_norm)
    _, _, sums, _, _, _ = exp.grad_tracker.measure(1.0, False)
    total = math.sqrt(math.fsum(float(s) for s in sums[:, 0]))
    want = float(exp.model.flat_grads.double().norm())
    print(f"tracker total {total!r} clip norm {clip_norm!r} float64 {want!r} "
          f"rel(tracker, clip) {abs(total - clip_norm) / want:.2e} rel(tracker, float64) {abs(total - want) / want:.2e}")
    assert clip_norm > clip > 0, "the clip did not act"
    assert abs(total - want) <= 1e-6 * want
    assert abs(total - clip_norm) <= 1e-6 * want
    assert abs(exp.last_grad_norms["grad_2.0_norm_total"] - total) <= 0.5e-4


def test_accumulation_records_the_window_mean(dev):
    """accumulate_grad_batches: 2 over four batches: one record per window, whose norms are those of (g1 + g2) / 2 formed by hand
    from two backward passes of an untracked twin."""
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, 4)
    lines = []

    class _Log:
        def write(self, s):
            lines.append(json.loads(s))

        def flush(self):
            pass

    exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False), accumulate_grad_batches=2, track_grad_norm=2, log_every=1,
                       log_file=_Log())
    exp.fit(lambda: iter(batches), None, max_epochs=1)
    recs = [l for l in lines if "grad_2.0_norm_total" in l]
    assert [r["step"] for r in recs] == [0, 1]
    twin = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False))
    g1, g2 = _backward(twin, batches[0], 0), _backward(twin, batches[1], 1)
    twin.model.flat_grads.copy_(g1 + g2)
    _assert_norm_record(recs[0], _want_norms(twin.model, 0.5, 2.0), 2.0, 0)
    whole = _want_norms(twin.model, 1.0, 2.0)
    k = "grad_2.0_norm/model.fc_mu.weight"
    assert abs(recs[0][k] - whole["fc_mu.weight"]) > 1e-3, "the sum's norm would not tell 1 / k apart"


class _StandInExchange:
    """A two-rank gradient exchange on one GPU: ``all_reduce`` adds the other rank's gradient (a fixed tensor) into the flat
    buffer, ``grad_scale`` is 1 / 2.  The interface VAEXperiment uses of ddp.GradBucketAllReduce, without a process group."""
    grad_scale, world, active = 0.5, 2, True

    def __init__(self, model, other):
        self.model, self.other, self.range = model, other, None

    def restrict(self, flat_slice):
        self.range = flat_slice

    def all_reduce(self, async_op=False):
        self.model.gather_torch_grads()
        self.model.flat_grads.add_(self.other)
        return []

    def reduce_scalars(self, scal):
        return scal


def test_ddp_scale(dev):
    """grad_scale 1 / 2: the norms are those of half the exchanged buffer."""
    from ctvae_amd.experiment import VAEXperiment
    m = _vanilla(dev)
    gen = torch.Generator().manual_seed(8)
    other = (torch.randn(m.flat_params.numel(), generator=gen) * 1e-3).to(dev)
    exp = VAEXperiment(m, dict(EXP, hipgraph=False), ddp=_StandInExchange(m, other), track_grad_norm=2, log_every=1)
    exp.fit(lambda: iter(_batches(dev, 1)), None, max_epochs=1)
    alone = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False))
    g = _backward(alone, _batches(dev, 1)[0], 0)
    assert torch.equal(m.flat_grads, g + other), "the buffer does not hold the exchanged sum"
    _assert_norm_record(exp.last_grad_norms, _want_norms(m, 0.5, 2.0), 2.0, 0)


# ---- histograms ----------------------------------------------------------------------------------------------
def test_histograms_equal_torch_histc(dev):
    """Counts per parameter against torch.histc on the CPU, run on the ``.grad`` copy times the scale (k = 2: scale 1 / 2)."""
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, 2)
    exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False), accumulate_grad_batches=2, watch_gradients=True, watch_log_freq=1)
    exp.fit(lambda: iter(batches), None, max_epochs=1)
    rec = exp.last_grad_hists
    assert rec["step"] == 0 and exp.last_grad_norms is None
    names = [n for n, _ in exp.model.named_parameters()]
    assert sorted(k for k in rec if k != "step") == sorted("gradients/" + n for n in names)
    spread = 0
    for n, prm in exp.model.named_parameters():
        v = (prm.grad.detach().float() * torch.tensor(0.5, dtype=torch.float32)).cpu().reshape(-1)
        r = rec["gradients/" + n]
        assert r["nonfinite"] == 0 and r["min"] == float(v.min()) and r["max"] == float(v.max()), n
        want = torch.histc(v, bins=64, min=r["min"], max=r["max"]).long().tolist()
        assert r["counts"] == want, (n, [i for i in range(64) if r["counts"][i] != want[i]][:6])
        assert sum(r["counts"]) == v.numel()
        spread += sum(1 for c in r["counts"] if c) > 8
    assert spread > len(names) // 2, "most histograms are degenerate"


# ---- CT-MCQ-VAE: parameters without a gradient -----------------------------------------------------------------
def _ct_records(dev, absent):
    from ctvae_amd.experiment import VAEXperiment
    params = dict(PARAMS, hipgraph=False)
    if absent is not None:
        params["adam_absent_grad"] = absent
    exp = VAEXperiment(_ct_model(dev), params, track_grad_norm=2, watch_gradients=True, watch_log_freq=1, log_every=1)
    norms, hists = [], []
    for i, batch in enumerate(_ct_batches(dev)[:3]):
        exp.model.zero_grad(lazy=True)
        from ctvae_amd import kernels as K
        K.backward(exp.training_step(batch, i))
        exp.optimizer_step()
        norms.append(exp.last_grad_norms)
        hists.append(exp.last_grad_hists)
    return exp, norms, hists


def test_ct_skip_leaves_out_parameters_without_a_gradient(dev, fixed_noise):
    """adam_absent_grad: skip over a base, an action (actions 0 and 3) and a causal step: a record holds exactly the ct_layer
    parameters the mode and the batch's actions give a gradient (tests/test_adam_blocks_host.expected_active)."""
    exp, norms, hists = _ct_records(dev, "skip")
    inside = [n for n, _ in exp.model.named_parameters() if n.startswith("ct_layer.")]
    stem = "grad_2.0_norm/model."
    for s, (mode, actions) in enumerate(SEQUENCE[:3]):
        want = sorted(n for n in inside if expected_active(n[len("ct_layer."):], mode, actions or []))
        assert sorted(k[len(stem):] for k in norms[s] if k.startswith(stem)) == want, (s, mode)
        assert sorted(k[len("gradients/"):] for k in hists[s] if k.startswith("gradients/")) == want, (s, mode)
        assert norms[s]["step"] == hists[s]["step"] == s
    base, action = norms[0], norms[1]
    assert stem + "ct_layer.mask.0.weight" not in base and stem + "ct_layer.mask.0.weight" in action
    scorers = sorted({int(k[len(stem):].split(".")[2]) for k in action if k.startswith(stem + "ct_layer.graph_discovers.")})
    assert scorers == [0, 1, 4]                       # scorer 0 and the scorers of actions 0 and 3
    assert not [k for k in base if k.startswith(stem) and not k.startswith(stem + "ct_layer.")], "a parameter outside the slice"
    # the last step is still visible to Python: the recorded norms are those of the .grad views
    present = {k[len(stem):] for k in norms[2] if k.startswith(stem)}
    for n, w in _want_norms(exp.model, 1.0, 2.0, present).items():
        assert abs(norms[2][stem + n] - w) <= 0.5e-4 + 1e-6 * w, n


def test_ct_zero_reports_every_parameter_of_the_slice(dev, fixed_noise):
    exp, norms, hists = _ct_records(dev, None)
    inside = sorted(n for n, _ in exp.model.named_parameters() if n.startswith("ct_layer."))
    stem = "grad_2.0_norm/model."
    for s in range(3):
        assert sorted(k[len(stem):] for k in norms[s] if k.startswith(stem)) == inside
        assert sorted(k[len("gradients/"):] for k in hists[s] if k.startswith("gradients/")) == inside
    assert norms[0][stem + "ct_layer.mask.0.weight"] == 0.0              # base mode: reported, as the zeros it is stepped with
    h = hists[0]["gradients/ct_layer.mask.0.weight"]
    assert h["min"] == h["max"] == 0.0 and h["counts"][32] == sum(h["counts"])


# ---- the runner ----------------------------------------------------------------------------------------------
def _cfg_with(tmp_path, sub, trainer=None, exp=None):
    path = _runner_cfg(tmp_path, sub, **(trainer or {}))
    cfg = yaml.safe_load(open(path))
    cfg["exp_params"].update(exp or {})
    open(path, "w").write(yaml.safe_dump(cfg))
    return path


def _jsonl(path):
    return [json.loads(l) for l in open(path)]


def test_runner_writes_both_records(dev, tmp_path):
    """run.main on synthetic data, 7 steps: the norm lines (with ``lr-Adam``) at the logged steps only -- ``log_every`` is 50,
    so at step 0 -- and a histogram line every ``watch_log_freq`` = 3 steps."""
    from ctvae_amd import run
    args = ["--steps-per-epoch", "7", "--max-epochs", "1"]
    run.main(["-c", _cfg_with(tmp_path, "on", {"track_grad_norm": 2}, {"watch_gradients": True, "watch_log_freq": 3})] + args)
    d = tmp_path / "on" / "VanillaVAE"
    norm_lines = [l for l in _jsonl(d / "metrics_rank0.jsonl") if "grad_2.0_norm_total" in l]
    assert [l["step"] for l in norm_lines] == [0]
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "vae.yaml")))
    assert norm_lines[0]["lr-Adam"] == cfg["exp_params"]["LR"]
    assert sum(1 for k in norm_lines[0] if k.startswith("grad_2.0_norm/model.")) == 48 and norm_lines[0]["grad_2.0_norm_total"] > 0
    hist_lines = _jsonl(d / "gradients_rank0.jsonl")
    assert [l["step"] for l in hist_lines] == [0, 3, 6]
    for l in hist_lines:
        assert len(l) == 49 and all(len(v["counts"]) == 64 for k, v in l.items() if k != "step")
        assert l["gradients/fc_mu.weight"]["nonfinite"] == 0 and sum(l["gradients/fc_mu.weight"]["counts"]) == 2048 * 128


def test_runner_without_the_keys_adds_nothing(dev, tmp_path):
    from ctvae_amd import run
    run.main(["-c", _cfg_with(tmp_path, "off"), "--steps-per-epoch", "2", "--max-epochs", "1"])
    d = tmp_path / "off" / "VanillaVAE"
    assert not (d / "gradients_rank0.jsonl").exists()
    for l in _jsonl(d / "metrics_rank0.jsonl"):
        assert not [k for k in l if k.startswith("grad_") or k == "lr-Adam"], l


@pytest.mark.parametrize("bad", [0, True])
def test_runner_refuses_track_grad_norm_by_name(dev, tmp_path, bad):
    from ctvae_amd import run
    with pytest.raises(SystemExit, match="track_grad_norm"):
        run.main(["-c", _cfg_with(tmp_path, "bad", {"track_grad_norm": bad}), "--steps-per-epoch", "2", "--max-epochs", "1"])


def test_untracked_steps_launch_nothing(dev):
    """log_every 4, watch_log_freq 3 over six steps: the library's launch log shows the stats pass on steps 0, 3 and 4 and the
    histogram pass on steps 0 and 3, and no tracking launch without the keys."""
    from ctvae_amd import native
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, 6)
    reports = {}
    for on in (False, True):
        kw = dict(track_grad_norm=2, watch_gradients=True, watch_log_freq=3, log_every=4) if on else dict(log_every=4)
        exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False), **kw)
        torch.cuda.synchronize()
        native.prof_enable(True)
        try:
            exp.fit(lambda: iter(batches), None, max_epochs=1)
            torch.cuda.synchronize()
        finally:
            native.prof_enable(False)
        reports[on] = {k: v["count"] for k, v in native.prof_report().items()}
    tracking = {"grad_stats_kernel": 3, "grad_stats_finalize_kernel": 3, "grad_hist_kernel": 2}
    assert {k: v for k, v in reports[True].items() if k.startswith("grad_stats") or k.startswith("grad_hist")} == tracking
    assert {k: v for k, v in reports[True].items() if k not in tracking} == reports[False]
