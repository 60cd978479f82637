"""GPU: ``exp_params.kld_schedule`` / ``kld_free_bits`` through the training harness (experiment.py, klcontrol.py): the device-resident
KL weight under a captured step, the free-bits loss path of the served models, checkpoints.

VanillaVAE (latent_dim 128) at B = 4, built with the helpers of tests/test_grad_accum_gpu.py, unless stated."""
import ctypes
import io
import json

import pytest
import torch

from ctvae_amd import filler
from tests import helpers as H
from tests import kl_checks as C
from tests.test_grad_accum_gpu import B, EXP, _assert_same, _batches, _snapshot, _vanilla
from tests.test_models_gpu import ZOO

pytestmark = pytest.mark.gpu
LINEAR8 = {"type": "linear", "warmup_steps": 8}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _fit(dev, params, batches, model=None, **kw):
    """One epoch over ``batches`` with every step logged; returns (experiment, training records)."""
    from ctvae_amd.experiment import VAEXperiment
    log = io.StringIO()
    exp = VAEXperiment(model if model is not None else _vanilla(dev), params, log_every=1, log_file=log, **kw)
    exp.fit(lambda: iter(batches), None, max_epochs=1)
    torch.cuda.synchronize()
    return exp, [json.loads(line) for line in log.getvalue().splitlines()]


# ---- (a) the weight is read at replay, not baked into the capture -------------------------------------------
def test_captured_steps_follow_the_schedule(dev):
    """Eight steps of a linear warm-up over eight steps with a floor: with hipGraph on, three warm steps, the capture and four
    replays.  Parameters, Adam moments and BatchNorm buffers equal the eager run's bit for bit, and every step logs the
    formula's weight.  A weight passed by value would stay at the capture step's from the first replay on."""
    from ctvae_amd.klcontrol import weight
    batches = _batches(dev, 8)
    keys = {"kld_schedule": LINEAR8, "kld_free_bits": 0.05}
    finals, logs = {}, {}
    for hipgraph in (True, False):
        exp, recs = _fit(dev, dict(EXP, hipgraph=hipgraph, **keys), batches)
        assert exp.global_step == 8 and len(recs) == 8
        if hipgraph:
            gs = list(exp._graphed.values())
            assert len(gs) == 1 and gs[0].graph is not None and gs[0].seen == 8
        want = [weight(exp.kl.schedule, EXP["kld_weight"], s) for s in range(8)]
        assert want[0] == 0.0 and len(set(want)) == 8
        assert [r["kld_weight"] for r in recs] == want and [r["step"] for r in recs] == list(range(8))
        assert exp.kl.fills == 8 and float(exp.kl.tensor[0]) == want[7]
        for r in recs:
            assert 0 <= r["KLD_floored_dims"] <= 128 and r["KLD_floored_dims"] == int(r["KLD_floored_dims"])
            assert r["KLD_free_bits"] >= -r["KLD"] * (1 - 1e-6) and r["KLD_free_bits"] >= 0.05 * r["KLD_floored_dims"]
        finals[hipgraph], logs[hipgraph] = _snapshot(exp), recs
    _assert_same(finals[True], finals[False], "captured against eager under a schedule")
    assert logs[True] == logs[False]


# ---- (b) a constant schedule without a floor is the plain run -----------------------------------------------
def test_constant_schedule_without_a_floor_trains_like_the_plain_run(dev):
    """``start: 1`` and ``kld_free_bits: 0.0`` against a run without the keys, six steps: per parameter tensor the bounds of
    tests/test_ct_gpu.py::test_harness_three_adam_steps_match_reference (three steps: 90 % of the elements within 0.15 lr, 98 %
    within 0.6 lr, all within 4 lr), scaled to six steps."""
    batches = _batches(dev, 6)
    keys = {"kld_schedule": {"type": "linear", "warmup_steps": 3, "start": 1}, "kld_free_bits": 0.0}
    plain, _ = _fit(dev, dict(EXP), batches)
    ctl, recs = _fit(dev, dict(EXP, **keys), batches)
    assert ctl.kl.fills == 1 and plain.kl is None                # a constant phase launches nothing
    assert all(r["kld_weight"] == ctypes.c_float(EXP["kld_weight"]).value for r in recs)
    assert all(r["KLD_floored_dims"] == 0 and abs(r["KLD_free_bits"] + r["KLD"]) <= 1e-6 * abs(r["KLD"]) for r in recs)
    lr, worst = EXP["LR"], 0.0
    got = dict(ctl.model.named_parameters())
    for k, p in plain.model.named_parameters():
        if k.endswith(".0.bias") and not k.startswith("final_layer.3"):
            continue        # conv bias in front of a BatchNorm: its gradient is rounding noise
        d = ((got[k].detach() - p.detach()).abs().flatten().cpu() / lr)[:1000000]
        q = torch.quantile(d, torch.tensor([0.9, 0.98, 1.0]))
        worst = max(worst, float(q[2]))
        assert float(q[0]) <= 0.3 and float(q[1]) <= 1.2 and float(q[2]) <= 8.0, (k, [float(v) for v in q])
    print(f"largest deviation after six steps: {worst:.4f} lr")


# ---- (c) without the keys ------------------------------------------------------------------------------------
def test_without_the_keys_nothing_is_launched_and_the_step_is_the_plain_one(dev, monkeypatch):
    """No ``ctvae_freebits_*`` call, no buffer, no log key, no checkpoint entry; the run equals, bit for bit, the step written out
    by hand with a float ``M_N``: forward, ``loss_function(M_N=kld_weight)``, backward, Adam."""
    from ctvae_amd import kernels as K
    from ctvae_amd import native
    from ctvae_amd.experiment import VAEXperiment
    calls = []
    inner = native.call

    def spy(name, *args):
        calls.append(name)
        return inner(name, *args)
    monkeypatch.setattr(native, "call", spy)
    batches = _batches(dev, 3)
    exp, recs = _fit(dev, dict(EXP, hipgraph=False), batches)
    assert calls and not [c for c in calls if c.startswith("ctvae_freebits_")]
    assert exp.kl is None and "kl" not in exp.state_dict()
    assert not any(k in r for r in recs for k in ("kld_weight", "KLD_free_bits", "KLD_floored_dims"))
    hand = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=False))
    for i, (x, labels) in enumerate(batches):
        hand.model.zero_grad(lazy=True)
        losses = hand.model.loss_function(*hand.model(x, labels=labels), M_N=EXP["kld_weight"], optimizer_idx=0, batch_idx=i)
        K.backward(losses["loss"])
        hand.model.settle_grads()
        hand.optimizer.step()
    _assert_same(_snapshot(exp), _snapshot(hand), "fit() without the keys against the hand-written float-M_N step")
    del calls[:]
    _fit(dev, dict(EXP, hipgraph=False, kld_free_bits=0.0), batches[:1])
    assert calls.count("ctvae_freebits_kl_forward_grad") == 1    # (the spy does see the launch when there is one)


# ---- (d) a floor above every column --------------------------------------------------------------------------
def test_a_floor_above_every_column_switches_the_kl_gradient_off(dev):
    """lambda = 50: all 128 dimensions are floored, g_mu = g_lv = 0, the encoder heads get the reconstruction gradient alone --
    the parameters after one step equal those of a run with ``kld_weight: 0`` bit for bit, and the loss is that run's plus the
    constant w * 128 * 50 within the rounding of the fp32 loss scalar."""
    batch = _batches(dev, 1)
    floor, recs_f = _fit(dev, dict(EXP, hipgraph=False, kld_free_bits=50.0), batch)
    zero, recs_0 = _fit(dev, dict(EXP, hipgraph=False, kld_weight=0.0), batch)
    rf, r0 = recs_f[0], recs_0[0]
    assert rf["KLD_floored_dims"] == 128 and rf["KLD_free_bits"] == 6400.0
    assert abs(rf["KLD"] - r0["KLD"]) <= C.VALUE_RTOL * abs(r0["KLD"]) and rf["KLD"] < 0
    const = EXP["kld_weight"] * 6400.0
    print(f"loss {rf['loss']!r} against {r0['loss']!r} + {const!r}; reconstruction {rf['Reconstruction_Loss']!r} / {r0['Reconstruction_Loss']!r}")
    assert abs(rf["Reconstruction_Loss"] - r0["Reconstruction_Loss"]) <= 2.0 ** -23 * abs(r0["Reconstruction_Loss"])
    assert abs(rf["loss"] - (r0["loss"] + const)) <= 4 * 2.0 ** -24 * abs(rf["loss"])
    _assert_same(_snapshot(floor), _snapshot(zero), "a floor above every column against kld_weight 0")


# ---- (e) resume ---------------------------------------------------------------------------------------------
def test_full_resume_in_the_middle_of_a_warm_up(dev):
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, 6)
    params = dict(EXP, hipgraph=False, kld_schedule=LINEAR8, kld_free_bits=0.05)
    straight, recs = _fit(dev, params, batches)
    first, _ = _fit(dev, params, batches[:3])
    trainer = first.state_dict()
    assert trainer["kl"] == {"schedule": {"type": "linear", "warmup_steps": 8, "start": 0.0}, "free_bits": 0.05}
    weights = {k: v.detach().clone() for k, v in first.model.state_dict().items()}
    m = _vanilla(dev, seed=77)                                   # other weights: everything has to come from the checkpoint
    m.load_state_dict(weights)
    log = io.StringIO()
    resumed = VAEXperiment(m, dict(params), log_every=1, log_file=log)
    resumed.load_state_dict(trainer)
    assert resumed.global_step == 3
    resumed.fit(lambda: iter(batches[3:]), None, max_epochs=1)
    later = [json.loads(line) for line in log.getvalue().splitlines()]
    assert [r["kld_weight"] for r in later] == [r["kld_weight"] for r in recs[3:]] and later == recs[3:]
    _assert_same(_snapshot(straight), _snapshot(resumed), "resumed at step 3 of a warm-up of 8")
    other = VAEXperiment(_vanilla(dev), dict(params, kld_schedule={"type": "linear", "warmup_steps": 9}))
    with pytest.raises(RuntimeError, match=r"kld_schedule.*warmup_steps.*exp_params\.kld_schedule"):
        other.load_state_dict(trainer)


# ---- (f) the other served models -----------------------------------------------------------------------------
SERVED = [z for z in ZOO if z[0] in ("ConditionalVAE", "MSSIMVAE", "LogCoshVAE", "BetaVAE", "TwoStageVAE")]


@pytest.mark.parametrize("name,cfg", SERVED, ids=[z[0] for z in SERVED])
def test_served_models_take_one_step_with_the_keys(dev, name, cfg):
    from ctvae_amd.models import vae_models
    params = {"LR": 0.0005, "weight_decay": 0.0, "kld_weight": 0.00025, "hipgraph": False}
    keys = {"kld_schedule": {"type": "cyclical", "cycle_steps": 4, "ratio": 0.5}, "kld_free_bits": 0.05}
    recs = {}
    for with_keys in (False, True):
        torch.manual_seed(3)
        m = vae_models[name](**{k: (list(v) if isinstance(v, list) else v) for k, v in cfg.items()}, name=name).to(dev).train()
        labels = H.cvae_labels(900, 8).to(dev) if name == "ConditionalVAE" else torch.zeros(8, device=dev)
        # two steps: the cyclical weight is 0 at step 0 and kld_weight / 2 at step 1
        batches = [(H.zoo_prepare(name, m, filler.synthetic_batch(900 + i, 8)[0].to(dev)), labels) for i in range(2)]
        before = m.flat_params.clone()
        exp, recs[with_keys] = _fit(dev, dict(params, **(keys if with_keys else {})), batches, model=m)
        assert torch.isfinite(m.flat_params).all() and not torch.equal(m.flat_params, before)
    plain, ctl = recs[False], recs[True]
    assert ctl[0]["kld_weight"] == 0.0 and ctl[1]["kld_weight"] > 0.0
    for r in ctl:
        assert r["loss"] == r["loss"] and abs(r["loss"]) < float("inf")
        assert 0 <= r["KLD_floored_dims"] <= 128 and r["KLD_free_bits"] >= abs(r["KLD"]) * (1 - 1e-6)
    assert "KLD_floored_dims" not in plain[0] and "kld_weight" not in plain[0]
    print(f"{name}: KLD {ctl[0]['KLD']!r} with the keys, {plain[0]['KLD']!r} without")
    assert abs(ctl[0]["KLD"] - plain[0]["KLD"]) <= C.VALUE_RTOL * abs(plain[0]["KLD"])      # step 0: the same weights and batch
