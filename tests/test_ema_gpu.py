"""GPU: the weight average (``exp_params.ema_decay`` / ``ema_warmup`` / ``ema_eval``) through the training harness, the runner
and a checkpoint: optim.WeightEMA on csrc/ema.hip, its place behind the optimizer step, and evaluation with the averaged weights.

VanillaVAE (latent_dim 128) at B = 4 unless stated; CT-MCQ-VAE is the configuration the rollout tests use (tests/test_ct_gpu:
``build_ct``) with ``update_parameters: ct_layer``; the runner case is MCQVAE at 8, as the full-resume test of tests/test_ct_gpu.py.
Error bound of a trajectory of s updates: s * 2^-22 * max|value| -- every update stays within 2^-22 * max(|ema|, |p|) of its exact
result (tests/test_ema_ops_gpu.py), an update is a contraction (it never enlarges an earlier error: |1 - w| < 1), and an average
never leaves the range of the values it has seen."""
import ctypes
import os
import socket

import pytest
import torch
import yaml

from ctvae_amd import filler
from tests.test_ct_gpu import _FixedNoise, build_ct
from tests.test_grad_accum_gpu import B, EXP, _assert_same, _batches, _snapshot, _vanilla

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = 12


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture()
def fixed_noise(dev):
    from ctvae_amd.models import causal
    prev = causal.set_noise_source(_FixedNoise(dev))
    yield
    causal.set_noise_source(prev)


def _f32(x):
    return ctypes.c_float(x).value


def _epochs(batches, per_epoch):
    """A ``train_batches`` callable that hands out the next ``per_epoch`` batches on every call."""
    calls = [0]

    def train():
        lo = calls[0] * per_epoch
        calls[0] += 1
        return iter(batches[lo:lo + per_epoch])
    return train


def _spy_on_updates(exp, snaps):
    """Record the optimizer's slice right behind every optimizer step: in front of the update that follows it."""
    inner = exp.ema_update

    def spy():
        snaps.append(exp.model.flat_params[exp.optimizer.slice].clone())
        inner()
    exp.ema_update = spy


# ---- 1. training does not notice ---------------------------------------------------------------------------
@pytest.mark.parametrize("hipgraph", [True, False])
def test_training_is_bit_for_bit_the_same(dev, hipgraph):
    """Six steps, a validation epoch (under ema_eval: with the average swapped in) after the third; with hipGraph on, three warm
    steps, the capture and replays.  Parameters, both Adam moments, the step counter, the BatchNorm buffers and the model's noise
    state equal those of a run without the key."""
    from ctvae_amd.experiment import VAEXperiment
    train, val = _batches(dev, 6), _batches(dev, 2, seed=4900)
    finals, rngs = {}, {}
    for name, extra in (("plain", {}), ("ema", {"ema_decay": 0.5})):
        exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=hipgraph, **extra))
        hist = exp.fit(_epochs(train, 3), lambda: iter(val), max_epochs=2)
        assert exp.global_step == 6 and "val_loss" in hist[0]
        if hipgraph:
            gs = list(exp._graphed.values())
            assert len(gs) == 1 and gs[0].graph is not None and gs[0].seen == 6
        finals[name], rngs[name] = _snapshot(exp), exp.model._rng_state.clone()
        assert (exp.ema is None) == (name == "plain")
        if exp.ema is not None:
            assert exp.ema.updates == 6 and not exp.ema.swapped
            assert not torch.equal(exp.ema.buffer, exp.model.flat_params)
    _assert_same(finals["plain"], finals["ema"], "with and without ema_decay")
    assert torch.equal(rngs["plain"], rngs["ema"])


# ---- 2. the trajectory -------------------------------------------------------------------------------------
@pytest.mark.parametrize("hipgraph", [True, False])
@pytest.mark.parametrize("decay,warmup", [(0.5, False), (0.999, True)])
def test_average_follows_the_float64_recurrence(dev, hipgraph, decay, warmup):
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.optim import ema_decay_at
    exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=hipgraph, ema_decay=decay, ema_warmup=warmup))
    start = exp.model.flat_params.clone()
    assert torch.equal(exp.ema.buffer, start) and exp.ema.updates == 0
    snaps = []
    _spy_on_updates(exp, snaps)
    exp.fit(lambda: iter(_batches(dev, 6)), None, max_epochs=1)
    torch.cuda.synchronize()
    assert exp.ema.updates == 6 and len(snaps) == 6
    ref, top = start.double(), float(start.abs().max())
    for t, p in enumerate(snaps, start=1):
        w = _f32(1.0 - ema_decay_at(decay, warmup, t))
        ref = ref + w * (p.double() - ref)
        top = max(top, float(p.abs().max()))
    if warmup:
        assert _f32(1.0 - 2 / 11) == _f32(1.0 - exp.ema.decay_at(1)) and exp.ema.decay_at(6) == 7 / 16
    bound = 6 * 2.0 ** -22 * top
    err = float((exp.ema.buffer.double() - ref).abs().max())
    print(f"decay {decay} warmup {warmup}: max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert float((exp.ema.buffer - snaps[-1]).abs().max()) > 10 * bound, "the average sits on the last weights"


# ---- 3. evaluation -----------------------------------------------------------------------------------------
VAL_SEED = 777      # without gradients VanillaVAE draws its latent noise from torch's device generator: the same for every record


def _validated_alone(dev, weights, rng, val):
    """The validation record of a fresh model holding ``weights``, with plain weights and the given noise state."""
    from ctvae_amd.experiment import VAEXperiment
    m = _vanilla(dev)
    m.load_state_dict(weights)
    m._rng_state = rng.clone()
    exp = VAEXperiment(m, dict(EXP, LR=1e-2, hipgraph=False))
    torch.manual_seed(VAL_SEED)
    return exp.fit(lambda: iter([]), lambda: iter(val), max_epochs=1)[0]


def _val_part(rec):
    out = {k: v for k, v in rec.items() if k.startswith("val_")}
    assert "val_loss" in out and "val_Reconstruction_Loss" in out
    return out


def test_ema_eval_validates_with_the_average(dev):
    from ctvae_amd.experiment import VAEXperiment
    train, val = _batches(dev, 3), _batches(dev, 2, seed=4900)
    recs = {}
    for ema_eval in (True, False):
        extra = {} if ema_eval else {"ema_eval": False}           # (on by default)
        exp = VAEXperiment(_vanilla(dev), dict(EXP, LR=1e-2, hipgraph=False, ema_decay=0.5, **extra))
        exp.fit(lambda: iter(train), None, max_epochs=1)
        rng = exp.model._rng_state.clone()
        live = {k: v.detach().clone() for k, v in exp.model.state_dict().items()}
        averaged = exp.ema_model_state_dict()
        before = _snapshot(exp)
        torch.manual_seed(VAL_SEED)
        recs[ema_eval] = _val_part(exp.fit(lambda: iter([]), lambda: iter(val), max_epochs=1)[0])
        assert not exp.ema.swapped
        after = _snapshot(exp)
        _assert_same(before, after, "validation left the live weights as they were")
        if ema_eval:
            moved = [k for k in live if not torch.equal(live[k].cpu(), averaged[k])]
            same = [k for k in live if torch.equal(live[k].cpu(), averaged[k])]
            assert any(k.endswith("weight") for k in moved) and any(k.endswith("running_mean") for k in same)
            recs["from ema_state_dict"] = _val_part(_validated_alone(dev, averaged, rng, val))
            recs["from state_dict"] = _val_part(_validated_alone(dev, live, rng, val))
    print({k: v["val_loss"] for k, v in recs.items()})
    assert recs[True] == recs["from ema_state_dict"]
    assert recs[False] == recs["from state_dict"]
    assert recs[True]["val_loss"] != recs[False]["val_loss"]
    assert recs[True]["val_Reconstruction_Loss"] != recs[False]["val_Reconstruction_Loss"]


# ---- 4. accumulate_grad_batches ----------------------------------------------------------------------------
@pytest.mark.parametrize("hipgraph", [True, False])
def test_updates_count_optimizer_steps_under_accumulation(dev, hipgraph):
    from ctvae_amd.experiment import VAEXperiment
    exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=hipgraph, ema_decay=0.5), accumulate_grad_batches=2)
    snaps = []
    _spy_on_updates(exp, snaps)
    exp.fit(lambda: iter(_batches(dev, 4)), None, max_epochs=1)
    assert exp.global_step == 2 and exp.ema.updates == 2 and len(snaps) == 2
    assert not torch.equal(snaps[0], snaps[1])


# ---- 5. update_parameters ----------------------------------------------------------------------------------
def _ct_batch(dev, seed, mode, actions=None):
    x, y, _ = filler.synthetic_pairs(seed, B, A)
    opts = {"mode": [mode] * B}
    if mode != "base":
        opts.update(input_y=y.to(dev), action=torch.nn.functional.one_hot(torch.tensor(actions), A).float().to(dev))
    return (x.to(dev), torch.zeros(B, device=dev), opts)


CT_PARAMS = {"LR": 5e-4, "weight_decay": 0.0, "kld_weight": 0.00025, "update_parameters": "ct_layer", "hipgraph": False}


def _ct_step(exp, batch, i):
    from ctvae_amd import kernels as K
    exp.model.zero_grad(lazy=True)
    K.backward(exp.training_step(batch, i))
    exp.optimizer_step()
    torch.cuda.synchronize()


def test_update_parameters_averages_and_swaps_the_slice_alone(dev, fixed_noise):
    from ctvae_amd.experiment import VAEXperiment
    m = build_ct(dev, 5)
    exp = VAEXperiment(m, dict(CT_PARAMS, ema_decay=0.5))
    sl = m.flat_range("ct_layer")
    assert exp.optimizer.slice == sl and 0 < sl.start and sl.stop - sl.start < m.flat_params.numel()
    assert exp.ema.buffer.numel() == sl.stop - sl.start
    assert exp.ema.buffer.data_ptr() % 16 == m.flat_params[sl].data_ptr() % 16
    _ct_step(exp, _ct_batch(dev, 301, "action", [0, 3, 0, 3]), 0)
    assert exp.ema.updates == 1
    flat, avg = m.flat_params.clone(), exp.ema.buffer.clone()
    assert not torch.equal(flat[sl], avg)
    exp.ema.swap()
    torch.cuda.synchronize()
    now = m.flat_params
    assert torch.equal(now[:sl.start].view(torch.int32), flat[:sl.start].view(torch.int32))
    assert torch.equal(now[sl.stop:].view(torch.int32), flat[sl.stop:].view(torch.int32))
    assert torch.equal(now[sl], avg) and torch.equal(exp.ema.buffer, flat[sl]) and exp.ema.swapped
    with pytest.raises(RuntimeError, match="swapped in"):
        exp.ema.update()
    exp.ema.swap()
    torch.cuda.synchronize()
    assert torch.equal(m.flat_params, flat) and torch.equal(exp.ema.buffer, avg) and not exp.ema.swapped
    with pytest.raises(ZeroDivisionError):                 # the live weights come back when the body raises
        with exp.ema.swapped_in():
            assert torch.equal(m.flat_params[sl], avg)
            1 / 0
    assert torch.equal(m.flat_params, flat) and not exp.ema.swapped


# ---- 7. skip mode: a block that did not step is still averaged ----------------------------------------------
def test_skip_mode_block_without_a_step_is_still_averaged(dev, fixed_noise):
    """adam_absent_grad: skip.  An action-mode step moves the mask network and leaves its average between the old and the new
    weights; the base-mode step behind it gives the mask network no gradient: its weights stay bit for bit, its average moves
    on towards them."""
    from ctvae_amd.experiment import VAEXperiment
    m = build_ct(dev, 5)
    exp = VAEXperiment(m, dict(CT_PARAMS, adam_absent_grad="skip", ema_decay=0.5))
    sl = exp.optimizer.slice
    p = m.get_parameter("ct_layer.mask.0.weight")
    lo = (p.data_ptr() - m.flat_params.data_ptr()) // 4 - sl.start
    hi = lo + p.numel()
    assert p.is_contiguous() and 0 <= lo < hi <= sl.stop - sl.start
    p0 = m.flat_params[sl].clone()
    _ct_step(exp, _ct_batch(dev, 301, "action", [0, 3, 0, 3]), 0)
    p1, e1 = m.flat_params[sl].clone(), exp.ema.buffer.clone()
    _ct_step(exp, _ct_batch(dev, 300, "base"), 1)
    p2, e2 = m.flat_params[sl].clone(), exp.ema.buffer.clone()
    assert exp.ema.updates == 2
    assert not torch.equal(p1[lo:hi], p0[lo:hi]), "the action-mode step did not move the mask network"
    assert not torch.equal(e1[lo:hi], p1[lo:hi])
    assert torch.equal(p2[lo:hi].view(torch.int32), p1[lo:hi].view(torch.int32)), "the block stepped in base mode"
    assert not torch.equal(p2, p1), "nothing stepped in base mode"
    ref = e1[lo:hi].double() + 0.5 * (p1[lo:hi].double() - e1[lo:hi].double())
    bound = 2.0 ** -22 * torch.maximum(e1[lo:hi].abs(), p1[lo:hi].abs()).double()
    assert bool(((e2[lo:hi].double() - ref).abs() <= bound).all())
    assert not torch.equal(e2[lo:hi], e1[lo:hi]), "the average of the block that did not step stood still"


# ---- 8. data-parallel --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_rank_rccl(dev):
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("a process group already exists in this process")
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    yield dist
    torch.cuda.synchronize()
    dist.destroy_process_group()


def test_average_under_rccl_equals_single_process(dev, one_rank_rccl):
    """A 1-rank RCCL group: the step of every rank of an N-GPU job (gradient exchange and Adam eagerly behind the graph), the
    update behind it and no collective of its own.  The average equals the single-process one bit for bit."""
    from ctvae_amd.ddp import GradBucketAllReduce
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, 5)
    finals = {}
    for use_ddp in (False, True):
        m = _vanilla(dev)
        ddp = GradBucketAllReduce(m, force=True) if use_ddp else None
        exp = VAEXperiment(m, dict(EXP, hipgraph=True, ema_decay=0.9), ddp=ddp)
        exp.fit(lambda: iter(batches), None, max_epochs=1)
        torch.cuda.synchronize()
        assert exp.ema.updates == 5 and all(g.graph is not None for g in exp._graphed.values())
        finals[use_ddp] = (exp.ema.buffer.clone(), m.flat_params.clone())
    assert torch.equal(finals[True][1], finals[False][1])
    assert torch.equal(finals[True][0], finals[False][0])
    assert not torch.equal(finals[True][0], finals[True][1])


# ---- 6. the runner: checkpoints and resume ------------------------------------------------------------------
def _runner_cfg(tmp_path, sub, exp=None, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "mcq_vae.yaml")))
    cfg["logging_params"]["save_dir"] = str(tmp_path / sub)
    cfg["data_params"]["train_batch_size"] = 8
    cfg["data_params"]["val_batch_size"] = 8
    cfg["exp_params"].update(exp or {})
    cfg["trainer_params"].update(trainer)
    p = tmp_path / f"{sub}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_resumes_the_average_bit_exactly(dev, tmp_path, monkeypatch):
    from ctvae_amd import run
    ema = {"ema_decay": 0.9, "ema_warmup": True}
    last = lambda sub: tmp_path / sub / "MCQVAE" / "checkpoints" / "last.ckpt"
    steps = ["--steps-per-epoch", "5"]
    h2 = run.main(["-c", _runner_cfg(tmp_path, "straight", ema)] + steps + ["--max-epochs", "2"])
    run.main(["-c", _runner_cfg(tmp_path, "first", ema)] + steps + ["--max-epochs", "1"])
    hr = run.main(["-c", _runner_cfg(tmp_path, "resumed", ema, resume_from_checkpoint=str(last("first")))] + steps + ["--max-epochs", "2"])
    a, b = torch.load(last("straight"), weights_only=True), torch.load(last("resumed"), weights_only=True)
    assert a["trainer"]["ema"] == b["trainer"]["ema"] == {"decay": 0.9, "warmup": True, "updates": 10}
    assert sorted(a["ema_state_dict"]) == sorted(a["state_dict"]) == sorted(b["ema_state_dict"])
    assert all(k.startswith("model.") for k in a["ema_state_dict"])
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    for k, v in a["ema_state_dict"].items():
        assert torch.equal(v, b["ema_state_dict"][k]), k
    differ = [k for k, v in a["state_dict"].items() if not torch.equal(v, a["ema_state_dict"][k])]
    assert any(k.endswith("weight") for k in differ) and not any("running_" in k or "num_batches" in k for k in differ)
    assert hr[0]["val_Reconstruction_Loss"] == h2[1]["val_Reconstruction_Loss"]          # (validated with the average, both)
    # a run without the key ignores both entries and writes neither
    run.main(["-c", _runner_cfg(tmp_path, "nokey", resume_from_checkpoint=str(last("first")))] + steps + ["--max-epochs", "2"])
    c = torch.load(last("nokey"), weights_only=True)
    assert "ema_state_dict" not in c and "ema" not in c["trainer"]
    for k, v in a["state_dict"].items():
        assert torch.equal(v, c["state_dict"][k]), k                                     # and trains as the others did
    # under the key: a checkpoint without the entries, or with another decay, is refused by name
    with pytest.raises(SystemExit, match=r"exp_params\.ema_decay.*nokey"):
        run.main(["-c", _runner_cfg(tmp_path, "bad", ema, resume_from_checkpoint=str(last("nokey")))] + steps + ["--max-epochs", "3"])
    with pytest.raises(SystemExit, match=r"exp_params\.ema_decay.*first"):
        run.main(["-c", _runner_cfg(tmp_path, "bad", {"ema_decay": 0.99, "ema_warmup": True},
                                    resume_from_checkpoint=str(last("first")))] + steps + ["--max-epochs", "2"])
    assert not last("bad").exists()
    # load_weights_only: the average starts from the loaded weights
    seen = {}
    fit = run.VAEXperiment.fit

    def spy(self, *args, **kw):
        seen["updates"] = self.ema.updates
        seen["equal"] = torch.equal(self.ema.buffer, self.model.flat_params[self.optimizer.slice])
        seen["weight"] = self.model.state_dict()["encoder.0.0.weight"].detach().cpu().clone()
        return fit(self, *args, **kw)
    monkeypatch.setattr(run.VAEXperiment, "fit", spy)
    run.main(["-c", _runner_cfg(tmp_path, "wo", ema, resume_from_checkpoint=str(last("nokey")), load_weights_only=True),
              "--steps-per-epoch", "2", "--max-epochs", "1"])
    assert seen["updates"] == 0 and seen["equal"] and torch.equal(seen["weight"], c["state_dict"]["model.encoder.0.0.weight"])
    d = torch.load(last("wo"), weights_only=True)
    assert d["trainer"]["ema"]["updates"] == 2


# ---- the checkpoint tools ----------------------------------------------------------------------------------
def test_tools_load_the_averaged_weights_under_ema(dev, tmp_path):
    """``--ema`` of apply_action and causal_graph: a checkpoint whose ``ema_state_dict`` holds other weights than its ``state_dict``
    gives, under the flag, exactly what a checkpoint with those weights as its ``state_dict`` gives, and something else without."""
    from ctvae_amd import apply_action, causal_graph
    from ctvae_amd.models import vae_models
    from tests import helpers as H
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))
    cfg["model_params"]["action_dim"] = 4
    cfg["data_params"].update(val_batch_size=B, train_batch_size=B)
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    path = tmp_path / "ct.yaml"
    path.write_text(yaml.safe_dump(cfg))
    weights = []
    for seed in (9, 11):
        torch.manual_seed(seed)
        m = vae_models["CTMCQVAE"](**dict(cfg["model_params"], hidden_dims=list(cfg["model_params"]["hidden_dims"])))
        m.load_state_dict(filler.fill_state(H.mcq_specs(H.CT_CONV_CFG), 10), strict=False)
        weights.append({"model." + k: v.detach().cpu().contiguous() for k, v in m.state_dict().items()})
    torch.save({"state_dict": weights[0], "ema_state_dict": weights[1], "epoch": 0}, tmp_path / "both.ckpt")
    torch.save({"state_dict": weights[1], "epoch": 0}, tmp_path / "averaged.ckpt")
    for tool, extra in ((causal_graph, []), (apply_action, ["--steps", "1"])):
        def run(ckpt, *flags):
            out = tmp_path / f"{tool.__name__}_{ckpt}_{len(flags)}"
            tool.main(["-c", str(path), "--checkpoint", str(tmp_path / f"{ckpt}.ckpt"), "--out", str(out)] + extra + list(flags))
            return {f: open(out / f, "rb").read() for f in sorted(os.listdir(out))}          # every file the tool wrote
        with_flag, live, alone = run("both", "--ema"), run("both"), run("averaged")
        assert len(with_flag) >= 3 and with_flag == alone, tool.__name__
        differ = [f for f in with_flag if with_flag[f] != live[f]]
        assert [f for f in differ if f.endswith(".png")], (tool.__name__, differ)
