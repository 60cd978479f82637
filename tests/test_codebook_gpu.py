"""GPU: codebook usage statistics and dead-code restarts (``exp_params.codebook_stats`` / ``codebook_restart_every``) through the
training harness, the runner and a checkpoint: optim.CodebookUsage on csrc/vqusage.hip, its observer on the quantisers, its place
behind the optimizer step.

MCQVAE of configs/mcq_vae.yaml at B = 4 (P = 256 latent rows, C = 4, K = 64, Dc = 32) unless stated; one CTMCQVAE and one VQVAE
case.  The model has neither BatchNorm nor noise, so a quantisation of the test's own in front of a step (``_StepByStep``) leaves
the trajectory alone -- which the tests check, bit for bit -- and says what the step's own index search will find.  Everything
is integers and raw words and compared exactly; perplexity is float64 on both sides over at most 512 terms: relative 1e-12."""
import io
import json
import os

import numpy as np
import pytest
import torch
import yaml

from ctvae_amd import filler
from tests import helpers as H
from tests.test_ct_gpu import _FixedNoise, build_ct

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, P, C, KC, DC, D = 4, 256, 4, 64, 32, 128
SEED = 1320
EXP = {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 0.00025, "manual_seed": SEED}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _mcq(dev, poison=None):
    """The same weights on every call; ``poison`` = (c, k): that code row is set to 1e3, so it cannot win a search."""
    from ctvae_amd.models import vae_models
    m = vae_models["MCQVAE"](**{**H.MCQ_CFG, "hidden_dims": list(H.MCQ_CFG["hidden_dims"])})
    m.load_state_dict(filler.fill_state(H.mcq_specs(H.MCQ_CFG), SEED + 1))
    m = m.to(dev).train()
    if poison is not None:
        with torch.no_grad():
            m.vq_layer.quantizers[poison[0]].embedding.weight[poison[1]].fill_(1e3)
    return m


def _batches(dev, n, seed=4100):
    return [(filler.synthetic_batch(seed + i, B)[0].to(dev), torch.zeros(B, device=dev)) for i in range(n)]


def _snapshot(exp):
    torch.cuda.synchronize()
    opt = exp.optimizer
    return {"param": exp.model.flat_params.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(),
            "state": opt.state[:8].clone()}


def _assert_same(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (what, k)


def _quantise(model, x):
    """(host bincounts [C, K], latent rows [P, D] on the device) of one batch with the model's weights as they are, by the
    quantiser's own ``compute_inds`` -- with no observer attached."""
    from ctvae_amd import kernels as K
    assert model.vq_layer.usage_observer is None
    with torch.no_grad():
        lat = model.encode(x)[0]
        inds = model.vq_layer.compute_inds(lat)
        rows = K.to_nhwc(lat).reshape(-1, lat.size(1)).clone()
    inds = inds.reshape(inds.size(0), -1, inds.size(-2) * inds.size(-1)).cpu()
    n_codes = getattr(model.vq_layer, "num_embeddings", None) or model.vq_layer.K
    return torch.stack([torch.bincount(inds[:, c].reshape(-1), minlength=n_codes) for c in range(inds.size(1))]), rows


class _StepByStep:
    """A run without the keys, one ``fit()`` per batch, with ``_quantise`` in front of every batch: ``counts[i]`` and ``rows[i]``
    are what batch i's own index search finds and reads."""

    def __init__(self, exp):
        self.exp, self.counts, self.rows, self.epochs = exp, [], [], 0

    def run(self, batches):
        for b in batches:
            c, r = _quantise(self.exp.model, b[0])
            self.counts.append(c)
            self.rows.append(r)
            self.exp.fit(lambda: iter([b]), None, max_epochs=self.epochs + 1, start_epoch=self.epochs)
            self.epochs += 1
        return self


def _numpy_record(counts, prefix):
    """The statistics restated with NumPy: {key: value} per codebook."""
    rec = {}
    for i, row in enumerate(np.asarray(counts, dtype=np.float64)):
        p = row[row > 0] / row.sum()
        rec[f"{prefix}codebook_perplexity_{i}"] = float(np.exp(-(p * np.log(p)).sum()))
        rec[f"{prefix}codebook_usage_{i}"] = float((row > 0).sum()) / len(row)
        rec[f"{prefix}codebook_dead_{i}"] = int((row == 0).sum())
    return rec


def _assert_record(got, ref):
    for k, v in ref.items():
        if "perplexity" in k:
            assert abs(got[k] - v) <= 1e-12 * v, (k, got[k], v)
        else:
            assert got[k] == v, (k, got[k], v)


def _lines(log, key):
    return [r for r in map(json.loads, log.getvalue().splitlines()) if key in r]


# ---- 1. codebook_stats alone --------------------------------------------------------------------------------
def test_stats_alone_leave_training_alone_and_match_a_recount(dev):
    from ctvae_amd.experiment import VAEXperiment
    train, val = _batches(dev, 6), _batches(dev, 2, seed=4900)
    finals = {}
    for name, extra in (("plain", {}), ("stats", {"codebook_stats": True})):
        log = io.StringIO()
        exp = VAEXperiment(_mcq(dev), dict(EXP, **extra), log_file=log)
        calls = [0]

        def epoch_batches():
            lo = 3 * calls[0]
            calls[0] += 1
            return iter(train[lo:lo + 3])
        hist = exp.fit(epoch_batches, lambda: iter(val), max_epochs=2)
        finals[name] = _snapshot(exp)
        assert exp.global_step == 6 and exp.codebook is None and exp.model.vq_layer.usage_observer is None
        if name == "plain":
            assert exp.val_codebook is None and not any("codebook" in k for k in hist[1]) and not _lines(log, "val_codebook_usage")
            continue
        exp.model.eval()
        counts = sum(_quantise(exp.model, b[0])[0] for b in val)             # epoch 1 validated with the final weights
        assert int(counts.sum()) == 2 * P * C
        _assert_record(hist[1], _numpy_record(counts, "val_"))
        for stem in ("perplexity", "usage", "dead"):
            per = [hist[1][f"val_codebook_{stem}_{i}"] for i in range(C)]
            assert abs(hist[1][f"val_codebook_{stem}"] - sum(per) / C) <= 1e-12 * max(per)
        assert hist[0]["val_codebook_usage_0"] > 0 and "val_codebook_invalid" not in hist[1]
        logged = _lines(log, "val_codebook_usage")
        assert len(logged) == 2 and logged[1]["val_codebook_perplexity_3"] == hist[1]["val_codebook_perplexity_3"]
    _assert_same(finals["plain"], finals["stats"], "with and without codebook_stats")


# ---- 2. counting does not touch training --------------------------------------------------------------------
@pytest.mark.parametrize("hipgraph", [True, False])
def test_counting_leaves_training_alone_and_matches_a_recount(dev, hipgraph):
    """codebook_restart_every larger than the steps run: six steps (with hipGraph: three warm, the capture, two replays) end with
    the parameters and moments of a run without the key; the window's counts are the sum of the steps' own, the pool holds the last
    step's latents."""
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, 6)
    params = dict(EXP, hipgraph=hipgraph)
    plain = VAEXperiment(_mcq(dev), dict(params))
    plain.fit(lambda: iter(batches), None, max_epochs=1)
    keyed = VAEXperiment(_mcq(dev), dict(params, codebook_restart_every=1000))
    keyed.fit(lambda: iter(batches), None, max_epochs=1)
    ref = _StepByStep(VAEXperiment(_mcq(dev), dict(params))).run(batches)
    if hipgraph:
        for exp in (plain, keyed, ref.exp):
            gs = list(exp._graphed.values())
            assert len(gs) == 1 and gs[0].graph is not None and gs[0].seen == 6
    _assert_same(_snapshot(plain), _snapshot(keyed), "with and without codebook_restart_every")
    _assert_same(_snapshot(plain), _snapshot(ref.exp), "the recounting run left the trajectory")
    counts, invalid = keyed.codebook.read()
    assert invalid == 0 and torch.equal(counts, sum(ref.counts)) and int(counts.sum()) == 6 * P * C
    assert keyed.codebook.valid_rows == P and keyed.codebook_ordinal == 0 and keyed.last_codebook_restart is None
    assert torch.equal(keyed.codebook.pool[:P].view(torch.int32), ref.rows[-1].view(torch.int32))
    assert not keyed.codebook.pool[P:].any() and keyed.model.vq_layer.usage_observer is None
    sd = keyed.state_dict()["codebook"]
    assert torch.equal(sd["counts"], counts) and sd["valid_rows"] == P and sd["every"] == 1000 and sd["pool"] == 1024


# ---- 3. one restart ----------------------------------------------------------------------------------------
POISON = (2, 5)


@pytest.mark.parametrize("min_count", [1, 3])
def test_restart_after_step_two(dev, min_count):
    """One code row is 1e3, so no latent chooses it; every = 2.  After step 2 every dead row equals its pool slice
    pool[row][c : c + Dc) bitwise -- the pool being step 2's latents, the rows the stated draw -- its moments are zero, and
    every other word equals the run without the key.  With min_count 3 codes that were chosen (and have moments) restart too."""
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.optim import codebook_restart_rows
    batches = _batches(dev, 2)
    log = io.StringIO()
    extra = {"codebook_restart_every": 2} if min_count == 1 else {"codebook_restart_every": 2, "codebook_restart_min_count": min_count}
    keyed = VAEXperiment(_mcq(dev, POISON), dict(EXP, **extra), log_file=log)
    keyed.fit(lambda: iter(batches), None, max_epochs=1)
    ref = _StepByStep(VAEXperiment(_mcq(dev, POISON), dict(EXP))).run(batches)
    window = ref.counts[0] + ref.counts[1]
    dead = [(c, k) for c in range(C) for k in range(KC) if int(window[c, k]) < min_count]
    assert POISON in dead and 0 < len(dead) < C * KC
    rows = codebook_restart_rows(SEED, 0, len(dead), P)
    want = _snapshot(ref.exp)
    cb = keyed.codebook
    lo_p = (keyed.model.vq_layer.quantizers[0].embedding.weight.data_ptr() - keyed.model.flat_params.data_ptr()) // 4
    lo_m = lo_p - int(keyed.optimizer.slice.start or 0)
    moved = 0
    for (c, k), row in zip(dead, rows):
        at = (c * KC + k) * DC
        moved += int(want["exp_avg"][lo_m + at:lo_m + at + DC].ne(0).any())
        want["param"][lo_p + at:lo_p + at + DC] = ref.rows[1][row, c:c + DC]
        want["exp_avg"][lo_m + at:lo_m + at + DC] = 0
        want["exp_avg_sq"][lo_m + at:lo_m + at + DC] = 0
    if min_count == 3:
        assert moved > 0, "no restarted code had a moment to zero"
    _assert_same(want, _snapshot(keyed), "restart")
    w = keyed.model.vq_layer.quantizers[POISON[0]].embedding.weight[POISON[1]]
    assert torch.equal(w.detach(), cb.pool[rows[dead.index(POISON)], POISON[0]:POISON[0] + DC]) and float(w.detach().abs().max()) < 1e3
    counts, invalid = cb.read()
    assert not counts.any() and invalid == 0
    assert (keyed.codebook_ordinal, keyed.codebook_restarted, keyed.global_step) == (1, len(dead), 2)
    line, = _lines(log, "codebook_restarts")
    assert line == keyed.last_codebook_restart
    assert line["codebook_restarts"] == len(dead) and line["step"] == 1
    assert [line[f"codebook_restarts_{i}"] for i in range(C)] == [sum(1 for c, _ in dead if c == i) for i in range(C)]
    ref_rec = {k: v for k, v in _numpy_record(window, "").items() if "_dead_" not in k}
    _assert_record(line, ref_rec)
    assert set(line) == set(ref_rec) | {"codebook_restarts", "step"} | {f"codebook_restarts_{i}" for i in range(C)}


# ---- 4. captured and eager ---------------------------------------------------------------------------------
def test_captured_and_eager_runs_agree(dev):
    """Eight steps, every = 3: restarts behind steps 3 (eager in both) and 6 (behind a replay), two more steps counted."""
    from ctvae_amd.experiment import VAEXperiment
    batches = _batches(dev, 8)
    out = {}
    for hipgraph in (True, False):
        log = io.StringIO()
        exp = VAEXperiment(_mcq(dev, POISON), dict(EXP, hipgraph=hipgraph, codebook_restart_every=3, codebook_restart_min_count=3),
                           log_file=log)
        exp.fit(lambda: iter(batches), None, max_epochs=1)
        if hipgraph:
            gs = list(exp._graphed.values())
            assert len(gs) == 1 and gs[0].graph is not None and gs[0].seen == 8
        else:
            assert not exp._graphed
        out[hipgraph] = (_snapshot(exp), exp.codebook.read(), _lines(log, "codebook_restarts"), exp.codebook_restarted)
    _assert_same(out[True][0], out[False][0], "captured and eager")
    assert torch.equal(out[True][1][0], out[False][1][0]) and int(out[True][1][0].sum()) == 2 * P * C
    assert out[True][2] == out[False][2] and [r["step"] for r in out[True][2]] == [2, 5]
    assert out[True][3] == out[False][3] == sum(r["codebook_restarts"] for r in out[True][2]) > 0


# ---- 5. accumulate_grad_batches ----------------------------------------------------------------------------
@pytest.mark.parametrize("hipgraph", [True, False])
def test_every_micro_batch_counts_and_restarts_follow_optimizer_steps(dev, hipgraph):
    from ctvae_amd.experiment import VAEXperiment
    exp = VAEXperiment(_mcq(dev), dict(EXP, hipgraph=hipgraph, codebook_restart_every=1), accumulate_grad_batches=2)
    windows = []
    inner = exp.codebook.restart

    def spy(*a, **kw):
        res = inner(*a, **kw)
        windows.append(res[0])
        return res
    exp.codebook.restart = spy
    batches = _batches(dev, 4)
    exp.fit(lambda: iter(batches), None, max_epochs=1)
    assert exp.global_step == 2 and exp.codebook_ordinal == 2 and len(windows) == 2
    for w in windows:
        assert [int(v) for v in w.sum(dim=1)] == [2 * P] * C              # both micro-batches of the window, every codebook
    assert not exp.codebook.read()[0].any()


# ---- 6. the runner: save inside a window, resume -----------------------------------------------------------
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


def test_runner_resumes_inside_a_window_bit_exactly(dev, tmp_path):
    """Five steps per epoch, every = 3: the checkpoint of epoch 0 lies two steps into the window that step 6 ends."""
    from ctvae_amd import run
    keys = {"codebook_stats": True, "codebook_restart_every": 3, "codebook_restart_min_count": 20}
    last = lambda sub: tmp_path / sub / "MCQVAE" / "checkpoints" / "last.ckpt"
    steps = ["--steps-per-epoch", "5"]
    h2 = run.main(["-c", _runner_cfg(tmp_path, "straight", keys)] + steps + ["--max-epochs", "2"])
    run.main(["-c", _runner_cfg(tmp_path, "first", keys)] + steps + ["--max-epochs", "1"])
    hr = run.main(["-c", _runner_cfg(tmp_path, "resumed", keys, resume_from_checkpoint=str(last("first")))] + steps + ["--max-epochs", "2"])
    f = torch.load(last("first"), weights_only=True)["trainer"]["codebook"]
    assert (f["every"], f["min_count"], f["pool"], f["ordinal"]) == (3, 20, 1024, 1) and int(f["counts"].sum()) == 2 * 8 * 64 * C
    a, b = torch.load(last("straight"), weights_only=True), torch.load(last("resumed"), weights_only=True)
    ca, cb = a["trainer"]["codebook"], b["trainer"]["codebook"]
    assert torch.equal(ca["counts"], cb["counts"]) and int(ca["counts"].sum()) == 8 * 64 * C      # step 10 is one past step 9's restart
    assert {k: v for k, v in ca.items() if k != "counts"} == {k: v for k, v in cb.items() if k != "counts"}
    assert ca["ordinal"] == 3 and ca["restarted"] > f["restarted"] > 0
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(a["trainer"]["optimizer"][k], b["trainer"]["optimizer"][k]), k
    assert hr[0]["val_codebook_perplexity"] == h2[1]["val_codebook_perplexity"]
    recs = [json.loads(l) for l in open(tmp_path / "straight" / "MCQVAE" / "metrics_rank0.jsonl")]
    assert [r["step"] for r in recs if "codebook_restarts" in r] == [2, 5, 8]
    # a run without the keys ignores the entry and writes none
    run.main(["-c", _runner_cfg(tmp_path, "nokey", resume_from_checkpoint=str(last("first")))] + steps + ["--max-epochs", "2"])
    assert "codebook" not in torch.load(last("nokey"), weights_only=True)["trainer"]
    # under the key: other settings, or a checkpoint without the entry, are refused by name
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_restart_every.*first"):
        run.main(["-c", _runner_cfg(tmp_path, "bad", dict(keys, codebook_restart_every=4),
                                    resume_from_checkpoint=str(last("first")))] + steps + ["--max-epochs", "2"])
    with pytest.raises(SystemExit, match=r"exp_params\.codebook_restart_every.*nokey"):
        run.main(["-c", _runner_cfg(tmp_path, "bad", keys, resume_from_checkpoint=str(last("nokey")))] + steps + ["--max-epochs", "3"])
    assert not last("bad").exists()
    # load_weights_only starts a fresh window
    run.main(["-c", _runner_cfg(tmp_path, "wo", keys, resume_from_checkpoint=str(last("first")), load_weights_only=True),
              "--steps-per-epoch", "2", "--max-epochs", "1"])
    d = torch.load(last("wo"), weights_only=True)["trainer"]["codebook"]
    assert d["ordinal"] == 0 and d["restarted"] == 0 and int(d["counts"].sum()) == 2 * 8 * 64 * C


# ---- 7. CT-MCQ-VAE: statistics under update_parameters, no restarts ------------------------------------------
A = 12
CT_PARAMS = {"LR": 5e-4, "weight_decay": 0.0, "kld_weight": 0.00025, "update_parameters": "ct_layer", "hipgraph": False}


@pytest.fixture()
def fixed_noise(dev):
    from ctvae_amd.models import causal
    prev = causal.set_noise_source(_FixedNoise(dev))
    yield
    causal.set_noise_source(prev)


def _ct_batch(dev, seed, mode, actions=None):
    x, y, _ = filler.synthetic_pairs(seed, B, A)
    opts = {"mode": [mode] * B}
    if mode != "base":
        opts.update(input_y=y.to(dev), action=torch.nn.functional.one_hot(torch.tensor(actions), A).float().to(dev))
    return (x.to(dev), torch.zeros(B, device=dev), opts)


def test_ct_statistics_count_both_images_and_restart_is_refused(dev, fixed_noise):
    from ctvae_amd.experiment import VAEXperiment
    m = build_ct(dev, 5)
    with pytest.raises(ValueError, match="codebook_restart_every.*update_parameters='ct_layer'"):
        VAEXperiment(m, dict(CT_PARAMS, codebook_restart_every=2))
    exp = VAEXperiment(m, dict(CT_PARAMS, codebook_stats=True))
    val = [_ct_batch(dev, 300, "base"), _ct_batch(dev, 301, "action", [0, 3, 0, 3])]
    hist = exp.fit(lambda: iter([]), lambda: iter(val), max_epochs=1)
    m.eval()
    counts = _quantise(m, val[0][0])[0] + _quantise(m, val[1][0])[0] + _quantise(m, val[1][2]["input_y"])[0]
    assert tuple(counts.shape) == (1, 64) and int(counts.sum()) == 3 * B * 64           # x of the base batch, x and y of the pair
    _assert_record(hist[0], _numpy_record(counts, "val_"))
    assert hist[0]["val_codebook_usage"] == hist[0]["val_codebook_usage_0"] and m.vq_layer.usage_observer is None


# ---- 8. VQVAE: K = 512, a single-codebook quantiser ---------------------------------------------------------
def test_vqvae_statistics_and_one_restart(dev):
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    from ctvae_amd.optim import codebook_restart_rows

    def build():
        m = vae_models["VQVAE"](**{**H.VQVAE_CFG, "hidden_dims": list(H.VQVAE_CFG["hidden_dims"])})
        m.load_state_dict(filler.fill_state(H.vqvae_specs(), 77))
        return m.to(dev).train()
    batches, val = _batches(dev, 2), _batches(dev, 1, seed=4900)
    exp = VAEXperiment(build(), dict(EXP, codebook_stats=True, codebook_restart_every=2))
    hist = exp.fit(lambda: iter(batches), lambda: iter(val), max_epochs=1)
    ref = _StepByStep(VAEXperiment(build(), dict(EXP))).run(batches)
    cb = exp.codebook
    assert (cb.C, cb.K, cb.Dc, cb.D, cb.valid_rows) == (1, 512, 64, 64, 1024)
    window = ref.counts[0] + ref.counts[1]
    dead = [(0, k) for k in range(512) if int(window[0, k]) == 0]
    assert 0 < len(dead) < 512 and exp.codebook_restarted == len(dead) and exp.last_codebook_restart["codebook_restarts_0"] == len(dead)
    rows = codebook_restart_rows(SEED, 0, len(dead), 1024)
    assert torch.equal(cb.pool.view(torch.int32), ref.rows[1].view(torch.int32))
    want = _snapshot(ref.exp)
    lo_p = (exp.model.vq_layer.embedding.weight.data_ptr() - exp.model.flat_params.data_ptr()) // 4
    for (_, k), row in zip(dead, rows):
        want["param"][lo_p + k * 64:lo_p + (k + 1) * 64] = ref.rows[1][row]
        want["exp_avg"][lo_p + k * 64:lo_p + (k + 1) * 64] = 0
        want["exp_avg_sq"][lo_p + k * 64:lo_p + (k + 1) * 64] = 0
    _assert_same(want, _snapshot(exp), "VQVAE restart")
    exp.model.eval()
    _assert_record(hist[0], _numpy_record(_quantise(exp.model, val[0][0])[0], "val_"))
