"""GPU: the code prior end to end -- ``codeprior.MarkovCodePrior`` on csrc/codeprior.hip, ``exp_params.code_prior`` through the
training harness, and the ``fit_code_prior`` command on a checkpoint of that run.

MCQVAE of configs/mcq_vae.yaml at B = 4 (C = 4, K = 64, an 8 x 8 grid) and the reference's VQVAE(3, 64, 512) (C = 1, K = 512,
16 x 16), the models of tests/test_codebook_gpu.py.  Tables, samples, parameters and the pre-existing record keys are compared
exactly.  lambda after 20 EM rounds is float64 on both sides and differs by the summation order of the responsibilities: the
difference measured on the fixture is 2.2e-16 (MCQVAE's shape) and 1.1e-16 (VQVAE's), asserted at 100 times that."""
import io
import json
import os

import numpy as np
import pytest
import torch
import yaml

from ctvae_amd import filler
from tests import codeprior_checks as R
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1320
EXP = {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 0.00025, "manual_seed": SEED}
LAMBDA_BOUND = 100 * 2.2e-16                      # 100 times the measured difference; never looser than 1e-8
EXPERT_KEYS = [f"val_code_prior_weight_{e}" for e in ("uniform", "position", "left", "up", "previous")]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _build(name, dev):
    from ctvae_amd.models import vae_models
    if name == "MCQVAE":
        m = vae_models["MCQVAE"](**{**H.MCQ_CFG, "hidden_dims": list(H.MCQ_CFG["hidden_dims"])})
        m.load_state_dict(filler.fill_state(H.mcq_specs(H.MCQ_CFG), SEED + 1))
    else:
        m = vae_models["VQVAE"](**{**H.VQVAE_CFG, "hidden_dims": list(H.VQVAE_CFG["hidden_dims"])})
        m.load_state_dict(filler.fill_state(H.vqvae_specs(), 77))
    return m.to(dev).train()


def _batches(dev, n, seed=4100, bs=4):
    return [(filler.synthetic_batch(seed + i, bs)[0].to(dev), torch.zeros(bs, device=dev)) for i in range(n)]


def _snapshot(exp):
    torch.cuda.synchronize()
    opt = exp.optimizer
    return {"param": exp.model.flat_params.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone()}


def _prior_keys(rec):
    return {k: v for k, v in rec.items() if k.startswith("val_code_prior_")}


# ---- 1. the library on a known chain -------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 4, 8, 8), (512, 1, 16, 16)])
def test_two_fits_agree_bit_for_bit_and_lambda_follows_the_restatement(dev, shape, tmp_path):
    from ctvae_amd.codeprior import MarkovCodePrior, fit_halves
    K, C, H_, W = shape
    grids = R.chain_fixture(31 + K, 64, K, C, H_, W)
    x = torch.from_numpy(grids).to(dev)
    priors = []
    for _ in range(2):
        p = MarkovCodePrior(K, C, H_, W, dev)
        info = fit_halves(p, x, 20, 1e-3)
        assert info == {"rows": 32, "bad": 0} and p.rows == 32 and p.invalid == 0 and p.em_iters == 20
        g = torch.Generator(device=dev)
        g.manual_seed(9)
        priors.append((p, p.sample(5, g)))
    (a, sa), (b, sb) = priors
    for ta, tb in zip(a.tables, b.tables):
        assert torch.equal(ta, tb)
    assert np.array_equal(a.weights.view(np.int64), b.weights.view(np.int64)) and torch.equal(sa, sb)
    # against the restatement: the tables exactly, lambda within the measured bound
    ref_tables, ref_invalid = R.count(grids[0::2], K)
    for got, want in zip(a.tables, ref_tables):
        assert np.array_equal(got.cpu().numpy(), want)
    ref_lam = R.em(grids[1::2], ref_tables, K, 20, 1e-3)
    diff = float(np.abs(a.weights - ref_lam).max())
    print(f"{shape}: max |lambda - restatement| after 20 rounds = {diff:.3e}")
    assert LAMBDA_BOUND <= 1e-8 and diff <= LAMBDA_BOUND
    assert np.abs(a.weights.sum(axis=1) - 1).max() < 1e-14 and (a.weights[:, 0] >= 1e-3 * (1 - 1e-12)).all()
    # the samples are the restatement's for the device's own lambda and uniforms
    g = torch.Generator(device=dev)
    g.manual_seed(9)
    u = torch.rand(5, H_ * W, C, 2, generator=g, device=dev, dtype=torch.float64)
    assert np.array_equal(sa.cpu().numpy(), R.sample(ref_tables, a.weights, u.cpu().numpy(), H_, W))
    assert torch.equal(a.sample(5, u=u), sa)
    # held-out nats: the summary against the restatement, and far below ln K
    fresh = R.chain_fixture(77, 16, K, C, H_, W)
    s = a.summary(torch.from_numpy(fresh).to(dev))
    assert abs(s["nats_per_code"] - R.nats_per_code(fresh, ref_tables, a.weights, K)) <= 1e-12 * s["uniform_nats"]
    assert s["nats_per_code"] < s["uniform_nats"] - 0.5 and s["rows"] == 16 and s["bad"] == 0 and len(s["per_codebook"]) == C
    assert abs(s["bits_per_code"] * np.log(2.0) - s["nats_per_code"]) < 1e-12
    # save / load
    path = tmp_path / "p.npz"
    a.save(path)
    back = MarkovCodePrior.load(str(path), device=dev)
    assert (back.K, back.C, back.H, back.W, back.rows, back.em_iters, back.uniform_floor) == (K, C, H_, W, 32, 20, 1e-3)
    assert np.array_equal(back.weights.view(np.int64), a.weights.view(np.int64)) and torch.equal(back.sample(5, u=u), sa)
    assert sorted(np.load(path).files) == sorted(["pos", "left", "up", "prev", "lambda", "K", "C", "H", "W", "rows", "em_iters",
                                                  "uniform_floor"])
    assert open(path, "rb").read() == open(path, "rb").read() and back.state_dict()["pos"].dtype == np.int64


# ---- 2. the training hook ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["MCQVAE", "VQVAE"])
def test_hook_leaves_training_alone_and_writes_its_record_and_files(dev, tmp_path, name):
    from ctvae_amd.codeprior import MarkovCodePrior, grid_indices
    from ctvae_amd.experiment import VAEXperiment
    train, val = _batches(dev, 2), _batches(dev, 3, seed=4900)
    key = {"code_prior": {"type": "markov", "em_iters": 5}}
    runs = {"plain": {}, "keyed": key, "stats": {"codebook_stats": True}, "both": dict(key, codebook_stats=True)}
    finals, hists, rngs = {}, {}, {}
    for tag, extra in runs.items():
        log = io.StringIO()
        exp = VAEXperiment(_build(name, dev), dict(EXP, **extra), log_file=log, sample_dir=str(tmp_path / tag), run_name="run",
                           val_sampling=True)
        torch.manual_seed(5)
        hists[tag] = exp.fit(lambda: iter(train), lambda: iter(val), max_epochs=1, test_batches=lambda: iter(val))
        finals[tag] = _snapshot(exp)
        rngs[tag] = (torch.get_rng_state(), torch.cuda.get_rng_state(dev))
        assert exp.model.vq_layer.usage_observer is None and "code_prior" not in exp.state_dict()
        if "code_prior" not in extra:
            assert exp.val_code_prior is None and exp.last_code_prior is None and not _prior_keys(hists[tag][0])
            assert not (tmp_path / tag / "Priors").exists()
            assert not (tmp_path / tag / "Samples" / "sample_code_prior_run_Epoch_0.png").exists()
            assert "val_code_prior" not in log.getvalue()
            continue
        rec = _prior_keys(hists[tag][0])
        C = exp.val_code_prior.shape[0]
        assert set(rec) == {"val_code_prior_nats", "val_code_prior_bits", "val_code_prior_uniform_nats", "val_code_prior_rows",
                            "val_code_prior_invalid", *EXPERT_KEYS, *(f"val_code_prior_nats_{c}" for c in range(C))}
        assert rec["val_code_prior_rows"] == 6 and rec["val_code_prior_invalid"] == 0 and exp.val_code_prior.rows == 12
        assert abs(sum(rec[k] for k in EXPERT_KEYS) - 1) < 1e-12 and rec["val_code_prior_weight_uniform"] >= 1e-3 * (1 - 1e-12)
        assert rec["val_code_prior_uniform_nats"] == float(np.log(exp.model.num_embeddings))
        assert abs(rec["val_code_prior_nats"] - sum(rec[f"val_code_prior_nats_{c}"] for c in range(C)) / C) < 1e-12
        assert 0 < rec["val_code_prior_nats"] < rec["val_code_prior_uniform_nats"] + 1.0
        logged = [r for r in map(json.loads, log.getvalue().splitlines()) if "val_code_prior_nats" in r]
        assert len(logged) == 1 and logged[0]["val_code_prior_nats"] == rec["val_code_prior_nats"]
        # the buffer holds the validation indices of the final weights, in order; the record is a recount of them
        exp.model.eval()
        with torch.no_grad():
            want = torch.cat([grid_indices(exp.model, b[0]) for b in val])
        assert torch.equal(exp.val_code_prior.view(), want)
        saved = MarkovCodePrior.load(str(tmp_path / tag / "Priors" / "code_prior_run_Epoch_0.npz"), device=dev)
        ref_tables, _ = R.count(want.cpu().numpy()[0::2], saved.K)
        for got, t in zip(saved.tables, ref_tables):
            assert np.array_equal(got.cpu().numpy(), t)
        assert saved.rows == 6 and saved.em_iters == 5
        assert abs(saved.summary(want[1::2].contiguous())["nats_per_code"] - rec["val_code_prior_nats"]) < 1e-12
        sheet = tmp_path / tag / "Samples" / "sample_code_prior_run_Epoch_0.png"
        assert sheet.exists() and sheet.stat().st_size > 0
    for tag in ("keyed", "stats", "both"):
        for k in finals["plain"]:
            assert torch.equal(finals["plain"][k].view(torch.int32), finals[tag][k].view(torch.int32)), (tag, k)
        assert torch.equal(rngs["plain"][0], rngs[tag][0]) and torch.equal(rngs["plain"][1], rngs[tag][1])
        for k, v in hists["plain"][0].items():
            if k != "epoch_seconds":
                assert hists[tag][0][k] == v, (tag, k)
    # codebook_stats' numbers are what they were, and the chained observers saw the same searches
    stats_keys = [k for k in hists["stats"][0] if k.startswith("val_codebook_")]
    assert stats_keys and all(hists["both"][0][k] == hists["stats"][0][k] for k in stats_keys)
    assert _prior_keys(hists["both"][0]) == _prior_keys(hists["keyed"][0])
    if name == "MCQVAE":           # the model's own sample sheet is unchanged next to the new one
        own = [open(tmp_path / tag / "Samples" / "sample_run_Epoch_0.png", "rb").read() for tag in ("plain", "keyed")]
        assert own[0] == own[1]


def test_too_few_rows_leave_an_error_and_the_epoch_completes(dev, tmp_path):
    from ctvae_amd.experiment import VAEXperiment
    val = _batches(dev, 1, seed=4900, bs=1)
    exp = VAEXperiment(_build("MCQVAE", dev), dict(EXP, code_prior={"type": "markov"}), sample_dir=str(tmp_path), run_name="run",
                       val_sampling=True)
    hist = exp.fit(lambda: iter(_batches(dev, 1)), lambda: iter(val), max_epochs=1, test_batches=lambda: iter(val))
    rec = _prior_keys(hist[0])
    assert set(rec) == {"val_code_prior_error"} and "at least 2 rows" in rec["val_code_prior_error"]
    assert "val_loss" in hist[0] and exp.global_step == 1 and exp.last_code_prior is None
    assert not (tmp_path / "Priors").exists() and not (tmp_path / "Samples" / "sample_code_prior_run_Epoch_0.png").exists()


def test_unserved_model_and_bad_setting_are_refused_by_the_experiment(dev):
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    with pytest.raises(ValueError, match="code_prior needs a quantising model.*VanillaVAE"):
        VAEXperiment(vae_models["VanillaVAE"](in_channels=3, latent_dim=16), dict(EXP, code_prior={"type": "markov"}))
    with pytest.raises(ValueError, match="code_prior.em_iters"):
        VAEXperiment(_build("MCQVAE", dev), dict(EXP, code_prior={"type": "markov", "em_iters": 0}))


# ---- 3. the command ------------------------------------------------------------------------------------------
def _tool_cfg(tmp_path, name):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "mcq_vae.yaml")))
    if name == "VQVAE":
        cfg["model_params"] = dict(H.VQVAE_CFG, name="VQVAE", hidden_dims=list(H.VQVAE_CFG["hidden_dims"]))
        cfg["logging_params"]["name"] = "VQVAE"
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    cfg["data_params"]["train_batch_size"] = cfg["data_params"]["val_batch_size"] = 4
    p = tmp_path / f"{name}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p), cfg


@pytest.mark.parametrize("name", ["MCQVAE", "VQVAE"])
def test_command_writes_its_files_on_a_checkpoint_of_a_run(dev, tmp_path, name):
    from ctvae_amd import fit_code_prior
    from ctvae_amd.codeprior import MarkovCodePrior
    from ctvae_amd.experiment import VAEXperiment
    exp = VAEXperiment(_build(name, dev), dict(EXP, code_prior={"type": "markov", "em_iters": 2}))
    exp.fit(lambda: iter(_batches(dev, 2)), lambda: iter(_batches(dev, 1, seed=4900)), max_epochs=1)
    ckpt = tmp_path / "run.ckpt"
    torch.save({"state_dict": {"model." + k: v.detach().cpu().contiguous() for k, v in exp.model.state_dict().items()},
                "epoch": 0}, ckpt)
    cfg_path, cfg = _tool_cfg(tmp_path, name)
    out = tmp_path / "out"
    torch.manual_seed(123)
    before = (torch.get_rng_state(), torch.cuda.get_rng_state(dev))
    summary = fit_code_prior.main(["-c", cfg_path, "--checkpoint", str(ckpt), "--out", str(out), "--samples", "14",
                                   "--em-iters", "4"])
    assert torch.equal(torch.get_rng_state(), before[0]) and torch.equal(torch.cuda.get_rng_state(dev), before[1])
    files = fit_code_prior.FILES + ((fit_code_prior.NOISE_FILE,) if name == "MCQVAE" else ())
    assert sorted(os.listdir(out)) == sorted(files) and len(files) == (4 if name == "MCQVAE" else 3)
    on_disk = json.load(open(out / "code_prior.json"))
    assert on_disk == json.loads(json.dumps(summary))
    assert {"fit", "train", "test", "weights", "experts", "rows", "invalid", "arguments"} == set(on_disk)
    K = cfg["model_params"]["num_embeddings"]
    C = cfg["model_params"].get("codebooks", 1)
    for split in ("train", "test"):
        s = on_disk[split]
        assert {"nats_per_code", "bits_per_code", "uniform_nats", "per_codebook", "rows", "bad"} == set(s)
        assert s["uniform_nats"] == float(np.log(K)) and len(s["per_codebook"]) == C and s["bad"] == 0 and s["nats_per_code"] > 0
    assert on_disk["rows"] == 16 and on_disk["train"]["rows"] == 16 and on_disk["test"]["rows"] == 32 and on_disk["invalid"] == 0
    assert on_disk["arguments"]["em_iters"] == 4 and len(on_disk["weights"]) == C
    assert all(abs(sum(row) - 1) < 1e-12 and row[0] >= 1e-3 * (1 - 1e-12) for row in on_disk["weights"])
    prior = MarkovCodePrior.load(str(out / "code_prior.npz"), device=dev)
    assert (prior.K, prior.C, prior.rows, prior.em_iters) == (K, C, 16, 4)
    assert [[float(v) for v in row] for row in prior.weights] == on_disk["weights"]
    assert int(prior.tables[0].sum()) == 16 * C * prior.H * prior.W
    for f in files:
        assert (out / f).stat().st_size > 0
    # the default directory, --rows
    capped = fit_code_prior.main(["-c", cfg_path, "--checkpoint", str(ckpt), "--rows", "6", "--samples", "3", "--em-iters", "1"])
    d = tmp_path / "logs" / cfg["logging_params"]["name"] / "fit_code_prior"
    assert sorted(os.listdir(d)) == sorted(files) and capped["rows"] == 3 and capped["train"]["rows"] == 3
