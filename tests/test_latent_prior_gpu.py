"""GPU: the sample prior (``exp_params.sample_prior``) through the training harness, and the tool on a checkpoint:
latentprior.GaussianMixturePrior on csrc/gmm.hip, fed by ``validation_step`` with ``BaseVAE.gaussian_posterior``.

BetaTCVAE (latent_dim 10) with ``covariance: full`` at B = 8 and six validation batches -- 24 fitted and 24 held-out rows -- and
VanillaVAE (latent_dim 128) with ``covariance: diag`` at B = 4 and eight batches, both with two components, on
``filler.synthetic_batch``.  The reference is the float64 restatement of tests/prior_checks.py on the very tensors the harness
handed to the code buffer (a spy on ``append``):

* from shared state -- the held-out rows under the parameters the run saved -- the record's likelihoods must hold the project's
  fp32 parity bound, 1e-4 relative;
* after the restatement's own full loop from the same start the final mean log-likelihood gets ``LOOP_MARGIN``, four times the
  deviation measured on the MI355X for these two cases (EM amplifies the kernels' fp32 rounding through the assignments)."""
import io
import json
import os

import numpy as np
import pytest
import torch
import yaml

from ctvae_amd import filler
from tests import helpers as H
from tests import prior_checks as PC
from tests.test_grad_accum_gpu import EXP, _assert_same, _snapshot, _vanilla
from tests.test_latent_stats_gpu import _epochs, _lines, _png_size, _save, _tool_cfg

pytestmark = pytest.mark.gpu
RTOL = 1e-4
LOOP_MEASURED = {"BetaTCVAE": 6.15e-6, "VanillaVAE": 4.32e-7}       # |record - restatement's loop| / |restatement's|, MI355X
LOOP_MARGIN = {k: 4 * v for k, v in LOOP_MEASURED.items()}          # (7 resp. 4 iterations on both sides)
RECORD = {"val_prior_" + k for k in ("mixture_loglik", "standard_loglik", "iterations", "rows", "nonfinite")}
CASES = {"BetaTCVAE": (8, 6, {"type": "gmm", "components": 2, "covariance": "full"}),
         "VanillaVAE": (4, 8, {"type": "gmm", "components": 2, "covariance": "diag"})}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _model(name, dev):
    if name == "VanillaVAE":
        return _vanilla(dev)
    from ctvae_amd.models import vae_models
    m = vae_models["BetaTCVAE"](**H.BETATC_CFG)
    m.load_state_dict(filler.fill_state(H.betatc_specs(), 1401))
    return m.to(dev).train()


def _mk(dev, n, bs, seed):
    return [(filler.synthetic_batch(seed + i, bs)[0].to(dev), torch.zeros(bs, device=dev)) for i in range(n)]


def _spy(exp, seen):
    inner = exp.val_prior.append

    def append(codes):
        seen.append(codes.detach().clone())
        inner(codes)
    exp.val_prior.append = append


def _prior_keys(rec):
    return {k: v for k, v in rec.items() if k.startswith("val_prior_")}


# ---- 1. the record, the log, the files ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_record_log_and_files(dev, tmp_path, name):
    from ctvae_amd import latentprior as LP
    from ctvae_amd.experiment import VAEXperiment
    bs, nval, cfg = CASES[name]
    train, val = _mk(dev, 2, bs, 5100), _mk(dev, nval, bs, 5900)
    log, seen = io.StringIO(), []
    exp = VAEXperiment(_model(name, dev), dict(EXP, sample_prior=cfg), log_file=log, sample_dir=str(tmp_path), run_name="run")
    _spy(exp, seen)
    torch.manual_seed(5)                # (BetaTCVAE's training noise comes from the device's generator)
    hist = exp.fit(_epochs(train, 1), lambda: iter(val), max_epochs=2)
    D = exp.model.latent_dim
    assert len(seen) == 2 * nval and all(tuple(c.shape) == (bs, D) for c in seen)
    rec = _prior_keys(hist[1])
    print(name, rec)
    assert set(rec) == RECORD
    rows = nval * bs // 2
    assert rec["val_prior_rows"] == rows and rec["val_prior_nonfinite"] == 0 and 1 <= rec["val_prior_iterations"] <= 50
    lines = _lines(log, "val_prior_rows")
    assert len(lines) == 2 and {k: v for k, v in lines[1].items() if k != "step"} == rec and lines[1]["step"] == 2
    # the tensors handed over in epoch 1: even ordinals are fitted, odd ordinals held out
    X = torch.cat(seen[nval:]).cpu().numpy()
    fitted, held = X[0::2], X[1::2]
    assert len(fitted) == rows and len(held) == rows
    std = PC.standard_log_prob(held).mean()
    assert abs(rec["val_prior_standard_loglik"] - std) <= 1e-12 * abs(std)
    # from shared state: the saved parameters, which round-trip through load
    path = tmp_path / "Priors" / "latent_prior_run_Epoch_1.npz"
    assert sorted(os.listdir(tmp_path / "Priors")) == ["latent_prior_run_Epoch_0.npz", "latent_prior_run_Epoch_1.npz"]
    saved = np.load(path)
    assert sorted(saved.files) == sorted(["weights", "means", "covariances", "covariance_type", "reg_covar", "rows", "iterations",
                                          "converged"])
    assert saved["weights"].dtype == saved["means"].dtype == saved["covariances"].dtype == np.float64
    assert saved["covariance_type"].tolist() == [cfg["covariance"]] and saved["rows"].tolist() == [rows]
    assert saved["iterations"].tolist() == [rec["val_prior_iterations"]] and saved["reg_covar"].tolist() == [1e-6]
    loaded = LP.GaussianMixturePrior.load(str(path), device=dev)
    again = loaded.state_dict()
    assert all(np.array_equal(again[k], saved[k]) for k in saved.files)
    w, mu, c = saved["weights"], saved["means"], saved["covariances"]
    shared = PC.mean_log_prob(held, w, mu, c, cfg["covariance"])
    e_shared = abs(rec["val_prior_mixture_loglik"] - shared) / abs(shared)
    ll, bad = loaded.log_prob(torch.from_numpy(held).to(dev))
    assert loaded.mean_over_finite(ll, bad) == rec["val_prior_mixture_loglik"]
    # the restatement's own loop from the same start
    init = PC.default_start(fitted, 2, exp.epoch_seed(1), cfg["covariance"], 1e-6)
    rw, rmu, rc, info = PC.fit(fitted, init, cfg["covariance"], 1e-6, max_iter=50, tol=1e-3)
    loop = PC.mean_log_prob(held, rw, rmu, rc, cfg["covariance"])
    e_loop = abs(rec["val_prior_mixture_loglik"] - loop) / abs(loop)
    print(f"{name}: mixture {rec['val_prior_mixture_loglik']:.6f} shared-state {shared:.6f} ({e_shared:.2e}) restatement's loop "
          f"{loop:.6f} ({e_loop:.2e}); iterations {rec['val_prior_iterations']} / {info['iterations']}; standard {std:.4f}")
    assert e_shared <= RTOL
    assert e_loop <= LOOP_MARGIN[name]


# ---- 2. the mixture sheet next to the prior's --------------------------------------------------------------
def test_mixture_sheet_has_the_grid_size(dev, tmp_path):
    from ctvae_amd.experiment import VAEXperiment
    bs, nval, cfg = CASES["BetaTCVAE"]
    train, val = _mk(dev, 1, bs, 5100), _mk(dev, nval, bs, 5900)
    sheets = {}
    for key, extra in (("plain", {}), ("prior", {"sample_prior": cfg})):
        exp = VAEXperiment(_model("BetaTCVAE", dev), dict(EXP, **extra), sample_dir=str(tmp_path / key), run_name="run", val_sampling=True)
        torch.manual_seed(5)            # (BetaTCVAE's training noise comes from the device's generator)
        exp.fit(lambda: iter(train), lambda: iter(val), max_epochs=1, test_batches=lambda: iter(val))
        sheets[key] = open(tmp_path / key / "Samples" / "sample_run_Epoch_0.png", "rb").read()
    assert sheets["plain"] == sheets["prior"]                               # the prior's own sheet is unchanged
    assert not (tmp_path / "plain" / "Samples" / "sample_mixture_run_Epoch_0.png").exists()
    mix = tmp_path / "prior" / "Samples" / "sample_mixture_run_Epoch_0.png"
    assert _png_size(mix) == _png_size(tmp_path / "prior" / "Samples" / "sample_run_Epoch_0.png")


# ---- 3. training does not notice; codes: sample moves no other stream --------------------------------------
@pytest.mark.parametrize("hipgraph", [True, False])
def test_training_is_bit_for_bit_the_same(dev, tmp_path, hipgraph):
    from ctvae_amd.experiment import VAEXperiment
    bs, nval, cfg = CASES["VanillaVAE"]
    train, val = _mk(dev, 4, bs, 4100), _mk(dev, nval, bs, 4900)
    finals, rngs, recs = {}, {}, {}
    for key, extra in (("plain", {}), ("mean", {"sample_prior": cfg}), ("sample", {"sample_prior": dict(cfg, codes="sample")})):
        log = io.StringIO()
        exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=hipgraph, **extra), log_file=log, sample_dir=str(tmp_path / key),
                           run_name="run")
        torch.manual_seed(5)
        hist = exp.fit(_epochs(train, 2), lambda: iter(val), max_epochs=2)
        assert exp.global_step == 4
        finals[key] = _snapshot(exp)
        rngs[key] = (exp.model._rng_state.clone(), torch.get_rng_state(), torch.cuda.get_rng_state(dev))
        recs[key] = hist[1]
        if key == "plain":             # no buffer, no file, no key
            assert exp.val_prior is None and exp.sample_prior is None and not (tmp_path / key).exists()
            assert not any("prior" in k for k in hist[1]) and not _lines(log, "val_prior_rows")
        else:
            assert hist[1]["val_prior_rows"] == nval * bs // 2 and (tmp_path / key / "Priors").is_dir()
    for key in ("mean", "sample"):
        _assert_same(finals["plain"], finals[key], f"with and without sample_prior ({key})")
        for a, b in zip(rngs["plain"], rngs[key]):
            assert torch.equal(a, b)
        for k, v in recs["plain"].items():         # every validation key that existed keeps its value
            if k != "epoch_seconds":
                assert recs[key][k] == v, k
    assert recs["mean"]["val_prior_mixture_loglik"] != recs["sample"]["val_prior_mixture_loglik"]


# ---- 4. a refused fit --------------------------------------------------------------------------------------
def test_refused_fit_leaves_an_error_and_the_epoch_completes(dev, tmp_path):
    from ctvae_amd.experiment import VAEXperiment
    bs, nval, cfg = CASES["BetaTCVAE"]
    train, val = _mk(dev, 1, bs, 5100), _mk(dev, nval, bs, 5900)
    log = io.StringIO()
    exp = VAEXperiment(_model("BetaTCVAE", dev), dict(EXP, sample_prior=dict(cfg, components=64)), log_file=log,
                       sample_dir=str(tmp_path), run_name="run", val_sampling=True)
    hist = exp.fit(lambda: iter(train), lambda: iter(val), max_epochs=1, test_batches=lambda: iter(val))
    rec = _prior_keys(hist[0])
    assert set(rec) == {"val_prior_error"} and "24" in rec["val_prior_error"] and "64" in rec["val_prior_error"]
    assert "val_loss" in hist[0] and exp.global_step == 1
    lines = _lines(log, "val_prior_error")
    assert len(lines) == 1 and isinstance(lines[0]["val_prior_error"], str)
    assert not (tmp_path / "Priors").exists() and not (tmp_path / "Samples" / "sample_mixture_run_Epoch_0.png").exists()
    assert (tmp_path / "Samples" / "sample_run_Epoch_0.png").exists()


def test_unsupported_model_and_bad_setting_are_refused(dev):
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    name, cfg, _ = H.IW_CASES["iwae"]
    with pytest.raises(ValueError, match="sample_prior needs a model.*IWAE"):
        VAEXperiment(vae_models[name](**cfg), dict(EXP, sample_prior={"type": "gmm"}))
    with pytest.raises(ValueError, match="sample_prior.components"):
        VAEXperiment(_vanilla(dev), dict(EXP, sample_prior={"type": "gmm", "components": 0}))


# ---- 5. the library's fit against the restatement's, through fit(init=...) ----------------------------------
@pytest.mark.parametrize("case", [c[0] for c in PC.GOLDEN_CASES])
def test_fit_from_a_given_start_follows_scikit_learn(dev, golden, case):
    """Six iterations at tol = 0 from the recorded start: the library against what scikit-learn ended with (and so against the
    restatement, which equals it to 1e-10).  The data are well separated enough for EM not to amplify: the fp32 parity bound."""
    from ctvae_amd import latentprior as LP
    g = golden("gmm_sklearn")
    _, N, D, K, cov = next(c for c in PC.GOLDEN_CASES if c[0] == case)
    prior = LP.GaussianMixturePrior(D, K, covariance=cov, reg_covar=1e-6, device=dev)
    X = torch.from_numpy(g[case + "_X"]).to(dev)
    info = prior.fit(X, seed=0, max_iter=6, tol=0.0, init=(g[case + "_w0"], g[case + "_mu0"], g[case + "_cov0"]))
    assert info["iterations"] == 6 and not info["converged"] and info["rows"] == N and info["nonfinite"] == 0
    assert len(info["loglik_trace"]) == 6 and all(b >= a - 1e-4 * abs(a) for a, b in zip(info["loglik_trace"], info["loglik_trace"][1:]))
    errs = {k: float(np.abs(getattr(prior, a).numpy() - g[f"{case}_{k}"]).max() / np.abs(g[f"{case}_{k}"]).max())
            for k, a in (("w", "weights"), ("mu", "means"), ("cov", "covariances"))}
    ll, bad = prior.log_prob(X)
    score = prior.mean_over_finite(ll, bad)
    errs["score"] = abs(score - float(g[case + "_score"])) / abs(float(g[case + "_score"]))
    print(case, errs)
    assert max(errs.values()) <= RTOL
    again = LP.GaussianMixturePrior(D, K, covariance=cov, reg_covar=1e-6, device=dev)
    again.fit(X, seed=0, max_iter=6, tol=0.0, init=(g[case + "_w0"], g[case + "_mu0"], g[case + "_cov0"]))
    for a in ("weights", "means", "covariances"):                          # two fits of the same data are bit-identical
        assert torch.equal(getattr(prior, a), getattr(again, a))


def test_fit_refusals_and_the_default_start(dev):
    from ctvae_amd import latentprior as LP
    X = torch.from_numpy(PC.blobs(3, 40, 5, 2)).to(dev)
    prior = LP.GaussianMixturePrior(5, 3, device=dev)
    with pytest.raises(ValueError, match="at least 2"):
        prior.fit(X[:1], seed=0)
    with pytest.raises(ValueError, match="2 finite rows cannot carry 3 components"):
        prior.fit(X[:2], seed=0)
    bad = X.clone()
    bad[3:, 0] = float("nan")
    with pytest.raises(ValueError, match="3 finite rows cannot carry 4"):
        LP.GaussianMixturePrior(5, 4, device=dev).fit(bad, seed=0)
    w0, mu0, c0 = LP.GaussianMixturePrior(5, 2, device=dev).default_start(X, seed=1)
    c0[1] = -c0[1]                                      # not positive definite
    with pytest.raises(ValueError, match="component 1.*larger reg_covar or covariance: diag"):
        LP.GaussianMixturePrior(5, 2, device=dev).fit(X, seed=0, init=(w0, mu0, c0))
    # the default start: K distinct finite rows, the data's covariance, uniform weights -- the restatement's
    Xn = X.clone()
    Xn[7, 2] = float("inf")
    w, mu, c = prior.default_start(Xn, seed=11)
    rw, rmu, rc = PC.default_start(Xn.cpu().numpy(), 3, 11, "full", 1e-6)
    assert np.array_equal(mu.numpy(), rmu) and np.array_equal(w.numpy(), rw)
    assert np.abs(c.numpy() - rc).max() <= RTOL * np.abs(rc).max()
    info = prior.fit(Xn, seed=11)
    assert info["rows"] == 39 and info["nonfinite"] == 1 and np.isfinite(info["loglik_trace"]).all()
    z, k = prior.sample(64, torch.Generator(device=dev).manual_seed(1))
    assert tuple(z.shape) == (64, 5) and torch.isfinite(z).all() and int(k.min()) >= 0 and int(k.max()) < 3
    z2, k2 = prior.sample(64, torch.Generator(device=dev).manual_seed(1))
    assert torch.equal(z, z2) and torch.equal(k, k2)


# ---- 6. the tool -------------------------------------------------------------------------------------------
def test_tool_writes_its_four_files(dev, tmp_path):
    from ctvae_amd import fit_prior, latentprior as LP
    from ctvae_amd.experiment import VAEXperiment
    exp = VAEXperiment(_vanilla(dev), dict(EXP, LR=1e-2, hipgraph=False, ema_decay=0.5))
    exp.fit(_epochs(_mk(dev, 4, 4, 4100), 2), None, max_epochs=2)
    plain, both = tmp_path / "plain.ckpt", tmp_path / "both.ckpt"
    _save(exp.model, plain)
    _save(exp.model, both, ema=exp.ema_model_state_dict())
    cfg_path, cfg = _tool_cfg(tmp_path, "vae.yaml")
    with pytest.raises(SystemExit, match="fit_prior: --ema.*plain.ckpt holds no ema_state_dict"):
        fit_prior.main(["-c", cfg_path, "--checkpoint", str(plain), "--ema"])
    swae_path, _ = _tool_cfg(tmp_path, "swae.yaml")
    with pytest.raises(SystemExit, match="fit_prior: model_params.name is 'SWAE'.*VanillaVAE"):
        fit_prior.main(["-c", swae_path, "--checkpoint", str(plain)])
    assert not (tmp_path / "logs").exists()
    out = tmp_path / "out"
    args = ["--components", "2", "--covariance", "diag", "--max-iter", "20"]
    torch.manual_seed(123)
    before = (torch.get_rng_state(), torch.cuda.get_rng_state(dev))
    summary = fit_prior.main(["-c", cfg_path, "--checkpoint", str(both), "--out", str(out), "--samples", "14"] + args)
    assert torch.equal(torch.get_rng_state(), before[0]) and torch.equal(torch.cuda.get_rng_state(dev), before[1])
    assert sorted(os.listdir(out)) == sorted(fit_prior.FILES)
    on_disk = json.load(open(out / "latent_prior.json"))
    assert on_disk == json.loads(json.dumps(summary))
    assert {"fit", "train_loglik_mixture", "train_loglik_standard", "test_loglik_mixture", "test_loglik_standard", "weights",
            "arguments"} == set(on_disk)
    assert set(on_disk["fit"]) == {"iterations", "converged", "loglik_trace", "rows", "nonfinite"}
    assert on_disk["fit"]["rows"] == 8 * 4 and on_disk["fit"]["nonfinite"] == 0 and len(on_disk["weights"]) == 2
    assert abs(sum(on_disk["weights"]) - 1) < 1e-12 and on_disk["arguments"]["components"] == 2
    assert on_disk["train_loglik_mixture"] > on_disk["train_loglik_standard"]     # a mixture fitted to the rows beats N(0, I) on them
    prior = LP.GaussianMixturePrior.load(str(out / "latent_prior.npz"), device=dev)
    assert prior.covariance == "diag" and prior.rows == 32 and [float(w) for w in prior.weights] == on_disk["weights"]
    assert _png_size(out / "samples_standard.png") == _png_size(out / "samples_mixture.png") == (12 * 66 + 2, 2 * 66 + 2)
    # default output directory, the averaged weights, a cap on the rows: other numbers
    ema = fit_prior.main(["-c", cfg_path, "--checkpoint", str(both), "--ema", "--rows", "20", "--samples", "3"] + args)
    d = tmp_path / "logs" / cfg["logging_params"]["name"] / "fit_prior"
    assert sorted(os.listdir(d)) == sorted(fit_prior.FILES) and ema["fit"]["rows"] == 20
    assert ema["test_loglik_mixture"] != summary["test_loglik_mixture"]
