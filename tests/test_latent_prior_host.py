"""CPU: the float64 restatement of the Gaussian-mixture prior (tests/prior_checks.py) against what scikit-learn's
``GaussianMixture`` ended with (tests/golden/gmm_sklearn.npz, recorded by tools/gen_gmm_golden.py; live where scikit-learn
imports), ``exp_params.sample_prior`` and its refusals, the supported models, the sampling rule, and what the tool refuses without
a device."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import prior_checks as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 0.00025}
ATOL = 1e-10                       # absolute, on parameters of order 1 (a probe gave <= 2e-12 for this construction, D up to 128)
SUPPORTED = {"VanillaVAE", "VAE", "GaussianVAE", "BetaVAE", "LogCoshVAE", "DIPVAE", "MSSIMVAE", "TwoStageVAE", "InfoVAE", "VampVAE",
             "BetaTCVAE"}


# ---- the restatement is scikit-learn's algorithm ---------------------------------------------------------------
@pytest.mark.parametrize("case", [c[0] for c in PC.GOLDEN_CASES])
def test_restatement_equals_the_recorded_scikit_learn_results(golden, case):
    g = golden("gmm_sklearn")
    _, N, D, K, cov = next(c for c in PC.GOLDEN_CASES if c[0] == case)
    X = g[case + "_X"]
    assert X.dtype == np.float32 and X.shape == (N, D)
    data_seed, start_seed = PC.GOLDEN_SEEDS[case]
    assert np.array_equal(X, PC.blobs(data_seed, N, D, K))                       # the generator's inputs are reproducible here
    init = PC.blob_start(X, K, start_seed, cov)
    for got, key in zip(init, ("_w0", "_mu0", "_cov0")):
        assert np.array_equal(got, g[case + key])
    w, mu, c, info = PC.fit(X, init, cov, reg_covar=1e-6, max_iter=6, tol=0.0)
    assert info["iterations"] == 6 and not info["converged"] and len(info["states"]) == 6
    score = PC.mean_log_prob(X, w, mu, c, cov)
    errs = [np.abs(w - g[case + "_w"]).max(), np.abs(mu - g[case + "_mu"]).max(), np.abs(c - g[case + "_cov"]).max(),
            abs(score - float(g[case + "_score"]))]
    print(case, errs)
    assert max(errs) <= ATOL
    assert abs(w.sum() - 1) < 1e-14
    if cov == "full":
        assert max(np.linalg.cond(ck) for ck in c) < 1e4


@pytest.mark.parametrize("cov", ["full", "diag"])
def test_restatement_equals_scikit_learn_live(cov):
    pytest.importorskip("sklearn")
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_gmm_golden as G
    finally:
        sys.path.pop(0)
    N, D, K = 1500, 128, 4
    X = PC.blobs(41, N, D, K)
    init = PC.blob_start(X, K, 3, cov)
    sw, smu, sc, sscore = G.sklearn_fit(X, init, cov)
    w, mu, c, _ = PC.fit(X, init, cov, reg_covar=1e-6, max_iter=6, tol=0.0)
    errs = [np.abs(w - sw).max(), np.abs(mu - smu).max(), np.abs(c - sc).max(), abs(PC.mean_log_prob(X, w, mu, c, cov) - sscore)]
    print(cov, errs)
    assert max(errs) <= ATOL


def test_the_centred_single_pass_is_the_two_pass_covariance():
    """The M step centred at the OLD means equals the textbook one centred at the new means, wherever the old means lie."""
    X = PC.blobs(5, 300, 6, 3).astype(np.float64) + 50.0                        # far from the origin: an uncentred pass would cancel
    init = PC.blob_start(X, 3, 1, "full")
    r, _, bad = PC.estep(X, *init, "full")
    w, mu, c = PC.mstep(X, r, bad, init[1], "full", 1e-6)
    w2, mu2, c2 = PC.mstep(X, r, bad, init[1] + 7.0, "full", 1e-6)              # another centre, the same result
    nk = r.sum(axis=0)
    for k in range(3):
        d = X - (r[:, k] @ X) / nk[k]
        two_pass = (r[:, k, None] * d).T @ d / nk[k] + 1e-6 * np.eye(6)
        assert np.abs(c[k] - two_pass).max() < 1e-11 and np.abs(c2[k] - two_pass).max() < 1e-10
    assert np.abs(mu - mu2).max() < 1e-12 and np.abs(w - nk / 300).max() < 1e-14


def test_estep_flags_nonfinite_rows_and_mstep_leaves_them_out():
    X = PC.blobs(6, 50, 4, 2).astype(np.float64)
    init = PC.blob_start(X, 2, 2, "diag")
    Xb = X.copy()
    Xb[3, 1], Xb[10, 0] = np.nan, np.inf
    r, ll, bad = PC.estep(Xb, *init, "diag")
    assert bad.tolist() == [1 if i in (3, 10) else 0 for i in range(50)]
    assert (r[[3, 10]] == 0).all() and (ll[[3, 10]] == 0).all() and np.allclose(r[bad == 0].sum(axis=1), 1.0, atol=1e-14)
    keep = np.ones(50, bool)
    keep[[3, 10]] = False
    want = PC.mstep(X[keep], r[keep], bad[keep], init[1], "diag", 1e-6)
    got = PC.mstep(Xb, r, bad, init[1], "diag", 1e-6)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert abs(got[0].sum() - 1) < 1e-14                                         # N_finite, not N


# ---- sampling ---------------------------------------------------------------------------------------------------
def test_sampling_picks_the_first_index_whose_cdf_exceeds_u():
    w = np.array([0.2, 0.0, 0.3, 0.5])
    cdf = np.cumsum(w)
    u = np.array([0.0, 0.1999999, 0.2, 0.2000001, 0.4999999, 0.5, 0.99, np.nextafter(1.0, 0.0)])
    k = PC.component_of(u, w)
    assert k.tolist() == [0, 0, 2, 2, 2, 3, 3, 3]                                # u == cdf[k] goes on; the empty component is never drawn
    assert all(cdf[ki] > ui and (ki == 0 or cdf[ki - 1] <= ui) for ki, ui in zip(k, u))
    assert PC.component_of(np.array([0.9999999]), np.array([0.5, 0.4999998])).tolist() == [1]       # a cdf that ends below 1
    rng = np.random.default_rng(0)
    X = PC.blobs(7, 80, 3, 2)
    _, mu, c = PC.blob_start(X, 4, 0, "full")
    eps = rng.normal(size=(len(u), 3))
    z, kz = PC.sample(u, eps, w, mu, c, "full")
    assert np.array_equal(kz, k)
    L = np.linalg.cholesky(c)
    for i in range(len(u)):
        assert np.allclose(z[i], mu[k[i]] + L[k[i]] @ eps[i], rtol=0, atol=1e-13)
    zd, _ = PC.sample(u, eps, w, mu, np.stack([np.diag(ck) for ck in c]), "diag")
    assert np.allclose(zd, mu[k] + np.sqrt(np.stack([np.diag(ck) for ck in c]))[k] * eps, rtol=0, atol=1e-13)


# ---- exp_params.sample_prior ------------------------------------------------------------------------------------
def test_setting_case_by_case():
    from ctvae_amd.latentprior import SETTING_DEFAULTS, prior_setting
    assert prior_setting(None) is None
    assert prior_setting({"type": "gmm"}) == {"type": "gmm", "components": 10, "covariance": "full", "max_iter": 50, "tol": 1e-3,
                                              "reg_covar": 1e-6, "codes": "mean"}
    assert set(SETTING_DEFAULTS) == {"components", "covariance", "max_iter", "tol", "reg_covar", "codes"}
    full = {"type": "gmm", "components": 64, "covariance": "diag", "max_iter": 1, "tol": 0, "reg_covar": 1, "codes": "sample"}
    got = prior_setting(full)
    assert got == dict(full, tol=0.0, reg_covar=1.0) and isinstance(got["tol"], float) and isinstance(got["reg_covar"], float)
    bad = [(True, "mapping"), ("gmm", "mapping"), ([], "mapping"), ({}, r"sample_prior\.type"), ({"type": "kde"}, r"sample_prior\.type"),
           ({"type": "gmm", "component": 3}, "unknown field.*component"), ({"type": "gmm", "seed": 1}, "unknown field.*seed")]
    for field, values in (("components", (0, 65, -1, True, 2.0, "3", None)), ("covariance", ("tied", "spherical", True, 1, None)),
                          ("max_iter", (0, -5, True, 1.5, "10", None)), ("tol", (-1e-9, True, "0", float("nan"), float("inf"), None)),
                          ("reg_covar", (0, 0.0, -1e-6, True, "1e-6", float("nan"), float("inf"), None)),
                          ("codes", ("mu", True, 0, None))):
        bad += [({"type": "gmm", field: v}, rf"sample_prior\.{field}") for v in values]
    for value, match in bad:
        with pytest.raises(ValueError, match=match):
            prior_setting(value)


def test_supported_models_over_the_whole_registry():
    from ctvae_amd.latentprior import PRIOR_MODELS, needs_supported_model, prior_supported
    from ctvae_amd.latentstats import has_gaussian_posterior
    from ctvae_amd.models import vae_models
    assert {n for n, cls in vae_models.items() if prior_supported(cls)} == SUPPORTED
    assert {vae_models[n].__name__ for n in SUPPORTED} == set(PRIOR_MODELS)
    for name, cls in vae_models.items():
        if prior_supported(cls):
            assert has_gaussian_posterior(cls), name                             # the codes come from gaussian_posterior
        else:
            msg = needs_supported_model(cls)
            assert msg.startswith("sample_prior needs a model") and msg.endswith("got " + cls.__name__)
    for name in ("IWAE", "MIWAE", "ConditionalVAE", "JointVAE", "MCQVAE", "VQVAE", "CTMCQVAE", "WAE_MMD", "SWAE", "HVAE", "LVAE",
                 "GammaVAE", "CategoricalVAE"):
        assert name in vae_models and not prior_supported(vae_models[name]), name
    assert needs_supported_model(None, name="'Nope'").endswith("got 'Nope'")


def test_experiment_builds_nothing_without_the_key_and_refuses_by_name():
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    vanilla = vae_models["VanillaVAE"](in_channels=3, latent_dim=16)
    exp = VAEXperiment(vanilla, dict(PARAMS))
    assert exp.sample_prior is None and exp.val_prior is None and exp.last_prior is None
    assert exp._prior_report not in exp._val_reports()
    exp = VAEXperiment(vanilla, dict(PARAMS, sample_prior={"type": "gmm", "components": 3}))
    assert exp.sample_prior["components"] == 3 and exp.val_prior.D == 16 and exp.val_prior._buf is None     # no buffer before a use
    assert exp._val_reports()[-1] == exp._prior_report
    for bad in (True, "gmm", {"type": "gmm", "components": 0}):
        with pytest.raises(ValueError, match="sample_prior"):
            VAEXperiment(vanilla, dict(PARAMS, sample_prior=bad))
    for name, cfg in (("WAE_MMD", None), ("HVAE", "hvae.yaml"), ("GammaVAE", "gammavae.yaml"), ("IWAE", None)):
        mp = yaml.safe_load(open(os.path.join(ROOT, "configs", cfg)))["model_params"] if cfg else dict(name=name, in_channels=3, latent_dim=16)
        with pytest.raises(ValueError, match=f"sample_prior needs a model.*got {name}"):
            VAEXperiment(vae_models[name](**mp), dict(PARAMS, sample_prior={"type": "gmm"}))


def test_code_buffer_and_library_refuse_on_the_host():
    from ctvae_amd import kernels as K
    from ctvae_amd import latentprior as LP
    buf = LP.CodeBuffer(3, "cpu", capacity=4)          # (the buffer itself is plain torch: its growth is checked here)
    rows = [torch.arange(3 * n, dtype=torch.float32).reshape(n, 3) + 100 * i for i, n in enumerate((2, 1, 3, 7, 1))]
    caps = []
    for r in rows:
        buf.append(r)
        caps.append(buf._buf.size(0))
    assert caps == [4, 4, 8, 16, 16] and buf.rows == 14 and torch.equal(buf.view(), torch.cat(rows))
    buf.clear()
    assert buf.rows == 0 and buf.view().shape == (0, 3)
    with pytest.raises(ValueError, match=r"\[B, 3\]"):
        buf.append(torch.zeros(2, 4))
    for D, Kc in ((0, 2), (257, 2), (4, 0), (4, 65), (True, 2)):
        with pytest.raises(ValueError):
            LP.GaussianMixturePrior(D, Kc, device="cpu")
    with pytest.raises(ValueError, match="covariance"):
        LP.GaussianMixturePrior(4, 2, covariance="tied", device="cpu")
    prior = LP.GaussianMixturePrior(4, 2, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        prior.fit(torch.zeros(8, 4), seed=0)
    with pytest.raises(RuntimeError, match="fit or load"):
        prior.state_dict()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.gmm_estep(torch.zeros(4, 3), torch.zeros(2), torch.zeros(2, 3), torch.ones(2, 3), torch.zeros(2), full=False)
    with pytest.raises(ValueError, match="N >= K"):
        K.gmm_mstep(torch.zeros(2, 3), torch.zeros(2, 5), None, torch.zeros(5, 3), full=False)
    # finish_mstep is the restatement's mfinish
    rng = np.random.default_rng(1)
    Nk, S1, m = rng.random(3) * 10, rng.normal(size=(3, 4)), rng.normal(size=(3, 4))
    A = rng.normal(size=(3, 4, 4))
    S2 = A @ np.swapaxes(A, 1, 2) * 10
    for full, s2 in ((True, S2), (False, np.stack([np.diag(a) for a in S2]))):
        got = LP.finish_mstep(Nk, S1, s2, m, full, 1e-3)
        want = PC.mfinish(Nk, S1, s2, m, "full" if full else "diag", 1e-3)
        assert all(np.allclose(g.numpy(), w, rtol=0, atol=1e-13) for g, w in zip(got, want))
    # state round trip (the parameters are host tensors)
    prior._set(np.array([0.25, 0.75]), rng.normal(size=(2, 4)), np.stack([np.eye(4), 2 * np.eye(4)]))
    sd = prior.state_dict()
    other = LP.GaussianMixturePrior(4, 2, device="cpu")
    other.load_state_dict(sd)
    assert all(np.array_equal(other.state_dict()[k], v) for k, v in sd.items())
    with pytest.raises(ValueError, match="is diag, the state is full"):
        LP.GaussianMixturePrior(4, 2, covariance="diag", device="cpu").load_state_dict(sd)


# ---- the runner and the tool ------------------------------------------------------------------------------------
def _config(tmp_path, name, exp=None):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["exp_params"].update(exp or {})
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_refuses_by_name(tmp_path):
    from ctvae_amd import run
    for bad in (True, "gmm", {"type": "kde"}, {"type": "gmm", "components": 2.0}, {"type": "gmm", "extra": 1},
                {"type": "gmm", "reg_covar": 0}):
        with pytest.raises(SystemExit, match=r"exp_params\.sample_prior"):
            run.main(["-c", _config(tmp_path, "vae.yaml", exp={"sample_prior": bad})])
    for cfg, name in (("mcq_vae.yaml", "MCQVAE"), ("lvae.yaml", "LVAE"), ("hvae.yaml", "HVAE"), ("gammavae.yaml", "GammaVAE"),
                      ("swae.yaml", "SWAE"), ("cvae.yaml", "ConditionalVAE")):
        with pytest.raises(SystemExit, match=rf"exp_params\.sample_prior needs a model.*{name}"):
            run.main(["-c", _config(tmp_path, cfg, exp={"sample_prior": {"type": "gmm"}})])
    assert not (tmp_path / "logs").exists()
    for cfg in ("vae.yaml", "betatc_vae.yaml", "vampvae.yaml", "mssim_vae.yaml"):
        on = run.exp_sample_prior(yaml.safe_load(open(_config(tmp_path, cfg, exp={"sample_prior": {"type": "gmm", "components": 4}}))))
        assert on["components"] == 4 and on["max_iter"] == 50
        assert run.exp_sample_prior(yaml.safe_load(open(_config(tmp_path, cfg)))) is None


def test_command_refuses_with_a_reason(tmp_path):
    from ctvae_amd import fit_prior
    for cfg, name in (("mcq_vae.yaml", "MCQVAE"), ("swae.yaml", "SWAE"), ("cvae.yaml", "ConditionalVAE")):
        with pytest.raises(SystemExit, match=f"fit_prior: .*{name}.*sample_prior needs a model"):
            fit_prior.main(["-c", _config(tmp_path, cfg)])
    with pytest.raises(SystemExit, match="fit_prior: no checkpoint"):
        fit_prior.main(["-c", _config(tmp_path, "vae.yaml")])
    missing = str(tmp_path / "missing.ckpt")
    with pytest.raises(SystemExit, match="missing.ckpt does not exist"):
        fit_prior.main(["-c", _config(tmp_path, "vae.yaml"), "--checkpoint", missing])
    for flag, bad in (("--components", "0"), ("--components", "65"), ("--covariance", "tied"), ("--max-iter", "0"), ("--tol", "-1"),
                      ("--tol", "nan"), ("--reg-covar", "0"), ("--codes", "mu"), ("--rows", "1"), ("--samples", "0")):
        with pytest.raises(SystemExit, match="fit_prior: " + flag):
            fit_prior.main(["-c", _config(tmp_path, "vae.yaml"), "--checkpoint", missing, flag, bad])
    ckpt = tmp_path / "plain.ckpt"
    torch.save({"state_dict": {}, "epoch": 0}, ckpt)
    with pytest.raises(SystemExit, match="--ema.*plain.ckpt holds no ema_state_dict"):
        fit_prior.main(["-c", _config(tmp_path, "vae.yaml"), "--checkpoint", str(ckpt), "--ema"])
    assert not os.path.exists(tmp_path / "logs")                    # nothing was written
