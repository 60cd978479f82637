"""Host side of the latent statistics (``exp_params.latent_stats``; ctvae_amd/latentstats.py, latent_stats.py): ``summarize``
against NumPy's own covariance, correlation and log-determinant, the ranking and the traversal rows, the settings validator, the
model hook on stub results, and the refusals of the experiment, the runner and the tool.  No GPU: nothing here launches a
kernel.  ``summarize`` and the references are float64 over the same sums in another order (one pass against two): they agree
to a relative 1e-9 of the magnitudes involved, eight digits below anything a wrong formula would give."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import latent_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"LR": 1e-3, "weight_decay": 0.0, "kld_weight": 1.0, "manual_seed": 11}
VANILLA_FAMILY = ("VanillaVAE", "BetaVAE", "LogCoshVAE", "DIPVAE", "MSSIMVAE", "TwoStageVAE", "VampVAE", "IWAE", "MIWAE")
OTHERS = ("MCQVAE", "VQVAE", "CTMCQVAE", "LVAE", "HVAE", "GammaVAE", "WAE_MMD", "SWAE", "CategoricalVAE")


# ---- the restatement ---------------------------------------------------------------------------------------
def test_ref_accumulate_is_the_row_order_loop():
    mu, lv = C.inputs(1, 5, 3)
    st = C.ref_accumulate(C.new_state(3), mu, lv)
    kl = np.zeros(3)
    cov = np.zeros((3, 3))
    for r in range(5):
        for d in range(3):
            m, v = float(mu[r, d]), float(lv[r, d])
            kl[d] = kl[d] + 0.5 * (((m * m + np.exp(v)) - v) - 1.0)
            for e in range(3):
                cov[d, e] = cov[d, e] + m * float(mu[r, e])
    assert np.array_equal(st["kl_sum"], kl) and np.array_equal(st["cov_sum"], cov) and st["rows"].tolist() == [5]
    assert np.array_equal(st["cov_sum"], st["cov_sum"].T) and st["nonfinite"].tolist() == [0, 0, 0]
    two = C.ref_accumulate(C.ref_accumulate(C.new_state(3), mu[:2], lv[:2]), mu[2:], lv[2:])
    assert all(np.array_equal(two[k], st[k]) for k in C.KEYS)
    bad_mu, bad_lv = mu.copy(), lv.copy()
    bad_mu[1, 0], bad_lv[3, 2], bad_lv[4, 2] = np.nan, np.inf, -np.inf
    bad = C.ref_accumulate(C.new_state(3), bad_mu, bad_lv)
    assert bad["nonfinite"].tolist() == [1, 0, 2] and np.isnan(bad["mu_sum"][0]) and np.isinf(bad["sig2_sum"][2])


# ---- summarize ---------------------------------------------------------------------------------------------
def _close(a, b, scale=1.0):
    return np.all(np.abs(np.asarray(a) - np.asarray(b)) <= 1e-9 * scale)


def test_summarize_matches_numpy():
    from ctvae_amd import latentstats as S
    B, L = 200, 6
    mu, lv = C.inputs(2, B, L, constant_col=4)
    mu[:, 1] = (0.8 * mu[:, 0] + 0.6 * mu[:, 1]).astype(np.float32)          # correlated with column 0
    mu[:, 5] *= np.float32(0.05)                                             # alive but not active: variance 0.0025
    res = S.summarize(C.ref_accumulate(C.new_state(L), mu, lv))
    m64, lv64 = mu.astype(np.float64), lv.astype(np.float64)
    kl = (0.5 * (m64 * m64 + np.exp(lv64) - lv64 - 1.0)).mean(axis=0)
    assert res["rows"] == B and res["nonfinite"] == 0
    assert _close(res["kl"], kl, kl.max()) and _close(res["kl_total"], kl.sum(), kl.sum())
    assert _close(res["mu_mean"], m64.mean(axis=0)) and _close(res["sigma2_mean"], np.exp(lv64).mean(axis=0), 8.0)
    cov = np.cov(m64, rowvar=False)
    assert res["cov"].shape == (L, L) and _close(res["cov"], cov) and _close(res["mu_var"], np.diag(cov))
    # the collapsed column: exactly nothing
    assert res["kl"][4] == 0.0 and res["mu_var"][4] == 0.0 and res["mu_mean"][4] == 0.0 and res["sigma2_mean"][4] == 1.0
    assert res["collapsed"] == 1 and res["active_units"] == 4
    active = [0, 1, 2, 3]
    corr = np.corrcoef(m64[:, [0, 1, 2, 3, 5]], rowvar=False)
    assert _close(res["corr"][np.ix_([0, 1, 2, 3, 5], [0, 1, 2, 3, 5])], corr)
    assert not res["corr"][4].any() and not res["corr"][:, 4].any()           # zero row and column where the variance is 0
    ca = np.abs(corr[:4, :4])
    assert _close(res["mean_abs_corr"], (ca.sum() - 4.0) / 12.0)
    assert res["corr"][0, 1] > 0.7
    sub = cov[np.ix_(active, active)]
    sign, logdet = np.linalg.slogdet(sub)
    assert sign > 0 and _close(res["gaussian_tc"], 0.5 * (np.log(np.diag(sub)).sum() - logdet))
    assert res["gaussian_tc"] > 0.3                                           # columns 0 and 1: -0.5 log(1 - 0.8^2) = 0.51
    assert set(S.record(res)) == {"val_latent_" + k for k in S.RECORD_KEYS}
    assert S.record(res)["val_latent_active_units"] == 4


def test_summarize_leaves_out_what_is_undefined():
    from ctvae_amd import latentstats as S
    mu, lv = C.inputs(3, 1, 4)
    one = S.summarize(C.ref_accumulate(C.new_state(4), mu, lv))
    assert sorted(one) == ["collapsed", "kl", "kl_total", "nonfinite", "rows"] and one["rows"] == 1
    assert S.summarize(C.new_state(4)) == {"rows": 0, "nonfinite": 0}
    # one active dimension: the pairwise entries have nothing to say
    mu, lv = C.inputs(4, 50, 3)
    mu[:, 1:] = 0.0
    few = S.summarize(C.ref_accumulate(C.new_state(3), mu, lv))
    assert few["active_units"] == 1 and "mean_abs_corr" not in few and "gaussian_tc" not in few and "cov" in few
    assert set(S.record(few)) == {"val_latent_" + k for k in ("kl_total", "active_units", "collapsed", "nonfinite", "rows")}
    mu, lv = C.inputs(5, 8, 2)
    mu[2, 0] = np.nan
    assert S.summarize(C.ref_accumulate(C.new_state(2), mu, lv))["nonfinite"] == 1


def test_rank_dims_breaks_ties_towards_the_lower_index():
    from ctvae_amd.latentstats import rank_dims
    assert rank_dims([0.5, 2.0, 0.5, 2.0, 0.0, 3.0], 4) == [5, 1, 3, 0]
    assert rank_dims([0.5, 2.0, 0.5, 2.0, 0.0, 3.0], 10) == [5, 1, 3, 0, 2, 4]
    assert rank_dims([1.0, 1.0, 1.0], 2) == [0, 1] and rank_dims([1.0], 0) == []


def test_traversal_latents_element_by_element():
    from ctvae_amd.latentstats import traversal_latents
    mu = torch.tensor([0.5, -1.0, 2.0, 7.0])
    dims, values = [2, 0, 2], [-3.0, 0.0, 3.0, 4.5]
    z = traversal_latents(mu, dims, values)
    assert tuple(z.shape) == (12, 4) and z.dtype == mu.dtype
    for r, d in enumerate(dims):
        for s, v in enumerate(values):
            for e in range(4):
                assert z[r * 4 + s, e].item() == (v if e == d else mu[e].item()), (r, s, e)
    assert mu.tolist() == [0.5, -1.0, 2.0, 7.0]                              # the input is not written
    assert tuple(traversal_latents(np.zeros((1, 3), np.float32), [1], np.linspace(-1, 1, 5)).shape) == (5, 3)
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        traversal_latents(mu, [4], values)


# ---- the settings and the model hook -------------------------------------------------------------------------
def test_setting_is_a_bool():
    from ctvae_amd.latentstats import latent_stats_setting
    assert latent_stats_setting(None) is False and latent_stats_setting(False) is False and latent_stats_setting(True) is True
    for bad in (1, 0, "true", 1.0, [True]):
        with pytest.raises(ValueError, match="latent_stats"):
            latent_stats_setting(bad)


def _results(n, B, L, lead=()):
    """n distinct tensors; entry i is filled with i; entries of the posterior get the lead axes."""
    return [torch.full((B,) + lead + (L,), float(i)) for i in range(n)]


def test_gaussian_posterior_positions_and_shapes():
    from ctvae_amd.models import vae_models
    B, L = 3, 5
    for name in VANILLA_FAMILY + ("BetaTCVAE", "ConditionalVAE"):
        mu, lv = vae_models[name].gaussian_posterior(None, _results(6, B, L))
        assert tuple(mu.shape) == (B, L) and mu[0, 0].item() == 2.0 and lv[0, 0].item() == 3.0, name
    for name in ("InfoVAE", "JointVAE"):
        mu, lv = vae_models[name].gaussian_posterior(None, _results(6, B, L))
        assert tuple(mu.shape) == (B, L) and mu[0, 0].item() == 3.0 and lv[0, 0].item() == 4.0, name
    # IWAE [B, S, L] and MIWAE [B, M, S, L]: expanded views, as their forward builds them -- index 0 on every middle axis, no copy
    base_mu, base_lv = torch.arange(B * L, dtype=torch.float32).view(B, L), -torch.arange(B * L, dtype=torch.float32).view(B, L)
    for name, lead in (("IWAE", (4,)), ("MIWAE", (2, 4))):
        ones = (1,) * len(lead)
        res = [None, None, base_mu.view((B,) + ones + (L,)).expand((B,) + lead + (L,)),
               base_lv.view((B,) + ones + (L,)).expand((B,) + lead + (L,))]
        mu, lv = vae_models[name].gaussian_posterior(None, res)
        assert tuple(mu.shape) == (B, L) and torch.equal(mu, base_mu) and torch.equal(lv, base_lv), name
        assert mu.data_ptr() == base_mu.data_ptr() and mu.stride() == (L, 1), name
    for name in OTHERS:
        assert vae_models[name].gaussian_posterior(None, _results(6, B, L)) is None, name


def test_experiment_builds_nothing_without_the_key_and_refuses_by_name():
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    vanilla = vae_models["VanillaVAE"](in_channels=3, latent_dim=16)
    exp = VAEXperiment(vanilla, dict(PARAMS))
    assert exp.latent_stats is False and exp.val_latents is None
    exp = VAEXperiment(vanilla, dict(PARAMS, latent_stats=True))
    assert exp.latent_stats is True and exp.val_latents.L == 16 and exp.val_latents._buf is None      # no buffer before a use
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        exp.val_latents.zero()
    for bad in (1, "yes", 0.5):
        with pytest.raises(ValueError, match="latent_stats"):
            VAEXperiment(vanilla, dict(PARAMS, latent_stats=bad))
    torch.manual_seed(7)
    mcq = vae_models["MCQVAE"](in_channels=3, embedding_dim=16, hidden_dims=[8, 16], num_embeddings=8, img_size=64, codebooks=4)
    with pytest.raises(ValueError, match="latent_stats.*Gaussian posterior.*MCQVAE"):
        VAEXperiment(mcq, dict(PARAMS, latent_stats=True))
    assert VAEXperiment(mcq, dict(PARAMS, latent_stats=False)).val_latents is None
    for name in ("LVAE", "HVAE", "GammaVAE"):
        cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", {"LVAE": "lvae.yaml", "HVAE": "hvae.yaml", "GammaVAE": "gammavae.yaml"}[name])))
        model = vae_models[name](**cfg["model_params"])
        with pytest.raises(ValueError, match=f"latent_stats.*Gaussian posterior.*{name}"):
            VAEXperiment(model, dict(PARAMS, latent_stats=True))


def test_kernel_wrapper_refuses_on_the_host():
    from ctvae_amd import kernels as K
    state = {k: torch.from_numpy(v) for k, v in C.new_state(4).items()}
    mu, lv = torch.zeros(3, 4), torch.zeros(3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.latent_accumulate(mu, lv, state)
    with pytest.raises(ValueError, match="log_var must be a torch.float32"):
        K.latent_accumulate(mu, lv.double(), state)
    with pytest.raises(ValueError, match="one shape"):
        K.latent_accumulate(mu, torch.zeros(3, 5), state)
    with pytest.raises(ValueError, match=r"mu must be a torch.float32 \[B, L\]"):
        K.latent_accumulate(torch.zeros(3, 2, 4), lv, state)
    with pytest.raises(ValueError, match="cov_sum must be"):
        K.latent_accumulate(mu, lv, dict(state, cov_sum=torch.zeros(4, 5, dtype=torch.float64)))
    with pytest.raises(ValueError, match="nonfinite must be a torch.int32"):
        K.latent_accumulate(mu, lv, dict(state, nonfinite=torch.zeros(4, dtype=torch.int64)))
    with pytest.raises(ValueError, match="1 <= L <= 1024"):
        K.latent_accumulate(torch.zeros(1, 1025), torch.zeros(1, 1025), state)


# ---- the runner and the tool ---------------------------------------------------------------------------------
def _config(tmp_path, name, exp=None, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["trainer_params"].update(trainer)
    cfg["exp_params"].update(exp or {})
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_refuses_by_name(tmp_path):
    from ctvae_amd import run
    for bad in (1, "on", 2.5):
        with pytest.raises(SystemExit, match=r"exp_params\.latent_stats"):
            run.main(["-c", _config(tmp_path, "vae.yaml", exp={"latent_stats": bad})])
    for cfg, name in (("mcq_vae.yaml", "MCQVAE"), ("lvae.yaml", "LVAE"), ("hvae.yaml", "HVAE"), ("gammavae.yaml", "GammaVAE")):
        with pytest.raises(SystemExit, match=rf"exp_params\.latent_stats.*Gaussian posterior.*{name}"):
            run.main(["-c", _config(tmp_path, cfg, exp={"latent_stats": True})])
    assert not (tmp_path / "logs").exists()
    for cfg in ("vae.yaml", "betatc_vae.yaml", "cvae.yaml"):
        assert run.exp_latent_stats(yaml.safe_load(open(_config(tmp_path, cfg, exp={"latent_stats": True})))) is True
        assert run.exp_latent_stats(yaml.safe_load(open(_config(tmp_path, cfg)))) is False


def test_command_refuses_with_a_reason(tmp_path):
    from ctvae_amd import latent_stats
    with pytest.raises(SystemExit, match="latent_stats: .*MCQVAE.*Gaussian posterior"):
        latent_stats.main(["-c", _config(tmp_path, "mcq_vae.yaml")])
    with pytest.raises(SystemExit, match="no checkpoint"):
        latent_stats.main(["-c", _config(tmp_path, "vae.yaml")])
    missing = str(tmp_path / "missing.ckpt")
    with pytest.raises(SystemExit, match="missing.ckpt does not exist"):
        latent_stats.main(["-c", _config(tmp_path, "vae.yaml"), "--checkpoint", missing])
    for flag, bad in (("--traverse", "-1"), ("--steps", "0"), ("--span", "0"), ("--span", "nan"), ("--image-index", "-2")):
        with pytest.raises(SystemExit, match=flag):
            latent_stats.main(["-c", _config(tmp_path, "vae.yaml"), "--checkpoint", missing, flag, bad])
    ckpt = tmp_path / "plain.ckpt"
    torch.save({"state_dict": {}, "epoch": 0}, ckpt)
    with pytest.raises(SystemExit, match="--ema.*plain.ckpt holds no ema_state_dict"):
        latent_stats.main(["-c", _config(tmp_path, "vae.yaml"), "--checkpoint", str(ckpt), "--ema"])
    assert not os.path.exists(tmp_path / "logs")                    # nothing was written
