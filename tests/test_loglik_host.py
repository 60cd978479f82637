"""CPU: the importance-sampled log-likelihood's host side -- the float64 restatement of tests/loglik_checks.py against itself
(``np.logaddexp``, the chunk cuts, K = 1, Jensen, the linear-Gaussian closed form), ``loglik.loglik_setting`` and the flags of
``python -m ctvae_amd.log_likelihood``, the model lists, ``run.py``'s refusal, and the refusals every checkpoint command shares."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

from tests import loglik_checks as C
from tests import test_tool_host as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = "VanillaVAE, BetaVAE, LogCoshVAE, DIPVAE, MSSIMVAE, TwoStageVAE, InfoVAE, BetaTCVAE, IWAE, MIWAE"
NEEDS = ("log_likelihood needs a model with a Gaussian posterior, a standard-normal prior and a decoder that takes "
         f"[n, latent_dim] latents alone ({MODELS}), got ")
COMMAND = ("vae.yaml", "mcq_vae.yaml", None, "model_params.name is 'MCQVAE': " + NEEDS + "'MCQVAE'")
CLOSED = dict(seed=11, P=48, L=4, sigma=0.5)          # the closed-form case tests/test_loglik_ops_gpu.py runs on the device


def _far_weights(seed, B=4, K=24):
    """Log-weights around -1e5 with a spread of 1e3: exp() of any of them is 0."""
    rng = np.random.default_rng(seed)
    return -1e5 + 1e3 * rng.standard_normal((B, K))


# ---- 1. the restatement against itself ---------------------------------------------------------------------
def test_finish_of_merge_is_logsumexp():
    lw = _far_weights(1)
    loglik, elbo, ess = C.estimate(lw)
    want = np.logaddexp.reduce(lw, axis=1) - math.log(lw.shape[1])
    assert np.all(np.abs(loglik - want) <= 1e-13 * np.abs(want))
    assert np.all(np.abs(elbo - lw.mean(1)) <= 1e-13 * np.abs(lw.mean(1)))
    w = np.exp(lw - lw.max(1, keepdims=True))
    assert np.all(np.abs(ess - w.sum(1) ** 2 / (w * w).sum(1)) <= 1e-12 * ess)
    assert np.all(ess >= 1.0) and np.all(ess <= lw.shape[1])
    assert np.all(loglik >= elbo)                                # Jensen, per image


def test_sequential_merge_does_not_depend_on_the_cut():
    lw = _far_weights(2)
    states = [C.merge_cut(lw, cut) for cut in C.CUTS]
    for st, fl in states[1:]:
        assert st.tobytes() == states[0][0].tobytes() and fl.tobytes() == states[0][1].tobytes()
    up, down = np.sort(lw, axis=1), np.sort(lw, axis=1)[:, ::-1]          # every step rescales / none after the first does
    for order in (up, down):
        got = [C.merge_cut(order, cut)[0].tobytes() for cut in C.CUTS]
        assert got[0] == got[1] == got[2]
        want = np.logaddexp.reduce(order, axis=1) - math.log(order.shape[1])
        assert np.all(np.abs(C.finish(C.merge_cut(order, [24])[0])[0] - want) <= 1e-13 * np.abs(want))


def test_one_sample_is_the_elbo():
    lw = _far_weights(3, K=1)
    loglik, elbo, ess = C.estimate(lw)
    assert np.array_equal(loglik, lw[:, 0]) and np.array_equal(elbo, lw[:, 0]) and np.array_equal(ess, np.ones(len(lw)))


def test_nonfinite_weights_flag_their_image_only():
    lw = _far_weights(4)
    bad = lw.copy()
    bad[1, 5], bad[2, 0] = np.nan, np.inf
    st, fl = C.merge_cut(bad, [1, 7, 16])
    clean, _ = C.merge_cut(lw, [1, 7, 16])
    assert fl.tolist() == [0, 1, 1, 0] and st[[0, 3]].tobytes() == clean[[0, 3]].tobytes()
    assert st[1, 4] == 23 and st[2, 4] == 23                     # the bad weight is not merged


def test_linear_gaussian_weights_equal_the_closed_form():
    case = C.linear_gaussian(**CLOSED)
    K = 32
    eps = np.random.default_rng(5).standard_normal((3, K, CLOSED["L"]))
    lw, _, _ = C.linear_gaussian_log_weights(case, eps)
    assert np.all(np.abs(lw - case["logpx"][:, None]) <= 1e-10 * np.abs(case["logpx"][:, None]))
    loglik, elbo, ess = C.estimate(lw)
    assert np.all(np.abs(ess - K) <= 1e-9 * K)
    assert np.all(np.abs(loglik - case["logpx"]) <= 1e-10 * np.abs(case["logpx"]))


def test_the_closed_form_case_survives_fp32():
    """What the device test asks of the library, on the host first: z and xhat formed and stored in fp32, the weights in float64
    over them, stay within the fp32 parity bound of log p(x) and keep ess >= K (1 - 1e-3)."""
    case = C.linear_gaussian(**CLOSED)
    K = 32
    eps = np.random.default_rng(5).standard_normal((3, K, CLOSED["L"])).astype(np.float32)
    lw, _, _ = C.linear_gaussian_log_weights(case, eps, dtype=np.float32)
    loglik, _, ess = C.estimate(lw)
    print("fp32 closed form: rel err", np.abs(loglik - case["logpx"]) / np.abs(case["logpx"]), "ess", ess)
    assert np.all(np.abs(loglik - case["logpx"]) <= 1e-4 * np.abs(case["logpx"]))
    assert np.all(ess >= K * (1 - 1e-3))


# ---- 2. the setting, the flags, the models -----------------------------------------------------------------
def test_setting_accepts_and_completes():
    from ctvae_amd import loglik
    assert loglik.loglik_setting(None) is None
    assert loglik.loglik_setting({"samples": 16, "sigma": 0.5}) == {"samples": 16, "sigma": 0.5, "chunk": 16}
    assert loglik.loglik_setting({"samples": 4096, "sigma": 1}) == {"samples": 4096, "sigma": 1.0, "chunk": 64}
    assert loglik.loglik_setting({"samples": 100, "sigma": 2.0, "chunk": 100})["chunk"] == 100


@pytest.mark.parametrize("value, message", [
    (True, "val_loglik must be a mapping with samples and sigma, got True"),
    ([16], "val_loglik must be a mapping with samples and sigma, got [16]"),
    ({"samples": 16, "sigma": 0.5, "rows": 3}, "val_loglik has unknown field(s) rows; known: samples, sigma, chunk"),
    ({"sigma": 0.5}, "val_loglik.samples is required"),
    ({"samples": 16}, "val_loglik.sigma is required"),
    ({"samples": True, "sigma": 0.5}, "val_loglik.samples must be an integer in 1..4096, got True"),
    ({"samples": 16.0, "sigma": 0.5}, "val_loglik.samples must be an integer in 1..4096, got 16.0"),
    ({"samples": 0, "sigma": 0.5}, "val_loglik.samples must be an integer in 1..4096, got 0"),
    ({"samples": 4097, "sigma": 0.5}, "val_loglik.samples must be an integer in 1..4096, got 4097"),
    ({"samples": 16, "sigma": 0.5, "chunk": 17}, "val_loglik.chunk must be an integer in 1..samples (samples=16), got 17"),
    ({"samples": 16, "sigma": 0.5, "chunk": 0}, "val_loglik.chunk must be an integer in 1..samples (samples=16), got 0"),
    ({"samples": 16, "sigma": 0.5, "chunk": 4.0}, "val_loglik.chunk must be an integer in 1..samples (samples=16), got 4.0"),
    ({"samples": 16, "sigma": 0.5, "chunk": False}, "val_loglik.chunk must be an integer in 1..samples (samples=16), got False"),
    ({"samples": 16, "sigma": 0}, "val_loglik.sigma must be a float > 0, got 0"),
    ({"samples": 16, "sigma": -1.0}, "val_loglik.sigma must be a float > 0, got -1.0"),
    ({"samples": 16, "sigma": True}, "val_loglik.sigma must be a float > 0, got True"),
    ({"samples": 16, "sigma": float("nan")}, "val_loglik.sigma must be a float > 0, got nan"),
    ({"samples": 16, "sigma": "0.5"}, "val_loglik.sigma must be a float > 0, got '0.5'"),
    ({"samples": 16, "sigma": "mse"}, "val_loglik.sigma: mse needs a second pass over the rows and is python -m "
                                      "ctvae_amd.log_likelihood's alone; give a float > 0"),
])
def test_setting_refuses_by_name(value, message):
    from ctvae_amd import loglik
    with pytest.raises(ValueError) as e:
        loglik.loglik_setting(value)
    assert str(e.value) == message


def test_model_lists():
    from ctvae_amd import loglik
    from ctvae_amd.models import vae_models
    assert ", ".join(loglik.LOGLIK_MODELS) == MODELS
    served = {name for name, cls in vae_models.items() if loglik.loglik_supported(cls)}
    assert {cls.__name__ for name, cls in vae_models.items() if name in served} == set(loglik.LOGLIK_MODELS)
    for name in ("VampVAE", "ConditionalVAE", "JointVAE", "VQVAE", "MCQVAE", "CTMCQVAE", "WAE_MMD", "SWAE", "HVAE", "LVAE", "GammaVAE",
                 "CategoricalVAE"):
        assert name in vae_models and name not in served, name
        assert loglik.needs_supported_model(vae_models[name]) == NEEDS + vae_models[name].__name__
    assert all(vae_models[n] is vae_models["VanillaVAE"] for n in served if vae_models[n].__name__ == "VanillaVAE")


@pytest.mark.parametrize("flags, message", [
    (["--samples", "0"], "--samples must be an integer in 1..65536, got 0"),
    (["--samples", "65537"], "--samples must be an integer in 1..65536, got 65537"),
    (["--samples", "8.0"], "--samples must be an integer in 1..65536, got '8.0'"),
    (["--samples", "True"], "--samples must be an integer in 1..65536, got 'True'"),
    (["--samples", "8", "--chunk", "9"], "--chunk must be an integer in 1..8, got 9"),
    (["--samples", "8", "--chunk", "0"], "--chunk must be an integer in 1..8, got 0"),
    (["--chunk", "2.5"], "--chunk must be an integer in 1..512, got '2.5'"),
    (["--rows", "0"], "--rows must be an integer of at least 1, got 0"),
    (["--rows", "1e3"], "--rows must be an integer of at least 1, got '1e3'"),
    (["--sigma", "0"], "--sigma must be a float > 0 or mse, got 0.0"),
    (["--sigma", "-0.5"], "--sigma must be a float > 0 or mse, got -0.5"),
    (["--sigma", "inf"], "--sigma must be a float > 0 or mse, got inf"),
    (["--sigma", "MSE"], "--sigma must be a float > 0 or mse, got 'MSE'"),
    (["--sigma", "True"], "--sigma must be a float > 0 or mse, got 'True'"),
])
def test_command_refuses_its_flags_by_name(tmp_path, flags, message):
    """Before a device is touched and before the checkpoint is looked at: the checkpoint named here does not exist."""
    argv = ["-c", T._config(tmp_path, "vae.yaml"), "--checkpoint", str(tmp_path / "missing.ckpt")] + flags
    assert T._refusal("log_likelihood", argv) == "log_likelihood: " + message
    assert not os.path.exists(tmp_path / "logs")


def test_check_flags_on_python_values():
    from ctvae_amd import log_likelihood as LL
    assert LL.check_flags(512, None, "mse", None) == (512, 64, "mse", None)
    assert LL.check_flags("8", None, "0.25", "3") == (8, 8, 0.25, 3)
    assert LL.check_flags(65536, 1, 2, 1) == (65536, 1, 2.0, 1)
    for args, flag in (((True, None, 1.0, None), "--samples"), ((8.0, None, 1.0, None), "--samples"), ((8, True, 1.0, None), "--chunk"),
                       ((8, 2.0, 1.0, None), "--chunk"), ((8, None, True, None), "--sigma"), ((8, None, 1.0, 2.5), "--rows"),
                       ((8, None, 1.0, False), "--rows")):
        with pytest.raises(SystemExit, match="log_likelihood: " + flag + " must be"):
            LL.check_flags(*args)


def _exp_config(tmp_path, name, exp=None):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["exp_params"].update(exp or {})
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_refuses_by_name(tmp_path):
    from ctvae_amd import run
    ok = {"samples": 4, "sigma": 0.5}
    for bad in (True, {"samples": 4}, {"samples": 4.0, "sigma": 0.5}, {"samples": 5000, "sigma": 0.5}, dict(ok, extra=1),
                dict(ok, sigma="mse"), dict(ok, chunk=5)):
        with pytest.raises(SystemExit, match=r"^exp_params\.val_loglik"):
            run.main(["-c", _exp_config(tmp_path, "vae.yaml", exp={"val_loglik": bad})])
    for cfg, name in (("mcq_vae.yaml", "MCQVAE"), ("vampvae.yaml", "VampVAE"), ("cvae.yaml", "ConditionalVAE"), ("swae.yaml", "SWAE")):
        with pytest.raises(SystemExit) as e:
            run.main(["-c", _exp_config(tmp_path, cfg, exp={"val_loglik": ok})])
        assert str(e.value) == f"exp_params.val_loglik: {NEEDS}'{name}' (model_params.name)"
    assert not (tmp_path / "logs").exists()
    for cfg in ("vae.yaml", "betatc_vae.yaml", "mssim_vae.yaml"):
        on = run.exp_val_loglik(yaml.safe_load(open(_exp_config(tmp_path, cfg, exp={"val_loglik": ok}))))
        assert on == {"samples": 4, "sigma": 0.5, "chunk": 4}
        assert run.exp_val_loglik(yaml.safe_load(open(_exp_config(tmp_path, cfg)))) is None
    for name in ("IWAE", "MIWAE"):                               # (no config of their own: vae.yaml under their name)
        config = yaml.safe_load(open(_exp_config(tmp_path, "vae.yaml", exp={"val_loglik": ok})))
        config["model_params"]["name"] = name
        assert run.exp_val_loglik(config) == {"samples": 4, "sigma": 0.5, "chunk": 4}


def test_experiment_refuses_by_name():
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    exp = {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 0.00025}
    model = vae_models["VampVAE"](in_channels=3, latent_dim=16)
    with pytest.raises(ValueError) as e:
        VAEXperiment(model, dict(exp, val_loglik={"samples": 4, "sigma": 0.5}))
    assert str(e.value) == "val_loglik: " + NEEDS + "VampVAE"
    with pytest.raises(ValueError, match=r"val_loglik\.samples must be an integer in 1\.\.4096"):
        VAEXperiment(model, dict(exp, val_loglik={"samples": 0, "sigma": 0.5}))


def test_summarize_leaves_out_what_has_no_image():
    from ctvae_amd import loglik
    st, fl = C.merge_cut(_far_weights(6), [24])
    fl[2] = 1
    res = loglik.finish(st, fl)
    want = C.finish(st)
    keep = [0, 1, 3]
    assert np.array_equal(res["loglik"][keep], want[0][keep]) and np.isnan(res["loglik"][2]) and res["nonfinite"].tolist() == [0, 0, 1, 0]
    s = loglik.summarize(res, 48)
    assert s["rows"] == 4 and s["nonfinite"] == 1
    assert s["loglik"] == math.fsum(want[0][keep].tolist()) / 3 and s["loglik_per_dim"] == s["loglik"] / 48
    assert s["gap"] == s["loglik"] - s["elbo"] and s["gap"] >= 0 and s["ess_min"] == want[2][keep].min()
    assert set(loglik.record(s)) == {"val_loglik", "val_loglik_elbo", "val_loglik_gap", "val_loglik_ess", "val_loglik_rows",
                                     "val_loglik_nonfinite"}
    none = loglik.summarize(loglik.finish(st, np.ones(4, np.int32)), 48)
    assert none == {"rows": 4, "nonfinite": 4} and loglik.record(none) == {"val_loglik_rows": 4, "val_loglik_nonfinite": 4}
    empty = loglik.summarize(loglik.finish(np.zeros((0, 5)), np.zeros(0, np.int32)), 48)
    assert empty == {"rows": 0, "nonfinite": 0}
    unseen = loglik.finish(*C.new_state(2))                       # a row no sample reached has nothing to stand on either
    assert unseen["nonfinite"].tolist() == [1, 1]


# ---- 3. the refusals every checkpoint command shares -------------------------------------------------------
def test_command_refuses_alike_and_writes_nothing(tmp_path, monkeypatch):
    monkeypatch.setitem(T.COMMANDS, "log_likelihood", COMMAND)
    T.test_every_command_refuses_alike_and_writes_nothing("log_likelihood", tmp_path)


def test_the_last_host_refusal_leaves_the_generator_alone(tmp_path, monkeypatch):
    monkeypatch.setitem(T.COMMANDS, "log_likelihood", COMMAND)
    T.test_the_last_host_refusal_leaves_the_generator_alone("log_likelihood", tmp_path, monkeypatch)
