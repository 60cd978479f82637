"""Host side of the KL weight schedules and free bits (``exp_params.kld_schedule`` / ``kld_free_bits``; ctvae_amd/klcontrol.py):
``weight(step)`` at the boundaries of both schedule types, every refusal by name -- of the library (ValueError), of the runner
(SystemExit) and of a resume under other settings -- the models that are served, and the ``trainer['kl']`` entry.  No GPU: nothing
here launches a kernel."""
import ctypes
import os

import pytest
import torch
import yaml

from tests import kl_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"LR": 1e-3, "weight_decay": 0.0, "kld_weight": 0.00025, "manual_seed": 11}
KW = 0.00025


def _f32(x):
    return ctypes.c_float(x).value


# ---- weight(step) ------------------------------------------------------------------------------------------
def test_linear_weight_at_the_boundaries():
    from ctvae_amd.klcontrol import kld_schedule_setting, weight
    N = 8
    s0 = kld_schedule_setting({"type": "linear", "warmup_steps": N})
    assert s0 == {"type": "linear", "warmup_steps": 8, "start": 0.0}
    assert weight(s0, KW, 0) == 0.0
    assert weight(s0, KW, N - 1) == _f32(KW * (7 / 8))
    assert weight(s0, KW, N) == weight(s0, KW, N + 1) == weight(s0, KW, 10 ** 9) == _f32(KW)
    assert weight(s0, KW, 3) == _f32(KW * (3 / 8))
    sa = kld_schedule_setting({"type": "linear", "warmup_steps": N, "start": 0.25})
    assert weight(sa, KW, 0) == _f32(KW * 0.25)
    assert weight(sa, KW, N - 1) == _f32(KW * (0.25 + 0.75 * (7 / 8)))
    assert weight(sa, KW, N) == weight(sa, KW, N + 1) == _f32(KW)
    one = kld_schedule_setting({"type": "linear", "warmup_steps": 1, "start": 1})
    assert [weight(one, KW, s) for s in (0, 1, 2)] == [_f32(KW)] * 3
    assert weight(None, KW, 0) == weight(None, KW, 77) == _f32(KW)
    ws = [weight(s0, KW, s) for s in range(N + 1)]
    assert all(a < b for a, b in zip(ws, ws[1:])), "the warm-up rises with every step"
    assert all(w == _f32(w) for w in ws), "rounded to fp32 once"


def test_cyclical_weight_at_the_boundaries():
    from ctvae_amd.klcontrol import kld_schedule_setting, weight
    M, r, n = 10, 0.5, 2
    sc = kld_schedule_setting({"type": "cyclical", "cycle_steps": M, "cycles": n})
    assert sc == {"type": "cyclical", "cycle_steps": 10, "ratio": 0.5, "cycles": 2}
    assert weight(sc, KW, 0) == 0.0
    assert weight(sc, KW, 1) == _f32(KW * ((1 / 10) / 0.5))
    assert weight(sc, KW, int(r * M)) == _f32(KW), "tau = r: the plateau begins"
    assert weight(sc, KW, int(r * M) - 1) == _f32(KW * ((4 / 10) / 0.5)) < _f32(KW)
    assert weight(sc, KW, M - 1) == _f32(KW)
    assert weight(sc, KW, M) == 0.0, "the second cycle starts over"
    assert weight(sc, KW, M + 2) == weight(sc, KW, 2)
    assert weight(sc, KW, n * M - 1) == _f32(KW)
    assert weight(sc, KW, n * M) == weight(sc, KW, n * M + 1) == weight(sc, KW, n * M + 3 * M) == _f32(KW), "constant behind n cycles"
    forever = kld_schedule_setting({"type": "cyclical", "cycle_steps": M, "ratio": 0.5})
    assert "cycles" not in forever
    assert weight(forever, KW, 1000 * M) == 0.0 and weight(forever, KW, 1000 * M + 3) == weight(sc, KW, 3)
    whole = kld_schedule_setting({"type": "cyclical", "cycle_steps": 4, "ratio": 1})
    assert [weight(whole, KW, s) for s in range(5)] == [0.0, _f32(KW * 0.25), _f32(KW * 0.5), _f32(KW * 0.75), 0.0]


# ---- refusals ----------------------------------------------------------------------------------------------
BAD_SCHEDULES = [
    ("linear", "kld_schedule must be a mapping"),
    ([1, 2], "kld_schedule must be a mapping"),
    (True, "kld_schedule must be a mapping"),
    ({}, r"kld_schedule\.type"),
    ({"type": "cosine", "warmup_steps": 3}, r"kld_schedule\.type.*'cosine'"),
    ({"type": True}, r"kld_schedule\.type"),
    ({"type": "linear"}, "kld_schedule.*needs warmup_steps"),
    ({"type": "linear", "warmup_steps": 0}, r"kld_schedule\.warmup_steps"),
    ({"type": "linear", "warmup_steps": 4.0}, r"kld_schedule\.warmup_steps"),
    ({"type": "linear", "warmup_steps": True}, r"kld_schedule\.warmup_steps"),
    ({"type": "linear", "warmup_steps": "4"}, r"kld_schedule\.warmup_steps"),
    ({"type": "linear", "warmup_steps": 4, "start": -0.1}, r"kld_schedule\.start"),
    ({"type": "linear", "warmup_steps": 4, "start": 1.5}, r"kld_schedule\.start"),
    ({"type": "linear", "warmup_steps": 4, "start": True}, r"kld_schedule\.start"),
    ({"type": "linear", "warmup_steps": 4, "start": float("nan")}, r"kld_schedule\.start"),
    ({"type": "linear", "warmup_steps": 4, "ratio": 0.5}, "kld_schedule.*no field 'ratio'"),
    ({"type": "linear", "warmup_steps": 4, "cycle_steps": 5}, "kld_schedule.*no field 'cycle_steps'"),
    ({"type": "cyclical"}, "kld_schedule.*needs cycle_steps"),
    ({"type": "cyclical", "cycle_steps": 1}, r"kld_schedule\.cycle_steps"),
    ({"type": "cyclical", "cycle_steps": 10.0}, r"kld_schedule\.cycle_steps"),
    ({"type": "cyclical", "cycle_steps": False}, r"kld_schedule\.cycle_steps"),
    ({"type": "cyclical", "cycle_steps": 10, "ratio": 0}, r"kld_schedule\.ratio"),
    ({"type": "cyclical", "cycle_steps": 10, "ratio": 1.01}, r"kld_schedule\.ratio"),
    ({"type": "cyclical", "cycle_steps": 10, "ratio": True}, r"kld_schedule\.ratio"),
    ({"type": "cyclical", "cycle_steps": 10, "cycles": 0}, r"kld_schedule\.cycles"),
    ({"type": "cyclical", "cycle_steps": 10, "cycles": 2.0}, r"kld_schedule\.cycles"),
    ({"type": "cyclical", "cycle_steps": 10, "cycles": True}, r"kld_schedule\.cycles"),
    ({"type": "cyclical", "cycle_steps": 10, "cycles": None}, r"kld_schedule\.cycles"),
    ({"type": "cyclical", "cycle_steps": 10, "warmup_steps": 3}, "kld_schedule.*no field 'warmup_steps'"),
    ({"type": "cyclical", "cycle_steps": 10, "start": 0.5}, "kld_schedule.*no field 'start'"),
]
BAD_FREE_BITS = [True, False, "0.1", -0.01, float("nan"), float("inf"), [0.1]]


@pytest.mark.parametrize("bad,match", BAD_SCHEDULES, ids=[str(i) for i in range(len(BAD_SCHEDULES))])
def test_schedule_refusals_by_name(bad, match):
    from ctvae_amd.klcontrol import kld_schedule_setting
    with pytest.raises(ValueError, match=match):
        kld_schedule_setting(bad)


def test_free_bits_setting():
    from ctvae_amd.klcontrol import kl_settings, kld_free_bits_setting
    for bad in BAD_FREE_BITS:
        with pytest.raises(ValueError, match="kld_free_bits"):
            kld_free_bits_setting(bad)
    assert kld_free_bits_setting(None) is None
    assert kld_free_bits_setting(0.0) == 0.0 and kld_free_bits_setting(0) == 0.0 and kld_free_bits_setting(0.25) == 0.25
    assert kl_settings({}) == (None, None)
    assert kl_settings({"kld_free_bits": 0.5}) == (None, 0.5)
    assert kl_settings({"kld_schedule": {"type": "linear", "warmup_steps": 2}}) == ({"type": "linear", "warmup_steps": 2, "start": 0.0}, None)


# ---- the models --------------------------------------------------------------------------------------------
def test_served_models():
    from ctvae_amd import klcontrol
    from ctvae_amd.models import vae_models
    served = {"VanillaVAE", "VAE", "GaussianVAE", "TwoStageVAE", "ConditionalVAE", "MSSIMVAE", "LogCoshVAE"}
    for name, cls in vae_models.items():
        if name == "BetaVAE":
            assert klcontrol.serves(cls, loss_type='H') and not klcontrol.serves(cls, loss_type='B') and not klcontrol.serves(cls)
        else:
            assert klcontrol.serves(cls) == (name in served), name


def test_experiment_builds_nothing_without_the_keys_and_refuses_by_name():
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    vanilla = vae_models["VanillaVAE"](in_channels=3, latent_dim=16)
    exp = VAEXperiment(vanilla, dict(PARAMS))
    assert exp.kl is None and "kl" not in exp.state_dict() and exp.loss_options() == {"M_N": KW}
    exp.write_kl_weight()                                        # nothing to write
    exp = VAEXperiment(vanilla, dict(PARAMS, kld_free_bits=0.0))
    assert exp.kl.schedule is None and exp.kl.free_bits == 0.0 and exp.kl.fills == 0
    opts = exp.loss_options()
    assert opts["M_N"] is exp.kl.tensor and opts["free_bits"] == 0.0 and tuple(exp.kl.tensor.shape) == (1,)
    exp = VAEXperiment(vanilla, dict(PARAMS, kld_schedule={"type": "linear", "warmup_steps": 4}))
    assert exp.kl.free_bits is None and exp.loss_options()["free_bits"] == 0.0
    for bad, _ in BAD_SCHEDULES[:8]:
        with pytest.raises(ValueError, match="kld_schedule"):
            VAEXperiment(vanilla, dict(PARAMS, kld_schedule=bad))
    for bad in BAD_FREE_BITS:
        with pytest.raises(ValueError, match="kld_free_bits"):
            VAEXperiment(vanilla, dict(PARAMS, kld_free_bits=bad))
    type_b = vae_models["BetaVAE"](in_channels=3, latent_dim=16, loss_type='B')
    with pytest.raises(ValueError, match="kld_free_bits needs a model.*BetaVAE with loss_type 'B'"):
        VAEXperiment(type_b, dict(PARAMS, kld_free_bits=0.1))
    with pytest.raises(ValueError, match="kld_schedule needs a model.*BetaVAE with loss_type 'B'"):
        VAEXperiment(type_b, dict(PARAMS, kld_schedule={"type": "linear", "warmup_steps": 4}, kld_free_bits=0.1))
    assert VAEXperiment(type_b, dict(PARAMS)).kl is None
    type_h = vae_models["BetaVAE"](in_channels=3, latent_dim=16, loss_type='H')
    assert VAEXperiment(type_h, dict(PARAMS, kld_free_bits=0.1)).kl is not None
    for name, cfg in (("DIPVAE", dict(in_channels=3, latent_dim=16)), ("IWAE", dict(in_channels=3, latent_dim=16)),
                      ("InfoVAE", dict(in_channels=3, latent_dim=16)), ("VampVAE", dict(in_channels=3, latent_dim=16)),
                      ("MCQVAE", dict(in_channels=3, embedding_dim=16, hidden_dims=[8, 16], num_embeddings=8, img_size=64, codebooks=4))):
        torch.manual_seed(7)
        with pytest.raises(ValueError, match=f"kld_free_bits needs a model.*got {name}"):
            VAEXperiment(vae_models[name](**cfg), dict(PARAMS, kld_free_bits=0.1))


def test_the_write_fills_only_when_the_value_changes():
    from ctvae_amd.klcontrol import KLControl, kld_schedule_setting
    kl = KLControl(kld_schedule_setting({"type": "linear", "warmup_steps": 2}), 0.05, KW, "cpu")
    seen = [(kl.write(s), kl.fills, float(kl.tensor[0])) for s in (0, 0, 1, 2, 3, 4)]
    assert [f for _, f, _ in seen] == [1, 1, 2, 3, 3, 3]
    assert all(w == t for w, _, t in seen) and seen[-1][0] == _f32(KW)
    const = KLControl(None, 0.0, KW, "cpu")
    assert [const.write(s) for s in range(5)] == [_f32(KW)] * 5 and const.fills == 1 and const.floor == 0.0
    assert KLControl(kld_schedule_setting({"type": "linear", "warmup_steps": 2}), None, KW, "cpu").floor == 0.0


# ---- checkpoints -------------------------------------------------------------------------------------------
def test_trainer_entry_round_trip_and_refusals(tmp_path):
    from ctvae_amd import run
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    sched = {"type": "linear", "warmup_steps": 8}
    keys = {"kld_schedule": sched, "kld_free_bits": 0.05}
    vanilla = vae_models["VanillaVAE"](in_channels=3, latent_dim=16)
    exp = VAEXperiment(vanilla, dict(PARAMS, **keys))
    exp.global_step = 3
    sd = exp.state_dict()
    assert sd["kl"] == {"schedule": {"type": "linear", "warmup_steps": 8, "start": 0.0}, "free_bits": 0.05}
    path = tmp_path / "t.ckpt"
    torch.save({"trainer": sd}, path)
    back = torch.load(path, weights_only=True)["trainer"]
    assert back["kl"] == sd["kl"]
    again = VAEXperiment(vae_models["VanillaVAE"](in_channels=3, latent_dim=16), dict(PARAMS, **keys))
    again.load_state_dict(back)
    assert again.global_step == 3 and again.kl.weight(again.global_step) == _f32(KW * 3 / 8)
    plain = VAEXperiment(vae_models["VanillaVAE"](in_channels=3, latent_dim=16), dict(PARAMS))
    plain.load_state_dict(back)                                  # a run without the keys ignores the entry
    assert plain.kl is None and plain.global_step == 3
    for other, match in (({"kld_schedule": {"type": "linear", "warmup_steps": 9}, "kld_free_bits": 0.05}, "kld_schedule"),
                         ({"kld_schedule": sched, "kld_free_bits": 0.5}, "kld_free_bits"),
                         ({"kld_schedule": sched}, "kld_free_bits"),
                         ({"kld_free_bits": 0.05}, "kld_schedule"),
                         ({"kld_schedule": {"type": "cyclical", "cycle_steps": 8}, "kld_free_bits": 0.05}, "kld_schedule")):
        e = VAEXperiment(vae_models["VanillaVAE"](in_channels=3, latent_dim=16), dict(PARAMS, **other))
        with pytest.raises(RuntimeError, match=match):
            e.load_state_dict(back)
        assert e.global_step == 0                                # refused before anything was read
        s, f = run.exp_kl({"exp_params": other, "model_params": {"name": "VanillaVAE"}})
        with pytest.raises(SystemExit, match=rf"exp_params\.kld_schedule / kld_free_bits.*{match}.*t\.ckpt"):
            run.check_kl_checkpoint({"trainer": back}, str(path), s, f)
    no_entry = {k: v for k, v in back.items() if k != "kl"}
    with pytest.raises(RuntimeError, match=r"trainer\['kl'\]"):
        again.load_state_dict(no_entry)
    with pytest.raises(SystemExit, match=r"exp_params\.kld_schedule.*trainer\['kl'\].*t\.ckpt"):
        run.check_kl_checkpoint({"trainer": no_entry}, str(path), *run.exp_kl({"exp_params": keys, "model_params": {"name": "VAE"}}))
    run.check_kl_checkpoint({"trainer": back}, str(path), *run.exp_kl({"exp_params": keys, "model_params": {"name": "VAE"}}))


# ---- the runner --------------------------------------------------------------------------------------------
def _config(tmp_path, name, exp=None, model=None):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["exp_params"].update(exp or {})
    cfg["model_params"].update(model or {})
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_refuses_by_name(tmp_path):
    from ctvae_amd import run
    for bad, _ in BAD_SCHEDULES[:10]:
        with pytest.raises(SystemExit, match=r"exp_params\.kld_schedule"):
            run.main(["-c", _config(tmp_path, "vae.yaml", exp={"kld_schedule": bad})])
    for bad in ("0.1", -1.0, True):
        with pytest.raises(SystemExit, match=r"exp_params\.kld_free_bits"):
            run.main(["-c", _config(tmp_path, "vae.yaml", exp={"kld_free_bits": bad})])
    for cfg, name in (("mcq_vae.yaml", "MCQVAE"), ("lvae.yaml", "LVAE"), ("vampvae.yaml", "VampVAE"), ("betatc_vae.yaml", "BetaTCVAE"),
                      ("swae.yaml", "SWAE")):
        with pytest.raises(SystemExit, match=rf"exp_params\.kld_free_bits needs a model.*{name}"):
            run.main(["-c", _config(tmp_path, cfg, exp={"kld_free_bits": 0.1})])
    beta = {"name": "BetaVAE", "beta": 4}
    with pytest.raises(SystemExit, match=r"exp_params\.kld_schedule needs a model.*'BetaVAE' with loss_type 'B'"):
        run.main(["-c", _config(tmp_path, "vae.yaml", exp={"kld_schedule": {"type": "linear", "warmup_steps": 5}}, model=beta)])
    with pytest.raises(SystemExit, match=r"exp_params\.kld_free_bits needs a model.*'BetaVAE' with loss_type 'B'"):
        run.main(["-c", _config(tmp_path, "vae.yaml", exp={"kld_free_bits": 0.1}, model=dict(beta, loss_type='B'))])
    assert not (tmp_path / "logs").exists()                      # refused before a device or a directory was touched
    ok = yaml.safe_load(open(_config(tmp_path, "vae.yaml", exp={"kld_free_bits": 0.1}, model=dict(beta, loss_type='H'))))
    assert run.exp_kl(ok) == (None, 0.1)
    for cfg in ("vae.yaml", "cvae.yaml", "mssim_vae.yaml"):
        keys = {"kld_schedule": {"type": "cyclical", "cycle_steps": 10}, "kld_free_bits": 0.0}
        assert run.exp_kl(yaml.safe_load(open(_config(tmp_path, cfg, exp=keys)))) == ({"type": "cyclical", "cycle_steps": 10, "ratio": 0.5}, 0.0)
        assert run.exp_kl(yaml.safe_load(open(_config(tmp_path, cfg)))) == (None, None)


# ---- the test inputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(1, 4), (3, 10), (64, 128), (257, 200)])
def test_input_builder_separates_the_columns(B, L):
    mu, lv = C.make_inputs(B, L)
    assert mu.dtype == lv.dtype == torch.float32 and tuple(mu.shape) == tuple(lv.shape) == (B, L)
    again = C.make_inputs(B, L)
    assert torch.equal(mu, again[0]) and torch.equal(lv, again[1])
    m = C.reference(mu, lv, 1.0, 1.0, 0.0)["m"]
    print(f"({B}, {L}): collapsed max {float(m[0::2].max()):.3e}, active min {float(m[1::2].min()):.3f}")
    assert float(m[0::2].max()) <= 0.002 and float(m[1::2].min()) >= 0.79
    for lam in (0.05, 0.5):
        ref = C.reference(mu, lv, 0.37, 1.0, lam)
        assert ref["out"][3] == (L + 1) // 2 and bool(ref["active"][1::2].all()) and not bool(ref["active"][0::2].any())
        assert bool((ref["g_mu"][:, 0::2] == 0).all()) and bool((ref["g_lv"][:, 0::2] == 0).all())
        assert ref["out"][2] == pytest.approx(float(ref["m"][1::2].sum()) + lam * ((L + 1) // 2), rel=1e-12)
    assert C.reference(mu, lv, 0.37, 1.0, 0.0)["out"][3] == 0


def test_reference_keeps_a_nan_column_active():
    mu, lv = C.make_inputs(3, 4)
    mu[1, 0] = float("nan")
    ref = C.reference(mu, lv, 1.0, 1.0, 0.0)
    assert bool(ref["active"][0]) and ref["out"][3] == 0 and ref["out"][1] != ref["out"][1]
