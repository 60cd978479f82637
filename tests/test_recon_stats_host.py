"""Host side of the reconstruction statistics (``exp_params.recon_stats``; ctvae_amd/reconstats.py, recon_stats.py): the float64
restatement (tests/recon_checks.py) against closed forms, the settings validator, ``summarize`` on hand-made records, the model
hook on stub results, and the refusals of the experiment, the runner and the tool.  No GPU: nothing here launches a kernel."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import recon_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"LR": 1e-3, "weight_decay": 0.0, "kld_weight": 1.0, "manual_seed": 11}


# ---- the restatement against closed forms ----------------------------------------------------------------------
def test_reference_ssim_of_a_picture_with_itself_is_one():
    a, _ = C.pictures(1, 2, 3, 17)
    rec, flags = C.ref_records(a, a)
    assert flags.tolist() == [0, 0] and rec[:, 3].tolist() == [1.0, 1.0] and rec[:, :3].tolist() == [[0.0] * 3] * 2
    r, _ = C.pictures(2, 1, 1, 12, kind="randn")
    assert C.ref_records(r, r, R=2.0)[0][0, 3] == 1.0


def test_reference_ssim_of_two_constant_pictures():
    """No variance, no covariance: the structure factor is C2 / C2 and the luminance factor stays."""
    for va, vb, R in ((0.25, 0.75, 1.0), (0.0, 1.0, 1.0), (40.0, 200.0, 255.0)):
        a, b = np.full((1, 2, 13, 13), va, np.float32), np.full((1, 2, 13, 13), vb, np.float32)
        rec, _ = C.ref_records(a, b, R)
        c1 = (0.01 * R) ** 2
        x, y = float(np.float32(va)), float(np.float32(vb))
        assert abs(rec[0, 3] - (2 * x * y + c1) / (x * x + y * y + c1)) <= 1e-12
        assert abs(rec[0, 0] - (x - y) ** 2) <= 1e-12 * (x - y) ** 2 and rec[0, 2] == abs(x - y)


def test_reference_is_invariant_under_a_common_scale():
    a, b = C.pictures(3, 2, 3, 16)
    a255, b255 = (a.astype(np.float64) * 255.0), (b.astype(np.float64) * 255.0)        # float64: the scaling itself rounds nothing away
    rec, _ = C.ref_records(a.astype(np.float64), b.astype(np.float64), 1.0)
    rec255, _ = C.ref_records(a255, b255, 255.0)
    assert np.abs(rec[:, 3] - rec255[:, 3]).max() <= 1e-12
    psnr, psnr255 = 10 * np.log10(1.0 / rec[:, 0]), 10 * np.log10(255.0 ** 2 / rec255[:, 0])
    assert np.abs(psnr - psnr255).max() <= 1e-12 * np.abs(psnr).max()
    s, s255 = C.ref_summary(rec, [0, 0], 1.0), C.ref_summary(rec255, [0, 0], 255.0)
    assert abs(s["psnr"] - s255["psnr"]) <= 1e-12 * abs(s["psnr"]) and abs(s["ssim"] - s255["ssim"]) <= 1e-12


def test_reference_window_and_worst_order():
    G = C.window2d()
    assert G.shape == (11, 11) and abs(G.sum() - 1.0) <= 1e-15 and G[5, 5] == G.max() and np.array_equal(G, G.T)
    a, b = C.pictures(4, 4, 1, 11)
    a[3], b[3] = a[1], b[1]                           # a tie: the lower row goes first
    a[2, 0, 0, 0] = np.nan                            # never enters
    rows, ssim, wa, wb = C.ref_worst([(a[:1], b[:1]), (a[1:], b[1:])], 4)
    rec, flags = C.ref_records(a, b)
    assert flags.tolist() == [0, 0, 1, 0] and rows[3] == -1 and sorted(rows[:3].tolist()) == [0, 1, 3]
    assert list(rows[:3]).index(1) < list(rows[:3]).index(3) and np.all(np.diff(ssim[:3]) >= 0)
    assert np.array_equal(wa[0], a[rows[0]]) and np.array_equal(wb[0], b[rows[0]]) and not wa[3].any()
    one = C.ref_worst([(a, b)], 4)
    assert all(np.array_equal(x, y) for x, y in zip(one, (rows, ssim, wa, wb)))


# ---- the settings ------------------------------------------------------------------------------------------------
def test_settings_defaults_and_refusals():
    from ctvae_amd.reconstats import recon_settings
    assert recon_settings({}) == (False, None, None) and recon_settings({"recon_stats": False}) == (False, None, None)
    assert recon_settings({"recon_stats": True}) == (True, 1.0, 8)
    assert recon_settings({"recon_stats": True, "recon_stats_range": 255.0, "recon_stats_worst": 0}) == (True, 255.0, 0)
    assert recon_settings({"recon_stats": True, "recon_stats_worst": 32}) == (True, 1.0, 32)
    for bad in (1, 0, "true", 1.0, [True]):
        with pytest.raises(ValueError, match="recon_stats must be"):
            recon_settings({"recon_stats": bad})
    for bad in (True, 1, 255, 0.0, -1.0, float("inf"), float("nan"), "1.0"):
        with pytest.raises(ValueError, match="recon_stats_range"):
            recon_settings({"recon_stats": True, "recon_stats_range": bad})
    for bad in (True, 8.0, -1, 33, "8"):
        with pytest.raises(ValueError, match="recon_stats_worst"):
            recon_settings({"recon_stats": True, "recon_stats_worst": bad})
    for on in ({}, {"recon_stats": False}):
        with pytest.raises(ValueError, match="recon_stats_range.*without recon_stats"):
            recon_settings({**on, "recon_stats_range": 1.0})
        with pytest.raises(ValueError, match="recon_stats_worst.*without recon_stats"):
            recon_settings({**on, "recon_stats_worst": 4})


# ---- summarize ---------------------------------------------------------------------------------------------------
def test_summarize_on_hand_made_records():
    from ctvae_amd import reconstats as S
    #            mse    mae   max   ssim
    rec = [[0.01, 0.08, 0.30, 0.90],
           [0.04, 0.15, 0.50, 0.60],
           [0.00, 0.00, 0.00, 1.00],       # exact: out of the PSNR statistics only
           [9.99, 9.99, 9.99, -5.0],       # flagged: out of everything
           [0.0025, 0.04, 0.20, 0.95]]
    flags = [0, 0, 0, 1, 0]
    res = S.summarize(rec, flags, R=1.0)
    assert res["rows"] == 5 and res["nonfinite"] == 1 and res["exact"] == 1
    psnr = np.array([20.0, 10 * np.log10(1 / 0.04), 10 * np.log10(1 / 0.0025)])
    ssim = np.array([0.90, 0.60, 1.00, 0.95])
    assert abs(res["psnr"] - psnr.mean()) <= 1e-12 and abs(res["psnr_min"] - psnr.min()) <= 1e-12
    assert abs(res["psnr_p05"] - np.percentile(psnr, 5)) <= 1e-12
    assert res["ssim"] == ssim.mean() and res["ssim_min"] == 0.60 and res["ssim_p05"] == np.percentile(ssim, 5)
    assert abs(res["ssim_p05"] - (0.60 + 0.15 * (0.90 - 0.60))) <= 1e-12        # linear interpolation at rank 0.05 * 3
    assert abs(res["mae"] - (0.08 + 0.15 + 0.0 + 0.04) / 4) <= 1e-15 and res["max_err"] == 0.50
    assert res == C.ref_summary(rec, flags, 1.0)
    assert S.summarize(rec, flags, R=2.0)["psnr"] == pytest.approx(res["psnr"] + 10 * np.log10(4.0), abs=1e-12)
    log = S.record(res)
    assert set(log) == {"val_recon_" + k for k in S.RECORD_KEYS} and log["val_recon_rows"] == 5
    assert set(S.record(res, suffix="_base")) == {"val_recon_" + k + "_base" for k in S.RECORD_KEYS}


def test_summarize_leaves_out_what_has_no_image():
    from ctvae_amd import reconstats as S
    assert S.summarize(np.zeros((0, 4)), []) == {"rows": 0, "nonfinite": 0, "exact": 0}
    only_bad = S.summarize([[np.nan] * 4, [np.inf] * 4], [1, 1])
    assert only_bad == {"rows": 2, "nonfinite": 2, "exact": 0}
    only_exact = S.summarize([[0.0, 0.0, 0.0, 1.0]] * 3, [0, 0, 0])
    assert only_exact["exact"] == 3 and only_exact["ssim"] == 1.0 and not any(k.startswith("psnr") for k in only_exact)
    assert set(S.record(only_exact)) == {"val_recon_" + k for k in ("ssim", "mae", "max_err", "ssim_p05", "ssim_min", "rows",
                                                                   "nonfinite", "exact")}
    for res in (only_bad, only_exact):
        assert all(np.isfinite(v) for v in res.values())
    with pytest.raises(ValueError, match="3 records and 2 flags"):
        S.summarize(np.zeros((3, 4)), [0, 0])


# ---- the model hook ----------------------------------------------------------------------------------------------
def test_reconstruction_pair_hook():
    from ctvae_amd.models import vae_models
    from ctvae_amd.models.base import BaseVAE
    r, x = torch.zeros(2, 3, 16, 16), torch.ones(2, 3, 16, 16)
    for name in ("VanillaVAE", "MCQVAE", "BetaTCVAE", "LVAE"):
        pair = vae_models[name].reconstruction_pair(None, [r, x, torch.zeros(2, 4), torch.zeros(2, 4)])
        assert pair[0] is r and pair[1] is x, name
    assert BaseVAE.reconstruction_pair(None, [torch.zeros(2, 5, 3, 16, 16), x]) is None          # IWAE's [B, S, C, H, W]
    assert BaseVAE.reconstruction_pair(None, [torch.zeros(2, 12), torch.zeros(2, 12)]) is None
    assert BaseVAE.reconstruction_pair(None, [r, torch.ones(2, 3, 8, 8)]) is None and BaseVAE.reconstruction_pair(None, [r]) is None
    ct = vae_models["CTMCQVAE"]
    y = torch.full((2, 3, 16, 16), 2.0)
    zero = torch.zeros(())
    assert ct.reconstruction_pair.__qualname__.startswith("CTMCQVAE")
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
    torch.manual_seed(3)
    m = ct(**cfg)
    base = m.reconstruction_pair([r, x, zero, zero, {"mode": "base"}])
    action = m.reconstruction_pair([r, y, zero, zero, {"mode": "action"}])
    assert base[0] is r and base[1] is x and action[0] is r and action[1] is y
    assert m.reconstruction_pair([torch.zeros(2, 12), torch.zeros(2, 12), zero, zero, {"mode": "causal"}]) is None
    assert m.reconstruction_pair([r, x, zero, zero, {"mode": "causal"}]) is None                  # the mode decides, not the shapes


# ---- the experiment ----------------------------------------------------------------------------------------------
def test_experiment_builds_nothing_without_the_key_and_refuses_by_name():
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    from ctvae_amd.reconstats import ReconStats
    vanilla = vae_models["VanillaVAE"](in_channels=3, latent_dim=16)
    exp = VAEXperiment(vanilla, dict(PARAMS))
    assert exp.recon_stats is False and exp.val_recon is None
    assert VAEXperiment(vanilla, dict(PARAMS, recon_stats=False)).val_recon is None
    exp = VAEXperiment(vanilla, dict(PARAMS, recon_stats=True, recon_stats_worst=4, recon_stats_range=2.0))
    assert exp.recon_stats is True and list(exp.val_recon) == [""]
    acc = exp.val_recon[""]
    assert isinstance(acc, ReconStats) and acc.K == 4 and acc.R == 2.0 and acc.records is None and acc.sides is None   # no buffer yet
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.reset()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        acc.observe(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    for bad, key in (({"recon_stats": 1}, "recon_stats must"), ({"recon_stats": True, "recon_stats_range": 1}, "recon_stats_range"),
                     ({"recon_stats": True, "recon_stats_worst": 40}, "recon_stats_worst"),
                     ({"recon_stats_worst": 4}, "recon_stats_worst.*without recon_stats")):
        with pytest.raises(ValueError, match=key):
            VAEXperiment(vanilla, dict(PARAMS, **bad))
    for name in ("IWAE", "MIWAE"):
        m = vae_models[name](in_channels=3, latent_dim=16)
        with pytest.raises(ValueError, match=f"recon_stats.*{name}"):
            VAEXperiment(m, dict(PARAMS, recon_stats=True))
        assert VAEXperiment(m, dict(PARAMS)).val_recon is None
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
    torch.manual_seed(3)
    exp = VAEXperiment(vae_models["CTMCQVAE"](**cfg), dict(PARAMS, recon_stats=True))
    assert list(exp.val_recon) == ["_base", "_action"]


def test_kernel_wrappers_refuse_on_the_host():
    from ctvae_amd import kernels as K
    consts = K.recon_consts(1.0)
    g = np.array(consts[:11])
    assert len(consts) == 13 and abs(g.sum() - 1.0) <= 1e-15 and abs(consts[11] - 1e-4) <= 1e-18 and abs(consts[12] - 9e-4) <= 1e-18
    assert np.abs(np.outer(g, g) - C.window2d()).max() <= 1e-16
    with pytest.raises(ValueError, match="recon_stats_range"):
        K.recon_consts(0.0)
    rec, flags = torch.zeros(8, 4, dtype=torch.float64), torch.zeros(8, dtype=torch.int32)
    ok = torch.zeros(2, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.recon_record(ok, ok, consts, rec, flags, 0)
    for S in (10, 65):
        with pytest.raises(ValueError, match="11 <= S <= 64"):
            K.recon_record(torch.zeros(1, 3, S, S), torch.zeros(1, 3, S, S), consts, rec, flags, 0)
    with pytest.raises(ValueError, match="11 <= S <= 64"):
        K.recon_record(torch.zeros(1, 3, 16, 20), torch.zeros(1, 3, 16, 20), consts, rec, flags, 0)
    with pytest.raises(ValueError, match="one shape"):
        K.recon_record(ok, torch.zeros(2, 3, 17, 17), consts, rec, flags, 0)
    with pytest.raises(ValueError, match="target must be a torch.float32"):
        K.recon_record(ok, ok.double(), consts, rec, flags, 0)
    with pytest.raises(ValueError, match="leave the capacity 8"):
        K.recon_record(ok, ok, consts, rec, flags, 7)
    with pytest.raises(ValueError, match="records must be a torch.float64"):
        K.recon_record(ok, ok, consts, rec.float(), flags, 0)
    with pytest.raises(ValueError, match="1 <= K <= 32"):
        K.recon_worst_state(33, 16, 3, "cpu")
    side = K.recon_worst_state(2, 16, 3, "cpu")
    with pytest.raises(ValueError, match="nothing is merged in place"):
        K.recon_worst(side, side, rec, flags, 0, ok.permute(0, 2, 3, 1).contiguous(), ok.permute(0, 2, 3, 1).contiguous())


# ---- the runner and the tool -------------------------------------------------------------------------------------
def _config(tmp_path, name, exp=None, model=None):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["exp_params"].update(exp or {})
    cfg["model_params"].update(model or {})
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_refuses_by_name_before_a_device_is_touched(tmp_path, monkeypatch):
    from ctvae_amd import run

    def no_device(*a, **k):
        raise AssertionError("a device call was made before the refusal")
    monkeypatch.setattr(torch.cuda, "is_available", no_device)
    monkeypatch.setattr(torch.cuda, "set_device", no_device)
    for bad in (1, "on", 2.5):
        with pytest.raises(SystemExit, match=r"exp_params\.recon_stats must"):
            run.main(["-c", _config(tmp_path, "vae.yaml", exp={"recon_stats": bad})])
    with pytest.raises(SystemExit, match=r"exp_params\.recon_stats_range"):
        run.main(["-c", _config(tmp_path, "vae.yaml", exp={"recon_stats": True, "recon_stats_range": 255})])
    with pytest.raises(SystemExit, match=r"exp_params\.recon_stats_worst"):
        run.main(["-c", _config(tmp_path, "mcq_vae.yaml", exp={"recon_stats": True, "recon_stats_worst": 33})])
    with pytest.raises(SystemExit, match=r"exp_params\.recon_stats_worst.*without recon_stats"):
        run.main(["-c", _config(tmp_path, "mcq_vae.yaml", exp={"recon_stats_worst": 4})])
    for name in ("IWAE", "MIWAE"):
        with pytest.raises(SystemExit, match=rf"exp_params\.recon_stats.*{name}"):
            run.main(["-c", _config(tmp_path, "vae.yaml", exp={"recon_stats": True}, model={"name": name})])
    assert not (tmp_path / "logs").exists()
    for cfg in ("vae.yaml", "mcq_vae.yaml", "ct_mcq_vae.yaml"):
        assert run.exp_recon_stats(yaml.safe_load(open(_config(tmp_path, cfg, exp={"recon_stats": True})))) == (True, 1.0, 8)
        assert run.exp_recon_stats(yaml.safe_load(open(_config(tmp_path, cfg)))) == (False, None, None)


def test_command_refuses_with_a_reason(tmp_path):
    from ctvae_amd import recon_stats
    for name in ("IWAE", "MIWAE"):
        with pytest.raises(SystemExit, match=f"recon_stats: .*{name}"):
            recon_stats.main(["-c", _config(tmp_path, "vae.yaml", model={"name": name})])
    with pytest.raises(SystemExit, match="no checkpoint"):
        recon_stats.main(["-c", _config(tmp_path, "vae.yaml")])
    missing = str(tmp_path / "missing.ckpt")
    with pytest.raises(SystemExit, match="missing.ckpt does not exist"):
        recon_stats.main(["-c", _config(tmp_path, "vae.yaml"), "--checkpoint", missing])
    for flag, bad in (("--worst", "-1"), ("--worst", "33"), ("--range", "0"), ("--range", "nan")):
        with pytest.raises(SystemExit, match=flag):
            recon_stats.main(["-c", _config(tmp_path, "vae.yaml"), "--checkpoint", missing, flag, bad])
    ckpt = tmp_path / "plain.ckpt"
    torch.save({"state_dict": {}, "epoch": 0}, ckpt)
    with pytest.raises(SystemExit, match="--ema.*plain.ckpt holds no ema_state_dict"):
        recon_stats.main(["-c", _config(tmp_path, "vae.yaml"), "--checkpoint", str(ckpt), "--ema"])
    assert not os.path.exists(tmp_path / "logs")                    # nothing was written
