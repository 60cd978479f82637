"""GPU: the reconstruction statistics (``exp_params.recon_stats``) through the training harness, and the tool on a checkpoint:
reconstats.ReconStats on csrc/reconstat.hip, fed by ``validation_step`` with ``BaseVAE.reconstruction_pair``.

VanillaVAE at B = 4, MCQVAE at B = 4 and one CT-MCQ-VAE case, on ``filler.synthetic_batch`` / ``synthetic_pairs`` -- what
``run.SyntheticData`` hands out.  The reference is ``recon_checks.ref_summary`` of the very tensors the harness handed over (a spy on
``observe``).  Bounds (tests/test_recon_stats_ops_gpu.py): per image ``mse`` and ``mae`` 1e-12 relative, ``ssim`` 1e-9 absolute, ``max``
equal; a mean, a minimum or an interpolated percentile of such values keeps the bound, and PSNR = 10 log10(R^2 / mse) turns a
relative 1e-12 of the mse into 10 / ln 10 * 1e-12 = 4.4e-12 absolute: 1e-11.  Against ``val_Reconstruction_Loss`` the fp32 loss
kernel is the looser side: the project's fp32 tolerance, 1e-4 relative."""
import io
import json
import os
import struct

import numpy as np
import pytest
import torch
import yaml

from ctvae_amd import filler
from tests import recon_checks as C
from tests.test_codebook_gpu import CT_PARAMS, _ct_batch, _mcq, fixed_noise  # noqa: F401
from tests.test_ct_gpu import build_ct
from tests.test_grad_accum_gpu import B, EXP, _assert_same, _batches, _snapshot, _vanilla

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4
KEYS = ("psnr", "ssim", "mae", "max_err", "psnr_p05", "ssim_p05", "psnr_min", "ssim_min", "rows", "nonfinite", "exact")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _epochs(batches, per_epoch):
    calls = [0]

    def train():
        lo = calls[0] * per_epoch
        calls[0] += 1
        return iter(batches[lo:lo + per_epoch])
    return train


def _spy(acc, seen):
    inner = acc.observe

    def observe(recons, target):
        seen.append((recons.detach().clone(), target.detach().clone()))
        inner(recons, target)
    acc.observe = observe


def _ref_of(pairs, R=1.0):
    """(summary, records, flags) of the restatement over the pairs handed to ``observe``."""
    a = np.concatenate([p[0].float().cpu().numpy() for p in pairs])
    b = np.concatenate([p[1].float().cpu().numpy() for p in pairs])
    rec, flags = C.ref_records(a, b, R)
    return C.ref_summary(rec, flags, R), rec, flags


def _assert_summary(got, want, prefix="val_recon_", suffix=""):
    """``got``: a record; ``want``: a ``ref_summary``.  The same keys, within the module docstring's bounds."""
    mine = {k[len(prefix):len(k) - len(suffix)]: v for k, v in got.items()
            if k.startswith(prefix) and k.endswith(suffix) and k[len(prefix):len(k) - len(suffix)] in KEYS}
    print(suffix or "-", mine)
    assert sorted(mine) == sorted(want), (sorted(mine), sorted(want))
    for k in ("rows", "nonfinite", "exact", "max_err"):
        assert mine[k] == want[k], (k, mine[k], want[k])
    for k in ("psnr", "psnr_p05", "psnr_min"):
        assert abs(mine[k] - want[k]) <= 1e-11, (k, mine[k], want[k])
    for k in ("ssim", "ssim_p05", "ssim_min"):
        assert abs(mine[k] - want[k]) <= 1e-9, (k, mine[k], want[k])
    assert abs(mine["mae"] - want["mae"]) <= 1e-12 * want["mae"]


def _png_size(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR"
    return struct.unpack(">II", data[16:24])          # (width, height)


def _lines(log, key):
    return [r for r in map(json.loads, log.getvalue().splitlines()) if key in r]


# ---- 1. VanillaVAE: the record, the log, the files -----------------------------------------------------------
def test_vanilla_record_log_and_files(dev, tmp_path):
    from ctvae_amd import imagegrid
    from ctvae_amd.experiment import VAEXperiment
    train, val = _batches(dev, 6), _batches(dev, 2, seed=4900)
    log, seen = io.StringIO(), []
    exp = VAEXperiment(_vanilla(dev), dict(EXP, recon_stats=True), log_file=log, sample_dir=str(tmp_path), run_name="run")
    _spy(exp.val_recon[""], seen)
    hist = exp.fit(_epochs(train, 3), lambda: iter(val), max_epochs=2)
    assert len(seen) == 4 and all(tuple(r.shape) == tuple(t.shape) == (B, 3, 64, 64) for r, t in seen)
    assert all(torch.equal(t, v[0]) for (_, t), v in zip(seen[2:], val)), "the target is the validation batch itself"
    rec = {k: v for k, v in hist[1].items() if k.startswith("val_recon_")}
    want, ref_rec, ref_flags = _ref_of(seen[2:])
    _assert_summary(rec, want)
    assert rec["val_recon_rows"] == 2 * B and rec["val_recon_nonfinite"] == 0 and rec["val_recon_exact"] == 0
    lines = _lines(log, "val_recon_rows")
    assert len(lines) == 2 and {k: v for k, v in lines[1].items() if k != "step"} == rec and lines[1]["step"] == 6
    for e in (0, 1):
        npz = np.load(tmp_path / "Recon" / f"recon_stats_run_Epoch_{e}.npz")
        assert sorted(npz.files) == ["mae", "max_err", "mse", "nonfinite", "ssim", "worst_rows"]
        assert npz["mse"].shape == (2 * B,) and npz["mse"].dtype == np.float64 and npz["nonfinite"].tolist() == [0] * (2 * B)
        _, _, Hg, Wg = imagegrid.grid_geometry(2 * 8, 64, 64, 8, 2)             # 2 x K tiles, K = 8: every validation image
        assert _png_size(tmp_path / "Recon" / f"worst_run_Epoch_{e}.png") == (Wg, Hg)
    npz = np.load(tmp_path / "Recon" / "recon_stats_run_Epoch_1.npz")
    assert np.abs(npz["mse"] - ref_rec[:, 0]).max() <= 1e-12 * ref_rec[:, 0].max() and np.array_equal(npz["max_err"], ref_rec[:, 2])
    assert np.abs(npz["ssim"] - ref_rec[:, 3]).max() <= 1e-9
    assert npz["worst_rows"].tolist() == np.argsort(ref_rec[:, 3], kind="stable").tolist()        # K = 8: all of them, worst first
    # equal-sized validation batches: the mean of the per-image mse is the mean of the steps' batch-mean MSE
    loss = hist[1]["val_Reconstruction_Loss"]
    print("mean mse", npz["mse"].mean(), "val_Reconstruction_Loss", loss)
    assert abs(npz["mse"].mean() - loss) <= RTOL * loss


# ---- 2. training does not notice; without the key there is nothing --------------------------------------------
@pytest.mark.parametrize("hipgraph", [True, False])
def test_training_and_every_other_record_key_are_bit_for_bit_the_same(dev, tmp_path, hipgraph):
    from ctvae_amd.experiment import VAEXperiment
    train, val = _batches(dev, 8), _batches(dev, 2, seed=4900)
    finals, rngs, hists = {}, {}, {}
    for name, extra in (("plain", {}), ("stats", {"recon_stats": True, "recon_stats_worst": 2})):
        log = io.StringIO()
        exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=hipgraph, **extra), log_file=log, sample_dir=str(tmp_path / name),
                           run_name="run")
        torch.manual_seed(5)
        hists[name] = exp.fit(_epochs(train, 4), lambda: iter(val), max_epochs=2)
        assert exp.global_step == 8
        finals[name] = _snapshot(exp)
        rngs[name] = (exp.model._rng_state.clone(), torch.get_rng_state(), torch.cuda.get_rng_state(dev))
        if name == "plain":            # no buffer, no file, no key
            assert exp.val_recon is None and not (tmp_path / name).exists()
            assert not any("recon_" in k for h in hists[name] for k in h) and not _lines(log, "val_recon_rows")
        else:
            assert hists[name][1]["val_recon_rows"] == 2 * B and (tmp_path / name / "Recon").is_dir()
    _assert_same(finals["plain"], finals["stats"], "with and without recon_stats")
    for a, b in zip(rngs["plain"], rngs["stats"]):
        assert torch.equal(a, b)
    for plain, stats in zip(hists["plain"], hists["stats"]):
        assert set(stats) - set(plain) <= {"val_recon_" + k for k in KEYS} and set(plain) <= set(stats)
        for k in plain:
            if k != "epoch_seconds":
                assert plain[k] == stats[k], (k, plain[k], stats[k])


# ---- 3. MCQVAE -----------------------------------------------------------------------------------------------
def test_mcqvae_record_without_files(dev):
    from ctvae_amd.experiment import VAEXperiment
    train, val = _batches(dev, 2), _batches(dev, 2, seed=4900)
    log, seen = io.StringIO(), []
    exp = VAEXperiment(_mcq(dev), dict(EXP, recon_stats=True, recon_stats_worst=4), log_file=log)      # no sample_dir: numbers only
    _spy(exp.val_recon[""], seen)
    hist = exp.fit(lambda: iter(train), lambda: iter(val), max_epochs=1)
    want, ref_rec, _ = _ref_of(seen)
    _assert_summary(hist[0], want)
    assert len(seen) == 2 and hist[0]["val_recon_rows"] == 2 * B
    loss = hist[0]["val_Reconstruction_Loss"]
    print("mean mse", ref_rec[:, 0].mean(), "val_Reconstruction_Loss", loss)
    assert abs(ref_rec[:, 0].mean() - loss) <= RTOL * loss
    res = exp.val_recon[""].result()
    assert res["worst_rows"].tolist() == np.argsort(ref_rec[:, 3], kind="stable")[:4].tolist()
    flat_r, flat_t = torch.cat([p[0] for p in seen]), torch.cat([p[1] for p in seen])
    rows = torch.as_tensor(res["worst_rows"].astype(np.int64), device=dev)
    assert torch.equal(res["worst_recons"], flat_r[rows]) and torch.equal(res["worst_target"], flat_t[rows])


# ---- 4. ema_eval ---------------------------------------------------------------------------------------------
def test_ema_eval_describes_the_averaged_weights(dev):
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.evalrun import eval_mode
    train, val = _batches(dev, 3), _batches(dev, 2, seed=4900)
    got, want = {}, {}
    for ema_eval in (True, False):
        extra = {} if ema_eval else {"ema_eval": False}
        exp = VAEXperiment(_vanilla(dev), dict(EXP, LR=1e-2, hipgraph=False, ema_decay=0.5, recon_stats=True, recon_stats_worst=0,
                                               **extra))
        exp.fit(lambda: iter(train), None, max_epochs=1)
        torch.manual_seed(7)               # without gradients the latent noise comes from torch's device generator
        got[ema_eval] = exp.fit(lambda: iter([]), lambda: iter(val), max_epochs=1)[0]["val_recon_psnr"]
        torch.manual_seed(7)               # the same draws for the forward passes below
        with exp.ema_weights() if ema_eval else torch.no_grad():
            with eval_mode(exp.model), torch.no_grad():
                pairs = [exp.model(b[0], labels=b[1])[:2] for b in val]
            want[ema_eval] = _ref_of(pairs)[0]["psnr"]
        assert not exp.ema.swapped
    print(got, want)
    assert abs(want[True] - want[False]) > 10 * RTOL * want[False], "the averaged and the live weights give the same PSNR"
    for k in (True, False):
        assert abs(got[k] - want[k]) <= RTOL * want[k]


# ---- 5. CT-MCQ-VAE: one accumulator per picture mode ---------------------------------------------------------
def test_ct_modes_feed_separate_accumulators(dev, fixed_noise, tmp_path):
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    m = build_ct(dev, 5)
    exp = VAEXperiment(m, dict(CT_PARAMS, recon_stats=True, recon_stats_worst=2), sample_dir=str(tmp_path), run_name="ct")
    seen = {"_base": [], "_action": []}
    for sfx in seen:
        _spy(exp.val_recon[sfx], seen[sfx])
    val = [_ct_batch(dev, 300, "base"), _ct_batch(dev, 301, "action", [0, 3, 0, 3]), _ct_batch(dev, 302, "causal", [1, 5, 2, 9]),
           _ct_batch(dev, 303, "base")]
    rec = exp.fit(lambda: iter([]), lambda: iter(val), max_epochs=1)[0]
    assert len(seen["_base"]) == 2 and len(seen["_action"]) == 1                      # the causal batch fed none
    assert rec["val_recon_rows_base"] == 2 * B and rec["val_recon_rows_action"] == B
    assert rec["val_recon_rows_base"] + rec["val_recon_rows_action"] == (len(val) - 1) * B
    assert not any(k.startswith("val_recon_") and not k.endswith(("_base", "_action")) for k in rec)
    assert torch.equal(seen["_action"][0][1], val[1][2]["input_y"]), "in action mode the target is input_y"
    assert torch.equal(seen["_base"][1][1], val[3][0])
    for sfx in seen:
        _assert_summary(rec, _ref_of(seen[sfx])[0], suffix=sfx)
        assert (tmp_path / "Recon" / f"recon_stats_ct{sfx}_Epoch_0.npz").is_file()
        assert (tmp_path / "Recon" / f"worst_ct{sfx}_Epoch_0.png").is_file()
    name, cfg = "IWAE", dict(in_channels=3, latent_dim=16)
    with pytest.raises(ValueError, match="recon_stats.*IWAE"):
        VAEXperiment(vae_models[name](**cfg).to(dev), dict(EXP, recon_stats=True))


# ---- 6. the tool ---------------------------------------------------------------------------------------------
def _tool_cfg(tmp_path, name):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    cfg["data_params"]["train_batch_size"] = cfg["data_params"]["val_batch_size"] = 4
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p), cfg


def test_tool_on_a_checkpoint(dev, tmp_path, monkeypatch):
    from ctvae_amd import recon_stats, reconstats
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.run import SyntheticData
    exp = VAEXperiment(_vanilla(dev), dict(EXP, LR=1e-2, hipgraph=False, ema_decay=0.5))
    exp.fit(lambda: iter(_batches(dev, 3)), None, max_epochs=1)
    state = {"state_dict": {"model." + k: v.detach().cpu().contiguous() for k, v in exp.model.state_dict().items()}, "epoch": 0,
             "ema_state_dict": {"model." + k: v for k, v in exp.ema_model_state_dict().items()}}
    ckpt = tmp_path / "both.ckpt"
    torch.save(state, ckpt)
    cfg_path, cfg = _tool_cfg(tmp_path, "vae.yaml")
    seen, inner = [], reconstats.ReconStats.observe

    def observe(self, recons, target):
        seen.append((recons.detach().clone(), target.detach().clone()))
        inner(self, recons, target)
    monkeypatch.setattr(reconstats.ReconStats, "observe", observe)
    torch.manual_seed(123)
    before = (torch.get_rng_state(), torch.cuda.get_rng_state(dev))
    out = tmp_path / "out"
    summary = recon_stats.main(["-c", cfg_path, "--checkpoint", str(ckpt), "--out", str(out), "--worst", "3"])
    assert torch.equal(torch.get_rng_state(), before[0]) and torch.equal(torch.cuda.get_rng_state(dev), before[1])
    assert sorted(os.listdir(out)) == sorted(recon_stats.FILES)
    on_disk = json.load(open(out / "recon_stats.json"))
    assert on_disk == summary and on_disk["rows"] == 8 * 4 == sum(len(p[0]) for p in seen)
    want, ref_rec, _ = _ref_of(seen)
    _assert_summary(on_disk, want, prefix="")
    npz = np.load(out / "recon_stats.npz")
    assert npz["worst_rows"].tolist() == np.argsort(ref_rec[:, 3], kind="stable")[:3].tolist()
    assert _png_size(out / "worst.png") == (3 * 66 + 2, 2 * 66 + 2)
    # the averaged weights, the default directory, no picture: other numbers, two files
    del seen[:]
    ema = recon_stats.main(["-c", cfg_path, "--checkpoint", str(ckpt), "--ema", "--worst", "0"])
    d = tmp_path / "logs" / cfg["logging_params"]["name"] / "recon_stats"
    assert sorted(os.listdir(d)) == sorted(recon_stats.FILES[:2]) and ema["psnr"] != summary["psnr"]
    _assert_summary(ema, _ref_of(seen)[0], prefix="")
    # collect() on a live model in training mode: its BatchNorm buffers, parameters, flag and the generators stay as found
    model = exp.model.train()
    data = SyntheticData(cfg["data_params"], cfg["model_params"], dev, 0, 1, steps_per_epoch=2, seed=3)
    snap = ({k: v.clone() for k, v in model.named_buffers()}, model.flat_params.clone(), torch.get_rng_state(),
            torch.cuda.get_rng_state(dev), model._rng_state.clone())
    stats = recon_stats.collect(model, data.test(), 1.0, 2, seed=3)
    assert stats[""].result()["flags"].shape == (8,) and model.training
    assert all(torch.equal(v, snap[0][k]) for k, v in model.named_buffers()) and torch.equal(model.flat_params, snap[1])
    assert torch.equal(torch.get_rng_state(), snap[2]) and torch.equal(torch.cuda.get_rng_state(dev), snap[3])
    assert torch.equal(model._rng_state, snap[4])
