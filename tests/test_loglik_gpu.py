"""GPU: the importance-sampled log-likelihood through a model, through ``python -m ctvae_amd.log_likelihood`` on a saved
checkpoint, and through the training harness (``exp_params.val_loglik``): loglik.ImportanceLogLik on csrc/loglik.hip.

The reference is the float64 restatement of tests/loglik_checks.py on the very tensors the library saw -- a spy on ``decode``
records every z and xhat, the noise is redrawn from a generator seeded alike -- so the two differ by the summation order of
float64 sums and by the device's ``exp``: 1e-10 relative leaves four digits."""
import io
import json
import math
import os

import numpy as np
import pytest
import torch

from ctvae_amd import filler
from tests import helpers as H
from tests import loglik_checks as C
from tests.test_grad_accum_gpu import EXP, _assert_same, _snapshot, _vanilla
from tests.test_latent_stats_gpu import _epochs, _lines, _save, _tool_cfg

pytestmark = pytest.mark.gpu
RECORD = {"val_loglik", "val_loglik_elbo", "val_loglik_gap", "val_loglik_ess", "val_loglik_rows", "val_loglik_nonfinite"}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _mk(dev, n, bs, seed):
    return [(filler.synthetic_batch(seed + i, bs)[0].to(dev), torch.zeros(bs, device=dev)) for i in range(n)]


def _model(name, dev):
    if name == "VanillaVAE":
        return _vanilla(dev)
    from ctvae_amd.models import vae_models
    m = vae_models["IWAE"](in_channels=3, latent_dim=128, num_samples=2)
    m.load_state_dict(filler.fill_state(H.vanilla_specs(), 1266))
    return m.to(dev).train()


def _nchw(t):
    return t.detach().cpu().contiguous().reshape(t.size(0), -1).numpy()


def _restate(x, log_var, seen, eps, sigma):
    """(loglik, elbo, ess) of the restatement over the chunks the library saw: ``seen`` [(z, xhat)], ``eps`` the chunks' noise."""
    B = x.size(0)
    state, flags = C.new_state(B)
    for (z, xhat), e in zip(seen, eps):
        S = z.size(0) // B
        lw, _ = C.log_weights(_nchw(xhat), _nchw(x), S, z.cpu().numpy(), e.reshape(B * S, -1).cpu().numpy(), log_var.cpu().numpy(), sigma)
        C.merge(state, flags, lw, S)
    assert not flags.any()
    return C.finish(state)


# ---- 1. the whole path through a model ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["VanillaVAE", "IWAE"])
def test_whole_path_follows_the_restatement(dev, name):
    from ctvae_amd import loglik
    from ctvae_amd.evalrun import eval_mode
    model = _model(name, dev)
    B, K_, chunk, sigma = 4, 8, 4, 0.5
    x = filler.synthetic_batch(4100, B)[0].to(dev)
    inner, seen = loglik.decoder_of(model), []

    def decode(z):
        xhat = inner(z)
        seen.append((z.clone(), xhat.clone()))
        return xhat

    acc = loglik.ImportanceLogLik(model.latent_dim, 3 * 64 * 64, sigma, K_, chunk, dev)
    with eval_mode(model):
        mu, log_var = model.encode(x)
        acc.add_batch(loglik.images_for(model, x), mu, log_var, decode, torch.Generator(device=dev).manual_seed(77))
    g = torch.Generator(device=dev).manual_seed(77)
    eps = [torch.randn((B, chunk, model.latent_dim), generator=g, device=dev) for _ in range(K_ // chunk)]
    assert len(seen) == 2 and all(tuple(z.shape) == (B * chunk, model.latent_dim) and tuple(xh.shape) == (B * chunk, 3, 64, 64)
                                  for z, xh in seen)
    res = acc.result()
    want = _restate(x, log_var, seen, eps, sigma)
    for k, w in zip(("loglik", "elbo", "ess"), want):
        err = np.abs(res[k] - w) / np.abs(w)
        print(name, k, res[k], "rel err", err.max())
        assert np.all(err <= 1e-10), k
    assert not res["nonfinite"].any() and np.all(res["loglik"] >= res["elbo"])
    assert np.all(res["ess"] >= 1) and np.all(res["ess"] <= K_)


# ---- 2. the tool on a saved checkpoint ---------------------------------------------------------------------
def test_tool_on_a_saved_checkpoint(dev, tmp_path):
    from ctvae_amd import log_likelihood as LL
    from ctvae_amd.evalrun import eval_mode
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.run import SyntheticData
    exp = VAEXperiment(_vanilla(dev), dict(EXP, LR=1e-2, hipgraph=False, ema_decay=0.5))
    exp.fit(_epochs(_mk(dev, 4, 4, 4100), 2), None, max_epochs=2)
    plain, both = tmp_path / "plain.ckpt", tmp_path / "both.ckpt"
    _save(exp.model, plain)
    _save(exp.model, both, ema=exp.ema_model_state_dict())
    cfg_path, cfg = _tool_cfg(tmp_path, "vae.yaml")
    with pytest.raises(SystemExit, match="log_likelihood: --ema.*plain.ckpt holds no ema_state_dict"):
        LL.main(["-c", cfg_path, "--checkpoint", str(plain), "--ema"])
    assert not (tmp_path / "logs").exists()
    args = ["--samples", "8", "--chunk", "3", "--rows", "10"]               # (the last chunk is short: 3 + 3 + 2)
    torch.manual_seed(123)
    before = (torch.get_rng_state(), torch.cuda.get_rng_state(dev))
    out = tmp_path / "out"
    summary = LL.main(["-c", cfg_path, "--checkpoint", str(both), "--out", str(out)] + args)
    assert torch.equal(torch.get_rng_state(), before[0]) and torch.equal(torch.cuda.get_rng_state(dev), before[1])
    assert sorted(os.listdir(out)) == sorted(LL.FILES) == ["log_likelihood.json", "log_likelihood.npz"]
    on_disk = json.load(open(out / "log_likelihood.json"))
    assert on_disk == json.loads(json.dumps(summary))
    assert set(on_disk) == {"loglik", "loglik_per_dim", "elbo", "gap", "ess_mean", "ess_min", "rows", "nonfinite", "sigma", "sigma_source",
                            "samples", "chunk", "arguments"}
    assert on_disk["rows"] == 10 and on_disk["nonfinite"] == 0 and on_disk["samples"] == 8 and on_disk["chunk"] == 3
    assert on_disk["sigma_source"] == "mse" and on_disk["gap"] >= 0 and 1 <= on_disk["ess_min"] <= on_disk["ess_mean"] <= 8
    assert on_disk["loglik_per_dim"] == on_disk["loglik"] / 12288
    z = np.load(out / "log_likelihood.npz")
    assert sorted(z.files) == ["elbo", "ess", "loglik", "nonfinite"] and all(len(z[k]) == 10 for k in z.files)
    assert z["loglik"].dtype == np.float64 and z["nonfinite"].dtype == np.int32
    assert on_disk["loglik"] == math.fsum(z["loglik"].tolist()) / 10 and np.all(z["loglik"] >= z["elbo"])
    # sigma: mse is the restatement's over decode(mu) of the same ten rows, under the checkpoint's own weights
    seed = int(cfg["exp_params"].get("manual_seed", 0) or 0)
    data = SyntheticData(cfg["data_params"], cfg["model_params"], dev, 0, 1, seed=seed)
    sse, model = [], exp.model
    with eval_mode(model):
        for xb, _ in list(data.test())[:3]:
            sse.append(C.sse_rows(_nchw(model.decode(model.encode(xb)[0])), _nchw(xb), 1))
    want = math.sqrt(math.fsum(np.concatenate(sse)[:10].tolist()) / (10 * 12288))
    print("sigma", on_disk["sigma"], "restated", want)
    assert abs(on_disk["sigma"] - want) <= 1e-10 * want
    # two runs write identical bytes
    again = tmp_path / "again"
    LL.main(["-c", cfg_path, "--checkpoint", str(both), "--out", str(again)] + args)
    for f in LL.FILES[1:]:
        assert open(out / f, "rb").read() == open(again / f, "rb").read()
    second = json.load(open(again / "log_likelihood.json"))
    assert {k: v for k, v in second.items() if k != "arguments"} == {k: v for k, v in on_disk.items() if k != "arguments"}
    # a given sigma, the averaged weights, the default output directory: other numbers
    ema = LL.main(["-c", cfg_path, "--checkpoint", str(both), "--ema", "--sigma", "0.5", "--samples", "2", "--rows", "4"])
    d = tmp_path / "logs" / cfg["logging_params"]["name"] / "log_likelihood"
    assert sorted(os.listdir(d)) == sorted(LL.FILES)
    assert ema["sigma"] == 0.5 and ema["sigma_source"] == "given" and ema["rows"] == 4 and ema["chunk"] == 2


# ---- 3. the harness ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hipgraph", [True, False])
def test_harness_records_and_training_does_not_notice(dev, tmp_path, hipgraph):
    from ctvae_amd.experiment import VAEXperiment
    bs, nval = 4, 3
    train, val = _mk(dev, 4, bs, 4100), _mk(dev, nval, bs, 4900)
    finals, rngs, recs, logs = {}, {}, {}, {}
    for key, extra in (("plain", {}), ("loglik", {"val_loglik": {"samples": 4, "sigma": 0.5}})):
        log = io.StringIO()
        exp = VAEXperiment(_vanilla(dev), dict(EXP, hipgraph=hipgraph, **extra), log_file=log, sample_dir=str(tmp_path / key),
                           run_name="run")
        torch.manual_seed(5)
        hist = exp.fit(_epochs(train, 2), lambda: iter(val), max_epochs=2)
        assert exp.global_step == 4
        finals[key] = _snapshot(exp)
        rngs[key] = (exp.model._rng_state.clone(), torch.get_rng_state(), torch.cuda.get_rng_state(dev))
        recs[key], logs[key] = hist, log
        if key == "plain":                 # no buffer, no launch, no file, no key
            assert exp.val_loglik is None and exp.loglik_cfg is None and not (tmp_path / key).exists()
            assert not any("loglik" in k for k in hist[1]) and not _lines(log, "val_loglik_rows")
    _assert_same(finals["plain"], finals["loglik"], "with and without val_loglik")
    for a, b in zip(rngs["plain"], rngs["loglik"]):
        assert torch.equal(a, b)
    for e in range(2):
        for k, v in recs["plain"][e].items():      # every validation key that existed keeps its value
            if k != "epoch_seconds":
                assert recs["loglik"][e][k] == v, k
        rec = {k: v for k, v in recs["loglik"][e].items() if "loglik" in k}
        print(rec)
        assert set(rec) == RECORD and set(recs["loglik"][e]) - set(recs["plain"][e]) == RECORD
        assert rec["val_loglik_rows"] == nval * bs and rec["val_loglik_nonfinite"] == 0
        assert rec["val_loglik_gap"] == rec["val_loglik"] - rec["val_loglik_elbo"] and rec["val_loglik_gap"] >= 0
        assert 1 <= rec["val_loglik_ess"] <= 4
    lines = _lines(logs["loglik"], "val_loglik_rows")
    assert len(lines) == 2
    for e, line in enumerate(lines):
        assert {k: v for k, v in line.items() if k != "step"} == {k: v for k, v in recs["loglik"][e].items() if "loglik" in k}
        assert line["step"] == 2 * (e + 1)
    assert sorted(os.listdir(tmp_path / "loglik" / "Loglik")) == ["loglik_run_Epoch_0.npz", "loglik_run_Epoch_1.npz"]
    z = np.load(tmp_path / "loglik" / "Loglik" / "loglik_run_Epoch_1.npz")
    assert sorted(z.files) == ["elbo", "ess", "loglik", "nonfinite"] and len(z["loglik"]) == nval * bs
    assert recs["loglik"][1]["val_loglik"] == math.fsum(z["loglik"].tolist()) / (nval * bs)


def test_harness_feeds_an_iwae_and_refuses_other_models(dev):
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    val = _mk(dev, 2, 4, 4900)
    exp = VAEXperiment(_model("IWAE", dev), dict(EXP, val_loglik={"samples": 5, "sigma": 0.5, "chunk": 2}))
    hist = exp.fit(lambda: iter(_mk(dev, 1, 4, 4100)), lambda: iter(val), max_epochs=1)
    rec = {k: v for k, v in hist[0].items() if "loglik" in k}
    assert set(rec) == RECORD and rec["val_loglik_rows"] == 8 and rec["val_loglik_nonfinite"] == 0 and rec["val_loglik_gap"] >= 0
    with pytest.raises(ValueError, match="val_loglik: log_likelihood needs a model.*got VampVAE"):
        VAEXperiment(vae_models["VampVAE"](in_channels=3, latent_dim=16), dict(EXP, val_loglik={"samples": 4, "sigma": 0.5}))
