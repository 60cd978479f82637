"""GPU: ctvae_amd/metrics.py end to end -- Metric / MetricSet over a 6 x 5 x 4 factor grid of 120 images against the numpy
restatement of tests/metrics_checks.py fed the same plan and the same codes, through a real model, through the harness
(fit() with and without val_metric must train bit for bit the same) and through the runner."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from tests import metrics_checks as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (6, 5, 4)
# brightness of channel k per value of factor k: between the column's minimum and maximum none sits on the 1/20 grid
LEVELS = ([10, 47, 95, 131, 188, 240], [15, 70, 122, 171, 233], [30, 90, 163, 222])
CONST = 0.3125


def grid_images():
    """[120, 64, 64, 3] uint8: item = np.ravel_multi_index(factor values, SIZES); channel k is flat at LEVELS[k][value k]."""
    pos = np.stack(np.unravel_index(np.arange(120), SIZES), axis=-1)
    img = np.zeros((120, 64, 64, 3), dtype=np.uint8)
    for k in range(3):
        img[:, :, :, k] = np.array(LEVELS[k], dtype=np.uint8)[pos[:, k]][:, None, None]
    return img


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda")


@pytest.fixture(scope="module")
def dataset(dev):
    from ctvae_amd import data as D
    from ctvae_amd import metrics as M
    store = D.HbmImageStore(torch.from_numpy(grid_images()), dev, crop=64, size=64)
    return M.FactorData(store, M.FactorGrid(SIZES))


NOISE = np.random.default_rng(77).uniform(0.0, 1.0, 120).astype(np.float32)


def analytic_repr(x):
    """[B, 3, 64, 64] on the device -> [B, 5]: the three channel means (exact: float64 sum of 4096 equal values), one constant
    column, one column of fixed pseudo-noise looked up by the item the three levels identify."""
    means = x.double().mean(dim=(2, 3))
    item = torch.zeros(x.size(0), dtype=torch.int64, device=x.device)
    for k in range(3):
        lv = torch.tensor(LEVELS[k], dtype=torch.float64, device=x.device) / 255.0
        item = item * SIZES[k] + (means[:, k:k + 1] - lv[None, :]).abs().argmin(dim=1)
    noise = torch.from_numpy(NOISE).to(x.device)[item]
    return torch.cat([means.float(), torch.full_like(noise, CONST)[:, None], noise[:, None]], dim=1)


def _codes(dataset, rows):
    shape = np.shape(rows)
    z = analytic_repr(dataset.items(np.reshape(rows, -1))).cpu().numpy()
    return z.reshape(shape + (z.shape[-1],))


def test_fetch_follows_the_grid(dataset):
    f = np.array([[5, 0, 3], [2, 4, 1]])
    x = dataset.observations(f)
    want = torch.tensor([[240, 15, 222], [95, 233, 90]], dtype=torch.float32) / 255.0
    assert torch.equal(x[:, :, 7, 9].cpu(), want) and x.shape == (2, 3, 64, 64)


def test_mig_equals_the_restatement(dataset):
    from ctvae_amd import metrics as M
    metric = M.Metric("MIG", dataset, batch_size=16, num_train=200, seed=11)
    got = metric.compute(analytic_repr)
    plan = metric.plan()
    want = C.ref_mig(_codes(dataset, plan["rows"]), plan["factors"], SIZES)       # asserts the edge margin of these codes
    print(f"mig: got {got['mig.discrete_score']:.8f} restatement {want:.8f}")
    assert list(got) == ["mig.discrete_score"]
    assert abs(got["mig.discrete_score"] - want) <= 1e-5
    assert 0.5 < want <= 1.0
    other = metric.compute(analytic_repr, seed=12)["mig.discrete_score"]
    assert other != got["mig.discrete_score"] and got == metric.compute(analytic_repr)


def test_factor_vae_score_equals_the_restatement(dataset):
    from ctvae_amd import metrics as M
    metric = M.Metric("FactorVaeScore", dataset, batch_size=16, num_train=40, num_test=20, seed=11)
    got = metric.compute(analytic_repr)
    plan = metric.plan()
    want = C.ref_factor_vae(_codes(dataset, plan["variance_rows"]), _codes(dataset, plan["train_rows"]), plan["train_factor"],
                            _codes(dataset, plan["eval_rows"]), plan["eval_factor"], 3)
    assert got == want
    assert got == {"factor_vae.train_accuracy": 1.0, "factor_vae.eval_accuracy": 1.0, "factor_vae.num_active_dims": 4}
    dead = metric.compute(lambda x: torch.zeros(x.size(0), 5, device=x.device))
    assert dead == {"factor_vae.train_accuracy": 0.0, "factor_vae.eval_accuracy": 0.0, "factor_vae.num_active_dims": 0}


def _vanilla(dev, seed=1266):
    from ctvae_amd import filler
    from ctvae_amd import specs as H
    from ctvae_amd.models import vae_models
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
    m.load_state_dict(filler.fill_state(H.vanilla_specs(), seed))
    return m.to(dev).train()


PARAMS = {"LR": 0.005, "weight_decay": 0.0, "scheduler_gamma": 0.95, "kld_weight": 0.00025, "manual_seed": 1265}
KEYS = ["factor_vae.eval_accuracy", "factor_vae.num_active_dims", "factor_vae.train_accuracy", "mig.discrete_score"]


def test_metric_set_through_a_real_model(dev, dataset):
    from ctvae_amd import metrics as M
    from ctvae_amd.experiment import VAEXperiment
    exp = VAEXperiment(_vanilla(dev), dict(PARAMS))
    ms = M.MetricSet(["MIG", "FactorVaeScore"], dataset, batch_size=16, num_train=32, num_test=16, seed=3)
    cpu_rng, dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state(dev)
    p0 = exp.model.flat_params.clone()
    res = ms.compute(exp.metric_func)
    assert sorted(res) == KEYS
    assert all(np.isfinite(v) for v in res.values())
    assert 0.0 <= res["mig.discrete_score"] <= 1.0
    assert 0.0 <= res["factor_vae.train_accuracy"] <= 1.0 and 0.0 <= res["factor_vae.eval_accuracy"] <= 1.0
    assert 0 <= res["factor_vae.num_active_dims"] <= 128
    # the model is back in training mode, and nothing random or trainable moved
    assert exp.model.training and all(m.training for m in exp.model.modules())
    assert torch.equal(cpu_rng, torch.get_rng_state()) and torch.equal(dev_rng, torch.cuda.get_rng_state(dev))
    assert torch.equal(p0, exp.model.flat_params)
    exp.model.eval()
    ms.compute(exp.metric_func)
    assert not exp.model.training


def test_val_metric_changes_nothing_but_the_records(dev, dataset):
    """Two epochs of fit() on the same batches with and without val_metric: the flat parameter buffer bit for bit, the epoch
    records equal apart from the added val_mig.* / val_factor_vae.* keys (and the wall time)."""
    from ctvae_amd import filler, metrics as M
    from ctvae_amd.experiment import VAEXperiment
    zeros = torch.zeros(8, device=dev)
    train = [(filler.synthetic_batch(40 + i, 8)[0].to(dev), zeros) for i in range(5)]
    val = [(filler.synthetic_batch(90 + i, 8)[0].to(dev), zeros) for i in range(2)]
    out = {}
    for with_metric in (False, True):
        torch.manual_seed(5)
        ms = M.MetricSet(["MIG", "FactorVaeScore"], dataset, batch_size=16, num_train=32, num_test=16) if with_metric else None
        exp = VAEXperiment(_vanilla(dev), dict(PARAMS), val_metric=ms)
        hist = exp.fit(lambda: iter(train), lambda: iter(val), max_epochs=2)
        torch.cuda.synchronize()
        out[with_metric] = (exp.model.flat_params.clone(), hist)
    assert torch.equal(out[False][0], out[True][0])
    for plain, full in zip(out[False][1], out[True][1]):
        assert sorted(set(full) - set(plain)) == ["val_" + k for k in KEYS]
        assert {k: v for k, v in plain.items() if k != "epoch_seconds"} == \
               {k: v for k, v in full.items() if k in plain and k != "epoch_seconds"}
    a, b = out[True][1]
    assert a["val_mig.discrete_score"] != b["val_mig.discrete_score"]          # another epoch: other weights, another seed


def _runner_cfg(tmp_path, sub, metrics, **data):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "vae.yaml")))
    npy = tmp_path / "grid.npy"
    if not npy.exists():
        np.save(npy, grid_images())
    cfg["data_params"].update(dataset_name="shapes", data_path=str(tmp_path), hbm_images=str(npy), hbm_factor_sizes=list(SIZES),
                              crop_size=64, train_batch_size=8, val_batch_size=8)
    cfg["data_params"].update(data)
    for k, v in data.items():
        if v is None:
            del cfg["data_params"][k]
    cfg["exp_params"]["metrics"] = metrics
    cfg["trainer_params"].update(gpus=[0], max_epochs=1)
    cfg["logging_params"]["save_dir"] = str(tmp_path / sub)
    p = tmp_path / f"{sub}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_builds_the_metric_set_from_the_yaml(dev, tmp_path):
    from ctvae_amd import run
    hist = run.main(["-c", _runner_cfg(tmp_path, "ok", ["MIG", "FactorVaeScore"])])
    assert all("val_" + k in hist[-1] for k in KEYS)
    lines = [json.loads(l) for l in open(tmp_path / "ok" / "VanillaVAE" / "metrics_rank0.jsonl")]
    logged = [l for l in lines if "val_mig.discrete_score" in l]
    assert len(logged) == 1 and all(logged[0]["val_" + k] == hist[-1]["val_" + k] for k in KEYS)
    with pytest.raises(SystemExit, match="DCI.*gradient-boosted"):
        run.main(["-c", _runner_cfg(tmp_path, "dci", ["DCI"])])
    with pytest.raises(SystemExit, match="hbm_factor_sizes"):
        run.main(["-c", _runner_cfg(tmp_path, "nosizes", ["MIG"], hbm_factor_sizes=None)])
    with pytest.raises(SystemExit, match="synthetic"):
        run.main(["-c", _runner_cfg(tmp_path, "synth", ["MIG"], hbm_images=None), "--steps-per-epoch", "2"])
    with pytest.raises(SystemExit, match="120 items"):
        run.main(["-c", _runner_cfg(tmp_path, "wrong", ["MIG"], hbm_factor_sizes=[6, 5, 5])])
