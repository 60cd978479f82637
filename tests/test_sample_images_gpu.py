"""GPU: VAEXperiment.sample_images / fit(..., test_batches=) / exp_params.val_sampling -- the reference's end-of-validation
picture grids (experiment.py:114-150): the files and their contents, that the training run does not notice them, the models
whose sample / generate differ (VQVAE, ConditionalVAE, CTMCQVAE), and the runner."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import grid_checks as G
from tests import helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"LR": 0.005, "weight_decay": 0.0, "scheduler_gamma": 0.95, "kld_weight": 0.00025, "manual_seed": 1265}
B = 16
GRID_16 = (2 * 66 + 2, 12 * 66 + 2)          # 16 images of 64 x 64, nrow 12, padding 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", torch.cuda.current_device())


def _vanilla(dev, seed=1266):
    from ctvae_amd import filler
    from ctvae_amd import specs
    from ctvae_amd.models import vae_models
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
    m.load_state_dict(filler.fill_state(specs.vanilla_specs(), seed))
    return m.to(dev).train()


def _batches(dev, base, n, bs=B):
    from ctvae_amd import filler
    zeros = torch.zeros(bs, device=dev)
    return [(filler.synthetic_batch(base + i, bs)[0].to(dev), zeros) for i in range(n)]


def _png(path):
    with open(path, "rb") as f:
        img, kinds = G.read_png(f.read())
    assert kinds == ["IHDR", "IDAT", "IEND"]
    return img


def _grid(x):
    from ctvae_amd import imagegrid
    return imagegrid.make_grid_u8(x, nrow=12, normalize=True).cpu().numpy()


def _fit(dev, sample_dir, val_sampling=True):
    from ctvae_amd.experiment import VAEXperiment
    train, val, test = _batches(dev, 40, 4), _batches(dev, 90, 2), _batches(dev, 70, 2)
    torch.manual_seed(5)
    exp = VAEXperiment(_vanilla(dev), dict(PARAMS), val_sampling=val_sampling, sample_dir=sample_dir, run_name="Vanilla")
    hist = exp.fit(lambda: iter(train), lambda: iter(val), max_epochs=2, test_batches=lambda: iter(test))
    torch.cuda.synchronize()
    return exp, hist, test


def test_vanilla_writes_the_three_grids_per_epoch(dev, tmp_path):
    exp, hist, test = _fit(dev, str(tmp_path))
    names = {d: sorted(os.listdir(tmp_path / d)) for d in ("Inputs", "Reconstructions", "Samples")}
    assert names == {"Inputs": ["inputs_Vanilla_Epoch_0.png", "inputs_Vanilla_Epoch_1.png"],
                     "Reconstructions": ["recons_Vanilla_Epoch_0.png", "recons_Vanilla_Epoch_1.png"],
                     "Samples": ["sample_Vanilla_Epoch_0.png", "sample_Vanilla_Epoch_1.png"]}
    pics = {(d, f): _png(tmp_path / d / f) for d, fs in names.items() for f in fs}
    assert all(p.shape == GRID_16 + (3,) for p in pics.values())
    want_in = _grid(test[0][0])                             # only the FIRST test batch is read
    for e in (0, 1):
        assert np.array_equal(pics[("Inputs", f"inputs_Vanilla_Epoch_{e}.png")], want_in)
    # the last epoch's reconstruction and sample: the trained model in eval mode, the draws seeded manual_seed * 1000003 + epoch
    assert not exp.model.training
    with torch.no_grad(), torch.random.fork_rng(devices=[dev]):
        torch.manual_seed(1265 * 1_000_003 + 1)
        recons = exp.model.generate(test[0][0], labels=test[0][1])
        sample = exp.model.sample(16, dev, labels=test[0][1][:16])
    assert np.array_equal(pics[("Reconstructions", "recons_Vanilla_Epoch_1.png")], _grid(recons))
    assert np.array_equal(pics[("Samples", "sample_Vanilla_Epoch_1.png")], _grid(sample))
    assert not np.array_equal(pics[("Reconstructions", "recons_Vanilla_Epoch_0.png")], pics[("Reconstructions", "recons_Vanilla_Epoch_1.png")])
    assert not np.array_equal(pics[("Samples", "sample_Vanilla_Epoch_0.png")], pics[("Samples", "sample_Vanilla_Epoch_1.png")])


def test_sampling_leaves_the_run_untouched(dev, tmp_path):
    """Two epochs x four steps (the fourth of a signature is captured into a hipGraph and replayed) with sampling on and off:
    parameters, BatchNorm buffers, Adam moments, the in-kernel noise state, the epoch records and torch's generators agree."""
    out = {}
    for on in (False, True):
        exp, hist, _ = _fit(dev, str(tmp_path / "on"), val_sampling=on)
        assert any(g.graph is not None for g in exp._graphed.values())
        out[on] = dict(state={k: v.clone() for k, v in exp.model.state_dict().items()}, flat=exp.model.flat_params.clone(),
                       opt={k: v.clone() for k, v in exp.optimizer.state_dict().items() if torch.is_tensor(v)},
                       model_rng=exp.model._rng_state.clone(), hist=hist, cpu_rng=torch.get_rng_state(),
                       dev_rng=torch.cuda.get_rng_state(dev), training=[m.training for m in exp.model.modules()])
    assert os.path.isdir(tmp_path / "on" / "Samples") and len(os.listdir(tmp_path / "on" / "Samples")) == 2
    off, on = out[False], out[True]
    assert off["state"].keys() == on["state"].keys() and any("running_mean" in k for k in on["state"])
    for k in on["state"]:
        assert torch.equal(off["state"][k], on["state"][k]), k
    assert torch.equal(off["flat"], on["flat"])
    assert {"exp_avg", "exp_avg_sq", "state"} <= set(on["opt"])
    for k in on["opt"]:
        assert torch.equal(off["opt"][k], on["opt"][k]), k
    assert torch.equal(off["model_rng"], on["model_rng"])
    strip = lambda recs: [{k: v for k, v in r.items() if k != "epoch_seconds"} for r in recs]      # noqa: E731
    assert strip(off["hist"]) == strip(on["hist"])
    assert torch.equal(off["cpu_rng"], on["cpu_rng"]) and torch.equal(off["dev_rng"], on["dev_rng"])
    assert off["training"] == on["training"]


def test_sampling_needs_every_switch(dev, tmp_path):
    """val_sampling off, no sample_dir, or no test_batches: nothing is written and nothing is asked of the test loader."""
    from ctvae_amd.experiment import VAEXperiment
    train, val = _batches(dev, 40, 1), _batches(dev, 90, 1)

    def never():
        raise AssertionError("the test loader was read")

    for kw, tb in ((dict(val_sampling=False, sample_dir=str(tmp_path)), never), (dict(val_sampling=True, sample_dir=None), never),
                   (dict(val_sampling=True, sample_dir=str(tmp_path)), None)):
        exp = VAEXperiment(_vanilla(dev), dict(PARAMS), **kw)
        exp.fit(lambda: iter(train), lambda: iter(val), max_epochs=1, test_batches=tb)
    assert os.listdir(tmp_path) == []


def test_vqvae_has_no_sampler(dev, tmp_path):
    """VQVAE.sample raises Warning: inputs and reconstructions are written, the sample file is skipped, nothing else is raised;
    the model's mode comes back; any other exception propagates."""
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    torch.manual_seed(3)
    m = vae_models["VQVAE"](**{**H.VQVAE_CFG, "hidden_dims": list(H.VQVAE_CFG["hidden_dims"])}).to(dev).train()
    exp = VAEXperiment(m, dict(PARAMS), val_sampling=True, sample_dir=str(tmp_path), run_name="VQVAE")
    batch = _batches(dev, 70, 1)[0]
    written = exp.sample_images(batch, 3)
    assert [os.path.relpath(p, tmp_path) for p in written] == [os.path.join("Inputs", "inputs_VQVAE_Epoch_3.png"),
                                                              os.path.join("Reconstructions", "recons_VQVAE_Epoch_3.png")]
    assert os.listdir(tmp_path / "Samples") == []
    assert _png(written[1]).shape == GRID_16 + (3,)
    assert m.training and all(x.training for x in m.modules())

    def boom(*a, **k):
        raise ValueError("not a Warning")
    m.sample = boom
    with pytest.raises(ValueError, match="not a Warning"):
        exp.sample_images(batch, 4)
    assert m.training


def test_conditional_vae_samples_with_the_first_labels(dev, tmp_path):
    """A 16-row test batch: 16 samples, decoded next to the batch's 16 label rows (the reference's fixed 32 could not be
    concatenated with them)."""
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    torch.manual_seed(4)
    m = vae_models["ConditionalVAE"](**H.CVAE_CFG).to(dev).train()
    exp = VAEXperiment(m, dict(PARAMS), val_sampling=True, sample_dir=str(tmp_path), run_name="CVAE")
    labels = H.cvae_labels(900, 40).to(dev)
    from ctvae_amd import filler
    seen = []
    orig = m.sample
    m.sample = lambda n, d, **kw: seen.append((n, kw["labels"].clone())) or orig(n, d, **kw)
    for rows, want_n in ((16, 16), (40, 32)):
        x = filler.synthetic_batch(71, rows)[0].to(dev)
        written = exp.sample_images((x, labels[:rows]), rows)
        assert len(written) == 3
        n, lab = seen[-1]
        assert n == want_n and torch.equal(lab, labels[:want_n])
        ymaps = -(-want_n // 12)
        assert _png(written[2]).shape == (ymaps * 66 + 2, 794, 3)
    with torch.no_grad(), torch.random.fork_rng(devices=[dev]):
        m.eval()
        torch.manual_seed(1265 * 1_000_003 + 40)
        x = filler.synthetic_batch(71, 40)[0].to(dev)
        m.generate(x, labels=labels)
        want = orig(32, dev, labels=labels[:32])
        m.train()
    assert np.array_equal(_png(written[2]), _grid(want))


def test_ctmcqvae_causal_batch_goes_through_generate(dev, tmp_path):
    """CTMCQVAE (action_dim 12) with a causal-mode option batch: generate() remaps causal -> action, so the reconstruction is
    a picture grid (forward_causal itself returns action probabilities [B, 12]); a per-row mode list counts as its one mode."""
    from ctvae_amd import filler
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
    cfg.update(action_dim=12)
    torch.manual_seed(11)
    m = vae_models["CTMCQVAE"](**cfg)
    m.load_state_dict(filler.fill_state(H.mcq_specs(H.CT_CONV_CFG), 12), strict=False)
    m = m.to(dev).train()
    exp = VAEXperiment(m, dict(PARAMS), val_sampling=True, sample_dir=str(tmp_path), run_name="CT")
    x, y, a = filler.synthetic_pairs(11, 6, 12)
    for e, mode in enumerate(("causal", ["causal"] * 6)):
        opts = {"mode": mode, "action": a.to(dev), "input_y": y.to(dev)}
        written = exp.sample_images((x.to(dev), torch.zeros(6, device=dev), opts), e)
        assert [os.path.basename(p) for p in written] == [f"inputs_CT_Epoch_{e}.png", f"recons_CT_Epoch_{e}.png", f"sample_CT_Epoch_{e}.png"]
        assert opts["mode"] == mode                                            # the caller's dict is not edited
        assert all(_png(p).shape == (68, 6 * 66 + 2, 3) for p in written)
    with torch.no_grad(), torch.random.fork_rng(devices=[dev]):
        m.eval()
        torch.manual_seed(1265 * 1_000_003 + 0)
        want = m(x.to(dev), mode="action", action=a.to(dev), input_y=y.to(dev))[0]
        m.train()
    assert np.array_equal(_png(os.path.join(tmp_path, "Reconstructions", "recons_CT_Epoch_0.png")), _grid(want))


def _cfg(tmp_path, sub, **exp_params):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "vae.yaml")))
    cfg["data_params"].update(train_batch_size=16, val_batch_size=16)
    cfg["exp_params"].update(exp_params)
    cfg["trainer_params"].update(gpus=[0])
    cfg["logging_params"]["save_dir"] = str(tmp_path / sub)
    p = tmp_path / f"{sub}.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_runner_val_sampling_key(dev, tmp_path):
    from ctvae_amd import run
    run.main(["-c", _cfg(tmp_path, "on", val_sampling=True), "--max-epochs", "1", "--steps-per-epoch", "2"])
    log = tmp_path / "on" / "VanillaVAE"
    for d, stem in (("Inputs", "inputs"), ("Reconstructions", "recons"), ("Samples", "sample")):
        assert os.listdir(log / d) == [f"{stem}_VanillaVAE_Epoch_0.png"]
        assert _png(log / d / f"{stem}_VanillaVAE_Epoch_0.png").shape == GRID_16 + (3,)
    run.main(["-c", _cfg(tmp_path, "off"), "--max-epochs", "1", "--steps-per-epoch", "2"])
    assert sorted(os.listdir(tmp_path / "off" / "VanillaVAE")) == ["checkpoints", "metrics_rank0.jsonl"]
