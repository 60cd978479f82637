"""GPU: ctvae_amd/rollout.py and the apply_action command on a CT-MCQ-VAE (action_dim 12, 64 x 64): the rollout against a plain
loop of the same model calls, the per-action accuracies against the model's own batch means and the numpy restatement, the
sheet against single pictures, that the caller's run does not notice any of it, and the command end to end."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from ctvae_amd import filler
from tests import grid_checks as G
from tests import helpers as H
from tests import rollout_checks as R
from tests.test_ct_gpu import _FixedNoise, build_ct

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B = 12, 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def noise(dev):
    """One deterministic noise source for the whole module: a call made by rollout.py and the same call made by a test draw
    the same noise whatever the torch generators hold."""
    from ctvae_amd.models import causal
    prev = causal.set_noise_source(_FixedNoise(dev))
    yield
    causal.set_noise_source(prev)


@pytest.fixture(scope="module")
def model(dev, noise):
    return build_ct(dev, 5)


@pytest.fixture(scope="module")
def x(dev):
    return filler.synthetic_pairs(21, B, A)[0].to(dev)


@pytest.fixture(scope="module")
def frames(model, x):
    from ctvae_amd import rollout
    return rollout.action_rollout(model, x[0], steps=3)


class _Eval:
    """What the test's own model calls run under: eval + no_grad, train mode back afterwards."""

    def __init__(self, m):
        self.m, self.ng = m, torch.no_grad()

    def __enter__(self):
        self.m.eval()
        self.ng.__enter__()

    def __exit__(self, *exc):
        self.ng.__exit__(*exc)
        self.m.train()


def _onehot(a, rows, dev):
    t = torch.zeros(rows, A, device=dev)
    t[:, a] = 1.0
    return t


def test_action_rollout_is_the_plain_loop(model, x, frames, dev):
    assert frames.shape == (4, A, 3, 64, 64) and frames.dtype == torch.float32
    assert torch.equal(frames[0], x[0].expand(A, -1, -1, -1))
    eye = torch.eye(A, device=dev)
    with _Eval(model):
        cur = x[0:1].expand(A, -1, -1, -1).contiguous()
        for s in range(1, 4):
            cur = model(cur, labels=None, mode=["action"] * A, action=eye, input_y=cur)[0]
            assert torch.equal(frames[s], cur), s
    assert not torch.equal(frames[1], frames[0]) and not torch.equal(frames[2], frames[1])
    from ctvae_amd import rollout
    assert torch.equal(rollout.action_rollout(model, x[0:1], steps=1), frames[:2])       # [1,3,H,W] is the same image
    with pytest.raises(ValueError, match="one image"):
        rollout.action_rollout(model, x[:2])


def test_rollout_leaves_the_run_as_found(dev, noise, x):
    """Train mode, every buffer and parameter, torch's generators and the parameter epoch are as before; the next training
    steps equal those of a twin that never ran a rollout."""
    from ctvae_amd import kernels as K
    from ctvae_amd import rollout
    from ctvae_amd.experiment import VAEXperiment
    batches = []
    for i in range(3):
        bx, by, ba = filler.synthetic_pairs(200 + i, B, A)
        mode = ["base", "action", "causal"][i]
        opts = {"mode": [mode] * B}
        if mode != "base":
            opts.update(input_y=by.to(dev), action=ba.to(dev))
        batches.append((bx.to(dev), torch.zeros(B, device=dev), opts))
    params = {"LR": 5e-4, "weight_decay": 0.0, "scheduler_gamma": 0.99, "kld_weight": 0.00025, "update_parameters": "ct_layer",
              "hipgraph": False}
    finals = {}
    for rolled in (False, True):
        m = build_ct(dev, 5)
        if rolled:
            state = {k: v.clone() for k, v in m.state_dict().items()}
            flags = [mod.training for mod in m.modules()]
            cpu_rng, dev_rng, epoch = torch.get_rng_state(), torch.cuda.get_rng_state(dev), K._param_epoch[0]
            rollout.action_rollout(m, x[0], steps=2)
            rollout.rollout_accuracy(m, x[:2], steps=1)
            rollout.split_accuracy(m, batches)
            assert m.training and [mod.training for mod in m.modules()] == flags
            after = m.state_dict()
            assert after.keys() == state.keys()
            for k in state:
                assert torch.equal(after[k], state[k]), k
            assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(dev), dev_rng)
            assert K._param_epoch[0] == epoch
        exp = VAEXperiment(m, dict(params))
        exp.fit(lambda: iter(batches), None, max_epochs=1)
        torch.cuda.synchronize()
        finals[rolled] = m.flat_params.clone()
    assert torch.isfinite(finals[True]).all()
    assert torch.equal(finals[True], finals[False]), float((finals[True] - finals[False]).abs().max())


def test_rollout_accuracy_follows_the_contract(model, x, dev):
    """steps = 2 over 4 images: per step the counts of hits_ref over the outputs of the same calls in the contract's order;
    per causal call the model's own causal_acc / causal_nodir_acc times B are that call's hit counts."""
    from ctvae_amd import rollout
    names = ["f0", "f1", "f2", "f3", "f4", "f5"]
    got = rollout.rollout_accuracy(model, x, steps=2, names=names)
    assert len(got) == 2
    cur = [x] * A
    with _Eval(model):
        for s in range(2):
            want = np.zeros((A, 3), dtype=np.int64)
            for a in range(A):
                action = _onehot(a, B, dev)
                out = model(cur[a], labels=None, mode=["action"] * B, action=action, input_y=cur[a])[0]
                res = model(x, labels=None, mode=["causal"] * B, action=action, input_y=out)
                call = R.hits_ref(res[0].cpu().numpy(), action.cpu().numpy())
                acc, nodir = float(res[4]["causal_acc"]), float(res[4]["causal_nodir_acc"])
                print(f"step {s} action {a}: causal_acc {acc} nodir {nodir} counts {call[a].tolist()}")
                assert call[a, 0] == B and call.sum() == call[a].sum()
                assert int(round(acc * B)) == call[a, 1] and int(round(nodir * B)) == call[a, 2]
                want += call
                cur[a] = out
            assert got[s] == rollout.summarize(want, names), s
            assert got[s]["n"] == [B] * A
    with pytest.raises(ValueError, match="names"):
        rollout.rollout_accuracy(model, x, names=["a"])


def test_split_accuracy_counts_the_causal_batches_only(model, dev):
    from ctvae_amd import rollout
    batches = []
    for i in range(6):
        bx, by, ba = filler.synthetic_pairs(300 + i, B, A)
        ba = ba[:, torch.randperm(A, generator=torch.Generator().manual_seed(i))]          # other actions than 0 .. B-1
        mode = ["base", "action", "causal"][i % 3]
        opts = {"mode": [mode] * B}
        if mode != "base":
            opts.update(input_y=by.to(dev), action=ba.to(dev))
        batches.append((bx.to(dev), torch.zeros(B, device=dev), opts))
    got = rollout.split_accuracy(model, iter(batches))
    assert sum(got["n"]) == 2 * B
    hits = np.zeros(2)
    want = np.zeros((A, 3), dtype=np.int64)
    with _Eval(model):
        for bx, lab, opts in batches:
            if opts["mode"][0] != "causal":
                continue
            res = model(bx, labels=lab, **opts)
            hits += [round(float(res[4]["causal_acc"]) * B), round(float(res[4]["causal_nodir_acc"]) * B)]
            want += R.hits_ref(res[0].cpu().numpy(), res[1].cpu().numpy())
    assert got == rollout.summarize(want)
    assert got["causal_acc"] == hits[0] / (2 * B) and got["causal_nodir_acc"] == hits[1] / (2 * B)      # the row-weighted mean
    none = rollout.split_accuracy(model, iter(batches[:2]))
    assert none["causal_acc"] is None and sum(none["n"]) == 0


def _png(path):
    with open(path, "rb") as f:
        img, kinds = G.read_png(f.read())
    assert kinds == ["IHDR", "IDAT", "IEND"]
    return img


def test_rollout_sheet_tiles_are_the_single_pictures(frames, tmp_path):
    from ctvae_amd import imagegrid, rollout
    path = tmp_path / "sheet.png"
    rollout.save_rollout_sheet(frames, str(path))
    sheet = _png(path)
    assert sheet.shape == (A * 66 + 2, 4 * 66 + 2, 3)
    for a in range(A):
        for s in range(4):
            alone = imagegrid.make_grid_u8(frames[s, a][None], normalize=True).cpu().numpy()       # what save_image writes
            assert alone.shape == (68, 68, 3)
            tile = sheet[a * 66 + 2:a * 66 + 66, s * 66 + 2:s * 66 + 66]
            assert np.array_equal(tile, alone[2:66, 2:66]), (a, s)
    imagegrid.save_image(frames[2, 7][None], str(tmp_path / "one.png"), normalize=True)
    assert np.array_equal(_png(tmp_path / "one.png")[2:66, 2:66], sheet[7 * 66 + 2:7 * 66 + 66, 2 * 66 + 2:2 * 66 + 66])
    border = np.ones(sheet.shape[:2], dtype=bool)
    for a in range(A):
        for s in range(4):
            border[a * 66 + 2:a * 66 + 66, s * 66 + 2:s * 66 + 66] = False
    assert (sheet[border] == 0).all()


def test_apply_action_command_end_to_end(dev, tmp_path):
    """Synthetic transition data (4 actions to keep it short), a checkpoint saved from the filler model, --steps 2: the three
    files, the JSON's keys, and a second run that writes the same bytes."""
    from ctvae_amd import apply_action
    from ctvae_amd.models import vae_models
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))
    cfg["model_params"]["action_dim"] = 4
    cfg["data_params"].update(val_batch_size=B, train_batch_size=B)
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    torch.manual_seed(9)
    m = vae_models["CTMCQVAE"](**dict(cfg["model_params"], hidden_dims=list(cfg["model_params"]["hidden_dims"])))
    m.load_state_dict(filler.fill_state(H.mcq_specs(H.CT_CONV_CFG), 10), strict=False)
    ckpt = tmp_path / "last.ckpt"
    torch.save({"state_dict": {"model." + k: v.detach().cpu().contiguous() for k, v in m.state_dict().items()}, "epoch": 0}, ckpt)
    cfg["trainer_params"]["resume_from_checkpoint"] = str(ckpt)
    cfg["data_params"]["hbm_factor_names"] = ["hue", "size"]
    path = tmp_path / "ct.yaml"
    path.write_text(yaml.safe_dump(cfg))
    files = ("rollout_input.png", "rollout_sheet.png", "action_accuracy.json")
    runs = []
    torch.manual_seed(123)
    before = (torch.get_rng_state(), torch.cuda.get_rng_state(dev))
    for out in (None, str(tmp_path / "again")):
        apply_action.main(["-c", str(path), "--steps", "2", "--image-index", "1"] + (["--out", out] if out else []))
        assert torch.equal(torch.get_rng_state(), before[0]) and torch.equal(torch.cuda.get_rng_state(dev), before[1])
        d = out or str(tmp_path / "logs" / "CTMCQVAE" / "apply_action")
        assert sorted(os.listdir(d)) == sorted(files)
        runs.append({f: open(os.path.join(d, f), "rb").read() for f in files})
    assert runs[0] == runs[1]
    assert _png(os.path.join(d, "rollout_input.png")).shape == (68, 68, 3)
    assert _png(os.path.join(d, "rollout_sheet.png")).shape == (4 * 66 + 2, 3 * 66 + 2, 3)
    res = json.loads(runs[0]["action_accuracy.json"])
    assert set(res) == {"rollout", "test_split"} and len(res["rollout"]) == 2
    keys = {f"{n}_{s}_{kind}" for n in ("hue", "size") for s in "+-" for kind in ("causal_acc", "causal_nodir_acc")}
    for part in res["rollout"] + [res["test_split"]]:
        assert set(part) == keys | {"causal_acc", "causal_nodir_acc", "n"}
    assert all(p["n"] == [B] * 4 for p in res["rollout"])
    assert sum(res["test_split"]["n"]) == 2 * B                     # 8 synthetic test batches: two of them causal
    with pytest.raises(SystemExit, match="3 names.*2 factors"):
        apply_action.main(["-c", str(path), "--factor-names", "a,b,c"])
