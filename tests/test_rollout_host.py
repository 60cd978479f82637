"""CPU: the host half of ctvae_amd/rollout.py and apply_action.py (counts -> result dict, names, refusals) and the self-checks of
the restatements the GPU tests compare against (tests/rollout_checks.py)."""
import os

import numpy as np
import pytest
import torch
import yaml

from tests import grid_checks as G
from tests import rollout_checks as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
CRAFTED = {                      # row -> torch.argmax, checked on the CPU
    "tie: the first maximum": ([1.0, 3.0, 3.0, 0.0], 1),
    "NaN is maximal, the first NaN": ([NAN, 5.0, NAN, 1.0], 0),
    "NaN beats +inf": ([INF, 1.0, INF, NAN], 3),
    "all -inf": ([-INF, -INF, -INF, -INF], 0),
    "all equal": ([0.25, 0.25, 0.25, 0.25], 0),
    "+inf twice": ([0.0, INF, INF, -INF], 1),
    "NaN later": ([2.0, 7.0, NAN, 9.0], 2),
}


@pytest.mark.parametrize("name", list(CRAFTED))
def test_argmax_restatement_on_crafted_rows(name):
    row, want = CRAFTED[name]
    assert int(torch.argmax(torch.tensor(row))) == want
    assert R.argmax_ref(np.array(row, dtype=np.float32)) == want


def test_argmax_restatement_on_random_rows():
    """1000 rows of 12 from a few values (many ties) with NaN and infinities sprinkled in."""
    rng = np.random.default_rng(7)
    rows = rng.choice(np.array([-INF, -1.0, 0.0, 0.5, 0.5, 2.0, INF, NAN], dtype=np.float32), size=(1000, 12),
                      p=[0.05, 0.2, 0.2, 0.2, 0.15, 0.1, 0.05, 0.05])
    want = torch.argmax(torch.from_numpy(rows), dim=-1).numpy()
    got = np.array([R.argmax_ref(r) for r in rows])
    assert np.array_equal(got, want)
    assert np.isnan(rows).any(axis=1).sum() > 100 and (~np.isnan(rows).any(axis=1)).sum() > 100


def test_hits_restatement_counts():
    """A = 4 (V = 2): p = a, p = a + V (direction-agnostic only), a plain miss, and a soft action row."""
    action = np.array([[1, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1], [0.1, 0.2, 0.6, 0.1]], dtype=np.float32)
    probas = np.array([[.7, .1, .1, .1], [.1, .1, .7, .1], [.7, .1, .1, .1], [.1, .1, .1, .7]], dtype=np.float32)
    assert R.hits_ref(probas, action).tolist() == [[2, 1, 2], [0, 0, 0], [1, 0, 0], [1, 0, 0]]


def test_summarize_names_signs_and_totals():
    from ctvae_amd import rollout
    counts = np.array([[4, 2, 3], [0, 0, 0], [5, 5, 5], [8, 1, 2], [2, 0, 2], [1, 1, 1]])
    res = rollout.summarize(counts, ["hue", "size", "angle"])
    acc = [k for k in res if k.endswith("_causal_acc")]
    assert acc == ["hue_+_causal_acc", "size_+_causal_acc", "angle_+_causal_acc",
                   "hue_-_causal_acc", "size_-_causal_acc", "angle_-_causal_acc"]          # index i: factor i % V, "+" for i < V
    assert [k for k in res if k.endswith("_causal_nodir_acc") and k != "causal_nodir_acc"] == [k.replace("_acc", "_nodir_acc") for k in acc]
    assert res["n"] == [4, 0, 5, 8, 2, 1] and sum(res["n"]) == 20
    assert res["causal_acc"] == 9 / 20 and res["causal_nodir_acc"] == 13 / 20             # totals = sums of the per-action counts
    assert res["hue_+_causal_acc"] == 0.5 and res["hue_+_causal_nodir_acc"] == 0.75
    assert res["hue_-_causal_acc"] == 1 / 8 and res["angle_-_causal_nodir_acc"] == 1.0
    assert res["size_+_causal_acc"] is None and res["size_+_causal_nodir_acc"] is None    # never occurred: None, not NaN
    import json
    json.loads(json.dumps(res, allow_nan=False))
    assert rollout.summarize(counts)["action1_-_causal_acc"] == 0.0
    empty = rollout.summarize(np.zeros((6, 3), dtype=np.int64))
    assert empty["causal_acc"] is None and empty["causal_nodir_acc"] is None
    for bad in (["a", "b"], ["a", "b", "c", "d"], []):
        with pytest.raises(ValueError, match="names"):
            rollout.summarize(counts, bad)
    with pytest.raises(ValueError, match=r"\[A, 3\]"):
        rollout.summarize(np.zeros((5, 3)))


def test_grid_each_restatement_of_one_image_is_the_batch_restatement():
    x = G.grid_inputs(21, (1, 3, 5, 7))
    for scan in (False, True):
        assert np.array_equal(R.grid_each_ref(x, nrow=8, padding=2, scanlines=scan),
                              G.ref_grid_bytes(x, nrow=8, padding=2, normalize=True, scanlines=scan))
    # ... and of several it is not: the second image of a batch reaches 0 and 255 on its own range only
    y = R.each_inputs(22, (4, 3, 4, 4))
    each = R.grid_each_ref(y, nrow=2, padding=1).reshape(11, 11, 3)
    assert each[6:10, 6:10].min() == 0 and each[6:10, 6:10].max() == 255          # image 3: its own lo and hi
    assert (each[1:5, 6:10] == 0).all() and (each[6:10, 1:5] == 0).all()          # the constant image, the all-NaN image
    assert int((each[1:5, 1:5] == 0).sum()) >= 5                                  # image 0's NaN pixels


def test_no_cpu_path():
    from ctvae_amd import imagegrid, rollout
    from ctvae_amd.models import vae_models
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rollout.ActionHits(12, "cuda").update(torch.zeros(3, 12), torch.zeros(3, 12))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imagegrid.make_grid_u8(torch.zeros(2, 3, 4, 4), normalize=True, scale_each=True)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
    model = vae_models["CTMCQVAE"](**cfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rollout.action_rollout(model, torch.zeros(3, 64, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rollout.rollout_accuracy(model, torch.zeros(2, 3, 64, 64))
    vanilla = vae_models["VanillaVAE"](in_channels=3, latent_dim=16)
    for fn, arg in ((rollout.action_rollout, torch.zeros(3, 64, 64)), (rollout.rollout_accuracy, torch.zeros(2, 3, 64, 64)),
                    (rollout.split_accuracy, [])):
        with pytest.raises(TypeError, match="VanillaVAE"):
            fn(vanilla, arg)


def _config(tmp_path, name, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["trainer_params"].update(trainer)
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_command_refuses_with_a_reason(tmp_path):
    from ctvae_amd import apply_action
    with pytest.raises(SystemExit, match="VanillaVAE.*CTMCQVAE"):
        apply_action.main(["-c", _config(tmp_path, "vae.yaml")])
    with pytest.raises(SystemExit, match="no checkpoint"):
        apply_action.main(["-c", _config(tmp_path, "ct_mcq_vae.yaml")])
    missing = str(tmp_path / "missing.ckpt")
    with pytest.raises(SystemExit, match="missing.ckpt does not exist"):
        apply_action.main(["-c", _config(tmp_path, "ct_mcq_vae.yaml"), "--checkpoint", missing])
    with pytest.raises(SystemExit, match="missing.ckpt does not exist"):
        apply_action.main(["-c", _config(tmp_path, "ct_mcq_vae.yaml", resume_from_checkpoint=missing)])
    with pytest.raises(SystemExit, match="2 names.*6 factors"):
        apply_action.main(["-c", _config(tmp_path, "ct_mcq_vae.yaml"), "--checkpoint", missing, "--factor-names", "a,b"])
    assert not os.path.exists(tmp_path / "logs")                    # nothing was written
