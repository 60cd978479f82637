"""The reference's ``apply_action.ipynb`` as a command: ``python -m ctvae_amd.apply_action -c configs/ct_mcq_vae.yaml``.

Builds the CT-MCQ-VAE of ``model_params``, loads a checkpoint the way ``run.py`` does (``model.`` prefix stripped, strict), takes
the first action-mode batch of the test split (``run.py``'s own ``HbmData`` / ``SyntheticData`` choice) and writes under ``--out``
(default ``<save_dir>/<name>/apply_action``):

* ``rollout_input.png``     the chosen test image
* ``rollout_sheet.png``     every action applied ``--steps`` times to it: a row per action, a column per step (rollout.py)
* ``action_accuracy.json``  ``{"rollout": [per step ...], "test_split": {...}}``: how often the causal mode recognises the
  applied action over that batch, and causal accuracy over the causal-mode batches of the test split, both by action

Factor names: ``--factor-names a,b,c``, else ``data_params.hbm_factor_names`` (a list of length action_dim / 2), else
``action<i>``.  Seeded with ``exp_params.manual_seed``; the torch generators come back as they were.  ``--ema`` loads the
checkpoint's averaged weights (``ema_state_dict``, written under ``exp_params.ema_decay``) in place of ``state_dict``; a checkpoint
without them is refused.  Checkpoint, model and data come through ``tool.py``, as for every checkpoint command.  Bad input ends with a
SystemExit that says why.
"""
import argparse
import json
import os

from . import imagegrid, rollout, tool
from .evalrun import batch_mode, unpack_batch
from .models.ct_mcq_vae import CTMCQVAE

_fail = tool.fail("apply_action")


def _accept(cls, name):
    if not (isinstance(cls, type) and issubclass(cls, CTMCQVAE)):
        return f"model_params.name is {name!r}: actions exist only in a CTMCQVAE"


def main(argv=None):
    ap = argparse.ArgumentParser(description="apply every action of a trained CT-MCQ-VAE and measure its causal accuracy")
    tool.add_arguments(ap, "apply_action", 'configs/ct_mcq_vae.yaml')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--image-index', type=int, default=0, help="row of the first action-mode test batch")
    ap.add_argument('--factor-names', default=None, help="comma-separated, action_dim / 2 of them")
    args = ap.parse_args(argv)
    configured = tool.configure(args, "apply_action", _accept)
    mp, dp = configured[2:4]
    try:
        names = rollout.configured_factor_names(mp, dp, args.factor_names)
    except ValueError as e:
        _fail(str(e))
    if args.steps < 1:
        _fail(f"--steps must be at least 1, got {args.steps}")
    model, data, dev, seed, out_dir = tool.load(args, "apply_action", configured)

    first = next((b for b in data.test() if batch_mode(unpack_batch(b)[2]) == "action"), None)
    if first is None:
        _fail("the test split has no action-mode batch")
    x = first[0]
    if not 0 <= args.image_index < x.size(0):
        _fail(f"--image-index {args.image_index} is outside the batch of {x.size(0)}")
    os.makedirs(out_dir, exist_ok=True)

    image = x[args.image_index:args.image_index + 1]
    imagegrid.save_image(image, os.path.join(out_dir, "rollout_input.png"), normalize=True)
    frames = rollout.action_rollout(model, image, steps=args.steps, seed=seed)
    rollout.save_rollout_sheet(frames, os.path.join(out_dir, "rollout_sheet.png"))
    res = {"rollout": rollout.rollout_accuracy(model, x, steps=args.steps, names=names, seed=seed),
           "test_split": rollout.split_accuracy(model, data.test(), names=names, seed=seed)}
    with open(os.path.join(out_dir, "action_accuracy.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return res


if __name__ == "__main__":
    main()
