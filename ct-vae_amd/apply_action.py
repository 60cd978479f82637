"""The reference's ``apply_action.ipynb`` as a command: ``python -m ctvae_amd.apply_action -c configs/ct_mcq_vae.yaml``.

Builds the CT-MCQ-VAE of ``model_params``, loads a checkpoint the way ``run.py`` does (``model.`` prefix stripped, strict), takes
the first action-mode batch of the test split (``run.py``'s own ``HbmData`` / ``SyntheticData`` choice) and writes under ``--out``
(default ``<save_dir>/<name>/apply_action``):

* ``rollout_input.png``     the chosen test image
* ``rollout_sheet.png``     every action applied ``--steps`` times to it: a row per action, a column per step (rollout.py)
* ``action_accuracy.json``  ``{"rollout": [per step ...], "test_split": {...}}``: how often the causal mode recognises the
  applied action over that batch, and causal accuracy over the causal-mode batches of the test split, both by action

Factor names: ``--factor-names a,b,c``, else ``data_params.hbm_factor_names`` (a list of length action_dim / 2), else
``action<i>``.  Seeded with ``exp_params.manual_seed``.  ``--ema`` loads the checkpoint's averaged weights (``ema_state_dict``, written
under ``exp_params.ema_decay``) in place of ``state_dict``; a checkpoint without them is refused.  Bad input ends with a
SystemExit that says why.
"""
import argparse
import json
import os

import torch
import yaml


def _fail(msg: str):
    raise SystemExit(f"apply_action: {msg}")


def main(argv=None):
    ap = argparse.ArgumentParser(description="apply every action of a trained CT-MCQ-VAE and measure its causal accuracy")
    ap.add_argument('--config', '-c', dest="filename", metavar='FILE', default='configs/ct_mcq_vae.yaml')
    ap.add_argument('--checkpoint', default=None, help="default: trainer_params.resume_from_checkpoint")
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--image-index', type=int, default=0, help="row of the first action-mode test batch")
    ap.add_argument('--out', default=None, help="default: <save_dir>/<name>/apply_action")
    ap.add_argument('--factor-names', default=None, help="comma-separated, action_dim / 2 of them")
    ap.add_argument('--ema', action='store_true', help="load the checkpoint's averaged weights (ema_state_dict) in place of state_dict")
    args = ap.parse_args(argv)
    with open(args.filename) as f:
        config = yaml.safe_load(f)

    from .models import vae_models
    from .models.ct_mcq_vae import CTMCQVAE
    mp = dict(config['model_params'])
    cls = vae_models.get(mp.get('name'))
    if cls is None or not (isinstance(cls, type) and issubclass(cls, CTMCQVAE)):
        _fail(f"model_params.name is {mp.get('name')!r}: actions exist only in a CTMCQVAE")
    A = int(mp.get('action_dim', 0))
    if A < 2 or A % 2:
        _fail(f"model_params.action_dim must be even and at least 2, got {mp.get('action_dim')!r}")
    dp, tp, lp = config.get('data_params', {}), config.get('trainer_params', {}) or {}, config.get('logging_params', {}) or {}
    if args.factor_names is not None:
        names, src = [n.strip() for n in args.factor_names.split(",")], "--factor-names"
    else:
        names, src = dp.get('hbm_factor_names'), "data_params.hbm_factor_names"
    if names is not None and len(names) != A // 2:
        _fail(f"{src} has {len(names)} names, but action_dim {A} means {A // 2} factors")
    ckpt_path = args.checkpoint or tp.get('resume_from_checkpoint')
    if not ckpt_path:
        _fail("no checkpoint: give --checkpoint or set trainer_params.resume_from_checkpoint")
    if not os.path.isfile(ckpt_path):
        _fail(f"checkpoint {ckpt_path} does not exist")
    if args.steps < 1:
        _fail(f"--steps must be at least 1, got {args.steps}")
    ckpt = None
    if args.ema:          # (asked for by name: a checkpoint without the average is refused before anything is built)
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        if 'ema_state_dict' not in ckpt:
            _fail(f"--ema: checkpoint {ckpt_path} holds no ema_state_dict (it was written without exp_params.ema_decay)")
    if not torch.cuda.is_available():
        _fail("ctvae_amd runs on MI355X GPUs only: the hot path has no CPU fallback")

    from . import imagegrid, rollout
    from .run import HbmData, SyntheticData
    dev = torch.device("cuda", torch.cuda.current_device())
    seed = int(config.get('exp_params', {}).get('manual_seed', 0) or 0)
    torch.manual_seed(seed)
    model = cls(**mp).to(dev)
    if ckpt is None:
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    weights = ckpt['ema_state_dict' if args.ema else 'state_dict']
    model.load_state_dict({k[6:]: v for k, v in weights.items() if k.startswith("model.")}, strict=True)
    data = HbmData(dp, mp, dev, 0, 1, seed) if dp.get('hbm_images') else SyntheticData(dp, mp, dev, 0, 1, seed=seed)

    def mode_of(batch):
        m = batch[2].get("mode") if len(batch) > 2 and isinstance(batch[2], dict) else None
        return m[0] if isinstance(m, (list, tuple)) and m else m

    first = next((b for b in data.test() if mode_of(b) == "action"), None)
    if first is None:
        _fail("the test split has no action-mode batch")
    x = first[0]
    if not 0 <= args.image_index < x.size(0):
        _fail(f"--image-index {args.image_index} is outside the batch of {x.size(0)}")
    out_dir = args.out or os.path.join(lp.get('save_dir', 'logs/'), lp.get('name', mp['name']), "apply_action")
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
