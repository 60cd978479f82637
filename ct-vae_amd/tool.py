"""The front end of the commands that work on a trained checkpoint (``apply_action``, ``causal_graph``, ``latent_stats``,
``recon_stats``, ``fit_prior``, ``log_likelihood``, ``fit_code_prior``): the arguments they share and the way from those to a model with its weights and its data.

A command's ``main`` reads, in this order: ``add_arguments`` and its own ``ap.add_argument`` lines; ``configure``, which reads the
YAML and refuses a model the command does not serve -- host only; the checks of its own flags; ``load``, which refuses a bad
checkpoint and a machine without a GPU, then builds the model, loads the weights strictly and chooses the data; its work; and
``os.makedirs(out_dir)`` behind the last refusal that precedes writing.  Bad input ends with ``SystemExit("<command>: <reason>")``.
The model is built under ``evalrun.seeded_torch_rng``: the caller's torch generators come back as they were.
"""
import os

import torch
import yaml

from .evalrun import seeded_torch_rng
from .models import vae_models
from .run import HbmData, SyntheticData, model_weights


def fail(command: str):
    """The command's refusal: ``fail("fit_prior")("no checkpoint")`` raises ``SystemExit("fit_prior: no checkpoint")``."""
    def _fail(msg: str):
        raise SystemExit(f"{command}: {msg}")
    return _fail


def add_arguments(ap, command: str, config: str) -> None:
    """``--config/-c`` (default: ``config``), ``--checkpoint``, ``--out`` and ``--ema``, in this order in front of the command's own."""
    ap.add_argument('--config', '-c', dest="filename", metavar='FILE', default=config)
    ap.add_argument('--checkpoint', default=None, help="default: trainer_params.resume_from_checkpoint")
    ap.add_argument('--out', default=None, help=f"default: <save_dir>/<name>/{command}")
    ap.add_argument('--ema', action='store_true', help="load the checkpoint's averaged weights (ema_state_dict) in place of state_dict")


def configure(args, command: str, accept) -> tuple:
    """Host only: the YAML of ``args`` and the class of ``model_params.name``.  ``accept(cls, name)`` (``cls`` is None for an unknown
    name) returns why the command does not serve the model, or None.  Returns ``(config, cls, mp, dp, tp, lp, ep)``: the model, data,
    trainer, logging and experiment parameters."""
    with open(args.filename) as f:
        config = yaml.safe_load(f)
    mp = dict(config['model_params'])
    cls = vae_models.get(mp.get('name'))
    why = accept(cls, mp.get('name'))
    if why is not None:
        fail(command)(why)
    tp, lp, ep = (config.get(k, {}) or {} for k in ('trainer_params', 'logging_params', 'exp_params'))
    return config, cls, mp, config.get('data_params', {}), tp, lp, ep


def load(args, command: str, configured: tuple) -> tuple:
    """``configure``'s result -> ``(model, data, dev, seed, out_dir)``: the model of ``model_params`` on the current device with the
    checkpoint's ``state_dict`` (``--ema``: ``ema_state_dict``) loaded strictly, ``run.py``'s own ``HbmData`` / ``SyntheticData`` choice
    seeded with ``exp_params.manual_seed``, and ``--out`` or ``<save_dir>/<name>/<command>``, which is not created here."""
    _, cls, mp, dp, tp, lp, ep = configured
    _fail = fail(command)
    ckpt_path = args.checkpoint or tp.get('resume_from_checkpoint')
    if not ckpt_path:
        _fail("no checkpoint: give --checkpoint or set trainer_params.resume_from_checkpoint")
    if not os.path.isfile(ckpt_path):
        _fail(f"checkpoint {ckpt_path} does not exist")
    ckpt = None
    if args.ema:          # (asked for by name: a checkpoint without the average is refused before anything is built)
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        if 'ema_state_dict' not in ckpt:
            _fail(f"--ema: checkpoint {ckpt_path} holds no ema_state_dict (it was written without exp_params.ema_decay)")
    if not torch.cuda.is_available():
        _fail("ctvae_amd runs on MI355X GPUs only: the hot path has no CPU fallback")

    dev = torch.device("cuda", torch.cuda.current_device())
    seed = int(ep.get('manual_seed', 0) or 0)
    with seeded_torch_rng(seed, dev):                     # the model's initial draws: the caller's generators come back
        model = cls(**mp).to(dev)
    if ckpt is None:
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    model.load_state_dict(model_weights(ckpt['ema_state_dict' if args.ema else 'state_dict']), strict=True)
    data = HbmData(dp, mp, dev, 0, 1, seed) if dp.get('hbm_images') else SyntheticData(dp, mp, dev, 0, 1, seed=seed)
    out_dir = args.out or os.path.join(lp.get('save_dir', 'logs/'), lp.get('name', mp['name']), command)
    return model, data, dev, seed, out_dir
