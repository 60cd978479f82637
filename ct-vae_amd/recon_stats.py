"""The reconstruction quality of a trained model: ``python -m ctvae_amd.recon_stats -c configs/vae.yaml --checkpoint <path>``.

Builds the model of ``model_params`` and loads a checkpoint the way ``latent_stats.py`` does, runs the test split through it
(``reconstats.ReconStats`` on the pair ``BaseVAE.reconstruction_pair`` returns for every batch) and writes under ``--out``
(default ``<save_dir>/<name>/recon_stats``):

* ``recon_stats.json``  the scalars of ``reconstats.summarize``: ``psnr``, ``ssim``, ``mae``, ``max_err``, ``psnr_p05``, ``ssim_p05``,
  ``psnr_min``, ``ssim_min``, ``rows``, ``nonfinite``, ``exact`` (what has no image to stand on is left out)
* ``recon_stats.npz``   per image ``mse``, ``mae``, ``max_err``, ``ssim`` (float64), ``nonfinite`` and ``worst_rows``
* ``worst.png``         the ``--worst K`` (default ``exp_params.recon_stats_worst``, else 8; 0: no picture) worst targets by SSIM
  over their reconstructions, worst first

A CT-MCQ-VAE reports its base- and action-mode batches apart: the keys and the file stems carry ``_base`` / ``_action``, and
causal batches have no picture pair.  ``--range R`` is the data range of the pictures (default ``exp_params.recon_stats_range``,
else 1.0).  IWAE and MIWAE hand out several reconstructions per image and are refused by name.  Seeded with
``exp_params.manual_seed``; the model runs in eval mode and the torch generators come back as they were.  ``--ema`` loads the
checkpoint's averaged weights (``ema_state_dict``) in place of ``state_dict``; a checkpoint without them is refused.  Bad input
ends with a SystemExit that says why.
"""
import argparse
import json
import os

import torch
import yaml

FILES = ("recon_stats.json", "recon_stats.npz", "worst.png")


def _fail(msg: str):
    raise SystemExit(f"recon_stats: {msg}")


def collect(model, batches, R: float, K: int, seed: int = 0) -> dict:
    """{key suffix: ReconStats} over ``batches`` (``(x, labels[, options])``): ``""`` for every model but a CT-MCQ-VAE, whose
    base and action batches go to ``"_base"`` / ``"_action"``.  Eval mode and ``no_grad``; the model's BatchNorm statistics, its
    training flag, its parameters and torch's generators are left as found."""
    from . import reconstats
    from .experiment import seeded_torch_rng
    from .metrics import _eval_mode
    from .models.ct_mcq_vae import CTMCQVAE
    dev = next(model.parameters()).device
    suffixes = ("_base", "_action") if isinstance(model, CTMCQVAE) else ("",)
    stats = {sfx: reconstats.ReconStats(dev, R, K) for sfx in suffixes}
    for acc in stats.values():
        acc.reset()
    with _eval_mode(model), seeded_torch_rng(seed, dev), torch.no_grad():
        for batch in batches:
            x, labels, *rest = batch
            opts = rest[0] if rest and isinstance(rest[0], dict) else {}
            if getattr(model, 'uses_labels', False) and torch.is_tensor(labels) and labels.dim() == 1:
                labels = labels.reshape(-1, 1)            # one label per image is one class column
            results = model(x, labels=labels, **opts)
            pair = model.reconstruction_pair(results)
            if pair is not None:
                stats["" if "" in stats else "_" + results[4]["mode"]].observe(*pair)
    return stats


def main(argv=None):
    ap = argparse.ArgumentParser(description="PSNR, SSIM and the worst reconstructions of a trained model over the test split")
    ap.add_argument('--config', '-c', dest="filename", metavar='FILE', default='configs/vae.yaml')
    ap.add_argument('--checkpoint', default=None, help="default: trainer_params.resume_from_checkpoint")
    ap.add_argument('--out', default=None, help="default: <save_dir>/<name>/recon_stats")
    ap.add_argument('--ema', action='store_true', help="load the checkpoint's averaged weights (ema_state_dict) in place of state_dict")
    ap.add_argument('--worst', type=int, default=None, metavar='K', help="images of worst.png (0: off; default: recon_stats_worst, else 8)")
    ap.add_argument('--range', type=float, default=None, metavar='R', dest="data_range",
                    help="the data range of the pictures (default: recon_stats_range, else 1.0)")
    args = ap.parse_args(argv)
    with open(args.filename) as f:
        config = yaml.safe_load(f)

    from . import reconstats
    from .models import vae_models
    mp = dict(config['model_params'])
    cls = vae_models.get(mp.get('name'))
    if cls is None:
        _fail(f"model_params.name is {mp.get('name')!r}: not a model")
    why = reconstats.refuses_model(cls, name=repr(mp.get('name')))
    if why is not None:
        _fail(f"model_params.name: {why}")
    ep = config.get('exp_params', {}) or {}
    dp, tp, lp = config.get('data_params', {}), config.get('trainer_params', {}) or {}, config.get('logging_params', {}) or {}
    K = args.worst if args.worst is not None else ep.get('recon_stats_worst', reconstats.DEFAULT_WORST)
    R = args.data_range if args.data_range is not None else ep.get('recon_stats_range', reconstats.DEFAULT_RANGE)
    if isinstance(K, bool) or not isinstance(K, int) or not 0 <= K <= reconstats.MAX_WORST:
        _fail(f"--worst must be an integer, 0 <= K <= {reconstats.MAX_WORST}, got {K!r}")
    if isinstance(R, bool) or not isinstance(R, float) or not (R > 0 and R < float("inf")):
        _fail(f"--range must be a finite number > 0, got {R!r}")
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

    from .experiment import seeded_torch_rng
    from .run import HbmData, SyntheticData
    dev = torch.device("cuda", torch.cuda.current_device())
    seed = int(ep.get('manual_seed', 0) or 0)
    with seeded_torch_rng(seed, dev):                     # the model's initial draws: the caller's generators come back
        model = cls(**mp).to(dev)
    if ckpt is None:
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    weights = ckpt['ema_state_dict' if args.ema else 'state_dict']
    model.load_state_dict({k[6:]: v for k, v in weights.items() if k.startswith("model.")}, strict=True)
    data = HbmData(dp, mp, dev, 0, 1, seed) if dp.get('hbm_images') else SyntheticData(dp, mp, dev, 0, 1, seed=seed)

    stats = collect(model, data.test(), R, K, seed=seed)
    results = {sfx: acc.result() for sfx, acc in stats.items()}
    if not any(len(res["flags"]) for res in results.values()):
        _fail("the test split has no batch with a picture pair")
    out_dir = args.out or os.path.join(lp.get('save_dir', 'logs/'), lp.get('name', mp['name']), "recon_stats")
    os.makedirs(out_dir, exist_ok=True)
    summary = {}
    for sfx, res in results.items():
        summary.update(reconstats.record(reconstats.summarize(res["records"], res["flags"], R), prefix="", suffix=sfx))
        if len(res["flags"]):
            reconstats.write_files(res, os.path.join(out_dir, f"recon_stats{sfx}.npz"),
                                   os.path.join(out_dir, f"worst{sfx}.png") if K > 0 else None)
    with open(os.path.join(out_dir, "recon_stats.json"), "w") as f:
        json.dump(summary, f, indent=1, allow_nan=False)
        f.write("\n")
    return summary


if __name__ == "__main__":
    main()
