"""The reconstruction quality of a trained model: ``python -m ctvae_amd.recon_stats -c configs/vae.yaml --checkpoint <path>``.

Builds the model of ``model_params`` and loads a checkpoint as every checkpoint command does (``tool.py``), runs the test split
through it (``reconstats.ReconStats`` on the pair ``BaseVAE.reconstruction_pair`` returns for every batch) and writes under ``--out``
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

from . import reconstats, tool
from .evalrun import eval_mode, seeded_torch_rng, unpack_batch
from .models.ct_mcq_vae import CTMCQVAE

FILES = ("recon_stats.json", "recon_stats.npz", "worst.png")
_fail = tool.fail("recon_stats")


def _accept(cls, name):
    if cls is None:
        return f"model_params.name is {name!r}: not a model"
    why = reconstats.refuses_model(cls, name=repr(name))
    return None if why is None else f"model_params.name: {why}"


def collect(model, batches, R: float, K: int, seed: int = 0) -> dict:
    """{key suffix: ReconStats} over ``batches`` (``(x, labels[, options])``): ``""`` for every model but a CT-MCQ-VAE, whose
    base and action batches go to ``"_base"`` / ``"_action"``.  Eval mode and ``no_grad``; the model's BatchNorm statistics, its
    training flag, its parameters and torch's generators are left as found."""
    dev = next(model.parameters()).device
    suffixes = ("_base", "_action") if isinstance(model, CTMCQVAE) else ("",)
    stats = {sfx: reconstats.ReconStats(dev, R, K) for sfx in suffixes}
    for acc in stats.values():
        acc.reset()
    with eval_mode(model), seeded_torch_rng(seed, dev), torch.no_grad():
        for batch in batches:
            x, labels, opts = unpack_batch(batch, model)
            results = model(x, labels=labels, **opts)
            pair = model.reconstruction_pair(results)
            if pair is not None:
                stats["" if "" in stats else "_" + results[4]["mode"]].observe(*pair)
    return stats


def main(argv=None):
    ap = argparse.ArgumentParser(description="PSNR, SSIM and the worst reconstructions of a trained model over the test split")
    tool.add_arguments(ap, "recon_stats", 'configs/vae.yaml')
    ap.add_argument('--worst', type=int, default=None, metavar='K', help="images of worst.png (0: off; default: recon_stats_worst, else 8)")
    ap.add_argument('--range', type=float, default=None, metavar='R', dest="data_range",
                    help="the data range of the pictures (default: recon_stats_range, else 1.0)")
    args = ap.parse_args(argv)
    configured = tool.configure(args, "recon_stats", _accept)
    ep = configured[6]
    K = args.worst if args.worst is not None else ep.get('recon_stats_worst', reconstats.DEFAULT_WORST)
    R = args.data_range if args.data_range is not None else ep.get('recon_stats_range', reconstats.DEFAULT_RANGE)
    if isinstance(K, bool) or not isinstance(K, int) or not 0 <= K <= reconstats.MAX_WORST:
        _fail(f"--worst must be an integer, 0 <= K <= {reconstats.MAX_WORST}, got {K!r}")
    if isinstance(R, bool) or not isinstance(R, float) or not (R > 0 and R < float("inf")):
        _fail(f"--range must be a finite number > 0, got {R!r}")
    model, data, dev, seed, out_dir = tool.load(args, "recon_stats", configured)

    stats = collect(model, data.test(), R, K, seed=seed)
    results = {sfx: acc.result() for sfx, acc in stats.items()}
    if not any(len(res["flags"]) for res in results.values()):
        _fail("the test split has no batch with a picture pair")
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
