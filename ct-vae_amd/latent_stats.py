"""The latent usage of a trained Gaussian model: ``python -m ctvae_amd.latent_stats -c configs/vae.yaml --checkpoint <path>``.

Builds the model of ``model_params`` and loads a checkpoint as every checkpoint command does (``tool.py``), runs the test split
through it (``latentstats.LatentStats`` on the ``mu`` / ``log_var`` of every batch) and writes under ``--out`` (default
``<save_dir>/<name>/latent_stats``):

* ``latent_stats.json``  the scalars of ``latentstats.summarize`` (``kl_total``, ``active_units``, ``collapsed``, ``mean_abs_corr``,
  ``gaussian_tc``, ``nonfinite``, ``rows``; the undefined ones are left out), ``kl``, the mean KL per dimension in nats, and
  ``ranked_dims``, every dimension by descending KL
* ``latent_stats.npz``   ``kl``, ``mu_mean``, ``mu_var``, ``sigma2_mean`` [L], ``cov`` [L, L] (float64) and ``rows``
* ``latent_corr.png``    |corr| of the posterior means, [0, 1] on ``causalgraph.colormap()``
* ``traversal.png``      ``--traverse K`` (default 10; 0: off) rows, the K highest-KL dimensions, and ``--steps S`` (default 11)
  columns, the dimension set to ``linspace(-span, span, S)`` (``--span``, default 3.0) while the others keep the posterior mean of
  test image ``--image-index`` (default 0)

The traversal needs a ``decode`` that takes [N, L] latents: the VanillaVAE family and BetaTCVAE.  For ConditionalVAE and JointVAE
it is refused by name -- after the statistics, which do not need it, are written.  Seeded with ``exp_params.manual_seed``; the
model runs in eval mode and the torch generators come back as they were.  ``--ema`` loads the checkpoint's averaged weights
(``ema_state_dict``) in place of ``state_dict``; a checkpoint without them is refused.  Bad input ends with a SystemExit that says
why.
"""
import argparse
import json
import os

import numpy as np

from . import latentstats, tool
from .evalrun import eval_mode, seeded_torch_rng, unpack_batch

FILES = ("latent_stats.json", "latent_stats.npz", "latent_corr.png", "traversal.png")
_fail = tool.fail("latent_stats")


def _accept(cls, name):
    if cls is None or not latentstats.has_gaussian_posterior(cls):
        return f"model_params.name is {name!r}: " + latentstats.needs_gaussian_posterior(cls, name=repr(name))


def main(argv=None):
    ap = argparse.ArgumentParser(description="per-dimension KL, active units, correlation and a traversal of a trained Gaussian model")
    tool.add_arguments(ap, "latent_stats", 'configs/vae.yaml')
    ap.add_argument('--traverse', type=int, default=10, metavar='K', help="rows of traversal.png: the K highest-KL dimensions (0: off)")
    ap.add_argument('--steps', type=int, default=11, metavar='S', help="columns of traversal.png")
    ap.add_argument('--span', type=float, default=3.0, help="the traversed dimension runs over linspace(-span, span, S)")
    ap.add_argument('--image-index', type=int, default=0, help="the test image whose posterior mean the traversal starts from")
    args = ap.parse_args(argv)
    configured = tool.configure(args, "latent_stats", _accept)
    if args.traverse < 0:
        _fail(f"--traverse must be at least 0, got {args.traverse}")
    if args.steps < 1:
        _fail(f"--steps must be at least 1, got {args.steps}")
    if not (args.span > 0 and args.span < float("inf")):
        _fail(f"--span must be a positive number, got {args.span}")
    if args.image_index < 0:
        _fail(f"--image-index must be at least 0, got {args.image_index}")
    model, data, dev, seed, out_dir = tool.load(args, "latent_stats", configured)
    mp = configured[2]

    stats = latentstats.LatentStats(model.latent_dim, dev)
    stats.zero()
    image, seen = None, 0
    with eval_mode(model), seeded_torch_rng(seed, dev):
        for batch in data.test():
            x, labels, opts = unpack_batch(batch, model)
            stats.observe(*model.gaussian_posterior(model(x, labels=labels, **opts)))
            if image is None and seen <= args.image_index < seen + x.size(0):
                image = x[args.image_index - seen].clone()
            seen += x.size(0)
    res = stats.result()
    if res["rows"] < 2:
        _fail(f"the test split has {res['rows']} rows: the statistics need at least two")
    os.makedirs(out_dir, exist_ok=True)

    ranked = latentstats.rank_dims(res["kl"], len(res["kl"]))
    summary = {**latentstats.record(res, prefix=""), "kl": [float(v) for v in res["kl"]], "ranked_dims": ranked}
    with open(os.path.join(out_dir, "latent_stats.json"), "w") as f:
        json.dump(summary, f, indent=1, allow_nan=not np.isfinite(res["kl"]).all())
        f.write("\n")
    latentstats.write_files(res, os.path.join(out_dir, "latent_stats.npz"), os.path.join(out_dir, "latent_corr.png"))

    if args.traverse > 0:
        if not latentstats.traversal_supported(model):
            _fail(f"--traverse: the decoder of {mp['name']} does not take [N, L] latents alone (the VanillaVAE family and BetaTCVAE "
                  f"do); the statistics are in {out_dir}, --traverse 0 ends without this message")
        if image is None:
            _fail(f"--image-index {args.image_index}: the test split has only {seen} images")
        dims = ranked[:args.traverse]
        values = np.linspace(-args.span, args.span, args.steps)
        latentstats.save_traversal(model, image, dims, values, os.path.join(out_dir, "traversal.png"))
        summary["traversal_dims"] = dims
    return summary


if __name__ == "__main__":
    main()
