"""Fit an interpolated Markov prior to the code grids of a trained quantising model and sample from it:
``python -m ctvae_amd.fit_code_prior -c configs/mcq_vae.yaml --checkpoint <path>``.

Builds the model of ``model_params`` and loads a checkpoint as every checkpoint command does (``tool.py``), encodes the training
split to index grids (``model.vq_layer.compute_inds(model.encode(x)[0])``; ``--rows N`` caps the rows; default all), counts the rows
with an even ordinal into ``codeprior.MarkovCodePrior``, fits the interpolation weights on the rows with an odd ordinal
(``--em-iters 20``, ``--uniform-floor 1e-3``), scores the test split and writes under ``--out`` (default
``<save_dir>/<name>/fit_code_prior``):

* ``code_prior.npz``          int64 ``pos``, ``left``, ``up``, ``prev``, float64 ``lambda``, and ``K``, ``C``, ``H``, ``W``, ``rows``, ``em_iters``,
  ``uniform_floor`` (``MarkovCodePrior.load`` reads it)
* ``code_prior.json``         ``train`` (the held-out odd rows the weights were fitted on) and ``test``: ``nats_per_code``,
  ``bits_per_code``, ``uniform_nats`` = ln K, ``per_codebook``, ``rows``, ``bad``; the ``weights``, ``rows`` (counted), ``invalid`` and the
  arguments.  The test split's number is the clean one: no statistic has seen those rows.
* ``samples_code_prior.png``  ``--samples`` (default 32) decoded ancestral draws from the prior
* ``samples_noise.png``       ``MCQVAE`` only: the model's own ``sample()`` -- quantised noise -- for comparison

Models other than ``codeprior.CODE_PRIOR_MODELS`` are refused by name before a device is touched.  Seeded with
``exp_params.manual_seed``; the model runs in eval mode and the torch generators come back as they were.  ``--ema`` loads the
checkpoint's averaged weights (``ema_state_dict``) in place of ``state_dict``; a checkpoint without them is refused.  Bad input
ends with a SystemExit that says why.
"""
import argparse
import json
import os

import torch

from . import codeprior, imagegrid, tool
from .evalrun import eval_mode, seeded_torch_rng, unpack_batch

FILES = ("code_prior.npz", "code_prior.json", "samples_code_prior.png")
NOISE_FILE = "samples_noise.png"
_fail = tool.fail("fit_code_prior")


def _accept(cls, name):
    if cls is None or not codeprior.prior_supported(cls):
        return f"model_params.name is {name!r}: " + codeprior.needs_supported_model(cls, name=repr(name))


def _encode(model, batches, cap):
    """The index grids of ``batches`` [rows, C, H, W] on the device, at most ``cap`` rows (None: all)."""
    buf = codeprior.CodeGridBuffer(next(model.parameters()).device)
    for batch in batches:
        x, _, _ = unpack_batch(batch, model)
        inds = codeprior.grid_indices(model, x)
        buf.append(inds if cap is None else inds[:cap - buf.rows])
        if cap is not None and buf.rows >= cap:
            break
    return buf.view()


def main(argv=None):
    ap = argparse.ArgumentParser(description="fit an interpolated Markov prior to the code grids of a trained quantising model; sample from it")
    tool.add_arguments(ap, "fit_code_prior", 'configs/mcq_vae.yaml')
    ap.add_argument('--em-iters', type=int, default=20, help="rounds of deleted interpolation")
    ap.add_argument('--uniform-floor', type=float, default=1e-3, help="the weight the uniform expert keeps, inside (0, 1)")
    ap.add_argument('--rows', type=int, default=None, metavar='N', help="a cap on the training rows encoded (default: all)")
    ap.add_argument('--samples', type=int, default=32, help="images per sample sheet")
    args = ap.parse_args(argv)
    configured = tool.configure(args, "fit_code_prior", _accept)
    try:
        codeprior.check_options(args.em_iters, args.uniform_floor, what="--")
    except ValueError as e:
        _fail(str(e))
    if args.rows is not None and args.rows < 2:
        _fail(f"--rows must be at least 2, got {args.rows}")
    if args.samples < 1:
        _fail(f"--samples must be at least 1, got {args.samples}")
    model, data, dev, seed, out_dir = tool.load(args, "fit_code_prior", configured)

    gen = torch.Generator(device=dev)                  # what the sample sheet draws from: no other stream moves
    gen.manual_seed(seed)
    with eval_mode(model), seeded_torch_rng(seed, dev):
        train = _encode(model, data.train(), args.rows)
        if train.size(0) < 2:
            _fail(f"the training split gave {train.size(0)} rows, a code prior needs at least 2")
        _, C, H, W = train.shape
        try:
            prior = codeprior.MarkovCodePrior(int(model.num_embeddings), C, H, W, dev)
            fit = codeprior.fit_halves(prior, train, args.em_iters, args.uniform_floor)
        except ValueError as e:
            _fail(str(e))
        test = _encode(model, data.test(), None)
        summary = {"fit": fit, "train": prior.summary(train[1::2].contiguous())}
        if test.size(0):
            summary["test"] = prior.summary(test)
        for split in ("train", "test"):
            if split in summary:
                del summary[split]["weights"]
        os.makedirs(out_dir, exist_ok=True)
        inds = prior.sample(args.samples, gen)
        imagegrid.save_image(prior.decode_samples(model, inds), os.path.join(out_dir, "samples_code_prior.png"), normalize=True,
                             nrow=12)
        if type(model).__name__ == "MCQVAE":
            imagegrid.save_image(model.sample(args.samples, dev), os.path.join(out_dir, NOISE_FILE), normalize=True, nrow=12)
    summary["weights"] = [[float(v) for v in row] for row in prior.weights]
    summary["experts"] = list(codeprior.EXPERTS)
    summary["rows"], summary["invalid"] = prior.rows, prior.invalid
    summary["arguments"] = {k: v for k, v in vars(args).items() if k != "filename"}
    summary["arguments"]["config"] = args.filename
    prior.save(os.path.join(out_dir, "code_prior.npz"))
    with open(os.path.join(out_dir, "code_prior.json"), "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    return summary


if __name__ == "__main__":
    main()
