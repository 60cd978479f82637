"""Fit a Gaussian-mixture latent prior to a trained Gaussian model and sample from it:
``python -m ctvae_amd.fit_prior -c configs/vae.yaml --checkpoint <path>``.

Builds the model of ``model_params`` and loads a checkpoint as every checkpoint command does (``tool.py``), encodes the
training split (``--rows N`` caps the rows; default all), fits ``latentprior.GaussianMixturePrior`` (``--components 10``,
``--covariance full|diag``, ``--max-iter 100``, ``--tol 1e-3``, ``--reg-covar 1e-6``; ``--codes mean`` fits on the posterior means, ``--codes sample`` on
``mu + exp(0.5 log_var) * eps`` with eps from a generator of its own) and writes under ``--out`` (default
``<save_dir>/<name>/fit_prior``):

* ``latent_prior.npz``      float64 ``weights``, ``means``, ``covariances``, and ``covariance_type``, ``reg_covar``, ``rows``,
  ``iterations``, ``converged`` (``GaussianMixturePrior.load`` reads it)
* ``latent_prior.json``     the ``fit`` dict (``iterations``, ``converged``, ``loglik_trace``, ``rows``, ``nonfinite``),
  ``train_loglik_mixture`` / ``train_loglik_standard`` and ``test_loglik_mixture`` / ``test_loglik_standard`` -- the mean
  log-likelihood, in nats, of the split's finite rows under the mixture and under N(0, I); a statistic with no row to stand on is
  left out -- the ``weights`` and the arguments
* ``samples_standard.png``  ``--samples`` (default 32) decoded draws eps ~ N(0, I)
* ``samples_mixture.png``   the same eps through the mixture, ``mu_k + L_k eps``

Models other than ``latentprior.PRIOR_MODELS`` are refused by name before a device is touched.  Seeded with
``exp_params.manual_seed``; the model runs in eval mode and the torch generators come back as they were.  ``--ema`` loads the
checkpoint's averaged weights (``ema_state_dict``) in place of ``state_dict``; a checkpoint without them is refused.  Bad input
ends with a SystemExit that says why.
"""
import argparse
import json
import os

import torch

from . import imagegrid, latentprior, tool
from .evalrun import eval_mode, seeded_torch_rng, unpack_batch

FILES = ("latent_prior.npz", "latent_prior.json", "samples_standard.png", "samples_mixture.png")
_fail = tool.fail("fit_prior")


def _accept(cls, name):
    if cls is None or not latentprior.prior_supported(cls):
        return f"model_params.name is {name!r}: " + latentprior.needs_supported_model(cls, name=repr(name))


def _encode(model, batches, codes, generator, cap):
    """The codes of ``batches`` [rows, latent_dim] on the device, at most ``cap`` rows (None: all)."""
    buf = latentprior.CodeBuffer(model.latent_dim, next(model.parameters()).device)
    for batch in batches:
        x, labels, opts = unpack_batch(batch, model)           # the label column: a no-op, no model of PRIOR_MODELS uses labels
        z = latentprior.draw_codes(*model.gaussian_posterior(model(x, labels=labels, **opts)), codes, generator)
        buf.append(z if cap is None else z[:cap - buf.rows])
        if cap is not None and buf.rows >= cap:
            break
    return buf.view()


def main(argv=None):
    ap = argparse.ArgumentParser(description="fit a Gaussian-mixture prior to the latent codes of a trained Gaussian model; sample from it")
    tool.add_arguments(ap, "fit_prior", 'configs/vae.yaml')
    ap.add_argument('--components', type=int, default=10, metavar='K', help="mixture components, 1..64")
    ap.add_argument('--covariance', default="full", help="full or diag")
    ap.add_argument('--max-iter', type=int, default=100)
    ap.add_argument('--tol', type=float, default=1e-3, help="stop when the mean log-likelihood moves by less")
    ap.add_argument('--reg-covar', type=float, default=1e-6, help="added to the diagonal of every covariance")
    ap.add_argument('--codes', default="mean", help="mean: the posterior means; sample: draws from the posteriors")
    ap.add_argument('--rows', type=int, default=None, metavar='N', help="a cap on the training rows encoded (default: all)")
    ap.add_argument('--samples', type=int, default=32, help="images per sample sheet")
    args = ap.parse_args(argv)
    configured = tool.configure(args, "fit_prior", _accept)
    try:
        latentprior.check_options(args.components, args.covariance, args.max_iter, args.tol, args.reg_covar, args.codes, what="--")
    except ValueError as e:
        _fail(str(e))
    if args.rows is not None and args.rows < 2:
        _fail(f"--rows must be at least 2, got {args.rows}")
    if args.samples < 1:
        _fail(f"--samples must be at least 1, got {args.samples}")
    model, data, dev, seed, out_dir = tool.load(args, "fit_prior", configured)

    gen = torch.Generator(device=dev)                  # what --codes sample and the sample sheets draw from: no other stream moves
    gen.manual_seed(seed)
    prior = latentprior.GaussianMixturePrior(model.latent_dim, args.components, args.covariance, args.reg_covar, dev)
    with eval_mode(model), seeded_torch_rng(seed, dev):
        train = _encode(model, data.train(), args.codes, gen, args.rows)
        try:
            fit = prior.fit(train, seed=seed, max_iter=args.max_iter, tol=args.tol)
        except ValueError as e:
            _fail(str(e))
        test = _encode(model, data.test(), args.codes, gen, None)
        summary = {"fit": fit}
        for split, rows in (("train", train), ("test", test)):
            if rows.size(0) == 0:
                continue
            mix = prior.mean_over_finite(*prior.log_prob(rows))
            if mix is not None:
                summary[f"{split}_loglik_mixture"] = mix
                summary[f"{split}_loglik_standard"] = prior.mean_over_finite(*prior.standard_log_prob(rows))
        eps = torch.randn(args.samples, model.latent_dim, generator=gen, device=dev)
        u = torch.rand(args.samples, generator=gen, device=dev)
        z, _ = prior.sample(args.samples, u=u, eps=eps)
        os.makedirs(out_dir, exist_ok=True)
        imagegrid.save_image(model.decode(eps), os.path.join(out_dir, "samples_standard.png"), normalize=True, nrow=12)
        imagegrid.save_image(model.decode(z), os.path.join(out_dir, "samples_mixture.png"), normalize=True, nrow=12)
    summary["weights"] = [float(w) for w in prior.weights]
    summary["arguments"] = {k: v for k, v in vars(args).items() if k != "filename"}
    summary["arguments"]["config"] = args.filename
    prior.save(os.path.join(out_dir, "latent_prior.npz"))
    with open(os.path.join(out_dir, "latent_prior.json"), "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    return summary


if __name__ == "__main__":
    main()
