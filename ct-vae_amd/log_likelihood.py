"""Estimate the test log-likelihood of a trained Gaussian model by importance sampling (the IWAE bound, Burda et al. 2016):
``python -m ctvae_amd.log_likelihood -c configs/vae.yaml --checkpoint <path>``.

Builds the model of ``model_params`` and loads a checkpoint as every checkpoint command does (``tool.py``), walks the test split
(``--rows N`` caps the rows; default all) and feeds ``loglik.ImportanceLogLik`` (csrc/loglik.hip) ``--samples K`` (an int,
1 <= K <= 65536, default 512) draws z ~ q(z|x) per image in chunks of ``--chunk S`` (1 <= S <= K, default min(K, 64)): one decoder
pass of ``batch * S`` rows per chunk.  The observation model is N(decode(z), sigma^2 I) for every served model, whatever
reconstruction term it was trained with; ``--sigma`` is a float > 0 or ``mse`` (the default): sigma^2 = the mean squared error per
element of the posterior-mean reconstructions ``decode(mu)`` over the rows evaluated, found in a first pass over the same rows
(so it is calibrated on the rows it then scores) and recorded.  Writes under ``--out`` (default
``<save_dir>/<name>/log_likelihood``):

* ``log_likelihood.json``  ``loglik`` (mean nats per image), ``loglik_per_dim``, ``elbo``, ``gap`` (``loglik - elbo``), ``ess_mean``,
  ``ess_min`` -- over the images without a non-finite log-weight; a statistic with no image to stand on is left out -- ``rows``,
  ``nonfinite``, ``sigma``, ``sigma_source`` (``given`` or ``mse``), ``samples``, ``chunk`` and the arguments
* ``log_likelihood.npz``   per image ``loglik``, ``elbo``, ``ess`` (float64) and ``nonfinite`` (int32)

Models other than ``loglik.LOGLIK_MODELS`` are refused by name before a device is touched, and so is a flag that is not a number
of the kind asked for or lies out of range.  Seeded with ``exp_params.manual_seed``; the model runs in eval mode (BatchNorm uses
its running statistics: a row does not depend on its batch), the noise comes from a generator of the command's own and the torch
generators come back as they were.  ``--ema`` loads the checkpoint's averaged weights.  Bad input ends with a SystemExit that says why.
"""
import argparse
import json
import os

import torch

from . import loglik, tool
from .evalrun import eval_mode, seeded_torch_rng, unpack_batch

FILES = ("log_likelihood.json", "log_likelihood.npz")
_fail = tool.fail("log_likelihood")


def _accept(cls, name):
    if cls is None or not loglik.loglik_supported(cls):
        return f"model_params.name is {name!r}: " + loglik.needs_supported_model(cls, name=repr(name))


def _int(flag, v, lo, hi=None):
    """An int flag as the command line hands it over (text) or as a caller does (a number): a bool, a float or text that is no
    integer is refused like a value out of range, by the flag's name."""
    span = f"an integer in {lo}..{hi}" if hi is not None else f"an integer of at least {lo}"
    if isinstance(v, str):
        try:
            v = int(v.strip())
        except ValueError:
            _fail(f"{flag} must be {span}, got {v!r}")
    if isinstance(v, bool) or not isinstance(v, int) or v < lo or (hi is not None and v > hi):
        _fail(f"{flag} must be {span}, got {v!r}")
    return v


def _sigma(v):
    if isinstance(v, str) and v.strip() != "mse":
        try:
            v = float(v.strip())
        except ValueError:
            _fail(f"--sigma must be a float > 0 or mse, got {v!r}")
    try:
        return loglik.check_options(1, None, v.strip() if isinstance(v, str) else v, what="--", allow_mse=True)[2]
    except ValueError as e:
        _fail(str(e))


def check_flags(samples, chunk, sigma, rows) -> tuple:
    """``(samples, chunk, sigma, rows)`` validated, host only; a SystemExit names the flag."""
    samples = _int("--samples", samples, 1, loglik.MAX_SAMPLES)
    chunk = min(samples, loglik.DEFAULT_CHUNK) if chunk is None else _int("--chunk", chunk, 1, samples)
    return samples, chunk, _sigma(sigma), (None if rows is None else _int("--rows", rows, 1))


def _batches(model, data, cap):
    """(x, mu, log_var) of the test split's batches, at most ``cap`` rows (None: all)."""
    seen = 0
    for batch in data.test():
        x, _labels, _opts = unpack_batch(batch, model)             # the label column: no model of LOGLIK_MODELS uses labels
        mu, log_var = model.encode(x)[:2]
        x = loglik.images_for(model, x)
        if cap is not None:
            x, mu, log_var = x[:cap - seen], mu[:cap - seen], log_var[:cap - seen]
        yield x, mu, log_var
        seen += x.size(0)
        if cap is not None and seen >= cap:
            return


def main(argv=None):
    ap = argparse.ArgumentParser(description="estimate the test log-likelihood of a trained Gaussian model by importance sampling")
    tool.add_arguments(ap, "log_likelihood", 'configs/vae.yaml')
    ap.add_argument('--samples', default=loglik.DEFAULT_SAMPLES, metavar='K', help="importance samples per image, 1..65536")
    ap.add_argument('--chunk', default=None, metavar='S', help="samples per decoder pass, 1..K (default: min(K, 64))")
    ap.add_argument('--sigma', default="mse", help="the observation model's sigma: a float > 0, or mse (calibrated on the rows evaluated)")
    ap.add_argument('--rows', default=None, metavar='N', help="a cap on the test rows evaluated (default: all)")
    args = ap.parse_args(argv)
    configured = tool.configure(args, "log_likelihood", _accept)
    samples, chunk, sigma, cap = check_flags(args.samples, args.chunk, args.sigma, args.rows)
    model, data, dev, seed, out_dir = tool.load(args, "log_likelihood", configured)

    gen = torch.Generator(device=dev)                  # what the importance samples draw from: no other stream moves
    gen.manual_seed(seed)
    decode = loglik.decoder_of(model)
    P = None
    with eval_mode(model), seeded_torch_rng(seed, dev):
        source = "given"
        if sigma == "mse":
            source, first = "mse", None
            for x, mu, _ in _batches(model, data, cap):
                if first is None:
                    first = loglik.SigmaFromMSE(x[0].numel(), dev)
                first.add_batch(x, mu, decode)
            try:
                if first is None:
                    raise ValueError("the test split has no rows")
                sigma = first.sigma()
            except ValueError as e:
                _fail(str(e))
        acc = None
        for x, mu, log_var in _batches(model, data, cap):
            if acc is None:
                P = x[0].numel()
                acc = loglik.ImportanceLogLik(model.latent_dim, P, sigma, samples, chunk, dev)
            acc.add_batch(x, mu, log_var, decode, gen)
        if acc is None:
            _fail("the test split has no rows")
        result = acc.result()
    summary = loglik.summarize(result, P)
    summary.update(sigma=sigma, sigma_source=source, samples=samples, chunk=chunk)
    summary["arguments"] = {k: v for k, v in vars(args).items() if k != "filename"}
    summary["arguments"]["config"] = args.filename
    os.makedirs(out_dir, exist_ok=True)
    loglik.write_file(result, os.path.join(out_dir, "log_likelihood.npz"))
    with open(os.path.join(out_dir, "log_likelihood.json"), "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
    return summary


if __name__ == "__main__":
    main()
