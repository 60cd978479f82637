"""The marginal log-likelihood of held-out images by importance sampling (Burda et al. 2016, "Importance Weighted Autoencoders",
section 5; Wu et al. 2017): for z_k ~ q(z|x), k = 1..K,

    log p^(x) = logsumexp_k [ log p(x|z_k) + log p(z_k) - log q(z_k|x) ] - log K,

a lower bound on log p(x) in expectation that tightens with K; at K = 1 it is a one-sample ELBO.

The observation model is p(x|z) = N(decode(z), sigma^2 I), the model under which an MSE reconstruction term is a likelihood.  It
is the evaluation's own choice for every served model, those trained with another reconstruction term (LogCoshVAE, MSSIMVAE)
included: the numbers compare models under one yardstick, they are not the objective a model was trained on.  ``sigma`` is a
float > 0, or -- the command's ``--sigma mse`` -- the ELBO-optimal shared variance (Rybkin et al. 2021): sigma^2 = the mean squared
error per element of the posterior-mean reconstructions ``decode(mu)``, one scalar over ``rows * P`` elements, calibrated on the
evaluated rows themselves in a first pass (``SigmaFromMSE``).

* ``ImportanceLogLik`` -- per chunk of S samples: ``ctvae_loglik_latent`` (z and log p(z) - log q(z|x)), ``decode(z)``,
  ``ctvae_loglik_rows`` (the log-weights, float64), ``ctvae_loglik_merge`` (csrc/loglik.hip).  The per-image state lives on the
  device and grows by doubling; ``result()`` finishes it on the host in float64 from one copy.
* ``summarize`` / ``record`` / ``write_file`` -- the statistics, the epoch record's keys, the ``.npz``.
* ``loglik_setting`` / ``check_options`` / ``loglik_supported`` / ``needs_supported_model`` -- ``exp_params.val_loglik``, the command's
  flags and the models both are refused for.

There is no CPU path for the device parts.
"""
import math

import numpy as np
import torch

from . import kernels as K
from .evalrun import npz_bytes

LOGLIK_DIR = "Loglik"
LOGLIK_MODELS = ("VanillaVAE", "BetaVAE", "LogCoshVAE", "DIPVAE", "MSSIMVAE", "TwoStageVAE", "InfoVAE", "BetaTCVAE", "IWAE", "MIWAE")
MAX_SAMPLES = 65536                       # the command's --samples
SETTING_MAX_SAMPLES = 4096                # exp_params.val_loglik.samples: every validation epoch pays for it
DEFAULT_SAMPLES, DEFAULT_CHUNK = 512, 64
FIRST_CAPACITY = 1024
DECODE_ROWS = 256                         # a decoder pass takes the chunk of as many images as fit this many rows (one at least)
SETTING_FIELDS = ("samples", "sigma", "chunk")
RECORD_KEYS = (("loglik", "val_loglik"), ("elbo", "val_loglik_elbo"), ("gap", "val_loglik_gap"), ("ess_mean", "val_loglik_ess"),
               ("rows", "val_loglik_rows"), ("nonfinite", "val_loglik_nonfinite"))
_GPU_ONLY = "ImportanceLogLik runs on the GPU only: there is no CPU fallback"


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def check_options(samples, chunk, sigma, max_samples=MAX_SAMPLES, what="val_loglik.", allow_mse=False) -> tuple:
    """``(samples, chunk, sigma)`` after the checks the key and the command share: ``samples`` an int in 1..``max_samples``,
    ``chunk`` None (``min(samples, 64)``) or an int in 1..samples, ``sigma`` a finite float > 0 (or ``"mse"`` where allowed).  A
    ValueError names the field (``what`` goes in front of its name)."""
    if not _is_int(samples) or not 1 <= samples <= max_samples:
        raise ValueError(f"{what}samples must be an integer in 1..{max_samples}, got {samples!r}")
    if chunk is None:
        chunk = min(samples, DEFAULT_CHUNK)
    elif not _is_int(chunk) or not 1 <= chunk <= samples:
        raise ValueError(f"{what}chunk must be an integer in 1..samples (samples={samples}), got {chunk!r}")
    if sigma == "mse" and isinstance(sigma, str):
        if not allow_mse:
            raise ValueError(f"{what}sigma: mse needs a second pass over the rows and is python -m ctvae_amd.log_likelihood's alone; "
                             f"give a float > 0")
    elif isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not (sigma > 0 and math.isfinite(sigma)):
        raise ValueError(f"{what}sigma must be a float > 0{' or mse' if allow_mse else ''}, got {sigma!r}")
    else:
        sigma = float(sigma)
    return samples, chunk, sigma


def loglik_setting(value):
    """Validated ``exp_params.val_loglik``: None (absent: off) or a mapping with ``samples`` (an int, 1..4096, required), ``sigma`` (a
    float > 0, required; ``mse`` is refused by name) and the optional ``chunk`` (an int, 1..samples; default min(samples, 64)).
    Returns None or the complete dict; anything else is a ValueError that names the field."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError(f"val_loglik must be a mapping with samples and sigma, got {value!r}")
    extra = sorted(str(k) for k in value if k not in SETTING_FIELDS)
    if extra:
        raise ValueError(f"val_loglik has unknown field(s) {', '.join(extra)}; known: {', '.join(SETTING_FIELDS)}")
    for field in ("samples", "sigma"):
        if field not in value:
            raise ValueError(f"val_loglik.{field} is required")
    samples, chunk, sigma = check_options(value["samples"], value.get("chunk"), value["sigma"], SETTING_MAX_SAMPLES)
    return {"samples": samples, "sigma": sigma, "chunk": chunk}


def loglik_supported(model_or_class) -> bool:
    """Whether the model has a Gaussian posterior, the prior N(0, I) and a decoder that takes [n, latent_dim] alone:
    ``LOGLIK_MODELS`` by class (the aliases of VanillaVAE are that class)."""
    cls = model_or_class if isinstance(model_or_class, type) else type(model_or_class)
    return getattr(cls, "__name__", None) in LOGLIK_MODELS


def needs_supported_model(model_or_class, name=None) -> str:
    """The refusal of the estimate for any other model, by name."""
    cls = model_or_class if isinstance(model_or_class, type) else type(model_or_class)
    return (f"log_likelihood needs a model with a Gaussian posterior, a standard-normal prior and a decoder that takes "
            f"[n, latent_dim] latents alone ({', '.join(LOGLIK_MODELS)}), got "
            f"{name if name is not None else getattr(cls, '__name__', cls)}")


def decoder_of(model):
    """The model's decoder on rows, ``[R, latent_dim] -> [R, C, H, W]``: ``model.decode``, and for IWAE / MIWAE -- whose own decode
    takes [B, (M,) S, L] -- the base class's."""
    from .models.iwae import MIWAE
    from .models.vanilla_vae import VanillaVAE
    if isinstance(model, MIWAE):
        return lambda z: VanillaVAE.decode(model, z)
    return model.decode


def images_for(model, x):
    """The batch's images where the model already holds them in its decoder's memory format: the NCHW view of the NHWC tensor
    its encoder read (``_cached_nhwc``: no launch when ``x`` is the tensor the last forward saw), else ``x`` itself."""
    cached = getattr(model, "_cached_nhwc", None)
    return x if cached is None else K.to_nchw_view(cached(x))


def _in_format_of(x, xhat):
    """``x`` in a memory format ``xhat`` lies in: itself where the two share one, else ONE copy of the B images (against B * K
    decoded rows) -- made here, in the open; ``kernels.loglik_rows`` itself never copies."""
    fh = K.loglik_memory_formats(xhat)
    if not fh or set(fh) & set(K.loglik_memory_formats(x)):
        return x                          # (an xhat that is not dense is the wrapper's to refuse)
    return x.contiguous(memory_format=torch.channels_last if "nhwc" in fh else torch.contiguous_format)


def _images(what, x, P):
    if not torch.is_tensor(x) or x.dim() != 4 or x.dtype != torch.float32 or (x.size(0) and x[0].numel() != P):
        raise ValueError(f"{what}: x must be a torch.float32 [B, C, H, W] tensor of {P} elements per image, got "
                         f"{getattr(x, 'dtype', type(x).__name__)} {tuple(getattr(x, 'shape', ()))}")
    if not x.is_cuda:
        raise RuntimeError(_GPU_ONLY)
    return x.detach()


class SigmaFromMSE:
    """The first pass of ``sigma: mse``: the squared error of the posterior-mean reconstructions ``decode(mu)`` against the images,
    per image in float64 by the row kernel itself (``a = 0``, ``S = 1``, constants (1, 0): ``lw = -sse``), summed on the host from
    one copy."""

    def __init__(self, pixels: int, device):
        self.P, self.device = int(pixels), torch.device(device)
        self.parts = []
        self.consts = None

    def add_batch(self, x, mu, decode) -> None:
        x = _images("SigmaFromMSE.add_batch", x, self.P)
        with torch.cuda.device(self.device), torch.no_grad():
            if self.consts is None:
                self.consts = torch.tensor([1.0, 0.0], dtype=torch.float64, device=self.device)
            mu = mu.detach().to(torch.float32).contiguous()
            for b0 in range(0, x.size(0), DECODE_ROWS):          # the decoder's batch stays in the range training runs it at
                xhat = decode(mu[b0:b0 + DECODE_ROWS])
                if b0 == 0:
                    x = _in_format_of(x, xhat)
                self.parts.append(K.loglik_rows(xhat, x[b0:b0 + DECODE_ROWS], 1, None, self.consts))

    def sse(self) -> np.ndarray:
        """-lw = the per-image sums of squares, float64 on the host."""
        if not self.parts:
            return np.zeros(0, np.float64)
        return -torch.cat(self.parts).cpu().numpy()

    def sigma(self) -> float:
        """sqrt(sum sse / (rows * P)); a ValueError without rows, or when the mean squared error is not a finite number > 0."""
        sse = self.sse()
        mse = math.fsum(sse.tolist()) / (len(sse) * self.P) if len(sse) else float("nan")
        if not (mse > 0 and math.isfinite(mse)):
            raise ValueError(f"sigma: mse needs a finite mean squared error > 0 over the evaluated rows, got {mse!r} over {len(sse)} rows")
        return math.sqrt(mse)


class ImportanceLogLik:
    """The importance-sampling state of a stream of images, on the device (include/ctvae_hip.h: ``ctvae_loglik_latent`` /
    ``_rows`` / ``_merge``): per image (m, s, s2, t, n) in float64 and an int32 flag, grown by doubling."""

    def __init__(self, latent_dim: int, pixels: int, sigma: float, samples: int, chunk=None, device="cuda", capacity: int = FIRST_CAPACITY):
        if not _is_int(latent_dim) or latent_dim < 1 or (pixels is not None and (not _is_int(pixels) or pixels < 1)):
            raise ValueError(f"ImportanceLogLik: latent_dim and pixels must be integers of at least 1 (pixels None: the first batch's "
                             f"C * H * W), got {latent_dim!r}, {pixels!r}")
        self.samples, self.chunk, self.sigma = check_options(samples, chunk, sigma, what="ImportanceLogLik: ")
        self.L, self.P, self.device = latent_dim, pixels, torch.device(device)
        self._cap0 = max(int(capacity), 1)
        self.rows = 0                      # the host's count: every add_batch knows its B
        self.state = self.flags = self.consts = None       # made by the first use: constructing one touches no device

    def reset(self) -> None:
        """Back to no rows; the buffers are kept."""
        self.rows = 0

    def _reserve(self, n: int) -> None:
        """Room for n images, the rows behind ``self.rows`` empty: a new state and a copy of the old rows, in stream order."""
        cap = 0 if self.flags is None else self.flags.numel()
        if n > cap:
            new_cap = max(self._cap0, cap)
            while new_cap < n:
                new_cap *= 2
            state, flags = K.loglik_state(new_cap, self.device)
            if self.rows:
                state[:self.rows].copy_(self.state[:self.rows])
                flags[:self.rows].copy_(self.flags[:self.rows])
            self.state, self.flags = state, flags
        else:                              # rows a reset left behind
            self.state[self.rows:n, 0] = float("-inf")
            self.state[self.rows:n, 1:] = 0.0
            self.flags[self.rows:n] = 0

    def add_batch(self, x, mu, log_var, decode, generator=None) -> None:
        """The batch's images ``x`` [B, C, H, W] with their posteriors ``mu``, ``log_var`` [B, L] (fp32 device tensors), ``samples``
        draws each in chunks of ``chunk`` (the last may be short): ``eps = torch.randn((B, S, L), generator=generator)`` -- no
        other stream moves -- then latent, ``decode(z)`` ([R, L] -> [R, C, H, W]), rows and merge.  The decoder sees the chunk of
        as many images at a time as fit ``DECODE_ROWS`` rows (one image at least), so its batch stays in the range the
        training step runs it at whatever B * S is.  No host synchronisation."""
        what = "ImportanceLogLik.add_batch"
        if self.P is None and torch.is_tensor(x) and x.dim() == 4 and x.size(0):
            self.P = x[0].numel()
        x = _images(what, x, self.P)
        if self.device.type != "cuda":
            raise RuntimeError(_GPU_ONLY)
        for name, t in (("mu", mu), ("log_var", log_var)):
            if not torch.is_tensor(t) or t.dim() != 2 or tuple(t.shape) != (x.size(0), self.L) or t.dtype != torch.float32:
                raise ValueError(f"{what}: {name} must be a torch.float32 [{x.size(0)}, {self.L}] tensor, got "
                                 f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
        B = x.size(0)
        if B == 0:
            return
        with torch.cuda.device(self.device), torch.no_grad():
            if self.consts is None:
                self.consts = K.loglik_consts(self.sigma, self.P, self.device)
            self._reserve(self.rows + B)
            mu, log_var = mu.detach().contiguous(), log_var.detach().contiguous()
            done = 0
            while done < self.samples:
                S = min(self.chunk, self.samples - done)
                eps = torch.randn((B, S, self.L), generator=generator, device=self.device, dtype=torch.float32)
                z, a = K.loglik_latent(mu, log_var, eps)
                group = max(1, DECODE_ROWS // S)                 # images per decoder pass
                for b0 in range(0, B, group):
                    b1 = min(B, b0 + group)
                    xhat = decode(z[b0 * S:b1 * S])
                    if done == 0 and b0 == 0:
                        x = _in_format_of(x, xhat)
                    lw = K.loglik_rows(xhat, x[b0:b1], S, a[b0 * S:b1 * S], self.consts)
                    K.loglik_merge(lw, S, self.state, self.flags, self.rows + b0)
                done += S
        self.rows += B

    def result(self) -> dict:
        """The images on the host, by ONE device -> host copy, finished in float64: ``loglik`` = m + log s - log n, ``elbo`` =
        t / n, ``ess`` = s^2 / s2 (float64 [rows]) and ``nonfinite`` (int32 [rows]: a log-weight that was NaN or infinite; such an
        image's numbers are NaN), and the raw ``state`` [rows, 5]."""
        n = self.rows
        if n == 0:
            return finish(np.zeros((0, 5), np.float64), np.zeros(0, np.int32))
        host = torch.cat([self.state[:n].reshape(-1).view(torch.uint8), self.flags[:n].view(torch.uint8)]).cpu().numpy()
        return finish(host[:40 * n].view(np.float64).reshape(n, 5).copy(), host[40 * n:].view(np.int32).copy())


def finish(state, flags) -> dict:
    """The merge state as per-image numbers, float64 numpy, no GPU."""
    state = np.asarray(state, dtype=np.float64).reshape(-1, 5)
    flags = np.asarray(flags).reshape(-1)
    m, s, s2, t, n = (state[:, i] for i in range(5))
    bad = (flags != 0) | ~(n > 0)
    ok = ~bad
    loglik, elbo, ess = (np.full(len(flags), np.nan) for _ in range(3))
    loglik[ok] = m[ok] + np.log(s[ok]) - np.log(n[ok])
    elbo[ok] = t[ok] / n[ok]
    ess[ok] = s[ok] * s[ok] / s2[ok]
    return {"loglik": loglik, "elbo": elbo, "ess": ess, "nonfinite": bad.astype(np.int32), "state": state}


def summarize(result: dict, pixels: int) -> dict:
    """The images as statistics, no GPU.  Over the images whose flag is 0: ``loglik`` (mean nats per image), ``loglik_per_dim``
    (``loglik / P``), ``elbo``, ``gap`` (``loglik - elbo``, the estimate of KL(q || p(z|x)), >= 0), ``ess_mean``, ``ess_min``; and
    ``rows``, ``nonfinite``.  A statistic with no image to stand on is left out, never written as NaN."""
    bad = np.asarray(result["nonfinite"]).reshape(-1) != 0
    out = {"rows": int(len(bad)), "nonfinite": int(bad.sum())}
    if bad.all():
        return out
    ll, elbo, ess = (np.asarray(result[k], dtype=np.float64)[~bad] for k in ("loglik", "elbo", "ess"))
    mean = lambda v: math.fsum(v.tolist()) / len(v)
    out.update(loglik=mean(ll), loglik_per_dim=mean(ll) / int(pixels), elbo=mean(elbo), gap=mean(ll) - mean(elbo),
               ess_mean=mean(ess), ess_min=float(ess.min()))
    return out


def record(summary: dict) -> dict:
    """``summarize``'s scalars as the epoch record's keys (``RECORD_KEYS``); what is undefined is left out."""
    return {key: summary[k] for k, key in RECORD_KEYS if k in summary}


def file_arrays(result: dict) -> dict:
    return {"loglik": result["loglik"], "elbo": result["elbo"], "ess": result["ess"],
            "nonfinite": np.asarray(result["nonfinite"], dtype=np.int32)}


def write_file(result: dict, path) -> None:
    """Per image ``loglik``, ``elbo``, ``ess`` (float64) and ``nonfinite`` (int32) as an ``.npz`` whose bytes depend on the arrays
    alone."""
    with open(path, "wb") as f:
        f.write(npz_bytes(file_arrays(result)))
