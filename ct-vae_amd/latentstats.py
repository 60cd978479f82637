"""Latent usage of the Gaussian models: per-dimension KL, active units, the correlation of the posterior means, traversals.

The models with a Gaussian posterior fail by posterior collapse: a latent dimension falls back to the prior, its KL goes to 0
and its mean stops moving with the data -- which neither the ``KLD`` scalar nor the disentanglement metrics show.  Everything
needed is on the device in every validation step, ``mu`` and ``log_var`` [B, L] (``BaseVAE.gaussian_posterior``):

* ``LatentStats`` -- float64 sums of the per-element KL, of mu, of sigma^2 and of mu mu^T, int32 counts of non-finite elements
  and of the rows, on the device (csrc/latentstat.hip: ``ctvae_latent_accumulate``, one launch per batch, no host
  synchronisation).  Every accumulator element is the sum of its rows in ascending order, so a result does not depend on the
  batch size.
* ``summarize`` -- the accumulators as statistics, float64 numpy on the host.
* ``rank_dims`` / ``traversal_latents`` / ``save_traversal`` -- the standard latent traversal picture: one row per chosen
  dimension, the dimension swept over ``values`` while the others keep the posterior mean of one image.
* ``latent_stats_setting`` / ``needs_gaussian_posterior`` -- ``exp_params.latent_stats`` and the models it is refused for.

There is no CPU path for the device parts.
"""
import numpy as np
import torch

from . import imagegrid
from . import kernels as K
from .causalgraph import save_heatmaps
from .evalrun import eval_mode, npz_bytes, seeded_torch_rng

ACTIVE_VAR = 0.01            # a unit is active when the variance of its posterior mean over the data exceeds it (Burda et al. 2016)
COLLAPSED_KL = 0.01          # a dimension counts as collapsed below this mean KL, in nats
DECODE_ROWS = 256            # save_traversal: latent rows per decode call
LATENT_DIR = "Latents"
STATE_KEYS = tuple(name for name, _, _ in K.LATENT_STATE)
GAUSSIAN_MODELS = ("VanillaVAE", "BetaVAE", "LogCoshVAE", "DIPVAE", "MSSIMVAE", "TwoStageVAE", "VampVAE", "IWAE", "MIWAE", "InfoVAE",
                   "JointVAE", "BetaTCVAE", "ConditionalVAE")
RECORD_KEYS = ("kl_total", "active_units", "collapsed", "mean_abs_corr", "gaussian_tc", "nonfinite", "rows")


def latent_stats_setting(value) -> bool:
    """Validated ``exp_params.latent_stats``: a bool (absent: False); anything else is a ValueError that names the key."""
    if value is None:
        return False
    if not isinstance(value, bool):
        raise ValueError(f"latent_stats must be true or false, got {value!r}")
    return value


def has_gaussian_posterior(model_or_class) -> bool:
    """Whether the model overrides ``BaseVAE.gaussian_posterior`` (the default returns None)."""
    from .models.base import BaseVAE
    cls = model_or_class if isinstance(model_or_class, type) else type(model_or_class)
    return getattr(cls, "gaussian_posterior", None) is not BaseVAE.gaussian_posterior


def needs_gaussian_posterior(model_or_class, name=None) -> str:
    """The refusal of ``latent_stats`` for a model without a Gaussian posterior, by name."""
    cls = model_or_class if isinstance(model_or_class, type) else type(model_or_class)
    return (f"latent_stats needs a model with a Gaussian posterior ({', '.join(GAUSSIAN_MODELS)}), got "
            f"{name if name is not None else cls.__name__}")


class LatentStats:
    """The accumulators of ``ctvae_latent_accumulate`` for L latent dimensions (include/ctvae_hip.h), in one device buffer."""

    def __init__(self, L: int, device):
        self.L = int(L)
        if not 1 <= self.L <= K.LATENT_MAX_L:
            raise ValueError(f"LatentStats covers 1 <= latent_dim <= {K.LATENT_MAX_L}, got {L}")
        self.device = torch.device(device)
        self._buf = self._views = None          # made by the first use: constructing one touches no device

    def _layout(self):
        """Word offsets in the one int32 buffer: the float64 parts first (8-byte aligned), then the counts."""
        L = self.L
        off, lay = 0, {}
        for name, n in (("kl_sum", 2 * L), ("mu_sum", 2 * L), ("sig2_sum", 2 * L), ("cov_sum", 2 * L * L), ("nonfinite", L), ("rows", 1)):
            lay[name] = (off, n)
            off += n
        return lay, off

    def _state(self) -> dict:
        if self._views is None:
            if self.device.type != "cuda":
                raise RuntimeError("LatentStats runs on the GPU only: there is no CPU fallback")
            lay, words = self._layout()
            self._buf = torch.zeros(words, dtype=torch.int32, device=self.device)
            views = {}
            for name, dtype, rank in K.LATENT_STATE:
                off, n = lay[name]
                v = self._buf[off:off + n]
                if dtype == torch.float64:
                    v = v.view(torch.float64)
                views[name] = v.view(self.L, self.L) if rank == 2 else v
            self._views = views
        return self._views

    def zero(self) -> None:
        self._state()
        self._buf.zero_()

    def observe(self, mu: torch.Tensor, log_var: torch.Tensor) -> None:
        """Add the rows of mu, log_var [B, L]: one launch, no host synchronisation (``kernels.latent_accumulate``)."""
        if mu.dim() != 2 or mu.size(1) != self.L:
            raise ValueError(f"LatentStats.observe takes mu, log_var [B, {self.L}], got {tuple(mu.shape)}")
        with torch.cuda.device(self.device):
            K.latent_accumulate(mu, log_var, self._state())

    def state(self) -> dict:
        """Host copies of the accumulators (one device -> host copy): ``kl_sum``, ``mu_sum``, ``sig2_sum`` float64 [L],
        ``cov_sum`` float64 [L, L], ``nonfinite`` int32 [L], ``rows`` int32 [1]."""
        self._state()
        host = self._buf.cpu().numpy()
        lay = self._layout()[0]
        out = {}
        for name, dtype, rank in K.LATENT_STATE:
            off, n = lay[name]
            v = host[off:off + n]
            if dtype == torch.float64:
                v = v.view(np.float64)
            out[name] = (v.reshape(self.L, self.L) if rank == 2 else v).copy()
        return out

    def result(self) -> dict:
        return summarize(self.state())


def summarize(state: dict) -> dict:
    """The accumulators as statistics, float64 numpy, no GPU.  With n = rows:

    * ``kl`` [L] = kl_sum / n, the mean KL per dimension in nats; ``kl_total`` their sum; ``collapsed`` = #(kl < 0.01)
    * ``mu_mean``, ``sigma2_mean`` [L]
    * ``cov`` [L, L] = (cov_sum - n mu_mean mu_mean^T) / (n - 1), the unbiased covariance of the posterior means (``np.cov``);
      ``mu_var`` = its diagonal; ``active_units`` = #(mu_var > 0.01) (Burda et al. 2016)
    * ``corr`` [L, L], zero rows and columns where mu_var <= 0; ``mean_abs_corr``, the mean of |corr| off the diagonal over the
      active dimensions
    * ``gaussian_tc`` = 0.5 (sum log diag(cov_a) - log det cov_a) over the ACTIVE dimensions only: the total correlation of a
      Gaussian with that covariance.  disentanglement_lib's ``gaussian_total_correlation`` takes all dimensions, which one
      collapsed dimension (variance 0) makes singular; here it does not enter
    * ``nonfinite``, the total count of non-finite posterior parameters; ``rows``

    With n < 2 only the KL entries (and ``nonfinite``, ``rows``) are produced, with n = 0 only the two counts; with fewer than
    two active dimensions ``mean_abs_corr`` and ``gaussian_tc`` are left out, and ``gaussian_tc`` also where the covariance of the
    active dimensions is singular -- n rows give it rank n - 1 at most, so it needs more rows than active dimensions."""
    n = int(np.asarray(state["rows"]).reshape(-1)[0])
    out = {"rows": n, "nonfinite": int(np.asarray(state["nonfinite"], dtype=np.int64).sum())}
    if n < 1:
        return out
    kl = np.asarray(state["kl_sum"], dtype=np.float64) / n
    out.update(kl=kl, kl_total=float(kl.sum()), collapsed=int((kl < COLLAPSED_KL).sum()))
    if n < 2:
        return out
    mu_mean = np.asarray(state["mu_sum"], dtype=np.float64) / n
    cov = (np.asarray(state["cov_sum"], dtype=np.float64) - n * np.outer(mu_mean, mu_mean)) / (n - 1)
    mu_var = np.diag(cov).copy()
    active = mu_var > ACTIVE_VAR
    with np.errstate(invalid="ignore", divide="ignore"):
        sd = np.sqrt(np.where(mu_var > 0, mu_var, 1.0))
        corr = cov / np.outer(sd, sd)
    live = mu_var > 0
    corr = np.where(np.outer(live, live), corr, 0.0)
    out.update(mu_mean=mu_mean, sigma2_mean=np.asarray(state["sig2_sum"], dtype=np.float64) / n, cov=cov, mu_var=mu_var,
               active_units=int(active.sum()), corr=corr)
    a = int(active.sum())
    if a >= 2:
        ca = cov[np.ix_(active, active)]
        ra = np.abs(corr[np.ix_(active, active)])
        out["mean_abs_corr"] = float((ra.sum() - np.trace(ra)) / (a * (a - 1)))
        if n > a:                    # (a sample covariance of n rows has rank n - 1 at most)
            sign, logdet = np.linalg.slogdet(ca)
            if sign > 0:
                out["gaussian_tc"] = float(0.5 * (np.log(np.diag(ca)).sum() - logdet))
    return out


def record(result: dict, prefix: str = "val_latent_") -> dict:
    """The scalars of ``summarize`` as log entries; the undefined ones are left out."""
    return {prefix + k: result[k] for k in RECORD_KEYS if k in result}


def rank_dims(kl, k: int) -> list:
    """The ``k`` dimensions with the largest KL, descending; ties go to the lower index."""
    kl = np.asarray(kl, dtype=np.float64).reshape(-1)
    return [int(i) for i in np.argsort(-kl, kind="stable")[:max(int(k), 0)]]


def traversal_latents(mu_row, dims, values) -> torch.Tensor:
    """[len(dims) * len(values), L]: row (r, s) is ``mu_row`` with element ``dims[r]`` replaced by ``values[s]``.  On
    ``mu_row``'s device and of its dtype."""
    mu_row = torch.as_tensor(mu_row).detach().reshape(-1)
    L = mu_row.numel()
    dims = [int(d) for d in dims]
    if any(d < 0 or d >= L for d in dims):
        raise ValueError(f"traversal_latents: dims must lie in [0, {L}), got {dims}")
    vals = torch.as_tensor(values, dtype=mu_row.dtype).reshape(-1).to(mu_row.device)
    R, S = len(dims), vals.numel()
    out = mu_row.reshape(1, 1, L).repeat(R, S, 1)
    for r, d in enumerate(dims):
        out[r, :, d] = vals
    return out.reshape(R * S, L)


def traversal_supported(model) -> bool:
    """A traversal decodes [N, L] latents: the VanillaVAE family and BetaTCVAE.  ConditionalVAE's decoder also takes the label
    and JointVAE's the categorical code."""
    from .models import BetaTCVAE, VanillaVAE
    return isinstance(model, (VanillaVAE, BetaTCVAE))


def save_traversal(model, x_row, dims, values, path) -> tuple:
    """The traversal picture of one image: ``x_row`` [C, H, W] (or [1, C, H, W]) is encoded, its posterior mean goes through
    ``traversal_latents`` and the rows are decoded, at most ``DECODE_ROWS`` per ``decode`` call, into one sheet with a row per
    dimension (``imagegrid.save_image(normalize=True, nrow=len(values))``).  Eval mode and ``no_grad``: BatchNorm statistics and
    training flags stay as found, and so does every random stream.  Returns the sheet's (rows, columns)."""
    if not traversal_supported(model):
        raise TypeError(f"save_traversal needs a model whose decode takes [N, L] latents (the VanillaVAE family, BetaTCVAE), got "
                        f"{type(model).__name__}")
    if not torch.is_tensor(x_row) or not x_row.is_cuda:
        raise RuntimeError("save_traversal runs on the GPU only: there is no CPU fallback")
    x = x_row if x_row.dim() == 4 else x_row.unsqueeze(0)
    if x.dim() != 4 or x.size(0) != 1:
        raise ValueError(f"save_traversal takes one image [C, H, W], got {tuple(x_row.shape)}")
    dims, values = list(dims), [float(v) for v in values]
    if not dims or not values:
        raise ValueError("save_traversal needs at least one dimension and one value")
    with eval_mode(model), seeded_torch_rng(0, x.device):
        mu = model.encode(x)[0].reshape(-1)
        z = traversal_latents(mu, dims, values)
        imgs = torch.cat([model.decode(z[i:i + DECODE_ROWS].contiguous()) for i in range(0, z.size(0), DECODE_ROWS)])
        imgs = imgs.reshape((z.size(0),) + tuple(imgs.shape[-3:]))
        imagegrid.save_image(imgs, path, normalize=True, nrow=len(values))
    return len(dims), len(values)


def write_files(result: dict, npz_path, png_path) -> None:
    """``summarize``'s arrays as an ``.npz`` (``kl``, ``mu_mean``, ``mu_var``, ``sigma2_mean``, ``cov``, ``rows``; bytes that
    depend on the arrays alone) and |corr| as a heat map over [0, 1].  Needs n >= 2 rows."""
    arrays = {k: result[k] for k in ("kl", "mu_mean", "mu_var", "sigma2_mean", "cov")}
    arrays["rows"] = np.asarray([result["rows"]], dtype=np.int64)
    with open(npz_path, "wb") as f:
        f.write(npz_bytes(arrays))
    L = result["corr"].shape[0]
    save_heatmaps(np.abs(result["corr"]).astype(np.float32).reshape(1, L, L), png_path, cell=max(1, min(16, 512 // L)))
