"""A Gaussian-mixture latent prior fitted after training, and samples from it (Ghosh et al. 2020, "From Variational to Deterministic
Autoencoders", section 4: ex-post density estimation).

A Gaussian VAE trained with a small ``kld_weight`` has an aggregate posterior q(z) = 1/N sum_i q(z|x_i) far from N(0, I): prior
samples land where the decoder was never trained.  The remedy is to fit a mixture to the latent codes and to sample from that:

* ``GaussianMixturePrior`` -- EM on the device (csrc/gmm.hip: ``ctvae_gmm_estep`` / ``ctvae_gmm_mstep``, two GEMM-shaped passes per
  iteration over an [N, D] matrix that never leaves the device), the K Cholesky factorisations in float64 on the host
  (``torch.linalg``), scikit-learn's ``GaussianMixture`` rules for ``reg_covar``, the ``10 * eps`` on the component masses and the
  stopping test; ``log_prob``, ``standard_log_prob`` (the same rows under N(0, I)), ``sample`` (``ctvae_gmm_sample``), ``save`` /
  ``load``.
* ``prior_setting`` / ``prior_supported`` / ``needs_supported_model`` -- ``exp_params.sample_prior`` and the models it is refused for.
* ``CodeBuffer`` -- the validation codes of an epoch in one device buffer that grows by doubling.

There is no CPU path for the device parts.
"""
import math

import numpy as np
import torch

from . import kernels as K
from .evalrun import npz_bytes

PRIOR_DIR = "Priors"
PRIOR_MODELS = ("VanillaVAE", "BetaVAE", "LogCoshVAE", "DIPVAE", "MSSIMVAE", "TwoStageVAE", "InfoVAE", "VampVAE", "BetaTCVAE")
COVARIANCES = ("full", "diag")
CODES = ("mean", "sample")
SETTING_DEFAULTS = {"components": 10, "covariance": "full", "max_iter": 50, "tol": 1e-3, "reg_covar": 1e-6, "codes": "mean"}
RECORD_PREFIX = "val_prior_"
_EPS10 = 10 * np.finfo(np.float64).eps          # scikit-learn's guard on the component masses
_LOG_2PI = math.log(2.0 * math.pi)


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _is_real(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def check_options(components, covariance, max_iter, tol, reg_covar, codes="mean", what="sample_prior.") -> None:
    """The ranges every entry to the mixture shares; a ValueError names the field (``what`` goes in front of its name; "--":
    as a command-line option)."""
    def nm(field):
        return what + (field.replace("_", "-") if what == "--" else field)
    if not _is_int(components) or not 1 <= components <= K.GMM_MAX_K:
        raise ValueError(f"{nm('components')} must be an integer in 1..{K.GMM_MAX_K}, got {components!r}")
    if covariance not in COVARIANCES:
        raise ValueError(f"{nm('covariance')} must be one of {', '.join(COVARIANCES)}, got {covariance!r}")
    if not _is_int(max_iter) or max_iter < 1:
        raise ValueError(f"{nm('max_iter')} must be an integer of at least 1, got {max_iter!r}")
    if not _is_real(tol) or tol < 0:
        raise ValueError(f"{nm('tol')} must be a number of at least 0, got {tol!r}")
    if not _is_real(reg_covar) or not reg_covar > 0:
        raise ValueError(f"{nm('reg_covar')} must be a positive number, got {reg_covar!r}")
    if codes not in CODES:
        raise ValueError(f"{nm('codes')} must be one of {', '.join(CODES)}, got {codes!r}")


def prior_setting(value):
    """Validated ``exp_params.sample_prior``: None (absent: off) or a mapping with ``type: gmm`` and the optional ``components``
    (1..64, default 10), ``covariance`` (full | diag), ``max_iter`` (>= 1, default 50), ``tol`` (>= 0, default 1e-3), ``reg_covar``
    (> 0, default 1e-6), ``codes`` (mean | sample).  Returns None or the complete dict; anything else is a ValueError that names
    the field."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError(f"sample_prior must be a mapping with type: gmm, got {value!r}")
    if value.get("type") != "gmm":
        raise ValueError(f"sample_prior.type must be gmm, got {value.get('type')!r}")
    extra = sorted(str(k) for k in value if k != "type" and k not in SETTING_DEFAULTS)
    if extra:
        raise ValueError(f"sample_prior has unknown field(s) {', '.join(extra)}; known: type, {', '.join(SETTING_DEFAULTS)}")
    out = {"type": "gmm", **SETTING_DEFAULTS, **{k: v for k, v in value.items() if k != "type"}}
    check_options(out["components"], out["covariance"], out["max_iter"], out["tol"], out["reg_covar"], out["codes"])
    out["tol"], out["reg_covar"] = float(out["tol"]), float(out["reg_covar"])
    return out


def prior_supported(model_or_class) -> bool:
    """Whether the model has a Gaussian posterior and a ``sample()`` that is ``decode(randn(n, latent_dim))`` with a decoder that
    takes [n, latent_dim] alone: ``PRIOR_MODELS`` by class (the aliases of VanillaVAE are that class)."""
    cls = model_or_class if isinstance(model_or_class, type) else type(model_or_class)
    return cls.__name__ in PRIOR_MODELS


def needs_supported_model(model_or_class, name=None) -> str:
    """The refusal of ``sample_prior`` for any other model, by name."""
    cls = model_or_class if isinstance(model_or_class, type) else type(model_or_class)
    return (f"sample_prior needs a model with a Gaussian posterior whose decoder takes [n, latent_dim] latents alone "
            f"({', '.join(PRIOR_MODELS)}), got {name if name is not None else getattr(cls, '__name__', cls)}")


def draw_codes(mu: torch.Tensor, log_var: torch.Tensor, codes: str, generator=None) -> torch.Tensor:
    """The rows the mixture is fitted on: ``mu`` for ``codes: mean``, ``mu + exp(0.5 log_var) * eps`` for ``codes: sample`` with eps
    from ``generator`` (a generator of the prior's own, so that no other random stream moves)."""
    if codes == "mean":
        return mu.detach()
    eps = torch.randn(mu.shape, generator=generator, device=mu.device, dtype=mu.dtype)
    return mu.detach() + torch.exp(0.5 * log_var.detach()) * eps


def finish_mstep(Nk, S1, S2, m, full: bool, reg_covar: float):
    """The host's end of an M step, float64 torch on the CPU: from ``ctvae_gmm_mstep``'s sums centred at ``m`` [K, D] (the fp32
    means the kernel saw, as float64) to ``(weights, means, covariances)``.  nk = Nk + 10 eps (scikit-learn's guard), weights =
    nk / sum nk (which is Nk / N_finite up to that guard, and sums to 1), means = m + S1 / nk, covariances = S2 / nk -
    (means - m)(means - m)^T + reg_covar I."""
    Nk, S1, S2, m = (torch.as_tensor(t, dtype=torch.float64).cpu() for t in (Nk, S1, S2, m))
    Kc, D = m.shape
    nk = Nk + _EPS10
    d = S1 / nk.reshape(Kc, 1)
    if full:
        cov = S2 / nk.reshape(Kc, 1, 1) - d.unsqueeze(2) * d.unsqueeze(1) + reg_covar * torch.eye(D, dtype=torch.float64)
    else:
        cov = S2 / nk.reshape(Kc, 1) - d * d + reg_covar
    return nk / nk.sum(), m + d, cov


class CodeBuffer:
    """[rows, D] fp32 on the device, appended to batch by batch; the capacity doubles when a batch does not fit."""

    def __init__(self, D: int, device, capacity: int = 1024):
        self.D, self.device, self.rows = int(D), torch.device(device), 0
        self._cap0 = max(int(capacity), 1)
        self._buf = None

    def append(self, codes: torch.Tensor) -> None:
        if codes.dim() != 2 or codes.size(1) != self.D:
            raise ValueError(f"CodeBuffer.append takes codes [B, {self.D}], got {tuple(codes.shape)}")
        B = codes.size(0)
        if self._buf is None:
            self._buf = torch.empty(max(self._cap0, B), self.D, dtype=torch.float32, device=self.device)
        if self.rows + B > self._buf.size(0):
            cap = self._buf.size(0)
            while cap < self.rows + B:
                cap *= 2
            grown = torch.empty(cap, self.D, dtype=torch.float32, device=self.device)
            grown[:self.rows].copy_(self._buf[:self.rows])
            self._buf = grown
        self._buf[self.rows:self.rows + B].copy_(codes.detach())
        self.rows += B

    def clear(self) -> None:
        self.rows = 0

    def view(self) -> torch.Tensor:
        if self._buf is None:
            return torch.empty(0, self.D, dtype=torch.float32, device=self.device)
        return self._buf[:self.rows]


class GaussianMixturePrior:
    """K Gaussians over D latent dimensions.  The parameters live on the host in float64 (``weights`` [K], ``means`` [K, D],
    ``covariances`` [K, D, D], or [K, D] for ``diag``); the kernels see fp32 copies prepared by ``_prepare``."""

    def __init__(self, D: int, K_: int, covariance: str = "full", reg_covar: float = 1e-6, device="cuda"):
        if not _is_int(D) or not 1 <= D <= K.GMM_MAX_D:
            raise ValueError(f"GaussianMixturePrior covers 1 <= D <= {K.GMM_MAX_D}, got {D!r}")
        check_options(K_, covariance, 1, 0.0, reg_covar, what="GaussianMixturePrior: ")
        self.D, self.K, self.covariance, self.reg_covar = D, K_, covariance, float(reg_covar)
        self.device = torch.device(device)
        self.weights = self.means = self.covariances = None
        self.rows, self.iterations, self.converged = 0, 0, False
        self._dev = None                      # the device copies of the current parameters

    @property
    def full(self) -> bool:
        return self.covariance == "full"

    # ---- parameters ---------------------------------------------------------------------------------------------------------
    def _set(self, weights, means, covariances) -> None:
        Kc, D = self.K, self.D
        w = torch.as_tensor(np.asarray(weights), dtype=torch.float64).reshape(-1).clone()
        m = torch.as_tensor(np.asarray(means), dtype=torch.float64).clone()
        c = torch.as_tensor(np.asarray(covariances), dtype=torch.float64).clone()
        want = (Kc, D, D) if self.full else (Kc, D)
        if tuple(w.shape) != (Kc,) or tuple(m.shape) != (Kc, D) or tuple(c.shape) != want:
            raise ValueError(f"GaussianMixturePrior: weights, means, covariances must be [{Kc}], [{Kc}, {D}], {list(want)}, got "
                             f"{list(w.shape)}, {list(m.shape)}, {list(c.shape)}")
        if not (torch.isfinite(w).all() and (w > 0).all()):
            raise ValueError("GaussianMixturePrior: the weights must be positive and finite")
        self.weights, self.means, self.covariances = w, m, c
        self._dev = None

    def _factor(self):
        """(L [K, D, D] or sqrt(var) [K, D], P = its inverse, log_det_half [K]) in float64; a ValueError names a component whose
        covariance is not positive definite."""
        c = self.covariances
        if self.full:
            L, info = torch.linalg.cholesky_ex(c)
            bad = torch.nonzero((info != 0) | ~torch.isfinite(L).reshape(self.K, -1).all(1)).reshape(-1)
            if bad.numel():
                raise ValueError(f"the covariance of component {int(bad[0])} is not positive definite (its Cholesky factorisation "
                                 f"failed): use a larger reg_covar or covariance: diag")
            eye = torch.eye(self.D, dtype=torch.float64).expand(self.K, self.D, self.D)
            P = torch.tril(torch.linalg.solve_triangular(L, eye, upper=False))
            ldh = torch.log(torch.diagonal(L, dim1=1, dim2=2)).sum(1)
        else:
            bad = torch.nonzero(~((c > 0) & torch.isfinite(c)).all(1)).reshape(-1)
            if bad.numel():
                raise ValueError(f"the variance of component {int(bad[0])} is not positive: use a larger reg_covar")
            L = torch.sqrt(c)
            P = 1.0 / L
            ldh = torch.log(L).sum(1)
        return L, P, ldh

    def _prepare(self) -> dict:
        if self.weights is None:
            raise RuntimeError("GaussianMixturePrior: fit or load the mixture first")
        if self._dev is None:
            if self.device.type != "cuda":
                raise RuntimeError("GaussianMixturePrior runs on the GPU only: there is no CPU fallback")
            L, P, ldh = self._factor()
            f = lambda t, dtype=torch.float32: t.to(dtype).contiguous().to(self.device)
            self._dev = {"log_w": f(torch.log(self.weights)), "mu": f(self.means), "P": f(P), "ldh": f(ldh), "L": f(L),
                         "cdf": f(torch.cumsum(self.weights, 0), torch.float64)}
        return self._dev

    def _rows(self, X, what):
        if not torch.is_tensor(X) or X.dim() != 2 or X.size(1) != self.D:
            raise ValueError(f"{what} takes X [N, {self.D}], got {tuple(getattr(X, 'shape', ()))}")
        if not X.is_cuda:
            raise RuntimeError("GaussianMixturePrior runs on the GPU only: there is no CPU fallback")
        return X.detach().to(torch.float32).contiguous()

    # ---- EM -----------------------------------------------------------------------------------------------------------------
    def _moments(self, X, bad):
        """(mean [D], biased covariance [D, D] or variance [D]) of the finite rows, float64 on the host: two M steps of one
        component with unit responsibilities, the second centred at the first one's mean."""
        ones = (bad == 0).to(torch.float32).reshape(-1, 1).contiguous()
        zero = torch.zeros(1, self.D, dtype=torch.float32, device=X.device)
        Nk, S1, _ = K.gmm_mstep(X, ones, bad, zero, full=False)
        m32 = (S1 / Nk.reshape(1, 1)).to(torch.float32).contiguous()
        Nk, S1, S2 = K.gmm_mstep(X, ones, bad, m32, full=self.full)
        n = Nk.cpu()[0]
        d = (S1.cpu() / n)[0]
        cov = S2.cpu()[0] / n - (torch.outer(d, d) if self.full else d * d)
        return m32.cpu().double()[0] + d, cov

    def default_start(self, X, seed: int):
        """(weights, means, covariances) of the default start: K distinct finite rows of X as the means, drawn from a CPU generator
        seeded with ``seed``; every component the data's covariance (variance for ``diag``) plus ``reg_covar``; uniform weights."""
        X = self._rows(X, "default_start")
        finite = torch.nonzero(torch.isfinite(X).all(1)).reshape(-1).cpu()
        self._enough(int(finite.numel()), X.size(0))
        g = torch.Generator(device="cpu")
        g.manual_seed(int(seed))
        pick = finite[torch.randperm(finite.numel(), generator=g)[:self.K]]
        means = X[pick.to(X.device)].cpu().double()
        bad = (~torch.isfinite(X).all(1)).to(torch.int32)
        _, cov = self._moments(X, bad)
        cov = cov + self.reg_covar * (torch.eye(self.D, dtype=torch.float64) if self.full else 1.0)
        return (torch.full((self.K,), 1.0 / self.K, dtype=torch.float64), means,
                cov.unsqueeze(0).repeat((self.K,) + (1,) * cov.dim()))

    def _enough(self, finite: int, total: int) -> None:
        if total < 2 or finite < 2:
            raise ValueError(f"a mixture needs at least 2 finite rows, got {finite} of {total}")
        if finite < self.K:
            raise ValueError(f"{finite} finite rows cannot carry {self.K} components: the fit needs at least as many rows as components")

    def fit(self, X, seed: int = 0, max_iter: int = 100, tol: float = 1e-3, init=None) -> dict:
        """EM from ``init = (weights, means, covariances)`` or the default start, until |delta mean ll| < tol (scikit-learn's rule;
        one scalar read per iteration) or ``max_iter``.  Returns ``iterations``, ``converged``, ``loglik_trace`` (the mean
        log-likelihood of the finite rows under the parameters each iteration started from), ``rows`` and ``nonfinite``."""
        check_options(self.K, self.covariance, max_iter, tol, self.reg_covar, what="fit: ")
        X = self._rows(X, "fit")
        N, D, Kc = X.size(0), self.D, self.K
        if N < 2 or N < Kc:
            self._enough(N, N)
        with torch.cuda.device(self.device):
            finite = int(torch.isfinite(X).all(1).sum())
            self._enough(finite, N)
            self._set(*(init if init is not None else self.default_start(X, seed)))
            ws, trace, prev, converged, it = None, [], None, False, 0
            for it in range(1, int(max_iter) + 1):
                dev = self._prepare()
                r, ll, bad = K.gmm_estep(X, dev["log_w"], dev["mu"], dev["P"], dev["ldh"], full=self.full)
                if ws is None:
                    ws = torch.empty(int(K.native.load().ctvae_gmm_mstep_workspace_bytes(N, D, Kc, 1 if self.full else 0)) // 8,
                                     dtype=torch.float64, device=X.device)
                centre = dev["mu"]
                if self.full:
                    # the vector pass (float64 throughout) gives the new means; the tile pass is centred at THEM, so its fp32
                    # rounding is relative to a component's own spread, not to how far its mean moved in this iteration -- a
                    # component that contracts onto a few rows keeps a positive definite covariance
                    Nk, S1, _ = K.gmm_mstep(X, r, bad, centre, full=False, ws=ws)
                    centre = (centre.double() + S1 / (Nk + _EPS10).reshape(Kc, 1)).to(torch.float32).contiguous()
                Nk, S1, S2 = K.gmm_mstep(X, r, bad, centre, full=self.full, ws=ws)
                mean_ll = float(ll.sum(dtype=torch.float64)) / finite             # the iteration's scalar read
                trace.append(mean_ll)
                m = centre.cpu().double()                                         # the point the kernel centred at
                self.weights, self.means, self.covariances = finish_mstep(Nk, S1, S2, m, self.full, self.reg_covar)
                self._dev = None
                if prev is not None and abs(mean_ll - prev) < tol:
                    converged = True
                    break
                prev = mean_ll
            self._factor()                    # the parameters left behind must be usable: a failure is reported now
        self.rows, self.iterations, self.converged = finite, it, converged
        return {"iterations": it, "converged": converged, "loglik_trace": trace, "rows": finite, "nonfinite": N - finite}

    # ---- densities and samples ----------------------------------------------------------------------------------------------
    def log_prob(self, X):
        """(ll [N] fp32, nonfinite [N] int32) on the device: the E step alone.  A row with a non-finite value has ll = 0 and
        flag 1."""
        X = self._rows(X, "log_prob")
        with torch.cuda.device(self.device):
            dev = self._prepare()
            _, ll, bad = K.gmm_estep(X, dev["log_w"], dev["mu"], dev["P"], dev["ldh"], full=self.full)
        return ll, bad

    def standard_log_prob(self, X):
        """The same rows under N(0, I): (ll [N] float64, nonfinite [N] int32), plain torch."""
        X = self._rows(X, "standard_log_prob")
        bad = ~torch.isfinite(X).all(1)
        x = torch.where(bad.unsqueeze(1), torch.zeros_like(X), X).double()
        ll = -0.5 * (x * x).sum(1) - 0.5 * self.D * _LOG_2PI
        return torch.where(bad, torch.zeros_like(ll), ll), bad.to(torch.int32)

    @staticmethod
    def mean_over_finite(ll, bad):
        """The mean of ``ll`` over the rows whose flag is 0 as a float, or None when there is no such row."""
        n = int((bad == 0).sum())
        return float(ll.sum(dtype=torch.float64)) / n if n else None

    def sample(self, n: int, generator=None, u=None, eps=None):
        """(z [n, D] fp32, k [n] int32): ``u = torch.rand(n)`` and ``eps = torch.randn(n, D)`` from ``generator`` (a device
        generator the caller passes), unless given.  The kernel holds no random state."""
        with torch.cuda.device(self.device):
            dev = self._prepare()
            if u is None:
                u = torch.rand(n, generator=generator, device=self.device, dtype=torch.float32)
            if eps is None:
                eps = torch.randn(n, self.D, generator=generator, device=self.device, dtype=torch.float32)
            return K.gmm_sample(u.contiguous(), eps.contiguous(), dev["cdf"], dev["mu"], dev["L"], full=self.full)

    # ---- persistence --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """float64 ``weights`` [K], ``means`` [K, D], ``covariances``, and as one-element arrays ``covariance_type``, ``reg_covar``,
        ``rows`` (the finite rows of the fit), ``iterations``, ``converged``."""
        if self.weights is None:
            raise RuntimeError("GaussianMixturePrior: fit or load the mixture first")
        return {"weights": self.weights.numpy().copy(), "means": self.means.numpy().copy(),
                "covariances": self.covariances.numpy().copy(), "covariance_type": np.asarray([self.covariance]),
                "reg_covar": np.asarray([self.reg_covar], dtype=np.float64), "rows": np.asarray([self.rows], dtype=np.int64),
                "iterations": np.asarray([self.iterations], dtype=np.int64), "converged": np.asarray([bool(self.converged)])}

    def load_state_dict(self, state) -> None:
        one = lambda k: np.asarray(state[k]).reshape(-1)[0]
        if str(one("covariance_type")) != self.covariance:
            raise ValueError(f"GaussianMixturePrior is {self.covariance}, the state is {one('covariance_type')}")
        self._set(state["weights"], state["means"], state["covariances"])
        self.reg_covar = float(one("reg_covar"))
        self.rows, self.iterations, self.converged = int(one("rows")), int(one("iterations")), bool(one("converged"))

    def save(self, path) -> None:
        with open(path, "wb") as f:
            f.write(npz_bytes(self.state_dict()))

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path, allow_pickle=False) as z:
            state = {k: z[k] for k in z.files}
        Kc, D = state["means"].shape
        prior = cls(int(D), int(Kc), covariance=str(state["covariance_type"].reshape(-1)[0]),
                    reg_covar=float(state["reg_covar"].reshape(-1)[0]),
                    device=device)
        prior.load_state_dict(state)
        return prior
