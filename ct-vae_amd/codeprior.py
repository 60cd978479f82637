"""An interpolated Markov prior over the code grids of the quantising models, so that they can sample (van den Oord et al. 2017,
section 3.3, with counts in place of a PixelCNN; the interpolation weights by deleted interpolation, Jelinek & Mercer 1980).

An image is a grid of codes ``i[c][h][w]`` in [0, K): C codebooks (1 for ``VQVAE``), H x W positions, ordered raster over (h, w) and
within a position codebooks 0 .. C-1.  ``p(image) = prod p(i[c][h][w] | context)`` with ``p(k | context) = sum_j lambda[c][j]
P_j(k | context_j)`` over the experts ``EXPERTS``: uniform, position (h, w), left neighbour, upper neighbour, previous codebook at
the same position -- the last three with the boundary symbol K where there is no neighbour.  ``P_j`` is a row of an int64 count
table divided by the row's total; an empty row is uniform.

* ``MarkovCodePrior`` -- ``count`` (``ctvae_code_prior_count``: exact integer statistics), ``fit_weights`` (EM on rows that were not
  counted; one ``ctvae_code_prior_score`` launch per round, the weights kept in float64 on the host), ``log_prob``, ``sample``
  (``ctvae_code_prior_sample``: ancestral, from float64 uniforms of a generator of the prior's own), ``decode_samples``
  (``ctvae_code_prior_embed``, then ``model.decode``), ``save`` / ``load``, ``summary``.
* ``code_prior_setting`` / ``prior_supported`` / ``needs_supported_model`` -- ``exp_params.code_prior`` and the models it is refused for.
* ``CodeGridBuffer`` -- the validation indices of an epoch in one device buffer that grows by doubling.
* ``grid_indices`` / ``codebooks_of`` -- a served model's index grid [B, C, H, W] of a batch, and its codebooks.

There is no CPU path for the device parts.
"""
import math

import numpy as np
import torch

from . import kernels as K
from .evalrun import eval_mode, npz_bytes

CODE_PRIOR_DIR = "Priors"
CODE_PRIOR_MODELS = ("MCQVAE", "VQVAE")
EXPERTS = K.CODE_PRIOR_EXPERTS
J = len(EXPERTS)
SETTING_DEFAULTS = {"em_iters": 20, "uniform_floor": 1e-3}
RECORD_PREFIX = "val_code_prior_"


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def check_options(em_iters, uniform_floor, what="code_prior.") -> None:
    """The ranges every entry to the fit shares; a ValueError names the field (``what`` goes in front of its name; "--": as a
    command-line option)."""
    def nm(field):
        return what + (field.replace("_", "-") if what == "--" else field)
    if not _is_int(em_iters) or em_iters < 1:
        raise ValueError(f"{nm('em_iters')} must be an integer of at least 1, got {em_iters!r}")
    if isinstance(uniform_floor, bool) or not isinstance(uniform_floor, float) or not 0.0 < uniform_floor < 1.0:
        raise ValueError(f"{nm('uniform_floor')} must be a float inside (0, 1), got {uniform_floor!r}")


def code_prior_setting(value):
    """Validated ``exp_params.code_prior``: None (absent: off) or a mapping with ``type: markov`` and the optional ``em_iters`` (an
    int >= 1, default 20) and ``uniform_floor`` (a float inside (0, 1), default 1e-3).  Returns None or the complete dict; anything
    else is a ValueError that names the field."""
    if value is None:
        return None
    if not isinstance(value, dict):
        raise ValueError(f"code_prior must be a mapping with type: markov, got {value!r}")
    if value.get("type") != "markov":
        raise ValueError(f"code_prior.type must be markov, got {value.get('type')!r}")
    extra = sorted(str(k) for k in value if k != "type" and k not in SETTING_DEFAULTS)
    if extra:
        raise ValueError(f"code_prior has unknown field(s) {', '.join(extra)}; known: type, {', '.join(SETTING_DEFAULTS)}")
    out = {"type": "markov", **SETTING_DEFAULTS, **{k: v for k, v in value.items() if k != "type"}}
    check_options(out["em_iters"], out["uniform_floor"])
    return out


def _class_of(model_or_class):
    return model_or_class if isinstance(model_or_class, type) else type(model_or_class)


def prior_supported(model_or_class) -> bool:
    """Whether the model is one of ``CODE_PRIOR_MODELS``, by class."""
    return _class_of(model_or_class).__name__ in CODE_PRIOR_MODELS


def needs_supported_model(model_or_class, name=None) -> str:
    """The refusal of ``code_prior`` for any other model, by name."""
    cls = _class_of(model_or_class)
    got = name if name is not None else getattr(cls, "__name__", cls)
    if getattr(cls, "__name__", None) == "CTMCQVAE":
        return (f"code_prior does not serve CTMCQVAE (got {got}): its batches come in modes and its decoder input passes through "
                f"the causal-transition layer, which is out of scope here; served: {', '.join(CODE_PRIOR_MODELS)}")
    return (f"code_prior needs a quantising model whose decoder takes the quantised grid alone ({', '.join(CODE_PRIOR_MODELS)}), "
            f"got {got}")


def codebooks_of(model) -> list:
    """The C codebooks [K, Dc] of a served model, stored back to back."""
    vq = model.vq_layer
    return vq._codebooks() if hasattr(vq, "_codebooks") else [vq.embedding.weight]


def grid_indices(model, x) -> torch.Tensor:
    """int64 [B, C, H, W]: ``model.vq_layer.compute_inds(model.encode(x)[0])``; ``VQVAE``'s [B, H, W] gets its codebook axis."""
    inds = model.vq_layer.compute_inds(model.encode(x)[0])
    return (inds.unsqueeze(1) if inds.dim() == 3 else inds).contiguous()


class CodeGridBuffer:
    """[rows, C, H, W] int64 on the device, appended to batch by batch; the capacity doubles when a batch does not fit.  The grid
    shape is the first batch's."""

    def __init__(self, device, capacity: int = 1024):
        self.device, self.rows, self.shape = torch.device(device), 0, None
        self._cap0 = max(int(capacity), 1)
        self._buf = None

    def append(self, inds: torch.Tensor) -> None:
        if inds.dim() == 3:
            inds = inds.unsqueeze(1)
        if inds.dim() != 4 or inds.dtype != torch.int64 or (self.shape is not None and tuple(inds.shape[1:]) != self.shape):
            want = list(self.shape) if self.shape is not None else ["C", "H", "W"]
            raise ValueError(f"CodeGridBuffer.append takes int64 indices [B, {', '.join(str(s) for s in want)}], got "
                             f"{getattr(inds, 'dtype', None)} {tuple(inds.shape)}")
        B = inds.size(0)
        if self._buf is None:
            self.shape = tuple(inds.shape[1:])
            self._buf = torch.empty(max(self._cap0, B), *self.shape, dtype=torch.int64, device=self.device)
        if self.rows + B > self._buf.size(0):
            cap = self._buf.size(0)
            while cap < self.rows + B:
                cap *= 2
            grown = torch.empty(cap, *self.shape, dtype=torch.int64, device=self.device)
            grown[:self.rows].copy_(self._buf[:self.rows])
            self._buf = grown
        self._buf[self.rows:self.rows + B].copy_(inds.detach())
        self.rows += B

    def clear(self) -> None:
        self.rows = 0

    def view(self) -> torch.Tensor:
        if self._buf is None:
            return torch.empty(0, 1, 1, 1, dtype=torch.int64, device=self.device)
        return self._buf[:self.rows]


class MarkovCodePrior:
    """The four count tables on the device (int64), ``weights`` (lambda, float64 [C, J]) on the host."""

    def __init__(self, K_: int, C: int, H: int, W: int, device="cuda"):
        K.code_prior_limits("MarkovCodePrior", K_, C, H, W)
        self.K, self.C, self.H, self.W = K_, C, H, W
        self.device = torch.device(device)
        self.weights = np.full((C, J), 1.0 / J, dtype=np.float64)
        self.rows, self.invalid, self.em_iters, self.uniform_floor = 0, 0, 0, 0.0
        self.tables = self._invalid = None
        self._dev = None                      # (totals, lambda) on the device for the current tables and weights

    # ---- statistics ---------------------------------------------------------------------------------------------------------
    def _grid(self, inds, what):
        if not torch.is_tensor(inds) or inds.dim() != 4 or tuple(inds.shape[1:]) != (self.C, self.H, self.W):
            raise ValueError(f"{what} takes inds [B, {self.C}, {self.H}, {self.W}], got {tuple(getattr(inds, 'shape', ()))}")
        if not inds.is_cuda:
            raise RuntimeError("MarkovCodePrior runs on the GPU only: there is no CPU fallback")
        return inds.detach().contiguous()

    def _ensure_tables(self):
        if self.tables is None:
            if self.device.type != "cuda":
                raise RuntimeError("MarkovCodePrior runs on the GPU only: there is no CPU fallback")
            self.tables, self._invalid = K.code_prior_tables(self.K, self.C, self.H, self.W, self.device)

    def count(self, inds) -> int:
        """Adds the tokens of ``inds`` [B, C, H, W] to the tables (they accumulate over calls); returns the tokens left out so
        far because a code was out of range (one scalar read)."""
        inds = self._grid(inds, "count")
        self._ensure_tables()
        with torch.cuda.device(self.device):
            if inds.size(0):
                K.code_prior_count(inds, self.tables, self._invalid)
            self.invalid = int(self._invalid)
        self.rows += inds.size(0)
        self._dev = None
        return self.invalid

    def _prepare(self):
        if self.tables is None:
            raise RuntimeError("MarkovCodePrior: count or load the tables first")
        if self._dev is None:
            totals = K.code_prior_totals(self.tables)
            lam = torch.from_numpy(np.ascontiguousarray(self.weights)).to(self.device)
            self._dev = (totals, lam)
        return self._dev

    def _set_weights(self, lam) -> None:
        self.weights = np.ascontiguousarray(lam, dtype=np.float64)
        if self._dev is not None:
            self._dev = (self._dev[0], torch.from_numpy(self.weights).to(self.device))

    def fit_weights(self, inds, em_iters: int = 20, uniform_floor: float = 1e-3) -> dict:
        """``em_iters`` rounds of deleted interpolation on ``inds`` -- rows that were NOT counted -- from lambda = 1/J: r_j =
        lambda_j P_j / sum_j' lambda_j' P_j' per token, lambda_j <- the mean of r_j over the tokens of codebook c (the images with
        an out-of-range index left out), then lambda <- (1 - eps) lambda + eps e_0.  One launch and one copy of ``resp`` per round,
        summed on the host in float64, always in the same order.  Returns ``rows`` (the images used) and ``bad``."""
        check_options(em_iters, uniform_floor, what="fit_weights: ")
        inds = self._grid(inds, "fit_weights")
        if inds.size(0) < 1:
            raise ValueError("fit_weights needs at least 1 row")
        eps = float(uniform_floor)
        e0 = np.zeros(J, dtype=np.float64)
        e0[0] = 1.0
        self._set_weights(np.full((self.C, J), 1.0 / J, dtype=np.float64))
        good = None
        with torch.cuda.device(self.device):
            for _ in range(int(em_iters)):
                totals, lam = self._prepare()
                _, resp, bad = K.code_prior_score(inds, self.tables, totals, lam)
                if good is None:              # (the flags depend on the indices alone: read once)
                    good = int((bad == 0).sum())
                    if good == 0:
                        raise ValueError("fit_weights: every row holds an index outside [0, K)")
                tokens = float(good * self.H * self.W)
                new = np.add.reduce(resp.cpu().numpy(), axis=0) / tokens    # the round's copy (the rows of bad images are zeros)
                self._set_weights((1.0 - eps) * new + eps * e0)
        self.em_iters, self.uniform_floor = int(em_iters), eps
        return {"rows": good, "bad": int(inds.size(0)) - good}

    # ---- densities and samples ----------------------------------------------------------------------------------------------
    def log_prob(self, inds):
        """(logp float64 [B, C], bad int32 [B]) on the device; an image with an out-of-range index has logp = 0 and flag 1."""
        inds = self._grid(inds, "log_prob")
        with torch.cuda.device(self.device):
            totals, lam = self._prepare()
            logp, _, bad = K.code_prior_score(inds, self.tables, totals, lam)
        return logp, bad

    def summary(self, inds) -> dict:
        """``nats_per_code`` (mean -log p per code over the images without a bad index), ``bits_per_code``, ``uniform_nats`` = ln K,
        ``nats_per_code_<c>`` per codebook as the list ``per_codebook``, ``weights`` [C][J], ``rows`` and ``bad``; the nats are left
        out when no image is left."""
        logp, bad = self.log_prob(inds)
        ok = bad.cpu().numpy() == 0
        lp = logp.cpu().numpy()[ok]
        out = {"uniform_nats": math.log(self.K), "weights": [[float(v) for v in row] for row in self.weights],
               "rows": int(ok.sum()), "bad": int((~ok).sum())}
        if len(lp):
            per = -lp.sum(axis=0, dtype=np.float64) / (len(lp) * self.H * self.W)
            out["per_codebook"] = [float(v) for v in per]
            out["nats_per_code"] = float(per.sum() / self.C)
            out["bits_per_code"] = out["nats_per_code"] / math.log(2.0)
        return out

    def sample(self, n: int, generator=None, u=None):
        """int64 ``inds`` [n, C, H, W]: token t of image i consumes ``u[i][h*W + w][c][0..1]``, drawn with ``torch.rand(...,
        dtype=float64)`` from ``generator`` (a device generator of the caller's) unless ``u`` is given.  The kernel holds no
        random state."""
        with torch.cuda.device(self.device):
            totals, lam = self._prepare()
            if u is None:
                u = torch.rand(int(n), self.H * self.W, self.C, 2, generator=generator, device=self.device, dtype=torch.float64)
            return K.code_prior_sample(self.tables, totals, lam, u, self.H, self.W)

    def decode_samples(self, model, inds):
        """``model.decode`` of the quantised grid of ``inds`` (``ctvae_code_prior_embed``: the codes' rows, NHWC), in eval mode."""
        inds = self._grid(inds, "decode_samples")
        with eval_mode(model), torch.cuda.device(self.device):
            q = K.code_prior_embed(inds, [w.detach() for w in codebooks_of(model)])
            return model.decode(K.to_nchw_view(q))

    # ---- persistence --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """int64 ``pos``, ``left``, ``up``, ``prev``, float64 ``lambda`` [C, J], and as one-element arrays ``K``, ``C``, ``H``, ``W``,
        ``rows``, ``em_iters``, ``uniform_floor``."""
        if self.tables is None:
            raise RuntimeError("MarkovCodePrior: count or load the tables first")
        one = lambda v, dtype=np.int64: np.asarray([v], dtype=dtype)
        out = {name: t.cpu().numpy() for name, t in zip(K.CODE_PRIOR_TABLES, self.tables)}
        out.update({"lambda": self.weights.copy(), "K": one(self.K), "C": one(self.C), "H": one(self.H), "W": one(self.W),
                    "rows": one(self.rows), "em_iters": one(self.em_iters), "uniform_floor": one(self.uniform_floor, np.float64)})
        return out

    def load_state_dict(self, state) -> None:
        one = lambda k: np.asarray(state[k]).reshape(-1)[0]
        if tuple(int(one(k)) for k in "KCHW") != (self.K, self.C, self.H, self.W):
            raise ValueError(f"MarkovCodePrior is (K, C, H, W) = {(self.K, self.C, self.H, self.W)}, the state is "
                             f"{tuple(int(one(k)) for k in 'KCHW')}")
        lam = np.asarray(state["lambda"], dtype=np.float64)
        if lam.shape != (self.C, J) or not np.isfinite(lam).all() or (lam < 0).any():
            raise ValueError(f"MarkovCodePrior: lambda must be [{self.C}, {J}], finite and non-negative")
        self._ensure_tables()
        for name, t in zip(K.CODE_PRIOR_TABLES, self.tables):
            src = np.asarray(state[name])
            if src.dtype != np.int64 or tuple(src.shape) != tuple(t.shape):
                raise ValueError(f"MarkovCodePrior: {name} must be int64 {list(t.shape)}, got {src.dtype} {list(src.shape)}")
            t.copy_(torch.from_numpy(np.ascontiguousarray(src)))
        self._invalid.zero_()
        self._dev = None
        self._set_weights(lam)
        self.rows, self.em_iters, self.uniform_floor = int(one("rows")), int(one("em_iters")), float(one("uniform_floor"))

    def save(self, path) -> None:
        with open(path, "wb") as f:
            f.write(npz_bytes(self.state_dict()))

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path, allow_pickle=False) as z:
            state = {k: z[k] for k in z.files}
        prior = cls(*(int(np.asarray(state[k]).reshape(-1)[0]) for k in "KCHW"), device=device)
        prior.load_state_dict(state)
        return prior


def fit_halves(prior, inds, em_iters, uniform_floor) -> dict:
    """What the training hook and the command share: the even-ordinal rows of ``inds`` are counted, the odd-ordinal rows fit the
    weights.  Fewer than 2 rows is a ValueError."""
    if inds.size(0) < 2:
        raise ValueError(f"a code prior needs at least 2 rows (one to count, one to fit the weights on), got {inds.size(0)}")
    prior.count(inds[0::2].contiguous())
    return prior.fit_weights(inds[1::2].contiguous(), em_iters, uniform_floor)


def record(summary: dict, counted_rows: int, invalid: int) -> dict:
    """A ``summary`` as log entries: ``val_code_prior_nats`` / ``_bits`` / ``_uniform_nats`` / ``_nats_<c>`` / ``_weight_<expert>`` (the
    mean over the codebooks) / ``_rows`` (the rows counted) / ``_invalid``."""
    p = RECORD_PREFIX
    rec = {}
    if "nats_per_code" in summary:
        rec[p + "nats"], rec[p + "bits"] = summary["nats_per_code"], summary["bits_per_code"]
    rec[p + "uniform_nats"] = summary["uniform_nats"]
    for c, v in enumerate(summary.get("per_codebook", ())):
        rec[f"{p}nats_{c}"] = v
    w = np.asarray(summary["weights"], dtype=np.float64)
    for j, name in enumerate(EXPERTS):
        rec[f"{p}weight_{name}"] = float(w[:, j].sum() / w.shape[0])
    rec[p + "rows"], rec[p + "invalid"] = int(counted_rows), int(invalid)
    return rec
