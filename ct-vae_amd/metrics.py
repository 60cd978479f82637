"""Disentanglement metrics on the GPU: counterpart of the reference's ``metrics/metric.py`` (``METRICS``, ``Metric``,
``MetricSet``) for the two metrics that are dense arithmetic over a code matrix.

The reference wraps ``disent.metrics`` (0.7.0).  That package is not a dependency here, so the result names and the arithmetic
are restated from the published algorithms as disentanglement_lib implements them, which disent follows:

* **MIG** (Chen et al. 2018, "Isolating Sources of Disentanglement in VAEs"): the codes of ``num_train`` randomly drawn factor
  rows, every column cut into 20 equal-width bins between its minimum and maximum, the latent x factor mutual information
  matrix, and ``mean_f((top1_f - top2_f) / H_f)`` with ``H_f = MI(f, f)`` the factor's entropy.  Key ``mig.discrete_score``.
* **FactorVaeScore** (Kim & Mnih 2018, "Disentangling by Factorising"): global column variances (ddof = 1) over
  ``num_variance_estimate`` random items; a column is active when ``sqrt(var) >= 0.05``; each group fixes one factor for
  ``batch_size`` items and votes for the active column with the smallest group variance over global variance; the classifier
  is the majority vote per column.  Keys ``factor_vae.train_accuracy``, ``factor_vae.eval_accuracy``,
  ``factor_vae.num_active_dims``.

Parity with disent itself is **unpinned**: nothing here was compared against a disent run, only against the float64 numpy
restatement of the same algorithms kept with the tests.  Known differences: random draws come from one private
``numpy.random.Generator`` (``draw_plan``), so individual samples differ from disent's; the vote table is indexed by the raw
column, not by the position among the active columns (the accuracies are the same).

``"DCI"`` (gradient-boosted trees) and ``"SAP"`` (a linear SVM per latent x factor pair) are CPU-library algorithms and are
refused by name.  The hot arithmetic runs in three HIP kernels (csrc/disent.hip); the top-2, the entropies, the vote table and
the classifier stay on the host.  There is no CPU fallback: codes must be device tensors.
"""
from typing import Callable, List, Sequence

import numpy as np
import torch

from . import native
from .evalrun import eval_mode

METRICS = {"MIG": "mig", "FactorVaeScore": "factor_vae", "": None}
UNSUPPORTED = {"DCI": "it fits gradient-boosted trees (a CPU-library algorithm with no kernel here)",
               "SAP": "it fits one linear SVM per latent x factor pair (a CPU-library algorithm with no kernel here)"}
NUM_BINS = 20
ACTIVE_STD = 0.05
MAX_FACTORS, MAX_FACTOR_SIZE = 16, 256      # csrc/disent.hip


# ---------------------------------------------------------------------------------------------------------------------
# ground truth
# ---------------------------------------------------------------------------------------------------------------------
class FactorGrid:
    """A dataset whose items are the full grid of its ground-truth factors, ordered row-major (the last factor varies
    fastest), as the disent datasets are: item index = ``np.ravel_multi_index(position, factor_sizes)``."""

    def __init__(self, factor_sizes: Sequence[int]):
        sizes = tuple(int(s) for s in factor_sizes)
        if not sizes or any(s < 1 for s in sizes):
            raise ValueError(f"factor_sizes must be a non-empty list of positive sizes, got {list(factor_sizes)}")
        self.factor_sizes = sizes
        self.num_factors = len(sizes)
        self.size = int(np.prod(sizes, dtype=np.int64))
        self._mult = np.array([int(np.prod(sizes[i + 1:], dtype=np.int64)) for i in range(len(sizes))], dtype=np.int64)

    def __len__(self):
        return self.size

    def pos_to_idx(self, pos) -> np.ndarray:
        """positions [..., F] -> item indices [...]."""
        pos = np.asarray(pos, dtype=np.int64)
        if pos.shape[-1] != self.num_factors or (pos < 0).any() or (pos >= np.array(self.factor_sizes)).any():
            raise ValueError("factor position out of range")
        return pos @ self._mult

    def idx_to_pos(self, idx) -> np.ndarray:
        """item indices [...] -> positions [..., F]."""
        idx = np.asarray(idx, dtype=np.int64)
        if (idx < 0).any() or (idx >= self.size).any():
            raise ValueError("item index out of range")
        return (idx[..., None] // self._mult) % np.array(self.factor_sizes, dtype=np.int64)

    def sample_factors(self, n: int, rng: np.random.Generator) -> np.ndarray:
        """n uniformly drawn factor rows [n, F] (int64)."""
        return rng.integers(0, np.array(self.factor_sizes, dtype=np.int64), size=(n, self.num_factors), dtype=np.int64)


class FactorData:
    """An ``HbmImageStore`` that holds the whole grid: ``observations(factor_rows)`` fetches the items of factor rows."""

    def __init__(self, store, grid: FactorGrid):
        if len(store) != grid.size:
            raise ValueError(f"the store holds {len(store)} items but factor sizes {list(grid.factor_sizes)} span {grid.size}")
        self.store, self.grid = store, grid

    def __len__(self):
        return self.grid.size

    def observations(self, factor_rows) -> torch.Tensor:
        return self.items(self.grid.pos_to_idx(factor_rows))

    def items(self, rows) -> torch.Tensor:
        return self.store.fetch(torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int64)))


# ---------------------------------------------------------------------------------------------------------------------
# every random draw of an evaluation
# ---------------------------------------------------------------------------------------------------------------------
def draw_plan(metric_name: str, grid: FactorGrid, batch_size: int, num_train: int, num_eval: int = 0,
              num_variance_estimate: int = 0, seed: int = 0) -> dict:
    """Plain host arrays (int64) naming every item an evaluation encodes, from a private ``numpy.random.Generator``.

    MIG: ``factors`` [num_train, F] and their item ``rows`` [num_train].  FactorVaeScore: ``variance_rows``
    [num_variance_estimate]; per stage (``train``: num_train groups, ``eval``: num_eval groups) the fixed factor of each
    group ``<stage>_factor`` [G] and the items ``<stage>_rows`` [G, batch_size], whose factor rows all carry the first
    one's value of the fixed factor."""
    rng = np.random.default_rng(int(seed))
    if metric_name == "MIG":
        factors = grid.sample_factors(num_train, rng)
        return {"factors": factors, "rows": grid.pos_to_idx(factors)}
    if metric_name == "FactorVaeScore":
        plan = {"variance_rows": grid.pos_to_idx(grid.sample_factors(num_variance_estimate, rng))}
        for stage, groups in (("train", num_train), ("eval", num_eval)):
            fixed = rng.integers(0, grid.num_factors, size=groups, dtype=np.int64)
            factors = grid.sample_factors(groups * batch_size, rng).reshape(groups, batch_size, grid.num_factors)
            g = np.arange(groups)
            factors[g, :, fixed] = factors[g, 0, fixed][:, None]
            plan[stage + "_factor"] = fixed
            plan[stage + "_rows"] = grid.pos_to_idx(factors)
        return plan
    raise ValueError(f"no plan for metric {metric_name!r}")


# ---------------------------------------------------------------------------------------------------------------------
# the three launches (csrc/disent.hip)
# ---------------------------------------------------------------------------------------------------------------------
def _codes(z: torch.Tensor, dim: int) -> torch.Tensor:
    if not (torch.is_tensor(z) and z.is_cuda):
        raise RuntimeError("the metric kernels need the codes on a GPU (no CPU fallback)")
    if z.dim() != dim:
        raise ValueError(f"expected a {dim}-d code tensor, got shape {tuple(z.shape)}")
    return z.detach().to(torch.float32).contiguous()


def column_moments(z: torch.Tensor):
    """z [N, L] -> (mean, unbiased variance, min, max), each [L]."""
    z = _codes(z, 2)
    N, L = z.shape
    out = torch.empty((4, L), dtype=torch.float32, device=z.device)
    native.call("ctvae_column_moments", z.data_ptr(), N, L, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                out[3].data_ptr())
    return out[0], out[1], out[2], out[3]


def mi_matrix(z: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, factors: torch.Tensor, sizes: Sequence[int],
              want_bins: bool = False):
    """Mutual information [L, F] (nats) between the 20-bin discretisation of every column of z [N, L] over [lo, hi] and the
    factors [N, F] (int32 on the device, factor f in 0 .. sizes[f]-1); with ``want_bins`` also the bins [N, L] (uint8)."""
    z = _codes(z, 2)
    N, L = z.shape
    F = len(sizes)
    if tuple(factors.shape) != (N, F) or factors.dtype != torch.int32 or not factors.is_cuda:
        raise ValueError(f"factors must be an int32 device tensor [{N}, {F}]")
    factors = factors.contiguous()
    lo, hi = _codes(lo, 1), _codes(hi, 1)
    if lo.numel() != L or hi.numel() != L:
        raise ValueError("lo / hi must have one entry per column")
    sizes_host = np.ascontiguousarray(sizes, dtype=np.int32)          # read by the launcher before the launch
    mi = torch.empty((L, F), dtype=torch.float32, device=z.device)
    bins = torch.empty((N, L), dtype=torch.uint8, device=z.device) if want_bins else None
    native.call("ctvae_mi_matrix", z.data_ptr(), lo.data_ptr(), hi.data_ptr(), factors.data_ptr(), sizes_host.ctypes.data, N, L, F,
                mi.data_ptr(), native.ptr(bins))
    return (mi, bins) if want_bins else mi


def group_var_argmin(z: torch.Tensor, global_var: torch.Tensor, active: torch.Tensor):
    """z [G, B, L] -> (arg [G] int32, val [G]): per group the active column with the smallest unbiased variance over the B
    rows divided by global_var; ties go to the lowest column; -1 / inf without an active column."""
    z = _codes(z, 3)
    G, B, L = z.shape
    global_var = _codes(global_var, 1)
    active = active.to(device=z.device, dtype=torch.uint8).contiguous()
    if global_var.numel() != L or active.numel() != L:
        raise ValueError("global_var / active must have one entry per column")
    arg = torch.empty(G, dtype=torch.int32, device=z.device)
    val = torch.empty(G, dtype=torch.float32, device=z.device)
    native.call("ctvae_group_var_argmin", z.data_ptr(), global_var.data_ptr(), active.data_ptr(), G, B, L, arg.data_ptr(),
                val.data_ptr())
    return arg, val


# ---------------------------------------------------------------------------------------------------------------------
# the metrics
# ---------------------------------------------------------------------------------------------------------------------
ENCODE_ROWS = 256       # FactorVaeScore: whole groups up to this many items go through one repr_func call


def _encode(dataset: FactorData, repr_func: Callable, rows: np.ndarray, chunk: int) -> torch.Tensor:
    """Codes [len(rows), L] of the items ``rows``, ``chunk`` items per ``repr_func`` call."""
    out = None
    for i in range(0, len(rows), chunk):
        z = repr_func(dataset.items(rows[i:i + chunk]))
        z = _codes(z.reshape(z.size(0), -1), 2)
        if out is None:
            out = torch.empty((len(rows), z.size(1)), dtype=torch.float32, device=z.device)
        out[i:i + z.size(0)] = z
    return out


def metric_mig(dataset: FactorData, repr_func: Callable, plan: dict, batch_size: int) -> dict:
    sizes = dataset.grid.factor_sizes
    z = _encode(dataset, repr_func, plan["rows"], batch_size)
    if z.size(1) < 2:
        raise ValueError("MIG needs at least two latent columns")
    _, _, lo, hi = column_moments(z)
    factors = torch.from_numpy(plan["factors"].astype(np.int32)).to(z.device)
    mi = mi_matrix(z, lo, hi, factors, sizes)
    top = torch.topk(mi, 2, dim=0).values.double().cpu().numpy()          # [2, F]
    gaps = []
    for f, s in enumerate(sizes):                                         # H_f = MI(f, f): the entropy of the drawn values
        p = np.bincount(plan["factors"][:, f], minlength=s) / float(len(plan["factors"]))
        p = p[p > 0]
        gaps.append((top[0, f] - top[1, f]) / -(p * np.log(p)).sum())
    return {"mig.discrete_score": float(np.mean(gaps))}


def _votes(dataset, repr_func, rows, fixed, gvar, active, num_factors, batch_size):
    G, L = len(fixed), gvar.numel()
    per_call = max(1, ENCODE_ROWS // batch_size)
    args = []
    for g in range(0, G, per_call):
        r = rows[g:g + per_call]
        z = _encode(dataset, repr_func, r.reshape(-1), r.size)
        args.append(group_var_argmin(z.view(r.shape[0], batch_size, L), gvar, active)[0])
    votes = np.zeros((num_factors, L), dtype=np.int64)
    np.add.at(votes, (fixed, torch.cat(args).cpu().numpy().astype(np.int64)), 1)
    return votes


def metric_factor_vae(dataset: FactorData, repr_func: Callable, plan: dict, batch_size: int) -> dict:
    if batch_size < 2:
        raise ValueError("FactorVaeScore needs groups of at least two items (batch_size >= 2)")
    F = dataset.grid.num_factors
    zv = _encode(dataset, repr_func, plan["variance_rows"], ENCODE_ROWS)
    gvar = column_moments(zv)[1]
    active = gvar.sqrt() >= ACTIVE_STD
    num_active = int(active.sum())
    if num_active == 0:
        return {"factor_vae.train_accuracy": 0.0, "factor_vae.eval_accuracy": 0.0, "factor_vae.num_active_dims": 0}
    train = _votes(dataset, repr_func, plan["train_rows"], plan["train_factor"], gvar, active, F, batch_size)
    classifier = train.argmax(axis=0)
    cols = np.arange(train.shape[1])
    ev = _votes(dataset, repr_func, plan["eval_rows"], plan["eval_factor"], gvar, active, F, batch_size)
    return {"factor_vae.train_accuracy": float(train[classifier, cols].sum() / train.sum()),
            "factor_vae.eval_accuracy": float(ev[classifier, cols].sum() / ev.sum()),
            "factor_vae.num_active_dims": num_active}


_COMPUTE = {"MIG": metric_mig, "FactorVaeScore": metric_factor_vae}


class Metric:
    """One metric over a ``FactorData`` (metrics/metric.py:17-46, with the reference's argument handling: MIG drops
    ``num_test``; FactorVaeScore turns it into ``num_eval`` and uses ``num_variance_estimate = 512``)."""

    def __init__(self, metric_name: str, dataset: FactorData, batch_size: int = 64, num_train: int = 1000, num_test: int = 500,
                 seed: int = 0, **kwargs):
        if metric_name in UNSUPPORTED:
            raise ValueError(f"metric {metric_name!r} is not supported: {UNSUPPORTED[metric_name]}; "
                             f"supported: {sorted(k for k in METRICS if k)}")
        if metric_name not in METRICS:
            raise ValueError(f"unknown metric {metric_name!r}; supported: {sorted(k for k in METRICS if k)}")
        self.metric = METRICS[metric_name]
        self.name = metric_name
        self.dataset = dataset
        self.seed = int(seed)
        self.args = {"batch_size": batch_size, "num_train": num_train, "num_test": num_test}
        if metric_name == "MIG":
            del self.args["num_test"]
        if metric_name == "FactorVaeScore":
            del self.args["num_test"]
            self.args["num_eval"] = num_test
            self.args["num_variance_estimate"] = 64 * 2 ** 3
        if self.metric is not None and dataset is not None:
            sizes = dataset.grid.factor_sizes
            if len(sizes) > MAX_FACTORS or min(sizes) < 2 or max(sizes) > MAX_FACTOR_SIZE:
                raise ValueError(f"factor sizes {list(sizes)}: the kernels take up to {MAX_FACTORS} factors of 2 to "
                                 f"{MAX_FACTOR_SIZE} values")

    def plan(self, seed=None) -> dict:
        a = self.args
        return draw_plan(self.name, self.dataset.grid, a["batch_size"], a["num_train"], a.get("num_eval", 0),
                         a.get("num_variance_estimate", 0), self.seed if seed is None else seed)

    def compute(self, repr_func: Callable, model=None, seed=None) -> dict:
        """Draw the plan, encode it with ``repr_func`` and score it.  ``model`` (the module behind ``repr_func``) runs under
        ``eval()`` and ``no_grad()`` and gets its previous mode back; ``seed`` overrides the constructor's for this call.
        Touches neither torch's CPU / device generators nor a model's own random state."""
        if self.metric is None:
            return {}
        if model is None:                      # exp.metric_func: the harness's model is the module behind it
            model = getattr(getattr(repr_func, "__self__", None), "model", None)
        plan = self.plan(seed)
        with eval_mode(model):
            return _COMPUTE[self.name](self.dataset, repr_func, plan, self.args["batch_size"])


class MetricSet(Metric):
    """Several metrics over one dataset; ``compute`` merges their result dicts (metrics/metric.py:49-68)."""

    def __init__(self, metric_names: List[str], dataset: FactorData, batch_size: int = 64, num_train: int = 1000,
                 num_test: int = 500, seed: int = 0, **kwargs):
        self.metrics = [Metric(name, dataset, batch_size, num_train, num_test, seed) for name in metric_names]

    def compute(self, repr_func: Callable, model=None, seed=None) -> dict:
        res = {}
        for metric in self.metrics:
            res.update(metric.compute(repr_func, model=model, seed=seed))
        return res
