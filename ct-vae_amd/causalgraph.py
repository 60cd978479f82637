"""The causal graphs a CT-MCQ-VAE learns, per action and as pictures.

``CausalTransition`` infers an adjacency over the S latent nodes with one graph discoverer per action, and an intervention mask
that says where an action acts (models/causal.py).  The model reports both only as means over whatever a batch holds; here they
are accumulated PER GROUP -- group 0: no intervention (base mode), group 1 + a: action a -- over as many batches as one likes:

* ``GraphStats`` -- float64 sums of the adjacencies and masks, int32 counts of the edges above a threshold and of the rows, on
  the device (csrc/graphstat.hip: ``ctvae_graph_accumulate``, one launch per batch, no host synchronisation).  Every
  accumulator element is the sum of its rows in ascending order, so a result does not depend on the batch size.  An instance is
  also the ``graph_observer`` of a ``CausalTransition``.
* ``colormap`` / ``heatmap_u8`` / ``save_heatmaps`` -- matrices as a tiled, colour-mapped PNG sheet in one kernel pass
  (``ctvae_heatmap_u8``) and ``imagegrid.png_bytes``.  The value range is fixed, never taken from the data: the sheets of
  different actions and epochs are comparable.
* ``collect_graphs`` -- the base- and action-mode batches of an iterable through a model; ``summarize`` -- the result as a
  JSON-ready dict per group.

Every model call runs under ``evalrun.eval_mode`` and ``evalrun.seeded_torch_rng`` (rollout.py).  There is no CPU path.
"""
from typing import Iterable, Optional, Sequence

import numpy as np
import torch

from . import imagegrid, native
from .evalrun import batch_mode, eval_mode, seeded_torch_rng, unpack_batch
from .rollout import _need_ct, _need_gpu, factor_names

# (index, (R, G, B)): black - purple - red - orange - white.  No channel ever falls, and in every segment one channel climbs by at
# least one per step, so the 256 entries are distinct and their luminance strictly increases.
ANCHORS = ((0, (0, 0, 0)), (64, (72, 0, 104)), (128, (200, 40, 110)), (192, (255, 168, 112)), (255, (255, 255, 255)))
PAD_COLOR = (64, 64, 64)           # a grey that the table does not hold: borders and empty cells cannot be mistaken for values


def colormap() -> np.ndarray:
    """The [256, 3] uint8 colour table: integer interpolation between ``ANCHORS``."""
    table = np.zeros((256, 3), dtype=np.uint8)
    for (i0, c0), (i1, c1) in zip(ANCHORS[:-1], ANCHORS[1:]):
        n = i1 - i0
        for k in range(n + 1):
            table[i0 + k] = [a + (b - a) * k // n for a, b in zip(c0, c1)]
    return table


class GraphStats:
    """Per-group accumulators of adjacencies [B, S, S] and masks [B, S] (include/ctvae_hip.h: ctvae_graph_accumulate)."""

    def __init__(self, groups: int, S: int, device, threshold: float = 0.5):
        self.G, self.S, self.threshold = int(groups), int(S), float(threshold)
        if self.G < 1 or self.S < 1:
            raise ValueError(f"GraphStats needs at least one group and one node, got {groups} groups of {S} nodes")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GraphStats runs on the GPU only: there is no CPU fallback")
        self.hw = None                          # (h, w) of the latent grid, once an observed forward has told it
        self._buf = None                        # made by the first update: constructing one touches no device

    def _layout(self):
        """Word offsets in the one int32 buffer: the float64 parts first (8-byte aligned), then the counts."""
        G, SS, S = self.G, self.S * self.S, self.S
        names = (("adj_sum", 2 * G * SS), ("mask_sum", 2 * G * S), ("edge_count", G * SS), ("rows", G), ("mask_rows", G), ("skipped", 1))
        off, lay = 0, {}
        for k, n in names:
            lay[k] = (off, n)
            off += n
        return lay, off

    def _buffer(self) -> torch.Tensor:
        if self._buf is None:
            self._buf = torch.zeros(self._layout()[1], dtype=torch.int32, device=self.device)
        return self._buf

    def update(self, adj: torch.Tensor, group: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> None:
        """Add the rows of adj [B, S, S]; group [B] (integers; None: every row is group 0), mask [B, S] or None.  One launch, no
        host sync.  A row whose group lies outside [0, groups) only counts as skipped."""
        adj = _need_gpu(adj, "GraphStats.update")
        if adj.dim() != 3 or adj.size(1) != self.S or adj.size(2) != self.S:
            raise ValueError(f"GraphStats.update takes adj [B, {self.S}, {self.S}], got {tuple(adj.shape)}")
        B = adj.size(0)
        if group is not None and tuple(_need_gpu(group, "GraphStats.update").shape) != (B,):
            raise ValueError(f"group must be [{B}], got {tuple(group.shape)}")
        if mask is not None and _need_gpu(mask, "GraphStats.update").numel() != B * self.S:
            raise ValueError(f"mask must hold {B} x {self.S} values, got {tuple(mask.shape)}")
        buf = self._buffer()
        if B == 0:
            return
        a = adj.detach().to(device=self.device, dtype=torch.float32).contiguous()
        if group is None:
            g = torch.zeros(B, dtype=torch.int32, device=self.device)
        else:
            g = group.detach().to(device=self.device, dtype=torch.int32).contiguous()
        m = None if mask is None else mask.detach().to(device=self.device, dtype=torch.float32).reshape(B, self.S).contiguous()
        lay = self._layout()[0]
        base = buf.data_ptr()
        p = {k: base + 4 * off for k, (off, _) in lay.items()}
        with torch.cuda.device(self.device):
            native.call("ctvae_graph_accumulate", a.data_ptr(), g.data_ptr(), native.ptr(m), self.threshold, B, self.S, self.G,
                        p["adj_sum"], p["edge_count"], p["mask_sum"], p["rows"], p["mask_rows"], p["skipped"])

    def observe(self, adj, mask, group, hw) -> None:
        """The ``graph_observer`` of a ``CausalTransition``: (per-sample adjacency, mask or None, group or None, (h, w))."""
        self.hw = (int(hw[0]), int(hw[1]))
        self.update(adj, group, mask)

    def result(self) -> dict:
        """One device -> host copy.  ``adjacency_mean`` [G, S, S], ``edge_freq`` [G, S, S] (the share of a group's graphs with
        the edge above the threshold) and ``mask_mean`` [G, S], float64, NaN where a group has no rows (no masked rows);
        ``rows`` and ``mask_rows`` [G] int64, ``skipped``, ``threshold`` and ``hw``."""
        host = self._buffer().cpu().numpy()
        lay = self._layout()[0]
        G, S = self.G, self.S

        def part(k, dtype=np.int32):
            off, n = lay[k]
            return host[off:off + n].view(dtype)

        rows, mask_rows = part("rows").astype(np.int64), part("mask_rows").astype(np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            nan = np.float64("nan")
            r3 = rows.astype(np.float64).reshape(G, 1, 1)
            adjacency_mean = np.where(r3 > 0, part("adj_sum", np.float64).reshape(G, S, S) / r3, nan)
            edge_freq = np.where(r3 > 0, part("edge_count").reshape(G, S, S).astype(np.float64) / r3, nan)
            m2 = mask_rows.astype(np.float64).reshape(G, 1)
            mask_mean = np.where(m2 > 0, part("mask_sum", np.float64).reshape(G, S) / m2, nan)
        return {"adjacency_mean": adjacency_mean, "edge_freq": edge_freq, "mask_mean": mask_mean, "rows": rows,
                "mask_rows": mask_rows, "skipped": int(part("skipped")[0]), "threshold": self.threshold, "hw": self.hw}


def group_keys(G: int, names: Optional[Sequence[str]] = None) -> list:
    """``none`` and, for action i of A = G - 1, ``<factor>_<sign>`` by the rule of ``rollout.factor_names``: factor i % V, ``+``
    for i < V."""
    A = int(G) - 1
    if A < 2 or A % 2:
        raise ValueError(f"{G} groups are no intervention plus {A} actions, but actions come as factors in two directions")
    V = A // 2
    names = factor_names(A, names)
    return ["none"] + [f"{names[i % V]}_{'+' if i < V else '-'}" for i in range(A)]


def summarize(result: dict, names: Optional[Sequence[str]] = None) -> dict:
    """``GraphStats.result()`` -> {group key: {...}} (``group_keys``), ready for standard JSON.  Per group: ``rows``; ``edges``,
    the mean number of edges above the threshold per graph; ``density`` = edges / S^2; ``top_edges``, the ten strongest mean
    edges as [i, j, value], strongest first (ties: the lower (i, j) first); ``mask_node``, the node with the largest mean mask
    (the first of several), for a group that has a mask.  What a group without rows (without a mask) cannot say is None."""
    mean, freq, mask = (np.asarray(result[k], dtype=np.float64) for k in ("adjacency_mean", "edge_freq", "mask_mean"))
    rows = np.asarray(result["rows"], dtype=np.int64)
    G, S = mean.shape[0], mean.shape[1]
    if mean.shape != (G, S, S) or freq.shape != (G, S, S) or mask.shape != (G, S) or rows.shape != (G,):
        raise ValueError(f"not a GraphStats result: shapes {mean.shape}, {freq.shape}, {mask.shape}, {rows.shape}")
    out = {}
    for g, key in enumerate(group_keys(G, names)):
        rec = {"rows": int(rows[g]), "edges": None, "density": None, "top_edges": None, "mask_node": None}
        if rows[g] > 0:
            edges = float(freq[g].sum())
            flat = mean[g].reshape(-1)
            order = np.argsort(-flat, kind="stable")[:10]
            rec.update(edges=edges, density=edges / float(S * S), top_edges=[[int(i // S), int(i % S), float(flat[i])] for i in order])
        if not np.isnan(mask[g]).any():
            rec["mask_node"] = int(np.argmax(mask[g]))
        out[key] = rec
    return out


def _values_on_gpu(values, what: str) -> torch.Tensor:
    if not torch.is_tensor(values):
        values = torch.as_tensor(np.asarray(values))
        if not torch.cuda.is_available():
            raise RuntimeError(f"{what} runs on the GPU only: there is no CPU fallback")
        values = values.to(torch.device("cuda", torch.cuda.current_device()))
    values = _need_gpu(values, what)
    if values.dim() == 2:
        values = values.unsqueeze(0)
    if values.dim() != 3 or values.numel() == 0:
        raise ValueError(f"{what} takes values [M, H, W] (or one [H, W]), got {tuple(values.shape)}")
    return values.detach().to(torch.float32).contiguous()


def heatmap_u8(values, lo: float = 0.0, hi: float = 1.0, cell: int = 4, nrow: int = 8, padding: int = 2, scanlines: bool = False,
               pad_color=PAD_COLOR) -> torch.Tensor:
    """values [M, H, W] as the bytes of a sheet of M colour-mapped tiles, every value ``cell`` x ``cell`` pixels, on the values'
    device: [Hg, Wg, 3], or with ``scanlines`` [Hg, 1 + 3*Wg] (``imagegrid.make_grid_u8``'s layout for tiles of H*cell x W*cell).
    A value v takes ``colormap()[floor(t*255 + 0.5)]``, t = (clamp(v, lo, hi) - lo) / (hi - lo); NaN takes entry 0."""
    values = _values_on_gpu(values, "heatmap_u8")
    cell, nrow, padding = int(cell), int(nrow), int(padding)
    if cell < 1 or nrow < 1 or padding < 0 or not float(hi) > float(lo):
        raise ValueError(f"heatmap_u8 needs cell >= 1, nrow >= 1, padding >= 0 and hi > lo, got {cell}, {nrow}, {padding}, [{lo}, {hi}]")
    M, H, W = values.shape
    _, _, Hg, Wg = imagegrid.grid_geometry(M, H * cell, W * cell, nrow, padding)
    pitch = (1 if scanlines else 0) + 3 * Wg
    total = Hg * pitch
    out = torch.empty((total + 3) // 4 * 4, dtype=torch.uint8, device=values.device)
    table = np.ascontiguousarray(colormap())
    with torch.cuda.device(values.device):
        native.call("ctvae_heatmap_u8", values.data_ptr(), M, H, W, float(lo), float(hi), cell, nrow, padding, int(pad_color[0]),
                    int(pad_color[1]), int(pad_color[2]), table.ctypes.data, int(bool(scanlines)), out.data_ptr(), out.numel())
    return out[:total].view(Hg, pitch) if scanlines else out[:total].view(Hg, Wg, 3)


def save_heatmaps(values, path, lo: float = 0.0, hi: float = 1.0, cell: int = 4, nrow: int = 8, padding: int = 2,
                  pad_color=PAD_COLOR) -> None:
    """``heatmap_u8`` as a PNG file.  values: a GPU tensor, or a numpy array (it goes to the current device as float32)."""
    sheet = heatmap_u8(values, lo=lo, hi=hi, cell=cell, nrow=nrow, padding=padding, scanlines=True, pad_color=pad_color)
    height, pitch = sheet.shape
    data = imagegrid.png_bytes(sheet.cpu().numpy().tobytes(), (pitch - 1) // 3, height)
    with open(path, "wb") as f:
        f.write(data)


def model_nodes(model) -> int:
    """The node count S of a CTMCQVAE's latent graph: codebooks x the latent grid."""
    return int(model.codebooks) * int(model.nb_latents) ** 2


def collect_graphs(model, batches: Iterable, seed: int = 0, threshold: float = 0.5) -> GraphStats:
    """The base- and action-mode batches ``(x, labels, options)`` of a split through the model, their graphs accumulated by
    group.  Causal-mode batches are skipped: ``forward_transition`` runs ``forward_action`` once per HYPOTHESISED action, and
    those graphs belong to no action that was observed.  One forward and one launch per batch; nothing of the caller's run
    moves (module docstring)."""
    A = _need_ct(model, "collect_graphs")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("collect_graphs runs on the GPU only: there is no CPU fallback")
    stats = GraphStats(A + 1, model_nodes(model), dev, threshold)
    ct = model.ct_layer
    prev, ct.graph_observer = ct.graph_observer, stats.observe
    try:
        with eval_mode(model), seeded_torch_rng(seed, dev):
            for batch in batches:
                x, labels, opts = unpack_batch(batch)
                if batch_mode(opts, "base") not in ("base", "action"):
                    continue
                model(_need_gpu(x, "collect_graphs"), labels=labels, **opts)
    finally:
        ct.graph_observer = prev
    return stats
