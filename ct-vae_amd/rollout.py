"""Applying actions with a trained CT-MCQ-VAE: the reference's only inference workflow, its ``apply_action.ipynb`` notebook.

* ``action_rollout`` / ``save_rollout_sheet`` -- cell 6: one image, every action (each factor, both directions) applied
  repeatedly, the pictures saved.  The notebook saves every frame on its own with ``normalize=True``; the sheet is one PNG whose
  tiles are scaled the same way (``imagegrid.save_image(..., scale_each=True)``).
* ``rollout_accuracy`` -- cell 7: how often the causal mode recognises the action that was just applied, per action and step.
* ``split_accuracy`` -- cell 9: causal accuracy over the causal-mode batches of a split.

The model reports ``causal_acc`` / ``causal_nodir_acc`` only as batch means; the breakdown by action is a segmented count,
``ActionHits`` over csrc/acteval.hip, which accumulates on the device with no host synchronisation per batch.  Action index
``i`` of ``A = 2 V`` means factor ``i % V``, direction ``+`` for ``i < V`` and ``-`` otherwise (cells 5-7).

Every model call runs under ``evalrun.eval_mode`` (eval + no_grad, training flags restored) and
``evalrun.seeded_torch_rng``: no BatchNorm statistic, no parameter epoch and no torch generator of the caller's run moves.
There is no CPU path: tensors must be on the GPU.
"""
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import imagegrid, native
from .evalrun import batch_mode, eval_mode, seeded_torch_rng, unpack_batch
from .models.ct_mcq_vae import CTMCQVAE


def _need_ct(model, what: str) -> int:
    if not isinstance(model, CTMCQVAE):
        raise TypeError(f"{what} needs a CTMCQVAE (actions are its causal-transition layer's), got {type(model).__name__}")
    return int(model.ct_layer.action_dim)


def _need_gpu(t: torch.Tensor, what: str) -> torch.Tensor:
    if not torch.is_tensor(t):
        raise TypeError(f"{what} takes a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{what} runs on the GPU only: there is no CPU fallback")
    return t


def factor_names(A: int, names: Optional[Sequence[str]] = None) -> List[str]:
    """The V = A / 2 factor names: ``names`` checked for its length, or ``action0`` ..."""
    V = A // 2
    if names is None:
        return [f"action{i}" for i in range(V)]
    names = [str(n) for n in names]
    if len(names) != V:
        raise ValueError(f"{A} actions are {V} factors in two directions, but {len(names)} names were given: {names}")
    return names


def configured_factor_names(mp: dict, dp: dict, given: Optional[str] = None) -> Optional[List[str]]:
    """The factor names a command hands ``factor_names``: ``given`` (its comma-separated ``--factor-names``), else
    ``data_params.hbm_factor_names``, else None.  A ValueError names an odd ``model_params.action_dim`` or a wrong count."""
    A = int(mp.get('action_dim', 0))
    if A < 2 or A % 2:
        raise ValueError(f"model_params.action_dim must be even and at least 2, got {mp.get('action_dim')!r}")
    if given is not None:
        names, src = [n.strip() for n in given.split(",")], "--factor-names"
    else:
        names, src = dp.get('hbm_factor_names'), "data_params.hbm_factor_names"
    if names is not None and len(names) != A // 2:
        raise ValueError(f"{src} has {len(names)} names, but action_dim {A} means {A // 2} factors")
    return names


def summarize(counts, names: Optional[Sequence[str]] = None) -> dict:
    """counts [A, 3] (rows, directed hits, direction-agnostic hits per action) -> the result dict: ``causal_acc`` and
    ``causal_nodir_acc`` over all rows, ``<name>_<sign>_causal_acc`` / ``<name>_<sign>_causal_nodir_acc`` per action, and ``n``,
    the rows per action.  A rate over no rows is None (never NaN: the dict goes into standard JSON)."""
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim != 2 or c.shape[1] != 3 or c.shape[0] < 2 or c.shape[0] % 2:
        raise ValueError(f"counts must be [A, 3] with A even, got {c.shape}")
    A = c.shape[0]
    V = A // 2
    names = factor_names(A, names)

    def rate(hits, rows):
        return float(hits) / float(rows) if rows > 0 else None

    tot = c.sum(axis=0)
    res = {"causal_acc": rate(tot[1], tot[0]), "causal_nodir_acc": rate(tot[2], tot[0])}
    for i in range(A):
        key = f"{names[i % V]}_{'+' if i < V else '-'}"
        res[key + "_causal_acc"] = rate(c[i, 1], c[i, 0])
        res[key + "_causal_nodir_acc"] = rate(c[i, 2], c[i, 0])
    res["n"] = [int(v) for v in c[:, 0]]
    return res


class ActionHits:
    """Per-action hit counts [A, 3] int32 on the device (include/ctvae_hip.h: ctvae_action_hits)."""

    def __init__(self, A: int, device):
        self.A = int(A)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ActionHits runs on the GPU only: there is no CPU fallback")
        self._counts = None                     # made by the first update: constructing one touches no device

    def _buffer(self) -> torch.Tensor:
        if self._counts is None:
            self._counts = torch.zeros(self.A, 3, dtype=torch.int32, device=self.device)
        return self._counts

    def update(self, probas: torch.Tensor, action: torch.Tensor) -> None:
        """Add the rows of probas / action [N, A] (forward_causal's outputs 0 and 1).  One launch, no host sync."""
        probas, action = _need_gpu(probas, "ActionHits.update"), _need_gpu(action, "ActionHits.update")
        if probas.dim() != 2 or probas.shape != action.shape or probas.size(1) != self.A:
            raise ValueError(f"ActionHits.update takes two [N, {self.A}] tensors, got {tuple(probas.shape)} and {tuple(action.shape)}")
        counts = self._buffer()
        if probas.size(0) == 0:
            return
        p = probas.detach().to(device=self.device, dtype=torch.float32).contiguous()
        a = action.detach().to(device=self.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(self.device):
            native.call("ctvae_action_hits", p.data_ptr(), a.data_ptr(), p.size(0), self.A, counts.data_ptr())

    def counts(self) -> np.ndarray:
        """[A, 3] int64 on the host: one device -> host copy."""
        return self._buffer().cpu().numpy().astype(np.int64)

    def result(self, names: Optional[Sequence[str]] = None) -> dict:
        return summarize(self.counts(), names)


def _one_hot_rows(a: int, rows: int, A: int, device) -> torch.Tensor:
    t = torch.zeros(rows, A, device=device)
    t[:, a] = 1.0
    return t


def action_rollout(model, image: torch.Tensor, steps: int = 5, seed: int = 0) -> torch.Tensor:
    """frames [steps + 1, A, 3, H, W]: frame 0 is ``image`` ([3,H,W] or [1,3,H,W]) A times; frame s is action a applied to
    frame s - 1's row a -- ``model(frame, labels=None, mode=["action"] * A, action=eye(A), input_y=frame)[0]``, one forward of
    A rows per step, the notebook's call."""
    A = _need_ct(model, "action_rollout")
    image = _need_gpu(image, "action_rollout")
    if image.dim() == 3:
        image = image.unsqueeze(0)
    if image.dim() != 4 or image.size(0) != 1:
        raise ValueError(f"action_rollout takes one image [3,H,W] or [1,3,H,W], got {tuple(image.shape)}")
    dev = image.device
    frames = [image.detach().float().expand(A, -1, -1, -1).contiguous()]
    eye = torch.eye(A, device=dev)
    with eval_mode(model), seeded_torch_rng(seed, dev):
        for _ in range(int(steps)):
            cur = frames[-1]
            frames.append(model(cur, labels=None, mode=["action"] * A, action=eye, input_y=cur)[0].detach())
    return torch.stack(frames)


def save_rollout_sheet(frames: torch.Tensor, path) -> None:
    """One PNG of frames [S + 1, A, 3, H, W]: a row per action, the input and steps 1 ... S as columns, every tile scaled by its
    own range as a picture saved alone with ``normalize=True`` is."""
    frames = _need_gpu(frames, "save_rollout_sheet")
    if frames.dim() != 5:
        raise ValueError(f"save_rollout_sheet takes frames [S+1, A, C, H, W], got {tuple(frames.shape)}")
    S1, A, C, H, W = frames.shape
    imagegrid.save_image(frames.transpose(0, 1).reshape(-1, C, H, W), path, nrow=S1, normalize=True, scale_each=True)


def rollout_accuracy(model, x: torch.Tensor, steps: int = 1, names: Optional[Sequence[str]] = None, seed: int = 0) -> List[dict]:
    """One result dict (``summarize``) per step over the batch x [B,3,H,W].  The call order is part of the contract -- it makes
    the result reproducible against a plain loop and gives every forward the notebook's batch shape: for each step, for each
    action a ascending,
        out    = model(x_a, mode action, action = onehot(a) B times, input_y = x_a)[0]
        probas = model(x,   mode causal, action = the same,          input_y = out)[0]
        hits.update(probas, action);  x_a = out
    with x_a = x before the first step."""
    A = _need_ct(model, "rollout_accuracy")
    x = _need_gpu(x, "rollout_accuracy")
    names = factor_names(A, names)
    dev, B = x.device, x.size(0)
    cur = [x] * A
    hits = [ActionHits(A, dev) for _ in range(int(steps))]
    with eval_mode(model), seeded_torch_rng(seed, dev):
        for s in range(int(steps)):
            for a in range(A):
                action = _one_hot_rows(a, B, A, dev)
                out = model(cur[a], labels=None, mode=["action"] * B, action=action, input_y=cur[a])[0]
                probas = model(x, labels=None, mode=["causal"] * B, action=action, input_y=out)[0]
                hits[s].update(probas, action)
                cur[a] = out
    return [h.result(names) for h in hits]


def split_accuracy(model, batches: Iterable, names: Optional[Sequence[str]] = None, seed: int = 0) -> dict:
    """Causal accuracy by action over the causal-mode batches ``(x, labels, options)`` of a split; other modes are skipped.
    One forward and one count launch per batch, one device -> host copy at the end."""
    A = _need_ct(model, "split_accuracy")
    names = factor_names(A, names)
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("split_accuracy runs on the GPU only: there is no CPU fallback")
    hits = ActionHits(A, dev)
    with eval_mode(model), seeded_torch_rng(seed, dev):
        for batch in batches:
            x, labels, opts = unpack_batch(batch)
            if batch_mode(opts) != "causal":
                continue
            out = model(_need_gpu(x, "split_accuracy"), labels=labels, **opts)
            hits.update(out[0], out[1])
    return hits.result(names)
