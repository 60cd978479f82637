"""Reconstruction quality at validation: PSNR, SSIM and the worst images (``exp_params.recon_stats``).

Every model is trained to get the reconstruction right, and ``val_Reconstruction_Loss`` -- a batch-mean MSE -- cannot tell
"uniformly slightly blurry" from "sharp, except for 2 % of the images".  Here every validation image gets a record of its own:

* ``ReconStats`` -- per image ``mse``, ``mae``, ``max_err`` and the SSIM of Wang et al. 2004 (11-tap Gaussian window, sigma 1.5,
  valid positions only, C1 = (0.01 R)^2, C2 = (0.03 R)^2: skimage's ``structural_similarity(gaussian_weights=True, sigma=1.5,
  use_sample_covariance=False, data_range=R)``), float64 on the device from the fp32 pictures, plus a flag for a non-finite
  element (csrc/reconstat.hip: ``ctvae_recon_record``, one launch per batch), and a running set of the K worst images by SSIM
  with their pictures (``ctvae_recon_worst``, two launches per batch).  Nothing comes back to the host before ``result()``, which
  makes the one copy; the record buffer grows on the device without a synchronisation.
* ``summarize`` -- the records as the epoch's statistics, float64 numpy on the host; ``record`` -- as log entries.
* ``write_files`` -- the per-image arrays as an ``.npz`` and the worst images as a picture.
* ``recon_settings`` / ``refuses_model`` -- ``exp_params.recon_stats`` / ``recon_stats_range`` / ``recon_stats_worst`` and the models
  they are refused for.

The reference has none of this, so parity here is defined by this project: by the float64 restatement in tests/recon_checks.py.
There is no CPU path for the device parts.
"""
import numpy as np
import torch

from . import imagegrid
from . import kernels as K
from .evalrun import npz_bytes

RECON_DIR = "Recon"
DEFAULT_RANGE = 1.0
DEFAULT_WORST = 8
MAX_WORST = K.RECON_MAX_K
FIRST_CAPACITY = 1024
MULTI_SAMPLE_MODELS = ("IWAE", "MIWAE")
RECORD_KEYS = ("psnr", "ssim", "mae", "max_err", "psnr_p05", "ssim_p05", "psnr_min", "ssim_min", "rows", "nonfinite", "exact")


def recon_settings(params) -> tuple:
    """Validated ``(on, R, K)`` from ``recon_stats`` (a bool; absent: False), ``recon_stats_range`` (a float > 0, default 1.0) and
    ``recon_stats_worst`` (an int, 0 <= K <= 32, default 8; 0: no worst set) of ``params``.  The two dependent keys are refused
    without ``recon_stats``.  Anything else is a ValueError that names the key.  Off: ``(False, None, None)``."""
    on = params.get("recon_stats")
    if on is None:
        on = False
    if not isinstance(on, bool):
        raise ValueError(f"recon_stats must be true or false, got {on!r}")
    R, worst = params.get("recon_stats_range"), params.get("recon_stats_worst")
    if not on:
        for key, v in (("recon_stats_range", R), ("recon_stats_worst", worst)):
            if v is not None:
                raise ValueError(f"{key} is set without recon_stats: true (it would do nothing)")
        return False, None, None
    if R is None:
        R = DEFAULT_RANGE
    elif isinstance(R, bool) or not isinstance(R, float) or not (R > 0 and R < float("inf")):
        raise ValueError(f"recon_stats_range must be a float > 0 (the data range of the pictures), got {R!r}")
    if worst is None:
        worst = DEFAULT_WORST
    elif isinstance(worst, bool) or not isinstance(worst, int) or not 0 <= worst <= MAX_WORST:
        raise ValueError(f"recon_stats_worst must be an integer, 0 <= K <= {MAX_WORST}, got {worst!r}")
    return True, float(R), int(worst)


def refuses_model(model_or_class, name=None):
    """The refusal of ``recon_stats`` for a model whose ``forward`` hands out several reconstructions per image, by name; None
    for every other model."""
    from .models.iwae import MIWAE
    cls = model_or_class if isinstance(model_or_class, type) else type(model_or_class)
    if isinstance(cls, type) and issubclass(cls, MIWAE):
        return (f"recon_stats needs one reconstruction per image: {name if name is not None else cls.__name__} hands out "
                f"[B, S, C, H, W] samples ({', '.join(MULTI_SAMPLE_MODELS)} are not served)")
    return None


class ReconStats:
    """The per-image records of one validation epoch and its K worst images, on the device (include/ctvae_hip.h:
    ``ctvae_recon_record``, ``ctvae_recon_worst``)."""

    def __init__(self, device, R: float = DEFAULT_RANGE, K_worst: int = DEFAULT_WORST):
        self.device = torch.device(device)
        self.R, self.K = float(R), int(K_worst)
        if not 0 <= self.K <= MAX_WORST:
            raise ValueError(f"ReconStats keeps 0 <= K <= {MAX_WORST} worst images, got {K_worst}")
        self.consts = K.recon_consts(self.R)
        self.rows = 0                      # the host's count: every observe knows its B
        self.records = self.flags = None   # made by the first use: constructing one touches no device
        self.sides = None                  # the worst set's two sides; sides[self.cur] holds the state
        self.cur = 0
        self.shape = None                  # (C, S) of the pictures seen

    def reset(self) -> None:
        """Back to no rows and an empty worst set; the buffers are kept."""
        if self.device.type != "cuda":
            raise RuntimeError("ReconStats runs on the GPU only: there is no CPU fallback")
        self.rows = 0
        if self.sides is not None:
            self.sides[self.cur]["row"].fill_(-1)

    def _reserve(self, n: int) -> None:
        """Room for n rows: a new buffer and a copy of the old rows, all on the device and in stream order."""
        cap = 0 if self.flags is None else self.flags.numel()
        if n <= cap:
            return
        new_cap = max(FIRST_CAPACITY, cap)
        while new_cap < n:
            new_cap *= 2
        records = torch.zeros(new_cap, 4, dtype=torch.float64, device=self.device)
        flags = torch.zeros(new_cap, dtype=torch.int32, device=self.device)
        if self.rows:
            records[:self.rows].copy_(self.records[:self.rows])
            flags[:self.rows].copy_(self.flags[:self.rows])
        self.records, self.flags = records, flags

    def observe(self, recons: torch.Tensor, target: torch.Tensor) -> None:
        """Add the pairs of one batch, logical [B, C, S, S] fp32 device tensors: one launch, and two more with a worst set; no
        host synchronisation."""
        for t in (recons, target):
            if torch.is_tensor(t) and not t.is_cuda:
                raise RuntimeError("ReconStats runs on the GPU only: there is no CPU fallback")
        if self.device.type != "cuda":
            raise RuntimeError("ReconStats runs on the GPU only: there is no CPU fallback")
        if torch.is_tensor(recons) and recons.dim() == 4:
            shape = (recons.size(1), recons.size(2))
            if self.shape is not None and shape != self.shape:
                raise ValueError(f"ReconStats.observe: pictures changed from C, S = {self.shape} to {shape} within one accumulator")
        with torch.cuda.device(self.device):
            B = recons.size(0) if torch.is_tensor(recons) and recons.dim() == 4 else 0
            self._reserve(self.rows + B)
            a, b = K.recon_record(recons, target, self.consts, self.records, self.flags, self.rows)
            if self.shape is None:
                self.shape = (a.size(3), a.size(1))
            if self.K > 0 and B > 0:
                if self.sides is None:
                    self.sides = [K.recon_worst_state(self.K, a.size(1), a.size(3), self.device) for _ in range(2)]
                old, new = self.sides[self.cur], self.sides[1 - self.cur]
                K.recon_worst(old, new, self.records, self.flags, self.rows, a, b)
                self.cur = 1 - self.cur
            self.rows += B

    def result(self) -> dict:
        """The epoch on the host, by ONE device -> host copy: ``records`` float64 [rows, 4] (``kernels.RECON_COLUMNS``), ``flags``
        int32 [rows], ``worst_rows`` int32 [k] and ``worst_ssim`` float64 [k], the k <= K filled slots, worst first; and, still on
        the device, ``worst_recons`` / ``worst_target`` [k, C, S, S] (views of the NHWC slots)."""
        n, Kw = self.rows, self.K if self.sides is not None else 0
        out = {"records": np.zeros((0, 4), np.float64), "flags": np.zeros(0, np.int32), "worst_rows": np.zeros(0, np.int32),
               "worst_ssim": np.zeros(0, np.float64), "worst_recons": None, "worst_target": None, "R": self.R}
        if n == 0:
            return out
        parts = [self.records[:n].reshape(-1).view(torch.uint8), self.flags[:n].view(torch.uint8)]
        side = self.sides[self.cur] if Kw else None
        if Kw:
            parts += [side["ssim"].view(torch.uint8), side["row"].view(torch.uint8)]
        host = torch.cat(parts).cpu().numpy()
        o = 0
        out["records"] = host[o:o + 32 * n].view(np.float64).reshape(n, 4).copy()
        o += 32 * n
        out["flags"] = host[o:o + 4 * n].view(np.int32).copy()
        o += 4 * n
        if Kw:
            ssim = host[o:o + 8 * Kw].view(np.float64).copy()
            rows = host[o + 8 * Kw:o + 12 * Kw].view(np.int32).copy()
            k = int((rows >= 0).sum())                   # the filled slots lead
            out.update(worst_rows=rows[:k], worst_ssim=ssim[:k], worst_recons=side["a"][:k].permute(0, 3, 1, 2),
                       worst_target=side["b"][:k].permute(0, 3, 1, 2))
        return out


def summarize(records, flags, R: float = DEFAULT_RANGE) -> dict:
    """The records as statistics, float64 numpy, no GPU.  Over the images whose flag is 0:

    * ``ssim``, ``mae`` the means; ``max_err`` the maximum; ``ssim_p05`` the 5th percentile (numpy's linear interpolation),
      ``ssim_min``
    * ``psnr`` the mean of 10 log10(R^2 / mse_i) over the images with mse_i > 0, ``psnr_p05``, ``psnr_min`` likewise
    * ``exact``, the images with mse_i == 0 (left out of the PSNR statistics only); ``nonfinite``, the flagged images (left out
      of everything else); ``rows``

    A statistic with no image to stand on is left out, never written as NaN or inf."""
    records = np.asarray(records, dtype=np.float64).reshape(-1, 4)
    flags = np.asarray(flags).reshape(-1)
    if len(flags) != len(records):
        raise ValueError(f"summarize: {len(records)} records and {len(flags)} flags")
    ok = records[flags == 0]
    out = {"rows": int(len(flags)), "nonfinite": int((flags != 0).sum()), "exact": int((ok[:, 0] == 0).sum())}
    if len(ok) == 0:
        return out
    ssim = ok[:, 3]
    out.update(ssim=float(ssim.mean()), mae=float(ok[:, 1].mean()), max_err=float(ok[:, 2].max()),
               ssim_p05=float(np.percentile(ssim, 5)), ssim_min=float(ssim.min()))
    mse = ok[ok[:, 0] > 0, 0]
    if len(mse):
        psnr = 10.0 * np.log10(float(R) * float(R) / mse)
        out.update(psnr=float(psnr.mean()), psnr_p05=float(np.percentile(psnr, 5)), psnr_min=float(psnr.min()))
    return out


def record(res: dict, prefix: str = "val_recon_", suffix: str = "") -> dict:
    """The scalars of ``summarize`` as log entries ``<prefix><key><suffix>``, ``psnr`` -> ``val_recon_psnr``; what is undefined is
    left out."""
    return {prefix + k + suffix: res[k] for k in RECORD_KEYS if k in res}


def write_files(result: dict, npz_path, png_path=None) -> None:
    """``ReconStats.result()`` as files: the per-image ``mse``, ``mae``, ``max_err``, ``ssim`` (float64), ``nonfinite`` (int32) and
    ``worst_rows`` as an ``.npz`` whose bytes depend on the arrays alone, and -- with ``png_path`` and at least one worst image --
    the worst targets (top row) over their reconstructions (bottom row), worst first, through ``imagegrid.save_image`` with the
    arguments ``sample_images`` uses and one column per image."""
    rec = result["records"]
    arrays = {name: np.ascontiguousarray(rec[:, i]) for i, name in enumerate(K.RECON_COLUMNS)}
    arrays["nonfinite"] = np.asarray(result["flags"], dtype=np.int32)
    arrays["worst_rows"] = np.asarray(result["worst_rows"], dtype=np.int32)
    with open(npz_path, "wb") as f:
        f.write(npz_bytes(arrays))
    k = len(result["worst_rows"])
    if png_path is not None and k > 0:
        sheet = torch.cat([result["worst_target"], result["worst_recons"]])      # [2k, C, S, S]: targets, then reconstructions
        imagegrid.save_image(sheet, png_path, normalize=True, nrow=k)
