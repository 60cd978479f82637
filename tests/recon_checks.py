"""Float64 numpy restatement of the reconstruction statistics (``exp_params.recon_stats``; csrc/reconstat.hip, reconstats.py), from
the definition: per image the mean squared, mean absolute and largest absolute error, and the SSIM of Wang et al. 2004 as a
DIRECT 2-D windowed sum over the valid positions -- the 11 x 11 window G = g (x) g is laid over every position and multiplied out,
nothing is separated into passes -- so that it shares no structure with the kernel.  Pictures are [B, C, S, S] arrays."""
import numpy as np

TAPS = 11
SIGMA = 1.5


def window2d():
    t = np.arange(TAPS, dtype=np.float64)
    g = np.exp(-((t - 5.0) ** 2) / (2.0 * SIGMA ** 2))
    g = g / g.sum()
    return np.outer(g, g)


def ssim_map(a, b, R):
    """The SSIM map of two [S, S] float64 planes: [S - 10, S - 10]."""
    G = window2d()
    c1, c2 = (0.01 * R) ** 2, (0.03 * R) ** 2
    # [W, W, 11, 11]: the 11 x 11 patch under every valid position (a view, nothing is summed yet)
    pa = np.lib.stride_tricks.sliding_window_view(a, (TAPS, TAPS))
    pb = np.lib.stride_tricks.sliding_window_view(b, (TAPS, TAPS))
    mu_a, mu_b = (G * pa).sum(axis=(-2, -1)), (G * pb).sum(axis=(-2, -1))
    s_aa = (G * pa * pa).sum(axis=(-2, -1)) - mu_a * mu_a
    s_bb = (G * pb * pb).sum(axis=(-2, -1)) - mu_b * mu_b
    s_ab = (G * pa * pb).sum(axis=(-2, -1)) - mu_a * mu_b
    return ((2 * mu_a * mu_b + c1) * (2 * s_ab + c2)) / ((mu_a * mu_a + mu_b * mu_b + c1) * (s_aa + s_bb + c2))


def ref_records(a, b, R=1.0):
    """(records [B, 4] float64: mse, mae, max, ssim; flags [B] int32) of the pairs a, b [B, C, S, S]."""
    a32, b32 = np.asarray(a), np.asarray(b)
    a, b = a32.astype(np.float64), b32.astype(np.float64)
    B, C = a.shape[:2]
    rec = np.zeros((B, 4), dtype=np.float64)
    flags = np.zeros(B, dtype=np.int32)
    for i in range(B):
        flags[i] = 0 if (np.isfinite(a[i]).all() and np.isfinite(b[i]).all()) else 1
        with np.errstate(invalid="ignore", over="ignore"):
            d = a[i] - b[i]
            rec[i, 0] = (d * d).mean()
            rec[i, 1] = np.abs(d).mean()
            rec[i, 2] = np.abs(d).max()
            rec[i, 3] = np.mean([ssim_map(a[i, c], b[i, c], R).mean() for c in range(C)]) if not flags[i] else np.nan
    return rec, flags


def ref_worst(stream_of_batches, K, R=1.0):
    """The K worst images of a stream of (a, b) batches by a sort of the whole stream on (ssim ascending, global row ascending);
    non-finite images never enter.  Returns (rows [K] int32, -1 where empty; ssim [K]; a [K, C, S, S]; b likewise, zero where
    empty)."""
    rows, pics = [], []
    n = 0
    for a, b in stream_of_batches:
        rec, flags = ref_records(a, b, R)
        for i in range(len(flags)):
            if not flags[i]:
                rows.append((rec[i, 3], n + i))
                pics.append((np.asarray(a)[i], np.asarray(b)[i]))
        n += len(flags)
    order = sorted(range(len(rows)), key=lambda j: rows[j])[:K]
    shape = np.asarray(stream_of_batches[0][0]).shape[1:]
    out_rows = np.full(K, -1, dtype=np.int32)
    out_ssim = np.zeros(K, dtype=np.float64)
    out_a = np.zeros((K,) + shape, dtype=np.float32)
    out_b = np.zeros((K,) + shape, dtype=np.float32)
    for s, j in enumerate(order):
        out_ssim[s], out_rows[s] = rows[j]
        out_a[s], out_b[s] = pics[j]
    return out_rows, out_ssim, out_a, out_b


def ref_summary(rec, flags, R=1.0):
    """The epoch scalars from records and flags, from the issue's definitions; what has no image to stand on is left out."""
    rec, flags = np.asarray(rec, dtype=np.float64), np.asarray(flags)
    out = {"rows": int(len(flags)), "nonfinite": int((flags != 0).sum())}
    ok = rec[flags == 0]
    out["exact"] = int((ok[:, 0] == 0).sum()) if len(ok) else 0
    if len(ok):
        out.update(ssim=float(ok[:, 3].mean()), mae=float(ok[:, 1].mean()), max_err=float(ok[:, 2].max()),
                   ssim_p05=float(np.percentile(ok[:, 3], 5)), ssim_min=float(ok[:, 3].min()))
        pos = ok[ok[:, 0] > 0, 0]
        if len(pos):
            psnr = 10.0 * np.log10(R * R / pos)
            out.update(psnr=float(psnr.mean()), psnr_p05=float(np.percentile(psnr, 5)), psnr_min=float(psnr.min()))
    return out


def pictures(seed, B, C, S, kind="unit"):
    """A pair of [B, C, S, S] float32 batches: ``unit`` in [0, 1] (the target uniform, the reconstruction a noisy copy clipped
    back), ``randn`` standard normal and unrelated."""
    rng = np.random.default_rng(seed)
    if kind == "unit":
        b = rng.random((B, C, S, S))
        a = np.clip(b + 0.1 * rng.standard_normal((B, C, S, S)), 0.0, 1.0)
    else:
        a, b = rng.standard_normal((B, C, S, S)), rng.standard_normal((B, C, S, S))
    return a.astype(np.float32), b.astype(np.float32)
