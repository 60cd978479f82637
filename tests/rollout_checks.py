"""Shared by the rollout tests (no GPU, no test functions): numpy restatements of csrc/acteval.hip (per-action hit counts) and of
the per-image grid (imggrid.hip: ctvae_image_grid_each_u8), the latter as tests/grid_checks.py's batch restatement applied image
by image -- with its own allowance for values near a rounding boundary, asserted there per image."""
import warnings

import numpy as np

from tests import grid_checks as G


def argmax_ref(row) -> int:
    """torch.argmax of one row: the first maximal value wins, NaN counts as maximal and the first NaN wins."""
    row = np.asarray(row)
    nan = np.flatnonzero(np.isnan(row))
    if nan.size:
        return int(nan[0])
    best = 0
    for i in range(1, row.size):
        if row[i] > row[best]:
            best = i
    return best


def hits_ref(probas, action) -> np.ndarray:
    """probas, action [N, A] -> int64 [A, 3]: rows, directed hits (p == a), direction-agnostic hits (p % V == a % V) per
    action a = argmax(action row), with p = argmax(probas row) and V = A / 2."""
    probas, action = np.asarray(probas), np.asarray(action)
    assert probas.ndim == 2 and probas.shape == action.shape and probas.shape[1] % 2 == 0
    A = probas.shape[1]
    V = A // 2
    counts = np.zeros((A, 3), dtype=np.int64)
    for pr, ar in zip(probas, action):
        a, p = argmax_ref(ar), argmax_ref(pr)
        counts[a, 0] += 1
        counts[a, 1] += int(p == a)
        counts[a, 2] += int(p % V == a % V)
    return counts


def grid_each_ref(x, nrow=8, padding=2, pad_value=0.0, scanlines=False) -> np.ndarray:
    """make_grid(normalize=True, scale_each=True) as bytes: the frame (borders, empty cells, filter bytes) is G.ref_grid_bytes of
    a batch of zeros, every tile G.ref_grid_bytes(normalize=True) of that image alone (its own minimum and maximum; an all-NaN
    image is all byte 0).  uint8 [Hg, 3*Wg] or, with scanlines, [Hg, 1 + 3*Wg]."""
    x = np.asarray(x)
    N, C, H, W = x.shape
    xmaps, ymaps, Hg, Wg = G.geometry(N, H, W, nrow, padding)
    grid = G.ref_grid_bytes(np.zeros_like(x), nrow=nrow, padding=padding, pad_value=pad_value).reshape(Hg, Wg, 3).copy()
    for k in range(N):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)          # numpy's "All-NaN slice" for an image without a range
            tile = G.ref_grid_bytes(x[k:k + 1], nrow=1, padding=0, normalize=True)
        r0, c0 = (k // xmaps) * (H + padding) + padding, (k % xmaps) * (W + padding) + padding
        grid[r0:r0 + H, c0:c0 + W, :] = tile.reshape(H, W, 3)
    flat = grid.reshape(Hg, 3 * Wg)
    if scanlines:
        flat = np.concatenate([np.zeros((Hg, 1), dtype=np.uint8), flat], axis=1)
    return flat


def each_inputs(seed, shape) -> np.ndarray:
    """float32 [N,C,H,W] for the per-image grid: image k is G.grid_inputs over its own, clearly different range (so every
    v*255 + 0.5 keeps G.MARGIN from an integer under ITS range, and one element is its lo, one its hi).  Image 0 also has NaN
    pixels (none of them its lo or hi); with N >= 2 image 1 is constant (hi - lo < 1e-5), with N >= 3 image 2 is all NaN."""
    N = shape[0]
    rng = np.random.default_rng(seed)
    x = np.empty(shape, dtype=np.float32)
    for k in range(N):
        lo = -3.0 + 0.75 * (k % 7)
        hi = lo + 0.5 + 1.25 * ((k * 5) % 6)
        x[k] = G.grid_inputs(seed * 1000 + k, (1,) + tuple(shape[1:]), lo=lo, hi=hi)[0]
    flat = x[0].reshape(-1)
    free = np.flatnonzero((flat != flat.min()) & (flat != flat.max()))
    flat[rng.choice(free, size=min(5, free.size), replace=False)] = np.nan
    if N >= 2:
        x[1] = 0.37
    if N >= 3:
        x[2] = np.nan
    return x
