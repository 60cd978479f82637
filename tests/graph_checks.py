"""Shared by the causal-graph tests (no GPU): float64 numpy restatements of csrc/graphstat.hip -- ``ref_accumulate`` adds the rows
of a batch one at a time in ascending order, which is the kernel's contract to the bit (float32 -> float64 is exact, a float64
add rounds once, and the order is fixed); ``ref_heatmap_bytes`` is the sheet of ``ctvae_heatmap_u8``, exact as long as every
value keeps ``MARGIN`` away from a rounding boundary of t*255 + 0.5, which it asserts -- and seeded input builders."""
import numpy as np

from tests import grid_checks as G

MARGIN = G.MARGIN


def new_state(Gn, S):
    """The accumulators of ctvae_graph_accumulate, zeroed."""
    return {"adj_sum": np.zeros((Gn, S, S), np.float64), "edge_count": np.zeros((Gn, S, S), np.int32),
            "mask_sum": np.zeros((Gn, S), np.float64), "rows": np.zeros(Gn, np.int32), "mask_rows": np.zeros(Gn, np.int32),
            "skipped": np.zeros(1, np.int32)}


def ref_accumulate(state, adj, group=None, mask=None, threshold=0.5):
    """Adds adj [B,S,S] float32 (group [B] integers or None = all 0, mask [B,S] float32 or None) into ``state`` IN PLACE, one
    row at a time in ascending row order; returns it."""
    adj = np.asarray(adj)
    assert adj.dtype == np.float32 and adj.ndim == 3 and adj.shape[1] == adj.shape[2]
    B = adj.shape[0]
    Gn = state["rows"].shape[0]
    group = np.zeros(B, np.int64) if group is None else np.asarray(group).astype(np.int64)
    thr = np.float32(threshold)
    if mask is not None:
        mask = np.asarray(mask)
        assert mask.dtype == np.float32 and mask.shape == (B, adj.shape[1])
    for b in range(B):
        g = int(group[b])
        if g < 0 or g >= Gn:
            state["skipped"][0] += 1
            continue
        state["adj_sum"][g] = state["adj_sum"][g] + adj[b].astype(np.float64)
        state["edge_count"][g] += (adj[b] > thr)                  # strict, in float32; NaN does not count
        state["rows"][g] += 1
        if mask is not None:
            state["mask_sum"][g] = state["mask_sum"][g] + mask[b].astype(np.float64)
            state["mask_rows"][g] += 1
    return state


def result_of(state):
    """``GraphStats.result()``'s three mean arrays from a state (NaN for a group without rows / without masked rows)."""
    rows = state["rows"].astype(np.float64)
    mrows = state["mask_rows"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        nan = np.float64("nan")
        mean = np.where(rows[:, None, None] > 0, state["adj_sum"] / rows[:, None, None], nan)
        freq = np.where(rows[:, None, None] > 0, state["edge_count"].astype(np.float64) / rows[:, None, None], nan)
        mask = np.where(mrows[:, None] > 0, state["mask_sum"] / mrows[:, None], nan)
    return mean, freq, mask


def table_index(values, lo=0.0, hi=1.0, margin=MARGIN, nudge=0.0):
    """The colour-table index of every value: floor(t*255 + 0.5), t = (clamp(v, lo, hi) - lo) / (hi - lo), NaN -> 0.  Asserts
    that no t*255 + 0.5 lies within ``margin`` of an integer (float32 evaluation then cannot land on another index).
    nudge: added to t*255 + 0.5 before the floor (``sheet_matches``)."""
    v = np.asarray(values)
    assert v.dtype == np.float32 or margin == 0.0
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    assert hi > lo
    v = v.astype(np.float64)
    v = np.where(np.isnan(v), lo, np.clip(v, lo, hi))
    t = (v - lo) / (hi - lo) * 255.0 + 0.5
    dist = np.abs(t - np.round(t))
    assert dist.size == 0 or dist.min() >= margin, f"a value sits {dist.min():.3g} from a rounding boundary"
    return np.clip(np.floor(t + nudge), 0, 255).astype(np.int64)


def ref_heatmap_bytes(values, table, lo=0.0, hi=1.0, cell=4, nrow=8, padding=2, pad_color=(0, 0, 0), scanlines=True, margin=MARGIN,
                      nudge=0.0):
    """values [M,H,W] float32 -> uint8 [Hg, 1 + 3*Wg] (scanlines: a zero first in every row) or [Hg, 3*Wg]."""
    values = np.asarray(values)
    assert values.ndim == 3
    table = np.asarray(table)
    assert table.shape == (256, 3) and table.dtype == np.uint8
    M, H, W = values.shape
    idx = table_index(values, lo, hi, margin, nudge)
    tiles = table[idx]                                                        # [M, H, W, 3]
    tiles = np.repeat(np.repeat(tiles, cell, axis=1), cell, axis=2)           # every value cell x cell pixels
    Hc, Wc = H * cell, W * cell
    xmaps, ymaps, Hg, Wg = G.geometry(M, Hc, Wc, nrow, padding)
    sheet = np.empty((Hg, Wg, 3), np.uint8)
    sheet[:] = np.asarray(pad_color, np.uint8)
    for k in range(M):
        r0, c0 = (k // xmaps) * (Hc + padding) + padding, (k % xmaps) * (Wc + padding) + padding
        sheet[r0:r0 + Hc, c0:c0 + Wc] = tiles[k]
    flat = sheet.reshape(Hg, 3 * Wg)
    if scanlines:
        flat = np.concatenate([np.zeros((Hg, 1), np.uint8), flat], axis=1)
    return flat


SLACK = 1e-3          # see sheet_matches


def sheet_matches(img, values, table, **kw):
    """Is img uint8 [Hg, Wg, 3] the sheet of ``values`` (float64 means that a model produced, so they keep no margin)?  The
    kernel casts to float32 and forms t*255 + 0.5 in four float32 operations on numbers of at most 256: it is off by less than
    6 * 2^-24 * 256 < 1e-4, so its index is floor(t*255 + 0.5 + d) for some |d| < SLACK.  Every pixel must therefore be the
    pixel of the sheet nudged down by SLACK or of the sheet nudged up -- borders and empty cells are the same in both."""
    values = np.asarray(values, dtype=np.float64)
    down = ref_heatmap_bytes(values, table, scanlines=False, margin=0.0, nudge=-SLACK, **kw).reshape(img.shape)
    up = ref_heatmap_bytes(values, table, scanlines=False, margin=0.0, nudge=SLACK, **kw).reshape(img.shape)
    ok = (img == down).all(axis=-1) | (img == up).all(axis=-1)
    return bool(ok.all()), int((~ok).sum()), int(((down != up).any(axis=-1)).sum())


def heat_inputs(seed, shape, lo=0.0, hi=1.0):
    """float32 [M,H,W] as ``grid_checks.grid_inputs`` builds them: every element aims at a table index k in [0, 256) with an
    offset in [0.1, 0.9] inside it, so that t*255 + 0.5 = k + f; then a share is moved below lo, above hi and to NaN."""
    x = G.grid_inputs(seed, (shape[0], 1) + tuple(shape[1:]), lo=lo, hi=hi, pin=False)[:, 0]
    rng = np.random.default_rng(seed + 1)
    flat = x.reshape(-1)
    n = flat.size
    if n >= 8:
        pick = rng.choice(n, size=max(3, n // 16) * 3, replace=False).reshape(3, -1)
        flat[pick[0]] = np.float32(lo - 0.75 * (hi - lo))
        flat[pick[1]] = np.float32(hi + 2.5 * (hi - lo))
        flat[pick[2]] = np.float32("nan")
    return x


def accumulate_inputs(seed, B, S, Gn, groups=None, on_threshold=True, threshold=0.5):
    """adj [B,S,S] in [0, 1) spread over 40 binary orders of magnitude -- so that the float64 adds really round and a sum in
    another order would show -- with a share of the values EXACTLY on the threshold (they do not count), mask [B,S] of zeros
    and ones, group [B] in [0, Gn) (or ``groups``)."""
    rng = np.random.default_rng(seed)
    expo = np.where(rng.random((B, S, S)) < 0.5, 0, rng.integers(0, 40, size=(B, S, S)))          # half of them of order 1
    adj = (rng.random((B, S, S)) * 2.0 ** -expo.astype(np.float64)).astype(np.float32)
    if on_threshold:
        adj[rng.random((B, S, S)) < 0.1] = np.float32(threshold)
    mask = (rng.random((B, S)) < 0.3).astype(np.float32)
    group = rng.integers(0, Gn, size=B).astype(np.int32) if groups is None else np.asarray(groups, np.int32)
    assert group.shape == (B,)
    return adj, group, mask
