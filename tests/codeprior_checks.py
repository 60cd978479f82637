"""Float64 NumPy restatement of csrc/codeprior.hip and ctvae_amd/codeprior.py's EM, written from the definitions of
include/ctvae_hip.h.  No torch, no GPU import: tests/test_code_prior_host.py pins it against hand-made tables and a known chain,
the GPU tests compare the kernels with it.

* ``count`` / ``totals``     the four int64 tables (``np.add.at``) and the tokens left out; their row sums
* ``contexts``               the rows (position, left, up, previous codebook; K at a boundary) of every token
* ``token_probs``            P_j of every token's own code [B, C, H, W, J]; an empty row is 1/K
* ``score``                  logp [B, C], resp [B, C, J], bad [B] and the summed magnitudes the rounding error is measured against
* ``em``                     deleted interpolation: lambda after ``em_iters`` rounds with the uniform floor
* ``sample``                 ancestral sampling from given uniforms, operation by operation as the kernel does
* ``chain_fixture``          seeded index grids from a known first-order chain along w
"""
import math

import numpy as np

J = 5
EXPERTS = ("uniform", "position", "left", "up", "previous")


def empty_tables(K, C, H, W):
    return [np.zeros((C, H * W, K), dtype=np.int64)] + [np.zeros((C, K + 1, K), dtype=np.int64) for _ in range(3)]


def contexts(inds, K):
    """(pos_row, left, up, prev) int64 [B, C, H, W]: the table rows of every token; K where there is no neighbour."""
    inds = np.asarray(inds, dtype=np.int64)
    B, C, H, W = inds.shape
    pos = np.broadcast_to((np.arange(H)[:, None] * W + np.arange(W)[None, :])[None, None], inds.shape)
    left = np.full_like(inds, K)
    left[:, :, :, 1:] = inds[:, :, :, :-1]
    up = np.full_like(inds, K)
    up[:, :, 1:, :] = inds[:, :, :-1, :]
    prev = np.full_like(inds, K)
    prev[:, 1:] = inds[:, :-1]
    return pos, left, up, prev


def count(inds, K, tables=None):
    """(tables, invalid): every token added to pos / left / up / prev; a token whose own code or an existing neighbour's lies
    outside [0, K) is counted in ``invalid`` alone."""
    inds = np.asarray(inds, dtype=np.int64)
    B, C, H, W = inds.shape
    tables = [t.copy() for t in tables] if tables is not None else empty_tables(K, C, H, W)
    pos, left, up, prev = contexts(inds, K)
    inside = (inds >= 0) & (inds < K)
    ok = inside.copy()
    ok[:, :, :, 1:] &= inside[:, :, :, :-1]
    ok[:, :, 1:, :] &= inside[:, :, :-1, :]
    ok[:, 1:] &= inside[:, :-1]
    c = np.broadcast_to(np.arange(C)[None, :, None, None], inds.shape)
    for table, row in zip(tables, (pos, left, up, prev)):
        np.add.at(table, (c[ok], row[ok], inds[ok]), 1)
    return tables, int((~ok).sum())


def totals(tables):
    return [t.sum(axis=2, dtype=np.int64) for t in tables]


def token_probs(inds, tables, K):
    """float64 [B, C, H, W, J]: P_j(own code | row_j).  The indices must lie inside [0, K)."""
    inds = np.asarray(inds, dtype=np.int64)
    B, C, H, W = inds.shape
    c = np.broadcast_to(np.arange(C)[None, :, None, None], inds.shape)
    out = np.empty(inds.shape + (J,), dtype=np.float64)
    out[..., 0] = 1.0 / np.float64(K)
    for j, (table, tot, row) in enumerate(zip(tables, totals(tables), contexts(inds, K)), start=1):
        n = table[c, row, inds].astype(np.float64)
        d = tot[c, row].astype(np.float64)
        out[..., j] = np.where(d > 0, n / np.where(d > 0, d, 1.0), 1.0 / np.float64(K))
    return out


def score(inds, tables, lam, K):
    """(logp [B, C], resp [B, C, J], bad [B], logp_scale [B, C], resp_scale [B, C, J]); the scales are the sums of the magnitudes
    of what is added.  An image with an index outside [0, K) has bad = 1 and zeros."""
    inds = np.asarray(inds, dtype=np.int64)
    lam = np.asarray(lam, dtype=np.float64)
    B, C, H, W = inds.shape
    bad = ((inds < 0) | (inds >= K)).reshape(B, -1).any(axis=1)
    safe = np.where(bad[:, None, None, None], 0, inds)
    P = token_probs(safe, tables, K)
    m = lam[None, :, None, None, :] * P
    mix = (((m[..., 0] + m[..., 1]) + m[..., 2]) + m[..., 3]) + m[..., 4]
    lg = np.log(mix)
    r = m / mix[..., None]
    logp = np.array([[math.fsum(lg[b, c].ravel()) for c in range(C)] for b in range(B)])
    resp = np.array([[[math.fsum(r[b, c, :, :, j].ravel()) for j in range(J)] for c in range(C)] for b in range(B)])
    logp_scale = np.abs(lg).sum(axis=(2, 3))
    resp_scale = r.sum(axis=(2, 3))
    for arr in (logp, resp, logp_scale, resp_scale):
        arr[bad] = 0.0
    return logp, resp, bad.astype(np.int32), logp_scale, resp_scale


def em(inds, tables, K, em_iters, uniform_floor):
    """lambda float64 [C, J] after ``em_iters`` rounds from 1/J on ``inds`` (rows that were not counted)."""
    inds = np.asarray(inds, dtype=np.int64)
    B, C, H, W = inds.shape
    lam = np.full((C, J), 1.0 / J, dtype=np.float64)
    e0 = np.zeros(J)
    e0[0] = 1.0
    for _ in range(em_iters):
        _, resp, bad, _, _ = score(inds, tables, lam, K)
        tokens = float(int((bad == 0).sum()) * H * W)
        lam = (1.0 - uniform_floor) * (resp.sum(axis=0) / tokens) + uniform_floor * e0
    return lam


def nats_per_code(inds, tables, lam, K):
    logp, _, bad, _, _ = score(inds, tables, lam, K)
    B, C, H, W = np.asarray(inds).shape
    return -float(logp[bad == 0].sum()) / (int((bad == 0).sum()) * C * H * W)


def pick_expert(u1, lam_c):
    """The smallest j with u1 < lam_c[0] + ... + lam_c[j], added left to right; J - 1 when none."""
    cum = np.float64(0.0)
    for j in range(J):
        cum = cum + np.float64(lam_c[j])
        if u1 < cum:
            return j
    return J - 1


def sample(tables, lam, u, H, W):
    """int64 [n, C, H, W] from u float64 [n, H*W, C, 2]: the same IEEE operations as the kernel, one multiplication per decision."""
    u = np.asarray(u, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    n, HW, C, _ = u.shape
    K = tables[0].shape[2]
    tot = totals(tables)
    out = np.empty((n, C, H, W), dtype=np.int64)
    for i in range(n):
        for p in range(HW):
            h, w = divmod(p, W)
            for c in range(C):
                u1, u2 = u[i, p, c, 0], u[i, p, c, 1]
                j = pick_expert(u1, lam[c])
                row = None
                if j == 1:
                    row = p
                elif j == 2:
                    row = out[i, c, h, w - 1] if w > 0 else K
                elif j == 3:
                    row = out[i, c, h - 1, w] if h > 0 else K
                elif j == 4:
                    row = out[i, c - 1, h, w] if c > 0 else K
                total = int(tot[j - 1][c, row]) if j > 0 else 0
                if total == 0:
                    k = min(K - 1, int(np.floor(u2 * np.float64(K))))
                else:
                    t = min(total - 1, int(np.floor(u2 * np.float64(total))))
                    k = int(np.searchsorted(np.cumsum(tables[j - 1][c, row]), t, side="right"))
                out[i, c, h, w] = k
    return out


def chain_fixture(seed, B, K, C, H, W, stay=0.7):
    """Seeded grids from a known first-order chain along w: the first column is uniform, every next code repeats its left
    neighbour with probability ``stay`` and is uniform otherwise (every codebook and row on its own).  Its conditional entropy
    is far below ln K, and only the ``left`` expert can see it."""
    rng = np.random.default_rng(seed)
    x = np.empty((B, C, H, W), dtype=np.int64)
    x[..., 0] = rng.integers(0, K, size=(B, C, H))
    for w in range(1, W):
        fresh = rng.integers(0, K, size=(B, C, H))
        x[..., w] = np.where(rng.random((B, C, H)) < stay, x[..., w - 1], fresh)
    return x
