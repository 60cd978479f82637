"""Shared by tests/test_vq_ops_gpu.py (the HIP quantiser kernels of csrc/vq.hip, op by op) and tests/test_vq_reference_host.py
(the same reference and inputs, checked on the CPU): a float64 reference of the multi-codebook quantiser written from
mcq_vae.py:26-64 and :100-127, the case tables (one id per dispatch path) and the seeded input generators.

Layouts are the kernels': latents ``x`` [P = B*HW][D] (NHWC, flattened), codebooks ``E`` [C][K][Dc = D/C], indices [B][C][HW].
Codebook ``i`` reads latent columns ``i .. i+Dc-1`` -- the reference's slice ``latents[:, i:i+Dc]`` (mcq_vae.py:104,117), not
``i*Dc``.  Nothing here imports oracle/vae_cpu.py: test_vq_reference_host.py pins the two against each other.
"""
from collections import namedtuple
from functools import lru_cache

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24                      # unit round-off of float32

Case = namedtuple("Case", "id D K C HW B path")


def _c(id, D, K, C, HW, B, path):
    return Case(id, D, K, C, HW, B, path)


# ---------------------------------------------------------------------------------------------------------------------
# index search: launch_vq_inds picks vq_inds_reg_kernel<Dc> for K <= 64 and Dc in {32, 64, 128}, else vq_inds_kernel
# ---------------------------------------------------------------------------------------------------------------------
IND_CASES = [
    _c("reg32-P192", 128, 64, 4, 64, 3, "reg"),              # model shape; 12 blocks of 16 rows
    _c("reg32-P245-tail5", 128, 64, 4, 49, 5, "reg"),        # last block has 5 rows, HW odd
    _c("reg32-K37", 128, 37, 4, 64, 2, "reg"),               # K < 64: masked lanes, clamped codebook staging
    _c("reg64-P252", 128, 64, 2, 36, 7, "reg"),              # vq_inds_reg_kernel<64>
    _c("reg64-K1", 64, 1, 1, 16, 1, "reg"),                  # one code
    _c("reg128-P256", 128, 64, 1, 64, 4, "reg"),             # CT shape, 64 rows per block
    _c("reg128-P2112", 128, 64, 1, 64, 33, "reg"),
    _c("reg128-K50-P75-tail11", 128, 50, 1, 25, 3, "reg"),   # one full block + 11 rows
    _c("generic-K512", 64, 512, 1, 256, 2, "generic"),       # VQ-VAE shape, 8 codes per lane
    _c("generic-K65-P27", 64, 65, 1, 9, 3, "generic"),       # K = 64 + 1
    _c("generic-C8-Dc5-K200", 40, 200, 8, 30, 5, "generic"),  # Dc not a multiple of 4, K = 3*64 + 8
    _c("generic-C3-Dc7-K37", 21, 37, 3, 10, 7, "generic"),
    _c("generic-Dc192", 192, 64, 1, 4, 5, "generic"),        # three staging rounds per lane
    _c("reg32-P38400-nbclamp", 128, 64, 4, 64, 600, "reg"),  # P > 2048*16: more than 16 rows per workgroup
    _c("generic-K512-P38400-blocksclamp", 64, 512, 1, 64, 600, "generic"),   # P > 512*64
]
IND_LABEL = {"reg": "vq_inds_reg_kernel", "generic": "vq_inds_kernel"}

# cases of (a) whose integers are drawn from -1 .. 1 instead of -2 .. 2 (the tie share of the wider range is below 2 %)
EXACT_NARROW = {"generic-K65-P27", "generic-Dc192"}

# (c): (case id, kind).  "o1": x ~ N(0,1), E ~ N(0,1).  "model": E ~ U(-1/K, 1/K) as the models initialise it
# (mcq_vae.py:22-23), x ~ N(0,1).  "model-small": the same codebook, x ~ N(0,1) / K.
RANDOM_KINDS = ("o1", "model", "model-small")
IND_RANDOM = [(c.id, "o1") for c in IND_CASES if c.K > 1] + [
    ("reg32-P192", "model"), ("reg32-P192", "model-small"), ("reg32-P245-tail5", "model"), ("reg32-K37", "model"),
    ("reg64-P252", "model-small"), ("reg128-P2112", "model-small"), ("reg128-K50-P75-tail11", "model-small"),
    ("generic-K512", "model-small"), ("generic-K65-P27", "model"), ("generic-C8-Dc5-K200", "model"),
    ("generic-C3-Dc7-K37", "model"), ("generic-Dc192", "model-small"), ("reg32-P38400-nbclamp", "model"),
]
# (with x ~ N(0,1) against a +-1/K codebook and Dc >= 64 the bound of tol_rows() cannot separate the best two codes on more
# than 1 % of the rows -- 1.4 % to 16 % measured on the reference -- so those shapes take the model's codebook with small latents)

# ---------------------------------------------------------------------------------------------------------------------
# lookup + loss
# ---------------------------------------------------------------------------------------------------------------------
LOOKUP_CASES = [
    (_c("C4-P192", 128, 64, 4, 64, 3, None), 0.25),
    (_c("C4-P245", 128, 64, 4, 49, 5, None), 1.0),
    (_c("C1-PD270336-gridstride", 128, 64, 1, 64, 33, None), 1.0),      # P*D > 1024 blocks * 256
    (_c("C3-PD1470-fewpartials", 21, 37, 3, 10, 7, None), 0.0),         # 6 partials for the finish kernel's 64 lanes
    (_c("C8-Dc5", 40, 200, 8, 30, 5, None), 0.25),
    (_c("C1-K512", 64, 512, 1, 256, 2, None), 0.25),
]

# ---------------------------------------------------------------------------------------------------------------------
# backward: launch_vq_backward picks pos (Dc <= 32, K <= 128), posw (Dc <= 128, K <= 74) or scan, S slices
# ---------------------------------------------------------------------------------------------------------------------
BWD_CASES = [
    _c("pos-P192", 128, 64, 4, 64, 3, "pos"),
    _c("pos-P245", 128, 64, 4, 49, 5, "pos"),
    _c("pos-P2053-S9", 128, 64, 4, 2053, 1, "pos"),          # reduce kernel: 8-wide body + a tail of 1
    _c("pos-P5", 128, 64, 4, 5, 1, "pos"),                   # fewer positions than half-waves
    _c("pos-K128", 128, 128, 4, 64, 2, "pos"),
    _c("pos-K37", 128, 37, 4, 64, 2, "pos"),
    _c("pos-C8-Dc5-K100", 40, 100, 8, 30, 5, "pos"),         # lanes d >= Dc idle
    _c("posw-Dc128-P75", 128, 64, 1, 25, 3, "posw"),
    _c("posw-Dc128-P2112-S33", 128, 64, 1, 64, 33, "posw"),
    _c("posw-Dc64-C2", 128, 64, 2, 36, 7, "posw"),
    _c("posw-Dc33-K73-C2", 66, 73, 2, 10, 7, "posw"),
    _c("scan1-K512-P512", 64, 512, 1, 256, 2, "scan1"),
    _c("scan1-K80-P100", 64, 80, 1, 25, 4, "scan1"),
    _c("scan1-Dc192", 192, 64, 1, 4, 5, "scan1"),
    _c("scan1-Dc256-K16", 256, 16, 1, 9, 3, "scan1"),
    _c("scanS2-K512-P2048", 64, 512, 1, 256, 8, "scanS"),
    _c("scanS5-K200-Dc40-P2600", 40, 200, 1, 100, 26, "scanS"),   # slice length 520
    _c("scanS5-K200-Dc40-P2587", 40, 200, 1, 199, 13, "scanS"),   # slice length 518, last slice 515
]
# path -> (label of the codebook-gradient kernel, vq_cb_reduce_kernel runs)
BWD_LABEL = {"pos": ("vq_bwd_codebook_pos_kernel", True), "posw": ("vq_bwd_codebook_posw_kernel", True),
             "scan1": ("vq_bwd_codebook_kernel", False), "scanS": ("vq_bwd_codebook_kernel", True)}
BWD_ALL_LABELS = ("vq_bwd_codebook_pos_kernel", "vq_bwd_codebook_posw_kernel", "vq_bwd_codebook_kernel")


def bwd_path(D, K, C, P):
    """The launcher's choice (csrc/vq.hip launch_vq_backward) with ample scratch, and the number of slices."""
    Dc = D // C
    if Dc <= 32 and K <= 128:
        S = min(-(-P // 256), 512)
        return "pos", -(-P // -(-P // S))
    if Dc <= 128 and (4 * K * 128 + 4 * K) * 4 <= 150 * 1024:
        S = min(-(-P // 64), 512)
        return "posw", -(-P // -(-P // S))
    S = min(1024 // (K * C), P // 512)
    return ("scanS", S) if S >= 2 else ("scan1", 1)


def case_of(cases, id):
    return next(c for c in cases if c.id == id)


def seed_of(case, salt=0):
    return 7919 * (case.D + 3 * case.K + 5 * case.C + 7 * case.HW + 11 * case.B) + salt


# ---------------------------------------------------------------------------------------------------------------------
# reference (float64)
# ---------------------------------------------------------------------------------------------------------------------
def rows_of(inds):
    """[B, C, HW] -> [P, C]: the index of row p = b*HW + hw for codebook i."""
    B, C, HW = inds.shape
    return inds.permute(0, 2, 1).reshape(B * HW, C)


def inds_of(rows, B, HW):
    """[P, C] -> [B, C, HW]"""
    return rows.view(B, HW, -1).permute(0, 2, 1).contiguous()


def dist64(x, E):
    """dist[p, i, k] = sum_d (x[p, i+d] - E[i, k, d])^2 in float64, difference form (no cancellation).  x [P, D], E [C, K, Dc]
    float32 (cast up here)."""
    C, K, Dc = E.shape
    P = x.shape[0]
    x, E = x.double(), E.double()
    out = torch.empty(P, C, K, dtype=torch.float64)
    step = max(1, (1 << 24) // (K * Dc))
    for i in range(C):
        for lo in range(0, P, step):
            xs = x[lo:lo + step, i:i + Dc]
            out[lo:lo + step, i] = ((xs[:, None, :] - E[i][None, :, :]) ** 2).sum(-1)
    return out


def expanded32(x, E):
    """The reference's own float32 arithmetic (mcq_vae.py:32-34): (|x|^2 + |e|^2) - 2 x.e, per codebook.  [P, C, K] float32."""
    C, K, Dc = E.shape
    out = torch.empty(x.shape[0], C, K, dtype=torch.float32)
    for i in range(C):
        xs = x[:, i:i + Dc]
        out[:, i] = torch.sum(xs ** 2, dim=1, keepdim=True) + torch.sum(E[i] ** 2, dim=1) - 2 * torch.matmul(xs, E[i].t())
    return out


def first_argmin(dist):
    """Index of the FIRST minimum along the last axis (what torch.argmin documents), written out so that it does not rest on it."""
    K = dist.shape[-1]
    m = dist.min(-1, keepdim=True).values
    k = torch.arange(K).expand_as(dist)
    return torch.where(dist == m, k, torch.full_like(k, K)).min(-1).values


def tie_share(dist):
    """Share of the (row, codebook) pairs whose minimum is attained by more than one code."""
    m = dist.min(-1, keepdim=True).values
    return float(((dist == m).sum(-1) > 1).double().mean())


def tol_rows(x, E):
    """tol[p, i] = 4 * (Dc + 3) * u * (|x_p,i| + max_k |e_i,k|)^2, u = 2^-24.

    A float32 dot product of length n summed in any order (fused or not) errs by at most gamma_n * sum |a_j b_j| <=
    n u |a||b| to first order (Cauchy-Schwarz).  The kernel forms xx = x.x, ee = e.e and dot = x.e this way, then
    (xx + ee) - 2 dot: the three sums contribute Dc u (|x|^2 + |e|^2 + 2|x||e|) = Dc u (|x| + |e|)^2, the two additions at most
    u each of intermediates no larger than (|x| + |e|)^2, the doubling is exact: |computed - true| <= (Dc + 2) u (|x| + |e|)^2;
    Dc + 3 covers the second-order terms.  The arg-min compares two computed distances, so a code can win only if its true
    distance is within twice that of the true minimum; the constant 4 leaves a factor 2 on top.  |e| is replaced by its maximum
    over the codebook, which only loosens the bound."""
    C, K, Dc = E.shape
    x, E = x.double(), E.double()
    emax = E.norm(dim=-1).max(-1).values                                  # [C]
    xn = torch.stack([x[:, i:i + Dc].norm(dim=-1) for i in range(C)], 1)   # [P, C]
    return 4.0 * (Dc + 3) * U32 * (xn + emax[None, :]) ** 2


def runner_up_share(dist, tol):
    """Share of the (row, codebook) pairs whose float64 runner-up lies within tol of the minimum: the rows on which the bound
    of tol_rows() could not tell the arg-min from the second best."""
    two = dist.topk(2, dim=-1, largest=False).values
    return float(((two[..., 1] - two[..., 0]) <= tol).double().mean())


def excess(dist, chosen_rows, tol):
    """dist64[p, chosen] - min_k dist64[p, k] - tol(p), per (row, codebook): must be <= 0 everywhere."""
    got = dist.gather(-1, chosen_rows[..., None]).squeeze(-1)
    return got - dist.min(-1).values - tol


def forward64(x, E, rows, beta):
    """(quantized [P, D], vq_loss) of mcq_vae.py:41-64,112-127 for given indices, as a float64 autograd graph over x and E."""
    C, K, Dc = E.shape
    qs, losses = [], []
    for i in range(C):
        xs = x[:, i:i + Dc]
        q = E[i][rows[:, i]]
        losses.append(F.mse_loss(q.detach(), xs) * beta + F.mse_loss(q, xs.detach()))
        qs.append(xs + (q - xs).detach())
    return torch.cat(qs, 1), sum(losses)


def reference64(x, E, inds, beta, g_q=None, g_vq=None):
    """dict(quantized, vq_loss, g_lat, d_cb) in float64 from float32 inputs; the gradients are those of
    sum(quantized * g_q) + vq_loss * g_vq (a missing factor counts as zero) by float64 autograd."""
    x64 = x.double().requires_grad_(True)
    E64 = E.double().requires_grad_(True)
    q, loss = forward64(x64, E64, rows_of(inds), beta)
    out = dict(quantized=q.detach(), vq_loss=loss.detach())
    obj = q.sum() * 0.0
    if g_q is not None:
        obj = obj + (q * g_q.double().view_as(q)).sum()
    if g_vq is not None:
        obj = obj + loss * float(g_vq)
    g_lat, d_cb = torch.autograd.grad(obj, [x64, E64], allow_unused=True)
    out["g_lat"] = g_lat if g_lat is not None else torch.zeros_like(x64)
    out["d_cb"] = d_cb if d_cb is not None else torch.zeros_like(E64)
    return out


def quantized32(x, E, inds):
    """float32 torch x + (E[idx] - x) with the slice quirk: the kernel promises this rounding, element by element."""
    C, K, Dc = E.shape
    rows = rows_of(inds)
    return torch.cat([x[:, i:i + Dc] + (E[i][rows[:, i]] - x[:, i:i + Dc]) for i in range(C)], 1)


def straight_through32(g_q, C):
    """g_lat[p][j] = sum_i g_q[p][i*Dc + j - i] in float32, terms added in the order i = ilo .. ihi (vq_bwd_latents_kernel)."""
    P, D = g_q.shape
    Dc = D // C
    g = torch.zeros(P, D, dtype=torch.float32)
    for i in range(C):
        g[:, i:i + Dc] += g_q[:, i * Dc:(i + 1) * Dc]
    return g


# ---------------------------------------------------------------------------------------------------------------------
# inputs (all from seeds)
# ---------------------------------------------------------------------------------------------------------------------
def _gen(case, salt):
    return torch.Generator().manual_seed(seed_of(case, salt))


@lru_cache(maxsize=4)
def exact_inputs(case):
    """(a): small integers as float32.  Every product and partial sum of the expanded form is an integer far below 2^24, so
    float32 computes it exactly in any order and ties for the minimum are frequent."""
    g = _gen(case, 1)
    r = 1 if case.id in EXACT_NARROW else 2
    P, Dc = case.B * case.HW, case.D // case.C
    x = torch.randint(-r, r + 1, (P, case.D), generator=g).float()
    E = torch.randint(-r, r + 1, (case.C, case.K, Dc), generator=g).float()
    return x, E


def duplicate_pairs(K):
    """(src, dst), src < dst: code row dst is a copy of row src.  k / k+64 and k / k+128 sit in one lane's walk of the generic
    kernel, k / k+5 and k / k+33 in different lanes of one wave, and K-1 is the last valid code."""
    pairs, used = [], set()
    for src, dst in ((1, 65), (2, 130), (3, 8), (4, 37), (0, K - 1)):
        if src < dst < K and not {src, dst} & used:
            pairs.append((src, dst))
            used |= {src, dst}
    return pairs


@lru_cache(maxsize=4)
def planted_inputs(case):
    """(b): O(1) random data, some code rows copied onto later rows, every fourth latent row set equal (for one codebook) to a
    duplicated code row.  Returns x, E, planted [P, C] bool, want [P, C] (the lower index of the pair where planted)."""
    g = _gen(case, 2)
    P, Dc, C = case.B * case.HW, case.D // case.C, case.C
    x = torch.randn(P, case.D, generator=g)
    E = torch.randn(C, case.K, Dc, generator=g)
    pairs = duplicate_pairs(case.K)
    for src, dst in pairs:
        E[:, dst] = E[:, src]
    planted = torch.zeros(P, C, dtype=torch.bool)
    want = torch.zeros(P, C, dtype=torch.int64)
    for n, p in enumerate(range(0, P, 4)):
        i = n % C
        src, _ = pairs[(n // C) % len(pairs)]
        x[p, i:i + Dc] = E[i, src]
        planted[p, i] = True
        want[p, i] = src
    return x, E, planted, want


@lru_cache(maxsize=4)
def random_inputs(case, kind):
    """(c)"""
    g = _gen(case, 3 + RANDOM_KINDS.index(kind))
    P, Dc = case.B * case.HW, case.D // case.C
    x = torch.randn(P, case.D, generator=g)
    if kind == "o1":
        E = torch.randn(case.C, case.K, Dc, generator=g)
    else:
        E = (torch.rand(case.C, case.K, Dc, generator=g) * 2 - 1) / case.K
        if kind == "model-small":
            x = x / case.K
    return x, E


def given_inds(case, kind, salt=0):
    """[B, C, HW] int64.  "uniform": every code equally likely.  "skewed": codes 0 .. 2 only, more than half of the positions
    on code 1 (long runs of one code, most codes never hit)."""
    g = _gen(case, 20 + salt)
    inds = torch.randint(0, case.K, (case.B, case.C, case.HW), generator=g)
    if kind == "skewed":
        inds = inds % 3
        inds[torch.rand(inds.shape, generator=g) < 0.6] = 1
        inds = inds.clamp_(max=case.K - 1)
    return inds


def exact_gvq(case):
    """P*Dc/2 as a float: the kernels' scale g_vq * 2 / (P*Dc) is then exactly 1 (P*Dc < 2^24 in every case here)."""
    n = case.B * case.HW * (case.D // case.C)
    assert n < 2 ** 24
    return n / 2.0


def exact_dcb(case, x, E, inds):
    """Codebook gradient for the integer inputs of (a) and g_vq = exact_gvq(case): count * E - sum x, an integer in every
    element.  float64 autograd returns it to ~1e-13 (its 2/(P*Dc) is rounded unless P*Dc is a power of two); rounding that to
    the nearest integer gives the true value, which float32 holds exactly and any summation order must reproduce."""
    want = reference64(x, E, inds, 0.25, None, exact_gvq(case))["d_cb"]
    assert float((want - want.round()).abs().max()) < 1e-9
    assert float(want.abs().max()) < 2 ** 24
    return want.round()
