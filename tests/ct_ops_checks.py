"""Float64 references and case tables of the causal-transition kernels (csrc/glinear.hip, gatlayer.hip, ctmisc.hip, pairmlp.hip),
written from the formulas of include/ctvae_hip.h.  No GPU import: tests/test_ct_ops_reference_host.py pins every reference to
the project's torch path and evaluates the input conditions of every case; tests/test_ct_ops_gpu.py calls the C ABI.

Conventions: inputs are float32 tensors (what the kernels read), references convert them to float64 first, so both sides see
the same numbers.  The clamp bound of the samplers / the cross-entropy is the float32 value of 1e-4 (BOUND), as in the kernels.
"""
import zlib
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch

EPS32 = 2.0 ** -23                       # spacing of float32 at 1: twice the unit roundoff
BOUND = float(np.float32(1e-4))          # clamp(min=1e-4) as the kernels hold it
EXCLUDE_CAP = 0.005                      # at most 0.5 % of a case's hard decisions may lie inside the float32 margin
SLOPE_PAIR = 0.01                        # nn.LeakyReLU() of the discoverers
SLOPE_GAT = 0.2                          # GATv2Conv negative_slope
LEAKY = 0.01                             # nn.LeakyReLU() between the two GATv2 layers (act = 1)
ERR_BAD_ARG, ERR_WORKSPACE = -22, -12


def seed_of(cid: str, salt: int = 0) -> int:
    return (zlib.crc32(cid.encode()) + 7919 * salt) % (2 ** 31)


def gen_of(cid: str, salt: int = 0) -> torch.Generator:
    return torch.Generator().manual_seed(seed_of(cid, salt))


def _f32(fn):
    """Inputs are float32 whatever default dtype the caller runs under."""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **k):
        prev = torch.get_default_dtype()
        torch.set_default_dtype(torch.float32)
        try:
            return fn(*a, **k)
        finally:
            torch.set_default_dtype(prev)
    return wrapped


def d(t):
    return None if t is None else t.detach().to(torch.float64)


def case_of(cases, cid):
    return next(c for c in cases if c.id == cid)


# =====================================================================================================================
# glinear
# =====================================================================================================================
@dataclass(frozen=True)
class Seg:
    G: int                      # matrices in this segment's bank
    grouped: bool               # group ids given (else NULL: matrix 0 for everybody)
    koff: int = 0               # column offset of the K used columns inside the bank's rows
    tail: int = 0               # unused columns behind them: ldw = koff + K + tail
    bias: bool = True
    spare: bool = False         # grouped: the last bank row is used by no sample


@dataclass(frozen=True)
class GLCase:
    id: str
    B: int
    K: int
    N: int
    segs: Tuple[Seg, ...]
    xpad: int = 0               # ldx = K + xpad
    ypad: int = 0               # ldy = nseg*N + ypad
    salt: int = 0

    @property
    def nseg(self):
        return len(self.segs)


U = Seg(1, False)
GL_CASES = [
    GLCase("K4-N4-B2", 2, 4, 4, (U,)),
    GLCase("K36-N12-s2", 3, 36, 12, (Seg(1, False, bias=False), Seg(3, True, koff=4, tail=8, spare=True)), xpad=4, ypad=8),
    GLCase("K64-N64-s3", 3, 64, 64, (Seg(2, True), Seg(1, False, koff=8), Seg(4, True, tail=4, bias=False, spare=True)), ypad=4),
    GLCase("K68-N96-s4", 3, 68, 96, (U, Seg(2, True, koff=8, tail=4), Seg(1, False, bias=False), Seg(3, True, spare=True)), xpad=12),
    GLCase("K100-N132-s2", 2, 100, 132, (Seg(2, True, koff=4), Seg(1, False, tail=12)), xpad=4, ypad=12),
    GLCase("K64-N96-B10", 10, 64, 96, (U,)),
    # batch slices of the weight gradient (ungrouped: S = clamp(B/8, 1, 16); grouped: S = clamp(B/(4G), 1, 16); then ++S until a
    # slice holds at most 64 samples)
    GLCase("B7-S1", 7, 36, 12, (Seg(1, False, tail=4),)),
    GLCase("B19-S2", 19, 36, 12, (U,), xpad=4),
    GLCase("B130-S16", 130, 4, 12, (U,)),
    GLCase("G2-B16-S2", 16, 36, 12, (Seg(2, True),)),
    GLCase("G5-B10-S1", 10, 36, 12, (Seg(5, True, koff=4, spare=True),)),
    GLCase("G20-B65-S2", 65, 4, 4, (Seg(20, True),)),
]
GL_EXPECT_S = {"K4-N4-B2": 1, "B7-S1": 1, "B19-S2": 2, "B130-S16": 16, "G2-B16-S2": 2, "G5-B10-S1": 1, "G20-B65-S2": 2}


def gl_slices(B: int, G: int, grouped: bool) -> int:
    """The number of batch slices ctvae_glinear_wgrad uses (restated from the header's description of the launcher)."""
    S = B // (4 * G) if grouped else B // 8
    S = max(1, min(16, S))
    while -(-B // S) > 64:
        S += 1
    return S


def gl_ws_floats(G, N, K, S):
    return S * G * N * (K + 1)


@_f32
def gl_inputs(case: GLCase, kind: str):
    """kind 'int': integers in [-3, 3]; 'gauss': N(0, 1).  Returns dict(x [B,64,K], dy [B,64,nseg*N], banks [(W [G,N,ldw], bias
    [G,N] or None, group int32 [B] or None)])."""
    g = gen_of(case.id, {"int": 1, "gauss": 2}[kind] + 10 * case.salt)

    def draw(*shape):
        if kind == "int":
            return torch.randint(-3, 4, shape, generator=g).float()
        return torch.randn(*shape, generator=g)

    x = draw(case.B, 64, case.K)
    dy = draw(case.B, 64, case.nseg * case.N)
    banks = []
    for s in case.segs:
        W = draw(s.G, case.N, s.koff + case.K + s.tail)
        b = draw(s.G, case.N) if s.bias else None
        grp = None
        if s.grouped:
            hi = s.G - 1 if s.spare else s.G
            grp = torch.randint(0, hi, (case.B,), generator=g).to(torch.int32)
            grp[: min(hi, case.B)] = torch.arange(min(hi, case.B), dtype=torch.int32)      # every other row is used
        banks.append((W, b, grp))
    return dict(x=x, dy=dy, banks=banks)


def glinear_ref(case: GLCase, inp, drop_k_tail=False, skip_slab=None):
    """Forward and, by float64 autograd of per-sample matmuls, dx / dW / dbias.  Also the |a| @ |b| sums of the derived bound.
    drop_k_tail / skip_slab: deliberately wrong variants (a kernel that forgets the last partial 32-chunk of K; a reduction
    that skips the slab of one batch slice) for the host test's sensitivity check."""
    K, N = case.K, case.N
    x = d(inp["x"]).requires_grad_(True)
    dy = d(inp["dy"])
    Ws, bs, ys, ya = [], [], [], []
    Keff = (K - 1) // 32 * 32 if drop_k_tail else K
    for s, (W, b, grp) in zip(case.segs, inp["banks"]):
        Wu = d(W)[:, :, s.koff:s.koff + K].clone().requires_grad_(True)
        bu = d(b).clone().requires_grad_(True) if b is not None else None
        idx = grp.long() if grp is not None else torch.zeros(case.B, dtype=torch.long)
        Wb = Wu[idx]                                             # [B, N, K]
        y = torch.einsum("bmk,bnk->bmn", x[..., :Keff], Wb[..., :Keff])
        a = torch.einsum("bmk,bnk->bmn", x.detach().abs(), Wb.detach().abs())
        if bu is not None:
            y = y + bu[idx][:, None, :]
            a = a + bu.detach().abs()[idx][:, None, :]
        Ws.append(Wu), bs.append(bu), ys.append(y), ya.append(a)
    y = torch.cat(ys, -1)
    y.backward(dy)
    out = dict(y=y.detach(), y_abs=torch.cat(ya, -1), dx=x.grad, dW=[w.grad for w in Ws], db=[b.grad if b is not None else None for b in bs])
    # abs sums of the two gradient directions
    dxa = torch.zeros_like(x.grad)
    out["dW_abs"], out["db_abs"], out["rows"] = [], [], []
    for si, (s, (W, b, grp)) in enumerate(zip(case.segs, inp["banks"])):
        idx = grp.long() if grp is not None else torch.zeros(case.B, dtype=torch.long)
        Wa = d(W)[:, :, s.koff:s.koff + K].abs()
        dys = dy[..., si * N:(si + 1) * N]
        dxa += torch.einsum("bmn,bnk->bmk", dys.abs(), Wa[idx])
        oh = torch.nn.functional.one_hot(idx, s.G).to(torch.float64)                     # [B, G]
        out["dW_abs"].append(torch.einsum("bg,bmn,bmk->gnk", oh, dys.abs(), x.detach().abs()))
        out["db_abs"].append(torch.einsum("bg,bmn->gn", oh, dys.abs()))
        out["rows"].append(64 * oh.sum(0))                                               # reduction length per group
        if skip_slab is not None:                                                        # the samples of one slice never arrive
            S = gl_slices(case.B, s.G if s.grouped else 1, s.grouped)
            per = -(-case.B // S)
            keep = torch.ones(case.B, dtype=torch.float64)
            keep[skip_slab * per:(skip_slab + 1) * per] = 0.0
            out["dW"][si] = torch.einsum("bg,bmn,bmk->gnk", oh * keep[:, None], dys, x.detach())
    out["dx_abs"] = dxa
    return out


def dot_bound(L, abs_sum):
    """|fl(sum of L products) - exact| <= L * 2^-23 * sum |a_i| |b_i|: the forward error bound of a float32 dot product of length
    L in any summation order (gamma_L = L u / (1 - L u) with u = 2^-24; the factor 2 covers 1 / (1 - L u) and one final add)."""
    return L * EPS32 * abs_sum


# =====================================================================================================================
# fused GATv2 layer
# =====================================================================================================================
@dataclass(frozen=True)
class GatCase:
    id: str
    B: int
    Hs: int
    C: int
    graphs: Tuple[str, ...]          # one adjacency pattern per sample
    H: int = 0                       # heads of the parameter tensors (0: == Hs, head_map NULL)
    head_map: Optional[Tuple[Tuple[int, ...], ...]] = None
    act: int = 0
    ldpad: int = 0                   # xl | xr sit in one buffer of row stride 2*Hs*C + ldpad
    opad: int = 0                    # ldo = Hs*C + opad
    dpad: int = 0                    # d_xl | d_xr in one buffer of row stride 2*Hs*C + dpad
    dadj: str = "write"              # "null" | "write" | "acc"
    salt: int = 0


GAT_CASES = [
    GatCase("C16-H1-B1-rand", 1, 1, 16, ("rand",), salt=0),
    GatCase("C20-H2-B3-rand-dense-empty", 3, 2, 20, ("rand", "dense", "empty"), act=1, ldpad=8, opad=4, dpad=12, salt=1),
    GatCase("C64-H3-B3-map", 3, 3, 64, ("isolated", "diag", "neg"), H=5, head_map=((0, 2, 2), (4, 0, 1), (2, 2, 0)), dadj="acc", opad=8,
            salt=0),
    GatCase("C68-H2-B1-dense", 1, 2, 68, ("dense",), dadj="null", act=1, salt=0),
    GatCase("C128-H1-B3", 3, 1, 128, ("rand", "neg", "diag"), act=1, dpad=4, salt=0),
    GatCase("C128-H2-B1-map", 1, 2, 128, ("isolated",), H=4, head_map=((3, 3),), ldpad=4, dadj="acc", salt=0),
    GatCase("C16-H3-B1-empty", 1, 3, 16, ("empty",), salt=0),
]


def gat_graph(kind: str, g: torch.Generator):
    on = (torch.rand(64, 64, generator=g) < 0.6).float()
    w = torch.rand(64, 64, generator=g) * 0.9 + 0.1
    eye = torch.eye(64)
    if kind == "rand":
        return on * w * (1 - eye)
    if kind == "dense":
        return w * (1 - eye)
    if kind == "empty":
        return torch.zeros(64, 64)
    if kind == "isolated":            # target 5 has no incoming edge, target 9 exactly one
        a = on * w * (1 - eye)
        a[:, 5] = 0.0
        a[:, 9] = 0.0
        a[3, 9] = 0.75
        return a
    if kind == "diag":                # existing self loops: must be ignored
        a = on * w * (1 - eye)
        return a + eye * (torch.rand(64, generator=g) + 0.5)
    if kind == "neg":
        return on * (w - 0.55) * 2.0 * (1 - eye)
    raise ValueError(kind)


@_f32
def gat_inputs(case: GatCase):
    g = gen_of(case.id, 3 + case.salt)
    H = case.H or case.Hs
    adj = torch.stack([gat_graph(k, g) for k in case.graphs])
    return dict(xl=torch.randn(case.B, 64, case.Hs, case.C, generator=g), xr=torch.randn(case.B, 64, case.Hs, case.C, generator=g),
                adj=adj, we=torch.randn(H, case.C, generator=g), att=torch.randn(H, case.C, generator=g) / case.C ** 0.5,
                bias=torch.randn(H, case.C, generator=g),
                head_map=None if case.head_map is None else torch.tensor(case.head_map, dtype=torch.int32),
                g_out=torch.randn(case.B, 64, case.Hs, case.C, generator=g),
                dadj0=torch.randn(case.B, 64, 64, generator=g))


def gat_attr(adj):
    """(a' with the self-loop mean on the diagonal, kept pairs, edges, in-degree) of adj [B,64,64] (float64)."""
    eye = torch.eye(64, dtype=torch.bool)
    edge = (adj != 0) & ~eye
    w = adj * edge
    deg = edge.sum(1)
    loop = w.sum(1) / deg.clamp(min=1)
    return w + torch.diag_embed(loop), edge | eye, edge, deg


def gat_layer_ref(xl, xr, adj, we, att, bias, head_map, slope, act, g_out=None):
    """out [B,64,Hs,C], alpha [B,Hs,64,64] and (g_out given) d_xl, d_xr, d_adj and the per-slot d_bias / d_att / d_we [B,Hs,C].
    Also m [B,Hs,64,64,C], the leaky-ReLU arguments, and keep [B,64,64]."""
    B, _, Hs, C = xl.shape
    xl, xr, adj = d(xl).requires_grad_(True), d(xr).requires_grad_(True), d(adj).requires_grad_(True)
    hm = head_map.long() if head_map is not None else torch.arange(Hs).expand(B, Hs)
    wes, atts, biass = (d(t)[hm].clone().requires_grad_(True) for t in (we, att, bias))          # [B,Hs,C] per slot
    attr, keep, _, _ = gat_attr(adj)
    xls, xrs = xl.permute(0, 2, 1, 3), xr.permute(0, 2, 1, 3)                                   # [B,Hs,64,C]
    m = xls[:, :, :, None, :] + xrs[:, :, None, :, :] + attr[:, None, :, :, None] * wes[:, :, None, None, :]
    s = (torch.nn.functional.leaky_relu(m, slope) * atts[:, :, None, None, :]).sum(-1)
    alpha = torch.softmax(s.masked_fill(~keep[:, None], float("-inf")), dim=2)                   # over the sources r
    out = torch.einsum("bhrc,bhrk->bchk", alpha, xls) + biass[:, None]
    if act == 1:
        out = torch.nn.functional.leaky_relu(out, LEAKY)
    res = dict(out=out.detach(), alpha=alpha.detach(), m=m.detach(), keep=keep, attr=attr.detach())
    if g_out is not None:
        out.backward(d(g_out))
        res.update(d_xl=xl.grad, d_xr=xr.grad, d_adj=adj.grad, d_bias=biass.grad, d_att=atts.grad, d_we=wes.grad)
    return res


def gat_margin_count(case: GatCase, inp, ref):
    """Number of (kept pair, channel) leaky-ReLU arguments inside the float32 margin, and the number of them in all.  The kernels
    form m = fma(a', we, fl(xl + xr)) (or fl(fma(a', we, xl) + xr)): two roundings of at most 2^-24 relative each, on partial
    results bounded by |xl| + |xr| + |a' we|  ->  |m32 - m| <= 2^-23 (|xl| + |xr| + |a' we|).  On the diagonal a' is itself a
    float32 mean of up to 63 terms: |a'32 - a'| <= 64 * 2^-24 * mean |a|, times |we|."""
    hm = inp["head_map"].long() if inp["head_map"] is not None else torch.arange(case.Hs).expand(case.B, case.Hs)
    we = d(inp["we"])[hm].abs()                                                                  # [B,Hs,C]
    xl, xr = d(inp["xl"]).abs().permute(0, 2, 1, 3), d(inp["xr"]).abs().permute(0, 2, 1, 3)
    attr = ref["attr"].abs()
    mag = xl[:, :, :, None, :] + xr[:, :, None, :, :] + attr[:, None, :, :, None] * we[:, :, None, None, :]
    bound = EPS32 * mag
    adj = d(inp["adj"])
    _, _, edge, deg = gat_attr(adj)
    loop_abs = (adj.abs() * edge).sum(1) / deg.clamp(min=1)                                      # [B,64]
    extra = 64 * 2.0 ** -24 * loop_abs[:, None, :, None] * we[:, :, None, :]                      # [B,Hs,64,C]
    idx = torch.arange(64)
    bound[:, :, idx, idx, :] += extra
    kept = ref["keep"][:, None, :, :, None].expand_as(bound)
    inside = (ref["m"].abs() <= bound) & kept
    return int(inside.sum()), int(kept.sum())


# =====================================================================================================================
# regulariser
# =====================================================================================================================
@dataclass(frozen=True)
class RegCase:
    id: str
    B: int
    coef: Tuple[float, float, float]         # ckl, cgs, cpt (already divided by B by the caller)
    g_loss: float
    special: Tuple[str, ...] = ()            # per sample: "", "ones" (rows with exact 1.0), "allrows" (pt = 0), "zerograph"


REG_CASES = [
    RegCase("B1-plain", 1, (0.4, 0.4, 0.4), 1.0, ("",)),
    RegCase("B3-ones-allrows-zerograph", 3, (0.4 / 3, 0.25 / 3, 0.7 / 3), -1.75, ("ones", "allrows", "zerograph")),
    RegCase("B3-ckl0", 3, (0.0, 0.5, 0.3), 0.5, ("ones", "", "zerograph")),
    RegCase("B1-cpt0", 1, (0.3, 0.2, 0.0), 2.0, ("ones",)),
]


@_f32
def reg_inputs(case: RegCase):
    g = gen_of(case.id, 5)
    adj = torch.rand(case.B, 64, 64, generator=g) * 0.08          # small entries: the row products stay O(0.1)
    adj[:, 40:] = torch.rand(case.B, 24, 64, generator=g)         # rows uniform in (0, 1): products of O(1e-28)
    graph = (torch.rand(case.B, 64, 64, generator=g) < 0.4).float()
    adj[:, 7, ::9] = 0.0                                          # entries that are exactly 0
    for b, sp in enumerate(case.special):
        if sp == "ones":
            adj[b, 3, 17] = 1.0                                   # one exact 1.0: P_3 = 0
            adj[b, 11, 0] = 1.0
            adj[b, 11, 63] = 1.0                                  # two: every exclusive product of the row is 0 too
        elif sp == "allrows":
            adj[b, torch.arange(64), (torch.arange(64) * 5) % 64] = 1.0
        elif sp == "zerograph":
            graph[b] = 0.0
    return dict(adj=adj, graph=graph, uni=torch.rand(case.B, 4096, generator=g))


def exclusive_products(q, shift=0):
    """others[..., j] = prod_{j' != j} q[..., j'] from exclusive prefix and suffix products (exact when a factor is 0).
    shift != 0: the prefix taken one lane off -- a deliberately wrong variant for the host test."""
    one = torch.ones_like(q[..., :1])
    pre = torch.cat([one, torch.cumprod(q, -1)[..., :-1]], -1)
    suf = torch.cat([torch.cumprod(q.flip(-1), -1)[..., :-1].flip(-1), one], -1)
    if shift:
        pre = torch.roll(pre, shift, -1)
    return pre * suf


def reg_ref(adj, graph, uni, ckl, cgs, cpt, g_loss=1.0, shift=0):
    """part4 [B,4] = {KL_b, ||graph_b||_F, ||prod_j (1 - adj_b[i,j])||_2, ckl KL + cgs ||.||_F + cpt ||.||_2} and the analytic
    gradients of g_loss * sum_b part4[b,3]; the gradient of a zero norm is 0."""
    adj, graph, uni = d(adj), d(graph), d(uni)
    B = adj.shape[0]
    la = torch.log_softmax(adj.reshape(B, -1), -1)
    lt = torch.log_softmax(uni.reshape(B, -1), -1)
    kl = (lt.exp() * (lt - la)).sum(-1)
    gs = graph.reshape(B, -1).norm(dim=-1)
    q = 1.0 - adj
    P = q.prod(-1)                                                # [B,64]
    pt = P.norm(dim=-1)
    part4 = torch.stack([kl, gs, pt, ckl * kl + cgs * gs + cpt * pt], 1)
    others = exclusive_products(q, shift)
    kpt = torch.where(pt > 0, cpt / pt.clamp(min=1e-300), torch.zeros_like(pt))
    kgs = torch.where(gs > 0, cgs / gs.clamp(min=1e-300), torch.zeros_like(gs))
    d_adj = g_loss * (ckl * (la.exp() - lt.exp()).view_as(adj) - kpt[:, None, None] * P[:, :, None] * others)
    d_graph = g_loss * kgs[:, None, None] * graph
    return dict(part4=part4, d_adj=d_adj, d_graph=d_graph, others=others, P=P)


# =====================================================================================================================
# blend + softmax, latent cross-entropy
# =====================================================================================================================
@dataclass(frozen=True)
class RowCase:
    id: str
    R: int
    D: int
    Hs: int = 2
    g_loss: float = 1.0


BS_CASES = [RowCase("R1-D1-H1", 1, 1, 1), RowCase("R3-D10-H2", 3, 10, 2), RowCase("R5-D20-H1", 5, 20, 1), RowCase("R5-D63-H2", 5, 63, 2),
            RowCase("R130-D64-H2", 130, 64, 2), RowCase("R130-D20-H1", 130, 20, 1), RowCase("R1-D64-H2", 1, 64, 2)]
CE_CASES = [RowCase("R1-D1", 1, 1, g_loss=-0.5), RowCase("R3-D10", 3, 10, g_loss=2.5), RowCase("R5-D20", 5, 20), RowCase("R5-D63", 5, 63, g_loss=0.3),
            RowCase("R130-D64", 130, 64, g_loss=-1.25), RowCase("R1-D64", 1, 64)]


@_f32
def bs_inputs(case: RowCase):
    g = gen_of(case.id, 7)
    y = torch.randn(case.R, case.Hs, case.D, generator=g) * 3
    if case.D > 1:
        y[0, :, 0] = 80.0                                         # +-80: max subtraction
        y[0, :, case.D - 1] = -80.0
        if case.R > 2:
            y[2, 0] = 80.0
            y[2, case.Hs - 1, 1] = -80.0
    mask = torch.rand(case.R, generator=g)
    mask[::3] = 0.0
    mask[1::3] = 1.0
    return dict(y=y, mask=mask if case.Hs == 2 else None, g=torch.randn(case.R, case.D, generator=g))


def blend_softmax_ref(y, mask, g=None):
    y = d(y).requires_grad_(True)
    m = d(mask).requires_grad_(True) if mask is not None else None
    v = y[:, 0] if m is None else y[:, 0] * (1 - m[:, None]) + y[:, 1] * m[:, None]
    probs = torch.softmax(v, -1)
    res = dict(probs=probs.detach())
    if g is not None:
        probs.backward(d(g))
        res.update(dy=y.grad, dmask=None if m is None else m.grad)
    return res


@_f32
def ce_inputs(case: RowCase):
    g = gen_of(case.id, 9)
    p = torch.softmax(torch.randn(case.R, case.D, generator=g) * 2, -1)
    tgt = torch.randint(0, case.D, (case.R,), generator=g)
    tgt[0] = 0
    tgt[-1] = case.D - 1
    if case.D >= 10:
        for r in range(case.R):                                   # exact zeros and values inside (0, 1e-4), at and off the target
            p[r, (r + 1) % case.D] = 0.0
            p[r, (r + 4) % case.D] = 3e-5
            if r % 4 == 1:
                p[r, tgt[r]] = 0.0
            if r % 4 == 2:
                p[r, tgt[r]] = 7e-5
            if r % 4 == 3:
                p[r, (r + 6) % case.D] = BOUND                    # exactly the bound: no gradient (at or below)
    return dict(probs=p, target=tgt)


def latent_ce_ref(probs, target, g_loss=1.0):
    """row_loss[r] = logsumexp(lp) - lp[target], lp = log(max(p, 1e-4)); d_probs of g_loss * mean(row_loss), zero at or below
    the bound."""
    p = d(probs)
    R = p.shape[0]
    lp = torch.log(p.clamp(min=BOUND))
    row = torch.logsumexp(lp, -1) - lp.gather(1, target.view(-1, 1)).squeeze(1)
    dlp = (torch.softmax(lp, -1) - torch.nn.functional.one_hot(target, p.shape[1])) * (g_loss / R)
    return dict(row_loss=row, d_probs=torch.where(p > BOUND, dlp / p.clamp(min=BOUND), torch.zeros_like(p)))


# =====================================================================================================================
# intervention mask, straight-through Bernoulli sample
# =====================================================================================================================
@dataclass(frozen=True)
class MaskCase:
    id: str
    B: int
    A: int
    keep: bool


MASK_CASES = [MaskCase("A1-B1", 1, 1, False), MaskCase("A5-B3-keep", 3, 5, True), MaskCase("A12-B3", 3, 12, False),
              MaskCase("A20-B1-keep", 1, 20, True), MaskCase("A5-B1", 1, 5, False)]


def positional_table(S=64, D=64):
    pos = torch.arange(S).unsqueeze(1)
    div = torch.exp(torch.arange(0, D, 2) * (-np.log(10000.0) / D))
    pe = torch.zeros(S, D)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


@_f32
def mask_inputs(case: MaskCase):
    g = gen_of(case.id, 11)
    B, A = case.B, case.A
    x = torch.nn.functional.one_hot(torch.randint(0, 64, (B, 64), generator=g), 64).float()
    action = torch.nn.functional.one_hot(torch.randint(0, A, (B,), generator=g), A).float()
    keep = (torch.rand(B, 64, 64, generator=g) < 0.9).float() if case.keep else None
    return dict(x=x, action=action, pe=positional_table(), keep=keep, scale=float(np.float32(1 / 0.9)) if case.keep else 1.0,
                W=torch.randn(64, A + 64, generator=g) * 0.3, bias=torch.randn(64, generator=g) * 0.3,
                expo=torch.empty(B, 64, 2).exponential_(generator=g).clamp_(min=1e-6), g=torch.randn(B, 64, generator=g))


def st_sample(p, expo):
    """a0, a1, soft = sigmoid(a1 - a0), hard = [a1 > a0] and d (a1 - a0) / d p of the 2-class Gumbel-softmax of
    log(clamp([1 - p, p], 1e-4)) with Gumbel noise -log(expo)."""
    a0 = torch.log((1 - p).clamp(min=BOUND)) - torch.log(expo[..., 0])
    a1 = torch.log(p.clamp(min=BOUND)) - torch.log(expo[..., 1])
    soft = torch.sigmoid(a1 - a0)
    dd = torch.where(p > BOUND, 1 / p.clamp(min=BOUND), torch.zeros_like(p)) \
        + torch.where((1 - p) > BOUND, 1 / (1 - p).clamp(min=BOUND), torch.zeros_like(p))
    return a0, a1, soft, (a1 > a0).to(p.dtype), dd


def mask_ref(x, action, pe, keep, scale, W, bias, expo, g=None):
    x, action, pe, W, bias, expo = d(x), d(action), d(pe), d(W), d(bias), d(expo)
    B, S, D = x.shape
    pos = pe.expand(B, S, D) * (d(keep) * scale if keep is not None else 1.0)
    inp = torch.cat([action[:, None, :].expand(B, S, action.shape[1]), pos], -1)                 # [B,S,A+D]
    z = inp @ W.t() + bias
    z_abs = inp.abs() @ W.abs().t() + bias.abs()
    inter = torch.sigmoid(z)
    p = (x * inter).sum(-1)
    a0, a1, soft, hard, dd = st_sample(p, expo)
    res = dict(inter=inter, p=p, a0=a0, a1=a1, soft=soft, sample=hard, z_abs=z_abs)
    if g is not None:
        dp = d(g) * soft * (1 - soft) * dd
        dz = dp[..., None] * x * inter * (1 - inter)
        res.update(dWp=torch.einsum("bsi,bsd->bid", inp, dz), dbp=dz.sum(1))
    return res


def mask_error_bounds(case: MaskCase, inp, ref):
    """Float32 error bounds of the mask kernel's inter / p and of its decision variable a1 - a0.
    z is a float32 dot product of length A + 64 plus the bias, pos itself a product of three floats (2 roundings):
      |z32 - z| <= (A + 64 + 3) * 2^-23 * (|in| @ |W| + |bias|);
    sigmoid has slope <= 1/4 and is evaluated with __expf and a division: a few ulp of a value <= 1 -> + 4 * 2^-23;
    x is one-hot, so p is one inter value (adding zeros is exact);
    log(max(p, 1e-4)) moves by at most dp / max(p, 1e-4), log(max(1 - p, 1e-4)) by dp' / max(1 - p, 1e-4) where 1 - p adds one
    rounding; each __logf adds its own error: 2^-21 absolute near 1, a few ulp relative elsewhere -> 8 * 2^-23 * (1 + |log|).
    The two intrinsic terms (4 * 2^-23 for the sigmoid, 8 * 2^-23 * (1 + |log|) per __logf) are ASSUMED accuracies of __expf /
    __logf / the division taken from the published ulp figures of the fast-math intrinsics; they are not derived from operand
    rounding and were not measured.  They serve as the exclusion margin and as the tolerance of inter / p / soft alike."""
    L = case.A + 64 + 3
    d_inter = 0.25 * L * EPS32 * ref["z_abs"] + 4 * EPS32
    d_p = (d(inp["x"]) * d_inter).sum(-1)
    p, e = ref["p"], d(inp["expo"])
    logs = [torch.log(p.clamp(min=BOUND)), torch.log((1 - p).clamp(min=BOUND)), torch.log(e[..., 0]), torch.log(e[..., 1])]
    d_a = d_p / p.clamp(min=BOUND) + (d_p + 2.0 ** -24) / (1 - p).clamp(min=BOUND) + sum(8 * EPS32 * (1 + l.abs()) for l in logs)
    return d_inter, d_p, d_a


SAMPLE_N = [1, 3, 255, 256, 257, 4101]


@_f32
def sample_inputs(n: int):
    g = gen_of(f"sample-n{n}", 13)
    p = torch.rand(n, generator=g)
    special = [0.0, 1.0, 3e-5, 1 - 3e-5, BOUND, 0.5]
    for i, v in enumerate(special[:n] if n < 6 else special):
        p[(i * 37) % n if n >= 6 else i] = v
    return dict(p=p, expo=torch.empty(n, 2).exponential_(generator=g).clamp_(min=1e-6), g_s=torch.randn(n, generator=g),
                g_w=torch.randn(n, generator=g))


def sample_ref(p, expo, g_s=None, g_w=None):
    p, expo = d(p), d(expo)
    a0, a1, soft, hard, dd = st_sample(p, expo)
    gs = (d(g_s) if g_s is not None else 0.0) + (d(g_w) * p if g_w is not None else 0.0)
    g_p = gs * soft * (1 - soft) * dd + (d(g_w) * hard if g_w is not None else 0.0)
    return dict(a0=a0, a1=a1, soft=soft, sample=hard, weighted=p * hard, g_p=g_p)


def sample_margin(p, expo):
    """Float32 bound of |(a1 - a0)32 - (a1 - a0)| for ct_sample (p is an input, so exact): 1 - p adds one rounding (2^-24
    absolute), moved by 1 / max(1 - p, 1e-4) through the log; each of the four __logf adds 8 * 2^-23 * (1 + |log|) as in
    mask_error_bounds (an assumed, not measured, accuracy of the intrinsic); the three subtractions add one ulp of the partial
    results each."""
    p, e = d(p), d(expo)
    logs = [torch.log(p.clamp(min=BOUND)), torch.log((1 - p).clamp(min=BOUND)), torch.log(e[..., 0]), torch.log(e[..., 1])]
    return 2.0 ** -24 / (1 - p).clamp(min=BOUND) + sum((8 + 2) * EPS32 * (1 + l.abs()) for l in logs)


# =====================================================================================================================
# pair scorer
# =====================================================================================================================
@dataclass(frozen=True)
class PairCase:
    id: str
    B: int
    N: int
    H: int
    pad: int                     # u | v are column blocks of one buffer of row stride 2*H + pad; d_u | d_v likewise (+ 4)
    row_of: Optional[Tuple[int, ...]] = None      # per-sample scorer rows (None: one shared scorer)
    G: int = 1


PAIR_CASES = [PairCase("N1-H8", 2, 1, 8, 4), PairCase("N37-H40-rows", 4, 37, 40, 8, row_of=(2, 0, 2, 3), G=5),
              PairCase("N37-H33-shared", 2, 37, 33, 3), PairCase("N1-H5-rows", 3, 1, 5, 1, row_of=(1, 1, 0), G=3)]


@_f32
def pair_inputs(case: PairCase):
    g = gen_of(case.id, 15)
    return dict(u=torch.randn(case.B, case.N, case.H, generator=g), v=torch.randn(case.B, case.N, case.H, generator=g),
                w2=torch.randn(case.G, case.H, generator=g) / case.H ** 0.5, b2=torch.randn(case.G, generator=g),
                row_of=None if case.row_of is None else torch.tensor(case.row_of, dtype=torch.int32),
                g=torch.randn(case.B, case.N, case.N, generator=g))


def pair_mlp_ref(u, v, w2, b2, row_of, slope, g=None):
    """out[b,i,j] = sigmoid(b2 + sum_h w2[h] lrelu(u[b,i,h] + v[b,j,h])); per-sample partials of w2 / b2."""
    B = u.shape[0]
    u, v = d(u).requires_grad_(True), d(v).requires_grad_(True)
    rows = row_of.long() if row_of is not None else torch.zeros(B, dtype=torch.long)
    w = d(w2)[rows].clone().requires_grad_(True)                  # [B,H]
    b = d(b2)[rows].clone().requires_grad_(True)                  # [B]
    t = u[:, :, None, :] + v[:, None, :, :]
    out = torch.sigmoid((torch.nn.functional.leaky_relu(t, slope) * w[:, None, None, :]).sum(-1) + b[:, None, None])
    res = dict(out=out.detach(), t=t.detach())
    if g is not None:
        out.backward(d(g))
        res.update(d_u=u.grad, d_v=v.grad, d_w2=w.grad, d_b2=b.grad)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# pair scorer, the 64-node kernels: dispatch mirror, cases, analytic float64 reference with its |.| sums, rounding chains
# ---------------------------------------------------------------------------------------------------------------------
FWD64B, FWD64, FWD, BWD64, BWD = ("pair_mlp_fwd64b_kernel", "pair_mlp_fwd64_kernel", "pair_mlp_fwd_kernel", "pair_mlp_bwd64_kernel",
                                  "pair_mlp_bwd_kernel")
SLOPE_PAIR32 = float(np.float32(SLOPE_PAIR))     # the slope as the kernels receive it: both sides see the same number
STEP_MIN = 2.0 ** -60                            # satmath.hpp: [t > 0] = sat(t * 2^60) is exact for t <= 0 and t >= 2^-60


def pair_kernels(N, H, ld, u_al=True, v_al=True, out_al=True, w2_al=True):
    """(forward kernel, backward kernel or None = refused) as launch_pair_mlp_forward / _backward choose them; *_al: the pointer is
    16-byte aligned.  Bank rows sit H floats apart, so with H % 4 == 0 every row is aligned as the bank is."""
    vec = N == 64 and H % 4 == 0 and ld % 4 == 0 and u_al and v_al and out_al
    fwd = (FWD64B if w2_al else FWD64) if vec else FWD
    bwd = None if N > 64 else BWD64 if N == 64 else BWD
    return fwd, bwd


@dataclass(frozen=True)
class Pair64Case:
    id: str
    B: int
    N: int
    H: int
    fwd: str                     # the kernels the case is there to reach; the mirror and the launch log must both agree
    bwd: Optional[str]           # None: the backward refuses (N > 64)
    ld: int = 0                  # row stride of the buffer holding u | v (0: 2H)
    dpad: int = 4                # d_u | d_v sit at the same columns of a buffer of row stride ldd = ld + dpad
    ucol: int = 0                # u occupies columns ucol .. ucol + H - 1, v the H columns behind it
    uvoff: int = 0               # the u | v buffer, the scorer bank and out start this many floats behind a 16-byte boundary
    w2off: int = 0
    outoff: int = 0
    bias: bool = True            # False: b2 == NULL in the forward
    row_of: Optional[Tuple[int, ...]] = None      # per-sample scorer rows (None: one shared scorer, row 0 of the bank)
    G: int = 1

    @property
    def ld_(self):
        return self.ld or 2 * self.H

    @property
    def ldd_(self):
        return self.ld_ + self.dpad

    def alignment(self):
        """u, v, out, w2 16-byte aligned?"""
        return ((self.uvoff + self.ucol) % 4 == 0, (self.uvoff + self.ucol + self.H) % 4 == 0, self.outoff % 4 == 0, self.w2off % 4 == 0)


def _p64(H, **k):
    return Pair64Case(k.pop("id", f"H{H}"), k.pop("B", 2), 64, H, k.pop("fwd", FWD64B), BWD64, **k)


ROWS = dict(row_of=(2, 4, 2), G=5)               # a repeated row (2) and unused rows (0, 1, 3)
PAIR64_CASES = [
    # one partial chunk in both forwards; one live backward wave, ha lanes 4..15 and every hb lane clamped
    _p64(4, B=1), _p64(4, id="H4-w2off", fwd=FWD64, w2off=1, B=1), _p64(4, id="H4-w2off-rows", fwd=FWD64, w2off=1, B=3, **ROWS),
    # exactly one backward wave, half a 64b chunk, one full fwd64 chunk
    _p64(32), _p64(32, id="H32-w2off", fwd=FWD64, w2off=1, B=1),
    # second backward wave with 4 live ha lanes, every hb clamped
    _p64(36, ld=2 * 36 + 8), _p64(36, id="H36-w2off", fwd=FWD64, w2off=1), _p64(36, id="H36-w2off-rows", fwd=FWD64, w2off=1, B=3, **ROWS),
    # 64b chunk boundary / buffer swap: full, exactly full, nearly empty last chunk
    _p64(60, B=1), _p64(64, B=1, dpad=0), _p64(68), _p64(68, id="H68-w2off", fwd=FWD64, w2off=1), _p64(68, id="H68-w2off-rows", fwd=FWD64, w2off=1, B=3, **ROWS),
    # second backward workgroup whose waves 1..3 return behind the barriers; three 64b chunks
    _p64(132, B=1),
    # the model's layout uv = [u0 | v0 | ua | va]: pair 0 with the shared scorer (row 0), pair 1 with the rows of row_of
    _p64(48, id="H48-model-pair0", B=3, ld=4 * 48, G=5), _p64(48, id="H48-model-pair1", B=3, ld=4 * 48, ucol=2 * 48, **ROWS),
    # the generic forward in front of the 64-node backward
    _p64(5, fwd=FWD, ld=2 * 5 + 1), _p64(33, fwd=FWD, ld=2 * 33 + 1, B=3, **ROWS), _p64(36, id="H36-ldodd", fwd=FWD, ld=2 * 36 + 3),
    _p64(36, id="H36-uvoff", fwd=FWD, uvoff=1), _p64(36, id="H36-outoff", fwd=FWD, outoff=1, B=1), _p64(68, id="H68-ldodd", fwd=FWD, ld=2 * 68 + 3),
    # b2 == NULL on each of the three forwards
    _p64(36, id="H36-nobias", bias=False, B=1), _p64(36, id="H36-w2off-nobias", fwd=FWD64, w2off=1, bias=False, B=1),
    _p64(33, id="H33-nobias", fwd=FWD, bias=False, B=1),
    # the generic kernels at the register bound; the forward's j0 loop in front of a backward that must refuse
    Pair64Case("N63-H33", 2, 63, 33, FWD, BWD, ld=2 * 33 + 3), Pair64Case("N65-H5", 1, 65, 5, FWD, None),
]
PAIR_SCALE_CASES = ("H68", "H68-w2off", "H68-ldodd")     # the power-of-two metamorphic case on every forward kernel
PAIR_SCALE_K = (20, -20)


def pair_chain(kernel, N, H):
    """L of dot_bound: the longest chain of float32 roundings between an input and one output element, read off csrc/pairmlp.hip
    (line numbers of that file).  Additions of staged zeros count: L depends on the shape only.  slope itself is given to the
    reference as the float32 the kernel receives (SLOPE_PAIR32), so it adds nothing."""
    if kernel == FWD64B:
        # 216 oms = 1 - slope (1); 232 w2 * oms (1); 243 the clamped add t (1); 243-244 a wave's fmas, 16 per chunk of 64 (16 nch);
        # 264 the merge of the four waves (3); 269 + slope * (...) + bias (2).  The linear part is one shorter: 225 a term's own
        # product (1, none if contracted) and the adds behind it (16 nch in a thread), 248 quad (2), 269 al + ar, * slope, two adds (4).
        nch = -(-H // 64)
        return dict(out=16 * nch + 8)
    if kernel == FWD64:
        # 139 w2 * (1 - slope) (2); 150 t (1); 151-152 one thread's fmas over every h, 32 per chunk (32 nch); 169 two adds (2).
        # linear part: 128 three roundings per j, four j per chunk (12 nch); 156-157 (2); 169 (4)
        nch = -(-H // 32)
        return dict(out=32 * nch + 5)
    if kernel == FWD:
        # 67 t (1); 68 t * slope (1); 69 a term's own product (1, none if contracted) and the adds behind it -- one packed half takes
        # every other h: 16 per chunk of 32 (16 nch); 73 the two halves (1); 74 + bias (1)
        nch = -(-H // 32)
        return dict(out=16 * nch + 5)
    if kernel == BWD64:
        # G = g * s * (1 - s): 375 (3).  The step is exact (0 or 1), so g * step is exact and each fma rounds once.
        # d_b2: 383 row sums (64), 386 wave_sum (6)
        # d_u : 383 RS (64) or 428-429 A (64 fmas, one per column); 450 slope * RS (1); 402 oms (1); 451 fma (1); 453 * w (1)
        # d_v : 392 CS (64) or 428-433 (8 fmas, 1 add, 2 quad); 434, 435 as for d_u (3); 440 * w (1)
        # d_w2: the d_v chain up to 435 (3 + 64 + 3), then 436 dwj, 64 fmas (64), 460 the final add (1); 2^60 / 2^-60 are exact.
        #       (the u side is shorter: 452 16 fmas, 457 quad 2)
        return dict(d_b2=3 + 64 + 6, d_u=3 + 64 + 4, d_v=3 + 64 + 4, d_w2=3 + 64 + 3 + 64 + 1)
    if kernel == BWD:
        # gs: 293 (3).  d_b2: 296 16 adds per thread, block_sum_256 (6 + 3).
        # d_u : 324 g * sl (1), 325 one add per column (N), 336 * w (1);  d_v: 324 (1), 326 32 adds per half (32), 330 (2)
        # d_w2: 322 t (1), 324 (1), 327 a term's own product (1) and the adds behind it, 32 per column in a packed half (32 N), 332 (1)
        return dict(d_b2=3 + 16 + 9, d_u=3 + 1 + N + 1, d_v=3 + 1 + 32 + 2, d_w2=3 + 3 + 32 * N + 1)
    raise ValueError(kernel)


def pair_terms(u, v, w2, b2, row_of, slope, g=None, out32=False, mutate=None, hdrop=0):
    """The pair scorer written out in float64 with analytic gradients, and the sums of absolute values behind every result.
    b2 None: no bias.  out32: G = g s (1 - s) is formed from this forward's out rounded to float32 -- what the backward kernel is
    handed when it is tested alone -- instead of the float64 values.  `*_abs` are the |.| sums of the generic kernels, `*_abs_split`
    those of the 64-node kernels, which take lrelu(t) = slope t + (1 - slope) relu(t) apart, and t = u + v with it.
    mutate: a deliberately wrong variant for the host test --
      "drop_tail"   hidden units H - hdrop .. H - 1 never arrive (forward: not summed; backward: their gradients stay 0)
      "ignore_rows" row_of is ignored, sample b reads row b
      "no_linear"   the forward omits slope * (al + ar)
      "transpose_g" the backward reads G[j,i]
      "step_ge"     the backward's step function is [t >= 0]
      "double_last" d_w2 counts unit H - 1 twice"""
    B, _, H = u.shape
    u, v, w2 = d(u), d(v), d(w2)
    rows = row_of.long() if row_of is not None else torch.zeros(B, dtype=torch.long)
    if mutate == "ignore_rows":
        rows = torch.arange(B)
    w = w2[rows]                                                          # [B,H]
    b = d(b2)[rows] if b2 is not None else torch.zeros(B, dtype=torch.float64)
    live = torch.ones(H, dtype=torch.float64)
    if mutate == "drop_tail":
        live[H - hdrop:] = 0.0
    t = u[:, :, None, :] + v[:, None, :, :]                               # [B,i,j,h]
    pos = (t >= 0) if mutate == "step_ge" else (t > 0)
    relu = t.clamp(min=0)
    lr = torch.where(t > 0, t, slope * t)
    wl = (w * live)[:, None, None, :]
    pre = ((1 - slope) * relu * wl).sum(-1) + b[:, None, None]
    if mutate != "no_linear":
        pre = pre + slope * (t * wl).sum(-1)
    res = dict(out=torch.sigmoid(pre), t=t)
    mag = u.abs()[:, :, None, :] + v.abs()[:, None, :, :]
    aw = w.abs()[:, None, None, :]
    res["out_abs"] = b.abs()[:, None, None] + (aw * lr.abs()).sum(-1)
    res["out_abs_split"] = b.abs()[:, None, None] + (aw * ((1 - slope) * relu + slope * mag)).sum(-1)
    if g is None:
        return res
    s = res["out"].float().double() if out32 else res["out"]
    G = d(g) * s * (1 - s)
    if mutate == "transpose_g":
        G = G.transpose(1, 2)
    dl = torch.where(pos, torch.ones_like(t), torch.full_like(t, slope))
    Ga = G.abs()
    res["d_u"] = w[:, None, :] * torch.einsum("bij,bijh->bih", G, dl) * live
    res["d_v"] = w[:, None, :] * torch.einsum("bij,bijh->bjh", G, dl) * live
    res["d_w2"] = torch.einsum("bij,bijh->bh", G, torch.where(pos, t, slope * t)) * live
    if mutate == "double_last":
        res["d_w2"][:, H - 1] *= 2.0
    res["d_b2"] = G.sum((1, 2))
    res["d_u_abs"] = w.abs()[:, None, :] * Ga.sum(2)[:, :, None].expand(-1, -1, H)
    res["d_v_abs"] = w.abs()[:, None, :] * Ga.sum(1)[:, :, None].expand(-1, -1, H)
    res["d_w2_abs"] = torch.einsum("bij,bijh->bh", Ga, lr.abs())
    res["d_w2_abs_split"] = torch.einsum("bij,bijh->bh", Ga, dl * mag)
    res["d_b2_abs"] = Ga.sum((1, 2))
    for k in ("d_u", "d_v", "d_b2"):
        res[k + "_abs_split"] = res[k + "_abs"]
    return res


def pair_abs(res, name, kernel):
    """The |.| sum behind result `name` as `kernel` forms it."""
    return res[name + ("_abs" if kernel in (FWD, BWD) else "_abs_split")]


def pair_out_tol(L, out_abs):
    """|sigmoid'| <= 1/4 times the dot-product bound of the pre-activation, plus the 2e-6 the project allows __expf and the
    division (test_ct_gpu.test_pair_mlp_kernel)."""
    return 0.25 * dot_bound(L, out_abs) + 2e-6


def pair_sums32(u, v):
    """Every float32 sum u[b,i,h] + v[b,j,h], as the kernels form it."""
    return u.float()[:, :, None, :] + v.float()[:, None, :, :]
