"""Shared by tests/test_wgrad_reference_host.py (CPU) and tests/test_wgrad_ops_gpu.py (GPU): float64 references of
ctvae_conv_wgrad in the library's own layouts, the two input regimes with their bounds, a Python mirror of launch_wgrad's kernel
selection (csrc/wgrad.hip) and the case lists.  Pure torch: importable without a GPU and without the library.

Layouts: x [B,H,W,Ci] and dy [B,Ho,Wo,Co] are NHWC; dW is the packed block [tap][Ci][Co] (tap = ky*k + kx), with CTVAE_W_CI_TAP
the Linear block [Ci][tap][Co]; dbias [Co].

Reference.  wgrad_ref() is the im2col GEMM of the forward tap geometry (csrc/geom.hpp build_geom, ported in build_geom() below and
pinned to torch's float64 autograd in the host test):

    dW[wtap(t)][c][n] = sum_m x'[gpix(m, t)][c] * g[spix(m)][n]          dbias[n] = sum_m g[spix(m)][n]

Transforms on load:
  InXform  x' = act(x*scale[c] + shift[c]) inside the image, 0 in the padding.
  DyXform  g  = k1*g_a*act'(y*scale + shift) + k2*y + k3 per output channel, coef rows 0..4 = k1, k2, k3, scale, shift
           (act'(t) = 1 for t > 0, else the slope: 0.01 LeakyReLU, 0 ReLU, 1 none).  The transposed-conv kernel writes g to
           gy_out.  The encoder kernel (csrc/image.hip img_enc_wgrad_kernel) writes no g; with dgamma / dbeta given its block 0
           commits  dgamma[c] = (bn_accumulate ? dgamma[c] : 0) + coef[5][c],  dbeta[c] = (...) + coef[6][c]  -- rows 5 and 6 are
           taken as they are, one float32 addition each.

Regimes.  `int`: x, dy and every coefficient are small integers, every partial sum of every order stays below 2^24
(int_exact_margin(), asserted per case on the host), so float32 arithmetic is exact in any order and the GPU result must equal
the reference bit for bit.  `randn`: O(1) data; a sum of terms t_i evaluated in float32 in ANY order whose longest chain of
additions has L links satisfies |err| <= gamma_L * sum |t_i|, gamma_L = L u / (1 - L u), u = 2^-24 (Higham, Accuracy and
Stability of Numerical Algorithms, 4.2).  chain_links() gives L per kernel family from its loop structure alone: the tile
kernels add chunks_per_split * 32 pixels in a row and then S slabs; the persistent kernels add at most (tiles per workgroup) *
(pixels per tile) terms inside a workgroup in whatever order, then their slabs.  The transforms' own roundings are added
per term (apply_in_xform(), apply_dy_xform()).  Nothing here was tuned on a kernel."""
import math
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn.functional as F

U = 2.0 ** -24
ACT_NONE, ACT_LRELU, ACT_RELU = 0, 1, 2
CONV, CONVT, W_CI_TAP = 0, 1, 0x100
ERR_BAD_ARG, ERR_WORKSPACE = -22, -12
WS_BYTES = 256 << 20          # ctvae_workspace_bytes()
MC = 32                       # pixels per chunk (csrc/wgrad_fast.hpp)
REDUCE_WIDE_ITEMS = 65536
DEFER_JOBS_PER_LAUNCH = 24
UP_WS_FLOATS = 512 * (9 * 32 * 32 + 32)
ENC_WS_FLOATS = 512 * (27 * 32 + 32)
THIN_WGS, UP_WGS, IMG_WGS, ENC_WGS = 768, 512, 512, 512


def ceil_div(a, b):
    return -(-a // b)


def slope(act):
    return {ACT_NONE: 1.0, ACT_LRELU: 0.01, ACT_RELU: 0.0}[act]


# ---------------------------------------------------------------------------------------------------------------------
# geometry (csrc/geom.hpp build_geom, forward kinds 0 / 1)
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Geom:
    B: int
    gH: int
    gW: int
    gC: int
    sH: int
    sW: int
    sC: int
    Qh: int
    Qw: int
    is_: int
    os: int
    k: int
    flat: bool
    py: list = field(default_factory=list)
    px: list = field(default_factory=list)
    taps: list = field(default_factory=list)      # per class: [(dy, dx, wtap)]

    @property
    def ncls(self):
        return len(self.taps)

    @property
    def ntaps(self):
        return [len(t) for t in self.taps]

    @property
    def taps_total(self):
        return sum(self.ntaps)

    @property
    def Mc(self):
        return self.B * self.Qh * self.Qw

    @property
    def packed(self):                      # packed_weights(): a CI_TAP block is packed only when it has one tap
        return (not self.flat) or self.k == 1


def build_geom(kind, B, H, W, Ci, Co, k, s, p, op):
    base, flat = kind & ~W_CI_TAP, bool(kind & W_CI_TAP)
    tr = base == CONVT
    if tr:
        Ho, Wo = (H - 1) * s - 2 * p + k + op, (W - 1) * s - 2 * p + k + op
    else:
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    assert Ho > 0 and Wo > 0 and s in (1, 2)
    if not tr:
        assert k * k <= 16
        if s == 2:
            taps = [(ky - p, kx - p, ky * k + kx) for qy in range(2) for qx in range(2) for ky in range(k) for kx in range(k)
                    if ((ky - p) & 1) == (qy ^ 1) and ((kx - p) & 1) == (qx ^ 1)]
        else:
            taps = [(ky - p, kx - p, ky * k + kx) for ky in range(k) for kx in range(k)]
        return Geom(B, H, W, Ci, Ho, Wo, Co, Ho, Wo, s, 1, k, flat, [0], [0], [taps])
    assert Ho % s == 0 and Wo % s == 0 and not flat
    g = Geom(B, H, W, Ci, Ho, Wo, Co, Ho // s, Wo // s, 1, s, k, False)
    for c in range(s * s):
        py, px = c // s, c % s
        taps = []
        for ky in range(k):
            if (py + p - ky) % s:
                continue
            for kx in range(k):
                if (px + p - kx) % s:
                    continue
                taps.append((int((py + p - ky) / s), int((px + p - kx) / s), ky * k + kx))     # C++: truncation (exact multiple)
        assert len(taps) <= 16
        g.py.append(py); g.px.append(px); g.taps.append(taps)
    return g


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    hits: str                    # what the case is there to hit
    kind: int
    B: int
    H: int
    W: int
    Ci: int
    Co: int
    k: int
    s: int
    p: int
    op: int = 0
    xf: int = -1                 # InXform activation, -1: none (randn regime: this one; int regime: ReLU unless NONE)
    dyx: int = -1                # DyXform activation, -1: none
    dy_out: str = ""             # "gy" (gy_out) or "commit" (dgamma / dbeta)
    wino: bool = False
    ws_floats: Optional[int] = None     # workspace handed to the call (None: all of it)
    bias: bool = True
    expect: tuple = ()           # kernel label the case must log
    S: Optional[int] = None      # number of slabs it must reduce
    red: Optional[tuple] = None  # (small, vec) of the weight job
    rc: int = 0

    def args(self):
        return (self.kind, self.B, self.H, self.W, self.Ci, self.Co, self.k, self.s, self.p, self.op)

    def geom(self):
        return build_geom(*self.args())

    def ws(self):
        return WS_BYTES // 4 if self.ws_floats is None else self.ws_floats


# ---------------------------------------------------------------------------------------------------------------------
# mirror of launch_wgrad's selection (csrc/wgrad.hip, thin.hip, upconv.hip, image.hip, wino.hip)
# ---------------------------------------------------------------------------------------------------------------------
def _taps_within(g, lo, hi):
    return all(lo <= dy <= hi and lo <= dx <= hi for cl in g.taps for dy, dx, _ in cl)


def thin_patch(g, wgrad=True):
    TH, TW = 8, 32 if g.gC == 32 else 16
    dys = [t[0] for cl in g.taps for t in cl]
    dxs = [t[1] for cl in g.taps for t in cl]
    PH = (TH - 1) * g.is_ + max(dys) - min(dys) + 1
    PW = (TW - 1) * g.is_ + max(dxs) - min(dxs) + 1
    smem = PH * PW * (g.gC + 4) * 4 + (TH * TW * 16 if wgrad else 0)
    merge = 4 * (4 if max(g.ntaps) <= 4 else 9) * 4 * 3 * (g.gC // 4) * 4 if wgrad else 0
    return PH, PW, max(smem, merge)


def thin_shape_ok(g, wgrad=True):
    if not g.packed or g.sC != 3 or g.gC not in (32, 64):
        return False
    TH, TW = 8, 32 if g.gC == 32 else 16
    if g.Qh % TH or g.Qw % TW or max(g.ntaps) > 9:
        return False
    PH, PW, smem = thin_patch(g, wgrad)
    return PH * PW < 900 and smem <= 160 * 1024


def thin_ws_floats(g):
    return THIN_WGS * (g.taps_total * g.gC * g.sC + g.ncls * g.sC)


def img_conv_supported(g):
    return (g.packed and g.gC == 32 and g.sC == 3 and g.ncls == 1 and g.is_ == 1 and g.os == 1 and g.ntaps[0] == 9 and
            g.gH == g.sH and g.gW == g.sW and g.sH % 8 == 0 and g.sW % 32 == 0 and _taps_within(g, -1, 1))


def img_enc_supported(g):
    return (g.packed and g.gC == 3 and g.sC == 32 and g.ncls == 1 and g.is_ == 2 and g.os == 1 and g.ntaps[0] == 9 and
            g.gH == 2 * g.sH and g.gW == 2 * g.sW and g.sH % 8 == 0 and g.sW % 32 == 0 and _taps_within(g, -1, 1))


def upconv_supported(g):
    return (g.packed and g.gC == 32 and g.sC == 32 and g.is_ == 1 and g.os == 2 and g.ncls == 4 and g.sH == 2 * g.gH and
            g.sW == 2 * g.gW and g.gH % 8 == 0 and g.gW % 32 == 0 and g.ntaps == [1, 2, 2, 4] and _taps_within(g, 0, 1))


def wino_wgrad_splits(g, ws_floats):
    """wino_wgrad_supported(): the split count, or 0."""
    if not (g.packed and g.is_ == 1 and g.os == 1 and g.ncls == 1 and g.ntaps[0] == 9 and g.gH == g.sH and g.gW == g.sW):
        return 0
    if [t for t in g.taps[0]] != [(a // 3 - 1, a % 3 - 1, a) for a in range(9)]:
        return 0
    if g.gH % 4 or g.gW % 8 or g.gC % 64 or g.sC % 64:
        return 0
    nchunks = g.B * (g.gH // 2) * (g.gW // 2) // 8
    out_tiles = (g.gC // 64) * (g.sC // 64)
    S = min(ceil_div(256, out_tiles), nchunks // 8)
    if S < 1 or S * out_tiles < 128:
        return 0
    while S > 1 and S * (9 * g.gC + 1) * g.sC > ws_floats:
        S -= 1
    if S * (9 * g.gC + 1) * g.sC > ws_floats:
        return 0
    cps = ceil_div(nchunks, S)
    return ceil_div(nchunks, cps)


def wgrad_ws_floats(g, S):
    return S * g.taps_total * g.gC * g.sC + S * g.ncls * g.sC


def choose_splits(g, KT, NT, ws_floats, target):
    ktiles = sum(ceil_div(n * g.gC, KT) for n in g.ntaps)
    tiles = ktiles * ceil_div(g.sC, NT)
    nchunks = ceil_div(g.Mc, MC)
    S = max(1, target // max(tiles, 1))
    S = min(S, max(1, ceil_div(nchunks, 8 if nchunks >= 32 else 4)))
    while S > 1 and wgrad_ws_floats(g, S) > ws_floats:
        S -= 1
    return S


def reduce_shape(n, S, part_off_floats=0):
    """reduce_job_blocks(): (small, vec, blocks) of one job; the slabs start part_off_floats into the (aligned) workspace."""
    if n <= 0 or S <= 0:
        return None
    vec = int(n % 4 == 0 and part_off_floats % 4 == 0)
    items = n // 4 if vec else n
    small = 1 if S <= 8 else (2 if items >= REDUCE_WIDE_ITEMS else 0)
    blocks = ceil_div(items, 256) if small == 1 else (ceil_div(items, 64) if small == 2 else ceil_div(items, 16))
    return small, vec, blocks


@dataclass
class Plan:
    rc: int = 0
    kernel: str = ""
    S: int = 0                   # slabs of the weight job
    Sb: int = 0                  # slabs of the bias job
    n: int = 0
    red_w: Optional[tuple] = None
    red_b: Optional[tuple] = None
    cps: int = 0                 # chunks per split (tile kernels)
    tiles: int = 0               # persistent kernels: tiles per class, and the grid
    nwg: int = 0
    tile_px: int = 0
    family: str = ""

    @property
    def labels(self):
        return [] if self.rc else sorted([self.kernel, "reduce_partials_kernel"])


def plan(c: Case) -> Plan:
    g, wsf = c.geom(), c.ws()
    has_xf, has_dy = c.xf >= 0, c.dyx >= 0
    want_b = c.bias

    def done(pl, n, S, Sb, bias_n):
        pl.n, pl.S, pl.Sb = n, S, Sb
        pl.red_w = reduce_shape(n, S)
        pl.red_b = reduce_shape(bias_n, Sb, S * n) if want_b else None
        return pl

    if not has_xf and not has_dy and c.wino:
        S = wino_wgrad_splits(g, wsf)
        if S:
            nchunks = g.B * (g.gH // 2) * (g.gW // 2) // 8
            return done(Plan(kernel="wino_wgrad_kernel", family="wino", cps=ceil_div(nchunks, S)), 9 * g.gC * g.sC, S, S, g.sC)
    up = upconv_supported(g) and wsf >= UP_WS_FLOATS
    enc = img_enc_supported(g) and not has_xf and wsf >= ENC_WS_FLOATS
    if has_dy and not up and not (enc and c.dy_out != "gy"):
        return Plan(rc=ERR_BAD_ARG)
    if has_dy and up and c.dy_out != "gy":
        return Plan(rc=ERR_BAD_ARG)
    if up or enc:
        tiles = g.B * (g.gH // 8) * (g.gW // 32) if up else g.B * (g.sH // 8) * (g.sW // 32)
        nwg = min(tiles, UP_WGS if up else ENC_WGS)
        pl = Plan(kernel="up_wgrad_kernel" if up else "img_enc_wgrad_kernel", family="up" if up else "enc", tiles=tiles, nwg=nwg,
                  tile_px=256)
        return done(pl, 9 * 32 * 32 if up else 27 * 32, nwg, nwg, 32)
    thin = thin_shape_ok(g) and thin_ws_floats(g) <= wsf
    if has_xf and not thin and not (g.gC % 4 == 0 and g.sC % 4 == 0):
        return Plan(rc=ERR_BAD_ARG)
    if thin:
        if img_conv_supported(g):
            tiles = g.B * (g.sH // 8) * (g.sW // 32)
            nwg = min(tiles, IMG_WGS)
            return done(Plan(kernel="img_wgrad_kernel", family="img", tiles=tiles, nwg=nwg, tile_px=256), 9 * 32 * 3, nwg, nwg, 3)
        TW = 32 if g.gC == 32 else 16
        tiles = g.B * (g.Qh // 8) * (g.Qw // TW)
        nwg = min(tiles, THIN_WGS)
        pl = Plan(kernel="thin_tile_kernel<wgrad>", family="thin", tiles=tiles, nwg=nwg, tile_px=8 * TW)
        return done(pl, g.taps_total * g.gC * 3, nwg, nwg * g.ncls, 3)
    N, Mc = g.sC, g.Mc
    rows = g.taps_total * g.gC
    xvec, dvec, narrow = g.gC % 4 == 0, N % 4 == 0, N <= 32
    big = (not has_xf) and xvec and dvec and N % 128 == 0 and Mc >= 8192 and all((n * g.gC) % 128 == 0 for n in g.ntaps)
    if big:
        t128 = sum(n * g.gC // 128 for n in g.ntaps) * (N // 128)
        big = t128 >= 16 and ceil_div(Mc, MC) * t128 >= 8 * 1024
    KT, NT = (128, 128) if big else ((128, 32) if narrow else (64, 64))
    S = choose_splits(g, KT, NT, wsf, 512 if big else 1024)
    if wgrad_ws_floats(g, S) > wsf:
        return Plan(rc=ERR_WORKSPACE)
    if big:
        name, fam = "wgrad_fast_kernel<2,2,2,2>", "fast128"
    elif xvec and dvec and not narrow:
        name, fam = "wgrad_fast_kernel<2,2,1,1>", "fast64"
    else:
        name = "wgrad_kernel<%d,%d,%s,%s>" % (4 if narrow else 2, 1 if narrow else 2, "true" if xvec else "false", "true" if dvec else "false")
        fam = "plain"
    pl = Plan(kernel=name, family=fam, cps=ceil_div(ceil_div(Mc, MC), S))
    return done(pl, rows * N, S, S * g.ncls, N)


def chain_links(c: Case, pl: Plan):
    """Longest chain of float32 additions behind one element of (dW, dbias) (see the module docstring)."""
    if pl.family in ("plain", "fast64", "fast128"):
        inner = pl.cps * MC
    elif pl.family == "wino":
        inner = pl.cps * 8 + 16          # 8 tiles per chunk at each frequency; the three transforms add <= 2 + 2 + 6 links, + spare
    else:
        inner = ceil_div(pl.tiles, pl.nwg) * pl.tile_px
    inner_b = pl.cps * 32 if pl.family == "wino" else inner      # the bias sums pixels, not tiles
    # + slabs, `accumulate`, one spare for the product's own rounding
    return inner + pl.S + 2, inner_b + pl.Sb + 2


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _gen(cid, regime):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(cid + regime)) % (2 ** 31))


def out_hw(c: Case):
    g = c.geom()
    return g.sH, g.sW


def make_inputs(c: Case, regime):
    """float32 tensors: x, dy (g_a with DyXform), xf = (scale, shift, act) or None, dyx = (y, coef[7][Co], act) or None."""
    gen = _gen(c.id, regime)
    Ho, Wo = out_hw(c)
    if regime == "int":
        x = torch.randint(-4, 5, (c.B, c.H, c.W, c.Ci), generator=gen).float()
        dy = torch.randint(-4, 5, (c.B, Ho, Wo, c.Co), generator=gen).float()
    else:
        x = torch.randn(c.B, c.H, c.W, c.Ci, generator=gen)
        dy = torch.randn(c.B, Ho, Wo, c.Co, generator=gen)
    xf = dyx = None
    if c.xf >= 0:
        if regime == "int":
            sc = torch.randint(-2, 3, (c.Ci,), generator=gen).float()
            sh = torch.randint(-3, 4, (c.Ci,), generator=gen).float()
            xf = (sc, sh, ACT_NONE if c.xf == ACT_NONE else ACT_RELU)
        else:
            xf = (0.5 + torch.rand(c.Ci, generator=gen), torch.randn(c.Ci, generator=gen) * 0.5, c.xf)
    if c.dyx >= 0:
        if regime == "int":
            y = torch.randint(-4, 5, (c.B, Ho, Wo, c.Co), generator=gen).float()
            coef = torch.cat([torch.randint(-2, 3, (3, c.Co), generator=gen).float(),      # k1 k2 k3
                              torch.randint(-2, 3, (1, c.Co), generator=gen).float(),      # scale
                              torch.randint(-3, 4, (1, c.Co), generator=gen).float(),      # shift (y*scale + shift == 0 is exact: act' = slope)
                              torch.randint(-9, 10, (2, c.Co), generator=gen).float()])    # d gamma, d beta
            dyx = (y, coef, ACT_NONE if c.dyx == ACT_NONE else ACT_RELU)
        else:
            y = torch.randn(c.B, Ho, Wo, c.Co, generator=gen)
            coef = torch.cat([0.5 + torch.rand(1, c.Co, generator=gen), torch.randn(2, c.Co, generator=gen) * 0.1,
                              0.5 + torch.rand(1, c.Co, generator=gen), torch.randn(3, c.Co, generator=gen) * 0.5])
            dyx = (y, coef, c.dyx)
    return x, dy, xf, dyx


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def act64(t, act):
    return torch.where(t > 0, t, t * slope(act))


def apply_in_xform(x, xf):
    """x' in float64 and the per-element rounding slack of forming it in float32: t = x*sc (+) sh is two roundings (one when
    contracted), the slope product one more."""
    sc, sh, act = xf
    t = x.double() * sc.double() + sh.double()
    slack = U * ((x.double() * sc.double()).abs() + 2 * t.abs()) + U * t.abs()
    return act64(t, act), slack


def apply_dy_xform(ga, dyx):
    """g = k1*g_a*act'(y*scale+shift) + k2*y + k3 in float64 and its float32 slack: three products and two additions, plus --
    where the float32 pre-activation could land on the other side of 0 -- the whole jump of act'."""
    y, coef, act = dyx
    k1, k2, k3, sc, sh = (coef[i].double() for i in range(5))
    y, ga = y.double(), ga.double()
    t = y * sc + sh
    d = torch.where(t > 0, torch.ones_like(t), torch.full_like(t, slope(act)))
    a, b = k1 * ga * d, k2 * y
    g = a + b + k3
    slack = U * (3 * a.abs() + 3 * b.abs() + 2 * k3.abs().expand_as(a) + 2 * g.abs())
    near0 = t.abs() <= 2 * U * ((y * sc).abs() + sh.abs())
    slack = slack + torch.where(near0, (k1 * ga).abs() * (1.0 - slope(act)), torch.zeros_like(a))
    return g, slack


def wgrad_sums(g: Geom, x, d):
    """sum over pixels of x[gpix] (x) d[spix] in float64: rows [tap][gC] x sC (packed order), and the pixel sum of d."""
    B = g.B
    P = 8
    xp = F.pad(x, (0, 0, P, P + g.is_ * g.Qw, P, P + g.is_ * g.Qh))
    dW = torch.zeros(g.k * g.k, g.gC, g.sC, dtype=torch.float64)
    db = torch.zeros(g.sC, dtype=torch.float64)
    for cl in range(g.ncls):
        D = d[:, g.py[cl]::g.os, g.px[cl]::g.os][:, :g.Qh, :g.Qw].reshape(-1, g.sC)
        assert D.shape[0] == g.Mc
        db += D.sum(0)
        for dy_, dx_, wt in g.taps[cl]:
            X = xp[:, P + dy_:P + dy_ + g.is_ * g.Qh:g.is_, P + dx_:P + dx_ + g.is_ * g.Qw:g.is_].reshape(-1, g.gC)
            dW[wt] += X.t() @ D
    return dW, db


def to_layout(g: Geom, dW):
    """[tap][Ci][Co] -> the library's block (CTVAE_W_CI_TAP: [Ci][tap][Co])."""
    return dW.permute(1, 0, 2).contiguous() if g.flat else dW


def reference(c: Case, regime):
    """dict: dw, db (float64, library layout), gy (or None), the absolute sums aw, ab that scale the bounds, and the extra
    slack sw, sb of the transforms' float32 roundings."""
    g = c.geom()
    x, dy, xf, dyx = make_inputs(c, regime)
    x64, d64 = x.double(), dy.double()
    sx = torch.zeros_like(x64)
    sd = torch.zeros_like(d64)
    if xf is not None:
        x64, sx = apply_in_xform(x, xf)
    gy = None
    if dyx is not None:
        d64, sd = apply_dy_xform(dy, dyx)
        gy = d64
    dw, db = wgrad_sums(g, x64, d64)
    aw, ab = wgrad_sums(g, x64.abs(), d64.abs())
    if xf is None and dyx is None:
        sw, sb = torch.zeros_like(dw), torch.zeros_like(db)
    else:
        sw, sb = wgrad_sums(g, sx, d64.abs() + sd)
        sw = sw + wgrad_sums(g, x64.abs(), sd)[0]
        sb = wgrad_sums(g, sx, sd)[1]
    return dict(dw=to_layout(g, dw), db=db, gy=gy, aw=to_layout(g, aw), ab=ab, sw=to_layout(g, sw), sb=sb, gy_slack=sd)


def gamma(L):
    return L * U / (1.0 - L * U)


def bounds(c: Case, pl: Plan, ref):
    """Elementwise bounds of the randn regime for dw and db."""
    L, Lb = chain_links(c, pl)
    aw = ref["aw"]
    if pl.family == "wino":
        x, dy, _, _ = make_inputs(c, "randn")
        aw = wino_sums(c.geom(), x.double(), dy.double(), absolute=True)
    return dict(dw=gamma(L) * aw + ref["sw"] + 1e-300, db=gamma(Lb) * ref["ab"] + ref["sb"] + 1e-300, L=L, Lb=Lb)


# Winograd F(3x3 dW, 2x2 dy) over 4 x 4 input tiles (points 0, 1, -1, inf): per tile  dW = A^T [(B^T x B) . (G d G^T)] A.  The
# products it adds are not those of the direct sum (the cross terms cancel only in exact arithmetic), so in place of
# sum |x||dy| its bound is scaled by the same expression over absolute values, wino_sums(..., absolute=True): what a float32
# evaluation in any order can have rounded.
WINO_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, 1]], dtype=torch.float64)
WINO_G = torch.tensor([[1, 0], [0.5, 0.5], [0.5, -0.5], [0, 1]], dtype=torch.float64)
WINO_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]], dtype=torch.float64)


def wino_sums(g: Geom, x, d, absolute=False):
    """The 3x3 / stride 1 / pad 1 weight gradient [9][Ci][Co] through the Winograd identity in float64; absolute=True: every
    matrix and operand replaced by its absolute value."""
    At, G, Bt = (m.abs() if absolute else m for m in (WINO_AT, WINO_G, WINO_BT))
    if absolute:
        x, d = x.abs(), d.abs()
    xt = F.pad(x, (0, 0, 1, 1, 1, 1)).unfold(1, 4, 2).unfold(2, 4, 2).reshape(-1, g.gC, 4, 4)      # [T, Ci, 4, 4]
    dt = d.unfold(1, 2, 2).unfold(2, 2, 2).reshape(-1, g.sC, 2, 2)                                  # [T, Co, 2, 2]
    V = torch.einsum("ai,tcij,bj->abtc", Bt, xt, Bt)
    Uu = torch.einsum("ai,tnij,bj->abtn", G, dt, G)
    M = torch.einsum("abtc,abtn->abcn", V, Uu)
    return torch.einsum("ka,abcn,lb->klcn", At, M, At).reshape(9, g.gC, g.sC)


def emulate_wino32(c: Case, pl: Plan, regime="randn"):
    """float32 evaluation of the Winograd identity, the tiles cut into pl.S slabs that are added in order."""
    g = c.geom()
    x, dy, _, _ = make_inputs(c, regime)
    At, G, Bt = WINO_AT.float(), WINO_G.float(), WINO_BT.float()
    xt = F.pad(x, (0, 0, 1, 1, 1, 1)).unfold(1, 4, 2).unfold(2, 4, 2).reshape(-1, g.gC, 4, 4)
    dt = dy.unfold(1, 2, 2).unfold(2, 2, 2).reshape(-1, g.sC, 2, 2)
    per = pl.cps * 8
    total = torch.zeros(9, g.gC, g.sC, dtype=torch.float32)
    for t0 in range(0, xt.shape[0], per):
        V = torch.einsum("ai,tcij,bj->abtc", Bt, xt[t0:t0 + per], Bt)
        Uu = torch.einsum("ai,tnij,bj->abtn", G, dt[t0:t0 + per], G)
        M = torch.einsum("abtc,abtn->abcn", V, Uu)
        total = total + torch.einsum("ka,abcn,lb->klcn", At, M, At).reshape(9, g.gC, g.sC)
    return total


def int_exact_margin(c: Case, ref):
    """Largest absolute partial sum any order can meet, over 2^24 (must be < 1).  Winograd's accumulators hold the transforms
    before the halves of G are applied: at most 4 x 4 (B) * 2 x 2 (unscaled G) = 64 times a product, in units of 1."""
    m = max(float(ref["aw"].max()), float(ref["ab"].max()))
    return m * (64.0 if c.wino else 1.0) / 2.0 ** 24


def emulate_chunked(c: Case, pl: Plan, regime="randn", order="naive", unit=MC):
    """float32 emulation of a chunked summation of the same GEMM.  The pixels are cut into max(pl.S, 1) contiguous slices (the
    kernels' slabs); inside a slice units of `unit` pixels (1: every pixel by itself; 32: a chunk, summed by a float32 matmul) are
    added one after the other (`naive`) or as a balanced tree (`pairwise`), then the slices in order.  dW in the library layout."""
    g = c.geom()
    x, dy, xf, dyx = make_inputs(c, regime)
    one = torch.tensor(1.0)
    if xf is not None:
        sc, sh, act = xf
        t = x * sc + sh
        x = torch.maximum(t, t * torch.tensor(slope(act), dtype=torch.float32)) if act != ACT_NONE else t
    if dyx is not None:
        y, coef, act = dyx
        t = y * coef[3] + coef[4]
        dy = coef[0] * dy * torch.where(t > 0, one, torch.tensor(slope(act), dtype=torch.float32)) + coef[1] * y + coef[2]
    P = 8
    xp = F.pad(x, (0, 0, P, P + g.is_ * g.Qw, P, P + g.is_ * g.Qh))
    dW = torch.zeros(g.k * g.k, g.gC, g.sC, dtype=torch.float32)
    nsl = max(pl.S, 1)
    per = ceil_div(ceil_div(g.Mc, nsl), unit) * unit
    for cl in range(g.ncls):
        D = dy[:, g.py[cl]::g.os, g.px[cl]::g.os][:, :g.Qh, :g.Qw].reshape(-1, g.sC)
        for dy_, dx_, wt in g.taps[cl]:
            X = xp[:, P + dy_:P + dy_ + g.is_ * g.Qh:g.is_, P + dx_:P + dx_ + g.is_ * g.Qw:g.is_].reshape(-1, g.gC)
            total = torch.zeros(g.gC, g.sC, dtype=torch.float32)
            for s0 in range(0, g.Mc, per):
                parts = [X[r:min(r + unit, s0 + per)].t() @ D[r:min(r + unit, s0 + per)] for r in range(s0, min(s0 + per, g.Mc), unit)]
                if order == "naive":
                    acc = torch.zeros(g.gC, g.sC, dtype=torch.float32)
                    for q in parts:
                        acc = acc + q
                else:
                    while len(parts) > 1:
                        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
                    acc = parts[0]
                total = total + acc
            dW[wt] += total
    return to_layout(g, dW)


# ---------------------------------------------------------------------------------------------------------------------
# the case lists
# ---------------------------------------------------------------------------------------------------------------------
def _c(id, hits, kind, B, H, W, Ci, Co, k, s, p, op=0, **kw):
    return Case(id, hits, kind, B, H, W, Ci, Co, k, s, p, op, **kw)


P41 = "wgrad_kernel<4,1,%s,%s>"
P22 = "wgrad_kernel<2,2,%s,%s>"
F64 = "wgrad_fast_kernel<2,2,1,1>"
F128 = "wgrad_fast_kernel<2,2,2,2>"

GENERIC_CASES = [
    _c("n-tt-64-32-k3s2", "128x32 plain kernel, vector x and dy", CONV, 2, 16, 16, 64, 32, 3, 2, 1, expect=(P41 % ("true", "true"),)),
    _c("n-tt-xf", "128x32 plain kernel with InXform", CONV, 2, 16, 16, 64, 32, 3, 2, 1, xf=ACT_LRELU, expect=(P41 % ("true", "true"),)),
    _c("n-ft-3-32-w24", "128x32, scalar x (Ci=3), 24-wide output", CONV, 2, 48, 48, 3, 32, 3, 2, 1, expect=(P41 % ("false", "true"),)),
    _c("n-tf-32-3-w24", "128x32, scalar dy (Co=3), W % 32 != 0", CONV, 2, 24, 24, 32, 3, 3, 1, 1, expect=(P41 % ("true", "false"),)),
    _c("n-ff-3-5", "128x32, scalar x and dy; scalar small reduction (n % 4 != 0)", CONV, 2, 9, 11, 3, 5, 3, 1, 1,
       expect=(P41 % ("false", "false"),), red=(1, 0)),
    _c("w-ft-3-64-k4s2", "64x64 plain kernel, scalar x", CONV, 2, 32, 32, 3, 64, 4, 2, 1, expect=(P22 % ("false", "true"),)),
    _c("w-tf-64-66", "64x64 plain kernel, scalar dy, two N tiles", CONV, 2, 8, 8, 64, 66, 3, 1, 1, expect=(P22 % ("true", "false"),)),
    _c("w-ff-6-34", "64x64 plain kernel, scalar x and dy", CONV, 2, 8, 8, 6, 34, 3, 1, 1, expect=(P22 % ("false", "false"),)),
    _c("f-pow2", "lean 64x64, shift decode (Qh, Qw powers of two)", CONV, 2, 16, 16, 64, 64, 3, 1, 1, expect=(F64,)),
    _c("f-pow2-xf", "lean 64x64 with InXform", CONV, 2, 16, 16, 64, 64, 3, 1, 1, xf=ACT_LRELU, expect=(F64,)),
    _c("f-pow2-xf-none", "lean 64x64 with an affine-only InXform (no activation)", CONV, 2, 16, 16, 64, 64, 3, 1, 1, xf=ACT_NONE, expect=(F64,)),
    _c("f-npow2-c48-n68", "lean 64x64: decode_m, gC = 48 (lgC = -1), Ktot % 64 != 0, N = 68, Mc % 32 != 0, short last split",
       CONV, 3, 11, 13, 48, 68, 3, 1, 1, expect=(F64,)),
    _c("f-npow2-xf", "lean 64x64 with InXform on the division decode", CONV, 3, 11, 13, 48, 68, 3, 1, 1, xf=ACT_LRELU, expect=(F64,)),
    _c("f-s12-1x1", "lean 64x64, S = 12: one XCD-reordered group of 8 slices and a plain-order tail of 4; split reduction",
       CONV, 3, 31, 31, 64, 64, 1, 1, 0, expect=(F64,), S=12, red=(0, 1)),
    _c("f-below-big", "just below the 128x128 condition (Mc = 7168 < 8192): 64x64 kernel", CONV, 7, 64, 64, 128, 256, 4, 2, 1,
       expect=(F64,)),
    _c("b-128-256-k4s2", "128x128 lean kernel at its smallest shape: Mc = 8192, 32 tiles", CONV, 8, 64, 64, 128, 256, 4, 2, 1,
       expect=(F128,)),
]

GEOMETRY_CASES = [
    _c("g-k4s1p0", "tap offsets up to +3 (bit-mask encoding)", CONV, 2, 11, 11, 64, 64, 4, 1, 0, expect=(F64,)),
    _c("g-t-k4s1p0", "tap offsets down to -3", CONVT, 2, 8, 8, 64, 64, 4, 1, 0, expect=(F64,)),
    _c("g-k3s2-parity", "stride-2 3x3, parity-grouped tap order", CONV, 2, 17, 17, 64, 64, 3, 2, 1, expect=(F64,)),
    _c("g-t-k4s2", "transposed, four classes of four taps", CONVT, 2, 8, 8, 64, 64, 4, 2, 1, expect=(F64,)),
    _c("g-t-k3s2-512-256", "transposed, classes of 1, 2, 2, 4 taps: unequal Ktot per class", CONVT, 3, 2, 2, 512, 256, 3, 2, 1, 1,
       expect=(F64,)),
    _c("g-flat-narrow", "CTVAE_W_CI_TAP on a narrow layer", CONV | W_CI_TAP, 3, 2, 2, 32, 12, 2, 1, 0, expect=(P41 % ("true", "true"),)),
    _c("g-flat-wide", "CTVAE_W_CI_TAP on a wide layer", CONV | W_CI_TAP, 7, 2, 2, 512, 256, 2, 2, 0, expect=(F64,)),
    _c("g-linear-b7", "Linear, B = 7", CONV, 7, 1, 1, 2048, 256, 1, 1, 0, expect=(F64,)),
    _c("g-linear-b130", "Linear, B = 130: five chunks, the last with two rows", CONV, 130, 1, 1, 128, 2048, 1, 1, 0, expect=(F64,)),
    # the two shapes of the thin-kernel suspicion: the tile kernels must take them
    _c("g-thin-32-3-k3s2", "32->3 k3 s2 at a tile-aligned size: patch 17 x 65 is past the thin kernel's limit", CONV, 2, 16, 64, 32, 3, 3,
       2, 1, expect=(P41 % ("true", "false"),)),
    _c("g-thin-32-3-k4s2", "32->3 k4 s2 at a tile-aligned size", CONV, 2, 16, 64, 32, 3, 4, 2, 1, expect=(P41 % ("true", "false"),)),
    _c("g-thin-64-3-k4s2", "64->3 k4 s2 p1 at a tile-aligned size", CONV, 2, 16, 32, 64, 3, 4, 2, 1, expect=(P41 % ("true", "false"),)),
]

UP = dict(kind=CONVT, Ci=32, Co=32, k=3, s=2, p=1, op=1)
ENC = dict(kind=CONV, Ci=3, Co=32, k=3, s=2, p=1)
IMG = dict(kind=CONV, Ci=32, Co=3, k=3, s=1, p=1)


def _d(id, hits, geo, B, H, W, **kw):
    return Case(id, hits, geo["kind"], B, H, W, geo["Ci"], geo["Co"], geo["k"], geo["s"], geo["p"], geo.get("op", 0), **kw)


DEDICATED_CASES = [
    _d("up-1tile", "upconv kernel, one tile", UP, 1, 8, 32, expect=("up_wgrad_kernel",), S=1),
    _d("up-1tile-xf", "upconv kernel with InXform", UP, 1, 8, 32, xf=ACT_LRELU, expect=("up_wgrad_kernel",), S=1),
    _d("up-dyx", "upconv kernel with DyXform writing gy_out", UP, 2, 8, 32, dyx=ACT_LRELU, dy_out="gy", expect=("up_wgrad_kernel",), S=2),
    _d("up-520", "upconv kernel, 520 tiles on 512 workgroups", UP, 5, 64, 416, expect=("up_wgrad_kernel",), S=512),
    _d("enc-1tile", "encoder kernel, one tile", ENC, 1, 16, 64, expect=("img_enc_wgrad_kernel",), S=1),
    _d("enc-commit", "encoder kernel, DyXform committing dgamma / dbeta", ENC, 2, 16, 64, dyx=ACT_LRELU, dy_out="commit",
       expect=("img_enc_wgrad_kernel",), S=2),
    _d("enc-520", "encoder kernel, 520 tiles on 512 workgroups", ENC, 5, 128, 832, expect=("img_enc_wgrad_kernel",), S=512),
    _d("img-1tile", "image kernel, one tile", IMG, 1, 8, 32, expect=("img_wgrad_kernel",), S=1),
    _d("img-xf", "image kernel with InXform", IMG, 2, 8, 32, xf=ACT_LRELU, expect=("img_wgrad_kernel",), S=2),
    _d("img-520", "image kernel, 520 tiles on 512 workgroups", IMG, 5, 64, 416, expect=("img_wgrad_kernel",), S=512),
    _c("thin-32-k3p0", "thin kernel LP=8, 9 taps", CONV, 1, 10, 34, 32, 3, 3, 1, 0, expect=("thin_tile_kernel<wgrad>",), S=1),
    _c("thin-32-k3p0-xf", "thin kernel with InXform", CONV, 2, 10, 34, 32, 3, 3, 1, 0, xf=ACT_LRELU, expect=("thin_tile_kernel<wgrad>",), S=2),
    _c("thin-t32-k4s2", "thin kernel LP=8, 4 taps per class, four classes", CONVT, 1, 8, 32, 32, 3, 4, 2, 1,
       expect=("thin_tile_kernel<wgrad>",), S=1),
    _c("thin-t64-k4s2", "thin kernel LP=16, 4 taps per class", CONVT, 1, 8, 16, 64, 3, 4, 2, 1, expect=("thin_tile_kernel<wgrad>",), S=1),
    _c("thin-64-k3p1", "thin kernel LP=16, 9 taps", CONV, 1, 8, 16, 64, 3, 3, 1, 1, expect=("thin_tile_kernel<wgrad>",), S=1),
    _c("thin-64-k3s2-lds", "thin kernel with more than 64 KB of dynamic LDS", CONV, 1, 16, 32, 64, 3, 3, 2, 1,
       expect=("thin_tile_kernel<wgrad>",), S=1),
    _c("thin-776", "thin kernel LP=8, 776 tiles on 768 workgroups", CONV, 97, 18, 130, 32, 3, 3, 1, 0,
       expect=("thin_tile_kernel<wgrad>",), S=768),
    _c("thin-t64-776", "thin kernel LP=16 transposed, 776 tiles on 768 workgroups per class", CONVT, 97, 16, 64, 64, 3, 4, 2, 1,
       expect=("thin_tile_kernel<wgrad>",), S=768),
]

WINO_CASES = [
    _c("wino-b8", "Winograd weight gradient at its smallest batch", CONV, 8, 16, 16, 256, 256, 3, 1, 1, wino=True,
       expect=("wino_wgrad_kernel",), S=8),
    _c("wino-b7", "one image less: below Winograd's workgroup floor, the 64x64 kernel", CONV, 7, 16, 16, 256, 256, 3, 1, 1, wino=True,
       expect=(F64,)),
    _c("wino-ws-s3", "a workspace that leaves Winograd three slabs", CONV, 8, 16, 16, 256, 256, 3, 1, 1, wino=True,
       ws_floats=3 * (9 * 256 + 1) * 256 + 5, expect=("wino_wgrad_kernel",), S=3),
]

# dispatch edges: a workspace just below a dedicated kernel's need -> the tile kernels
FALLBACK_CASES = [
    _d("fb-up", "workspace one float below the upconv kernel's need", UP, 1, 8, 32, ws_floats=UP_WS_FLOATS - 1,
       expect=(P41 % ("true", "true"),)),
    _d("fb-enc", "workspace one float below the encoder kernel's need", ENC, 1, 16, 64, ws_floats=ENC_WS_FLOATS - 1,
       expect=(P41 % ("false", "true"),)),
    _c("fb-thin", "workspace one float below the thin kernel's need", CONV, 1, 10, 34, 32, 3, 3, 1, 0,
       ws_floats=THIN_WGS * (9 * 32 * 3 + 3) - 1, expect=(P41 % ("true", "false"),)),
    _c("fb-lower-s", "a workspace that makes choose_splits lower S from 12 to 5", CONV, 3, 31, 31, 64, 64, 1, 1, 0,
       ws_floats=5 * (64 * 64 + 64) + 7, expect=(F64,), S=5, red=(1, 1)),
    _c("fb-ws-s1", "a workspace one float short of S = 1", CONV, 3, 31, 31, 64, 64, 1, 1, 0, ws_floats=64 * 64 + 64 - 1, rc=ERR_WORKSPACE),
    # below Winograd's own S = 1 need the tile kernel's S = 1 need (the same 9*Ci*Co + Co floats) is not met either
    _c("fb-wino-ws", "a workspace one float short of Winograd's single slab: the tile kernel needs as much", CONV, 8, 16, 16, 256, 256, 3,
       1, 1, wino=True, ws_floats=(9 * 256 + 1) * 256 - 1, rc=ERR_WORKSPACE),
]

# reduction shapes: (small | split | wide) x (vector | scalar)
REDUCE_CASES = [
    _c("r-small-vec", "small reduction (S <= 8), float4", CONV, 2, 16, 16, 64, 64, 3, 1, 1, expect=(F64,), red=(1, 1)),
    _c("r-small-scalar", "small reduction, scalar (n % 4 != 0)", CONV, 2, 9, 11, 3, 5, 3, 1, 1, expect=(P41 % ("false", "false"),), red=(1, 0)),
    _c("r-split-vec", "split reduction (S > 8, < 65536 items), float4", CONV, 3, 31, 31, 64, 64, 1, 1, 0, expect=(F64,), S=12, red=(0, 1)),
    _c("r-split-scalar", "split reduction, scalar", CONV, 3, 40, 40, 3, 5, 3, 1, 1, expect=(P41 % ("false", "false"),), red=(0, 0)),
    _c("r-wide-vec", "wide reduction (S > 8, >= 65536 float4 items)", CONV, 9, 32, 32, 256, 128, 3, 2, 1, expect=(F64,), S=9, red=(2, 1)),
    _c("r-wide-scalar", "wide reduction, scalar: 130 x 505 weights", CONV, 3, 27, 27, 130, 505, 1, 1, 0, expect=(P22 % ("false", "false"),),
       red=(2, 0)),
]

RUN_CASES = GENERIC_CASES + GEOMETRY_CASES + DEDICATED_CASES + WINO_CASES + [c for c in FALLBACK_CASES if c.rc == 0]
ALL_CASES = RUN_CASES + [c for c in FALLBACK_CASES if c.rc != 0] + REDUCE_CASES

# (what, case, keyword changes of the call) -> ERR_BAD_ARG with nothing launched and nothing written
ERROR_CASES = [
    _c("e-dyx-generic", "DyXform on a layer that is neither upconv nor encoder", CONV, 2, 16, 16, 64, 64, 3, 1, 1, dyx=ACT_LRELU,
       dy_out="gy", rc=ERR_BAD_ARG),
    _d("e-up-no-gy", "DyXform on upconv without gy_out", UP, 1, 8, 32, dyx=ACT_LRELU, dy_out="none", rc=ERR_BAD_ARG),
    _d("e-enc-gy", "DyXform with gy_out on the encoder layer", ENC, 1, 16, 64, dyx=ACT_LRELU, dy_out="gy", rc=ERR_BAD_ARG),
    _c("e-xf-scalar", "InXform on a non-vector layer (Ci = 6)", CONV, 2, 8, 8, 6, 34, 3, 1, 1, xf=ACT_LRELU, rc=ERR_BAD_ARG),
]

# the 13 layers of the deferred-reduction test (with bias 26 jobs: two reduce_multi_kernel launches), then DEFER_TWICE once more
DEFER_IDS = ["n-tt-64-32-k3s2", "n-ft-3-32-w24", "n-tf-32-3-w24", "n-ff-3-5", "w-tf-64-66", "w-ff-6-34", "f-pow2", "f-npow2-c48-n68",
             "f-s12-1x1", "g-k4s1p0", "g-t-k4s2", "g-flat-narrow", "g-t-k4s1p0"]
DEFER_TWICE = "f-pow2"
DEFER_WS_FLOATS = 1 << 20      # workspace of each call: what a call takes from the arena


def case_by_id(cid):
    return next(c for c in ALL_CASES + ERROR_CASES if c.id == cid)
