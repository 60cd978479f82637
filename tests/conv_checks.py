"""Shared by tests/test_conv_reference_host.py (CPU) and tests/test_conv_ops_gpu.py (GPU): float64 references of
ctvae_conv_forward / ctvae_conv_dgrad / ctvae_linear_pixmajor_forward / ctvae_conv_forward_lazy in the library's own layouts, the
two input regimes with their bounds, a Python mirror of launch_tapgemm's kernel selection (csrc/tapgemm.hip, thin.hip, image.hip,
upconv.hip, upimg.hip, wino.hip, api.hip) and the case lists.  Pure torch: importable without a GPU and without the library.

Layouts: every activation tensor is NHWC; the weights are the packed block [tap][Ci][Co] (tap = ky*k + kx), with CTVAE_W_CI_TAP
the Linear block [Ci][tap][Co].  A case describes the LAYER (input [B,H,W,Ci], Co, k, s, p, op); `op` says which of its two
gather-GEMMs runs: "fwd" gathers x and scatters y, "dgrad" gathers dy and scatters dx with the weights transposed per tap.

Reference (csrc/geom.hpp build_geom kinds 0..3, ported in build_geom() below and pinned to torch's float64 conv ops, to torch's
float64 autograd and to tests/host_emul/geom_emul.cpp in the host test):

    pre[spix(m)][n] = sum_t sum_c G'[gpix(m,t)][c] * Wmat[t][c][n] + bias[n] + add[spix(m)][n]
    out             = act(pre) * act'(mask)

G' = act_in(G*scale[c] + shift[c]) inside the image, 0 in the padding (InXform); act'(mask) = mask > 0 ? 1 : slope for LeakyReLU /
ReLU and 1 - mask^2 for tanh, applied after the activation (splitk_finish_body in csrc/finish.hpp, the tile epilogues).

Regimes.  `int`: data, weights, bias, add and the InXform coefficients are small integers, activations are NONE / ReLU, masks are
integers (exact signs); every partial sum of every order stays below 2^24 (int_exact_margin(), asserted per case on the host), so
float32 arithmetic is exact in any order and the GPU result must equal the reference bit for bit.  Winograd's transforms only
halve and quarter: all its intermediates are multiples of 1/4 bounded by the same pipeline over absolute values, so 4 * that
bound < 2^24 keeps them exact as well.  `randn`: O(1) data; a sum of terms t_i evaluated in float32 in ANY order whose longest
chain of additions has L links satisfies |err| <= gamma_L * sum |t_i|, gamma_L = L u / (1 - L u), u = 2^-24 (Higham, Accuracy and
Stability of Numerical Algorithms, 4.2).  L = (terms of the longest reduction: max over classes of ntaps * gC) + (K slices) + 3
(bias, add, one spare for the product's own rounding): valid for any order, which is what MFMA accumulation needs.  LeakyReLU /
ReLU are 1-Lipschitz, so the bound on `pre` carries over; each further epilogue product adds one rounding u |out|; the tanh
kernel adds TANH_ABS (tests/loss_checks.py).  Winograd adds other products than the direct sum (the cross terms cancel only in
exact arithmetic): its bound is the same transform pipeline over absolute values (wino_forward(..., absolute=True)) with the
chain length of that pipeline.  Nothing here was tuned on a kernel."""
import time
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn.functional as F

from tests import wgrad_checks as V
from tests.loss_checks import TANH_ABS
from tests.wgrad_checks import U, ceil_div

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3
CONV, CONVT, W_CI_TAP = V.CONV, V.CONVT, V.W_CI_TAP
ERR_BAD_ARG = V.ERR_BAD_ARG
WS_BYTES = V.WS_BYTES
KC = 32
LEAKY = float(torch.tensor(0.01, dtype=torch.float32))        # common.hpp kLeaky as the float32 it is
MAX_TENSOR_BYTES = 128 << 20
FIN = "splitk_finish_kernel"


def slope(act):
    return {ACT_NONE: 1.0, ACT_LRELU: LEAKY, ACT_RELU: 0.0}[act]


# ---------------------------------------------------------------------------------------------------------------------
# geometry (csrc/geom.hpp build_geom, kinds 0..3)
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Geom(V.Geom):
    wT: int = 0
    wCi: int = 0
    wCo: int = 0

    @property
    def packed(self):                      # packed_weights(): wrs == wCo and wts == wCi*wCo
        return (not self.flat) or (self.k == 1 and self.wCi == 1)

    @property
    def Kmax(self):
        return max(self.ntaps) * self.gC


def _convlike_taps(k, s, p):
    """scattered index q; gathered = q*s + (ky - p).  Stride 2: grouped by the parity of the offsets."""
    if s == 2:
        return [(ky - p, kx - p, ky * k + kx) for qy in range(2) for qx in range(2) for ky in range(k) for kx in range(k)
                if ((ky - p) & 1) == (qy ^ 1) and ((kx - p) & 1) == (qx ^ 1)]
    return [(ky - p, kx - p, ky * k + kx) for ky in range(k) for kx in range(k)]


def _trunc_div(a, b):
    return int(a / b)                      # C++ division truncates toward zero ((par+p-ky) is an exact multiple of s here)


def build_geom(gkind, B, H, W, Ci, Co, k, s, p, op, flat=False):
    """gkind 0 conv fwd, 1 convT fwd, 2 conv dgrad, 3 convT dgrad; (B,H,W,Ci) the LAYER's input.  None where build_geom refuses."""
    tr = gkind in (1, 3)
    if tr:
        Ho, Wo = (H - 1) * s - 2 * p + k + op, (W - 1) * s - 2 * p + k + op
    else:
        Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    if Ho <= 0 or Wo <= 0 or k * k > 64 or s < 1 or s > 2:
        return None
    fwd = gkind in (0, 1)
    if fwd:
        gH, gW, gC, sH, sW, sC = H, W, Ci, Ho, Wo, Co
    else:
        gH, gW, gC, sH, sW, sC = Ho, Wo, Co, H, W, Ci
    if gkind in (0, 3):
        if k * k > 16:
            return None
        return Geom(B, gH, gW, gC, sH, sW, sC, sH, sW, s, 1, k, flat, [0], [0], [_convlike_taps(k, s, p)], 0 if fwd else 1, Ci, Co)
    if sH % s or sW % s:
        return None
    g = Geom(B, gH, gW, gC, sH, sW, sC, sH // s, sW // s, 1, s, k, flat, wT=0 if fwd else 1, wCi=Ci, wCo=Co)
    for c in range(s * s):
        py, px = c // s, c % s
        taps = [(_trunc_div(py + p - ky, s), _trunc_div(px + p - kx, s), ky * k + kx)
                for ky in range(k) if (py + p - ky) % s == 0 for kx in range(k) if (px + p - kx) % s == 0]
        if len(taps) > 16:
            return None
        g.py.append(py); g.px.append(px); g.taps.append(taps)
    return g


def conv_kind_ok(kind):
    base = kind & ~W_CI_TAP
    return base == CONV or (base == CONVT and not (kind & W_CI_TAP))


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    hits: str                    # what the case is there to hit
    op: str                      # "fwd" | "dgrad"
    kind: int
    B: int
    H: int
    W: int
    Ci: int
    Co: int
    k: int
    s: int
    p: int
    opad: int = 0
    act: int = ACT_NONE          # forward activation (randn regime: this one; int regime: ReLU unless NONE)
    xf: int = -1                 # InXform activation, -1: none
    add: bool = False
    mask: int = -1               # mask_act of the data gradient, -1: no mask
    bias: bool = True            # forward only (the data gradient has none)
    wino: bool = False
    ws_floats: Optional[int] = None     # workspace handed to the call (None: all of it, -1: a NULL workspace)
    expect: tuple = ()           # kernel labels the case must log
    sk: Optional[int] = None     # split count it must log (tile kernels)
    rc: int = 0
    regimes: tuple = ("int", "randn")

    def args(self):
        return (self.kind, self.B, self.H, self.W, self.Ci, self.Co, self.k, self.s, self.p, self.opad)

    def geom(self):
        base = self.kind & ~W_CI_TAP
        return build_geom((0 if self.op == "fwd" else 2) + (0 if base == CONV else 1), *self.args()[1:], flat=bool(self.kind & W_CI_TAP))

    def ws(self):
        return WS_BYTES // 4 if self.ws_floats is None else max(self.ws_floats, 0)

    def acts(self, regime):
        """(act, xf act, mask act) of a regime: the int regime has no LeakyReLU (0.01 is no float32 integer multiple)."""
        f = (lambda a: a if a in (-1, ACT_NONE) else ACT_RELU) if regime == "int" else (lambda a: a)
        return f(self.act), f(self.xf), f(self.mask)


# ---------------------------------------------------------------------------------------------------------------------
# mirror of launch_tapgemm's selection
# ---------------------------------------------------------------------------------------------------------------------
def _within(g, lo, hi):
    return all(lo <= dy <= hi and lo <= dx <= hi for cl in g.taps for dy, dx, _ in cl)


def _img_taps_ok(g):
    return (g.ncls == 1 and g.is_ == 1 and g.os == 1 and g.ntaps[0] == 9 and g.gH == g.sH and g.gW == g.sW and g.sH % 8 == 0 and
            g.sW % 32 == 0 and _within(g, -1, 1))


def img_conv_supported(g):
    return g.packed and g.wT == 0 and g.gC == 32 and g.sC == 3 and g.wCi == 32 and g.wCo == 3 and _img_taps_ok(g)


def img_dgrad_supported(g):
    return g.packed and g.wT == 1 and g.gC == 3 and g.sC == 32 and g.wCi == 32 and g.wCo == 3 and _img_taps_ok(g)


def img_enc_supported(g):
    return g.wT == 0 and g.wCi == 3 and g.wCo == 32 and V.img_enc_supported(g)


def upconv_supported(g):
    return g.wT == 0 and g.wCi == 32 and g.wCo == 32 and V.upconv_supported(g)


def upimg_supported(g):
    return (g.packed and g.wT == 0 and g.is_ == 1 and g.os == 2 and g.ncls == 4 and g.gC == 64 and g.sC == 3 and g.gH % 8 == 0 and
            g.gW % 32 == 0 and g.sH == 2 * g.gH and g.sW == 2 * g.gW and g.ntaps == [4, 4, 4, 4] and
            all(g.py[c] == c // 2 and g.px[c] == c % 2 for c in range(4)) and _within(g, -1, 1))


def thin_forward_supported(g):
    return g.wT == 0 and V.thin_shape_ok(g, wgrad=False)


def thin_wgrad_supported(g):
    return g.wT == 0 and V.thin_shape_ok(g, wgrad=True)


def wino_block(g):
    """(bh, bw, nb) of wino_block(), or None."""
    H, W = g.gH, g.gW
    if H % 2 or W % 2:
        return None
    TH, TW = H // 2, W // 2
    if TH * TW <= 64:
        if 64 % (TH * TW):
            return None
        bh, bw, nb = TH, TW, 64 // (TH * TW)
    else:
        if TH % 8 or TW % 8:
            return None
        bh, bw, nb = 8, 8, 1
    return (bh, bw, nb) if nb * (2 * bh + 2) * (2 * bw + 2) <= 640 else None


def wino_taps_ok(g):
    if not (g.packed and g.is_ == 1 and g.os == 1 and g.ncls == 1 and g.ntaps[0] == 9 and g.gH == g.sH and g.gW == g.sW):
        return False
    return _within(g, -1, 1) and len({(dy, dx) for dy, dx, _ in g.taps[0]}) == 9


def wino_supported(g, ws_floats):
    if not wino_taps_ok(g) or wino_block(g) is None:
        return False
    if g.gC % 8 or g.gC < 64 or g.sC % 64:
        return False
    tiles = g.B * (g.gH // 2) * (g.gW // 2)
    if ceil_div(tiles, 64) * (g.sC // 64) < 64:
        return False
    return 16 * g.gC * g.sC <= ws_floats


def wino_filter_floats(c, wino_on):
    """ctvae_conv_wino_filter_floats() of the case's layer."""
    if c.kind != CONV or not wino_on:
        return 0
    gf, gb = build_geom(0, *c.args()[1:]), build_geom(2, *c.args()[1:])
    if gf is None or gb is None:
        return 0
    return 16 * c.Ci * c.Co if wino_supported(gf, c.ws()) and wino_supported(gb, c.ws()) else 0


@dataclass
class TilePlan:
    thin: bool = False
    BM: int = 0
    BN: int = 0
    mtiles: int = 0
    ntiles: int = 0
    splitk: int = 1


def tapgemm_plan(g, ws_floats):
    """tapgemm_plan() outside ctvae_conv_backward (no pair context)."""
    Mc, N = g.Mc, g.sC
    if img_enc_supported(g) or upconv_supported(g):
        return TilePlan()
    if thin_forward_supported(g):
        return TilePlan(thin=True)
    avec = g.gC % KC == 0
    bvec = avec if g.wT else N % 4 == 0
    pl = TilePlan(BM=128, BN=32)
    if not (N <= 32 or not avec or not bvec):
        tiles128 = ceil_div(Mc, 128) * ceil_div(N, 64) * g.ncls
        kch = min(n * g.gC // KC for n in g.ntaps)
        pl.BM = 128 if (tiles128 >= 512 and kch > 72) else 64
        pl.BN = 64
    pl.mtiles, pl.ntiles = ceil_div(Mc, pl.BM), ceil_div(N, pl.BN)
    wgs = pl.mtiles * pl.ntiles * g.ncls
    nch_min = min((n * g.gC // KC) if avec else ceil_div(n * g.gC, KC) for n in g.ntaps)
    if avec and bvec and N % 4 == 0 and wgs < 256 and nch_min >= 8:
        sk = min(ceil_div(768, wgs), nch_min // 4, 16)
        per = g.B * g.sH * g.sW * N
        while sk > 1 and per * sk > ws_floats:          # the workspace clamp
            sk -= 1
        if sk > 1:
            pl.splitk = sk
    return pl


def input_transform_supported(c, wino_on):
    """ctvae_conv_input_transform_supported() of the case's layer (forward geometry)."""
    if not conv_kind_ok(c.kind):
        return False
    base = c.kind & ~W_CI_TAP
    g = build_geom(0 if base == CONV else 1, *c.args()[1:], flat=bool(c.kind & W_CI_TAP))
    if g is None:
        return False
    if thin_forward_supported(g) and thin_wgrad_supported(g):
        return True
    if upconv_supported(g):
        return True
    if img_enc_supported(g) or img_conv_supported(g):
        return False
    if wino_on and wino_supported(g, 1 << 26):
        return False
    pl = tapgemm_plan(g, 1 << 26)
    if pl.thin or pl.BM == 0:
        return False
    return g.gC % KC == 0 and g.sC % 4 == 0 and g.wT == 0


def out_pix_supported(g, ws_floats, P):
    if P <= 1 or g.os != 1 or g.ncls != 1 or g.ntaps[0] != 1 or g.sH * g.sW != 1 or g.sC % P or g.wT:
        return False
    if g.gC % KC or g.sC % 4:
        return False
    pl = tapgemm_plan(g, ws_floats)
    return (not pl.thin) and pl.BM != 0 and pl.splitk <= 1


def linear_pixmajor_supported(B, Ci, C, P, ws_floats):
    if B <= 0 or Ci <= 0 or C <= 0 or P <= 1:
        return False
    return out_pix_supported(build_geom(0, B, 1, 1, Ci, C * P, 1, 1, 0, 0), ws_floats, P)


def lazy_slices(c, wino_on=False):
    """ctvae_conv_forward_lazy_slices() of the case's layer."""
    g = c.geom()
    if not conv_kind_ok(c.kind) or g is None or c.op != "fwd":
        return 0
    if img_enc_supported(g) or img_conv_supported(g) or upconv_supported(g) or (wino_on and wino_supported(g, c.ws())):
        return 0
    pl = tapgemm_plan(g, c.ws())
    return 0 if (pl.thin or pl.splitk <= 1) else pl.splitk


def fast_label(pl, wt, pf, xf):
    wm, wn, tm = (4, 1, 1) if pl.BN == 32 else ((2, 2, 2) if pl.BM == 128 else (2, 2, 1))
    return "tapgemm_fast_kernel<%d,%d,%d,1,%s,%d%s>" % (wm, wn, tm, "true" if wt else "false", pf, ",true" if (xf and not wt) else "")


def masked_label(wt, avec, bvec):
    b = lambda v: "true" if v else "false"
    return "tapgemm_masked_kernel<%s,%s,%s>" % (b(wt), b(avec), b(bvec))


@dataclass
class Sel:
    rc: int = 0
    labels: list = field(default_factory=list)     # [] for a refusal: nothing is launched
    sk: int = 0                                    # slices the tile kernel writes (0: not a tile kernel)
    family: str = ""
    cls_rot: int = 0
    L: int = 0                                     # links of the longest addition chain behind one output element


def select(c: Case, filters_out=False, filters_ready=False, out_pix=0) -> Sel:
    """What a ctvae_conv_forward / ctvae_conv_dgrad call of the case launches: api.hip's own checks, then launch_tapgemm's order.
    filters_out / filters_ready: wino_dgrad_filters_out, or wino_fwd_filters / wino_filters, is given."""
    refuse = Sel(rc=ERR_BAD_ARG)
    if not conv_kind_ok(c.kind):
        return refuse
    g = c.geom()
    if g is None:
        return refuse
    has_xf, has_add, has_mask = c.xf >= 0, c.add, c.mask >= 0
    has_bias = c.bias and c.op == "fwd"
    has_ws = c.ws_floats != -1
    wsf = c.ws() if has_ws else 0
    if (filters_out or filters_ready) and not wino_filter_floats(c, c.wino):
        return refuse
    if c.op == "fwd" and has_xf and not input_transform_supported(c, c.wino):      # the guard of ctvae_conv_forward
        return refuse
    if out_pix > 1 and (not out_pix_supported(g, wsf, out_pix) or has_add or has_mask):
        return refuse
    Kmax = g.Kmax

    def done(family, labels, sk=0, cls_rot=0, L=None):
        return Sel(0, sorted(labels), sk, family, cls_rot, (Kmax + max(sk, 1) + 3) if L is None else L)

    if not has_mask and not has_xf and has_ws and c.wino and wino_supported(g, wsf):
        bh, bw, nb = wino_block(g)
        mtiles = ceil_div(g.B, nb) if nb > 1 else g.B * ((g.gH // 2) // bh) * ((g.gW // 2) // bw)
        fsplit = mtiles * (g.sC // 64) < 200
        plain_fwd = g.wT == 0 and all(wt == (dy + 1) * 3 + dx + 1 for dy, dx, wt in g.taps[0])
        if filters_ready:
            labels = []
        elif filters_out and plain_fwd and g.gC % 32 == 0 and g.sC % 32 == 0:
            labels = ["wino_weight2_kernel"]
        else:
            labels = ["wino_weight_kernel"]
        # chain: the channel sum (gC products per frequency), B^T d B two links, G g G^T six, A^T M A four, bias, add, spare
        return done("wino", labels + ["wino_conv_fs_kernel" if fsplit else "wino_conv_kernel"], L=g.gC + 2 + 6 + 4 + 3)
    if img_dgrad_supported(g) and not has_bias and not has_add and not has_mask and c.act == ACT_NONE and not has_xf:
        return done("img_dgrad", ["img_dgrad_kernel"])
    if img_enc_supported(g) and c.act != ACT_TANH and not has_add and not has_mask and not has_xf:
        return done("img_enc", ["img_enc_fwd_kernel"])
    if upconv_supported(g) and not has_add and not has_mask:
        return done("up", ["up_fwd_kernel"])
    if g.Mc <= 0 or g.sC <= 0 or not _within(g, -3, 4):
        return refuse
    wt = g.wT != 0
    avec = g.gC % KC == 0
    bvec = avec if wt else g.sC % 4 == 0
    if not avec and not thin_forward_supported(g) and any(n * g.gC > 64 for n in g.ntaps):
        return refuse                                   # the scalar path keeps its k-table in LDS
    pl = tapgemm_plan(g, wsf)
    if has_xf and not pl.thin and not (avec and bvec and not wt):
        return refuse
    if pl.thin:
        if has_add or has_mask:
            return refuse                               # launch_thin_forward: no residual operand, no mask
        if img_conv_supported(g):
            return done("img", ["img_fwd_kernel"])
        if upimg_supported(g) and not has_xf:
            return done("upimg", ["upimg_fwd_kernel"])
        return done("thin", ["thin_tile_kernel<fwd>"])
    if not avec or not bvec:
        return done("masked", [masked_label(wt, avec, bvec)], sk=0)
    # launch_fast_cfg computes its own tiles (the plan of a dedicated shape that fell through has BM = BN = 0: the 64 x 64 tile)
    BM, BN = (128, 32) if pl.BN == 32 else ((128, 64) if pl.BM == 128 else (64, 64))
    pf = 3 if pl.mtiles * pl.ntiles * g.ncls * pl.splitk <= 1024 else 0
    total = ceil_div(g.Mc, BM) * ceil_div(g.sC, BN) * g.ncls * pl.splitk
    cls_rot = 1 if (g.ncls == 4 and total <= 1024 and pl.splitk > 1) else 0
    labels = [fast_label(pl, wt, pf, has_xf)] + ([FIN] if pl.splitk > 1 else [])
    return done("fast%dx%d" % (BM, BN), labels, sk=pl.splitk, cls_rot=cls_rot)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _gen(cid, regime):
    return torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate("conv" + cid + regime)) % (2 ** 31))


def w_shape(c: Case):
    kk = c.k * c.k
    return (c.Ci, kk, c.Co) if c.kind & W_CI_TAP else (kk, c.Ci, c.Co)


def make_inputs(c: Case, regime):
    """float32 tensors in the library's layouts: dict(G gathered operand, W, bias, add, mask, xf = (scale, shift, act) or None)."""
    gen = _gen(c.id, regime)
    g = c.geom()
    act, xfa, maska = c.acts(regime)
    gs, ss = (g.B, g.gH, g.gW, g.gC), (g.B, g.sH, g.sW, g.sC)
    if regime == "int":
        rnd = lambda shape, lo=-4, hi=4: torch.randint(lo, hi + 1, shape, generator=gen).float()
        G, W = rnd(gs), rnd(w_shape(c))
        bias = rnd((g.sC,), -9, 9) if (c.bias and c.op == "fwd") else None
        add = rnd(ss, -9, 9) if c.add else None
        mask = rnd(ss, -2, 2) if c.mask >= 0 else None
        xf = (rnd((g.gC,), -2, 2), rnd((g.gC,), -3, 3), xfa) if c.xf >= 0 else None
    else:
        rn = lambda shape: torch.randn(shape, generator=gen)
        G, W = rn(gs), rn(w_shape(c))
        bias = rn((g.sC,)) if (c.bias and c.op == "fwd") else None
        add = rn(ss) if c.add else None
        mask = rn(ss) * (0.5 if maska == ACT_TANH else 1.0) if c.mask >= 0 else None
        xf = (0.5 + torch.rand(g.gC, generator=gen), rn((g.gC,)) * 0.5, xfa) if c.xf >= 0 else None
    return dict(G=G, W=W, bias=bias, add=add, mask=mask, xf=xf)


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def wmat(g: Geom, W):
    """The library's weight block -> Wmat[tap][c][n] (c gathered, n scattered channel), float64."""
    W = W.double()
    if g.flat:
        W = W.permute(1, 0, 2)                          # [Ci][tap][Co] -> [tap][Ci][Co]
    return W.transpose(1, 2) if g.wT else W


def gather_gemm(g: Geom, G, Wm):
    """S[spix(m)][n] = sum_t sum_c G[gpix(m,t)][c] * Wm[wtap(t)][c][n] in the dtype of the operands; NHWC [B,sH,sW,sC]."""
    P = 8
    Gp = F.pad(G, (0, 0, P, P + g.is_ * g.Qw, P, P + g.is_ * g.Qh))
    out = torch.zeros(g.B, g.sH, g.sW, g.sC, dtype=G.dtype)
    for cl in range(g.ncls):
        acc = torch.zeros(g.Mc, g.sC, dtype=G.dtype)
        for dy, dx, wt in g.taps[cl]:
            X = Gp[:, P + dy:P + dy + g.is_ * g.Qh:g.is_, P + dx:P + dx + g.is_ * g.Qw:g.is_].reshape(-1, g.gC)
            acc += X @ Wm[wt]
        out[:, g.py[cl]::g.os, g.px[cl]::g.os][:, :g.Qh, :g.Qw] = acc.view(g.B, g.Qh, g.Qw, g.sC)
    return out


def act64(t, act):
    return torch.tanh(t) if act == ACT_TANH else torch.where(t > 0, t, t * slope(act))


def mask_factor(mask, mask_act):
    m = mask.double()
    if mask_act == ACT_TANH:
        return 1.0 - m * m
    return torch.where(m > 0, torch.ones_like(m), torch.full_like(m, slope(mask_act)))


# Winograd F(2x2, 3x3): Y = A^T [(G g G^T) . (B^T d B)] A per 2 x 2 output tile (csrc/wino.hip)
WINO_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
WINO_G = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=torch.float64)
WINO_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def wino_forward(g: Geom, G, Wm, absolute=False):
    """The 3x3 / stride 1 / pad 1 gather-GEMM through the Winograd identity in float64; absolute=True: every matrix and operand
    replaced by its absolute value (what a float32 evaluation of the pipeline in any order can have rounded)."""
    Bt, Gm, At = (m.abs() if absolute else m for m in (WINO_BT, WINO_G, WINO_AT))
    if absolute:
        G, Wm = G.abs(), Wm.abs()
    geff = torch.zeros(3, 3, g.gC, g.sC, dtype=torch.float64)
    for dy, dx, wt in g.taps[0]:
        geff[dy + 1, dx + 1] = Wm[wt]
    d = F.pad(G, (0, 0, 1, 1, 1, 1)).unfold(1, 4, 2).unfold(2, 4, 2)                # [B, TH, TW, C, 4, 4]
    Bn, TH, TW = d.shape[:3]
    Vv = torch.einsum("ai,btucij,ej->aebtuc", Bt, d, Bt).reshape(4, 4, -1, g.gC)
    Uu = torch.einsum("ai,ijcn,ej->aecn", Gm, geff, Gm)
    M = torch.einsum("aetc,aecn->aetn", Vv, Uu)
    Y = torch.einsum("ya,aetn,xe->tyxn", At, M, At).reshape(Bn, TH, TW, 2, 2, g.sC)
    return Y.permute(0, 1, 3, 2, 4, 5).reshape(Bn, 2 * TH, 2 * TW, g.sC)


def reference(c: Case, regime, inputs=None):
    """dict: sum (pre-bias gather-GEMM), pre, out (float64, NHWC), asum = sum |terms| + |bias| + |add| (scales the bound), xs = the
    extra slack of the InXform's float32 roundings carried through the GEMM, factor = act'(mask) or None, seconds."""
    t0 = time.perf_counter()
    g = c.geom()
    inp = make_inputs(c, regime) if inputs is None else inputs
    act, _, maska = c.acts(regime)
    G64 = inp["G"].double()
    sG = None
    if inp["xf"] is not None:
        G64, sG = V.apply_in_xform(inp["G"], (inp["xf"][0], inp["xf"][1], inp["xf"][2]))
        if inp["xf"][2] == ACT_LRELU:                   # V's act64 uses 0.01; the kernels' slope is float32(0.01)
            t = inp["G"].double() * inp["xf"][0].double() + inp["xf"][1].double()
            G64 = torch.where(t > 0, t, t * LEAKY)
    Wm = wmat(g, inp["W"])
    s = gather_gemm(g, G64, Wm)
    asum = gather_gemm(g, G64.abs(), Wm.abs())
    xs = gather_gemm(g, sG, Wm.abs()) if sG is not None else torch.zeros_like(s)
    pre = s.clone()
    if inp["bias"] is not None:
        pre += inp["bias"].double()
        asum = asum + inp["bias"].double().abs()
    if inp["add"] is not None:
        pre += inp["add"].double()
        asum = asum + inp["add"].double().abs()
    out = act64(pre, act)
    factor = None
    if inp["mask"] is not None:
        factor = mask_factor(inp["mask"], maska)
        out = out * factor
    return dict(sum=s, pre=pre, out=out, asum=asum, xs=xs, factor=factor, seconds=time.perf_counter() - t0)


def pixmajor_ref(x, w, bias, C, P):
    """ctvae_linear_pixmajor_forward before the activation: column c*P + p of the Linear goes to pixel p, channel c.  [B, P, C]."""
    pre = x.double() @ w.double()
    if bias is not None:
        pre = pre + bias.double()
    return pre.view(x.shape[0], C, P).permute(0, 2, 1).contiguous()


def gamma(L):
    return L * U / (1.0 - L * U)


def bounds(c: Case, sel: Sel, ref, inputs=None):
    """Elementwise bound of the randn regime on `out` (and `pre_bound` on the pre-activation sum)."""
    g = c.geom()
    act, _, maska = c.acts("randn")
    asum = ref["asum"]
    if sel.family == "wino":
        inp = make_inputs(c, "randn") if inputs is None else inputs
        asum = wino_forward(g, inp["G"].double(), wmat(g, inp["W"]), absolute=True)
        if inp["bias"] is not None:
            asum = asum + inp["bias"].double().abs()
        if inp["add"] is not None:
            asum = asum + inp["add"].double().abs()
    pre_b = gamma(sel.L) * asum + ref["xs"]
    a = act64(ref["pre"], act).abs()
    b = pre_b.clone()                                   # LeakyReLU / ReLU / tanh are 1-Lipschitz
    if act == ACT_TANH:
        b = b + TANH_ABS
    elif act == ACT_LRELU:
        b = b + U * a                                   # the slope product
    if ref["factor"] is not None:
        f = ref["factor"].abs()
        # tanh mask: m*m and 1 - m*m are one rounding each; then the product with the factor, one more
        ferr = U * (inputs_mask_sq(c, inputs) + f) if maska == ACT_TANH else 0.0
        b = b * f + a * ferr + U * ref["out"].abs()
    return dict(out=b + 1e-300, pre=pre_b + 1e-300, L=sel.L)


def inputs_mask_sq(c, inputs):
    inp = make_inputs(c, "randn") if inputs is None else inputs
    return inp["mask"].double() ** 2


def int_exact_margin(c: Case, sel: Sel, ref, inputs=None):
    """Largest absolute partial sum any order can meet, over 2^24 (must be < 1).  Winograd: its intermediates are multiples of
    1/4 bounded by the absolute pipeline, so four times that bound counts."""
    m = float(ref["asum"].max())
    if sel.family == "wino":
        inp = make_inputs(c, "int") if inputs is None else inputs
        g = c.geom()
        m = 4.0 * float(wino_forward(g, inp["G"].double(), wmat(g, inp["W"]), absolute=True).max()) + 18.0
    return m / 2.0 ** 24


def emulate32(c: Case, sel: Sel, order, inputs=None):
    """float32 evaluation of the same sums up to `pre`: `taps` adds one float32 matmul per tap in the geometry's order, `reversed`
    in the opposite order, `slices` cuts the gathered channels into max(sk, 2) slices that are summed at the end."""
    g = c.geom()
    inp = make_inputs(c, "randn") if inputs is None else inputs
    G = inp["G"]
    if inp["xf"] is not None:
        sc, sh, a = inp["xf"]
        t = G * sc + sh
        G = torch.maximum(t, t * torch.tensor(slope(a), dtype=torch.float32)) if a != ACT_NONE else t
    Wm = wmat(g, inp["W"]).float()
    if order == "slices":
        n = max(sel.sk, 2)
        step = ceil_div(g.gC, n)
        s = torch.zeros(g.B, g.sH, g.sW, g.sC)
        for c0 in range(0, g.gC, step):
            part = Geom(**{**g.__dict__, "gC": min(step, g.gC - c0)})
            s = s + gather_gemm(part, G[..., c0:c0 + step].contiguous(), Wm[:, c0:c0 + step].contiguous())
    else:
        gg = g
        if order == "reversed":
            gg = Geom(**{**g.__dict__, "taps": [list(reversed(t)) for t in g.taps]})
        s = gather_gemm(gg, G, Wm)
    if inp["bias"] is not None:
        s = s + inp["bias"]
    if inp["add"] is not None:
        s = s + inp["add"]
    return s


def max_tensor_bytes(c: Case):
    g = c.geom()
    return 4 * max(g.B * g.gH * g.gW * g.gC, g.B * g.sH * g.sW * g.sC, c.k * c.k * c.Ci * c.Co)


# ---------------------------------------------------------------------------------------------------------------------
# the case lists
# ---------------------------------------------------------------------------------------------------------------------
def _f(id, hits, kind, B, H, W, Ci, Co, k, s, p, opad=0, **kw):
    return Case(id, hits, "fwd", kind, B, H, W, Ci, Co, k, s, p, opad, **kw)


def _g(id, hits, kind, B, H, W, Ci, Co, k, s, p, opad=0, **kw):
    return Case(id, hits, "dgrad", kind, B, H, W, Ci, Co, k, s, p, opad, bias=False, **kw)


def FK(wm, wn, tm, wt, pf, xf=False):
    return "tapgemm_fast_kernel<%d,%d,%d,1,%s,%d%s>" % (wm, wn, tm, "true" if wt else "false", pf, ",true" if xf else "")


F64, F64X = FK(2, 2, 1, False, 3), FK(2, 2, 1, False, 3, True)
N32, F128 = FK(4, 1, 1, False, 3), FK(2, 2, 2, False, 3)
D64, DN32 = FK(2, 2, 1, True, 3), FK(4, 1, 1, True, 3)
PER_T64 = 2 * 8 * 8 * 128               # floats of one slice of the t-64-128 layer

TILE_CASES = [
    _f("t-64-128-sk4", "64x64 tile, split-K 4 with finish", CONV, 2, 16, 16, 64, 128, 3, 2, 1, expect=(F64, FIN), sk=4),
    _f("t-64-128-ws-sk2", "the same layer with a workspace of two slices: the clamp gives sk = 2", CONV, 2, 16, 16, 64, 128, 3, 2, 1,
       ws_floats=2 * PER_T64 + 5, expect=(F64, FIN), sk=2),
    _f("t-64-128-nows", "the same layer with no workspace: unsplit", CONV, 2, 16, 16, 64, 128, 3, 2, 1, ws_floats=-1, expect=(F64,), sk=1),
    _f("t-64-128-lrelu", "split-K finish with LeakyReLU", CONV, 2, 16, 16, 64, 128, 3, 2, 1, act=ACT_LRELU, expect=(F64, FIN), sk=4),
    _f("t-64-128-add-nobias", "split-K finish with add, bias absent", CONV, 2, 16, 16, 64, 128, 3, 2, 1, add=True, bias=False,
       expect=(F64, FIN), sk=4),
    _f("t-64-128-add-nows", "tile epilogue with add and LeakyReLU, unsplit", CONV, 2, 16, 16, 64, 128, 3, 2, 1, add=True, act=ACT_LRELU,
       ws_floats=-1, expect=(F64,), sk=1),
    _f("t-64-128-tanh-nows", "tile epilogue with tanh", CONV, 2, 16, 16, 64, 128, 3, 2, 1, act=ACT_TANH, ws_floats=-1, expect=(F64,), sk=1,
       regimes=("randn",)),
    _f("t-xf-lrelu", "InXform (LeakyReLU) on the 64x64 tile, split", CONV, 2, 16, 16, 64, 128, 3, 2, 1, xf=ACT_LRELU, expect=(F64X, FIN), sk=4),
    _f("t-xf-none", "InXform (affine only) on the 64x64 tile, unsplit", CONV, 2, 16, 16, 64, 128, 3, 2, 1, xf=ACT_NONE, ws_floats=-1,
       expect=(F64X,), sk=1),
    _f("t-n32-split", "128x32 tile (N = 32), split", CONV, 2, 16, 16, 64, 32, 3, 2, 1, expect=(N32, FIN), sk=4),
    _f("t-n32-k1-m150", "128x32 tile unsplit (k1: two K chunks), ragged M = 150", CONV, 2, 5, 15, 64, 32, 1, 1, 0, expect=(N32,), sk=1),
    _f("t-128x64", "128x64 tile: 512 tiles of 128 rows, 81 K chunks", CONV, 8, 32, 32, 288, 512, 3, 1, 1, expect=(F128,), sk=1),
    _f("t-pf0", "single-buffer loop: 1028 workgroups", CONV, 257, 8, 8, 32, 256, 1, 1, 0, expect=(FK(2, 2, 1, False, 0),), sk=1),
    _f("t-pf0-xf", "single-buffer loop with InXform", CONV, 257, 8, 8, 32, 256, 1, 1, 0, xf=ACT_LRELU, expect=(FK(2, 2, 1, False, 0, True),), sk=1),
    _f("t-m75-n96", "ragged M (75 pixels) and ragged N (96), split", CONV, 3, 5, 5, 64, 96, 3, 1, 1, expect=(F64, FIN), sk=4),
    _f("t-m75-n160", "ragged M and N = 160 (three N tiles, the last half full), unsplit", CONV, 3, 5, 5, 32, 160, 1, 1, 0, expect=(F64,), sk=1),
    _f("t-6x10", "H != W and a grid that is no power of two (lgQw = -1)", CONV, 2, 6, 10, 64, 64, 3, 1, 1, expect=(F64, FIN), sk=4),
    _f("t-8x8", "the same layer on a power-of-two grid", CONV, 2, 8, 8, 64, 64, 3, 1, 1, expect=(F64, FIN), sk=4),
    _f("t-4x16", "H != W on a power-of-two grid", CONV, 2, 4, 16, 64, 64, 3, 1, 1, expect=(F64, FIN), sk=4),
    _f("t-6x10-s2", "H != W at stride 2 (output 3 x 5)", CONV, 2, 6, 10, 64, 64, 3, 2, 1, expect=(F64, FIN), sk=4),
]

TRANSPOSED_CASES = [
    _f("tt-k3-clsrot", "transposed k3 s2 p1 op1 (1/2/2/4 taps), split: class rows rotated by the K slice", CONVT, 2, 4, 4, 256, 64, 3, 2, 1, 1,
       expect=(F64, FIN), sk=2),
    _f("tt-k3-3x5", "transposed k3 s2 on a 3 x 5 input, unsplit", CONVT, 2, 3, 5, 64, 64, 3, 2, 1, 1, expect=(F64,), sk=1),
    _f("tt-k4-160-96", "transposed k4 s2 p1, 160 -> 96 channels, 3 x 5 input", CONVT, 2, 3, 5, 160, 96, 4, 2, 1, expect=(F64, FIN), sk=5),
]

MASKED_CASES = [
    _f("m-3-32-24", "masked <false,false,true>: 3 -> 32 at a 24 x 24 output", CONV, 2, 48, 48, 3, 32, 3, 2, 1,
       expect=("tapgemm_masked_kernel<false,false,true>",)),
    _f("m-5-6", "masked <false,false,false>: 5 -> 6", CONV, 2, 9, 11, 5, 6, 3, 1, 1, expect=("tapgemm_masked_kernel<false,false,false>",)),
    _f("m-32-3-w24", "masked <false,true,false>: 32 -> 3 at W % 32 != 0", CONV, 2, 24, 24, 32, 3, 3, 1, 1, act=ACT_TANH,
       expect=("tapgemm_masked_kernel<false,true,false>",), regimes=("randn",)),
    _f("m-32-3-w24-relu", "masked <false,true,false> with ReLU", CONV, 2, 24, 24, 32, 3, 3, 1, 1, act=ACT_RELU,
       expect=("tapgemm_masked_kernel<false,true,false>",)),
    _g("m-d-3", "masked <true,false,false>: data gradient with 3 gathered channels", CONV, 2, 24, 24, 32, 3, 3, 1, 1,
       expect=("tapgemm_masked_kernel<true,false,false>",)),
    _g("m-d-6", "masked <true,false,false>: 6 gathered channels, add and mask", CONV, 2, 9, 11, 34, 6, 3, 1, 1, add=True, mask=ACT_LRELU,
       expect=("tapgemm_masked_kernel<true,false,false>",)),
    _f("m-refuse-12", "scalar path refusal: ntaps*gC = 108 > 64", CONV, 2, 8, 8, 12, 32, 3, 1, 1, rc=ERR_BAD_ARG),
]

ENC = dict(kind=CONV, Ci=3, Co=32, k=3, s=2, p=1)
IMG = dict(kind=CONV, Ci=32, Co=3, k=3, s=1, p=1)
UPC = dict(kind=CONVT, Ci=32, Co=32, k=3, s=2, p=1, opad=1)
UPI = dict(kind=CONVT, Ci=64, Co=3, k=4, s=2, p=1)


def _d(id, hits, geo, B, H, W, op="fwd", **kw):
    return Case(id, hits, op, geo["kind"], B, H, W, geo["Ci"], geo["Co"], geo["k"], geo["s"], geo["p"], geo.get("opad", 0),
                **({"bias": False, **kw} if op == "dgrad" else kw))


THIN = "thin_tile_kernel<fwd>"
DEDICATED_CASES = [
    _d("enc-1tile", "img_enc_fwd_kernel, one tile", ENC, 1, 16, 64, act=ACT_LRELU, expect=("img_enc_fwd_kernel",)),
    _d("enc-1025", "img_enc_fwd_kernel, 1025 tiles on 1024 workgroups", ENC, 1025, 16, 64, expect=("img_enc_fwd_kernel",)),
    _d("img-1tile", "img_fwd_kernel, one tile", IMG, 1, 8, 32, expect=("img_fwd_kernel",)),
    _d("img-xf", "img_fwd_kernel with InXform", IMG, 1, 8, 32, xf=ACT_LRELU, expect=("img_fwd_kernel",)),
    _d("img-tanh", "img_fwd_kernel with tanh", IMG, 1, 8, 32, act=ACT_TANH, expect=("img_fwd_kernel",), regimes=("randn",)),
    _d("img-1025", "img_fwd_kernel, 1025 tiles on 1024 workgroups", IMG, 1025, 8, 32, expect=("img_fwd_kernel",)),
    _d("up-1tile", "up_fwd_kernel, one tile", UPC, 1, 8, 32, act=ACT_LRELU, expect=("up_fwd_kernel",)),
    _d("up-xf", "up_fwd_kernel with InXform", UPC, 1, 8, 32, xf=ACT_LRELU, expect=("up_fwd_kernel",)),
    _d("up-513", "up_fwd_kernel, 513 tiles on 512 workgroups", UPC, 513, 8, 32, expect=("up_fwd_kernel",)),
    _d("upimg-1tile", "upimg_fwd_kernel, one tile", UPI, 1, 8, 32, expect=("upimg_fwd_kernel",)),
    _d("upimg-tanh-3", "upimg_fwd_kernel, three tiles, tanh", UPI, 3, 8, 32, act=ACT_TANH, expect=("upimg_fwd_kernel",), regimes=("randn",)),
    _f("thin-32-t4", "thin kernel gC 32, <= 4 taps (transposed k4 s2)", CONVT, 1, 8, 32, 32, 3, 4, 2, 1, expect=(THIN,)),
    _f("thin-32-t9", "thin kernel gC 32, 9 taps (k3 p0, input 10 x 34)", CONV, 1, 10, 34, 32, 3, 3, 1, 0, expect=(THIN,)),
    _f("thin-32-t9-xf", "thin kernel gC 32, 9 taps, InXform and ReLU", CONV, 2, 10, 34, 32, 3, 3, 1, 0, xf=ACT_LRELU, act=ACT_RELU, expect=(THIN,)),
    _f("thin-64-t4", "thin kernel gC 64, <= 4 taps (k2)", CONV, 1, 9, 17, 64, 3, 2, 1, 0, expect=(THIN,)),
    _d("thin-64-upimg-xf", "the upimg shape with InXform: thin kernel gC 64, 4 taps per class", UPI, 1, 8, 32, xf=ACT_LRELU, expect=(THIN,)),
    _f("thin-64-t9", "thin kernel gC 64, 9 taps", CONV, 1, 8, 16, 64, 3, 3, 1, 1, expect=(THIN,)),
    _f("thin-2049", "thin kernel gC 32, 2049 tiles on 2048 workgroups", CONV, 2049, 10, 34, 32, 3, 3, 1, 0, expect=(THIN,)),
]

MASKED_ENC = "tapgemm_masked_kernel<false,false,true>"
MASKED_D = "tapgemm_masked_kernel<true,false,false>"
FALLTHROUGH_CASES = [
    _d("ft-enc-tanh", "img_enc shape with tanh: the masked kernel", ENC, 1, 16, 64, act=ACT_TANH, expect=(MASKED_ENC,), regimes=("randn",)),
    _d("ft-enc-add", "img_enc shape with add: the masked kernel", ENC, 1, 16, 64, add=True, expect=(MASKED_ENC,)),
    _d("ft-up-add", "upconv shape with add: plan.BM = 0, the 64x64 tile for N = 32", UPC, 1, 8, 32, add=True, act=ACT_LRELU, expect=(F64,), sk=1),
    _d("ft-up-add-b3", "upconv shape with add, three images (48 M tiles per class)", UPC, 3, 8, 32, add=True, expect=(F64,), sk=1),
    _d("ft-imgd-add", "img_dgrad shape with add: the masked kernel", IMG, 1, 8, 32, op="dgrad", add=True, expect=(MASKED_D,)),
    _d("ft-imgd-mask", "img_dgrad shape with mask: the masked kernel", IMG, 1, 8, 32, op="dgrad", mask=ACT_LRELU, expect=(MASKED_D,)),
]

# launch_thin_forward takes neither a residual operand nor a mask and, unlike its neighbours, does not hand the launch on: -22.
# (A mask exists only on ctvae_conv_dgrad, whose weights are transposed per tap, and no thin shape has wT = 1: thin + mask cannot
# be reached through the C ABI.)
THIN_REFUSALS = [
    _d("thin-add-img", "img_fwd shape with add", IMG, 1, 8, 32, add=True, rc=ERR_BAD_ARG),
    _d("thin-add-upimg", "upimg shape with add", UPI, 1, 8, 32, add=True, rc=ERR_BAD_ARG),
    _f("thin-add-t9", "thin shape with add", CONV, 1, 10, 34, 32, 3, 3, 1, 0, add=True, rc=ERR_BAD_ARG),
]

DGRAD_CASES = [
    _g("d-s1", "conv s1 data gradient: one class, split", CONV, 2, 8, 8, 64, 64, 3, 1, 1, expect=(D64, FIN), sk=4),
    _g("d-s1-6x10", "conv s1 data gradient, H != W", CONV, 2, 6, 10, 64, 64, 3, 1, 1, expect=(D64, FIN), sk=4),
    _g("d-s2-k3", "conv s2 k3 data gradient: classes of 1/2/2/4 taps", CONV, 2, 16, 16, 64, 128, 3, 2, 1, expect=(D64,), sk=1),
    _g("d-s2-k4", "conv s2 k4 data gradient: four classes of four taps, split (class rotation)", CONV, 2, 16, 16, 64, 64, 4, 2, 1,
       expect=(D64, FIN), sk=2),
    _g("d-s2-k4-12x20", "conv s2 k4 data gradient, 12 x 20 input", CONV, 2, 12, 20, 64, 64, 4, 2, 1, expect=(D64, FIN), sk=2),
    _g("d-s2-odd", "conv s2 data gradient of an odd input size: refused", CONV, 2, 15, 15, 64, 64, 3, 2, 1, rc=ERR_BAD_ARG),
    _g("d-t-s2", "transposed s2 data gradient: parity-grouped taps", CONVT, 2, 4, 4, 64, 64, 3, 2, 1, 1, expect=(D64, FIN), sk=4),
    _g("d-t-s2-n32", "transposed s2 data gradient into 32 channels: the 128x32 tile", CONVT, 2, 4, 6, 32, 64, 4, 2, 1, expect=(DN32, FIN), sk=8),
    _g("d-add-mask-lrelu", "add and LeakyReLU mask through splitk_finish_kernel", CONV, 2, 8, 8, 64, 64, 3, 1, 1, add=True, mask=ACT_LRELU,
       expect=(D64, FIN), sk=4),
    _g("d-mask-relu", "ReLU mask through splitk_finish_kernel", CONV, 2, 8, 8, 64, 64, 3, 1, 1, mask=ACT_RELU, expect=(D64, FIN), sk=4),
    _g("d-mask-tanh", "tanh mask through splitk_finish_kernel", CONV, 2, 8, 8, 64, 64, 3, 1, 1, mask=ACT_TANH, expect=(D64, FIN), sk=4,
       regimes=("randn",)),
    _g("d-add-mask-lrelu-nows", "add and LeakyReLU mask in the tile epilogue", CONV, 2, 8, 8, 64, 64, 3, 1, 1, add=True, mask=ACT_LRELU,
       ws_floats=-1, expect=(D64,), sk=1),
    _g("d-mask-relu-nows", "ReLU mask in the tile epilogue", CONV, 2, 8, 8, 64, 64, 3, 1, 1, mask=ACT_RELU, ws_floats=-1, expect=(D64,), sk=1),
    _g("d-mask-tanh-nows", "tanh mask in the tile epilogue", CONV, 2, 8, 8, 64, 64, 3, 1, 1, mask=ACT_TANH, ws_floats=-1, expect=(D64,), sk=1,
       regimes=("randn",)),
    _d("imgd-1tile", "img_dgrad_kernel, one tile", IMG, 1, 8, 32, op="dgrad", expect=("img_dgrad_kernel",)),
    _d("imgd-1025", "img_dgrad_kernel, 1025 tiles on 1024 workgroups", IMG, 1025, 8, 32, op="dgrad", expect=("img_dgrad_kernel",)),
    _f("flat-fwd", "CTVAE_W_CI_TAP forward: C = 64, k2", CONV | W_CI_TAP, 4, 2, 2, 64, 64, 2, 2, 0, expect=(F64, FIN), sk=2),
    _g("flat-dgrad", "CTVAE_W_CI_TAP data gradient: C = 64, k2", CONV | W_CI_TAP, 4, 2, 2, 64, 64, 2, 2, 0, expect=(D64,), sk=1),
    _g("flat-dgrad-256", "CTVAE_W_CI_TAP data gradient, 256 gathered channels, split", CONV | W_CI_TAP, 4, 2, 2, 64, 256, 2, 2, 0,
       expect=(D64, FIN), sk=2),
]

WW, WFS, WC = "wino_weight_kernel", "wino_conv_fs_kernel", "wino_conv_kernel"
WINO_CASES = [
    _f("w-fs-b16", "wino_conv_fs_kernel at the floor of 64 workgroups (8 x 8 tile blocks)", CONV, 16, 32, 32, 64, 64, 3, 1, 1, wino=True,
       act=ACT_LRELU, expect=(WW, WFS)),
    _f("w-b15-direct", "one image less: 60 workgroups, the direct kernel", CONV, 15, 32, 32, 64, 64, 3, 1, 1, wino=True, expect=(F64, FIN), sk=4),
    _f("w-full-b50", "wino_conv_kernel: 200 workgroups, one image per block (H = 16)", CONV, 50, 16, 16, 64, 256, 3, 1, 1, wino=True,
       expect=(WW, WC)),
    _f("w-h8-b62", "blocks of 4 images (H = 8), batch no multiple of the block", CONV, 62, 8, 8, 64, 256, 3, 1, 1, wino=True, expect=(WW, WFS)),
    _f("w-h4-b250", "blocks of 16 images (H = 4), batch no multiple of the block", CONV, 250, 4, 4, 64, 256, 3, 1, 1, wino=True,
       expect=(WW, WFS)),
    _f("w-add", "Winograd epilogue with add", CONV, 16, 32, 32, 64, 64, 3, 1, 1, wino=True, add=True, expect=(WW, WFS)),
    _f("w-16x64", "Winograd, H != W", CONV, 16, 16, 64, 64, 64, 3, 1, 1, wino=True, expect=(WW, WFS)),
    _g("w-dgrad", "Winograd data gradient (mirrored taps, transposed read)", CONV, 16, 32, 32, 64, 64, 3, 1, 1, wino=True, expect=(WW, WFS)),
    _g("w-dgrad-mask", "a mask keeps the data gradient off Winograd", CONV, 16, 32, 32, 64, 64, 3, 1, 1, wino=True, mask=ACT_RELU,
       expect=(D64,), sk=1),
]

RUN_CASES = TILE_CASES + TRANSPOSED_CASES + [c for c in MASKED_CASES if c.rc == 0] + DEDICATED_CASES + FALLTHROUGH_CASES + \
    [c for c in DGRAD_CASES if c.rc == 0] + WINO_CASES
REFUSED_CASES = [c for c in MASKED_CASES + DGRAD_CASES if c.rc] + THIN_REFUSALS
ALL_CASES = RUN_CASES + REFUSED_CASES

# ctvae_conv_forward_lazy: (case, slices)
LAZY_CASES = [(TILE_CASES[0], 4), (TRANSPOSED_CASES[0], 2)]
# shapes that ctvae_conv_forward_lazy_slices answers with 0: the call must refuse before any launch
LAZY_REFUSED = ["t-n32-k1-m150", "t-64-128-nows", "img-1tile", "enc-1tile", "up-1tile", "upimg-1tile", "thin-32-t9", "w-fs-b16"]

# ctvae_linear_pixmajor_forward: (B, Ci, C, P, ws_floats, supported)
PIXMAJOR = [(8, 128, 32, 4, WS_BYTES // 4, True), (8, 100, 32, 4, WS_BYTES // 4, False), (8, 128, 32, 1, WS_BYTES // 4, False),
            (8, 512, 32, 4, WS_BYTES // 4, False), (8, 512, 32, 4, 0, True)]


def case_by_id(cid):
    return next(c for c in ALL_CASES if c.id == cid)
