"""Float64 references, input makers, case tables and error bounds of the BatchNorm kernels (csrc/bn.hip), written from the
formulas at the top of that file and in include/ctvae_hip.h.  No GPU import: tests/test_bn_reference_host.py pins the references
to torch's float64 batch_norm + autograd and evaluates every case's input conditions; tests/test_bn_ops_gpu.py calls the C ABI.

Conventions (those of tests/ct_ops_checks.py, whose seed_of / gen_of / EPS32 / EXCLUDE_CAP / dot_bound are reused): inputs are
float32 tensors, references convert them to float64 first, so both sides see the same numbers.  The activation tensor is a
row-major [R = B*H*W][C] matrix, statistics are per column.

Bounds.  Every bound below is a function of float64 reference quantities and of L, the length of the longest float32 addition
(or Chan-merge) chain a value passes through on the path a case takes; L is restated from the launcher arithmetic
(stat_blocks, fwd_chain, bwd_chain, FUSED_CHAIN, TILE_CHAIN).  u = EPS32 = 2^-23.

  mean      L u (|mu| + sigma)            every partial sum rounds at the size of its terms (<= a few sigma around the shift
                                          value) and every merge rounds the running mean at the size of the mean itself
  variance  L u sigma^2 + mean_bound^2    sums of squared deviations; a mean that is off by e adds e^2 (two-pass identity).  There
                                          is NO u |mu|^2 term: that is what E[x^2] - E[x]^2 would need, and what `naive32` shows
  invstd    invstd * (var_bound / (2 (var + eps)) + 2 u)
  scale     |gamma| invstd_bound + u |scale|
  shift     |scale| mean_bound + |mu| scale_bound + u (|mu scale| + |shift|)
  z         |y - mu| scale_bound + |scale| mean_bound + u (|y scale| + |mu scale| + |shift|)
            (the SAME rounded scale multiplies y and mu, so its error counts with |y - mu|; the last term is the rounding of the
            one-FMA form itself and grows with |mu| / sigma: the inherent cost of a = act(y*scale + shift))
  a         z_bound + u |a|  (+ TANH_ABS for tanh: common.hpp promises |err| < 1e-6 of its hardware exp / rcp form)
  dgamma, dbeta   dot_bound over their summands, plus what elements inside the activation's sign margin can contribute
  g_y       the propagated coefficient errors plus u (|k1 g'| + |k2 y| + |k2 mu| + |k1 dbeta / R| + |k3| + |g_y|) * 2

SAFETY multiplies every bound.  It is calibrated on the CPU only (test_bn_reference_host.py): a plain float32 two-pass NumPy
implementation (`twopass32`) must stay inside every bound on every case, a float32 E[x^2] - E[x]^2 implementation (`naive32`)
must violate the variance bound on the `offset` cases.
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch

from tests.ct_ops_checks import EPS32, EXCLUDE_CAP, dot_bound, gen_of, seed_of  # noqa: F401  (re-exported)

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3
ACT_NAME = {0: "none", 1: "lrelu", 2: "relu", 3: "tanh"}
LEAKY = 0.01
BN_EPS = 1e-5
MOMENTUM = 0.1
TANH_ABS = 1e-6                 # common.hpp act_fwd(ACT_TANH): "|err| < 1e-6"
ERR_BAD_ARG, ERR_WORKSPACE = -22, -12
MAX_BLOCKS = 2048               # kBnMaxBlocks
# The float32 two-pass model reaches at most 0.24 of any bound over every case (scale 0.23 and invstd 0.22 at R == 1, where only
# the 2 u rounding term is left; mean <= 0.08, var <= 0.10, a <= 0.11 -- printed by test_bn_reference_host.
# test_twopass_model_is_inside_every_bound_and_naive_model_is_not): the derived formulas need no factor on top.
SAFETY = 1.0


def f64(t):
    return None if t is None else t.detach().to(torch.float64)


# ---------------------------------------------------------------------------------------------------------------------
# launcher arithmetic (bn.hip stat_blocks, launch_bn_finish_forward, launch_bn_backward), restated
# ---------------------------------------------------------------------------------------------------------------------
def shape_ok(R, C):
    """bn_shape_ok: C % 4 == 0, and C/4 divides 256 or is a multiple of it."""
    if C % 4 or R <= 0:
        return False
    Q = C // 4
    return Q % 256 == 0 if Q >= 256 else 256 % Q == 0


def row_lanes(C):
    Q = C // 4
    return 1 if Q >= 256 else 256 // Q


def stat_blocks(R, C):
    """(partial rows, rows per block) of bn_stats_partial_kernel / bn_bwd_partial_kernel."""
    nb = max(1, min(MAX_BLOCKS, R // (row_lanes(C) * 8)))
    rpb = -(-R // nb)
    return -(-R // rpb), rpb


def workspace_floats(C):
    return MAX_BLOCKS * C * 3 + 5 * C


def fwd_labels(R, C, training=True):
    """The launches of ctvae_bn_forward, in order."""
    if not training:
        return ["bn_apply_act_kernel"]                      # bn_eval_coeff_kernel carries no log label
    nb, _ = stat_blocks(R, C)
    if nb <= 128 and C % 32 == 0:
        return ["bn_stats_partial_kernel", "bn_finalize_apply_kernel"]
    return ["bn_stats_partial_kernel", "bn_finalize_kernel", "bn_apply_act_kernel"]


def fwd_chain(R, C):
    """L of the stand-alone forward statistics: rows a lane of bn_stats_partial_kernel adds, the row lanes its first lane
    merges, and the merges of the finalize (finalize_apply: ceil(nb/8) rows per lane, then 7 lanes; finalize: ceil(nb/256)
    rows per lane, then an 8-level tree)."""
    nb, rpb = stat_blocks(R, C)
    rl = row_lanes(C)
    fin = -(-nb // 8) + 7 if (nb <= 128 and C % 32 == 0) else -(-nb // 256) + 8
    return -(-rpb // rl) + (rl - 1) + fin


def bwd_chain(R, C):
    """L of bn_bwd_partial_kernel's two sums: rows per lane + row lanes; the partial rows are then added in double (+ 2: the
    casts).  + 3 for the roundings of xhat = (y - mean) * invstd and of the product g' * xhat."""
    _, rpb = stat_blocks(R, C)
    rl = row_lanes(C)
    return -(-rpb // rl) + (rl - 1) + 2 + 3


# bn_fused_fwd/bwd_kernel: 4 rows per thread, 6 butterfly steps of a wave, up to 16 wave sums; + 3 as in bwd_chain
FUSED_CHAIN = 4 + 6 + 16 + 3
# statistics from a conv epilogue: at most 64 rows per lane, at most 8 merges inside the tile, then the finalize over the tile
# rows (one-launch form: at most 128 rows, 16 per lane + 7 lanes; the few-row shapes of the tests stay far below)
TILE_CHAIN = 64 + 8 + 16 + 7


def fused_ok(R, C):
    return R > 0 and R % 4 == 0 and C % 4 == 0 and R <= 4096 and R * C <= 1 << 20


def fused_instance(R, C):
    """(threads, channels per workgroup, slices in flight) of the channel-owner kernels."""
    cpw = 2 if C < 256 else 4
    return (64, cpw, 8) if R <= 256 else (256, cpw, 8) if R <= 1024 else (1024, cpw, 4)


def row_map(B, Qh, Qw, s):
    """pix[r] of the class-major row r = cls*Mc + (b*Qh + qy)*Qw + qx, Mc = B*Qh*Qw, cls = py*s + px: pixel
    (b, qy*s + py, qx*s + px) of the [B][Qh*s][Qw*s] tensor (geom.hpp line 10: spix(m) = (b, qy*os + py, qx*os + px) per
    output-parity class).  The identity for s == 1."""
    Mc = B * Qh * Qw
    r = torch.arange(s * s * Mc)
    cls, m = r // Mc, r % Mc
    b, qy, qx = m // (Qh * Qw), (m // Qw) % Qh, m % Qw
    return (b * Qh * s + qy * s + cls // s) * (Qw * s) + qx * s + cls % s


# ---------------------------------------------------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------------------------------------------------
def act64(z, act):
    if act == ACT_LRELU:
        return torch.where(z > 0, z, z * LEAKY)
    if act == ACT_RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == ACT_TANH:
        return torch.tanh(z)
    return z


def dact64(z, act):
    if act == ACT_LRELU:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, LEAKY))
    if act == ACT_RELU:
        return (z > 0).to(z.dtype)
    if act == ACT_TANH:
        return 1.0 - torch.tanh(z) ** 2
    return torch.ones_like(z)


def slope_gap(act):
    """|slope_hi - slope_lo| of the two branches of a piecewise-linear activation."""
    return {ACT_LRELU: 1.0 - LEAKY, ACT_RELU: 1.0}.get(act, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def forward_ref(y, gamma, beta, rm, rv, act, training=True, eps=BN_EPS, momentum=MOMENTUM):
    """dict of float64 tensors.  Training: batch statistics, running statistics updated with the unbiased variance (the
    biased one at R == 1, as the kernels do), nbt_inc = 1.  Eval: the running statistics, nothing changes."""
    y, gamma, beta, rm, rv = (f64(t) for t in (y, gamma, beta, rm, rv))
    R = y.shape[0]
    if training:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
        unb = var * R / (R - 1) if R > 1 else var
        rm1, rv1 = (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * unb
    else:
        mean, var, rm1, rv1 = rm, rv, rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    z = (y - mean) * scale + beta
    return dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, z=z, a=act64(z, act), running_mean=rm1,
                running_var=rv1, nbt_inc=1 if training else 0)


def forward_bounds(y, ref, gamma, rm, rv, L, act, training=True, eps=BN_EPS, momentum=MOMENTUM):
    """Bounds of the forward outputs (see the module docstring); elementwise `z` and `a`, per channel otherwise."""
    y, gamma = f64(y), f64(gamma)
    R = y.shape[0]
    mu, var, invstd, scale, shift = ref["mean"], ref["var"], ref["invstd"], ref["scale"], ref["shift"]
    sigma = var.sqrt()
    if training:
        mean_b = L * EPS32 * (mu.abs() + sigma)
        var_b = L * EPS32 * var + mean_b ** 2
    else:
        mean_b, var_b = torch.zeros_like(mu), torch.zeros_like(mu)
    invstd_b = invstd * (var_b / (2 * (var + eps)) + 2 * EPS32)
    scale_b = gamma.abs() * invstd_b + EPS32 * scale.abs()
    shift_b = scale.abs() * mean_b + mu.abs() * scale_b + EPS32 * ((mu * scale).abs() + shift.abs())
    z_b = (y - mu).abs() * scale_b + scale.abs() * mean_b + EPS32 * ((y * scale).abs() + (mu * scale).abs() + shift.abs())
    a_b = z_b + EPS32 * ref["a"].abs() + (TANH_ABS if act == ACT_TANH else 0.0)
    unb = R / (R - 1) if R > 1 else 1.0
    # (1 - m) * old + m * new: 1 - m, 0.1f itself, two products and the sum round (<= 2.5 u/2 per term)
    rm_b = momentum * mean_b + 2 * EPS32 * (((1 - momentum) * f64(rm)).abs() + (momentum * mu).abs())
    rv_b = momentum * unb * var_b + 2 * EPS32 * (((1 - momentum) * f64(rv)).abs() + momentum * unb * var)
    out = dict(mean=mean_b, var=var_b, invstd=invstd_b, scale=scale_b, shift=shift_b, z=z_b, a=a_b, running_mean=rm_b,
               running_var=rv_b)
    return {k: SAFETY * v for k, v in out.items()}


def backward_ref(g_a, y, gamma, beta, mean, invstd, act):
    """Autograd of a = act(gamma*xhat + beta), xhat = (y - mean)*invstd with batch statistics, written out: g' = g_a * act'(z),
    dgamma = sum g' xhat, dbeta = sum g', g_y = gamma invstd (g' - dbeta/R - xhat dgamma/R) = k1 g' + k2 y + k3.  mean / invstd
    are the saved float32 statistics (inputs of the backward kernels).  coef [7][C]: k1, k2, k3, scale, shift, dgamma, dbeta
    (finish.hpp BnFinJob); rows 0-4 are the [5][C] block."""
    g_a, y, gamma, beta, mean, invstd = (f64(t) for t in (g_a, y, gamma, beta, mean, invstd))
    R = y.shape[0]
    xhat = (y - mean) * invstd
    z = gamma * xhat + beta
    gp = g_a * dact64(z, act)
    dgamma, dbeta = (gp * xhat).sum(0), gp.sum(0)
    k1 = gamma * invstd
    k2 = -k1 * dgamma / R * invstd
    k3 = -k1 * dbeta / R - k2 * mean
    gy = k1 * (gp - dbeta / R - xhat * dgamma / R)
    coef = torch.stack([k1, k2, k3, k1, beta - mean * k1, dgamma, dbeta])
    return dict(xhat=xhat, z=z, gp=gp, dgamma=dgamma, dbeta=dbeta, gy=gy, gy_coef=k1 * gp + k2 * y + k3, coef=coef)


def backward_bounds(g_a, y, gamma, beta, mean, invstd, ref, L, act, ga_err=None):
    """Bounds of the backward outputs.  `exclude` marks the elements whose |z| lies inside the margin within which the kernels'
    recomputed sign of z may differ (both forms they use: gamma*xhat + beta and y*scale + shift); those are left out of the
    elementwise g_y check and their possible contribution enters the dgamma / dbeta bounds.  ga_err: elementwise bound of an
    error already in g_a (the float32 sum of split-K slices)."""
    g_a, y, gamma, beta, mean, invstd = (f64(t) for t in (g_a, y, gamma, beta, mean, invstd))
    R = y.shape[0]
    xhat, z, gp, coef = ref["xhat"], ref["z"], ref["gp"], ref["coef"]
    k1, k2, k3, shift, dgamma, dbeta = coef[0], coef[1], coef[2], coef[4], coef[5], coef[6]
    z_b = EPS32 * ((y * k1).abs() + (mean * k1).abs() + shift.abs() + 2 * (gamma * xhat).abs() + beta.abs() + z.abs())
    gap = slope_gap(act)
    exclude = (z.abs() <= z_b) if gap else torch.zeros_like(z, dtype=torch.bool)
    gp_b = EPS32 * gp.abs()
    if act == ACT_TANH:                   # act' = 1 - o^2, |d act'| <= 2 |d o|, d o <= z_b + TANH_ABS
        gp_b = gp_b + g_a.abs() * 2 * (z_b + TANH_ABS)
    if ga_err is not None:
        gp_b = gp_b + ga_err
    flip = g_a.abs() * gap * exclude
    db_b = dot_bound(L, gp.abs().sum(0)) + gp_b.sum(0) + flip.sum(0)
    dg_b = dot_bound(L, (gp * xhat).abs().sum(0)) + (gp_b * xhat.abs()).sum(0) + (flip * xhat.abs()).sum(0)
    k1_b = EPS32 * k1.abs()
    k2_b = (k1 * invstd).abs() / R * dg_b + 2 * EPS32 * k2.abs()
    k3_b = k1.abs() / R * db_b + mean.abs() * k2_b + EPS32 * (2 * (k1 * dbeta / R).abs() + (k2 * mean).abs() + k3.abs())
    shift_b = EPS32 * ((mean * k1).abs() + shift.abs())
    gy_b = (k1.abs() * gp_b + k1.abs() / R * db_b + (y - mean).abs() * ((k1 * invstd).abs() / R * dg_b)
            + 2 * EPS32 * ((k1 * gp).abs() + (k2 * y).abs() + (k2 * mean).abs() + (k1 * dbeta / R).abs() + k3.abs() + ref["gy"].abs()))
    coef_b = torch.stack([k1_b, k2_b, k3_b, k1_b, shift_b, dg_b + EPS32 * dgamma.abs(), db_b + EPS32 * dbeta.abs()])
    out = dict(dgamma=dg_b + EPS32 * dgamma.abs(), dbeta=db_b + EPS32 * dbeta.abs(), gy=gy_b, coef=coef_b)
    out = {k: SAFETY * v for k, v in out.items()}
    out["exclude"] = exclude
    out["z"] = z_b
    return out


# ---------------------------------------------------------------------------------------------------------------------
# float32 models for the calibration on the CPU
# ---------------------------------------------------------------------------------------------------------------------
def _finish32(y, mean, var, gamma, beta, act):
    f = np.float32
    invstd = (f(1.0) / np.sqrt(var + f(BN_EPS))).astype(f)
    scale = (gamma * invstd).astype(f)
    shift = (beta - mean * scale).astype(f)
    z = (y * scale + shift).astype(f)
    a = torch.from_numpy(z)
    a = act64(a, act) if act != ACT_TANH else torch.tanh(a.double()).float()
    return dict(mean=torch.from_numpy(mean), var=torch.from_numpy(var), invstd=torch.from_numpy(invstd),
                scale=torch.from_numpy(scale), shift=torch.from_numpy(shift), a=a)


def twopass32(y, gamma, beta, act):
    """Plain float32 two-pass batch statistics + the scale / shift form, every operation in float32 (NumPy)."""
    f = np.float32
    y, gamma, beta = (t.numpy().astype(f) for t in (y, gamma, beta))
    R = f(y.shape[0])
    yt = np.ascontiguousarray(y.T)                                 # sums along the contiguous axis: NumPy's pairwise summation
    mean = (yt.sum(1, dtype=f) / R).astype(f)
    d = (yt - mean[:, None]).astype(f)
    var = ((d * d).sum(1, dtype=f) / R).astype(f)
    return _finish32(y, mean, var, gamma, beta, act)


def naive32(y, gamma, beta, act):
    """Deliberately naive float32 E[x^2] - E[x]^2 (what the Chan merge and the shifted sums exist to avoid)."""
    f = np.float32
    y, gamma, beta = (t.numpy().astype(f) for t in (y, gamma, beta))
    R = f(y.shape[0])
    yt = np.ascontiguousarray(y.T)
    mean = (yt.sum(1, dtype=f) / R).astype(f)
    ex2 = ((yt * yt).sum(1, dtype=f) / R).astype(f)
    var = np.maximum(ex2 - mean * mean, f(0)).astype(f)
    return _finish32(y, mean, var, gamma, beta, act)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def const_channels(C):
    """The channels of a `const` input whose rows all hold one value."""
    return sorted({0, C // 2 + 1, C - 1})


@lru_cache(maxsize=2)
def make_y(cid, R, C, kind):
    """y [R, C] float32.  o1: randn.  offset: per channel std log-uniform in 1e-2 .. 1e2 and a mean of +-(1 .. 1e3, log-uniform)
    times that std.  const: o1 with the channels of const_channels() constant (var == 0)."""
    g = gen_of(cid, {"o1": 1, "offset": 2, "const": 3}[kind])
    y = torch.randn(R, C, generator=g, dtype=torch.float32)
    if kind == "offset":
        std = 10.0 ** (torch.rand(C, generator=g) * 4 - 2)
        ratio = 10.0 ** (torch.rand(C, generator=g) * 3)
        ratio[0] = 1e3                                            # the extreme is always present
        sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
        y = (y.double() * std.double() + (sign * ratio * std).double()).float()
    elif kind == "const":
        vals = torch.randn(C, generator=g) * 50.0
        for c in const_channels(C):
            y[:, c] = vals[c]
    return y


def make_params(cid, C):
    """gamma in [0.5, 1.5) with a few negative entries, beta in [-0.5, 0.5), non-trivial running statistics."""
    g = gen_of(cid, 7)
    gamma = torch.rand(C, generator=g) + 0.5
    gamma[1::5] *= -1.0
    beta = torch.rand(C, generator=g) - 0.5
    rm = torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.5
    return gamma, beta, rm, rv


def make_ga(cid, R, C, kind="randn", salt=0):
    g = gen_of(cid, 11 + salt)
    if kind == "int":
        return torch.randint(-3, 4, (R, C), generator=g).float()
    return torch.randn(R, C, generator=g)


def saved_stats(y):
    """save_mean / save_invstd of the float64 reference rounded to float32: the backward kernels' inputs."""
    y = f64(y)
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    return mean.float(), (1.0 / torch.sqrt(var + BN_EPS)).float()


def random_partition(cid, R, rows, salt=0):
    """`rows` disjoint index sets that cover 0 .. R-1 (some may be empty when rows > R)."""
    g = gen_of(cid, 23 + salt)
    owner = torch.randint(0, rows, (R,), generator=g)
    owner[:min(rows, R)] = torch.randperm(rows, generator=g)[:min(rows, R)]
    return [torch.nonzero(owner == i).flatten() for i in range(rows)]


def partial_rows(ref, parts):
    """part [rows][C][2] = (sum g', sum g' xhat) over each index set, in float64, rounded to float32; and the float64 sums of the
    ROUNDED rows: the dgamma / dbeta a kernel that is handed these rows must reproduce."""
    gp, gx = ref["gp"], ref["gp"] * ref["xhat"]
    part = torch.stack([torch.stack([gp[i].sum(0), gx[i].sum(0)], -1) for i in parts]).float()
    return part, part.double().sum(0)


def split_slices(cid, g_a, S, pix, salt=0):
    """[S][C][R] float32 slices whose float64 sum, read through the row map pix, is g_a [R][C]; and the sum of |slice|."""
    g = gen_of(cid, 31 + salt)
    R, C = g_a.shape
    cm = g_a.double()[pix].t().contiguous()                        # [C][R'], row r' holds pixel pix[r']
    parts = (torch.randn(S - 1, C, R, generator=g) * 0.7).float() if S > 1 else torch.zeros(0, C, R)
    last = (cm - parts.double().sum(0)).float()
    slices = torch.cat([parts, last[None]], 0)
    total = slices.double().sum(0)                                 # what the slices really add up to: the reference's g_a
    inv = torch.empty_like(pix)
    inv[pix] = torch.arange(R)
    return slices, total.t()[inv].contiguous(), slices.double().abs().sum(0).t()[inv].contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------------------------------
Fwd = namedtuple("Fwd", "id R C kind act why")
FWD_CASES = [
    Fwd("R1-C32", 1, 32, "o1", ACT_LRELU, "n == 1: biased running variance"),
    Fwd("R4099-C32", 4099, 32, "offset", ACT_LRELU, "16 partial rows; finalize_apply with 128 row ranges and the `two` tail"),
    Fwd("R4099-C32-const", 4099, 32, "const", ACT_TANH, "zero-variance channels"),
    Fwd("R37-C512", 37, 512, "offset", ACT_RELU, "16 channel blocks"),
    Fwd("R9-C2048", 9, 2048, "o1", ACT_NONE, "two quad passes of bn_stats_partial_kernel"),
    Fwd("R16519-C64", 16519, 64, "offset", ACT_TANH, "129 partial rows: finalize + fast apply loop"),
    Fwd("R38407-C64", 38407, 64, "o1", ACT_LRELU, "more than 256 partial rows"),
    Fwd("R3-C8", 3, 8, "const", ACT_RELU, "C % 32 != 0"),
    Fwd("R1029-C4", 1029, 4, "offset", ACT_NONE, "C % 32 != 0"),
    Fwd("R2053-C2048", 2053, 2048, "o1", ACT_TANH, "finalize + generic apply loop"),
    Fwd("R4194309-C4-clamp", 2048 * 2048 + 5, 4, "offset", ACT_LRELU, "block count clamped at 2048: the largest R"),
]
FWD_PARTIAL_ROWS = {"R1-C32": 1, "R4099-C32": 16, "R4099-C32-const": 16, "R37-C512": 2, "R9-C2048": 1, "R16519-C64": 129,
                    "R38407-C64": 298, "R3-C8": 1, "R1029-C4": 1, "R2053-C2048": 229, "R4194309-C4-clamp": 2048}
EVAL_CASES = [Fwd("eval-R5-C2048", 5, 2048, "offset", ACT_LRELU, "generic apply loop"),
              Fwd("eval-R33-C32", 33, 32, "o1", ACT_TANH, "fast apply loop")]

Bwd = namedtuple("Bwd", "id R C kind act form rows")
# plain: partial + finalize + apply over the forward shapes (all but the 16.8 M element one)
BWD_PLAIN = [Bwd("plain-" + c.id, c.R, c.C, c.kind, c.act, "plain", 0) for c in FWD_CASES if c.R * c.C < 1 << 23]
BWD_INT = [Bwd("int-R4099-C32", 4099, 32, "o1", ACT_NONE, "plain", 0), Bwd("int-R37-C512", 37, 512, "offset", ACT_NONE, "plain", 0),
           Bwd("int-R2053-C2048", 2053, 2048, "o1", ACT_NONE, "plain", 0)]
BWD_PART_ONE = [Bwd(f"part{rows}-R{R}-C{C}", R, C, kind, act, "part-one", rows)
                for rows, C, R, kind, act in [(1, 32, 33, "o1", ACT_LRELU), (7, 512, 33, "offset", ACT_RELU), (256, 32, 4099, "offset", ACT_TANH),
                                              (7, 32, 4099, "const", ACT_NONE), (256, 512, 33, "o1", ACT_LRELU), (1, 512, 4099, "o1", ACT_TANH)]]
BWD_PART_TWO = [Bwd("part257-R4099-C32", 4099, 32, "offset", ACT_LRELU, "part-two", 257),
                Bwd("part5-R1029-C8", 1029, 8, "o1", ACT_RELU, "part-two", 5)]
BWD_COEF_OUT = [Bwd("coefout-R4099-C32", 4099, 32, "offset", ACT_LRELU, "coef-out", 0),
                Bwd("coefout-R37-C512", 37, 512, "o1", ACT_TANH, "coef-out", 0)]
BWD_COEF_IN = [Bwd("coefin-R4099-C32", 4099, 32, "offset", ACT_RELU, "coef-in", 0),
               Bwd("coefin-R37-C2048", 37, 2048, "o1", ACT_LRELU, "coef-in", 0)]
BWD_CASES = BWD_PLAIN + BWD_PART_ONE + BWD_PART_TWO + BWD_COEF_OUT + BWD_COEF_IN
BWD_LABELS = {"plain": ["bn_bwd_partial_kernel", "bn_bwd_finalize_kernel", "bn_bwd_apply_kernel"],
              "part-one": ["bn_bwd_finalize_apply_kernel"], "part-two": ["bn_bwd_finalize_kernel", "bn_bwd_apply_kernel"],
              "coef-out": ["bn_bwd_partial_kernel", "bn_bwd_finalize_kernel"], "coef-in": ["bn_bwd_apply_kernel"]}


def bwd_case_chain(case):
    """L of a backward case: the kernel's own float32 sums, or 2 where float32 partial rows are handed in and added in double."""
    return bwd_chain(case.R, case.C) if case.form in ("plain", "coef-out") else 2 + 3


# ctvae_bn_backward_fused: the BatchNorm's tensor is [B][H][W][C], the slices were written by the data gradient of a layer
# (kind, k, stride, pad, out_pad) whose INPUT that tensor is.  stride 1: identity row map; stride 2 (conv): class-major rows.
Fused = namedtuple("Fused", "id B H W C S stride act kind")
FUSED_CASES = [
    Fused("R12-C8-ident", 3, 2, 2, 8, 1, 1, ACT_LRELU, "o1"),
    Fused("R12-C256-div-B3", 3, 2, 2, 256, 3, 2, ACT_RELU, "offset"),            # Mc = 3: division path
    Fused("R256-C8-pow2", 1, 16, 16, 8, 9, 2, ACT_TANH, "o1"),                  # S = 9: one slice beyond the unroll of eight
    Fused("R256-C256-ident", 4, 8, 8, 256, 8, 1, ACT_NONE, "offset"),
    Fused("R260-C8-ident", 1, 26, 10, 8, 3, 1, ACT_RELU, "const"),               # 256 threads, lanes beyond R
    Fused("R264-C256-div-Qw3", 1, 44, 6, 256, 1, 2, ACT_LRELU, "o1"),            # Qw = 3: division path
    Fused("R1024-C8-pow2", 4, 16, 16, 8, 8, 2, ACT_LRELU, "offset"),
    Fused("R1024-C256-ident", 1, 32, 32, 256, 3, 1, ACT_TANH, "o1"),
    Fused("R1028-C8-ident", 1, 257, 4, 8, 9, 1, ACT_NONE, "o1"),                 # 1024 threads (4 slices in flight), lanes beyond R
    Fused("R1032-C256-div-Qw3", 1, 172, 6, 256, 3, 2, ACT_RELU, "o1"),
    Fused("R4096-C8-pow2", 1, 64, 64, 8, 3, 2, ACT_TANH, "offset"),
    Fused("R4096-C256-pow2", 4, 32, 32, 256, 1, 2, ACT_LRELU, "o1"),
    Fused("R64-C512-perm", 1, 8, 8, 512, 3, 2, ACT_LRELU, "offset"),             # C % 256 == 0: fused_group permutes the groups
    Fused("R12-C768-perm-div", 3, 2, 2, 768, 9, 2, ACT_RELU, "o1"),
]


def fused_geom(case):
    """(kind CONV, B, H, W, Ci = C, Co, k, stride, pad, out_pad) of the layer whose data gradient wrote the slices."""
    return (0, case.B, case.H, case.W, case.C, 8, 3, case.stride, 1, 0)


def fused_pix(case):
    s = case.stride
    return row_map(case.B, case.H // s, case.W // s, s)


# ctvae_conv_bn_act_forward: transposed, B, H, Ci, Co, k, s, p, op, act, lazy (a_out NULL, coefficients out), what must run
Conv = namedtuple("Conv", "id tr B H Ci Co k s p op act lazy label")
CONV_FUSED_CASES = [
    Conv("conv-s2-R128-C256", False, 8, 8, 128, 256, 3, 2, 1, 0, ACT_LRELU, False, "bn_fused_fwd_kernel"),       # dense slices, 64 threads
    Conv("convT-R128-C128", True, 8, 2, 256, 128, 3, 2, 1, 1, ACT_RELU, False, "bn_fused_fwd_kernel"),          # class-major, 2-channel owners
    Conv("conv-s2-R12-C256-oddB", False, 3, 4, 128, 256, 3, 2, 1, 0, ACT_TANH, True, "bn_fused_fwd_kernel"),     # lanes beyond R, lazy output
    Conv("conv-s2-R512-C128", False, 8, 16, 64, 128, 3, 2, 1, 0, ACT_NONE, True, "bn_fused_fwd_kernel"),        # 256 threads
    Conv("conv-s2-R2048-C64", False, 8, 32, 32, 64, 3, 2, 1, 0, ACT_LRELU, False, "bn_fused_fwd_kernel"),       # 1024 threads
]
CONV_UNSPLIT_CASES = [
    Conv("tile-32to64", False, 64, 32, 32, 64, 3, 2, 1, 0, ACT_LRELU, False, None),       # general tile kernel; fewer rows split K
    Conv("masked-3to64-k4", False, 2, 64, 3, 64, 4, 2, 1, 0, ACT_RELU, True, None),       # its masked variant (Ci = 3)
    Conv("imgenc-3to32", False, 3, 64, 3, 32, 3, 2, 1, 0, ACT_LRELU, False, None),        # image.hip encoder
    Conv("upconv-32to32", True, 1, 64, 32, 32, 3, 2, 1, 1, ACT_TANH, True, None),         # upconv.hip
]
