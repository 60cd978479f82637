"""Float64 references, input makers, case tables and error bounds of kernels that turn network outputs into a latent sample and a
scalar objective, written from the formulas in the kernel files' headers and in include/ctvae_hip.h:

  csrc/loss.hip; reparam_*, gauss_latent_*, act_* of csrc/pointwise.hip; csrc/ladder.hip; csrc/tcvae.hip; csrc/vamp.hip;
  csrc/swd.hip; csrc/gamma.hip (reparameterisation, KL term, sigmoid); csrc/dip.hip; csrc/catlatent.hip; csrc/mmd.hip;
  csrc/iwloss.hip; csrc/ssim.hip.

No GPU import.  tests/test_loss_reference_host.py pins the references to oracle/vae_cpu.py (or to the torch expression the model
tests use) and evaluates every case's input conditions; tests/test_loss_ops_gpu.py calls the C ABI.

Conventions (those of tests/ct_ops_checks.py, whose seed_of / gen_of / EPS32 are reused): inputs are float32 tensors, references
convert them to float64 first, so both sides see the same numbers.  Scalars that cross the C ABI as `float` (M_N, alpha) are
rounded to float32 before the reference uses them.  Gradients come from torch.autograd in float64.

Bounds.  u = EPS32 = 2^-23 (one ulp at 1: twice the unit roundoff, so "one rounding" is counted as u |result| with a factor 2 in
hand).  Every bound is  u * (c_chain + c_fn) * A  per output element:

  A        the float64 reference with every summand replaced by its magnitude
  c_chain  the longest float32 addition chain the kernel's code shows (restated from the launcher arithmetic below);
           reductions finished in double count only their float32 part
  c_fn     roundings of the element's own expression: 1 per +, *, /, expf, logf, sqrtf (each correct to 1 ulp), and what an
           argument's rounding costs behind a function: exp(x (1 + k u)) = exp(x) (1 + k |x| u); for the fast intrinsics
           __expf(x): (2 + |x|) u relative, __frcp_rn: 1

Where c_fn differs per element (log-cosh: |x| = |2 alpha d| up to 60) it is carried as a per-element tensor and summed with the
terms.  No bound was tuned on a kernel.
"""
from collections import namedtuple

import numpy as np
import torch

from tests.ct_ops_checks import EPS32, gen_of, seed_of  # noqa: F401  (re-exported)

ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH = 0, 1, 2, 3
ACT_NAME = {0: "none", 1: "lrelu", 2: "relu", 3: "tanh"}
LEAKY = float(np.float32(0.01))
TANH_ABS = 1e-6                  # common.hpp act_fwd(ACT_TANH): "|err| < 1e-6"
ERR_BAD_ARG, ERR_WORKSPACE = -22, -12
LOGCOSH_ALPHA = 10.0             # configs/logcosh_vae.yaml
LOSS_BLOCKS, BWD_BLOCKS = 1024, 4096        # kLossBlocks; the cap of launch_mse_backward / launch_loss_backward / grid_for
LOSS_WS_FLOATS = 2 * LOSS_BLOCKS
MARGIN = 1e-3                    # sign / threshold decisions: a value is exactly 0 or at least this far from it
NAN_SCALE = 1.0                  # outputs start as NaN; a finite stand-in of scale 1 is what "far below" is measured against
N_FWD_WRAP = 4 * (256 * LOSS_BLOCKS + 300) + 3      # 1 049 779: the forward loop takes a second round, tail of 3
N_BWD_WRAP = 4 * (BWD_BLOCKS * 256 + 300) + 3       # 4 195 507: the backward loops take a second round


def f64(t):
    return None if t is None else t.detach().to(torch.float64)


def f32s(v):
    """A host scalar as the kernel receives it: rounded to float32."""
    return float(np.float32(v))


def case_of(cases, cid):
    return next(c for c in cases if c.id == cid)


def act_grad_from_out(o, act):
    """act_bwd_from_out of common.hpp on a float64 tensor: LRELU o > 0 ? 1 : 0.01f, RELU o > 0 ? 1 : 0, TANH 1 - o^2."""
    if act == ACT_LRELU:
        return torch.where(o > 0, torch.ones_like(o), torch.full_like(o, LEAKY))
    if act == ACT_RELU:
        return (o > 0).to(o.dtype)
    if act == ACT_TANH:
        return 1.0 - o * o
    return torch.ones_like(o)


def act_fwd64(v, act):
    if act == ACT_LRELU:
        return torch.where(v > 0, v, v * LEAKY)
    if act == ACT_RELU:
        return torch.where(v > 0, v, torch.zeros_like(v))
    if act == ACT_TANH:
        return torch.tanh(v)
    return v


# ---------------------------------------------------------------------------------------------------------------------
# csrc/loss.hip
# ---------------------------------------------------------------------------------------------------------------------
# layout of mu / logvar: dense [B][L]; the two halves of one [B][2L] tensor (row stride 2L); column slices of a [B][2L + 3]
# tensor (row stride 2L + 3, columns 1 .. L and L + 2 .. 2L + 1); none (mu = logvar = NULL)
LossCase = namedtuple("LossCase", "id mode n B L layout M_N extra ract why")
LOSS_CASES = [
    LossCase("mse-n1", "mse", 1, 1, 1, "dense", 0.00025, False, ACT_NONE, "tail only, one element; one KL element"),
    LossCase("mse-n3", "mse", 3, 6, 128, "halves", 4.0, True, ACT_LRELU, "tail of 3 without a vector part; KL strided over one block; extra"),
    LossCase("mse-n4", "mse", 4, 7, 33, "slices", 0.00025, False, ACT_RELU, "no tail; GaussKL's n = 4: KL loop over a one-block grid"),
    LossCase("mse-n5", "mse", 5, 7, 33, "dense", 0.0, True, ACT_TANH, "tail of 1; M_N = 0"),
    LossCase("mse-n1027", "mse", 1027, 6, 128, "slices", 4.0, False, ACT_LRELU, "two blocks, tail of 3; KL against two blocks"),
    LossCase("mse-n1027-nokl", "mse", 1027, 0, 0, "none", 0.00025, True, ACT_NONE, "mu = logvar = NULL: out[2] = out[3] = 0"),
    LossCase("mse-fwdwrap", "mse", N_FWD_WRAP, 7, 33, "halves", 0.00025, True, ACT_TANH, "forward loop wraps at 1024 blocks; KL against many blocks"),
    LossCase("mse-bwdwrap", "mse", N_BWD_WRAP, 6, 128, "dense", 0.00025, False, ACT_RELU, "backward loops wrap at 4096 blocks"),
    LossCase("mse-kl11-many", "mse", 1027 * 64, 1, 1, "dense", 4.0, False, ACT_NONE, "(B, L) = (1, 1) against a grid of many blocks"),
    LossCase("logcosh-n1", "logcosh", 1, 1, 1, "dense", 0.00025, False, ACT_NONE, "MODE 1 tail only"),
    LossCase("logcosh-n3", "logcosh", 3, 7, 33, "halves", 4.0, False, ACT_TANH, "MODE 1 tail of 3"),
    LossCase("logcosh-n4", "logcosh", 4, 6, 128, "slices", 0.00025, False, ACT_LRELU, "MODE 1 no tail"),
    LossCase("logcosh-n5", "logcosh", 5, 0, 0, "none", 0.0, False, ACT_NONE, "MODE 1 tail of 1, no KL"),
    LossCase("logcosh-n1027", "logcosh", 1027, 7, 33, "dense", 0.00025, False, ACT_RELU, "MODE 1 two blocks"),
    LossCase("logcosh-fwdwrap", "logcosh", N_FWD_WRAP, 6, 128, "dense", 0.00025, False, ACT_NONE, "MODE 1 forward wrap"),
    LossCase("logcosh-bwdwrap", "logcosh", N_BWD_WRAP, 7, 33, "slices", 0.00025, False, ACT_TANH, "MODE 1 backward wrap"),
    LossCase("l2l1-n1", "l2l1", 1, 0, 0, "none", 0.0, False, ACT_NONE, "MODE 2 tail only"),
    LossCase("l2l1-n3", "l2l1", 3, 0, 0, "none", 0.0, True, ACT_LRELU, "MODE 2 tail of 3; extra"),
    LossCase("l2l1-n4", "l2l1", 4, 0, 0, "none", 0.0, False, ACT_TANH, "MODE 2 no tail"),
    LossCase("l2l1-n5", "l2l1", 5, 0, 0, "none", 0.0, True, ACT_RELU, "MODE 2 tail of 1"),
    LossCase("l2l1-n1027", "l2l1", 1027, 0, 0, "none", 0.0, False, ACT_NONE, "MODE 2 two blocks; recons == x on a tenth"),
    LossCase("l2l1-fwdwrap", "l2l1", N_FWD_WRAP, 0, 0, "none", 0.0, True, ACT_TANH, "MODE 2 forward wrap"),
    LossCase("l2l1-bwdwrap", "l2l1", N_BWD_WRAP, 0, 0, "none", 0.0, False, ACT_LRELU, "MODE 2 backward wrap"),
]
G_LOSS = (1.0, -0.37)


def alpha_of(case):
    return LOGCOSH_ALPHA if case.mode == "logcosh" else 0.0


def head_views(heads, case):
    """(mu, logvar) as views of the one allocation `heads` (host or device) in the case's layout."""
    B, L = case.B, case.L
    if case.layout == "dense":
        return heads[:B], heads[B:]
    if case.layout == "halves":
        return heads[:, :L], heads[:, L:]
    return heads[:, 1:1 + L], heads[:, L + 2:2 * L + 2]


def loss_inputs(case, far=False):
    """dict(r, x [n]; mu, lv views [B][L] of `heads` (or None); extra [1] or None).
    recons is the output of case.ract: tanh(v) for TANH; for LRELU / RELU act(v) with exact zeros planted on a twentieth of the
    elements and every other value at least MARGIN from 0.  log-cosh draws both pictures from [0, 3): |2 alpha d| < 60.
    l2 + l1: recons == x exactly on a tenth of the elements, |d| >= MARGIN elsewhere.
    far (log-cosh backward only): a third of the elements with 2 alpha d < -89, a third with > +89."""
    g = gen_of(case.id, 1)
    n = case.n
    v = torch.randn(n, generator=g)
    span = 3.0 if case.mode == "logcosh" else 1.0
    x = torch.rand(n, generator=g) * span
    if case.ract == ACT_TANH:
        r = torch.tanh(v)
    elif case.ract in (ACT_LRELU, ACT_RELU):
        v = torch.where(v.abs() < 0.15, v.sign() * 0.15, v)            # 0.15 * 0.01 >= MARGIN
        r = act_fwd64(v.double(), case.ract).float()
        r[torch.rand(n, generator=g) < 0.05] = 0.0
        if n >= 4:
            r[1] = 0.0
    else:
        r = torch.rand(n, generator=g) * span
    if case.mode == "l2l1":
        same = (torch.rand(n, generator=g) < 0.1) | ((r - x).abs() < MARGIN)
        if n >= 4:
            same[2] = True
        x = torch.where(same, r, x)
    if case.mode == "logcosh" and case.ract != ACT_NONE:
        r, x = r.clamp(-1.0, 2.0), x * (2.0 / 3.0)                      # d in (-3, 2]
    if far:
        which = torch.arange(n) % 3                                     # 2 alpha d < -100, > +100, and a few tenths
        big = 5.0 + 2.0 * torch.rand(n, generator=g)
        d = torch.where(which == 0, -big, torch.where(which == 1, big, 0.1 * torch.randn(n, generator=g)))
        x = r - d
    out = dict(r=r, x=x, mu=None, lv=None, heads=None, extra=None)
    B, L = case.B, case.L
    if case.layout != "none":
        mu = torch.randn(B, L, generator=g)
        lv = torch.rand(B, L, generator=g) * 6.0 - 4.0                  # log-variances in [-4, 2)
        if case.layout == "dense":
            heads = torch.cat([mu, lv], 0)                              # two dense blocks in one allocation
        elif case.layout == "halves":
            heads = torch.cat([mu, lv], 1).contiguous()
        else:
            heads = torch.full((B, 2 * L + 3), float("nan"))            # the three columns nobody may read
            heads[:, 1:1 + L], heads[:, L + 2:2 * L + 2] = mu, lv
        out["heads"] = heads
        out["mu"], out["lv"] = head_views(heads, case)
    if case.extra:
        out["extra"] = torch.randn(1, generator=g)
    return out


def recon_terms64(d, mode, alpha):
    """Per-element reconstruction term as recon_term<MODE> forms it (log-cosh WITHOUT the -log 2 and 1/alpha of the finish)."""
    if mode == "mse":
        return d * d
    if mode == "l2l1":
        return d * d + d.abs()
    return alpha * d + torch.log1p(torch.exp(-2.0 * alpha * d))


def loss_ref(inp, case, g_loss=1.0):
    """out4 = [loss, recon, kld, -kld] and d loss / d (recons's pre-activation, mu, logvar) * g_loss, float64, by autograd.
    log-cosh: recon = mean(alpha t + log(1 + exp(-2 alpha t)) - log 2) / alpha; l2 + l1: mse + l1."""
    alpha, M_N = f32s(alpha_of(case)), f32s(case.M_N)
    r = f64(inp["r"]).requires_grad_(True)
    d = r - f64(inp["x"])
    if case.mode == "logcosh":      # log(1 + e^y) as logaddexp(0, y): no overflow for the saturated inputs (softplus is linear from 20 on)
        y = -2.0 * alpha * d
        recon = (torch.logaddexp(torch.zeros_like(y), y) + alpha * d - np.log(2.0)).mean() / alpha
    else:
        recon = recon_terms64(d, case.mode, alpha).mean()
    leaves = [r]
    if inp["mu"] is not None:
        mu, lv = f64(inp["mu"]).requires_grad_(True), f64(inp["lv"]).requires_grad_(True)
        kld = torch.mean(-0.5 * torch.sum(1 + lv - mu ** 2 - lv.exp(), dim=1), dim=0)
        leaves += [mu, lv]
    else:
        kld = torch.zeros((), dtype=torch.float64)
    loss = recon + M_N * kld
    if inp["extra"] is not None:
        loss = loss + f64(inp["extra"])[0]
    grads = torch.autograd.grad(loss, leaves)
    g = float(np.float32(g_loss))
    ref = dict(out4=torch.stack([loss, recon, kld, -kld]).detach(), g_r=g * grads[0] * act_grad_from_out(r.detach(), case.ract))
    if len(leaves) == 3:
        ref.update(g_mu=g * grads[1], g_lv=g * grads[2])
    return ref


def fwd_blocks(n):
    return max(1, min(LOSS_BLOCKS, (n // 4 + 255) // 256))


def fwd_chain(n, terms=None):
    """c_chain of mse_partial_kernel: float32 additions a thread makes (4 per quad of its grid-stride loop, one more in the tail
    of block 0), then wave_sum_full (6) and the 4-way LDS merge (3).  The partials are added in double.  terms: the KL loop's
    count of elements instead (one addition each, same grid)."""
    nb = fwd_blocks(n)
    if terms is not None:
        return -(-terms // (nb * 256)) + 6 + 3
    return 4 * -(-(n // 4) // (nb * 256)) + (1 if n % 4 else 0) + 6 + 3


def loss_forward_bounds(inp, case, ref):
    """Bounds of out4.
      recon  terms t_i; d = r - x is one rounding (relative u on d).  MSE: d*d carries 2 u from d and 1 of the product: 3 u t.
             l2+l1: 3 u d^2 + 2 u |d| (d's rounding, the addition).  log-cosh, x = -2 alpha d (2 roundings: relative 2 u):
             alpha d: 2 u |alpha d|; e = expf(x): relative (1 + 2 |x|) u; 1 + e: u; logf: u |log| and the argument's relative
             error passes with weight e / (1 + e); the last addition u |t|:
                 err_i <= u (2 |alpha d| + (2 + 2 |x|) e / (1 + e) + log(1 + e) + |t|)
             sum: + c_chain u sum |t_i|.  The finish is double up to (float)(mean) (1), - 0.69314718f (1, and the constant's own
             rounding, 1), * (1 / alpha) (2): + 5 u (mean |t| + log 2) / alpha.
      kld    terms k_i = 1 + l - m^2 - e^l: four additions / products and expf, each at most u (1 + |l| + m^2 + e^l) / 2, expf u e^l:
             4 u (1 + |l| + m^2 + e^l) per element; + c_chain u sum of the same magnitudes; * 0.5 / B; + u |kld| for the cast.
      loss   recon + M_N * kld (+ extra): the two bounds, and 2 u (|recon| + |M_N kld| + |extra|) for a product and two sums."""
    alpha = f32s(alpha_of(case))
    d = f64(inp["r"]) - f64(inp["x"])
    n = case.n
    t = recon_terms64(d, case.mode, alpha)
    if case.mode == "mse":
        elem = 3.0 * t
    elif case.mode == "l2l1":
        elem = 3.0 * d * d + 2.0 * d.abs()
    else:
        x = -2.0 * alpha * d
        e = torch.exp(x)
        elem = 2.0 * (alpha * d).abs() + (2.0 + 2.0 * x.abs()) * e / (1.0 + e) + torch.log1p(e) + t.abs()
    tabs = (alpha * d).abs() + torch.log1p(torch.exp(-2.0 * alpha * d)) if case.mode == "logcosh" else t.abs()
    b_recon = EPS32 * (float(elem.sum()) + fwd_chain(n) * float(tabs.sum())) / n
    if case.mode == "logcosh":
        b_recon = b_recon / alpha + 5.0 * EPS32 * (float(tabs.sum()) / n + np.log(2.0)) / alpha
    else:
        b_recon += EPS32 * float(ref["out4"][1].abs())
    b_kld = 0.0
    if inp["mu"] is not None:
        mu, lv = f64(inp["mu"]), f64(inp["lv"])
        mag = float((1.0 + lv.abs() + mu * mu + lv.exp()).sum())
        b_kld = EPS32 * (4.0 + fwd_chain(n, case.B * case.L)) * mag * 0.5 / case.B + EPS32 * float(ref["out4"][2].abs())
    M_N = abs(f32s(case.M_N))
    ex = float(f64(inp["extra"]).abs()[0]) if inp["extra"] is not None else 0.0
    b_loss = b_recon + M_N * b_kld + 2.0 * EPS32 * (float(ref["out4"][1].abs()) + M_N * float(ref["out4"][2].abs()) + ex)
    return torch.tensor([b_loss, b_recon, b_kld, b_kld], dtype=torch.float64)


def loss_grad_bounds(inp, case, g_loss):
    """Bounds of g_r, g_mu, g_lv.  sc = g * scale, scale = (float)(1 / (n alpha)): 2 roundings.
      g_r  = sc * term'(d) * act'(r).  d: 1; the two products: 2; act': LRELU / RELU exact, TANH 1 - o*o with o^2 <= 1: absolute
             u, i.e. u |sc term'| on g_r.
             MSE 2 d: exact                                              -> u (5 |g_r| + tanh_part)
             l2+l1 2 d + sign: 1 more, of magnitude 2 |d| + 1             -> u (5 |sc| (2 |d| + 1) |act'| + tanh_part)
             log-cosh alpha (1 - e) / (1 + e), e = expf(x) relative (1 + 2 |x|) u, d / de = -2 / (1 + e)^2; 1 - e, 1 + e, the
             product and the quotient: 4                                  -> u (8 |g_r| + |sc act'| alpha 2 e (1 + 2 |x|) / (1 + e)^2
                                                                                + tanh_part)
             (in the saturated branches e is inf or 0 and the result is -alpha / +alpha up to the products)
      g_mu = (g * M_N / B) * mu: 3 roundings                              -> 3 u |g_mu|
      g_lv = ksc * 0.5 * (expf(l) - 1): expf's ulp is absolute u e^l and meets the cancellation at l = 0 -> u (|ksc| e^l / 2 + 4 |g_lv|)"""
    alpha, g = f32s(alpha_of(case)), float(np.float32(g_loss))
    r = f64(inp["r"])
    d = r - f64(inp["x"])
    n = case.n
    sc = abs(g) / (n * (alpha if alpha > 0 else 1.0))
    ap = act_grad_from_out(r, case.ract).abs()
    if case.mode == "mse":
        core, extra = 2.0 * d.abs(), 0.0
        c = 5.0
    elif case.mode == "l2l1":
        core, extra = (2.0 * d.abs() + 1.0) * (d != 0), 0.0
        c = 5.0
    else:
        x = -2.0 * alpha * d
        e = torch.exp(x.clamp(max=700.0))
        core = alpha * torch.tanh(alpha * d).abs()
        extra = sc * ap * alpha * 2.0 * e * (1.0 + 2.0 * x.abs()) / (1.0 + e) ** 2
        c = 8.0
    tanh_part = sc * core if case.ract == ACT_TANH else 0.0
    out = dict(g_r=EPS32 * (c * sc * core * ap + extra + tanh_part))
    if inp["mu"] is not None:
        mu, lv = f64(inp["mu"]), f64(inp["lv"])
        ksc = abs(g) * abs(f32s(case.M_N)) / case.B
        out["g_mu"] = EPS32 * 3.0 * ksc * mu.abs()
        out["g_lv"] = EPS32 * (ksc * lv.exp() * 0.5 + 4.0 * ksc * 0.5 * (lv.exp() - 1.0).abs())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# csrc/pointwise.hip: reparam_*, gauss_latent_*, act_*; csrc/gamma.hip: sigmoid_*
# ---------------------------------------------------------------------------------------------------------------------
REPARAM_SHAPES = [(1, 1), (7, 33), (3, 300)]                 # one thread; two blocks with a ragged end; four blocks


def reparam_inputs(B, L, strided):
    g = gen_of(f"reparam-{B}-{L}-{strided}", 2)
    W = 2 * L + 3 if strided else L
    mu_full, lv_full = torch.randn(B, W, generator=g), torch.rand(B, W, generator=g) * 10.0 - 6.0
    off = 1 if strided else 0
    return dict(mu=mu_full[:, off:off + L], lv=lv_full[:, 2 * off:2 * off + L], mu_full=mu_full, lv_full=lv_full,
                eps=torch.randn(B, L, generator=g), g_z=torch.randn(B, L, generator=g))


def reparam_ref(mu, lv, eps, g_z):
    """z = eps exp(lv / 2) + mu; g_mu = g_z (exactly); g_lv = g_z eps exp(lv / 2) / 2.
    Bounds: expf (1), product (1), sum (1): u (2 |eps s| + |z|); g_lv: expf and three products (0.5 is exact): 3 u |g_lv|."""
    mu, lv, eps, g_z = f64(mu), f64(lv), f64(eps), f64(g_z)
    s = torch.exp(0.5 * lv)
    z = eps * s + mu
    g_lv = g_z * eps * 0.5 * s
    return dict(z=z, g_mu=g_z, g_lv=g_lv), dict(z=EPS32 * (2.0 * (eps * s).abs() + z.abs()), g_lv=EPS32 * 3.0 * g_lv.abs())


LatentCase = namedtuple("LatentCase", "id B L S bias why")
LATENT_CASES = [
    LatentCase("B1-L4-noslices", 1, 4, 0, False, "one thread; heads read, not written"),
    LatentCase("B5-L12-S1", 5, 12, 1, False, "S = 1: seven of eight loads clamped"),
    LatentCase("B5-L12-S7-bias", 5, 12, 7, True, "S = 7: one clamped load; bias"),
    LatentCase("B64-L128-S8", 64, 128, 8, False, "S = 8: exactly one round, nothing clamped; eight blocks"),
    LatentCase("B64-L128-S9-bias", 64, 128, 9, True, "S = 9: a second round with seven clamped loads"),
    LatentCase("B3-L344-S16-bias", 3, 344, 16, True, "S = 16: two full rounds; L no multiple of 256, ragged last block"),
    LatentCase("B3-L344-noslices", 3, 344, 0, False, "rows that straddle blocks, no slices"),
]
LATENT_BWD = [           # (B, L, gz_slices, which of g_mu / g_lv / g_z are given)
    ("B1-L4-all", 1, 4, 0, (1, 1, 1)), ("B5-L12-no-gmu", 5, 12, 1, (0, 1, 1)), ("B5-L12-no-glv", 5, 12, 9, (1, 0, 1)),
    ("B64-L128-no-gz", 64, 128, 0, (1, 1, 0)), ("B64-L128-S9", 64, 128, 9, (1, 1, 1)), ("B3-L344-S1", 3, 344, 1, (1, 1, 1)),
]
RNG_POSITIONS = [0, 1, 2 ** 32 - 1, 2 ** 32]


def latent_inputs(case):
    """slices [S][B][2L] (None for S = 0), bias [2L] or None, heads [B][2L] (the float32 input when S = 0), eps [B][L]."""
    g = gen_of(case.id, 3)
    B, L, S = case.B, case.L, case.S
    eps = torch.randn(B, L, generator=g)
    heads = torch.cat([torch.randn(B, L, generator=g), torch.rand(B, L, generator=g) * 10.0 - 6.0], 1)
    if S == 0:
        return dict(slices=None, bias=None, heads=heads, eps=eps)
    sl = torch.randn(S, B, 2 * L, generator=g)
    sl[:, :, L:] = sl[:, :, L:] * 2.0 / S ** 0.5                       # log-variances of a few units whatever S
    bias = torch.randn(2 * L, generator=g) if case.bias else None
    return dict(slices=sl, bias=bias, heads=None, eps=eps)


def latent_heads_ref(inp):
    """heads = sum_s slices[s] + bias in float64; bound: a chain of S additions (the first onto 0 is exact) and the bias:
    (S + 1) u (sum |slices| + |bias|)."""
    sl = f64(inp["slices"])
    S = sl.shape[0]
    h, a = sl.sum(0), sl.abs().sum(0)
    if inp["bias"] is not None:
        h, a = h + f64(inp["bias"]), a + f64(inp["bias"]).abs()
    return h, EPS32 * (S + 1) * a


def latent_z_ref(heads, eps):
    """z from the heads the kernel itself wrote (or read): both sides see the same numbers.  Bound as reparam_ref."""
    L = heads.shape[1] // 2
    ref, bnd = reparam_ref(heads[:, :L], heads[:, L:], eps, eps)
    return ref["z"], bnd["z"]


def latent_bwd_inputs(cid, B, L, S, given):
    g = gen_of("latent-bwd-" + cid, 4)
    heads = torch.cat([torch.randn(B, L, generator=g), torch.rand(B, L, generator=g) * 10.0 - 6.0], 1)
    return dict(heads=heads, eps=torch.randn(B, L, generator=g), g_mu=torch.randn(B, L, generator=g) if given[0] else None,
                g_lv=torch.randn(B, L, generator=g) if given[1] else None,
                g_z=torch.randn(max(S, 1), B, L, generator=g) if given[2] else None)


def latent_bwd_ref(inp):
    """g_heads[:, :L] = g_mu + sum_s g_z[s];  g_heads[:, L:] = g_lv + (sum_s g_z[s]) eps exp(lv / 2) / 2.
    Bounds: the slice chain S (S - 1 roundings and one for the sum with g_mu): (S + 1) u (|g_mu| + sum |g_z|); second half: the
    chain, expf, three products and the sum: T = sum |g_z| |eps| s / 2, (S + 4) u T + u (|g_lv| + T)."""
    B, L2 = inp["heads"].shape
    L = L2 // 2
    zero = torch.zeros(B, L, dtype=torch.float64)
    gz = f64(inp["g_z"]).sum(0) if inp["g_z"] is not None else zero
    gza = f64(inp["g_z"]).abs().sum(0) if inp["g_z"] is not None else zero
    S = inp["g_z"].shape[0] if inp["g_z"] is not None else 1
    gm = f64(inp["g_mu"]) if inp["g_mu"] is not None else zero
    gl = f64(inp["g_lv"]) if inp["g_lv"] is not None else zero
    w = f64(inp["eps"]) * 0.5 * torch.exp(0.5 * f64(inp["heads"][:, L:]))
    T = gza * w.abs()
    ref = torch.cat([gm + gz, gl + gz * w], 1)
    bnd = torch.cat([EPS32 * (S + 1) * (gm.abs() + gza), EPS32 * ((S + 4) * T + gl.abs() + T)], 1)
    return ref, bnd


ACT_SIZES = [1, 255, 257, BWD_BLOCKS * 256 + 5]             # one thread; a ragged block; two blocks; the grid-stride loop wraps
SIGMOID_SIZES = [4, 1028, 4 * (BWD_BLOCKS * 256 + 3)]


def act_inputs(n, act):
    """Pre-activations with exact zeros planted and every other |value| >= MARGIN / LEAKY (so LRELU outputs stay >= MARGIN)."""
    g = gen_of(f"act-{n}-{act}", 5)
    v = torch.randn(n, generator=g) * 3.0
    v = torch.where(v.abs() < 0.15, v.sign() * 0.15, v)
    v[torch.rand(n, generator=g) < 0.05] = 0.0
    v[0] = 0.0 if n > 1 else v[0]
    return v, torch.randn(n, generator=g)


def act_ref(v, g_out, act):
    """out = act(v): NONE / RELU exact, LRELU one product (u |out|), TANH within TANH_ABS of tanh in float64.
    g_in = g_out * act'(out) from the float32 output the kernel wrote: LRELU / RELU / NONE one product (u |g_in|); TANH 1 - o*o
    (absolute u) and the product: u (|g_out| + |g_in|)."""
    out = act_fwd64(f64(v), act)
    b_out = torch.full_like(out, TANH_ABS) if act == ACT_TANH else (EPS32 * out.abs() if act == ACT_LRELU else torch.zeros_like(out))
    return out, b_out


def act_bwd_ref(out32, g_out, act):
    o, g = f64(out32), f64(g_out)
    gin = g * act_grad_from_out(o, act)
    bnd = EPS32 * (g.abs() + gin.abs()) if act == ACT_TANH else EPS32 * gin.abs()
    return gin, bnd


def sigmoid_inputs(n):
    g = gen_of(f"sigmoid-{n}", 6)
    x = torch.rand(n, generator=g) * 60.0 - 30.0
    return x, torch.randn(n, generator=g)


def sigmoid_ref(x, g_out):
    """y = 1 / (1 + __expf(-x)): the fast exponential is (2 + |x|) u relative; it enters y with weight e / (1 + e) <= 1; the sum
    and the quotient 2 more: u y ((2 + |x|) e / (1 + e) + 2).  Backward from the float32 y the kernel wrote: g y (1 - y): 1 - y is
    exact to u / 2 absolute (y <= 1), two products: u (|g y| + 2 |g_x|)."""
    x64 = f64(x)
    e = torch.exp(-x64)
    y = 1.0 / (1.0 + e)
    return y, EPS32 * y * ((2.0 + x64.abs()) * e / (1.0 + e) + 2.0)


def sigmoid_bwd_ref(y32, g_out):
    y, g = f64(y32), f64(g_out)
    gx = g * y * (1.0 - y)
    return gx, EPS32 * ((g * y).abs() + 2.0 * gx.abs())


# ---------------------------------------------------------------------------------------------------------------------
# csrc/ladder.hip
# ---------------------------------------------------------------------------------------------------------------------
LadderCase = namedtuple("LadderCase", "id B D why")
LADDER_CASES = [
    LadderCase("B1-D1", 1, 1, "one element: 255 idle lanes add zeros"),
    LadderCase("B9-D20", 9, 20, "the model test's shape"),
    LadderCase("B3-D255", 3, 255, "one short of a full row walk"),
    LadderCase("B3-D257", 3, 257, "a second step of the row walk for one lane"),
    LadderCase("B2-D600", 2, 600, "three steps, ragged"),
    LadderCase("B2049-D257", 2049, 257, "526 593 elements: the backward grid (2048 blocks) wraps"),
]
LADDER_GRADS = ("no-gz", "no-gkl", "both")
MERGE_EPS = float(np.float32(1e-7))


def ladder_inputs(case):
    """Means N(0, 1); log-variances uniform in [-6, 4]."""
    g = gen_of("ladder-" + case.id, 7)
    B, D = case.B, case.D
    u = lambda: torch.rand(B, D, generator=g) * 10.0 - 6.0          # noqa: E731
    return dict(mu_e=torch.randn(B, D, generator=g), lv_e=u(), mu_t=torch.randn(B, D, generator=g), lv_t=u(),
                eps=torch.randn(B, D, generator=g), g_z=torch.randn(B, D, generator=g), g_kl=torch.randn(B, generator=g))


def ladder_forward64(mu_e, lv_e, mu_t, lv_t, eps):
    """The header of ladder.hip: p1 = 1 / (e^lv_e + 1e-7), p2 = 1 / (e^lv_t + 1e-7), P = p1 + p2, mu = (mu_e p1 + mu_t p2) / P,
    lv = log(1 / P), z = eps e^(lv / 2) + mu, kl[b] = sum_d (lv_e - lv) + (e^lv + (mu - mu_e)^2) / (2 e^lv_e) - 0.5."""
    p1, p2 = 1.0 / (lv_e.exp() + MERGE_EPS), 1.0 / (lv_t.exp() + MERGE_EPS)
    P = p1 + p2
    mu, lv = (mu_e * p1 + mu_t * p2) / P, torch.log(1.0 / P)
    z = eps * torch.exp(0.5 * lv) + mu
    kl = ((lv_e - lv) + (lv.exp() + (mu - mu_e) ** 2) / (2.0 * lv_e.exp()) - 0.5).sum(-1)
    return z, kl


def ladder_chain(D):
    """ladder_fwd_kernel: a lane adds ceil(D / 256) terms, wave_sum 6, the LDS merge 2 deep."""
    return -(-D // 256) + 6 + 2


def ladder_ref(inp, grads="both"):
    """(z, kl, the four gradients) in float64; gradients by autograd of sum(z g_z) + sum(kl g_kl) with the absent one left out."""
    t = [f64(inp[k]).requires_grad_(True) for k in ("mu_e", "lv_e", "mu_t", "lv_t")]
    z, kl = ladder_forward64(*t, f64(inp["eps"]))
    obj = 0.0
    if grads != "no-gz":
        obj = obj + (z * f64(inp["g_z"])).sum()
    if grads != "no-gkl":
        obj = obj + (kl * f64(inp["g_kl"])).sum()
    gs = torch.autograd.grad(obj, t)
    return dict(z=z.detach(), kl=kl.detach(), g_mu_e=gs[0], g_lv_e=gs[1], g_mu_t=gs[2], g_lv_t=gs[3])


def ladder_bounds(inp, grads="both"):
    """Forward.  E = expf(lv_e) (1), + 1e-7 (1), 1 / . (1): p1, p2 relative 3 u; P = p1 + p2 (positive summands): 4 u.
      mu   = (mu_e p1 + mu_t p2) / P: numerator 3 + 1 + 1, the quotient 1, P 4: 10 u M, M = (|mu_e| p1 + |mu_t| p2) / P >= |mu|
      lv   = logf(1 / P): argument relative 5 u -> absolute 5 u; logf's ulp u |lv|:  u (5 + |lv|)
      z    = eps expf(lv / 2) + mu: the exponential is relative (dlv / 2 + 1) u, product 1, sum 1:
             |eps| s (dlv / (2 u) + 2) u + dmu + u |z|
      kl   term = (lv_e - lv) + (e^lv + dl^2) / (2 E) - 0.5 with dl = mu - mu_e carrying dmu ABSOLUTE (mu - mu_e cancels where
             p2 << p1): per element
                 dlv + [e^lv (dlv + u) + 2 |dl| (dmu + u |dl|) + u dl^2] / (2 E) + 3 u (e^lv + dl^2) / (2 E) + 2 u (parts)
             with parts = |lv_e - lv| + (e^lv + dl^2) / (2 E) + 0.5; the row sum adds ladder_chain(D) u sum parts.
    Backward: ladder_backward_bounds."""
    mu_e, lv_e, mu_t, lv_t, eps = (f64(inp[k]) for k in ("mu_e", "lv_e", "mu_t", "lv_t", "eps"))
    E, T = lv_e.exp(), lv_t.exp()
    p1, p2 = 1.0 / (E + MERGE_EPS), 1.0 / (T + MERGE_EPS)
    P = p1 + p2
    mu, lv = (mu_e * p1 + mu_t * p2) / P, torch.log(1.0 / P)
    M = (mu_e.abs() * p1 + mu_t.abs() * p2) / P
    dmu = 10.0 * EPS32 * M
    dlv = EPS32 * (5.0 + lv.abs())
    s = torch.exp(0.5 * lv)
    z = eps * s + mu
    b_z = eps.abs() * s * (0.5 * dlv + 2.0 * EPS32) + dmu + EPS32 * z.abs()
    dl = (mu - mu_e).abs()
    q = (lv.exp() + dl * dl) / (2.0 * E)
    parts = (lv_e - lv).abs() + q + 0.5
    elem = dlv + (lv.exp() * (dlv + EPS32) + 2.0 * dl * (dmu + EPS32 * dl) + EPS32 * dl * dl) / (2.0 * E) + 3.0 * EPS32 * q + 2.0 * EPS32 * parts
    b_kl = elem.sum(-1) + ladder_chain(mu_e.shape[1]) * EPS32 * parts.sum(-1)
    out = dict(z=b_z, kl=b_kl)
    out.update(ladder_backward_bounds(inp, grads))
    return out


LADDER_OUT = ("g_mu_e", "g_lv_e", "g_mu_t", "g_lv_t")


def ladder_bwd_form(gz, gk, eps, dl, dt, E, T, p1, p2, P, magnitudes=False):
    """The closed forms of ladder_bwd_kernel, operation by operation, in the dtype of the arguments; dl = mu - mu_e, dt = mu_t - mu
    (the kernel's mu_e - mu is -dl exactly).  magnitudes: every summand and factor replaced by its magnitude (arguments >= 0)."""
    n = 1.0 if magnitudes else -1.0
    x = gk * dl / E
    Gmu = gz + x
    GP = gz * (n * 0.5 * eps / (P * torch.sqrt(P))) + gk * (1.0 / P + n * 1.0 / (2.0 * E * P * P))
    Gp1, Gp2 = Gmu * (n * dl) / P + GP, Gmu * dt / P + GP
    return (Gmu * p1 / P + n * x, Gp1 * (n * E * p1 * p1) + gk * (1.0 + n * (1.0 / P + dl * dl) / (2.0 * E)),
            Gmu * p2 / P, Gp2 * (n * T * p2 * p2))


def ladder_leaves(inp, dtype):
    """What the kernel computes before its closed forms, the way it computes it, in `dtype`: (eps, dl, dt, E, T, p1, p2, P), M."""
    mu_e, lv_e, mu_t, lv_t, eps = (inp[k].to(dtype) for k in ("mu_e", "lv_e", "mu_t", "lv_t", "eps"))
    E, T = lv_e.exp(), lv_t.exp()
    me = torch.tensor(MERGE_EPS, dtype=dtype)
    p1, p2 = 1.0 / (E + me), 1.0 / (T + me)
    P = p1 + p2
    mu = (mu_e * p1 + mu_t * p2) / P
    return (eps, mu - mu_e, mu_t - mu, E, T, p1, p2, P), (mu_e.abs() * p1 + mu_t.abs() * p2) / P


def ladder_backward_bounds(inp, grads="both"):
    """A running error analysis of ladder_bwd_kernel, first order.  Roundings are counted at the unit roundoff u / 2, a function's
    ulp at u.  The kernel first forms the leaves E, T (expf: u), p1, p2 (a sum and a quotient more: 2 u), P (2.5 u) and
        mu = (mu_e p1 + mu_t p2) / P:  five roundings at the size of M = (|mu_e| p1 + |mu_t| p2) / P, and the errors of p1, p2 with
             their sensitivities (mu_e - mu) p1 / P and (mu_t - mu) p2 / P, both |dl| p1 / P:   dmu = u (2.5 M + 4 |dl|)
        dl = mu - mu_e, dt = mu_t - mu:  dmu + u / 2 |dl| resp. |dt| -- ABSOLUTE errors: where p2 << p1 the difference cancels.
    Each output is then a rational function f of the leaves and the upstream gradients.  Its error is at most
        sum over leaves v of |df / dv| |error of v|        (autograd of the closed form in float64: a leaf's error reaches the
                                                            output with its true, signed sensitivity -- in g_mu_e = Gmu p1 / P -
                                                            g_kl dl / E the error of dl enters both terms and all but p2 / P of it
                                                            cancels)
      + 8 u A                                              (at most 16 roundings on the longest path behind the leaves, each at the
                                                            size of A: the closed form with every summand and factor replaced by
                                                            its magnitude, at the true |dl|, |dt| plus their errors)"""
    leaves64, M = ladder_leaves(inp, torch.float64)
    eps, dl, dt, E, T, p1, p2, P = leaves64
    zero = torch.zeros_like(dl)
    gz = f64(inp["g_z"]) if grads != "no-gz" else zero
    gk = f64(inp["g_kl"])[:, None].expand_as(dl) if grads != "no-gkl" else zero
    dmu = EPS32 * (2.5 * M + 4.0 * dl.abs())
    errs = dict(dl=dmu + 0.5 * EPS32 * dl.abs(), dt=dmu + 0.5 * EPS32 * dt.abs(), E=EPS32 * E, T=EPS32 * T, p1=2.0 * EPS32 * p1,
                p2=2.0 * EPS32 * p2, P=2.5 * EPS32 * P)
    names = ("dl", "dt", "E", "T", "p1", "p2", "P")
    var = [t.clone().requires_grad_(True) for t in (dl, dt, E, T, p1, p2, P)]
    outs = ladder_bwd_form(gz, gk, eps, *var)
    A = ladder_bwd_form(gz.abs(), gk.abs(), eps.abs(), dl.abs() + errs["dl"], dt.abs() + errs["dt"], E, T, p1, p2, P, magnitudes=True)
    res = {}
    for k, o, a in zip(LADDER_OUT, outs, A):
        gs = torch.autograd.grad(o.sum(), var, retain_graph=True, allow_unused=True)
        res[k] = (8.0 * EPS32 * a + sum(g.abs() * errs[nm] for nm, g in zip(names, gs) if g is not None)).detach()
    return res


# ---------------------------------------------------------------------------------------------------------------------
# csrc/tcvae.hip
# ---------------------------------------------------------------------------------------------------------------------
TC_MAX_D, TC_MAX_B = 32, 4096
LOG2PI = float(np.float32(1.8378770664093453))               # kLog2Pi as the kernel holds it
TCCase = namedtuple("TCCase", "id B D underflow why")
TC_CASES = ([TCCase(f"B8-D{D}", 8, D, False, "tc_*_kernel<16>" if D <= 16 else "tc_*_kernel<32>") for D in (1, 10, 16, 17, 32)]
            + [TCCase(f"B257-D{D}", 257, D, False, "a second step of the j walk; " + ("<16>" if D <= 16 else "<32>")) for D in (1, 16, 17, 32)]
            + [TCCase(f"B{B}-D10", B, 10, False, why) for B, why in ((2, "the smallest batch"), (255, "one short of the block"),
                                                                     (256, "exactly one step"), (257, "a second step for lane 0"),
                                                                     (600, "three steps, ragged"))]
            + [TCCase("B8-D10-underflow", 8, 10, True, "log_iw = -1e4 in three columns: components leave the logsumexp"),
               TCCase("B257-D17-underflow", 257, 17, True, "the same over two steps, <32>")])
TC_G3 = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.5, 6.0, 0.3)]
TC_DEAD = (1, 3, 6)                                          # the columns of the underflow cases (never the diagonal's only support)


def tc_log_iw(B):
    """BetaTCVAE._log_importance_weights for a dataset of 10 B samples (betatc_vae.py:128-140, as O.betatc_loss restates it)."""
    N = 10 * B
    strat = (N - B + 1) / (N * (B - 1))
    iw = torch.full((B, B), 1 / (B - 1))
    iw.view(-1)[::B] = 1 / N
    iw.view(-1)[1::B] = strat
    iw[B - 2, 0] = strat
    return iw.log()


def tc_inputs(case):
    g = gen_of("tc-" + case.id, 8)
    B, D = case.B, case.D
    mu, lv = torch.randn(B, D, generator=g), torch.rand(B, D, generator=g) * 3.0 - 2.0
    z = mu + torch.randn(B, D, generator=g) * torch.exp(0.5 * lv)
    liw = tc_log_iw(B)
    if case.underflow:
        liw[:, list(TC_DEAD)] = -1e4
    return dict(z=z, mu=mu, lv=lv, liw=liw)


def _logn(v, m, l):
    return -0.5 * (LOG2PI + l) - 0.5 * (v - m) ** 2 * torch.exp(-l)


def tc_forward64(z, mu, lv, liw, keep=None):
    """out3 = (mi, tc, kld), lse_s [B], lse_d [B][D] as the header of tcvae.hip defines them.  keep: the columns j that take part
    (the underflow cases' self-check: dropping the dead columns changes nothing)."""
    B, D = z.shape
    M = _logn(z.view(B, 1, D), mu.view(1, B, D), lv.view(1, B, D)) + liw.view(B, B, 1)
    if keep is not None:
        M = M[:, keep]
    lse_s, lse_d = torch.logsumexp(M.sum(2), dim=1), torch.logsumexp(M, dim=1)
    qzx, pz, prod = _logn(z, mu, lv).sum(1), _logn(z, torch.zeros_like(z), torch.zeros_like(z)).sum(1), lse_d.sum(1)
    return torch.stack([(qzx - lse_s).mean(), (lse_s - prod).mean(), (prod - pz).mean()]), lse_s, lse_d


def tc_ref(inp, g3=None):
    t = [f64(inp[k]).requires_grad_(g3 is not None) for k in ("z", "mu", "lv")]
    out3, lse_s, lse_d = tc_forward64(*t, f64(inp["liw"]))
    ref = dict(out3=out3.detach(), lse_s=lse_s.detach(), lse_d=lse_d.detach())
    if g3 is not None:
        gs = torch.autograd.grad((out3 * torch.tensor([float(np.float32(v)) for v in g3], dtype=torch.float64)).sum(), t)
        ref.update(g_z=gs[0], g_mu=gs[1], g_lv=gs[2])
    return ref


def tc_chain(B):
    """Merges (forward) or additions (backward) a value passes: ceil(B / 256) in a thread, 6 shuffles, 3 through LDS."""
    return -(-B // 256) + 6 + 3


def _tc_parts(inp):
    """The [B][B][D] tensors every bound below is made of.
    v = -0.5 (log2pi + l_j) - 0.5 dl^2 __expf(-l_j) + w: dl one rounding (2 u on dl^2), __expf(-l) (2 + |l|) u, three products, the
    sum log2pi + l and the constant's own rounding 2 u, two more sums:  eps_v = u (9 + |l_j|) V,  V = 0.5 (log2pi + |l_j|) +
    0.5 dl^2 e^-l + |w|.  s = sum_d v: eps_s = sum_d eps_v + D u sum_d |v|."""
    z, mu, lv, liw = (f64(inp[k]) for k in ("z", "mu", "lv", "liw"))
    B, D = z.shape
    l = lv.view(1, B, D)
    dl = z.view(B, 1, D) - mu.view(1, B, D)
    el = torch.exp(-l)
    q = 0.5 * dl * dl * el
    w = liw.view(B, B, 1)
    v = -0.5 * (LOG2PI + l) - q + w
    V = 0.5 * (LOG2PI + l.abs()) + q + w.abs()
    ev = EPS32 * (9.0 + l.abs()) * V
    s = v.sum(2)
    es = ev.sum(2) + D * EPS32 * v.abs().sum(2)
    return dict(z=z, mu=mu, lv=lv, B=B, D=D, l=l, dl=dl, el=el, q=q, v=v, V=V, ev=ev, s=s, es=es)


def _lse_bound(x, ex, chain):
    """Bound of r = mm + __logf(ll) for the running (max, sum) logsumexp over dim 1 of x with input errors ex.
    Every merge forms l __expf(m - mm) + l2 __expf(m2 - mm): per merge and element a fast exponential (2 u + |its argument| u), a
    product and a sum: 4 u and the argument.  The maximum only grows along an element's path, so its arguments telescope to
    x_j - mm: element j ends with the relative error u (4 chain + mm - x_j) + ex_j, weighted by its share p_j of the sum.
    __logf: 2 u max(1, |log ll|) absolute; mm + .: u |r|."""
    lse = torch.logsumexp(x, dim=1, keepdim=True)
    mm = x.max(dim=1, keepdim=True)[0]
    p = torch.exp(x - lse)
    gap = torch.where(p > 0, mm - x, torch.zeros_like(x))               # 0 * 1e4, not nan, for the components that left the sum
    ll = (lse - mm).abs()
    b = (p * (EPS32 * (4.0 * chain + gap) + ex)).sum(1, keepdim=True) + 2.0 * EPS32 * ll.clamp(min=1.0) + EPS32 * lse.abs()
    return b.squeeze(1), p, lse.squeeze(1)


def tc_forward_bounds(inp):
    """lse_d, lse_s: _lse_bound.  The row scalars are float32 sums of D terms (thread 0): qzx = sum_d v(i, i, d) without w, prod =
    sum_d lse_d, pz = sum_d -0.5 log2pi - 0.5 z^2 (3 u each): D u sum |terms| on top of the terms' own bounds.  tc_finish_kernel
    averages in double and rounds each difference once: out3 = the mean of the two rows' bounds + u |out3|."""
    P = _tc_parts(inp)
    B, D, c = P["B"], P["D"], tc_chain(P["B"])
    b_d, _, lse_d = _lse_bound(P["v"], P["ev"], c)
    b_s, _, lse_s = _lse_bound(P["s"], P["es"], c)
    i = torch.arange(B)
    w = f64(inp["liw"]).view(B, B, 1)
    vii = (P["v"] - w)[i, i]
    b_qzx = (EPS32 * (9.0 + P["lv"].abs()) * (P["V"] - w.abs())[i, i]).sum(1) + D * EPS32 * vii.abs().sum(1)
    b_prod = b_d.sum(1) + D * EPS32 * lse_d.abs().sum(1)
    pzt = 0.5 * LOG2PI + 0.5 * P["z"] ** 2
    b_pz = (3.0 + D) * EPS32 * pzt.sum(1)
    out3 = tc_forward64(P["z"], P["mu"], P["lv"], f64(inp["liw"]))[0]
    b3 = torch.stack([(b_qzx + b_s).mean(), (b_s + b_prod).mean(), (b_prod + b_pz).mean()]) + EPS32 * out3.abs()
    return dict(out3=b3, lse_s=b_s, lse_d=b_d)


def tc_backward_bounds(inp, g3, lse_err=None):
    """The kernel is handed lse_s / lse_d rounded to float32 (error u |lse|; lse_err = (bound [B], bound [B][D]): the forward
    kernel's own outputs instead, with their forward bounds) and recomputes v and s.
      S = __expf(s - lse_s): relative  rho_s = eps_s + u |lse_s| + u (3 + 2 |s - lse_s|)     (argument: the subtraction's rounding and
      P = __expf(v - lse_d): relative  rho_d = eps_v + u |lse_d| + u (3 + 2 |v - lse_d|)      its propagation; the exponential itself)
      cs = (-g0 + g1) / B, cp = (-g1 + g2) / B, ca, cz: 3 u each
      wd = cs S + cp P: |cs| S (rho_s + 5 u) + |cp| P (rho_d + 6 u)
      f  = dl el (d z, d mu): (4 + |l|) u;   -0.5 + 0.5 dl^2 el (d lv): (6 + |l|) u on the second summand and u on the sum
      terms wd f are added over the other index: (tc_chain + 2) u sum |wd f|, the two sums with the direct terms included;
      direct terms ca f(i, i), cz z: their factor's roundings and 3 u."""
    P = _tc_parts(inp)
    B, D, c = P["B"], P["D"], tc_chain(P["B"]) + 2
    g = [float(np.float32(v)) for v in g3]
    ca, cs, cp, cz = abs(g[0]) / B, abs(-g[0] + g[1]) / B, abs(-g[1] + g[2]) / B, abs(g[2]) / B
    lse_s, lse_d = torch.logsumexp(P["s"], 1), torch.logsumexp(P["v"], 1)          # [B], [B][D]
    xs, xd = P["s"] - lse_s.view(B, 1), P["v"] - lse_d.view(B, 1, D)
    S, Pd = torch.exp(xs), torch.exp(xd)
    el_s, el_d = (EPS32 * lse_s.abs(), EPS32 * lse_d.abs()) if lse_err is None else lse_err
    rho_s = P["es"] + el_s.view(B, 1) + EPS32 * (3.0 + 2.0 * xs.abs())
    rho_d = P["ev"] + el_d.view(B, 1, D) + EPS32 * (3.0 + 2.0 * xd.abs())
    rho_s, rho_d = torch.where(S > 0, rho_s, torch.zeros_like(S)), torch.where(Pd > 0, rho_d, torch.zeros_like(Pd))
    wd = cs * S.view(B, B, 1) + cp * Pd
    ewd = cs * (S * (rho_s + 5.0 * EPS32)).view(B, B, 1) + cp * Pd * (rho_d + 6.0 * EPS32)
    l, dl, el, q = P["l"], P["dl"], P["el"], P["q"]
    f1 = (dl * el).abs()
    t1 = ewd * f1 + wd * f1 * (4.0 + l.abs()) * EPS32 + c * EPS32 * wd * f1
    f2 = 0.5 + q
    t2 = ewd * f2 + wd * (q * (6.0 + l.abs()) + f2) * EPS32 + c * EPS32 * wd * f2
    i = torch.arange(B)
    d1, d2, li = f1[i, i], f2[i, i], P["lv"].abs()
    dir1 = ca * d1 * (7.0 + li + c) * EPS32
    return dict(g_z=t1.sum(1) + dir1 + cz * P["z"].abs() * (3.0 + c) * EPS32, g_mu=t1.sum(0) + dir1,
                g_lv=t2.sum(0) + ca * (q[i, i] * (9.0 + li) + d2 * (1.0 + c)) * EPS32)


# ---------------------------------------------------------------------------------------------------------------------
# csrc/vamp.hip
# ---------------------------------------------------------------------------------------------------------------------
VAMP_MAX_K = 512
FLT_MIN = 2.0 ** -126
VampCase = namedtuple("VampCase", "id B D K far why")
VAMP_CASES = ([VampCase(f"K{K}-D65-B{B}", B, 65, K, False, why) for K, B, why in (
                  (1, 1, "one component: weight 1, lse = s"), (3, 7, "fewer components than waves"), (4, 7, "one per wave"),
                  (5, 7, "a second round for wave 0"), (255, 7, "one short of one per thread"), (256, 7, "one per thread"),
                  (257, 1, "two per thread for thread 0"), (512, 7, "the limit: two per thread"))]
              + [VampCase(f"K5-D{D}-B{B}", B, D, 5, False, why) for D, B, why in (
                  (1, 7, "63 idle lanes"), (63, 7, "one short of a wave"), (64, 1, "exactly one step per lane"),
                  (200, 7, "four steps, ragged; D < 256: idle threads in the q sum"))]
              + [VampCase("K5-D65-B7-far", 7, 65, 5, True, "pseudo-inputs 30 apart: one weight rounds to 1, the rest underflow")])


def vamp_inputs(case):
    g = gen_of("vamp-" + case.id, 9)
    B, D, K = case.B, case.D, case.K
    # means of half a unit and log-variances in [-0.5, 0.5): |s| stays near 100 at D = 200, and with it the error of a weight
    mu, lv = 0.5 * torch.randn(B, D, generator=g), torch.rand(B, D, generator=g) - 0.5
    z = mu + torch.randn(B, D, generator=g) * torch.exp(0.5 * lv)
    pmu, plv = 0.5 * torch.randn(K, D, generator=g), torch.rand(K, D, generator=g) - 0.5
    if case.far:
        pmu = pmu * 0.1 + 30.0 * torch.arange(K, dtype=torch.float32).view(K, 1)
        z = z * 0.1 + 30.0 * (torch.arange(B) % K).float().view(B, 1)
    return dict(z=z, mu=mu, lv=lv, pmu=pmu, plv=plv)


def vamp_forward64(z, mu, lv, pmu, plv, keep=None):
    """(out3 = [kld, E_log_p, E_log_q], weights [B][K]) as the header of vamp.hip defines them.  keep [B]: only component
    keep[b] takes part in sample b's logsumexp (the far case's self-check); log K stays."""
    K = pmu.shape[0]
    q = (-0.5 * (lv + (z - mu) ** 2) / lv.exp()).sum(1)
    s = (-0.5 * (plv.unsqueeze(0) + (z.unsqueeze(1) - pmu.unsqueeze(0)) ** 2) / plv.unsqueeze(0).exp()).sum(2) - np.log(K)
    if keep is not None:
        s = s.gather(1, keep.view(-1, 1))
    lse = torch.logsumexp(s, dim=1)
    ep, eq = lse.mean(), q.mean()
    return torch.stack([-(ep - eq), ep, eq]), torch.softmax(s, dim=1)


def vamp_ref(inp, g=None):
    names = ("z", "mu", "lv", "pmu", "plv")
    t = [f64(inp[k]).requires_grad_(g is not None) for k in names]
    out3, w = vamp_forward64(*t)
    ref = dict(out3=out3.detach(), w=w.detach())
    if g is not None:
        gs = torch.autograd.grad(out3[0] * float(np.float32(g)), t)
        ref.update({"g_" + k: v for k, v in zip(names, gs)})
    return ref


def vamp_bounds(inp, g=1.0, own_weights=False):
    """Forward.  t = -0.5 (l + dl^2) __expf(-l): dl 1 (dl^2: 3), the sum 1, __expf 2 + |l|, the product 1:  eps_t = u (7 + |l|) T with
    T = 0.5 (|l| + dl^2) e^-l.  s_k: a lane adds ceil(D / 64) terms, 6 shuffles; - log K (one rounding; __logf(K) itself 2 u
    max(1, log K)):  eps_s = sum_d eps_t + (ceil(D / 64) + 6) u sum_d |t| + u |s| + 2 u max(1, log K).
    e_k = __expf(s_k - m): relative rho_k = eps_s + u (3 + 2 |s_k - m|); tot: ceil(K / 256) + 6 + 2 additions: rho_tot = sum_k p_k rho_k +
    c_e u.  lse = m + __logf(tot): rho_tot + 2 u max(1, |log tot|) + u |lse|.  w_k = e_k / tot: w_k (rho_k + rho_tot + u) + 2^-126.
    q: as s with ceil(D / 256) + 6 + 2 additions.  The finish is double: means of the row bounds + u |out|.
    Backward, from weights rounded to float32 (u w; own_weights: from the forward kernel's weights instead -- every term that
    carries a weight w_k then also carries its forward bound b_w in w's place):
      d mu = gq dl el: (6 + |l|) u |d mu|;  d lv = gq (-0.5 el (1 - l - dl^2)): (10 + |l|) u |gq| 0.5 el (1 + |l| + dl^2)
      d z  = gz + gp sum_k w_k (-pd_k e^-pl_k): K sequential additions: |gp| sum_k |term_k| (6 + |pl_k| + K) u + (6 + |l|) u |gz|
             + 2 u (|gz| + |gp| sum |term|)
      d pmu = gp el sum_b w pd: (B + 9 + |pl|) u |gp| el sum_b |w pd|
      d plv = gp (-0.5) el sum_b w (1 - pl - pd^2): (B + 10 + |pl|) u |gp| 0.5 el sum_b w (1 + |pl| + pd^2)"""
    z, mu, lv, pmu, plv = (f64(inp[k]) for k in ("z", "mu", "lv", "pmu", "plv"))
    B, D = z.shape
    K = pmu.shape[0]
    u = EPS32
    pl = plv.unsqueeze(0)
    pd = z.unsqueeze(1) - pmu.unsqueeze(0)
    epl = torch.exp(-pl)
    t = -0.5 * (pl + pd * pd) * epl
    T = 0.5 * (pl.abs() + pd * pd) * epl
    logK = float(np.log(K))
    s = t.sum(2) - logK
    es = (u * (7.0 + pl.abs()) * T).sum(2) + (-(-D // 64) + 6) * u * T.sum(2) + u * s.abs() + 2.0 * u * max(1.0, logK)
    m = s.max(1, keepdim=True)[0]
    lse = torch.logsumexp(s, 1, keepdim=True)
    p = torch.exp(s - lse)
    rho = torch.where(p > 0, es + u * (3.0 + 2.0 * (s - m).abs()), torch.zeros_like(s))
    rho_tot = (p * rho).sum(1, keepdim=True) + (-(-K // 256) + 8) * u
    b_lse = (rho_tot + 2.0 * u * (lse - m).abs().clamp(min=1.0) + u * lse.abs()).squeeze(1)
    b_w = p * (rho + rho_tot + u) + FLT_MIN                             # a weight below the float32 range is flushed to 0
    dl = z - mu
    el = torch.exp(-lv)
    tq, Tq = -0.5 * (lv + dl * dl) * el, 0.5 * (lv.abs() + dl * dl) * el
    b_q = (u * (7.0 + lv.abs()) * Tq).sum(1) + (-(-D // 256) + 8) * u * Tq.sum(1)
    ep, eq = float(lse.mean()), float(tq.sum(1).mean())
    b_ep, b_eq = float(b_lse.mean()) + u * abs(ep), float(b_q.mean()) + u * abs(eq)
    out = dict(out3=torch.tensor([b_ep + b_eq + u * abs(ep - eq), b_ep, b_eq], dtype=torch.float64), w=b_w)
    gq = abs(float(np.float32(g))) / B
    gz = gq * (dl * el).abs()
    term = p.unsqueeze(2) * (pd * epl).abs()                              # [B][K][D]
    st = term.sum(1)
    out["g_mu"] = (6.0 + lv.abs()) * u * gz
    out["g_lv"] = (10.0 + lv.abs()) * u * gq * 0.5 * el * (1.0 + lv.abs() + dl * dl)
    out["g_z"] = gq * (term * (6.0 + pl.abs() + K)).sum(1) * u + (6.0 + lv.abs()) * u * gz + 2.0 * u * (gz + gq * st)
    e0, l0 = torch.exp(-plv), plv.abs()
    out["g_pmu"] = (B + 9.0 + l0) * u * gq * e0 * (p.unsqueeze(2) * pd.abs()).sum(0)
    out["g_plv"] = (B + 10.0 + l0) * u * gq * 0.5 * e0 * (p.unsqueeze(2) * (1.0 + pl.abs() + pd * pd)).sum(0)
    if own_weights:
        out["g_z"] = out["g_z"] + gq * (b_w.unsqueeze(2) * (pd * epl).abs()).sum(1)
        out["g_pmu"] = out["g_pmu"] + gq * e0 * (b_w.unsqueeze(2) * pd.abs()).sum(0)
        out["g_plv"] = out["g_plv"] + gq * 0.5 * e0 * (b_w.unsqueeze(2) * (1.0 + pl.abs() + pd * pd)).sum(0)
    # the float32 range: a weight, a product or a result below 2^-126 is flushed to 0 -- an absolute 2^-126 on every weight and
    # every product of a sum, and on the result (components far from every sample: K = 257 at B = 1 has weights of 1e-40)
    out["g_z"] = out["g_z"] + FLT_MIN * (gq * ((pd * epl).abs() + 1.0).sum(1) + 1.0)
    out["g_pmu"] = out["g_pmu"] + FLT_MIN * (gq * e0 * (pd.abs() + 1.0).sum(0) + 1.0)
    out["g_plv"] = out["g_plv"] + FLT_MIN * (gq * 0.5 * e0 * (2.0 + pl.abs() + pd * pd).sum(0) + 1.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# csrc/swd.hip
# ---------------------------------------------------------------------------------------------------------------------
SWD_MAX_N = 1024
SWD_WEIGHT = 0.7
# exact cases: z, prior entries are integers in [-8192, 8192) / 4096, proj entries odd integers in [-63, 63] / 64 (no unit
# directions needed): every projection and every partial sum of one is a multiple of 2^-18 below 2^4 -- exact in float32 in any
# order -- so ranks are no matter of rounding and the gradient is compared element by element.  `seed` is the salt offset of the
# case's crc seed (gen_of("swd-" + id, 10 + seed)): the first one, searched on the CPU, without two equal projections on any
# direction; at N = 1024 only z's side can be kept tie-free (ties among
# the prior's projections are equal values and carry no gradient).
SwdCase = namedtuple("SwdCase", "id N D S p exact seed why")
SWD_CASES = [
    SwdCase("exact-N1", 1, 8, 7, 2.0, True, 0, "P = 2: one padded slot"),
    SwdCase("exact-N2", 2, 8, 7, 3.0, True, 0, "no padding, the smallest network; powf with negative bases"),
    SwdCase("exact-N3", 3, 8, 7, 4.0, True, 0, "P = 4: one padded slot"),
    SwdCase("exact-N37", 37, 8, 7, 2.0, True, 0, "P = 64: 27 padded slots"),
    SwdCase("exact-N256", 256, 8, 7, 3.0, True, 0, "one element per thread, no padding"),
    SwdCase("exact-N257", 257, 8, 7, 2.0, True, 3, "P = 512: a second element for thread 0, 255 padded slots"),
    SwdCase("exact-N1000", 1000, 4, 3, 4.0, True, 5, "P = 1024 with padding"),
    SwdCase("exact-N1024-S1", 1024, 4, 1, 2.0, True, 0, "the limit, no padding, one direction"),
    SwdCase("exact-N1024-S2", 1024, 4, 2, 3.0, True, 3, "the limit, two directions"),
    SwdCase("normal-N37-D128-S50", 37, 128, 50, 2.0, False, 0, "the model's shape"),
    SwdCase("normal-N257-D512-S1", 257, 512, 1, 4.0, False, 0, "D at its limit: the whole direction buffer"),
    SwdCase("normal-N1000-D128-S50", 1000, 128, 50, 3.0, False, 0, "many directions at a padded N"),
]


def swd_inputs(case):
    g = gen_of("swd-" + case.id, 10 + case.seed)
    N, D, S = case.N, case.D, case.S
    if case.exact:
        z = torch.randint(-8192, 8192, (N, D), generator=g).float() / 4096
        prior = torch.randint(-8192, 8192, (N, D), generator=g).float() / 4096
        proj = (2 * torch.randint(-32, 32, (S, D), generator=g) + 1).float() / 64
    else:
        z, prior = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g)
        r = torch.randn(S, D, generator=g)
        proj = r / r.norm(dim=1).view(-1, 1)
    return dict(z=z, prior=prior, proj=proj)


def swd_ties(a):
    """Pairs of equal neighbours among the sorted projections, over all directions (a [N][S])."""
    s = torch.sort(a.t(), dim=1)[0]
    return int((s[:, 1:] == s[:, :-1]).sum())


def swd_ref(inp, case):
    """weight / (S N) * sum_{s, r} (sort_r(z . w_s) - sort_r(prior . w_s))^p and its gradient w.r.t. z, in float64.  The
    coefficient is formed as the launcher forms it: float32 weight / (float32 S * float32 N)."""
    z = f64(inp["z"]).requires_grad_(True)
    pj = f64(inp["proj"])
    wd = torch.sort(z.matmul(pj.t()).t(), dim=1)[0] - torch.sort(f64(inp["prior"]).matmul(pj.t()).t(), dim=1)[0]
    coef = f32s(SWD_WEIGHT) / (case.S * case.N)
    out = coef * wd.pow(case.p).sum()
    (g,) = torch.autograd.grad(out, z)
    return dict(out=out.detach(), g_z=g, wd=wd.detach(), coef=coef)


def swd_bounds(inp, case, ref):
    """A projection is a float32 dot product of length D: error at most D u sum |z w| (0 in the exact cases).  Sorting is
    1-Lipschitz in the maximum norm, so a rank-wise difference d moves by at most da + dc, the largest projection errors of its
    direction, and u |d| for the subtraction (exact in the exact cases).  t = d^p: p |d|^(p-1) times that, and one rounding (d * d,
    or powf: 1 ulp).  The direction's sum: ceil(N / 256) + 6 + 2 additions; the partials are added in double; coef is a float32
    quotient of a float32 weight (2) and the result is cast once (1):
        out:  coef sum [p |d|^(p-1) dd + (1 + chain) u |t|] + 3 u |out|
    Gradient, exact cases only: dA = p d^(p-1) (2 d exact, else powf and a product: 2), S products and additions, coef (2 + 1):
        g_z:  (S + 6) u |coef| sum_s |dA w|"""
    z, pr, pj = f64(inp["z"]), f64(inp["prior"]), f64(inp["proj"])
    N, D, S, p = case.N, case.D, case.S, case.p
    wd, coef = ref["wd"], ref["coef"]                                   # [S][N]
    chain = -(-N // 256) + 8
    if case.exact:
        dd = torch.zeros(S, 1, dtype=torch.float64)
    else:
        da = D * EPS32 * (z.abs() @ pj.abs().t()).max(0)[0]
        dc = D * EPS32 * (pr.abs() @ pj.abs().t()).max(0)[0]
        dd = (da + dc).view(S, 1) + EPS32 * wd.abs()
    t = wd.abs().pow(p)
    b_out = coef * float((p * wd.abs().pow(p - 1.0) * dd + (1.0 + chain) * EPS32 * t).sum()) + 3.0 * EPS32 * float(ref["out"].abs())
    out = dict(out=torch.tensor(b_out, dtype=torch.float64))
    if case.exact:
        a = z.matmul(pj.t())                                            # [N][S]: exact
        order = torch.sort(a.t(), dim=1)[1]                             # [S][N] sample index at each rank
        dA = torch.zeros(N, S, dtype=torch.float64)
        dA[order, torch.arange(S).view(S, 1).expand(S, N)] = p * wd.abs().pow(p - 1.0)
        out["g_z"] = (S + 6.0) * EPS32 * coef * (dA @ pj.abs())
    return out


# ---------------------------------------------------------------------------------------------------------------------
# csrc/gamma.hip: the reparameterisation
# ---------------------------------------------------------------------------------------------------------------------
GAMMA_SIZES = [1, 255, 257, BWD_BLOCKS * 256 + 5]
GAMMA_SHAPES = (8.0, 1.0)


def gamma_inputs(n, shape_b):
    """alpha log-uniform in (0.01, 20), beta in (0.05, 20); zhat around alpha + shape_b as a Gamma(alpha + shape_b, 1) draw is."""
    g = gen_of(f"gamma-{n}-{shape_b}", 11)
    alpha = torch.exp(torch.rand(n, generator=g) * np.log(20.0 / 0.0101) + np.log(0.0101))
    beta = torch.exp(torch.rand(n, generator=g) * np.log(19.9 / 0.0501) + np.log(0.0501))
    zhat = (alpha + shape_b) * torch.exp(0.4 * torch.randn(n, generator=g))
    return dict(alpha=alpha, beta=beta, zhat=zhat, g=torch.randn(n, generator=g))


def gamma_reparam64(alpha, beta, zhat, shape_b):
    """GammaVAE.reparameterize as oracle/vae_cpu.py:gamma_forward writes it."""
    a = alpha + shape_b
    eps = torch.sqrt(9. * a - 3.) * ((zhat / (a - 1. / 3.)) ** (1. / 3.) - 1.)
    return (a - 1. / 3.) * (1 + eps / torch.sqrt(9. * a - 3.)) ** 3 / beta


def gamma_reparam_ref(inp, shape_b):
    alpha, beta = f64(inp["alpha"]).requires_grad_(True), f64(inp["beta"]).requires_grad_(True)
    z = gamma_reparam64(alpha, beta, f64(inp["zhat"]), shape_b)
    ga, gb = torch.autograd.grad((z * f64(inp["g"])).sum(), [alpha, beta])
    return dict(z=z.detach(), g_alpha=ga, g_beta=gb)


def gamma_reparam_bounds(inp, shape_b):
    """a = alpha + Bs (1);  q = 9 a - 3: 3 u a 9 / q <= 3.4 u (a >= 1);  s = sqrtf(q): 3 u;  m = a - 1/3 (the constant is a float32):
    3 u a / m <= 4.5 u.  x = zhat / m: 5.5 u;  r = powf(x, 1/3): a third of that, powf's ulp and the exponent's rounding
    |log x| / 3 u / 2:  rho_r = (3 + |log x| / 3) u.  eps = s (r - 1) inherits r's error ABSOLUTELY: s rho_r r + 4 u |eps|;
    t = 1 + eps / s = r up to rounding:  dt <= rho_r r + 7 u |r - 1| + u t.
      z = m t^3 / beta: z (4.5 u + 3 dt / t + 3 u)
      g_beta = -g z / beta: the same and two more roundings
      g_alpha = g (dha + dhe deps) / beta is a cancellation: both partials are O(t^3) and their sum is O(rounding) (z beta == zhat
        whatever alpha is).  Its A is the SUM OF THE MAGNITUDES of the two partials, not of the result:
        A = |g| / beta (t^3 + |13.5 m t^2 eps / (q s)| + dhe (|4.5 (r - 1) / s| + s r / (3 m))),  dhe = 3 m t^2 / s.
        Longest path: dhe (m 4.5, t^2 2 dt / t ~ 10, s 3, three operations: 20), deps (1.5 rho_r + 6: 11), the product, the sum,
        g and 1 / beta: c = 36."""
    alpha, beta, zhat, g = (f64(inp[k]) for k in ("alpha", "beta", "zhat", "g"))
    a = alpha + shape_b
    q, m = 9.0 * a - 3.0, a - 1.0 / 3.0
    s = q.sqrt()
    x = zhat / m
    r = x ** (1.0 / 3.0)
    eps = s * (r - 1.0)
    t = 1.0 + eps / s
    rho_r = (3.0 + x.log().abs() / 3.0) * EPS32
    dt = rho_r * r + 7.0 * EPS32 * (r - 1.0).abs() + EPS32 * t
    z = m * t ** 3 / beta
    bz = z * (7.5 * EPS32 + 3.0 * dt / t)
    dhe = 3.0 * m * t * t / s
    A = g.abs() / beta * (t ** 3 + (13.5 * m * t * t * eps / (q * s)).abs() + dhe * ((4.5 * (r - 1.0) / s).abs() + s * r / (3.0 * m)))
    return dict(z=bz, g_beta=(g * z / beta).abs() * (9.5 * EPS32 + 3.0 * dt / t), g_alpha=36.0 * EPS32 * A, partials=A)


# csrc/gamma.hip: the KL term between Gamma posteriors and the Gamma prior
GAMMA_KL_SHAPES = [(1, 1), (6, 40), (3, 255), (3, 257)]      # one element; one partial row walk; one short of / one past a full walk
GAMMA_PRIORS = [(2.0, 1.0), (0.5, 3.0)]                      # digammaf_pos(d) takes five resp. three recurrence steps
# lgammaf is a library call whose accuracy the code does not show.  Measured on an MI355X, 2026-10-20: torch.lgamma on a float32
# device tensor against float64 over 2^20 arguments log-uniform in (0.01, 20) and {0.5, 1, 2, 3}: largest
# |err| / (2^-23 max(1, |lgamma x|)) = LGAMMA_MEASURED.  The constant is 4 x that (one further rounding on either side, another
# argument reduction).  The yardstick is torch's device arithmetic, never the kernel under test.
LGAMMA_MEASURED = 2.42
C_LGAMMA = 4.0 * LGAMMA_MEASURED


def gamma_kl_inputs(B, D, prior):
    """alpha log-uniform in (0.01, 20); beta log-uniform in (0.01, 20): digammaf_pos runs zero to six recurrence steps."""
    g = gen_of(f"gamma-kl-{B}-{D}-{prior}", 12)
    lo, hi = np.log(0.0101), np.log(19.9)
    return dict(alpha=torch.exp(torch.rand(B, D, generator=g) * (hi - lo) + lo), beta=torch.exp(torch.rand(B, D, generator=g) * (hi - lo) + lo))


def gamma_kl64(alpha, beta, prior):
    """mean_b sum_d I(c, d, c, d) - I(1 / alpha, beta, c, d) with I(a, b, c, d) = -c d / a - b log a - lgamma(b) + (b - 1)(digamma(d) +
    log c), c = 1 / prior_alpha (a float32 quotient in the launcher), d = prior_beta: the header of gamma.hip."""
    c = torch.tensor(float(np.float32(1.0) / np.float32(prior[0])), dtype=torch.float64)
    d = torch.tensor(f32s(prior[1]), dtype=torch.float64)
    k0 = torch.special.digamma(d) + torch.log(c)
    i_prior = -d - d * torch.log(c) - torch.lgamma(d) + (d - 1.0) * k0
    i_post = -c * d * alpha + beta * torch.log(alpha) - torch.lgamma(beta) + (beta - 1.0) * k0
    return (i_prior - i_post).sum(1).mean()


def gamma_kl_ref(inp, prior, g=1.0):
    alpha, beta = f64(inp["alpha"]).requires_grad_(True), f64(inp["beta"]).requires_grad_(True)
    out = gamma_kl64(alpha, beta, prior)
    ga, gb = torch.autograd.grad(out * float(np.float32(g)), [alpha, beta])
    return dict(out=out.detach(), g_alpha=ga, g_beta=gb)


def digamma_bound(x):
    """digammaf_pos: k = ceil(6 - x) steps r -= 1 / x (a quotient and a sum each), then logf (1 ulp), 1 / x, its square and a Horner
    form of three terms below 1 / 12 (6 roundings at sizes below 1 + |log|); the series is cut behind i^6 / 252: the next term is
    below 1 / (240 * 6^8) = 2.5e-9.  (k + 6) u (sum of the 1 / (x + i) + |log(x + k)| + 1) + 2.5e-9."""
    k = torch.clamp(torch.ceil(6.0 - x), min=0.0)
    R = torch.zeros_like(x)
    for i in range(6):
        R = R + torch.where(k > i, 1.0 / (x + i), torch.zeros_like(x))
    return (k + 6.0) * EPS32 * (R + torch.log(x + k).abs() + 1.0) + 2.5e-9


def gamma_kl_bounds(inp, prior, g=1.0):
    """Scalars of the launch: k0 = psi(d) + logf(c): digamma_bound(d) + u (|log c| + |k0|);  i_prior = -d - d log c - lgamma(d) +
    (d - 1) k0: six roundings at the size of its magnitudes, lgammaf, and k0's error times |d - 1|.
    Element: i_prior - (-c d al + be logf(al) - lgammaf(be) + (be - 1) k0): eight roundings and a logf at the size of
    S = |i_prior| + c d al + be |log al| + |lgamma be| + |be - 1| |k0|:  9 u S + C_LGAMMA u max(1, |lgamma be|) + |be - 1| dk0 + di_prior.
    Row sum: ceil(D / 256) + 6 + 2 additions at the size of sum S; the rows are added in double; / B and one cast.
    Backward: s = g / B (1);  g_alpha = s (c d - be / al): 4 u |s| (c d + be / al);
      g_beta = s (-logf(al) + psi(be) - k0): |s| (digamma_bound(be) + dk0 + 4 u (|log al| + |psi be| + |k0|))."""
    alpha, beta = f64(inp["alpha"]), f64(inp["beta"])
    B, D = alpha.shape
    u = EPS32
    c = torch.tensor(float(np.float32(1.0) / np.float32(prior[0])), dtype=torch.float64)
    d = torch.tensor(f32s(prior[1]), dtype=torch.float64)
    k0 = torch.special.digamma(d) + torch.log(c)
    dk0 = digamma_bound(d) + u * (torch.log(c).abs() + k0.abs())
    ip_mag = d + d * torch.log(c).abs() + torch.lgamma(d).abs() + (d - 1.0).abs() * k0.abs()
    dip = 6.0 * u * ip_mag + C_LGAMMA * u * torch.lgamma(d).abs().clamp(min=1.0) + (d - 1.0).abs() * dk0
    S = ip_mag + c * d * alpha + beta * alpha.log().abs() + torch.lgamma(beta).abs() + (beta - 1.0).abs() * k0.abs()
    elem = 9.0 * u * S + C_LGAMMA * u * torch.lgamma(beta).abs().clamp(min=1.0) + (beta - 1.0).abs() * dk0 + dip
    rows = elem.sum(1) + (-(-D // 256) + 8) * u * S.sum(1)
    out = gamma_kl64(alpha, beta, prior)
    s = abs(float(np.float32(g))) / B
    psi = torch.special.digamma(beta)
    return dict(out=rows.mean() + u * out.abs(), g_alpha=4.0 * u * s * (c * d + beta / alpha),
                g_beta=s * (digamma_bound(beta) + dk0 + 4.0 * u * (alpha.log().abs() + psi.abs() + k0.abs())))


# ---------------------------------------------------------------------------------------------------------------------
# csrc/dip.hip
# ---------------------------------------------------------------------------------------------------------------------
DIP_MAX_D = 1024
DIP_LAMBDAS = (10.0, 5.0)                                    # lambda_diag, lambda_offdiag
DIP_SHAPES = [(1, 3), (3, 1), (5, 255), (5, 257), (2, 1024)]  # B < D with one sample; D = 1; one short of / one past a row walk; the limit


def dip_inputs(B, D):
    """mu, log_var as column slices of [B][D + 3] tensors (row stride D + 3)."""
    g = gen_of(f"dip-{B}-{D}", 13)
    mu_full, lv_full = torch.randn(B, D + 3, generator=g), torch.rand(B, D + 3, generator=g) * 2.0 - 1.5
    return dict(mu=mu_full[:, 1:1 + D], lv=lv_full[:, 2:2 + D], mu_full=mu_full, lv_full=lv_full)


def dip64(mu, lv, l_diag, l_off):
    """The header of dip.hip: c = mu - rowmean(mu), cz = c^T c + mean_{i < min(B, D)} exp(2 lv[i][i]),
    dip = l_off sum_{i != j} cz_ij^2 + l_diag sum_i (cz_ii - 1)^2."""
    c = mu - mu.mean(dim=1, keepdim=True)
    cz = c.t().matmul(c) + torch.diagonal((2.0 * lv).exp()).mean()
    dg = torch.diagonal(cz)
    return l_off * ((cz * cz).sum() - (dg * dg).sum()) + l_diag * ((dg - 1.0) ** 2).sum()


def dip_ref(inp, g=1.0):
    mu, lv = f64(inp["mu"]).requires_grad_(True), f64(inp["lv"]).requires_grad_(True)
    out = dip64(mu, lv, *DIP_LAMBDAS)
    gm, gl = torch.autograd.grad(out * float(np.float32(g)), [mu, lv])
    return dict(out=out.detach(), g_mu=gm, g_lv=gl)


def dip_bounds(inp, g=1.0):
    """Every step of the four kernels, first order; w(n) = ceil(n / 256) + 9 is a 256-thread walk with block_sum_256 behind it.
      mean = sum mu / D: (w(D) + 1) u mean |mu|;   c = mu - mean: dc = dmean + u |c|
      e = expf(2 lv): u e;   v = sum e / m: (w(m) + 2) u v
      cov_ij = sum_b c_bi c_bj: (B + 1) u sum |c_bi c_bj| + sum (|c_bi| dc_bj + dc_bi |c_bj|);   cz = cov + v: + dv + u |cz|
      t = cz - [i == j]:  dt = dcz + u |t|;   term = l t^2: l (2 |t| dt + 2 u t^2);   G = 2 l t: 2 l dt + u |G|
      dip: sum of the terms' errors + w(D) u sum of the terms (the rows are added in double) + u |dip|
      d dip / d v = sum G likewise;   g_lv[b][b] = g0 dv 2 e / m: |g0| 2 e / m (d(dv) + 5 u |dv|), every other entry exactly 0
      dcb_j = 2 sum_i c_bi G_ij: 2 ((D + 1) u sum |c_bi G_ij| + sum (dc_bi |G_ij| + |c_bi| dG_ij))
      g_mu = g0 (dcb - mean(dcb)): |g0| (d(dcb) + mean d(dcb) + (4 + 9 + 1) u mean |dcb| + 2 u (|dcb| + |mean|))"""
    mu, lv = f64(inp["mu"]), f64(inp["lv"])
    B, D = mu.shape
    m = min(B, D)
    u = EPS32
    ld, lo = DIP_LAMBDAS
    w = lambda n: -(-n // 256) + 9                                   # noqa: E731
    c = mu - mu.mean(1, keepdim=True)
    dc = (w(D) + 1) * u * mu.abs().mean(1, keepdim=True) + u * c.abs()
    e = torch.diagonal((2.0 * lv).exp())
    v = e.mean()
    dv = (w(m) + 2) * u * v
    ca = c.abs()
    cz = c.t() @ c + v
    dcz = (B + 1) * u * (ca.t() @ ca) + ca.t() @ dc + dc.t() @ ca + dv + u * cz.abs()
    eye = torch.eye(D, dtype=torch.float64)
    lam = lo + (ld - lo) * eye
    t = cz - eye
    dt = dcz + u * t.abs()
    term = lam * t * t
    dterm = lam * (2.0 * t.abs() * dt + 2.0 * u * t * t)
    G = 2.0 * lam * t
    dG = 2.0 * lam * dt + u * G.abs()
    dip = term.sum()
    b_out = dterm.sum() + w(D) * u * term.sum() + u * dip.abs()
    dvg = G.sum()
    d_dvg = dG.sum() + w(D) * u * G.abs().sum() + u * dvg.abs()
    g0 = abs(float(np.float32(g)))
    b_lv = torch.zeros(B, D, dtype=torch.float64)
    i = torch.arange(m)
    b_lv[i, i] = g0 * 2.0 * e / m * (d_dvg + 5.0 * u * dvg.abs())
    dcb = 2.0 * (c @ G)
    d_dcb = 2.0 * ((D + 1) * u * (ca @ G.abs()) + dc @ G.abs() + ca @ dG)
    mean = dcb.mean(1, keepdim=True)
    b_mu = g0 * (d_dcb + d_dcb.mean(1, keepdim=True) + 14.0 * u * dcb.abs().mean(1, keepdim=True) + 2.0 * u * (dcb.abs() + mean.abs()))
    return dict(out=b_out, g_mu=b_mu, g_lv=b_lv)


# ---------------------------------------------------------------------------------------------------------------------
# csrc/catlatent.hip
# ---------------------------------------------------------------------------------------------------------------------
CAT_MAX_Q = 256
CAT_EPS, CAT_TEMP = float(np.float32(1e-7)), 0.5
CatCase = namedtuple("CatCase", "id rows Q why")
CAT_CASES = [
    CatCase("Q1-rows600", 600, 1, "G = 1: 256 rows per block, <1>; every probability is 1"),
    CatCase("Q64-rows4101", 4101, 64, "G = 64, <1>, full lanes; more than 1024 * 4 rows: the KL forward grid wraps"),
    CatCase("Q65-rows7", 7, 65, "<2> with one element in the second round"),
    CatCase("Q128-rows33", 33, 128, "<2> full"),
    CatCase("Q129-rows7", 7, 129, "<4> with one element in the third round"),
    CatCase("Q256-rows4101", 4101, 256, "<4> full: the limit; the KL forward grid wraps"),
]


def cat_batch(rows):
    return 3 if rows % 3 == 0 else 1


def cat_inputs(case):
    """Logits 2 N(0, 1); uniform draws kept in [1e-3, 1 - 1e-3]: -log(-log(u + eps) + eps) amplifies a rounding of u + eps by
    1 / (-log u), without bound as u -> 1 (a condition of the case, checked on the host)."""
    g = gen_of("cat-" + case.id, 14)
    z = 2.0 * torch.randn(case.rows, case.Q, generator=g)
    u = torch.rand(case.rows, case.Q, generator=g) * 0.998 + 0.001
    return dict(z=z, u=u, gs=torch.randn(case.rows, case.Q, generator=g))


def _softmax_err(x, dx, npl):
    """Relative error of group_softmax's probabilities for float32 inputs x carrying absolute errors dx: x - m one rounding
    (|x - m| u / 2, passed on by the exponential), expf u; the sum is npl + 6 additions, 1 / s and the product 2 more; an input
    error moves p_k by dx_k relative, and the sum by its p-weighted mean:
        rho_k = a_k + sum_j p_j a_j + (npl + 8) u,   a_k = dx_k + (1 + |x_k - m|) u"""
    p = torch.softmax(x, dim=1)
    a = dx + (1.0 + (x - x.max(1, keepdim=True)[0]).abs()) * EPS32
    return p, a + (p * a).sum(1, keepdim=True) + (npl + 8.0) * EPS32


def cat_npl(Q):
    G = 1
    while G < Q and G < 64:
        G <<= 1
    return 1 if Q <= G else (2 if Q <= 2 * G else 4)


def gumbel_ref(inp, case):
    """s = softmax((z + g) / temp), g = -log(-log(u + eps) + eps)  (cat_vae.py:125-130).
    a = u + eps (u / 2 relative); L = logf(a): u |L| + u / 2 absolute; w = -L + eps: dw = u (|L| + 1 + |w|); g = -logf(w): dw / w + u |g|;
    t = (z + g) * (1 / temp): (dg + u |z + g|) / temp + u |t|; then _softmax_err."""
    z, u = f64(inp["z"]), f64(inp["u"])
    L = torch.log(u + CAT_EPS)
    w = -L + CAT_EPS
    g = -torch.log(w)
    it = float(np.float32(1.0) / np.float32(CAT_TEMP))
    t = (z + g) * it
    dg = EPS32 * (L.abs() + 1.0 + w.abs()) / w + EPS32 * g.abs()
    dt = (dg + EPS32 * (z + g).abs()) * it + EPS32 * t.abs()
    p, rho = _softmax_err(t, dt, cat_npl(case.Q))
    return p, p * rho


def gumbel_bwd_ref(s32, gs, case):
    """g_z = s (g_s - sum_q g_s s) / temp from the float32 sample handed in: the dot product is npl + 6 additions of products (+ 1),
    then a difference and two products:  ((npl + 7) u s sum |s g_s| + 3 u s (|g_s| + |dot|)) / temp."""
    s, g = f64(s32), f64(gs)
    it = float(np.float32(1.0) / np.float32(CAT_TEMP))
    dot = (s * g).sum(1, keepdim=True)
    gz = s * (g - dot) * it
    return gz, ((cat_npl(case.Q) + 7.0) * EPS32 * s * (s * g).abs().sum(1, keepdim=True) + 3.0 * EPS32 * s * (g.abs() + dot.abs())) * it


def cat_log_prior(Q):
    return float(np.float32(np.log(1.0 / Q + CAT_EPS)))


def cat_kl_ref(inp, case, g=1.0):
    q = f64(inp["z"]).requires_grad_(True)
    p = torch.softmax(q, dim=1)
    kld = (p * torch.log(p + CAT_EPS) - p * cat_log_prior(case.Q)).sum() / cat_batch(case.rows)
    (gq,) = torch.autograd.grad(kld * float(np.float32(g)), q)
    return dict(out=kld.detach(), g_q=gq)


def cat_kl_bounds(inp, case, g=1.0):
    """p with _softmax_err (dp = p rho).  term = p logf(p + eps) - p c: the derivative t = log(p + eps) + p / (p + eps) - c carries dp;
    p + eps and logf: u p (1 + |log|); two products and the difference: u (p |log| + p |c| + |term|).
    Sum: a group adds ceil(rows / (blocks * 256 / G)) rows of npl terms, block_sum_256 adds 9; the partials are added in double,
    / B and one cast.
    Backward g_q = (g / B) p (t - dot), dot = sum p t:  dt = u (|log| + 2 + 2 |t|) + 2 rho  (d/dp of t is below 2 / (p + eps));
    ddot = sum (dp |t| + p dt) + (npl + 7) u sum p |t|;  dg_q = |g / B| (dp |t - dot| + p (dt + ddot) + 3 u p (|t| + |dot|))."""
    q = f64(inp["z"])
    rows, Q = q.shape
    npl = cat_npl(Q)
    u = EPS32
    c = cat_log_prior(Q)
    p, rho = _softmax_err(q, torch.zeros_like(q), npl)
    dp = p * rho
    lg = torch.log(p + CAT_EPS)
    t = lg + p / (p + CAT_EPS) - c
    term = p * lg - p * c
    dterm = t.abs() * dp + u * p * (1.0 + lg.abs()) + u * (p * lg.abs() + p * abs(c) + term.abs())
    G = min(64, 1 << max(0, (Q - 1).bit_length()))
    gpb = 256 // G
    blocks = max(1, min(1024, -(-rows // gpb)))
    chain = -(-rows // (blocks * gpb)) * npl + 9
    B = cat_batch(rows)
    out = term.sum() / B
    b_out = (dterm.sum() + chain * u * (p * lg.abs() + p * abs(c)).sum()) / B + u * out.abs()
    sc = abs(float(np.float32(g))) / B
    dot = (p * t).sum(1, keepdim=True)
    dt = u * (lg.abs() + 2.0 + 2.0 * t.abs()) + 2.0 * rho
    ddot = (dp * t.abs() + p * dt).sum(1, keepdim=True) + (npl + 7.0) * u * (p * t.abs()).sum(1, keepdim=True)
    return dict(out=b_out, g_q=sc * (dp * (t - dot).abs() + p * (dt + ddot) + 3.0 * u * p * (t.abs() + dot.abs())))


# ---------------------------------------------------------------------------------------------------------------------
# csrc/mmd.hip
# ---------------------------------------------------------------------------------------------------------------------
MMD_MAX_D = 512
MMD_W = (float(np.float32(0.3)), float(np.float32(0.5)), float(np.float32(0.7)))          # w_pp, w_zz, w_pz
MMD_ZVAR, MMD_EPS = 2.0, float(np.float32(1e-7))
MmdCase = namedtuple("MmdCase", "id N D kind why")
MMD_CASES = ([MmdCase(f"{kind}-N5-D{D}", 5, D, kind, f"mmd_rows_kernel<{npl}, {kind}>" + tail)
              for kind in ("imq", "rbf")
              for D, npl, tail in ((1, 1, ": 63 idle lanes"), (64, 1, " full"), (65, 2, ": one element in the second round"), (128, 2, " full"),
                                   (129, 4, ""), (256, 4, " full"), (257, 8, ""), (512, 8, " full: the limit"))]
             + [MmdCase(f"{kind}-N{N}-D65", N, 65, kind, why) for kind in ("imq", "rbf")
                for N, why in ((1, "one row: imq sums are all 0 (only the diagonal)"), (2, "fewer rows than waves"))]
             + [MmdCase(f"{kind}-N129-D512", 129, 512, kind, "N D / 256 = 258: the rbf finish grid is capped at 256 blocks; 33 rows per wave")
                for kind in ("imq", "rbf")])


def mmd_npl(D):
    return 1 if D <= 64 else 2 if D <= 128 else 4 if D <= 256 else 8


def mmd_inputs(case):
    g = gen_of("mmd-" + case.id, 15)
    return dict(z=torch.randn(case.N, case.D, generator=g) * 1.3 + 0.2, prior=torch.randn(case.N, case.D, generator=g))


def mmd_c(D):
    return 2.0 * D * MMD_ZVAR


def mmd_kernel64(a, b, kind, c):
    """compute_kernel of wae_mmd.py:120-198 as the header of mmd.hip restates it: imq sums C / (eps + C + |a_i - b_j|^2) over i != j
    (the cross term's diagonal is removed too); rbf is the mean over all pairs of exp(-mean_d (a_i - b_j)^2 / C)."""
    d2 = (a.unsqueeze(1) - b.unsqueeze(0)).pow(2).sum(-1)
    if kind == "rbf":
        return torch.exp(-(d2 / a.shape[1]) / c).mean()
    k = c / (MMD_EPS + c + d2)
    return k.sum() - k.diag().sum()


def mmd_ref(inp, case):
    z, p = f64(inp["z"]).requires_grad_(True), f64(inp["prior"])
    c = mmd_c(case.D)
    pp, zz, pz = mmd_kernel64(p, p, case.kind, c), mmd_kernel64(z, z, case.kind, c), mmd_kernel64(p, z, case.kind, c)
    mmd = MMD_W[0] * pp + MMD_W[1] * zz - 2.0 * MMD_W[2] * pz
    (g,) = torch.autograd.grad(mmd, z)
    return dict(out4=torch.stack([mmd, pp, zz, pz]).detach(), g_z=g)


def mmd_bounds(inp, case):
    """d2 = sum_d (a - b)^2: a lane adds npl squares of rounded differences (3 u each), wave_sum 6:  dd2 = (npl + 9) u d2.
      imq  s = eps + C + d2 (2 u s), r = 1 / s, k = C r:  rho_r = (dd2 + 2 u s) / s + u,  k (rho_r + u)
      rbf  x = -(d2 / D) / C (1 / D, a product, a quotient: 3 u), k = expf(x):  rho_k = |x| ((npl + 9) u + 3 u) + u
      row sums: a wave adds ceil(N / 4) values, the merge 2 deep: (ceil(N / 4) + 2) u sum k; rows are added in double, * norm
      (rbf: 1 / (N N) as a float32, 1) and one cast (1): + 2 u |K|;  mmd = w_pp K_pp + w_zz K_zz - 2 w_pz K_pz: the three bounds with
      their weights and 3 u (|w_pp K_pp| + |w_zz K_zz| + |2 w_pz K_pz|).
      gradient: g_i = sum_j f_zz (z_i - z_j) + f_pz (z_i - p_j); imq f = +-2 w (-2 C r^2): 2 rho_r + 4 u; rbf f = +-2 w k (-2 / D / C):
      rho_k + 5 u; the difference and the product 2 u more; 2 ceil(N / 4) + 3 additions at the size of sum |terms|; rbf: * norm, 2 u."""
    z, p = f64(inp["z"]), f64(inp["prior"])
    N, D = z.shape
    u, c, npl = EPS32, mmd_c(D), mmd_npl(D)
    cN = -(-N // 4) + 2
    imq = case.kind == "imq"
    off = 1.0 - torch.eye(N, dtype=torch.float64) if imq else torch.ones(N, N, dtype=torch.float64)

    def pair(a, b):
        diff = a.unsqueeze(1) - b.unsqueeze(0)                            # [N][N][D]
        d2 = diff.pow(2).sum(-1)
        if imq:
            s = MMD_EPS + c + d2
            rho = ((npl + 9) * u * d2 + 2.0 * u * s) / s + u
            k = c / s * off
            return diff, k, k * (rho + u), 2.0 * c / (s * s) * off, 2.0 * rho + 4.0 * u
        x = d2 / D / c
        rho = x * (npl + 12) * u + u
        k = torch.exp(-x)
        return diff, k, k * rho, k * 2.0 / D / c, rho + 5.0 * u
    res = {}
    for name, a, b in (("pp", p, p), ("zz", z, z), ("zp", z, p)):
        diff, k, dk, f, rf = pair(a, b)
        norm = 1.0 if imq else 1.0 / (N * N)
        K = k.sum() * norm
        res[name] = (K, (dk.sum() + cN * u * k.sum()) * norm + 2.0 * u * K, diff, f, rf)
    w_pp, w_zz, w_pz = MMD_W
    b_out = (w_pp * res["pp"][1] + w_zz * res["zz"][1] + 2.0 * w_pz * res["zp"][1]
             + 3.0 * u * (w_pp * res["pp"][0] + w_zz * res["zz"][0] + 2.0 * w_pz * res["zp"][0]))
    out4 = torch.stack([b_out, res["pp"][1], res["zz"][1], res["zp"][1]])
    bg = torch.zeros(N, D, dtype=torch.float64)
    tot = torch.zeros(N, D, dtype=torch.float64)
    for name, w in (("zz", 2.0 * w_zz), ("zp", 2.0 * w_pz)):
        _, _, diff, f, rf = res[name]
        t = (w * f).unsqueeze(2) * diff.abs()
        bg = bg + (t * (rf + 2.0 * u).unsqueeze(2)).sum(1)
        tot = tot + t.sum(1)
    norm = 1.0 if imq else 1.0 / (N * N)
    return dict(out4=out4, g_z=(bg + (2 * cN + 3 + (0 if imq else 2)) * u * tot) * norm)


# ---------------------------------------------------------------------------------------------------------------------
# csrc/iwloss.hip
# ---------------------------------------------------------------------------------------------------------------------
IW_M_N = float(np.float32(0.025))
IwCase = namedtuple("IwCase", "id B S n L saturated why")
IW_CASES = [
    IwCase("S1-R300", 300, 1, 4, 1, False, "more than 256 groups: a second group for 44 threads of the finish; S = 1: weight 1"),
    IwCase("S2-n1028-L33", 4, 2, 1028, 33, False, "two steps of the row walk for one thread"),
    IwCase("S5-n1200-L300", 3, 5, 1200, 300, False, "L > 256: a second step of the KL walk"),
    IwCase("S5-saturated", 2, 5, 64, 8, True, "one sample's log-weight 60 above the others: its weight rounds to 1"),
]


def iw_inputs(case):
    """recons [B][S][n], x [B][n], mu, lv [B][S][L].  saturated: sample 2 of every group lies sqrt(60) off its picture."""
    g = gen_of("iw-" + case.id, 16)
    B, S, n, L = case.B, case.S, case.n, case.L
    x = torch.rand(B, n, generator=g)
    r = x.unsqueeze(1) + 0.3 * torch.randn(B, S, n, generator=g)
    if case.saturated:
        r[:, 2] = r[:, 2] + 60.0 ** 0.5 + 1.0
    return dict(recons=r, x=x, mu=torch.randn(B, S, L, generator=g), lv=torch.rand(B, S, L, generator=g) * 4.0 - 3.0)


def iw_forward64(recons, x, mu, lv, keep=None):
    """The header of iwloss.hip.  keep: the one sample per group that takes part (the saturated case's self-check)."""
    lp = ((recons - x.unsqueeze(1)) ** 2).mean(-1)
    kld = -0.5 * (1 + lv - mu ** 2 - lv.exp()).sum(-1)
    lw = lp + IW_M_N * kld
    lwk = lw if keep is None else lw[:, keep:keep + 1]
    w = torch.softmax(lwk, dim=-1)
    e = (w * lwk).sum(-1)
    return torch.stack([e.mean(), lp.mean(), kld.mean(), -kld.mean()]), lp, kld, lw, w, e


def iw_ref(inp, g=1.0):
    t = [f64(inp[k]).requires_grad_(True) for k in ("recons", "mu", "lv")]
    out4, lp, kld, lw, w, e = iw_forward64(t[0], f64(inp["x"]), t[1], t[2])
    gs = torch.autograd.grad(out4[0] * float(np.float32(g)), t + [lw], retain_graph=False)
    return dict(out4=out4.detach(), lp=lp.detach(), kld=kld.detach(), coef=gs[3] / float(np.float32(g)), g_recons=gs[0], g_mu=gs[1],
                g_lv=gs[2])


def iw_bounds(inp, g=1.0, own_coef=True):
    """lp = sum d^2 / n: a thread adds 4 ceil(n / 1024) squares of rounded differences (3 u each), block_sum_256 9, / n 1.
    kld = -0.5 sum (1 + l - m^2 - e^l): as loss.hip's KL term, 4 u per element and ceil(L / 256) + 9 additions at the size of
    1 + |l| + m^2 + e^l.  lw = lp + M_N kld: the two bounds and 2 u (|lp| + |M_N kld|).
    Softmax over the S samples of a group (one thread): w~_s = e^(lw_s - m) / den has the relative error
        rho_s = dlw_s + sum_t w~_t dlw_t + (S + 3 + |lw_s - m|) u        (the error of m is common and cancels)
    e = sum_s w~_s lw_s (the same weights in numerator and denominator: they stay normalised, so their errors act on lw_s - e):
        sum_s w~_s (rho_s |lw_s - e| + dlw_s) + (S + 2) u sum_s w~_s |lw_s|;  loss = mean_groups e in double, one cast.
    coef_s = w~_s (1 + lw_s - e) / groups: w~_s (rho_s |1 + lw_s - e| + dlw_s + de + 2 u (1 + |lw_s| + |e|) + 3 u |1 + lw_s - e|) / groups.
    Backward from the forward kernel's coef (own_coef: its bound rides on every gradient; else from coef rounded to float32):
    g_recons = g coef 2 / n (r - x): 6 u;  g_mu = g coef M_N mu: 4 u;
    g_lv = ck 0.5 (expf(l) - 1): u (|ck| e^l / 2 + 5 |g_lv|)."""
    r, x, mu, lv = (f64(inp[k]) for k in ("recons", "x", "mu", "lv"))
    B, S, n = r.shape
    L = mu.shape[-1]
    u = EPS32
    out4, lp, kld, lw, w, e = iw_forward64(r, x, mu, lv)
    dlp = (4 * -(-n // 1024) + 9 + 3 + 1) * u * lp
    dkld = (4 + -(-L // 256) + 9) * u * 0.5 * (1 + lv.abs() + mu * mu + lv.exp()).sum(-1) + u * kld.abs()
    dlw = dlp + IW_M_N * dkld + 2 * u * (lp.abs() + IW_M_N * kld.abs())
    m = lw.max(-1, keepdim=True)[0]
    rho = dlw + (w * dlw).sum(-1, keepdim=True) + (S + 3 + (lw - m).abs()) * u
    de = (w * (rho * (lw - e.unsqueeze(-1)).abs() + dlw)).sum(-1) + (S + 2) * u * (w * lw.abs()).sum(-1)
    groups = B
    t = 1 + lw - e.unsqueeze(-1)
    dcoef = w * (rho * t.abs() + dlw + de.unsqueeze(-1) + 2 * u * (1 + lw.abs() + e.abs().unsqueeze(-1)) + 3 * u * t.abs()) / groups
    b4 = torch.stack([de.mean() + u * out4[0].abs(), dlp.mean() + u * out4[1].abs(), dkld.mean() + u * out4[2].abs(),
                      dkld.mean() + u * out4[2].abs()])
    g0 = abs(float(np.float32(g)))
    coef = w * t / groups
    ck = g0 * coef.abs().unsqueeze(-1) * IW_M_N
    gl = ck * 0.5 * (lv.exp() - 1)
    dc = (dcoef if own_coef else u * coef.abs()).unsqueeze(-1) * g0
    dr = (2 / n * (r - x.unsqueeze(1))).abs()
    return dict(out4=b4, lp=dlp, kld=dkld, coef=dcoef, g_recons=6 * u * g0 * coef.abs().unsqueeze(-1) * dr + dc * dr,
                g_mu=4 * u * ck * mu.abs() + dc * IW_M_N * mu.abs(),
                g_lv=u * (ck * 0.5 * lv.exp() + 5 * gl.abs()) + dc * IW_M_N * 0.5 * (lv.exp() - 1).abs())


# ---------------------------------------------------------------------------------------------------------------------
# csrc/ssim.hip
# ---------------------------------------------------------------------------------------------------------------------
SSIM_SIDE, SSIM_LEVELS = 64, 5
SSIM_C1, SSIM_C2 = float(np.float32(0.01) * np.float32(0.01)), float(np.float32(0.03) * np.float32(0.03))      # kC1, kC2 as the kernel holds them
SSIM_WEIGHTS = [float(np.float32(v)) for v in (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)]
SsimCase = namedtuple("SsimCase", "id B C kind why")
SSIM_CASES = [
    SsimCase("B1-C1", 1, 1, "random", "one workgroup"),
    SsimCase("B2-C3", 2, 3, "random", "the model's channel count: channel-interleaved reads"),
    SsimCase("B3-C4", 3, 4, "random", "twelve workgroups"),
    SsimCase("B2-C3-same", 2, 3, "same", "recons == target: loss 0 and gradient 0 within the bound"),
    SsimCase("B2-C3-const", 2, 3, "const", "both pictures constant (1 / 8 and 1 / 16): only the stabilisers and the zero padding are left"),
]
SSIM_G = (1.0, -2.5)


def ssim_window():
    """The 11-tap window as kernels._mssim_host_arrays() hands it to the kernel (mssim_vae.py:203-206: a POSITIVE exponent), float32."""
    from math import exp
    k = torch.tensor([exp((x - 11 // 2) ** 2 / (2 * 1.5 ** 2)) for x in range(11)])
    return (k / k.sum()).float()


def ssim_inputs(case):
    """NCHW pictures in [0.05, 0.95]: the target uniform, the reconstruction the target plus N(0, 0.1^2) clamped to the range."""
    g = gen_of("ssim-" + case.id, 17)
    shape = (case.B, case.C, SSIM_SIDE, SSIM_SIDE)
    x = torch.rand(shape, generator=g) * 0.9 + 0.05
    if case.kind == "same":
        return dict(a=x.clone(), b=x)
    if case.kind == "const":
        return dict(a=torch.full(shape, 0.125), b=torch.full(shape, 0.0625))
    return dict(a=(x + 0.1 * torch.randn(shape, generator=g)).clamp(0.05, 0.95), b=x)


def _ssim_conv(t, win):
    C = t.shape[1]
    w2 = (win[:, None] * win[None, :]).expand(C, 1, 11, 11)
    return torch.nn.functional.conv2d(t, w2, padding=5, groups=C)


def ssim_moments(a, b, win):
    return _ssim_conv(a, win), _ssim_conv(b, win), _ssim_conv(a * a, win), _ssim_conv(b * b, win), _ssim_conv(a * b, win)


def ssim_maps(m1, m2, e11, e22, e12):
    """(cs map, ssim map, v1, v2) of one level from the five windowed moments, as the header of ssim.hip writes them."""
    mu11, mu22, mu12 = m1 * m1, m2 * m2, m1 * m2
    v1, v2 = 2.0 * (e12 - mu12) + SSIM_C2, (e11 - mu11) + (e22 - mu22) + SSIM_C2
    cs = v1 / v2
    return cs, (2.0 * mu12 + SSIM_C1) / (mu11 + mu22 + SSIM_C1) * cs, v1, v2


def ssim_forward64(a, b, win=None):
    """(loss, ms [5], mc [5], smallest contrast term) in the dtype of the pictures; the window's float32 values in that dtype."""
    win = ssim_window().to(a.dtype) if win is None else win
    ms, mc = [], []
    for l in range(SSIM_LEVELS):
        cs, ss, _, _ = ssim_maps(*ssim_moments(a, b, win))
        ms.append(ss.mean())
        mc.append(cs.mean())
        a, b = torch.nn.functional.avg_pool2d(a, 2), torch.nn.functional.avg_pool2d(b, 2)
    ms, mc = torch.stack(ms), torch.stack(mc)
    w = torch.tensor(SSIM_WEIGHTS, dtype=a.dtype)
    out = torch.prod(mc[:-1] ** w[:-1] * ms[-1] ** w[-1])
    return 1.0 - out, ms, mc


def ssim_coef64(loss, ms, mc, nwg):
    """coef[2 l] = d loss / d (ssim map element), coef[2 l + 1] = d loss / d (cs map element) of level l."""
    out, w = 1.0 - loss, SSIM_WEIGHTS
    coef = torch.zeros(2 * SSIM_LEVELS, dtype=torch.float64)
    for l in range(SSIM_LEVELS):
        n = nwg * (SSIM_SIDE >> l) ** 2
        if l == SSIM_LEVELS - 1:
            coef[2 * l] = -out * (SSIM_LEVELS - 1) * w[l] / ms[l] / n
        else:
            coef[2 * l + 1] = -out * w[l] / mc[l] / n
    return coef


def ssim_ref(inp, g=1.0):
    a = f64(inp["a"]).requires_grad_(True)
    loss, ms, mc = ssim_forward64(a, f64(inp["b"]))
    (ga,) = torch.autograd.grad(loss * float(np.float32(g)), a)
    B, C = a.shape[:2]
    return dict(loss=loss.detach(), ms=ms.detach(), mc=mc.detach(), coef=ssim_coef64(loss.detach(), ms.detach(), mc.detach(), B * C), g_a=ga)


def _ssim_pqr(m1, m2, e11, e22, e12, alpha, beta):
    """P, Q, R of ssim_bwd_kernel: the partial derivatives of alpha ssim + beta cs w.r.t. mu1, G*(a a), G*(a b); and their magnitude forms."""
    cs, _, v1, v2 = ssim_maps(m1, m2, e11, e22, e12)
    A1, A2 = 2.0 * m1 * m2 + SSIM_C1, m1 * m1 + m2 * m2 + SSIM_C1
    lum = A1 / A2
    dl, dc = 2.0 * (m2 - lum * m1) / A2, 2.0 * (cs * m1 - m2) / v2
    k = alpha * lum + beta
    kA = abs(alpha) * lum.abs() + abs(beta)
    PA = abs(alpha) * cs.abs() * 2.0 * (m2.abs() + (lum * m1).abs()) / A2 + kA * 2.0 * ((cs * m1).abs() + m2.abs()) / v2.abs()
    return (alpha * cs * dl + k * dc, -k * cs / v2, 2.0 * k / v2), (PA, kA * cs.abs() / v2.abs(), 2.0 * kA / v2.abs())


def ssim_bounds(inp, g=1.0):
    """First-order running error analysis, level by level (l = 0..4).  As in ladder_backward_bounds a rounding counts at the unit
    roundoff u / 2 (u = 2^-23), a library function's ulp at u.
    Leaves.  A pooled pixel of level l is l u relative (sums of positives).  A windowed moment is a sum of 121 positive products
    (window and pictures are positive): 11 + 11 additions, two products, for the second moments the product of two pixels and twice
    their pooled error:  rho(l) = (12.5 + 2 l) u relative on each of m1, m2, e11, e22, e12.
    Maps.  cs and ssim are rational functions of the five leaves: a leaf's error reaches them with the magnitude of its derivative
    (float64 autograd -- where s12 = e12 - m1 m2 cancels, that is exactly what the bound has to grow by); the operations behind the
    leaves add 4 u at the size of the magnitude form  (2 (e12 + m1 m2) + C2) / |v2| (1 + (e11 + e22 + m1^2 + m2^2 + C2) / |v2|).
    Means.  A thread adds max(1, S^2 / 1024) * 4 values, block_sum 8, the finish ceil(nwg / 256) + 8, / n:  that many u / 2 at mean |map|.
    loss = 1 - prod_{i<4} mc_i^w_i ms_4^w_4: five powf (u each), eight products, the difference (u / 2 each):
        out (sum_{i<4} w_i dmc_i / mc_i + 4 w_4 dms_4 / ms_4 + 10 u) + u |loss|;   coef: its mean's and out's relative bounds + 2 u.
    Gradient (coef handed over rounded: u).  P, Q, R like the maps (6 u at their magnitude forms); grad_l = G*P + 2 a G*Q + b G*R +
    a quarter of the coarser level's gradient: the filtered bounds of P, Q, R, (14 + l) u at G*|P| + 2 a G*|Q| + b G*|R|, a quarter
    of the coarser bound, u |grad_l|; * g: u."""
    a, b = f64(inp["a"]), f64(inp["b"])
    B, C = a.shape[:2]
    nwg = B * C
    u = EPS32
    win = ssim_window().double()
    ref = ssim_ref(inp, g)
    coef = ref["coef"]
    levels = []
    dms, dmc = [], []
    for l in range(SSIM_LEVELS):
        S = SSIM_SIDE >> l
        rho = (12.5 + 2.0 * l) * u
        leaves = [t.clone().requires_grad_(True) for t in ssim_moments(a, b, win)]
        cs, ss, v1, v2 = ssim_maps(*leaves)
        m1, m2, e11, e22, e12 = [t.detach() for t in leaves]
        A = (2.0 * (e12 + m1 * m2) + SSIM_C2) / v2.detach().abs() * (1.0 + (e11 + e22 + m1 * m1 + m2 * m2 + SSIM_C2) / v2.detach().abs())
        bmap = []
        for o in (ss, cs):
            gs = torch.autograd.grad(o.sum(), leaves, retain_graph=True)
            bmap.append(sum(gd.abs() * rho * t for gd, t in zip(gs, (m1, m2, e11, e22, e12))) + 4.0 * u * A)
        chain = max(1, S * S // 1024) * 4 + 8 + -(-nwg // 256) + 8 + 1
        dms.append(bmap[0].mean() + 0.5 * chain * u * ss.detach().abs().mean())
        dmc.append(bmap[1].mean() + 0.5 * chain * u * cs.detach().abs().mean())
        alpha, beta = float(coef[2 * l]), float(coef[2 * l + 1])
        (Pq, Qq, Rq), (PA, QA, RA) = _ssim_pqr(*leaves, alpha, beta)
        bpqr = []
        for o, oa in ((Pq, PA), (Qq, QA), (Rq, RA)):
            gs = torch.autograd.grad(o.sum(), leaves, retain_graph=True, allow_unused=True)           # R does not depend on e12
            bpqr.append((sum(gd.abs() * rho * t for gd, t in zip(gs, (m1, m2, e11, e22, e12)) if gd is not None) + 6.0 * u * oa.detach()).detach())
        levels.append((a, b, [t.detach() for t in (Pq, Qq, Rq)], bpqr))
        a, b = torch.nn.functional.avg_pool2d(a, 2), torch.nn.functional.avg_pool2d(b, 2)
    ms, mc, w = ref["ms"], ref["mc"], SSIM_WEIGHTS
    out = 1.0 - ref["loss"]
    rel_out = sum(w[i] * dmc[i] / mc[i].abs() for i in range(4)) + 4.0 * w[4] * dms[4] / ms[4].abs() + 10.0 * u
    b_loss = out.abs() * rel_out + u * ref["loss"].abs()
    b_coef = torch.zeros(10, dtype=torch.float64)
    for l in range(SSIM_LEVELS):
        rel_m = dms[l] / ms[l].abs() if l == 4 else dmc[l] / mc[l].abs()
        b_coef[2 * l if l == 4 else 2 * l + 1] = coef[2 * l if l == 4 else 2 * l + 1].abs() * (rel_out + rel_m + 2.0 * u)
    grad = bg = None
    for l in range(SSIM_LEVELS - 1, -1, -1):
        al, bl, (Pq, Qq, Rq), (bP, bQ, bR) = levels[l]
        f = lambda t: _ssim_conv(t, win)                                  # noqa: E731
        gr = f(Pq) + 2.0 * al * f(Qq) + bl * f(Rq)
        mag = f(Pq.abs()) + 2.0 * al * f(Qq.abs()) + bl * f(Rq.abs())
        bb = f(bP) + 2.0 * al * f(bQ) + bl * f(bR) + (14.0 + l) * u * mag
        if grad is not None:
            up = lambda t: 0.25 * torch.nn.functional.interpolate(t, scale_factor=2, mode="nearest")      # noqa: E731
            gr, bb = gr + up(grad), bb + up(bg)
        grad, bg = gr, bb + u * gr.abs()
    g0 = abs(float(np.float32(g)))
    return dict(loss=b_loss.detach(), coef=b_coef, g_a=g0 * (bg + u * grad.abs()), closed_form_grad=float(np.float32(g)) * grad,
                smallest_contrast=min(float(x) for x in mc[:4]), smallest_ms4=float(ms[4]))
