"""Float64 references, derived bounds, inputs, case tables and block tables for the fused Adam kernels of csrc/pointwise.hip
(adam_kernel, grad_sqnorm_kernel, adam_clip_kernel, adam_blocks_kernel, adam_mark_members_kernel).  No GPU, no native import:
tests/test_adam_reference_host.py pins the references to torch and sizes the bounds, tests/test_adam_ops_gpu.py holds the kernels
to them.

The references follow the torch definition (clip_grad_norm_ / clip_grad_value_ + torch.optim.Adam, no amsgrad) of ONE launch,
on the fp32 buffers and the fp32 state head widened to float64.  The chain is closed output by output: the moments from the
inputs, the parameter from the moments the kernel RETURNED, the clip factor from the norm the kernel REPORTED.  So each bound
covers the roundings of one short expression.  The only stated difference to torch is beta^t: the kernel keeps it as a running
fp32 product (it stores it back), and param_ref takes exactly that fl32(state[6] * b1), fl32(state[7] * b2).

Bounds: gamma(k) * sum |terms| with gamma(k) = k u / (1 - k u), u = 2^-24, k the number of fp32 roundings on the longest path
of the kernel's expression (the larger count where the 16-byte loop, the scalar loop and the blocks kernel differ in fusing),
plus the propagated bound of its rounded inputs.  Counts, from the code:
  g'   off / value: fl(g * gs), fl(wd * p), fl(sum)                                   3   (fused forms: 2)
       norm: fl(g * gs), fl(. * c), fl(wd * p), fl(sum)                               4   (fused forms: 3)
             + 4u |g gs c| for c itself: add, reciprocal, multiply (3) and one to spare for a reciprocal that is not
               correctly rounded
  m'   fl(1 - b1), fl(. * g'), fl(b1 * m), fl(sum)                                    4   + (1 - b1) bg
  v'   fl(1 - b2), fl(. * g'), fl(. * g'), fl(b2 * v), fl(sum)                        5   + (1 - b2) (2 |g'| bg + bg^2)
  p'   bc1, lr / bc1, bc2, sqrt(bc2), sqrt(v'), . / bc2s, . + eps, m' / ., step * .   9, and 1 more for square roots that are
       faithfully instead of correctly rounded: 10 on |p' - p|, + u |p'| for the final rounding (rigorous, and the largest term)
  norm all terms positive: relative L u / 2 + u (the square root halves the sum's error and rounds once), L = norm_roundings(n)
Worst |err| / bound of the host test (fp32 numpy emulation, unfused and fused, all 64 SMALL_CASES and one 200 001-element case):
m' 0.48, v' 0.53, p' 0.999 (the final-rounding term, which is rigorous), norm 0.10; g' is internal.  The kernels on the MI355X, all
cases of test_adam_ops_gpu.py: m' 0.49, v' 0.56, p' 0.9994, norm 0.10.  Bound / scale at most 9.3e-7 (m'), 1.6e-6 (v'), 5.9e-4
(p', against the case's largest step).  Against the element's OWN step the arithmetic part of the p' bound is within 1e-3 on every
element, and the whole bound on every element whose step is at least 2^-13 |p'|; below that half an ulp of p' alone is more than
0.5e-3 of the step (0.7 % of the elements have no step at all, 9.3 % a smaller one: test_bound_sizes_and_input_conditions).
"""
import dataclasses
import math

import numpy as np

U = 2.0 ** -24
F32_MIN_NORMAL = float(np.finfo(np.float32).tiny)
f32 = np.float32

# ---- restated from pointwise.hip ----------------------------------------------------------------------------------------------
TICKET_OFFSET = 16
ADAM_MAX_WGS = 2048
STATE_FLOATS = TICKET_OFFSET + 16 * (1 + ADAM_MAX_WGS // 32)
WGS = 1024                       # launch_adam / launch_adam_clipped / launch_adam_blocks
CLIP_MAX_WGS = 1024              # grad_sqnorm_kernel's workgroups = the clip workspace's floats
CLIP_NORM, CLIP_VALUE, CLIP_OFF = 0, 1, 2


def grid_for(n, cap):
    return int(max(1, min(cap, (n + 255) // 256)))


def step_grid(n, vec):
    """Workgroups of adam_kernel / adam_clip_kernel: over quads when all four buffers are 16-byte aligned, over floats otherwise."""
    return grid_for(n // 4 if vec else n, WGS)


def norm_parts(n):
    return grid_for(n // 4, CLIP_MAX_WGS)


def blocks_geometry(n):
    """launch_adam_blocks / adam_blocks_kernel: quads (the last may be partial), grid, quads per workgroup, the first workgroup
    whose range is empty (grid when none is)."""
    nq = (n + 3) // 4
    grid = grid_for(nq, WGS)
    qper = (nq + grid - 1) // grid
    first_empty = min(grid, (nq + qper - 1) // qper)
    return dict(nq=nq, grid=grid, qper=qper, first_empty=first_empty)


def blocks_threads_with(n, wg, k):
    """Threads of workgroup wg whose k-th quad (k = 0: qa of the first pass, 1: qb, 2: qa of the second pass) exists."""
    ge = blocks_geometry(n)
    q0 = wg * ge["qper"]
    q1 = min(q0 + ge["qper"], ge["nq"])
    return max(0, min(256, q1 - q0 - 256 * k))


def norm_roundings(n):
    """Roundings on the longest path of the norm's sum: the thread's fma chain over its quads (two quads of 4 per pass) and the tail
    element, the product g * gs (relative u on x, 2u on x^2), 6 butterfly steps, 2 wave adds; in the consumer the strided sum of
    the partials, 6 butterfly steps, 2 wave adds."""
    nq, parts = n // 4, norm_parts(n)
    chain = 8 * max(1, -(-nq // (2 * 256 * parts))) + 1
    return chain + 2 + 6 + 2 + -(-parts // 256) + 6 + 2


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- case tables ---------------------------------------------------------------------------------------------------------------
HYPERS = [dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2),
          dict(lr=5e-4, b1=0.5, b2=0.9, eps=1e-3, wd=0.0),
          dict(lr=3e-3, b1=0.0, b2=0.999, eps=1e-8, wd=0.1)]
T0S = [0, 1, 6, 999]
GRAD_SCALES = [1.0, 0.5, 1.0 / 3.0]
OFFSETS = {"aligned": (0, 0, 0, 0), "shifted": (1, 1, 1, 1), "g_only": (0, 1, 0, 0), "pmv_only": (1, 0, 1, 1)}   # p, g, m, v
MODES = ["off", "value", "norm_active", "norm_inactive"]
ALGORITHM = {"off": CLIP_OFF, "value": CLIP_VALUE, "norm_active": CLIP_NORM, "norm_inactive": CLIP_NORM}

# n -> (size class, scalar grid, 16-byte grid, blocks grid)
SIZES = {1: ("tail", 1, 1, 1), 3: ("tail", 1, 1, 1), 4: ("tail", 1, 1, 1), 5: ("tail", 1, 1, 1), 7: ("tail", 1, 1, 1),
         1023: ("tail", 4, 1, 1),
         256 * 31 + 1: ("groups", 32, 8, 8),
         256 * 32 + 1: ("groups", 33, 8, 9),
         4 * 256 * 32 + 7: ("groups", 129, 33, 33),
         256 * 63 + 5: ("groups", 64, 16, 16),
         256 * 64 + 5: ("groups", 65, 17, 17),
         300001: ("cap", 1024, 293, 293)}
N_EMPTY = 4 * (1024 * 256 + 1) - 3          # 1 048 577: blocks workgroups 1021..1023 own nothing
N_TWO = 4 * (1024 * 515 - 9) - 2            # 2 109 402: every blocks thread has a second quad
# ticket grids: n whose launch has 1, 32, 33, 64, 65, 1024 workgroups -- the plain kernels on their scalar grid (buffers shifted
# by one float), the blocks kernel on its quad grid
TICKET_SCALAR = {1: 1, 256 * 31 + 1: 32, 256 * 32 + 1: 33, 256 * 63 + 5: 64, 256 * 64 + 5: 65, 300001: 1024}
TICKET_BLOCKS = {1023: 1, 4 * 256 * 31 + 7: 32, 4 * 256 * 32 + 7: 33, 4 * 256 * 63 + 5: 64, 4 * 256 * 64 + 5: 65, N_EMPTY: 1024}


def check_geometry():
    """The size tables against the launch arithmetic restated above: a change of the launch geometry fails here."""
    for n, (_, gs, gv, gb) in SIZES.items():
        assert (step_grid(n, False), step_grid(n, True), blocks_geometry(n)["grid"]) == (gs, gv, gb), n
    assert {n % 4 for n in (1, 3, 4, 5, 7, 1023)} == {0, 1, 3} and N_TWO % 4 == 2      # every n % 4, below and above one quad
    for n, grid in TICKET_SCALAR.items():
        assert step_grid(n, False) == grid, n
    for n, grid in TICKET_BLOCKS.items():
        assert blocks_geometry(n)["grid"] == grid, n
    assert 300001 > 1024 * 256 and 300001 < 2 * 1024 * 256            # the strided scalar loop: some threads take two floats
    ge = blocks_geometry(N_EMPTY)
    assert ge == dict(nq=262145, grid=1024, qper=257, first_empty=1021) and N_EMPTY == 1048577
    assert blocks_threads_with(N_EMPTY, 0, 1) == 1 and blocks_threads_with(N_EMPTY, 1020, 0) == 5
    assert all(blocks_threads_with(N_EMPTY, w, 0) == 0 for w in (1021, 1022, 1023))
    ge = blocks_geometry(N_TWO)
    assert ge == dict(nq=527351, grid=1024, qper=515, first_empty=1024) and N_TWO == 2109402 and N_TWO % 4 == 2
    assert blocks_threads_with(N_TWO, 0, 1) == 256 and blocks_threads_with(N_TWO, 0, 2) == 3
    assert blocks_threads_with(N_TWO, 1023, 1) == 527351 - 1023 * 515 - 256 and blocks_threads_with(N_TWO, 1022, 1) == 256
    assert norm_parts(N_TWO) == 1024 and norm_parts(1023) == 1 and norm_parts(4 * 256 * 32 + 7) == 33
    assert STATE_FLOATS == 1056


@dataclasses.dataclass(frozen=True)
class Case:
    n: int
    hyper: int = 0
    t0: int = 0
    gs: float = 1.0
    mode: str = "off"
    offset: str = "aligned"
    seed: int = 0

    @property
    def id(self):
        return f"n{self.n}-h{self.hyper}-t{self.t0}-gs{self.gs:.3g}-{self.mode}-{self.offset}"


def step_cases():
    """Every (offset, mode, size class) triple, and every value of every other axis at least once: the hyper set, the starting
    step and grad_scale cycle with different periods over the list."""
    reps = {"tail": [1, 3, 4, 5, 7, 1023], "groups": [256 * 31 + 1, 256 * 32 + 1, 4 * 256 * 32 + 7, 256 * 63 + 5, 256 * 64 + 5],
            "cap": [300001]}
    out, k = [], 0
    for cls, ns in reps.items():
        for off in OFFSETS:
            for mode in MODES:
                # the triple on one size of the class in rotation, so that every size meets every offset and several modes
                for n in ([ns[k % len(ns)]] if cls != "tail" else [ns[k % len(ns)], ns[(k + 3) % len(ns)]]):
                    out.append(Case(n, k % 3, T0S[(k // 3) % 4], GRAD_SCALES[(k // 2) % 3], mode, off, seed=k))
                    k += 1
    return out


SMALL_CASES = step_cases()


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def head_at(hyper, t):
    """The fp32 state head after t steps: the powers by repeated fp32 multiplication, as the device forms them."""
    h = HYPERS[hyper] if isinstance(hyper, int) else hyper
    b1, b2 = f32(h["b1"]), f32(h["b2"])
    p1, p2 = f32(1), f32(1)
    for _ in range(int(t)):
        p1, p2 = f32(p1 * b1), f32(p2 * b2)
    return np.array([t, h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], p1, p2], dtype=np.float32)


def _value_anchor(gs):
    """A gradient whose fp32 product with grad_scale IS the value-mode clip."""
    g0 = f32(0.15)
    return g0, f32(g0 * f32(gs))


def adam_inputs(case, t_elem=None):
    """p, g, m, v (fp32), the state head, the clip value and the float64 norm of g * grad_scale for a Case.  t_elem: per-element
    starting step (block tables); None: case.t0 everywhere."""
    rng = np.random.default_rng(1000 + case.seed)
    n, h, gs = case.n, HYPERS[case.hyper], f32(case.gs)
    head = head_at(case.hyper, case.t0)
    b1, b2, wd = (float(head[i]) for i in (2, 3, 5))
    p = (0.3 * rng.standard_normal(n)).astype(np.float32)
    mag = 10.0 ** rng.uniform(-6.0, 1.0, n)
    g = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * mag).astype(np.float32)
    zeros = np.zeros(n, dtype=bool)
    if n > 1:
        zeros[5 % n::17] = True                                        # a fixed share of exact zeros
        zeros[0] = False
    if n >= 64:
        zeros[n // 2:n // 2 + 8] = True                                # one run of 8 consecutive zeros
    g[zeros] = 0.0
    clip = f32(1.0)
    if case.mode == "value":
        g0, clip = _value_anchor(gs)
        if n >= 64:
            g[[3, 40]] = g0
            g[[7, 41]] = -g0
    t = np.full(n, case.t0) if t_elem is None else np.asarray(t_elem)
    gp = 10.0 ** rng.uniform(-4.0, 1.0, n)
    v = np.where(t > 0, (1.0 - b2) * gp * gp, 0.0).astype(np.float32)
    m = np.where(t > 0, 0.5 * rng.standard_normal(n) * np.sqrt(v), 0.0).astype(np.float32)
    thr = math.sqrt(1e-15 / (1.0 - b2))
    for _ in range(20):                                                # the denormal condition: redraw what falls below it
        norm = float(np.sqrt(np.sum((g.astype(np.float64) * float(gs)) ** 2)))
        if case.mode == "norm_active":
            clip = f32(0.5 * norm)
        elif case.mode == "norm_inactive":
            clip = f32(1e30)
        c = float(coef_ref(f32(norm), clip)) if case.mode.startswith("norm") else 1.0
        gq = grad_ref(p, g, gs, wd, case.mode, clip, c)
        bad = (gq != 0) & ((1.0 - b2) * gq * gq < 1.01e-15)
        if not bad.any():
            break
        k = int(bad.sum())
        sign = np.where(g[bad] < 0, -1.0, 1.0) * np.where(g[bad] == 0, 0.0, 1.0)
        g[bad] = (sign * 2.0 * thr / (float(gs) * min(c, 1.0)) * 10.0 ** rng.uniform(0.0, 1.0, k)).astype(np.float32)
        p[bad & (g == 0)] = f32(0.3)                                   # an exact-zero gradient with a tiny wd * p
    return dict(p=p, g=g, m=m, v=v, head=head, gs=gs, clip=clip, norm=norm, mode=case.mode, n=n)


# ---- float64 references ----------------------------------------------------------------------------------------------------------
def _w(x):
    return np.asarray(x, dtype=np.float64)


def norm_ref(g, gs):
    return float(np.sqrt(np.sum((_w(g) * float(gs)) ** 2)))


def coef_ref(total32, clip):
    """min(1, clip / (total + 1e-6)) from the norm the kernel reported; NaN stays NaN, an infinite norm gives 0."""
    t = float(total32)
    if math.isnan(t):
        return float("nan")
    return min(1.0, float(clip) / (t + 1e-6))


def grad_ref(p, g, gs, wd, mode, clip=None, c=1.0):
    x = _w(g) * float(gs)
    if mode == "value":
        cl = float(clip)
        with np.errstate(invalid="ignore"):
            x = np.where(x < -cl, -cl, np.where(x > cl, cl, x))        # NaN stays NaN, +-inf clamps
    elif mode.startswith("norm"):
        x = x * float(c)
    return x + float(wd) * _w(p)


def moments_ref(gq, m, v, b1, b2):
    b1, b2 = float(b1), float(b2)
    return b1 * _w(m) + (1.0 - b1) * gq, b2 * _w(v) + (1.0 - b2) * gq * gq


def beta_powers(s6, s7, b1, b2):
    """This step's beta^t as the kernel holds and stores them: the fp32 product."""
    return np.asarray(s6, dtype=np.float32) * f32(b1), np.asarray(s7, dtype=np.float32) * f32(b2)


def param_ref(p, m1, v1, lr, eps, b1t, b2t):
    """p' from the moments the kernel returned; b1t, b2t fp32 (scalars or per element), everything after them float64."""
    b1t, b2t = _w(b1t), _w(b2t)
    upd = float(lr) / (1.0 - b1t) * _w(m1) / (np.sqrt(_w(v1)) / np.sqrt(1.0 - b2t) + float(eps))
    return _w(p) - upd, upd


def grad_bound(p, g, gs, wd, mode, c=1.0, clip=None):
    a = np.abs(_w(g) * float(gs))
    if mode.startswith("norm"):
        a = a * abs(float(c))
        return gamma(4) * (a + np.abs(float(wd) * _w(p))) + 4 * U * a
    if mode == "value":        # a product beyond +-clip rounds to one beyond or at it (clip is fp32) and clamps to clip exactly
        a = np.minimum(a, abs(float(clip)))
    return gamma(3) * (a + np.abs(float(wd) * _w(p)))


def moment_bounds(gq, bg, m, v, b1, b2):
    b1, b2 = float(b1), float(b2)
    bm = gamma(4) * (np.abs(b1 * _w(m)) + np.abs((1.0 - b1) * gq)) + (1.0 - b1) * bg
    bv = gamma(5) * (np.abs(b2 * _w(v)) + (1.0 - b2) * gq * gq) + (1.0 - b2) * (2.0 * np.abs(gq) * bg + bg * bg)
    return bm, bv


def param_bound(p_ref, upd):
    return gamma(10) * np.abs(upd) + U * np.abs(p_ref)


def norm_bound(n):
    """Relative."""
    return gamma(norm_roundings(n)) / 2.0 + U


def state_ref(head):
    """The head after one launch of any of the three kernels."""
    out = np.array(head[:8], dtype=np.float32)
    out[0] = f32(out[0] + f32(1))
    out[6], out[7] = beta_powers(head[6], head[7], head[2], head[3])
    return out


def bstate_rows(hyper, counters):
    """Block-state rows {step, beta1^step, beta2^step, seen} for the given counters."""
    cache = {int(t): head_at(hyper, int(t)) for t in set(int(c) for c in counters)}
    return np.array([[t, cache[int(t)][6], cache[int(t)][7], 1.0 if t > 0 else 0.0] for t in counters], dtype=np.float32)


def bstate_ref(rows, active, b1, b2):
    out = np.array(rows, dtype=np.float32)
    a = np.asarray(active) != 0
    out[a, 0] = out[a, 0] + f32(1)
    out[a, 1] = out[a, 1] * f32(b1)
    out[a, 2] = out[a, 2] * f32(b2)
    out[a, 3] = 1.0
    return out


def check_step(inp, out, elem=None, b1t=None, b2t=None):
    """One launch's outputs against the references.  out: m, v, p (fp32) and norm (fp32 or None) as returned.  elem: boolean
    mask of the elements that step (None: all); b1t / b2t: per-element fp32 powers of this step (None: from the head).
    Returns {output: (worst |err| / bound, number of elements beyond the bound, the bound, the reference)}."""
    head, mode = inp["head"], inp["mode"]
    lr, b1, b2, eps, wd = (float(head[i]) for i in range(1, 6))
    sel = slice(None) if elem is None else elem
    p, g, m, v = (inp[k][sel] for k in "pgmv")
    res = {}
    c = 1.0
    if mode.startswith("norm"):
        nb = norm_bound(inp["n"]) * inp["norm"]
        err = abs(float(out["norm"]) - inp["norm"])
        res["norm"] = (err / nb if nb > 0 else float(err > 0), int(not err <= nb), nb, inp["norm"])
        c = coef_ref(out["norm"], inp["clip"])
    gq = grad_ref(p, g, inp["gs"], wd, mode, inp["clip"], c)
    bg = grad_bound(p, g, inp["gs"], wd, mode, c, inp["clip"])
    m_ref, v_ref = moments_ref(gq, m, v, b1, b2)
    bm, bv = moment_bounds(gq, bg, m, v, b1, b2)
    if b1t is None:
        b1t, b2t = beta_powers(head[6], head[7], head[2], head[3])
    else:
        b1t, b2t = b1t[sel], b2t[sel]
    p_ref, upd = param_ref(p, out["m"][sel], out["v"][sel], lr, eps, b1t, b2t)
    bp = param_bound(p_ref, upd)
    for name, got, ref, bound in (("m", out["m"][sel], m_ref, bm), ("v", out["v"][sel], v_ref, bv), ("p", out["p"][sel], p_ref, bp)):
        err = np.abs(_w(got) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        bad = ~(err <= bound)                                           # a NaN fails
        res[name] = (float(np.max(ratio)) if ratio.size else 0.0, int(bad.sum()), bound, ref)
    return res


# ---- fp32 emulation of the documented update (and wrong variants of it) ----------------------------------------------------------
def _fma(a, b, c):
    return (_w(a) * _w(b) + _w(c)).astype(np.float32)


WRONG = ["prev_bias", "eps_in_sqrt", "no_sqrt_bc2", "old_v", "wd_before_clip", "no_grad_scale", "decoupled_wd",
         "clamp_before_scale", "c_not_clamped"]


def emulate(inp, fused=False, wrong=None):
    """The update in numpy fp32, operation by operation.  fused: the fused operations the kernel comments name (fma(g, gs, wd p)
    / fma(g gs, c, wd p), fma(b, m, .), fma(-step, q, p)).  wrong: one of WRONG."""
    head, mode = inp["head"], inp["mode"]
    lr, b1, b2, eps, wd = (f32(head[i]) for i in range(1, 6))
    one = f32(1)
    p, g, m, v, gs, clip = inp["p"], inp["g"], inp["m"], inp["v"], f32(inp["gs"]), f32(inp["clip"])
    if wrong == "no_grad_scale":
        gs = one
    norm, c = None, one
    with np.errstate(all="ignore"):
        if mode.startswith("norm"):
            x = g * gs
            norm = f32(np.sqrt(np.sum((x * x).astype(np.float32), dtype=np.float32)))
            c = f32(f32(one / f32(norm + f32(1e-6))) * clip)
            if wrong != "c_not_clamped":
                c = one if c > one else c
        wdp = wd * p
        if wrong == "decoupled_wd":
            wdp = wdp * f32(0)
        if mode == "value":
            x = np.clip(g, -clip, clip) * gs if wrong == "clamp_before_scale" else g * gs
            if wrong == "wd_before_clip":
                gq = np.clip(x + wdp, -clip, clip)
            else:
                x = np.clip(x, -clip, clip)
                gq = _fma(wd, p, x) if fused and wrong != "decoupled_wd" else x + wdp
        elif mode.startswith("norm"):
            if wrong == "wd_before_clip":
                gq = (g * gs + wdp) * c
            else:
                gq = _fma(g * gs, c, wdp) if fused else (g * gs) * c + wdp
        else:
            gq = _fma(g, gs, wdp) if fused else g * gs + wdp
        gs1, gs2 = (one - b1) * gq, ((one - b2) * gq) * gq
        m1 = _fma(b1, m, gs1) if fused else b1 * m + gs1
        v1 = _fma(b2, v, gs2) if fused else b2 * v + gs2
        b1t, b2t = (f32(head[6]), f32(head[7])) if wrong == "prev_bias" else beta_powers(head[6], head[7], b1, b2)
        step = lr / (one - b1t)
        bc2s = one if wrong == "no_sqrt_bc2" else np.sqrt(one - b2t)
        vv = v if wrong == "old_v" else v1
        den = np.sqrt(vv / (bc2s * bc2s) + eps) if wrong == "eps_in_sqrt" else np.sqrt(vv) / bc2s + eps
        q = m1 / den
        p1 = _fma(-step, q, p) if fused else p - step * q
        if wrong == "decoupled_wd":
            p1 = (p1 - lr * wd * p).astype(np.float32)
    return dict(m=m1.astype(np.float32), v=v1.astype(np.float32), p=p1.astype(np.float32), norm=norm)


# ---- block tables ----------------------------------------------------------------------------------------------------------------
BLOCK_SIZES = [1, 2, 3, 4, 5, 7, 17, 64, 1023, 4096, 8192]
BLOCK_GAPS = [0, 0, 1, 2, 3, 4, 9]
COUNTERS = [0, 1, 6, 999]
TABLE_STYLES = ["dense", "edges", "one", "first_gap"]


def valid_table(ranges, n):
    """AdamBlockTable's own rule, restated (the host test runs the class itself on every table)."""
    prev = 0
    for lo, hi in ranges:
        if not prev <= lo < hi <= n:
            return False
        prev = hi
    return bool(ranges) and n < 2 ** 31


def make_table(n, seed, style):
    """Sorted, disjoint [lo, hi) ranges over n floats."""
    rng = np.random.default_rng(7000 + seed)
    if style == "one":
        return [(0, n)]
    if style == "first_gap":
        cuts = [5] + sorted(set(int(x) for x in rng.integers(6, max(7, n), 6))) + [n]
        return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if a < b]
    if style == "dense":
        sizes = [s for s in BLOCK_SIZES if s <= max(4, n // 16)]
        out, pos = [], 0
        while True:
            if rng.random() < 1.0 / 16.0 and pos + 8 <= n:              # four blocks of one float in one quad
                pos = (pos + 3) // 4 * 4
                out.extend((pos + k, pos + k + 1) for k in range(4))
                pos += 4
            pos += int(rng.choice(BLOCK_GAPS))
            hi = pos + int(rng.choice(sizes))
            if hi > n:
                break
            out.append((pos, hi))
            pos = hi
        return out
    assert style == "edges"
    ge = blocks_geometry(n)
    cuts = {0, n // 2 - 1, n // 2, n // 2 + 1}
    for wg in sorted({1, 2, ge["grid"] // 2, ge["first_empty"] - 1, ge["grid"] - 1}):
        q0 = wg * ge["qper"]
        for b in (4 * q0, 4 * (q0 + 256), 4 * (q0 + 512)):
            cuts.update((b - 1, b, b + 1))
    end = n - seed % 4                                                   # the last block ends at n, or 1..3 floats before it
    cuts = sorted(c for c in cuts if 0 <= c < end) + [end]
    out = [(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    drop = set(range(4, len(out) - 1, 5))                               # every fifth range becomes a gap (whole quads inside)
    return [r for k, r in enumerate(out) if k not in drop]


def make_activity(nb, seed, kind):
    if kind == "all":
        return np.ones(nb, dtype=np.int32)
    if kind == "none":
        return np.zeros(nb, dtype=np.int32)
    return (np.random.default_rng(8000 + seed).random(nb) < 0.5).astype(np.int32)


def make_counters(nb, seed, equal=None):
    if equal is not None:
        return np.full(nb, equal, dtype=np.int64)
    return np.random.default_rng(9000 + seed).choice(COUNTERS, nb)


def block_of(n, ranges):
    """Per element: the index of its block, -1 in a gap."""
    lo = np.array([r[0] for r in ranges], dtype=np.int64)
    hi = np.array([r[1] for r in ranges], dtype=np.int64)
    e = np.arange(n, dtype=np.int64)
    k = np.searchsorted(hi, e, side="right")
    inside = (k < len(ranges)) & (lo[np.minimum(k, len(ranges) - 1)] <= e)
    return np.where(inside, k, -1)


def block_inputs(case, ranges, act, cnt):
    """adam_inputs under a block table: per-block starting steps, zero gradient in gaps and inactive blocks."""
    blk = block_of(case.n, ranges)
    inp = adam_inputs(case, np.where(blk >= 0, cnt[np.maximum(blk, 0)], 0))
    still = (blk < 0) | (act[np.maximum(blk, 0)] == 0)
    inp["g"][still] = 0.0
    inp["norm"] = norm_ref(inp["g"], inp["gs"])
    if case.mode == "norm_active":
        inp["clip"] = np.float32(0.5 * inp["norm"]) if inp["norm"] > 0 else np.float32(1.0)
    return inp


def table_stats(n, ranges):
    """What the table exercises: blocks, the most blocks inside one quad, gaps that hold a whole quad, boundaries off a multiple of 4."""
    blk = block_of(n, ranges)
    nq = n // 4
    quads = blk[:4 * nq].reshape(nq, 4)
    first = np.concatenate([np.ones((nq, 1), dtype=bool), np.diff(quads, axis=1) != 0], axis=1)       # blocks ascend along a quad
    per_quad = (first & (quads >= 0)).sum(axis=1)                       # distinct block indices, gaps not counted
    return dict(nb=len(ranges), max_blocks_in_quad=int(per_quad.max()) if nq else 0,
                whole_gap_quads=int((quads == -1).all(axis=1).sum()) if nq else 0,
                odd_boundaries=sum(1 for lo, hi in ranges if lo % 4 or hi % 4))
