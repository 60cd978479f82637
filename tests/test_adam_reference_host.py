"""CPU: the float64 references of tests/adam_checks.py pinned to torch (clip_grad_norm_ / clip_grad_value_ + torch.optim.Adam in
float64), their bounds sized against an fp32 emulation and against deliberately wrong variants of the update, the input
conditions, the block tables and the launch geometry the size tables rely on.  tests/test_adam_ops_gpu.py holds the kernels to
the same references and bounds.  Run with -s to see the ratios."""
import numpy as np
import pytest
import torch

from tests import adam_checks as V

HOST_CASES = V.SMALL_CASES
LARGE = V.Case(200001, 0, 6, 1.0 / 3.0, "norm_active", seed=77)


def _torch_step(inp, ranges=None, active=None, counters=None):
    """One torch step in float64 over one tensor per block (None: one tensor); returns p, m, v over the n floats and the norm."""
    head = inp["head"]
    lr, b1, b2, eps, wd = (float(head[i]) for i in range(1, 6))
    n = inp["n"]
    ranges = [(0, n)] if ranges is None else ranges
    active = [1] * len(ranges) if active is None else active
    counters = [int(head[0])] * len(ranges) if counters is None else counters
    t = {k: torch.from_numpy(inp[k].astype(np.float64)) for k in "pgmv"}
    params = [torch.nn.Parameter(t["p"][lo:hi].clone()) for lo, hi in ranges]
    opt = torch.optim.Adam(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for q, (lo, hi), a, c in zip(params, ranges, active, counters):
        opt.state[q] = dict(step=torch.tensor(float(c), dtype=torch.float64), exp_avg=t["m"][lo:hi].clone(), exp_avg_sq=t["v"][lo:hi].clone())
        q.grad = (t["g"][lo:hi] * float(inp["gs"])).clone() if a else None
    norm = None
    if inp["mode"].startswith("norm"):
        norm = float(torch.nn.utils.clip_grad_norm_(params, float(inp["clip"])))
    elif inp["mode"] == "value":
        torch.nn.utils.clip_grad_value_(params, float(inp["clip"]))
    opt.step()
    out = {k: inp[k].astype(np.float64) for k in "pmv"}
    for q, (lo, hi) in zip(params, ranges):
        out["p"][lo:hi] = q.detach().numpy()
        out["m"][lo:hi] = opt.state[q]["exp_avg"].numpy()
        out["v"][lo:hi] = opt.state[q]["exp_avg_sq"].numpy()
    return out, norm


def _reference(inp, t_next, blk=None, act=None):
    """The references chained in float64, with the exact beta^t torch uses (t_next: scalar or per element)."""
    head = inp["head"]
    lr, b1, b2, eps, wd = (float(head[i]) for i in range(1, 6))
    c = V.coef_ref(inp["norm"], inp["clip"]) if inp["mode"].startswith("norm") else 1.0
    gq = V.grad_ref(inp["p"], inp["g"], inp["gs"], wd, inp["mode"], inp["clip"], c)
    m1, v1 = V.moments_ref(gq, inp["m"], inp["v"], b1, b2)
    t_next = np.asarray(t_next, dtype=np.float64)
    p1, _ = V.param_ref(inp["p"], m1, v1, lr, eps, b1 ** t_next, b2 ** t_next)
    out = dict(p=p1, m=m1, v=v1)
    if blk is not None:
        still = (blk < 0) | (np.asarray(act)[np.maximum(blk, 0)] == 0)
        for k in "pmv":
            out[k] = np.where(still, inp[k].astype(np.float64), out[k])
    return out


def _close(a, b, what):
    err = np.abs(a - b)
    assert np.all(err <= 1e-12 * (1.0 + np.abs(b))), (what, float(err.max()))


def test_geometry_of_the_size_tables():
    V.check_geometry()
    triples = {(c.offset, c.mode, V.SIZES[c.n][0]) for c in V.SMALL_CASES}
    assert len(triples) == len(V.OFFSETS) * len(V.MODES) * 3
    assert {c.n for c in V.SMALL_CASES} == set(V.SIZES)
    assert {c.hyper for c in V.SMALL_CASES} == {0, 1, 2} and {c.t0 for c in V.SMALL_CASES} == set(V.T0S)
    assert {c.gs for c in V.SMALL_CASES} == set(V.GRAD_SCALES)
    print(f"{len(V.SMALL_CASES)} step cases")


@pytest.mark.parametrize("case", [c for c in HOST_CASES if c.offset == "aligned"], ids=lambda c: c.id)
def test_references_match_torch(case):
    inp = V.adam_inputs(case)
    want, norm = _torch_step(inp)
    got = _reference(inp, case.t0 + 1)
    for k in "pmv":
        _close(got[k], want[k], k)
    if norm is not None:
        assert abs(norm - V.norm_ref(inp["g"], inp["gs"])) <= 1e-12 * norm


@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("style", V.TABLE_STYLES)
def test_block_references_match_torch_per_block(style, mode):
    n = 1023
    ranges = V.make_table(n, 3, style)
    act, cnt = V.make_activity(len(ranges), 3, "all" if style == "one" else "half"), V.make_counters(len(ranges), 3)
    blk = V.block_of(n, ranges)
    inp = V.block_inputs(V.Case(n, 0, 0, 0.5, mode, seed=5), ranges, act, cnt)
    want, norm = _torch_step(inp, ranges, act, cnt)
    got = _reference(inp, np.where(blk >= 0, cnt[np.maximum(blk, 0)], 0) + 1, blk, act)
    for k in "pmv":
        _close(got[k], want[k], k)
    if norm is not None and act.any():
        assert abs(norm - inp["norm"]) <= 1e-12 * norm


def test_fp32_beta_powers_against_exact_ones():
    worst = 0.0
    for h in range(3):
        for t0 in V.T0S:
            head = V.head_at(h, t0)
            b1t, b2t = V.beta_powers(head[6], head[7], head[2], head[3])
            for bt, b in ((b1t, float(head[2])), (b2t, float(head[3]))):
                exact = 1.0 - b ** (t0 + 1)
                worst = max(worst, abs((1.0 - float(bt)) - exact) / exact)
    print(f"largest relative gap of 1 - beta^t between the fp32 product and float64 over the tabled steps: {worst:.3e}")
    assert worst <= 1001 * V.U / (1.0 - 0.999)          # t roundings of beta^t <= 1, against 1 - beta^t >= 1 - b2


def _emulation_ratios(cases):
    worst = {}
    for case in cases:
        inp = V.adam_inputs(case)
        for fused in (False, True):
            res = V.check_step(inp, V.emulate(inp, fused))
            for k, (ratio, bad, _, _) in res.items():
                assert bad == 0, (case.id, fused, k, ratio, bad)
                worst[k] = max(worst.get(k, 0.0), ratio)
    return worst


def test_bounds_hold_for_the_fp32_emulation():
    worst = _emulation_ratios(HOST_CASES + [LARGE])
    for k, r in sorted(worst.items()):
        print(f"emulation / bound, worst over {len(HOST_CASES) + 1} cases x (unfused, fused): {k}: {r:.4f}")
    assert set(worst) == {"m", "v", "p", "norm"}


WRONG_CASES = {"prev_bias": V.Case(1023, 0, 1, 1.0, "off", seed=1), "eps_in_sqrt": V.Case(1023, 0, 0, 1.0, "off", seed=2),
               "no_sqrt_bc2": V.Case(1023, 0, 6, 1.0, "off", seed=3), "old_v": V.Case(1023, 0, 6, 1.0, "off", seed=4),
               "wd_before_clip": V.Case(1023, 2, 6, 1.0, "value", seed=5), "no_grad_scale": V.Case(1023, 0, 6, 0.5, "off", seed=6),
               "decoupled_wd": V.Case(1023, 2, 6, 1.0, "off", seed=7), "clamp_before_scale": V.Case(1023, 0, 6, 0.5, "value", seed=8),
               "c_not_clamped": V.Case(1023, 0, 6, 1.0, "norm_inactive", seed=9)}


@pytest.mark.parametrize("wrong", V.WRONG)
def test_wrong_variants_leave_the_bounds(wrong):
    case = WRONG_CASES[wrong]
    inp = V.adam_inputs(case)
    caught = {}
    for fused in (False, True):
        res = V.check_step(inp, V.emulate(inp, fused, wrong))
        for k, (_, bad, _, _) in res.items():
            caught[k] = max(caught.get(k, 0), bad)
    print(f"{wrong}: caught on " + ", ".join(f"{k}: {100.0 * b / case.n:.1f} %" for k, b in caught.items() if k != "norm" and b))
    assert any(b > 0 for b in caught.values()), f"{wrong} stays inside every bound"
    also = V.check_step(inp, V.emulate(inp, False))
    assert all(bad == 0 for _, bad, _, _ in also.values())          # the right update passes on the same case


def test_bound_sizes_and_input_conditions():
    worst = dict(p=0.0, m=0.0, v=0.0)
    elementwise = [0, 0, 0]
    for case in HOST_CASES + [LARGE]:
        inp = V.adam_inputs(case)
        head = inp["head"]
        b2, wd = float(head[3]), float(head[5])
        c = V.coef_ref(np.float32(inp["norm"]), inp["clip"]) if case.mode.startswith("norm") else 1.0
        gq = V.grad_ref(inp["p"], inp["g"], inp["gs"], wd, case.mode, inp["clip"], c)
        term = (1.0 - b2) * gq * gq
        assert np.all((term == 0) | (term >= 1e-15)), case.id                       # no result hangs on fp32 denormals
        assert np.all((inp["v"] == 0) | (inp["v"] >= 1e-15)) and np.all(inp["v"] >= 0)
        if case.n > 17:
            assert (inp["g"] == 0).any()
        if case.n >= 64:
            z = inp["g"] == 0
            assert np.convolve(z.astype(int), np.ones(8, dtype=int), "valid").max() == 8
        x = inp["g"].astype(np.float64) * float(inp["gs"])
        if case.mode == "norm_active":
            assert inp["norm"] > float(inp["clip"]) and c < 1.0
        if case.mode == "norm_inactive":
            assert c == 1.0
        if case.mode == "value" and case.n >= 64:
            cl = float(inp["clip"])
            assert (np.abs(x) < cl).any() and (x > cl).any() and (x < -cl).any()
            xr = (inp["g"] * inp["gs"]).astype(np.float32)
            assert (xr == inp["clip"]).sum() >= 2 and (xr == -inp["clip"]).sum() >= 2
        res = V.check_step(inp, V.emulate(inp, False))
        step = np.abs(res["p"][3] - inp["p"].astype(np.float64))
        scale = dict(p=float(step.max()), m=float(np.abs(res["m"][3]).max()), v=float(np.abs(res["v"][3]).max()))
        for k in "pmv":
            if scale[k] == 0.0:
                assert case.n <= 7, case.id
                continue
            ratio = res[k][2] / scale[k]
            assert int((ratio > 1e-3).sum()) == 0, (case.id, k, float(ratio.max()))
            worst[k] = max(worst[k], float(ratio.max()))
        # p' against the element's OWN step.  The bound is gamma(10) |step| for the arithmetic plus u |p'|, half an ulp of the
        # stored result.  The first part is within 1e-3 of the step on EVERY element.  The second is no property of the kernel:
        # where half an ulp of p' is more than 0.5e-3 of the step, no fp32 parameter can show that step to 1e-3.  That class is
        # exempt, it is counted by kind, and outside it the whole bound is within 1e-3 of the step with no element left over.
        half_ulp = V.U * np.abs(res["p"][3])
        assert int((res["p"][2] - half_ulp > 1e-3 * step).sum()) == 0, case.id
        exempt = half_ulp > 0.5e-3 * step
        assert int(((res["p"][2] > 1e-3 * step) & ~exempt).sum()) == 0, case.id
        assert exempt[step == 0].all()
        elementwise[0] += int((step == 0).sum())
        elementwise[1] += int((exempt & (step != 0)).sum())
        elementwise[2] += case.n
    for k in "pmv":
        print(f"bound / scale, worst: {k}: {worst[k]:.3e}")
    print(f"p': exempt from the element-wise size check: {100.0 * elementwise[0] / elementwise[2]:.2f} % without a step (zero gradient, "
          f"zero moments, no weight decay), {100.0 * elementwise[1] / elementwise[2]:.2f} % with a step below 2^-13 |p'| (tiny gradients "
          "under eps = 1e-3, moments far below sqrt(v)); every other element is inside 1e-3 of its own step")


@pytest.mark.parametrize("n", [1023, 4 * 256 * 32 + 7, V.N_EMPTY, V.N_TWO])
def test_block_tables(n):
    from ctvae_amd.kernels import AdamBlockTable
    for style in V.TABLE_STYLES:
        for seed in (0, 1, 2, 3):
            ranges = V.make_table(n, seed, style)
            assert V.valid_table(ranges, n)
            AdamBlockTable(ranges, [-1] * len(ranges), n, 0, "cpu")                # the class's own rule
            blk = V.block_of(n, ranges)
            for b in (0, len(ranges) // 2, len(ranges) - 1):
                lo, hi = ranges[b]
                assert (blk[lo:hi] == b).all() and (lo == 0 or blk[lo - 1] != b) and (hi == n or blk[hi] != b)
            assert int((blk >= 0).sum()) == sum(hi - lo for lo, hi in ranges)
    st = V.table_stats(n, V.make_table(n, 0, "dense"))
    print(n, "dense:", st)
    assert st["max_blocks_in_quad"] >= 3 and st["whole_gap_quads"] >= 1 and st["odd_boundaries"] > st["nb"] // 2
    if n == V.N_TWO:
        assert 1500 <= st["nb"] <= 2500
    if n >= V.N_EMPTY:
        assert st["nb"] > 256                                                     # the last workgroup's bstate loop runs twice
    assert V.make_table(n, 0, "first_gap")[0][0] == 5
    ends = {n - V.make_table(n, s, "edges")[-1][1] for s in range(4)}
    assert ends == {0, 1, 2, 3}
    act = V.make_activity(50, 0, "half")
    assert 0 < act.sum() < 50 and V.make_activity(5, 0, "all").all() and not V.make_activity(5, 0, "none").any()
    assert set(V.make_counters(200, 0)) == set(V.COUNTERS)
