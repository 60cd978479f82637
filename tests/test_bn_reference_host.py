"""CPU: the float64 BatchNorm references of tests/bn_checks.py pinned to torch's float64 batch_norm + autograd, the row map of
split-K slices pinned to the scatter order of F.conv_transpose2d, the input conditions of every case of
tests/test_bn_ops_gpu.py evaluated on the reference alone, and the calibration of the bounds: a plain float32 two-pass model
stays inside every bound on every case, a float32 E[x^2] - E[x]^2 model violates the variance bound on the `offset` cases."""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_checks as V

PIN = 1e-12
ACTS = [V.ACT_NONE, V.ACT_LRELU, V.ACT_RELU, V.ACT_TANH]


def assert_pinned(got, want, what):
    got, want = got.detach().double(), want.detach().double()
    err = float((got - want).abs().max())
    scale = max(float(want.abs().max()), 1e-300)
    assert err <= PIN * scale, f"{what}: {err:.3e} against scale {scale:.3e}"


def torch_act(t, act):
    return {V.ACT_NONE: lambda v: v, V.ACT_LRELU: lambda v: F.leaky_relu(v, 0.01), V.ACT_RELU: F.relu, V.ACT_TANH: torch.tanh}[act](t)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("R,C", [(1, 8), (7, 12), (50, 4)])
def test_references_agree_with_torch_batch_norm_in_float64(R, C, act):
    cid = f"pin-{R}-{C}"
    y = V.make_y(cid, R, C, "o1") * 3.0 + 1.5
    gamma, beta, rm, rv = V.make_params(cid, C)
    ga = V.make_ga(cid, R, C)
    ref = V.forward_ref(y, gamma, beta, rm, rv, act)
    y64 = y.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    if R > 1:
        a = torch_act(F.batch_norm(y64, rm64, rv64, g64, b64, True, V.MOMENTUM, V.BN_EPS), act)
        assert_pinned(ref["running_mean"], rm64, "running_mean")
        assert_pinned(ref["running_var"], rv64, "running_var")
    else:       # torch refuses one value per channel in training; the formulas at R == 1: mean = y, var = 0, running var biased
        a = torch_act((y64 - y64.mean(0)) * (g64 / (V.BN_EPS ** 0.5)) + b64, act)
        assert_pinned(ref["running_var"], 0.9 * rv.double(), "running_var at R == 1")
    assert_pinned(ref["a"], a, "a")
    (a * ga.double()).sum().backward()
    mean32, invstd32 = ref["mean"], ref["invstd"]                  # the reference statistics themselves (float64): pure autograd
    bref = V.backward_ref(ga, y, gamma, beta, mean32, invstd32, act)
    if R > 1:
        assert_pinned(bref["gy"], y64.grad, "g_y")
    assert_pinned(bref["dgamma"], g64.grad, "dgamma")
    assert_pinned(bref["dbeta"], b64.grad, "dbeta")
    assert_pinned(bref["gy_coef"], bref["gy"], "k1*g' + k2*y + k3 against the textbook g_y")
    assert_pinned(bref["coef"][3], ref["scale"], "coef scale")
    assert_pinned(bref["coef"][4], ref["shift"], "coef shift")
    # eval: running statistics, nothing changes
    ev = V.forward_ref(y, gamma, beta, rm, rv, act, training=False)
    want = torch_act(F.batch_norm(y.double(), rm.double(), rv.double(), gamma.double(), beta.double(), False, V.MOMENTUM, V.BN_EPS), act)
    assert_pinned(ev["a"], want, "eval a")
    assert torch.equal(ev["running_mean"], rm.double()) and torch.equal(ev["running_var"], rv.double()) and ev["nbt_inc"] == 0


@pytest.mark.parametrize("B,Qh,Qw,s", [(1, 1, 1, 1), (3, 2, 5, 1), (2, 4, 4, 2), (3, 1, 1, 2), (1, 22, 3, 2), (5, 3, 7, 2)])
def test_row_map_is_a_permutation_in_conv_transpose_scatter_order(B, Qh, Qw, s):
    pix = V.row_map(B, Qh, Qw, s)
    Mc = B * Qh * Qw
    assert torch.equal(pix.sort().values, torch.arange(s * s * Mc))
    if s == 1:
        assert torch.equal(pix, torch.arange(Mc))
    m = torch.arange(1, Mc + 1, dtype=torch.float64).view(B, 1, Qh, Qw)
    for cls in range(s * s):
        w = torch.zeros(1, 1, s, s, dtype=torch.float64)
        w[0, 0, cls // s, cls % s] = 1.0                           # one-hot tap: class cls lands on its parity position
        out = F.conv_transpose2d(m, w, stride=s).flatten()
        assert torch.equal(out[pix[cls * Mc:(cls + 1) * Mc]], m.flatten())


def test_launcher_arithmetic_of_the_cases():
    for c in V.FWD_CASES + V.EVAL_CASES:
        assert V.shape_ok(c.R, c.C), c.id
    for c in V.FWD_CASES:
        assert V.stat_blocks(c.R, c.C)[0] == V.FWD_PARTIAL_ROWS[c.id], (c.id, V.stat_blocks(c.R, c.C))
    assert not V.shape_ok(5, 12) and not V.shape_ok(5, 6) and not V.shape_ok(0, 32)
    lab = {c.id: V.fwd_labels(c.R, c.C) for c in V.FWD_CASES}
    assert lab["R4099-C32"][-1] == "bn_finalize_apply_kernel" and lab["R16519-C64"][1:] == ["bn_finalize_kernel", "bn_apply_act_kernel"]
    assert lab["R3-C8"][1] == "bn_finalize_kernel" and lab["R2053-C2048"][1] == "bn_finalize_kernel"
    assert 1024 % 2048 != 0 and 1024 % 64 == 0                     # generic / fast apply loops
    # 4099 rows over 128 row ranges of 33: the 64-row stride leaves row 32 of a range to the first half only (`two` false)
    assert min(512 // (32 // 32), 4099 // 32) == 128 and -(-4099 // 128) == 33
    assert sorted({V.fused_instance(c.B * c.H * c.W, c.C) for c in V.FUSED_CASES if c.C in (8, 256)}) == [
        (64, 2, 8), (64, 4, 8), (256, 2, 8), (256, 4, 8), (1024, 2, 4), (1024, 4, 4)]
    for c in V.FUSED_CASES:
        assert V.fused_ok(c.B * c.H * c.W, c.C) and c.H % c.stride == 0 and c.W % c.stride == 0, c.id
    assert {c.S for c in V.FUSED_CASES} == {1, 3, 8, 9}


def _bwd_inputs(cid, R, C, kind, act, ga_kind="randn"):
    y = V.make_y(cid, R, C, kind)
    gamma, beta, _, _ = V.make_params(cid, C)
    mean, invstd = V.saved_stats(y)
    ga = V.make_ga(cid, R, C, ga_kind)
    return y, gamma, beta, mean, invstd, ga


@pytest.mark.parametrize("case", V.BWD_CASES + V.BWD_INT, ids=lambda c: c.id)
def test_backward_cases_exclude_few_elements(case):
    y, gamma, beta, mean, invstd, ga = _bwd_inputs(case.id, case.R, case.C, case.kind, case.act, "int" if case.id.startswith("int") else "randn")
    ref = V.backward_ref(ga, y, gamma, beta, mean, invstd, case.act)
    bnd = V.backward_bounds(ga, y, gamma, beta, mean, invstd, ref, V.bwd_case_chain(case), case.act)
    share = float(bnd["exclude"].double().mean())
    print(f"{case.id}: excluded share {share:.2e}")
    assert share <= V.EXCLUDE_CAP
    assert all(torch.isfinite(v).all() for v in bnd.values())
    if case.id.startswith("int"):
        assert float(ref["gp"].abs().sum(0).max()) < 2 ** 24           # every partial sum of integers is exact in float32


@pytest.mark.parametrize("case", V.FUSED_CASES, ids=lambda c: c.id)
def test_fused_backward_cases_exclude_few_elements(case):
    R = case.B * case.H * case.W
    y, gamma, beta, mean, invstd, ga = _bwd_inputs(case.id, R, case.C, case.kind, case.act)
    slices, total, abs_sum = V.split_slices(case.id, ga, case.S, V.fused_pix(case))
    assert float((total - ga.double()).abs().max()) <= 4 * V.EPS32 * float(abs_sum.max())
    ref = V.backward_ref(total, y, gamma, beta, mean, invstd, case.act)
    bnd = V.backward_bounds(total, y, gamma, beta, mean, invstd, ref, V.FUSED_CHAIN, case.act, ga_err=V.dot_bound(case.S, abs_sum))
    assert float(bnd["exclude"].double().mean()) <= V.EXCLUDE_CAP


CAL_KEYS = ("mean", "var", "invstd", "scale", "shift", "a")


def _ratios(model, ref, bnd):
    out = {}
    for k in CAL_KEYS:
        err = (model[k].double() - ref[k]).abs()
        out[k] = float((err / bnd[k].clamp(min=1e-300)).max()) if float(err.max()) > 0 else 0.0
    return out


@pytest.mark.parametrize("case", V.FWD_CASES, ids=lambda c: c.id)
def test_twopass_model_is_inside_every_bound_and_naive_model_is_not(case):
    y = V.make_y(case.id, case.R, case.C, case.kind)
    gamma, beta, rm, rv = V.make_params(case.id, case.C)
    ref = V.forward_ref(y, gamma, beta, rm, rv, case.act)
    bnd = V.forward_bounds(y, ref, gamma, rm, rv, V.fwd_chain(case.R, case.C), case.act)
    two = _ratios(V.twopass32(y, gamma, beta, case.act), ref, bnd)
    print(f"{case.id}: float32 two-pass err/bound " + " ".join(f"{k} {v:.4f}" for k, v in two.items()))
    assert max(two.values()) <= 1.0, two
    if case.kind == "offset":
        nv = _ratios(V.naive32(y, gamma, beta, case.act), ref, bnd)
        print(f"{case.id}: float32 E[x^2]-E[x]^2 err/bound " + " ".join(f"{k} {v:.3g}" for k, v in nv.items()))
        assert nv["var"] > 1.0 and nv["invstd"] > 1.0, nv
    if case.kind == "const":
        cc = V.const_channels(case.C)
        assert float(ref["var"][cc].max()) == 0.0
        assert_pinned(ref["a"][:, cc], V.act64(beta.double()[cc], case.act).expand(case.R, -1), "a == act(beta) on constant channels")


def test_bounds_do_not_grow_with_the_offset():
    """The variance bound relative to sigma^2 depends on |mu| / sigma only through the squared mean-error term."""
    cid, R, C = "grow", 4099, 32
    base = V.make_y(cid, R, C, "o1")
    gamma, beta, rm, rv = V.make_params(cid, C)
    rel = []
    for off in (0.0, 1e3):
        y = (base.double() + off).float()
        ref = V.forward_ref(y, gamma, beta, rm, rv, V.ACT_NONE)
        L = V.fwd_chain(R, C)
        bnd = V.forward_bounds(y, ref, gamma, rm, rv, L, V.ACT_NONE)
        rel.append(bnd["var"] / ref["var"])
        assert float((bnd["var"] - L * V.EPS32 * ref["var"] - bnd["mean"] ** 2).abs().max()) <= 1e-12 * float(bnd["var"].max())
    assert float(rel[1].max()) < 1e-3 and float(rel[0].max()) < 1e-4      # u * 1e6 = 0.12 would be the |mu|^2 term
