"""GPU: the BatchNorm kernels of csrc/bn.hip op by op through the C ABI (and, once each, through the autograd classes), on every
dispatch path, against the float64 references of tests/bn_checks.py (pinned to torch's float64 batch_norm + autograd, their
input conditions evaluated and their bounds calibrated in tests/test_bn_reference_host.py).

Every output buffer starts as NaN (integers as -1) and the workspace is filled with NaN before every call, so an element a
kernel skips, or scratch it reads without having written it, is seen.  Every call runs twice: the results must be finite and
bit-identical (bn.hip promises a fixed merge order).  Each case asserts through the library's launch log exactly which BatchNorm
kernels ran, and prints max err / bound per output.  Bounds are derived in bn_checks.py from the reference and the length of the
float32 addition chains alone; none was tuned on these kernels.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import bn_checks as V

pytestmark = pytest.mark.gpu

NAN = float("nan")
NBT0 = 5
PREFILL = 4096.0            # of dgamma / dbeta: far above every bound (asserted), so "gone" and "small" cannot be confused


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import native
    native.load()
    return native


@pytest.fixture(scope="module")
def K(N):
    from ctvae_amd import kernels
    return kernels


def dev():
    return torch.device("cuda")


def full(shape, fill=NAN, dtype=torch.float32):
    return torch.full(shape, fill, dtype=dtype, device=dev())


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def untouched(t, fill=NAN):
    return same(t, torch.full_like(t, fill))


def logged(native, fn):
    native.prof_report()
    native.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    return out, native.prof_report()


def bn_labels(rep):
    return sorted(k for k in rep if k.startswith("bn_"))


def twice(fn):
    """fn() -> dict of host tensors (None allowed), run twice from NaN scratch: finite where checked later, bit-identical here."""
    a, b = fn(), fn()
    for k in a:
        assert (a[k] is None and b[k] is None) or same(a[k], b[k]), f"{k}: two runs differ"
    return a


def within(what, got, want, tol, skip=None):
    """|got - want| <= tol elementwise (elements of `skip` left out); prints the largest ratio."""
    got = got.double().reshape(want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - want).abs()
    tol = tol.expand_as(err) if tol.shape != err.shape else tol
    if skip is not None:
        err, tol = err[~skip], tol[~skip]
    ratio = float((err / tol.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: max |err| {float(err.max()) if err.numel() else 0.0:.3e}, max err/bound = {ratio:.4f}")
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} of {err.numel()} elements beyond the bound, worst ratio {ratio:.3f}"
    return ratio


def fails(native, code, name, *args):
    with pytest.raises(RuntimeError, match=rf"{name} failed.*\(code {code}\)"):
        native.call(name, *args)


def nan_ws(native):
    ws = native.workspace(dev())
    ws.fill_(NAN)
    return ws


# ---------------------------------------------------------------------------------------------------------------------
# ctvae_bn_forward
# ---------------------------------------------------------------------------------------------------------------------
def run_forward(native, y, gamma, beta, rm, rv, act, training=True, ws_floats=None, R=None, C=None):
    yd, gd, bd, rmd, rvd = (t.to(dev()) for t in (y, gamma, beta, rm, rv))
    R = y.shape[0] if R is None else R
    C = y.shape[1] if C is None else C
    a, mean, invstd = full(tuple(y.shape)), full((y.shape[1],)), full((y.shape[1],))
    nbt = full((), NBT0, torch.int64)
    ws = nan_ws(native)
    native.call("ctvae_bn_forward", yd.data_ptr(), R, C, gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), V.MOMENTUM,
                V.BN_EPS, 1 if training else 0, act, a.data_ptr(), mean.data_ptr(), invstd.data_ptr(), nbt.data_ptr(), ws.data_ptr(),
                (ws.numel() if ws_floats is None else ws_floats) * 4)
    torch.cuda.synchronize()
    return dict(a=a.cpu(), mean=mean.cpu(), invstd=invstd.cpu(), running_mean=rmd.cpu(), running_var=rvd.cpu(), nbt=nbt.cpu())


def check_forward(cid, out, ref, bnd, keys=("a", "mean", "invstd", "running_mean", "running_var")):
    return {k: within(f"{cid}/{k}", out[k], ref[k], bnd[k]) for k in keys}


def fwd_inputs(case):
    return (V.make_y(case.id, case.R, case.C, case.kind),) + V.make_params(case.id, case.C)


@pytest.mark.parametrize("case", V.FWD_CASES, ids=lambda c: c.id)
def test_bn_forward_training(N, case):
    """Measured on an MI355X: every case is inside every bound; largest err/bound of invstd 0.54 (R9-C2048), 0.22 (R1-C32), 0.18
    (R37-C512), of running_var 0.46 (R37-C512), 0.005 / 0.03 at the clamped 4.2 M row case.  R37-C512 (`offset`, |mu| / sigma up
    to 1e3, two partial rows of 19) is the case that found the partial means' rounding: while bn_stats_partial_kernel wrote
    absolute float32 means, the d of a Chan merge carried u |mu| and d^2 a cross term ~ 2 sigma_d u |mu| -- linear in
    |mu| / sigma, which the variance bound (L u sigma^2 + mean_bound^2) excludes; save_invstd was 2.96 x its bound on 37 of 512
    channels.  The kernel now keeps its means relative to row 0 of the channel and the finalize adds that row back."""
    y, gamma, beta, rm, rv = fwd_inputs(case)
    assert V.stat_blocks(case.R, case.C)[0] == V.FWD_PARTIAL_ROWS[case.id]
    ref = V.forward_ref(y, gamma, beta, rm, rv, case.act)
    bnd = V.forward_bounds(y, ref, gamma, rm, rv, V.fwd_chain(case.R, case.C), case.act)
    out, rep = logged(N, lambda: run_forward(N, y, gamma, beta, rm, rv, case.act))
    assert bn_labels(rep) == sorted(V.fwd_labels(case.R, case.C)) and all(v["count"] == 1 for v in rep.values()), rep
    check_forward(case.id, out, ref, bnd)
    assert int(out["nbt"]) == NBT0 + 1
    if case.kind == "const":
        cc = V.const_channels(case.C)
        assert float(ref["var"][cc].max()) == 0.0
        within(f"{case.id}/constant channels: a against act(beta)", out["a"][:, cc],
               V.act64(beta.double()[cc], case.act).expand(case.R, -1), bnd["a"][:, cc])
        within(f"{case.id}/constant channels: invstd against 1/sqrt(eps)", out["invstd"][cc],
               torch.full((len(cc),), V.BN_EPS ** -0.5, dtype=torch.float64), bnd["invstd"][cc])
    if case.R * case.C < 1 << 23:
        again = run_forward(N, y, gamma, beta, rm, rv, case.act)
        assert all(same(out[k], again[k]) for k in out), "two runs differ"


@pytest.mark.parametrize("case", V.EVAL_CASES, ids=lambda c: c.id)
def test_bn_forward_eval(N, case):
    y, gamma, beta, rm, rv = fwd_inputs(case)
    ref = V.forward_ref(y, gamma, beta, rm, rv, case.act, training=False)
    bnd = V.forward_bounds(y, ref, gamma, rm, rv, 0, case.act, training=False)
    out, rep = logged(N, lambda: twice(lambda: run_forward(N, y, gamma, beta, rm, rv, case.act, training=False)))
    assert bn_labels(rep) == ["bn_apply_act_kernel"], rep
    within(f"{case.id}/a", out["a"], ref["a"], bnd["a"])
    assert same(out["running_mean"], rm) and same(out["running_var"], rv) and int(out["nbt"]) == NBT0
    assert untouched(out["mean"]) and untouched(out["invstd"])


def test_bn_argument_errors_launch_nothing(N):
    C = 32
    y = torch.zeros(4, 64, device=dev())
    vec = [torch.ones(64, device=dev()) for _ in range(4)]
    ws = N.workspace(dev())

    def fwd(R, C_, ws_bytes, code):
        a, mean, invstd = full((4, 64)), full((64,)), full((64,))
        nbt = full((), NBT0, torch.int64)

        def call():
            fails(N, code, "ctvae_bn_forward", y.data_ptr(), R, C_, vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(),
                  vec[3].data_ptr(), V.MOMENTUM, V.BN_EPS, 1, V.ACT_LRELU, a.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                  nbt.data_ptr(), ws.data_ptr(), ws_bytes)
        _, rep = logged(N, call)
        assert rep == {}, sorted(rep)
        assert untouched(a) and untouched(mean) and untouched(invstd) and int(nbt) == NBT0
        assert all(float(v.min()) == 1.0 and float(v.max()) == 1.0 for v in vec)

    fwd(4, 12, ws.numel() * 4, V.ERR_BAD_ARG)            # Q = 3 neither divides 256 nor is a multiple of it
    fwd(4, 6, ws.numel() * 4, V.ERR_BAD_ARG)
    fwd(0, C, ws.numel() * 4, V.ERR_BAD_ARG)
    fwd(4, C, (V.workspace_floats(C) - 1) * 4, V.ERR_WORKSPACE)

    def bwd(code, gy, coef_out, coef_in, part):
        dg, db = full((C,)), full((C,))

        def call():
            fails(N, code, "ctvae_bn_backward", y.data_ptr(), vec[1].data_ptr(), y.data_ptr(), 4, C, vec[0].data_ptr(), vec[2].data_ptr(),
                  vec[3].data_ptr(), V.ACT_LRELU, N.ptr(gy), dg.data_ptr(), db.data_ptr(), 0, N.ptr(part), 1 if part is not None else 0,
                  N.ptr(coef_out), N.ptr(coef_in), ws.data_ptr(), ws.numel() * 4)
        _, rep = logged(N, call)
        assert rep == {}, sorted(rep)
        assert untouched(dg) and untouched(db) and (gy is None or untouched(gy))

    bwd(V.ERR_BAD_ARG, None, None, None, None)                                      # neither g_y nor coef_out
    bwd(V.ERR_BAD_ARG, full((4, C)), None, torch.zeros(7, C, device=dev()), torch.zeros(1, C, 2, device=dev()))   # coef_in with part_in
    # an exact-size workspace is served
    out = run_forward(N, torch.randn(4, C), *[t[:C].cpu() for t in vec], V.ACT_NONE, ws_floats=V.workspace_floats(C))
    assert torch.isfinite(out["a"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# ctvae_bn_backward
# ---------------------------------------------------------------------------------------------------------------------
def run_backward(native, ga, y, gamma, beta, mean, invstd, act, accumulate, part=None, coef_out=False, coef_in=None, want_gy=True):
    gad, yd, gd, bd, md, isd = (t.to(dev()) for t in (ga, y, gamma, beta, mean, invstd))
    R, C = y.shape
    gy = full((R, C)) if want_gy else None
    dg, db = full((C,), PREFILL), full((C,), PREFILL)
    co = full((7, C)) if coef_out else None                       # [5][C] is what the call may write
    pd = None if part is None else part.to(dev())
    ci = None if coef_in is None else coef_in.to(dev())
    ws = nan_ws(native)
    native.call("ctvae_bn_backward", gad.data_ptr(), bd.data_ptr(), yd.data_ptr(), R, C, gd.data_ptr(), md.data_ptr(), isd.data_ptr(), act,
                native.ptr(gy), dg.data_ptr(), db.data_ptr(), accumulate, native.ptr(pd), 0 if part is None else part.shape[0],
                native.ptr(co), native.ptr(ci), ws.data_ptr(), ws.numel() * 4)
    torch.cuda.synchronize()
    return dict(gy=None if gy is None else gy.cpu(), dgamma=dg.cpu(), dbeta=db.cpu(), coef=None if co is None else co.cpu())


def bwd_inputs(case, ga_kind="randn"):
    y = V.make_y(case.id, case.R, case.C, case.kind)
    gamma, beta, _, _ = V.make_params(case.id, case.C)
    mean, invstd = V.saved_stats(y)
    return V.make_ga(case.id, case.R, case.C, ga_kind), y, gamma, beta, mean, invstd


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", V.BWD_CASES, ids=lambda c: c.id)
def test_bn_backward_forms(N, case, accumulate):
    ga, y, gamma, beta, mean, invstd = bwd_inputs(case)
    ref = V.backward_ref(ga, y, gamma, beta, mean, invstd, case.act)
    bnd = V.backward_bounds(ga, y, gamma, beta, mean, invstd, ref, V.bwd_case_chain(case), case.act)
    assert float(bnd["exclude"].double().mean()) <= V.EXCLUDE_CAP
    assert float(bnd["dgamma"].max()) < PREFILL / 2 and float(bnd["dbeta"].max()) < PREFILL / 2
    base = PREFILL if accumulate else 0.0
    acc_round = V.EPS32 * PREFILL if accumulate else 0.0
    kw, want_dg, want_db, tol_dg, tol_db = {}, ref["dgamma"], ref["dbeta"], bnd["dgamma"], bnd["dbeta"]
    if case.form in ("part-one", "part-two"):
        part, sums = V.partial_rows(ref, V.random_partition(case.id, case.R, case.rows))
        kw["part"] = part
        want_db, want_dg = sums[:, 0], sums[:, 1]                  # the double sum of the float32 rows, cast once
        tol_db, tol_dg = V.EPS32 * want_db.abs(), V.EPS32 * want_dg.abs()
    elif case.form == "coef-out":
        kw.update(coef_out=True, want_gy=False)
    elif case.form == "coef-in":
        kw["coef_in"] = ref["coef"].float()
    out, rep = logged(N, lambda: twice(lambda: run_backward(N, ga, y, gamma, beta, mean, invstd, case.act, accumulate, **kw)))
    assert bn_labels(rep) == sorted(V.BWD_LABELS[case.form]) and all(v["count"] == 2 for v in rep.values()), rep
    tag = f"{case.id}/acc{accumulate}"
    if case.form == "coef-in":
        c32 = kw["coef_in"]                                        # rows 5, 6 are committed as they are: one float32 addition
        assert torch.equal(out["dgamma"], torch.full_like(c32[5], base) + c32[5]) and torch.equal(out["dbeta"], torch.full_like(c32[6], base) + c32[6])
    else:
        within(f"{tag}/dgamma", out["dgamma"], want_dg + base, tol_dg + acc_round)
        within(f"{tag}/dbeta", out["dbeta"], want_db + base, tol_db + acc_round)
    if case.form == "coef-out":
        assert out["gy"] is None
        within(f"{tag}/coef[5][C]", out["coef"][:5], ref["coef"][:5], bnd["coef"][:5])
        assert untouched(out["coef"][5:])                          # a [5][C] block: nothing behind it is written
    else:
        within(f"{tag}/g_y", out["gy"], ref["gy"], bnd["gy"], skip=bnd["exclude"])


@pytest.mark.parametrize("case", V.BWD_INT, ids=lambda c: c.id)
def test_bn_backward_integer_gradients_sum_exactly(N, case):
    """Integer g_a, no activation: every partial sum of dbeta is an integer below 2^24, exact in float32 in any order -- a
    dropped or doubled row shows as a whole number."""
    ga, y, gamma, beta, mean, invstd = bwd_inputs(case, "int")
    ref = V.backward_ref(ga, y, gamma, beta, mean, invstd, case.act)
    assert float(ref["gp"].abs().sum(0).max()) < 2 ** 24
    out, rep = logged(N, lambda: run_backward(N, ga, y, gamma, beta, mean, invstd, case.act, 0))
    assert bn_labels(rep) == sorted(V.BWD_LABELS["plain"]), rep
    assert torch.equal(out["dbeta"].double(), ref["dbeta"])
    out = run_backward(N, ga, y, gamma, beta, mean, invstd, case.act, 1)
    assert torch.equal(out["dbeta"].double(), ref["dbeta"] + PREFILL)


# ---------------------------------------------------------------------------------------------------------------------
# ctvae_bn_backward_fused
# ---------------------------------------------------------------------------------------------------------------------
def run_fused_backward(native, case, slices, y, gamma, beta, mean, invstd, accumulate):
    sd, yd, gd, bd, md, isd = (t.to(dev()) for t in (slices, y, gamma, beta, mean, invstd))
    R, C = y.shape
    gy, dg, db = full((R, C)), full((C,), PREFILL), full((C,), PREFILL)
    native.call("ctvae_bn_backward_fused", sd.data_ptr(), case.S, *V.fused_geom(case), yd.data_ptr(), gd.data_ptr(), bd.data_ptr(),
                md.data_ptr(), isd.data_ptr(), case.act, gy.data_ptr(), dg.data_ptr(), db.data_ptr(), accumulate)
    torch.cuda.synchronize()
    return dict(gy=gy.cpu(), dgamma=dg.cpu(), dbeta=db.cpu())


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", V.FUSED_CASES, ids=lambda c: c.id)
def test_bn_backward_fused(N, case, accumulate):
    R = case.B * case.H * case.W
    y = V.make_y(case.id, R, case.C, case.kind)
    gamma, beta, _, _ = V.make_params(case.id, case.C)
    mean, invstd = V.saved_stats(y)
    slices, ga, abs_sum = V.split_slices(case.id, V.make_ga(case.id, R, case.C), case.S, V.fused_pix(case))
    ref = V.backward_ref(ga, y, gamma, beta, mean, invstd, case.act)
    bnd = V.backward_bounds(ga, y, gamma, beta, mean, invstd, ref, V.FUSED_CHAIN, case.act, ga_err=V.dot_bound(case.S, abs_sum))
    assert float(bnd["exclude"].double().mean()) <= V.EXCLUDE_CAP and float(max(bnd["dgamma"].max(), bnd["dbeta"].max())) < PREFILL / 2
    out, rep = logged(N, lambda: twice(lambda: run_fused_backward(N, case, slices, y, gamma, beta, mean, invstd, accumulate)))
    assert bn_labels(rep) == ["bn_fused_bwd_kernel"] and rep["bn_fused_bwd_kernel"]["count"] == 2, rep
    base = PREFILL if accumulate else 0.0
    acc_round = V.EPS32 * PREFILL if accumulate else 0.0
    tag = f"{case.id}/acc{accumulate} {V.fused_instance(R, case.C)}"
    within(f"{tag}/dgamma", out["dgamma"], ref["dgamma"] + base, bnd["dgamma"] + acc_round)
    within(f"{tag}/dbeta", out["dbeta"], ref["dbeta"] + base, bnd["dbeta"] + acc_round)
    within(f"{tag}/g_y", out["gy"], ref["gy"], bnd["gy"], skip=bnd["exclude"])


# ---------------------------------------------------------------------------------------------------------------------
# ctvae_conv_bn_act_forward: the only way to bn_fused_fwd_kernel and to the statistics epilogues of the conv kernels
# ---------------------------------------------------------------------------------------------------------------------
def pack(w, transposed):
    return (w.permute(2, 3, 0, 1) if transposed else w.permute(2, 3, 1, 0)).contiguous()


def conv64(x, w, b, case):
    """float64 conv of float32 inputs, NCHW; returns y [R][C] in pixel-major (NHWC) order and the sum of |products|."""
    def go(x_, w_, b_):
        o = (F.conv_transpose2d(x_, w_, b_, stride=case.s, padding=case.p, output_padding=case.op) if case.tr
             else F.conv2d(x_, w_, b_, stride=case.s, padding=case.p))
        return o.permute(0, 2, 3, 1).reshape(-1, case.Co)
    return go(x.double(), w.double(), b.double()), go(x.double().abs(), w.double().abs(), b.double().abs())


@pytest.fixture(scope="module")
def conv_inputs():
    cache = {}

    def make(case):
        if case.id not in cache:
            g = V.gen_of(case.id, 41)
            x = torch.randn(case.B, case.Ci, case.H, case.H, generator=g)
            fan = case.Ci * case.k * case.k / (case.s * case.s if case.tr else 1)
            w = torch.randn((case.Ci, case.Co, case.k, case.k) if case.tr else (case.Co, case.Ci, case.k, case.k), generator=g) / fan ** 0.5
            y0, _ = conv64(x, w, torch.zeros(case.Co), case)
            sign = torch.where(torch.rand(case.Co, generator=g) < 0.5, -1.0, 1.0)
            b = (30.0 * y0.std(0) * sign).float()                 # plants a mean of ~30 sigma in every channel
            cache[case.id] = (x, w, b) + V.make_params(case.id, case.Co) + conv64(x, w, b, case)
        return cache[case.id]
    return make


def run_conv_bn(K, native, case, x, w, b, gamma, beta, rm, rv, training=True):
    spec = K.ConvSpec(K.CONVT if case.tr else K.CONV, case.Ci, case.Co, case.k, case.s, case.p, case.op, K.ACT_NONE)
    g = spec.geom(case.B, case.H, case.H)
    ho, wo = spec.out_hw(case.H, case.H)
    R, C = case.B * ho * wo, case.Co
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev())
    wd, bd, gd, btd, rmd, rvd = (t.to(dev()) for t in (pack(w, case.tr), b, gamma, beta, rm, rv))
    y, mean, invstd = full((R, C)), full((C,)), full((C,))
    a = None if case.lazy else full((R, C))
    coef = full((2, C))
    nbt = full((), NBT0, torch.int64)
    ws = nan_ws(native)
    native.call("ctvae_conv_bn_act_forward", g[0], xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), gd.data_ptr(), btd.data_ptr(),
                rmd.data_ptr(), rvd.data_ptr(), V.MOMENTUM, V.BN_EPS, 1 if training else 0, case.act, y.data_ptr(), native.ptr(a),
                mean.data_ptr(), invstd.data_ptr(), coef.data_ptr(), nbt.data_ptr(), *g[1:], None, None, 0, ws.data_ptr(), ws.numel() * 4)
    torch.cuda.synchronize()
    return dict(y=y.cpu(), a=None if a is None else a.cpu(), mean=mean.cpu(), invstd=invstd.cpu(), coef=coef.cpu(),
                running_mean=rmd.cpu(), running_var=rvd.cpu(), nbt=nbt.cpu())


def check_conv_bn(case, out, inputs, L, training=True):
    """Raw y against the float64 conv (dot_bound over the taps, + 34 for bias, split-K slices and their sum); everything behind it
    against the BatchNorm reference of the y the kernel itself wrote, so that both sides see the same numbers."""
    x, w, b, gamma, beta, rm, rv, y64, yabs = inputs
    within(f"{case.id}/y", out["y"], y64, V.dot_bound(case.Ci * case.k * case.k + 34, yabs))
    mu = out["y"].double().mean(0)
    assert float((mu.abs() / out["y"].double().std(0)).min()) > 20.0            # the planted mean is there
    ref = V.forward_ref(out["y"], gamma, beta, rm, rv, case.act, training=training)
    bnd = V.forward_bounds(out["y"], ref, gamma, rm, rv, L, case.act, training=training)
    keys = ("mean", "invstd", "running_mean", "running_var") if training else ()
    check_forward(case.id, out, ref, bnd, keys + (() if case.lazy else ("a",)))
    within(f"{case.id}/scale", out["coef"][0], ref["scale"], bnd["scale"])
    within(f"{case.id}/shift", out["coef"][1], ref["shift"], bnd["shift"])
    return ref


def conv_spec_of(K, case):
    return K.ConvSpec(K.CONVT if case.tr else K.CONV, case.Ci, case.Co, case.k, case.s, case.p, case.op, K.ACT_NONE)


@pytest.mark.parametrize("case", V.CONV_FUSED_CASES, ids=lambda c: c.id)
def test_conv_bn_act_forward_split_k_channel_owners(N, K, conv_inputs, case):
    """Split-K convolution + bn_fused_fwd_kernel.  The three thread-count classes are reached by R = 12 / 128 (64 threads), 512
    (256) and 2048 (1024); C = 128 and 64 take the two-channel owners, 256 the four-channel ones."""
    inputs = conv_inputs(case)
    assert K.bn_apply_is_separate(conv_spec_of(K, case), case.B, case.H, case.H) is False
    out, rep = logged(N, lambda: twice(lambda: run_conv_bn(K, N, case, *inputs[:7])))
    assert bn_labels(rep) == ["bn_fused_fwd_kernel"] and rep["bn_fused_fwd_kernel"]["count"] == 2, sorted(rep)
    assert "splitk_finish_kernel" not in rep
    check_conv_bn(case, out, inputs, V.FUSED_CHAIN)
    assert int(out["nbt"]) == NBT0 + 1


UNSPLIT_PRODUCER = {"tile-32to64": "tapgemm_", "masked-3to64-k4": "tapgemm_masked_kernel", "imgenc-3to32": "img_enc_fwd_kernel", "upconv-32to32": "up_fwd_kernel"}


@pytest.mark.parametrize("case", V.CONV_UNSPLIT_CASES, ids=lambda c: c.id)
def test_conv_bn_act_forward_statistics_from_the_conv_epilogue(N, K, conv_inputs, case):
    """Unsplit convolution: the (count, mean, M2) partial rows come out of the conv kernel's epilogue -- one case per producer --
    and bn_stats_partial_kernel must NOT run.  thin.hip is no producer that this entry point can reach: its kernels serve the
    3-output-channel layers only (thin_bn_parts() is 0, and C = 3 is no BatchNorm shape), so the fourth case is the masked
    variant of the tile kernel instead."""
    inputs = conv_inputs(case)
    assert K.bn_apply_is_separate(conv_spec_of(K, case), case.B, case.H, case.H) is True
    out, rep = logged(N, lambda: twice(lambda: run_conv_bn(K, N, case, *inputs[:7])))
    print(case.id, sorted(rep))
    assert any(k.startswith(UNSPLIT_PRODUCER[case.id]) for k in rep), sorted(rep)
    want = ["bn_finalize_kernel"] if case.lazy else None
    got = bn_labels(rep)
    assert got == want if want else got in (["bn_finalize_apply_kernel"], ["bn_apply_act_kernel", "bn_finalize_kernel"]), got
    check_conv_bn(case, out, inputs, V.TILE_CHAIN)
    assert int(out["nbt"]) == NBT0 + 1


def test_conv_bn_act_forward_eval(N, K, conv_inputs):
    case = V.CONV_FUSED_CASES[0]
    inputs = conv_inputs(case)
    out, rep = logged(N, lambda: twice(lambda: run_conv_bn(K, N, case, *inputs[:7], training=False)))
    assert bn_labels(rep) == ["bn_apply_act_kernel"], sorted(rep)
    check_conv_bn(case, out, inputs, 0, training=False)
    assert same(out["running_mean"], inputs[5]) and same(out["running_var"], inputs[6]) and int(out["nbt"]) == NBT0
    assert untouched(out["mean"]) and untouched(out["invstd"])


# ---------------------------------------------------------------------------------------------------------------------
# through autograd: the Python wrappers pass accumulate / coef / part the way the raw tests assume
# ---------------------------------------------------------------------------------------------------------------------
AUTOGRAD = V.Conv("autograd-32to64", False, 3, 16, 32, 64, 3, 2, 1, 0, V.ACT_TANH, False, None)


@pytest.mark.parametrize("lazy_out", [False, True], ids=["tanh", "lazy_out"])
def test_conv_bn_act_through_autograd(N, K, conv_inputs, lazy_out):
    """K.ConvBNAct forward + backward.  The forward is checked as above (y is the tensor the BatchNorm link holds); g_y, dgamma
    and dbeta against the BatchNorm backward reference of that y and the saved statistics; dx, dw, dbias against the float64
    conv gradients of the reference g_y, with the g_y bound carried through |w| / |x| and the conv's own dot_bound added."""
    case = AUTOGRAD._replace(act=V.ACT_LRELU if lazy_out else V.ACT_TANH, lazy=lazy_out)
    x, w, b, gamma, beta, rm, rv, y64, yabs = inputs = conv_inputs(AUTOGRAD)
    spec = conv_spec_of(K, case)
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev()).requires_grad_(True)
    wp = torch.nn.Parameter(pack(w, False).to(dev()).permute(3, 2, 0, 1))
    bp, gp, btp = (torch.nn.Parameter(t.to(dev())) for t in (b, gamma, beta))
    rmd, rvd, nbt = rm.to(dev()), rv.to(dev()), full((), NBT0, torch.int64)
    out = K.ConvBNAct.apply(xd, wp, bp, gp, btp, rmd, rvd, True, spec, case.act, nbt, lazy_out)
    link = K.tag_of(out).bn_link
    R, C = y64.shape
    got = dict(y=link.y.detach().cpu().view(R, C), a=None if lazy_out else out.detach().cpu().view(R, C), mean=link.mean.cpu(),
               invstd=link.invstd.cpu(), running_mean=rmd.cpu(), running_var=rvd.cpu(),
               coef=K.tag_of(out).lazy_bn[0].cpu().view(2, C) if lazy_out else None)
    if not lazy_out:                # no coefficient block without lazy_out: check_conv_bn reads one
        fr = V.forward_ref(got["y"], gamma, beta, rm, rv, case.act)
        got["coef"] = torch.stack([fr["scale"], fr["shift"]]).float()
    check_conv_bn(case, got, inputs, max(V.TILE_CHAIN, V.FUSED_CHAIN))
    assert int(nbt) == NBT0 + 1
    if lazy_out:
        assert same(out.detach().cpu().view(R, C), got["y"])       # the output IS the raw conv output
    ga = V.make_ga(case.id, R, C)
    _, rep = logged(N, lambda: out.backward(ga.view(out.shape).to(dev())))
    assert any(k.startswith("bn_bwd") for k in rep), sorted(rep)
    ref = V.backward_ref(ga, got["y"], gamma, beta, got["mean"], got["invstd"], case.act)
    L = max(V.bwd_chain(R, C), V.TILE_CHAIN)
    bnd = V.backward_bounds(ga, got["y"], gamma, beta, got["mean"], got["invstd"], ref, L, case.act)
    tag = f"autograd/{'lazy_out' if lazy_out else 'tanh'}"
    within(f"{tag}/dgamma", gp.grad.cpu(), ref["dgamma"], bnd["dgamma"])
    within(f"{tag}/dbeta", btp.grad.cpu(), ref["dbeta"], bnd["dbeta"])
    # conv gradients of g_y (NCHW, float64); excluded elements may carry a flipped slope: |k1 g_a| * gap on top of their bound
    gy_b = bnd["gy"] + bnd["exclude"] * (ref["coef"][0] * ga.double()).abs() * V.slope_gap(case.act)
    nchw = lambda t: t.view(case.B, 8, 8, C).permute(0, 3, 1, 2).contiguous()   # noqa: E731
    gy, gyb, xx, ww = nchw(ref["gy"]), nchw(gy_b), x.double(), w.double()
    Lc = case.Ci * 9 + 34
    cin = lambda g_, w_: torch.nn.grad.conv2d_input(xx.shape, w_, g_, stride=2, padding=1)      # noqa: E731
    cw = lambda x_, g_: torch.nn.grad.conv2d_weight(x_, ww.shape, g_, stride=2, padding=1)      # noqa: E731
    within(f"{tag}/dx", xd.grad.cpu().permute(0, 3, 1, 2), cin(gy, ww), cin(gyb, ww.abs()) + V.dot_bound(Lc, cin(gy.abs(), ww.abs())))
    Lw = R + 34
    within(f"{tag}/dw", wp.grad.cpu(), cw(xx, gy), cw(xx.abs(), gyb) + V.dot_bound(Lw, cw(xx.abs(), gy.abs())))
    within(f"{tag}/dbias", bp.grad.cpu(), gy.sum((0, 2, 3)), gyb.sum((0, 2, 3)) + V.dot_bound(Lw, gy.abs().sum((0, 2, 3))))
