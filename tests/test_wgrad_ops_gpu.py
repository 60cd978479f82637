"""GPU: ctvae_conv_wgrad (csrc/wgrad.hip launch_wgrad) op by op through the C ABI on every dispatch path -- the nine kernel
families, the six shapes of the slab reduction, accumulate / dbias, the deferred reduction and every refusal -- against the float64
references of tests/wgrad_checks.py (pinned to torch's float64 autograd, their input conditions and bounds evaluated in
tests/test_wgrad_reference_host.py).

Every output starts as NaN and the workspace is filled with NaN before every call, so an element a kernel skips, or a slab
it reduces without having written it, is seen.  Every call runs twice: the results must be bit-identical (two passes, fixed
summation order, no float atomics).  Every case asserts through the library's launch log exactly which kernels ran (and, where
the case names it, the split count S), as the mirror of launch_wgrad's selection in wgrad_checks.py predicts.  In the `int`
regime the result must equal the reference bit for bit; in the `randn` regime it must lie inside a bound derived from the
length of the float32 addition chains alone, and max err / bound is printed.  No bound was tuned on these kernels."""
import dataclasses
import re

import pytest
import torch

from tests import wgrad_checks as V

pytestmark = pytest.mark.gpu

NAN = float("nan")
_REF = {}


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import native
    native.load()
    return native


@pytest.fixture(autouse=True)
def direct_kernels(N):
    """Winograd is on by default: every test here runs with it off unless its case switches it on (with_winograd)."""
    prev = N.winograd_enable(False)
    try:
        yield
    finally:
        N.winograd_enable(prev)


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
    native.prof_enable(True, detailed=True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    return out, native.prof_report()


def labels(rep):
    """{kernel label without the shape suffix: count} and the S= of the detailed names."""
    out, S = {}, None
    for name, v in rep.items():
        base = name.split(" ")[0] if not name.startswith("reduce_partials_kernel") else name
        out[base] = out.get(base, 0) + v["count"]
        m = re.search(r" S=(\d+)", name)
        if m:
            S = int(m.group(1))
    return out, S


def twice(fn):
    """fn() -> dict of host tensors (None allowed), run twice from NaN scratch: bit-identical."""
    a, b = fn(), fn()
    for k in a:
        assert (a[k] is None and b[k] is None) or same(a[k], b[k]), f"{k}: two runs differ"
    return a


def within(what, got, want, tol):
    """|got - want| <= tol elementwise, every element; prints and returns the largest ratio."""
    got = got.double().reshape(want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - want).abs()
    ratio = float((err / tol).max())
    print(f"{what}: max |err| {float(err.max()):.3e}, max err/bound = {ratio:.4f}")
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} of {err.numel()} elements beyond the bound, worst ratio {ratio:.3f}"
    return ratio


def exact(what, got, want):
    got = got.double().reshape(want.shape)
    bad = int((got != want).sum()) + int((~torch.isfinite(got)).sum())
    assert bad == 0, f"{what}: {bad} of {want.numel()} elements differ from the exact result, max |diff| {float((got - want).abs().nan_to_num(1e30).max()):.3e}"


def fails(native, code, name, *args):
    with pytest.raises(RuntimeError, match=rf"{name} failed.*\(code {code}\)"):
        native.call(name, *args)


def nan_ws(native):
    ws = native.workspace(dev())
    ws.fill_(NAN)
    return ws


def ref_of(case, regime):
    """One reference per (geometry, transforms, regime): shared by the tests, never modified."""
    key = (case.args(), case.xf, case.dyx, case.id, regime)
    if key not in _REF:
        _REF[key] = V.reference(case, regime)
    return _REF[key]


_INPUTS = {}


def inputs_of(case, regime):
    key = (case.id, regime)
    if key not in _INPUTS:
        _INPUTS[key] = V.make_inputs(case, regime)
    return _INPUTS[key]


def dw_shape(case):
    kk = case.k * case.k
    return (case.Ci, kk, case.Co) if case.kind & V.W_CI_TAP else (kk, case.Ci, case.Co)


def prefill_of(shape):
    n = 1
    for s in shape:
        n *= s
    return ((torch.arange(n) % 7) - 3).float().reshape(shape)


class Call:
    """Device tensors and argument list of one ctvae_conv_wgrad call of a case."""

    def __init__(self, native, case, regime, accumulate=0, bias=True, ws=None, ws_floats=None, bn_accumulate=0, drop=()):
        self.native, self.case = native, case
        x, dy, xf, dyx = inputs_of(case, regime)
        self.x, self.dy = x.to(dev()), dy.to(dev())
        self.dw = prefill_of(dw_shape(case)).to(dev()) if accumulate else full(dw_shape(case))
        self.db = None
        if bias:
            self.db = prefill_of((case.Co,)).to(dev()) if accumulate else full((case.Co,))
        self.sc = self.sh = self.y = self.coef = self.gy = self.dgamma = self.dbeta = None
        in_act = dy_act = 0
        if xf is not None:
            self.sc, self.sh, in_act = xf[0].to(dev()), xf[1].to(dev()), xf[2]
        if dyx is not None:
            self.y, self.coef, dy_act = dyx[0].to(dev()), dyx[1].to(dev()), dyx[2]
            if case.dy_out == "gy":
                self.gy = full(tuple(dy.shape))
            if case.dy_out == "commit":
                self.dgamma = prefill_of((case.Co,)).to(dev()) if bn_accumulate else full((case.Co,))
                self.dbeta = (prefill_of((case.Co,)) + 1).to(dev()) if bn_accumulate else full((case.Co,))
        for name in drop:                         # argument errors: leave one pointer out
            setattr(self, name, None)
        self.ws = nan_ws(native) if ws is None else ws
        self.ws_floats = case.ws() if ws_floats is None else ws_floats
        assert self.ws_floats <= self.ws.numel()
        P = native.ptr
        self.args = (case.kind, P(self.x), P(self.dy), P(self.dw), P(self.db), case.B, case.H, case.W, case.Ci, case.Co, case.k, case.s,
                     case.p, case.op, accumulate, P(self.sc), P(self.sh), in_act, P(self.y), P(self.coef), dy_act, P(self.gy),
                     P(self.dgamma), P(self.dbeta), bn_accumulate, P(self.ws), self.ws_floats * 4)

    def run(self):
        self.native.call("ctvae_conv_wgrad", *self.args)
        return self

    def outputs(self):
        torch.cuda.synchronize()
        host = lambda t: None if t is None else t.cpu()
        tail = self.ws[self.ws_floats:self.ws_floats + (1 << 20)]
        assert untouched(tail), "the call wrote beyond the workspace size it was given"
        return dict(dw=host(self.dw), db=host(self.db), gy=host(self.gy), dgamma=host(self.dgamma), dbeta=host(self.dbeta))

    def all_outputs_untouched(self):
        torch.cuda.synchronize()
        return all(t is None or untouched(t) for t in (self.dw, self.db, self.gy, self.dgamma, self.dbeta)) and untouched(self.ws)


def run_case(native, case, regime, **kw):
    return Call(native, case, regime, **kw).run().outputs()


def check_logged(case, rep, runs=2):
    pl = V.plan(case)
    got, S = labels(rep)
    assert got == {k: runs for k in pl.labels}, (got, pl.labels)
    if pl.family in ("plain", "fast64", "fast128", "wino"):
        assert S == pl.S, (S, pl.S)              # the detailed name carries the split count
    return pl


def check_values(case, regime, out, accumulate=0, what=None):
    """int: bit for bit; randn: inside the bounds.  Returns the largest err/bound (0 for int)."""
    what = what or f"{case.id}/{regime}"
    pl, ref = V.plan(case), ref_of(case, regime)
    want_w, want_b = ref["dw"], ref["db"]
    if accumulate:
        want_w, want_b = want_w + prefill_of(dw_shape(case)).double(), want_b + prefill_of((case.Co,)).double()
    worst = 0.0
    if regime == "int":
        assert V.int_exact_margin(case, ref) + (4.0 / 2 ** 24 if accumulate else 0.0) < 1.0
        exact(f"{what}/dw", out["dw"], want_w)
        if out["db"] is not None:
            exact(f"{what}/db", out["db"], want_b)
        if out["gy"] is not None:
            exact(f"{what}/gy", out["gy"], ref["gy"])
    else:
        bnd = V.bounds(case, pl, ref)
        acc_w = V.U * want_w.abs() if accumulate else 0.0
        acc_b = V.U * want_b.abs() if accumulate else 0.0
        worst = within(f"{what}/dw", out["dw"], want_w, bnd["dw"] + acc_w)
        if out["db"] is not None:
            worst = max(worst, within(f"{what}/db", out["db"], want_b, bnd["db"] + acc_b))
        if out["gy"] is not None:
            within(f"{what}/gy", out["gy"], ref["gy"], ref["gy_slack"] + V.U * ref["gy"].abs() + 1e-300)
    print(f"RATIO {pl.family} {what} {worst:.4f}")
    return worst


def with_winograd(native, case, fn):
    prev = native.winograd_enable(case.wino)
    try:
        return fn()
    finally:
        native.winograd_enable(prev)


# ---------------------------------------------------------------------------------------------------------------------
# every kernel family, geometry and dispatch edge
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["int", "randn"])
@pytest.mark.parametrize("case", V.RUN_CASES, ids=lambda c: c.id)
def test_wgrad_kernels(N, case, regime):
    """Measured on an MI355X: every int case is bit-exact, every randn case inside its bound; the largest err / bound
    (weights and bias together) per kernel family:
      wgrad_fast_kernel<2,2,1,1>     0.114 (g-t-k3s2-512-256: 12 pixels, L = 38), 0.104 (g-linear-b7), 0.088 (g-flat-wide)
      wgrad_kernel<4,1 | 2,2,*,*>    0.047 (g-flat-narrow), 0.033 (n-tt-xf), 0.032 (w-tf-64-66)
      wgrad_fast_kernel<2,2,2,2>     0.0014
      up_wgrad_kernel                0.0076 (up-1tile-xf); g_y written by the DyXform case 0.42 of its slack (5.5e-7 absolute)
      img_enc_wgrad_kernel           0.0045        img_wgrad_kernel    0.0040
      thin_tile_kernel<wgrad>        0.0067 (thin-t64-k4s2)
      wino_wgrad_kernel              0.0013 (against the absolute Winograd sum)
    The bounds are worst-case chains (every rounding in the same direction), so ratios of a few per cent are what correct
    arithmetic gives; the float32 emulations on the host sit at the same ratios.  g-thin-32-3-k3s2 is the case that found
    thin_shape_ok accepting a stride-2 patch of 17 x 65 pixels that launch_thin refused: the call returned -22 instead of
    running the tile kernel (csrc/thin.hip now checks the patch and LDS sizes in thin_shape_ok)."""
    out, rep = with_winograd(N, case, lambda: logged(N, lambda: twice(lambda: run_case(N, case, regime))))
    check_logged(case, rep)
    check_values(case, regime, out)


@pytest.mark.parametrize("bn_accumulate", [0, 1])
def test_encoder_kernel_commits_dgamma_dbeta(N, bn_accumulate):
    """img_enc_wgrad_kernel with DyXform: block 0 commits dgamma / dbeta = (bn_accumulate ? old : 0) + coef rows 5 / 6 -- one
    float32 addition, so the result is the float32 sum bit for bit in both regimes; weight accumulate follows bn_accumulate."""
    case = V.case_by_id("enc-commit")
    for regime in ("int", "randn"):
        out, rep = logged(N, lambda: twice(lambda: run_case(N, case, regime, accumulate=bn_accumulate, bn_accumulate=bn_accumulate)))
        check_logged(case, rep)
        check_values(case, regime, out, accumulate=bn_accumulate, what=f"{case.id}/{regime}/acc{bn_accumulate}")
        coef = inputs_of(case, regime)[3][1]
        base_g, base_b = (prefill_of((case.Co,)), prefill_of((case.Co,)) + 1) if bn_accumulate else (torch.zeros(case.Co), torch.zeros(case.Co))
        assert same(out["dgamma"], base_g + coef[5]) and same(out["dbeta"], base_b + coef[6])
    # without dgamma / dbeta nothing is committed and the weight gradient is the same
    plain = dataclasses.replace(case, dy_out="none")
    assert V.plan(plain).kernel == "img_enc_wgrad_kernel"
    out2 = run_case(N, plain, "int")
    assert out2["dgamma"] is None and same(out2["dw"], run_case(N, case, "int")["dw"])


# ---------------------------------------------------------------------------------------------------------------------
# the slab reduction: small / split / wide x vector / scalar, accumulate 0 / 1, dbias absent
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", V.REDUCE_CASES, ids=lambda c: c.id)
def test_reduction_shapes(N, case, accumulate):
    """accumulate 0 into NaN-prefilled dW / dbias, accumulate 1 onto an integer prefill; int regime bit for bit, randn inside
    the bound (plus one rounding of the accumulating addition)."""
    for regime in ("int", "randn"):
        out, rep = logged(N, lambda: twice(lambda: run_case(N, case, regime, accumulate=accumulate)))
        check_logged(case, rep)
        check_values(case, regime, out, accumulate=accumulate, what=f"{case.id}/{regime}/acc{accumulate}")


@pytest.mark.parametrize("cid", ["f-pow2", "f-s12-1x1", "n-ff-3-5", "g-t-k4s2", "thin-t32-k4s2", "up-1tile", "enc-1tile", "img-1tile"])
def test_no_dbias_no_bias_slab(N, cid):
    """dbias NULL: same weight gradient bit for bit, and the workspace behind the weight slabs -- where the bias slabs of the
    call with dbias lie -- stays untouched: none is written, none reduced."""
    case = V.case_by_id(cid)
    pl = V.plan(case)
    with_b = run_case(N, case, "int")
    call = Call(N, case, "int", bias=False)
    _, rep = logged(N, call.run)
    out = call.outputs()
    got, _ = labels(rep)
    assert got == {k: 1 for k in pl.labels}, got
    assert out["db"] is None and same(out["dw"], with_b["dw"])
    exact(f"{cid}/dw", out["dw"], ref_of(case, "int")["dw"])
    used = pl.S * pl.n
    assert not torch.isnan(call.ws[:used]).any(), "weight slabs not fully written"
    assert untouched(call.ws[used:used + 4 * pl.Sb * case.Co + 1024]), "something was written where the bias slabs would be"


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in V.FALLBACK_CASES if c.rc] + V.ERROR_CASES, ids=lambda c: c.id)
def test_refusals_launch_nothing(N, case):
    call = Call(N, case, "int")
    _, rep = with_winograd(N, case, lambda: logged(N, lambda: fails(N, case.rc, "ctvae_conv_wgrad", *call.args)))
    assert rep == {}, sorted(rep)
    assert call.all_outputs_untouched()


@pytest.mark.parametrize("cid,drop", [("enc-commit", ("dbeta",)), ("enc-commit", ("dgamma",)), ("f-pow2-xf", ("sh",)), ("f-pow2-xf", ("sc",)),
                                      ("up-dyx", ("coef",)), ("up-dyx", ("y",)), ("f-pow2", ("dw",))])
def test_argument_pairs(N, cid, drop):
    """dgamma without dbeta, in_scale without in_shift, dy_bn_y without dy_bn_coef (and the reverse of each), no dw: -22 at the
    top of ctvae_conv_wgrad."""
    case = V.case_by_id(cid)
    call = Call(N, case, "int", drop=drop)
    _, rep = logged(N, lambda: fails(N, V.ERR_BAD_ARG, "ctvae_conv_wgrad", *call.args))
    assert rep == {}, sorted(rep)
    assert call.all_outputs_untouched()


# ---------------------------------------------------------------------------------------------------------------------
# deferred reduction
# ---------------------------------------------------------------------------------------------------------------------
def _defer_sequence(N, regime, arena=None, arena_floats=0):
    """The 13 layers of DEFER_IDS with bias, then DEFER_TWICE again (accumulate 1 onto its first result); returns the calls."""
    lib = N.load()
    seq = [V.case_by_id(i) for i in V.DEFER_IDS]
    calls = []
    ws = nan_ws(N)
    if arena is not None:
        N.check(lib.ctvae_defer_begin(arena.data_ptr(), arena_floats * 4), "ctvae_defer_begin")
    try:
        for c in seq:
            calls.append(Call(N, c, regime, ws=ws, ws_floats=V.DEFER_WS_FLOATS).run())
        if arena is not None:
            assert lib.ctvae_defer_begin(arena.data_ptr(), arena_floats * 4) == V.ERR_BAD_ARG       # one deferral at a time
        first = calls[V.DEFER_IDS.index(V.DEFER_TWICE)]
        again = Call(N, first.case, regime, accumulate=1, ws=ws, ws_floats=V.DEFER_WS_FLOATS)
        again.dw, again.db = first.dw, first.db
        P = N.ptr
        again.args = again.args[:3] + (P(first.dw), P(first.db)) + again.args[5:]
        again.run()
    finally:
        if arena is not None:
            N.check(lib.ctvae_defer_flush(N.stream_ptr()), "ctvae_defer_flush")
    torch.cuda.synchronize()
    return calls


def test_deferred_reduction(N):
    """Between ctvae_defer_begin and ctvae_defer_flush the 13 calls record 26 jobs; the 14th call writes a gradient that has a
    recorded reduction, so the 26 run first (two reduce_multi_kernel launches: 24 + 2) and the 14th reduces at once.  Everything
    is bit-identical to the immediate path and, in the int regime, exact."""
    lib = N.load()
    assert lib.ctvae_defer_flush(N.stream_ptr()) == V.ERR_BAD_ARG            # no deferral open
    for regime in ("int", "randn"):
        now, rep0 = logged(N, lambda: _defer_sequence(N, regime))
        got0, _ = labels(rep0)
        assert got0.get("reduce_partials_kernel") == 14 and "reduce_multi_kernel" not in got0, got0
        arena = full((1 << 23,))
        later, rep = logged(N, lambda: _defer_sequence(N, regime, arena, arena.numel()))
        got, _ = labels(rep)
        assert got.get("reduce_multi_kernel") == 2 and got.get("reduce_partials_kernel") == 1, got
        assert {k: v for k, v in got.items() if not k.startswith("reduce_")} == {k: v for k, v in got0.items() if not k.startswith("reduce_")}
        assert untouched(later[0].ws), "a deferred call wrote slabs into its own workspace"
        for a, b in zip(now, later):
            assert same(a.dw, b.dw) and same(a.db, b.db), a.case.id
        if regime == "int":
            for c in later:
                twice_ = 2.0 if c.case.id == V.DEFER_TWICE else 1.0
                r = ref_of(c.case, "int")
                exact(f"deferred {c.case.id}/dw", c.dw.cpu(), twice_ * r["dw"])
                exact(f"deferred {c.case.id}/db", c.db.cpu(), twice_ * r["db"])
    assert lib.ctvae_defer_flush(N.stream_ptr()) == V.ERR_BAD_ARG


def test_deferred_reduction_small_arena(N):
    """An arena smaller than a call's workspace: that call keeps its own workspace and reduces immediately."""
    lib = N.load()
    case = V.case_by_id("f-pow2")
    arena = full((V.DEFER_WS_FLOATS - 1,))
    N.check(lib.ctvae_defer_begin(arena.data_ptr(), arena.numel() * 4), "ctvae_defer_begin")
    try:
        call = Call(N, case, "int", ws_floats=V.DEFER_WS_FLOATS)
        _, rep = logged(N, call.run)
        got, _ = labels(rep)
        assert got == {k: 1 for k in V.plan(case).labels}, got
        exact("small arena/dw", call.dw.cpu(), ref_of(case, "int")["dw"])
        exact("small arena/db", call.db.cpu(), ref_of(case, "int")["db"])
    finally:
        _, rep = logged(N, lambda: N.check(lib.ctvae_defer_flush(N.stream_ptr()), "ctvae_defer_flush"))
    assert rep == {} and untouched(arena)
