"""GPU: ctvae_conv_forward and ctvae_conv_dgrad (csrc/tapgemm.hip launch_tapgemm) op by op through the C ABI on every dispatch
path -- the Winograd pair, the dedicated image / transposed-conv kernels, the four thin instantiations, the three tile shapes of
the vector kernel (pipelined or not, transform on load or not, unsplit or split-K with splitk_finish_kernel), the five reachable
masked variants, every fall-through and every refusal -- plus ctvae_linear_pixmajor_forward, ctvae_conv_forward_lazy and
ctvae_wino_filters_batch, against the float64 references of tests/conv_checks.py (pinned to torch's float64 conv ops and
autograd, their exactness margins and bounds evaluated in tests/test_conv_reference_host.py).

Every output starts as NaN and the workspace is filled with NaN before every call; the megabyte behind the workspace size a call
was given must stay NaN.  The gathered operand (x, or dy of the data gradient) lies inside a larger NaN-filled allocation, at
least (3*gW + 3)*gC floats before and after it -- the distance the vector kernel's buffer binding reaches in front of the
tensor -- so a gather that reads a neighbour instead of the zero padding shows up as a non-finite output.  Every call runs twice
from scratch: the results must be bit-identical.  Every case asserts through the library's detailed launch log exactly which
kernels ran, the split count (sk=) of the tile kernels and the finish launch, as the mirror of launch_tapgemm's selection in
conv_checks.py predicts.  In the `int` regime the result must equal the reference bit for bit; in the `randn` regime it must lie
inside a bound derived from the length of the float32 addition chains alone, and max err / bound is printed.  No bound was tuned
on these kernels.

tapgemm_masked_kernel<false,true,true> and <true,true,true> are instantiated but cannot be reached from launch_tapgemm (vector
operands on both sides go to the vector kernel); they are not forced here."""
import dataclasses
import re

import pytest
import torch

from tests import conv_checks as C

pytestmark = pytest.mark.gpu

NAN = float("nan")
TAIL = 1 << 20


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import native
    native.load()
    return native


@pytest.fixture(autouse=True)
def direct_kernels(N):
    """Winograd is on by default: every test here runs with it off unless its case switches it on (with_winograd).  A device error
    (not a failed comparison) ends the session: nothing more is started on a GPU that has faulted."""
    prev = N.winograd_enable(False)
    try:
        yield
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:       # pragma: no cover
            pytest.exit(f"device error, stopping: {e}", returncode=3)
    finally:
        N.winograd_enable(prev)


def dev():
    return torch.device("cuda")


def full(shape, fill=NAN):
    return torch.full(shape, fill, dtype=torch.float32, device=dev())


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def untouched(t):
    return bool(torch.isnan(t).all()) and same(t, torch.full_like(t, NAN))


def guarded(t, guard):
    """t on the device inside a NaN-filled allocation, `guard` floats (rounded up to 64) before and after it."""
    gfl = -(-guard // 64) * 64
    buf = full((gfl + t.numel() + gfl,))
    view = buf[gfl:gfl + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


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
    """{kernel label without the shape suffix: count} and the sk= of the detailed names."""
    out, sk = {}, None
    for name, v in rep.items():
        base = name.split(" ")[0]
        out[base] = out.get(base, 0) + v["count"]
        m = re.search(r" sk=(\d+)", name)
        if m:
            sk = int(m.group(1))
    return out, sk


def twice(fn):
    a, b = fn(), fn()
    for k in a:
        assert (a[k] is None and b[k] is None) or same(a[k], b[k]), f"{k}: two runs differ"
    return a


def within(what, got, want, tol):
    got = got.double().reshape(want.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite values"
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


_KEEP = {}


def data_of(case, regime):
    """(inputs, reference) of a case; kept only while small (a few tests share them), never modified."""
    key = (case, regime)
    if key in _KEEP:
        return _KEEP[key]
    inp = C.make_inputs(case, regime)
    ref = C.reference(case, regime, inp)
    if ref["out"].numel() <= 1 << 20:
        _KEEP[key] = (inp, ref)
    return inp, ref


class Call:
    """Device tensors and argument list of one ctvae_conv_forward / ctvae_conv_dgrad call of a case."""

    def __init__(self, native, case, regime, inp, filters_out=None, filters_ready=None, drop=(), kind=None, xf_drop=None):
        self.native, self.case = native, case
        g = case.geom()
        act, xfa, maska = case.acts(regime)
        d = lambda t: None if t is None else t.to(dev())
        self.gbuf, self.G = guarded(inp["G"], (3 * g.gW + 3) * g.gC)
        self.W, self.bias, self.add, self.mask = d(inp["W"]), d(inp["bias"]), d(inp["add"]), d(inp["mask"])
        self.sc = self.sh = None
        if inp["xf"] is not None:
            self.sc, self.sh = d(inp["xf"][0]), d(inp["xf"][1])
        if xf_drop:
            setattr(self, xf_drop, None)
        self.out = full((g.B, g.sH, g.sW, g.sC))
        self.ws = nan_ws(native)
        self.has_ws = case.ws_floats != -1
        self.ws_floats = case.ws() if self.has_ws else 0
        assert self.ws_floats <= self.ws.numel()
        P = native.ptr
        wsp = P(self.ws) if self.has_ws else None
        ptrs = dict(G=P(self.G), W=P(self.W), out=P(self.out))
        for name in drop:
            ptrs[name] = None
        kind = case.kind if kind is None else kind
        shape = (case.B, case.H, case.W, case.Ci, case.Co, case.k, case.s, case.p, case.opad)
        if case.op == "fwd":
            self.name = "ctvae_conv_forward"
            self.args = (kind, ptrs["G"], ptrs["W"], P(self.bias), P(self.add), ptrs["out"], *shape, act, P(self.sc), P(self.sh),
                         max(xfa, 0), P(filters_out), P(filters_ready), wsp, self.ws_floats * 4)
        else:
            self.name = "ctvae_conv_dgrad"
            self.args = (kind, ptrs["G"], ptrs["W"], P(self.add), P(self.mask), max(maska, 0), ptrs["out"], *shape, P(filters_ready),
                         wsp, self.ws_floats * 4)

    def run(self):
        self.native.call(self.name, *self.args)
        return self

    def outputs(self):
        torch.cuda.synchronize()
        tail = self.ws[self.ws_floats:self.ws_floats + TAIL]
        assert untouched(tail), "the call wrote beyond the workspace size it was given"
        if not self.has_ws:
            assert untouched(self.ws[:TAIL]), "a call without a workspace wrote into the library's"
        lo = (self.gbuf.numel() - self.G.numel()) // 2
        assert untouched(self.gbuf[:lo]) and untouched(self.gbuf[lo + self.G.numel():]), "the guards around the gathered operand changed"
        return dict(out=self.out.cpu())

    def all_outputs_untouched(self):
        torch.cuda.synchronize()
        return untouched(self.out) and untouched(self.ws)


def with_winograd(native, on, fn):
    prev = native.winograd_enable(on)
    try:
        return fn()
    finally:
        native.winograd_enable(prev)


def check_logged(sel, rep, runs=2):
    got, sk = labels(rep)
    assert got == {k: runs for k in sel.labels}, (got, sel.labels)
    if sel.sk:
        assert sk == sel.sk, (sk, sel.sk)            # the detailed name of the tile kernel carries the split count
    return got


def check_values(case, regime, sel, out, inp, ref, what=None):
    what = what or f"{case.id}/{regime}"
    worst = 0.0
    if regime == "int":
        assert C.int_exact_margin(case, sel, ref, inp) < 1.0
        exact(what, out, ref["out"])
    else:
        worst = within(what, out, ref["out"], C.bounds(case, sel, ref, inp)["out"])
    print(f"RATIO {sel.family} {what} {worst:.4f} [{' + '.join(sel.labels)}{' sk=%d' % sel.sk if sel.sk else ''}]")
    return worst


def run_and_check(native, case, regime, **kw):
    sel = C.select(case, filters_out=kw.get("filters_out") is not None, filters_ready=kw.get("filters_ready") is not None)
    assert sel.rc == 0
    inp, ref = data_of(case, regime)
    out, rep = with_winograd(native, case.wino, lambda: logged(native, lambda: twice(lambda: Call(native, case, regime, inp, **kw).run().outputs())))
    check_logged(sel, rep)
    check_values(case, regime, sel, out["out"], inp, ref)
    return out["out"]


# ---------------------------------------------------------------------------------------------------------------------
# every kernel family, geometry, epilogue and dispatch edge
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,regime", [(c, r) for c in C.RUN_CASES for r in c.regimes], ids=lambda v: v.id if isinstance(v, C.Case) else v)
def test_conv_kernels(N, case, regime):
    """Forward and data gradient on every path of launch_tapgemm; see RUN_CASES in tests/conv_checks.py for what each case hits.
    Measured on an MI355X: every int case is bit-exact, every randn case inside its bound; the largest err / bound per family:
      tapgemm_fast_kernel 64x64      0.165 (t-pf0: K = 32, L = 36), 0.086 (t-m75-n160), 0.045 (flat-dgrad); split-K cases <= 0.014
      tapgemm_fast_kernel 128x32     0.045 (t-n32-k1-m150)          128x64  0.0024
      tapgemm_masked_kernel          0.121 (m-3-32-24), 0.104 (m-d-3), 0.102 (ft-imgd-mask)
      img_enc_fwd_kernel             0.216 (enc-1025: K = 27)        img_dgrad_kernel   0.155 (imgd-1025)
      img_fwd_kernel                 0.0048                          up_fwd_kernel      0.042 (up-513)
      upimg_fwd_kernel               0.0058                          thin_tile_kernel<fwd>  0.0092 (thin-32-t4)
      wino_conv_kernel / _fs_kernel  0.0038 (against the absolute Winograd sum)
      ctvae_linear_pixmajor_forward  0.018                           ctvae_conv_forward_lazy  0.0029
    The bounds are worst-case chains (every rounding in the same direction), so a reduction of a few dozen terms comes closest;
    the float32 emulations on the host sit at the same ratios.  No case found a wrong value: the upconv + add fall-through
    (64 x 64 tile for N = 32) and H != W are correct."""
    run_and_check(N, case, regime)


@pytest.mark.parametrize("case", C.REFUSED_CASES, ids=lambda c: c.id)
def test_refusals_launch_nothing(N, case):
    """ntaps*gC > 64 on the scalar path, an odd size in the stride-2 data gradient, and the thin shapes with a residual operand:
    launch_thin_forward takes neither `add` nor a mask and -- unlike img_enc / upconv / img_dgrad, which hand such a launch to the
    general kernels -- answers kErrBadArg.  Nothing is launched, nothing written."""
    inp = C.make_inputs(case, "int") if case.geom() is not None else _inputs_without_geometry(case)
    call = _refused_call(N, case, inp)
    _, rep = logged(N, lambda: fails(N, case.rc, call.name, *call.args))
    assert rep == {}, sorted(rep)
    assert call.all_outputs_untouched()


def _inputs_without_geometry(case):
    """A case build_geom refuses has no geometry to size its tensors by: the layer's own shapes."""
    Ho, Wo = (case.H + 2 * case.p - case.k) // case.s + 1, (case.W + 2 * case.p - case.k) // case.s + 1
    G = torch.ones(case.B, Ho, Wo, case.Co) if case.op == "dgrad" else torch.ones(case.B, case.H, case.W, case.Ci)
    return dict(G=G, W=torch.ones(C.w_shape(case)), bias=None, add=None, mask=None, xf=None)


class _RawCall:
    """A call whose geometry the library refuses: plain tensors, no mirror."""

    def __init__(self, native, case, inp):
        P = native.ptr
        self.G, self.W = inp["G"].to(dev()), inp["W"].to(dev())
        self.out = full((case.B, case.H, case.W, case.Ci) if case.op == "dgrad" else (case.B, 64, 64, case.Co))
        self.ws = nan_ws(native)
        shape = (case.B, case.H, case.W, case.Ci, case.Co, case.k, case.s, case.p, case.opad)
        if case.op == "fwd":
            self.name = "ctvae_conv_forward"
            self.args = (case.kind, P(self.G), P(self.W), None, None, P(self.out), *shape, 0, None, None, 0, None, None, P(self.ws),
                         self.ws.numel() * 4)
        else:
            self.name = "ctvae_conv_dgrad"
            self.args = (case.kind, P(self.G), P(self.W), None, None, 0, P(self.out), *shape, None, P(self.ws), self.ws.numel() * 4)

    def all_outputs_untouched(self):
        torch.cuda.synchronize()
        return untouched(self.out) and untouched(self.ws)


def _refused_call(native, case, inp):
    return Call(native, case, "int", inp) if case.geom() is not None else _RawCall(native, case, inp)


# ---------------------------------------------------------------------------------------------------------------------
# argument refusals
# ---------------------------------------------------------------------------------------------------------------------
T64 = "t-64-128-sk4"


@pytest.mark.parametrize("what", ["no-x", "no-w", "no-y", "kind-2", "kind-convt-ci-tap", "scale-only", "shift-only", "xf-enc", "xf-wino",
                                  "filters-out-direct", "filters-ready-direct", "d-no-dy", "d-no-dx", "d-kind-7", "d-filters-direct",
                                  "taps-below-minus-3"])
def test_argument_refusals(N, what):
    """-22 before anything is launched, outputs and workspace untouched: null pointers, a bad kind, one of in_scale / in_shift
    alone, the transform on load where ctvae_conv_input_transform_supported says 0 (the encoder's image conv; a Winograd shape,
    which the vector kernel would otherwise have taken with the transform), Winograd filter pointers on a shape that does not
    run Winograd, tap offsets outside [-3, 4]."""
    by = C.case_by_id
    wino = False
    kw = {}
    case = by(T64)
    if what in ("no-x", "d-no-dy"):
        kw = dict(drop=("G",))
    elif what == "no-w":
        kw = dict(drop=("W",))
    elif what in ("no-y", "d-no-dx"):
        kw = dict(drop=("out",))
    elif what == "kind-2":
        kw = dict(kind=2)
    elif what == "kind-convt-ci-tap":
        kw = dict(kind=C.CONVT | C.W_CI_TAP)
    elif what == "d-kind-7":
        kw = dict(kind=7)
    elif what in ("scale-only", "shift-only"):
        case = by("t-xf-lrelu")
        kw = dict(xf_drop="sh" if what == "scale-only" else "sc")
    elif what == "xf-enc":
        case = dataclasses.replace(by("enc-1tile"), xf=C.ACT_LRELU)
    elif what == "xf-wino":
        case, wino = dataclasses.replace(by("w-fs-b16"), xf=C.ACT_LRELU), True
        assert C.select(dataclasses.replace(case, wino=False)).labels == [C.FK(2, 2, 1, False, 3, True)]      # taken with Winograd off
    elif what == "taps-below-minus-3":
        case = C.Case("taps", "k4 p4: offsets down to -4", "fwd", C.CONV, 2, 8, 8, 64, 64, 4, 1, 4)
    if what.startswith("d-"):
        case = by("d-s1")
    filt = full((16 * 64 * 128,)) if "filters" in what else None
    if what == "filters-out-direct":
        kw = dict(filters_out=filt)
    elif what in ("filters-ready-direct", "d-filters-direct"):
        kw = dict(filters_ready=filt)
    if what in ("xf-enc", "xf-wino", "taps-below-minus-3") or "filters" in what:
        assert C.select(case, filters_out="out" in what, filters_ready="ready" in what or what == "d-filters-direct").rc == C.ERR_BAD_ARG
    call = Call(N, case, "int", C.make_inputs(case, "int"), **kw)
    _, rep = with_winograd(N, wino, lambda: logged(N, lambda: fails(N, C.ERR_BAD_ARG, call.name, *call.args)))
    assert rep == {}, sorted(rep)
    assert call.all_outputs_untouched()
    assert filt is None or untouched(filt)


# ---------------------------------------------------------------------------------------------------------------------
# Winograd filter hand-overs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["int", "randn"])
def test_winograd_filter_handover(N, regime):
    """wino_dgrad_filters_out: the forward's transform launch becomes wino_weight2_kernel and leaves the data gradient's filters;
    a data gradient fed those filters launches no transform and equals one that transforms its own bit for bit.
    ctvae_wino_filters_batch: both sets of a layer in one launch; a forward fed wino_fwd_filters launches no transform."""
    fwd, dgr = C.case_by_id("w-fs-b16"), C.case_by_id("w-dgrad")
    nfl = 16 * 64 * 64
    assert C.wino_filter_floats(fwd, True) == nfl
    lib = N.load()
    prev = N.winograd_enable(True)
    try:
        assert lib.ctvae_conv_wino_filter_floats(*fwd.args(), C.WS_BYTES) == nfl
    finally:
        N.winograd_enable(prev)
    bwd_filters = full((nfl + 64,))
    y_plain = run_and_check(N, fwd, regime)
    y_two = run_and_check(N, fwd, regime, filters_out=bwd_filters)
    assert untouched(bwd_filters[nfl:]) and not torch.isnan(bwd_filters[:nfl]).any()
    assert same(y_plain, y_two), "the forward result depends on which kernel transformed its filters"
    # the same weights in both cases?  The data gradient takes the forward's weights: run it on them
    inp_f, _ = data_of(fwd, regime)
    dgr_w = dataclasses.replace(dgr, id="w-dgrad-shared-" + regime)
    inp_d = dict(C.make_inputs(dgr, regime), W=inp_f["W"])
    ref_d = C.reference(dgr_w, regime, inp_d)
    outs = {}
    for name, ready in (("own", None), ("fed", bwd_filters)):
        sel = C.select(dgr_w, filters_ready=ready is not None)
        out, rep = with_winograd(N, True, lambda: logged(N, lambda: twice(lambda: Call(N, dgr_w, regime, inp_d, filters_ready=ready).run().outputs())))
        check_logged(sel, rep)
        check_values(dgr_w, regime, sel, out["out"], inp_d, ref_d, what=f"w-dgrad/{name}/{regime}")
        outs[name] = out["out"]
    assert same(outs["own"], outs["fed"]), "a data gradient fed the forward's filters differs from one that transforms its own"
    # ctvae_wino_filters_batch
    import ctypes
    W = inp_f["W"].to(dev())
    uf, ub = full((nfl + 64,)), full((nfl + 64,))
    arr = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
    ints = lambda v: (ctypes.c_int * 1)(v)
    keep = (arr(W), arr(uf), arr(ub), ints(64), ints(64))
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    _, rep = logged(N, lambda: N.call("ctvae_wino_filters_batch", 1, *(cast(a) for a in keep)))
    assert labels(rep)[0] == {"wino_weight2_batch_kernel": 1}
    assert untouched(uf[nfl:]) and untouched(ub[nfl:]) and not torch.isnan(uf[:nfl]).any()
    assert same(ub, bwd_filters), "the batch launch and the forward's own transform leave different data-gradient filters"
    y_fed = run_and_check(N, fwd, regime, filters_ready=uf)
    assert same(y_fed, y_plain)


# ---------------------------------------------------------------------------------------------------------------------
# ctvae_linear_pixmajor_forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["int", "randn"])
def test_linear_pixmajor(N, regime):
    """nn.Linear(Ci, C*P) written as the NHWC tensor [B, P, C]: column c*P + p goes to pixel p, channel c.  _supported is 1 for the
    unsplit vector kernel only: 0 for Ci % 32, P = 1 and a plan that splits K; the forward refuses the same shapes."""
    lib = N.load()
    for B, Ci, Cc, P, wsf, ok in C.PIXMAJOR:
        assert C.linear_pixmajor_supported(B, Ci, Cc, P, wsf) == ok
        assert bool(lib.ctvae_linear_pixmajor_supported(B, Ci, Cc, P, wsf * 4)) == ok, (B, Ci, Cc, P, wsf)
        gen = torch.Generator().manual_seed(Ci + P)
        if regime == "int":
            x, w, b = (torch.randint(-4, 5, s, generator=gen).float() for s in ((B, Ci), (Ci, Cc * P), (Cc * P,)))
        else:
            x, w, b = (torch.randn(s, generator=gen) for s in ((B, Ci), (Ci, Cc * P), (Cc * P,)))
        act = C.ACT_RELU if regime == "int" else C.ACT_LRELU

        def once():
            ws = nan_ws(N)
            xbuf, xd = guarded(x, 6 * Ci)
            y, wd, bd = full((B, P, Cc)), w.to(dev()), b.to(dev())
            args = (N.ptr(xd), N.ptr(wd), N.ptr(bd), N.ptr(y), B, Ci, Cc, P, act, N.ptr(ws) if wsf else None, wsf * 4)
            if ok:
                N.call("ctvae_linear_pixmajor_forward", *args)
            else:
                fails(N, C.ERR_BAD_ARG, "ctvae_linear_pixmajor_forward", *args)
            torch.cuda.synchronize()
            assert untouched(ws[wsf:wsf + TAIL]) and (ok or (untouched(y) and untouched(ws)))
            return dict(y=y.cpu())
        out, rep = logged(N, lambda: twice(once))
        if not ok:
            assert rep == {}
            continue
        got, sk = labels(rep)
        assert got == {C.FK(2, 2, 1, False, 3): 2} and sk == 1, (got, sk)
        pre = C.pixmajor_ref(x, w, b, Cc, P)
        want = C.act64(pre, act)
        if regime == "int":
            exact(f"pixmajor/{Ci}", out["y"], want)
        else:
            asum = C.pixmajor_ref(x.abs(), w.abs(), b.abs(), Cc, P)
            within(f"pixmajor/{Ci}", out["y"], want, C.gamma(Ci + 1 + 3) * asum + C.U * want.abs() + 1e-300)


# ---------------------------------------------------------------------------------------------------------------------
# ctvae_conv_forward_lazy
# ---------------------------------------------------------------------------------------------------------------------
def _lazy_args(N, case, x, w, slices, ws, ws_floats):
    return (case.kind, N.ptr(x), N.ptr(w), N.ptr(slices), case.B, case.H, case.W, case.Ci, case.Co, case.k, case.s, case.p, case.opad,
            N.ptr(ws), ws_floats * 4)


@pytest.mark.parametrize("case,n", C.LAZY_CASES, ids=lambda v: v.id if isinstance(v, C.Case) else str(v))
def test_forward_lazy_slices(N, case, n):
    """The raw K slices [S][B*Ho*Wo][Co] of a split layer, without bias or activation: their float64 sum is the pre-bias sum of
    the reference (a dense layer and a 4-class transposed one); no finishing launch, nothing in the workspace."""
    lib = N.load()
    assert C.lazy_slices(case) == n and lib.ctvae_conv_forward_lazy_slices(*case.args(), C.WS_BYTES) == n
    g, sel = case.geom(), C.select(case)
    per = g.B * g.sH * g.sW * g.sC
    for regime in ("int", "randn"):
        inp, ref = data_of(case, regime)

        def once():
            ws = nan_ws(N)
            xbuf, x = guarded(inp["G"], (3 * g.gW + 3) * g.gC)
            slices, wd = full((n * per + TAIL,)), inp["W"].to(dev())
            N.call("ctvae_conv_forward_lazy", *_lazy_args(N, case, x, wd, slices, ws, ws.numel()))
            torch.cuda.synchronize()
            assert untouched(ws) and untouched(slices[n * per:])
            return dict(slices=slices[:n * per].cpu())
        out, rep = logged(N, lambda: twice(once))
        got, sk = labels(rep)
        assert got == {sel.labels[-1]: 2} and sk == n, (got, sk)
        parts = out["slices"].view(n, g.B, g.sH, g.sW, g.sC).double()
        assert torch.isfinite(parts).all()
        total = parts.sum(0)
        if regime == "int":
            exact(f"lazy {case.id}", total, ref["sum"])
        else:
            inp_nb = dict(inp, bias=None)
            asum = C.reference(dataclasses.replace(case, bias=False), regime, inp_nb)["asum"]
            within(f"lazy {case.id}", total, ref["sum"], C.gamma(g.Kmax + 1) * asum + 1e-300)


@pytest.mark.parametrize("cid", C.LAZY_REFUSED)
def test_forward_lazy_refuses_unsplit_shapes(N, cid):
    """Where ctvae_conv_forward_lazy_slices answers 0 (unsplit, no workspace to split into, thin, dedicated, Winograd) there is no
    slice to write: the call returns -22 before any launch.  (It used to launch such a shape with a null output pointer.)"""
    case = C.case_by_id(cid)
    g = case.geom()
    lib = N.load()
    inp = C.make_inputs(case, "int")
    x, w = inp["G"].to(dev()), inp["W"].to(dev())
    slices = full((2 * g.B * g.sH * g.sW * g.sC,))
    ws = nan_ws(N)
    wsf = case.ws() if case.ws_floats != -1 else 0

    def go():
        assert lib.ctvae_conv_forward_lazy_slices(*case.args(), wsf * 4) == 0
        fails(N, C.ERR_BAD_ARG, "ctvae_conv_forward_lazy", *_lazy_args(N, case, x, w, slices, ws, wsf))
    _, rep = with_winograd(N, case.wino, lambda: logged(N, go))
    assert rep == {}, sorted(rep)
    torch.cuda.synchronize()
    assert untouched(slices) and untouched(ws)
