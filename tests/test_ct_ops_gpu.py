"""GPU: the causal-transition kernels (csrc/glinear.hip, gatlayer.hip, ctmisc.hip, pairmlp.hip) op by op through the C ABI,
against the float64 references of tests/ct_ops_checks.py (pinned to the torch paths, and their input conditions evaluated, in
tests/test_ct_ops_reference_host.py).

Every output, scratch and padding element starts as NaN (floats) or -1 (ints); what a call must not touch has to hold that fill
bit for bit afterwards.  Every op runs twice into fresh buffers and the two results must be identical (the header promises
deterministic results without atomics).  Tolerances are: exact (integer data, hard samples, fills), the derived float32
dot-product bound (ct_ops_checks.dot_bound), or the tolerance the project already uses for the kernel family (named where used).
"""
import ctypes

import pytest
import torch

from tests import ct_ops_checks as V

pytestmark = pytest.mark.gpu

NAN = float("nan")
# gat_layer: |got - want| <= GAT_FACTOR * (atol + rtol |want|) with the tolerances of test_ct_gpu.test_gat_score_kernel_and_layer
# (output 2e-5 / 1e-4; gradients 1e-4 * max(1, |want|_inf) / 1e-3).
GAT_FACTOR = 1.0


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import native
    native.load()
    return native


def dev():
    return torch.device("cuda")


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    """Bit-identical, NaN fills included."""
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def untouched(t, fill=NAN):
    return same(t, torch.full_like(t, fill))


def twice(fn):
    """fn() -> dict of host tensors (None allowed); run twice into fresh buffers: identical."""
    a, b = fn(), fn()
    for k in a:
        assert (a[k] is None and b[k] is None) or same(a[k], b[k]), f"{k}: two runs differ"
    return a


def logged(native, fn, detailed=False):
    native.prof_report()
    native.prof_enable(True, detailed=detailed)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    return out, native.prof_report()


def rows_buf(t, ld, fill=NAN):
    """t [..., w] -> device buffer [rows, ld] with t in the first w columns and `fill` behind them."""
    w = t.shape[-1]
    buf = torch.full((t.numel() // w, ld), fill, dtype=torch.float32, device=dev())
    buf[:, :w] = t.reshape(-1, w).to(dev())
    return buf


def full(shape, fill=NAN, dtype=torch.float32):
    return torch.full(shape, fill, dtype=dtype, device=dev())


def fails(native, code, name, *args):
    with pytest.raises(RuntimeError, match=rf"{name} failed.*\(code {code}\)"):
        native.call(name, *args)


def within(what, got, want, tol):
    """|got - want| <= tol elementwise; prints the largest ratio."""
    got = got.double()
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    err = (got - want).abs()
    ratio = float((err / tol.clamp(min=1e-300)).max()) if err.numel() else 0.0
    ok = bool((err <= tol).all())
    print(f"{what}: max |err| {float(err.max()) if err.numel() else 0.0:.3e}, max |err| / tol = {ratio:.4f}")
    assert ok, f"{what}: {int((err > tol).sum())} of {err.numel()} elements beyond the tolerance, worst ratio {ratio:.3f}"
    return ratio


def tol_of(want, atol, rtol, scaled=False):
    a = atol * max(1.0, float(want.abs().max())) if scaled else atol
    return a + rtol * want.abs()


# ---------------------------------------------------------------------------------------------------------------------
# glinear
# ---------------------------------------------------------------------------------------------------------------------
class GL:
    """Device buffers and host pointer arrays of one glinear case."""

    def __init__(self, case, inp):
        self.case, self.inp = case, inp
        K, Nn, nseg = case.K, case.N, case.nseg
        self.ldx, self.ldy = K + case.xpad, nseg * Nn + case.ypad
        self.x = rows_buf(inp["x"], self.ldx)
        self.dy = rows_buf(inp["dy"], self.ldy)
        self.W, self.b, self.g = [], [], []
        for s, (W, b, grp) in zip(case.segs, inp["banks"]):
            Wd = full(tuple(W.shape))                                  # only the K used columns of the used rows hold numbers
            used = range(s.G - 1) if s.spare else range(s.G)
            for gi in used:
                Wd[gi, :, s.koff:s.koff + K] = W[gi, :, s.koff:s.koff + K].to(dev())
            bd = None
            if b is not None:
                bd = full(tuple(b.shape))
                for gi in used:
                    bd[gi] = b[gi].to(dev())
            self.W.append(Wd), self.b.append(bd), self.g.append(None if grp is None else grp.to(dev()))
        C = ctypes
        self.host = ((C.c_void_p * nseg)(*[W.data_ptr() + 4 * s.koff for W, s in zip(self.W, case.segs)]),
                     (C.c_int * nseg)(*[W.stride(1) for W in self.W]),
                     (C.c_int64 * nseg)(*[W.stride(0) for W in self.W]),
                     (C.c_void_p * nseg)(*[None if b is None else b.data_ptr() for b in self.b]),
                     (C.c_int * nseg)(*[0 if b is None else b.shape[-1] for b in self.b]),
                     (C.c_void_p * nseg)(*[None if g is None else g.data_ptr() for g in self.g]))

    def forward(self, native):
        c, h = self.case, self.host
        y = full((c.B * 64, self.ldy))
        native.call("ctvae_glinear_forward", self.x.data_ptr(), self.ldx, c.K, c.nseg, c.N, h[0], h[1], h[2], h[3], h[4], h[5],
                    y.data_ptr(), self.ldy, c.B)
        torch.cuda.synchronize()
        return y.cpu()

    def dgrad(self, native):
        c, h = self.case, self.host
        dx = full((c.B * 64, self.ldx))
        native.call("ctvae_glinear_dgrad", self.dy.data_ptr(), self.ldy, c.nseg, c.N, h[0], h[1], h[2], h[5], dx.data_ptr(), self.ldx,
                    c.K, c.B)
        torch.cuda.synchronize()
        return dx.cpu()

    def wgrad(self, native, si, accumulate, prefill, with_bias=True, ws_short=0):
        """Segment si: dW into a bank-shaped buffer [G,N,ldw] at column koff (ldo = ldw), dbias [G,N] or NULL."""
        c, s = self.case, self.case.segs[si]
        Gk = s.G if s.grouped else 1
        S = V.gl_slices(c.B, Gk, s.grouped)
        nbytes = native.load().ctvae_glinear_wgrad_ws_bytes(Gk, c.N, c.K, c.B, int(s.grouped))      # the public query is exact
        assert nbytes == 4 * V.gl_ws_floats(Gk, c.N, c.K, S), (nbytes, S)
        ws = full((nbytes // 4,))
        dW = full(tuple(self.W[si].shape), prefill)
        db = full((s.G, c.N), prefill) if (s.bias and with_bias) else None
        native.call("ctvae_glinear_wgrad", self.x.data_ptr(), self.ldx, c.K, self.dy.data_ptr(), self.ldy, si * c.N, c.N,
                    None if self.g[si] is None else self.g[si].data_ptr(), Gk, c.B, dW.data_ptr() + 4 * s.koff, dW.stride(1),
                    None if db is None else db.data_ptr(), accumulate, ws.data_ptr(), (ws.numel() - ws_short) * 4)
        torch.cuda.synchronize()
        return dW.cpu(), None if db is None else db.cpu()


def gl_check(case, kind, what, got, want, L, abs_sum):
    if kind == "int":
        bad = got.double() != want
        assert not bool(bad.any()), f"{case.id}/{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at " \
                                    f"{bad.nonzero()[0].tolist()}: {float(got[bad][0])} want {float(want[bad][0])}"
    else:
        within(f"glinear {case.id}/{what}", got, want, V.dot_bound(L, abs_sum))


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("case", V.GL_CASES, ids=lambda c: c.id)
def test_glinear_three_directions(N, case, kind):
    inp = V.gl_inputs(case, kind)
    ref = V.glinear_ref(case, inp)
    K, Nn, nseg, B = case.K, case.N, case.nseg, case.B

    def run():
        gl = GL(case, inp)
        out = dict(y=gl.forward(N), dx=gl.dgrad(N))
        for si, s in enumerate(case.segs):
            out[f"dW{si}"], out[f"db{si}"] = gl.wgrad(N, si, 0, NAN)
            out[f"aW{si}"], out[f"ab{si}"] = gl.wgrad(N, si, 1, 0.125 if kind == "int" else 0.5)
        return out
    (got, rep) = logged(N, lambda: twice(run), detailed=True)
    labels = [k for k in rep if k.startswith("glinear_wgrad_kernel")]
    for si, s in enumerate(case.segs):
        Gk = s.G if s.grouped else 1
        S = V.gl_slices(B, Gk, s.grouped)
        assert f"glinear_wgrad_kernel K={K} N={Nn} G={Gk} S={S} grp={int(s.grouped)}" in labels, (si, labels)
    if case.id in V.GL_EXPECT_S:
        assert [int(k.split(" S=")[1].split()[0]) for k in labels] == [V.GL_EXPECT_S[case.id]], labels
    assert f"glinear_fwd_kernel K={K} N={Nn} nseg={nseg}" in rep and "glinear_dgrad_kernel" in rep and "glinear_reduce_kernel" in rep
    # forward
    y = got["y"]
    assert untouched(y[:, nseg * Nn:]), "ldy padding written"
    gl_check(case, kind, "y", y[:, :nseg * Nn].reshape(B, 64, -1), ref["y"], K, ref["y_abs"])
    # data gradient
    dx = got["dx"]
    assert untouched(dx[:, K:]), "ldx padding written"
    gl_check(case, kind, "dx", dx[:, :K].reshape(B, 64, K), ref["dx"], nseg * Nn, ref["dx_abs"])
    # weight / bias gradient per segment
    pre = 0.125 if kind == "int" else 0.5
    for si, s in enumerate(case.segs):
        Gk = s.G if s.grouped else 1
        S = V.gl_slices(B, Gk, s.grouped)
        L = (ref["rows"][si] + S)[:Gk]
        for tag, fill, add in (("dW", NAN, 0.0), ("aW", pre, pre)):
            dW = got[f"{tag}{si}"]
            inside = dW[:Gk, :, s.koff:s.koff + K]
            outside = dW.clone()
            outside[:Gk, :, s.koff:s.koff + K] = fill
            assert untouched(outside, fill), f"{tag}{si}: written outside the K columns of the {Gk} groups"
            gl_check(case, kind, f"{tag}{si}", inside, ref["dW"][si][:Gk] + add, (L + (1 if add else 0))[:, None, None],
                     ref["dW_abs"][si][:Gk] + abs(add))
            if s.spare:                                                # nobody uses the last row: exactly 0 / left unchanged
                assert bool((inside[-1] == add).all())
            db = got[f"{tag.replace('W', 'b')}{si}"]
            assert (db is None) == (not s.bias)
            if db is not None:
                assert untouched(db[Gk:], fill)
                gl_check(case, kind, f"{tag}{si} bias", db[:Gk], ref["db"][si][:Gk] + add, (L + (1 if add else 0))[:, None],
                         ref["db_abs"][si][:Gk] + abs(add))


def test_glinear_wgrad_null_bias_short_workspace_and_bad_arguments(N):
    case = V.case_of(V.GL_CASES, "K36-N12-s2")
    inp = V.gl_inputs(case, "int")
    ref = V.glinear_ref(case, inp)
    gl = GL(case, inp)
    s = case.segs[1]
    dW, db = gl.wgrad(N, 1, 0, NAN, with_bias=False)                  # dbias = NULL on a segment that has a bias
    assert db is None and torch.equal(dW[:, :, s.koff:s.koff + case.K].double(), ref["dW"][1])

    # a workspace one float short of the public query: the workspace error, no launch, dW / dbias untouched -- at S = 1 and S = 2
    for cid, si in (("K36-N12-s2", 1), ("B19-S2", 0)):
        c2 = V.case_of(V.GL_CASES, cid)
        g2 = gl if cid == case.id else GL(c2, V.gl_inputs(c2, "int"))
        s2 = c2.segs[si]
        Gk = s2.G if s2.grouped else 1
        nbytes = N.load().ctvae_glinear_wgrad_ws_bytes(Gk, c2.N, c2.K, c2.B, int(s2.grouped))
        S2 = V.gl_slices(c2.B, Gk, s2.grouped)
        assert S2 == (2 if cid == "B19-S2" else 1) and nbytes == 4 * V.gl_ws_floats(Gk, c2.N, c2.K, S2)
        ws2, dW2, db2 = full((nbytes // 4,)), full((s2.G, c2.N, c2.K)), full((s2.G, c2.N))
        args = [g2.x.data_ptr(), g2.ldx, c2.K, g2.dy.data_ptr(), g2.ldy, si * c2.N, c2.N, N.ptr(g2.g[si]), Gk, c2.B, dW2.data_ptr(), c2.K,
                db2.data_ptr(), 0, ws2.data_ptr()]
        _, rep = logged(N, lambda: fails(N, V.ERR_WORKSPACE, "ctvae_glinear_wgrad", *args, nbytes - 4))
        assert rep == {}, sorted(rep)
        torch.cuda.synchronize()
        assert untouched(dW2.cpu()) and untouched(db2.cpu()) and untouched(ws2.cpu())
        N.call("ctvae_glinear_wgrad", *args, nbytes)                      # exactly the query's size is accepted
        torch.cuda.synchronize()
        assert torch.equal(dW2.cpu().double(), V.glinear_ref(c2, g2.inp)["dW"][si])
    # the launcher refuses what would read or write out of bounds, before any launch (each dW stays untouched)
    c = case
    dWb = full((s.G, c.N, c.K))
    ws = full((4096,))
    ok = [gl.x.data_ptr(), gl.ldx, c.K, gl.dy.data_ptr(), gl.ldy, c.N, c.N, gl.g[1].data_ptr(), s.G, c.B, dWb.data_ptr(), c.K, None, 0,
          ws.data_ptr(), ws.numel() * 4]

    def bad():
        for pos, val in ((1, c.K - 4), (4, c.N), (4, 2 * c.N - 4), (11, c.K - 4), (2, c.K + 2), (6, c.N + 2), (5, 6), (1, gl.ldx + 2)):
            a = list(ok)
            a[pos] = val
            fails(N, V.ERR_BAD_ARG, "ctvae_glinear_wgrad", *a)
        h = gl.host
        fails(N, V.ERR_BAD_ARG, "ctvae_glinear_forward", gl.x.data_ptr(), c.K - 4, c.K, c.nseg, c.N, h[0], h[1], h[2], h[3], h[4], h[5],
              dWb.data_ptr(), gl.ldy, c.B)
        fails(N, V.ERR_BAD_ARG, "ctvae_glinear_forward", gl.x.data_ptr(), gl.ldx, c.K, c.nseg, c.N, h[0], h[1], h[2], h[3], h[4], h[5],
              dWb.data_ptr(), c.nseg * c.N - 4, c.B)
        fails(N, V.ERR_BAD_ARG, "ctvae_glinear_forward", gl.x.data_ptr(), gl.ldx, c.K, 5, c.N, h[0], h[1], h[2], h[3], h[4], h[5],
              dWb.data_ptr(), gl.ldy, c.B)
    _, rep = logged(N, bad)
    assert rep == {}, sorted(rep)
    torch.cuda.synchronize()
    assert untouched(dWb.cpu())


# ---------------------------------------------------------------------------------------------------------------------
# fused GATv2 layer
# ---------------------------------------------------------------------------------------------------------------------
def run_gat(native, case, inp, adj=None):
    B, Hs, C = case.B, case.Hs, case.C
    w = Hs * C
    ld, ldo, ldd = 2 * w + case.ldpad, w + case.opad, 2 * w + case.dpad
    xlr = rows_buf(torch.cat([inp["xl"].reshape(B, 64, w), inp["xr"].reshape(B, 64, w)], -1), ld)
    adj_d = (inp["adj"] if adj is None else adj).contiguous().to(dev())
    we, att, bias = (inp[k].contiguous().to(dev()) for k in ("we", "att", "bias"))
    hm = None if inp["head_map"] is None else inp["head_map"].contiguous().to(dev())
    out, alpha = full((B * 64, ldo)), full((B, Hs, 64, 64))
    native.call("ctvae_gat_layer_forward", xlr.data_ptr(), xlr.data_ptr() + 4 * w, ld, adj_d.data_ptr(), we.data_ptr(), att.data_ptr(),
                bias.data_ptr(), native.ptr(hm), out.data_ptr(), ldo, alpha.data_ptr(), B, Hs, C, V.SLOPE_GAT, case.act)
    g_out = rows_buf(inp["g_out"].reshape(B, 64, w), ldo)
    dS, dattr = full((B, Hs, 64, 64)), full((B, Hs, 64, 64))
    d_xlr = full((B * 64, ldd))
    parts = full((3, B, Hs, C))
    dadj = None if case.dadj == "null" else (inp["dadj0"].to(dev()).clone() if case.dadj == "acc" else full((B, 64, 64)))
    native.call("ctvae_gat_layer_backward", xlr.data_ptr(), xlr.data_ptr() + 4 * w, ld, adj_d.data_ptr(), we.data_ptr(), att.data_ptr(),
                bias.data_ptr(), native.ptr(hm), out.data_ptr(), ldo, alpha.data_ptr(), g_out.data_ptr(), dS.data_ptr(), dattr.data_ptr(),
                d_xlr.data_ptr(), d_xlr.data_ptr() + 4 * w, ldd, parts[0].data_ptr(), parts[1].data_ptr(), parts[2].data_ptr(),
                native.ptr(dadj), 1 if case.dadj == "acc" else 0, B, Hs, C, V.SLOPE_GAT, case.act)
    torch.cuda.synchronize()
    return dict(out=out.cpu(), alpha=alpha.cpu(), d_xlr=d_xlr.cpu(), parts=parts.cpu(), dadj=None if dadj is None else dadj.cpu())


@pytest.mark.parametrize("case", V.GAT_CASES, ids=lambda c: c.id)
def test_gat_layer(N, case):
    inp = V.gat_inputs(case)
    ref = V.gat_layer_ref(inp["xl"], inp["xr"], inp["adj"], inp["we"], inp["att"], inp["bias"], inp["head_map"], V.SLOPE_GAT, case.act,
                          inp["g_out"])
    got, rep = logged(N, lambda: twice(lambda: run_gat(N, case, inp)))
    tag = "[C<=64]" if case.C <= 64 else "[C>64]"
    want_labels = {"gat_layer_fwd_kernel" + tag, "gat_layer_bwd_kernel" + tag, "gat_proj_bwd_kernel"} | \
        (set() if case.dadj == "null" else {"gat_adj_reduce_kernel"})
    assert set(rep) == want_labels, sorted(rep)
    B, Hs, C = case.B, case.Hs, case.C
    w = Hs * C
    ratios = []
    # forward
    assert untouched(got["out"][:, w:]), "ldo padding written"
    alpha = got["alpha"].double()
    keep = ref["keep"][:, None].expand_as(alpha)
    assert float(alpha[~keep].abs().sum()) == 0.0, "alpha must be exactly 0 on dropped pairs"
    assert float((alpha.sum(2) - 1).abs().max()) <= 64 * V.EPS32, "alpha columns sum to 1"
    ratios.append(within(f"gat {case.id}/alpha", alpha, ref["alpha"], GAT_FACTOR * tol_of(ref["alpha"], 2e-5, 1e-4)))
    out = got["out"][:, :w].reshape(B, 64, Hs, C)
    ratios.append(within(f"gat {case.id}/out", out, ref["out"], GAT_FACTOR * tol_of(ref["out"], 2e-5, 1e-4)))
    for b, kind in enumerate(case.graphs):
        if kind == "empty":                                                # only the self loop: alpha = I, out = act(xl + bias)
            assert torch.equal(got["alpha"][b], torch.eye(64).expand(Hs, 64, 64))
            hm = inp["head_map"][b].long() if inp["head_map"] is not None else torch.arange(Hs)
            v = inp["xl"][b] + inp["bias"][hm][None]
            assert torch.equal(out[b], torch.where(v > 0, v, v * V.LEAKY) if case.act else v)
    # backward
    ldd = 2 * w + case.dpad
    assert untouched(got["d_xlr"][:, 2 * w:]), "ldd padding written"
    d_xl, d_xr = got["d_xlr"][:, :w].reshape(B, 64, Hs, C), got["d_xlr"][:, w:2 * w].reshape(B, 64, Hs, C)
    for name, g_, want in (("d_xl", d_xl, ref["d_xl"]), ("d_xr", d_xr, ref["d_xr"]), ("d_bias", got["parts"][0], ref["d_bias"]),
                           ("d_att", got["parts"][1], ref["d_att"]), ("d_we", got["parts"][2], ref["d_we"])):
        ratios.append(within(f"gat {case.id}/{name}", g_, want, GAT_FACTOR * tol_of(want, 1e-4, 1e-3, scaled=True)))
    idx = torch.arange(64)
    if case.dadj == "null":
        assert got["dadj"] is None
    else:
        base = V.d(inp["dadj0"]) if case.dadj == "acc" else torch.zeros(B, 64, 64, dtype=torch.float64)
        # accumulate: the project tolerance is taken of the quantity compared, old values + gradient
        ratios.append(within(f"gat {case.id}/d_adj", got["dadj"], ref["d_adj"] + base,
                             GAT_FACTOR * tol_of(ref["d_adj"] + base, 1e-4, 1e-3, scaled=True)))
        diag = got["dadj"][:, idx, idx]
        assert torch.equal(diag, inp["dadj0"][:, idx, idx] if case.dadj == "acc" else torch.zeros(B, 64)), "d_adj diagonal"
        noedge = (inp["adj"] == 0)
        assert torch.equal(got["dadj"][noedge], (inp["dadj0"] if case.dadj == "acc" else torch.zeros(B, 64, 64))[noedge])
    print(f"gat {case.id}: largest error ratio {max(ratios):.4f}")
    # entries on the diagonal of adj change nothing at all
    if "diag" in case.graphs:
        a2 = inp["adj"].clone()
        a2[:, idx, idx] = 0.0
        again = run_gat(N, case, inp, adj=a2)
        for k in got:
            assert (got[k] is None and again[k] is None) or same(got[k], again[k]), f"{k} depends on the diagonal of adj"


def test_gat_layer_bad_arguments_launch_nothing(N):
    case = V.case_of(V.GAT_CASES, "C16-H1-B1-rand")
    inp = V.gat_inputs(case)
    xlr = rows_buf(torch.cat([inp["xl"].reshape(1, 64, 16), inp["xr"].reshape(1, 64, 16)], -1), 32)
    adj, we, att, bias = (inp[k].to(dev()) for k in ("adj", "we", "att", "bias"))
    out, alpha = full((64, 16)), full((1, 1, 64, 64))

    def bad():
        for C, ld, ldo, slope, act in ((12, 32, 16, 0.2, 0), (132, 32, 16, 0.2, 0), (18, 32, 16, 0.2, 0), (16, 12, 16, 0.2, 0),
                                       (16, 32, 12, 0.2, 0), (16, 32, 16, 1.5, 0), (16, 32, 16, 0.2, 2)):
            fails(N, V.ERR_BAD_ARG, "ctvae_gat_layer_forward", xlr.data_ptr(), xlr.data_ptr() + 64, ld, adj.data_ptr(), we.data_ptr(),
                  att.data_ptr(), bias.data_ptr(), None, out.data_ptr(), ldo, alpha.data_ptr(), 1, 1, C, slope, act)
    _, rep = logged(N, bad)
    assert rep == {}, sorted(rep)
    assert untouched(out.cpu()) and untouched(alpha.cpu())


# ---------------------------------------------------------------------------------------------------------------------
# regulariser
# ---------------------------------------------------------------------------------------------------------------------
def run_reg(native, case, inp, Nn=64, part=None):
    adj, graph, uni = (inp[k].contiguous().to(dev()) for k in ("adj", "graph", "uni"))
    part = full((case.B, 4)) if part is None else part
    native.call("ctvae_ct_reg_forward", adj.data_ptr(), graph.data_ptr(), uni.data_ptr(), part.data_ptr(), *case.coef, case.B, Nn)
    gl = torch.tensor([case.g_loss], dtype=torch.float32, device=dev())
    d_adj, d_graph = full((case.B, 64, 64)), full((case.B, 64, 64))
    native.call("ctvae_ct_reg_backward", adj.data_ptr(), graph.data_ptr(), uni.data_ptr(), part.data_ptr(), gl.data_ptr(), *case.coef,
                d_adj.data_ptr(), d_graph.data_ptr(), case.B, Nn)
    torch.cuda.synchronize()
    return dict(part4=part.cpu(), d_adj=d_adj.cpu(), d_graph=d_graph.cpu())


@pytest.mark.parametrize("case", V.REG_CASES, ids=lambda c: c.id)
def test_ct_reg(N, case):
    """Tolerances: those of tests/ct_checks.check_parts for the same three quantities (KL 1e-6 + 1e-4 |KL|, graph size 1e-4
    relative, positive trial 1e-3 relative; gradients 1e-3 of the largest magnitude, 2e-3 where the row products enter)."""
    inp = V.reg_inputs(case)
    ckl, cgs, cpt = (float(torch.tensor(c, dtype=torch.float32)) for c in case.coef)
    ref = V.reg_ref(inp["adj"], inp["graph"], inp["uni"], ckl, cgs, cpt, case.g_loss)
    got, rep = logged(N, lambda: twice(lambda: run_reg(N, case, inp)))
    assert set(rep) == {"ct_reg_fwd_kernel", "ct_reg_bwd_kernel"}, sorted(rep)
    p4, w4 = got["part4"].double(), ref["part4"]
    tol = torch.stack([1e-6 + 1e-4 * w4[:, 0].abs(), 1e-4 * w4[:, 1], 1e-3 * w4[:, 2],
                       abs(ckl) * (1e-6 + 1e-4 * w4[:, 0].abs()) + abs(cgs) * 1e-4 * w4[:, 1] + abs(cpt) * 1e-3 * w4[:, 2] + 1e-6], 1)
    within(f"reg {case.id}/part4", p4, w4, tol)
    for b, sp in enumerate(case.special):
        if sp == "allrows":
            assert float(p4[b, 2]) == 0.0
        if sp == "zerograph":
            assert float(p4[b, 1]) == 0.0 and float(got["d_graph"][b].abs().sum()) == 0.0
    within(f"reg {case.id}/d_adj", got["d_adj"], ref["d_adj"], torch.full_like(ref["d_adj"], 2e-3 * float(ref["d_adj"].abs().max())))
    within(f"reg {case.id}/d_graph", got["d_graph"], ref["d_graph"],
           torch.full_like(ref["d_graph"], 1e-3 * float(ref["d_graph"].abs().max())))
    assert torch.isfinite(got["d_adj"]).all() and torch.isfinite(got["d_graph"]).all()


def test_ct_reg_refuses_other_node_counts(N):
    case = V.REG_CASES[0]
    inp = V.reg_inputs(case)

    def bad():
        for Nn in (32, 63, 65, 128):
            part = full((case.B, 4))
            with pytest.raises(RuntimeError, match=rf"ctvae_ct_reg_forward failed.*\(code {V.ERR_BAD_ARG}\)"):
                run_reg(N, case, inp, Nn, part)
            assert untouched(part.cpu())
            a = full((1, 64, 64), 0.5)
            out = full((1, 64, 64))
            fails(N, V.ERR_BAD_ARG, "ctvae_ct_reg_backward", a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(),
                  0.1, 0.1, 0.1, out.data_ptr(), out.data_ptr(), 1, Nn)
            assert untouched(out.cpu())
    _, rep = logged(N, bad)
    assert rep == {}, sorted(rep)


# ---------------------------------------------------------------------------------------------------------------------
# blend + softmax, latent cross-entropy
# ---------------------------------------------------------------------------------------------------------------------
def run_bs(native, case, inp, want_dmask=True):
    y, g = inp["y"].contiguous().to(dev()), inp["g"].contiguous().to(dev())
    m = None if inp["mask"] is None else inp["mask"].to(dev())
    R, D, Hs = case.R, case.D, case.Hs
    probs = full((R + 3, D))                                               # three rows behind the last: must stay untouched
    native.call("ctvae_ct_blend_softmax_forward", y.data_ptr(), native.ptr(m), probs.data_ptr(), R, Hs, D)
    dy, dm = full((R + 3, Hs, D)), (full((R + 3,)) if (m is not None and want_dmask) else None)
    native.call("ctvae_ct_blend_softmax_backward", g.data_ptr(), probs.data_ptr(), y.data_ptr(), native.ptr(m), dy.data_ptr(),
                native.ptr(dm), R, Hs, D)
    torch.cuda.synchronize()
    return dict(probs=probs.cpu(), dy=dy.cpu(), dmask=None if dm is None else dm.cpu())


@pytest.mark.parametrize("case", V.BS_CASES, ids=lambda c: c.id)
def test_ct_blend_softmax(N, case):
    """Tolerances of the project's sigmoid / softmax outputs (test_ct_gpu.test_pair_mlp_kernel): probabilities 2e-6 / 1e-5, gradients
    1e-5 * max(1, |want|_inf) / 1e-4."""
    inp = V.bs_inputs(case)
    ref = V.blend_softmax_ref(inp["y"], inp["mask"], inp["g"])
    got, rep = logged(N, lambda: twice(lambda: run_bs(N, case, inp)))
    assert set(rep) == {"ct_blend_softmax_fwd_kernel", "ct_blend_softmax_bwd_kernel"}, sorted(rep)
    R = case.R
    assert untouched(got["probs"][R:]) and untouched(got["dy"][R:])
    within(f"blend_softmax {case.id}/probs", got["probs"][:R], ref["probs"], tol_of(ref["probs"], 2e-6, 1e-5))
    assert float((got["probs"][:R].double().sum(-1) - 1).abs().max()) <= 64 * V.EPS32
    within(f"blend_softmax {case.id}/dy", got["dy"][:R], ref["dy"], tol_of(ref["dy"], 1e-5, 1e-4, scaled=True))
    if case.Hs == 2:
        assert untouched(got["dmask"][R:])
        within(f"blend_softmax {case.id}/dmask", got["dmask"][:R], ref["dmask"], tol_of(ref["dmask"], 1e-5, 1e-4, scaled=True))
        no = run_bs(N, case, inp, want_dmask=False)                        # dmask = NULL: the rest is unchanged
        assert no["dmask"] is None and same(no["dy"], got["dy"]) and same(no["probs"], got["probs"])


def run_ce(native, case, inp):
    p, t = inp["probs"].contiguous().to(dev()), inp["target"].to(dev())
    R, D = case.R, case.D
    rows, dp = full((R + 3,)), full((R + 3, D))
    gl = torch.tensor([case.g_loss], dtype=torch.float32, device=dev())
    native.call("ctvae_ct_latent_ce_forward", p.data_ptr(), t.data_ptr(), rows.data_ptr(), R, D)
    native.call("ctvae_ct_latent_ce_backward", p.data_ptr(), t.data_ptr(), gl.data_ptr(), dp.data_ptr(), R, D)
    torch.cuda.synchronize()
    return dict(row_loss=rows.cpu(), d_probs=dp.cpu())


@pytest.mark.parametrize("case", V.CE_CASES, ids=lambda c: c.id)
def test_ct_latent_ce(N, case):
    """Tolerances: tests/ct_checks (latent_loss 1e-4 absolute, here per row; gradient 1e-4 * max(1, |want|_inf) / 1e-3)."""
    inp = V.ce_inputs(case)
    ref = V.latent_ce_ref(inp["probs"], inp["target"], case.g_loss)
    got, rep = logged(N, lambda: twice(lambda: run_ce(N, case, inp)))
    assert set(rep) == {"ct_latent_ce_fwd_kernel", "ct_latent_ce_bwd_kernel"}, sorted(rep)
    R = case.R
    assert untouched(got["row_loss"][R:]) and untouched(got["d_probs"][R:])
    within(f"latent_ce {case.id}/row_loss", got["row_loss"][:R], ref["row_loss"], torch.full_like(ref["row_loss"], 1e-4))
    within(f"latent_ce {case.id}/d_probs", got["d_probs"][:R], ref["d_probs"], tol_of(ref["d_probs"], 1e-4, 1e-3, scaled=True))
    below = inp["probs"] <= V.BOUND
    assert float(got["d_probs"][:R][below].abs().sum()) == 0.0, "no gradient at or below the clamp bound"


def test_blend_softmax_and_ce_refuse_wide_rows(N):
    buf, out = full((8, 2, 65), 0.5), full((8, 2, 65))
    t = torch.zeros(8, dtype=torch.int64, device=dev())

    def bad():
        for D in (65, 0):
            fails(N, V.ERR_BAD_ARG, "ctvae_ct_blend_softmax_forward", buf.data_ptr(), buf.data_ptr(), out.data_ptr(), 8, 2, D)
            fails(N, V.ERR_BAD_ARG, "ctvae_ct_blend_softmax_backward", buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), buf.data_ptr(),
                  out.data_ptr(), out.data_ptr(), 8, 2, D)
            fails(N, V.ERR_BAD_ARG, "ctvae_ct_latent_ce_forward", buf.data_ptr(), t.data_ptr(), out.data_ptr(), 8, D)
            fails(N, V.ERR_BAD_ARG, "ctvae_ct_latent_ce_backward", buf.data_ptr(), t.data_ptr(), buf.data_ptr(), out.data_ptr(), 8, D)
        fails(N, V.ERR_BAD_ARG, "ctvae_ct_blend_softmax_forward", buf.data_ptr(), None, out.data_ptr(), 8, 2, 20)     # Hs = 2 needs a mask
        fails(N, V.ERR_BAD_ARG, "ctvae_ct_blend_softmax_forward", buf.data_ptr(), buf.data_ptr(), out.data_ptr(), 8, 3, 20)
    _, rep = logged(N, bad)
    assert rep == {}, sorted(rep)
    assert untouched(out.cpu())


# ---------------------------------------------------------------------------------------------------------------------
# intervention mask, straight-through sample
# ---------------------------------------------------------------------------------------------------------------------
def run_mask(native, case, inp):
    B, A = case.B, case.A
    t = {k: (None if inp[k] is None else inp[k].contiguous().to(dev())) for k in ("x", "action", "pe", "keep", "W", "bias", "expo", "g")}
    inter, p, sample, soft = full((B, 64, 64)), full((B, 64)), full((B, 64)), full((B, 64))
    native.call("ctvae_ct_mask_forward", t["x"].data_ptr(), t["action"].data_ptr(), t["pe"].data_ptr(), native.ptr(t["keep"]), inp["scale"],
                t["W"].data_ptr(), t["bias"].data_ptr(), t["expo"].data_ptr(), B, 64, 64, A, inter.data_ptr(), p.data_ptr(),
                sample.data_ptr(), soft.data_ptr())
    dWp, dbp = full((B, A + 64, 64)), full((B, 64))
    native.call("ctvae_ct_mask_backward", t["x"].data_ptr(), t["action"].data_ptr(), t["pe"].data_ptr(), native.ptr(t["keep"]), inp["scale"],
                inter.data_ptr(), p.data_ptr(), soft.data_ptr(), t["g"].data_ptr(), B, 64, 64, A, dWp.data_ptr(), dbp.data_ptr())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in dict(inter=inter, p=p, sample=sample, soft=soft, dWp=dWp, dbp=dbp).items()}


@pytest.mark.parametrize("case", V.MASK_CASES, ids=lambda c: c.id)
def test_ct_mask(N, case):
    """inter, p, soft: the derived float32 bounds of ct_ops_checks.mask_error_bounds; sample: EQUAL to the reference's decision
    wherever |a1 - a0| exceeds the bound of its float32 evaluation (at most 0.5 % of the samples lie inside, asserted on the host);
    dWp / dbp: tests/ct_checks' gradient tolerance 1e-4 * max(1, |want|_inf) / 1e-3."""
    inp = V.mask_inputs(case)
    ref = V.mask_ref(**{k: inp[k] for k in ("x", "action", "pe", "keep", "scale", "W", "bias", "expo", "g")})
    d_inter, d_p, d_a = V.mask_error_bounds(case, inp, ref)
    got, rep = logged(N, lambda: twice(lambda: run_mask(N, case, inp)))
    assert set(rep) == {"ct_mask_fwd_kernel", "ct_mask_bwd_kernel"}, sorted(rep)
    within(f"mask {case.id}/inter", got["inter"], ref["inter"], d_inter)
    within(f"mask {case.id}/p", got["p"], ref["p"], d_p)
    within(f"mask {case.id}/soft", got["soft"], ref["soft"], 0.25 * d_a + 4 * V.EPS32)
    sure = (ref["a1"] - ref["a0"]).abs() > d_a
    assert float((~sure).double().mean()) <= V.EXCLUDE_CAP
    s = got["sample"].double()
    assert bool(((s == 0) | (s == 1)).all()), "sample must be exactly 0 or 1"
    assert torch.equal(s[sure], ref["sample"][sure]), f"{int((s[sure] != ref['sample'][sure]).sum())} decisions differ outside the margin"
    within(f"mask {case.id}/dWp", got["dWp"], ref["dWp"], tol_of(ref["dWp"], 1e-4, 1e-3, scaled=True))
    within(f"mask {case.id}/dbp", got["dbp"], ref["dbp"], tol_of(ref["dbp"], 1e-4, 1e-3, scaled=True))


def run_sample(native, inp, n, weighted, gs, gw):
    p, expo = inp["p"].to(dev()), inp["expo"].contiguous().to(dev())
    out, soft, w = full((n + 5,)), full((n + 5,)), (full((n + 5,)) if weighted else None)
    native.call("ctvae_ct_sample_forward", p.data_ptr(), expo.data_ptr(), out.data_ptr(), soft.data_ptr(), native.ptr(w), n)
    g_s = inp["g_s"].to(dev()) if gs else None
    g_w = inp["g_w"].to(dev()) if gw else None
    gp = full((n + 5,))
    native.call("ctvae_ct_sample_backward", native.ptr(g_s), native.ptr(g_w), p.data_ptr(), soft.data_ptr(), out.data_ptr(), gp.data_ptr(), n)
    torch.cuda.synchronize()
    return dict(sample=out.cpu(), soft=soft.cpu(), weighted=None if w is None else w.cpu(), g_p=gp.cpu())


@pytest.mark.parametrize("gs,gw,weighted", [(True, False, False), (False, True, True), (True, True, True)], ids=["g_sample", "g_weighted", "both"])
@pytest.mark.parametrize("n", V.SAMPLE_N)
def test_ct_sample(N, n, gs, gw, weighted):
    """soft: 0.25 * (bound of a1 - a0) + the sigmoid's own few ulp; sample / weighted exact outside the margin; g_p: the
    tolerance of test_ct_gpu.test_gumbel_st_kernel for the same estimator (1e-4 / 1e-3), scaled by max(1, |want|_inf)."""
    inp = V.sample_inputs(n)
    ref = V.sample_ref(inp["p"], inp["expo"], inp["g_s"] if gs else None, inp["g_w"] if gw else None)
    margin = V.sample_margin(inp["p"], inp["expo"])
    got, rep = logged(N, lambda: twice(lambda: run_sample(N, inp, n, weighted, gs, gw)))
    assert set(rep) == {"ct_sample_fwd_kernel", "ct_sample_bwd_kernel"}, sorted(rep)
    for k in ("sample", "soft", "g_p") + (("weighted",) if weighted else ()):
        assert untouched(got[k][n:]), f"{k}: written behind the {n} elements"
    assert (got["weighted"] is None) == (not weighted)
    within(f"sample n{n}/soft", got["soft"][:n], ref["soft"], 0.25 * margin + 4 * V.EPS32)
    sure = (ref["a1"] - ref["a0"]).abs() > margin
    assert int((~sure).sum()) <= V.EXCLUDE_CAP * n
    s = got["sample"][:n].double()
    assert bool(((s == 0) | (s == 1)).all()) and torch.equal(s[sure], ref["sample"][sure])
    if weighted:
        assert torch.equal(got["weighted"][:n][sure], (inp["p"] * ref["sample"].float())[sure])
    # the gradient is continuous in soft but takes the kernel's own hard sample: compare where the decision is sure
    within(f"sample n{n}/g_p", got["g_p"][:n][sure], ref["g_p"][sure], tol_of(ref["g_p"], 1e-4, 1e-3, scaled=True)[sure])


# ---------------------------------------------------------------------------------------------------------------------
# small related ops
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 257])
def test_ct_blend(N, rows):
    """Two multiplies and an add per element (no fused multiply-add is promised either way): 3 ulp of the magnitudes involved;
    g_mask sums 64 products: the dot-product bound."""
    g = V.gen_of(f"blend{rows}")
    s0, s1, gr = (torch.rand(rows, 64, generator=g) for _ in range(3))
    m = torch.rand(rows, generator=g)
    m[::3] = 0.0
    m[1::3] = 1.0

    def run():
        d_ = [t.to(dev()) for t in (s0, s1, m, gr)]
        out, g0, g1, gm = full((rows + 2, 64)), full((rows + 2, 64)), full((rows + 2, 64)), full((rows + 2,))
        N.call("ctvae_ct_blend_forward", d_[0].data_ptr(), d_[1].data_ptr(), d_[2].data_ptr(), out.data_ptr(), rows)
        N.call("ctvae_ct_blend_backward", d_[3].data_ptr(), d_[0].data_ptr(), d_[1].data_ptr(), d_[2].data_ptr(), g0.data_ptr(), g1.data_ptr(),
               gm.data_ptr(), rows)
        torch.cuda.synchronize()
        return dict(out=out.cpu(), g0=g0.cpu(), g1=g1.cpu(), gm=gm.cpu())
    got = twice(run)
    for k in got:
        assert untouched(got[k][rows:])
    S0, S1, M, G = V.d(s0), V.d(s1), V.d(m)[:, None], V.d(gr)
    within("blend/out", got["out"][:rows], S0 * (1 - M) + S1 * M, 3 * V.EPS32 * (S0 * (1 - M) + S1 * M))
    assert torch.equal(got["g0"][:rows], gr * (1 - m[:, None])) and torch.equal(got["g1"][:rows], gr * m[:, None])
    within("blend/g_mask", got["gm"][:rows], (G * (S1 - S0)).sum(-1), V.dot_bound(64 + 1, (G * (S1 - S0)).abs().sum(-1)))
    assert torch.equal(got["out"][:rows][0::3], s0[0::3]) and torch.equal(got["out"][:rows][1::3], s1[1::3])


@pytest.mark.parametrize("n", [4, 12])
def test_ct_posenc(N, n):
    sd = 4
    g = V.gen_of(f"posenc{n}")
    x, pe, gr = torch.randn(n, generator=g), torch.randn(sd, generator=g), torch.randn(n, generator=g)
    keep = (torch.rand(n, generator=g) < 0.7).float()
    scale = float(torch.tensor(1 / 0.9, dtype=torch.float32))
    for kp in (None, keep):
        def run():
            d_ = [None if t is None else t.to(dev()) for t in (x, pe, kp, gr)]
            out, gx = full((n + 4,)), full((n + 4,))
            N.call("ctvae_ct_posenc_forward", d_[0].data_ptr(), d_[1].data_ptr(), N.ptr(d_[2]), scale, out.data_ptr(), n, sd)
            if kp is not None:
                N.call("ctvae_ct_posenc_backward", d_[3].data_ptr(), d_[2].data_ptr(), scale, gx.data_ptr(), n)
            torch.cuda.synchronize()
            return dict(out=out.cpu(), gx=gx.cpu())
        got = twice(run)
        assert untouched(got["out"][n:]) and untouched(got["gx"][n if kp is not None else 0:])
        want = V.d(x) + V.d(pe).repeat(n // sd)
        if kp is None:
            assert torch.equal(got["out"][:n], x + pe.repeat(n // sd))                  # one add: correctly rounded
        else:
            within("posenc/out", got["out"][:n], want * V.d(kp) * scale, 3 * V.EPS32 * (want * scale).abs())
            within("posenc/gx", got["gx"][:n], V.d(gr) * V.d(kp) * scale, 2 * V.EPS32 * (V.d(gr) * scale).abs())
            assert float(got["out"][:n][kp == 0].abs().sum()) == 0.0


def test_one_hot_first_and_last_index(N):
    for inds in ([0], [3], [0, 3, 1, 2, 3]):
        t = torch.tensor(inds, dtype=torch.int64, device=dev())
        out = full((len(inds) + 1, 4))
        N.call("ctvae_one_hot", t.data_ptr(), len(inds), 4, out.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(out[:len(inds)].cpu(), torch.nn.functional.one_hot(torch.tensor(inds), 4).float()) and untouched(out[len(inds):].cpu())
    fails(N, V.ERR_BAD_ARG, "ctvae_one_hot", t.data_ptr(), 1, 6, out.data_ptr())


def run_pair(native, case, inp):
    B, Nn, H = case.B, case.N, case.H
    ld, ldd = 2 * H + case.pad, 2 * H + case.pad + 4
    uv = rows_buf(torch.cat([inp["u"], inp["v"]], -1), ld)
    w2, b2, g = inp["w2"].contiguous().to(dev()), inp["b2"].to(dev()), inp["g"].contiguous().to(dev())
    ro = None if inp["row_of"] is None else inp["row_of"].to(dev())
    per = 0 if ro is None else 1
    out = full((B, Nn, Nn))
    native.call("ctvae_pair_mlp_forward", uv.data_ptr(), uv.data_ptr() + 4 * H, ld, w2.data_ptr(), b2.data_ptr(), out.data_ptr(), B, Nn, H,
                V.SLOPE_PAIR, per, native.ptr(ro))
    d_uv, dw2p, db2p = full((B * Nn, ldd)), full((B, H)), full((B,))
    native.call("ctvae_pair_mlp_backward", uv.data_ptr(), uv.data_ptr() + 4 * H, ld, w2.data_ptr(), out.data_ptr(), g.data_ptr(),
                d_uv.data_ptr(), d_uv.data_ptr() + 4 * H, ldd, dw2p.data_ptr(), db2p.data_ptr(), B, Nn, H, V.SLOPE_PAIR, per, native.ptr(ro))
    torch.cuda.synchronize()
    return dict(out=out.cpu(), d_uv=d_uv.cpu(), dw2p=dw2p.cpu(), db2p=db2p.cpu())


@pytest.mark.parametrize("case", V.PAIR_CASES, ids=lambda c: c.id)
def test_pair_mlp_strided_blocks_and_bank_rows(N, case):
    """Tolerances of test_ct_gpu.test_pair_mlp_kernel: output 2e-6 / 1e-5, gradients 1e-5 * max(1, |want|_inf) / 1e-4.  The
    leaky-ReLU sign needs no margin here: a float32 add has the sign of the exact sum (the host test asserts no sum is 0)."""
    inp = V.pair_inputs(case)
    ref = V.pair_mlp_ref(inp["u"], inp["v"], inp["w2"], inp["b2"], inp["row_of"], V.SLOPE_PAIR, inp["g"])
    got, rep = logged(N, lambda: twice(lambda: run_pair(N, case, inp)))
    assert set(rep) == {"pair_mlp_fwd_kernel", "pair_mlp_bwd_kernel"}, sorted(rep)
    B, Nn, H = case.B, case.N, case.H
    within(f"pair {case.id}/out", got["out"], ref["out"], tol_of(ref["out"], 2e-6, 1e-5))
    assert untouched(got["d_uv"][:, 2 * H:]), "ldd padding written"
    for name, g_, want in (("d_u", got["d_uv"][:, :H].reshape(B, Nn, H), ref["d_u"]), ("d_v", got["d_uv"][:, H:2 * H].reshape(B, Nn, H), ref["d_v"]),
                           ("d_w2", got["dw2p"], ref["d_w2"]), ("d_b2", got["db2p"], ref["d_b2"])):
        within(f"pair {case.id}/{name}", g_, want, tol_of(want, 1e-5, 1e-4, scaled=True))


# ---------------------------------------------------------------------------------------------------------------------
# pair scorer: the three 64-node kernels and every way into them
# ---------------------------------------------------------------------------------------------------------------------
def off_buf(n, off, fill=NAN):
    """n floats that start `off` floats behind a 16-byte boundary, NaN around them."""
    base = full((off + n + 4,), fill)
    assert base.data_ptr() % 16 == 0
    return base[off:off + n]


_pair_refs = {}


def pair64_ref(case):
    """(inputs, float64 reference) of a case, computed once.  The backward is tested alone: G is formed from the reference's out
    rounded to float32, which is what the kernel is handed."""
    if case.id not in _pair_refs:
        inp = V.pair_inputs(case)
        _pair_refs[case.id] = (inp, V.pair_terms(inp["u"], inp["v"], inp["w2"], inp["b2"] if case.bias else None, inp["row_of"],
                                                 V.SLOPE_PAIR32, inp["g"], out32=True))
    return _pair_refs[case.id]


class PairBufs:
    """Device inputs of one Pair64Case in the layout the case asks for; forward() / backward() run one entry point into fresh
    NaN-filled outputs with a guard row behind each.  k: u, v times 2^k and w2 times 2^-k."""

    def __init__(self, case, inp, ref_out, k=0):
        self.case = case
        B, Nn, H = case.B, case.N, case.H
        ld, c0 = case.ld_, case.ucol
        s = 2.0 ** k
        self.uv = off_buf(B * Nn * ld, case.uvoff).view(B * Nn, ld)
        self.uv[:, c0:c0 + H] = (inp["u"] * s).reshape(-1, H).to(dev())
        self.uv[:, c0 + H:c0 + 2 * H] = (inp["v"] * s).reshape(-1, H).to(dev())
        self.u_ptr, self.v_ptr = self.uv.data_ptr() + 4 * c0, self.uv.data_ptr() + 4 * (c0 + H)
        self.w2 = off_buf(case.G * H, case.w2off)
        self.w2[:] = (inp["w2"] / s).reshape(-1).to(dev())
        self.b2 = inp["b2"].to(dev()) if case.bias else None
        self.ro = None if inp["row_of"] is None else inp["row_of"].to(dev())
        self.per = 0 if self.ro is None else 1
        self.out_in = ref_out.float().contiguous().to(dev())
        self.g = inp["g"].contiguous().to(dev())

    def new_out(self):
        c = self.case
        return off_buf((c.B * c.N + 1) * c.N, c.outoff).view(c.B * c.N + 1, c.N)

    def aligned(self, out):
        return tuple(p % 16 == 0 for p in (self.u_ptr, self.v_ptr, out.data_ptr(), self.w2.data_ptr()))

    def fwd_args(self, native, out):
        c = self.case
        return [self.u_ptr, self.v_ptr, c.ld_, self.w2.data_ptr(), native.ptr(self.b2), out.data_ptr(), c.B, c.N, c.H, V.SLOPE_PAIR32,
                self.per, native.ptr(self.ro)]

    def new_grads(self):
        c = self.case
        return full((c.B * c.N + 1, c.ldd_)), full((c.B + 1, c.H)), full((c.B + 1,))

    def bwd_args(self, native, d_uv, dw2p, db2p):
        c = self.case
        return [self.u_ptr, self.v_ptr, c.ld_, self.w2.data_ptr(), self.out_in.data_ptr(), self.g.data_ptr(),
                d_uv.data_ptr() + 4 * c.ucol, d_uv.data_ptr() + 4 * (c.ucol + c.H), c.ldd_, dw2p.data_ptr(), db2p.data_ptr(), c.B, c.N,
                c.H, V.SLOPE_PAIR32, self.per, native.ptr(self.ro)]

    def forward(self, native):
        out = self.new_out()
        native.call("ctvae_pair_mlp_forward", *self.fwd_args(native, out))
        torch.cuda.synchronize()
        return dict(out=out.cpu())

    def backward(self, native):
        d_uv, dw2p, db2p = self.new_grads()
        native.call("ctvae_pair_mlp_backward", *self.bwd_args(native, d_uv, dw2p, db2p))
        torch.cuda.synchronize()
        return dict(d_uv=d_uv.cpu(), dw2p=dw2p.cpu(), db2p=db2p.cpu())


def pair_grad_views(case, got):
    """The written parts of the backward's buffers; asserts that everything else still holds the fill."""
    B, Nn, H, c0 = case.B, case.N, case.H, case.ucol
    d_uv = got["d_uv"]
    assert untouched(d_uv[:, :c0]) and untouched(d_uv[:, c0 + 2 * H:]), "columns beside d_u | d_v written"
    assert untouched(d_uv[B * Nn:]) and untouched(got["dw2p"][B:]) and untouched(got["db2p"][B:]), "guard row written"
    return dict(d_u=d_uv[:B * Nn, c0:c0 + H].reshape(B, Nn, H), d_v=d_uv[:B * Nn, c0 + H:c0 + 2 * H].reshape(B, Nn, H),
                d_w2=got["dw2p"][:B], d_b2=got["db2p"][:B])


@pytest.mark.parametrize("case", V.PAIR64_CASES, ids=lambda c: c.id)
def test_pair64_each_kernel_alone(N, case):
    """Forward and backward separately (the backward on the float32-rounded reference out) against the float64 reference, within
    dot_bound(L, |.| sum) with L of ct_ops_checks.pair_chain; the launch log must name the kernels the mirror of the launcher
    predicts from the actual pointers, which must be the ones the case table is there to reach."""
    inp, ref = pair64_ref(case)
    P = PairBufs(case, inp, ref["out"])
    B, Nn, H = case.B, case.N, case.H
    fk, bk = V.pair_kernels(Nn, H, case.ld_, *P.aligned(P.new_out()))
    assert (fk, bk) == (case.fwd, case.bwd)
    got, rep = logged(N, lambda: twice(lambda: P.forward(N)))
    assert set(rep) == {fk} and rep[fk]["count"] == 2, sorted(rep)
    assert untouched(got["out"][B * Nn:]), "guard row of out written"
    L = V.pair_chain(fk, Nn, H)["out"]
    within(f"pair64 {case.id}/out [{fk}, L={L}]", got["out"][:B * Nn].reshape(B, Nn, Nn), ref["out"], V.pair_out_tol(L, V.pair_abs(ref, "out", fk)))
    if bk is None:                       # N > 64: refused, nothing launched, nothing written
        bufs = P.new_grads()
        _, rep = logged(N, lambda: fails(N, V.ERR_BAD_ARG, "ctvae_pair_mlp_backward", *P.bwd_args(N, *bufs)))
        assert not rep and all(untouched(t.cpu()) for t in bufs)
        return
    got, rep = logged(N, lambda: twice(lambda: P.backward(N)))
    assert set(rep) == {bk} and rep[bk]["count"] == 2, sorted(rep)
    Ls = V.pair_chain(bk, Nn, H)
    for name, g_ in pair_grad_views(case, got).items():
        within(f"pair64 {case.id}/{name} [{bk}, L={Ls[name]}]", g_, ref[name], V.dot_bound(Ls[name], V.pair_abs(ref, name, bk)))


@pytest.mark.parametrize("cid", V.PAIR_SCALE_CASES)
def test_pair64_power_of_two_scaling_commutes(N, cid):
    """(2^k u, 2^k v, 2^-k w2) gives the same out bit for bit on each forward kernel, and, for the same out and g, d_u and d_v times
    2^-k, d_w2 times 2^k and the same d_b2 bit for bit: power-of-two scaling commutes with every operation of these kernels while
    nothing leaves the normal range (asserted for these inputs in the host test), the clamps that stand for relu and the step
    function included."""
    case = V.case_of(V.PAIR64_CASES, cid)
    inp, ref = pair64_ref(case)
    base = PairBufs(case, inp, ref["out"])
    (f0, b0), rep = logged(N, lambda: (base.forward(N), base.backward(N)))
    assert set(rep) == {case.fwd, case.bwd}, sorted(rep)
    g0 = pair_grad_views(case, b0)
    for k in V.PAIR_SCALE_K:
        P = PairBufs(case, inp, ref["out"], k=k)
        (f, b), rep = logged(N, lambda: (P.forward(N), P.backward(N)))
        assert set(rep) == {case.fwd, case.bwd}, sorted(rep)
        assert same(f["out"], f0["out"]), f"k={k}: out differs"
        g = pair_grad_views(case, b)
        s = 2.0 ** k
        assert same(g["d_u"], g0["d_u"] / s) and same(g["d_v"], g0["d_v"] / s), f"k={k}: d_u / d_v are not the 2^-k multiples"
        assert same(g["d_w2"], g0["d_w2"] * s), f"k={k}: d_w2 is not the 2^k multiple"
        assert same(g["d_b2"], g0["d_b2"]), f"k={k}: d_b2 differs"


def test_pair64_refusals_write_nothing(N):
    case = V.case_of(V.PAIR64_CASES, "H36")
    inp, ref = pair64_ref(case)
    P = PairBufs(case, inp, ref["out"])
    out, grads = P.new_out(), P.new_grads()
    fa, ba = P.fwd_args(N, out), P.bwd_args(N, *grads)

    def bad(args, **at):
        a = list(args)
        for i, v in at.items():
            a[int(i[1:])] = v
        return a

    def run():
        # forward: u, v, ld, w2, b2, out, B, N, H, ...
        for at in (dict(_2=case.H - 1), dict(_6=0), dict(_6=-1), dict(_7=0), dict(_7=-64), dict(_8=0), dict(_8=-4), dict(_0=None), dict(_1=None),
                   dict(_3=None), dict(_5=None)):
            fails(N, V.ERR_BAD_ARG, "ctvae_pair_mlp_forward", *bad(fa, **at))
        # backward: u, v, ld, w2, out, g_out, d_u, d_v, ldd, d_w2_part, d_b2_part, B, N, H, ...
        for at in (dict(_2=case.H - 1), dict(_8=case.H - 1), dict(_11=0), dict(_11=-1), dict(_12=0), dict(_12=-64), dict(_12=65), dict(_13=0),
                   dict(_13=-4), *[{f"_{i}": None} for i in (0, 1, 3, 4, 5, 6, 7, 9, 10)]):
            fails(N, V.ERR_BAD_ARG, "ctvae_pair_mlp_backward", *bad(ba, **at))

    _, rep = logged(N, run)
    assert not rep, sorted(rep)
    assert untouched(out.cpu()) and all(untouched(t.cpu()) for t in grads)


@pytest.mark.parametrize("nd", [1, 2])
def test_pair_scores_wrapper_folds_partials_into_bank_rows(N, nd):
    """kernels.PairScores as the model calls it, on plain tensors (no flat gradient buffer): column blocks of one GEMM output, the
    scorer bank read in place through grp, per-sample partials folded into the bank's rows by ctvae_group_rowsum.  Reference:
    float64 autograd of the written-out pre-activation; the sigmoid's derivative is taken at the out the forward saved (as the
    wrapper's backward does), so that the gradients' bounds need no term for the forward's own error."""
    from ctvae_amd import kernels as K
    B, H, G = 3, 48, 5
    gen = V.gen_of(f"pair-scores-nd{nd}", 17)
    uv = torch.randn(B, 64, nd * 2 * H, generator=gen)
    w2, b2 = torch.randn(G, H, generator=gen) / H ** 0.5, torch.randn(G, generator=gen)
    g = torch.randn(nd, B, 64, 64, generator=gen)
    grp = torch.tensor(V.ROWS["row_of"], dtype=torch.int32) if nd == 2 else None
    rows = [torch.zeros(B, dtype=torch.long)] + ([grp.long()] if nd == 2 else [])

    def run():
        a, w, b = (t.to(dev()).requires_grad_(True) for t in (uv, w2, b2))
        out = K.PairScores.apply(a, w, b, None if grp is None else grp.to(dev()), H)
        ga, gw, gb = torch.autograd.grad(out, (a, w, b), g.to(dev()))
        torch.cuda.synchronize()
        assert all(t.data_ptr() % 16 == 0 for t in (a, w, out))
        return dict(out=out.detach().cpu(), d_uv=ga.cpu(), d_w2=gw.cpu(), d_b2=gb.cpu())

    got, rep = logged(N, lambda: twice(run))
    assert set(rep) == {V.FWD64B, V.BWD64, "group_rowsum_kernel"}, sorted(rep)
    assert rep[V.FWD64B]["count"] == 2 * nd and rep[V.BWD64]["count"] == 2 * nd
    # float64: the same expression; per discoverer d the analytic terms give the |.| sums
    uv64, w64, b64 = (V.d(t).requires_grad_(True) for t in (uv, w2, b2))
    pre = []
    for dd in range(nd):
        u, v = uv64[..., 2 * dd * H:(2 * dd + 1) * H], uv64[..., (2 * dd + 1) * H:(2 * dd + 2) * H]
        t = u[:, :, None, :] + v[:, None, :, :]
        pre.append((torch.nn.functional.leaky_relu(t, V.SLOPE_PAIR32) * w64[rows[dd]][:, None, None, :]).sum(-1) + b64[rows[dd]][:, None, None])
    pre = torch.stack(pre)
    s = got["out"].double()
    (pre * (V.d(g) * s * (1 - s))).sum().backward()
    Lf, Lb = V.pair_chain(V.FWD64B, 64, H)["out"], V.pair_chain(V.BWD64, 64, H)
    w_abs, b_abs, cnt = torch.zeros(G, H, dtype=torch.float64), torch.zeros(G, dtype=torch.float64), torch.zeros(G)
    for dd in range(nd):
        cu, cv = slice(2 * dd * H, (2 * dd + 1) * H), slice((2 * dd + 1) * H, (2 * dd + 2) * H)
        terms = V.pair_terms(uv[..., cu], uv[..., cv], w2, b2, None if dd == 0 else grp, V.SLOPE_PAIR32)
        within(f"PairScores nd={nd}/out[{dd}]", got["out"][dd], torch.sigmoid(pre[dd].detach()), V.pair_out_tol(Lf, terms["out_abs_split"]))
        # the |.| sums with G from the saved out
        Ga = (V.d(g[dd]) * s[dd] * (1 - s[dd])).abs()
        wa = V.d(w2)[rows[dd]].abs()
        within(f"PairScores nd={nd}/d_u[{dd}]", got["d_uv"][..., cu], uv64.grad[..., cu], V.dot_bound(Lb["d_u"], wa[:, None, :] * Ga.sum(2)[:, :, None]))
        within(f"PairScores nd={nd}/d_v[{dd}]", got["d_uv"][..., cv], uv64.grad[..., cv], V.dot_bound(Lb["d_v"], wa[:, None, :] * Ga.sum(1)[:, :, None]))
        tt = V.d(uv[..., cu])[:, :, None, :] + V.d(uv[..., cv])[:, None, :, :]
        mag = V.d(uv[..., cu]).abs()[:, :, None, :] + V.d(uv[..., cv]).abs()[:, None, :, :]
        dl = torch.where(tt > 0, torch.ones_like(tt), torch.full_like(tt, V.SLOPE_PAIR32))
        w_abs.index_add_(0, rows[dd], torch.einsum("bij,bijh->bh", Ga, dl * mag))
        b_abs.index_add_(0, rows[dd], Ga.sum((1, 2)))
        cnt.index_add_(0, rows[dd], torch.ones(B))
    # ctvae_group_rowsum: at most B adds per call and one more to accumulate the second call
    Lw, Lbias = Lb["d_w2"] + B + 1, Lb["d_b2"] + B + 1
    within(f"PairScores nd={nd}/d_w2", got["d_w2"], w64.grad, V.dot_bound(Lw, w_abs))
    within(f"PairScores nd={nd}/d_b2", got["d_b2"], b64.grad, V.dot_bound(Lbias, b_abs))
    unused = cnt == 0
    assert unused.tolist() == ([False, True, False, True, False] if nd == 2 else [False, True, True, True, True]) and int(cnt[0]) == B
    assert float(got["d_w2"][unused].abs().sum()) == 0.0 and float(got["d_b2"][unused].abs().sum()) == 0.0, "rows nobody uses must be 0"
    assert float(w64.grad[unused].abs().sum()) == 0.0
