"""CPU: the float64 references, input regimes, bounds and the dispatch mirror of tests/wgrad_checks.py, before
tests/test_wgrad_ops_gpu.py relies on them.

  * the reference (an im2col GEMM over the ported tap tables) equals torch's float64 autograd weight / bias gradient after the
    layout change for every case geometry; InXform / DyXform equal the same chain written with plain torch ops;
  * every `int` case keeps every partial sum below 2^24;
  * every case's mirror output has the property the case is named for (kernel label, S, reduction shape, tile counts
    against the persistent grids' caps);
  * a float32 emulation of a chunked summation -- pixel by pixel, chunk by chunk, and as a balanced tree -- stays inside every
    `randn` bound, on every element;
  * the ported geometry gives what csrc/geom.hpp gives (tests/host_emul: the naive-loop weight gradient over build_geom)."""
import ctypes
import dataclasses
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_checks as V

_REF = {}


def ref_of(case, regime):
    key = (case.id, regime)
    if key not in _REF:
        _REF[key] = V.reference(case, regime)
    return _REF[key]


HOST_MAX_MC = 40000          # the 520 / 776-tile cases are the one-tile cases' geometry: their references are evaluated in the GPU suite only


def small(case):
    return case.geom().Mc <= HOST_MAX_MC


def torch_grads(case, x, d):
    """torch float64 autograd of the layer: (dW in the library layout, dbias); x, d NHWC float64."""
    base, flat = case.kind & ~V.W_CI_TAP, bool(case.kind & V.W_CI_TAP)
    xn = x.permute(0, 3, 1, 2).contiguous()
    if flat:
        w = torch.zeros(case.Co, case.Ci * case.k * case.k, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(case.Co, dtype=torch.float64, requires_grad=True)
        assert case.H == case.k and case.W == case.k
        y = F.linear(torch.flatten(xn, start_dim=1), w, b)
        y.backward(d.reshape(y.shape))
        return w.grad.t().reshape(case.Ci, case.k * case.k, case.Co), b.grad      # [in][out], in = ci*k*k + tap
    tr = base == V.CONVT
    w = torch.zeros((case.Ci, case.Co, case.k, case.k) if tr else (case.Co, case.Ci, case.k, case.k), dtype=torch.float64,
                    requires_grad=True)
    b = torch.zeros(case.Co, dtype=torch.float64, requires_grad=True)
    if tr:
        y = F.conv_transpose2d(xn, w, b, stride=case.s, padding=case.p, output_padding=case.op)
        pack = lambda t: t.permute(2, 3, 0, 1)
    else:
        y = F.conv2d(xn, w, b, stride=case.s, padding=case.p)
        pack = lambda t: t.permute(2, 3, 1, 0)
    y.backward(d.permute(0, 3, 1, 2).contiguous())
    return pack(w.grad).reshape(case.k * case.k, case.Ci, case.Co), b.grad


def torch_xforms(case, regime):
    """x' and g through plain torch ops in float64 (leaky_relu / its autograd), not through wgrad_checks' formulas."""
    x, dy, xf, dyx = V.make_inputs(case, regime)
    x64, d64 = x.double(), dy.double()
    if xf is not None:
        sc, sh, act = xf
        t = x64 * sc.double() + sh.double()
        x64 = {V.ACT_NONE: t, V.ACT_LRELU: F.leaky_relu(t, 0.01), V.ACT_RELU: F.relu(t)}[act]
    if dyx is not None:
        y, coef, act = dyx
        c = coef.double()
        t = (y.double() * c[3] + c[4]).requires_grad_(True)
        a = {V.ACT_NONE: t * 1.0, V.ACT_LRELU: F.leaky_relu(t, 0.01), V.ACT_RELU: F.relu(t)}[act]
        a.backward(d64)                                           # t.grad = g_a * act'(t)
        d64 = c[0] * t.grad + c[1] * y.double() + c[2]
    return x64, d64


HOST_CASES = [c for c in V.ALL_CASES if c.rc == 0]


@pytest.mark.parametrize("case", [c for c in HOST_CASES if small(c)], ids=lambda c: c.id)
def test_reference_matches_torch_float64_autograd(case):
    for regime in ("int", "randn"):
        ref = ref_of(case, regime)
        x64, d64 = torch_xforms(case, regime)
        dw, db = torch_grads(case, x64, d64)
        scale = max(1.0, float(dw.abs().max()))
        assert ref["dw"].shape == dw.shape
        assert float((ref["dw"] - dw).abs().max()) <= 1e-12 * scale, case.id
        assert float((ref["db"] - db).abs().max()) <= 1e-12 * max(1.0, float(db.abs().max())), case.id
        if case.dyx >= 0:
            assert float((ref["gy"] - d64).abs().max()) <= 1e-13 * max(1.0, float(d64.abs().max()))
        if regime == "int":
            assert torch.equal(dw, dw.round()) and torch.equal(db, db.round())


@pytest.mark.parametrize("case", [c for c in HOST_CASES if small(c)], ids=lambda c: c.id)
def test_int_regime_is_exact_in_float32(case):
    ref = ref_of(case, "int")
    m = V.int_exact_margin(case, ref)
    print(f"{case.id}: largest absolute sum / 2^24 = {m:.4f}")
    assert m < 1.0
    assert torch.equal(ref["dw"].float().double(), ref["dw"]) and torch.equal(ref["db"].float().double(), ref["db"])
    if case.dyx >= 0:
        assert torch.equal(ref["gy"], ref["gy"].round())


def test_int_margin_of_the_large_persistent_cases():
    """The 520 / 776-tile cases are not evaluated on the host; their margin follows from the element ranges: |x'| <= 4 (no
    transform on these), |dy| <= 4, terms per weight = B*Qh*Qw."""
    for c in HOST_CASES:
        if not small(c):
            assert c.xf < 0 and c.dyx < 0
            assert 16 * c.geom().Mc < 2 ** 24, c.id


@pytest.mark.parametrize("case", V.ALL_CASES + V.ERROR_CASES, ids=lambda c: c.id)
def test_case_hits_what_it_names(case):
    pl = V.plan(case)
    g = case.geom()
    assert pl.rc == case.rc, (pl.rc, case.rc)
    if case.rc:
        return
    assert pl.kernel == case.expect[0], pl.kernel
    if case.S is not None:
        assert pl.S == case.S, pl.S
    if case.red is not None:
        assert pl.red_w[:2] == case.red, pl.red_w
    print(f"{case.id}: {pl.kernel} S={pl.S} cps={pl.cps} tiles={pl.tiles}/{pl.nwg} red_w={pl.red_w} red_b={pl.red_b} L={V.chain_links(case, pl)}")


def test_named_properties():
    P = {c.id: (c, V.plan(c), c.geom()) for c in V.ALL_CASES}
    pow2 = lambda v: v & (v - 1) == 0
    c, pl, g = P["f-pow2"]
    assert pow2(g.Qh) and pow2(g.Qw) and pow2(g.gC)
    c, pl, g = P["f-npow2-c48-n68"]
    assert not pow2(g.Qw) and not pow2(g.gC) and (g.ntaps[0] * g.gC) % 64 and g.sC % 64 and g.Mc % 32
    nch = V.ceil_div(g.Mc, 32)
    assert 0 < nch - (pl.S - 1) * pl.cps < pl.cps                       # the last split is shorter
    c, pl, g = P["f-s12-1x1"]
    assert pl.S >= 9 and pl.S % 8 and pl.S // 8 >= 1
    c, pl, g = P["b-128-256-k4s2"]
    assert g.Mc == 8192 and sum(n * g.gC // 128 for n in g.ntaps) * (g.sC // 128) == 32
    c, pl, g = P["f-below-big"]
    assert g.Mc < 8192 and P["b-128-256-k4s2"][0].args()[2:] == c.args()[2:]
    assert max(t[0] for t in P["g-k4s1p0"][2].taps[0]) == 3 and min(t[0] for t in P["g-t-k4s1p0"][2].taps[0]) == -3
    g = P["g-k3s2-parity"][2]
    assert [t[2] for t in g.taps[0]] != sorted(t[2] for t in g.taps[0]) and sorted(t[2] for t in g.taps[0]) == list(range(9))
    assert P["g-t-k4s2"][2].ntaps == [4, 4, 4, 4] and P["g-t-k3s2-512-256"][2].ntaps == [1, 2, 2, 4]
    # persistent grids: slightly more tiles than workgroups -> some workgroups take two tiles, some one
    for cid, cap in (("up-520", V.UP_WGS), ("enc-520", V.ENC_WGS), ("img-520", V.IMG_WGS), ("thin-776", V.THIN_WGS), ("thin-t64-776", V.THIN_WGS)):
        c, pl, g = P[cid]
        assert cap < pl.tiles < 2 * cap and pl.nwg == cap, (cid, pl.tiles)
    for cid in ("up-1tile", "enc-1tile", "img-1tile", "thin-32-k3p0", "thin-t32-k4s2", "thin-t64-k4s2", "thin-64-k3p1", "thin-64-k3s2-lds"):
        assert P[cid][1].tiles == 1, cid
    # the four thin instantiations (LP = gC/4, TMAX = 4 | 9) and the LDS size
    inst = {cid: (P[cid][2].gC // 4, 4 if max(P[cid][2].ntaps) <= 4 else 9) for cid in ("thin-32-k3p0", "thin-t32-k4s2", "thin-t64-k4s2", "thin-64-k3p1")}
    assert sorted(inst.values()) == [(8, 4), (8, 9), (16, 4), (16, 9)]
    assert 64 * 1024 < V.thin_patch(P["thin-64-k3s2-lds"][2])[2] <= 160 * 1024
    assert all(V.thin_patch(P[cid][2])[2] <= 64 * 1024 for cid in inst)
    # the suspicion: geometry that passes every other thin condition, past the patch / LDS / tap limits
    g = P["g-thin-32-3-k3s2"][2]
    PH, PW, _ = V.thin_patch(g)
    assert (PH, PW) == (17, 65) and PH * PW >= 900 and g.Qh % 8 == 0 and g.Qw % 32 == 0 and max(g.ntaps) <= 9
    assert max(P["g-thin-32-3-k4s2"][2].ntaps) == 16 and max(P["g-thin-64-3-k4s2"][2].ntaps) == 16     # 16 taps: never thin
    g = P["g-thin-64-3-k4s2"][2]
    assert V.thin_patch(g)[:2] == (18, 34) and V.thin_patch(g)[2] > 160 * 1024 and g.Qh % 8 == 0 and g.Qw % 16 == 0
    # Winograd: B = 8 meets the floor of 128 workgroups, B = 7 does not
    assert V.wino_wgrad_splits(P["wino-b8"][2], V.WS_BYTES // 4) == 8 and V.wino_wgrad_splits(P["wino-b7"][2], V.WS_BYTES // 4) == 0
    # reductions: all six shapes, and bias jobs of both forms
    shapes = {V.plan(c).red_w[:2] for c in V.REDUCE_CASES}
    assert shapes == {(1, 1), (1, 0), (0, 1), (0, 0), (2, 1), (2, 0)}
    assert P["r-wide-vec"][1].n == 294912 and P["r-wide-vec"][1].S >= 9
    # deferred test: 13 calls with bias = 26 jobs = two launches, one layer twice
    assert len(set(V.DEFER_IDS)) == 13 and V.DEFER_JOBS_PER_LAUNCH < 2 * len(V.DEFER_IDS) <= 2 * V.DEFER_JOBS_PER_LAUNCH
    assert V.DEFER_TWICE in V.DEFER_IDS
    for i in V.DEFER_IDS:
        c = V.case_by_id(i)
        pl, small_ws = V.plan(c), V.plan(dataclasses.replace(c, ws_floats=V.DEFER_WS_FLOATS))
        assert pl.family in ("plain", "fast64") and (small_ws.kernel, small_ws.S) == (pl.kernel, pl.S)
        assert V.wgrad_ws_floats(c.geom(), pl.S) <= V.DEFER_WS_FLOATS


EMUL_MAX = 1 << 26           # Mc * gC * sC * taps of a case the emulation runs chunk by chunk


@pytest.mark.parametrize("case", [c for c in HOST_CASES if small(c)], ids=lambda c: c.id)
def test_float32_emulation_stays_inside_the_randn_bounds(case):
    g, pl = case.geom(), V.plan(case)
    ref = ref_of(case, "randn")
    bnd = V.bounds(case, pl, ref)
    work = g.Mc * g.gC * g.sC * g.taps_total
    orders = [("naive", 32), ("pairwise", 32)] if work <= EMUL_MAX * 64 else []
    if g.Mc * g.taps_total <= 6000:
        orders.append(("naive", 1))
    assert orders or case.id in ("b-128-256-k4s2", "f-below-big", "r-wide-vec"), case.id   # the largest GEMMs: by chunks only, below
    if not orders:
        orders = [("naive", 32)]
    for order, unit in orders:
        got = V.emulate_chunked(case, pl, "randn", order, unit).double()
        ratio = float(((got - ref["dw"]).abs() / bnd["dw"]).max())
        print(f"{case.id} {order}/{unit}: L = {bnd['L']}, max err/bound = {ratio:.4f}")
        assert ratio <= 1.0
        assert ratio > 0.0 or float(ref["aw"].max()) == 0.0


def test_winograd_identity_and_its_absolute_form():
    """wino_sums() is the weight gradient (so its absolute form bounds what a Winograd evaluation can round), and the absolute
    form is never below the direct sum's."""
    case = V.case_by_id("wino-b8")
    x, dy, _, _ = V.make_inputs(case, "randn")
    ref = ref_of(case, "randn")
    w = V.wino_sums(case.geom(), x.double(), dy.double())
    assert float((w - ref["dw"]).abs().max()) <= 1e-11 * float(ref["dw"].abs().max())
    wa = V.wino_sums(case.geom(), x.double(), dy.double(), absolute=True)
    assert bool((wa >= w.abs()).all()) and bool((wa >= ref["aw"] * (1 - 1e-12)).all())
    print(f"absolute Winograd sum / direct absolute sum: max {float((wa / ref['aw']).max()):.2f}")
    for cid in ("wino-b8", "wino-ws-s3"):                       # a float32 Winograd evaluation stays inside the bound
        c = V.case_by_id(cid)
        pl, r = V.plan(c), ref_of(c, "randn")
        ratio = float(((V.emulate_wino32(c, pl).double() - r["dw"]).abs() / V.bounds(c, pl, r)["dw"]).max())
        print(f"{cid}: float32 Winograd, max err/bound = {ratio:.4f}")
        assert 0.0 < ratio <= 1.0
        exact32 = V.emulate_wino32(c, pl, "int").double()
        assert torch.equal(exact32, ref_of(c, "int")["dw"])     # and is exact on the integer inputs


@pytest.fixture(scope="module")
def emul():
    here = os.path.dirname(os.path.abspath(__file__))
    src, so = os.path.join(here, "host_emul", "geom_emul.cpp"), os.path.join(here, "host_emul", "_geom_emul.so")
    hdr = os.path.join(os.path.dirname(here), "ct-vae_amd", "csrc", "geom.hpp")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", so, src])
    lib = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)
    lib.emul_wgrad.argtypes = [ctypes.c_int, fp, fp, fp] + [ctypes.c_int] * 9
    return lib


@pytest.mark.parametrize("case", [c for c in V.GENERIC_CASES + V.GEOMETRY_CASES + V.DEDICATED_CASES
                                  if c.xf < 0 and c.dyx < 0 and c.geom().Mc * c.Ci * c.Co * c.k * c.k <= 1 << 28], ids=lambda c: c.id)
def test_geometry_agrees_with_build_geom(emul, case):
    """csrc/geom.hpp itself (tests/host_emul: naive loops over build_geom's tap tables, weight strides included) on integer
    data: exact, so the ported tables must give the same weight gradient bit for bit."""
    x, dy, _, _ = V.make_inputs(case, "int")
    ref = ref_of(case, "int")
    xn, dn = x.numpy(), dy.numpy()
    dw = np.zeros(tuple(ref["dw"].shape), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert emul.emul_wgrad(case.kind, p(xn), p(dn), p(dw), case.B, case.H, case.W, case.Ci, case.Co, case.k, case.s, case.p, case.op) == 0
    assert np.array_equal(dw.astype(np.float64), ref["dw"].numpy())
