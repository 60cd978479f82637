"""GPU: the vector-quantiser kernels of csrc/vq.hip, op by op and on every dispatch path, against the float64 reference of
tests/vq_checks.py (pinned to the oracle, and its input conditions evaluated, in tests/test_vq_reference_host.py).

Index search (ctvae_vq_inds): exact integer data (indices must EQUAL the first-minimum arg-min), planted duplicate codes (the
lower index must win), random data (every row within a derived float32 bound of the true minimum).  Lookup + loss
(ctvae_vq_lookup) and backward (ctvae_vq_backward): given indices, float64 autograd of the reference's own expression, plus an
integer variant whose codebook gradient must equal the reference exactly.  Each case asserts, through the library's launch log,
the kernel the launcher picked.  Every output buffer is pre-filled (-1 / NaN), so a row or element a kernel skips is seen.
"""
import pytest
import torch

from tests import vq_checks as V

pytestmark = pytest.mark.gpu

NAN = float("nan")
IND = {c.id: c for c in V.IND_CASES}
# latent gradient: |got - want| <= LAT_FACTOR * (1e-6 * max(1, |want|_inf) + 1e-5 * |want|).  Measured on an MI355X over every
# case below: 0.042 at most (pos-P245, skewed indices), i.e. 4e-8 * max(1, |want|_inf) + 4e-7 * |want|; the bound is 4x that.
LAT_FACTOR = 0.16
# one case per codebook-gradient path (and per reduce shape) for the tests that need not visit all of BWD_CASES
BWD_ONE_PER_PATH = ["pos-P245", "pos-P2053-S9", "pos-C8-Dc5-K100", "posw-Dc128-P75", "posw-Dc33-K73-C2", "scan1-K80-P100",
                    "scan1-Dc256-K16", "scanS2-K512-P2048", "scanS5-K200-Dc40-P2587"]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import kernels
    from ctvae_amd import native
    native.load()
    return kernels


def _native():
    from ctvae_amd import native
    return native


def _dev():
    return torch.device("cuda")


def logged(fn):
    """Run fn with the library's launch log on; returns (fn's result, {label: ...})."""
    native = _native()
    native.prof_report()                       # drop whatever an earlier test left
    native.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    return out, native.prof_report()


# ---------------------------------------------------------------------------------------------------------------------
# index search
# ---------------------------------------------------------------------------------------------------------------------
def run_inds(case, x, E, K_=None):
    """ctvae_vq_inds on x [P, D], E [C, K, Dc] -> rows [P, C] on the host.  The index buffer starts as -1."""
    native, dev = _native(), _dev()
    K_ = case.K if K_ is None else K_
    xd, Ed = x.to(dev), E.contiguous().to(dev)
    inds = torch.full((case.B, case.C, case.HW), -1, dtype=torch.int64, device=dev)
    native.call("ctvae_vq_inds", xd.data_ptr(), Ed.data_ptr(), inds.data_ptr(), case.B, case.HW, case.D, K_, case.C)
    torch.cuda.synchronize()
    rows = V.rows_of(inds.cpu())
    assert int(rows.min()) >= 0 and int(rows.max()) < K_, "a row was not written, or an index is out of range"
    return rows


def assert_within_tol(case, what, d, rows, tol, mask=None):
    ex = V.excess(d, rows, tol)
    ratio = ex / tol
    if mask is not None:
        ex, ratio = ex[mask], ratio[mask]
    bad = int((ex > 0).sum())
    print(f"{case.id}/{what}: max (dist[chosen] - min - tol) / tol = {float(ratio.max()):.3f} (<= 0 passes), "
          f"{int((rows != V.first_argmin(d)).sum())} of {rows.numel()} indices differ from the float64 arg-min")
    assert bad == 0, f"{case.id}/{what}: {bad} rows chose a code farther than tol from the nearest"


@pytest.mark.parametrize("case", V.IND_CASES, ids=lambda c: c.id)
def test_inds_exact_data_equal_first_argmin(K, case):
    x, E = V.exact_inputs(case)
    want = V.first_argmin(V.dist64(x, E))
    rows, rep = logged(lambda: run_inds(case, x, E))
    assert list(rep) == [V.IND_LABEL[case.path]], sorted(rep)
    wrong = rows != want
    assert not bool(wrong.any()), (f"{int(wrong.sum())} of {wrong.numel()} indices differ; first (row, codebook): "
                                   f"{wrong.nonzero()[0].tolist()} got {int(rows[wrong][0])} want {int(want[wrong][0])}")
    # the autograd-free wrapper the models call returns the same tensor
    dev = _dev()
    Ed = E.to(dev)
    got = K.vq_compute_inds(x.view(case.B, case.HW, 1, case.D).to(dev), [Ed[i] for i in range(case.C)], case.K, case.C)
    assert got.shape == (case.B, case.C, case.HW, 1) and got.dtype == torch.int64
    assert torch.equal(V.rows_of(got.view(case.B, case.C, case.HW).cpu()), want)


@pytest.mark.parametrize("case", [c for c in V.IND_CASES if c.K > 1 and c.B < 600], ids=lambda c: c.id)
def test_inds_planted_duplicates_return_the_lower_index(K, case):
    x, E, planted, want = V.planted_inputs(case)
    rows = run_inds(case, x, E)
    wrong = (rows != want) & planted
    assert not bool(wrong.any()), (f"{int(wrong.sum())} of {int(planted.sum())} planted rows: got "
                                   f"{rows[wrong][:8].tolist()} want {want[wrong][:8].tolist()}")
    d = V.dist64(x, E)
    assert_within_tol(case, "planted, other rows", d, rows, V.tol_rows(x, E), ~planted)


@pytest.mark.parametrize("cid,kind", V.IND_RANDOM, ids=lambda v: v)
def test_inds_random_data_within_the_float32_bound(K, cid, kind):
    case = IND[cid]
    x, E = V.random_inputs(case, kind)
    rows, rep = logged(lambda: run_inds(case, x, E))
    assert list(rep) == [V.IND_LABEL[case.path]], sorted(rep)
    assert_within_tol(case, kind, V.dist64(x, E), rows, V.tol_rows(x, E))


@pytest.mark.parametrize("case", [c for c in V.IND_CASES if c.path == "reg" and c.K == 64 and c.B < 600], ids=lambda c: c.id)
def test_inds_register_and_generic_kernels_agree(K, case):
    """The register-blocked kernel promises the generic kernel's arithmetic: the same exact data with one far-away code row
    appended (K = 65, which only the generic kernel serves) gives the same indices."""
    x, E = V.exact_inputs(case)
    rows, rep = logged(lambda: run_inds(case, x, E))
    assert list(rep) == ["vq_inds_reg_kernel"]
    E65 = torch.cat([E, torch.full((case.C, 1, E.shape[2]), 100.0)], 1)
    rows65, rep65 = logged(lambda: run_inds(case, x, E65, 65))
    assert list(rep65) == ["vq_inds_kernel"]
    assert torch.equal(rows, rows65)


# ---------------------------------------------------------------------------------------------------------------------
# lookup + loss
# ---------------------------------------------------------------------------------------------------------------------
def run_lookup(case, x, E, inds, beta, nan_ws=False, ws_floats=None):
    native, dev = _native(), _dev()
    xd, Ed, idd = x.to(dev), E.contiguous().to(dev), inds.to(dev)
    q = torch.full_like(xd, NAN)
    loss = torch.full((), NAN, device=dev)
    ws = native.workspace(dev)
    if nan_ws:
        ws.fill_(NAN)
    native.call("ctvae_vq_lookup", xd.data_ptr(), Ed.data_ptr(), idd.data_ptr(), q.data_ptr(), loss.data_ptr(), float(beta),
                case.B, case.HW, case.D, case.K, case.C, ws.data_ptr(), (ws.numel() if ws_floats is None else ws_floats) * 4)
    torch.cuda.synchronize()
    return q.cpu(), loss.cpu()


@pytest.mark.parametrize("kind", ["uniform", "skewed"])
@pytest.mark.parametrize("case,beta", V.LOOKUP_CASES, ids=lambda v: v.id if isinstance(v, V.Case) else f"beta{v}")
def test_lookup_and_loss(K, case, beta, kind):
    x, E = V.random_inputs(case, "o1")
    inds = V.given_inds(case, kind)
    (q, loss), rep = logged(lambda: run_lookup(case, x, E, inds, beta, nan_ws=True))
    assert list(rep) == ["vq_lookup+loss_finish"]
    assert torch.equal(q, V.quantized32(x, E, inds))
    want = float(V.reference64(x, E, inds, beta)["vq_loss"])
    err = abs(float(loss) - want)
    print(f"lookup {case.id}/{kind}: vq_loss {float(loss):.8f} want {want:.8f} |err| / max(1, |want|) = {err / max(1.0, abs(want)):.2e}")
    assert err <= 1e-5 * max(1.0, abs(want))


def test_lookup_argument_errors_launch_nothing(K):
    ok = V.Case("C8", 64, 8, 8, 4, 2, None)
    x, E = V.random_inputs(ok, "o1")
    run_lookup(ok, x, E, V.given_inds(ok, "uniform"), 0.25)                       # C = 8 and an exact-size workspace are served
    run_lookup(ok, x, E, V.given_inds(ok, "uniform"), 0.25, ws_floats=1024 * 8)
    for case, ws_floats, code in [(V.Case("C9", 72, 8, 9, 4, 2, None), None, -22),
                                  (V.Case("D%C", 130, 8, 4, 4, 2, None), None, -22),
                                  (ok, 1024 * 8 - 1, -12)]:
        Dc = -(-case.D // case.C)
        x = torch.zeros(case.B * case.HW, case.D + 8)
        E = torch.zeros(case.C, case.K, Dc)
        inds = torch.zeros(case.B, case.C, case.HW, dtype=torch.int64)

        def call():
            with pytest.raises(RuntimeError, match=rf"ctvae_vq_lookup failed.*\(code {code}\)"):
                run_lookup(case, x, E, inds, 0.25, ws_floats=ws_floats)
        _, rep = logged(call)
        assert rep == {}, sorted(rep)


def test_inds_and_backward_argument_errors_launch_nothing(K):
    native, dev = _native(), _dev()
    for name, D, C in [("C9", 72, 9), ("D%C", 130, 4), ("Dc257", 257, 1)]:
        B, HW, Kc = 2, 4, 8
        x = torch.zeros(B * HW, D + 8, device=dev)
        E = torch.zeros(C, Kc, -(-D // C), device=dev)
        inds = torch.zeros(B, C, HW, dtype=torch.int64, device=dev)
        glat, dcb, gvq = torch.zeros_like(x), torch.zeros_like(E), torch.ones((), device=dev)
        ws = native.workspace(dev)

        def call():
            if name != "Dc257":                 # Dc = 257 is only beyond the BACKWARD's per-lane accumulators
                with pytest.raises(RuntimeError, match=r"ctvae_vq_inds failed.*\(code -22\)"):
                    native.call("ctvae_vq_inds", x.data_ptr(), E.data_ptr(), inds.data_ptr(), B, HW, D, Kc, C)
            with pytest.raises(RuntimeError, match=r"ctvae_vq_backward failed.*\(code -22\)"):
                native.call("ctvae_vq_backward", None, gvq.data_ptr(), x.data_ptr(), E.data_ptr(), inds.data_ptr(), glat.data_ptr(),
                            dcb.data_ptr(), 0, 0.25, B, HW, D, Kc, C, ws.data_ptr(), ws.numel() * 4)
        _, rep = logged(call)
        assert rep == {}, sorted(rep)
        assert float(glat.abs().sum()) == 0.0 and float(dcb.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def run_backward(case, x, E, inds, g_q, g_vq, beta=0.25, want_lat=True, want_cb=True, accumulate=0, prefill=NAN, nan_ws=False):
    """Raw ctvae_vq_backward.  g_q [P, D] or None, g_vq float or None.  Returns (g_latents, d_codebooks) on the host (None where
    not asked for); both start as NaN, d_codebooks as `prefill`."""
    native, dev = _native(), _dev()
    xd, Ed, idd = x.to(dev), E.contiguous().to(dev), inds.to(dev)
    gq = None if g_q is None else g_q.to(dev)
    gv = None if g_vq is None else torch.tensor(g_vq, dtype=torch.float32, device=dev)
    glat = torch.full_like(xd, NAN) if want_lat else None
    dcb = torch.full_like(Ed, prefill) if want_cb else None
    ws = native.workspace(dev)
    if nan_ws:
        ws.fill_(NAN)
    native.call("ctvae_vq_backward", native.ptr(gq), native.ptr(gv), xd.data_ptr(), Ed.data_ptr(), idd.data_ptr(),
                native.ptr(glat), native.ptr(dcb), accumulate, float(beta), case.B, case.HW, case.D, case.K, case.C,
                ws.data_ptr(), ws.numel() * 4)
    torch.cuda.synchronize()
    return (None if glat is None else glat.cpu()), (None if dcb is None else dcb.cpu())


def upstream(case, salt=0):
    """Random upstream gradients: g_q [P, D] and a scalar g_vq (a float32 value, so the reference sees the same number)."""
    g = torch.Generator().manual_seed(V.seed_of(case, 40 + salt))
    g_q = torch.randn(case.B * case.HW, case.D, generator=g)
    return g_q, float(torch.randn((), generator=g).float())


def assert_labels(case, rep):
    label, reduce = V.BWD_LABEL[case.path]
    assert [k for k in V.BWD_ALL_LABELS if k in rep] == [label], sorted(rep)
    assert ("vq_cb_reduce_kernel" in rep) == reduce, sorted(rep)


def check_lat(case, what, got, want):
    """Each element is a sum of at most min(C, Dc) <= 8 float32 terms: rounding of a short sum."""
    winf = float(want.abs().max())
    scaled = (got.double() - want).abs() / (1e-6 * max(1.0, winf) + 1e-5 * want.abs())
    print(f"bwd {case.id}/{what}: latent gradient max scaled error {float(scaled.max()):.4f} (|want|_inf {winf:.3e})")
    assert torch.isfinite(got).all()
    assert float(scaled.max()) <= LAT_FACTOR
    Dc = case.D // case.C
    assert float(got[:, case.C - 1 + Dc:].abs().sum()) == 0.0      # columns no codebook's slice reaches


def check_cb(case, what, got, want):
    winf = float(want.abs().max())
    err = float((got.double() - want).abs().max()) / max(1.0, winf)
    l2 = float((got.double() - want).norm() / want.norm().clamp_min(1e-300))
    print(f"bwd {case.id}/{what} [{case.path}]: codebook gradient max |err| / max(1, |want|_inf) = {err:.2e}, rel L2 = {l2:.2e}")
    assert torch.isfinite(got).all()
    assert err <= 1e-4 and l2 < 1e-5


def unused_codes(case, inds):
    counts = torch.stack([torch.bincount(r, minlength=case.K) for r in V.rows_of(inds).t()])
    return counts == 0                                             # [C, K]


def _flat_codebooks(E, dev):
    C, Kc, Dc = E.shape
    n = Kc * Dc
    pbuf = E.to(dev).reshape(-1).clone()
    gbuf = torch.zeros_like(pbuf)
    params = [torch.nn.Parameter(pbuf[i * n:(i + 1) * n].view(Kc, Dc)) for i in range(C)]
    for i, p in enumerate(params):
        p.grad = gbuf[i * n:(i + 1) * n].view(Kc, Dc)
    return params, gbuf


@pytest.mark.parametrize("kind", ["uniform", "skewed"])
@pytest.mark.parametrize("case", V.BWD_CASES, ids=lambda c: c.id)
def test_backward_through_vqlookup(K, case, kind):
    """Forward + backward through the autograd function the models use, codebook parameters and their .grad tensors views of
    one buffer each (what flatten_parameters arranges); latent and codebook gradient against float64 autograd."""
    dev = _dev()
    x, E = V.random_inputs(case, "o1")
    inds = V.given_inds(case, kind)
    g_q, g_vq = upstream(case)
    ref = V.reference64(x, E, inds, 0.25, g_q, g_vq)
    params, gbuf = _flat_codebooks(E, dev)
    lat = x.view(case.B, case.HW, 1, case.D).to(dev).requires_grad_(True)

    def step():
        q, loss = K.VQLookup.apply(lat, inds.view(case.B, case.C, case.HW, 1).to(dev), 0.25, case.K, case.C, *params)
        torch.autograd.backward([q, loss], [g_q.view_as(q).to(dev), torch.tensor(g_vq, device=dev)])
        return q, loss
    (q, loss), rep = logged(step)
    assert_labels(case, rep)
    assert "vq_lookup+loss_finish" in rep
    assert torch.equal(q.detach().cpu().view(-1, case.D), V.quantized32(x, E, inds))
    assert abs(float(loss.detach()) - float(ref["vq_loss"])) <= 1e-5 * max(1.0, abs(float(ref["vq_loss"])))
    check_lat(case, kind, lat.grad.cpu().view(-1, case.D), ref["g_lat"])
    got = gbuf.cpu().view(case.C, case.K, -1)
    check_cb(case, kind, got, ref["d_cb"])
    if kind == "skewed":
        none = unused_codes(case, inds)
        assert bool(none.any()) and float(got[none].abs().max()) == 0.0      # a code nobody chose gets exactly 0.0
    # a second backward accumulates into the same .grad views
    step()
    torch.cuda.synchronize()
    check_cb(case, kind + ", second backward", gbuf.cpu().view(case.C, case.K, -1), 2 * ref["d_cb"])


@pytest.mark.parametrize("kind", ["uniform", "skewed"])
@pytest.mark.parametrize("case", V.BWD_CASES, ids=lambda c: c.id)
def test_backward_exact_codebook_gradient(K, case, kind):
    """Integer inputs and g_vq = P*Dc/2 (the kernels' scale is then exactly 1): every count, sum and difference is a small
    integer in any order, so the codebook gradient must EQUAL the reference -- one dropped or doubled position shows.  With
    accumulate = 1 onto 0.125 the sum is still exact.  (The position-major kernels count hits in float: exact up to 2^24 hits
    per table, far beyond any shape here or in the models.)"""
    x, E = V.exact_inputs(case)
    inds = V.given_inds(case, kind)
    want = V.exact_dcb(case, x, E, inds)
    (_, got), rep = logged(lambda: run_backward(case, x, E, inds, None, V.exact_gvq(case), want_lat=False))
    assert_labels(case, rep)
    bad = got.double() != want
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements; first {bad.nonzero()[0].tolist()}: " \
                                f"{float(got[bad][0])} want {float(want[bad][0])}"
    _, got = run_backward(case, x, E, inds, None, V.exact_gvq(case), want_lat=False, accumulate=1, prefill=0.125)
    assert torch.equal(got.double(), want + 0.125)


@pytest.mark.parametrize("case", V.BWD_CASES, ids=lambda c: c.id)
def test_backward_accumulate_flag(K, case):
    x, E = V.random_inputs(case, "o1")
    inds = V.given_inds(case, "skewed", 1)
    g_q, g_vq = upstream(case, 1)
    want = V.reference64(x, E, inds, 0.25, g_q, g_vq)["d_cb"]
    (_, got), rep = logged(lambda: run_backward(case, x, E, inds, g_q, g_vq, accumulate=1, prefill=0.125))
    assert_labels(case, rep)
    check_cb(case, "accumulate=1", got, want + 0.125)
    _, got = run_backward(case, x, E, inds, g_q, g_vq, accumulate=0, prefill=0.125)
    check_cb(case, "accumulate=0", got, want)
    assert float(got[unused_codes(case, inds)].abs().max()) == 0.0           # the pre-fill is gone, not just small


@pytest.mark.parametrize("cid", BWD_ONE_PER_PATH)
def test_backward_null_pointer_contract(K, cid):
    case = V.case_of(V.BWD_CASES, cid)
    x, E = V.random_inputs(case, "o1")
    inds = V.given_inds(case, "uniform", 2)
    g_q, g_vq = upstream(case, 2)
    # no upstream gradient of the quantised tensor: only the loss term remains
    ref = V.reference64(x, E, inds, 0.25, None, g_vq)
    glat, dcb = run_backward(case, x, E, inds, None, g_vq)
    check_lat(case, "g_q absent", glat, ref["g_lat"])
    check_cb(case, "g_q absent", dcb, ref["d_cb"])
    # no upstream gradient of the loss: pure straight-through, bit for bit; the codebooks get exactly zero
    glat, dcb = run_backward(case, x, E, inds, g_q, None)
    assert torch.equal(glat, V.straight_through32(g_q, case.C))
    if case.C == 1:
        assert torch.equal(glat, g_q)
    assert float(dcb.abs().max()) == 0.0
    # one output only
    ref = V.reference64(x, E, inds, 0.25, g_q, g_vq)
    (glat, dcb), rep = logged(lambda: run_backward(case, x, E, inds, g_q, g_vq, want_cb=False))
    assert dcb is None and not [k for k in rep if k.startswith("vq_bwd_codebook") or k == "vq_cb_reduce_kernel"], sorted(rep)
    check_lat(case, "d_codebooks not wanted", glat, ref["g_lat"])
    (glat, dcb), rep = logged(lambda: run_backward(case, x, E, inds, g_q, g_vq, want_lat=False))
    assert glat is None
    assert_labels(case, rep)
    check_cb(case, "g_latents not wanted", dcb, ref["d_cb"])


@pytest.mark.parametrize("case", V.BWD_CASES, ids=lambda c: c.id)
def test_backward_and_lookup_are_reproducible_and_read_no_stale_scratch(K, case):
    """The same calls twice, the scratch buffer filled with NaN before each: bit-identical and finite (the file promises
    "no atomics, bit-reproducible" for every codebook-gradient form; no path may read scratch it did not write)."""
    x, E = V.random_inputs(case, "o1")
    inds = V.given_inds(case, "skewed", 3)
    g_q, g_vq = upstream(case, 3)
    runs = []
    for _ in range(2):
        q, loss = run_lookup(case, x, E, inds, 0.25, nan_ws=True)
        glat, dcb = run_backward(case, x, E, inds, g_q, g_vq, nan_ws=True)
        runs.append((q, loss, glat, dcb))
    for a, b in zip(*runs):
        assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("cid", ["pos-P245", "posw-Dc33-K73-C2"])
def test_vqlookup_mixed_fresh_and_accumulating_codebooks(K, cid):
    """VQLookup.backward's mixed branch: codebook 0's gradient block is declared zero but not written (zero_grad(lazy=True):
    its .grad holds stale values that must not survive), codebook 1's already holds a gradient.  One launch serves both: the
    fresh block is cleared and everything accumulates -- old + new per codebook."""
    from ctvae_amd.models.packing import _GradBlock
    dev = _dev()
    case = V.case_of(V.BWD_CASES, cid)
    x, E = V.random_inputs(case, "o1")
    inds = V.given_inds(case, "uniform", 4)
    g_q, g_vq = upstream(case, 4)
    want = V.reference64(x, E, inds, 0.25, g_q, g_vq)["d_cb"]
    params, gbuf = _flat_codebooks(E, dev)
    n = params[0].numel()
    for i, p in enumerate(params):
        p._grad_block = _GradBlock(i * n, (i + 1) * n)
        p._grad_block.fresh = i == 0
        p.grad.fill_(7.0 if i == 0 else 0.5)
    old = torch.full_like(want, 0.5)
    old[0] = 0.0
    lat = x.view(case.B, case.HW, 1, case.D).to(dev).requires_grad_(True)
    q, loss = K.VQLookup.apply(lat, inds.view(case.B, case.C, case.HW, 1).to(dev), 0.25, case.K, case.C, *params)
    torch.autograd.backward([q, loss], [g_q.view_as(q).to(dev), torch.tensor(g_vq, device=dev)])
    torch.cuda.synchronize()
    assert not any(p._grad_block.fresh for p in params)
    check_cb(case, "mixed fresh / accumulating", gbuf.cpu().view(case.C, case.K, -1), old + want)
    # all blocks fresh: overwritten, the stale values gone
    for p in params:
        p._grad_block.fresh = True
        p.grad.fill_(7.0)
    q, loss = K.VQLookup.apply(lat, inds.view(case.B, case.C, case.HW, 1).to(dev), 0.25, case.K, case.C, *params)
    torch.autograd.backward([q, loss], [g_q.view_as(q).to(dev), torch.tensor(g_vq, device=dev)])
    torch.cuda.synchronize()
    check_cb(case, "all fresh", gbuf.cpu().view(case.C, case.K, -1), want)
    # gradients that do not sit back to back are refused, not written somewhere else
    params[1].grad = torch.zeros_like(params[1])
    q, loss = K.VQLookup.apply(lat, inds.view(case.B, case.C, case.HW, 1).to(dev), 0.25, case.K, case.C, *params)
    with pytest.raises(RuntimeError, match="back to back"):
        torch.autograd.backward([q, loss], [g_q.view_as(q).to(dev), torch.tensor(g_vq, device=dev)])
