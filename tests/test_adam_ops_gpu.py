"""GPU: the fused Adam kernels of csrc/pointwise.hip op by op through the C ABI, against the float64 references of
tests/adam_checks.py.  The references are pinned to torch, their bounds sized and the case tables' launch geometry asserted in
tests/test_adam_reference_host.py.  tests/test_grad_clip_gpu.py and tests/test_adam_blocks_gpu.py stay as the multi-step,
torch-facing layer above this one.

Every buffer is a slice of a larger allocation with 8 guard words of a sentinel bit pattern on each side (one more in front for
a buffer shifted by one float); the guards must be bit-unchanged afterwards, and so must the gradient.  The clip workspace and
norm_out hold NaN before every call.  Every launch, and every sequence of three launches, of the step entry points runs twice
from identical inputs and all outputs must be bit-identical (not repeated: the 2000-launch sequence, whose every state is
checked against its exact value, and ctvae_adam_mark_members, whose words are compared with exact expectations).  The launch
log names the kernels that ran.  One launch is checked output by output: m', v' from the inputs, p' from the returned
moments, the clip factor from the reported norm -- every element, each under its derived bound (adam_checks.py).

entry point -> cases
  ctvae_adam_step (adam_kernel<16-byte / scalar>)                   test_step_against_float64 (mode off), test_state_and_tickets,
                                                                    test_beta_powers_over_many_launches, test_mixed_alignment,
                                                                    test_zero_gradient_is_a_fixed_point, test_refusals
  ctvae_adam_step_clipped (grad_sqnorm_kernel, adam_clip_kernel)    test_step_against_float64 (value, norm active / inactive),
                                                                    test_state_and_tickets, test_mixed_alignment,
                                                                    test_clip_edges_value, test_clip_edges_norm,
                                                                    test_zero_gradient_is_a_fixed_point, test_refusals
  ctvae_adam_step_blocks (grad_sqnorm_kernel, adam_blocks_kernel)   test_blocks_against_float64, test_blocks_all_or_none_active,
                                                                    test_blocks_with_every_block_active_equal_the_plain_kernels,
                                                                    test_state_and_tickets, test_mixed_alignment,
                                                                    test_zero_gradient_is_a_fixed_point, test_refusals
  ctvae_adam_mark_members                                           test_mark_members, test_refusals
  ctvae_adam_state_floats, ctvae_grad_clip_workspace_floats         test_state_and_tickets
"""
import numpy as np
import pytest
import torch

from tests import adam_checks as V

pytestmark = pytest.mark.gpu

SENT = 0x7FA5C3D2                      # a NaN with a payload no kernel produces
ADAM_KERNELS = ("adam_kernel", "adam_clip_kernel", "grad_sqnorm_kernel", "adam_blocks_kernel")
f32 = np.float32


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import native
    lib = native.load()
    assert int(lib.ctvae_adam_state_floats()) == V.STATE_FLOATS
    assert int(lib.ctvae_grad_clip_workspace_floats()) == V.CLIP_MAX_WGS
    return native


def framed(data, off=0):
    """data (fp32 or int32 numpy) inside 8 + off / 8 guard words: (whole allocation, the slice), both int32 views."""
    data = np.ascontiguousarray(data)
    n = data.shape[0]
    base = torch.full((n + 17,), SENT, dtype=torch.int32, device="cuda")
    assert base.data_ptr() % 16 == 0
    view = base[8 + off: 8 + off + n]
    view.copy_(torch.from_numpy(data.view(np.int32)))
    return base, view


def guards_intact(base, view):
    off = (view.data_ptr() - base.data_ptr()) // 4
    return bool((base[:off] == SENT).all()) and bool((base[off + view.numel():] == SENT).all())


def host(view, dtype=np.float32):
    return view.cpu().numpy().view(dtype)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def initial_state(head):
    st = np.zeros(V.STATE_FLOATS, dtype=np.float32)
    st[:8] = head
    st[8:16].view(np.int32)[:] = 0x7FB00000 + np.arange(8)            # words no kernel may touch
    return st


EXPECT_LOG = {("plain", "off"): {"adam_kernel": 1},
              ("plain", "value"): {"adam_clip_kernel": 1},
              ("plain", "norm"): {"grad_sqnorm_kernel": 1, "adam_clip_kernel": 1},
              ("blocks", "off"): {"adam_blocks_kernel": 1},
              ("blocks", "value"): {"adam_blocks_kernel": 1},
              ("blocks", "norm"): {"grad_sqnorm_kernel": 1, "adam_blocks_kernel": 1}}


def run(native, inp, offset="aligned", table=None, dev=None, want_norm=True, launches=1, state=None):
    """`launches` launches from the inputs of inp (dev: the arrays that go to the device where they differ from inp's, e.g.
    poisoned ones).  table: None (ctvae_adam_step / _clipped by mode) or dict(ranges, active, rows).  Returns the outputs on the
    host, the state words after every launch and the launch log; asserts guards, gradient and launch log."""
    mode, n = inp["mode"], inp["n"]
    offs = V.OFFSETS[offset]
    src = dict(inp if dev is None else dev)
    bufs = {k: framed(src[k], o) for k, o in zip("pgmv", offs)}
    st = framed(initial_state(inp["head"]) if state is None else state)
    ws = framed(np.full(V.CLIP_MAX_WGS, np.nan, dtype=np.float32))
    nrm = framed(np.full(1, np.nan, dtype=np.float32))
    norm_mode = mode.startswith("norm")
    ptr = {k: b[1].data_ptr() for k, b in bufs.items()}
    tb = None
    if table is not None:
        const = dict(lo=np.array([r[0] for r in table["ranges"]], dtype=np.int32),
                     hi=np.array([r[1] for r in table["ranges"]], dtype=np.int32), active=np.asarray(table["active"], dtype=np.int32))
        tb = {k: framed(a) for k, a in const.items()}
        tb["rows"] = framed(np.asarray(table["rows"], dtype=np.float32).reshape(-1))
    clip = float(inp["clip"])
    states, rows = [], []
    native.prof_report()
    native.prof_enable(True)
    try:
        for _ in range(launches):
            if table is not None:
                native.call("ctvae_adam_step_blocks", ptr["p"], ptr["g"], ptr["m"], ptr["v"], st[1].data_ptr(), n, float(inp["gs"]),
                            V.ALGORITHM[mode], 0.0 if mode == "off" else clip, ws[1].data_ptr() if norm_mode else None,
                            nrm[1].data_ptr() if (norm_mode and want_norm) else None, tb["lo"][1].data_ptr(), tb["hi"][1].data_ptr(),
                            tb["rows"][1].data_ptr(), tb["active"][1].data_ptr(), len(table["ranges"]))
            elif mode == "off":
                native.call("ctvae_adam_step", ptr["p"], ptr["g"], ptr["m"], ptr["v"], st[1].data_ptr(), n, float(inp["gs"]))
            else:
                native.call("ctvae_adam_step_clipped", ptr["p"], ptr["g"], ptr["m"], ptr["v"], st[1].data_ptr(), n, float(inp["gs"]),
                            V.ALGORITHM[mode], clip, ws[1].data_ptr() if norm_mode else None,
                            nrm[1].data_ptr() if (norm_mode and want_norm) else None)
            if launches > 1:
                states.append(st[1].clone())
                if tb is not None:
                    rows.append(tb["rows"][1].clone())
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    rep = native.prof_report()
    log = {k: v["count"] for k, v in rep.items() if k in ADAM_KERNELS}
    want_log = EXPECT_LOG[("plain" if table is None else "blocks", "norm" if norm_mode else mode)]
    assert log == {k: c * launches for k, c in want_log.items()}, log
    for name, (base, view) in list(bufs.items()) + [("state", st), ("ws", ws), ("norm", nrm)] + (list(tb.items()) if tb else []):
        assert guards_intact(base, view), f"{name}: guard words written"
    assert same(host(bufs["g"][1]), np.ascontiguousarray(src["g"])), "the gradient buffer was written"
    out = {k: host(bufs[k][1]) for k in "pmv"}
    out["norm"] = host(nrm[1])[0] if (norm_mode and want_norm) else None
    if not (norm_mode and want_norm):
        assert np.isnan(host(nrm[1])[0])
    if not norm_mode:
        assert np.isnan(host(ws[1])).all(), "the workspace was written outside norm mode"
    out["state"] = host(st[1], np.int32)
    out["states"] = [host(s, np.int32) for s in states] or [out["state"]]
    if tb is not None:
        out["rows"] = host(tb["rows"][1]).reshape(-1, 4)
        out["rows_each"] = [host(r).reshape(-1, 4) for r in rows] or [out["rows"]]
        for k, a in const.items():
            assert same(host(tb[k][1], np.int32), a), f"the table's {k} was written"
    return out


def twice(fn):
    a, b = fn(), fn()
    for k in ("p", "m", "v", "state") + (("rows",) if "rows" in a else ()):
        assert same(a[k], b[k]), f"{k}: two runs from identical inputs differ"
    assert (a["norm"] is None and b["norm"] is None) or same(np.array([a["norm"]]), np.array([b["norm"]])), "norm: two runs differ"
    for k in ("states",) + (("rows_each",) if "rows" in a else ()):   # after every launch of a sequence
        assert len(a[k]) == len(b[k]) and all(same(x, y) for x, y in zip(a[k], b[k])), f"{k}: two runs differ"
    return a


def state_after(head0, state_bits, launches=1):
    """The state words after `launches` launches: step up by exactly 1 each, the powers the fp32 products bit for bit, the other
    head words, state[8:16] and every ticket word as they were (the tickets: zero)."""
    want = initial_state(head0)
    for _ in range(launches):
        want[:8] = V.state_ref(want[:8])
    got = state_bits.view(np.float32)
    assert got[0] == head0[0] + launches
    assert same(got[6:8], want[6:8]), ("beta powers", got[6:8], want[6:8])
    assert same(got[1:6], want[1:6]) and same(got[8:16], want[8:16]), "state[1:6] / state[8:16] changed"
    left = np.flatnonzero(state_bits[V.TICKET_OFFSET:])
    assert left.size == 0, f"ticket words left set: {[(int(i), int(state_bits[V.TICKET_OFFSET + i])) for i in left[:8]]}"


def report(what, res):
    for k, (ratio, bad, _, _) in res.items():
        print(f"{what}: {k}: worst |err| / bound = {ratio:.4f}")
    for k, (ratio, bad, _, _) in res.items():
        assert bad == 0, f"{what}: {k}: {bad} elements beyond the bound, worst ratio {ratio:.3f}"


# ---------------------------------------------------------------------------------------------------------------------
# ctvae_adam_step, ctvae_adam_step_clipped
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", V.SMALL_CASES, ids=lambda c: c.id)
def test_step_against_float64(N, case):
    inp = V.adam_inputs(case)
    out = twice(lambda: run(N, inp, case.offset))
    report(case.id, V.check_step(inp, out))
    state_after(inp["head"], out["state"])


def ticket_table(n, hyper=0):
    ranges = V.make_table(n, 1, "dense")
    return dict(ranges=ranges, active=V.make_activity(len(ranges), 1, "half"), rows=V.bstate_rows(hyper, V.make_counters(len(ranges), 1)))


@pytest.mark.parametrize("kernel,n", [("adam_kernel", n) for n in V.TICKET_SCALAR] + [("adam_clip_kernel", n) for n in V.TICKET_SCALAR]
                         + [("adam_blocks_kernel", n) for n in V.TICKET_BLOCKS])
def test_state_and_tickets(N, kernel, n):
    mode = {"adam_kernel": "off", "adam_clip_kernel": "value", "adam_blocks_kernel": "off"}[kernel]
    case = V.Case(n, 0, 6, 1.0, mode, seed=n % 97)
    table = ticket_table(n) if kernel == "adam_blocks_kernel" else None
    inp = V.adam_inputs(case) if table is None else V.block_inputs(case, table["ranges"], table["active"],
                                                                   table["rows"][:, 0].astype(np.int64))
    out = twice(lambda: run(N, inp, "aligned" if table is not None else "shifted", table=table, launches=3))
    for k, bits in enumerate(out["states"]):
        state_after(inp["head"], bits, k + 1)
    if table is not None:
        want = table["rows"]
        for rows in out["rows_each"]:
            want = V.bstate_ref(want, table["active"], inp["head"][2], inp["head"][3])
            assert same(rows, want), "block-state rows"
        still = np.asarray(table["active"]) == 0
        assert still.any() and same(out["rows"][still], table["rows"][still])


def test_beta_powers_over_many_launches(N):
    T = 2000
    inp = V.adam_inputs(V.Case(4, 0, 0, 1.0, "off", seed=3))
    bufs = {k: framed(inp[k]) for k in "pgmv"}
    st = framed(initial_state(inp["head"]))
    rec = torch.zeros((T, 8), dtype=torch.int32, device="cuda")
    for t in range(T):
        N.call("ctvae_adam_step", bufs["p"][1].data_ptr(), bufs["g"][1].data_ptr(), bufs["m"][1].data_ptr(), bufs["v"][1].data_ptr(),
               st[1].data_ptr(), 4, 1.0)
        rec[t].copy_(st[1][:8])
    torch.cuda.synchronize()
    rec = rec.cpu().numpy().view(np.float32)
    bits = host(st[1], np.int32)
    assert rec[-1, 0] == T and not np.flatnonzero(bits[V.TICKET_OFFSET:]).size
    assert np.array_equal(rec[:, 0], np.arange(1, T + 1, dtype=np.float32))
    t = np.arange(1, T + 1, dtype=np.float64)
    for col, b in ((6, float(inp["head"][2])), (7, float(inp["head"][3]))):
        exact = b ** t
        normal = exact >= 2.0 * V.F32_MIN_NORMAL
        err = np.abs(rec[:, col].astype(np.float64) - exact)[normal]
        bound = (t * V.U / (1.0 - t * V.U) * exact)[normal]
        print(f"state[{col}]: normal for {int(normal.sum())} launches, worst err / (t u beta^t) = {float((err / bound).max()):.4f}")
        assert (err <= bound).all()
        assert not np.isnan(rec[:, col]).any()
    assert 0.0 <= rec[-1, 6] < V.F32_MIN_NORMAL
    assert all(guards_intact(*b) for b in list(bufs.values()) + [st])
    assert np.isfinite(host(bufs["p"][1])).all()


# ---------------------------------------------------------------------------------------------------------------------
# ctvae_adam_step_blocks
# ---------------------------------------------------------------------------------------------------------------------
def block_case(n, style, mode, gs, hyper, seed, activity="half", equal=None):
    """Inputs under a table.  Returns the inputs, the table, the arrays that go to the device (poisoned where only a wrong read
    could see it), the per-element block index and the mask of the elements that step."""
    ranges = V.make_table(n, seed, style)
    nb = len(ranges)
    act = V.make_activity(nb, seed, "all" if (style == "one" and activity == "half") else activity)
    cnt = V.make_counters(nb, seed, equal)
    t0 = 0 if equal is None else equal
    inp = V.block_inputs(V.Case(n, hyper, t0, gs, mode, seed=seed), ranges, act, cnt)
    blk = V.block_of(n, ranges)
    steps = (blk >= 0) & (act[np.maximum(blk, 0)] != 0)
    dev = {k: inp[k].copy() for k in "pgmv"}
    if not mode.startswith("norm"):                                    # the norm pass reads the whole gradient: zeros there
        dev["g"][~steps] = np.nan
        for k in "pmv":
            dev[k][blk < 0] = np.nan
    table = dict(ranges=ranges, active=act, rows=V.bstate_rows(hyper, cnt))
    return inp, table, dev, blk, steps


def check_blocks(N, what, inp, table, dev, blk, steps, offset):
    out = twice(lambda: run(N, inp, offset, table=table, dev=dev))
    for k in "pmv":
        assert same(out[k][~steps], dev[k][~steps]), f"{what}: {k} moved in a gap or in a block that does not step"
    rows = table["rows"]
    b1t, b2t = V.beta_powers(rows[np.maximum(blk, 0), 1], rows[np.maximum(blk, 0), 2], inp["head"][2], inp["head"][3])
    if steps.any():
        res = V.check_step(inp, out, steps, b1t, b2t)
        if not inp["mode"].startswith("norm"):
            res.pop("norm", None)
        report(what, res)
    elif inp["mode"].startswith("norm"):
        assert out["norm"] == 0.0
    state_after(inp["head"], out["state"])
    assert same(out["rows"], V.bstate_ref(rows, table["active"], inp["head"][2], inp["head"][3]))
    return out


@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("offset", ["aligned", "shifted"])
@pytest.mark.parametrize("mode", V.MODES)
@pytest.mark.parametrize("style", V.TABLE_STYLES)
@pytest.mark.parametrize("n", [1023, V.N_EMPTY, V.N_TWO])
def test_blocks_against_float64(N, n, style, mode, offset, gs):
    seed = V.TABLE_STYLES.index(style) + 5 * V.MODES.index(mode)       # edges: the last block ends 1, 2, 3, 0 floats before n
    inp, table, dev, blk, steps = block_case(n, style, mode, gs, seed % 3, seed)
    check_blocks(N, f"{n}-{style}-{mode}-{offset}-{gs}", inp, table, dev, blk, steps, offset)


@pytest.mark.parametrize("n", [1023, V.N_EMPTY, V.N_TWO])
@pytest.mark.parametrize("activity", ["all", "none"])
@pytest.mark.parametrize("mode", V.MODES)
def test_blocks_all_or_none_active(N, mode, activity, n):
    """None active: every workgroup classifies and skips every quad, the cursor walks the whole table, nothing moves and no
    block-state row changes, while the head still counts the launch.  All active: nothing is skipped."""
    k = V.MODES.index(mode) + (activity == "all")
    inp, table, dev, blk, steps = block_case(n, "dense", mode, (0.5, 1.0)[k % 2], k % 3, 11 + k, activity)
    assert steps.any() == (activity == "all")
    check_blocks(N, f"{n}-{activity}-{mode}", inp, table, dev, blk, steps, ("aligned", "shifted")[(k // 2) % 2])


@pytest.mark.parametrize("n", [V.N_TWO, 4 * 256 * 32 + 7])
@pytest.mark.parametrize("offset", ["aligned", "shifted"])
@pytest.mark.parametrize("gs", [1.0, 0.5])
@pytest.mark.parametrize("mode", V.MODES)
def test_blocks_with_every_block_active_equal_the_plain_kernels(N, mode, gs, offset, n):
    k = V.MODES.index(mode) + (gs == 0.5) + (offset == "shifted")
    style = ("dense", "edges")[k % 2]
    inp, table, dev, blk, steps = block_case(n, style, mode, gs, k % 3, 20 + k, "all", equal=V.T0S[k % 4])
    for name in "pgmv":                                                # zero-filled gaps, no poison: the plain kernels read them
        dev[name] = inp[name]
    assert steps.sum() == sum(hi - lo for lo, hi in table["ranges"]) and (~steps).any()
    blocks = twice(lambda: run(N, inp, offset, table=table, dev=dev))
    plain = twice(lambda: run(N, inp, offset, dev=dev))
    for name in "pmv":
        assert same(blocks[name][steps], plain[name][steps]), f"{name}: the blocks kernel differs from the plain kernel"
        assert same(blocks[name][~steps], inp[name][~steps])
    assert same(blocks["state"], plain["state"])
    if mode.startswith("norm"):
        assert same(np.array([blocks["norm"]]), np.array([plain["norm"]]))


# ---------------------------------------------------------------------------------------------------------------------
# alignment, clip edges, fixed point
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1023, 4 * 256 * 32 + 7])
@pytest.mark.parametrize("kernel", ["plain", "blocks"])
@pytest.mark.parametrize("mode", ["off", "value", "norm_active"])
def test_mixed_alignment(N, mode, kernel, n):
    if kernel == "blocks":
        inp, table, dev, _, _ = block_case(n, "dense", mode, 0.5, 0, 31)
    else:
        inp, table, dev = V.adam_inputs(V.Case(n, 0, 6, 0.5, mode, seed=31)), None, None
    got = {off: twice(lambda: run(N, inp, off, table=table, dev=dev)) for off in V.OFFSETS}
    for off in ("g_only", "pmv_only"):
        for k in ("p", "m", "v", "state"):
            assert same(got[off][k], got["shifted"][k]), f"{off}: {k} differs from the all-shifted run"
    if mode == "norm_active":
        for off in ("shifted", "g_only", "pmv_only"):                 # the reduction order is a function of n alone
            assert same(np.array([got[off]["norm"]]), np.array([got["aligned"]["norm"]])), off


EDGE_HYPER = dict(lr=1e-3, b1=0.0, b2=0.999, eps=1e-8, wd=0.0)         # b1 = 0, wd = 0, m = 0: m' IS the clipped gradient


def edge_inputs(g, gs, mode, clip):
    n = len(g)
    rng = np.random.default_rng(5)
    return dict(p=(0.3 * rng.standard_normal(n)).astype(np.float32), g=np.asarray(g, dtype=np.float32), m=np.zeros(n, dtype=np.float32),
                v=np.zeros(n, dtype=np.float32), head=V.head_at(EDGE_HYPER, 0), gs=f32(gs), clip=f32(clip), mode=mode, n=n,
                norm=V.norm_ref(np.asarray(g, dtype=np.float32), gs))


@pytest.mark.parametrize("offset", ["aligned", "shifted"])
@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_clip_edges_value(N, gs, offset):
    clip = f32(0.15)
    inside, outside = np.nextafter(clip, f32(0)), np.nextafter(clip, f32(1))
    x = np.array([clip, -clip, inside, -inside, outside, -outside, 0.0, -0.0, np.inf, -np.inf, np.nan, 0.01, -3.0], dtype=np.float32)
    want = np.array([clip, -clip, inside, -inside, clip, -clip, 0.0, 0.0, clip, -clip, np.nan, 0.01, -clip], dtype=np.float32)
    g = (x / f32(gs)).astype(np.float32)                               # a power of two: exact
    assert same((g * f32(gs)).astype(np.float32), x)
    ref = torch.from_numpy(x.astype(np.float64)).requires_grad_()
    ref.grad = ref.detach().clone()
    torch.nn.utils.clip_grad_value_([ref], float(clip))
    assert np.array_equal(ref.grad.numpy(), want.astype(np.float64), equal_nan=True)   # where clip_grad_value_ puts them
    inp = edge_inputs(g, gs, "value", clip)
    out = twice(lambda: run(N, inp, offset))
    assert np.array_equal(out["m"], want, equal_nan=True), (out["m"], want)
    nan = np.isnan(want)
    assert np.isnan(out["p"][nan]).all() and np.isnan(out["v"][nan]).all() and np.isfinite(out["p"][~nan]).all()
    report("clip edges", V.check_step(inp, out, np.isfinite(g)))      # the finite rows, output by output


@pytest.mark.parametrize("offset", ["aligned", "shifted"])
def test_clip_edges_norm(N, offset):
    clip = f32(1.0)
    edge = f32(clip + f32(1e-6))
    norms = [np.nextafter(clip, f32(0)), clip, np.nextafter(clip, f32(2)), np.nextafter(edge, f32(0)), edge, np.nextafter(edge, f32(2)), f32(0.25),
             f32(7.0)]
    for x in norms:
        for n, pos in ((4, 0), (7, 5)):                                # the one non-zero gradient in a quad, and in the tail
            g = np.zeros(n, dtype=np.float32)
            g[pos] = -x
            inp = edge_inputs(g, 1.0, "norm_active", clip)
            out = twice(lambda: run(N, inp, offset))
            assert out["norm"] == x, (out["norm"], x)                  # sqrt(fl(x^2)) == x in binary floating point
            c = V.coef_ref(out["norm"], clip)
            assert c <= 1.0 and (c == 1.0) == (float(x) + 1e-6 <= float(clip))
            assert abs(out["m"][pos]) <= x, "the clip factor exceeds 1"
            report(f"norm {float(x)!r} n {n}", V.check_step(inp, out))
            quiet = twice(lambda: run(N, inp, offset, want_norm=False))   # norm_out = NULL: the same update
            for k in ("p", "m", "v", "state"):
                assert same(quiet[k], out[k]), k
    for bad, c_want in ((np.nan, np.nan), (np.inf, 0.0)):              # a NaN norm gives c = NaN, an infinite one c = 0
        g = np.array([1.0, bad, 2.0, 0.5], dtype=np.float32)
        inp = edge_inputs(g, 1.0, "norm_active", clip)
        out = twice(lambda: run(N, inp, offset))
        assert (np.isnan(out["norm"]) and np.isnan(bad)) or out["norm"] == bad
        assert V.coef_ref(out["norm"], clip) == c_want or np.isnan(c_want)
        if np.isnan(bad):
            assert np.isnan(out["m"]).all()
        else:
            assert (out["m"][[0, 2, 3]] == 0).all() and np.isnan(out["m"][1])           # inf * 0


@pytest.mark.parametrize("offset", ["aligned", "shifted"])
@pytest.mark.parametrize("kernel", ["plain", "blocks"])
@pytest.mark.parametrize("mode", V.MODES)
def test_zero_gradient_is_a_fixed_point(N, mode, kernel, offset):
    n = 4 * 256 * 32 + 7
    inp = edge_inputs(np.zeros(n, dtype=np.float32), 0.5, mode, 1.0)
    inp["p"][3] = -0.0
    table = None
    if kernel == "blocks":
        ranges = V.make_table(n, 2, "dense")
        table = dict(ranges=ranges, active=V.make_activity(len(ranges), 2, "all"), rows=V.bstate_rows(EDGE_HYPER, np.zeros(len(ranges))))
    out = twice(lambda: run(N, inp, offset, table=table))
    for k in "pmv":
        assert same(out[k], inp[k]), k
    state_after(inp["head"], out["state"])                             # the step still counts
    if mode.startswith("norm"):
        assert out["norm"] == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# ctvae_adam_mark_members
# ---------------------------------------------------------------------------------------------------------------------
INT_MAX = 2 ** 31 - 1


@pytest.mark.parametrize("before", [0, 1])
def test_mark_members(N, before):
    def mark(nhits, group):
        hits = framed(np.full(nhits, before, dtype=np.int32))
        grp = None if group is None else framed(np.asarray(group, dtype=np.int32))
        N.call("ctvae_adam_mark_members", hits[1].data_ptr(), nhits, None if grp is None else grp[1].data_ptr(),
               0 if group is None else len(group))
        torch.cuda.synchronize()
        assert guards_intact(*hits) and (grp is None or (guards_intact(*grp) and np.array_equal(host(grp[1], np.int32), group)))
        want = np.full(nhits, before, dtype=np.int32)
        want[0] = 1
        for k in ([] if group is None else group):
            if 0 <= k < nhits:
                want[k] = 1
        got = host(hits[1], np.int32)
        assert np.array_equal(got, want), (nhits, got, want)

    mark(5, None)                                                      # group = NULL, B = 0: hits[0] alone
    mark(1, None)
    mark(1, [0, -1, 1, INT_MAX])                                       # nhits = 1: every other name is out of range
    mark(7, [3, 3, 3, -1, 7, INT_MAX, 5, 3, -2 ** 31, 6])              # duplicates, -1, nhits, INT_MAX
    rng = np.random.default_rng(1)
    for B in (1, 256, 257, 1000):
        nhits = 40
        group = rng.integers(-3, nhits + 3, B).astype(np.int64)
        group[-1] = nhits - 1                                          # the last sample, in the last workgroup
        mark(nhits, [int(k) for k in group])
        mark(2000, [int(k) for k in rng.integers(0, 2000, B)])


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals(N):
    n = 1023
    inp = V.adam_inputs(V.Case(n, 0, 6, 1.0, "norm_active", seed=2))
    ranges = V.make_table(n, 0, "dense")
    arrays = dict(p=inp["p"], g=inp["g"], m=inp["m"], v=inp["v"], state=initial_state(inp["head"]),
                  ws=np.full(V.CLIP_MAX_WGS, np.nan, dtype=np.float32), norm=np.full(1, np.nan, dtype=np.float32),
                  lo=np.array([r[0] for r in ranges], dtype=np.int32), hi=np.array([r[1] for r in ranges], dtype=np.int32),
                  rows=V.bstate_rows(0, V.make_counters(len(ranges), 0)).reshape(-1), active=V.make_activity(len(ranges), 0, "half"),
                  hits=np.zeros(8, dtype=np.int32), group=np.array([1, 2, 3], dtype=np.int32))
    bufs = {k: framed(a) for k, a in arrays.items()}
    P = {k: b[1].data_ptr() for k, b in bufs.items()}
    nb, clip = len(ranges), float(inp["clip"])

    def refused(name, *args):
        with pytest.raises(RuntimeError, match=rf"{name} failed"):
            N.call(name, *args)

    step = [P["p"], P["g"], P["m"], P["v"], P["state"], n, 1.0]
    clipped = step + [V.CLIP_NORM, clip, P["ws"], P["norm"]]
    blocks = clipped + [P["lo"], P["hi"], P["rows"], P["active"], nb]

    def without(args, i, value=None):
        return args[:i] + [value] + args[i + 1:]

    for i in range(5):                                                 # each NULL pointer in turn
        refused("ctvae_adam_step", *without(step, i))
        refused("ctvae_adam_step_clipped", *without(clipped, i))
        refused("ctvae_adam_step_blocks", *without(blocks, i))
    for i in (11, 12, 13, 14):
        refused("ctvae_adam_step_blocks", *without(blocks, i))
    for bad_n in (0, -1):
        refused("ctvae_adam_step", *without(step, 5, bad_n))
        refused("ctvae_adam_step_clipped", *without(clipped, 5, bad_n))
        refused("ctvae_adam_step_blocks", *without(blocks, 5, bad_n))
    for bad_clip in (0.0, -1.0, float("nan")):
        for alg in (V.CLIP_NORM, V.CLIP_VALUE):
            refused("ctvae_adam_step_clipped", *without(without(clipped, 8, bad_clip), 7, alg))
            refused("ctvae_adam_step_blocks", *without(without(blocks, 8, bad_clip), 7, alg))
    for alg in (-1, 3, 7):                                             # unknown algorithm (2, no clip, is the blocks kernel's alone)
        refused("ctvae_adam_step_clipped", *without(clipped, 7, alg))
        refused("ctvae_adam_step_blocks", *without(blocks, 7, alg))
    refused("ctvae_adam_step_clipped", *without(clipped, 7, V.CLIP_OFF))
    refused("ctvae_adam_step_clipped", *without(clipped, 9))          # norm mode without workspace
    refused("ctvae_adam_step_blocks", *without(blocks, 9))
    for bad_nb in (0, -1):
        refused("ctvae_adam_step_blocks", *without(blocks, 15, bad_nb))
    refused("ctvae_adam_mark_members", None, 8, P["group"], 3)
    for bad_nhits in (0, -1):
        refused("ctvae_adam_mark_members", P["hits"], bad_nhits, P["group"], 3)
    refused("ctvae_adam_mark_members", P["hits"], 8, None, 3)         # B > 0 without a group
    refused("ctvae_adam_mark_members", P["hits"], 8, P["group"], -1)
    torch.cuda.synchronize()
    for k, (base, view) in bufs.items():
        assert guards_intact(base, view) and same(host(view, np.int32), np.ascontiguousarray(arrays[k]).view(np.int32)), f"{k} changed"
