"""GPU: csrc/graphstat.hip through its two entry points, against the float64 numpy restatements of tests/graph_checks.py.
ctvae_graph_accumulate: float32 -> float64 is exact and the float64 adds run in a fixed order, so every accumulator must equal
the restatement BIT FOR BIT -- there is no tolerance.  ctvae_heatmap_u8: the inputs keep every value away from a rounding
boundary of the table index (asserted by the restatement), so the whole byte stream must be equal."""
import numpy as np
import pytest
import torch

from tests import graph_checks as C

pytestmark = pytest.mark.gpu

FILL = 0xAA


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import native
    native.load()
    return native


class _Dev:
    """The six accumulators as device tensors; ``add`` is one launch."""

    def __init__(self, native, G, S, threshold=0.5):
        self.native, self.G, self.S, self.thr = native, G, S, threshold
        self.t = {k: torch.from_numpy(v).cuda() for k, v in C.new_state(G, S).items()}

    def add(self, adj, group, mask=None):
        a = torch.from_numpy(np.ascontiguousarray(adj)).cuda()
        g = torch.from_numpy(np.ascontiguousarray(group, dtype=np.int32)).cuda()
        m = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask)).cuda()
        t = self.t
        self.native.call("ctvae_graph_accumulate", a.data_ptr(), g.data_ptr(), self.native.ptr(m), self.thr, a.size(0), self.S, self.G,
                         t["adj_sum"].data_ptr(), t["edge_count"].data_ptr(), t["mask_sum"].data_ptr(), t["rows"].data_ptr(),
                         t["mask_rows"].data_ptr(), t["skipped"].data_ptr())
        return self

    def host(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def _same(got, want, what=""):
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        # bit equality: array_equal on the raw words also tells -0.0 from 0.0 and would tell NaN payloads apart
        assert np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)), \
            (what, k, int((got[k] != want[k]).sum()), float(np.abs(got[k].astype(np.float64) - want[k]).max()))


def _groups_7():
    """B = 7 rows over G = 13 groups: groups 4 and 9 (and others) absent, one row at -1 and one at G."""
    return np.array([3, 12, -1, 0, 3, 13, 7], dtype=np.int32)


CASES = {                                            # (B, S, G, groups or None = seeded)
    "one element": (1, 1, 1, None),
    "3x3 grid, less than a wave": (5, 9, 3, None),
    "64 nodes, absent groups and skipped rows": (7, 64, 13, _groups_7()),
    "256 nodes": (3, 256, 2, None),
    "64 nodes, every row in one group": (16, 64, 5, np.full(16, 2, dtype=np.int32)),
    "more rows than one pass of 256": (300, 5, 4, None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_accumulate_equals_the_restatement_exactly(native, name):
    B, S, G, groups = CASES[name]
    adj, group, mask = C.accumulate_inputs(len(name), B, S, G, groups=groups)
    want = C.ref_accumulate(C.new_state(G, S), adj, group, mask)
    got = _Dev(native, G, S).add(adj, group, mask).host()
    print(name, "rows", got["rows"].tolist(), "skipped", got["skipped"].tolist(), "edges", int(got["edge_count"].sum()))
    _same(got, want, name)
    assert want["rows"].sum() + want["skipped"][0] == B
    if groups is not None and S == 64 and G == 13:
        assert want["skipped"][0] == 2 and want["rows"][4] == 0 and want["rows"][9] == 0 and want["rows"][3] == 2
    if name.startswith("64 nodes, every row"):
        assert want["rows"].tolist() == [0, 0, 16, 0, 0]


def test_accumulate_does_not_depend_on_the_split_into_calls(native):
    """The (7, 64, 13) rows in one call and as 2 + 5 rows: bit-identical accumulators (and equal to the restatement)."""
    adj, group, mask = C.accumulate_inputs(41, 7, 64, 13, groups=_groups_7())
    one = _Dev(native, 13, 64).add(adj, group, mask).host()
    two = _Dev(native, 13, 64).add(adj[:2], group[:2], mask[:2]).add(adj[2:], group[2:], mask[2:]).host()
    _same(two, one, "2 + 5")
    _same(one, C.ref_accumulate(C.new_state(13, 64), adj, group, mask), "one call")
    # 300 rows of a small graph: 300 = 256 + 44 inside one call, against 7 calls of uneven size
    adj, group, mask = C.accumulate_inputs(42, 300, 5, 4)
    one = _Dev(native, 4, 5).add(adj, group, mask).host()
    many = _Dev(native, 4, 5)
    cuts = [0, 1, 3, 70, 71, 200, 299, 300]
    for a, b in zip(cuts[:-1], cuts[1:]):
        many.add(adj[a:b], group[a:b], mask[a:b])
    _same(many.host(), one, "7 calls")


def test_values_on_the_threshold_do_not_count(native):
    """adj > threshold is strict and compared in float32: 0.5 itself and the float32 just below do not count, the one just above
    does; NaN never counts.  Another threshold moves the count."""
    half = np.float32(0.5)
    vals = np.array([half, np.nextafter(half, np.float32(0)), np.nextafter(half, np.float32(1)), np.float32("nan"), 0.0, 1.0,
                     np.float32("inf"), -1.0, 0.25], dtype=np.float32)
    adj = np.tile(vals.reshape(1, 3, 3), (4, 1, 1))
    got = _Dev(native, 1, 3).add(adj, np.zeros(4, np.int32)).host()
    assert got["edge_count"][0].tolist() == [[0, 0, 4], [0, 0, 4], [4, 0, 0]]
    _same({k: got[k] for k in ("edge_count", "rows")}, C.ref_accumulate(C.new_state(1, 3), adj), "threshold 0.5")
    low = _Dev(native, 1, 3, threshold=0.25).add(adj, np.zeros(4, np.int32)).host()
    assert low["edge_count"][0].tolist() == [[4, 4, 4], [0, 0, 4], [4, 0, 0]]


def test_a_call_without_a_mask_leaves_the_mask_words_alone(native):
    adj, group, mask = C.accumulate_inputs(43, 6, 9, 3)
    dev = _Dev(native, 3, 9).add(adj, group, mask)
    first = dev.host()
    both = dev.add(adj, group, None).host()
    assert np.array_equal(both["mask_sum"], first["mask_sum"]) and np.array_equal(both["mask_rows"], first["mask_rows"])
    assert np.array_equal(both["rows"], 2 * first["rows"]) and first["mask_sum"].any()
    want = C.ref_accumulate(C.ref_accumulate(C.new_state(3, 9), adj, group, mask), adj, group, None)
    _same(both, want, "mask, then none")


def test_the_same_call_twice_gives_the_same_bits(native):
    adj, group, mask = C.accumulate_inputs(44, 16, 64, 5)
    start = C.ref_accumulate(C.new_state(5, 64), *C.accumulate_inputs(45, 4, 64, 5))       # a start that is not zero
    runs = []
    for _ in range(2):
        dev = _Dev(native, 5, 64)
        for k, v in start.items():
            dev.t[k].copy_(torch.from_numpy(v))
        runs.append(dev.add(adj, group, mask).host())
    _same(runs[1], runs[0], "second run")
    _same(runs[0], C.ref_accumulate({k: v.copy() for k, v in start.items()}, adj, group, mask), "onto a start")


def test_accumulate_refuses_bad_arguments(native):
    dev = _Dev(native, 2, 4)
    adj, group, mask = C.accumulate_inputs(46, 3, 4, 2)
    t = dev.t
    a, g = torch.from_numpy(adj).cuda(), torch.from_numpy(group).cuda()
    ptrs = [t[k].data_ptr() for k in ("adj_sum", "edge_count", "mask_sum", "rows", "mask_rows", "skipped")]
    for B, S, G in ((-1, 4, 2), (3, 0, 2), (3, 4, 0), (3, 46341, 2), (3, 4, 65536)):
        with pytest.raises(RuntimeError, match="bad argument"):
            native.call("ctvae_graph_accumulate", a.data_ptr(), g.data_ptr(), None, 0.5, B, S, G, *ptrs)
    with pytest.raises(RuntimeError, match="bad argument"):
        native.call("ctvae_graph_accumulate", None, g.data_ptr(), None, 0.5, 3, 4, 2, *ptrs)
    native.call("ctvae_graph_accumulate", a.data_ptr(), g.data_ptr(), None, 0.5, 0, 4, 2, *ptrs)      # no rows: a no-op
    assert not any(v.any() for v in dev.host().values())


# ---- heat map ---------------------------------------------------------------------------------------------------------------

def _table(seed=0):
    """A table whose three channels are unrelated permutations: a swapped channel or a wrong index shows."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([rng.permutation(256) for _ in range(3)], axis=1).astype(np.uint8))


def _heat(native, values, table, lo, hi, cell, nrow, padding, pad_color, scanlines=True):
    from ctvae_amd import imagegrid
    M, H, W = values.shape
    _, _, Hg, Wg = imagegrid.grid_geometry(M, H * cell, W * cell, nrow, padding)
    pitch = (1 if scanlines else 0) + 3 * Wg
    total = Hg * pitch
    out = torch.full(((total + 3) // 4 * 4 + 64,), FILL, dtype=torch.uint8, device="cuda")
    v = torch.from_numpy(values).cuda()
    native.call("ctvae_heatmap_u8", v.data_ptr(), M, H, W, float(lo), float(hi), cell, nrow, padding, *[int(c) for c in pad_color],
                table.ctypes.data, int(scanlines), out.data_ptr(), (total + 3) // 4 * 4)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[total:] == FILL).all(), "bytes past the stream's length were written"
    return host[:total].reshape(Hg, pitch)


HEAT_CASES = [(1, 1, 1, 1, 8), (5, 3, 7, 3, 2), (13, 64, 64, 4, 7)]           # (M, H, W, cell, nrow)


@pytest.mark.parametrize("M,H,W,cell,nrow", HEAT_CASES)
def test_heatmap_bytes_equal_the_restatement(native, M, H, W, cell, nrow):
    """(1,1,1,1,8): the smallest sheet, all in the stream's last partial lane; (5,3,7,3,2): non-square tiles, an empty cell, a
    pitch that is no multiple of 4; (13,64,64,4,7): the sheet of thirteen 64-node graphs.  Values below lo, above hi and NaN,
    a range that is not [0, 1], a padding colour that is not black."""
    lo, hi, pad_color, padding = -0.25, 1.5, (200, 30, 90), 2
    values = C.heat_inputs(100 * M + cell, (M, H, W), lo=lo, hi=hi)
    if values.size >= 8:
        assert np.isnan(values).any() and (values < lo).any() and (values > hi).any()
    table = _table()
    for scan in (True, False):
        want = C.ref_heatmap_bytes(values, table, lo=lo, hi=hi, cell=cell, nrow=nrow, padding=padding, pad_color=pad_color,
                                   scanlines=scan)
        got = _heat(native, values, table, lo, hi, cell, nrow, padding, pad_color, scanlines=scan)
        assert got.shape == want.shape
        if scan and (M, H) == (5, 3):
            assert got.shape[1] % 4 != 0
        assert np.array_equal(got, want), (scan, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())


def test_heatmap_edge_values_and_library_entry(native):
    """NaN, -inf and everything below lo take entry 0, +inf and everything above hi entry 255; causalgraph.heatmap_u8 is the
    same call with the library's table."""
    from ctvae_amd import causalgraph
    inf = float("inf")
    values = np.array([[[float("nan"), -inf, -7.0, 0.0], [1.0, 7.0, inf, 0.4]]], dtype=np.float32)       # 0.4 -> 102.5
    table = causalgraph.colormap()
    want = C.ref_heatmap_bytes(values, table, cell=2, nrow=8, padding=1, pad_color=causalgraph.PAD_COLOR)
    idx = C.table_index(values)
    assert idx.tolist() == [[[0, 0, 0, 0], [255, 255, 255, 102]]]
    got = causalgraph.heatmap_u8(torch.from_numpy(values).cuda(), cell=2, nrow=8, padding=1, scanlines=True)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    plain = causalgraph.heatmap_u8(torch.from_numpy(values).cuda(), cell=2, nrow=8, padding=1)
    assert tuple(plain.shape) == (6, 10, 3) and np.array_equal(plain.cpu().numpy().reshape(6, 30), want[:, 1:])
    assert plain[1, 1].tolist() == [0, 0, 0] and plain[3, 1].tolist() == [255, 255, 255] and plain[0, 0].tolist() == [64, 64, 64]
    v = torch.from_numpy(values).cuda()
    out = torch.empty(1024, dtype=torch.uint8, device="cuda")
    for kw in (dict(M=0), dict(cell=0), dict(nrow=0), dict(padding=-1), dict(hi=0.0), dict(hi=float("nan")), dict(pad_r=256), dict(n=8)):
        a = dict(M=1, H=2, W=4, lo=0.0, hi=1.0, cell=2, nrow=8, padding=1, pad_r=0, n=1024)
        a.update(kw)
        with pytest.raises(RuntimeError, match="bad argument"):
            native.call("ctvae_heatmap_u8", v.data_ptr(), a["M"], a["H"], a["W"], a["lo"], a["hi"], a["cell"], a["nrow"], a["padding"],
                        a["pad_r"], 0, 0, table.ctypes.data, 1, out.data_ptr(), a["n"])


def test_graph_stats_is_the_kernel_behind_one_copy(native):
    """causalgraph.GraphStats over the same rows: result() divides the sums by the rows; groups without rows are NaN."""
    from ctvae_amd import causalgraph
    adj, group, mask = C.accumulate_inputs(47, 7, 64, 13, groups=_groups_7())
    stats = causalgraph.GraphStats(13, 64, "cuda")
    stats.update(torch.from_numpy(adj[:3]).cuda(), torch.from_numpy(group[:3]).cuda(), torch.from_numpy(mask[:3]).cuda())
    stats.update(torch.from_numpy(adj[3:]).cuda(), torch.from_numpy(group[3:]).cuda().long(), torch.from_numpy(mask[3:]).cuda().view(4, 64, 1))
    res = stats.result()
    want = C.ref_accumulate(C.new_state(13, 64), adj, group, mask)
    mean, freq, mk = C.result_of(want)
    for got, ref in ((res["adjacency_mean"], mean), (res["edge_freq"], freq), (res["mask_mean"], mk)):
        assert got.dtype == np.float64 and np.array_equal(got, ref, equal_nan=True)
    assert res["rows"].tolist() == want["rows"].tolist() and res["skipped"] == 2 and np.isnan(res["adjacency_mean"][4]).all()
    none = causalgraph.GraphStats(2, 3, "cuda")
    none.update(torch.from_numpy(adj[:2, :3, :3].copy()).cuda())                       # group None: all rows in group 0, no mask
    r = none.result()
    assert r["rows"].tolist() == [2, 0] and np.isnan(r["mask_mean"]).all() and np.isnan(r["adjacency_mean"][1]).all()
    assert np.array_equal(r["adjacency_mean"][0], (adj[0, :3, :3].astype(np.float64) + adj[1, :3, :3].astype(np.float64)) / 2.0)
    with pytest.raises(ValueError, match=r"\[B, 3, 3\]"):
        none.update(torch.zeros(2, 4, 4, device="cuda"))
