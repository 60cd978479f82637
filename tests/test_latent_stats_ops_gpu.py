"""GPU: csrc/latentstat.hip through ``ctvae_latent_accumulate`` and ``kernels.latent_accumulate``, against the float64 numpy
restatement of tests/latent_checks.py.  float32 -> float64 and the product of two float32 values are exact and the float64 adds
run in a fixed order, so ``mu_sum``, ``cov_sum``, ``nonfinite`` and ``rows`` must equal the restatement BIT FOR BIT; ``kl_sum``
and ``sig2_sum`` go through two implementations of the double ``exp`` and must lie within ``latent_checks.kl_bound``, which is
derived from the formats (a dropped or doubled row or an fp32 exp is eight orders of magnitude above it)."""
import numpy as np
import pytest
import torch

from tests import latent_checks as C

pytestmark = pytest.mark.gpu

FILL = 0xAA
GUARD = 64            # bytes in front of, between and behind the accumulators
EXACT = ("mu_sum", "cov_sum", "nonfinite", "rows")
# the issue's shapes, and (3, 300).  The kernel's boundaries: cov_sum tiles of 16 x 16 -- L = 3, 10 (inside one), 16 (one,
# full), 17 (one column over), 130 (8 tiles + 2), 300, 1024; workgroups of 32 columns of the [L] vectors -- L = 17 (inside one),
# 128 (4, full), 130 (4 + 2 columns), 300 (9 + 12); 64 rows of mu staged per turn -- B = 64 (one, full), 65, 257; 32 rows of
# terms per turn -- B = 33, 65, 257
SHAPES = [(1, 1), (7, 3), (5, 10), (33, 16), (64, 128), (65, 130), (257, 17), (2, 1024), (3, 300)]


@pytest.fixture(scope="module")
def native():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import native
    native.load()
    return native


class _Dev:
    """The six accumulators carved out of one byte buffer filled with 0xAA, ``GUARD`` bytes around each; ``add`` is one launch."""

    def __init__(self, native, L):
        self.native, self.L = native, L
        sizes = {"kl_sum": 8 * L, "mu_sum": 8 * L, "sig2_sum": 8 * L, "cov_sum": 8 * L * L, "nonfinite": 4 * L, "rows": 4}
        off, self.off = GUARD, {}
        for k in C.KEYS:
            self.off[k] = (off, sizes[k])
            off += sizes[k] + GUARD
        self.buf = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 8 == 0
        for k, (o, n) in self.off.items():
            self.buf[o:o + n] = 0
        self.keep = []

    def ptr(self, k):
        return self.buf.data_ptr() + self.off[k][0]

    def call(self, mu_ptr, pm, lv_ptr, pv, B, L, ptrs=None):
        ptrs = [self.ptr(k) for k in C.KEYS] if ptrs is None else ptrs
        self.native.call("ctvae_latent_accumulate", mu_ptr, pm, lv_ptr, pv, B, L, *ptrs)

    def add(self, mu, lv):
        m, v = torch.from_numpy(np.ascontiguousarray(mu)).cuda(), torch.from_numpy(np.ascontiguousarray(lv)).cuda()
        self.keep += [m, v]
        self.call(m.data_ptr(), self.L, v.data_ptr(), self.L, m.size(0), self.L)
        return self

    def host(self):
        torch.cuda.synchronize()
        raw = self.buf.cpu().numpy()
        mask = np.ones(raw.size, bool)
        out, ref = {}, C.new_state(self.L)
        for k, (o, n) in self.off.items():
            out[k] = raw[o:o + n].copy().view(ref[k].dtype).reshape(ref[k].shape)
            mask[o:o + n] = False
        assert (raw[mask] == FILL).all(), "a guard byte around the accumulators was written"
        return out


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _same(got, want, what="", keys=C.KEYS):
    for k in keys:
        assert _bits_equal(got[k], want[k]), (what, k, float(np.nanmax(np.abs(got[k].astype(np.float64) - want[k]))))


def _check(got, want, mu, lv, what=""):
    _same(got, want, what, EXACT)
    assert np.array_equal(got["cov_sum"], got["cov_sum"].T), what
    bound = C.kl_bound(mu, lv)
    for k in ("kl_sum", "sig2_sum"):
        err = np.abs(got[k] - want[k])
        print(what, k, "max err", float(err.max()), "bound at it", float(bound[err.argmax()]))
        assert (err <= bound).all(), (what, k, float(err.max()), float(bound.min()))


@pytest.mark.parametrize("B,L", SHAPES)
def test_accumulate_equals_the_restatement(native, B, L):
    const = L // 2
    mu, lv = C.inputs(1000 * B + L, B, L, constant_col=const)
    want = C.ref_accumulate(C.new_state(L), mu, lv)
    got = _Dev(native, L).add(mu, lv).host()
    _check(got, want, mu, lv, f"({B}, {L})")
    assert got["rows"].tolist() == [B] and not got["nonfinite"].any()
    # the constant column (mu = 0, logvar = 0): exact zeros, sigma^2 exactly 1 per row
    assert got["kl_sum"][const] == 0.0 and got["mu_sum"][const] == 0.0 and got["sig2_sum"][const] == float(B)
    assert not got["cov_sum"][const].any() and not got["cov_sum"][:, const].any()
    # a second batch onto the first: the stored value is where the adds start
    mu2, lv2 = C.inputs(77 + B + L, max(B // 2, 1), L)
    both = _Dev(native, L).add(mu, lv).add(mu2, lv2).host()
    _check(both, C.ref_accumulate(want, mu2, lv2), np.concatenate([mu, mu2]), np.concatenate([lv, lv2]), f"({B}, {L}) + second")


def test_accumulate_does_not_depend_on_the_split_into_calls(native):
    """37 rows in one call and as 5 + 32 rows: all six accumulators bit-identical -- kl_sum and sig2_sum too, the device's exp
    being the same function in both."""
    L = 40
    mu, lv = C.inputs(41, 37, L, constant_col=3)
    one = _Dev(native, L).add(mu, lv).host()
    two = _Dev(native, L).add(mu[:5], lv[:5]).add(mu[5:], lv[5:]).host()
    _same(two, one, "5 + 32")
    _check(one, C.ref_accumulate(C.new_state(L), mu, lv), mu, lv, "one call")
    mu, lv = C.inputs(42, 150, 5)                    # across the row chunk of 64: one call against seven uneven ones
    one = _Dev(native, 5).add(mu, lv).host()
    many = _Dev(native, 5)
    cuts = [0, 1, 3, 64, 65, 128, 149, 150]
    for a, b in zip(cuts[:-1], cuts[1:]):
        many.add(mu[a:b], lv[a:b])
    _same(many.host(), one, "7 calls")


def test_pitched_inputs_equal_the_contiguous_result(native):
    """The two column halves of one [B, 2L] heads tensor through the raw entry point and through the wrapper (no copy), and a
    slice of a stride-0 expanded [B, S, L] view through the wrapper: the accumulators of the contiguous call, bit for bit."""
    from ctvae_amd import kernels as K
    B, L = 19, 24
    mu, lv = C.inputs(51, B, L, constant_col=0)
    want = _Dev(native, L).add(mu, lv).host()
    heads = torch.from_numpy(np.concatenate([mu, lv], axis=1)).cuda()
    dev = _Dev(native, L)
    dev.call(heads.data_ptr(), 2 * L, heads.data_ptr() + 4 * L, 2 * L, B, L)
    _same(dev.host(), want, "halves, raw")

    def wrapped(m, v):
        st = {k: torch.from_numpy(a).cuda() for k, a in C.new_state(L).items()}
        K.latent_accumulate(m, v, st)
        torch.cuda.synchronize()
        return {k: t.cpu().numpy() for k, t in st.items()}

    _same(wrapped(heads[:, :L], heads[:, L:]), want, "halves, wrapper")
    m3 = torch.from_numpy(mu).cuda().view(B, 1, L).expand(B, 5, L)
    v3 = torch.from_numpy(lv).cuda().view(B, 1, L).expand(B, 5, L)
    assert m3.stride() == (L, 0, 1)
    _same(wrapped(m3[:, 0], v3[:, 0]), want, "expanded view")
    # rows that are closer together than L floats (a row expanded over the batch), and strided columns: copied, same numbers
    row = torch.from_numpy(mu[:1]).cuda().expand(B, L)
    assert row.stride() == (0, 1)
    rep = wrapped(row, torch.from_numpy(lv).cuda())
    _same(rep, _Dev(native, L).add(np.repeat(mu[:1], B, axis=0), lv).host(), "stride-0 rows")
    t = torch.from_numpy(np.ascontiguousarray(mu.T)).cuda().t()
    assert t.stride() == (1, B)
    _same(wrapped(t, torch.from_numpy(lv).cuda()), want, "transposed")


def test_no_rows_change_nothing_and_bad_arguments_are_refused(native):
    L = 6
    mu, lv = C.inputs(61, 4, L)
    dev = _Dev(native, L).add(mu, lv)
    before = dev.host()
    m, v = torch.from_numpy(mu).cuda(), torch.from_numpy(lv).cuda()
    dev.call(m.data_ptr(), L, v.data_ptr(), L, 0, L)                                  # B = 0: a successful no-op
    _same(dev.host(), before, "B = 0")
    ptrs = [dev.ptr(k) for k in C.KEYS]
    for B, Lb, pm, pv in ((-1, L, L, L), (4, 0, L, L), (4, 1025, 1025, 1025), (4, L, L - 1, L), (4, L, L, L - 1), (4, L, 0, L)):
        with pytest.raises(RuntimeError, match=r"bad argument.*-22"):
            dev.call(m.data_ptr(), pm, v.data_ptr(), pv, B, Lb)
    for i in range(6):
        with pytest.raises(RuntimeError, match=r"bad argument.*-22"):
            dev.call(m.data_ptr(), L, v.data_ptr(), L, 4, L, ptrs[:i] + [None] + ptrs[i + 1:])
    for mp, vp in ((None, v.data_ptr()), (m.data_ptr(), None)):
        with pytest.raises(RuntimeError, match=r"bad argument.*-22"):
            dev.call(mp, L, vp, L, 4, L)
    _same(dev.host(), before, "after the refusals")                                   # none of them launched anything


def test_nonfinite_values_are_counted_in_their_columns(native):
    B, L = 9, 35
    mu, lv = C.inputs(71, B, L)
    mu[2, 4] = np.nan
    lv[5, 4] = np.inf
    lv[7, 33] = -np.inf
    mu[8, 33], lv[8, 33] = np.inf, np.nan                       # one element, both parameters: counted once
    want = C.ref_accumulate(C.new_state(L), mu, lv)
    got = _Dev(native, L).add(mu, lv).host()
    expect = np.zeros(L, np.int32)
    expect[4], expect[33] = 2, 2
    assert got["nonfinite"].tolist() == expect.tolist() == want["nonfinite"].tolist()
    # they still go into the sums: the columns are NaN / inf as in the restatement, every other column is untouched
    for k in ("kl_sum", "mu_sum", "sig2_sum"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])) and np.array_equal(np.isinf(got[k]), np.isinf(want[k])), k
    assert np.isnan(got["mu_sum"][4]) and np.isnan(got["cov_sum"][4]).all() and np.isnan(got["cov_sum"][:, 4]).all()
    fine = np.ones(L, bool)
    fine[[4, 33]] = False
    sub = lambda s: {"mu_sum": s["mu_sum"][fine], "cov_sum": np.ascontiguousarray(s["cov_sum"][np.ix_(fine, fine)])}
    _same(sub(got), sub(want), "finite columns", ("mu_sum", "cov_sum"))
    bound = C.kl_bound(mu[:, fine], lv[:, fine])
    assert (np.abs(got["kl_sum"][fine] - want["kl_sum"][fine]) <= bound).all()


def test_latent_stats_is_the_kernel_behind_one_copy(native):
    """latentstats.LatentStats over the same rows in two batches: state() is the restatement, result() its summary."""
    from ctvae_amd import latentstats as S
    B, L = 48, 12
    mu, lv = C.inputs(81, B, L, constant_col=7)
    stats = S.LatentStats(L, "cuda")
    stats.zero()
    stats.observe(torch.from_numpy(mu[:20]).cuda(), torch.from_numpy(lv[:20]).cuda())
    stats.observe(torch.from_numpy(mu[20:]).cuda(), torch.from_numpy(lv[20:]).cuda())
    want = C.ref_accumulate(C.new_state(L), mu, lv)
    st = stats.state()
    _check(st, want, mu, lv, "LatentStats")
    res, ref = stats.result(), S.summarize(want)
    assert res["active_units"] == ref["active_units"] == L - 1 and res["collapsed"] == 1 and res["rows"] == B
    assert np.array_equal(res["cov"], ref["cov"]) and np.array_equal(res["mu_mean"], ref["mu_mean"])
    assert abs(res["kl_total"] - ref["kl_total"]) <= C.kl_bound(mu, lv).sum() / B
    stats.zero()
    assert stats.result() == {"rows": 0, "nonfinite": 0}
    with pytest.raises(ValueError, match=r"\[B, 12\]"):
        stats.observe(torch.zeros(2, 13, device="cuda"), torch.zeros(2, 13, device="cuda"))
