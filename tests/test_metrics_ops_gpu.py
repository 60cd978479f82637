"""GPU: the three kernels of csrc/disent.hip, each against the float64 restatement of tests/metrics_checks.py (which also
asserts the input conditions: the edge margin of the binning, the gap of the arg-min).  Output buffers are pre-filled by the
wrappers' torch.empty only, so every comparison covers the whole output; bad arguments must return the bad-argument code
without a launch (seen through the library's launch log)."""
import numpy as np
import pytest
import torch

from tests import metrics_checks as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import metrics, native
    native.load()
    return metrics


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()          # a writable copy: the cached inputs are read-only


def _rel(got, want):
    """max |got - want| / |want| over the entries with want != 0; entries with want == 0 must be exactly 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    zero = want == 0
    assert (got[zero] == 0).all()
    return float((np.abs(got - want)[~zero] / np.abs(want[~zero])).max()) if (~zero).any() else 0.0


@pytest.mark.parametrize("N,L", C.MOMENT_SHAPES)
def test_column_moments(M, N, L):
    """min / max bit-equal; mean / var within 1e-5 relative (Welford mean over <= 128 values per slice, pairwise merge, second
    pass for the variance: a few sqrt(N) * 2^-24); the last column is constant: var exactly 0, mean exactly the value."""
    z = C.moment_inputs(N, L)
    mean, var, lo, hi = C.ref_moments(z)
    g_mean, g_var, g_lo, g_hi = (t.cpu().numpy() for t in M.column_moments(_dev(z)))
    assert np.array_equal(g_lo.view(np.uint32), lo.view(np.uint32)) and np.array_equal(g_hi.view(np.uint32), hi.view(np.uint32))
    e_mean, e_var = _rel(g_mean, mean), _rel(g_var, var)
    print(f"column_moments N={N} L={L}: rel err mean {e_mean:.2e} var {e_var:.2e}")
    assert var[L - 1] == 0 and g_var[L - 1] == 0 and g_mean[L - 1] == z[0, L - 1]
    assert e_mean <= 1e-5 and e_var <= 1e-5


@pytest.mark.parametrize("N,L", C.MI_SHAPES)
def test_mi_matrix(M, N, L):
    """bins equal the restatement's (every value keeps 1e-3 bin widths from every edge, asserted there); mi within 2e-5
    absolute: counts are integers, the float32 error is a few ulp of logf times sum |terms| <= 2 log(20 * 183) ~ 16."""
    z, lo, hi, factors, bins, mi = C.mi_inputs(N, L)
    g_mi, g_bins = M.mi_matrix(_dev(z), _dev(lo), _dev(hi), _dev(factors), C.MI_SIZES, want_bins=True)
    assert np.array_equal(g_bins.cpu().numpy(), bins)
    err = float(np.abs(g_mi.cpu().numpy().astype(np.float64) - mi).max())
    print(f"mi_matrix N={N} L={L}: max abs err {err:.2e} (max mi {mi.max():.3f})")
    assert err <= 2e-5
    g2 = M.mi_matrix(_dev(z), _dev(lo), _dev(hi), _dev(factors), C.MI_SIZES)          # bins == NULL: the same numbers
    assert torch.equal(g2, g_mi)


def test_mi_matrix_small_factor_sizes_take_four_waves(M):
    """sizes <= 128 run four tables per workgroup instead of two (the launcher's other configuration); 16 factors."""
    N, L = 100, 37
    rng = np.random.default_rng(5)
    sizes = tuple(int(s) for s in rng.integers(2, 129, 16))
    z, lo, hi, _, bins, _ = C.mi_inputs(N, L, (2, 3))
    factors = np.stack([rng.integers(0, s, N) for s in sizes], axis=1).astype(np.int32)
    mi = C.ref_mi(bins, factors, sizes)
    g_mi, g_bins = M.mi_matrix(_dev(z), _dev(lo), _dev(hi), _dev(factors), sizes, want_bins=True)
    assert np.array_equal(g_bins.cpu().numpy(), bins)
    assert float(np.abs(g_mi.cpu().numpy().astype(np.float64) - mi).max()) <= 2e-5


@pytest.mark.parametrize("G,B,L", C.ARGMIN_SHAPES)
def test_group_var_argmin(M, G, B, L):
    """Indices equal (the restatement asserts a relative gap >= 1e-3 between the two smallest ratios of every group); the
    ratio within 1e-5 relative.  Columns 0, L-1 and a random fifth are inactive."""
    z, gvar, active, arg, val = C.argmin_inputs(G, B, L)
    g_arg, g_val = M.group_var_argmin(_dev(z), _dev(gvar), _dev(active))
    assert np.array_equal(g_arg.cpu().numpy().astype(np.int64), arg)
    err = _rel(g_val.cpu().numpy(), val)
    print(f"group_var_argmin G={G} B={B} L={L}: rel err {err:.2e}")
    assert err <= 1e-5


def test_group_var_argmin_tie_goes_to_the_lower_index(M):
    """Two identical columns (same values, same global variance) hold the smallest ratio: the lower index wins, on either
    side of a wave and of the 256-column stride; with no active column the answer is -1 / inf."""
    z, gvar, active, _, _ = C.argmin_inputs(7, 16, 130)
    for a, b in ((5, 6), (3, 70), (100, 17)):
        z2, gv2, act2 = z.copy(), gvar.copy(), active.copy()
        z2[:, :, a] = z2[:, :, b] = 1e-3 * z[:, :, 9]
        gv2[a] = gv2[b] = 1.0
        act2[a] = act2[b] = 1
        want, _ = C.ref_group_argmin(z2, gv2, act2, gap=None)
        assert (want == min(a, b)).all()
        g_arg, _ = M.group_var_argmin(_dev(z2), _dev(gv2), _dev(act2))
        assert (g_arg.cpu().numpy() == min(a, b)).all(), (a, b)
    g_arg, g_val = M.group_var_argmin(_dev(z), _dev(gvar), _dev(np.zeros_like(active)))
    assert (g_arg.cpu().numpy() == -1).all() and torch.isinf(g_val).all()


def test_bad_arguments_return_the_error_code_and_launch_nothing(M):
    from ctvae_amd import native
    lib = native.load()
    dev = torch.device("cuda")
    buf = torch.zeros(4096, dtype=torch.float32, device=dev)
    ints = torch.zeros(4096, dtype=torch.int32, device=dev)
    p, ip, st = buf.data_ptr(), ints.data_ptr(), native.stream_ptr()
    ok_sizes = np.array([2, 15, 183], dtype=np.int32)
    bad_sizes = np.array([2, 300, 183], dtype=np.int32)
    native.prof_report()
    native.prof_enable(True)
    try:
        codes = {
            "moments L=0": lib.ctvae_column_moments(p, 8, 0, p, p, p, p, st),
            "moments N=1": lib.ctvae_column_moments(p, 1, 8, p, p, p, p, st),
            "mi L=0": lib.ctvae_mi_matrix(p, p, p, ip, ok_sizes.ctypes.data, 8, 0, 3, p, None, st),
            "mi size 300": lib.ctvae_mi_matrix(p, p, p, ip, bad_sizes.ctypes.data, 8, 8, 3, p, None, st),
            "mi F=17": lib.ctvae_mi_matrix(p, p, p, ip, ok_sizes.ctypes.data, 8, 8, 17, p, None, st),
            "mi N=65536": lib.ctvae_mi_matrix(p, p, p, ip, ok_sizes.ctypes.data, 65536, 8, 3, p, None, st),
            "argmin B=1": lib.ctvae_group_var_argmin(p, p, ip, 4, 1, 8, ip, p, st),
            "argmin L=0": lib.ctvae_group_var_argmin(p, p, ip, 4, 4, 0, ip, p, st),
            "argmin L=16385": lib.ctvae_group_var_argmin(p, p, ip, 4, 4, 16385, ip, p, st),
        }
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    assert all(c == -22 for c in codes.values()), codes
    assert native.prof_report() == {}
    with pytest.raises(RuntimeError, match="bad argument"):
        M.column_moments(torch.zeros(1, 8, device=dev))
