"""GPU: csrc/gmm.hip op by op -- ``ctvae_gmm_estep``, ``ctvae_gmm_mstep``, ``ctvae_gmm_sample`` through ``kernels.gmm_*`` -- against the
float64 restatement of tests/prior_checks.py, from SHARED STATE: the GPU runs ONE E step, or ONE M step, on the parameters the
restatement's loop held at iterations 0 and 3, so EM's sensitivity to the assignments is not mistaken for kernel error.

Bound.  The project's fp32 parity bound, 1e-4 relative to each tensor's largest magnitude, for w, mu, Sigma, r and ll.  For ll at
D = 256 the bound is four times the largest deviation measured on the MI355X over this file's own D = 256 cases (``LL_256``).
The inputs keep every covariance's condition number below 1e4, which is asserted on the CPU."""
import functools

import numpy as np
import pytest
import torch

from tests import prior_checks as PC

pytestmark = pytest.mark.gpu

BOUND = 1e-4                 # relative to the tensor's largest magnitude
LL_256_MEASURED = 3.88e-7    # the largest |ll - ll_ref| / max |ll_ref| seen over the D = 256 cases below on the MI355X
LL_256 = 4 * LL_256_MEASURED  # (1030, 256, 2) diag at iteration 0, max |ll| 776; the other D = 256 figures: 1.3e-7 .. 3.8e-7
REG = 1e-2                   # keeps the covariance of a component that owns a handful of rows well conditioned
EPS32 = float(np.finfo(np.float32).eps)
FILL = 0xAA
GUARD = 256
# every D of {1, 5, 10, 33, 128, 256} (one partial tile, one full 64-tile + 1... two tiles, four tiles), every N of {2, 67, 257, 1030}
# (a partial row tile; two 64-row tiles of the E step; 2 and 5 slabs of the M step, the last one partial), every K of
# {1, 2, 3, 10, 64}
CASES = [(2, 1, 1), (2, 5, 2), (67, 5, 2), (67, 10, 3), (257, 10, 3), (257, 33, 10), (1030, 33, 10), (1030, 10, 64), (1030, 128, 3),
         (257, 128, 1), (1030, 256, 2), (1030, 256, 1)]
COVS = ("full", "diag")


@pytest.fixture(scope="module")
def Kn():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from ctvae_amd import kernels, native
    native.load()
    return kernels


@functools.lru_cache(maxsize=None)
def _case(N, D, K, cov):
    """(X fp32, states): the restatement's parameters at iterations 0 and 3 (computed once, shared, never written)."""
    X = PC.blobs(1000 + 7 * N + D + K, N, D, min(K, 4))
    init = PC.blob_start(X, K, 5 + N + D, cov, REG)
    info = PC.fit(X, init, cov, reg_covar=REG, max_iter=4, tol=0.0)[3]
    states = [info["states"][0], info["states"][3]]
    for w, mu, c in states:
        if cov == "full":
            assert max(np.linalg.cond(ck) for ck in c) < 1e4
        else:
            assert (c.max(axis=1) / c.min(axis=1)).max() < 1e4
    X.setflags(write=False)
    return X, states


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(dtype).cuda().contiguous()      # (a copy: the shared inputs are read-only)


def _params(w, mu, c, cov):
    L, P, ldh = PC.factor(c, cov)
    return dict(log_w=_dev(np.log(w)), mu=_dev(mu), P=_dev(P), log_det_half=_dev(ldh)), L


def _rel(a, ref):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def _estep(Kn, X, w, mu, c, cov):
    p, _ = _params(w, mu, c, cov)
    r, ll, bad = Kn.gmm_estep(_dev(X), p["log_w"], p["mu"], p["P"], p["log_det_half"], full=cov == "full")
    torch.cuda.synchronize()
    return r.cpu().numpy(), ll.cpu().numpy(), bad.cpu().numpy()


@pytest.mark.parametrize("cov", COVS)
@pytest.mark.parametrize("N,D,K", CASES)
def test_estep_against_restatement(Kn, N, D, K, cov):
    X, states = _case(N, D, K, cov)
    for it, (w, mu, c) in zip((0, 3), states):
        r, ll, bad = _estep(Kn, X, w, mu, c, cov)
        r_ref, ll_ref, bad_ref = PC.estep(X, w, mu, c, cov)
        e_r, e_ll = _rel(r, r_ref), _rel(ll, ll_ref)
        print(f"estep N={N} D={D} K={K} {cov} it={it}: r {e_r:.2e} ll {e_ll:.2e} (max |ll| {np.abs(ll_ref).max():.1f})")
        assert np.array_equal(bad, bad_ref) and not bad.any()
        assert e_r <= BOUND
        assert e_ll <= (LL_256 if D == 256 else BOUND)
        assert np.abs(r.astype(np.float64).sum(axis=1) - 1.0).max() <= 4 * EPS32 * K


@pytest.mark.parametrize("cov", COVS)
@pytest.mark.parametrize("N,D,K", CASES)
def test_mstep_against_restatement(Kn, N, D, K, cov):
    from ctvae_amd.latentprior import finish_mstep
    X, states = _case(N, D, K, cov)
    for it, (w, mu, c) in zip((0, 3), states):
        r32 = PC.estep(X, w, mu, c, cov)[0].astype(np.float32)
        bad = np.zeros(N, dtype=np.int32)
        m32 = mu.astype(np.float32)
        Nk, S1, S2 = Kn.gmm_mstep(_dev(X), _dev(r32), _dev(bad, torch.int32), _dev(m32), full=cov == "full")
        torch.cuda.synchronize()
        got = [t.numpy() for t in finish_mstep(Nk, S1, S2, m32.astype(np.float64), cov == "full", REG)]
        ref = PC.mstep(X, r32, bad, mu, cov, REG)
        errs = [_rel(g, f) for g, f in zip(got, ref)]
        print(f"mstep N={N} D={D} K={K} {cov} it={it} slabs={Kn.gmm_mstep_slabs(N, D, K, cov == 'full')}: "
              f"w {errs[0]:.2e} mu {errs[1]:.2e} Sigma {errs[2]:.2e}")
        assert max(errs) <= BOUND
        assert _rel(Nk.cpu().numpy(), r32.astype(np.float64).sum(axis=0)) <= 1e-12      # float64 throughout
        if cov == "full":
            s2 = S2.cpu().numpy()
            assert np.array_equal(s2, np.swapaxes(s2, 1, 2))                             # the mirror is a copy


def test_more_than_one_slab_is_merged(Kn):
    assert Kn.gmm_mstep_slabs(257, 10, 3, True) == 2 and Kn.gmm_mstep_slabs(1030, 33, 10, True) == 5
    assert Kn.gmm_mstep_slabs(2, 1, 1, False) == 1 and Kn.gmm_mstep_slabs(1030, 10, 64, False) == 5


@pytest.mark.parametrize("cov", COVS)
def test_far_component_takes_the_ten_eps_path(Kn, cov):
    from ctvae_amd.latentprior import finish_mstep
    N, D, K = 257, 10, 3
    X, states = _case(N, D, K, cov)
    w, mu, c = states[1]
    mu = mu.copy()
    mu[2] += 1e3                                                       # no row is anywhere near component 2
    r, ll, bad = _estep(Kn, X, w, mu, c, cov)
    r_ref, ll_ref, _ = PC.estep(X, w, mu, c, cov)
    assert (r[:, 2] == 0).all() and r_ref[:, 2].max() < 1e-300
    assert _rel(r, r_ref) <= BOUND and _rel(ll, ll_ref) <= BOUND
    m32 = mu.astype(np.float32)
    Nk, S1, S2 = Kn.gmm_mstep(_dev(X), _dev(r), _dev(bad, torch.int32), _dev(m32), full=cov == "full")
    assert float(Nk[2]) == 0.0
    got = [t.numpy() for t in finish_mstep(Nk, S1, S2, m32.astype(np.float64), cov == "full", REG)]
    ref = PC.mstep(X, r, bad, mu, cov, REG)
    assert all(np.isfinite(g).all() for g in got)
    assert 0 < got[0][2] < 1e-15                                       # 10 eps / N
    assert max(_rel(g, f) for g, f in zip(got, ref)) <= BOUND
    assert np.allclose(got[1][2], m32[2]) and np.allclose(got[2][2], REG * (np.eye(D) if cov == "full" else np.ones(D)))


@pytest.mark.parametrize("cov", COVS)
def test_nonfinite_rows_are_flagged_and_left_out(Kn, cov):
    from ctvae_amd.latentprior import finish_mstep
    N, D, K = 257, 33, 10
    X0, states = _case(N, D, K, cov)
    w, mu, c = states[1]
    X = X0.copy()
    X[5, 32] = np.nan
    X[70, 0] = np.inf
    X[256, 7] = -np.inf
    r, ll, bad = _estep(Kn, X, w, mu, c, cov)
    r_ref, ll_ref, bad_ref = PC.estep(X, w, mu, c, cov)
    assert np.array_equal(bad, bad_ref) and bad.sum() == 3 and list(np.nonzero(bad)[0]) == [5, 70, 256]
    assert (r[bad == 1] == 0).all() and (ll[bad == 1] == 0).all() and np.isfinite(r).all() and np.isfinite(ll).all()
    assert _rel(r, r_ref) <= BOUND and _rel(ll, ll_ref) <= BOUND
    m32 = mu.astype(np.float32)
    Nk, S1, S2 = Kn.gmm_mstep(_dev(X), _dev(r), _dev(bad, torch.int32), _dev(m32), full=cov == "full")
    assert abs(float(Nk.sum()) - (N - 3)) <= 4 * EPS32 * K * N         # N_finite
    got = [t.numpy() for t in finish_mstep(Nk, S1, S2, m32.astype(np.float64), cov == "full", REG)]
    ref = PC.mstep(X, r, bad, mu, cov, REG)
    assert all(np.isfinite(g).all() for g in got)
    assert max(_rel(g, f) for g, f in zip(got, ref)) <= BOUND


@pytest.mark.parametrize("cov", COVS)
def test_two_runs_are_bit_identical(Kn, cov):
    N, D, K = 1030, 33, 10
    X, states = _case(N, D, K, cov)
    w, mu, c = states[1]
    p, _ = _params(w, mu, c, cov)
    Xd = _dev(X)
    runs = []
    for _ in range(2):
        r, ll, bad = Kn.gmm_estep(Xd, p["log_w"], p["mu"], p["P"], p["log_det_half"], full=cov == "full")
        sums = Kn.gmm_mstep(Xd, r, bad, p["mu"], full=cov == "full")
        torch.cuda.synchronize()
        runs.append([t.cpu().numpy() for t in (r, ll, bad) + tuple(sums)])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("cov", COVS)
def test_outputs_stay_inside_their_buffers(Kn, cov):
    """Raw entry points with every output carved out of one 0xAA-filled buffer, at sizes that are no multiple of any tile."""
    from ctvae_amd import native
    N, D, K = 67, 33, 10
    full = cov == "full"
    X, states = _case(257, D, K, cov)
    X = X[:N]
    w, mu, c = states[1]
    p, L = _params(w, mu, c, cov)
    sizes = {"r": 4 * N * K, "ll": 4 * N, "bad": 4 * N, "Nk": 8 * K, "S1": 8 * K * D, "S2": 8 * K * D * (D if full else 1),
             "z": 4 * N * D, "comp": 4 * N}
    off, offs = GUARD, {}
    for k, n in sizes.items():
        offs[k] = off
        off += (n + 255) // 256 * 256 + GUARD
    buf = torch.full((off,), FILL, dtype=torch.uint8, device="cuda")
    ptr = lambda k: buf.data_ptr() + offs[k]
    Xd = _dev(X)
    native.call("ctvae_gmm_estep", Xd.data_ptr(), N, D, K, int(full), p["log_w"].data_ptr(), p["mu"].data_ptr(), p["P"].data_ptr(),
                p["log_det_half"].data_ptr(), ptr("r"), ptr("ll"), ptr("bad"))
    nbytes = int(native.load().ctvae_gmm_mstep_workspace_bytes(N, D, K, int(full)))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    native.call("ctvae_gmm_mstep", Xd.data_ptr(), ptr("r"), ptr("bad"), N, D, K, int(full), p["mu"].data_ptr(), ptr("Nk"), ptr("S1"),
                ptr("S2"), ws.data_ptr(), nbytes)
    rng = np.random.default_rng(3)
    u, eps = _dev(rng.random(N)), _dev(rng.normal(size=(N, D)))
    cdf = _dev(np.cumsum(w), torch.float64)
    native.call("ctvae_gmm_sample", u.data_ptr(), eps.data_ptr(), N, D, K, int(full), cdf.data_ptr(), p["mu"].data_ptr(),
                _dev(L).data_ptr(), ptr("z"), ptr("comp"))
    torch.cuda.synchronize()
    raw = buf.cpu().numpy()
    mask = np.ones(raw.size, bool)
    for k, n in sizes.items():
        mask[offs[k]:offs[k] + n] = False
    assert (raw[mask] == FILL).all(), "a byte outside the outputs was written"
    r = raw[offs["r"]:offs["r"] + sizes["r"]].view(np.float32).reshape(N, K)
    assert _rel(r, PC.estep(X, w, mu, c, cov)[0]) <= BOUND


def test_refusals(Kn):
    from ctvae_amd import native
    X = torch.zeros(4, 3, device="cuda")
    ok = dict(log_w=torch.zeros(2, device="cuda"), mu=torch.zeros(2, 3, device="cuda"), P=torch.ones(2, 3, device="cuda"),
              log_det_half=torch.zeros(2, device="cuda"))
    with pytest.raises(ValueError, match="N >= K"):                    # N < K
        Kn.gmm_mstep(torch.zeros(2, 3, device="cuda"), torch.zeros(2, 5, device="cuda"), None, torch.zeros(5, 3, device="cuda"), full=False)
    with pytest.raises(ValueError, match="D=0"):
        Kn.gmm_estep(torch.zeros(4, 0, device="cuda"), ok["log_w"], torch.zeros(2, 0, device="cuda"), torch.zeros(2, 0, device="cuda"),
                     ok["log_det_half"], full=False)
    with pytest.raises(ValueError, match="D=257"):
        Kn.gmm_estep(torch.zeros(4, 257, device="cuda"), ok["log_w"], torch.zeros(2, 257, device="cuda"),
                     torch.ones(2, 257, device="cuda"), ok["log_det_half"], full=False)
    with pytest.raises(ValueError, match="K=65"):
        Kn.gmm_estep(X, torch.zeros(65, device="cuda"), torch.zeros(65, 3, device="cuda"), torch.ones(65, 3, device="cuda"),
                     torch.zeros(65, device="cuda"), full=False)
    with pytest.raises(ValueError, match="P must be"):
        Kn.gmm_estep(X, ok["log_w"], ok["mu"], ok["P"], ok["log_det_half"], full=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Kn.gmm_estep(X.cpu(), *(t.cpu() for t in ok.values()), full=False)
    # the entry points themselves: -22 and nothing launched (the outputs keep their fill)
    out = torch.full((64,), 7.0, device="cuda")
    flags = torch.full((64,), 7, dtype=torch.int32, device="cuda")
    dsum = torch.full((64,), 7.0, dtype=torch.float64, device="cuda")
    for N, D, K in ((4, 0, 2), (4, 257, 2), (4, 3, 0), (4, 3, 65), (-1, 3, 2)):
        with pytest.raises(RuntimeError, match="bad argument"):
            native.call("ctvae_gmm_estep", X.data_ptr(), N, D, K, 0, ok["log_w"].data_ptr(), ok["mu"].data_ptr(), ok["P"].data_ptr(),
                        ok["log_det_half"].data_ptr(), out.data_ptr(), out.data_ptr(), flags.data_ptr())
    for N, D, K in ((1, 3, 2), (4, 0, 2), (4, 257, 2), (0, 3, 1)):     # N < K, D out of range, no row
        with pytest.raises(RuntimeError, match="bad argument"):
            native.call("ctvae_gmm_mstep", X.data_ptr(), out.data_ptr(), None, N, D, K, 0, ok["mu"].data_ptr(), dsum.data_ptr(),
                        dsum.data_ptr(), dsum.data_ptr(), dsum.data_ptr(), 64 * 8)
    with pytest.raises(RuntimeError, match="bad argument"):
        native.call("ctvae_gmm_sample", out.data_ptr(), out.data_ptr(), 4, 257, 2, 0, dsum.data_ptr(), ok["mu"].data_ptr(),
                    ok["P"].data_ptr(), out.data_ptr(), flags.data_ptr())
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (flags == 7).all() and (dsum == 7.0).all()


@pytest.mark.parametrize("cov", COVS)
@pytest.mark.parametrize("N,D,K", [(67, 5, 2), (257, 33, 10), (130, 256, 3), (64, 10, 64)])
def test_sample_against_restatement(Kn, N, D, K, cov):
    rng = np.random.default_rng(11 + D + K)
    X = PC.blobs(77 + D, max(4 * D, 8 * K), D, min(K, 4))
    w, mu, c = PC.blob_start(X, K, 9, cov, REG)
    w = rng.random(K) + 0.2
    w /= w.sum()
    cdf = np.cumsum(w)
    # u: around every cdf edge, 2e-6 to either side, and uniform draws moved off the edges; all as the fp32 the kernel reads
    edges = cdf[:-1]
    u = np.concatenate([edges - 2e-6, edges + 2e-6, [0.0, 1.0 - 2.0 ** -24], rng.random(N)]).astype(np.float32)
    u = np.clip(u, 0.0, 1.0 - 2.0 ** -24).astype(np.float32)
    close = np.abs(u.astype(np.float64)[:, None] - cdf[None, :]).min(axis=1) < 1e-6
    u = u[~close]
    assert np.abs(u.astype(np.float64)[:, None] - cdf[None, :]).min() >= 1e-6          # the test's own u stay off the edges
    n = len(u)
    eps = rng.normal(size=(n, D)).astype(np.float32)
    z_ref, k_ref = PC.sample(u, eps, w, mu, c, cov)
    L = PC.factor(c, cov)[0]
    z, k = Kn.gmm_sample(_dev(u), _dev(eps), _dev(cdf, torch.float64), _dev(mu), _dev(L), full=cov == "full")
    torch.cuda.synchronize()
    assert np.array_equal(k.cpu().numpy(), k_ref)
    assert len(np.unique(k_ref)) == K                              # every component is drawn
    L32 = L.astype(np.float32).astype(np.float64)
    mu32 = mu.astype(np.float32).astype(np.float64)
    z32 = mu32[k_ref] + (np.einsum("nij,nj->ni", L32[k_ref], eps.astype(np.float64)) if cov == "full" else L32[k_ref] * eps)
    e = _rel(z.cpu().numpy(), z_ref)
    print(f"sample n={n} D={D} K={K} {cov}: z {e:.2e}, against the fp32 parameters {_rel(z.cpu().numpy(), z32):.2e}")
    assert e <= BOUND
