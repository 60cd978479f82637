"""GPU: the EMA-codebook kernels (csrc/vqema.hip) op by op against the float64 restatement of tests/vq_ema_checks.py.

Statistics (``ctvae_vq_ema_stats``): one case per dispatch path, shapes from ``vq_checks.BWD_CASES`` (the launcher dispatches as
``launch_vq_backward`` does), each with uniform and skewed indices.  Integer-valued latents make every sum exact in fp32, so those
checks are bitwise; random latents are held to the bound of a fixed-order fp32 sum, n_k * u * sum |x| per element.
Update (``ctvae_vq_ema_update``): K in {1, 37, 64, 512} x C in {1, 4, 8} x Dc in {5, 32, 128} against float64 on the same fp32
inputs, with the bounds of ``vq_ema_checks.update_bounds``."""
import pytest
import torch

from tests import vq_checks as V
from tests import vq_ema_checks as EC

pytestmark = pytest.mark.gpu

STAT_IDS = ["pos-P245", "pos-P5", "pos-P2053-S9", "pos-C8-Dc5-K100", "posw-Dc128-P75", "posw-Dc33-K73-C2", "scan1-K512-P512",
            "scan1-Dc256-K16", "scanS5-K200-Dc40-P2587"]
LABEL = {"pos": "vq_ema_stats_pos_kernel", "posw": "vq_ema_stats_posw_kernel", "scan1": "vq_ema_stats_scan_kernel",
         "scanS": "vq_ema_stats_scan_kernel"}
ALL_LABELS = set(LABEL.values()) | {"vq_ema_reduce_kernel", "vq_ema_update_kernel"}
KINDS = ("uniform", "skewed")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _native():
    from ctvae_amd import native
    return native


def logged(fn):
    """Run fn with the library's launch log on; returns (fn's result, {label: ...})."""
    native = _native()
    native.prof_report()
    native.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    return out, native.prof_report()


def _case(id):
    return V.case_of(V.BWD_CASES, id)


def _acc(dev, case, n_fill=0, s_fill=0.0):
    Dc = case.D // case.C
    return (torch.full((case.C, case.K), n_fill, dtype=torch.int64, device=dev),
            torch.full((case.C, case.K, Dc), s_fill, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))


def _launch(dev, case, x, inds, acc, poison_ws=False):
    from ctvae_amd import kernels as K
    if poison_ws:
        _native().workspace(dev).fill_(float("nan"))
    K.vq_ema_stats(x.to(dev).view(case.B, case.HW, case.D), inds.to(dev), *acc)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


# ---- statistics ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("id", STAT_IDS)
def test_stats_exact_inputs(dev, id, kind):
    """(a) integer latents: counts and sums bit-equal to the integer reference, unused codes exactly zero, the dispatch path is
    the case's; (c) a second launch into the same accumulators gives the statistics of the concatenated batch, which one launch
    over that batch gives too; (d) sentinels in the accumulators are added to and a NaN-filled workspace does not leak."""
    case = _case(id)
    x, _ = V.exact_inputs(case)
    inds = V.given_inds(case, kind)
    counts, sums, _, invalid = EC.stats64(x, inds, case.K)
    assert invalid == 0 and int(counts.sum()) == case.B * case.HW * case.C and float(sums.abs().max()) < 2 ** 24
    if kind == "skewed" and case.K > 3:
        assert int((counts == 0).sum()) >= case.C * (case.K - 3)          # most codes unused
    acc = _acc(dev, case)
    _, log = logged(lambda: _launch(dev, case, x, inds, acc, poison_ws=True))
    assert log[LABEL[case.path]]["count"] == 1 and log["vq_ema_reduce_kernel"]["count"] == 1
    assert set(log) & ALL_LABELS == {LABEL[case.path], "vq_ema_reduce_kernel"}
    assert torch.equal(acc[0].cpu(), counts) and int(acc[2]) == 0
    assert torch.equal(acc[1].cpu().double(), sums)
    assert not acc[1].cpu()[counts == 0].any()                            # (also no -0.0: compared as values, then as bits)
    assert not _bits(acc[1])[counts == 0].any()
    # (c) a second batch into the same accumulators
    x2 = x.flip(0).neg().contiguous()
    inds2 = V.given_inds(case, kind, salt=1)
    c2, s2, _, _ = EC.stats64(x2, inds2, case.K)
    _launch(dev, case, x2, inds2, acc)
    assert torch.equal(acc[0].cpu(), counts + c2) and torch.equal(acc[1].cpu().double(), sums + s2) and int(acc[2]) == 0
    both = case._replace(B=2 * case.B)
    acc_b = _acc(dev, both)
    _launch(dev, both, torch.cat([x, x2]), torch.cat([inds, inds2]), acc_b)
    assert torch.equal(acc_b[0], acc[0]) and torch.equal(_bits(acc_b[1]), _bits(acc[1]))
    # (d) sentinels (integers, so the sums stay exact) and a NaN-filled workspace
    acc_d = _acc(dev, case, n_fill=7, s_fill=-3.0)
    acc_d[2].fill_(5)
    _launch(dev, case, x, inds, acc_d, poison_ws=True)
    assert torch.equal(acc_d[0].cpu(), counts + 7) and torch.equal(acc_d[1].cpu().double(), sums - 3.0) and int(acc_d[2]) == 5


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("id", STAT_IDS)
def test_stats_random_inputs(dev, id, kind):
    """(b) random latents against float64 within n_k * u * sum |x| per element; (e) two runs are bit-identical."""
    case = _case(id)
    x, _ = V.random_inputs(case, "o1")
    inds = V.given_inds(case, kind)
    counts, sums, asums, _ = EC.stats64(x, inds, case.K)
    runs = []
    for _ in range(2):
        acc = _acc(dev, case)
        _launch(dev, case, x, inds, acc, poison_ws=True)
        runs.append(acc)
    assert torch.equal(runs[0][0].cpu(), counts)
    err = (runs[0][1].cpu().double() - sums).abs()
    bound = EC.stats_bound(counts, asums)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{id} {kind}: worst error / bound = {worst:.3f}")
    assert bool((err <= bound).all()), worst
    assert torch.equal(_bits(runs[0][1]), _bits(runs[1][1])) and torch.equal(runs[0][0], runs[1][0])


@pytest.mark.parametrize("id", STAT_IDS)
def test_stats_invalid_indices_and_nan_latents(dev, id):
    """(f) planted indices outside [0, K) -- negative, K, and one whose low 32 bits are a valid code -- land in ``invalid`` only;
    (g) a NaN latent reaches exactly the elements its column feeds: (c, idx[p][c], j - c) for every codebook c whose slice
    [c, c + Dc) holds column j."""
    case = _case(id)
    P, Dc = case.B * case.HW, case.D // case.C
    x, _ = V.exact_inputs(case)
    inds = V.given_inds(case, "uniform").clone()
    flat = inds.view(-1)
    spots = sorted({0, flat.numel() // 2, flat.numel() - 1, min(3, flat.numel() - 1)})
    for n, at in enumerate(spots):
        flat[at] = (-1, case.K, 2 ** 33 + (case.K - 1), -(2 ** 40))[n % 4]
    counts, sums, _, invalid = EC.stats64(x, inds, case.K)
    assert invalid == len(spots)
    acc = _acc(dev, case)
    _launch(dev, case, x, inds, acc)
    assert int(acc[2]) == len(spots) and torch.equal(acc[0].cpu(), counts) and torch.equal(acc[1].cpu().double(), sums)
    assert int(acc[0].sum()) == P * case.C - len(spots)
    # (g)
    inds = V.given_inds(case, "uniform")
    rows = V.rows_of(inds)
    p0, j0 = P // 2, min(case.D - 1, case.C)            # a column that several codebooks' slices share when C > 1
    xn = x.clone()
    xn[p0, j0] = float("nan")
    x0 = x.clone()
    x0[p0, j0] = 0.0
    counts, sums, _, _ = EC.stats64(x0, inds, case.K)
    want_nan = torch.zeros(case.C, case.K, Dc, dtype=torch.bool)
    for c in range(case.C):
        if 0 <= j0 - c < Dc:
            want_nan[c, int(rows[p0, c]), j0 - c] = True
    assert int(want_nan.sum()) >= 1
    acc = _acc(dev, case)
    _launch(dev, case, xn, inds, acc)
    got = acc[1].cpu()
    assert torch.equal(got.isnan(), want_nan)
    assert torch.equal(got[~want_nan].double(), sums[~want_nan]) and torch.equal(acc[0].cpu(), counts) and int(acc[2]) == 0


def test_stats_argument_errors_launch_nothing(dev):
    """(h) the wrapper's refusals and the library's own: an error, no launch, the accumulators as they were."""
    from ctvae_amd import kernels as K
    native = _native()
    case = _case("pos-P245")
    x, _ = V.exact_inputs(case)
    x = x.to(dev).view(case.B, case.HW, case.D)
    inds = V.given_inds(case, "uniform").to(dev)
    acc = _acc(dev, case, n_fill=7, s_fill=-3.0)

    def refused():
        for bad in ((x.double(), inds, *acc), (x, inds.int(), *acc), (x.transpose(0, 1), inds, *acc), (x, inds[:, :2].contiguous(), *acc),
                    (x, inds, acc[0], acc[1][:, :, :8].contiguous(), acc[2]), (x, inds, acc[0].float(), acc[1], acc[2])):
            with pytest.raises(ValueError):
                K.vq_ema_stats(*bad)
        lib, ws = native.load(), native.workspace(dev)
        st = native.stream_ptr()
        a = (x.data_ptr(), inds.data_ptr(), acc[0].data_ptr(), acc[1].data_ptr(), acc[2].data_ptr())
        good = (case.B, case.HW, case.D, case.K, case.C)
        codes = [lib.ctvae_vq_ema_stats(*a, *shape, ws.data_ptr(), ws.numel() * 4, st)
                 for shape in ((case.B, case.HW, case.D + 1, case.K, case.C),        # D % C != 0
                               (case.B, case.HW, 9 * 4, case.K, 9),                  # C > 8
                               (case.B, case.HW, 257, case.K, 1),                    # Dc > 256
                               (0, case.HW, case.D, case.K, case.C), (case.B, case.HW, case.D, 0, case.C))]
        codes.append(lib.ctvae_vq_ema_stats(None, *a[1:], *good, ws.data_ptr(), ws.numel() * 4, st))
        codes.append(lib.ctvae_vq_ema_stats(*a, *good, None, ws.numel() * 4, st))
        assert codes == [-22] * 7, codes
        assert lib.ctvae_vq_ema_stats(*a, *good, ws.data_ptr(), 64, st) == -12            # a workspace below one record
        assert lib.ctvae_vq_ema_update(acc[1].data_ptr(), None, acc[1].data_ptr(), acc[0].data_ptr(), acc[1].data_ptr(),
                                       case.C, case.K, case.D // case.C, 0.9, 1e-5, st) == -22
        for decay, eps in ((1.0, 1e-5), (0.0, 1e-5), (0.9, 0.0), (float("nan"), 1e-5)):
            N = torch.ones(case.C, case.K, device=dev)
            assert lib.ctvae_vq_ema_update(acc[1].data_ptr(), N.data_ptr(), acc[1].data_ptr(), acc[0].data_ptr(), acc[1].data_ptr(),
                                           case.C, case.K, case.D // case.C, decay, eps, st) == -22
        assert lib.ctvae_vq_ema_supported(64, 4, 32) == 1 and lib.ctvae_vq_ema_supported(64, 9, 32) == 0
        assert lib.ctvae_vq_ema_supported(64, 1, 257) == 0 and lib.ctvae_vq_ema_supported(0, 1, 4) == 0
    _, log = logged(refused)
    assert not set(log) & ALL_LABELS, log
    assert bool((acc[0] == 7).all()) and bool((acc[1] == -3.0).all()) and int(acc[2]) == 0


# ---- update ----------------------------------------------------------------------------------------------------
def _update_inputs(K_, C, Dc, seed):
    g = torch.Generator().manual_seed(seed)
    N = torch.rand(C, K_, generator=g) * 4 + 0.01
    M = torch.randn(C, K_, Dc, generator=g)
    acc_n = torch.randint(0, 50, (C, K_), generator=g)
    acc_n[:, ::3] = 0                                                     # unused codes in every codebook (all of them when K = 1)
    acc_s = torch.randn(C, K_, Dc, generator=g) * acc_n[..., None]
    return N, M, acc_n, acc_s


@pytest.mark.parametrize("Dc", [5, 32, 128])
@pytest.mark.parametrize("C", [1, 4, 8])
@pytest.mark.parametrize("K_", [1, 37, 64, 512])
def test_update_matches_float64(dev, K_, C, Dc):
    from ctvae_amd import kernels as K
    for decay, eps in ((EC.fp32(0.99), EC.fp32(1e-5)), (EC.fp32(0.3), EC.fp32(0.5))):
        N, M, acc_n, acc_s = _update_inputs(K_, C, Dc, 1000 * K_ + 10 * C + Dc)
        ref = EC.update64(N, M, acc_n, acc_s, decay, eps)
        bound = EC.update_bounds(N, M, acc_n, acc_s, decay, eps)
        d = [t.to(dev) for t in (N, M, acc_n, acc_s)]
        cb = torch.full((C, K_, Dc), float("nan"), device=dev)           # every code is overwritten, whatever was there
        _, log = logged(lambda: K.vq_ema_update(cb, d[0], d[1], d[2], d[3], decay, eps))
        assert log["vq_ema_update_kernel"]["count"] == 1 and set(log) & ALL_LABELS == {"vq_ema_update_kernel"}
        for name, got in (("N", d[0]), ("M", d[1]), ("E", cb)):
            err = (got.cpu().double() - ref[name]).abs()
            worst = float((err / bound[name].clamp_min(1e-300)).max())
            assert bool((err <= bound[name]).all()), (name, decay, worst)
        assert not d[2].any() and not d[3].any() and not _bits(d[3]).any()      # the accumulators read zero afterwards


@pytest.mark.parametrize("K_,C,Dc", [(1, 1, 5), (37, 4, 32), (64, 4, 32), (64, 1, 128), (512, 1, 64), (512, 8, 128)])
def test_update_of_an_empty_window_leaves_the_codebook(dev, K_, C, Dc):
    """N = 1, M = E, nothing observed: E stays within the update's own bound of its old value; and over two more empty windows
    within twice that bound of the value before -- which itself carries one update's error against the exact M / Nt."""
    from ctvae_amd import kernels as K
    g = torch.Generator().manual_seed(K_ + C + Dc)
    E = torch.randn(C, K_, Dc, generator=g)
    decay, eps = EC.fp32(0.99), EC.fp32(1e-5)
    cb, N, M = E.to(dev), torch.ones(C, K_, device=dev), E.to(dev).clone()
    acc_n, acc_s = torch.zeros(C, K_, dtype=torch.int64, device=dev), torch.zeros(C, K_, Dc, device=dev)
    for step in range(3):
        bound = EC.update_bounds(N.cpu(), M.cpu(), acc_n.cpu(), acc_s.cpu(), decay, eps)["E"]
        old = cb.cpu().double()
        K.vq_ema_update(cb, N, M, acc_n, acc_s, decay, eps)
        err = (cb.cpu().double() - old).abs()
        limit = bound if step == 0 else 2 * bound
        assert bool((err <= limit).all()), (step, float((err / bound.clamp_min(1e-300)).max()))
    assert float(N.max()) < 1.0


def test_observe_update_and_reset_through_codebook_ema(dev):
    """optim.CodebookEMA on a stand-alone quantiser: observe() twice and update() equal the float64 update of the summed
    statistics; restarted codes then carry N = 1 and M = their row."""
    from ctvae_amd.models.mcq_vae import VectorQuantizerMS
    from ctvae_amd.optim import CodebookEMA
    case = _case("scan1-K80-P100")
    torch.manual_seed(5)
    vq = VectorQuantizerMS(case.K, case.D).to(dev)
    ema = CodebookEMA(vq, 0.9)
    E0 = vq.embedding.weight.detach().cpu().clone().unsqueeze(0)
    x, _ = V.random_inputs(case, "o1")
    stats = []
    for salt in (0, 1):
        inds = V.given_inds(case, "uniform", salt=salt)
        ema.observe(inds.to(dev).view(case.B, 1, 5, 5), x.to(dev).view(case.B, 5, 5, case.D))
        stats.append(EC.stats64(x, inds, case.K))
    assert ema.observed == 2 and torch.equal(ema.acc_n.cpu(), stats[0][0] + stats[1][0])
    acc_n, acc_s = ema.acc_n.cpu().clone(), ema.acc_s.cpu().clone()
    err = (acc_s.double() - (stats[0][1] + stats[1][1])).abs()
    assert bool((err <= EC.stats_bound(acc_n, stats[0][2] + stats[1][2])).all())
    ema.update()
    ref = EC.update64(torch.ones(1, case.K), E0, acc_n, acc_s, ema.decay, ema.eps)
    bound = EC.update_bounds(torch.ones(1, case.K), E0, acc_n, acc_s, ema.decay, ema.eps)
    got = vq.embedding.weight.detach().cpu().double().unsqueeze(0)
    assert bool(((got - ref["E"]).abs() <= bound["E"]).all()) and ema.updates == 1
    assert not ema.acc_n.any() and not ema.acc_s.any()
    rows = torch.arange(2 * case.D, dtype=torch.float32).view(2, case.D)
    before_N, before_M = ema.N.cpu().clone(), ema.M.cpu().clone()
    ema.reset_codes([(0, 3, 17), (0, 40, 2)], rows.to(dev))
    keep = torch.ones(case.K, dtype=torch.bool)
    keep[[3, 40]] = False
    assert ema.N.cpu()[0, [3, 40]].tolist() == [1.0, 1.0] and torch.equal(ema.M.cpu()[0, [3, 40]], rows)
    assert torch.equal(ema.N.cpu()[0, keep], before_N[0, keep]) and torch.equal(ema.M.cpu()[0, keep], before_M[0, keep])
    ema.reset_codes([(0, 5)])                                             # without rows: the code's own codebook row
    assert float(ema.N[0, 5]) == 1.0 and torch.equal(ema.M[0, 5], vq.embedding.weight.detach()[5])
