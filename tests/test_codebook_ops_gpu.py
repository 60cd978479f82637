"""GPU: the codebook usage kernels (csrc/vqusage.hip) op by op against torch: ``ctvae_vq_usage`` against ``torch.bincount``,
``ctvae_vq_pool_fill`` against the source rows, ``ctvae_vq_usage_pool_fill`` (both in one launch) against both,
``ctvae_vq_restart`` / ``ctvae_vq_restart_gather`` against a Python restatement.
Everything is integers or raw 32-bit words, so every comparison is exact.  Buffers under test sit between guard words."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GUARD = 8


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _guarded(dev, shape, dtype, fill):
    """(view of ``shape`` inside a buffer with GUARD words of ``fill`` on either side, the whole buffer)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return whole[GUARD:GUARD + n].view(shape), whole


def _guards_intact(whole, fill):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


def _words(t):
    return t.detach().contiguous().view(torch.int32).cpu()


# ---- usage -------------------------------------------------------------------------------------------------
def _bincounts(inds, C, K):
    """torch.bincount per codebook on the host, and the number of indices outside [0, K)."""
    flat = inds.cpu().reshape(inds.size(0), C, -1)
    ok = (flat >= 0) & (flat < K)
    ref = torch.stack([torch.bincount(flat[:, c][ok[:, c]], minlength=K) for c in range(C)])
    return ref, int((~ok).sum())


def _past_one_grid():
    from ctvae_amd import kernels as K
    return K.vq_usage_pass_indices() + 1


@pytest.mark.parametrize("C", [1, 4])
@pytest.mark.parametrize("K_", [1, 3, 64, 65, 512])
def test_usage_matches_bincount(dev, K_, C):
    """P = B * HW latent rows in {1, 63, 64, 65, 257, one past a full grid of workgroups}, as (B, HW) pairs that also move the
    codebook boundary (HW) off every power of two."""
    from ctvae_amd import kernels as K
    big = _past_one_grid()
    shapes = [(1, 1), (1, 63), (1, 64), (5, 13), (1, 257), (1, big), (7, -(-big // (7 * C)))]
    assert 7 * C * shapes[-1][1] > K.vq_usage_pass_indices()
    for i, (B, HW) in enumerate(shapes):
        g = torch.Generator().manual_seed(100 * K_ + 10 * C + i)
        inds = torch.randint(0, K_, (B, C, HW), generator=g).to(dev)
        counts, whole = _guarded(dev, (C, K_), torch.int64, -7)
        counts.zero_()
        invalid = torch.zeros(1, dtype=torch.int64, device=dev)
        K.vq_usage(inds, counts, invalid)
        ref, bad = _bincounts(inds, C, K_)
        assert torch.equal(counts.cpu(), ref), (B, HW)
        assert int(invalid) == bad == 0 and int(counts.sum()) == B * C * HW
        assert _guards_intact(whole, -7)


def test_usage_accumulates_and_takes_4d_indices(dev):
    """Two calls add up; [B, C, H, W] (what the quantisers hand over) is read as [B, C, HW]."""
    from ctvae_amd import kernels as K
    g = torch.Generator().manual_seed(3)
    a = torch.randint(0, 64, (4, 4, 8, 8), generator=g).to(dev)
    b = torch.randint(0, 64, (3, 4, 5, 7), generator=g).to(dev)
    counts, whole = _guarded(dev, (4, 64), torch.int64, -7)
    counts.copy_(torch.arange(256).view(4, 64))            # counts += histogram: what was there stays
    invalid = torch.full((1,), 5, dtype=torch.int64, device=dev)
    K.vq_usage(a, counts, invalid)
    K.vq_usage(b, counts, invalid)
    ref = torch.arange(256).view(4, 64) + _bincounts(a, 4, 64)[0] + _bincounts(b, 4, 64)[0]
    assert torch.equal(counts.cpu(), ref) and int(invalid) == 5 and _guards_intact(whole, -7)


@pytest.mark.parametrize("C,K_,code", [(1, 512, 511), (4, 64, 0), (4, 3, 1)])
def test_usage_under_worst_case_contention(dev, C, K_, code):
    """All indices equal: every lane of every wave adds to one LDS word, every workgroup to one global word."""
    from ctvae_amd import kernels as K
    HW = _past_one_grid() // C + 3
    inds = torch.full((2, C, HW), code, dtype=torch.int64, device=dev)
    counts, whole = _guarded(dev, (C, K_), torch.int64, -7)
    counts.zero_()
    invalid = torch.zeros(1, dtype=torch.int64, device=dev)
    K.vq_usage(inds, counts, invalid)
    ref = torch.zeros(C, K_, dtype=torch.int64)
    ref[:, code] = 2 * HW
    assert torch.equal(counts.cpu(), ref) and int(invalid) == 0 and _guards_intact(whole, -7)


def test_usage_counts_invalid_indices_apart(dev):
    """Negative and >= K indices land in ``invalid`` only: neither in a neighbouring code nor in a neighbouring codebook."""
    from ctvae_amd import kernels as K
    K_, C = 65, 4
    g = torch.Generator().manual_seed(9)
    inds = torch.randint(0, K_, (3, C, 300), generator=g)
    inds[0, 0, :7] = -1
    inds[1, 1, 5] = K_
    inds[2, 3, 299] = K_ + 1
    inds[2, 2, 0] = -(2 ** 40)
    inds[0, 3, 1] = 2 ** 33 + 3                            # (a truncation to 32 bits would make it code 3)
    inds = inds.to(dev)
    counts, whole = _guarded(dev, (C, K_), torch.int64, -7)
    counts.zero_()
    invalid, iw = _guarded(dev, (1,), torch.int64, -7)
    invalid.zero_()
    K.vq_usage(inds, counts, invalid)
    ref, bad = _bincounts(inds, C, K_)
    assert bad == 11 and int(invalid) == 11
    assert torch.equal(counts.cpu(), ref) and int(counts.sum()) == 3 * C * 300 - 11
    assert _guards_intact(whole, -7) and _guards_intact(iw, -7)


# ---- pool fill ---------------------------------------------------------------------------------------------
def _latents(dev, P, D, seed):
    """Random words, NaN payloads and -0 among them, as fp32 [P, D]."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(-2 ** 31, 2 ** 31 - 1, (P, D), generator=g, dtype=torch.int64).to(torch.int32)
    w[0, 0] = -2 ** 31                                      # -0
    w[-1, -1] = 0x7FC01234                                  # a NaN with a payload
    return w.to(dev).view(torch.float32)


@pytest.mark.parametrize("D", [32, 64, 128, 35])
@pytest.mark.parametrize("P,R", [(5, 9), (9, 9), (300, 9), (257, 1024), (1, 1)])
def test_pool_fill_copies_the_first_rows_bitwise(dev, D, P, R):
    from ctvae_amd import kernels as K
    lat = _latents(dev, P, D, 7 * D + P)
    pool, whole = _guarded(dev, (R, D), torch.float32, -3.5)
    before = _words(pool)
    rows = K.vq_pool_fill(lat, pool)
    assert rows == min(P, R)
    assert torch.equal(_words(pool)[:rows], _words(lat)[:rows])
    assert torch.equal(_words(pool)[rows:], before[rows:]), "rows beyond min(P, R) were written"
    assert _guards_intact(whole, -3.5)


def test_pool_fill_takes_nhwc_latents_and_an_unaligned_pool(dev):
    """[B, H, W, D] is P = B * H * W rows; a pool off the 16-byte grid runs the word-by-word path."""
    from ctvae_amd import kernels as K
    lat = _latents(dev, 4 * 3 * 5, 32, 1).view(4, 3, 5, 32)
    whole = torch.full((1 + 40 * 32 + GUARD,), -3.5, device=dev)
    pool = whole[1:1 + 40 * 32].view(40, 32)
    assert pool.data_ptr() % 16 == 4
    assert K.vq_pool_fill(lat, pool) == 40
    assert torch.equal(_words(pool), _words(lat.view(60, 32))[:40])
    assert float(whole[0]) == -3.5 and bool((whole[-GUARD:] == -3.5).all())


# ---- both in one launch ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K_,B,HW,D,R", [(4, 64, 4, 64, 128, 1024), (4, 64, 4, 64, 128, 100), (1, 512, 4, 256, 64, 1024),
                                           (4, 65, 3, 7, 35, 21), (1, 1, 1, 1, 32, 1), (4, 64, 5, -1, 128, 64)])
def test_usage_and_pool_fill_in_one_launch(dev, C, K_, B, HW, D, R):
    """What a training forward issues: the counting workgroups and the copying workgroups of one grid give what the two
    launches give.  HW = -1: one index past a full grid of counting workgroups."""
    from ctvae_amd import kernels as K
    if HW < 0:
        HW = _past_one_grid() // (B * C) + 1
    g = torch.Generator().manual_seed(C + K_ + B + D)
    inds = torch.randint(0, K_, (B, C, HW), generator=g)
    inds[0, 0, 0] = -1
    inds[-1, -1, -1] = K_
    inds = inds.to(dev)
    P = min(B * HW, 300)                                    # (the launch takes the latents' own row count)
    lat = _latents(dev, P, D, 5)
    counts, cw = _guarded(dev, (C, K_), torch.int64, -7)
    counts.fill_(2)
    invalid, iw = _guarded(dev, (1,), torch.int64, -7)
    invalid.zero_()
    pool, pw = _guarded(dev, (R, D), torch.float32, -3.5)
    before = _words(pool)
    rows = K.vq_usage_pool_fill(inds, counts, invalid, lat, pool)
    ref, bad = _bincounts(inds, C, K_)
    assert rows == min(P, R) and bad == int(invalid) == (1 if B * C * HW == 1 else 2)
    assert torch.equal(counts.cpu(), ref + 2)
    assert torch.equal(_words(pool)[:rows], _words(lat)[:rows]) and torch.equal(_words(pool)[rows:], before[rows:])
    assert _guards_intact(cw, -7) and _guards_intact(iw, -7) and _guards_intact(pw, -3.5)


def test_one_launch_refuses_either_half_before_writing(dev):
    from ctvae_amd import kernels as K
    inds = torch.zeros((2, 4, 16), dtype=torch.int64, device=dev)
    counts = torch.full((4, 64), 3, dtype=torch.int64, device=dev)
    invalid = torch.full((1,), 3, dtype=torch.int64, device=dev)
    pool = torch.full((8, 32), 3.0, device=dev)
    lat = torch.ones((32, 32), device=dev)
    with pytest.raises(ValueError, match="vq_usage_pool_fill: latents must be a torch.float32"):
        K.vq_usage_pool_fill(inds, counts, invalid, lat.double(), pool)
    with pytest.raises(ValueError, match="vq_usage_pool_fill: inds must be a torch.int64"):
        K.vq_usage_pool_fill(inds.int(), counts, invalid, lat, pool)
    with pytest.raises(ValueError, match="vq_usage_pool_fill: num_embeddings K=513"):
        K.vq_usage_pool_fill(inds[:, :1].contiguous(), torch.full((1, 513), 3, dtype=torch.int64, device=dev), invalid, lat, pool)
    with pytest.raises(ValueError, match="vq_usage_pool_fill: pool must be contiguous"):
        K.vq_usage_pool_fill(inds, counts, invalid, lat, torch.full((32, 8), 3.0, device=dev).t())
    torch.cuda.synchronize()
    assert bool((counts == 3).all()) and int(invalid) == 3 and bool((pool == 3.0).all())


# ---- restart -----------------------------------------------------------------------------------------------
def _restart_case(dev, C, K_, Dc, D, R, seed):
    g = torch.Generator().manual_seed(seed)

    def words(shape):
        w = torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32)
        w.view(-1)[::7] = 0x7FC00000 + 11                   # NaN payloads among the neighbours
        return w
    pool = words((R, D)).to(dev).view(torch.float32)
    bufs = []
    for _ in range(3):
        view, whole = _guarded(dev, (C, K_, Dc), torch.float32, -3.5)
        view.view(torch.int32).copy_(words((C, K_, Dc)))
        bufs.append((view, whole))
    return pool, bufs


def _restated(entries, pool_w, cb_w, m_w, v_w, Dc):
    """The Python restatement on raw words: E_c[k][d] = pool[row][c + d], both moments 0."""
    cb_w, m_w, v_w = cb_w.clone(), m_w.clone(), v_w.clone()
    for c, k, row in entries:
        for d in range(Dc):
            cb_w[c, k, d] = pool_w[row, c + d]
            m_w[c, k, d] = 0
            v_w[c, k, d] = 0
    return cb_w, m_w, v_w


def _entry_lists(C, K_, R, seed):
    g = torch.Generator().manual_seed(seed)
    everything = [(c, k, int(torch.randint(0, R, (1,), generator=g))) for c in range(C) for k in range(K_)]
    return {"none": [], "one": [(C - 1, K_ - 1, R - 1)], "two_same_row": [(0, 0, 3), (C - 1, 1 % K_, 3)] if C * K_ > 1 else [],
            "all": everything}


@pytest.mark.parametrize("C,K_,Dc,D", [(4, 64, 32, 128), (1, 64, 128, 128), (1, 512, 64, 64)])
@pytest.mark.parametrize("which", ["none", "one", "two_same_row", "all"])
def test_restart_matches_the_restatement(dev, C, K_, Dc, D, which):
    from ctvae_amd import kernels as K
    R = 40
    pool, bufs = _restart_case(dev, C, K_, Dc, D, R, 13 * C + K_)
    (cb, cbw), (m, mw), (v, vw) = bufs
    entries = _entry_lists(C, K_, R, 5)[which]
    if which == "two_same_row":
        assert len(entries) == 2 and entries[0][2] == entries[1][2]
    before = [_words(t) for t in (cb, m, v)]
    ref = _restated(entries, _words(pool), *before, Dc)
    K.vq_restart(entries, pool, R, cb, m, v)
    got = [_words(t) for t in (cb, m, v)]
    for name, a, b in zip(("codebook", "exp_avg", "exp_avg_sq"), got, ref):
        assert torch.equal(a, b), (name, which)
    if which == "none":
        assert all(torch.equal(a, b) for a, b in zip(got, before))
    else:
        c, k, row = entries[0]
        assert torch.equal(got[0][c, k], _words(pool)[row, c:c + Dc])          # the slice offset is c, not c * Dc
        assert not got[1][c, k].any() and not got[2][c, k].any()
    assert all(_guards_intact(w, -3.5) for w in (cbw, mw, vw))


def test_restart_reads_only_valid_rows_and_takes_a_tensor_list(dev):
    """valid_rows below R: rows behind it are refused; the list may be a host int64 [n, 3] tensor."""
    from ctvae_amd import kernels as K
    pool, bufs = _restart_case(dev, 4, 8, 4, 16, 10, 2)
    (cb, _), (m, _), (v, _) = bufs
    before = [_words(t) for t in (cb, m, v)]
    entries = torch.tensor([[1, 2, 5], [3, 7, 0]])
    K.vq_restart(entries, pool, 6, cb, m, v)
    ref = _restated(entries.tolist(), _words(pool), *before, 4)
    assert all(torch.equal(_words(t), r) for t, r in zip((cb, m, v), ref))
    with pytest.raises(ValueError, match=r"vq_restart: entry 0 \(c=1, k=2, row=6\)"):
        K.vq_restart([(1, 2, 6)], pool, 6, cb, m, v)


def test_restart_split_for_data_parallel_runs(dev):
    """gather -> (broadcast) -> scatter gives what the direct launch gives; the scatter does not read the pool."""
    from ctvae_amd import kernels as K
    C, K_, Dc, D, R = 4, 64, 32, 128, 40
    entries = _entry_lists(C, K_, R, 8)["all"][::3]
    pool, bufs = _restart_case(dev, C, K_, Dc, D, R, 21)
    direct = [t.clone() for t, _ in bufs]
    K.vq_restart(entries, pool, R, *direct)
    rows = K.vq_restart_gather(entries, pool, R, C, Dc)
    assert tuple(rows.shape) == (len(entries), Dc)
    pw = _words(pool)
    assert torch.equal(_words(rows), torch.stack([pw[r, c:c + Dc] for c, _, r in entries]))
    (cb, cbw), (m, mw), (v, vw) = bufs
    K.vq_restart(entries, None, 0, cb, m, v, rows=rows)
    assert all(torch.equal(_words(a), _words(b)) for a, b in zip((cb, m, v), direct))
    assert all(_guards_intact(w, -3.5) for w in (cbw, mw, vw))
    assert tuple(K.vq_restart_gather([], pool, R, C, Dc).shape) == (0, Dc)


# ---- refusals ----------------------------------------------------------------------------------------------
def test_refusals_name_the_argument_and_leave_memory_untouched(dev):
    from ctvae_amd import kernels as K
    inds = torch.zeros((2, 4, 16), dtype=torch.int64, device=dev)
    counts = torch.full((4, 64), 3, dtype=torch.int64, device=dev)
    invalid = torch.full((1,), 3, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="vq_usage: inds must be a torch.int64"):
        K.vq_usage(inds.int(), counts, invalid)
    with pytest.raises(ValueError, match="vq_usage: counts must be a torch.int64"):
        K.vq_usage(inds, counts.int(), invalid)
    with pytest.raises(ValueError, match="vq_usage: inds must be contiguous"):
        K.vq_usage(torch.zeros((2, 16, 4), dtype=torch.int64, device=dev).transpose(1, 2), counts, invalid)
    with pytest.raises(ValueError, match="vq_usage: counts must be contiguous"):
        K.vq_usage(inds, torch.zeros((64, 4), dtype=torch.int64, device=dev).t(), invalid)
    with pytest.raises(ValueError, match="do not fit together"):
        K.vq_usage(inds, torch.zeros((3, 64), dtype=torch.int64, device=dev), invalid)
    big = torch.full((1, 513), 3, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="K=513 with C=1"):
        K.vq_usage(inds[:, :1].contiguous(), big, invalid)
    wide = torch.full((32, 512), 3, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="K=512 with C=32"):
        K.vq_usage(torch.zeros((1, 32, 4), dtype=torch.int64, device=dev), wide, invalid)
    torch.cuda.synchronize()
    assert bool((counts == 3).all()) and bool((big == 3).all()) and bool((wide == 3).all()) and int(invalid) == 3

    pool = torch.full((8, 32), 3.0, device=dev)
    lat = torch.ones((4, 32), device=dev)
    with pytest.raises(ValueError, match="vq_pool_fill: latents must be a torch.float32"):
        K.vq_pool_fill(lat.double(), pool)
    with pytest.raises(ValueError, match="vq_pool_fill: latents must be contiguous"):
        K.vq_pool_fill(torch.ones((32, 4), device=dev).t(), pool)
    with pytest.raises(ValueError, match="vq_pool_fill: pool must be contiguous"):
        K.vq_pool_fill(lat, torch.full((32, 8), 3.0, device=dev).t())
    with pytest.raises(ValueError, match="do not fit together"):
        K.vq_pool_fill(torch.ones((4, 16), device=dev), pool)
    torch.cuda.synchronize()
    assert bool((pool == 3.0).all())

    cb, m, v = (torch.full((4, 8, 4), x, device=dev) for x in (1.0, 2.0, 3.0))
    rpool = torch.full((10, 16), 9.0, device=dev)
    for bad in ([(4, 0, 0)], [(0, 8, 0)], [(0, 0, 10)], [(-1, 0, 0)], [(0, 0, 0), (0, -1, 0)], [(0, 0, -1)]):
        with pytest.raises(ValueError, match=r"vq_restart: entry \d \(c=.*out of range"):
            K.vq_restart(bad, rpool, 10, cb, m, v)
    with pytest.raises(ValueError, match="listed twice"):
        K.vq_restart([(0, 1, 0), (0, 1, 2)], rpool, 10, cb, m, v)
    with pytest.raises(ValueError, match="vq_restart: exp_avg must be a torch.float32"):
        K.vq_restart([(0, 0, 0)], rpool, 10, cb, m.double(), v)
    with pytest.raises(ValueError, match="vq_restart: codebooks must be contiguous"):
        K.vq_restart([(0, 0, 0)], rpool, 10, torch.ones((4, 4, 8), device=dev).transpose(1, 2), m, v)
    with pytest.raises(ValueError, match="vq_restart: pool must be a torch.float32"):
        K.vq_restart([(0, 0, 0)], rpool.half(), 10, cb, m, v)
    with pytest.raises(ValueError, match="vq_restart: pool"):
        K.vq_restart([(0, 0, 0)], torch.ones((10, 6), device=dev), 10, cb, m, v)      # C - 1 + Dc = 7 channels do not fit 6
    with pytest.raises(ValueError, match="vq_restart: rows must be"):
        K.vq_restart([(0, 0, 0)], None, 0, cb, m, v, rows=torch.ones((2, 4), device=dev))
    with pytest.raises(ValueError, match=r"vq_restart_gather: entry 0 .*out of range"):
        K.vq_restart_gather([(0, 0, 10)], rpool, 10, 4, 4)
    torch.cuda.synchronize()
    assert bool((cb == 1.0).all()) and bool((m == 2.0).all()) and bool((v == 3.0).all())
