"""GPU: csrc/codeprior.hip op by op against the float64 restatement of tests/codeprior_checks.py, at the shapes at which the
kernels can go wrong: (K, C, H, W) = (5, 1, 1, 1) -- every context a boundary --, (64, 4, 8, 8) -- configs/mcq_vae.yaml --,
(65, 3, 2, 3) -- a ragged last lane, H != W -- and (512, 1, 16, 16) -- VQVAE, eight codes per lane; B or n in {1, 3, 70}.

Bounds.  count, sample, embed: integers and raw words, compared exactly, no element left out.  score: both sides are float64 over
the same quotients and differ by the summation order (a strided partial per thread and a tree of depth 8 against ``math.fsum``)
and by an ulp or two of ``log``: 1e-12 of the summed magnitudes per element, the project's float64 bound of the loglik tests.

The tables of a case are the restatement's count of seeded chain grids that never use the last code (so the context rows K - 1
are empty), with the position row 0 of codebook 0 emptied and two entries preset to 2^33 (nothing may be narrowed to 32 bits)."""
import functools

import numpy as np
import pytest
import torch

from ctvae_amd import filler
from tests import codeprior_checks as R
from tests import helpers as H

pytestmark = pytest.mark.gpu
SHAPES = [(5, 1, 1, 1), (64, 4, 8, 8), (65, 3, 2, 3), (512, 1, 16, 16)]
BATCHES = (1, 3, 70)
BIG = 1 << 33
NEAR_ONE = float(np.nextafter(1.0, 0.0))
LAM_BINARY = (0.125, 0.125, 0.25, 0.25, 0.25)            # exact sums: u1 can sit exactly on a boundary


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Host side of a shape, computed once and never modified: the tables, the grids to score, their reference."""
    K, C, H, W = shape
    seed = 100 + K
    train = R.chain_fixture(seed, 48, max(K - 1, 1), C, H, W)            # codes in [0, K - 1): the rows K - 1 stay empty
    tables, _ = R.count(train, K)
    if H * W > 1:
        tables[0][0, 0, :] = 0                                             # an empty position row
    tables[1][0, K, 0] += BIG                                              # the left boundary row of codebook 0
    tables[0][C - 1, H * W - 1, K - 1] += BIG
    grids = R.chain_fixture(seed + 1, 70, K, C, H, W)                      # every code, the last one included
    rng = np.random.default_rng(seed + 2)
    lam = rng.random((C, R.J)) + 0.05
    lam /= lam.sum(axis=1, keepdims=True)
    for t in tables:
        t.setflags(write=False)
    grids.setflags(write=False)
    return {"tables": tables, "grids": grids, "lam": lam, "score": R.score(grids, tables, lam, K)}


def _dev_tables(tables, dev):
    from ctvae_amd import kernels as Kn
    t = tuple(torch.from_numpy(np.array(x)).to(dev) for x in tables)
    return t, Kn.code_prior_totals(t)


# ---- count -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("shape", SHAPES)
def test_count_matches_add_at_and_accumulates(dev, shape, B):
    from ctvae_amd import kernels as Kn
    K, C, H, W = shape
    grids = np.array(_case(shape)["grids"][:B])
    if B > 1:                                                              # out of range: above, below, far outside
        grids[1, C - 1, H - 1, W - 1] = K
        grids[B - 1, 0, 0, 0] = -1
        grids[B // 2, 0, H // 2, 0] = 1 << 40
    ref, ref_invalid = R.count(grids, K)
    tables, invalid = Kn.code_prior_tables(K, C, H, W, dev)
    x = torch.from_numpy(grids).to(dev)
    Kn.code_prior_count(x, tables, invalid)
    for name, got, want in zip(Kn.CODE_PRIOR_TABLES, tables, ref):
        assert np.array_equal(got.cpu().numpy(), want), name
    assert int(invalid) == ref_invalid and (ref_invalid > 0) == (B > 1)
    assert all(int(t.sum()) == B * C * H * W - ref_invalid for t in tables)
    Kn.code_prior_count(x, tables, invalid)                                # a second call accumulates
    for name, got, want in zip(Kn.CODE_PRIOR_TABLES, tables, ref):
        assert np.array_equal(got.cpu().numpy(), 2 * want), name
    assert int(invalid) == 2 * ref_invalid


# ---- score -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_score_matches_the_restatement_and_ignores_the_batch(dev, shape):
    from ctvae_amd import kernels as Kn
    K, C, H, W = shape
    case = _case(shape)
    tables, totals = _dev_tables(case["tables"], dev)
    assert max(int(t.max()) for t in totals) >= BIG
    lam = torch.from_numpy(case["lam"]).to(dev)
    x = torch.from_numpy(np.array(case["grids"])).to(dev)
    ref_logp, ref_resp, ref_bad, logp_scale, resp_scale = case["score"]
    got = {}
    for B in BATCHES:
        logp, resp, bad = Kn.code_prior_score(x[:B].contiguous(), tables, totals, lam)
        got[B] = (logp.cpu().numpy(), resp.cpu().numpy(), bad.cpu().numpy())
        assert got[B][0].shape == (B, C) and got[B][1].shape == (B, C, R.J) and got[B][2].dtype == np.int32
        err_l, err_r = np.abs(got[B][0] - ref_logp[:B]), np.abs(got[B][1] - ref_resp[:B])
        print(f"{shape} B={B}: max logp err / scale {np.max(err_l / logp_scale[:B]):.2e}, "
              f"max resp err {np.max(err_r):.2e} of {np.max(resp_scale):.1f}")
        assert (err_l <= 1e-12 * logp_scale[:B]).all() and (err_r <= 1e-12 * resp_scale[:B]).all()
        assert not got[B][2].any() and np.isfinite(got[B][0]).all() and (got[B][0] < 0).all()
        # the responsibilities of a token sum to 1: H * W per (image, codebook)
        assert np.abs(got[B][1].sum(axis=2) - H * W).max() <= 1e-12 * H * W
    # a row's result does not depend on the batch it arrived in: bit for bit
    for B in (1, 3):
        assert np.array_equal(got[B][0].view(np.int64), got[70][0][:B].view(np.int64))
        assert np.array_equal(got[B][1].view(np.int64), got[70][1][:B].view(np.int64))
    for i in (37, 69):
        logp, resp, _ = Kn.code_prior_score(x[i:i + 1].contiguous(), tables, totals, lam)
        assert np.array_equal(logp.cpu().numpy().view(np.int64), got[70][0][i:i + 1].view(np.int64))
        assert np.array_equal(resp.cpu().numpy().view(np.int64), got[70][1][i:i + 1].view(np.int64))


@pytest.mark.parametrize("shape", SHAPES)
def test_score_flags_bad_images_and_zeroes_them(dev, shape):
    from ctvae_amd import kernels as Kn
    K, C, H, W = shape
    case = _case(shape)
    tables, totals = _dev_tables(case["tables"], dev)
    lam = torch.from_numpy(case["lam"]).to(dev)
    grids = np.array(case["grids"][:3])
    grids[0, C - 1, H - 1, W - 1] = K
    grids[2, 0, 0, 0] = -1
    logp, resp, bad = Kn.code_prior_score(torch.from_numpy(grids).to(dev), tables, totals, lam)
    assert bad.cpu().tolist() == [1, 0, 1]
    assert not logp[0].any() and not logp[2].any() and not resp[0].any() and not resp[2].any()
    ref = case["score"]
    assert np.array_equal(R.score(grids, case["tables"], case["lam"], K)[2], [1, 0, 1])
    assert (np.abs(logp[1].cpu().numpy() - ref[0][1]) <= 1e-12 * ref[3][1]).all()


# ---- sample ----------------------------------------------------------------------------------------------------------------
def _uniforms(shape, n, seed):
    """[n, H*W, C, 2] in [0, 1) with the edge values planted: u2 = 0 and nextafter(1, 0), u1 on the boundaries of LAM_BINARY."""
    K, C, H, W = shape
    rng = np.random.default_rng(seed)
    u = rng.random((n, H * W, C, 2))
    flat = u.reshape(-1, 2)
    m = len(flat)
    flat[rng.choice(m, max(m // 16, 1), replace=False), 1] = 0.0
    flat[rng.choice(m, max(m // 16, 1), replace=False), 1] = NEAR_ONE
    for b in (0.0, 0.125, 0.25, 0.5, 0.75, NEAR_ONE):
        flat[rng.choice(m, max(m // 32, 1), replace=False), 0] = b
    return u


@functools.lru_cache(maxsize=None)
def _sample_case(shape):
    K, C, H, W = shape
    case = _case(shape)
    lams = {"binary": np.tile(np.array(LAM_BINARY), (C, 1)), "fitted": case["lam"]}
    for j in range(R.J):
        one = np.zeros((C, R.J))
        one[:, j] = 1.0
        lams[f"onehot{j}"] = one
    out = {}
    for i, (name, lam) in enumerate(lams.items()):
        n = 70 if name == "binary" else 3
        u = _uniforms(shape, n, 900 + 10 * K + i)
        if name == "binary" and H * W * C >= 2:
            u[0, 0, 0] = (0.0, 0.0)                   # the first token of the first image: the first expert, the first code
            u[0, -1, -1] = (NEAR_ONE, NEAR_ONE)       # the last one: the last expert, the end of its row
        out[name] = (lam, u, R.sample(case["tables"], lam, u, H, W))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_sample_matches_the_restatement_bit_for_bit(dev, shape):
    from ctvae_amd import kernels as Kn
    K, C, H, W = shape
    tables, totals = _dev_tables(_case(shape)["tables"], dev)
    seen = set()
    for name, (lam, u, ref) in _sample_case(shape).items():
        lam_d, u_d = torch.from_numpy(lam).to(dev), torch.from_numpy(u).to(dev)
        for n in (BATCHES if name == "binary" else (3,)):
            got = Kn.code_prior_sample(tables, totals, lam_d, u_d[:n].contiguous(), H, W)
            assert got.dtype == torch.int64 and tuple(got.shape) == (n, C, H, W)
            got = got.cpu().numpy()
            assert np.array_equal(got, ref[:n]), (name, n, np.argwhere(got != ref[:n])[:4].tolist())
            assert got.min() >= 0 and got.max() < K
        seen.update(np.unique(ref).tolist())
    assert K - 1 in seen and 0 in seen                      # (the planted ends are reached)


def test_sample_reads_the_preset_2_33_row_in_64_bits(dev):
    """The left boundary row of codebook 0 holds 2^33 at code 0 and a few counts elsewhere: a total narrowed to 32 bits would
    choose the other codes almost always; in 64 bits nearly every draw at w = 0 under the left expert is code 0."""
    from ctvae_amd import kernels as Kn
    shape = (64, 4, 8, 8)
    K, C, H, W = shape
    tables, totals = _dev_tables(_case(shape)["tables"], dev)
    lam = np.zeros((C, R.J))
    lam[:, 2] = 1.0
    u = np.random.default_rng(5).random((3, H * W, C, 2))
    got = Kn.code_prior_sample(tables, totals, torch.from_numpy(lam).to(dev), torch.from_numpy(u).to(dev), H, W).cpu().numpy()
    assert np.array_equal(got, R.sample(_case(shape)["tables"], lam, u, H, W))
    assert (got[:, 0, :, 0] == 0).all()


# ---- embed -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("K, C, H, W, Dc", [(512, 1, 16, 16, 64), (64, 4, 8, 8, 32), (65, 4, 2, 3, 5)])
def test_embed_is_a_gather_bit_for_bit(dev, K, C, H, W, Dc, n):
    from ctvae_amd import kernels as Kn
    g = torch.Generator().manual_seed(K + n)
    cb = torch.randn(C, K, Dc, generator=g)
    cb[0, 0, 0], cb[C - 1, K - 1, Dc - 1] = -0.0, float("nan")               # raw words pass
    inds = torch.randint(0, K, (n, C, H, W), generator=g)
    inds[0, C - 1, H - 1, W - 1], inds[0, 0, 0, 0] = K - 1, 0
    want = torch.stack([cb[c][inds[:, c]] for c in range(C)], dim=3).reshape(n, H, W, C * Dc)      # [n, H, W, C, Dc]
    got = Kn.code_prior_embed(inds.to(dev), cb.to(dev))
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, H, W, C * Dc)
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    parts = list(cb.to(dev).unbind(0))                                        # views of one buffer: back to back
    assert torch.equal(Kn.code_prior_embed(inds.to(dev), parts).view(torch.int32), got.view(torch.int32))


def test_decoding_the_embedded_indices_is_the_models_own_reconstruction(dev):
    from ctvae_amd.codeprior import MarkovCodePrior, grid_indices
    from ctvae_amd.models import vae_models
    m = vae_models["MCQVAE"](**{**H.MCQ_CFG, "hidden_dims": list(H.MCQ_CFG["hidden_dims"])})
    m.load_state_dict(filler.fill_state(H.mcq_specs(H.MCQ_CFG), 1321))
    m = m.to(dev).eval()
    x = filler.synthetic_batch(4100, 4)[0].to(dev)
    with torch.no_grad():
        want = m.generate(x)
        inds = grid_indices(m, x)
        prior = MarkovCodePrior(m.num_embeddings, *inds.shape[1:], dev)
        got = prior.decode_samples(m, inds)
    err = (got - want).abs().max().item()
    print(f"decode(embed(inds(x))) against generate(x): max abs err {err:.2e}")
    assert tuple(got.shape) == tuple(want.shape) and err <= 1e-4


# ---- wrappers --------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments_by_name(dev):
    from ctvae_amd import kernels as Kn
    K, C, H, W = 8, 2, 2, 3
    tables, invalid = Kn.code_prior_tables(K, C, H, W, dev)
    totals = Kn.code_prior_totals(tables)
    inds = torch.zeros(2, C, H, W, dtype=torch.int64, device=dev)
    lam = torch.full((C, 5), 0.2, dtype=torch.float64, device=dev)
    u = torch.rand(2, H * W, C, 2, dtype=torch.float64, device=dev)
    cb = torch.zeros(C, K, 4, device=dev)

    def swap(seq, i, t):
        return tuple(t if j == i else s for j, s in enumerate(seq))

    bad = [
        (lambda: Kn.code_prior_count(inds.int(), tables, invalid), "code_prior_count: inds must be a torch.int64"),
        (lambda: Kn.code_prior_count(inds[:, :, :, :2], tables, invalid), "code_prior_count: inds must be contiguous"),
        (lambda: Kn.code_prior_count(inds.cpu(), tables, invalid), "code_prior_count: inds must be a device tensor"),
        (lambda: Kn.code_prior_count(inds[0], tables, invalid), r"code_prior_count: inds must be \[B, C, H, W\]"),
        (lambda: Kn.code_prior_count(inds, tables[:3], invalid), "code_prior_count: tables must be the four tensors"),
        (lambda: Kn.code_prior_count(inds, swap(tables, 1, tables[1][:, :K].contiguous()), invalid),
         r"code_prior_count: left must be \[2, 9, 8\]"),
        (lambda: Kn.code_prior_count(inds, swap(tables, 2, tables[2].int()), invalid), "code_prior_count: up must be a torch.int64"),
        (lambda: Kn.code_prior_count(inds, swap(tables, 3, tables[3].cpu()), invalid), "code_prior_count: prev must be a device"),
        (lambda: Kn.code_prior_count(inds, swap(tables, 0, tables[0][:, :, :0].contiguous()), invalid),
         r"code_prior_count: K must lie in 1\.\.512, got 0"),
        (lambda: Kn.code_prior_count(inds, tables, torch.zeros(2, dtype=torch.int64, device=dev)),
         "code_prior_count: invalid must be one int64 word"),
        (lambda: Kn.code_prior_score(inds, tables, totals[:2], lam), "code_prior_score: totals must be the four tensors"),
        (lambda: Kn.code_prior_score(inds, tables, swap(totals, 0, totals[0].float()), lam),
         "code_prior_score: pos_tot must be a torch.int64"),
        (lambda: Kn.code_prior_score(inds, tables, swap(totals, 1, totals[1][:, :K].contiguous()), lam),
         r"code_prior_score: left_tot must be \[2, 9\]"),
        (lambda: Kn.code_prior_score(inds, tables, swap(totals, 2, torch.full_like(totals[2], 1 << 53)), lam),
         r"code_prior_score: up_tot must lie in \[0, 2\^53\)"),
        (lambda: Kn.code_prior_score(inds, tables, totals, lam.float()), "code_prior_score: lambda must be a torch.float64"),
        (lambda: Kn.code_prior_score(inds, tables, totals, lam[:, :4].contiguous()), r"code_prior_score: lambda must be \[2, 5\]"),
        (lambda: Kn.code_prior_score(inds, tables, totals, lam.cpu()), "code_prior_score: lambda must be a device tensor"),
        (lambda: Kn.code_prior_sample(tables, totals, lam, u.float(), H, W), "code_prior_sample: u must be a torch.float64"),
        (lambda: Kn.code_prior_sample(tables, totals, lam, u[..., :1].contiguous(), H, W),
         r"code_prior_sample: u must be \[n, H\*W, C, 2\]"),
        (lambda: Kn.code_prior_sample(tables, totals, lam, u, W, W), r"code_prior_sample: u must be \[n, H\*W, C, 2\] for H=3"),
        (lambda: Kn.code_prior_sample(tables, totals, lam, u, 0, W), "code_prior_sample: H must be an integer of at least 1"),
        (lambda: Kn.code_prior_sample(tables, totals, lam, u.transpose(0, 1), H, W), "code_prior_sample: u must be contiguous"),
        (lambda: Kn.code_prior_sample(tables, swap(totals, 3, totals[3].cpu()), lam, u, H, W),
         "code_prior_sample: prev_tot must be a device"),
        (lambda: Kn.code_prior_embed(inds, cb.double()), "code_prior_embed: codebooks must be a torch.float32"),
        (lambda: Kn.code_prior_embed(inds, cb[:1]), r"code_prior_embed: codebooks must be \[C=2, K, Dc\]"),
        (lambda: Kn.code_prior_embed(inds, [cb[0], cb[0]]), r"code_prior_embed: codebooks\[1\] must be \[K, Dc\] and stored back"),
        (lambda: Kn.code_prior_embed(inds.float(), cb), "code_prior_embed: inds must be a torch.int64"),
        (lambda: Kn.code_prior_tables(513, 1, 1, 1, dev), r"code_prior_tables: K must lie in 1\.\.512, got 513"),
        (lambda: Kn.code_prior_tables(8, 0, 1, 1, dev), "code_prior_tables: C must be at least 1"),
    ]
    for call, message in bad:
        with pytest.raises(ValueError, match=message):
            call()
    assert not any(int(t.sum()) for t in tables) and int(invalid) == 0      # nothing was launched
