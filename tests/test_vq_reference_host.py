"""Host: the float64 quantiser reference and the inputs of tests/test_vq_ops_gpu.py, checked without a GPU.

* the reference of tests/vq_checks.py against oracle/vae_cpu.py's mcq_compute_inds / mcq_compute_latents (themselves pinned to
  fixtures captured from the reference project, test_oracle_golden.py);
* for EVERY case of the GPU module, the two conditions its index tests rest on, evaluated on the reference alone: exact data
  has a tied minimum on >= 2 % of the (row, codebook) pairs, and on random data the float64 runner-up lies within the derived
  tolerance on < 1 % of them.  Each test prints its figure (pytest -s / -rP shows them).
"""
import pytest
import torch

from oracle import vae_cpu as O
from tests import vq_checks as V

IND = {c.id: c for c in V.IND_CASES}


def _sd(E):
    return {f"vq_layer.quantizers.{i}.embedding.weight": E[i] for i in range(E.shape[0])}


def _nchw(x, case):
    return x.view(case.B, case.HW, 1, case.D).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("cid", ["reg32-P245-tail5", "generic-C3-Dc7-K37", "generic-K512"])
def test_reference_matches_the_pinned_oracle(cid):
    case = IND[cid]
    # indices: exact data, where the oracle's float32 expanded form is exact and ties are frequent
    x, E = V.exact_inputs(case)
    want = O.mcq_compute_inds(_sd(E), _nchw(x, case), case.C)                       # [B, C, HW, 1]
    got = V.inds_of(V.first_argmin(V.dist64(x, E)), case.B, case.HW)
    assert torch.equal(got, want.reshape(case.B, case.C, case.HW))
    # lookup, loss, gradients: random data, given indices
    x, E = V.random_inputs(case, "o1")
    inds = V.given_inds(case, "uniform")
    g = torch.Generator().manual_seed(5)
    g_q = torch.randn(x.shape, generator=g)
    g_vq = 0.7
    xo = _nchw(x, case).requires_grad_(True)
    Eo = E.clone().requires_grad_(True)
    q, loss = O.mcq_compute_latents(_sd(Eo), xo, inds.view(case.B, case.C, case.HW, 1), case.C, 0.25)
    ((q * _nchw(g_q, case)).sum() + loss * g_vq).backward()
    ref = V.reference64(x, E, inds, 0.25, g_q, g_vq)
    P = case.B * case.HW

    def close(a, b, what):
        s = max(1.0, float(b.abs().max()))
        assert float((a.double() - b).abs().max()) <= 2e-6 * s, what       # float32 rounding of sums of O(1) terms

    close(q.permute(0, 2, 3, 1).reshape(P, case.D).detach(), ref["quantized"], "quantized")
    close(loss.detach(), ref["vq_loss"], "vq_loss")
    close(xo.grad.permute(0, 2, 3, 1).reshape(P, case.D), ref["g_lat"], "latent gradient")
    close(Eo.grad, ref["d_cb"], "codebook gradient")
    assert torch.equal(V.quantized32(x, E, inds), q.permute(0, 2, 3, 1).reshape(P, case.D).detach())


def test_first_argmin_is_the_first_minimum():
    d = torch.tensor([[3.0, 1.0, 1.0, 2.0], [0.0, 0.0, 0.0, 0.0], [5.0, 4.0, 3.0, 3.0]], dtype=torch.float64)
    assert V.first_argmin(d).tolist() == [1, 0, 2]
    assert V.tie_share(d) == 1.0


@pytest.mark.parametrize("case", V.IND_CASES, ids=lambda c: c.id)
def test_exact_inputs_are_exact_and_tie_often(case):
    x, E = V.exact_inputs(case)
    d = V.dist64(x, E)
    assert torch.equal(V.expanded32(x, E).double(), d), "float32 expanded form is not exact on this data"
    assert float(d.max()) < 2 ** 24
    share = V.tie_share(d)
    print(f"{case.id}: tied minimum on {100 * share:.2f} % of {d.shape[0] * d.shape[1]} (row, codebook) pairs")
    if case.K > 1:
        assert share >= 0.02, f"{case.id}: only {100 * share:.2f} % ties: the case does not test the tie rule"


@pytest.mark.parametrize("cid,kind", V.IND_RANDOM, ids=lambda v: v)
def test_random_inputs_leave_the_bound_its_power(cid, kind):
    case = IND[cid]
    x, E = V.random_inputs(case, kind)
    d = V.dist64(x, E)
    tol = V.tol_rows(x, E)
    share = V.runner_up_share(d, tol)
    print(f"{cid}/{kind}: runner-up within tol on {100 * share:.3f} % of {d.shape[0] * d.shape[1]} (row, codebook) pairs")
    assert share < 0.01, f"{cid}/{kind}: {100 * share:.2f} % of the rows would accept the runner-up"
    # torch's float32 expanded form standing in for the kernel: the bound holds for it on every row
    stand_in = V.first_argmin(V.expanded32(x, E).double())
    assert float(V.excess(d, stand_in, tol).max()) <= 0.0


def test_every_random_case_is_a_gpu_case():
    assert {cid for cid, _ in V.IND_RANDOM} == {c.id for c in V.IND_CASES if c.K > 1}
    assert all(kind in V.RANDOM_KINDS for _, kind in V.IND_RANDOM)
    assert {kind for _, kind in V.IND_RANDOM} == set(V.RANDOM_KINDS)


@pytest.mark.parametrize("case", [c for c in V.IND_CASES if c.K > 1 and c.B < 600], ids=lambda c: c.id)
def test_planted_duplicates_tie_exactly(case):
    x, E, planted, want = V.planted_inputs(case)
    pairs = V.duplicate_pairs(case.K)
    assert (0, case.K - 1) in pairs and any(dst - src in (5, 33) for src, dst in pairs)
    if case.K > 130:
        assert (1, 65) in pairs and (2, 130) in pairs
    d = V.dist64(x, E)
    for src, dst in pairs:
        assert torch.equal(d[..., src], d[..., dst])
    assert int(planted.sum()) == (x.shape[0] + 3) // 4
    assert torch.equal(V.first_argmin(d)[planted], want[planted])
    assert float(d[planted].min(-1).values.max()) == 0.0


def test_case_tables_name_the_paths_the_launchers_take():
    for c in V.IND_CASES:
        Dc = c.D // c.C
        assert c.path == ("reg" if c.K <= 64 and Dc in (32, 64, 128) else "generic"), c.id
        assert (f"reg{Dc}" in c.id) == (c.path == "reg"), c.id
    slices = {}
    for c in V.BWD_CASES:
        path, S = V.bwd_path(c.D, c.K, c.C, c.B * c.HW)
        assert path == c.path, c.id
        slices[c.id] = S
    assert slices["pos-P2053-S9"] == 9 and slices["posw-Dc128-P2112-S33"] == 33
    assert slices["scanS2-K512-P2048"] == 2 and slices["scanS5-K200-Dc40-P2600"] == 5 and slices["scanS5-K200-Dc40-P2587"] == 5
    assert {c.path for c in V.BWD_CASES} == set(V.BWD_LABEL)
    for case, _ in V.LOOKUP_CASES:
        assert case.D % case.C == 0 and case.C <= 8
    pd = [case.B * case.HW * case.D for case, _ in V.LOOKUP_CASES]
    assert max(pd) > 262144 and min(pd) < 64 * 256
    assert {case.C for case, _ in V.LOOKUP_CASES} >= {1, 3, 8} and {b for _, b in V.LOOKUP_CASES} == {0.0, 0.25, 1.0}


@pytest.mark.parametrize("case", V.BWD_CASES, ids=lambda c: c.id)
def test_exact_codebook_gradient_is_integer_and_skew_leaves_codes_unused(case):
    x, E = V.exact_inputs(case)
    for kind in ("uniform", "skewed"):
        inds = V.given_inds(case, kind)
        assert int(inds.min()) >= 0 and int(inds.max()) < case.K
        want = V.exact_dcb(case, x, E, inds)
        assert torch.equal(want.float().double(), want)
        if kind == "skewed":
            counts = torch.stack([torch.bincount(r, minlength=case.K) for r in V.rows_of(inds).t()])
            assert int((counts == 0).sum()) > 0 and float(counts.max()) > 0.5 * case.B * case.HW
            assert float(want[counts == 0].abs().max()) == 0.0


@pytest.mark.parametrize("C,Dc", [(1, 16), (3, 7), (8, 5), (8, 8), (4, 2)])
def test_straight_through_sum_and_zero_columns(C, Dc):
    """Pure straight-through (no loss term): column j of the latent gradient is the sum over the codebooks whose slice covers
    it, and columns from C - 1 + Dc on are exactly zero."""
    case = V.Case("st", C * Dc, 11, C, 6, 3, None)
    x, E = V.random_inputs(case, "o1")
    inds = V.given_inds(case, "uniform")
    g_q = torch.randn(x.shape, generator=torch.Generator().manual_seed(C + Dc))
    ref = V.reference64(x, E, inds, 0.25, g_q, None)["g_lat"]
    got = V.straight_through32(g_q, C)
    assert float((got.double() - ref).abs().max()) <= 8 * 2.0 ** -23 * float(ref.abs().max())
    assert float(ref[:, C - 1 + Dc:].abs().sum()) == 0.0 and float(got[:, C - 1 + Dc:].abs().sum()) == 0.0
    if C == 1:
        assert torch.equal(got, g_q)
