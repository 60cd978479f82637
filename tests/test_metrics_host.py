"""CPU: the host side of ctvae_amd/metrics.py -- the factor grid, the random plan, the argument handling of the reference's
Metric / MetricSet, the refusals -- and the numpy restatement of tests/metrics_checks.py on a perfectly factorised code."""
import numpy as np
import pytest

from tests import metrics_checks as C

SIZES = (6, 5, 4)


@pytest.fixture(scope="module")
def M():
    from ctvae_amd import metrics
    return metrics


class _Store:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def test_factor_grid_is_row_major_ravel(M):
    for sizes in [SIZES, (2,), (3, 1, 7), (10, 10, 10, 8, 4, 15)]:
        grid = M.FactorGrid(sizes)
        n = int(np.prod(sizes))
        assert len(grid) == grid.size == n and grid.num_factors == len(sizes)
        idx = np.arange(n)
        pos = grid.idx_to_pos(idx)
        assert np.array_equal(pos, np.stack(np.unravel_index(idx, sizes), axis=-1))
        assert np.array_equal(grid.pos_to_idx(pos), np.ravel_multi_index(tuple(pos.T), sizes))
        assert np.array_equal(grid.pos_to_idx(pos), idx)
        assert grid.pos_to_idx(pos.reshape(n, 1, -1)).shape == (n, 1)
    grid = M.FactorGrid(SIZES)
    with pytest.raises(ValueError):
        grid.pos_to_idx([[6, 0, 0]])
    with pytest.raises(ValueError):
        grid.idx_to_pos([120])
    f = grid.sample_factors(500, np.random.default_rng(3))
    assert f.shape == (500, 3) and f.min() == 0 and (f.max(axis=0) == np.array(SIZES) - 1).all()


def test_factor_data_needs_the_whole_grid(M):
    grid = M.FactorGrid(SIZES)
    assert len(M.FactorData(_Store(120), grid)) == 120
    with pytest.raises(ValueError, match="119"):
        M.FactorData(_Store(119), grid)


def test_draw_plan_is_seeded_and_groups_share_their_fixed_factor(M):
    grid = M.FactorGrid(SIZES)
    a = M.draw_plan("FactorVaeScore", grid, 16, 40, 20, 512, seed=7)
    b = M.draw_plan("FactorVaeScore", grid, 16, 40, 20, 512, seed=7)
    c = M.draw_plan("FactorVaeScore", grid, 16, 40, 20, 512, seed=8)
    assert sorted(a) == ["eval_factor", "eval_rows", "train_factor", "train_rows", "variance_rows"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert any(not np.array_equal(a[k], c[k]) for k in a)
    assert a["variance_rows"].shape == (512,) and a["train_rows"].shape == (40, 16) and a["eval_rows"].shape == (20, 16)
    for stage, groups in (("train", 40), ("eval", 20)):
        rows, fixed = a[stage + "_rows"], a[stage + "_factor"]
        assert rows.dtype == np.int64 and rows.min() >= 0 and rows.max() < 120
        assert fixed.shape == (groups,) and fixed.min() >= 0 and fixed.max() < 3
        pos = grid.idx_to_pos(rows)                                  # [G, 16, 3]
        for g in range(groups):
            assert (pos[g, :, fixed[g]] == pos[g, 0, fixed[g]]).all()
        free = [pos[g, :, k] for g in range(groups) for k in range(3) if k != fixed[g]]
        assert sum(len(set(v.tolist())) > 1 for v in free) > len(free) * 0.9      # the other factors do vary
    assert a["variance_rows"].min() >= 0 and a["variance_rows"].max() < 120
    m = M.draw_plan("MIG", grid, 16, 200, seed=7)
    assert sorted(m) == ["factors", "rows"] and m["factors"].shape == (200, 3)
    assert np.array_equal(m["rows"], np.ravel_multi_index(tuple(m["factors"].T), SIZES))
    assert np.array_equal(m["rows"], M.draw_plan("MIG", grid, 16, 200, seed=7)["rows"])
    import torch
    s0 = torch.get_rng_state()
    M.draw_plan("MIG", grid, 16, 200, seed=9)
    assert torch.equal(s0, torch.get_rng_state())


def test_restatement_on_a_perfectly_factorised_code(M):
    """Column f = factor f (plus one constant column): MIG = 1, both accuracies = 1, three active columns.  Small integers sit ON
    the bin edges, which are exact for them in float32 as in float64 (widths 5/20, 4/20, 3/20 times k round the same way a
    comparison against an integer needs), so the edge-margin condition -- a condition for comparing against float32 kernels --
    is switched off here."""
    grid = M.FactorGrid(SIZES)

    def code(rows):
        pos = grid.idx_to_pos(rows).astype(np.float32)
        return np.concatenate([pos, np.full(pos.shape[:-1] + (1,), 0.5, np.float32)], axis=-1)

    # over the whole grid the factors are exactly independent, so every off-diagonal MI is 0 (a random sample leaves the
    # finite-sample MI between independent factors, about (S1-1)(S2-1)/2N, as the runner-up)
    rows = np.arange(grid.size)
    assert C.ref_mig(code(rows), grid.idx_to_pos(rows), SIZES, margin=None) == pytest.approx(1.0, abs=1e-12)
    plan = M.draw_plan("MIG", grid, 16, 300, seed=1)
    assert 0.9 < C.ref_mig(code(plan["rows"]), plan["factors"], SIZES, margin=None) < 1.0
    plan = M.draw_plan("FactorVaeScore", grid, 16, 40, 20, 512, seed=2)
    res = C.ref_factor_vae(code(plan["variance_rows"]), code(plan["train_rows"]), plan["train_factor"],
                           code(plan["eval_rows"]), plan["eval_factor"], 3)
    assert res == {"factor_vae.train_accuracy": 1.0, "factor_vae.eval_accuracy": 1.0, "factor_vae.num_active_dims": 3}
    dead = np.zeros((512, 4), np.float32)
    assert C.ref_factor_vae(dead, code(plan["train_rows"]), plan["train_factor"], code(plan["eval_rows"]),
                            plan["eval_factor"], 3)["factor_vae.num_active_dims"] == 0


def test_restatement_binning_is_numpy_digitize():
    z, lo, hi, _, bins, _ = C.mi_inputs(320, 10)
    for l in range(z.shape[1]):
        x = z[:, l].astype(np.float64)
        assert np.array_equal(np.digitize(x, np.histogram(x, C.NUM_BINS)[1][:-1]), bins[:, l]), l
    with pytest.raises(AssertionError, match="bin widths of an edge"):
        C.ref_bins(np.array([[0.0], [1.0], [0.25 + 1e-6]], np.float32), [0.0], [1.0])


def test_dci_and_sap_are_refused_by_name(M):
    ds = M.FactorData(_Store(120), M.FactorGrid(SIZES))
    for name, why in (("DCI", "gradient-boosted trees"), ("SAP", "SVM")):
        with pytest.raises(ValueError, match=name) as e:
            M.Metric(name, ds)
        assert why in str(e.value)
        with pytest.raises(ValueError, match=name):
            M.MetricSet(["MIG", name], ds)
    with pytest.raises(ValueError, match="unknown metric"):
        M.Metric("Modularity", ds)
    with pytest.raises(ValueError, match="factor sizes"):
        M.Metric("MIG", M.FactorData(_Store(300), M.FactorGrid((300,))))


def test_argument_handling_follows_the_reference(M):
    ds = M.FactorData(_Store(120), M.FactorGrid(SIZES))
    assert sorted(M.METRICS) == ["", "FactorVaeScore", "MIG"]
    assert M.Metric("MIG", ds).args == {"batch_size": 64, "num_train": 1000}
    assert M.Metric("FactorVaeScore", ds, 16, 320, 160).args == {"batch_size": 16, "num_train": 320, "num_eval": 160,
                                                                "num_variance_estimate": 512}
    none = M.Metric("", ds)
    assert none.metric is None and none.compute(lambda x: x) == {}
    ms = M.MetricSet(["MIG", "FactorVaeScore", ""], ds, batch_size=16, num_train=320, num_test=160, seed=5)
    assert [m.name for m in ms.metrics] == ["MIG", "FactorVaeScore", ""]
    assert ms.metrics[1].args["num_eval"] == 160 and ms.metrics[0].seed == 5
    p = ms.metrics[1].plan()
    assert p["train_rows"].shape == (320, 16) and p["eval_rows"].shape == (160, 16) and p["variance_rows"].shape == (512,)
    assert not np.array_equal(p["train_rows"], ms.metrics[1].plan(seed=6)["train_rows"])


def test_codes_must_be_on_the_device(M):
    import torch
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.column_moments(torch.zeros(4, 4))


def test_library_exports_the_metric_kernels():
    from ctvae_amd.build import build
    build()
    from ctvae_amd import native
    lib = native.load()
    for name in ("ctvae_column_moments", "ctvae_mi_matrix", "ctvae_group_var_argmin"):
        assert name in native.SIGNATURES and hasattr(lib, name)
    # a bad argument is refused on the host, before anything touches a device
    assert lib.ctvae_column_moments(None, 4, 4, None, None, None, None, None) == -22
