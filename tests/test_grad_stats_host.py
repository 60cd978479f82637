"""CPU: the host side of gradient tracking (trainer_params.track_grad_norm, exp_params.watch_gradients) -- the settings'
validators, ``FlatParamMixin.grad_segments`` on three models that never see a GPU, the segment table's chunk list, and the
numpy restatement of ``torch.histc``'s bin rule that the histogram kernel is tested against."""
import math
import os

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- settings ----------------------------------------------------------------------------------------------
def test_track_grad_norm_accepts_lightnings_values():
    from ctvae_amd.optim import grad_norm_key, track_grad_norm_setting
    assert track_grad_norm_setting(None) is None and track_grad_norm_setting(-1) is None
    assert track_grad_norm_setting(2) == 2.0 and isinstance(track_grad_norm_setting(2), float)
    assert track_grad_norm_setting(1) == 1.0 and track_grad_norm_setting(3.5) == 3.5 and track_grad_norm_setting(0.5) == 0.5
    assert track_grad_norm_setting("inf") == math.inf and track_grad_norm_setting(math.inf) == math.inf
    assert grad_norm_key(2) == "grad_2.0_norm" and grad_norm_key(math.inf) == "grad_inf_norm"


@pytest.mark.parametrize("bad", [True, False, 0, 0.0, -2, -0.5, "2", "Inf", "two", math.nan, [2], {"p": 2}])
def test_track_grad_norm_refuses_by_name(bad):
    from ctvae_amd.optim import track_grad_norm_setting
    with pytest.raises(ValueError, match="track_grad_norm"):
        track_grad_norm_setting(bad)


def test_watch_settings():
    from ctvae_amd.optim import watch_settings
    assert watch_settings(None) == (False, 500) and watch_settings(True) == (True, 500)
    assert watch_settings(True, 7) == (True, 7) and watch_settings(False, 1) == (False, 1)
    for bad in (1, "true", 0.0):
        with pytest.raises(ValueError, match="watch_gradients"):
            watch_settings(bad)
    for bad in (0, -3, 2.0, True, "500"):
        with pytest.raises(ValueError, match="watch_log_freq"):
            watch_settings(True, bad)


def test_runner_validators_exit_naming_the_key():
    from ctvae_amd import run
    assert run.trainer_track_grad_norm({}) is None and run.trainer_track_grad_norm({"track_grad_norm": "inf"}) == math.inf
    for bad in (0, True, -3, "l2"):
        with pytest.raises(SystemExit, match="trainer_params.track_grad_norm"):
            run.trainer_track_grad_norm({"track_grad_norm": bad})
    assert run.exp_watch_gradients({}) == (False, 500)
    with pytest.raises(SystemExit, match="exp_params.watch_log_freq"):
        run.exp_watch_gradients({"watch_gradients": True, "watch_log_freq": 0})
    with pytest.raises(SystemExit, match="exp_params.watch_gradients"):
        run.exp_watch_gradients({"watch_gradients": "yes"})


# ---- grad_segments -----------------------------------------------------------------------------------------
def _models():
    from ctvae_amd.models import vae_models
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
    cfg["action_dim"] = 12
    torch.manual_seed(3)
    return {"vanilla": lambda: vae_models["VanillaVAE"](in_channels=3, latent_dim=128),
            "joint": lambda: vae_models["JointVAE"](in_channels=3, latent_dim=128, categorical_dim=40),
            "ct": lambda: vae_models["CTMCQVAE"](**cfg)}


@pytest.fixture(scope="module", params=["vanilla", "joint", "ct"])
def model(request):
    return request.param, _models()[request.param]()


def _elements(desc):
    base, rows, period, col_lo, width = desc
    r = torch.arange(rows).reshape(-1, 1)
    c = torch.arange(width).reshape(1, -1)
    return (base + r * period + col_lo + c).reshape(-1)


def test_names_are_the_named_parameters_exactly_once(model):
    _, m = model
    segs = m.grad_segments()
    assert sorted(s[0] for s in segs) == sorted(n for n, _ in m.named_parameters())
    assert len({s[0] for s in segs}) == len(segs)


def test_segments_gather_each_parameters_gradient_and_are_disjoint(model):
    """arange written into the flat gradient buffer: gathering by a descriptor gives the same multiset of values as the
    parameter's .grad view, no element belongs to two segments, and every element outside all segments is an alignment gap or
    a padding row (no parameter's .grad holds it)."""
    _, m = model
    flat = m.flat_grads
    n = flat.numel()
    assert n < 2 ** 24                                   # arange stays exact in fp32
    with torch.no_grad():
        flat.copy_(torch.arange(n, dtype=torch.float32))
    owner = torch.zeros(n, dtype=torch.int32)
    params = dict(m.named_parameters())
    for name, *desc in m.grad_segments():
        idx = _elements(desc)
        assert int(idx.min()) >= 0 and int(idx.max()) < n
        assert idx.numel() == params[name].numel(), name
        got = flat[idx].sort().values
        want = params[name].grad.detach().reshape(-1).sort().values
        assert torch.equal(got, want), name
        owner[idx] += 1
    assert int(owner.max()) == 1, "two segments share an element"
    in_views = torch.zeros(n, dtype=torch.bool)
    for p in m.parameters():
        in_views[p.grad.detach().reshape(-1).long()] = True
    assert torch.equal(in_views, owner.bool()), "a segment holds a gap or padding element, or misses a gradient element"


def test_shapes_the_issue_names(model):
    name, m = model
    segs = {s[0]: s[1:] for s in m.grad_segments()}
    if name == "vanilla":
        mu, var = segs["fc_mu.weight"], segs["fc_var.weight"]
        assert mu[0] == var[0] and mu[1:3] == var[1:3] == (2048, 256)          # one block, rows of 256
        assert (mu[3], mu[4], var[3], var[4]) == (0, 128, 128, 128)           # neighbouring column ranges
        assert segs["fc_mu.bias"][1] == 1 and segs["fc_var.bias"][0] + segs["fc_var.bias"][3] == segs["fc_mu.bias"][0] + 128
    elif name == "joint":
        w, b = segs["decoder_input.weight"], segs["decoder_input.bias"]
        assert (w[1], w[4]) == (1, 168 * 2048)                                 # the 24 padding rows are left out ...
        assert b[0] - w[0] == 192 * 2048                                       # ... of a block that has them
    else:
        assert any(k.startswith("ct_layer.graph_discovers.") for k in segs) and "ct_layer.mask.0.weight" in segs
        assert all(s[1] == 1 for k, s in segs.items() if k.startswith("ct_layer."))


def test_segment_table_chunk_list_on_the_cpu(model):
    from ctvae_amd import kernels as K
    _, m = model
    segs = [s[1:] for s in m.grad_segments()]
    table = K.GradSegmentTable(segs, m.flat_params.numel(), "cpu", nflags=5, guard=4)
    chunk = table.chunk
    assert chunk >= 256 and table.nseg == len(segs)
    begin = table.seg_chunk_begin.tolist()
    assert begin[0] == 0 and begin[-1] == table.nchunks
    for s, (_, rows, _, _, width) in enumerate(segs):
        ks = range(begin[s], begin[s + 1])
        assert len(ks) == -(-rows * width // chunk) >= 1
        assert table.chunk_seg[ks.start:ks.stop].tolist() == [s] * len(ks)
        assert table.chunk_first[ks.start:ks.stop].tolist() == [i * chunk for i in range(len(ks))]
    assert table.out_sum.shape == (len(segs), 2) and table.out_sum.dtype == torch.float64
    assert table.out_hist.shape == (len(segs), 64) and table.out_flags.numel() == 5 and table.guards_intact()
    table.raw[0] = 0
    assert not table.guards_intact()


def test_segment_table_refuses_bad_segments():
    from ctvae_amd import kernels as K
    ok = [(0, 4, 8, 0, 4), (0, 4, 8, 4, 4), (32, 1, 10, 0, 10)]
    K.GradSegmentTable(ok, 42, "cpu")
    for bad in ([(0, 4, 8, 0, 5), (0, 4, 8, 4, 4)],           # column ranges overlap
                [(0, 1, 10, 0, 10), (9, 1, 4, 0, 4)],          # ranges overlap
                [(40, 1, 4, 0, 4)],                            # leaves the buffer
                [(0, 2, 4, 2, 4)],                             # columns wider than the period
                [(-1, 1, 4, 0, 4)], [(0, 0, 4, 0, 4)], []):
        with pytest.raises(ValueError, match="segment"):
            K.GradSegmentTable(bad, 42, "cpu")


def test_launches_need_a_gpu():
    from ctvae_amd import kernels as K
    table = K.GradSegmentTable([(0, 1, 8, 0, 8)], 8, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.grad_segment_stats(table, torch.zeros(8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        K.grad_segment_hist(table, torch.zeros(8))


# ---- the bin rule ------------------------------------------------------------------------------------------
def _histc_cases():
    rng = np.random.default_rng(20261019)
    sizes = [1, 2, 3, 63, 64, 65, 1000, 4097, 100003]
    for i in range(140):
        n = sizes[i % len(sizes)] if i < 36 else int(rng.integers(1, 100004))
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6)).astype(np.float32)
        if i % 3 == 0:
            v[rng.random(n) < 1 / 3] = 0.0
        if i % 7 == 0:
            v = np.abs(v)
        yield v


def test_numpy_bin_rule_agrees_with_torch_histc():
    """140 random arrays, n = 1 to 100003, a third of them with a third of the entries set to zero: the bin of every value by
    ``optim.histc_bins`` (the reference of the GPU tests) gives torch.histc's counts on the CPU."""
    from ctvae_amd.optim import histc_bins
    cases = mismatches = 0
    for v in _histc_cases():
        lo, hi = float(v.min()), float(v.max())
        want = torch.histc(torch.from_numpy(v), bins=64, min=lo, max=hi).numpy().astype(np.int64)
        got = np.bincount(histc_bins(v, lo, hi), minlength=64)
        assert got.sum() == v.size
        mismatches += int(not np.array_equal(got, want))
        cases += 1
    assert cases == 140 and mismatches == 0, mismatches


def test_numpy_bin_rule_edges():
    from ctvae_amd.optim import histc_bins
    assert histc_bins(np.array([0.375] * 5, np.float32), 0.375, 0.375).tolist() == [32] * 5           # widened to [-0.625, 1.375]
    assert histc_bins(np.array([0.0, -0.0], np.float32), 0.0, 0.0).tolist() == [32, 32]
    assert histc_bins(np.array([1.0, 2.0, 3.0], np.float32), 1.0, 3.0).tolist() == [0, 32, 63]        # the maximum: last bin
    big = np.float32(3.4028235e38)
    assert histc_bins(np.array([-big, 0.0, big], np.float32), -big, big).tolist() == [0, 0, 0]        # hi - lo overflows
    want = torch.histc(torch.tensor([0.375] * 5), bins=64, min=0.375, max=0.375)
    assert int(want[32]) == 5
