"""CPU: the host half of ctvae_amd/causalgraph.py and causal_graph.py (the colour table, result -> summary, refusals) and the
self-checks of the restatements the GPU tests compare against (tests/graph_checks.py)."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from tests import graph_checks as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def test_ref_accumulate_adds_rows_one_at_a_time_in_order():
    """S = 2, G = 3, hand-worked: group 1 gets rows 0 and 2, group 0 row 1, row 3 (group 3) and row 4 (group -1) are skipped.
    1.0 + 2^-53 + 2^-53 is 1.0 when added in this order and 1.0 + 2^-52 in the other: the order is part of the result."""
    tiny = np.float32(2.0 ** -53)
    adj = np.array([[[1.0, 0.5], [0.75, 0.0]],
                    [[0.25, 0.25], [0.25, 0.25]],
                    [[tiny, 0.50000006], [0.5, 1.0]],
                    [[9.0, 9.0], [9.0, 9.0]],
                    [[7.0, 7.0], [7.0, 7.0]]], dtype=np.float32)
    mask = np.array([[1, 0], [0, 0], [1, 1], [1, 1], [1, 1]], dtype=np.float32)
    st = C.ref_accumulate(C.new_state(3, 2), adj, [1, 0, 1, 3, -1], mask)
    assert st["rows"].tolist() == [1, 2, 0] and st["mask_rows"].tolist() == [1, 2, 0] and st["skipped"].tolist() == [2]
    assert st["adj_sum"][1].tolist() == [[1.0 + float(tiny), 0.5 + float(np.float32(0.50000006))], [1.25, 1.0]]
    assert st["adj_sum"][1][0, 0] == 1.0                              # 2^-53 is lost against 1.0 ...
    assert st["adj_sum"][0].tolist() == [[0.25, 0.25], [0.25, 0.25]] and not st["adj_sum"][2].any()
    assert st["edge_count"][1].tolist() == [[1, 1], [1, 1]]           # 0.5 does not count, 0.50000006 does; 0.75 and 1.0 once each
    assert st["edge_count"][0].tolist() == [[0, 0], [0, 0]]
    assert st["mask_sum"].tolist() == [[0.0, 0.0], [2.0, 1.0], [0.0, 0.0]]
    # ... but not against itself: two more rows of 2^-53 FIRST give another sum than the same rows LAST
    a = np.array([[[1.0]], [[tiny]], [[tiny]]], dtype=np.float32)
    first = C.ref_accumulate(C.new_state(1, 1), a[[1, 2, 0]])["adj_sum"][0, 0, 0]
    last = C.ref_accumulate(C.new_state(1, 1), a)["adj_sum"][0, 0, 0]
    assert last == 1.0 and first == 1.0 + 2.0 ** -52
    # a second call goes on from what the first left, a call without a mask leaves the mask words alone
    C.ref_accumulate(st, adj[:1], [1])
    assert st["rows"].tolist() == [1, 3, 0] and st["mask_rows"].tolist() == [1, 2, 0] and st["mask_sum"][1].tolist() == [2.0, 1.0]
    assert st["adj_sum"][1][0, 1] == 0.5 + float(np.float32(0.50000006)) + 0.5
    # group None: everything is group 0
    assert C.ref_accumulate(C.new_state(2, 2), adj)["rows"].tolist() == [5, 0]
    mean, freq, mk = C.result_of(st)
    assert mean[1][1, 0] == 2.0 / 3 and freq[1][0, 0] == 2.0 / 3 and np.isnan(mean[2]).all() and np.isnan(mk[2]).all()
    assert mk[1].tolist() == [1.0, 0.5]


def test_accumulate_inputs_make_the_order_matter():
    adj, group, mask = C.accumulate_inputs(3, 7, 8, 2, groups=[0] * 7)
    fwd = C.ref_accumulate(C.new_state(2, 8), adj, group, mask)
    rev = C.ref_accumulate(C.new_state(2, 8), adj[::-1].copy(), group, mask[::-1].copy())
    assert not np.array_equal(fwd["adj_sum"], rev["adj_sum"]) and np.allclose(fwd["adj_sum"], rev["adj_sum"], rtol=1e-12)
    assert np.array_equal(fwd["edge_count"], rev["edge_count"])
    assert (adj == np.float32(0.5)).sum() > 10 and fwd["edge_count"].sum() == (adj > np.float32(0.5)).sum() > 10


def test_ref_heatmap_bytes_on_a_hand_worked_sheet():
    """Three values of 1 x 2 (cell 2, nrow 2, padding 1): the sheet is 2 x 2 tiles with the fourth empty."""
    table = np.stack([np.arange(256), 255 - np.arange(256), np.full(256, 7)], axis=1).astype(np.uint8)
    v = np.array([[[0.0, 1.0]], [[0.5019, NAN]], [[-3.0, 9.0]]], dtype=np.float32)       # 0.5019*255 + 0.5 = 128.48
    rows = C.ref_heatmap_bytes(v, table, cell=2, nrow=2, padding=1, pad_color=(9, 8, 7))
    assert rows.shape == (2 * 3 + 1, 1 + 3 * (2 * 5 + 1)) and (rows[:, 0] == 0).all()
    img = rows[:, 1:].reshape(7, 11, 3)
    pad = [9, 8, 7]
    assert (img[0] == pad).all() and (img[3] == pad).all() and (img[6] == pad).all() and (img[:, 0] == pad).all()
    assert (img[:, 5] == pad).all() and (img[:, 10] == pad).all()
    assert (img[1:3, 1:3] == table[0]).all() and (img[1:3, 3:5] == table[255]).all()            # tile 0: values 0 and 1
    assert (img[1:3, 6:8] == table[128]).all() and (img[1:3, 8:10] == table[0]).all()           # tile 1: 0.5019 and NaN
    assert (img[4:6, 1:3] == table[0]).all() and (img[4:6, 3:5] == table[255]).all()            # tile 2: below lo, above hi
    assert (img[4:6, 6:10] == pad).all()                                                       # the empty cell
    plain = C.ref_heatmap_bytes(v, table, cell=2, nrow=2, padding=1, pad_color=(9, 8, 7), scanlines=False)
    assert np.array_equal(plain, rows[:, 1:])
    other = C.ref_heatmap_bytes(np.array([[[0.0, 2.0, -0.5]]], dtype=np.float32), table, lo=-1.0, hi=3.0, cell=1, nrow=8, padding=0)
    assert other.shape == (1, 1 + 3 * 3)                            # (v + 1) / 4 * 255 + 0.5 = 64.25, 191.75, 32.375
    assert other[0, 1:].reshape(3, 3).tolist() == table[[64, 191, 32]].tolist()
    with pytest.raises(AssertionError, match="rounding boundary"):
        C.ref_heatmap_bytes(np.array([[[0.5]]], dtype=np.float32), table)                       # 0.5 * 255 + 0.5 = 128 exactly


def test_heat_inputs_keep_their_margin_and_cover_the_edge_cases():
    x = C.heat_inputs(5, (5, 3, 7), lo=-0.25, hi=1.5)
    assert x.dtype == np.float32 and x.shape == (5, 3, 7)
    assert np.isnan(x).sum() >= 3 and (x < -0.25).sum() >= 3 and (x > 1.5).sum() >= 3
    idx = C.table_index(x, -0.25, 1.5)                               # asserts the margin
    assert idx.min() == 0 and idx.max() == 255 and len(np.unique(idx)) > 40


def test_colormap_entries_are_distinct_and_brighten():
    from ctvae_amd import causalgraph
    t = causalgraph.colormap()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert len({tuple(c) for c in t.tolist()}) == 256
    luma = t.astype(np.int64) @ np.array([299, 587, 114])               # ITU-R BT.601, in thousandths
    assert (np.diff(luma) > 0).all()
    assert t[0].tolist() == [0, 0, 0] and t[255].tolist() == [255, 255, 255]
    for i, c in causalgraph.ANCHORS:
        assert t[i].tolist() == list(c)
    assert tuple(causalgraph.PAD_COLOR) not in {tuple(c) for c in t.tolist()}
    assert np.array_equal(causalgraph.colormap(), t)


def _result():
    """G = 5 (A = 4, V = 2), S = 3: group 2 never occurred, group 0 has no mask."""
    mean = np.full((5, 3, 3), NAN)
    freq = np.full((5, 3, 3), NAN)
    mask = np.full((5, 3), NAN)
    mean[0] = [[0.9, 0.1, 0.2], [0.3, 0.8, 0.3], [0.0, 0.05, 0.7]]
    freq[0] = [[1.0, 0.0, 0.0], [0.25, 1.0, 0.25], [0.0, 0.0, 0.5]]
    for g in (1, 3, 4):
        mean[g] = np.arange(9).reshape(3, 3) / 10.0 * (1 if g != 4 else 0)
        freq[g] = (mean[g] > 0.5).astype(np.float64)
        mask[g] = [0.1, 0.7, 0.7] if g == 1 else [0.0, 0.0, 0.0]
    return {"adjacency_mean": mean, "edge_freq": freq, "mask_mean": mask, "rows": np.array([4, 2, 0, 1, 8]), "skipped": 0}


def test_summarize_on_a_hand_made_result():
    from ctvae_amd import causalgraph
    res = causalgraph.summarize(_result(), ["hue", "size"])
    assert list(res) == ["none", "hue_+", "size_+", "hue_-", "size_-"]         # action i: factor i % V, "+" for i < V
    none = res["none"]
    assert none["rows"] == 4 and none["edges"] == 3.0 and none["density"] == 3.0 / 9 and none["mask_node"] is None
    assert none["top_edges"] == [[0, 0, 0.9], [1, 1, 0.8], [2, 2, 0.7], [1, 0, 0.3], [1, 2, 0.3], [0, 2, 0.2], [0, 1, 0.1],
                                 [2, 1, 0.05], [2, 0, 0.0]]                    # all nine: fewer than ten; the tie by (i, j)
    assert res["hue_+"]["rows"] == 2 and res["hue_+"]["edges"] == 3.0 and res["hue_+"]["mask_node"] == 1      # the first of two maxima
    assert res["hue_+"]["top_edges"][0] == [2, 2, 0.8] and len(res["hue_+"]["top_edges"]) == 9
    assert res["size_+"] == {"rows": 0, "edges": None, "density": None, "top_edges": None, "mask_node": None}
    assert res["size_-"]["edges"] == 0.0 and res["size_-"]["density"] == 0.0 and res["size_-"]["mask_node"] == 0
    assert res["size_-"]["top_edges"][0] == [0, 0, 0.0]
    text = json.dumps(res, allow_nan=False)                                     # standard JSON: null, never NaN
    assert json.loads(text)["size_+"]["edges"] is None and "NaN" not in text
    assert list(causalgraph.summarize(_result())) == ["none", "action0_+", "action1_+", "action0_-", "action1_-"]
    big = _result()
    big["adjacency_mean"] = np.tile(np.linspace(0.0, 0.99, 16).reshape(1, 4, 4), (5, 1, 1))
    big["edge_freq"], big["mask_mean"] = np.zeros((5, 4, 4)), np.zeros((5, 4))
    top = causalgraph.summarize(big)["none"]["top_edges"]
    assert len(top) == 10 and top[0][:2] == [3, 3] and top[9][:2] == [1, 2]
    for bad in (["a"], ["a", "b", "c"], []):
        with pytest.raises(ValueError, match="names"):
            causalgraph.summarize(_result(), bad)
    odd = {k: (v[:4] if isinstance(v, np.ndarray) else v) for k, v in _result().items()}
    with pytest.raises(ValueError, match="two directions"):
        causalgraph.summarize(odd)


def test_graph_stats_construction_touches_no_device():
    """Like rollout.ActionHits: the buffer is made by the first update, so building one needs no GPU; using one does."""
    from ctvae_amd import causalgraph
    stats = causalgraph.GraphStats(13, 64, "cuda")
    assert stats._buf is None and (stats.G, stats.S, stats.threshold) == (13, 64, 0.5)
    lay, words = stats._layout()
    assert lay["adj_sum"][0] == 0 and lay["mask_sum"][0] % 2 == 0              # the float64 parts are 8-byte aligned
    assert words == 2 * 13 * 4096 + 2 * 13 * 64 + 13 * 4096 + 13 + 13 + 1
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        causalgraph.GraphStats(13, 64, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stats.update(torch.zeros(2, 64, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        causalgraph.heatmap_u8(torch.zeros(1, 4, 4))
    with pytest.raises(ValueError, match="at least one"):
        causalgraph.GraphStats(0, 64, "cuda")
    assert stats._buf is None


def test_collect_graphs_refuses_other_models():
    from ctvae_amd import causalgraph
    from ctvae_amd.models import vae_models
    vanilla = vae_models["VanillaVAE"](in_channels=3, latent_dim=16)
    with pytest.raises(TypeError, match="VanillaVAE"):
        causalgraph.collect_graphs(vanilla, [])
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
    model = vae_models["CTMCQVAE"](**cfg)
    assert model.ct_layer.graph_observer is None and causalgraph.model_nodes(model) == 64
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        causalgraph.collect_graphs(model, [])
    assert model.ct_layer.graph_observer is None


def test_val_graphs_is_refused_for_a_model_without_graphs():
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    params = {"LR": 0.005, "weight_decay": 0.0, "scheduler_gamma": 0.95, "kld_weight": 0.00025}
    vanilla = vae_models["VanillaVAE"](in_channels=3, latent_dim=16)
    with pytest.raises(ValueError, match="val_graphs needs a CTMCQVAE.*VanillaVAE"):
        VAEXperiment(vanilla, dict(params), val_graphs=True)
    assert VAEXperiment(vanilla, dict(params)).val_graphs is False            # off by default


def _config(tmp_path, name, **trainer):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", name)))
    cfg["trainer_params"].update(trainer)
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    p = tmp_path / name
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def test_command_refuses_with_a_reason(tmp_path):
    from ctvae_amd import causal_graph
    with pytest.raises(SystemExit, match="VanillaVAE.*CTMCQVAE"):
        causal_graph.main(["-c", _config(tmp_path, "vae.yaml")])
    with pytest.raises(SystemExit, match="no checkpoint"):
        causal_graph.main(["-c", _config(tmp_path, "ct_mcq_vae.yaml")])
    missing = str(tmp_path / "missing.ckpt")
    with pytest.raises(SystemExit, match="missing.ckpt does not exist"):
        causal_graph.main(["-c", _config(tmp_path, "ct_mcq_vae.yaml"), "--checkpoint", missing])
    with pytest.raises(SystemExit, match="2 names.*6 factors"):
        causal_graph.main(["-c", _config(tmp_path, "ct_mcq_vae.yaml"), "--checkpoint", missing, "--factor-names", "a,b"])
    assert not os.path.exists(tmp_path / "logs")                    # nothing was written
