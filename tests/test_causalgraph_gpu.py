"""GPU: ctvae_amd/causalgraph.py, the graph_observer hook, exp_params.val_graphs and the causal_graph command on the filler
CT-MCQ-VAE (action_dim 4, batches of 8, synthetic transition data): the accumulated graphs against a plain Python observer and
the numpy restatement, that the calling run does not notice any of it, the pictures, and the command end to end."""
import io
import json
import os

import numpy as np
import pytest
import torch
import yaml

from ctvae_amd import filler
from tests import graph_checks as C
from tests import grid_checks as G
from tests import helpers as H
from tests.test_ct_gpu import _FixedNoise, build_ct

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, S = 4, 8, 64
PARAMS = {"LR": 5e-4, "weight_decay": 0.0, "scheduler_gamma": 0.99, "kld_weight": 0.00025, "update_parameters": "ct_layer",
          "manual_seed": 7}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", torch.cuda.current_device())


@pytest.fixture(scope="module")
def noise(dev):
    """One deterministic noise source for the whole module: the same model call draws the same noise whoever makes it."""
    from ctvae_amd.models import causal
    prev = causal.set_noise_source(_FixedNoise(dev))
    yield
    causal.set_noise_source(prev)


def _batches(dev, base, n):
    """n transition batches, modes base / action / causal in turn, the actions shuffled per batch."""
    out = []
    for i in range(n):
        x, y, a = filler.synthetic_pairs(base + i, B, A)
        a = a[torch.randperm(B, generator=torch.Generator().manual_seed(base + i))]
        mode = ["base", "action", "causal"][i % 3]
        opts = {"mode": [mode] * B}
        if mode != "base":
            opts.update(input_y=y.to(dev), action=a.to(dev))
        out.append((x.to(dev), torch.zeros(B, device=dev), opts))
    return out


@pytest.fixture(scope="module")
def model(dev, noise):
    return build_ct(dev, 5, action_dim=A)


@pytest.fixture(scope="module")
def batches(dev):
    return _batches(dev, 500, 6)


class _Recorder:
    """A plain Python observer: copies what it is shown to the host."""

    def __init__(self):
        self.calls = []

    def __call__(self, adj, mask, group, hw):
        self.calls.append((adj.detach().cpu().numpy().copy(), None if mask is None else mask.detach().cpu().numpy().copy(),
                           None if group is None else group.detach().cpu().numpy().copy(), tuple(hw),
                           adj.dtype, None if group is None else group.dtype))


def _png(path):
    with open(path, "rb") as f:
        img, kinds = G.read_png(f.read())
    assert kinds == ["IHDR", "IDAT", "IEND"]
    return img


def test_collect_graphs_equals_a_plain_observer(model, batches, dev):
    """The same batches under eval + no_grad with a recording observer, its rows fed to ref_accumulate one call at a time: the
    means of collect_graphs are the restatement's, exactly.  The causal-mode batches show the observer nothing."""
    from ctvae_amd import causalgraph
    stats = causalgraph.collect_graphs(model, iter(batches))
    assert model.ct_layer.graph_observer is None and model.training
    res = stats.result()
    rec = _Recorder()
    model.ct_layer.graph_observer = rec
    try:
        model.eval()
        with torch.no_grad():
            for x, lab, opts in batches:
                model(x, labels=lab, **opts)
    finally:
        model.ct_layer.graph_observer = None
        model.train()
    assert len(rec.calls) == 4                                       # 2 base + 2 action batches; the 2 causal ones: nothing
    state = C.new_state(A + 1, S)
    for (adj, mask, group, hw, adt, gdt), (x, lab, opts) in zip(rec.calls, [b for b in batches if b[2]["mode"][0] != "causal"]):
        assert adj.shape == (B, S, S) and adt == torch.float32 and hw == (8, 8)
        if opts["mode"][0] == "base":
            assert mask is None and group is None
        else:
            assert mask.shape == (B, S) and gdt == torch.int32 and mask.min() > -1e-6 and mask.max() < 1 + 1e-6
            assert group.tolist() == (opts["action"].argmax(dim=-1) + 1).tolist()
        C.ref_accumulate(state, adj, group, mask)
    mean, freq, mk = C.result_of(state)
    print("rows", res["rows"].tolist(), "edges per graph", [float(np.nansum(f)) for f in freq])
    assert res["rows"].tolist() == state["rows"].tolist() and res["rows"].sum() == 4 * B and res["rows"][0] == 2 * B
    assert res["mask_rows"].tolist() == state["mask_rows"].tolist() and res["mask_rows"][0] == 0 and res["skipped"] == 0
    assert np.array_equal(res["adjacency_mean"], mean, equal_nan=True)
    assert np.array_equal(res["edge_freq"], freq, equal_nan=True)
    assert np.array_equal(res["mask_mean"], mk, equal_nan=True)
    assert np.isfinite(res["adjacency_mean"]).all() and np.isnan(res["mask_mean"][0]).all() and res["hw"] == (8, 8)
    assert (res["adjacency_mean"] > 0).all() and (res["adjacency_mean"] < 1).all()            # sigmoid outputs
    # the per-action graphs are not one graph: the discoverers differ
    assert not np.array_equal(res["adjacency_mean"][1], res["adjacency_mean"][2])
    # the model's own batch mean is the mean of what the observer saw (float32, so not to the bit)
    model.ct_layer.graph_observer = rec
    try:
        model.eval()
        with torch.no_grad():
            out = model(batches[1][0], labels=batches[1][1], **batches[1][2])
    finally:
        model.ct_layer.graph_observer = None
        model.train()
    np.testing.assert_allclose(out[4]["ct_adjacency"].cpu().numpy(), rec.calls[-1][0].mean(axis=0), rtol=0, atol=1e-6)
    np.testing.assert_allclose(out[4]["ct_mask"].cpu().numpy().reshape(-1), rec.calls[-1][1].mean(axis=0), rtol=0, atol=1e-6)


def test_collect_graphs_leaves_the_run_as_found(dev, noise, batches):
    from ctvae_amd import causalgraph
    from ctvae_amd import kernels as K
    m = build_ct(dev, 5, action_dim=A)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    flags = [mod.training for mod in m.modules()]
    cpu_rng, dev_rng, epoch = torch.get_rng_state(), torch.cuda.get_rng_state(dev), K._param_epoch[0]
    stats = causalgraph.collect_graphs(m, iter(batches))
    assert stats.result()["rows"].sum() == 4 * B
    assert m.training and [mod.training for mod in m.modules()] == flags and m.ct_layer.graph_observer is None
    after = m.state_dict()
    assert after.keys() == state.keys()
    for k in state:
        assert torch.equal(after[k], state[k]), k
    assert torch.equal(torch.get_rng_state(), cpu_rng) and torch.equal(torch.cuda.get_rng_state(dev), dev_rng)
    assert K._param_epoch[0] == epoch

    def boom(*a):
        raise ValueError("observer failed")
    m.ct_layer.graph_observer = boom                                # a caller's own observer comes back, also after an error
    with pytest.raises(TypeError, match="NoneType|callable|observer"):
        causalgraph.collect_graphs(m, iter([(None, None, {"mode": ["base"]})]))
    assert m.ct_layer.graph_observer is boom and m.training


def _fit(dev, sample_dir, val_graphs, log=None):
    from ctvae_amd.experiment import VAEXperiment
    train, val = _batches(dev, 600, 6), _batches(dev, 700, 3)
    m = build_ct(dev, 5, action_dim=A)
    exp = VAEXperiment(m, dict(PARAMS), sample_dir=sample_dir, run_name="CT", log_file=log, val_graphs=val_graphs)
    hist = exp.fit(lambda: iter(train), lambda: iter(val), max_epochs=2)
    torch.cuda.synchronize()
    return exp, hist, val


def test_fit_with_val_graphs_writes_the_sheets_and_changes_nothing(dev, noise, tmp_path):
    from ctvae_amd import causalgraph, imagegrid
    log = io.StringIO()
    off_exp, off_hist, _ = _fit(dev, str(tmp_path / "off"), False)
    on_exp, on_hist, val = _fit(dev, str(tmp_path / "on"), True, log)
    assert not os.path.exists(tmp_path / "off")                     # a run without the key has no Graphs/ directory
    assert torch.isfinite(on_exp.model.flat_params).all()
    assert torch.equal(on_exp.model.flat_params, off_exp.model.flat_params)
    for k, v in on_exp.model.state_dict().items():
        assert torch.equal(v, off_exp.model.state_dict()[k]), k
    extra = [k for k in on_hist[0] if k.startswith("val_graph_edges_")]
    strip = lambda recs: [{k: v for k, v in r.items() if k != "epoch_seconds" and k not in extra} for r in recs]      # noqa: E731
    assert strip(on_hist) == strip(off_hist) and not any(k.startswith("val_graph") for k in off_hist[0])
    assert on_exp.model.ct_layer.graph_observer is None
    # the validation split has one base and one action batch of 8 rows: its actions are those of that batch
    acts = sorted(set(val[1][2]["action"].argmax(dim=-1).tolist()))
    keys = causalgraph.group_keys(A + 1)
    assert sorted(extra) == sorted("val_graph_edges_" + keys[g] for g in [0] + [1 + a for a in acts])
    assert sorted(os.listdir(tmp_path / "on")) == ["Graphs"]
    assert sorted(os.listdir(tmp_path / "on" / "Graphs")) == ["adjacency_CT_Epoch_0.png", "adjacency_CT_Epoch_1.png",
                                                              "mask_CT_Epoch_0.png", "mask_CT_Epoch_1.png"]
    # the last epoch's sheets: the trained model, unchanged since, over the validation batches again
    res = causalgraph.collect_graphs(on_exp.model, iter(val)).result()
    seen = [g for g in range(A + 1) if res["rows"][g] > 0]
    assert seen == [0] + [1 + a for a in acts]
    summary = causalgraph.summarize(res)
    for g in seen:
        assert on_hist[1]["val_graph_edges_" + keys[g]] == summary[keys[g]]["edges"]
    lines = [json.loads(l) for l in log.getvalue().splitlines()]
    graph_lines = [l for l in lines if any(k.startswith("val_graph_edges_") for k in l)]
    assert len(graph_lines) == 2 and graph_lines[1] == {**{k: on_hist[1][k] for k in extra}, "step": 12}
    table = causalgraph.colormap()
    for e in (0, 1):
        adj_png, mask_png = _png(tmp_path / "on" / "Graphs" / f"adjacency_CT_Epoch_{e}.png"), _png(tmp_path / "on" / "Graphs" / f"mask_CT_Epoch_{e}.png")
        _, _, Hg, Wg = imagegrid.grid_geometry(len(seen), S * 4, S * 4, 8, 2)
        assert adj_png.shape == (Hg, Wg, 3)
        _, _, Hg, Wg = imagegrid.grid_geometry(len(acts), 8 * 16, 8 * 16, 8, 2)
        assert mask_png.shape == (Hg, Wg, 3)
    ok, bad, loose = C.sheet_matches(adj_png, res["adjacency_mean"][seen], table, cell=4, nrow=8, padding=2, pad_color=causalgraph.PAD_COLOR)
    print("adjacency sheet: pixels off", bad, "pixels with two admissible colours", loose)
    assert ok and loose < adj_png.shape[0] * adj_png.shape[1] // 100
    ok, bad, loose = C.sheet_matches(mask_png, res["mask_mean"][[1 + a for a in acts]].reshape(-1, 8, 8), table, cell=16, nrow=8,
                                     padding=2, pad_color=causalgraph.PAD_COLOR)
    assert ok, bad
    assert not np.array_equal(_png(tmp_path / "on" / "Graphs" / "adjacency_CT_Epoch_0.png"), adj_png)       # the model moved


def test_causal_graph_command_end_to_end(dev, tmp_path):
    """Synthetic transition data, a checkpoint saved from the filler model: exactly the five files, a second run that writes the
    same bytes, the JSON's keys under --factor-names, and the .npz's arrays as the tiles of the three sheets."""
    from ctvae_amd import causal_graph, causalgraph, imagegrid
    from ctvae_amd.models import vae_models
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))
    cfg["model_params"]["action_dim"] = A
    cfg["data_params"].update(val_batch_size=B, train_batch_size=B)
    cfg["logging_params"]["save_dir"] = str(tmp_path / "logs")
    torch.manual_seed(9)
    m = vae_models["CTMCQVAE"](**dict(cfg["model_params"], hidden_dims=list(cfg["model_params"]["hidden_dims"])))
    m.load_state_dict(filler.fill_state(H.mcq_specs(H.CT_CONV_CFG), 10), strict=False)
    ckpt = tmp_path / "last.ckpt"
    torch.save({"state_dict": {"model." + k: v.detach().cpu().contiguous() for k, v in m.state_dict().items()}, "epoch": 0}, ckpt)
    cfg["trainer_params"]["resume_from_checkpoint"] = str(ckpt)
    path = tmp_path / "ct.yaml"
    path.write_text(yaml.safe_dump(cfg))
    runs = []
    torch.manual_seed(123)
    before = (torch.get_rng_state(), torch.cuda.get_rng_state(dev))
    for out in (None, str(tmp_path / "again")):
        summary = causal_graph.main(["-c", str(path), "--factor-names", "hue,size"] + (["--out", out] if out else []))
        assert torch.equal(torch.get_rng_state(), before[0]) and torch.equal(torch.cuda.get_rng_state(dev), before[1])
        d = out or str(tmp_path / "logs" / "CTMCQVAE" / "causal_graph")
        assert sorted(os.listdir(d)) == sorted(causal_graph.FILES) and len(causal_graph.FILES) == 5
        runs.append({f: open(os.path.join(d, f), "rb").read() for f in causal_graph.FILES})
    assert runs[0] == runs[1]
    res = json.loads(runs[0]["causal_graphs.json"])
    assert res == summary and list(res) == ["none", "hue_+", "size_+", "hue_-", "size_-"]
    for rec in res.values():
        assert set(rec) == {"rows", "edges", "density", "top_edges", "mask_node"}
    # 8 synthetic test batches: 3 base (24 rows in group 0), 3 action (synthetic_pairs gives action b % 4: 6 rows each), 2 causal
    assert [res[k]["rows"] for k in res] == [3 * B, 6, 6, 6, 6]
    assert res["none"]["mask_node"] is None and all(0 <= res[k]["mask_node"] < S for k in list(res)[1:])
    assert len(res["none"]["top_edges"]) == 10 and res["none"]["density"] == res["none"]["edges"] / S ** 2
    npz = np.load(io.BytesIO(runs[0]["causal_graphs.npz"]))
    assert sorted(npz.files) == ["adjacency_mean", "edge_freq", "mask_mean", "rows"]
    assert npz["adjacency_mean"].shape == (5, S, S) and npz["adjacency_mean"].dtype == np.float64 and npz["rows"].tolist() == [24, 6, 6, 6, 6]
    assert res["hue_-"]["top_edges"][0][2] == npz["adjacency_mean"][3].max()
    table, pad = causalgraph.colormap(), causalgraph.PAD_COLOR
    for name, values, cell in (("graph_adjacency.png", npz["adjacency_mean"], 4), ("graph_edge_freq.png", npz["edge_freq"], 4),
                               ("graph_mask.png", npz["mask_mean"][1:].reshape(4, 8, 8), 16)):
        img = _png(os.path.join(d, name))
        _, _, Hg, Wg = imagegrid.grid_geometry(values.shape[0], values.shape[1] * cell, values.shape[2] * cell, 8, 2)
        assert img.shape == (Hg, Wg, 3), name
        ok, bad, loose = C.sheet_matches(img, values, table, cell=cell, nrow=8, padding=2, pad_color=pad)
        print(name, "pixels off", bad, "pixels with two admissible colours", loose)
        assert ok, (name, bad)
    with pytest.raises(SystemExit, match="3 names.*2 factors"):
        causal_graph.main(["-c", str(path), "--factor-names", "a,b,c"])
    with pytest.raises(SystemExit, match="--cell must be at least 1"):
        causal_graph.main(["-c", str(path), "--cell", "0"])


def test_runner_val_graphs_key(dev, tmp_path):
    """exp_params.val_graphs in the runner: Graphs/ with the two sheets of the epoch next to the usual files, the scalars in the
    epoch record and the JSONL log; a model without graphs is refused before anything is written."""
    from ctvae_amd import run
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))
    cfg["model_params"]["action_dim"] = A
    cfg["data_params"].update(train_batch_size=B, val_batch_size=B)
    cfg["exp_params"]["val_graphs"] = True
    cfg["logging_params"]["save_dir"] = str(tmp_path / "ct")
    p = tmp_path / "ct.yaml"
    p.write_text(yaml.safe_dump(cfg))
    hist = run.main(["-c", str(p), "--steps-per-epoch", "3", "--max-epochs", "1"])
    log = tmp_path / "ct" / "CTMCQVAE"
    assert sorted(os.listdir(log)) == ["Graphs", "checkpoints", "metrics_rank0.jsonl"]
    assert sorted(os.listdir(log / "Graphs")) == ["adjacency_CTMCQVAE_Epoch_0.png", "mask_CTMCQVAE_Epoch_0.png"]
    # three validation batches of 8: one base, one action (synthetic_pairs: actions 0..3 twice each), one causal
    edges = {k: v for k, v in hist[0].items() if k.startswith("val_graph_edges_")}
    assert sorted(edges) == sorted("val_graph_edges_" + k for k in ("none", "action0_+", "action1_+", "action0_-", "action1_-"))
    assert all(0.0 <= v <= S * S for v in edges.values())
    assert _png(log / "Graphs" / "adjacency_CTMCQVAE_Epoch_0.png").shape == (258 + 2, 5 * 258 + 2, 3)
    assert _png(log / "Graphs" / "mask_CTMCQVAE_Epoch_0.png").shape == (130 + 2, 4 * 130 + 2, 3)
    lines = [json.loads(l) for l in open(log / "metrics_rank0.jsonl")]
    assert [l for l in lines if "val_graph_edges_none" in l] == [{**edges, "step": 3}]
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "vae.yaml")))
    cfg["exp_params"]["val_graphs"] = True
    cfg["trainer_params"].update(gpus=[0])
    cfg["logging_params"]["save_dir"] = str(tmp_path / "vanilla")
    p = tmp_path / "vae.yaml"
    p.write_text(yaml.safe_dump(cfg))
    with pytest.raises(SystemExit, match="val_graphs needs a CTMCQVAE.*VanillaVAE"):
        run.main(["-c", str(p), "--max-epochs", "1", "--steps-per-epoch", "1"])
    assert not os.path.exists(tmp_path / "vanilla")
