"""The graphs a trained CT-MCQ-VAE has learned, per action: ``python -m ctvae_amd.causal_graph -c configs/ct_mcq_vae.yaml``.

Builds the CT-MCQ-VAE of ``model_params`` and loads a checkpoint the way ``apply_action.py`` does, runs the base- and action-mode
batches of the test split through it (``causalgraph.collect_graphs``) and writes under ``--out`` (default
``<save_dir>/<name>/causal_graph``):

* ``graph_adjacency.png``  the mean adjacency of every group that had rows, one tile each: no intervention first, then the actions
* ``graph_edge_freq.png``  the same tiles for the share of graphs whose edge lies above ``--threshold``
* ``graph_mask.png``       the mean intervention mask of every action that had rows, as a picture of the latent grid
* ``causal_graphs.npz``    ``adjacency_mean`` [G,S,S], ``edge_freq`` [G,S,S], ``mask_mean`` [G,S] (float64, NaN for a group without
  rows) and ``rows`` [G]; group 0 is no intervention, group 1 + i action i
* ``causal_graphs.json``   per group (``none``, ``<factor>_<sign>``): rows, mean edges per graph, density, the ten strongest mean
  edges, the node with the largest mean mask (``causalgraph.summarize``)

All pictures map [0, 1] onto ``causalgraph.colormap()``, so they compare across actions and runs.  Factor names: ``--factor-names
a,b,c``, else ``data_params.hbm_factor_names``, else ``action<i>``.  Seeded with ``exp_params.manual_seed``.  ``--ema`` loads the
checkpoint's averaged weights (``ema_state_dict``, written under ``exp_params.ema_decay``) in place of ``state_dict``; a checkpoint
without them is refused.  Bad input ends with a SystemExit that says why.
"""
import argparse
import io
import json
import os
import zipfile

import numpy as np
import torch
import yaml

FILES = ("graph_adjacency.png", "graph_edge_freq.png", "graph_mask.png", "causal_graphs.npz", "causal_graphs.json")


def _fail(msg: str):
    raise SystemExit(f"causal_graph: {msg}")


def npz_bytes(arrays: dict) -> bytes:
    """An uncompressed ``.npz`` (``np.load`` reads it) whose bytes depend on the arrays alone: ``np.savez`` stamps every member
    with the current time."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for k, v in arrays.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.ascontiguousarray(v), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), member.getvalue())
    return buf.getvalue()


def main(argv=None):
    ap = argparse.ArgumentParser(description="the causal graphs a trained CT-MCQ-VAE has learned, per action, as pictures and numbers")
    ap.add_argument('--config', '-c', dest="filename", metavar='FILE', default='configs/ct_mcq_vae.yaml')
    ap.add_argument('--checkpoint', default=None, help="default: trainer_params.resume_from_checkpoint")
    ap.add_argument('--out', default=None, help="default: <save_dir>/<name>/causal_graph")
    ap.add_argument('--factor-names', default=None, help="comma-separated, action_dim / 2 of them")
    ap.add_argument('--ema', action='store_true', help="load the checkpoint's averaged weights (ema_state_dict) in place of state_dict")
    ap.add_argument('--threshold', type=float, default=0.5, help="an edge counts when its coefficient lies above it")
    ap.add_argument('--cell', type=int, default=4, help="pixels per matrix element (the mask sheet: four times as many)")
    args = ap.parse_args(argv)
    with open(args.filename) as f:
        config = yaml.safe_load(f)

    from .models import vae_models
    from .models.ct_mcq_vae import CTMCQVAE
    mp = dict(config['model_params'])
    cls = vae_models.get(mp.get('name'))
    if cls is None or not (isinstance(cls, type) and issubclass(cls, CTMCQVAE)):
        _fail(f"model_params.name is {mp.get('name')!r}: causal graphs exist only in a CTMCQVAE")
    A = int(mp.get('action_dim', 0))
    if A < 2 or A % 2:
        _fail(f"model_params.action_dim must be even and at least 2, got {mp.get('action_dim')!r}")
    dp, tp, lp = config.get('data_params', {}), config.get('trainer_params', {}) or {}, config.get('logging_params', {}) or {}
    if args.factor_names is not None:
        names, src = [n.strip() for n in args.factor_names.split(",")], "--factor-names"
    else:
        names, src = dp.get('hbm_factor_names'), "data_params.hbm_factor_names"
    if names is not None and len(names) != A // 2:
        _fail(f"{src} has {len(names)} names, but action_dim {A} means {A // 2} factors")
    ckpt_path = args.checkpoint or tp.get('resume_from_checkpoint')
    if not ckpt_path:
        _fail("no checkpoint: give --checkpoint or set trainer_params.resume_from_checkpoint")
    if not os.path.isfile(ckpt_path):
        _fail(f"checkpoint {ckpt_path} does not exist")
    if args.cell < 1:
        _fail(f"--cell must be at least 1, got {args.cell}")
    if not args.threshold == args.threshold:
        _fail("--threshold is not a number")
    ckpt = None
    if args.ema:          # (asked for by name: a checkpoint without the average is refused before anything is built)
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        if 'ema_state_dict' not in ckpt:
            _fail(f"--ema: checkpoint {ckpt_path} holds no ema_state_dict (it was written without exp_params.ema_decay)")
    if not torch.cuda.is_available():
        _fail("ctvae_amd runs on MI355X GPUs only: the hot path has no CPU fallback")

    from . import causalgraph
    from .run import HbmData, SyntheticData
    dev = torch.device("cuda", torch.cuda.current_device())
    seed = int(config.get('exp_params', {}).get('manual_seed', 0) or 0)
    torch.manual_seed(seed)
    model = cls(**mp).to(dev)
    if ckpt is None:
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
    weights = ckpt['ema_state_dict' if args.ema else 'state_dict']
    model.load_state_dict({k[6:]: v for k, v in weights.items() if k.startswith("model.")}, strict=True)
    data = HbmData(dp, mp, dev, 0, 1, seed) if dp.get('hbm_images') else SyntheticData(dp, mp, dev, 0, 1, seed=seed)

    stats = causalgraph.collect_graphs(model, data.test(), seed=seed, threshold=args.threshold)
    res = stats.result()
    seen = [g for g in range(stats.G) if res["rows"][g] > 0]
    masked = [g for g in range(1, stats.G) if res["mask_rows"][g] > 0]
    if not seen:
        _fail("the test split has no base-mode or action-mode batch")
    if not masked:
        _fail("the test split has no action-mode batch")
    out_dir = args.out or os.path.join(lp.get('save_dir', 'logs/'), lp.get('name', mp['name']), "causal_graph")
    os.makedirs(out_dir, exist_ok=True)

    h, w = res["hw"]
    causalgraph.save_heatmaps(res["adjacency_mean"][seen], os.path.join(out_dir, "graph_adjacency.png"), cell=args.cell)
    causalgraph.save_heatmaps(res["edge_freq"][seen], os.path.join(out_dir, "graph_edge_freq.png"), cell=args.cell)
    causalgraph.save_heatmaps(res["mask_mean"][masked].reshape(len(masked), h, w), os.path.join(out_dir, "graph_mask.png"),
                              cell=4 * args.cell)
    with open(os.path.join(out_dir, "causal_graphs.npz"), "wb") as f:
        f.write(npz_bytes({k: res[k] for k in ("adjacency_mean", "edge_freq", "mask_mean", "rows")}))
    summary = causalgraph.summarize(res, names)
    with open(os.path.join(out_dir, "causal_graphs.json"), "w") as f:
        json.dump(summary, f, indent=1, allow_nan=False)
        f.write("\n")
    return summary


if __name__ == "__main__":
    main()
