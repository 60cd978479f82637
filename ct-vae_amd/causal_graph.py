"""The graphs a trained CT-MCQ-VAE has learned, per action: ``python -m ctvae_amd.causal_graph -c configs/ct_mcq_vae.yaml``.

Builds the CT-MCQ-VAE of ``model_params`` and loads a checkpoint as every checkpoint command does (``tool.py``), runs the base- and
action-mode batches of the test split through it (``causalgraph.collect_graphs``) and writes under ``--out`` (default
``<save_dir>/<name>/causal_graph``):

* ``graph_adjacency.png``  the mean adjacency of every group that had rows, one tile each: no intervention first, then the actions
* ``graph_edge_freq.png``  the same tiles for the share of graphs whose edge lies above ``--threshold``
* ``graph_mask.png``       the mean intervention mask of every action that had rows, as a picture of the latent grid
* ``causal_graphs.npz``    ``adjacency_mean`` [G,S,S], ``edge_freq`` [G,S,S], ``mask_mean`` [G,S] (float64, NaN for a group without
  rows) and ``rows`` [G]; group 0 is no intervention, group 1 + i action i
* ``causal_graphs.json``   per group (``none``, ``<factor>_<sign>``): rows, mean edges per graph, density, the ten strongest mean
  edges, the node with the largest mean mask (``causalgraph.summarize``)

All pictures map [0, 1] onto ``causalgraph.colormap()``, so they compare across actions and runs.  Factor names: ``--factor-names
a,b,c``, else ``data_params.hbm_factor_names``, else ``action<i>``.  Seeded with ``exp_params.manual_seed``; the torch generators come
back as they were.  ``--ema`` loads the checkpoint's averaged weights (``ema_state_dict``, written under ``exp_params.ema_decay``) in
place of ``state_dict``; a checkpoint without them is refused.  Bad input ends with a SystemExit that says why.
"""
import argparse
import json
import os

from . import causalgraph, rollout, tool
from .evalrun import npz_bytes
from .models.ct_mcq_vae import CTMCQVAE

FILES = ("graph_adjacency.png", "graph_edge_freq.png", "graph_mask.png", "causal_graphs.npz", "causal_graphs.json")
_fail = tool.fail("causal_graph")


def _accept(cls, name):
    if not (isinstance(cls, type) and issubclass(cls, CTMCQVAE)):
        return f"model_params.name is {name!r}: causal graphs exist only in a CTMCQVAE"


def main(argv=None):
    ap = argparse.ArgumentParser(description="the causal graphs a trained CT-MCQ-VAE has learned, per action, as pictures and numbers")
    tool.add_arguments(ap, "causal_graph", 'configs/ct_mcq_vae.yaml')
    ap.add_argument('--factor-names', default=None, help="comma-separated, action_dim / 2 of them")
    ap.add_argument('--threshold', type=float, default=0.5, help="an edge counts when its coefficient lies above it")
    ap.add_argument('--cell', type=int, default=4, help="pixels per matrix element (the mask sheet: four times as many)")
    args = ap.parse_args(argv)
    configured = tool.configure(args, "causal_graph", _accept)
    mp, dp = configured[2:4]
    try:
        names = rollout.configured_factor_names(mp, dp, args.factor_names)
    except ValueError as e:
        _fail(str(e))
    if args.cell < 1:
        _fail(f"--cell must be at least 1, got {args.cell}")
    if not args.threshold == args.threshold:
        _fail("--threshold is not a number")
    model, data, dev, seed, out_dir = tool.load(args, "causal_graph", configured)

    stats = causalgraph.collect_graphs(model, data.test(), seed=seed, threshold=args.threshold)
    res = stats.result()
    seen = [g for g in range(stats.G) if res["rows"][g] > 0]
    masked = [g for g in range(1, stats.G) if res["mask_rows"][g] > 0]
    if not seen:
        _fail("the test split has no base-mode or action-mode batch")
    if not masked:
        _fail("the test split has no action-mode batch")
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
