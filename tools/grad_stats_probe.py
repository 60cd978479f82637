"""Cost of one gradient-tracking step: the three launches of csrc/gradstat.hip on the optimizer's slice of a
real model -- VanillaVAE's whole flat buffer, or CT-MCQ-VAE's ``ct_layer`` slice at action_dim 12 -- timed by the library's own
event brackets (``native.prof_enable``), and the wall time of a whole ``GradientTracker.measure`` call, which ends in the one
device-to-host copy.

    python tools/grad_stats_probe.py --model vanilla
"""
import argparse
import json
import os
import sys
import time

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["vanilla", "ct"], default="vanilla")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--norm-type", type=float, default=2.0)
    args = ap.parse_args()
    from ctvae_amd import native
    from ctvae_amd.models import vae_models
    from ctvae_amd.optim import FlatAdam, GradientTracker
    dev = torch.device("cuda")
    torch.manual_seed(0)
    if args.model == "vanilla":
        m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128).to(dev)
        sl = None
    else:
        cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
        cfg["action_dim"] = 12
        m = vae_models[cfg["name"]](**cfg).to(dev)
        sl = m.flat_range("ct_layer")
    opt = FlatAdam(m, lr=1e-3, params_slice=sl)
    tr = GradientTracker(opt, norm_type=args.norm_type, watch=True, watch_log_freq=1)
    g = m.flat_grads[opt.slice]
    g.normal_()
    for _ in range(args.warmup):
        tr.measure(1.0, True)
    torch.cuda.synchronize()
    walls = {}
    for hist in (False, True):
        t0 = time.perf_counter()
        for _ in range(args.reps):
            tr.measure(1.0, hist)
        walls[hist] = (time.perf_counter() - t0) / args.reps * 1e3
    native.prof_enable(True)
    try:
        for _ in range(args.reps):
            tr.measure(1.0, True)
        torch.cuda.synchronize()
    finally:
        native.prof_enable(False)
    rep = native.prof_report()
    print(json.dumps({"model": args.model, "slice_floats": g.numel(), "segments": tr.table.nseg, "chunks": tr.table.nchunks,
                      "copy_bytes": 4 * tr.table.raw.numel(), "norm_type": args.norm_type,
                      "kernel_us": {k: round(v["ms"] / v["count"] * 1e3, 2) for k, v in rep.items() if k.startswith("grad_")},
                      "measure_wall_ms_norms": round(walls[False], 4), "measure_wall_ms_norms_hist": round(walls[True], 4)}),
          flush=True)


if __name__ == "__main__":
    main()
