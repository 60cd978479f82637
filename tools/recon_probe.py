"""Cost of the reconstruction statistics (exp_params.recon_stats) on one MI355X.  One process measures one thing,
so that configurations can be alternated as separate processes:

* ``--launches``: the per-launch event time (the library's own event pairs, ``prof_report``) of ``recon_record_kernel``,
  ``recon_select_kernel`` and ``recon_gather_kernel`` at B = 64 and 256 (3 x 64 x 64 pictures, K = 8), next to the empty event pair;
* ``--val MODEL --bs N [--recon]``: the time per validation step of VanillaVAE or MCQVAE through ``VAEXperiment.fit`` -- no training
  batches, ``--steps`` validation batches behind ``--warmup`` more -- from device events recorded between the batches (a validation
  step ends with the device-to-host copy of its scalars, so the span between two events is one whole step); ``--recon`` sets
  ``recon_stats: true`` (K = 8).  ``--tree DIR`` imports the package from another checkout (the parent commit's, which has no
  ``--recon``).

Prints one JSON line.

    python tools/recon_probe.py --launches
    python tools/recon_probe.py --val VanillaVAE --bs 64 --recon
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def launch_times(dev, launches, reps):
    from ctvae_amd import native
    from ctvae_amd.reconstats import ReconStats
    out, empty = {}, []
    for B in (64, 256):
        target = torch.rand(B, 3, 64, 64, device=dev).contiguous(memory_format=torch.channels_last)
        recons = (target + 0.1 * torch.randn_like(target)).contiguous(memory_format=torch.channels_last)
        acc = ReconStats(dev, 1.0, 8)
        acc.reset()
        for _ in range(20):
            acc.observe(recons, target)
        torch.cuda.synchronize()
        us = {"recon_record_kernel": [], "recon_select_kernel": [], "recon_gather_kernel": []}
        for _ in range(reps):
            acc.reset()
            native.prof_enable(True)
            try:
                for _ in range(launches):
                    acc.observe(recons, target)
                native.prof_calibrate(64)
                torch.cuda.synchronize()
            finally:
                native.prof_enable(False)
            rep = native.prof_report()
            for k in us:
                us[k].append(rep[k]["ms"] * 1e3 / rep[k]["count"])
            cal = rep.get("(empty event pair)")
            if cal:
                empty.append(cal["ms"] * 1e3 / cal["count"])
        out[f"B{B}"] = {k: spread(v) for k, v in us.items()}
    out["empty_event_pair_us"] = spread(empty) if empty else None
    return out


def val_step_times(dev, model_name, bs, recon, steps, warmup):
    from ctvae_amd import filler, specs
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    params = {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 0.00025, "manual_seed": 1265}
    if recon:
        params.update(recon_stats=True, recon_stats_worst=8)
    if model_name == "VanillaVAE":
        m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
        m.load_state_dict(filler.fill_state(specs.vanilla_specs(), 1266))
    else:
        cfg = {**specs.MCQ_CFG, "hidden_dims": list(specs.MCQ_CFG["hidden_dims"])}
        m = vae_models["MCQVAE"](**cfg)
        m.load_state_dict(filler.fill_state(specs.mcq_specs(specs.MCQ_CFG), 1321))
    exp = VAEXperiment(m.to(dev).train(), params)
    val = [(filler.synthetic_batch(1265 + i, bs)[0].to(dev), torch.zeros(bs, device=dev)) for i in range(4)]
    n = warmup + steps
    events = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]

    def batches():
        for i in range(n):
            events[i].record()
            yield val[i % 4]
        events[n].record()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = exp.fit(lambda: iter([]), batches, max_epochs=1)[0]
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    ms = [events[i].elapsed_time(events[i + 1]) for i in range(warmup, n)]
    return {"model": model_name, "bs": bs, "recon": bool(recon), "step_ms": spread(ms), "epoch_wall_s": wall,
            "val_recon_rows": rec.get("val_recon_rows")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--val", default=None, choices=["VanillaVAE", "MCQVAE"])
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--recon", action="store_true")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    if not torch.cuda.is_available():
        raise SystemExit("recon_probe measures on the GPU: no device found")
    dev = torch.device("cuda")
    if args.launches:
        res = {"launch_us": launch_times(dev, 200, args.reps)}
    elif args.val:
        res = val_step_times(dev, args.val, args.bs, args.recon, args.steps, args.warmup)
    else:
        raise SystemExit("recon_probe: give --launches or --val MODEL")
    if args.tag:
        res["tag"] = args.tag
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
