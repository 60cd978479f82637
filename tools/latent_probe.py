"""Cost of the latent statistics (exp_params.latent_stats), in one process on one MI355X:

* ``launch_us``: the per-launch event time (the library's own event pairs, ``prof_report``) of ``ctvae_latent_accumulate`` at
  (B, L) = (64, 128) and (256, 128), on the column halves of a [B, 2L] heads tensor as the harness hands them over, next to the
  empty event pair;
* ``val_epoch_s``: the validation epoch of VanillaVAE (configs/vae.yaml's model) at bs = 64 through ``VAEXperiment.fit`` --
  ``--batches`` validation batches, no training batches -- with the key on and off, the two alternating, host clock around a run
  that ends in a device synchronise, ``--reps`` rounds behind a warm-up round.  The key's share includes the one device-to-host
  copy and the host summary at the epoch's end (no ``sample_dir``: no files).

Prints one JSON object: medians with the min .. max spread over the rounds.

    python tools/latent_probe.py [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def launch_times(dev, shapes, launches, reps):
    from ctvae_amd import native
    from ctvae_amd.latentstats import LatentStats
    out, empty = {}, []
    for B, L in shapes:
        heads = torch.randn(B, 2 * L, device=dev)
        mu, lv = heads[:, :L], heads[:, L:]
        stats = LatentStats(L, dev)
        stats.zero()
        for _ in range(20):
            stats.observe(mu, lv)
        torch.cuda.synchronize()
        us = []
        for _ in range(reps):
            stats.zero()
            native.prof_enable(True)
            try:
                for _ in range(launches):
                    stats.observe(mu, lv)
                native.prof_calibrate(64)
                torch.cuda.synchronize()
            finally:
                native.prof_enable(False)
            rep = native.prof_report()
            k = rep["latent_accumulate_kernel"]
            us.append(k["ms"] * 1e3 / k["count"])
            cal = rep.get("(empty event pair)")
            if cal:
                empty.append(cal["ms"] * 1e3 / cal["count"])
        out[f"B{B}_L{L}"] = spread(us)
    out["empty_event_pair_us"] = spread(empty) if empty else None
    return out


def val_epoch_times(dev, bs, batches, reps):
    from ctvae_amd import filler, specs
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    params = {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 0.00025, "manual_seed": 1265}
    val = [(filler.synthetic_batch(1265 + i, bs)[0].to(dev), torch.zeros(bs, device=dev)) for i in range(4)]
    exps = {}
    for name, extra in (("off", {}), ("on", {"latent_stats": True})):
        m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
        m.load_state_dict(filler.fill_state(specs.vanilla_specs(), 1266))
        exps[name] = VAEXperiment(m.to(dev).train(), dict(params, **extra))

    def run(exp):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        exp.fit(lambda: iter([]), lambda: (val[i % 4] for i in range(batches)), max_epochs=1)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for exp in exps.values():
        run(exp)
    s = {name: [] for name in exps}
    for _ in range(reps):
        for name, exp in exps.items():
            s[name].append(run(exp))
    out = {name: spread(v) for name, v in s.items()}
    out["on_minus_off_s"] = spread([a - b for a, b in zip(s["on"], s["off"])])
    out["batches"], out["bs"] = batches, bs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("latent_probe measures on the GPU: no device found")
    dev = torch.device("cuda")
    res = {"launch_us": launch_times(dev, ((64, 128), (256, 128)), args.launches, args.reps),
           "val_epoch_s": val_epoch_times(dev, args.bs, args.batches, args.reps)}
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
