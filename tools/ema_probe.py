"""Cost of the weight average (exp_params.ema_decay), in one process on one MI355X:

* the VanillaVAE training step through the harness (``VAEXperiment.fit``, hipGraph on) at bs = 64 and bs = 256, with and without
  ``ema_decay``: host clock around ``--steps`` steps that end in a device synchronise, the two variants alternating, ``--reps``
  rounds behind a warm-up round that also captures the graphs;
* the per-launch event time of ``ema_update`` next to a ``grad_accumulate`` "add" launch on the same n -- both read two vectors
  and write one, 12 B per element, with the same access pattern, so that launch is the yardstick -- and of ``buffer_swap``
  (16 B per element), from the library's own event pairs (``prof_report``), alternating, ``--reps`` rounds of ``--launches``.

Prints one JSON object: medians with the min .. max spread over the rounds.

    python tools/ema_probe.py [--out FILE]
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


def step_times(dev, bs, steps, reps):
    from ctvae_amd import filler
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    params = {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 0.00025, "hipgraph": True}
    batches = [(filler.synthetic_batch(1265 + i, bs)[0].to(dev), torch.zeros(bs, device=dev)) for i in range(4)]
    exps = {}
    for name, extra in (("plain", {}), ("ema", {"ema_decay": 0.999})):
        torch.manual_seed(1265)
        m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128).to(dev).train()
        exps[name] = VAEXperiment(m, dict(params, **extra), log_every=10 ** 9)

    def run(exp):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        exp.fit(lambda: (batches[i % 4] for i in range(steps)), None, max_epochs=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    for exp in exps.values():                       # warm-up: the eager steps, the capture, replays
        run(exp)
    ms = {name: [] for name in exps}
    for _ in range(reps):
        for name, exp in exps.items():
            ms[name].append(run(exp))
    out = {name: spread(v) for name, v in ms.items()}
    out["ema_minus_plain_ms"] = spread([a - b for a, b in zip(ms["ema"], ms["plain"])])
    out["n_floats"] = int(exps["ema"].ema.buffer.numel())
    return out


def launch_times(dev, launches, reps):
    from ctvae_amd import kernels as K
    from ctvae_amd import native
    from ctvae_amd.models import vae_models
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128).to(dev)
    p = m.flat_params
    p.normal_()
    ema, acc = K.grad_accumulator_like(p), K.grad_accumulator_like(p)
    ema.normal_()                                   # ("add" grows acc by p every launch: zeroed between rounds, it stays finite)
    kinds = {"ema_update": lambda: K.ema_update(ema, p, 0.001),
             "grad_accumulate_add": lambda: K.grad_accumulate(acc, p, "add"),
             "buffer_swap": lambda: K.buffer_swap(ema, acc)}
    names = {"ema_update": "ema_update_kernel", "grad_accumulate_add": "grad_accumulate_kernel", "buffer_swap": "buffer_swap_kernel"}
    for f in kinds.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    us = {k: [] for k in kinds}
    empty = []
    for _ in range(reps):
        for k, f in kinds.items():
            native.prof_enable(True)
            try:
                for _ in range(launches):
                    f()
                native.prof_calibrate(64)
                torch.cuda.synchronize()
            finally:
                native.prof_enable(False)
            rep = native.prof_report()
            us[k].append(rep[names[k]]["ms"] * 1e3 / rep[names[k]]["count"])
            cal = rep.get("(empty event pair)")
            if cal:
                empty.append(cal["ms"] * 1e3 / cal["count"])
        acc.zero_()
    n = p.numel()
    out = {k: dict(spread(v), bytes_per_launch=(16 if k == "buffer_swap" else 12) * n) for k, v in us.items()}
    out["empty_event_pair_us"] = spread(empty) if empty else None
    out["ema_over_add"] = spread([a / b for a, b in zip(us["ema_update"], us["grad_accumulate_add"])])
    out["n_floats"] = int(n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ema_probe measures on the GPU: no device found")
    dev = torch.device("cuda")
    res = {"launch_us": launch_times(dev, args.launches, args.reps)}
    for bs in (64, 256):
        res[f"step_ms_bs{bs}"] = step_times(dev, bs, args.steps, args.reps)
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
