"""Cost of codebook usage counting and of a restart step (exp_params.codebook_restart_every), in one process on
one MI355X: the MCQVAE training step of configs/mcq_vae.yaml at bs = 256 through the harness (``VAEXperiment.fit``, hipGraph on)
under three settings --

* ``plain``: without the key;
* ``counting``: ``codebook_restart_every`` so large that no restart falls into the run -- the usage and pool-fill launches ride
  inside the captured step;
* ``restarting``: ``codebook_restart_every: 1`` with a ``codebook_restart_min_count`` no code reaches, so that EVERY step is
  followed by a restart of all C * K = 256 codes (the collective-free single-GPU form: one device-to-host copy, the draw, one
  upload of the list, one launch).  ``restarting`` minus ``counting`` is the cost of one restart step at its largest.

Host clock around ``--steps`` steps that end in a device synchronise, the three variants alternating, ``--reps`` rounds behind a
warm-up round that also captures the graphs.  In front of that, the per-launch event time of the forward's one launch at the
step's shape (``launch_times``).  Prints one JSON object: medians with the min .. max spread over the rounds.

    python tools/codebook_probe.py [--out FILE]
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
    from ctvae_amd import filler, specs
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    params = {"LR": 0.0005, "weight_decay": 0.0, "kld_weight": 0.00025, "manual_seed": 1320, "hipgraph": True}
    batches = [(filler.synthetic_batch(1320 + i, bs)[0].to(dev), torch.zeros(bs, device=dev)) for i in range(4)]
    variants = (("plain", {}), ("counting", {"codebook_restart_every": 10 ** 9}),
                ("restarting", {"codebook_restart_every": 1, "codebook_restart_min_count": 10 ** 9}))
    exps = {}
    for name, extra in variants:
        cfg = specs.MCQ_CFG
        m = vae_models["MCQVAE"](**{**cfg, "hidden_dims": list(cfg["hidden_dims"])})
        m.load_state_dict(filler.fill_state(specs.mcq_specs(cfg), 1321))
        exps[name] = VAEXperiment(m.to(dev).train(), dict(params, **extra), log_every=10 ** 9)

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
    out["counting_minus_plain_ms"] = spread([a - b for a, b in zip(ms["counting"], ms["plain"])])
    out["restart_step_ms"] = spread([a - b for a, b in zip(ms["restarting"], ms["counting"])])
    out["codes_restarted_per_step"] = exps["restarting"].codebook_restarted // max(exps["restarting"].codebook_ordinal, 1)
    out["indices_per_step"] = bs * cfg["codebooks"] * 64
    return out


def launch_times(dev, bs, launches, reps):
    """Per-launch event time (the library's own event pairs, ``prof_report``) of the training forward's one launch at the step's
    shape, for three index tensors: the model's own (its first forward: whatever collapse the weights have), uniform random
    codes, and one code for all (worst-case contention)."""
    from ctvae_amd import filler, kernels as K, native, specs
    from ctvae_amd.models import vae_models
    cfg = specs.MCQ_CFG
    m = vae_models["MCQVAE"](**{**cfg, "hidden_dims": list(cfg["hidden_dims"])})
    m.load_state_dict(filler.fill_state(specs.mcq_specs(cfg), 1321))
    m = m.to(dev)
    with torch.no_grad():
        lat = K.to_nhwc(m.encode(filler.synthetic_batch(1320, bs)[0].to(dev))[0]).contiguous()
        own = m.vq_layer.compute_inds(K.to_nchw_view(lat))
    C, Kc = cfg["codebooks"], cfg["num_embeddings"]
    kinds = {"model": own, "uniform": torch.randint(0, Kc, own.shape, device=dev), "one_code": torch.zeros_like(own)}
    words = torch.zeros(C * Kc + 1, dtype=torch.int64, device=dev)
    counts, invalid = words[:-1].view(C, Kc), words[-1:]
    pool = torch.zeros((1024, lat.size(-1)), device=dev)
    calls = {k: (lambda t=t: K.vq_usage_pool_fill(t, counts, invalid, lat, pool)) for k, t in kinds.items()}
    calls["usage_alone_model"] = lambda: K.vq_usage(own, counts, invalid)
    calls["pool_fill_alone"] = lambda: K.vq_pool_fill(lat, pool)
    names = {k: "vq_usage_fill_kernel" for k in kinds}
    names.update(usage_alone_model="vq_usage_kernel", pool_fill_alone="vq_pool_fill_kernel")
    for f in calls.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    us, empty = {k: [] for k in calls}, []
    for _ in range(reps):
        for k, f in calls.items():
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
    out = {k: spread(v) for k, v in us.items()}
    out["empty_event_pair_us"] = spread(empty) if empty else None
    out["indices"] = int(own.numel())
    out["pool_bytes"] = int(min(lat.numel() // lat.size(-1), 1024) * lat.size(-1) * 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("codebook_probe measures on the GPU: no device found")
    res = {f"launch_us_bs{args.bs}": launch_times(torch.device("cuda"), args.bs, args.launches, args.reps),
           f"step_ms_bs{args.bs}": step_times(torch.device("cuda"), args.bs, args.steps, args.reps)}
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
