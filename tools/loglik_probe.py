"""Cost of the importance-sampled log-likelihood (loglik.py, csrc/loglik.hip), in one process on one MI355X:

* ``rows_kernel``: the per-launch event time (the library's own event pairs, ``prof_report``) of ``loglik_rows_kernel`` at
  ``--rows`` x ``--pixels`` (default 4096 x 12288: 64 images, 64 samples each), behind a warm-up, next to the empty event pair.  The
  launches rotate over ``--buffers`` decoded-row tensors (default 4 x 201 MB), more than the 256 MiB Infinity Cache holds, so the
  rows come from HBM; ``bytes`` = 4 R P + 4 B P and ``share_of_hbm_peak`` counts them against the 6.29 TB/s a float4 copy reaches;
* ``torch_float64_us``: a plain-torch float64 restatement of the same reduction on the same tensors (device events), for context;
* ``latent_us`` / ``merge_us``: the other two launches of a chunk at the same R, with L = ``--latent``;
* ``val_step_s`` (``--val``): the validation step of VanillaVAE at bs = 64 through ``VAEXperiment.validation_step`` inside an armed
  ``_validate`` -- ``--batches`` validation batches, no training batches -- with the ``exp_params`` given as JSON in ``--exp``
  (``{}``: the key off): per-batch host time of an epoch that ends in a device synchronise.  One process measures one setting;
  a driver alternates processes (and trees) and takes the median of their medians;
* ``tool_s`` (``--tool CKPT_DIR``): the wall time of ``python -m ctvae_amd.log_likelihood`` in this process at its default K over
  ``--tool-rows`` rows of the synthetic test split, host clock around ``main``.

Prints one JSON object: medians with the min .. max spread over the rounds.

    python tools/loglik_probe.py [--val --exp JSON] [--tool DIR] [--out FILE]
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
HBM_PEAK = 6.29e12


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def event_us(fn, reps, launches=1):
    us = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for j in range(launches):
            fn(j)
        b.record()
        torch.cuda.synchronize()
        if i:
            us.append(a.elapsed_time(b) * 1e3 / launches)
    return spread(us)


def rows_kernel(dev, B, S, P, L, buffers, reps):
    from ctvae_amd import kernels as K, native
    R = B * S
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(B, 3, P // 3, 1, generator=g, device=dev)
    xhats = [x.repeat_interleave(S, 0) + 0.1 * torch.randn(R, 3, P // 3, 1, generator=g, device=dev) for _ in range(buffers)]
    a = torch.randn(R, generator=g, device=dev, dtype=torch.float64)
    consts = K.loglik_consts(0.5, P, dev)
    for xh in xhats:
        K.loglik_rows(xh, x, S, a, consts)
    torch.cuda.synchronize()
    us, empty = [], []
    for _ in range(reps):
        native.prof_enable(True)
        try:
            for xh in xhats:
                K.loglik_rows(xh, x, S, a, consts)
            native.prof_calibrate(64)
            torch.cuda.synchronize()
        finally:
            native.prof_enable(False)
        rep = native.prof_report()
        k = rep["loglik_rows_kernel"]
        us.append(k["ms"] * 1e3 / k["count"])
        cal = rep.get("(empty event pair)")
        if cal:
            empty.append(cal["ms"] * 1e3 / cal["count"])
    nbytes = 4.0 * R * P + 4.0 * B * P
    out = {"shape": [R, P, S], "kernel_us": spread(us), "empty_event_pair_us": spread(empty) if empty else None, "bytes": nbytes,
           "buffers": buffers}
    t = out["kernel_us"]["median"] * 1e-6
    out["bytes_per_s"] = nbytes / t
    out["share_of_hbm_peak"] = nbytes / t / HBM_PEAK

    def restated(j):
        d = xhats[j % buffers].double().reshape(B, S, P) - x.double().reshape(B, 1, P)
        return (d * d).sum(2)

    restated(0)
    out["torch_float64_us"] = event_us(restated, reps, launches=buffers)
    mu, lv = torch.randn(B, L, generator=g, device=dev), torch.randn(B, L, generator=g, device=dev)
    eps = torch.randn(B, S, L, generator=g, device=dev)
    lw = K.loglik_rows(xhats[0], x, S, a, consts)
    state, flags = K.loglik_state(B, dev)
    out["latent_us"] = event_us(lambda j: K.loglik_latent(mu, lv, eps), reps, launches=20)
    out["merge_us"] = event_us(lambda j: K.loglik_merge(lw, S, state, flags, 0), reps, launches=20)
    return out


def val_step_times(dev, bs, batches, reps, exp_params):
    """Per-batch host time of a validation epoch (``batches`` steps and what the armed reports write behind them)."""
    from ctvae_amd import filler, specs
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    params = {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 0.00025, "manual_seed": 1265}
    val = [(filler.synthetic_batch(1265 + i, bs)[0].to(dev), torch.zeros(bs, device=dev)) for i in range(4)]
    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
    m.load_state_dict(filler.fill_state(specs.vanilla_specs(), 1266))
    exp = VAEXperiment(m.to(dev).train(), dict(params, **exp_params))

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        exp.fit(lambda: iter([]), lambda: (val[i % 4] for i in range(batches)), max_epochs=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / batches

    run()
    out = spread([run() for _ in range(reps)])
    out.update(batches=batches, bs=bs, exp_params=exp_params)
    return out


def tool_time(dev, ckpt_dir, rows, bs):
    """The command at its defaults over ``rows`` synthetic test rows: a checkpoint of filler weights, vae.yaml with
    ``val_batch_size: bs``, and -- here only -- a synthetic split of ``rows / bs`` batches in place of its 8."""
    import yaml
    from ctvae_amd import filler, log_likelihood, specs, tool
    from ctvae_amd.run import SyntheticData
    tool.SyntheticData = lambda *a, **k: SyntheticData(*a, steps_per_epoch=(rows + bs - 1) // bs, **k)
    os.makedirs(ckpt_dir, exist_ok=True)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "vae.yaml")))
    cfg["data_params"]["val_batch_size"] = bs
    cfg["logging_params"]["save_dir"] = os.path.join(ckpt_dir, "logs")
    cfg_path = os.path.join(ckpt_dir, "vae.yaml")
    with open(cfg_path, "w") as f:
        yaml.safe_dump(cfg, f)
    ckpt = os.path.join(ckpt_dir, "filler.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in filler.fill_state(specs.vanilla_specs(), 1266).items()}, "epoch": 0}, ckpt)
    argv = ["-c", cfg_path, "--checkpoint", ckpt, "--out", os.path.join(ckpt_dir, "out"), "--rows", str(rows)]
    log_likelihood.main(argv + ["--samples", "8"])                          # warm-up: code objects, the data
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    summary = log_likelihood.main(argv)
    torch.cuda.synchronize()
    return {"seconds": time.perf_counter() - t0, "rows": summary["rows"], "samples": summary["samples"], "chunk": summary["chunk"],
            "sigma_source": summary["sigma_source"], "bs": bs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--pixels", type=int, default=12288)
    ap.add_argument("--latent", type=int, default=128)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--val", action="store_true")
    ap.add_argument("--exp", default="{}", help="exp_params of the --val run, as JSON")
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--batches", type=int, default=50)
    ap.add_argument("--tool", default=None, metavar="DIR", help="time the command; DIR takes its checkpoint, config and output")
    ap.add_argument("--tool-rows", type=int, default=4096)
    ap.add_argument("--tool-bs", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loglik_probe measures on the GPU: no device found")
    dev = torch.device("cuda")
    res = {}
    if not args.no_kernels:
        res["rows_kernel"] = rows_kernel(dev, args.images, args.chunk, args.pixels, args.latent, args.buffers, args.reps)
    if args.val:
        res["val_step_s"] = val_step_times(dev, args.bs, args.batches, args.reps, json.loads(args.exp))
    if args.tool:
        res["tool_s"] = tool_time(dev, args.tool, args.tool_rows, args.tool_bs)
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
