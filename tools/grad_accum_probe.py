"""Kernel cost of gradient accumulation: the three modes of ctvae_grad_accumulate on the optimizer's slice of a real model --
VanillaVAE's whole flat buffer, or CT-MCQ-VAE's ``ct_layer`` slice (configs/ct_mcq_vae.yaml, ``update_parameters``) -- next to
the Adam launch on the same slice, for one kernel trace.

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/grad_accum_probe.py --model vanilla
    python tools/rocpd_export.py OUT/run_results.db > stats.csv
"""
import argparse
import os
import sys

import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=["vanilla", "ct"], default="vanilla")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from ctvae_amd import kernels as K
    from ctvae_amd.models import vae_models
    from ctvae_amd.optim import FlatAdam
    dev = torch.device("cuda")
    torch.manual_seed(0)
    if args.model == "vanilla":
        m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128).to(dev)
        sl = None
    else:
        cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
        m = vae_models[cfg["name"]](**cfg).to(dev)
        sl = m.flat_range("ct_layer")
    opt = FlatAdam(m, lr=1e-3, params_slice=sl, accumulate=2)
    g = m.flat_grads[opt.slice]
    g.normal_()
    for i in range(args.warmup + args.reps):
        for mode in ("store", "add", "finish"):
            K.grad_accumulate(opt.acc, g, mode)
        g.mul_(1.0 / 3.0)                        # "finish" left 3 g: keep the values where they were
        opt.step()
        if i == args.warmup - 1:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    print(f"{args.model}: slice of {g.numel()} floats ({4 * g.numel() / 2 ** 20:.2f} MiB) at float offset {int(opt.slice.start or 0)}, "
          f"{args.warmup + args.reps} launches of every mode", flush=True)


if __name__ == "__main__":
    main()
