#!/usr/bin/env python3
"""Benchmark of the hot path: one VanillaVAE training step (forward + loss + backward + gradient
all-reduce (N>1) + Adam) on synthetic 64x64x3 batches, one process per GPU.

    python bench.py --gpus 1 --steps 50 --warmup 10 [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

Workload = the configuration BASELINE.json's metric is quoted on: VanillaVAE, configs/vae.yaml shapes (in_channels 3,
latent_dim 128), per-GPU batch 64, fp32 end to end (parity target 1e-4 forces exact-f32 MFMA).  Inputs are resident in HBM
before the timed region (4 rotating synthetic batches); forward/loss/backward (+Adam at N=1) replay as ONE
hipGraph.  A plain run sets up, warms up, times --steps steps and prints one JSON line (rank 0) with the throughput and
`ms_per_step`.

--full adds what the headline does not need: a `roofline` object for the dominant kernel (HIP-event timed per launch
through the library's own profiler, algorithmic FLOPs from the launch geometry), the per-kernel tables, the bs=256,
MCQ-VAE and CT-MCQ-VAE configurations of BASELINE.json in the line's `configs` array, and a `cpu_baseline` object (the
CPU oracle = pure-torch port of the reference arithmetic, timed on the host cores on a bounded sample).

--dump-outputs DIR writes what the last timed step computed (losses, model outputs, parameters after the optimizer
step, gradients) as DIR/<name>.npy, float32 / float64, at most 64 MB in all (larger arrays as a fixed seeded sample),
so that two builds can be compared output for output on identical inputs.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

FLOP_PER_IMG = {"VanillaVAE": 312_606_720, "MCQVAE": 4_208_984_064,    # SURVEY.md §8d convention (fwd+bwd)
                "CTMCQVAE": 4_932_501_504}                             # action-mode pair, conv path only
PEAK_F32_MFMA_TFLOPS = 157.3                                             # MI355X_MICROARCH.md chip table
PEAK_HBM_GBS = 8000.0
CT_PREFIXES = ("gat_", "pair_mlp", "glinear", "group_rowsum", "ct_")            # kernels of the causal-transition layer
BASELINE_METRIC = "images/sec/GPU fwd+bwd, 64\u00d764\u00d73 bs=64; recon+KL vs CPU ref"   # BASELINE.json "metric", verbatim


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default: 64 VanillaVAE = the metric's own "
                                                             "configuration, 256 MCQVAE, 128 pairs CTMCQVAE)")
    ap.add_argument("--model", default="VanillaVAE", choices=["VanillaVAE", "MCQVAE", "CTMCQVAE"],
                    help="CTMCQVAE: ct_mcq_vae.yaml shapes, action-mode pairs (x, y, one-hot action), eager launches "
                         "(the causal-transition layer has data-dependent host control flow)")
    ap.add_argument("--action-dim", type=int, default=12, help="CTMCQVAE: 12 (TShapes3D, the YAML) or 20 (TCelebA-shaped)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: roofline and per-kernel tables, the `configs` array "
                         "and the CPU baseline (each can still be dropped with its --no-* option)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32/float64, <= 64 MB in all)")
    ap.add_argument("--no-configs", action="store_true", help="skip the `configs` array (bs=64, MCQVAE, CTMCQVAE entries)")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--overlap", action="store_true",
                    help="N>1: cut the backward at the latent (two hipGraphs) and exchange the decoder-side gradient range "
                         "while the encoder's backward runs.  Off by default: measured on MI355X the asynchronous "
                         "collective + second graph cost 0.13 ms per step, more than the ~8 MB exchange they hide")
    ap.add_argument("--split-backward", action="store_true", help="use the two-stage backward even at N=1 (diagnostic)")
    ap.add_argument("--ct-graph", action="store_true", help="(kept for old command lines: CTMCQVAE steps are captured by default now)")
    ap.add_argument("--rehearse-ddp", action="store_true",
                    help="N=1 only: initialise a 1-rank RCCL group and run the exact N>1 step (diagnostic)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--detail", action="store_true", help="per-shape kernel table on stderr (diagnostic)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if not args.full:
        args.no_configs = args.no_cpu_baseline = args.no_roofline = True
    if args.batch is None:
        args.batch = {"VanillaVAE": 64, "MCQVAE": 256, "CTMCQVAE": 128}[args.model]
    return args


def pmc_traffic(kernel_name, workload):
    """HBM-side bytes per launch of `kernel_name` from the newest committed PMC summary OF THIS WORKLOAD that lists it
    (profiles/*_pmc_traffic.json, written by tools/pmc_summary.py from two separate `rocprofv3 --pmc` passes of this same
    command; summaries written before round 3 carry no "workload" key and are VanillaVAE bs=256) or None."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_traffic.json")))
    want = kernel_name.replace(" ", "")
    for path in reversed(files):          # newest summary that holds this kernel (a round re-measures the kernels it changed)
        try:
            with open(path) as f:
                d = json.load(f)
        except (OSError, ValueError):
            continue
        base = os.path.basename(path)
        legacy = "CTMCQVAE bs=128 a12" if "ctmcqvae_a12" in base else "VanillaVAE bs=256"
        if d.get("workload", legacy) != workload:
            continue
        kern = d.get("kernels", {})
        for k, v in kern.items():
            if k.replace(" ", "") == want:
                return v["hbm_bytes_per_launch"], os.path.relpath(path, ROOT)
        # the library's profiler names a kernel without the template arguments its variants carry in the trace
        # (conv_bwd_pair_kernel<false, 1> / <true, 1>): launch-weighted mean over the variants
        var = [v for k, v in kern.items() if "<" not in want and k.split("<")[0] == want]
        if var:
            w = sum(v["launches_per_step"] for v in var)
            return round(sum(v["hbm_bytes_per_launch"] * v["launches_per_step"] for v in var) / max(w, 1e-9)), os.path.relpath(path, ROOT)
    return None, None


def build_model(name, dev, seed, action_dim=12):
    from ctvae_amd import filler
    from ctvae_amd.models import vae_models
    if name == "VanillaVAE":
        m = vae_models[name](in_channels=3, latent_dim=128)
    elif name == "CTMCQVAE":
        import yaml
        cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
        cfg["action_dim"] = action_dim          # 12 = TShapes3D (the YAML), 20 = TCelebA-shaped (BASELINE.json configs[4])
        torch.manual_seed(seed)
        m = vae_models[name](**cfg)
        from ctvae_amd import specs as H
        conv = filler.fill_state(H.mcq_specs(H.CT_CONV_CFG), seed + 1)
        ctl = filler.fill_state(H.ct_layer_specs(action_dim), seed + 3)
        m.load_state_dict({**conv, **{"ct_layer." + k: v for k, v in ctl.items() if k != "pos_encoding.pe"}}, strict=False)
        return m.to(dev).train()
    else:
        m = vae_models[name](in_channels=3, embedding_dim=128, hidden_dims=[64, 128, 256], num_embeddings=64,
                             img_size=64, codebooks=4, beta=0.25)
    m.load_state_dict(filler.fill_state(filler.specs_of(m), seed + 1))
    return m.to(dev).train()


def _with_adam(sd, grads_of, lr):
    """One CPU training step = grads_of(current state) followed by torch.optim.Adam on the float parameters (experiment.py:158)."""
    cur = dict(sd)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()
              if v.is_floating_point() and not k.endswith(("running_mean", "running_var"))}
    opt = torch.optim.Adam(list(leaves.values()), lr=lr)

    def fn():
        for k, g in grads_of(cur).items():
            leaves[k].grad = g
        opt.step()
        cur.update({k: v.detach() for k, v in leaves.items()})
    return fn


def cpu_baseline(model_name, seconds, action_dim=12):
    """Reference arithmetic (the oracle = pure-torch port, pinned by tests/golden/) forward + loss + backward + torch.optim.Adam
    step on the host cores -- the same step contents as the GPU line (experiment.py:44-59,152-160).  VanillaVAE / MCQVAE: the
    metric's own batch (64).  CTMCQVAE: action-mode pairs incl. the causal-transition layer (its GATv2 part is the oracle's
    unpinned restatement), 8 pairs per step -- the pair tensors of the layer are 13 MB per sample -- without the optimizer."""
    from ctvae_amd import filler
    from oracle import vae_cpu as O
    from ctvae_amd import specs as H
    # a one-GPU box grants ~16 host cores to the job; more torch threads than that only oversubscribes
    threads = max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
    torch.set_num_threads(threads)
    unit = "images/s"
    if model_name == "VanillaVAE":
        B = 64
        sd = filler.fill_state(H.vanilla_specs(), 1266)
        x, eps = filler.synthetic_batch(1265, B)
        fn = _with_adam(sd, lambda cur: O.vanilla_step(cur, x, eps, 0.00025)[1], 0.005)
        what = f"VanillaVAE bs={B}"
    elif model_name == "MCQVAE":
        B = 64
        sd = filler.fill_state(H.mcq_specs(H.MCQ_CFG), 1321)
        x, _ = filler.synthetic_batch(1320, B)
        fn = _with_adam(sd, lambda cur: O.mcq_step(cur, x, 4, 0.25)[1], 0.0005)
        what = f"MCQVAE (mcq_vae.yaml) bs={B}"
    else:
        import yaml
        from oracle import causal_cpu as C
        B, A, unit = 8, action_dim, "pairs/s"
        cfg = yaml.safe_load(open(os.path.join(ROOT, "configs", "ct_mcq_vae.yaml")))["model_params"]
        from ctvae_amd.models import vae_models
        torch.manual_seed(1250)
        ref = vae_models["CTMCQVAE"](**{**cfg, "action_dim": A, "hidden_dims": list(cfg["hidden_dims"])})
        sd = {k: v.detach().clone().contiguous() for k, v in ref.state_dict().items()}
        hp = dict(alpha=cfg["c_alpha"], beta=cfg["c_beta"], delta=cfg["c_delta"], epsilon=cfg["c_epsilon"], noise=cfg["noise"])
        mcfg = dict(num_embeddings=64, codebooks=1, beta=cfg["beta"], skip_transition=False)
        x, y, a = filler.synthetic_pairs(1250, B, A)
        ns = H.CTNoise(1250, "cpu")

        def fn():
            ns.reset()
            return C.ctmcq_step(sd, mcfg, cfg["gamma"], x, ns, C.gat_gnn(A + 1), "action", input_y=y, action=a, hp=hp)
        what = f"CTMCQVAE (ct_mcq_vae.yaml, action_dim={A}) action-mode, {B} pairs"
    fn()
    t0 = time.perf_counter()
    n = 0
    while True:
        fn()
        n += 1
        el = time.perf_counter() - t0
        if el >= seconds or n >= 200:
            break
    return {"value": round(n * B / el, 2), "unit": unit, "cores": threads, "kind": "port",
            "sample": f"{n} steps of {what} fwd+loss+bwd{'+Adam' if unit == 'images/s' else ', no optimizer step'} "
                      f"(oracle/, torch CPU fp32, {threads} threads, {el:.1f} s)"}


DUMP_BYTES = 64 * 10 ** 6          # --dump-outputs: all .npy files together, headers included
OUT_NAMES = {"VanillaVAE": ("recons", "input", "mu", "log_var"), "MCQVAE": ("recons", "input", "vq_loss")}


def dump_outputs(out_dir, arrays):
    """Write {name: tensor} as out_dir/<name>.npy (float64 stays float64, other float types become float32; non-float
    tensors are skipped).  When the arrays together exceed DUMP_BYTES, the budget is shared out from the smallest array up
    and an array larger than its share is written as a fixed seeded sample of its flattened elements (sorted indices)."""
    import numpy as np
    arrs = {}
    for name, t in arrays.items():
        if t is None or not t.is_floating_point():
            continue
        a = t.detach().cpu()
        a = a.numpy() if a.dtype == torch.float64 else a.float().numpy()
        arrs[name.replace(os.sep, "_")] = a
    os.makedirs(out_dir, exist_ok=True)
    left = DUMP_BYTES - 256 * len(arrs)                       # npy header: 128 bytes, twice that as margin
    for i, (name, a) in enumerate(sorted(arrs.items(), key=lambda kv: (kv[1].nbytes, kv[0]))):
        share = left // (len(arrs) - i)
        if a.nbytes > share:
            k = max(1, share // a.itemsize)
            idx = np.sort(np.random.default_rng(1265).choice(a.size, size=k, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)
        left -= a.nbytes


class Workload:
    """One benchmark configuration: model, per-GPU batch (images, or (x, y, action) pairs for CTMCQVAE), action_dim."""

    def __init__(self, model, batch, action_dim=12):
        self.model, self.batch, self.action_dim = model, batch, action_dim

    @property
    def unit(self):
        return "pairs/s" if self.model == "CTMCQVAE" else "images/s"

    def label(self, world):
        tail = "fwd+loss+bwd+Adam" + ("+allreduce" if world > 1 else "")
        if self.model == "CTMCQVAE":
            return (f"CTMCQVAE (ct_mcq_vae.yaml, action_dim={self.action_dim}) 64x64x3 action-mode pairs, causal-transition layer "
                    f"included, train step {tail}")
        return f"{self.model} 64x64x3 train step {tail}"


def run_workload(wl, args, ctx, want_kernels=False, dump_dir=None):
    """Build the model of `wl`, capture its step, time exactly args.steps steps (barrier + synchronize on both sides, MAX over
    ranks), -- rank 0 -- write what the last timed step computed to `dump_dir` and time its kernels with HIP events unless
    --no-roofline.  Returns a dict of measurements."""
    from ctvae_amd import filler, native
    from ctvae_amd import kernels as kernels_mod
    from ctvae_amd.ddp import GradBucketAllReduce
    from ctvae_amd.optim import FlatAdam
    rank, world, dev, multi, ddp_on = ctx["rank"], ctx["world"], ctx["dev"], ctx["multi"], ctx["ddp_on"]
    B = wl.batch
    seed = {"VanillaVAE": 1265, "MCQVAE": 1320, "CTMCQVAE": 1250}[wl.model]
    # torch's default generators start from a per-process seed; the model's noise key (VanillaVAE draws it from them at its
    # first forward) is fixed here so that the same arguments give the same computation in every run
    torch.manual_seed(seed + 1000 * rank)
    model = build_model(wl.model, dev, seed, wl.action_dim)
    opt = FlatAdam(model, lr=0.005 if wl.model == "VanillaVAE" else 0.0005)
    ddp = GradBucketAllReduce(model, force=args.rehearse_ddp) if ddp_on else None
    kld_w = 0.00025
    # 4 rotating synthetic batches per rank, resident in HBM, NCHW-contiguous like a DataLoader would hand over
    batches = [filler.synthetic_batch(seed + 1000 * rank + i, B)[0].to(dev) for i in range(4)]
    static_x = kernels_mod.staging_like(batches[0])   # channels_last: the per-step hand-over is the NCHW -> NHWC conversion
    ct_kw = None
    if wl.model == "CTMCQVAE":
        _, y, act = filler.synthetic_pairs(seed + 1000 * rank, B, wl.action_dim)
        ct_kw = {"mode": ["action"] * B, "input_y": y.to(dev), "action": act.to(dev)}
    # --dump-outputs: what the latest step handed back (detached; inside a captured step these are the graph's tensors, which
    # every replay rewrites), the loss terms and the model's outputs.  Without it no reference is held, so that the captured
    # step's memory pool is laid out as it always was
    last = {}

    def keep(losses, out=()):
        if dump_dir is None:
            return
        last.clear()
        last.update({"loss." + k: v.detach() for k, v in losses.items() if torch.is_tensor(v)})
        names = OUT_NAMES.get(wl.model, ())
        last.update({(names[i] if i < len(names) else f"out{i}"): v.detach() for i, v in enumerate(out) if torch.is_tensor(v)})

    def fwd_bwd():
        model.zero_grad(lazy=True)                 # as the harness does (experiment._GraphedTrainStep): no fill launch, first
        out = model(static_x, **ct_kw) if ct_kw is not None else model(static_x)     # writers overwrite their block
        losses = model.loss_function(*out, M_N=kld_w)
        keep(losses, out)
        kernels_mod.backward(losses["loss"])       # loss.backward() with a cached root gradient (as the harness does)
        model.gather_torch_grads()                 # zeros for blocks no kernel wrote + autograd-produced gradients (CT layer) into the
                                                   # flat buffer, INSIDE the captured step (as experiment._GraphedTrainStep does)
        return losses["loss"].detach()

    def local_step():
        l = fwd_bwd()
        if not multi:
            opt.step()
        return l

    # N>1 default: ONE hipGraph (forward + backward), then the stream-ordered all-reduce of the flat gradient buffer, then
    # Adam: +0.012 ms per step over the single-GPU step before any wire time (bench.py --rehearse-ddp).
    # --overlap: the backward pass is cut at the latent (ddp.SplitBackward) and the decoder-side gradient range is
    # all-reduced asynchronously while the encoder's backward (second graph) runs
    split = None
    if wl.model == "VanillaVAE" and ((multi and args.overlap) or args.split_backward):
        from ctvae_amd.ddp import SplitBackward
        split = SplitBackward(model)

    def stage1():
        model.zero_grad()
        losses = split.stage1(static_x, M_N=kld_w)
        keep(losses)
        return losses["loss"].detach()

    graph = graph2 = None
    if not args.no_graph:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        kernels_mod.stage_batch(static_x, batches[0])
        with torch.cuda.stream(s):
            for _ in range(3):
                if split is not None:
                    stage1()
                    split.stage2()
                    if not multi:
                        opt.step()
                else:
                    local_step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        if split is not None:
            with kernels_mod.capture_graph(graph):
                stage1()
            graph2 = torch.cuda.CUDAGraph()
            with kernels_mod.capture_graph(graph2, pool=graph.pool()):
                split.stage2()
                if not multi:
                    opt.step()
        else:
            with kernels_mod.capture_graph(graph):
                local_step()

    def step(i):
        kernels_mod.stage_batch(static_x, batches[i % 4])
        if split is not None:
            if graph is not None:
                graph.replay()
            else:
                stage1()
            works = ddp.all_reduce_range(split.split, split.total) if multi else []
            if graph2 is not None:
                graph2.replay()
            else:
                split.stage2()
                if not multi:
                    opt.step()
            if multi:
                ddp.all_reduce_range(0, split.split, async_op=False)     # nothing left to overlap with
                ddp.wait(works)
                opt.step(grad_scale=ddp.grad_scale)
            return
        if graph is not None:
            graph.replay()
        else:
            local_step()
        if multi:
            ddp.all_reduce()
            opt.step(grad_scale=ddp.grad_scale)

    for i in range(args.warmup):
        step(i)
    torch.cuda.synchronize()
    if multi:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        step(i)
    torch.cuda.synchronize()
    if multi:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if multi:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    res = {"ms_per_step": elapsed / args.steps * 1e3, "value": B * world * args.steps / elapsed, "elapsed": elapsed,
           "hipgraph": graph is not None, "overlap": bool(split is not None and world > 1), "roofline": None, "kernels": None,
           "hbm_kernels": None, "roofline_ct": None}

    if rank == 0 and dump_dir is not None:
        # the last timed step's results, before anything below runs more steps: loss terms and outputs, the parameters and
        # buffers after its optimizer step, the gradients it applied
        arrays = dict(last)
        arrays.update({"state." + k: v for k, v in model.state_dict().items()})
        arrays.update({"grad." + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
        dump_outputs(dump_dir, arrays)

    if rank == 0 and not args.no_roofline:
        # per-kernel HIP-event timing on the launch stream (eager launches; the graph replays the same kernels)
        for i in range(2):
            kernels_mod.stage_batch(static_x, batches[i % 4])
            local_step()
        torch.cuda.synchronize()
        native.prof_enable(True)
        nprof = 5
        # eager launches are host-bound (3.5 ms of Python per 1.9 ms of GPU work): park the stream behind a spin kernel
        # so that the profiled launches queue up and run back to back like they do inside the hipGraph; otherwise each
        # HIP-event pair would also time the idle gap in front of its kernel
        torch.cuda._sleep(int(6e7))
        native.prof_calibrate(64)
        for i in range(nprof):
            kernels_mod.stage_batch(static_x, batches[i % 4])
            local_step()
        torch.cuda.synchronize()
        native.prof_enable(False)
        rep = native.prof_report()
        # what an event pair costs with no kernel inside: subtracted from every timed launch (the rocprofv3 kernel
        # trace in profiles/ measures dispatch->completion without it)
        cal = rep.pop("(empty event pair)", None)
        pair_ms = cal["ms"] / cal["count"] if cal and cal["count"] else 0.0
        for v in rep.values():
            v["ms"] = max(v["ms"] - pair_ms * v["count"], 1e-9)
        if want_kernels:
            res["kernels"] = {k: {"launches_per_step": v["count"] / nprof, "ms_per_step": round(v["ms"] / nprof, 4),
                                  "avg_us": round(v["ms"] / v["count"] * 1e3, 2)}
                              for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["ms"])}
        name, top = max(rep.items(), key=lambda kv: kv[1]["ms"])
        if top["flops"] > 0:
            ach = top["flops"] / (top["ms"] * 1e-3) / 1e12
            roofline = {"bound": "mfma", "kernel": name, "achieved": round(ach, 2), "peak": PEAK_F32_MFMA_TFLOPS,
                        "unit": "TFLOP/s", "frac": round(ach / PEAK_F32_MFMA_TFLOPS, 4), "traffic": None,
                        "avg_launch_us": round(top["ms"] / top["count"] * 1e3, 2),
                        "launches_per_step": top["count"] / nprof,
                        "algorithmic_flop_per_launch": round(top["flops"] / top["count"]),
                        "algorithmic_bytes_per_launch": round(top["bytes"] / top["count"])}
            if name.startswith("wino_"):
                # Winograd F(2x2,3x3): the layer's convolution FLOPs are what `top["flops"]` counts, but the MFMA units execute
                # only 16/36 of them.  The ROOFLINE figure (achieved / frac) is the EXECUTED rate; the convolution-equivalent
                # rate (which can exceed the peak) is reported beside it, never as `frac`.
                roofline["conv_equivalent_tflops"] = roofline["achieved"]
                roofline["conv_equivalent_frac"] = roofline["frac"]
                roofline["achieved"] = round(ach * 16.0 / 36.0, 2)
                roofline["frac"] = roofline["executed_frac"] = round(ach * 16.0 / 36.0 / PEAK_F32_MFMA_TFLOPS, 4)
                roofline["note"] = ("Winograd F(2x2,3x3): achieved/frac = MFMA FLOP actually executed (16/36 of the direct "
                                    "convolution's) / time; conv_equivalent_* = direct-convolution FLOP / time")
        else:
            ach = top["bytes"] / (top["ms"] * 1e-3) / 1e9
            roofline = {"bound": "hbm", "kernel": name, "achieved": round(ach, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s",
                        "frac": round(ach / PEAK_HBM_GBS, 4), "traffic": None,
                        "avg_launch_us": round(top["ms"] / top["count"] * 1e3, 2),
                        "launches_per_step": top["count"] / nprof}
        wl_key = f"{wl.model} bs={B}" + (f" a{wl.action_dim}" if wl.model == "CTMCQVAE" else "")
        roofline["traffic"], src = pmc_traffic(name, "VanillaVAE bs=256" if (wl_key == "MCQVAE bs=256" and name.startswith("wino_")
                                                                        and pmc_traffic(name, wl_key)[0] is None) else wl_key)
        if src:
            roofline["traffic_source"] = src + " (bytes per launch; FETCH_SIZE x2 gfx950 correction + WRITE_SIZE)"
        # GB/s against the 8 TB/s HBM peak for the HBM-bound kernels (loss reductions, reparameterisation, VQ lookup,
        # BatchNorm, Adam, layout changes): algorithmic bytes of the launch geometry / HIP-event time; counter traffic beside it
        hbm = []
        for k, v in sorted(rep.items(), key=lambda kv: -kv[1]["ms"]):
            if v["flops"] > 0 or v["bytes"] <= 0 or k == name:
                continue
            gbs = v["bytes"] / (v["ms"] * 1e-3) / 1e9
            e = {"kernel": k, "launches_per_step": v["count"] / nprof, "avg_launch_us": round(v["ms"] / v["count"] * 1e3, 2),
                 "algorithmic_bytes_per_launch": round(v["bytes"] / v["count"]), "achieved_gbs": round(gbs, 1),
                 "frac_of_8tbs": round(gbs / PEAK_HBM_GBS, 4)}
            t, _ = pmc_traffic(k, wl_key)
            if t is not None:
                e["traffic"] = t
                e["traffic_gbs"] = round(t * v["count"] / (v["ms"] * 1e-3) / 1e9, 1)
            hbm.append(e)
        res["hbm_kernels"] = hbm[:12]
        if wl.model == "CTMCQVAE":
            # the causal-transition layer (ct_mcq_vae.py:42-333): its dominant kernel against the f32 vector / matrix peak (both
            # 157.3 TFLOP/s on MI355X: f32 MFMA runs at the vector rate), and the step fraction with the layer's arithmetic counted
            ct = {k: v for k, v in rep.items() if k.startswith(CT_PREFIXES) and v["flops"] > 0}
            if ct:
                k, v = max(ct.items(), key=lambda kv: kv[1]["ms"])
                ach = v["flops"] / (v["ms"] * 1e-3) / 1e12
                ct_flop_step = sum(x["flops"] for x in ct.values()) / nprof
                ct_ms_step = sum(x["ms"] for kk, x in rep.items() if kk.startswith(CT_PREFIXES)) / nprof
                res["roofline_ct"] = {
                    "bound": "mfma" if k.startswith(("glinear", "gat_layer_mfma", "pair_mlp_mfma")) else "valu", "kernel": k,
                    "achieved": round(ach, 2), "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": round(ach / PEAK_F32_MFMA_TFLOPS, 4),
                    "avg_launch_us": round(v["ms"] / v["count"] * 1e3, 2), "launches_per_step": v["count"] / nprof,
                    "algorithmic_flop_per_launch": round(v["flops"] / v["count"]),
                    "algorithmic_bytes_per_launch": round(v["bytes"] / v["count"]),
                    "layer_kernels_ms_per_step": round(ct_ms_step, 4), "layer_flop_per_step": round(ct_flop_step),
                    "note": "FLOP = the arithmetic of the reference's formulas for these kernels (2 per multiply-add of the GEMMs, the "
                            "packed add/max/fma count of the pair and attention kernels), launch geometry x per-element count"}
                tot = (FLOP_PER_IMG[wl.model] * B + ct_flop_step) * (args.steps / elapsed) / 1e12
                roofline["step_frac_with_ct_layer"] = round(tot / PEAK_F32_MFMA_TFLOPS, 4)
        roofline["event_pair_overhead_us"] = round(pair_ms * 1e3, 2)
        step_tflops = FLOP_PER_IMG[wl.model] * (B * args.steps / elapsed) / 1e12
        roofline["step_conv_tflops_per_gpu"] = round(step_tflops, 2)
        roofline["step_frac_of_f32_mfma_peak"] = round(step_tflops / PEAK_F32_MFMA_TFLOPS, 4)
        res["roofline"] = roofline

    if rank == 0 and args.detail:
        native.prof_enable(True, detailed=True)
        for i in range(3):
            kernels_mod.stage_batch(static_x, batches[i % 4])
            local_step()
        torch.cuda.synchronize()
        native.prof_enable(False)
        for k, v in sorted(native.prof_report().items(), key=lambda kv: -kv[1]["ms"]):
            tf = v["flops"] / (v["ms"] * 1e-3) / 1e12 if v["ms"] > 0 else 0.0
            print(f"{v['ms'] / 3 * 1e3:9.1f} us/step  {v['count'] // 3:3d}x  {tf:7.1f} TF/s  {v['bytes'] / max(v['ms'], 1e-9) / 1e6:8.1f} GB/s  {k}",
                  file=sys.stderr)
    del graph, graph2, model, opt, ddp, batches, static_x
    torch.cuda.empty_cache()
    return res


def main():
    args = parse()
    # stdout carries exactly ONE JSON line (rank 0).  Native libraries write there too (RCCL prints a five-line version
    # banner to fd 1 when its communicator comes up), so fd 1 is pointed at stderr for the whole run and the result line
    # goes to the saved descriptor at the end.
    sys.stdout.flush()
    result_fd = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world > 1:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the hot path has no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # --rehearse-ddp: run the N>1 code path (graphs + RCCL collectives on the communication stream) in a 1-rank group
    ddp_on = multi = world > 1 or args.rehearse_ddp
    if ddp_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29517")
        dist.init_process_group("nccl", device_id=dev, rank=rank, world_size=world)

    from ctvae_amd import native
    native.load()
    ctx = {"rank": rank, "world": world, "dev": dev, "multi": multi, "ddp_on": ddp_on}

    head = Workload(args.model, args.batch, args.action_dim)
    r = run_workload(head, args, ctx, want_kernels=True, dump_dir=args.dump_outputs)

    # BASELINE.json configs[1..4] and the metric's own bs=64 wording, measured in the same process so that one driver-run
    # line covers them: same step contents, same timing protocol, DDP exchange included at N>1 (the >= 6x scaling target
    # of BASELINE.json is quoted on CT-MCQ-VAE)
    extra = []
    if not args.no_configs and (args.model, args.batch, args.action_dim) == ("VanillaVAE", 64, 12):
        for wl in (Workload("VanillaVAE", 256), Workload("MCQVAE", 256), Workload("CTMCQVAE", 128, 12), Workload("CTMCQVAE", 128, 20)):
            e = run_workload(wl, args, ctx)
            entry = {"workload": wl.label(world), "per_gpu_batch": wl.batch, "global_batch": wl.batch * world,
                     "ms_per_step": round(e["ms_per_step"], 4), "value": round(e["value"], 1), "unit": wl.unit,
                     "per_gpu": round(e["value"] / world, 1), "hipgraph": e["hipgraph"]}
            if e["roofline"] is not None:
                rf = e["roofline"]
                entry["step_frac_of_f32_mfma_peak"] = rf["step_frac_of_f32_mfma_peak"]
                entry["roofline"] = {k: rf[k] for k in ("bound", "kernel", "achieved", "peak", "unit", "frac", "avg_launch_us",
                                                         "launches_per_step", "executed_frac", "conv_equivalent_frac") if k in rf}
                if e["hbm_kernels"]:
                    entry["hbm_kernels"] = e["hbm_kernels"][:5]
                if wl.model == "CTMCQVAE":
                    entry["step_frac_note"] = ("step_frac_of_f32_mfma_peak: conv-path FLOP only (SURVEY 8d convention); "
                                               "step_frac_with_ct_layer adds the causal-transition layer's kernels")
                    if "step_frac_with_ct_layer" in rf:
                        entry["step_frac_with_ct_layer"] = rf["step_frac_with_ct_layer"]
                    if e["roofline_ct"] is not None:
                        entry["roofline_ct"] = e["roofline_ct"]
            extra.append(entry)

    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(args.model, args.cpu_seconds, args.action_dim)

    if rank == 0:
        B = args.batch
        unit = head.unit
        line = {
            # BASELINE.json's metric string verbatim for the configuration it is quoted on; other command lines say what they ran
            "metric": (BASELINE_METRIC if (args.model, B) == ("VanillaVAE", 64)
                       else f"{unit.split('/')[0]}/sec/GPU fwd+bwd, {args.model} 64x64x3 bs={B}; recon+KL vs CPU ref"),
            "value": round(r["value"], 1), "unit": unit, "per_gpu": round(r["value"] / world, 1),
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(r["ms_per_step"], 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": head.label(world) + (" (configs/vae.yaml shapes at the batch BASELINE.json's metric names, bs=64, on "
                                                        "one MI355X; BASELINE.json configs[1..4] are the `configs` entries)"
                                                        if (args.model, B) == ("VanillaVAE", 64) else ""),
                       "per_gpu_batch": B, "global_batch": B * world, "latent_dim": 128,
                       "parallelism": f"dp{world}" if world > 1 else "single", "hipgraph": r["hipgraph"],
                       "allreduce_overlap": r["overlap"]},
            "roofline": r["roofline"], "cpu_baseline": cpu,
        }
        if extra:
            line["configs"] = extra
        if r["roofline_ct"] is not None:
            line["roofline_ct"] = r["roofline_ct"]
        if r["hbm_kernels"]:
            line["hbm_kernels"] = r["hbm_kernels"]
        if r["kernels"] is not None:
            line["kernels"] = r["kernels"]
        sys.stdout.flush()
        os.write(result_fd, (json.dumps(line) + "\n").encode())
    if multi:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
