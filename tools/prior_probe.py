"""Cost of the Gaussian-mixture prior (latentprior.py, csrc/gmm.hip), in one process on one MI355X:

* ``kernels_us``: the per-launch event time (the library's own event pairs, ``prof_report``) of every kernel of one EM iteration at
  (N, D, K) = (162 770, 128, 10) -- CelebA's training split at VanillaVAE's latent size -- full and diag, behind a warm-up, next to
  the empty event pair; ``estep_share_of_f32_peak`` counts 2 N D^2 K flops against 157.3 TF;
* ``torch_iteration_us``: a plain-torch fp32 restatement of the same iteration (device events), for context;
* ``fit_s``: ``GaussianMixturePrior.fit`` of 20 iterations (``tol=0``), host clock around a run that ends in a device synchronise:
  the kernels, the K Cholesky factorisations on the host and the copies in between;
* ``code_buffer_append_us``: the copy of one batch's codes (bs = 64) into the code buffer, device events over 200 copies;
* ``val_epoch_s`` (``--val``): the validation epoch of VanillaVAE at bs = 64 through ``VAEXperiment.fit`` -- ``--batches``
  validation batches, no training batches -- with ``sample_prior`` on and off, the two alternating.

Prints one JSON object: medians with the min .. max spread over the rounds.

    python tools/prior_probe.py [--val] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
F32_PEAK = 157.3e12


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "rounds": len(xs)}


def make_data(dev, N, D, K, seed=0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    centres = torch.randn(K, D, generator=g, device=dev) * 1.5
    which = torch.randint(0, K, (N,), generator=g, device=dev)
    scale = 0.5 + torch.rand(K, 1, generator=g, device=dev)
    return (centres[which] + scale[which] * torch.randn(N, D, generator=g, device=dev)).contiguous()


def start(prior, X):
    w, mu, cov = prior.default_start(X, seed=0)
    prior._set(w, mu, cov)
    return prior._prepare()


def kernel_times(dev, X, K, full, reps):
    from ctvae_amd import kernels as Kn, native
    from ctvae_amd.latentprior import GaussianMixturePrior
    N, D = X.shape
    prior = GaussianMixturePrior(D, K, "full" if full else "diag", device=dev)
    p = start(prior, X)
    ws = torch.empty(int(native.load().ctvae_gmm_mstep_workspace_bytes(N, D, K, int(full))) // 8, dtype=torch.float64, device=dev)

    def iteration():
        r, ll, bad = Kn.gmm_estep(X, p["log_w"], p["mu"], p["P"], p["ldh"], full=full)
        return Kn.gmm_mstep(X, r, bad, p["mu"], full=full, ws=ws)

    for _ in range(3):
        iteration()
    torch.cuda.synchronize()
    per, empty = {}, []
    for _ in range(reps):
        native.prof_enable(True)
        try:
            for _ in range(5):
                iteration()
            native.prof_calibrate(64)
            torch.cuda.synchronize()
        finally:
            native.prof_enable(False)
        rep = native.prof_report()
        for name, k in rep.items():
            if name.startswith("gmm_"):
                per.setdefault(name, []).append(k["ms"] * 1e3 / k["count"])
        cal = rep.get("(empty event pair)")
        if cal:
            empty.append(cal["ms"] * 1e3 / cal["count"])
    out = {name: spread(v) for name, v in per.items()}
    out["iteration_us"] = spread([sum(v[i] for v in per.values()) for i in range(reps)])
    out["empty_event_pair_us"] = spread(empty) if empty else None
    if full:
        e = out["gmm_estep_full_kernel"]["median"] * 1e-6
        out["estep_share_of_f32_peak"] = 2.0 * N * D * D * K / e / F32_PEAK
    out["mstep_slabs"] = Kn.gmm_mstep_slabs(N, D, K, full)
    return out


def torch_iteration(dev, X, K, full, reps):
    from ctvae_amd.latentprior import GaussianMixturePrior
    N, D = X.shape
    p = start(GaussianMixturePrior(D, K, "full" if full else "diag", device=dev), X)
    c = 0.5 * D * math.log(2 * math.pi)

    def iteration():
        lp = torch.empty(N, K, device=dev)
        for k in range(K):
            xc = X - p["mu"][k]
            y = xc @ p["P"][k].T if full else xc * p["P"][k]
            lp[:, k] = p["log_w"][k] - 0.5 * (y * y).sum(1) - p["ldh"][k] - c
        ll = torch.logsumexp(lp, 1)
        r = torch.exp(lp - ll[:, None])
        nk = r.sum(0)
        out = []
        for k in range(K):
            xc = X - p["mu"][k]
            wx = r[:, k, None] * xc
            out.append((wx.sum(0), wx.T @ xc if full else (wx * xc).sum(0)))
        return nk, out

    for _ in range(2):
        iteration()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        iteration()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return spread(us)


def fit_times(dev, X, K, full, reps, iters=20):
    from ctvae_amd.latentprior import GaussianMixturePrior
    s = []
    for i in range(reps + 1):
        prior = GaussianMixturePrior(X.size(1), K, "full" if full else "diag", device=dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = prior.fit(X, seed=0, max_iter=iters, tol=0.0)
        torch.cuda.synchronize()
        if i:
            s.append(time.perf_counter() - t0)
    return {"iterations": info["iterations"], **spread(s)}


def append_times(dev, bs, D, reps, launches=200):
    """The copy of one batch's codes -- a column half of a [B, 2D] heads tensor -- into the code buffer, device events."""
    from ctvae_amd.latentprior import CodeBuffer
    mu = torch.randn(bs, 2 * D, device=dev)[:, :D]
    buf = CodeBuffer(D, dev, capacity=bs * launches)
    us = []
    for i in range(reps + 1):
        buf.clear()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            buf.append(mu)
        b.record()
        torch.cuda.synchronize()
        if i:
            us.append(a.elapsed_time(b) * 1e3 / launches)
    return spread(us)


def val_epoch_times(dev, bs, batches, reps, extras):
    """``extras``: {name: exp_params to add}.  Also used from outside to time one tree against another."""
    from ctvae_amd import filler, specs
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    params = {"LR": 0.005, "weight_decay": 0.0, "kld_weight": 0.00025, "manual_seed": 1265}
    val = [(filler.synthetic_batch(1265 + i, bs)[0].to(dev), torch.zeros(bs, device=dev)) for i in range(4)]
    exps = {}
    for name, extra in extras.items():
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
    out["batches"], out["bs"] = batches, bs
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=162770)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--components", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--val", action="store_true")
    ap.add_argument("--bs", type=int, default=64)
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prior_probe measures on the GPU: no device found")
    dev = torch.device("cuda")
    X = make_data(dev, args.rows, args.dim, args.components)
    res = {"shape": [args.rows, args.dim, args.components]}
    for name, full in (("full", True), ("diag", False)):
        res[name] = {"kernels_us": kernel_times(dev, X, args.components, full, args.reps),
                     "torch_iteration_us": torch_iteration(dev, X, args.components, full, args.reps),
                     "fit_s": fit_times(dev, X, args.components, full, 3)}
    res["code_buffer_append_us"] = append_times(dev, args.bs, args.dim, args.reps)
    if args.val:
        prior = {"type": "gmm", "components": args.components, "max_iter": 1}
        res["val_epoch_s"] = val_epoch_times(dev, args.bs, args.batches, args.reps,
                                             {"off": {}, "on": {"sample_prior": prior},
                                              "on_diag": {"sample_prior": dict(prior, covariance="diag")}})
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
