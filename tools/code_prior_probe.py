"""Cost of the code prior (exp_params.code_prior) on one MI355X.

* ``kernels``: ``ctvae_code_prior_sample`` at n = 144 (a ``val_sampling`` sheet) for (K, C, H, W) = (64, 4, 8, 8) and
  (512, 1, 16, 16), and ``ctvae_code_prior_score`` at B = 4096, each against a plain-torch restatement of the same step sequence
  on the same GPU (the sampler: one batched gather / cumsum / searchsorted per token, C*H*W dependent steps; the scorer: four
  gathers and a reduction).  Device events around every launch behind a warm-up; per process the median over ``--launches``.
* ``step``: the validation step of MCQVAE (configs/mcq_vae.yaml) at bs = 64 through ``VAEXperiment.validation_step`` with the
  epoch's reports armed as ``_validate`` arms them -- for this tree without the key, this tree with the key and, with
  ``--parent DIR`` (a built checkout of the parent commit), the parent.  Device events per step, per process the median.

Every measurement runs in ``--procs`` (3) separate processes, the step variants alternating; a process gets ``--limit`` seconds and
the probe stops at the first one that fails.  Reported: the median of the processes' medians with their min .. max.  Prints one
JSON object.

    python tools/code_prior_probe.py [--parent DIR] [--out FILE]
"""
import argparse
import contextlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((64, 4, 8, 8), (512, 1, 16, 16))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "processes": len(xs)}


def _event_us(torch, call, launches, warm=10):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    us = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return statistics.median(us)


def _torch_sample(torch, tables, totals, lam, u, H, W):
    """The sampler's step sequence in plain torch, batched over the images: per token one expert choice, one row gather, one
    cumsum and one searchsorted."""
    n, HW, C, _ = u.shape
    K = tables[0].size(2)
    cum = torch.cumsum(lam, dim=1)
    out = torch.empty(n, C, H, W, dtype=torch.int64, device=u.device)
    img = torch.arange(n, device=u.device)
    boundary = torch.full((n,), K, dtype=torch.int64, device=u.device)
    for p in range(HW):
        h, w = divmod(p, W)
        for c in range(C):
            u1, u2 = u[:, p, c, 0], u[:, p, c, 1]
            j = torch.clamp((u1.unsqueeze(1) >= cum[c].unsqueeze(0)).sum(1), max=4)
            ctx = torch.stack([boundary, boundary, out[:, c, h, w - 1] if w > 0 else boundary,
                               out[:, c, h - 1, w] if h > 0 else boundary, out[:, c - 1, h, w] if c > 0 else boundary])
            rows = torch.stack([tables[0][c, p].expand(n, K), tables[0][c, p].expand(n, K), tables[1][c][ctx[2]], tables[2][c][ctx[3]],
                                tables[3][c][ctx[4]]])[j, img]
            csum = torch.cumsum(rows, dim=1)
            total = csum[:, -1]
            empty = (j == 0) | (total == 0)
            t = torch.minimum(total - 1, torch.floor(u2 * total.double()).long())
            k = torch.searchsorted(csum, t.unsqueeze(1), right=True).squeeze(1)
            ku = torch.clamp(torch.floor(u2 * float(K)).long(), max=K - 1)
            out[:, c, h, w] = torch.where(empty, ku, torch.clamp(k, max=K - 1))
    return out


def _torch_score(torch, inds, tables, totals, lam):
    B, C, H, W = inds.shape
    K = tables[0].size(2)
    c = torch.arange(C, device=inds.device).view(1, C, 1, 1).expand_as(inds)
    pos = torch.arange(H * W, device=inds.device).view(1, 1, H, W).expand_as(inds)
    left, up, prev = (torch.full_like(inds, K) for _ in range(3))
    left[:, :, :, 1:], up[:, :, 1:], prev[:, 1:] = inds[:, :, :, :-1], inds[:, :, :-1], inds[:, :-1]
    ctxs = (pos, left, up, prev)
    P = [torch.full(inds.shape, 1.0 / K, dtype=torch.float64, device=inds.device)]
    for t, tot, ctx in zip(tables, totals, ctxs):
        d = tot[c, ctx].double()
        P.append(torch.where(d > 0, t[c, ctx, inds].double() / d.clamp(min=1), P[0]))
    m = torch.stack(P, dim=-1) * lam.view(1, C, 1, 1, 5)
    mix = m.sum(-1)
    return torch.log(mix).sum((2, 3)), (m / mix.unsqueeze(-1)).sum((2, 3))


def worker_kernels(args):
    import torch
    sys.path.insert(0, ROOT)
    from ctvae_amd import kernels as Kn
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    res = {}
    for K, C, H, W in SHAPES:
        tables, invalid = Kn.code_prior_tables(K, C, H, W, dev)
        Kn.code_prior_count(torch.randint(0, K, (2048, C, H, W), generator=g, device=dev), tables, invalid)
        totals = Kn.code_prior_totals(tables)
        lam = torch.full((C, 5), 0.2, dtype=torch.float64, device=dev)
        u = torch.rand(144, H * W, C, 2, generator=g, device=dev, dtype=torch.float64)
        grids = torch.randint(0, K, (4096, C, H, W), generator=g, device=dev)
        ptr = lambda ts: [t.data_ptr() for t in ts]
        out = torch.empty(144, C, H, W, dtype=torch.int64, device=dev)
        logp = torch.empty(4096, C, dtype=torch.float64, device=dev)
        resp = torch.empty(4096, C, 5, dtype=torch.float64, device=dev)
        bad = torch.empty(4096, dtype=torch.int32, device=dev)
        sample = lambda: Kn.native.call("ctvae_code_prior_sample", *ptr(tables), *ptr(totals), lam.data_ptr(), u.data_ptr(),
                                        out.data_ptr(), 144, C, H, W, K)
        score = lambda: Kn.native.call("ctvae_code_prior_score", grids.data_ptr(), *ptr(tables), *ptr(totals), lam.data_ptr(),
                                       logp.data_ptr(), resp.data_ptr(), bad.data_ptr(), 4096, C, H, W, K)
        sample()
        same = bool(torch.equal(out, _torch_sample(torch, tables, totals, lam, u, H, W)))
        key = f"K{K}_C{C}_{H}x{W}"
        res[key] = {"sample_n144_us": _event_us(torch, sample, args.launches),
                    "sample_n144_torch_us": _event_us(torch, lambda: _torch_sample(torch, tables, totals, lam, u, H, W), 3, warm=1),
                    "sample_equals_torch": same,
                    "score_B4096_us": _event_us(torch, score, args.launches),
                    "score_B4096_torch_us": _event_us(torch, lambda: _torch_score(torch, grids, tables, totals, lam), args.launches)}
    print("RESULT " + json.dumps(res), flush=True)


def worker_step(args):
    root = args.tree
    sys.path.insert(0, root)
    import torch
    from ctvae_amd import filler, specs
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    dev = torch.device("cuda")
    cfg = specs.MCQ_CFG
    m = vae_models["MCQVAE"](**{**cfg, "hidden_dims": list(cfg["hidden_dims"])})
    m.load_state_dict(filler.fill_state(specs.mcq_specs(cfg), 1321))
    params = {"LR": 0.0005, "weight_decay": 0.0, "kld_weight": 0.00025, "manual_seed": 1320}
    if args.key:
        params["code_prior"] = {"type": "markov"}
    exp = VAEXperiment(m.to(dev), params, log_every=10 ** 9)
    batches = [(filler.synthetic_batch(1320 + i, 64)[0].to(dev), torch.zeros(64, device=dev)) for i in range(4)]
    exp.model.eval()
    i = [0]

    def step():
        exp.validation_step(batches[i[0] % 4], i[0])
        i[0] += 1
    with contextlib.ExitStack() as armed:
        for report in exp._val_reports():
            armed.enter_context(report(0))
        us = _event_us(torch, step, args.launches, warm=20)
    print("RESULT " + json.dumps({"validation_step_us": us}), flush=True)


def spawn(argv, limit):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"code_prior_probe: worker {argv} ended with {r.returncode}; nothing more is started\n{r.stdout}\n{r.stderr}")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--key", action="store_true")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--limit", type=int, default=150, help="seconds per worker process")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker == "kernels":
        return worker_kernels(args)
    if args.worker == "step":
        return worker_step(args)
    n = ["--launches", str(args.launches)]
    kern = [spawn(["--worker", "kernels"] + n, args.limit) for _ in range(args.procs)]
    res = {"kernels": {shape: {k: (spread([p[shape][k] for p in kern]) if k.endswith("_us") else all(p[shape][k] for p in kern))
                               for k in kern[0][shape]} for shape in kern[0]}}
    variants = {"no_key": ["--worker", "step"], "key": ["--worker", "step", "--key"]}
    if args.parent:
        variants = {"parent": ["--worker", "step", "--tree", os.path.abspath(args.parent)], **variants}
    steps = {v: [] for v in variants}
    for _ in range(args.procs):                     # alternating
        for v, argv in variants.items():
            steps[v].append(spawn(argv + n, args.limit)["validation_step_us"])
    res["validation_step_bs64_us"] = {v: spread(xs) for v, xs in steps.items()}
    if args.parent:
        p = res["validation_step_bs64_us"]["parent"]
        res["no_key_within_parent_spread"] = p["min"] <= res["validation_step_bs64_us"]["no_key"]["median"] <= p["max"]
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
