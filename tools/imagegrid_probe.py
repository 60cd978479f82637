"""Cost of the sample-image path, on the GPU:

  1. imagegrid.make_grid_u8 on the reference's validation batch (144 x 3 x 64 x 64, channels_last, normalize, nrow 12) against
     the same arithmetic composed from torch ops on the same device (min / max, sub / div, a copy into a pre-filled grid, mul /
     add / clamp / to(uint8), permute + contiguous) -- alternating rounds in one process, device events around each round, and
     the two byte streams compared;
  2. what VAEXperiment.sample_images adds to one VanillaVAE validation epoch at val_batch_size 64: the whole call next to the
     validation loop, and its parts (device work, the device -> host copies, zlib, the file writes) timed on their own.

    python tools/imagegrid_probe.py [--rounds 20] [--calls 50]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_grid(x, nrow=12, padding=2):
    """torchvision's make_grid(normalize=True) + save_image's byte conversion, as torch ops -> uint8 [Hg, Wg, 3]."""
    N, C, H, W = x.shape
    xmaps = min(nrow, N)
    ymaps = -(-N // xmaps)
    lo, hi = x.min(), x.max()
    v = (x.clamp(lo, hi) - lo) / (hi - lo).clamp_min(1e-5)
    grid = x.new_zeros((ymaps, xmaps, C, H + padding, W + padding))
    grid.view(-1, C, H + padding, W + padding)[:N, :, padding:, padding:] = v
    grid = grid.permute(2, 0, 3, 1, 4).reshape(C, ymaps * (H + padding), xmaps * (W + padding))
    grid = torch.nn.functional.pad(grid, (0, padding, 0, padding))          # make_grid's frame: the last `padding` rows / columns
    return grid.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def _events(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls          # us per call


def _wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), min(out)        # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=50)
    args = ap.parse_args()
    from ctvae_amd import filler, imagegrid, specs
    from ctvae_amd.experiment import VAEXperiment
    from ctvae_amd.models import vae_models
    dev = torch.device("cuda", 0)

    x = (filler.synthetic_batch(7, 144)[0] * 2 - 1).to(dev).contiguous(memory_format=torch.channels_last)
    ours = lambda: imagegrid.make_grid_u8(x, nrow=12, normalize=True)          # noqa: E731
    theirs = lambda: torch_grid(x)                                             # noqa: E731
    same = bool(torch.equal(ours(), theirs()))
    for _ in range(3):
        _events(ours, args.calls), _events(theirs, args.calls)
    t_ours, t_theirs = [], []
    for _ in range(args.rounds):
        t_ours.append(_events(ours, args.calls))
        t_theirs.append(_events(theirs, args.calls))
    print(json.dumps({"what": "make_grid_u8 vs torch ops, 144x3x64x64 channels_last, us per call (enqueue-to-done, eager)",
                      "bytes_equal": same, "hip_median": statistics.median(t_ours), "hip_min": min(t_ours),
                      "torch_median": statistics.median(t_theirs), "torch_min": min(t_theirs)}), flush=True)

    m = vae_models["VanillaVAE"](in_channels=3, latent_dim=128)
    m.load_state_dict(filler.fill_state(specs.vanilla_specs(), 1266))
    m = m.to(dev)
    zeros = torch.zeros(64, device=dev)
    val = [(filler.synthetic_batch(90 + i, 64)[0].to(dev), zeros) for i in range(8)]
    batch = (filler.synthetic_batch(70, 64)[0].to(dev), zeros)
    with tempfile.TemporaryDirectory() as tmp:
        exp = VAEXperiment(m, {"LR": 0.005, "kld_weight": 0.00025, "manual_seed": 1265}, val_sampling=True, sample_dir=tmp)
        m.eval()

        def val_epoch():
            for i, b in enumerate(val):
                exp.validation_step(b, i)

        def device_part():
            with torch.no_grad():
                g = [imagegrid.make_grid_u8(batch[0], nrow=12, normalize=True, scanlines=True),
                     imagegrid.make_grid_u8(m.generate(batch[0], labels=zeros), nrow=12, normalize=True, scanlines=True),
                     imagegrid.make_grid_u8(m.sample(32, dev, labels=zeros[:32]), nrow=12, normalize=True, scanlines=True)]
            return g

        grids = device_part()
        host = [g.cpu().numpy().tobytes() for g in grids]
        packed = [zlib.compress(h, 6) for h in host]

        def write():
            for i, p in enumerate(packed):
                with open(os.path.join(tmp, f"{i}.bin"), "wb") as f:
                    f.write(p)

        for fn in (val_epoch, lambda: exp.sample_images(batch, 0), device_part):
            fn()
        res = {"what": "VanillaVAE val_batch_size 64, ms (median, min) of 15",
               "validation_epoch_8_batches": _wall(val_epoch, 15), "sample_images": _wall(lambda: exp.sample_images(batch, 0), 15),
               "device_work": _wall(device_part, 15), "d2h_copies": _wall(lambda: [g.cpu() for g in grids], 15),
               "zlib": _wall(lambda: [zlib.compress(h, 6) for h in host], 15), "file_writes": _wall(write, 15),
               "stream_bytes": [len(h) for h in host], "png_bytes": [len(p) for p in packed]}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
