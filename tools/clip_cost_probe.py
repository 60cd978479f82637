"""Kernel cost of gradient clipping: trains one config through ctvae_amd.run twice in one process -- with
trainer_params.gradient_clip_val and with the key removed -- so that one kernel trace holds adam_kernel next to
grad_sqnorm_kernel + adam_clip_kernel for the same parameter count ("Gradient clipping").

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/clip_cost_probe.py configs/gammavae.yaml --batch 64
    python tools/rocpd_export.py OUT/run_results.db > stats.csv
"""
import argparse
import os
import sys
import tempfile

import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--clip", type=float, default=0.8)
    ap.add_argument("--algorithm", default="norm")
    args = ap.parse_args()
    from ctvae_amd import run
    with tempfile.TemporaryDirectory() as tmp:
        for clip in (args.clip, None):
            cfg = yaml.safe_load(open(args.config))
            cfg["data_params"]["train_batch_size"] = cfg["data_params"]["val_batch_size"] = args.batch
            cfg["logging_params"]["save_dir"] = os.path.join(tmp, str(clip))
            cfg["trainer_params"].pop("gradient_clip_val", None)
            if clip is not None:
                cfg["trainer_params"].update(gradient_clip_val=clip, gradient_clip_algorithm=args.algorithm)
            path = os.path.join(tmp, f"{clip}.yaml")
            with open(path, "w") as f:
                yaml.safe_dump(cfg, f)
            run.main(["-c", path, "--steps-per-epoch", str(args.steps), "--max-epochs", "1"])
            print(f"clip {clip}: {args.steps} steps of {cfg['model_params']['name']} at batch {args.batch}", flush=True)


if __name__ == "__main__":
    main()
