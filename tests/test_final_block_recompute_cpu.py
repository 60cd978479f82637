"""CPU (hipcc -S, no GPU): the two kernels of the final block's recompute path keep their registers.

up_wgrad_kernel<Recompute> runs one wave per SIMD with nine accumulators, two g_a accumulators, two slots of y values and the 28
hoisted constants of the picture-side conv; a third slot of y values spilled five registers to scratch (upconv.hip).  A spill
reload in its step loop drains the loads issued ahead (tests/test_host_logic.py pins the same for <true> / <false>).
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_recompute_kernels_have_no_scratch():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    files = [os.path.join(ROOT, "ct-vae_amd", "csrc", f) for f in ("upconv.hip", "image.hip")]
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_audit.py")] + files, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-500:]
    lines = out.stdout.splitlines()
    for name in ("void up_wgrad_kernel<Recompute>", "void img_bwd_fused_kernel<false>", "void img_bwd_fused_kernel<true>"):
        heads = [i for i, l in enumerate(lines) if not l.startswith("    ") and ": " in l and l.split(": ", 1)[1].startswith(name)]
        assert heads, (name, [l for l in lines if not l.startswith("    ")])
        for i in heads:
            assert "scratch 0 B" in lines[i + 1], (name, lines[i + 1])
