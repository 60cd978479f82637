"""tools/isa_audit.py on tapgemm_fast.hip (hipcc -S, no GPU): the paired backward kernels with a 128 x 32 role (VanillaVAE
encoder.1 / decoder.3) keep the properties of the 64 x 64 pair -- no scratch at all, hence no spill reloads in
their loops, and the kernel arguments of both roles fetched behind ONE batch of scalar loads (common.hpp kernarg_warm_get)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_narrow_pair_kernels_have_no_scratch_and_one_argument_batch():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "ct-vae_amd", "csrc", "tapgemm_fast.hip")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_audit.py"), src], capture_output=True, text=True, timeout=1200)
    assert out.returncode == 0, out.stderr[-500:]
    blocks, cur = {}, None
    for line in out.stdout.splitlines():
        if not line.startswith("    "):
            cur = line.split(": ", 1)[1] if ": " in line else line
            blocks[cur] = []
        elif cur is not None:
            blocks[cur].append(line)
    for prefix in ("void conv_bwd_pair_kernel<true, 1, 4, 2>", "void conv_bwd_pair_kernel<false, 1, 2, 4>"):
        hits = [k for k in blocks if k.startswith(prefix)]
        assert len(hits) == 1, (prefix, list(blocks))
        lines = blocks[hits[0]]
        assert "scratch 0 B" in lines[0] and "argument lines fetched in one batch" in lines[0], (prefix, lines[0])
        assert not any(l.strip().startswith("loop") and l.rstrip().endswith("scratch") for l in lines), (prefix, lines)
