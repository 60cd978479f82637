"""CPU: which channels a workgroup of the channel-owner BatchNorm kernels owns (ct-vae_amd/csrc/bnowner.hpp, the header the
kernels and the launcher of csrc/bn.hip use), compiled as plain C++ and checked for every channel count the launcher accepts:
C % 4 == 0 up to 1024, with two and with four channels per workgroup (the launcher's own pick among them is asserted to be one
of the two).

  * the map is a bijection on [0, C / CPW): every channel has exactly one owner;
  * when the grid G = C / CPW is a multiple of 8, the workgroups of each residue id % 8 (one XCD, by the round-robin dispatch
    the placement assumes for speed) own C / 8 channels: ONE contiguous run -- except for C a multiple of 256, where the
    measured-faster form was kept: whole 128-byte lines of 32 channels, line j with residue j % 8, which is the
    same contiguous run at C = 256 and C / 256 separate lines beyond;
  * any other G is left as it is (group = id).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_emul", "bn_owner_emul.cpp")
SO = os.path.join(HERE, "host_emul", "_bn_owner_emul.so")
HDR = os.path.join(os.path.dirname(HERE), "ct-vae_amd", "csrc", "bnowner.hpp")

CHANNELS = list(range(4, 1025, 4))


@pytest.fixture(scope="module")
def emul():
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-o", SO, SRC])
    lib = ctypes.CDLL(SO)
    lib.bn_owner_emul_cpw.argtypes = [ctypes.c_int]
    lib.bn_owner_emul_cpw.restype = ctypes.c_int
    lib.bn_owner_emul_groups.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    lib.bn_owner_emul_groups.restype = None
    return lib


def groups_of(lib, C, cpw):
    out = np.full(C // cpw, -1, np.int32)
    lib.bn_owner_emul_groups(C, cpw, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    return out.astype(np.int64)


def test_launcher_picks_two_or_four_channels_per_workgroup(emul):
    for C in CHANNELS:
        cpw = emul.bn_owner_emul_cpw(C)
        assert cpw in (2, 4) and C % cpw == 0, (C, cpw)
    assert emul.bn_owner_emul_cpw(128) == 2 and emul.bn_owner_emul_cpw(256) == 4      # the threshold measured in tools/negative/README.md, round 6


@pytest.mark.parametrize("cpw", [2, 4])
def test_owner_map(emul, cpw):
    runs = lines = same = 0
    for C in CHANNELS:
        G = C // cpw
        grp = groups_of(emul, C, cpw)
        assert np.array_equal(np.sort(grp), np.arange(G)), f"C={C} CPW={cpw}: not a bijection on [0, {G})"
        if G % 8 != 0:
            assert np.array_equal(grp, np.arange(G)), f"C={C} CPW={cpw}: G={G} is no multiple of 8, the map must be the identity"
            same += 1
            continue
        run = C // 8
        for x in range(8):
            ch = np.sort(np.concatenate([g * cpw + np.arange(cpw) for g in grp[x::8]]))      # channels of the workgroups id % 8 == x
            assert len(ch) == run, f"C={C} CPW={cpw} XCD {x}: {len(ch)} channels"
            if C % 256 == 0:
                want = np.concatenate([32 * j + np.arange(32) for j in range(x, C // 32, 8)])   # whole lines x, x + 8, ...
            else:
                want = x * run + np.arange(run)                                                  # one contiguous run
            assert np.array_equal(ch, want), f"C={C} CPW={cpw} XCD {x}: channels {ch.tolist()}"
        if C % 256 == 0:
            lines += 1
        else:
            runs += 1
    assert lines == 4 and runs > 0 and same > 0 and lines + runs + same == len(CHANNELS)
