// Channel-owner BatchNorm launches (bn.hip bn_fused_fwd_kernel / bn_fused_bwd_kernel): how many channels a workgroup owns and
// which ones.  Plain C++ shared by the launcher, both kernels and the host emulation of the CPU tests
// (tests/host_emul/bn_owner_emul.cpp): nothing here is device-only.
#pragma once

#if defined(__HIPCC__)
#define CTVAE_BNOWNER_HD __host__ __device__ __forceinline__
#else
#define CTVAE_BNOWNER_HD inline
#endif

namespace ctvae {

// two channels per workgroup where four would leave most of the chip idle (fewer than kBnFusedTwoBelow channels)
constexpr int kBnFusedTwoBelow = 256;

CTVAE_BNOWNER_HD int bn_owner_cpw(int C) { return C < kBnFusedTwoBelow ? 2 : 4; }

// Channel group of the workgroup with dispatch index `id` in the grid of G = C / cpw groups.  A workgroup writes / reads 8 or 16
// bytes of every NHWC row, and workgroups are dealt to the eight XCDs in launch order (id % 8: observed, relied on for speed
// only).  With group = id the owners of one 32-byte sector sit on several XCDs: every L2 holds partly written sectors of every
// row (masked partial write-backs, 8 x the bytes of the tensor at C = 128) and fills every line of y to use a piece of it.
//   * C a multiple of 256: whole 128-byte lines (32 channels) per XCD, line j on XCD j % 8:
//     id = (line % 8) + 8 * (slot + slots * (line / 8)), slots = groups per line.
//   * any other G that is a multiple of 8: the workgroups of XCD x own ONE contiguous run of C / 8 channels -- 64 bytes = two
//     whole sectors of every row at C = 128, one sector at C = 64, half a sector at C = 32.
//     (At C = 256 the two forms are the same map.  At C = 512 the contiguous form -- lines 2x and 2x + 1 on XCD x -- measured
//     0.2 - 0.4 us slower per launch at R = 1024 than lines x and x + 8, so the multiples of 256 keep theirs: DESIGN.md 4.8.)
//   * every other G (a group count that does not deal out evenly, e.g. fewer than 16 channels at two per workgroup): group = id.
// The map is a permutation of the groups: a channel's own arithmetic does not depend on which workgroup runs it.
CTVAE_BNOWNER_HD int bn_owner_group(int id, int C, int cpw) {
  const int G = C / cpw;
  if (C % 256 == 0) {   // cpw (2 or 4) divides 32, so G = (C / 256) * 8 * slots: the eight-line blocks below tile the grid exactly
    const int slots = 32 / cpw, x = id & 7, t = id >> 3, slot = t % slots, jh = t / slots;
    return (jh * 8 + x) * slots + slot;
  }
  if (G == 0 || G % 8 != 0) return id;
  return (id & 7) * (G / 8) + (id >> 3);
}

}  // namespace ctvae
