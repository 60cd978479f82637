// Host view of the channel-owner BatchNorm placement (ct-vae_amd/csrc/bnowner.hpp) for tests/test_bn_owner_placement_host.py:
// the header itself, compiled as plain C++, behind a C ABI.
#include "../../ct-vae_amd/csrc/bnowner.hpp"

extern "C" {

int bn_owner_emul_cpw(int C) { return ctvae::bn_owner_cpw(C); }

// out[id] = channel group of workgroup id, for the grid of C / cpw workgroups the launcher starts
void bn_owner_emul_groups(int C, int cpw, int* out) {
  for (int id = 0; id < C / cpw; ++id) out[id] = ctvae::bn_owner_group(id, C, cpw);
}

}  // extern "C"
