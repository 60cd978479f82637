// Per-action hit counts of the causal mode (rollout.py: ActionHits): probas [N][A] is forward_causal's recons_action, action
// [N][A] the one-hot action that was applied.  With V = A / 2, a = argmax(action row), p = argmax(probas row):
//   counts[a][0] += 1                       rows of action a
//   counts[a][1] += (p == a)                directed hits            (CausalTransition.causal_accuracy, per action)
//   counts[a][2] += (p % V == a % V)        direction-agnostic hits  (causal_undirected_accuracy folds the two halves)
// argmax is torch.argmax: the first maximal value wins, NaN counts as maximal and the first NaN wins.
// A group of G = min(64, pow2ceil(A)) lanes owns one row at a time (consecutive lanes read consecutive columns, as catlatent.hip
// does), the (value, index) pair goes through xor shuffles inside the group, the group's first lane adds into a per-workgroup
// [A][3] histogram in LDS, and the workgroup ends with ONE global atomic add per non-zero histogram word.  Integer adds only:
// the result does not depend on the order of workgroups or launches, and successive launches accumulate.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kHitsMaxA = 256;
constexpr int kHitsMaxBlocks = 512;

// does (bv, bi) come before (av, ai) in torch.argmax's order?  A strict total order over distinct indices.
__device__ __forceinline__ bool argmax_before(float av, int ai, float bv, int bi) {
  const bool an = av != av, bn = bv != bv;
  if (an || bn) return (an && bn) ? bi < ai : bn;
  return bv > av || (bv == av && bi < ai);
}

template <int NPL>
__device__ __forceinline__ int group_argmax(const float* __restrict__ row, int A, int G, int gl, bool live) {
  float v = -INFINITY;
  int i = 0x7fffffff;                         // the padding beyond A loses every tie, also against -inf
#pragma unroll
  for (int k = 0; k < NPL; ++k) {
    const int q = gl + k * G;
    if (live && q < A) {
      const float t = row[q];
      if (argmax_before(v, i, t, q)) { v = t; i = q; }
    }
  }
  for (int o = G >> 1; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (argmax_before(v, i, ov, oi)) { v = ov; i = oi; }
  }
  return i;
}

template <int NPL>
__global__ __launch_bounds__(256) void action_hits_kernel(const float* __restrict__ probas, const float* __restrict__ action, int N,
                                                          int A, int G, int* __restrict__ counts) {
  __shared__ int hist[kHitsMaxA * 3];
  for (int i = threadIdx.x; i < 3 * A; i += 256) hist[i] = 0;
  __syncthreads();
  const int gl = threadIdx.x & (G - 1), gpb = 256 / G, V = A >> 1;
  // the loop bound is the same for the whole workgroup: every lane of a wave takes part in every shuffle
  for (long base = (long)blockIdx.x * gpb; base < N; base += (long)gridDim.x * gpb) {
    const long row = base + threadIdx.x / G;
    const bool live = row < N;
    const long off = live ? row * A : 0;
    const int a = group_argmax<NPL>(action + off, A, G, gl, live);
    const int p = group_argmax<NPL>(probas + off, A, G, gl, live);
    if (live && gl == 0) {                    // a, p < A: a live row has A >= 2 real columns in front of the padding
      atomicAdd(&hist[3 * a], 1);
      if (p == a) atomicAdd(&hist[3 * a + 1], 1);
      if (p % V == a % V) atomicAdd(&hist[3 * a + 2], 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * A; i += 256) {
    const int h = hist[i];
    if (h != 0) atomicAdd(&counts[i], h);
  }
}

int launch_action_hits(const float* probas, const float* action, int N, int A, int* counts, hipStream_t st) {
  if (!probas || !action || !counts || N < 0 || A < 2 || A > kHitsMaxA || (A & 1) != 0) return kErrBadArg;
  if (N == 0) return 0;
  int G = 2;
  while (G < A && G < 64) G <<= 1;
  const int npl = (A + G - 1) / G, gpb = 256 / G;
  const long want = ((long)N + gpb - 1) / gpb;
  const dim3 grid((unsigned)(want < kHitsMaxBlocks ? want : kHitsMaxBlocks));
  ProfScope ps("action_hits_kernel", st, 4.0 * N * A, 8.0 * N * A);
  if (npl == 1)
    hipLaunchKernelGGL(action_hits_kernel<1>, grid, dim3(256), 0, st, probas, action, N, A, G, counts);
  else if (npl == 2)
    hipLaunchKernelGGL(action_hits_kernel<2>, grid, dim3(256), 0, st, probas, action, N, A, G, counts);
  else
    hipLaunchKernelGGL(action_hits_kernel<4>, grid, dim3(256), 0, st, probas, action, N, A, G, counts);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
