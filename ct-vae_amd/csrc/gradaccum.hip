// Gradient accumulation over the micro-batches of one optimizer step (trainer_params.accumulate_grad_batches, optim.py).
//   grad_accumulate_kernel   the window's running sum `acc` against the optimizer's slice `g` of the flat gradient buffer:
//                              STORE   acc = g          first micro-batch of a window
//                              ADD     acc = acc + g    every further one that does not end the window
//                              FINISH  g   = acc + g    the one that ends it: the sum lands in the flat buffer in place, acc stays
//   adam_flags_window_kernel the same three modes on FlatAdam's nb int32 block-activity words:
//                              window = active, window = max(window, active), active = max(window, active)
//
// Accumulate.  One fp32 add per element, `acc` always the left operand, so a window of micro-batches g0, g1, g2 ends as
// ((g0 + g1) + g2) whatever the launch geometry: the result is a function of the values alone.  Pure streaming (8 or 12 bytes
// per element, no reuse), so 16-byte accesses and a grid-stride loop over at most kAccumMaxWgs workgroups, two independent
// quads per thread in flight per turn (the shape adam_kernel streams at).  A slice of the flat buffer may start at any float
// (flat_range()) and n need not be a multiple of 4: `head` floats in front of g's first 16-byte boundary and the n - head -
// 4 * quads floats behind the last whole quad are handled float by float by the first threads of the grid.  The quad loop
// needs acc + head on a 16-byte boundary as well (FlatAdam allocates its accumulator that way); otherwise the whole range
// runs float by float.  64-bit indices, no atomics, plain loads and stores, nothing outside [0, n) is read or written.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kAccumStore = 0, kAccumAdd = 1, kAccumFinish = 2;
constexpr int kAccumThreads = 256, kAccumMaxWgs = 2048;
// floats one turn of a full grid's quad loop covers; a longer range wraps the grid-stride loop
constexpr long kAccumPassFloats = (long)kAccumMaxWgs * kAccumThreads * 8;

template <int MODE>
__global__ __launch_bounds__(kAccumThreads) void grad_accumulate_kernel(float* __restrict__ acc, float* __restrict__ g, long n,
                                                                        long head, long quads) {
  const long tid = (long)blockIdx.x * kAccumThreads + threadIdx.x;
  const long stride = (long)gridDim.x * kAccumThreads;
  if (quads > 0) {
    f32x4* a4 = reinterpret_cast<f32x4*>(acc + head);
    f32x4* g4 = reinterpret_cast<f32x4*>(g + head);
    for (long i = tid; i < quads; i += 2 * stride) {
      const long i2 = i + stride;
      const bool two = i2 < quads;
      if constexpr (MODE == kAccumStore) {
        const f32x4 ga = g4[i];
        const f32x4 gb = two ? g4[i2] : ga;
        a4[i] = ga;
        if (two) a4[i2] = gb;
      } else {
        const f32x4 aa = a4[i], ga = g4[i];
        const f32x4 ab = two ? a4[i2] : aa, gb = two ? g4[i2] : ga;
        if constexpr (MODE == kAccumAdd) {
          a4[i] = aa + ga;
          if (two) a4[i2] = ab + gb;
        } else {
          g4[i] = aa + ga;
          if (two) g4[i2] = ab + gb;
        }
      }
    }
  }
  // the floats in front of the first quad and behind the last one (everything when quads == 0)
  const long body = quads * 4, rest = n - body;
  for (long r = tid; r < rest; r += stride) {
    const long i = r < head ? r : r + body;
    if constexpr (MODE == kAccumStore) acc[i] = g[i];
    else if constexpr (MODE == kAccumAdd) acc[i] = acc[i] + g[i];
    else g[i] = acc[i] + g[i];
  }
}

size_t grad_accumulate_pass_floats() { return (size_t)kAccumPassFloats; }

int launch_grad_accumulate(float* acc, float* g, long n, int mode, hipStream_t st) {
  if (!acc || !g || n <= 0 || mode < kAccumStore || mode > kAccumFinish) return kErrBadArg;
  if ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(g)) % 4 != 0) return kErrBadArg;
  {   // the two ranges must not overlap (both are __restrict__, and a window's sum must not alias a gradient)
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(acc), g0 = reinterpret_cast<uintptr_t>(g), bytes = (uintptr_t)n * 4;
    if (a0 < g0 + bytes && g0 < a0 + bytes) return kErrBadArg;
  }
  long head = (long)(((16 - reinterpret_cast<uintptr_t>(g) % 16) % 16) / 4);
  if (head > n) head = n;
  long quads = (n - head) / 4;
  if (reinterpret_cast<uintptr_t>(acc + head) % 16 != 0) {   // the buffers' 16-byte phases differ: float by float throughout
    head = 0;
    quads = 0;
  }
  const long rest = n - 4 * quads;
  long threads = (quads + 1) / 2;                 // two quads per thread and turn
  if (threads < rest) threads = rest;
  long wgs = (threads + kAccumThreads - 1) / kAccumThreads;
  if (wgs > kAccumMaxWgs) wgs = kAccumMaxWgs;
  if (wgs < 1) wgs = 1;
  ProfScope ps("grad_accumulate_kernel", st, (double)(mode == kAccumStore ? 0 : n), (mode == kAccumStore ? 8.0 : 12.0) * (double)n);
  const dim3 grid((unsigned)wgs), block(kAccumThreads);
  if (mode == kAccumStore) hipLaunchKernelGGL(grad_accumulate_kernel<kAccumStore>, grid, block, 0, st, acc, g, n, head, quads);
  else if (mode == kAccumAdd) hipLaunchKernelGGL(grad_accumulate_kernel<kAccumAdd>, grid, block, 0, st, acc, g, n, head, quads);
  else hipLaunchKernelGGL(grad_accumulate_kernel<kAccumFinish>, grid, block, 0, st, acc, g, n, head, quads);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

// One workgroup, as the other block-flag launches (nb is a few hundred words at most).
__global__ __launch_bounds__(256) void adam_flags_window_kernel(int* __restrict__ window, int* __restrict__ active, int nb,
                                                                int mode) {
  for (int b = threadIdx.x; b < nb; b += 256) {
    const int a = active[b];
    if (mode == kAccumStore) {
      window[b] = a;
    } else {
      const int w = window[b];
      const int m = w > a ? w : a;
      if (mode == kAccumAdd) window[b] = m;
      else active[b] = m;
    }
  }
}

int launch_adam_flags_window(int* window, int* active, int nb, int mode, hipStream_t st) {
  if (!window || !active || window == active || nb < 1 || mode < kAccumStore || mode > kAccumFinish) return kErrBadArg;
  hipLaunchKernelGGL(adam_flags_window_kernel, dim3(1), dim3(256), 0, st, window, active, nb, mode);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
