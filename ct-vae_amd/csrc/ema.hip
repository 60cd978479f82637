// Exponential moving average of the weights (exp_params.ema_decay, optim.py: WeightEMA), on the optimizer's slice of the flat
// parameter buffer:
//   ema_update_kernel    ema = fmaf(one_minus_decay, p - ema, ema)   once per optimizer step, eagerly behind it; p is read only
//   buffer_swap_kernel   a <-> b as raw 32-bit words                 evaluation with the averaged weights: captured steps hold the
//                                                                    flat buffer's addresses, so contents move, not pointers
//
// Update.  One fp32 subtraction and one fma per element, in this form and no other: where ema == p the difference is an exact
// zero and the fma returns ema, so an average that has reached its parameter stays on it (a -0 pair becomes +0: equal in value).
// A NaN or Inf in p makes that element's average non-finite and no other's.  One step's error against the exact result is at
// most 2^-22 * max(|ema|, |p|): the subtraction rounds by 2^-24 * |p - ema| <= 2^-23 * max, scaled by 1 - d < 1, and the fma
// rounds once, by 2^-24 * |out|.
//
// Swap.  Loads and stores only, no arithmetic: NaN payloads and -0 pass through, and swapping twice is the identity bit for bit.
//
// Both stream the way grad_accumulate_kernel does (gradaccum.hip): 12 / 16 bytes per element and no reuse, so 16-byte accesses in
// a grid-stride loop over at most kEmaMaxWgs workgroups, two independent quads per thread in flight per turn.  A slice may start
// at any float and n need not be a multiple of 4: `head` floats in front of the second buffer's first 16-byte boundary and the
// n - head - 4 * quads floats behind the last whole quad go float by float through the first threads of the grid.  The quad loop
// needs the first buffer + head on a 16-byte boundary as well (WeightEMA allocates its buffer that way); otherwise the whole
// range runs float by float.  64-bit indices, no atomics, plain loads and stores, nothing outside [0, n) is read or written.
#include <cmath>

#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kEmaThreads = 256, kEmaMaxWgs = 2048;      // (grad_accumulate_kernel's geometry and cap)

__device__ __forceinline__ float ema_one(float e, float p, float w) { return fmaf(w, p - e, e); }

__device__ __forceinline__ f32x4 ema_quad(f32x4 e, f32x4 p, float w) {
  f32x4 r;
  r.x = ema_one(e.x, p.x, w);
  r.y = ema_one(e.y, p.y, w);
  r.z = ema_one(e.z, p.z, w);
  r.w = ema_one(e.w, p.w, w);
  return r;
}

__global__ __launch_bounds__(kEmaThreads) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long n,
                                                                 long head, long quads, float w) {
  const long tid = (long)blockIdx.x * kEmaThreads + threadIdx.x;
  const long stride = (long)gridDim.x * kEmaThreads;
  if (quads > 0) {
    f32x4* e4 = reinterpret_cast<f32x4*>(ema + head);
    const f32x4* p4 = reinterpret_cast<const f32x4*>(p + head);
    for (long i = tid; i < quads; i += 2 * stride) {
      const long i2 = i + stride;
      const bool two = i2 < quads;
      const f32x4 ea = e4[i], pa = p4[i];
      const f32x4 eb = two ? e4[i2] : ea, pb = two ? p4[i2] : pa;
      e4[i] = ema_quad(ea, pa, w);
      if (two) e4[i2] = ema_quad(eb, pb, w);
    }
  }
  // the floats in front of the first quad and behind the last one (everything when quads == 0)
  const long body = quads * 4, rest = n - body;
  for (long r = tid; r < rest; r += stride) {
    const long i = r < head ? r : r + body;
    ema[i] = ema_one(ema[i], p[i], w);
  }
}

__global__ __launch_bounds__(kEmaThreads) void buffer_swap_kernel(float* __restrict__ a, float* __restrict__ b, long n, long head,
                                                                  long quads) {
  const long tid = (long)blockIdx.x * kEmaThreads + threadIdx.x;
  const long stride = (long)gridDim.x * kEmaThreads;
  if (quads > 0) {
    f32x4* a4 = reinterpret_cast<f32x4*>(a + head);
    f32x4* b4 = reinterpret_cast<f32x4*>(b + head);
    for (long i = tid; i < quads; i += 2 * stride) {
      const long i2 = i + stride;
      const bool two = i2 < quads;
      const f32x4 aa = a4[i], ba = b4[i];
      const f32x4 ab = two ? a4[i2] : aa, bb = two ? b4[i2] : ba;
      a4[i] = ba;
      b4[i] = aa;
      if (two) {
        a4[i2] = bb;
        b4[i2] = ab;
      }
    }
  }
  const long body = quads * 4, rest = n - body;
  for (long r = tid; r < rest; r += stride) {
    const long i = r < head ? r : r + body;
    const float x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
}

namespace {

// What both launchers refuse, and the split of [0, n) into head floats, whole quads and the rest (gradaccum.hip's).
struct EmaGeometry {
  long head, quads;
  unsigned wgs;
};

bool ema_geometry(const void* first, const void* second, long n, EmaGeometry* out) {
  if (!first || !second || n <= 0) return false;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(first), b0 = reinterpret_cast<uintptr_t>(second), bytes = (uintptr_t)n * 4;
  if ((a0 | b0) % 4 != 0) return false;
  if (a0 < b0 + bytes && b0 < a0 + bytes) return false;      // both are __restrict__: the ranges must not overlap
  long head = (long)(((16 - b0 % 16) % 16) / 4);
  if (head > n) head = n;
  long quads = (n - head) / 4;
  if ((a0 + (uintptr_t)head * 4) % 16 != 0) {                // the buffers' 16-byte phases differ: float by float throughout
    head = 0;
    quads = 0;
  }
  const long rest = n - 4 * quads;
  long threads = (quads + 1) / 2;                            // two quads per thread and turn
  if (threads < rest) threads = rest;
  long wgs = (threads + kEmaThreads - 1) / kEmaThreads;
  if (wgs > kEmaMaxWgs) wgs = kEmaMaxWgs;
  if (wgs < 1) wgs = 1;
  out->head = head;
  out->quads = quads;
  out->wgs = (unsigned)wgs;
  return true;
}

}  // namespace

int launch_ema_update(float* ema, const float* p, long n, float one_minus_decay, hipStream_t st) {
  EmaGeometry g;
  if (!ema_geometry(ema, p, n, &g)) return kErrBadArg;
  if (!std::isfinite(one_minus_decay) || !(one_minus_decay > 0.f && one_minus_decay < 1.f)) return kErrBadArg;
  ProfScope ps("ema_update_kernel", st, 2.0 * (double)n, 12.0 * (double)n);
  hipLaunchKernelGGL(ema_update_kernel, dim3(g.wgs), dim3(kEmaThreads), 0, st, ema, p, n, g.head, g.quads, one_minus_decay);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_buffer_swap(float* a, float* b, long n, hipStream_t st) {
  EmaGeometry g;
  if (!ema_geometry(a, b, n, &g)) return kErrBadArg;
  ProfScope ps("buffer_swap_kernel", st, 0.0, 16.0 * (double)n);
  hipLaunchKernelGGL(buffer_swap_kernel, dim3(g.wgs), dim3(kEmaThreads), 0, st, a, b, n, g.head, g.quads);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
