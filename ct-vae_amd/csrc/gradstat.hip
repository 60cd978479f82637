// Gradient tracking (trainer_params.track_grad_norm, exp_params.watch_gradients; optim.py GradientTracker): per-parameter norms and
// 64-bin histograms straight from the flat gradient buffer, in three launches and without a host round trip in between.
//   grad_stats_kernel     one workgroup per chunk: sum |v|^p (double), max |v|, min / max over the finite values, the count of
//                         non-finite ones -> one partial per chunk
//   grad_stats_finalize_kernel   one workgroup per segment: its chunks' partials in a fixed order -> the segment's record; zeroes the
//                         segment's 64 bin counts; workgroup 0 also copies the caller's block-flag words next to the records
//   grad_hist_kernel      one workgroup per chunk: the finite values into the 64 bins between the segment's finished min and max
//
// A SEGMENT names the elements of one parameter inside the buffer: (base, rows, period, col_lo, width) stands for the elements
// base + r * period + col_lo + c, r < rows, c < width.  A contiguous parameter is one row; the heads of a PackedLinearGroup are
// column ranges of the rows of one block.  Element e of a segment (row-major, e = r * width + c) is what the chunk list counts in:
// chunk k covers elements [first[k], first[k] + kChunk) of segment seg[k], cut at the segment's end.  The list is built on the host,
// once per table, from the descriptors alone, so no launch geometry and no buffer size depends on the gradient's values.  Thread t
// of a workgroup takes elements first + t, first + t + 256, ...: the lanes of a wave read 64 neighbouring floats of a row.
//
// The value every kernel works on is v = fl32(g * scale) (one correctly rounded fp32 multiply, never contracted into what
// follows).  Sums run in double: the squares of fp32 values are exact there, every thread sums its (at most 16) terms in element
// order, the 64 lanes of a wave merge by a fixed butterfly, the four waves and then the chunks in index order -- no floating-point
// atomic anywhere, so a norm is a function of the values and the table alone.  max |v| keeps a NaN once it has met one (as
// torch.norm(inf) does); the sum does so by itself.  min and max order the finite values by their bits (-0 below +0), so they are
// exact whatever order the merges run in.
//
// Bins follow torch.histc on the CPU, in fp32: bin = min((long)((v - lo) / (hi - lo) * 64.0f), 63) with a correctly rounded
// division; lo == hi is widened to lo - 1, hi + 1.  A quotient that is not a number (hi - lo overflowed, or lo - 1 == lo) counts
// in bin 0.  Bin counts are integers: LDS atomics per wave, one global integer atomic per non-empty bin and chunk -- integer sums
// do not depend on their order.
//
// `g` is read only; every address is checked against n.  Writes go to the partials and to the caller's output arrays alone.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kStatThreads = 256, kStatPerThread = 16;
constexpr long kStatChunk = (long)kStatThreads * kStatPerThread;      // elements per chunk
constexpr int kStatBins = 64;
constexpr int kNormTwo = 0, kNormOne = 1, kNormPow = 2, kNormInf = 3;

struct SegDesc {
  long base, rows, period, col_lo, width;
};

// order-preserving integer key of an fp32 value: a < b as floats (and -0 < +0) iff key(a) < key(b)
__device__ __forceinline__ int stat_key(float v) {
  const int b = __builtin_bit_cast(int, v);
  return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float stat_unkey(int k) { return __builtin_bit_cast(float, k ^ ((k >> 31) & 0x7fffffff)); }
constexpr int kKeyPosInf = 0x7f800000;            // key(+inf); key(-inf) = ~key(+inf)

__device__ __forceinline__ float amax_merge(float a, float b) { return (b > a || b != b) ? b : a; }   // NaN is kept once met

__device__ __forceinline__ long seg_address(const SegDesc& d, long e) {
  if (d.rows == 1) return d.base + d.col_lo + e;
  const long r = e / d.width;
  return d.base + r * d.period + d.col_lo + (e - r * d.width);
}

template <int KIND>
__global__ __launch_bounds__(kStatThreads) void grad_stats_kernel(const float* __restrict__ g, long n, float scale, double p,
                                                                  const SegDesc* __restrict__ seg, const int* __restrict__ chunk_seg,
                                                                  const long* __restrict__ chunk_first, double* __restrict__ part_sum,
                                                                  float* __restrict__ part_f, int* __restrict__ part_bad) {
  __shared__ double s_sum[4];
  __shared__ float s_amax[4];
  __shared__ int s_min[4], s_max[4], s_bad[4];
  const int k = blockIdx.x;
  const SegDesc d = seg[chunk_seg[k]];
  const long first = chunk_first[k], count = d.rows * d.width;
  double sum = 0.0;
  float amax = 0.f;
  int kmin = kKeyPosInf, kmax = ~kKeyPosInf, bad = 0;
#pragma unroll 4
  for (int j = 0; j < kStatPerThread; ++j) {
    const long e = first + threadIdx.x + (long)j * kStatThreads;
    if (e >= count) break;
    const long a = seg_address(d, e);
    if (a < 0 || a >= n) continue;
    const float v = __fmul_rn(g[a], scale);
    const float av = fabsf(v);
    amax = amax_merge(amax, av);
    if constexpr (KIND == kNormTwo) sum += (double)v * (double)v;
    else if constexpr (KIND == kNormOne) sum += (double)av;
    else if constexpr (KIND == kNormPow) sum += pow((double)av, p);
    if (av < __builtin_inff()) {
      const int key = stat_key(v);
      kmin = key < kmin ? key : kmin;
      kmax = key > kmax ? key : kmax;
    } else {
      ++bad;
    }
  }
  sum = wave_sum_d(sum);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    amax = amax_merge(amax, __shfl_xor(amax, o, 64));
    const int m = __shfl_xor(kmin, o, 64), M = __shfl_xor(kmax, o, 64);
    kmin = m < kmin ? m : kmin;
    kmax = M > kmax ? M : kmax;
    bad += __shfl_xor(bad, o, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_sum[w] = sum;
    s_amax[w] = amax;
    s_min[w] = kmin;
    s_max[w] = kmax;
    s_bad[w] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = s_sum[0];
    float am = s_amax[0];
    int m = s_min[0], M = s_max[0], b = s_bad[0];
    for (int i = 1; i < 4; ++i) {
      t += s_sum[i];
      am = amax_merge(am, s_amax[i]);
      m = s_min[i] < m ? s_min[i] : m;
      M = s_max[i] > M ? s_max[i] : M;
      b += s_bad[i];
    }
    part_sum[k] = t;
    part_f[3 * (long)k] = am;
    part_f[3 * (long)k + 1] = stat_unkey(m);       // +inf / -inf where the chunk holds no finite value
    part_f[3 * (long)k + 2] = stat_unkey(M);
    part_bad[k] = b;
  }
}

// One workgroup per segment.  Thread t merges chunks begin + t, begin + t + 256, ... in that order, then the 256 threads merge by
// a fixed tree in LDS.
__global__ __launch_bounds__(kStatThreads) void grad_stats_finalize_kernel(const int* __restrict__ seg_chunk_begin,
                                                                           const double* __restrict__ part_sum,
                                                                           const float* __restrict__ part_f,
                                                                           const int* __restrict__ part_bad, double* __restrict__ out_sum,
                                                                           float* __restrict__ out_range, int* __restrict__ out_bad,
                                                                           int* __restrict__ out_hist, const int* __restrict__ flags_in,
                                                                           int* __restrict__ flags_out, int nflags) {
  __shared__ double s_sum[kStatThreads];
  __shared__ float s_amax[kStatThreads];
  __shared__ int s_min[kStatThreads], s_max[kStatThreads], s_bad[kStatThreads];
  const int s = blockIdx.x, t = threadIdx.x;
  const int begin = seg_chunk_begin[s], end = seg_chunk_begin[s + 1];
  double sum = 0.0;
  float amax = 0.f;
  int kmin = kKeyPosInf, kmax = ~kKeyPosInf, bad = 0;
  for (int k = begin + t; k < end; k += kStatThreads) {
    sum += part_sum[k];
    amax = amax_merge(amax, part_f[3 * (long)k]);
    const int m = stat_key(part_f[3 * (long)k + 1]), M = stat_key(part_f[3 * (long)k + 2]);
    kmin = m < kmin ? m : kmin;
    kmax = M > kmax ? M : kmax;
    bad += part_bad[k];
  }
  s_sum[t] = sum;
  s_amax[t] = amax;
  s_min[t] = kmin;
  s_max[t] = kmax;
  s_bad[t] = bad;
  __syncthreads();
  for (int o = kStatThreads / 2; o > 0; o >>= 1) {
    if (t < o) {
      s_sum[t] += s_sum[t + o];
      s_amax[t] = amax_merge(s_amax[t], s_amax[t + o]);
      s_min[t] = s_min[t + o] < s_min[t] ? s_min[t + o] : s_min[t];
      s_max[t] = s_max[t + o] > s_max[t] ? s_max[t + o] : s_max[t];
      s_bad[t] += s_bad[t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    out_sum[2 * (long)s] = s_sum[0];
    out_sum[2 * (long)s + 1] = (double)s_amax[0];
    out_range[2 * (long)s] = stat_unkey(s_min[0]);           // +inf, -inf: no finite value in the segment
    out_range[2 * (long)s + 1] = stat_unkey(s_max[0]);
    out_bad[s] = s_bad[0];
  }
  if (t < kStatBins) out_hist[(long)s * kStatBins + t] = 0;
  if (s == 0)
    for (int i = t; i < nflags; i += kStatThreads) flags_out[i] = flags_in[i];
}

__global__ __launch_bounds__(kStatThreads) void grad_hist_kernel(const float* __restrict__ g, long n, float scale,
                                                                 const SegDesc* __restrict__ seg, const int* __restrict__ chunk_seg,
                                                                 const long* __restrict__ chunk_first,
                                                                 const float* __restrict__ out_range, int* __restrict__ out_hist) {
  __shared__ int s_bins[4][kStatBins];
  const int k = blockIdx.x, s = chunk_seg[k];
  const SegDesc d = seg[s];
  float lo = out_range[2 * (long)s], hi = out_range[2 * (long)s + 1];
  if (!(lo <= hi)) return;                          // no finite value (lo = +inf, hi = -inf): the counts stay zero
  if (lo == hi) {
    lo = __fsub_rn(lo, 1.f);
    hi = __fadd_rn(hi, 1.f);
  }
  const float span = __fsub_rn(hi, lo);
  const int w = threadIdx.x >> 6;
  s_bins[w][threadIdx.x & 63] = 0;
  __syncthreads();
  const long first = chunk_first[k], count = d.rows * d.width;
#pragma unroll 4
  for (int j = 0; j < kStatPerThread; ++j) {
    const long e = first + threadIdx.x + (long)j * kStatThreads;
    if (e >= count) break;
    const long a = seg_address(d, e);
    if (a < 0 || a >= n) continue;
    const float v = __fmul_rn(g[a], scale);
    if (!(fabsf(v) < __builtin_inff())) continue;
    const float q = __fmul_rn(__fdiv_rn(__fsub_rn(v, lo), span), (float)kStatBins);
    const int bin = q >= (float)kStatBins ? kStatBins - 1 : (q >= 0.f ? (int)q : 0);     // (a NaN quotient: bin 0)
    atomicAdd(&s_bins[w][bin], 1);
  }
  __syncthreads();
  if (threadIdx.x < kStatBins) {
    const int c = s_bins[0][threadIdx.x] + s_bins[1][threadIdx.x] + s_bins[2][threadIdx.x] + s_bins[3][threadIdx.x];
    if (c) atomicAdd(&out_hist[(long)s * kStatBins + threadIdx.x], c);
  }
}

size_t grad_segment_chunk_floats() { return (size_t)kStatChunk; }

int launch_grad_segment_stats(const float* g, long n, float scale, float p, const long* seg, int nseg, const int* chunk_seg,
                              const long* chunk_first, const int* seg_chunk_begin, int nchunks, double* part_sum, float* part_f,
                              int* part_bad, double* out_sum, float* out_range, int* out_bad, int* out_hist, const int* flags_in,
                              int* flags_out, int nflags, hipStream_t st) {
  if (!g || n <= 0 || !seg || nseg < 1 || !chunk_seg || !chunk_first || !seg_chunk_begin || nchunks < nseg) return kErrBadArg;
  if (!part_sum || !part_f || !part_bad || !out_sum || !out_range || !out_bad || !out_hist) return kErrBadArg;
  if (nflags < 0 || (nflags > 0 && (!flags_in || !flags_out))) return kErrBadArg;
  if (!(p > 0.f)) return kErrBadArg;                  // (NaN included); +inf: the max alone
  static_assert(sizeof(SegDesc) == 5 * sizeof(long), "a descriptor is five 64-bit words");
  const SegDesc* sd = reinterpret_cast<const SegDesc*>(seg);
  const int kind = p == 2.f ? kNormTwo : (p == 1.f ? kNormOne : (p == __builtin_inff() ? kNormInf : kNormPow));
  const dim3 grid((unsigned)nchunks), block(kStatThreads);
  {
    ProfScope ps("grad_stats_kernel", st, 0.0, 4.0 * (double)nchunks * (double)kStatChunk);
    if (kind == kNormTwo)
      hipLaunchKernelGGL(grad_stats_kernel<kNormTwo>, grid, block, 0, st, g, n, scale, (double)p, sd, chunk_seg, chunk_first, part_sum,
                         part_f, part_bad);
    else if (kind == kNormOne)
      hipLaunchKernelGGL(grad_stats_kernel<kNormOne>, grid, block, 0, st, g, n, scale, (double)p, sd, chunk_seg, chunk_first, part_sum,
                         part_f, part_bad);
    else if (kind == kNormPow)
      hipLaunchKernelGGL(grad_stats_kernel<kNormPow>, grid, block, 0, st, g, n, scale, (double)p, sd, chunk_seg, chunk_first, part_sum,
                         part_f, part_bad);
    else
      hipLaunchKernelGGL(grad_stats_kernel<kNormInf>, grid, block, 0, st, g, n, scale, (double)p, sd, chunk_seg, chunk_first, part_sum,
                         part_f, part_bad);
    CTVAE_LAUNCH_CHECK();
  }
  {
    ProfScope ps("grad_stats_finalize_kernel", st, 0.0, 24.0 * (double)nchunks);
    hipLaunchKernelGGL(grad_stats_finalize_kernel, dim3((unsigned)nseg), block, 0, st, seg_chunk_begin, part_sum, part_f, part_bad,
                       out_sum, out_range, out_bad, out_hist, flags_in, flags_out, nflags);
    CTVAE_LAUNCH_CHECK();
  }
  return 0;
}

int launch_grad_segment_hist(const float* g, long n, float scale, const long* seg, int nseg, const int* chunk_seg,
                             const long* chunk_first, int nchunks, const float* out_range, int* out_hist, hipStream_t st) {
  if (!g || n <= 0 || !seg || nseg < 1 || !chunk_seg || !chunk_first || nchunks < nseg || !out_range || !out_hist) return kErrBadArg;
  ProfScope ps("grad_hist_kernel", st, 0.0, 4.0 * (double)nchunks * (double)kStatChunk);
  hipLaunchKernelGGL(grad_hist_kernel, dim3((unsigned)nchunks), dim3(kStatThreads), 0, st, g, n, scale,
                     reinterpret_cast<const SegDesc*>(seg), chunk_seg, chunk_first, out_range, out_hist);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
