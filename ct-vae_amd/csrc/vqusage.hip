// Codebook usage of the vector-quantised models (exp_params.codebook_stats / codebook_restart_every; optim.py: CodebookUsage):
//   vq_usage_kernel      counts[c][k] += number of indices of codebook c equal to k        int64 inds [B][C][HW] -> int64 [C][K]
//   vq_pool_fill_kernel  pool[0 : rows) = latents[0 : rows), word for word                 restart candidates, rows = min(P, R)
//   vq_usage_fill_kernel both in ONE launch (the training forward's: one graph node instead of two)
//   vq_restart_kernel    E_c[k][:] = pool[row][c : c + Dc) (or a gathered row), both Adam moments of those elements = 0
//   vq_restart_gather_kernel   rows[i][:] = pool[row_i][c_i : c_i + Dc)                    the data-parallel split: gather, broadcast,
//                                                                                         scatter through vq_restart_kernel
//
// Usage.  The indices are one flat array of n = B * C * HW 64-bit words; element e belongs to codebook (e / HW) % C.  One pass:
// every lane reads one index per load (a wave reads 512 contiguous bytes), four independent loads in flight per turn, grid-stride
// over at most kUsageMaxWgs workgroups.  A workgroup keeps a histogram of C * K 32-bit words in LDS (integer LDS atomics; a
// workgroup's share of 2^31 indices stays far below 2^32) and hands every non-zero word to the global counts with one 64-bit
// integer atomic add -- so a workgroup is given at least kUsageIndicesPerWg indices: with one index per thread every workgroup
// would flush nearly one global atomic per index onto the same C * K addresses (MCQ-VAE at bs 256: 65536 of them instead of 4096).
// Integer adds commute, so the result is exact and independent of the order; there is no float atomic.  An index outside
// [0, K) is counted in `invalid` (through one LDS word per workgroup) and nowhere else.  Covered: 1 <= K <= kUsageMaxK,
// C * K <= kUsageMaxWords (32 KiB of LDS); everything else is refused without a launch.  All arguments are pointers and shape
// integers, so a captured launch replays correctly.  The loop is latency-bound, not bandwidth-bound (MCQ-VAE at bs 256:
// 65536 indices, 512 KiB), so 8-byte loads are kept and the tail needs no special case.
//
// Pool fill.  min(P, R) * D contiguous 32-bit words from the front of the NHWC latents to the front of the pool: 16-byte
// accesses when both pointers sit on a 16-byte boundary, the words behind the last whole quad (D need not be a multiple of 4)
// one by one; loads and stores only, so NaN payloads and -0 pass.  Rows behind min(P, R) are not touched.
//
// Restart.  One thread per (entry, d); an entry is three 64-bit words (c, k, row).  The source channel is c + d, not c * Dc + d:
// codebook c is compared against latents[:, c : c + Dc) (the slice quirk, models/mcq_vae.py), and the restarted code has to lie
// where those latents are.  The host has checked every entry; the kernel skips an entry outside the ranges all the same, so no
// word outside the three buffers' listed rows is ever written.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kUsageThreads = 256, kUsageMaxWgs = 256;      // one resident workgroup per CU; beyond: grid-stride
constexpr int kUsageIndicesPerWg = 4096;                    // at least this many indices per workgroup (16 per thread)
constexpr int kUsageMaxK = 512, kUsageMaxWords = 8192;      // LDS histogram: C * K 32-bit words
constexpr int kFillThreads = 256, kFillMaxWgs = 1024;
constexpr int kRestartThreads = 256;

struct UsageArgs {
  const long long* inds;
  unsigned long long* counts;
  unsigned long long* invalid;
  long n;
  int C, HW, K;
};

struct FillArgs {
  const unsigned* src;
  unsigned* dst;
  long n, quads;
};

// workgroup `wg` of `wgs` (every thread of the workgroup calls it: it synchronises)
__device__ __forceinline__ void usage_body(const UsageArgs& a, unsigned* hist, int wg, int wgs) {
  const int words = a.C * a.K;          // hist: [C * K] + one word for the indices outside [0, K)
  for (int j = threadIdx.x; j <= words; j += kUsageThreads) hist[j] = 0u;
  __syncthreads();
  const long stride = (long)wgs * kUsageThreads;
  for (long e0 = (long)wg * kUsageThreads + threadIdx.x; e0 < a.n; e0 += 4 * stride) {
    long long k[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long e = e0 + j * stride;
      k[j] = e < a.n ? a.inds[e] : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long e = e0 + j * stride;
      if (e < a.n) {
        const int c = (int)((e / a.HW) % a.C);
        const bool ok = k[j] >= 0 && k[j] < (long long)a.K;
        atomicAdd(&hist[ok ? c * a.K + (int)k[j] : words], 1u);
      }
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j <= words; j += kUsageThreads) {
    const unsigned h = hist[j];
    if (h != 0u) atomicAdd(j < words ? &a.counts[j] : a.invalid, (unsigned long long)h);
  }
}

__device__ __forceinline__ void fill_body(const FillArgs& a, int wg, int wgs) {
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  const long tid = (long)wg * kFillThreads + threadIdx.x;
  const long stride = (long)wgs * kFillThreads;
  const u32x4* s4 = reinterpret_cast<const u32x4*>(a.src);
  u32x4* d4 = reinterpret_cast<u32x4*>(a.dst);
  for (long i = tid; i < a.quads; i += stride) d4[i] = s4[i];
  for (long i = a.quads * 4 + tid; i < a.n; i += stride) a.dst[i] = a.src[i];
}

__global__ __launch_bounds__(kUsageThreads) void vq_usage_kernel(UsageArgs a) {
  extern __shared__ unsigned hist[];
  usage_body(a, hist, (int)blockIdx.x, (int)gridDim.x);
}

__global__ __launch_bounds__(kFillThreads) void vq_pool_fill_kernel(FillArgs a) {
  fill_body(a, (int)blockIdx.x, (int)gridDim.x);
}

// the first usage_wgs workgroups count, the others copy
static_assert(kUsageThreads == kFillThreads, "one launch, one workgroup size");
__global__ __launch_bounds__(kUsageThreads) void vq_usage_fill_kernel(UsageArgs u, int usage_wgs, FillArgs f) {
  extern __shared__ unsigned hist[];
  const int wg = (int)blockIdx.x;
  if (wg < usage_wgs)
    usage_body(u, hist, wg, usage_wgs);
  else
    fill_body(f, wg - usage_wgs, (int)gridDim.x - usage_wgs);
}

struct RestartEntry {
  long long c, k, row;
};

// rows != nullptr: the code's new value is rows[i][d] (gathered, maybe on another rank); else pool[row][c + d]
__global__ __launch_bounds__(kRestartThreads) void vq_restart_kernel(const RestartEntry* __restrict__ list, int n,
                                                                     const unsigned* __restrict__ pool, int valid_rows, int D,
                                                                     const unsigned* __restrict__ rows, unsigned* __restrict__ cb,
                                                                     unsigned* __restrict__ m, unsigned* __restrict__ v, int C, int K,
                                                                     int Dc) {
  const long t = (long)blockIdx.x * kRestartThreads + threadIdx.x;
  if (t >= (long)n * Dc) return;
  const int i = (int)(t / Dc), d = (int)(t - (long)i * Dc);
  const RestartEntry e = list[i];
  const bool dst_ok = e.c >= 0 && e.c < C && e.k >= 0 && e.k < K;
  const bool src_ok = rows != nullptr || (e.row >= 0 && e.row < valid_rows);
  if (!dst_ok || !src_ok) return;
  const long dst = ((long)e.c * K + e.k) * Dc + d;
  cb[dst] = rows ? rows[(long)i * Dc + d] : pool[e.row * D + e.c + d];
  m[dst] = 0u;
  v[dst] = 0u;
}

__global__ __launch_bounds__(kRestartThreads) void vq_restart_gather_kernel(const RestartEntry* __restrict__ list, int n,
                                                                            const unsigned* __restrict__ pool, int valid_rows, int D,
                                                                            int C, int Dc, unsigned* __restrict__ rows) {
  const long t = (long)blockIdx.x * kRestartThreads + threadIdx.x;
  if (t >= (long)n * Dc) return;
  const int i = (int)(t / Dc), d = (int)(t - (long)i * Dc);
  const RestartEntry e = list[i];
  if (e.c < 0 || e.c >= C || e.row < 0 || e.row >= valid_rows) return;
  rows[t] = pool[e.row * D + e.c + d];
}

size_t vq_usage_pass_indices() { return (size_t)kUsageIndicesPerWg * kUsageMaxWgs; }

namespace {

struct UsagePlan {
  UsageArgs args;
  unsigned wgs;
  size_t lds;
};

bool usage_plan(const long* inds, long* counts, long* invalid, int B, int C, int HW, int K, UsagePlan* out) {
  if (!inds || !counts || !invalid || B < 1 || C < 1 || HW < 1) return false;
  if (K < 1 || K > kUsageMaxK || (long)C * K > kUsageMaxWords) return false;
  if ((reinterpret_cast<uintptr_t>(inds) | reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(invalid)) % 8 != 0)
    return false;
  const long n = (long)B * C * HW;
  long wgs = (n + kUsageIndicesPerWg - 1) / kUsageIndicesPerWg;
  if (wgs > kUsageMaxWgs) wgs = kUsageMaxWgs;
  out->args = UsageArgs{reinterpret_cast<const long long*>(inds), reinterpret_cast<unsigned long long*>(counts),
                        reinterpret_cast<unsigned long long*>(invalid), n, C, HW, K};
  out->wgs = (unsigned)wgs;
  out->lds = ((size_t)C * K + 1) * sizeof(unsigned);
  return true;
}

struct FillPlan {
  FillArgs args;
  unsigned wgs;
};

bool fill_plan(const float* latents, float* pool, long P, int D, long R, FillPlan* out) {
  if (!latents || !pool || P < 1 || D < 1 || R < 1) return false;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(latents), d0 = reinterpret_cast<uintptr_t>(pool);
  if ((s0 | d0) % 4 != 0) return false;
  const long n = (P < R ? P : R) * (long)D;
  if (s0 < d0 + (uintptr_t)n * 4 && d0 < s0 + (uintptr_t)n * 4) return false;      // (both are __restrict__-like: no overlap)
  const long quads = (s0 | d0) % 16 == 0 ? n / 4 : 0;
  const long threads = quads > n - 4 * quads ? quads : n - 4 * quads;
  long wgs = (threads + kFillThreads - 1) / kFillThreads;
  if (wgs > kFillMaxWgs) wgs = kFillMaxWgs;
  out->args = FillArgs{reinterpret_cast<const unsigned*>(latents), reinterpret_cast<unsigned*>(pool), n, quads};
  out->wgs = (unsigned)wgs;
  return true;
}

}  // namespace

int launch_vq_usage(const long* inds, long* counts, long* invalid, int B, int C, int HW, int K, hipStream_t st) {
  UsagePlan u;
  if (!usage_plan(inds, counts, invalid, B, C, HW, K, &u)) return kErrBadArg;
  ProfScope ps("vq_usage_kernel", st, 0.0, 8.0 * (double)u.args.n);
  hipLaunchKernelGGL(vq_usage_kernel, dim3(u.wgs), dim3(kUsageThreads), u.lds, st, u.args);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_vq_pool_fill(const float* latents, float* pool, long P, int D, long R, hipStream_t st) {
  FillPlan f;
  if (!fill_plan(latents, pool, P, D, R, &f)) return kErrBadArg;
  ProfScope ps("vq_pool_fill_kernel", st, 0.0, 8.0 * (double)f.args.n);
  hipLaunchKernelGGL(vq_pool_fill_kernel, dim3(f.wgs), dim3(kFillThreads), 0, st, f.args);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_vq_usage_pool_fill(const long* inds, long* counts, long* invalid, int B, int C, int HW, int K, const float* latents,
                              float* pool, long P, int D, long R, hipStream_t st) {
  UsagePlan u;
  FillPlan f;
  if (!usage_plan(inds, counts, invalid, B, C, HW, K, &u) || !fill_plan(latents, pool, P, D, R, &f)) return kErrBadArg;
  ProfScope ps("vq_usage_fill_kernel", st, 0.0, 8.0 * (double)u.args.n + 8.0 * (double)f.args.n);
  hipLaunchKernelGGL(vq_usage_fill_kernel, dim3(u.wgs + f.wgs), dim3(kUsageThreads), u.lds, st, u.args, (int)u.wgs, f.args);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

namespace {

// what both restart launchers refuse; n == 0 is fine (and launches nothing)
bool restart_shape_ok(const long* list, int n, int valid_rows, int D, int C, int Dc) {
  if (n < 0 || valid_rows < 0 || D < 1 || C < 1 || Dc < 1) return false;
  if ((long)C - 1 + Dc > D) return false;                    // the last codebook's slice [C - 1, C - 1 + Dc) lies inside a row
  if (n > 0 && (!list || reinterpret_cast<uintptr_t>(list) % 8 != 0)) return false;
  return true;
}

unsigned restart_wgs(int n, int Dc) { return (unsigned)(((long)n * Dc + kRestartThreads - 1) / kRestartThreads); }

}  // namespace

int launch_vq_restart(const long* list, int n, const float* pool, int valid_rows, int D, const float* rows, float* codebooks,
                      float* exp_avg, float* exp_avg_sq, int C, int K, int Dc, hipStream_t st) {
  if (!restart_shape_ok(list, n, valid_rows, D, C, Dc) || K < 1) return kErrBadArg;
  if (n == 0) return 0;
  if (!codebooks || !exp_avg || !exp_avg_sq || (!rows && (!pool || valid_rows < 1))) return kErrBadArg;
  ProfScope ps("vq_restart_kernel", st, 0.0, 16.0 * (double)n * Dc);
  hipLaunchKernelGGL(vq_restart_kernel, dim3(restart_wgs(n, Dc)), dim3(kRestartThreads), 0, st,
                     reinterpret_cast<const RestartEntry*>(list), n, reinterpret_cast<const unsigned*>(pool), valid_rows, D,
                     reinterpret_cast<const unsigned*>(rows), reinterpret_cast<unsigned*>(codebooks),
                     reinterpret_cast<unsigned*>(exp_avg), reinterpret_cast<unsigned*>(exp_avg_sq), C, K, Dc);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_vq_restart_gather(const long* list, int n, const float* pool, int valid_rows, int D, int C, int Dc, float* rows,
                             hipStream_t st) {
  if (!restart_shape_ok(list, n, valid_rows, D, C, Dc)) return kErrBadArg;
  if (n == 0) return 0;
  if (!pool || !rows || valid_rows < 1) return kErrBadArg;
  ProfScope ps("vq_restart_gather_kernel", st, 0.0, 8.0 * (double)n * Dc);
  hipLaunchKernelGGL(vq_restart_gather_kernel, dim3(restart_wgs(n, Dc)), dim3(kRestartThreads), 0, st,
                     reinterpret_cast<const RestartEntry*>(list), n, reinterpret_cast<const unsigned*>(pool), valid_rows, D, C, Dc,
                     reinterpret_cast<unsigned*>(rows));
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
