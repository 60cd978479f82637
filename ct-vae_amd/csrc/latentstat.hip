// Latent usage of the Gaussian models (exp_params.latent_stats; latentstats.py: LatentStats):
//   latent_accumulate_kernel   one batch of posterior parameters mu, logvar [B][L] (fp32, a row pitch each) added into persistent
//                              accumulators: float64 sums of the per-element KL, of mu, of sigma^2 and of mu mu^T, int32 counts of
//                              the non-finite elements per column and of the rows
//
// Ownership.  Every accumulator element has ONE owner thread in ONE workgroup, which loads the stored value, adds the batch's rows
// in ascending order and stores it back -- graph_accumulate_kernel's rule (graphstat.hip): no atomics, no reduction tree, and
// every element ends up as  (((old + t_0) + t_1) + ...)  over the rows 0, 1, ..., whatever the launch geometry and however the
// rows were split into calls.
//
// Workgroups [0, nt * nt), nt = ceil(L / 16): tile (ti, tj) of cov_sum, 16 x 16 elements, one per thread.  The walk: kCovRows rows
// at a time, the tile's two column ranges of mu go to LDS (the two ranges of a diagonal tile are the same and are staged twice,
// which is cheaper than a second code path); then every thread adds its product row by row.  The product of two fp32 values has
// at most 48 significant bits, so it is exact in double and  acc + a * b  rounds once whether or not the compiler contracts it
// into an FMA: the sums equal a numpy float64 loop bit for bit, and cov_sum[i][j] == cov_sum[j][i] to the bit because the
// products commute.  The whole matrix is computed: at L <= 1024 the mirror half is a few microseconds, and a reader of the raw
// accumulators needs no convention.  No f64 MFMA: its internal K order is not the row order.
//
// Workgroups [nt * nt, nt * nt + ceil(L / 32)): 32 columns of the four [L] vectors.  The double exp is most of a row's work (with
// one thread walking its column alone the launch took 14 us at B = 64 and 42 us at B = 256, and more loads in flight made it
// slower, not faster: DESIGN 4.19), and it does not depend on the sum, so it is spread out: thread (q, c) = (tid / 32, tid % 32)
// forms the terms of rows q, q + 8, ... of a turn of kVecRows rows for column c and leaves them in LDS,
//   m = mu, lv = logvar, s2 = exp(lv);  t_kl = 0.5 * (((m * m + s2) - lv) - 1)      (all in double; m * m is exact, so contraction
//                                                                                   does not move the result)
// and the column's owner, thread (0, c), adds kl_sum += t_kl, mu_sum += m, sig2_sum += s2 in ascending row order.  nonfinite
// counts the elements whose mu or logvar is NaN or +-inf (exponent bits all ones); such values still go into the sums.  Thread 0
// of the first of these workgroups adds B to rows[0].
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kLatThreads = 256;
constexpr int kCovTile = 16;            // a workgroup's tile of cov_sum: kCovTile x kCovTile, one element per thread
constexpr int kCovRows = 64;            // rows of mu staged per turn
constexpr int kVecCols = 32;            // columns of the [L] vectors per workgroup
constexpr int kVecRows = 32;            // rows whose terms are formed per turn: kLatThreads / kVecCols threads per column
constexpr int kLatentMaxL = 1024;       // cov_sum is L * L doubles: 8 MB here

__device__ __forceinline__ bool nonfinite_f32(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) == 0x7f800000u; }

__global__ __launch_bounds__(kLatThreads) void latent_accumulate_kernel(
    const float* __restrict__ mu, long mu_pitch, const float* __restrict__ logvar, long lv_pitch, int B, int L, int nt,
    double* __restrict__ kl_sum, double* __restrict__ mu_sum, double* __restrict__ sig2_sum, double* __restrict__ cov_sum,
    int* __restrict__ nonfinite, int* __restrict__ rows) {
  __shared__ float sa[kCovRows][kCovTile];
  __shared__ float sb[kCovRows][kCovTile];
  __shared__ double t_kl[kVecRows][kVecCols];
  __shared__ double t_s2[kVecRows][kVecCols];
  __shared__ float t_mu[kVecRows][kVecCols];
  __shared__ int t_bad[kVecRows][kVecCols];
  const int tid = threadIdx.x;
  const int cov_tiles = nt * nt;
  if ((int)blockIdx.x >= cov_tiles) {                          // ---- 32 columns of the [L] vectors
    const int vb = (int)blockIdx.x - cov_tiles;
    const int c = tid & (kVecCols - 1), q = tid / kVecCols;    // q: 0 .. 7
    const int d = vb * kVecCols + c;
    const bool live = d < L, owner = live && q == 0;
    double kl = 0.0, sm = 0.0, ss = 0.0;
    int nf = 0;
    if (owner) {
      kl = kl_sum[d];
      sm = mu_sum[d];
      ss = sig2_sum[d];
      nf = nonfinite[d];
    }
    constexpr int kPer = kVecRows / (kLatThreads / kVecCols);  // rows per thread and turn: 4
    for (long r0 = 0; r0 < B; r0 += kVecRows) {                // (long: r0 + kVecRows may pass 2^31 - 1)
      const int nr = B - r0 < kVecRows ? (int)(B - r0) : kVecRows;
      float m[kPer], v[kPer];
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const int r = q + u * (kVecRows / kPer);
        const bool in = live && r < nr;
        m[u] = in ? mu[(r0 + r) * mu_pitch + d] : 0.f;
        v[u] = in ? logvar[(r0 + r) * lv_pitch + d] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kPer; ++u) {
        const int r = q + u * (kVecRows / kPer);
        const double md = (double)m[u], lv = (double)v[u];
        const double s2 = exp(lv);
        t_kl[r][c] = 0.5 * (((md * md + s2) - lv) - 1.0);
        t_s2[r][c] = s2;
        t_mu[r][c] = m[u];
        t_bad[r][c] = (nonfinite_f32(m[u]) || nonfinite_f32(v[u])) ? 1 : 0;
      }
      __syncthreads();
      if (owner) {
        for (int r = 0; r < nr; ++r) {
          kl += t_kl[r][c];
          sm += (double)t_mu[r][c];
          ss += t_s2[r][c];
          nf += t_bad[r][c];
        }
      }
      __syncthreads();                                         // the terms are rewritten by the next rows
    }
    if (owner) {
      kl_sum[d] = kl;
      mu_sum[d] = sm;
      sig2_sum[d] = ss;
      nonfinite[d] = nf;
    }
    if (vb == 0 && tid == 0) rows[0] += B;                     // the only writer of this word
    return;
  }
  // ---- tile (ti, tj) of cov_sum
  const int ti = (int)blockIdx.x / nt, tj = (int)blockIdx.x - ti * nt;
  const int i0 = ti * kCovTile, j0 = tj * kCovTile;
  const int ty = tid >> 4, tx = tid & 15;
  const int i = i0 + ty, j = j0 + tx;                          // this thread's element
  const bool live = i < L && j < L;
  double acc = live ? cov_sum[(long)i * L + j] : 0.0;
  for (long r0 = 0; r0 < B; r0 += kCovRows) {
    const int nr = B - r0 < kCovRows ? (int)(B - r0) : kCovRows;
#pragma unroll
    for (int k = 0; k < kCovRows / 16; ++k) {                  // staging: 16 lanes on one row's 16 columns, 16 rows per pass
      const int r = ty + 16 * k;
      const bool in = r < nr;
      const float* row = mu + (r0 + (in ? r : 0)) * mu_pitch;
      sa[r][tx] = (in && i0 + tx < L) ? row[i0 + tx] : 0.f;
      sb[r][tx] = (in && j0 + tx < L) ? row[j0 + tx] : 0.f;
    }
    __syncthreads();
    for (int r = 0; r < nr; ++r) acc += (double)sa[r][ty] * (double)sb[r][tx];
    __syncthreads();                                           // sa / sb are rewritten by the next rows
  }
  if (live) cov_sum[(long)i * L + j] = acc;
}

int launch_latent_accumulate(const float* mu, long mu_pitch, const float* logvar, long lv_pitch, int B, int L, double* kl_sum,
                             double* mu_sum, double* sig2_sum, double* cov_sum, int* nonfinite, int* rows, hipStream_t st) {
  if (!mu || !logvar || !kl_sum || !mu_sum || !sig2_sum || !cov_sum || !nonfinite || !rows) return kErrBadArg;
  if (B < 0 || L < 1 || L > kLatentMaxL || mu_pitch < L || lv_pitch < L) return kErrBadArg;
  if (B == 0) return 0;
  const int nt = (L + kCovTile - 1) / kCovTile;
  const int vec_wgs = (L + kVecCols - 1) / kVecCols;
  ProfScope ps("latent_accumulate_kernel", st, 2.0 * B * L * L + 8.0 * B * L, 8.0 * B * L * (1.0 + nt) + 16.0 * L * L + 56.0 * L);
  hipLaunchKernelGGL(latent_accumulate_kernel, dim3(nt * nt + vec_wgs), dim3(kLatThreads), 0, st, mu, mu_pitch, logvar, lv_pitch, B,
                     L, nt, kl_sum, mu_sum, sig2_sum, cov_sum, nonfinite, rows);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
