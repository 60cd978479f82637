// Test log-likelihood by importance sampling (loglik.py: ImportanceLogLik; Burda et al. 2016, section 5).  For z_k ~ q(z|x),
// k = 1..K, log p^(x) = logsumexp_k [ log p(x|z_k) + log p(z_k) - log q(z_k|x) ] - log K under p(x|z) = N(decode(z), sigma^2 I).
// An image's K samples arrive in chunks of S; one chunk is R = B * S decoder rows, row r belongs to image r / S.
//   loglik_latent_kernel   z = mu + expf(0.5f * log_var) * eps in fp32, and a[r] = log p(z) - log q(z|x) =
//                          -0.5 * sum_d (z^2 - eps^2 - log_var) in double from the fp32 z that was stored (the log 2 pi terms cancel)
//   loglik_rows_kernel     sse[r] = sum_i ((double)xhat[r][i] - (double)x[r / S][i])^2 over the P elements of a row, then
//                          lw[r] = -sse * c[0] - c[1] + a[r] with c = (1 / (2 sigma^2), (P / 2) log(2 pi sigma^2)) from device memory
//   loglik_merge_kernel    per image the state (m, s, s2, t, n) = (running maximum, sum exp(lw - m), sum exp(2 (lw - m)), sum lw,
//                          count) takes the chunk's S log-weights one at a time, in sample order
// The finish (loglik = m + log s - log n, elbo = t / n, ess = s^2 / s2) is the host's, in float64 from one copy of the state.
//
// Ownership.  No atomics anywhere.  rows: one workgroup per decoder row; thread t adds the elements t, t + 256, ... (vectors of
// four where the rows are 16-byte aligned) in ascending order into four accumulators that meet in a fixed order, the 64 lanes
// of a wave meet in a fixed shuffle tree, the four waves in wave order: a row's bits depend on P and the load width alone, not
// on R, S or the other rows.  latent: one wave per row, the same shuffle tree.  merge: ONE thread owns an image and walks its
// samples sequentially -- a tree over the chunk would make the state depend on where the chunks were cut; walked one by one the
// state after K samples is the same bits for every cut.  Its arithmetic is not contracted (every operation rounds on its own),
// so the host can restate it operation by operation.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

#include <cstdint>

namespace ctvae {

constexpr int kLlThreads = 256;          // rows and latent: four waves
constexpr int kLlMergeThreads = 64;      // merge: one image per thread
constexpr int kLlState = 5;              // m, s, s2, t, n

__device__ __forceinline__ double ll_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;                              // valid in lane 0
}

// ---- latent ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kLlThreads) void loglik_latent_kernel(const float* __restrict__ mu, const float* __restrict__ lv,
                                                                   const float* __restrict__ eps, int R, int S, int L,
                                                                   float* __restrict__ z, double* __restrict__ a) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (kLlThreads / 64) + (threadIdx.x >> 6);
  if (r >= R) return;                    // (whole waves leave: no barrier follows)
  const long img = (long)(r / S) * L, row = (long)r * L;
  double acc = 0.0;
  for (int d = lane; d < L; d += 64) {
    const float m = mu[img + d], v = lv[img + d], e = eps[row + d];
    const float zz = m + expf(0.5f * v) * e;
    z[row + d] = zz;
    const double zd = (double)zz, ed = (double)e;
    acc += zd * zd - ed * ed - (double)v;
  }
  acc = ll_wave_sum(acc);
  if (lane == 0) a[r] = -0.5 * acc;
}

// ---- rows ------------------------------------------------------------------------------------------------------------------
template <bool kVec>
__global__ __launch_bounds__(kLlThreads) void loglik_rows_kernel(const float* __restrict__ xhat, const float* __restrict__ x, int S,
                                                                 long P, const double* __restrict__ a,
                                                                 const double* __restrict__ consts, double* __restrict__ lw) {
  __shared__ double red[kLlThreads / 64];
  const int tid = threadIdx.x;
  const long r = blockIdx.x;
  const float* ph = xhat + r * P;
  const float* px = x + (r / S) * P;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (kVec) {
    const float4* vh = reinterpret_cast<const float4*>(ph);
    const float4* vx = reinterpret_cast<const float4*>(px);
    const long n4 = P >> 2;
    long i = tid;
    for (; i + 3 * kLlThreads < n4; i += 4 * kLlThreads) {   // four 16-byte loads of each row in flight
      float4 h[4], g[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        h[u] = vh[i + u * kLlThreads];
        g[u] = vx[i + u * kLlThreads];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double d0 = (double)h[u].x - (double)g[u].x, d1 = (double)h[u].y - (double)g[u].y;
        const double d2 = (double)h[u].z - (double)g[u].z, d3 = (double)h[u].w - (double)g[u].w;
        s0 = fma(d0, d0, s0);
        s1 = fma(d1, d1, s1);
        s2 = fma(d2, d2, s2);
        s3 = fma(d3, d3, s3);
      }
    }
    for (; i < n4; i += kLlThreads) {
      const float4 h = vh[i], g = vx[i];
      const double d0 = (double)h.x - (double)g.x, d1 = (double)h.y - (double)g.y;
      const double d2 = (double)h.z - (double)g.z, d3 = (double)h.w - (double)g.w;
      s0 = fma(d0, d0, s0);
      s1 = fma(d1, d1, s1);
      s2 = fma(d2, d2, s2);
      s3 = fma(d3, d3, s3);
    }
  } else {
    for (long i = tid; i < P; i += kLlThreads) {
      const double d = (double)ph[i] - (double)px[i];
      s0 = fma(d, d, s0);
    }
  }
  const double w = ll_wave_sum((s0 + s1) + (s2 + s3));
  if ((tid & 63) == 0) red[tid >> 6] = w;
  __syncthreads();
  if (tid == 0) {
    const double sse = (red[0] + red[1]) + (red[2] + red[3]);
    lw[r] = -sse * consts[0] - consts[1] + (a ? a[r] : 0.0);
  }
}

// ---- merge -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ll_finite(double v) {
  return (__builtin_bit_cast(unsigned long long, v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

__global__ __launch_bounds__(kLlMergeThreads) void loglik_merge_kernel(const double* __restrict__ lw, int B, int S,
                                                                       double* __restrict__ state, int* __restrict__ flag, int row0) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * kLlMergeThreads + threadIdx.x;
  if (b >= B) return;
  double* st = state + (long)(row0 + b) * kLlState;
  double m = st[0], s = st[1], s2 = st[2], t = st[3], n = st[4];
  int bad = flag[row0 + b];
  const double* w = lw + (long)b * S;
  for (int k = 0; k < S; ++k) {
    const double v = w[k];
    if (!ll_finite(v)) {
      bad = 1;
      continue;
    }
    if (v > m) {                         // the maximum moves: what was summed is rescaled (m = -inf at first: exp gives 0)
      const double c = exp(m - v);
      s = s * c + 1.0;
      s2 = s2 * (c * c) + 1.0;
      m = v;
    } else {
      const double e = exp(v - m);
      s = s + e;
      s2 = s2 + e * e;
    }
    t = t + v;
    n = n + 1.0;
  }
  st[0] = m;
  st[1] = s;
  st[2] = s2;
  st[3] = t;
  st[4] = n;
  flag[row0 + b] = bad;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
int launch_loglik_latent(const float* mu, const float* lv, const float* eps, int B, int S, int L, float* z, double* a,
                         hipStream_t st) {
  if (!mu || !lv || !eps || !z || !a) return kErrBadArg;
  if (B < 0 || S < 1 || L < 1 || (long)B * S > 0x7fffffffL) return kErrBadArg;
  if (B == 0) return 0;
  const int R = B * S;
  const int per = kLlThreads / 64;
  ProfScope ps("loglik_latent_kernel", st, 8.0 * R * L, 8.0 * R * L + 8.0 * B * L + 8.0 * R);
  hipLaunchKernelGGL(loglik_latent_kernel, dim3((R + per - 1) / per), dim3(kLlThreads), 0, st, mu, lv, eps, R, S, L, z, a);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_loglik_rows(const float* xhat, const float* x, int B, int S, long P, const double* a, const double* consts, double* lw,
                       hipStream_t st) {
  if (!xhat || !x || !consts || !lw) return kErrBadArg;
  if (B < 0 || S < 1 || P < 1 || (long)B * S > 0x7fffffffL) return kErrBadArg;
  if (B == 0) return 0;
  const int R = B * S;
  const bool vec = (P & 3) == 0 && (((uintptr_t)xhat | (uintptr_t)x) & 15) == 0;
  ProfScope ps("loglik_rows_kernel", st, 3.0 * R * P, 4.0 * R * P + 4.0 * B * P + 16.0 * R);
  if (vec)
    hipLaunchKernelGGL(loglik_rows_kernel<true>, dim3(R), dim3(kLlThreads), 0, st, xhat, x, S, P, a, consts, lw);
  else
    hipLaunchKernelGGL(loglik_rows_kernel<false>, dim3(R), dim3(kLlThreads), 0, st, xhat, x, S, P, a, consts, lw);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_loglik_merge(const double* lw, int B, int S, double* state, int* flag, int row0, int capacity, hipStream_t st) {
  if (!lw || !state || !flag) return kErrBadArg;
  if (B < 0 || S < 1 || row0 < 0 || capacity < 0 || (long)row0 + B > (long)capacity) return kErrBadArg;
  if (B == 0) return 0;
  ProfScope ps("loglik_merge_kernel", st, 8.0 * B * S, 8.0 * B * S + 88.0 * B);
  hipLaunchKernelGGL(loglik_merge_kernel, dim3((B + kLlMergeThreads - 1) / kLlMergeThreads), dim3(kLlMergeThreads), 0, st, lw, B, S,
                     state, flag, row0);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
