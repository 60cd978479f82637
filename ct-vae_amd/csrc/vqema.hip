// Exponential-moving-average codebooks of the vector-quantised models (exp_params.codebook_ema_decay; optim.py: CodebookEMA;
// van den Oord et al. 2017, appendix A.1).  The codebook is not trained by the optimizer: code k of codebook c is the running
// mean of the latent slices assigned to it.
//   vq_ema_stats_*_kernel   per slice z of the position range: the window statistics of that slice,
//                             cnt[c][k] = #{p : idx[p][c] = k},  sum[c][k][d] = sum_{p : idx[p][c] = k} lat[p][c + d]
//                           into the workspace (one record of W = C*K*Dc + C*K + C words per slice: sums, counts, invalid)
//   vq_ema_reduce_kernel    acc_s[o] = (((acc_s[o] + rec_0[o]) + rec_1[o]) + ...), acc_n and `invalid` likewise in integers
//   vq_ema_update_kernel    N <- g N + (1-g) acc_n,  M <- g M + (1-g) acc_s,  E <- M / Ntilde,  accumulators <- 0
//
// Statistics.  The sums are the ones vq.hip forms inside the codebook gradient, and the three kernels are its three, with the
// same dispatch: organised by POSITIONS with one private LDS table per half-wave (Dc <= 32, K <= 128) or per wave (Dc <= 128,
// table fits 150 KiB), or a scan per code for everything else.  One owner per table and per output element, positions walked in
// a fixed order, records added in slice order: no float atomic anywhere, the result is a function of the inputs and the shapes
// alone.  The source channel of codebook c is c + d, not c * Dc + d (the slice quirk, models/mcq_vae.py).  An index outside
// [0, K) touches no table (the LDS forms would write out of bounds otherwise) and is counted in the slice's invalid word.  A
// non-finite latent is added like any other value.  Counts are 32-bit integers inside a slice (a slice holds < 2^31 positions)
// and 64-bit in the accumulators.  Pointers and shape integers only: a captured launch replays correctly.
//
// Update.  One workgroup per codebook.  n = sum_k N_k is formed by ONE thread in float64 in index order from LDS (K <= 16384),
// Ntilde_k = (N_k + eps) / (n + K eps) * n in float64, rounded to fp32 once; N and M take two roundings each
// (fmaf(g, old, fl32((1-g) * acc)), the product formed in float64), E one division.  g and eps are by-value arguments, so
// this launch is never captured.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kEmaMaxK = 16384;            // update: N and Ntilde of one codebook in LDS (2 * K floats)

// record layout per slice: [0, n_all) float sums, [n_all, n_all + C*K) uint counts, [.., + C) uint invalid per codebook
__device__ __forceinline__ size_t ema_rec(int z, int n_all, int C, int K) { return (size_t)z * ((size_t)n_all + (size_t)C * K + C); }

// grid (S, C), block 256: half-wave h of wave w owns table [w*2+h][K][32] and counts [w*2+h][K]
__global__ __launch_bounds__(256) void vq_ema_stats_pos_kernel(const float* __restrict__ lat, const long long* __restrict__ inds,
                                                               float* __restrict__ part, int P, int D, int K, int Dc, int C,
                                                               int HW, int Ps) {
  extern __shared__ float ema_smem[];
  float* sAcc = ema_smem;                                                  // [8][K][32]
  unsigned* sCnt = reinterpret_cast<unsigned*>(sAcc + (size_t)8 * K * 32);  // [8][K] + [8] invalid
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, d = lane & 31;
  const int i = blockIdx.y;
  for (int e = tid; e < 8 * K * 32; e += 256) sAcc[e] = 0.f;
  for (int e = tid; e < 8 * K + 8; e += 256) sCnt[e] = 0u;
  __syncthreads();
  const int t = wave * 2 + half;
  float* tAcc = sAcc + (size_t)t * K * 32;
  unsigned* tCnt = sCnt + t * K;
  unsigned* tBad = sCnt + 8 * K + t;
  const int p_lo = blockIdx.x * Ps;
  const int p_hi = p_lo + Ps < P ? p_lo + Ps : P;
  constexpr int U = 4;                                 // positions in flight per half-wave
  for (int base = p_lo + t; base < p_hi; base += 8 * U) {
    long long kk[U];
    float vv[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = base + 8 * u;
      live[u] = p < p_hi;
      kk[u] = -1;
      vv[u] = 0.f;
      if (live[u]) {
        const int b = p / HW, hw = p - b * HW;
        kk[u] = inds[((size_t)b * C + i) * HW + hw];
        if (d < Dc) vv[u] = lat[(size_t)p * D + i + d];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!live[u]) continue;                          // uniform over the half-wave, like the two tests below
      if (kk[u] >= 0 && kk[u] < (long long)K) {
        const int k = (int)kk[u];
        tAcc[k * 32 + d] += vv[u];
        if (d == 0) tCnt[k] += 1u;
      } else if (d == 0) {
        *tBad += 1u;
      }
    }
  }
  __syncthreads();
  const int n_all = C * K * Dc;
  float* rec = part + ema_rec(blockIdx.x, n_all, C, K);
  unsigned* rec_u = reinterpret_cast<unsigned*>(rec);
  for (int e = tid; e < K * Dc; e += 256) {
    const int k = e / Dc, dd = e - k * Dc;
    float sx = 0.f;
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) sx += sAcc[((size_t)tt * K + k) * 32 + dd];
    rec[((size_t)i * K + k) * Dc + dd] = sx;
  }
  for (int k = tid; k <= K; k += 256) {                // k == K: the invalid word
    unsigned c = 0u;
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) c += k < K ? sCnt[tt * K + k] : sCnt[8 * K + tt];
    rec_u[k < K ? (size_t)n_all + (size_t)i * K + k : (size_t)n_all + (size_t)C * K + i] = c;
  }
}

// wide slices (32 < Dc <= 128): a wave owns a position per step (lane = d and d + 64) and table [wave][K][128]
__global__ __launch_bounds__(256) void vq_ema_stats_posw_kernel(const float* __restrict__ lat, const long long* __restrict__ inds,
                                                                float* __restrict__ part, int P, int D, int K, int Dc, int C,
                                                                int HW, int Ps) {
  extern __shared__ float ema_smem[];
  float* sAcc = ema_smem;                                                   // [4][K][128]
  unsigned* sCnt = reinterpret_cast<unsigned*>(sAcc + (size_t)4 * K * 128);  // [4][K] + [4] invalid
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.y;
  for (int e = tid; e < 4 * K * 128; e += 256) sAcc[e] = 0.f;
  for (int e = tid; e < 4 * K + 4; e += 256) sCnt[e] = 0u;
  __syncthreads();
  float* tAcc = sAcc + (size_t)wave * K * 128;
  unsigned* tCnt = sCnt + wave * K;
  unsigned* tBad = sCnt + 4 * K + wave;
  const int p_lo = blockIdx.x * Ps;
  const int p_hi = p_lo + Ps < P ? p_lo + Ps : P;
  constexpr int U = 4;                                 // positions in flight per wave
  for (int base = p_lo + wave; base < p_hi; base += 4 * U) {
    long long kk[U];
    float v0[U], v1[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = base + 4 * u;
      live[u] = p < p_hi;
      kk[u] = -1;
      v0[u] = v1[u] = 0.f;
      if (live[u]) {
        const int b = p / HW, hw = p - b * HW;
        kk[u] = inds[((size_t)b * C + i) * HW + hw];
        if (lane < Dc) v0[u] = lat[(size_t)p * D + i + lane];
        if (lane + 64 < Dc) v1[u] = lat[(size_t)p * D + i + lane + 64];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!live[u]) continue;                          // uniform over the wave, like the two tests below
      if (kk[u] >= 0 && kk[u] < (long long)K) {
        const int k = (int)kk[u];
        tAcc[k * 128 + lane] += v0[u];
        tAcc[k * 128 + 64 + lane] += v1[u];
        if (lane == 0) tCnt[k] += 1u;
      } else if (lane == 0) {
        *tBad += 1u;
      }
    }
  }
  __syncthreads();
  const int n_all = C * K * Dc;
  float* rec = part + ema_rec(blockIdx.x, n_all, C, K);
  unsigned* rec_u = reinterpret_cast<unsigned*>(rec);
  for (int e = tid; e < K * Dc; e += 256) {
    const int k = e / Dc, dd = e - k * Dc;
    float sx = 0.f;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) sx += sAcc[((size_t)tt * K + k) * 128 + dd];
    rec[((size_t)i * K + k) * Dc + dd] = sx;
  }
  for (int k = tid; k <= K; k += 256) {
    unsigned c = 0u;
#pragma unroll
    for (int tt = 0; tt < 4; ++tt) c += k < K ? sCnt[tt * K + k] : sCnt[4 * K + tt];
    rec_u[k < K ? (size_t)n_all + (size_t)i * K + k : (size_t)n_all + (size_t)C * K + i] = c;
  }
}

// everything else (Dc <= 256): workgroup (k, c, z) scans its slice for index k, a wave gathers its hits row by row; the
// workgroup of code 0 also counts the indices outside [0, K)
__global__ __launch_bounds__(256) void vq_ema_stats_scan_kernel(const float* __restrict__ lat, const long long* __restrict__ inds,
                                                                float* __restrict__ part, int P, int D, int K, int Dc, int C,
                                                                int HW, int Ps) {
  __shared__ float sAcc[4][256];
  __shared__ unsigned sCnt[4], sBad[4];
  const int k = blockIdx.x, i = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};  // d = lane + 64*u, Dc <= 256
  unsigned cnt = 0u, bad = 0u;
  const int p_lo = blockIdx.z * Ps;
  const int p_hi = p_lo + Ps < P ? p_lo + Ps : P;
  for (int base = p_lo + wave * 64; base < p_hi; base += 256) {
    const int p = base + lane;
    bool hit = false, out = false;
    if (p < p_hi) {
      const int b = p / HW, hw = p - b * HW;
      const long long idx = inds[((size_t)b * C + i) * HW + hw];
      hit = idx == (long long)k;
      out = idx < 0 || idx >= (long long)K;
    }
    unsigned long long mask = __ballot(hit);
    cnt += (unsigned)__popcll(mask);
    bad += (unsigned)__popcll(__ballot(out));
    while (mask) {
      const int l = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const float* x = lat + (size_t)(base + l) * D + i;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int d = lane + 64 * u;
        if (d < Dc) acc[u] += x[d];
      }
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) sAcc[wave][lane + 64 * u] = acc[u];
  if (lane == 0) {
    sCnt[wave] = cnt;
    sBad[wave] = bad;
  }
  __syncthreads();
  const int n_all = C * K * Dc;
  float* rec = part + ema_rec(blockIdx.z, n_all, C, K);
  unsigned* rec_u = reinterpret_cast<unsigned*>(rec);
  if (tid < Dc) rec[((size_t)i * K + k) * Dc + tid] = ((sAcc[0][tid] + sAcc[1][tid]) + sAcc[2][tid]) + sAcc[3][tid];
  if (tid == 0) {
    rec_u[(size_t)n_all + (size_t)i * K + k] = sCnt[0] + sCnt[1] + sCnt[2] + sCnt[3];
    if (k == 0) rec_u[(size_t)n_all + (size_t)C * K + i] = sBad[0] + sBad[1] + sBad[2] + sBad[3];
  }
}

// one thread per word of a record; records added in slice order, eight loads in flight (vq_cb_reduce_kernel's loop)
__global__ __launch_bounds__(256) void vq_ema_reduce_kernel(const float* __restrict__ part, float* __restrict__ acc_s,
                                                            unsigned long long* __restrict__ acc_n,
                                                            unsigned long long* __restrict__ invalid, int n_all, int CK, int C,
                                                            int S) {
  const int W = n_all + CK + C;
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= W) return;
  if (o < n_all) {
    float v = acc_s[o];
    int z = 0;
    for (; z + 8 <= S; z += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = part[(size_t)(z + u) * W + o];
#pragma unroll
      for (int u = 0; u < 8; ++u) v += t[u];
    }
    for (; z < S; ++z) v += part[(size_t)z * W + o];
    acc_s[o] = v;
    return;
  }
  const unsigned* part_u = reinterpret_cast<const unsigned*>(part);
  unsigned long long v = 0ull;
  int z = 0;
  for (; z + 8 <= S; z += 8) {
    unsigned t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = part_u[(size_t)(z + u) * W + o];
#pragma unroll
    for (int u = 0; u < 8; ++u) v += t[u];
  }
  for (; z < S; ++z) v += part_u[(size_t)z * W + o];
  if (o < n_all + CK) acc_n[o - n_all] += v;
  else if (v != 0ull) atomicAdd(invalid, v);           // C threads, one word: an integer atomic (exact in any order)
}

// grid (C), block 256, LDS 2 * K floats + one double
__global__ __launch_bounds__(256) void vq_ema_update_kernel(float* __restrict__ cb, float* __restrict__ Nbuf, float* __restrict__ Mbuf,
                                                            unsigned long long* __restrict__ acc_n, float* __restrict__ acc_s,
                                                            int K, int Dc, float g, float eps) {
  extern __shared__ double ema_upd_smem[];
  double* sTot = ema_upd_smem;                           // [1]
  float* sN = reinterpret_cast<float*>(ema_upd_smem + 1); // [K]
  float* sNt = sN + K;                                   // [K]
  const int c = blockIdx.x, tid = threadIdx.x;
  const double omg = 1.0 - (double)g;                    // exact; omg * acc is formed in float64 and rounded to fp32 ONCE
  float* N = Nbuf + (size_t)c * K;
  unsigned long long* an = acc_n + (size_t)c * K;
  for (int k = tid; k < K; k += 256) {
    const float nk = fmaf(g, N[k], (float)(omg * (double)an[k]));
    N[k] = nk;
    sN[k] = nk;
    an[k] = 0ull;
  }
  __syncthreads();
  if (tid == 0) {
    double n = 0.0;
    for (int k = 0; k < K; ++k) n += (double)sN[k];     // index order
    sTot[0] = n;
  }
  __syncthreads();
  const double n = sTot[0];
  const double den = n + (double)K * (double)eps;
  for (int k = tid; k < K; k += 256) sNt[k] = (float)(((double)sN[k] + (double)eps) / den * n);
  __syncthreads();
  const size_t base = (size_t)c * K * Dc;
  for (int e = tid; e < K * Dc; e += 256) {
    const int k = e / Dc;
    const float m = fmaf(g, Mbuf[base + e], (float)(omg * (double)acc_s[base + e]));
    Mbuf[base + e] = m;
    cb[base + e] = m / sNt[k];
    acc_s[base + e] = 0.f;
  }
}

namespace {

bool ema_shape_ok(int B, int HW, int D, int K, int C) {
  if (B < 1 || HW < 1 || D < 1 || K < 1 || C < 1 || C > 8 || D % C != 0 || D / C > 256) return false;
  if ((long)B * HW > 0x7fffffffL) return false;
  if ((long)C * K * (D / C) + (long)C * K + C > 0x7fffffffL) return false;
  return true;
}

}  // namespace

int vq_ema_supported(int K, int C, int Dc) {
  return K >= 1 && K <= kEmaMaxK && C >= 1 && C <= 8 && Dc >= 1 && Dc <= 256 && (long)C * K * Dc + (long)C * K + C <= 0x7fffffffL;
}

int launch_vq_ema_stats(const float* lat, const long* inds_, long* acc_n, float* acc_s, long* invalid, int B, int HW, int D, int K,
                        int C, float* ws, size_t ws_bytes, hipStream_t st) {
  if (!lat || !inds_ || !acc_n || !acc_s || !invalid || !ws) return kErrBadArg;
  if (!ema_shape_ok(B, HW, D, K, C)) return kErrBadArg;
  if ((reinterpret_cast<uintptr_t>(inds_) | reinterpret_cast<uintptr_t>(acc_n) | reinterpret_cast<uintptr_t>(invalid)) % 8 != 0)
    return kErrBadArg;
  if ((reinterpret_cast<uintptr_t>(lat) | reinterpret_cast<uintptr_t>(acc_s) | reinterpret_cast<uintptr_t>(ws)) % 4 != 0)
    return kErrBadArg;
  const long long* inds = reinterpret_cast<const long long*>(inds_);
  const int Dc = D / C, P = B * HW;
  const int n_all = C * K * Dc, CK = C * K;
  const size_t W = (size_t)n_all + CK + C, cap = ws_bytes / sizeof(float);
  if (cap < W) return kErrWorkspace;
  const double rd = 4.0 * (double)P * D + 8.0 * (double)P * C;
  int S;
  if (Dc <= 32 && K <= 128) {
    S = ceil_div(P, 256);                              // ~256 positions per workgroup
    if (S > 512) S = 512;
    if ((size_t)S * W > cap) S = (int)(cap / W);
    const int Ps = ceil_div(P, S);
    S = ceil_div(P, Ps);
    const size_t smem = ((size_t)8 * K * 32 + 8 * K + 8) * sizeof(float);
    static bool attr_set = false;
    if (!attr_set) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(vq_ema_stats_pos_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024);
      attr_set = true;
    }
    ProfScope ps("vq_ema_stats_pos_kernel", st, 0.0, rd + 4.0 * S * W);
    hipLaunchKernelGGL(vq_ema_stats_pos_kernel, dim3(S, C), dim3(256), smem, st, lat, inds, ws, P, D, K, Dc, C, HW, Ps);
    CTVAE_LAUNCH_CHECK();
  } else if (Dc <= 128 && (size_t)(4 * K * 128 + 4 * K) * sizeof(float) <= 150 * 1024) {
    S = ceil_div(P, 64);                               // a wave per position: ~64 positions per workgroup
    if (S > 512) S = 512;
    if ((size_t)S * W > cap) S = (int)(cap / W);
    const int Ps = ceil_div(P, S);
    S = ceil_div(P, Ps);
    const size_t smem = ((size_t)4 * K * 128 + 4 * K + 4) * sizeof(float);
    static bool attr_set_w = false;
    if (!attr_set_w) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(vq_ema_stats_posw_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                160 * 1024);
      attr_set_w = true;
    }
    ProfScope ps("vq_ema_stats_posw_kernel", st, 0.0, rd + 4.0 * S * W);
    hipLaunchKernelGGL(vq_ema_stats_posw_kernel, dim3(S, C), dim3(256), smem, st, lat, inds, ws, P, D, K, Dc, C, HW, Ps);
    CTVAE_LAUNCH_CHECK();
  } else {
    if (K > 65535) return kErrBadArg;
    S = 1024 / (K * C);                                // enough slices for ~1024 workgroups, each slice >= 512 positions
    if (S > P / 512) S = P / 512;
    if (S < 1) S = 1;
    if ((size_t)S * W > cap) S = (int)(cap / W);
    const int Ps = ceil_div(P, S);
    S = ceil_div(P, Ps);
    ProfScope ps("vq_ema_stats_scan_kernel", st, 0.0, 4.0 * (double)P * D + 8.0 * (double)P * C * (double)K / S + 4.0 * S * W);
    hipLaunchKernelGGL(vq_ema_stats_scan_kernel, dim3(K, C, S), dim3(256), 0, st, lat, inds, ws, P, D, K, Dc, C, HW, Ps);
    CTVAE_LAUNCH_CHECK();
  }
  ProfScope pr("vq_ema_reduce_kernel", st, 0.0, 4.0 * (S + 2.0) * W);
  hipLaunchKernelGGL(vq_ema_reduce_kernel, dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, ws, acc_s,
                     reinterpret_cast<unsigned long long*>(acc_n), reinterpret_cast<unsigned long long*>(invalid), n_all, CK, C, S);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_vq_ema_update(float* cb, float* N, float* M, long* acc_n, float* acc_s, int C, int K, int Dc, float decay, float eps,
                         hipStream_t st) {
  if (!cb || !N || !M || !acc_n || !acc_s) return kErrBadArg;
  if (!vq_ema_supported(K, C, Dc)) return kErrBadArg;
  if (!(decay > 0.f && decay < 1.f) || !(eps > 0.f) || !(eps < 3.0e38f)) return kErrBadArg;
  if (reinterpret_cast<uintptr_t>(acc_n) % 8 != 0) return kErrBadArg;
  if ((reinterpret_cast<uintptr_t>(cb) | reinterpret_cast<uintptr_t>(N) | reinterpret_cast<uintptr_t>(M) |
       reinterpret_cast<uintptr_t>(acc_s)) % 4 != 0)
    return kErrBadArg;
  const size_t smem = sizeof(double) + (size_t)2 * K * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(vq_ema_update_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    attr_set = true;
  }
  ProfScope ps("vq_ema_update_kernel", st, 0.0, 20.0 * (double)C * K * Dc + 16.0 * (double)C * K);
  hipLaunchKernelGGL(vq_ema_update_kernel, dim3(C), dim3(256), smem, st, cb, N, M, reinterpret_cast<unsigned long long*>(acc_n),
                     acc_s, K, Dc, decay, eps);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
