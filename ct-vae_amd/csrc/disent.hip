// Dense arithmetic of the disentanglement metrics (metrics.py) over a code matrix z [N][L] (contiguous row-major f32, the
// flattened encoder output of N items): MIG (Chen et al. 2018) needs a 20-bin discretisation of every latent column and the
// latent x factor mutual-information matrix; the FactorVAE score (Kim & Mnih 2018) needs per-group column variances over a
// global variance and an arg-min.  L is the width of a feature map (8192 for CT-MCQ-VAE), N a few hundred rows: three small
// bandwidth-bound kernels, lanes along L (coalesced rows), no global atomics.
//   column_moments_kernel      z -> mean, unbiased variance, min, max per column     (Welford mean, merged pairwise; second pass for the variance)
//   mi_matrix_kernel           z, lo, hi, factors -> mi [L][F] (+ bins [N][L])       (bins live in LDS; counts are integers)
//   group_var_argmin_kernel    z [G][B][L] -> per group arg-min of var / global_var  ((value, index) through wave shuffles)
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kDisMaxL = 16384, kDisMaxN = 65535, kDisMaxF = 16, kDisMaxSize = 256, kDisBins = 20;

// Welford state of a set of values and the merge of two of them (Chan et al.): n elements, their mean, M2 = sum (x - mean)^2
struct Moments {
  float n, mean, m2;
};
__device__ __forceinline__ void moments_push(Moments& a, float x) {
  a.n += 1.f;
  const float d = x - a.mean;
  a.mean += __fdiv_rn(d, a.n);
  a.m2 += d * (x - a.mean);
}
__device__ __forceinline__ Moments moments_merge(const Moments& a, const Moments& b) {
  if (b.n == 0.f) return a;
  if (a.n == 0.f) return b;
  Moments r;
  r.n = a.n + b.n;
  const float d = b.mean - a.mean, fb = __fdiv_rn(b.n, r.n);
  r.mean = a.mean + d * fb;
  r.m2 = a.m2 + b.m2 + d * d * a.n * fb;
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// column moments: block = 64 columns x 4 row slices (row r goes to slice r % 4); each wave reads 256 contiguous bytes of a row.
// Sums of squares of up to 16384 values per slice accumulate serially in f32; the variance's error stays ~ sqrt(N) * 2^-24.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void column_moments_kernel(const float* __restrict__ z, int N, int L, float* __restrict__ mean,
                                                             float* __restrict__ var, float* __restrict__ mn, float* __restrict__ mx) {
  __shared__ Moments sm[4][64];
  __shared__ float smin[4][64], smax[4][64], smean[64];
  const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + lane;
  Moments a{0.f, 0.f, 0.f};
  float lo = INFINITY, hi = -INFINITY;
  if (col < L) {
    for (int r = slice; r < N; r += 4) {
      const float x = z[(size_t)r * L + col];
      moments_push(a, x);
      lo = fminf(lo, x);
      hi = fmaxf(hi, x);
    }
  }
  sm[slice][lane] = a;
  smin[slice][lane] = lo;
  smax[slice][lane] = hi;
  __syncthreads();
  if (slice == 0) {
    // ((0 + 1) + (2 + 3)): a balanced tree over the four slices
    const Moments b = moments_merge(moments_merge(sm[0][lane], sm[1][lane]), moments_merge(sm[2][lane], sm[3][lane]));
    smean[lane] = b.mean;
    if (col < L) {
      mean[col] = b.mean;
      mn[col] = fminf(fminf(smin[0][lane], smin[1][lane]), fminf(smin[2][lane], smin[3][lane]));
      mx[col] = fmaxf(fmaxf(smax[0][lane], smax[1][lane]), fmaxf(smax[2][lane], smax[3][lane]));
    }
  }
  __syncthreads();
  // second pass (the tile is in cache): sum (x - mean)^2 around the FINAL mean, whose rounding error enters squared -- the
  // single-pass M2 carries it linearly, |mean| / std times 2^-24
  const float m = smean[lane];
  float q = 0.f;
  if (col < L)
    for (int r = slice; r < N; r += 4) {
      const float d = z[(size_t)r * L + col] - m;
      q += d * d;
    }
  __syncthreads();
  smin[slice][lane] = q;
  __syncthreads();
  if (slice == 0 && col < L) var[col] = __fdiv_rn((smin[0][lane] + smin[1][lane]) + (smin[2][lane] + smin[3][lane]), (float)(N - 1));
}

int launch_column_moments(const float* z, int N, int L, float* mean, float* var, float* mn, float* mx, hipStream_t st) {
  if (N < 2 || N > kDisMaxN || L < 1 || L > kDisMaxL) return kErrBadArg;
  ProfScope ps("column_moments_kernel", st, 6.0 * N * L, 4.0 * ((double)N * L + 4.0 * L));
  hipLaunchKernelGGL(column_moments_kernel, dim3(ceil_div(L, 64)), dim3(256), 0, st, z, N, L, mean, var, mn, mx);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// mutual information of every (latent column, factor) pair
// ---------------------------------------------------------------------------------------------------------------------
// np.digitize(x, np.histogram(x, 20)[1][:-1]): the number of k in 0..19 with edge_k <= x, edge_k = lo + k * ((hi - lo) / 20),
// each operation rounded to f32 on its own (no fused multiply-add); a constant column takes [lo - 0.5, hi + 0.5]
__device__ __forceinline__ int bin_of(float x, float lo, float hi) {
  if (hi == lo) {
    lo = __fsub_rn(lo, 0.5f);
    hi = __fadd_rn(hi, 0.5f);
  }
  const float w = __fdiv_rn(__fsub_rn(hi, lo), (float)kDisBins);
  int b = 0;
#pragma unroll
  for (int k = 0; k < kDisBins; ++k) b += (__fadd_rn(lo, __fmul_rn((float)k, w)) <= x) ? 1 : 0;
  return b;
}

constexpr size_t kMiMaxSmem = 150 * 1024;      // of the CU's 160 KiB; the worst case below needs ~121 KiB
struct MiSizes {
  int s[kDisMaxF];
};

// One workgroup owns CB consecutive columns (CB a power of two <= 32: a row's CB floats are one contiguous run) and all N rows:
// it bins its z tile ONCE into LDS bytes, then each wave takes columns w, w + nw, ... and walks the factors: joint counts
// (bin, value) by LDS atomics in the wave's own table, MI = sum over the non-zero cells of c/N * log(c*N / (c_bin * c_value)).
// The value counts of every factor are formed once per workgroup.  Dynamic LDS (launch_mi_matrix sizes it):
//   cs [F][smax] u32 | cb [nw][20] u32 | table [nw][20*smax] u32 | bins [N][CB] u8
// Every wave runs the same number of column rounds, so the barriers are uniform; a round past the last column only waits.
__global__ __launch_bounds__(256) void mi_matrix_kernel(const float* __restrict__ z, const float* __restrict__ lo,
                                                        const float* __restrict__ hi, const int32_t* __restrict__ factors,
                                                        MiSizes sizes, int N, int L, int F, int CB, int smax,
                                                        float* __restrict__ mi, uint8_t* __restrict__ bins_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned mi_smem[];
  const int nt = blockDim.x, nw = nt >> 6, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned* cs = mi_smem;
  unsigned* cb = cs + F * smax;
  unsigned* table = cb + nw * kDisBins + w * kDisBins * smax;
  uint8_t* bins = reinterpret_cast<uint8_t*>(cb + nw * kDisBins + nw * kDisBins * smax);
  unsigned* mycb = cb + w * kDisBins;
  const int c0 = blockIdx.x * CB, lgCB = __ffs(CB) - 1;
  __shared__ int ssz[kDisMaxF];      // a lane-indexed read of the argument struct would go through scratch
  if (threadIdx.x < kDisMaxF) ssz[threadIdx.x] = sizes.s[threadIdx.x];

  for (int i = threadIdx.x; i < F * smax; i += nt) cs[i] = 0u;
  // bin the tile: thread -> (row, column) with the column fastest
  for (int i = threadIdx.x; i < N * CB; i += nt) {
    const int r = i >> lgCB, c = c0 + (i & (CB - 1));
    int b = 0;
    if (c < L) {
      b = bin_of(z[(size_t)r * L + c], lo[c], hi[c]);
      if (bins_out) bins_out[(size_t)r * L + c] = (uint8_t)b;
    }
    bins[i] = (uint8_t)b;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < N * F; i += nt) {
    const int f = i % F;
    const unsigned v = (unsigned)factors[i];
    if (v < (unsigned)ssz[f]) atomicAdd(&cs[f * smax + v], 1u);
  }
  __syncthreads();

  const float fN = (float)N, invN = __fdiv_rn(1.f, (float)N);
  for (int c1 = 0; c1 < CB; c1 += nw) {
    const int cc = c1 + w, c = c0 + cc;
    const bool live = cc < CB && c < L;
    if (lane < kDisBins) mycb[lane] = 0u;
    __syncthreads();
    if (live)
      for (int r = lane; r < N; r += 64) {
        const int b = bins[r * CB + cc];
        if (b >= 1) atomicAdd(&mycb[b - 1], 1u);
      }
    for (int f = 0; f < F; ++f) {
      const int S = ssz[f], cells = kDisBins * S;
      for (int i = lane; i < cells; i += 64) table[i] = 0u;
      __syncthreads();
      if (live)
        for (int r = lane; r < N; r += 64) {
          const int b = bins[r * CB + cc];
          const unsigned v = (unsigned)factors[(size_t)r * F + f];
          if (b >= 1 && v < (unsigned)S) atomicAdd(&table[(b - 1) * S + (int)v], 1u);
        }
      __syncthreads();
      float acc = 0.f;
      if (live)
        for (int i = lane; i < cells; i += 64) {
          const unsigned cnt = table[i];
          if (cnt) {
            const int b = i / S, v = i - b * S;
            const float pm = (float)mycb[b] * (float)cs[f * smax + v];
            acc += (float)cnt * invN * logf(__fdiv_rn((float)cnt * fN, pm));
          }
        }
      acc = wave_sum(acc);
      if (live && lane == 0) mi[(size_t)c * F + f] = acc;
      __syncthreads();       // the table is free for the next factor
    }
  }
}

int launch_mi_matrix(const float* z, const float* lo, const float* hi, const int32_t* factors, const int32_t* sizes, int N, int L,
                     int F, float* mi, uint8_t* bins, hipStream_t st) {
  if (N < 2 || N > kDisMaxN || L < 1 || L > kDisMaxL || F < 1 || F > kDisMaxF) return kErrBadArg;
  MiSizes sz{};
  int smax = 2;
  for (int f = 0; f < F; ++f) {
    if (sizes[f] < 2 || sizes[f] > kDisMaxSize) return kErrBadArg;
    sz.s[f] = sizes[f];
    smax = sizes[f] > smax ? sizes[f] : smax;
  }
  // tables: 80 * smax bytes each -- four waves up to 128 values per factor, two above (40 KiB of tables at most);
  // bins: the widest power-of-two column block whose N x CB bytes stay within 64 KiB (CB = 1 at N = 65535)
  const int nw = smax <= 128 ? 4 : 2;
  int CB = 32;
  while (CB > 1 && (size_t)N * CB > 65536) CB >>= 1;
  const size_t words = (size_t)F * smax + (size_t)nw * kDisBins + (size_t)nw * kDisBins * smax;
  const size_t smem = words * 4 + (((size_t)N * CB + 15) & ~(size_t)15);
  if (smem > kMiMaxSmem) return kErrBadArg;
  static bool raised = false;
  if (!raised) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mi_matrix_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMiMaxSmem);
    raised = true;
  }
  ProfScope ps("mi_matrix_kernel", st, 40.0 * N * L + 2.0 * N * L * F,
               4.0 * N * L + 8.0 * L + 4.0 * N * F + 4.0 * L * F + (bins ? (double)N * L : 0.0));
  hipLaunchKernelGGL(mi_matrix_kernel, dim3(ceil_div(L, CB)), dim3(64 * nw), smem, st, z, lo, hi, factors, sz, N, L, F, CB, smax,
                     mi, bins);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// FactorVAE score: per group g the active column with the smallest var_B(z[g][:, l]) / global_var[l]
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ratio_less(float v, int i, float bv, int bi) { return v < bv || (v == bv && i < bi); }

// One workgroup per group; thread t takes columns t, t + 256, ... (a wave reads 256 contiguous bytes of each of the B rows).
// No active column: arg = -1, val = +inf.
__global__ __launch_bounds__(256) void group_var_argmin_kernel(const float* __restrict__ z, const float* __restrict__ gvar,
                                                               const uint8_t* __restrict__ active, int B, int L,
                                                               int32_t* __restrict__ arg, float* __restrict__ val) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const float* zg = z + (size_t)blockIdx.x * B * L;
  float bv = INFINITY;
  int bi = 0x7fffffff;
  for (int l = threadIdx.x; l < L; l += 256) {
    if (!active[l]) continue;
    Moments a{0.f, 0.f, 0.f};
    for (int r = 0; r < B; ++r) moments_push(a, zg[(size_t)r * L + l]);
    float q = 0.f;                                   // around the final mean, as column_moments_kernel (the rows are in L1)
    for (int r = 0; r < B; ++r) {
      const float d = zg[(size_t)r * L + l] - a.mean;
      q += d * d;
    }
    const float v = __fdiv_rn(__fdiv_rn(q, (float)(B - 1)), gvar[l]);
    if (ratio_less(v, l, bv, bi)) { bv = v; bi = l; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ratio_less(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = bv; si[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k)
      if (ratio_less(sv[k], si[k], bv, bi)) { bv = sv[k]; bi = si[k]; }
    arg[blockIdx.x] = bi == 0x7fffffff ? -1 : bi;
    val[blockIdx.x] = bv;
  }
}

int launch_group_var_argmin(const float* z, const float* gvar, const uint8_t* active, int G, int B, int L, int32_t* arg, float* val,
                            hipStream_t st) {
  if (G < 1 || G > kDisMaxN || B < 2 || B > kDisMaxN || L < 1 || L > kDisMaxL) return kErrBadArg;
  ProfScope ps("group_var_argmin_kernel", st, 6.0 * G * B * L, 4.0 * G * B * L + 5.0 * L + 8.0 * G);
  hipLaunchKernelGGL(group_var_argmin_kernel, dim3(G), dim3(256), 0, st, z, gvar, active, B, L, arg, val);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
