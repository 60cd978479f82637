// A Gaussian-mixture latent prior fitted by EM (latentprior.py: GaussianMixturePrior; include/ctvae_hip.h: ctvae_gmm_*):
//   gmm_estep_full_kernel   64 rows of X per workgroup, every component in turn: Y = (X - mu_k) P_k^T as 64 x 64 f32 MFMA tiles
//                           (v_mfma_f32_32x32x2_f32, 4 waves = 2 x 2 blocks of 32 x 32, 32-deep chunks through LDS as glinear.hip
//                           does), the tile's squares summed per row; then the log-sum-exp over the components and r, ll
//   gmm_estep_diag_kernel   the same with P_k a vector: a wave owns the components k = w, w + 4, ..., a lane one row
//   gmm_mstep_vec_kernel    Nk, S1 and the diagonal of S2 of one (component, slab): a thread owns a column, float64 throughout
//   gmm_mstep_full_kernel   one 64 x 64 tile (i-tile >= j-tile) of S2 of one (component, slab): fp32 MFMA over 256 rows at a time,
//                           float64 across those blocks
//   gmm_mstep_merge_kernel  the slabs summed in ascending order, one owner per output element; the lower triangle mirrored
//   gmm_sample_kernel       one workgroup per drawn row: the component from the cdf, z = mu_k + L_k eps
//
// Determinism.  Every accumulator element has one owner thread, which adds its rows in a fixed order; slabs are merged in
// ascending order; there is no atomic anywhere.  An MFMA is a k-ordered fmaf chain, so the tiles have a fixed order too.
//
// P_k is lower triangular: a tile of Y needs the chunks j < i0 + 64 only, which is 3/4 of the square at D = 128.  LDS per
// workgroup of the E step: two [64][36] operand tiles, the [64][65] row-norm partials and the [64][65] log-probabilities, 51 KB:
// three workgroups per CU.  P_k itself (64 KB at D = 128) is not kept in LDS whole: every workgroup walks all of it once per
// component, 640 KB for K = 10, which stays in L2.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

namespace {

constexpr int kGmmThreads = 256;
constexpr int kGmmMaxD = 256;
constexpr int kGmmMaxK = 64;
constexpr int kERows = 64;              // rows of X per workgroup of the E step
constexpr int kLP = 36;                 // LDS row stride of a [64][32] operand tile (glinear.hip)
constexpr int kLQ = 68;                 // LDS row stride of a [32][64] operand tile
constexpr int kMBlockChunks = 8;        // M step: 32-row chunks per fp32 block (256 rows), then one float64 add
constexpr int kMSlabRows = 256;         // M step: rows per slab at least (one fp32 block)
constexpr size_t kMWsCap = 256u << 20;  // M step: the slabs' scratch stays below this
constexpr float kHalfLog2Pi = 0.91893853320467274178f;

__device__ __forceinline__ bool gmm_nonfinite(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) == 0x7f800000u; }

// ---- the E step's tail: lps[row][k] -> ll, r.  bad rows: r = 0, ll = 0, flag 1.  r is e_k / sum_k e_k with e_k = exp(lp_k - max):
// the same number as exp(lp_k - ll), but a row of r then sums to 1 within the roundings of K divisions and one K-term sum, where
// going through the rounded ll would add |ll| * eps.
__device__ __forceinline__ void estep_finish(float (*lps)[kGmmMaxK + 1], const int* bad, float* ms, float* ss, long n0, int nr, int K,
                                             float* __restrict__ r, float* __restrict__ ll, int* __restrict__ nonfinite) {
  const int tid = threadIdx.x;
  if (tid < nr) {
    float m = lps[tid][0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, lps[tid][k]);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += expf(lps[tid][k] - m);
    const int b = bad[tid];
    ms[tid] = m;
    ss[tid] = s;
    ll[n0 + tid] = b ? 0.f : m + logf(s);
    nonfinite[n0 + tid] = b;
  }
  __syncthreads();
  for (int e = tid; e < nr * K; e += kGmmThreads) {
    const int row = e / K, k = e - row * K;
    r[n0 * K + e] = bad[row] ? 0.f : expf(lps[row][k] - ms[row]) / ss[row];
  }
}

__device__ __forceinline__ void estep_flags(const float* __restrict__ X, long n0, int nr, int D, int* bad) {
  const int tid = threadIdx.x;
  if (tid < kERows) bad[tid] = 0;
  __syncthreads();
  const float* x = X + n0 * D;
  for (int e = tid; e < nr * D; e += kGmmThreads)
    if (gmm_nonfinite(x[e])) bad[e / D] = 1;             // (every writer stores the same word)
  __syncthreads();
}

__global__ __launch_bounds__(kGmmThreads) void gmm_estep_full_kernel(
    const float* __restrict__ X, int N, int D, int K, const float* __restrict__ log_w, const float* __restrict__ mu,
    const float* __restrict__ P, const float* __restrict__ ldh, float* __restrict__ r, float* __restrict__ ll,
    int* __restrict__ nonfinite) {
  __shared__ __attribute__((aligned(16))) float As[kERows * kLP];      // (x - mu_k)[row][j chunk]
  __shared__ __attribute__((aligned(16))) float Bs[64 * kLP];          // P_k[i tile][j chunk]
  __shared__ float sq[kERows][65];                                     // |y|^2 partials: [row][wn * 32 + li]
  __shared__ float lps[kERows][kGmmMaxK + 1];
  __shared__ float ms[kERows], ss[kERows];
  __shared__ int bad[kERows];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, li = lane & 31, lh = lane >> 5;
  const long n0 = (long)blockIdx.x * kERows;
  const int nr = N - n0 < kERows ? (int)(N - n0) : kERows;
  estep_flags(X, n0, nr, D, bad);
  const int lrow = tid >> 2, lk = (tid & 3) * 8;                       // staging: 64 rows x 32 columns, 8 per thread
  const bool xok = lrow < nr;
  const float* xrow = X + (n0 + (xok ? lrow : 0)) * D;
  const float base = -(float)D * kHalfLog2Pi;
  for (int k = 0; k < K; ++k) {
    const float* muk = mu + (long)k * D;
    const float* Pk = P + (long)k * D * D;
    float rs[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) rs[i] = 0.f;
    for (int i0 = 0; i0 < D; i0 += 64) {
      const int irow = i0 + lrow;
      const bool pok = irow < D;
      const float* prow = Pk + (long)(pok ? irow : 0) * D;
      const int jend = i0 + 64 < D ? i0 + 64 : D;                      // P_k[i][j] = 0 for j > i
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      float av[8], bv[8];
      auto fetch = [&](int j0) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int j = j0 + lk + u;
          const bool in = j < D;
          av[u] = (xok && in) ? xrow[j] - muk[j] : 0.f;
          bv[u] = (pok && in && j <= irow) ? prow[j] : 0.f;
        }
      };
      fetch(0);
      for (int j0 = 0; j0 < jend; j0 += 32) {
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          As[lrow * kLP + lk + u] = av[u];
          Bs[lrow * kLP + lk + u] = bv[u];
        }
        __syncthreads();
        if (j0 + 32 < jend) fetch(j0 + 32);
#pragma unroll
        for (int kg = 0; kg < 4; ++kg) {
          const f32x4 af = *reinterpret_cast<const f32x4*>(&As[(wm * 32 + li) * kLP + kg * 8 + 4 * lh]);
          const f32x4 bf = *reinterpret_cast<const f32x4*>(&Bs[(wn * 32 + li) * kLP + kg * 8 + 4 * lh]);
#pragma unroll
          for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[j], bf[j], acc, 0, 0, 0);
        }
      }
      // acc[i]: row wm*32 + 8*(i>>2) + 4*lh + (i&3) of the tile, output column i0 + wn*32 + li
#pragma unroll
      for (int i = 0; i < 16; ++i) rs[i] += acc[i] * acc[i];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) sq[wm * 32 + 8 * (i >> 2) + 4 * lh + (i & 3)][wn * 32 + li] = rs[i];
    __syncthreads();
    if (tid < kERows) {
      float s = 0.f;
      for (int c = 0; c < 64; ++c) s += sq[tid][c];
      lps[tid][k] = ((log_w[k] - 0.5f * s) - ldh[k]) + base;
    }
    __syncthreads();                                                   // sq is rewritten by the next component
  }
  estep_finish(lps, bad, ms, ss, n0, nr, K, r, ll, nonfinite);
}

__global__ __launch_bounds__(kGmmThreads) void gmm_estep_diag_kernel(
    const float* __restrict__ X, int N, int D, int K, const float* __restrict__ log_w, const float* __restrict__ mu,
    const float* __restrict__ P, const float* __restrict__ ldh, float* __restrict__ r, float* __restrict__ ll,
    int* __restrict__ nonfinite) {
  __shared__ float xs[kERows][33];
  __shared__ float lps[kERows][kGmmMaxK + 1];
  __shared__ float ms[kERows], ss[kERows];
  __shared__ int bad[kERows];
  const int tid = threadIdx.x, row = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long n0 = (long)blockIdx.x * kERows;
  const int nr = N - n0 < kERows ? (int)(N - n0) : kERows;
  estep_flags(X, n0, nr, D, bad);
  constexpr int kPer = kGmmMaxK / 4;                                   // components per wave: k = w + 4 * u
  float acc[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) acc[u] = 0.f;
  const int lrow = tid >> 2, lk = (tid & 3) * 8;
  for (int j0 = 0; j0 < D; j0 += 32) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int j = j0 + lk + u;
      xs[lrow][lk + u] = (lrow < nr && j < D) ? X[(n0 + lrow) * D + j] : 0.f;
    }
    __syncthreads();
    const int jn = D - j0 < 32 ? D - j0 : 32;
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int k = w + 4 * u;                                         // wave-uniform: mu and P come through scalar loads
      if (k < K) {
        const float* muk = mu + (long)k * D + j0;
        const float* pk = P + (long)k * D + j0;
        float s = acc[u];
        for (int j = 0; j < jn; ++j) {
          const float y = (xs[row][j] - muk[j]) * pk[j];
          s = fmaf(y, y, s);
        }
        acc[u] = s;
      }
    }
  }
  const float base = -(float)D * kHalfLog2Pi;
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int k = w + 4 * u;
    if (k < K) lps[row][k] = ((log_w[k] - 0.5f * acc[u]) - ldh[k]) + base;
  }
  __syncthreads();
  estep_finish(lps, bad, ms, ss, n0, nr, K, r, ll, nonfinite);
}

// ---- M step.  Slab s covers the rows [s * per, min(N, (s + 1) * per)).  Scratch: vec [S][K][1 + 2 D] doubles (Nk, S1, diag S2),
// then for full mat [S][K][D][D] doubles, of which the tiles' entries are written.
__global__ __launch_bounds__(kGmmThreads) void gmm_mstep_vec_kernel(
    const float* __restrict__ X, const float* __restrict__ r, const int* __restrict__ nonfinite, int N, int D, int K, int per,
    const float* __restrict__ m, double* __restrict__ vec) {
  const int k = blockIdx.x, s = blockIdx.y, d = threadIdx.x;
  const long lo = (long)s * per, hi = lo + per < N ? lo + per : N;
  const bool live = d < D;
  const double md = live ? (double)m[(long)k * D + d] : 0.0;
  double nk = 0.0, s1 = 0.0, s2 = 0.0;
  constexpr int kU = 16;                                               // rows whose loads are in flight together
  const long dd = live ? d : 0;
  for (long n = lo; n < hi; n += kU) {
    float rv[kU], xv[kU];
    int bf[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {                                     // every load is in bounds and none waits for another:
      const long nn = n + u < hi ? n + u : hi - 1;                     // a row past the slab re-reads the slab's last row
      bf[u] = nonfinite ? nonfinite[nn] : 0;
      rv[u] = r[nn * K + k];
      xv[u] = X[nn * D + dd];
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const bool in = n + u < hi && bf[u] == 0;                        // (block-uniform)
      rv[u] = in ? rv[u] : 0.f;
      xv[u] = (in && live) ? xv[u] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {                                     // ascending rows; a row left out adds +0.0
      const double xc = (double)xv[u] - md;
      const double t = (double)rv[u] * xc;
      nk += (double)rv[u];
      s1 += t;
      s2 += t * xc;
    }
  }
  double* out = vec + ((long)s * K + k) * (1 + 2 * D);
  if (d == 0) out[0] = nk;
  if (live) {
    out[1 + d] = s1;
    out[1 + D + d] = s2;
  }
}

__global__ __launch_bounds__(kGmmThreads) void gmm_mstep_full_kernel(
    const float* __restrict__ X, const float* __restrict__ r, const int* __restrict__ nonfinite, int N, int D, int K, int per,
    const float* __restrict__ m, double* __restrict__ mat) {
  __shared__ __attribute__((aligned(16))) float Ws[32 * kLQ];          // r (x - m)[row chunk][i tile]
  __shared__ __attribute__((aligned(16))) float Xs[32 * kLQ];          // (x - m)[row chunk][j tile]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, li = lane & 31, lh = lane >> 5;
  int ti = 0, t = blockIdx.x;                                          // tile (ti, tj), tj <= ti, in row-major order of the triangle
  while (t > ti) { t -= ti + 1; ++ti; }
  const int tj = t, i0 = ti * 64, j0 = tj * 64;
  const int k = blockIdx.y, s = blockIdx.z;
  const long lo = (long)s * per, hi = lo + per < N ? lo + per : N;
  const float* mk = m + (long)k * D;
  const int row = tid >> 3, cq = (tid & 7) * 8;                        // staging: 32 rows x 64 columns, 8 per thread
  float mi[8], mj[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    mi[u] = i0 + cq + u < D ? mk[i0 + cq + u] : 0.f;
    mj[u] = j0 + cq + u < D ? mk[j0 + cq + u] : 0.f;
  }
  f32x16 acc;
  double accd[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc[i] = 0.f; accd[i] = 0.0; }
  float wv[8], xv[8];
  auto fetch = [&](long n) {                                           // n: the chunk's first row
    const long nn = n + row;
    const bool in = nn < hi && !(nonfinite && nonfinite[nn]);
    const float rv = in ? r[nn * K + k] : 0.f;
    const float* xr = X + (in ? nn : 0) * D;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int ci = i0 + cq + u, cj = j0 + cq + u;
      wv[u] = (in && ci < D) ? rv * (xr[ci] - mi[u]) : 0.f;
      xv[u] = (in && cj < D) ? xr[cj] - mj[u] : 0.f;
    }
  };
  if (lo < hi) fetch(lo);
  int inblock = 0;
  for (long n = lo; n < hi; n += 32) {
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      Ws[row * kLQ + cq + u] = wv[u];
      Xs[row * kLQ + cq + u] = xv[u];
    }
    __syncthreads();
    if (n + 32 < hi) fetch(n + 32);
#pragma unroll
    for (int kg = 0; kg < 4; ++kg)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int mm = kg * 8 + 4 * lh + j;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[mm * kLQ + wm * 32 + li], Xs[mm * kLQ + wn * 32 + li], acc, 0, 0, 0);
      }
    if (++inblock == kMBlockChunks) {
#pragma unroll
      for (int i = 0; i < 16; ++i) { accd[i] += (double)acc[i]; acc[i] = 0.f; }
      inblock = 0;
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) accd[i] += (double)acc[i];
  double* out = mat + ((long)s * K + k) * D * D;
  const int col = j0 + wn * 32 + li;
  if (col < D) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ri = i0 + wm * 32 + 8 * (i >> 2) + 4 * lh + (i & 3);
      if (ri < D) out[(long)ri * D + col] = accd[i];
    }
  }
}

// One thread per output element: e in [0, K * (1 + 2 D)) the vectors, behind them for full the K * D * D matrix elements with
// j <= i, which also write their mirror.  The diagonal of the full S2 comes from the vector part (float64 throughout).
__global__ __launch_bounds__(kGmmThreads) void gmm_mstep_merge_kernel(
    const double* __restrict__ vec, const double* __restrict__ mat, int S, int D, int K, int full, double* __restrict__ Nk,
    double* __restrict__ S1, double* __restrict__ S2) {
  const long nvec = (long)K * (1 + 2 * D);
  const long e = (long)blockIdx.x * kGmmThreads + threadIdx.x;
  if (e < nvec) {
    double a = 0.0;
    for (int s = 0; s < S; ++s) a += vec[(long)s * nvec + e];
    const int k = (int)(e / (1 + 2 * D)), q = (int)(e - (long)k * (1 + 2 * D));
    if (q == 0) Nk[k] = a;
    else if (q <= D) S1[(long)k * D + q - 1] = a;
    else if (full) S2[((long)k * D + (q - 1 - D)) * D + (q - 1 - D)] = a;
    else S2[(long)k * D + q - 1 - D] = a;
    return;
  }
  if (!full) return;
  const long f = e - nvec, nmat = (long)K * D * D;
  if (f >= nmat) return;
  const int k = (int)(f / ((long)D * D));
  const int ij = (int)(f - (long)k * D * D), i = ij / D, j = ij - i * D;
  if (j >= i) return;
  double a = 0.0;
  for (int s = 0; s < S; ++s) a += mat[(long)s * nmat + f];
  S2[((long)k * D + i) * D + j] = a;
  S2[((long)k * D + j) * D + i] = a;
}

__global__ __launch_bounds__(kGmmThreads) void gmm_sample_kernel(
    const float* __restrict__ u, const float* __restrict__ eps, int D, int K, int full, const double* __restrict__ cdf,
    const float* __restrict__ mu, const float* __restrict__ L, float* __restrict__ z, int* __restrict__ comp) {
  __shared__ float es[kGmmMaxD];
  const long n = blockIdx.x;
  const int i = threadIdx.x;
  const double uv = (double)u[n];
  int k = K - 1;
  for (int c = K - 1; c >= 0; --c)
    if (cdf[c] > uv) k = c;                                            // the first index whose cdf exceeds u
  if (i < D) es[i] = eps[n * D + i];
  __syncthreads();
  if (i == 0) comp[n] = k;
  if (i >= D) return;
  float a = mu[(long)k * D + i];
  if (full) {
    const float* Lr = L + ((long)k * D + i) * D;
    for (int j = 0; j <= i; ++j) a = fmaf(Lr[j], es[j], a);
  } else {
    a = fmaf(L[(long)k * D + i], es[i], a);
  }
  z[n * D + i] = a;
}

bool gmm_dims_ok(int D, int K) { return D >= 1 && D <= kGmmMaxD && K >= 1 && K <= kGmmMaxK; }

}  // namespace

int launch_gmm_estep(const float* X, int N, int D, int K, int full, const float* log_w, const float* mu, const float* P,
                     const float* ldh, float* r, float* ll, int* nonfinite, hipStream_t st) {
  if (!X || !log_w || !mu || !P || !ldh || !r || !ll || !nonfinite) return kErrBadArg;
  if (N < 0 || !gmm_dims_ok(D, K)) return kErrBadArg;
  if (N == 0) return 0;
  const int wgs = (N + kERows - 1) / kERows;
  if (full) {
    ProfScope ps("gmm_estep_full_kernel", st, 2.0 * N * D * D * K, 4.0 * N * (D + K + 2) + 4.0 * K * D * D);
    hipLaunchKernelGGL(gmm_estep_full_kernel, dim3(wgs), dim3(kGmmThreads), 0, st, X, N, D, K, log_w, mu, P, ldh, r, ll, nonfinite);
    CTVAE_LAUNCH_CHECK();
  } else {
    ProfScope ps("gmm_estep_diag_kernel", st, 4.0 * N * D * K, 4.0 * N * (D + K + 2) + 8.0 * K * D);
    hipLaunchKernelGGL(gmm_estep_diag_kernel, dim3(wgs), dim3(kGmmThreads), 0, st, X, N, D, K, log_w, mu, P, ldh, r, ll, nonfinite);
    CTVAE_LAUNCH_CHECK();
  }
  return 0;
}

int gmm_mstep_slabs(int N, int D, int K, int full) {
  if (N < 1 || !gmm_dims_ok(D, K)) return 0;
  long S = ((long)N + kMSlabRows - 1) / kMSlabRows;
  if (S > 64) S = 64;
  const size_t per_slab = (size_t)K * (1 + 2 * D + (full ? (size_t)D * D : 0)) * sizeof(double);
  const long cap = (long)(kMWsCap / per_slab);
  if (S > cap) S = cap;
  return S < 1 ? 1 : (int)S;
}

size_t gmm_mstep_workspace_bytes(int N, int D, int K, int full) {
  const int S = gmm_mstep_slabs(N, D, K, full);
  return (size_t)S * K * (1 + 2 * D + (full ? (size_t)D * D : 0)) * sizeof(double);
}

int launch_gmm_mstep(const float* X, const float* r, const int* nonfinite, int N, int D, int K, int full, const float* m, double* Nk,
                     double* S1, double* S2, double* ws, size_t ws_bytes, hipStream_t st) {
  if (!X || !r || !m || !Nk || !S1 || !S2 || !ws) return kErrBadArg;
  if (N < 1 || !gmm_dims_ok(D, K) || N < K) return kErrBadArg;
  if (ws_bytes < gmm_mstep_workspace_bytes(N, D, K, full) || ((uintptr_t)ws & 7)) return kErrWorkspace;
  const int S = gmm_mstep_slabs(N, D, K, full);
  int per = (N + S - 1) / S;
  per = (per + 31) / 32 * 32;                                          // whole 32-row chunks: the block boundaries do not move
  double* vec = ws;
  double* mat = ws + (size_t)S * K * (1 + 2 * D);
  {
    ProfScope ps("gmm_mstep_vec_kernel", st, 6.0 * N * D * K, 4.0 * N * K * (D + 1));
    hipLaunchKernelGGL(gmm_mstep_vec_kernel, dim3(K, S), dim3(kGmmThreads), 0, st, X, r, nonfinite, N, D, K, per, m, vec);
    CTVAE_LAUNCH_CHECK();
  }
  if (full) {
    const int nt = (D + 63) / 64, tiles = nt * (nt + 1) / 2;
    ProfScope ps("gmm_mstep_full_kernel", st, 2.0 * N * 4096.0 * tiles * K, 4.0 * N * K * tiles * 130.0);
    hipLaunchKernelGGL(gmm_mstep_full_kernel, dim3(tiles, K, S), dim3(kGmmThreads), 0, st, X, r, nonfinite, N, D, K, per, m, mat);
    CTVAE_LAUNCH_CHECK();
  }
  const long elems = (long)K * (1 + 2 * D) + (full ? (long)K * D * D : 0);
  ProfScope ps("gmm_mstep_merge_kernel", st, 1.0 * S * elems, 8.0 * (S + 1) * elems);
  hipLaunchKernelGGL(gmm_mstep_merge_kernel, dim3((unsigned)((elems + kGmmThreads - 1) / kGmmThreads)), dim3(kGmmThreads), 0, st, vec,
                     mat, S, D, K, full ? 1 : 0, Nk, S1, S2);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_gmm_sample(const float* u, const float* eps, int n, int D, int K, int full, const double* cdf, const float* mu,
                      const float* L, float* z, int* comp, hipStream_t st) {
  if (!u || !eps || !cdf || !mu || !L || !z || !comp) return kErrBadArg;
  if (n < 0 || !gmm_dims_ok(D, K)) return kErrBadArg;
  if (n == 0) return 0;
  ProfScope ps("gmm_sample_kernel", st, full ? 1.0 * n * D * D : 2.0 * n * D, 8.0 * n * D);
  hipLaunchKernelGGL(gmm_sample_kernel, dim3(n), dim3(kGmmThreads), 0, st, u, eps, D, K, full ? 1 : 0, cdf, mu, L, z, comp);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
