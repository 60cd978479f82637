// Free bits and a device-resident weight for the Gaussian KL term (exp_params.kld_free_bits / kld_schedule; klcontrol.py,
// kernels.FreeBitsKL):
//   klfloor_kernel          per-dimension batch means of the KL, the floor, the masked gradients -- and, when one workgroup owns
//                           every column, the four scalars as well
//   klfloor_finish_kernel   the four scalars from the per-column results of several workgroups
//
// Terms.  t_bd = 1 + lv - mu^2 - e^lv in fp32, the expression of loss.hip's KL body (k_bd = -0.5 t_bd).  The column mean is
//   m_d = -0.5 * (sum_b (double)t_bd) / B,   rows added in ascending order by ONE owner thread,
// so it depends on the values alone: not on the grid, not on how the rows were staged.  a_d = 1 when m_d > lambda or m_d is not
// finite (a diverging run keeps its NaN), else 0; f_d = a_d ? m_d : lambda.  The weight is w = scale * w_dev[0], read from device
// memory by the launch: a captured launch sees the value of the replay, not of the capture.
//
// Layout (latentstat.hip's vector part, wider).  A workgroup of 1024 threads owns 128 columns over ALL rows.  Thread (q, c) =
// (tid / 128, tid % 128) forms the terms of rows q, q + 8, ... of a turn of 64 rows and leaves them in LDS; the owner (0, c) adds the
// turn's rows in order; after the last turn it publishes a_d, a barrier, and every thread walks its rows once more (mu / logvar
// are L1 / L2 hits by then) and writes
//   g_mu = a_d * (w / B) * mu,   g_lv = a_d * (w / B) * 0.5 * (e^lv - 1)      -- loss.hip's expressions at go = 1, M_N = w --
// with exactly 0.0f where a_d = 0.  No atomics, no ticket, nothing waits for another workgroup.  The reduction over the columns
// (klfloor_finish: 256 threads in column order, doubles, a fixed tree) runs at the end of the same launch when L <= 128 -- the
// models' latent sizes -- and as a second launch of one workgroup otherwise; both give the same bits.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kFloorThreads = 1024;
constexpr int kFloorCols = 128;                                  // columns per workgroup
constexpr int kFloorQ = kFloorThreads / kFloorCols;              // threads per column: 8
constexpr int kFloorRows = 64;                                   // rows whose terms are formed per turn
constexpr int kFloorPer = kFloorRows / kFloorQ;                  // rows per thread and turn: 8
constexpr int kFloorMaxL = 1024;
constexpr int kFloorFinish = 256;                                // threads that reduce over the columns

// out[0] = w * sum_d f_d, out[1] = sum_d m_d, out[2] = sum_d f_d, out[3] = #{d : a_d = 0}.  Called by every thread of a workgroup
// of at least kFloorFinish threads; m / act may be LDS or global memory.
__device__ __forceinline__ void klfloor_finish(const double* m, const int* act, int L, float lambda, float w,
                                               float* __restrict__ out, double* smd /* 8 */, int* smi /* 4 */) {
  const int tid = threadIdx.x;
  if (tid < kFloorFinish) {                                      // whole waves: the shuffles below see full waves
    double sm = 0.0, sf = 0.0;
    int nf = 0;
    for (int d = tid; d < L; d += kFloorFinish) {
      const double md = m[d];
      const bool a = act[d] != 0;
      sm += md;
      sf += a ? md : (double)lambda;
      nf += a ? 0 : 1;
    }
    sm = wave_sum_d(sm);
    sf = wave_sum_d(sf);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nf += __shfl_xor(nf, o, 64);
    if ((tid & 63) == 0) {
      smd[tid >> 6] = sm;
      smd[4 + (tid >> 6)] = sf;
      smi[tid >> 6] = nf;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const float kld = (float)(((smd[0] + smd[1]) + smd[2]) + smd[3]);
    const float fl = (float)(((smd[4] + smd[5]) + smd[6]) + smd[7]);
    out[0] = w * fl;
    out[1] = kld;
    out[2] = fl;
    out[3] = (float)(smi[0] + smi[1] + smi[2] + smi[3]);
  }
}

__global__ __launch_bounds__(kFloorThreads) void klfloor_kernel(const float* __restrict__ mu, long mu_pitch,
                                                                const float* __restrict__ lv, long lv_pitch, int B, int L,
                                                                const float* __restrict__ w_dev, float scale, float lambda,
                                                                double* __restrict__ col_m, int* __restrict__ col_a,
                                                                float* __restrict__ g_mu, float* __restrict__ g_lv,
                                                                float* __restrict__ out) {
  __shared__ float t[kFloorRows][kFloorCols];
  __shared__ double s_m[kFloorCols];
  __shared__ int s_a[kFloorCols];
  __shared__ double smd[8];
  __shared__ int smi[4];
  const int tid = threadIdx.x;
  const int c = tid & (kFloorCols - 1), q = tid / kFloorCols;
  const int d = (int)blockIdx.x * kFloorCols + c;
  const bool live = d < L, owner = live && q == 0;
  double acc = 0.0;
  for (long r0 = 0; r0 < B; r0 += kFloorRows) {                  // (long: r0 + kFloorRows may pass 2^31 - 1)
    const int nr = B - r0 < kFloorRows ? (int)(B - r0) : kFloorRows;
    float m[kFloorPer], v[kFloorPer];
#pragma unroll
    for (int u = 0; u < kFloorPer; ++u) {
      const int r = q + u * kFloorQ;
      const bool in = live && r < nr;
      m[u] = in ? mu[(r0 + r) * mu_pitch + d] : 0.f;
      v[u] = in ? lv[(r0 + r) * lv_pitch + d] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < kFloorPer; ++u) t[q + u * kFloorQ][c] = 1.f + v[u] - m[u] * m[u] - expf(v[u]);
    __syncthreads();
    if (owner)
      for (int r = 0; r < nr; ++r) acc += (double)t[r][c];
    __syncthreads();                                             // the terms are rewritten by the next rows
  }
  const float w = scale * w_dev[0];
  if (q == 0) {
    const double md = -0.5 * acc / (double)B;
    const int a = (md > (double)lambda || !__builtin_isfinite(md)) ? 1 : 0;
    s_m[c] = md;
    s_a[c] = a;
    if (live && gridDim.x > 1) {
      col_m[d] = md;
      col_a[d] = a;
    }
  }
  __syncthreads();
  if (g_mu != nullptr && live) {
    const bool a = s_a[c] != 0;
    const float ksc = w / (float)B;
    for (long r = q; r < B; r += kFloorQ) {
      const float mm = mu[r * mu_pitch + d], l = lv[r * lv_pitch + d];
      g_mu[r * L + d] = a ? ksc * mm : 0.f;
      g_lv[r * L + d] = a ? ksc * 0.5f * (expf(l) - 1.f) : 0.f;
    }
  }
  if (gridDim.x == 1) klfloor_finish(s_m, s_a, L, lambda, w, out, smd, smi);
}

__global__ __launch_bounds__(kFloorFinish) void klfloor_finish_kernel(const double* __restrict__ col_m, const int* __restrict__ col_a,
                                                                      int L, const float* __restrict__ w_dev, float scale,
                                                                      float lambda, float* __restrict__ out) {
  __shared__ double smd[8];
  __shared__ int smi[4];
  klfloor_finish(col_m, col_a, L, lambda, scale * w_dev[0], out, smd, smi);
}

size_t freebits_workspace_bytes(int L) { return L > kFloorCols ? (size_t)L * (sizeof(double) + sizeof(int)) : 0; }

int launch_freebits_kl(const float* mu, long mu_pitch, const float* lv, long lv_pitch, int B, int L, const float* w_dev, float scale,
                       float lambda, float* out4, float* g_mu, float* g_lv, float* ws, size_t ws_bytes, hipStream_t st) {
  if (!mu || !lv || !w_dev || !out4 || (g_mu == nullptr) != (g_lv == nullptr)) return kErrBadArg;
  if (B < 1 || L < 1 || L > kFloorMaxL || mu_pitch < L || lv_pitch < L) return kErrBadArg;
  if (!(lambda >= 0.f) || !(lambda < 3.0e38f) || !(scale == scale)) return kErrBadArg;
  const int wgs = (L + kFloorCols - 1) / kFloorCols;
  double* col_m = nullptr;
  int* col_a = nullptr;
  if (wgs > 1) {
    if (!ws || ((uintptr_t)ws & 7) != 0 || ws_bytes < freebits_workspace_bytes(L)) return kErrWorkspace;
    col_m = reinterpret_cast<double*>(ws);
    col_a = reinterpret_cast<int*>(col_m + L);
  }
  {
    ProfScope ps("klfloor_kernel", st, 14.0 * B * L, (g_mu ? 16.0 : 8.0) * B * L + 12.0 * L);
    hipLaunchKernelGGL(klfloor_kernel, dim3(wgs), dim3(kFloorThreads), 0, st, mu, mu_pitch, lv, lv_pitch, B, L, w_dev, scale, lambda,
                       col_m, col_a, g_mu, g_lv, out4);
  }
  CTVAE_LAUNCH_CHECK();
  if (wgs > 1) {
    ProfScope ps("klfloor_finish_kernel", st, 3.0 * L, 12.0 * L + 16.0);
    hipLaunchKernelGGL(klfloor_finish_kernel, dim3(1), dim3(kFloorFinish), 0, st, col_m, col_a, L, w_dev, scale, lambda, out4);
    CTVAE_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace ctvae
