// Reconstruction quality at validation (exp_params.recon_stats; reconstats.py: ReconStats):
//   recon_record_kernel   per image of a batch of picture pairs a (the reconstruction), b (the target), fp32 NHWC [B][S][S][C]:
//                         mse, mae, the largest absolute error and SSIM (Wang et al. 2004: 11-tap Gaussian window, VALID positions
//                         only, C1 = (0.01 R)^2, C2 = (0.03 R)^2), all in double, into rows [row0, row0 + B) of a [capacity][4]
//                         record buffer, and an int32 flag per row: a non-finite element in either picture
//   recon_select_kernel   the K worst (ssim ascending, global row ascending) of the K held slots and the batch's B new rows
//   recon_gather_kernel   the pictures of the chosen slots, from the other side of the ping-pong state or from the batch
//
// Ownership.  One workgroup per image, and the geometry of its walk depends on S and C alone: every thread adds its own terms
// in a fixed order, the 256 partial sums meet in a fixed tree.  No atomics, one owner per output: an image's record does not
// depend on the batch it arrived in, on B or on row0.
//
// The walk of one image, per channel: input rows in chunks of kChunk = 8.  A chunk's rows of a and b are staged in LDS as fp32
// (the pixel statistics are taken from the staged values: every element is staged exactly once); the HORIZONTAL pass forms the
// five window sums over x of a, b, a a, b b, a b for the chunk's rows and leaves them, as doubles, in a ring of kRing = kChunk +
// 10 rows; the VERTICAL pass then finishes every output row whose last input row lies in this chunk: rows oy .. oy + 10 of the
// ring are all it needs, and the ring holds exactly the 18 rows the chunk's outputs span.  The five moments share the staged
// values, no row of horizontal sums is formed twice, and no full intermediate plane exists.
// LDS: ring 5 x 18 x 54 doubles = 38,880 B, stage 2 x 8 x 64 floats = 4,096 B, reduction 256 doubles = 2,048 B: 45,024 B, so
// three workgroups fit the CU's 160 KiB.
//
// Arithmetic.  The product of two fp32 values is exact in double, so fma(g, a * b, acc) rounds once.  The SSIM map itself is
// evaluated WITHOUT contraction (ssim_point): with a == b numerator and denominator are then the same bits, the map is exactly
// 1.0 and so is the mean.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kRecThreads = 256;         // the record kernel's workgroup (512 threads on 16-row chunks took the same time)
constexpr int kSelThreads = 256;         // select and gather
constexpr int kRecTaps = 11;
constexpr int kRecMaxS = 64;
constexpr int kRecMaxW = kRecMaxS - kRecTaps + 1;     // 54 valid positions per row at most
constexpr int kRecChunk = 8;
constexpr int kRecRing = kRecChunk + kRecTaps - 1;    // 18
constexpr int kRecMaxK = 32;

struct ReconConsts {
  double g[kRecTaps];
  double c1, c2;
};

__device__ __forceinline__ bool rec_nonfinite(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) == 0x7f800000u; }

// one position of the SSIM map from the five window sums; every operation rounds on its own
__device__ __forceinline__ double ssim_point(double ma, double mb, double vaa, double vbb, double vab, double c1, double c2) {
#pragma clang fp contract(off)
  const double mab = ma * mb, maa = ma * ma, mbb = mb * mb;
  const double saa = vaa - maa, sbb = vbb - mbb, sab = vab - mab;
  const double num = (2.0 * mab + c1) * (2.0 * sab + c2);
  const double den = ((maa + mbb) + c1) * ((saa + sbb) + c2);
  return num / den;
}

// fixed tree over the 256 threads' values; the result is valid in thread 0
template <bool kMax>
__device__ __forceinline__ double rec_block_reduce(double v, double* sm) {
  __syncthreads();
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int o = kRecThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double x = sm[threadIdx.x], y = sm[threadIdx.x + o];
      sm[threadIdx.x] = kMax ? (x > y ? x : y) : x + y;
    }
    __syncthreads();
  }
  return sm[0];
}

__global__ __launch_bounds__(kRecThreads) void recon_record_kernel(const float* __restrict__ a, const float* __restrict__ b, int S,
                                                                   int C, ReconConsts k, double* __restrict__ rec,
                                                                   int* __restrict__ flag, int row0) {
  __shared__ double ring[5][kRecRing][kRecMaxW];
  __shared__ float sa[kRecChunk][kRecMaxS];
  __shared__ float sb[kRecChunk][kRecMaxS];
  __shared__ double red[kRecThreads];
  const int tid = threadIdx.x;
  const int img = blockIdx.x;
  const int W = S - kRecTaps + 1;
  const long base = (long)img * S * S * C;
  double sq = 0.0, ab = 0.0, mx = 0.0, ss = 0.0;
  int bad = 0;
  for (int c = 0; c < C; ++c) {
    for (int y0 = 0; y0 < S; y0 += kRecChunk) {
      const int nr = S - y0 < kRecChunk ? S - y0 : kRecChunk;
      // ---- stage the chunk's rows of this channel; the pixel statistics ride along
      for (int i = tid; i < nr * S; i += kRecThreads) {
        const int r = i / S, x = i - r * S;
        const long at = base + ((long)(y0 + r) * S + x) * C + c;
        const float va = a[at], vb = b[at];
        sa[r][x] = va;
        sb[r][x] = vb;
        bad |= (rec_nonfinite(va) || rec_nonfinite(vb)) ? 1 : 0;
        const double d = (double)va - (double)vb;
        const double ad = d < 0.0 ? -d : d;
        sq = fma(d, d, sq);
        ab += ad;
        mx = ad > mx ? ad : mx;
      }
      __syncthreads();
      // ---- horizontal: the five window sums of the chunk's rows into the ring
      for (int i = tid; i < nr * W; i += kRecThreads) {
        const int r = i / W, x = i - r * W;
        double ha = 0.0, hb = 0.0, haa = 0.0, hbb = 0.0, hab = 0.0;
#pragma unroll
        for (int t = 0; t < kRecTaps; ++t) {
          const double va = (double)sa[r][x + t], vb = (double)sb[r][x + t], g = k.g[t];
          ha = fma(g, va, ha);
          hb = fma(g, vb, hb);
          haa = fma(g, va * va, haa);
          hbb = fma(g, vb * vb, hbb);
          hab = fma(g, va * vb, hab);
        }
        const int q = (y0 + r) % kRecRing;
        ring[0][q][x] = ha;
        ring[1][q][x] = hb;
        ring[2][q][x] = haa;
        ring[3][q][x] = hbb;
        ring[4][q][x] = hab;
      }
      __syncthreads();
      // ---- vertical: the output rows whose last input row lies in this chunk
      const int oy_lo = y0 - (kRecTaps - 1) > 0 ? y0 - (kRecTaps - 1) : 0;
      const int oy_hi = y0 + nr - (kRecTaps - 1);           // exclusive; <= S - 10 = W
      const int no = oy_hi - oy_lo;
      for (int i = tid; i < no * W; i += kRecThreads) {
        const int r = i / W, x = i - r * W;
        const int oy = oy_lo + r;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t < kRecTaps; ++t) {
          const int q = (oy + t) % kRecRing;
          const double g = k.g[t];
#pragma unroll
          for (int u = 0; u < 5; ++u) m[u] = fma(g, ring[u][q][x], m[u]);
        }
        ss += ssim_point(m[0], m[1], m[2], m[3], m[4], k.c1, k.c2);
      }
      __syncthreads();                                       // the next chunk rewrites sa / sb and the oldest ring rows
    }
  }
  const double n_el = (double)S * (double)S * (double)C;
  const double n_pos = (double)W * (double)W * (double)C;
  const double t_sq = rec_block_reduce<false>(sq, red);
  const double t_ab = rec_block_reduce<false>(ab, red);
  const double t_mx = rec_block_reduce<true>(mx, red);
  const double t_ss = rec_block_reduce<false>(ss, red);
  const double t_bad = rec_block_reduce<true>((double)bad, red);
  if (tid == 0) {
    double* o = rec + (long)(row0 + img) * 4;
    o[0] = t_sq / n_el;
    o[1] = t_ab / n_el;
    o[2] = t_mx;
    o[3] = t_ss / n_pos;
    flag[row0 + img] = t_bad != 0.0 ? 1 : 0;
  }
}

// (ssim, row) of candidate i: i < K an old slot (row < 0: empty), else batch row i - K (flagged: not a candidate)
__device__ __forceinline__ bool rec_candidate(int i, int K, const double* old_ssim, const int* old_row, const double* rec,
                                              const int* flag, int row0, double& s, int& row) {
  if (i < K) {
    row = old_row[i];
    s = old_ssim[i];
    return row >= 0;
  }
  row = row0 + (i - K);
  s = rec[(long)row * 4 + 3];
  return flag[row] == 0 && s == s;
}

// One workgroup.  Every valid candidate counts the candidates in front of it -- the keys (ssim, row) are distinct, because the
// rows are -- and the one with rank r < K owns output slot r; the slots behind the last valid candidate stay empty.  The
// candidates pass through LDS in tiles of kSelThreads, one per thread, and every thread compares its own against the tile
// (all lanes read the same LDS word: a broadcast; eight entries per turn, so that the reads overlap -- one entry per turn was
// a dependent LDS round trip each and slower than reading global memory); a candidate compared with itself is not in front
// of itself.
__global__ __launch_bounds__(kSelThreads) void recon_select_kernel(const double* __restrict__ old_ssim, const int* __restrict__ old_row,
                                                                   const double* __restrict__ rec, const int* __restrict__ flag,
                                                                   int row0, int B, int K, double* __restrict__ new_ssim,
                                                                   int* __restrict__ new_row, int* __restrict__ src) {
  __shared__ double tile_s[kSelThreads];
  __shared__ int tile_row[kSelThreads];                      // -1: not a candidate
  const int tid = threadIdx.x;
  if (tid < K) {
    new_ssim[tid] = 0.0;
    new_row[tid] = -1;
    src[tid] = -1;
  }
  __syncthreads();
  const int n = K + B;
  for (int i0 = 0; i0 < n; i0 += kSelThreads) {              // (both loops are uniform over the workgroup: n alone bounds them)
    const int i = i0 + tid;
    double s = 0.0;
    int row = -1;
    const bool mine = i < n && rec_candidate(i, K, old_ssim, old_row, rec, flag, row0, s, row);
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += kSelThreads) {
      const int j = j0 + tid;
      double sj = 0.0;
      int rj = -1;
      const bool cand = j < n && rec_candidate(j, K, old_ssim, old_row, rec, flag, row0, sj, rj);
      tile_s[tid] = sj;
      tile_row[tid] = cand ? rj : -1;
      __syncthreads();
      if (mine) {                                            // the whole tile: the entries past n hold row -1
        for (int t0 = 0; t0 < kSelThreads; t0 += 8) {          // eight entries' reads in flight at a time
          double st[8];
          int rt[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            st[u] = tile_s[t0 + u];
            rt[u] = tile_row[t0 + u];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) rank += (rt[u] >= 0 && (st[u] < s || (st[u] == s && rt[u] < row))) ? 1 : 0;
        }
      }
      __syncthreads();                                       // the next tile rewrites the two arrays
    }
    if (mine && rank < K) {
      new_ssim[rank] = s;
      new_row[rank] = row;
      src[rank] = i;                     // < K: old slot i; else batch row i - K
    }
  }
}

// grid (K, chunks): slot s of the new side gets both pictures of its source, word for word; an empty slot is zeroed
__global__ __launch_bounds__(kSelThreads) void recon_gather_kernel(const int* __restrict__ src, int K, const float* __restrict__ old_a,
                                                                   const float* __restrict__ old_b, const float* __restrict__ bat_a,
                                                                   const float* __restrict__ bat_b, long n, float* __restrict__ new_a,
                                                                   float* __restrict__ new_b) {
  const int s = blockIdx.x;
  const int from = src[s];
  const float* pa = from < 0 ? nullptr : (from < K ? old_a + (long)from * n : bat_a + (long)(from - K) * n);
  const float* pb = from < 0 ? nullptr : (from < K ? old_b + (long)from * n : bat_b + (long)(from - K) * n);
  float* qa = new_a + (long)s * n;
  float* qb = new_b + (long)s * n;
  for (long i = (long)blockIdx.y * kSelThreads + threadIdx.x; i < n; i += (long)gridDim.y * kSelThreads) {
    qa[i] = pa ? pa[i] : 0.f;
    qb[i] = pb ? pb[i] : 0.f;
  }
}

int launch_recon_record(const float* a, const float* b, int B, int S, int C, const double* consts, double* rec, int* flag, int row0,
                        int capacity, hipStream_t st) {
  if (!a || !b || !consts || !rec || !flag) return kErrBadArg;
  if (B < 0 || S < kRecTaps || S > kRecMaxS || C < 1 || row0 < 0 || capacity < 0 || (long)row0 + B > (long)capacity) return kErrBadArg;
  if (B == 0) return 0;
  ReconConsts k;
  for (int t = 0; t < kRecTaps; ++t) k.g[t] = consts[t];
  k.c1 = consts[kRecTaps];
  k.c2 = consts[kRecTaps + 1];
  if (!(k.c1 > 0.0) || !(k.c2 > 0.0)) return kErrBadArg;
  const double el = (double)B * S * S * C;
  ProfScope ps("recon_record_kernel", st, 2.0 * 110.0 * el, 8.0 * el + 36.0 * B);
  hipLaunchKernelGGL(recon_record_kernel, dim3(B), dim3(kRecThreads), 0, st, a, b, S, C, k, rec, flag, row0);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_recon_worst(const double* old_ssim, const int* old_row, const float* old_a, const float* old_b, const double* rec,
                       const int* flag, int row0, int B, int capacity, const float* bat_a, const float* bat_b, int S, int C, int K,
                       double* new_ssim, int* new_row, float* new_a, float* new_b, int* src, hipStream_t st) {
  if (!old_ssim || !old_row || !old_a || !old_b || !rec || !flag || !bat_a || !bat_b || !new_ssim || !new_row || !new_a || !new_b ||
      !src)
    return kErrBadArg;
  if (K < 1 || K > kRecMaxK || B < 0 || S < 1 || C < 1 || row0 < 0 || capacity < 0 || (long)row0 + B > (long)capacity) return kErrBadArg;
  if (old_ssim == new_ssim || old_row == new_row || old_a == new_a || old_b == new_b) return kErrBadArg;   // nothing moves in place
  const long n = (long)S * S * C;
  {
    ProfScope ps("recon_select_kernel", st, 2.0 * (K + B) * (K + B), 12.0 * (K + B) + 16.0 * K);
    hipLaunchKernelGGL(recon_select_kernel, dim3(1), dim3(kSelThreads), 0, st, old_ssim, old_row, rec, flag, row0, B, K, new_ssim,
                       new_row, src);
    CTVAE_LAUNCH_CHECK();
  }
  {
    const int chunks = (int)((n + 4 * kSelThreads - 1) / (4 * kSelThreads));
    ProfScope ps("recon_gather_kernel", st, 0.0, 16.0 * K * n);
    hipLaunchKernelGGL(recon_gather_kernel, dim3(K, chunks < 1 ? 1 : (chunks > 16 ? 16 : chunks)), dim3(kSelThreads), 0, st, src, K,
                       old_a, old_b, bat_a, bat_b, n, new_a, new_b);
    CTVAE_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace ctvae
