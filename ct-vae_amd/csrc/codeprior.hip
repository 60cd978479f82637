// Interpolated Markov prior over the code grids of the quantising models (exp_params.code_prior; codeprior.py: MarkovCodePrior):
//   code_prior_count_kernel    pos / left / up / prev += the tokens of inds          int64 [B][C][H][W] -> four int64 count tables
//   code_prior_score_kernel    logp[b][c], resp[b][c][j], bad[b]                      one workgroup per image, float64 throughout
//   code_prior_sample_kernel   inds[n][c][h][w] from the uniforms u[n][H*W][C][2]     one wavefront per image, a dependent chain
//   code_prior_embed_kernel    out[n][h][w][c*Dc + d] = codebooks[c][inds][d]         a copy of 32-bit words
//
// The model.  p(k | context) = sum_j lambda[c][j] P_j(k | row_j) over J = 5 experts: uniform (1/K), position (row h*W + w of
// pos[C][H*W][K]), left (row i[c][h][w-1] of left[C][K+1][K]; the boundary row K when w = 0), up (i[c][h-1][w]; K when h = 0) and
// previous codebook (i[c-1][h][w]; K when c = 0).  P_j(k | row) = count[row][k] / total[row]; a row whose total is 0 is 1/K.
//
// Count.  One thread per token, grid-stride; four 64-bit integer atomic adds per token onto rows that differ from token to token
// (no LDS histogram: the position table alone is C*H*W*K words).  Integer adds commute: exact, independent of the order.  A token
// whose own code or any context code lies outside [0, K) adds 1 to `invalid` and nothing else.
//
// Score.  Workgroup b owns image b.  Per codebook c the threads walk the H*W positions in strides of the workgroup, each adds
// log p and the five responsibilities of its tokens into six float64 registers in position order, and one LDS tree with a fixed
// shape adds the 256 partials: the result of a row depends on that row and the tables alone, never on the batch around it.  No
// float atomic.  An image that holds an index outside [0, K) gets bad = 1 and zeros.
//
// Sample.  Wave n owns image n and walks its C*H*W tokens in raster order, codebooks innermost.  The uniforms of 64 tokens are
// read at once (lane l: token base + l, one 16-byte load), and every lane picks the expert of ITS token from u1 and the running
// sum of lambda[c][:] -- that choice needs no context, so it is off the chain.  Per token the chain is: the expert and u2 of lane
// i (v_readlane: wave-uniform), the context code from the LDS history (one row of W*C codes: the entry of column w is the up
// neighbour until the token overwrites it, then the left neighbour of column w + 1 and the previous codebook's of c + 1), one
// row load (lane l owns the PER = ceil(K/64) consecutive codes from l*PER on), a lane-local inclusive prefix, a wave-wide
// inclusive scan of the lane sums (6 cross-lane moves of 64-bit words), t = min(total-1, floor(u2 * total)), a ballot for the
// first lane whose sum exceeds t, and that lane's code broadcast.  Expert 0 and rows with total 0 take min(K-1, floor(u2 * K))
// and skip the row.  Every float64 operation of the path is a single multiplication, addition or comparison -- there is
// nothing to contract, and contraction is off for this file all the same -- so a NumPy restatement computes the same bits.
//
// Everything is pointers and shape integers.  Refused without a launch: a null or misaligned pointer, K outside 1..512, a
// non-positive extent, more than 2^31-1 tokens per launch, and for the sampler a history row of more than kSampleMaxHist codes.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

#pragma clang fp contract(off)

namespace ctvae {

constexpr int kPriorExperts = 5;
constexpr int kPriorMaxK = 512;
constexpr int kCountThreads = 256, kCountMaxWgs = 2048;
constexpr int kScoreThreads = 256;
constexpr int kSampleMaxHist = 8192;                      // W * C codes of history in LDS (32 KiB)
constexpr int kEmbedThreads = 256;

struct PriorTables {
  const long long* pos;       // [C][HW][K]
  const long long* left;      // [C][K+1][K]
  const long long* up;
  const long long* prev;
  const long long* pos_tot;   // [C][HW]
  const long long* left_tot;  // [C][K+1]
  const long long* up_tot;
  const long long* prev_tot;
};

__global__ __launch_bounds__(kCountThreads) void code_prior_count_kernel(const long long* __restrict__ inds,
                                                                         unsigned long long* pos, unsigned long long* left,
                                                                         unsigned long long* up, unsigned long long* prev,
                                                                         unsigned long long* invalid, long n, int C, int H, int W,
                                                                         int K) {
  const int HW = H * W;
  const long stride = (long)gridDim.x * kCountThreads;
  const long long Kl = K;
  for (long e = (long)blockIdx.x * kCountThreads + threadIdx.x; e < n; e += stride) {
    const int r = (int)(e % ((long)C * HW));
    const int c = r / HW, p = r - c * HW;
    const int h = p / W, w = p - h * W;
    const long long k = inds[e];
    const long long kl = w > 0 ? inds[e - 1] : Kl;
    const long long ku = h > 0 ? inds[e - W] : Kl;
    const long long kp = c > 0 ? inds[e - HW] : Kl;
    // (a boundary is the symbol K itself; a neighbour that exists must lie inside [0, K))
    const bool ok = k >= 0 && k < Kl && kl >= 0 && (w > 0 ? kl < Kl : true) && ku >= 0 && (h > 0 ? ku < Kl : true) && kp >= 0 &&
                    (c > 0 ? kp < Kl : true);
    if (!ok) {
      atomicAdd(invalid, 1ull);
      continue;
    }
    const long rows = (long)c * (K + 1);
    atomicAdd(&pos[((long)c * HW + p) * K + k], 1ull);
    atomicAdd(&left[(rows + kl) * K + k], 1ull);
    atomicAdd(&up[(rows + ku) * K + k], 1ull);
    atomicAdd(&prev[(rows + kp) * K + k], 1ull);
  }
}

__device__ __forceinline__ double expert_prob(const long long* table, const long long* totals, long row, int K, long long k,
                                              double uniform) {
  const long long tot = totals[row];
  return tot > 0 ? (double)table[row * K + k] / (double)tot : uniform;
}

__global__ __launch_bounds__(kScoreThreads) void code_prior_score_kernel(const long long* __restrict__ inds, PriorTables t,
                                                                         const double* __restrict__ lambda, double* logp,
                                                                         double* resp, int* bad, int C, int H, int W, int K) {
  __shared__ double red[(kPriorExperts + 1) * kScoreThreads];
  const int tid = threadIdx.x, HW = H * W;
  const long b = blockIdx.x;
  const long long* img = inds + b * (long)C * HW;
  int mine = 0;
  for (long e = tid; e < (long)C * HW; e += kScoreThreads) {
    const long long k = img[e];
    mine |= (k < 0 || k >= (long long)K) ? 1 : 0;
  }
  const int any_bad = __syncthreads_or(mine);
  if (tid == 0) bad[b] = any_bad ? 1 : 0;
  if (any_bad) {
    for (int i = tid; i < C; i += kScoreThreads) logp[b * C + i] = 0.0;
    for (int i = tid; i < C * kPriorExperts; i += kScoreThreads) resp[b * C * kPriorExperts + i] = 0.0;
    return;
  }
  const double uniform = 1.0 / (double)K;
  for (int c = 0; c < C; ++c) {
    double lam[kPriorExperts], acc[kPriorExperts + 1];
#pragma unroll
    for (int j = 0; j < kPriorExperts; ++j) lam[j] = lambda[c * kPriorExperts + j];
#pragma unroll
    for (int j = 0; j <= kPriorExperts; ++j) acc[j] = 0.0;
    const long long* plane = img + (long)c * HW;
    const long rows = (long)c * (K + 1);
    for (int p = tid; p < HW; p += kScoreThreads) {
      const int h = p / W, w = p - h * W;
      const long long k = plane[p];
      const long long kl = w > 0 ? plane[p - 1] : (long long)K;
      const long long ku = h > 0 ? plane[p - W] : (long long)K;
      const long long kp = c > 0 ? plane[p - HW] : (long long)K;
      double m[kPriorExperts];
      m[0] = lam[0] * uniform;
      m[1] = lam[1] * expert_prob(t.pos, t.pos_tot, (long)c * HW + p, K, k, uniform);
      m[2] = lam[2] * expert_prob(t.left, t.left_tot, rows + kl, K, k, uniform);
      m[3] = lam[3] * expert_prob(t.up, t.up_tot, rows + ku, K, k, uniform);
      m[4] = lam[4] * expert_prob(t.prev, t.prev_tot, rows + kp, K, k, uniform);
      const double mix = (((m[0] + m[1]) + m[2]) + m[3]) + m[4];
      acc[0] += log(mix);
#pragma unroll
      for (int j = 0; j < kPriorExperts; ++j) acc[1 + j] += m[j] / mix;
    }
    __syncthreads();                     // (the previous codebook's tree has been read)
#pragma unroll
    for (int j = 0; j <= kPriorExperts; ++j) red[j * kScoreThreads + tid] = acc[j];
    __syncthreads();
    for (int s = kScoreThreads / 2; s > 0; s >>= 1) {
      if (tid < s) {
#pragma unroll
        for (int j = 0; j <= kPriorExperts; ++j) red[j * kScoreThreads + tid] += red[j * kScoreThreads + tid + s];
      }
      __syncthreads();
    }
    if (tid == 0) {
      logp[b * C + c] = red[0];
#pragma unroll
      for (int j = 0; j < kPriorExperts; ++j) resp[(b * C + c) * kPriorExperts + j] = red[(1 + j) * kScoreThreads];
    }
  }
}

__device__ __forceinline__ int lane_int(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }

__device__ __forceinline__ double lane_double(double v, int lane) {
  const long long bits = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(bits & 0xffffffffll), lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)bits >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// one wavefront per image; lane l owns the codes [l * PER, (l + 1) * PER)
template <int PER>
__global__ __launch_bounds__(64) void code_prior_sample_kernel(PriorTables t, const double* __restrict__ lambda,
                                                               const double* __restrict__ u, long long* __restrict__ out, int C,
                                                               int H, int W, int K) {
  extern __shared__ int hist[];          // [W][C]: the last code written at column w for codebook c
  const int lane = threadIdx.x, HW = H * W;
  const long T = (long)C * HW;
  const long img = blockIdx.x;
  const double* ui = u + img * T * 2;
  long long* oi = out + img * T;
  const double Kd = (double)K;
  for (long base = 0; base < T; base += 64) {
    // the uniforms and the expert of token base + lane
    const long mytok = base + lane;
    double u2_mine = 0.0;
    int j_mine = 0;
    if (mytok < T) {
      const double2 uu = *reinterpret_cast<const double2*>(ui + mytok * 2);
      u2_mine = uu.y;
      const double* lam = lambda + (mytok % C) * kPriorExperts;
      double cum = 0.0;                  // left to right, additions only
      j_mine = kPriorExperts - 1;
      bool found = false;
#pragma unroll
      for (int j = 0; j < kPriorExperts; ++j) {
        cum = cum + lam[j];
        if (!found && uu.x < cum) {
          j_mine = j;
          found = true;
        }
      }
    }
    const int steps = (int)(T - base < 64 ? T - base : 64);
    for (int i = 0; i < steps; ++i) {
      const long tok = base + i;
      const int p = (int)(tok / C), c = (int)(tok - (long)p * C);
      const int h = p / W, w = p - h * W;
      const int j = lane_int(j_mine, i);
      const double u2 = lane_double(u2_mine, i);
      const long long* row = nullptr;
      long long total = 0;
      if (j == 1) {
        const long r = (long)c * HW + p;
        row = t.pos + r * K;
        total = t.pos_tot[r];
      } else if (j >= 2) {
        int ctx = K;
        if (j == 2) {
          if (w > 0) ctx = hist[(w - 1) * C + c];
        } else if (j == 3) {
          if (h > 0) ctx = hist[w * C + c];
        } else {
          if (c > 0) ctx = hist[w * C + c - 1];
        }
        ctx = __builtin_amdgcn_readfirstlane(ctx);
        const long r = (long)c * (K + 1) + ctx;
        row = (j == 2 ? t.left : j == 3 ? t.up : t.prev) + r * K;
        total = (j == 2 ? t.left_tot : j == 3 ? t.up_tot : t.prev_tot)[r];
      }
      int k;
      if (total <= 0) {
        const long long f = (long long)(u2 * Kd);          // u2 >= 0: the conversion truncates = floor
        k = (int)(f < (long long)(K - 1) ? f : (long long)(K - 1));
      } else {
        long long cnt[PER];
#pragma unroll
        for (int q = 0; q < PER; ++q) {
          const int code = lane * PER + q;
          cnt[q] = code < K ? row[code] : 0;
        }
#pragma unroll
        for (int q = 1; q < PER; ++q) cnt[q] += cnt[q - 1];
        long long incl = cnt[PER - 1];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const long long o = __shfl_up(incl, d, 64);
          if (lane >= d) incl += o;
        }
        const long long f = (long long)(u2 * (double)total);
        const long long tt = f < total - 1 ? f : total - 1;
        const unsigned long long over = __ballot(incl > tt);
        // (the totals are the tables' row sums, so the last lane's sum exceeds tt; a table that disagrees ends at code K - 1)
        const int first = over ? __builtin_ctzll(over) : 63;
        const long long excl = incl - cnt[PER - 1];
        int kk = lane * PER + PER - 1;
#pragma unroll
        for (int q = PER - 1; q >= 0; --q)
          if (excl + cnt[q] > tt) kk = lane * PER + q;
        k = __builtin_amdgcn_readlane(kk, first);
        k = k < K - 1 ? k : K - 1;
      }
      hist[w * C + c] = k;                 // (every lane writes the same word; LDS accesses of one wave stay in order)
      if (lane == 0) oi[((long)c * H + h) * W + w] = (long long)k;
    }
  }
}

__global__ __launch_bounds__(kEmbedThreads) void code_prior_embed_kernel(const long long* __restrict__ inds,
                                                                         const unsigned* __restrict__ cb, unsigned* __restrict__ out,
                                                                         long n, int C, int HW, int K, int Dc) {
  const long stride = (long)gridDim.x * kEmbedThreads;
  const int D = C * Dc;
  for (long e = (long)blockIdx.x * kEmbedThreads + threadIdx.x; e < n; e += stride) {
    const int ch = (int)(e % D);
    const long pix = e / D;                       // image * HW + position
    const long img = pix / HW;
    const int p = (int)(pix - img * HW);
    const int c = ch / Dc, d = ch - c * Dc;
    const long long k = inds[(img * C + c) * HW + p];
    out[e] = (k >= 0 && k < (long long)K) ? cb[((long)c * K + k) * Dc + d] : 0u;      // (an index outside the codebook: zeros)
  }
}

namespace {

bool aligned8(const void* p) { return p && reinterpret_cast<uintptr_t>(p) % 8 == 0; }

bool prior_shape_ok(long B, int C, int H, int W, int K) {
  if (B < 1 || C < 1 || H < 1 || W < 1 || K < 1 || K > kPriorMaxK) return false;
  const long hw = (long)H * W;
  if (hw > 0x7fffffffl || (long)C * hw > 0x7fffffffl) return false;
  return B <= 0x7fffffffl / ((long)C * hw);
}

bool tables_ok(const long* pos, const long* left, const long* up, const long* prev) {
  return aligned8(pos) && aligned8(left) && aligned8(up) && aligned8(prev);
}

PriorTables make_tables(const long* pos, const long* left, const long* up, const long* prev, const long* pos_tot,
                        const long* left_tot, const long* up_tot, const long* prev_tot) {
  auto q = [](const long* p) { return reinterpret_cast<const long long*>(p); };
  return PriorTables{q(pos), q(left), q(up), q(prev), q(pos_tot), q(left_tot), q(up_tot), q(prev_tot)};
}

template <int PER>
void sample_launch(const PriorTables& t, const double* lambda, const double* u, long long* out, int n, int C, int H, int W, int K,
                   hipStream_t st) {
  hipLaunchKernelGGL(code_prior_sample_kernel<PER>, dim3((unsigned)n), dim3(64), (size_t)W * C * sizeof(int), st, t, lambda, u, out,
                     C, H, W, K);
}

}  // namespace

int launch_code_prior_count(const long* inds, long* pos, long* left, long* up, long* prev, long* invalid, int B, int C, int H, int W,
                            int K, hipStream_t st) {
  if (!prior_shape_ok(B, C, H, W, K) || !aligned8(inds) || !tables_ok(pos, left, up, prev) || !aligned8(invalid)) return kErrBadArg;
  const long n = (long)B * C * H * W;
  long wgs = (n + kCountThreads - 1) / kCountThreads;
  if (wgs > kCountMaxWgs) wgs = kCountMaxWgs;
  auto q = [](long* p) { return reinterpret_cast<unsigned long long*>(p); };
  ProfScope ps("code_prior_count_kernel", st, 0.0, 40.0 * (double)n);
  hipLaunchKernelGGL(code_prior_count_kernel, dim3((unsigned)wgs), dim3(kCountThreads), 0, st,
                     reinterpret_cast<const long long*>(inds), q(pos), q(left), q(up), q(prev), q(invalid), n, C, H, W, K);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_code_prior_score(const long* inds, const long* pos, const long* left, const long* up, const long* prev,
                            const long* pos_tot, const long* left_tot, const long* up_tot, const long* prev_tot, const double* lambda,
                            double* logp, double* resp, int* bad, int B, int C, int H, int W, int K, hipStream_t st) {
  if (!prior_shape_ok(B, C, H, W, K) || !aligned8(inds) || !tables_ok(pos, left, up, prev) ||
      !tables_ok(pos_tot, left_tot, up_tot, prev_tot) || !aligned8(lambda) || !aligned8(logp) || !aligned8(resp) || !bad ||
      reinterpret_cast<uintptr_t>(bad) % 4 != 0)
    return kErrBadArg;
  const PriorTables t = make_tables(pos, left, up, prev, pos_tot, left_tot, up_tot, prev_tot);
  ProfScope ps("code_prior_score_kernel", st, 0.0, 72.0 * (double)B * C * H * W);
  hipLaunchKernelGGL(code_prior_score_kernel, dim3((unsigned)B), dim3(kScoreThreads), 0, st,
                     reinterpret_cast<const long long*>(inds), t, lambda, logp, resp, bad, C, H, W, K);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int code_prior_sample_max_history() { return kSampleMaxHist; }

int launch_code_prior_sample(const long* pos, const long* left, const long* up, const long* prev, const long* pos_tot,
                             const long* left_tot, const long* up_tot, const long* prev_tot, const double* lambda, const double* u,
                             long* inds, int n, int C, int H, int W, int K, hipStream_t st) {
  if (!prior_shape_ok(n, C, H, W, K) || !tables_ok(pos, left, up, prev) || !tables_ok(pos_tot, left_tot, up_tot, prev_tot) ||
      !aligned8(lambda) || !u || reinterpret_cast<uintptr_t>(u) % 16 != 0 || !aligned8(inds))
    return kErrBadArg;
  if ((long)W * C > kSampleMaxHist) return kErrBadArg;
  const PriorTables t = make_tables(pos, left, up, prev, pos_tot, left_tot, up_tot, prev_tot);
  long long* out = reinterpret_cast<long long*>(inds);
  ProfScope ps("code_prior_sample_kernel", st, 0.0, 8.0 * (double)n * C * H * W * (K + 3));
  switch ((K + 63) / 64) {
    case 1: sample_launch<1>(t, lambda, u, out, n, C, H, W, K, st); break;
    case 2: sample_launch<2>(t, lambda, u, out, n, C, H, W, K, st); break;
    case 3: sample_launch<3>(t, lambda, u, out, n, C, H, W, K, st); break;
    case 4: sample_launch<4>(t, lambda, u, out, n, C, H, W, K, st); break;
    case 5: sample_launch<5>(t, lambda, u, out, n, C, H, W, K, st); break;
    case 6: sample_launch<6>(t, lambda, u, out, n, C, H, W, K, st); break;
    case 7: sample_launch<7>(t, lambda, u, out, n, C, H, W, K, st); break;
    default: sample_launch<8>(t, lambda, u, out, n, C, H, W, K, st); break;
  }
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_code_prior_embed(const long* inds, const float* codebooks, float* out, int n, int C, int H, int W, int K, int Dc,
                            hipStream_t st) {
  if (n < 1 || C < 1 || H < 1 || W < 1 || K < 1 || Dc < 1 || !aligned8(inds) || !codebooks || !out) return kErrBadArg;
  if ((reinterpret_cast<uintptr_t>(codebooks) | reinterpret_cast<uintptr_t>(out)) % 4 != 0) return kErrBadArg;
  const long hw = (long)H * W;
  if (hw > 0x7fffffffl || (long)C * Dc > 0x7fffffffl || (long)C * K > 0x7fffffffl / Dc) return kErrBadArg;
  const long total = (long)n * hw * C * Dc;
  long wgs = (total + kEmbedThreads - 1) / kEmbedThreads;
  if (wgs > 65536) wgs = 65536;
  ProfScope ps("code_prior_embed_kernel", st, 0.0, 8.0 * (double)total);
  hipLaunchKernelGGL(code_prior_embed_kernel, dim3((unsigned)wgs), dim3(kEmbedThreads), 0, st,
                     reinterpret_cast<const long long*>(inds), reinterpret_cast<const unsigned*>(codebooks),
                     reinterpret_cast<unsigned*>(out), total, C, (int)hw, K, Dc);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
