// The learned causal graphs of CT-MCQ-VAE, per action and as pictures (causalgraph.py).
//   graph_accumulate_kernel   one batch of per-sample adjacencies adj [B][S][S] (and intervention masks mask [B][S]) added into
//                             per-group accumulators: float64 sums, int32 counts of adj > threshold, rows per group
//   heatmap_kernel            values [M][H][W] -> the bytes of a tiled, colour-mapped sheet (imggrid.hip's layout), one pass
//
// Accumulate.  group [B] names every row's group (0: no intervention, 1 + a: action a); a row whose group lies outside [0, G)
// touches nothing but the `skipped` word.  Workgroup (tile, g) owns 256 consecutive elements of group g's S*S adjacency sum (the
// tiles behind them, when there is a mask: 256 elements of its S mask sum) -- one element per thread, so nobody else ever
// writes it: no atomics, and every element ends up as  (((old + x_r0) + x_r1) + ...)  over the group's rows r0 < r1 < ... in
// ascending order, whatever the launch geometry and however the rows were split into calls.  The walk: 256 rows of `group` at a
// time, every thread looks at one, a ballot + popcount compaction leaves the matching row numbers in LDS IN ORDER; then every
// thread loads its element of up to kRowsAhead listed rows at once (consecutive lanes, consecutive floats: coalesced; the loads
// do not depend on each other, only the adds do) and adds them in list order.  float -> double is exact and a double add
// rounds once, so the result equals a numpy loop bit for bit.  Tile 0 of a group adds the row counts with plain stores.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kGraphThreads = 256;
constexpr int kRowsAhead = 8;

__global__ __launch_bounds__(kGraphThreads) void graph_accumulate_kernel(
    const float* __restrict__ adj, const int* __restrict__ group, const float* __restrict__ mask, float thr, int B, int S, int G,
    int adj_tiles, double* __restrict__ adj_sum, int* __restrict__ edge_count, double* __restrict__ mask_sum, int* __restrict__ rows,
    int* __restrict__ mask_rows, int* __restrict__ skipped) {
  __shared__ int list[kGraphThreads];
  __shared__ int wcnt[2][4];                                   // per wave: matching rows, rows outside [0, G)
  const int g = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const bool is_adj = (int)blockIdx.x < adj_tiles;
  const long ne = is_adj ? (long)S * S : (long)S;              // elements per row of what this workgroup sums
  const long e = (long)(is_adj ? blockIdx.x : blockIdx.x - adj_tiles) * kGraphThreads + tid;
  const bool live = e < ne;
  const float* __restrict__ src = is_adj ? adj : mask;
  double* __restrict__ dst = is_adj ? adj_sum : mask_sum;
  double acc = live ? dst[g * ne + e] : 0.0;
  int cnt = (live && is_adj) ? edge_count[g * ne + e] : 0;
  int nrows = 0, nbad = 0;
  for (int b0 = 0; b0 < B; b0 += kGraphThreads) {
    const int b = b0 + tid;
    const int gb = b < B ? group[b] : 0;
    const bool hit = b < B && gb == g, bad = b < B && (gb < 0 || gb >= G);
    const unsigned long long mh = __ballot(hit), mb = __ballot(bad);
    if (lane == 0) {
      wcnt[0][w] = __popcll(mh);
      wcnt[1][w] = __popcll(mb);
    }
    __syncthreads();
    int off = 0, n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < w) off += wcnt[0][i];
      n += wcnt[0][i];
      nbad += wcnt[1][i];
    }
    if (hit) list[off + __popcll(mh & ((1ull << lane) - 1ull))] = b;
    __syncthreads();
    if (live) {
      for (int i = 0; i < n; i += kRowsAhead) {
        float v[kRowsAhead];
#pragma unroll
        for (int u = 0; u < kRowsAhead; ++u) v[u] = i + u < n ? src[(long)list[i + u] * ne + e] : 0.f;
#pragma unroll
        for (int u = 0; u < kRowsAhead; ++u) {
          if (i + u < n) {
            acc += (double)v[u];
            cnt += v[u] > thr ? 1 : 0;
          }
        }
      }
    }
    nrows += n;
    __syncthreads();                                           // list / wcnt are rewritten by the next 256 rows
  }
  if (live) {
    dst[g * ne + e] = acc;
    if (is_adj) edge_count[g * ne + e] = cnt;
  }
  if (blockIdx.x == 0 && tid == 0) {                           // adjacency tile 0 of the group: the only writer of these words
    rows[g] += nrows;
    if (mask) mask_rows[g] += nrows;
    if (g == 0) skipped[0] += nbad;
  }
}

int launch_graph_accumulate(const float* adj, const int* group, const float* mask, float thr, int B, int S, int G, double* adj_sum,
                            int* edge_count, double* mask_sum, int* rows, int* mask_rows, int* skipped, hipStream_t st) {
  if (!adj || !group || !adj_sum || !edge_count || !mask_sum || !rows || !mask_rows || !skipped) return kErrBadArg;
  if (B < 0 || S < 1 || S > 46340 || G < 1 || G > 65535) return kErrBadArg;      // S*S in an int, G a grid dimension
  if (B == 0) return 0;
  const long ss = (long)S * S;
  const int adj_tiles = (int)((ss + kGraphThreads - 1) / kGraphThreads);
  const int mask_tiles = mask ? (S + kGraphThreads - 1) / kGraphThreads : 0;
  ProfScope ps("graph_accumulate_kernel", st, 2.0 * B * ss, 4.0 * B * ss + 24.0 * G * ss);
  hipLaunchKernelGGL(graph_accumulate_kernel, dim3(adj_tiles + mask_tiles, G), dim3(kGraphThreads), 0, st, adj, group, mask, thr, B, S,
                     G, adj_tiles, adj_sum, edge_count, mask_sum, rows, mask_rows, skipped);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Heat map.  Every value becomes cell x cell pixels of colour table[floor(t*255 + 0.5)], t = (clamp(v, lo, hi) - lo) / (hi - lo)
// -- imggrid.hip's byte conversion, one f32 rounding per operation; NaN clamps to lo, i.e. entry 0.  The sheet is imggrid.hip's
// grid of M tiles of H*cell x W*cell pixels; borders and the empty cells of the last grid row take the padding colour.  As
// there, the output is one flat byte stream and a lane owns 16 consecutive bytes of it; a pixel's colour is looked up once, when
// the lane meets its first byte.  The table travels as a kernel argument and is copied into LDS: no device buffer to keep.
// ---------------------------------------------------------------------------------------------------------------------------
struct HeatTable {
  unsigned w[192];          // 256 x RGB, packed
};

struct HeatGeom {
  int M, H, W, cell, xmaps, ymaps, pad, lead, pitch;
  long total;
};

__global__ __launch_bounds__(256) void heatmap_kernel(const float* __restrict__ values, HeatGeom g, float lo, float hi, unsigned pad_rgb,
                                                      HeatTable table, uint8_t* __restrict__ out) {
  __shared__ unsigned tab[192];
  if (threadIdx.x < 192) tab[threadIdx.x] = table.w[threadIdx.x];
  __syncthreads();
  const uint8_t* tb = reinterpret_cast<const uint8_t*>(tab);
  const long b0 = ((long)blockIdx.x * 256 + threadIdx.x) * 16;
  if (b0 >= g.total) return;
  const float den = __fsub_rn(hi, lo);
  const int th = g.H * g.cell + g.pad, tw = g.W * g.cell + g.pad;      // tile pitch in pixels
  int row = (int)(b0 / g.pitch), r = (int)(b0 - (long)row * g.pitch);
  const int nb = g.total - b0 < 16 ? (int)(g.total - b0) : 16;
  int col = 0, ch = -1;                                                 // ch < 0: the pixel of the next byte is not known yet
  unsigned rgb = 0u;
  unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < nb) {
      unsigned byte = 0u;                                               // r < lead: PNG filter type 0 (None)
      if (r >= g.lead) {
        if (ch < 0) {
          const int q = r - g.lead;
          col = q / 3;
          ch = q - col * 3;
          rgb = pad_rgb;
          const int cy = row / th, iy = row - cy * th - g.pad;
          const int cx = col / tw, ix = col - cx * tw - g.pad;
          const int k = cy * g.xmaps + cx;
          if (iy >= 0 && ix >= 0 && cy < g.ymaps && cx < g.xmaps && k < g.M) {
            const float v = values[((long)k * g.H + iy / g.cell) * g.W + ix / g.cell];
            const float t = __fdiv_rn(__fsub_rn(fminf(fmaxf(v, lo), hi), lo), den);      // fmaxf(NaN, lo) = lo
            const unsigned idx = (unsigned)fminf(fmaxf(__fadd_rn(__fmul_rn(t, 255.f), 0.5f), 0.f), 255.f);
            rgb = (unsigned)tb[3 * idx] | ((unsigned)tb[3 * idx + 1] << 8) | ((unsigned)tb[3 * idx + 2] << 16);
          }
        }
        byte = (rgb >> (8 * ch)) & 0xffu;
        if (++ch == 3) ch = -1;
      }
      w[j >> 2] |= byte << (8 * (j & 3));
      if (++r == g.pitch) { r = 0; ++row; ch = -1; }
    }
  }
  if (nb == 16) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 v;
    v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    *reinterpret_cast<u32x4*>(out + b0) = v;
  } else {                                                   // the stream's last lane: whole dwords, then single bytes
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (4 * d + 4 <= nb) {
        *reinterpret_cast<unsigned*>(out + b0 + 4 * d) = w[d];
      } else {
        for (int j = 4 * d; j < nb; ++j) out[b0 + j] = (uint8_t)(w[d] >> (8 * (j & 3)));
      }
    }
  }
}

int launch_heatmap_u8(const float* values, int M, int H, int W, float lo, float hi, int cell, int nrow, int pad, int pad_r, int pad_g,
                      int pad_b, const uint8_t* table, int scanlines, uint8_t* out, size_t out_bytes, hipStream_t st) {
  if (!values || !table || !out || M < 1 || H < 1 || W < 1 || cell < 1 || nrow < 1 || pad < 0 || !(hi > lo)) return kErrBadArg;
  if ((pad_r | pad_g | pad_b) < 0 || pad_r > 255 || pad_g > 255 || pad_b > 255) return kErrBadArg;
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return kErrBadArg;
  if ((long)H * cell > 0x3fffffff || (long)W * cell > 0x3fffffff || (long)M * H * W > 0x7fffffffL) return kErrBadArg;
  HeatGeom g{};
  g.M = M; g.H = H; g.W = W; g.cell = cell; g.pad = pad;
  g.xmaps = nrow < M ? nrow : M;
  g.ymaps = (M + g.xmaps - 1) / g.xmaps;
  const long Hg = (long)g.ymaps * ((long)H * cell + pad) + pad, Wg = (long)g.xmaps * ((long)W * cell + pad) + pad;
  g.lead = scanlines ? 1 : 0;
  const long pitch = g.lead + 3 * Wg;
  if (Hg > 0x3fffffff || pitch > 0x3fffffff || Hg * pitch > 0x7fffffffL) return kErrBadArg;      // int coordinates in the kernel
  g.pitch = (int)pitch;
  g.total = Hg * pitch;
  if (out_bytes < (size_t)((g.total + 3) & ~3L)) return kErrBadArg;
  HeatTable t;
  for (int i = 0; i < 192; ++i)
    t.w[i] = (unsigned)table[4 * i] | ((unsigned)table[4 * i + 1] << 8) | ((unsigned)table[4 * i + 2] << 16) | ((unsigned)table[4 * i + 3] << 24);
  const unsigned pad_rgb = (unsigned)pad_r | ((unsigned)pad_g << 8) | ((unsigned)pad_b << 16);
  const long lanes = (g.total + 15) / 16;
  ProfScope ps("heatmap_kernel", st, 6.0 * g.total, 4.0 * M * H * W + (double)g.total);
  hipLaunchKernelGGL(heatmap_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, values, g, lo, hi, pad_rgb, t, out);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
