// Image grids as bytes (imagegrid.py): make_grid + save_image of torchvision.utils, restated in f32, for an f32 batch
// x [N][C][H][W] read IN PLACE through four element strides (the decoders hand out channels_last memory, the data stores
// contiguous NCHW).  With xmaps = min(nrow, N), ymaps = ceil(N / xmaps) the grid is Hg = ymaps*(H+pad)+pad rows of
// Wg = xmaps*(W+pad)+pad pixels; image k sits at row (k / xmaps)*(H+pad)+pad, column (k % xmaps)*(W+pad)+pad, everything else
// (borders, the empty cells of the last grid row) holds pad_value.  The output is three bytes per pixel (C == 1 replicated),
// either plain [Hg][Wg][3] or as the scanlines a PNG IDAT stream deflates: [Hg][1 + 3*Wg], each row led by filter type 0.
//   grid_range_kernel     x -> one (min, max) pair per workgroup, NaN ignored       (only with normalize and no value_range)
//   grid_compose_kernel   every workgroup merges those few pairs itself (they sit in L2: no finishing launch, no ticket),
//                         then writes the byte stream
// The scanline pitch 1 + 3*Wg is no multiple of 4, so the output is treated as ONE flat byte stream: a lane owns 16 consecutive
// bytes, finds the (row, column, channel) of each, and stores four whole dwords at once; only the stream's last partial dword
// goes out as single bytes.  Arithmetic, one f32 rounding per operation (no contraction), so that a byte equals torch's:
//   normalize:  v = (clamp(x, lo, hi) - lo) / max(hi - lo, 1e-5)     otherwise  v = x
//   byte = (uint8) clamp(v * 255 + 0.5, 0, 255)                      pad_value: the same conversion, never normalised
// NaN: fminf / fmaxf return their other operand, so the range skips it and the clamps turn it into lo, i.e. byte 0 (torch
// would propagate it into the range and blank the picture); +-inf clamp to hi / lo.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

constexpr int kGridMaxParts = 256;        // workgroups of the range pass = (min, max) pairs the compose pass merges

struct GridIn {
  const float* x;
  long sN, sC, sH, sW;      // element strides
  int N, C, H, W;
};

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// block-wide (min, max) for blockDim.x == 256; valid in every thread
__device__ __forceinline__ void block_range_256(float& lo, float& hi, float (*sm)[4]) {
  lo = wave_min(lo);
  hi = wave_max(hi);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sm[0][w] = lo; sm[1][w] = hi; }
  __syncthreads();
  lo = fminf(fminf(sm[0][0], sm[0][1]), fminf(sm[0][2], sm[0][3]));
  hi = fmaxf(fmaxf(sm[1][0], sm[1][1]), fmaxf(sm[1][2], sm[1][3]));
}

// DENSE: the batch covers n consecutive floats from a 16-byte aligned x in some order (contiguous NCHW, channels_last): a range
// does not care about the order, so the block streams them as float4.  Otherwise every element is found through its strides.
template <bool DENSE>
__global__ __launch_bounds__(256) void grid_range_kernel(GridIn in, long n, float* __restrict__ part) {
  __shared__ float sm[2][4];
  float lo = INFINITY, hi = -INFINITY;
  const long t0 = (long)blockIdx.x * 256 + threadIdx.x, nt = (long)gridDim.x * 256;
  if (DENSE) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(in.x);
    const long n4 = n >> 2;
    for (long i = t0; i < n4; i += nt) {
      const f32x4 v = x4[i];
      lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
      hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
    for (long i = (n4 << 2) + t0; i < n; i += nt) {
      lo = fminf(lo, in.x[i]);
      hi = fmaxf(hi, in.x[i]);
    }
  } else {
    const long hw = (long)in.H * in.W, chw = hw * in.C;
    for (long i = t0; i < n; i += nt) {
      const long k = i / chw, r = i - k * chw;
      const int c = (int)(r / hw), p = (int)(r - c * hw), y = p / in.W, xx = p - y * in.W;
      const float v = in.x[k * in.sN + c * in.sC + y * in.sH + xx * in.sW];
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  block_range_256(lo, hi, sm);
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = lo;
    part[2 * blockIdx.x + 1] = hi;
  }
}

struct GridOut {
  int xmaps, ymaps, pad, Hg, Wg;
  int lead;          // 1: scanlines (a filter byte in front of every row), 0: plain [Hg][Wg][3]
  int pitch;         // lead + 3 * Wg
  long total;        // Hg * pitch
};

__device__ __forceinline__ unsigned to_byte(float v) {
  return (unsigned)fminf(fmaxf(__fadd_rn(__fmul_rn(v, 255.f), 0.5f), 0.f), 255.f);      // fmaxf(NaN, 0) = 0
}

// byte `r` of output row `row`
__device__ __forceinline__ unsigned grid_byte(const GridIn& in, const GridOut& g, int row, int r, bool normalize, float lo, float hi,
                                              float den, unsigned pad_byte) {
  if (r < g.lead) return 0u;                                 // PNG filter type 0 (None)
  const int q = r - g.lead, col = q / 3, ch = q - col * 3;
  const int ch_ = in.C == 1 ? 0 : ch;
  const int cy = row / (in.H + g.pad), iy = row - cy * (in.H + g.pad) - g.pad;
  const int cx = col / (in.W + g.pad), ix = col - cx * (in.W + g.pad) - g.pad;
  const int k = cy * g.xmaps + cx;
  if (iy < 0 || ix < 0 || cy >= g.ymaps || cx >= g.xmaps || k >= in.N) return pad_byte;
  float v = in.x[k * in.sN + ch_ * in.sC + iy * in.sH + ix * in.sW];
  if (normalize) v = __fdiv_rn(__fsub_rn(fminf(fmaxf(v, lo), hi), lo), den);
  return to_byte(v);
}

// One lane = 16 consecutive bytes of the stream.  nparts > 0: lo / hi come from the range pass's pairs.
__global__ __launch_bounds__(256) void grid_compose_kernel(GridIn in, GridOut g, int normalize, const float* __restrict__ part,
                                                           int nparts, float lo, float hi, float pad_value,
                                                           uint8_t* __restrict__ out) {
  __shared__ float sm[2][4];
  if (nparts > 0) {
    lo = INFINITY;
    hi = -INFINITY;
    if ((int)threadIdx.x < nparts) {
      lo = part[2 * threadIdx.x];
      hi = part[2 * threadIdx.x + 1];
    }
    block_range_256(lo, hi, sm);
  }
  const float den = fmaxf(__fsub_rn(hi, lo), 1e-5f);
  const unsigned pad_byte = to_byte(pad_value);
  const long b0 = ((long)blockIdx.x * 256 + threadIdx.x) * 16;
  if (b0 >= g.total) return;
  int row = (int)(b0 / g.pitch), r = (int)(b0 - (long)row * g.pitch);
  const int nb = g.total - b0 < 16 ? (int)(g.total - b0) : 16;
  unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < nb) {
      w[j >> 2] |= grid_byte(in, g, row, r, normalize != 0, lo, hi, den, pad_byte) << (8 * (j & 3));
      if (++r == g.pitch) { r = 0; ++row; }
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

// the batch's floats are n consecutive ones from x: sorted by stride, every dimension of size > 1 steps over exactly the smaller ones
static bool grid_dense(const GridIn& in) {
  long st[4] = {in.sN, in.sC, in.sH, in.sW};
  long sz[4] = {in.N, in.C, in.H, in.W};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (st[j] < st[i] || (st[j] == st[i] && sz[j] < sz[i])) {
        const long a = st[i], b = sz[i];
        st[i] = st[j]; sz[i] = sz[j];
        st[j] = a; sz[j] = b;
      }
  long run = 1;
  for (int i = 0; i < 4; ++i) {
    if (sz[i] == 1) continue;
    if (st[i] != run) return false;
    run *= sz[i];
  }
  return true;
}

size_t image_grid_workspace_bytes() { return (size_t)kGridMaxParts * 2 * sizeof(float); }

int launch_image_grid_u8(const float* x, long sN, long sC, long sH, long sW, int N, int C, int H, int W, int nrow, int pad,
                         int normalize, int has_range, float lo, float hi, float pad_value, int scanlines, uint8_t* out,
                         size_t out_bytes, float* ws, size_t ws_bytes, hipStream_t st) {
  if (!x || !out || (C != 1 && C != 3) || N < 1 || H < 1 || W < 1 || nrow < 1 || pad < 0) return kErrBadArg;
  if (sN < 0 || sC < 0 || sH < 0 || sW < 0) return kErrBadArg;
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return kErrBadArg;
  GridIn in{x, sN, sC, sH, sW, N, C, H, W};
  GridOut g{};
  g.xmaps = nrow < N ? nrow : N;
  g.ymaps = (N + g.xmaps - 1) / g.xmaps;
  g.pad = pad;
  const long Hg = (long)g.ymaps * ((long)H + pad) + pad, Wg = (long)g.xmaps * ((long)W + pad) + pad;
  g.lead = scanlines ? 1 : 0;
  const long pitch = g.lead + 3 * Wg;
  if (Hg > 0x3fffffff || pitch > 0x3fffffff || Hg * pitch > 0x7fffffffL) return kErrBadArg;      // int coordinates below
  g.Hg = (int)Hg; g.Wg = (int)Wg; g.pitch = (int)pitch;
  g.total = Hg * pitch;
  if (out_bytes < (size_t)((g.total + 3) & ~3L)) return kErrBadArg;
  const long n = (long)N * C * H * W;
  int nparts = 0;
  if (normalize && !has_range) {
    if (!ws || ws_bytes < image_grid_workspace_bytes() || (reinterpret_cast<uintptr_t>(ws) & 7) != 0) return kErrBadArg;
    // a workgroup per 16 floats of every thread, at most kGridMaxParts of them
    const long want = (n + 256 * 16 - 1) / (256 * 16);
    nparts = (int)(want < kGridMaxParts ? want : kGridMaxParts);
    const bool dense = grid_dense(in) && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    ProfScope ps("grid_range_kernel", st, 2.0 * n, 4.0 * n);
    if (dense)
      hipLaunchKernelGGL(grid_range_kernel<true>, dim3(nparts), dim3(256), 0, st, in, n, ws);
    else
      hipLaunchKernelGGL(grid_range_kernel<false>, dim3(nparts), dim3(256), 0, st, in, n, ws);
    CTVAE_LAUNCH_CHECK();
  }
  const long lanes = (g.total + 15) / 16;
  ProfScope ps("grid_compose_kernel", st, 6.0 * g.total, 4.0 * n * (C == 1 ? 3 : 1) + (double)g.total);
  hipLaunchKernelGGL(grid_compose_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, in, g, normalize, ws, nparts, lo, hi,
                     pad_value, out);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// scale_each: every image k is normalised by its OWN (lo_k, hi_k) -- torchvision's make_grid(normalize=True, scale_each=True),
// what saving every picture on its own with normalize=True gives.  Same two passes, segmented:
//   grid_range_each_kernel     workgroup (p, k) -> the (min, max) of its share of image k, part[k][P][2], NaN ignored
//   grid_compose_each_kernel   a lane merges the P pairs of the image a byte lies in (they sit in L2) and keeps them while its
//                              16 bytes stay inside that image: one merge per lane almost everywhere, two across a border
// Arithmetic and NaN rule are grid_byte's: an all-NaN image has lo = +inf, hi = -inf and comes out as byte 0 everywhere.
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int kGridEachMaxParts = 16;     // workgroups per image of the segmented range pass

// DENSE: image k is C*H*W consecutive floats from the 16-byte aligned x + k*sN, in some order
template <bool DENSE>
__global__ __launch_bounds__(256) void grid_range_each_kernel(GridIn in, float* __restrict__ part) {
  __shared__ float sm[2][4];
  float lo = INFINITY, hi = -INFINITY;
  const int k = blockIdx.y, P = gridDim.x;
  const long hw = (long)in.H * in.W, chw = hw * in.C;
  const long t0 = (long)blockIdx.x * 256 + threadIdx.x, nt = (long)P * 256;
  const float* xk = in.x + k * in.sN;
  if (DENSE) {
    const f32x4* x4 = reinterpret_cast<const f32x4*>(xk);
    const long n4 = chw >> 2;
    for (long i = t0; i < n4; i += nt) {
      const f32x4 v = x4[i];
      lo = fminf(fminf(lo, v.x), fminf(v.y, fminf(v.z, v.w)));
      hi = fmaxf(fmaxf(hi, v.x), fmaxf(v.y, fmaxf(v.z, v.w)));
    }
    for (long i = (n4 << 2) + t0; i < chw; i += nt) {
      lo = fminf(lo, xk[i]);
      hi = fmaxf(hi, xk[i]);
    }
  } else {
    for (long i = t0; i < chw; i += nt) {
      const int c = (int)(i / hw), p = (int)(i - c * hw), y = p / in.W, xx = p - y * in.W;
      const float v = xk[c * in.sC + y * in.sH + xx * in.sW];
      lo = fminf(lo, v);
      hi = fmaxf(hi, v);
    }
  }
  block_range_256(lo, hi, sm);
  if (threadIdx.x == 0) {
    part[2 * ((long)k * P + blockIdx.x)] = lo;
    part[2 * ((long)k * P + blockIdx.x) + 1] = hi;
  }
}

// One lane = 16 consecutive bytes of the stream, as in grid_compose_kernel; always normalising, by the byte's own image.
__global__ __launch_bounds__(256) void grid_compose_each_kernel(GridIn in, GridOut g, const float* __restrict__ part, int P,
                                                                float pad_value, uint8_t* __restrict__ out) {
  const unsigned pad_byte = to_byte(pad_value);
  const long b0 = ((long)blockIdx.x * 256 + threadIdx.x) * 16;
  if (b0 >= g.total) return;
  int row = (int)(b0 / g.pitch), r = (int)(b0 - (long)row * g.pitch);
  const int nb = g.total - b0 < 16 ? (int)(g.total - b0) : 16;
  int kc = -1;                              // the image lo / hi / den belong to
  float lo = 0.f, hi = 0.f, den = 1.f;
  unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    if (j < nb) {
      unsigned b = 0u;                                         // r < lead: PNG filter type 0 (None)
      if (r >= g.lead) {
        const int q = r - g.lead, col = q / 3, ch = q - col * 3;
        const int ch_ = in.C == 1 ? 0 : ch;
        const int cy = row / (in.H + g.pad), iy = row - cy * (in.H + g.pad) - g.pad;
        const int cx = col / (in.W + g.pad), ix = col - cx * (in.W + g.pad) - g.pad;
        const int k = cy * g.xmaps + cx;
        if (iy < 0 || ix < 0 || cy >= g.ymaps || cx >= g.xmaps || k >= in.N) {
          b = pad_byte;
        } else {
          if (k != kc) {
            kc = k;
            lo = INFINITY;
            hi = -INFINITY;
            for (int p = 0; p < P; ++p) {
              lo = fminf(lo, part[2 * ((long)k * P + p)]);
              hi = fmaxf(hi, part[2 * ((long)k * P + p) + 1]);
            }
            den = fmaxf(__fsub_rn(hi, lo), 1e-5f);
          }
          const float v = in.x[k * in.sN + ch_ * in.sC + iy * in.sH + ix * in.sW];
          b = to_byte(__fdiv_rn(__fsub_rn(fminf(fmaxf(v, lo), hi), lo), den));
        }
      }
      w[j >> 2] |= b << (8 * (j & 3));
      if (++r == g.pitch) { r = 0; ++row; }
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

// The parameter list of launch_image_grid_u8.  With a range, or without normalize, every image has the same range and the call
// IS launch_image_grid_u8 (torchvision's scale_each changes nothing there either).
int launch_image_grid_each_u8(const float* x, long sN, long sC, long sH, long sW, int N, int C, int H, int W, int nrow, int pad,
                              int normalize, int has_range, float lo, float hi, float pad_value, int scanlines, uint8_t* out,
                              size_t out_bytes, float* ws, size_t ws_bytes, hipStream_t st) {
  if (!normalize || has_range)
    return launch_image_grid_u8(x, sN, sC, sH, sW, N, C, H, W, nrow, pad, normalize, has_range, lo, hi, pad_value, scanlines, out,
                                out_bytes, ws, ws_bytes, st);
  if (!x || !out || (C != 1 && C != 3) || N < 1 || H < 1 || W < 1 || nrow < 1 || pad < 0) return kErrBadArg;
  if (sN < 0 || sC < 0 || sH < 0 || sW < 0) return kErrBadArg;
  if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return kErrBadArg;
  GridIn in{x, sN, sC, sH, sW, N, C, H, W};
  GridOut g{};
  g.xmaps = nrow < N ? nrow : N;
  g.ymaps = (N + g.xmaps - 1) / g.xmaps;
  g.pad = pad;
  const long Hg = (long)g.ymaps * ((long)H + pad) + pad, Wg = (long)g.xmaps * ((long)W + pad) + pad;
  g.lead = scanlines ? 1 : 0;
  const long pitch = g.lead + 3 * Wg;
  if (Hg > 0x3fffffff || pitch > 0x3fffffff || Hg * pitch > 0x7fffffffL) return kErrBadArg;      // int coordinates in the kernel
  g.Hg = (int)Hg; g.Wg = (int)Wg; g.pitch = (int)pitch;
  g.total = Hg * pitch;
  if (out_bytes < (size_t)((g.total + 3) & ~3L)) return kErrBadArg;
  const long chw = (long)C * H * W, n = chw * N;
  // a workgroup per 16 floats of every thread, at most kGridEachMaxParts of them per image
  const long want = (chw + 256 * 16 - 1) / (256 * 16);
  const int P = (int)(want < kGridEachMaxParts ? want : kGridEachMaxParts);
  if (N > 65535 || !ws || ws_bytes < (size_t)N * P * 2 * sizeof(float) || (reinterpret_cast<uintptr_t>(ws) & 7) != 0) return kErrBadArg;
  GridIn one = in;
  one.N = 1;
  const bool dense = grid_dense(one) && (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (N == 1 || (sN & 3) == 0);
  {
    ProfScope ps("grid_range_each_kernel", st, 2.0 * n, 4.0 * n);
    if (dense)
      hipLaunchKernelGGL(grid_range_each_kernel<true>, dim3(P, N), dim3(256), 0, st, in, ws);
    else
      hipLaunchKernelGGL(grid_range_each_kernel<false>, dim3(P, N), dim3(256), 0, st, in, ws);
    CTVAE_LAUNCH_CHECK();
  }
  const long lanes = (g.total + 15) / 16;
  ProfScope ps("grid_compose_each_kernel", st, 6.0 * g.total, 4.0 * n * (C == 1 ? 3 : 1) + (double)g.total);
  hipLaunchKernelGGL(grid_compose_each_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, in, g, ws, P, pad_value, out);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
