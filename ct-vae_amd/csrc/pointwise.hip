// HBM-bound pointwise kernels of the training step: layout changes at the NCHW API boundary,
// activation backward, Gaussian reparameterisation (vanilla_vae.py:107-117) and the flat fused Adam
// update (experiment.py:158-160).  Roofline for all of them: bytes moved / 8 TB/s.
#include "common.hpp"
#include "ops.hpp"
#include "prof.hpp"

namespace ctvae {

// out[b][p][c] = in[b][c][p]   (NCHW -> NHWC with p = h*W+w), or the inverse with to_nhwc = 0
__global__ __launch_bounds__(256) void permute_cp_kernel(const float* __restrict__ in, float* __restrict__ out, int B,
                                                         int C, int P, int to_nhwc) {
  const long n = (long)B * C * P;
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    if (to_nhwc) {  // i indexes out [b][p][c]
      int c = (int)(i % C);
      long t = i / C;
      int p = (int)(t % P);
      long b = t / P;
      out[i] = in[(b * C + c) * P + p];
    } else {  // i indexes out [b][c][p]
      int p = (int)(i % P);
      long t = i / P;
      int c = (int)(t % C);
      long b = t / C;
      out[i] = in[(b * P + p) * C + c];
    }
  }
}

// The picture's case, C = 3 and P % 4 == 0: one thread moves 4 pixels with three 16-byte loads and three 16-byte stores
// (the element-wise kernel above spends two 64-bit divisions and a 4-byte access pair per element: 11 us for the 12.6 MB batch
// of VanillaVAE bs = 256 at the head of every step).
__global__ __launch_bounds__(256) void permute3_kernel(const float* __restrict__ in, float* __restrict__ out, long quads, int P4,
                                                       int to_nhwc) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;   // quad index: (b, p/4)
  if (i >= quads) return;
  const long b = i / P4;
  const int q = (int)(i - b * P4);
  const f32x4* planes = reinterpret_cast<const f32x4*>(in) + b * 3 * P4 + q;        // NCHW side: plane c at + c*P4
  f32x4* oplanes = reinterpret_cast<f32x4*>(out) + b * 3 * P4 + q;
  const f32x4* pix = reinterpret_cast<const f32x4*>(in) + (b * P4 + q) * 3;         // NHWC side: 12 consecutive floats
  f32x4* opix = reinterpret_cast<f32x4*>(out) + (b * P4 + q) * 3;
  if (to_nhwc) {
    const f32x4 r = planes[0], g = planes[P4], bl = planes[2 * P4];
    opix[0] = f32x4{r[0], g[0], bl[0], r[1]};
    opix[1] = f32x4{g[1], bl[1], r[2], g[2]};
    opix[2] = f32x4{bl[2], r[3], g[3], bl[3]};
  } else {
    const f32x4 v0 = pix[0], v1 = pix[1], v2 = pix[2];
    oplanes[0] = f32x4{v0[0], v0[3], v1[2], v2[1]};
    oplanes[P4] = f32x4{v0[1], v1[0], v1[3], v2[2]};
    oplanes[2 * P4] = f32x4{v0[2], v1[1], v2[0], v2[3]};
  }
}

// gin = gout * act'(out)
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ out,
                                                      float* __restrict__ gin, long n, int act) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) gin[i] = gout[i] * act_bwd_from_out(out[i], act);
}

// out = act(in)   (standalone nn.LeakyReLU sites, mcq_vae.py:185,216, when not fused into a producer)
__global__ __launch_bounds__(256) void act_fwd_kernel(const float* __restrict__ in, float* __restrict__ out, long n, int act) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) out[i] = act_fwd(in[i], act);
}

// z = eps * exp(0.5*logvar) + mu          (row strides allow mu/logvar to be column slices of one head GEMM)
__global__ __launch_bounds__(256) void reparam_fwd_kernel(const float* __restrict__ mu, long mu_rs, const float* __restrict__ lv,
                                                          long lv_rs, const float* __restrict__ eps, float* __restrict__ z,
                                                          int B, int L) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * L) return;
  const int b = i / L, d = i - b * L;
  z[i] = eps[i] * expf(0.5f * lv[b * lv_rs + d]) + mu[b * mu_rs + d];
}

// g_mu = g_z ; g_lv = g_z * eps * 0.5 * exp(0.5*logvar)
__global__ __launch_bounds__(256) void reparam_bwd_kernel(const float* __restrict__ gz, const float* __restrict__ lv, long lv_rs,
                                                          const float* __restrict__ eps, float* __restrict__ gmu,
                                                          float* __restrict__ glv, int B, int L) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * L) return;
  const int b = i / L, d = i - b * L;
  const float g = gz[i];
  gmu[i] = g;
  glv[i] = g * eps[i] * 0.5f * expf(0.5f * lv[b * lv_rs + d]);
}

// ---- Gaussian latent as one node (vanilla_vae.py:85-92,107-122): heads [B][2L] = fc_mu | fc_var output ----------------------
// forward : z = eps * exp(0.5*logvar) + mu with mu = heads[:, :L], logvar = heads[:, L:]; eps given, or drawn here:
//           Philox4x32-10 keyed by rng[0] with counter (rng[1], element quad), Box-Muller -> N(0,1); eps is kept for backward.
// backward: g_heads[:, :L] = g_mu + g_z,  g_heads[:, L:] = g_logvar + g_z * eps * 0.5 * exp(0.5*logvar) in one launch (autograd
//           otherwise adds the two contributions with a launch each and concatenates with a third); when the noise was drawn
//           here, thread 0 advances rng[1] -- the forward kernel of the next step runs strictly later.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// slices != nullptr: the heads are still S raw split-K slices [S][B][2L] of the fc_mu | fc_var GEMM (SplitKRaw, pixel-major):
// this kernel sums them (+ bias), writes `heads` for the loss / the backward pass and goes on -- the split-K finish launch between
// the GEMM and the latent disappears
__global__ __launch_bounds__(256) void gauss_latent_fwd_kernel(float* __restrict__ heads, const float* __restrict__ eps_in,
                                                              const unsigned long long* __restrict__ rng, float* __restrict__ eps_out,
                                                              float* __restrict__ z, int B, int L, const float* __restrict__ slices,
                                                              int S, const float* __restrict__ bias) {
  const int q = blockIdx.x * 256 + threadIdx.x;          // one thread = four consecutive elements (L % 4 == 0)
  const int i = 4 * q;
  if (i >= B * L) return;
  const int b = i / L, d = i - b * L;
  f32x4 e;
  if (eps_in != nullptr) {
    e = *reinterpret_cast<const f32x4*>(eps_in + i);
  } else {
    const unsigned long long key = rng[0], ctr = rng[1];
    unsigned o[4];
    philox4x32_10((unsigned)q, (unsigned)ctr, (unsigned)(ctr >> 32), 0x5eedu, (unsigned)key, (unsigned)(key >> 32), o);
    // Box-Muller on two pairs; u in (0, 1]
    const float u0 = ((o[0] >> 8) + 1) * (1.f / 16777216.f), u1 = (o[1] >> 8) * (1.f / 16777216.f);
    const float u2 = ((o[2] >> 8) + 1) * (1.f / 16777216.f), u3 = (o[3] >> 8) * (1.f / 16777216.f);
    const float r0 = sqrtf(-2.f * __logf(u0)), r1 = sqrtf(-2.f * __logf(u2));
    float s0, c0, s1, c1;
    __sincosf(6.28318530718f * u1, &s0, &c0);
    __sincosf(6.28318530718f * u3, &s1, &c1);
    e = f32x4{r0 * c0, r0 * s0, r1 * c1, r1 * s1};
  }
  f32x4 mu, lv;
  if (slices != nullptr) {
    const long o = (long)b * 2 * L + d, st = (long)B * 2 * L;
    mu = f32x4{0.f, 0.f, 0.f, 0.f};
    lv = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < S; s0 += 8) {   // eight slices of loads in flight (a slice index beyond S re-reads the last one, weight 0)
      f32x4 tm[8], tl[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const long so = (long)(s0 + u < S ? s0 + u : S - 1) * st + o;
        tm[u] = *reinterpret_cast<const f32x4*>(slices + so);
        tl[u] = *reinterpret_cast<const f32x4*>(slices + so + L);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (s0 + u < S) { mu += tm[u]; lv += tl[u]; }
      }
    }
    if (bias != nullptr) {
      mu += *reinterpret_cast<const f32x4*>(bias + d);
      lv += *reinterpret_cast<const f32x4*>(bias + L + d);
    }
    *reinterpret_cast<f32x4*>(heads + o) = mu;
    *reinterpret_cast<f32x4*>(heads + o + L) = lv;
  } else {
    mu = *reinterpret_cast<const f32x4*>(heads + (long)b * 2 * L + d);
    lv = *reinterpret_cast<const f32x4*>(heads + (long)b * 2 * L + L + d);
  }
  f32x4 zz;
#pragma unroll
  for (int k = 0; k < 4; ++k) zz[k] = e[k] * expf(0.5f * lv[k]) + mu[k];
  *reinterpret_cast<f32x4*>(z + i) = zz;
  *reinterpret_cast<f32x4*>(eps_out + i) = e;
}

__global__ __launch_bounds__(256) void gauss_latent_bwd_kernel(const float* __restrict__ g_mu, const float* __restrict__ g_lv,
                                                              const float* __restrict__ g_z, const float* __restrict__ heads,
                                                              const float* __restrict__ eps, float* __restrict__ g_heads,
                                                              unsigned long long* __restrict__ rng_bump, int B, int L, int gz_slices) {
  // gz_slices > 0: g_z is gz_slices raw split-K slices [S][B][L] of decoder_input's data gradient, summed here
  const int i = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (i == 0 && rng_bump != nullptr) rng_bump[1] += 1ull;
  if (i >= B * L) return;
  const int b = i / L, d = i - b * L;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 gz = zero;
  if (g_z) {
    const int S = gz_slices > 0 ? gz_slices : 1;
    for (int s0 = 0; s0 < S; s0 += 8) {   // eight slices of loads in flight
      f32x4 t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = *reinterpret_cast<const f32x4*>(g_z + (long)(s0 + u < S ? s0 + u : S - 1) * B * L + i);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (s0 + u < S) gz += t[u];
      }
    }
  }
  const f32x4 gm = g_mu ? *reinterpret_cast<const f32x4*>(g_mu + i) : zero;
  const f32x4 gl = g_lv ? *reinterpret_cast<const f32x4*>(g_lv + i) : zero;
  const f32x4 lv = *reinterpret_cast<const f32x4*>(heads + (long)b * 2 * L + L + d);
  const f32x4 e = *reinterpret_cast<const f32x4*>(eps + i);
  f32x4 o1;
#pragma unroll
  for (int k = 0; k < 4; ++k) o1[k] = gl[k] + gz[k] * e[k] * 0.5f * expf(0.5f * lv[k]);
  *reinterpret_cast<f32x4*>(g_heads + (long)b * 2 * L + d) = gm + gz;
  *reinterpret_cast<f32x4*>(g_heads + (long)b * 2 * L + L + d) = o1;
}

// ---- Adam ---------------------------------------------------------------------------------------------
// state[0]=step (as float), [1]=lr, [2]=beta1, [3]=beta2, [4]=eps, [5]=weight_decay, [6]=beta1^t, [7]=beta2^t,
// [16 + 16k], k = 0..64: ticket counters (bits), zero between launches -- kAdamStateFloats floats in all
constexpr int kAdamTicketOffset = 16, kAdamMaxWgs = 2048, kAdamStateFloats = kAdamTicketOffset + 16 * (1 + kAdamMaxWgs / 32);
// torch.optim.Adam (no amsgrad): g += wd*p; m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
// p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
// The step counter's advance rides in this launch: every thread forms beta^t of THIS step from the stored beta^(t-1), and the
// workgroup that finishes last -- every other one has read the state by then -- writes the advanced state back.  With ONE
// ticket counter the 2048 same-address atomics serialised behind the kernel (19.5 -> 37.7 us, tools/negative), and fewer,
// fatter workgroups stream slower (512: 27.5 us, 256: 43 us): hence the two-level ticket below.
template <bool VEC>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, float* state, long n, float grad_scale) {
  const float lr = state[1], b1 = state[2], b2 = state[3], eps = state[4], wd = state[5];
  const float b1t = state[6] * b1, b2t = state[7] * b2;
  const float bc1 = 1.f - b1t, bc2 = 1.f - b2t;
  const float step_size = lr / bc1, bc2s = sqrtf(bc2);
  const long stride = (long)gridDim.x * 256;
  auto upd = [&](float& pi, float gi, float& mi, float& vi) {
    gi = gi * grad_scale + wd * pi;
    mi = b1 * mi + (1.f - b1) * gi;
    vi = b2 * vi + (1.f - b2) * gi * gi;
    pi = pi - step_size * (mi / (sqrtf(vi) / bc2s + eps));
  };
  const long n4 = VEC ? n / 4 : 0;
  if constexpr (VEC) {   // all four buffers 16-byte aligned: 16-byte accesses, two quads per thread in flight
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* m4 = reinterpret_cast<f32x4*>(m);
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += 2 * stride) {
      const long i2 = i + stride;
      const bool two = i2 < n4;
      f32x4 pa = p4[i], ga = g4[i], ma = m4[i], va = v4[i];
      f32x4 pb = two ? p4[i2] : pa, gb = two ? g4[i2] : ga, mb = two ? m4[i2] : ma, vb = two ? v4[i2] : va;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float pq = pa[q], mq = ma[q], vq = va[q];
        upd(pq, ga[q], mq, vq);
        pa[q] = pq; ma[q] = mq; va[q] = vq;
      }
      m4[i] = ma; v4[i] = va; p4[i] = pa;
      if (two) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float pq = pb[q], mq = mb[q], vq = vb[q];
          upd(pq, gb[q], mq, vq);
          pb[q] = pq; mb[q] = mq; vb[q] = vq;
        }
        m4[i2] = mb; v4[i2] = vb; p4[i2] = pb;
      }
    }
  }
  for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i];
    upd(pi, g[i], mi, vi);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
  __syncthreads();   // every thread of this workgroup holds its copy of the state
  if (threadIdx.x == 0) {
    // two-level ticket, every counter on its own 64-byte line: 32 workgroups share a first-level counter, the last of each
    // group takes a ticket of the top-level one (<= 64 groups)
    unsigned* tk = reinterpret_cast<unsigned*>(state + kAdamTicketOffset);
    const unsigned grp = blockIdx.x >> 5, ngrp = (gridDim.x + 31) >> 5;
    const unsigned gsize = gridDim.x - grp * 32 < 32 ? gridDim.x - grp * 32 : 32;
    if (atomicAdd(tk + 16 * (1 + grp), 1u) == gsize - 1) {
      atomicExch(tk + 16 * (1 + grp), 0u);
      if (atomicAdd(tk, 1u) == ngrp - 1) {
        atomicExch(tk, 0u);
        state[0] += 1.f;
        state[6] = b1t;
        state[7] = b2t;
      }
    }
  }
}

// ---- gradient clipping in front of the Adam step -------------------------------------------------------
// torch.nn.utils.clip_grad_norm_(max_norm = clip, norm_type = 2) / clip_grad_value_(clip) on the DDP-averaged gradient
// g * grad_scale, then Adam on the clipped gradient (weight decay added after the clip, as torch.optim.Adam does).
// Norm mode is two launches: grad_sqnorm_kernel writes one fp32 partial of sum (g * grad_scale)^2 per workgroup, and every
// workgroup of adam_clip_kernel merges those partials itself, from L2: the kernel boundary makes them visible, no in-launch
// hand-over.  The grid, the elements each thread adds, their order and the reduction tree depend on n only -- the 16-byte
// and the scalar variant add the same elements in the same order -- so the norm is bit-reproducible run to run, between
// eager and graph replay and across DDP ranks holding the same all-reduced gradient.  Value mode is adam_clip_kernel alone.
constexpr int kClipMaxWgs = 1024, kClipNorm = 0, kClipValue = 1;

// Sum over the 256 threads of a workgroup, the same in every thread: xor butterfly per wave, then the four wave sums in a
// fixed order.  lds: 4 floats.
__device__ inline float block_sum256(float v, float* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// Thread t of workgroup b adds the quads b*256 + t + k*gridDim.x*256 (k = 0, 1, ...) element by element, then the n % 4
// trailing elements go to the first threads of workgroup 0.
template <bool VEC>
__global__ __launch_bounds__(256) void grad_sqnorm_kernel(const float* __restrict__ g, long n, float grad_scale,
                                                          float* __restrict__ partial) {
  __shared__ float lds[4];
  const long nq = n / 4, stride = (long)gridDim.x * 256, t = (long)blockIdx.x * 256 + threadIdx.x;
  auto quad = [&](long q) -> f32x4 {
    if constexpr (VEC) return reinterpret_cast<const f32x4*>(g)[q];
    else return f32x4{g[4 * q], g[4 * q + 1], g[4 * q + 2], g[4 * q + 3]};
  };
  float acc = 0.f;
  for (long i = t; i < nq; i += 2 * stride) {   // two quads in flight per thread
    const long i2 = i + stride;
    const f32x4 a = quad(i);
    const f32x4 b = i2 < nq ? quad(i2) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float x = a[q] * grad_scale;
      acc = fmaf(x, x, acc);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float x = b[q] * grad_scale;
      acc = fmaf(x, x, acc);
    }
  }
  if (t < n - 4 * nq) {
    const float x = g[4 * nq + t] * grad_scale;
    acc = fmaf(x, x, acc);
  }
  const float s = block_sum256(acc, lds);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// adam_kernel with the clip folded in.  Norm mode: c = clip / (||g * grad_scale|| + 1e-6) clamped to 1 the way torch forms
// it (reciprocal times max_norm; a NaN norm gives c = NaN, an infinite one c = 0), every gradient is multiplied by c, also
// when c == 1.  Value mode: clamp(g * grad_scale, -clip, clip), NaN stays NaN.  With grad_scale == 1 and c == 1 the update
// is bit-identical to adam_kernel's.  Workgroup 0 writes the pre-clip norm to norm_out (when not NULL).
template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void adam_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, float* state, long n, float grad_scale,
                                                        float clip, const float* partial, int nparts, float* norm_out) {
  const float lr = state[1], b1 = state[2], b2 = state[3], eps = state[4], wd = state[5];
  const float b1t = state[6] * b1, b2t = state[7] * b2;
  const float bc1 = 1.f - b1t, bc2 = 1.f - b2t;
  const float step_size = lr / bc1, bc2s = sqrtf(bc2);
  float c = 1.f;
  if constexpr (MODE == kClipNorm) {
    __shared__ float lds[4];
    float s = 0.f;
    for (int k = threadIdx.x; k < nparts; k += 256) s += partial[k];
    const float total = sqrtf(block_sum256(s, lds));
    c = (1.f / (total + 1e-6f)) * clip;
    c = c > 1.f ? 1.f : c;                     // not fminf: a NaN coefficient must stay NaN
    if (norm_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = total;
  }
  const long stride = (long)gridDim.x * 256;
  // In norm mode the weight decay joins the clipped gradient with the roundings adam_kernel's `gi * grad_scale + wd * pi`
  // compiles to -- fma(g, grad_scale, wd * p) in its 16-byte loop, fma(wd, p, g * grad_scale) in its scalar loops -- so that
  // c == 1 with grad_scale == 1 reproduces its update bit for bit on every path.
  auto upd = [&](float& pi, float gi, float& mi, float& vi, bool quad) {
    if constexpr (MODE == kClipNorm) {
      gi = quad ? fmaf(gi * grad_scale, c, wd * pi) : fmaf(wd, pi, (gi * grad_scale) * c);
    } else {
      gi = gi * grad_scale;
      gi = gi < -clip ? -clip : (gi > clip ? clip : gi);   // comparisons, not fminf / fmaxf: NaN stays NaN
      gi = fmaf(wd, pi, gi);
    }
    mi = b1 * mi + (1.f - b1) * gi;
    vi = b2 * vi + (1.f - b2) * gi * gi;
    pi = pi - step_size * (mi / (sqrtf(vi) / bc2s + eps));
  };
  const long n4 = VEC ? n / 4 : 0;
  if constexpr (VEC) {
    f32x4* p4 = reinterpret_cast<f32x4*>(p);
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
    f32x4* m4 = reinterpret_cast<f32x4*>(m);
    f32x4* v4 = reinterpret_cast<f32x4*>(v);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += 2 * stride) {
      const long i2 = i + stride;
      const bool two = i2 < n4;
      f32x4 pa = p4[i], ga = g4[i], ma = m4[i], va = v4[i];
      f32x4 pb = two ? p4[i2] : pa, gb = two ? g4[i2] : ga, mb = two ? m4[i2] : ma, vb = two ? v4[i2] : va;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float pq = pa[q], mq = ma[q], vq = va[q];
        upd(pq, ga[q], mq, vq, true);
        pa[q] = pq; ma[q] = mq; va[q] = vq;
      }
      m4[i] = ma; v4[i] = va; p4[i] = pa;
      if (two) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float pq = pb[q], mq = mb[q], vq = vb[q];
          upd(pq, gb[q], mq, vq, true);
          pb[q] = pq; mb[q] = mq; vb[q] = vq;
        }
        m4[i2] = mb; v4[i2] = vb; p4[i2] = pb;
      }
    }
  }
  for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float pi = p[i], mi = m[i], vi = v[i];
    upd(pi, g[i], mi, vi, false);
    m[i] = mi;
    v[i] = vi;
    p[i] = pi;
  }
  __syncthreads();   // every thread of this workgroup holds its copy of the state
  if (threadIdx.x == 0) {   // adam_kernel's two-level ticket: the last workgroup advances the step counter
    unsigned* tk = reinterpret_cast<unsigned*>(state + kAdamTicketOffset);
    const unsigned grp = blockIdx.x >> 5, ngrp = (gridDim.x + 31) >> 5;
    const unsigned gsize = gridDim.x - grp * 32 < 32 ? gridDim.x - grp * 32 : 32;
    if (atomicAdd(tk + 16 * (1 + grp), 1u) == gsize - 1) {
      atomicExch(tk + 16 * (1 + grp), 0u);
      if (atomicAdd(tk, 1u) == ngrp - 1) {
        atomicExch(tk, 0u);
        state[0] += 1.f;
        state[6] = b1t;
        state[7] = b2t;
      }
    }
  }
}

// ---- block-aware Adam: parameters that got no gradient stand still ---------------------------------------
// torch.optim.Adam keeps a step counter per parameter and leaves a parameter whose .grad is None alone (no moment decay, no
// weight decay, no counter advance).  FlatAdam's absent_grad = "skip" / "skip_until_first" gets that from a BLOCK TABLE over the
// flat buffer: blk_lo / blk_hi are nb sorted, disjoint ranges [lo, hi) of the n floats (floats in no range are alignment gaps:
// never read, never written), bstate[4b ..] = {step, beta1^step, beta2^step, seen} of block b, and active[b] != 0 means block b
// steps in this launch, with its OWN bias corrections.
// A workgroup owns one contiguous range of quads: thread 0 finds the first block that reaches into it by binary search, every
// thread walks on from there with a cursor that only moves forward (its quads ascend).  A quad inside one block takes the
// 16-byte path, or is skipped whole; a quad that straddles a boundary or the end of the buffer goes float by float, each
// float under its own block.  The update's roundings are adam_kernel's / adam_clip_kernel's for the same position of the
// buffer (16-byte region or tail), so with every block active and equal counters the step is theirs bit for bit.
constexpr int kClipOff = 2;

template <bool VEC, int MODE>
__global__ __launch_bounds__(256) void adam_blocks_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                          float* __restrict__ v, float* state, long n, float grad_scale, float clip,
                                                          const float* partial, int nparts, float* norm_out,
                                                          const int* __restrict__ blk_lo, const int* __restrict__ blk_hi,
                                                          float* bstate, const int* __restrict__ active, int nb) {
  __shared__ int s_first, s_last;
  const float lr = state[1], b1 = state[2], b2 = state[3], eps = state[4], wd = state[5];
  float c = 1.f;
  if constexpr (MODE == kClipNorm) {
    __shared__ float lds[4];
    float s = 0.f;
    for (int k = threadIdx.x; k < nparts; k += 256) s += partial[k];
    const float total = sqrtf(block_sum256(s, lds));
    c = (1.f / (total + 1e-6f)) * clip;
    c = c > 1.f ? 1.f : c;                     // not fminf: a NaN coefficient must stay NaN
    if (norm_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *norm_out = total;
  }
  const long nq = (n + 3) / 4;                 // the last quad may be partial
  const long qper = (nq + gridDim.x - 1) / gridDim.x;
  const long q0 = (long)blockIdx.x * qper, q1 = q0 + qper < nq ? q0 + qper : nq;
  if (threadIdx.x == 0) {                      // first block that ends behind this workgroup's first float
    const long e = 4 * q0;
    int lo = 0, hi = nb;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if ((long)blk_hi[mid] <= e) lo = mid + 1;
      else hi = mid;
    }
    s_first = lo;
  }
  __syncthreads();
  int bi = s_first, cur = -1;
  float step_size = 0.f, bc2s = 1.f;
  auto use_block = [&](int b) {                // bias corrections of block b's own step count
    if (b != cur) {
      // beta^t rounded before the subtraction, as adam_kernel has it (it stores beta^t); contracted, 1 - x * b would fuse
#pragma clang fp contract(off)
      cur = b;
      const float b1t = bstate[4 * b + 1] * b1, b2t = bstate[4 * b + 2] * b2;
      const float bc1 = 1.f - b1t, bc2 = 1.f - b2t;
      step_size = lr / bc1;
      bc2s = sqrtf(bc2);
    }
  };
  auto upd = [&](float& pi, float gi, float& mi, float& vi, bool quad) {
    // no contraction in here: every fused operation is written as one
#pragma clang fp contract(off)
    if constexpr (MODE == kClipNorm) {
      gi = quad ? fmaf(gi * grad_scale, c, wd * pi) : fmaf(wd, pi, (gi * grad_scale) * c);
    } else if constexpr (MODE == kClipValue) {
      gi = gi * grad_scale;
      gi = gi < -clip ? -clip : (gi > clip ? clip : gi);   // comparisons, not fminf / fmaxf: NaN stays NaN
      gi = fmaf(wd, pi, gi);
    } else {
      gi = quad ? fmaf(gi, grad_scale, wd * pi) : fmaf(wd, pi, gi * grad_scale);
    }
    // the moments with the roundings the compiler gives adam_kernel / adam_clip_kernel (read off the ISA): fused in their
    // 16-byte loops, two rounded products and an add in their scalar loops -- spelled out, so that this kernel's float-by-float
    // path inside the 16-byte region still rounds like their 16-byte loop
    const float gs1 = (1.f - b1) * gi, gs2 = gi * ((1.f - b2) * gi);
    if (quad) {
      mi = fmaf(b1, mi, gs1);
      vi = fmaf(b2, vi, gs2);
    } else {
      mi = b1 * mi + gs1;
      vi = b2 * vi + gs2;
    }
    pi = fmaf(-step_size, mi / (sqrtf(vi) / bc2s + eps), pi);
  };
  const long nfull = VEC ? (n / 4) * 4 : 0;    // where adam_kernel runs its 16-byte loop
  // quad q: blk >= 0 -> inside the active block blk (16-byte path); mixed -> some float of it may lie in a block, go float by float
  auto classify = [&](long q, int& blk, bool& mixed) {
    blk = -1;
    mixed = false;
    const long e0 = 4 * q;
    while (bi < nb && (long)blk_hi[bi] <= e0) ++bi;
    if (bi >= nb) return;
    const long lo = blk_lo[bi], hi = blk_hi[bi];
    if (lo <= e0 && e0 + 4 <= hi && e0 + 4 <= n) {
      if (active[bi]) {
        if (VEC) blk = bi;
        else mixed = true;
      }
    } else if (lo < e0 + 4) {
      mixed = true;
    }
  };
  auto by_float = [&](long q) {
    int bj = bi;
    for (int k = 0; k < 4; ++k) {
      const long e = 4 * q + k;
      if (e >= n) break;
      while (bj < nb && (long)blk_hi[bj] <= e) ++bj;
      if (bj >= nb) break;
      if ((long)blk_lo[bj] <= e && active[bj]) {
        use_block(bj);
        float pi = p[e], mi = m[e], vi = v[e];
        upd(pi, g[e], mi, vi, e < nfull);
        m[e] = mi;
        v[e] = vi;
        p[e] = pi;
      }
    }
  };
  f32x4* p4 = reinterpret_cast<f32x4*>(p);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
  f32x4* m4 = reinterpret_cast<f32x4*>(m);
  f32x4* v4 = reinterpret_cast<f32x4*>(v);
  for (long qa = q0 + threadIdx.x; qa < q1; qa += 512) {   // two quads per thread in flight
    const long qb = qa + 256;
    int ba, bb = -1;
    bool mixa, mixb = false;
    classify(qa, ba, mixa);
    const int bia = bi;                        // cursor at quad a, for its float-by-float walk
    if (qb < q1) classify(qb, bb, mixb);
    f32x4 pa, ga, ma, va, pb, gb, mb, vb;
    if (ba >= 0) { pa = p4[qa]; ga = g4[qa]; ma = m4[qa]; va = v4[qa]; }
    if (bb >= 0) { pb = p4[qb]; gb = g4[qb]; mb = m4[qb]; vb = v4[qb]; }
    if (ba >= 0) {
      use_block(ba);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float pq = pa[q], mq = ma[q], vq = va[q];
        upd(pq, ga[q], mq, vq, true);
        pa[q] = pq; ma[q] = mq; va[q] = vq;
      }
      m4[qa] = ma; v4[qa] = va; p4[qa] = pa;
    }
    if (bb >= 0) {
      use_block(bb);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float pq = pb[q], mq = mb[q], vq = vb[q];
        upd(pq, gb[q], mq, vq, true);
        pb[q] = pq; mb[q] = mq; vb[q] = vq;
      }
      m4[qb] = mb; v4[qb] = vb; p4[qb] = pb;
    }
    if (mixa) {
      const int keep = bi;
      bi = bia;
      by_float(qa);
      bi = keep;
    }
    if (mixb) by_float(qb);
  }
  __syncthreads();   // every thread of this workgroup has read the block states it needs
  if (threadIdx.x == 0) {   // adam_kernel's two-level ticket
    unsigned* tk = reinterpret_cast<unsigned*>(state + kAdamTicketOffset);
    const unsigned grp = blockIdx.x >> 5, ngrp = (gridDim.x + 31) >> 5;
    const unsigned gsize = gridDim.x - grp * 32 < 32 ? gridDim.x - grp * 32 : 32;
    int last = 0;
    if (atomicAdd(tk + 16 * (1 + grp), 1u) == gsize - 1) {
      atomicExch(tk + 16 * (1 + grp), 0u);
      if (atomicAdd(tk, 1u) == ngrp - 1) {
        atomicExch(tk, 0u);
        last = 1;
      }
    }
    s_last = last;
  }
  __syncthreads();
  if (s_last) {   // the workgroup that finished last: the counters of the blocks that stepped move on, the others stand
    for (int b = threadIdx.x; b < nb; b += 256) {
      if (active[b]) {
        bstate[4 * b] += 1.f;
        bstate[4 * b + 1] *= b1;
        bstate[4 * b + 2] *= b2;
        bstate[4 * b + 3] = 1.f;
      }
    }
    if (threadIdx.x == 0) {                    // launches so far; the buffer-wide beta^t keep their meaning for the record
      state[0] += 1.f;
      state[6] *= b1;
      state[7] *= b2;
    }
  }
}

// hits[k] = 1 for member 0 of a parameter bank and for every member group[b] a sample of this forward selects (racing
// threads store the same 1)
__global__ __launch_bounds__(256) void adam_mark_members_kernel(int* __restrict__ hits, int nhits, const int* __restrict__ group,
                                                                int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i == 0) hits[0] = 1;
  if (group != nullptr && i < B) {
    const int k = group[i];
    if (k >= 0 && k < nhits) hits[k] = 1;
  }
}

// active[b] = present[b] (what the host knows: a gradient kernel wrote the block / autograd produced a gradient), for a bank
// member and its hit word too; until_first: a block that has stepped once steps ever after.  Consumes the hit words.
__global__ __launch_bounds__(256) void adam_block_flags_kernel(const int* __restrict__ present, const int* __restrict__ hit_index,
                                                               int* hits, int nhits, const float* __restrict__ bstate,
                                                               int* __restrict__ active, int nb, int until_first) {
  for (int b = threadIdx.x; b < nb; b += 256) {
    int a = present[b] != 0;
    const int h = hit_index[b];
    if (h >= 0) a = a && (h < nhits && hits[h] != 0);
    if (until_first && bstate[4 * b + 3] != 0.f) a = 1;
    active[b] = a;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nhits; k += 256) hits[k] = 0;
}

// The two halves of adam_block_flags_kernel for a step whose flags are reduced across ranks in between (MAX: a block steps
// everywhere iff it got a gradient somewhere).  Local half: raw[b] = present[b] && hit(b), whatever the block's history; consumes
// the hit words.
__global__ __launch_bounds__(256) void adam_block_flags_local_kernel(const int* __restrict__ present,
                                                                     const int* __restrict__ hit_index, int* hits, int nhits,
                                                                     int* __restrict__ active, int nb) {
  for (int b = threadIdx.x; b < nb; b += 256) {
    int a = present[b] != 0;
    const int h = hit_index[b];
    if (h >= 0) a = a && (h < nhits && hits[h] != 0);
    active[b] = a;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nhits; k += 256) hits[k] = 0;
}

// Finish half, on the reduced words in place: 0 / 1 again, and until_first's "has stepped once steps ever after".
__global__ __launch_bounds__(256) void adam_block_flags_finish_kernel(const float* __restrict__ bstate, int* __restrict__ active,
                                                                      int nb, int until_first) {
  for (int b = threadIdx.x; b < nb; b += 256) {
    int a = active[b] != 0;
    if (until_first && bstate[4 * b + 3] != 0.f) a = 1;
    active[b] = a;
  }
}

// Straight-through Bernoulli sample through a 2-class Gumbel-softmax (tau = 1, hard) of
// log(clamp([1-p, p], 1e-4)) (ct_mcq_vae.py:126,177-183).  noise = 2 standard Gumbel draws/element.
__global__ __launch_bounds__(256) void gumbel_st_fwd_kernel(const float* __restrict__ p, const float* __restrict__ noise,
                                                            float* __restrict__ out, float* __restrict__ soft, long n) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float pi = p[i];
    const float a0 = logf(fmaxf(1.f - pi, 1e-4f)) + noise[2 * i];
    const float a1 = logf(fmaxf(pi, 1e-4f)) + noise[2 * i + 1];
    const float y1 = 1.f / (1.f + expf(a0 - a1));
    const float hard = a1 > a0 ? 1.f : 0.f;      // argmax keeps the first maximum on ties
    out[i] = (hard - y1) + y1;                   // y_hard - y_soft.detach() + y_soft
    soft[i] = y1;
  }
}

__global__ __launch_bounds__(256) void gumbel_st_bwd_kernel(const float* __restrict__ go, const float* __restrict__ p,
                                                            const float* __restrict__ soft, float* __restrict__ gp, long n) {
  const long stride = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float pi = p[i], y1 = soft[i];
    const float d = (pi > 1e-4f ? 1.f / pi : 0.f) + ((1.f - pi) > 1e-4f ? 1.f / (1.f - pi) : 0.f);
    gp[i] = go[i] * y1 * (1.f - y1) * d;
  }
}

static inline unsigned grid_for(long n, int cap = 4096) {
  long b = (n + 255) / 256;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (unsigned)b;
}

int launch_permute(const float* in, float* out, int B, int C, int P, int to_nhwc, hipStream_t st) {
  if (C == 3 && P % 4 == 0 && (reinterpret_cast<uintptr_t>(in) % 16) == 0 && (reinterpret_cast<uintptr_t>(out) % 16) == 0) {
    ProfScope ps("permute3_kernel", st, 0.0, 8.0 * (double)B * C * P);
    const long quads = (long)B * (P / 4);
    hipLaunchKernelGGL(permute3_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, in, out, quads, P / 4, to_nhwc);
    CTVAE_LAUNCH_CHECK();
    return 0;
  }
  ProfScope ps("permute_cp_kernel", st, 0.0, 8.0 * (double)B * C * P);
  hipLaunchKernelGGL(permute_cp_kernel, dim3(grid_for((long)B * C * P)), dim3(256), 0, st, in, out, B, C, P, to_nhwc);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_act_bwd(const float* gout, const float* out, float* gin, long n, int act, hipStream_t st) {
  ProfScope ps("act_bwd_kernel", st, 0.0, 12.0 * (double)n);
  hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, st, gout, out, gin, n, act);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_act_fwd(const float* in, float* out, long n, int act, hipStream_t st) {
  hipLaunchKernelGGL(act_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, st, in, out, n, act);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_reparam_fwd(const float* mu, long mu_rs, const float* lv, long lv_rs, const float* eps, float* z, int B, int L,
                       hipStream_t st) {
  hipLaunchKernelGGL(reparam_fwd_kernel, dim3(ceil_div(B * L, 256)), dim3(256), 0, st, mu, mu_rs, lv, lv_rs, eps, z, B, L);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_reparam_bwd(const float* gz, const float* lv, long lv_rs, const float* eps, float* gmu, float* glv, int B, int L,
                       hipStream_t st) {
  hipLaunchKernelGGL(reparam_bwd_kernel, dim3(ceil_div(B * L, 256)), dim3(256), 0, st, gz, lv, lv_rs, eps, gmu, glv, B, L);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_gumbel_fwd(const float* p, const float* noise, float* out, float* soft, long n, hipStream_t st) {
  hipLaunchKernelGGL(gumbel_st_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, st, p, noise, out, soft, n);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_gumbel_bwd(const float* go, const float* p, const float* soft, float* gp, long n, hipStream_t st) {
  hipLaunchKernelGGL(gumbel_st_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, st, go, p, soft, gp, n);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

size_t adam_state_floats() { return kAdamStateFloats; }

int launch_adam(float* p, const float* g, float* m, float* v, float* state, long n, float grad_scale, hipStream_t st) {
  ProfScope ps("adam_kernel", st, 0.0, 28.0 * (double)n);
  constexpr int wgs = 1024;
  static_assert(wgs <= kAdamMaxWgs, "the Adam state is sized for kAdamMaxWgs workgroups");
  const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                     reinterpret_cast<uintptr_t>(v)) % 16) == 0;
  if (vec) hipLaunchKernelGGL(adam_kernel<true>, dim3(grid_for(n / 4, wgs)), dim3(256), 0, st, p, g, m, v, state, n, grad_scale);
  else hipLaunchKernelGGL(adam_kernel<false>, dim3(grid_for(n, wgs)), dim3(256), 0, st, p, g, m, v, state, n, grad_scale);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

size_t grad_clip_workspace_floats() { return kClipMaxWgs; }

int launch_adam_clipped(float* p, const float* g, float* m, float* v, float* state, long n, float grad_scale, int algorithm,
                        float clip, float* ws, float* norm_out, hipStream_t st) {
  constexpr int wgs = 1024;
  static_assert(wgs <= kAdamMaxWgs, "the Adam state is sized for kAdamMaxWgs workgroups");
  const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                     reinterpret_cast<uintptr_t>(v)) % 16) == 0;
  const dim3 grid(vec ? grid_for(n / 4, wgs) : grid_for(n, wgs));
  int nparts = 0;
  if (algorithm == kClipNorm) {
    nparts = (int)grid_for(n / 4, kClipMaxWgs);     // a function of n alone: the reduction order does not follow alignment
    ProfScope ps("grad_sqnorm_kernel", st, 0.0, 4.0 * (double)n + 4.0 * nparts);
    if (reinterpret_cast<uintptr_t>(g) % 16 == 0)
      hipLaunchKernelGGL(grad_sqnorm_kernel<true>, dim3(nparts), dim3(256), 0, st, g, n, grad_scale, ws);
    else hipLaunchKernelGGL(grad_sqnorm_kernel<false>, dim3(nparts), dim3(256), 0, st, g, n, grad_scale, ws);
    CTVAE_LAUNCH_CHECK();
  }
  ProfScope ps("adam_clip_kernel", st, 0.0, 28.0 * (double)n + 4.0 * nparts);
  if (algorithm == kClipNorm) {
    if (vec) hipLaunchKernelGGL((adam_clip_kernel<true, kClipNorm>), grid, dim3(256), 0, st, p, g, m, v, state, n, grad_scale, clip,
                                ws, nparts, norm_out);
    else hipLaunchKernelGGL((adam_clip_kernel<false, kClipNorm>), grid, dim3(256), 0, st, p, g, m, v, state, n, grad_scale, clip,
                            ws, nparts, norm_out);
  } else {
    if (vec) hipLaunchKernelGGL((adam_clip_kernel<true, kClipValue>), grid, dim3(256), 0, st, p, g, m, v, state, n, grad_scale,
                                clip, nullptr, 0, nullptr);
    else hipLaunchKernelGGL((adam_clip_kernel<false, kClipValue>), grid, dim3(256), 0, st, p, g, m, v, state, n, grad_scale,
                            clip, nullptr, 0, nullptr);
  }
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_adam_mark_members(int* hits, int nhits, const int* group, int B, hipStream_t st) {
  hipLaunchKernelGGL(adam_mark_members_kernel, dim3((unsigned)((B > 1 ? B : 1) + 255) / 256), dim3(256), 0, st, hits, nhits, group, B);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_adam_block_flags(const int* present, const int* hit_index, int* hits, int nhits, const float* bstate, int* active,
                            int nb, int until_first, hipStream_t st) {
  hipLaunchKernelGGL(adam_block_flags_kernel, dim3(1), dim3(256), 0, st, present, hit_index, hits, nhits, bstate, active, nb,
                     until_first);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_adam_block_flags_local(const int* present, const int* hit_index, int* hits, int nhits, int* active, int nb,
                                  hipStream_t st) {
  hipLaunchKernelGGL(adam_block_flags_local_kernel, dim3(1), dim3(256), 0, st, present, hit_index, hits, nhits, active, nb);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_adam_block_flags_finish(const float* bstate, int* active, int nb, int until_first, hipStream_t st) {
  hipLaunchKernelGGL(adam_block_flags_finish_kernel, dim3(1), dim3(256), 0, st, bstate, active, nb, until_first);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_adam_blocks(float* p, const float* g, float* m, float* v, float* state, long n, float grad_scale, int algorithm,
                       float clip, float* ws, float* norm_out, const int* blk_lo, const int* blk_hi, float* bstate,
                       const int* active, int nb, hipStream_t st) {
  constexpr int wgs = 1024;
  static_assert(wgs <= kAdamMaxWgs, "the Adam state is sized for kAdamMaxWgs workgroups");
  if (n > 0x7fffffffL) return kErrBadArg;       // the block table holds 32-bit offsets
  const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                     reinterpret_cast<uintptr_t>(v)) % 16) == 0;
  const dim3 grid(grid_for((n + 3) / 4, wgs));
  int nparts = 0;
  if (algorithm == kClipNorm) {                 // blocks that do not step and gaps hold zeros: the norm pass is adam_clip's
    nparts = (int)grid_for(n / 4, kClipMaxWgs);
    ProfScope ps("grad_sqnorm_kernel", st, 0.0, 4.0 * (double)n + 4.0 * nparts);
    if (reinterpret_cast<uintptr_t>(g) % 16 == 0)
      hipLaunchKernelGGL(grad_sqnorm_kernel<true>, dim3(nparts), dim3(256), 0, st, g, n, grad_scale, ws);
    else hipLaunchKernelGGL(grad_sqnorm_kernel<false>, dim3(nparts), dim3(256), 0, st, g, n, grad_scale, ws);
    CTVAE_LAUNCH_CHECK();
  }
  ProfScope ps("adam_blocks_kernel", st, 0.0, 28.0 * (double)n + 4.0 * nparts);
#define CTVAE_ADAM_BLOCKS(V, M)                                                                                              \
  hipLaunchKernelGGL((adam_blocks_kernel<V, M>), grid, dim3(256), 0, st, p, g, m, v, state, n, grad_scale, clip, ws, nparts, \
                     norm_out, blk_lo, blk_hi, bstate, active, nb)
  if (algorithm == kClipNorm) {
    if (vec) CTVAE_ADAM_BLOCKS(true, kClipNorm);
    else CTVAE_ADAM_BLOCKS(false, kClipNorm);
  } else if (algorithm == kClipValue) {
    if (vec) CTVAE_ADAM_BLOCKS(true, kClipValue);
    else CTVAE_ADAM_BLOCKS(false, kClipValue);
  } else {
    if (vec) CTVAE_ADAM_BLOCKS(true, kClipOff);
    else CTVAE_ADAM_BLOCKS(false, kClipOff);
  }
#undef CTVAE_ADAM_BLOCKS
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_gauss_latent_fwd(float* heads, const float* eps_in, const unsigned long long* rng, float* eps_out, float* z, int B,
                            int L, hipStream_t st, const float* slices, int S, const float* bias) {
  if (!heads || !eps_out || !z || (!eps_in && !rng) || B <= 0 || L <= 0 || L % 4 || (slices != nullptr && S < 1)) return kErrBadArg;
  ProfScope ps("gauss_latent_fwd_kernel", st, 0.0, 4.0 * (5.0 + (slices ? 2.0 * S : 0.0)) * B * L);
  hipLaunchKernelGGL(gauss_latent_fwd_kernel, dim3((B * L / 4 + 255) / 256), dim3(256), 0, st, heads, eps_in, rng, eps_out, z, B, L,
                     slices, S, bias);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

int launch_gauss_latent_bwd(const float* g_mu, const float* g_lv, const float* g_z, const float* heads, const float* eps,
                            float* g_heads, unsigned long long* rng_bump, int B, int L, hipStream_t st, int gz_slices) {
  if (!heads || !eps || !g_heads || B <= 0 || L <= 0 || L % 4 || (gz_slices > 0 && !g_z)) return kErrBadArg;
  ProfScope ps("gauss_latent_bwd_kernel", st, 0.0, 4.0 * (7.0 + (gz_slices > 1 ? gz_slices - 1.0 : 0.0)) * B * L);
  hipLaunchKernelGGL(gauss_latent_bwd_kernel, dim3((B * L / 4 + 255) / 256), dim3(256), 0, st, g_mu, g_lv, g_z, heads, eps, g_heads,
                     rng_bump, B, L, gz_slices);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

// out[b][c][p] (NCHW) = sum_s slices[s][(b*P + p)*C + c]: the split-K finish of a data gradient written NHWC and the
// NHWC -> NCHW layout change behind it (decoder.0's data gradient in front of decoder_input, vanilla_vae.py:102) as one launch.
// Tiny tensors ([B,512,2,2]): thread = one output element, reads along c are strided by design.
__global__ __launch_bounds__(256) void splitk_permute_kernel(const float* __restrict__ slices, int S, float* __restrict__ out, int B,
                                                            int C, int P) {
  const long n = (long)B * C * P, i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int p = (int)(i % P), c = (int)((i / P) % C), b = (int)(i / ((long)P * C));
  const long src = ((long)b * P + p) * C + c;
  float v = slices[src];
  for (int s = 1; s < S; ++s) v += slices[(long)s * n + src];
  out[i] = v;
}

int launch_splitk_permute(const float* slices, int S, float* out, int B, int C, int P, hipStream_t st) {
  if (!slices || !out || S < 1 || B <= 0 || C <= 0 || P <= 0) return kErrBadArg;
  const long n = (long)B * C * P;
  ProfScope ps("splitk_permute_kernel", st, 0.0, 4.0 * (S + 1.0) * n);
  hipLaunchKernelGGL(splitk_permute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slices, S, out, B, C, P);
  CTVAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace ctvae
