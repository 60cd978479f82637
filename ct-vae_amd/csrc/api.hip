// extern "C" entry points of libctvae_hip.so (see include/ctvae_hip.h).  Thin argument checks + dispatch
// into the kernel launchers; nothing here allocates or synchronises.
#include "../../include/ctvae_hip.h"

#include "common.hpp"
#include "convpaths.hpp"
#include "gatlayer.hpp"
#include "glinear.hpp"
#include "ops.hpp"
#include "pair.hpp"

using namespace ctvae;

// `kind` of the conv entry points: CTVAE_CONV / CTVAE_CONVT, for CTVAE_CONV optionally | CTVAE_W_CI_TAP (weights stored
// [Ci][tap][Co]: the block of a Linear layer over torch.flatten(NCHW), run as a k x k convolution on the NHWC tensor)
static bool conv_kind_ok(int kind) {
  const int base = kind & ~CTVAE_W_CI_TAP;
  return base == CTVAE_CONV || (base == CTVAE_CONVT && !(kind & CTVAE_W_CI_TAP));
}
// gkind0: 0 for the forward / weight-gradient geometry, 2 for the data gradient's
static int conv_geom(ConvGeom& g, int kind, int gkind0, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad) {
  const int rc = build_geom(g, gkind0 + ((kind & ~CTVAE_W_CI_TAP) == CTVAE_CONV ? 0 : 1), B, H, W, Ci, Co, k, stride, pad, out_pad);
  if (rc) return rc;
  if (kind & CTVAE_W_CI_TAP) {
    g.wts = Co;
    g.wrs = k * k * Co;
  }
  return 0;
}

extern "C" {

const char* ctvae_version(void) { return "0.1.0"; }
const char* ctvae_arch(void) { return "gfx950"; }

const char* ctvae_error_string(int code) {
  if (code == 0) return "success";
  if (code == kErrBadArg) return "ctvae: unsupported shape or bad argument";
  if (code == kErrWorkspace) return "ctvae: workspace too small";
  if (code > 0) return hipGetErrorString((hipError_t)code);
  return "ctvae: unknown error";
}

int ctvae_crop_resize_u8(const uint8_t* images, const int64_t* rows, float* out, int B, int N, int H, int W, int crop, int size,
                         void* stream) {
  if (!images || !rows || !out) return kErrBadArg;
  return launch_crop_resize_u8(images, (const long long*)rows, out, B, N, H, W, crop, size, (hipStream_t)stream);
}

int ctvae_winograd_enable(int on) { return wino_set_enabled(on); }

size_t ctvae_workspace_bytes(void) { return (size_t)256 << 20; }

int ctvae_conv_forward(int kind, const float* x, const float* w, const float* bias, const float* add, float* y, int B,
                       int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int act, const float* in_scale,
                       const float* in_shift, int in_act, float* wino_dgrad_filters_out, const float* wino_fwd_filters, float* ws,
                       size_t ws_bytes, void* stream) {
  if (!x || !w || !y || !conv_kind_ok(kind)) return kErrBadArg;
  if ((in_scale != nullptr) != (in_shift != nullptr)) return kErrBadArg;
  // the transform on load exists where the header says so and nowhere else: a shape whose weight gradient (or whose Winograd
  // forward) cannot apply it is refused here, not run by whichever kernel happens to take the operand
  if (in_scale != nullptr && !ctvae_conv_input_transform_supported(kind, B, H, W, Ci, Co, k, stride, pad, out_pad)) return kErrBadArg;
  ConvGeom g;
  if (conv_geom(g, kind, 0, B, H, W, Ci, Co, k, stride, pad, out_pad)) return kErrBadArg;
  if ((wino_dgrad_filters_out != nullptr || wino_fwd_filters != nullptr) &&
      !ctvae_conv_wino_filter_floats(kind, B, H, W, Ci, Co, k, stride, pad, out_pad, ws_bytes))
    return kErrBadArg;
  const InXform xf{in_scale, in_shift, in_act};
  // wino_fwd_filters: both filter sets were made ahead of time (ctvae_wino_filters_batch): no transform launch here
  const WinoFilters wf{wino_fwd_filters, wino_fwd_filters != nullptr ? nullptr : wino_dgrad_filters_out};
  return launch_tapgemm(g, x, w, bias, add, nullptr, 0, y, act, nullptr, ws, ws_bytes / sizeof(float), (hipStream_t)stream,
                        nullptr, &xf, &wf);
}

int ctvae_linear_pixmajor_supported(int B, int Ci, int C, int P, size_t ws_bytes) {
  ConvGeom g;
  if (B <= 0 || Ci <= 0 || C <= 0 || P <= 1 || conv_geom(g, CTVAE_CONV, 0, B, 1, 1, Ci, C * P, 1, 1, 0, 0)) return 0;
  return out_pix_supported(g, ws_bytes / sizeof(float), P) ? 1 : 0;
}

int ctvae_linear_pixmajor_forward(const float* x, const float* w, const float* bias, float* y, int B, int Ci, int C, int P, int act,
                                  float* ws, size_t ws_bytes, void* stream) {
  if (!x || !w || !y || !ctvae_linear_pixmajor_supported(B, Ci, C, P, ws_bytes)) return kErrBadArg;
  ConvGeom g;
  if (conv_geom(g, CTVAE_CONV, 0, B, 1, 1, Ci, C * P, 1, 1, 0, 0)) return kErrBadArg;
  return launch_tapgemm(g, x, w, bias, nullptr, nullptr, 0, y, act, nullptr, ws, ws_bytes / sizeof(float), (hipStream_t)stream,
                        nullptr, nullptr, nullptr, nullptr, P);
}

int ctvae_wino_filters_batch(int n, const float* const* w, float* const* fwd_filters, float* const* dgrad_filters, const int* Ci,
                             const int* Co, void* stream) {
  return launch_wino_filters_batch(n, w, fwd_filters, dgrad_filters, Ci, Co, (hipStream_t)stream);
}

size_t ctvae_conv_wino_filter_floats(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                     size_t ws_bytes) {
  if (kind != CTVAE_CONV || !wino_enabled()) return 0;
  ConvGeom gf, gb;
  if (build_geom(gf, 0, B, H, W, Ci, Co, k, stride, pad, out_pad) || build_geom(gb, 2, B, H, W, Ci, Co, k, stride, pad, out_pad))
    return 0;
  const size_t wsf = ws_bytes / sizeof(float);
  return (wino_supported(gf, wsf) && wino_supported(gb, wsf)) ? (size_t)16 * Ci * Co : 0;
}

int ctvae_conv_input_transform_supported(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad,
                                         int out_pad) {
  if (!conv_kind_ok(kind)) return 0;
  ConvGeom g;
  if (conv_geom(g, kind, 0, B, H, W, Ci, Co, k, stride, pad, out_pad)) return 0;
  if (thin_forward_supported(g) && thin_wgrad_supported(g)) return 1;
  // the general tile kernels: forward on the vector path (not one of the dedicated picture-side / transposed-conv kernels, not
  // Winograd) and the weight gradient on the lean 64 x 64 kernel -- both form act(BN(.)) between the global load and the LDS store
  if (upconv_wgrad_supported(g)) return 1;     // 32 -> 32 transposed conv: both kernels stage the input patch once per tile
  if (img_enc_supported(g) || img_conv_supported(g)) return 0;
  if (wino_enabled() && wino_supported(g, (size_t)1 << 26)) return 0;
  TapGemmPlan pl;
  tapgemm_plan(g, (size_t)1 << 26, pl, false);
  if (pl.thin || pl.BM == 0) return 0;
  return ((g.gC % KC) == 0 && (g.sC % 4) == 0 && g.wT == 0) ? 1 : 0;
}

int ctvae_conv_bn_act_apply_is_separate(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                        size_t ws_bytes) {
  if (!conv_kind_ok(kind)) return 0;
  ConvGeom g;
  if (conv_geom(g, kind, 0, B, H, W, Ci, Co, k, stride, pad, out_pad)) return 0;
  TapGemmPlan plan;
  tapgemm_plan(g, ws_bytes / sizeof(float), plan, false);
  return (plan.splitk > 1 && bn_fused_ok(g.B * g.sH * g.sW, Co)) ? 0 : 1;   // 0: the channel-owner launch writes a anyway
}

int ctvae_conv_bn_act_forward(int kind, const float* x, const float* w, const float* bias, const float* gamma,
                              const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                              int training, int act, float* y, float* a_out, float* save_mean, float* save_invstd,
                              float* scale_shift_out, int64_t* num_batches_tracked, int B, int H, int W, int Ci, int Co, int k,
                              int stride, int pad, int out_pad, const float* in_scale, const float* in_shift, int in_act,
                              float* ws, size_t ws_bytes, void* stream) {
  long long* nbt = (long long*)num_batches_tracked;
  if (!x || !w || !gamma || !beta || !y || !ws || !conv_kind_ok(kind)) return kErrBadArg;
  if ((in_scale != nullptr) != (in_shift != nullptr)) return kErrBadArg;
  if (in_scale != nullptr && !ctvae_conv_input_transform_supported(kind, B, H, W, Ci, Co, k, stride, pad, out_pad)) return kErrBadArg;
  const InXform xf{in_scale, in_shift, in_act};
  const InXform* xfp = in_scale != nullptr ? &xf : nullptr;
  if (!a_out && !scale_shift_out) return kErrBadArg;   // either materialise a or hand out the coefficients
  if (training && (!save_mean || !save_invstd)) return kErrBadArg;
  if (!training && (!running_mean || !running_var)) return kErrBadArg;
  if (Co % 4 != 0) return kErrBadArg;
  ConvGeom g;
  if (conv_geom(g, kind, 0, B, H, W, Ci, Co, k, stride, pad, out_pad)) return kErrBadArg;
  const size_t wsf = ws_bytes / sizeof(float);
  TapGemmPlan plan;
  tapgemm_plan(g, wsf, plan, false);
  const int R = g.B * g.sH * g.sW;
  if (plan.splitk > 1 || !training) {
    // small layer run split-K (or eval mode).  Training, a few MB at most: the slices stay channel-major in the workspace and ONE
    // channel-owner launch sums them, takes the statistics, finalizes and applies (bn.hip bn_fused_fwd_kernel).  Otherwise:
    // conv (+ split-K finish) first, then statistics from y with the stand-alone kernels
    SplitKRaw raw{ws, 0};
    const bool fused = training && plan.splitk > 1 && bn_fused_ok(R, Co);
    int rc = launch_tapgemm(g, x, w, bias, nullptr, nullptr, 0, y, ACT_NONE, nullptr, ws, wsf, (hipStream_t)stream, nullptr, xfp,
                            nullptr, fused ? &raw : nullptr);
    if (rc) return rc;
    if (raw.splitk > 1) {
      const BnFusedFwd p{ws, row_map_of(g), raw.splitk, R, Co, bias, gamma, beta, running_mean, running_var, momentum, eps, save_mean, save_invstd,
                         scale_shift_out, nbt, y, a_out, act};
      return launch_bn_fused_forward(p, (hipStream_t)stream);
    }
    return launch_bn_forward(y, R, Co, gamma, beta, running_mean, running_var, momentum, eps, training, act, a_out, save_mean,
                             save_invstd, ws, ws_bytes, nbt, (hipStream_t)stream, scale_shift_out);
  }
  const int nparts = plan.bn_parts;
  if (wsf < bn_workspace_floats(Co, nparts)) return kErrWorkspace;
  int rc = launch_tapgemm(g, x, w, bias, nullptr, nullptr, 0, y, ACT_NONE, ws, nullptr, 0, (hipStream_t)stream, nullptr, xfp);
  if (rc) return rc;
  return launch_bn_finish_forward(y, R, Co, nparts, gamma, beta, running_mean, running_var, momentum, eps, training, act,
                                  a_out, save_mean, save_invstd, ws, nbt, (hipStream_t)stream, scale_shift_out);
}

int ctvae_conv_dgrad(int kind, const float* dy, const float* w, const float* add, const float* mask, int mask_act,
                     float* dx, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                     const float* wino_filters, float* ws, size_t ws_bytes, void* stream) {
  if (!dy || !w || !dx || !conv_kind_ok(kind)) return kErrBadArg;
  ConvGeom g;
  if (conv_geom(g, kind, 2, B, H, W, Ci, Co, k, stride, pad, out_pad)) return kErrBadArg;
  if (wino_filters != nullptr && !ctvae_conv_wino_filter_floats(kind, B, H, W, Ci, Co, k, stride, pad, out_pad, ws_bytes))
    return kErrBadArg;
  const WinoFilters wf{wino_filters, nullptr};
  return launch_tapgemm(g, dy, w, nullptr, add, mask, mask_act, dx, ACT_NONE, nullptr, ws, ws_bytes / sizeof(float),
                        (hipStream_t)stream, nullptr, nullptr, &wf);
}

int ctvae_conv_wgrad(int kind, const float* x, const float* dy, float* dw, float* dbias, int B, int H, int W, int Ci,
                     int Co, int k, int stride, int pad, int out_pad, int accumulate, const float* in_scale,
                     const float* in_shift, int in_act, const float* dy_bn_y, const float* dy_bn_coef, int dy_bn_act,
                     float* gy_out, float* bn_dgamma, float* bn_dbeta, int bn_accumulate, float* ws, size_t ws_bytes,
                     void* stream) {
  if (!x || !dy || !dw || !ws || !conv_kind_ok(kind)) return kErrBadArg;
  if ((in_scale != nullptr) != (in_shift != nullptr)) return kErrBadArg;
  if ((dy_bn_y != nullptr) != (dy_bn_coef != nullptr) || (gy_out != nullptr && dy_bn_y == nullptr)) return kErrBadArg;
  if ((bn_dgamma != nullptr) != (bn_dbeta != nullptr) || (bn_dgamma != nullptr && (dy_bn_y == nullptr || gy_out != nullptr)))
    return kErrBadArg;
  ConvGeom g;
  if (conv_geom(g, kind, 0, B, H, W, Ci, Co, k, stride, pad, out_pad)) return kErrBadArg;
  const InXform xf{in_scale, in_shift, in_act};
  const DyXform dyx{dy_bn_y, dy_bn_coef, gy_out, dy_bn_act, bn_dgamma, bn_dbeta, bn_accumulate};
  float* wws = defer_wgrad_ws(ws, ws_bytes / sizeof(float));   // between ctvae_defer_begin / _flush: slabs into the arena
  const int rc = launch_wgrad(g, x, dy, dw, dbias, wws, ws_bytes, accumulate, (hipStream_t)stream, &xf, &dyx);
  defer_wgrad_done();
  return rc;
}

int ctvae_defer_begin(float* arena, size_t arena_bytes) { return defer_begin(arena, arena_bytes / sizeof(float)); }
int ctvae_defer_flush(void* stream) { return defer_flush((hipStream_t)stream); }

int ctvae_conv_backward_bn_rows(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                size_t ws_bytes) {
  if (!conv_kind_ok(kind)) return 0;
  ConvGeom g;
  if (conv_geom(g, kind, 2, B, H, W, Ci, Co, k, stride, pad, out_pad)) return 0;
  return tapgemm_bnb_rows(g, ((ws_bytes / 2) & ~(size_t)255) / sizeof(float), true);   // plan as ctvae_conv_backward does
}

// the picture-side conv behind the transposed conv of geometry g1 (kind 0): its data-gradient taps for the recompute mode
static bool recompute_geom(const ConvGeom& g1, int kind2, int Co2, int k2, int stride2, int pad2, int out_pad2, DyRecompute* rc) {
  if (!upconv_wgrad_supported(g1) || !conv_kind_ok(kind2)) return false;
  ConvGeom g2;
  if (conv_geom(g2, kind2, 2, g1.B, g1.sH, g1.sW, g1.sC, Co2, k2, stride2, pad2, out_pad2)) return false;
  if (!img_dgrad_supported(g2) || g2.B != g1.B || g2.sH != g1.sH || g2.sW != g1.sW) return false;
  if (rc != nullptr)
    for (int t = 0; t < 9; ++t) { rc->tdy[t] = g2.taps[0][t].dy; rc->tdx[t] = g2.taps[0][t].dx; rc->twt[t] = g2.taps[0][t].wtap; }
  return true;
}

// One paired backward call.  The five ctvae_conv_backward* entry points fill in what they have; the rest stays null / 0
struct ConvShape {
  int kind, B, H, W, Ci, Co, k, stride, pad, out_pad;
};
struct ConvBackwardCall {
  ConvShape s;
  const float *x, *dy, *w;      // dy is absent (null) with dyx.rc: formed in the kernel
  float *dw, *dbias, *dx;
  int accumulate;
  const float* mask;
  int mask_act;
  const float* wino_filters;
  BnBwdFuse bn;                 // bn.part != nullptr: the data gradient emits the backward sums of the BatchNorm below
  int bn_part_rows;
  float* bn_coef_out;           // that BatchNorm's finalize rides in the finishing launch,
  float *bn_dgamma, *bn_dbeta;  // and commits its parameter gradients
  int bn_accumulate;
  InXform in;
  DyXform dyx;                  // dyx.rc: ctvae_conv_backward_recompute
  float* ws;
  size_t ws_bytes;
  bool no_dx;                   // ctvae_conv_backward_nodx: the picture-side conv's g_a is not written
  float* dx_slices;             // ctvae_conv_backward_lazy: the data gradient must run split-K and leaves its raw slices here
  int slices_pixel_major;       // (SplitKRaw), channel-major or pixel-major; dx is not written
};

static int conv_backward_impl(const ConvBackwardCall& c, hipStream_t st) {
  const ConvShape& s = c.s;
  const BnBwdFuse& f = c.bn;
  const DyRecompute* const recompute = c.dyx.rc;
  if (!c.x || (!c.dy && !recompute) || !c.w || !c.dw || (!c.dx && !c.dx_slices && !c.no_dx) || !c.ws || !conv_kind_ok(s.kind))
    return kErrBadArg;
  if (recompute != nullptr && (c.dyx.y == nullptr || c.dyx.gy_out == nullptr)) return kErrBadArg;
  const bool bn = f.part != nullptr;
  if (c.bn_coef_out != nullptr && !bn) return kErrBadArg;
  if ((c.bn_dgamma != nullptr) != (c.bn_dbeta != nullptr) || (c.bn_dgamma != nullptr && c.bn_coef_out == nullptr)) return kErrBadArg;
  if ((c.in.scale != nullptr) != (c.in.shift != nullptr)) return kErrBadArg;
  if ((c.dyx.y != nullptr) != (c.dyx.coef != nullptr) || (c.dyx.y != nullptr) != (c.dyx.gy_out != nullptr)) return kErrBadArg;
  if (bn && (!f.y || !f.mean || !f.invstd || !f.gamma || !f.beta)) return kErrBadArg;
  ConvGeom gw, gd;
  if (conv_geom(gw, s.kind, 0, s.B, s.H, s.W, s.Ci, s.Co, s.k, s.stride, s.pad, s.out_pad)) return kErrBadArg;
  if (conv_geom(gd, s.kind, 2, s.B, s.H, s.W, s.Ci, s.Co, s.k, s.stride, s.pad, s.out_pad)) return kErrBadArg;
  // the two GEMMs run concurrently: each gets its own half of the workspace
  const size_t half_bytes = (c.ws_bytes / 2) & ~(size_t)255, half_floats = half_bytes / sizeof(float);
  float* ws_d = c.ws + half_floats;
  if (c.wino_filters != nullptr &&
      !ctvae_conv_wino_filter_floats(s.kind, s.B, s.H, s.W, s.Ci, s.Co, s.k, s.stride, s.pad, s.out_pad, half_bytes))
    return kErrBadArg;
  if (bn) {
    const int rows = tapgemm_bnb_rows(gd, half_floats, true);
    if (rows <= 0 || rows != c.bn_part_rows || (img_dgrad_supported(gd) && c.mask != nullptr)) return kErrBadArg;
  }
  PairCtx ctx;
  {   // how much of the chip the data gradient fills on its own: the weight gradient that shares its launch is sized to match
    TapGemmPlan pl;
    tapgemm_plan(gd, half_floats, pl, true);
    ctx.dgrad_wgs = (long)pl.mtiles * pl.ntiles * gd.ncls * (pl.splitk > 1 ? pl.splitk : 1);
    int kmax = 0;
    for (int cl = 0; cl < gd.ncls; ++cl) kmax = gd.ntaps[cl] * gd.gC / KC > kmax ? gd.ntaps[cl] * gd.gC / KC : kmax;
    ctx.dgrad_chunks = pl.splitk > 1 ? (kmax + pl.splitk - 1) / pl.splitk : kmax;
  }
  int rc;
  const bool img_fused = bn && f.act != ACT_TANH && c.x == f.y && c.in.scale != nullptr && c.in.act == f.act && c.mask == nullptr &&
                         c.dyx.y == nullptr && img_conv_supported(gw) && img_dgrad_supported(gd) &&
                         img_backward_fused_ws_floats(gd) <= half_floats;
  // only the kernels that can do without
  if ((c.no_dx && !img_fused) || (recompute != nullptr && !upconv_wgrad_supported(gw))) return kErrBadArg;
  if (img_fused) {
    // picture-side conv behind BatchNorm + activation (final_layer.1-3): the data gradient's pass over y also forms the
    // weight gradient (image.hip img_bwd_fused_kernel) -- x of the weight gradient is act(BN(y)), which that pass computes
    float *part = nullptr, *pb = nullptr;
    int np = 0;
    rc = launch_img_backward_fused(gd, c.dy, c.w, c.dx, &f, c.ws, &part, &pb, &np, c.dbias != nullptr, st);
    if (!rc) rc = wgrad_finish_slabs(part, c.dw, 9L * 32 * 3, np, pb, c.dbias, 3L, c.accumulate, st, &ctx);
  } else {
    // (a finishing launch that carries the BatchNorm finalize of the layer below stays in the chain, without the reduction:
    // deferring it too measured 1.615 vs 1.611 ms, VanillaVAE)
    float* wws = c.bn_coef_out == nullptr ? defer_wgrad_ws(c.ws, half_floats) : c.ws;
    rc = launch_wgrad(gw, c.x, c.dy, c.dw, c.dbias, wws, half_bytes, c.accumulate, st, &c.in, &c.dyx, &ctx);
    defer_wgrad_done();
    if (!rc) {
      const WinoFilters wf{c.wino_filters, nullptr};
      // dyx: dy was g_a of the BatchNorm behind this layer; the weight-gradient kernel left g_y in gy_out for the data gradient
      SplitKRaw raw{c.dx_slices, 0, c.slices_pixel_major};
      rc = launch_tapgemm(gd, c.dyx.gy_out != nullptr ? c.dyx.gy_out : c.dy, c.w, nullptr, nullptr, c.mask, c.mask_act, c.dx, ACT_NONE,
                          nullptr, ws_d, half_floats, st, bn ? &f : nullptr, nullptr, &wf, c.dx_slices != nullptr ? &raw : nullptr, 0,
                          &ctx);
      if (!rc && c.dx_slices != nullptr && raw.splitk <= 1) rc = kErrBadArg;   // the caller asked ctvae_conv_backward_lazy_slices first
    }
  }
  if (rc) return rc;
  if (c.bn_coef_out != nullptr) {   // the finalize of the BatchNorm below rides in the finishing launch
    ctx.haveBF = true;
    ctx.bf = BnFinJob{f.part, c.bn_part_rows, s.Ci, (float)((long)s.B * s.H * s.W), f.gamma, f.mean, f.invstd, f.beta, c.bn_coef_out,
                      c.bn_dgamma, c.bn_dbeta, c.bn_accumulate};
  }
  return pair_flush(ctx, st);
}

int ctvae_conv_backward(int kind, const float* x, const float* dy, const float* w, float* dw, float* dbias, float* dx, int B,
                        int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int accumulate, const float* mask,
                        int mask_act, const float* wino_filters, const float* bn_y, const float* bn_mean,
                        const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_act, float* bn_part,
                        int bn_part_rows, float* bn_coef_out, float* bn_dgamma, float* bn_dbeta, int bn_accumulate,
                        const float* in_scale, const float* in_shift, int in_act,
                        const float* dy_bn_y, const float* dy_bn_coef, int dy_bn_act, float* gy_out, float* ws, size_t ws_bytes,
                        void* stream) {
  ConvBackwardCall c{};
  c.s = ConvShape{kind, B, H, W, Ci, Co, k, stride, pad, out_pad};
  c.x = x; c.dy = dy; c.w = w; c.dw = dw; c.dbias = dbias; c.dx = dx; c.accumulate = accumulate;
  c.mask = mask; c.mask_act = mask_act; c.wino_filters = wino_filters;
  c.bn = BnBwdFuse{bn_y, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_act, bn_part};
  c.bn_part_rows = bn_part_rows; c.bn_coef_out = bn_coef_out;
  c.bn_dgamma = bn_dgamma; c.bn_dbeta = bn_dbeta; c.bn_accumulate = bn_accumulate;
  c.in = InXform{in_scale, in_shift, in_act};
  c.dyx = DyXform{dy_bn_y, dy_bn_coef, gy_out, dy_bn_act};
  c.ws = ws; c.ws_bytes = ws_bytes;
  return conv_backward_impl(c, (hipStream_t)stream);
}

int ctvae_conv_backward_nodx(int kind, const float* x, const float* dy, const float* w, float* dw, float* dbias, int B, int H,
                             int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int accumulate, const float* bn_y,
                             const float* bn_mean, const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_act,
                             float* bn_part, int bn_part_rows, float* bn_coef_out, float* bn_dgamma, float* bn_dbeta,
                             int bn_accumulate, const float* in_scale, const float* in_shift, int in_act, float* ws, size_t ws_bytes,
                             void* stream) {
  ConvBackwardCall c{};
  c.s = ConvShape{kind, B, H, W, Ci, Co, k, stride, pad, out_pad};
  c.x = x; c.dy = dy; c.w = w; c.dw = dw; c.dbias = dbias; c.accumulate = accumulate;
  c.bn = BnBwdFuse{bn_y, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_act, bn_part};
  c.bn_part_rows = bn_part_rows; c.bn_coef_out = bn_coef_out;
  c.bn_dgamma = bn_dgamma; c.bn_dbeta = bn_dbeta; c.bn_accumulate = bn_accumulate;
  c.in = InXform{in_scale, in_shift, in_act};
  c.ws = ws; c.ws_bytes = ws_bytes;
  c.no_dx = true;
  return conv_backward_impl(c, (hipStream_t)stream);
}

int ctvae_conv_recompute_supported(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int kind2,
                                   int Co2, int k2, int stride2, int pad2, int out_pad2) {
  if (!conv_kind_ok(kind)) return 0;
  ConvGeom g;
  if (conv_geom(g, kind, 0, B, H, W, Ci, Co, k, stride, pad, out_pad)) return 0;
  return recompute_geom(g, kind2, Co2, k2, stride2, pad2, out_pad2, nullptr) ? 1 : 0;
}

int ctvae_conv_backward_recompute(int kind, const float* x, const float* g_pre, const float* w2, const float* w, float* dw,
                                  float* dbias, float* dx, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                  int accumulate, const float* bn_y, const float* bn_mean, const float* bn_invstd,
                                  const float* bn_gamma, const float* bn_beta, int bn_act, float* bn_part, int bn_part_rows,
                                  float* bn_coef_out, float* bn_dgamma, float* bn_dbeta, int bn_accumulate, const float* in_scale,
                                  const float* in_shift, int in_act, const float* dy_bn_y, const float* dy_bn_coef, int dy_bn_act,
                                  float* gy_out, int kind2, int Co2, int k2, int stride2, int pad2, int out_pad2, float* ws,
                                  size_t ws_bytes, void* stream) {
  if (!g_pre || !w2 || !dx || !dy_bn_y || !dy_bn_coef || !gy_out || !conv_kind_ok(kind)) return kErrBadArg;
  ConvGeom g;
  DyRecompute rc{g_pre, w2, {}, {}, {}};
  if (conv_geom(g, kind, 0, B, H, W, Ci, Co, k, stride, pad, out_pad)) return kErrBadArg;
  if (!recompute_geom(g, kind2, Co2, k2, stride2, pad2, out_pad2, &rc)) return kErrBadArg;
  ConvBackwardCall c{};
  c.s = ConvShape{kind, B, H, W, Ci, Co, k, stride, pad, out_pad};
  c.x = x; c.w = w; c.dw = dw; c.dbias = dbias; c.dx = dx; c.accumulate = accumulate;
  c.bn = BnBwdFuse{bn_y, bn_mean, bn_invstd, bn_gamma, bn_beta, bn_act, bn_part};
  c.bn_part_rows = bn_part_rows; c.bn_coef_out = bn_coef_out;
  c.bn_dgamma = bn_dgamma; c.bn_dbeta = bn_dbeta; c.bn_accumulate = bn_accumulate;
  c.in = InXform{in_scale, in_shift, in_act};
  c.dyx = DyXform{dy_bn_y, dy_bn_coef, gy_out, dy_bn_act};
  c.dyx.rc = &rc;
  c.ws = ws; c.ws_bytes = ws_bytes;
  return conv_backward_impl(c, (hipStream_t)stream);
}

int ctvae_conv_wgrad_recompute(int kind, const float* x, const float* g_pre, const float* w2, float* dw, float* dbias, int B, int H,
                               int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int accumulate, const float* in_scale,
                               const float* in_shift, int in_act, const float* dy_bn_y, const float* dy_bn_coef, int dy_bn_act,
                               float* gy_out, int kind2, int Co2, int k2, int stride2, int pad2, int out_pad2, float* ws,
                               size_t ws_bytes, void* stream) {
  if (!x || !g_pre || !w2 || !dw || !ws || !dy_bn_y || !dy_bn_coef || !gy_out || !conv_kind_ok(kind)) return kErrBadArg;
  if ((in_scale != nullptr) != (in_shift != nullptr)) return kErrBadArg;
  ConvGeom g;
  DyRecompute rc{g_pre, w2, {}, {}, {}};
  if (conv_geom(g, kind, 0, B, H, W, Ci, Co, k, stride, pad, out_pad)) return kErrBadArg;
  if (!recompute_geom(g, kind2, Co2, k2, stride2, pad2, out_pad2, &rc)) return kErrBadArg;
  const InXform xf{in_scale, in_shift, in_act};
  DyXform dyx{dy_bn_y, dy_bn_coef, gy_out, dy_bn_act};
  dyx.rc = &rc;
  float* wws = defer_wgrad_ws(ws, ws_bytes / sizeof(float));
  const int rcode = launch_wgrad(g, x, nullptr, dw, dbias, wws, ws_bytes, accumulate, (hipStream_t)stream, &xf, &dyx);
  defer_wgrad_done();
  return rcode;
}

int ctvae_conv_backward_lazy_slices(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                    int for_bn, size_t ws_bytes) {
  if (!conv_kind_ok(kind)) return 0;
  ConvGeom g;
  if (conv_geom(g, kind, 2, B, H, W, Ci, Co, k, stride, pad, out_pad)) return 0;
  const size_t half_floats = ((ws_bytes / 2) & ~(size_t)255) / sizeof(float);
  if (img_dgrad_supported(g) || (wino_enabled() && wino_supported(g, half_floats))) return 0;
  TapGemmPlan pl;
  tapgemm_plan(g, half_floats, pl, true);   // plan as ctvae_conv_backward does
  const long Mc = (long)g.B * g.Qh * g.Qw;
  if (pl.thin || pl.splitk <= 1) return 0;
  if (for_bn && (Mc % 4 != 0 || !bn_fused_ok(B * H * W, Ci))) return 0;   // channel-major slices for the BatchNorm's channel owners
  return pl.splitk;
}

int ctvae_conv_backward_lazy(int kind, const float* x, const float* dy, const float* w, float* dw, float* dbias, float* dx_slices,
                             int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int accumulate,
                             const float* in_scale, const float* in_shift, int in_act, int pixel_major, float* ws, size_t ws_bytes,
                             void* stream) {
  if (!dx_slices) return kErrBadArg;
  ConvBackwardCall c{};
  c.s = ConvShape{kind, B, H, W, Ci, Co, k, stride, pad, out_pad};
  c.x = x; c.dy = dy; c.w = w; c.dw = dw; c.dbias = dbias; c.accumulate = accumulate;
  c.in = InXform{in_scale, in_shift, in_act};
  c.ws = ws; c.ws_bytes = ws_bytes;
  c.dx_slices = dx_slices; c.slices_pixel_major = pixel_major;
  return conv_backward_impl(c, (hipStream_t)stream);
}

int ctvae_bn_backward_fused(const float* g_a_slices, int slices, int kind, int B, int H, int W, int Ci, int Co, int k, int stride,
                            int pad, int out_pad, const float* y, const float* gamma, const float* beta, const float* save_mean,
                            const float* save_invstd, int act, float* g_y, float* dgamma, float* dbeta, int accumulate, void* stream) {
  if (!g_a_slices || slices < 1 || !y || !gamma || !beta || !save_mean || !save_invstd || !g_y || !dgamma || !dbeta) return kErrBadArg;
  if (!conv_kind_ok(kind)) return kErrBadArg;
  ConvGeom g;   // the data gradient that wrote the slices: its class-major row order -> pixels of y
  if (conv_geom(g, kind, 2, B, H, W, Ci, Co, k, stride, pad, out_pad)) return kErrBadArg;
  const BnFusedBwd p{g_a_slices, row_map_of(g), slices, B * H * W, Ci, y, gamma, beta, save_mean, save_invstd, act, g_y, dgamma,
                     dbeta, accumulate};
  return launch_bn_fused_backward(p, (hipStream_t)stream);
}

int ctvae_conv_wgrad_bn_apply_supported(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad) {
  if (!conv_kind_ok(kind)) return 0;
  ConvGeom g;
  if (conv_geom(g, kind, 0, B, H, W, Ci, Co, k, stride, pad, out_pad)) return 0;
  if (upconv_wgrad_supported(g)) return 1;
  return img_enc_supported(g) ? 2 : 0;
}

int ctvae_bn_forward(const float* y, int R, int C, const float* gamma, const float* beta, float* running_mean,
                     float* running_var, float momentum, float eps, int training, int act, float* out,
                     float* save_mean, float* save_invstd, int64_t* num_batches_tracked, float* ws, size_t ws_bytes,
                     void* stream) {
  if (!y || !gamma || !beta || !out || !ws) return kErrBadArg;
  if (training && (!save_mean || !save_invstd)) return kErrBadArg;
  if (!training && (!running_mean || !running_var)) return kErrBadArg;
  return launch_bn_forward(y, R, C, gamma, beta, running_mean, running_var, momentum, eps, training, act, out, save_mean,
                           save_invstd, ws, ws_bytes, (long long*)num_batches_tracked, (hipStream_t)stream);
}

int ctvae_bn_backward(const float* g_a, const float* beta, const float* y, int R, int C, const float* gamma,
                      const float* save_mean, const float* save_invstd, int act, float* g_y, float* dgamma,
                      float* dbeta, int accumulate, const float* part_in, int part_rows, float* coef_out,
                      const float* coef_in, float* ws, size_t ws_bytes, void* stream) {
  if (!g_a || !beta || !y || !gamma || !save_mean || !save_invstd || !dgamma || !dbeta || !ws) return kErrBadArg;
  if (!g_y && !coef_out) return kErrBadArg;   // either apply here or hand the coefficients to the consumer
  if ((part_in != nullptr) != (part_rows > 0)) return kErrBadArg;
  if (coef_in != nullptr && (!g_y || part_in != nullptr || coef_out != nullptr)) return kErrBadArg;
  return launch_bn_backward(g_a, beta, y, R, C, gamma, save_mean, save_invstd, act, g_y, dgamma, dbeta, accumulate, ws,
                            ws_bytes, part_in, part_rows, (hipStream_t)stream, coef_out, coef_in);
}

int ctvae_gat_score(int mode, const float* xl, const float* xr, const float* attr, const float* we, const float* att, float* out,
                    int B, int N, int H, int C, float slope, void* stream) {
  if (!xl || !xr || !attr || !we || !att || !out || (mode != 0 && mode != 1)) return kErrBadArg;
  return launch_gat_score(mode, xl, xr, attr, we, att, out, B, N, H, C, slope, (hipStream_t)stream);
}

int ctvae_gat_score_backward(const float* xl, const float* xr, const float* attr, const float* we, const float* att,
                             const float* g, float* d_xl, float* d_xr, float* d_att_part, float* d_we_part, int B, int N, int H,
                             int C, float slope, void* stream) {
  if (!xl || !xr || !attr || !we || !att || !g || !d_xl || !d_xr || !d_att_part || !d_we_part) return kErrBadArg;
  return launch_gat_score_backward(xl, xr, attr, we, att, g, d_xl, d_xr, d_att_part, d_we_part, B, N, H, C, slope,
                                   (hipStream_t)stream);
}

int ctvae_gat_layer_forward(const float* xl, const float* xr, int ld, const float* adj, const float* we, const float* att,
                            const float* bias, const int32_t* head_map, float* out, int ldo, float* alpha, int B, int Hs, int C,
                            float slope, int act, void* stream) {
  const GatLayerArgs a{xl, xr, ld, adj, we, att, bias, head_map, out, ldo, alpha, B, Hs, C, slope, act};
  return launch_gat_layer_forward(a, (hipStream_t)stream);
}

int ctvae_gat_layer_backward(const float* xl, const float* xr, int ld, const float* adj, const float* we, const float* att,
                             const float* bias, const int32_t* head_map, const float* out, int ldo, const float* alpha,
                             const float* g_out, float* dS, float* dattr, float* d_xl, float* d_xr, int ldd, float* d_bias_part,
                             float* d_att_part, float* d_we_part, float* d_adj, int accumulate_dadj, int B, int Hs, int C,
                             float slope, int act, void* stream) {
  GatBwdArgs p{};
  p.f = GatLayerArgs{xl, xr, ld, adj, we, att, bias, head_map, const_cast<float*>(out), ldo, const_cast<float*>(alpha), B, Hs, C,
                     slope, act};
  p.g_out = g_out; p.dS = dS; p.dattr = dattr; p.dxl = d_xl; p.dxr = d_xr; p.ldd = ldd;
  p.dbias_part = d_bias_part; p.datt_part = d_att_part; p.dwe_part = d_we_part;
  return launch_gat_layer_backward(p, d_adj, accumulate_dadj, (hipStream_t)stream);
}

int ctvae_gauss_latent_forward(float* heads, const float* eps_in, const uint64_t* rng, float* eps_out, float* z, int B, int L,
                               const float* head_slices, int slices, const float* head_bias, void* stream) {
  return launch_gauss_latent_fwd(heads, eps_in, (const unsigned long long*)rng, eps_out, z, B, L, (hipStream_t)stream, head_slices,
                                 slices, head_bias);
}

int ctvae_gauss_latent_backward(const float* g_mu, const float* g_logvar, const float* g_z, const float* heads, const float* eps,
                                float* g_heads, uint64_t* rng_bump, int B, int L, int g_z_slices, void* stream) {
  return launch_gauss_latent_bwd(g_mu, g_logvar, g_z, heads, eps, g_heads, (unsigned long long*)rng_bump, B, L, (hipStream_t)stream,
                                 g_z_slices);
}

int ctvae_splitk_permute(const float* slices, int n_slices, float* out, int B, int C, int P, void* stream) {
  return launch_splitk_permute(slices, n_slices, out, B, C, P, (hipStream_t)stream);
}

int ctvae_conv_forward_lazy_slices(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                   size_t ws_bytes) {
  if (!conv_kind_ok(kind)) return 0;
  ConvGeom g;
  if (conv_geom(g, kind, 0, B, H, W, Ci, Co, k, stride, pad, out_pad)) return 0;
  const size_t wsf = ws_bytes / sizeof(float);
  if (img_enc_supported(g) || img_conv_supported(g) || upconv_wgrad_supported(g) || (wino_enabled() && wino_supported(g, wsf))) return 0;
  TapGemmPlan pl;
  tapgemm_plan(g, wsf, pl, false);
  return (pl.thin || pl.splitk <= 1) ? 0 : pl.splitk;
}

int ctvae_conv_forward_lazy(int kind, const float* x, const float* w, float* y_slices, int B, int H, int W, int Ci, int Co, int k,
                            int stride, int pad, int out_pad, float* ws, size_t ws_bytes, void* stream) {
  if (!x || !w || !y_slices || !ws || !conv_kind_ok(kind)) return kErrBadArg;
  // only the split tile kernel writes slices; every other launch (unsplit, thin, dedicated, Winograd) would store through the
  // null output pointer handed down below, so a shape the query answers with 0 is refused before anything is launched
  if (ctvae_conv_forward_lazy_slices(kind, B, H, W, Ci, Co, k, stride, pad, out_pad, ws_bytes) <= 1) return kErrBadArg;
  ConvGeom g;
  if (conv_geom(g, kind, 0, B, H, W, Ci, Co, k, stride, pad, out_pad)) return kErrBadArg;
  SplitKRaw raw{y_slices, 0, 1};
  const int rc = launch_tapgemm(g, x, w, nullptr, nullptr, nullptr, 0, nullptr, ACT_NONE, nullptr, ws, ws_bytes / sizeof(float),
                                (hipStream_t)stream, nullptr, nullptr, nullptr, &raw);
  if (rc) return rc;
  return raw.splitk > 1 ? 0 : kErrBadArg;   // the caller asked ctvae_conv_forward_lazy_slices first
}

int ctvae_ct_reg_forward(const float* adj, const float* graph, const float* uniform, float* part4, float ckl, float cgs, float cpt,
                         int B, int N, void* stream) {
  return launch_ct_reg_forward(adj, graph, uniform, part4, ckl, cgs, cpt, B, N, (hipStream_t)stream);
}

int ctvae_ct_reg_backward(const float* adj, const float* graph, const float* uniform, const float* part4, const float* g_loss,
                          float ckl, float cgs, float cpt, float* d_adj, float* d_graph, int B, int N, void* stream) {
  return launch_ct_reg_backward(adj, graph, uniform, part4, g_loss, ckl, cgs, cpt, d_adj, d_graph, B, N, (hipStream_t)stream);
}

int ctvae_ct_blend_softmax_forward(const float* y, const float* mask, float* probs, long R, int Hs, int D, void* stream) {
  return launch_ct_blend_softmax_forward(y, mask, probs, R, Hs, D, (hipStream_t)stream);
}

int ctvae_ct_blend_softmax_backward(const float* g, const float* probs, const float* y, const float* mask, float* dy, float* dmask,
                                    long R, int Hs, int D, void* stream) {
  return launch_ct_blend_softmax_backward(g, probs, y, mask, dy, dmask, R, Hs, D, (hipStream_t)stream);
}

int ctvae_ct_latent_ce_forward(const float* probs, const int64_t* target, float* row_loss, long R, int D, void* stream) {
  return launch_ct_latent_ce_forward(probs, (const long long*)target, row_loss, R, D, (hipStream_t)stream);
}

int ctvae_ct_latent_ce_backward(const float* probs, const int64_t* target, const float* g_loss, float* d_probs, long R, int D,
                                void* stream) {
  return launch_ct_latent_ce_backward(probs, (const long long*)target, g_loss, d_probs, R, D, (hipStream_t)stream);
}

int ctvae_ct_mask_forward(const float* x, const float* action, const float* pe, const float* keep, float scale, const float* W,
                          const float* bias, const float* expo, int B, int S, int D, int A, float* inter, float* p, float* sample,
                          float* soft, void* stream) {
  return launch_ct_mask_forward(x, action, pe, keep, scale, W, bias, expo, B, S, D, A, inter, p, sample, soft, (hipStream_t)stream);
}

int ctvae_ct_mask_backward(const float* x, const float* action, const float* pe, const float* keep, float scale, const float* inter,
                           const float* p, const float* soft, const float* g, int B, int S, int D, int A, float* dWp, float* dbp,
                           void* stream) {
  return launch_ct_mask_backward(x, action, pe, keep, scale, inter, p, soft, g, B, S, D, A, dWp, dbp, (hipStream_t)stream);
}

int ctvae_ct_sample_forward(const float* p, const float* expo, float* sample, float* soft, float* weighted, long n, void* stream) {
  return launch_ct_sample_forward(p, expo, sample, soft, weighted, n, (hipStream_t)stream);
}

int ctvae_ct_sample_backward(const float* g_sample, const float* g_weighted, const float* p, const float* soft, const float* sample,
                             float* g_p, long n, void* stream) {
  return launch_ct_sample_backward(g_sample, g_weighted, p, soft, sample, g_p, n, (hipStream_t)stream);
}

int ctvae_ct_blend_forward(const float* s0, const float* s1, const float* mask, float* out, long rows, void* stream) {
  return launch_ct_blend_forward(s0, s1, mask, out, rows, (hipStream_t)stream);
}

int ctvae_ct_blend_backward(const float* g, const float* s0, const float* s1, const float* mask, float* g0, float* g1, float* g_mask,
                            long rows, void* stream) {
  return launch_ct_blend_backward(g, s0, s1, mask, g0, g1, g_mask, rows, (hipStream_t)stream);
}

int ctvae_ct_posenc_forward(const float* x, const float* pe, const float* keep, float scale, float* out, long n, int sd,
                            void* stream) {
  return launch_ct_posenc_forward(x, pe, keep, scale, out, n, sd, (hipStream_t)stream);
}

int ctvae_ct_posenc_backward(const float* g, const float* keep, float scale, float* g_x, long n, void* stream) {
  return launch_ct_posenc_backward(g, keep, scale, g_x, n, (hipStream_t)stream);
}

int ctvae_one_hot(const int64_t* inds, long n, int N, float* out, void* stream) {
  return launch_one_hot((const long long*)inds, n, N, out, (hipStream_t)stream);
}

int ctvae_group_rowsum(const float* parts, long mat_stride, int nmat, int rows, int C, int ld, const int32_t* group, int G, float* out,
                       int accumulate, void* stream) {
  return launch_group_rowsum(parts, mat_stride, nmat, rows, C, ld, group, G, out, accumulate, (hipStream_t)stream);
}

static int glin_fill(GLinArgs& a, int nseg, int N, const float* const* W, const int* ldw, const int64_t* w_gstride,
                     const float* const* bias, const int* b_gstride, const int32_t* const* group) {
  if (nseg < 1 || nseg > kGLinMaxSeg || !W || !ldw || !w_gstride) return kErrBadArg;
  a.nseg = nseg;
  a.N = N;
  for (int s = 0; s < nseg; ++s) {
    a.W[s] = W[s];
    a.ldw[s] = ldw[s];
    a.wgs[s] = (long)w_gstride[s];
    a.bias[s] = bias ? bias[s] : nullptr;
    a.bgs[s] = b_gstride ? b_gstride[s] : 0;
    a.group[s] = group ? group[s] : nullptr;
  }
  return 0;
}

int ctvae_glinear_forward(const float* x, int ldx, int K, int nseg, int N, const float* const* W, const int* ldw,
                          const int64_t* w_gstride, const float* const* bias, const int* b_gstride,
                          const int32_t* const* group, float* y, int ldy, int B, void* stream) {
  GLinArgs a{};
  if (int rc = glin_fill(a, nseg, N, W, ldw, w_gstride, bias, b_gstride, group)) return rc;
  a.x = x; a.ldx = ldx; a.K = K; a.y = y; a.ldy = ldy; a.B = B;
  return launch_glinear_forward(a, (hipStream_t)stream);
}

int ctvae_glinear_dgrad(const float* dy, int ldy, int nseg, int N, const float* const* W, const int* ldw,
                        const int64_t* w_gstride, const int32_t* const* group, float* dx, int ldx, int K, int B, void* stream) {
  GLinArgs a{};
  if (int rc = glin_fill(a, nseg, N, W, ldw, w_gstride, nullptr, nullptr, group)) return rc;
  a.x = nullptr; a.ldx = ldx; a.K = K; a.y = const_cast<float*>(dy); a.ldy = ldy; a.B = B;
  return launch_glinear_dgrad(a, dx, (hipStream_t)stream);
}

size_t ctvae_glinear_wgrad_ws_bytes(int G, int N, int K, int B, int grouped) {
  if (G <= 0 || N <= 0 || K <= 0 || B <= 0) return 0;
  return glinear_wgrad_ws_floats(G, N, K, glinear_wgrad_slices(B, G, grouped != 0)) * sizeof(float);
}

int ctvae_glinear_wgrad(const float* x, int ldx, int K, const float* dy, int ldy, int col0, int N, const int32_t* group, int G,
                        int B, float* dW, int ldo, float* dbias, int accumulate, float* ws, size_t ws_bytes, void* stream) {
  return launch_glinear_wgrad(x, ldx, K, dy, ldy, col0, N, group, G, B, dW, ldo, dbias, accumulate, ws, ws_bytes / sizeof(float),
                              (hipStream_t)stream);
}

int ctvae_pair_mlp_forward(const float* u, const float* v, int ld, const float* w2, const float* b2, float* out, int B, int N,
                           int H, float slope, int per_sample, const int32_t* row_of, void* stream) {
  if (!u || !v || !w2 || !out) return kErrBadArg;
  return launch_pair_mlp_forward(u, v, ld, w2, b2, out, B, N, H, slope, per_sample, row_of, (hipStream_t)stream);
}

int ctvae_pair_mlp_backward(const float* u, const float* v, int ld, const float* w2, const float* out, const float* g_out,
                            float* d_u, float* d_v, int ldd, float* d_w2_part, float* d_b2_part, int B, int N, int H, float slope,
                            int per_sample, const int32_t* row_of, void* stream) {
  if (!u || !v || !w2 || !out || !g_out || !d_u || !d_v || !d_w2_part || !d_b2_part) return kErrBadArg;
  return launch_pair_mlp_backward(u, v, ld, w2, out, g_out, d_u, d_v, ldd, d_w2_part, d_b2_part, B, N, H, slope, per_sample,
                                  row_of, (hipStream_t)stream);
}

int ctvae_permute(const float* in, float* out, int B, int C, int P, int to_nhwc, void* stream) {
  if (!in || !out || B <= 0 || C <= 0 || P <= 0) return kErrBadArg;
  return launch_permute(in, out, B, C, P, to_nhwc, (hipStream_t)stream);
}

int ctvae_act_forward(const float* in, float* out, long n, int act, void* stream) {
  if (!in || !out || n <= 0) return kErrBadArg;
  return launch_act_fwd(in, out, n, act, (hipStream_t)stream);
}

int ctvae_act_backward(const float* g_out, const float* out, float* g_in, long n, int act, void* stream) {
  if (!g_out || !out || !g_in || n <= 0) return kErrBadArg;
  return launch_act_bwd(g_out, out, g_in, n, act, (hipStream_t)stream);
}

int ctvae_reparam_forward(const float* mu, long mu_rs, const float* logvar, long lv_rs, const float* eps, float* z, int B,
                          int L, void* stream) {
  if (!mu || !logvar || !eps || !z || B <= 0 || L <= 0) return kErrBadArg;
  return launch_reparam_fwd(mu, mu_rs, logvar, lv_rs, eps, z, B, L, (hipStream_t)stream);
}

int ctvae_reparam_backward(const float* g_z, const float* logvar, long lv_rs, const float* eps, float* g_mu,
                           float* g_logvar, int B, int L, void* stream) {
  if (!g_z || !logvar || !eps || !g_mu || !g_logvar || B <= 0 || L <= 0) return kErrBadArg;
  return launch_reparam_bwd(g_z, logvar, lv_rs, eps, g_mu, g_logvar, B, L, (hipStream_t)stream);
}

int ctvae_loss_forward(const float* recons, const float* x, long n, const float* mu, long mu_rs, const float* logvar,
                       long lv_rs, int B, int L, float M_N, const float* extra, float* out4, float* ws, size_t ws_bytes,
                       void* stream) {
  if (!recons || !x || !out4 || !ws || n <= 0) return kErrBadArg;
  if ((mu == nullptr) != (logvar == nullptr)) return kErrBadArg;
  return launch_loss_forward(recons, x, n, mu, mu_rs, logvar, lv_rs, B, L, M_N, extra, out4, ws, ws_bytes,
                             (hipStream_t)stream, 0.f);
}

int ctvae_loss_forward_grad(const float* recons, const float* x, long n, const float* mu, long mu_rs, const float* logvar,
                            long lv_rs, int B, int L, float M_N, const float* extra, float* out4, float* g_recons, float* g_mu,
                            float* g_logvar, int recons_act, float* ws, size_t ws_bytes, void* stream) {
  if (!recons || !x || !out4 || !ws || n <= 0 || !mu || !logvar || !g_recons || !g_mu || !g_logvar) return kErrBadArg;
  return launch_loss_forward(recons, x, n, mu, mu_rs, logvar, lv_rs, B, L, M_N, extra, out4, ws, ws_bytes,
                             (hipStream_t)stream, 0.f, g_recons, g_mu, g_logvar, recons_act);
}

int ctvae_mse_backward(const float* recons, const float* x, const float* g_loss, float* g_recons, long n, int recons_act,
                       void* stream) {
  if (!recons || !x || !g_loss || !g_recons || n <= 0) return kErrBadArg;
  return launch_mse_backward(recons, x, g_loss, g_recons, n, (hipStream_t)stream, 0.f, recons_act);
}

int ctvae_loss_backward(const float* recons, const float* x, const float* g_loss, float* g_recons, long n, float logcosh_alpha,
                        const float* mu, long mu_rs, const float* logvar, long lv_rs, float* g_mu, float* g_logvar, int B, int L,
                        float M_N, int recons_act, void* stream) {
  if (!recons || !x || !g_loss || !g_recons || n <= 0 || !mu || !logvar || !g_mu || !g_logvar || B <= 0 || L <= 0) return kErrBadArg;
  return launch_loss_backward(recons, x, g_loss, g_recons, n, logcosh_alpha, mu, mu_rs, logvar, lv_rs, g_mu, g_logvar, B, L, M_N,
                              (hipStream_t)stream, recons_act);
}

int ctvae_l2l1_loss_forward(const float* recons, const float* x, long n, const float* extra, float* out4, float* ws, size_t ws_bytes,
                            void* stream) {
  if (!recons || !x || !out4 || !ws || n <= 0) return kErrBadArg;
  return launch_loss_forward(recons, x, n, nullptr, 0, nullptr, 0, 0, 0, 0.f, extra, out4, ws, ws_bytes, (hipStream_t)stream, -1.f);
}

int ctvae_l2l1_backward(const float* recons, const float* x, const float* g_loss, float* g_recons, long n, int recons_act,
                        void* stream) {
  if (!recons || !x || !g_loss || !g_recons || n <= 0) return kErrBadArg;
  return launch_mse_backward(recons, x, g_loss, g_recons, n, (hipStream_t)stream, -1.f, recons_act);
}

int ctvae_ladder_merge_forward(const float* mu_e, const float* logvar_e, const float* mu_t, const float* logvar_t, const float* eps,
                               int B, int D, float* z, float* kl, void* stream) {
  return launch_ladder_forward(mu_e, logvar_e, mu_t, logvar_t, eps, B, D, z, kl, (hipStream_t)stream);
}

int ctvae_ladder_merge_backward(const float* g_z, const float* g_kl, const float* mu_e, const float* logvar_e, const float* mu_t,
                                const float* logvar_t, const float* eps, int B, int D, float* g_mu_e, float* g_logvar_e,
                                float* g_mu_t, float* g_logvar_t, void* stream) {
  return launch_ladder_backward(g_z, g_kl, mu_e, logvar_e, mu_t, logvar_t, eps, B, D, g_mu_e, g_logvar_e, g_mu_t, g_logvar_t,
                                (hipStream_t)stream);
}

int ctvae_gamma_reparam_forward(const float* alpha, const float* beta, const float* zhat, float gamma_shape, float* z, long n,
                                void* stream) {
  return launch_gamma_reparam_forward(alpha, beta, zhat, gamma_shape, z, n, (hipStream_t)stream);
}

int ctvae_gamma_reparam_backward(const float* g_z, const float* alpha, const float* beta, const float* zhat, float gamma_shape,
                                 float* g_alpha, float* g_beta, long n, void* stream) {
  return launch_gamma_reparam_backward(g_z, alpha, beta, zhat, gamma_shape, g_alpha, g_beta, n, (hipStream_t)stream);
}

int ctvae_gamma_kl_forward(const float* alpha, const float* beta, int B, int D, float prior_alpha, float prior_beta, float* out,
                           float* ws, size_t ws_bytes, void* stream) {
  return launch_gamma_kl_forward(alpha, beta, B, D, prior_alpha, prior_beta, out, ws, ws_bytes, (hipStream_t)stream);
}

int ctvae_gamma_kl_backward(const float* g_kld, const float* alpha, const float* beta, int B, int D, float prior_alpha,
                            float prior_beta, float* g_alpha, float* g_beta, void* stream) {
  return launch_gamma_kl_backward(g_kld, alpha, beta, B, D, prior_alpha, prior_beta, g_alpha, g_beta, (hipStream_t)stream);
}

int ctvae_sigmoid_forward(const float* x, float* y, long n, void* stream) { return launch_sigmoid(x, nullptr, y, n, 0, (hipStream_t)stream); }

int ctvae_sigmoid_backward(const float* g, const float* y, float* g_x, long n, void* stream) {
  return launch_sigmoid(g, y, g_x, n, 1, (hipStream_t)stream);
}

int ctvae_tc_forward(const float* z, const float* mu, const float* logvar, const float* log_iw, int B, int D, float* out3, float* lse_s,
                     float* lse_d, float* ws, size_t ws_bytes, void* stream) {
  return launch_tc_forward(z, mu, logvar, log_iw, B, D, out3, lse_s, lse_d, ws, ws_bytes, (hipStream_t)stream);
}

int ctvae_tc_backward(const float* z, const float* mu, const float* logvar, const float* log_iw, const float* lse_s, const float* lse_d,
                      const float* g3, int B, int D, float* g_z, float* g_mu, float* g_logvar, void* stream) {
  return launch_tc_backward(z, mu, logvar, log_iw, lse_s, lse_d, g3, B, D, g_z, g_mu, g_logvar, (hipStream_t)stream);
}

int ctvae_vamp_kl_forward(const float* z, const float* mu, const float* logvar, const float* prior_mu, const float* prior_logvar,
                          int B, int D, int K, float* out3, float* weights, float* ws, size_t ws_bytes, void* stream) {
  return launch_vamp_forward(z, mu, logvar, prior_mu, prior_logvar, B, D, K, out3, weights, ws, ws_bytes, (hipStream_t)stream);
}

int ctvae_vamp_kl_backward(const float* z, const float* mu, const float* logvar, const float* prior_mu, const float* prior_logvar,
                           const float* weights, const float* g_kld, int B, int D, int K, float* g_z, float* g_mu, float* g_logvar,
                           float* g_prior_mu, float* g_prior_logvar, void* stream) {
  return launch_vamp_backward(z, mu, logvar, prior_mu, prior_logvar, weights, g_kld, B, D, K, g_z, g_mu, g_logvar, g_prior_mu,
                              g_prior_logvar, (hipStream_t)stream);
}

int ctvae_swd_forward(const float* z, const float* prior, const float* proj, int N, int D, int S, float p, float weight, float* out,
                      float* grad_z, float* ws, size_t ws_bytes, void* stream) {
  return launch_swd_forward(z, prior, proj, N, D, S, p, weight, out, grad_z, ws, ws_bytes, (hipStream_t)stream);
}

int ctvae_logcosh_loss_forward(const float* recons, const float* x, long n, float alpha, const float* mu, long mu_rs,
                               const float* logvar, long lv_rs, int B, int L, float M_N, float* out4, float* ws,
                               size_t ws_bytes, void* stream) {
  if (!recons || !x || !out4 || !ws || n <= 0 || !(alpha > 0.f)) return kErrBadArg;
  if ((mu == nullptr) != (logvar == nullptr)) return kErrBadArg;
  return launch_loss_forward(recons, x, n, mu, mu_rs, logvar, lv_rs, B, L, M_N, nullptr, out4, ws, ws_bytes,
                             (hipStream_t)stream, alpha);
}

int ctvae_logcosh_backward(const float* recons, const float* x, const float* g_loss, float* g_recons, long n, float alpha,
                           int recons_act, void* stream) {
  if (!recons || !x || !g_loss || !g_recons || n <= 0 || !(alpha > 0.f)) return kErrBadArg;
  return launch_mse_backward(recons, x, g_loss, g_recons, n, (hipStream_t)stream, alpha, recons_act);
}

int ctvae_kl_backward(const float* mu, long mu_rs, const float* logvar, long lv_rs, const float* g_loss, float* g_mu,
                      float* g_logvar, int B, int L, float M_N, void* stream) {
  if (!mu || !logvar || !g_loss || !g_mu || !g_logvar) return kErrBadArg;
  return launch_kl_backward(mu, mu_rs, logvar, lv_rs, g_loss, g_mu, g_logvar, B, L, M_N, (hipStream_t)stream);
}

int ctvae_vq_inds(const float* latents, const float* codebooks, int64_t* inds, int B, int HW, int D, int K, int C,
                  void* stream) {
  if (!latents || !codebooks || !inds || B <= 0 || HW <= 0 || C <= 0) return kErrBadArg;
  return launch_vq_inds(latents, codebooks, (long long*)inds, B, HW, D, K, C, (hipStream_t)stream);
}

int ctvae_vq_lookup(const float* latents, const float* codebooks, const int64_t* inds, float* quantized, float* vq_loss,
                    float beta, int B, int HW, int D, int K, int C, float* ws, size_t ws_bytes, void* stream) {
  if (!latents || !codebooks || !inds || !quantized || !vq_loss || !ws || C <= 0) return kErrBadArg;
  return launch_vq_lookup(latents, codebooks, (const long long*)inds, quantized, vq_loss, beta, B, HW, D, K, C, ws, ws_bytes,
                          (hipStream_t)stream);
}

int ctvae_vq_backward(const float* g_quantized, const float* g_vq_loss, const float* latents, const float* codebooks,
                      const int64_t* inds, float* g_latents, float* d_codebooks, int accumulate, float beta, int B, int HW,
                      int D, int K, int C, float* ws, size_t ws_bytes, void* stream) {
  if (!latents || !codebooks || !inds || C <= 0) return kErrBadArg;
  return launch_vq_backward(g_quantized, g_vq_loss, latents, codebooks, (const long long*)inds, g_latents, d_codebooks,
                            accumulate, beta, B, HW, D, K, C, ws, ws_bytes, (hipStream_t)stream);
}

int ctvae_gumbel_st_forward(const float* p, const float* gumbel_noise, float* sample, float* soft, long n, void* stream) {
  if (!p || !gumbel_noise || !sample || !soft || n <= 0) return kErrBadArg;
  return launch_gumbel_fwd(p, gumbel_noise, sample, soft, n, (hipStream_t)stream);
}

int ctvae_gumbel_st_backward(const float* g_sample, const float* p, const float* soft, float* g_p, long n, void* stream) {
  if (!g_sample || !p || !soft || !g_p || n <= 0) return kErrBadArg;
  return launch_gumbel_bwd(g_sample, p, soft, g_p, n, (hipStream_t)stream);
}

int ctvae_gumbel_softmax_forward(const float* logits, const float* uniform, float* sample, long rows, int Q, float temperature,
                                 float eps, void* stream) {
  if (!logits || !uniform || !sample || rows <= 0 || Q <= 0 || !(temperature > 0.f)) return kErrBadArg;
  return launch_gumbel_softmax_fwd(logits, uniform, sample, rows, Q, temperature, eps, (hipStream_t)stream);
}

int ctvae_gumbel_softmax_backward(const float* g_sample, const float* sample, float* g_logits, long rows, int Q,
                                  float temperature, void* stream) {
  if (!g_sample || !sample || !g_logits || rows <= 0 || Q <= 0 || !(temperature > 0.f)) return kErrBadArg;
  return launch_gumbel_softmax_bwd(g_sample, sample, g_logits, rows, Q, temperature, (hipStream_t)stream);
}

int ctvae_cat_kl_forward(const float* logits, long rows, int Q, int B, float eps, float log_prior, float* kld, float* ws,
                         size_t ws_bytes, void* stream) {
  if (!logits || !kld || !ws || rows <= 0 || Q <= 0 || B <= 0) return kErrBadArg;
  return launch_cat_kl_fwd(logits, rows, Q, B, eps, log_prior, kld, ws, ws_bytes, (hipStream_t)stream);
}

int ctvae_cat_kl_backward(const float* logits, const float* g_kld, float* g_logits, long rows, int Q, int B, float eps,
                          float log_prior, void* stream) {
  if (!logits || !g_kld || !g_logits || rows <= 0 || Q <= 0 || B <= 0) return kErrBadArg;
  return launch_cat_kl_bwd(logits, g_kld, g_logits, rows, Q, B, eps, log_prior, (hipStream_t)stream);
}

int ctvae_iw_loss_forward(const float* recons, const float* x, long n, int R, int rep, const float* mu, const float* logvar,
                          int L, int S, float M_N, float* lp, float* kld, float* coef, float* out4, void* stream) {
  if (!recons || !x || !mu || !logvar || !lp || !kld || !coef || !out4) return kErrBadArg;
  if (n <= 0 || (n & 3) || R <= 0 || rep <= 0 || R % rep || S <= 0 || R % S || L <= 0) return kErrBadArg;
  return launch_iw_loss_forward(recons, x, n, R, rep, mu, logvar, L, S, M_N, lp, kld, coef, out4, (hipStream_t)stream);
}

int ctvae_iw_loss_backward(const float* recons, const float* x, long n, int R, int rep, const float* mu, const float* logvar,
                           int L, float M_N, const float* coef, const float* g_loss, float* g_recons, float* g_mu,
                           float* g_logvar, void* stream) {
  if (!recons || !x || !mu || !logvar || !coef || !g_loss || (g_mu == nullptr) != (g_logvar == nullptr)) return kErrBadArg;
  if (n <= 0 || (n & 3) || R <= 0 || rep <= 0 || R % rep || L <= 0) return kErrBadArg;
  return launch_iw_loss_backward(recons, x, n, R, rep, mu, logvar, L, M_N, coef, g_loss, g_recons, g_mu, g_logvar,
                                 (hipStream_t)stream);
}

int ctvae_mmd_forward(const float* z, const float* prior, int N, int D, int kind, float c, float eps, float w_pp, float w_zz,
                      float w_pz, float* out4, float* grad_z, float* ws, size_t ws_bytes, void* stream) {
  if (!z || !prior || !out4 || !grad_z || !ws || N <= 0 || D <= 0 || (kind != 0 && kind != 1) || !(c > 0.f)) return kErrBadArg;
  return launch_mmd_forward(z, prior, N, D, kind, c, eps, w_pp, w_zz, w_pz, out4, grad_z, ws, ws_bytes, (hipStream_t)stream);
}

size_t ctvae_dip_state_floats(int B, int D) { return dip_state_floats(B, D); }

int ctvae_dip_forward(const float* mu, long mu_rs, const float* logvar, long lv_rs, int B, int D, float lambda_diag,
                      float lambda_offdiag, float* state, void* stream) {
  if (!mu || !logvar || !state || B <= 0 || D <= 0) return kErrBadArg;
  return launch_dip_forward(mu, mu_rs, logvar, lv_rs, B, D, lambda_diag, lambda_offdiag, state, (hipStream_t)stream);
}

int ctvae_dip_backward(const float* state, const float* g_dip, float* g_mu, float* g_logvar, int B, int D, void* stream) {
  if (!state || !g_dip || !g_mu || !g_logvar || B <= 0 || D <= 0) return kErrBadArg;
  return launch_dip_backward(state, g_dip, g_mu, g_logvar, B, D, (hipStream_t)stream);
}

int ctvae_column_moments(const float* z, int N, int L, float* mean, float* var, float* min, float* max, void* stream) {
  if (!z || !mean || !var || !min || !max) return kErrBadArg;
  return launch_column_moments(z, N, L, mean, var, min, max, (hipStream_t)stream);
}

int ctvae_mi_matrix(const float* z, const float* lo, const float* hi, const int32_t* factors, const int32_t* sizes, int N, int L,
                    int F, float* mi, uint8_t* bins, void* stream) {
  if (!z || !lo || !hi || !factors || !sizes || !mi) return kErrBadArg;
  return launch_mi_matrix(z, lo, hi, factors, sizes, N, L, F, mi, bins, (hipStream_t)stream);
}

int ctvae_group_var_argmin(const float* z, const float* global_var, const uint8_t* active, int G, int B, int L, int32_t* arg,
                           float* val, void* stream) {
  if (!z || !global_var || !active || !arg || !val) return kErrBadArg;
  return launch_group_var_argmin(z, global_var, active, G, B, L, arg, val, (hipStream_t)stream);
}

int ctvae_image_grid_u8(const float* x, long stride_n, long stride_c, long stride_h, long stride_w, int N, int C, int H, int W,
                        int nrow, int padding, int normalize, int has_range, float range_lo, float range_hi, float pad_value,
                        int scanlines, uint8_t* out, size_t out_bytes, float* workspace, size_t workspace_bytes, void* stream) {
  return launch_image_grid_u8(x, stride_n, stride_c, stride_h, stride_w, N, C, H, W, nrow, padding, normalize, has_range, range_lo,
                              range_hi, pad_value, scanlines, out, out_bytes, workspace, workspace_bytes, (hipStream_t)stream);
}

int ctvae_image_grid_each_u8(const float* x, long stride_n, long stride_c, long stride_h, long stride_w, int N, int C, int H, int W,
                             int nrow, int padding, int normalize, int has_range, float range_lo, float range_hi, float pad_value,
                             int scanlines, uint8_t* out, size_t out_bytes, float* workspace, size_t workspace_bytes, void* stream) {
  return launch_image_grid_each_u8(x, stride_n, stride_c, stride_h, stride_w, N, C, H, W, nrow, padding, normalize, has_range,
                                   range_lo, range_hi, pad_value, scanlines, out, out_bytes, workspace, workspace_bytes,
                                   (hipStream_t)stream);
}

int ctvae_action_hits(const float* probas, const float* action, int N, int A, int* counts, void* stream) {
  return launch_action_hits(probas, action, N, A, counts, (hipStream_t)stream);
}

int ctvae_graph_accumulate(const float* adj, const int32_t* group, const float* mask, float threshold, int B, int S, int G,
                           double* adj_sum, int32_t* edge_count, double* mask_sum, int32_t* rows, int32_t* mask_rows,
                           int32_t* skipped, void* stream) {
  return launch_graph_accumulate(adj, group, mask, threshold, B, S, G, adj_sum, edge_count, mask_sum, rows, mask_rows, skipped,
                                 (hipStream_t)stream);
}

int ctvae_heatmap_u8(const float* values, int M, int H, int W, float lo, float hi, int cell, int nrow, int padding, int pad_r,
                     int pad_g, int pad_b, const uint8_t* table, int scanlines, uint8_t* out, size_t out_bytes, void* stream) {
  return launch_heatmap_u8(values, M, H, W, lo, hi, cell, nrow, padding, pad_r, pad_g, pad_b, table, scanlines, out, out_bytes,
                           (hipStream_t)stream);
}

int ctvae_latent_accumulate(const float* mu, long mu_pitch, const float* logvar, long logvar_pitch, int B, int L, double* kl_sum,
                            double* mu_sum, double* sig2_sum, double* cov_sum, int32_t* nonfinite, int32_t* rows, void* stream) {
  return launch_latent_accumulate(mu, mu_pitch, logvar, logvar_pitch, B, L, kl_sum, mu_sum, sig2_sum, cov_sum, nonfinite, rows,
                                  (hipStream_t)stream);
}

int ctvae_gmm_estep(const float* X, int N, int D, int K, int full, const float* log_w, const float* mu, const float* P,
                    const float* log_det_half, float* r, float* ll, int32_t* nonfinite, void* stream) {
  return launch_gmm_estep(X, N, D, K, full, log_w, mu, P, log_det_half, r, ll, nonfinite, (hipStream_t)stream);
}

int ctvae_gmm_mstep_slabs(int N, int D, int K, int full) { return gmm_mstep_slabs(N, D, K, full); }
size_t ctvae_gmm_mstep_workspace_bytes(int N, int D, int K, int full) { return gmm_mstep_workspace_bytes(N, D, K, full); }

int ctvae_gmm_mstep(const float* X, const float* r, const int32_t* nonfinite, int N, int D, int K, int full, const float* m,
                    double* Nk, double* S1, double* S2, double* ws, size_t ws_bytes, void* stream) {
  return launch_gmm_mstep(X, r, nonfinite, N, D, K, full, m, Nk, S1, S2, ws, ws_bytes, (hipStream_t)stream);
}

int ctvae_gmm_sample(const float* u, const float* eps, int n, int D, int K, int full, const double* cdf, const float* mu,
                     const float* L, float* z, int32_t* comp, void* stream) {
  return launch_gmm_sample(u, eps, n, D, K, full, cdf, mu, L, z, comp, (hipStream_t)stream);
}

int ctvae_recon_record(const float* a, const float* b, int B, int S, int C, const double* consts, double* records, int32_t* flags,
                       int row0, int capacity, void* stream) {
  return launch_recon_record(a, b, B, S, C, consts, records, flags, row0, capacity, (hipStream_t)stream);
}

int ctvae_recon_worst(const double* old_ssim, const int32_t* old_row, const float* old_a, const float* old_b, const double* records,
                      const int32_t* flags, int row0, int B, int capacity, const float* batch_a, const float* batch_b, int S, int C,
                      int K, double* new_ssim, int32_t* new_row, float* new_a, float* new_b, int32_t* source, void* stream) {
  return launch_recon_worst(old_ssim, old_row, old_a, old_b, records, flags, row0, B, capacity, batch_a, batch_b, S, C, K, new_ssim,
                            new_row, new_a, new_b, source, (hipStream_t)stream);
}

int ctvae_loglik_latent(const float* mu, const float* logvar, const float* eps, int B, int S, int L, float* z, double* a,
                        void* stream) {
  return launch_loglik_latent(mu, logvar, eps, B, S, L, z, a, (hipStream_t)stream);
}

int ctvae_loglik_rows(const float* xhat, const float* x, int B, int S, long P, const double* a, const double* consts, double* lw,
                      void* stream) {
  return launch_loglik_rows(xhat, x, B, S, P, a, consts, lw, (hipStream_t)stream);
}

int ctvae_loglik_merge(const double* lw, int B, int S, double* state, int32_t* flags, int row0, int capacity, void* stream) {
  return launch_loglik_merge(lw, B, S, state, flags, row0, capacity, (hipStream_t)stream);
}

size_t ctvae_freebits_workspace_bytes(int L) { return freebits_workspace_bytes(L); }

int ctvae_freebits_kl_forward_grad(const float* mu, long mu_pitch, const float* logvar, long logvar_pitch, int B, int L,
                                   const float* w_dev, float scale, float free_bits, float* out, float* g_mu, float* g_logvar,
                                   float* ws, size_t ws_bytes, void* stream) {
  return launch_freebits_kl(mu, mu_pitch, logvar, logvar_pitch, B, L, w_dev, scale, free_bits, out, g_mu, g_logvar, ws, ws_bytes,
                            (hipStream_t)stream);
}

size_t ctvae_adam_state_floats(void) { return adam_state_floats(); }

size_t ctvae_mssim_part_floats(int B, int C) { return (size_t)5 * B * C * 2; }
int ctvae_mssim_forward(const float* a, const float* b, const float* window, const float* weights, float* part, float* loss,
                        float* coef, int B, int C, int H, int W, void* stream) {
  return launch_ssim_forward(a, b, window, part, loss, coef, B, C, H, W, weights, (hipStream_t)stream);
}
int ctvae_mssim_backward(const float* a, const float* b, const float* window, const float* coef, const float* g_loss, float* g_a,
                         int B, int C, int H, int W, void* stream) {
  return launch_ssim_backward(a, b, window, coef, g_loss, g_a, B, C, H, W, (hipStream_t)stream);
}

int ctvae_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* state, long n,
                    float grad_scale, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !state || n <= 0) return kErrBadArg;
  return launch_adam(params, grads, exp_avg, exp_avg_sq, state, n, grad_scale, (hipStream_t)stream);
}

size_t ctvae_grad_clip_workspace_floats(void) { return grad_clip_workspace_floats(); }

int ctvae_adam_step_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* state, long n,
                            float grad_scale, int algorithm, float clip_val, float* workspace, float* norm_out, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !state || n <= 0 || !(clip_val > 0.f)) return kErrBadArg;
  if (algorithm != CTVAE_CLIP_NORM && algorithm != CTVAE_CLIP_VALUE) return kErrBadArg;
  if (algorithm == CTVAE_CLIP_NORM && !workspace) return kErrBadArg;
  return launch_adam_clipped(params, grads, exp_avg, exp_avg_sq, state, n, grad_scale, algorithm, clip_val, workspace, norm_out,
                             (hipStream_t)stream);
}

int ctvae_adam_mark_members(int* hits, int nhits, const int* group, int B, void* stream) {
  if (!hits || nhits < 1 || B < 0 || (B > 0 && !group)) return kErrBadArg;
  return launch_adam_mark_members(hits, nhits, B > 0 ? group : nullptr, B, (hipStream_t)stream);
}

int ctvae_adam_block_flags(const int* present, const int* hit_index, int* hits, int nhits, const float* block_state, int* active,
                           int nb, int until_first, void* stream) {
  if (!present || !hit_index || !block_state || !active || nb < 1 || nhits < 0 || (nhits > 0 && !hits)) return kErrBadArg;
  return launch_adam_block_flags(present, hit_index, hits, nhits, block_state, active, nb, until_first, (hipStream_t)stream);
}

int ctvae_adam_block_flags_local(const int* present, const int* hit_index, int* hits, int nhits, int* active, int nb, void* stream) {
  if (!present || !hit_index || !active || nb < 1 || nhits < 0 || (nhits > 0 && !hits)) return kErrBadArg;
  return launch_adam_block_flags_local(present, hit_index, hits, nhits, active, nb, (hipStream_t)stream);
}

int ctvae_adam_block_flags_finish(const float* block_state, int* active, int nb, int until_first, void* stream) {
  if (!block_state || !active || nb < 1) return kErrBadArg;
  return launch_adam_block_flags_finish(block_state, active, nb, until_first, (hipStream_t)stream);
}

int ctvae_adam_step_blocks(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* state, long n,
                           float grad_scale, int algorithm, float clip_val, float* workspace, float* norm_out,
                           const int* block_lo, const int* block_hi, float* block_state, const int* active, int nb, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !state || n <= 0) return kErrBadArg;
  if (!block_lo || !block_hi || !block_state || !active || nb < 1) return kErrBadArg;
  if (algorithm != CTVAE_CLIP_NORM && algorithm != CTVAE_CLIP_VALUE && algorithm != CTVAE_ADAM_NO_CLIP) return kErrBadArg;
  if (algorithm != CTVAE_ADAM_NO_CLIP && !(clip_val > 0.f)) return kErrBadArg;
  if (algorithm == CTVAE_CLIP_NORM && !workspace) return kErrBadArg;
  return launch_adam_blocks(params, grads, exp_avg, exp_avg_sq, state, n, grad_scale, algorithm, clip_val, workspace, norm_out,
                            block_lo, block_hi, block_state, active, nb, (hipStream_t)stream);
}

size_t ctvae_grad_accumulate_pass_floats(void) { return grad_accumulate_pass_floats(); }

int ctvae_grad_accumulate(float* acc, float* grads, long n, int mode, void* stream) {
  return launch_grad_accumulate(acc, grads, n, mode, (hipStream_t)stream);
}

int ctvae_adam_flags_window(int* window, int* active, int nb, int mode, void* stream) {
  return launch_adam_flags_window(window, active, nb, mode, (hipStream_t)stream);
}

int ctvae_ema_update(float* ema, const float* p, long n, float one_minus_decay, void* stream) {
  return launch_ema_update(ema, p, n, one_minus_decay, (hipStream_t)stream);
}

int ctvae_buffer_swap(float* a, float* b, long n, void* stream) { return launch_buffer_swap(a, b, n, (hipStream_t)stream); }

size_t ctvae_vq_usage_pass_indices(void) { return vq_usage_pass_indices(); }

int ctvae_vq_usage(const long* inds, long* counts, long* invalid, int B, int C, int HW, int K, void* stream) {
  return launch_vq_usage(inds, counts, invalid, B, C, HW, K, (hipStream_t)stream);
}

int ctvae_vq_pool_fill(const float* latents, float* pool, long P, int D, long R, void* stream) {
  return launch_vq_pool_fill(latents, pool, P, D, R, (hipStream_t)stream);
}

int ctvae_vq_usage_pool_fill(const long* inds, long* counts, long* invalid, int B, int C, int HW, int K, const float* latents,
                             float* pool, long P, int D, long R, void* stream) {
  return launch_vq_usage_pool_fill(inds, counts, invalid, B, C, HW, K, latents, pool, P, D, R, (hipStream_t)stream);
}

int ctvae_vq_restart(const long* list, int n, const float* pool, int valid_rows, int D, const float* rows, float* codebooks,
                     float* exp_avg, float* exp_avg_sq, int C, int K, int Dc, void* stream) {
  return launch_vq_restart(list, n, pool, valid_rows, D, rows, codebooks, exp_avg, exp_avg_sq, C, K, Dc, (hipStream_t)stream);
}

int ctvae_vq_restart_gather(const long* list, int n, const float* pool, int valid_rows, int D, int C, int Dc, float* rows,
                            void* stream) {
  return launch_vq_restart_gather(list, n, pool, valid_rows, D, C, Dc, rows, (hipStream_t)stream);
}

int ctvae_vq_lookup_commit(const float* latents, const float* codebooks, const int64_t* inds, float* quantized, float* vq_loss,
                           float beta, int B, int HW, int D, int K, int C, float* ws, size_t ws_bytes, void* stream) {
  if (!latents || !codebooks || !inds || !quantized || !vq_loss || !ws || C <= 0) return kErrBadArg;
  return launch_vq_lookup_commit(latents, codebooks, (const long long*)inds, quantized, vq_loss, beta, B, HW, D, K, C, ws, ws_bytes,
                                 (hipStream_t)stream);
}

int ctvae_vq_ema_supported(int K, int C, int Dc) { return vq_ema_supported(K, C, Dc); }

int ctvae_vq_ema_stats(const float* latents, const long* inds, long* acc_n, float* acc_s, long* invalid, int B, int HW, int D, int K,
                       int C, float* ws, size_t ws_bytes, void* stream) {
  return launch_vq_ema_stats(latents, inds, acc_n, acc_s, invalid, B, HW, D, K, C, ws, ws_bytes, (hipStream_t)stream);
}

int ctvae_vq_ema_update(float* codebooks, float* N, float* M, long* acc_n, float* acc_s, int C, int K, int Dc, float decay, float eps,
                        void* stream) {
  return launch_vq_ema_update(codebooks, N, M, acc_n, acc_s, C, K, Dc, decay, eps, (hipStream_t)stream);
}

int ctvae_code_prior_sample_max_history(void) { return code_prior_sample_max_history(); }

int ctvae_code_prior_count(const long* inds, long* pos, long* left, long* up, long* prev, long* invalid, int B, int C, int H, int W,
                           int K, void* stream) {
  return launch_code_prior_count(inds, pos, left, up, prev, invalid, B, C, H, W, K, (hipStream_t)stream);
}

int ctvae_code_prior_score(const long* inds, const long* pos, const long* left, const long* up, const long* prev,
                           const long* pos_tot, const long* left_tot, const long* up_tot, const long* prev_tot, const double* lambda,
                           double* logp, double* resp, int* bad, int B, int C, int H, int W, int K, void* stream) {
  return launch_code_prior_score(inds, pos, left, up, prev, pos_tot, left_tot, up_tot, prev_tot, lambda, logp, resp, bad, B, C, H, W,
                                 K, (hipStream_t)stream);
}

int ctvae_code_prior_sample(const long* pos, const long* left, const long* up, const long* prev, const long* pos_tot,
                            const long* left_tot, const long* up_tot, const long* prev_tot, const double* lambda, const double* u,
                            long* inds, int n, int C, int H, int W, int K, void* stream) {
  return launch_code_prior_sample(pos, left, up, prev, pos_tot, left_tot, up_tot, prev_tot, lambda, u, inds, n, C, H, W, K,
                                  (hipStream_t)stream);
}

int ctvae_code_prior_embed(const long* inds, const float* codebooks, float* out, int n, int C, int H, int W, int K, int Dc,
                           void* stream) {
  return launch_code_prior_embed(inds, codebooks, out, n, C, H, W, K, Dc, (hipStream_t)stream);
}

size_t ctvae_grad_segment_chunk_floats(void) { return grad_segment_chunk_floats(); }

int ctvae_grad_segment_stats(const float* grads, long n, float scale, float norm_type, const long* segments, int nseg,
                             const int* chunk_seg, const long* chunk_first, const int* seg_chunk_begin, int nchunks,
                             double* part_sum, float* part_f, int* part_bad, double* out_sum, float* out_range, int* out_bad,
                             int* out_hist, const int* flags_in, int* flags_out, int nflags, void* stream) {
  return launch_grad_segment_stats(grads, n, scale, norm_type, segments, nseg, chunk_seg, chunk_first, seg_chunk_begin, nchunks,
                                   part_sum, part_f, part_bad, out_sum, out_range, out_bad, out_hist, flags_in, flags_out, nflags,
                                   (hipStream_t)stream);
}

int ctvae_grad_segment_hist(const float* grads, long n, float scale, const long* segments, int nseg, const int* chunk_seg,
                            const long* chunk_first, int nchunks, const float* out_range, int* out_hist, void* stream) {
  return launch_grad_segment_hist(grads, n, scale, segments, nseg, chunk_seg, chunk_first, nchunks, out_range, out_hist,
                                  (hipStream_t)stream);
}

}  // extern "C"
