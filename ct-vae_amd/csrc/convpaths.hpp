// Launchers and shape predicates of the convolution path that more than one file calls: the dedicated kernels behind the
// tap-GEMM / weight-gradient dispatch (tapgemm.hip, wgrad.hip, thin.hip) and what api.hip reaches directly.  Grouped by the
// file that defines them; each of those files includes this header, so a definition that drifts from its declaration
// does not compile.  The tile kernels' own launchers are in tapgemm.hpp, the paired backward call's in pair.hpp, the
// channel-owner BatchNorm's in finish.hpp.
#pragma once
#include "common.hpp"

namespace ctvae {

// bn.hip
size_t bn_workspace_floats(int C, int nparts);
// coef_out [2][C] (null: kept in ws): scale, shift of the apply pass, for a caller that applies them on load (out == null).
// mean_base [C]: what the means of the partial triples are relative to (null: absolute, as the conv epilogues write them)
int launch_bn_finish_forward(const float* y, int R, int C, int nparts, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, float momentum, float eps, int training, int act,
                             float* out, float* save_mean, float* save_invstd, float* ws, long long* nbt, hipStream_t st,
                             float* coef_out = nullptr, const float* mean_base = nullptr);
int launch_bn_forward(const float* y, int R, int C, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, float momentum, float eps, int training, int act, float* out,
                      float* save_mean, float* save_invstd, float* ws, size_t ws_bytes, long long* nbt, hipStream_t st,
                      float* coef_out = nullptr);
// coef_out [5][C] (null: kept in ws): k1, k2, k3, scale, shift of g_y = k1*g_a*act'(y*scale+shift) + k2*y + k3.
// coef_in [7][C]: the finalize already ran (ctvae_conv_backward bn_coef_out): apply + commit d gamma / d beta (rows 5, 6) only
int launch_bn_backward(const float* ga, const float* beta, const float* y, int R, int C, const float* gamma,
                       const float* save_mean, const float* save_invstd, int act, float* gy, float* dgamma,
                       float* dbeta, int accumulate, float* ws, size_t ws_bytes, const float* part_in, int part_rows,
                       hipStream_t st, float* coef_out = nullptr, const float* coef_in = nullptr);

// image.hip
bool img_conv_supported(const ConvGeom& g);
bool img_dgrad_supported(const ConvGeom& g);
bool img_enc_supported(const ConvGeom& g);
int img_enc_rows(const ConvGeom& g);
int launch_img_enc_forward(const ConvGeom& g, const float* X, const float* W, const float* bias, float* S, int act,
                           float* bn_part, hipStream_t st);
int launch_img_enc_wgrad(const ConvGeom& g, const float* X, const float* dY, float* ws, float** part_out, float** pbias_out,
                         int* nparts, bool want_bias, hipStream_t st, const DyXform* dyx);
int img_wgrad_parts(const ConvGeom& g);
int img_dgrad_rows(const ConvGeom& g);
int launch_img_forward(const ConvGeom& g, const float* X, const float* W, const float* bias, float* S, int act,
                       const InXform* xf, hipStream_t st);
int launch_img_wgrad(const ConvGeom& g, const float* X, const float* dY, float* ws, float** part_out, float** pbias_out,
                     int* nparts, bool want_bias, const InXform* xf, hipStream_t st);
int launch_img_backward_fused(const ConvGeom& g, const float* dY, const float* W, float* dX, const BnBwdFuse* bnb, float* ws,
                              float** part_out, float** pbias_out, int* nparts, bool want_bias, hipStream_t st);
size_t img_backward_fused_ws_floats(const ConvGeom& g);
int launch_img_dgrad(const ConvGeom& g, const float* dY, const float* W, float* dX, const BnBwdFuse* bnb, hipStream_t st);

// tapgemm.hip
bool out_pix_supported(const ConvGeom& g, size_t ws_floats, int out_pix);

// thin.hip
bool thin_forward_supported(const ConvGeom& g);
bool thin_wgrad_supported(const ConvGeom& g);
int thin_bn_parts(const ConvGeom&);
size_t thin_wgrad_workspace_floats(const ConvGeom& g);
int launch_thin_forward(const ConvGeom& g, const float* G, const float* W, const float* bias, const float* add,
                        const float* mask, int mask_act, float* S, int act, float* bn_part, hipStream_t st,
                        const InXform* xf);
int launch_thin_wgrad(const ConvGeom& g, const float* X, const float* dY, float* ws, float** part_out, float** pbias_out,
                      int* nparts_w, int* nparts_b, bool want_bias, hipStream_t st, const InXform* xf);

// upconv.hip
bool upconv_supported(const ConvGeom& g);
bool upconv_wgrad_supported(const ConvGeom& g);
int upconv_rows(const ConvGeom& g);
int launch_upconv_forward(const ConvGeom& g, const float* X, const float* W, const float* bias, float* S, int act,
                          float* bn_part, hipStream_t st, const InXform* xf);
int launch_upconv_wgrad(const ConvGeom& g, const float* X, const float* dY, float* ws, float** part_out, float** pbias_out,
                        int* nparts, bool want_bias, hipStream_t st, const DyXform* dyx, const InXform* xf);

// upimg.hip
bool upimg_supported(const ConvGeom& g);
int launch_upimg_forward(const ConvGeom& g, const float* X, const float* Wp, const float* bias, float* Y, int act,
                         hipStream_t st);

// wgrad.hip
float* defer_wgrad_ws(float* ws, size_t ws_floats);
void defer_wgrad_done();
int defer_begin(float* arena, size_t arena_floats);
int defer_flush(hipStream_t st);
size_t wgrad_workspace_floats(const ConvGeom& g, int S);

// wino.hip
bool wino_enabled();
int wino_set_enabled(int on);
size_t wino_ws_floats(const ConvGeom& g);
bool wino_supported(const ConvGeom& g, size_t ws_floats);
int launch_wino_filters_batch(int n, const float* const* W, float* const* Uf, float* const* Ub, const int* Ci, const int* Co,
                              hipStream_t st);
int launch_wino_conv(const ConvGeom& g, const float* X, const float* Wp, const float* bias, float* Y, int act, float* ws,
                     size_t ws_floats, hipStream_t st, const float* filters_ready, float* bwd_out, const float* add);
bool wino_wgrad_supported(const ConvGeom& g, size_t ws_floats, int* splits);
int launch_wino_wgrad(const ConvGeom& g, const float* X, const float* dY, float* ws, size_t ws_floats, int* nparts,
                      bool want_bias, float** pbias_out, hipStream_t st);

}  // namespace ctvae
