/* ctvae_hip.h — C ABI of libctvae_hip.so (MI355X / gfx950).
 *
 * The reference (Strong-AI-Lab/ct-vae) is 100 % Python and has no FFI of its own: every kernel is
 * reached implicitly through torch.nn / torch.autograd.  This header therefore
 * declares, per implicit op on the hot path, the entry point a binding for that op calls instead;
 * each declaration cites the reference call site it replaces.  All tensors are fp32, activations are
 * NHWC ("channels_last") in HBM, weights are packed [kh*kw][Cin][Cout] (Conv2d AND ConvTranspose2d,
 * with Cin/Cout the layer's input/output channels; Linear = 1x1 conv on a 1x1 image).  No function
 * allocates, synchronises or touches the host: callers own every buffer, incl. the scratch workspace
 * (ctvae_workspace_bytes()), so every call is hipGraph-capturable.  Return value: 0, a hipError_t
 * (>0) or a negative argument/workspace error; ctvae_error_string() maps either to text.
 * `stream` is a hipStream_t passed as void*.
 */
#ifndef CTVAE_HIP_H
#define CTVAE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* activation codes */
#define CTVAE_ACT_NONE 0
#define CTVAE_ACT_LRELU 1 /* nn.LeakyReLU() slope 0.01, vanilla_vae.py:31 */
#define CTVAE_ACT_RELU 2  /* nn.ReLU(True), vq_vae.py:65 */
#define CTVAE_ACT_TANH 3  /* nn.Tanh(), vanilla_vae.py:75, mcq_vae.py:237 */

/* layer kinds */
#define CTVAE_CONV 0  /* nn.Conv2d / nn.Linear */
#define CTVAE_CONVT 1 /* nn.ConvTranspose2d */
/* CTVAE_CONV | CTVAE_W_CI_TAP: the weight block is [Ci][kh*kw][Co] instead of [kh*kw][Ci][Co].  That is the [in][out] block of
 * an nn.Linear whose input is torch.flatten(h, start_dim=1) of an NCHW tensor h [B,Ci,k,k] (vanilla_vae.py:36-37,87-91: in =
 * Ci*k*k, feature index ci*k*k + ky*k + kx): with this flag the layer runs as a k x k convolution straight on the NHWC tensor
 * (forward, data gradient, weight gradient), without the NHWC <-> NCHW copies around the flatten. */
#define CTVAE_W_CI_TAP 0x100

const char* ctvae_version(void);
const char* ctvae_arch(void); /* "gfx950" */
const char* ctvae_error_string(int code);
size_t ctvae_workspace_bytes(void); /* scratch size that is sufficient for every call below */

/* y = act(conv(x, w) + bias + add)
 * Conv2d:          vanilla_vae.py:28-29,73-74; mcq_vae.py:170-171,178-179,189-190,205-209; vq_vae.py:63-67
 * ConvTranspose2d: vanilla_vae.py:50-55,65-70; mcq_vae.py:223-236        Linear: vanilla_vae.py:36-37,43
 * x [B,H,W,Ci], y [B,Ho,Wo,Co]; bias/add may be NULL (add has y's layout: ResidualLayer skip, vq_vae.py:69-70).
 * add is NOT taken on the thin shapes (3 output channels, 32 or 64 input channels, output a multiple of 8 x 32 resp. 8 x 16
 * pixels per parity class -- the image-side convs): kErrBadArg there, nothing launched.  The dedicated kernels of the other
 * image-side shapes (3 -> 32 k3 s2, 32 -> 32 transposed k3 s2) hand a call with add, or with tanh, to the general tile kernels.
 * ws: scratch for the split-K partial sums of small-grid layers (may be NULL: no split-K).
 * in_scale/in_shift [Ci] (both or neither; NULL = plain x): the layer reads x' = act_in(x*scale[c] + shift[c]) instead
 * of x, i.e. the BatchNorm2d + LeakyReLU in front of it (vanilla_vae.py:71-74) is applied while loading and its
 * output never touches memory.  Only where ctvae_conv_input_transform_supported() says 1 (the 3-output-channel
 * image-side layers); kErrBadArg otherwise.
 * wino_dgrad_filters_out (may be NULL): for a layer whose forward AND data gradient run Winograd
 * (ctvae_conv_wino_filter_floats() > 0, that many floats), the forward's filter-transform launch also leaves the data
 * gradient's transformed filters there; hand them to ctvae_conv_dgrad of the same layer and weights (one transform
 * launch per layer and step instead of two).
 * wino_fwd_filters (may be NULL; same size): the forward's own transformed filters made ahead of time by
 * ctvae_wino_filters_batch for the CURRENT weights -- no transform launch at all in this call. */
int ctvae_conv_forward(int kind, const float* x, const float* w, const float* bias, const float* add, float* y, int B,
                       int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int act, const float* in_scale,
                       const float* in_shift, int in_act, float* wino_dgrad_filters_out, const float* wino_fwd_filters, float* ws,
                       size_t ws_bytes, void* stream);
/* nn.Linear(Ci, C*P) followed by .view(-1, C, h, w), h*w = P (decoder_input, vanilla_vae.py:43,101-102): y is written as the
 * NHWC tensor [B, h, w, C] the next layer gathers -- output feature c*P + p goes to column p*C + c in the GEMM's epilogue, no
 * layout launch behind it.  x [B, Ci], w the packed [Ci][C*P] block, bias [C*P] or NULL.  _supported: 1 where the layer runs on
 * the vector tile kernel without a K split (Ci % 32 == 0, enough rows); elsewhere use ctvae_conv_forward + ctvae_permute.
 * Backward is unchanged: ctvae_permute / ctvae_splitk_permute of the gradient, then ctvae_conv_backward of the Linear. */
int ctvae_linear_pixmajor_supported(int B, int Ci, int C, int P, size_t ws_bytes);
int ctvae_linear_pixmajor_forward(const float* x, const float* w, const float* bias, float* y, int B, int Ci, int C, int P, int act,
                                  float* ws, size_t ws_bytes, void* stream);
/* Both Winograd filter sets (forward / data gradient, ctvae_conv_wino_filter_floats() floats each) of n 3x3 stride-1 layers
 * in ONE launch: w[l] = the layer's packed weights [9][Ci][Co], Ci, Co multiples of 32.  The residual stacks of MCQ-VAE /
 * CT-MCQ-VAE have 13 / 14 such layers (vq_vae.py:57-70 via mcq_vae.py:182-216); their weights change once per optimizer step.
 * w, fwd_filters, dgrad_filters, Ci, Co: HOST arrays of n entries (device pointers / ints). */
int ctvae_wino_filters_batch(int n, const float* const* w, float* const* fwd_filters, float* const* dgrad_filters, const int* Ci,
                             const int* Co, void* stream);
size_t ctvae_conv_wino_filter_floats(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                     size_t ws_bytes);
int ctvae_conv_input_transform_supported(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad,
                                         int out_pad);

/* Conv2d|ConvTranspose2d -> BatchNorm2d -> activation as one call (nn.Sequential blocks vanilla_vae.py:25-35,47-75):
 * y = conv(x)+bias (kept for backward); the conv epilogue emits per-tile (count, mean, M2) so the batch
 * statistics cost no extra pass over y; a_out = act(BN(y)).  Arguments as ctvae_conv_forward / ctvae_bn_forward.
 * scale_shift_out [2][Co] (may be NULL): receives the per-channel affine a = act(y*scale + shift); with a_out == NULL
 * the apply pass is skipped altogether and the consumer applies it on load (ctvae_conv_forward in_scale/in_shift).
 * in_scale / in_shift [Ci] / in_act (both NULL normally): x is itself the raw BatchNorm input of the PREVIOUS block, handed over
 * that way, and this layer reads act(x*in_scale + in_shift) -- where ctvae_conv_input_transform_supported() says 1; the chain
 * Conv -> BN -> LeakyReLU -> Conv -> BN ... (vanilla_vae.py:25-35,47-62) then runs without a stand-alone apply launch. */
/* 1 when a training call of ctvae_conv_bn_act_forward with this geometry runs BatchNorm's apply as a launch of its own (which
 * a_out == NULL + scale_shift_out saves), 0 when the activated tensor comes out of the channel-owner launch that follows a
 * split-K convolution anyway (then handing the consumer the raw tensor only costs it arithmetic). */
int ctvae_conv_bn_act_apply_is_separate(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                        size_t ws_bytes);
int ctvae_conv_bn_act_forward(int kind, const float* x, const float* w, const float* bias, const float* gamma,
                              const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                              int training, int act, float* y, float* a_out, float* save_mean, float* save_invstd,
                              float* scale_shift_out, int64_t* num_batches_tracked, int B, int H, int W, int Ci, int Co, int k,
                              int stride, int pad, int out_pad, const float* in_scale, const float* in_shift, int in_act,
                              float* ws, size_t ws_bytes, void* stream);

/* dx = (dgrad(dy, w) + add) * act'(mask)      (autograd of the ops above)
 * add / mask (saved post-activation output of the PREVIOUS layer, layout of dx) may be NULL.
 * Stride 2, CTVAE_CONV: H and W must be even (dx is written per output-parity class); an odd size is kErrBadArg, nothing launched.
 * wino_filters: NULL, or what ctvae_conv_forward left in wino_dgrad_filters_out for these weights. */
int ctvae_conv_dgrad(int kind, const float* dy, const float* w, const float* add, const float* mask, int mask_act,
                     float* dx, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                     const float* wino_filters, float* ws, size_t ws_bytes, void* stream);

/* dw (+)= wgrad(x, dy);  dbias (+)= sum over pixels of dy (dbias may be NULL).  Deterministic two-pass. */
/* in_scale/in_shift/in_act: as ctvae_conv_forward (x is then the raw BatchNorm input y of the previous block). */
int ctvae_conv_wgrad(int kind, const float* x, const float* dy, float* dw, float* dbias, int B, int H, int W, int Ci,
                     int Co, int k, int stride, int pad, int out_pad, int accumulate, const float* in_scale,
                     const float* in_shift, int in_act, const float* dy_bn_y, const float* dy_bn_coef, int dy_bn_act,
                     float* gy_out, float* bn_dgamma, float* bn_dbeta, int bn_accumulate, float* ws, size_t ws_bytes,
                     void* stream);
/* A layer's whole backward pass in one call: weight (+ bias) gradient as ctvae_conv_wgrad(x, dy -> dw, dbias) and data
 * gradient as ctvae_conv_dgrad(dy, w -> dx; optional mask, Winograd filters).  The two GEMMs are independent; when both
 * take their 64x64 tile kernels they are issued as ONE launch (conv_bwd_pair_kernel: one kernel boundary instead of two,
 * the weight-gradient workgroups start while the data gradient's stores drain), otherwise as the separate launches of
 * those entry points.  Each GEMM uses one half of ws.
 * bn_part [bn_part_rows][Ci][2] (with bn_y / bn_mean / bn_invstd / bn_gamma / bn_beta / bn_act; NULL: no BatchNorm fusion):
 * dx is the gradient w.r.t. a = act(BN(y)), the output of a train-mode BatchNorm2d (+ activation) that fed this layer (autograd of
 * vanilla_vae.py:28-31 chained into the next block), and the data gradient's epilogue also emits, per output tile, that
 * BatchNorm's backward sums (sum g', sum g'*xhat; g' = dx*act'(gamma*xhat+beta), xhat = (y-mean)*invstd), which
 * ctvae_bn_backward takes as part_in: one pass over (g_a, y) less.  bn_part_rows must equal ctvae_conv_backward_bn_rows() of
 * the same geometry and workspace; that function returns 0 when this layer's data gradient cannot emit the sums (split-K).
 * bn_coef_out [7][Ci] (may be NULL; needs bn_part): that BatchNorm's backward FINALIZE rides as extra blocks of this call's
 * finishing launch (the slab reduction) -- rows 0-4 = k1,k2,k3,scale,shift as ctvae_bn_backward's coef_out, rows 5,6 = this
 * pass's d gamma, d beta.  ctvae_bn_backward(coef_in = bn_coef_out) then only applies and commits them: one launch less per
 * Conv->BN->act->Conv link of the backward pass (vanilla_vae.py:25-35,47-62).  bn_dgamma / bn_dbeta (both or none):
 * the rider commits the parameter gradients itself (+= under bn_accumulate) -- for a caller that applies the coefficients
 * on load (ctvae_conv_wgrad dy_bn_*) and therefore never calls ctvae_bn_backward.
 * in_scale / in_shift / in_act and dy_bn_y / dy_bn_coef / dy_bn_act / gy_out: the weight gradient's options as in
 * ctvae_conv_wgrad (the layers of the final block, vanilla_vae.py:64-75); with gy_out the data gradient reads g_y from it.
 * x == bn_y with in_scale / in_shift given (they must then be that BatchNorm's scale / shift, in_act == bn_act) on the 32 -> 3
 * picture-side conv (vanilla_vae.py:73-74): ONE kernel forms the data gradient, the BatchNorm-backward sums and the weight
 * gradient in a single pass over y (image.hip img_bwd_fused_kernel). */
int ctvae_conv_backward_bn_rows(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                size_t ws_bytes);
int ctvae_conv_backward(int kind, const float* x, const float* dy, const float* w, float* dw, float* dbias, float* dx, int B,
                        int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int accumulate, const float* mask,
                        int mask_act, const float* wino_filters, const float* bn_y, const float* bn_mean,
                        const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_act, float* bn_part,
                        int bn_part_rows, float* bn_coef_out, float* bn_dgamma, float* bn_dbeta, int bn_accumulate,
                        const float* in_scale, const float* in_shift, int in_act,
                        const float* dy_bn_y, const float* dy_bn_coef, int dy_bn_act, float* gy_out, float* ws, size_t ws_bytes,
                        void* stream);

/* Small layers behind a train-mode BatchNorm (the deep encoder / decoder blocks at small batch, vanilla_vae.py:25-35,47-62): the
 * data gradient runs split-K and its consumer is that BatchNorm's backward pass, so the slices are never summed into a tensor of
 * their own.  ctvae_conv_backward_lazy_slices: the number S (>= 2) of K slices such a call would produce for this geometry and
 * workspace, or 0 when this form does not apply (unsplit / Winograd / picture-side data gradient, or a tensor beyond the few MB
 * the channel-owner kernel pays for; for_bn = 0 drops that size condition -- any split data gradient -- for consumers that take
 * the slices pixel-major, see ctvae_gauss_latent_backward / ctvae_splitk_permute).  ctvae_conv_backward_lazy (pixel_major = 0
 * for the BatchNorm consumer): weight (+ bias) gradient as ctvae_conv_backward (in_scale /
 * in_shift / in_act: its x operand read through the previous block's BatchNorm + activation, as there), and the data
 * gradient's raw slices, CHANNEL-MAJOR, in dx_slices [S][Ci][B*H*W] (no mask, no BatchNorm sums, dx itself is not written;
 * the rows of a slice are in the data gradient's class-major order, not pixel order).
 * ctvae_bn_backward_fused (kind ... out_pad: the geometry of the ctvae_conv_backward_lazy call that wrote the slices; the
 * BatchNorm's tensor is that layer's input [B,H,W,Ci]): g_y, d gamma, d beta from those slices in ONE launch -- a workgroup
 * owns 2 or 4 channels and all R = B*H*W rows: slice sum, g' = g_a * act'(gamma*xhat+beta), both reductions, the coefficients and g_y = k1*g' + k2*y + k3.
 * Replaces split-K finish + ctvae_bn_backward's partial / finalize / apply launches (reference: autograd of
 * nn.BatchNorm2d + nn.LeakyReLU). */
int ctvae_conv_backward_lazy_slices(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                    int for_bn, size_t ws_bytes);
int ctvae_conv_backward_lazy(int kind, const float* x, const float* dy, const float* w, float* dw, float* dbias, float* dx_slices,
                             int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int accumulate,
                             const float* in_scale, const float* in_shift, int in_act, int pixel_major, float* ws, size_t ws_bytes,
                             void* stream);
int ctvae_bn_backward_fused(const float* g_a_slices, int slices, int kind, int B, int H, int W, int Ci, int Co, int k, int stride,
                            int pad, int out_pad, const float* y, const float* gamma, const float* beta, const float* save_mean,
                            const float* save_invstd, int act, float* g_y, float* dgamma, float* dbeta, int accumulate, void* stream);

/* dy_bn_y / dy_bn_coef / gy_out (all or none): `dy` is then g_a, the gradient w.r.t. the output of the BatchNorm +
 * activation that follows this layer; the kernel forms g_y = k1*g_a*act'(y*scale+shift) + k2*y + k3 while loading
 * (coef = [5][Co]: k1,k2,k3,scale,shift as written by ctvae_bn_backward coef_out), uses it for dw/dbias and writes it to
 * gy_out for the ctvae_conv_dgrad call that follows: the separate BatchNorm-backward apply pass disappears.
 * Only where ctvae_conv_wgrad_bn_apply_supported() says 1 (the 32->32 transposed conv of the final block).
 * Where it says 2 (encoder.0, the 3 -> 32 picture-side conv, vanilla_vae.py:25-35 with i = 0: no data gradient follows, the
 * input is the picture) gy_out must be NULL -- g_y is used for dw/dbias and never written -- coef is the [7][Co] block of
 * ctvae_conv_backward's bn_coef_out, and bn_dgamma / bn_dbeta (both or none; += under bn_accumulate) receive its rows 5, 6:
 * the BatchNorm-backward apply launch and its 33 MB output disappear. */
int ctvae_conv_wgrad_bn_apply_supported(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad,
                                        int out_pad);

/* The final block (vanilla_vae.py:64-75: ConvTranspose2d 32->32 s2, BatchNorm2d, LeakyReLU, Conv2d 32->3 k3 p1, Tanh) without
 * the tensor g_a between its two convolutions.  g_a [B,2H,2W,32] is the picture-side conv's data gradient: a K = 27 dot product
 * of its 3-channel gradient g_pre with its weights w2 per element, written once and read once.  Instead:
 * ctvae_conv_backward_nodx: ctvae_conv_backward of the picture-side conv in its one-kernel form (x == bn_y, in_scale / in_shift of
 * that BatchNorm: image.hip img_bwd_fused_kernel) with no dx -- weight and bias gradient, the BatchNorm's backward sums in
 * bn_part and the finalize rider (bn_coef_out, bn_dgamma / bn_dbeta) as there, the same values in the same order; kErrBadArg
 * for every layer that is not that form.
 * ctvae_conv_backward_recompute / ctvae_conv_wgrad_recompute: ctvae_conv_backward / ctvae_conv_wgrad of the transposed conv
 * with dy_bn_y / dy_bn_coef / gy_out (all required) where dy is absent: the weight-gradient kernel stages g_pre [B,2H,2W,3]
 * per tile and forms g_a itself with w2 [9][32][3] (same K order as the picture-side kernel: bit-identical g_a, hence g_y, dw,
 * dbias and dx).  kind2, Co2, k2, stride2, pad2, out_pad2: the picture-side conv (its input is this layer's output).
 * Only where ctvae_conv_recompute_supported says 1 (this layer 32->32 k3 s2 p1 op1 with H % 8 == 0, W % 32 == 0; that conv 32->3
 * k3 s1 p1), else kErrBadArg. */
int ctvae_conv_recompute_supported(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int kind2,
                                   int Co2, int k2, int stride2, int pad2, int out_pad2);
int ctvae_conv_backward_nodx(int kind, const float* x, const float* dy, const float* w, float* dw, float* dbias, int B, int H,
                             int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int accumulate, const float* bn_y,
                             const float* bn_mean, const float* bn_invstd, const float* bn_gamma, const float* bn_beta, int bn_act,
                             float* bn_part, int bn_part_rows, float* bn_coef_out, float* bn_dgamma, float* bn_dbeta,
                             int bn_accumulate, const float* in_scale, const float* in_shift, int in_act, float* ws, size_t ws_bytes,
                             void* stream);
int ctvae_conv_backward_recompute(int kind, const float* x, const float* g_pre, const float* w2, const float* w, float* dw,
                                  float* dbias, float* dx, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                  int accumulate, const float* bn_y, const float* bn_mean, const float* bn_invstd,
                                  const float* bn_gamma, const float* bn_beta, int bn_act, float* bn_part, int bn_part_rows,
                                  float* bn_coef_out, float* bn_dgamma, float* bn_dbeta, int bn_accumulate, const float* in_scale,
                                  const float* in_shift, int in_act, const float* dy_bn_y, const float* dy_bn_coef, int dy_bn_act,
                                  float* gy_out, int kind2, int Co2, int k2, int stride2, int pad2, int out_pad2, float* ws,
                                  size_t ws_bytes, void* stream);
int ctvae_conv_wgrad_recompute(int kind, const float* x, const float* g_pre, const float* w2, float* dw, float* dbias, int B, int H,
                               int W, int Ci, int Co, int k, int stride, int pad, int out_pad, int accumulate, const float* in_scale,
                               const float* in_shift, int in_act, const float* dy_bn_y, const float* dy_bn_coef, int dy_bn_act,
                               float* gy_out, int kind2, int Co2, int k2, int stride2, int pad2, int out_pad2, float* ws,
                               size_t ws_bytes, void* stream);

/* Train/eval BatchNorm2d + activation on an [R=B*H*W][C] matrix (vanilla_vae.py:30-31,56-57,71-72).
 * training: batch statistics (biased var, eps), running stats updated with `momentum` and the unbiased
 * variance; save_mean/save_invstd [C] are written for the backward pass; num_batches_tracked (may be NULL) is
 * incremented on the device (nn.BatchNorm2d bookkeeping without an extra launch).
 * Shapes (ctvae_bn_forward and ctvae_bn_backward; kErrBadArg otherwise): R > 0, C % 4 == 0, and C/4 divides 256 or is a
 * multiple of it (C = 4, 8, 16, ... 1024, 2048, 3072, ...).  ws: at least (2048 * 3 + 5) * C floats, kErrWorkspace otherwise. */
int ctvae_bn_forward(const float* y, int R, int C, const float* gamma, const float* beta, float* running_mean,
                     float* running_var, float momentum, float eps, int training, int act, float* out,
                     float* save_mean, float* save_invstd, int64_t* num_batches_tracked, float* ws, size_t ws_bytes,
                     void* stream);
/* g_y from g_a (grad wrt the activated output); the activation derivative is re-derived from the sign of
 * gamma*invstd*(y-mean)+beta, so the activated tensor is not read; dgamma/dbeta (+)= ...
 * part_in/part_rows: the per-tile sums ctvae_conv_backward left in bn_part for this g_a (NULL/0: computed here).
 * coef_out [5][C] (may be NULL): k1,k2,k3,scale,shift of g_y = k1*g_a*act'(y*scale+shift) + k2*y + k3; with
 * g_y == NULL the apply pass is left to ctvae_conv_wgrad (dy_bn_*).
 * coef_in [7][C] (NULL normally; excludes part_in / coef_out, needs g_y): the finalize already ran as a rider of
 * ctvae_conv_backward(bn_coef_out) for exactly this g_a; only the apply pass runs and d gamma / d beta (rows 5,6) are
 * committed to dgamma / dbeta under `accumulate`. */
int ctvae_bn_backward(const float* g_a, const float* beta, const float* y, int R, int C, const float* gamma,
                      const float* save_mean, const float* save_invstd, int act, float* g_y, float* dgamma,
                      float* dbeta, int accumulate, const float* part_in, int part_rows, float* coef_out,
                      const float* coef_in, float* ws, size_t ws_bytes, void* stream);

/* Pairwise edge scorer of CausalTransition.graph_discovers[k] (ct_mcq_vae.py:86-95,147-151), after the separable first
 * Linear: u = x W1[:, :D]^T, v = x W1[:, D:]^T + b1 ([B,N,H] each, computed by the caller):
 *   out[b,i,j] = sigmoid(b2 + sum_h w2[h] * leaky_relu(u[b,i,h] + v[b,j,h], slope))        out [B,N,N]
 * No [B,N,N,H] tensor is ever materialised.  Backward (N <= 64): d_u, d_v [B,N,H]; d_w2_part [B][H] and d_b2_part [B]
 * are per-sample partials the caller sums over B (deterministic, no atomics).
 * per_sample = 1: w2 is [B][H] and b2 [B] -- every sample has its own scorer (the per-action discoverers of one batch in
 * ONE launch, ct_mcq_vae.py:149-151); the partials then ARE the gradients of those rows.
 * row_of [B] (per_sample only, may be NULL = the sample's own row): the row of the w2 / b2 bank sample b uses -- the bank of
 * all discoverers is then read in place, indexed by the sample's action.
 * u / v rows have stride ld (>= H), d_u / d_v rows stride ldd: they may be column blocks of one wider GEMM output / gradient.
 * No alignment is required: the N == 64 forward kernels that move float4s run only for H % 4 == 0, ld % 4 == 0 and 16-byte
 * aligned u, v and out (w2 aligned or not selects between two of them); every other call takes the any-N forward kernel. */
int ctvae_pair_mlp_forward(const float* u, const float* v, int ld, const float* w2, const float* b2, float* out, int B, int N,
                           int H, float slope, int per_sample, const int32_t* row_of, void* stream);
int ctvae_pair_mlp_backward(const float* u, const float* v, int ld, const float* w2, const float* out, const float* g_out,
                            float* d_u, float* d_v, int ldd, float* d_w2_part, float* d_b2_part, int B, int N, int H, float slope,
                            int per_sample, const int32_t* row_of, void* stream);

/* GATv2 attention scores of CausalTransition.graph_transitioner (ct_mcq_vae.py:103-114; torch_geometric GATv2Conv with
 * edge_dim=1 on dense graphs): xl, xr [B,N,H,C] = lin_l(x), lin_r(x); attr [B,N,N] edge attribute of r -> c (self loops
 * included); we, att [H,C].
 *   mode 0: out[b,h,r,c] = sum_k att[h,k] * leaky_relu(xl[b,r,h,k] + xr[b,c,h,k] + attr[b,r,c]*we[h,k], slope)
 *   mode 1: out[b,h,r,c] = sum_k att[h,k] * we[h,k] * leaky_relu'(same argument)          (d out / d attr)
 * N*N <= 4352 (N <= 65), slope < 1.  Backward (C <= 128): d_xl, d_xr [B,N,H,C]; d_att_part, d_we_part [B][H][C] are
 * per-sample partials for the caller to sum; d attr = sum_h g * (mode 1 output). */
int ctvae_gat_score(int mode, const float* xl, const float* xr, const float* attr, const float* we, const float* att, float* out,
                    int B, int N, int H, int C, float slope, void* stream);
int ctvae_gat_score_backward(const float* xl, const float* xr, const float* attr, const float* we, const float* att,
                             const float* g, float* d_xl, float* d_xr, float* d_att_part, float* d_we_part, int B, int N, int H,
                             int C, float slope, void* stream);

/* One whole GATv2Conv layer of CausalTransition.graph_transitioner (ct_mcq_vae.py:103-114; torch_geometric GATv2Conv(in, C,
 * edge_dim=1, heads=H), add_self_loops / fill_value 'mean', negative_slope = slope) on B dense graphs over the 64 LATENT
 * nodes (the appended action node has no outgoing edge and its own output is discarded, ct_mcq_vae.py:203-221, so it never
 * reaches a latent node).  xl / xr: rows [B*64] of stride ld, head slot hs at columns hs*C..; adj [B,64,64] weighted
 * adjacency (adj[b,r,c] != 0: edge r -> c); we, att, bias [H][C].  head_map [B*Hs] (or NULL: slot == head): the head whose
 * parameters slot hs of sample b uses -- _compute_y reads only head 0 and head 1+action of the last layer (:224-226).
 *   out[b,c,hs,:] = act(sum_r alpha[b,hs,r,c] * xl[b,r,hs,:] + bias[head]),  alpha = softmax over the kept sources of
 *   S[r,c] = sum_k att[k] * leaky_relu(xl[r,k] + xr[c,k] + a'[r,c]*we[k], slope);  alpha [B,Hs,64,64] is kept for backward.
 * act: 0 or 1 (nn.LeakyReLU() between the two layers).  16 <= C <= 128.
 * Backward: g_out like out; writes dS, dattr [B,Hs,64,64] (scratch the caller provides), d_xl / d_xr (rows of stride ldd),
 * per-sample partials d_bias_part / d_att_part / d_we_part [B][Hs][C] (the caller sums them per head: deterministic, no
 * atomics) and, when d_adj != NULL, d_adj [B,64,64] (+= when accumulate_dadj). */
int ctvae_gat_layer_forward(const float* xl, const float* xr, int ld, const float* adj, const float* we, const float* att,
                            const float* bias, const int32_t* head_map, float* out, int ldo, float* alpha, int B, int Hs, int C,
                            float slope, int act, void* stream);
int ctvae_gat_layer_backward(const float* xl, const float* xr, int ld, const float* adj, const float* we, const float* att,
                             const float* bias, const int32_t* head_map, const float* out, int ldo, const float* alpha,
                             const float* g_out, float* dS, float* dattr, float* d_xl, float* d_xr, int ldd, float* d_bias_part,
                             float* d_att_part, float* d_we_part, float* d_adj, int accumulate_dadj, int B, int Hs, int C,
                             float slope, int act, void* stream);

/* Grouped Linear on blocks of 64 rows per sample (the 64 latent nodes of CausalTransition): per output segment s < nseg
 * (<= 4) every sample picks one matrix of a stacked weight bank by its group id,
 *   y[b, m, s*N + n] = sum_k x[b, m, k] * W[s][group[s][b]][n][k] + bias[s][group[s][b]][n],
 * element (g, n, k) of bank s at W[s] + g*w_gstride[s] + n*ldw[s] + k, bias (may be NULL) at bias[s] + g*b_gstride[s] + n;
 * group[s] == NULL: everybody uses matrix 0 (a plain nn.Linear).  Replaces the per-group nn.Linear calls + batch splitting
 * of ct_mcq_vae.py:129-154 (graph_discovers[0] and graph_discovers[1+argmax(action)]) and the lin_l / lin_r rows of the two
 * heads of the last GATv2Conv that _compute_y reads (:224-226), without gathering weights per sample.  W / ldw / w_gstride /
 * bias / b_gstride / group are HOST arrays of nseg entries holding device pointers / ints.  K, N, ld*, strides: multiples of 4.
 * dgrad: dx[b,m,k] = sum_s sum_n dy[b,m,s*N+n] * W[s][g][n][k].
 * wgrad (one segment, columns col0..col0+N-1 of dy): dW[(g*N + n)*ldo + k] (+)= sum_{b: group[b]==g} sum_m dy[b,m,col0+n] *
 * x[b,m,k] (ldo >= K: the destination may be a column block of a wider bank), dbias[g*N + n] (+)= column sums (may be NULL);
 * batch slices meet in a fixed-order slab
 * reduction inside ws: deterministic, no atomics.  ctvae_glinear_wgrad_ws_bytes(G, N, K, B, grouped) is the exact size the
 * call needs for that batch (one slab [G][N][K+1] per batch slice; grouped = group != NULL); a smaller ws is refused with the
 * workspace error and nothing is written. */
int ctvae_glinear_forward(const float* x, int ldx, int K, int nseg, int N, const float* const* W, const int* ldw,
                          const int64_t* w_gstride, const float* const* bias, const int* b_gstride,
                          const int32_t* const* group, float* y, int ldy, int B, void* stream);
int ctvae_glinear_dgrad(const float* dy, int ldy, int nseg, int N, const float* const* W, const int* ldw,
                        const int64_t* w_gstride, const int32_t* const* group, float* dx, int ldx, int K, int B, void* stream);
size_t ctvae_glinear_wgrad_ws_bytes(int G, int N, int K, int B, int grouped);
int ctvae_glinear_wgrad(const float* x, int ldx, int K, const float* dy, int ldy, int col0, int N, const int32_t* group, int G,
                        int B, float* dW, int ldo, float* dbias, int accumulate, float* ws, size_t ws_bytes, void* stream);

/* CausalTransition._compute_adj's blend (ct_mcq_vae.py:153): out[r, j] = s0[r, j] * (1 - mask[r]) + s1[r, j] * mask[r] for
 * `rows` = B*64 rows of 64 targets (s0: discoverer 0's scores, s1: the action's discoverer, mask: the intervention mask per
 * (sample, source node)); backward: g0 = g * (1 - mask), g1 = g * mask, g_mask[r] = sum_j g * (s1 - s0). */
int ctvae_ct_blend_forward(const float* s0, const float* s1, const float* mask, float* out, long rows, void* stream);
int ctvae_ct_blend_backward(const float* g, const float* s0, const float* s1, const float* mask, float* g0, float* g1, float* g_mask,
                            long rows, void* stream);
/* PositionalEncoding.forward (ct_mcq_vae.py:33-38) on n = B*S*D elements, sd = S*D (the table pe [S][D] repeats per sample):
 * out = (x + pe) * keep * scale with keep the dropout mask (NULL: no dropout) and scale = 1/(1-p); backward g * keep * scale. */
int ctvae_ct_posenc_forward(const float* x, const float* pe, const float* keep, float scale, float* out, long n, int sd,
                            void* stream);
int ctvae_ct_posenc_backward(const float* g, const float* keep, float scale, float* g_x, long n, void* stream);
/* F.one_hot(inds, N).float() (CTMCQVAE.ct_preprocess, ct_mcq_vae.py:472-480): out [n][N], N % 4 == 0. */
int ctvae_one_hot(const int64_t* inds, long n, int N, float* out, void* stream);
/* Per-sample partial gradients into the rows of a parameter bank, in row order (deterministic, no atomics):
 * out[z][g][c] (+)= sum_{r < rows, group[r] == g} parts[z*mat_stride + r*ld + c], z < nmat, g < G, c < C; group == NULL: every
 * row belongs to group 0.  Replaces the one_hot(group)^T @ parts products behind the scorer rows of graph_discovers
 * (ct_mcq_vae.py:147-151) and the per-head vectors of the last GATv2Conv (:224-226). */
int ctvae_group_rowsum(const float* parts, long mat_stride, int nmat, int rows, int C, int ld, const int32_t* group, int G, float* out,
                       int accumulate, void* stream);

/* forward_action's regulariser (ct_mcq_vae.py:275): beta * adjacency_KL_loss(adj) + delta * graph_size_loss(graph) + epsilon *
 * positive_trial_loss(adj) (:314-323) on adj, graph [B,64,64] with the uniform draws of the KL target [B,4096] given
 * (torch.rand in :316).  forward writes part4 [B][4] = {KL_b, ||graph_b||_F, ||prod_j(1 - adj_b[i,j])||_2,
 * ckl*KL_b + cgs*||.||_F + cpt*||.||_2}; the regulariser is the sum of the last column over the batch.  backward (g_loss: device scalar) writes
 * d_adj, d_graph for ckl = beta/B, cgs = delta/B, cpt = epsilon/B; the row products' gradient uses exclusive prefix / suffix
 * products (exact when a factor is 0). */
int ctvae_ct_reg_forward(const float* adj, const float* graph, const float* uniform, float* part4, float ckl, float cgs, float cpt,
                         int B, int N, void* stream);
int ctvae_ct_reg_backward(const float* adj, const float* graph, const float* uniform, const float* part4, const float* g_loss,
                          float ckl, float cgs, float cpt, float* d_adj, float* d_graph, int B, int N, void* stream);
/* Tail of _compute_y (ct_mcq_vae.py:226-228) per node row r < R: probs[r,:] = softmax_d(y[r,0,:] * (1 - mask[r]) + y[r,1,:] *
 * mask[r]) (Hs == 2) or softmax_d(y[r,0,:]) (Hs == 1, mask unused); D <= 64.  Backward: dy like y, dmask [R] (may be NULL). */
int ctvae_ct_blend_softmax_forward(const float* y, const float* mask, float* probs, long R, int Hs, int D, void* stream);
int ctvae_ct_blend_softmax_backward(const float* g, const float* probs, const float* y, const float* mask, float* dy, float* dmask,
                                    long R, int Hs, int D, void* stream);
/* latent_CrossEntropy_loss (ct_mcq_vae.py:306-311) per node row: row_loss[r] = logsumexp_d(lp) - lp[target[r]] with
 * lp = log(max(probs, 1e-4)); the loss is the mean of row_loss.  Backward: d_probs for d loss = g_loss[0] (device scalar). */
int ctvae_ct_latent_ce_forward(const float* probs, const int64_t* target, float* row_loss, long R, int D, void* stream);
int ctvae_ct_latent_ce_backward(const float* probs, const int64_t* target, const float* g_loss, float* d_probs, long R, int D,
                                void* stream);

/* CausalTransition._compute_mask (ct_mcq_vae.py:117-127) for S == D == 64: pos = pe [S,D] * keep [B,S,D] * scale (the dropout of
 * PositionalEncoding applied to zeros; keep == NULL: eval mode), inter = sigmoid(W [action_b ; pos] + bias) with W [D][A+D]
 * (mask.0.weight), p[b,s] = sum_d x[b,s,d] * inter[b,s,d], sample = straight-through Bernoulli(p) from the exponential draws
 * expo [B,S,2] (Gumbel = -log E).  Outputs inter [B,S,D], p, sample, soft [B,S].  Backward for g = d loss / d sample: per-sample
 * partials dWp [B][A+D][D] (transposed like W^T) and dbp [B][D], which the caller sums over B (deterministic). */
int ctvae_ct_mask_forward(const float* x, const float* action, const float* pe, const float* keep, float scale, const float* W,
                          const float* bias, const float* expo, int B, int S, int D, int A, float* inter, float* p, float* sample,
                          float* soft, void* stream);
int ctvae_ct_mask_backward(const float* x, const float* action, const float* pe, const float* keep, float scale, const float* inter,
                           const float* p, const float* soft, const float* g, int B, int S, int D, int A, float* dWp, float* dbp,
                           void* stream);
/* Straight-through Bernoulli(p) like ctvae_gumbel_st_forward but from exponential draws expo [n][2] (what F.gumbel_softmax
 * draws: Gumbel = -log E) and, when weighted != NULL, also weighted = p * sample (weighted_graph, ct_mcq_vae.py:244,271).
 * Backward: gp = (g_sample + g_weighted * p) * d sample/d p + g_weighted * sample (either gradient may be NULL). */
int ctvae_ct_sample_forward(const float* p, const float* expo, float* sample, float* soft, float* weighted, long n, void* stream);
int ctvae_ct_sample_backward(const float* g_sample, const float* g_weighted, const float* p, const float* soft, const float* sample,
                             float* g_p, long n, void* stream);

/* layout change at the NCHW API boundary: to_nhwc=1: in [B,C,P] -> out [B,P,C]; 0: the inverse
 * (torch.flatten on NCHW, vanilla_vae.py:85; .view(-1,512,2,2), vanilla_vae.py:102) */
int ctvae_permute(const float* in, float* out, int B, int C, int P, int to_nhwc, void* stream);
int ctvae_act_forward(const float* in, float* out, long n, int act, void* stream);           /* mcq_vae.py:185,216 */
int ctvae_act_backward(const float* g_out, const float* out, float* g_in, long n, int act, void* stream);

/* The Gaussian latent as one node (vanilla_vae.py:85-92,107-122): heads [B][2L] holds mu | logvar (the fused fc_mu / fc_var
 * GEMM output, L % 4 == 0).  forward: z = eps*exp(0.5*logvar) + mu; eps_in given (injected noise), or NULL: N(0,1) drawn in
 * the kernel (Philox4x32-10 keyed by rng[0], stream position rng[1]; rng: two uint64 on the device) -- eps_out [B,L] keeps it
 * for backward.  backward: g_heads [B][2L] = (g_mu + g_z | g_logvar + g_z*eps*0.5*exp(0.5*logvar)) in one launch (any of the
 * three incoming gradients may be NULL = 0); rng_bump != NULL advances rng[1] by one (pass it when eps was drawn in forward). */
int ctvae_gauss_latent_forward(float* heads, const float* eps_in, const uint64_t* rng, float* eps_out, float* z, int B, int L,
                               const float* head_slices, int slices, const float* head_bias, void* stream);
int ctvae_gauss_latent_backward(const float* g_mu, const float* g_logvar, const float* g_z, const float* heads, const float* eps,
                                float* g_heads, uint64_t* rng_bump, int B, int L, int g_z_slices, void* stream);
/* Split-K results handed to an element-wise consumer as raw slices (the small-batch step: one launch less per hand-over).
 * head_slices [slices][B][2L] + head_bias [2L] (NULL normally): the fused heads are still the slices of their GEMM
 * (ctvae_conv_forward_lazy); ctvae_gauss_latent_forward sums them, writes `heads` (then an output) and goes on.
 * g_z_slices > 0: g_z is that many slices [S][B][L] of decoder_input's data gradient (ctvae_conv_backward_lazy, pixel_major).
 * ctvae_conv_forward_lazy_slices / ctvae_conv_forward_lazy: the number of K slices a forward conv of this geometry would run
 * (0: not split / not the general tile kernel) and the launch that leaves them, without bias or activation, in
 * y_slices [S][B*Ho*Wo][Co]; where _slices answers 0 there is nothing to write and ctvae_conv_forward_lazy returns kErrBadArg before
 * any launch.  ctvae_splitk_permute: out[b][c][p] = sum_s slices[s][(b*P+p)*C+c] -- the slice sum of an NHWC
 * data gradient and the NHWC -> NCHW change behind it (the .view(-1,512,2,2) of vanilla_vae.py:102, backward) in one launch. */
int ctvae_conv_forward_lazy_slices(int kind, int B, int H, int W, int Ci, int Co, int k, int stride, int pad, int out_pad,
                                   size_t ws_bytes);
int ctvae_conv_forward_lazy(int kind, const float* x, const float* w, float* y_slices, int B, int H, int W, int Ci, int Co, int k,
                            int stride, int pad, int out_pad, float* ws, size_t ws_bytes, void* stream);
int ctvae_splitk_permute(const float* slices, int n_slices, float* out, int B, int C, int P, void* stream);
/* z = eps*exp(0.5*logvar)+mu (vanilla_vae.py:115-117); mu/logvar rows may be strided (slices of one head GEMM) */
int ctvae_reparam_forward(const float* mu, long mu_row_stride, const float* logvar, long lv_row_stride, const float* eps,
                          float* z, int B, int L, void* stream);
int ctvae_reparam_backward(const float* g_z, const float* logvar, long lv_row_stride, const float* eps, float* g_mu,
                           float* g_logvar, int B, int L, void* stream);

/* out4 = {loss, mse, kld, -kld}: mse = mean((r-x)^2) (F.mse_loss, vanilla_vae.py:140, mcq_vae.py:279);
 * kld = mean_b(-0.5*sum_d(1+lv-mu^2-e^lv)) (vanilla_vae.py:143) when mu != NULL; loss = mse + M_N*kld (+ extra[0]) */
int ctvae_loss_forward(const float* recons, const float* x, long n, const float* mu, long mu_row_stride,
                       const float* logvar, long lv_row_stride, int B, int L, float M_N, const float* extra, float* out4,
                       float* ws, size_t ws_bytes, void* stream);
/* The same, and in the same pass the gradients of `loss` for a unit upstream gradient: g_recons [n] (w.r.t. the input of
 * recons_act when the reconstruction is that activation's output, as ctvae_loss_backward), g_mu / g_logvar [B][L] dense.
 * The loss value is not an operand of its own gradient, so a caller whose backward pass starts at `loss` needs no
 * ctvae_loss_backward launch (and no second read of both pictures). */
int ctvae_loss_forward_grad(const float* recons, const float* x, long n, const float* mu, long mu_row_stride, const float* logvar,
                            long lv_row_stride, int B, int L, float M_N, const float* extra, float* out4, float* g_recons,
                            float* g_mu, float* g_logvar, int recons_act, float* ws, size_t ws_bytes, void* stream);
/* recons_act (CTVAE_ACT_*; 0 = none) in the three reconstruction backward calls: recons is the OUTPUT of that activation
 * (the Tanh closing final_layer, vanilla_vae.py:74 / the decoder, mcq_vae.py:236) and g_recons is the gradient w.r.t. the
 * activation's input, g * act'(recons): the producer's activation-backward pass folded into this one. */
int ctvae_mse_backward(const float* recons, const float* x, const float* g_loss, float* g_recons, long n, int recons_act,
                       void* stream);
/* ctvae_mse_backward (or ctvae_logcosh_backward when logcosh_alpha > 0) and ctvae_kl_backward in ONE launch. */
int ctvae_loss_backward(const float* recons, const float* x, const float* g_loss, float* g_recons, long n, float logcosh_alpha,
                        const float* mu, long mu_row_stride, const float* logvar, long lv_row_stride, float* g_mu, float* g_logvar,
                        int B, int L, float M_N, int recons_act, void* stream);
/* LogCoshVAE's objective (logcosh_vae.py:141-155): out4 = {loss, rl, kld, -kld} with
 * rl = 1/alpha * mean(alpha t + log(1 + exp(-2 alpha t)) - log 2), t = recons - x; loss = rl + M_N * kld (the caller passes
 * M_N = beta * kld_weight).  Backward of the reconstruction term: g_recons = g_loss[0] * tanh(alpha t) / n; the KL term
 * uses ctvae_kl_backward. */
int ctvae_logcosh_loss_forward(const float* recons, const float* x, long n, float alpha, const float* mu, long mu_row_stride,
                               const float* logvar, long lv_row_stride, int B, int L, float M_N, float* out4, float* ws,
                               size_t ws_bytes, void* stream);
int ctvae_logcosh_backward(const float* recons, const float* x, const float* g_loss, float* g_recons, long n, float alpha,
                           int recons_act, void* stream);
int ctvae_kl_backward(const float* mu, long mu_row_stride, const float* logvar, long lv_row_stride, const float* g_loss,
                      float* g_mu, float* g_logvar, int B, int L, float M_N, void* stream);

/* Multi-codebook VQ on latents [B*HW][D]; C codebooks [K][D/C] stored back to back at `codebooks`;
 * codebook i reads channels [i, i+D/C) (reference quirk, mcq_vae.py:104,117); inds [B,C,HW] int64.
 * compute_inds: mcq_vae.py:26-39,100-110;  compute_latents: mcq_vae.py:41-64,112-127 */
int ctvae_vq_inds(const float* latents, const float* codebooks, int64_t* inds, int B, int HW, int D, int K, int C,
                  void* stream);
int ctvae_vq_lookup(const float* latents, const float* codebooks, const int64_t* inds, float* quantized, float* vq_loss,
                    float beta, int B, int HW, int D, int K, int C, float* ws, size_t ws_bytes, void* stream);
/* g_latents (may be NULL) = straight-through g_q + commitment term; d_codebooks (may be NULL) (+)= embedding term.
 * ws (may be NULL): scratch that lets the codebook pass split the positions over more workgroups (fixed-order sum). */
int ctvae_vq_backward(const float* g_quantized, const float* g_vq_loss, const float* latents, const float* codebooks,
                      const int64_t* inds, float* g_latents, float* d_codebooks, int accumulate, float beta, int B, int HW,
                      int D, int K, int C, float* ws, size_t ws_bytes, void* stream);

/* Straight-through Bernoulli(p) sample = F.gumbel_softmax(log(clamp([1-p,p],1e-4)), tau=1, hard=True)[...,1]
 * (ct_mcq_vae.py:126,177-183).  gumbel_noise [n][2] standard Gumbel draws (injectable);
 * `soft` [n] keeps the soft probability for the backward pass. */
int ctvae_gumbel_st_forward(const float* p, const float* gumbel_noise, float* sample, float* soft, long n, void* stream);
int ctvae_gumbel_st_backward(const float* g_sample, const float* p, const float* soft, float* g_p, long n, void* stream);

/* Categorical latent of CategoricalVAE (models/cat_vae.py).  rows = B * latent_dim, Q = categorical_dim (<= 256).
 * Gumbel-softmax reparameterisation (cat_vae.py:118-132): sample = softmax((logits + g) / temperature) along Q with
 * g = -log(-log(uniform + eps) + eps); `uniform` [rows][Q] are the U[0,1) draws (injectable).
 * Backward: g_logits = sample * (g_sample - sum_Q g_sample * sample) / temperature. */
int ctvae_gumbel_softmax_forward(const float* logits, const float* uniform, float* sample, long rows, int Q, float temperature,
                                 float eps, void* stream);
int ctvae_gumbel_softmax_backward(const float* g_sample, const float* sample, float* g_logits, long rows, int Q,
                                  float temperature, void* stream);
/* KL between softmax(logits) and the uniform categorical prior (cat_vae.py:147,160-167):
 * kld[0] = 1/B * sum_rows sum_Q p * (log(p + eps) - log_prior), log_prior = log(1/Q + eps) (computed by the caller in
 * double like the reference's np.log).  ws: >= 4 KiB of scratch.  Backward writes g_logits = g_kld[0] * d kld / d logits. */
int ctvae_cat_kl_forward(const float* logits, long rows, int Q, int B, float eps, float log_prior, float* kld, float* ws,
                         size_t ws_bytes, void* stream);
int ctvae_cat_kl_backward(const float* logits, const float* g_kld, float* g_logits, long rows, int Q, int B, float eps,
                          float log_prior, void* stream);

/* Importance-weighted objective of IWAE / MIWAE (models/iwae.py:126-155, models/miwae.py:130-163).  recons [R][n] are the
 * reconstructions of the R = B*M*S latent samples, row r belongs to image r / rep of x [R/rep][n] (rep = M*S; same
 * per-image layout as recons, n % 4 == 0); mu / logvar [R][L] are the (repeated) posterior parameters of each row.
 *   lp[r] = mean_n (recons - x)^2, kld[r] = -0.5 sum_d (1 + lv - mu^2 - e^lv), lw = lp + M_N*kld, w = softmax over the S
 *   consecutive rows of a group, out4 = {loss = mean_groups sum_s w*lw, mean lp, mean kld, -mean kld};
 *   coef[r] = d loss / d lw[r] (weights NOT detached, like the reference) is kept for the backward call, which writes
 *   g_recons (may be NULL) and g_mu / g_logvar (both or neither) scaled by g_loss[0]. */
int ctvae_iw_loss_forward(const float* recons, const float* x, long n, int R, int rep, const float* mu, const float* logvar,
                          int L, int S, float M_N, float* lp, float* kld, float* coef, float* out4, void* stream);
int ctvae_iw_loss_backward(const float* recons, const float* x, long n, int R, int rep, const float* mu, const float* logvar,
                           int L, float M_N, const float* coef, const float* g_loss, float* g_recons, float* g_mu,
                           float* g_logvar, void* stream);

/* SWAE's reconstruction term F.mse_loss + F.l1_loss (swae.py:121-125) in one pass: out4 = {loss, rl, 0, 0} with
 * rl = mean((r-x)^2) + mean(|r-x|), loss = rl (+ extra[0]); backward g_recons = g_loss[0] * (2 t + sign(t)) / n * act'(recons)
 * (recons_act as in ctvae_mse_backward). */
int ctvae_l2l1_loss_forward(const float* recons, const float* x, long n, const float* extra, float* out4, float* ws, size_t ws_bytes,
                            void* stream);
int ctvae_l2l1_backward(const float* recons, const float* x, const float* g_loss, float* g_recons, long n, int recons_act,
                        void* stream);
/* One rung of LVAE's top-down pass (lvae.py:166-204) on [B][D] tensors: merge_gauss of the bottom-up (mu_e, logvar_e) and the
 * top-down (mu_t, logvar_t) Gaussians, z = eps * exp(logvar/2) + mu of the merged one, kl[b] = sum_d compute_kl_divergence(merged,
 * bottom-up) as the reference writes it.  Backward: g_z [B][D] and / or g_kl [B] -> gradients of the four inputs. */
int ctvae_ladder_merge_forward(const float* mu_e, const float* logvar_e, const float* mu_t, const float* logvar_t, const float* eps,
                               int B, int D, float* z, float* kl, void* stream);
int ctvae_ladder_merge_backward(const float* g_z, const float* g_kl, const float* mu_e, const float* logvar_e, const float* mu_t,
                                const float* logvar_t, const float* eps, int B, int D, float* g_mu_e, float* g_logvar_e,
                                float* g_mu_t, float* g_logvar_t, void* stream);
/* GammaVAE (gamma_vae.py:108-193).  Reparameterisation by shape augmentation with the draw zhat ~ Gamma(alpha + gamma_shape, 1)
 * given: z = h(a, h^-1(a, zhat)) / beta, a = alpha + gamma_shape (:108-149); backward g_alpha (both partials, as autograd forms
 * them), g_beta.  KL of the Gamma posteriors to the Gamma(prior_alpha, prior_beta) prior as the reference writes it (:151-171),
 * out[0] = mean_b sum_d; g_kld one float on the device.  The final layer's nn.Sigmoid (:78) as an elementwise pair
 * (n % 4 == 0).  ws: >= 4*B bytes. */
int ctvae_gamma_reparam_forward(const float* alpha, const float* beta, const float* zhat, float gamma_shape, float* z, long n,
                                void* stream);
int ctvae_gamma_reparam_backward(const float* g_z, const float* alpha, const float* beta, const float* zhat, float gamma_shape,
                                 float* g_alpha, float* g_beta, long n, void* stream);
int ctvae_gamma_kl_forward(const float* alpha, const float* beta, int B, int D, float prior_alpha, float prior_beta, float* out,
                           float* ws, size_t ws_bytes, void* stream);
int ctvae_gamma_kl_backward(const float* g_kld, const float* alpha, const float* beta, int B, int D, float prior_alpha,
                            float prior_beta, float* g_alpha, float* g_beta, void* stream);
int ctvae_sigmoid_forward(const float* x, float* y, long n, void* stream);
int ctvae_sigmoid_backward(const float* g, const float* y, float* g_x, long n, void* stream);
/* BetaTCVAE's decomposition of the KL term (betatc_vae.py:128-199) on z, mu, logvar [B][D] (D <= 32, 2 <= B <= 4096) with the
 * log importance weights log_iw [B][B] of minibatch stratified sampling (:176-184): M[i,j,d] = log N(z_i[d]; mu_j[d], e^lv_j[d]) +
 * log_iw[i,j]; log_q_z = logsumexp_j sum_d M, log_prod = sum_d logsumexp_j M, log_q_zx / log_p_z the sample's own and the
 * standard normal log density; out3 = {mi, tc, kld} = means of (log_q_zx - log_q_z, log_q_z - log_prod, log_prod - log_p_z).
 * lse_s [B], lse_d [B][D] keep the logsumexps for the backward call; g3: d loss / d {mi, tc, kld} (3 floats on the device).
 * ws: >= 16*B bytes. */
int ctvae_tc_forward(const float* z, const float* mu, const float* logvar, const float* log_iw, int B, int D, float* out3, float* lse_s,
                     float* lse_d, float* ws, size_t ws_bytes, void* stream);
int ctvae_tc_backward(const float* z, const float* mu, const float* logvar, const float* log_iw, const float* lse_s, const float* lse_d,
                      const float* g3, int B, int D, float* g_z, float* g_mu, float* g_logvar, void* stream);
/* VampPrior KL term of VampVAE (vampvae.py:140-171): z, mu, logvar [B][D] (contiguous), prior_mu / prior_logvar [K][D] (the
 * encoder on the K pseudo-inputs, K <= 512): out3 = {kld, E_log_p, E_log_q} with E_log_q = mean_b sum_d -0.5 (lv + (z-mu)^2) /
 * e^lv, E_log_p = mean_b logsumexp_k (sum_d -0.5 (plv_k + (z - pmu_k)^2) / e^plv_k - log K), kld = -(E_log_p - E_log_q);
 * weights [B][K] receives softmax_k of the component scores for the backward call (g_kld: one float on the device).
 * ws: >= 8*B bytes. */
int ctvae_vamp_kl_forward(const float* z, const float* mu, const float* logvar, const float* prior_mu, const float* prior_logvar,
                          int B, int D, int K, float* out3, float* weights, float* ws, size_t ws_bytes, void* stream);
int ctvae_vamp_kl_backward(const float* z, const float* mu, const float* logvar, const float* prior_mu, const float* prior_logvar,
                           const float* weights, const float* g_kld, int B, int D, int K, float* g_z, float* g_mu, float* g_logvar,
                           float* g_prior_mu, float* g_prior_logvar, void* stream);
/* Sliced Wasserstein distance of SWAE (swae.py:150-178) between z and prior draws [N][D] (N <= 1024, D <= 512, D % 4 == 0) along
 * the S unit directions proj [S][D]: out[0] = weight * mean_{s,r} (sort_r(z . w_s) - sort_r(prior . w_s))^p (torch.sort + pow + mean
 * in the reference); grad_z [N][D] receives d out / d z (the backward pass scales it by the incoming gradient).
 * ws: >= 4 * (S + N*S) bytes. */
int ctvae_swd_forward(const float* z, const float* prior, const float* proj, int N, int D, int S, float p, float weight, float* out,
                      float* grad_z, float* ws, size_t ws_bytes, void* stream);

/* Maximum-mean-discrepancy regulariser of WAE_MMD / InfoVAE (wae_mmd.py:120-203, info_vae.py:150-229) between the latent
 * codes z [N][D] and prior draws [N][D] (D <= 512):  out4 = {mmd, K(p,p), K(z,z), K(p,z)},
 * mmd = w_pp*K(p,p) + w_zz*K(z,z) - 2*w_pz*K(p,z);  kind 0 (imq): K(a,b) = sum_{i != j} c / (eps + c + |a_i - b_j|^2),
 * kind 1 (rbf): K(a,b) = mean_{i,j} exp(-mean_d (a_i - b_j)^2 / c);  c = 2 * D * latent_var is passed by the caller.
 * grad_z [N][D] receives d mmd / d z (the backward pass scales it by the incoming gradient).  ws: >= 12*N bytes. */
int ctvae_mmd_forward(const float* z, const float* prior, int N, int D, int kind, float c, float eps, float w_pp, float w_zz,
                      float w_pz, float* out4, float* grad_z, float* ws, size_t ws_bytes, void* stream);

/* DIP-VAE II regulariser (dip_vae.py:147-159) on the posterior parameters mu / logvar [B][D] (row strides in floats, D <= 1024):
 * c = mu - mean over the latent dimension, cov = c^T c, v = mean of the main diagonal of exp(2*logvar) (one scalar, as the
 * reference computes it), cz = cov + v, dip = lambda_offdiag * sum_{i != j} cz_ij^2 + lambda_diag * sum_i (cz_ii - 1)^2.
 * state: ctvae_dip_state_floats(B, D) floats kept by the caller between the two calls; dip = state[B*D + D*D + 3*D].
 * Backward writes dense g_mu / g_logvar [B][D] scaled by g_dip[0]. */
size_t ctvae_dip_state_floats(int B, int D);
int ctvae_dip_forward(const float* mu, long mu_row_stride, const float* logvar, long lv_row_stride, int B, int D,
                      float lambda_diag, float lambda_offdiag, float* state, void* stream);
int ctvae_dip_backward(const float* state, const float* g_dip, float* g_mu, float* g_logvar, int B, int D, void* stream);

/* Disentanglement metrics (metrics.py) over a contiguous row-major f32 code matrix z [N][L]: 2 <= N <= 65535, 1 <= L <= 16384.
 * Anything out of range is a bad argument (-22) and launches nothing.
 * ctvae_column_moments: per column the mean, the unbiased variance (ddof = 1; f32: Welford mean merged pairwise, then sum (x - mean)^2), and the exact
 * minimum and maximum.
 * ctvae_mi_matrix: mi[l][f] = mutual information in nats between the 20-bin discretisation of column l and factor f, for
 * factors [N][F] (device, value of factor f in 0 .. sizes[f]-1) and sizes[F] (HOST memory: checked before the launch;
 * 1 <= F <= 16, 2 <= sizes[f] <= 256).  The bin of x is the number of k in 0..19 with lo + k*((hi - lo)/20) <= x, every
 * operation rounded to f32 on its own: np.digitize(x, np.histogram(x, 20)[1][:-1]) with lo / hi the column's minimum / maximum
 * (1..20; x = hi lands in 20; hi == lo is widened to lo - 0.5, hi + 0.5).  bins [N][L] (uint8) receives the bins when non-NULL.
 * ctvae_group_var_argmin: z [G][B][L] (B >= 2); per group g the active column (active[l] != 0) with the smallest
 * var_B(z[g][:, l]) / global_var[l] (unbiased variance; ties go to the lowest column): arg[g] its column index, val[g] the ratio
 * (-1 and +inf when no column is active). */
int ctvae_column_moments(const float* z, int N, int L, float* mean, float* var, float* min, float* max, void* stream);
int ctvae_mi_matrix(const float* z, const float* lo, const float* hi, const int32_t* factors, const int32_t* sizes, int N, int L,
                    int F, float* mi, uint8_t* bins, void* stream);
int ctvae_group_var_argmin(const float* z, const float* global_var, const uint8_t* active, int G, int B, int L, int32_t* arg,
                           float* val, void* stream);

/* Image grid as bytes (imagegrid.py): torchvision.utils.make_grid + save_image's byte conversion of an f32 batch x [N][C][H][W],
 * C = 1 (replicated) or 3, read in place through four element strides (>= 0; contiguous NCHW and channels_last alike).
 * xmaps = min(nrow, N), ymaps = ceil(N / xmaps), Hg = ymaps*(H+padding)+padding, Wg = xmaps*(W+padding)+padding; image k sits at
 * row (k / xmaps)*(H+padding)+padding, column (k % xmaps)*(W+padding)+padding; borders and the empty cells of the last grid row
 * hold pad_value.  out: Hg rows of 3*Wg bytes (R, G, B per pixel), or with scanlines != 0 of 1 + 3*Wg bytes, the first being
 * PNG filter type 0 -- the stream a PNG IDAT chunk deflates.  out must be 16-byte aligned and out_bytes at least the stream's
 * length rounded up to a multiple of 4; bytes past the stream's length are not written.
 * normalize != 0: v = (clamp(x, lo, hi) - lo) / max(hi - lo, 1e-5) with lo / hi = range_lo / range_hi when has_range != 0, else
 * the minimum / maximum over the whole batch (one more launch; workspace: device, 8-byte aligned, at least 2048 bytes).
 * normalize == 0: v = x.  byte = (uint8) clamp(v*255 + 0.5, 0, 255); pad_value takes the same conversion un-normalised.
 * Every operation is rounded to f32 on its own.  NaN does not enter the minimum / maximum and becomes byte 0 (torch would
 * propagate it); +-inf clamp.  A bad argument (C not 1 or 3, N / H / W / nrow < 1, padding < 0, NULL x / out, a stream of
 * 2^31 bytes or more, out or the workspace too small or misaligned) returns -22 and launches nothing. */
int ctvae_image_grid_u8(const float* x, long stride_n, long stride_c, long stride_h, long stride_w, int N, int C, int H, int W,
                        int nrow, int padding, int normalize, int has_range, float range_lo, float range_hi, float pad_value,
                        int scanlines, uint8_t* out, size_t out_bytes, float* workspace, size_t workspace_bytes, void* stream);

/* The same grid with every image scaled by its OWN range: torchvision's make_grid(normalize=True, scale_each=True), i.e. what
 * saving each picture on its own with normalize=True shows (the reference's apply_action notebook, cell 6).  Same parameters,
 * layout, byte conversion and NaN rule; image k uses lo_k / hi_k = its own minimum / maximum (an all-NaN image is all byte 0).
 * Two launches: a segmented range pass (P = min(16, ceil(C*H*W / 4096)) workgroups per image, N <= 65535; workspace: device,
 * 8-byte aligned, at least N*P*8 bytes) and the compose pass.  With has_range != 0 or normalize == 0 every image has the same
 * range and the call is ctvae_image_grid_u8 itself. */
int ctvae_image_grid_each_u8(const float* x, long stride_n, long stride_c, long stride_h, long stride_w, int N, int C, int H, int W,
                             int nrow, int padding, int normalize, int has_range, float range_lo, float range_hi, float pad_value,
                             int scanlines, uint8_t* out, size_t out_bytes, float* workspace, size_t workspace_bytes, void* stream);

/* Per-action hit counts of CT-MCQ-VAE's causal mode (rollout.py; the reference's apply_action notebook, cells 7 and 9):
 * probas [N][A] = forward_causal's action probabilities, action [N][A] = the one-hot action, counts [A][3] int32.  With V = A / 2,
 * a = argmax(action row), p = argmax(probas row), every row ADDS 1 to counts[a][0], (p == a) to counts[a][1] and
 * (p % V == a % V) to counts[a][2] -- rows, directed hits, direction-agnostic hits; successive launches accumulate, and integer
 * adds make the result independent of their order.  argmax is torch.argmax: the first maximal value wins, NaN counts as maximal
 * and the first NaN wins.  A even, 2 <= A <= 256; N == 0 is a successful no-op; N < 0, another A or a NULL pointer returns -22. */
int ctvae_action_hits(const float* probas, const float* action, int N, int A, int* counts, void* stream);

/* Per-group statistics of CT-MCQ-VAE's learned graphs (causalgraph.py: GraphStats).  One batch -- adj [B][S][S], the per-sample
 * adjacency; group [B] int32, 0 = no intervention, 1 + a = action a; mask [B][S], the intervention mask, or NULL -- is ADDED
 * into accumulators for G groups (device memory, zero before the first call):
 *   adj_sum [G][S][S] double     sum of the group's adjacencies
 *   edge_count [G][S][S] int32   rows with adj > threshold (strict; NaN does not count)
 *   mask_sum [G][S] double       sum of the group's masks          (untouched when mask is NULL)
 *   rows [G] int32               rows of the group
 *   mask_rows [G] int32          rows of the group that came with a mask (untouched when mask is NULL)
 *   skipped [1] int32            rows whose group lies outside [0, G); such a row touches nothing else
 * Every element ends up as if the rows had been added one at a time in ascending row order onto what earlier calls left
 * (float -> double conversion, then one double add per row): one owner per element, no atomics, so the result is bit-identical
 * however the rows are split into calls and from run to run.  One launch, no host synchronisation; the int32 counts hold up to
 * 2^31 - 1 rows.  Any S in 1 .. 46340 and G in 1 .. 65535; B == 0 is a successful no-op; B < 0, another S or G or a NULL pointer
 * (mask excepted) returns -22 and launches nothing. */
int ctvae_graph_accumulate(const float* adj, const int32_t* group, const float* mask, float threshold, int B, int S, int G,
                           double* adj_sum, int32_t* edge_count, double* mask_sum, int32_t* rows, int32_t* mask_rows,
                           int32_t* skipped, void* stream);

/* Latent usage of the Gaussian models (latentstats.py: LatentStats).  One batch of posterior parameters -- mu and logvar, fp32
 * [B][L], row r of each starting at mu + r * mu_pitch resp. logvar + r * logvar_pitch (pitches in floats, so the two may be the
 * column halves of one [B][2L] tensor) -- is ADDED into accumulators (device memory, zero before the first call):
 *   kl_sum [L] double       sum over rows of 0.5 * (((m*m + s2) - lv) - 1), m = mu, lv = logvar, s2 = exp(lv), all in double
 *   mu_sum [L] double       sum of m
 *   sig2_sum [L] double     sum of s2
 *   cov_sum [L][L] double   sum of m_i * m_j (the whole matrix; it is symmetric to the bit)
 *   nonfinite [L] int32     elements whose mu or logvar is NaN or +-inf (they still go into the sums)
 *   rows [1] int32          rows
 * Every element ends up as if the rows had been added one at a time in ascending row order onto what earlier calls left: one
 * owner per element, no atomics, so the result is bit-identical however the rows are split into calls and from run to run.  The
 * product of two fp32 values is exact in double: mu_sum and cov_sum equal a float64 loop on the host bit for bit; kl_sum and
 * sig2_sum differ from one by the two double exp implementations only.  One launch, no host synchronisation.  L in 1 .. 1024
 * (cov_sum is L * L doubles); B == 0 is a successful no-op that touches nothing; B < 0, another L, a pitch below L or a NULL
 * pointer returns -22 and launches nothing. */
int ctvae_latent_accumulate(const float* mu, long mu_pitch, const float* logvar, long logvar_pitch, int B, int L, double* kl_sum,
                            double* mu_sum, double* sig2_sum, double* cov_sum, int32_t* nonfinite, int32_t* rows, void* stream);

/* A Gaussian-mixture latent prior fitted by EM (latentprior.py: GaussianMixturePrior; csrc/gmm.hip).  X is fp32 [N][D] row-major,
 * 1 <= D <= 256, K components with 1 <= K <= 64; full != 0: full covariances, full == 0: diagonal ones.  The host prepares the
 * mixture (fp32 device buffers): log_w [K]; mu [K][D]; P, for full [K][D][D] the INVERSE of the lower Cholesky factor L_k of
 * Sigma_k (lower triangular; only j <= i is read), for diag [K][D] = 1 / sqrt(var); log_det_half [K] = sum_i log diag(L_k)_i.
 *
 * E step.  lp[n][k] = log_w[k] - 0.5 * |P_k (x_n - mu_k)|^2 - log_det_half[k] - 0.5 * D * log(2 pi)   (x_n - mu_k is formed in fp32
 * before the product; full: f32 MFMA tiles with a row-norm epilogue, the k order of the chain is ascending j),
 * ll[n] = m + log(sum_k exp(lp[n][k] - m)) with m = max_k lp[n][k], r[n][k] = exp(lp[n][k] - ll[n]).  Writes r [N][K] and ll [N]
 * fp32 and nonfinite [N] int32.  A row with a NaN or +-inf element gets r = 0, ll = 0 and nonfinite = 1 (else 0).  A fixed
 * summation order: the same bits from run to run.  One launch, no host synchronisation.  N == 0 is a successful no-op; N < 0,
 * another D or K or a NULL pointer returns -22 and launches nothing. */
int ctvae_gmm_estep(const float* X, int N, int D, int K, int full, const float* log_w, const float* mu, const float* P,
                    const float* log_det_half, float* r, float* ll, int32_t* nonfinite, void* stream);

/* M step: one pass over X and r [N][K] (ctvae_gmm_estep's) forms the float64 sums, centred at the CURRENT means m [K][D] fp32:
 *   Nk [K]              sum_n r[n][k]
 *   S1 [K][D]           sum_n r[n][k] (x_n - m_k)
 *   S2                  full: [K][D][D] = sum_n r[n][k] (x_n - m_k)(x_n - m_k)^T, the lower triangle mirrored into the upper;
 *                       diag: [K][D], that matrix's diagonal
 * Rows whose nonfinite [N] flag is not 0 are left out (nonfinite may be NULL: no row is).  The host finishes: mu_new = m + S1 / Nk,
 * Sigma = S2 / Nk - (mu_new - m)(mu_new - m)^T.  Nk, S1 and the diagonal of S2 are float64 throughout (the fp32 operands are
 * converted first); an off-diagonal tile of the full S2 is an fp32 MFMA sum over 256 rows at a time, added in float64 across
 * those blocks.  The rows are split into slabs, ctvae_gmm_mstep_slabs(N, D, K, full) of them, every slab summed in ascending row
 * order by one owner per element and the slabs merged in ascending order by a second launch: no atomics, the same bits from run
 * to run.  ws: ctvae_gmm_mstep_workspace_bytes(N, D, K, full) bytes of scratch, 8-byte aligned.  N < K, N < 1, another D or K or a
 * NULL pointer (nonfinite excepted) returns -22, a workspace too small -12; nothing is launched then. */
int ctvae_gmm_mstep_slabs(int N, int D, int K, int full);
size_t ctvae_gmm_mstep_workspace_bytes(int N, int D, int K, int full);
int ctvae_gmm_mstep(const float* X, const float* r, const int32_t* nonfinite, int N, int D, int K, int full, const float* m,
                    double* Nk, double* S1, double* S2, double* ws, size_t ws_bytes, void* stream);

/* Sampling: z[i][:] = mu_k + L_k eps[i][:] with k = the first index whose cdf[k] > u[i] (K - 1 when none is: a cdf whose last
 * entry rounds below 1).  u [n] fp32 in [0, 1), eps [n][D] fp32, cdf [K] double (the running sum of the weights), mu [K][D] fp32,
 * L for full [K][D][D] the lower Cholesky factors (only j <= i is read; an fp32 fma chain over ascending j), for diag [K][D] =
 * sqrt(var).  Writes z [n][D] fp32 and comp [n] int32.  The kernel holds no random state.  n == 0 is a successful no-op; n < 0,
 * another D or K or a NULL pointer returns -22 and launches nothing. */
int ctvae_gmm_sample(const float* u, const float* eps, int n, int D, int K, int full, const double* cdf, const float* mu,
                     const float* L, float* z, int32_t* comp, void* stream);

/* Reconstruction quality per image (exp_params.recon_stats; reconstats.py: ReconStats).  a (the reconstruction) and b (the target)
 * are fp32 NHWC [B][S][S][C], 11 <= S <= 64, C >= 1.  consts: 13 doubles in HOST memory, read before the call returns: the 11-tap
 * window g (Wang et al. 2004: g[t] ~ exp(-(t-5)^2 / (2 * 1.5^2)), normalised to sum 1), then C1 = (0.01 R)^2 and C2 = (0.03 R)^2
 * for the data range R, both > 0.  Image i writes row row0 + i of records [capacity][4] double and of flags [capacity] int32:
 *   records[.][0] mse   the mean over all S*S*C elements of (a - b)^2, in double
 *   records[.][1] mae   the mean of |a - b|
 *   records[.][2] max   the largest |a - b|
 *   records[.][3] ssim  the mean over the (S-10)^2 VALID window positions of every channel of
 *                       (2 mu_a mu_b + C1)(2 s_ab + C2) / ((mu_a^2 + mu_b^2 + C1)(s_aa + s_bb + C2)),
 *                       mu_x = G*x, s_xy = G*(x y) - mu_x mu_y, G = g (x) g; no padding.  Identical pictures give exactly 1.0
 *   flags[.]            1 when any element of either picture is NaN or +-inf, else 0
 * One workgroup per image, a fixed summation order, no atomics: a row's bits do not depend on B, on row0 or on the other images
 * of the batch.  One launch, no host synchronisation.  B == 0 is a successful no-op; B < 0, another S or C, row0 < 0,
 * row0 + B > capacity, a constant that is not > 0 or a NULL pointer returns -22 and launches nothing. */
int ctvae_recon_record(const float* a, const float* b, int B, int S, int C, const double* consts, double* records, int32_t* flags,
                       int row0, int capacity, void* stream);

/* The running set of the K worst images (1 <= K <= 32) behind ctvae_recon_record of the same batch.  The state is K slots --
 * ssim [K] double, row [K] int32 (the global row; -1: the slot is empty), and both pictures [K][S][S][C] fp32 -- held twice:
 * the call reads the old side and writes the new side, nothing moves in place (a pointer shared by the two sides returns -22).
 * Select (one launch): the old slots and rows [row0, row0 + B) of records whose flag is 0 are ordered by (ssim ascending, row
 * ascending) -- the rows are distinct, so ties are decided -- and the first K fill new_ssim / new_row; the slots behind the last
 * candidate are empty; source [K] int32 says where a slot comes from: j in [0, K) old slot j, K + i batch image i, -1 empty.
 * Gather (one launch): the pictures follow word for word; an empty slot's pictures are zeroed.  After any cut of a stream of
 * images into batches the state equals the first K of a sort of the whole stream. */
int ctvae_recon_worst(const double* old_ssim, const int32_t* old_row, const float* old_a, const float* old_b, const double* records,
                      const int32_t* flags, int row0, int B, int capacity, const float* batch_a, const float* batch_b, int S, int C,
                      int K, double* new_ssim, int32_t* new_row, float* new_a, float* new_b, int32_t* source, void* stream);

/* Test log-likelihood by importance sampling (exp_params.val_loglik, python -m ctvae_amd.log_likelihood; loglik.py:
 * ImportanceLogLik).  An image's K samples z_k ~ q(z|x) arrive in chunks of S: one chunk is R = B * S decoder rows, row r belongs
 * to image r / S.  Three entry points, one launch each, no atomics, no host synchronisation; the finish is the host's, in
 * float64 from one copy of the state: loglik = m + log s - log n, elbo = t / n, ess = s^2 / s2.
 *
 * Latent: mu, logvar fp32 [B][L], eps fp32 [B][S][L], any L >= 1.  Writes z fp32 [R][L], z = mu + expf(0.5f * logvar) * eps, and
 * a double [R], a[r] = log p(z) - log q(z|x) = -0.5 * sum_d (z^2 - eps^2 - logvar) -- the log 2 pi terms cancel -- formed in
 * double from the fp32 z that was stored.  One wave per row, a fixed shuffle tree.  B == 0 is a successful no-op; B < 0, S < 1,
 * L < 1 or a NULL pointer returns -22 and launches nothing. */
int ctvae_loglik_latent(const float* mu, const float* logvar, const float* eps, int B, int S, int L, float* z, double* a,
                        void* stream);

/* Rows: xhat fp32 [R][P] (the decoded rows), x fp32 [B][P] (the images), both dense and in ONE element order (the caller pairs
 * NCHW with NCHW or NHWC with NHWC; the kernel sees P elements per row).  sse[r] = sum_i ((double)xhat[r][i] - (double)x[r / S][i])^2
 * in a fixed order -- 16-byte loads when P % 4 == 0 and both base pointers are 16-byte aligned, scalar loads otherwise; the
 * two orders differ in the last bits -- then lw[r] = -sse * consts[0] - consts[1] + a[r], double [R].  consts: two doubles in
 * DEVICE memory, 1 / (2 sigma^2) and (P / 2) log(2 pi sigma^2); (1, 0) makes lw = -sse.  a: double [R], or NULL for 0.  One
 * workgroup per row.  A row's bits do not depend on B, S or the other rows.  B == 0 is a successful no-op; B < 0, S < 1, P < 1
 * or a NULL pointer (a excepted) returns -22 and launches nothing. */
int ctvae_loglik_rows(const float* xhat, const float* x, int B, int S, long P, const double* a, const double* consts, double* lw,
                      void* stream);

/* Merge: image i of the batch owns row row0 + i of state [capacity][5] double -- m (the running maximum; -inf when empty), s =
 * sum exp(lw - m), s2 = sum exp(2 (lw - m)), t = sum lw, n (the count) -- and of flags [capacity] int32.  ONE thread takes the
 * chunk's S log-weights lw[i][0..S) one at a time, in sample order; when the maximum moves, s and s2 are rescaled by exp(m - lw)
 * and its square.  No operation is contracted.  The state after K samples is therefore the same bits however they were cut
 * into chunks.  A log-weight that is NaN or +-inf sets the image's flag and is not merged.  Rows outside [row0, row0 + B) are
 * not written.  B == 0 is a successful no-op; B < 0, S < 1, row0 < 0, row0 + B > capacity or a NULL pointer returns -22 and
 * launches nothing. */
int ctvae_loglik_merge(const double* lw, int B, int S, double* state, int32_t* flags, int row0, int capacity, void* stream);

/* The Gaussian KL term with free bits and a weight that lives in device memory (exp_params.kld_free_bits / kld_schedule;
 * klcontrol.py, kernels.FreeBitsKL).  mu and logvar are fp32 [B][L] with a row pitch each, as for ctvae_latent_accumulate.
 *   t_bd = 1 + lv - m^2 - e^lv in fp32 (ctvae_loss_forward's expression);  m_d = -0.5 * (sum_b t_bd) / B, the sum in double with
 *   the rows in ascending order;  a_d = 1 if m_d > free_bits or m_d is not finite, else 0;  f_d = a_d ? m_d : free_bits;
 *   w = scale * w_dev[0] -- w_dev is DEVICE memory, read by the launch, so a captured launch follows the value it holds at replay.
 *   out[0] = w * sum_d f_d, out[1] = sum_d m_d (ctvae_loss_forward's kld), out[2] = sum_d f_d, out[3] = the number of d with a_d = 0
 *   g_mu, g_logvar (dense [B][L]; both NULL: not wanted): the gradients of out[0] for a unit upstream gradient,
 *   a_d * (w / B) * m  resp.  a_d * (w / B) * 0.5 * (e^lv - 1) -- ctvae_loss_forward_grad's expressions -- and exactly 0.0f where a_d = 0.
 * One owner thread per column and a fixed reduction tree over the columns: no atomics, the same bits from run to run and
 * between an eager and a captured launch.  One launch for L <= 128, two (the second of one workgroup) above; L in 1 .. 1024,
 * B >= 1, free_bits finite and >= 0.  ws: ctvae_freebits_workspace_bytes(L) bytes of scratch, 8-byte aligned (0: may be NULL).
 * Anything else returns -22 (-12: the workspace) and launches nothing. */
size_t ctvae_freebits_workspace_bytes(int L);
int ctvae_freebits_kl_forward_grad(const float* mu, long mu_pitch, const float* logvar, long logvar_pitch, int B, int L,
                                   const float* w_dev, float scale, float free_bits, float* out, float* g_mu, float* g_logvar,
                                   float* ws, size_t ws_bytes, void* stream);

/* values [M][H][W] f32 (contiguous) as a colour-mapped, tiled sheet (causalgraph.py: heatmap_u8): every value becomes cell x cell
 * pixels of colour table[floor(t*255 + 0.5)] with t = (clamp(v, lo, hi) - lo) / (hi - lo), every operation rounded to f32 on its
 * own (ctvae_image_grid_u8's byte conversion); NaN takes entry 0, +-inf clamp.  table: 256 x RGB bytes in HOST memory, read
 * before the call returns.  The layout is ctvae_image_grid_u8's for M images of H*cell x W*cell pixels: xmaps = min(nrow, M),
 * ymaps = ceil(M / xmaps), borders and the empty cells of the last grid row hold the colour (pad_r, pad_g, pad_b), each 0 .. 255;
 * out is Hg rows of 3*Wg bytes, or with scanlines != 0 of 1 + 3*Wg bytes led by PNG filter type 0; 16-byte aligned, out_bytes at
 * least the stream's length rounded up to a multiple of 4, bytes past the stream's length are not written.  One pass, no
 * upscaled intermediate.  A bad argument (M / H / W / cell / nrow < 1, padding < 0, hi <= lo or NaN, a colour outside 0 .. 255,
 * NULL pointers, a stream of 2^31 bytes or more, out too small or misaligned) returns -22 and launches nothing. */
int ctvae_heatmap_u8(const float* values, int M, int H, int W, float lo, float hi, int cell, int nrow, int padding, int pad_r,
                     int pad_g, int pad_b, const uint8_t* table, int scanlines, uint8_t* out, size_t out_bytes, void* stream);

/* MSSIMVAE's reconstruction loss (mssim_vae.py:182-279): 1 - prod_{i<4} (mcs_i^w_i * mssim_4^w_4) over five levels of SSIM with the
 * reference's 11-tap window (2x2 average pooling between levels), for NHWC pictures a (the reconstruction) and b [B,64,64,C].
 * window [11] and weights [5]: HOST arrays (the window as the reference builds it: exp(+(x-5)^2 / 4.5), normalised).
 * part: ctvae_mssim_part_floats(B, C) floats of scratch; loss [1]; coef [10]: d loss / d (element of the ssim / cs map) per
 * level, which ctvae_mssim_backward reads.  Backward: g_a [B,64,64,C] = g_loss[0] * d loss / d a. */
size_t ctvae_mssim_part_floats(int B, int C);
int ctvae_mssim_forward(const float* a, const float* b, const float* window, const float* weights, float* part, float* loss,
                        float* coef, int B, int C, int H, int W, void* stream);
int ctvae_mssim_backward(const float* a, const float* b, const float* window, const float* coef, const float* g_loss, float* g_a,
                         int B, int C, int H, int W, void* stream);

/* Deferred slab reductions.  A parameter gradient is not read before the optimizer step, so the finishing launch behind a
 * weight-gradient kernel (the deterministic reduction of its per-slice partial dW slabs) need not sit in the backward chain.
 * Between ctvae_defer_begin and ctvae_defer_flush (one deferral at a time per process; the calls in between may come from
 * another thread, as autograd's do), ctvae_conv_wgrad / ctvae_conv_backward write their slabs
 * into `arena` (each call behind the previous call's slabs; a call that finds less than its workspace size left, or whose
 * finishing launch carries a BatchNorm finalize, or that writes a gradient an earlier deferred call wrote, runs as usual)
 * and only record the reduction; ctvae_defer_flush issues all of them in one launch per 24 jobs.  dw / dbias of the deferred
 * calls are valid only after the flush.  `arena` must stay untouched in between. */
int ctvae_defer_begin(float* arena, size_t arena_bytes);
int ctvae_defer_flush(void* stream);

/* torch.optim.Adam step over one flat buffer (experiment.py:158-160).  state (device, ctvae_adam_state_floats() floats, 64-byte
 * aligned): [0..7] = {step, lr, beta1, beta2, eps, weight_decay, beta1^step, beta2^step}, the rest scratch (ticket counters),
 * all zero when the caller creates the state.  The call advances step inside its one launch: the workgroup that finishes
 * last writes the advanced state back. */
size_t ctvae_adam_state_floats(void);
int ctvae_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* state, long n,
                    float grad_scale, void* stream);

/* ctvae_adam_step with gradient clipping in front of it (Lightning's gradient_clip_val / gradient_clip_algorithm, 32-bit):
 * the gradient g * grad_scale (grad_scale: the DDP 1/world factor, applied before the clip) is clipped, then Adam adds the
 * weight decay to the clipped gradient and steps exactly as ctvae_adam_step does (same state, same step counter advance).
 *   CTVAE_CLIP_NORM  torch.nn.utils.clip_grad_norm_(max_norm = clip_val, norm_type = 2): total = ||g * grad_scale||_2 over
 *                    the n elements, c = clip_val / (total + 1e-6) clamped to at most 1, every gradient multiplied by c (also
 *                    when c == 1).  A NaN norm makes c and every updated element NaN; an infinite norm gives c = 0.  Two
 *                    launches: a streaming sum of squares into one partial per workgroup in `workspace`
 *                    (ctvae_grad_clip_workspace_floats() floats, device), and the Adam update, whose every workgroup merges
 *                    the partials.  The norm is bit-reproducible for a given n.  total is written to norm_out (device, one
 *                    float; may be NULL).
 *   CTVAE_CLIP_VALUE torch.nn.utils.clip_grad_value_(clip_val): clamp(g * grad_scale, -clip_val, clip_val), NaN stays NaN.
 *                    One launch; workspace and norm_out are not used (may be NULL).
 * clip_val must be > 0 (no clipping: call ctvae_adam_step). */
#define CTVAE_CLIP_NORM 0
#define CTVAE_CLIP_VALUE 1
size_t ctvae_grad_clip_workspace_floats(void);
int ctvae_adam_step_clipped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* state, long n,
                            float grad_scale, int algorithm, float clip_val, float* workspace, float* norm_out, void* stream);

/* Block-aware Adam: torch.optim.Adam's treatment of parameters WITHOUT a gradient (FlatAdam absent_grad "skip" /
 * "skip_until_first").  A block table lies over the n floats: block_lo / block_hi (device, nb sorted disjoint ranges [lo, hi),
 * 32-bit, hi <= n; floats in no range are alignment gaps and are neither read nor written), block_state (device, 4 floats
 * per block: step, beta1^step, beta2^step, seen; created as {0, 1, 1, 0}) and active (device, nb words).
 *   ctvae_adam_step_blocks  ctvae_adam_step / ctvae_adam_step_clipped (algorithm CTVAE_ADAM_NO_CLIP, CTVAE_CLIP_NORM or _VALUE; same `state`,
 *                           same arithmetic) on the blocks whose active word is non-zero, each with the bias corrections of its
 *                           own step count; every other float keeps parameter and moments bit for bit.  A 16-byte quad that
 *                           straddles a block boundary is handled float by float.  The workgroup that finishes last advances
 *                           step / beta^step of the active blocks and sets their seen word, and counts the launch in state[0].
 *                           The norm of CTVAE_CLIP_NORM runs over all n gradients: inactive blocks and gaps must hold zeros.
 *   ctvae_adam_block_flags  fills `active` in front of it (one small launch): active[b] = present[b], for a block with
 *                           hit_index[b] >= 0 (a member of a parameter bank, whose presence only the device knows) only if
 *                           hits[hit_index[b]] != 0 as well; until_first != 0: a block whose seen word is set is active
 *                           whatever else.  Clears the nhits hit words.
 *   ctvae_adam_block_flags_local / _finish  the same flags in two launches, for data-parallel training, where the caller
 *                           MAX-reduces `active` across ranks in between (a block steps on every rank iff it got a gradient
 *                           on at least one).  _local: active[b] = present[b] (and the hit word, as above), whatever the seen
 *                           word says; clears the nhits hit words.  _finish, on the reduced words in place: non-zero becomes
 *                           1, and with until_first != 0 a block whose seen word is set becomes 1.  With nothing in between
 *                           the two leave what ctvae_adam_block_flags leaves.
 *   ctvae_adam_mark_members the forward pass's side: hits[0] = 1 and hits[group[b]] = 1 for the B samples' groups (int32,
 *                           values outside [0, nhits) are ignored; B = 0: member 0 only). */
#define CTVAE_ADAM_NO_CLIP 2
int ctvae_adam_mark_members(int* hits, int nhits, const int* group, int B, void* stream);
int ctvae_adam_block_flags(const int* present, const int* hit_index, int* hits, int nhits, const float* block_state, int* active,
                           int nb, int until_first, void* stream);
int ctvae_adam_block_flags_local(const int* present, const int* hit_index, int* hits, int nhits, int* active, int nb, void* stream);
int ctvae_adam_block_flags_finish(const float* block_state, int* active, int nb, int until_first, void* stream);
int ctvae_adam_step_blocks(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* state, long n,
                           float grad_scale, int algorithm, float clip_val, float* workspace, float* norm_out,
                           const int* block_lo, const int* block_hi, float* block_state, const int* active, int nb, void* stream);

/* Gradient accumulation over the micro-batches of one optimizer step (Lightning's accumulate_grad_batches): the window's running
 * sum `acc` (n floats of the caller's) against the optimizer's slice `grads` of the flat gradient buffer, one launch:
 *   CTVAE_ACCUM_STORE   acc = grads            the first micro-batch of a window
 *   CTVAE_ACCUM_ADD     acc = acc + grads      every further one that does not end the window
 *   CTVAE_ACCUM_FINISH  grads = acc + grads    the one that ends it; acc is left as it is
 * One correctly rounded fp32 add per element with acc as the left operand, so the result depends on the values alone.  Either
 * pointer may sit at any float; 16-byte accesses are used where grads and acc have the same offset from a 16-byte boundary
 * (otherwise the range is walked float by float).  The two ranges must not overlap.  Nothing outside [0, n) is touched.
 * ctvae_grad_accumulate_pass_floats: the floats one turn of the kernel's full grid covers (a longer range wraps its loop).
 * ctvae_adam_flags_window: the same three modes on the nb int32 block-activity words of ctvae_adam_block_flags_local, a
 * launch of its own: window = active, window = max(window, active), active = max(window, active) -- a block steps at the end
 * of a window iff some micro-batch of it had a gradient for it.  The caller then runs ctvae_adam_block_flags_finish (behind
 * its reduction across ranks, if any) and ctvae_adam_step_blocks on `active`. */
#define CTVAE_ACCUM_STORE 0
#define CTVAE_ACCUM_ADD 1
#define CTVAE_ACCUM_FINISH 2
size_t ctvae_grad_accumulate_pass_floats(void);
int ctvae_grad_accumulate(float* acc, float* grads, long n, int mode, void* stream);
int ctvae_adam_flags_window(int* window, int* active, int nb, int mode, void* stream);

/* Exponential moving average of the weights (exp_params.ema_decay), on the optimizer's slice of the flat parameter buffer.
 *   ctvae_ema_update   ema = fmaf(one_minus_decay, p - ema, ema) per element, in this form only: where ema == p it stays p.  `p`
 *                      is read only.  one_minus_decay is finite and inside (0, 1); it is passed by value, so it may change from
 *                      launch to launch (a warm-up schedule).  One launch's error against the exact result is at most
 *                      2^-22 * max(|ema|, |p|) per element.  A NaN or Inf in p reaches that element's average and no other.
 *   ctvae_buffer_swap  exchanges the contents of a and b as raw 32-bit words (loads and stores only: NaN payloads and -0
 *                      survive); swapping twice is the identity bit for bit.
 * Either pointer may sit at any float; 16-byte accesses are used where both have the same offset from a 16-byte boundary
 * (otherwise the range is walked float by float).  The two ranges must not overlap.  Nothing outside [0, n) is touched.  A null
 * pointer, n <= 0, a pointer that is not 4-byte aligned, overlapping ranges or a refused one_minus_decay return the bad-argument
 * code without a launch. */
int ctvae_ema_update(float* ema, const float* p, long n, float one_minus_decay, void* stream);
int ctvae_buffer_swap(float* a, float* b, long n, void* stream);

/* Codebook usage and dead-code restarts of the vector-quantised models (exp_params.codebook_stats / codebook_restart_every).
 *   ctvae_vq_usage           counts[c][k] += the number of indices of codebook c equal to k.  `inds` is int64 [B][C][HW] (what
 *                            ctvae_vq_inds writes), `counts` int64 [C][K], `invalid` one int64 word: an index outside [0, K) adds 1
 *                            to it and is written nowhere else.  Integer atomics only: exact, independent of the order.  Covered:
 *                            1 <= K <= 512 and C * K <= 8192; everything else returns the bad-argument code without a launch.
 *                            Pointers and shape integers only: a captured launch replays correctly.
 *   ctvae_vq_usage_pass_indices   the indices one turn of that kernel's grid covers (more of them: a grid-stride loop).
 *   ctvae_vq_pool_fill       pool[0 : rows) = latents[0 : rows) as raw 32-bit words, rows = min(P, R), for NHWC latents [P][D] and a
 *                            pool [R][D]; rows behind min(P, R) are not touched.  The ranges must not overlap.
 *   ctvae_vq_usage_pool_fill both of the above in ONE launch (the first workgroups count, the others copy): what a training
 *                            forward issues, one node of a captured step instead of two.  The same arguments, checks and results.
 *   ctvae_vq_restart         for every entry i = (c, k, row) of `list` (n entries of three int64 words, on the device) and d < Dc:
 *                            codebooks[c][k][d] = pool[row][c + d] -- the offset is c, not c * Dc: the slice of the latents codebook
 *                            c is compared against -- or, with `rows` non-null, = rows[i][d] (`pool` is then not read); exp_avg and
 *                            exp_avg_sq of the same elements = 0.  codebooks / exp_avg / exp_avg_sq are [C][K][Dc], row < valid_rows
 *                            <= R, C - 1 + Dc <= D.  No other word is written; an entry outside its ranges is skipped; n = 0
 *                            launches nothing.
 *   ctvae_vq_restart_gather  rows[i][d] = pool[row_i][c_i + d]: the first half of a data-parallel restart (gather, broadcast from
 *                            rank 0, ctvae_vq_restart with `rows`). */
size_t ctvae_vq_usage_pass_indices(void);
int ctvae_vq_usage(const long* inds, long* counts, long* invalid, int B, int C, int HW, int K, void* stream);
int ctvae_vq_pool_fill(const float* latents, float* pool, long P, int D, long R, void* stream);
int ctvae_vq_usage_pool_fill(const long* inds, long* counts, long* invalid, int B, int C, int HW, int K, const float* latents,
                             float* pool, long P, int D, long R, void* stream);
int ctvae_vq_restart(const long* list, int n, const float* pool, int valid_rows, int D, const float* rows, float* codebooks,
                     float* exp_avg, float* exp_avg_sq, int C, int K, int Dc, void* stream);
int ctvae_vq_restart_gather(const long* list, int n, const float* pool, int valid_rows, int D, int C, int Dc, float* rows,
                            void* stream);

/* Exponential-moving-average codebooks of the vector-quantised models (exp_params.codebook_ema_decay; van den Oord et al. 2017,
 * appendix A.1): the codebook is the running mean of the latents assigned to each code instead of an optimizer-trained weight.
 *   ctvae_vq_ema_supported   1 when (K, C, Dc) is covered: 1 <= K <= 16384, 1 <= C <= 8, 1 <= Dc <= 256.
 *   ctvae_vq_ema_stats       the statistics of one micro-batch, ADDED to the window accumulators: acc_n[c][k] (int64 [C][K]) += the
 *                            number of positions p with inds[p][c] = k, acc_s[c][k][d] (fp32 [C][K][Dc]) += the sum over those
 *                            positions of latents[p][c + d] -- the source channel is c + d, not c * Dc + d, the slice codebook c is
 *                            compared against.  latents [P = B*HW][D] NHWC, inds int64 [B][C][HW], Dc = D / C.  Deterministic: one
 *                            owner per element, positions in a fixed order, slices of the position range go through `ws` and are
 *                            added in slice order; no float atomic.  An index outside [0, K) contributes nowhere and adds 1 to the
 *                            int64 word `invalid`; a non-finite latent is summed like any other value.  Covered: C <= 8, Dc <= 256,
 *                            D % C == 0, B * HW < 2^31 (scan form: K <= 65535); `ws` must hold at least C*K*Dc + C*K + C words.
 *                            Everything else returns an error code without a launch.  Pointers and shape integers only: a
 *                            captured launch replays correctly.  Two launches (statistics per slice, reduce).
 *   ctvae_vq_ema_update      per codebook c, with g = decay: N[c][k] = fma(g, N[c][k], fl32((1-g) * acc_n[c][k])), M likewise from
 *                            acc_s, n = sum_k N[c][k] in float64 in index order, Nt_k = fl32((N_k + eps) / (n + K eps) * n) formed
 *                            in float64, codebooks[c][k][d] = M[c][k][d] / Nt_k for EVERY code; acc_n and acc_s = 0 in the same
 *                            launch.  0 < decay < 1 and eps > 0 are by-value arguments (do not capture this launch).
 *   ctvae_vq_lookup_commit   ctvae_vq_lookup with vq_loss = sum_i beta * mse_i, the commitment term alone (the embedding term has
 *                            no one to train).  `quantized` is bit for bit ctvae_vq_lookup's; the backward pass is
 *                            ctvae_vq_backward with d_codebooks = NULL. */
int ctvae_vq_ema_supported(int K, int C, int Dc);
int ctvae_vq_ema_stats(const float* latents, const long* inds, long* acc_n, float* acc_s, long* invalid, int B, int HW, int D, int K,
                       int C, float* ws, size_t ws_bytes, void* stream);
int ctvae_vq_ema_update(float* codebooks, float* N, float* M, long* acc_n, float* acc_s, int C, int K, int Dc, float decay, float eps,
                        void* stream);
int ctvae_vq_lookup_commit(const float* latents, const float* codebooks, const int64_t* inds, float* quantized, float* vq_loss,
                           float beta, int B, int HW, int D, int K, int C, float* ws, size_t ws_bytes, void* stream);

/* Interpolated Markov prior over the code grids of the quantising models (exp_params.code_prior; codeprior.py).  An image is
 * int64 codes i[c][h][w] in [0, K); tokens are ordered raster over (h, w), codebooks innermost.  p(k | context) =
 * sum_j lambda[c][j] P_j(k | row_j) over J = 5 experts in this order: uniform (1/K), position (row h*W + w of pos[C][H*W][K]),
 * left (row i[c][h][w-1] of left[C][K+1][K], the boundary row K when w = 0), up (i[c][h-1][w], K when h = 0; up[C][K+1][K]),
 * previous codebook (i[c-1][h][w], K when c = 0; prev[C][K+1][K]).  P_j(k | row) = count[row][k] / total[row]; a row whose
 * total is 0 is 1/K.  The tables and their row totals (pos_tot[C][H*W], left_tot / up_tot / prev_tot [C][K+1]) are int64,
 * lambda is float64 [C][5].  Covered: 1 <= K <= 512, C, H, W >= 1, at most 2^31 - 1 tokens per launch; totals below 2^53 (the
 * caller's to check).  Everything else returns the bad-argument code without a launch.  Pointers and shape integers only.
 *   ctvae_code_prior_count   adds every token of inds [B][C][H][W] to the four tables.  Integer atomics only: exact,
 *                            independent of the order; two calls accumulate.  A token whose own code or any context code lies
 *                            outside [0, K) adds 1 to the int64 word `invalid` and is written nowhere else.
 *   ctvae_code_prior_score   logp[b][c] = sum of log p over the tokens of codebook c of image b, resp[b][c][j] = sum of the
 *                            responsibilities r_j = lambda_j P_j / p over the same tokens (float64), bad[b] (int32) = 1 when the
 *                            image holds an index outside [0, K): its logp and resp are then zeros.  One workgroup per image,
 *                            float64 throughout, a fixed order of additions and no float atomic: a row's result does not depend
 *                            on the batch it arrived in.
 *   ctvae_code_prior_sample  inds [n][C][H][W] by ancestral sampling from u float64 [n][H*W][C][2] (16-byte aligned): per token,
 *                            the expert is the smallest j with u1 < lambda[c][0] + ... + lambda[c][j] (added left to right; J-1
 *                            when none); expert 0 or a row of total 0 gives min(K-1, floor(u2 * K)); otherwise t =
 *                            min(total-1, floor(u2 * (double)total)) and the code is the smallest whose inclusive cumulative
 *                            count exceeds t.  One multiplication per decision, nothing to contract: a float64 restatement
 *                            gives the same integers.  One wavefront per image; W * C <=
 *                            ctvae_code_prior_sample_max_history() (the row of context codes it keeps in LDS).
 *   ctvae_code_prior_embed   out[n][h][w][c*Dc + d] = codebooks[c][inds[n][c][h][w]][d] as raw 32-bit words (codebooks [C][K][Dc]
 *                            back to back, out fp32 NHWC [n][H][W][C*Dc]); an index outside [0, K) gives zeros. */
int ctvae_code_prior_sample_max_history(void);
int ctvae_code_prior_count(const long* inds, long* pos, long* left, long* up, long* prev, long* invalid, int B, int C, int H, int W,
                           int K, void* stream);
int ctvae_code_prior_score(const long* inds, const long* pos, const long* left, const long* up, const long* prev,
                           const long* pos_tot, const long* left_tot, const long* up_tot, const long* prev_tot, const double* lambda,
                           double* logp, double* resp, int* bad, int B, int C, int H, int W, int K, void* stream);
int ctvae_code_prior_sample(const long* pos, const long* left, const long* up, const long* prev, const long* pos_tot,
                            const long* left_tot, const long* up_tot, const long* prev_tot, const double* lambda, const double* u,
                            long* inds, int n, int C, int H, int W, int K, void* stream);
int ctvae_code_prior_embed(const long* inds, const float* codebooks, float* out, int n, int C, int H, int W, int K, int Dc,
                           void* stream);

/* Gradient tracking: per-parameter norms and 64-bin histograms from the flat gradient buffer (Lightning's track_grad_norm, wandb's
 * watch).  `grads` (n floats) is read only.  A segment is five 64-bit words (base, rows, period, col_lo, width) and names the
 * elements base + r * period + col_lo + c, r < rows, c < width (a contiguous parameter: one row; the heads of a grouped Linear
 * block: column ranges of its rows).  The caller cuts every segment's rows * width elements (row-major) into chunks of
 * ctvae_grad_segment_chunk_floats() elements: chunk k covers the elements from chunk_first[k] on of segment chunk_seg[k], the
 * chunks of segment s are seg_chunk_begin[s] .. seg_chunk_begin[s + 1] - 1 (nseg + 1 words, every segment has at least one).
 * All tables are device memory.  The kernels work on v = fl32(grads * scale).
 *   ctvae_grad_segment_stats  two launches.  One workgroup per chunk writes a partial (part_sum: nchunks doubles, part_f:
 *       3 * nchunks floats, part_bad: nchunks words), one workgroup per segment merges them in index order:
 *       out_sum[2 s] = sum |v|^norm_type over ALL elements, in double (norm_type > 0; 2 and 1 without pow; +inf: left 0),
 *       out_sum[2 s + 1] = max |v| (NaN once an element is NaN), out_range[2 s], [2 s + 1] = min, max over the FINITE elements
 *       (-0 orders below +0; +inf, -inf when there is none), out_bad[s] = the number of non-finite elements, out_hist[64 s ..]
 *       = 0.  No floating-point atomics: the results depend on the values and the tables alone.  The nflags words of flags_in
 *       (e.g. ctvae_adam_step_blocks' active words; may be NULL with nflags 0) are copied to flags_out.
 *   ctvae_grad_segment_hist   one launch behind it: out_hist[64 s + b] += the number of finite elements of segment s in bin
 *       b = min((long)((v - lo) / (hi - lo) * 64.0f), 63), in fp32 with a correctly rounded division -- torch.histc's rule on
 *       the CPU -- where lo, hi = out_range[2 s], [2 s + 1], widened to lo - 1, hi + 1 when equal; a quotient that is not a
 *       number counts in bin 0; a segment without a finite element keeps its zeros.
 * Nothing but the part_* and out_* arrays and flags_out is written. */
size_t ctvae_grad_segment_chunk_floats(void);
int ctvae_grad_segment_stats(const float* grads, long n, float scale, float norm_type, const long* segments, int nseg,
                             const int* chunk_seg, const long* chunk_first, const int* seg_chunk_begin, int nchunks,
                             double* part_sum, float* part_f, int* part_bad, double* out_sum, float* out_range, int* out_bad,
                             int* out_hist, const int* flags_in, int* flags_out, int nflags, void* stream);
int ctvae_grad_segment_hist(const float* grads, long n, float scale, const long* segments, int nseg, const int* chunk_seg,
                            const long* chunk_first, int nchunks, const float* out_range, int* out_hist, void* stream);

/* Input side: the reference's per-sample pipeline ToTensor -> CenterCrop(crop) -> Resize(size)
 * (dataset.py:72-80; bilinear, align_corners=False, no antialias -- what transforms.Resize does to a tensor; images smaller
 * than the crop are zero-padded as torchvision's center_crop does) for a batch of rows of a uint8 dataset
 * images[N][H][W][3] resident in HBM.  rows[B] int64 (out-of-range rows give zeros); out[B][size][size][3] fp32 NHWC. */
int ctvae_crop_resize_u8(const uint8_t* images, const int64_t* rows, float* out, int B, int N, int H, int W, int crop, int size,
                         void* stream);

/* 3x3 / stride-1 / pad-1 layers with at least 64 channels run Winograd F(2x2,3x3) (forward, data gradient) and
 * F(3x3,2x2) (weight and bias gradient) instead of the direct tap-GEMM (csrc/wino.hip): 2.25x fewer MFMA
 * operations, results within a few 1e-6 of the direct kernels.  This switch (default on) selects the direct kernels
 * for A/B parity checks.  Returns the previous setting. */
int ctvae_winograd_enable(int on);

/* Measurement aid (bench.py roofline leg): when enabled every launcher brackets its kernels with HIP events
 * on the launch stream.  ctvae_prof_report synchronises them and writes one line per kernel name
 * "name\tcount\ttotal_ms\talgorithmic_flops\talgorithmic_bytes"; returns the buffer size needed.  Must be off
 * during hipGraph capture. */
void ctvae_prof_enable(int on);
void ctvae_prof_calibrate(void* stream, int n); /* n empty event pairs, reported as "(empty event pair)" */
size_t ctvae_prof_report(char* buf, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* CTVAE_HIP_H */
