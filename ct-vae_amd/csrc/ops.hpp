// Plain-pointer launchers behind the entry points of api.hip, outside the convolution path (convpaths.hpp): losses,
// latents, the causal-transition ops, optimizer, metrics, reports.  Grouped by the file that defines them; each of those
// files includes this header, so a definition that drifts from its declaration does not compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace ctvae {

// acteval.hip
int launch_action_hits(const float* probas, const float* action, int N, int A, int* counts, hipStream_t st);

// catlatent.hip
size_t cat_kl_workspace_floats();
int launch_gumbel_softmax_fwd(const float* z, const float* u, float* s, long rows, int Q, float temp, float eps, hipStream_t st);
int launch_gumbel_softmax_bwd(const float* gs, const float* s, float* gz, long rows, int Q, float temp, hipStream_t st);
int launch_cat_kl_fwd(const float* logits, long rows, int Q, int B, float eps, float c, float* out, float* ws, size_t ws_bytes,
                      hipStream_t st);
int launch_cat_kl_bwd(const float* logits, const float* go, float* gq, long rows, int Q, int B, float eps, float c, hipStream_t st);

// ctmisc.hip
int launch_ct_blend_forward(const float* s0, const float* s1, const float* mask, float* out, long rows, hipStream_t st);
int launch_ct_blend_backward(const float* g, const float* s0, const float* s1, const float* mask, float* g0, float* g1, float* gm,
                             long rows, hipStream_t st);
int launch_ct_posenc_forward(const float* x, const float* pe, const float* keep, float scale, float* out, long n, int sd,
                             hipStream_t st);
int launch_ct_posenc_backward(const float* g, const float* keep, float scale, float* gx, long n, hipStream_t st);
int launch_one_hot(const long long* inds, long n, int N, float* out, hipStream_t st);
int launch_group_rowsum(const float* parts, long mat_stride, int nmat, int rows, int C, int ld, const int* grp, int G, float* out,
                        int accumulate, hipStream_t st);
int launch_ct_reg_forward(const float* adj, const float* graph, const float* uni, float* part, float ckl, float cgs, float cpt,
                          int B, int N, hipStream_t st);
int launch_ct_reg_backward(const float* adj, const float* graph, const float* uni, const float* part, const float* g_loss,
                           float ckl, float cgs, float cpt, float* d_adj, float* d_graph, int B, int N, hipStream_t st);
int launch_ct_blend_softmax_forward(const float* y, const float* mask, float* probs, long R, int Hs, int D, hipStream_t st);
int launch_ct_blend_softmax_backward(const float* g, const float* probs, const float* y, const float* mask, float* dy, float* dmask,
                                     long R, int Hs, int D, hipStream_t st);
int launch_ct_latent_ce_forward(const float* probs, const long long* target, float* row_loss, long R, int D, hipStream_t st);
int launch_ct_latent_ce_backward(const float* probs, const long long* target, const float* g_loss, float* d_probs, long R, int D,
                                 hipStream_t st);
int launch_ct_mask_forward(const float* x, const float* action, const float* pe, const float* keep, float scale, const float* W,
                           const float* bias, const float* expo, int B, int S, int D, int A, float* inter, float* p, float* sample,
                           float* soft, hipStream_t st);
int launch_ct_mask_backward(const float* x, const float* action, const float* pe, const float* keep, float scale,
                            const float* inter, const float* p, const float* soft, const float* g, int B, int S, int D, int A,
                            float* dWp, float* dbp, hipStream_t st);
int launch_ct_sample_forward(const float* p, const float* expo, float* out, float* soft, float* weighted, long n, hipStream_t st);
int launch_ct_sample_backward(const float* gs, const float* gw, const float* p, const float* soft, const float* sample, float* gp,
                              long n, hipStream_t st);

// dataio.hip
int launch_crop_resize_u8(const unsigned char* img, const long long* rows, float* out, int B, int N, int H, int W, int crop,
                          int S, hipStream_t st);

// dip.hip
size_t dip_state_floats(int B, int D);
int launch_dip_forward(const float* mu, long mu_rs, const float* lv, long lv_rs, int B, int D, float l_diag, float l_off,
                       float* state, hipStream_t st);
int launch_dip_backward(const float* state, const float* go, float* g_mu, float* g_lv, int B, int D, hipStream_t st);

// disent.hip
int launch_column_moments(const float* z, int N, int L, float* mean, float* var, float* mn, float* mx, hipStream_t st);
int launch_mi_matrix(const float* z, const float* lo, const float* hi, const int32_t* factors, const int32_t* sizes, int N, int L,
                     int F, float* mi, uint8_t* bins, hipStream_t st);
int launch_group_var_argmin(const float* z, const float* gvar, const uint8_t* active, int G, int B, int L, int32_t* arg, float* val,
                            hipStream_t st);

// ema.hip
int launch_ema_update(float* ema, const float* p, long n, float one_minus_decay, hipStream_t st);
int launch_buffer_swap(float* a, float* b, long n, hipStream_t st);

// gamma.hip
int launch_gamma_reparam_forward(const float* alpha, const float* beta, const float* zhat, float shape_b, float* z, long n, hipStream_t st);
int launch_gamma_reparam_backward(const float* g, const float* alpha, const float* beta, const float* zhat, float shape_b, float* ga,
                                  float* gb, long n, hipStream_t st);
int launch_gamma_kl_forward(const float* alpha, const float* beta, int B, int D, float prior_alpha, float prior_beta, float* out,
                            float* ws, size_t ws_bytes, hipStream_t st);
int launch_gamma_kl_backward(const float* g, const float* alpha, const float* beta, int B, int D, float prior_alpha, float prior_beta,
                             float* ga, float* gb, hipStream_t st);
int launch_sigmoid(const float* x_or_g, const float* y, float* out, long n, int backward, hipStream_t st);

// gat.hip
int launch_gat_score(int mode, const float* xl, const float* xr, const float* attr, const float* we, const float* att, float* out,
                     int B, int N, int H, int C, float slope, hipStream_t st);
int launch_gat_score_backward(const float* xl, const float* xr, const float* attr, const float* we, const float* att,
                              const float* g, float* dxl, float* dxr, float* datt_part, float* dwe_part, int B, int N, int H,
                              int C, float slope, hipStream_t st);

// gmm.hip
int launch_gmm_estep(const float* X, int N, int D, int K, int full, const float* log_w, const float* mu, const float* P,
                     const float* ldh, float* r, float* ll, int* nonfinite, hipStream_t st);
int gmm_mstep_slabs(int N, int D, int K, int full);
size_t gmm_mstep_workspace_bytes(int N, int D, int K, int full);
int launch_gmm_mstep(const float* X, const float* r, const int* nonfinite, int N, int D, int K, int full, const float* m, double* Nk,
                     double* S1, double* S2, double* ws, size_t ws_bytes, hipStream_t st);
int launch_gmm_sample(const float* u, const float* eps, int n, int D, int K, int full, const double* cdf, const float* mu,
                      const float* L, float* z, int* comp, hipStream_t st);

// gradaccum.hip
size_t grad_accumulate_pass_floats();
int launch_grad_accumulate(float* acc, float* g, long n, int mode, hipStream_t st);
int launch_adam_flags_window(int* window, int* active, int nb, int mode, hipStream_t st);

// gradstat.hip
size_t grad_segment_chunk_floats();
int launch_grad_segment_stats(const float* g, long n, float scale, float p, const long* seg, int nseg, const int* chunk_seg,
                              const long* chunk_first, const int* seg_chunk_begin, int nchunks, double* part_sum, float* part_f,
                              int* part_bad, double* out_sum, float* out_range, int* out_bad, int* out_hist, const int* flags_in,
                              int* flags_out, int nflags, hipStream_t st);
int launch_grad_segment_hist(const float* g, long n, float scale, const long* seg, int nseg, const int* chunk_seg,
                             const long* chunk_first, int nchunks, const float* out_range, int* out_hist, hipStream_t st);

// graphstat.hip
int launch_graph_accumulate(const float* adj, const int* group, const float* mask, float thr, int B, int S, int G, double* adj_sum,
                            int* edge_count, double* mask_sum, int* rows, int* mask_rows, int* skipped, hipStream_t st);
int launch_heatmap_u8(const float* values, int M, int H, int W, float lo, float hi, int cell, int nrow, int pad, int pad_r, int pad_g,
                      int pad_b, const uint8_t* table, int scanlines, uint8_t* out, size_t out_bytes, hipStream_t st);

// imggrid.hip
size_t image_grid_workspace_bytes();
int launch_image_grid_u8(const float* x, long sN, long sC, long sH, long sW, int N, int C, int H, int W, int nrow, int pad,
                         int normalize, int has_range, float lo, float hi, float pad_value, int scanlines, uint8_t* out,
                         size_t out_bytes, float* ws, size_t ws_bytes, hipStream_t st);
int launch_image_grid_each_u8(const float* x, long sN, long sC, long sH, long sW, int N, int C, int H, int W, int nrow, int pad,
                              int normalize, int has_range, float lo, float hi, float pad_value, int scanlines, uint8_t* out,
                              size_t out_bytes, float* ws, size_t ws_bytes, hipStream_t st);

// iwloss.hip
int launch_iw_loss_forward(const float* recons, const float* x, long n, int R, int rep, const float* mu, const float* lv, int L,
                           int S, float M_N, float* lp, float* kld, float* coef, float* out4, hipStream_t st);
int launch_iw_loss_backward(const float* recons, const float* x, long n, int R, int rep, const float* mu, const float* lv, int L,
                            float M_N, const float* coef, const float* go, float* g_recons, float* g_mu, float* g_lv,
                            hipStream_t st);

// klfloor.hip
size_t freebits_workspace_bytes(int L);
int launch_freebits_kl(const float* mu, long mu_pitch, const float* lv, long lv_pitch, int B, int L, const float* w_dev, float scale,
                       float lambda, float* out4, float* g_mu, float* g_lv, float* ws, size_t ws_bytes, hipStream_t st);

// ladder.hip
int launch_ladder_forward(const float* mu_e, const float* lv_e, const float* mu_t, const float* lv_t, const float* eps, int B, int D,
                          float* z, float* kl, hipStream_t st);
int launch_ladder_backward(const float* gz, const float* gkl, const float* mu_e, const float* lv_e, const float* mu_t, const float* lv_t,
                           const float* eps, int B, int D, float* g_mu_e, float* g_lv_e, float* g_mu_t, float* g_lv_t, hipStream_t st);

// latentstat.hip
int launch_latent_accumulate(const float* mu, long mu_pitch, const float* logvar, long lv_pitch, int B, int L, double* kl_sum,
                             double* mu_sum, double* sig2_sum, double* cov_sum, int* nonfinite, int* rows, hipStream_t st);

// loglik.hip
int launch_loglik_latent(const float* mu, const float* lv, const float* eps, int B, int S, int L, float* z, double* a,
                         hipStream_t st);
int launch_loglik_rows(const float* xhat, const float* x, int B, int S, long P, const double* a, const double* consts, double* lw,
                       hipStream_t st);
int launch_loglik_merge(const double* lw, int B, int S, double* state, int* flag, int row0, int capacity, hipStream_t st);

// loss.hip.  logcosh_alpha: > 0 the log-cosh reconstruction term with that alpha, 0 the squared error, < 0 the squared +
// absolute error term (ctvae_l2l1_loss_forward).  ract: the activation whose OUTPUT r is (CTVAE_ACT_*; 0 = none) -- gr is
// then the gradient w.r.t. that activation's input.  g_r / g_mu / g_lv (null: not wanted): the gradients of the loss for a
// unit upstream gradient, formed in the same pass (ctvae_loss_forward_grad)
size_t loss_workspace_floats();
int launch_loss_forward(const float* r, const float* x, long n, const float* mu, long mu_rs, const float* lv, long lv_rs,
                        int B, int L, float M_N, const float* extra, float* out4, float* ws, size_t ws_bytes,
                        hipStream_t st, float logcosh_alpha, float* g_r = nullptr, float* g_mu = nullptr, float* g_lv = nullptr,
                        int ract = 0);
int launch_mse_backward(const float* r, const float* x, const float* go, float* gr, long n, hipStream_t st, float logcosh_alpha,
                        int ract = 0);
int launch_kl_backward(const float* mu, long mu_rs, const float* lv, long lv_rs, const float* go, float* gmu, float* glv,
                       int B, int L, float M_N, hipStream_t st);
int launch_loss_backward(const float* r, const float* x, const float* go, float* gr, long n, float logcosh_alpha, const float* mu,
                         long mu_rs, const float* lv, long lv_rs, float* gmu, float* glv, int B, int L, float M_N, hipStream_t st,
                         int ract = 0);

// mmd.hip
size_t mmd_workspace_floats(int N);
int launch_mmd_forward(const float* z, const float* p, int N, int D, int kind, float c, float eps, float w_pp, float w_zz,
                       float w_pz, float* out4, float* grad, float* ws, size_t ws_bytes, hipStream_t st);

// pairmlp.hip
int launch_pair_mlp_forward(const float* u, const float* v, int ld, const float* w2, const float* b2, float* out, int B, int N,
                            int H, float slope, int per_sample, const int* row_of, hipStream_t st);
int launch_pair_mlp_backward(const float* u, const float* v, int ld, const float* w2, const float* out, const float* g_out,
                             float* dU, float* dV, int ldd, float* dw2_part, float* db2_part, int B, int N, int H, float slope,
                             int per_sample, const int* row_of, hipStream_t st);

// pointwise.hip
int launch_permute(const float* in, float* out, int B, int C, int P, int to_nhwc, hipStream_t st);
int launch_act_bwd(const float* gout, const float* out, float* gin, long n, int act, hipStream_t st);
int launch_act_fwd(const float* in, float* out, long n, int act, hipStream_t st);
int launch_reparam_fwd(const float* mu, long mu_rs, const float* lv, long lv_rs, const float* eps, float* z, int B, int L,
                       hipStream_t st);
int launch_reparam_bwd(const float* gz, const float* lv, long lv_rs, const float* eps, float* gmu, float* glv, int B, int L,
                       hipStream_t st);
int launch_gumbel_fwd(const float* p, const float* noise, float* out, float* soft, long n, hipStream_t st);
int launch_gumbel_bwd(const float* go, const float* p, const float* soft, float* gp, long n, hipStream_t st);
size_t adam_state_floats();
int launch_adam(float* p, const float* g, float* m, float* v, float* state, long n, float grad_scale, hipStream_t st);
size_t grad_clip_workspace_floats();
int launch_adam_clipped(float* p, const float* g, float* m, float* v, float* state, long n, float grad_scale, int algorithm,
                        float clip, float* ws, float* norm_out, hipStream_t st);
int launch_adam_mark_members(int* hits, int nhits, const int* group, int B, hipStream_t st);
int launch_adam_block_flags(const int* present, const int* hit_index, int* hits, int nhits, const float* bstate, int* active,
                            int nb, int until_first, hipStream_t st);
int launch_adam_block_flags_local(const int* present, const int* hit_index, int* hits, int nhits, int* active, int nb,
                                  hipStream_t st);
int launch_adam_block_flags_finish(const float* bstate, int* active, int nb, int until_first, hipStream_t st);
int launch_adam_blocks(float* p, const float* g, float* m, float* v, float* state, long n, float grad_scale, int algorithm,
                       float clip, float* ws, float* norm_out, const int* blk_lo, const int* blk_hi, float* bstate,
                       const int* active, int nb, hipStream_t st);
int launch_gauss_latent_fwd(float* heads, const float* eps_in, const unsigned long long* rng, float* eps_out, float* z, int B,
                            int L, hipStream_t st, const float* slices, int S, const float* bias);
int launch_gauss_latent_bwd(const float* g_mu, const float* g_lv, const float* g_z, const float* heads, const float* eps,
                            float* g_heads, unsigned long long* rng_bump, int B, int L, hipStream_t st, int gz_slices);
int launch_splitk_permute(const float* slices, int S, float* out, int B, int C, int P, hipStream_t st);

// reconstat.hip
int launch_recon_record(const float* a, const float* b, int B, int S, int C, const double* consts, double* rec, int* flag, int row0,
                        int capacity, hipStream_t st);
int launch_recon_worst(const double* old_ssim, const int* old_row, const float* old_a, const float* old_b, const double* rec,
                       const int* flag, int row0, int B, int capacity, const float* bat_a, const float* bat_b, int S, int C, int K,
                       double* new_ssim, int* new_row, float* new_a, float* new_b, int* src, hipStream_t st);

// ssim.hip
int launch_ssim_forward(const float* a, const float* b, const float* window, float* part, float* loss, float* coef, int B, int C, int H,
                        int W, const float* weights, hipStream_t st);
int launch_ssim_backward(const float* a, const float* b, const float* window, const float* coef, const float* g_loss, float* g_a, int B,
                         int C, int H, int W, hipStream_t st);

// swd.hip
int launch_swd_forward(const float* z, const float* prior, const float* proj, int N, int D, int S, float p, float weight, float* out,
                       float* grad_z, float* ws, size_t ws_bytes, hipStream_t st);

// tcvae.hip
int launch_tc_forward(const float* z, const float* mu, const float* lv, const float* liw, int B, int D, float* out3, float* lse_s,
                      float* lse_d, float* ws, size_t ws_bytes, hipStream_t st);
int launch_tc_backward(const float* z, const float* mu, const float* lv, const float* liw, const float* lse_s, const float* lse_d,
                       const float* g3, int B, int D, float* dz, float* dmu, float* dlv, hipStream_t st);

// vamp.hip
int launch_vamp_forward(const float* z, const float* mu, const float* lv, const float* pmu, const float* plv, int B, int D, int K,
                        float* out3, float* wgt, float* ws, size_t ws_bytes, hipStream_t st);
int launch_vamp_backward(const float* z, const float* mu, const float* lv, const float* pmu, const float* plv, const float* wgt,
                         const float* g, int B, int D, int K, float* dz, float* dmu, float* dlv, float* dpmu, float* dplv,
                         hipStream_t st);

// vq.hip
size_t vq_workspace_floats(int C);
int launch_vq_inds(const float* lat, const float* cb, long long* inds, int B, int HW, int D, int K, int C, hipStream_t st);
int launch_vq_lookup(const float* lat, const float* cb, const long long* inds, float* out, float* vq_loss, float beta, int B,
                     int HW, int D, int K, int C, float* ws, size_t ws_bytes, hipStream_t st);
int launch_vq_lookup_commit(const float* lat, const float* cb, const long long* inds, float* out, float* vq_loss, float beta, int B,
                            int HW, int D, int K, int C, float* ws, size_t ws_bytes, hipStream_t st);
int launch_vq_backward(const float* gq, const float* gvq, const float* lat, const float* cb, const long long* inds,
                       float* glat, float* dcb, int accumulate, float beta, int B, int HW, int D, int K, int C, float* ws,
                       size_t ws_bytes, hipStream_t st);

// vqema.hip
int vq_ema_supported(int K, int C, int Dc);
int launch_vq_ema_stats(const float* lat, const long* inds_, long* acc_n, float* acc_s, long* invalid, int B, int HW, int D, int K,
                        int C, float* ws, size_t ws_bytes, hipStream_t st);
int launch_vq_ema_update(float* cb, float* N, float* M, long* acc_n, float* acc_s, int C, int K, int Dc, float decay, float eps,
                         hipStream_t st);

// codeprior.hip
int code_prior_sample_max_history();
int launch_code_prior_count(const long* inds, long* pos, long* left, long* up, long* prev, long* invalid, int B, int C, int H, int W,
                            int K, hipStream_t st);
int launch_code_prior_score(const long* inds, const long* pos, const long* left, const long* up, const long* prev,
                            const long* pos_tot, const long* left_tot, const long* up_tot, const long* prev_tot, const double* lambda,
                            double* logp, double* resp, int* bad, int B, int C, int H, int W, int K, hipStream_t st);
int launch_code_prior_sample(const long* pos, const long* left, const long* up, const long* prev, const long* pos_tot,
                             const long* left_tot, const long* up_tot, const long* prev_tot, const double* lambda, const double* u,
                             long* inds, int n, int C, int H, int W, int K, hipStream_t st);
int launch_code_prior_embed(const long* inds, const float* codebooks, float* out, int n, int C, int H, int W, int K, int Dc,
                            hipStream_t st);

// vqusage.hip
size_t vq_usage_pass_indices();
int launch_vq_usage(const long* inds, long* counts, long* invalid, int B, int C, int HW, int K, hipStream_t st);
int launch_vq_pool_fill(const float* latents, float* pool, long P, int D, long R, hipStream_t st);
int launch_vq_usage_pool_fill(const long* inds, long* counts, long* invalid, int B, int C, int HW, int K, const float* latents,
                              float* pool, long P, int D, long R, hipStream_t st);
int launch_vq_restart(const long* list, int n, const float* pool, int valid_rows, int D, const float* rows, float* codebooks,
                      float* exp_avg, float* exp_avg_sq, int C, int K, int Dc, hipStream_t st);
int launch_vq_restart_gather(const long* list, int n, const float* pool, int valid_rows, int D, int C, int Dc, float* rows,
                             hipStream_t st);

}  // namespace ctvae
