// Launchers that only the step plan (plan.hip) and the live mosaic (mosaic_live.hip) call: forms of public entry points with extra operands (fp8 copies,
// per-block maxima, frames read in place).  Not part of the C ABI (include/rawvae_hip.h) and not exported.
#pragma once
#include "../../include/rawvae_hip.h"

#define RV_INTERNAL extern "C" __attribute__((visibility("hidden")))

// The pickers behind rv_gemm_plan (gemm_launch.hip).
RV_INTERNAL int rv_gemm_pick(long Mp, long Np, long Kp, int max_splits, int* bm, int* bn, int* splits);
RV_INTERNAL int rv_gemm_tile(long Mp, long Np, int splits, int* bm, int* bn);
// whether rv_latent_fwd / rv_latent_bwd run their row-local kernels on this shape (1) or the GEMM forms (0): csrc/latent.hip
RV_INTERNAL int rv_latent_rowlocal(long Bp, long Hp, long Lp);
RV_INTERNAL int rv_latent_bwd_pp(long Bp, long Hp, long Lp);
RV_INTERNAL int rv_latent_bwd_tile_rows(long Bp, long Hp, long Lp);
// ... of the fused loss forward on fp8 operands (never 256 x 256)
RV_INTERNAL int rv_gemm_tile_fp8_loss(long Mp, long Np, int* bm, int* bn);
RV_INTERNAL int rv_dgrad_wgrad_pick(long Mp, long Np, long Kp, int* paired, int* bm_dgrad, int* splits);
RV_INTERNAL int rv_wgrad_adam_fits(long Mp, long Np, long Kp, int splits);

// rv_cast_pad_bf16 that also writes the fp8 operand (dst_fp8 may be NULL) and, when `fp8_state` is given, latches the
// delayed activation scale for this step in its first wave from the previous step's per-block maxima
// `amax_part[n_amax]` (state block layout: RV_OPT_FP8 in the public header), and dP1's scale likewise from the
// `n_amax2` maxima that follow them (rv_heads_bwd_ex; 0 = none).  dst_bf16 may be NULL when dst_fp8 is given.
RV_INTERNAL int rv_cast_pad_bf16_q8(const float* src, long rows, long cols, long ld_src, void* dst_bf16, long rows_p,
                                    long cols_p, long ld_dst, void* dst_fp8, long ld_fp8, float* fp8_state,
                                    const float* amax_part, int n_amax, int n_amax2, long long* step_counter, void* stream);
// The same from hop-strided frames of a resident fp32 waveform (rv_gather_frames + the cast in one kernel).
RV_INTERNAL int rv_gather_cast_frames(const float* audio, long n_samples, const long long* frame_index, long first_frame,
                                      long n_frames, long S, long hop, void* dst_bf16, long rows_p, long cols_p,
                                      long ld_dst, void* dst_fp8, long ld_fp8, float* fp8_state, const float* amax_part,
                                      int n_amax, int n_amax2, long long* step_counter, void* stream);
// The two operands of a GEMM: bf16, or -- dq != NULL -- e4m3 bytes, dq then being the device scalar 1 / (scale_a * scale_b)
// that undoes their scales.  Leading dims in elements either way.
struct rv_gemm_operands {
  const void* a; long lda;
  const void* b; long ldb;
  const float* dq;
};
// Frames read from a resident waveform (rv_plan_step_frames): frame r = waveform[f * hop ...], f = idx ? idx[r] : first + r
struct rv_frame_src {
  const long long* idx;
  long first, hop, n_samples;
  const void* bf16;   // the waveform as bf16 (fc1's operand is gathered from it), or null
};
// rv_linear_fwd with every option of a bias/ReLU forward GEMM (NULL = not wanted): fp8 operands (op.dq); the output also
// as fp8(y * *q_scale) (the next layer's fp8 operand) and max|y| of every block in amax_part[block], from which the next
// step derives its scale (delayed scaling); rv_linear_fwd_frames' form when `fr` is given: A's first n_frames rows are
// gathered from fr->bf16, op.a (may be NULL) receives them as a by-product and block 0 bumps *step_counter.
RV_INTERNAL int rv_linear_fwd_ex(rv_gemm_operands op, const float* bias, long Mp, long Np, long Kp, int act, void* y_bf16,
                                 long ldy, void* y_fp8, long ldy_fp8, const float* q_scale, float* amax_part,
                                 const rv_frame_src* fr, long n_frames, long long* step_counter, void* stream);
// rv_decode_out_loss_fwd on bf16 or fp8 operands (op.dq); the fp32 target rows are x's, or -- `fr` -- frames of the
// waveform x read in place.  dP4_fp8 != NULL (fp8 operands only): the epilogue also writes fp8(dP4 * *dp4_scale), the
// fp8 fc4 backward's operand; dP4_bf16 may then be NULL.
RV_INTERNAL int rv_decode_out_loss_fwd_ex(rv_gemm_operands op, const float* b4, long Bp, long Sp, long Hp, long B, long S,
                                          const float* x, long ldx, const rv_frame_src* fr, float* recon, long ld_recon,
                                          void* dP4_bf16, long ld_dp4, void* dP4_fp8, long ld_dp4q, const float* dp4_scale,
                                          float* mse_partial, float* db4_partial, void* stream);
// max|W1|, max|W4| of the fp8 weight shadows (n1 / n4 bytes) into the 2 x 1024 slots behind the fp8 state block
// (RV_OPT_FP8): the plan runs it behind the optimizer, the next step's first kernel turns it into the weight scales.
RV_INTERNAL int rv_fp8_wmax(const void* w1q, long n1, const void* w4q, long n4, float* fp8_state, void* stream);
// rv_latent_fwd with the fp8 forward's extra outputs of fc3 (NULL = not wanted): h3 also as fp8(h3 * *q_scale), and
// max|h3| of every wave's outputs in amax_part[8 * (Bp / 16)].
RV_INTERNAL int rv_latent_fwd_ex(const void* h_bf16, long ldh, const void* wh_bf16, long ldwh, const float* bias_heads,
                                 const void* w3_bf16, long ldw3, const float* bias3, long Bp, long Hp, long Lp, long B, long L,
                                 const float* eps_in, float* eps_out, unsigned long long seed, const long long* step_counter,
                                 float* mulv, void* z_bf16, float* kl_partial, void* h3_bf16, long ldh3, void* h3_fp8, long ldq,
                                 const float* q_scale, float* amax_part, void* stream);
// Device-side cross-stream signalling (elementwise.hip): publish `value` behind the stream's earlier work / hold the
// stream until the flag has reached `value` (bounded; timeouts are counted in *timeouts).
RV_INTERNAL int rv_flag_set(int* flag, int value, void* stream);
// ... and *copy_dst = *copy_src first (same one-wave kernel)
RV_INTERNAL int rv_flag_set_copy(int* flag, int value, const long long* copy_src, long long* copy_dst, void* stream);
RV_INTERNAL int rv_flag_wait(const int* flag, int value, int* timeouts, long max_ms, void* stream);
// rv_adam_multi that withholds the update when `*poison` is non-zero (poison may be NULL): the data-parallel step passes
// its count of flag waits that ran out, so that a step whose exchange did not complete in time changes no parameter.
RV_INTERNAL int rv_adam_multi_guarded(const rv_param_desc* descs, int n_desc, float* param, float* exp_avg, float* exp_avg_sq,
                                      float* grad_out, const void* grad_bf16, float lr, float grad_scale,
                                      const long long* step_counter, const int* poison, void* stream);
// The loss scalar (total, mse, kld) from a forward's partial sums, and rv_grad_finalize times a device-side scalar
// (elementwise.hip): the two pieces of rv_plan_loss / rv_plan_set_loss_grad (plan.hip).
RV_INTERNAL int rv_loss_from_partials(const float* mse_partial, int n_mse, const float* kl_partial, int n_kl, long B, long S,
                                      long L, float kl_beta, float* out3, void* stream);
RV_INTERNAL int rv_grad_finalize_scaled(const rv_param_desc* descs, int n_desc, void* grad_out, int out_bf16,
                                        const float* scale_dev, void* stream);
// What the rider blocks of rv_linear_wgrad_riders do with the tensors of their table: the fused Adam update
// (rv_linear_wgrad_adam), or -- grad_out != NULL -- only sum their slabs into a flat payload arena (fp32, or bf16 when
// out_bf16): rv_grad_finalize's work.
struct rv_rider_target {
  float* param; float* exp_avg; float* exp_avg_sq;
  float lr, grad_scale;
  const long long* step_counter;
  void* grad_out; int out_bf16;
};
// rv_linear_wgrad_adam's launch shape (256 x 256 weight-gradient GEMM + rider blocks on the idle CUs) on bf16 or fp8
// operands (gemm_launch.hip).  fp8: dy [Kp(batch), Mp] and x [Kp, Np] both read MN-major (the contraction index is the
// row of both matrices), dq = 1 / (scale_dy * scale_x).
RV_INTERNAL int rv_linear_wgrad_riders(rv_gemm_operands op, long Mp, long Np, long Kp, int splits, void* dw_slabs, long lddw,
                                       int slab_dtype, float* slab_unscale, const rv_param_desc* descs, int n_desc,
                                       rv_rider_target riders, int n_rider_blocks, void* stream);
// The heads' backward that writes its fp8 left operand (latent.hip).
RV_INTERNAL int rv_heads_bwd_ex(const void* dmulv_bf16, const void* wh_bf16, long ldw, const void* h1_bf16, long ldh, long Bp,
                                long Hp, long Lp, void* dp1_bf16, long ldp, float* db1_partial, float* dwh_slabs, long lddw,
                                void* dp1_fp8, long ldq, const float* q_scale, float* amax_part, float* dwh_unscale,
                                void* stream);
// One-shot: the next paired dgrad + wgrad launch (bf16 or fp8) signals `hip_event` when it completes -- the event is the
// launch's own completion signal (hipExtLaunchKernelGGL), cheaper on both streams than a hipEventRecord behind it.
// Not under stream capture.  Returns 1 when an event armed earlier was still pending, i.e. no paired launch took it
// (other tile forms): call with NULL behind the backward to disarm and to learn which.
RV_INTERNAL int rv_pair_stop_event(void* hip_event);
// Whether the paired fc4 backward on fp8 operands fits the extents (gemm_launch.hip), and rv_linear_dgrad_wgrad on
// bf16 or fp8 operands: dgrad = {dy, w}, wgrad = {dy, x}; the dgrad's ReLU mask is the bf16 `mask` or -- mask_is_fp8 --
// an fp8 image (ldmask in bytes).
RV_INTERNAL int rv_dgrad_wgrad_fp8_fits(long Mp, long Np, long Kp, int splits);
RV_INTERNAL int rv_linear_dgrad_wgrad_ex(rv_gemm_operands dgrad, rv_gemm_operands wgrad, const void* mask, long ldmask,
                                         int mask_is_fp8, long Mp, long Np, long Kp, void* dx_bf16, long lddx,
                                         float* colsum_partial, void* dw_slabs, long lddw, int splits, int slab_dtype,
                                         float* slab_unscale, void* stream);
// The two ends of rv_stream_process (stream.hip) for the live mosaic, which searches the corpus between them.
// rv_stream_encode: rv_stream_process's checks (no temperature, no eps), its fc1 launch on [history | x] and its heads
// launch with q [n_streams * F, L] = mu * scale + offset in place of the reparameterised z; *z and *frames receive the
// stream workspace's latent rows [n_streams * F, L] and decoded frames [n_streams * F, S].  q == NULL: the checks and
// the two pointers only, nothing is launched (RV_MOSAIC_LIVE_DRAIN).
// rv_stream_synth: decode != 0: fc3 and fc4 on the latent rows into the frames; then k_stream_ola on the frames.
RV_INTERNAL int rv_stream_encode(const rv_stream_desc* d, float* q, float** z, float** frames, void* stream);
RV_INTERNAL int rv_stream_synth(const rv_stream_desc* d, int decode, void* stream);
// the streams' frame counters [n_streams] int64 in the stream workspace (frames since the stream's last reset; moved on
// by the overlap-add at the end of a block call)
RV_INTERNAL const long long* rv_stream_counters(const rv_stream_desc* d);
// Candidates per row at most, of every rv_mosaic op that takes k (mosaic*.hip, grain.hip)
constexpr int KMAX = 16;
// Query rows RV_MOSAIC_KNN_SMALL accepts, and up to which RV_MOSAIC_LIVE searches with it: measured faster than
// k_knn_topk at every T up to here (1.4-1.9x at 64 rows, 4-10x at 16 and fewer against 1.24 M corpus rows)
constexpr int SMALL_T_MAX = 64;
// The kNN search of rv_mosaic (mosaic_knn.hip), small != 0 being its few-query form: RV_MOSAIC_KNN / _KNN_SMALL -- checks
// first, then the search and its merge, no sync and no read of the device -- and RV_MOSAIC_KNN_WORKSPACE /
// _KNN_SMALL_WORKSPACE, which runs the checks, writes d->ws_bytes and launches nothing (the live block's layout calls
// it on a copy of its descriptor with T = its query rows).
RV_INTERNAL int rv_knn_search(const rv_mosaic_desc* d, int small, void* stream);
RV_INTERNAL int rv_knn_workspace(rv_mosaic_desc* d, int small);
// RV_MOSAIC_GATHER_MEAN and RV_MOSAIC_OLA (mosaic.hip): checks first, then one launch each.  rv_gather_mean_launch is
// the former's launch on explicit operands, without the op's checks: the live block gathers latent rows or grains
// with it.
RV_INTERNAL int rv_gather_mean(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_gather_mean_launch(const float* src, long src_len, const long long* row_start, long stride, long n_rows,
                                      long width, const int* idx, long T, int k, float* out, long ldo, void* stream);
RV_INTERNAL int rv_ola(const rv_mosaic_desc* d, void* stream);
// The offline unit selection of rv_mosaic (mosaic_path.hip): RV_MOSAIC_TRANSITION, RV_MOSAIC_PATH_FORWARD and
// RV_MOSAIC_PATH_BACKTRACK -- checks first, then one launch each, no sync and no read of the device -- and
// RV_MOSAIC_PATH_WORKSPACE, which writes d->ws_bytes and launches nothing.
RV_INTERNAL int rv_path_transition(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_path_forward(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_path_backtrack(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_path_workspace(rv_mosaic_desc* d);
// The live block of rv_mosaic (mosaic_live.hip): RV_MOSAIC_LIVE_WORKSPACE, which writes d->ws_bytes and launches
// nothing; RV_MOSAIC_LIVE_RESET; and rv_live_block: RV_MOSAIC_LIVE, or -- drain != 0 -- RV_MOSAIC_LIVE_DRAIN.
RV_INTERNAL int rv_live_workspace(rv_mosaic_desc* d);
RV_INTERNAL int rv_live_reset(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_live_block(const rv_mosaic_desc* d, int drain, void* stream);
// The two grain-fitting ops of rv_mosaic (grain.hip): RV_GRAIN_FIT and RV_GRAIN_GATHER on the fields the public header
// names for them; checks first, then one launch each, no sync and no read of the device.
RV_INTERNAL int rv_grain_fit(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_grain_gather(const rv_mosaic_desc* d, void* stream);
// The live mosaic's grain fit (grain.hip; the rule: the public header, "Live grain fitting"), on the fields the header
// names: fit_radius, gain_max, shift / gain / score [M, sel_k], next_of [3 N] = successors then room.
// rv_grain_live_check: the fit's argument checks for op `op` (d->live is not null); run: also the tables and outputs.
// rv_grain_live_ring: floats of one stream's target ring.  rv_grain_live_reset: silence in the rings of n streams from
// `first`.  rv_grain_live: the block into the rings, the fit of sel [M, sel_k] against the target frames the rows stand
// for (tfr [M] from the lagged selection, or NULL: the frames arriving now) and the gather of the fitted grains into
// frames [M, S]; three launches, no sync and no read of the device.
RV_INTERNAL int rv_grain_live_check(const rv_mosaic_desc* d, const char* op, int run);
RV_INTERNAL long rv_grain_live_ring(long S, long hop, long block, long lag);
RV_INTERNAL int rv_grain_live_reset(float* ring, long C, long first, long n, void* stream);
RV_INTERNAL int rv_grain_live(const rv_mosaic_desc* d, const int* sel, int sel_k, float* ring, const long long* cnt,
                              const long long* tfr, float* frames, void* stream);
// The two evaluation ops of rv_mosaic (eval.hip): RV_EVAL_FRAMES and RV_EVAL_DIMS on the fields the public header names
// for them; checks first, then one launch (EVAL_DIMS: two beyond one block of rows), no sync and no read of the device.
RV_INTERNAL int rv_eval_frames(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_eval_dims(const rv_mosaic_desc* d, void* stream);
// The latent-PCA ops of rv_mosaic (pca.hip): RV_PCA_MOMENTS, RV_PCA_EIG and RV_PCA_APPLY on the fields the public header
// names for them -- checks first, then the launches, no sync and no read of the device -- and RV_PCA_WORKSPACE, which
// writes d->ws_bytes and launches nothing.
RV_INTERNAL int rv_pca_moments(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_pca_eig(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_pca_apply(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_pca_workspace(rv_mosaic_desc* d);
// The latent-walk ops of rv_mosaic (walk.hip): RV_PCA_LAGCOV, RV_WALK_FIT and RV_WALK_STEP on the fields the public
// header names for them -- checks first, then the launches, no sync and no read of the device -- and RV_WALK_WORKSPACE,
// which writes d->ws_bytes and launches nothing.
RV_INTERNAL int rv_pca_lagcov(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_walk_fit(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_walk_step(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_walk_workspace(rv_mosaic_desc* d);
// The alignment ops of rv_mosaic (align.hip): RV_ALIGN_COST, RV_ALIGN_FORWARD, RV_ALIGN_BACKTRACK and RV_ALIGN_WARP on the
// fields the public header names for them -- checks first, then one launch each, no sync and no read of the device -- and
// RV_ALIGN_WORKSPACE, which writes d->ws_bytes and launches nothing.
RV_INTERNAL int rv_align_cost(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_align_forward(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_align_backtrack(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_align_warp(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_align_workspace(rv_mosaic_desc* d);
// The structure ops of rv_mosaic (structure.hip): RV_STRUCT_NOVELTY and RV_STRUCT_PEAKS on the fields the public header
// names for them -- checks first, then the launches, no sync and no read of the device -- and RV_STRUCT_WORKSPACE, which
// writes d->ws_bytes and launches nothing.
RV_INTERNAL int rv_struct_novelty(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_struct_peaks(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_struct_workspace(rv_mosaic_desc* d);
// The restoration ops of rv_mosaic (smooth.hip): RV_SMOOTH_FILTER, RV_SMOOTH_BACKWARD and RV_SMOOTH_SPLICE on the fields the
// public header names for them -- checks first, then the launches, no sync and no read of the device -- and
// RV_SMOOTH_WORKSPACE, which writes d->ws_bytes and launches nothing.
RV_INTERNAL int rv_smooth_filter(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_smooth_backward(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_smooth_splice(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_smooth_workspace(rv_mosaic_desc* d);
// The recurrence ops of rv_mosaic (recur.hip): RV_RECUR_PROFILE on the fields the public header names for it -- checks
// first, then the launches, no sync and no read of the device -- and RV_RECUR_WORKSPACE, which writes d->ws_bytes and
// launches nothing.
RV_INTERNAL int rv_recur_profile(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_recur_workspace(rv_mosaic_desc* d);
// The latent-state ops of rv_mosaic (hmm.hip): RV_HMM_EMIT, RV_HMM_FORWARD_BACKWARD, RV_HMM_MSTEP and RV_HMM_VITERBI on the
// fields the public header names for them -- checks first, then the launches, no sync and no read of the device -- and
// RV_HMM_WORKSPACE, which writes d->ws_bytes and launches nothing.
RV_INTERNAL int rv_hmm_emit(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_hmm_forward_backward(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_hmm_mstep(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_hmm_viterbi(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_hmm_workspace(rv_mosaic_desc* d);
// The latent-attribute ops of rv_mosaic (attr.hip): RV_ATTR_DESCRIBE and RV_ATTR_FIT on the fields the public header names
// for them -- checks first, then the launches, no sync and no read of the device -- and RV_ATTR_WORKSPACE, which writes
// d->ws_bytes and launches nothing.
RV_INTERNAL int rv_attr_describe(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_attr_fit(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_attr_workspace(rv_mosaic_desc* d);
// The switching-walk ops of rv_mosaic (switch.hip): RV_SWITCH_RESIDUAL, RV_SWITCH_MOMENTS, RV_SWITCH_FIT and RV_SWITCH_STEP
// on the fields the public header names for them -- checks first, then the launches, no sync and no read of the device --
// and RV_SWITCH_WORKSPACE, which writes d->ws_bytes and launches nothing.
RV_INTERNAL int rv_switch_residual(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_switch_moments(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_switch_fit(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_switch_step(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_switch_workspace(rv_mosaic_desc* d);
// The latent-transport ops of rv_mosaic (transport.hip): RV_OT_WHITEN, RV_OT_SOFTMIN, RV_OT_MAP and RV_OT_LIVE on the fields the
// public header names for them -- checks first, then the launches, no sync and no read of the device -- and RV_OT_WORKSPACE,
// which writes d->ws_bytes and launches nothing.
RV_INTERNAL int rv_ot_whiten(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_ot_softmin(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_ot_map(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_ot_live(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_ot_workspace(rv_mosaic_desc* d);
// The beat ops of rv_mosaic (beat.hip): RV_BEAT_ONSET, RV_BEAT_TEMPOGRAM and RV_BEAT_TRACK on the fields the public header
// names for them -- checks first, then the launches, no sync and no read of the device -- and RV_BEAT_WORKSPACE, which
// writes d->ws_bytes and launches nothing.
RV_INTERNAL int rv_beat_onset(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_beat_tempogram(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_beat_track(const rv_mosaic_desc* d, void* stream);
RV_INTERNAL int rv_beat_workspace(rv_mosaic_desc* d);
