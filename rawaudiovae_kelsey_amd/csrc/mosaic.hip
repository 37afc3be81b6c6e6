// rv_mosaic(op, desc, stream): the one entry point of the audio tools, a dispatch table over 62 ops (codes 0 .. 37, 40, 41,
// 43 .. 47, 49 .. 56 and 58 .. 66; 38, 39, 42, 48 and 57 are unassigned and answer as unknown ops).  Each family keeps its kernels, checks and launches in its own
// file and hands rv_mosaic one function per op (internal.h):
//    0, 1, 8, 9   RV_MOSAIC_KNN, _KNN_WORKSPACE, _KNN_SMALL, _KNN_SMALL_WORKSPACE        mosaic_knn.hip
//    2, 3         RV_MOSAIC_GATHER_MEAN, RV_MOSAIC_OLA                                   this file
//    4 .. 7       RV_MOSAIC_TRANSITION, _PATH_FORWARD, _PATH_BACKTRACK, _PATH_WORKSPACE  mosaic_path.hip
//   10 .. 13      RV_MOSAIC_LIVE, _LIVE_WORKSPACE, _LIVE_RESET, _LIVE_DRAIN              mosaic_live.hip
//   14, 15        RV_GRAIN_FIT, RV_GRAIN_GATHER                                          grain.hip
//   16, 17        RV_EVAL_FRAMES, RV_EVAL_DIMS                                           eval.hip
//   18 .. 21      RV_PCA_MOMENTS, _EIG, _APPLY, _WORKSPACE                               pca.hip
//   22 .. 25      RV_PCA_LAGCOV, RV_WALK_FIT, _STEP, _WORKSPACE                          walk.hip
//   26 .. 30      RV_ALIGN_COST, _FORWARD, _BACKTRACK, _WARP, _WORKSPACE                 align.hip
//   31 .. 33      RV_STRUCT_NOVELTY, _PEAKS, _WORKSPACE                                  structure.hip
//   34 .. 37      RV_SMOOTH_FILTER, _BACKWARD, _SPLICE, _WORKSPACE                       smooth.hip
//   40, 41        RV_RECUR_PROFILE, _WORKSPACE                                           recur.hip
//   43 .. 47      RV_HMM_EMIT, _FORWARD_BACKWARD, _MSTEP, _VITERBI, _WORKSPACE           hmm.hip
//   49 .. 51      RV_ATTR_DESCRIBE, _FIT, _WORKSPACE                                     attr.hip
//   52 .. 56      RV_SWITCH_RESIDUAL, _MOMENTS, _FIT, _STEP, _WORKSPACE                  switch.hip
//   58 .. 62      RV_OT_WHITEN, _SOFTMIN, _MAP, _LIVE, _WORKSPACE                        transport.hip
//   63 .. 66      RV_BEAT_ONSET, _TEMPOGRAM, _TRACK, _WORKSPACE                          beat.hip
// Here also the two synthesis ops of the offline mosaic (rawaudiovae_kelsey_amd/mosaic.py):
//   RV_MOSAIC_GATHER_MEAN  out[t] = (1/k) sum_j src[start(idx[t, j]) : + width] (grains or latent rows)
//   RV_MOSAIC_OLA          offline weighted overlap-add normalised by the window sum
#include "common.h"
#include "internal.h"

using namespace rv;

namespace {

// One block per output row (grid-stride), threads over the width: ascending-j fp32 sum from +0, times 1/k once.
// Indices outside [0, n_rows) (-1: no neighbour) and rows outside src contribute nothing.
__global__ void __launch_bounds__(256)
k_gather_mean(const float* __restrict__ src, long src_len, const long long* __restrict__ row_start, long stride,
              long n_rows, long width, const int* __restrict__ idx, long T, int k, float* __restrict__ out, long ldo) {
  const float inv = 1.0f / (float)k;
  for (long t = blockIdx.x; t < T; t += gridDim.x) {
    for (long w = threadIdx.x; w < width; w += 256) {
      float acc = 0.f;
      for (int j = 0; j < k; ++j) {
        const long i = idx[t * k + j];
        if (i < 0 || i >= n_rows) continue;
        const long st = row_start ? row_start[i] : i * stride;
        if (st < 0 || st + width > src_len) continue;
        acc += src[st + w];
      }
      out[t * ldo + w] = acc * inv;
    }
  }
}

__device__ __forceinline__ float wola_add(float num, float w, float d) {
#pragma clang fp contract(off)
  return num + w * d;
}

// out[t] = sum_f w[t - f hop] D_f[t - f hop] / sum_f w[t - f hop] over the frames f that cover t, both sums in
// ascending f from +0 (the products rounded before the add); 0 where the normaliser is 0.  window NULL: all ones.
__global__ void __launch_bounds__(256)
k_ola(const float* __restrict__ frames, long F, long S, long hop, const float* __restrict__ window, long n_out,
      float* __restrict__ out) {
  for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < n_out; t += (long)gridDim.x * 256) {
    const long jlo = t >= S ? (t - S) / hop + 1 : 0;
    const long jhi = t / hop < F - 1 ? t / hop : F - 1;
    float num = 0.f, den = 0.f;
    for (long j = jlo; j <= jhi; ++j) {
      const long o = t - j * hop;
      const float w = window ? window[o] : 1.f;
      num = wola_add(num, w, frames[j * S + o]);
      den += w;
    }
    out[t] = den == 0.f ? 0.f : num / den;
  }
}

}  // namespace

int rv_gather_mean_launch(const float* src, long src_len, const long long* row_start, long stride, long n_rows,
                          long width, const int* idx, long T, int k, float* out, long ldo, void* stream) {
  hipLaunchKernelGGL(k_gather_mean, dim3(blocks_for(T, 65536)), dim3(256), 0, (hipStream_t)stream, src, src_len,
                     row_start, stride, n_rows, width, idx, T, k, out, ldo);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_gather_mean(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->src && d->idx && d->out, RV_ERR_NULL, "rv_mosaic(GATHER_MEAN): null pointer");
  RV_REQUIRE(d->T >= 1 && d->k >= 1 && d->k <= KMAX && d->width >= 1 && d->n_rows >= 1 && d->src_len >= d->width &&
                 d->ldo >= d->width && (d->row_start || d->stride >= 0),
             RV_ERR_SHAPE, "rv_mosaic(GATHER_MEAN): bad extents T=%ld k=%ld width=%ld n_rows=%ld src_len=%ld "
             "ldo=%ld stride=%ld", d->T, d->k, d->width, d->n_rows, d->src_len, d->ldo, d->stride);
  return rv_gather_mean_launch(d->src, d->src_len, d->row_start, d->stride, d->n_rows, d->width, d->idx, d->T,
                               (int)d->k, d->out, d->ldo, stream);
}

int rv_ola(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->frames && d->out, RV_ERR_NULL, "rv_mosaic(OLA): null pointer");
  RV_REQUIRE(d->F >= 1 && d->S >= 1 && d->hop >= 1 && d->n_out >= 1, RV_ERR_SHAPE,
             "rv_mosaic(OLA): bad extents F=%ld S=%ld hop=%ld n_out=%ld", d->F, d->S, d->hop, d->n_out);
  hipLaunchKernelGGL(k_ola, dim3(blocks_for((d->n_out + 255) / 256, 65536)), dim3(256), 0, (hipStream_t)stream, d->frames,
                     d->F, d->S, d->hop, d->window, d->n_out, d->out);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_mosaic(int op, rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d, RV_ERR_NULL, "rv_mosaic: null descriptor");
  switch (op) {
    case RV_MOSAIC_KNN: return rv_knn_search(d, 0, stream);
    case RV_MOSAIC_KNN_WORKSPACE: return rv_knn_workspace(d, 0);
    case RV_MOSAIC_GATHER_MEAN: return rv_gather_mean(d, stream);
    case RV_MOSAIC_OLA: return rv_ola(d, stream);
    case RV_MOSAIC_TRANSITION: return rv_path_transition(d, stream);
    case RV_MOSAIC_PATH_FORWARD: return rv_path_forward(d, stream);
    case RV_MOSAIC_PATH_BACKTRACK: return rv_path_backtrack(d, stream);
    case RV_MOSAIC_PATH_WORKSPACE: return rv_path_workspace(d);
    case RV_MOSAIC_KNN_SMALL: return rv_knn_search(d, 1, stream);
    case RV_MOSAIC_KNN_SMALL_WORKSPACE: return rv_knn_workspace(d, 1);
    case RV_MOSAIC_LIVE: return rv_live_block(d, 0, stream);
    case RV_MOSAIC_LIVE_WORKSPACE: return rv_live_workspace(d);
    case RV_MOSAIC_LIVE_RESET: return rv_live_reset(d, stream);
    case RV_MOSAIC_LIVE_DRAIN: return rv_live_block(d, 1, stream);
    case RV_GRAIN_FIT: return rv_grain_fit(d, stream);
    case RV_GRAIN_GATHER: return rv_grain_gather(d, stream);
    case RV_EVAL_FRAMES: return rv_eval_frames(d, stream);
    case RV_EVAL_DIMS: return rv_eval_dims(d, stream);
    case RV_PCA_MOMENTS: return rv_pca_moments(d, stream);
    case RV_PCA_EIG: return rv_pca_eig(d, stream);
    case RV_PCA_APPLY: return rv_pca_apply(d, stream);
    case RV_PCA_WORKSPACE: return rv_pca_workspace(d);
    case RV_PCA_LAGCOV: return rv_pca_lagcov(d, stream);
    case RV_WALK_FIT: return rv_walk_fit(d, stream);
    case RV_WALK_STEP: return rv_walk_step(d, stream);
    case RV_WALK_WORKSPACE: return rv_walk_workspace(d);
    case RV_ALIGN_COST: return rv_align_cost(d, stream);
    case RV_ALIGN_FORWARD: return rv_align_forward(d, stream);
    case RV_ALIGN_BACKTRACK: return rv_align_backtrack(d, stream);
    case RV_ALIGN_WARP: return rv_align_warp(d, stream);
    case RV_ALIGN_WORKSPACE: return rv_align_workspace(d);
    case RV_STRUCT_NOVELTY: return rv_struct_novelty(d, stream);
    case RV_STRUCT_PEAKS: return rv_struct_peaks(d, stream);
    case RV_STRUCT_WORKSPACE: return rv_struct_workspace(d);
    case RV_SMOOTH_FILTER: return rv_smooth_filter(d, stream);
    case RV_SMOOTH_BACKWARD: return rv_smooth_backward(d, stream);
    case RV_SMOOTH_SPLICE: return rv_smooth_splice(d, stream);
    case RV_SMOOTH_WORKSPACE: return rv_smooth_workspace(d);
    case RV_RECUR_PROFILE: return rv_recur_profile(d, stream);
    case RV_RECUR_WORKSPACE: return rv_recur_workspace(d);
    case RV_HMM_EMIT: return rv_hmm_emit(d, stream);
    case RV_HMM_FORWARD_BACKWARD: return rv_hmm_forward_backward(d, stream);
    case RV_HMM_MSTEP: return rv_hmm_mstep(d, stream);
    case RV_HMM_VITERBI: return rv_hmm_viterbi(d, stream);
    case RV_HMM_WORKSPACE: return rv_hmm_workspace(d);
    case RV_ATTR_DESCRIBE: return rv_attr_describe(d, stream);
    case RV_ATTR_FIT: return rv_attr_fit(d, stream);
    case RV_ATTR_WORKSPACE: return rv_attr_workspace(d);
    case RV_SWITCH_RESIDUAL: return rv_switch_residual(d, stream);
    case RV_SWITCH_MOMENTS: return rv_switch_moments(d, stream);
    case RV_SWITCH_FIT: return rv_switch_fit(d, stream);
    case RV_SWITCH_STEP: return rv_switch_step(d, stream);
    case RV_SWITCH_WORKSPACE: return rv_switch_workspace(d);
    case RV_OT_WHITEN: return rv_ot_whiten(d, stream);
    case RV_OT_SOFTMIN: return rv_ot_softmin(d, stream);
    case RV_OT_MAP: return rv_ot_map(d, stream);
    case RV_OT_LIVE: return rv_ot_live(d, stream);
    case RV_OT_WORKSPACE: return rv_ot_workspace(d);
    case RV_BEAT_ONSET: return rv_beat_onset(d, stream);
    case RV_BEAT_TEMPOGRAM: return rv_beat_tempogram(d, stream);
    case RV_BEAT_TRACK: return rv_beat_track(d, stream);
    case RV_BEAT_WORKSPACE: return rv_beat_workspace(d);
  }
  return rv_fail(RV_ERR_UNSUPPORTED, "rv_mosaic: unknown op %d", op);
}
