// Latent audio mosaicing (rawaudiovae_kelsey_amd/mosaic.py): frame-level nearest neighbours in the latent space and
// the synthesis built on them, behind the one entry point rv_mosaic(op, desc, stream):
//   RV_MOSAIC_KNN          k nearest corpus rows of every query row, direct squared distances (the hot path):
//                          k_knn_topk over (query tile, corpus split), then k_knn_merge of the per-split partials
//   RV_MOSAIC_GATHER_MEAN  out[t] = (1/k) sum_j src[start(idx[t, j]) : + width] (grains or latent rows)
//   RV_MOSAIC_OLA          offline weighted overlap-add normalised by the window sum
// Layout, split and merge, and the measured figures: DESIGN.md section 7.5.
#include <limits.h>

#include "common.h"
#include "../../include/rawvae_hip.h"

using namespace rv;

namespace {

// k_knn_topk tile: rv_som_bmu's (BR query rows x BN corpus rows per step, KT latent elements per LDS stage, 16 x 16
// threads each owning an 8 x 4 register tile), so every distance is its arithmetic bit for bit.  The finished
// BR x BN distance tile goes through LDS and is scanned by two lanes per query row, each keeping a sorted top-KM
// list in registers over its half of the corpus rows: 2 KM VGPRs per lane instead of 8 rows x 2 KM.
constexpr int BR = 128, BN = 64, KT = 32, TR = 8, TN = 4, PAD = 4, DPAD = 1;
constexpr int STAGE_FLOATS = KT * (BR + PAD) + KT * (BN + PAD), DIST_FLOATS = BR * (BN + DPAD);
constexpr int SMEM_FLOATS = STAGE_FLOATS > DIST_FLOATS ? STAGE_FLOATS : DIST_FLOATS;
constexpr int KMAX = 16;
constexpr long TARGET_BLOCKS = 1024;   // 4 workgroups per CU of a 256-CU MI355X
constexpr long MIN_SPLIT_TILES = 4;    // corpus tiles per split before a search is split further

// (d, i) < (e, j) in the order "smaller distance, then lower index" (rv_som_bmu's): a total order on the candidates of
// one query row (corpus indices are distinct), so the top k do not depend on the visiting order.  NaN never wins.
__device__ __forceinline__ bool cand_less(float d, int i, float e, int j) { return d < e || (d == e && i < j); }

// sorted insert by a compare-and-swap cascade over static indices (selects only): the list stays in registers
template <int KM>
__device__ __forceinline__ void topk_insert(float d, int i, float (&bd)[KM], int (&bi)[KM]) {
  if (!cand_less(d, i, bd[KM - 1], bi[KM - 1])) return;
#pragma unroll
  for (int s = 0; s < KM; ++s) {
    const bool lt = cand_less(d, i, bd[s], bi[s]);
    const float td = bd[s];
    const int ti = bi[s];
    bd[s] = lt ? d : td;
    bi[s] = lt ? i : ti;
    d = lt ? td : d;
    i = lt ? ti : i;
  }
}

// One block per (query tile, corpus split).  Split s covers corpus rows [s * per_split, (s + 1) * per_split) with
// per_split a multiple of BN.  With one split the block writes the result; otherwise its first k entries per row go
// to the workspace (raw: empty slots are (+inf, INT_MAX)).
template <int KM>
__global__ void __launch_bounds__(256)
k_knn_topk(const float* __restrict__ q, long T, const float* __restrict__ c, long N, long L, int k, long per_split,
           int n_splits, int* __restrict__ idx, float* __restrict__ dist, float* __restrict__ ws_d,
           int* __restrict__ ws_i) {
  // the staging tiles and the distance tile share LDS (33 KB instead of 59 KB: four workgroups per CU, not two)
  __shared__ __attribute__((aligned(16))) float smem[SMEM_FLOATS];
  float(*Xs)[BR + PAD] = reinterpret_cast<float(*)[BR + PAD]>(smem);
  float(*Ws)[BN + PAD] = reinterpret_cast<float(*)[BN + PAD]>(smem + KT * (BR + PAD));
  float(*D)[BN + DPAD] = reinterpret_cast<float(*)[BN + DPAD]>(smem);
  const int tid = threadIdx.x, tn = tid & 15, tr = tid >> 4;
  const int srow = tid >> 1, shalf = tid & 1;   // scan: lanes 2 r and 2 r + 1 share query row r
  const long r0 = (long)blockIdx.x * BR;
  const int split = blockIdx.y;
  const long n_lo = (long)split * per_split;
  const long n_hi = n_lo + per_split < N ? n_lo + per_split : N;
  float bd[KM];
  int bi[KM];
#pragma unroll
  for (int s = 0; s < KM; ++s) { bd[s] = INFINITY; bi[s] = INT_MAX; }
  for (long m0 = n_lo; m0 < n_hi; m0 += BN) {
    float tot[TR][TN];
#pragma unroll
    for (int i = 0; i < TR; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) tot[i][j] = 0.f;
    for (long k0 = 0; k0 < L; k0 += KT) {
      // out-of-range rows and k are zeros: (0 - 0)^2 adds an exact 0
#pragma unroll
      for (int s = 0; s < KT * BR / 256; ++s) {
        const int e = tid + 256 * s, kk = e & (KT - 1), rr = e / KT;
        const long gk = k0 + kk, gr = r0 + rr;
        Xs[kk][rr] = (gr < T && gk < L) ? q[gr * L + gk] : 0.f;
      }
#pragma unroll
      for (int s = 0; s < KT * BN / 256; ++s) {
        const int e = tid + 256 * s, kk = e & (KT - 1), rr = e / KT;
        const long gk = k0 + kk, gm = m0 + rr;
        Ws[kk][rr] = (gm < n_hi && gk < L) ? c[gm * L + gk] : 0.f;
      }
      __syncthreads();
      // this K tile's sum of (x - c)^2, each term one fma in ascending k; then tot += part (rv_som_bmu's two levels)
      float part[TR][TN];
#pragma unroll
      for (int i = 0; i < TR; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) part[i][j] = 0.f;
#pragma unroll 4
      for (int kk = 0; kk < KT; ++kk) {
        const f32x4 xa = *reinterpret_cast<const f32x4*>(&Xs[kk][tr * TR]);
        const f32x4 xb = *reinterpret_cast<const f32x4*>(&Xs[kk][tr * TR + 4]);
        const f32x4 wa = *reinterpret_cast<const f32x4*>(&Ws[kk][tn * TN]);
        const float xv[TR] = {xa[0], xa[1], xa[2], xa[3], xb[0], xb[1], xb[2], xb[3]};
        const float wv[TN] = {wa[0], wa[1], wa[2], wa[3]};
#pragma unroll
        for (int i = 0; i < TR; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            const float d = xv[i] - wv[j];
            part[i][j] = __builtin_fmaf(d, d, part[i][j]);
          }
      }
#pragma unroll
      for (int i = 0; i < TR; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) tot[i][j] += part[i][j];
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < TR; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) D[tr * TR + i][tn * TN + j] = tot[i][j];
    __syncthreads();
    const int nv = n_hi - m0 < BN ? (int)(n_hi - m0) : BN;
    for (int j = 0; j < BN / 2; ++j) {
      const int col = shalf * (BN / 2) + j;
      if (col < nv) topk_insert<KM>(D[srow][col], (int)(m0 + col), bd, bi);
    }
    __syncthreads();   // the next step stages over D
  }
  // merge the two lanes of a row: copy the partner's list first, then insert it
  float pd[KM];
  int pi[KM];
#pragma unroll
  for (int s = 0; s < KM; ++s) {
    pd[s] = __shfl_xor(bd[s], 1, 64);
    pi[s] = __shfl_xor(bi[s], 1, 64);
  }
#pragma unroll
  for (int s = 0; s < KM; ++s) topk_insert<KM>(pd[s], pi[s], bd, bi);
  const long r = r0 + srow;
  if (shalf == 0 && r < T) {
#pragma unroll
    for (int s = 0; s < KM; ++s) {
      if (s < k) {
        if (n_splits == 1) {
          idx[r * k + s] = bi[s] == INT_MAX ? -1 : bi[s];
          dist[r * k + s] = bd[s];
        } else {
          const long o = ((long)split * T + r) * k + s;
          ws_d[o] = bd[s];
          ws_i[o] = bi[s];
        }
      }
    }
  }
}

// One wave per query row (grid-stride): lane l keeps the top KM of the partials of splits l, l + 64, ..., then k
// rounds of a wave-wide minimum of the lanes' heads pop the result in (distance, index) order.
template <int KM>
__global__ void __launch_bounds__(256)
k_knn_merge(const float* __restrict__ ws_d, const int* __restrict__ ws_i, long T, int k, int n_splits,
            int* __restrict__ idx, float* __restrict__ dist) {
  const int lane = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < T; r += (long)gridDim.x * 4) {
    float bd[KM];
    int bi[KM];
#pragma unroll
    for (int s = 0; s < KM; ++s) { bd[s] = INFINITY; bi[s] = INT_MAX; }
    for (int sp = lane; sp < n_splits; sp += 64) {
      const long o = ((long)sp * T + r) * k;
      for (int j = 0; j < k; ++j) topk_insert<KM>(ws_d[o + j], ws_i[o + j], bd, bi);
    }
    for (int j = 0; j < k; ++j) {
      float wd = bd[0];
      int wi = bi[0];
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const float od = __shfl_xor(wd, off, 64);
        const int oi = __shfl_xor(wi, off, 64);
        if (cand_less(od, oi, wd, wi)) { wd = od; wi = oi; }
      }
      // corpus indices of different splits are distinct, so one lane holds the winner (none when it is empty)
      if (wi != INT_MAX && bi[0] == wi) {
#pragma unroll
        for (int s = 0; s + 1 < KM; ++s) { bd[s] = bd[s + 1]; bi[s] = bi[s + 1]; }
        bd[KM - 1] = INFINITY;
        bi[KM - 1] = INT_MAX;
      }
      if (lane == 0) {
        idx[r * k + j] = wi == INT_MAX ? -1 : wi;
        dist[r * k + j] = wd;
      }
    }
  }
}

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

unsigned blocks_for(long n, long cap) { return (unsigned)(n < 1 ? 1 : (n > cap ? cap : n)); }

// corpus rows per split (a multiple of BN) and the number of splits: enough (query tile, split) blocks to fill the
// chip, at least MIN_SPLIT_TILES corpus tiles per split; `forced` > 0 asks for that many splits instead
void knn_split(long T, long N, long forced, long* per_split, long* n_splits) {
  const long q_tiles = (T + BR - 1) / BR, n_tiles = (N + BN - 1) / BN;
  long want = forced > 0 ? forced : (TARGET_BLOCKS + q_tiles - 1) / q_tiles;
  if (forced <= 0 && want > n_tiles / MIN_SPLIT_TILES) want = n_tiles / MIN_SPLIT_TILES;
  if (want > n_tiles) want = n_tiles;
  if (want < 1) want = 1;
  const long tiles = (n_tiles + want - 1) / want;
  *per_split = tiles * BN;
  *n_splits = (n_tiles + tiles - 1) / tiles;
}

template <int KM>
void launch_knn(const rv_mosaic_desc* d, long per_split, long n_splits, float* ws_d, int* ws_i, hipStream_t st) {
  const dim3 grid((unsigned)((d->T + BR - 1) / BR), (unsigned)n_splits);
  hipLaunchKernelGGL(k_knn_topk<KM>, grid, dim3(256), 0, st, d->q, d->T, d->c, d->N, d->L, (int)d->k, per_split,
                     (int)n_splits, d->idx, d->dist, ws_d, ws_i);
  if (n_splits > 1)
    hipLaunchKernelGGL(k_knn_merge<KM>, dim3(blocks_for((d->T + 3) / 4, 65536)), dim3(256), 0, st, ws_d, ws_i, d->T,
                       (int)d->k, (int)n_splits, d->idx, d->dist);
}

int knn_check(const rv_mosaic_desc* d, long* per_split, long* n_splits) {
  RV_REQUIRE(d->T >= 1 && d->N >= 1 && d->L >= 1 && d->N < INT_MAX - BN, RV_ERR_SHAPE,
             "rv_mosaic(KNN): bad extents T=%ld N=%ld L=%ld", d->T, d->N, d->L);
  RV_REQUIRE(d->k >= 1 && d->k <= KMAX && d->k <= d->N, RV_ERR_SHAPE,
             "rv_mosaic(KNN): k=%ld must be in [1, %d] and at most N=%ld", d->k, KMAX, d->N);
  RV_REQUIRE(d->splits >= 0 && d->splits <= 65535, RV_ERR_SHAPE, "rv_mosaic(KNN): splits=%ld outside [0, 65535]",
             d->splits);
  RV_REQUIRE((d->T + BR - 1) / BR < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(KNN): T=%ld too large", d->T);
  knn_split(d->T, d->N, d->splits, per_split, n_splits);
  return RV_OK;
}

long knn_ws_bytes(long T, long k, long n_splits) { return n_splits > 1 ? n_splits * T * k * 8 : 0; }

}  // namespace

extern "C" int rv_mosaic(int op, rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d, RV_ERR_NULL, "rv_mosaic: null descriptor");
  const hipStream_t st = (hipStream_t)stream;
  long per_split = 0, n_splits = 0;
  switch (op) {
    case RV_MOSAIC_KNN_WORKSPACE: {
      const int rc = knn_check(d, &per_split, &n_splits);
      if (rc) return rc;
      d->ws_bytes = knn_ws_bytes(d->T, d->k, n_splits);
      return RV_OK;
    }
    case RV_MOSAIC_KNN: {
      RV_REQUIRE(d->q && d->c && d->idx && d->dist, RV_ERR_NULL, "rv_mosaic(KNN): null pointer");
      const int rc = knn_check(d, &per_split, &n_splits);
      if (rc) return rc;
      const long need = knn_ws_bytes(d->T, d->k, n_splits);
      RV_REQUIRE(need == 0 || (d->ws && d->ws_bytes >= need), RV_ERR_SHAPE,
                 "rv_mosaic(KNN): workspace of %ld bytes, %ld needed for %ld splits", d->ws_bytes, need, n_splits);
      float* ws_d = (float*)d->ws;
      int* ws_i = need ? (int*)((char*)d->ws + n_splits * d->T * d->k * 4) : nullptr;
      if (d->k <= 2) launch_knn<2>(d, per_split, n_splits, ws_d, ws_i, st);
      else if (d->k <= 4) launch_knn<4>(d, per_split, n_splits, ws_d, ws_i, st);
      else if (d->k <= 8) launch_knn<8>(d, per_split, n_splits, ws_d, ws_i, st);
      else launch_knn<16>(d, per_split, n_splits, ws_d, ws_i, st);
      RV_CHECK_LAUNCH();
      return RV_OK;
    }
    case RV_MOSAIC_GATHER_MEAN: {
      RV_REQUIRE(d->src && d->idx && d->out, RV_ERR_NULL, "rv_mosaic(GATHER_MEAN): null pointer");
      RV_REQUIRE(d->T >= 1 && d->k >= 1 && d->k <= KMAX && d->width >= 1 && d->n_rows >= 1 && d->src_len >= d->width &&
                     d->ldo >= d->width && (d->row_start || d->stride >= 0),
                 RV_ERR_SHAPE, "rv_mosaic(GATHER_MEAN): bad extents T=%ld k=%ld width=%ld n_rows=%ld src_len=%ld "
                 "ldo=%ld stride=%ld", d->T, d->k, d->width, d->n_rows, d->src_len, d->ldo, d->stride);
      hipLaunchKernelGGL(k_gather_mean, dim3(blocks_for(d->T, 65536)), dim3(256), 0, st, d->src, d->src_len,
                         d->row_start, d->stride, d->n_rows, d->width, d->idx, d->T, (int)d->k, d->out, d->ldo);
      RV_CHECK_LAUNCH();
      return RV_OK;
    }
    case RV_MOSAIC_OLA: {
      RV_REQUIRE(d->frames && d->out, RV_ERR_NULL, "rv_mosaic(OLA): null pointer");
      RV_REQUIRE(d->F >= 1 && d->S >= 1 && d->hop >= 1 && d->n_out >= 1, RV_ERR_SHAPE,
                 "rv_mosaic(OLA): bad extents F=%ld S=%ld hop=%ld n_out=%ld", d->F, d->S, d->hop, d->n_out);
      hipLaunchKernelGGL(k_ola, dim3(blocks_for((d->n_out + 255) / 256, 65536)), dim3(256), 0, st, d->frames, d->F,
                         d->S, d->hop, d->window, d->n_out, d->out);
      RV_CHECK_LAUNCH();
      return RV_OK;
    }
    default:
      RV_REQUIRE(false, RV_ERR_UNSUPPORTED, "rv_mosaic: unknown op %d", op);
  }
  return RV_OK;
}
