// The exact kNN search of latent mosaicing (rawaudiovae_kelsey_amd/mosaic.py): the k nearest corpus rows of every query
// row in sqdist.h's direct squared distances.  Four ops of rv_mosaic (mosaic.hip) and the live block's search
// (mosaic_live.hip):
//   RV_MOSAIC_KNN        k_knn_topk over (query tile, corpus split), then k_knn_merge of the per-split partials
//   RV_MOSAIC_KNN_SMALL  the same results for at most 64 query rows: k_knn_small, one thread per corpus row
//   RV_MOSAIC_KNN_WORKSPACE / _KNN_SMALL_WORKSPACE   the bytes of ws of the two
// Layout, split and merge, and the measured figures: DESIGN.md sections 7.5 and 7.6.
#include <limits.h>

#include "common.h"
#include "internal.h"
#include "sqdist.h"

using namespace rv;
using namespace rv::sqd;

namespace {

// k_knn_topk: sqdist.h's tile over BR query rows x BN corpus rows per step.  The finished BR x BN distance tile goes
// through LDS and is scanned by two lanes per query row, each keeping a sorted top-KM list in registers over its half
// of the corpus rows: 2 KM VGPRs per lane instead of 8 rows x 2 KM.
constexpr long TARGET_BLOCKS = 1024;   // 4 workgroups per CU of a 256-CU MI355X
constexpr long MIN_SPLIT_TILES = 4;    // corpus tiles per split before a search is split further

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
    tile_sq_dist(Xs, Ws, q, c, r0, m0, L, [&](long gr) { return gr < T; }, [&](long gm) { return gm < n_hi; }, tot);
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

// The lanes of a wave each hold a sorted list over disjoint corpus rows: k rounds of a wave-wide minimum of the lanes'
// heads pop the first k of their union in (distance, index) order; every lane sees each (j, distance, index) in `out`.
template <int KM, class Out>
__device__ __forceinline__ void topk_pop(float (&bd)[KM], int (&bi)[KM], int k, Out out) {
  for (int j = 0; j < k; ++j) {
    float wd = bd[0];
    int wi = bi[0];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float od = __shfl_xor(wd, off, 64);
      const int oi = __shfl_xor(wi, off, 64);
      if (cand_less(od, oi, wd, wi)) { wd = od; wi = oi; }
    }
    // the lanes' corpus indices are distinct, so one lane holds the winner (none when it is empty)
    if (wi != INT_MAX && bi[0] == wi) {
#pragma unroll
      for (int s = 0; s + 1 < KM; ++s) { bd[s] = bd[s + 1]; bi[s] = bi[s + 1]; }
      bd[KM - 1] = INFINITY;
      bi[KM - 1] = INT_MAX;
    }
    out(j, wd, wi);
  }
}

// One wave per query row (grid-stride): lane l keeps the top KM of the partials of splits l, l + 64, ..., then
// topk_pop gives the result in (distance, index) order.
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
    topk_pop<KM>(bd, bi, k, [&](int j, float wd, int wi) {
      if (lane == 0) {
        idx[r * k + j] = wi == INT_MAX ? -1 : wi;
        dist[r * k + j] = wd;
      }
    });
  }
}

// ---- The search for few query rows ----
// k_knn_topk pads its queries to tiles of BR = 128 rows; a live block has 1..16.  Here one thread owns one corpus row
// of a run of SRUN, a block walks the runs of its split, and a pass covers up to SQ query rows, so the corpus is read
// once per pass.  Each KT-wide slice of the run goes through LDS (16-byte global loads, eight lanes per row, one slice
// ahead in registers; row stride SLICE_ROW).  The query values are wave-uniform and come through the scalar cache.  A
// pair's arithmetic is sqdist.h's, a slice being a tile.  The run's TQ x SRUN distances go through LDS to SRUN / TQ
// lanes per query row, each with a sorted top-KM list; at the end one wave per query row merges them.
constexpr int SQ = 16, SRUN = 256, SLD4 = SRUN * (KT / 4) / 256;
static_assert(SMALL_T_MAX == 4 * SQ, "RV_MOSAIC_KNN_SMALL takes up to four passes");

// part = fmaf(d, d, part) with d = qv[x] - cv[x] for x = 0..3 in order, the wave-uniform qv read from their SGPRs: the
// instructions the compiler emits for the plain expression, written out because its SLP pass otherwise pairs the
// chains of neighbouring query rows into packed operations and first moves every query value into a VGPR (more VALU
// work than it saves).  v_sub_f32 and v_fmac_f32 round as the C expressions do.
__device__ __forceinline__ void sq_acc4_uniform(float& part, const float* __restrict__ qv, const f32x4& cv) {
  float d;
  asm("v_sub_f32 %1, %2, %6\n\tv_fmac_f32 %0, %1, %1\n\t"
      "v_sub_f32 %1, %3, %7\n\tv_fmac_f32 %0, %1, %1\n\t"
      "v_sub_f32 %1, %4, %8\n\tv_fmac_f32 %0, %1, %1\n\t"
      "v_sub_f32 %1, %5, %9\n\tv_fmac_f32 %0, %1, %1"
      : "+v"(part), "=&v"(d)
      : "s"(qv[0]), "s"(qv[1]), "s"(qv[2]), "s"(qv[3]), "v"(cv[0]), "v"(cv[1]), "v"(cv[2]), "v"(cv[3]));
}

template <int KM, int TQ, bool VEC>
__global__ void __launch_bounds__(256)
k_knn_small(const float* __restrict__ q, int T, const float* __restrict__ c, long N, long L, int k, long per_split,
            int n_splits, int* __restrict__ idx, float* __restrict__ dist, float* __restrict__ ws_d) {
  static_assert(SRUN * SLICE_ROW >= 2 * 256 * KM && SRUN * SLICE_ROW >= TQ * SRUN,
                "the lists and the distances fit the stage");
  __shared__ __attribute__((aligned(16))) float smem[SRUN * SLICE_ROW];
  constexpr int LPQ = SRUN / TQ;   // lanes per query row in the scan
  const int tid = threadIdx.x, srow = tid / LPQ, ssub = tid % LPQ;
  const int t0 = blockIdx.x * SQ, split = blockIdx.y;
  const long n_lo = (long)split * per_split;
  const long n_hi = n_lo + per_split < N ? n_lo + per_split : N;
  // wave-uniform offsets of the query rows (T * L < 2^31); rows past T repeat the last one and are not written
  auto q_row = [&](int i, int l) { return q + (t0 + i < T ? t0 + i : T - 1) * (int)L + l; };
  float bd[KM];
  int bi[KM];
#pragma unroll
  for (int s = 0; s < KM; ++s) { bd[s] = INFINITY; bi[s] = INT_MAX; }
  f32x4 pre[SLD4];
  // rows past n_hi and columns past L stage zeros
  auto fetch = [&](long m0, long k0) {
#pragma unroll
    for (int u = 0; u < SLD4; ++u) {
      const int e = tid + 256 * u;
      const long gm = m0 + (e >> 3), gk = k0 + (e & 7) * 4;
      pre[u] = gm < n_hi ? slice_fetch4(c + gm * L, gk, L, VEC) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  const float* crow = smem + tid * SLICE_ROW;
  fetch(n_lo, 0);
  for (long m0 = n_lo; m0 < n_hi; m0 += SRUN) {
    float tot[TQ];
#pragma unroll
    for (int i = 0; i < TQ; ++i) tot[i] = 0.f;
    for (long k0 = 0; k0 < L; k0 += KT) {
#pragma unroll
      for (int u = 0; u < SLD4; ++u) {
        const int e = tid + 256 * u;
        *reinterpret_cast<f32x4*>(smem + (e >> 3) * SLICE_ROW + (e & 7) * 4) = pre[u];
      }
      __syncthreads();
      const bool wrap = k0 + KT >= L;
      if (!wrap || m0 + SRUN < n_hi) fetch(wrap ? m0 + SRUN : m0, wrap ? 0 : k0 + KT);
      float part[TQ];
#pragma unroll
      for (int i = 0; i < TQ; ++i) part[i] = 0.f;
      if (k0 + KT <= L) {
        // the row's slice in registers, then one query row after the other: its KT values are two scalar loads
        f32x4 cv[KT / 4];
#pragma unroll
        for (int u = 0; u < KT / 4; ++u) cv[u] = *reinterpret_cast<const f32x4*>(crow + 4 * u);
#pragma unroll
        for (int i = 0; i < TQ; ++i) {
          const float* qr = q_row(i, (int)k0);
#pragma unroll
          for (int u = 0; u < KT / 4; ++u) sq_acc4_uniform(part[i], qr + 4 * u, cv[u]);
        }
      } else {
        // the last, partial slice: the terms past L would add an exact 0
        for (int kk = 0; k0 + kk < L; ++kk) {
          const float cv = crow[kk];
#pragma unroll
          for (int i = 0; i < TQ; ++i) {
            const float d = *q_row(i, (int)k0 + kk) - cv;
            part[i] = __builtin_fmaf(d, d, part[i]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < TQ; ++i) tot[i] += part[i];
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < TQ; ++i) smem[i * SRUN + tid] = tot[i];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TQ; ++j) {
      const int col = ssub + LPQ * j;
      if (m0 + col < n_hi) topk_insert<KM>(smem[srow * SRUN + col], (int)(m0 + col), bd, bi);
    }
    __syncthreads();   // the next run stages over the distances
  }
  // every thread's list goes to LDS; wave w merges the LPQ lists of query rows w, w + 4, ...
  float* ld = smem;
  int* li = reinterpret_cast<int*>(smem + 256 * KM);
#pragma unroll
  for (int s = 0; s < KM; ++s) {
    ld[tid * KM + s] = bd[s];
    li[tid * KM + s] = bi[s];
  }
  __syncthreads();
  const int lane = tid & 63;
  for (int r = tid >> 6; r < TQ; r += 4) {
#pragma unroll
    for (int s = 0; s < KM; ++s) { bd[s] = INFINITY; bi[s] = INT_MAX; }
    for (int x = lane; x < LPQ; x += 64) {
      const int o = (r * LPQ + x) * KM;
      for (int s = 0; s < KM; ++s) topk_insert<KM>(ld[o + s], li[o + s], bd, bi);
    }
    const int t = t0 + r;
    topk_pop<KM>(bd, bi, k, [&](int j, float wd, int wi) {
      if (lane == 0 && t < T) {
        if (n_splits == 1) {
          idx[t * k + j] = wi == INT_MAX ? -1 : wi;
          dist[t * k + j] = wd;
        } else {
          const long o = ((long)split * T + t) * k + j;     // the indices follow the n_splits * T * k distances
          ws_d[o] = wd;
          reinterpret_cast<int*>(ws_d + (long)n_splits * T * k)[o] = wi;
        }
      }
    });
  }
}

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

// k_knn_small's split: corpus rows per split (a multiple of SRUN) and the number of splits; enough (pass, split)
// blocks to fill the chip, down to one run per split; `forced` > 0 asks for that many splits instead
void knn_small_split(long T, long N, long forced, long* per_split, long* n_splits) {
  const long passes = (T + SQ - 1) / SQ, n_runs = (N + SRUN - 1) / SRUN;
  long want = forced > 0 ? forced : (TARGET_BLOCKS + passes - 1) / passes;
  if (want > n_runs) want = n_runs;
  if (want < 1) want = 1;
  const long runs = (n_runs + want - 1) / want;
  *per_split = runs * SRUN;
  *n_splits = (n_runs + runs - 1) / runs;
}

template <int KM, int TQ>
void launch_knn_small_q(const rv_mosaic_desc* d, long per_split, long n_splits, float* ws_d, int* ws_i, hipStream_t st) {
  const dim3 grid((unsigned)((d->T + SQ - 1) / SQ), (unsigned)n_splits);
  if (rows_vec16(d->c, d->L))
    hipLaunchKernelGGL((k_knn_small<KM, TQ, true>), grid, dim3(256), 0, st, d->q, (int)d->T, d->c, d->N, d->L, (int)d->k,
                       per_split, (int)n_splits, d->idx, d->dist, ws_d);
  else
    hipLaunchKernelGGL((k_knn_small<KM, TQ, false>), grid, dim3(256), 0, st, d->q, (int)d->T, d->c, d->N, d->L, (int)d->k,
                       per_split, (int)n_splits, d->idx, d->dist, ws_d);
  if (n_splits > 1)
    hipLaunchKernelGGL(k_knn_merge<KM>, dim3(blocks_for((d->T + 3) / 4, 65536)), dim3(256), 0, st, ws_d, ws_i, d->T,
                       (int)d->k, (int)n_splits, d->idx, d->dist);
}

template <int KM>
void launch_knn_small(const rv_mosaic_desc* d, long per_split, long n_splits, float* ws_d, int* ws_i, hipStream_t st) {
  if (d->T <= 1) launch_knn_small_q<KM, 1>(d, per_split, n_splits, ws_d, ws_i, st);
  else if (d->T <= 2) launch_knn_small_q<KM, 2>(d, per_split, n_splits, ws_d, ws_i, st);
  else if (d->T <= 4) launch_knn_small_q<KM, 4>(d, per_split, n_splits, ws_d, ws_i, st);
  else if (d->T <= 8) launch_knn_small_q<KM, 8>(d, per_split, n_splits, ws_d, ws_i, st);
  else launch_knn_small_q<KM, 16>(d, per_split, n_splits, ws_d, ws_i, st);
}

int knn_check(const rv_mosaic_desc* d, bool small, long* per_split, long* n_splits) {
  RV_REQUIRE(d->T >= 1 && d->N >= 1 && d->L >= 1 && d->N < INT_MAX - BN, RV_ERR_SHAPE,
             "rv_mosaic(KNN): bad extents T=%ld N=%ld L=%ld", d->T, d->N, d->L);
  RV_REQUIRE(d->k >= 1 && d->k <= KMAX && d->k <= d->N, RV_ERR_SHAPE,
             "rv_mosaic(KNN): k=%ld must be in [1, %d] and at most N=%ld", d->k, KMAX, d->N);
  RV_REQUIRE(d->splits >= 0 && d->splits <= 65535, RV_ERR_SHAPE, "rv_mosaic(KNN): splits=%ld outside [0, 65535]",
             d->splits);
  RV_REQUIRE((d->T + BR - 1) / BR < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(KNN): T=%ld too large", d->T);
  RV_REQUIRE(!small || (d->T <= SMALL_T_MAX && d->L <= (1L << 24)), RV_ERR_SHAPE,
             "rv_mosaic(KNN_SMALL): T=%ld above %d or L=%ld above 2^24, use RV_MOSAIC_KNN", d->T, SMALL_T_MAX, d->L);
  if (small) knn_small_split(d->T, d->N, d->splits, per_split, n_splits);
  else knn_split(d->T, d->N, d->splits, per_split, n_splits);
  return RV_OK;
}

long knn_ws_bytes(long T, long k, long n_splits) { return n_splits > 1 ? n_splits * T * k * 8 : 0; }

}  // namespace

int rv_knn_workspace(rv_mosaic_desc* d, int small) {
  long per_split = 0, n_splits = 0;
  const int rc = knn_check(d, small, &per_split, &n_splits);
  if (rc) return rc;
  d->ws_bytes = knn_ws_bytes(d->T, d->k, n_splits);
  return RV_OK;
}

// RV_MOSAIC_KNN / RV_MOSAIC_KNN_SMALL: checks, then the search and its merge on the stream
int rv_knn_search(const rv_mosaic_desc* d, int small, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  long per_split = 0, n_splits = 0;
  RV_REQUIRE(d->q && d->c && d->idx && d->dist, RV_ERR_NULL, "rv_mosaic(KNN): null pointer");
  const int rc = knn_check(d, small, &per_split, &n_splits);
  if (rc) return rc;
  const long need = knn_ws_bytes(d->T, d->k, n_splits);
  RV_REQUIRE(need == 0 || (d->ws && d->ws_bytes >= need), RV_ERR_SHAPE,
             "rv_mosaic(KNN): workspace of %ld bytes, %ld needed for %ld splits", d->ws_bytes, need, n_splits);
  float* ws_d = (float*)d->ws;
  int* ws_i = need ? (int*)((char*)d->ws + n_splits * d->T * d->k * 4) : nullptr;
  if (small) {
    if (d->k <= 2) launch_knn_small<2>(d, per_split, n_splits, ws_d, ws_i, st);
    else if (d->k <= 4) launch_knn_small<4>(d, per_split, n_splits, ws_d, ws_i, st);
    else if (d->k <= 8) launch_knn_small<8>(d, per_split, n_splits, ws_d, ws_i, st);
    else launch_knn_small<16>(d, per_split, n_splits, ws_d, ws_i, st);
  } else {
    if (d->k <= 2) launch_knn<2>(d, per_split, n_splits, ws_d, ws_i, st);
    else if (d->k <= 4) launch_knn<4>(d, per_split, n_splits, ws_d, ws_i, st);
    else if (d->k <= 8) launch_knn<8>(d, per_split, n_splits, ws_d, ws_i, st);
    else launch_knn<16>(d, per_split, n_splits, ws_d, ws_i, st);
  }
  RV_CHECK_LAUNCH();
  return RV_OK;
}
