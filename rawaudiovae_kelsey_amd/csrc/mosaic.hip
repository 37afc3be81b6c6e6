// Latent audio mosaicing (rawaudiovae_kelsey_amd/mosaic.py): frame-level nearest neighbours in the latent space and
// the synthesis built on them, behind the one entry point rv_mosaic(op, desc, stream):
//   RV_MOSAIC_KNN          k nearest corpus rows of every query row, direct squared distances (the hot path):
//                          k_knn_topk over (query tile, corpus split), then k_knn_merge of the per-split partials
//   RV_MOSAIC_GATHER_MEAN  out[t] = (1/k) sum_j src[start(idx[t, j]) : + width] (grains or latent rows)
//   RV_MOSAIC_OLA          offline weighted overlap-add normalised by the window sum
//   RV_MOSAIC_TRANSITION   candidate-to-candidate concatenation costs [rows, k, k] in the search's arithmetic
//   RV_MOSAIC_PATH_FORWARD / _BACKTRACK   Viterbi unit selection over the k candidates of every row (one wave each)
//   RV_MOSAIC_KNN_SMALL    RV_MOSAIC_KNN's results for at most 64 query rows: k_knn_small, one thread per corpus row
//   RV_MOSAIC_LIVE         one block of live audio: the stream's encoder (stream.hip), the search, unit selection
//                          (k_live_select: greedy; k_live_lag: Viterbi over a window of lag + 1 frames, committing
//                          the oldest), gather-mean, then the stream's decoder / overlap-add
//   RV_MOSAIC_LIVE_DRAIN   one block that plays out the frames a lag still holds back: no encoder, no search
//   RV_GRAIN_FIT / RV_GRAIN_GATHER   shift-and-gain fit of every candidate grain to its target frame: grain.hip
//   RV_EVAL_FRAMES / RV_EVAL_DIMS    held-out evaluation, per-frame scores and per-dimension KL sums: eval.hip
// Layout, split and merge, and the measured figures: DESIGN.md sections 7.5, 7.6 and 7.7.
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
constexpr int KMAX = 16;
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
// Query rows RV_MOSAIC_KNN_SMALL accepts, and up to which RV_MOSAIC_LIVE searches with it: measured faster than
// k_knn_topk at every T up to here (1.4-1.9x at 64 rows, 4-10x at 16 and fewer against 1.24 M corpus rows; section 7.6)
constexpr int SMALL_T_MAX = 4 * SQ;

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

// ---- Unit selection over the candidates ("Continuity") ----

// Every kernel of the unit selection (k_transition, k_live_select, k_live_lag) takes its costs from sqdist.h's pair
// form, so that they are k_knn_topk's bit for bit.  k_transition stages latent rows in LDS tile by tile (KT elements,
// row stride SLICE_ROW).
constexpr int TRB_MAX = 32;   // rows of T per workgroup at most

// KP = k rounded up to a power of two: a workgroup covers RB rows of T, one thread per (row, i, j) pair, and stages
// NR = RB * 2 KP latent rows per tile (KP successor rows, then KP candidate rows, per row of T).
template <int KP>
struct trans_cfg {
  static constexpr int PP = KP * KP;
  static constexpr int RB = 256 / PP < TRB_MAX ? 256 / PP : TRB_MAX;
  static constexpr int NR = RB * 2 * KP;
  static constexpr int LD4 = (NR * (KT / 4) + 255) / 256;   // 16-byte loads per thread and tile
};

// trans[t - row0, i, j] = D(mu[next_of[idx[t-1, i]]], mu[idx[t, j]]), D being sqdist.h's.  Missing candidates (and
// indices outside [0, N)) stage zeros and give +inf.  The next tile's rows are loaded into registers while this one is
// summed.
template <int KP>
__global__ void __launch_bounds__(256)
k_transition(const float* __restrict__ mu, long N, long L, const int* __restrict__ next_of,
             const int* __restrict__ idx, int k, long row0, long rows, int vec, float* __restrict__ trans) {
  using C = trans_cfg<KP>;
  __shared__ __attribute__((aligned(16))) float V[C::NR][SLICE_ROW];
  __shared__ int src[C::NR];
  const int tid = threadIdx.x;
  const long tb = row0 + (long)blockIdx.x * C::RB, t_end = row0 + rows;
  for (int e = tid; e < C::NR; e += 256) {
    const int r = e / (2 * KP), w = e % (2 * KP);
    const long t = tb + r;
    int s = -1;
    if (t < t_end && t >= 1) {
      if (w < KP) {
        if (w < k) {
          const int a = idx[(t - 1) * k + w];
          if (a >= 0 && a < N) s = next_of[a];
        }
      } else if (w - KP < k) {
        s = idx[t * k + (w - KP)];
      }
      if (s < 0 || s >= N) s = -1;
    }
    src[e] = s;
  }
  __syncthreads();
  f32x4 pre[C::LD4];
  auto fetch = [&](long k0) {
#pragma unroll
    for (int u = 0; u < C::LD4; ++u) {
      const int e = tid + 256 * u, row = e >> 3, c = (e & 7) * 4;
      const int s = e < C::NR * (KT / 4) ? src[row] : -1;
      pre[u] = s >= 0 ? slice_fetch4(mu + (long)s * L, k0 + c, L, vec) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  const int r = tid / C::PP, pr = tid % C::PP, i = pr / KP, j = pr % KP;
  const bool active = tid < C::RB * C::PP;
  const int ra = active ? r * 2 * KP + i : 0, rb = active ? r * 2 * KP + KP + j : 0;
  float tot = 0.f;
  fetch(0);
  for (long k0 = 0; k0 < L; k0 += KT) {
#pragma unroll
    for (int u = 0; u < C::LD4; ++u) {
      const int e = tid + 256 * u;
      if (e < C::NR * (KT / 4)) *reinterpret_cast<f32x4*>(&V[e >> 3][(e & 7) * 4]) = pre[u];
    }
    __syncthreads();
    if (k0 + KT < L) fetch(k0 + KT);
    if (active) {
      float part = 0.f;
#pragma unroll
      for (int kk = 0; kk < KT; kk += 4) {
        const f32x4 xa = *reinterpret_cast<const f32x4*>(&V[ra][kk]);
        const f32x4 wb = *reinterpret_cast<const f32x4*>(&V[rb][kk]);
        sq_acc4(part, xa, wb);
      }
      tot += part;
    }
    __syncthreads();
  }
  const long t = tb + r;
  if (active && t < t_end && i < k && j < k) {
    float v = 0.f;   // row 0 has no predecessor: all 0
    if (t >= 1) v = (src[ra] >= 0 && src[rb] >= 0 && tot == tot) ? tot : INFINITY;
    trans[((t - row0) * k + i) * k + j] = v;
  }
}

constexpr int PATH_NONE = 255;   // back / end byte: no predecessor, no finite score
constexpr int PATH_PF = 16;      // rows of trans, dist and idx held in registers ahead of the dependent chain
constexpr int BT_CH = 256;       // rows per staged chunk of the backtrack

__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// workspace of the PATH ops for (T, k): the last row's scores [16] fp32, the transition cost met at (t, j) [T, k] fp32,
// back [T, k] bytes, end [T] bytes; every part starts on a 16-byte boundary
struct path_ws {
  long btr, back, end, bytes;
};
path_ws path_layout(long T, long k) {
  path_ws w;
  w.btr = 64;
  w.back = (w.btr + 4 * T * k + 15) & ~15L;
  w.end = (w.back + T * k + 15) & ~15L;
  w.bytes = (w.end + T + 15) & ~15L;
  return w;
}

// v of another lane by a DPP move: quad_perm [1,0,3,2] / [2,3,0,1] (lane ^ 1, lane ^ 2) and row_ror:4 / :8 (the lane
// 4 or 8 further on in its row of 16) -- a few cycles, where a shuffle through the LDS crossbar takes a round trip
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_ROR4 = 0x124, DPP_ROR8 = 0x128;
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) { return __int_as_float(dpp_i<CTRL>(__float_as_int(v))); }

// (v, i) becomes the better of itself and (ov, oi): smaller value, then lower index (i = PATH_NONE where v is +inf).
// The order is total, so an all-reduce gives every lane the same pair whatever the exchange pattern.
__device__ __forceinline__ void path_take(float& v, int& i, float ov, int oi) {
  if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// over the 4 lanes of a column (q = lane & 3)
__device__ __forceinline__ void path_min_q(float& v, int& i) {
  path_take(v, i, dpp_f<DPP_XOR1>(v), dpp_i<DPP_XOR1>(i));
  path_take(v, i, dpp_f<DPP_XOR2>(v), dpp_i<DPP_XOR2>(i));
}
// over the 16 columns (j = lane >> 2): the 4 columns of a row of 16 lanes by rotations, the 4 rows by shuffles
__device__ __forceinline__ void path_min_j(float& v, int& i) {
  path_take(v, i, dpp_f<DPP_ROR8>(v), dpp_i<DPP_ROR8>(i));
  path_take(v, i, dpp_f<DPP_ROR4>(v), dpp_i<DPP_ROR4>(i));
  path_take(v, i, __shfl_xor(v, 16, 64), __shfl_xor(i, 16, 64));
  path_take(v, i, __shfl_xor(v, 32, 64), __shfl_xor(i, 32, 64));
}

// The forward rule's pieces, shared by k_path_forward and k_live_lag; lane = 4 j + q as described below.
// fl(lambda * trans), never 0 * inf
__device__ __forceinline__ float path_weigh(float lam, float tr) { return tr < INFINITY ? mul_rn(lam, tr) : INFINITY; }
// a candidate's own cost: +inf for a missing candidate or NaN
__device__ __forceinline__ float path_target(bool jv, int ci, float d) { return (jv && ci >= 0 && d == d) ? d : INFINITY; }
// hands every lane the new scores of its 4 predecessors (raw, not yet reduced by their minimum) and the row's
// (minimum, lowest-j argmin)
__device__ __forceinline__ void path_spread(float nw, int j, int q, float (&raw)[4], float& m, int& mj) {
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) raw[ii] = __shfl(nw, (4 * q + ii) * 4, 64);
  m = nw;
  mj = j;
  path_min_j(m, mj);
}
// One row: p = the weighted transitions from this lane's 4 predecessors into column j, tg = column j's own cost.
// Updates the carried (nw, raw, m, mj) and returns back[t, j] (PATH_NONE where the row starts a sequence: `first`, or
// no new[j] finite).
__device__ __forceinline__ int path_step(const float (&p)[4], float tg, bool first, int j, int q, float& nw,
                                         float (&raw)[4], float& m, int& mj) {
  const bool fin = m < INFINITY;
  float best = INFINITY;
  int bi = PATH_NONE;
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const float c = (fin ? raw[ii] - m : raw[ii]) + p[ii];   // +inf where s[i] or the transition is
    if (c < best) { best = c; bi = 4 * q + ii; }
  }
  path_min_q(best, bi);
  nw = bi != PATH_NONE ? tg + best : INFINITY;
  int bk = nw < INFINITY ? bi : PATH_NONE;
  path_spread(nw, j, q, raw, m, mj);
  if (first || !(m < INFINITY)) {   // wave-uniform: the row starts a new sequence
    nw = tg;
    bk = PATH_NONE;
    path_spread(nw, j, q, raw, m, mj);
  }
  return bk;
}
// the backtrack's step from row t to row t - 1: b = back[t, slot[t]] (PATH_NONE for a row without a slot), e = end[t - 1]
__device__ __forceinline__ int path_back(int b, int e, int k) {
  if (b >= k) b = PATH_NONE;
  return b != PATH_NONE ? b : (e < k ? e : -1);
}

// The forward pass of rows [row0, row0 + rows): ONE wave, lane = 4 j + q owns column j and the predecessors
// i = 4 q .. 4 q + 3.  Per row the dependent chain is: 4 adds and compares, 2 DPP steps over q, + dist, 2 DPP and 2
// shuffle steps over j (minimum and end), while the 4 shuffles that hand every lane its predecessors' new scores run
// beside them.  trans, dist and idx of the next PATH_PF rows are already in registers, raw (a static ring; the loop
// is unrolled by PATH_PF; nothing is consumed at load time, so no wait follows a load): every lane loads from a
// clamped, valid address and masks what it does not own when it uses it.  fl(lambda * trans) is formed off the chain.
__global__ void __launch_bounds__(64)
k_path_forward(const float* __restrict__ trans, const int* __restrict__ idx, const float* __restrict__ dist, int k,
               long row0, long rows, float lam, float* __restrict__ score, float* __restrict__ btr,
               unsigned char* __restrict__ back, unsigned char* __restrict__ end) {
  const int lane = threadIdx.x, j = lane >> 2, q = lane & 3;
  const bool jv = j < k;
  const int jc = jv ? j : k - 1;
  float trr[PATH_PF][4], tdr[PATH_PF];
  int tir[PATH_PF], ioff[4];
  bool iv[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    iv[ii] = jv && 4 * q + ii < k;
    ioff[ii] = (4 * q + ii < k ? 4 * q + ii : k - 1) * k;
  }
  // running per-lane pointers: rows are loaded, and written, strictly in order; past the last row they stay on it
  const float* tp = trans + jc;
  const float* dp = dist + row0 * k + jc;
  const int* ip = idx + row0 * k + jc;
  const long kk = (long)k * k;
  long ld = 0;   // the next row to load
  auto load = [&](int s) {
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) trr[s][ii] = tp[ioff[ii]];
    tdr[s] = *dp;
    tir[s] = *ip;
    ++ld;
    const bool more = ld < rows;   // wave-uniform
    tp += more ? kk : 0;
    dp += more ? k : 0;
    ip += more ? k : 0;
  };
#pragma unroll
  for (int s = 0; s < PATH_PF; ++s) load(s);
  // the carried scores: raw (not yet reduced by their minimum); a call at row 0 starts from nothing
  float nw = (row0 > 0 && jv) ? score[j] : INFINITY;
  float m, raw[4];
  int mj;
  path_spread(nw, j, q, raw, m, mj);
  unsigned char* bp = back + row0 * k + j;
  float* mp = btr + row0 * k + j;
  for (long base = 0; base < rows; base += PATH_PF) {
#pragma unroll
    for (int s = 0; s < PATH_PF; ++s) {
      const long tl = base + s;
      if (tl < rows) {
        const long t = row0 + tl;
        float tr[4], p[4];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
          tr[ii] = iv[ii] ? trr[s][ii] : INFINITY;
          p[ii] = path_weigh(lam, tr[ii]);
        }
        float tg = path_target(jv, tir[s], tdr[s]);
        // pin tg here: computed any later, the ring slot's old value would outlive the load that refills it, and the
        // ring would be copied (behind a full wait) at the loop's back edge
        asm volatile("" : "+v"(tg));
        load(s);
        const int bk = path_step(p, tg, t == 0, j, q, nw, raw, m, mj);
        // the lane that holds the chosen predecessor's transition cost writes (t, j)
        if (jv && q == (bk == PATH_NONE ? 0 : bk >> 2)) {
          const int w = bk & 3;
          const float tv = w == 0 ? tr[0] : (w == 1 ? tr[1] : (w == 2 ? tr[2] : tr[3]));
          *bp = (unsigned char)bk;
          *mp = bk == PATH_NONE ? 0.f : tv;
        }
        bp += k;
        mp += k;
        if (lane == 0) end[t] = (unsigned char)(m < INFINITY ? mj : PATH_NONE);
      }
    }
  }
  if (jv && q == 0) score[j] = nw;
}

// slot, choice and the two cost sums: ONE wave.  Descending chunks of BT_CH rows: all lanes stage back and end in
// LDS, lane 0 walks the chunk, all lanes write slot and choice.  Then ascending chunks: all lanes stage the path's
// dist and transition cost, lane 0 adds them in fp64 in ascending t.
__global__ void __launch_bounds__(64)
k_path_backtrack(const int* __restrict__ idx, const float* __restrict__ dist, long T, int k,
                 const float* __restrict__ btr, const unsigned char* __restrict__ back,
                 const unsigned char* __restrict__ end, int* __restrict__ slot, int* __restrict__ choice,
                 double* __restrict__ cost) {
  __shared__ __attribute__((aligned(16))) unsigned char backL[BT_CH * KMAX];
  __shared__ unsigned char endL[BT_CH];
  __shared__ int slotL[BT_CH];
  __shared__ float v0L[BT_CH], v1L[BT_CH];
  __shared__ int curL;
  const int lane = threadIdx.x;
  if (lane == 0) curL = end[T - 1] == PATH_NONE ? -1 : end[T - 1];
  for (long c0 = (T - 1) / BT_CH * BT_CH; c0 >= 0; c0 -= BT_CH) {
    const int n = T - c0 < BT_CH ? (int)(T - c0) : BT_CH;
    // c0 * k is a multiple of 4 and `back` starts on a 16-byte boundary: whole words; the last word may reach up to
    // 3 bytes past back's T * k, which the workspace's layout covers
    const unsigned* bw = reinterpret_cast<const unsigned*>(back + c0 * k);
    for (int x = lane; x < (n * k + 3) / 4; x += 64) reinterpret_cast<unsigned*>(backL)[x] = bw[x];
    for (int x = lane; x < n; x += 64) endL[x] = c0 + x >= 1 ? end[c0 + x - 1] : PATH_NONE;   // end[t - 1]
    __syncthreads();
    if (lane == 0) {
      int c = curL;
      for (int x = n - 1; x >= 0; --x) {
        slotL[x] = c;
        if (c0 + x > 0) {
          const int e = endL[x];
          c = path_back(c < 0 ? PATH_NONE : backL[x * k + c], e, k);
        }
      }
      curL = c;
    }
    __syncthreads();
    for (int x = lane; x < n; x += 64) {
      const long t = c0 + x;
      const int s = slotL[x];
      slot[t] = s;
      choice[t] = s >= 0 ? idx[t * k + s] : -1;
    }
    __syncthreads();
  }
  double a0 = 0.0, a1 = 0.0;
  for (long c0 = 0; c0 < T; c0 += BT_CH) {
    const int n = T - c0 < BT_CH ? (int)(T - c0) : BT_CH;
    for (int x = lane; x < n; x += 64) {
      const long t = c0 + x;
      const int s = slot[t];   // this wave's own stores, ordered by the barriers above
      v0L[x] = s >= 0 ? dist[t * k + s] : 0.f;
      v1L[x] = s >= 0 ? btr[t * k + s] : 0.f;
    }
    __syncthreads();
    if (lane == 0)
      for (int x = 0; x < n; ++x) {
        a0 += (double)v0L[x];
        a1 += (double)v1L[x];
      }
    __syncthreads();
  }
  if (lane == 0) {
    cost[0] = a0;
    cost[1] = a1;
  }
}

// ---- Live mosaicing: greedy unit selection ----
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// The cost of entering a frame from the stream's previous choice p, lane j < k (own) holding candidate ci = idx[t, j]
// and dp = &dist[t, j]: succ = next_of[p] (-1 when p or it lies outside [0, N)); with a successor,
// cost = dist + fl(w * D(c[succ], c[ci])) in the search's arithmetic.  Returns whether the candidate stands: a corpus
// row whose cost is not NaN.
__device__ __forceinline__ bool live_entry(const float* __restrict__ c, long N, long L, const int* __restrict__ next_of,
                                           int p, int ci, const float* __restrict__ dp, float w, bool own, int vec,
                                           int& succ, float& cost) {
  bool valid = own && ci >= 0 && ci < N;
  succ = -1;
  if (p >= 0 && p < N) succ = next_of[p];
  if (succ < 0 || succ >= N) succ = -1;
  cost = 0.f;
  if (succ >= 0) {   // wave-uniform
    const float* a = c + (long)succ * L;
    const float* b = c + (long)(valid ? ci : 0) * L;
    const float tot = vec ? row_sq_dist4(a, b, L) : row_sq_dist(a, b, L);
    cost = add_rn(*dp, mul_rn(w, tot));
    valid = valid && cost == cost;
  }
  return valid;
}

// a weight that is not finite and >= 0 counts as 0
__device__ __forceinline__ float live_weight(float w) { return (w >= 0.f && w < INFINITY) ? w : 0.f; }

// One wave per stream, its F frames in order; lane j owns candidate j of the frame.  prev < 0 (or without a successor
// in the table): the lowest j whose candidate is a corpus row.  Otherwise lane j walks D(c[next_of[prev]], c[idx[r, j]])
// in the search's arithmetic and the wave takes the least dist + fl(w * D), strict < in ascending j, NaN skipped.
__global__ void __launch_bounds__(64)
k_live_select(const float* __restrict__ c, long N, long L, const int* __restrict__ next_of, const int* __restrict__ idx,
              const float* __restrict__ dist, int k, long F, const float* __restrict__ weight, int* __restrict__ prev,
              int* __restrict__ choice) {
  const long s = blockIdx.x;
  const int lane = threadIdx.x, jl = lane < k ? lane : k - 1;
  const float w = live_weight(weight[s]);
  int p = prev[s];
  for (long f = 0; f < F; ++f) {
    const long r = s * F + f;
    const int ci = idx[r * k + jl];
    int succ;
    float cost;
    const bool valid = live_entry(c, N, L, next_of, p, ci, dist + r * k + jl, w, lane < k, 0, succ, cost);
    int slot = -1;
    float best = 0.f;
    for (int j = 0; j < k; ++j) {
      const float cj = __shfl(cost, j, 64);
      const bool vj = __shfl((int)valid, j, 64) != 0;
      if (vj && (slot < 0 || (succ >= 0 && cj < best))) { best = cj; slot = j; }
    }
    p = slot >= 0 ? __shfl(ci, slot, 64) : -1;
    if (lane == 0) choice[r] = p;
  }
  if (lane == 0) prev[s] = p;
}

// ---- Live mosaicing with look-ahead: fixed-lag Viterbi unit selection ----
constexpr int LAG_MAX = 64;   // frames of look-ahead at most: a window holds up to LAG_MAX + 1 rows
constexpr int LAG_PF = 8;     // ring rows held in registers ahead of the forward pass's dependent chain

// One window solve by ONE wave (all 64 lanes; k_path_forward's layout, lane = 4 j + q): the n pending rows of a stream
// start at ring row `head`.  The oldest row's scores are live_entry's costs from the previous choice p, the rows after
// it follow path_step over their raw transitions weighted by w; back and end go to LDS, lane 0 walks them back to the
// oldest row.  Returns the corpus frame committed for that row (-1: it has no candidate), in every lane.
__device__ __forceinline__ int lag_solve(const float* __restrict__ c, long N, long L, const int* __restrict__ next_of,
                                         int k, float w, int p, int vec, const int* ri, const float* rd, const float* rt,
                                         int head, int n, int R, unsigned char* backL, unsigned char* endL) {
  const int lane = threadIdx.x & 63, j = lane >> 2, q = lane & 3;
  const bool jv = j < k;
  const int jc = jv ? j : k - 1, jl = lane < k ? lane : k - 1;
  const long kk = (long)k * k;
  float trr[LAG_PF][4], tdr[LAG_PF];
  int tir[LAG_PF], ioff[4];
  bool iv[4];
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    iv[ii] = jv && 4 * q + ii < k;
    ioff[ii] = (4 * q + ii < k ? 4 * q + ii : k - 1) * k;
  }
  // rows 1 .. n - 1 of the window are loaded strictly in order, the ring position wrapping at R; past the last row
  // (and with n = 1) the position stays on a row of the window: every load reads a valid address
  int lpos = n > 1 ? (head + 1 == R ? 0 : head + 1) : head, ld = 1;
  auto load = [&](int s) {
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) trr[s][ii] = rt[lpos * kk + ioff[ii] + jc];
    tdr[s] = rd[lpos * k + jc];
    tir[s] = ri[lpos * k + jc];
    ++ld;
    if (ld < n) lpos = lpos + 1 == R ? 0 : lpos + 1;   // wave-uniform
  };
#pragma unroll
  for (int s = 0; s < LAG_PF; ++s) load(s);
  // the oldest row: lane l < k owns its candidate l
  const int ci = ri[head * k + jl];
  const float* dp = rd + head * k + jl;
  int succ;
  float cost;
  const bool valid = live_entry(c, N, L, next_of, p, ci, dp, w, lane < k, vec, succ, cost);
  float e = succ >= 0 ? cost : *dp;
  if (!valid || !(e == e)) e = INFINITY;
  e = __shfl(e, jc, 64);
  float nw = jv ? e : INFINITY;
  float m, raw[4];
  int mj;
  path_spread(nw, j, q, raw, m, mj);
  if (lane == 0) endL[0] = (unsigned char)(m < INFINITY ? mj : PATH_NONE);
  for (int base = 1; base < n; base += LAG_PF) {
#pragma unroll
    for (int s = 0; s < LAG_PF; ++s) {
      const int r = base + s;
      if (r < n) {
        float pw[4];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) pw[ii] = path_weigh(w, iv[ii] ? trr[s][ii] : INFINITY);
        float tg = path_target(jv, tir[s], tdr[s]);
        asm volatile("" : "+v"(tg));   // as in k_path_forward: the ring slot is free before its refill is issued
        load(s);
        const int bk = path_step(pw, tg, false, j, q, nw, raw, m, mj);
        if (jv && q == 0) backL[r * KMAX + j] = (unsigned char)bk;
        if (lane == 0) endL[r] = (unsigned char)(m < INFINITY ? mj : PATH_NONE);
      }
    }
  }
  // this wave's own LDS stores, in order; the fence keeps the compiler from moving the walk above them
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  int slot = -1;
  if (lane == 0) {
    slot = path_back(PATH_NONE, endL[n - 1], k);
    for (int r = n - 1; r >= 1; --r) slot = path_back(slot < 0 ? PATH_NONE : backL[r * KMAX + slot], endL[r - 1], k);
  }
  slot = __shfl(slot, 0, 64);
  return slot >= 0 ? ri[head * k + slot] : -1;
}

// Selection with a lag of R - 1 frames: one workgroup per stream, its frames in order.  The stream's pending rows (idx,
// dist and the raw transitions from the row before, [R] each) live in a ring in the workspace with (head, count) in
// `state`; prev is k_live_select's.  push != 0, per new frame: (a) all threads, one per (i, j) pair: the frame's
// transition row against the last pending row, in k_transition's arithmetic, stored raw beside its idx and dist;
// (b) wave 0: once R rows are pending, lag_solve commits the oldest.  choice[r] = that corpus frame, -1 while fewer
// rows are pending.  push == 0 (drain): no new rows; up to F times, lag_solve on the shrinking window while rows are
// pending, -1 after.  No index is used as an address before it is checked against [0, N).  The ring is written by
// some threads and read by others across the barriers, so its pointers are not __restrict__.
// stamp != NULL (a grain fit follows): every pending row also keeps the frame count at which it arrived, fcnt[s] + f,
// in stamp [n_streams, R], and tfr[r] = the committed row's stamp: the target frame it stands for.  Thread 0 alone
// writes and reads the stamps.
__global__ void __launch_bounds__(256)
k_live_lag(const float* __restrict__ c, long N, long L, const int* __restrict__ next_of, const int* __restrict__ idx,
           const float* __restrict__ dist, int k, long F, int push, int R, int vec, const float* __restrict__ weight,
           int* __restrict__ prev, int* __restrict__ state, int* ridx, float* rdist, float* rtrans,
           int* __restrict__ choice, const long long* __restrict__ fcnt, long long* stamp, long long* __restrict__ tfr) {
  __shared__ unsigned char backL[(LAG_MAX + 1) * KMAX];
  __shared__ unsigned char endL[LAG_MAX + 1];
  const long s = blockIdx.x;
  const int tid = threadIdx.x;
  const int kk = k * k;
  int* ri = ridx + s * R * k;
  float* rd = rdist + s * R * k;
  float* rt = rtrans + s * R * kk;
  // between calls at most R - 1 rows are pending; anything else in the workspace counts as an empty ring
  int head = state[2 * s], cnt = state[2 * s + 1];
  if (head < 0 || head >= R || cnt < 0 || cnt >= R) head = cnt = 0;
  const float w = live_weight(weight[s]);
  int p = prev[s];
  const int pi = tid / k, pj = tid - pi * k;
  for (long f = 0; f < F; ++f) {
    const long r = s * F + f;
    if (push) {
      const int pos = (head + cnt) % R;   // free: cnt < R here
      if (tid < kk) {
        float v = INFINITY;
        if (cnt > 0) {
          const int ia = ri[(pos == 0 ? R - 1 : pos - 1) * k + pi], ib = idx[r * k + pj];
          int succ = -1;
          if (ia >= 0 && ia < N) succ = next_of[ia];
          if (succ >= 0 && succ < N && ib >= 0 && ib < N) {
            const float* a = c + (long)succ * L;
            const float* b = c + (long)ib * L;
            const float tot = vec ? row_sq_dist4(a, b, L) : row_sq_dist(a, b, L);
            if (tot == tot) v = tot;
          }
        }
        rt[pos * kk + tid] = v;
      }
      if (tid < k) {
        ri[pos * k + tid] = idx[r * k + tid];
        rd[pos * k + tid] = dist[r * k + tid];
      }
      if (stamp && tid == 0) stamp[s * R + pos] = fcnt[s] + f;
      ++cnt;
      __syncthreads();   // the row is in the ring for wave 0, and for the next frame's transitions
    }
    if (push ? cnt == R : cnt > 0) {   // uniform over the workgroup
      if (tid < 64) {
        p = lag_solve(c, N, L, next_of, k, w, p, vec, ri, rd, rt, head, cnt, R, backL, endL);
        if (tid == 0) {
          choice[r] = p;
          if (stamp) tfr[r] = stamp[s * R + head];
        }
      }
      head = head + 1 == R ? 0 : head + 1;
      --cnt;
    } else if (tid == 0) {
      choice[r] = -1;
    }
    __syncthreads();   // wave 0 has read the committed row before the next frame overwrites it
  }
  if (tid == 0) {
    prev[s] = p;
    state[2 * s] = head;
    state[2 * s + 1] = cnt;
  }
}

__global__ void __launch_bounds__(256) k_live_lag_clear(int* __restrict__ state, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < 2 * n) state[i] = 0;
}

__global__ void __launch_bounds__(256) k_live_clear(int* __restrict__ prev, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) prev[i] = -1;
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

template <int KP>
void launch_transition(const rv_mosaic_desc* d, int vec, hipStream_t st) {
  const long rb = trans_cfg<KP>::RB;
  hipLaunchKernelGGL(k_transition<KP>, dim3((unsigned)((d->rows + rb - 1) / rb)), dim3(256), 0, st, d->c, d->N, d->L,
                     d->next_of, d->idx, (int)d->k, d->row0, d->rows, vec, d->trans);
}

int path_check(const rv_mosaic_desc* d, const char* op, bool chunk) {
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 40), RV_ERR_SHAPE, "rv_mosaic(%s): T=%ld outside [1, 2^40)", op, d->T);
  RV_REQUIRE(d->k >= 1 && d->k <= KMAX, RV_ERR_SHAPE, "rv_mosaic(%s): k=%ld must be in [1, %d]", op, d->k, KMAX);
  if (chunk)
    RV_REQUIRE(d->row0 >= 0 && d->rows >= 1 && d->row0 <= d->T && d->rows <= d->T - d->row0, RV_ERR_SHAPE,
               "rv_mosaic(%s): rows [%ld, %ld + %ld) outside the T=%ld rows", op, d->row0, d->row0, d->rows, d->T);
  return RV_OK;
}

long knn_ws_bytes(long T, long k, long n_splits) { return n_splits > 1 ? n_splits * T * k * 8 : 0; }

// RV_MOSAIC_KNN / RV_MOSAIC_KNN_SMALL: checks, then the search and its merge on `st`
int run_knn(const rv_mosaic_desc* d, bool small, hipStream_t st) {
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

// RV_MOSAIC_LIVE's workspace: prev [n_streams] int32, the query rows [M, L] fp32, the search's partials; with a lag of
// D = d->lag > 0 frames then the lagged selection's state: (head, count) [n_streams, 2] int32 and the rings of
// R = D + 1 rows per stream, idx [n_streams, R, k] int32, dist [n_streams, R, k] fp32, trans [n_streams, R, k, k] fp32.
// With a grain fit (d->fit_radius > 0 or d->gain_max > 0) then the TARGET RINGS [n_streams, C] fp32, C = P + 2 D hop + block:
// input sample a of a stream (counted from its last reset) at ring[a mod C], silence before the reset; the block is
// written at the stream's frame count before the fit reads it, so the ring holds the block and the P + 2 D hop samples
// before it (a row that drains interleave with blocks can wait up to 2 D frames).  With a lag also the pending rows'
// arrival stamps [n_streams, R] int64 and the committed rows' target frames [M] int64.
// Every part starts on a 256-byte boundary.  M = n_streams * block / hop rows go to k_knn_small up to SMALL_T_MAX.
struct live_ws {
  long M, q, knn, knn_bytes, bytes;
  bool small;
  long lag, state, ridx, rdist, rtrans;
  bool fit;
  long C, ring, stamp, tfr;
};
int live_layout(const rv_mosaic_desc* d, const char* op, live_ws* w, bool run = false) {
  const rv_stream_desc* sd = d->live;
  RV_REQUIRE(sd, RV_ERR_NULL, "rv_mosaic(%s): null stream descriptor", op);
  RV_REQUIRE(sd->n_streams >= 1 && sd->hop >= 1 && sd->block >= sd->hop && sd->block % sd->hop == 0 && sd->S >= sd->hop &&
                 sd->n_streams <= 0x7fffffffL && sd->n_streams * (sd->block / sd->hop) <= 0x7fffffffL,
             RV_ERR_SHAPE, "rv_mosaic(%s): bad stream extents n_streams=%ld block=%ld hop=%ld S=%ld", op, sd->n_streams,
             sd->block, sd->hop, sd->S);
  RV_REQUIRE(d->L == sd->L, RV_ERR_SHAPE, "rv_mosaic(%s): corpus rows of L=%ld, the model's latent has %ld", op, d->L,
             sd->L);
  RV_REQUIRE(d->lag >= 0 && d->lag <= LAG_MAX, RV_ERR_SHAPE, "rv_mosaic(%s): lag=%ld outside [0, %d]", op, d->lag,
             LAG_MAX);
  RV_REQUIRE(d->lag == 0 || d->weight, RV_ERR_NULL, "rv_mosaic(%s): lag=%ld needs unit selection: weight is null", op,
             d->lag);
  const int frc = rv_grain_live_check(d, op, run);
  if (frc) return frc;
  w->M = sd->n_streams * (sd->block / sd->hop);
  w->small = w->M <= SMALL_T_MAX;
  rv_mosaic_desc kd = *d;
  kd.T = w->M;
  long per_split = 0, n_splits = 0;
  const int rc = knn_check(&kd, w->small, &per_split, &n_splits);
  if (rc) return rc;
  auto up = [](long n) { return (n + 255) & ~255L; };
  w->q = up(sd->n_streams * 4);
  w->knn = w->q + up(w->M * d->L * 4);
  w->knn_bytes = knn_ws_bytes(w->M, d->k, n_splits);
  w->bytes = w->knn + up(w->knn_bytes);
  w->lag = d->lag;
  if (w->lag > 0) {
    const long rows = sd->n_streams * (w->lag + 1);
    w->state = w->bytes;
    w->ridx = w->state + up(sd->n_streams * 8);
    w->rdist = w->ridx + up(rows * d->k * 4);
    w->rtrans = w->rdist + up(rows * d->k * 4);
    w->bytes = w->rtrans + up(rows * d->k * d->k * 4);
  }
  w->fit = d->fit_radius > 0 || d->gain_max > 0.f;
  if (w->fit) {
    w->C = rv_grain_live_ring(sd->S, sd->hop, sd->block, w->lag);
    w->ring = w->bytes;
    w->bytes = w->ring + up(sd->n_streams * w->C * 4);
    if (w->lag > 0) {
      w->stamp = w->bytes;
      w->tfr = w->stamp + up(sd->n_streams * (w->lag + 1) * 8);
      w->bytes = w->tfr + up(w->M * 8);
    }
  }
  return RV_OK;
}

}  // namespace

extern "C" int rv_mosaic(int op, rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d, RV_ERR_NULL, "rv_mosaic: null descriptor");
  const hipStream_t st = (hipStream_t)stream;
  long per_split = 0, n_splits = 0;
  switch (op) {
    case RV_MOSAIC_KNN_WORKSPACE:
    case RV_MOSAIC_KNN_SMALL_WORKSPACE: {
      const int rc = knn_check(d, op == RV_MOSAIC_KNN_SMALL_WORKSPACE, &per_split, &n_splits);
      if (rc) return rc;
      d->ws_bytes = knn_ws_bytes(d->T, d->k, n_splits);
      return RV_OK;
    }
    case RV_MOSAIC_KNN:
    case RV_MOSAIC_KNN_SMALL:
      return run_knn(d, op == RV_MOSAIC_KNN_SMALL, st);
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
    case RV_MOSAIC_TRANSITION: {
      const int rc = path_check(d, "TRANSITION", true);
      if (rc) return rc;
      RV_REQUIRE(d->c && d->idx && d->next_of && d->trans, RV_ERR_NULL, "rv_mosaic(TRANSITION): null pointer");
      RV_REQUIRE(d->N >= 1 && d->N < INT_MAX && d->L >= 1, RV_ERR_SHAPE, "rv_mosaic(TRANSITION): bad extents N=%ld L=%ld",
                 d->N, d->L);
      RV_REQUIRE((d->rows + trans_cfg<16>::RB - 1) / trans_cfg<16>::RB < (1L << 31), RV_ERR_SHAPE,
                 "rv_mosaic(TRANSITION): rows=%ld too many for one call", d->rows);
      const int vec = rows_vec16(d->c, d->L);
      if (d->k <= 1) launch_transition<1>(d, vec, st);
      else if (d->k <= 2) launch_transition<2>(d, vec, st);
      else if (d->k <= 4) launch_transition<4>(d, vec, st);
      else if (d->k <= 8) launch_transition<8>(d, vec, st);
      else launch_transition<16>(d, vec, st);
      RV_CHECK_LAUNCH();
      return RV_OK;
    }
    case RV_MOSAIC_PATH_WORKSPACE: {
      const int rc = path_check(d, "PATH_WORKSPACE", false);
      if (rc) return rc;
      d->ws_bytes = path_layout(d->T, d->k).bytes;
      return RV_OK;
    }
    case RV_MOSAIC_PATH_FORWARD: {
      const int rc = path_check(d, "PATH_FORWARD", true);
      if (rc) return rc;
      RV_REQUIRE(d->trans && d->idx && d->dist && d->ws, RV_ERR_NULL, "rv_mosaic(PATH_FORWARD): null pointer");
      RV_REQUIRE(d->lam >= 0.f && d->lam < INFINITY, RV_ERR_SHAPE,
                 "rv_mosaic(PATH_FORWARD): lambda=%g must be finite and not negative", (double)d->lam);
      const path_ws w = path_layout(d->T, d->k);
      RV_REQUIRE(d->ws_bytes >= w.bytes && ((unsigned long)d->ws & 15) == 0, RV_ERR_SHAPE,
                 "rv_mosaic(PATH_FORWARD): workspace of %ld bytes (16-byte aligned), %ld needed", d->ws_bytes, w.bytes);
      char* ws = (char*)d->ws;
      hipLaunchKernelGGL(k_path_forward, dim3(1), dim3(64), 0, st, d->trans, d->idx, d->dist, (int)d->k, d->row0,
                         d->rows, d->lam, (float*)ws, (float*)(ws + w.btr), (unsigned char*)(ws + w.back),
                         (unsigned char*)(ws + w.end));
      RV_CHECK_LAUNCH();
      return RV_OK;
    }
    case RV_MOSAIC_PATH_BACKTRACK: {
      const int rc = path_check(d, "PATH_BACKTRACK", false);
      if (rc) return rc;
      RV_REQUIRE(d->idx && d->dist && d->ws && d->slot && d->choice && d->cost, RV_ERR_NULL,
                 "rv_mosaic(PATH_BACKTRACK): null pointer");
      const path_ws w = path_layout(d->T, d->k);
      RV_REQUIRE(d->ws_bytes >= w.bytes && ((unsigned long)d->ws & 15) == 0, RV_ERR_SHAPE,
                 "rv_mosaic(PATH_BACKTRACK): workspace of %ld bytes (16-byte aligned), %ld needed", d->ws_bytes, w.bytes);
      char* ws = (char*)d->ws;
      hipLaunchKernelGGL(k_path_backtrack, dim3(1), dim3(64), 0, st, d->idx, d->dist, d->T, (int)d->k,
                         (const float*)(ws + w.btr), (const unsigned char*)(ws + w.back),
                         (const unsigned char*)(ws + w.end), d->slot, d->choice, d->cost);
      RV_CHECK_LAUNCH();
      return RV_OK;
    }
    case RV_MOSAIC_LIVE_WORKSPACE: {
      live_ws w;
      const int rc = live_layout(d, "LIVE_WORKSPACE", &w);
      if (rc) return rc;
      d->ws_bytes = w.bytes;
      return RV_OK;
    }
    case RV_MOSAIC_LIVE_RESET: {
      live_ws w;
      int rc = live_layout(d, "LIVE_RESET", &w);
      if (rc) return rc;
      const long NS = d->live->n_streams;
      RV_REQUIRE(d->ws && d->ws_bytes >= w.bytes, RV_ERR_SHAPE, "rv_mosaic(LIVE_RESET): workspace of %ld bytes, %ld needed",
                 d->ws_bytes, w.bytes);
      RV_REQUIRE(d->which >= -1 && d->which < NS, RV_ERR_SHAPE, "rv_mosaic(LIVE_RESET): stream %ld of %ld", d->which, NS);
      rc = rv_stream_reset(d->live, d->which, stream);
      if (rc) return rc;
      const long first = d->which < 0 ? 0 : d->which, n = d->which < 0 ? NS : 1;
      hipLaunchKernelGGL(k_live_clear, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int*)d->ws + first, n);
      if (w.lag > 0)   // nothing pending
        hipLaunchKernelGGL(k_live_lag_clear, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, st,
                           (int*)((char*)d->ws + w.state) + 2 * first, n);
      RV_CHECK_LAUNCH();
      if (w.fit) return rv_grain_live_reset((float*)((char*)d->ws + w.ring), w.C, first, n, stream);
      return RV_OK;
    }
    case RV_MOSAIC_LIVE:
    case RV_MOSAIC_LIVE_DRAIN: {
      const bool drain = op == RV_MOSAIC_LIVE_DRAIN;
      const char* who = drain ? "LIVE_DRAIN" : "LIVE";
      live_ws w;
      int rc = live_layout(d, who, &w, true);
      if (rc) return rc;
      const rv_stream_desc* sd = d->live;
      const bool decode = d->mode == RV_LIVE_DECODE;
      RV_REQUIRE(decode || d->mode == RV_LIVE_GRAINS, RV_ERR_UNSUPPORTED, "rv_mosaic(%s): mode %ld", who, d->mode);
      RV_REQUIRE(!drain || w.lag > 0, RV_ERR_SHAPE, "rv_mosaic(LIVE_DRAIN): lag=%ld: nothing is pending without a lag",
                 d->lag);
      RV_REQUIRE(d->c && d->idx && d->dist && d->ws && (decode || (d->src && d->row_start)) &&
                     (!d->weight || (d->next_of && d->choice)), RV_ERR_NULL,
                 "rv_mosaic(%s): null pointer (lag=%ld; unit selection needs weight, next_of and choice)", who,
                 d->lag);
      RV_REQUIRE(d->ws_bytes >= w.bytes && ((unsigned long)d->ws & 255) == 0, RV_ERR_SHAPE,
                 "rv_mosaic(%s): workspace of %ld bytes (256-byte aligned), %ld needed at lag=%ld", who, d->ws_bytes,
                 w.bytes, d->lag);
      RV_REQUIRE(d->N < INT_MAX && (decode || d->src_len >= sd->S), RV_ERR_SHAPE,
                 "rv_mosaic(%s): bad extents N=%ld src_len=%ld", who, d->N, d->src_len);
      char* ws = (char*)d->ws;
      float *qrows = (float*)(ws + w.q), *z = nullptr, *frames = nullptr;
      rc = rv_stream_encode(sd, drain ? nullptr : qrows, &z, &frames, stream);   // a drain encodes nothing
      if (rc) return rc;
      if (!drain) {
        rv_mosaic_desc kd = *d;
        kd.T = w.M;
        kd.q = qrows;
        kd.ws = ws + w.knn;
        kd.ws_bytes = w.knn_bytes;
        rc = run_knn(&kd, w.small, st);
        if (rc) return rc;
      }
      const int* sel = d->idx;
      int sel_k = (int)d->k;
      // with a fit the lagged selection stamps its rows: tfr [M] = the target frame each committed row stands for
      const long long* fcnt = w.fit ? rv_stream_counters(sd) : nullptr;
      long long *stamp = nullptr, *tfr = nullptr;
      if (w.fit && w.lag > 0) {
        stamp = (long long*)(ws + w.stamp);
        tfr = (long long*)(ws + w.tfr);
      }
      if (d->weight) {
        if (w.lag > 0) {
          const int vec = rows_vec16(d->c, d->L);
          hipLaunchKernelGGL(k_live_lag, dim3((unsigned)sd->n_streams), dim3(256), 0, st, d->c, d->N, d->L, d->next_of,
                             d->idx, d->dist, (int)d->k, sd->block / sd->hop, drain ? 0 : 1, (int)w.lag + 1, vec, d->weight,
                             (int*)ws, (int*)(ws + w.state), (int*)(ws + w.ridx), (float*)(ws + w.rdist),
                             (float*)(ws + w.rtrans), d->choice, fcnt, stamp, tfr);
        } else {
          hipLaunchKernelGGL(k_live_select, dim3((unsigned)sd->n_streams), dim3(64), 0, st, d->c, d->N, d->L, d->next_of,
                             d->idx, d->dist, (int)d->k, sd->block / sd->hop, d->weight, (int*)ws, d->choice);
        }
        sel = d->choice;
        sel_k = 1;
      }
      if (decode) {
        hipLaunchKernelGGL(k_gather_mean, dim3(blocks_for(w.M, 65536)), dim3(256), 0, st, d->c, d->N * d->L, nullptr,
                           d->L, d->N, d->L, sel, w.M, sel_k, z, d->L);
      } else if (w.fit) {   // each grain fitted to the target frame it stands for, then gathered
        rc = rv_grain_live(d, sel, sel_k, (float*)(ws + w.ring), fcnt, tfr, frames, stream);
        if (rc) return rc;
      } else {
        hipLaunchKernelGGL(k_gather_mean, dim3(blocks_for(w.M, 65536)), dim3(256), 0, st, d->src, d->src_len,
                           d->row_start, 0L, d->N, sd->S, sel, w.M, sel_k, frames, sd->S);
      }
      RV_CHECK_LAUNCH();
      return rv_stream_synth(sd, decode, stream);
    }
    case RV_GRAIN_FIT:
      return rv_grain_fit(d, stream);
    case RV_GRAIN_GATHER:
      return rv_grain_gather(d, stream);
    case RV_EVAL_FRAMES:
      return rv_eval_frames(d, stream);
    case RV_EVAL_DIMS:
      return rv_eval_dims(d, stream);
    case RV_PCA_MOMENTS:
      return rv_pca_moments(d, stream);
    case RV_PCA_EIG:
      return rv_pca_eig(d, stream);
    case RV_PCA_APPLY:
      return rv_pca_apply(d, stream);
    case RV_PCA_WORKSPACE:
      return rv_pca_workspace(d);
    case RV_PCA_LAGCOV:
      return rv_pca_lagcov(d, stream);
    case RV_WALK_FIT:
      return rv_walk_fit(d, stream);
    case RV_WALK_STEP:
      return rv_walk_step(d, stream);
    case RV_WALK_WORKSPACE:
      return rv_walk_workspace(d);
    case RV_ALIGN_COST: return rv_align_cost(d, stream);
    case RV_ALIGN_FORWARD: return rv_align_forward(d, stream);
    case RV_ALIGN_BACKTRACK: return rv_align_backtrack(d, stream);
    case RV_ALIGN_WARP: return rv_align_warp(d, stream);
    case RV_ALIGN_WORKSPACE: return rv_align_workspace(d);
    case RV_STRUCT_NOVELTY: return rv_struct_novelty(d, stream);
    case RV_STRUCT_PEAKS: return rv_struct_peaks(d, stream);
    case RV_STRUCT_WORKSPACE: return rv_struct_workspace(d);
    default:
      RV_REQUIRE(false, RV_ERR_UNSUPPORTED, "rv_mosaic: unknown op %d", op);
  }
  return RV_OK;
}
