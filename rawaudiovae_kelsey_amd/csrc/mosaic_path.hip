// Continuity-aware mosaicing (rawaudiovae_kelsey_amd/mosaic.py): offline Viterbi unit selection over the k candidates
// of every row ("Continuity").  Four ops of rv_mosaic (mosaic.hip):
//   RV_MOSAIC_TRANSITION      candidate-to-candidate concatenation costs [rows, k, k] in the search's arithmetic
//   RV_MOSAIC_PATH_FORWARD    the forward pass of a chunk of rows, one wave, on viterbi.h's rule
//   RV_MOSAIC_PATH_BACKTRACK  slot, choice and the two cost sums, one wave
//   RV_MOSAIC_PATH_WORKSPACE  the bytes of ws of the two passes
#include <limits.h>

#include "common.h"
#include "internal.h"
#include "sqdist.h"
#include "viterbi.h"

using namespace rv;
using namespace rv::sqd;
using namespace rv::vit;

namespace {

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

constexpr int PATH_PF = 16;      // rows of trans, dist and idx held in registers ahead of the dependent chain
constexpr int BT_CH = 256;       // rows per staged chunk of the backtrack

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

}  // namespace

int rv_path_transition(const rv_mosaic_desc* d, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
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

int rv_path_workspace(rv_mosaic_desc* d) {
  const int rc = path_check(d, "PATH_WORKSPACE", false);
  if (rc) return rc;
  d->ws_bytes = path_layout(d->T, d->k).bytes;
  return RV_OK;
}

int rv_path_forward(const rv_mosaic_desc* d, void* stream) {
  const int rc = path_check(d, "PATH_FORWARD", true);
  if (rc) return rc;
  RV_REQUIRE(d->trans && d->idx && d->dist && d->ws, RV_ERR_NULL, "rv_mosaic(PATH_FORWARD): null pointer");
  RV_REQUIRE(d->lam >= 0.f && d->lam < INFINITY, RV_ERR_SHAPE,
             "rv_mosaic(PATH_FORWARD): lambda=%g must be finite and not negative", (double)d->lam);
  const path_ws w = path_layout(d->T, d->k);
  RV_REQUIRE(d->ws_bytes >= w.bytes && ((unsigned long)d->ws & 15) == 0, RV_ERR_SHAPE,
             "rv_mosaic(PATH_FORWARD): workspace of %ld bytes (16-byte aligned), %ld needed", d->ws_bytes, w.bytes);
  char* ws = (char*)d->ws;
  hipLaunchKernelGGL(k_path_forward, dim3(1), dim3(64), 0, (hipStream_t)stream, d->trans, d->idx, d->dist, (int)d->k,
                     d->row0, d->rows, d->lam, (float*)ws, (float*)(ws + w.btr), (unsigned char*)(ws + w.back),
                     (unsigned char*)(ws + w.end));
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_path_backtrack(const rv_mosaic_desc* d, void* stream) {
  const int rc = path_check(d, "PATH_BACKTRACK", false);
  if (rc) return rc;
  RV_REQUIRE(d->idx && d->dist && d->ws && d->slot && d->choice && d->cost, RV_ERR_NULL,
             "rv_mosaic(PATH_BACKTRACK): null pointer");
  const path_ws w = path_layout(d->T, d->k);
  RV_REQUIRE(d->ws_bytes >= w.bytes && ((unsigned long)d->ws & 15) == 0, RV_ERR_SHAPE,
             "rv_mosaic(PATH_BACKTRACK): workspace of %ld bytes (16-byte aligned), %ld needed", d->ws_bytes, w.bytes);
  char* ws = (char*)d->ws;
  hipLaunchKernelGGL(k_path_backtrack, dim3(1), dim3(64), 0, (hipStream_t)stream, d->idx, d->dist, d->T, (int)d->k,
                     (const float*)(ws + w.btr), (const unsigned char*)(ws + w.back),
                     (const unsigned char*)(ws + w.end), d->slot, d->choice, d->cost);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
