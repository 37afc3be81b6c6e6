// Live mosaicing (rawaudiovae_kelsey_amd/mosaic.py, StreamingMosaic): one block of live audio matched against a corpus
// on the device.  Four ops of rv_mosaic (mosaic.hip):
//   RV_MOSAIC_LIVE            the stream's encoder (stream.hip), the search (mosaic_knn.hip), unit selection
//                             (k_live_select: greedy; k_live_lag: viterbi.h's rule over a window of lag + 1 frames,
//                             committing the oldest), gather-mean (mosaic.hip) or the fitted grains (grain.hip), then
//                             the stream's decoder / overlap-add
//   RV_MOSAIC_LIVE_DRAIN      one block that plays out the frames a lag still holds back: no encoder, no search
//   RV_MOSAIC_LIVE_RESET      a stream, or all, back to "nothing chosen, nothing pending"
//   RV_MOSAIC_LIVE_WORKSPACE  the bytes of ws of the three
// The measured figures: DESIGN.md sections 7.6 and 7.7.
#include <limits.h>

#include "common.h"
#include "internal.h"
#include "sqdist.h"
#include "viterbi.h"

using namespace rv;
using namespace rv::sqd;
using namespace rv::vit;

namespace {

// ---- Live mosaicing: greedy unit selection ----
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
  const int rc = rv_knn_workspace(&kd, w->small);
  if (rc) return rc;
  w->q = up256(sd->n_streams * 4);
  w->knn = w->q + up256(w->M * d->L * 4);
  w->knn_bytes = kd.ws_bytes;
  w->bytes = w->knn + up256(w->knn_bytes);
  w->lag = d->lag;
  if (w->lag > 0) {
    const long rows = sd->n_streams * (w->lag + 1);
    w->state = w->bytes;
    w->ridx = w->state + up256(sd->n_streams * 8);
    w->rdist = w->ridx + up256(rows * d->k * 4);
    w->rtrans = w->rdist + up256(rows * d->k * 4);
    w->bytes = w->rtrans + up256(rows * d->k * d->k * 4);
  }
  w->fit = d->fit_radius > 0 || d->gain_max > 0.f;
  if (w->fit) {
    w->C = rv_grain_live_ring(sd->S, sd->hop, sd->block, w->lag);
    w->ring = w->bytes;
    w->bytes = w->ring + up256(sd->n_streams * w->C * 4);
    if (w->lag > 0) {
      w->stamp = w->bytes;
      w->tfr = w->stamp + up256(sd->n_streams * (w->lag + 1) * 8);
      w->bytes = w->tfr + up256(w->M * 8);
    }
  }
  return RV_OK;
}

}  // namespace

int rv_live_workspace(rv_mosaic_desc* d) {
  live_ws w;
  const int rc = live_layout(d, "LIVE_WORKSPACE", &w);
  if (rc) return rc;
  d->ws_bytes = w.bytes;
  return RV_OK;
}

int rv_live_reset(const rv_mosaic_desc* d, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
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

int rv_live_block(const rv_mosaic_desc* d, int drain, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
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
    rc = rv_knn_search(&kd, w.small, stream);
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
    RV_CHECK_LAUNCH();
    sel = d->choice;
    sel_k = 1;
  }
  if (decode)   // the chosen latent rows, then the decoder
    rc = rv_gather_mean_launch(d->c, d->N * d->L, nullptr, d->L, d->N, d->L, sel, w.M, sel_k, z, d->L, stream);
  else if (w.fit)   // each grain fitted to the target frame it stands for, then gathered
    rc = rv_grain_live(d, sel, sel_k, (float*)(ws + w.ring), fcnt, tfr, frames, stream);
  else
    rc = rv_gather_mean_launch(d->src, d->src_len, d->row_start, 0L, d->N, sd->S, sel, w.M, sel_k, frames, sd->S, stream);
  if (rc) return rc;
  return rv_stream_synth(sd, decode, stream);
}
