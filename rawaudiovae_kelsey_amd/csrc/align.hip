// Time alignment of two latent trajectories (rawaudiovae_kelsey_amd/align.py): banded dynamic time warping over the
// encoder's mu rows.  Five ops of rv_mosaic; the rules: include/rawvae_hip.h, "Latent alignment"; the design and the
// measured figures: DESIGN.md section 7.12.
//   RV_ALIGN_COST       the local costs of the band, the search's distance bit for bit: k_align_cost, sqdist.h's
//                       register tile over (row block, column tile of the block's band); the finished tile
//                       goes through LDS and out in rows of 64 consecutive band slots.  No atomics, one launch.
//   RV_ALIGN_FORWARD    the DP in fp64: k_align_forward, ONE workgroup of 1024 threads over the anti-diagonals, three
//                       rolling diagonals of C in LDS (or in ws beyond FW_DIAG_LDS cells), a __syncthreads() between
//                       the diagonals, the next diagonal's local costs loaded before the barrier.
//   RV_ALIGN_BACKTRACK  k_align_backtrack: thread 0 walks the back table, then the workgroup reverses the walk into the
//                       path, and the path's own cost is added in ascending order.
//   RV_ALIGN_WARP       k_align_warp: the index tables of a synthesis on A's, B's or the path's timeline.
//   RV_ALIGN_WORKSPACE  the bytes of ws of FORWARD and BACKTRACK.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "internal.h"
#include "sqdist.h"

using namespace rv;
using namespace rv::sqd;

namespace {

constexpr int AL_LMAX = 4096;
constexpr int FW_THREADS = 1024;
constexpr int FW_DIAG_LDS = 2048;   // cells of the longest diagonal up to which the rolling diagonals live in LDS
constexpr int BT_THREADS = 1024;

// The band of include/rawvae_hip.h.  r = 0: the whole matrix.  num = Tb - 1, den = max(Ta - 1, 1).
struct band {
  long Ta, Tb, r, W, num, den;
};

// floor(x / y) for 0 <= x < 2^62, 0 < y < 2^31 and a quotient below 2^32: the fp64 quotient is within 1 of it (both
// roundings are relative 2^-53), one exact correction
__host__ __device__ __forceinline__ long div_floor(long x, long y) {
  long q = (long)((double)x / (double)y);
  const long rem = x - q * y;
  if (rem < 0) --q;
  else if (rem >= y) ++q;
  return q;
}

__host__ __device__ __forceinline__ long centre_of(const band& g, long i) { return div_floor(i * g.num, g.den); }

// band-local column of (i, j); the caller knows it is inside [0, W)
__device__ __forceinline__ long col_of(const band& g, long i, long j) { return g.r ? j - centre_of(g, i) + g.r : j; }

// One block per (row block of BR rows of a, tile of BN columns of the block's band).  The band columns of the block's
// rows are [centre(first) - r, centre(last) + r]; tile t starts at its first column + BN t.  Columns outside [0, Tb)
// stage zeros and their slots are written +inf; a tile wholly outside computes nothing.
__global__ void __launch_bounds__(256)
k_align_cost(const float* __restrict__ a, const float* __restrict__ b, long L, band g, long nt, float* __restrict__ dm) {
  __shared__ __attribute__((aligned(16))) float smem[SMEM_FLOATS];
  float(*Xs)[BR + PAD] = reinterpret_cast<float(*)[BR + PAD]>(smem);
  float(*Ws)[BN + PAD] = reinterpret_cast<float(*)[BN + PAD]>(smem + KT * (BR + PAD));
  float(*D)[BN + DPAD] = reinterpret_cast<float(*)[BN + DPAD]>(smem);
  const int tid = threadIdx.x, tn = tid & 15, tr = tid >> 4;
  const long rb = (long)blockIdx.x / nt, t = (long)blockIdx.x - rb * nt;
  const long r0 = rb * BR, rl = r0 + BR - 1 < g.Ta - 1 ? r0 + BR - 1 : g.Ta - 1;
  const long jfirst = g.r ? centre_of(g, r0) - g.r : 0, jlast = g.r ? centre_of(g, rl) + g.r : g.Tb - 1;
  const long m0 = jfirst + BN * t;
  if (m0 > jlast) return;   // the band of these rows has fewer tiles than the widest row block
  const bool inside = m0 + BN > 0 && m0 < g.Tb;
  float tot[TR][TN] = {};
  if (inside)
    tile_sq_dist(Xs, Ws, a, b, r0, m0, L, [&](long gr) { return gr < g.Ta; },
                 [&](long gm) { return gm >= 0 && gm < g.Tb; }, tot);
#pragma unroll
  for (int i = 0; i < TR; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) D[tr * TR + i][tn * TN + j] = tot[i][j];
  __syncthreads();
  // a wave writes the tile's 64 columns of one row: consecutive band slots, 256 bytes
  const int cc = tid & 63;
  const long j = m0 + cc;
  for (int row = tid >> 6; row < BR; row += 4) {
    const long i = r0 + row;
    if (i >= g.Ta) break;
    const long col = col_of(g, i, j);
    if (col >= 0 && col < g.W) dm[i * g.W + col] = (j >= 0 && j < g.Tb) ? D[row][cc] : INFINITY;
  }
}

// The rows i of anti-diagonal d = i + j that lie in the matrix and in the band, [lo, hi] (empty: hi < lo).
// i + centre(i) = floor(i (num + den) / den) rises by at least 1 per row, so the rows with |d - i - centre(i)| <= r
// are the run ceil((d - r) den / (num + den)) <= i <= ceil((d + r + 1) den / (num + den)) - 1.
__device__ __forceinline__ void diag_rows(const band& g, long d, long& lo, long& hi) {
  lo = d - (g.Tb - 1) > 0 ? d - (g.Tb - 1) : 0;
  hi = d < g.Ta - 1 ? d : g.Ta - 1;
  if (g.r) {
    const long s = g.num + g.den;
    if (d - g.r > 0) {
      const long blo = div_floor((d - g.r) * g.den + s - 1, s);
      lo = blo > lo ? blo : lo;
    }
    const long bhi = div_floor((d + g.r + 1) * g.den + s - 1, s) - 1;
    hi = bhi < hi ? bhi : hi;
  }
}

// the end of FORWARD, read by BACKTRACK: C at the end cell (+inf: not reached) and the end cell's column j
struct end_rec {
  double c;
  long j;
};

// ONE workgroup.  Diagonal d's accumulated costs live in buffer d % 3, indexed by the row i (modulo FW_DIAG_LDS in
// LDS: a diagonal has at most that many cells, and a neighbour is read only when its row lies in the run of its own
// diagonal, so no stale cell is ever read).  Thread t owns cells lo + t, lo + t + 1024, ... of a diagonal; the local
// cost of its first cell on the NEXT diagonal is loaded before the barrier.
template <bool IN_LDS>
__global__ void __launch_bounds__(FW_THREADS)
k_align_forward(const float* __restrict__ dm, band g, int subseq, double p, double* gdiag,
                unsigned char* __restrict__ back, double* lastrow, double* __restrict__ out, end_rec* __restrict__ endp) {
  __shared__ double sdiag[IN_LDS ? 3 * FW_DIAG_LDS : 1];
  __shared__ double redv[FW_THREADS / 64];
  __shared__ long redj[FW_THREADS / 64];
  const int tid = threadIdx.x;
  double* const base = IN_LDS ? sdiag : gdiag;
  const long pitch = IN_LDS ? FW_DIAG_LDS : g.Ta;
  auto ix = [&](long i) { return IN_LDS ? (i & (FW_DIAG_LDS - 1)) : i; };
  const long nd = g.Ta + g.Tb - 1;
  long lo2 = 0, hi2 = -1, lo1 = 0, hi1 = -1, lo, hi;
  diag_rows(g, 0, lo, hi);
  float cur = INFINITY;
  if (lo + tid <= hi) cur = dm[(lo + tid) * g.W + col_of(g, lo + tid, 0 - (lo + tid))];
  for (long d = 0; d < nd; ++d) {
    long nlo = 0, nhi = -1;
    float nxt = INFINITY;
    if (d + 1 < nd) {
      diag_rows(g, d + 1, nlo, nhi);
      const long i = nlo + tid;
      if (i <= nhi) nxt = dm[i * g.W + col_of(g, i, d + 1 - i)];
    }
    double* const b0 = base + (d % 3) * pitch;
    const double* const b1 = base + ((d + 2) % 3) * pitch;   // diagonal d - 1
    const double* const b2 = base + ((d + 1) % 3) * pitch;   // diagonal d - 2
    for (long i = lo + tid; i <= hi; i += FW_THREADS) {
      const long j = d - i;
      const long at = i * g.W + col_of(g, i, j);
      const float dv = i == lo + tid ? cur : dm[at];
      const double dd = (double)dv;
      const bool blocked = dv != dv || dv == INFINITY;
      const bool start = subseq ? i == 0 : d == 0;
      double best = INFINITY;
      int step = 3;
      if (i - 1 >= lo2 && i - 1 <= hi2) {
        const double c = b2[ix(i - 1)];
        if (c < best) { best = c; step = 0; }
      }
      if (i - 1 >= lo1 && i - 1 <= hi1) {
        const double c = b1[ix(i - 1)] + p;
        if (c < best) { best = c; step = 1; }
      }
      if (i >= lo1 && i <= hi1 && !(subseq && i == 0)) {
        const double c = b1[ix(i)] + p;
        if (c < best) { best = c; step = 2; }
      }
      double c;
      if (blocked) { c = INFINITY; step = 3; }
      else if (start) { c = dd; step = 3; }
      else c = step == 3 ? (double)INFINITY : dd + best;
      b0[ix(i)] = c;
      back[at] = (unsigned char)step;
      if (i == g.Ta - 1) {
        if (subseq) {
          lastrow[j] = c;
          if (out) out[j] = c;
        } else if (j == g.Tb - 1) {
          endp->c = c;
          endp->j = j;
        }
      }
    }
    __syncthreads();
    lo2 = lo1; hi2 = hi1; lo1 = lo; hi1 = hi; lo = nlo; hi = nhi;
    cur = nxt;
  }
  if (subseq) {
    // the lowest-j argmin of the finite C[Ta - 1, .]: +inf never wins, so j stays LONG_MAX when nothing is finite
    double bv = INFINITY;
    long bj = LONG_MAX;
    for (long j = tid; j < g.Tb; j += FW_THREADS) {
      const double v = lastrow[j];
      if (v < bv) { bv = v; bj = j; }
    }
    auto take = [&](double ov, long oj) {
      if (ov < bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
    };
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) take(__shfl_xor(bv, o, 64), __shfl_xor(bj, o, 64));
    if ((tid & 63) == 0) { redv[tid >> 6] = bv; redj[tid >> 6] = bj; }
    __syncthreads();
    if (tid == 0)
      for (int w = 1; w < FW_THREADS / 64; ++w) take(redv[w], redj[w]);
    if (tid == 0) {
      endp->c = bv;
      endp->j = bj == LONG_MAX ? 0 : bj;
    }
  }
}

// ONE workgroup.  Thread 0 walks the back table from the end cell: at most Ta + Tb - 1 cells whatever the table holds,
// and a move that would leave the matrix or the band ends the walk.  The cells go to rev in walking order; the
// workgroup then writes them reversed, fills the rest with -1 and adds the path's local costs in ascending order.
__global__ void __launch_bounds__(BT_THREADS)
k_align_backtrack(const float* __restrict__ dm, band g, const unsigned char* __restrict__ back,
                  const end_rec* __restrict__ endp, int* rev, int* __restrict__ path, int* __restrict__ choice,
                  double* __restrict__ cost) {
  __shared__ long sP;
  __shared__ double chunk[BT_THREADS];
  const int tid = threadIdx.x;
  const long cap = g.Ta + g.Tb - 1;
  const double cend = endp->c;
  const bool reached = cend < (double)INFINITY;
  if (tid == 0) {
    long n = 0;
    if (reached) {
      long i = g.Ta - 1, j = endp->j;
      if (j < 0 || j >= g.Tb) j = g.Tb - 1;
      while (n < cap) {
        const long col = col_of(g, i, j);
        if (col < 0 || col >= g.W) break;
        rev[2 * n] = (int)i;
        rev[2 * n + 1] = (int)j;
        ++n;
        const int step = back[i * g.W + col];
        if (step > 2) break;
        const long pi = step == 2 ? i : i - 1, pj = step == 1 ? j : j - 1;
        if (pi < 0 || pj < 0) break;
        i = pi;
        j = pj;
      }
    }
    sP = n;
  }
  __syncthreads();
  const long P = sP;
  for (long m = tid; m < cap; m += BT_THREADS) {
    path[2 * m] = m < P ? rev[2 * (P - 1 - m)] : -1;
    path[2 * m + 1] = m < P ? rev[2 * (P - 1 - m) + 1] : -1;
  }
  // sum of (double)Dm along the path in ascending order from +0: the workgroup fetches 1024 terms, thread 0 adds them
  double acc = 0.0;
  for (long m0 = 0; m0 < P; m0 += BT_THREADS) {
    const long m = m0 + tid;
    if (m < P) {
      const long i = rev[2 * (P - 1 - m)], j = rev[2 * (P - 1 - m) + 1];
      chunk[tid] = (double)dm[i * g.W + col_of(g, i, j)];
    }
    __syncthreads();
    if (tid == 0) {
      const long n = P - m0 < BT_THREADS ? P - m0 : BT_THREADS;
      for (long x = 0; x < n; ++x) acc += chunk[x];
    }
    __syncthreads();
  }
  if (tid == 0) {
    choice[0] = (int)P;
    choice[1] = P ? rev[2 * (P - 1) + 1] : -1;
    choice[2] = P ? rev[1] : -1;
    choice[3] = reached ? 1 : 0;
    cost[0] = reached ? cend : (double)INFINITY;
    cost[1] = acc;
  }
}

// idx [n, 2] = (ia, ib).  ON_PATH: the path.  ON_A / ON_B: row x of the timeline takes the LOWEST path entry whose
// own coordinate is x (the path is ascending in both coordinates: a binary search), (-1, -1) when there is none.
__global__ void __launch_bounds__(256)
k_align_warp(const int* __restrict__ path, const int* __restrict__ choice, long cap, long n, int timeline,
             int* __restrict__ idx) {
  const long x = (long)blockIdx.x * 256 + threadIdx.x;
  if (x >= n) return;
  long P = choice[0];
  P = P < 0 ? 0 : (P > cap ? cap : P);
  int ia = -1, ib = -1;
  if (timeline == RV_ALIGN_ON_PATH) {
    if (x < P) { ia = path[2 * x]; ib = path[2 * x + 1]; }
  } else {
    const int own = timeline == RV_ALIGN_ON_A ? 0 : 1;
    long lo = 0, hi = P;   // the first entry whose own coordinate is >= x
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (path[2 * mid + own] < x) lo = mid + 1;
      else hi = mid;
    }
    if (lo < P && path[2 * lo + own] == x) { ia = path[2 * lo]; ib = path[2 * lo + 1]; }
  }
  idx[2 * x] = ia;
  idx[2 * x + 1] = ib;
}

struct align_ws {
  long maxdiag, diag, lastrow, rev, end, bytes;
};

// the shared checks of (T, N, band) and the band they make
int align_band(const rv_mosaic_desc* d, const char* op, band* g) {
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): T=%ld outside [1, 2^31)", op, d->T);
  RV_REQUIRE(d->N >= 1 && d->N < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): N=%ld outside [1, 2^31)", op, d->N);
  RV_REQUIRE(d->band >= 0 && d->band < (1L << 30), RV_ERR_SHAPE, "rv_mosaic(%s): band=%ld outside [0, 2^30)", op,
             d->band);
  g->Ta = d->T;
  g->Tb = d->N;
  g->r = d->band;
  g->W = g->r ? 2 * g->r + 1 : g->Tb;
  g->num = g->Tb - 1;
  g->den = g->Ta > 1 ? g->Ta - 1 : 1;
  if (g->r) {
    // a path exists iff no row's band starts beyond the end of the row before it
    const long slope = g->Ta > 1 ? (g->num + g->den - 1) / g->den : 0;
    const long least = g->Ta > 1 ? (slope > 3 ? slope / 2 : 1) : g->num;
    RV_REQUIRE(g->Ta > 1 ? slope <= g->W : g->num <= g->r, RV_ERR_SHAPE,
               "rv_mosaic(%s): band=%ld: the band admits no path through T=%ld by N=%ld; the least band that does is %ld "
               "(0: the whole matrix)", op, d->band, d->T, d->N, least);
  }
  RV_REQUIRE(g->Ta * g->W < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): T=%ld rows of %ld band slots (band=%ld) reach 2^31",
             op, d->T, g->W, d->band);
  return RV_OK;
}

align_ws align_layout(const band& g) {
  align_ws w;
  w.maxdiag = g.Ta < g.Tb ? g.Ta : g.Tb;
  if (g.r && g.W < w.maxdiag) w.maxdiag = g.W;
  w.diag = up256(g.Ta * g.W);
  w.lastrow = w.diag + (w.maxdiag > FW_DIAG_LDS ? up256(3 * g.Ta * 8) : 0);
  w.rev = w.lastrow + up256(g.Tb * 8);
  w.end = w.rev + up256((g.Ta + g.Tb - 1) * 8);
  w.bytes = w.end + 256;
  return w;
}

int align_ws_check(const rv_mosaic_desc* d, const char* op, const align_ws& w) {
  RV_REQUIRE(d->ws_bytes >= w.bytes, RV_ERR_SHAPE, "rv_mosaic(%s): ws_bytes=%ld, T=%ld by N=%ld at band=%ld need %ld", op,
             d->ws_bytes, d->T, d->N, d->band, w.bytes);
  RV_REQUIRE(d->ws, RV_ERR_NULL, "rv_mosaic(%s): ws is null, T=%ld by N=%ld at band=%ld need %ld bytes", op, d->T, d->N,
             d->band, w.bytes);
  RV_REQUIRE(((unsigned long)d->ws & 255) == 0, RV_ERR_SHAPE, "rv_mosaic(%s): ws is not 256-byte aligned", op);
  return RV_OK;
}

}  // namespace

int rv_align_workspace(rv_mosaic_desc* d) {
  band g;
  const int rc = align_band(d, "ALIGN_WORKSPACE", &g);
  if (rc) return rc;
  d->ws_bytes = align_layout(g).bytes;
  return RV_OK;
}

int rv_align_cost(const rv_mosaic_desc* d, void* stream) {
  band g;
  const int rc = align_band(d, "ALIGN_COST", &g);
  if (rc) return rc;
  RV_REQUIRE(d->L >= 1 && d->L <= AL_LMAX, RV_ERR_SHAPE, "rv_mosaic(ALIGN_COST): L=%ld outside [1, %d]", d->L, AL_LMAX);
  RV_REQUIRE(d->a, RV_ERR_NULL, "rv_mosaic(ALIGN_COST): a is null");
  RV_REQUIRE(d->b, RV_ERR_NULL, "rv_mosaic(ALIGN_COST): b is null");
  RV_REQUIRE(d->local_costs, RV_ERR_NULL, "rv_mosaic(ALIGN_COST): local_costs is null");
  // column tiles of the widest row block: BR - 1 rows move the centre by at most floor((BR - 1) num / den) + 1
  const long span = g.r ? (BR - 1) * g.num / g.den + 1 + g.W : g.Tb;
  const long nt = (span + BN - 1) / BN, nrb = (g.Ta + BR - 1) / BR;
  RV_REQUIRE(nrb * nt < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(ALIGN_COST): T=%ld by N=%ld at band=%ld make %ld tiles, 2^31 or more",
             d->T, d->N, d->band, nrb * nt);
  hipLaunchKernelGGL(k_align_cost, dim3((unsigned)(nrb * nt)), dim3(256), 0, (hipStream_t)stream, d->a, d->b, d->L, g, nt,
                     d->local_costs);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_align_forward(const rv_mosaic_desc* d, void* stream) {
  band g;
  const int rc = align_band(d, "ALIGN_FORWARD", &g);
  if (rc) return rc;
  RV_REQUIRE(d->mode == RV_ALIGN_GLOBAL || d->mode == RV_ALIGN_SUBSEQUENCE, RV_ERR_SHAPE,
             "rv_mosaic(ALIGN_FORWARD): mode=%ld is neither RV_ALIGN_GLOBAL nor RV_ALIGN_SUBSEQUENCE", d->mode);
  RV_REQUIRE(d->mode == RV_ALIGN_GLOBAL || d->band == 0, RV_ERR_SHAPE,
             "rv_mosaic(ALIGN_FORWARD): band=%ld: RV_ALIGN_SUBSEQUENCE (mode) runs on the whole matrix, band 0", d->band);
  RV_REQUIRE(d->penalty >= 0.f && d->penalty < INFINITY, RV_ERR_SHAPE,
             "rv_mosaic(ALIGN_FORWARD): penalty=%g must be finite and not negative", (double)d->penalty);
  RV_REQUIRE(d->local_costs, RV_ERR_NULL, "rv_mosaic(ALIGN_FORWARD): local_costs is null");
  const align_ws w = align_layout(g);
  const int wrc = align_ws_check(d, "ALIGN_FORWARD", w);
  if (wrc) return wrc;
  char* const ws = (char*)d->ws;
  const int subseq = d->mode == RV_ALIGN_SUBSEQUENCE;
  if (w.maxdiag <= FW_DIAG_LDS)
    hipLaunchKernelGGL(k_align_forward<true>, dim3(1), dim3(FW_THREADS), 0, (hipStream_t)stream, d->local_costs, g, subseq,
                       (double)d->penalty, (double*)nullptr, (unsigned char*)ws, (double*)(ws + w.lastrow), d->end_costs,
                       (end_rec*)(ws + w.end));
  else
    hipLaunchKernelGGL(k_align_forward<false>, dim3(1), dim3(FW_THREADS), 0, (hipStream_t)stream, d->local_costs, g, subseq,
                       (double)d->penalty, (double*)(ws + w.diag), (unsigned char*)ws, (double*)(ws + w.lastrow), d->end_costs,
                       (end_rec*)(ws + w.end));
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_align_backtrack(const rv_mosaic_desc* d, void* stream) {
  band g;
  const int rc = align_band(d, "ALIGN_BACKTRACK", &g);
  if (rc) return rc;
  RV_REQUIRE(d->local_costs, RV_ERR_NULL, "rv_mosaic(ALIGN_BACKTRACK): local_costs is null");
  RV_REQUIRE(d->path, RV_ERR_NULL, "rv_mosaic(ALIGN_BACKTRACK): the path is null");
  RV_REQUIRE(d->summary, RV_ERR_NULL, "rv_mosaic(ALIGN_BACKTRACK): the summary is null");
  RV_REQUIRE(d->path_costs, RV_ERR_NULL, "rv_mosaic(ALIGN_BACKTRACK): path_costs is null");
  const align_ws w = align_layout(g);
  const int wrc = align_ws_check(d, "ALIGN_BACKTRACK", w);
  if (wrc) return wrc;
  char* const ws = (char*)d->ws;
  hipLaunchKernelGGL(k_align_backtrack, dim3(1), dim3(BT_THREADS), 0, (hipStream_t)stream, d->local_costs, g,
                     (const unsigned char*)ws, (const end_rec*)(ws + w.end), (int*)(ws + w.rev), d->path, d->summary,
                     d->path_costs);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_align_warp(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(ALIGN_WARP): T=%ld outside [1, 2^31)", d->T);
  RV_REQUIRE(d->N >= 1 && d->N < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(ALIGN_WARP): N=%ld outside [1, 2^31)", d->N);
  RV_REQUIRE(d->mode == RV_ALIGN_ON_A || d->mode == RV_ALIGN_ON_B || d->mode == RV_ALIGN_ON_PATH, RV_ERR_SHAPE,
             "rv_mosaic(ALIGN_WARP): mode=%ld is none of RV_ALIGN_ON_A, RV_ALIGN_ON_B, RV_ALIGN_ON_PATH", d->mode);
  RV_REQUIRE(d->path, RV_ERR_NULL, "rv_mosaic(ALIGN_WARP): the path is null");
  RV_REQUIRE(d->summary, RV_ERR_NULL, "rv_mosaic(ALIGN_WARP): the summary is null");
  RV_REQUIRE(d->warp_table, RV_ERR_NULL, "rv_mosaic(ALIGN_WARP): warp_table is null");
  const long cap = d->T + d->N - 1;
  const long n = d->mode == RV_ALIGN_ON_A ? d->T : d->mode == RV_ALIGN_ON_B ? d->N : cap;
  hipLaunchKernelGGL(k_align_warp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d->path,
                     d->summary, cap, n, (int)d->mode, d->warp_table);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
