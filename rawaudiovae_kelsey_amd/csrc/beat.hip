// The pulse of a latent trajectory (rawaudiovae_kelsey_amd/beats.py): onset strength, tempo and beats.  Four ops of
// rv_mosaic; the rules: include/rawvae_hip.h, "Latent beats"; the design and the measured figures: DESIGN.md section 7.20.
//   RV_BEAT_ONSET      the novelty curve rectified and divided by its RMS: the squares in RV_EVAL_DIMS's order
//                      (k_onset_part, k_onset_total), then one division per frame (k_onset_scale).
//   RV_BEAT_TEMPOGRAM  the windowed autocorrelation A [nW, lags]: k_tempo_acf, a workgroup per (window, 256 lags), a thread
//                      per lag; the window's stretch of o and win go through LDS once and every thread walks them in tiles
//                      of 64 (o[a] and win[i] are broadcasts, o[a + tau] consecutive doubles: no bank conflict).  Then the
//                      period every window prefers (k_tempo_period, a workgroup per window) and the sum over the windows
//                      with the period it prefers (k_tempo_total, ONE workgroup, a thread per lag).
//   RV_BEAT_TRACK      the dynamic programme and its backtrack in ONE workgroup (k_beat_track): a block of dlo frames
//                      depends on earlier blocks only, so its frames run side by side, each frame's window spread over
//                      the lanes that are left; the last values of C in an LDS ring.
//   RV_BEAT_WORKSPACE  the bytes of ws of ONSET.
#include <math.h>

#include "common.h"
#include "internal.h"

// every product below is rounded before it is added (the header's rule; numpy reproduces it bit for bit)
#pragma clang fp contract(off)

using namespace rv;

namespace {

constexpr int ON_ROWS = 256;       // frames of one block of the sum of squares: RV_EVAL_DIMS's (the header states it)
constexpr int TG_WMAX = 8192;      // the longest window
constexpr int TG_LAGMAX = 1024;    // the largest lag
constexpr int TG_THREADS = 256;    // lags of one workgroup of k_tempo_acf
constexpr int TG_TILE = 64;        // values of i in one chain
constexpr int TG_LDS_MAX = (2 * TG_WMAX + TG_LAGMAX) * 8;
constexpr int TR_DMAX = 2048;      // the furthest predecessor, and the longest end window
constexpr int TR_THREADS = 1024;
constexpr int TR_RING = 4096;      // >= dhi + dlo: a frame of the running block never lands on a slot that block reads

__device__ __forceinline__ bool finite64(double v) { return fabs(v) < (double)INFINITY; }

// Block b = frames [256 b, 256 b + 256): the sum of h h in ascending t from +0, the entries > 0 and the finite ones.
__global__ void __launch_bounds__(ON_ROWS)
k_onset_part(const double* __restrict__ nov, long T, double* __restrict__ bsum, int* __restrict__ bpos,
             int* __restrict__ bfin) {
  __shared__ double vals[ON_ROWS];
  const int tid = threadIdx.x;
  const long t = (long)blockIdx.x * ON_ROWS + tid;
  vals[tid] = t < T ? nov[t] : (double)NAN;
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    int pos = 0, fin = 0;
    for (int x = 0; x < ON_ROWS; ++x) {
      const double v = vals[x];
      if (!finite64(v)) continue;
      ++fin;
      if (v > 0.0) { acc += v * v; ++pos; }
    }
    bsum[blockIdx.x] = acc;
    bpos[blockIdx.x] = pos;
    bfin[blockIdx.x] = fin;
  }
}

// ONE workgroup: the block sums in ascending order from +0 (fetched 256 at a time, thread 0 adds them), s = sqrt(q / T).
__global__ void __launch_bounds__(ON_ROWS)
k_onset_total(const double* __restrict__ bsum, const int* __restrict__ bpos, const int* __restrict__ bfin, long nb, long T,
              double* __restrict__ tot, int* __restrict__ summary, double* __restrict__ cost) {
  __shared__ double vals[ON_ROWS];
  __shared__ int poss[ON_ROWS], fins[ON_ROWS];
  const int tid = threadIdx.x;
  double acc = 0.0;
  long pos = 0, fin = 0;
  for (long b0 = 0; b0 < nb; b0 += ON_ROWS) {
    const long b = b0 + tid;
    vals[tid] = b < nb ? bsum[b] : 0.0;
    poss[tid] = b < nb ? bpos[b] : 0;
    fins[tid] = b < nb ? bfin[b] : 0;
    __syncthreads();
    if (tid == 0) {
      const int m = nb - b0 < ON_ROWS ? (int)(nb - b0) : ON_ROWS;
      for (int x = 0; x < m; ++x) { acc += vals[x]; pos += poss[x]; fin += fins[x]; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double s = sqrt(acc / (double)T);
    *tot = s;
    summary[0] = (int)pos;
    summary[1] = (int)fin;
    summary[2] = 0;
    summary[3] = 0;
    cost[0] = s;
    cost[1] = 0.0;
  }
}

__global__ void __launch_bounds__(ON_ROWS)
k_onset_scale(const double* __restrict__ nov, long T, const double* __restrict__ tot, double* __restrict__ o) {
  const long t = (long)blockIdx.x * ON_ROWS + threadIdx.x;
  if (t >= T) return;
  const double v = nov[t], s = *tot;
  const double h = finite64(v) && v > 0.0 ? v : 0.0;
  o[t] = s > 0.0 ? h / s : 0.0;
}

// The larger of two candidates (value, lag): a larger value wins, equal values go to the smaller lag; lag 0 is "none".
__device__ __forceinline__ void best_of(double& v, int& tau, double v2, int tau2) {
  if (tau2 && (!tau || v2 > v || (v2 == v && tau2 < tau))) { v = v2; tau = tau2; }
}

// Workgroup (n, y): window n, the lags lo + 256 y + tid.  LDS: seg [Wn + hi] = o[n Hw ..] (0 beyond T: never used, a term
// whose second factor lies beyond T is skipped by index), then win [Wn].
__global__ void __launch_bounds__(TG_THREADS)
k_tempo_acf(const double* __restrict__ o, long T, int Wn, long Hw, int lo, int hi, const double* __restrict__ win,
            double* __restrict__ A, long ldo) {
  extern __shared__ __attribute__((aligned(16))) double tg_lds[];
  double* const seg = tg_lds;
  double* const wv = tg_lds + Wn + hi;
  const int tid = threadIdx.x;
  const long n = blockIdx.x, a0 = n * Hw;
  for (int x = tid; x < Wn + hi; x += TG_THREADS) seg[x] = a0 + x < T ? o[a0 + x] : 0.0;
  for (int x = tid; x < Wn; x += TG_THREADS) wv[x] = win[x];
  __syncthreads();
  const int tau = lo + (int)blockIdx.y * TG_THREADS + tid;
  if (tau > hi) return;
  // i < Wn and a0 + i + tau < T
  const long room = T - a0 - tau;
  const int iend = room < Wn ? (room > 0 ? (int)room : 0) : Wn;
  double acc = 0.0;
  for (int i0 = 0; i0 < iend; i0 += TG_TILE) {
    const int i1 = i0 + TG_TILE < iend ? i0 + TG_TILE : iend;
    double tile = 0.0;
    for (int i = i0; i < i1; ++i) {
      const double p = seg[i] * seg[i + tau];
      tile += wv[i] * p;
    }
    acc += tile;
  }
  A[n * ldo + (tau - lo)] = acc;
}

// The best of the THREADS candidates in cand_v / cand_t (one per thread) into slot 0, by best_of: the tie rule is in the
// comparison, so the tree's shape cannot change the winner.
template <int THREADS>
__device__ __forceinline__ void best_reduce(double* cand_v, int* cand_t, int tid) {
  __syncthreads();
  for (int s = THREADS / 2; s >= 1; s >>= 1) {
    if (tid < s) {
      double v = cand_v[tid];
      int t = cand_t[tid];
      best_of(v, t, cand_v[tid + s], cand_t[tid + s]);
      cand_v[tid] = v;
      cand_t[tid] = t;
    }
    __syncthreads();
  }
}

// Workgroup n (grid-stride): period[n] = the lag of the largest finite fl(prior A[n, .]) > 0, ties to the smaller lag.
__global__ void __launch_bounds__(TG_THREADS)
k_tempo_period(const double* __restrict__ A, long ldo, long nW, int lo, int hi, const double* __restrict__ prior,
               int* __restrict__ period) {
  __shared__ double cand_v[TG_THREADS];
  __shared__ int cand_t[TG_THREADS];
  const int tid = threadIdx.x;
  for (long n = blockIdx.x; n < nW; n += gridDim.x) {
    double bv = 0.0;
    int bt = 0;
    for (int tau = lo + tid; tau <= hi; tau += TG_THREADS) {   // ascending: an equal later lag does not replace
      const double sc = prior[tau - lo] * A[n * ldo + (tau - lo)];
      if (finite64(sc) && sc > 0.0) best_of(bv, bt, sc, tau);
    }
    cand_v[tid] = bv;
    cand_t[tid] = bt;
    best_reduce<TG_THREADS>(cand_v, cand_t, tid);
    if (tid == 0) period[n] = cand_t[0];
    __syncthreads();
  }
}

// ONE workgroup, thread x = lag lo + x: G in ascending n from +0, its score, then P.
__global__ void __launch_bounds__(TG_LAGMAX)
k_tempo_total(const double* __restrict__ A, long ldo, long nW, int lo, int hi, const double* __restrict__ prior,
              double* __restrict__ G, int* __restrict__ info, double* __restrict__ cost) {
  __shared__ double cand_v[TG_LAGMAX], gs[TG_LAGMAX];
  __shared__ int cand_t[TG_LAGMAX];
  const int tid = threadIdx.x, tau = lo + tid;
  double g = 0.0, bv = 0.0;
  int bt = 0;
  if (tau <= hi) {
    for (long n = 0; n < nW; ++n) g += A[n * ldo + tid];
    G[tid] = g;
    const double sc = prior[tid] * g;
    if (finite64(sc) && sc > 0.0) { bv = sc; bt = tau; }
  }
  gs[tid] = g;
  cand_v[tid] = bv;
  cand_t[tid] = bt;
  best_reduce<TG_LAGMAX>(cand_v, cand_t, tid);
  if (tid == 0) {
    const int P = cand_t[0];
    info[0] = P;
    info[1] = (int)nW;
    info[2] = 0;
    info[3] = 0;
    cost[0] = P ? cand_v[0] : 0.0;
    cost[1] = P ? gs[P - lo] : 0.0;
  }
}

// ONE workgroup.  LPF = lanes per frame (a power of two, at most 64), FP = 1024 / LPF frames side by side; a block of
// dlo frames takes ceil(dlo / FP) passes.  ring[t & 4095] = C[t] for the last 4096 frames.
__global__ void __launch_bounds__(TR_THREADS)
k_beat_track(const double* __restrict__ o, long T, int dlo, int dhi, int P, const double* __restrict__ pen, int LPF,
             double* __restrict__ C, int* __restrict__ back, int* __restrict__ path, long n_out, int* __restrict__ summary,
             double* __restrict__ cost) {
  __shared__ double ring[TR_RING];
  __shared__ double pn[TR_DMAX];
  __shared__ double cand_v[TR_THREADS];
  __shared__ int cand_t[TR_THREADS];
  __shared__ long sh_n;
  const int tid = threadIdx.x, nd = dhi - dlo + 1;
  const int FP = TR_THREADS / LPF, g = tid / LPF, l = tid - g * LPF;
  for (int x = tid; x < nd; x += TR_THREADS) pn[x] = pen[x];
  __syncthreads();
  for (long b0 = 0; b0 < T; b0 += dlo) {
    const long bend = b0 + dlo < T ? b0 + dlo : T;
    for (long f0 = b0; f0 < bend; f0 += FP) {
      const long t = f0 + g;
      const bool ok = t < bend;
      double bv = -(double)INFINITY;
      int bd = 0;   // delta of the best candidate, 0: none
      if (ok) {
        const long far = t < dhi ? t : dhi;   // p >= 0
        for (int dl = dlo + l; dl <= far; dl += LPF) {   // ascending delta: an equal later (further) one does not replace
          const double v = ring[(t - dl) & (TR_RING - 1)] + pn[dl - dlo];
          if (v > bv) { bv = v; bd = dl; }
        }
      }
      for (int m = 1; m < LPF; m <<= 1) {
        const double v2 = __shfl_xor(bv, m);
        const int d2 = __shfl_xor(bd, m);
        if (d2 && (!bd || v2 > bv || (v2 == bv && d2 < bd))) { bv = v2; bd = d2; }
      }
      if (ok && l == 0) {
        const double x = o[t], h = finite64(x) ? x : 0.0;
        const double c = bd ? h + bv : h;
        ring[t & (TR_RING - 1)] = c;
        C[t] = c;
        back[t] = bd ? (int)(t - bd) : -1;
      }
    }
    __syncthreads();   // the next block reads this block's C
  }
  // the end: the largest C over [max(0, T - P), T), ties to the earlier frame
  {
    const long e0 = T - P > 0 ? T - P : 0;
    double bv = 0.0;
    int bt = 0;   // 1 + the offset from e0, 0: none
    for (long t = e0 + tid; t < T; t += TR_THREADS) {
      const double c = ring[t & (TR_RING - 1)];
      if (!bt || c > bv) { bv = c; bt = (int)(t - e0) + 1; }
    }
    cand_v[tid] = bv;
    cand_t[tid] = bt;
    best_reduce<TR_THREADS>(cand_v, cand_t, tid);
    // the walk back, by thread 0: beat i from the end lands in path[n_out - 1 - i]
    if (tid == 0) {
      const long tstar = e0 + cand_t[0] - 1;
      long n = 0;
      for (long t = tstar; t >= 0; t = back[t]) { path[n_out - 1 - n] = (int)t; ++n; }
      sh_n = n;
      summary[0] = (int)n;
      summary[1] = (int)tstar;
      summary[2] = 0;
      summary[3] = 0;
      cost[0] = cand_v[0];
    }
    __syncthreads();
  }
  // beats to the front in ascending order, -1 behind them; sum of h at the beats in ascending order
  const long n = sh_n, shift = n_out - n;
  double acc = 0.0;
  for (long j0 = 0; j0 < n_out; j0 += TR_THREADS) {
    const long j = j0 + tid;
    const int beat = j < n ? path[j + shift] : -1;
    double h = 0.0;
    if (j < n) {
      const double x = o[beat];
      h = finite64(x) ? x : 0.0;
    }
    cand_v[tid] = h;
    __syncthreads();   // every source of this chunk is read before any of its slots is written
    if (j < n_out) path[j] = beat;
    if (tid == 0 && j0 < n) {
      const int m = n - j0 < TR_THREADS ? (int)(n - j0) : TR_THREADS;
      for (int x = 0; x < m; ++x) acc += cand_v[x];
    }
    __syncthreads();
  }
  if (tid == 0) cost[1] = acc;
}

struct onset_ws {
  long nb, bsum, bpos, bfin, tot, bytes;
};

onset_ws onset_layout(long T) {
  onset_ws w;
  w.nb = (T + ON_ROWS - 1) / ON_ROWS;
  w.bsum = 0;
  w.bpos = w.bsum + up256(8 * w.nb);
  w.bfin = w.bpos + up256(4 * w.nb);
  w.tot = w.bfin + up256(4 * w.nb);
  w.bytes = w.tot + 256;
  return w;
}

int beat_T(const rv_mosaic_desc* d, const char* op) {
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): T=%ld outside [1, 2^31)", op, d->T);
  return RV_OK;
}

}  // namespace

int rv_beat_workspace(rv_mosaic_desc* d) {
  const int rc = beat_T(d, "BEAT_WORKSPACE");
  if (rc) return rc;
  d->ws_bytes = onset_layout(d->T).bytes;
  return RV_OK;
}

int rv_beat_onset(const rv_mosaic_desc* d, void* stream) {
  const int rc = beat_T(d, "BEAT_ONSET");
  if (rc) return rc;
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(BEAT_ONSET): moment (the novelty curve) is null");
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(BEAT_ONSET): result (the onset curve) is null");
  RV_REQUIRE((const void*)d->result != (const void*)d->moment, RV_ERR_SHAPE,
             "rv_mosaic(BEAT_ONSET): result may not be moment: the curve is read again after the sum");
  RV_REQUIRE(d->summary, RV_ERR_NULL, "rv_mosaic(BEAT_ONSET): the summary is null");
  RV_REQUIRE(d->cost, RV_ERR_NULL, "rv_mosaic(BEAT_ONSET): cost is null");
  const onset_ws w = onset_layout(d->T);
  RV_REQUIRE(d->ws_bytes >= w.bytes, RV_ERR_SHAPE, "rv_mosaic(BEAT_ONSET): ws_bytes=%ld, T=%ld needs %ld", d->ws_bytes, d->T,
             w.bytes);
  RV_REQUIRE(d->ws, RV_ERR_NULL, "rv_mosaic(BEAT_ONSET): ws is null, T=%ld needs %ld bytes", d->T, w.bytes);
  RV_REQUIRE(((unsigned long)d->ws & 255) == 0, RV_ERR_SHAPE, "rv_mosaic(BEAT_ONSET): ws is not 256-byte aligned");
  char* const ws = (char*)d->ws;
  double* const bsum = (double*)(ws + w.bsum);
  int* const bpos = (int*)(ws + w.bpos);
  int* const bfin = (int*)(ws + w.bfin);
  double* const tot = (double*)(ws + w.tot);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 blocks((unsigned)w.nb), threads(ON_ROWS);
  hipLaunchKernelGGL(k_onset_part, blocks, threads, 0, st, d->moment, d->T, bsum, bpos, bfin);
  hipLaunchKernelGGL(k_onset_total, dim3(1), threads, 0, st, (const double*)bsum, (const int*)bpos, (const int*)bfin, w.nb,
                     d->T, tot, d->summary, d->cost);
  hipLaunchKernelGGL(k_onset_scale, blocks, threads, 0, st, d->moment, d->T, (const double*)tot, d->result);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_beat_tempogram(const rv_mosaic_desc* d, void* stream) {
  const int rc = beat_T(d, "BEAT_TEMPOGRAM");
  if (rc) return rc;
  RV_REQUIRE(d->width >= 1 && d->width <= TG_WMAX, RV_ERR_SHAPE, "rv_mosaic(BEAT_TEMPOGRAM): width=%ld (the window) outside [1, %d]",
             d->width, TG_WMAX);
  RV_REQUIRE(d->hop >= 1 && d->hop < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(BEAT_TEMPOGRAM): hop=%ld (the frames between two windows) "
             "outside [1, 2^31)", d->hop);
  RV_REQUIRE(d->lag >= 1 && d->lag <= TG_LAGMAX, RV_ERR_SHAPE, "rv_mosaic(BEAT_TEMPOGRAM): lag=%ld (the least lag) outside [1, %d]",
             d->lag, TG_LAGMAX);
  RV_REQUIRE(d->N >= d->lag && d->N <= TG_LAGMAX, RV_ERR_SHAPE, "rv_mosaic(BEAT_TEMPOGRAM): N=%ld (the largest lag) outside "
             "[lag=%ld, %d]", d->N, d->lag, TG_LAGMAX);
  const long nlag = d->N - d->lag + 1, nW = (d->T + d->hop - 1) / d->hop;
  RV_REQUIRE(nW <= (1L << 22), RV_ERR_SHAPE, "rv_mosaic(BEAT_TEMPOGRAM): hop=%ld cuts T=%ld frames into %ld windows, more than 2^22",
             d->hop, d->T, nW);
  RV_REQUIRE(d->ldo >= nlag, RV_ERR_SHAPE, "rv_mosaic(BEAT_TEMPOGRAM): ldo=%ld holds no row of %ld lags", d->ldo, nlag);
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(BEAT_TEMPOGRAM): moment (the onset curve) is null");
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(BEAT_TEMPOGRAM): basis (the window and the prior) is null");
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(BEAT_TEMPOGRAM): result (the tempogram) is null");
  RV_REQUIRE(d->centre, RV_ERR_NULL, "rv_mosaic(BEAT_TEMPOGRAM): centre (the sum over the windows) is null");
  RV_REQUIRE(d->path, RV_ERR_NULL, "rv_mosaic(BEAT_TEMPOGRAM): the path (the windows' periods) is null");
  RV_REQUIRE(d->info, RV_ERR_NULL, "rv_mosaic(BEAT_TEMPOGRAM): info is null");
  RV_REQUIRE(d->cost, RV_ERR_NULL, "rv_mosaic(BEAT_TEMPOGRAM): cost is null");
  const int Wn = (int)d->width, lo = (int)d->lag, hi = (int)d->N;
  const double* const win = d->basis;
  const double* const prior = d->basis + Wn;
  const hipStream_t st = (hipStream_t)stream;
  const int lds = (2 * Wn + hi) * 8;   // 136 KiB at the limits: one workgroup per CU; 24 KiB for 8 s windows at 86 frames a second
  static std::atomic<unsigned long long> attr_done{0};
  lds_opt_in((const void*)k_tempo_acf, TG_LDS_MAX, attr_done);
  // grid.x takes up to 2^31 - 1 windows
  hipLaunchKernelGGL(k_tempo_acf, dim3((unsigned)nW, (unsigned)((nlag + TG_THREADS - 1) / TG_THREADS)), dim3(TG_THREADS), lds, st,
                     d->moment, d->T, Wn, d->hop, lo, hi, win, d->result, d->ldo);
  hipLaunchKernelGGL(k_tempo_period, dim3(blocks_for(nW, 65536)), dim3(TG_THREADS), 0, st, (const double*)d->result, d->ldo, nW,
                     lo, hi, prior, d->path);
  hipLaunchKernelGGL(k_tempo_total, dim3(1), dim3(TG_LAGMAX), 0, st, (const double*)d->result, d->ldo, nW, lo, hi, prior,
                     d->centre, d->info, d->cost);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_beat_track(const rv_mosaic_desc* d, void* stream) {
  const int rc = beat_T(d, "BEAT_TRACK");
  if (rc) return rc;
  RV_REQUIRE(d->lag >= 1 && d->lag <= TR_DMAX, RV_ERR_SHAPE, "rv_mosaic(BEAT_TRACK): lag=%ld (the nearest predecessor) outside [1, %d]",
             d->lag, TR_DMAX);
  RV_REQUIRE(d->width >= d->lag && d->width <= TR_DMAX, RV_ERR_SHAPE, "rv_mosaic(BEAT_TRACK): width=%ld (the furthest predecessor) "
             "outside [lag=%ld, %d]", d->width, d->lag, TR_DMAX);
  RV_REQUIRE(d->N >= 1 && d->N <= TR_DMAX, RV_ERR_SHAPE, "rv_mosaic(BEAT_TRACK): N=%ld (the end window) outside [1, %d]", d->N,
             TR_DMAX);
  const long need = (d->T - 1) / d->lag + 1;
  RV_REQUIRE(d->n_out >= need && d->n_out < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(BEAT_TRACK): n_out=%ld, T=%ld frames at least "
             "lag=%ld apart need %ld (below 2^31)", d->n_out, d->T, d->lag, need);
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(BEAT_TRACK): moment (the onset curve) is null");
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(BEAT_TRACK): basis (the transition scores) is null");
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(BEAT_TRACK): result (the scores C) is null");
  RV_REQUIRE(d->idx, RV_ERR_NULL, "rv_mosaic(BEAT_TRACK): idx (the predecessors) is null");
  RV_REQUIRE(d->path, RV_ERR_NULL, "rv_mosaic(BEAT_TRACK): the path (the beats) is null");
  RV_REQUIRE(d->summary, RV_ERR_NULL, "rv_mosaic(BEAT_TRACK): the summary is null");
  RV_REQUIRE(d->cost, RV_ERR_NULL, "rv_mosaic(BEAT_TRACK): cost is null");
  const int dlo = (int)d->lag;
  int lpf = 1;   // the lanes of a frame: the largest power of two with lpf * dlo <= 1024, at most a wave
  while (lpf < 64 && 2 * lpf * dlo <= TR_THREADS) lpf *= 2;
  hipLaunchKernelGGL(k_beat_track, dim3(1), dim3(TR_THREADS), 0, (hipStream_t)stream, d->moment, d->T, dlo, (int)d->width, (int)d->N,
                     (const double*)d->basis, lpf, d->result, d->idx, d->path, d->n_out, d->summary, d->cost);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
