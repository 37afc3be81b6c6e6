// Structure of a latent trajectory (rawaudiovae_kelsey_amd/structure.py): where a recording changes.  Three ops of
// rv_mosaic; the rules: include/rawvae_hip.h, "Latent structure"; the design and the measured figures: DESIGN.md
// section 7.13.
//   RV_STRUCT_NOVELTY    a tapered checkerboard kernel slid along the diagonal of the banded self-distance matrix that
//                        RV_ALIGN_COST(a = b) wrote: k_struct_novelty, a thread per (frame t, row u of its (2R) x (2R)
//                        window), 1024 / 2R consecutive frames per workgroup.  The window those frames share goes
//                        through LDS once, in chunks of 32 columns (a wave loads two runs of 32 consecutive band slots,
//                        the pitch of 33 floats is odd: no bank conflict on either side); every thread carries its
//                        row's four chains across the chunks in ascending v, the row results go through LDS and one
//                        lane per (frame, chain) adds them in ascending u.  No atomics, one launch.
//   RV_STRUCT_PEAKS      the boundaries of a novelty curve: the mean |nov| in RV_EVAL_DIMS's order (k_peaks_part,
//                        k_peaks_total), the test of every frame and its rank among its block's boundaries
//                        (k_peaks_flag), the scan over the blocks (k_peaks_scan) and the offsets (k_peaks_write).
//   RV_STRUCT_WORKSPACE  the bytes of ws of PEAKS.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "internal.h"

// every product below is rounded before it is added (the header's rule; numpy reproduces it bit for bit)
#pragma clang fp contract(off)

using namespace rv;

namespace {

constexpr int NOV_RMAX = 512;
// k_struct_novelty runs NOV_THREADS threads whatever R is: a workgroup takes TB = NOV_THREADS / 2R consecutive frames (one
// beyond R = 256) and stages the window they share once.
constexpr int NOV_THREADS = 1024;
constexpr int NOV_VC = 32, NOV_PITCH = NOV_VC + 1;   // columns of a chunk, floats between two rows of it in LDS
constexpr int NOV_SUMS = 4 * NOV_THREADS * 8;        // bytes of the row results [4][NOV_THREADS] fp64, which reuse the tile
constexpr int NOV_LDS_MAX = NOV_THREADS * NOV_PITCH * 4;
constexpr int PK_ROWS = 256;             // rows of one block of the mean |nov|: RV_EVAL_DIMS's (the header states it)
constexpr long PK_MAX = 65536;           // the largest lag and width

// A workgroup takes the TB frames t0 .. t0 + TB - 1; thread (f, u) = (tid / 2R, tid % 2R) owns row u of frame t0 + f's
// window.  The windows of the TB frames lie in one (2R + TB - 1)^2 window of the matrix, from row and column
// base = t0 - R: union index x is matrix index base + x, and row u / column v of frame f are union row u + f / column
// v + f.  The union window goes through LDS once, in chunks of 32 columns; [xlo, xhi) are its indices inside the
// matrix (the others are skipped by index), and cells further than 2R - 1 off the diagonal belong to no frame's
// window (and to no band slot).  A row's chain over v < R and its chain over v >= R are its within and cross sums,
// which of the two depending on the side of the row.
__global__ void __launch_bounds__(NOV_THREADS)
k_struct_novelty(const float* __restrict__ dm, long T, long W, long r, int R, int TB, const double* __restrict__ w,
                 double* __restrict__ nov) {
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [2R + TB - 1][NOV_PITCH], at least NOV_SUMS + 32 TB bytes
  __shared__ double wt[NOV_THREADS];
  const int tid = threadIdx.x, n = 2 * R, rows_u = n + TB - 1;
  const long t0 = (long)blockIdx.x * TB, base = t0 - R;
  const int xlo = base < 0 ? (int)-base : 0, xhi = T - base < rows_u ? (int)(T - base) : rows_u;
  if (tid < n) wt[tid] = w[tid];
  const int f = tid / n, u = tid - f * n, xr = u + f;
  const bool rowok = f < TB && t0 + f < T && xr >= xlo && xr < xhi;
  const int vlo = xlo - f > 0 ? xlo - f : 0, vhi = xhi - f < n ? xhi - f : n;   // this frame's columns inside the matrix
  const int sv = tid & (NOV_VC - 1), su = tid / NOV_VC;   // this thread's column of every chunk, its first row
  double wu = 0.0, pa = 0.0, ca = 0.0, pb = 0.0, cb = 0.0;   // sum c d and sum c over v < R (a) and over v >= R (b)
  for (int v0 = 0; v0 < rows_u; v0 += NOV_VC) {
    __syncthreads();   // the chunk before has been read (first pass: wt is written)
    const int x = v0 + sv;
    const bool colok = x >= xlo && x < xhi;
    for (int uu = su; uu < rows_u; uu += NOV_THREADS / NOV_VC) {
      const bool ok = colok && uu >= xlo && uu < xhi && x - uu < n && uu - x < n;
      tile[uu * NOV_PITCH + sv] = ok ? dm[(base + uu) * W + (r ? x - uu + r : base + x)] : 0.f;
    }
    __syncthreads();
    if (rowok) {
      wu = wt[u];
      const float* const row = tile + xr * NOV_PITCH;
      const int off = f - v0;   // row[off + v]: column v of this frame's window
      const int a = v0 - f > vlo ? v0 - f : vlo, b = v0 + NOV_VC - f < vhi ? v0 + NOV_VC - f : vhi;
      const int mid = R < a ? a : (R > b ? b : R);
#pragma unroll 4
      for (int v = a; v < mid; ++v) {
        const double c = wu * wt[v];
        pa += c * (double)row[off + v];
        ca += c;
      }
#pragma unroll 4
      for (int v = mid; v < b; ++v) {
        const double c = wu * wt[v];
        pb += c * (double)row[off + v];
        cb += c;
      }
    }
  }
  __syncthreads();
  const bool past = u < R;
  double* const rows = reinterpret_cast<double*>(tile);   // [4][NOV_THREADS]; a row outside the matrix adds +0
  double* const fin = rows + 4 * NOV_THREADS;             // [TB][4]
  rows[tid] = past ? pb : pa;                      // cross
  rows[NOV_THREADS + tid] = past ? cb : ca;        // its weights
  rows[2 * NOV_THREADS + tid] = past ? pa : pb;    // within
  rows[3 * NOV_THREADS + tid] = past ? ca : cb;
  __syncthreads();
  for (int s = tid; s < 4 * TB; s += NOV_THREADS) {   // frame s / 4, chain s % 4: the frame's rows in ascending u
    const double* const part = rows + (s & 3) * NOV_THREADS + (s >> 2) * n;
    double acc = 0.0;
    for (int k = 0; k < n; ++k) acc += part[k];
    fin[s] = acc;
  }
  __syncthreads();
  if (tid < TB && t0 + tid < T) {
    const double* const q = fin + 4 * tid;
    nov[t0 + tid] = (q[1] > 0.0 && q[3] > 0.0) ? q[0] / q[1] - q[2] / q[3] : 0.0;
  }
}

__device__ __forceinline__ bool finite64(double v) { return fabs(v) < (double)INFINITY; }

struct peaks_total {
  double G;
  long finite;
};

// Block b = rows [256 b, 256 b + 256): sum of |nov| over the finite entries in ascending t from +0, and their count.
__global__ void __launch_bounds__(PK_ROWS)
k_peaks_part(const double* __restrict__ nov, long T, double* __restrict__ bsum, int* __restrict__ bcnt) {
  __shared__ double vals[PK_ROWS];
  const int tid = threadIdx.x;
  const long t = (long)blockIdx.x * PK_ROWS + tid;
  const double v = t < T ? nov[t] : (double)NAN;
  vals[tid] = v;
  __syncthreads();
  if (tid == 0) {
    double acc = 0.0;
    int cnt = 0;
    for (int x = 0; x < PK_ROWS; ++x)
      if (finite64(vals[x])) { acc += fabs(vals[x]); ++cnt; }
    bsum[blockIdx.x] = acc;
    bcnt[blockIdx.x] = cnt;
  }
}

// ONE workgroup: the block sums in ascending order from +0 (fetched 256 at a time, thread 0 adds them), one division.
__global__ void __launch_bounds__(PK_ROWS)
k_peaks_total(const double* __restrict__ bsum, const int* __restrict__ bcnt, long nb, peaks_total* __restrict__ tot) {
  __shared__ double vals[PK_ROWS];
  __shared__ int cnts[PK_ROWS];
  const int tid = threadIdx.x;
  double acc = 0.0;
  long cnt = 0;
  for (long b0 = 0; b0 < nb; b0 += PK_ROWS) {
    const long b = b0 + tid;
    vals[tid] = b < nb ? bsum[b] : 0.0;
    cnts[tid] = b < nb ? bcnt[b] : 0;
    __syncthreads();
    if (tid == 0) {
      const int m = nb - b0 < PK_ROWS ? (int)(nb - b0) : PK_ROWS;
      for (int x = 0; x < m; ++x) { acc += vals[x]; cnt += cnts[x]; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    tot->G = cnt ? acc / (double)cnt : 0.0;
    tot->finite = cnt;
  }
}

// Frame t's test, then its rank among the boundaries of its block of 256 (-1: no boundary) and the block's count.
__global__ void __launch_bounds__(PK_ROWS)
k_peaks_flag(const double* __restrict__ nov, long T, long g, long m, double delta, const peaks_total* __restrict__ tot,
             int* __restrict__ rank, int* __restrict__ bflag) {
  __shared__ int scan[PK_ROWS];
  const int tid = threadIdx.x;
  const long t = (long)blockIdx.x * PK_ROWS + tid;
  const long ge = g > 1 ? g : 1;
  bool is = false;
  if (t < T && t >= ge && t <= T - ge) {
    const double x = nov[t];
    if (finite64(x)) {
      const long lo = t - m > 0 ? t - m : 0, hi = t + m < T - 1 ? t + m : T - 1;
      double acc = 0.0;
      long cnt = 0;
      for (long s = lo; s <= hi; ++s) {
        const double y = nov[s];
        if (finite64(y)) { acc += y; ++cnt; }
      }
      const double thr = acc / (double)cnt + delta * tot->G;
      is = x > thr;
      for (long s = t - g; is && s < t; ++s) {
        const double y = nov[s];
        if (finite64(y) && !(x > y)) is = false;
      }
      const long last = t + g < T - 1 ? t + g : T - 1;
      for (long s = t + 1; is && s <= last; ++s) {
        const double y = nov[s];
        if (finite64(y) && !(x >= y)) is = false;
      }
    }
  }
  scan[tid] = is ? 1 : 0;
  __syncthreads();
  for (int o = 1; o < PK_ROWS; o <<= 1) {   // inclusive scan in LDS
    const int add = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  if (t < T) rank[t] = is ? scan[tid] - 1 : -1;
  if (tid == PK_ROWS - 1) bflag[blockIdx.x] = scan[tid];
}

// ONE workgroup: the exclusive scan of the blocks' counts; summary = {F, finite entries, 0, 0}.
__global__ void __launch_bounds__(PK_ROWS)
k_peaks_scan(const int* __restrict__ bflag, long nb, const peaks_total* __restrict__ tot, int* __restrict__ boff,
             int* __restrict__ summary) {
  __shared__ int cnts[PK_ROWS], offs[PK_ROWS];
  const int tid = threadIdx.x;
  int run = 0;   // thread 0's
  for (long b0 = 0; b0 < nb; b0 += PK_ROWS) {
    const long b = b0 + tid;
    cnts[tid] = b < nb ? bflag[b] : 0;
    __syncthreads();
    if (tid == 0)
      for (int x = 0; x < PK_ROWS; ++x) { offs[x] = run; run += cnts[x]; }
    __syncthreads();
    if (b < nb) boff[b] = offs[tid];
    __syncthreads();
  }
  if (tid == 0) {
    summary[0] = run + 1;
    summary[1] = (int)tot->finite;
    summary[2] = 0;
    summary[3] = 0;
  }
}

// path[0] = 0 and path[x] for x >= F by thread x; path[1 .. F - 1] by the boundaries' own threads.
__global__ void __launch_bounds__(PK_ROWS)
k_peaks_write(const int* __restrict__ rank, const int* __restrict__ boff, const int* __restrict__ summary, long T,
              int* __restrict__ path) {
  const long x = (long)blockIdx.x * PK_ROWS + threadIdx.x;
  if (x > T) return;
  const long F = summary[0];
  if (x == 0) path[0] = 0;
  else if (x == F) path[x] = (int)T;
  else if (x > F) path[x] = -1;
  if (x < T) {
    const int rk = rank[x];
    if (rk >= 0) path[1 + boff[x / PK_ROWS] + rk] = (int)x;
  }
}

struct peaks_ws {
  long nb, bsum, bcnt, tot, rank, bflag, boff, bytes;
};

peaks_ws peaks_layout(long T) {
  peaks_ws w;
  w.nb = (T + PK_ROWS - 1) / PK_ROWS;
  w.bsum = 0;
  w.bcnt = w.bsum + up256(8 * w.nb);
  w.tot = w.bcnt + up256(4 * w.nb);
  w.rank = w.tot + 256;
  w.bflag = w.rank + up256(4 * T);
  w.boff = w.bflag + up256(4 * w.nb);
  w.bytes = w.boff + up256(4 * w.nb);
  return w;
}

// T of PEAKS and WORKSPACE: path holds T + 1 int32 whose largest value is T
int peaks_T(const rv_mosaic_desc* d, const char* op) {
  RV_REQUIRE(d->T >= 1 && d->T < INT_MAX, RV_ERR_SHAPE, "rv_mosaic(%s): T=%ld outside [1, 2^31 - 1)", op, d->T);
  return RV_OK;
}

}  // namespace

int rv_struct_workspace(rv_mosaic_desc* d) {
  const int rc = peaks_T(d, "STRUCT_WORKSPACE");
  if (rc) return rc;
  d->ws_bytes = peaks_layout(d->T).bytes;
  return RV_OK;
}

int rv_struct_novelty(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(STRUCT_NOVELTY): T=%ld outside [1, 2^31)", d->T);
  RV_REQUIRE(d->k >= 1 && d->k <= NOV_RMAX, RV_ERR_SHAPE, "rv_mosaic(STRUCT_NOVELTY): k=%ld outside [1, %d]", d->k, NOV_RMAX);
  RV_REQUIRE(d->band >= 0 && d->band < (1L << 30), RV_ERR_SHAPE, "rv_mosaic(STRUCT_NOVELTY): band=%ld outside [0, 2^30)",
             d->band);
  RV_REQUIRE(d->band == 0 || d->band >= 2 * d->k - 1, RV_ERR_SHAPE,
             "rv_mosaic(STRUCT_NOVELTY): band=%ld does not hold the window of k=%ld; the least band that does is %ld "
             "(0: the whole matrix)", d->band, d->k, 2 * d->k - 1);
  const long W = d->band ? 2 * d->band + 1 : d->T;
  RV_REQUIRE(d->T * W < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(STRUCT_NOVELTY): T=%ld rows of %ld band slots (band=%ld) reach 2^31",
             d->T, W, d->band);
  RV_REQUIRE(d->local_costs, RV_ERR_NULL, "rv_mosaic(STRUCT_NOVELTY): local_costs is null");
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(STRUCT_NOVELTY): moment is null");
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(STRUCT_NOVELTY): result is null");
  const int R = (int)d->k, TB = NOV_THREADS / (2 * R);
  const int tile_bytes = (2 * R + TB - 1) * NOV_PITCH * 4, sums_bytes = NOV_SUMS + 32 * TB;
  const int lds = tile_bytes > sums_bytes ? tile_bytes : sums_bytes;   // 132 KiB at R = 512: one workgroup per CU
  static std::atomic<unsigned long long> attr_done{0};
  lds_opt_in((const void*)k_struct_novelty, NOV_LDS_MAX, attr_done);
  hipLaunchKernelGGL(k_struct_novelty, dim3((unsigned)((d->T + TB - 1) / TB)), dim3(NOV_THREADS), lds, (hipStream_t)stream,
                     d->local_costs, d->T, W, d->band, R, TB, d->moment, d->result);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_struct_peaks(const rv_mosaic_desc* d, void* stream) {
  const int rc = peaks_T(d, "STRUCT_PEAKS");
  if (rc) return rc;
  RV_REQUIRE(d->lag >= 0 && d->lag <= PK_MAX, RV_ERR_SHAPE, "rv_mosaic(STRUCT_PEAKS): lag=%ld outside [0, %ld]", d->lag, PK_MAX);
  RV_REQUIRE(d->width >= 0 && d->width <= PK_MAX, RV_ERR_SHAPE, "rv_mosaic(STRUCT_PEAKS): width=%ld outside [0, %ld]", d->width,
             PK_MAX);
  RV_REQUIRE(d->lam >= 0.f && d->lam < INFINITY, RV_ERR_SHAPE, "rv_mosaic(STRUCT_PEAKS): lam=%g must be finite and not negative",
             (double)d->lam);
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(STRUCT_PEAKS): moment is null");
  RV_REQUIRE(d->path, RV_ERR_NULL, "rv_mosaic(STRUCT_PEAKS): the path is null");
  RV_REQUIRE(d->summary, RV_ERR_NULL, "rv_mosaic(STRUCT_PEAKS): the summary is null");
  const peaks_ws w = peaks_layout(d->T);
  RV_REQUIRE(d->ws_bytes >= w.bytes, RV_ERR_SHAPE, "rv_mosaic(STRUCT_PEAKS): ws_bytes=%ld, T=%ld needs %ld", d->ws_bytes, d->T,
             w.bytes);
  RV_REQUIRE(d->ws, RV_ERR_NULL, "rv_mosaic(STRUCT_PEAKS): ws is null, T=%ld needs %ld bytes", d->T, w.bytes);
  RV_REQUIRE(((unsigned long)d->ws & 255) == 0, RV_ERR_SHAPE, "rv_mosaic(STRUCT_PEAKS): ws is not 256-byte aligned");
  char* const ws = (char*)d->ws;
  double* const bsum = (double*)(ws + w.bsum);
  int* const bcnt = (int*)(ws + w.bcnt);
  peaks_total* const tot = (peaks_total*)(ws + w.tot);
  int* const rank = (int*)(ws + w.rank);
  int* const bflag = (int*)(ws + w.bflag);
  int* const boff = (int*)(ws + w.boff);
  const hipStream_t st = (hipStream_t)stream;
  const dim3 blocks((unsigned)w.nb), threads(PK_ROWS);
  hipLaunchKernelGGL(k_peaks_part, blocks, threads, 0, st, d->moment, d->T, bsum, bcnt);
  hipLaunchKernelGGL(k_peaks_total, dim3(1), threads, 0, st, (const double*)bsum, (const int*)bcnt, w.nb, tot);
  hipLaunchKernelGGL(k_peaks_flag, blocks, threads, 0, st, d->moment, d->T, d->lag, d->width, (double)d->lam,
                     (const peaks_total*)tot, rank, bflag);
  hipLaunchKernelGGL(k_peaks_scan, dim3(1), threads, 0, st, (const int*)bflag, w.nb, (const peaks_total*)tot, boff, d->summary);
  hipLaunchKernelGGL(k_peaks_write, dim3((unsigned)((d->T + 1 + PK_ROWS - 1) / PK_ROWS)), threads, 0, st, (const int*)rank,
                     (const int*)boff, (const int*)d->summary, d->T, d->path);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
