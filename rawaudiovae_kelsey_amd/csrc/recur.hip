// Recurrence of a latent trajectory (rawaudiovae_kelsey_amd/recur.py): what repeats in a recording.  Two ops of rv_mosaic;
// the rules: include/rawvae_hip.h, "Latent recurrence"; the design and the measured figures: DESIGN.md section 7.15.
//   RV_RECUR_PROFILE    the matrix profile of the distance matrix RV_ALIGN_COST(band 0) wrote: for every window of m rows
//                       the nearest admitted window under the sum of the frame distances along a diagonal.
//                       k_recur_profile: a workgroup takes REC_BI consecutive rows and walks its share of the diagonals
//                       in tiles of REC_BJ, a thread per diagonal e = j - i'.  The REC_BI windows of a diagonal overlap
//                       in all but REC_BI - 1 of their cells, so a thread reads every cell of its diagonal ONCE, from
//                       global memory (the lanes of a wave read consecutive columns of one row: whole lines), and adds it
//                       to the chain of every window that holds it: REC_BI fp64 adds per load, and no staging in LDS,
//                       which could add no reuse to that.  Every chain is still the direct sum in ascending u.  The
//                       thread keeps the best (W, j) of each of the block's rows in registers across the tiles; a wave
//                       reduction and a cross-wave reduction through LDS under the (W, j) order close the rows.
//                       With more than one split the partial pairs go to ws and k_recur_merge takes their least.
//   RV_RECUR_WORKSPACE  the bytes of ws of PROFILE.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "internal.h"

using namespace rv;

namespace {

constexpr int REC_MMAX = 256;     // the longest window
constexpr int REC_BI = 16;        // rows of a workgroup's block: the chains a thread carries
constexpr int REC_BJ = 256;       // diagonals of a tile = threads of a workgroup
constexpr int REC_WAVES = REC_BJ / WAVE;
constexpr long REC_SPLITS_MAX = 1024;
// workgroups the library's own split count aims at: eight rounds of the 1024 the chip holds at once (four to a CU), so that
// a last round with few workgroups in it idles at most an eighth of the launch (measured: 1040 workgroups took the time of 2048)
constexpr long REC_FILL = 8192;

// (w, j) before (bw, bj) in the total order: smaller W, then lower j.  The caller never offers a NaN or +inf W with j >= 0.
__device__ __forceinline__ bool before(double w, int j, double bw, int bj) { return w < bw || (w == bw && j < bj); }

// the chains of the block's rows that hold cell r of the diagonal: row i' holds it as its term u = r - i', 0 <= u < m
__device__ __forceinline__ void add_some(double (&acc)[REC_BI], double v, int r, int m) {
#pragma unroll
  for (int i = 0; i < REC_BI; ++i)
    if ((unsigned)(r - i) < (unsigned)m) acc[i] += v;   // wave-uniform
}

// Block b = blockIdx.x: slab rows [ib, ib + REC_BI), ib = REC_BI b.  Split s = blockIdx.y: the tiles [s nt / S, (s + 1) nt / S)
// of the diagonals e = -(REC_BI - 1) .. N - m; window j = i' + e of row ib + i'.  j - g = e - ib - row0 for every row of the
// block: a diagonal is admitted or not as a whole, and a tile without an admitted diagonal is skipped.  Cell r of diagonal
// e is Dm[ib + r, r + e]: read iff the diagonal is admitted and 0 <= r + e < N (every cell of an existing window is); rows
// stop at n_rows.  S == 1: P and I are written here; otherwise the partial pairs [S, T].
__global__ void __launch_bounds__(REC_BJ)
k_recur_profile(const float* __restrict__ dm, long stride, long n_rows, long N, int m, long T, long row0, long lo, long hi,
                int mirror, long nt, double* __restrict__ P, int* __restrict__ I) {
  __shared__ double sw[REC_BI][REC_WAVES];
  __shared__ int sj[REC_BI][REC_WAVES];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const long ib = (long)blockIdx.x * REC_BI;
  const long S = gridDim.y, s = blockIdx.y;
  const long t0 = s * nt / S, t1 = (s + 1) * nt / S;
  const long left = n_rows - ib;
  const int R = left < REC_BI + m - 1 ? (int)left : REC_BI + m - 1;       // cells of a diagonal inside the slab
  const int r1 = R < REC_BI - 1 ? R : REC_BI - 1;
  const int rm = m < R ? m : R;
  const int r2 = r1 > rm ? r1 : rm;
  const float* const base = dm + ib * stride;
  double bw[REC_BI];
  int bj[REC_BI];
#pragma unroll
  for (int i = 0; i < REC_BI; ++i) { bw[i] = (double)INFINITY; bj[i] = -1; }
  for (long t = t0; t < t1; ++t) {
    const long e0 = t * REC_BJ - (REC_BI - 1);
    const long a = e0 - ib - row0, b = a + REC_BJ - 1;                    // j - g of the tile's diagonals
    if (!((a <= hi && b >= lo) || (mirror && -b <= hi && -a >= lo))) continue;
    const long e = e0 + tid, dd = e - ib - row0;
    const bool adm = (dd >= lo && dd <= hi) || (mirror && -dd >= lo && -dd <= hi);
    double acc[REC_BI];
#pragma unroll
    for (int i = 0; i < REC_BI; ++i) acc[i] = 0.0;
    const float* const diag = base + e;                                    // cell r: diag[r (stride + 1)]
    const long clo = -e, chi = N - e;                                      // r + e in [0, N)  <=>  clo <= r < chi
    int r = 0;
    for (; r < r1; ++r) {                                                  // the first rows' chains only
      const float f = adm && r >= clo && r < chi ? diag[r * (stride + 1)] : 0.f;
      add_some(acc, (double)f, r, m);
    }
#pragma unroll 4
    for (; r < r2; ++r) {                                                  // REC_BI - 1 <= r < m: every chain
      const float f = adm && r >= clo && r < chi ? diag[r * (stride + 1)] : 0.f;
      const double v = (double)f;
#pragma unroll
      for (int i = 0; i < REC_BI; ++i) acc[i] += v;
    }
    for (; r < R; ++r) {                                                   // the last rows' chains only
      const float f = adm && r >= clo && r < chi ? diag[r * (stride + 1)] : 0.f;
      add_some(acc, (double)f, r, m);
    }
#pragma unroll
    for (int i = 0; i < REC_BI; ++i) {
      const long j = e + i;
      // strict <: the diagonals of a thread ascend, so the lower j stays on a tie; NaN and +inf fail the comparison
      if (adm && ib + i < T && j >= 0 && j <= N - m && acc[i] < bw[i] && acc[i] > -(double)INFINITY) {
        bw[i] = acc[i];
        bj[i] = (int)j;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < REC_BI; ++i) {
    double w = bw[i];
    int j = bj[i];
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
      const double ow = __shfl_xor(w, o, WAVE);
      const int oj = __shfl_xor(j, o, WAVE);
      if (before(ow, oj, w, j)) { w = ow; j = oj; }
    }
    if (lane == 0) { sw[i][wave] = w; sj[i][wave] = j; }
  }
  __syncthreads();
  if (tid < REC_BI && ib + tid < T) {
    double w = sw[tid][0];
    int j = sj[tid][0];
    for (int x = 1; x < REC_WAVES; ++x)
      if (before(sw[tid][x], sj[tid][x], w, j)) { w = sw[tid][x]; j = sj[tid][x]; }
    const long at = s * T + ib + tid;                                      // S == 1: s = 0
    P[at] = w;
    I[at] = j;
  }
}

// Row i: the least of its S partial pairs under the (W, j) order.
__global__ void __launch_bounds__(256)
k_recur_merge(const double* __restrict__ pw, const int* __restrict__ pj, long T, long S, double* __restrict__ P,
              int* __restrict__ I) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= T) return;
  double w = pw[i];
  int j = pj[i];
  for (long s = 1; s < S; ++s)
    if (before(pw[s * T + i], pj[s * T + i], w, j)) { w = pw[s * T + i]; j = pj[s * T + i]; }
  P[i] = w;
  I[i] = j;
}

struct recur_plan {
  long nt, splits, pj, bytes;   // tiles of a row block, workgroups they are divided among, the partial j in ws, bytes of ws
};

// The checks RECUR_WORKSPACE and RECUR_PROFILE share (T, N, k, splits), then the plan.
int recur_layout(const rv_mosaic_desc* d, const char* op, recur_plan* p) {
  RV_REQUIRE(d->k >= 1 && d->k <= REC_MMAX, RV_ERR_SHAPE, "rv_mosaic(%s): k=%ld outside [1, %d]", op, d->k, REC_MMAX);
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): T=%ld outside [1, 2^31)", op, d->T);
  RV_REQUIRE(d->N >= d->k && d->N < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): N=%ld outside [k=%ld, 2^31)", op, d->N, d->k);
  RV_REQUIRE(d->splits >= 0 && d->splits <= REC_SPLITS_MAX, RV_ERR_SHAPE, "rv_mosaic(%s): splits=%ld outside [0, %ld]", op,
             d->splits, REC_SPLITS_MAX);
  p->nt = (d->N - d->k + REC_BI + REC_BJ - 1) / REC_BJ;
  p->splits = d->splits;
  if (!p->splits) {   // enough workgroups for the chip whatever T is, never more than there are tiles
    const long nb = (d->T + REC_BI - 1) / REC_BI, want = (REC_FILL + nb - 1) / nb;
    p->splits = want < p->nt ? want : p->nt;
  }
  p->pj = up256(8 * p->splits * d->T);
  p->bytes = p->splits > 1 ? p->pj + up256(4 * p->splits * d->T) : 0;
  return RV_OK;
}

}  // namespace

int rv_recur_workspace(rv_mosaic_desc* d) {
  recur_plan p;
  const int rc = recur_layout(d, "RECUR_WORKSPACE", &p);
  if (rc) return rc;
  d->ws_bytes = p.bytes;
  return RV_OK;
}

int rv_recur_profile(const rv_mosaic_desc* d, void* stream) {
  static const char* const op = "RECUR_PROFILE";
  recur_plan p;
  const int rc = recur_layout(d, op, &p);
  if (rc) return rc;
  RV_REQUIRE(d->n_rows >= d->k && d->T == d->n_rows - d->k + 1, RV_ERR_SHAPE,
             "rv_mosaic(%s): T=%ld is not n_rows=%ld - k + 1 (k=%ld)", op, d->T, d->n_rows, d->k);
  RV_REQUIRE(d->stride >= d->N, RV_ERR_SHAPE, "rv_mosaic(%s): stride=%ld below N=%ld", op, d->stride, d->N);
  RV_REQUIRE(d->stride < (1L << 31) && d->n_rows * d->stride < (1L << 31), RV_ERR_SHAPE,
             "rv_mosaic(%s): n_rows=%ld rows of stride=%ld reach 2^31", op, d->n_rows, d->stride);
  RV_REQUIRE(d->row0 >= 0 && d->row0 < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): row0=%ld outside [0, 2^31)", op, d->row0);
  RV_REQUIRE(d->lag > -(1L << 31) && d->lag < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): lag=%ld outside (-2^31, 2^31)", op, d->lag);
  RV_REQUIRE(d->width > -(1L << 31) && d->width < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): width=%ld outside (-2^31, 2^31)", op,
             d->width);
  RV_REQUIRE(d->lag <= d->width, RV_ERR_SHAPE, "rv_mosaic(%s): lag=%ld above width=%ld", op, d->lag, d->width);
  RV_REQUIRE(d->mode == 0 || d->mode == RV_RECUR_MIRROR, RV_ERR_SHAPE, "rv_mosaic(%s): mode=%ld is neither 0 nor RV_RECUR_MIRROR", op,
             d->mode);
  RV_REQUIRE(d->local_costs, RV_ERR_NULL, "rv_mosaic(%s): local_costs is null", op);
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(%s): result is null", op);
  RV_REQUIRE(d->idx, RV_ERR_NULL, "rv_mosaic(%s): idx is null", op);
  double* pw = d->result;
  int* pj = d->idx;
  if (p.splits > 1) {
    RV_REQUIRE(d->ws_bytes >= p.bytes, RV_ERR_SHAPE, "rv_mosaic(%s): ws_bytes=%ld, T=%ld with splits=%ld needs %ld", op, d->ws_bytes,
               d->T, p.splits, p.bytes);
    RV_REQUIRE(d->ws, RV_ERR_NULL, "rv_mosaic(%s): ws is null, T=%ld with splits=%ld needs %ld bytes", op, d->T, p.splits, p.bytes);
    RV_REQUIRE(((unsigned long)d->ws & 255) == 0, RV_ERR_SHAPE, "rv_mosaic(%s): ws is not 256-byte aligned", op);
    pw = (double*)d->ws;
    pj = (int*)((char*)d->ws + p.pj);
  }
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_recur_profile, dim3((unsigned)((d->T + REC_BI - 1) / REC_BI), (unsigned)p.splits), dim3(REC_BJ), 0, st,
                     (const float*)d->local_costs, d->stride, d->n_rows, d->N, (int)d->k, d->T, d->row0, d->lag, d->width,
                     (int)d->mode, p.nt, pw, pj);
  if (p.splits > 1)
    hipLaunchKernelGGL(k_recur_merge, dim3((unsigned)((d->T + 255) / 256)), dim3(256), 0, st, (const double*)pw, (const int*)pj,
                       d->T, p.splits, d->result, d->idx);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
