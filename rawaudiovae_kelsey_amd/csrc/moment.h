// The fp64 corpus statistics of the audio tools: the second moments of RV_PCA_MOMENTS (pca.hip, the covariance) and
// RV_PCA_LAGCOV (walk.hip, the lag-1 moment), and the blocked column sums of RV_PCA_MOMENTS (the mean) and RV_EVAL_DIMS
// (eval.hip, the KL sums).  Defined here once, down to the order of every add; no atomics anywhere, so the bits depend
// on the data and its shape alone.
//   Second moment.  d[t][c] = (double)x[t][c] - centre[c].  Element (i, j) of the range of RANGE rows from t0 is
//   sum_t a[t][i] b[t][j], with a = b = d (covariance, t a row), a[t] = d[t + 1], b[t] = keep[t] d[t] (lag-1, t a
//   pair), a = gamma, b = y or y o y, two fp64 matrices (the weighted moments of RV_HMM_MSTEP, hmm.hip), or a = keep (u - ubar),
//   b = keep (v - vbar), two fp64 matrices about their column means (RV_ATTR_FIT, attr.hip), or a[p] = fl(g[p + 1] r[p + 1])
//   (or g[p + 1]), b[p] = keep[p] r[p] (or its square, or that of r[p + 1]), the gated moments of a pair of rows under the
//   weights of its second row (RV_SWITCH_MOMENTS, switch.hip): v_mfma_f64_16x16x4_f64 over the rows t0, t0 + 4, .. in ascending order from +0, each instruction adding its
//   four rows to the element.  Rows and columns beyond the data stage zeros.  Then the ranges' partials of an element
//   in ascending range order from +0 (range_sum), and the caller's one division.
//   Column sum.  Blocks of ROWS rows: a block's terms in ascending t from +0 (colsum_block), then the block sums in
//   ascending block order from +0 (colsum_total).
// The tiling and the measured figures: DESIGN.md sections 7.9 to 7.11.
#pragma once
#include "common.h"

namespace rv {
namespace mom {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int RANGE = 4096;        // rows (pairs) of one range (the public header states it)
constexpr int CHUNK = 32;          // rows staged in LDS at a time
constexpr int MT = 64;             // the workgroup's tile: 4 x 4 MFMA tiles of 16 x 16, one row of them per wave
constexpr int LD = 80;             // LDS row pitch in doubles: rows k .. k + 3 of an operand fall into disjoint banks
constexpr int TILE_THREADS = 256;
constexpr int STAGE = CHUNK * LD;  // doubles of one operand's LDS stage
constexpr int TILE = MT * MT;      // doubles of one partial tile
constexpr int ROWS = 256;          // rows of one block of a column sum (the public header states it)
constexpr int THREADS = 64;        // a column per thread

// Number of the 64 x 64 tile (I, J) within a range: among the tiles on or above the diagonal, row by row (J >= I, the
// covariance), or in the full square (the lag-1 moment).
__host__ __device__ __forceinline__ int tile_number(int I, int J, int nI) { return I * nI - I * (I - 1) / 2 + (J - I); }
__host__ __device__ __forceinline__ int square_number(int I, int J, int nI) { return I * nI + J; }

// The partial tiles of `rows` rows (pairs) of L columns in ws
struct tiles {
  long n_ranges, doubles;
  int nI, n_tiles;   // tiles along a side, tiles per range
};

inline tiles tile_layout(long rows, long L, bool lag) {
  tiles w;
  w.n_ranges = (rows + RANGE - 1) / RANGE;
  w.nI = (int)((L + MT - 1) / MT);
  w.n_tiles = lag ? w.nI * w.nI : w.nI * (w.nI + 1) / 2;
  w.doubles = w.n_ranges * w.n_tiles * (long)TILE;
  return w;
}

// The operands of a tile as its loop sees them.  A thread carries one column of each operand: `raw` is what it holds of a
// row between the load and the staging, load() reads row tr of its two columns, left() and right() are the doubles that
// go into LDS, keeps() whether the right operand of the row counts at all.
// centred: d = (double)x - centre of one fp32 matrix on both sides (the covariance), or -- LAG -- row t + 1 on the left
// and keep[t] d[t] on the right (the lag-1 moment).
template <bool LAG>
struct centred {
  const float* __restrict__ xa;
  const float* __restrict__ xb;
  const unsigned char* __restrict__ keep;
  long L;
  double ma, mb;
  bool diag;
  struct raw { float a, b; unsigned char k; };
  __device__ __forceinline__ void load(long tr, raw& r) const {
    if constexpr (LAG) {
      r.a = xa[(tr + 1) * L];
      r.b = xb[tr * L];
      r.k = keep[tr];
    } else {
      r.a = xa[tr * L];
      r.b = diag ? 0.f : xb[tr * L];
    }
  }
  __device__ __forceinline__ double left(const raw& r) const { return (double)r.a - ma; }
  __device__ __forceinline__ double right(const raw& r) const { return (double)r.b - mb; }
  __device__ __forceinline__ bool keeps(const raw& r) const { return LAG ? r.k != 0 : true; }
};
// weighted: two different fp64 matrices, ga [n, lda] on the left as it stands and yb [n, ldb] on the right, or --
// SQUARE -- its elementwise square, one rounded product formed while staging (the weighted moments of hmm.hip).
template <bool SQUARE>
struct weighted {
  const double* __restrict__ ga;
  const double* __restrict__ yb;
  long lda, ldb;
  struct raw { double a, b; };
  __device__ __forceinline__ void load(long tr, raw& r) const {
    r.a = ga[tr * lda];
    r.b = yb[tr * ldb];
  }
  __device__ __forceinline__ double left(const raw& r) const { return r.a; }
  __device__ __forceinline__ double right(const raw& r) const { return SQUARE ? r.b * r.b : r.b; }
  __device__ __forceinline__ bool keeps(const raw&) const { return true; }
};

// paired: two fp64 matrices a [n, lda] and b [n, ldb], each minus its column's mean, times the row's keep byte: a row whose
// byte is 0 stages zeros on both sides (the centred moments of RV_ATTR_FIT, attr.hip).
struct paired {
  const double* __restrict__ a;
  const double* __restrict__ b;
  const unsigned char* __restrict__ keep;
  long lda, ldb;
  double ma, mb;
  struct raw { double a, b; unsigned char k; };
  __device__ __forceinline__ void load(long tr, raw& r) const {
    r.a = a[tr * lda];
    r.b = b[tr * ldb];
    r.k = keep[tr];
  }
  __device__ __forceinline__ double left(const raw& r) const { return r.k ? r.a - ma : 0.0; }
  __device__ __forceinline__ double right(const raw& r) const { return r.b - mb; }
  __device__ __forceinline__ bool keeps(const raw& r) const { return r.k != 0; }
};

// gated: the moments of a pair (p, p + 1) of rows of one fp64 matrix r [n + 1, ldr] under the weights g [n + 1, ldg] of the
// pair's SECOND row and the pair's keep byte, which gates the right operand only (RV_SWITCH_MOMENTS, switch.hip).
//   GATED_CROSS    left = fl(g[p + 1, col] r[p + 1, a]), one rounded product formed while staging, `col` one fixed column of
//                  g; right = keep[p] ? r[p, b] : 0
//   GATED_NEXT_SQ  left = g[p + 1, a]; right = keep[p] ? fl(r[p + 1, b]^2) : 0
//   GATED_THIS_SQ  left = g[p + 1, a]; right = keep[p] ? fl(r[p, b]^2) : 0
enum { GATED_CROSS = 0, GATED_NEXT_SQ = 1, GATED_THIS_SQ = 2 };
template <int FORM>
struct gated {
  const double* __restrict__ g;    // row 0 of the thread's column of g
  const double* __restrict__ ra;   // ... of r on the left (GATED_CROSS)
  const double* __restrict__ rb;   // ... of r on the right
  const unsigned char* __restrict__ keep;
  long ldg, ldr;
  struct raw { double g, a, b; unsigned char k; };
  __device__ __forceinline__ void load(long tr, raw& r) const {
    r.g = g[(tr + 1) * ldg];
    r.a = FORM == GATED_CROSS ? ra[(tr + 1) * ldr] : 1.0;
    r.b = rb[(FORM == GATED_NEXT_SQ ? tr + 1 : tr) * ldr];
    r.k = keep[tr];
  }
  __device__ __forceinline__ double left(const raw& r) const { return FORM == GATED_CROSS ? r.g * r.a : r.g; }
  __device__ __forceinline__ double right(const raw& r) const { return FORM == GATED_CROSS ? r.b : r.b * r.b; }
  __device__ __forceinline__ bool keeps(const raw& r) const { return r.k != 0; }
};

// The thread's column of both operands at rows t, t + 4, ..  A row beyond the range is read from the range's last row
// (the caller stores a zero in its place).
template <class Ops, int PER>
__device__ __forceinline__ void fetch(const Ops& ops, long t, long t1, typename Ops::raw (&f)[PER]) {
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const long tt = t + 4 * i;
    ops.load(tt < t1 ? tt : t1 - 1, f[i]);
  }
}

// One range (blockIdx.x) of the n rows (pairs) and one 64 x 64 tile of the product, which is number blockIdx.y of the
// n_tiles of a range in part.  TILE_THREADS threads; As and Bs are STAGE doubles of LDS each.  Thread (cc = lane, ti)
// stages column cc of both operands (va, vb: whether its column of the left / right operand exists).  Wave w owns the
// MFMA tiles (w, 0 .. 3) of the tile; on a diagonal tile (`diag`: both operands are the same columns of the same
// matrix) those left of the diagonal are skipped (and not written) and B is read from As.
// v_mfma_f64_16x16x4_f64: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; with
// A[i][k] = a[t + k][i0 + i] and B[k][j] = b[t + k][j0 + j] one instruction adds four rows to the tile.  Its result:
// column l & 15, row (l >> 4) + 4 reg.
template <class Ops>
__device__ __forceinline__ void tile_loop(double* As, double* Bs, const Ops& ops, long n, bool va, bool vb, bool diag,
                                          int n_tiles, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, ti = threadIdx.x >> 6;
  const double* const Bsrc = diag ? As : Bs;
  f64x4 acc[4];
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) acc[tj] = f64x4{0.0, 0.0, 0.0, 0.0};
  const long t0 = (long)blockIdx.x * RANGE, t1 = t0 + RANGE < n ? t0 + RANGE : n;
  // Staging: the thread carries its columns for the rows ti, ti + 4, .. of a chunk.  The loads of the next chunk are
  // issued before the MFMAs of this one; a row or column beyond the data is read from a clamped address and replaced
  // by zero on its way into LDS.
  constexpr int PER = CHUNK / (TILE_THREADS / MT);   // rows per thread and chunk
  const int cc = lane;
  typename Ops::raw f[PER];
  fetch<Ops, PER>(ops, t0 + ti, t1, f);
  for (long tc = t0; tc < t1; tc += CHUNK) {
    __syncthreads();   // the MFMAs of the chunk before have read LDS
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int r = ti + 4 * i;
      const bool vt = tc + r < t1;
      As[r * LD + cc] = (vt && va) ? ops.left(f[i]) : 0.0;
      if (!diag) Bs[r * LD + cc] = (vt && vb && ops.keeps(f[i])) ? ops.right(f[i]) : 0.0;
    }
    __syncthreads();
    if (tc + CHUNK < t1) fetch<Ops, PER>(ops, tc + CHUNK + ti, t1, f);
#pragma unroll
    for (int kk = 0; kk < CHUNK; kk += 4) {
      const int row = (kk + (lane >> 4)) * LD + (lane & 15);
      const double a = As[row + ti * 16];
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) {
        if (diag && tj < ti) continue;   // wave-uniform
        const double b = Bsrc[row + tj * 16];
        acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[tj], 0, 0, 0);
      }
    }
  }
  double* const part_tile = part + ((long)blockIdx.x * n_tiles + blockIdx.y) * TILE;
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    if (diag && tj < ti) continue;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      part_tile[(ti * 16 + (lane >> 4) + 4 * reg) * MT + tj * 16 + (lane & 15)] = acc[tj][reg];
  }
}

// The tile (I, J) of the second moment of x [n (+ 1 when LAG), L] about centre: the covariance's (J >= I, the diagonal
// tiles in their half form) or the lag-1 moment's.
template <bool LAG>
__device__ __forceinline__ void moment_tile(double* As, double* Bs, const float* __restrict__ x, long n, int L,
                                            const double* __restrict__ centre, const unsigned char* __restrict__ keep,
                                            int I, int J, int n_tiles, double* __restrict__ part) {
  const bool diag = !LAG && I == J;
  const int cc = threadIdx.x & 63;
  const int ca = I * MT + cc, cb = J * MT + cc;
  const bool va = ca < L, vb = cb < L;
  const centred<LAG> ops{x + (va ? ca : L - 1), x + (vb ? cb : L - 1), keep, L,
                         va ? centre[ca] : 0.0, vb ? centre[cb] : 0.0, diag};
  tile_loop(As, Bs, ops, n, va, vb, diag, n_tiles, part);
}

// The one tile of ga^T yb (SQUARE: ga^T (yb o yb)) for ga [n, na <= 64] and yb [n, nb <= 64], both fp64 and packed:
// element (i, j) = sum_t ga[t, i] yb[t, j].
template <bool SQUARE>
__device__ __forceinline__ void weighted_tile(double* As, double* Bs, const double* __restrict__ ga, int na,
                                              const double* __restrict__ yb, int nb, long n, int n_tiles,
                                              double* __restrict__ part) {
  const int cc = threadIdx.x & 63;
  const bool va = cc < na, vb = cc < nb;
  const weighted<SQUARE> ops{ga + (va ? cc : na - 1), yb + (vb ? cc : nb - 1), na, nb};
  tile_loop(As, Bs, ops, n, va, vb, false, n_tiles, part);
}

// The one tile of (a - ma)^T (b - mb) over the kept rows for a [n, na <= 64] and b [n, nb <= 64], both fp64 and packed, ma
// and mb their column means: element (i, j) = sum_t keep[t] (a[t, i] - ma[i]) (b[t, j] - mb[j]).
__device__ __forceinline__ void paired_tile(double* As, double* Bs, const double* __restrict__ a, int na,
                                            const double* __restrict__ ma, const double* __restrict__ b, int nb,
                                            const double* __restrict__ mb, const unsigned char* __restrict__ keep, long n,
                                            int n_tiles, double* __restrict__ part) {
  const int cc = threadIdx.x & 63;
  const bool va = cc < na, vb = cc < nb;
  const paired ops{a + (va ? cc : na - 1), b + (vb ? cc : nb - 1), keep, na, nb, va ? ma[cc] : 0.0, vb ? mb[cc] : 0.0};
  tile_loop(As, Bs, ops, n, va, vb, false, n_tiles, part);
}

// The one tile of a gated moment over the n pairs of r [n + 1, nr <= 64] under g [n + 1, ng <= 64], both fp64 and packed:
// GATED_CROSS, element (a, b) = sum_p fl(g[p + 1, col] r[p + 1, a]) keep[p] r[p, b]; the two squares, element (i, b) =
// sum_p g[p + 1, i] keep[p] fl(r[p + 1 or p, b]^2).
template <int FORM>
__device__ __forceinline__ void gated_tile(double* As, double* Bs, const double* __restrict__ g, int ng, int col,
                                           const double* __restrict__ r, int nr, const unsigned char* __restrict__ keep, long n,
                                           int n_tiles, double* __restrict__ part) {
  const int cc = threadIdx.x & 63;
  const bool va = cc < (FORM == GATED_CROSS ? nr : ng), vb = cc < nr;
  const int cr = vb ? cc : nr - 1;
  const gated<FORM> ops{g + (FORM == GATED_CROSS ? col : (va ? cc : ng - 1)), r + cr, r + cr, keep, ng, nr};
  tile_loop(As, Bs, ops, n, va, vb, false, n_tiles, part);
}

// Element (i, j) of the matrix: its partials in ascending range order from +0.  `tile` is the number of the element's
// tile within a range, of n_tiles.
__device__ __forceinline__ double range_sum(const double* __restrict__ part, long n_ranges, int n_tiles, int tile, int i,
                                            int j) {
  const long at = (long)tile * TILE + (i & 63) * MT + (j & 63);
  double acc = 0.0;
  for (long r = 0; r < n_ranges; ++r) acc += part[r * n_tiles * TILE + at];
  return acc;
}

// Grid (blocks of ROWS rows, tiles of THREADS columns): part[b, j] = term(t, j) over the rows [256 b, 256 b + 256) of
// column j, added in ascending t from +0.
template <class Term>
__device__ __forceinline__ void colsum_block(Term term, long T, long L, double* __restrict__ part) {
  const long j = (long)blockIdx.y * THREADS + threadIdx.x;
  if (j >= L) return;
  const long t0 = (long)blockIdx.x * ROWS, t1 = t0 + ROWS < T ? t0 + ROWS : T;
  double acc = 0.0;
  for (long t = t0; t < t1; ++t) acc += term(t, j);
  part[(long)blockIdx.x * L + j] = acc;
}

// The nb block sums of column j in ascending block order from +0
__device__ __forceinline__ double colsum_total(const double* __restrict__ part, long nb, long L, long j) {
  double acc = 0.0;
  long b = 0;
  for (; b + 8 <= nb; b += 8) {   // eight loads in flight, added in ascending order all the same
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = part[(b + i) * L + j];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += v[i];
  }
  for (; b < nb; ++b) acc += part[b * L + j];
  return acc;
}

}  // namespace mom
}  // namespace rv
