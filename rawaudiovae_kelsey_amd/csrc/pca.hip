// Latent PCA (rawaudiovae_kelsey_amd/pca.py): four ops of rv_mosaic.  The rules: include/rawvae_hip.h, "Latent PCA";
// the tiling, the error model and the measured figures: DESIGN.md section 7.10.
//   RV_PCA_MOMENTS   fp64 column means (k_pca_mean_block / k_pca_mean_sum, RV_EVAL_DIMS's order of adding) and the
//                    fp64 sample covariance: k_pca_cov, one workgroup per (range of 4096 rows, 64 x 64 tile on or
//                    above the diagonal) on v_mfma_f64_16x16x4_f64, then k_pca_cov_sum over the ranges.  No atomics.
//   RV_PCA_EIG       cyclic two-sided Jacobi in fp64: k_pca_eig, ONE workgroup, the matrix in global memory, a
//                    __syncthreads() between the steps; nothing waits on another workgroup.
//   RV_PCA_APPLY     projection, reconstruction and edits along the components: k_pca_apply, a tile of rows per
//                    workgroup, every dot product one fp64 fma chain.
//   RV_PCA_WORKSPACE the bytes of ws of the first two.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "internal.h"

using namespace rv;

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int PCA_LMAX = 512;
constexpr int MEAN_ROWS = 256;           // rows of one block of the mean (the header states it)
constexpr int MEAN_THREADS = 64;
constexpr int CV_RANGE = 4096;           // rows of one range of the covariance (the header states it)
constexpr int CV_CHUNK = 32;             // rows staged in LDS at a time
constexpr int CV_MT = 64;                // the workgroup's tile: 4 x 4 MFMA tiles of 16 x 16, one row of them per wave
constexpr int CV_LD = 80;                // LDS row pitch in doubles: rows k .. k + 3 of an operand fall into disjoint banks
constexpr int CV_THREADS = 256;
constexpr int EG_THREADS = 1024;
constexpr int EG_SWEEPS = 40;
constexpr int AP_THREADS = 256;
constexpr int AP_VC = 8;                 // columns of the component tile staged per step
constexpr int AP_VLD = AP_VC + 1;

// part[b, j] = rows [256 b, 256 b + 256) of column j added in ascending t from +0
__global__ void __launch_bounds__(MEAN_THREADS)
k_pca_mean_block(const float* __restrict__ x, long T, long L, double* __restrict__ part) {
  const long j = (long)blockIdx.y * MEAN_THREADS + threadIdx.x;
  if (j >= L) return;
  const long t0 = (long)blockIdx.x * MEAN_ROWS, t1 = t0 + MEAN_ROWS < T ? t0 + MEAN_ROWS : T;
  double acc = 0.0;
  for (long t = t0; t < t1; ++t) acc += (double)x[t * L + j];
  part[(long)blockIdx.x * L + j] = acc;
}

// centre[j] = (the block sums of column j in ascending block order from +0) / T
__global__ void __launch_bounds__(MEAN_THREADS)
k_pca_mean_sum(const double* __restrict__ part, long nb, long L, long T, double* __restrict__ centre) {
  const long j = (long)blockIdx.x * MEAN_THREADS + threadIdx.x;
  if (j >= L) return;
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
  centre[j] = acc / (double)T;
}

// number of the 64 x 64 tile (I, J >= I) among the tiles on or above the diagonal, row by row
__host__ __device__ __forceinline__ int tile_number(int I, int J, int nI) { return I * nI - I * (I - 1) / 2 + (J - I); }

// The thread's column of both operands at rows t, t + 4, ..; a row beyond the range is read from the range's last row
// (the caller stores a zero in its place).
template <int PER>
__device__ __forceinline__ void cov_fetch(const float* __restrict__ xa, const float* __restrict__ xb, long t, long t1, long L,
                                          bool diag, float (&fa)[PER], float (&fb)[PER]) {
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const long tt = t + 4 * i;
    const long tr = (tt < t1 ? tt : t1 - 1) * L;
    fa[i] = xa[tr];
    fb[i] = diag ? 0.f : xb[tr];
  }
}

// Grid (ranges, tiles on or above the diagonal).  Wave w owns the MFMA tiles (w, 0 .. 3) of the 64 x 64 tile; on a
// diagonal tile those left of the diagonal are skipped.  v_mfma_f64_16x16x4_f64: lane l holds A[i = l & 15][k = l >> 4]
// and B[k = l >> 4][j = l & 15]; with A[i][k] = d[t + k][i0 + i] and B[k][j] = d[t + k][j0 + j] one instruction adds
// four rows of d to the tile.  Its result: column l & 15, row (l >> 4) + 4 reg.
__global__ void __launch_bounds__(CV_THREADS)
k_pca_cov(const float* __restrict__ x, long T, int L, const double* __restrict__ centre, int nI, int n_tiles,
          double* __restrict__ part) {
  __shared__ double As[CV_CHUNK * CV_LD];
  __shared__ double Bs[CV_CHUNK * CV_LD];
  int I = 0, rem = (int)blockIdx.y;
  while (rem >= nI - I) {
    rem -= nI - I;
    ++I;
  }
  const int J = I + rem;
  const bool diag = I == J;
  const int lane = threadIdx.x & 63, ti = threadIdx.x >> 6;
  const double* const Bsrc = diag ? As : Bs;
  f64x4 acc[4];
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) acc[tj] = f64x4{0.0, 0.0, 0.0, 0.0};
  const long t0 = (long)blockIdx.x * CV_RANGE, t1 = t0 + CV_RANGE < T ? t0 + CV_RANGE : T;
  // Staging: thread (cc = lane, ti) carries column cc of both operands for the rows ti, ti + 4, .. of a chunk.  The
  // loads of the next chunk are issued before the MFMAs of this one; a row or column beyond the data is read from a
  // clamped address and replaced by zero on its way into LDS.
  constexpr int PER = CV_CHUNK / (CV_THREADS / CV_MT);   // rows per thread and chunk
  const int cc = lane;
  const int ca = I * CV_MT + cc, cb = J * CV_MT + cc;
  const bool va = ca < L, vb = cb < L;
  const double ma = va ? centre[ca] : 0.0, mb = vb ? centre[cb] : 0.0;
  const float* const xa = x + (va ? ca : L - 1);
  const float* const xb = x + (vb ? cb : L - 1);
  float fa[PER], fb[PER];
  cov_fetch<PER>(xa, xb, t0 + ti, t1, L, diag, fa, fb);
  for (long tc = t0; tc < t1; tc += CV_CHUNK) {
    __syncthreads();   // the MFMAs of the chunk before have read LDS
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int r = ti + 4 * i;
      const bool vt = tc + r < t1;
      As[r * CV_LD + cc] = (vt && va) ? (double)fa[i] - ma : 0.0;
      if (!diag) Bs[r * CV_LD + cc] = (vt && vb) ? (double)fb[i] - mb : 0.0;
    }
    __syncthreads();
    if (tc + CV_CHUNK < t1) cov_fetch<PER>(xa, xb, tc + CV_CHUNK + ti, t1, L, diag, fa, fb);
#pragma unroll
    for (int kk = 0; kk < CV_CHUNK; kk += 4) {
      const int row = (kk + (lane >> 4)) * CV_LD + (lane & 15);
      const double a = As[row + ti * 16];
#pragma unroll
      for (int tj = 0; tj < 4; ++tj) {
        if (diag && tj < ti) continue;   // wave-uniform
        const double b = Bsrc[row + tj * 16];
        acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[tj], 0, 0, 0);
      }
    }
  }
  double* const o = part + ((long)blockIdx.x * n_tiles + blockIdx.y) * (CV_MT * CV_MT);
#pragma unroll
  for (int tj = 0; tj < 4; ++tj) {
    if (diag && tj < ti) continue;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
      o[(ti * 16 + (lane >> 4) + 4 * reg) * CV_MT + tj * 16 + (lane & 15)] = acc[tj][reg];
  }
}

// Grid (tiles of 64 columns, rows): element (i, j >= i) = its partials in ascending range order from +0, over T - 1,
// written to [i, j] and [j, i].
__global__ void __launch_bounds__(64)
k_pca_cov_sum(const double* __restrict__ part, long n_ranges, int n_tiles, int nI, int L, long T, double* __restrict__ cov) {
  const int i = (int)blockIdx.y, j = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (j >= L || j < i) return;
  const long at = (long)tile_number(i >> 6, j >> 6, nI) * (CV_MT * CV_MT) + (i & 63) * CV_MT + (j & 63);
  double acc = 0.0;
  for (long r = 0; r < n_ranges; ++r) acc += part[r * n_tiles * (CV_MT * CV_MT) + at];
  const double v = acc / (double)(T - 1);
  cov[(long)i * L + j] = v;
  cov[(long)j * L + i] = v;
}

// Sum of one double per thread over the 1024 threads in a fixed order: the xor butterfly within a wave, then the 16
// wave sums in ascending wave order.  Valid in every thread.
__device__ __forceinline__ double eig_block_sum(double v, double* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();   // red may still be read from the call before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < EG_THREADS / 64; ++w) s += red[w];
  return s;
}

// A 2 x 2 block x[a][b] whose axis 0 carries the pair of the lower pair number: that pair's rotation (c0, s0) along
// axis 0 first, then the other's (c1, s1) along axis 1.  Blocks (k, m) and (m, k) of a symmetric matrix run this on
// the same four values, so the matrix stays bitwise symmetric.
__device__ __forceinline__ void rotate_block(double c0, double s0, double c1, double s1, double& x00, double& x01,
                                             double& x10, double& x11) {
#pragma clang fp contract(off)
  const double r00 = __builtin_fma(c0, x00, -(s0 * x10)), r01 = __builtin_fma(c0, x01, -(s0 * x11));
  const double r10 = __builtin_fma(s0, x00, c0 * x10), r11 = __builtin_fma(s0, x01, c0 * x11);
  x00 = __builtin_fma(c1, r00, -(s1 * r01));
  x01 = __builtin_fma(s1, r00, c1 * r01);
  x10 = __builtin_fma(c1, r10, -(s1 * r11));
  x11 = __builtin_fma(s1, r10, c1 * r11);
}

// ONE workgroup.  A [L, L] symmetric, rotated in place and overwritten by the eigenvectors (rows) at the end;
// Vt [L, L] scratch, the transposed product of the rotations.  Every loop bound is an argument or a constant, and no
// thread waits for anything but the workgroup's own barrier.
__global__ void __launch_bounds__(EG_THREADS)
k_pca_eig(double* A, int L, double* Vt, double* lam_out, int* info) {
  __shared__ double red[EG_THREADS / 64];
  __shared__ double sc[PCA_LMAX / 2], ss[PCA_LMAX / 2], spp[PCA_LMAX / 2], sqq[PCA_LMAX / 2];
  __shared__ int sp[PCA_LMAX / 2], sq[PCA_LMAX / 2];
  __shared__ double slam[PCA_LMAX], ssign[PCA_LMAX];
  __shared__ int srank[PCA_LMAX];
  const int tid = threadIdx.x;
  const int n = (L + 1) & ~1, h = n >> 1;
  const long LL = (long)L * L;

  double part = 0.0;
  for (long e = tid; e < LL; e += EG_THREADS) {
    const double a = A[e];
    part = __builtin_fma(a, a, part);
    Vt[e] = (e / L == e % L) ? 1.0 : 0.0;
  }
  const double thr = (double)L * 0x1p-52 * sqrt(eig_block_sum(part, red));

  int sweeps = 0, converged = 0;
  for (int sweep = 0; sweep <= EG_SWEEPS; ++sweep) {
    part = 0.0;
    for (long e = tid; e < LL; e += EG_THREADS) {
      const double a = A[e];
      if (e / L != e % L) part = __builtin_fma(a, a, part);
    }
    const double off = sqrt(eig_block_sum(part, red));   // the same bits in every thread
    if (off <= thr) {
      converged = 1;
      break;
    }
    if (sweep == EG_SWEEPS) break;
    for (int s = 0; s < n - 1; ++s) {
      if (tid < h) {
        int a = tid == 0 ? n - 1 : (s + tid) % (n - 1);
        int b = tid == 0 ? s : (s - tid + (n - 1)) % (n - 1);
        const int p = a < b ? a : b, q = a < b ? b : a;
        double c = 1.0, sn = 0.0, npp = 0.0, nqq = 0.0;
        if (q < L) {
          const double app = A[(long)p * L + p], aqq = A[(long)q * L + q], apq = A[(long)p * L + q];
          npp = app;
          nqq = aqq;
          if (apq != 0.0) {
            const double theta = (aqq - app) / (2.0 * apq);
            const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            c = 1.0 / sqrt(t * t + 1.0);
            sn = t * c;
            npp = app - t * apq;
            nqq = aqq + t * apq;
          }
        } else if (p < L) {
          npp = A[(long)p * L + p];
        }
        sp[tid] = p;
        sq[tid] = q;
        sc[tid] = c;
        ss[tid] = sn;
        spp[tid] = npp;
        sqq[tid] = nqq;
      }
      __syncthreads();
      for (int b = tid; b < h * h; b += EG_THREADS) {
        const int k = b / h, m = b - k * h;
        const int pk = sp[k], qk = sq[k], pm = sp[m], qm = sq[m];
        const bool vk = qk < L, vm = qm < L;   // only a pair's larger index can be the padding index
        if (k == m) {
          if (pk < L) A[(long)pk * L + pk] = spp[k];
          if (vk) {
            A[(long)qk * L + qk] = sqq[k];
            A[(long)pk * L + qk] = 0.0;
            A[(long)qk * L + pk] = 0.0;
          }
          continue;
        }
        if (pk >= L || pm >= L) continue;
        double* const a00 = A + (long)pk * L + pm;
        double* const a01 = A + (long)pk * L + qm;
        double* const a10 = A + (long)qk * L + pm;
        double* const a11 = A + (long)qk * L + qm;
        double x00 = *a00, x01 = vm ? *a01 : 0.0, x10 = vk ? *a10 : 0.0, x11 = (vk && vm) ? *a11 : 0.0;
        if (k < m) rotate_block(sc[k], ss[k], sc[m], ss[m], x00, x01, x10, x11);
        else rotate_block(sc[m], ss[m], sc[k], ss[k], x00, x10, x01, x11);
        *a00 = x00;
        if (vm) *a01 = x01;
        if (vk) *a10 = x10;
        if (vk && vm) *a11 = x11;
      }
      for (int e = tid; e < h * L; e += EG_THREADS) {
        const int k = e / L, col = e - k * L;
        const int p = sp[k], q = sq[k];
        if (q >= L) continue;
        const double c = sc[k], sn = ss[k];
        const double vp = Vt[(long)p * L + col], vq = Vt[(long)q * L + col];
        Vt[(long)p * L + col] = c * vp - sn * vq;
        Vt[(long)q * L + col] = sn * vp + c * vq;
      }
      __syncthreads();
    }
    sweeps = sweep + 1;
  }

  // eigenvalues in descending order (equal values: the lower index first), the sign rule, the rows out
  for (int i = tid; i < L; i += EG_THREADS) slam[i] = A[(long)i * L + i];
  __syncthreads();
  for (int j = tid; j < L; j += EG_THREADS) {
    const double lj = slam[j];
    int rank = 0;
    for (int i = 0; i < L; ++i) rank += (slam[i] > lj || (slam[i] == lj && i < j)) ? 1 : 0;
    srank[j] = rank;
    double best = -1.0, sign = 1.0;
    for (int l = 0; l < L; ++l) {
      const double v = Vt[(long)j * L + l];
      if (fabs(v) > best) {
        best = fabs(v);
        sign = v < 0.0 ? -1.0 : 1.0;
      }
    }
    ssign[j] = sign;
    lam_out[rank] = lj;
  }
  __syncthreads();
  for (long e = tid; e < LL; e += EG_THREADS) {
    const int j = (int)(e / L), l = (int)(e - (long)j * L);
    A[(long)srank[j] * L + l] = ssign[j] * Vt[e];
  }
  if (tid == 0) {
    info[0] = sweeps;
    info[1] = converged;
  }
}

// One workgroup per RT rows.  LDS: d [RT, L] (x - centre), y [RT, k] (the coordinates, then the coefficients of the
// components), vt [256, AP_VC (+1)] (a tile of the components, so that thread j reads row j without a strided global
// load).  Pass 1: thread j owns coordinate j of every row, one chain over l.  Pass 2: thread l owns column l of every
// row, one chain over j, the components read along their rows.
template <int RT>
__global__ void __launch_bounds__(AP_THREADS)
k_pca_apply(int mode, const float* __restrict__ q, long T, int L, int k, const double* __restrict__ centre,
            const double* __restrict__ basis, const double* __restrict__ lam, const float* __restrict__ gains,
            const float* __restrict__ shifts, float* __restrict__ out, long ldo) {
  extern __shared__ double sm[];
  double* const d = sm;
  double* const y = d + RT * L;
  double* const vt = y + RT * k;
  const int tid = threadIdx.x;
  const long t0 = (long)blockIdx.x * RT;
  const int nr = T - t0 < RT ? (int)(T - t0) : RT;
  if (mode != RV_PCA_RECONSTRUCT) {
    for (int e = tid; e < RT * L; e += AP_THREADS) {
      const int r = e / L, l = e - r * L;
      d[e] = r < nr ? (double)q[(t0 + r) * L + l] - centre[l] : 0.0;
    }
    for (int jb = 0; jb < k; jb += AP_THREADS) {
      double acc[RT];
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[r] = 0.0;
      for (int l0 = 0; l0 < L; l0 += AP_VC) {
        __syncthreads();   // d is written; the tile of the step before is read
        for (int e = tid; e < AP_THREADS * AP_VC; e += AP_THREADS) {
          const int jr = e / AP_VC, lc = e - jr * AP_VC;
          const int j = jb + jr, l = l0 + lc;
          vt[jr * AP_VLD + lc] = (j < k && l < L) ? basis[(long)j * L + l] : 0.0;
        }
        __syncthreads();
        const int lim = L - l0 < AP_VC ? L - l0 : AP_VC;
        for (int lc = 0; lc < lim; ++lc) {
          const double v = vt[tid * AP_VLD + lc];
#pragma unroll
          for (int r = 0; r < RT; ++r) acc[r] = __builtin_fma(d[r * L + l0 + lc], v, acc[r]);
        }
      }
      const int j = jb + tid;
      if (j < k) {
        if (mode == RV_PCA_PROJECT) {
#pragma unroll
          for (int r = 0; r < RT; ++r)
            if (r < nr) out[(t0 + r) * ldo + j] = (float)acc[r];
        } else {
          const double g1 = (double)gains[j] - 1.0, hs = (double)shifts[j] * sqrt(fmax(lam[j], 0.0));
#pragma unroll
          for (int r = 0; r < RT; ++r) y[r * k + j] = __builtin_fma(g1, acc[r], hs);
        }
      }
    }
    if (mode == RV_PCA_PROJECT) return;
  } else {
    for (int e = tid; e < RT * k; e += AP_THREADS) {
      const int r = e / k, j = e - r * k;
      y[e] = r < nr ? (double)q[(t0 + r) * k + j] : 0.0;
    }
  }
  __syncthreads();
  for (int l = tid; l < L; l += AP_THREADS) {
    double acc[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) acc[r] = 0.0;
    for (int j = 0; j < k; ++j) {
      const double v = basis[(long)j * L + l];
#pragma unroll
      for (int r = 0; r < RT; ++r) acc[r] = __builtin_fma(y[r * k + j], v, acc[r]);
    }
    if (mode == RV_PCA_EDIT) {
#pragma unroll
      for (int r = 0; r < RT; ++r) {
        if (r >= nr) continue;
        const float xv = q[(t0 + r) * L + l];
        out[(t0 + r) * ldo + l] = acc[r] == 0.0 ? xv : (float)((double)xv + acc[r]);
      }
    } else {
      const double c = centre[l];
#pragma unroll
      for (int r = 0; r < RT; ++r)
        if (r < nr) out[(t0 + r) * ldo + l] = (float)(c + acc[r]);
    }
  }
}

struct moments_ws {
  long nb, n_ranges, mean_doubles, bytes;
  int nI, n_tiles;
};

moments_ws moments_layout(long T, long L) {
  moments_ws w;
  w.nb = (T + MEAN_ROWS - 1) / MEAN_ROWS;
  w.n_ranges = (T + CV_RANGE - 1) / CV_RANGE;
  w.nI = (int)((L + CV_MT - 1) / CV_MT);
  w.n_tiles = w.nI * (w.nI + 1) / 2;
  w.mean_doubles = w.nb * L;
  w.bytes = (w.mean_doubles + w.n_ranges * w.n_tiles * (long)(CV_MT * CV_MT)) * (long)sizeof(double);
  return w;
}

long eig_bytes(long L) { return L * L * (long)sizeof(double); }

}  // namespace

int rv_pca_workspace(rv_mosaic_desc* d) {
  RV_REQUIRE(d->T == 0 || (d->T >= 2 && d->T < (1L << 31)), RV_ERR_SHAPE,
             "rv_mosaic(PCA_WORKSPACE): T=%ld must be 0 (RV_PCA_EIG only) or in [2, 2^31)", d->T);
  RV_REQUIRE(d->L >= 1 && d->L <= PCA_LMAX, RV_ERR_SHAPE, "rv_mosaic(PCA_WORKSPACE): L=%ld outside [1, %d]", d->L, PCA_LMAX);
  long need = eig_bytes(d->L);
  if (d->T >= 2) {
    const long m = moments_layout(d->T, d->L).bytes;
    need = m > need ? m : need;
  }
  d->ws_bytes = need;
  return RV_OK;
}

int rv_pca_moments(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->T >= 2 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(PCA_MOMENTS): T=%ld outside [2, 2^31)", d->T);
  RV_REQUIRE(d->L >= 1 && d->L <= PCA_LMAX, RV_ERR_SHAPE, "rv_mosaic(PCA_MOMENTS): L=%ld outside [1, %d]", d->L, PCA_LMAX);
  RV_REQUIRE(d->q, RV_ERR_NULL, "rv_mosaic(PCA_MOMENTS): q is null");
  RV_REQUIRE(d->centre, RV_ERR_NULL, "rv_mosaic(PCA_MOMENTS): centre is null");
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(PCA_MOMENTS): basis is null");
  const moments_ws w = moments_layout(d->T, d->L);
  RV_REQUIRE(d->ws_bytes >= w.bytes, RV_ERR_SHAPE, "rv_mosaic(PCA_MOMENTS): ws_bytes=%ld, T=%ld rows of L=%ld need %ld",
             d->ws_bytes, d->T, d->L, w.bytes);
  RV_REQUIRE(d->ws, RV_ERR_NULL, "rv_mosaic(PCA_MOMENTS): ws is null, T=%ld rows of L=%ld need %ld bytes", d->T, d->L, w.bytes);
  const hipStream_t st = (hipStream_t)stream;
  const int L = (int)d->L;
  double* const mean_part = (double*)d->ws;
  double* const cov_part = mean_part + w.mean_doubles;
  const unsigned col_tiles = (unsigned)((L + MEAN_THREADS - 1) / MEAN_THREADS);
  hipLaunchKernelGGL(k_pca_mean_block, dim3((unsigned)w.nb, col_tiles), dim3(MEAN_THREADS), 0, st, d->q, d->T, d->L, mean_part);
  hipLaunchKernelGGL(k_pca_mean_sum, dim3(col_tiles), dim3(MEAN_THREADS), 0, st, (const double*)mean_part, w.nb, d->L, d->T,
                     d->centre);
  hipLaunchKernelGGL(k_pca_cov, dim3((unsigned)w.n_ranges, (unsigned)w.n_tiles), dim3(CV_THREADS), 0, st, d->q, d->T, L,
                     d->centre, w.nI, w.n_tiles, cov_part);
  hipLaunchKernelGGL(k_pca_cov_sum, dim3((unsigned)((L + 63) / 64), (unsigned)L), dim3(64), 0, st, (const double*)cov_part,
                     w.n_ranges, w.n_tiles, w.nI, L, d->T, d->basis);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_pca_eig(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->L >= 1 && d->L <= PCA_LMAX, RV_ERR_SHAPE, "rv_mosaic(PCA_EIG): L=%ld outside [1, %d]", d->L, PCA_LMAX);
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(PCA_EIG): basis is null");
  RV_REQUIRE(d->eigenvalues, RV_ERR_NULL, "rv_mosaic(PCA_EIG): the eigenvalues are null");
  RV_REQUIRE(d->info, RV_ERR_NULL, "rv_mosaic(PCA_EIG): info is null");
  const long need = eig_bytes(d->L);
  RV_REQUIRE(d->ws_bytes >= need, RV_ERR_SHAPE, "rv_mosaic(PCA_EIG): ws_bytes=%ld, L=%ld needs %ld", d->ws_bytes, d->L, need);
  RV_REQUIRE(d->ws, RV_ERR_NULL, "rv_mosaic(PCA_EIG): ws is null, L=%ld needs %ld bytes", d->L, need);
  hipLaunchKernelGGL(k_pca_eig, dim3(1), dim3(EG_THREADS), 0, (hipStream_t)stream, d->basis, (int)d->L, (double*)d->ws,
                     d->eigenvalues, d->info);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_pca_apply(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->mode == RV_PCA_PROJECT || d->mode == RV_PCA_RECONSTRUCT || d->mode == RV_PCA_EDIT, RV_ERR_SHAPE,
             "rv_mosaic(PCA_APPLY): mode=%ld is none of RV_PCA_PROJECT, RV_PCA_RECONSTRUCT, RV_PCA_EDIT", d->mode);
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(PCA_APPLY): T=%ld outside [1, 2^31)", d->T);
  RV_REQUIRE(d->L >= 1 && d->L <= PCA_LMAX, RV_ERR_SHAPE, "rv_mosaic(PCA_APPLY): L=%ld outside [1, %d]", d->L, PCA_LMAX);
  RV_REQUIRE(d->k >= 1 && d->k <= d->L, RV_ERR_SHAPE, "rv_mosaic(PCA_APPLY): k=%ld outside [1, L=%ld]", d->k, d->L);
  RV_REQUIRE(d->q, RV_ERR_NULL, "rv_mosaic(PCA_APPLY): q is null");
  RV_REQUIRE(d->out, RV_ERR_NULL, "rv_mosaic(PCA_APPLY): out is null");
  RV_REQUIRE(d->centre, RV_ERR_NULL, "rv_mosaic(PCA_APPLY): centre is null");
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(PCA_APPLY): basis is null");
  const long width = d->mode == RV_PCA_PROJECT ? d->k : d->L;
  RV_REQUIRE(d->ldo >= width, RV_ERR_SHAPE, "rv_mosaic(PCA_APPLY): ldo=%ld holds no row of %ld values", d->ldo, width);
  if (d->mode == RV_PCA_EDIT) {
    RV_REQUIRE(d->eigenvalues, RV_ERR_NULL, "rv_mosaic(PCA_APPLY): the eigenvalues are null");
    RV_REQUIRE(d->gains, RV_ERR_NULL, "rv_mosaic(PCA_APPLY): the gains are null");
    RV_REQUIRE(d->shifts, RV_ERR_NULL, "rv_mosaic(PCA_APPLY): the shifts are null");
  }
  const hipStream_t st = (hipStream_t)stream;
  const int L = (int)d->L, k = (int)d->k;
  if (L <= 256) {   // k <= L
    constexpr int RT = 8;
    const size_t lds = ((size_t)RT * (L + k) + AP_THREADS * AP_VLD) * sizeof(double);
    hipLaunchKernelGGL(k_pca_apply<RT>, dim3((unsigned)((d->T + RT - 1) / RT)), dim3(AP_THREADS), lds, st, (int)d->mode, d->q,
                       d->T, L, k, d->centre, d->basis, d->eigenvalues, d->gains, d->shifts, d->out, d->ldo);
  } else {
    constexpr int RT = 4;
    const size_t lds = ((size_t)RT * (L + k) + AP_THREADS * AP_VLD) * sizeof(double);
    hipLaunchKernelGGL(k_pca_apply<RT>, dim3((unsigned)((d->T + RT - 1) / RT)), dim3(AP_THREADS), lds, st, (int)d->mode, d->q,
                       d->T, L, k, d->centre, d->basis, d->eigenvalues, d->gains, d->shifts, d->out, d->ldo);
  }
  RV_CHECK_LAUNCH();
  return RV_OK;
}
