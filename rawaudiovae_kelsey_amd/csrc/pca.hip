// Latent PCA (rawaudiovae_kelsey_amd/pca.py): four ops of rv_mosaic.  The rules: include/rawvae_hip.h, "Latent PCA";
// the tiling, the error model and the measured figures: DESIGN.md section 7.10.
//   RV_PCA_MOMENTS   fp64 column means (k_pca_mean_block / k_pca_mean_sum, moment.h's blocked column sum) and the
//                    fp64 sample covariance: k_pca_cov, one workgroup per (range of 4096 rows, 64 x 64 tile on or
//                    above the diagonal) on moment.h's MFMA tile, then k_pca_cov_sum over the ranges.  No atomics.
//   RV_PCA_EIG       cyclic two-sided Jacobi in fp64: k_pca_eig, ONE workgroup, the matrix in global memory, a
//                    __syncthreads() between the steps; nothing waits on another workgroup.
//   RV_PCA_APPLY     projection, reconstruction and edits along the components: k_pca_apply, a tile of rows per
//                    workgroup, every dot product one fp64 fma chain.
//   RV_PCA_WORKSPACE the bytes of ws of the first two.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "internal.h"
#include "moment.h"

using namespace rv;

namespace {

constexpr int PCA_LMAX = 512;
constexpr int EG_THREADS = 1024;
constexpr int EG_SWEEPS = 40;
constexpr int AP_THREADS = 256;
constexpr int AP_VC = 8;                 // columns of the component tile staged per step
constexpr int AP_VLD = AP_VC + 1;

// part[b, j] = rows [256 b, 256 b + 256) of column j added in ascending t from +0
__global__ void __launch_bounds__(mom::THREADS)
k_pca_mean_block(const float* __restrict__ x, long T, long L, double* __restrict__ part) {
  mom::colsum_block([=](long t, long j) { return (double)x[t * L + j]; }, T, L, part);
}

// centre[j] = (the block sums of column j in ascending block order from +0) / T
__global__ void __launch_bounds__(mom::THREADS)
k_pca_mean_sum(const double* __restrict__ part, long nb, long L, long T, double* __restrict__ centre) {
  const long j = (long)blockIdx.x * mom::THREADS + threadIdx.x;
  if (j >= L) return;
  centre[j] = mom::colsum_total(part, nb, L, j) / (double)T;
}

// Grid (ranges, tiles on or above the diagonal): moment.h's tile in its symmetric form, A[i][k] = d[t + k][i0 + i]
// and B[k][j] = d[t + k][j0 + j].
__global__ void __launch_bounds__(mom::TILE_THREADS)
k_pca_cov(const float* __restrict__ x, long T, int L, const double* __restrict__ centre, int nI, int n_tiles,
          double* __restrict__ part) {
  __shared__ double As[mom::STAGE];
  __shared__ double Bs[mom::STAGE];
  int I = 0, rem = (int)blockIdx.y;
  while (rem >= nI - I) {
    rem -= nI - I;
    ++I;
  }
  mom::moment_tile<false>(As, Bs, x, T, L, centre, nullptr, I, I + rem, n_tiles, part);
}

// Grid (tiles of 64 columns, rows): element (i, j >= i) = its partials in ascending range order from +0, over T - 1,
// written to [i, j] and [j, i].
__global__ void __launch_bounds__(64)
k_pca_cov_sum(const double* __restrict__ part, long n_ranges, int n_tiles, int nI, int L, long T, double* __restrict__ cov) {
  const int i = (int)blockIdx.y, j = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (j >= L || j < i) return;
  const double acc = mom::range_sum(part, n_ranges, n_tiles, mom::tile_number(i >> 6, j >> 6, nI), i, j);
  const double v = acc / (double)(T - 1);
  cov[(long)i * L + j] = v;
  cov[(long)j * L + i] = v;
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
  const double thr = (double)L * 0x1p-52 * sqrt(block_sum_f64<EG_THREADS / 64>(part, red));

  int sweeps = 0, converged = 0;
  for (int sweep = 0; sweep <= EG_SWEEPS; ++sweep) {
    part = 0.0;
    for (long e = tid; e < LL; e += EG_THREADS) {
      const double a = A[e];
      if (e / L != e % L) part = __builtin_fma(a, a, part);
    }
    const double off = sqrt(block_sum_f64<EG_THREADS / 64>(part, red));   // the same bits in every thread
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
  long nb, mean_doubles, bytes;
  mom::tiles cov;
};

moments_ws moments_layout(long T, long L) {
  moments_ws w;
  w.nb = (T + mom::ROWS - 1) / mom::ROWS;
  w.mean_doubles = w.nb * L;
  w.cov = mom::tile_layout(T, L, false);
  w.bytes = (w.mean_doubles + w.cov.doubles) * (long)sizeof(double);
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
  const unsigned col_tiles = (unsigned)((L + mom::THREADS - 1) / mom::THREADS);
  hipLaunchKernelGGL(k_pca_mean_block, dim3((unsigned)w.nb, col_tiles), dim3(mom::THREADS), 0, st, d->q, d->T, d->L, mean_part);
  hipLaunchKernelGGL(k_pca_mean_sum, dim3(col_tiles), dim3(mom::THREADS), 0, st, (const double*)mean_part, w.nb, d->L, d->T,
                     d->centre);
  hipLaunchKernelGGL(k_pca_cov, dim3((unsigned)w.cov.n_ranges, (unsigned)w.cov.n_tiles), dim3(mom::TILE_THREADS), 0, st, d->q,
                     d->T, L, d->centre, w.cov.nI, w.cov.n_tiles, cov_part);
  hipLaunchKernelGGL(k_pca_cov_sum, dim3((unsigned)((L + 63) / 64), (unsigned)L), dim3(64), 0, st, (const double*)cov_part,
                     w.cov.n_ranges, w.cov.n_tiles, w.cov.nI, L, d->T, d->basis);
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
