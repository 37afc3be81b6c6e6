// Latent attributes (rawaudiovae_kelsey_amd/attributes.py): audio descriptors of every frame of a waveform and the
// regression of per-frame targets on the whitened latents of a corpus.  Three ops of rv_mosaic; the rules, down to the
// order of every sum: include/rawvae_hip.h, "Latent attributes"; the LDS layout, the launch list and the measured
// figures: DESIGN.md section 7.17.
//   RV_ATTR_DESCRIBE   k_attr_describe, one workgroup of 256 threads per frame: level, zero-crossing rate and crest from
//                      the samples, centroid and flatness from spectrum.h's power spectrum in LDS; all sums in fp64.
//   RV_ATTR_FIT        k_attr_observe (y = P (x - c), the targets and the observed flags to ws: sequence.h's staging),
//                      k_attr_colsum and k_attr_means (moment.h's blocked column sum: n and the means), k_attr_moments
//                      (moment.h's MFMA tile on two centred fp64 operands: Yc^T Yc, Dc^T Yc and Dc^T Dc, a workgroup
//                      per range of 4096 frames and product), k_attr_close (ONE workgroup: the range sums, the Cholesky
//                      factor of Cyy + lam I in LDS, a wave per target for the two triangular solves and r2).
//   RV_ATTR_WORKSPACE  the bytes of ws.
// No atomics, no polling; every output element is written by exactly one thread.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"
#include "internal.h"
#include "moment.h"
#include "sequence.h"
#include "spectrum.h"

using namespace rv;

namespace {

constexpr int AT_THREADS = spec::THREADS;
constexpr int AT_KMAX = 64;       // axes: one 64 x 64 tile holds Cyy, one wave a vector over the axes
constexpr int AT_NMAX = 64;       // targets: one tile holds Cdy and Cdd
constexpr int AT_LMAX = 512;
constexpr int AT_PITCH = AT_KMAX + 1;
constexpr double AT_PIVOT = 0x1p-40;   // a pivot counts as positive above this share of its diagonal element (the header states it)

// One workgroup per frame t, x = xs + t * hop.  Thread u takes the terms u, u + 256, .. of every sum in ascending order
// from +0 in fp64, then block_sum_f64.  SPEC: zr = the N + 1 powers after spectrum.h's transform of fl(w x), N = S / 2.
template <bool SPEC>
__global__ void __launch_bounds__(AT_THREADS)
k_attr_describe(const float* __restrict__ xs, long hop, int S, const float* __restrict__ win, const float* __restrict__ tw,
                float floor_scale, double* __restrict__ out, long ldo) {
  extern __shared__ float lds[];   // SPEC: 2 N + 1 floats, sized by the launch; none otherwise
  __shared__ double red[AT_THREADS / 64];
  __shared__ float redf[AT_THREADS / 64];
  const long t = blockIdx.x;
  const float* x = xs + t * hop;
  const int N = S >> 1;
  const int lg = spec::stages(N);
  float* const zr = lds;            // N + 1
  float* const zi = zr + N + 1;     // N

  double en = 0.0, cross = 0.0;
  float peak = 0.f;
  for (int n = threadIdx.x; n < S; n += AT_THREADS) {
    const float xv = x[n];
    en += (double)xv * (double)xv;
    peak = fmaxf(peak, fabsf(xv));
    if (n >= 1 && (xv < 0.f) != (x[n - 1] < 0.f)) cross += 1.0;
    if constexpr (SPEC) spec::put(zr, zi, n, lg, win[n] * xv);
  }
  en = block_sum_f64<AT_THREADS / 64>(en, red);
  cross = block_sum_f64<AT_THREADS / 64>(cross, red);   // a count: exact
  peak = spec::block_max_f32(peak, redf);
  const double e = en / (double)S;
  double centroid = 0.0, flatness = 0.0;
  if constexpr (SPEC) {
    float pmax = 0.f;
    bool bad = false;
    spec::powers(zr, zi, tw, N, pmax, bad);
    pmax = spec::block_max_f32(pmax, redf);
    const int nbad = __syncthreads_or(bad);
    const float fl = pmax * floor_scale;
    double num = 0.0, den = 0.0, sa = 0.0, sl = 0.0;
    for (int k = threadIdx.x; k <= N; k += AT_THREADS) {
      const float pa = zr[k];
      num += (double)k * (double)pa;
      den += (double)pa;
      if (k >= 1) {
        sa += (double)pa;
        sl += log((double)(pa + fl));
      }
    }
    num = block_sum_f64<AT_THREADS / 64>(num, red);
    den = block_sum_f64<AT_THREADS / 64>(den, red);
    sa = block_sum_f64<AT_THREADS / 64>(sa, red);
    sl = block_sum_f64<AT_THREADS / 64>(sl, red);
    const double A = sa / (double)N, G = exp(sl / (double)N);
    centroid = den == 0.0 ? __builtin_nan("") : num / den / (double)S;
    flatness = A == 0.0 ? __builtin_nan("") : 10.0 * log10(G / A);
    if (nbad) centroid = flatness = __builtin_nan("");
  }
  if (threadIdx.x == 0) {
    double* o = out + t * ldo;
    const double p = (double)peak;
    o[0] = 10.0 * log10(e);
    o[1] = S > 1 ? cross / (double)(S - 1) : 0.0;
    o[2] = e == 0.0 ? __builtin_nan("") : 10.0 * log10(p * p / e);
    if constexpr (SPEC) {
      o[3] = centroid;
      o[4] = flatness;
    }
  }
}

// y [T, k], the targets [T, N] and obs [T] to ws.  obs = 1: the frame's x row and its D row are finite throughout; any
// other frame's y and targets are written as +0.
__global__ void __launch_bounds__(seq::THREADS)
k_attr_observe(const float* __restrict__ x, long ldx, const double* __restrict__ centre, const double* __restrict__ P,
               const double* __restrict__ D, long T, int L, int k, int N, double* __restrict__ ys, double* __restrict__ ds,
               unsigned char* __restrict__ obs) {
  __shared__ double sy[seq::FRAMES * seq::PITCH];
  __shared__ unsigned char sflag[seq::THREADS], sbad[seq::FRAMES];
  const int tid = threadIdx.x;
  const long t0 = (long)blockIdx.x * seq::FRAMES;
  const int nf = T - t0 < seq::FRAMES ? (int)(T - t0) : seq::FRAMES;
  seq::stage_frames(x, ldx, centre, P, t0, nf, L, k, sy, sflag, sbad);
  {
    const int f = tid >> 2, q = tid & 3;
    bool bad = false;
    if (f < nf) {
      const double* const dr = D + (t0 + f) * N;
      for (int j = q; j < N; j += 4) bad |= !(fabs(dr[j]) <= DBL_MAX);
    }
    sflag[tid] = bad;
  }
  __syncthreads();
  if (tid < seq::FRAMES) sbad[tid] |= sflag[4 * tid] | sflag[4 * tid + 1] | sflag[4 * tid + 2] | sflag[4 * tid + 3];
  __syncthreads();
  for (int e = tid; e < nf * k; e += seq::THREADS) {
    const int f = e / k, j = e - f * k;
    ys[t0 * k + e] = sbad[f] ? 0.0 : sy[f * seq::PITCH + j];
  }
  for (int e = tid; e < nf * N; e += seq::THREADS) ds[t0 * N + e] = sbad[e / N] ? 0.0 : D[t0 * N + e];
  if (tid < nf) obs[t0 + tid] = !sbad[tid];
}

// Column 0: the observed flags; 1 .. k: y; k + 1 .. k + N: the targets (both +0 in an unobserved frame already)
__global__ void __launch_bounds__(mom::THREADS)
k_attr_colsum(const double* __restrict__ ys, const double* __restrict__ ds, const unsigned char* __restrict__ obs, long T, long k,
              long N, double* __restrict__ part) {
  mom::colsum_block(
      [=](long t, long j) { return j == 0 ? (double)obs[t] : j <= k ? ys[t * k + j - 1] : ds[t * N + j - 1 - k]; }, T,
      1 + k + N, part);
}

// head = [ n | ybar (k) | dbar (N) ]: the block sums in ascending block order from +0, one division by n
__global__ void __launch_bounds__(AT_THREADS)
k_attr_means(const double* __restrict__ part, long nb, long cols, double* __restrict__ head) {
  const long j = threadIdx.x;
  if (j >= cols) return;
  const double n = mom::colsum_total(part, nb, cols, 0);
  head[j] = j == 0 ? n : mom::colsum_total(part, nb, cols, j) / n;
}

// Grid (ranges, 3): tile 0 of a range is Yc^T Yc, tile 1 Dc^T Yc, tile 2 Dc^T Dc
__global__ void __launch_bounds__(mom::TILE_THREADS)
k_attr_moments(const double* __restrict__ ys, int k, const double* __restrict__ ds, int N, const unsigned char* __restrict__ obs,
               const double* __restrict__ head, long T, double* __restrict__ part) {
  __shared__ double As[mom::STAGE];
  __shared__ double Bs[mom::STAGE];
  const double* const ybar = head + 1;
  const double* const dbar = head + 1 + k;
  if (blockIdx.y == 0) mom::paired_tile(As, Bs, ys, k, ybar, ys, k, ybar, obs, T, 3, part);
  else if (blockIdx.y == 1) mom::paired_tile(As, Bs, ds, N, dbar, ys, k, ybar, obs, T, 3, part);
  else mom::paired_tile(As, Bs, ds, N, dbar, ds, N, dbar, obs, T, 3, part);
}

// sum over the wave's 64 lanes by the xor butterfly: every lane ends with the same bits
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ONE workgroup.  sG: above and on the diagonal Cyy (element (i, j), i <= j, at sG[i * AT_PITCH + j]), below it the
// Cholesky factor R of G = Cyy + lam I (R[i][p], p < i, at sG[i * AT_PITCH + p]); sd: R's diagonal.
// result = [ n | ybar (k) | dbar (N) | Cdd (N N) | B (N k) | r2 (N) ]; the head was written by k_attr_means.
__global__ void __launch_bounds__(AT_THREADS)
k_attr_close(const double* __restrict__ part, long n_ranges, int k, int N, double lam, double* __restrict__ result,
             int* __restrict__ info) {
  __shared__ double sG[AT_KMAX * AT_PITCH];
  __shared__ double sd[AT_KMAX];
  __shared__ double scol[AT_KMAX];
  __shared__ int sfail;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const double n = result[0];
  const double dof = n - 1.0;
  double* const Cdd = result + 1 + k + N;
  double* const B = Cdd + (long)N * N;
  double* const r2 = B + (long)N * k;
  if (tid == 0) sfail = 0;
  for (int e = tid; e < k * k; e += AT_THREADS) {
    const int i = e / k, j = e - i * k;
    if (i <= j) sG[i * AT_PITCH + j] = mom::range_sum(part, n_ranges, 3, 0, i, j) / dof;
  }
  for (int e = tid; e < N * N; e += AT_THREADS) Cdd[e] = mom::range_sum(part, n_ranges, 3, 2, e / N, e % N) / dof;
  __syncthreads();
  int status = n < (double)(k + 2) ? 1 : 0;   // (uniform: every thread read the same n)
  // left-looking Cholesky, a column at a time: s = G[i][j] - sum_p R[i][p] R[j][p] in ascending p, one fma each
  for (int j = 0; j < k && !status; ++j) {
    double s = 0.0;
    if (tid >= j && tid < k) {
      s = sG[j * AT_PITCH + tid];
      if (tid == j) s += lam;
      const double gjj = s;
      for (int p = 0; p < j; ++p) s = __builtin_fma(-sG[tid * AT_PITCH + p], sG[j * AT_PITCH + p], s);
      scol[tid] = s;
      if (tid == j && !(s > AT_PIVOT * gjj)) sfail = 1;
    }
    __syncthreads();
    if (sfail) {
      status = 2;
      break;
    }
    const double dj = sqrt(scol[j]);
    if (tid == j) sd[j] = dj;
    if (tid > j && tid < k) sG[tid * AT_PITCH + j] = s / dj;
    __syncthreads();
  }
  if (tid == 0) {
    info[0] = status;
    info[1] = (int)n;
  }
  // wave wv takes the targets wv, wv + 4, ..; lane i owns component i of every vector over the axes
  for (int a = wv; a < N; a += AT_THREADS / 64) {
    const bool in = lane < k;
    const double g = in ? mom::range_sum(part, n_ranges, 3, 1, a, lane) / dof : 0.0;
    const double cdd = mom::range_sum(part, n_ranges, 3, 2, a, a) / dof;
    double beta = 0.0, r = 0.0;
    if (!status && cdd != 0.0) {
      // R z = g: once z_j is final, every lane below it takes fma(-R[i][j], z_j, .) -- row i in ascending j
      double s = g;
      for (int j = 0; j < k; ++j) {
        const double zj = __shfl(s, j, 64) / sd[j];
        if (lane == j) s = zj;
        if (in && lane > j) s = __builtin_fma(-sG[lane * AT_PITCH + j], zj, s);
      }
      // R^T beta = z: in descending j, the lanes above take fma(-R[j][i], beta_j, .)
      for (int j = k - 1; j >= 0; --j) {
        const double bj = __shfl(s, j, 64) / sd[j];
        if (lane == j) s = bj;
        if (lane < j) s = __builtin_fma(-sG[j * AT_PITCH + lane], bj, s);
      }
      beta = in ? s : 0.0;
      // (Cyy beta)_i in ascending j from +0, then the two dot products over the lanes
      double cb = 0.0;
      for (int j = 0; j < k; ++j) {
        const double bj = __shfl(beta, j, 64);
        if (in) cb = __builtin_fma(lane <= j ? sG[lane * AT_PITCH + j] : sG[j * AT_PITCH + lane], bj, cb);
      }
      const double bg = wave_sum_f64(beta * g), bcb = wave_sum_f64(beta * cb);
      r = 1.0 - (cdd - 2.0 * bg + bcb) / cdd;
    }
    if (in) B[(long)a * k + lane] = beta;
    if (lane == 0) r2[a] = r;
  }
}

// ws, every part on a 256-byte boundary: [y (T k) | targets (T N) | obs (T) bytes | the column sums' block sums
// (nb (1 + k + N)) | the partial tiles (n_ranges 3 64 64)]
struct attr_ws {
  long y, d, obs, nb, colsum, n_ranges, bytes;
};

attr_ws attr_layout(long T, long k, long N) {
  attr_ws w;
  const long D = (long)sizeof(double);
  w.y = up256(T * k * D);
  w.d = up256(T * N * D);
  w.obs = up256(T);
  w.nb = (T + mom::ROWS - 1) / mom::ROWS;
  w.colsum = up256(w.nb * (1 + k + N) * D);
  w.n_ranges = (T + mom::RANGE - 1) / mom::RANGE;
  w.bytes = w.y + w.d + w.obs + w.colsum + w.n_ranges * 3 * (long)mom::TILE * D;
  return w;
}

// the checks FIT and WORKSPACE share: T, k, N
int attr_shape(const rv_mosaic_desc* d, const char* op) {
  RV_REQUIRE(d->T >= 2 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): T=%ld outside [2, 2^31)", op, d->T);
  RV_REQUIRE(d->k >= 1 && d->k <= AT_KMAX, RV_ERR_SHAPE, "rv_mosaic(%s): k=%ld (the axes) outside [1, %d]", op, d->k, AT_KMAX);
  RV_REQUIRE(d->N >= 1 && d->N <= AT_NMAX, RV_ERR_SHAPE, "rv_mosaic(%s): N=%ld (the targets) outside [1, %d]", op, d->N, AT_NMAX);
  return RV_OK;
}

}  // namespace

int rv_attr_workspace(rv_mosaic_desc* d) {
  const int rc = attr_shape(d, "ATTR_WORKSPACE");
  if (rc) return rc;
  d->ws_bytes = attr_layout(d->T, d->k, d->N).bytes;
  return RV_OK;
}

int rv_attr_describe(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(ATTR_DESCRIBE): T=%ld outside [1, 2^31)", d->T);
  RV_REQUIRE(d->S >= 1 && d->S < INT_MAX, RV_ERR_SHAPE, "rv_mosaic(ATTR_DESCRIBE): S=%ld outside [1, 2^31)", d->S);
  RV_REQUIRE(d->hop >= 1 && d->hop < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(ATTR_DESCRIBE): hop=%ld outside [1, 2^31)", d->hop);
  RV_REQUIRE(d->frames, RV_ERR_NULL, "rv_mosaic(ATTR_DESCRIBE): frames is null");
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(ATTR_DESCRIBE): result (desc) is null");
  RV_REQUIRE(d->n_out >= d->S && (d->T - 1) * d->hop <= d->n_out - d->S, RV_ERR_SHAPE,
             "rv_mosaic(ATTR_DESCRIBE): T=%ld frames of S=%ld at hop=%ld overrun n_out=%ld", d->T, d->S, d->hop, d->n_out);
  RV_REQUIRE(d->dynamic_range > 0.f && d->dynamic_range <= 120.f, RV_ERR_SHAPE,
             "rv_mosaic(ATTR_DESCRIBE): dynamic_range=%g dB must be in (0, 120]", (double)d->dynamic_range);
  const long cols = d->window ? 5 : 3;
  RV_REQUIRE(d->ldo >= cols, RV_ERR_SHAPE, "rv_mosaic(ATTR_DESCRIBE): ldo=%ld holds no row of %ld descriptors", d->ldo, cols);
  if (d->window) {
    RV_REQUIRE(d->S >= spec::SMIN && d->S <= spec::SMAX && (d->S & (d->S - 1)) == 0, RV_ERR_SHAPE,
               "rv_mosaic(ATTR_DESCRIBE): S=%ld: the spectral columns (window given) need a power of two in [%d, %d]",
               d->S, spec::SMIN, spec::SMAX);
    RV_REQUIRE(d->twiddles, RV_ERR_NULL, "rv_mosaic(ATTR_DESCRIBE): window given but twiddles is null");
  }
  const float floor_scale = (float)pow(10.0, -(double)d->dynamic_range / 10.0);
  const dim3 grid((unsigned)d->T), block(AT_THREADS);
  const hipStream_t st = (hipStream_t)stream;
  if (d->window)
    hipLaunchKernelGGL(k_attr_describe<true>, grid, block, (2 * (d->S / 2) + 1) * sizeof(float), st, d->frames, d->hop, (int)d->S,
                       d->window, d->twiddles, floor_scale, d->result, d->ldo);
  else
    hipLaunchKernelGGL(k_attr_describe<false>, grid, block, 0, st, d->frames, d->hop, (int)d->S, (const float*)nullptr,
                       (const float*)nullptr, floor_scale, d->result, d->ldo);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_attr_fit(const rv_mosaic_desc* d, void* stream) {
  const int rc = attr_shape(d, "ATTR_FIT");
  if (rc) return rc;
  RV_REQUIRE(d->L >= d->k && d->L <= AT_LMAX, RV_ERR_SHAPE, "rv_mosaic(ATTR_FIT): L=%ld outside [k=%ld, %d]", d->L, d->k, AT_LMAX);
  RV_REQUIRE(d->stride >= d->L, RV_ERR_SHAPE, "rv_mosaic(ATTR_FIT): stride=%ld (the row pitch of x) holds no row of L=%ld values",
             d->stride, d->L);
  RV_REQUIRE(d->q, RV_ERR_NULL, "rv_mosaic(ATTR_FIT): q (the latent rows x) is null");
  RV_REQUIRE(d->centre, RV_ERR_NULL, "rv_mosaic(ATTR_FIT): centre is null");
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(ATTR_FIT): basis (P) is null");
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(ATTR_FIT): moment (the targets D) is null");
  RV_REQUIRE(isfinite(d->lam) && d->lam >= 0.f, RV_ERR_SHAPE, "rv_mosaic(ATTR_FIT): lam=%g (the ridge) must be finite and >= 0",
             (double)d->lam);
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(ATTR_FIT): result is null");
  RV_REQUIRE(d->info, RV_ERR_NULL, "rv_mosaic(ATTR_FIT): info is null");
  const attr_ws w = attr_layout(d->T, d->k, d->N);
  RV_REQUIRE(d->ws_bytes >= w.bytes, RV_ERR_SHAPE, "rv_mosaic(ATTR_FIT): ws_bytes=%ld, T=%ld frames of k=%ld axes and N=%ld targets need %ld",
             d->ws_bytes, d->T, d->k, d->N, w.bytes);
  RV_REQUIRE(d->ws, RV_ERR_NULL, "rv_mosaic(ATTR_FIT): ws is null, T=%ld frames of k=%ld axes and N=%ld targets need %ld bytes", d->T,
             d->k, d->N, w.bytes);
  RV_REQUIRE(((uintptr_t)d->ws & 255) == 0, RV_ERR_SHAPE, "rv_mosaic(ATTR_FIT): ws is not 256-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const int k = (int)d->k, N = (int)d->N;
  const long cols = 1 + d->k + d->N;
  char* at = (char*)d->ws;
  double* const ys = (double*)at;
  double* const ds = (double*)(at += w.y);
  unsigned char* const obs = (unsigned char*)(at += w.d);
  double* const colsum = (double*)(at += w.obs);
  double* const part = (double*)(at += w.colsum);
  hipLaunchKernelGGL(k_attr_observe, dim3((unsigned)((d->T + seq::FRAMES - 1) / seq::FRAMES)), dim3(seq::THREADS), 0, st, d->q,
                     d->stride, (const double*)d->centre, (const double*)d->basis, d->moment, d->T, (int)d->L, k, N, ys, ds, obs);
  hipLaunchKernelGGL(k_attr_colsum, dim3((unsigned)w.nb, (unsigned)((cols + mom::THREADS - 1) / mom::THREADS)), dim3(mom::THREADS), 0,
                     st, (const double*)ys, (const double*)ds, (const unsigned char*)obs, d->T, d->k, d->N, colsum);
  hipLaunchKernelGGL(k_attr_means, dim3(1), dim3(AT_THREADS), 0, st, (const double*)colsum, w.nb, cols, d->result);
  hipLaunchKernelGGL(k_attr_moments, dim3((unsigned)w.n_ranges, 3), dim3(mom::TILE_THREADS), 0, st, (const double*)ys, k,
                     (const double*)ds, N, (const unsigned char*)obs, (const double*)d->result, d->T, part);
  hipLaunchKernelGGL(k_attr_close, dim3(1), dim3(AT_THREADS), 0, st, (const double*)part, w.n_ranges, k, N, (double)d->lam,
                     d->result, d->info);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
