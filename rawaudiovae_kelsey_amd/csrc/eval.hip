// Held-out evaluation (rawaudiovae_kelsey_amd/evaluate.py): the two scoring ops of rv_mosaic.  The rules: include/
// rawvae_hip.h, "Evaluation"; the LDS layout, the error model and the measured figures: DESIGN.md section 7.9.
//   RV_EVAL_FRAMES  per frame pair (x, y): squared error, energy, KL, log-spectral distance and the two sums of the
//                   spectral convergence: k_eval_frames, one workgroup of 256 threads per pair.  The spectra come from a
//                   radix-2 transform in LDS, each signal transformed on its own.
//   RV_EVAL_DIMS    the KL sum of every latent dimension over the rows: k_eval_dims_block (one thread per (block of
//                   256 rows, dimension)), then k_eval_dims_sum over the blocks: moment.h's blocked column sum, which
//                   RV_PCA_MOMENTS' mean shares.  No atomics.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "internal.h"
#include "moment.h"
#include "spectrum.h"

using namespace rv;

namespace {

constexpr int EV_THREADS = spec::THREADS;
constexpr int EV_SMAX = spec::SMAX;      // longest frame with spectral columns
constexpr int EV_SMIN = spec::SMIN;

__device__ __forceinline__ double kl_term(float mu, float lv) {
  const double m = (double)mu, l = (double)lv;
  return -0.5 * (1.0 + l - m * m - exp(l));
}

// One workgroup per row t.  x = xs + t * hop, y = ys + t * stride, S samples each.
//
// Columns 0 / 1: thread u adds the terms n = u, u + 256, ... in ascending n from +0 in fp64, then block_sum_f64.
// Column 2 likewise over j < L.
//
// Spectral columns (SPEC): a[n] = fl(w[n] x[n]) and b[n] = fl(w[n] y[n]) go through spectrum.h's transform, each signal
// on its own, into the powers ar[0 .. N] and br[0 .. N], N = S / 2.  LDS: 4 N + 2 floats of dynamic shared memory (8 200
// bytes at S = 1024, 32 776 at S = 4096).
template <bool SPEC>
__global__ void __launch_bounds__(EV_THREADS)
k_eval_frames(const float* __restrict__ xs, long hop, const float* __restrict__ ys, long stride, int S,
              const float* __restrict__ mu, const float* __restrict__ lv, int L, const float* __restrict__ win,
              const float* __restrict__ tw, float floor_scale, float* __restrict__ out, long ldo) {
  extern __shared__ float lds[];   // SPEC: 4 N + 2 floats, sized by the launch; none otherwise
  __shared__ double red[EV_THREADS / 64];
  __shared__ float redf[EV_THREADS / 64];
  const long t = blockIdx.x;
  const float* x = xs + t * hop;
  const float* y = ys + t * stride;
  const int N = S >> 1;
  const int lg = spec::stages(N);
  float* const ar = lds;               // N + 1
  float* const ai = ar + N + 1;        // N
  float* const br = ai + N;            // N + 1
  float* const bi = br + N + 1;        // N

  double sse = 0.0, en = 0.0;
  for (int n = threadIdx.x; n < S; n += EV_THREADS) {
    const float xv = x[n], yv = y[n];
    const float d = yv - xv;
    sse += (double)d * (double)d;
    en += (double)xv * (double)xv;
    if constexpr (SPEC) {
      const float w = win[n];
      spec::put(ar, ai, n, lg, w * xv);
      spec::put(br, bi, n, lg, w * yv);
    }
  }
  sse = block_sum_f64<EV_THREADS / 64>(sse, red);
  en = block_sum_f64<EV_THREADS / 64>(en, red);
  double kl = 0.0;
  if (mu) {
    for (int j = threadIdx.x; j < L; j += EV_THREADS) kl += kl_term(mu[t * L + j], lv[t * L + j]);
    kl = block_sum_f64<EV_THREADS / 64>(kl, red);
  }
  float lsd = 0.f, serr = 0.f, sref = 0.f;
  if constexpr (SPEC) {
    float pmax = 0.f, pmax_b = 0.f;
    bool bad_a = false, bad_b = false;
    spec::powers(ar, ai, tw, N, pmax, bad_a);
    spec::powers(br, bi, tw, N, pmax_b, bad_b);
    pmax = spec::block_max_f32(fmaxf(pmax, pmax_b), redf);
    const int nbad_a = __syncthreads_or(bad_a), nbad_b = __syncthreads_or(bad_b);
    const float fl = pmax * floor_scale;
    double d2 = 0.0, se = 0.0, sr = 0.0;
    for (int k = threadIdx.x; k <= N; k += EV_THREADS) {
      const float pa = ar[k], pb = br[k];
      sr += (double)pa;
      if (fl > 0.f) {
        const float d = 10.f * log10f((pa + fl) / (pb + fl));
        const float e = sqrtf(pa) - sqrtf(pb);
        d2 += (double)(d * d);
        se += (double)(e * e);
      }
    }
    d2 = block_sum_f64<EV_THREADS / 64>(d2, red);
    se = block_sum_f64<EV_THREADS / 64>(se, red);
    sr = block_sum_f64<EV_THREADS / 64>(sr, red);
    if (fl > 0.f) {
      lsd = (float)sqrt(d2 / (double)(N + 1));
      serr = (float)se;
      sref = (float)sr;
    }
    if (nbad_a || nbad_b) lsd = serr = NAN;
    if (nbad_a) sref = NAN;
  }
  if (threadIdx.x == 0) {
    float* o = out + t * ldo;
    o[0] = (float)sse;
    o[1] = (float)en;
    o[2] = (float)kl;
    o[3] = lsd;
    o[4] = serr;
    o[5] = sref;
  }
}

// Grid (blocks of 256 rows, tiles of 64 dimensions), moment.h's blocked column sum: thread (b, j) adds rows
// [256 b, 256 b + 256) of dimension j in ascending t from +0 into part[b, j] (which is `cost` itself when there is one
// block).
__global__ void __launch_bounds__(mom::THREADS)
k_eval_dims_block(const float* __restrict__ mu, const float* __restrict__ lv, long T, long L, double* __restrict__ part) {
  mom::colsum_block([=](long t, long j) { return kl_term(mu[t * L + j], lv[t * L + j]); }, T, L, part);
}

// cost[j] = the block sums of dimension j in ascending block order from +0
__global__ void __launch_bounds__(mom::THREADS)
k_eval_dims_sum(const double* __restrict__ part, long nb, long L, double* __restrict__ cost) {
  const long j = (long)blockIdx.x * mom::THREADS + threadIdx.x;
  if (j >= L) return;
  cost[j] = mom::colsum_total(part, nb, L, j);
}

}  // namespace

int rv_eval_frames(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(EVAL_FRAMES): T=%ld outside [1, 2^31)", d->T);
  RV_REQUIRE(d->S >= 1 && d->S < INT_MAX, RV_ERR_SHAPE, "rv_mosaic(EVAL_FRAMES): S=%ld outside [1, 2^31)", d->S);
  RV_REQUIRE(d->hop >= 1 && d->hop < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(EVAL_FRAMES): hop=%ld outside [1, 2^31)", d->hop);
  RV_REQUIRE(d->stride >= 1 && d->stride < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(EVAL_FRAMES): stride=%ld outside [1, 2^31)",
             d->stride);
  RV_REQUIRE(d->frames, RV_ERR_NULL, "rv_mosaic(EVAL_FRAMES): frames is null");
  RV_REQUIRE(d->src, RV_ERR_NULL, "rv_mosaic(EVAL_FRAMES): src is null");
  RV_REQUIRE(d->out, RV_ERR_NULL, "rv_mosaic(EVAL_FRAMES): out is null");
  RV_REQUIRE(d->ldo >= 6, RV_ERR_SHAPE, "rv_mosaic(EVAL_FRAMES): ldo=%ld holds no row of 6 scores", d->ldo);
  RV_REQUIRE(d->n_out >= d->S && (d->T - 1) * d->hop <= d->n_out - d->S, RV_ERR_SHAPE,
             "rv_mosaic(EVAL_FRAMES): T=%ld frames of S=%ld at hop=%ld overrun n_out=%ld", d->T, d->S, d->hop, d->n_out);
  RV_REQUIRE(d->src_len >= d->S && (d->T - 1) * d->stride <= d->src_len - d->S, RV_ERR_SHAPE,
             "rv_mosaic(EVAL_FRAMES): T=%ld rows of S=%ld at stride=%ld overrun src_len=%ld", d->T, d->S, d->stride,
             d->src_len);
  RV_REQUIRE(!d->mu == !d->logvar, RV_ERR_NULL, "rv_mosaic(EVAL_FRAMES): %s is null but %s is not: the KL column needs both",
             d->mu ? "logvar" : "mu", d->mu ? "mu" : "logvar");
  if (d->mu)
    RV_REQUIRE(d->L >= 1 && d->L <= (1L << 20), RV_ERR_SHAPE, "rv_mosaic(EVAL_FRAMES): L=%ld outside [1, 2^20]", d->L);
  RV_REQUIRE(d->dynamic_range > 0.f && d->dynamic_range <= 120.f, RV_ERR_SHAPE,
             "rv_mosaic(EVAL_FRAMES): dynamic_range=%g dB must be in (0, 120]", (double)d->dynamic_range);
  if (d->window) {
    RV_REQUIRE(d->S >= EV_SMIN && d->S <= EV_SMAX && (d->S & (d->S - 1)) == 0, RV_ERR_SHAPE,
               "rv_mosaic(EVAL_FRAMES): S=%ld: the spectral columns (window given) need a power of two in [%d, %d]",
               d->S, EV_SMIN, EV_SMAX);
    RV_REQUIRE(d->twiddles, RV_ERR_NULL, "rv_mosaic(EVAL_FRAMES): window given but twiddles is null");
  }
  const float floor_scale = (float)pow(10.0, -(double)d->dynamic_range / 10.0);
  const dim3 grid((unsigned)d->T), block(EV_THREADS);
  const hipStream_t st = (hipStream_t)stream;
  if (d->window)
    hipLaunchKernelGGL(k_eval_frames<true>, grid, block, (4 * (d->S / 2) + 2) * sizeof(float), st, d->frames, d->hop, d->src, d->stride, (int)d->S, d->mu,
                       d->logvar, (int)d->L, d->window, d->twiddles, floor_scale, d->out, d->ldo);
  else
    hipLaunchKernelGGL(k_eval_frames<false>, grid, block, 0, st, d->frames, d->hop, d->src, d->stride, (int)d->S, d->mu,
                       d->logvar, (int)d->L, (const float*)nullptr, (const float*)nullptr, floor_scale, d->out, d->ldo);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_eval_dims(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(EVAL_DIMS): T=%ld outside [1, 2^31)", d->T);
  RV_REQUIRE(d->L >= 1 && d->L <= (1L << 20), RV_ERR_SHAPE, "rv_mosaic(EVAL_DIMS): L=%ld outside [1, 2^20]", d->L);
  RV_REQUIRE(d->mu, RV_ERR_NULL, "rv_mosaic(EVAL_DIMS): mu is null");
  RV_REQUIRE(d->logvar, RV_ERR_NULL, "rv_mosaic(EVAL_DIMS): logvar is null");
  RV_REQUIRE(d->cost, RV_ERR_NULL, "rv_mosaic(EVAL_DIMS): cost is null");
  const long nb = (d->T + mom::ROWS - 1) / mom::ROWS;
  const long need = nb > 1 ? nb * d->L * (long)sizeof(double) : 0;
  RV_REQUIRE(d->ws_bytes >= need, RV_ERR_SHAPE, "rv_mosaic(EVAL_DIMS): ws_bytes=%ld, T=%ld rows of L=%ld need %ld", d->ws_bytes,
             d->T, d->L, need);
  RV_REQUIRE(need == 0 || d->ws, RV_ERR_NULL, "rv_mosaic(EVAL_DIMS): ws is null, T=%ld rows of L=%ld need %ld bytes", d->T,
             d->L, need);
  const hipStream_t st = (hipStream_t)stream;
  const unsigned tiles = (unsigned)((d->L + mom::THREADS - 1) / mom::THREADS);
  double* part = nb > 1 ? (double*)d->ws : d->cost;
  hipLaunchKernelGGL(k_eval_dims_block, dim3((unsigned)nb, tiles), dim3(mom::THREADS), 0, st, d->mu, d->logvar, d->T, d->L, part);
  if (nb > 1)
    hipLaunchKernelGGL(k_eval_dims_sum, dim3(tiles), dim3(mom::THREADS), 0, st, (const double*)d->ws, nb, d->L, d->cost);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
