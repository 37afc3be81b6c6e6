// Latent interpolation and resynthesis (tutorial.ipynb:456-530, 834-925, 1200-1279): the two element-wise steps between the
// exact-fp32 encoder and decoder GEMMs (rv_linear_fp32).
//   rv_match_pad  : a source's padded device waveform -- repeat-the-shorter or crop, then zeros up to the framing's
//                   padded length (one launch, no host copy of the matched audio).
//   rv_latent_mix : mu = mu_a (1 - a) + mu_b a, logvar likewise, z = mu + eps exp(logvar / 2), for one chunk of output
//                   rows; a from a list of scalars, a per-frame array, or a control curve stretched in the kernel
//                   (scipy.interpolate.interp1d evaluated at numpy.linspace).
#include "common.h"
#include "philox.h"
#include "reparam.h"
#include "../../include/rawvae_hip.h"

using namespace rv;

namespace {

unsigned grid_of(long n, long cap = 4096) {
  long g = (n + 255) / 256;
  return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

__global__ void __launch_bounds__(256)
k_match_pad(const float* __restrict__ src, long n_src, long n_valid, float* __restrict__ dst, long n_out) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_out; i += (long)gridDim.x * 256)
    dst[i] = i < n_valid ? src[i % n_src] : 0.f;
}

// alpha of output row r (frame n = r mod N, list entry k = r / N).  The fp32 modes return (1 - a, a) rounded as torch
// rounds them: a python/numpy float64 scalar meets an fp32 tensor as an fp32 scalar (so 1 - a is formed in float64 and
// rounded once); an fp32 tensor a gives 1 - a in fp32.
__device__ __forceinline__ double curve_alpha(const double* __restrict__ y, long C, long N, long n) {
#pragma clang fp contract(off)
  // numpy.linspace(0, C - 1, N): x = n * step + 0, step = (C - 1) / (N - 1), the last point exactly C - 1
  double x;
  if (N == 1) x = 0.0;
  else if (n == N - 1) x = (double)(C - 1);
  else x = (double)n * ((double)(C - 1) / (double)(N - 1)) + 0.0;
  // interp1d(arange(C), y) on a 1-D curve evaluates through numpy.interp: j = the grid point at or below x; x on the
  // grid (the last point included) gives y[j] itself, otherwise y[j] + slope (x - j), slope = (y[j+1] - y[j]) / 1
  long j = (long)floor(x);
  j = j > C - 1 ? C - 1 : j;
  if (x == (double)j) return y[j];
  const double slope = y[j + 1] - y[j];
  return slope * (x - (double)j) + y[j];
}

// a * wa + b * wb with every product and the sum rounded to nearest (what __fmul_rn / __fadd_rn mean).  Plain operators
// under the pragma: the __*_rn helpers are header functions whose own fmul / fadd carry the file's fp-contract=fast
// flag, and after inlining the backend fused them into v_fmac.  Checked in the ISA: v_mul + v_mul + v_add (or their
// v_pk_ forms), no v_fma / v_fmac on the mix.  The same holds for the fp64 helpers below.
__device__ __forceinline__ float mix_f32(float a, float wa, float b, float wb) {
#pragma clang fp contract(off)
  return a * wa + b * wb;
}

__device__ __forceinline__ double mix_f64(double a, double wa, double b, double wb) {
#pragma clang fp contract(off)
  return a * wa + b * wb;
}

// fp64 reparameterisation of torch's float64 path (std = exp(0.5 logvar); mu + eps * std), no contraction
__device__ __forceinline__ double reparam_f64(double m, double lv, double e) {
#pragma clang fp contract(off)
  return m + e * exp(0.5 * lv);
}

template <int MODE>
__global__ void __launch_bounds__(256)
k_latent_mix(const float* __restrict__ mu_a, const float* __restrict__ lv_a, const float* __restrict__ mu_b,
             const float* __restrict__ lv_b, long N, long L, const void* __restrict__ alpha, long n_alpha, long row0,
             long rows, const float* __restrict__ eps_in, float* __restrict__ eps_out, uint64_t seed, uint64_t offset,
             float* __restrict__ z, float* __restrict__ mu_out, float* __restrict__ lv_out,
             double* __restrict__ alpha_out) {
  const long total = rows * L;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long r = row0 + i / L, l = i % L;
    const long n = MODE == RV_ALPHA_LIST ? r % N : r;
    const long src = n * L + l;
    const long gi = r * L + l;   // flat index of the element in the whole [rows_total, L] output: the Philox counter
    float e;
    if (eps_in) {
      e = eps_in[i];
    } else {
      e = normal1(seed, (uint64_t)gi, offset);
      if (eps_out) eps_out[i] = e;
    }
    if constexpr (MODE == RV_ALPHA_LIST || MODE == RV_ALPHA_F32) {
      float wa, wb;
      if constexpr (MODE == RV_ALPHA_LIST) {
        const double a = static_cast<const double*>(alpha)[r / N];
        wa = (float)(1.0 - a);
        wb = (float)a;
      } else {
        wb = static_cast<const float*>(alpha)[n];
        wa = 1.f - wb;
      }
      const float m = mix_f32(mu_a[src], wa, mu_b[src], wb);
      const float lv = mix_f32(lv_a[src], wa, lv_b[src], wb);
      z[i] = reparam_z(m, lv, e);
      if (mu_out) mu_out[i] = m;
      if (lv_out) lv_out[i] = lv;
      if (alpha_out && l == 0) alpha_out[i / L] = (double)wb;
    } else {
      const double a = MODE == RV_ALPHA_CURVE ? curve_alpha(static_cast<const double*>(alpha), n_alpha, N, n)
                                              : static_cast<const double*>(alpha)[n];
      const double wa = 1.0 - a;
      const double m = mix_f64(mu_a[src], wa, mu_b[src], a);
      const double lv = mix_f64(lv_a[src], wa, lv_b[src], a);
      z[i] = (float)reparam_f64(m, lv, e);
      if (mu_out) mu_out[i] = (float)m;
      if (lv_out) lv_out[i] = (float)lv;
      if (alpha_out && l == 0) alpha_out[i / L] = a;
    }
  }
}

}  // namespace

extern "C" int rv_match_pad(const float* src, long n_src, long n_valid, float* dst, long n_out, void* stream) {
  RV_REQUIRE(dst && (src || n_valid == 0), RV_ERR_NULL, "rv_match_pad: null pointer");
  RV_REQUIRE(n_src >= 0 && n_valid >= 0 && n_valid <= n_out && (n_valid == 0 || n_src > 0), RV_ERR_SHAPE,
             "rv_match_pad: bad extents n_src=%ld n_valid=%ld n_out=%ld", n_src, n_valid, n_out);
  if (n_out == 0) return RV_OK;
  hipLaunchKernelGGL(k_match_pad, dim3(grid_of(n_out)), dim3(256), 0, (hipStream_t)stream, src, n_src, n_valid, dst,
                     n_out);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_latent_mix(const float* mu_a, const float* lv_a, const float* mu_b, const float* lv_b, long N,
                             long L, int alpha_mode, const void* alpha, long n_alpha, long row0, long rows,
                             const float* eps_in, float* eps_out, unsigned long long seed, unsigned long long offset,
                             float* z, float* mu_out, float* lv_out, double* alpha_out, void* stream) {
  RV_REQUIRE(mu_a && lv_a && mu_b && lv_b && alpha && z, RV_ERR_NULL, "rv_latent_mix: null pointer");
  RV_REQUIRE(alpha_mode >= RV_ALPHA_LIST && alpha_mode <= RV_ALPHA_CURVE, RV_ERR_UNSUPPORTED,
             "rv_latent_mix: alpha_mode %d", alpha_mode);
  RV_REQUIRE(N > 0 && L > 0 && row0 >= 0 && rows >= 0, RV_ERR_SHAPE, "rv_latent_mix: bad extents N=%ld L=%ld", N, L);
  const long rows_total = alpha_mode == RV_ALPHA_LIST ? n_alpha * N : N;
  RV_REQUIRE(alpha_mode == RV_ALPHA_CURVE ? n_alpha >= 2 : (alpha_mode == RV_ALPHA_LIST ? n_alpha >= 1 : n_alpha == N),
             RV_ERR_SHAPE, "rv_latent_mix: %ld alpha values for mode %d and %ld frames", n_alpha, alpha_mode, N);
  RV_REQUIRE(row0 + rows <= rows_total, RV_ERR_SHAPE, "rv_latent_mix: rows [%ld, %ld) outside the %ld output rows",
             row0, row0 + rows, rows_total);
  if (rows == 0) return RV_OK;
  const dim3 g(grid_of(rows * L)), b(256);
  auto st = (hipStream_t)stream;
#define RV_MIX_LAUNCH(M)                                                                                              \
  hipLaunchKernelGGL(k_latent_mix<M>, g, b, 0, st, mu_a, lv_a, mu_b, lv_b, N, L, alpha, n_alpha, row0, rows, eps_in, \
                     eps_out, (uint64_t)seed, (uint64_t)offset, z, mu_out, lv_out, alpha_out)
  switch (alpha_mode) {
    case RV_ALPHA_LIST: RV_MIX_LAUNCH(RV_ALPHA_LIST); break;
    case RV_ALPHA_F32: RV_MIX_LAUNCH(RV_ALPHA_F32); break;
    case RV_ALPHA_F64: RV_MIX_LAUNCH(RV_ALPHA_F64); break;
    default: RV_MIX_LAUNCH(RV_ALPHA_CURVE); break;
  }
#undef RV_MIX_LAUNCH
  RV_CHECK_LAUNCH();
  return RV_OK;
}
