// Switching walk (rawaudiovae_kelsey_amd/switching.py): one linear-Gaussian law per state of a fitted hidden Markov model,
// fitted under its posteriors and run block by block like the latent walk.  Five ops of rv_mosaic; the rules, down to the
// order of every add: include/rawvae_hip.h, "Switching walk"; the derivation and the measured figures: DESIGN.md section 7.18.
//   RV_SWITCH_RESIDUAL   k_switch_residual: a workgroup per block of 64 frames stages their y in LDS (sequence.h) and writes
//                        the standardised residual r [T, k] and the observed flags.
//   RV_SWITCH_MOMENTS    k_switch_keep (which pairs count), k_switch_occupancy (moment.h's blocked column sum),
//                        k_switch_moments (moment.h's MFMA tile under its `gated` operands: S + 2 tiles per range of 4096
//                        pairs), k_switch_sum over the ranges.
//   RV_SWITCH_FIT        k_switch_dynamics and k_switch_gram (A_j and Q_j of every state), k_switch_noise (the guard and
//                        [A_j^T | B_j^T]).  Small dense fp64, not tuned.
//   RV_SWITCH_STEP       F frames of every stream in one launch, one workgroup per stream: k_switch_step; then
//                        rv_stream_synth's fc3, fc4 and overlap-add.
//   RV_SWITCH_WORKSPACE  the bytes of ws of RV_SWITCH_MOMENTS.
// No atomics, no polling; every output element is written by exactly one thread.
#include <math.h>

#include "common.h"
#include "philox.h"
#include "internal.h"
#include "moment.h"
#include "sequence.h"

using namespace rv;

namespace {

constexpr int SW_SMAX = 64;
constexpr int SW_KMAX = 64;
constexpr int SW_LMAX = 512;
constexpr int SW_THREADS = seq::THREADS;
constexpr int SW_FRAMES = seq::FRAMES;
constexpr int SW_PITCH = seq::PITCH;

// one rounding each, never contracted into an fma
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// (of the HMM's theta = [m (S k) | w (S k) | ..] only m and w are read, at offsets 0 and S k)
// the parts of phi = [m (S k) | sd (S k) | pi (S) | A_hmm (S S) | dyn (S 2 k k)]
struct phi_at {
  long m, sd, pi, A, dyn, doubles;
};
__host__ __device__ __forceinline__ phi_at phi_layout(long S, long k) {
  phi_at o;
  o.m = 0;
  o.sd = S * k;
  o.pi = 2 * S * k;
  o.A = o.pi + S;
  o.dyn = o.A + S * S;
  o.doubles = o.dyn + S * 2 * k * k;
  return o;
}

// r[t, j] = chain fma(gamma[t, i], fl(fl(y_j - m_ij) sqrt(w_ij)), .) in ascending i from +0; +0 for an unobserved frame
__global__ void __launch_bounds__(SW_THREADS)
k_switch_residual(const float* __restrict__ x, long ldx, const double* __restrict__ centre, const double* __restrict__ P,
                  const double* __restrict__ theta, const double* __restrict__ gamma, long T, int L, int k, int S,
                  double* __restrict__ r, unsigned char* __restrict__ obs) {
  __shared__ double sy[SW_FRAMES * SW_PITCH];
  __shared__ unsigned char sflag[SW_THREADS], sbad[SW_FRAMES];
  const long t0 = (long)blockIdx.x * SW_FRAMES;
  const int nf = T - t0 < SW_FRAMES ? (int)(T - t0) : SW_FRAMES;
  seq::stage_frames(x, ldx, centre, P, t0, nf, L, k, sy, sflag, sbad);
  const double* const m = theta;
  const double* const w = theta + (long)S * k;
  for (int e = threadIdx.x; e < nf * k; e += SW_THREADS) {
    const int f = e / k, j = e - f * k;
    double acc = 0.0;
    if (!sbad[f]) {
      const double y = sy[f * SW_PITCH + j];
      const double* const g = gamma + (t0 + f) * S;
      for (int i = 0; i < S; ++i)
        acc = __builtin_fma(g[i], mul_rn(add_rn(y, -m[(long)i * k + j]), sqrt(w[(long)i * k + j])), acc);
    }
    r[t0 * k + e] = acc;
  }
  if (threadIdx.x < nf) obs[t0 + threadIdx.x] = !sbad[threadIdx.x];
}

// keep[p] = 1 when frames p and p + 1 lie in one file (RV_PCA_LAGCOV's rule: p + 1 is none of row_start[0 .. n_files]) and
// both are observed
__global__ void __launch_bounds__(256)
k_switch_keep(const long long* __restrict__ row_start, long n_files, const unsigned char* __restrict__ obs, long n_pairs,
              unsigned char* __restrict__ keep) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pairs) return;
  keep[p] = (!seq::pair_spans_files(row_start, n_files, p) && obs[p] && obs[p + 1]) ? 1 : 0;
}

// npart[b, j] = keep[p] gamma[p + 1, j] over the pairs of block b in ascending p from +0
__global__ void __launch_bounds__(mom::THREADS)
k_switch_occupancy(const double* __restrict__ gamma, const unsigned char* __restrict__ keep, long n_pairs, long S,
                   double* __restrict__ npart) {
  mom::colsum_block([=](long p, long j) { return keep[p] ? gamma[(p + 1) * S + j] : 0.0; }, n_pairs, S, npart);
}

// Grid (ranges of pairs, S + 2): tile j < S is C1_j, tile S is D', tile S + 1 is D
__global__ void __launch_bounds__(mom::TILE_THREADS)
k_switch_moments(const double* __restrict__ gamma, int S, const double* __restrict__ r, int k,
                 const unsigned char* __restrict__ keep, long n_pairs, double* __restrict__ part) {
  __shared__ double As[mom::STAGE];
  __shared__ double Bs[mom::STAGE];
  const int j = (int)blockIdx.y, n_tiles = S + 2;
  if (j < S) mom::gated_tile<mom::GATED_CROSS>(As, Bs, gamma, S, j, r, k, keep, n_pairs, n_tiles, part);
  else if (j == S) mom::gated_tile<mom::GATED_NEXT_SQ>(As, Bs, gamma, S, 0, r, k, keep, n_pairs, n_tiles, part);
  else mom::gated_tile<mom::GATED_THIS_SQ>(As, Bs, gamma, S, 0, r, k, keep, n_pairs, n_tiles, part);
}

// out = [N (S) | D' (S k) | D (S k) | C1 (S k k)]: the block sums / the ranges' partials in ascending order from +0
__global__ void __launch_bounds__(256)
k_switch_sum(const double* __restrict__ npart, long nb, const double* __restrict__ part, long n_ranges, int S, int k,
             double* __restrict__ out) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long sk = (long)S * k, kk = (long)k * k;
  if (e < S) {
    out[e] = mom::colsum_total(npart, nb, S, e);
  } else if (e < S + 2 * sk) {
    const long f = e - S;
    const int which = f >= sk, g = (int)(f - which * sk);
    out[e] = mom::range_sum(part, n_ranges, S + 2, S + which, g / k, g % k);
  } else if (e < S + 2 * sk + S * kk) {
    const long f = e - S - 2 * sk;
    const int j = (int)(f / kk), g = (int)(f - j * kk);
    out[e] = mom::range_sum(part, n_ranges, S + 2, j, g / k, g % k);
  }
}

__device__ __forceinline__ bool positive_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

// A_j[a, b] = (C1_j[a, b] / sqrt(D'_j[a])) / sqrt(D_j[b]); 0 where a D is not positive and finite, or where N_j < 2
__global__ void __launch_bounds__(256)
k_switch_dynamics(const double* __restrict__ mo, int S, int k, double* __restrict__ A, int* __restrict__ info) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long kk = (long)k * k;
  if (e >= S * kk) return;
  const int j = (int)(e / kk), g = (int)(e - j * kk), a = g / k, b = g - a * k;
  const bool thin = !(mo[j] >= 2.0);
  if (g == 0) info[j] = thin;
  const double dn = mo[S + (long)j * k + a], dt = mo[S + (long)S * k + (long)j * k + b];
  double v = 0.0;
  if (!thin && positive_finite(dn) && positive_finite(dt)) v = (mo[S + 2L * S * k + e] / sqrt(dn)) / sqrt(dt);
  A[e] = v;
}

// Q_j[i, l] for i <= l = (i == l ? 1 : 0) - chain_m fma(A_j[i, m], A_j[l, m], .), written to [i, l] and [l, i]: RV_WALK_FIT's
// rule for Q.  Grid (blocks of 256 elements, S).
__global__ void __launch_bounds__(256)
k_switch_gram(const double* __restrict__ A, int k, double* __restrict__ Q) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)k * k) return;
  const int i = (int)(e / k), l = (int)(e - (long)i * k);
  if (i > l) return;
  const double* const a = A + (long)blockIdx.y * k * k;
  double* const q = Q + (long)blockIdx.y * k * k;
  double acc = 0.0;
  for (int m = 0; m < k; ++m) acc = __builtin_fma(a[(long)i * k + m], a[(long)l * k + m], acc);
  const double v = (i == l ? 1.0 : 0.0) - acc;
  q[(long)i * k + l] = v;
  q[(long)l * k + i] = v;
}

// The contraction guard and dyn_j = [A_j^T | B_j^T].  Grid (blocks of 256 elements, S).
__global__ void __launch_bounds__(256)
k_switch_noise(const double* __restrict__ A, const double* __restrict__ U, const double* __restrict__ q, int k,
               double* __restrict__ dyn, double* __restrict__ shrink) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const long kk = (long)k * k, s = blockIdx.y;
  if (e >= kk) return;
  const double* const qs = q + s * k;
  double qmin = qs[0];
  for (int j = 1; j < k; ++j) qmin = qs[j] < qmin ? qs[j] : qmin;
  const bool act = qmin < 0.0;
  const double h = act ? 1.0 / add_rn(1.0, -qmin) : 1.0;
  const double g = act ? sqrt(h) : 1.0;
  const int j = (int)(e / k), i = (int)(e - (long)j * k);
  const double a = A[s * kk + (long)i * k + j];
  double qj = qs[j];
  if (act) qj = add_rn(1.0, -mul_rn(h, add_rn(1.0, -qj)));
  dyn[s * 2 * kk + e] = act ? mul_rn(g, a) : a;
  dyn[s * 2 * kk + kk + e] = mul_rn(sqrt(fmax(qj, 0.0)), U[s * kk + e]);
  if (e == 0) shrink[s] = g;
}

using seq::latent_of;
using seq::noise_of;

// the uniform of (seed, stream, absolute frame): the first word of Philox at (lo = frame, hi = 2^32 + stream)
__device__ __forceinline__ float state_uniform(uint64_t seed, uint64_t frame, uint64_t stream) {
  const u32x4 r = philox4x32_10(seed, frame, ((uint64_t)1 << 32) + stream);
  return fminf(((float)r.x + 0.5f) * 2.3283064365386963e-10f, 0.99999994f);
}

// the first j with v < cum_j, cum the plain sums of law in ascending j from +0; none: the highest j with law_j > 0 (0
// when there is none)
__device__ __forceinline__ int draw_state(const double* __restrict__ law, int S, double v) {
  double cum = 0.0;
  int last = 0;
  for (int j = 0; j < S; ++j) {
    const double p = law[j];
    cum = add_rn(cum, p);
    if (v < cum) return j;
    if (p > 0.0) last = j;
  }
  return last;
}

// One workgroup per stream; the F frames of the call one after the other.  LDS: the standardised state u, the frame's
// noise e, the new state, the whitened row y.  Thread i owns coordinate i (A^T and B^T are read along their rows), then
// thread l owns latent l (R read along its rows).
__global__ void __launch_bounds__(SW_THREADS)
k_switch_step(const double* __restrict__ phi, const double* __restrict__ R, const double* __restrict__ centre, int S, int k,
              int L, long F, const long long* __restrict__ cnt, const float* __restrict__ eps, uint64_t seed,
              const float* __restrict__ temperature, const float* __restrict__ offset, const int* __restrict__ forced,
              const float* __restrict__ uniforms, double* __restrict__ state, int* __restrict__ primed,
              int* __restrict__ current, int* __restrict__ path, float* __restrict__ z, float* __restrict__ out, long ldo) {
  __shared__ double su[SW_KMAX], se[SW_KMAX], sn[SW_KMAX], sy[SW_KMAX];
  __shared__ int snext;
  const long s = blockIdx.x;
  const int tid = threadIdx.x;
  const phi_at o = phi_layout(S, k);
  const long long c0 = cnt[s];
  bool pr = primed[s] != 0;
  int cur = current[s];
  const double temp = (double)temperature[s];
  if (tid < k) su[tid] = state[s * k + tid];
  for (long fr = 0; fr < F; ++fr) {
    const long row = s * F + fr;
    if (tid == 0) {
      const int want = forced ? forced[row] : -1;
      int nx = want;
      if (want < 0 || want >= S) {
        const float v = uniforms ? uniforms[row] : state_uniform(seed, (uint64_t)(c0 + fr), (uint64_t)s);
        const bool chain = pr && cur >= 0 && cur < S;
        nx = draw_state(phi + (chain ? o.A + (long)cur * S : o.pi), S, (double)v);
      }
      snext = nx;
      path[row] = nx;
    }
    if (tid < k) {
      const float e = eps ? eps[row * k + tid] : normal1(seed, (uint64_t)((c0 + fr) * k + tid), (uint64_t)s);
      se[tid] = noise_of(temp, e);
    }
    __syncthreads();   // the state, e and u are written; the latent rows of the frame before have read y
    cur = snext;
    const double* const At = phi + o.dyn + (long)cur * 2 * k * k;
    const double* const Bt = At + (long)k * k;
    if (tid < k) {
      double acc = se[tid];
      if (pr) {
        acc = 0.0;
        for (int j = 0; j < k; ++j) acc = __builtin_fma(At[(long)j * k + tid], su[j], acc);
        for (int j = 0; j < k; ++j) acc = __builtin_fma(Bt[(long)j * k + tid], se[j], acc);
      }
      sn[tid] = acc;
      sy[tid] = __builtin_fma(phi[o.sd + (long)cur * k + tid], acc, phi[o.m + (long)cur * k + tid]);
    }
    __syncthreads();
    if (tid < k) su[tid] = sn[tid];
    pr = true;
    for (int l = tid; l < L; l += SW_THREADS) {
      double acc = 0.0;
      for (int j = 0; j < k; ++j) acc = __builtin_fma(sy[j], R[(long)j * L + l], acc);
      const float v = latent_of(centre[l], offset[s * L + l], acc);
      z[row * L + l] = v;
      if (out) out[row * ldo + l] = v;
    }
    __syncthreads();   // y and the state's number are read before the next frame writes them
  }
  if (tid < k) state[s * k + tid] = su[tid];
  if (tid == 0) {
    primed[s] = 1;
    current[s] = cur;
  }
}

// ws of RV_SWITCH_MOMENTS, every part on a 256-byte boundary: [keep (T - 1) bytes | the occupancy's block sums (nb S) | the
// partial tiles (n_ranges (S + 2) 64 64)]
struct switch_ws {
  long n_pairs, keep, nb, npart, n_ranges, bytes;
};

switch_ws switch_layout(long T, long S) {
  switch_ws w;
  const long D = (long)sizeof(double);
  w.n_pairs = T - 1;
  w.keep = up256(w.n_pairs);
  w.nb = (w.n_pairs + mom::ROWS - 1) / mom::ROWS;
  w.npart = up256(w.nb * S * D);
  w.n_ranges = (w.n_pairs + mom::RANGE - 1) / mom::RANGE;
  w.bytes = w.keep + w.npart + w.n_ranges * (S + 2) * (long)mom::TILE * D;
  return w;
}

// the checks every op shares: S, k
int switch_shape(const rv_mosaic_desc* d, const char* op) {
  RV_REQUIRE(d->S >= 1 && d->S <= SW_SMAX, RV_ERR_SHAPE, "rv_mosaic(%s): S=%ld (the states) outside [1, %d]", op, d->S, SW_SMAX);
  RV_REQUIRE(d->k >= 1 && d->k <= SW_KMAX, RV_ERR_SHAPE, "rv_mosaic(%s): k=%ld (the axes) outside [1, %d]", op, d->k, SW_KMAX);
  return RV_OK;
}

unsigned blocks256(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

int rv_switch_workspace(rv_mosaic_desc* d) {
  RV_REQUIRE(d->T >= 2 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(SWITCH_WORKSPACE): T=%ld outside [2, 2^31)", d->T);
  const int rc = switch_shape(d, "SWITCH_WORKSPACE");
  if (rc) return rc;
  d->ws_bytes = switch_layout(d->T, d->S).bytes;
  return RV_OK;
}

int rv_switch_residual(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(SWITCH_RESIDUAL): T=%ld outside [1, 2^31)", d->T);
  const int rc = switch_shape(d, "SWITCH_RESIDUAL");
  if (rc) return rc;
  RV_REQUIRE(d->L >= d->k && d->L <= SW_LMAX, RV_ERR_SHAPE, "rv_mosaic(SWITCH_RESIDUAL): L=%ld outside [k=%ld, %d]", d->L, d->k,
             SW_LMAX);
  RV_REQUIRE(d->stride >= d->L, RV_ERR_SHAPE,
             "rv_mosaic(SWITCH_RESIDUAL): stride=%ld (the row pitch of x) holds no row of L=%ld values", d->stride, d->L);
  RV_REQUIRE(d->q, RV_ERR_NULL, "rv_mosaic(SWITCH_RESIDUAL): q (the latent rows x) is null");
  RV_REQUIRE(d->centre, RV_ERR_NULL, "rv_mosaic(SWITCH_RESIDUAL): centre is null");
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(SWITCH_RESIDUAL): basis (P) is null");
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(SWITCH_RESIDUAL): moment (theta) is null");
  RV_REQUIRE(d->state, RV_ERR_NULL, "rv_mosaic(SWITCH_RESIDUAL): state (gamma) is null");
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(SWITCH_RESIDUAL): result (the residual block) is null");
  RV_REQUIRE(((uintptr_t)d->result & 255) == 0, RV_ERR_SHAPE, "rv_mosaic(SWITCH_RESIDUAL): result is not 256-byte aligned");
  unsigned char* const obs = (unsigned char*)d->result + up256(d->T * d->k * (long)sizeof(double));
  hipLaunchKernelGGL(k_switch_residual, dim3((unsigned)((d->T + SW_FRAMES - 1) / SW_FRAMES)), dim3(SW_THREADS), 0,
                     (hipStream_t)stream, d->q, d->stride, (const double*)d->centre, (const double*)d->basis, d->moment,
                     (const double*)d->state, d->T, (int)d->L, (int)d->k, (int)d->S, d->result, obs);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_switch_moments(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->T >= 2 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(SWITCH_MOMENTS): T=%ld outside [2, 2^31)", d->T);
  const int rc = switch_shape(d, "SWITCH_MOMENTS");
  if (rc) return rc;
  RV_REQUIRE(d->n_rows >= 1 && d->n_rows < (1L << 31), RV_ERR_SHAPE,
             "rv_mosaic(SWITCH_MOMENTS): n_rows=%ld (the files) outside [1, 2^31)", d->n_rows);
  RV_REQUIRE(d->row_start, RV_ERR_NULL, "rv_mosaic(SWITCH_MOMENTS): row_start is null");
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(SWITCH_MOMENTS): moment (the residual block) is null");
  RV_REQUIRE(((uintptr_t)d->moment & 255) == 0, RV_ERR_SHAPE, "rv_mosaic(SWITCH_MOMENTS): moment is not 256-byte aligned");
  RV_REQUIRE(d->state, RV_ERR_NULL, "rv_mosaic(SWITCH_MOMENTS): state (gamma) is null");
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(SWITCH_MOMENTS): result (the moments) is null");
  const switch_ws w = switch_layout(d->T, d->S);
  RV_REQUIRE(d->ws_bytes >= w.bytes, RV_ERR_SHAPE, "rv_mosaic(SWITCH_MOMENTS): ws_bytes=%ld, T=%ld frames of S=%ld states need %ld",
             d->ws_bytes, d->T, d->S, w.bytes);
  RV_REQUIRE(d->ws, RV_ERR_NULL, "rv_mosaic(SWITCH_MOMENTS): ws is null, T=%ld frames of S=%ld states need %ld bytes", d->T, d->S,
             w.bytes);
  RV_REQUIRE(((uintptr_t)d->ws & 255) == 0, RV_ERR_SHAPE, "rv_mosaic(SWITCH_MOMENTS): ws is not 256-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  const int S = (int)d->S, k = (int)d->k;
  const double* const r = d->moment;
  const unsigned char* const obs = (const unsigned char*)d->moment + up256(d->T * d->k * (long)sizeof(double));
  const double* const gamma = d->state;
  unsigned char* const keep = (unsigned char*)d->ws;
  double* const npart = (double*)(keep + w.keep);
  double* const part = (double*)(keep + w.keep + w.npart);
  hipLaunchKernelGGL(k_switch_keep, dim3(blocks256(w.n_pairs)), dim3(256), 0, st, d->row_start, d->n_rows, obs, w.n_pairs, keep);
  hipLaunchKernelGGL(k_switch_occupancy, dim3((unsigned)w.nb, 1), dim3(mom::THREADS), 0, st, gamma, (const unsigned char*)keep,
                     w.n_pairs, d->S, npart);
  hipLaunchKernelGGL(k_switch_moments, dim3((unsigned)w.n_ranges, (unsigned)(S + 2)), dim3(mom::TILE_THREADS), 0, st, gamma, S, r,
                     k, (const unsigned char*)keep, w.n_pairs, part);
  hipLaunchKernelGGL(k_switch_sum, dim3(blocks256(d->S + 2 * d->S * d->k + d->S * d->k * d->k)), dim3(256), 0, st,
                     (const double*)npart, w.nb, (const double*)part, w.n_ranges, S, k, d->result);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_switch_fit(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->mode == RV_SWITCH_DYNAMICS || d->mode == RV_SWITCH_NOISE, RV_ERR_SHAPE,
             "rv_mosaic(SWITCH_FIT): mode=%ld is neither RV_SWITCH_DYNAMICS nor RV_SWITCH_NOISE", d->mode);
  const int rc = switch_shape(d, "SWITCH_FIT");
  if (rc) return rc;
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(SWITCH_FIT): result is null");
  const hipStream_t st = (hipStream_t)stream;
  const int S = (int)d->S, k = (int)d->k;
  const long kk = (long)k * k;
  if (d->mode == RV_SWITCH_DYNAMICS) {
    RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(SWITCH_FIT): moment (the moments) is null");
    RV_REQUIRE(d->info, RV_ERR_NULL, "rv_mosaic(SWITCH_FIT): info is null");
    RV_REQUIRE((const double*)d->result != d->moment, RV_ERR_SHAPE,
               "rv_mosaic(SWITCH_FIT): result and moment are the same block; [A | Q] needs its own");
    hipLaunchKernelGGL(k_switch_dynamics, dim3(blocks256(S * kk)), dim3(256), 0, st, d->moment, S, k, d->result, d->info);
    hipLaunchKernelGGL(k_switch_gram, dim3(blocks256(kk), (unsigned)S), dim3(256), 0, st, (const double*)d->result, k,
                       d->result + S * kk);
  } else {
    RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(SWITCH_FIT): basis (A) is null");
    RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(SWITCH_FIT): moment (the eigenvectors of Q) is null");
    RV_REQUIRE(d->eigenvalues, RV_ERR_NULL, "rv_mosaic(SWITCH_FIT): the eigenvalues of Q are null");
    hipLaunchKernelGGL(k_switch_noise, dim3(blocks256(kk), (unsigned)S), dim3(256), 0, st, (const double*)d->basis, d->moment,
                       (const double*)d->eigenvalues, k, d->result, d->result + S * 2 * kk);
  }
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_switch_step(const rv_mosaic_desc* d, void* stream) {
  const rv_stream_desc* sd = d->live;
  RV_REQUIRE(sd, RV_ERR_NULL, "rv_mosaic(SWITCH_STEP): the stream (live) is null");
  const int rc0 = switch_shape(d, "SWITCH_STEP");
  if (rc0) return rc0;
  RV_REQUIRE(d->L >= d->k && d->L <= SW_LMAX, RV_ERR_SHAPE, "rv_mosaic(SWITCH_STEP): L=%ld outside [k=%ld, %d]", d->L, d->k, SW_LMAX);
  RV_REQUIRE(d->L == sd->L, RV_ERR_SHAPE, "rv_mosaic(SWITCH_STEP): L=%ld, the stream's model has L=%ld", d->L, sd->L);
  RV_REQUIRE(d->centre, RV_ERR_NULL, "rv_mosaic(SWITCH_STEP): centre is null");
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(SWITCH_STEP): basis (R) is null");
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(SWITCH_STEP): moment (phi) is null");
  RV_REQUIRE(d->state, RV_ERR_NULL, "rv_mosaic(SWITCH_STEP): the state is null");
  RV_REQUIRE(d->primed, RV_ERR_NULL, "rv_mosaic(SWITCH_STEP): the primed flags are null");
  RV_REQUIRE(d->idx, RV_ERR_NULL, "rv_mosaic(SWITCH_STEP): idx (the current states) is null");
  RV_REQUIRE(d->path, RV_ERR_NULL, "rv_mosaic(SWITCH_STEP): path (the states out) is null");
  RV_REQUIRE(sd->temperature, RV_ERR_NULL, "rv_mosaic(SWITCH_STEP): live->temperature is null");
  RV_REQUIRE(!d->out || d->ldo >= d->L, RV_ERR_SHAPE, "rv_mosaic(SWITCH_STEP): ldo=%ld holds no row of L=%ld values", d->ldo, d->L);
  float *z = nullptr, *frames = nullptr;
  const int rc = rv_stream_encode(sd, nullptr, &z, &frames, stream);   // the stream's own checks; launches nothing
  if (rc) return rc;
  hipLaunchKernelGGL(k_switch_step, dim3((unsigned)sd->n_streams), dim3(SW_THREADS), 0, (hipStream_t)stream, d->moment,
                     (const double*)d->basis, (const double*)d->centre, (int)d->S, (int)d->k, (int)d->L, sd->block / sd->hop,
                     rv_stream_counters(sd), sd->eps_in, (uint64_t)sd->seed, sd->temperature, sd->offset, d->next_of, d->weight,
                     d->state, d->primed, d->idx, d->path, z, d->out, d->ldo);
  RV_CHECK_LAUNCH();
  return rv_stream_synth(sd, 1, stream);
}
