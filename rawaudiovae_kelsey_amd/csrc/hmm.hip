// Latent states (rawaudiovae_kelsey_amd/states.py): a hidden Markov model with diagonal Gaussian emissions over the
// whitened coordinates y = P (x - c) of a corpus's latent rows.  Five ops of rv_mosaic; the rules, down to the order of
// every sum: include/rawvae_hip.h, "Latent states"; the tiling and the measured figures: DESIGN.md section 7.16.
//   RV_HMM_EMIT              k_hmm_emit: a workgroup per block of 64 frames stages their y in LDS once (sequence.h's
//                            chain, the one RV_SMOOTH_FILTER observes with) and writes logb for all S states.
//   RV_HMM_FORWARD_BACKWARD  k_hmm_fb, one workgroup per sequence: A in LDS for the whole sequence, wave 0 runs the
//                            scaled recursion with lane j owning state j (alpha and u pass between lanes through
//                            LDS), all four waves accumulate xi in registers, 16 columns of a row per thread.
//   RV_HMM_MSTEP             k_hmm_observe (y and the observed flags to ws), k_hmm_occupancy (moment.h's blocked
//                            column sum of gamma), k_hmm_moments (moment.h's MFMA tile in its two-operand form: gamma^T y
//                            and gamma^T (y o y), a workgroup per range of 4096 frames and product), k_hmm_close (ONE
//                            workgroup: the range sums, the divisions, g, pi, A and the logarithms).
//   RV_HMM_VITERBI           k_hmm_viterbi, one wave per sequence: max-plus in fp64, log A in LDS, byte back-pointers.
//   RV_HMM_WORKSPACE         the bytes of ws.
// No atomics, no polling; every output element is written by exactly one thread.
#include <math.h>

#include "common.h"
#include "internal.h"
#include "moment.h"
#include "sequence.h"

using namespace rv;

namespace {

constexpr int HM_SMAX = 64;       // states: one wave holds a vector over the states (the header states it)
constexpr int HM_KMAX = 64;       // axes: one 64 x 64 tile holds a weighted moment
constexpr int HM_LMAX = 512;
constexpr int HM_THREADS = seq::THREADS;
constexpr int HM_FRAMES = seq::FRAMES;   // frames of one workgroup of k_hmm_emit / k_hmm_observe (the header states it)
constexpr int HM_PITCH = seq::PITCH;
constexpr int HM_NONE = 255;      // back-pointer: no predecessor with a score above -inf
constexpr double LOG_2PI = 1.8378770664093453;   // fl64(log(2 pi))

// one rounding each, never contracted into an fma
__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double add_rn(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// the parts of theta = [m (S k) | w (S k) | g (S) | pi (S) | A (S S) | log pi (S) | log A (S S)]
struct theta_at {
  long m, w, g, pi, A, logpi, logA, doubles;
};
__host__ __device__ __forceinline__ theta_at theta_layout(long S, long k) {
  theta_at o;
  o.m = 0;
  o.w = S * k;
  o.g = 2 * S * k;
  o.pi = o.g + S;
  o.A = o.pi + S;
  o.logpi = o.A + S * S;
  o.logA = o.logpi + S;
  o.doubles = o.logA + S * S;
  return o;
}

// logb[t, s] = g_s - 0.5 q, q = chain fma(fl(w_sj d), d, .), d = y_j - m_sj, in ascending j from +0; a row of NaN for a
// frame whose x row is not finite
__global__ void __launch_bounds__(HM_THREADS)
k_hmm_emit(const float* __restrict__ x, long ldx, const double* __restrict__ centre, const double* __restrict__ P,
           const double* __restrict__ theta, long T, int L, int k, int S, double* __restrict__ logb) {
  __shared__ double sy[HM_FRAMES * HM_PITCH];
  __shared__ unsigned char sflag[HM_THREADS], sbad[HM_FRAMES];
  const long t0 = (long)blockIdx.x * HM_FRAMES;
  const int nf = T - t0 < HM_FRAMES ? (int)(T - t0) : HM_FRAMES;
  seq::stage_frames(x, ldx, centre, P, t0, nf, L, k, sy, sflag, sbad);
  const theta_at o = theta_layout(S, k);
  for (int e = threadIdx.x; e < nf * S; e += HM_THREADS) {
    const int f = e / S, s = e - f * S;
    double v = __builtin_nan("");
    if (!sbad[f]) {
      const double* const m = theta + o.m + (long)s * k;
      const double* const w = theta + o.w + (long)s * k;
      const double* const y = sy + f * HM_PITCH;
      double q = 0.0;
      for (int j = 0; j < k; ++j) {
        const double d = y[j] - m[j];
        q = __builtin_fma(mul_rn(w[j], d), d, q);
      }
      v = add_rn(theta[o.g + s], -mul_rn(0.5, q));
    }
    logb[t0 * S + e] = v;
  }
}

// y [T, k] and obs [T] (1: the frame's x row is finite) for RV_HMM_MSTEP
__global__ void __launch_bounds__(HM_THREADS)
k_hmm_observe(const float* __restrict__ x, long ldx, const double* __restrict__ centre, const double* __restrict__ P, long T,
              int L, int k, double* __restrict__ ys, unsigned char* __restrict__ obs) {
  __shared__ double sy[HM_FRAMES * HM_PITCH];
  __shared__ unsigned char sflag[HM_THREADS], sbad[HM_FRAMES];
  const long t0 = (long)blockIdx.x * HM_FRAMES;
  const int nf = T - t0 < HM_FRAMES ? (int)(T - t0) : HM_FRAMES;
  seq::stage_frames(x, ldx, centre, P, t0, nf, L, k, sy, sflag, sbad);
  for (int e = threadIdx.x; e < nf * k; e += HM_THREADS) {
    const int f = e / k, j = e - f * k;
    ys[t0 * k + e] = sy[f * HM_PITCH + j];
  }
  if (threadIdx.x < nf) obs[t0 + threadIdx.x] = !sbad[threadIdx.x];
}

// Wave 0's view of frame t: lane j < S holds logb[t, j].  unobserved (any NaN in the row): M = 0 and b~ = 1; else
// M = max_s logb[t, s] and b~ = exp(logb[t, j] - M).  Lanes >= S: b~ = 0.
__device__ __forceinline__ void frame_scale(const double* __restrict__ logb, long t, int S, int lane, double& M, double& bt,
                                            double& lb, bool& unobs) {
  const bool in = lane < S;
  lb = in ? logb[t * S + lane] : -INFINITY;
  unobs = __ballot(in && lb != lb) != 0;
  double m = lb;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
  M = unobs ? 0.0 : m;
  bt = !in ? 0.0 : (unobs ? 1.0 : exp(lb - m));
}

// One workgroup per sequence.  LDS: A (pitch S | 1: a row's and a column's elements fall into different banks), the
// normalised alpha of the frame before, the unnormalised one, u.
__global__ void __launch_bounds__(HM_THREADS)
k_hmm_fb(const double* __restrict__ logb, const long long* __restrict__ row_start, const double* __restrict__ theta, long T,
         int S, int k, double* __restrict__ alphas, double* __restrict__ cs, double* __restrict__ gamma,
         double* __restrict__ xi, double* __restrict__ ll) {
  __shared__ double sA[HM_SMAX * HM_PITCH];
  __shared__ double salpha[HM_SMAX], sun[HM_SMAX], su[HM_SMAX];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, SP = S | 1;
  const bool in = lane < S;
  const theta_at o = theta_layout(S, k);
  for (int e = tid; e < S * S; e += HM_THREADS) {
    const int i = e / S, j = e - i * S;
    sA[i * SP + j] = theta[o.A + e];
  }
  long t0, t1;
  seq::rows_of(row_start, blockIdx.x, T, t0, t1);
  double llacc = 0.0, a = 0.0;
  __syncthreads();
  for (long t = t0; t < t1; ++t) {
    double M = 0.0;
    if (wv == 0) {
      double bt, lb;
      bool unobs;
      frame_scale(logb, t, S, lane, M, bt, lb, unobs);
      if (in) {
        if (t == t0) {
          a = mul_rn(theta[o.pi + lane], bt);
        } else {
          double acc = 0.0;
          for (int i = 0; i < S; ++i) acc = __builtin_fma(salpha[i], sA[i * SP + lane], acc);
          a = mul_rn(bt, acc);
        }
        sun[lane] = a;
      }
    }
    __syncthreads();
    if (wv == 0) {
      double c = 0.0;
      for (int j = 0; j < S; ++j) c += sun[j];
      a = a / c;
      if (in) {
        salpha[lane] = a;
        alphas[t * S + lane] = a;
      }
      if (lane == 0) {
        cs[t] = c;
        llacc = add_rn(llacc, add_rn(log(c), M));
      }
    }
    __syncthreads();
  }
  // backward: beta_{t1 - 1} = 1; thread (i = lane, wv) accumulates xi[i, 16 wv .. 16 wv + 15]
  double beta = 1.0;
  double acc[16];
#pragma unroll
  for (int jj = 0; jj < 16; ++jj) acc[jj] = 0.0;
  if (wv == 0 && in && t1 > t0) gamma[(t1 - 1) * S + lane] = mul_rn(a, beta);
  for (long t = t1 - 2; t >= t0; --t) {
    if (wv == 0) {
      double M, bt, lb;
      bool unobs;
      frame_scale(logb, t + 1, S, lane, M, bt, lb, unobs);
      if (in) su[lane] = mul_rn(bt, beta) / cs[t + 1];
    }
    __syncthreads();
    const double ai = in ? alphas[t * S + lane] : 0.0;
    if (wv == 0 && in) {
      double nb = 0.0;
      for (int j = 0; j < S; ++j) nb = __builtin_fma(sA[lane * SP + j], su[j], nb);
      beta = nb;
      gamma[t * S + lane] = mul_rn(ai, beta);
    }
    if (in) {
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int j = wv * 16 + jj;
        if (j < S) acc[jj] = __builtin_fma(mul_rn(ai, sA[lane * SP + j]), su[j], acc[jj]);
      }
    }
    __syncthreads();
  }
  if (in) {
    double* const xr = xi + ((long)blockIdx.x * S + lane) * S;
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
      const int j = wv * 16 + jj;
      if (j < S) xr[j] = acc[jj];
    }
  }
  if (tid == 0) ll[blockIdx.x] = llacc;
}

// One wave per sequence, lane j owns state j.  (v, i) wins over the best so far only when v is larger: ascending i, so
// ties go to the lower i, and NaN and -inf never win.
__global__ void __launch_bounds__(WAVE)
k_hmm_viterbi(const double* __restrict__ logb, const long long* __restrict__ row_start, const double* __restrict__ theta,
              long T, int S, int k, unsigned char* __restrict__ back, int* __restrict__ path, double* __restrict__ score) {
  __shared__ double slA[HM_SMAX * HM_PITCH];
  __shared__ double sd[HM_SMAX];
  const int lane = threadIdx.x, SP = S | 1;
  const bool in = lane < S;
  const theta_at o = theta_layout(S, k);
  for (int e = lane; e < S * S; e += WAVE) {
    const int i = e / S, j = e - i * S;
    slA[i * SP + j] = theta[o.logA + e];
  }
  long t0, t1;
  seq::rows_of(row_start, blockIdx.x, T, t0, t1);
  for (long t = t0; t < t1; ++t) {
    double M, bt, lb;
    bool unobs;
    frame_scale(logb, t, S, lane, M, bt, lb, unobs);
    const double add = unobs ? 0.0 : lb;
    double d = -INFINITY;
    if (in) {
      if (t == t0) {
        d = add_rn(add, theta[o.logpi + lane]);
      } else {
        double best = -INFINITY;
        int bi = HM_NONE;
        for (int i = 0; i < S; ++i) {
          const double v = add_rn(sd[i], slA[i * SP + lane]);
          if (v > best) {
            best = v;
            bi = i;
          }
        }
        d = add_rn(add, best);
        back[t * S + lane] = (unsigned char)bi;
      }
    }
    __syncthreads();   // every lane has read the scores of the frame before
    if (in) sd[lane] = d;
    __syncthreads();
  }
  if (lane != 0) return;
  double best = -INFINITY;
  int e = HM_NONE;
  for (int j = 0; j < S && t1 > t0; ++j) {
    if (sd[j] > best) {
      best = sd[j];
      e = j;
    }
  }
  score[blockIdx.x] = t1 > t0 ? best : 0.0;
  for (long t = t1 - 1; t >= t0; --t) {
    path[t] = e < S ? e : -1;
    if (t > t0 && e < S) e = back[t * S + e];
  }
}

// npart[b, s] = the gamma[t, s] of the observed frames of block b in ascending t from +0
__global__ void __launch_bounds__(mom::THREADS)
k_hmm_occupancy(const double* __restrict__ gamma, const unsigned char* __restrict__ obs, long T, long S,
                double* __restrict__ npart) {
  mom::colsum_block([=](long t, long j) { return obs[t] ? gamma[t * S + j] : 0.0; }, T, S, npart);
}

// Grid (ranges, 2): tile 0 of a range is gamma^T y, tile 1 gamma^T (y o y)
__global__ void __launch_bounds__(mom::TILE_THREADS)
k_hmm_moments(const double* __restrict__ gamma, int S, const double* __restrict__ ys, int k, long T,
              double* __restrict__ part) {
  __shared__ double As[mom::STAGE];
  __shared__ double Bs[mom::STAGE];
  if (blockIdx.y == 0) mom::weighted_tile<false>(As, Bs, gamma, S, ys, k, T, 2, part);
  else mom::weighted_tile<true>(As, Bs, gamma, S, ys, k, T, 2, part);
}

// p[0], p[step], .. (n terms) in ascending order from +0, eight loads in flight
__device__ __forceinline__ double ascending_sum(const double* __restrict__ p, long n, long step) {
  double acc = 0.0;
  long b = 0;
  for (; b + 8 <= n; b += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = p[(b + i) * step];
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += v[i];
  }
  for (; b < n; ++b) acc += p[b * step];
  return acc;
}

// ONE workgroup: the closing steps of the M-step.  sbuf holds the variances [S, k], then A's numerators [S, S].
__global__ void __launch_bounds__(HM_THREADS)
k_hmm_close(const double* __restrict__ npart, long nb, const double* __restrict__ part, long n_ranges,
            const double* __restrict__ gamma, const double* __restrict__ xi, const long long* __restrict__ row_start,
            long n_rows, long T, int S, int k, double floor_v, const double* __restrict__ old, double* __restrict__ neu,
            int* __restrict__ info, double* __restrict__ moments) {
  __shared__ double sbuf[HM_SMAX * HM_SMAX];
  __shared__ double sN[HM_SMAX], srow[HM_SMAX];
  const int tid = threadIdx.x;
  const theta_at o = theta_layout(S, k);
  if (tid < S) sN[tid] = mom::colsum_total(npart, nb, S, tid);
  __syncthreads();
  for (int e = tid; e < S * k; e += HM_THREADS) {
    const int s = e / k, j = e - s * k;
    const double N = sN[s];
    const double m1 = mom::range_sum(part, n_ranges, 2, 0, s, j), m2 = mom::range_sum(part, n_ranges, 2, 1, s, j);
    if (moments) {
      double* const row = moments + (long)s * (1 + 2 * k);
      if (j == 0) row[0] = N;
      row[1 + j] = m1;
      row[1 + k + j] = m2;
    }
    if (!(N >= 1.0)) {   // a dead state keeps its emission
      neu[o.m + e] = old[o.m + e];
      neu[o.w + e] = old[o.w + e];
      continue;
    }
    const double m = m1 / N;
    const double raw = add_rn(m2 / N, -mul_rn(m, m));
    const double v = raw > floor_v ? raw : floor_v;
    neu[o.m + e] = m;
    neu[o.w + e] = 1.0 / v;
    sbuf[e] = v;
  }
  __syncthreads();
  if (tid < S) {
    const bool dead = !(sN[tid] >= 1.0);
    double g = old[o.g + tid];
    if (!dead) {
      double acc = 0.0;
      for (int j = 0; j < k; ++j) acc += log(sbuf[tid * k + j]);
      g = mul_rn(-0.5, add_rn(mul_rn((double)k, LOG_2PI), acc));
    }
    neu[o.g + tid] = g;
    info[tid] = dead;
    // the first frame's gamma of every sequence that has one, in ascending sequence order from +0
    double acc = 0.0;
    long n = 0;
    for (long s = 0; s < n_rows; ++s) {
      long t0, t1;
      seq::rows_of(row_start, s, T, t0, t1);
      if (t1 > t0) {
        acc += gamma[t0 * S + tid];
        ++n;
      }
    }
    const double p = n ? acc / (double)n : old[o.pi + tid];
    neu[o.pi + tid] = p;
    neu[o.logpi + tid] = log(p);
  }
  __syncthreads();
  for (int e = tid; e < S * S; e += HM_THREADS) sbuf[e] = ascending_sum(xi + e, n_rows, (long)S * S);
  __syncthreads();
  if (tid < S) {
    double acc = 0.0;
    for (int j = 0; j < S; ++j) acc += sbuf[tid * S + j];
    srow[tid] = acc;
  }
  __syncthreads();
  for (int e = tid; e < S * S; e += HM_THREADS) {
    const double rs = srow[e / S];
    const double a = rs > 0.0 ? sbuf[e] / rs : old[o.A + e];
    neu[o.A + e] = a;
    neu[o.logA + e] = log(a);
  }
}

// ws, every part on a 256-byte boundary.  FORWARD_BACKWARD: [alpha (T S) | c (T)].  VITERBI: [back (T S) bytes].
// MSTEP: [y (T k) | obs (T) bytes | the occupancy's block sums (nb S) | the partial tiles (n_ranges 2 64 64)].
struct hmm_ws {
  long alpha, fb, vit, y, obs, nb, npart, n_ranges, mstep, bytes;
};

hmm_ws hmm_layout(long T, long S, long k) {
  hmm_ws w;
  const long D = (long)sizeof(double);
  w.alpha = up256(T * S * D);
  w.fb = w.alpha + up256(T * D);
  w.vit = up256(T * S);
  w.y = up256(T * k * D);
  w.obs = up256(T);
  w.nb = (T + mom::ROWS - 1) / mom::ROWS;
  w.npart = up256(w.nb * S * D);
  w.n_ranges = (T + mom::RANGE - 1) / mom::RANGE;
  w.mstep = w.y + w.obs + w.npart + w.n_ranges * 2 * (long)mom::TILE * D;
  w.bytes = w.fb > w.vit ? w.fb : w.vit;
  w.bytes = w.mstep > w.bytes ? w.mstep : w.bytes;
  return w;
}

// the checks every op shares: T, S, k
int hmm_shape(const rv_mosaic_desc* d, const char* op) {
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): T=%ld outside [1, 2^31)", op, d->T);
  RV_REQUIRE(d->S >= 1 && d->S <= HM_SMAX, RV_ERR_SHAPE, "rv_mosaic(%s): S=%ld (the states) outside [1, %d]", op, d->S, HM_SMAX);
  RV_REQUIRE(d->k >= 1 && d->k <= HM_KMAX, RV_ERR_SHAPE, "rv_mosaic(%s): k=%ld (the axes) outside [1, %d]", op, d->k, HM_KMAX);
  return RV_OK;
}

// ... of the two ops that read the latent rows: L, stride, q, centre, basis
int hmm_rows(const rv_mosaic_desc* d, const char* op) {
  RV_REQUIRE(d->L >= d->k && d->L <= HM_LMAX, RV_ERR_SHAPE, "rv_mosaic(%s): L=%ld outside [k=%ld, %d]", op, d->L, d->k, HM_LMAX);
  RV_REQUIRE(d->stride >= d->L, RV_ERR_SHAPE, "rv_mosaic(%s): stride=%ld (the row pitch of x) holds no row of L=%ld values", op,
             d->stride, d->L);
  RV_REQUIRE(d->q, RV_ERR_NULL, "rv_mosaic(%s): q (the latent rows x) is null", op);
  RV_REQUIRE(d->centre, RV_ERR_NULL, "rv_mosaic(%s): centre is null", op);
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(%s): basis (P) is null", op);
  return RV_OK;
}

// ... of the three ops over sequences: n_rows, row_start, ws
int hmm_sequences(const rv_mosaic_desc* d, const char* op, long need) {
  RV_REQUIRE(d->n_rows >= 1 && d->n_rows < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): n_rows=%ld (the sequences) outside [1, 2^31)",
             op, d->n_rows);
  RV_REQUIRE(d->row_start, RV_ERR_NULL, "rv_mosaic(%s): row_start is null", op);
  RV_REQUIRE(d->ws_bytes >= need, RV_ERR_SHAPE, "rv_mosaic(%s): ws_bytes=%ld, T=%ld frames of S=%ld states and k=%ld axes need %ld",
             op, d->ws_bytes, d->T, d->S, d->k, need);
  RV_REQUIRE(d->ws, RV_ERR_NULL, "rv_mosaic(%s): ws is null, T=%ld frames of S=%ld states and k=%ld axes need %ld bytes", op, d->T,
             d->S, d->k, need);
  RV_REQUIRE(((uintptr_t)d->ws & 255) == 0, RV_ERR_SHAPE, "rv_mosaic(%s): ws is not 256-byte aligned", op);
  return RV_OK;
}

// state = the posteriors, one block: [gamma (T S) | xi (n_rows S S) | ll (n_rows)]
struct posteriors {
  double *gamma, *xi, *ll;
};
posteriors posteriors_of(const rv_mosaic_desc* d) {
  posteriors p;
  p.gamma = d->state;
  p.xi = p.gamma + d->T * d->S;
  p.ll = p.xi + d->n_rows * d->S * d->S;
  return p;
}

unsigned frame_blocks(long T) { return (unsigned)((T + HM_FRAMES - 1) / HM_FRAMES); }

}  // namespace

int rv_hmm_workspace(rv_mosaic_desc* d) {
  const int rc = hmm_shape(d, "HMM_WORKSPACE");
  if (rc) return rc;
  d->ws_bytes = hmm_layout(d->T, d->S, d->k).bytes;
  return RV_OK;
}

int rv_hmm_emit(const rv_mosaic_desc* d, void* stream) {
  int rc = hmm_shape(d, "HMM_EMIT");
  if (rc) return rc;
  rc = hmm_rows(d, "HMM_EMIT");
  if (rc) return rc;
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(HMM_EMIT): moment (theta) is null");
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(HMM_EMIT): result (logb) is null");
  hipLaunchKernelGGL(k_hmm_emit, dim3(frame_blocks(d->T)), dim3(HM_THREADS), 0, (hipStream_t)stream, d->q, d->stride,
                     (const double*)d->centre, (const double*)d->basis, d->moment, d->T, (int)d->L, (int)d->k, (int)d->S, d->result);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_hmm_forward_backward(const rv_mosaic_desc* d, void* stream) {
  int rc = hmm_shape(d, "HMM_FORWARD_BACKWARD");
  if (rc) return rc;
  const hmm_ws w = hmm_layout(d->T, d->S, d->k);
  rc = hmm_sequences(d, "HMM_FORWARD_BACKWARD", w.fb);
  if (rc) return rc;
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(HMM_FORWARD_BACKWARD): result (logb) is null");
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(HMM_FORWARD_BACKWARD): moment (theta) is null");
  RV_REQUIRE(d->state, RV_ERR_NULL, "rv_mosaic(HMM_FORWARD_BACKWARD): state (the posteriors) is null");
  const posteriors p = posteriors_of(d);
  double* const alphas = (double*)d->ws;
  double* const cs = (double*)((char*)d->ws + w.alpha);
  hipLaunchKernelGGL(k_hmm_fb, dim3((unsigned)d->n_rows), dim3(HM_THREADS), 0, (hipStream_t)stream, (const double*)d->result,
                     d->row_start, d->moment, d->T, (int)d->S, (int)d->k, alphas, cs, p.gamma, p.xi, p.ll);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_hmm_viterbi(const rv_mosaic_desc* d, void* stream) {
  int rc = hmm_shape(d, "HMM_VITERBI");
  if (rc) return rc;
  const hmm_ws w = hmm_layout(d->T, d->S, d->k);
  rc = hmm_sequences(d, "HMM_VITERBI", w.vit);
  if (rc) return rc;
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(HMM_VITERBI): result (logb) is null");
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(HMM_VITERBI): moment (theta) is null");
  RV_REQUIRE(d->path, RV_ERR_NULL, "rv_mosaic(HMM_VITERBI): path is null");
  RV_REQUIRE(d->score, RV_ERR_NULL, "rv_mosaic(HMM_VITERBI): score is null");
  hipLaunchKernelGGL(k_hmm_viterbi, dim3((unsigned)d->n_rows), dim3(WAVE), 0, (hipStream_t)stream, (const double*)d->result,
                     d->row_start, d->moment, d->T, (int)d->S, (int)d->k, (unsigned char*)d->ws, d->path, d->score);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_hmm_mstep(const rv_mosaic_desc* d, void* stream) {
  int rc = hmm_shape(d, "HMM_MSTEP");
  if (rc) return rc;
  rc = hmm_rows(d, "HMM_MSTEP");
  if (rc) return rc;
  const hmm_ws w = hmm_layout(d->T, d->S, d->k);
  rc = hmm_sequences(d, "HMM_MSTEP", w.mstep);
  if (rc) return rc;
  RV_REQUIRE(isfinite(d->lam) && d->lam > 0.f, RV_ERR_SHAPE,
             "rv_mosaic(HMM_MSTEP): lam=%g (the variance floor) must be finite and positive", (double)d->lam);
  RV_REQUIRE(d->mode == 0 || d->mode == RV_HMM_MOMENTS, RV_ERR_SHAPE, "rv_mosaic(HMM_MSTEP): mode=%ld is neither 0 nor RV_HMM_MOMENTS",
             d->mode);
  RV_REQUIRE(d->state, RV_ERR_NULL, "rv_mosaic(HMM_MSTEP): state (the posteriors) is null");
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(HMM_MSTEP): moment (the old theta) is null");
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(HMM_MSTEP): result (the new theta) is null");
  RV_REQUIRE((const double*)d->result != d->moment, RV_ERR_SHAPE,
             "rv_mosaic(HMM_MSTEP): result and moment are the same block; the new theta needs its own");
  const posteriors p = posteriors_of(d);
  double* const moments = d->mode == RV_HMM_MOMENTS ? d->result + theta_layout(d->S, d->k).doubles : nullptr;
  RV_REQUIRE(d->info, RV_ERR_NULL, "rv_mosaic(HMM_MSTEP): info is null");
  const hipStream_t st = (hipStream_t)stream;
  const int S = (int)d->S, k = (int)d->k;
  double* const ys = (double*)d->ws;
  unsigned char* const obs = (unsigned char*)d->ws + w.y;
  double* const npart = (double*)((char*)d->ws + w.y + w.obs);
  double* const part = (double*)((char*)d->ws + w.y + w.obs + w.npart);
  hipLaunchKernelGGL(k_hmm_observe, dim3(frame_blocks(d->T)), dim3(HM_THREADS), 0, st, d->q, d->stride, (const double*)d->centre,
                     (const double*)d->basis, d->T, (int)d->L, k, ys, obs);
  hipLaunchKernelGGL(k_hmm_occupancy, dim3((unsigned)w.nb, 1), dim3(mom::THREADS), 0, st, (const double*)p.gamma,
                     (const unsigned char*)obs, d->T, d->S, npart);
  hipLaunchKernelGGL(k_hmm_moments, dim3((unsigned)w.n_ranges, 2), dim3(mom::TILE_THREADS), 0, st, (const double*)p.gamma, S,
                     (const double*)ys, k, d->T, part);
  hipLaunchKernelGGL(k_hmm_close, dim3(1), dim3(HM_THREADS), 0, st, (const double*)npart, w.nb, (const double*)part, w.n_ranges,
                     (const double*)p.gamma, (const double*)p.xi, d->row_start, d->n_rows, d->T, S, k, (double)d->lam, d->moment,
                     d->result, d->info, moments);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
