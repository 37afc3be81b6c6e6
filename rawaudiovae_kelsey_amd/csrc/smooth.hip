// Latent restoration (rawaudiovae_kelsey_amd/smooth.py): inference with the latent walk's model w' = A w + B e.  A Kalman
// filter and a fixed-interval smoother (modified Bryson-Frazier) over sequences of latent rows whose frames are partly
// missing, and the splice of a resynthesis into the original.  Four ops of rv_mosaic; the rules: include/rawvae_hip.h,
// "Latent restoration"; the derivation and the measured figures: DESIGN.md section 7.14.
//   RV_SMOOTH_FILTER    k_smooth_qn (Qn = B B^T, dense mode), k_smooth_observe (y_t = P (x_t - c), a thread per frame
//                       and axis), then one workgroup per sequence: k_smooth_filter (dense: P, A and the factor in
//                       LDS) or k_smooth_filter_diag (a thread per axis, no barrier) and k_smooth_diag_sums.
//   RV_SMOOTH_BACKWARD  one workgroup per sequence in descending t: k_smooth_backward (the two triangular solves in
//                       one wave, the running vector passed by lane) or k_smooth_backward_diag; then k_smooth_rows, a
//                       workgroup per frame, writes the latent rows.
//   RV_SMOOTH_SPLICE    k_smooth_splice, a thread per sample.
//   RV_SMOOTH_WORKSPACE the bytes of ws.
// Every sum is a fixed sequence of fp64 fmas (dot4: four interleaved chains added as (a0 + a1) + (a2 + a3)), so a
// sequence's bits depend on its own rows, weights and the model only.  No atomics, no polling.
#include <math.h>

#include "common.h"
#include "internal.h"
#include "sequence.h"

using namespace rv;

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_KDENSE = 64;            // dense mode: one wave holds a vector of the state (the header states it)
constexpr int SM_LMAX = 512;
constexpr double SM_LAM_MIN = 1e-8, SM_LAM_MAX = 1e8;

// sum_m p[m sp] q[m sq] over m in [0, n): four chains over m mod 4 in ascending m from +0, then (a0 + a1) + (a2 + a3)
__device__ __forceinline__ double dot4(const double* p, int sp, const double* q, int sq, int n) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  int m = 0;
  for (; m + 4 <= n; m += 4) {
    a0 = __builtin_fma(p[(m + 0) * sp], q[(m + 0) * sq], a0);
    a1 = __builtin_fma(p[(m + 1) * sp], q[(m + 1) * sq], a1);
    a2 = __builtin_fma(p[(m + 2) * sp], q[(m + 2) * sq], a2);
    a3 = __builtin_fma(p[(m + 3) * sp], q[(m + 3) * sq], a3);
  }
  if (m < n) a0 = __builtin_fma(p[m * sp], q[m * sq], a0);
  if (m + 1 < n) a1 = __builtin_fma(p[(m + 1) * sp], q[(m + 1) * sq], a1);
  if (m + 2 < n) a2 = __builtin_fma(p[(m + 2) * sp], q[(m + 2) * sq], a2);
  return (a0 + a1) + (a2 + a3);
}

// frame t is observed iff weight[t] > 0 (NaN, 0 and negative: missing); weight NULL: every frame, weight 1
__device__ __forceinline__ bool observed(const float* __restrict__ weight, long t) { return !weight || weight[t] > 0.f; }

__device__ __forceinline__ double noise_at(const float* __restrict__ weight, float lam, long t) {
  return weight ? (double)lam / (double)weight[t] : (double)lam;
}

using seq::rows_of;   // the sequence's rows, clamped to [0, T] (sequence.h)

// Qn = B B^T from B^T [k, k]: element (i, j), i <= j, one ascending chain, written to [i, j] and [j, i]
__global__ void __launch_bounds__(256)
k_smooth_qn(const double* __restrict__ Bt, int k, double* __restrict__ qn) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)k * k) return;
  const int i = (int)(e / k), j = (int)(e - (long)i * k);
  if (i > j) return;
  double acc = 0.0;
  for (int m = 0; m < k; ++m) acc = __builtin_fma(Bt[(long)m * k + i], Bt[(long)m * k + j], acc);
  qn[(long)i * k + j] = acc;
  qn[(long)j * k + i] = acc;
}

// y[t, j] = sum_l P[j, l] ((double)x[t, l] - c[l]) in ascending l from +0; +0 at a missing frame, whose row is not read
__global__ void __launch_bounds__(256)
k_smooth_observe(const float* __restrict__ x, const float* __restrict__ weight, const double* __restrict__ centre,
                 const double* __restrict__ P, long T, int L, int k, double* __restrict__ ys) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= T * k) return;
  const long t = e / k;
  const int j = (int)(e - t * k);
  double acc = 0.0;
  if (observed(weight, t)) acc = seq::whiten_axis(P + (long)j * L, x + t * L, centre, L);
  ys[e] = acc;
}

// Dense filter, one workgroup per sequence.  LDS (pitch kp = k | 1 doubles: the rows of a matrix fall into different
// banks): A, X = the covariance (P+ of the frame before, then P-, then P+), Y = first M = A P+, then the 2 k + 1 rows of
// the factorisation: rows [0, k) G, rows [k, 2 k) W^T = P- G^-T, row 2 k the vector a = G^-1 v.  Row r of Y obeys one
// rule, column after column: Y[r, j] = (base[r, j] - sum_{m < j} Y[r, m] G[j, m]) / G[j, j] with base = S, P- and v.
__global__ void __launch_bounds__(SM_THREADS)
k_smooth_filter(const double* __restrict__ dyn, const double* __restrict__ qn, const float* __restrict__ weight, float lam,
                int k, long T, const long long* __restrict__ row_start, const double* __restrict__ ys,
                double* __restrict__ wms, double* __restrict__ as, double* __restrict__ gds, double* __restrict__ pgs,
                double* __restrict__ result, long ldo) {
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
  const int kp = k | 1, kk = k * k, tid = threadIdx.x;
  double* const sA = (double*)smem_dyn;
  double* const X = sA + k * kp;
  double* const Y = X + k * kp;
  double* const sw = Y + (2 * k + 1) * kp;
  double* const swm = sw + k;
  double* const sv = swm + k;
  double* const sgd = sv + k;
  long t0, t1;
  rows_of(row_start, blockIdx.x, T, t0, t1);
  for (int e = tid; e < kk; e += SM_THREADS) {
    const int m = e / k, i = e - m * k;
    sA[i * kp + m] = dyn[e];   // dyn = A^T: A[i, m] = dyn[m, i]
  }
  for (long t = t0; t < t1; ++t) {
    __syncthreads();   // A is staged; w+ and P+ of the frame before are written and Y is free
    if (t == t0) {
      for (int e = tid; e < kk; e += SM_THREADS) {
        const int i = e / k, j = e - i * k;
        X[i * kp + j] = i == j ? 1.0 : 0.0;
      }
      if (tid < k) swm[tid] = 0.0;
    } else {
      if (tid < k) swm[tid] = dot4(sA + tid * kp, 1, sw, 1, k);
      for (int e = tid; e < kk; e += SM_THREADS) {
        const int i = e / k, j = e - i * k;
        Y[i * kp + j] = dot4(sA + i * kp, 1, X + j, kp, k);
      }
      __syncthreads();
      for (int e = tid; e < kk; e += SM_THREADS) {
        const int i = e / k, j = e - i * k;
        if (i > j) continue;
        const double v = dot4(Y + i * kp, 1, sA + j * kp, 1, k) + qn[e];
        X[i * kp + j] = v;
        X[j * kp + i] = v;
      }
    }
    __syncthreads();
    const bool obs = observed(weight, t);
    double* const pg = pgs + t * kk;
    if (tid < k) wms[t * k + tid] = swm[tid];
    if (!obs) {
      for (int e = tid; e < kk; e += SM_THREADS) {
        const int i = e / k, j = e - i * k;
        pg[e] = X[i * kp + j];
      }
      if (tid < k) {
        sw[tid] = swm[tid];
        if (result) result[t * ldo + tid] = swm[tid];
      }
      if (result && tid == k) result[t * ldo + k] = -1.0;
      if (result && tid == k + 1) result[t * ldo + k + 1] = 0.0;
      continue;
    }
    const double rt = noise_at(weight, lam, t);
    if (tid < k) sv[tid] = ys[t * k + tid] - swm[tid];
    __syncthreads();
    {
      const int r = tid;
      const double* const base = r < k ? X + r * kp : (r < 2 * k ? X + (r - k) * kp : sv);
      for (int j = 0; j < k; ++j) {
        const bool active = r < k ? r >= j : r <= 2 * k;
        double s = 0.0;
        if (active) {
          s = base[j] - dot4(Y + r * kp, 1, Y + j * kp, 1, j);
          if (r == j) {
            s += rt;
            sgd[j] = sqrt(s);
          }
        }
        __syncthreads();
        if (active) Y[r * kp + j] = r == j ? sgd[j] : s / sgd[j];
        __syncthreads();
      }
    }
    const double* const a = Y + 2 * k * kp;
    if (tid < k) {
      as[t * k + tid] = a[tid];
      gds[t * k + tid] = sgd[tid];
      const double wp = swm[tid] + dot4(Y + (k + tid) * kp, 1, a, 1, k);
      sw[tid] = wp;
      if (result) result[t * ldo + tid] = wp;
    } else if (result && tid == k) {
      result[t * ldo + k] = dot4(a, 1, a, 1, k);
    } else if (result && tid == k + 1) {
      double acc = 0.0;
      for (int m = 0; m < k; ++m) acc += log(sgd[m]);
      result[t * ldo + k + 1] = 2.0 * acc;
    }
    for (int e = tid; e < kk; e += SM_THREADS) {
      const int i = e / k, j = e - i * k;
      if (i > j) {
        pg[e] = Y[i * kp + j];
        continue;
      }
      const double pm = X[i * kp + j];
      pg[e] = pm;
      const double v = pm - dot4(Y + (k + i) * kp, 1, Y + (k + j) * kp, 1, k);
      X[i * kp + j] = v;
      X[j * kp + i] = v;
    }
  }
}

// Diagonal filter: thread j runs the scalar filter of axis j over the sequence's frames; nothing is shared.
__global__ void __launch_bounds__(SM_THREADS)
k_smooth_filter_diag(const double* __restrict__ dyn, const float* __restrict__ weight, float lam, int k, long T,
                     const long long* __restrict__ row_start, const double* __restrict__ ys, double* __restrict__ wms,
                     double* __restrict__ us, double* __restrict__ pms, double* __restrict__ ss, double* __restrict__ nis,
                     double* __restrict__ lds, double* __restrict__ result, long ldo) {
  long t0, t1;
  rows_of(row_start, blockIdx.x, T, t0, t1);
  for (int j = threadIdx.x; j < k; j += SM_THREADS) {
    const double a = dyn[(long)j * k + j], b = dyn[(long)k * k + (long)j * k + j];
    const double q = b * b;
    double w = 0.0, p = 1.0;
    for (long t = t0; t < t1; ++t) {
      const double wm = t == t0 ? 0.0 : a * w;
      const double pm = t == t0 ? 1.0 : __builtin_fma(a * p, a, q);
      const long at = t * k + j;
      wms[at] = wm;
      pms[at] = pm;
      if (observed(weight, t)) {
        const double rt = noise_at(weight, lam, t);
        const double s = pm + rt, v = ys[at] - wm;
        const double u = v / s;
        w = __builtin_fma(pm, u, wm);
        p = pm * rt / s;
        us[at] = u;
        ss[at] = s;
        nis[at] = v * u;
        lds[at] = log(s);
      } else {
        w = wm;
        p = pm;
      }
      if (result) result[t * ldo + j] = w;
    }
  }
}

// result[t, k] and [t, k + 1] of the diagonal filter: the axes' terms added in ascending j from +0; -1 and 0 when missing
__global__ void __launch_bounds__(256)
k_smooth_diag_sums(const float* __restrict__ weight, const double* __restrict__ nis, const double* __restrict__ lds, long T,
                   int k, double* __restrict__ result, long ldo) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  double n = -1.0, l = 0.0;
  if (observed(weight, t)) {
    n = 0.0;
    for (int j = 0; j < k; ++j) {
      n += nis[t * k + j];
      l += lds[t * k + j];
    }
  }
  result[t * ldo + k] = n;
  result[t * ldo + k + 1] = l;
}

// sum_m P-[i, m] v[m] from the packed tile (P-'s upper triangle; the strict lower one holds G): P-[i, m] = P-[m, i]
__device__ __forceinline__ double symdot(const double* sG, int kp, int i, const double* v, int k) {
  double a0 = 0.0, a1 = 0.0;
  int m = 0;
  for (; m + 2 <= k; m += 2) {
    a0 = __builtin_fma(i <= m ? sG[i * kp + m] : sG[m * kp + i], v[m], a0);
    a1 = __builtin_fma(i <= m + 1 ? sG[i * kp + m + 1] : sG[(m + 1) * kp + i], v[m + 1], a1);
  }
  if (m < k) a0 = __builtin_fma(i <= m ? sG[i * kp + m] : sG[m * kp + i], v[m], a0);
  return a0 + a1;
}

// Dense backward pass (modified Bryson-Frazier), one workgroup per sequence, descending t.  LDS: A^T, the frame's
// packed tile [P- upper | G strict lower], lambda and lambda-hat.  Wave 0 solves G b = P- lambda and G^T d = a - b with
// lane i owning element i: the pivot's value goes from lane j to every lane, no barrier inside a solve.
__global__ void __launch_bounds__(SM_THREADS)
k_smooth_backward(const double* __restrict__ dyn, const float* __restrict__ weight, int k, long T,
                  const long long* __restrict__ row_start, const double* __restrict__ wms, const double* __restrict__ as,
                  const double* __restrict__ gds, const double* __restrict__ pgs, double* __restrict__ whs,
                  double* __restrict__ state) {
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
  const int kp = k | 1, kk = k * k, tid = threadIdx.x;
  double* const sAt = (double*)smem_dyn;
  double* const sG = sAt + k * kp;
  double* const slam = sG + k * kp;
  double* const slh = slam + k;
  long t0, t1;
  rows_of(row_start, blockIdx.x, T, t0, t1);
  for (int e = tid; e < kk; e += SM_THREADS) {
    const int i = e / k, j = e - i * k;
    sAt[i * kp + j] = dyn[e];
  }
  if (tid < k) slam[tid] = 0.0;
  for (long t = t1 - 1; t >= t0; --t) {
    __syncthreads();   // lambda is written; the tile of the frame after is no longer read
    const double* const pg = pgs + t * kk;
    for (int e = tid; e < kk; e += SM_THREADS) {
      const int i = e / k, j = e - i * k;
      sG[i * kp + j] = pg[e];
    }
    __syncthreads();
    const bool obs = observed(weight, t);
    if (tid < WAVE) {
      const int i = tid;
      const bool in = i < k;
      const double li = in ? slam[i] : 0.0;
      double lh = li;
      if (obs) {
        double p = in ? symdot(sG, kp, i, slam, k) : 0.0;
        const double rg = in ? 1.0 / gds[t * k + i] : 1.0;
        double b = 0.0;
        for (int j = 0; j < k; ++j) {
          const double q = __shfl(p * rg, j, WAVE);
          if (i == j) b = q;
          if (in && i > j) p = __builtin_fma(-sG[i * kp + j], q, p);
        }
        double c = (in ? as[t * k + i] : 0.0) - b;
        double d = 0.0;
        for (int j = k - 1; j >= 0; --j) {
          const double q = __shfl(c * rg, j, WAVE);
          if (i == j) d = q;
          if (i < j) c = __builtin_fma(-sG[j * kp + i], q, c);
        }
        lh = li + d;
      }
      if (in) slh[i] = lh;
    }
    __syncthreads();
    if (tid < k) {
      const double wh = wms[t * k + tid] + symdot(sG, kp, tid, slh, k);
      whs[t * k + tid] = wh;
      if (state) state[t * k + tid] = wh;
      slam[tid] = dot4(sAt + tid * kp, 1, slh, 1, k);   // wave 0 read lambda before the barrier above
    }
  }
}

__global__ void __launch_bounds__(SM_THREADS)
k_smooth_backward_diag(const double* __restrict__ dyn, const float* __restrict__ weight, int k, long T,
                       const long long* __restrict__ row_start, const double* __restrict__ wms,
                       const double* __restrict__ us, const double* __restrict__ pms, const double* __restrict__ ss,
                       double* __restrict__ whs, double* __restrict__ state) {
  long t0, t1;
  rows_of(row_start, blockIdx.x, T, t0, t1);
  for (int j = threadIdx.x; j < k; j += SM_THREADS) {
    const double a = dyn[(long)j * k + j];
    double lam = 0.0;
    for (long t = t1 - 1; t >= t0; --t) {
      const long at = t * k + j;
      const double pm = pms[at];
      double lh = lam;
      if (observed(weight, t)) lh = us[at] + lam - pm * lam / ss[at];
      const double wh = __builtin_fma(pm, lh, wms[at]);
      whs[at] = wh;
      if (state) state[at] = wh;
      lam = a * lh;
    }
  }
}

__device__ __forceinline__ float row_value(double c, double acc, double rho) {
#pragma clang fp contract(off)
  return (float)(c + acc + rho);
}

__device__ __forceinline__ double rho_of(float x, double c, double acc) {
#pragma clang fp contract(off)
  return (double)x - c - acc;
}

// The latent row of frame t = blockIdx.x (grid-stride), a thread per latent l: both sums in ascending j from +0
__global__ void __launch_bounds__(SM_THREADS)
k_smooth_rows(const float* __restrict__ x, const float* __restrict__ weight, const double* __restrict__ centre,
              const double* __restrict__ R, long T, int L, int k, const double* __restrict__ ys,
              const double* __restrict__ whs, float* __restrict__ out, long ldo) {
  __shared__ double sy[SM_LMAX], sw[SM_LMAX];
  for (long t = blockIdx.x; t < T; t += gridDim.x) {
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += SM_THREADS) {
      sy[j] = ys[t * k + j];
      sw[j] = whs[t * k + j];
    }
    __syncthreads();
    const bool obs = observed(weight, t);
    for (int l = threadIdx.x; l < L; l += SM_THREADS) {
      double aw = 0.0, ay = 0.0;
      for (int j = 0; j < k; ++j) {
        const double r = R[(long)j * L + l];
        aw = __builtin_fma(sw[j], r, aw);
        ay = __builtin_fma(sy[j], r, ay);
      }
      const double c = centre[l];
      out[t * ldo + l] = row_value(c, aw, obs ? rho_of(x[t * L + l], c, ay) : 0.0);
    }
  }
}

__device__ __forceinline__ float splice_mix(double g, float a, float b) {
#pragma clang fp contract(off)
  return (float)((1.0 - g) * (double)a + g * (double)b);
}

// d = the distance in samples from n to the nearest range (0 inside): frames where d = 0, src where d > F, else the
// raised cosine g = 0.5 + 0.5 cos(pi d / (F + 1)).  The ranges are ascending and disjoint: the nearest is the first that
// ends beyond n or the one before it.
__global__ void __launch_bounds__(256)
k_smooth_splice(const float* __restrict__ src, const float* __restrict__ frames, const int* __restrict__ room, long n_ranges,
                long F, long n_out, float* __restrict__ out) {
  for (long n = (long)blockIdx.x * 256 + threadIdx.x; n < n_out; n += (long)gridDim.x * 256) {
    long lo = 0, hi = n_ranges;
    while (lo < hi) {
      const long mid = (lo + hi) >> 1;
      if (room[2 * mid + 1] <= n) lo = mid + 1;
      else hi = mid;
    }
    long d = F + 1;
    if (lo < n_ranges) {
      const long s = room[2 * lo];
      d = s <= n ? 0 : s - n;
    }
    if (lo > 0) {
      const long dl = n - room[2 * (lo - 1) + 1] + 1;
      d = dl < d ? dl : d;
    }
    float v;
    if (d <= 0) v = frames[n];
    else if (d > F) v = src[n];
    else v = splice_mix(0.5 + 0.5 * cospi((double)d / (double)(F + 1)), src[n], frames[n]);
    out[n] = v;
  }
}

// ws: [Qn (dense) | y | w- | a (diagonal: u) | w-hat | dense: diag G, the tiles [P- upper | G strict lower]
//                                                     | diagonal: P-, S, the axes' terms of the two sums]
struct smooth_ws {
  long qn, vec, bytes;   // bytes of Qn, doubles of one [T, k] array, bytes in all
  int dense;
  double* at(void* ws, int n) const { return (double*)((char*)ws + qn) + n * vec; }
};

smooth_ws smooth_layout(long T, long k, long mode) {
  smooth_ws w;
  w.dense = mode == RV_SMOOTH_DENSE;
  w.qn = w.dense ? up256(k * k * (long)sizeof(double)) : 0;
  w.vec = T * k;
  w.bytes = up256(w.qn + (w.dense ? 5 + k : 8) * w.vec * (long)sizeof(double));
  return w;
}

// the checks FILTER, BACKWARD and WORKSPACE share: mode, T, L, k
int smooth_shape(const rv_mosaic_desc* d, const char* op) {
  RV_REQUIRE(d->mode == RV_SMOOTH_DENSE || d->mode == RV_SMOOTH_DIAGONAL, RV_ERR_SHAPE,
             "rv_mosaic(%s): mode=%ld is neither RV_SMOOTH_DENSE nor RV_SMOOTH_DIAGONAL", op, d->mode);
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): T=%ld outside [1, 2^31)", op, d->T);
  RV_REQUIRE(d->L >= 1 && d->L <= SM_LMAX, RV_ERR_SHAPE, "rv_mosaic(%s): L=%ld outside [1, %d]", op, d->L, SM_LMAX);
  RV_REQUIRE(d->k >= 1 && d->k <= d->L, RV_ERR_SHAPE, "rv_mosaic(%s): k=%ld outside [1, L=%ld]", op, d->k, d->L);
  RV_REQUIRE(d->mode != RV_SMOOTH_DENSE || d->k <= SM_KDENSE, RV_ERR_SHAPE,
             "rv_mosaic(%s): k=%ld exceeds the dense mode's limit of %d axes (RV_SMOOTH_DIAGONAL takes up to L)", op, d->k,
             SM_KDENSE);
  return RV_OK;
}

// ... and the operands the two passes share
int smooth_operands(const rv_mosaic_desc* d, const char* op, const char* basis, const smooth_ws& w) {
  RV_REQUIRE(d->n_rows >= 1 && d->n_rows <= d->T, RV_ERR_SHAPE, "rv_mosaic(%s): n_rows=%ld (the sequences) outside [1, T=%ld]",
             op, d->n_rows, d->T);
  RV_REQUIRE(isfinite(d->lam) && (double)d->lam >= SM_LAM_MIN && (double)d->lam <= SM_LAM_MAX, RV_ERR_SHAPE,
             "rv_mosaic(%s): lam=%g (the observation noise r) must be finite and in [1e-8, 1e8]", op, (double)d->lam);
  RV_REQUIRE(d->q, RV_ERR_NULL, "rv_mosaic(%s): q (the latent rows x) is null", op);
  RV_REQUIRE(d->row_start, RV_ERR_NULL, "rv_mosaic(%s): row_start is null", op);
  RV_REQUIRE(d->centre, RV_ERR_NULL, "rv_mosaic(%s): centre is null", op);
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(%s): basis (%s) is null", op, basis);
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(%s): moment (the dynamics [A^T | B^T]) is null", op);
  RV_REQUIRE(d->ws_bytes >= w.bytes, RV_ERR_SHAPE, "rv_mosaic(%s): ws_bytes=%ld, T=%ld frames of k=%ld (mode=%ld) need %ld", op,
             d->ws_bytes, d->T, d->k, d->mode, w.bytes);
  RV_REQUIRE(d->ws, RV_ERR_NULL, "rv_mosaic(%s): ws is null, T=%ld frames of k=%ld need %ld bytes", op, d->T, d->k, w.bytes);
  RV_REQUIRE(((uintptr_t)d->ws & 255) == 0, RV_ERR_SHAPE, "rv_mosaic(%s): ws is not 256-byte aligned", op);
  return RV_OK;
}

unsigned blocks256(long n) { return (unsigned)((n + 255) / 256); }

// dynamic LDS of the two dense kernels at k axes, in bytes (their own carving of smem_dyn)
constexpr int filter_lds(int k) { return (2 * k * (k | 1) + (2 * k + 1) * (k | 1) + 4 * k) * (int)sizeof(double); }
constexpr int backward_lds(int k) { return (2 * k * (k | 1) + 2 * k) * (int)sizeof(double); }

}  // namespace

int rv_smooth_workspace(rv_mosaic_desc* d) {
  const int rc = smooth_shape(d, "SMOOTH_WORKSPACE");
  if (rc) return rc;
  d->ws_bytes = smooth_layout(d->T, d->k, d->mode).bytes;
  return RV_OK;
}

int rv_smooth_filter(const rv_mosaic_desc* d, void* stream) {
  int rc = smooth_shape(d, "SMOOTH_FILTER");
  if (rc) return rc;
  const smooth_ws w = smooth_layout(d->T, d->k, d->mode);
  rc = smooth_operands(d, "SMOOTH_FILTER", "P", w);
  if (rc) return rc;
  RV_REQUIRE(!d->result || d->ldo >= d->k + 2, RV_ERR_SHAPE,
             "rv_mosaic(SMOOTH_FILTER): ldo=%ld holds no row of k + 2 = %ld values", d->ldo, d->k + 2);
  const hipStream_t st = (hipStream_t)stream;
  const int k = (int)d->k, L = (int)d->L;
  const long T = d->T;
  const double* const Bt = d->moment + (long)k * k;
  hipLaunchKernelGGL(k_smooth_observe, dim3(blocks256(T * k)), dim3(256), 0, st, d->q, d->weight, (const double*)d->centre,
                     (const double*)d->basis, T, L, k, w.at(d->ws, 0));
  if (w.dense) {
    // beyond the static 64 KB on purpose: A, the covariance and the 2 k + 1 rows of the factorisation stay in LDS for
    // the whole sequence (132.5 KB at k = 64, of the CU's 160 KB)
    static std::atomic<unsigned long long> attr_done{0};
    lds_opt_in((const void*)k_smooth_filter, filter_lds(SM_KDENSE), attr_done);
    const int smem = filter_lds(k);
    double* const qn = (double*)d->ws;
    hipLaunchKernelGGL(k_smooth_qn, dim3(blocks256((long)k * k)), dim3(256), 0, st, Bt, k, qn);
    hipLaunchKernelGGL(k_smooth_filter, dim3((unsigned)d->n_rows), dim3(SM_THREADS), smem, st, d->moment, (const double*)qn,
                       d->weight, d->lam, k, T, d->row_start, (const double*)w.at(d->ws, 0), w.at(d->ws, 1), w.at(d->ws, 2),
                       w.at(d->ws, 4), w.at(d->ws, 5), d->result, d->ldo);
  } else {
    hipLaunchKernelGGL(k_smooth_filter_diag, dim3((unsigned)d->n_rows), dim3(SM_THREADS), 0, st, d->moment, d->weight, d->lam, k,
                       T, d->row_start, (const double*)w.at(d->ws, 0), w.at(d->ws, 1), w.at(d->ws, 2), w.at(d->ws, 4),
                       w.at(d->ws, 5), w.at(d->ws, 6), w.at(d->ws, 7), d->result, d->ldo);
    if (d->result)
      hipLaunchKernelGGL(k_smooth_diag_sums, dim3(blocks256(T)), dim3(256), 0, st, d->weight, (const double*)w.at(d->ws, 6),
                         (const double*)w.at(d->ws, 7), T, k, d->result, d->ldo);
  }
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_smooth_backward(const rv_mosaic_desc* d, void* stream) {
  int rc = smooth_shape(d, "SMOOTH_BACKWARD");
  if (rc) return rc;
  const smooth_ws w = smooth_layout(d->T, d->k, d->mode);
  rc = smooth_operands(d, "SMOOTH_BACKWARD", "R", w);
  if (rc) return rc;
  RV_REQUIRE(d->out, RV_ERR_NULL, "rv_mosaic(SMOOTH_BACKWARD): out is null");
  RV_REQUIRE(d->ldo >= d->L, RV_ERR_SHAPE, "rv_mosaic(SMOOTH_BACKWARD): ldo=%ld holds no row of L=%ld values", d->ldo, d->L);
  const hipStream_t st = (hipStream_t)stream;
  const int k = (int)d->k, L = (int)d->L;
  const long T = d->T;
  if (w.dense) {
    static std::atomic<unsigned long long> attr_done{0};
    lds_opt_in((const void*)k_smooth_backward, backward_lds(SM_KDENSE), attr_done);   // 66 KB at k = 64
    const int smem = backward_lds(k);
    hipLaunchKernelGGL(k_smooth_backward, dim3((unsigned)d->n_rows), dim3(SM_THREADS), smem, st, d->moment, d->weight, k, T,
                       d->row_start, (const double*)w.at(d->ws, 1), (const double*)w.at(d->ws, 2),
                       (const double*)w.at(d->ws, 4), (const double*)w.at(d->ws, 5), w.at(d->ws, 3), d->state);
  } else {
    hipLaunchKernelGGL(k_smooth_backward_diag, dim3((unsigned)d->n_rows), dim3(SM_THREADS), 0, st, d->moment, d->weight, k, T,
                       d->row_start, (const double*)w.at(d->ws, 1), (const double*)w.at(d->ws, 2),
                       (const double*)w.at(d->ws, 4), (const double*)w.at(d->ws, 5), w.at(d->ws, 3), d->state);
  }
  hipLaunchKernelGGL(k_smooth_rows, dim3(blocks_for(T, 65536)), dim3(SM_THREADS), 0, st, d->q, d->weight,
                     (const double*)d->centre, (const double*)d->basis, T, L, k, (const double*)w.at(d->ws, 0),
                     (const double*)w.at(d->ws, 3), d->out, d->ldo);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_smooth_splice(const rv_mosaic_desc* d, void* stream) {
  RV_REQUIRE(d->n_out >= 1 && d->n_out < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(SMOOTH_SPLICE): n_out=%ld outside [1, 2^31)",
             d->n_out);
  RV_REQUIRE(d->n_rows >= 1 && d->n_rows < (1L << 31), RV_ERR_SHAPE,
             "rv_mosaic(SMOOTH_SPLICE): n_rows=%ld (the ranges) outside [1, 2^31)", d->n_rows);
  RV_REQUIRE(d->width >= 0 && d->width < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(SMOOTH_SPLICE): width=%ld (the fade) outside [0, 2^31)",
             d->width);
  RV_REQUIRE(d->src, RV_ERR_NULL, "rv_mosaic(SMOOTH_SPLICE): src is null");
  RV_REQUIRE(d->frames, RV_ERR_NULL, "rv_mosaic(SMOOTH_SPLICE): frames is null");
  RV_REQUIRE(d->room, RV_ERR_NULL, "rv_mosaic(SMOOTH_SPLICE): room (the ranges) is null");
  RV_REQUIRE(d->out, RV_ERR_NULL, "rv_mosaic(SMOOTH_SPLICE): out is null");
  hipLaunchKernelGGL(k_smooth_splice, dim3(blocks_for((d->n_out + 255) / 256, 65536)), dim3(256), 0, (hipStream_t)stream, d->src,
                     d->frames, d->room, d->n_rows, d->width, d->n_out, d->out);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
