// Latent transport (rawaudiovae_kelsey_amd/transport.py): entropic optimal transport between two clouds of whitened latent
// rows, its Sinkhorn half-step and its barycentric map.  Five ops of rv_mosaic; the rules: include/rawvae_hip.h, "Latent
// transport"; the tiling and what was measured: DESIGN.md section 7.19.
//   RV_OT_WHITEN     k_ot_whiten: a workgroup per block of 64 frames stages their y (sequence.h's chain, the one RV_HMM_EMIT
//                    observes with) and writes y [T, k] and the observed flags.
//   RV_OT_SOFTMIN    k_ot_scan<ND, false>, then k_ot_merge.
//   RV_OT_MAP        k_ot_whiten into ws, k_ot_scan<ND, true>, then k_ot_apply (the merge, the diagnostics and the latent rows).
//   RV_OT_LIVE       rv_stream_encode, RV_OT_MAP's three launches on the block's latent rows, rv_stream_synth.
//   RV_OT_WORKSPACE  the bytes of ws.
// k_ot_scan is fp64 attention without the matrix.  A workgroup of four waves owns 64 query rows (16 to a wave) and one slab
// of the columns; it walks the slab in chunks of 64 columns staged in LDS with their norms, potentials and log-weights, a
// wave in tiles of 16 columns.  Both contractions run on v_mfma_f64_16x16x4_f64.  The score tile is computed TRANSPOSED
// (the columns as the A operand, the queries as B): lane l then holds query i = l & 15 and columns (l >> 4) + 4 reg, so
// register `reg` of the finished weights IS the A operand of k-step `reg` of the second contraction (moment.h states the
// layout) and w V needs no trip through LDS.  A row's running maximum is a reduction over the four registers and the lanes
// l, l ^ 16, l ^ 32; its sums stay per lane until the slab ends.  The slab's partials go to ws; a second kernel merges a
// row's slabs in ascending slab order.  No atomics, no polling; every output element is written by exactly one thread.
// The split of the columns into slabs depends on N alone, and no element of a tile depends on another row of it: a row's
// bits are the same whatever T is and whichever rows stand beside it.
#include <math.h>

#include "common.h"
#include "internal.h"
#include "moment.h"
#include "sequence.h"

using namespace rv;

namespace {

using mom::f64x4;

constexpr int OT_KMAX = 64;        // axes (the header states it)
constexpr int OT_LMAX = 512;
constexpr int OT_THREADS = 256;    // k_ot_scan: four waves
constexpr int OT_ROWS = 64;        // query rows of a workgroup, 16 to a wave
constexpr int OT_COLS = 64;        // columns staged at a time
constexpr int OT_SLABS = 8;        // slabs at most
constexpr long OT_SLAB_MIN = 256;  // columns of a slab at least (the header states the rule)
constexpr int OT_FRAMES = seq::FRAMES;
constexpr int OT_PITCH = seq::PITCH;

__device__ __forceinline__ double mul_rn(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}

// The slabs of N columns: ceil(N / 8) columns rounded up to 64, 256 at least.
struct ot_split {
  long slab;
  int n_slabs;
};
__host__ __device__ __forceinline__ ot_split split_of(long N) {
  ot_split s;
  s.slab = ((N + OT_SLABS - 1) / OT_SLABS + OT_COLS - 1) / OT_COLS * OT_COLS;
  if (s.slab < OT_SLAB_MIN) s.slab = OT_SLAB_MIN;
  s.n_slabs = (int)((N + s.slab - 1) / s.slab);
  return s;
}

// doubles of one (row, slab) partial: [m, sum w] or [m, sum w, sum w^2, sum w c, sum w V (k)]
__host__ __device__ __forceinline__ int partial_width(bool map, int k) { return map ? 4 + k : 2; }

// y [T, k] and info [T] (1: the frame's x row is finite; y = +0 otherwise)
__global__ void __launch_bounds__(seq::THREADS)
k_ot_whiten(const float* __restrict__ x, long ldx, const double* __restrict__ centre, const double* __restrict__ P, long T, int L,
            int k, double* __restrict__ ys, int* __restrict__ info) {
  __shared__ double sy[OT_FRAMES * OT_PITCH];
  __shared__ unsigned char sflag[seq::THREADS], sbad[OT_FRAMES];
  const long t0 = (long)blockIdx.x * OT_FRAMES;
  const int nf = T - t0 < OT_FRAMES ? (int)(T - t0) : OT_FRAMES;
  seq::stage_frames(x, ldx, centre, P, t0, nf, L, k, sy, sflag, sbad);
  for (int e = threadIdx.x; e < nf * k; e += seq::THREADS) {
    const int f = e / k, j = e - f * k;
    ys[t0 * k + e] = sy[f * OT_PITCH + j];
  }
  if ((int)threadIdx.x < nf) info[t0 + threadIdx.x] = sbad[threadIdx.x] ? 0 : 1;
}

// the four lanes that share a query (l & 15) hold four addends: ((p0 + p1) + p2) + p3 in ascending lane order, in every lane
__device__ __forceinline__ double quad_sum(double v, int li) {
  const double a = __shfl(v, li, 64), b = __shfl(v, li + 16, 64), c = __shfl(v, li + 32, 64), d = __shfl(v, li + 48, 64);
  return ((a + b) + c) + d;
}

// Block (x: 64 query rows, y: the slab).  A [T, k] the queries, B [N, k] the columns, h [N] their potential, lw [N] their
// log-weights.  c_ij = max(fma(-2, a.b, |a|^2 + |b|^2), 0), the norms chains fma(v, v, .) in ascending d from +0 and a.b the
// MFMA's sum in ascending d; s_ij = fma(h_j - c_ij, 1 / eps, lw_j), -inf where lw_j is.  Per tile of 16 columns:
// m' = max(m, the tile's maximum), every sum so far times exp(m - m'), then w = exp(s - m') added in ascending register order.
template <int ND, bool MAP>
__global__ void __launch_bounds__(OT_THREADS)
k_ot_scan(const double* __restrict__ A, const double* __restrict__ B, const double* __restrict__ h, const double* __restrict__ lw,
          long T, long N, int k, double eps, long slab, int n_slabs, double* __restrict__ part) {
  constexpr int KP = 16 * ND, P = KP + 1;
  __shared__ double Vs[OT_COLS * P];
  __shared__ double sh[OT_COLS], slw[OT_COLS], snb[OT_COLS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, li = lane & 15, lg = lane >> 4;
  const long i0 = (long)blockIdx.x * OT_ROWS + wv * 16;
  const bool active = i0 < T;   // wave-uniform
  const long irow = i0 + li < T ? i0 + li : T - 1;
  const double inv = 1.0 / eps;
  double qb[4 * ND];
#pragma unroll
  for (int s = 0; s < 4 * ND; ++s) {
    const int d = 4 * s + lg;
    qb[s] = d < k ? A[irow * k + d] : 0.0;
  }
  double na = 0.0;
  for (int d = 0; d < k; ++d) {
    const double a = A[irow * k + d];
    na = __builtin_fma(a, a, na);
  }
  double m = -INFINITY, sw = 0.0, sw2 = 0.0, swc = 0.0;
  f64x4 acc[ND];
#pragma unroll
  for (int nd = 0; nd < ND; ++nd) acc[nd] = f64x4{0.0, 0.0, 0.0, 0.0};
  const long j_lo = (long)blockIdx.y * slab, j_hi = j_lo + slab < N ? j_lo + slab : N;
  for (long j0 = j_lo; j0 < j_hi; j0 += OT_COLS) {
    __syncthreads();   // the tiles of the chunk before have read LDS
    for (int e = tid; e < OT_COLS * KP; e += OT_THREADS) {
      const int jj = e / KP, d = e - jj * KP;
      const long j = j0 + jj;
      Vs[jj * P + d] = (j < j_hi && d < k) ? B[j * k + d] : 0.0;
    }
    __syncthreads();
    if (tid < OT_COLS) {
      const long j = j0 + tid;
      double nb = 0.0;
      for (int d = 0; d < k; ++d) nb = __builtin_fma(Vs[tid * P + d], Vs[tid * P + d], nb);
      snb[tid] = nb;
      sh[tid] = j < j_hi ? h[j] : 0.0;
      slw[tid] = j < j_hi ? lw[j] : -INFINITY;
    }
    __syncthreads();
    if (!active) continue;
    for (int jt = 0; jt < OT_COLS && j0 + jt < j_hi; jt += 16) {
      f64x4 dot = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4 * ND; ++s)
        dot = __builtin_amdgcn_mfma_f64_16x16x4f64(Vs[(jt + li) * P + 4 * s + lg], qb[s], dot, 0, 0, 0);
      double sv[4], cv[4], tmax = -INFINITY;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int jj = jt + lg + 4 * r;
        double c = __builtin_fma(-2.0, dot[r], na + snb[jj]);
        c = c < 0.0 ? 0.0 : c;
        const double l = slw[jj];
        cv[r] = c;
        sv[r] = l == -INFINITY ? -INFINITY : __builtin_fma(sh[jj] - c, inv, l);
        tmax = fmax(tmax, sv[r]);
      }
      tmax = fmax(tmax, __shfl_xor(tmax, 16, 64));
      tmax = fmax(tmax, __shfl_xor(tmax, 32, 64));
      const double mn = fmax(m, tmax);
      const double scale = mn == m ? 1.0 : exp(m - mn);
      m = mn;
      double w[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) w[r] = (mn == -INFINITY || sv[r] == -INFINITY) ? 0.0 : exp(sv[r] - mn);
      sw = mul_rn(sw, scale);
#pragma unroll
      for (int r = 0; r < 4; ++r) sw += w[r];
      if constexpr (MAP) {
        sw2 = mul_rn(sw2, mul_rn(scale, scale));
        swc = mul_rn(swc, scale);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sw2 = __builtin_fma(w[r], w[r], sw2);
          swc = __builtin_fma(w[r], cv[r], swc);
        }
        if (__any(scale != 1.0)) {   // the accumulator's rows are (l >> 4) + 4 reg: their factors live in the lanes of that number
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double sc = __shfl(scale, lg + 4 * r, 64);
#pragma unroll
            for (int nd = 0; nd < ND; ++nd) acc[nd][r] = mul_rn(acc[nd][r], sc);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int nd = 0; nd < ND; ++nd)
            acc[nd] = __builtin_amdgcn_mfma_f64_16x16x4f64(w[r], Vs[(jt + 4 * r + lg) * P + nd * 16 + li], acc[nd], 0, 0, 0);
        }
      }
    }
  }
  if (!active) return;
  const int PW = partial_width(MAP, k);
  const double tw = quad_sum(sw, li);
  double tw2 = 0.0, twc = 0.0;
  if constexpr (MAP) {
    tw2 = quad_sum(sw2, li);
    twc = quad_sum(swc, li);
  }
  if (lg == 0 && i0 + li < T) {
    double* const p = part + ((i0 + li) * n_slabs + blockIdx.y) * PW;
    p[0] = m;
    p[1] = tw;
    if constexpr (MAP) {
      p[2] = tw2;
      p[3] = twc;
    }
  }
  if constexpr (MAP) {
#pragma unroll
    for (int nd = 0; nd < ND; ++nd) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long row = i0 + lg + 4 * r;
        const int d = nd * 16 + li;
        if (row < T && d < k) part[(row * n_slabs + blockIdx.y) * PW + 4 + d] = acc[nd][r];
      }
    }
  }
}

// The merge of a row's slabs: M = max_s m_s, e_s = exp(m_s - M) (0 for an empty slab), Z = sum_s fl(sw_s e_s) in ascending s
// from +0.  Returns false when no column had a finite weight.
__device__ __forceinline__ bool merge_slabs(const double* __restrict__ p, int n_slabs, int PW, double* e, double& M, double& Z) {
  M = -INFINITY;
  for (int s = 0; s < n_slabs; ++s) M = fmax(M, p[s * PW]);
  Z = 0.0;
  if (M == -INFINITY) return false;
  for (int s = 0; s < n_slabs; ++s) {
    const double ms = p[s * PW];
    e[s] = ms == -INFINITY ? 0.0 : (ms == M ? 1.0 : exp(ms - M));
    Z += mul_rn(p[s * PW + 1], e[s]);
  }
  return true;
}

// f_i = -eps (M + log Z); +inf for a row with no column of finite weight
__global__ void __launch_bounds__(256)
k_ot_merge(const double* __restrict__ part, long T, int n_slabs, double eps, double* __restrict__ f) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= T) return;
  double e[OT_SLABS], M, Z;
  const bool ok = merge_slabs(part + i * n_slabs * 2, n_slabs, 2, e, M, Z);
  f[i] = ok ? -mul_rn(eps, M + log(Z)) : INFINITY;
}

// One workgroup of 64 threads per row: the merge, the row of diagnostics and the latent row.  alpha [rows / per] or NULL (1).
// out may be x (neither is __restrict__): a thread reads an element of x before it writes that element of out, and no other.
__global__ void __launch_bounds__(64)
k_ot_apply(const float* x, long ldx, const double* __restrict__ W, const double* __restrict__ ys,
           const int* __restrict__ obs, const double* __restrict__ part, int n_slabs, int k, int L, double eps,
           const float* __restrict__ alpha, long per, float* out, long ldo, double* __restrict__ state) {
  __shared__ double sdiff[OT_KMAX];
  const long row = blockIdx.x;
  const int tid = threadIdx.x, PW = 4 + k;
  const double* const p = part + row * n_slabs * PW;
  double e[OT_SLABS], M, Z;
  const bool ok = merge_slabs(p, n_slabs, PW, e, M, Z) && obs[row] != 0;
  double* const st = state + row * (3 + k);
  if (tid < k) {
    double td = __builtin_nan("");
    if (ok) {
      double acc = 0.0;
      for (int s = 0; s < n_slabs; ++s) acc = __builtin_fma(p[s * PW + 4 + tid], e[s], acc);
      td = acc / Z;
    }
    st[3 + tid] = td;
    sdiff[tid] = td - ys[row * k + tid];
  }
  if (tid == 0) {
    if (ok) {
      double z2 = 0.0, zc = 0.0;
      for (int s = 0; s < n_slabs; ++s) {
        z2 = __builtin_fma(p[s * PW + 2], mul_rn(e[s], e[s]), z2);
        zc = __builtin_fma(p[s * PW + 3], e[s], zc);
      }
      st[0] = -mul_rn(eps, M + log(Z));
      st[1] = mul_rn(Z, Z) / z2;
      st[2] = zc / Z;
    } else {
      st[0] = obs[row] != 0 ? INFINITY : __builtin_nan("");
      st[1] = 0.0;
      st[2] = __builtin_nan("");
    }
  }
  __syncthreads();
  const double a = alpha ? (double)alpha[row / per] : 1.0;
  for (int l = tid; l < L; l += 64) {
    const float xv = x[row * ldx + l];
    float o = xv;
    if (ok) {
      double acc = 0.0;
      for (int d = 0; d < k; ++d) acc = __builtin_fma(W[(long)l * k + d], sdiff[d], acc);
      const double delta = mul_rn(a, acc);
      if (delta != 0.0) o = (float)((double)xv + delta);
    }
    out[row * ldo + l] = o;
  }
}

template <bool MAP>
void scan_launch(const double* A, const double* B, const double* h, const double* lw, long T, long N, int k, double eps,
                 double* part, hipStream_t st) {
  const ot_split sp = split_of(N);
  const dim3 grid((unsigned)((T + OT_ROWS - 1) / OT_ROWS), (unsigned)sp.n_slabs);
  const int nd = (k + 15) / 16;
#define OT_SCAN(ND_) \
  hipLaunchKernelGGL((k_ot_scan<ND_, MAP>), grid, dim3(OT_THREADS), 0, st, A, B, h, lw, T, N, k, eps, sp.slab, sp.n_slabs, part)
  if (nd == 1) OT_SCAN(1);
  else if (nd == 2) OT_SCAN(2);
  else if (nd == 3) OT_SCAN(3);
  else OT_SCAN(4);
#undef OT_SCAN
}

// ws of RV_OT_MAP: [ y (T k) doubles | observed (T) int32 | the partials (T n_slabs (4 + k)) doubles ]; of RV_OT_SOFTMIN: the
// partials (T n_slabs 2) alone.  Every part on a 256-byte boundary.
struct ot_ws {
  long y, obs, part, map_bytes, softmin_bytes, bytes;
};
ot_ws ot_layout(long T, long N, long k) {
  ot_ws w;
  const ot_split sp = split_of(N);
  w.y = 0;
  w.obs = up256(T * k * 8);
  w.part = w.obs + up256(T * 4);
  w.map_bytes = w.part + up256(T * sp.n_slabs * (4 + k) * 8);
  w.softmin_bytes = up256(T * sp.n_slabs * 2 * 8);
  w.bytes = w.map_bytes > w.softmin_bytes ? w.map_bytes : w.softmin_bytes;
  return w;
}

int ot_shape(const rv_mosaic_desc* d, const char* op, long T, bool columns) {
  RV_REQUIRE(T >= 1 && T < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): T=%ld outside [1, 2^31)", op, T);
  RV_REQUIRE(d->k >= 1 && d->k <= OT_KMAX, RV_ERR_SHAPE, "rv_mosaic(%s): k=%ld (the axes) outside [1, %d]", op, d->k, OT_KMAX);
  if (columns) RV_REQUIRE(d->N >= 1 && d->N < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(%s): N=%ld (the columns) outside [1, 2^31)", op, d->N);
  return RV_OK;
}

int ot_columns(const rv_mosaic_desc* d, const char* op) {
  RV_REQUIRE(isfinite(d->lam) && d->lam > 0.f, RV_ERR_SHAPE, "rv_mosaic(%s): lam=%g (epsilon) must be finite and positive", op,
             (double)d->lam);
  RV_REQUIRE(d->moment, RV_ERR_NULL, "rv_mosaic(%s): moment (the columns' cloud) is null", op);
  RV_REQUIRE(d->centre, RV_ERR_NULL, "rv_mosaic(%s): centre (the potential and the log-weights) is null", op);
  return RV_OK;
}

int ot_rows(const rv_mosaic_desc* d, const char* op, long L) {
  RV_REQUIRE(L >= d->k && L <= OT_LMAX, RV_ERR_SHAPE, "rv_mosaic(%s): L=%ld outside [k=%ld, %d]", op, L, d->k, OT_LMAX);
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(%s): basis (the whitening block) is null", op);
  return RV_OK;
}

int ot_workspace(const rv_mosaic_desc* d, const char* op, long T, long need) {
  RV_REQUIRE(d->ws_bytes >= need, RV_ERR_SHAPE, "rv_mosaic(%s): ws_bytes=%ld, T=%ld rows against N=%ld columns of k=%ld axes need %ld",
             op, d->ws_bytes, T, d->N, d->k, need);
  RV_REQUIRE(d->ws, RV_ERR_NULL, "rv_mosaic(%s): ws is null, T=%ld rows against N=%ld columns of k=%ld axes need %ld bytes", op, T,
             d->N, d->k, need);
  RV_REQUIRE(((uintptr_t)d->ws & 255) == 0, RV_ERR_SHAPE, "rv_mosaic(%s): ws is not 256-byte aligned", op);
  return RV_OK;
}

unsigned frame_blocks(long T) { return (unsigned)((T + OT_FRAMES - 1) / OT_FRAMES); }

// RV_OT_MAP's three launches on explicit rows: x [T, L] with pitch ldx -> out [T, ldo] and state; ws as ot_layout(T, N, k)
int map_launch(const rv_mosaic_desc* d, const float* x, long ldx, long T, long L, const float* alpha, long per, float* out,
               long ldo, char* ws, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  const int k = (int)d->k;
  const ot_ws w = ot_layout(T, d->N, d->k);
  const ot_split sp = split_of(d->N);
  const double eps = (double)d->lam;
  const double* const centre = d->basis;
  const double* const P = centre + L;
  const double* const W = P + d->k * L;
  double* const ys = (double*)(ws + w.y);
  int* const obs = (int*)(ws + w.obs);
  double* const part = (double*)(ws + w.part);
  hipLaunchKernelGGL(k_ot_whiten, dim3(frame_blocks(T)), dim3(seq::THREADS), 0, st, x, ldx, centre, P, T, (int)L, k, ys, obs);
  scan_launch<true>(ys, d->moment, (const double*)d->centre, (const double*)d->centre + d->N, T, d->N, k, eps, part, st);
  hipLaunchKernelGGL(k_ot_apply, dim3((unsigned)T), dim3(64), 0, st, x, ldx, W, (const double*)ys, (const int*)obs,
                     (const double*)part, sp.n_slabs, k, (int)L, eps, alpha, per, out, ldo, d->state);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

long live_rows(const rv_stream_desc* sd) { return sd->hop >= 1 ? sd->n_streams * (sd->block / sd->hop) : 0; }

}  // namespace

int rv_ot_workspace(rv_mosaic_desc* d) {
  const long T = d->live ? live_rows(d->live) : d->T;
  const int rc = ot_shape(d, "OT_WORKSPACE", T, true);
  if (rc) return rc;
  d->ws_bytes = ot_layout(T, d->N, d->k).bytes + (d->live ? up256(T * d->live->L * 4) : 0);
  return RV_OK;
}

int rv_ot_whiten(const rv_mosaic_desc* d, void* stream) {
  int rc = ot_shape(d, "OT_WHITEN", d->T, false);
  if (rc) return rc;
  rc = ot_rows(d, "OT_WHITEN", d->L);
  if (rc) return rc;
  RV_REQUIRE(d->stride >= d->L, RV_ERR_SHAPE, "rv_mosaic(OT_WHITEN): stride=%ld (the row pitch of x) holds no row of L=%ld values",
             d->stride, d->L);
  RV_REQUIRE(d->a, RV_ERR_NULL, "rv_mosaic(OT_WHITEN): a (the latent rows x) is null");
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(OT_WHITEN): result (y) is null");
  RV_REQUIRE(d->info, RV_ERR_NULL, "rv_mosaic(OT_WHITEN): info is null");
  hipLaunchKernelGGL(k_ot_whiten, dim3(frame_blocks(d->T)), dim3(seq::THREADS), 0, (hipStream_t)stream, d->a, d->stride,
                     (const double*)d->basis, (const double*)d->basis + d->L, d->T, (int)d->L, (int)d->k, d->result, d->info);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_ot_softmin(const rv_mosaic_desc* d, void* stream) {
  int rc = ot_shape(d, "OT_SOFTMIN", d->T, true);
  if (rc) return rc;
  rc = ot_columns(d, "OT_SOFTMIN");
  if (rc) return rc;
  RV_REQUIRE(d->basis, RV_ERR_NULL, "rv_mosaic(OT_SOFTMIN): basis (the rows' cloud) is null");
  RV_REQUIRE(d->result, RV_ERR_NULL, "rv_mosaic(OT_SOFTMIN): result is null");
  rc = ot_workspace(d, "OT_SOFTMIN", d->T, ot_layout(d->T, d->N, d->k).softmin_bytes);
  if (rc) return rc;
  const hipStream_t st = (hipStream_t)stream;
  const double eps = (double)d->lam;
  scan_launch<false>(d->basis, d->moment, (const double*)d->centre, (const double*)d->centre + d->N, d->T, d->N, (int)d->k, eps,
                     (double*)d->ws, st);
  hipLaunchKernelGGL(k_ot_merge, dim3((unsigned)((d->T + 255) / 256)), dim3(256), 0, st, (const double*)d->ws, d->T,
                     split_of(d->N).n_slabs, eps, d->result);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_ot_map(const rv_mosaic_desc* d, void* stream) {
  int rc = ot_shape(d, "OT_MAP", d->T, true);
  if (rc) return rc;
  rc = ot_rows(d, "OT_MAP", d->L);
  if (rc) return rc;
  rc = ot_columns(d, "OT_MAP");
  if (rc) return rc;
  RV_REQUIRE(d->stride >= d->L, RV_ERR_SHAPE, "rv_mosaic(OT_MAP): stride=%ld (the row pitch of x) holds no row of L=%ld values",
             d->stride, d->L);
  RV_REQUIRE(d->ldo >= d->L, RV_ERR_SHAPE, "rv_mosaic(OT_MAP): ldo=%ld holds no row of L=%ld values", d->ldo, d->L);
  RV_REQUIRE(d->a, RV_ERR_NULL, "rv_mosaic(OT_MAP): a (the latent rows x) is null");
  RV_REQUIRE(d->out, RV_ERR_NULL, "rv_mosaic(OT_MAP): out is null");
  RV_REQUIRE(d->state, RV_ERR_NULL, "rv_mosaic(OT_MAP): state (the diagnostics) is null");
  rc = ot_workspace(d, "OT_MAP", d->T, ot_layout(d->T, d->N, d->k).map_bytes);
  if (rc) return rc;
  return map_launch(d, d->a, d->stride, d->T, d->L, d->weight, d->T, d->out, d->ldo, (char*)d->ws, stream);
}

int rv_ot_live(const rv_mosaic_desc* d, void* stream) {
  const rv_stream_desc* sd = d->live;
  RV_REQUIRE(sd, RV_ERR_NULL, "rv_mosaic(OT_LIVE): the stream (live) is null");
  const long M = live_rows(sd);
  int rc = ot_shape(d, "OT_LIVE", M, true);
  if (rc) return rc;
  rc = ot_rows(d, "OT_LIVE", sd->L);
  if (rc) return rc;
  rc = ot_columns(d, "OT_LIVE");
  if (rc) return rc;
  RV_REQUIRE(d->weight, RV_ERR_NULL, "rv_mosaic(OT_LIVE): weight (the amount of every stream) is null");
  RV_REQUIRE(d->state, RV_ERR_NULL, "rv_mosaic(OT_LIVE): state (the diagnostics) is null");
  const long qbytes = up256(M * sd->L * 4);
  rc = ot_workspace(d, "OT_LIVE", M, qbytes + ot_layout(M, d->N, d->k).map_bytes);
  if (rc) return rc;
  char* const ws = (char*)d->ws;
  float *q = (float*)ws, *z = nullptr, *frames = nullptr;
  rc = rv_stream_encode(sd, q, &z, &frames, stream);
  if (rc) return rc;
  rc = map_launch(d, q, sd->L, M, sd->L, d->weight, sd->block / sd->hop, z, sd->L, ws + qbytes, stream);
  if (rc) return rc;
  return rv_stream_synth(sd, 1, stream);
}
