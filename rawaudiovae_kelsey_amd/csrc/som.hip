// Self-organising map of latent vectors (the SOM that picks the sources of tutorial.ipynb:725-805 and 1078-1146):
//   rv_segment_mean  : one descriptor per file, the fp64 mean of its frames' mu, rounded once
//   rv_som_bmu       : best and second-best node of every row, direct squared distances (the hot path)
//   rv_som_node_sums : per-node fp64 sums of member rows and member counts, in ascending row order (no atomics)
//   rv_som_update    : the batch-SOM step w[m] = sum_b h(m, b) sums[b] / sum_b h(m, b) counts[b] in fp64
// Layout, tiling, reduction orders and the accuracy argument: DESIGN.md section 7.3.
#include <limits.h>

#include "common.h"
#include "sqdist.h"
#include "../../include/rawvae_hip.h"

using namespace rv;
using namespace rv::sqd;

namespace {

// branch-free (selects), so the per-row state stays in registers
__device__ __forceinline__ void top2_insert(float d, int i, float& b1, int& i1, float& b2, int& i2) {
  const bool lt1 = cand_less(d, i, b1, i1), lt2 = cand_less(d, i, b2, i2);
  b2 = lt1 ? b1 : (lt2 ? d : b2);
  i2 = lt1 ? i1 : (lt2 ? i : i2);
  b1 = lt1 ? d : b1;
  i1 = lt1 ? i : i1;
}

__global__ void __launch_bounds__(256)
k_som_bmu(const float* __restrict__ x, long N, const float* __restrict__ w, int M, long L, int* __restrict__ best,
          int* __restrict__ second, float* __restrict__ d_best, float* __restrict__ d_second) {
  // the stages of sqdist.h's tile; the top twos stay in registers, so no distance tile shares LDS with them
  __shared__ __attribute__((aligned(16))) float Xs[KT][BR + PAD];
  __shared__ __attribute__((aligned(16))) float Ws[KT][BN + PAD];
  const int tid = threadIdx.x, tn = tid & 15, tr = tid >> 4;
  const long n_tiles = (N + BR - 1) / BR;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const long r0 = tile * BR;
    float b1[TR], b2[TR];
    int i1[TR], i2[TR];
#pragma unroll
    for (int i = 0; i < TR; ++i) { b1[i] = b2[i] = INFINITY; i1[i] = i2[i] = INT_MAX; }
    for (int m0 = 0; m0 < M; m0 += BN) {
      float tot[TR][TN];
      // node indices fit an int (M < INT_MAX - BN): the node predicate stays a 32-bit compare
      tile_sq_dist(Xs, Ws, x, w, r0, m0, L, [&](long gr) { return gr < N; }, [&](long gm) { return (int)gm < M; }, tot);
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int m = m0 + tn * TN + j;
        if (m < M) {
#pragma unroll
          for (int i = 0; i < TR; ++i) top2_insert(tot[i][j], m, b1[i], i1[i], b2[i], i2[i]);
        }
      }
    }
    // the 16 lanes sharing a row hold disjoint node sets: merge their top twos (lanes 16 q .. 16 q + 15 of a wave)
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
#pragma unroll
      for (int i = 0; i < TR; ++i) {
        const float pb1 = __shfl_xor(b1[i], o, 64), pb2 = __shfl_xor(b2[i], o, 64);
        const int pi1 = __shfl_xor(i1[i], o, 64), pi2 = __shfl_xor(i2[i], o, 64);
        top2_insert(pb1, pi1, b1[i], i1[i], b2[i], i2[i]);
        top2_insert(pb2, pi2, b1[i], i1[i], b2[i], i2[i]);
      }
    }
    if (tn == 0) {
#pragma unroll
      for (int i = 0; i < TR; ++i) {
        const long r = r0 + tr * TR + i;
        if (r < N) {
          best[r] = i1[i] == INT_MAX ? -1 : i1[i];
          second[r] = i2[i] == INT_MAX ? -1 : i2[i];
          d_best[r] = b1[i];
          d_second[r] = b2[i];
        }
      }
    }
  }
}

// one block per segment (grid-stride), threads over the latent index: ascending-row fp64 sum, divided and rounded once
__global__ void __launch_bounds__(256)
k_segment_mean(const float* __restrict__ x, long R, long L, const long long* __restrict__ offsets, long F,
               float* __restrict__ out) {
  for (long f = blockIdx.x; f < F; f += gridDim.x) {
    long lo = offsets[f], hi = offsets[f + 1];
    lo = lo < 0 ? 0 : (lo > R ? R : lo);   // the host checked its copy of the offsets; clamping keeps a device copy
    hi = hi < lo ? lo : (hi > R ? R : hi); //   that disagrees inside x (an empty segment then gives NaN)
    for (long l = threadIdx.x; l < L; l += 256) {
      double s = 0.0;
      for (long r = lo; r < hi; ++r) s += (double)x[r * L + l];
      out[f * L + l] = (float)(s / (double)(hi - lo));
    }
  }
}

constexpr int NS_ROWS = 256;   // rows of bmu scanned per step of k_som_node_sums
constexpr int NS_LC = 4;       // latent elements per thread per pass: 1024 per pass
constexpr int NS_BATCH = 8;    // member rows whose loads are in flight before their adds

// one block per node (grid-stride): scan bmu in steps of 256 rows, compact the members of the step into LDS in
// ascending order, add their rows into fp64 accumulators in that order.  Fixed order, no atomics: bit-identical runs.
__global__ void __launch_bounds__(256)
k_som_node_sums(const float* __restrict__ x, long N, long L, const int* __restrict__ bmu, int M,
                double* __restrict__ sums, long long* __restrict__ counts) {
  __shared__ long list[NS_ROWS];
  __shared__ int wave_n[4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int m = blockIdx.x; m < M; m += gridDim.x) {
    long long count = 0;
    for (long l0 = 0; l0 < L; l0 += 256 * NS_LC) {
      double acc[NS_LC];
#pragma unroll
      for (int c = 0; c < NS_LC; ++c) acc[c] = 0.0;
      count = 0;
      for (long c0 = 0; c0 < N; c0 += NS_ROWS) {
        const long r = c0 + tid;
        const bool hit = r < N && bmu[r] == m;
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) wave_n[wv] = __popcll(mask);
        __syncthreads();
        int base = 0;
        for (int q = 0; q < wv; ++q) base += wave_n[q];
        const int n_hit = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
        if (hit) list[base + __popcll(mask & ((1ull << lane) - 1))] = r;
        __syncthreads();
        for (int p0 = 0; p0 < n_hit; p0 += NS_BATCH) {
          const int nb = n_hit - p0 < NS_BATCH ? n_hit - p0 : NS_BATCH;
#pragma unroll
          for (int c = 0; c < NS_LC; ++c) {
            const long l = l0 + tid + 256 * c;
            if (l < L) {
              float v[NS_BATCH];
#pragma unroll
              for (int q = 0; q < NS_BATCH; ++q) v[q] = q < nb ? x[list[q < nb ? p0 + q : p0] * L + l] : 0.f;
#pragma unroll
              for (int q = 0; q < NS_BATCH; ++q)
                if (q < nb) acc[c] += (double)v[q];
            }
          }
        }
        count += n_hit;
        __syncthreads();   // list and wave_n are rewritten by the next step
      }
#pragma unroll
      for (int c = 0; c < NS_LC; ++c) {
        const long l = l0 + tid + 256 * c;
        if (l < L) sums[(long)m * L + l] = acc[c];
      }
    }
    if (tid == 0) counts[m] = count;
  }
}

constexpr int UP_LC = 4;

// one block per node m (grid-stride): h(m, b) for 256 nodes b at a time in LDS, then every thread forms the same
// denominator and the numerators of its latent elements, ascending b, in fp64
__global__ void __launch_bounds__(256)
k_som_update(const double* __restrict__ sums, const long long* __restrict__ counts, const float* __restrict__ w_old,
             int rows, int cols, long L, double two_sigma2, float* __restrict__ w_new) {
  __shared__ double h[256];
  const int tid = threadIdx.x, M = rows * cols;
  for (int m = blockIdx.x; m < M; m += gridDim.x) {
    const int mr = m / cols, mc = m % cols;
    for (long l0 = 0; l0 < L; l0 += 256 * UP_LC) {
      double num[UP_LC], den = 0.0;
#pragma unroll
      for (int c = 0; c < UP_LC; ++c) num[c] = 0.0;
      for (int b0 = 0; b0 < M; b0 += 256) {
        const int b = b0 + tid;
        if (b < M) {
          const double dr = (double)(mr - b / cols), dc = (double)(mc - b % cols), d2 = dr * dr + dc * dc;
          h[tid] = d2 == 0.0 ? 1.0 : exp(-d2 / two_sigma2);   // the node itself is 1 even when 2 sigma^2 underflows
        }
        __syncthreads();
        const int nb = M - b0 < 256 ? M - b0 : 256;
        for (int q = 0; q < nb; ++q) {
          const double hq = h[q];
          den += hq * (double)counts[b0 + q];
#pragma unroll
          for (int c = 0; c < UP_LC; ++c) {
            const long l = l0 + tid + 256 * c;
            if (l < L) num[c] += hq * sums[(long)(b0 + q) * L + l];
          }
        }
        __syncthreads();
      }
#pragma unroll
      for (int c = 0; c < UP_LC; ++c) {
        const long l = l0 + tid + 256 * c;
        if (l < L) w_new[(long)m * L + l] = den == 0.0 ? w_old[(long)m * L + l] : (float)(num[c] / den);
      }
    }
  }
}

}  // namespace

extern "C" int rv_segment_mean(const float* x, long R, long L, const long long* offsets,
                               const long long* offsets_host, long F, float* out, void* stream) {
  RV_REQUIRE(x && offsets && offsets_host && out, RV_ERR_NULL, "rv_segment_mean: null pointer");
  RV_REQUIRE(R >= 1 && L >= 1 && F >= 1, RV_ERR_SHAPE, "rv_segment_mean: bad extents R=%ld L=%ld F=%ld", R, L, F);
  RV_REQUIRE(offsets_host[0] >= 0 && offsets_host[F] <= R, RV_ERR_SHAPE,
             "rv_segment_mean: offsets [%lld, %lld] outside the %ld rows", offsets_host[0], offsets_host[F], R);
  for (long f = 0; f < F; ++f)
    RV_REQUIRE(offsets_host[f + 1] > offsets_host[f], RV_ERR_SHAPE,
               "rv_segment_mean: segment %ld is empty (offsets %lld, %lld)", f, offsets_host[f], offsets_host[f + 1]);
  hipLaunchKernelGGL(k_segment_mean, dim3(blocks_for(F, 65536)), dim3(256), 0, (hipStream_t)stream, x, R, L, offsets,
                     F, out);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_som_bmu(const float* x, long N, const float* w, long M, long L, int* best, int* second,
                          float* d_best, float* d_second, void* stream) {
  RV_REQUIRE(x && w && best && second && d_best && d_second, RV_ERR_NULL, "rv_som_bmu: null pointer");
  RV_REQUIRE(N >= 1 && M >= 2 && M < INT_MAX - BN && L >= 1, RV_ERR_SHAPE,
             "rv_som_bmu: bad extents N=%ld M=%ld L=%ld", N, M, L);
  hipLaunchKernelGGL(k_som_bmu, dim3(blocks_for((N + BR - 1) / BR, 1L << 20)), dim3(256), 0, (hipStream_t)stream, x,
                     N, w, (int)M, L, best, second, d_best, d_second);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_som_node_sums(const float* x, long N, long L, const int* bmu, long M, double* sums,
                                long long* counts, void* stream) {
  RV_REQUIRE(x && bmu && sums && counts, RV_ERR_NULL, "rv_som_node_sums: null pointer");
  RV_REQUIRE(N >= 1 && L >= 1 && M >= 1 && M < INT_MAX, RV_ERR_SHAPE,
             "rv_som_node_sums: bad extents N=%ld L=%ld M=%ld", N, L, M);
  hipLaunchKernelGGL(k_som_node_sums, dim3(blocks_for(M, 65536)), dim3(256), 0, (hipStream_t)stream, x, N, L, bmu,
                     (int)M, sums, counts);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

extern "C" int rv_som_update(const double* sums, const long long* counts, const float* w_old, long rows, long cols,
                             long L, double sigma, float* w_new, void* stream) {
  RV_REQUIRE(sums && counts && w_old && w_new, RV_ERR_NULL, "rv_som_update: null pointer");
  RV_REQUIRE(rows >= 1 && cols >= 1 && rows * cols >= 2 && rows * cols < INT_MAX && L >= 1, RV_ERR_SHAPE,
             "rv_som_update: bad extents rows=%ld cols=%ld L=%ld", rows, cols, L);
  RV_REQUIRE(sigma > 0.0 && sigma < INFINITY, RV_ERR_SHAPE, "rv_som_update: sigma %g must be positive and finite",
             sigma);
  RV_REQUIRE(w_old != w_new, RV_ERR_SHAPE, "rv_som_update: w_new must not alias w_old");
  hipLaunchKernelGGL(k_som_update, dim3(blocks_for(rows * cols, 65536)), dim3(256), 0, (hipStream_t)stream, sums,
                     counts, w_old, (int)rows, (int)cols, L, 2.0 * sigma * sigma, w_new);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
