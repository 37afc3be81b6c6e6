// What the ops over sequences of latent rows share (smooth.hip, hmm.hip, attr.hip, walk.hip, switch.hip): the rows a
// sequence owns, which pairs of rows lie in one file, the whitened coordinate of a frame, a workgroup's staging of 64 frames
// of them, and the roundings of a generated frame.  Defined here once, down to the order of every fma.
#pragma once
#include "common.h"

namespace rv {
namespace seq {

// the sequence's rows, clamped to [0, T]: a row_start the caller did not check reads and writes nothing outside
__device__ __forceinline__ void rows_of(const long long* __restrict__ row_start, long s, long T, long& t0, long& t1) {
  t0 = row_start[s];
  t1 = row_start[s + 1];
  t0 = t0 < 0 ? 0 : (t0 > T ? T : t0);
  t1 = t1 < t0 ? t0 : (t1 > T ? T : t1);
}

// whether the pair of rows (p, p + 1) spans two files: p + 1 is one of row_start[0 .. n_files] (ascending; the first entry
// >= p + 1 by bisection).  RV_PCA_LAGCOV's and RV_SWITCH_MOMENTS' rule.
__device__ __forceinline__ bool pair_spans_files(const long long* __restrict__ row_start, long n_files, long p) {
  long lo = 0, hi = n_files + 1;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (row_start[mid] < p + 1) lo = mid + 1;
    else hi = mid;
  }
  return lo <= n_files && row_start[lo] == p + 1;
}

// The two roundings of a generated frame that RV_WALK_STEP and RV_SWITCH_STEP share, never contracted into an fma: the
// noise temperature * eps, and the latent (float)(c + (double)offset + acc).
__device__ __forceinline__ double noise_of(double temp, float e) {
#pragma clang fp contract(off)
  return temp * (double)e;
}
__device__ __forceinline__ float latent_of(double c, float off, double acc) {
#pragma clang fp contract(off)
  return (float)(c + (double)off + acc);
}

// y_j = sum_l P[j, l] ((double)x[l] - c[l]) in ascending l from +0: pr = row j of P, xr = the frame's latent row
__device__ __forceinline__ double whiten_axis(const double* __restrict__ pr, const float* __restrict__ xr,
                                              const double* __restrict__ centre, int L) {
  double acc = 0.0;
  for (int l = 0; l < L; ++l) acc = __builtin_fma(pr[l], (double)xr[l] - centre[l], acc);
  return acc;
}

constexpr int THREADS = 256;   // the workgroup of stage_frames
constexpr int FRAMES = 64;     // frames it stages
constexpr int PITCH = 65;      // doubles between two frames' y in LDS

// The frames [t0, t0 + nf) of a workgroup of THREADS threads: sbad[f] != 0 iff row f of x holds a value that is not
// finite, and sy[f * PITCH + j] = y_j of frame f (+0 for such a frame).  sflag: THREADS bytes of scratch.
__device__ __forceinline__ void stage_frames(const float* __restrict__ x, long ldx, const double* __restrict__ centre,
                                             const double* __restrict__ P, long t0, int nf, int L, int k, double* sy,
                                             unsigned char* sflag, unsigned char* sbad) {
  const int tid = threadIdx.x;
  {
    const int f = tid >> 2, q = tid & 3;
    bool bad = false;
    if (f < nf) {
      const float* const xr = x + (t0 + f) * ldx;
      for (int l = q; l < L; l += 4) bad |= !(fabsf(xr[l]) <= 3.402823466e38f);
    }
    sflag[tid] = bad;
  }
  __syncthreads();
  if (tid < FRAMES) sbad[tid] = sflag[4 * tid] | sflag[4 * tid + 1] | sflag[4 * tid + 2] | sflag[4 * tid + 3];
  __syncthreads();
  // a wave shares an axis (P's row is read by all its lanes at once), a lane walks its own frame's row
  for (int e = tid; e < FRAMES * k; e += THREADS) {
    const int j = e / FRAMES, f = e - j * FRAMES;
    if (f >= nf) continue;
    sy[f * PITCH + j] = sbad[f] ? 0.0 : whiten_axis(P + (long)j * L, x + (t0 + f) * ldx, centre, L);
  }
  __syncthreads();
}

}  // namespace seq
}  // namespace rv
