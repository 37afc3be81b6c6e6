// What the ops over sequences of latent rows share (smooth.hip, hmm.hip, attr.hip): the rows a sequence owns, the whitened
// coordinate of a frame and a workgroup's staging of 64 frames of them.  Defined here once, down to the order of every fma.
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
