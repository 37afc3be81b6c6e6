// What the ops over sequences of latent rows share (smooth.hip, hmm.hip): the rows a sequence owns and the whitened
// coordinate of a frame.  Defined here once, down to the order of every fma.
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

}  // namespace seq
}  // namespace rv
