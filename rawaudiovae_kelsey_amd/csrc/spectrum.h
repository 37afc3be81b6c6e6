// The power spectrum of one windowed frame in LDS, defined once for RV_EVAL_FRAMES (eval.hip) and RV_ATTR_DESCRIBE
// (attr.hip); the rules: include/rawvae_hip.h, "Evaluation".  Plain fp32 with every product and sum rounded on its own
// (no contraction), so that the float32 restatement of tests/eval_oracle.py states it operation for operation.
//   N = S / 2, lg = log2 N.  The windowed signal a[n] = fl(w[n] x[n]) is read as N complex points
//   z[m] = a[2m] + i a[2m + 1] and stored bit-reversed, z[m] at zr / zi [rev(m)] (put).  lg stages of decimation-in-time
//   butterflies in place, h = 1, 2, .., N / 2: butterfly j < N / 2 has p = j mod h, i0 = 2 h (j div h) + p, i1 = i0 + h,
//   W = tw[p * (N / h)] (tw[q] = exp(-2 pi i q / S), S / 2 entries), t = W z[i1], z[i1] = z[i0] - t, z[i0] = z[i0] + t.
//   Then the real-transform post-pass on the pairs (k, N - k), k = 0 .. N / 2, with Z[N] = Z[0]:
//   E = (Z[k] + conj Z[N - k]) / 2, O = (Z[k] - conj Z[N - k]) / 2i, T = tw[k] O, and the two powers P[k] = |E + T|^2,
//   P[N - k] = |E - T|^2, written over zr[k], zr[N - k] (zr has N + 1 slots) -- every pair is read and written by one
//   thread.  LDS: 2 N + 1 floats per signal.  The bit-reversed store of the load sends consecutive lanes N / 64 floats
//   apart (16-way bank conflicts at N = 2048, 4-way at N = 512), once per sample; the stages with h < 32 are 2-way
//   conflicted.
#pragma once
#include <math.h>

#include "common.h"

namespace rv {
namespace spec {

constexpr int THREADS = 256;   // the workgroup of every caller
constexpr int SMAX = 4096;     // longest frame with a spectrum
constexpr int SMIN = 32;

__device__ __forceinline__ float block_max_f32(float v, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

struct cpx {
  float r, i;
};

__device__ __forceinline__ cpx cmul(float wr, float wi, float zr, float zi) {
#pragma clang fp contract(off)
  cpx o;
  o.r = wr * zr - wi * zi;
  o.i = wr * zi + wi * zr;
  return o;
}

__device__ __forceinline__ float power(float r, float i) {
#pragma clang fp contract(off)
  return r * r + i * i;
}

// log2 of the N = S / 2 complex points
__device__ __forceinline__ int stages(int N) { return 31 - __clz(N > 0 ? N : 1); }

// sample n of the windowed signal to its bit-reversed place: even n the real part, odd n the imaginary one
__device__ __forceinline__ void put(float* zr, float* zi, int n, int lg, float a) {
  const int m = (int)(__brev((unsigned)(n >> 1)) >> (32 - lg));
  if (n & 1) zi[m] = a;
  else zr[m] = a;
}

// After every thread's puts: the lg butterfly stages and the post-pass.  On return zr[0 .. N] holds the thread's own
// pairs of the powers (the caller's next barrier publishes the rest), pmax has taken the thread's powers in by fmaxf and
// bad is set where one of them is NaN or +inf (fmaxf would drop a NaN, so it is carried on its own).
__device__ __forceinline__ void powers(float* zr, float* zi, const float* __restrict__ tw, int N, float& pmax, bool& bad) {
  const int half = N >> 1;
  for (int h = 1, sh = 0; h < N; h <<= 1, ++sh) {
    __syncthreads();
    const int tstep = N >> sh;   // N / h
    for (int j = threadIdx.x; j < half; j += THREADS) {
      const int p = j & (h - 1);
      const int i0 = ((j >> sh) << (sh + 1)) + p, i1 = i0 + h;
      const float wr = tw[2 * p * tstep], wi = tw[2 * p * tstep + 1];
      const cpx tt = cmul(wr, wi, zr[i1], zi[i1]);
      const float ur = zr[i0], ui = zi[i0];
      zr[i0] = ur + tt.r;
      zi[i0] = ui + tt.i;
      zr[i1] = ur - tt.r;
      zi[i1] = ui - tt.i;
    }
  }
  __syncthreads();
  // the pair (k, N - k) belongs to one thread, so the powers may overwrite the points in place
  for (int k = threadIdx.x; k <= half; k += THREADS) {
    const int kn = k == 0 ? 0 : N - k;
    const float wr = tw[2 * k], wi = tw[2 * k + 1];
    const float er = 0.5f * (zr[k] + zr[kn]), ei = 0.5f * (zi[k] - zi[kn]);
    const float orr = 0.5f * (zi[k] + zi[kn]), oi = -0.5f * (zr[k] - zr[kn]);
    const cpx tt = cmul(wr, wi, orr, oi);
    const float p0 = power(er + tt.r, ei + tt.i);
    const float p1 = power(er - tt.r, ei - tt.i);
    zr[k] = p0;
    if (N - k != k) zr[N - k] = p1;
    bad = bad || !(p0 < INFINITY) || !(p1 < INFINITY);
    pmax = fmaxf(pmax, fmaxf(p0, p1));
  }
}

}  // namespace spec
}  // namespace rv
