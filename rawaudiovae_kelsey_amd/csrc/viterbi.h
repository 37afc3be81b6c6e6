// The Viterbi rule of the unit selection over a row's k <= 16 candidates, as one wave computes it: the offline path
// (k_path_forward / k_path_backtrack, mosaic_path.hip) and the lagged live selection (lag_solve in k_live_lag,
// mosaic_live.hip) step through the same device-inline pieces, so that a window solve is the offline pass bit for bit.
// Defined here once; the rule and its measured figures: DESIGN.md sections 7.5 ("Continuity") and 7.7.
#pragma once
#include "common.h"

namespace rv {
namespace vit {

constexpr int PATH_NONE = 255;   // back / end byte: no predecessor, no finite score

// one rounding each, never contracted into an fma
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// v of another lane by a DPP move: quad_perm [1,0,3,2] / [2,3,0,1] (lane ^ 1, lane ^ 2) and row_ror:4 / :8 (the lane
// 4 or 8 further on in its row of 16) -- a few cycles, where a shuffle through the LDS crossbar takes a round trip
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_ROR4 = 0x124, DPP_ROR8 = 0x128;
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) { return __int_as_float(dpp_i<CTRL>(__float_as_int(v))); }

// (v, i) becomes the better of itself and (ov, oi): smaller value, then lower index (i = PATH_NONE where v is +inf).
// The order is total, so an all-reduce gives every lane the same pair whatever the exchange pattern.
__device__ __forceinline__ void path_take(float& v, int& i, float ov, int oi) {
  if (ov < v || (ov == v && oi < i)) { v = ov; i = oi; }
}
// over the 4 lanes of a column (q = lane & 3)
__device__ __forceinline__ void path_min_q(float& v, int& i) {
  path_take(v, i, dpp_f<DPP_XOR1>(v), dpp_i<DPP_XOR1>(i));
  path_take(v, i, dpp_f<DPP_XOR2>(v), dpp_i<DPP_XOR2>(i));
}
// over the 16 columns (j = lane >> 2): the 4 columns of a row of 16 lanes by rotations, the 4 rows by shuffles
__device__ __forceinline__ void path_min_j(float& v, int& i) {
  path_take(v, i, dpp_f<DPP_ROR8>(v), dpp_i<DPP_ROR8>(i));
  path_take(v, i, dpp_f<DPP_ROR4>(v), dpp_i<DPP_ROR4>(i));
  path_take(v, i, __shfl_xor(v, 16, 64), __shfl_xor(i, 16, 64));
  path_take(v, i, __shfl_xor(v, 32, 64), __shfl_xor(i, 32, 64));
}

// The forward rule's pieces, shared by k_path_forward and k_live_lag; lane = 4 j + q owns column j and the predecessors
// i = 4 q .. 4 q + 3 (k_path_forward's layout).
// fl(lambda * trans), never 0 * inf
__device__ __forceinline__ float path_weigh(float lam, float tr) { return tr < INFINITY ? mul_rn(lam, tr) : INFINITY; }
// a candidate's own cost: +inf for a missing candidate or NaN
__device__ __forceinline__ float path_target(bool jv, int ci, float d) { return (jv && ci >= 0 && d == d) ? d : INFINITY; }
// hands every lane the new scores of its 4 predecessors (raw, not yet reduced by their minimum) and the row's
// (minimum, lowest-j argmin)
__device__ __forceinline__ void path_spread(float nw, int j, int q, float (&raw)[4], float& m, int& mj) {
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) raw[ii] = __shfl(nw, (4 * q + ii) * 4, 64);
  m = nw;
  mj = j;
  path_min_j(m, mj);
}
// One row: p = the weighted transitions from this lane's 4 predecessors into column j, tg = column j's own cost.
// Updates the carried (nw, raw, m, mj) and returns back[t, j] (PATH_NONE where the row starts a sequence: `first`, or
// no new[j] finite).
__device__ __forceinline__ int path_step(const float (&p)[4], float tg, bool first, int j, int q, float& nw,
                                         float (&raw)[4], float& m, int& mj) {
  const bool fin = m < INFINITY;
  float best = INFINITY;
  int bi = PATH_NONE;
#pragma unroll
  for (int ii = 0; ii < 4; ++ii) {
    const float c = (fin ? raw[ii] - m : raw[ii]) + p[ii];   // +inf where s[i] or the transition is
    if (c < best) { best = c; bi = 4 * q + ii; }
  }
  path_min_q(best, bi);
  nw = bi != PATH_NONE ? tg + best : INFINITY;
  int bk = nw < INFINITY ? bi : PATH_NONE;
  path_spread(nw, j, q, raw, m, mj);
  if (first || !(m < INFINITY)) {   // wave-uniform: the row starts a new sequence
    nw = tg;
    bk = PATH_NONE;
    path_spread(nw, j, q, raw, m, mj);
  }
  return bk;
}
// the backtrack's step from row t to row t - 1: b = back[t, slot[t]] (PATH_NONE for a row without a slot), e = end[t - 1]
__device__ __forceinline__ int path_back(int b, int e, int k) {
  if (b >= k) b = PATH_NONE;
  return b != PATH_NONE ? b : (e < k ? e : -1);
}

}  // namespace vit
}  // namespace rv
