// The distance between two latent rows, and the order among candidates, of the whole latent search family: rv_som_bmu
// (som.hip), the kNN search and its few-query form (mosaic_knn.hip), the unit selection (mosaic_path.hip,
// mosaic_live.hip), the alignment's local costs (align.hip).  Defined here once, down to the bit:
//   D(x, w) = tot, where per tile of KT latent elements  part = fmaf(d, d, part), d = x[l] - w[l], in ascending l from
//   +0, then tot += part, the tiles in ascending order from +0.
//   Out-of-range rows, columns and k stage zeros: (0 - 0)^2 adds an exact 0.
//   Candidates are ordered "smaller distance, then lower index" (cand_less).
// Two forms of it: the 128 x 64 x 32 register tile over LDS stages (tile_sq_dist) and the pair form (sq_acc4,
// row_sq_dist, row_sq_dist4).  Layout and the accuracy argument: DESIGN.md section 7.3.
#pragma once
#include "common.h"

namespace rv {
namespace sqd {

// The tile: BR rows x BN columns per block, KT latent elements per LDS stage; 256 threads as 16 (rows) x 16
// (columns), each owning a TR x TN = 8 x 4 register tile (8 x 8 with both accumulator levels spills past 256 VGPRs).
constexpr int BR = 128, BN = 64, KT = 32, TR = 8, TN = 4, PAD = 4, DPAD = 1;
// LDS floats of the two staging arrays, of a finished BR x BN distance tile, and of a kernel that lets them share
constexpr int STAGE_FLOATS = KT * (BR + PAD) + KT * (BN + PAD), DIST_FLOATS = BR * (BN + DPAD);
constexpr int SMEM_FLOATS = STAGE_FLOATS > DIST_FLOATS ? STAGE_FLOATS : DIST_FLOATS;
// Row stride of a kernel that stages whole rows' KT-wide slices in LDS (k_knn_small, k_transition): rows stay 16-byte
// aligned and the b128 reads of 16 consecutive rows cover all 64 banks.
constexpr int SLICE_ROW = KT + 4;

// (d, i) < (e, j) in the order "smaller distance, then lower index": a total order on the candidates of one row
// (indices are distinct), so the top k of a set do not depend on the order it is visited in.  NaN never wins.
__device__ __forceinline__ bool cand_less(float d, int i, float e, int j) { return d < e || (d == e && i < j); }

// tot[i][j] = D(x[r0 + 8 tr + i], w[m0 + 4 tn + j]) for thread (tr, tn) = (tid >> 4, tid & 15) of 256, over all of L.
// Xs / Ws are the k-major staging arrays (a thread's 8 rows are one 32-byte run); row_ok(gr) / col_ok(gm) say which
// rows of x / w exist (the others stage zeros).  Ends with a barrier: the stages may be overwritten on return.
template <class RowOk, class ColOk>
__device__ __forceinline__ void tile_sq_dist(float (*Xs)[BR + PAD], float (*Ws)[BN + PAD], const float* __restrict__ x,
                                             const float* __restrict__ w, long r0, long m0, long L, RowOk row_ok,
                                             ColOk col_ok, float (&tot)[TR][TN]) {
  const int tid = threadIdx.x, tn = tid & 15, tr = tid >> 4;
#pragma unroll
  for (int i = 0; i < TR; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) tot[i][j] = 0.f;
  for (long k0 = 0; k0 < L; k0 += KT) {
    // stage x[r0 : r0 + BR, k0 : k0 + KT] and w[m0 : m0 + BN, k0 : k0 + KT]; 32 lanes read 128 contiguous bytes of
    // one row
#pragma unroll
    for (int s = 0; s < KT * BR / 256; ++s) {
      const int e = tid + 256 * s, kk = e & (KT - 1), rr = e / KT;
      const long gk = k0 + kk, gr = r0 + rr;
      Xs[kk][rr] = (row_ok(gr) && gk < L) ? x[gr * L + gk] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < KT * BN / 256; ++s) {
      const int e = tid + 256 * s, kk = e & (KT - 1), rr = e / KT;
      const long gk = k0 + kk, gm = m0 + rr;
      Ws[kk][rr] = (col_ok(gm) && gk < L) ? w[gm * L + gk] : 0.f;
    }
    __syncthreads();
    float part[TR][TN];
#pragma unroll
    for (int i = 0; i < TR; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) part[i][j] = 0.f;
#pragma unroll 4
    for (int k = 0; k < KT; ++k) {
      const f32x4 xa = *reinterpret_cast<const f32x4*>(&Xs[k][tr * TR]);
      const f32x4 xb = *reinterpret_cast<const f32x4*>(&Xs[k][tr * TR + 4]);
      const f32x4 wa = *reinterpret_cast<const f32x4*>(&Ws[k][tn * TN]);
      const float xv[TR] = {xa[0], xa[1], xa[2], xa[3], xb[0], xb[1], xb[2], xb[3]};
      const float wv[TN] = {wa[0], wa[1], wa[2], wa[3]};
#pragma unroll
      for (int i = 0; i < TR; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const float d = xv[i] - wv[j];
          part[i][j] = __builtin_fmaf(d, d, part[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < TR; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) tot[i][j] += part[i][j];
    __syncthreads();
  }
}

// four terms of a tile's part, in order
__device__ __forceinline__ void sq_acc4(float& part, const f32x4& a, const f32x4& b) {
#pragma unroll
  for (int x = 0; x < 4; ++x) {
    const float d = a[x] - b[x];
    part = __builtin_fmaf(d, d, part);
  }
}

// D(a, b) of two latent rows in global memory, element by element
__device__ __forceinline__ float row_sq_dist(const float* __restrict__ a, const float* __restrict__ b, long L) {
  float tot = 0.f;
  for (long k0 = 0; k0 < L; k0 += KT) {
    const int n = L - k0 < KT ? (int)(L - k0) : KT;
    float part = 0.f;
    for (int kk = 0; kk < n; ++kk) {
      const float d = a[k0 + kk] - b[k0 + kk];
      part = __builtin_fmaf(d, d, part);
    }
    tot += part;
  }
  return tot;
}

// the same by 16-byte loads: rows_vec16 holds for the rows
__device__ __forceinline__ float row_sq_dist4(const float* __restrict__ a, const float* __restrict__ b, long L) {
  float tot = 0.f;
  for (long k0 = 0; k0 < L; k0 += KT) {
    const int n = L - k0 < KT ? (int)(L - k0) : KT;
    float part = 0.f;
    for (int kk = 0; kk < n; kk += 4)
      sq_acc4(part, *reinterpret_cast<const f32x4*>(a + k0 + kk), *reinterpret_cast<const f32x4*>(b + k0 + kk));
    tot += part;
  }
  return tot;
}

// Whether the rows of a [., L] matrix at c can be read by 16-byte loads: every row starts on a 16-byte boundary and a
// vector that starts inside a row ends inside it.
inline bool rows_vec16(const float* c, long L) { return L % 4 == 0 && ((unsigned long)c & 15) == 0; }

// 16 bytes of a row at column gk, zeros past L: one vector load when `vec` (rows_vec16), else element by element
__device__ __forceinline__ f32x4 slice_fetch4(const float* __restrict__ row, long gk, long L, bool vec) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  const float* p = row + gk;
  if (vec) {
    if (gk < L) v = *reinterpret_cast<const f32x4*>(p);
  } else {
#pragma unroll
    for (int x = 0; x < 4; ++x)
      if (gk + x < L) v[x] = p[x];
  }
  return v;
}

}  // namespace sqd
}  // namespace rv
