// Grain fitting for latent mosaicing (rawaudiovae_kelsey_amd/mosaic.py: fit_grains, gather_fitted): the two ops of
// rv_mosaic that refine a selected corpus frame against its target frame.  The rule: include/rawvae_hip.h, "Grain
// fitting"; the measured figures: DESIGN.md section 7.5, "Grain fitting".
//   RV_GRAIN_FIT     per (target frame, candidate) the shift in [-R, R] and the gain of the least-squares fit of the
//                    shifted grain to the frame: k_grain_fit, one workgroup per pair
//   RV_GRAIN_GATHER  RV_MOSAIC_GATHER_MEAN with a shift and a gain per candidate: k_grain_gather
// and the live path's use of both (RV_MOSAIC_LIVE / LIVE_DRAIN with a fit, mosaic_live.hip): rv_grain_live_* keep the
// streams' input in a TARGET RING (k_live_target), fit the frames a block is about to play against the target frames
// they stand for (k_grain_fit reading its frame from the ring) and gather them into the stream's frame buffer.
#include <limits.h>
#include <math.h>

#include "common.h"
#include "internal.h"

using namespace rv;

namespace {

constexpr int FIT_RMAX = 1024;     // largest R
constexpr int FIT_CH = 1024;       // samples of a frame staged at a time; a longer frame goes chunk by chunk
constexpr int FIT_NS = 4;          // adjacent shifts per thread: one 16-byte LDS read of the grain feeds 32 fmas
constexpr int FIT_THREADS = 256;
constexpr int FIT_SPAN = FIT_CH + 2 * FIT_RMAX + 8;   // floats of the staged grain span: 12 320 bytes, 16 KB with x

// a before b in the order of the choice: greater score, then smaller |delta|, then the negative delta.  Scores are
// never NaN (a NaN sum scores 0) and the deltas of one pair are distinct, so the order is total and the winner does
// not depend on who compares first.
__device__ __forceinline__ bool fit_before(double sa, int da, double sb, int db) {
  if (sa != sb) return sa > sb;
  const int aa = da < 0 ? -da : da, ab = db < 0 ? -db : db;
  return aa < ab || (aa == ab && da < db);
}

// Where the live path's target frames live (header, "Live grain fitting").  Per stream a ring of C floats: input
// sample a (counted from the stream's last reset; a < 0 is the silence before it) sits at ring[a mod C].  Target frame
// n is samples [n hop - P, n hop - P + S).  Row r of the fit is stream r / F, frame r % F of the block; it stands for
// target frame tfr[r] (the lagged selection's stamp of the committed row) or, tfr == NULL, cnt[stream] + r % F, the
// frame arriving now.  A frame older than max_age frames has left the ring and is not fitted.
struct fit_ring {
  const long long* cnt;
  const long long* tfr;
  long F, C, P;
  long max_age;
};

// One workgroup per (t, j).  Shift delta = lo + d, d in [0, nsh): thread u of a pass owns d = 4 u .. 4 u + 3 and
// walks n with two accumulators per shift, c = fmaf(x[n], g[n + d], c) and e = fmaf(g[n + d], g[n + d], e), each a
// plain ascending chain over n from +0 -- the chain of a (delta, n) term never depends on which thread, pass or chunk
// holds it.  The frame x and the span g[0 .. len + nsh - 1) are staged in LDS per chunk of FIT_CH samples; per four n
// a thread reads x as one broadcast b128 and four new grain samples as one b128 at consecutive 16-byte slots across
// lanes (conflict-free), and keeps the other four in registers (the sliding window).
// RING false: the frame is tgt[t hop, t hop + S) of one waveform (RV_GRAIN_FIT).  RING true: tgt holds the streams'
// target rings and `ring` says where row t's frame starts; only the staging of x differs.
template <bool RING>
__global__ void __launch_bounds__(FIT_THREADS)
k_grain_fit(const float* __restrict__ tgt, long hop, int S, const int* __restrict__ idx, int k,
            const float* __restrict__ src, long src_len, const long long* __restrict__ row_start, long n_rows,
            const int* __restrict__ room, int R, float gain_max, int* __restrict__ shift, float* __restrict__ gain,
            double* __restrict__ score, fit_ring ring) {
  __shared__ __attribute__((aligned(16))) float xs[FIT_CH];
  __shared__ __attribute__((aligned(16))) float gs[FIT_SPAN];
  __shared__ double red_s[FIT_THREADS / 64];
  __shared__ int red_d[FIT_THREADS / 64];
  const long tj = blockIdx.x;
  const long t = tj / k;
  const long i = idx[tj];
  // everything up to the first barrier is uniform over the workgroup
  bool ok = i >= 0 && i < n_rows;
  long st = 0;
  if (ok) {
    st = row_start[i];
    ok = st >= 0 && st <= src_len - S;
  }
  const float* x = tgt + t * hop;
  long xb = 0;   // RING: the frame's first sample in the stream's ring, in [0, C)
  if constexpr (RING) {
    const long sr = t / ring.F, j = t - sr * ring.F;
    const long long now = ring.cnt[sr] + j, tf = ring.tfr ? ring.tfr[t] : now;
    ok = ok && tf <= now && now - tf <= ring.max_age;
    x = tgt + sr * ring.C;
    if (ok) {
      xb = (long)((tf * hop - ring.P) % ring.C);
      if (xb < 0) xb += ring.C;
    }
  }
  if (!ok) {
    if (threadIdx.x == 0) {
      shift[tj] = 0;
      gain[tj] = 0.f;
      score[tj] = 0.0;
    }
    return;
  }
  const int rb = room[2 * i], rf = room[2 * i + 1];
  int lo = -(rb < 0 ? 0 : (rb < R ? rb : R)), hi = rf < 0 ? 0 : (rf < R ? rf : R);
  if (st + lo < 0) lo = (int)-st;                              // whatever room says, a grain never leaves src
  if (st + hi > src_len - S) hi = (int)(src_len - S - st);
  const int nsh = hi - lo + 1;
  const float* g = src + st + lo;

  double best_s = -1.0;   // below every score: the first permitted shift replaces it
  int best_d = INT_MAX;
  float best_c = 0.f, best_e = 0.f;
  for (int u0 = 0; FIT_NS * u0 < nsh; u0 += blockDim.x) {
    const int d0 = FIT_NS * (u0 + (int)threadIdx.x);
    const bool active = d0 < nsh;
    float c[FIT_NS], e[FIT_NS];
#pragma unroll
    for (int s = 0; s < FIT_NS; ++s) c[s] = e[s] = 0.f;
    for (int n0 = 0; n0 < S; n0 += FIT_CH) {
      const int len = S - n0 < FIT_CH ? S - n0 : FIT_CH;
      const int xlen = (len + 3) & ~3;          // the reads below reach xs[0, xlen) and gs[0, glen + 7)
      const int glen = len + nsh - 1;           // <= FIT_CH + 2 FIT_RMAX
      __syncthreads();
      if constexpr (RING) {
        for (int m = threadIdx.x; m < xlen; m += blockDim.x) {
          long p = xb + n0 + m;   // < 2 C: S <= C
          if (p >= ring.C) p -= ring.C;
          xs[m] = m < len ? x[p] : 0.f;
        }
      } else {
        for (int m = threadIdx.x; m < xlen; m += blockDim.x) xs[m] = m < len ? x[n0 + m] : 0.f;
      }
      for (int m = threadIdx.x; m < glen + 8; m += blockDim.x) gs[m] = m < glen ? g[n0 + m] : 0.f;
      __syncthreads();
      if (!active) continue;
      const float* gp = gs + d0;
      f32x4 w0 = *reinterpret_cast<const f32x4*>(gp);
      const int full = len & ~3;
      int n = 0;
      for (; n < full; n += 4) {
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + n);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(gp + n + 4);
        const float w[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
#pragma unroll
          for (int s = 0; s < FIT_NS; ++s) {
            c[s] = __builtin_fmaf(xv[m], w[m + s], c[s]);
            e[s] = __builtin_fmaf(w[m + s], w[m + s], e[s]);
          }
        }
        w0 = w1;
      }
      if (n < len) {   // the last 1..3 samples of a frame whose length is no multiple of 4
        const int rem = len - n;
        const f32x4 xv = *reinterpret_cast<const f32x4*>(xs + n);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(gp + n + 4);
        const float w[8] = {w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], w1[2], w1[3]};
#pragma unroll
        for (int m = 0; m < 3; ++m) {
          if (m < rem) {
#pragma unroll
            for (int s = 0; s < FIT_NS; ++s) {
              c[s] = __builtin_fmaf(xv[m], w[m + s], c[s]);
              e[s] = __builtin_fmaf(w[m + s], w[m + s], e[s]);
            }
          }
        }
      }
    }
    if (active) {
#pragma unroll
      for (int s = 0; s < FIT_NS; ++s) {
        if (d0 + s < nsh) {
          const float cs = c[s], es = e[s];
          const bool pos = cs > 0.f && es > 0.f && cs < INFINITY && es < INFINITY;   // false for a NaN
          const double sc = pos ? (double)cs * (double)cs / (double)es : 0.0;
          const int dl = lo + d0 + s;
          if (fit_before(sc, dl, best_s, best_d)) {
            best_s = sc;
            best_d = dl;
            best_c = cs;
            best_e = es;
          }
        }
      }
    }
  }
  // the workgroup's first under the order: within a wave by shuffles, then over the waves' firsts through LDS
  double ws = best_s;
  int wd = best_d;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double os = __shfl_xor(ws, o, 64);
    const int od = __shfl_xor(wd, o, 64);
    if (fit_before(os, od, ws, wd)) {
      ws = os;
      wd = od;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    red_s[threadIdx.x >> 6] = ws;
    red_d[threadIdx.x >> 6] = wd;
  }
  __syncthreads();
  ws = red_s[0];
  wd = red_d[0];
  for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
    if (fit_before(red_s[w], red_d[w], ws, wd)) {
      ws = red_s[w];
      wd = red_d[w];
    }
  if (best_d == wd) {   // the one thread that holds the chosen shift's sums
    float gn = 1.f;
    if (gain_max != 0.f) {
      // c / e through fp64 is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2 bits)
      gn = ws > 0.0 ? fminf((float)((double)best_c / (double)best_e), gain_max) : 0.f;
    }
    shift[tj] = wd;
    gain[tj] = gn;
    score[tj] = ws;
  }
}

__device__ __forceinline__ float scaled_add(float acc, float g, float v) {
#pragma clang fp contract(off)
  return acc + g * v;
}

// k_gather_mean (mosaic.hip) with candidate j of row t read `shift[t, j]` samples later and scaled by `gain[t, j]`:
// the product rounded before its add, ascending j from +0, times 1/k once.
__global__ void __launch_bounds__(256)
k_grain_gather(const float* __restrict__ src, long src_len, const long long* __restrict__ row_start, long stride,
               long n_rows, long width, const int* __restrict__ idx, const int* __restrict__ shift,
               const float* __restrict__ gain, long T, int k, float* __restrict__ out, long ldo) {
  const float inv = 1.0f / (float)k;
  for (long t = blockIdx.x; t < T; t += gridDim.x) {
    for (long w = threadIdx.x; w < width; w += 256) {
      float acc = 0.f;
      for (int j = 0; j < k; ++j) {
        const long i = idx[t * k + j];
        if (i < 0 || i >= n_rows) continue;
        const long st = (row_start ? row_start[i] : i * stride) + shift[t * k + j];
        if (st < 0 || st + width > src_len) continue;
        acc = scaled_add(acc, gain[t * k + j], src[st + w]);
      }
      out[t * ldo + w] = acc * inv;
    }
  }
}

// The block of every stream into its target ring at the stream's frame count (k_stream_ola moves the count on at the
// end of the call, so every kernel of one call reads the same count).  Grid (ceil(block / 256), n_streams).
__global__ void __launch_bounds__(256)
k_live_target(const float* __restrict__ x, long ld_x, long block, long hop, long C, const long long* __restrict__ cnt,
              float* __restrict__ ring) {
  const long s = blockIdx.y, i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= block) return;
  const long p = (long)((cnt[s] * hop + i) % C);
  ring[s * C + p] = x[s * ld_x + i];
}

// Grid (ceil(C / 256), streams): silence in the rings of streams [first, first + gridDim.y)
__global__ void __launch_bounds__(256) k_live_target_clear(float* __restrict__ ring, long C, long first) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < C) ring[(first + blockIdx.y) * C + i] = 0.f;
}

unsigned fit_threads(long R) {
  const long units = (2 * R + 1 + FIT_NS - 1) / FIT_NS;
  return (unsigned)(units >= FIT_THREADS ? FIT_THREADS : (units + 63) / 64 * 64);
}

int fit_tk_check(const rv_mosaic_desc* d, const char* op) {
  RV_REQUIRE(d->T >= 1 && d->T < (1L << 40), RV_ERR_SHAPE, "rv_mosaic(%s): T=%ld outside [1, 2^40)", op, d->T);
  RV_REQUIRE(d->k >= 1 && d->k <= KMAX, RV_ERR_SHAPE, "rv_mosaic(%s): k=%ld must be in [1, %d]", op, d->k, KMAX);
  return RV_OK;
}

}  // namespace

int rv_grain_fit(const rv_mosaic_desc* d, void* stream) {
  const int rc = fit_tk_check(d, "GRAIN_FIT");
  if (rc) return rc;
  RV_REQUIRE(d->fit_radius >= 0 && d->fit_radius <= FIT_RMAX, RV_ERR_SHAPE,
             "rv_mosaic(GRAIN_FIT): fit_radius=%ld outside [0, %d]", d->fit_radius, FIT_RMAX);
  RV_REQUIRE(d->gain_max >= 0.f && d->gain_max < INFINITY, RV_ERR_SHAPE,
             "rv_mosaic(GRAIN_FIT): gain_max=%g must be finite and not negative", (double)d->gain_max);
  RV_REQUIRE(d->idx, RV_ERR_NULL, "rv_mosaic(GRAIN_FIT): idx is null");
  RV_REQUIRE(d->frames, RV_ERR_NULL, "rv_mosaic(GRAIN_FIT): frames is null");
  RV_REQUIRE(d->src, RV_ERR_NULL, "rv_mosaic(GRAIN_FIT): src is null");
  RV_REQUIRE(d->row_start, RV_ERR_NULL, "rv_mosaic(GRAIN_FIT): row_start is null");
  RV_REQUIRE(d->room, RV_ERR_NULL, "rv_mosaic(GRAIN_FIT): room is null");
  RV_REQUIRE(d->shift, RV_ERR_NULL, "rv_mosaic(GRAIN_FIT): shift is null");
  RV_REQUIRE(d->gain, RV_ERR_NULL, "rv_mosaic(GRAIN_FIT): gain is null");
  RV_REQUIRE(d->score, RV_ERR_NULL, "rv_mosaic(GRAIN_FIT): score is null");
  RV_REQUIRE(d->S >= 1 && d->S < INT_MAX && d->hop >= 1 && d->hop < (1L << 20), RV_ERR_SHAPE,
             "rv_mosaic(GRAIN_FIT): bad framing S=%ld hop=%ld", d->S, d->hop);
  RV_REQUIRE(d->n_out >= 1 && d->S <= d->n_out && (d->T - 1) * d->hop <= d->n_out - d->S, RV_ERR_SHAPE,
             "rv_mosaic(GRAIN_FIT): T=%ld frames of S=%ld at hop=%ld overrun n_out=%ld", d->T, d->S, d->hop, d->n_out);
  RV_REQUIRE(d->n_rows >= 1 && d->n_rows < INT_MAX, RV_ERR_SHAPE, "rv_mosaic(GRAIN_FIT): n_rows=%ld outside [1, 2^31)",
             d->n_rows);
  RV_REQUIRE(d->src_len >= d->S, RV_ERR_SHAPE, "rv_mosaic(GRAIN_FIT): src_len=%ld holds no grain of S=%ld", d->src_len,
             d->S);
  RV_REQUIRE(d->T * d->k < (1L << 31), RV_ERR_SHAPE, "rv_mosaic(GRAIN_FIT): T=%ld rows of k=%ld too many for one call",
             d->T, d->k);
  hipLaunchKernelGGL(k_grain_fit<false>, dim3((unsigned)(d->T * d->k)), dim3(fit_threads(d->fit_radius)), 0,
                     (hipStream_t)stream, d->frames, d->hop, (int)d->S, d->idx, (int)d->k, d->src, d->src_len,
                     d->row_start, d->n_rows, d->room, (int)d->fit_radius, d->gain_max, d->shift, d->gain, d->score, fit_ring{});
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_grain_gather(const rv_mosaic_desc* d, void* stream) {
  const int rc = fit_tk_check(d, "GRAIN_GATHER");
  if (rc) return rc;
  RV_REQUIRE(d->idx, RV_ERR_NULL, "rv_mosaic(GRAIN_GATHER): idx is null");
  RV_REQUIRE(d->src, RV_ERR_NULL, "rv_mosaic(GRAIN_GATHER): src is null");
  RV_REQUIRE(d->out, RV_ERR_NULL, "rv_mosaic(GRAIN_GATHER): out is null");
  RV_REQUIRE(d->shift, RV_ERR_NULL, "rv_mosaic(GRAIN_GATHER): shift is null");
  RV_REQUIRE(d->gain, RV_ERR_NULL, "rv_mosaic(GRAIN_GATHER): gain is null");
  RV_REQUIRE(d->width >= 1 && d->n_rows >= 1 && d->src_len >= d->width && d->ldo >= d->width &&
                 (d->row_start || d->stride >= 0),
             RV_ERR_SHAPE, "rv_mosaic(GRAIN_GATHER): bad extents width=%ld n_rows=%ld src_len=%ld ldo=%ld stride=%ld",
             d->width, d->n_rows, d->src_len, d->ldo, d->stride);
  const long blocks = d->T > 65536 ? 65536 : d->T;
  hipLaunchKernelGGL(k_grain_gather, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d->src, d->src_len,
                     d->row_start, d->stride, d->n_rows, d->width, d->idx, d->shift, d->gain, d->T, (int)d->k, d->out,
                     d->ldo);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

long rv_grain_live_ring(long S, long hop, long block, long lag) { return S - hop + 2 * lag * hop + block; }

int rv_grain_live_check(const rv_mosaic_desc* d, const char* op, int run) {
  RV_REQUIRE(d->fit_radius >= 0 && d->fit_radius <= FIT_RMAX, RV_ERR_SHAPE, "rv_mosaic(%s): fit_radius=%ld outside [0, %d]",
             op, d->fit_radius, FIT_RMAX);
  RV_REQUIRE(d->gain_max >= 0.f && d->gain_max < INFINITY, RV_ERR_SHAPE,
             "rv_mosaic(%s): gain_max=%g must be finite and not negative", op, (double)d->gain_max);
  if (d->fit_radius == 0 && d->gain_max == 0.f) return RV_OK;
  RV_REQUIRE(d->mode == RV_LIVE_GRAINS, RV_ERR_UNSUPPORTED,
             "rv_mosaic(%s): a fit (fit_radius=%ld, gain_max=%g) needs mode RV_LIVE_GRAINS, mode=%ld plays no "
             "corpus audio", op, d->fit_radius, (double)d->gain_max, d->mode);
  const rv_stream_desc* sd = d->live;
  RV_REQUIRE(sd->S < INT_MAX && sd->hop < (1L << 20) && sd->n_streams * (sd->block / sd->hop) * d->k < (1L << 31) &&
                 (sd->block + 255) / 256 < (1L << 31) && sd->n_streams <= 65535, RV_ERR_SHAPE,
             "rv_mosaic(%s): a fit takes S=%ld < 2^31, hop=%ld < 2^20, n_streams=%ld <= 65535 and fewer than 2^31 "
             "(frame, candidate) pairs", op, sd->S, sd->hop, sd->n_streams);
  if (!run) return RV_OK;
  RV_REQUIRE(d->next_of, RV_ERR_NULL, "rv_mosaic(%s): with a fit next_of [3 N] holds the successors and room: it is null",
             op);
  RV_REQUIRE(d->shift, RV_ERR_NULL, "rv_mosaic(%s): shift is null", op);
  RV_REQUIRE(d->gain, RV_ERR_NULL, "rv_mosaic(%s): gain is null", op);
  RV_REQUIRE(d->score, RV_ERR_NULL, "rv_mosaic(%s): score is null", op);
  return RV_OK;
}

int rv_grain_live_reset(float* ring, long C, long first, long n, void* stream) {
  hipLaunchKernelGGL(k_live_target_clear, dim3((unsigned)((C + 255) / 256), (unsigned)n), dim3(256), 0,
                     (hipStream_t)stream, ring, C, first);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_grain_live(const rv_mosaic_desc* d, const int* sel, int sel_k, float* ring, const long long* cnt,
                  const long long* tfr, float* frames, void* stream) {
  const rv_stream_desc* sd = d->live;
  const hipStream_t st = (hipStream_t)stream;
  const long F = sd->block / sd->hop, M = sd->n_streams * F;
  const long C = rv_grain_live_ring(sd->S, sd->hop, sd->block, d->lag);
  hipLaunchKernelGGL(k_live_target, dim3((unsigned)((sd->block + 255) / 256), (unsigned)sd->n_streams), dim3(256), 0, st,
                     sd->x, sd->ld_x, sd->block, sd->hop, C, cnt, ring);
  const fit_ring fr{cnt, tfr, F, C, sd->S - sd->hop, 2 * d->lag};
  hipLaunchKernelGGL(k_grain_fit<true>, dim3((unsigned)(M * sel_k)), dim3(fit_threads(d->fit_radius)), 0, st, ring,
                     sd->hop, (int)sd->S, sel, sel_k, d->src, d->src_len, d->row_start, d->N, d->next_of + d->N,
                     (int)d->fit_radius, d->gain_max, d->shift, d->gain, d->score, fr);
  hipLaunchKernelGGL(k_grain_gather, dim3((unsigned)(M > 65536 ? 65536 : M)), dim3(256), 0, st, d->src, d->src_len,
                     d->row_start, 0L, d->N, sd->S, sel, d->shift, d->gain, M, sel_k, frames, sd->S);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
