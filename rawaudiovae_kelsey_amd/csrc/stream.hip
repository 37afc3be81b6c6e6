// Streaming resynthesis: a few frames per call through the exact-fp32 inference arithmetic, with per-stream state.
//   rv_small_linear_f32 : y = act(x W^T + b) for few rows.  One lane owns one output column and R rows; the lane walks
//                         its weight row in ascending k with the R accumulators side by side (R independent fmaf chains
//                         share each weight load), weights and inputs loaded straight into VGPRs one chunk ahead.  No
//                         LDS, no split-K: every output is acc = +0, acc = fmaf(x[k], w[k], acc) for k = 0..K-1, + b,
//                         then the activation -- the k-ordered chain v_mfma_f32_32x32x2_f32 computes in rv_linear_fp32.
//   rv_stream_process   : five launches per block -- fc1 reading its frames from the history and the new block, the two
//                         heads + latent controls + reparameterisation, fc3, fc4, then overlap-add + history update.
//   rv_stream_reset     : zero one stream's state (or every stream's).
//   rv_stream_encode / rv_stream_synth (internal.h): the two ends of rv_stream_process for the live mosaic
//                         (mosaic_live.hip), which puts a corpus search between them.
#include "common.h"
#include "philox.h"
#include "reparam.h"
#include "internal.h"

using namespace rv;

namespace {

constexpr int KU = 32;        // k per chunk of rv_small_linear_f32 (8 float4 of the weight row per lane)
constexpr int KU_HEADS = 16;  // ... of the heads (two weight rows per lane)

// Where the rows of the left operand live.  Row r is stream s = r / F, frame j = r % F; its element k sits at position
// t = j * hop + k of the concatenation [history of stream s (P samples) | b + s * ldb].  The history of stream s is
// a + ((cnt[s] / F) & 1) * alt + s * lda (two buffers, ping-ponged by the call count).  A plain matrix is P = 0, F = M,
// hop = ldx, ldb = 0.
struct Rows {
  const float* a;
  const float* b;
  long lda, ldb, alt, F, hop, P;
  const long long* cnt;
};

struct RowPtr {
  const float* a;
  const float* b;
  long t0, P;
  __device__ __forceinline__ float ld1(long k) const {
    const long t = t0 + k;
    return *(t < P ? a + t : b + (t - P));
  }
  // t0, P and k multiples of 4: a float4 never straddles the two sources
  __device__ __forceinline__ float4 ld4(long k) const {
    const long t = t0 + k;
    return *reinterpret_cast<const float4*>(t < P ? a + t : b + (t - P));
  }
};

__device__ __forceinline__ RowPtr row_ptr(const Rows& xs, long r) {
  const long s = r / xs.F, j = r - s * xs.F;
  RowPtr p;
  p.a = xs.b + s * xs.ldb;   // (unused when P == 0; a null here crashed the compiler's CFG simplification)
  if (xs.P > 0) {
    const long par = (xs.cnt[s] / xs.F) & 1;
    p.a = xs.a + par * xs.alt + s * xs.lda;
  }
  p.b = xs.b + s * xs.ldb;
  p.t0 = j * xs.hop;
  p.P = xs.P;
  return p;
}

template <int ACT>
__device__ __forceinline__ float act_of(float v) {
  if (ACT == 1) v = fmaxf(v, 0.f);
  if (ACT == 2) v = tanhf(v);
  return v;
}

// acc[i][h] = sum_k x_i[k] * W_h[k] as one fmaf chain in ascending k, for NH weight rows (wr[h]) and R rows of x.
template <int R, int NH, int U, bool VEC>
__device__ __forceinline__ void chains(const RowPtr (&xr)[R], const float* const (&wr)[NH], long K, float (&acc)[R][NH]) {
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int h = 0; h < NH; ++h) acc[i][h] = 0.f;
  long k = 0;
  if constexpr (VEC) {
    constexpr int Q = U / 4;
    const long KC = K - K % U;
    if (KC > 0) {
      float4 wc[NH][Q], xc[R][Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
#pragma unroll
        for (int h = 0; h < NH; ++h) wc[h][q] = *reinterpret_cast<const float4*>(wr[h] + 4 * q);
#pragma unroll
        for (int i = 0; i < R; ++i) xc[i][q] = xr[i].ld4(4 * q);
      }
      for (; k < KC; k += U) {
        // the next chunk's loads are issued before this chunk's FMAs
        float4 wn[NH][Q], xn[R][Q];
        const long kn = k + U < KC ? k + U : k;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
#pragma unroll
          for (int h = 0; h < NH; ++h) wn[h][q] = *reinterpret_cast<const float4*>(wr[h] + kn + 4 * q);
#pragma unroll
          for (int i = 0; i < R; ++i) xn[i][q] = xr[i].ld4(kn + 4 * q);
        }
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
          for (int i = 0; i < R; ++i)
#pragma unroll
            for (int h = 0; h < NH; ++h) {
              acc[i][h] = fmaf(xc[i][q].x, wc[h][q].x, acc[i][h]);
              acc[i][h] = fmaf(xc[i][q].y, wc[h][q].y, acc[i][h]);
              acc[i][h] = fmaf(xc[i][q].z, wc[h][q].z, acc[i][h]);
              acc[i][h] = fmaf(xc[i][q].w, wc[h][q].w, acc[i][h]);
            }
#pragma unroll
        for (int q = 0; q < Q; ++q) {
#pragma unroll
          for (int h = 0; h < NH; ++h) wc[h][q] = wn[h][q];
#pragma unroll
          for (int i = 0; i < R; ++i) xc[i][q] = xn[i][q];
        }
      }
    }
  }
  for (; k < K; ++k) {
    float wk[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) wk[h] = wr[h][k];
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const float xk = xr[i].ld1(k);
#pragma unroll
      for (int h = 0; h < NH; ++h) acc[i][h] = fmaf(xk, wk[h], acc[i][h]);
    }
  }
}

// grid (ceil(N / 64), ceil(M / R)), one wave per workgroup: lane = output column, R consecutive rows per workgroup.
template <int ACT, int R, bool VEC>
__global__ void __launch_bounds__(64)
k_small_linear(Rows xs, const float* __restrict__ w, long ldw, const float* __restrict__ bias, long M, long N, long K,
               float* __restrict__ y, long ldy) {
  const long n = (long)blockIdx.x * 64 + threadIdx.x;
  const long nc = n < N ? n : N - 1;   // lanes past N walk the last row and store nothing
  const long r0 = (long)blockIdx.y * R;
  RowPtr xr[R];
#pragma unroll
  for (int i = 0; i < R; ++i) xr[i] = row_ptr(xs, r0 + i < M ? r0 + i : M - 1);
  const float* const wr[1] = {w + nc * ldw};
  float acc[R][1];
  chains<R, 1, KU, VEC>(xr, wr, K, acc);
  if (n >= N) return;
  const float b = bias ? bias[n] : 0.f;
#pragma unroll
  for (int i = 0; i < R; ++i)
    if (r0 + i < M) y[(r0 + i) * ldy + n] = act_of<ACT>(acc[i][0] + b);
}

// mu' = mu * scale + offset with both roundings (torch's two ops; no contraction)
__device__ __forceinline__ float latent_ctl(float m, float sc, float of) {
#pragma clang fp contract(off)
  return m * sc + of;
}

// fc21 and fc22 (lane = latent index l, both weight rows), then per row: the controls and the reparameterisation.
// REPARAM false (the live mosaic's query): z = mu' alone; eps, seed and temperature are not read.
template <int R, bool VEC, bool REPARAM>
__global__ void __launch_bounds__(64)
k_stream_heads(const float* __restrict__ h1, long H, const float* __restrict__ w21, const float* __restrict__ b21,
               const float* __restrict__ w22, const float* __restrict__ b22, long M, long L, long F,
               const long long* __restrict__ cnt, const float* __restrict__ eps_in, uint64_t seed,
               const float* __restrict__ scale, const float* __restrict__ offset, const float* __restrict__ temperature,
               float* __restrict__ mu, float* __restrict__ lv, float* __restrict__ z) {
  const long l = (long)blockIdx.x * 64 + threadIdx.x;
  const long lc = l < L ? l : L - 1;
  const long r0 = (long)blockIdx.y * R;
  Rows xs{nullptr, h1, 0, 0, 0, M, H, 0, nullptr};
  RowPtr xr[R];
#pragma unroll
  for (int i = 0; i < R; ++i) xr[i] = row_ptr(xs, r0 + i < M ? r0 + i : M - 1);
  const float* const wr[2] = {w21 + lc * H, w22 + lc * H};
  float acc[R][2];
  chains<R, 2, KU_HEADS, VEC>(xr, wr, H, acc);
  if (l >= L) return;
  const float bm = b21[l], bl = b22[l];
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const long r = r0 + i;
    if (r >= M) continue;
    const long s = r / F, f = cnt[s] + (r - s * F);
    const float m = acc[i][0] + bm, v = acc[i][1] + bl;
    const float mc = latent_ctl(m, scale[s * L + l], offset[s * L + l]);
    if constexpr (REPARAM) {
      const float e = eps_in ? eps_in[r * L + l] : normal1(seed, (uint64_t)(f * L + l), (uint64_t)s);
      z[r * L + l] = reparam_z(mc, v, temperature[s] * e);
    } else {
      z[r * L + l] = mc;
    }
    mu[r * L + l] = m;
    lv[r * L + l] = v;
  }
}

__device__ __forceinline__ float wola_add(float num, float w, float d) {
#pragma clang fp contract(off)
  return num + w * d;
}

// One workgroup per stream.  Positions u of [0, block + P) relative to this call's first output sample: u < block is
// output, the rest the next call's tail.  Numerator: the old tail (u < P) or +0, then the products of the frames that
// cover u in ascending frame order.  The history of the next call is the last P samples of [history | x].
__global__ void __launch_bounds__(256)
k_stream_ola(const float* __restrict__ dec, const float* __restrict__ window, const float* __restrict__ norm, long NS,
             long S, long hop, long block, long F, long P, const float* __restrict__ x, long ld_x, float* __restrict__ y,
             long ld_y, float* __restrict__ carry, float* __restrict__ tail, long long* __restrict__ cnt) {
  const long s = blockIdx.x;
  const long long c = cnt[s];
  const long par = (c / F) & 1;
  const float* car_o = carry + par * NS * P + s * P;
  float* car_n = carry + (1 - par) * NS * P + s * P;
  const float* tail_o = tail + par * NS * P + s * P;
  float* tail_n = tail + (1 - par) * NS * P + s * P;
  const long T0 = (long)c * hop;
  const float* d = dec + s * F * S;
  for (long u = threadIdx.x; u < block + P; u += 256) {
    float num = u < P ? tail_o[u] : 0.f;
    const long jlo = u >= S ? (u - S) / hop + 1 : 0;
    const long jhi = u / hop < F - 1 ? u / hop : F - 1;
    for (long j = jlo; j <= jhi; ++j) {
      const long o = u - j * hop;
      num = wola_add(num, window[o], d[j * S + o]);
    }
    if (u < block) {
      const long t = T0 + u;
      const float den = t < P ? norm[t] : norm[P + t % hop];
      y[s * ld_y + u] = den == 0.f ? 0.f : num / den;
    } else {
      tail_n[u - block] = num;
    }
  }
  for (long i = threadIdx.x; i < P; i += 256) {
    const long src = block + i;
    car_n[i] = src < P ? car_o[src] : x[s * ld_x + (src - P)];
  }
  __syncthreads();   // every thread has read cnt[s]
  if (threadIdx.x == 0) cnt[s] = c + F;
}

__global__ void __launch_bounds__(256)
k_stream_reset(float* __restrict__ carry, float* __restrict__ tail, long long* __restrict__ cnt, long NS, long P,
               long first) {
  const long s = first + blockIdx.x;
  for (long i = threadIdx.x; i < P; i += 256) {
    carry[s * P + i] = 0.f;
    carry[(NS + s) * P + i] = 0.f;
    tail[s * P + i] = 0.f;
    tail[(NS + s) * P + i] = 0.f;
  }
  if (threadIdx.x == 0) cnt[s] = 0;
}

// ---- host side ----
int rows_per_group(long M, int cap) {
  int R = 1;
  while (R < cap && (M + R - 1) / R > 8) R *= 2;
  return R;
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <int ACT, int R>
void launch_linear_r(const Rows& xs, bool vec, const float* w, long ldw, const float* b, long M, long N, long K,
                     float* y, long ldy, hipStream_t st) {
  const dim3 g((unsigned)((N + 63) / 64), (unsigned)((M + R - 1) / R));
  if (vec) hipLaunchKernelGGL((k_small_linear<ACT, R, true>), g, dim3(64), 0, st, xs, w, ldw, b, M, N, K, y, ldy);
  else hipLaunchKernelGGL((k_small_linear<ACT, R, false>), g, dim3(64), 0, st, xs, w, ldw, b, M, N, K, y, ldy);
}

template <int ACT>
void launch_linear_a(const Rows& xs, bool vec, const float* w, long ldw, const float* b, long M, long N, long K,
                     float* y, long ldy, hipStream_t st) {
  switch (rows_per_group(M, 8)) {
    case 1: launch_linear_r<ACT, 1>(xs, vec, w, ldw, b, M, N, K, y, ldy, st); break;
    case 2: launch_linear_r<ACT, 2>(xs, vec, w, ldw, b, M, N, K, y, ldy, st); break;
    case 4: launch_linear_r<ACT, 4>(xs, vec, w, ldw, b, M, N, K, y, ldy, st); break;
    default: launch_linear_r<ACT, 8>(xs, vec, w, ldw, b, M, N, K, y, ldy, st); break;
  }
}

int launch_linear(const Rows& xs, bool vec_x, const float* w, long ldw, const float* b, long M, long N, long K,
                  int act, float* y, long ldy, hipStream_t st) {
  const bool vec = vec_x && al16(w) && ldw % 4 == 0;
  if (act == 0) launch_linear_a<0>(xs, vec, w, ldw, b, M, N, K, y, ldy, st);
  if (act == 1) launch_linear_a<1>(xs, vec, w, ldw, b, M, N, K, y, ldy, st);
  if (act == 2) launch_linear_a<2>(xs, vec, w, ldw, b, M, N, K, y, ldy, st);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

long grid_rows_ok(long M) { return (M + rows_per_group(M, 8) - 1) / rows_per_group(M, 8) <= 65535; }

// Workspace: counters [NS] int64, then h1 / h3 [M, H], z [M, L], dec [M, S], history and tail [2, NS, P] each.
struct Ws {
  long long* cnt;
  float *h1, *h3, *z, *dec, *carry, *tail;
};

long ws_layout(long S, long H, long L, long NS, long block, long hop, char* base, Ws* w) {
  const long M = NS * (block / hop), P = S - hop;
  const long sizes[7] = {NS * 8, M * H * 4, M * H * 4, M * L * 4, M * S * 4, 2 * NS * P * 4, 2 * NS * P * 4};
  long off[7], o = 0;
  for (int i = 0; i < 7; ++i) {
    off[i] = o;
    o += up256(sizes[i]);
  }
  if (w) {
    w->cnt = (long long*)(base + off[0]);
    w->h1 = (float*)(base + off[1]);
    w->h3 = (float*)(base + off[2]);
    w->z = (float*)(base + off[3]);
    w->dec = (float*)(base + off[4]);
    w->carry = (float*)(base + off[5]);
    w->tail = (float*)(base + off[6]);
  }
  return o;
}

bool extents_ok(long S, long H, long L, long NS, long block, long hop) {
  return S > 0 && H > 0 && L > 0 && NS > 0 && hop > 0 && block > 0 && S % hop == 0 && block % hop == 0 &&
         NS <= 0x7fffffffL && NS * (block / hop) <= 0x7fffffffL;
}

// The argument checks of a block call; `who` names the caller in the message.  The live mosaic reads no temperature.
int stream_check(const rv_stream_desc* d, const char* who, bool reparam) {
  RV_REQUIRE(d, RV_ERR_NULL, "%s: null descriptor", who);
  const long S = d->S, H = d->H, L = d->L, NS = d->n_streams, block = d->block, hop = d->hop;
  RV_REQUIRE(extents_ok(S, H, L, NS, block, hop) && block >= hop, RV_ERR_SHAPE,
             "%s: bad extents S=%ld H=%ld L=%ld n_streams=%ld block=%ld hop=%ld (S %% hop == 0, "
             "block %% hop == 0, block >= hop)", who, S, H, L, NS, block, hop);
  RV_REQUIRE(d->w1 && d->b1 && d->w21 && d->b21 && d->w22 && d->b22 && d->w3 && d->b3 && d->w4 && d->b4, RV_ERR_NULL,
             "%s: null weight", who);
  RV_REQUIRE(d->x && d->y && d->mu && d->logvar && d->scale && d->offset && (d->temperature || !reparam) && d->window &&
                 d->norm && d->workspace, RV_ERR_NULL, "%s: null buffer", who);
  RV_REQUIRE(d->ld_x >= block && d->ld_y >= block, RV_ERR_SHAPE, "%s: ld_x=%ld ld_y=%ld < block %ld", who, d->ld_x,
             d->ld_y, block);
  RV_REQUIRE(grid_rows_ok(NS * (block / hop)) && (S + 63) / 64 <= 65535 && (H + 63) / 64 <= 65535, RV_ERR_SHAPE,
             "%s: %ld rows exceed the launch grid", who, NS * (block / hop));
  return RV_OK;
}

// fc1 on the frames of [history | x] of every stream, then the heads: z_out = the reparameterised z, or mu' alone
template <bool REPARAM>
int stream_encode(const rv_stream_desc* d, const Ws& w, float* z_out, hipStream_t st) {
  const long S = d->S, H = d->H, L = d->L, NS = d->n_streams, hop = d->hop;
  const long F = d->block / hop, M = NS * F, P = S - hop;
  const Rows fr{w.carry, d->x, P, d->ld_x, NS * P, F, hop, P, w.cnt};
  const bool vec1 = al16(d->x) && al16(w.carry) && d->ld_x % 4 == 0 && hop % 4 == 0 && P % 4 == 0;
  const int rc = launch_linear(fr, vec1, d->w1, S, d->b1, M, H, S, 1, w.h1, H, st);
  if (rc) return rc;
  const bool vec = al16(w.h1) && al16(d->w21) && al16(d->w22) && H % 4 == 0;
  const int R = rows_per_group(M, 4);
  const dim3 g((unsigned)((L + 63) / 64), (unsigned)((M + R - 1) / R));
#define RV_HEADS(RR, V)                                                                                                \
  hipLaunchKernelGGL((k_stream_heads<RR, V, REPARAM>), g, dim3(64), 0, st, w.h1, H, d->w21, d->b21, d->w22, d->b22, M, \
                     L, F, w.cnt, d->eps_in, (uint64_t)d->seed, d->scale, d->offset, d->temperature, d->mu, d->logvar, \
                     z_out)
  if (vec) {
    if (R == 1) RV_HEADS(1, true); else if (R == 2) RV_HEADS(2, true); else RV_HEADS(4, true);
  } else {
    if (R == 1) RV_HEADS(1, false); else if (R == 2) RV_HEADS(2, false); else RV_HEADS(4, false);
  }
#undef RV_HEADS
  RV_CHECK_LAUNCH();
  return RV_OK;
}

// (decode: fc3 and fc4 on w.z into w.dec, then) overlap-add of w.dec + history update
int stream_synth(const rv_stream_desc* d, const Ws& w, bool decode, hipStream_t st) {
  const long S = d->S, H = d->H, L = d->L, NS = d->n_streams, hop = d->hop, block = d->block;
  const long F = block / hop, M = NS * F, P = S - hop;
  if (decode) {
    const Rows zr{nullptr, w.z, 0, 0, 0, M, L, 0, nullptr};
    int rc = launch_linear(zr, L % 4 == 0, d->w3, L, d->b3, M, H, L, 1, w.h3, H, st);
    if (rc) return rc;
    const Rows hr{nullptr, w.h3, 0, 0, 0, M, H, 0, nullptr};
    rc = launch_linear(hr, H % 4 == 0, d->w4, H, d->b4, M, S, H, 2, w.dec, S, st);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_stream_ola, dim3((unsigned)NS), dim3(256), 0, st, w.dec, d->window, d->norm, NS, S, hop, block,
                     F, P, d->x, d->ld_x, d->y, d->ld_y, w.carry, w.tail, w.cnt);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

}  // namespace

extern "C" int rv_small_linear_f32(const float* x, long ldx, const float* w, long ldw, const float* bias, long M,
                                   long N, long K, int act, float* y, long ldy, void* stream) {
  RV_REQUIRE(x && w && y, RV_ERR_NULL, "rv_small_linear_f32: null operand");
  RV_REQUIRE(M > 0 && N > 0 && K > 0 && ldx >= 1 && ldw >= K && ldy >= N, RV_ERR_SHAPE,
             "rv_small_linear_f32: bad extents M=%ld N=%ld K=%ld ldx=%ld ldw=%ld ldy=%ld", M, N, K, ldx, ldw, ldy);
  RV_REQUIRE(act >= 0 && act <= 2, RV_ERR_UNSUPPORTED, "rv_small_linear_f32: act %d (0 none, 1 relu, 2 tanh)", act);
  RV_REQUIRE((N + 63) / 64 <= 0x7fffffffL && grid_rows_ok(M), RV_ERR_SHAPE,
             "rv_small_linear_f32: %ld rows exceed the launch grid", M);
  const Rows xs{nullptr, x, 0, 0, 0, M, ldx, 0, nullptr};
  return launch_linear(xs, al16(x) && ldx % 4 == 0, w, ldw, bias, M, N, K, act, y, ldy, (hipStream_t)stream);
}

extern "C" long rv_stream_workspace_bytes(long S, long H, long L, long n_streams, long block, long hop) {
  if (!extents_ok(S, H, L, n_streams, block, hop) || block < hop) return -1;
  return ws_layout(S, H, L, n_streams, block, hop, nullptr, nullptr);
}

extern "C" int rv_stream_process(const rv_stream_desc* d, void* stream) {
  int rc = stream_check(d, "rv_stream_process", true);
  if (rc) return rc;
  Ws w;
  ws_layout(d->S, d->H, d->L, d->n_streams, d->block, d->hop, (char*)d->workspace, &w);
  rc = stream_encode<true>(d, w, w.z, (hipStream_t)stream);
  if (rc) return rc;
  return stream_synth(d, w, true, (hipStream_t)stream);
}

RV_INTERNAL int rv_stream_encode(const rv_stream_desc* d, float* q, float** z, float** frames, void* stream) {
  const int rc = stream_check(d, "rv_mosaic(LIVE)", false);
  if (rc) return rc;
  Ws w;
  ws_layout(d->S, d->H, d->L, d->n_streams, d->block, d->hop, (char*)d->workspace, &w);
  *z = w.z;
  *frames = w.dec;
  if (!q) return RV_OK;
  return stream_encode<false>(d, w, q, (hipStream_t)stream);
}

RV_INTERNAL const long long* rv_stream_counters(const rv_stream_desc* d) {
  Ws w;
  ws_layout(d->S, d->H, d->L, d->n_streams, d->block, d->hop, (char*)d->workspace, &w);
  return w.cnt;
}

RV_INTERNAL int rv_stream_synth(const rv_stream_desc* d, int decode, void* stream) {
  Ws w;
  ws_layout(d->S, d->H, d->L, d->n_streams, d->block, d->hop, (char*)d->workspace, &w);
  return stream_synth(d, w, decode != 0, (hipStream_t)stream);
}

extern "C" int rv_stream_reset(const rv_stream_desc* d, long which, void* stream) {
  RV_REQUIRE(d && d->workspace, RV_ERR_NULL, "rv_stream_reset: null descriptor or workspace");
  const long S = d->S, NS = d->n_streams, hop = d->hop;
  RV_REQUIRE(extents_ok(S, d->H, d->L, NS, d->block, hop) && d->block >= hop, RV_ERR_SHAPE,
             "rv_stream_reset: bad extents");
  RV_REQUIRE(which >= -1 && which < NS, RV_ERR_SHAPE, "rv_stream_reset: stream %ld of %ld", which, NS);
  Ws w;
  ws_layout(S, d->H, d->L, NS, d->block, hop, (char*)d->workspace, &w);
  const long first = which < 0 ? 0 : which, n = which < 0 ? NS : 1;
  hipLaunchKernelGGL(k_stream_reset, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, w.carry, w.tail, w.cnt, NS,
                     S - hop, first);
  RV_CHECK_LAUNCH();
  return RV_OK;
}
