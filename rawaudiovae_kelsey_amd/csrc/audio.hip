// Audio ingest on the device: WAV payload bytes -> fp32 channel 0 (rv_pcm_to_f32), and the windowed-sinc polyphase
// resampler of torchaudio.functional.resample (rv_resample_sinc_hann), the two host steps of dataset.py:47-58 that the
// streaming loader otherwise runs on the CPU (data.read_wav + data._resample_sinc_hann).
#include "common.h"
#include "../../include/rawvae_hip.h"

using namespace rv;

namespace {

// ---- rv_pcm_to_f32 ----------------------------------------------------------------------------------------------
// A byte-stream kernel: thread t owns the channel-0 samples whose first byte lies in [16 t, 16 t + 16) and reads the
// two aligned 16-byte pieces [16 t, 16 t + 32) (a sample is at most 8 bytes, so it ends inside them).  Pieces that
// reach past the payload are read byte by byte up to its end.
constexpr int PCM_THREADS = 256;

__device__ __forceinline__ uint32_t byte_window(const uint32_t (&w)[8], int q) {
  // w[q] for a small run-time q without an indexed register array (which would go to scratch)
  uint32_t r = w[0];
#pragma unroll
  for (int i = 1; i < 8; ++i) r = q == i ? w[i] : r;
  return r;
}

template <int BPS, int KIND>   // KIND: 0 PCM, 1 IEEE float
__device__ __forceinline__ float pcm_sample(const uint32_t (&w)[8], int o) {
  const int q = o >> 2, sh = (o & 3) * 8;
  const uint32_t w0 = byte_window(w, q), w1 = byte_window(w, q + 1);
  // bytes o .. o + 3 of the window, little-endian
  const uint32_t lo = sh ? (w0 >> sh) | (w1 << (32 - sh)) : w0;
  if constexpr (BPS == 1) {
    return ((float)(lo & 0xffu) - 128.0f) * 0.0078125f;           // (x - 128) / 128, exact
  } else if constexpr (BPS == 2) {
    return (float)(int16_t)(lo & 0xffffu) * 3.0517578125e-05f;    // x / 2^15, exact
  } else if constexpr (BPS == 3) {
    return (float)(int32_t)(lo << 8) * 4.656612873077393e-10f;    // scipy's left-justified int32 / 2^31, exact
  } else if constexpr (BPS == 4) {
    if constexpr (KIND == 1) return __uint_as_float(lo);
    return (float)(int32_t)lo * 4.656612873077393e-10f;           // RNE to fp32, then / 2^31 (exact)
  } else {   // 8-byte IEEE float: 8-byte aligned in the payload (o is 0 or 8), so lo = w0
    const unsigned long long b = (unsigned long long)w1 << 32 | w0;
    return (float)__longlong_as_double((long long)b);             // RNE, as numpy's astype(float32)
  }
}

template <int BPS, int KIND>
__global__ __launch_bounds__(PCM_THREADS) void k_pcm_to_f32(const uint8_t* __restrict__ src, long nbytes,
                                                            long block_align, long n, float* __restrict__ out,
                                                            long n_out) {
  const long t = (long)blockIdx.x * PCM_THREADS + threadIdx.x;
  const long b0 = t * 16;
  if (b0 < nbytes) {
    uint32_t w[8];
    if (b0 + 32 <= nbytes) {
      const uint4 a = *reinterpret_cast<const uint4*>(src + b0);
      const uint4 c = *reinterpret_cast<const uint4*>(src + b0 + 16);
      w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = c.x; w[5] = c.y; w[6] = c.z; w[7] = c.w;
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const long b = b0 + 4 * i + k;
          if (b < nbytes) v |= (uint32_t)src[b] << (8 * k);
        }
        w[i] = v;
      }
    }
    // channel-0 samples starting in [b0, b0 + 16): frames ceil(b0 / ba) ..
    for (long f = (b0 + block_align - 1) / block_align; f < n && f * block_align < b0 + 16; ++f)
      out[f] = pcm_sample<BPS, KIND>(w, (int)(f * block_align - b0));
  }
  // the zero padding up to n_out
  const long stride = (long)gridDim.x * PCM_THREADS;
  for (long f = n + t; f < n_out; f += stride) out[f] = 0.f;
}

// ---- rv_resample_sinc_hann --------------------------------------------------------------------------------------
// out[j * new + i] = sum_k bank[i][k] * xp[j * orig + k], xp = the input with `width` zeros in front (and zeros past
// its end).  A block computes RS_PT phases (one per lane) x RS_JT frames (RS_R per thread, a wave per RS_R frames);
// the taps run in chunks of RS_KC: per chunk the block stages the phases' filter pieces (rows padded to 68 floats, so
// the 16-byte reads of 64 lanes down a column hit every bank once) and, per frame, its piece of the input window
// (read by the whole wave at one address: a broadcast).  fp32 operands, fp32 fmaf accumulation in tap order.
constexpr int RS_PT = 64, RS_WAVES = 4, RS_R = 8, RS_JT = RS_WAVES * RS_R, RS_KC = 64, RS_LDW = RS_KC + 4;
constexpr int RS_THREADS = RS_WAVES * WAVE;

__global__ __launch_bounds__(RS_THREADS) void k_resample_sinc_hann(const float* __restrict__ x, long n,
                                                                    const float* __restrict__ bank, long orig, long nw,
                                                                    long width, long taps, long target,
                                                                    float* __restrict__ out, long n_out) {
  __shared__ __attribute__((aligned(16))) float wb[RS_PT * RS_LDW];
  __shared__ __attribute__((aligned(16))) float xs[RS_JT * RS_KC];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long j0 = (long)blockIdx.x * RS_JT, i0 = (long)blockIdx.y * RS_PT;
  float acc[RS_R];
#pragma unroll
  for (int r = 0; r < RS_R; ++r) acc[r] = 0.f;

  for (long k0 = 0; k0 < taps; k0 += RS_KC) {
    // filter pieces: element e = p * RS_KC + kk, taps fastest (contiguous in the bank's rows)
    for (int e = tid; e < RS_PT * RS_KC; e += RS_THREADS) {
      const int p = e / RS_KC, kk = e % RS_KC;
      const long i = i0 + p, k = k0 + kk;
      wb[p * RS_LDW + kk] = (i < nw && k < taps) ? bank[i * taps + k] : 0.f;
    }
    // input pieces: frame r reads xp[(j0 + r) * orig + k0 + kk] = x[... - width], zero outside [0, n)
    for (int e = tid; e < RS_JT * RS_KC; e += RS_THREADS) {
      const int r = e / RS_KC, kk = e % RS_KC;
      const long pos = (j0 + r) * orig + k0 + kk - width;
      xs[e] = (k0 + kk < taps && pos >= 0 && pos < n) ? x[pos] : 0.f;
    }
    __syncthreads();
    const float* wrow = wb + lane * RS_LDW;
    const float* xrow = xs + wv * RS_R * RS_KC;
#pragma unroll 4
    for (int kk = 0; kk < RS_KC; kk += 4) {
      const f32x4 w4 = *reinterpret_cast<const f32x4*>(wrow + kk);
#pragma unroll
      for (int r = 0; r < RS_R; ++r) {
        const f32x4 x4 = *reinterpret_cast<const f32x4*>(xrow + r * RS_KC + kk);
        acc[r] = fmaf(w4[0], x4[0], acc[r]);
        acc[r] = fmaf(w4[1], x4[1], acc[r]);
        acc[r] = fmaf(w4[2], x4[2], acc[r]);
        acc[r] = fmaf(w4[3], x4[3], acc[r]);
      }
    }
    __syncthreads();
  }
  const long i = i0 + lane;
  if (i >= nw) return;
#pragma unroll
  for (int r = 0; r < RS_R; ++r) {
    const long m = (j0 + wv * RS_R + r) * nw + i;
    if (m < n_out) out[m] = m < target ? acc[r] : 0.f;
  }
}

}  // namespace

extern "C" {

int rv_pcm_to_f32(const void* src, long nbytes, int format, int channels, int bytes_per_sample, long hop, float* out,
                  long n_out, void* stream) {
  RV_REQUIRE(nbytes >= 0 && channels >= 1 && hop >= 1, RV_ERR_SHAPE, "rv_pcm_to_f32: bad extents");
  RV_REQUIRE(format == RV_WAV_PCM || format == RV_WAV_FLOAT, RV_ERR_UNSUPPORTED, "rv_pcm_to_f32: format %d", format);
  const int bps = bytes_per_sample;
  const bool ok = format == RV_WAV_PCM ? (bps >= 1 && bps <= 4) : (bps == 4 || bps == 8);
  RV_REQUIRE(ok, RV_ERR_UNSUPPORTED, "rv_pcm_to_f32: %d-byte %s samples", bps, format == RV_WAV_PCM ? "PCM" : "float");
  const long ba = (long)channels * bps;
  const long n = nbytes / ba;
  const long padded = (n + hop - 1) / hop * hop;
  RV_REQUIRE(n_out == padded, RV_ERR_SHAPE, "rv_pcm_to_f32: n_out %ld, expected %ld (%ld frames padded to hop %ld)",
             n_out, padded, n, hop);
  if (n_out == 0) return RV_OK;
  RV_REQUIRE(out, RV_ERR_NULL, "rv_pcm_to_f32: null output");
  RV_REQUIRE(nbytes == 0 || src, RV_ERR_NULL, "rv_pcm_to_f32: null source");
  RV_REQUIRE(((uintptr_t)src & 15) == 0, RV_ERR_SHAPE, "rv_pcm_to_f32: source must be 16-byte aligned");
  const long pieces = (nbytes + 15) / 16;
  const long zero_threads = n_out - n;
  const long threads = pieces > zero_threads ? pieces : zero_threads;
  long blocks = (threads + PCM_THREADS - 1) / PCM_THREADS;
  RV_REQUIRE(blocks <= 0x7fffffffL, RV_ERR_SHAPE, "rv_pcm_to_f32: payload too large");
  const hipStream_t s = (hipStream_t)stream;
  const uint8_t* p = (const uint8_t*)src;
#define RV_PCM_LAUNCH(B, K) \
  hipLaunchKernelGGL((k_pcm_to_f32<B, K>), dim3((unsigned)blocks), dim3(PCM_THREADS), 0, s, p, nbytes, ba, n, out, n_out)
  if (format == RV_WAV_FLOAT) {
    if (bps == 4) RV_PCM_LAUNCH(4, 1);
    else RV_PCM_LAUNCH(8, 1);
  } else {
    switch (bps) {
      case 1: RV_PCM_LAUNCH(1, 0); break;
      case 2: RV_PCM_LAUNCH(2, 0); break;
      case 3: RV_PCM_LAUNCH(3, 0); break;
      default: RV_PCM_LAUNCH(4, 0); break;
    }
  }
#undef RV_PCM_LAUNCH
  RV_CHECK_LAUNCH();
  return RV_OK;
}

int rv_resample_sinc_hann(const float* src, long n, const float* bank, long orig, long new_, long width, float* out,
                          long n_out, void* stream) {
  RV_REQUIRE(n >= 0 && orig >= 1 && new_ >= 1 && width >= 0 && n_out >= 0, RV_ERR_SHAPE,
             "rv_resample_sinc_hann: bad extents");
  RV_REQUIRE(orig != new_, RV_ERR_SHAPE, "rv_resample_sinc_hann: equal rates (the caller keeps its input)");
  // ceil(new * n / orig) outputs are kept
  RV_REQUIRE(n <= (1L << 40) && new_ <= (1L << 20) && orig <= (1L << 20), RV_ERR_SHAPE,
             "rv_resample_sinc_hann: extents out of range");
  const long target = (new_ * n + orig - 1) / orig;
  RV_REQUIRE(n_out >= target, RV_ERR_SHAPE, "rv_resample_sinc_hann: n_out %ld < %ld outputs", n_out, target);
  if (n_out == 0) return RV_OK;
  RV_REQUIRE(bank && out && (n == 0 || src), RV_ERR_NULL, "rv_resample_sinc_hann: null pointer");
  const long taps = 2 * width + orig;
  const long frames = (n_out + new_ - 1) / new_;
  const long gx = (frames + RS_JT - 1) / RS_JT, gy = (new_ + RS_PT - 1) / RS_PT;
  RV_REQUIRE(gx <= 0x7fffffffL && gy <= 65535, RV_ERR_SHAPE, "rv_resample_sinc_hann: grid too large");
  hipLaunchKernelGGL(k_resample_sinc_hann, dim3((unsigned)gx, (unsigned)gy), dim3(RS_THREADS), 0, (hipStream_t)stream,
                     src, n, bank, orig, new_, width, taps, target, out, n_out);
  RV_CHECK_LAUNCH();
  return RV_OK;
}

}  // extern "C"
