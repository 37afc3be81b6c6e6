// Host-side checks of the C ABI under AddressSanitizer + UBSan (tests/test_host_cpu.py builds the four
// translation units with `-fsanitize=address,undefined -fno-gpu-sanitize` and runs this on the CPU):
// tile/split pickers over a sweep of extents, and the argument validation / error paths that return
// before any HIP call.  No GPU needed.
#include <stdio.h>
#include <string.h>
#include "rawvae_hip.h"
#include "../../rawaudiovae_kelsey_amd/csrc/internal.h"   // the step plan's launchers (hidden symbols of the objects linked here)

// `rc` is the expected error code and the message starts with `prefix`
static int expect(int rc, int code, const char* prefix, int line) {
  if (rc == code && strncmp(rv_last_error(), prefix, strlen(prefix)) == 0) return 0;
  printf("line %d: got %d \"%s\", expected %d \"%s...\"\n", line, rc, rv_last_error(), code, prefix);
  return 1;
}
#define EXPECT(call, code, prefix) expect((call), (code), (prefix), __LINE__)

// A leading dimension smaller than the row width it belongs to (rows would overlap) is RV_ERR_SHAPE before any launch, for
// every operand and every output of the bf16 GEMM entry points; each line has exactly one offending value, 8 (or 4) below
// its width, so the alignment rules are kept.  Extents (M, N, K) = (256, 256, 512).
static int ld_checks() {
  alignas(16) static char buf[64];
  float* f = (float*)buf;
  const long M = 256, N = 256, K = 512;
  const char* opnd = "operand leading dims";
  char msg[160];
  int fails = 0;
  snprintf(msg, sizeof msg, "rv_linear_fwd: %s", opnd);
  fails += EXPECT(rv_linear_fwd(buf, K - 8, buf, K, NULL, M, N, K, RV_ACT_RELU, buf, N, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_fwd(buf, K, buf, K - 8, NULL, M, N, K, RV_ACT_RELU, buf, N, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_fwd(buf, K, buf, K, NULL, M, N, K, RV_ACT_RELU, buf, N - 8, NULL), RV_ERR_SHAPE,
                  "rv_linear_fwd: output leading dim 248");
  snprintf(msg, sizeof msg, "rv_linear_fwd_f32: %s", opnd);
  fails += EXPECT(rv_linear_fwd_f32(buf, K - 8, buf, K, NULL, M, N, K, 2, f, N, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_fwd_f32(buf, K, buf, K - 8, NULL, M, N, K, 2, f, N, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_fwd_f32(buf, K, buf, K, NULL, M, N, K, 2, f, N - 4, NULL), RV_ERR_SHAPE,
                  "rv_linear_fwd_f32: output leading dim 252");
  // (a packed per-split K share is smaller than the row: the check is against the whole row, not the split's share)
  fails += EXPECT(rv_linear_fwd_f32(buf, K / 2, buf, K, NULL, M, N, K, 2, f, N, NULL), RV_ERR_SHAPE, msg);
  snprintf(msg, sizeof msg, "rv_decode_out_loss_fwd: %s", opnd);
  fails += EXPECT(rv_decode_out_loss_fwd(buf, K - 8, buf, K, NULL, M, N, K, M - 3, N - 5, f, N - 5, f, N - 5, buf, N, f, NULL, NULL),
                  RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_decode_out_loss_fwd(buf, K, buf, K - 8, NULL, M, N, K, M - 3, N - 5, f, N - 5, f, N - 5, buf, N, f, NULL, NULL),
                  RV_ERR_SHAPE, msg);
  const char* dec = "rv_decode_out_loss_fwd: leading dims of x / recon / dP4";
  fails += EXPECT(rv_decode_out_loss_fwd(buf, K, buf, K, NULL, M, N, K, M - 3, N - 5, f, N - 6, f, N - 5, buf, N, f, NULL, NULL),
                  RV_ERR_SHAPE, dec);
  fails += EXPECT(rv_decode_out_loss_fwd(buf, K, buf, K, NULL, M, N, K, M - 3, N - 5, f, N - 5, f, N - 6, buf, N, f, NULL, NULL),
                  RV_ERR_SHAPE, dec);
  fails += EXPECT(rv_decode_out_loss_fwd(buf, K, buf, K, NULL, M, N, K, M - 3, N - 5, f, N - 5, f, N - 5, buf, N - 8, f, NULL, NULL),
                  RV_ERR_SHAPE, dec);
  // dgrad: dy [M, K], w [K, N]
  snprintf(msg, sizeof msg, "rv_linear_dgrad: %s", opnd);
  fails += EXPECT(rv_linear_dgrad(buf, K - 8, buf, N, M, N, K, NULL, 0, NULL, 0, NULL, f, N, 2, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_dgrad(buf, K, buf, N - 8, M, N, K, NULL, 0, NULL, 0, NULL, f, N, 2, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_dgrad(buf, K, buf, N, M, N, K, NULL, 0, NULL, 0, NULL, f, N - 4, 2, NULL), RV_ERR_SHAPE,
                  "rv_linear_dgrad: slab leading dim 252");
  fails += EXPECT(rv_linear_dgrad(buf, K, buf, N, M, N, K, buf, N - 8, buf, N, NULL, NULL, 0, 1, NULL), RV_ERR_SHAPE,
                  "rv_linear_dgrad: leading dims of mask / dx (248, 256)");
  fails += EXPECT(rv_linear_dgrad(buf, K, buf, N, M, N, K, buf, N, buf, N - 8, NULL, NULL, 0, 1, NULL), RV_ERR_SHAPE,
                  "rv_linear_dgrad: leading dims of mask / dx (256, 248)");
  // wgrad: dy [K(batch), M], x [K, N]
  snprintf(msg, sizeof msg, "rv_linear_wgrad: %s", opnd);
  fails += EXPECT(rv_linear_wgrad(buf, M - 8, buf, N, M, N, K, 2, RV_TILE_AUTO, f, N, RV_SLAB_F32, NULL, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_wgrad(buf, M, buf, N - 8, M, N, K, 2, RV_TILE_AUTO, f, N, RV_SLAB_F32, NULL, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_wgrad(buf, M, buf, N, M, N, K, 2, RV_TILE_AUTO, f, N - 4, RV_SLAB_F32, NULL, NULL), RV_ERR_SHAPE,
                  "weight gradient: slab leading dim 252");
  fails += EXPECT(rv_linear_wgrad(buf, M, buf, N, M, N, K, 2, RV_TILE_AUTO, f, N + 4, RV_SLAB_F16, f, NULL), RV_ERR_SHAPE,
                  "weight gradient: slab leading dim 260");   // fp16 slabs: rows of whole 16-byte pieces
  // dgrad + wgrad of one layer: dy [M, K], w [K, N], x [M, N]
  int paired = 0, bm = 0, sp = 0;
  fails += rv_gemm_plan(RV_PLAN_PAIR, M, N, K, 0, &bm, NULL, &sp, &paired) != 0;
  snprintf(msg, sizeof msg, "rv_linear_dgrad_wgrad: %s", opnd);
  fails += EXPECT(rv_linear_dgrad_wgrad(buf, K - 8, buf, N, buf, N, M, N, K, buf, N, NULL, f, N, sp, RV_SLAB_F32, NULL, NULL),
                  RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_dgrad_wgrad(buf, K, buf, N - 8, buf, N, M, N, K, buf, N, NULL, f, N, sp, RV_SLAB_F32, NULL, NULL),
                  RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_dgrad_wgrad(buf, K, buf, N, buf, N - 8, M, N, K, buf, N, NULL, f, N, sp, RV_SLAB_F32, NULL, NULL),
                  RV_ERR_SHAPE, "rv_linear_dgrad_wgrad: leading dims of mask / dx (248, 256)");
  fails += EXPECT(rv_linear_dgrad_wgrad(buf, K, buf, N, buf, N, M, N, K, buf, N - 8, NULL, f, N, sp, RV_SLAB_F32, NULL, NULL),
                  RV_ERR_SHAPE, "rv_linear_dgrad_wgrad: leading dims of mask / dx (256, 248)");
  fails += EXPECT(rv_linear_dgrad_wgrad(buf, K, buf, N, buf, N, M, N, K, buf, N, NULL, f, N - 4, sp, RV_SLAB_F32, NULL, NULL),
                  RV_ERR_SHAPE, "weight gradient: slab leading dim 252");
  snprintf(msg, sizeof msg, "rv_linear_dgrad_wgrad_f32: %s", opnd);
  fails += EXPECT(rv_linear_dgrad_wgrad_f32(buf, K - 8, buf, N, buf, N, M, N, K, f, N, 1, f, N, 2, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_dgrad_wgrad_f32(buf, K, buf, N - 8, buf, N, M, N, K, f, N, 1, f, N, 2, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_dgrad_wgrad_f32(buf, K, buf, N, buf, N - 8, M, N, K, f, N, 1, f, N, 2, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_dgrad_wgrad_f32(buf, K, buf, N, buf, N, M, N, K, f, N - 4, 1, f, N, 2, NULL), RV_ERR_SHAPE,
                  "rv_linear_dgrad_wgrad_f32: slab leading dims 252 / 256");
  fails += EXPECT(rv_linear_dgrad_wgrad_f32(buf, K, buf, N, buf, N, M, N, K, f, N, 1, f, N - 4, 2, NULL), RV_ERR_SHAPE,
                  "rv_linear_dgrad_wgrad_f32: slab leading dims 256 / 252");
  return fails;
}

// The rejections of the GEMM launchers that return before any HIP call.
static int launcher_checks() {
  alignas(16) static char buf[64];
  const float* dq = (const float*)buf;   // non-NULL: fp8 operands
  const char* fp8_ld = "K and leading dims must be multiples of 128 / 16 fp8 elements";
  char msg[160];
  int fails = 0;
  // bias/ReLU forward (bf16, fp8, frames)
  fails += EXPECT(rv_linear_fwd(NULL, 1024, buf, 1024, NULL, 256, 256, 1024, RV_ACT_RELU, buf, 256, NULL), RV_ERR_NULL,
                  "rv_linear_fwd: null operand");
  fails += EXPECT(rv_linear_fwd_ex({buf, 1024, NULL, 1024, dq}, NULL, 256, 256, 1024, RV_ACT_RELU, buf, 256, NULL, 0, NULL, NULL,
                                   NULL, 0, NULL, NULL), RV_ERR_NULL, "rv_linear_fwd: null operand");
  snprintf(msg, sizeof msg, "rv_linear_fwd: %s", fp8_ld);
  fails += EXPECT(rv_linear_fwd_ex({buf, 1000, buf, 1024, dq}, NULL, 256, 256, 1024, RV_ACT_RELU, buf, 256, NULL, 0, NULL, NULL,
                                   NULL, 0, NULL, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_fwd_ex({buf, 1088, buf, 1088, dq}, NULL, 256, 256, 1088, RV_ACT_RELU, buf, 256, NULL, 0, NULL, NULL,
                                   NULL, 0, NULL, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_fwd_frames(NULL, NULL, 0, 256, 256, buf, 1024, NULL, 256, 256, 1024, RV_ACT_RELU, buf, 256, NULL, 0,
                                       NULL, NULL), RV_ERR_NULL, "rv_linear_fwd_frames: null operand");
  fails += EXPECT(rv_linear_fwd_frames(buf, NULL, 0, 260, 256, buf, 1024, NULL, 256, 256, 1024, RV_ACT_RELU, buf, 256, NULL, 0,
                                       NULL, NULL), RV_ERR_SHAPE, "rv_linear_fwd_frames: hop 260 must be a multiple of 8");
  // fc4 + tanh + loss forward
  fails += EXPECT(rv_decode_out_loss_fwd(NULL, 2048, buf, 2048, NULL, 256, 256, 2048, 256, 256, NULL, 0, NULL, 0, NULL, 0, NULL,
                                         NULL, NULL), RV_ERR_NULL, "rv_decode_out_loss_fwd: null operand");
  snprintf(msg, sizeof msg, "rv_decode_out_loss_fwd: %s", fp8_ld);
  fails += EXPECT(rv_decode_out_loss_fwd_ex({buf, 2008, buf, 2048, dq}, NULL, 256, 256, 2048, 256, 256, NULL, 0, NULL, NULL, 0, NULL,
                                            0, NULL, 0, NULL, NULL, NULL, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_decode_out_loss_fwd_ex({buf, 2112, buf, 2112, dq}, NULL, 256, 256, 2112, 256, 256, NULL, 0, NULL, NULL, 0, NULL,
                                            0, NULL, 0, NULL, NULL, NULL, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_decode_out_loss_fwd_ex({buf, 2048, buf, 2048, dq}, NULL, 256, 256, 2048, 256, 256, NULL, 0, NULL, NULL, 0, NULL,
                                            0, buf, 256, NULL, NULL, NULL, NULL), RV_ERR_SHAPE,
                  "rv_decode_out_loss_fwd: the fp8 image of dP4 belongs to the fp8 forward and needs its scale");
  // paired dgrad + wgrad (fc4's extents at B = 4096: the fp8 pair fits)
  int paired = 0, bm = 0, sp = 0;
  fails += rv_gemm_plan(RV_PLAN_PAIR, 4096, 2048, 1024, 0, &bm, NULL, &sp, &paired) != 0;
  fails += !rv_dgrad_wgrad_fp8_fits(4096, 2048, 1024, sp);
  fails += EXPECT(rv_linear_dgrad_wgrad(buf, 1024, buf, 2048, NULL, 2048, 4096, 2048, 1024, buf, 2048, NULL, buf, 2048, sp,
                                        RV_SLAB_F32, NULL, NULL), RV_ERR_NULL, "rv_linear_dgrad_wgrad: null operand");
  fails += EXPECT(rv_linear_dgrad_wgrad_ex({buf, 1024, buf, 2048, dq}, {buf, 1024, buf, 2048, dq}, NULL, 2048, 0, 4096, 2048, 1024,
                                           buf, 2048, NULL, buf, 2048, sp, RV_SLAB_F32, NULL, NULL),
                  RV_ERR_NULL, "rv_linear_dgrad_wgrad: null operand");
  snprintf(msg, sizeof msg, "rv_linear_dgrad_wgrad: %s", fp8_ld);
  fails += EXPECT(rv_linear_dgrad_wgrad_ex({buf, 1000, buf, 2048, dq}, {buf, 1000, buf, 2048, dq}, buf, 2048, 1, 4096, 2048, 1024,
                                           buf, 2048, NULL, buf, 2048, sp, RV_SLAB_F32, NULL, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_dgrad_wgrad_ex({buf, 1088, buf, 2048, dq}, {buf, 1088, buf, 2048, dq}, buf, 2048, 1, 4096, 2048, 1088,
                                           buf, 2048, NULL, buf, 2048, sp, RV_SLAB_F32, NULL, NULL), RV_ERR_SHAPE,
                  "rv_linear_dgrad_wgrad: 4096 x 2048 x 1088");
  // weight gradient + rider blocks (fc1's extents at B = 4096, 4 K splits)
  rv_param_desc d[1];
  memset(d, 0, sizeof d);
  const rv_rider_target adam = {(float*)buf, (float*)buf, (float*)buf, 1e-3f, 1.f, (const long long*)buf, NULL, 0};
  const rv_rider_target fin = {NULL, NULL, NULL, 0.f, 1.f, NULL, buf, 0};
  fails += EXPECT(rv_linear_wgrad_adam(buf, 2048, buf, 1024, 2048, 1024, 4096, 4, buf, 1024, RV_SLAB_F32, NULL, d, 1, NULL,
                                       (float*)buf, (float*)buf, 1e-3f, 1.f, (const long long*)buf, 128, NULL),
                  RV_ERR_NULL, "rv_linear_wgrad_adam: null pointer");
  fails += EXPECT(rv_linear_wgrad_riders({NULL, 2048, buf, 1024, dq}, 2048, 1024, 4096, 4, buf, 1024, RV_SLAB_F32, NULL, d, 1, fin,
                                         128, NULL), RV_ERR_NULL, "rv_linear_wgrad_riders: null pointer");
  snprintf(msg, sizeof msg, "rv_linear_wgrad_adam: %s", fp8_ld);
  fails += EXPECT(rv_linear_wgrad_riders({buf, 2008, buf, 1024, dq}, 2048, 1024, 4096, 4, buf, 1024, RV_SLAB_F32, NULL, d, 1, adam,
                                         128, NULL), RV_ERR_SHAPE, msg);
  fails += EXPECT(rv_linear_wgrad_riders({buf, 2048, buf, 1024, dq}, 2048, 1024, 4160, 4, buf, 1024, RV_SLAB_F32, NULL, d, 1, adam,
                                         128, NULL), RV_ERR_SHAPE, "rv_linear_wgrad_adam: 2048 x 1024 x 4160 / 4 splits does not tile");
  for (int n = 0; n <= 4097; n += 4097) {
    snprintf(msg, sizeof msg, "rv_linear_wgrad_adam: %d rider blocks", n);
    fails += EXPECT(rv_linear_wgrad_adam(buf, 2048, buf, 1024, 2048, 1024, 4096, 4, buf, 1024, RV_SLAB_F32, NULL, d, 1, (float*)buf,
                                         (float*)buf, (float*)buf, 1e-3f, 1.f, (const long long*)buf, n, NULL), RV_ERR_SHAPE, msg);
    snprintf(msg, sizeof msg, "rv_linear_wgrad_riders: %d rider blocks", n);
    fails += EXPECT(rv_linear_wgrad_riders({buf, 2048, buf, 1024, dq}, 2048, 1024, 4096, 4, buf, 1024, RV_SLAB_F32, NULL, d, 1, fin,
                                           n, NULL), RV_ERR_SHAPE, msg);
  }
  fails += ld_checks();
  // the reparameterisation launchers serve the padded latent widths rv_pad_dims produces (64, 128, 256) and nothing else:
  // any other width is RV_ERR_SHAPE before the launch (1 and 2 made the kernels divide by Lp / 4 == 0; 4 .. 32 and 512 passed
  // the old `Bp * Lp % 1024 == 0` / `256 % Lp == 0` rules)
  float* f = (float*)buf;
  const long long* ctr = (const long long*)buf;
  const long bad_lp[] = {1, 2, 3, 4, 8, 16, 32, 96, 192, 512, 0, -64};
  for (long lp : bad_lp) {
    const long L = lp < 1 ? 1 : (lp < 3 ? lp : 3);
    fails += EXPECT(rv_reparam_fwd(f, 1, 1024, lp, 100, L, NULL, f, 1, ctr, f, buf, f, NULL), RV_ERR_SHAPE,
                    "rv_reparam_fwd: the padded latent width must be 64, 128 or 256");
    fails += EXPECT(rv_reparam_bwd(f, 1, 1024, lp, 100, L, 512, f, f, 1e-4f, NULL, NULL, buf, f, NULL, 0, NULL, 0, NULL, ctr, 4, NULL),
                    RV_ERR_SHAPE, "rv_reparam_bwd: the padded latent width must be 64, 128 or 256");
  }
  // (the other extent rules still hold at a good width)
  fails += EXPECT(rv_reparam_fwd(f, 0, 1024, 64, 100, 3, NULL, f, 1, ctr, f, buf, f, NULL), RV_ERR_SHAPE, "rv_reparam_fwd: bad extents");
  fails += EXPECT(rv_reparam_fwd(f, 1, 1024, 64, 100, 65, NULL, f, 1, ctr, f, buf, f, NULL), RV_ERR_SHAPE, "rv_reparam_fwd: bad extents");
  fails += EXPECT(rv_reparam_fwd(f, 1, 1000, 64, 100, 3, NULL, f, 1, ctr, f, buf, f, NULL), RV_ERR_SHAPE, "rv_reparam_fwd: bad extents");
  fails += EXPECT(rv_reparam_bwd(f, 1, 1000, 64, 100, 3, 512, f, f, 1e-4f, NULL, NULL, buf, f, NULL, 0, NULL, 0, NULL, ctr, 4, NULL),
                  RV_ERR_SHAPE, "rv_reparam_bwd: bad extents");
  return fails;
}

// The plan's tables on fake base addresses (nothing is dereferenced): every named buffer lies inside the workspace, 256-byte
// aligned and in layout order; the lookups that must give NULL do; every option that edits the descriptor tables, then both
// tables read back, with and without a gradient arena.
static int plan_checks() {
  static const char* names[] = {
      "xb", "W1b", "Whb", "W3b", "W4b", "b1p", "bhp", "b3p", "b4p", "h1", "mulv_slabs", "mulv", "eps", "z", "h3", "dP4", "dP3",
      "dz_slabs", "dmulv", "dP1", "dW1", "dWh", "dWh_us", "dW3", "dW4", "dW1_us", "dW4_us", "db1p", "dbhp", "db3p", "db4p", "xq",
      "W1q", "W4q", "h3q", "dP4q", "dP1q", "fp8_state", "h3_amax", "ddp_flags", "mse_part", "kl_part"};
  int fails = 0;
  char* const base = (char*)0x10000000000;
  for (int with_grad = 0; with_grad < 2; ++with_grad) {
    rv_plan* pl = NULL;
    fails += rv_plan_create(&pl, 4096, 1024, 2048, 64) != 0;
    fails += rv_plan_buffer(pl, "xb", NULL) != NULL;                     // not bound yet
    const long ws_bytes = rv_plan_workspace_bytes(pl);
    rv_plan_buffers b;
    memset(&b, 0, sizeof b);
    b.param = (float*)(base + 0x100000000); b.exp_avg = (float*)(base + 0x200000000);
    b.exp_avg_sq = (float*)(base + 0x300000000); b.grad = with_grad ? (float*)(base + 0x400000000) : NULL;
    b.workspace = base; b.step_counter = (long long*)(base + 0x500000000); b.loss_ring = (float*)(base + 0x500001000);
    b.ring = 4;
    fails += rv_plan_bind(pl, &b) != 0;
    long end = 0;
    for (const char* name : names) {
      long n = -1;
      char* ptr = (char*)rv_plan_buffer(pl, name, &n);
      fails += !(ptr && ptr - base == end && n > 0 && end % 256 == 0);
      end = (ptr - base) + (n + 255) / 256 * 256;
    }
    fails += end != ws_bytes;
    fails += rv_plan_buffer(pl, "no_such_buffer", NULL) != NULL;
    fails += rv_plan_buffer(pl, NULL, NULL) != NULL;
    fails += rv_plan_buffer(NULL, "xb", NULL) != NULL;
    rv_param_desc slab[10], flat[10];
    const int opts[][2] = {{RV_OPT_FP8, 1}, {RV_OPT_FP8, 2}, {RV_OPT_FP8, 0}, {RV_OPT_SLAB_DTYPE, RV_SLAB_F32},
                           {RV_OPT_SLAB_DTYPE, RV_SLAB_F16}, {RV_OPT_LATENT_FUSED, 0}, {RV_OPT_LATENT_FUSED, 1}};
    for (const auto& o : opts) {
      fails += rv_plan_set_option(pl, o[0], o[1]) != 0;
      fails += rv_plan_descs(pl, slab, 0) != 0;
      fails += rv_plan_descs(pl, flat, 1) != 0;
      for (int i = 0; i < 10; ++i) {
        fails += !(flat[i].offset == slab[i].offset && flat[i].shadow_fp8 == slab[i].shadow_fp8);
        if (with_grad) fails += !(flat[i].grad_slabs == b.grad + slab[i].offset && flat[i].grad_splits == 1 && !flat[i].grad_half);
        else fails += !(flat[i].grad_slabs == slab[i].grad_slabs && flat[i].grad_splits == slab[i].grad_splits);
      }
    }
    fails += EXPECT(rv_plan_set_option(pl, RV_OPT_FP8, 3), RV_ERR_UNSUPPORTED, "rv_plan_set_option: RV_OPT_FP8 takes 0, 1 or 2");
    rv_plan_destroy(pl);
  }
  return fails;
}

int main() {
  long Bp, Sp, Hp, Lp; int bm, bn, sp, paired;
  int fails = 0;
  fails += rv_pad_dims(4096, 1024, 2048, 64, &Bp, &Sp, &Hp, &Lp) != 0;
  fails += !(Bp == 4096 && Sp == 1024 && Hp == 2048 && Lp == 64);
  fails += rv_pad_dims(1, 1, 1, 300, &Bp, &Sp, &Hp, &Lp) == 0;          // latent > 256: rejected
  fails += strstr(rv_last_error(), "latent_dim") == NULL;
  for (long m = 64; m <= 8192; m *= 2) for (long n = 64; n <= 4096; n *= 2) for (long k = 64; k <= 8192; k *= 4) {
    fails += rv_gemm_plan(RV_PLAN_GEMM, m, n, k, 16, &bm, &bn, &sp, NULL) != 0;
    fails += !(m % bm == 0 && n % bn == 0 && (k / 64) % sp == 0);
    fails += rv_gemm_plan(RV_PLAN_PAIR, m, n, k, 0, &bm, NULL, &sp, &paired) != 0;
    fails += !(m % bm == 0);
  }
  fails += rv_gemm_plan(RV_PLAN_GEMM, 100, 64, 64, 16, &bm, &bn, &sp, NULL) == 0;            // not a multiple of 64
  rv_param_desc d[20]; memset(d, 0, sizeof d);
  float x[4];
  fails += rv_adam_multi(d, 20, x, x, x, NULL, NULL, 1e-3f, 1.f, (const long long*)x, NULL) == 0;  // > 16 descriptors
  fails += rv_adam_multi(d, 1, x, x, x, NULL, NULL, 1e-3f, 1.f, (const long long*)x, NULL) == 0;   // invalid descriptor
  fails += rv_linear_fwd(NULL, 0, NULL, 0, NULL, 64, 64, 64, 1, NULL, 0, NULL) == 0;
  fails += rv_linear_fp32(x, 1, x, 1, NULL, 0, 1, 1, 0, x, 1, NULL) == 0;
  rv_plan* pl = NULL;
  fails += rv_plan_create(&pl, 4096, 1024, 2048, 64) != 0;
  { int a_ = 0, b_ = 0; fails += rv_plan_riders(pl, &a_, &b_) == 0; }  // needs a bound plan
  fails += rv_plan_set_option(pl, RV_OPT_FP8, 1) == 0;                 // not bound
  rv_comm_desc c; memset(&c, 0, sizeof c);
  c.comm = x; c.world = 2; c.rank = 2;
  fails += rv_plan_attach_comm(pl, &c) == 0;                           // rank out of range
  c.rank = 0;
  fails += rv_plan_attach_comm(pl, &c) == 0;                           // no collective given
  fails += strstr(rv_last_error(), "no collective") == NULL;
  fails += rv_plan_attach_comm(pl, NULL) == 0;
  memset(&c, 0, sizeof c);
  fails += rv_plan_attach_comm(pl, &c) != 0;                           // comm == NULL: detach, always allowed
  fails += rv_gemm_plan(7, 256, 256, 256, 1, &bm, &bn, &sp, &paired) == 0;   // unknown query
  rv_plan_destroy(pl);
  fails += launcher_checks();
  fails += plan_checks();
  printf("host checks: %d failures; last error: %s\n", fails, rv_last_error());
  return fails != 0;
}
