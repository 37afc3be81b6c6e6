/* rawvae_hip.h -- C ABI of librawvae_hip.so: the MI355X (gfx950) training path of
 * the raw-audio VAE.
 *
 * The reference (kelseyicotton/rawaudiovae_kelsey) has no FFI of its own: its hot
 * path sits behind a Python module surface (rawvae/model.py, train.py).  Each entry
 * point below names the reference statement(s) whose arithmetic it replaces; the
 * Python classes in rawaudiovae_kelsey_amd/ (re-exported as rawvae.model) keep the
 * reference's signatures and call these through ctypes.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no torch / HIP types in signatures
 *     (`stream` is a hipStream_t passed as void*; NULL = the default stream).
 *   - every pointer is a DEVICE pointer owned by the caller; the library allocates no
 *     device memory at all -- only the opaque rv_plan / rv_graph host objects and a
 *     plan's internal streams and events.
 *   - one process per GPU, one host thread calling in at a time: the per-kernel
 *     "dynamic LDS attribute set" latches (and the test hook of
 *     rawvae_hip_diag.h) are plain process-wide statics (not per device, not thread-safe).
 *   - every function returns 0 on success or a negative RV_ERR_* code;
 *     rv_last_error() gives the message.  Nothing throws, aborts or synchronises
 *     unless its name ends in _sync; all launches are safe under stream capture.
 *   - "bf16 padded" operands: row-major bfloat16 whose extents are multiples of the
 *     GEMM tile (rows of the batch: 128; feature dims: 128; latent: 64) with zero
 *     padding -- see rv_pad_dims().  fp32 tensors at the reference boundary
 *     (frames, recon, mu, logvar, parameters, gradients) keep their exact shapes.
 *   - leading dimensions (every `ld*` argument of the bf16 GEMM family below) count ELEMENTS of the tensor they
 *     belong to and must be at least that tensor's row width as the entry point states it: a smaller one is
 *     RV_ERR_SHAPE before anything is launched (rows never overlap; rv_linear_fp32 / rv_small_linear_f32 are the
 *     exceptions and say so).  Alignment: a multiple of 8 for a bf16 tensor (operand, mask or output: rows of whole
 *     16-byte pieces) and for fp16 slabs, a multiple of 4 for fp32 slabs; the exact-shape fp32 tensors x and recon of
 *     rv_decode_out_loss_fwd and the source of rv_cast_pad_bf16 take any leading dimension >= their width.  The base
 *     pointer of every bf16 tensor and of every slab is 16-byte aligned.  A kernel touches columns [0, width) of a
 *     row only: the gap [width, ld) is neither read nor written.
 *   - split outputs: an entry point that writes `splits` partial slabs of a [rows, cols] result with leading
 *     dimension ld writes slab s at element offset s * rows * ld (NOT s * rows * cols): element (r, c) of slab s is
 *     at s * rows * ld + r * ld + c, `rows` being the padded row count the entry point names.  The same stride goes
 *     into rv_param_desc.grad_split_stride.
 */
#ifndef RAWVAE_HIP_H
#define RAWVAE_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RV_OK 0
#define RV_ERR_SHAPE (-1)
#define RV_ERR_NULL (-2)
#define RV_ERR_HIP (-3)
#define RV_ERR_UNSUPPORTED (-4)
#define RV_ERR_STATE (-5)

#define RV_ACT_NONE 0
#define RV_ACT_RELU 1

int rv_version(void);
const char* rv_last_error(void);

/* Padded extents used by every bf16 operand: Bp, Sp, Hp multiples of 128, Lp of 64. */
int rv_pad_dims(long B, long S, long H, long L, long* Bp, long* Sp, long* Hp, long* Lp);

/* GEMM tiling decisions, exposed because callers size partial-sum buffers from them (NULL outputs are skipped):
 *   RV_PLAN_GEMM  recommended split-K count *splits (<= splits_in, a power of two) and block tile (*bm x *bn) of a
 *                 padded Mp x Np x Kp GEMM;
 *   RV_PLAN_TILE  the tile the library uses when that GEMM is launched with exactly splits_in splits; per-row-tile
 *                 outputs (column-sum partials, MSE partials) then have Mp / bm row tiles and Np / bn column tiles;
 *   RV_PLAN_PAIR  for rv_linear_dgrad_wgrad(Mp, Np, Kp): *paired (one 256 x 256 launch for both GEMMs), the row tile
 *                 *bm of its column-sum partials and the weight gradient's split count *splits. */
enum { RV_PLAN_GEMM = 0, RV_PLAN_TILE = 1, RV_PLAN_PAIR = 2 };
int rv_gemm_plan(int what, long Mp, long Np, long Kp, int splits_in, int* bm, int* bn, int* splits, int* paired);

/* fp32 [rows, cols] (leading dim ld_src >= cols, any alignment) -> zero-padded bf16 [rows_p, cols_p] (leading dim
 * ld_dst >= cols_p, a multiple of 8; columns [cols_p, ld_dst) are left alone).
 * Replaces the implicit fp32 operand read of F.linear (model.py:20) for frames and
 * is how weight shadows are (re)built after load_state_dict.  If `step_counter` is
 * non-NULL the kernel also increments *step_counter (device int64) once: it is the
 * first kernel of a training step. */
int rv_cast_pad_bf16(const float* src, long rows, long cols, long ld_src, void* dst_bf16,
                     long rows_p, long cols_p, long ld_dst, long long* step_counter, void* stream);

/* y = act(x W^T + b) -> bf16.  nn.Linear + F.relu, model.py:20 (fc1) and :29 (fc3).
 * x [Mp,Kp] bf16, w [Np,Kp] bf16 (nn.Linear [out,in] layout), bias [Np] fp32 or NULL.
 * ldx >= Kp, ldw >= Kp, ldy >= Np, each a multiple of 8. */
int rv_linear_fwd(const void* x_bf16, long ldx, const void* w_bf16, long ldw, const float* bias,
                  long Mp, long Np, long Kp, int act, void* y_bf16, long ldy, void* stream);

/* Same contraction, fp32 output written as `splits` partial slabs of [Mp,Np]
 * (slab s covers K range s*Kp/splits..); bias (may be NULL) is added by slab 0 only.
 * ldx >= Kp, ldw >= Kp (multiples of 8), ldy >= Np (a multiple of 4); consecutive slabs are Mp * ldy elements apart.
 * Used for the fused mu|logvar head GEMM, model.py:21 (fc21, fc22). */
int rv_linear_fwd_f32(const void* x_bf16, long ldx, const void* w_bf16, long ldw,
                      const float* bias, long Mp, long Np, long Kp, int splits, float* y_f32,
                      long ldy, void* stream);

/* Exact-fp32 y = act(x W^T + b) for the inference surface: `model(test_sample)[0]` under
 * torch.no_grad() (train.py:218-232) and the notebooks' encode / decode calls
 * (tutorial.ipynb:461,505-506,922-923).  F.linear + F.relu / F.tanh, model.py:20-21,29-30, in the
 * reference's own precision: f32-input MFMA (a k-ordered fmaf chain), so outputs match the
 * reference to f32 summation order.  Exact shapes (no padding), x [M,K], w [N,K] ([out,in]),
 * bias [N] or NULL, y [M,N]; act: 0 none, 1 relu, 2 tanh.  ldx may be smaller than K: rows of x
 * may overlap (hop-strided frames read straight from a waveform, rv_match_pad). */
int rv_linear_fp32(const float* x, long ldx, const float* w, long ldw, const float* bias, long M,
                   long N, long K, int act, float* y, long ldy, void* stream);

/* recon = tanh(h3 W4^T + b4), model.py:30, fused with the reconstruction half of
 * loss_function (model.py:39) and its derivative:
 *   recon   (optional) exact [B,S] fp32
 *   if x != NULL: mse_partial[block] = sum (recon-x)^2 over the block's valid elements
 *                 dP4 bf16 [Bp,Sp]   = (2/(B*S)) (recon-x)(1-recon^2)   (0 in padding)
 *                 db4_partial [Bp/bm][Sp] column sums of dP4 (optional)
 * with (bm, bn) = rv_gemm_plan(RV_PLAN_TILE, Bp, Sp, Hp, 1, ...): n_mse_partials = (Bp/bm)*(Sp/bn).
 * h3 [Bp,Hp] and w4 [Sp,Hp] bf16: ldh >= Hp, ldw >= Hp, multiples of 8.  x and recon [B,S] fp32: ldx >= S, ld_recon >= S,
 * any alignment; rows [B, Bp) and columns [S, Sp) of them are not touched.  ld_dp4 >= Sp, a multiple of 8. */
int rv_decode_out_loss_fwd(const void* h3_bf16, long ldh, const void* w4_bf16, long ldw,
                           const float* b4, long Bp, long Sp, long Hp, long B, long S,
                           const float* x, long ldx, float* recon, long ld_recon,
                           void* dP4_bf16, long ld_dp4, float* mse_partial, float* db4_partial,
                           void* stream);

/* dX = dY W (autograd of F.linear, train.py:191).  dy [Mp,Kp] bf16, w [Kp,Np] bf16
 * ([out,in] layout, consumed as-is through transposing LDS reads).
 *   mask != NULL : dx_bf16 = (mask > 0) ? dX : 0   (ReLU', threshold_backward) and
 *                  colsum_partial [Mp/bm][Np] (optional) = column sums = bias grads,
 *                  bm from rv_gemm_plan(RV_PLAN_TILE, Mp, Np, Kp, 1, ...)
 *   mask == NULL : dx_f32 written as `splits` fp32 partial slabs [Mp,Np], Mp * lddx32 elements apart.
 * lddy >= Kp, ldw >= Np (multiples of 8); mask and dx_bf16 [Mp,Np]: ldmask >= Np, lddx >= Np (multiples of 8);
 * lddx32 >= Np (a multiple of 4).  The leading dimensions of the form that is not used are not read. */
int rv_linear_dgrad(const void* dy_bf16, long lddy, const void* w_bf16, long ldw, long Mp,
                    long Np, long Kp, const void* mask_bf16, long ldmask, void* dx_bf16,
                    long lddx, float* colsum_partial, float* dx_f32, long lddx32, int splits,
                    void* stream);

/* Split-K slab element type of a weight gradient: fp32, or block-floating-point fp16 -- fp16(partial * 2^e) with
 * one exponent e per wave tile of one slab, taken from that tile's own largest magnitude, so gradients of ANY
 * magnitude keep fp16's 11 significant bits relative to their tile (same element strides as fp32 slabs).  The GEMM
 * writes the factors that undo the scales, 2^-e, to `slab_unscale`: [splits][Mp / 32][Np / 32] fp32, one per
 * 32 x 32 granule of each slab (required with RV_SLAB_F16, ignored with RV_SLAB_F32).  The sum over slabs stays fp32
 * in rv_adam_multi / rv_grad_finalize, which are told by rv_param_desc.grad_half / grad_unscale.  Halves the bytes
 * the GEMM writes and the optimizer reads back. */
enum { RV_SLAB_F32 = 0, RV_SLAB_F16 = 1 };

/* Both halves of a Linear layer's backward in ONE launch when the extents allow 256x256 tiles
 * (neither GEMM alone has enough such tiles to fill 256 CUs; together they do):
 *   dx_bf16 [Mp,Np] = (x > 0) ? dY W : 0     with column-sum partials [Mp/bm][Np] (bias grads)
 *   dw_slabs [splits][Kp][Np] = dY^T x        (split over the batch)
 * dy [Mp(batch), Kp(out)], w [Kp, Np] ([out,in]), x [Mp, Np] = the layer's ReLU output (mask AND
 * wgrad operand).  `splits` and `bm` must come from rv_gemm_plan(RV_PLAN_PAIR, Mp, Np, Kp, ...); when the
 * 256x256 pairing does not apply (e.g. the heads: Kp = 2 Lp) the two GEMMs still go out in one
 * launch if they share a small tile, otherwise as rv_linear_dgrad + rv_linear_wgrad.
 * lddy >= Kp, ldw >= Np, ldx >= Np, lddx >= Np (multiples of 8); lddw >= Np, a multiple of 4 (fp32 slabs) or 8 (fp16 slabs);
 * consecutive dw slabs are Kp * lddw elements apart (fp32 or fp16 elements alike).  The slab_unscale table and the column-sum
 * partials are packed and have no leading dimension. */
int rv_linear_dgrad_wgrad(const void* dy_bf16, long lddy, const void* w_bf16, long ldw, const void* x_bf16, long ldx,
                          long Mp, long Np, long Kp, void* dx_bf16, long lddx, float* colsum_partial, void* dw_slabs,
                          long lddw, int splits, int slab_dtype, float* slab_unscale, void* stream);

/* Backward of a Linear layer whose input had no activation (fc3, whose input is z): dX = dY W as
 * `dgrad_splits` fp32 slabs [Mp, Np] and dW = dY^T X as `wgrad_splits` slabs [Kp, Np], in ONE launch
 * when both GEMMs run on the same small tile (they read the same dY; each alone is mostly launch and
 * store-tail time).  dy [Mp(batch), Kp(out)], w [Kp, Np], x [Mp, Np].  Autograd of F.linear, train.py:191.
 * lddy >= Kp, ldw >= Np, ldx >= Np (multiples of 8); lddx >= Np, lddw >= Np (multiples of 4); dx slabs are Mp * lddx elements
 * apart, dw slabs Kp * lddw. */
int rv_linear_dgrad_wgrad_f32(const void* dy_bf16, long lddy, const void* w_bf16, long ldw,
                              const void* x_bf16, long ldx, long Mp, long Np, long Kp, float* dx_slabs,
                              long lddx, int dgrad_splits, float* dw_slabs, long lddw, int wgrad_splits,
                              void* stream);

/* dW = dY^T X as `splits` partial slabs [Mp(out), Np(in)] (split over the batch) of element type slab_dtype.
 * dy [Kp(batch), Mp] bf16, x [Kp(batch), Np] bf16; both read through transposing LDS
 * reads.  Autograd of F.linear w.r.t. weight, train.py:191.  `tile`: RV_TILE_AUTO (the picker's choice) or a named
 * block tile (extents must be multiples of it; `splits` must divide Kp/64; RV_TILE_256x256 runs the ping-pong main
 * loop when Kp/64/splits is even).
 * lddy >= Mp, ldx >= Np (multiples of 8); lddw >= Np, a multiple of 4 (fp32 slabs) or 8 (fp16 slabs); consecutive slabs are
 * Mp * lddw elements apart (fp32 or fp16 elements alike); slab_unscale is packed, [splits][Mp / 32][Np / 32]. */
enum { RV_TILE_AUTO = -1, RV_TILE_64x64 = 0, RV_TILE_128x128 = 4, RV_TILE_256x128 = 2, RV_TILE_256x256 = 7 };
int rv_linear_wgrad(const void* dy_bf16, long lddy, const void* x_bf16, long ldx, long Mp, long Np, long Kp,
                    int splits, int tile, void* dw_slabs, long lddw, int slab_dtype, float* slab_unscale, void* stream);

/* Reparameterisation forward, model.py:23-26, fused with the KL half of
 * loss_function (model.py:45):
 *   mulv_slabs [splits][Bp][2Lp] fp32 partial head outputs (mu at col l, logvar at Lp+l)
 *   -> mulv [Bp][2Lp] fp32 (summed, zero in padding), z bf16 [Bp][Lp],
 *      kl_partial[block] = sum over valid (b,l) of 1 + logvar - mu^2 - exp(logvar).
 * eps: explicit [B,L] fp32 when eps_in != NULL (parity runs), otherwise generated
 * on-device (Philox4x32-10 + Box-Muller, keyed by seed and *step_counter: the counter layout is stated at rv_randn) and
 * written to eps_out [B,L].  n_kl_partials = Bp*Lp/1024.  Lp is 64, 128 or 256 (rv_pad_dims), else RV_ERR_SHAPE. */
int rv_reparam_fwd(const float* mulv_slabs, int splits, long Bp, long Lp, long B, long L,
                   const float* eps_in, float* eps_out, unsigned long long seed,
                   const long long* step_counter, float* mulv, void* z_bf16, float* kl_partial,
                   void* stream);

/* encode's heads + reparameterize in one call, model.py:21-26 (fc21 | fc22 as ONE [2Lp, Kp] weight, then
 * z = mu + eps * exp(logvar / 2)) with the KL partials of model.py:45: rv_linear_fwd_f32 into `mulv_slabs`
 * (workspace, [splits][Bp][2Lp] fp32) followed by rv_reparam_fwd -- two launches back to back on `stream`.
 * A one-launch form was priced and not built: at 2L = 128 outputs the GEMM only fills the chip as 512 split-K
 * blocks, and combining split-K partials inside a launch (release fence + arrival ticket + acquire, 5-13 us per seam
 * on this chip: MI355X_MICROARCH.md, price list row "splitk-seam") costs more than the ~1.5 us kernel boundary it
 * removes; without split-K every block re-streams the whole head weight through its CU's ~60 GB/s L2->LDS port
 * (12-14 us for any row tile from 16 to 64 against 12.9 us for the two launches).  See DESIGN.md section 3.
 * h [Bp,Kp], wh [2Lp,Kp] bf16: ldh >= Kp, ldw >= Kp, multiples of 8.  mulv_slabs, mulv, z, eps and the KL partials are packed
 * (slabs Bp * 2Lp elements apart). */
int rv_heads_reparam_fwd(const void* h_bf16, long ldh, const void* wh_bf16, long ldw, const float* bias_heads,
                         long Bp, long Lp, long Kp, long B, long L, int splits, float* mulv_slabs,
                         const float* eps_in, float* eps_out, unsigned long long seed, const long long* step_counter,
                         float* mulv, void* z_bf16, float* kl_partial, void* stream);

/* The latent-sized forward in ONE launch for a padded latent width of 64 (L <= 64; BASELINE's C2): heads GEMM
 * (model.py:21) + reparameterisation and KL partials (model.py:23-26,45) + fc3 with bias and ReLU (model.py:29),
 * 16 batch rows per workgroup, all three steps row-local.  Every workgroup streams the whole head weight and W3
 * through its CU (832 KB at C2, the L2 -> LDS port's ~60 GB/s sets the time): the K dimension of the heads GEMM and
 * the columns of fc3 are cut over the 8 waves, each wave running private LDS-DMA rings with counted vmcnt, no
 * workgroup barrier in the streaming loops (csrc/latent.hip).  Replaces rv_heads_reparam_fwd followed by
 * rv_linear_fwd(fc3): same outputs (mulv [Bp][128], z bf16 [Bp][64], kl_partial[Bp / 16], eps_out, h3 bf16
 * [Bp][Hp]); mu / logvar differ from the split-K route by fp32 summation order only; eps draws and the KL partial
 * layout are identical.  RV_ERR_UNSUPPORTED for other latent widths or a padded hidden width that is not a multiple
 * of 512 up to 2048.  18.8 us against 21-22 us for the three launches at C2 (profiles/r03_*): the training plan's
 * default where it applies (rv_plan_set_option, RV_OPT_LATENT_FUSED).
 * w3_bf16 == NULL: heads + reparameterisation only (bias3, h3_bf16 unused; 576 KB per CU instead of 832); fc3 is then
 * the caller's (rv_linear_fwd).
 * Padded latent widths 128 / 256 (the reference's own latent_dim = 256, default.ini:18), batches above 8192 and other
 * hidden widths (multiples of 128): the same call runs its GEMM form -- the heads GEMM on 64 x 128 tiles (256-row tiles at
 * large batches: 256 x 128, from Lp = 128 on 256 x 256 ping-pong) with bias, eps, exp, z and the KL partials in the
 * epilogue, then fc3 as a forward GEMM.  Same outputs and eps draws; kl_partial [Bp Lp / 1024] then holds one non-zero
 * slot per tile and zeros in the others (only the sum is defined).
 * h [Bp,Hp], wh [2Lp,Hp], w3 [Hp,Lp], h3 [Bp,Hp] bf16: ldh >= Hp, ldwh >= Hp, ldw3 >= Lp, ldh3 >= Hp, multiples of 8 (ldw3 and
 * ldh3 are not read when w3_bf16 == NULL).  mulv, z, eps and kl_partial are packed. */
int rv_latent_fwd(const void* h_bf16, long ldh, const void* wh_bf16, long ldwh, const float* bias_heads,
                  const void* w3_bf16, long ldw3, const float* bias3, long Bp, long Hp, long Lp, long B, long L,
                  const float* eps_in, float* eps_out, unsigned long long seed, const long long* step_counter,
                  float* mulv, void* z_bf16, float* kl_partial, void* h3_bf16, long ldh3, void* stream);

/* The backward mirror of rv_latent_fwd's first two steps in ONE launch (same shape limits): dz = dP3 W3 (autograd of
 * fc3's input, model.py:29) for 16 batch rows per workgroup over the full contraction, then rv_reparam_bwd's
 * arithmetic on that block's dz while it is still in LDS -- no dz slabs, no second launch.  Arguments as
 * rv_reparam_bwd with dP3 [Bp, Hp] bf16 and W3 [Hp, Lp] bf16 ([out, in]) in place of the dz slabs; dz differs from the
 * split-K route by fp32 summation order only.  With z_bf16 != NULL the launch also computes fc3's weight gradient
 * dW3 [Hp, Lp] = dP3^T z as `dw3_splits` fp32 slabs (rv_linear_wgrad's result, bit for bit) on extra workgroups that
 * share the CUs with the dz workgroups (80 KiB of LDS each): the second read of dP3 fills the bubbles of the first.
 * GEMM form (same shapes as rv_latent_fwd's): dz tiles of 64 rows (256 at large batches; ONE 256 x 256 ping-pong tile per
 * 256 rows at Lp = 256) with the reparameterisation backward in the epilogue, dW3 on the launch's first workgroups.
 * dbh_partial [Bp / 16][2 Lp] keeps its layout: the row-local kernel fills every row, the GEMM forms the first row of each
 * dz tile's rows and ZEROS in the rest (a reader may sum every row, or every (tile rows / 16)-th).
 * dP3 [Bp,Hp], W3 [Hp,Lp], z [Bp,Lp] bf16: lddp >= Hp, ldw3 >= Lp, ldz >= Lp, multiples of 8; lddw3 >= Lp, a multiple of 4;
 * consecutive dW3 slabs are Hp * lddw3 elements apart (ldz and lddw3 are not read when z_bf16 == NULL).  mulv, eps, dmulv,
 * dbh_partial and loss_out are packed. */
int rv_latent_bwd(const void* dp3_bf16, long lddp, const void* w3_bf16, long ldw3, long Bp, long Hp, long Lp, long B,
                  long L, long S, const float* mulv, const float* eps, float kl_beta, const float* dmu_ext,
                  const float* dlv_ext, void* dmulv_bf16, float* dbh_partial, const float* mse_partial, int n_mse,
                  const float* kl_partial, int n_kl, float* loss_out, const long long* step_counter, int ring,
                  const void* z_bf16, long ldz, float* dw3_slabs, long lddw3, int dw3_splits, void* stream);

/* The heads' backward (autograd of fc21 | fc22, model.py:21, with fc1's ReLU) for a padded latent width of 64 as ONE
 * streaming launch that reads h1 once: dp1 [Bp, Hp] bf16 = (h1 > 0) ? dmulv Wh : 0, its column sums per 512-row group
 * (db1_partial [Bp / 512][Hp], fc1's bias gradient) and dWh = dmulv^T h1 as one fp32 slab per 512-row group
 * (dwh_slabs [Bp / 512][128][lddw]: rv_linear_dgrad_wgrad's outputs with Bp / 512 splits).  dmulv [Bp, 128] bf16 (mu
 * columns 0..63, logvar 64..127: rv_reparam_bwd's output), wh [128, Hp] bf16 (fc21 | fc22, [out, in]), h1 [Bp, Hp]
 * bf16.  A workgroup keeps its 64-column slice of Wh in LDS and walks 512 rows in tiles of 64; the same staged h1
 * tile is the ReLU mask of the first product and the operand of the second.  RV_ERR_UNSUPPORTED unless Lp == 64,
 * Bp % 512 == 0 and Hp % 64 == 0.
 * ldw >= Hp, ldh >= Hp, ldp >= Hp (multiples of 8); lddw >= Hp, a multiple of 4; consecutive dWh slabs are 128 * lddw
 * elements apart.  dmulv [Bp, 128] and db1_partial are packed. */
int rv_heads_bwd(const void* dmulv_bf16, const void* wh_bf16, long ldw, const void* h1_bf16, long ldh, long Bp, long Hp,
                 long Lp, void* dp1_bf16, long ldp, float* db1_partial, float* dwh_slabs, long lddw, void* stream);

/* Backward of reparameterize + KL:
 *   dmu = dz + kl_beta mu/(B L);  dlv = dz eps std/2 + kl_beta (exp(logvar)-1)/(2 B L)
 * dz_slabs [splits][Bp][Lp] fp32 -> dmulv bf16 [Bp][2Lp] and per-block column sums
 * dbh_partial [Bp/16][2Lp] (bias grads of fc21|fc22).  One block also finishes the
 * loss: loss_out[0] = sum(mse_partial)/(B S) + kl_beta*(-0.5*sum(kl_partial)/(B L)),
 * loss_out[1] = mse term, loss_out[2] = KL term (pass NULL partials to skip).  When
 * step_counter != NULL and ring > 0, loss_out is a ring of [ring][4] floats and the slot written is (*step_counter - 1)
 * mod ring in [0, ring) (ring - 1 for a counter of 0), so graph replays log every step.  Lp as for rv_reparam_fwd. */
/* Gradients that arrive from outside are added in (exact [B, L] fp32, either may be NULL):
 * dmu += dmu_ext, dlv += dlv_ext -- what autograd hands the backward of reparameterize when mu / logvar also feed
 * a loss term directly (the KL half of loss_function, model.py:45).  Pass kl_beta = 0 when the KL gradient is
 * already inside dmu_ext / dlv_ext. */
int rv_reparam_bwd(const float* dz_slabs, int splits, long Bp, long Lp, long B, long L, long S,
                       const float* mulv, const float* eps, float kl_beta, const float* dmu_ext,
                       const float* dlv_ext, void* dmulv_bf16, float* dbh_partial, const float* mse_partial,
                       int n_mse, const float* kl_partial, int n_kl, float* loss_out,
                       const long long* step_counter, int ring, void* stream);

/* loss_function(recon_x, x, mu, logvar, kl_beta, segment_length), model.py:38-47, as ONE
 * wave-reduced kernel over exact-shape fp32 tensors; also emits the gradients autograd
 * would produce for (recon, mu, logvar) so loss.backward() needs no second pass.
 * workspace: rv_loss_fused_workspace_bytes() bytes, zero-initialised once by the caller.
 * loss_out[0..2] = total, mse, kld.  Any of the gradient pointers may be NULL. */
long rv_loss_fused_workspace_bytes(void);
int rv_loss_fused(const float* recon, const float* x, const float* mu, const float* logvar,
                  long B, long S, long L, float kl_beta, float* loss_out, float* d_recon,
                  float* d_mu, float* d_logvar, void* workspace, void* stream);

/* z = mu + eps*exp(logvar/2), exact-shape fp32 (VAE.reparameterize called on its own,
 * e.g. tutorial.ipynb:505).  eps_in NULL -> generated from (seed, offset). */
int rv_reparameterize(const float* mu, const float* logvar, long n, const float* eps_in,
                      float* eps_out, unsigned long long seed, unsigned long long offset,
                      float* z, void* stream);

/* Backward of reparameterize for callers that use it on its own: dmu = dz,
 * dlv = dz*eps*exp(logvar/2)/2 (either output may be NULL). */
int rv_reparameterize_bwd(const float* dz, const float* eps, const float* logvar, long n,
                          float* dmu, float* dlv, void* stream);

/* Backward of F.tanh (model.py:30) for VAE.decode used without the fused loss:
 * dP4 = d_recon*(1-recon^2), exact fp32 [B,S] inputs -> zero-padded bf16 [Bp,Sp]. */
int rv_tanh_bwd_pack(const float* d_recon, const float* recon, long B, long S, void* dP4_bf16,
                     long Bp, long Sp, void* stream);

/* fp32 elementwise steps of the strict-fp32 training mode (rawaudiovae_kelsey_amd/strict.py; autograd of
 * model.py:20,29,30): op 0: out = a*(1-b*b) (tanh backward), 1: out = b>0 ? a : 0 (ReLU backward), 2: out = a+b. */
int rv_ew_f32(int op, const float* a, const float* b, long n, float* out, void* stream);

/* Partial column sums (bias gradients): out[rb][c] = sum of rows [256 rb, 256 rb+256) of
 * column c; src is fp32 or bf16 [rows, cols] with leading dim ld.  ceil(rows/256) slabs,
 * summed by rv_grad_finalize / rv_adam_multi. */
int rv_colsum_partial(const void* src, int is_bf16, long rows, long cols, long ld, float* out,
                      long ld_out, void* stream);

/* out[i] = a[i] * scalar[0] (device scalar): applies the upstream gradient of the 0-dim
 * loss tensor to the gradients rv_loss_fused saved. */
int rv_scale_by(const float* a, const float* scalar, long n, float* out, void* stream);
/* The same for up to three tensors in one launch (out_k[i] = a_k[i] * scalar[0]; n_k = 0 skips tensor k): the three
 * gradients loss_function's backward hands on -- the autograd path is bound by host time per launch. */
int rv_scale_by3(const float* a0, float* out0, long n0, const float* a1, float* out1, long n1, const float* a2,
                 float* out2, long n2, const float* scalar, void* stream);

/* Hop-strided framing on the device (AudioDataset, rawvae/dataset.py:99-121): the padded
 * waveform stays in HBM and out[i, :] = audio[f*hop : f*hop + S] with f = frame_index[i]
 * (int64, e.g. one slice of the epoch's shuffle) or first_frame + i when frame_index is NULL
 * (TestDataset, dataset.py:147-157, is hop == S).  Samples past n_samples read as 0. */
int rv_gather_frames(const float* audio, long n_samples, const long long* frame_index,
                     long first_frame, long n_frames, long S, long hop, float* out, void* stream);

/* Audio ingest on the device: the file loading of IterableAudioDataset (rawvae/dataset.py:47-58,
 * `torchaudio.load` + channel 0 + `torchaudio.functional.resample`), for the streaming loader's
 * device ingest (data.StreamingFrames(ingest="device")).
 *
 * rv_pcm_to_f32: a WAV `data` payload (nbytes raw bytes on the device, 16-byte aligned; interleaved
 * `channels` channels of `bytes_per_sample` bytes) -> channel 0 as fp32, out[0 : n) with
 * n = nbytes / (channels * bytes_per_sample), zeros up to n_out, which must be n rounded up to a
 * multiple of `hop` (hop = 1: no padding).  RV_WAV_PCM: 1-byte unsigned ((x - 128) / 128), 2-, 3-
 * (scipy's left-justified int32) and 4-byte signed (x / 2^(bits - 1)); RV_WAV_FLOAT: 4- and 8-byte
 * IEEE (8-byte rounded to nearest).  Bit-identical to data._to_float32(scipy's read)[:, 0]. */
#define RV_WAV_PCM 1
#define RV_WAV_FLOAT 3
int rv_pcm_to_f32(const void* src, long nbytes, int format, int channels, int bytes_per_sample, long hop, float* out,
                  long n_out, void* stream);

/* rv_resample_sinc_hann: `torchaudio.functional.resample(x, sr_in, sr_out)` (dataset.py:50-51; defaults
 * sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) in its polyphase form.  orig / new_ = the rates
 * over their gcd (orig != new_: at equal rates the caller keeps its input), bank = [new_][2 * width + orig]
 * fp32 filters as data._sinc_hann_bank builds them; out[j * new_ + i] = filter i at offset j * orig of the
 * input padded by `width` zeros in front and zeros behind.  The ceil(new_ * n / orig) kept outputs are
 * written to out[0 : ...), zeros up to n_out (>= that count).  fp32 operands and accumulation. */
int rv_resample_sinc_hann(const float* src, long n, const float* bank, long orig, long new_, long width, float* out,
                          long n_out, void* stream);

/* Latent interpolation and resynthesis of whole waveforms (the reference's tutorial.ipynb: stepwise mix
 * 456-530, meso-scale curve 834-925, the same at hop_length 128 "with extensions" 1200-1279), between the exact-fp32
 * encoder and decoder GEMMs (rv_linear_fp32).
 *
 * rv_match_pad: dst[i] = src[i % n_src] for i < n_valid, 0 for n_valid <= i < n_out.  n_valid > n_src repeats
 * the shorter source (the notebook's doubling-then-crop, tutorial.ipynb:429-437), n_valid <= n_src crops it
 * (423-427); n_out is the framing's padded length (AudioDataset: a multiple of hop, dataset.py:99-104;
 * TestDataset: a multiple of S, dataset.py:141-146).  fc1 reads the frames from dst through rv_linear_fp32
 * with ldx = hop: frame f is dst[f * hop, f * hop + S). */
int rv_match_pad(const float* src, long n_src, long n_valid, float* dst, long n_out, void* stream);

/* rv_latent_mix: output rows [row0, row0 + rows) of z = mu + eps * exp(logvar / 2) with mu = mu_a (1 - a) + mu_b a
 * and logvar likewise (tutorial.ipynb:501-505, 916-923); mu_a .. lv_b are
 * [N, L] fp32; z, eps_in / eps_out, mu_out, lv_out are [rows, L] fp32 (this chunk), alpha_out [rows] fp64 (the a
 * of each row).  eps_in NULL: eps = the Philox draw of rv_reparameterize at flat index (row0 + i) * L + l.
 *   RV_ALPHA_LIST : alpha = n_alpha fp64 scalars, n_alpha * N output rows in alpha-major order (row = k N + n).
 *                   fp32 arithmetic: (1 - a) formed in fp64 and rounded, a rounded; each product and sum rounded
 *                   (no contraction); z by rv_reparameterize's expression (bit-equal on the mixed mu / logvar).
 *   RV_ALPHA_F32  : alpha = [N] fp32 per frame; (1 - a) in fp32, otherwise as RV_ALPHA_LIST.
 *   RV_ALPHA_F64  : alpha = [N] fp64 per frame; mix and reparameterisation in fp64 (torch's promotion), z, mu_out
 *                   and lv_out rounded once to fp32.
 *   RV_ALPHA_CURVE: alpha = [n_alpha] fp64 curve stretched to N frames as scipy.interpolate.interp1d(arange(C),
 *                   curve) evaluated at numpy.linspace(0, C - 1, N) (tutorial.ipynb:907-908; scipy evaluates a
 *                   1-D linear interp1d through numpy.interp, whose rule is restated), then RV_ALPHA_F64. */
#define RV_ALPHA_LIST 0
#define RV_ALPHA_F32 1
#define RV_ALPHA_F64 2
#define RV_ALPHA_CURVE 3
int rv_latent_mix(const float* mu_a, const float* lv_a, const float* mu_b, const float* lv_b, long N, long L,
                  int alpha_mode, const void* alpha, long n_alpha, long row0, long rows, const float* eps_in,
                  float* eps_out, unsigned long long seed, unsigned long long offset, float* z, float* mu_out,
                  float* lv_out, double* alpha_out, void* stream);

/* Self-organising map of latent vectors (the SOM whose clusters.json / data-concatenated.json pick the sources of
 * tutorial.ipynb:725-805 and 1078-1146; rawaudiovae_kelsey_amd/som.py).
 *
 * rv_segment_mean: out[f] = mean(x[offsets[f] : offsets[f+1]]) for f < F; x [R, L] fp32, out [F, L] fp32.  offsets is
 * [F+1] int64 in device memory, offsets_host the same values in host memory: they are checked before the launch
 * (0 <= offsets[0], offsets[F] <= R) and an empty segment is RV_ERR_SHAPE.  Each mean is an fp64 sum in ascending row
 * order divided by the count and rounded once. */
int rv_segment_mean(const float* x, long R, long L, const long long* offsets, const long long* offsets_host, long F,
                    float* out, void* stream);

/* rv_som_bmu: for each row n of x [N, L] fp32 the best and second-best node of w [M, L] fp32 under the squared
 * distance sum_l (x[n,l] - w[m,l])^2: best / second [N] int32, d_best / d_second [N] fp32.  Any N >= 1, M >= 2,
 * L >= 1.  Ties go to the lower node index; a row whose distances are all NaN gets index -1.  Direct form in fp32:
 * each term one fma, summed in ascending l within tiles of 32, the tile sums added in order (relative error at most
 * about (34 + L / 32) * 2^-24 of the distance). */
int rv_som_bmu(const float* x, long N, const float* w, long M, long L, int* best, int* second, float* d_best,
               float* d_second, void* stream);

/* rv_som_node_sums: for bmu [N] int32 (indices into M nodes) sums[m] = sum of the rows x[n] with bmu[n] == m, [M, L]
 * fp64 in ascending n, and counts[m] = their number [M] int64.  No atomics: bit-identical from run to run. */
int rv_som_node_sums(const float* x, long N, long L, const int* bmu, long M, double* sums, long long* counts,
                     void* stream);

/* rv_som_update: the batch-SOM step on a rows x cols grid (node m at (m / cols, m % cols)):
 * w_new[m] = sum_b h(m,b) sums[b] / sum_b h(m,b) counts[b], h = exp(-((dr)^2 + (dc)^2) / (2 sigma^2)), in fp64
 * ascending b, rounded once to fp32; w_new[m] = w_old[m] where the denominator is 0.  sums [M, L] fp64, counts [M]
 * int64, w_old / w_new [M, L] fp32 (distinct buffers), sigma > 0. */
int rv_som_update(const double* sums, const long long* counts, const float* w_old, long rows, long cols, long L,
                  double sigma, float* w_new, void* stream);

/* ---- Latent audio mosaicing (csrc/mosaic*.hip, rawaudiovae_kelsey_amd/mosaic.py) ----
 * rv_mosaic(op, d, stream): one entry point for the operations below, each reading the fields of *d its op names.
 *
 * RV_MOSAIC_KNN (rv_knn_topk): for each query row of q [T, L] fp32 the k nearest rows of c [N, L] fp32 under the
 * squared distance: idx [T, k] int32 and dist [T, k] fp32 in ascending (distance, index) order.  1 <= k <= 16, k <= N.
 * The arithmetic is rv_som_bmu's direct form (each term one fma in ascending l within tiles of 32, the tile sums added
 * in order), so identical rows give exactly 0 and for k <= 2 the result is rv_som_bmu's best / second bit for bit.
 * Ties go to the lower corpus index, NaN never wins, and a row with fewer than k candidates gets -1 / +inf in the
 * remaining slots.  The corpus is split across workgroups (`splits` of them; 0 = the library's choice, which fills the
 * chip for any T) and a second launch merges the per-split partials; the result does not depend on the split count.
 * ws / ws_bytes: the workspace of the partials (device memory; unused with one split).
 * RV_MOSAIC_KNN_WORKSPACE (rv_knn_workspace_bytes): stores the bytes RV_MOSAIC_KNN needs for (T, N, L, k, splits) in
 * d->ws_bytes and launches nothing.
 *
 * RV_MOSAIC_GATHER_MEAN (rv_gather_mean): out[t, :width] = (1/k) sum_j src[start(idx[t, j]) : + width] for t < T with
 * row stride ldo; the sum in fp32 in ascending j from +0, then multiplied by 1/k once.  start(i) = row_start[i] (int64)
 * when row_start is not NULL, else i * stride.  Indices outside [0, n_rows) (-1: no neighbour) and rows that would
 * leave src [src_len] add nothing.
 *
 * RV_MOSAIC_OLA (rv_ola): offline weighted overlap-add of F frames [F, S] at `hop` into out [n_out]:
 * out[t] = sum_f w[t - f hop] D_f[t - f hop] / sum_f w[t - f hop] over the frames f that cover t, both sums in
 * ascending f from +0 in fp32 (each product rounded before its add), 0 where the normaliser is 0.  window [S] fp32, or
 * NULL for rectangular.
 *
 * Unit selection over the KNN candidates (Viterbi; DESIGN.md section 7.5 "Continuity"): choose one candidate per row
 * so that J(p) = sum_t dist[t, p_t] + lambda * sum_{t>=1} trans[t, p_{t-1}, p_t] is least.  idx [T, k] / dist [T, k]
 * are always the whole tables as RV_MOSAIC_KNN writes them, 1 <= k <= 16; the rows of one call are [row0, row0 + rows).
 *
 * RV_MOSAIC_TRANSITION: trans [rows, k, k] fp32, trans[t - row0, i, j] = D(c[next_of[idx[t-1, i]]], c[idx[t, j]]) with
 * D the search's distance (same arithmetic, so a candidate that is the successor of the previous one costs exactly 0);
 * +inf when either candidate is -1 (or outside [0, N)) or the value is NaN; row t = 0 is all 0.  c [N, L] fp32 are the
 * corpus latents, next_of [N] int32 the successor table (0 <= next_of[i] < N; anything else counts as missing).
 *
 * RV_MOSAIC_PATH_FORWARD: the forward pass over the rows of `trans` [rows, k, k], in fp32, one row after the other:
 * m = min_i score[i]; s[i] = score[i] - m when m is finite; new[j] = dist[t, j] + min_i (s[i] + fl(lambda * trans[i, j]))
 * over the pairs whose s[i] and trans are finite (product rounded before the add, strict < in ascending i: ties go to
 * the lower i), back[t, j] = that i.  Row t = 0, and a row where no new[j] is finite, starts a new sequence:
 * new = dist[t] (+inf for -1 / NaN), back = none.  end[t] = the lowest-j argmin of the row's scores, none if no score
 * is finite.  back, end, the transition cost met at (t, j) and the scores of the last row live in ws; a call with
 * row0 = 0 resets the scores, and the caller feeds the chunks in ascending order without gaps (the library keeps no
 * host state and never reads the device).  0 <= lambda < +inf.
 *
 * RV_MOSAIC_PATH_BACKTRACK: after the forward pass over all T rows: slot [T] int32 (from end[T-1] backwards through
 * back; end[t-1] where row t started a sequence or has no candidate; -1 for a row without candidates),
 * choice [T] int32 = idx[t, slot[t]] (-1 likewise) and cost [2] fp64 = sum_t dist[t, slot[t]] and the sum of the
 * transition costs met along the path (without lambda), both added in ascending t from +0.
 *
 * RV_MOSAIC_PATH_WORKSPACE: stores the bytes of ws the two PATH ops need for (T, k) in d->ws_bytes; launches nothing.
 *
 * RV_MOSAIC_KNN_SMALL: RV_MOSAIC_KNN's contract and results, bit for bit, by a kernel built for few query rows
 * (1 <= T <= 64; more is RV_ERR_SHAPE): the corpus is read once per 16 query rows, one thread per corpus row
 * (DESIGN.md section 7.6).  RV_MOSAIC_KNN_SMALL_WORKSPACE: its ws_bytes for (T, N, L, k, splits); launches nothing.
 *
 * Live mosaicing: one block of samples per stream in, one block built from the nearest corpus frames out.
 * RV_MOSAIC_LIVE enqueues, without a sync or a read of the device: rv_stream_process's fc1 and heads launches on
 * *live (the query rows are mu * scale + offset; temperature, eps_in and seed are not read), the search of the
 * n_streams * F query rows in c [N, L] (k, splits; KNN_SMALL's kernel up to its 64 rows, KNN's beyond: the same bits)
 * into idx / dist [n_streams * F, k], the selection, the synthesis and rv_stream_process's overlap-add on live->y.
 *   weight == NULL: every frame is the mean of its k candidates (GATHER_MEAN's arithmetic); choice is not written.
 *   weight [n_streams] (device; a value that is not finite and >= 0 counts as 0): greedy unit selection, per stream and
 *     frame in order.  prev = the stream's last chosen corpus frame (-1 after a reset, kept in ws).  prev < 0, or
 *     next_of[prev] outside [0, N): the lowest j with idx[t, j] in [0, N).  Otherwise the argmin over those j of
 *     dist[t, j] + fl(w * D(c[next_of[prev]], c[idx[t, j]])), D the search's distance, the product rounded before the
 *     add, strict < in ascending j, a NaN cost skipped.  choice[t] = that idx[t, j] = the new prev; -1 when no j is
 *     left.  The frame is the chosen corpus frame alone.  This is the lag-0 rule, not PATH_FORWARD's Viterbi search
 *     (`lag` below buys look-ahead); with k = 1 both choose the same frames.
 *   mode RV_LIVE_GRAINS: frames from the corpus audio src [src_len] at row_start [N]; RV_LIVE_DECODE: the mean (or the
 *     chosen row) of c through fc3 and fc4.
 *   lag = D, the lag in frames, 0 <= D <= 64 (read by LIVE, LIVE_DRAIN, LIVE_WORKSPACE and LIVE_RESET; D > 0 needs
 *     weight): fixed-lag Viterbi selection.  D = 0 is the greedy rule above: the same launches, workspace and bits.
 *     Per stream the workspace keeps prev and the PENDING rows: the frames searched but not yet committed, oldest
 *     first, at most D + 1, each with its idx[k], dist[k] and the unweighted transitions [k, k] from the row before it.
 *     Window solve: commits the oldest pending row a, given the pending rows a..b.  Row a's scores are the greedy
 *     rule's expression: prev < 0, or next_of[prev] outside [0, N): score[j] = dist[a, j]; otherwise score[j] =
 *     dist[a, j] + fl(w * D(c[next_of[prev]], c[idx[a, j]])); +inf where idx[a, j] is outside [0, N) or the value is NaN.
 *     Rows a+1..b follow PATH_FORWARD's row rule with lambda = w over TRANSITION's trans (a row where no new[j] is
 *     finite starts a new sequence), end = the lowest-j argmin of row b's scores, and the walk back to row a is
 *     PATH_BACKTRACK's.  The committed frame = idx[a, slot], -1 when row a has no slot; it becomes prev and row a
 *     leaves.  w = weight[stream] as read by the call, for every row of the window.
 *     Per new frame: it joins the pending rows; with D + 1 pending one window solve commits a frame, otherwise
 *     (the first D frames after a reset) nothing is committed.  choice[t] = the frame committed at new frame t, which
 *     is frame t - D's, or -1; the block is synthesised from choice, so the audio is D * hop samples later than at
 *     D = 0, and a -1 adds what a frame without candidates adds.  idx / dist are the new frames', as at D = 0.
 * RV_MOSAIC_LIVE_DRAIN (lag = D > 0): one block that plays out pending rows: no encoder, no search, no new row; per
 *   stream up to F window solves on the shrinking window (choice as above, -1 once nothing is pending), then the
 *   synthesis and rv_stream_process's overlap-add, history roll and frame count as for a block of input: live->x must
 *   be a block of zeros.  prev is kept and RV_MOSAIC_LIVE may follow.
 * RV_MOSAIC_LIVE_WORKSPACE: the bytes of ws (device; RV_MOSAIC_LIVE_RESET before the first block) for live's extents
 * and (N, L, k, splits, lag) in d->ws_bytes; launches nothing.  RV_MOSAIC_LIVE_RESET: rv_stream_reset(live, which),
 * prev = -1 and no pending rows for stream `which` (-1: every stream).
 *
 * Live grain fitting (mode RV_LIVE_GRAINS only): fit_radius = R > 0 or gain_max > 0, read by LIVE, LIVE_DRAIN,
 * LIVE_WORKSPACE and LIVE_RESET as they read `lag`; both 0 = no fit: the launches, workspace bytes and bits above.
 *   Every corpus frame a block is about to play is first fitted, by THE RULE of "Grain fitting" below (the c / e
 *   chains, the score, the tie order, the gain and the room limits unchanged), to the TARGET FRAME IT STANDS FOR, and
 *   the fitted grains are gathered by RV_GRAIN_GATHER's arithmetic in place of GATHER_MEAN's.
 *   Target frame n of a stream (n counted from the stream's last reset, as the stream's frame counter counts) is
 *   samples [n hop, n hop + S) of the stream's input since the reset prefixed by P = S - hop zeros: the frame the
 *   encoder saw.  A LIVE_DRAIN block counts as input (zeros).
 *   weight == NULL: each of the k candidates of new frame n is fitted to target frame n on its own and the k fitted
 *     grains are averaged; the fit's rows are idx [M, k], M = n_streams * F, and its outputs [M, k].
 *   weight != NULL: the one chosen or committed frame is fitted; the rows are choice [M, 1] and the outputs [M, 1].
 *     With lag = D > 0 the frame committed at new frame n is fitted to the target frame that was new when its
 *     candidates arrived: n - D while blocks follow one another, older for a row that waited through a LIVE_DRAIN
 *     (at most 2 D frames old).  A choice of -1 (the first D frames after a reset, a dry drain, a frame without
 *     candidates) gets shift 0, gain 0 and score 0 and adds nothing: the contract for a missing candidate.
 *   Fields: shift [M, kf] int32, gain [M, kf] fp32 and score [M, kf] fp64, the fit's outputs for the block's
 *     frames (kf = k without weight, 1 with); next_of = ONE table [3 N] int32: the successor table [N] (unread
 *     without weight) followed by room [N, 2]; src, src_len, row_start as for RV_LIVE_GRAINS, n_rows = N.
 *   State, in ws after the parts above: per stream a TARGET RING of C = P + 2 D hop + block floats, input sample a
 *     (counted from the reset) at ring[a mod C], zeros before the reset.  One small launch writes the block at the
 *     stream's frame count before the fit reads the ring, which then holds the block and the P + 2 D hop samples
 *     before it, for any block length and any number of wraps; with D > 0 also the arrival frame of every pending row
 *     [n_streams, D + 1] int64 and the target frame of every committed row [M] int64.  LIVE_RESET zeroes the rings of
 *     the streams it resets.  LIVE / LIVE_DRAIN launch, between the selection and the overlap-add: the ring update,
 *     the fit, the gather; no sync, no read of the device, capturable as before.
 *   Errors before any launch, naming the field: fit_radius outside [0, 1024]; gain_max not finite or negative; a
 *     fit in mode RV_LIVE_DECODE; next_of, shift, gain or score null; ws_bytes too small.
 *
 * Grain fitting (csrc/grain.hip; DESIGN.md section 7.5 "Grain fitting"): after the selection, fit each candidate grain
 * to its target frame by a shift of at most R samples and a gain.  THE RULE.  For target frame t, x[n] =
 * frames[t hop + n], n < S.  For candidate j, i = idx[t, j] in [0, n_rows).  room [n_rows, 2] int32 (host-built)
 * says how far frame i's start may move back (room[i, 0]) and forward (room[i, 1]) while the grain stays
 * inside its own file's padded waveform (a negative entry counts as 0), so a shifted grain never reads a neighbouring
 * file of src.  Every shift delta with max(-R, -room[i, 0]) <= delta <= min(R, room[i, 1]) is considered (the range is
 * cut further where a grain would leave src [src_len]; delta = 0 is always permitted):
 *   g[n] = src[row_start[i] + delta + n];  c(delta) = sum_n x[n] g[n];  e(delta) = sum_n g[n]^2, both in fp32, every
 *   term one fma, c = fmaf(x[n], g[n], c) and e = fmaf(g[n], g[n], e), one plain chain each in ascending n from +0.
 *   The order depends on nothing else (not T, k, R, the candidate's position or the launch): equal data, equal bits.
 *   score(delta) = (double)c * (double)c / (double)e when c > 0, e > 0 and both are finite, otherwise 0 (a NaN never
 *   wins).  The choice is the delta of greatest score; ties go to the smaller |delta|, then to the negative delta; when
 *   every score is 0 that is delta = 0.
 *   gain: 1 when gain_max == 0 ("shift only"); otherwise min(fl32(c / e), gain_max) at the chosen delta when its score
 *   is > 0, else 0.
 *   A candidate outside [0, n_rows), or whose unshifted grain is not inside src, gets shift 0, gain 0 and score 0.
 * RV_GRAIN_FIT: T, k, idx [T, k]; frames = the target's padded waveform [n_out] with (T - 1) hop + S <= n_out; hop, S;
 *   src, src_len, row_start [n_rows], n_rows; room; fit_radius = R, 0 <= R <= 1024; gain_max, finite and
 *   >= 0.  Outputs: shift [T, k] int32, gain [T, k] fp32, score [T, k] fp64.  Any
 *   S >= 1.  One launch; no sync and no read of the device (it may run under capture).
 * RV_GRAIN_GATHER: RV_MOSAIC_GATHER_MEAN's fields and contract with shift [T, k] int32 and gain [T, k] fp32:
 *   out[t, n] = (1/k) sum_j fl(gain[t, j] * src[start(idx[t, j]) + shift[t, j] + n]), each product rounded
 *   before its add, the sum in ascending j from +0, 1/k applied once; a candidate outside [0, n_rows) or a shifted
 *   grain that would leave src adds nothing.  With shift 0 and gain 1 it is RV_MOSAIC_GATHER_MEAN bit for bit.
 * Both return an RV_ERR_* whose message names the field before anything is launched: fit_radius, T, k, a null table,
 * frames that overrun n_out, gain_max.
 *
 * Evaluation (csrc/eval.hip, rawaudiovae_kelsey_amd/evaluate.py): how close a test signal y is
 * to a reference signal x, frame by frame, and how the KL term spreads over the latent dimensions.
 * RV_EVAL_FRAMES scores T frame pairs.  Fields:
 *   T            the frame pairs, 1 <= T < 2^31;  S, hop: frame length and hop (S >= 1, hop >= 1)
 *   frames, n_out  x, a padded waveform [n_out]: frame t = frames[t hop, t hop + S), (T - 1) hop + S <= n_out
 *   src, stride, src_len  y: row t = src[t stride, t stride + S), (T - 1) stride + S <= src_len, stride >= 1
 *                (stride >= S: decoded frames [T, S]; stride = hop: a second waveform whose rows overlap)
 *   mu, logvar, L  [T, L] fp32; both NULL: no KL column (written as 0); exactly one NULL is an error
 *   window       [S] fp32, or NULL: the spectral columns 3..5 are not computed (written as 0)
 *   twiddles     the twiddle table [S] fp32, required with a window: S / 2 complex pairs, twiddles[2 j] = cos(2 pi j / S),
 *                twiddles[2 j + 1] = -sin(2 pi j / S) for j < S / 2, computed by the caller in float64 and rounded once
 *   dynamic_range  R in dB, 0 < R <= 120
 *   out, ldo     [T, ldo] fp32, ldo >= 6; only columns 0..5 of rows 0..T-1 are written:
 *     0  sse = sum_n (y[n] - x[n])^2   the differences in fp32, their squares and the sum in fp64, rounded once
 *     1  energy = sum_n x[n]^2         likewise
 *     2  kl = sum_j -0.5 (1 + lv - mu^2 - exp(lv))   every term and the sum in fp64, rounded once
 *     3  lsd (dB), 4  spec_err = sum_k (sqrt Pa[k] - sqrt Pb[k])^2, 5  spec_ref = sum_k Pa[k]
 *   The spectral columns need S a power of two, 32 <= S <= 4096 (a window with another S is RV_ERR_SHAPE).
 *   a[n] = fl32(window[n] x[n]), b[n] = fl32(window[n] y[n]); A, B their S-point DFTs at the K = S / 2 + 1 bins
 *   k = 0 .. S / 2; Pa = |A|^2, Pb = |B|^2; floor = max(max_k Pa, max_k Pb) * fl32(10^(-R / 10));
 *   D[k] = 10 log10((Pa[k] + floor) / (Pb[k] + floor)); lsd = sqrt(mean_k D[k]^2).  floor == 0 (both frames silent):
 *   columns 3..5 are 0.  Each signal is transformed ON ITS OWN (an S/2-point complex radix-2 transform of its even
 *   and odd samples in LDS and the real-transform post-pass), in fp32 with every product and sum rounded on its own;
 *   D^2, (sqrt Pa - sqrt Pb)^2 and Pa are fp32 terms added in fp64 and rounded once.
 *   A sample that is NaN or Inf makes the columns it enters non-finite in that row and touches no other row: 0 and 1
 *   by the arithmetic above; a power Pa[k] or Pb[k] that is not finite makes 3 and 4 NaN, a Pa[k] also 5.
 *   A row's six values depend on that row's data, S, L, R, the window and the table only -- not on T, hop, stride, ldo
 *   or the launch: one workgroup of 256 threads per row, every sum in an order fixed by S and L.  A row scored alone
 *   is bit-equal to the same row scored among others; identical x and y give sse = lsd = spec_err = +0 exactly.
 *   One launch; no sync and no read of the device (it may run under capture).
 * RV_EVAL_DIMS: mu, logvar [T, L] fp32 (1 <= T < 2^31, 1 <= L <= 2^20) -> cost [L] fp64,
 *   cost[j] = sum_t -0.5 (1 + lv[t, j] - mu[t, j]^2 - exp(lv[t, j])), every term in fp64.  The rows are taken in blocks
 *   of 256: block b = rows [256 b, 256 b + 256) is added in ascending t from +0, then the block sums are added in
 *   ascending b from +0.  ws / ws_bytes: 8 * ceil(T / 256) * L bytes of device scratch when T > 256 (unused, and may
 *   be NULL / 0, up to 256 rows).  No atomics: bit-identical from run to run.  One launch, two when T > 256.
 * Both return an RV_ERR_* whose message names the field before anything is launched and without reading a device
 * pointer: T, S, hop, stride, L out of range; frames that overrun n_out or src_len; ldo < 6; a null frames, src, out
 * or cost; one of mu / logvar without the other; dynamic_range out of range; a window without twiddles or with an S
 * that is no power of two in [32, 4096]; ws_bytes too small. */
#define RV_MOSAIC_KNN 0
#define RV_MOSAIC_KNN_WORKSPACE 1
#define RV_MOSAIC_GATHER_MEAN 2
#define RV_MOSAIC_OLA 3
#define RV_MOSAIC_TRANSITION 4
#define RV_MOSAIC_PATH_FORWARD 5
#define RV_MOSAIC_PATH_BACKTRACK 6
#define RV_MOSAIC_PATH_WORKSPACE 7
#define RV_MOSAIC_KNN_SMALL 8
#define RV_MOSAIC_KNN_SMALL_WORKSPACE 9
#define RV_MOSAIC_LIVE 10
#define RV_MOSAIC_LIVE_WORKSPACE 11
#define RV_MOSAIC_LIVE_RESET 12
#define RV_MOSAIC_LIVE_DRAIN 13
#define RV_GRAIN_FIT 14
#define RV_GRAIN_GATHER 15
#define RV_EVAL_FRAMES 16
#define RV_EVAL_DIMS 17
/* Latent PCA (csrc/pca.hip, rawaudiovae_kelsey_amd/pca.py): the principal axes of a corpus's
 * latents and edits along them.  All arithmetic is fp64; no op syncs or reads the device, each may run under capture,
 * and each returns an RV_ERR_* whose message names the field before anything is launched and without reading a device
 * pointer: T, L, k, mode out of range; a null q, out, centre, basis, eigenvalues, info, gains, shifts or ws; ldo too
 * small; ws_bytes too small.
 * RV_PCA_MOMENTS: q = x [T, L] fp32 (2 <= T < 2^31, 1 <= L <= 512) -> centre [L] fp64 = the column means and
 *   basis [L, L] fp64 = the sample covariance with ddof = 1 (numpy.cov(x64, rowvar=False)).
 *   Mean: RV_EVAL_DIMS's order: the rows in blocks of 256, block b = rows [256 b, 256 b + 256) added in ascending t
 *   from +0 in fp64, the block sums added in ascending b from +0, one division by T.
 *   Covariance: a second pass over d = (double)x - centre.  T is cut into ranges of 4096 rows; a workgroup owns one
 *   range and one 64 x 64 tile (I, J >= I) of the matrix, stages 32 rows of d at a time in LDS (columns beyond L and
 *   rows beyond the range as zeros, in LDS only) and adds them, four rows per v_mfma_f64_16x16x4_f64, in ascending
 *   row order into its 16 x 16 tiles; 16 x 16 tiles below the diagonal are not computed.  The range's partial tile
 *   goes to ws; a second launch adds the partials of every element (i, j >= i) in ascending range order from +0,
 *   divides once by T - 1 and writes basis[i, j] and basis[j, i] from that one value: exactly symmetric.  No atomics; the bits depend on x, T and L only, not on the launch or the device.  Four launches.
 * RV_PCA_EIG: basis [L, L] symmetric fp64 (1 <= L <= 512), in place -> basis row j = the j-th unit eigenvector,
 *   eigenvalues [L] fp64 in descending order (equal values: the lower Jacobi index first), info [2] int32 =
 *   {sweeps run, 1 if converged else 0}.  Cyclic two-sided Jacobi in fp64 by ONE workgroup of 1024 threads,
 *   the matrix in global memory, __syncthreads() between steps.  n = L rounded up to even; a sweep is the n - 1 steps
 *   of the round-robin (circle) order, step s rotating the n / 2 disjoint pairs {n - 1, s} and
 *   {(s + m) mod (n - 1), (s - m) mod (n - 1)}, m = 1 .. n / 2 - 1, each as (p < q), at once (a pair with an index
 *   >= L is skipped).  Rotation of (p, q) with a_pq != 0: theta = (a_qq - a_pp) / (2 a_pq),
 *   t = sgn(theta) / (|theta| + sqrt(theta^2 + 1)) (sgn(0) = 1), c = 1 / sqrt(t^2 + 1), s = t c; a_pp -= t a_pq,
 *   a_qq += t a_pq, a_pq = 0; every other 2 x 2 block (pair, pair) gets the rotation of the lower pair number first,
 *   so the matrix stays bitwise symmetric.  Before every sweep the off-diagonal Frobenius norm is summed directly
 *   over the off-diagonal entries; the solver stops when it is <= L 2^-52 ||C||_F (||C||_F of the input), or after 40
 *   sweeps.  Sign: the entry of largest magnitude of each eigenvector is positive (exact ties: the lowest index).
 *   Negative eigenvalues are reported as computed.  One launch.  ws: 8 L^2 bytes.
 * RV_PCA_APPLY: mode = RV_PCA_PROJECT / RV_PCA_RECONSTRUCT / RV_PCA_EDIT; 1 <= T < 2^31, 1 <= k <= L <= 512;
 *   basis [k, L] fp64 = the first k components v_j, centre [L] fp64, eigenvalues [k] fp64 = theirs (read by EDIT
 *   only).  Rows are independent: a row's bits do not depend on T or on the launch.  Every dot product is one chain
 *   acc = fma(a, b, acc) in ascending index from +0 in fp64; each output is rounded to fp32 once.
 *   PROJECT      q = x [T, L] -> out [T, ldo >= k]: y_j = sum_l (x_l - centre_l) v_jl
 *   RECONSTRUCT  q = y [T, k] -> out [T, ldo >= L]: centre_l + sum_j y_j v_jl
 *   EDIT         q = x [T, L], gains g [k] fp32, shifts h [k] fp32, both on the device -> out [T, ldo >= L]:
 *                x_l + sum_j ((g_j - 1) y_j + h_j sqrt(max(eigenvalues_j, 0))) v_jl with y_j of PROJECT unrounded; where the
 *                sum is zero the output is x_l itself, so g = 1, h = 0 returns x bit for bit.
 *   Only columns [0, k) (PROJECT) or [0, L) of out are written.  One launch.
 * RV_PCA_WORKSPACE: the bytes of ws for RV_PCA_EIG at L and, when T >= 2 (T = 0: EIG only), RV_PCA_MOMENTS at (T, L),
 *   in d->ws_bytes; launches nothing and touches no device. */
#define RV_PCA_MOMENTS 18
#define RV_PCA_EIG 19
#define RV_PCA_APPLY 20
#define RV_PCA_WORKSPACE 21
#define RV_PCA_PROJECT 0
#define RV_PCA_RECONSTRUCT 1
#define RV_PCA_EDIT 2
/* Latent walk (csrc/walk.hip, rawaudiovae_kelsey_amd/walk.py): a first-order linear-Gaussian
 * model of how a corpus's latents move from one frame to the next, in whitened principal coordinates, and its run as a
 * generator of new latent rows.  It extends "Latent PCA" above and keeps its conventions: no op syncs or reads a
 * device pointer on the host, each may run under capture, and each returns an RV_ERR_* whose message names the field
 * before anything is launched.
 * The model.  x [T, L] fp32 are the corpus's latents in file order, file f owning rows [row_start[f], row_start[f+1]);
 * c, v_j, lambda_j the centre, components and eigenvalues (ddof = 1) of RV_PCA_MOMENTS / RV_PCA_EIG on x.  The walk
 * keeps the first k axes, lambda_j > 0 on each.  P [k, L] has rows v_j / sqrt(lambda_j) and R [k, L] rows
 * sqrt(lambda_j) v_j.  With C1 the lag-1 moment below, A = P C1 P^T [k, k], Q = I - A A^T, Q = U diag(q) U^T and
 * B = U diag(sqrt(max(q, 0))), so that A A^T + B B^T = I.  C1 is divided by T - 1, the covariance's own divisor: the
 * Gram matrix of the frames stacked with their successors (zero at file ends) is positive semidefinite with both
 * diagonal blocks (T - 1) C0, hence ||A||_2 <= 1 and the state w' = A w + B e, e ~ N(0, I), is stable and has I as its
 * stationary covariance: the latent rows c + R^T w have the corpus's mean and its covariance on the kept axes.
 * RV_PCA_LAGCOV: q = x [T, L] fp32 (2 <= T < 2^31, 1 <= L <= 512), row_start [n_rows + 1] int64 on the device
 *   (n_rows = the files, 1 <= n_rows <= T; ascending from 0 to T: the CALLER checks that on its host copy, the library
 *   never reads the pointer and the kernels only compare its values), centre [L] fp64 -> basis = C1 [L, L] fp64,
 *   C1[i, j] = (1 / (T - 1)) sum d[t+1, i] d[t, j], d[t] = (double)x[t] - centre, over the pairs (t, t + 1) of one file (a
 *   file of one row has none).  C1 is the full matrix and is not symmetric.  RV_PCA_MOMENTS' discipline: the T - 1
 *   pairs are cut into ranges of 4096 in ascending order; a workgroup owns one range and one 64 x 64 tile, stages 32
 *   pairs at a time in LDS (row t + 1 left, row t right, zero where the pair crosses a file end, where a column is
 *   beyond L or a pair beyond the range) and adds them, four pairs per v_mfma_f64_16x16x4_f64, in ascending order; the
 *   range's partial tile goes to ws and a last launch adds the partials of every element in ascending range order from
 *   +0 and divides once by T - 1.  No atomics; the bits depend on x, row_start, T and L only.  Three launches.
 * RV_WALK_FIT: the dense fp64 products of the fit; every sum is one chain acc = fma(a, b, acc) in ascending index from
 *   +0.  1 <= k <= L <= 512.
 *   mode RV_WALK_DYNAMICS: basis [k, L], eigenvalues = lambda [k], moment = C1 [L, L] fp64 -> result = fp64 [A (k k) | Q (k k) |
 *     P (k L) | R (k L)]: P = v / sqrt(lambda), R = sqrt(lambda) v, M = P C1 (in ws, 8 k L bytes), A = M P^T;
 *     Q[i, j] for i <= j = (i == j ? 1 : 0) - sum_m A[i, m] A[j, m], written to [i, j] and [j, i]: bitwise symmetric.
 *   mode RV_WALK_NOISE: basis = A [k, k], moment = the eigenvectors of Q as RV_PCA_EIG leaves them (row j the j-th) fp64,
 *     eigenvalues = q [k] -> result = fp64 [A^T | B^T] (2 k k), B^T[j, i] = sqrt(max(q_j, 0)) u_j[i]: the layout RV_WALK_STEP
 *     reads, consecutive lanes at consecutive addresses.
 *   mode RV_WALK_DIAGONAL: basis = A [k, k] -> result = [A^T | B^T] of the diagonal model: a_jj on the diagonal of the
 *     first, sqrt(max(fma(-a_jj, a_jj, 1), 0)) on that of the second, zeros elsewhere (|a_jj| <= ||A||_2 <= 1).
 * RV_WALK_STEP: one block of every stream of *live generated, enqueued without a sync: the step launch, then
 *   rv_stream_process's fc3, fc4 and overlap-add launches (four in all).  live carries the model's decoder, the block
 *   output y, window, norm, the stream workspace (frame counters, overlap-add tail), seed, temperature [n_streams],
 *   offset [n_streams, L] and eps_in; its x must be a readable block (it only feeds the unused input history), and
 *   scale, mu, logvar are not read.  L = live->L, 1 <= k <= L <= 512; centre [L], basis = R [k, L], moment = [A^T | B^T]
 *   fp64; state = w [n_streams, k] fp64 and primed = the flags [n_streams] int32, both read and written.
 *   One workgroup per stream steps the F = block / hop frames of the call in order.  For stream s, absolute frame f
 *   (the stream workspace's counter) and axis j: e_j = (double)temperature[s] * (double)eps, eps = eps_in[(s F + frame)
 *   k + j] (eps_in is [n_streams * F, k] here) or, with eps_in NULL, Philox(seed) at index f k + j, offset s: element
 *   f k + j of rv_randn(seed, offset = s).  Not primed: w = e and the flag is set.  Otherwise w'_i is ONE chain
 *   acc = fma(A[i, j], w_j, acc) over ascending j from +0 continued by fma(B[i, j], e_j, acc) over ascending j.
 *   The latent row: z_l = (float)(centre_l + (double)offset[s, l] + chain_j fma(w_j, R[j, l], .)), written to the stream
 *   workspace's latent row s F + frame and, when out is not NULL, to out [n_streams * F, ldo >= L].  A stream's bits
 *   depend on its own state, noise and controls only, not on n_streams or on the block length.
 * RV_WALK_WORKSPACE: the bytes of ws for RV_WALK_FIT at (k, L) (k = 0: none) and, when T >= 2 (T = 0: none),
 *   RV_PCA_LAGCOV at (T, L), in d->ws_bytes; launches nothing and touches no device. */
#define RV_PCA_LAGCOV 22
#define RV_WALK_FIT 23
#define RV_WALK_STEP 24
#define RV_WALK_WORKSPACE 25
#define RV_WALK_DYNAMICS 0
#define RV_WALK_NOISE 1
#define RV_WALK_DIAGONAL 2
#define RV_LIVE_GRAINS 0
#define RV_LIVE_DECODE 1
/* Latent alignment (csrc/align.hip, rawaudiovae_kelsey_amd/align.py): a monotone alignment of two
 * latent trajectories by dynamic time warping, over the whole matrix or a band around the straight line.  The family's
 * conventions: no op syncs or reads a device pointer on the host, each may run under capture, and each returns an RV_ERR_*
 * whose message names the field before anything is launched: T, N, L, band, mode, penalty, a null a / b / local_costs / ws / path /
 * summary / path_costs / warp_table, ws_bytes too small.
 * Notation: a [Ta, L] fp32 with Ta = T; b [Tb, L] fp32 with Tb = N; rows contiguous; 1 <= L <= 4096; r = band >= 0;
 * p = penalty, the step penalty, finite and >= 0.
 * The band.  r = 0: the whole matrix, W = Tb, the band-local column of j is j.  r >= 1: centre(i) =
 * floor(i (Tb - 1) / max(Ta - 1, 1)) in integer arithmetic; cell (i, j) is in the band iff |j - centre(i)| <= r and
 * 0 <= j < Tb; W = 2 r + 1 and the band-local column of j is j - centre(i) + r.  The band admits a path iff
 * ceil((Tb - 1) / (Ta - 1)) <= 2 r + 1 for Ta > 1, or Tb - 1 <= r for Ta = 1; a band that does not is RV_ERR_SHAPE naming
 * band and the least r that would do.  Ta W < 2^31.
 * RV_ALIGN_COST: a, b, L, T, N, band -> local_costs = Dm [Ta, W] fp32, Dm[i, col(j)] = D(a_i, b_j), D RV_MOSAIC_KNN's distance
 *   bit for bit: part = fmaf(d, d, part) in ascending l within tiles of 32, tot += part per tile, from +0.  A band slot
 *   whose j falls outside [0, Tb) is written +inf; every slot of Dm is written.  One launch over (blocks of 128 rows of
 *   a, tiles of 64 columns of the block's band), RV_MOSAIC_KNN's register tile; no atomics; the bits depend on a, b, L and
 *   the band only.
 * RV_ALIGN_FORWARD: local_costs = Dm, T, N, band, mode = RV_ALIGN_GLOBAL or RV_ALIGN_SUBSEQUENCE (the latter requires band 0),
 *   penalty, ws.  The accumulated cost C is fp64.  The cell rule: dd = (double)Dm[i, j]; a NaN or +inf makes the cell
 *   blocked: C = +inf, step = 3.  The candidates in this order: 0 diag: C[i-1, j-1]; 1 up: fl64(C[i-1, j] + (double)p);
 *   2 left: fl64(C[i, j-1] + (double)p); anything outside the matrix or the band is +inf.  best = +inf, step = 3, then in
 *   that order `if (cand < best) { best = cand; step = k; }`: ties go diag, up, left, and +inf or NaN never wins.
 *   C[i, j] = step == 3 ? +inf : fl64(dd + best).  Start cells (C = dd, step 3): GLOBAL: (0, 0) only; SUBSEQUENCE: every
 *   (0, j), and row 0 takes no left move.  End: GLOBAL: (Ta - 1, Tb - 1); SUBSEQUENCE: the lowest-j argmin of the finite
 *   C[Ta - 1, .], and when end_costs is not NULL, C[Ta - 1, .] is also written there as [Tb] fp64.  ONE workgroup of 1024
 *   threads sweeps the anti-diagonals d = i + j in ascending order, a cell per thread (looping when a diagonal is
 *   longer), a barrier between the diagonals; three rolling diagonals of C in LDS while no diagonal has more than 2048
 *   cells, in ws otherwise; the step codes go to a back table [Ta, W] uint8 in ws.  One launch, no atomics, no polling.
 * RV_ALIGN_BACKTRACK: local_costs = Dm, T, N, band, ws as FORWARD left it -> path [Ta + Tb - 1, 2] int32, the (i, j) pairs
 *   in ascending order, rows >= P filled with -1; summary [4] int32 = {P, j of the first pair, j of the last pair, reached
 *   (1 / 0)}; path_costs [2] fp64 = {C at the end cell, the sum of (double)Dm along the path added in ascending order from +0}:
 *   with p = 0 the two are the same bits.  Not reached (no finite end cell): P = 0, reached = 0, path_costs = {+inf, 0}, path all
 *   -1, summary[1] = summary[2] = -1.  The walk is bounded by Ta + Tb - 1 steps whatever the table holds.  One launch.
 * RV_ALIGN_WARP: path, summary, T, N, mode = the timeline RV_ALIGN_ON_A, RV_ALIGN_ON_B or RV_ALIGN_ON_PATH ->
 *   warp_table [n, 2] int32 = (ia, ib).  ON_A: n = Ta, ia[i] = i, ib[i] = path[m, 1] for the LOWEST m with path[m, 0] = i.  ON_B:
 *   the mirror image, n = Tb.  ON_PATH: n = Ta + Tb - 1, the path itself, -1 beyond P.  A row the path never visits gets
 *   (-1, -1).  Every entry of warp_table is written by exactly one thread.
 * RV_ALIGN_WORKSPACE: the bytes of ws of FORWARD and BACKTRACK for (T, N, band) in d->ws_bytes; launches nothing and
 *   touches no device.  ws is 256-byte aligned. */
#define RV_ALIGN_COST 26
#define RV_ALIGN_FORWARD 27
#define RV_ALIGN_BACKTRACK 28
#define RV_ALIGN_WARP 29
#define RV_ALIGN_WORKSPACE 30
#define RV_ALIGN_GLOBAL 0
#define RV_ALIGN_SUBSEQUENCE 1
#define RV_ALIGN_ON_A 0
#define RV_ALIGN_ON_B 1
#define RV_ALIGN_ON_PATH 2
/* Latent structure (csrc/structure.hip, rawaudiovae_kelsey_amd/structure.py): where a latent
 * trajectory changes.  A novelty curve from the banded self-distance matrix of the trajectory, and the boundaries picked
 * from it.  The family's conventions: no op syncs or reads a device pointer on the host, each may run under capture, and
 * each returns an RV_ERR_* whose message names the field before anything is launched: T, band, k, lag, width, lam, a null
 * local_costs / moment / result / path / summary / ws, ws_bytes too small.
 * The matrix.  RV_ALIGN_COST with a = b = mu [T, L] and N = T writes Dm [T, W] fp32: centre(i) = i, so band = 0 is the
 * whole matrix (W = T, the column of j is j) and band = r >= 1 keeps |j - i| <= r (W = 2 r + 1, the column of j is
 * j - i + r).  T W < 2^31.
 * RV_STRUCT_NOVELTY: T >= 1, local_costs = Dm, band = 0 or r >= 2 R - 1 (a narrower band is RV_ERR_SHAPE naming band and
 *   2 R - 1, the least that holds the window), k = R, the half-width of the kernel in frames, 1 <= R <= 512,
 *   moment = the taper w [2 R] fp64 on the device -> result = nov [T] fp64.  For frame t the offsets u, v run over
 *   [-R, R), i = t + u, j = t + v; a term whose i or j is outside [0, T) is skipped, by index (the +inf of such a band
 *   slot is never read).  c(u, v) = fl64(w[u + R] * w[v + R]), d = (double)Dm[i, col(j)]; a term is CROSS when
 *   (u < 0) != (v < 0), WITHIN otherwise.  Row u has four fp64 chains over ascending v, each from +0:
 *   cross_u += fl64(c * d) and wc_u += c over its cross terms, within_u += fl64(c * d) and ww_u += c over its within
 *   terms: every product is rounded before it is added, nothing is contracted into an fma.  The four row results are
 *   added over ascending u from +0 into Cross, Wc, Within, Ww, and nov[t] = Cross / Wc - Within / Ww when Wc > 0 and
 *   Ww > 0, +0 otherwise (t = 0 has no past: +0).  A NaN in Dm makes NaN exactly the nov[t] whose window holds it.  A
 *   thread per (frame t, row u), 1024 threads to a workgroup: it takes floor(1024 / 2R) consecutive frames and stages
 *   the window they share once, through LDS in chunks of 32 columns, the chains carried across the chunks in
 *   ascending v; the row results go through LDS and one lane per (frame, chain) adds them in ascending u.  One launch,
 *   no atomics; the bits depend on Dm, T, R and w only, not on the band or on the launch: the whole matrix and any
 *   admissible band give the same bits.
 * RV_STRUCT_PEAKS: T >= 1, moment = nov [T] fp64, lag = g, the minimum gap in frames, 0 <= g <= 65536, width = m, the
 *   radius of the local mean, 0 <= m <= 65536, lam = delta, finite and >= 0, ws / ws_bytes -> path = offsets [T + 1]
 *   int32, summary [4] int32.  G = the mean of |nov[t]| over the finite entries: RV_EVAL_DIMS's order (blocks of 256 rows
 *   added in ascending t from +0, the block sums added in ascending order from +0), one division by their count, 0 when
 *   there is none.  m[t] = the mean of the finite nov[t'], t' in [max(0, t - m), min(T - 1, t + m)], added in ascending
 *   t' from +0 and divided once by their count.  With ge = max(g, 1), frame t is a boundary iff ge <= t <= T - ge and
 *   t < T; nov[t] is finite; nov[t] > fl64(m[t] + fl64((double)delta * G)); nov[t] > nov[t'] for every finite t' in
 *   [t - g, t); nov[t] >= nov[t'] for every finite t' in (t, t + g].  Ties go to the earlier frame; a NaN never wins
 *   and is never compared.  Two boundaries are more than g frames apart and every segment is non-empty.
 *   path[0] = 0, then the boundaries in ascending order, path[F] = T, then -1 up to path[T]; F >= 1 is the number of
 *   segments; summary = {F, the number of finite entries of nov, 0, 0}.  Every entry of path and summary is written, each
 *   by one thread; the compaction is a scan in ascending t (per 256 frames, then over the blocks), no atomics.  Five
 *   launches.
 * RV_STRUCT_WORKSPACE: the bytes of ws of RV_STRUCT_PEAKS for T in d->ws_bytes; launches nothing and touches no device.
 *   ws is 256-byte aligned. */
#define RV_STRUCT_NOVELTY 31
#define RV_STRUCT_PEAKS 32
#define RV_STRUCT_WORKSPACE 33
/* Latent restoration (csrc/smooth.hip, rawaudiovae_kelsey_amd/smooth.py): inference with the model
 * of "Latent walk" above, w' = A w + B e with A A^T + B B^T = I: a Kalman filter and a fixed-interval smoother over
 * sequences of latent rows whose frames are partly missing, and the splice of a resynthesis into the original.  The
 * family's conventions: no op syncs or reads a device pointer on the host, each may run under capture, and each returns
 * an RV_ERR_* whose message names the field before anything is launched: mode, T, L, k, n_rows, lam, a null q / row_start /
 * centre / basis / moment / ws / out / src / frames / room, ws_bytes too small, ws not 256-byte aligned, ldo, n_out, width.
 * The model, per sequence.  q = x [T, L] fp32 (1 <= T < 2^31); sequence s owns rows [row_start[s], row_start[s+1]),
 * row_start [n_rows + 1] int64 on the device, ascending from 0 to T (the CALLER checks that on its host copy; the kernels
 * clamp what they read to [0, T]).  centre = c [L], P, R [k, L] and moment = dyn = [A^T | B^T] [2, k, k] fp64 are the fitted
 * walk's arrays.  Qn = B B^T, element (i, j), i <= j, one chain fma(B[i, m], B[j, m], .) in ascending m from +0, written to
 * [i, j] and [j, i].  The observation of frame t is y_t = P (x_t - c): y_j = chain fma(P[j, l], (double)x[t, l] - c[l], .) in
 * ascending l from +0 (fp64 from the fp32 row, not RV_PCA_APPLY's rounded output).  Its noise is r_t I, r = lam (finite,
 * 1e-8 <= r <= 1e8), r_t = fl64((double)r / (double)weight[t]).  Frame t is OBSERVED iff weight[t] > 0 (weight [T] fp32;
 * NaN, 0 and negative: missing); weight NULL: every frame observed with weight 1.  The row x_t of a missing frame is never
 * read and may hold NaN.
 * dot4: every inner product below is four chains of fmas over the indices m mod 4 = 0 .. 3, each in ascending m from +0,
 * added as (a0 + a1) + (a2 + a3).
 * mode RV_SMOOTH_DENSE: 1 <= k <= 64 (more is RV_ERR_SHAPE naming k and the limit), k <= L <= 512.  mode
 * RV_SMOOTH_DIAGONAL: the caller asserts that A^T and B^T are diagonal, only their diagonals are read, k independent
 * scalar filters, 1 <= k <= L <= 512, ws is O(k) per frame.
 * RV_SMOOTH_FILTER: q, weight, lam, centre, basis = P, moment = dyn, T, L, k, n_rows, row_start, mode, ws, ws_bytes ->
 *   result [T, ldo >= k + 2] fp64 or NULL.  Per sequence in ascending t.  First frame: w- = 0, P- = I (the walk's
 *   stationary law).  Later: w- = A w+, M = A P+, P-[i, j] = dot4(M[i, .], A[j, .]) + Qn[i, j] for i <= j, mirrored.
 *   Missing frame: w+ = w-, P+ = P-.  Observed: S = P- + r_t I = G G^T, v = y_t - w-, and with base = [S; P-; v^T]
 *   (2 k + 1 rows) every row r obeys, column after column, Y[r, j] = (base[r, j] - dot4(Y[r, :j], G[j, :j])) / G[j, j],
 *   G[j, j] = sqrt(S[j, j] - dot4(G[j, :j], G[j, :j])): rows [0, k) are G (Cholesky-Crout), rows [k, 2 k) W^T = P- G^-T
 *   and the last a = G^-1 v, the forward solves folded into the factorisation.  w+ = w- + W^T a (= w- + P- u with
 *   u = S^-1 v = G^-T a); P+[i, j] = P-[i, j] - dot4(W^T[i, .], W^T[j, .]) for i <= j, mirrored.  P- <= I always, so
 *   cond(S) <= (1 + r_t) / r_t: why r has a floor and no inverse of P- appears.  A row of result: [0, k) w+; column k
 *   the normalised innovation squared v^T u = a^T a (missing: -1); column k + 1 log det S = 2 sum log G[j, j] in ascending
 *   j (missing: 0).  ws receives y, w-, a, diag G and the tile [P- upper triangle | G strict lower triangle] of every frame.
 *   DIAGONAL, axis j with a = A[j, j], q = B[j, j]^2: w- = a w+, P- = fma(a P+, a, q); S = P- + r_t, u = v / S,
 *   w+ = fma(P-, u, w-), P+ = P- r_t / S; the columns k and k + 1 are sum_j v_j u_j and sum_j log S_j in ascending j from
 *   +0.  One workgroup per sequence (dense: A, the covariance and Y in 132.5 KB of LDS at k = 64, opted in by launch
 *   attribute; diagonal: a thread per axis, no barrier) behind the launches of Qn and y: three launches (diagonal with
 *   result: also three).
 * RV_SMOOTH_BACKWARD: the modified Bryson-Frazier recursion, which needs S^-1 only.  q, weight, lam, centre, basis = R,
 *   moment = dyn and ws as FILTER left it for the same (T, L, k, n_rows, row_start, mode) -> out [T, ldo >= L] fp32 (only
 *   columns [0, L) are written) and state [T, k] fp64 or NULL.  Per sequence in descending t from lambda = 0.  Observed:
 *   lambda-hat = lambda + G^-T (a - G^-1 (P- lambda)) (= u + lambda - S^-1 P- lambda), two substitutions with the
 *   reciprocals of diag G; missing: lambda-hat = lambda.  w-hat_t = w-_t + P-_t lambda-hat; lambda <- A^T lambda-hat.
 *   DIAGONAL: lambda-hat = u + lambda - P- lambda / S, w-hat = fma(P-, lambda-hat, w-), lambda <- a lambda-hat.
 *   The latent row: z_l = (float)(c_l + chain_j fma(w-hat_j, R[j, l], .) + g_t rho_l), rho_l = (double)x[t, l] - c_l -
 *   chain_j fma(y_j, R[j, l], .), the part of an observed row outside the kept axes; g_t = 1 observed, 0 missing (rho is
 *   then not computed): a frame the model does not touch keeps what the walk cannot see.  Two launches.  BACKWARD
 *   leaves FILTER's part of ws as it was (w-hat has its own place) and may be repeated.
 *   A sequence's bits depend on its own rows, weights and the model only, not on n_rows, on where it lies in x or on
 *   the launch; w+[t] depends on the frames up to t only.  No atomics, no polling.
 * RV_SMOOTH_SPLICE: src = the original [n_out] fp32, frames = the resynthesis [n_out] fp32, room [n_rows, 2] int32 on
 *   the device = the damaged sample ranges [s, e), ascending and disjoint (the CALLER checks that), 1 <= n_rows,
 *   width = F >= 0 fade samples, 1 <= n_out < 2^31 -> out [n_out], out[n] = (float)((1 - g) (double)src[n] + g
 *   (double)frames[n]), both products rounded.  d = the distance from n to the nearest range (0 inside);
 *   g = 1 for d = 0, g = 0.5 + 0.5 cos(pi d / (F + 1)) for 1 <= d <= F (the maximum over the ranges where ramps meet),
 *   g = 0 beyond.  Where g = 0 the output is src[n] bit for bit, where g = 1 frames[n] bit for bit.  One launch, every
 *   sample written by one thread.
 * RV_SMOOTH_WORKSPACE: the bytes of ws for (T, L, k, mode) in d->ws_bytes; launches nothing and touches no device.  ws is
 *   256-byte aligned.  Dense: 8 (k^2 rounded up to 256 bytes + T k (k + 5)); diagonal: 64 T k. */
#define RV_SMOOTH_FILTER 34
#define RV_SMOOTH_BACKWARD 35
#define RV_SMOOTH_SPLICE 36
#define RV_SMOOTH_WORKSPACE 37
#define RV_SMOOTH_DENSE 0
#define RV_SMOOTH_DIAGONAL 1
/* Latent recurrence (csrc/recur.hip, rawaudiovae_kelsey_amd/recur.py): what repeats in a latent
 * trajectory.  The matrix profile of a distance matrix: for every window of m consecutive frames the nearest other
 * window under the sum of the frame distances along a diagonal.  The family's conventions: no op syncs or reads a device
 * pointer on the host, each may run under capture, and each returns an RV_ERR_* whose message names the field before
 * anything is launched: k, T, N, splits, n_rows, stride, row0, lag, width, mode, a null local_costs / result / idx / ws,
 * ws_bytes too small, ws not 256-byte aligned.  No atomics, no polling.  The op codes 38 and 39 are unassigned: rv_mosaic
 * answers them as unknown ops.
 * RV_RECUR_PROFILE: local_costs = Dm fp32, n_rows rows of N columns with a row pitch of stride >= N elements,
 *   Dm[r, j] = D(a[row0 + r], b[j]): what RV_ALIGN_COST with band 0 writes for a slab of a's rows (stride = N).  k = m,
 *   the window in frames, 1 <= m <= 256.  T = n_rows - m + 1 >= 1, the windows of the slab: a T that disagrees is
 *   RV_ERR_SHAPE naming T and n_rows.  N >= m; window j exists for 0 <= j <= N - m.  n_rows stride < 2^31.  row0 >= 0,
 *   the slab's first row in the whole recording.  lag = lo and width = hi, lo <= hi, any sign, |lo|, |hi| < 2^31.
 *   mode = 0 or RV_RECUR_MIRROR.
 *   Admission.  With g = row0 + i, window j is admitted for row i iff lo <= j - g <= hi, and under RV_RECUR_MIRROR also
 *   iff lo <= g - j <= hi.  A self-join with an exclusion zone of e frames: lo = e, hi = 2^31 - 1, MIRROR.  Loop
 *   candidates: lo = the shortest loop, hi = the longest, no mirror.  A join against another recording: the full range.
 *   The window sum W(i, j) is ONE fp64 chain: s = +0, then s += (double)Dm[i + u, j + u] for u = 0 .. m - 1 in ascending
 *   u.  A direct sum for every cell, neither a sliding update nor a difference of prefix sums: the bits depend on Dm, m,
 *   i and j only, not on the slab, the tiling, splits or the launch.
 *   -> result = P [T] fp64 and idx = I [T] int32: over the admitted j whose W is finite, (P[i], I[i]) is the least (W, j),
 *   ordered by the smaller W, then the lower j.  NaN and +inf never win; with no such j, P[i] = +inf and I[i] = -1.  Every
 *   entry of P and I is written by exactly one thread.  Cells outside the matrix are skipped by index, the padding
 *   between N and stride is never read, and a cell of Dm is read only for an admitted diagonal.
 *   splits = the workgroups the columns of a block of 16 rows are divided among, 0 <= splits <= 1024; 0 = the library's
 *   choice, which fills the chip for any T.  With more than one split the partial (W, j) pairs go to ws (ws_bytes) and a
 *   second launch takes their least; the order is total, so the result is the same bits for every split count.  With
 *   one split ws is not read.
 *   A workgroup takes 16 rows and walks its share of the diagonals j - i in tiles of 256, a thread per diagonal: the 16
 *   windows of a diagonal share all but 15 of their cells, so the thread reads each cell once (a wave reads consecutive
 *   columns of one row) and adds it to the chain of every window that holds it, each chain in its own ascending u.  It
 *   keeps the best pair of every row in registers across the tiles; a wave reduction and a cross-wave reduction under
 *   the (W, j) order close the rows.
 * RV_RECUR_WORKSPACE: the bytes of ws of RV_RECUR_PROFILE for (T, N, k, splits) in d->ws_bytes (0 with one split);
 *   launches nothing and touches no device.  ws is 256-byte aligned. */
#define RV_RECUR_PROFILE 40
#define RV_RECUR_WORKSPACE 41
#define RV_RECUR_MIRROR 1
/* Latent states (csrc/hmm.hip, rawaudiovae_kelsey_amd/states.py): a hidden Markov model with
 * diagonal Gaussian emissions over the whitened coordinates of "Latent restoration", fitted to a whole corpus by EM.  The
 * family's conventions: no op syncs or reads a device pointer on the host, each may run under capture, and each returns an
 * RV_ERR_* whose message names the field before anything is launched: T, S, k, L, stride, n_rows, lam, mode, a null q / centre /
 * basis / moment / result / state / info / path / score / row_start / ws, ws_bytes too small, ws not 256-byte aligned.  No
 * atomics, no polling; every output element is written by exactly one thread.  No new member and no new role of the
 * descriptor: every field is an existing member under its existing name and type, and S, the frame length of the
 * synthesis ops, counts the states here.  The op code 42 is unassigned like 38 and 39: rv_mosaic answers it as an unknown op.
 * The fields.  moment = theta, the parameter block.  result = logb [T, S] fp64 (EMIT writes it, FORWARD_BACKWARD and VITERBI
 * read it); in MSTEP result = the new parameter block.  state = the posteriors, ONE block of T S + n_rows S S + n_rows
 * doubles: [ gamma (T S) | xi (n_rows S S) | ll (n_rows) ], which FORWARD_BACKWARD writes and MSTEP reads.
 * The model.  S = the states, 1 <= S <= 64; k = the axes, 1 <= k <= 64; k <= L <= 512; 1 <= T < 2^31; more is RV_ERR_SHAPE
 * naming the field and its limit.  q = x [T, L] fp32 with a row pitch of stride >= L elements, centre = c [L] and basis = P
 * [k, L] fp64 (a fitted PCA's or walk's).  y_t = P (x_t - c): y_j = chain fma(P[j, l], (double)x[t, l] - c[l], .) in
 * ascending l from +0, the device code RV_SMOOTH_FILTER observes with (csrc/sequence.h).  A frame whose x row holds a value
 * that is not finite is UNOBSERVED.  State s emits N(m_s, diag(v_s)) in these coordinates; pi [S] is the initial law and
 * A [S, S] the transition matrix (rows sum to 1).  theta, fp64 on the device, 2 S k + 3 S + 2 S^2 doubles:
 *   [ m (S k) | w = 1 / v (S k) | g (S) | pi (S) | A (S S) | log pi (S) | log A (S S) ]
 * with g_s = -0.5 (k log(2 pi) + sum_j log v_sj): fl(k * fl64(log(2 pi))), the logarithms added in ascending j from +0, one
 * add, one product.  Sequence s owns rows [row_start[s], row_start[s+1]), row_start [n_rows + 1] int64 on the device,
 * 1 <= n_rows < 2^31, under RV_SMOOTH_FILTER's rules (the CALLER checks it on its host copy, the kernels clamp to [0, T]);
 * an empty sequence is legal and contributes nothing.
 * RV_HMM_EMIT: q, stride, centre, basis, moment = theta, T, L, k, S -> result = logb [T, S] fp64.  logb[t, s] = g_s - 0.5 q with q one chain
 *   fma(fl(w_sj d), d, .), d = y_j - m_sj, in ascending j from +0 (the product w_sj d rounded on its own).  An unobserved
 *   frame gets a row of NaN and changes no other row.  A workgroup takes 64 frames, stages their y in LDS once and writes
 *   the rows of all S states; one launch over the whole chip.
 * RV_HMM_FORWARD_BACKWARD: result = logb, row_start, n_rows, moment = theta, T, S, k, ws, ws_bytes -> state = the
 *   posteriors: gamma [T, S], xi [n_rows, S, S] and ll [n_rows], all fp64.  The scaled recursion, one workgroup per sequence.  A frame is unobserved iff its row of logb
 *   holds a NaN: then M_t = 0 and b~_t[s] = 1; else M_t = max_s logb[t, s] and b~_t[s] = exp(logb[t, s] - M_t).
 *   Forward: alpha_0[j] = fl(pi_j b~_0[j]); alpha_t[j] = fl(b~_t[j] * chain_i fma(alpha_{t-1}[i], A[i, j], .)) in ascending i
 *   from +0; c_t = sum_j alpha_t[j] in ascending j from +0; alpha_t /= c_t; ll = fl(ll + fl(log c_t + M_t)) in ascending t
 *   from +0.  Backward in descending t from beta = 1: u_j = fl(b~_{t+1}[j] beta_{t+1}[j]) / c_{t+1}, beta_t[i] =
 *   chain_j fma(A[i, j], u_j, .) in ascending j from +0, gamma_t[i] = fl(alpha_t[i] beta_t[i]).  xi[seq, i, j] = chain over
 *   the sequence's pairs in descending t from +0 of fma(fl(alpha_t[i] A[i, j]), u_j, .); a sequence of one frame or none
 *   writes zeros, and ll = 0 for an empty one.  alpha and c live in ws.  A stays in LDS for the whole sequence; wave 0
 *   runs the recursion with lane j owning state j, alpha and u passing between its lanes through LDS, and all four waves
 *   accumulate xi in registers, 16 columns of a row per thread.  A sequence's bits depend on its own rows and theta only,
 *   not on n_rows or on where it lies.
 * RV_HMM_MSTEP: q, stride, centre, basis, state = the posteriors (ll is not read), row_start, n_rows, moment = the old
 *   theta, lam = the variance floor (finite, > 0), T, L, k, S, mode = 0 or RV_HMM_MOMENTS, ws, ws_bytes -> result = the new
 *   theta (a block of its own) and info [S] int32; under RV_HMM_MOMENTS result holds S (1 + 2 k) more doubles behind theta,
 *   the moments [S, 1 + 2 k]: row s = [N_s | M1[s, .] | M2[s, .]].  Unobserved frames contribute nothing to the
 *   three moments.  N_s = sum_t gamma[t, s]: blocks of 256 frames, a block in ascending t from +0, the blocks in
 *   ascending order from +0.  M1 = gamma^T Y and M2 = gamma^T (Y o Y), y^2 one rounded product: ranges of 4096 frames,
 *   within a range v_mfma_f64_16x16x4_f64 over the frames t0, t0 + 4, .. in ascending order from +0, each instruction
 *   adding its four frames to the element, 32 frames staged in LDS at a time, the partial tiles to ws, then the ranges in
 *   ascending order from +0: the tile and the sums of "Latent PCA", in the tile's two-operand form.  Then m = M1 / N,
 *   v = max(fl(M2 / N - fl(m m)), lam) (NaN gives lam), w = 1 / v, g as above.  A state with N_s < 1 (or NaN) keeps its old
 *   m, w and g, and info[s] = 1 (else 0).  pi_s = the mean over the non-empty sequences of their first frame's gamma,
 *   added in ascending sequence order from +0 (no such sequence: the old pi).  A[i, j] = (sum_seq xi[seq, i, j] in ascending
 *   seq from +0) / (the sum of row i's numerators in ascending j from +0); a row whose sum is not positive keeps its old row.
 *   log pi and log A with log(0) = -inf.  Four launches; the last is one workgroup.
 * RV_HMM_VITERBI: result = logb, row_start, n_rows, moment = theta, T, S, k, ws, ws_bytes -> path [T] int32, score [n_rows]
 *   fp64.  Max-plus in
 *   fp64 with plain adds: d_0[j] = a_0[j] + log pi_j, d_t[j] = a_t[j] + max_i (d_{t-1}[i] + log A[i, j]), a_t[j] = logb[t, j], or
 *   0 in an unobserved frame (a NaN in the row).  The max is taken under the total order larger value first, then lower
 *   i; NaN and -inf never win, and where nothing wins d_t[j] = a_t[j] + (-inf).  score = the best d of the last frame under
 *   the same order and the path goes back from its state; where no end state wins, score = -inf and the sequence's path
 *   is -1 throughout.  An empty sequence: score = 0.  Rows outside every sequence are not written.  One wave per
 *   sequence, log A in LDS, the back-pointers bytes in ws.  Given logb and theta the output is exact.
 * RV_HMM_WORKSPACE: the bytes of ws for (T, S, k) that serve all three in d->ws_bytes; launches nothing and touches no
 *   device.  ws is 256-byte aligned.  One EM iteration is EMIT, FORWARD_BACKWARD and MSTEP on one stream and one ws, no
 *   host sync between them. */
#define RV_HMM_EMIT 43
#define RV_HMM_FORWARD_BACKWARD 44
#define RV_HMM_MSTEP 45
#define RV_HMM_VITERBI 46
#define RV_HMM_WORKSPACE 47
#define RV_HMM_MOMENTS 1
/* Latent attributes (csrc/attr.hip, rawaudiovae_kelsey_amd/attributes.py): audio descriptors of every
 * frame of a waveform, and the linear regression of per-frame targets (those descriptors or the caller's own labels) on the
 * whitened latents of a corpus, whose coefficients turn "this descriptor by that much" into a latent offset.  The family's
 * conventions: no op syncs or reads a device pointer on the host, each may run under capture, and each returns an RV_ERR_*
 * whose message names the field before anything is launched: T, S, hop, k, N, L, stride, lam, dynamic_range, ldo, frames
 * that overrun n_out, a window without twiddles or with an S that is no power of two in [32, 4096], a null frames / result /
 * q / centre / basis / moment / info / ws, ws_bytes too small, ws not 256-byte aligned.  No atomics, no polling; every output
 * element is written by exactly one thread.  No new member and no new role of the descriptor: every field is an existing
 * member under its existing name and type.  The op code 48 is unassigned like 38, 39 and 42: rv_mosaic answers it as an
 * unknown op.
 * RV_ATTR_DESCRIBE: frames, n_out (a padded waveform [n_out]: frame t = frames[t hop, t hop + S), (T - 1) hop + S <= n_out),
 *   T (1 <= T < 2^31), S, hop (>= 1), window [S] fp32 or NULL, twiddles (RV_EVAL_FRAMES' table, required with a window),
 *   dynamic_range = R in dB, 0 < R <= 120 -> result = desc [T, ldo] fp64; only columns 0..4 (0..2 without a window) of rows
 *   0..T-1 are written.  With a window S is a power of two in [32, 4096] and ldo >= 5; without one any S >= 1 and ldo >= 3.
 *     0  level (dB) = 10 log10(e), e = (1/S) sum_n x[n]^2: the squares and the sum in fp64 in the order of RV_EVAL_FRAMES'
 *        column 1, one division; silence gives -inf
 *     1  zcr = #{1 <= n < S : (x[n] < 0) != (x[n-1] < 0)} / (S - 1): the count an exact integer, one division; 0 at S = 1; a
 *        NaN compares as not negative
 *     2  crest (dB) = 10 log10(p^2 / e), p = max_n |x[n]| (fp32, exact), p^2 one fp64 product; e == 0 gives NaN
 *     3  centroid (cycles/sample) = (sum_k k Pa[k]) / (sum_k Pa[k]) / S over k = 0 .. S/2, the terms (double)k * (double)Pa[k];
 *        a zero denominator gives NaN
 *     4  flatness (dB) over k = 1 .. S/2: 10 log10(G / A), A = (sum_k Pa[k]) / (S/2), G = exp((sum_k log((double)(Pa[k] + fl)))
 *        / (S/2)), fl = max_{k >= 0} Pa[k] * fl32(10^(-R/10)) the fp32 product of RV_EVAL_FRAMES, the add Pa[k] + fl rounded
 *        in fp32; A == 0 gives NaN
 *   Pa = the power spectrum of a[n] = fl32(window[n] x[n]) by the transform of "Evaluation" (csrc/spectrum.h, which both ops
 *   call): fp32, every product and sum rounded on its own.  Every sum over n or k is in fp64: thread u of the frame's 256
 *   takes the terms u, u + 256, .. in ascending order from +0, then the xor butterfly over each wave's lanes and the four
 *   waves' sums left to right.  Every logarithm is the fp64 library one; each dB is one log10 and one product by 10.
 *   A sample that is NaN or Inf makes the columns it enters non-finite in that row and touches no other row; a power that is
 *   not finite makes columns 3 and 4 NaN.  A row's values depend on that row's data, S, R, the window and the table only --
 *   not on T, hop, ldo or the launch.  One workgroup of 256 threads per frame, one launch; LDS: 2 (S/2) + 1 floats and the
 *   reductions' scratch.
 * RV_ATTR_FIT: q = x [T, L] fp32 with a row pitch of stride >= L elements, centre = c [L] and basis = P [k, L] fp64 (rows
 *   v_j / sqrt(lambda_j) of a fitted PCA), moment = the targets D [T, N] fp64, packed, lam = the ridge (finite, >= 0), ws,
 *   ws_bytes, T, L, k, N with 1 <= k <= 64, k <= L <= 512, 1 <= N <= 64, 2 <= T < 2^31 -> result (fp64) and info [2] int32.
 *   A frame is OBSERVED iff its x row and its D row are finite throughout.  y_t = P (x_t - c) by the chain of "Latent states"
 *   (csrc/sequence.h).  Five launches on one stream:
 *   1. y, D and the observed flags to ws, a workgroup per 64 frames; an unobserved frame's y and D rows are written as +0.
 *   2. n = the observed frames and the column sums of y and D over them by the blocked column sum of RV_EVAL_DIMS (blocks of
 *      256 frames in ascending t from +0, then the blocks in ascending order from +0); then ybar = sum / n, dbar = sum / n,
 *      one division each (a launch of its own, one workgroup).
 *   3. Three 64 x 64 tiles per range of 4096 frames: Yc^T Yc, Dc^T Yc and Dc^T Dc of the centred operands u - ubar, with
 *      an unobserved row staged as zeros on both sides: v_mfma_f64_16x16x4_f64 over the frames t0, t0 + 4, .. in ascending
 *      order from +0, 32 frames staged in LDS at a time, the partial tiles to ws -- the tile of "Latent PCA" in a third
 *      operand form (csrc/moment.h).
 *   4. ONE workgroup closes.  Cyy [k, k], Cdy [N, k], Cdd [N, N] = (the ranges' partials in ascending order from +0) / (n - 1).
 *      G = Cyy + lam I (one add on the diagonal).  G = R R^T by the left-looking Cholesky, column j = 0 .. k-1:
 *      s_i = chain fma(-R[i, p], R[j, p], .) from G[i, j] in ascending p < j, for i >= j; R[j, j] = sqrt(s_j), R[i, j] =
 *      s_i / R[j, j].  The pivot s_j counts as positive iff s_j > 2^-40 G[j, j]: an axis that repeats another leaves a pivot
 *      of rounding errors of either sign, which is not one.  For every target a, g = Cdy[a, .]: R z = g with z_j = s_j / R[j, j] and then s_i = fma(-R[i, j], z_j,
 *      s_i) for i > j, in ascending j from s = g; R^T beta = z likewise in descending j.  r2_a = 1 - (Cdd[a, a] - 2 (beta . g)
 *      + beta^T (Cyy beta)) / Cdd[a, a] with (Cyy beta)_i = chain fma(Cyy[i, j], beta_j, .) in ascending j from +0 and the two
 *      dot products summed over the axes by the xor butterfly of one wave (absent axes add +0).  A target with Cdd[a, a] == 0
 *      gets beta = 0 and r2 = 0.
 *   result = [ n | ybar (k) | dbar (N) | Cdd (N N) | B (N k), row a = beta_a | r2 (N) ], 1 + k + 2 N + N N + N k doubles.
 *   info = { status, n }: 0 = ok, 1 = fewer than k + 2 observed frames, 2 = a pivot s_j of the Cholesky was not positive (the rule above).
 *   With a non-zero status B and r2 are written as zeros (n, the means and Cdd by the rules above all the same; fewer
 *   than two observed frames leave them not finite).  The result is bit-identical from run to run: it depends on the
 *   data and the shapes only.
 * RV_ATTR_WORKSPACE: the bytes of ws for (T, k, N) in d->ws_bytes: [ y (T k) | D (T N) | the flags (T bytes) | the block sums
 *   (ceil(T / 256) (1 + k + N)) | the partial tiles (ceil(T / 4096) 3 64 64) ], doubles unless noted, every part on a
 *   256-byte boundary; launches nothing and touches no device.  ws is 256-byte aligned. */
#define RV_ATTR_DESCRIBE 49
#define RV_ATTR_FIT 50
#define RV_ATTR_WORKSPACE 51
/* Switching walk (csrc/switch.hip, rawaudiovae_kelsey_amd/switching.py): one linear-Gaussian law per
 * state of the hidden Markov model of "Latent states", fitted under its posteriors and run block by block like "Latent
 * walk".  The family's conventions: all arithmetic in fp64, no atomics, no polling, every output element written by exactly
 * one thread; no op syncs or reads a device pointer on the host, each may run under capture, and each returns an RV_ERR_*
 * whose message names the field before anything is launched: T, S, k, L, stride, n_rows, mode, ldo, a null q / centre / basis /
 * moment / state / result / info / eigenvalues / row_start / primed / idx / path / live / ws, ws_bytes too small, a block
 * that is not 256-byte aligned.  No new member and no new role of the descriptor.  The codes 38, 39, 42 and 48 stay unassigned.
 * The limits are the HMM's: 1 <= S <= 64, 1 <= k <= 64, k <= L <= 512.
 * The model.  y_t = P (x_t - c) [k] as in "Latent states"; state s emits N(m_s, diag(v_s)), w = 1 / v.  The standardised
 * residual of a frame under its posterior gamma_t is r_t = sum_i gamma_t(i) (y_t - m_i) sqrt(w_i); an UNOBSERVED frame (a value
 * of its x row is not finite) has r_t = +0.  Pair p = frames (p, p + 1), 0 <= p < T - 1; keep[p] = 1 iff both frames lie in
 * one file (RV_PCA_LAGCOV's rule: p + 1 is none of row_start[0 .. n_rows]) and both are observed.  With ' marking frame p + 1
 * the moments of state j are N_j = sum keep gamma'(j), C1_j [k, k] = sum (gamma'(j) r') (keep r)^T, D'_j [k] = sum gamma'(j)
 * keep r'^2 and D_j [k] = sum gamma'(j) keep r^2; A_j[a, b] = C1_j[a, b] / (sqrt(D'_j[a]) sqrt(D_j[b])).  Q_j = I - A_j A_j^T =
 * U diag(q) U^T; where q_min < 0 the guard sets h = 1 / (1 - q_min), g = sqrt(h), A_j <- g A_j and q_i <- max(1 - h (1 - q_i),
 * 0), U unchanged; B_j = U diag(sqrt(q)), so A_j A_j^T + B_j B_j^T = I for every state.
 * RV_SWITCH_RESIDUAL: q = x [T, L] fp32 with a row pitch of stride >= L, centre, basis = P [k, L], moment = theta (the HMM's
 *   block; m and w are read), state = gamma [T, S] fp64, T (1 <= T < 2^31), L, k, S -> result = the residual block, 256-byte
 *   aligned: [ r (T k) fp64 | observed (T) bytes at byte offset 8 T k rounded up to 256 ].  y by csrc/sequence.h's chain;
 *   r[t, j] = ONE chain acc = fma(gamma[t, i], fl(fl(y_j - m_ij) * sqrt(w_ij)), acc) in ascending i from +0; observed[t] = 1
 *   iff the x row is finite.  A workgroup takes 64 frames; one launch over the whole chip.
 * RV_SWITCH_MOMENTS: moment = the residual block, state = gamma [T, S], row_start [n_rows + 1] int64 on the device (the CALLER
 *   checks it on its host copy), n_rows, T (2 <= T < 2^31), S, k, ws, ws_bytes -> result = fp64 [ N (S) | D' (S k) | D (S k) |
 *   C1 (S k k) ].  Four launches.  keep as above.  N_j: the terms keep[p] ? gamma[p + 1, j] : 0 of the pairs in blocks of 256, a
 *   block in ascending p from +0, the blocks in ascending order from +0 (RV_EVAL_DIMS's blocked column sum).  The other three
 *   on the tile of "Latent PCA" under a fourth operand form, `gated` (csrc/moment.h): the T - 1 pairs in ranges of 4096; a
 *   workgroup owns one range and one of its S + 2 tiles, stages 32 pairs at a time in LDS and adds them, four pairs per
 *   v_mfma_f64_16x16x4_f64, in ascending p from +0.  Tile j < S is C1_j: left = fl(gamma[p + 1, j] r[p + 1, a]) (one rounded
 *   product formed while staging), right = keep[p] ? r[p, b] : 0.  Tile S is D': left = gamma[p + 1, i], right = keep[p] ?
 *   fl(r[p + 1, b]^2) : 0.  Tile S + 1 is D: left = gamma[p + 1, i], right = keep[p] ? fl(r[p, b]^2) : 0.  Only the right
 *   operand is gated.  The partial tiles go to ws; the last launch adds every element's partials in ascending range order
 *   from +0.  No division.  The bits depend on the inputs and the shapes only.
 * RV_SWITCH_FIT, 1 <= S <= 64, 1 <= k <= 64:
 *   mode RV_SWITCH_DYNAMICS: moment = the moments block of RV_SWITCH_MOMENTS -> result = fp64 [ A (S k k) | Q (S k k) ] (a block of
 *     its own) and info [S] int32.  A_j[a, b] = fl(fl(C1_j[a, b] / sqrt(D'_j[a])) / sqrt(D_j[b])); 0 where D'_j[a] or D_j[b] is not
 *     positive and finite; the whole A_j = 0 and info[j] = 1 (else 0) where N_j < 2 (or NaN).  Q_j[i, l] for i <= l =
 *     (i == l ? 1 : 0) - chain_m fma(A_j[i, m], A_j[l, m], .) in ascending m from +0, written to [i, l] and [l, i]: bitwise
 *     symmetric, RV_WALK_FIT's rule.  Two launches.  The caller then runs RV_PCA_EIG on every Q_j in place.
 *   mode RV_SWITCH_NOISE: basis = A [S, k, k], moment = the eigenvectors of every Q_j as RV_PCA_EIG leaves them (row i the i-th)
 *     [S, k, k], eigenvalues = q [S, k] -> result = fp64 [ dyn (S 2 k k) | g (S) ], dyn_j = [A_j^T | B_j^T] in RV_WALK_STEP's
 *     layout.  q_min = the least q_i (ties and order do not matter).  q_min < 0: h = 1 / fl(1 - q_min), g = sqrt(h), A^T[b, a] =
 *     fl(g A[a, b]), q_i' = fl(1 - fl(h fl(1 - q_i))); otherwise g = 1, A as it stands, q' = q.  B^T[i, a] = fl(sqrt(max(q_i',
 *     0)) u_i[a]).  One launch.
 * RV_SWITCH_STEP: one block of every stream of *live generated, enqueued without a sync: the step launch, then
 *   rv_stream_process's fc3, fc4 and overlap-add launches (four in all); live as in RV_WALK_STEP, eps_in [n_streams * F, k].
 *   L = live->L, k <= L <= 512; centre [L], basis = R [k, L] (the un-whitening rows), moment = phi fp64 =
 *     [ m (S k) | sd (S k) | pi (S) | A_hmm (S S) | dyn (S 2 k k) ],
 *   state = u [n_streams, k] fp64 (the standardised state), primed [n_streams] int32 and idx = the current state of every
 *   stream [n_streams] int32, all three read and written; next_of = the forced states [n_streams * F] int32 or NULL; weight = fp32
 *   uniforms [n_streams * F] or NULL; path = the states out [n_streams * F] int32; out [n_streams * F, ldo >= L] or NULL.
 *   One workgroup per stream steps the F = block / hop frames in order.  For stream s and absolute frame f:
 *   1. The state.  A forced state in [0, S) is taken as given.  Otherwise (no next_of, -1 or >= S) v = the caller's uniform of
 *      the frame or, without weight, min((float(word) + 0.5f) 2^-32, 0.99999994f) of the FIRST word of Philox(seed) at counter
 *      (lo = f, hi = 2^32 + s); the noise below uses hi = s < 2^31, so the two never collide.  The law is pi when the stream is
 *      not primed (or idx is outside [0, S)), else row idx of A_hmm.  cum_j = the law's plain sums in ascending j from +0;
 *      s' = the first j with (double)v < cum_j, or, if none, the highest j of positive probability (none: 0).
 *   2. The noise.  e_j = (double)temperature[s] * (double)eps as in RV_WALK_STEP: eps_in, or Philox(seed) at index f k + j,
 *      offset s.
 *   3. The standardised state.  Not primed: u = e and the flag is set.  Otherwise u'_i is ONE chain acc = fma(A_s'[i, j], u_j, acc)
 *      over ascending j from +0 continued by fma(B_s'[i, j], e_j, acc) over ascending j.
 *   4. The latent row.  y_j = fma(sd[s', j], u_j, m[s', j]); z_l = (float)(centre_l + (double)offset[s, l] + chain_j fma(y_j,
 *      R[j, l], .)) in ascending j from +0, to the stream workspace's latent row s F + frame and, when out is not NULL, to out.
 *   5. The record.  path[s F + frame] = s'; after the block idx[s] = the last s'.
 *   A stream's bits depend on its own state, controls and draws only, not on n_streams or on the block length.
 * RV_SWITCH_WORKSPACE: the bytes of ws of RV_SWITCH_MOMENTS for (T >= 2, S, k) in d->ws_bytes: [ keep (T - 1) bytes | the block
 *   sums (ceil((T - 1) / 256) S) | the partial tiles (ceil((T - 1) / 4096) (S + 2) 64 64) ], doubles unless noted, every part on
 *   a 256-byte boundary; launches nothing and touches no device.  ws is 256-byte aligned. */
#define RV_SWITCH_RESIDUAL 52
#define RV_SWITCH_MOMENTS 53
#define RV_SWITCH_FIT 54
#define RV_SWITCH_STEP 55
#define RV_SWITCH_WORKSPACE 56
#define RV_SWITCH_DYNAMICS 0
#define RV_SWITCH_NOISE 1
/* ---- Latent transport (csrc/transport.hip; rawaudiovae_kelsey_amd/transport.py) ----
 * Entropic optimal transport between two clouds of whitened latent rows: the Sinkhorn half-step and the barycentric map,
 * fp64 attention that never stores its N x M matrix.  The family's conventions: all arithmetic in fp64, no atomics, no polling,
 * every output element written by exactly one thread; no op syncs or reads a device pointer on the host, each may run under
 * capture, and each returns an RV_ERR_* whose message names the field before anything is launched.  No new member and no new
 * role of the descriptor.  The codes 38, 39, 42, 48 and 57 stay unassigned.  Limits: 1 <= k <= 64, k <= L <= 512, T and N in
 * [1, 2^31).  The slots: fp64 pointers basis, moment, result, centre, state; fp32 pointers a, out (one slot with result: an op
 * uses one of the two), weight; int pointer info; lam = epsilon (fp32, widened once to fp64); the longs T, N, L, k, stride, ldo,
 * ws_bytes; live and ws.
 * Definitions.  For a row a_i and a column b_j [k]: c_ij = max(fma(-2, a_i . b_j, |a_i|^2 + |b_j|^2), 0), the norms chains
 * fma(v, v, .) in ascending d from +0 and the product the sum of v_mfma_f64_16x16x4_f64 in ascending d.  This Gram form carries
 * a rounding of about u (|a|^2 + |b|^2); nothing here pins its bits against a summation order.  s_ij = fma(h_j - c_ij, 1 / eps,
 * lw_j), and -inf where lw_j is -inf: such a column contributes an exact 0.  The N columns are cut into slabs of
 * max(256, ceil(N / 8) rounded up to 64) columns, a rule of N alone.  Within a slab a row takes the columns in tiles of 16: m' =
 * max(m, the tile's maximum), every running sum times exp(m - m') (skipped when m' = m), then w_ij = exp(s_ij - m') added.  A row's
 * slabs are merged in ascending slab order: M = max_s m_s, e_s = exp(m_s - M), Z = sum_s fl(sw_s e_s) from +0.  The running
 * maximum is always subtracted: nothing overflows for a row 10^3 standard deviations out.  No element depends on another row of
 * the call: a row's bits are the same whatever T is and whichever rows stand beside it, and two runs are bit-equal.
 * RV_OT_WHITEN: a = x [T, L] fp32 with a row pitch of stride >= L, basis = [ centre (L) | P (k L) ] -> result = y [T, k] fp64 by
 *   csrc/sequence.h's chain (the bits RV_HMM_EMIT observes with) and info [T] int32, 1 for an observed row; a row of x that holds
 *   a value that is not finite gives y = +0 and info 0.  One launch, a workgroup per 64 frames.
 * RV_OT_SOFTMIN, one Sinkhorn half-step: basis = A [T, k], moment = B [N, k], centre = [ h (N) | lw (N) ] (the other side's
 *   potential and its log-weights), lam = eps > 0, ws, ws_bytes -> result [T] fp64 = -eps (M_i + log Z_i); +inf for a row with no
 *   column of finite weight.  Two launches.  ws holds the slabs' partials [T, n_slabs, 2].
 * RV_OT_MAP, the barycentric map: a = x [T, L] with pitch stride, basis = [ centre (L) | P (k L) | W (L k) ] (W the un-whitening,
 *   columns v_d sqrt(lambda_d)), moment = V [N, k], centre = [ g | lw ], lam = eps, weight = alpha [1] fp32 on the device or NULL
 *   (1), ws, ws_bytes -> out [T, ldo >= L] fp32 and state [T, 3 + k] fp64.  Three launches: y = RV_OT_WHITEN's of x into ws, the
 *   scan, the merge.  T_i = sum_j w_ij V_j / Z_i (the second MFMA, then the slabs in ascending order by fma, then one division);
 *   x'_il = (float)((double)x_il + fl(alpha sum_d W[l, d] (T_id - y_id))), the sum one fma chain in ascending d from +0; where
 *   that product is 0 the output is the input's bits.  Only the kept subspace moves.  state row i = [ f_i, support_i, cbar_i, T_i0 ..
 *   T_i,k-1 ]: f_i as RV_OT_SOFTMIN, support_i = Z^2 / sum w^2 (1: the row was mosaiced; N: it got the target's mean), cbar_i =
 *   sum w c / Z.  A row of x that is not finite passes through unchanged, its state row NaN, 0, NaN, NaN ..; a finite row with no
 *   column of finite weight passes through as well, its state row +inf, 0, NaN, NaN ...  out may be x itself.
 * RV_OT_LIVE, one block of the streaming engine: live = the rv_stream_desc; rv_stream_encode (q = mu * scale + offset),
 *   RV_OT_MAP's launches on the n_streams * F latent rows (L = live->L; weight = alpha [n_streams] on the device, row r takes
 *   alpha[r / F]; state [n_streams * F, 3 + k]), then fc3, fc4 and the overlap-add.  No host sync inside; it may be captured.
 *   ws = [ q (n_streams F L) fp32 | RV_OT_MAP's ws ].  A block's rows equal RV_OT_MAP's of the same latent rows bit for bit.
 * RV_OT_WORKSPACE: the bytes of ws in d->ws_bytes, for (T, N, k) the larger of RV_OT_SOFTMIN's and RV_OT_MAP's ([ y (T k) |
 *   observed (T) int32 | partials (T n_slabs (4 + k)) ], doubles unless noted, every part on a 256-byte boundary); with live set,
 *   RV_OT_LIVE's for (live, N, k).  Launches nothing and touches no device.  ws is 256-byte aligned. */
#define RV_OT_WHITEN 58
#define RV_OT_SOFTMIN 59
#define RV_OT_MAP 60
#define RV_OT_LIVE 61
#define RV_OT_WORKSPACE 62
/* Latent beats (csrc/beat.hip, rawaudiovae_kelsey_amd/beats.py): the pulse of a latent trajectory.
 * The novelty curve of "Latent structure" under a small kernel is an onset-strength curve at the frame rate; these ops
 * condition it, find the period it prefers and place the beats (the dynamic programme of Ellis 2007).  The family's
 * conventions: all arithmetic in fp64, every product rounded before it is added (nothing is contracted into an fma), fixed
 * summation orders, no atomics, no polling, every output element written by exactly one thread; no op syncs or reads a
 * device pointer on the host, each may run under capture, and each returns an RV_ERR_* whose message names the field before
 * anything is launched: T, width, hop, lag, N, ldo, n_out, a null moment / basis / result / centre / path / idx / info /
 * summary / cost / ws, ws_bytes too small, ws not 256-byte aligned.  No new member and no new role of the descriptor.
 * RV_BEAT_ONSET: T >= 1, moment = nov [T] fp64 (what RV_STRUCT_NOVELTY writes), ws / ws_bytes -> result = o [T] fp64,
 *   summary [4] int32, cost [2] fp64.  h[t] = nov[t] where it is finite and > 0, +0 otherwise.  q = sum of fl64(h[t] * h[t]) in
 *   RV_EVAL_DIMS's order: blocks of 256 frames added in ascending t from +0, the block sums added in ascending order from +0.
 *   s = sqrt(q / (double)T), o[t] = h[t] / s when s > 0 and +0 otherwise: one IEEE division, one IEEE square root and one
 *   IEEE division per frame.  summary = {the entries that are finite and > 0, the finite entries, 0, 0}, cost = {s, +0}.
 *   Three launches.  result may not be moment.
 * RV_BEAT_TEMPOGRAM: T >= 1, moment = o [T] fp64, width = Wn, the window in frames, 1 <= Wn <= 8192, hop = Hw >= 1, the frames
 *   between two windows, lag = lo and N = hi, the lags, 1 <= lo <= hi <= 1024, basis = [ win (Wn) | prior (hi - lo + 1) ] fp64
 *   -> result = A [nW, ldo] fp64 with nW = ceil(T / Hw) <= 2^22 and ldo >= hi - lo + 1 (the column of lag tau is tau - lo; the columns
 *   beyond are not written), centre = G [hi - lo + 1] fp64, path = period [nW] int32, info [4] int32, cost [2] fp64.
 *   A[n, tau] = the sum over i in [0, Wn), with a = n Hw + i, of fl64(win[i] * fl64(o[a] * o[a + tau])); a term with
 *   a + tau >= T is skipped, by index.  The sum goes in tiles of 64 values of i: each tile a chain from +0 in ascending i,
 *   the tile sums added in ascending order from +0.  G[tau] = sum_n A[n, tau] in ascending n from +0; score[tau] =
 *   fl64(prior[tau - lo] * G[tau]); P = the tau of the largest score that is finite and > 0, ties to the smaller tau, 0 when
 *   there is none (silence); period[n] by the same rule on fl64(prior[tau - lo] * A[n, tau]).  info = {P, nW, 0, 0},
 *   cost = {score[P], G[P]}, and {+0, +0} when P = 0.  A workgroup takes one window and 256 lags, a thread per lag, and
 *   stages o[n Hw, n Hw + Wn + hi) and win once in LDS ((2 Wn + hi) doubles, at most 136 KiB); then a workgroup per window
 *   picks its period and one workgroup adds G and picks P.  Three launches; the bits depend on the operands only, not on the
 *   launch.
 * RV_BEAT_TRACK: T >= 1, moment = o [T] fp64, lag = dlo and width = dhi, the nearest and the furthest predecessor in frames,
 *   1 <= dlo <= dhi <= 2048, N = P, the end window, 1 <= P <= 2048, basis = pen [dhi - dlo + 1] fp64, the transition scores
 *   (pen[delta - dlo] for a step of delta frames) -> result = C [T] fp64, idx = back [T] int32, path = beats [n_out] int32
 *   with n_out >= (T - 1) / dlo + 1, summary [4] int32, cost [2] fp64.  h[t] = o[t] where it is finite, +0 otherwise.  The
 *   candidates of frame t are p = t - delta, delta in [dlo, dhi], p >= 0, with v = fl64(C[p] + pen[delta - dlo]); a NaN is
 *   skipped; best = the largest v > -inf, ties to the nearer p.  With no such v, C[t] = h[t] and back[t] = -1; otherwise
 *   C[t] = fl64(h[t] + best) and back[t] = p.  t* = the frame of the largest C over [max(0, T - P), T), ties to the earlier
 *   frame.  beats = t* followed back to -1, written in ascending order, n of them; the rest of path is -1.  summary =
 *   {n, t*, 0, 0}, cost = {C[t*], the sum of h at the beats in ascending order from +0}.  Every entry of every output is
 *   written.  ONE workgroup, one launch: the frames [b dlo, (b + 1) dlo) read only C[p] with p < b dlo, so a block of dlo
 *   frames is taken at once, every frame's window spread over the lanes that are left (a power of two, at most a wave); the
 *   last dhi + dlo values of C live in LDS.  The maximum and the single rounded add make the bits independent of how the
 *   window is split.
 * RV_BEAT_WORKSPACE: the bytes of ws of RV_BEAT_ONSET for T in d->ws_bytes; launches nothing and touches no device.
 *   ws is 256-byte aligned. */
#define RV_BEAT_ONSET 63
#define RV_BEAT_TEMPOGRAM 64
#define RV_BEAT_TRACK 65
#define RV_BEAT_WORKSPACE 66
struct rv_stream_desc;
typedef struct rv_mosaic_desc {
  /* A slot that ops read under more than one name is an anonymous union of its roles: same address, the type of the
   * role.  Set the member the op's documentation names. */
  long T, k;                     /* query / output rows, neighbours per row (KNN, GATHER_MEAN) */
  union { int* idx;              /* [T, k]: KNN output, GATHER_MEAN input */
          int* warp_table; };    /* ALIGN_WARP [n, 2] */
  union { const float* q;        /* KNN */
          const float* mu;       /* EVAL ops [T, L] */
          const float* a; };     /* ALIGN_COST [Ta, L] */
  union { const float* c;
          const float* logvar;   /* EVAL ops [T, L] */
          const float* b;        /* ALIGN_COST [Tb, L] */
          const float* shifts; };  /* PCA_APPLY (EDIT) [k] */
  long N, L, splits;
  union { float* dist;
          float* local_costs;    /* ALIGN ops: Dm [Ta, W] */
          double* basis; };      /* PCA and walk ops: the fp64 matrix the op names */
  void* ws;
  long ws_bytes;
  union { const float* src;      /* GATHER_MEAN */
          const double* moment; };  /* WALK_FIT, WALK_STEP: the fp64 input matrix the op names; HMM ops: theta; ATTR_FIT: the targets D */
  long src_len;
  const long long* row_start;
  long stride, n_rows;
  union { long width;
          long fit_radius;       /* GRAIN_FIT, LIVE ops: R */
          long band; };          /* ALIGN ops: r */
  union { float* out;            /* GATHER_MEAN [T, ldo], OLA [n_out] */
          double* result;        /* WALK_FIT; HMM ops: logb [T, S], HMM_MSTEP: the new theta; ATTR ops: desc [T, ldo] / the fit */
          double* end_costs; };  /* ALIGN_FORWARD (SUBSEQUENCE) [Tb], or NULL */
  long ldo;
  const float* frames;           /* OLA */
  long F, S, hop;                /* S: the frame length; HMM ops: the states */
  const float* window;
  long n_out;
  union { const int* next_of;    /* TRANSITION [N]; LIVE with a fit: [3 N], successors then room */
          const int* room; };    /* GRAIN_FIT [n_rows, 2] */
  long row0;                     /* TRANSITION, PATH_FORWARD: rows [row0, row0 + rows) of T; RECUR_PROFILE: the slab's first row */
  union { long rows;
          long lag; };           /* LIVE ops: D; RECUR_PROFILE: lo (width: hi) */
  union { float* trans;          /* [rows, k, k]: TRANSITION output, PATH_FORWARD input */
          float* gain;           /* GRAIN ops, LIVE with a fit */
          double* centre; };     /* PCA and walk ops [L] */
  union { float lam;             /* PATH_FORWARD: lambda, the weight of the transition costs */
          float gain_max;        /* GRAIN_FIT, LIVE ops */
          float dynamic_range;   /* EVAL_FRAMES: R in dB */
          float penalty; };      /* ALIGN_FORWARD: p */
  union { int* slot;             /* PATH_BACKTRACK [T] */
          int* shift;            /* GRAIN ops, LIVE with a fit */
          int* path; };          /* ALIGN_BACKTRACK, ALIGN_WARP [Ta + Tb - 1, 2] */
  union { int* choice;           /* PATH_BACKTRACK [T]; LIVE with weight */
          int* info;             /* PCA_EIG [2] */
          int* primed;           /* WALK_STEP [n_streams] */
          int* summary; };       /* ALIGN_BACKTRACK, ALIGN_WARP [4] */
  union { double* cost;          /* PATH_BACKTRACK [2]; EVAL_DIMS [L] */
          double* score;         /* GRAIN_FIT, LIVE with a fit */
          double* eigenvalues;   /* PCA ops, WALK_FIT */
          double* state;         /* WALK_STEP [n_streams, k]; HMM ops: the posteriors [gamma | xi | ll] */
          double* path_costs; }; /* ALIGN_BACKTRACK [2] */
  const struct rv_stream_desc* live; /* LIVE ops: weights, block I/O, scale / offset, window, norm, stream workspace */
  long mode;                     /* LIVE: RV_LIVE_GRAINS / RV_LIVE_DECODE; ALIGN_FORWARD: the DP's mode; ALIGN_WARP: the timeline */
  union { const float* weight;   /* LIVE [n_streams] on the device, or NULL: the mean of the k candidates */
          const float* gains;    /* PCA_APPLY (EDIT) [k] */
          const float* twiddles; };  /* EVAL_FRAMES, ATTR_DESCRIBE [S] */
  long which;                    /* LIVE_RESET: the stream, -1 for all */
} rv_mosaic_desc;
int rv_mosaic(int op, rv_mosaic_desc* d, void* stream);

/* ---- Streaming resynthesis (csrc/stream.hip) ----
 * rv_small_linear_f32: y = act(x W^T + b) for few rows, one lane per output column: acc = +0, then
 * acc = fmaf(x[k], W[n,k], acc) in ascending k, + b, then fmaxf / tanhf (act 0 none, 1 relu, 2 tanh) -- the arithmetic of
 * rv_linear_fp32, and a row's value does not depend on M.  x [M, K] with row stride ldx (rows may overlap), W [N, K]
 * with row stride ldw >= K, b [N] or NULL, y [M, N] with row stride ldy >= N. */
int rv_small_linear_f32(const float* x, long ldx, const float* w, long ldw, const float* bias, long M, long N, long K,
                        int act, float* y, long ldy, void* stream);

/* One call of the streaming engine: n_streams streams, `block` new samples each, frames of S samples every `hop`
 * (P = S - hop samples of history), F = block / hop frames decoded per stream.  Weights are the model's fp32 tensors
 * in place ([out, in], contiguous).  Rows of mu / logvar / eps are stream-major: row s * F + j.  The controls give
 * mu' = mu * scale + offset and z = mu' + (temperature * eps) * exp(logvar / 2); eps is eps_in [n_streams * F, L] or,
 * when eps_in is NULL, Philox(seed) keyed by (stream, absolute frame, latent index).  window [S] (ones for a
 * rectangular window) and norm [P + hop] (the window sums of output position t, t < P, and of P + t % hop beyond) are
 * the caller's.  State (history, overlap-add tail, frame counters) lives in the workspace of
 * rv_stream_workspace_bytes, zeroed before the first call. */
typedef struct rv_stream_desc {
  long S, H, L, n_streams, block, hop;
  const float *w1, *b1, *w21, *b21, *w22, *b22, *w3, *b3, *w4, *b4;
  const float* x;      /* [n_streams, ld_x]: the block of every stream             */
  long ld_x;
  float* y;            /* [n_streams, ld_y]: the block of output of every stream   */
  long ld_y;
  float *mu, *logvar;  /* [n_streams * F, L]                                       */
  const float* eps_in; /* [n_streams * F, L] or NULL                               */
  unsigned long long seed;
  const float *scale, *offset; /* [n_streams, L]                                   */
  const float* temperature;    /* [n_streams]                                      */
  const float *window, *norm;
  void* workspace;
} rv_stream_desc;
long rv_stream_workspace_bytes(long S, long H, long L, long n_streams, long block, long hop);
int rv_stream_process(const rv_stream_desc* d, void* stream);
/* Zero the state of stream `which` (-1: every stream) of the workspace laid out for d's extents. */
int rv_stream_reset(const rv_stream_desc* d, long which, void* stream);

/* Standard normal draws (replaces torch.randn_like, model.py:25).
 *
 * THE RANDOM NUMBERS OF THIS LIBRARY, in one place (csrc/philox.h; tests/rng_oracle.py is the same contract in numpy and
 * tests/test_rng_gpu.py holds every consumer to it bit for bit):
 *   words    = Philox4x32-10(key, counter), key = (seed & m, seed >> 32), counter = (lo & m, lo >> 32, hi & m, hi >> 32)
 *              for a 64-bit pair (lo, hi), m = 2^32 - 1
 *   uniforms = min((float(word) + 0.5f) * 2^-32, 0.99999994f) in fp32, one per word: u_x, u_y, u_z, u_w in [2^-33, 1 - 2^-24]
 *   normals  = lane 0: r0 cos a0, lane 1: r0 sin a0, lane 2: r1 cos a1, lane 3: r1 sin a1 with r0 = sqrt(-2 ln u_x),
 *              a0 = 2 pi u_y, r1 = sqrt(-2 ln u_z), a1 = 2 pi u_w (Box-Muller; radii from 3.45e-4 to 6.8)
 * Two forms of the last step draw the same values from the same words: the accurate one (logf, sincospif; within 7.1e-7 of
 * the float64 value as measured) and the fast one of the training step (hardware log / sin / cos; within 1.8e-6).  A value depends on
 * (seed, lo, hi, lane) alone -- never on the launch shape, the kernel form or the batch beside it.  Who uses which counter:
 *   accurate form, element i of a flat tensor = lane i & 3 of counter (lo = i >> 2, hi = offset):
 *     rv_randn(n, seed, offset)          i in [0, n)
 *     rv_reparameterize(seed, offset)    i in [0, n): eps_out is rv_randn's output
 *     rv_latent_mix(seed, offset)        i = (row0 + r) * L + l for row r of the call
 *     rv_stream_process (seed)           i = f * L + l, offset = the stream's number s, f the stream's absolute frame number
 *                                        (counted from its last reset): stream s draws rv_randn(seed, s) laid out [frame][L]
 *     RV_WALK_STEP (seed)                i = f * k + j, offset = s likewise
 *   fast form, element (b, l) of the [B, L] eps grid = lane l & 3 of counter (lo = b * (Lp / 4) + l / 4, hi = *step_counter;
 *   0 when step_counter is NULL), Lp the padded latent width:
 *     rv_reparam_fwd, rv_heads_reparam_fwd, rv_latent_fwd in each of its forms, and through them rv_plan_step: the cast at
 *     the head of a step increments *step_counter first, so step t of a run (1-based) draws with hi = t, eagerly and in
 *     every replay of a captured step. */
int rv_randn(float* out, long n, unsigned long long seed, unsigned long long offset,
             void* stream);

/* One parameter tensor as seen by the fused optimizer / gradient finaliser. */
typedef struct rv_param_desc {
  long offset;             /* element offset of the tensor in the flat fp32 arenas   */
  long rows, cols;         /* exact shape ([out,in]; bias: rows=1)                   */
  const float* grad_slabs; /* partial-gradient slabs: element (r,c) of slab s is at  */
  long grad_ld;            /*   grad_slabs[s*grad_split_stride + r*grad_ld + c]      */
  long grad_split_stride;
  int grad_splits;
  void* shadow_bf16;       /* padded bf16 copy refreshed with the new weight (or NULL) */
  float* shadow_f32;       /* padded fp32 copy (biases as read by GEMM epilogues), or NULL */
  long shadow_ld;
  void* shadow_fp8;        /* padded fp8 (e4m3) copy fp8(w * *fp8_scale), leading dim shadow_ld, or NULL */
  const float* fp8_scale;  /* device scalar */
  int grad_half;           /* non-zero: grad_slabs holds fp16 values fp16(partial * 2^e) (same element strides), e per */
  const float* grad_unscale; /* 32 x 32 granule and slab: element (r,c) of slab s is scaled back by                 */
  long us_ld;              /*   grad_unscale[s*us_split_stride + (r/32)*us_ld + c/32]                               */
  long us_split_stride;    /* (the table a weight-gradient GEMM writes with RV_SLAB_F16)                            */
} rv_param_desc;

/* torch.optim.Adam(lr) step (train.py:163,193: betas 0.9/0.999, eps 1e-8, no weight
 * decay, no amsgrad) over the flat arenas in one launch: sums the gradient slabs,
 * updates exp_avg / exp_avg_sq / param, rewrites the bf16 shadow, and (optional)
 * stores the summed gradient to grad_out (flat, exact) for inspection.
 * t = *step_counter (1-based).  grad_scale multiplies the summed gradient first
 * (1/world_size after an all-reduce SUM).  `descs` is HOST memory (copied per call).
 * grad_bf16 != NULL: the gradient is taken from that flat bf16 arena (same element offsets as the fp32 arenas; a bf16
 * all-reduce's result) instead of the descriptors' slabs; grad_out must then be NULL.  The descriptors may be the ones the
 * slabs were summed with (fp16 slabs included): only offset, shape and shadows are used, and every element is updated. */
int rv_adam_multi(const rv_param_desc* descs, int n_desc, float* param, float* exp_avg,
                  float* exp_avg_sq, float* grad_out, const void* grad_bf16, float lr, float grad_scale,
                  const long long* step_counter, void* stream);

/* Sum gradient slabs into the flat exact-shape gradient arena only (no update):
 * what loss.backward() leaves in .grad; also the all-reduce payload builder.  out_bf16 != 0: grad_out is a flat
 * bf16 arena (same element offsets) and receives the fp32 sum rounded to bf16 -- half the all-reduce bytes. */
int rv_grad_finalize(const rv_param_desc* descs, int n_desc, void* grad_out, int out_bf16, void* stream);
/* dW = dY^T X on 256x256 tiles (as rv_linear_wgrad with RV_TILE_256x256) in a launch that ALSO runs the
 * fused Adam update (rv_adam_multi) of the `n_desc` tensors in `descs` -- tensors whose gradients earlier
 * launches completed, never the one this GEMM produces -- on `n_adam_blocks` extra 512-thread blocks that take
 * the CUs the GEMM's tiles * splits blocks leave idle (extents must tile by 256 x 256 x 64). */
int rv_linear_wgrad_adam(const void* dy_bf16, long lddy, const void* x_bf16, long ldx, long Mp, long Np, long Kp,
                         int splits, void* dw_slabs, long lddw, int slab_dtype, float* slab_unscale,
                         const rv_param_desc* descs, int n_desc,
                         float* param, float* exp_avg, float* exp_avg_sq, float lr, float grad_scale,
                         const long long* step_counter, int n_adam_blocks, void* stream);

/* Parameters (unless `param` is NULL: shadows only; `flat` may then be the parameter arena itself, which is how
 * rv_plan_refresh_shadows rebuilds all shadows in one launch) AND every operand shadow of the `descs` tensors from a flat
 * fp32 source: arena element o is flat[o - flat_base]. */
int rv_params_from_flat(const rv_param_desc* descs, int n_desc, const float* flat, long flat_base, float* param,
                        void* stream);

/* ---- fp8 (e4m3, OCP) operand path for the two large forward GEMMs (BASELINE configs[4]; a build extension,
 * the reference has no reduced-precision path).  Operands are quantised per tensor:
 * q = fp8(value * scale), the GEMM accumulates in fp32 on v_mfma_scale_f32_16x16x128_f8f6f4 (unit block
 * scales) and multiplies the accumulator by *dq = 1 / (scale_A * scale_B) before bias / activation.
 * K extents and leading dims are in fp8 elements (multiples of 128 / 16). ---- */
/* fp32 [rows, cols] -> zero-padded fp8 [rows_p, cols_p]: fp8(src * *scale), saturating at +-448. */
int rv_cast_pad_fp8(const float* src, long rows, long cols, long ld_src, void* dst_fp8, long rows_p, long cols_p,
                    long ld_dst, const float* scale, void* stream);
/* rv_linear_fwd whose operand rows are read where the audio lives (AudioDataset.__getitem__,
 * rawvae/dataset.py:108-118): row r < B is the frame audio_bf16[f*hop : f*hop + Kp], f = frame_index ? frame_index[r]
 * : first_frame + r, of the waveform kept in HBM as bf16 (cast once when it was uploaded; rounding to bf16 is what
 * rv_cast_pad_bf16 does per batch, so the operand is bit-identical); rows B..Mp repeat row B - 1 (padding).  The A
 * tile loader stages each frame's 16-byte pieces straight from the waveform -- no cast / gather kernel, no fp32
 * read.  hop % 8 == 0, 16-byte aligned waveform, and the buffer must extend Kp elements past the last frame's start.
 * frames_bf16 (or NULL) receives the framed [Mp][ld_frames] bf16 matrix as a by-product (the weight gradient's
 * operand): the block with tile_n == kt % tiles_n copies K tile kt of its rows out of LDS.  step_counter (or NULL)
 * is incremented by block 0 (the step's first kernel does that). */
int rv_linear_fwd_frames(const void* audio_bf16, const long long* frame_index, long first_frame, long hop, long B,
                         const void* w_bf16, long ldw, const float* bias, long Mp, long Np, long Kp, int act,
                         void* y_bf16, long ldy, void* frames_bf16, long ld_frames, long long* step_counter,
                         void* stream);
/* ---- whole-step plan: one call enqueues forward, loss, backward (and Adam) ---- */
typedef struct rv_plan rv_plan;

typedef struct rv_plan_buffers {
  /* flat fp32 arenas, PARAM order fc1.w fc1.b fc21.w fc21.b fc22.w fc22.b fc3.w fc3.b fc4.w fc4.b */
  float* param; float* exp_avg; float* exp_avg_sq; float* grad; /* grad may be NULL */
  void* workspace;             /* rv_plan_workspace_bytes() bytes, zero-initialised   */
  long long* step_counter;     /* device int64, number of steps started               */
  float* loss_ring;            /* [ring][4] fp32: total, mse, kld, unused             */
  int ring;
} rv_plan_buffers;

#define RV_PHASE_FWD 1      /* cast, fc1, heads, reparam, fc3, fc4+loss              */
#define RV_PHASE_BWD_A 2    /* fc4 backward (paired dgrad+wgrad), dz, reparam bwd, fc3 wgrad */
#define RV_PHASE_BWD_B 4    /* heads dgrad/wgrad, fc1 wgrad                           */
#define RV_PHASE_FINALIZE_A 8  /* fc3,fc4 slabs -> flat fp32 grad arena                */
#define RV_PHASE_FINALIZE_B 32 /* fc1,fc21,fc22 slabs -> flat grad arena               */
#define RV_PHASE_ADAM 16       /* optimizer + bf16 shadow refresh (all ten tensors)    */
#define RV_PHASE_ADAM_A 64     /* ... only fc3, fc4                                    */
#define RV_PHASE_ADAM_B 128    /* ... only fc1, fc21, fc22                             */
/* finer split, in gradient-availability order (data-parallel buckets: fc4 | fc1 | the rest):  */
#define RV_PHASE_BWD_FC4 0x0100   /* fc4 backward: fc4.w, fc4.b, fc3.b gradients ready         */
#define RV_PHASE_BWD_CHAIN 0x0200 /* dz, reparam bwd, heads dgrad+wgrad, fc1 wgrad: fc1.*, heads  */
#define RV_PHASE_BWD_REST 0x0400  /* fc3 wgrad                                                 */
#define RV_PHASE_FIN_FC4 0x0800
#define RV_PHASE_FIN_FC1 0x1000
#define RV_PHASE_FIN_MID 0x2000   /* fc21, fc22, fc3                                           */
#define RV_PHASE_ADAM_FC4 0x4000
#define RV_PHASE_ADAM_FC1 0x8000
#define RV_PHASE_ADAM_MID 0x10000
#define RV_PHASE_ALL_LOCAL (1 | 2 | 4 | 16)

int rv_plan_create(rv_plan** out, long B, long S, long H, long L);
void rv_plan_destroy(rv_plan*);
long rv_plan_workspace_bytes(const rv_plan*);
int rv_plan_bind(rv_plan*, const rv_plan_buffers*);
/* Plan options (the plan must be bound):
 *   RV_OPT_LATENT_FUSED  1 (default): heads GEMM, reparameterisation and fc3 of the forward are ONE launch
 *     (rv_latent_fwd; with the fp8 forward it also emits fc4's fp8 operand) when the padded latent width is 64 and
 *     the padded hidden width a multiple of 512 up to 2048, and dz + the reparameterisation backward likewise (rv_latent_bwd); 0, or any
 *     other shape: three launches (rv_heads_reparam_fwd + fc3) and dz as split-K slabs + rv_reparam_bwd.  The same
 *     switch selects the heads' backward: rv_heads_bwd (one pass over h1; needs a padded batch that is a multiple of
 *     512) or the generic rv_linear_dgrad_wgrad; the partial counts of fc21 / fc22 weights and of fc1's bias in
 *     rv_plan_descs follow the form in use.
 *   RV_OPT_FP8  the fp8 (e4m3) weight path.  2: fp8 forward for fc1 and fc4 (weights AND their input activations in e4m3;
 *     backward, heads, fc3 stay bf16).  1: that forward AND fc4's backward -- dgrad and wgrad in one 256 x 256 launch -- on
 *     fp8 operands: the fc4 forward's epilogue writes dP4 as fp8(dP4 * [12]) instead of bf16 (|dP4| <= 2 * 2 / (B S) by
 *     construction, so the scale is fixed), the dgrad multiplies it with the fp8 weight shadow (read MN-major through
 *     ds_read_b64_tr_b8), the wgrad with the fp8 image of h3 the fc3 forward wrote; K tiles are 128 deep, half the LDS
 *     fill per flop of the bf16 pair.  Where the extents do not tile (256 x 256 tiles, an even number of 128-deep K
 *     tiles per block) and for gradients from outside (rv_plan_set_external_grads) the backward stays bf16.  In the full
 *     local step (all phases in one call) and in rv_plan_step_ddp's all-reduce schedule fc1's weight gradient -- the
 *     launch that also carries rider blocks -- runs on fp8 operands as well, under the same tiling conditions: the heads' backward writes dP1 as fp8(dP1 * [13])
 *     only, the GEMM multiplies it with the fp8 image of the frames fc1's forward read (both MN-major), and neither
 *     bf16 copy is written; [13] follows the maximum of |dP1| measured in the previous step, like h3's scale.
 *     The workspace buffer "fp8_state" holds 16 floats (then 2 x 1024 slots) the caller initialises before rv_plan_refresh_shadows:
 *       [0] scale of x   [1] scale of W1   [2] scale of W4   [3] scale of h3 (this step)
 *       [4] max|h3| of the previous step (reduced from the fc3 forward's per-block maxima, workspace buffer
 *           "h3_amax"; this step's h3 scale is 224 / it: delayed scaling)
 *       [5] 1/([0][1])   [6] 1/([3][2])   (both rewritten at the start of every step)
 *       [7] non-zero: keep [3], [13] and the weight scales fixed (parity runs)
 *       [10] 1/([12][2])   [11] 1/([12][3])   (fc4's fp8 backward: dgrad / wgrad dequantisation, rewritten every step)
 *       [12] scale of dP4's fp8 image: 112 / (2 / (B S)), set by the caller
 *       [13] scale of dP1's fp8 image (this step; the caller's first guess, then 224 / [14])   [14] max|dP1| of the
 *           previous step (reduced from the per-wave maxima rv_heads_bwd left behind h3's in "h3_amax")
 *       [15] 1/([13][0])   (fc1's fp8 weight gradient: dequantisation, rewritten every step)
 *       [8] max|W1|, [9] max|W4| as the last optimizer update left them in the fp8 shadows (0 = none yet; reduced by
 *           the step's first kernel from [32 ..]: 2 x 1024 slots that a small kernel behind the optimizer fills with
 *           max|q| / scale over slices of the two shadows, and that the first kernel resets); [16..31] reserved.  The
 *           caller zero-initialises the whole buffer.
 *     Weight scales start as the caller's (224 / max|W| at refresh).  Adam rewrites the fp8 shadows with the current
 *     scale; the first kernel of the next step, AFTER latching [5] / [6] from the scales the shadows were written
 *     with, moves [1] / [2] to 224 / the measured maximum for the coming update (delayed scaling: a weight that grows
 *     never meets a scale older than one step; one that has saturated reads as 448 / scale, so the scale halves until
 *     it fits).
 *   RV_OPT_SLAB_DTYPE  element type of the split-K slabs of the two large weight gradients (fc1.weight, fc4.weight;
 *     2 x 33.5 MB of fp32 slabs per step at C2): RV_SLAB_F16 (default: block-floating-point fp16, see above), which
 *     halves what the two weight-gradient GEMMs write and Adam reads back, or RV_SLAB_F32.  Each partial is an fp32
 *     sum over a quarter of the batch; rounding it to fp16 adds ~3e-4 relative noise to those two gradients whatever
 *     their magnitude (the sum over slabs stays fp32).  Where the plan runs the streaming heads' backward (rv_heads_bwd's
 *     form: padded latent width 64, padded batch a multiple of 512) the row-group partials of fc21.weight / fc22.weight
 *     follow the same switch (8.4 MB of fp32 slabs per step at C2); rv_plan_descs reports the form in use.
 *   RV_OPT_ROCTX  1: roctx ranges (rocprofv3 --marker-trace) around the host calls that enqueue the step's phases --
 *     "rv:fwd", "rv:fc4-bwd", "rv:rest-bwd", "rv:adam" (local step) / "rv:rest-bwd+exchange+adam" (data-parallel step) --
 *     so that a kernel timeline reads as phases (tracing).  The marker library is loaded at run time
 *     (librocprofiler-sdk-roctx.so, else libroctx64.so); RV_ERR_UNSUPPORTED when neither can be.  Default 0.
 *   RV_OPT_DDP_SIGNAL  how the compute stream and the collective stream of rv_plan_step_ddp (all-reduce schedule) hand
 *     work to each other: 1 (default) device-side sequence flags in the workspace buffer "ddp_flags" -- a one-wave kernel
 *     behind the producer publishes the step's number, a one-wave kernel in front of the consumer waits for it (~1.8 us
 *     per crossing; deadlock-free for any stream -> hardware-queue mapping because every waiter is enqueued after its
 *     setter; every wait is bounded -- 5 s where the setter follows this device's own kernels, RV_OPT_DDP_WAIT_MS where
 *     it follows a collective -- and timeouts are counted in ddp_flags[8], which must stay 0) -- or 0: HIP events (~9 us
 *     per crossing).  Steps enqueued under stream capture always use events (a graph needs the edges).
 *   RV_OPT_DDP_WAIT_MS  bound, in milliseconds, of a flag wait whose setter sits behind a collective, i.e. behind the
 *     slowest peer rank (default 30000 = thirty seconds: a spinning wave cannot be cancelled from the host, so the bound
 *     is what a dead peer costs; ranks reach a step seconds apart around a checkpoint or an evaluation pass as a matter
 *     of course -- a caller whose ranks drift further apart than that raises it, or synchronises the ranks first).  A
 *     wait that runs out is counted in ddp_flags[8] and POISONS the plan on the device: the optimizer launches of
 *     rv_plan_step_ddp read the count and apply no update while it is non-zero, so a partial all-reduce never reaches
 *     the parameters; the host side must read the count (it is never cleared on the device), agree on it across ranks
 *     and stop every rank.
 *   RV_OPT_DDP_DEFER_TAIL  1: rv_plan_step_ddp (all-reduce schedule, device-side flags, bf16 operands) returns with its
 *     LAST wait -- second exchange done -- and the update of that bucket (fc1, heads, fc3) not yet enqueued; the next
 *     rv_plan_step_ddp call enqueues its own cast launch first (it needs no parameter, and the compute stream has nothing
 *     else to do while the exchange is on the links), then that wait and update, then its forward.  Anything else that
 *     follows a step -- reading parameters or optimizer state, a checkpoint, an evaluation pass, the end of training --
 *     needs rv_plan_ddp_flush(plan, stream) first (rv_plan_step and rv_plan_step_frames do it themselves).  The deferred
 *     update takes its step number from a copy latched inside the step, so results are bit-identical to 0 (default).
 *   RV_OPT_DDP_W1_WIDE  1: in rv_plan_step_ddp's all-reduce schedule fc1's weight gradient -- the last GEMM of the
 *     backward, which has no optimizer riders there -- runs with twice the K splits of the local step, i.e. on all 256
 *     CUs instead of 128 (where the extents allow).  0 (default): the local step's split count on 128 CUs, whose rider
 *     blocks sum the slabs of the second bucket's other tensors into the payload meanwhile.  Which is faster depends on
 *     what the collective that runs beside this launch does to the CUs it occupies: with workgroups that leave room
 *     for a 256 x 256 GEMM block beside them the wide form wins (modelled: 241 against 247 us per step at 8 ranks), with
 *     workgroups that take their CUs whole it runs in two rounds and loses (263 against 250) -- the default is the
 *     form whose time does not depend on it.  (With 0 and the fp32 payload a one-rank step reproduces rv_plan_step bit
 *     for bit; the sums over 4 and over 8 partial slabs round differently.) */
enum { RV_OPT_LATENT_FUSED = 0, RV_OPT_FP8 = 1, RV_OPT_SLAB_DTYPE = 2, RV_OPT_ROCTX = 3, RV_OPT_DDP_SIGNAL = 4, RV_OPT_DDP_W1_WIDE = 5,
       RV_OPT_DDP_WAIT_MS = 6, /* 7, 8: retired in round 6 (the paired latent forward and fc3 inside the fc4 forward, both
       measured slower in the step: DESIGN.md section 6, profiles/r05_latent_pair_ab.txt, r05_fc3_in_fc4.txt) */
       RV_OPT_DDP_DEFER_TAIL = 9 };
int rv_plan_set_option(rv_plan*, int option, int value);
/* Enqueue what a data-parallel step left to "the next call" (RV_OPT_DDP_DEFER_TAIL): the wait for the second exchange
 * and the update behind it -- always on the stream that step was enqueued on (`stream`: that stream, or NULL; anything
 * else is RV_ERR_STATE, as is a following rv_plan_step_ddp on another stream).  No-op when nothing is pending. */
int rv_plan_ddp_flush(rv_plan*, void* stream);
/* Gradients from outside for the following BWD / FINALIZE phases (the autograd boundary of rawvae.model.VAE.forward:
 * any loss, not only loss_function).  d_recon [B,S] with recon [B,S] (the forward's output, for tanh'), dmu and
 * dlogvar [B,L], all exact-shape fp32, each NULL = zero; the reparameterisation backward then takes kl_beta from
 * the rv_plan_step call (pass 0 when dmu / dlogvar already hold the KL gradient).  grad_out (or NULL = the bound
 * grad arena) receives the FINALIZE phases' flat fp32 gradients.  All NULL restores the fused loss of the forward
 * phase.  A full local step (BWD_A | BWD_B | ADAM without FINALIZE) with them set is RV_ERR_STATE. */
int rv_plan_set_external_grads(rv_plan*, const float* d_recon, const float* recon, const float* dmu,
                               const float* dlogvar, float* grad_out);
/* The plan's OWN loss across the autograd boundary (loss_function of rawvae/model.py:38-47 called on the untouched
 * outputs of the fused forward: the drop-in loop of train.py:184-193).  rv_plan_loss: (total, mse, kld) of the forward
 * phase that ran last into out3[3] (device), one small launch, the value -- and summation order -- the backward later
 * writes to the loss ring.  rv_plan_set_loss_grad: the following BWD / FINALIZE phases use the forward's fused loss
 * gradient (nothing from outside) and leave (*d_loss_dev) x gradient in grad_out (flat fp32 [n_params]; NULL = the
 * bound grad arena); d_loss_dev is the upstream gradient of the scalar loss, a DEVICE pointer read at finalize time (the
 * host never synchronises on it).  d_loss_dev = NULL and grad_out = NULL switch it off.  RV_ERR_STATE while gradients
 * from outside are set. */
int rv_plan_loss(rv_plan*, float kl_beta, float* out3, void* stream);
int rv_plan_set_loss_grad(rv_plan*, const float* d_loss_dev, float* grad_out);
/* The plan's ten parameter descriptors (PARAM order): gradient slabs of its own workspace (from_flat = 0) or the
 * bound flat gradient arena (1), and the operand shadows Adam must refresh.  For callers that drive
 * rv_adam_multi / rv_params_from_flat themselves. */
int rv_plan_descs(const rv_plan*, rv_param_desc* out10, int from_flat);
/* How the full local step divides the optimizer (train.py:193) between its last two launches: tensors [*first, *last) of
 * the descriptor table are updated by rider blocks beside fc1's weight gradient (rv_linear_wgrad_adam), all others by the
 * step's last launch (rv_adam_multi).  [2, 10) at a latent width of 64 (only fc1 is left for the last launch); [2, 8) --
 * the heads and fc3 -- at the reference's own latent_dim = 256 (default.ini:18), where everything but fc1 would make the
 * riders twice as long as the GEMM beside them.  RV_ERR_STATE for an unbound plan. */
int rv_plan_riders(const rv_plan*, int* first, int* last);
/* Rebuild every bf16 weight shadow from the fp32 param arena (after init / load). */
int rv_plan_refresh_shadows(rv_plan*, void* stream);
/* Enqueue the selected phases of one training step (train.py:184-193) on `stream`.
 * x: exact [B,S] fp32 frames.  eps: explicit [B,L] or NULL (on-device RNG, `seed`).
 * recon_out: optional exact [B,S].  adam_from_flat != 0 makes the Adam phase read the
 * flat grad arena (e.g. after an all-reduce), scaled by grad_scale, instead of the slabs. */
int rv_plan_step(rv_plan*, int phases, const float* x, const float* eps, float* recon_out,
                 float kl_beta, float lr, float grad_scale, int adam_from_flat,
                 unsigned long long seed, void* stream);
/* rv_plan_step whose batch is B hop-strided frames of a waveform resident in HBM (AudioDataset semantics,
 * rawvae/dataset.py:99-121; frame i = audio[f*hop : f*hop + S], f = frame_index ? frame_index[i] : first_frame + i,
 * samples past n_samples read as 0).  With audio_bf16 (the same waveform as bf16, n_samples + Sp + 8 elements, zero
 * past n_samples; hop % 8 == 0) the step launches NO cast or gather kernel: fc1's A-tile loader reads frame f at
 * f*hop of the bf16 waveform (rv_linear_fwd_frames) and fc4's loss epilogue reads its fp32 target at f*hop of `audio`
 * (rv_decode_out_loss_fwd_frames).  audio_bf16 == NULL (or an unaligned hop, a frame length that is not a multiple of
 * 128 -- the padded columns must be zeros, not the samples behind the frame -- or the fp8 forward) falls back to one
 * cast kernel per step (rv_gather_cast_frames). */
int rv_plan_step_frames(rv_plan*, int phases, const float* audio, const void* audio_bf16, long n_samples,
                        const long long* frame_index, long first_frame, long hop, const float* eps, float* recon_out,
                        float kl_beta, float lr, float grad_scale, int adam_from_flat, unsigned long long seed,
                        void* stream);
/* ---- data-parallel step with the collective driven from here (no reference code:
 * the reference is single-process).  `allreduce` is the collective library's in-place-capable
 * all-reduce with RCCL's ncclAllReduce signature -- (sendbuf, recvbuf, count, dtype, op, comm, stream),
 * returning 0 on success -- and `comm` its communicator; the caller creates both (see
 * rawaudiovae_kelsey_amd/ddp.py: RCCL loaded with ctypes, unique id shared over torch.distributed).
 * rv_plan_step_ddp enqueues ONE whole training step: forward, loss, backward with two gradient
 * buckets (fc4 | fc1,fc21,fc22,fc3) summed across ranks on an internal high-priority stream as
 * soon as backward has produced them, and Adam per bucket with the 1/world mean -- one host call,
 * no host synchronisation, capturable in a hipGraph.  Needs a grad arena and a non-default stream. */
typedef int (*rv_allreduce_fn)(const void* sendbuf, void* recvbuf, size_t count, int dtype, int op,
                               void* comm, void* stream);
/* Everything rv_plan_step_ddp needs from the caller, in one descriptor (copied; attach again to change a field,
 * comm == NULL detaches and keeps only comm_stream).  (Rounds 3-5 also carried a sharded-optimizer schedule -- reduce-scatter,
 * Adam on a rank's 1 / world of the arenas, all-gather of parameters or of a 16-bit parameter message; it won no row of the
 * 8-rank model (a second collective's start-up for an update that is 13 us to begin with) and was
 * removed in round 6.) */
typedef struct rv_comm_desc {
  void* comm; int world; int rank;
  rv_allreduce_fn allreduce;
  void* grad_bf16; /* optional: bf16 payload -- each rank's summed gradient rounded to bf16 into this arena */
                   /*   (as many 2-byte elements as the fp32 arenas hold floats) and summed by the collective in bf16;  */
                   /*   NULL: fp32, the exact mean of the ranks' fp32 gradients                                         */
  void* comm_stream; /* the stream the collectives are issued on, or NULL: one high-priority stream per process,     */
                   /*   created by the library.  Why a caller may want to choose: the HIP runtime multiplexes streams   */
                   /*   onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4), and when the collective stream shares */
                   /*   a queue with the compute stream the runtime resolves their cross-stream waits on the host --    */
                   /*   every kernel of the step then starts ~50 us late (880 us instead of 255 us per step at one      */
                   /*   rank).  ddp.pick_comm_stream times a short ping-pong against the compute stream and hands over  */
                   /*   the first candidate that is not affected.  The stream stays the caller's.                       */
} rv_comm_desc;
int rv_plan_attach_comm(rv_plan*, const rv_comm_desc*);
int rv_plan_step_ddp(rv_plan*, const float* x, const float* eps, float* recon_out, float kl_beta,
                     float lr, unsigned long long seed, void* stream);
/* Device pointer to (and, if n_bytes is given, size of) one buffer of the bound workspace, for tests and tools.  NULL for an
 * unknown or NULL name and for an unbound plan.  The names, in layout order:
 *   bf16 operands and padded biases   "xb" "W1b" "Whb" "W3b" "W4b" "b1p" "bhp" "b3p" "b4p"
 *   forward                           "h1" "mulv_slabs" "mulv" "eps" "z" "h3"
 *   backward                          "dP4" "dP3" "dz_slabs" "dmulv" "dP1"
 *   weight-gradient slabs, fp16 scales "dW1" "dWh" "dWh_us" "dW3" "dW4" "dW1_us" "dW4_us"
 *   bias-gradient partial rows        "db1p" "dbhp" "db3p" "db4p"
 *   fp8 images and state              "xq" "W1q" "W4q" "h3q" "dP4q" "dP1q" "fp8_state" "h3_amax"
 *   data-parallel flags, loss partials "ddp_flags" "mse_part" "kl_part" */
void* rv_plan_buffer(rv_plan*, const char* name, long* n_bytes);

/* ---- hipGraph capture of any sequence of the calls above on one stream ---- */
typedef struct rv_graph rv_graph;
int rv_graph_begin(void* stream);
int rv_graph_end(void* stream, rv_graph** out);
int rv_graph_launch(rv_graph*, void* stream);
void rv_graph_destroy(rv_graph*);

#ifdef __cplusplus
}
#endif
#endif /* RAWVAE_HIP_H */
