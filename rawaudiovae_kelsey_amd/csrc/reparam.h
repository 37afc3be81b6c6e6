// The latent rules of the VAE, each defined here once, down to the bit: the reparameterisation with its KL term, its
// backward, and the finish of the loss scalar.  Every kernel that applies one calls it from here -- the step's row-local
// and GEMM forms (k_reparam_fwd / k_reparam_bwd, k_latent_fwd / k_latent_bwd, the EPI_REPARAM / EPI_REPARAM_BWD epilogues,
// k_dz_reparam_gemm, k_loss_from_partials) and the audio tools (k_reparameterize, k_latent_mix, k_stream_heads) -- and
// keeps its own loads, masks, eps fetches, stores and reductions.  Operand order and contraction decide the last bit of
// these expressions, and the step is bit-reproducible across its schedules: change a rule here, nowhere else.
#pragma once
#include "common.h"

namespace rv {

// z = mu + eps * exp(logvar / 2)   (reparameterize, model.py:23-26)
__device__ __forceinline__ float reparam_z(float mu, float lv, float e) { return mu + e * __expf(0.5f * lv); }

// The same z, and kl += 1 + logvar - mu^2 - sigma^2 (the summand of KLD, model.py:45), sigma^2 as the square of the sd
// that z uses.  (Not through reparam_z: sd is computed once and used twice.  z leaves through a reference so that it is
// assigned before the KL term is formed, the statement order the kernels have always had: a returned z would be assigned
// after it, and the instruction scheduler follows that order.)
__device__ __forceinline__ void reparam_fwd(float mu, float lv, float e, float& z, float& kl) {
  const float sd = __expf(0.5f * lv);
  z = mu + e * sd;
  kl += 1.f + lv - mu * mu - sd * sd;
}

// Gradients of the loss (model.py:38-47) with respect to mu and logvar through z (dz) and through the KL term, whose
// weight is kl_beta / (B L) = kl_beta * inv_nk.  Gradients arriving from outside are the caller's to add.
__device__ __forceinline__ void reparam_bwd(float dz, float mu, float lv, float e, float kl_beta, float inv_nk, float& dmu,
                                            float& dlv) {
  const float sd = __expf(0.5f * lv);
  dmu = dz + kl_beta * mu * inv_nk;
  dlv = dz * e * 0.5f * sd + kl_beta * 0.5f * (sd * sd - 1.f) * inv_nk;
}

// The eps of latents l .. l + 3 of batch row b that the step draws itself is normal4_fast's draw number
// b (Lp / 4) + l / 4, the group's index over the padded [Bp, Lp / 4] grid.  Not a function: k_reparam_fwd and k_latent_fwd
// have that index before they have b and l (their flat thread index), and forming it again from b and l costs
// instructions in both (profiles/reparam_rules_ab.txt).

// The loss scalar from the partial sums of a step (loss_function, model.py:38-47), by one block of NW waves:
// threads 0..255 sum mse_partial[n_mse] and kl_partial[n_kl] in strides of 256, the block adds them up, and thread 0
// writes {mse + kl_beta kld, mse, kld} to loss_out, or to slot (counter - 1) mod ring of a ring of 4-float slots there
// (a counter of 0: slot ring - 1; no counter or no ring: slot 0).
// reduce(v) is the calling kernel's own sum over its block, valid in thread 0: block_sum_256 in the 256-thread
// kernels, block_sum<8> in the 512-thread one, as each has always had.  The two differ in the sign of a zero sum
// (0 + -0 against -0), so they stay two.
template <int NW, class BlockSum>
__device__ __forceinline__ void loss_finish(const float* mse_partial, int n_mse, const float* kl_partial, int n_kl, long B,
                                            long S, long L, float kl_beta, float* loss_out, const long long* step_counter,
                                            int ring, BlockSum reduce) {
  const int tid = threadIdx.x;
  float m = 0.f, k = 0.f;
  if (NW == 4 || tid < 256) {   // (a block of 4 waves has no other threads)
    for (int i = tid; i < n_mse; i += 256) m += mse_partial[i];
    for (int i = tid; i < n_kl; i += 256) k += kl_partial[i];
  }
  m = reduce(m);
  k = reduce(k);
  if (tid == 0) {
    const float mse = m / ((float)B * (float)S);
    const float kld = -0.5f * k * (1.0f / ((float)B * (float)L));
    if (step_counter && ring > 0) loss_out += 4 * (((*step_counter - 1) % ring + ring) % ring);
    loss_out[0] = mse + kl_beta * kld;
    loss_out[1] = mse;
    loss_out[2] = kld;
  }
}

}  // namespace rv
