"""Plain reference of the device RNG (csrc/philox.h), numpy only.

Philox4x32-10 is written from its published definition (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy
as 1, 2, 3", SC'11): ten rounds of

    (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0))

with M0 = 0xD2511F53, M1 = 0xCD9E8D57 and the key bumped by the Weyl constants (0x9E3779B9, 0xBB67AE85) between rounds.

How the device uses it (the contract the GPU tests pin):

  key      = (seed & m, seed >> 32)
  counter  = (ctr_lo & m, ctr_lo >> 32, ctr_hi & m, ctr_hi >> 32)           m = 2^32 - 1
  uniforms = min((float(word) + 0.5f) * 2^-32, 0.99999994f), all in fp32, float(word) rounded to nearest even
  normals  = (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1),  r0 = sqrt(-2 ln u_x), a0 = 2 pi u_y,
                                                            r1 = sqrt(-2 ln u_z), a1 = 2 pi u_w

The uniforms are reproduced bit for bit; the Box-Muller values are float64 functions of those exact uniforms, so the only
difference to a device value is the device's own fp32 log / sqrt / sin / cos arithmetic.

Counter layouts of the consumers:

  rv_randn, rv_reparameterize, rv_latent_mix, the streaming engine, the latent walk (accurate form):
      element i of a flat tensor is lane i & 3 of counter (ctr_lo = i >> 2, ctr_hi = offset)
  rv_reparam_fwd, rv_latent_fwd in every form (fast form, the training step's eps):
      element (b, l) of the [B, L] grid is lane l & 3 of counter (ctr_lo = b * (Lp / 4) + l / 4, ctr_hi = *step_counter)
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
U_MAX = np.float32(0.99999994)       # 1 - 2^-24, the largest fp32 below 1


def philox4x32_10_words(counter, key):
    """Philox4x32-10 on explicit words: counter = four uint64 arrays holding 32-bit values, key = two python ints.
    Returns the four output words as uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & M32 for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
        p0, p1 = _M0 * c0, _M1 * c2                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & M32, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & M32
    return c0, c1, c2, c3


def philox4x32_10(seed, ctr_lo, ctr_hi):
    """The device's call: 64-bit seed, 64-bit counter halves (uint64 arrays or ints) -> words [n, 4] uint64."""
    lo, hi = np.atleast_1d(np.asarray(ctr_lo, dtype=np.uint64)), np.atleast_1d(np.asarray(ctr_hi, dtype=np.uint64))
    lo, hi = np.broadcast_arrays(lo, hi)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10_words((lo & M32, lo >> _S32, hi & M32, hi >> _S32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=-1)


def uniforms(words):
    """The device's fp32 uniforms of 32-bit words, bit for bit."""
    f = np.asarray(words, dtype=np.uint64).astype(np.float64).astype(np.float32)   # exact, then one rounding to nearest even
    u = (f + np.float32(0.5)) * np.float32(2.0 ** -32)
    assert u.dtype == np.float32
    return np.minimum(u, U_MAX)


def normals4(seed, ctr_lo, ctr_hi):
    """[n, 4] float64 Box-Muller values of the exact fp32 uniforms of counters (ctr_lo, ctr_hi)."""
    u = uniforms(philox4x32_10(seed, ctr_lo, ctr_hi)).astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a, b = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    return np.stack([ra * np.cos(a), ra * np.sin(a), rb * np.cos(b), rb * np.sin(b)], axis=-1)


def randn_ref(n, seed, offset):
    """rv_randn(n, seed, offset) in float64: element i is lane i & 3 of counter (i >> 2, offset)."""
    n4 = (n + 3) // 4
    return normals4(seed, np.arange(n4, dtype=np.uint64), np.uint64(offset)).reshape(-1)[:n]


def eps_grid_ref(B, L, Lp, seed, step, row0=0):
    """The training step's eps [B, L] in float64: element (b, l) is lane l & 3 of counter (b * (Lp / 4) + l / 4, step).
    row0 > 0: rows [row0, B) only."""
    assert Lp % 4 == 0 and L <= Lp and 0 <= row0 < B
    g = (L + 3) // 4
    idx = (np.arange(row0, B, dtype=np.uint64)[:, None] * np.uint64(Lp // 4) + np.arange(g, dtype=np.uint64)[None, :]).reshape(-1)
    return normals4(seed, idx, np.uint64(step)).reshape(B - row0, 4 * g)[:, :L]


# Counters whose words sit at the edges of the uniform's range, for seed 1234 and ctr_lo = 0 (found by a search over
# ctr_hi < 2^26; tests/test_rng_cpu.py recomputes every one of them).  A word >= 0xffffff80 rounds to 2^32 as fp32, the
# uniform to 1.0, and the clamp makes the smallest radius, sqrt(-2 ln(1 - 2^-24)) = 3.45e-4; a word below 0x100 gives
# radii of 5.8 and more.
EDGE_SEED = 1234
EDGE_X_HIGH = (2145465, 0xFFFFFFAE)     # (ctr_hi, word x)
EDGE_X_LOW = (11184793, 0xAF)
EDGE_Z_HIGH = (23388563, 0xFFFFFFDF)     # (ctr_hi, word z): the second pair of the draw
EDGE_Z_LOW = (41067945, 0x83)
EDGES = (EDGE_X_HIGH, EDGE_X_LOW, EDGE_Z_HIGH, EDGE_Z_LOW)
