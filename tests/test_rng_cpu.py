"""The RNG oracle (tests/rng_oracle.py) against the published Philox4x32-10 known answers, and the facts about the fp32
uniforms that the GPU tests (tests/test_rng_gpu.py) lean on.  No GPU."""
import numpy as np

import rng_oracle as R


def _words(ctr, key):
    w = R.philox4x32_10_words([np.array([c], dtype=np.uint64) for c in ctr], key)
    return " ".join("%08x" % int(x[0]) for x in w)


def test_published_known_answers():
    """The three Philox4x32-10 vectors of the Random123 distribution (kat_vectors): zeros, ones, digits of pi."""
    assert _words((0, 0, 0, 0), (0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _words((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _words((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_seed_and_counter_halves_are_the_words():
    """philox4x32_10(seed, lo, hi): key = the halves of seed, counter = (lo & m, lo >> 32, hi & m, hi >> 32)."""
    seed = (0x299F31D0 << 32) | 0xA4093822
    lo, hi = (0x85A308D3 << 32) | 0x243F6A88, (0x03707344 << 32) | 0x13198A2E
    w = R.philox4x32_10(seed, lo, hi)
    assert w.shape == (1, 4) and [int(x) for x in w[0]] == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    # arrays broadcast, every element is its own counter
    many = R.philox4x32_10(seed, np.array([lo, 0, lo], dtype=np.uint64), np.uint64(hi))
    assert (many[0] == w[0]).all() and (many[2] == w[0]).all() and not (many[1] == w[0]).all()


def test_uniforms_are_the_devices_fp32_arithmetic():
    words = np.array([0, 1, 0xAF, 0x7FFFFFFF, 0x80000000, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFAE, 0xFFFFFFFF], dtype=np.uint64)
    u = R.uniforms(words)
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -33) and u[1] == np.float32(1.5 * 2.0 ** -32) and u[2] == np.float32(175.5 * 2.0 ** -32)
    # 0x7fffffff rounds up to 2^31 as fp32 (nearest even), so both land on 0.5
    assert u[3] == np.float32(0.5) and u[4] == np.float32(0.5)
    # the last word that stays below 2^32 as fp32, and the first that rounds to 2^32: u = 1.0, clamped
    assert u[5] == R.U_MAX and float(u[5]) == 1.0 - 2.0 ** -24
    assert (u[6:] == R.U_MAX).all()
    # every uniform is in [2^-33, 1 - 2^-24]: log and sqrt stay finite
    rng = np.random.default_rng(0)
    r = R.uniforms(rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64))
    assert r.min() >= np.float32(2.0 ** -33) and r.max() <= R.U_MAX
    # normal4's `+ 1e-30f` changes no uniform: half an ulp of the smallest one (2^-33) is 2^-57 = 6.9e-18
    for a in (u, r):
        assert ((a + np.float32(1e-30)) == a).all() and (a + np.float32(1e-30)).dtype == np.float32


def test_edge_counters_hit_the_edges():
    """The constants the GPU tests launch as single counters, recomputed: word x at the top of the range (u rounds to 1.0
    and is clamped: the smallest radius there is, 3.45e-4) and near the bottom (a radius of about 5.8)."""
    hi, word = R.EDGE_X_HIGH
    w = R.philox4x32_10(R.EDGE_SEED, 0, hi)[0]
    assert int(w[0]) == word == 0xFFFFFFAE and R.uniforms(w[:1])[0] == R.U_MAX
    n = R.normals4(R.EDGE_SEED, 0, hi)[0]
    assert abs(np.hypot(n[0], n[1]) - 3.4527e-4) < 1e-8 and np.isfinite(n).all()
    hi, word = R.EDGE_X_LOW
    w = R.philox4x32_10(R.EDGE_SEED, 0, hi)[0]
    assert int(w[0]) == word == 0xAF
    n = R.normals4(R.EDGE_SEED, 0, hi)[0]
    assert abs(np.hypot(n[0], n[1]) - 5.8333) < 1e-3 and np.isfinite(n).all()
    # the same two edges for word z (the second Box-Muller pair of the draw)
    hi, word = R.EDGE_Z_HIGH
    w = R.philox4x32_10(R.EDGE_SEED, 0, hi)[0]
    assert int(w[2]) == word == 0xFFFFFFDF and R.uniforms(w[2:3])[0] == R.U_MAX
    n = R.normals4(R.EDGE_SEED, 0, hi)[0]
    assert abs(np.hypot(n[2], n[3]) - 3.4527e-4) < 1e-8 and np.isfinite(n).all()
    hi, word = R.EDGE_Z_LOW
    w = R.philox4x32_10(R.EDGE_SEED, 0, hi)[0]
    assert int(w[2]) == word == 0x83
    n = R.normals4(R.EDGE_SEED, 0, hi)[0]
    assert 5.8 < np.hypot(n[2], n[3]) < 5.95 and np.isfinite(n).all()
    assert len(R.EDGES) == 4


def test_index_helpers():
    seed = 0x9E3779B97F4A7C15
    a = R.randn_ref(11, seed, 5)
    n4 = R.normals4(seed, np.arange(3, dtype=np.uint64), 5)
    assert a.shape == (11,) and (a == n4.reshape(-1)[:11]).all()
    # a longer draw starts with the shorter one; the offset is the counter's high half
    assert (R.randn_ref(4099, seed, 5)[:11] == a).all() and not (R.randn_ref(11, seed, 6) == a).any()
    assert not (R.randn_ref(11, seed, (1 << 32) + 5) == a).any()
    g = R.eps_grid_ref(5, 7, 64, seed, 3)
    assert g.shape == (5, 7)
    for b, l in [(0, 0), (0, 6), (4, 3), (2, 4)]:
        assert g[b, l] == R.normals4(seed, b * 16 + l // 4, 3)[0, l & 3]
    # another padded width moves every row but the first
    g2 = R.eps_grid_ref(5, 7, 128, seed, 3)
    assert (g2[0] == g[0]).all() and not (g2[1:] == g[1:]).any()
    # moments of the float64 values over 2^18 draws (a wrong transform would show here already)
    big = R.randn_ref(1 << 18, 1234, 0)
    assert abs(big.mean()) < 1e-2 and abs(big.std() - 1) < 1e-2
