"""CPU checks of the streaming resynthesis contract: the float64 WOLA of tests/stream_oracle.py returns the input
delayed by P with an identity decoder, the framing / latency arithmetic, the C ABI's new entries, and the CLI's
argument checks (no device).  And the fp32 oracle that tests/test_stream_edges_gpu.py holds the kernels to, checked on the
host: fma32 against rational arithmetic, chain32 and wola32 against float64 within their rounding bounds, frames32 and
latent_ctl against their statements."""
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO  # noqa: E402

import stream_oracle as SO  # noqa: E402


def _stream():
    from rawaudiovae_kelsey_amd import stream
    return stream


@pytest.mark.parametrize("S,hop,window", [(64, 32, "hann"), (64, 16, "hann"), (1024, 256, "hann"),
                                          (64, 64, None), (64, 16, None), (64, 8, None), (48, 12, None)])
def test_identity_decoder_wola_is_a_pure_delay(S, hop, window):
    rng = np.random.default_rng(S + hop)
    x = rng.uniform(-1, 1, 10 * S)
    w = _stream().window_values(S, window).astype(np.float64)
    fr = SO.frames(x, S, hop)                  # the identity decoder: D_f = frame f
    P = S - hop
    y = SO.wola(fr, w, hop, fr.shape[0] * hop)
    ref = np.concatenate([np.zeros(P), x])[:y.size]
    lo = 1 if window == "hann" else 0         # Yp[0] = 0 under Hann (w[0] = 0 and only frame 0 covers t = 0)
    np.testing.assert_allclose(y[lo:], ref[lo:], rtol=0, atol=1e-12)
    if P > 0 or window:
        assert y[0] == 0.0


def test_latency_and_framing():
    st = _stream()
    assert st.check_args(1024, 1024) == (1024, 0, 1)
    assert st.check_args(1024, 1024, 256, "hann") == (256, 768, 4)
    assert st.check_args(1024, 256, 256) == (256, 768, 1)
    assert st.check_args(1024, 4096, 128) == (128, 896, 32)
    for S, block, hop, window in [(1024, 1024, 1000, None), (1024, 1000, 256, None), (1024, 128, 256, None),
                                  (1024, 1024, 1024, "hann"), (1024, 1024, 512 * 2, "hann"), (1024, 1024, 256, "hamming"),
                                  (1024, 0, 256, None)]:
        with pytest.raises(ValueError):
            st.check_args(S, block, hop, window)
    assert st.check_args(1024, 1024, 512, "hann")[1] == 512
    # frames of the oracle: after feeding k blocks, k * block / hop frames are complete
    S, hop, block = 64, 16, 32
    for k in range(1, 5):
        assert SO.frames(np.zeros(k * block), S, hop).shape[0] == k * block // hop


def test_window_values_and_norm():
    st = _stream()
    S = 1024
    w = st.window_values(S, "hann")
    ref = (0.5 - 0.5 * np.cos(2 * np.pi * np.arange(S) / S)).astype(np.float32)
    assert w.dtype == np.float32 and np.array_equal(w, ref) and w[0] == 0
    n = st.window_norm(w, 256)
    assert n.shape == (768 + 256,) and n[0] == 0 and np.all(n[1:] > 0)
    np.testing.assert_allclose(n[768:], 2.0, rtol=1e-6)      # periodic Hann at hop S/4 sums to 2
    assert np.array_equal(st.window_norm(st.window_values(S, None), S), np.ones(S, dtype=np.float32))


# ---- the fp32 oracle of tests/test_stream_edges_gpu.py, checked on the host ------------------------------------------

def _rn32(v):
    """A Fraction rounded to the nearest fp32, ties to even (normal range), as a Python float."""
    if v == 0:
        return 0.0
    e = 0
    while abs(v) >= Fraction(2) ** (e + 1):
        e += 1
    while abs(v) < Fraction(2) ** e:
        e -= 1
    assert -126 <= e <= 127
    q = Fraction(2) ** (e - 23)
    return float(round(v / q) * q)              # Fraction.__round__ rounds a half to even; the result fits 25 bits


def test_fma32_is_the_correctly_rounded_fma():
    rng = np.random.default_rng(2024)
    n = 3000
    x = rng.uniform(-2, 2, n).astype(np.float32)
    w = rng.uniform(-2, 2, n).astype(np.float32)
    acc = rng.uniform(-2, 2, n).astype(np.float32)
    p32 = (x.astype(np.float64) * w.astype(np.float64)).astype(np.float32)
    # forced near-cancellations: acc = -fl(x w) and its neighbours up to 3 ulps away, and an acc 2^24 times the product
    # (the product decides a tie of the sum at most)
    for i, k in enumerate(range(n // 3, 2 * n // 3)):
        a = -p32[k]
        for _ in range(i % 4):
            a = np.nextafter(a, np.float32(np.inf if i % 8 < 4 else -np.inf), dtype=np.float32)
        acc[k] = a
    big = slice(2 * n // 3, 2 * n // 3 + 300)
    acc[big] = (p32[big].astype(np.float64) * 2.0 ** rng.integers(22, 27, 300)).astype(np.float32)
    half = slice(2 * n // 3 + 300, 2 * n // 3 + 600)          # exact ties of the fp32 rounding: x w = 2^-24 = ulp(acc) / 2
    x[half], w[half] = np.float32(2.0 ** -12), np.float32(2.0 ** -12)
    acc[half] = (1.0 + np.arange(300) * 2.0 ** -23).astype(np.float32)
    got = SO.fma32(x, w, acc)
    assert got.dtype == np.float32
    want = np.array([_rn32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))) for a, b, c in zip(x, w, acc)])
    assert np.array_equal(got.astype(np.float64), want), np.argwhere(got.astype(np.float64) != want)[:5].tolist()
    # the near-cancellations did cancel (an unfused fl(x w) + acc loses them), and the ties went to even
    two = (p32 + acc).astype(np.float32)
    assert (np.abs(got[n // 3:2 * n // 3]) < 1e-5).all() and (got != two).sum() > n // 10
    assert np.array_equal(got[half], np.where(np.arange(300) % 2 == 0, acc[half], np.nextafter(acc[half], np.float32(2))))


@pytest.mark.parametrize("M,N,K", [(3, 5, 1), (4, 7, 31), (2, 9, 76), (1, 3, 320)])
def test_chain32_stays_within_gamma_of_float64(M, N, K):
    rng = np.random.default_rng(M + N + K)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    b = rng.uniform(-1, 1, N).astype(np.float32)
    for bias in (b, None):
        got = SO.chain32(x, W, bias)                          # (asserts that no intermediate is subnormal)
        assert got.dtype == np.float32 and got.shape == (M, N)
        b64 = 0.0 if bias is None else b.astype(np.float64)
        ref = x.astype(np.float64) @ W.astype(np.float64).T + b64
        mag = np.abs(x).astype(np.float64) @ np.abs(W).astype(np.float64).T + np.abs(b64)
        assert (np.abs(got - ref) <= SO.gamma(K) * mag).all(), (np.abs(got - ref) / mag).max() / SO.gamma(K)
        assert np.array_equal(SO.chain32(x, W, bias, 1), np.maximum(got, 0))
        assert np.array_equal(SO.chain32(x, W, bias, 2), got)   # the pre-activation
    # one term: the chain is the rounded product, then the rounded sum
    one = SO.chain32(x[:, :1], W[:, :1], b)
    assert np.array_equal(one, (x[:, :1] * W[None, :, 0]).astype(np.float32) + b)


def test_frames32_and_latent_ctl_follow_the_kernels_statements():
    rng = np.random.default_rng(6)
    S, hop, block = 12, 3, 6
    x = rng.uniform(-1, 1, 5 * block).astype(np.float32)
    hist = np.zeros(S - hop, dtype=np.float32)
    rows = []
    for k in range(5):
        fr, hist = SO.frames32(hist, x[k * block:(k + 1) * block], S, hop)
        assert fr.dtype == np.float32 and fr.shape == (block // hop, S) and hist.shape == (S - hop,)
        rows.append(fr)
    assert np.array_equal(np.concatenate(rows).astype(np.float64), SO.frames(x, S, hop))
    fr, h0 = SO.frames32(np.zeros(0, dtype=np.float32), x[:8], 4, 4)      # P = 0
    assert np.array_equal(fr, x[:8].reshape(2, 4)) and h0.size == 0
    m, sc, of = (rng.uniform(-2, 2, 4000).astype(np.float32) for _ in range(3))
    got = SO.latent_ctl(m, sc, of)
    two = (m.astype(np.float64) * sc).astype(np.float32).astype(np.float64) + of
    assert got.dtype == np.float32 and np.array_equal(got, two.astype(np.float32))
    assert (got != SO.fma32(m, sc, of)).any()                 # two roundings, not one


@pytest.mark.parametrize("S,hop,window", [(12, 3, "hann"), (40, 8, "hann"), (36, 36, None), (320, 80, "hann"),
                                          (24, 8, None)])
def test_wola32_stays_within_the_bound_of_float64(S, hop, window):
    st = _stream()
    rng = np.random.default_rng(S * 3 + hop)
    nf, c = 11, S // hop
    dec = np.tanh(rng.uniform(-2, 2, (nf, S))).astype(np.float32)
    w = st.window_values(S, window)
    norm = st.window_norm(w, hop)
    n = nf * hop
    got = SO.wola32(dec, w, norm, hop, n)
    assert got.dtype == np.float32 and got.shape == (n,)
    SO.assert_normal(got, "wola32")
    ref = SO.wola(dec, w, hop, n)
    mag = SO.wola(np.abs(dec), w, hop, n)
    bound = SO.gamma(2 * c + 3) * mag
    assert (np.abs(got - ref) <= bound).all(), (np.abs(got - ref).max(), bound.max())
    if window == "hann":
        assert got[0] == 0 and norm[0] == 0                   # the normaliser's zero
    if hop == S:
        assert np.array_equal(got, dec.reshape(-1))           # one frame per sample, weight 1: the rows themselves
    # the order of the frames is ascending: a descending accumulation differs somewhere once three frames overlap
    if c >= 3:
        num = np.zeros(n + S, dtype=np.float32)
        for f in reversed(range(nf)):
            num[f * hop:f * hop + S] += w * dec[f]
        t = np.arange(n)
        den = norm[np.where(t < S - hop, t, S - hop + t % hop)]
        rev = np.divide(num[:n], den, out=np.zeros(n, dtype=np.float32), where=den != 0)
        assert (rev != got).any()


def _decls():
    with open(os.path.join(REPO, "include", "rawvae_hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_stream_entries_and_binding(tmp_path):
    from rawaudiovae_kelsey_amd import _lib
    names = _decls()
    new = ["rv_small_linear_f32", "rv_stream_workspace_bytes", "rv_stream_process", "rv_stream_reset"]
    assert set(new) <= set(names) and len(names) <= 70
    assert set(new) <= set(_lib.EXPORTED)
    src = tmp_path / "c.c"
    src.write_text('#include "rawvae_hip.h"\nint main(void) { rv_stream_desc d = {0}; d.S = 1024; '
                   'return (int)sizeof(d) > 0 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(tmp_path / "c.o")], check=True)
    lib = _lib.lib()
    assert lib.rv_stream_workspace_bytes(1024, 2048, 256, 16, 1024, 256) > 0
    assert lib.rv_stream_workspace_bytes(1024, 2048, 256, 16, 1000, 256) == -1


def test_resynth_help_and_bad_flags():
    r = subprocess.run([sys.executable, os.path.join(REPO, "resynth.py"), "--help"], capture_output=True, text=True,
                       cwd=REPO)
    assert r.returncode == 0 and "--window" in r.stdout and "--hop" in r.stdout
    sys.path.insert(0, REPO)
    import resynth
    base = ["--config", os.path.join(REPO, "default.ini"), "--checkpoint", "none.pt", "--in", "a.wav", "--out", "b.wav"]
    for extra in (["--hop", "1000"], ["--hop", "1024", "--window", "hann"], ["--window", "hamming"],
                  ["--hop", "256", "--block", "300"], ["--hop", "0"], ["--temperature", "x"]):
        with pytest.raises(ValueError):
            resynth.main(base + extra)
