"""CPU checks of the streaming resynthesis contract: the float64 WOLA of tests/stream_oracle.py returns the input
delayed by P with an identity decoder, the framing / latency arithmetic, the C ABI's new entries, and the CLI's
argument checks (no device)."""
import os
import re
import subprocess
import sys

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
