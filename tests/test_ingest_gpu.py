"""Device ingest of the streaming loader: rv_pcm_to_f32 bit-equal to the host decode, rv_resample_sinc_hann against
the interpolation formula and the host restatement, and StreamingFrames(ingest="device") against ingest="host"."""
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
from test_ingest_cpu import FORMATS, random_samples, wav_file  # noqa: E402

PAIRS = [(48000, 44100), (44100, 48000), (22050, 44100), (32000, 44100), (44100, 16000), (96000, 44100),
         (8000, 44100), (44100, 192000), (192000, 44100)]


def _device_decode(path, hop=1):
    from rawaudiovae_kelsey_amd import data as D
    h, buf = D.read_wav_payload(path)
    out, n = D.pcm_to_f32_device(buf.cuda(), h, hop)
    return out.cpu().numpy(), n


@pytest.mark.gpu
@pytest.mark.parametrize("kind,tag,bps,bits,dtype", FORMATS)
@pytest.mark.parametrize("channels", [1, 2, 6])
def test_pcm_to_f32_is_the_host_decode(tmp_path, kind, tag, bps, bits, dtype, channels):
    from rawaudiovae_kelsey_amd import data as D
    rng = np.random.default_rng(100 + bps * 7 + channels)
    for n, hop in ((4099, 1), (4099, 128), (1, 64), (0, 128), (37, 1)):
        raw, _ = random_samples(kind, max(n, 1), channels, rng)
        raw = raw[:n * channels * bps]
        p = wav_file(tmp_path / ("x%d_%d.wav" % (n, hop)), raw, tag, channels, 16000, bits, bps, extra=n == 37)
        a, _ = D.read_wav(p)
        ref = a if a.ndim == 1 else a[:, 0]
        got, m = _device_decode(p, hop)
        assert m == n and len(got) == (n + hop - 1) // hop * hop
        assert got.dtype == np.float32 and np.array_equal(got[:n].view(np.uint32), ref.view(np.uint32)), (kind, n)
        assert not got[n:].any()


def _direct(a, sr_in, sr_out, pos, lpw=6, rolloff=0.99):
    """The windowed-sinc interpolation formula in float64 at output positions `pos` (test_train_entry.py's)."""
    g = math.gcd(sr_in, sr_out)
    orig, new = sr_in // g, sr_out // g
    base = min(orig, new) * rolloff
    out = []
    for m in pos:
        t = np.clip((np.arange(len(a)) - m * orig / new) / orig * base, -lpw, lpw)
        w = np.cos(t * math.pi / lpw / 2) ** 2
        tt = t * math.pi
        s = np.where(tt == 0, 1.0, np.sin(tt) / np.where(tt == 0, 1.0, tt))
        out.append(float(np.sum(a * s * w) * base / orig))
    return np.array(out)


@pytest.mark.gpu
@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_resampler_matches_the_formula_and_the_host(sr_in, sr_out):
    from rawaudiovae_kelsey_amd import data as D
    g = math.gcd(sr_in, sr_out)
    orig, new = sr_in // g, sr_out // g
    taps = D._sinc_hann_bank(sr_in, sr_out)[3].shape[1]
    rng = np.random.default_rng(sr_in + sr_out)
    # edge lengths: empty, one sample, shorter than one filter, not a multiple of orig; then a long one
    for n in (0, 1, taps // 2, 3 * orig + 1, 5000, 40000):
        a = rng.standard_normal(n).astype(np.float32)
        y, m = D.resample_sinc_hann_device(torch.from_numpy(a).cuda(), sr_in, sr_out)
        y = y.cpu().numpy()
        assert m == len(y) == math.ceil(new * n / orig) == len(D._resample_sinc_hann(a, sr_in, sr_out)), n
        if n == 0:
            continue
        assert np.abs(y - D._resample_sinc_hann(a, sr_in, sr_out)).max() <= 1e-5, n
        pos = sorted({0, m // 2, m - 1} | set(range(0, m, max(1, m // 7))))
        if n <= 5000:
            # most of the distance to the formula is the fp32 rounding of the filter bank, which the host shares: on
            # some inputs the host itself is past 5e-6, and the device may then be as far as the host is (+1e-6)
            d = _direct(a.astype(np.float64), sr_in, sr_out, pos)
            host_err = np.abs(D._resample_sinc_hann(a, sr_in, sr_out)[pos] - d).max()
            assert np.abs(y[pos] - d).max() < max(5e-6, host_err + 1e-6), (n, host_err)
    # the inputs the host path is held to 5e-6 on (test_train_entry.py draws them in this order)
    rng0 = np.random.default_rng(0)
    for si, so in [(48000, 44100), (44100, 22050), (22050, 44100), (32000, 44100), (44100, 16000)]:
        a = rng0.standard_normal(3000).astype(np.float32)
        if (si, so) == (sr_in, sr_out):
            y, m = D.resample_sinc_hann_device(torch.from_numpy(a).cuda(), sr_in, sr_out)
            pos = [0, 1, 2, 57, 500, m // 2, m - 3, m - 1]
            assert np.abs(y.cpu().numpy()[pos] - _direct(a.astype(np.float64), sr_in, sr_out, pos)).max() < 5e-6
    # zero padding to a hop, and an offset source of n samples inside a longer buffer
    a = rng.standard_normal(3001).astype(np.float32)
    x = torch.from_numpy(np.concatenate([a, np.full(50, 7.0, np.float32)])).cuda()
    y, m = D.resample_sinc_hann_device(x, sr_in, sr_out, n=3001, hop=128)
    y = y.cpu().numpy()
    assert len(y) % 128 == 0 and len(y) - m < 128 and not y[m:].any()
    assert np.abs(y[:m] - D._resample_sinc_hann(a, sr_in, sr_out)).max() <= 1e-5


@pytest.mark.gpu
def test_resampler_equal_rates_returns_the_source_and_bad_extents_raise():
    from rawaudiovae_kelsey_amd import _lib
    from rawaudiovae_kelsey_amd import data as D
    x = torch.randn(1000, device="cuda")
    y, n = D.resample_sinc_hann_device(x, 44100, 44100)
    assert y is x and n == 1000
    out = torch.empty(10, device="cuda")
    bank = D._device_bank(48000, 44100, x.device)
    with pytest.raises(_lib.RvError):      # n_out shorter than ceil(new * n / orig)
        _lib.lib().rv_resample_sinc_hann(x.data_ptr(), 1000, bank[3].data_ptr(), 160, 147, bank[2], out.data_ptr(), 10,
                                         None)
    with pytest.raises(_lib.RvError):      # equal reduced rates
        _lib.lib().rv_resample_sinc_hann(x.data_ptr(), 10, bank[3].data_ptr(), 3, 3, 7, out.data_ptr(), 10, None)
    with pytest.raises(_lib.RvError):      # n_out must be the hop-padded sample count
        _lib.lib().rv_pcm_to_f32(x.data_ptr(), 4000, _lib.WAV_PCM, 1, 2, 1, out.data_ptr(), 10, None)


def _tone_wav(path, seconds, sr, f0, channels=1, kind="i16"):
    from scipy.io import wavfile
    t = np.arange(int(seconds * sr)) / sr
    a = 0.5 * np.sin(2 * np.pi * f0 * t) + 0.2 * np.sin(2 * np.pi * 2.7 * f0 * t)
    if channels > 1:
        a = np.stack([a] + [a * (-1) ** c * 0.5 for c in range(1, channels)], axis=1)
    wavfile.write(str(path), sr, (a * 32767).astype(np.int16) if kind == "i16" else a.astype(np.float32))


def _corpus(tmp_path, sr, file_sr=None):
    files = []
    for i, (sec, ch) in enumerate([(0.7, 1), (0.25, 2), (0.05, 1), (1.1, 2), (0.4, 1)]):
        p = tmp_path / ("f%d.wav" % i)
        _tone_wav(p, sec, file_sr or sr, 110.0 * (i + 2), channels=ch, kind="f32" if i == 4 else "i16")
        files.append(p)
    return files


def _run(files, sr, ingest, bs, nb, **kw):
    from rawaudiovae_kelsey_amd import data as D
    st = D.StreamingFrames(files, sr, 64, 256, "cuda", ingest=ingest, **kw)
    return torch.cat(list(st.batches(bs, nb))).cpu().numpy(), st


@pytest.mark.gpu
def test_streaming_device_ingest_is_the_host_stream(tmp_path):
    files = _corpus(tmp_path, 8000)
    # files of 400 to 8800 samples (the 0.05 s one: 3 frames); batches of 50 straddle file boundaries
    for kw in (dict(shuffle=False), dict(shuffle=True, seed=5), dict(shuffle=True, seed=5, cache_bytes=12000)):
        ref, _ = _run(files, 8000, "host", 50, 23, **kw)
        got, st = _run(files, 8000, "device", 50, 23, **kw)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), kw
        if "cache_bytes" in kw:                # evicted and re-ingested: the cache stays within its bound + one file
            assert len(st._cache) < len(files)
    # two iterators of one stream (a fresh file order each, prefetch state carried over)
    from rawaudiovae_kelsey_amd import data as D
    sh = D.StreamingFrames(files, 8000, 64, 256, "cuda", seed=9, cache_bytes=20000)
    sd = D.StreamingFrames(files, 8000, 64, 256, "cuda", seed=9, cache_bytes=20000, ingest="device")
    for _ in range(2):
        a = torch.cat(list(sh.batches(64, 9))).cpu().numpy()
        b = torch.cat(list(sd.batches(64, 9))).cpu().numpy()
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_streaming_device_ingest_off_rate_and_no_full_frame(tmp_path):
    files = _corpus(tmp_path, 8000, file_sr=11025)
    ref, _ = _run(files, 8000, "host", 64, 15, shuffle=True, seed=2)
    got, _ = _run(files, 8000, "device", 64, 15, shuffle=True, seed=2)
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-5
    short = tmp_path / "short"
    short.mkdir()
    _tone_wav(short / "s.wav", 0.01, 8000, 440.0)
    from rawaudiovae_kelsey_amd import data as D
    with pytest.raises(ValueError, match="full 256-sample frame"):
        list(D.StreamingFrames([short / "s.wav"], 8000, 64, 256, "cuda", ingest="device").batches(8, 2))


@pytest.mark.gpu
def test_train_iterable_device_ingest_matches_host(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import train_iterable as TI
    from test_train_entry import _dataset, _ini

    ds = _dataset(tmp_path)

    def run(**kw):
        TI.main(["--config", str(_ini(ds, iterable=True, **kw))])
        out = capsys.readouterr().out
        return [float(l.split("Loss: ")[1].split()[0]) for l in out.splitlines() if l.startswith("====> Batch:")]
    ref = run(mi355x__ingest="host")
    got = run(mi355x__ingest="device")
    assert len(got) == len(ref) == 7 and all(np.isfinite(got))
    np.testing.assert_allclose(got, ref, rtol=2e-2)
