"""Host side of the streaming loader's device ingest: the WAV header reader against scipy.io.wavfile, the filter bank
factored out of `_resample_sinc_hann` (the function's output must not move), and the `ingest` switches."""
import math
import os
import struct
import sys
import warnings

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402

# (name, format tag, bytes per sample, bits, numpy dtype of scipy's read)
FORMATS = [("u8", 1, 1, 8, np.uint8), ("i16", 1, 2, 16, np.int16), ("i24", 1, 3, 24, np.int32),
           ("i32", 1, 4, 32, np.int32), ("f32", 3, 4, 32, np.float32), ("f64", 3, 8, 64, np.float64)]


def random_samples(kind, n, channels, rng):
    """[n, channels] samples of a format, as the payload's little-endian bytes and as scipy will return them."""
    if kind == "u8":
        a = rng.integers(0, 256, (n, channels), dtype=np.uint8)
        return a.tobytes(), a
    if kind == "i16":
        a = rng.integers(-32768, 32768, (n, channels), dtype=np.int16)
        a[0, 0], a[-1, 0] = -32768, 32767
        return a.astype("<i2").tobytes(), a
    if kind == "i24":
        v = rng.integers(-(1 << 23), 1 << 23, (n, channels), dtype=np.int32)
        v[0, 0], v[-1, 0] = -(1 << 23), (1 << 23) - 1
        raw = v.astype("<i4").view(np.uint8).reshape(n, channels, 4)[:, :, :3].tobytes()
        return raw, v << 8                   # scipy left-justifies 24-bit samples into int32
    if kind == "i32":
        a = rng.integers(-(1 << 31), 1 << 31, (n, channels), dtype=np.int64).astype(np.int32)
        a[0, 0], a[-1, 0] = -(1 << 31), (1 << 31) - 1
        return a.astype("<i4").tobytes(), a
    if kind == "f32":
        a = (rng.standard_normal((n, channels)) * 0.5).astype(np.float32)
        return a.astype("<f4").tobytes(), a
    a = rng.standard_normal((n, channels)) * 0.5
    a[0, 0] = 1.0 + 2.0 ** -30               # rounds to nearest, not down
    return a.astype("<f8").tobytes(), a


def wav_file(path, payload, tag, channels, rate, bits, bps, extensible=False, extra=False):
    """A WAV file written byte by byte: optional WAVE_FORMAT_EXTENSIBLE fmt chunk, optional LIST / JUNK / odd-sized
    unknown chunks around the fmt and data chunks (an odd data chunk gets its pad byte)."""
    block_align = channels * bps
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * block_align, block_align, bits)
    if extensible:
        guid = struct.pack("<I", tag) + b"\x00\x00\x10\x00\x80\x00\x00\xAA\x00\x38\x9B\x71"
        fmt += struct.pack("<HHI", 22, bits, 0) + guid

    def chunk(cid, body):
        return cid + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")
    body = b"WAVE"
    if extra:
        body += chunk(b"JUNK", b"\x00" * 28) + chunk(b"LIST", b"INFOISFT\x05\x00\x00\x00abcd\x00\x00")
    body += chunk(b"fmt ", fmt)
    if extra:
        body += chunk(b"xtra", b"\x01\x02\x03")   # unknown, odd-sized: skipped with its pad byte
    body += chunk(b"data", payload)
    if extra:
        body += chunk(b"LIST", b"INFOICMT\x03\x00\x00\x00hi\x00\x00")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path


def scipy_read(path):
    from scipy.io import wavfile
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return wavfile.read(str(path))


@pytest.mark.parametrize("kind,tag,bps,bits,dtype", FORMATS)
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("layout", ["plain", "extra_chunks", "extensible"])
def test_wav_header_agrees_with_scipy(tmp_path, kind, tag, bps, bits, dtype, channels, layout):
    from rawaudiovae_kelsey_amd import _lib
    from rawaudiovae_kelsey_amd import data as D
    rng = np.random.default_rng(bps * 10 + channels)
    n = 1001                                   # odd: a u8 mono payload has an odd length (and a pad byte)
    raw, want = random_samples(kind, n, channels, rng)
    p = wav_file(tmp_path / "x.wav", raw, tag, channels, 22050, bits, bps, extensible=layout == "extensible",
                 extra=layout == "extra_chunks")
    sr, a = scipy_read(p)
    h = D.read_wav_header(p)
    assert h.format == tag and h.format in (_lib.WAV_PCM, _lib.WAV_FLOAT)
    assert (h.channels, h.rate, h.bits, h.bytes_per_sample) == (channels, sr, bits, bps)
    assert h.block_align == channels * bps and h.data_bytes == len(raw) == a.shape[0] * h.block_align
    assert a.dtype == dtype and np.array_equal(a.reshape(n, -1), want)
    with open(p, "rb") as f:
        f.seek(h.data_offset)
        assert f.read(h.data_bytes) == raw
    hh, buf = D.read_wav_payload(p, pin_memory=False)
    assert hh == h and buf.numpy().tobytes() == raw


def test_wav_header_of_scipy_written_files(tmp_path):
    from scipy.io import wavfile
    from rawaudiovae_kelsey_amd import data as D
    rng = np.random.default_rng(3)
    for dt in (np.uint8, np.int16, np.int32, np.float32, np.float64):
        for shape in ((777,), (777, 2), (777, 6)):
            a = (rng.uniform(-1, 1, shape) * (100 if dt != np.float32 and dt != np.float64 else 1)).astype(dt)
            p = tmp_path / ("s_%s_%d.wav" % (np.dtype(dt).name, len(shape) and (shape + (1,))[1]))
            wavfile.write(str(p), 48000, a)
            h = D.read_wav_header(p)
            sr, b = wavfile.read(str(p))
            assert h.rate == sr == 48000 and h.channels == (1 if b.ndim == 1 else b.shape[1])
            assert h.bytes_per_sample == b.dtype.itemsize and h.data_bytes == b.nbytes
            with open(p, "rb") as f:
                f.seek(h.data_offset)
                assert f.read(h.data_bytes) == b.tobytes()


def test_wav_header_refuses_what_the_converter_does_not_serve(tmp_path):
    from rawaudiovae_kelsey_amd import data as D
    raw = b"\x00" * 64
    cases = [dict(tag=1, bits=64, bps=8),          # int64 PCM: _to_float32 reads it, the device converter does not
             dict(tag=1, bits=40, bps=5),
             dict(tag=3, bits=16, bps=2),          # 16-bit float: scipy refuses it too
             dict(tag=2, bits=4, bps=1)]           # ADPCM
    for i, c in enumerate(cases):
        p = wav_file(tmp_path / ("bad%d.wav" % i), raw, c["tag"], 1, 8000, c["bits"], c["bps"])
        with pytest.raises(ValueError):
            D.read_wav_header(p)
    (tmp_path / "rifx.wav").write_bytes(b"RIFX" + b"\x00" * 40)
    with pytest.raises(ValueError):
        D.read_wav_header(tmp_path / "rifx.wav")
    p = tmp_path / "nodata.wav"
    p.write_bytes(b"RIFF\x1c\x00\x00\x00WAVE" + b"fmt \x10\x00\x00\x00" + struct.pack("<HHIIHH", 1, 1, 8000, 16000, 2, 16))
    with pytest.raises(ValueError):
        D.read_wav_header(p)


def _resample_sinc_hann_before_the_bank_was_factored_out(a, sr_in, sr_out, lowpass_filter_width=6, rolloff=0.99,
                                                           chunk=1 << 18):
    """`data._resample_sinc_hann` as it was before `_sinc_hann_bank` was factored out of it (frozen copy)."""
    g = math.gcd(int(sr_in), int(sr_out))
    orig, new = int(sr_in) // g, int(sr_out) // g
    if orig == new:
        return a
    base = min(orig, new) * rolloff
    width = int(math.ceil(lowpass_filter_width * orig / base))
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    t = (np.arange(0, -new, -1).astype(np.float32) / np.float32(new)).astype(np.float64)[:, None] + idx
    t *= base
    np.clip(t, -lowpass_filter_width, lowpass_filter_width, out=t)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        kernels = np.where(t == 0, 1.0, np.sin(t) / t)
    kernels = (kernels * window * (base / orig)).astype(np.float32)
    taps = kernels.shape[1]
    n = len(a)
    x = np.zeros(n + 2 * width + orig, np.float32)
    x[width:width + n] = a
    n_frames = (len(x) - taps) // orig + 1
    out = np.empty((n_frames, new), np.float32)
    kt = np.ascontiguousarray(kernels.T)
    for f0 in range(0, n_frames, chunk):
        f1 = min(n_frames, f0 + chunk)
        seg = x[f0 * orig:(f1 - 1) * orig + taps]
        frames = np.lib.stride_tricks.as_strided(seg, shape=(f1 - f0, taps), strides=(orig * seg.itemsize, seg.itemsize),
                                                 writeable=False)
        np.matmul(frames, kt, out=out[f0:f1])
    target = int(math.ceil(new * n / orig))
    return out.reshape(-1)[:target]


def test_resampler_output_unchanged_by_the_shared_filter_bank():
    from rawaudiovae_kelsey_amd import data as D
    rng = np.random.default_rng(11)
    pairs = [(48000, 44100), (44100, 48000), (22050, 44100), (32000, 44100), (44100, 16000), (96000, 44100),
             (8000, 44100), (44100, 192000), (192000, 44100), (44100, 22050)]
    for si, so in pairs:
        for n in (0, 1, 7, 2500):
            a = rng.standard_normal(n).astype(np.float32)
            y = D._resample_sinc_hann(a, si, so)
            assert y.dtype == np.float32
            assert np.array_equal(y, _resample_sinc_hann_before_the_bank_was_factored_out(a, si, so)), (si, so, n)
        orig, new, width, bank = D._sinc_hann_bank(si, so)
        g = math.gcd(si, so)
        assert (orig, new) == (si // g, so // g) and bank.shape == (new, 2 * width + orig) and bank.dtype == np.float32
    assert D._sinc_hann_bank(44100, 44100) is None
    # the sizes the device kernel must handle at the ends of the 8 k - 192 kHz range
    assert D._sinc_hann_bank(192000, 44100)[3].shape == (147, 694)
    assert D._sinc_hann_bank(44100, 192000)[3].shape == (640, 161)


def test_ingest_switch_is_checked():
    from rawaudiovae_kelsey_amd import data as D
    with pytest.raises(ValueError, match="ingest"):
        D.StreamingFrames(["a.wav"], 8000, 64, 256, "cpu", ingest="gpu")


def test_train_iterable_rejects_an_unknown_ingest(tmp_path):
    import configparser
    sys.path.insert(0, REPO)
    import train_iterable as TI
    for d in ("audio", "test_audio"):
        (tmp_path / d).mkdir()
    cfg = configparser.ConfigParser(allow_no_value=True)
    cfg.read(os.path.join(REPO, "default_iterable.ini"))
    assert cfg["mi355x"]["ingest"] == "host"
    cfg["dataset"]["datapath"] = str(tmp_path)
    cfg["mi355x"]["ingest"] = "disk"
    p = tmp_path / "run.ini"
    with open(p, "w") as f:
        cfg.write(f)
    with pytest.raises(ValueError, match="ingest"):
        TI.main(["--config", str(p)])
