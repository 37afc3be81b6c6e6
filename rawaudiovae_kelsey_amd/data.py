"""Audio framing for the training path, device-resident.

Semantics follow the reference's datasets (`rawvae/dataset.py`):
  * `AudioDataset` (dataset.py:86-121): concatenate all training wavs, zero-pad to a multiple
    of `hop`, frame i = audio[i*hop : i*hop + S], len = N/hop - S/hop + 1, `ValueError` when
    S is not a multiple of hop; `DataLoader(shuffle=True)` draws a fresh permutation per epoch
    and keeps the ragged last batch (train.py:134).
  * `TestDataset` (dataset.py:129-160): non-overlapping frames, tail zero-padded to S.
  * `IterableAudioDataset` (dataset.py:11-84): shuffle the FILE list once per iterator, cycle
    it forever, per file take channel 0, pad to `hop`, emit hop-strided frames in order.

A Python DataLoader delivers ~0.1 M frames/s; the step consumes >15 M frames/s, so
the waveform is uploaded once and frames are gathered on the GPU (`rv_gather_frames`): frames
overlap S/hop-fold, so the unique bytes are 1/8 of the framed batch at hop 128.

wav I/O uses scipy (librosa / soundfile / torchaudio are not available here): PCM is scaled to
[-1, 1] float32; `librosa.load(sr=...)`'s mono mix-down (mean of channels) and resampling
(polyphase here, not librosa's soxr) are restated; the streaming path's `torchaudio.functional.resample` is restated from
its published algorithm (`_resample_sinc_hann`).
"""
import collections
import itertools
import random
import struct

import numpy as np
import torch

from . import _lib
from ._lib import lib, ptr, stream_ptr


def _to_float32(a):
    if a.dtype == np.float32:
        return a
    if a.dtype == np.float64:
        return a.astype(np.float32)
    if a.dtype == np.uint8:
        return (a.astype(np.float32) - 128.0) / 128.0
    if np.issubdtype(a.dtype, np.integer):
        return a.astype(np.float32) / float(2 ** (8 * a.dtype.itemsize - 1))
    raise ValueError("unsupported wav sample type %s" % a.dtype)


def read_wav(path):
    """-> (float32 [n] or [n, channels], sample_rate)."""
    from scipy.io import wavfile
    sr, a = wavfile.read(str(path))
    return _to_float32(a), int(sr)


def _resample(a, sr_in, sr_out):
    if sr_in == sr_out:
        return a
    from math import gcd
    from scipy.signal import resample_poly
    g = gcd(int(sr_in), int(sr_out))
    return resample_poly(a, sr_out // g, sr_in // g).astype(np.float32)


def _sinc_hann_bank(sr_in, sr_out, lowpass_filter_width=6, rolloff=0.99):
    """The filter bank of `_resample_sinc_hann` (torchaudio's `_get_sinc_resample_kernel`): (orig, new, width, fp32
    [new, 2 * width + orig]) with orig / new the rates over their gcd, or None at equal rates.  Evaluated in float64 and
    rounded to float32; the host convolution and the device one (`resample_sinc_hann_device`) share it."""
    import math
    g = math.gcd(int(sr_in), int(sr_out))
    orig, new = int(sr_in) // g, int(sr_out) // g
    if orig == new:
        return None
    base = min(orig, new) * rolloff
    width = int(math.ceil(lowpass_filter_width * orig / base))
    idx = np.arange(-width, width + orig, dtype=np.float64)[None, :] / orig
    # (torch divides the int64 phase indices by new_freq in float32 before they meet the float64 tap positions)
    t = (np.arange(0, -new, -1).astype(np.float32) / np.float32(new)).astype(np.float64)[:, None] + idx
    t *= base
    np.clip(t, -lowpass_filter_width, lowpass_filter_width, out=t)
    window = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    with np.errstate(divide="ignore", invalid="ignore"):
        kernels = np.where(t == 0, 1.0, np.sin(t) / t)
    kernels = (kernels * window * (base / orig)).astype(np.float32)          # [new, 2 * width + orig]
    return orig, new, width, kernels


def _resample_sinc_hann(a, sr_in, sr_out, lowpass_filter_width=6, rolloff=0.99, chunk=1 << 18):
    """`torchaudio.functional.resample(waveform, orig_freq, new_freq)` with its defaults (resampling_method
    "sinc_interp_hann", lowpass_filter_width 6, rolloff 0.99), the call of dataset.py:50-51, restated from the
    published algorithm of torchaudio 2.x (`torchaudio/functional/functional.py`: `_get_sinc_resample_kernel` +
    `_apply_sinc_resample_kernel`) -- torchaudio is not installed here, so no fixture pins this ("parity unpinned",
    DESIGN.md section 4; tests check it against the interpolation formula it implements).  With orig / new the two rates
    over their gcd: a bank of `new` Hann-windowed sinc filters of 2 * width + orig taps, cut-off rolloff * min(orig, new)
    / 2, applied with stride orig to the signal padded by (width, width + orig) zeros; output j * new + i is filter i at
    input frame j; ceil(new * n / orig) samples are kept.  The filter bank is evaluated in float64 and rounded to
    float32, the convolution runs in float32, as torchaudio's does."""
    import math
    bank = _sinc_hann_bank(sr_in, sr_out, lowpass_filter_width, rolloff)
    if bank is None:
        return a
    orig, new, width, kernels = bank
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


WavHeader = collections.namedtuple(
    "WavHeader", "format channels rate bits block_align bytes_per_sample data_offset data_bytes")
_WAVE_FORMAT_EXTENSIBLE = 0xFFFE
_GUID_TAIL = b"\x00\x00\x10\x00\x80\x00\x00\xAA\x00\x38\x9B\x71"


def read_wav_header(path):
    """Everything `rv_pcm_to_f32` needs from a WAV file, read the way `scipy.io.wavfile.read` reads it (little-endian
    RIFF; the format tag of WAVE_FORMAT_EXTENSIBLE taken from its sub-format GUID; unknown chunks skipped, with their
    pad byte).  -> WavHeader: format (_lib.WAV_PCM or _lib.WAV_FLOAT), channels, rate, bits per sample, block align,
    container bytes per sample, and offset / length in bytes of the `data` payload (cut at the end of the file).
    Files the device converter does not serve raise ValueError: other formats or containers (what scipy refuses, and
    PCM in 5- to 8-byte containers, which `_to_float32` reads as int64), RIFX / RF64, no fmt or data chunk."""
    import os
    size = os.path.getsize(str(path))
    with open(str(path), "rb") as f:
        riff = f.read(12)
        if len(riff) < 12 or riff[:4] != b"RIFF" or riff[8:12] != b"WAVE":
            raise ValueError("%s: not a little-endian RIFF WAVE file (%r)" % (path, riff[:4]))
        fmt = None
        while True:
            ch = f.read(8)
            if len(ch) < 8:
                raise ValueError("%s: no data chunk" % path)
            cid, csize = ch[:4], struct.unpack("<I", ch[4:])[0]
            start = f.tell()
            if cid == b"fmt ":
                if csize < 16:
                    raise ValueError("Binary structure of wave file is not compliant")
                body = f.read(csize)
                tag, channels, rate, byte_rate, block_align, bits = struct.unpack("<HHIIHH", body[:16])
                if tag == _WAVE_FORMAT_EXTENSIBLE and csize >= 18:
                    if struct.unpack("<H", body[16:18])[0] < 22 or len(body) < 40:
                        raise ValueError("Binary structure of wave file is not compliant")
                    guid = body[24:40]
                    if guid.endswith(_GUID_TAIL):
                        tag = struct.unpack("<I", guid[:4])[0]
                if tag not in (_lib.WAV_PCM, _lib.WAV_FLOAT):
                    raise ValueError("Unknown wave file format: 0x%X. Supported formats: PCM, IEEE_FLOAT" % tag)
                if channels < 1:
                    raise ValueError("%s: %d channels" % (path, channels))
                if tag == _lib.WAV_PCM and byte_rate != rate * block_align:
                    raise ValueError("WAV header is invalid: nAvgBytesPerSec must equal product of nSamplesPerSec and "
                                     "nBlockAlign, but file has nSamplesPerSec = %d, nBlockAlign = %d, and "
                                     "nAvgBytesPerSec = %d" % (rate, block_align, byte_rate))
                bps = block_align // channels
                if tag == _lib.WAV_FLOAT:
                    served = bits in (32, 64) and bps == bits // 8
                    kind = "floating-point"
                else:
                    served = (bits <= 8 and bps == 1) or (8 < bits <= 8 * bps and bps in (2, 3, 4))
                    kind = "integer"
                if not served:
                    raise ValueError("unsupported wav sample type: %d-bit %s data in %d-byte containers"
                                     % (bits, kind, bps))
                fmt = (tag, channels, rate, bits, block_align, bps)
            elif cid == b"data":
                if fmt is None:
                    raise ValueError("No fmt chunk before data")
                return WavHeader(*fmt, data_offset=start, data_bytes=max(0, min(csize, size - start)))
            f.seek(start + csize + (csize & 1))


def read_wav_payload(path, pin_memory=True):
    """(WavHeader, uint8 CPU tensor holding the `data` payload) -- the raw bytes, read straight into (pinned) memory."""
    h = read_wav_header(path)
    buf = torch.empty(h.data_bytes, dtype=torch.uint8, pin_memory=pin_memory)
    with open(str(path), "rb") as f:
        f.seek(h.data_offset)
        got = f.readinto(buf.numpy()) if h.data_bytes else 0
    if got != h.data_bytes:
        raise ValueError("%s: short read of the data chunk (%d of %d bytes)" % (path, got, h.data_bytes))
    return h, buf


def pcm_to_f32_device(payload, header, hop=1, stream=None):
    """`_to_float32(read_wav(path)[0])[:, 0]` on the device (rv_pcm_to_f32): payload = the `data` bytes as a uint8
    device tensor -> (fp32 channel 0 zero-padded to a multiple of `hop`, number of samples)."""
    n = payload.numel() // header.block_align
    padded = (n + hop - 1) // hop * hop
    out = torch.empty(padded, dtype=torch.float32, device=payload.device)
    lib().rv_pcm_to_f32(ptr(payload) if payload.numel() else None, payload.numel(), header.format, header.channels,
                        header.bytes_per_sample, hop, ptr(out) if padded else None, padded, stream_ptr(stream))
    return out, n


_device_banks = {}


def _device_bank(sr_in, sr_out, device):
    """`_sinc_hann_bank` uploaded once per rate pair and device: (orig, new, width, fp32 device [new, taps]) or None."""
    key = (int(sr_in), int(sr_out), str(device))
    if key not in _device_banks:
        bank = _sinc_hann_bank(sr_in, sr_out)
        _device_banks[key] = None if bank is None else bank[:3] + (torch.from_numpy(bank[3]).to(device),)
    return _device_banks[key]


def resample_sinc_hann_device(x, sr_in, sr_out, n=None, hop=1, stream=None):
    """`_resample_sinc_hann` on the device (rv_resample_sinc_hann): the first `n` samples of the fp32 device tensor x
    (default: all) -> (ceil(new * n / orig) resampled samples zero-padded to a multiple of `hop`, their count).  At
    equal rates nothing is launched and x itself is returned."""
    n = x.numel() if n is None else int(n)
    bank = _device_bank(sr_in, sr_out, x.device)
    if bank is None:
        return x, n
    orig, new, width, b = bank
    target = (new * n + orig - 1) // orig
    padded = (target + hop - 1) // hop * hop
    out = torch.empty(padded, dtype=torch.float32, device=x.device)
    lib().rv_resample_sinc_hann(ptr(x) if n else None, n, ptr(b), orig, new, width, ptr(out) if padded else None,
                                padded, stream_ptr(stream))
    return out, target


def load_audio_mono(path, sampling_rate):
    """`librosa.load(path, sr=sampling_rate)` (train.py:120): mono float32 at `sampling_rate`."""
    a, sr = read_wav(path)
    if a.ndim == 2:
        a = a.mean(axis=1).astype(np.float32)
    return _resample(a, sr, sampling_rate)


def load_audio_ch0(path, sampling_rate):
    """`torchaudio.load` + first channel only (dataset.py:47-58)."""
    a, sr = read_wav(path)
    if a.ndim == 2:
        a = np.ascontiguousarray(a[:, 0])
    return _resample_sinc_hann(a, sr, sampling_rate)


def write_wav(path, samples, sampling_rate):
    """`soundfile.write(path, samples, sr)` stand-in: float32 wav."""
    from scipy.io import wavfile
    wavfile.write(str(path), int(sampling_rate), np.asarray(samples, dtype=np.float32))


def frame_count(n_samples, segment_length, hop):
    """(number of frames, padded length) of AudioDataset (dataset.py:99-104,121)."""
    if segment_length % hop != 0:
        raise ValueError("segment_length {} is not a multiple of hop_size {}".format(segment_length, hop))
    padded = n_samples if n_samples % hop == 0 else n_samples + hop - n_samples % hop
    return padded // hop - segment_length // hop + 1, padded


class DeviceAudio:
    """AudioDataset with the waveform resident in HBM and frames gathered on the device."""

    def __init__(self, audio_np, segment_length, hop_size, device="cuda"):
        self.segment_length, self.hop_size = int(segment_length), int(hop_size)
        self.n_frames, self.padded = frame_count(len(audio_np), self.segment_length, self.hop_size)
        self.device = torch.device(device)
        buf = np.zeros(self.padded, dtype=np.float32)
        buf[:len(audio_np)] = audio_np
        self.audio = torch.from_numpy(buf).to(self.device)
        self._cast_bf16()

    def _cast_bf16(self):
        # The same waveform as bf16, cast ONCE here (round to nearest even: what the per-batch cast kernel did to every
        # frame), followed by zeros: fc1's GEMM stages its operand tiles straight from it (rv_linear_fwd_frames), and a
        # frame's padded tail (segment length rounded up to the tile grid) reads past the last sample.
        slack = (self.segment_length + 127) // 128 * 128 + 8
        self.audio_bf16 = torch.zeros(self.padded + slack, dtype=torch.bfloat16, device=self.device)
        self.audio_bf16[:self.padded].copy_(self.audio)

    @classmethod
    def from_device(cls, audio, n_samples, segment_length, hop_size):
        """The same object from a waveform already on the device: `audio` = n_samples samples zero-padded to a multiple
        of hop_size (what pcm_to_f32_device / resample_sinc_hann_device return).  The bf16 copy is cast on the current
        stream."""
        self = cls.__new__(cls)
        self.segment_length, self.hop_size = int(segment_length), int(hop_size)
        self.n_frames, self.padded = frame_count(int(n_samples), self.segment_length, self.hop_size)
        if audio.numel() != self.padded:
            raise ValueError("waveform of %d samples, expected %d" % (audio.numel(), self.padded))
        self.device = audio.device
        self.audio = audio
        self._cast_bf16()
        return self

    def __len__(self):
        return max(self.n_frames, 0)

    def num_batches(self, batch_size):
        return (len(self) + batch_size - 1) // batch_size

    def _perm(self, n, shuffle, generator):
        """The epoch's frame order (DataLoader(shuffle=True) draws a fresh permutation per epoch, train.py:134).
        Drawn ON THE DEVICE unless a CPU generator is passed: torch's CPU randperm takes ~50 ms for 2e5 frames,
        several epochs' worth of training steps."""
        if not shuffle:
            return torch.arange(n, device=self.device)
        if generator is not None and generator.device.type == "cpu":
            return torch.randperm(n, generator=generator).to(self.device)
        return torch.randperm(n, device=self.device, generator=generator)

    def gather(self, index, out=None, stream=None):
        """index: int64 device tensor of frame numbers -> fp32 [len(index), S]."""
        n = index.numel()
        if out is None:
            out = torch.empty((n, self.segment_length), dtype=torch.float32, device=self.device)
        lib().rv_gather_frames(ptr(self.audio), self.padded, ptr(index), 0, n, self.segment_length,
                               self.hop_size, ptr(out), stream_ptr(stream))
        return out

    def frames(self, first, n, out=None, stream=None):
        """n consecutive frames starting at frame `first`."""
        if out is None:
            out = torch.empty((n, self.segment_length), dtype=torch.float32, device=self.device)
        lib().rv_gather_frames(ptr(self.audio), self.padded, None, first, n, self.segment_length,
                               self.hop_size, ptr(out), stream_ptr(stream))
        return out

    def batches(self, batch_size, shuffle=True, generator=None):
        """One epoch: DataLoader(dataset, batch_size, shuffle) -- fresh permutation, ragged last batch kept."""
        n = len(self)
        perm = self._perm(n, shuffle, generator)
        for lo in range(0, n, batch_size):
            yield self.gather(perm[lo:lo + batch_size])


    def index_batches(self, batch_size, shuffle=True, generator=None):
        """One epoch as device int64 index tensors (what `batches` gathers): for `TrainEngine.step_frames`, which
        reads the frames where the waveform lives instead of from a gathered copy."""
        n = len(self)
        perm = self._perm(n, shuffle, generator)
        for lo in range(0, n, batch_size):
            yield perm[lo:lo + batch_size].contiguous()

    def sharded_batches(self, batch_size, rank, world, shuffle=True, generator=None):
        """One data-parallel epoch.  The epoch's permutation (the same `generator` state on every rank) is
        cut into global batches of world * batch_size frames and rank r takes the r-th slice of each; the
        ragged tail is split evenly, because every rank must step with the same batch size for the mean of
        rank gradients to be the global-batch gradient (up to world - 1 frames of an epoch are left out)."""
        n = len(self)
        perm = self._perm(n, shuffle, generator)
        gb = world * batch_size
        full = n // gb
        for i in range(full):
            lo = i * gb + rank * batch_size
            yield self.gather(perm[lo:lo + batch_size])
        tail = (n - full * gb) // world
        if tail:
            lo = full * gb + rank * tail
            yield self.gather(perm[lo:lo + tail])


class DeviceEvalAudio(DeviceAudio):
    """TestDataset: non-overlapping frames, tail zero-padded to a whole frame."""

    def __init__(self, audio_np, segment_length, device="cuda"):
        n = len(audio_np)
        pad = n if n % segment_length == 0 else n + segment_length - n % segment_length
        a = np.zeros(pad, dtype=np.float32)
        a[:n] = audio_np
        super().__init__(a, segment_length, segment_length, device)

    def batches(self, batch_size, shuffle=False, generator=None):
        return super().batches(batch_size, shuffle=False)


class _Lookahead:
    """An iterator whose next items can be looked at without taking them."""

    def __init__(self, it):
        self._it, self._buf = it, collections.deque()

    def __iter__(self):
        return self

    def __next__(self):
        return self._buf.popleft() if self._buf else next(self._it)

    def peek(self, k):
        while len(self._buf) < k:
            self._buf.append(next(self._it))
        return list(self._buf)[:k]


class _DeviceIngest:
    """StreamingFrames(ingest="device"): a background thread reads each file's `data` payload into pinned memory (no
    host decode); on the calling thread the bytes are copied to the device on a dedicated ingest stream, converted
    (rv_pcm_to_f32) and resampled (rv_resample_sinc_hann) there, and an event marks the file's DeviceAudio ready.  At
    most `depth` files are in flight; the consumer's stream waits for the event, the host never synchronises."""

    def __init__(self, sampling_rate, hop_size, segment_length, device, depth=2):
        from concurrent.futures import ThreadPoolExecutor
        self.sampling_rate, self.hop_size, self.segment_length = sampling_rate, hop_size, segment_length
        self.device, self.depth = device, depth
        self.stream = torch.cuda.Stream(device)
        self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="wav-ingest")
        self._pending = collections.OrderedDict()   # file -> [future of (header, pinned bytes), (DeviceAudio, event)]

    def retain(self, files):
        """Forget files in flight that are no longer among the next ones (a new iterator drew another order)."""
        for f in [f for f in self._pending if f not in files]:
            del self._pending[f]

    def submit(self, f):
        """Start reading `f` unless it is already in flight or `depth` files are."""
        if f not in self._pending and len(self._pending) < self.depth:
            self._pending[f] = [self._pool.submit(read_wav_payload, f), None]

    def poll(self):
        """Enqueue the device work of every file whose bytes have arrived."""
        for entry in self._pending.values():
            if entry[1] is None and entry[0].done():
                self._launch(entry)

    def _launch(self, entry):
        header, host = entry[0].result()
        entry[0] = None
        with torch.cuda.stream(self.stream):
            payload = torch.empty(host.numel(), dtype=torch.uint8, device=self.device)
            payload.copy_(host, non_blocking=True)   # the host allocator keeps `host` until this copy has run
            if header.rate == self.sampling_rate:
                audio, n = pcm_to_f32_device(payload, header, self.hop_size)
            else:
                pcm, n_in = pcm_to_f32_device(payload, header)
                audio, n = resample_sinc_hann_device(pcm, header.rate, self.sampling_rate, n_in, self.hop_size)
            d = DeviceAudio.from_device(audio, n, self.segment_length, self.hop_size)
            ready = torch.cuda.Event()
            ready.record(self.stream)
        entry[1] = (d, ready)

    def take(self, f):
        """f's DeviceAudio, ordered before the current stream's next work (read now if it was not prefetched)."""
        self.submit(f)
        entry = self._pending.pop(f, None)
        if entry is None:            # `depth` other files in flight: read this one first anyway
            entry = [self._pool.submit(read_wav_payload, f), None]
        if entry[1] is None:
            self._launch(entry)
        d, ready = entry[1]
        consumer = torch.cuda.current_stream(self.device)
        consumer.wait_event(ready)
        # the buffers were allocated on the ingest stream: their memory must not be reused before the consumer's work
        d.audio.record_stream(consumer)
        d.audio_bf16.record_stream(consumer)
        return d


class StreamingFrames:
    """IterableAudioDataset + DataLoader(batch_size, shuffle=False) + islice: an endless stream of
    fixed-size batches of hop-strided 1024-sample... `segment_length`-sample frames, file order
    shuffled once per iterator (dataset.py:38-42,77-84).  Each file's waveform is uploaded once
    and cached on the device; a batch that straddles a file boundary is gathered in two pieces.

    ingest="host" (default) decodes and resamples each file on the host (load_audio_ch0); ingest="device" reads the
    raw WAV payload in a background thread and converts / resamples it on the GPU (_DeviceIngest), prefetching the
    next files of the drawn order while the current one trains.  Both give the same batches (bit-identical at the
    target rate; resampled files agree to fp32 summation order)."""

    def __init__(self, files, sampling_rate, hop_size, segment_length, device="cuda", shuffle=True, seed=None,
                 cache_bytes=8 << 30, ingest="host"):
        self.files = list(files)
        if not self.files:
            raise FileNotFoundError("no .wav files to stream")
        self.sampling_rate, self.hop_size, self.segment_length = int(sampling_rate), int(hop_size), int(segment_length)
        self.device = torch.device(device)
        self.shuffle = shuffle
        self._rng = random.Random(seed)
        # decoded waveforms kept on the device, least recently used first out once `cache_bytes` is exceeded
        # (the reference streams files lazily, dataset.py:44-75; a corpus larger than HBM must not pile up here)
        self._cache, self._cache_bytes, self.cache_limit = {}, 0, int(cache_bytes)
        if ingest not in ("host", "device"):
            raise ValueError("ingest = %r (expected 'host' or 'device')" % (ingest,))
        self.ingest = ingest
        self._ingest = None
        if ingest == "device":
            self._ingest = _DeviceIngest(self.sampling_rate, self.hop_size, self.segment_length, self.device)

    def _dataset(self, f):
        d = self._cache.pop(f, None)
        if d is None:
            if self._ingest is not None:
                d = self._ingest.take(f)
            else:
                d = DeviceAudio(load_audio_ch0(f, self.sampling_rate), self.segment_length, self.hop_size, self.device)
            self._cache_bytes += d.audio.numel() * 4
            while self._cache and self._cache_bytes > self.cache_limit:
                old = self._cache.pop(next(iter(self._cache)))
                self._cache_bytes -= old.audio.numel() * 4
        self._cache[f] = d   # most recently used last
        return d

    def batches(self, batch_size, n_batches):
        order = self._rng.sample(self.files, len(self.files)) if self.shuffle else list(self.files)
        stream = itertools.cycle(order)
        if self._ingest is not None:
            stream = _Lookahead(stream)
        cur, pos = None, 0
        empty_run = 0   # consecutive files without a single full frame
        for _ in range(n_batches):
            if self._ingest is not None:
                self._ingest.poll()
            out = torch.empty((batch_size, self.segment_length), dtype=torch.float32, device=self.device)
            filled = 0
            while filled < batch_size:
                if cur is None or pos >= len(cur):
                    cur, pos = self._dataset(next(stream)), 0
                    if self._ingest is not None:
                        self._prefetch(stream.peek(self._ingest.depth))
                    if len(cur) <= 0:
                        cur = None
                        empty_run += 1
                        if empty_run >= len(order):
                            raise ValueError("no file yields a full %d-sample frame" % self.segment_length)
                        continue
                    empty_run = 0
                take = min(batch_size - filled, len(cur) - pos)
                cur.frames(pos, take, out=out[filled:filled + take])
                filled += take
                pos += take
            yield out

    def _prefetch(self, upcoming):
        """Start reading the next files of the drawn order that are not cached (at most two in flight)."""
        self._ingest.retain(upcoming)
        for f in upcoming:
            if f not in self._cache:
                self._ingest.submit(f)
        self._ingest.poll()
