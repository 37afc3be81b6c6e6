"""The front door of every tool and of the streaming trainer, exactly and between guards: rv_pcm_to_f32 and
rv_resample_sinc_hann (csrc/audio.hip), rv_gather_frames (csrc/elementwise.hip), rv_match_pad and rv_latent_mix
(csrc/resynth.hip) and rv_linear_fp32 (csrc/linear_fp32.hip), called through _lib on pointers cut from tests/guarded.py
buffers, at the smallest shapes that take each loop into another trip or another path.

  - every output lies between sentinel guards and is checked with assert_untouched after every call;
  - every float input lies between NaN guards (gap columns and alignment shifts included): a read outside it poisons
    the result;
  - uint8 and int64 inputs have no NaN: a payload's guards hold 0x55 bytes (a non-zero sample in every format), an
    index's guards hold valid frame numbers;
  - every comparison is one of integer views (-0 and NaN by their bits), against tests/ingest_oracle.py,
    stream_oracle.chain32 or the host decode.  Two assertions are tolerances and say so: tanh (act 2 of rv_linear_fp32)
    against float64 within TANH_TOL, and the float64 modes' z of rv_latent_mix, which passes through the device's exp,
    within one fp32 ulp of the oracle's.

The draws of rv_latent_mix (eps_in == NULL) are held to rv_randn on the same counters bit for bit, and to
rng_oracle.randn_ref within test_rng_gpu.ACC_BOUND: the oracle's Philox words and uniforms are exact, its Box-Muller
values are float64 and differ from any device's by that device's log / sqrt / sincos (tests/rng_oracle.py).

rv_resample_sinc_hann: (orig, new, width, taps) of every pair of RESAMPLE, from data._sinc_hann_bank:
    (2, 1)          2    1  13   28   one phase
    (1, 2)          1    2   7   15   two phases
    (3, 2)          3    2  10   23   fewer than 64 taps
    (64, 63)       64   63   7   78   new one below the 64-phase tile, a second tap chunk of 14
    (63, 64)       63   64   7   77   new exactly the phase tile
    (64, 65)       64   65   7   78   a second phase tile of one phase
    (30, 11)       30   11  17   64   taps exactly one chunk
    (60, 11)       60   11  34  128   taps exactly two chunks
    (19, 2)        19    2  58  135   more than 128 taps: a third chunk of 7
    (48000, 44100) 160 147   7  174   the trainer's pair: three phase tiles, three chunks
A search of the coprime pairs below 130 finds taps == 64 first at (30, 11) and taps == 128 first at (60, 11); both are
in the list.  The last tap of every bank is 0 in every phase (the window is clipped there)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ingest_oracle as IO  # noqa: E402
import rng_oracle as R  # noqa: E402
import stream_oracle as SO  # noqa: E402
from guarded import SENTINEL, guarded, guarded_flat  # noqa: E402
from test_ingest_cpu import FORMATS, random_samples, wav_file  # noqa: E402
from test_rng_gpu import ACC_BOUND  # noqa: E402
from test_stream_edges_gpu import TANH_TOL, _operand  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64, U8, I64 = torch.float32, torch.float64, torch.uint8, torch.int64
GRID = 4096 * 256                    # threads of the capped grids of rv_gather_frames, rv_match_pad and rv_latent_mix


def _L():
    from rawaudiovae_kelsey_amd import _lib
    return _lib


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, (what, "%d of %d elements differ" % (len(bad), got.size), bad[:5].tolist(),
                           got[tuple(bad[0])], want[tuple(bad[0])])


def _vec(a, dtype=F32, guard=None):
    """an input vector between NaN guards (or `guard` values)"""
    a = np.asarray(a)
    return guarded_flat(a.size, dtype, a, guard)


def _mat(a):
    return guarded(a.shape[0], a.shape[1], a.shape[1], F32, a)


def _refused(call, outs, what):
    """the call raises RvError and leaves every buffer of `outs` as it was, payload included"""
    before = [g.flat.clone() for g in outs]
    with pytest.raises(_L().RvError):
        call()
    torch.cuda.synchronize()
    for g, was in zip(outs, before):
        g.assert_untouched(what)
        assert torch.equal(g.flat.view(torch.uint8), was.view(torch.uint8)), what


# ---- rv_pcm_to_f32 ---------------------------------------------------------------------------------------------------
# thread = one 16-byte piece reading a 32-byte window (vector when it ends inside the payload, byte-wise otherwise),
# block = 256 pieces = 4096 bytes

PCM_BYTES = (31, 32, 33, 47, 48, 4095, 4096, 4097, 8192 + 5)
PCM_GUARD = 0x55


def _pcm_call(raw, tag, channels, bps, hop, n_out=None, shift=0, bps_arg=None):
    """-> (the output buffer, n, n_out) of one rv_pcm_to_f32 call on `raw` uploaded between 0x55 guards"""
    L = _L()
    nbytes = len(raw)
    n = nbytes // (channels * bps)
    padded = -(-n // hop) * hop
    n_out = padded if n_out is None else n_out
    src = _vec(np.frombuffer(raw + b"\x00" * (nbytes == 0), dtype=np.uint8), U8, guard=[PCM_GUARD])
    out = guarded_flat(max(n_out, 1), F32)
    assert src.ptr % 16 == 0
    L.lib().rv_pcm_to_f32(src.ptr + shift, nbytes, tag, channels, bps if bps_arg is None else bps_arg, hop, out.ptr,
                          n_out, L.stream_ptr())
    torch.cuda.synchronize()
    out.assert_untouched("rv_pcm_to_f32 output (%d bytes, hop %d)" % (nbytes, hop))
    return out, n, n_out


@pytest.mark.parametrize("kind,tag,bps,bits,dtype", FORMATS)
@pytest.mark.parametrize("channels", [1, 2, 6])
def test_pcm_to_f32_is_the_host_decode_between_guards(tmp_path, kind, tag, bps, bits, dtype, channels):
    from rawaudiovae_kelsey_amd import data as D
    ba = channels * bps
    rng = np.random.default_rng(1000 + 10 * bps + channels)
    # whole frames: every length rounded down to a frame (at least one), and exactly one frame
    payloads = {max(1, t // ba) * ba: 0 for t in (ba,) + PCM_BYTES}
    # a trailing partial frame: the lengths themselves where they are no multiple of the frame (1 .. ba - 1 bytes over)
    payloads.update({t: t % ba for t in PCM_BYTES if t % ba and t > ba})
    cases = [(t, extra, hop) for t, extra in sorted(payloads.items()) for hop in (1, 128)]
    cases += [(ba, 0, 8192)]                   # n = 1: 8191 zero-padding threads, 32 blocks, one piece
    if ba > 1:
        cases += [(2 * ba - 1, ba - 1, 8192)]  # the same with the longest partial frame behind it
    count = partial = 0
    for nbytes, extra, hop in cases:
        n = nbytes // ba
        raw, _ = random_samples(kind, n, channels, rng)
        assert len(raw) == n * ba == nbytes - extra
        p = wav_file(tmp_path / ("x%d_%d.wav" % (nbytes, hop)), raw, tag, channels, 16000, bits, bps)
        a, _ = D.read_wav(p)
        want = np.ascontiguousarray(a if a.ndim == 1 else a[:, 0])
        assert want.dtype == np.float32 and want.shape == (n,)
        tail = bytes(rng.integers(1, 256, extra, dtype=np.uint8))          # non-zero bytes of a frame that is not there
        out, m, n_out = _pcm_call(raw + tail, tag, channels, bps, hop)
        got = _np(out.payload()).reshape(-1)
        assert m == n and n_out == -(-n // hop) * hop == got.size
        _same_bits(got[:n], want, "%s x%d, %d bytes, hop %d" % (kind, channels, nbytes, hop))
        assert not _bits(got[n:]).any(), "the padding is +0"
        count += 1
        partial += extra > 0
    # n = 0: RV_OK, nothing launched; with no byte at all and with a partial frame alone
    for raw in (b"",) + ((b"\x7f" * (ba - 1),) if ba > 1 else ()):
        out, m, n_out = _pcm_call(raw, tag, channels, bps, 128)
        assert m == 0 and n_out == 0 and float(out.payload().view(-1)[0]) == SENTINEL
    print("rv_pcm_to_f32 %s x%d: %d payloads bit-equal to the host decode (%d with a partial frame), %d..%d bytes"
          % (kind, channels, count, partial, cases[0][0], max(c[0] for c in cases)))


@pytest.mark.parametrize("kind,tag,bps,bits,dtype", FORMATS)
def test_pcm_to_f32_refusals_leave_the_output_untouched(kind, tag, bps, bits, dtype):
    L = _L()
    channels, n, hop = 2, 40, 16
    raw = bytes(np.random.default_rng(bps).integers(1, 256, n * channels * bps, dtype=np.uint8))
    src = _vec(np.frombuffer(raw, dtype=np.uint8), U8, guard=[PCM_GUARD])
    out = guarded_flat(64, F32)

    def call(n_out=48, bps_arg=bps, shift=0):
        return lambda: L.lib().rv_pcm_to_f32(src.ptr + shift, len(raw), tag, channels, bps_arg, hop, out.ptr, n_out,
                                             L.stream_ptr())
    bad_bps = 8 if tag == L.WAV_PCM else 2
    for what, c in (("n_out one short", call(n_out=47)), ("n_out not padded", call(n_out=40)),
                    ("n_out a hop over", call(n_out=64)), ("%d-byte samples" % bad_bps, call(bps_arg=bad_bps)),
                    ("source at + 4 bytes", call(shift=4))):
        _refused(c, [out], "rv_pcm_to_f32 %s: %s" % (kind, what))
    call()()                                     # the same arguments without the fault are served
    torch.cuda.synchronize()
    assert not bool((out.payload().view(-1)[:48] == SENTINEL).any())


# ---- rv_resample_sinc_hann -------------------------------------------------------------------------------------------
# block = 32 frames x 64 phases, taps in chunks of 64; the table of the pairs is in the module doc

RESAMPLE = {(2, 1): (2, 1, 13, 28), (1, 2): (1, 2, 7, 15), (3, 2): (3, 2, 10, 23), (64, 63): (64, 63, 7, 78),
            (63, 64): (63, 64, 7, 77), (64, 65): (64, 65, 7, 78), (30, 11): (30, 11, 17, 64), (60, 11): (60, 11, 34, 128),
            (19, 2): (19, 2, 58, 135), (48000, 44100): (160, 147, 7, 174)}


def _resample_call(a, gbank, orig, new, width, n_out):
    L = _L()
    src = _vec(a)                              # n samples between NaN guards: a read at pos < 0 or pos >= n poisons
    out = guarded_flat(n_out, F32)
    L.lib().rv_resample_sinc_hann(src.ptr, a.size, gbank.ptr, orig, new, width, out.ptr, n_out, L.stream_ptr())
    torch.cuda.synchronize()
    out.assert_untouched("rv_resample_sinc_hann output (%d -> %d, n %d, n_out %d)" % (orig, new, a.size, n_out))
    return _np(out.payload()).reshape(-1)


@pytest.mark.parametrize("sr_in,sr_out", list(RESAMPLE))
def test_resampler_is_the_fma_chain_in_tap_order(sr_in, sr_out):
    from rawaudiovae_kelsey_amd import data as D
    orig, new, width, bank = D._sinc_hann_bank(sr_in, sr_out)
    taps = bank.shape[1]
    assert (orig, new, width, taps) == RESAMPLE[(sr_in, sr_out)]
    gbank = _mat(bank)
    rng = np.random.default_rng(sr_in + sr_out)
    # frames = ceil(n_out / new) of 1, 32 (a full block) and 33: n = (frames - 1) * orig + 1; then one sample, less than
    # the front padding, one input frame and a sample
    lengths = sorted({1, width, orig + 1, 31 * orig + 1, 32 * orig + 1})
    outputs = 0
    for n in lengths:
        a = rng.standard_normal(n).astype(np.float32)
        target = IO.resample_target(n, orig, new)
        sizes = [target]
        if n in (orig + 1, 31 * orig + 1):     # hop padding that reaches into a further frame (and a further block)
            sizes.append(-(-(target + new + 1) // 8) * 8)
        for n_out in sizes:
            frames = -(-n_out // new)
            if n_out == target and n in (1, 31 * orig + 1, 32 * orig + 1):
                assert frames == (n - 1) // orig + 1 and frames in (1, 32, 33)
            want = IO.resample_chain(a, orig, new, width, bank, n_out)
            got = _resample_call(a, gbank, orig, new, width, n_out)
            _same_bits(got, want, "%d -> %d, n %d, n_out %d (target %d, %d frames)" % (orig, new, n, n_out, target, frames))
            assert not _bits(got[target:]).any()
            outputs += n_out
    print("rv_resample_sinc_hann %d -> %d (width %d, %d taps): %d outputs over n in %s bit-equal to the chain"
          % (orig, new, width, taps, outputs, lengths))


# ---- rv_gather_frames ------------------------------------------------------------------------------------------------
# 4 samples per thread, one 16-byte store per thread when S % 4 == 0, scalar stores otherwise; grid capped at 4096 blocks

def _gather_call(audio, n_samples, idx, first, n, S, hop):
    L = _L()
    ga = _vec(audio[:n_samples])               # NaN at every position outside [0, n_samples)
    gi = None if idx is None else _vec(idx, I64, guard=[0, 1])
    out = guarded(n, S, S, F32)
    L.lib().rv_gather_frames(ga.ptr, n_samples, None if gi is None else gi.ptr, first, n, S, hop, out.ptr, L.stream_ptr())
    torch.cuda.synchronize()
    out.assert_untouched("rv_gather_frames output (S %d hop %d, %d frames)" % (S, hop, n))
    return _np(out.payload())


@pytest.mark.parametrize("S,hop", [(1, 1), (3, 2), (4, 4), (5, 1), (100, 100), (256, 64)])
def test_gather_frames_zero_fills_outside_the_waveform(S, hop):
    rng = np.random.default_rng(10 * S + hop)
    q = 9 + S // hop
    # q * hop samples: frame q starts exactly at the end.  One sample fewer (where hop > 1): frame q - 1 starts before the
    # end and runs past it, whatever S >= hop is
    for n_samples in (q * hop,) + ((q * hop - 1,) if hop > 1 else ()):
        audio = rng.standard_normal(n_samples).astype(np.float32)
        inside = (n_samples - S) // hop + 1    # frames that lie inside the waveform
        extra = [-1, q - 1, q, q + 1000, inside, -(S // hop) - 1, 0]
        idx = np.concatenate([rng.permutation(inside), extra]).astype(np.int64)
        want = IO.gather(audio, n_samples, idx, 0, idx.size, S, hop)
        cut = want[inside + 1]                 # frame q - 1
        assert cut[0] != 0 and (n_samples == q * hop or cut[-1] == 0)
        assert not want[inside + 2].any() and not want[inside + 3].any() and not want[inside + 5].any()
        _same_bits(_gather_call(audio, n_samples, idx, 0, idx.size, S, hop), want, "explicit index, S %d hop %d" % (S, hop))
        first, n = 2, q + 3                    # consecutive frames 2 .. q + 4: the last ones reach or pass the end
        want = IO.gather(audio, n_samples, None, first, n, S, hop)
        _same_bits(_gather_call(audio, n_samples, None, first, n, S, hop), want, "consecutive from 2, S %d hop %d" % (S, hop))
        print("rv_gather_frames S %d hop %d over %d samples: %d indexed and %d consecutive frames bit-equal"
              % (S, hop, n_samples, idx.size, n))


@pytest.mark.parametrize("S,n_frames", [(4, GRID + 3), (5, GRID // 2 + 3)])
def test_gather_frames_takes_a_second_trip(S, n_frames):
    assert n_frames * ((S + 3) // 4) > GRID
    rng = np.random.default_rng(S)
    n_samples = 41
    audio = rng.standard_normal(n_samples).astype(np.float32)
    idx = rng.integers(-S - 1, n_samples + 2, n_frames).astype(np.int64)
    want = IO.gather(audio, n_samples, idx, 0, n_frames, S, 1)
    _same_bits(_gather_call(audio, n_samples, idx, 0, n_frames, S, 1), want, "second trip, S %d" % S)
    print("rv_gather_frames S %d hop 1: %d frames (%d threads over a grid of %d) bit-equal"
          % (S, n_frames, n_frames * ((S + 3) // 4), GRID))


def test_gather_frames_refuses_an_unaligned_output():
    L = _L()
    audio = _vec(np.ones(64, dtype=np.float32))
    out = guarded_flat(64, F32)
    _refused(lambda: L.lib().rv_gather_frames(audio.ptr, 64, None, 0, 4, 8, 8, out.ptr + 4, L.stream_ptr()), [out],
             "rv_gather_frames with the output at + 4 bytes")


# ---- rv_match_pad ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_src,n_valid,n_out", [(1, 5, 8), (7, 0, 4), (1000, 2345, 2368), (1000, 700, 704),
                                                 (3, GRID + 2, GRID + 5)])
def test_match_pad_repeats_crops_and_pads(n_src, n_valid, n_out):
    L = _L()
    rng = np.random.default_rng(n_src + n_out)
    src = rng.standard_normal(n_src).astype(np.float32)
    gs = _vec(src)
    out = guarded_flat(n_out, F32)
    L.lib().rv_match_pad(gs.ptr, n_src, n_valid, out.ptr, n_out, L.stream_ptr())
    torch.cuda.synchronize()
    out.assert_untouched("rv_match_pad output")
    want = IO.match_pad(src, n_src, n_valid, n_out)
    _same_bits(_np(out.payload()).reshape(-1), want, "rv_match_pad %d %d %d" % (n_src, n_valid, n_out))
    print("rv_match_pad n_src %d n_valid %d n_out %d: bit-equal" % (n_src, n_valid, n_out))


def test_match_pad_refuses_more_valid_samples_than_outputs():
    L = _L()
    gs = _vec(np.ones(16, dtype=np.float32))
    out = guarded_flat(8, F32)
    _refused(lambda: L.lib().rv_match_pad(gs.ptr, 16, 9, out.ptr, 8, L.stream_ptr()), [out], "rv_match_pad n_valid > n_out")


# ---- rv_latent_mix ---------------------------------------------------------------------------------------------------

MODES = {"list": IO.LIST, "f32": IO.F32, "f64": IO.F64, "curve": IO.CURVE}
SEED, OFFSET = 0x9E3779B97F4A7C15, (1 << 32) + 5      # both key words and the counter's high word count


class Mix:
    """The four distributions [N, L] and one alpha vector between NaN guards; call() is one rv_latent_mix launch into
    fresh guarded outputs."""

    def __init__(self, N, L, mode, alpha, seed):
        rng = np.random.default_rng(seed)
        self.N, self.L, self.mode = N, L, MODES[mode]
        self.d = [(rng.standard_normal((N, L)) * s).astype(np.float32) for s in (1.0, 0.7, 1.3, 0.5)]
        self.alpha = np.ascontiguousarray(alpha, dtype=np.float32 if mode == "f32" else np.float64)
        self.total = self.alpha.size * N if mode == "list" else N
        self.gd = [_mat(t) for t in self.d]
        self.ga = _vec(self.alpha, F32 if mode == "f32" else F64)

    def call(self, row0, rows, eps=None, outs=True, n_alpha=None, keep=None):
        """-> dict of numpy arrays z, eps, and with outs: mu, logvar, alpha.  eps [rows, L] or None (the Philox draw).
        keep: a list that receives the guarded outputs instead (for the refusals)."""
        L_, Lw = _L(), self.L
        ge = None if eps is None else _mat(eps)
        g = dict(z=guarded(rows, Lw, Lw, F32))
        if eps is None:
            g["eps"] = guarded(rows, Lw, Lw, F32)
        if outs:
            g.update(mu=guarded(rows, Lw, Lw, F32), logvar=guarded(rows, Lw, Lw, F32), alpha=guarded_flat(rows, F64))
        p = {k: v.ptr for k, v in g.items()}
        if keep is not None:
            keep.extend(g.values())
        L_.lib().rv_latent_mix(*[t.ptr for t in self.gd], self.N, Lw, self.mode, self.ga.ptr,
                               self.alpha.size if n_alpha is None else n_alpha, row0, rows, None if ge is None else ge.ptr,
                               p.get("eps"), SEED, OFFSET, p["z"], p.get("mu"), p.get("logvar"), p.get("alpha"),
                               L_.stream_ptr())
        torch.cuda.synchronize()
        for k, v in g.items():
            v.assert_untouched("rv_latent_mix %s (rows %d + %d)" % (k, row0, rows))
        res = {k: _np(v.payload()) for k, v in g.items()}
        if "alpha" in res:
            res["alpha"] = res["alpha"].reshape(-1)
        if eps is not None:
            res["eps"] = eps
        return res


def _randn(n):
    """rv_randn(n, SEED, OFFSET) between guards, and held to the oracle's float64 values"""
    L = _L()
    g = guarded_flat(n, F32)
    L.lib().rv_randn(g.ptr, n, SEED, OFFSET, L.stream_ptr())
    torch.cuda.synchronize()
    g.assert_untouched("rv_randn")
    got = _np(g.payload()).reshape(-1)
    err = float(np.abs(got.astype(np.float64) - R.randn_ref(n, SEED, OFFSET)).max())
    assert err <= ACC_BOUND, err
    return got, err


def _reparameterize(mu, lv, eps):
    L = _L()
    gm, gl, ge = _mat(mu), _mat(lv), _mat(eps)
    z = guarded(mu.shape[0], mu.shape[1], mu.shape[1], F32)
    L.lib().rv_reparameterize(gm.ptr, gl.ptr, mu.size, ge.ptr, None, 0, 0, z.ptr, L.stream_ptr())
    torch.cuda.synchronize()
    z.assert_untouched("rv_reparameterize z")
    return _np(z.payload())


def _ordered(a):
    """fp32 bits as integers that ascend with the value: neighbours differ by one"""
    b = _bits(np.ascontiguousarray(a, dtype=np.float32)).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _check_mix(mx, philox, what, split=True):
    """Every property of one (mode, shape, alpha) under one eps source -> (elements, what was measured: a string)"""
    N, L, total = mx.N, mx.L, mx.total
    rng = np.random.default_rng(total + L)
    eps = None if philox else rng.standard_normal((total, L)).astype(np.float32)
    full = mx.call(0, total, eps)
    seen = ""
    if philox:
        draw, err = _randn(total * L)
        seen = "; max |eps - float64 Box-Muller| %.2e (bound %.2e)" % (err, ACC_BOUND)
        _same_bits(full["eps"].reshape(-1), draw, what + ": eps_out is rv_randn at the rows' flat indices")
    want = IO.latent_mix(*mx.d, mx.mode, mx.alpha, eps=full["eps"])
    for k in ("mu", "logvar", "alpha"):
        _same_bits(full[k], want[k], "%s: %s" % (what, k))
    if mx.mode in (IO.LIST, IO.F32):
        _same_bits(full["z"], _reparameterize(full["mu"], full["logvar"], full["eps"]), what + ": z is rv_reparameterize's")
        seen = "; z == rv_reparameterize" + seen
    else:
        assert not np.isnan(full["z"]).any()
        d = np.abs(_ordered(full["z"]) - _ordered(want["z"]))
        assert d.max() <= 1, (what, "z is %d fp32 ulps from the oracle's" % d.max(), np.argwhere(d > 1)[:5].tolist())
        seen = "; z within 1 fp32 ulp of the float64 oracle, %d of %d one ulp off" % (int((d == 1).sum()), d.size) + seen
    bare = mx.call(0, total, eps, outs=False)                   # mu_out, lv_out, alpha_out NULL
    _same_bits(bare["z"], full["z"], what + ": z without the optional outputs")
    _same_bits(bare["eps"], full["eps"], what + ": eps without the optional outputs")
    if split and total > 1:
        r = max(1, total * 3 // 7)
        for outs in (True, False):
            a = mx.call(0, r, None if philox else eps[:r], outs=outs)
            b = mx.call(r, total - r, None if philox else eps[r:], outs=outs)
            for k in a:
                _same_bits(np.concatenate([a[k], b[k]]), full[k], "%s: %s of rows [0, %d) + [%d, %d)" % (what, k, r, r, total))
    return total * L, seen


def _list_alphas(*a):
    """list-mode alphas; at one of them at least (float32)(1.0 - a), the stated weight, is not 1f - (float32)a"""
    a = np.array(a, dtype=np.float64)
    assert ((1.0 - a).astype(np.float32) != np.float32(1) - a.astype(np.float32)).any()
    return a


def _alpha_of(mode, N, rng, C=7):
    if mode == "list":
        return _list_alphas(0.0, 0.6, 1.0)
    if mode == "f32":
        return rng.uniform(0, 1, N).astype(np.float32)
    if mode == "f64":
        return rng.uniform(0, 1, N)
    return rng.uniform(-0.5, 1.5, C)


@pytest.mark.parametrize("philox", [False, True], ids=["eps_in", "philox"])
@pytest.mark.parametrize("N,L", [(1, 1), (37, 24), (129, 40)])
@pytest.mark.parametrize("mode", list(MODES))
def test_latent_mix_is_the_oracles_in_one_call_and_in_two(mode, N, L, philox):
    rng = np.random.default_rng(N + L)
    mx = Mix(N, L, mode, _alpha_of(mode, N, rng), seed=N * L)
    what = "%s N %d L %d %s" % (mode, N, L, "philox" if philox else "eps_in")
    n, seen = _check_mix(mx, philox, what)
    print("rv_latent_mix %s: mu, logvar, alpha%s bit-equal over %d elements%s" % (what, ", eps" if philox else "", n, seen))


@pytest.mark.parametrize("philox", [False, True], ids=["eps_in", "philox"])
@pytest.mark.parametrize("C", [2, 7])
def test_latent_mix_curve_on_and_off_the_grid(C, philox):
    rng = np.random.default_rng(C)
    y = rng.uniform(-0.5, 1.5, C)
    for N in (1, C, 2 * C - 1, 50):
        mx = Mix(N, 3, "curve", y, seed=N + C)
        n, seen = _check_mix(mx, philox, "curve C %d N %d" % (C, N))
        x = np.linspace(0, C - 1, N)
        on_grid = int((x == np.floor(x)).sum())
        print("rv_latent_mix curve C %d N %d %s: alpha bit-equal (%d of %d points on the grid)%s"
              % (C, N, "philox" if philox else "eps_in", on_grid, N, seen))
        assert on_grid >= {1: 1, C: C, 2 * C - 1: C}.get(N, 2)


@pytest.mark.parametrize("mode", list(MODES))
def test_latent_mix_takes_a_second_trip(mode):
    N, L = 4082, 257
    assert N * L > GRID
    rng = np.random.default_rng(3)
    if mode != "list":
        mx = Mix(N, L, mode, _alpha_of(mode, N, rng), seed=9)
        n, seen = _check_mix(mx, True, "%s second trip" % mode, split=False)
    else:                                      # two alphas: rows [100, 100 + N) wrap over the frames in the second trip
        mx = Mix(N, L, mode, _list_alphas(0.65, 0.85), seed=9)
        got = mx.call(100, N)
        draw, err = _randn((100 + N) * L)
        _same_bits(got["eps"].reshape(-1), draw[100 * L:], "list second trip: eps_out")
        want = IO.latent_mix(*mx.d, mx.mode, mx.alpha, row0=100, rows=N)
        for k in ("mu", "logvar", "alpha"):
            _same_bits(got[k], want[k], "list second trip: %s" % k)
        _same_bits(got["z"], _reparameterize(got["mu"], got["logvar"], got["eps"]), "list second trip: z")
        n, seen = N * L, "; z == rv_reparameterize; max |eps - float64 Box-Muller| %.2e (bound %.2e)" % (err, ACC_BOUND)
    print("rv_latent_mix %s N %d L %d (%d elements over a grid of %d): mu, logvar, alpha, eps bit-equal%s"
          % (mode, N, L, n, GRID, seen))


def test_latent_mix_refusals_leave_the_outputs_untouched():
    N, L = 9, 5
    rng = np.random.default_rng(1)
    eps = rng.standard_normal((N, L)).astype(np.float32)
    bad = {"list": [dict(n_alpha=0), dict(row0=20, rows=8)],                  # 3 alphas: 27 rows
           "f32": [dict(n_alpha=N - 1), dict(n_alpha=N + 1), dict(row0=1, rows=N)],
           "f64": [dict(n_alpha=N - 1), dict(n_alpha=N + 1), dict(row0=N, rows=1)],
           "curve": [dict(n_alpha=1), dict(n_alpha=0), dict(row0=5, rows=5)]}
    for mode, cases in bad.items():
        mx = Mix(N, L, mode, _alpha_of(mode, N, rng), seed=2)
        for over in cases:
            kw = dict(row0=0, rows=N)
            kw.update(over)
            for e in (eps[:1].repeat(kw["rows"], 0), None):
                outs = []
                with pytest.raises(_L().RvError):
                    mx.call(kw["row0"], kw["rows"], e, n_alpha=kw.get("n_alpha"), keep=outs)
                torch.cuda.synchronize()
                assert len(outs) == (4 if e is not None else 5)
                for g in outs:
                    g.assert_untouched("rv_latent_mix %s refused %s" % (mode, over))
                    assert bool((g.view == SENTINEL).all()), (mode, over)
        mx.call(0, N, eps)                     # and the mode is served without the fault


# ---- rv_linear_fp32 --------------------------------------------------------------------------------------------------
# 64 x 64 tile, K in steps of 16, four floats per staging thread: one 16-byte load when the operand's base is 16-byte
# aligned and its ld % 4 == 0 (and the four lie below K), scalar loads otherwise
# (_operand is tests/test_stream_edges_gpu.py's: rows at pitch ld, `shift` floats past an aligned base, NaN around and
# between; overlap = the flat vector whose windows at pitch ld < cols the rows are)

def _r4(k):
    return -(-k // 4) * 4


def _linear_checks(x, W, b, px, ldx, pW, ldw, gb, ldys, what):
    """acts 0, 1, 2 with and without bias into fresh outputs at every ldy -> (launches, worst tanh error)"""
    L = _L()
    (M, K), N = x.shape, W.shape[0]
    worst, launches = 0.0, 0
    for bias in (True, False):
        pre = SO.chain32(x, W, b if bias else None)
        for ldy in ldys:
            for act in (0, 1, 2):
                gy = guarded(M, N, ldy, F32)
                L.lib().rv_linear_fp32(px, ldx, pW, ldw, gb.ptr if bias else None, M, N, K, act, gy.ptr, ldy, L.stream_ptr())
                torch.cuda.synchronize()
                w = "%s ldy %d bias %d act %d" % (what, ldy, bias, act)
                gy.assert_untouched(w)
                got = _np(gy.payload())
                launches += 1
                if act == 2:
                    err = np.abs(got.astype(np.float64) - np.tanh(pre.astype(np.float64)))
                    assert not np.isnan(got).any() and err.max() <= TANH_TOL, (w, err.max())
                    worst = max(worst, float(err.max()))
                else:
                    _same_bits(got, pre if act == 0 else np.maximum(pre, np.float32(0)), w)
    return launches, worst


@pytest.mark.parametrize("M,N,K", [(1, 1, 1), (3, 5, 7), (64, 64, 16), (65, 63, 17), (33, 130, 35)])
def test_linear_fp32_is_the_chain_on_every_staging_path(M, N, K):
    rng = np.random.default_rng(100 * M + 10 * N + K)
    x = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    b = rng.uniform(-1, 1, N).astype(np.float32)
    gb = _vec(b)
    odd = K if K % 4 else K + 1
    # (ld, shift): vector eligible; off the 16-byte grid with ld % 4 == 0; ld % 4 != 0
    xs = [(_r4(K) + 4, 0), (_r4(K) + 4, 1), (odd, 0)]
    ws = sorted({(K, 0), (K + 3, 0), (K + 8, 0), (_r4(K), 0), (_r4(K), 1), (odd + 4, 0)})
    assert any(ld % 4 == 0 and s == 0 for ld, s in ws) and any(ld % 4 for ld, s in ws) and any(s for ld, s in ws)
    launches, worst = 0, 0.0
    for ldx, sx in xs:
        gx, px = _operand(x, ldx, sx)
        for ldw, sw in ws:
            gW, pW = _operand(W, ldw, sw)
            n, e = _linear_checks(x, W, b, px, ldx, pW, ldw, gb, (N, N + 5),
                                  "M %d N %d K %d ldx %d+%d ldw %d+%d" % (M, N, K, ldx, sx, ldw, sw))
            launches, worst = launches + n, max(worst, e)
    print("rv_linear_fp32 M %d N %d K %d: %d launches over %d x and %d w layouts; acts 0, 1 bit-equal to chain32, act 2 "
          "worst |y - tanh64(pre)| = %.3e, bound %.1e" % (M, N, K, launches, len(xs), len(ws), worst, TANH_TOL))


@pytest.mark.parametrize("M,N,K,ldx", [(65, 63, 17, 4), (33, 130, 35, 4), (65, 63, 17, 3), (33, 130, 35, 3)])
def test_linear_fp32_reads_overlapping_rows(M, N, K, ldx):
    rng = np.random.default_rng(M + N + K + ldx)
    v = rng.uniform(-1, 1, (M - 1) * ldx + K).astype(np.float32)
    x = np.stack([v[r * ldx:r * ldx + K] for r in range(M)])
    W = rng.uniform(-1, 1, (N, K)).astype(np.float32)
    b = rng.uniform(-1, 1, N).astype(np.float32)
    gb = _vec(b)
    launches, worst = 0, 0.0
    for sx in (0, 1):
        gx, px = _operand(x, ldx, sx, overlap=v)
        for ldw, sw in ((K, 0), (_r4(K) + 4, 0)):
            gW, pW = _operand(W, ldw, sw)
            n, e = _linear_checks(x, W, b, px, ldx, pW, ldw, gb, (N, N + 5),
                                  "overlap M %d N %d K %d ldx %d+%d ldw %d" % (M, N, K, ldx, sx, ldw))
            launches, worst = launches + n, max(worst, e)
    print("rv_linear_fp32 M %d N %d K %d with rows every %d floats: %d launches; acts 0, 1 bit-equal to chain32, act 2 "
          "worst |y - tanh64(pre)| = %.3e, bound %.1e" % (M, N, K, ldx, launches, worst, TANH_TOL))


def test_linear_fp32_refuses_short_leading_dimensions_and_an_unknown_act():
    L = _L()
    M, N, K = 9, 70, 76
    gx, gw = _mat(np.ones((M, K), dtype=np.float32)), _mat(np.ones((N, K), dtype=np.float32))
    gy = guarded(M, N, N, F32)
    for ldw, ldy, act in ((K - 1, N, 0), (K, N - 1, 0), (K, N, 3), (K, N, -1)):
        _refused(lambda: L.lib().rv_linear_fp32(gx.ptr, K, gw.ptr, ldw, None, M, N, K, act, gy.ptr, ldy, L.stream_ptr()),
                 [gy], "rv_linear_fp32 ldw %d ldy %d act %d" % (ldw, ldy, act))
