"""Plain restatements of the ingest, framing and interpolation kernels' rules (csrc/audio.hip: rv_resample_sinc_hann;
csrc/elementwise.hip: rv_gather_frames; csrc/resynth.hip: rv_match_pad, rv_latent_mix), rounding for rounding, in numpy
alone.  tests/test_ingest_oracle_cpu.py checks them against the host resampler, oracle.vae_oracle, scipy and torch-CPU;
tests/test_ingest_edges_gpu.py holds the kernels to them bit for bit.

rv_pcm_to_f32 has no entry here: its rule is the host decode (data.read_wav), which the tests call.  rv_linear_fp32's
rule is stream_oracle.chain32."""
import numpy as np

from stream_oracle import assert_normal, fma32

LIST, F32, F64, CURVE = 0, 1, 2, 3          # RV_ALPHA_* (include/rawvae_hip.h)


def resample_target(n, orig, new):
    """ceil(new * n / orig): the outputs rv_resample_sinc_hann keeps of n input samples"""
    return (new * n + orig - 1) // orig


def resample_chain(a, orig, new, width, bank, n_out=None):
    """The resampler's stated rule on a [n] fp32 with bank [new, taps = 2 width + orig] fp32: for every output
    m = j new + i < target = ceil(new n / orig), acc = +0, then acc = fma32(bank[i, k], xp[j orig + k], acc) for
    k = 0 .. taps - 1 ascending, xp = a with `width` zeros in front and zeros after.  Outputs [target, n_out) are +0
    (n_out defaults to target).  Asserts that no intermediate is subnormal."""
    a, bank = np.asarray(a), np.asarray(bank)
    assert a.dtype == np.float32 and bank.dtype == np.float32 and a.ndim == 1
    taps = 2 * width + orig
    assert bank.shape == (new, taps), (bank.shape, new, taps)
    n = a.size
    target = resample_target(n, orig, new)
    n_out = target if n_out is None else n_out
    assert n_out >= target
    frames = -(-target // new)
    xp = np.zeros(max(frames - 1, 0) * orig + taps + width + n, dtype=np.float32)
    xp[width:width + n] = a
    acc = np.zeros((frames, new), dtype=np.float32)
    j = np.arange(frames) * orig
    for k in range(taps):
        acc = fma32(bank[None, :, k], xp[j + k][:, None], acc)
        assert_normal(acc, "resample_chain at tap %d" % k)
    out = np.zeros(n_out, dtype=np.float32)
    out[:target] = acc.reshape(-1)[:target]
    return out


def gather(audio, n_samples, idx, first, n, S, hop):
    """rv_gather_frames: frame f = samples (idx[f] or first + f) * hop + [0, S) of audio[:n_samples], +0 at every
    position outside [0, n_samples) -> [n, S] fp32"""
    audio = np.asarray(audio)
    assert audio.dtype == np.float32 and audio.size >= n_samples
    f = first + np.arange(n, dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64)
    assert f.shape == (n,)
    pos = f[:, None] * hop + np.arange(S, dtype=np.int64)[None, :]
    inside = (pos >= 0) & (pos < n_samples)
    return np.where(inside, audio[np.where(inside, pos, 0)], np.float32(0))


def match_pad(src, n_src, n_valid, n_out):
    """rv_match_pad: src[i % n_src] for i < n_valid, +0 for n_valid <= i < n_out"""
    return np.concatenate([np.asarray(src)[np.arange(n_valid) % max(n_src, 1)], np.zeros(n_out - n_valid, np.float32)])


def curve_alpha(y, N):
    """scipy.interpolate.interp1d(arange(C), y)(numpy.linspace(0, C - 1, N)) as the kernel's curve_alpha forms it:
    x = n * ((C - 1) / (N - 1)) + 0 with the last point exactly C - 1 (0 when N == 1); j = floor(x) capped at C - 1; y[j]
    itself where x == j, else (y[j + 1] - y[j]) * (x - j) + y[j].  Every operation is one float64 rounding."""
    y = np.asarray(y)
    assert y.dtype == np.float64 and y.ndim == 1 and y.size >= 2
    C = y.size
    if N == 1:
        x = np.zeros(1)
    else:
        step = np.float64(C - 1) / np.float64(N - 1)
        x = np.arange(N).astype(np.float64) * step + 0.0
        x[N - 1] = np.float64(C - 1)
    j = np.minimum(np.floor(x).astype(np.int64), C - 1)
    on_grid = x == j.astype(np.float64)
    slope = y[np.minimum(j + 1, C - 1)] - y[j]
    return np.where(on_grid, y[j], slope * (x - j.astype(np.float64)) + y[j])


def latent_mix(mu_a, lv_a, mu_b, lv_b, mode, alpha, eps=None, row0=0, rows=None):
    """rv_latent_mix on mu_a, lv_a, mu_b, lv_b [N, L] fp32 for output rows [row0, row0 + rows) (default: to the end) ->
    dict(mu, logvar [rows, L] fp32, alpha [rows] float64, z).  Output row r reads frame r % N and alpha[r / N] in LIST
    mode (K alphas: K N rows), frame r and its own alpha otherwise.

      LIST   alpha [K] float64: weights ((float32)(1.0 - a), (float32)a); alpha out is the fp32 weight of b as float64
      F32    alpha [N] fp32:    weights (1f - a, a)
        mu = f32(f32(mu_a wa) + f32(mu_b wb)), logvar likewise: two rounded products, one rounded add.  z is None (the
        device's z goes through its fp32 exp; the tests hold it to rv_reparameterize on the returned mu, logvar, eps)
      F64    alpha [N] float64; CURVE alpha = the control points [C] float64, stretched by curve_alpha
        the same in float64 with weights (1.0 - a, a), mu and logvar returned rounded to fp32, and
        z = float32(m + e * exp(0.5 lv)) on the unrounded float64 m, lv with eps [rows, L] fp32 (None: z is None)"""
    t = [np.asarray(x) for x in (mu_a, lv_a, mu_b, lv_b)]
    assert all(x.dtype == np.float32 and x.shape == t[0].shape and x.ndim == 2 for x in t)
    N, L = t[0].shape
    alpha = np.asarray(alpha)
    assert alpha.ndim == 1 and alpha.dtype == (np.float32 if mode == F32 else np.float64)
    total = alpha.size * N if mode == LIST else N
    assert mode in (LIST, CURVE) or alpha.size == N
    rows = total - row0 if rows is None else rows
    assert 0 <= row0 and row0 + rows <= total
    r = row0 + np.arange(rows)
    n = r % N if mode == LIST else r
    ma, la, mb, lb = (x[n] for x in t)
    if mode in (LIST, F32):
        if mode == LIST:
            a64 = alpha[r // N]
            wa, wb = (1.0 - a64).astype(np.float32), a64.astype(np.float32)
        else:
            wb = alpha[n]
            wa = np.subtract(np.float32(1), wb, dtype=np.float32)

        def mix(a, b):
            pa = np.multiply(a, wa[:, None], dtype=np.float32)
            pb = np.multiply(b, wb[:, None], dtype=np.float32)
            return np.add(pa, pb, dtype=np.float32)
        return dict(mu=mix(ma, mb), logvar=mix(la, lb), alpha=wb.astype(np.float64), z=None)
    a = curve_alpha(alpha, N)[n] if mode == CURVE else alpha[n]
    wa = 1.0 - a

    def mix64(x, y):
        return x.astype(np.float64) * wa[:, None] + y.astype(np.float64) * a[:, None]
    m, lv = mix64(ma, mb), mix64(la, lb)
    z = None
    if eps is not None:
        eps = np.asarray(eps)
        assert eps.dtype == np.float32 and eps.shape == (rows, L)
        z = (m + eps.astype(np.float64) * np.exp(0.5 * lv)).astype(np.float32)
    return dict(mu=m.astype(np.float32), logvar=lv.astype(np.float32), alpha=a, z=z)
