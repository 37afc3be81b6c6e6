"""Float64 restatement of the streaming resynthesis contract (rawaudiovae_kelsey_amd/stream.py) for the tests:
framing with P = S - hop zeros in front, the one-hidden-layer forward, and weighted overlap-add normalised by the
window sum.

Below that, the same contract in the fp32 arithmetic the device states (include/rawvae_hip.h, csrc/stream.hip), rounding
for rounding, in numpy alone: fma32 (one correctly rounded fp32 fused multiply-add), chain32 (rv_small_linear_f32's
k-ordered chain), frames32 (the frames of [history | block]), latent_ctl (the two roundings of the controls) and wola32
(the numerator in ascending frame order, one division by the table).  tests/test_stream_cpu.py checks them against
rational arithmetic and float64; tests/test_stream_edges_gpu.py holds the kernels to them bit for bit."""
import numpy as np

U32 = 2.0 ** -24                  # unit roundoff of fp32
TINY32 = 2.0 ** -126              # the smallest normal fp32


def frames(x, S, hop):
    """Every complete frame of Xp = [0] * (S - hop) + x: [n, S] (frame f = Xp[f hop : f hop + S])."""
    xp = np.concatenate([np.zeros(S - hop, dtype=np.float64), np.asarray(x, dtype=np.float64)])
    n = (xp.size - S) // hop + 1
    return np.stack([xp[f * hop:f * hop + S] for f in range(n)]) if n > 0 else np.zeros((0, S))


def wola(dec, w, hop, n_out):
    """Yp[t] = sum_f w[t - f hop] D_f[t - f hop] / sum_f w[t - f hop] over the frames f that cover t (0 where the
    sum of weights is 0), for t < n_out."""
    dec = np.asarray(dec, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    S = w.size
    num = np.zeros(max(n_out, dec.shape[0] * hop + S))
    den = np.zeros_like(num)
    for f in range(dec.shape[0]):
        num[f * hop:f * hop + S] += w * dec[f]
        den[f * hop:f * hop + S] += w
    num, den = num[:n_out], den[:n_out]
    out = np.zeros(n_out)
    nz = den != 0
    out[nz] = num[nz] / den[nz]
    return out


def forward(p, x, eps, scale=None, offset=None, temperature=1.0):
    """Float64 forward of frames x [n, S] with eps [n, L]: (decoded [n, S], mu, logvar).  p: name -> array."""
    g = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    h1 = np.maximum(x @ g["fc1.weight"].T + g["fc1.bias"], 0.0)
    mu = h1 @ g["fc21.weight"].T + g["fc21.bias"]
    lv = h1 @ g["fc22.weight"].T + g["fc22.bias"]
    m = mu if scale is None else mu * scale
    m = m if offset is None else m + offset
    z = m + temperature * eps * np.exp(0.5 * lv)
    h3 = np.maximum(z @ g["fc3.weight"].T + g["fc3.bias"], 0.0)
    return np.tanh(h3 @ g["fc4.weight"].T + g["fc4.bias"]), mu, lv


# ---- the device's fp32 arithmetic, rounding for rounding -------------------------------------------------------------

def gamma(n):
    """gamma_n = n u / (1 - n u), the bound of n accumulated fp32 roundings."""
    return n * U32 / (1.0 - n * U32)


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype      # a float64 handed in by mistake would be rounded silently
    return a


def assert_normal(a, what="value"):
    """No non-zero element is subnormal in fp32 (or overflowed): the inputs were drawn at order 1."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    assert np.isfinite(a).all(), "%s: not finite" % what
    assert not ((a != 0) & (a < TINY32)).any(), "%s: a subnormal intermediate" % what


def fma32(x, w, acc):
    """RN_fp32(x * w + acc) with ONE rounding, elementwise on fp32 arrays.  The product of two fp32 values is exact in
    fp64.  TwoSum gives s = RN_fp64(p + acc) and the exact error e.  Where e != 0 and s's last mantissa bit is even, s
    moves to its neighbour on e's side: that is p + acc rounded to odd at 53 bits, and 53 >= 2 * 24 + 2 makes the
    rounding of it to fp32 the correct rounding of the exact sum."""
    p = _f32(x).astype(np.float64) * _f32(w).astype(np.float64)
    a = _f32(acc).astype(np.float64)
    p, a = np.broadcast_arrays(p, a)
    s = p + a
    bb = s - p
    e = (p - (s - bb)) + (a - bb)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where((e != 0) & even, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def chain32(x, W, b=None, act=0):
    """rv_small_linear_f32's rule on x [M, K], W [N, K], b [N] or None -> [M, N] fp32: acc = +0, acc = fma32(x[m, k],
    W[n, k], acc) for k = 0 .. K-1, then one fp32 add of b[n], then max(v, 0) for act 1.  act 2 returns the
    PRE-activation (tanhf is not reproducible on the host).  Asserts that no intermediate is subnormal."""
    x, W = _f32(x), _f32(W)
    assert x.ndim == 2 and W.ndim == 2 and x.shape[1] == W.shape[1] and act in (0, 1, 2)
    acc = np.zeros((x.shape[0], W.shape[0]), dtype=np.float32)
    for k in range(x.shape[1]):
        acc = fma32(x[:, k:k + 1], W[None, :, k], acc)
        assert_normal(acc, "chain32 at k = %d" % k)
    if b is not None:
        acc = acc + _f32(b)[None, :]
        assert acc.dtype == np.float32
        assert_normal(acc, "chain32 + b")
    return np.maximum(acc, np.float32(0)) if act == 1 else acc


def frames32(history, x, S, hop):
    """The frames of one block of one stream: [history (P = S - hop samples) | x (block samples)] cut every hop ->
    (frames [block / hop, S] fp32, the next call's history: the last P samples of the concatenation)."""
    history, x = _f32(history), _f32(x)
    P = S - hop
    assert history.shape == (P,) and x.ndim == 1 and x.size % hop == 0 and x.size >= hop
    cat = np.concatenate([history, x])
    fr = np.stack([cat[j * hop:j * hop + S] for j in range(x.size // hop)])
    return fr, cat[cat.size - P:].copy()


def latent_ctl(m, sc, of):
    """mu' = f32(f32(mu * scale) + offset): two roundings, no contraction."""
    prod = np.multiply(_f32(m), _f32(sc), dtype=np.float32)
    return np.add(prod, _f32(of), dtype=np.float32)


def wola32(dec, window, norm, hop, n):
    """The first n output samples of the overlap-add of dec [nf, S] fp32 (frame f at f hop): num = +0, then
    num = f32(num + f32(w[t - f hop] * dec[f, t - f hop])) over the frames that cover t in ascending f; the result is
    num / norm[t] for t < P = S - hop and num / norm[P + t % hop] beyond, one fp32 division, 0 where the normaliser
    is 0.  window [S] and norm [P + hop] are stream.window_values / stream.window_norm."""
    dec, window, norm = _f32(dec), _f32(window), _f32(norm)
    nf, S = dec.shape
    P = S - hop
    assert window.shape == (S,) and norm.shape == (P + hop,) and n <= nf * hop
    num = np.zeros(nf * hop + S, dtype=np.float32)
    for f in range(nf):                          # position t meets its frames in ascending f
        prod = np.multiply(window, dec[f], dtype=np.float32)
        num[f * hop:f * hop + S] = np.add(num[f * hop:f * hop + S], prod, dtype=np.float32)
    t = np.arange(n)
    den = norm[np.where(t < P, t, P + t % hop)]
    out = np.zeros(n, dtype=np.float32)
    nz = den != 0
    out[nz] = np.divide(num[:n][nz], den[nz], dtype=np.float32)
    return out
