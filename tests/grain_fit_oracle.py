"""Numpy restatement of grain fitting (RV_GRAIN_FIT / RV_GRAIN_GATHER in csrc/grain.hip, fit_grains / gather_fitted in
rawaudiovae_kelsey_amd/mosaic.py) for the tests.  The rule is the one of include/rawvae_hip.h, "Grain fitting":

fit: per (target frame t, candidate j) and every permitted shift, c = fmaf(x[n], g[n], c) and e = fmaf(g[n], g[n], e) in
fp32, one ascending chain over n from +0 each; score = c^2 / e in float64 when c > 0, e > 0 and both are finite, else 0;
the shift of greatest score, ties to the smaller |shift|, then to the negative one; gain 1 at gain_max 0, otherwise
min(fl32(c / e), gain_max) where the score is > 0, else 0.
gather: (1/k) sum_j fl(gain * grain) in ascending j from +0, each product rounded before its add."""
import numpy as np


def _fma(a, b, acc):
    """fmaf(a, b, acc) elementwise for fp32 arrays, mosaic_oracle._fma_sq's way: a * b is exact in float64, the
    float64 sum is corrected by its rounding error where it lands on an fp32 midpoint (the only case where rounding
    twice differs from rounding once)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    z = acc.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + z
        bp = s - p
        err = (p - (s - bp)) + (z - bp)
        r = s.astype(np.float32)
        rd = r.astype(np.float64)
        lo = np.where(rd < s, r, np.nextafter(r, np.float32(-np.inf)))
        hi = np.where(rd > s, r, np.nextafter(r, np.float32(np.inf)))
        mid = (rd != s) & np.isfinite(s) & (lo.astype(np.float64) + hi.astype(np.float64) == 2.0 * s) & (err != 0)
        return np.where(mid, np.where(err > 0, hi, lo), r).astype(np.float32)


def shift_room(lengths, S, hop=None):
    """room [N, 2]: samples each frame's start may move back / forward inside its file's padded waveform (hop=None:
    files padded to whole frames, frames every S; an int: padded to a multiple of hop, frames every hop)."""
    rows = []
    for n in lengths:
        if hop is None:
            padded, step = -(-n // S) * S, S
            frames = padded // S
        else:
            padded, step = -(-n // hop) * hop, hop
            frames = padded // hop - S // hop + 1
        for p in range(max(frames, 0)):
            rows.append((p * step, padded - S - p * step))
    return np.array(rows, np.int32).reshape(-1, 2)


def correlations(target, hop, S, idx, src, row_start, room, R):
    """(c, e, ok), each [T, k, 2R + 1] over the shifts -R .. R: the two fp32 sums and whether the shift is permitted
    (ok is all False for a candidate outside [0, N) or whose unshifted grain is not inside src)."""
    target = np.asarray(target, np.float32)
    src = np.asarray(src, np.float32)
    idx = np.asarray(idx).astype(np.int64)
    row_start = np.asarray(row_start, np.int64)
    room = np.asarray(room, np.int64)
    T, k = idx.shape
    N = row_start.size
    valid = (idx >= 0) & (idx < N)
    ii = np.where(valid, idx, 0)
    st = row_start[ii]
    valid &= (st >= 0) & (st + S <= src.size)
    delta = np.arange(-R, R + 1, dtype=np.int64)
    back = np.minimum(np.maximum(room[ii, 0], 0), st)                       # never outside src either
    fwd = np.minimum(np.maximum(room[ii, 1], 0), src.size - S - st)
    ok = valid[..., None] & (delta >= -np.minimum(R, back)[..., None]) & (delta <= np.minimum(R, fwd)[..., None])
    start = np.where(ok, st[..., None] + delta, 0)
    c = np.zeros((T, k, delta.size), np.float32)
    e = np.zeros_like(c)
    frame0 = np.arange(T, dtype=np.int64) * hop
    for n in range(S):
        g = src[start + n]
        x = np.broadcast_to(target[frame0 + n][:, None, None], g.shape)
        c = _fma(x, g, c)
        e = _fma(g, g, e)
    return c, e, ok


def fit(target, hop, S, idx, src, row_start, room, R, gain_max):
    """(shift [T, k] int32, gain [T, k] fp32, score [T, k] fp64) of the rule."""
    c, e, ok = correlations(target, hop, S, idx, src, row_start, room, R)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        pos = ok & (c > 0) & (e > 0) & np.isfinite(c) & np.isfinite(e)
        c64, e64 = c.astype(np.float64), e.astype(np.float64)
        score = np.where(pos, c64 * c64 / np.where(pos, e64, 1.0), 0.0)
        ratio = (c64 / np.where(pos, e64, 1.0)).astype(np.float32)
    delta = np.arange(-R, R + 1)
    # first in (score descending, |delta|, delta) among the permitted shifts; -1 sorts an unpermitted shift last
    key = np.where(ok, score, -1.0)
    order = np.lexsort((np.broadcast_to(delta, key.shape), np.broadcast_to(np.abs(delta), key.shape), -key), axis=-1)
    first = order[..., :1]
    best = np.take_along_axis(score, first, -1)[..., 0]
    any_ok = ok.any(-1)
    shift = np.where(any_ok, delta[first[..., 0]], 0).astype(np.int32)
    best = np.where(any_ok, best, 0.0)
    if gain_max == 0:
        gain = np.where(any_ok, np.float32(1), np.float32(0))
    else:
        r = np.take_along_axis(ratio, first, -1)[..., 0]
        gain = np.where(any_ok & (best > 0), np.minimum(r, np.float32(gain_max)), np.float32(0))
    return shift, gain.astype(np.float32), best.astype(np.float64)


def gather(src, row_start, idx, shift, gain, width):
    """[T, width] fp32: (1/k) sum_j fl(gain[t, j] * src[row_start[idx[t, j]] + shift[t, j] : + width]) in ascending j
    from +0; a candidate outside [0, N) or a grain that would leave src adds nothing."""
    src = np.asarray(src, np.float32)
    idx = np.asarray(idx).astype(np.int64)
    row_start = np.asarray(row_start, np.int64)
    shift = np.asarray(shift).astype(np.int64)
    gain = np.asarray(gain, np.float32)
    T, k = idx.shape
    acc = np.zeros((T, width), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(k):
            i = idx[:, j]
            ok = (i >= 0) & (i < row_start.size)
            st = row_start[np.where(ok, i, 0)] + shift[:, j]
            ok &= (st >= 0) & (st + width <= src.size)
            rows = src[np.where(ok, st, 0)[:, None] + np.arange(width)[None, :]]
            prod = (gain[:, j][:, None] * rows).astype(np.float32)
            acc = np.where(ok[:, None], acc + prod, acc).astype(np.float32)
        return (acc * (np.float32(1.0) / np.float32(k))).astype(np.float32)
