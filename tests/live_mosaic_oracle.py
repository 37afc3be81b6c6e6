"""Numpy statement of live mosaicing (RV_MOSAIC_LIVE in csrc/mosaic_live.hip,
rawaudiovae_kelsey_amd.mosaic.StreamingMosaic) for the tests.

greedy: the lag-0 selection rule.  Per frame, in order, with prev = the last chosen corpus frame (-1 at the start):
prev < 0, or next_of[prev] outside [0, N): the lowest j whose candidate is a corpus row.  Otherwise the argmin over
those j of dist[t, j] + fl(w * D(mu[next_of[prev]], mu[idx[t, j]])) with D = mosaic_oracle's distance, the product
rounded before the add, strict < in ascending j, NaN costs skipped.  A row with nothing left gets slot -1, choice -1 and
prev -1.  A weight that is not finite and >= 0 counts as 0.

block_ola: k_stream_ola's blockwise overlap-add (numerator carried in a tail of S - hop samples, each product rounded
before its add, frames in ascending order; divided by the normaliser table of stream.window_norm), block after block."""
import numpy as np

import mosaic_oracle as O

f32 = np.float32


def weight_of(w):
    w = f32(w)
    return w if (np.isfinite(w) and w >= 0) else f32(0)


def greedy(idx, dist, mu, next_of, w, prev=-1):
    """(slot [T] int32, choice [T] int32, prev after the last row, cost [2] float64: the sums of the chosen dist and
    of the chosen D).  w: a scalar or one value per row."""
    idx = np.asarray(idx)
    dist = np.asarray(dist, f32)
    mu = np.asarray(mu, f32)
    N = mu.shape[0]
    T, k = idx.shape
    ws = np.broadcast_to(np.asarray(w, np.float64), (T,))
    slot = np.full(T, -1, np.int32)
    choice = np.full(T, -1, np.int32)
    cost = np.zeros(2, np.float64)
    prev = int(prev)
    for t in range(T):
        valid = (idx[t] >= 0) & (idx[t] < N)
        succ = int(next_of[prev]) if 0 <= prev < N else -1
        if not 0 <= succ < N:
            succ = -1
        s, D = -1, None
        if succ < 0:
            if valid.any():
                s = int(np.argmax(valid))
        else:
            D = O.sq_dist(mu[succ][None], mu[np.where(valid, idx[t], 0)])[0]
            with np.errstate(invalid="ignore", over="ignore"):
                c = (dist[t] + (weight_of(ws[t]) * D).astype(f32)).astype(f32)
            valid = valid & ~np.isnan(c)
            best = None
            for j in range(k):
                if valid[j] and (s < 0 or c[j] < best):
                    s, best = j, c[j]
        slot[t] = s
        choice[t] = idx[t, s] if s >= 0 else -1
        if s >= 0:
            cost[0] += np.float64(dist[t, s])
            if D is not None:
                cost[1] += np.float64(D[s])
        prev = int(choice[t])
    return slot, choice, prev, cost


def block_ola(frames, hop, block, window, norm):
    """[F * hop] fp32: the stream's output for frames [F, S] fed `block` samples (block // hop frames) at a time."""
    frames = np.asarray(frames, f32)
    F, S = frames.shape
    P, fb = S - hop, block // hop
    assert F % fb == 0
    window = np.asarray(window, f32)
    tail = np.zeros(P, f32)
    out = np.zeros(F * hop, f32)
    for b in range(F // fb):
        num = np.zeros(block + P, f32)
        num[:P] = tail
        for j in range(fb):
            sl = slice(j * hop, j * hop + S)
            num[sl] = num[sl] + (window * frames[b * fb + j]).astype(f32)
        t = b * block + np.arange(block)
        den = np.where(t < P, norm[np.minimum(t, P + hop - 1)], norm[P + t % hop])
        y = np.zeros(block, f32)
        nz = den != 0
        y[nz] = num[:block][nz] / den[nz]
        out[b * block:(b + 1) * block] = y
        tail = num[block:]
    return out
