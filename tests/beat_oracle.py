"""Float64 restatement of the three beat rules of include/rawvae_hip.h, "Latent beats" (csrc/beat.hip,
rawaudiovae_kelsey_amd/beats.py), and nothing else: the onset curve of a novelty curve, the windowed autocorrelation with
the periods it prefers, and the dynamic-programming beat tracker, each in the header's summation order with a separate
multiply and add per term.

A skipped term is added as +0 where that is bit-neutral (a chain that starts at +0 never holds -0); where the skipped
operand could be NaN it is masked first.  track_blocks is the tracker evaluated the way the kernel runs it: every block of
dlo frames from a frozen copy of C, the frames of a block in descending order, so that a frame that read a value of its
own block would read 0 and differ."""
import math

import numpy as np

ROWS = 256      # the blocks of the sum of squares: RV_EVAL_DIMS's
TILE = 64       # values of i in one chain of the autocorrelation


def onset(nov):
    """(o [T] fp64, summary [4] int32, cost [2] fp64) of RV_BEAT_ONSET."""
    nov = np.asarray(nov, np.float64)
    T = nov.size
    fin = np.isfinite(nov)
    pos = fin & (nov > 0)
    h = np.where(pos, nov, 0.0)
    q = 0.0
    for b0 in range(0, T, ROWS):
        part = 0.0
        for x in h[b0:b0 + ROWS]:
            x = float(x)
            part = part + x * x
        q = q + part
    s = math.sqrt(q / T) if q < math.inf else math.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        o = h / s if s > 0 else np.zeros(T)
    return o, np.array([pos.sum(), fin.sum(), 0, 0], np.int32), np.array([s, 0.0])


def prefer(score, lo):
    """The lag of the largest finite score > 0, ties to the smaller lag; 0 when there is none."""
    ok = np.isfinite(score) & (score > 0)
    if not ok.any():
        return 0
    return lo + int(np.argmax(np.where(ok, score, -np.inf)))        # the first of equal maxima


def tempogram(o, Wn, Hw, lo, hi, win, prior):
    """(A [nW, hi - lo + 1], G, period [nW] int32, info [4] int32, cost [2]) of RV_BEAT_TEMPOGRAM."""
    o, win, prior = (np.asarray(a, np.float64) for a in (o, win, prior))
    T, nlag = o.size, hi - lo + 1
    assert win.shape == (Wn,) and prior.shape == (nlag,)
    nW = -(-T // Hw)
    op = np.concatenate([o, np.zeros(nW * Hw + Wn + hi)])
    taus = np.arange(lo, hi + 1)
    a0 = np.arange(nW) * Hw
    A = np.zeros((nW, nlag))
    tile = np.zeros((nW, nlag))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(Wn):
            a = a0 + i
            second = a[:, None] + taus[None, :]
            p = op[a][:, None] * op[second]
            term = win[i] * p
            tile = tile + np.where(second < T, term, 0.0)
            if i % TILE == TILE - 1 or i == Wn - 1:
                A = A + tile
                tile = np.zeros((nW, nlag))
        G = np.zeros(nlag)
        for n in range(nW):
            G = G + A[n]
        score = prior * G
        P = prefer(score, lo)
        period = np.array([prefer(prior * A[n], lo) for n in range(nW)], np.int32)
    cost = np.array([score[P - lo], G[P - lo]]) if P else np.zeros(2)
    return A, G, period, np.array([P, nW, 0, 0], np.int32), cost


def _frame(C, h, t, dlo, dhi, pen):
    """(C[t], back[t]) from the values of C before t."""
    far = min(t, dhi)
    if far >= dlo:
        d = np.arange(dlo, far + 1)
        with np.errstate(invalid="ignore"):
            v = C[t - d] + pen[d - dlo]
            ok = v > -np.inf                                        # a NaN is skipped
        if ok.any():
            j = int(np.argmax(np.where(ok, v, -np.inf)))            # the first of equal maxima: the nearer p
            return float(h[t]) + float(v[j]), t - int(d[j])
    return float(h[t]), -1


def _finish(o, h, C, back, dlo, P, n_out):
    T = o.size
    n_out = (T - 1) // dlo + 1 if n_out is None else n_out
    e0 = max(0, T - P)
    tstar = e0 + int(np.argmax(C[e0:]))                             # the first of equal maxima: the earlier frame
    beats, t = [], tstar
    while t >= 0:
        beats.append(t)
        t = int(back[t])
    beats = beats[::-1]
    path = np.full(n_out, -1, np.int32)
    path[:len(beats)] = beats
    acc = 0.0
    for t in beats:
        acc = acc + float(h[t])
    return C, back, path, np.array([len(beats), tstar, 0, 0], np.int32), np.array([C[tstar], acc])


def track(o, dlo, dhi, P, pen, n_out=None):
    """(C [T], back [T] int32, beats [n_out] int32, summary [4] int32, cost [2]) of RV_BEAT_TRACK, frame by frame."""
    o, pen = np.asarray(o, np.float64), np.asarray(pen, np.float64)
    T = o.size
    assert pen.shape == (dhi - dlo + 1,) and 1 <= dlo <= dhi
    h = np.where(np.isfinite(o), o, 0.0)
    C, back = np.zeros(T), np.full(T, -1, np.int32)
    for t in range(T):
        C[t], back[t] = _frame(C, h, t, dlo, dhi, pen)
    return _finish(o, h, C, back, dlo, P, n_out)


def track_blocks(o, dlo, dhi, P, pen, n_out=None):
    """The same outputs, every block of dlo frames evaluated from a frozen copy of C (see the module doc)."""
    o, pen = np.asarray(o, np.float64), np.asarray(pen, np.float64)
    T = o.size
    h = np.where(np.isfinite(o), o, 0.0)
    C, back = np.zeros(T), np.full(T, -1, np.int32)
    for b0 in range(0, T, dlo):
        frozen = C.copy()
        for t in reversed(range(b0, min(T, b0 + dlo))):
            C[t], back[t] = _frame(frozen, h, t, dlo, dhi, pen)
    return _finish(o, h, C, back, dlo, P, n_out)


# ---- the host helpers, restated ----

def window_values(Wn):
    n = np.arange(Wn, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (n + 0.5) / Wn)


def tempo_prior(lo, hi, centre, octaves=1.0):
    tau = np.arange(lo, hi + 1, dtype=np.float64)
    if centre is None:
        return np.ones(tau.size)
    return np.exp(-0.5 * (np.log2(tau / centre) / octaves) ** 2)


def penalty_table(P, tightness=100.0):
    dlo, dhi = (P + 1) // 2, 2 * P
    d = np.arange(dlo, dhi + 1, dtype=np.float64)
    return dlo, dhi, -tightness * np.log(d / P) ** 2


# ---- inputs ----

def pulse_curve(P0, T, j, seed=0):
    """(curve [T], the pulse frames): N(0, 0.3) noise (RandomState(seed).randn) with +3 at every pulse and +1 on the frame
    after it; the pulses at 0, P0, 2 P0, ... below T, each moved by a uniform integer in [-j, j] (the same generator, after
    the noise) and kept inside [0, T - 2]."""
    rng = np.random.RandomState(seed)
    x = 0.3 * rng.randn(T)
    at = []
    for c in range(0, T, P0):
        t = min(max(c + (int(rng.randint(-j, j + 1)) if j else 0), 0), T - 2)
        at.append(t)
        x[t] += 3.0
        x[t + 1] += 1.0
    return x, np.array(at)


def chain(curve, lo, hi, Wn, Hw, centre, tightness=100.0, octaves=1.0):
    """onset -> tempogram -> track on a novelty curve: (P, beats, the three ops' outputs)."""
    on = onset(curve)
    tg = tempogram(on[0], Wn, Hw, lo, hi, window_values(Wn), tempo_prior(lo, hi, centre, octaves))
    P = int(tg[3][0])
    if P == 0:
        return 0, np.zeros(0, np.int32), on, tg, None
    dlo, dhi, pen = penalty_table(P, tightness)
    tr = track(on[0], dlo, dhi, P, pen)
    return P, tr[2][:tr[3][0]], on, tg, tr
