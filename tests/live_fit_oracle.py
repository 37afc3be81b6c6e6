"""Numpy statement of live grain fitting (RV_MOSAIC_LIVE / LIVE_DRAIN with width = R or lam = gain_max in
csrc/mosaic_live.hip and csrc/grain.hip, StreamingMosaic(fit=R, gain_max=g) in rawaudiovae_kelsey_amd/mosaic.py) for the
tests, built from the other oracles: live_mosaic_oracle.greedy / live_lag_oracle.fixed_lag choose, grain_fit_oracle.fit
and .gather fit and scale the grains, live_lag_oracle.play overlap-adds them.

The rule.  A stream's TIMELINE is everything its calls fed since the reset, a drain counting as a block of zeros.
Target frame n is samples [n hop, n hop + S) of the timeline prefixed by P = S - hop zeros.  A row (the candidates of
one frame) ARRIVES at the absolute frame n at which it was searched.  Whatever is played for a row, at once (no
selection, or lag 0) or when the lag commits it, is fitted to target frame `arrival[row]`, never to the audio arriving
when it is played.  Without selection each of the k candidates is fitted on its own and the fitted grains are averaged;
with selection the one chosen frame is fitted.  An output frame that plays nothing (-1) has shift 0, gain 0, score 0."""
import numpy as np

import grain_fit_oracle as GF
import live_lag_oracle as G
import live_mosaic_oracle as LO

f32 = np.float32


def timeline(x, calls, block):
    """[len(calls) * block] fp32: the blocks of x [n] in order for every 'p' of calls, zeros for every 'd'"""
    x = np.asarray(x, f32)
    out = np.zeros(len(calls) * block, f32)
    b = 0
    for n, c in enumerate(calls):
        if c == "p":
            out[n * block:(n + 1) * block] = x[b * block:(b + 1) * block]
            b += 1
    return out


def target_frames(line, S, hop):
    """[len(line) // hop, S]: target frame n of the timeline, the frame the encoder saw"""
    padded = np.concatenate([np.zeros(S - hop, f32), np.asarray(line, f32)])
    n = len(line) // hop
    return padded[np.arange(n)[:, None] * hop + np.arange(S)[None, :]]


def arrival(calls, F):
    """[T] int: the absolute frame at which each row fed arrived (a drain moves time on without feeding)"""
    return np.concatenate([n * F + np.arange(F) for n, c in enumerate(calls) if c == "p"] or [np.zeros(0, np.int64)])


def fit_played(line, S, hop, tf, sel, src, row_start, room, R, gain_max):
    """The fits and the fitted frames of the output frames: sel [n_out, kf] the corpus frames each plays (-1: none),
    tf [n_out] the target frame each stands for (ignored where sel is -1) ->
    (shift [n_out, kf] int32, gain [n_out, kf] fp32, score [n_out, kf] fp64, frames [n_out, S] fp32)."""
    sel = np.asarray(sel)
    frames = target_frames(line, S, hop)
    tf = np.where((sel >= 0).any(1), tf, 0)
    target = frames[tf].reshape(-1)                              # frame r at r * S: grain_fit_oracle's hop = S
    shift, gain, score = GF.fit(target, S, S, sel, src, row_start, room, R, gain_max)
    return shift, gain, score, GF.gather(src, row_start, sel, shift, gain, S)


def run(x, calls, block, S, hop, idx, dist, src, row_start, room, R, gain_max, window=None, mu=None, next_of=None,
        weight_of_call=None, lag=0):
    """One stream through `calls` ('p': the next block of x, 'd': a drain) with the device's own candidates idx / dist
    [T, k] of the rows fed.  weight_of_call None: no selection (the mean of the k fitted candidates); else
    weight_of_call(n) is the stream's weight during call n, and mu [N, L], next_of [N] and lag say how rows are chosen.
    -> dict(choice [n_out] as emitted (-1 everywhere without selection), shift, gain, score [n_out, kf],
            y [n_out * hop], emit [n_out], tf [n_out])."""
    F = block // hop
    idx = np.asarray(idx)
    line = timeline(x, calls, block)
    arr = arrival(calls, F)
    T = arr.size
    assert idx.shape[0] == T
    if weight_of_call is None:
        assert "d" not in calls
        emit = np.arange(T)
        sel, want = idx, np.full(T, -1, np.int32)
    else:
        last, emit, _ = G.schedule(calls, F, lag)
        w = np.zeros(T)
        for pos, a in enumerate(emit):
            if a >= 0:
                w[a] = weight_of_call(pos // F)
        if lag == 0:
            _, choice, _, _ = LO.greedy(idx, dist, mu, next_of, w)
        else:
            _, choice, _ = G.fixed_lag(idx, dist, mu, next_of, w, lag, last=last)
        want = np.where(emit >= 0, choice[np.maximum(emit, 0)], -1).astype(np.int32)
        sel = want[:, None]
    tf = np.where(emit >= 0, arr[np.maximum(emit, 0)], 0)
    shift, gain, score, frames = fit_played(line, S, hop, tf, sel, src, row_start, room, R, gain_max)
    pos_of = {int(a): p for p, a in enumerate(emit) if a >= 0}
    y = G.play(emit, np.arange(T), lambda a: frames[pos_of[a]], S, hop, window)
    return dict(choice=want, shift=shift, gain=gain, score=score, y=y, emit=emit, tf=tf)
