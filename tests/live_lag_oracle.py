"""Numpy statement of live mosaicing with a lag (k_live_lag in csrc/mosaic_live.hip, StreamingMosaic(lag=D) and drain()
in rawaudiovae_kelsey_amd/mosaic.py) for the tests, built on mosaic_oracle (the distance, the overlap-add),
mosaic_path_oracle (transitions, the forward rule, the backtrack) and live_mosaic_oracle (the weight rule).

The rule.  Frames arrive in order and wait as PENDING rows, at most lag + 1 of them.  A window solve commits the oldest
pending row a given the pending rows a..b:
  row a:       prev < 0, or next_of[prev] outside [0, N): score[j] = dist[a, j]; otherwise
               score[j] = dist[a, j] + fl(w * D(mu[next_of[prev]], mu[idx[a, j]])); +inf where idx[a, j] is outside
               [0, N) or the value is NaN (the greedy rule's expression)
  rows a+1..b: mosaic_path_oracle.forward's row rule with lam = w over the raw transitions
  end          the lowest-j argmin of row b's scores, walked back to row a by mosaic_path_oracle.backtrack
  choice[a] = idx[a, slot] (-1 without a slot) becomes prev.
A new frame joins the pending rows; with lag + 1 pending one solve runs, otherwise nothing is committed.  A drain step
runs one solve on the shrinking window while rows are pending.  w is the weight read by the call that commits row a
(live_mosaic_oracle.weight_of: not finite and >= 0 counts as 0)."""
import numpy as np

import live_mosaic_oracle as LO
import mosaic_oracle as O
import mosaic_path_oracle as P

f32 = np.float32
INF = f32(np.inf)


def schedule(calls, F, lag):
    """The order of events for `calls`, a string of 'p' (process: F new frames) and 'd' (drain: F steps) ->
    (last [T] int: the newest pending row when row a was committed (rows not yet committed at the end: T - 1, what a
    full drain would see), emit [len(calls) * F] int: the row committed at each output frame, -1 for none,
    T: the frames fed)."""
    T = calls.count("p") * F
    last = np.full(T, T - 1, np.int64)
    emit = []
    t, a = 0, 0                                                  # rows pushed so far, the oldest pending row
    for c in calls:
        for _ in range(F):
            if c == "p":
                t += 1
                go = t - a == lag + 1
            else:
                go = t - a > 0
            if go:
                last[a] = t - 1
                emit.append(a)
                a += 1
            else:
                emit.append(-1)
    return last, np.asarray(emit, np.int64), T


def entry_scores(idx_a, dist_a, mu, next_of, w, prev):
    """(score [k] fp32, D [k] fp32 or None) of the oldest row of a window, entered from the committed frame prev."""
    N = mu.shape[0]
    valid = (idx_a >= 0) & (idx_a < N)
    succ = int(next_of[prev]) if 0 <= prev < N else -1
    if not 0 <= succ < N:
        return np.where(valid & ~np.isnan(dist_a), dist_a, INF).astype(f32), None
    D = O.sq_dist(mu[succ][None], mu[np.where(valid, idx_a, 0)])[0]
    with np.errstate(invalid="ignore", over="ignore"):
        c = (dist_a + (LO.weight_of(w) * D).astype(f32)).astype(f32)
    return np.where(valid & ~np.isnan(c), c, INF).astype(f32), D


def solve(idx, dist, tr, mu, next_of, a, b, w, prev):
    """The slot committed for row a from the pending rows a..b, and the D its entry met (0 without a successor)."""
    score, D = entry_scores(idx[a], dist[a], mu, next_of, w, prev)
    wi, wd = idx[a:b + 1].copy(), dist[a:b + 1].copy()
    wi[0] = np.where(np.isfinite(score), idx[a], -1)             # row 0 of forward() takes its dist as the scores
    wd[0] = score
    back, end, _ = P.forward(wd, tr[a:b + 1], wi, LO.weight_of(w))
    slot = int(P.backtrack(back, end)[0])
    return slot, (float(D[slot]) if (slot >= 0 and D is not None) else 0.0)


def fixed_lag(idx, dist, mu, next_of, w_per_commit, lag, last=None, prev=-1):
    """(slot [T] int32, choice [T] int32, cost [2] float64: the sums of the chosen dist and of the D met between
    consecutive choices).  w_per_commit: a scalar, or the weight in force when each row is committed.  last: from
    schedule(); None = every frame in one run and a full drain at the end."""
    idx = np.asarray(idx)
    dist = np.asarray(dist, f32)
    mu = np.asarray(mu, f32)
    T, k = idx.shape
    ws = np.broadcast_to(np.asarray(w_per_commit, np.float64), (T,))
    if last is None:
        last = np.minimum(np.arange(T) + int(lag), T - 1)
    tr = P.transitions(mu, idx, next_of)
    slot = np.full(T, -1, np.int32)
    choice = np.full(T, -1, np.int32)
    cost = np.zeros(2, np.float64)
    prev = int(prev)
    for a in range(T):
        s, met = solve(idx, dist, tr, mu, next_of, a, int(last[a]), ws[a], prev)
        slot[a] = s
        if s >= 0:
            choice[a] = idx[a, s]
            cost[0] += np.float64(dist[a, s])
            cost[1] += met
        prev = int(choice[a])
    return slot, choice, cost


def play(emit, choice, frame_of, S, hop, window=None, blank=None):
    """The stream's output [len(emit) * hop] fp32 for the emitted rows: frame_of(i) [S] for the corpus frame committed
    at each output frame, `blank` where nothing was (warm-up: [blank] * lag + the chosen frames; a dry drain), through
    mosaic_oracle.ola.  blank = None: zeros, which is what grains mode adds; decode mode adds the decoder's frame of
    the zero latent there, as it does for a row without a candidate.  frame_of(-1) is the frame of such a row."""
    frames = np.zeros((len(emit), S), f32)
    if blank is not None:
        frames[:] = blank
    for f, e in enumerate(emit):
        if e >= 0:
            frames[f] = frame_of(int(choice[e]))
    return O.ola(frames, hop, len(emit) * hop, window)


def switches(choice, n_file):
    """How often consecutive choices lie in different files of n_file frames each."""
    f = np.asarray(choice) // n_file
    return int((f[1:] != f[:-1]).sum())
