"""Numpy statement of continuity-aware mosaicing (RV_MOSAIC_TRANSITION / RV_MOSAIC_PATH_* in csrc/mosaic_path.hip,
rawaudiovae_kelsey_amd.mosaic.best_path) for the tests.

Inputs: candidates idx [T, k] and dist [T, k] as the kNN search writes them (ascending, -1 / +inf for missing), corpus
latents mu [N, L], a successor table next_of [N], a weight lam >= 0.

transitions: trans[t, i, j] = D(mu[next_of[idx[t-1, i]]], mu[idx[t, j]]) with D = mosaic_oracle's distance (the kernel's
arithmetic bit for bit); +inf when either candidate is -1 or the value is NaN; trans[0] = 0.
forward (fp32, row by row): m = min_i score[i]; s = score - m when m is finite;
new[j] = dist[t, j] + min_i (s[i] + fl(lam * trans[t, i, j])) over the pairs whose s[i] and trans are finite, strict <
in ascending i (ties to the lower i), back[t, j] = that i.  Row 0, and a row where no new[j] is finite, starts a new
sequence: new = dist[t] (+inf for -1 / NaN), back = NONE.  end[t] = lowest-j argmin of the row's scores, -1 if none is
finite.
backtrack: from end[T-1]; slot[t], then back[t, slot], or end[t-1] where the row started a sequence or is closed.
cost: [sum_t dist[t, slot[t]], sum of the transitions met along the path], float64 sums in ascending t from +0 over the
rows that have a slot; a row that starts a sequence adds no transition."""
import numpy as np

import mosaic_oracle as O

f32 = np.float32
INF = f32(np.inf)
NONE = 255


def batch_sq_dist(a, b):
    """[R, ka, kb] fp32: mosaic_oracle.sq_dist of a[r] [ka, L] against b[r] [kb, L] for every r."""
    a = np.asarray(a, f32)
    b = np.asarray(b, f32)
    R, ka, L = a.shape
    kb = b.shape[1]
    tot = np.zeros((R, ka, kb), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k0 in range(0, L, O.KT):
            part = np.zeros((R, ka, kb), f32)
            for l in range(k0, min(L, k0 + O.KT)):
                part = O._fma_sq(a[:, :, l][:, :, None] - b[:, :, l][:, None, :], part)
            tot = tot + part
    return tot


def transitions(mu, idx, next_of, chunk=512):
    mu = np.asarray(mu, f32)
    idx = np.asarray(idx)
    next_of = np.asarray(next_of)
    T, k = idx.shape
    tr = np.full((T, k, k), np.inf, f32)
    tr[0] = 0
    for t0 in range(1, T, chunk):
        t1 = min(T, t0 + chunk)
        a, b = idx[t0 - 1:t1 - 1], idx[t0:t1]
        va, vb = a >= 0, b >= 0
        d = batch_sq_dist(mu[next_of[np.where(va, a, 0)]], mu[np.where(vb, b, 0)])
        ok = va[:, :, None] & vb[:, None, :] & ~np.isnan(d)
        tr[t0:t1] = np.where(ok, d, INF)
    return tr


def targets(idx, dist):
    return np.where((np.asarray(idx) >= 0) & ~np.isnan(dist), dist, INF).astype(f32)


def forward(dist, tr, idx, lam):
    """(back [T, k] uint8, end [T] int32, met [T, k] fp32: the transition cost of (back[t, j], j), 0 where back is NONE)"""
    T, k = dist.shape
    lam = f32(lam)
    tgt = targets(idx, dist)
    back = np.full((T, k), NONE, np.uint8)
    met = np.zeros((T, k), f32)
    end = np.full(T, -1, np.int32)
    score = np.full(k, INF, f32)
    cols = np.arange(k)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            m = score.min()
            s = (score - m).astype(f32) if np.isfinite(m) else score
            fin = np.isfinite(tr[t]) & np.isfinite(s)[:, None]
            prod = (lam * np.where(fin, tr[t], f32(0))).astype(f32)          # rounded before the add; no 0 * inf
            c = np.where(fin, (s[:, None] + prod).astype(f32), INF)
            c = np.where(np.isfinite(c), c, INF)
            bi = c.argmin(0)                                                 # the first (lowest i) of equal minima
            best = c[bi, cols]
            new = np.where(np.isfinite(best), (tgt[t] + best).astype(f32), INF)
            ok = np.isfinite(new)
            new = np.where(ok, new, INF)
            if t == 0 or not ok.any():
                new = tgt[t].copy()
            else:
                back[t] = np.where(ok, bi, NONE)
                met[t] = np.where(ok, tr[t][bi, cols], f32(0))
            score = new
            end[t] = int(score.argmin()) if np.isfinite(score.min()) else -1
    return back, end, met


def backtrack(back, end):
    T = len(end)
    slot = np.full(T, -1, np.int32)
    cur = int(end[T - 1])
    for t in range(T - 1, -1, -1):
        slot[t] = cur
        if t:
            cur = int(end[t - 1]) if (cur < 0 or back[t, cur] == NONE) else int(back[t, cur])
    return slot


def best_path(idx, dist, mu, next_of, lam, tr=None):
    """(slot [T] int32, choice [T] int32, cost [2] float64)"""
    idx = np.asarray(idx)
    dist = np.asarray(dist, f32)
    if tr is None:
        tr = transitions(mu, idx, next_of)
    back, end, met = forward(dist, tr, idx, lam)
    slot = backtrack(back, end)
    T = len(slot)
    rows = np.arange(T)
    choice = np.where(slot >= 0, idx[rows, np.maximum(slot, 0)], -1).astype(np.int32)
    cost = np.zeros(2, np.float64)
    for t in range(T):
        if slot[t] >= 0:
            cost[0] += np.float64(dist[t, slot[t]])
            cost[1] += np.float64(met[t, slot[t]])
    return slot, choice, cost


def path_cost(slot, dist, tr, lam):
    """J of a path in float64 over one run of open rows (for the brute-force comparison)."""
    c = sum(float(dist[t, p]) for t, p in enumerate(slot))
    trs = sum(float(tr[t, slot[t - 1], slot[t]]) for t in range(1, len(slot)))
    return c + (trs if np.isinf(trs) else float(lam) * trs)   # an infinite transition stays infinite at lam = 0


def two_file_case(F=40, L=8, seed=0):
    """The two-file construction: file A a random walk a_f with integer steps of 2..4 in dimensions 1..L-1 and
    a_f[0] = 0, file B = A + e_0, target q_t = a_t + c_t e_0 with c_t = 3/8 on even and 5/8 on odd t.  Both files' frame
    t are always the two candidates of target frame t and the nearer one alternates.  A jump between the files costs
    lam * |e_0|^2 = lam at every frame, staying in one file (5/8)^2 - (3/8)^2 = 1/4 more target cost at every second
    frame: staying wins for lam > 1/8.  All values are exact in fp32.  -> (mu [2F, L], q [F, L], next_of [2F])"""
    rng = np.random.default_rng(seed)
    a = np.cumsum(rng.integers(2, 5, (F, L)) * rng.choice([-1, 1], (F, L)), 0).astype(f32)
    a[:, 0] = 0
    b = a.copy()
    b[:, 0] += 1
    mu = np.concatenate([a, b])
    i = np.arange(2 * F)
    next_of = np.where((i + 1) % F != 0, i + 1, i).astype(np.int32)
    q = a.copy()
    q[:, 0] = np.where(np.arange(F) % 2 == 0, 3 / 8, 5 / 8)
    return mu, q, next_of
