"""numpy oracle of the latent states (include/rawvae_hip.h, "Latent states"): a Gaussian hidden Markov model.

Two restatements.  The float64 one writes the header's chain orders out -- every fma through fma(), an error-free
product and sum, so that what the header calls exact can be compared bit for bit: EMIT, VITERBI, the moments and the
closing divisions of MSTEP.  The numpy.longdouble one is the log-domain recursion (logsumexp, no rescaling), the
reference for what passes through exp and log on the device: gamma, xi, ll, g and the logarithms of pi and A.

The gates.  The device's exp and log are not numpy's; both are a few ulp from the true value.  So each gate is 4 times
the distance measured on the CPU between the float64 oracle and the longdouble one at the tests' own shapes
(tests/test_states_cpu.py::test_gates_hold_on_the_cpu measures them again and holds them to the constants below):

  gamma   |d gamma|, relative to 1
  xi      |d xi| / max(1, the sequence's pairs)
  ll      |d ll| / sum_t |log c_t + M_t|
  g       |d g| / (k log(2 pi) + sum_j |log v_sj|)
  log A   |d log A| / max(1, |log A|) over the finite entries (and log pi likewise)
"""
import functools

import numpy as np

LD = np.longdouble
LOG_2PI = 1.8378770664093453
RANGE, CHUNK, ROWS = 4096, 32, 256     # csrc/moment.h
EMIT_FRAMES = 64                       # frames of one workgroup of RV_HMM_EMIT
NONE = 255

GATE_GAMMA = 4 * 2.56e-11    # measured 2.56e-11 (S 2 with the frame 1e3 standard deviations out: logb - M ~ 1e7 is rounded
#                              to 2e-9 before exp; without that frame 4.58e-15 at S 17)
GATE_XI = 4 * 6.71e-12       # measured 6.71e-12 (S 1, the same frame; without it 2.38e-16 at S 2)
GATE_LL = 4 * 9.70e-16       # measured 9.70e-16 (S 17, no outlier)
GATE_G = 4 * 2.20e-16        # measured 2.20e-16 (S 64, k 64)
GATE_LOG_A = 4 * 1.09e-16    # measured 1.09e-16 (S 64, k 64); log pi 9.87e-17

GATED_STATES = (1, 2, 17, 64)
GATED_LENGTHS = (1, 2, 257)
MSTEP_SHAPES = ((3, 3), (17, 33), (64, 64))    # (S, k) at T = 300


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def fma(a, b, c):
    """fl(a b + c) elementwise in float64: the product's error by Dekker's splitting, the sum's by Knuth's two-sum.
    (The last add rounds s + (t + e) where t + e is itself rounded: off by a bit only when that sum lands within one
    rounding of a tie, a chance of 2^-52 per operation.)  Non-finite operands go through plain arithmetic."""
    a, b, c = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64)
    with np.errstate(all="ignore"):
        p = a * b
        ah, al = _split(a)
        bh, bl = _split(b)
        e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        s = p + c
        bb = s - p
        t = (p - (s - bb)) + (c - bb)
        r = s + (t + e)
        ok = np.isfinite(r)
        if ok.all():
            return r
        return np.where(ok & np.isfinite(p) & np.isfinite(c), r, p + c)


def layout(S, k):
    o, at = {}, 0
    for name, n in (("m", S * k), ("w", S * k), ("g", S), ("pi", S), ("A", S * S), ("logpi", S), ("logA", S * S)):
        o[name] = slice(at, at + n)
        at += n
    o["doubles"] = at
    return o


def _log0(a):
    with np.errstate(divide="ignore"):
        return np.log(a)


def g_of(v):
    """g [S] of the variances v [S, k]: the logarithms added in ascending j from +0"""
    acc = np.zeros(v.shape[0], v.dtype)
    for j in range(v.shape[1]):
        acc = acc + np.log(v[:, j])
    return v.dtype.type(-0.5) * (v.dtype.type(v.shape[1]) * v.dtype.type(LOG_2PI) + acc)


def pack(m, v, pi, A):
    """theta of means m [S, k], variances v [S, k], pi [S] and A [S, S]"""
    S, k = m.shape
    o = layout(S, k)
    th = np.empty(o["doubles"])
    th[o["m"]], th[o["w"]], th[o["g"]] = m.ravel(), (1.0 / v).ravel(), g_of(np.asarray(v, np.float64))
    th[o["pi"]], th[o["A"]] = pi, A.ravel()
    th[o["logpi"]], th[o["logA"]] = _log0(pi), _log0(A).ravel()
    return th


def unpack(th, S, k):
    o = layout(S, k)
    return dict(m=th[o["m"]].reshape(S, k), w=th[o["w"]].reshape(S, k), g=th[o["g"]], pi=th[o["pi"]],
                A=th[o["A"]].reshape(S, S), logpi=th[o["logpi"]], logA=th[o["logA"]].reshape(S, S))


def sequences(row_start, T):
    rs = np.clip(np.asarray(row_start, np.int64), 0, T)
    return [(int(a), int(max(a, b))) for a, b in zip(rs[:-1], rs[1:])]


def observed(x):
    return np.isfinite(np.asarray(x)).all(axis=1)


def whiten(x, c, P):
    """y [T, k]: y_j = chain fma(P[j, l], (double)x[t, l] - c[l], .) in ascending l from +0 (+0 in an unobserved frame)"""
    x64 = np.asarray(x, np.float64)
    y = np.zeros((x64.shape[0], P.shape[0]))
    with np.errstate(all="ignore"):
        for l in range(x64.shape[1]):
            y = fma(P[:, l][None, :], (x64[:, l] - c[l])[:, None], y)
    y[~observed(x)] = 0.0
    return y


def emit(x, c, P, th, S, k):
    p = unpack(th, S, k)
    y = whiten(x, c, P)
    q = np.zeros((y.shape[0], S))
    for j in range(k):
        d = y[:, j][:, None] - p["m"][:, j][None, :]
        q = fma(p["w"][:, j][None, :] * d, d, q)
    logb = p["g"][None, :] - 0.5 * q
    logb[~observed(x)] = np.nan
    return logb


def _scale(row):
    """(M_t, b~_t) of a row of logb"""
    if np.isnan(row).any():
        return 0.0, np.ones_like(row)
    M = row.max()
    with np.errstate(all="ignore"):
        return M, np.exp(row - M)


def forward_backward(logb, row_start, th, S, k):
    """The scaled recursion in float64, the header's orders written out -> gamma [T, S], xi [n, S, S], ll [n] and
    ll's scale sum_t |log c_t + M_t| [n]"""
    p = unpack(th, S, k)
    A, T = p["A"], logb.shape[0]
    seqs = sequences(row_start, T)
    gamma, xi = np.zeros((T, S)), np.zeros((len(seqs), S, S))
    ll, scale = np.zeros(len(seqs)), np.zeros(len(seqs))
    for n, (t0, t1) in enumerate(seqs):
        alpha, cs = np.zeros((t1 - t0, S)), np.zeros(t1 - t0)
        for t in range(t0, t1):
            M, bt = _scale(logb[t])
            if t == t0:
                a = p["pi"] * bt
            else:
                acc = np.zeros(S)
                for i in range(S):
                    acc = fma(alpha[t - t0 - 1, i], A[i, :], acc)
                a = bt * acc
            c = 0.0
            for j in range(S):
                c = c + a[j]
            alpha[t - t0], cs[t - t0] = a / c, c
            term = np.log(c) + M
            ll[n] = ll[n] + term
            scale[n] += abs(term)
        beta = np.ones(S)
        if t1 > t0:
            gamma[t1 - 1] = alpha[-1] * beta
        for t in range(t1 - 2, t0 - 1, -1):
            _, bt = _scale(logb[t + 1])
            u = (bt * beta) / cs[t + 1 - t0]
            nb = np.zeros(S)
            for j in range(S):
                nb = fma(A[:, j], u[j], nb)
            beta = nb
            gamma[t] = alpha[t - t0] * beta
            xi[n] = fma(alpha[t - t0][:, None] * A, u[None, :], xi[n])
    return gamma, xi, ll, scale


def _lse(a, axis):
    m = np.max(a, axis=axis, keepdims=True)
    m = np.where(np.isfinite(m), m, LD(0))
    with np.errstate(divide="ignore"):
        return np.log(np.sum(np.exp(a - m), axis=axis)) + np.squeeze(m, axis)


def forward_backward_ld(logb, row_start, th, S, k):
    """The same in the log domain in longdouble: no rescaling, no chain order -> gamma, xi, ll"""
    p = unpack(th, S, k)
    with np.errstate(divide="ignore"):
        lA, lpi = np.log(p["A"].astype(LD)), np.log(p["pi"].astype(LD))
    T = logb.shape[0]
    seqs = sequences(row_start, T)
    gamma, xi, ll = np.zeros((T, S), LD), np.zeros((len(seqs), S, S), LD), np.zeros(len(seqs), LD)
    lb = np.where(np.isnan(logb).any(axis=1)[:, None], 0.0, logb).astype(LD)
    for n, (t0, t1) in enumerate(seqs):
        if t1 == t0:
            continue
        la, lbeta = np.zeros((t1 - t0, S), LD), np.zeros((t1 - t0, S), LD)
        la[0] = lpi + lb[t0]
        for t in range(t0 + 1, t1):
            la[t - t0] = lb[t] + _lse(la[t - t0 - 1][:, None] + lA, 0)
        ll[n] = _lse(la[-1], 0)
        for t in range(t1 - 2, t0 - 1, -1):
            lbeta[t - t0] = _lse(lA + (lb[t + 1] + lbeta[t - t0 + 1])[None, :], 1)
            xi[n] += np.exp(la[t - t0][:, None] + lA + (lb[t + 1] + lbeta[t - t0 + 1])[None, :] - ll[n])
        gamma[t0:t1] = np.exp(la + lbeta - ll[n])
    return gamma, xi, ll


def viterbi(logb, row_start, th, S, k):
    """path [T] int32 (rows outside every sequence: the fill -77), score [n]: the header's total order written out"""
    p = unpack(th, S, k)
    T = logb.shape[0]
    seqs = sequences(row_start, T)
    path, score = np.full(T, -77, np.int32), np.zeros(len(seqs))
    with np.errstate(all="ignore"):
        for n, (t0, t1) in enumerate(seqs):
            if t1 == t0:
                continue
            back = np.full((t1 - t0, S), NONE, np.int64)
            d = None
            for t in range(t0, t1):
                add = np.zeros(S) if np.isnan(logb[t]).any() else logb[t]
                if t == t0:
                    d = add + p["logpi"]
                    continue
                best, bi = np.full(S, -np.inf), np.full(S, NONE, np.int64)
                for i in range(S):
                    v = d[i] + p["logA"][i, :]
                    take = v > best
                    best, bi = np.where(take, v, best), np.where(take, i, bi)
                d, back[t - t0] = add + best, bi
            top, e = -np.inf, NONE
            for j in range(S):
                if d[j] > top:
                    top, e = d[j], j
            score[n] = top
            for t in range(t1 - 1, t0 - 1, -1):
                path[t] = e if e < S else -1
                if t > t0 and e < S:
                    e = int(back[t - t0, e])
    return path, score


def moments(y, obs, gamma):
    """N [S], M1 [S, k], M2 [S, k] in csrc/moment.h's orders: N in blocks of 256 frames, each in ascending t from +0,
    the blocks in ascending order from +0; M1 and M2 in ranges of 4096 frames, within a range one fma per frame in
    ascending t from +0 (v_mfma_f64_16x16x4_f64 adds its four frames one after the other), the ranges in ascending order
    from +0.  Unobserved frames contribute nothing: their y is +0 and their gamma is left out of N."""
    T, S = gamma.shape
    gn = np.where(obs[:, None], gamma, 0.0)
    N = np.zeros(S)
    for b0 in range(0, T, ROWS):
        acc = np.zeros(S)
        for row in gn[b0:b0 + ROWS]:
            acc = acc + row
        N = N + acc
    y2 = y * y
    M1, M2 = np.zeros((S, y.shape[1])), np.zeros((S, y.shape[1]))
    for r0 in range(0, T, RANGE):
        a1, a2 = np.zeros_like(M1), np.zeros_like(M2)
        for t in range(r0, min(r0 + RANGE, T)):
            a1 = fma(gamma[t][:, None], y[t][None, :], a1)
            a2 = fma(gamma[t][:, None], y2[t][None, :], a2)
        M1, M2 = M1 + a1, M2 + a2
    return N, M1, M2


def mstep(x, c, P, gamma, xi, row_start, th_old, S, k, floor):
    """-> dict(theta, info, N, M1, M2, v): the header's M-step in float64 (g, log pi and log A through numpy's log)"""
    old = unpack(th_old, S, k)
    floor = np.float64(np.float32(floor))
    y, obs = whiten(x, c, P), observed(x)
    N, M1, M2 = moments(y, obs, gamma)
    dead = ~(N >= 1.0)
    with np.errstate(all="ignore"):
        m = M1 / N[:, None]
        raw = M2 / N[:, None] - m * m
        v = np.where(raw > floor, raw, floor)
    m = np.where(dead[:, None], old["m"], m)
    w = np.where(dead[:, None], old["w"], 1.0 / v)
    v = np.where(dead[:, None], 1.0, v)
    g = np.where(dead, old["g"], g_of(v))
    seqs = [s for s in sequences(row_start, gamma.shape[0]) if s[1] > s[0]]
    acc = np.zeros(S)
    for t0, _ in seqs:
        acc = acc + gamma[t0]
    pi = acc / len(seqs) if seqs else old["pi"]
    num = np.zeros((S, S))
    for n in range(xi.shape[0]):
        num = num + xi[n]
    rs = np.zeros(S)
    for j in range(S):
        rs = rs + num[:, j]
    with np.errstate(all="ignore"):
        A = np.where((rs > 0)[:, None], num / rs[:, None], old["A"])
    o = layout(S, k)
    th = np.empty(o["doubles"])
    th[o["m"]], th[o["w"]], th[o["g"]], th[o["pi"]], th[o["A"]] = m.ravel(), w.ravel(), g, pi, A.ravel()
    th[o["logpi"]], th[o["logA"]] = _log0(pi), _log0(A).ravel()
    return dict(theta=th, info=dead.astype(np.int32), N=N, M1=M1, M2=M2, v=v)


def logs_ld(res, S, k):
    """(g, log pi, log A, g's scale) in longdouble of an M-step's variances, pi and A (dead states: g is not recomputed)"""
    p = unpack(res["theta"], S, k)
    v = res["v"].astype(LD)
    with np.errstate(divide="ignore"):
        return (g_of(v), np.log(p["pi"].astype(LD)), np.log(p["A"].astype(LD)),
                k * LOG_2PI + np.abs(np.log(res["v"])).sum(axis=1))


def log_distance(got, want):
    """max |got - want| / max(1, |want|) over the finite entries; the infinite ones must agree exactly"""
    got, want = np.asarray(got, LD), np.asarray(want, LD)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], want[~fin])
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1, np.abs(want[fin])), initial=0))


# ---- the test inputs ----

@functools.lru_cache(maxsize=None)
def basis(k, L, seed=0):
    """(c [L], P [k, L]) fp64: rows of a random rotation over scales 0.5 .. 2.  Read-only."""
    rng = np.random.default_rng(1000 * k + L + seed)
    Q = np.linalg.qr(rng.standard_normal((L, L)))[0][:k]
    P = Q / np.geomspace(0.5, 2.0, k)[:, None]
    c = rng.uniform(-1, 1, L)
    c.setflags(write=False)
    P.setflags(write=False)
    return c, P


def random_theta(S, k, seed=0, zeros=False):
    """A parameter block with means a few units apart, variances in 0.25 .. 4 and a random A (zeros: with exact zeros in
    pi and A, so that log has -inf to write)"""
    rng = np.random.default_rng(7 * S + k + seed)
    m, v = rng.normal(0, 2, (S, k)), rng.uniform(0.25, 4, (S, k))
    A, pi = rng.uniform(0.05, 1, (S, S)) + 4 * np.eye(S), rng.uniform(0.2, 1, S)
    if zeros and S > 1:
        A[rng.uniform(size=(S, S)) < 0.3] = 0
        A[np.arange(S), np.arange(S)] = 1
        pi[1::2] = 0
    return pack(m, v, pi / pi.sum(), A / A.sum(axis=1, keepdims=True))


def latents(T, L, seed=0):
    x = np.random.default_rng(31 * T + L + seed).normal(0, 1.5, (T, L)).astype(np.float32)
    return x


def starts(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def gated_case(S, outlier=False):
    """(logb [T, S], row_start, theta, k) for the gated comparisons: sequences of 1, 2 and 257 frames drawn around the
    states' means; outlier: the long sequence holds one frame 1e3 standard deviations from every state and one
    unobserved frame.  Read-only."""
    k, L = 4, 8
    c, P = basis(k, L)
    th = random_theta(S, k)
    rs = starts(GATED_LENGTHS)
    rng = np.random.default_rng(S)
    p = unpack(th, S, k)
    st = rng.integers(0, S, int(rs[-1]))
    y = p["m"][st] + rng.standard_normal((int(rs[-1]), k)) / np.sqrt(p["w"][st])
    x = (c + y @ np.linalg.pinv(P).T).astype(np.float32)
    if outlier:
        x[100] = (c + (1e3 * 4 * np.ones(k)) @ np.linalg.pinv(P).T).astype(np.float32)
        x[150] = np.nan
    logb = emit(x, c, P, th, S, k)
    for a in (logb, rs, th):
        a.setflags(write=False)
    return logb, rs, th, k


def gated_distances(got, S, outlier=False):
    """(d gamma, d xi, d ll) of (gamma, xi, ll) against the longdouble oracle at gated_case(S, outlier)"""
    logb, rs, th, k = gated_case(S, outlier)
    gamma, xi, ll = got
    _, _, _, scale = forward_backward(logb, rs, th, S, k)
    rg, rx, rl = forward_backward_ld(logb, rs, th, S, k)
    pairs = np.maximum(1, np.diff(rs) - 1)[:, None, None]
    nz = scale > 0
    return (float(np.abs(gamma - rg).max()), float((np.abs(xi - rx) / pairs).max()),
            float((np.abs(ll - rl)[nz] / scale[nz]).max()))


@functools.lru_cache(maxsize=None)
def mstep_case(S, k, T=300, lengths=None, L=None):
    """(x [T, L] fp32 with one unobserved frame, L = k + 6 unless given, c, P, gamma, xi, row_start, theta with zeros in
    pi and A) for the M-step.  gamma's rows are random laws that favour the early states by up to 1e4, so the late ones
    hold less than one frame and die; xi is random with zero columns (log A = -inf) and the last state's row all zero (it
    keeps its old row of A).  Read-only."""
    L = k + 6 if L is None else L
    c, P = basis(k, L)
    x = latents(T, L)
    if T > 2:
        x[T // 2] = np.nan
    th = random_theta(S, k, zeros=True)
    rs = starts(lengths if lengths is not None else [T // 3, 0, T - T // 3])
    rng = np.random.default_rng(T + 11 * S + k)
    gamma = rng.uniform(0, 1, (T, S)) * np.geomspace(1, 1e-4, S)
    gamma /= gamma.sum(axis=1, keepdims=True)
    xi = rng.uniform(0, 1, (rs.size - 1, S, S))
    xi[:, :, 1::3] = 0
    xi[:, S - 1, :] = 0
    for a in (x, gamma, xi, rs, th):
        a.setflags(write=False)
    return x, c, P, gamma, xi, rs, th


def mstep_distances(theta, res, S, k):
    """(d g, d log pi, d log A) of an M-step's theta against the longdouble logarithms of the oracle's result `res`"""
    p = unpack(np.asarray(theta), S, k)
    gl, lpi, lA, gs = logs_ld(res, S, k)
    alive = res["info"] == 0
    return (float(np.max(np.abs(p["g"] - gl)[alive] / gs[alive], initial=0)), log_distance(p["logpi"], lpi),
            log_distance(p["logA"], lA))


# ---- planted data and the oracle's own fit ----

PLANT_SEED = 1     # the seed of LatentStates.fit at which the oracle's fit meets both conditions (test_states_cpu.py)
PLANT = dict(S=3, k=4, L=8, n=3, length=400, stay=0.95, iters=20)


@functools.lru_cache(maxsize=None)
def planted():
    """(x [1200, 8] fp32, row_start, labels [1200], c, P): three sequences of 400 frames from a 3-state chain with
    self-transition 0.95 whose means lie 8 standard deviations apart along the whitened axes.  Read-only."""
    S, k, L, n, length = (PLANT[q] for q in ("S", "k", "L", "n", "length"))
    rng = np.random.default_rng(2024)
    c, P = basis(k, L)
    means = np.zeros((S, k))
    means[1, 0], means[2, 1] = 8.0, 8.0
    labels = np.empty(n * length, np.int64)
    for f in range(n):
        s = rng.integers(0, S)
        for t in range(length):
            if t and rng.uniform() >= PLANT["stay"]:
                s = (s + rng.integers(1, S)) % S
            labels[f * length + t] = s
    y = means[labels] + rng.standard_normal((n * length, k))
    x = (c + y @ np.linalg.pinv(P).T).astype(np.float32)
    rs = starts([length] * n)
    for a in (x, rs, labels):
        a.setflags(write=False)
    return x, rs, labels, c, P


def initial(x, c, P, S, k, seed):
    """LatentStates.fit's start: S distinct observed frames chosen by RandomState(seed) as means, v = 1, pi uniform,
    A = 0.9 I + 0.1 / S"""
    ok = np.flatnonzero(observed(x))
    pick = np.sort(np.random.RandomState(seed).choice(ok.size, S, replace=False))
    m = (np.asarray(x, np.float64)[ok[pick]] - c) @ P[:k].T
    return pack(m, np.ones((S, k)), np.full(S, 1.0 / S), 0.9 * np.eye(S) + 0.1 / S)


def fit(x, row_start, c, P, S, k, iters, seed, floor=1e-3):
    """iters EM iterations from initial(): -> (theta, the ll history [iters] = each iteration's sum over the sequences
    in ascending order from +0, the scales [iters])"""
    th = initial(x, c, P, S, k, seed)
    hist, scales = [], []
    for _ in range(iters):
        logb = emit(x, c, P, th, S, k)
        gamma, xi, ll, scale = forward_backward(logb, row_start, th, S, k)
        tot = 0.0
        for v in ll:
            tot = tot + v
        hist.append(tot)
        scales.append(float(scale.sum()))
        th = mstep(x, c, P, gamma, xi, row_start, th, S, k, floor)["theta"]
    return th, np.array(hist), np.array(scales)


@functools.lru_cache(maxsize=None)
def planted_fit():
    """fit() on planted() at PLANT_SEED, computed once.  Read-only."""
    x, rs, _, c, P = planted()
    out = fit(x, rs, c, P, PLANT["S"], PLANT["k"], PLANT["iters"], PLANT_SEED)
    for a in out:
        a.setflags(write=False)
    return out


def agreement(path, labels, S):
    """the share of frames on which path agrees with labels under the best permutation of the S <= 3 states"""
    import itertools
    return max(float(np.mean(np.asarray(perm)[path] == labels)) for perm in itertools.permutations(range(S)))
