"""numpy.longdouble oracle of latent restoration (include/rawvae_hip.h, "Latent restoration").

The TEXTBOOK Kalman filter (gain K = P- S^-1 by an explicit solve, P+ = (I - K) P-, symmetrised) and a
Rauch-Tung-Striebel smoother (gain C_t = P+_t A^T (P-_{t+1})^-1 by an explicit solve): another algorithm than the
kernels' Cholesky-Crout filter and Bryson-Frazier backward pass, so agreement is not a shared mistake.  bryson_frazier is
the kernels' recursion restated in longdouble, held against the RTS result by tests/test_smooth_cpu.py.  Also the splice
gain and brute-force forms of the mask and region logic.  Corpora: walk_oracle.make_corpus; models: walk_oracle.fit, in
numpy, so the kernels are tested independently of the GPU fit.

The gates of tests/test_smooth_gpu.py.  Each is 8 x the largest value MEASURED on an MI355X over every case of that file
(the slack is for other boxes and other compiler orderings); k 2^-53 cond(S) with cond <= 1e4 puts the expectation near
1e-10 and a measured value above 1e-8 would be a defect of the kernel, not a reason for a wider gate.  State errors are
normalised by max(1, ||y||_inf) of the sequence; nis by its own value; logdet by sum_j |log eig_j(S)| (its own value
where the terms share a sign: a sum of logarithms that cancels has no relative error to speak of)."""
import functools

import numpy as np

import walk_oracle as WO

LD = np.longdouble
CEILING = 1e-8                     # above this a measured error is a defect

GATE_FILTERED = 8 * 8.19e-15       # w+     measured 8.19e-15 (k 64, L 70, dense, r 1e-4)
GATE_SMOOTHED = 8 * 8.19e-15       # w-hat  measured 8.19e-15 (the same case)
GATE_NIS = 8 * 1.01e-13            # nis    measured 1.01e-13 (k 1, r 1e-2: one squared innovation, v = y - w- cancels)
GATE_LOGDET = 8 * 2.54e-9          # logdet measured 2.54e-9 (r 1e-4 with weights up to 1e3: r_t = 1e-7, and S = 1 + 1e-7 at a
#                                    sequence's first frame holds log S = 1e-7 to 2^-53 / 1e-7 = 1.1e-9 already; 1.39e-13 at r = 1)

# (k, L, diagonal): the shapes of the issue; dense up to k = 64, diagonal beyond
SHAPES = [(1, 1, False), (2, 3, False), (17, 17, False), (17, 70, False), (64, 64, False), (64, 70, False),
          (70, 70, True), (300, 512, True)]
LENGTHS = [(1,), (2,), (1, 2, 5), (37, 1, 90)]
MASKS = ("none", "first", "last", "sequence", "alternating", "gap30", "weights")
NOISES = (1e-4, 1e-2, 1.0)


@functools.lru_cache(maxsize=None)
def model(k, L, diagonal=False):
    """walk_oracle.fit on a one-file corpus of max(300, L + 100) frames: dict of centre, P, R, A, B, ... (float64)."""
    lengths = (max(300, L + 100),)
    m = WO.fit(WO.make_corpus(lengths, L), WO.row_start(lengths), k, diagonal)
    for a in m.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return m


def weights_for(mask, lengths, seed=0):
    """fp32 [T] weights of one mask kind over sequences of `lengths`: 1 observed, 0 missing ("weights": log-uniform over
    [1e-3, 1e3], all observed).  "sequence": the middle sequence is missing whole; "gap30": frames [20, 50) of the
    longest sequence (clipped to it, its first frame kept where it has more than one)."""
    T = int(sum(lengths))
    rs = WO.row_start(lengths)
    w = np.ones(T, dtype=np.float32)
    if mask == "none":
        return w
    if mask == "weights":
        return np.exp(np.random.default_rng(seed + T).uniform(np.log(1e-3), np.log(1e3), T)).astype(np.float32)
    for s, n in enumerate(lengths):
        a = int(rs[s])
        if mask == "first":
            w[a] = 0
        elif mask == "last":
            w[a + n - 1] = 0
        elif mask == "alternating":
            w[a + 1:a + n:2] = 0
        elif mask == "sequence" and s == len(lengths) // 2:
            w[a:a + n] = 0
        elif mask == "gap30" and s == int(np.argmax(lengths)):
            w[a + min(20, n - 1):a + min(50, n)] = 0
    return w


def observe(x, weight, m):
    """y [T, k] longdouble = P (x - c) (zero at missing frames, whose rows are not read), obs [T] bool, r-scale [T]."""
    obs = np.asarray(weight) > 0
    P, c = m["P"].astype(LD), m["centre"].astype(LD)
    y = np.zeros((len(obs), P.shape[0]), dtype=LD)
    y[obs] = (np.asarray(x)[obs].astype(LD) - c) @ P.T
    return y, obs


def noise_of(r, weight):
    """r_t = fl64((double)(float)r / (double)weight[t]) as float64 (inf or NaN where the frame is missing)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.float64(np.float32(r)) / np.asarray(weight, dtype=np.float32).astype(np.float64)


def solve(M, B, logdet=False):
    """M^-1 B in longdouble: Gaussian elimination with partial pivoting on [M | B] (numpy.linalg has no longdouble).
    logdet: also sum log |pivot| = log |det M|."""
    n = len(M)
    W = np.concatenate([np.array(M, dtype=LD), np.array(B, dtype=LD).reshape(n, -1)], axis=1)
    ld = LD(0)
    for j in range(n):
        p = j + int(np.argmax(np.abs(W[j:, j])))
        if p != j:
            W[[j, p]] = W[[p, j]]
        ld += np.log(np.abs(W[j, j]))
        W[j + 1:, j:] -= np.outer(W[j + 1:, j] / W[j, j], W[j, j:])
    X = W[:, n:]
    for j in range(n - 1, -1, -1):
        X[j] = (X[j] - W[j, j + 1:n] @ X[j + 1:]) / W[j, j]
    return (X, ld) if logdet else X


def kalman_rts(y, obs, rt, A, B, diagonal=False):
    """One sequence by the textbook -> dict of wp (w+), wh (w-hat) [T, k], nis, logdet [T] and logabs [T] =
    sum_j |log eig_j(S)| (float64).  diagonal: A and B are diagonal and every axis is filtered on its own (the same
    formulas on scalars)."""
    T, k = y.shape
    if diagonal:
        return _scalar_rts(y, obs, rt, np.diag(A).astype(LD), np.diag(B).astype(LD))
    A, B = np.asarray(A).astype(LD), np.asarray(B).astype(LD)
    Qn, I = B @ B.T, np.eye(k, dtype=LD)
    wm, Pm, wp, Pp = [], [], [], []
    nis, logdet, logabs = np.full(T, -1.0), np.zeros(T), np.zeros(T)
    w, P = np.zeros(k, dtype=LD), I.copy()
    for t in range(T):
        if t:
            w, P = A @ w, A @ P @ A.T + Qn
            P = (P + P.T) / 2
        wm.append(w), Pm.append(P)
        if obs[t]:
            r = LD(rt[t])
            S = P + r * I
            v = y[t] - w
            X, ld = solve(S, np.column_stack([P, v]), logdet=True)
            K, u = X[:, :k].T, X[:, k]              # P S^-1 (both symmetric) and S^-1 v
            w = w + K @ v
            P = (I - K) @ P
            P = (P + P.T) / 2
            nis[t] = float(v @ u)
            ev = np.linalg.eigvalsh(S.astype(np.float64))
            logabs[t] = np.abs(np.log(ev)).sum()
            logdet[t] = float(ld)
        wp.append(w), Pp.append(P)
    wh = [None] * T
    wh[T - 1] = wp[T - 1]
    for t in range(T - 2, -1, -1):
        # w+_t + C_t (w-hat_{t+1} - w-_{t+1}) with the gain C_t = P+_t A^T (P-_{t+1})^-1 applied to the one vector
        wh[t] = wp[t] + Pp[t] @ (A.T @ solve(Pm[t + 1], wh[t + 1] - wm[t + 1])[:, 0])
    return dict(wp=np.array(wp, dtype=LD), wh=np.array(wh, dtype=LD), nis=nis, logdet=logdet, logabs=logabs)


def _scalar_rts(y, obs, rt, a, b):
    T, k = y.shape
    q = b * b
    wm, Pm, wp, Pp = (np.zeros((T, k), dtype=LD) for _ in range(4))
    nis, logdet, logabs = np.full(T, -1.0), np.zeros(T), np.zeros(T)
    w, P = np.zeros(k, dtype=LD), np.ones(k, dtype=LD)
    for t in range(T):
        if t:
            w, P = a * w, a * P * a + q
        wm[t], Pm[t] = w, P
        if obs[t]:
            r = LD(rt[t])
            S = P + r
            v = y[t] - w
            K = P / S
            w = w + K * v
            P = (1 - K) * P
            nis[t] = float((v * v / S).sum())
            logdet[t] = float(np.log(S).sum())
            logabs[t] = float(np.abs(np.log(S)).sum())
        wp[t], Pp[t] = w, P
    wh = np.zeros((T, k), dtype=LD)
    wh[T - 1] = wp[T - 1]
    for t in range(T - 2, -1, -1):
        wh[t] = wp[t] + Pp[t] * a / Pm[t + 1] * (wh[t + 1] - wm[t + 1])
    return dict(wp=wp, wh=wh, nis=nis, logdet=logdet, logabs=logabs)


def bryson_frazier(y, obs, rt, A, B):
    """The header's recursion in longdouble, with explicit solves in place of the factorisation -> (w+ [T, k],
    w-hat [T, k])."""
    T, k = y.shape
    A, B = np.asarray(A).astype(LD), np.asarray(B).astype(LD)
    Qn, I = B @ B.T, np.eye(k, dtype=LD)
    w, P = np.zeros(k, dtype=LD), I.copy()
    wm, Pm, us, wp = [], [], [], []
    for t in range(T):
        if t:
            w, P = A @ w, A @ P @ A.T + Qn
        wm.append(w), Pm.append(P)
        u = None
        if obs[t]:
            S = P + LD(rt[t]) * I
            u = solve(S, y[t] - w)[:, 0]
            w, P = w + P @ u, P - P @ solve(S, P)
        us.append(u), wp.append(w)
    lam, wh = np.zeros(k, dtype=LD), [None] * T
    for t in range(T - 1, -1, -1):
        lh = lam
        if obs[t]:
            lh = us[t] + lam - solve(Pm[t] + LD(rt[t]) * I, Pm[t] @ lam)[:, 0]
        wh[t] = wm[t] + Pm[t] @ lh
        lam = A.T @ lh
    return np.array(wp, dtype=LD), np.array(wh, dtype=LD)


def latent_rows(x, obs, y, wh, m):
    """(z [T, L] longdouble, terms [T, L] = |c_l| + sum_j |R_jl| + |rho_l|, the scale of the fp64 error of a row)."""
    R, c = m["R"].astype(LD), m["centre"].astype(LD)
    T = len(obs)
    rho = np.zeros((T, c.size), dtype=LD)
    rho[obs] = np.asarray(x)[obs].astype(LD) - c - y[obs] @ R
    z = c + wh @ R + rho
    terms = np.abs(c) + np.abs(R).sum(0) + np.abs(rho)
    return z, terms


@functools.lru_cache(maxsize=None)
def case(k, L, diagonal, lengths, mask, r):
    """The reference of one batch: dict of x (fp32 [T, L], NaN rows at missing frames), weight, row_start, y, obs and,
    per sequence concatenated, wp, wh, nis, logdet, logabs, ynorm [T] = max(1, ||y||_inf of the frame's sequence),
    z, terms.  Computed once and shared; read-only."""
    m = model(k, L, diagonal)
    T = int(sum(lengths))
    x = np.array(WO.make_corpus((max(300, L + 100),), L)[7:7 + T])
    weight = weights_for(mask, lengths)
    y, obs = observe(x, weight, m)
    x[~obs] = np.nan
    rt = noise_of(r, weight)
    rs = WO.row_start(lengths)
    parts = [kalman_rts(y[a:b], obs[a:b], rt[a:b], m["A"], m["B"], diagonal) for a, b in zip(rs[:-1], rs[1:])]
    out = {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    out["ynorm"] = np.concatenate([np.full(b - a, max(1.0, float(np.abs(y[a:b]).max()))) for a, b in zip(rs[:-1], rs[1:])])
    out["z"], out["terms"] = latent_rows(x, obs, y, out["wh"], m)
    out.update(x=x, weight=weight, row_start=rs, y=y, obs=obs, model=m)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ---- the splice ------------------------------------------------------------------------------------------------------

def splice_gain(n_out, ranges, fade):
    """g [n_out] float64: 1 inside a range, 0.5 + 0.5 cos(pi d / (fade + 1)) at distance 1 <= d <= fade from the
    nearest one, 0 beyond (the maximum over the ranges, sample by sample)."""
    n = np.arange(n_out)
    g = np.zeros(n_out)
    for s, e in ranges:
        d = np.where(n < s, s - n, np.where(n >= e, n - e + 1, 0))
        gr = np.where(d == 0, 1.0, np.where(d <= fade, 0.5 + 0.5 * np.cos(np.pi * d / (fade + 1.0)), 0.0))
        g = np.maximum(g, gr)
    return g


def splice(src, frames, ranges, fade):
    """(expected [n] float64, g [n])"""
    g = splice_gain(len(src), ranges, fade)
    return (1 - g) * np.asarray(src, np.float64) + g * np.asarray(frames, np.float64), g


# ---- mask and regions, sample by sample and frame by frame -------------------------------------------------------------

def frame_mask(n_samples, S, hop, ranges):
    """bool [frames]: frame f holds a damaged sample.  hop None: non-overlapping frames of the zero-padded file."""
    step = S if hop is None else hop
    padded = -(-n_samples // step) * step
    n_frames = padded // step - S // step + 1
    bad = np.zeros(max(padded, S) + S, dtype=bool)
    for s, e in ranges:
        bad[max(s, 0):max(e, 0)] = True
    return np.array([bad[f * step:f * step + S].any() for f in range(n_frames)], dtype=bool)


def regions(mask, context):
    """[(f0, f1)]: the runs of the frames within `context` frames of a missing one."""
    n = len(mask)
    near = np.array([bool(np.any(mask[max(0, f - context):f + context + 1])) for f in range(n)] + [False])
    out, start = [], None
    for f in range(n + 1):
        if near[f] and start is None:
            start = f
        if not near[f] and start is not None:
            out.append((start, f))
            start = None
    return out
