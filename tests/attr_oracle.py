"""numpy restatement of the latent-attribute ops (include/rawvae_hip.h, "Latent attributes").

  describe(wave, hop, T, S, window, R, dtype=np.float64)   RV_ATTR_DESCRIBE in float64: the yardstick of every column
  describe(..., dtype=np.float32)                          the same with the spectral part (the powers, the floor and the
                                                           add Pa + fl) by eval_oracle's FLOAT32 restatement of the very
                                                           algorithm the kernel runs; its disagreement with the float64
                                                           run is what float32 costs: the yardstick of columns 3 and 4
                                                           (tests/test_attributes_gpu.py).  Columns 0..2 are float64 in both.
  fit(x, c, P, D, lam)                                     RV_ATTR_FIT in float64 through numpy.linalg.solve
  move(B, R, rows, delta)                                  LatentAttributes.move's algebra
  signals(S, T, seed), latents(T, L, seed), whitening(x, k)    the inputs of the tests
"""
import numpy as np

import eval_oracle as E

NAMES = ("level", "zcr", "crest", "centroid", "flatness")
KINDS = ("noise", "on-bin sine", "off-bin sine", "dc", "impulse", "quiet noise", "silence")
PIVOT = 2.0 ** -40


def describe(wave, hop, T, S, window=None, R=60.0, dtype=np.float64):
    """[T, 5] float64 (columns 3, 4 NaN-free only with a window; without one [T, 3])"""
    rt = dtype
    x = E.rows_of(wave, hop, T, S)
    x64 = x.astype(np.float64)
    out = np.zeros((T, 3 if window is None else 5), dtype=np.float64)
    with np.errstate(all="ignore"):
        e = (x64 * x64).sum(axis=1) / S
        out[:, 0] = 10.0 * np.log10(e)
        if S > 1:
            out[:, 1] = ((x[:, 1:] < 0) != (x[:, :-1] < 0)).sum(axis=1) / (S - 1)
        p = np.fmax.reduce(np.abs(x64), axis=1, initial=0.0)
        out[:, 2] = np.where(e == 0, np.nan, 10.0 * np.log10(p * p / e))
        if window is None:
            return out
        N = S // 2
        w = np.asarray(window, dtype=np.float32)
        a = (w * x).astype(np.float32)                       # fl32(w x): the header's definition, in both precisions
        Pa = E.powers(a, E.twiddles(S, rt), rt)
        scale = rt(np.float32(10.0 ** (-float(np.float32(R)) / 10.0)))
        k = np.arange(N + 1, dtype=np.float64)
        for t in range(T):
            pa = Pa[t]
            bad = not np.all(np.isfinite(pa))
            fl = rt(np.fmax.reduce(np.where(np.isfinite(pa), pa, 0), initial=0.0)) * scale
            padd = pa + fl
            assert padd.dtype == rt
            p64 = pa.astype(np.float64)
            num, den = (k * p64).sum(), p64.sum()
            A = p64[1:].sum() / N
            G = np.exp(np.log(padd[1:].astype(np.float64)).sum() / N)
            out[t, 3] = np.nan if den == 0 else num / den / S
            out[t, 4] = np.nan if A == 0 else 10.0 * np.log10(G / A)
            if bad:
                out[t, 3:] = np.nan
    return out


def spectral_errors(got, f64):
    """[T, 2]: the error measures of columns 3 and 4: the difference in cycles/sample and in dB; NaN where float64 is NaN"""
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(got, dtype=np.float64)[:, 3:5] - f64[:, 3:5])


def signals(S, T, seed, hop=None):
    """(wave, hop): T frames cycling through KINDS.  hop = S: the frames side by side; hop < S: one waveform whose
    stretches of 3 S samples are of one kind each, so overlapping frames straddle two kinds."""
    rng = np.random.default_rng(seed)

    def one(kind, length):
        m = np.arange(length)
        if kind == 0:
            return rng.uniform(-1, 1, length)
        if kind == 1:
            return 0.8 * np.sin(2 * np.pi * int(rng.integers(2, S // 4)) * m / S + 0.3)
        if kind == 2:
            return 0.8 * np.sin(2 * np.pi * (rng.integers(2, S // 4) + 0.37) * m / S)
        if kind == 3:
            return np.full(length, 0.5)
        if kind == 4:
            v = np.zeros(length)
            v[S // 2::S] = 1.0    # one unit sample per frame length, where a Hann window of a frame that starts at 0 is 1
            return v
        if kind == 5:
            return 1e-4 * rng.uniform(-1, 1, length)
        return np.zeros(length)

    if hop is None or hop == S:
        return np.concatenate([one(t % len(KINDS), S) for t in range(T)]).astype(np.float32), S
    total = (T - 1) * hop + S
    parts = [one(i % len(KINDS), 3 * S) for i in range(-(-total // (3 * S)))]
    return np.concatenate(parts)[:total].astype(np.float32), hop


def bin_of_sine(S, b, phase=0.3):
    return (0.8 * np.sin(2 * np.pi * b * np.arange(S) / S + phase)).astype(np.float32)


# ---- the fit ---------------------------------------------------------------------------------------------------------

def layout(k, N):
    o, at = {}, 0
    for name, n in (("n", 1), ("ybar", k), ("dbar", N), ("Cdd", N * N), ("B", N * k), ("r2", N)):
        o[name] = slice(at, at + n)
        at += n
    return o, at


def observed(x, D):
    return np.isfinite(x).all(axis=1) & np.isfinite(D).all(axis=1)


def cholesky_status(G):
    """0, or 2 when a pivot of the left-looking Cholesky of G is not above 2^-40 of its diagonal element"""
    k = G.shape[0]
    Rm = np.zeros((k, k))
    for j in range(k):
        s = G[j, j] - Rm[j, :j] @ Rm[j, :j]
        if not s > PIVOT * G[j, j]:
            return 2
        Rm[j, j] = np.sqrt(s)
        Rm[j + 1:, j] = (G[j + 1:, j] - Rm[j + 1:, :j] @ Rm[j, :j]) / Rm[j, j]
    return 0


def fit(x, c, P, D, lam=0.0):
    """dict(n, ybar, dbar, Cyy, Cdy, Cdd, B, r2, status, cond) of x [T, L] float32, c [L], P [k, L], D [T, N] float64"""
    x = np.asarray(x, dtype=np.float32)
    D = np.asarray(D, dtype=np.float64)
    k, N = P.shape[0], D.shape[1]
    lam = float(np.float32(lam))
    obs = observed(x, D)
    n = int(obs.sum())
    Y = (x[obs].astype(np.float64) - c) @ P.T
    Dd = D[obs]
    out = dict(n=n, status=0, B=np.zeros((N, k)), r2=np.zeros(N), cond=np.inf)
    with np.errstate(all="ignore"):
        out["ybar"], out["dbar"] = Y.sum(axis=0) / n, Dd.sum(axis=0) / n
        Yc, Dc = Y - out["ybar"], Dd - out["dbar"]
        out["Cyy"], out["Cdy"], out["Cdd"] = Yc.T @ Yc / (n - 1), Dc.T @ Yc / (n - 1), Dc.T @ Dc / (n - 1)
    if n < k + 2:
        out["status"] = 1
        return out
    G = out["Cyy"] + lam * np.eye(k)
    out["status"] = cholesky_status(G)
    if out["status"]:
        return out
    out["cond"] = np.linalg.cond(G)
    for a in range(N):
        cdd = out["Cdd"][a, a]
        if cdd == 0:
            continue
        g = out["Cdy"][a]
        beta = np.linalg.solve(G, g)
        out["B"][a] = beta
        out["r2"][a] = 1.0 - (cdd - 2.0 * (beta @ g) + beta @ out["Cyy"] @ beta) / cdd
    return out


def pack(res):
    return np.concatenate([[res["n"]], res["ybar"], res["dbar"], res["Cdd"].ravel(), res["B"].ravel(), res["r2"]])


def latents(T, L, seed=0):
    """x [T, L] float32: correlated Gaussian rows with a decaying spectrum (condition number of the whitened
    covariance about 1)"""
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((L, L)) / np.sqrt(L) + np.eye(L)
    scale = 1.0 / (1.0 + 0.05 * np.arange(L))
    return ((rng.standard_normal((T, L)) * scale) @ mix + rng.standard_normal(L)).astype(np.float32)


def whitening(x, k):
    """(c [L], P [k, L], lam [k], V [k, L]) float64: the leading principal axes of the finite rows of x, P's rows
    v_j / sqrt(lambda_j)"""
    x64 = np.asarray(x, dtype=np.float64)
    x64 = x64[np.isfinite(x64).all(axis=1)]
    c = x64.mean(axis=0)
    lam, V = np.linalg.eigh(np.cov(x64, rowvar=False).reshape(x64.shape[1], x64.shape[1]))
    order = np.argsort(lam)[::-1][:k]
    lam, V = lam[order], V[:, order].T
    return c, V / np.sqrt(lam)[:, None], lam, V


def move(B, R, rows, delta):
    """(offset [L] float64, predicted [N], norm) of w = M^T (M M^T)^-1 delta, M = B[rows]"""
    M = B[list(rows)]
    w = M.T @ np.linalg.solve(M @ M.T, np.asarray(delta, dtype=np.float64)) if len(rows) else np.zeros(B.shape[1])
    return R.T @ w, B @ w, float(np.sqrt(w @ w))
