"""Float64 restatement of the recurrence ops (csrc/recur.hip, rawaudiovae_kelsey_amd/recur.py) for the tests: the window
sums, the admission rule and the (W, j) order of include/rawvae_hip.h, "Latent recurrence", and the host rules on P and I
(motifs, discords, best loop, the plan of the looped rows), each written from the rule and not from the package's code.
Dm comes from align_oracle.local_costs."""
import numpy as np

MIRROR = 1
INF = np.inf


def window_sums(dm, m):
    """W [n_rows - m + 1, N - m + 1] fp64: W[i, j] = the chain s = +0, s += (double)dm[i + u, j + u] in ascending u, on whole
    diagonally shifted arrays."""
    dm = np.asarray(dm)
    T, J = dm.shape[0] - m + 1, dm.shape[1] - m + 1
    s = np.zeros((T, J), np.float64)
    with np.errstate(invalid="ignore"):
        for u in range(m):
            s = s + dm[u:u + T, u:u + J].astype(np.float64)
    return s


def admitted(T, J, row0, lo, hi, mirror):
    """[T, J] bool: window j is admitted for row i."""
    d = np.arange(J, dtype=np.int64)[None, :] - (row0 + np.arange(T, dtype=np.int64))[:, None]
    ok = (d >= lo) & (d <= hi)
    if mirror:
        ok |= (-d >= lo) & (-d <= hi)
    return ok


def profile(dm, m, row0=0, lo=-(2 ** 31 - 1), hi=2 ** 31 - 1, mirror=0):
    """(P [T] fp64, I [T] int32): over the admitted j whose W is finite the least (W, j); +inf / -1 with none."""
    W = window_sums(dm, m)
    T, J = W.shape
    ok = admitted(T, J, row0, lo, hi, mirror) & np.isfinite(W)
    key = np.where(ok, W, INF)
    I = np.argmin(key, axis=1)                     # the first of equal minima: the lower j
    P = key[np.arange(T), I]
    none = ~ok.any(axis=1)
    return np.where(none, INF, P), np.where(none, -1, I).astype(np.int32)


def _pick(P, I, exclude, K, greatest):
    P = np.asarray(P, np.float64)
    masked = [not np.isfinite(v) for v in P]
    out = []
    for _ in range(K):
        best = None
        for i, v in enumerate(P):
            if masked[i]:
                continue
            if best is None or (v > P[best] if greatest else v < P[best]):
                best = i
        if best is None:
            break
        j = int(I[best])
        out.append((best, j, float(P[best])))
        for r in range(len(P)):
            if abs(r - best) <= exclude or abs(r - j) <= exclude:
                masked[r] = True
    return out


def motifs(P, I, exclude, K):
    return _pick(P, I, exclude, K, False)


def discords(P, I, exclude, K):
    return _pick(P, I, exclude, K, True)


def best_loop(P, I):
    found = _pick(P, I, 0, 1, False)
    return found[0] if found else None


def seam_weights(m):
    return (np.arange(1, m + 1, dtype=np.float64) / (m + 1)).astype(np.float32)


def loop_plan(T, start, end, m, repeats):
    """[(src, other, g)] per output row; other = -1: row src itself."""
    if end + m > T or start < 0:
        raise ValueError("end")
    if end - start < m:
        raise ValueError("start")
    g = seam_weights(m)
    plan = [(r, -1, np.float32(0)) for r in range(end)]
    for _ in range(repeats - 1):
        plan += [(end + u, start + u, g[u]) for u in range(m)]
        plan += [(r, -1, np.float32(0)) for r in range(start + m, end)]
    plan += [(start + u, end + u, g[u]) for u in range(m)]
    plan += [(r, -1, np.float32(0)) for r in range(end + m, T)]
    return plan


def loop_rows(mu, start, end, m, repeats):
    """The looped rows [T + (repeats - 1) (end - start), L] fp32 of mu [T, L] fp32: plain rows copied, a seam row
    fl32(fl32(a wa) + fl32(b wb)) with wb = g and wa = fl32(1 - g): rv_latent_mix under RV_ALPHA_F32."""
    mu = np.asarray(mu, np.float32)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for src, other, g in loop_plan(mu.shape[0], start, end, m, repeats):
            if other < 0:
                out.append(mu[src].copy())
            else:
                wb = np.float32(g)
                wa = np.float32(np.float32(1) - wb)
                out.append((mu[src] * wa).astype(np.float32) + (mu[other] * wb).astype(np.float32))
    return np.stack(out).astype(np.float32)


def brute_profile(dm, m, row0, lo, hi, mirror):
    """The header's rule cell by cell in three loops, sharing nothing with profile()."""
    n_rows, N = dm.shape
    T = n_rows - m + 1
    P, I = np.full(T, INF), np.full(T, -1, np.int32)
    for i in range(T):
        g = row0 + i
        for j in range(N - m + 1):
            if not (lo <= j - g <= hi or (mirror and lo <= g - j <= hi)):
                continue
            s = 0.0
            for u in range(m):
                s = s + float(dm[i + u, j + u])
            if np.isfinite(s) and s < P[i]:
                P[i], I[i] = s, j
    return P, I
