"""numpy float64 oracle of the latent walk (include/rawvae_hip.h, "Latent walk"): time-correlated multi-file corpora,
the lag-1 moment over the frame pairs of one file, the whitened dynamics with numpy.linalg.eigh for Q, and the step (in
numpy.longdouble, so that its own rounding is far below the bounds the fp64 kernels are held to)."""
import functools

import numpy as np

U = 2.0 ** -53
RANK_TOL = 1e-12

# (file lengths, L): one pair; a one-row file; a file boundary exactly on and just off a 4096-pair range edge; a 64-wide
# tile edge; many ranges
CORPORA = [((2,), 1), ((1, 2, 5), 3), ((100, 1, 156), 17), ((4096, 2, 300), 70), ((4095, 3), 65),
           ((2500, 3000, 3500), 256)]


def row_start(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def make_corpus(lengths, L):
    """x [T, L] fp32: per file an AR(1) process per axis, persistences spread over (-0.5, 0.995), a geometric spectrum
    3 .. 3e-2 in a random rotation, a mean that is not small against the spread.  Every file restarts from a stationary
    draw, so consecutive files are unrelated.  Read-only."""
    rng = np.random.default_rng(1000 * L + len(lengths))
    rho = np.linspace(0.995, -0.5, L) if L > 1 else np.array([0.9])
    sig = np.geomspace(3, 3e-2, L)
    rot = np.linalg.qr(rng.standard_normal((L, L)))[0]
    mean = rng.uniform(-2, 2, L)
    files = []
    for n in lengths:
        s = np.empty((n, L))
        s[0] = rng.standard_normal(L)
        for t in range(1, n):
            s[t] = rho * s[t - 1] + np.sqrt(1 - rho * rho) * rng.standard_normal(L)
        files.append(s)
    x = ((np.concatenate(files) * sig) @ rot + mean).astype(np.float32)
    x.setflags(write=False)
    return x


def pair_mask(rs, T):
    """keep [T - 1] bool: rows t and t + 1 lie in one file."""
    keep = np.ones(T - 1, dtype=bool)
    inner = np.asarray(rs)[1:-1]
    keep[inner[(inner >= 1) & (inner <= T - 1)] - 1] = False
    return keep


def lagcov(x, rs, centre):
    """C1 [L, L] = (1 / (T - 1)) sum d[t+1]^T d[t] over the pairs of one file, d = x64 - centre."""
    d = np.asarray(x, dtype=np.float64) - np.asarray(centre, dtype=np.float64)
    T = d.shape[0]
    keep = pair_mask(rs, T)
    return d[1:][keep].T @ d[:-1][keep] / (T - 1)


def moments(x):
    x64 = np.asarray(x, dtype=np.float64)
    c = x64.mean(0)
    return c, np.atleast_2d(np.cov(x64, rowvar=False))


def axes(C0):
    """(lambda descending, V with row j the j-th eigenvector, rank) of the covariance."""
    lam, V = np.linalg.eigh(C0)
    lam, V = lam[::-1].copy(), V[:, ::-1].T.copy()
    return lam, V, int(np.count_nonzero(lam > RANK_TOL * lam[0]))


def dynamics(C1, V, lam, k, diagonal=False):
    """dict of P, R [k, L], A, Q, B [k, k], terms = |P| |C1| |P|^T (the sum of |terms| of every element of A),
    q (eigenvalues of Q; full mode) from the first k axes."""
    V, lam = np.asarray(V, dtype=np.float64)[:k], np.asarray(lam, dtype=np.float64)[:k]
    s = np.sqrt(lam)
    P, R = V / s[:, None], V * s[:, None]
    A = P @ C1 @ P.T
    terms = np.abs(P) @ np.abs(C1) @ np.abs(P).T
    Q = np.eye(k) - A @ A.T
    Q = np.triu(Q) + np.triu(Q, 1).T
    if diagonal:
        a = np.diag(A)
        return dict(P=P, R=R, A=np.diag(a), Afull=A, Q=Q, B=np.diag(np.sqrt(np.maximum(1 - a * a, 0))), terms=terms)
    q, Uq = np.linalg.eigh(Q)
    return dict(P=P, R=R, A=A, Afull=A, Q=Q, q=q, B=Uq * np.sqrt(np.maximum(q, 0)), terms=terms)


def fit(x, rs, k=None, diagonal=False):
    """The whole fit in numpy; k = None keeps every axis of the rank."""
    c, C0 = moments(x)
    lam, V, r = axes(C0)
    k = r if k is None else k
    assert 1 <= k <= r
    m = dynamics(lagcov(x, rs, c), V, lam, k, diagonal)
    m.update(centre=c, lam=lam[:k], V=V[:k], rank=r, C0=C0)
    return m


def closure(A, B):
    """||A A^T + B B^T - I||_F"""
    return float(np.linalg.norm(A @ A.T + B @ B.T - np.eye(A.shape[0])))


def run(A, B, R, centre, eps, temperature=1.0, offset=None, w0=None):
    """n frames of one stream in longdouble.  eps [n, k]; w0 None: not primed (w = e at the first frame).
    -> (w [n, k], z [n, L], drive [n] = || |A||w_prev| + |B||e| ||_2 per frame (|e| where the state was drawn),
        zterms [n, L] = |c| + |offset| + sum_j |w_j R_jl|), as float64 arrays."""
    ld = np.longdouble
    A, B, R, c = (np.asarray(a, dtype=np.float64).astype(ld) for a in (A, B, R, centre))
    off = np.zeros(c.size, dtype=ld) if offset is None else np.asarray(offset, dtype=np.float32).astype(ld)
    e_all = ld(np.float32(temperature)) * np.asarray(eps, dtype=np.float32).astype(ld)
    w = None if w0 is None else np.asarray(w0).astype(ld)
    ws, zs, drive, zterms = [], [], [], []
    for e in e_all:
        if w is None:
            drive.append(np.linalg.norm(np.abs(e).astype(np.float64)))
            w = e.copy()
        else:
            drive.append(np.linalg.norm((np.abs(A) @ np.abs(w) + np.abs(B) @ np.abs(e)).astype(np.float64)))
            w = A @ w + B @ e
        ws.append(w.astype(np.float64))
        zs.append((c + off + w @ R).astype(np.float64))
        zterms.append((np.abs(c) + np.abs(off) + np.abs(w) @ np.abs(R)).astype(np.float64))
    return np.array(ws), np.array(zs), np.array(drive), np.array(zterms)
