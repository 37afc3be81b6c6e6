"""numpy float64 oracle of the latent PCA (include/rawvae_hip.h, "Latent PCA"): the test inputs, the blocked mean, the
covariance, the cyclic Jacobi in the kernel's pair order with its stopping rule, and the three apply forms.

The Jacobi here applies a step's rotations as whole-row and whole-column updates (all rows first, then all columns);
the kernel orders the two rotations of every 2 x 2 block by pair number.  Both are the same similarity transform, so
the oracle restates the algorithm (order of pairs, rotation formulas, stopping rule), not the kernel's bits.
"""
import functools

import numpy as np

U = 2.0 ** -52
MEAN_ROWS = 256
MAX_SWEEPS = 40


@functools.lru_cache(maxsize=None)
def make_latents(N, L):
    """x [N, L] fp32 with a geometric spectrum 3 .. 1e-3 in a random rotation, means that are not small against the
    spread, a collapsed dimension (column 1 = 0.25: its fp64 sums are exact, so its variance is exactly 0) from L = 3
    and a duplicated one (column 5 = column 4: an exactly singular covariance) from L = 64.  Read-only."""
    rng = np.random.default_rng(L)
    sig = np.geomspace(3, 1e-3, L)
    Q = np.linalg.qr(rng.standard_normal((L, L)))[0]
    x = (rng.standard_normal((N, L)) * sig) @ Q + rng.uniform(-3, 3, L)
    if L >= 3:
        x[:, 1] = 0.25
    if L >= 64:
        x[:, 5] = x[:, 4]
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def blocked_mean(x):
    """fp64 column means in the kernel's order: blocks of 256 rows, each added in ascending t from +0, the block sums
    added in ascending block order from +0, one division by N."""
    x64 = np.asarray(x, dtype=np.float64)
    N, L = x64.shape
    total = np.zeros(L)
    for b0 in range(0, N, MEAN_ROWS):
        acc = np.zeros(L)
        for row in x64[b0:b0 + MEAN_ROWS]:
            acc = acc + row
        total = total + acc
    return total / N


@functools.lru_cache(maxsize=None)
def covariance(N, L):
    """numpy.cov of make_latents(N, L) in float64 (ddof = 1).  Read-only."""
    c = np.atleast_2d(np.cov(make_latents(N, L).astype(np.float64), rowvar=False))
    c.setflags(write=False)
    return c


def pair_order(n, s):
    """(p [n / 2], q [n / 2]), p < q: the disjoint pairs of step s of the round-robin order over n (even) indices:
    {n - 1, s} and {(s + m) mod (n - 1), (s - m) mod (n - 1)} for m = 1 .. n / 2 - 1."""
    m = np.arange(1, n // 2)
    a = np.concatenate([[n - 1], (s + m) % (n - 1)])
    b = np.concatenate([[s], (s - m) % (n - 1)])
    return np.minimum(a, b), np.maximum(a, b)


def jacobi(C, max_sweeps=MAX_SWEEPS):
    """(eigenvalues descending, components with row j the j-th eigenvector, sweeps, converged) of a symmetric C by the
    cyclic Jacobi of the kernel: pair order, rotation formulas, off-diagonal norm summed directly, the stop at
    L 2^-52 ||C||_F or max_sweeps, descending order, the sign rule."""
    A = np.array(C, dtype=np.float64)
    L = A.shape[0]
    n = (L + 1) & ~1
    Vt = np.eye(L)
    thr = L * U * np.sqrt((A * A).sum())
    offmask = ~np.eye(L, dtype=bool)
    sweeps, converged = 0, False
    for sweep in range(max_sweeps + 1):
        if np.sqrt((A[offmask] ** 2).sum()) <= thr:
            converged = True
            break
        if sweep == max_sweeps:
            break
        for s in range(n - 1):
            p, q = pair_order(n, s)
            ok = q < L
            p, q = p[ok], q[ok]
            app, aqq, apq = A[p, p], A[q, q], A[p, q]
            rot = apq != 0
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                theta = (aqq - app) / (2 * apq)
                t = np.where(theta < 0, -1.0, 1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1))
            t = np.where(rot, t, 0.0)
            c = 1 / np.sqrt(t * t + 1)
            sn = t * c
            Ap, Aq = A[p, :].copy(), A[q, :].copy()
            A[p, :], A[q, :] = c[:, None] * Ap - sn[:, None] * Aq, sn[:, None] * Ap + c[:, None] * Aq
            Ap, Aq = A[:, p].copy(), A[:, q].copy()
            A[:, p], A[:, q] = c * Ap - sn * Aq, sn * Ap + c * Aq
            A[p, p], A[q, q] = app - t * apq, aqq + t * apq
            A[p, q] = A[q, p] = np.where(rot, 0.0, apq)
            Vp, Vq = Vt[p, :].copy(), Vt[q, :].copy()
            Vt[p, :], Vt[q, :] = c[:, None] * Vp - sn[:, None] * Vq, sn[:, None] * Vp + c[:, None] * Vq
        sweeps = sweep + 1
    lam = np.diag(A).copy()
    order = np.argsort(-lam, kind="stable")
    return lam[order], apply_sign_rule(Vt[order]), sweeps, converged


def apply_sign_rule(rows):
    """Each row with its entry of largest magnitude positive (exact ties: the lowest index)."""
    rows = np.array(rows, dtype=np.float64)
    lead = np.argmax(np.abs(rows), axis=1)     # argmax returns the first of equal maxima
    flip = rows[np.arange(rows.shape[0]), lead] < 0
    rows[flip] *= -1
    return rows


def eigh_descending(C):
    """numpy.linalg.eigh with the eigenvalues descending and the eigenvectors as rows under the sign rule."""
    lam, V = np.linalg.eigh(np.asarray(C, dtype=np.float64))
    return lam[::-1].copy(), apply_sign_rule(V[:, ::-1].T)


def project(x, comp, centre):
    """(y float64 [N, k], sum of |terms| [N, k])"""
    d = np.asarray(x, dtype=np.float64) - centre
    return d @ comp.T, np.abs(d) @ np.abs(comp.T)


def reconstruct(y, comp, centre):
    """(x^ float64 [N, L], sum of |terms| [N, L]); the centre counts as a term"""
    y = np.asarray(y, dtype=np.float64)
    return centre + y @ comp, np.abs(centre) + np.abs(y) @ np.abs(comp)


def edit(x, comp, centre, lam, gains, shifts):
    """(x' float64 [N, L], sum of |terms| [N, L]) with the coordinates unrounded"""
    x = np.asarray(x, dtype=np.float64)
    y, ay = project(x, comp, centre)
    g1 = np.asarray(gains, dtype=np.float64) - 1
    hs = np.asarray(shifts, dtype=np.float64) * np.sqrt(np.maximum(lam, 0))
    coef = g1 * y + hs
    return x + coef @ comp, np.abs(x) + (np.abs(g1) * ay + np.abs(hs)) @ np.abs(comp)
