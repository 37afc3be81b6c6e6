"""numpy float64 restatement, bit for bit, of the fp64 statistics and chains of the latent PCA and the latent walk
(include/rawvae_hip.h, "Latent PCA" and "Latent walk"; csrc/moment.h, csrc/pca.hip, csrc/walk.hip).

Every fma goes through states_oracle.fma (an error-free product and sum), every other operation is one IEEE float64
operation of numpy's, in the order the header gives.  What the device adds to this is nothing: a zero staged for a row
or column beyond the data leaves an accumulator that started at +0 as it is, and v_mfma_f64_16x16x4_f64 adds its four
rows one after the other (tests/states_oracle.py, which tests/test_states_gpu.py holds the device to).

  covariance_bits / lagcov_bits   the second moments of RV_PCA_MOMENTS and RV_PCA_LAGCOV.  A `schedule` (the rows of
                                  every range in the order they are added) and, for the lag-1 moment, a `keep` mask may
                                  be given: tests/test_moment_oracle_cpu.py builds deliberately wrong restatements from
                                  them and checks that the test inputs tell each from the right one.
  apply_bits                      RV_PCA_APPLY's three modes
  walk_fit_bits, walk_noise_bits, walk_diagonal_bits     RV_WALK_FIT's three modes
  walk_step_bits                  RV_WALK_STEP's state and latent rows
and the cases the GPU tests (tests/test_moment_edges_gpu.py) and the CPU tests share.
"""
import functools

import numpy as np

import pca_oracle as PO
import walk_oracle as WO
from states_oracle import CHUNK, RANGE, fma

PROJECT, RECONSTRUCT, EDIT = 0, 1, 2          # RV_PCA_APPLY's mode
LISTED_ROWS = (0, 15, 16, 63, 64, 65, 127, 128, 255, 256, 257)     # and L - 1: what a wide case compares
FULL_LIMIT = 3e7                              # the whole matrix is compared where T L L <= this

# RV_PCA_MOMENTS: (T, L)
MOMENT_CASES = ((2, 1), (33, 63), (4095, 64), (4096, 65), (4097, 129), (8193, 17), (300, 257), (4097, 321), (300, 511),
                (300, 512))
# RV_PCA_LAGCOV: (file lengths, L).  Every set of file lengths and every width the tests must cover occurs: the
# pair alone; one-row files; a file end exactly on a range edge of 4096 pairs (4096, 2, 300), one before it (4095, 3)
# and one after it (4097, 1, 4095, which also fills the second range to its last pair), each at one tile a side and at
# more; a single file of three ranges; and the two widest with T = 700 and a file end inside.
LAG_CASES = (((2,), 3), ((1, 1, 2), 3), ((1, 1, 2), 65), ((4096, 2, 300), 70), ((4096, 2, 300), 129), ((4095, 3), 65),
             ((4095, 3), 70), ((4097, 1, 4095), 65), ((4097, 1, 4095), 129), ((8194,), 65), ((300, 1, 399), 321),
             ((257, 443), 512))
# The cases whose input has uncorrelated columns (white_rows) instead of the correlated corpus of pca_oracle /
# walk_oracle: see white_rows.
WHITE_MOMENTS = ((4095, 64), (8193, 17))
WHITE_LAGS = (((4097, 1, 4095), 65), ((4097, 1, 4095), 129), ((8194,), 65))


def compared_rows(T, L):
    """The rows of an [L, L] moment of T rows that a test compares (over all columns): all of them, or the listed ones"""
    if T * L * L <= FULL_LIMIT:
        return np.arange(L)
    return np.array(sorted({r for r in LISTED_ROWS + (L - 1,) if r < L}))


def default_schedule(n):
    """The rows (pairs) 0 .. n - 1 of every range of 4096, each range in ascending order"""
    return [list(range(r0, min(r0 + RANGE, n))) for r0 in range(0, n, RANGE)]


def range_partials(operands, shape, schedule, reuse=None):
    """One partial per range: acc = fma(a, b, acc) over the range's rows in the schedule's order from +0, (a, b) =
    operands(t).  reuse = (a schedule, its partials): a range whose rows are the same list is taken from there."""
    out = []
    for r, rows in enumerate(schedule):
        if reuse is not None and r < len(reuse[0]) and reuse[0][r] == rows:
            out.append(reuse[1][r])
            continue
        acc = np.zeros(shape)
        for t in rows:
            a, b = operands(t)
            acc = fma(a, b, acc)
        out.append(acc)
    return out


def range_total(partials, shape, divisor):
    """The partials in ascending range order from +0, then the one division"""
    total = np.zeros(shape)
    for p in partials:
        total = total + p
    return total / divisor


def _rows(rows, L):
    return np.arange(L) if rows is None else np.asarray(rows, np.int64)


def covariance_operands(x, rows=None, mirror=True):
    """(operands(t), shape) of the covariance of x [T, L] about pca_oracle.blocked_mean: element (i, j >= i) has
    d[t, i] on the left and d[t, j] on the right; (i, j < i) is the value of (j, i), so d[t, j] is on its left (mirror
    False: d[t, i] on the left everywhere)."""
    x64 = np.asarray(x, np.float64)
    d = x64 - PO.blocked_mean(x)
    rows = _rows(rows, d.shape[1])
    upper = np.arange(d.shape[1])[None, :] >= rows[:, None]

    def operands(t):
        a, b = d[t, rows][:, None], d[t][None, :]
        return (np.where(upper, a, b), np.where(upper, b, a)) if mirror else (a, b)
    return operands, (rows.size, d.shape[1])


def covariance_bits(x, rows=None, schedule=None, mirror=True):
    """RV_PCA_MOMENTS' covariance [len(rows), L] of x [T, L] fp32, bit for bit."""
    T = np.asarray(x).shape[0]
    operands, shape = covariance_operands(x, rows, mirror)
    return range_total(range_partials(operands, shape, schedule or default_schedule(T)), shape, float(T - 1))


def lagcov_operands(x, row_start, centre, rows=None, keep=None):
    """(operands(p), shape) of the lag-1 moment over the T - 1 pairs: d[p + 1, i] on the left, d[p, j] on the right or +0
    where walk_oracle.pair_mask (or `keep`) drops the pair."""
    d = np.asarray(x, np.float64) - np.asarray(centre, np.float64)
    rows = _rows(rows, d.shape[1])
    keep = WO.pair_mask(row_start, d.shape[0]) if keep is None else keep
    zero = np.zeros(d.shape[1])

    def operands(p):
        return d[p + 1, rows][:, None], (d[p] if keep[p] else zero)[None, :]
    return operands, (rows.size, d.shape[1])


def lagcov_bits(x, row_start, centre, rows=None, schedule=None, keep=None):
    """RV_PCA_LAGCOV's C1 [len(rows), L] of x [T, L] fp32 about the given centre, bit for bit."""
    T = np.asarray(x).shape[0]
    operands, shape = lagcov_operands(x, row_start, centre, rows, keep)
    return range_total(range_partials(operands, shape, schedule or default_schedule(T - 1)), shape, float(T - 1))


# ---- deliberately wrong schedules -----------------------------------------------------------------------------------

def swapped(schedule, p):
    """rows p and p + 1 (of one range) added in swapped order"""
    out = [list(r) for r in schedule]
    r, i = divmod(p, RANGE)
    out[r][i], out[r][i + 1] = out[r][i + 1], out[r][i]
    return out


def dropped(schedule, p):
    """row p left out"""
    out = [list(r) for r in schedule]
    out[p // RANGE].remove(p)
    return out


def edge_moved(schedule, r, back):
    """The edge between ranges r and r + 1 off by one: the last row of range r added first in range r + 1 (back), or
    the first row of range r + 1 added last in range r."""
    out = [list(x) for x in schedule]
    if back:
        out[r + 1].insert(0, out[r].pop())
    else:
        out[r].append(out[r + 1].pop(0))
    return out


def reversed_groups(schedule):
    """every full group of four rows (an MFMA's) added in reverse order"""
    out = []
    for rows in schedule:
        full = len(rows) // 4 * 4
        out.append([t for g in range(0, full, 4) for t in rows[g:g + 4][::-1]] + list(rows[full:]))
    return out


def swap_positions(n):
    """Where two adjacent rows p | p + 1 are swapped: rows 0 | 1, the edge between two MFMAs (four rows each) and the
    edge between two chunks nearest the middle of the first range, and the last two rows of every range."""
    mid = min(n, RANGE) // 2
    at = {0, mid // 4 * 4 + 3, mid // CHUNK * CHUNK + CHUNK - 1}
    at |= {min(r0 + RANGE, n) - 2 for r0 in range(0, n, RANGE)}
    return sorted(p for p in at if 0 <= p and p + 1 < n and p // RANGE == (p + 1) // RANGE)


def drop_positions(n):
    """Which row is dropped: the last of the first full chunk of 32, the last of the last full chunk, the last row"""
    return sorted({p for p in (CHUNK - 1, n // CHUNK * CHUNK - 1, n - 1) if 0 <= p < n})


# ---- RV_PCA_APPLY -----------------------------------------------------------------------------------------------------

def _chain(a_of, b_of, n, shape):
    acc = np.zeros(shape)
    for i in range(n):
        acc = fma(a_of(i), b_of(i), acc)
    return acc


def project_chain(x, comp, centre):
    """y [T, k] float64, unrounded: fma(d_l, v_jl, .) in ascending l from +0, d = (double)x - centre"""
    d = np.asarray(x, np.float32).astype(np.float64) - centre
    return _chain(lambda l: d[:, l][:, None], lambda l: comp[:, l][None, :], d.shape[1], (d.shape[0], comp.shape[0]))


def apply_bits(mode, q, comp, centre, lam=None, g=None, h=None, coords=None):
    """RV_PCA_APPLY's out (fp32) for q [T, L] (PROJECT, EDIT) or [T, k] (RECONSTRUCT), comp [k, L], centre [L] and, for
    EDIT, the eigenvalues lam [k] and the fp32 gains g and shifts h [k].  coords: project_chain(q, comp, centre) where
    the caller has it already."""
    comp, centre = np.asarray(comp, np.float64), np.asarray(centre, np.float64)
    k, L = comp.shape
    q = np.asarray(q, np.float32)
    if mode != RECONSTRUCT and coords is None:
        coords = project_chain(q, comp, centre)
    if mode == PROJECT:
        return coords.astype(np.float32)
    if mode == RECONSTRUCT:
        coef = q.astype(np.float64)
    else:
        g1 = np.asarray(g, np.float32).astype(np.float64) - 1.0
        hs = np.asarray(h, np.float32).astype(np.float64) * np.sqrt(np.maximum(np.asarray(lam, np.float64), 0.0))
        coef = fma(g1[None, :], coords, hs[None, :])
    acc = _chain(lambda j: coef[:, j][:, None], lambda j: comp[j][None, :], k, (q.shape[0], L))
    if mode == RECONSTRUCT:
        return (centre + acc).astype(np.float32)
    return np.where(acc == 0.0, q, (q.astype(np.float64) + acc).astype(np.float32))      # a sum of exactly zero: x itself


# ---- RV_WALK_FIT ------------------------------------------------------------------------------------------------------

def chain_product(X, Y, block=64, threads=8):
    """out[i, j] = the chain fma(X[i, l], Y[l, j], .) in ascending l from +0.  The elements are independent, so blocks of
    columns run on a few threads (numpy's loops release the interpreter lock); 512 x 512 x 512 takes a second or two."""
    from concurrent.futures import ThreadPoolExecutor
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)

    def columns(j0):
        Yb = np.ascontiguousarray(Y[:, j0:j0 + block])
        return _chain(lambda l: X[:, l][:, None], lambda l: Yb[l][None, :], X.shape[1], (X.shape[0], Yb.shape[1]))
    starts = range(0, Y.shape[1], block)
    if len(starts) == 1:
        return columns(0)
    with ThreadPoolExecutor(threads) as pool:
        return np.concatenate(list(pool.map(columns, starts)), axis=1)


def walk_fit_bits(V, lam, C1, k):
    """RV_WALK_DYNAMICS: dict(A [k, k], Q [k, k], P [k, L], R [k, L]) of the components V, their eigenvalues lam and the
    lag-1 moment C1 [L, L].  M = P C1, A = M P^T and A A^T each as one ascending fma chain per element; Q from i <= j."""
    V, lam, C1 = np.asarray(V, np.float64)[:k], np.asarray(lam, np.float64)[:k], np.asarray(C1, np.float64)
    L = V.shape[1]
    s = np.sqrt(lam)[:, None]
    P, R = V / s, s * V
    M = chain_product(P, C1)
    A = chain_product(M, P.T)
    Q = np.eye(k) - chain_product(A, A.T)
    return dict(A=A, Q=np.triu(Q) + np.triu(Q, 1).T, P=P, R=R)


def walk_fit_packed(res):
    """result of RV_WALK_DYNAMICS: [A | Q | P | R]"""
    return np.concatenate([res[name].ravel() for name in ("A", "Q", "P", "R")])


def walk_noise_bits(A, U, q):
    """RV_WALK_NOISE: [A^T | B^T] [2, k, k], B^T[j, i] = sqrt(max(q_j, 0)) u_j[i] (U's row j the j-th eigenvector)"""
    A, U, q = (np.asarray(a, np.float64) for a in (A, U, q))
    return np.stack([A.T, np.sqrt(np.maximum(q, 0.0))[:, None] * U])


def walk_diagonal_bits(A):
    """RV_WALK_DIAGONAL: [A^T | B^T] [2, k, k] of the diagonal model: a_jj and sqrt(max(fma(-a_jj, a_jj, 1), 0))"""
    a = np.diag(np.asarray(A, np.float64)).copy()
    return np.stack([np.diag(a), np.diag(np.sqrt(np.maximum(fma(-a, a, np.ones_like(a)), 0.0)))])


# ---- RV_WALK_STEP -----------------------------------------------------------------------------------------------------

def walk_step_bits(dyn, R, centre, offset, temperature, eps, w0, primed):
    """n frames of every stream: dyn = [A^T | B^T] [2, k, k], R [k, L], centre [L] float64; offset [streams, L] and
    temperature [streams] fp32; eps [streams, n, k] fp32; w0 [streams, k] float64 and primed [streams] (bool) before the
    first frame.  -> (w [streams, n, k] float64 after every frame, z [streams, n, L] fp32).
    A stream that is not primed takes w = e = (double)temperature (double)eps; afterwards w'_i is the chain
    fma(A[i, j], w_j, .) over ascending j from +0 continued by fma(B[i, j], e_j, .); z_l = (float)(centre_l +
    (double)offset_l + chain_j fma(w_j, R[j, l], .))."""
    dyn, R, centre = (np.asarray(a, np.float64) for a in (dyn, R, centre))
    At, Bt = dyn[0], dyn[1]
    k, L = R.shape
    eps = np.asarray(eps, np.float32).astype(np.float64)
    off = np.asarray(offset, np.float32).astype(np.float64)
    temp = np.asarray(temperature, np.float32).astype(np.float64)
    ns, n = eps.shape[:2]
    w = np.array(w0, np.float64).reshape(ns, k)
    pr = np.array(primed, bool).reshape(ns)
    ws, zs = np.empty((ns, n, k)), np.empty((ns, n, L), np.float32)
    for f in range(n):
        e = temp[:, None] * eps[:, f]
        acc = np.zeros((ns, k))
        for j in range(k):
            acc = fma(At[j][None, :], w[:, j][:, None], acc)
        for j in range(k):
            acc = fma(Bt[j][None, :], e[:, j][:, None], acc)
        w = np.where(pr[:, None], acc, e)
        pr[:] = True
        lat = _chain(lambda j: w[:, j][:, None], lambda j: R[j][None, :], k, (ns, L))
        ws[:, f], zs[:, f] = w, (centre[None, :] + off + lat).astype(np.float32)
    return ws, zs


# ---- the test inputs --------------------------------------------------------------------------------------------------

def white_rows(T, L):
    """x [T, L] fp32 with independent columns, scales 2 .. 0.5 and means in (-1, 1).  One swapped pair of rows inside a
    chain of thousands changes one rounding, and that shows in the result only where a later rounding falls differently
    for it: in a few elements of a thousand on the correlated corpora (every element's sum grows with the leading
    axis's), and in none of the compared ones for some swaps of the cases listed in WHITE_MOMENTS and WHITE_LAGS.  With
    independent columns the off-diagonal sums grow like sqrt(t), ten times as many elements show a swap, and with this
    seed every instance of tests/test_moment_oracle_cpu.py shows in those cases too."""
    rng = np.random.default_rng(10007 * T + L + 1)
    return (rng.standard_normal((T, L)) * np.geomspace(2, 0.5, L) + rng.uniform(-1, 1, L)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def moment_input(T, L):
    """x [T, L] fp32 of a RV_PCA_MOMENTS case: pca_oracle.make_latents, or white_rows.  Read-only."""
    if (T, L) not in WHITE_MOMENTS:
        return PO.make_latents(T, L)
    x = white_rows(T, L)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def lag_input(lengths, L):
    """(x [T, L] fp32, row_start, centre = the blocked mean) of a RV_PCA_LAGCOV case: walk_oracle.make_corpus, or
    white_rows.  Read-only."""
    x = white_rows(sum(lengths), L) if (lengths, L) in WHITE_LAGS else WO.make_corpus(lengths, L)
    rs, c = WO.row_start(lengths), PO.blocked_mean(x)
    for a in (x, rs, c):
        a.setflags(write=False)
    return x, rs, c


@functools.lru_cache(maxsize=None)
def rotation(L, seed=0):
    """A random orthonormal [L, L] (rows), float64.  Read-only."""
    q = np.linalg.qr(np.random.default_rng(77 * L + seed).standard_normal((L, L)))[0]
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def apply_input(L, T=9):
    """(x [T, L] fp32, centre [L], eigenvalues [L] descending, gains and shifts [L] fp32) for RV_PCA_APPLY on the rows
    of rotation(L).  Read-only."""
    rng = np.random.default_rng(500 + L)
    x = rng.normal(0, 1.5, (T, L)).astype(np.float32)
    centre = rng.uniform(-2, 2, L)
    lam = np.geomspace(3.0, 1e-3, L)
    g, h = rng.uniform(0, 2, L).astype(np.float32), rng.uniform(-2, 2, L).astype(np.float32)
    g[0] = 1.0                                        # an axis whose coordinate enters through the shift alone
    for a in (x, centre, lam, g, h):
        a.setflags(write=False)
    return x, centre, lam, g, h


@functools.lru_cache(maxsize=None)
def fit_input(k, L):
    """(V [k, L] orthonormal rows, lam [k] > 0, C1 [L, L]) for RV_WALK_FIT: no corpus behind them.  Read-only."""
    rng = np.random.default_rng(900 + 7 * k + L)
    V = rotation(L, 1)[:k]
    lam = np.geomspace(2.0, 0.05, k)
    C1 = rng.standard_normal((L, L)) * 0.3 / np.sqrt(L)
    for a in (lam, C1):
        a.setflags(write=False)
    return V, lam, C1


@functools.lru_cache(maxsize=None)
def noise_input(k):
    """(A [k, k], U [k, k] orthonormal rows, q [k] with negative and zero entries) for RV_WALK_NOISE and _DIAGONAL; the
    diagonal of A holds 1, -1 (b = 0), a value a hair above 1 (the clamp, from k = 3) and values inside (-1, 1)."""
    rng = np.random.default_rng(1300 + k)
    A = rng.uniform(-0.95, 0.95, (k, k))
    for i, v in enumerate((1.0, -1.0, 1.0 + 2.0 ** -40)[:k]):
        A[i, i] = v
    q = rng.uniform(0, 1, k)
    q[::3] = -q[::3] * 1e-12
    if k > 1:
        q[1] = 0.0
    U = rotation(k, 2)
    for a in (A, q):
        a.setflags(write=False)
    return A, U, q


@functools.lru_cache(maxsize=None)
def step_input(L, k, streams=3, frames=8):
    """(dyn [2, k, k] with ||A||_2 = 0.95, R [k, L], centre [L], offset [streams, L] fp32, temperature [streams] fp32,
    eps [streams, frames, k] fp32) for RV_WALK_STEP.  Read-only."""
    rng = np.random.default_rng(1700 + 3 * L + k)
    A = rotation(k, 3) @ (np.linspace(0.95, 0.2, k)[:, None] * rotation(k, 4))
    B = rng.standard_normal((k, k)) / np.sqrt(k)
    dyn = np.stack([A.T, B.T]).copy()
    R = np.geomspace(1.5, 0.1, k)[:, None] * rotation(L, 5)[:k]
    centre = rng.uniform(-2, 2, L)
    offset = rng.uniform(-0.5, 0.5, (streams, L)).astype(np.float32)
    offset[0] = 0
    temperature = np.array([1.0, 0.7, 1.3], np.float32)[:streams]
    eps = rng.standard_normal((streams, frames, k)).astype(np.float32)
    for a in (dyn, R, centre, offset, temperature, eps):
        a.setflags(write=False)
    return dyn, R, centre, offset, temperature, eps
