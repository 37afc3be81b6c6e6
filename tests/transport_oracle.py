"""numpy oracle of the latent transport (include/rawvae_hip.h, "Latent transport"): entropic optimal transport between two
clouds of whitened latent rows.

The whitening chain is states_oracle's float64 restatement, bit for bit.  Everything that passes through exp and log is
numpy.longdouble with float64 results, the cost in its DIFFERENCE form c_ij = sum_d (a_id - b_jd)^2: softmin, the barycentric
map with its diagnostics, and the Sinkhorn loop under the schedule of rawaudiovae_kelsey_amd/transport.py.  epsilon is the
float32 the device reads, widened.

The ceilings.  The device computes c in Gram form, |a|^2 + |b|^2 - 2 a.b, whose rounding is about u (|a|^2 + |b|^2) however
close the two points are; divided by epsilon that is the error of a score.  With a slack of 8 over the k + 8 roundings of a
score, for row i

    delta_s(i) = 8 (k + 8) 2^-53 (1 + C_i / eps),   C_i = |a_i|^2 + max_j |b_j|^2

bounds |d f_i| / eps (a soft minimum moves by no more than its scores do); 4 delta_s max_j |V_j|_inf bounds |d T_id| (a
softmax's weights move by at most twice the scores' error, relatively, in numerator and denominator); 8 delta_s bounds the
relative error of support (two such ratios) and 4 delta_s max_j c_ij + 8 (k + 8) 2^-53 C_i that of cbar (the weights, then
the Gram form's own error in c).  A measured error above its ceiling is a defect.

The gates.  Each is 4 x the largest error measured on the MI355X against this oracle, as a fraction of its ceiling, over the
cases of tests/test_transport_gpu.py; the case that produced it is written beside it.  No gate exceeds 1: the ceiling holds
as well.
"""
import numpy as np

import states_oracle as SO

LD = np.longdouble
U = 2.0 ** -53
SLAB_MIN, SLABS, COLS = 256, 8, 64     # csrc/transport.hip: the slabs of N columns

# fractions of the ceilings: 4 x the largest measured on the MI355X (the case: k, N, T, eps / mean cost, mask)
GATE_F = 4 * 0.0792        # measured 0.0791 (SOFTMIN k 1, N 515, T 64, eps 100, no mask; MAP's f 0.0771, a slab masked): at
#                            eps = 100 x the mean cost the ceiling is 8 (k + 8) u, and log and exp leave a few u
GATE_T = 4 * 0.0125        # measured 0.0124 (k 1, N 515, T 64, eps 100, no mask)
GATE_SUPPORT = 4 * 0.0130  # measured 0.0130 (k 1, N 515, T 64, eps 100, a slab masked)
GATE_CBAR = 4 * 0.00597    # measured 0.00596 (k 1, N 515, T 64, eps 100, the last column masked)

CASES = ((1, 1, 1), (3, 15, 15), (16, 16, 17), (17, 17, 64), (64, 255, 65), (3, 256, 130), (16, 257, 1), (17, 515, 130),
         (64, 515, 17), (1, 515, 64), (64, 16, 15), (16, 2049, 17))       # (k, N, T); 2049 columns: 7 slabs of 320
EPSILONS = (0.01, 1.0, 100.0)         # x the mean cost
AMOUNTS = (0.0, 0.5, 1.0)             # alpha, one per epsilon (alpha = 0 runs once more at each of the other two)
WHITEN_T, WHITEN_L, WHITEN_K = (1, 63, 64, 65, 130), (4, 70, 256), (1, 3, 17, 64)


def eps32(e):
    return float(np.float32(e))


def slabs(N):
    """(columns of a slab, slabs) of N columns"""
    slab = max(SLAB_MIN, -(-(-(-N // SLABS)) // COLS) * COLS)
    return slab, -(-N // slab)


def whiten(x, c, P):
    """(y [T, k] float64 bit for bit, observed [T] int32)"""
    return SO.whiten(x, c, P), SO.observed(x).astype(np.int32)


def costs(A, B):
    """c [T, N] longdouble in difference form"""
    A, B = np.asarray(A, LD), np.asarray(B, LD)
    c = np.zeros((A.shape[0], B.shape[0]), LD)
    for d in range(A.shape[1]):
        diff = A[:, d][:, None] - B[:, d][None, :]
        c += diff * diff
    return c


def scores(c, h, lw, eps):
    lw = np.asarray(lw, LD)
    with np.errstate(invalid="ignore"):
        s = lw[None, :] + (np.asarray(h, LD)[None, :] - c) / LD(eps)
    s[:, np.isneginf(np.asarray(lw, np.float64))] = -np.inf
    return s


def _weights(s):
    """(m [T], w [T, N], Z [T]) with w = exp(s - m); a row with no finite score has m = -inf, w = 0, Z = 0"""
    m = s.max(axis=1)
    safe = np.where(np.isneginf(m), LD(0), m)
    with np.errstate(under="ignore"):
        w = np.exp(s - safe[:, None])
    return m, w, w.sum(axis=1)


def softmin(A, B, h, lw, eps):
    """f [T] float64 = -eps (m + log Z); +inf for a row with no column of finite weight"""
    m, _, Z = _weights(scores(costs(A, B), h, lw, eps))
    with np.errstate(divide="ignore"):
        f = -LD(eps) * (m + np.log(Z))
    return np.where(np.isneginf(m), np.inf, f).astype(np.float64)


def transport_map(y, V, g, lw, eps):
    """dict of float64 f, support, cbar [T] and T [T, k], and the longdouble c [T, N] (for the ceilings)"""
    c = costs(y, V)
    m, w, Z = _weights(scores(c, g, lw, eps))
    with np.errstate(all="ignore"):
        f = np.where(np.isneginf(m), np.inf, -LD(eps) * (m + np.log(Z)))
        Tm = (w @ np.asarray(V, LD)) / Z[:, None]
        support = Z * Z / (w * w).sum(axis=1)
        cbar = (w * c).sum(axis=1) / Z
    return dict(f=f.astype(np.float64), support=support.astype(np.float64), cbar=cbar.astype(np.float64),
                T=Tm.astype(np.float64), T_ld=Tm, c=c)


def moved(x, y, T_ld, W, alpha):
    """x' [T, L] longdouble: x + alpha W (T - y) (before its rounding to float32)"""
    return np.asarray(x, LD) + LD(alpha) * ((T_ld - np.asarray(y, LD)) @ np.asarray(W, LD).T)


def delta_s(A, B, eps, k):
    """The ceiling of a score's error for every row [T]"""
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    C = (A * A).sum(axis=1) + (B * B).sum(axis=1).max()
    return 8 * (k + 8) * U * (1 + C / eps), C


def unwhitening(P):
    return np.ascontiguousarray(np.linalg.solve(P @ P.T, P).T)


def mean_cost(a, b):
    """the mean of c_ij over all pairs of the observed rows a and b, from the first and second moments"""
    return float((a * a).sum(axis=1).mean() + (b * b).sum(axis=1).mean() - 2.0 * (a.mean(axis=0) * b.mean(axis=0)).sum())


def log_weights(obs):
    obs = np.asarray(obs) != 0
    with np.errstate(divide="ignore"):
        return np.where(obs, -np.log(float(obs.sum())), -np.inf)


def schedule(epsilon, cost, level_iters):
    target = eps32(epsilon * cost)
    levels, l = [], 0
    while cost * 2.0 ** -l > target and l < 64:
        levels.append((eps32(cost * 2.0 ** -l), int(level_iters)))
        l += 1
    return levels, target


def marginal_error(g_prev, g, lwt, eps):
    bt = np.exp(lwt)
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.where(bt > 0, np.abs(np.exp((g_prev - g) / eps) - 1.0), 0.0)
    return float((bt * d).sum())


def sinkhorn(ys, lws, yt, lwt, epsilon=0.05, iters=500, tol=1e-3, level_iters=10, check_every=10, cost=None):
    """The loop of LatentTransport.fit on whitened clouds -> dict f, g, epsilon, history [(iteration, error)], n_iter, err"""
    if cost is None:
        cost = mean_cost(ys[~np.isneginf(lws)], yt[~np.isneginf(lwt)])
    levels, target = schedule(epsilon, cost, level_iters)
    f, g = np.zeros(ys.shape[0]), np.zeros(yt.shape[0])
    cst, csT = costs(ys, yt), None
    csT = cst.T

    def half(c, h, lw, eps):
        m, _, Z = _weights(scores(c, h, lw, eps))
        with np.errstate(divide="ignore"):
            return np.where(np.isneginf(m), np.inf, -LD(eps) * (m + np.log(Z))).astype(np.float64)

    n_iter, history, err = 0, [], float("inf")
    for eps, n in levels:
        for _ in range(n):
            f = half(cst, g, lwt, eps)
            g = half(csT, f, lws, eps)
            n_iter += 1
    for i in range(1, iters + 1):
        prev = g
        f = half(cst, g, lwt, target)
        g = half(csT, f, lws, target)
        n_iter += 1
        if i % check_every == 0 or i == iters:
            err = marginal_error(prev, g, lwt, target)
            history.append((n_iter, err))
            if err <= tol:
                break
    return dict(f=f, g=g, epsilon=target, history=history, n_iter=n_iter, err=err, cost=cost)


def plan(ys, lws, yt, lwt, f, g, eps):
    """The plan P_ij = exp(lws_i + lwt_j + (f_i + g_j - c_ij) / eps) [Ns, Nt] longdouble"""
    with np.errstate(invalid="ignore", under="ignore"):
        e = (np.asarray(lws, LD)[:, None] + np.asarray(lwt, LD)[None, :]
             + (np.asarray(f, LD)[:, None] + np.asarray(g, LD)[None, :] - costs(ys, yt)) / LD(eps))
    e[np.isneginf(np.asarray(lws, np.float64))] = -np.inf
    e[:, np.isneginf(np.asarray(lwt, np.float64))] = -np.inf
    return np.exp(e)


# ---- the cases ------------------------------------------------------------------------------------------------------------

def masks(N):
    """{name: bool [N], True = the column has weight}: none masked, the first, the last, a whole slab"""
    out = {"none": np.ones(N, bool)}
    if N > 1:
        first, last = np.ones(N, bool), np.ones(N, bool)
        first[0], last[-1] = False, False
        out["first"], out["last"] = first, last
    slab, n = slabs(N)
    if n > 1:
        whole = np.ones(N, bool)
        whole[:slab] = False
        out["slab"] = whole
    return out


def case(k, N, T, seed=0):
    """Two clouds of a case: A [T, k] (row 0 of T > 1 rows 10^3 standard deviations out), B [N, k] off to one side, the
    columns' potential h [N] and the mean cost between them"""
    rng = np.random.default_rng(100003 * k + 101 * N + T + seed)
    A = rng.standard_normal((T, k))
    if T > 1:
        A[0] = 1e3 * np.sign(rng.standard_normal(k))
    B = rng.standard_normal((N, k)) * 0.7 + 1.5 / np.sqrt(k)
    cost = 2.0 * k
    h = rng.standard_normal(N) * 0.1 * cost
    return A, B, h, cost


def map_case(k, N, T, seed=0):
    """x [T, L] fp32 whose whitened rows are case()'s A (to float32's rounding), with the basis and its un-whitening"""
    A, B, h, cost = case(k, N, T, seed)
    L = min(512, k + 3)
    c, P = SO.basis(k, L)
    W = unwhitening(P)
    x = (c[None, :] + A @ W.T).astype(np.float32)
    return x, c, P, W, B, h, cost


def lattice_case(k, N, T, seed=0):
    """Distinct points V [N, k] of the integer lattice and queries V_j + o with |o_d| <= 0.25 -> (Q [T, k], V, nearest [T]).
    Two lattice points differ by >= 1 in some coordinate, so the second-nearest column's cost exceeds the nearest's by
    >= (1 - 0.25)^2 - 0.25^2 = 0.5; at eps = 2^-11 its exponent is <= -1024 and its weight an exact 0 in float64."""
    rng = np.random.default_rng(7 * k + 13 * N + T + seed)
    side = int(np.ceil(N ** (1.0 / k))) + 1
    rest = rng.choice(min(side ** k, 1 << 40), N, replace=False).astype(np.int64)
    digits = []
    for _ in range(k):
        digits.append(rest % side)
        rest = rest // side
    V = np.stack(digits, axis=1).astype(np.float64) - side // 2
    assert len({tuple(v) for v in V}) == N
    near = rng.integers(0, N, T)
    Q = V[near] + rng.integers(-2, 3, (T, k)) / 8.0
    return Q, V, near
