"""numpy float64 oracle of the switching walk (include/rawvae_hip.h, "Switching walk"): the header's order of every add
written out, every fma through states_oracle.fma, so that what the header calls exact can be compared bit for bit: the
residual, the pairs that count, the moments (one fma per pair in ascending order for the MFMA sums, as the M-step's oracle
does), the dynamics and Q, the guard and [A^T | B^T] given the eigenvectors, and the step.  The eigendecomposition itself is
numpy.linalg.eigh here; the device's is RV_PCA_EIG.
"""
import functools

import numpy as np

import rng_oracle as RNG
import states_oracle as SO
from states_oracle import fma

RANGE, ROWS = 4096, 256     # csrc/moment.h
U = 2.0 ** -53


def phi_layout(S, k):
    o, at = {}, 0
    for name, n in (("m", S * k), ("sd", S * k), ("pi", S), ("A", S * S), ("dyn", S * 2 * k * k)):
        o[name] = slice(at, at + n)
        at += n
    o["doubles"] = at
    return o


def pack_phi(m, sd, pi, A, dyn):
    S, k = m.shape
    o = phi_layout(S, k)
    phi = np.empty(o["doubles"])
    for name, a in (("m", m), ("sd", sd), ("pi", pi), ("A", A), ("dyn", dyn)):
        phi[o[name]] = np.asarray(a, np.float64).ravel()
    return phi


def unpack_phi(phi, S, k):
    o = phi_layout(S, k)
    return dict(m=phi[o["m"]].reshape(S, k), sd=phi[o["sd"]].reshape(S, k), pi=phi[o["pi"]], A=phi[o["A"]].reshape(S, S),
                dyn=phi[o["dyn"]].reshape(S, 2, k, k))


# ---- the fit ------------------------------------------------------------------------------------------------------------

def residual(x, c, P, th, gamma, S, k):
    """(r [T, k], observed [T] uint8): r[t, j] = chain fma(gamma[t, i], fl(fl(y_j - m_ij) sqrt(w_ij)), .) in ascending i from
    +0; +0 in an unobserved frame"""
    p = SO.unpack(th, S, k)
    y, obs = SO.whiten(x, c, P), SO.observed(x)
    sw = np.sqrt(p["w"])
    r = np.zeros_like(y)
    for i in range(S):
        r = fma(gamma[:, i][:, None], (y - p["m"][i][None, :]) * sw[i][None, :], r)
    r[~obs] = 0.0
    return r, obs.astype(np.uint8)


def keep_mask(row_start, obs, T, file_ends=True, gate=True):
    """keep [T - 1]: pair p counts iff p + 1 is none of row_start[0 .. n] and both frames are observed.  file_ends=False and
    gate=False leave a rule out: the wrong orders the tests tell from the right one."""
    keep = np.ones(T - 1, bool)
    if file_ends:
        cuts = np.asarray(row_start, np.int64) - 1
        keep[cuts[(cuts >= 0) & (cuts < T - 1)]] = False
    if gate:
        o = np.asarray(obs, bool)
        keep &= o[:-1] & o[1:]
    return keep


def moments(r, gamma, keep, this_gamma=False):
    """dict(N [S], Dn [S, k] (D'), Dt [S, k] (D), C1 [S, k, k]) in csrc/moment.h's orders: N in blocks of 256 pairs, each in
    ascending p from +0, the blocks in ascending order from +0; the others in ranges of 4096 pairs, one fma per pair in
    ascending p from +0, the ranges in ascending order from +0.  Only the right operand is gated.  this_gamma: gamma_p in
    place of gamma_{p+1} (a wrong rule the tests tell from the right one)."""
    T, S = gamma.shape
    k = r.shape[1]
    n = T - 1
    g = gamma[:-1] if this_gamma else gamma[1:]
    gn = np.where(keep[:, None], g, 0.0)
    N = np.zeros(S)
    for b0 in range(0, n, ROWS):
        acc = np.zeros(S)
        for row in gn[b0:b0 + ROWS]:
            acc = acc + row
        N = N + acc
    rn, rt = r[1:], np.where(keep[:, None], r[:-1], 0.0)
    sq_n = np.where(keep[:, None], r[1:] * r[1:], 0.0)
    sq_t = np.where(keep[:, None], r[:-1] * r[:-1], 0.0)
    Dn, Dt, C1 = np.zeros((S, k)), np.zeros((S, k)), np.zeros((S, k, k))
    for r0 in range(0, n, RANGE):
        an, at, ac = np.zeros((S, k)), np.zeros((S, k)), np.zeros((S, k, k))
        for p in range(r0, min(r0 + RANGE, n)):
            an = fma(g[p][:, None], sq_n[p][None, :], an)
            at = fma(g[p][:, None], sq_t[p][None, :], at)
            left = g[p][:, None] * rn[p][None, :]                       # [S, k]: one rounded product
            ac = fma(left[:, :, None], rt[p][None, None, :], ac)
        Dn, Dt, C1 = Dn + an, Dt + at, C1 + ac
    return dict(N=N, Dn=Dn, Dt=Dt, C1=C1)


def pack_moments(mo):
    return np.concatenate([mo["N"].ravel(), mo["Dn"].ravel(), mo["Dt"].ravel(), mo["C1"].ravel()])


def dynamics(mo):
    """(A [S, k, k], Q [S, k, k], info [S]): A = (C1 / sqrt(D'[a])) / sqrt(D[b]), 0 where a D is not positive and finite, all 0
    where N < 2; Q[i, l] = (i == l) - chain_m fma(A[i, m], A[l, m], .), mirrored"""
    N, Dn, Dt, C1 = mo["N"], mo["Dn"], mo["Dt"], mo["C1"]
    S, k = Dn.shape
    thin = ~(N >= 2.0)
    ok = lambda d: (d > 0) & np.isfinite(d)   # noqa: E731
    with np.errstate(all="ignore"):
        A = (C1 / np.sqrt(Dn)[:, :, None]) / np.sqrt(Dt)[:, None, :]
    good = ok(Dn)[:, :, None] & ok(Dt)[:, None, :] & ~thin[:, None, None]
    A = np.where(good, A, 0.0)
    acc = np.zeros((S, k, k))
    for m in range(k):
        acc = fma(A[:, :, m][:, :, None], A[:, :, m][:, None, :], acc)
    Q = np.eye(k)[None] - acc
    iu = np.triu_indices(k)
    Qs = np.zeros_like(Q)
    Qs[:, iu[0], iu[1]] = Q[:, iu[0], iu[1]]
    Qs[:, iu[1], iu[0]] = Q[:, iu[0], iu[1]]
    return A, Qs, thin.astype(np.int32)


def noise(A, Uv, q):
    """(dyn [S, 2, k, k], g [S]) from A, the eigenvectors (row i the i-th) and q of every Q: the guard, then [A^T | B^T]"""
    S, k, _ = A.shape
    dyn, g = np.zeros((S, 2, k, k)), np.ones(S)
    for s in range(S):
        qmin = q[s].min()
        a, qs = A[s], q[s]
        if qmin < 0:
            h = 1.0 / (1.0 - qmin)
            g[s] = np.sqrt(h)
            a = g[s] * a
            qs = 1.0 - h * (1.0 - qs)
        dyn[s, 0] = a.T
        dyn[s, 1] = np.sqrt(np.maximum(qs, 0.0))[:, None] * Uv[s]
    return dyn, g


def eigh_desc(Q):
    """(q [S, k] descending, U [S, k, k] with row i the i-th eigenvector) by numpy.linalg.eigh, under RV_PCA_EIG's sign: the
    entry of largest magnitude of each eigenvector is positive (ties: the lowest index)"""
    lam, V = np.linalg.eigh(Q)
    Uv = np.ascontiguousarray(np.swapaxes(V, 1, 2)[:, ::-1])
    big = np.take_along_axis(Uv, np.abs(Uv).argmax(axis=2)[:, :, None], axis=2)
    return lam[:, ::-1].copy(), np.where(big < 0, -Uv, Uv)


def fit(x, row_start, c, P, th, gamma, S, k):
    """The whole fit on the host -> dict(r, obs, keep, mo, A, Q, info, dyn, g, phi)"""
    T = x.shape[0]
    r, obs = residual(x, c, P, th, gamma, S, k)
    keep = keep_mask(row_start, obs, T)
    mo = moments(r, gamma, keep)
    A, Q, info = dynamics(mo)
    q, Uv = eigh_desc(Q)
    dyn, g = noise(A, Uv, q)
    p = SO.unpack(th, S, k)
    phi = pack_phi(p["m"], np.sqrt(1.0 / p["w"]), p["pi"], p["A"], dyn)
    return dict(r=r, obs=obs, keep=keep, mo=mo, A=A, Q=Q, info=info, q=q, U=Uv, dyn=dyn, g=g, phi=phi)


def closure(dyn):
    """max over the states of ||A A^T + B B^T - I||_F in long double"""
    worst = 0.0
    for d in dyn:
        A, B = d[0].T.astype(np.longdouble), d[1].T.astype(np.longdouble)
        worst = max(worst, float(np.sqrt(((A @ A.T + B @ B.T - np.eye(A.shape[0])) ** 2).sum())))
    return worst


# ---- the step -----------------------------------------------------------------------------------------------------------

def state_uniform(seed, frame, stream):
    """The fp32 uniform of (seed, stream, absolute frame): the first word of Philox at (lo = frame, hi = 2^32 + stream)"""
    w = RNG.philox4x32_10(seed, np.uint64(frame), np.uint64((1 << 32) + stream))
    return RNG.uniforms(w[:, 0])[0]


def draw_state(law, v):
    cum, last = 0.0, 0
    for j, p in enumerate(law):
        cum = cum + p
        if float(v) < cum:
            return j
        if p > 0:
            last = j
    return last


def step(phi, R, c, S, k, u, primed, cur, eps, uniforms, forced, temp=1.0, offset=None):
    """F frames of one stream: eps [F, k] fp32, uniforms [F] fp32, forced [F] int or None -> (u, cur, path [F], z [F, L] fp32).
    The header's five steps per frame."""
    p = unpack_phi(phi, S, k)
    L = R.shape[1]
    off = np.zeros(L, np.float32) if offset is None else np.asarray(offset, np.float32)
    u = np.array(u, np.float64)
    F = eps.shape[0]
    path, z = np.zeros(F, np.int32), np.zeros((F, L), np.float32)
    t = np.float64(np.float32(temp))
    for f in range(F):
        want = -1 if forced is None else int(forced[f])
        if 0 <= want < S:
            nx = want
        else:
            chain = primed and 0 <= cur < S
            nx = draw_state(p["A"][cur] if chain else p["pi"], np.float32(uniforms[f]))
        e = t * eps[f].astype(np.float64)
        if primed:
            At, Bt = p["dyn"][nx, 0], p["dyn"][nx, 1]
            acc = np.zeros(k)
            for j in range(k):
                acc = fma(At[j], u[j], acc)
            for j in range(k):
                acc = fma(Bt[j], e[j], acc)
            u = acc
        else:
            u = e.copy()
        y = fma(p["sd"][nx], u, p["m"][nx])
        acc = np.zeros(L)
        for j in range(k):
            acc = fma(y[j], R[j], acc)
        z[f] = ((c + off.astype(np.float64)) + acc).astype(np.float32)
        path[f], cur, primed = nx, nx, True
    return u, cur, path, z


# ---- cases --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def moments_case(S, k, T, lengths=None, holes=()):
    """(x [T, L] fp32 with the frames `holes` unobserved, c, P, theta, gamma [T, S], row_start), L = k + 6.  gamma's rows are
    random laws that favour the early states by up to 1e4.  Read-only."""
    L = k + 6
    c, P = SO.basis(k, L)
    x = SO.latents(T, L)
    for h in holes:
        x[h] = np.nan
    th = SO.random_theta(S, k)
    rs = SO.starts(lengths if lengths is not None else [T])
    rng = np.random.default_rng(T + 13 * S + k)
    gamma = rng.uniform(0, 1, (T, S)) * np.geomspace(1, 1e-4, S)
    gamma /= gamma.sum(axis=1, keepdims=True)
    for a in (x, gamma, rs, th):
        a.setflags(write=False)
    return x, c, P, th, gamma, rs


def random_phi(S, k, seed=0, zeros=False):
    """A model block with contractive random dynamics (A A^T + B B^T = I by construction) and a random A_hmm (zeros: with exact
    zeros in a row)"""
    rng = np.random.default_rng(5 * S + k + seed)
    m, sd = rng.normal(0, 2, (S, k)), rng.uniform(0.5, 2, (S, k))
    A = rng.uniform(0.05, 1, (S, S)) + 2 * np.eye(S)
    if zeros and S > 1:
        A[0, 1::2] = 0
        A[S - 1, S - 1] = 0
    pi = rng.uniform(0.2, 1, S)
    dyn = np.zeros((S, 2, k, k))
    for s in range(S):
        a = rng.standard_normal((k, k))
        a *= rng.uniform(0.5, 0.95) / np.linalg.norm(a, 2)
        q, Uv = eigh_desc((np.eye(k) - a @ a.T)[None])
        dyn[s] = noise(a[None], Uv, q)[0][0]
    return pack_phi(m, sd, pi / pi.sum(), A / A.sum(axis=1, keepdims=True), dyn)


@functools.lru_cache(maxsize=None)
def planted(n_files=4, n_frames=3000, S=3, k=2, seed=0):
    """Planted switching data in the whitened coordinates themselves (L = k, P = I, c = 0): S states 8 standard deviations
    apart, self-transition 0.95, distinct contractive A_j.  -> (x fp32, row_start, theta, labels, A_true [S, k, k])"""
    rng = np.random.default_rng(seed)
    m = np.zeros((S, k))
    m[:, 0] = 8.0 * np.arange(S)
    v = np.ones((S, k))
    Ah = np.full((S, S), 0.05 / max(S - 1, 1)) + (0.95 - 0.05 / max(S - 1, 1)) * np.eye(S)
    pi = np.full(S, 1.0 / S)
    rot = lambda a: np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])   # noqa: E731
    At = np.stack([(0.3 + 0.25 * s) * rot(0.4 * s - 0.3) for s in range(S)])
    xs, labels = [], []
    for _ in range(n_files):
        s = rng.integers(S)
        u = rng.standard_normal(k)
        for t in range(n_frames):
            if t:
                s = rng.choice(S, p=Ah[s])
                a = At[s]
                w, V = np.linalg.eigh(np.eye(k) - a @ a.T)
                u = a @ u + (V * np.sqrt(np.maximum(w, 0))) @ rng.standard_normal(k)
            xs.append(m[s] + u)
            labels.append(s)
    x = np.asarray(xs, np.float32)
    rs = SO.starts([n_frames] * n_files)
    th = SO.pack(m, v, pi, Ah)
    labels = np.asarray(labels)
    for a in (x, rs, th, labels, At):
        a.setflags(write=False)
    return x, rs, th, labels, At


@functools.lru_cache(maxsize=None)
def planted_fit():
    """The oracle's fit of planted() under the exact posteriors of its HMM -> (fit dict, N [S])"""
    x, rs, th, labels, At = planted()
    S, k = At.shape[0], At.shape[1]
    c, P = np.zeros(k), np.eye(k)
    logb = SO.emit(x, c, P, th, S, k)
    gamma = SO.forward_backward(logb, rs, th, S, k)[0]
    return fit(x, rs, c, P, th, gamma, S, k)
