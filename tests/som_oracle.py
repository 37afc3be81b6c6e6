"""Float64 numpy batch SOM: the yardstick of rawaudiovae_kelsey_amd/som.py and csrc/som.hip (tests/test_som_*.py).

Plain restatement of the algorithm in LatentSOM's doc, with every quantity in float64 and no tiling."""
import numpy as np


def sq_dists(x, w, chunk=4096):
    """[N, M] float64 squared distances, exact-ish: sum over l of (x - w)^2, chunked over rows."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    out = np.empty((x.shape[0], w.shape[0]))
    for i in range(0, x.shape[0], chunk):
        xc = x[i:i + chunk]
        # ||x||^2 - 2 x.w + ||w||^2 in float64: only used to shortlist candidates, whose distances bmu() recomputes
        out[i:i + chunk] = (xc * xc).sum(1)[:, None] - 2.0 * xc @ w.T + (w * w).sum(1)[None, :]
    return np.maximum(out, 0.0)


def direct_dist(x, w, idx):
    """float64 sum_l (x[n, l] - w[idx[n], l])^2 for each row n."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    return ((x - w[np.asarray(idx)]) ** 2).sum(1)


def bmu(x, w, chunk=4096):
    """(best, second, d_best, d_second): the 8 nearest nodes by the float64 expansion, then their direct float64
    distances ordered by (distance, node index), so ties go to the lower index."""
    x = np.asarray(x, np.float64)
    w = np.asarray(w, np.float64)
    N, M = x.shape[0], w.shape[0]
    k = min(M, 8)
    best = np.empty(N, np.int64)
    second = np.empty(N, np.int64)
    for i in range(0, N, chunk):
        xc = x[i:i + chunk]
        cand = np.argpartition(sq_dists(xc, w), k - 1, axis=1)[:, :k]
        dd = ((xc[:, None, :] - w[cand]) ** 2).sum(-1)
        order = np.lexsort((cand, dd), axis=-1)
        r = np.arange(xc.shape[0])
        best[i:i + chunk], second[i:i + chunk] = cand[r, order[:, 0]], cand[r, order[:, 1]]
    return best, second, direct_dist(x, w, best), direct_dist(x, w, second)


def node_sums(x, best, M):
    x = np.asarray(x, np.float64)
    sums = np.zeros((M, x.shape[1]))
    np.add.at(sums, np.asarray(best), x)
    counts = np.bincount(np.asarray(best), minlength=M).astype(np.int64)
    return sums, counts


def neighbourhood(rows, cols, sigma):
    m = np.arange(rows * cols)
    r, c = m // cols, m % cols
    d2 = (r[:, None] - r[None, :]) ** 2 + (c[:, None] - c[None, :]) ** 2
    with np.errstate(divide="ignore", over="ignore", under="ignore"):
        return np.where(d2 == 0, 1.0, np.exp(-d2 / (2.0 * sigma * sigma)))


def update(sums, counts, w_old, rows, cols, sigma):
    h = neighbourhood(rows, cols, sigma)
    num = h @ np.asarray(sums, np.float64)
    den = h @ np.asarray(counts, np.float64)
    out = np.array(w_old, np.float64, copy=True)
    nz = den != 0
    out[nz] = num[nz] / den[nz, None]
    return out


def sigma_schedule(sigma0, sigma1, epochs):
    if epochs == 1:
        return np.array([float(sigma0)])
    t = np.arange(epochs, dtype=np.float64)
    return sigma0 * (sigma1 / sigma0) ** (t / (epochs - 1))


def fit(x, rows, cols, sigma0=None, sigma1=0.5, epochs=50, seed=0):
    """-> (weights [M, L] float64, final best [N]) of the batch SOM from LatentSOM's initialisation."""
    x = np.asarray(x)
    N = x.shape[0]
    M = rows * cols
    sigma0 = max(rows, cols) / 2.0 if sigma0 is None else sigma0
    w = np.asarray(x[np.random.default_rng(seed).choice(N, M, replace=N < M)], np.float64)
    for s in sigma_schedule(sigma0, sigma1, epochs):
        best = bmu(x, w)[0]
        sums, counts = node_sums(x, best, M)
        w = update(sums, counts, w, rows, cols, s)
    return w, bmu(x, w)[0]


def blobs(n_per, centers, spread, seed):
    """Well-separated Gaussian clusters: ([K * n_per, L] float32, labels)."""
    rng = np.random.default_rng(seed)
    centers = np.asarray(centers, np.float64)
    x = np.concatenate([c + spread * rng.standard_normal((n_per, centers.shape[1])) for c in centers])
    return x.astype(np.float32), np.repeat(np.arange(len(centers)), n_per)
