"""Float64 numpy batch SOM: the yardstick of rawaudiovae_kelsey_amd/som.py and csrc/som.hip (tests/test_som_*.py).

Plain restatement of the algorithm in LatentSOM's doc, with every quantity in float64 and no tiling."""
import numpy as np

import mosaic_oracle


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


def bmu_exact(x, w):
    """(best int32, second int32, d_best fp32, d_second fp32) as rv_som_bmu writes them, to the bit: the search's fp32
    distance (mosaic_oracle.sq_dist, csrc/sqdist.h) and the first two nodes in (distance, index) order.  A node whose
    distance is NaN is never taken; where fewer than two remain the slot is -1 / +inf."""
    idx, dist = mosaic_oracle.knn(x, w, 2)
    return idx[:, 0].astype(np.int32), idx[:, 1].astype(np.int32), dist[:, 0].copy(), dist[:, 1].copy()


def node_sums(x, best, M):
    """(sums [M, L] float64, counts [M] int64).  np.add.at is unbuffered: it adds the rows one by one in ascending row
    order, each node's sum starting from +0 -- k_som_node_sums's order, so the sums are the kernel's bit for bit.  Rows
    whose entry lies outside [0, M) belong to no node."""
    x = np.asarray(x, np.float64)
    best = np.asarray(best).astype(np.int64)
    ok = (best >= 0) & (best < M)
    sums = np.zeros((M, x.shape[1]))
    np.add.at(sums, best[ok], x[ok])
    counts = np.bincount(best[ok], minlength=M).astype(np.int64)
    return sums, counts


def segment_mean(x, offsets):
    """[F, L] float32 as rv_segment_mean writes it: per segment the float64 sum of its rows in ascending order from +0,
    divided by their number, rounded to float32 once."""
    x = np.asarray(x, np.float32)
    offsets = np.asarray(offsets, np.int64)
    out = np.empty((offsets.size - 1, x.shape[1]), np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        for f in range(offsets.size - 1):
            s = np.zeros(x.shape[1], np.float64)
            for r in range(int(offsets[f]), int(offsets[f + 1])):
                s = s + x[r].astype(np.float64)
            out[f] = (s / np.float64(offsets[f + 1] - offsets[f])).astype(np.float32)
    return out


def neighbourhood(rows, cols, sigma):
    m = np.arange(rows * cols)
    r, c = m // cols, m % cols
    d2 = (r[:, None] - r[None, :]) ** 2 + (c[:, None] - c[None, :]) ** 2
    with np.errstate(divide="ignore", over="ignore", under="ignore", invalid="ignore"):   # 0 / 0 at d2 = 0: masked
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
