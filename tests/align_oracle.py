"""Float64 restatement of the alignment ops (csrc/align.hip, rawaudiovae_kelsey_amd/align.py) for the tests: the band,
the cell rule, the backtrack and the three timelines of include/rawvae_hip.h, "Latent alignment", over
mosaic_oracle.sq_dist's fp32 matrix.  The DP runs one anti-diagonal at a time on the whole [Ta, Tb] matrix with +inf
outside the band: a cell outside the band and a blocked cell are the same thing to their neighbours (C = +inf, never a
winner)."""
import numpy as np

from mosaic_oracle import sq_dist

GLOBAL, SUBSEQUENCE = 0, 1
ON_A, ON_B, ON_PATH = 0, 1, 2
INF = np.inf


def centre(i, Ta, Tb):
    return (np.asarray(i, dtype=np.int64) * (Tb - 1)) // max(Ta - 1, 1)


def band_width(Tb, r):
    return 2 * r + 1 if r else Tb


def in_band(Ta, Tb, r):
    """[Ta, Tb] bool: the cells of the band (r = 0: all)."""
    if not r:
        return np.ones((Ta, Tb), bool)
    j = np.arange(Tb)[None, :]
    return np.abs(j - centre(np.arange(Ta), Ta, Tb)[:, None]) <= r


def admits(Ta, Tb, r):
    """The header's rule for whether the band holds a monotone path from (0, 0) to (Ta - 1, Tb - 1)."""
    if not r:
        return True
    if Ta == 1:
        return Tb - 1 <= r
    return -(-(Tb - 1) // (Ta - 1)) <= 2 * r + 1


def banded(full, r, fill=INF):
    """[Ta, Tb] -> the band layout [Ta, W]; slots whose j falls outside [0, Tb) hold `fill`."""
    Ta, Tb = full.shape
    if not r:
        return full.copy()
    out = np.full((Ta, 2 * r + 1), fill, full.dtype)
    for i in range(Ta):
        c = int(centre(i, Ta, Tb))
        lo, hi = max(0, c - r), min(Tb - 1, c + r)
        out[i, lo - c + r:hi - c + r + 1] = full[i, lo:hi + 1]
    return out


def local_costs(a, b, r=0, rows=64):
    """(Dm [Ta, W] fp32 as RV_ALIGN_COST writes it, the full matrix [Ta, Tb] fp32 with +inf outside the band).  With a
    band, sq_dist is asked only for the columns the band of each chunk of `rows` rows touches."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    Ta, Tb = a.shape[0], b.shape[0]
    if not r:
        full = sq_dist(a, b)
    else:
        full = np.full((Ta, Tb), np.float32(INF), np.float32)
        for i0 in range(0, Ta, rows):
            i1 = min(Ta, i0 + rows)
            lo, hi = max(0, int(centre(i0, Ta, Tb)) - r), min(Tb - 1, int(centre(i1 - 1, Ta, Tb)) + r)
            full[i0:i1, lo:hi + 1] = sq_dist(a[i0:i1], b[lo:hi + 1])
        full = np.where(in_band(Ta, Tb, r), full, np.float32(INF)).astype(np.float32)
    return banded(full, r, np.float32(INF)), full


def forward(full, mode=GLOBAL, penalty=0.0):
    """The DP over the full matrix (fp32, +inf outside the band) -> (C [Ta, Tb] fp64, step [Ta, Tb] uint8)."""
    Ta, Tb = full.shape
    p = float(np.float32(penalty))
    dd = full.astype(np.float64)
    blocked = ~(dd < INF)                      # NaN or +inf
    Cp = np.full((Ta + 1, Tb + 1), INF)        # C[i, j] at Cp[i + 1, j + 1]: the border is "outside the matrix"
    step = np.full((Ta, Tb), 3, np.uint8)
    for d in range(Ta + Tb - 1):
        i = np.arange(max(0, d - (Tb - 1)), min(Ta - 1, d) + 1)
        j = d - i
        cands = [Cp[i, j], Cp[i, j + 1] + p, Cp[i + 1, j] + p]
        if mode == SUBSEQUENCE:
            cands[2] = np.where(i == 0, INF, cands[2])
        best = np.full(i.size, INF)
        st = np.full(i.size, 3, np.uint8)
        for k, c in enumerate(cands):
            win = c < best
            best = np.where(win, c, best)
            st = np.where(win, np.uint8(k), st)
        start = (i == 0) if mode == SUBSEQUENCE else (i == 0) & (j == 0)
        with np.errstate(invalid="ignore"):
            c = np.where(st == 3, INF, dd[i, j] + best)
        c = np.where(start, dd[i, j], c)
        st = np.where(start, np.uint8(3), st)
        c = np.where(blocked[i, j], INF, c)
        st = np.where(blocked[i, j], np.uint8(3), st)
        Cp[i + 1, j + 1] = c
        step[i, j] = st
    return Cp[1:, 1:].copy(), step


def backtrack(full, C, step, mode=GLOBAL):
    """-> dict(path [Ta + Tb - 1, 2] int32 (-1 beyond P), P, choice [4] int32, cost [2] fp64, end_costs [Tb] fp64)."""
    Ta, Tb = full.shape
    cap = Ta + Tb - 1
    path = np.full((cap, 2), -1, np.int32)
    last = C[Ta - 1]
    if mode == SUBSEQUENCE:
        finite = last < INF
        jend = int(np.argmin(np.where(finite, last, INF))) if finite.any() else 0
    else:
        jend = Tb - 1
    cend = C[Ta - 1, jend]
    if not cend < INF:
        return dict(path=path, P=0, choice=np.array([0, -1, -1, 0], np.int32), cost=np.array([INF, 0.0]), end_costs=last)
    cells, i, j = [], Ta - 1, jend
    while len(cells) < cap:
        cells.append((i, j))
        s = int(step[i, j])
        if s > 2:
            break
        i, j = (i if s == 2 else i - 1), (j if s == 1 else j - 1)
        if i < 0 or j < 0:
            break
    cells.reverse()
    P = len(cells)
    path[:P] = cells
    acc = 0.0
    for i, j in cells:
        acc = acc + float(full[i, j])
    return dict(path=path, P=P, choice=np.array([P, cells[0][1], cells[-1][1], 1], np.int32),
                cost=np.array([cend, acc]), end_costs=last)


def align(a, b, r=0, mode=GLOBAL, penalty=0.0):
    """Everything the three ops produce for a, b: local_costs, forward and backtrack in one dict (plus dm, full)."""
    dm, full = local_costs(a, b, r)
    C, step = forward(full, mode, penalty)
    out = backtrack(full, C, step, mode)
    out.update(dm=dm, full=full, C=C, step=step)
    return out


def warp(path, P, Ta, Tb, timeline):
    """idx [n, 2] int32 of RV_ALIGN_WARP."""
    cap = Ta + Tb - 1
    if timeline == ON_PATH:
        return path[:cap].astype(np.int32).copy()
    own = 0 if timeline == ON_A else 1
    n = Ta if timeline == ON_A else Tb
    out = np.full((n, 2), -1, np.int32)
    for m in range(P - 1, -1, -1):         # descending, so the lowest m of a row is the one that stays
        out[path[m, own]] = path[m]
    return out


# ---- inputs ----

def random_latents(T, L, seed):
    return np.random.RandomState(seed).randn(T, L).astype(np.float32)


def binary_latents(T, L, seed):
    """0/1-valued rows: every distance is a small integer and many accumulated costs tie exactly."""
    return np.random.RandomState(seed).randint(0, 2, size=(T, L)).astype(np.float32)


def planted_warp(Ta, L, seed):
    """(a [Ta, L], b = a with each row repeated 1-3 times, the path [P, 2]): the only path of cost 0 (a's rows are
    distinct, so D(a_i, b_j) = 0 exactly where b_j is a copy of a_i), known without any DP."""
    rs = np.random.RandomState(seed)
    a = rs.randn(Ta, L).astype(np.float32)
    a[:, 0] = np.arange(Ta, dtype=np.float32)           # distinct rows, whatever the draw
    reps = rs.randint(1, 4, size=Ta)
    src = np.repeat(np.arange(Ta), reps)
    b = a[src].copy()
    path = np.stack([src, np.arange(src.size)], 1).astype(np.int32)
    return a, b, path
