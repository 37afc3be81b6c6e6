"""The loop edges of the rv_mosaic ops from before the guard-band habit (csrc/mosaic*.hip: KNN, KNN_SMALL and their merge,
GATHER_MEAN, OLA, TRANSITION, PATH_*, LIVE without a fit), exactly and between guards: rv_mosaic calls (_lib.mosaic_call)
on pointers cut from tests/guarded.py buffers, against mosaic_oracle and mosaic_path_oracle bit for bit.

  - every output lies between sentinel guards and is checked with assert_untouched after the call;
  - every workspace is a guarded buffer of EXACTLY the bytes its *_WORKSPACE op reports, at the alignment the op demands
    (the caching allocator would round a bare tensor up to 512 bytes and hide an op that under-reports);
  - every float input lies between NaN guards, EXCEPT a corpus (c, mu): its back guard is attractive.  NaN never wins a
    search and a NaN transition is +inf, exactly what a missing candidate gives, so a corpus row read at an index >= N
    would pass unseen behind NaN.  The search's corpus has copies of the query rows there (distance 0: the row wins and
    the comparison fails on an index >= N), the transitions' mu copies of its own rows (a finite cost where the oracle
    has +inf);
  - integer inputs have no NaN: their guards hold values the kernel would act on visibly.

Shapes are the smallest that take a loop into another trip or another path; the workload shapes are in
test_mosaic_gpu.py and test_mosaic_path_gpu.py."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import mosaic_oracle as O  # noqa: E402
import mosaic_path_oracle as P  # noqa: E402
from guarded import INT_FILL, guarded, guarded_flat  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
INT_MAX = 2 ** 31 - 1


def _L():
    from rawaudiovae_kelsey_amd import _lib
    return _lib


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _mat(a, dtype=F32, guard=None):
    a = np.asarray(a)
    return guarded(a.shape[0], a.shape[1], a.shape[1], dtype, a, guard)


WS_FILL = 0xA5     # every byte of a workspace's guards: not a slot, not PATH_NONE = 255, not a float's low zero bytes


def _workspace(nbytes, align):
    """exactly nbytes between guards of WS_FILL bytes, on an `align`-byte boundary (None for 0 bytes).  Bytes, not
    floats: the PATH ops store single bytes, and a 0 written over the low byte of a float sentinel would not show."""
    if nbytes == 0:
        return None
    g = guarded_flat(nbytes, torch.uint8, WS_FILL)
    assert g.ptr % align == 0 and g.view.numel() == nbytes
    return g


def _eq(got, want, what):
    bad = np.argwhere(_bits(got) != _bits(want))
    assert got.shape == want.shape and len(bad) == 0, (what, bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- KNN, KNN_SMALL and the merge ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _knn_case(T, N, L, k):
    """(q, c, the oracle's idx, dist at k), computed once and left unchanged"""
    rng = np.random.default_rng(T * 31 + N * 7 + L)
    c = rng.standard_normal((N, L)).astype(np.float32)
    q = rng.standard_normal((T, L)).astype(np.float32)
    if T > 8:
        q[3:6] = c[[N // 2, 0, N - 1]]                            # exact hits, the last corpus row among them
        c[N // 3] = c[N - 1]                                      # and a tie
    idx, dist = O.knn(q, c, k)
    for a in (q, c, idx, dist):
        a.setflags(write=False)
    return q, c, idx, dist


def _knn_call(q, c, k, splits, small, off_by_4=False):
    """one search into guarded idx / dist through an exact workspace; c's back guard holds copies of q.  off_by_4: the
    corpus starts 4 bytes past a 16-byte boundary (its element 0 is a NaN pad in front of it)."""
    L = _L()
    T, Ld = q.shape
    N = c.shape[0]
    gq = _mat(q)
    if off_by_4:
        gc = guarded_flat(N * Ld + 1, F32, np.concatenate([[np.nan], c.reshape(-1)]), guard=q)
        c_ptr = gc.ptr + 4
        assert c_ptr % 16 == 4
    else:
        gc = _mat(c, guard=q)                                     # row N + i of c is q[i % T]
        c_ptr = gc.ptr
    gi, gd = guarded(T, k, k, I32, INT_FILL), guarded(T, k, k, F32)
    nbytes = L.mosaic_call(L.MOSAIC_KNN_SMALL_WORKSPACE if small else L.MOSAIC_KNN_WORKSPACE, T=T, N=N, L=Ld, k=k,
                           splits=splits).ws_bytes
    assert nbytes % 8 == 0 and (splits != 1 or nbytes == 0)
    gw = _workspace(nbytes, 4)
    L.mosaic_call(L.MOSAIC_KNN_SMALL if small else L.MOSAIC_KNN, T=T, N=N, L=Ld, k=k, splits=splits, q=gq.ptr, c=c_ptr,
                  idx=gi.ptr, dist=gd.ptr, ws=None if gw is None else gw.ptr, ws_bytes=nbytes)
    for g, name in ((gi, "idx"), (gd, "dist")) + (((gw, "workspace"),) if gw else ()):
        g.assert_untouched("%s (T %d N %d L %d k %d splits %d)" % (name, T, N, Ld, k, splits))
    return _np(gi.payload()), _np(gd.payload())


def _check_knn(T, N, L, k, splits, small, k_ref=None):
    q, c, ri, rd = _knn_case(T, N, L, k_ref or k)
    gi, gd = _knn_call(q, c, k, splits, small)
    what = (T, N, L, k, splits, small)
    assert gi.max() < N, (what, "a row of the guard won", np.argwhere(gi >= N)[:5].tolist())
    assert np.array_equal(gi, ri[:, :k]), (what, np.argwhere(gi != ri[:, :k])[:5].tolist())
    _eq(gd, rd[:, :k], what)
    gi2, gd2 = _knn_call(q, c, k, splits, small)
    assert np.array_equal(gi2, gi) and np.array_equal(_bits(gd2), _bits(gd)), what


@pytest.mark.parametrize("T,N,L,k,splits", [
    (1, 2, 1, 1, 0), (129, 65, 33, 2, 0), (129, 65, 33, 2, 2), (128, 64, 32, 4, 0), (128, 64, 32, 4, 1),
    (130, 4200, 8, 16, 66),   # one 64-row tile per split: the merge's lanes 0 and 1 take a second split each
    (5, 4200, 100, 3, 66)])
def test_knn_is_the_oracles_between_guards(T, N, L, k, splits):
    _check_knn(T, N, L, k, splits, False)


@pytest.mark.parametrize("N,L", [(300, 7), (257, 64), (513, 100)])
@pytest.mark.parametrize("T", [1, 2, 3, 5, 9, 17, 64])       # every TQ class (1, 2, 4, 8, 16), and passes 2 to 4
def test_knn_small_is_the_oracles_between_guards(T, N, L):
    for k in (1, 5):
        for splits in (0, 1, 2):
            _check_knn(T, N, L, k, splits, True, k_ref=5)         # the first column of the top 5 is the top 1


def test_knn_small_merges_more_than_64_splits_between_guards():
    _check_knn(16, 16796, 8, 4, 66, True)                         # one run of 256 rows per split


def test_knn_small_reads_a_corpus_off_the_16_byte_grid_element_by_element():
    q, c, ri, rd = _knn_case(9, 300, 8, 4)                        # L % 4 == 0: only the base keeps the vector loads away
    for splits in (0, 2):
        gi, gd = _knn_call(q, c, 4, splits, True, off_by_4=True)
        ai, ad = _knn_call(q, c, 4, splits, True)
        assert np.array_equal(gi, ai) and np.array_equal(_bits(gd), _bits(ad))
        assert np.array_equal(gi, ri) and np.array_equal(_bits(gd), _bits(rd))


# ---- GATHER_MEAN ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["row_start", "stride"])
@pytest.mark.parametrize("width", [1, 255, 256, 257, 600])
def test_gather_mean_is_the_oracles_between_guards(width, form):
    L = _L()
    rng = np.random.default_rng(width)
    T, n_rows, ldo = 9, 40, width + 8
    if form == "row_start":
        src_len, stride = 3000, 0
        starts = rng.integers(0, src_len - width + 1, n_rows + 8).astype(np.int64)   # n_rows of them count
        starts[3] = src_len - width                               # ends where src does: taken
        starts[4] = src_len - width + 1                           # one past: skipped
        starts[5] = -1                                            # before src: skipped
        table = guarded_flat(n_rows + 8, I64, starts, guard=[0])  # a start read past the table is a valid one
    else:
        stride = width + 3
        src_len = (n_rows - 1) * stride + width                   # the last row ends where src does: taken
        starts = np.arange(n_rows + 8, dtype=np.int64) * stride
        table = None
    src = rng.standard_normal(src_len).astype(np.float32)
    gs = guarded_flat(src_len, F32, src)
    for k in (1, 7, 16):
        idx = rng.integers(0, n_rows, (T, k)).astype(np.int32)
        idx[0, 0], idx[1, k - 1], idx[2, 0], idx[T - 1, 0] = -1, n_rows + 3, n_rows, n_rows - 1
        idx[3, :] = [3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4, 5, 3][:k]
        idx[4, :] = -1                                            # no neighbour at all: +0
        gi = guarded(T, k, k, I32, idx, guard=[0])
        out = guarded(T, width, ldo, F32)
        L.mosaic_call(L.MOSAIC_GATHER_MEAN, T=T, k=k, idx=gi.ptr, src=gs.ptr, src_len=src_len,
                      row_start=None if table is None else table.ptr, stride=stride, n_rows=n_rows, width=width,
                      out=out.ptr, ldo=ldo)
        out.assert_untouched("out (width %d k %d %s)" % (width, k, form))
        want = O.gather_mean(src, starts, idx, width, src_len=src_len, n_rows=n_rows)
        got = _np(out.payload())
        _eq(got, want, (width, form, k))
        assert np.array_equal(_bits(got[4]), np.zeros(width, np.int32))


# ---- OLA ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("F,S,hop,n_out,window", [(1, 64, 64, 64, None), (1, 64, 64, 100, None), (5, 64, 100, 470, None),
                                                  (7, 48, 20, 7 * 20 + 48 - 5, "hann"), (3, 1, 1, 3, None)])
def test_ola_is_the_oracles_between_guards(F, S, hop, n_out, window):
    from rawaudiovae_kelsey_amd.stream import window_values
    L = _L()
    frames = np.random.default_rng(F + S + hop).standard_normal((F, S)).astype(np.float32)
    w = None if window is None else window_values(S, window)
    gf, gw = _mat(frames), None if w is None else guarded_flat(S, F32, w)
    out = guarded_flat(n_out, F32)
    L.mosaic_call(L.MOSAIC_OLA, frames=gf.ptr, F=F, S=S, hop=hop, window=None if gw is None else gw.ptr, n_out=n_out,
                  out=out.ptr)
    out.assert_untouched("out")
    got, want = _np(out.payload()).reshape(n_out), O.ola(frames, hop, n_out, w)
    _eq(got, want, (F, S, hop, n_out, window))
    if hop > S:
        assert (got[S:hop] == 0).all()                            # between two frames
    if n_out > (F - 1) * hop + S:
        assert (got[(F - 1) * hop + S:] == 0).all()               # past the last one


# ---- TRANSITION -----------------------------------------------------------------------------------------------------------

TT, TN = 70, 200
CHUNKS = [(0, 70), (0, 1), (1, 33), (37, 33), (69, 1)]


@functools.lru_cache(maxsize=None)
def _trans_case(k, L):
    rng = np.random.default_rng(100 * k + L)
    mu = rng.standard_normal((TN, L)).astype(np.float32)
    next_of = np.minimum(np.arange(TN) + 1, TN - 1).astype(np.int32)
    idx = rng.integers(0, TN, (TT, k)).astype(np.int32)
    idx[rng.integers(0, TT, 12), rng.integers(0, k, 12)] = [-1, -1, -1, -1, TN, TN, TN, TN + 5, TN + 64, INT_MAX, -7,
                                                            -2 ** 31]
    idx[[0, 1, 36, 37, 69], 0] = [TN, -1, TN, TN - 1, TN]         # at the chunks' edges too
    for t in range(2, TT, 5):
        idx[t, k - 1] = next_of[idx[t - 1, 0]] if 0 <= idx[t - 1, 0] < TN else 0    # the corpus plays on: cost 0
    inside = np.where((idx < 0) | (idx >= TN), -1, idx)           # outside [0, N) is a missing candidate
    tr = P.transitions(mu, inside, next_of)
    for a in (mu, next_of, idx, tr):
        a.setflags(write=False)
    return mu, next_of, idx, tr


@pytest.mark.parametrize("L", [7, 64])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 9, 16])     # every KP class (1, 2, 4, 8, 16), k below and equal to KP
def test_transition_is_the_oracles_between_guards(k, L):
    lib = _L()
    mu, next_of, idx, tr = _trans_case(k, L)
    assert np.isinf(tr[1:]).any() and (tr[1:] == 0).any()
    gm = _mat(mu, guard=mu[:64])                                  # finite rows past N, where the oracle has +inf
    gn = guarded_flat(TN, I32, next_of, guard=[TN, TN + 1, INT_MAX])
    gi = guarded(TT, k, k, I32, idx, guard=[0])
    for row0, rows in CHUNKS:
        out = guarded_flat(rows * k * k, F32)
        lib.mosaic_call(lib.MOSAIC_TRANSITION, T=TT, k=k, idx=gi.ptr, c=gm.ptr, N=TN, L=L, next_of=gn.ptr, row0=row0,
                        rows=rows, trans=out.ptr)
        out.assert_untouched("trans (k %d L %d rows [%d, +%d))" % (k, L, row0, rows))
        _eq(_np(out.payload()).reshape(rows, k, k), tr[row0:row0 + rows], (k, L, row0, rows))


# ---- PATH_FORWARD + PATH_BACKTRACK ----------------------------------------------------------------------------------------

LAM = 0.3      # fl(lambda * trans) is inexact: a product fused into the add would show


@functools.lru_cache(maxsize=None)
def _path_case(T, k):
    rng = np.random.default_rng(T * 17 + k)
    N, L = 200, 8
    mu = rng.standard_normal((N, L)).astype(np.float32)
    q = mu[rng.integers(0, N, T)] + 0.3 * rng.standard_normal((T, L)).astype(np.float32)
    idx, dist = O.knn(q, mu, k)
    idx, dist = idx.astype(np.int32), dist.copy()
    next_of = np.minimum(np.arange(N) + 1, N - 1).astype(np.int32)
    if T >= 16:
        idx[T // 2], dist[T // 2] = -1, np.inf                    # a closed row: the path restarts behind it
        idx[5, k - 1], dist[5, k - 1] = -1, np.inf
        idx[T - 2, k // 2:], dist[T - 2, k // 2:] = -1, np.inf
        if k > 1:
            dist[9, 0] = np.nan                                   # a NaN distance is a missing candidate
    tr = P.transitions(mu, idx, next_of)
    want = P.best_path(idx, dist, mu, next_of, LAM, tr=tr)
    for a in (idx, dist, tr) + tuple(want):
        a.setflags(write=False)
    return idx, dist, tr, want


def _path_call(idx, dist, tr, step):
    """forward in chunks of `step` rows, each over its own guarded chunk of trans, then the backtrack"""
    lib = _L()
    T, k = idx.shape
    gi, gd = guarded(T, k, k, I32, idx, guard=[0]), _mat(dist)
    nbytes = lib.mosaic_call(lib.MOSAIC_PATH_WORKSPACE, T=T, k=k).ws_bytes
    assert nbytes % 16 == 0
    gw = _workspace(nbytes, 16)
    for r0 in range(0, T, step):
        rows = min(step, T - r0)
        gt = guarded_flat(rows * k * k, F32, tr[r0:r0 + rows].reshape(-1))
        lib.mosaic_call(lib.MOSAIC_PATH_FORWARD, T=T, k=k, idx=gi.ptr, dist=gd.ptr, row0=r0, rows=rows, trans=gt.ptr,
                        lam=LAM, ws=gw.ptr, ws_bytes=nbytes)
        gw.assert_untouched("workspace after rows [%d, +%d) of T %d k %d" % (r0, rows, T, k))
    gs, gc, gcost = guarded_flat(T, I32, INT_FILL), guarded_flat(T, I32, INT_FILL), guarded_flat(2, F64)
    lib.mosaic_call(lib.MOSAIC_PATH_BACKTRACK, T=T, k=k, idx=gi.ptr, dist=gd.ptr, ws=gw.ptr, ws_bytes=nbytes,
                    slot=gs.ptr, choice=gc.ptr, cost=gcost.ptr)
    for g, name in ((gs, "slot"), (gc, "choice"), (gcost, "cost"), (gw, "workspace")):
        g.assert_untouched("%s (T %d k %d)" % (name, T, k))
    return _np(gs.payload()).reshape(T), _np(gc.payload()).reshape(T), _np(gcost.payload()).reshape(2)


@pytest.mark.parametrize("k", [1, 5, 16])
@pytest.mark.parametrize("T", [1, 2, 16, 17, 255, 256, 257, 600])   # the 16-row prefetch, the 256-row backtrack chunk
def test_path_is_the_oracles_between_guards(T, k):
    idx, dist, tr, (rs, rc, rcost) = _path_case(T, k)
    slot, choice, cost = _path_call(idx, dist, tr, T)
    assert np.array_equal(slot, rs), (np.argwhere(slot != rs)[:5].tolist(), slot[:8], rs[:8])
    assert np.array_equal(choice, rc)
    assert cost.dtype == np.float64 and np.array_equal(_bits(cost), _bits(rcost)), (cost, rcost)
    closed = np.isinf(P.targets(idx, dist)).all(1)
    assert np.array_equal(slot < 0, closed) and (T < 16 or closed[T // 2]) and not closed[0]
    s2, c2, cost2 = _path_call(idx, dist, tr, 100)                # rows [0, 100), [100, 200), ...: the scores carried
    assert np.array_equal(s2, slot) and np.array_equal(c2, choice) and np.array_equal(_bits(cost2), _bits(cost))


# ---- LIVE without a fit ---------------------------------------------------------------------------------------------------

S_LIVE, HOP = 64, 16


@pytest.fixture(scope="module")
def index():
    from rawaudiovae_kelsey_amd import mosaic
    from rawvae.model import VAE
    torch.manual_seed(5)
    index = mosaic.LatentIndex(VAE(S_LIVE, 96, 8).cuda().eval(), hop=HOP)
    rng = np.random.default_rng(9)
    for i, n in enumerate((700, 1000, 513, 1290)):
        t = np.arange(n) / 8000.0
        w = 0.6 * np.sin(2 * np.pi * (150 + 170 * i) * t) + 0.2 * rng.standard_normal(n)
        w[: n // 5] = 0                                           # leading silence: duplicate all-zero frames
        index.add(w.astype(np.float32), "f%d" % i)
    return index


def _live_run(sm, x):
    """every block of x, then the drains of a lag -> the outputs and the matches, call after call"""
    out = dict(y=[], idx=[], dist=[], choice=[])
    for b in range(x.shape[1] // sm.block):
        out["y"].append(sm.process(x[:, b * sm.block:(b + 1) * sm.block]).clone())
        i, d, c = sm.last_matches()
        out["idx"].append(i.clone()), out["dist"].append(d.clone()), out["choice"].append(c.clone())
    for _ in range(sm.drain_blocks if sm.lag else 0):
        out["y"].append(sm.drain().clone())
        out["choice"].append(sm.last_matches()[2].clone())
    return {k: _bits(_np(torch.cat(v, 1))) for k, v in out.items()}


@pytest.mark.parametrize("mode", ["grains", "decode"])
@pytest.mark.parametrize("continuity,lag", [(0.0, 0), (0.5, 0), (0.5, 2)])
def test_live_without_a_fit_stays_inside_its_exact_workspace(index, continuity, lag, mode):
    from rawaudiovae_kelsey_amd import mosaic as M
    rng = np.random.default_rng(25)
    t = np.arange(32 * 5)
    x = np.stack([0.5 * np.sin(t * (0.05 + 0.03 * s)) for s in range(2)]) + 0.1 * rng.standard_normal((2, t.size))
    x = torch.from_numpy(x.astype(np.float32)).cuda()
    kw = dict(hop=HOP, k=4, mode=mode, window="hann", continuity=continuity, lag=lag)
    ref = _live_run(M.StreamingMosaic(index, 2, 32, **kw), x)     # the unguarded twin
    sm = M.StreamingMosaic(index, 2, 32, **kw)
    n = sm._ws.numel()
    assert n % 256 == 0 and n == sm._call(_L().MOSAIC_LIVE_WORKSPACE, None, None).ws_bytes
    gws = _workspace(n, 256)
    sm._ws = gws.view.reshape(-1)
    assert sm._ws.numel() == n and sm._ws.data_ptr() == gws.ptr
    sm.reset()
    got = _live_run(sm, x)
    gws.assert_untouched("workspace after the blocks%s" % (" and the drains" if lag else ""))
    sm.reset(1)
    sm.reset()
    gws.assert_untouched("workspace after the resets")
    assert sorted(got) == sorted(ref)
    for key in ref:
        assert np.array_equal(got[key], ref[key]), (key, np.argwhere(got[key] != ref[key])[:5].tolist())
    assert np.array_equal(_live_run(sm, x)["y"], ref["y"])        # and again after the resets
    gws.assert_untouched("workspace after the second run")
