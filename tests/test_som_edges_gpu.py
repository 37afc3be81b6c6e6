"""The loop edges of csrc/som.hip, exactly and between guards: raw rv_som_bmu, rv_som_node_sums, rv_som_update and
rv_segment_mean calls on pointers cut from tests/guarded.py buffers.

Every output lies between sentinel guards (assert_untouched after each call), every float input between NaN guards, and
the node matrix of rv_som_bmu has an ATTRACTIVE back guard: copies of the first rows of x, so a node read at an index
>= M is at distance 0 of some row and wins -- the exact comparison with som_oracle.bmu_exact then fails.  Integer
inputs have no NaN; their guards hold values the kernel would act on visibly (node numbers in bmu's, huge counts).

Shapes are the smallest at which a loop takes another trip: the 128 x 64 x 32 tile of k_som_bmu (one off and exactly
on it), the 256-row scan and the 1024-element L pass of k_som_node_sums, the 256-node h pass (with a tail of 16, and
exactly two) and the L pass of k_som_update, the 256-element pass of k_segment_mean.  Each call runs twice into fresh
outputs: equal bits."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import som_oracle as O  # noqa: E402
from guarded import INT_FILL, guarded, guarded_flat  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64


def _lib():
    from rawaudiovae_kelsey_amd import _lib
    return _lib


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _mat(a, dtype=F32, guard=None):
    return guarded(a.shape[0], a.shape[1], a.shape[1], dtype, a, guard)


def _same_bits(got, want, what):
    """bit equality; a NaN must be a NaN in both (its payload bits are the adder's business)"""
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), (what, "NaN at", np.argwhere(gn != wn)[:5].tolist())
    bad = np.argwhere((_bits(got) != _bits(want)) & ~wn)
    assert len(bad) == 0, (what, bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- rv_som_bmu -----------------------------------------------------------------------------------------------------

def _bmu_call(x, w):
    L = _lib()
    N, M = x.shape[0], w.shape[0]
    gx = _mat(x)
    gw = _mat(w, guard=x[:64])                                    # attractive: row M + i of w is x[i % 64]
    outs = [guarded_flat(N, I32, INT_FILL), guarded_flat(N, I32, INT_FILL), guarded_flat(N, F32), guarded_flat(N, F32)]
    L.lib().rv_som_bmu(gx.ptr, N, gw.ptr, M, x.shape[1], *[g.ptr for g in outs], L.stream_ptr())
    for g, name in zip(outs, ("best", "second", "d_best", "d_second")):
        g.assert_untouched(name)
    return [_np(g.payload()).reshape(N) for g in outs]


@pytest.mark.parametrize("N,M,L,kind", [(1, 2, 1, ""), (129, 65, 33, ""), (128, 64, 32, ""), (257, 130, 70, ""),
                                        (300, 1000, 7, ""), (257, 130, 70, "nan"), (1, 2, 1, "one-node"),
                                        (129, 2, 33, "one-node")])
def test_bmu_is_the_oracles_bit_for_bit_between_guards(N, M, L, kind):
    rng = np.random.default_rng(N * 7 + M * 3 + L)
    x = rng.standard_normal((N, L)).astype(np.float32)
    w = rng.standard_normal((M, L)).astype(np.float32)
    if N > 8:
        x[5:8] = w[[M // 2, 0, M - 1]]                            # exact hits, the last node among them
        w[M // 3] = w[M - 1]                                      # and a tie between two nodes
    if kind == "nan":
        w[[0, 64, M - 1], [0, L - 1, 3]] = np.nan                 # three NaN nodes
        x[128] = np.nan                                           # one NaN row
    if kind == "one-node":
        w[1, L - 1] = np.nan
    got = _bmu_call(x, w)
    want = O.bmu_exact(x, w)
    for g, r, name in zip(got, want, ("best", "second", "d_best", "d_second")):
        assert np.array_equal(_bits(g), _bits(r)), (name, np.argwhere(_bits(g) != _bits(r))[:5].tolist(), g[:8], r[:8])
    assert got[0].max() < M and got[1].max() < M                  # no row of the guard won
    if kind == "nan":
        assert got[0][128] == -1 and got[1][128] == -1 and np.isinf(got[2][128]) and np.isinf(got[3][128])
        assert not np.isin(got[0], [0, 64, M - 1]).any() and not np.isin(got[1], [0, 64, M - 1]).any()
        assert (np.delete(got[0], 128) >= 0).all() and (np.delete(got[1], 128) >= 0).all()
    elif kind == "one-node":
        assert (got[0] == 0).all() and (got[1] == -1).all() and np.isinf(got[3]).all() and np.isfinite(got[2]).all()
    else:
        assert got[0].min() >= 0 and got[1].min() >= 0 and (got[0] != got[1]).all()
    for g, a in zip(_bmu_call(x, w), got):
        assert np.array_equal(_bits(g), _bits(a))


# ---- rv_som_node_sums -------------------------------------------------------------------------------------------------

def _node_sums_call(x, bmu, M):
    L = _lib()
    N, Ld = x.shape
    gx = _mat(x)
    gb = guarded_flat(N, I32, bmu, guard=np.arange(M))            # a row scanned past N would join a node
    gs, gc = guarded(M, Ld, Ld, F64), guarded_flat(M, I64, INT_FILL)
    L.lib().rv_som_node_sums(gx.ptr, N, Ld, gb.ptr, M, gs.ptr, gc.ptr, L.stream_ptr())
    gs.assert_untouched("sums"), gc.assert_untouched("counts")
    return _np(gs.payload()), _np(gc.payload()).reshape(M)


@pytest.mark.parametrize("N,L,M", [(1, 1, 1), (255, 3, 5), (256, 1025, 3), (257, 2049, 4), (1000, 70, 300)])
def test_node_sums_are_the_oracles_bit_for_bit_between_guards(N, L, M):
    rng = np.random.default_rng(N + L + M)
    x = (rng.standard_normal((N, L)) * 10.0 ** rng.integers(-3, 4, (N, 1))).astype(np.float32)
    bmu = rng.integers(0, M, N).astype(np.int32)
    if M >= 3:
        bmu[bmu == M - 1] = 0                                     # the last node stays empty
        bmu[rng.choice(np.arange(1, N // 2), 9, replace=False)] = [-1, -1, -1, M, M, M + 7, 2 ** 31 - 1, -2 ** 31, -5]
        bmu[[0, N - 1]] = [M - 2, 0]                                # the first and the last row belong to a node
        x[N // 2] = np.nan                                        # one NaN row, on node 1
        bmu[N // 2] = 1
    sums, counts = _node_sums_call(x, bmu, M)
    rs, rc = O.node_sums(x, bmu, M)
    assert counts.dtype == np.int64 and np.array_equal(counts, rc), (counts[:8], rc[:8])
    _same_bits(sums, rs, "sums")
    if M >= 3:
        assert counts[M - 1] == 0 and np.array_equal(_bits(sums[M - 1]), np.zeros(L, np.int64))    # +0
        assert np.isnan(sums[1]).all() and not np.isnan(np.delete(sums, 1, axis=0)).any()
        assert counts.sum() == N - 9
    else:
        assert counts.sum() == N
    s2, c2 = _node_sums_call(x, bmu, M)
    assert np.array_equal(_bits(s2), _bits(sums)) and np.array_equal(c2, counts)


# ---- rv_som_update ----------------------------------------------------------------------------------------------------

SIGMAS = (3.0, 0.7, 1e-3, 1e-200)


def _ulp32(ref):
    """the fp32 spacing at |ref| (float64 array): 2^(e - 23) for 2^e <= |ref| < 2^(e+1), the denormal spacing below"""
    _, e = np.frexp(np.abs(ref))
    return np.ldexp(1.0, np.maximum(e - 1, -126) - 23)


def _update_call(sums, counts, w_old, rows, cols, sigma):
    L = _lib()
    M, Ld = w_old.shape
    gs, gw = _mat(sums, F64), _mat(w_old)
    gc = guarded_flat(M, I64, counts, guard=[1 << 40])            # an int has no NaN: a count read past M swamps den
    gn = guarded(M, Ld, Ld, F32)
    L.lib().rv_som_update(gs.ptr, gc.ptr, gw.ptr, rows, cols, Ld, float(sigma), gn.ptr, L.stream_ptr())
    gn.assert_untouched("w_new")
    return _np(gn.payload())


@pytest.mark.parametrize("rows,cols,L", [(1, 2, 1), (6, 7, 70), (16, 17, 5), (2, 256, 3), (3, 4, 1030)])
def test_update_is_the_float64_oracle_rounded_between_guards(rows, cols, L):
    from rawaudiovae_kelsey_amd import som as S
    M = rows * cols
    empty = 1 if M == 2 else 2                                    # the last nodes have no member
    rng = np.random.default_rng(rows * 100 + cols + L)
    N = 4 * M
    x = rng.standard_normal((N, L)).astype(np.float32)
    bmu = rng.permutation(np.arange(N) % (M - empty)).astype(np.int32)     # every other node has members
    sums, counts = S.node_sums(torch.from_numpy(x).cuda(), torch.from_numpy(bmu).cuda(), M)
    sums, counts = _np(sums), _np(counts)                         # the device's own
    assert (counts[M - empty:] == 0).all() and counts.sum() == N
    w_old = rng.standard_normal((M, L)).astype(np.float32)
    for sigma in SIGMAS:
        got = _update_call(sums, counts, w_old, rows, cols, sigma)
        ref = O.update(sums, counts, w_old, rows, cols, sigma)
        err = np.abs(got.astype(np.float64) - ref)
        half = 0.5 * _ulp32(ref)
        excess = np.where(ref != 0, (err - half) / np.where(ref != 0, np.abs(ref), 1.0), 0.0).max()
        print("som_update grid %dx%d L %d sigma %g: largest (|got - ref| - 0.5 ulp) / |ref| = %.3e"
              % (rows, cols, L, sigma, excess))
        bad = np.argwhere(err > half + 1e-12 * np.abs(ref))
        assert len(bad) == 0, (sigma, bad[:5].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
        den = O.neighbourhood(rows, cols, sigma) @ counts.astype(np.float64)
        assert np.array_equal(_bits(got[den == 0]), _bits(w_old[den == 0]))
        if sigma <= 1e-3:      # the neighbourhood is the node itself: its own mean, and w_old where it has no member
            assert (den == 0).sum() == empty and (den[M - empty:] == 0).all()
            own = (sums[:M - empty] / counts[:M - empty, None]).astype(np.float32)
            assert np.array_equal(_bits(got[:M - empty]), _bits(own))
        again = _update_call(sums, counts, w_old, rows, cols, sigma)
        assert np.array_equal(_bits(again), _bits(got))


# ---- rv_segment_mean ------------------------------------------------------------------------------------------------------

LENS = [1, 5, 1, 300, 2]


def _segment_mean_call(x, off_dev, off_host):
    L = _lib()
    R, Ld = x.shape
    F = len(off_host) - 1
    gx = _mat(x)
    go = guarded_flat(F + 1, I64, np.asarray(off_dev, np.int64), guard=[1 << 40])
    out = guarded(F, Ld, Ld, F32)
    host = np.ascontiguousarray(off_host, dtype=np.int64)
    L.lib().rv_segment_mean(gx.ptr, R, Ld, go.ptr, host.ctypes.data_as(L.C.POINTER(L.c_i64)), F, out.ptr,
                            L.stream_ptr())
    torch.cuda.synchronize()                                      # `host` is read by the call, `go` by the kernel
    out.assert_untouched("out")
    return _np(out.payload())


@pytest.mark.parametrize("L", [1, 256, 257, 600])
def test_segment_mean_is_the_oracles_bit_for_bit_between_guards(L):
    rng = np.random.default_rng(L)
    R = sum(LENS)
    x = (rng.standard_normal((R, L)) * 10 + 3).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(LENS)])
    want = O.segment_mean(x, off)
    got = _segment_mean_call(x, off, off)
    assert np.array_equal(_bits(got), _bits(want)), np.argwhere(_bits(got) != _bits(want))[:5].tolist()
    assert np.array_equal(got[0], x[0]) and np.array_equal(got[2], x[6])
    assert np.array_equal(_bits(_segment_mean_call(x, off, off)), _bits(got))
    if L == 257:
        # a device copy of the offsets that disagrees with the host's: the kernel clamps it to the R rows, so the last
        # segment is what is left of it inside x and nothing of x's guard is read
        wild = off.copy()
        wild[-1] = R + 50
        assert np.array_equal(_bits(_segment_mean_call(x, wild, off)), _bits(want))
