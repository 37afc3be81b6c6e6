"""The fp64 statistics and chains of the latent PCA and the latent walk on the GPU, bit for bit against
tests/moment_oracle.py, at the edges of their loops and past 256 columns: RV_PCA_MOMENTS, RV_PCA_LAGCOV, RV_PCA_APPLY,
RV_WALK_FIT and RV_WALK_STEP; RV_PCA_EIG past 128 pairs within the bounds of tests/test_pca_gpu.py.

Every call goes to rv_mosaic directly, so the test owns every buffer (tests/guarded.py): x, centre, the components and
row_start lie between NaN guards (row_start, an integer, between values no file starts at); ws is exactly as large as
the *_WORKSPACE op says and lies between sentinel guards, as every output does; all guards are checked afterwards.
A wide moment (T L L > 3e7) is compared on moment_oracle.LISTED_ROWS over all columns, everything else in full.
tests/test_moment_oracle_cpu.py shows that the inputs used here tell a wrong order of the adds from the right one.
"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import guarded as G  # noqa: E402
import moment_oracle as M  # noqa: E402
import pca_oracle as PO  # noqa: E402
from test_states_gpu import _np, _same  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
NO_ROW = -(1 << 40)                             # what lies around row_start
APPLY_K = (1, 8, 9, 255, 256, 257)              # and L
APPLY_T = (1, 3, 4, 5, 7, 8, 9)                 # 8 rows a workgroup up to L = 256, 4 beyond: full, partial and one over
EIG_CASES = ((1000, 257), (1000, 258), (2000, 512))    # (rows of the corpus, L): h = 129 pairs, odd L with the padding index
FIT_CASES = ((1, 1), (16, 17), (64, 70), (255, 256), (257, 320), (512, 512))      # (k, L)
STEP_CASES = ((17, 16), (320, 255), (320, 257), (512, 512))                        # (L, k)


def _lib():
    from rawaudiovae_kelsey_amd import _lib
    return _lib


def _call(op, **fields):
    return _lib().mosaic_call(op, **fields)


def _in(a, dtype=F64):
    """an input between NaN guards (an integer one: between NO_ROW) -> the Guarded"""
    a = np.asarray(a)
    return G.guarded_flat(a.size, dtype, a.reshape(-1), None if dtype.is_floating_point else np.array([NO_ROW]))


def _out(n, dtype=F64, fill=G.SENTINEL):
    return G.guarded_flat(int(n), dtype, fill)


def _values(g, shape):
    return _np(g.payload()).reshape(shape)


def _untouched(**buffers):
    torch.cuda.synchronize()
    for name, g in buffers.items():
        g.assert_untouched(name)


# ---- RV_PCA_MOMENTS ---------------------------------------------------------------------------------------------------

def _moments(x, ws_fill):
    """(centre [L], C [L, L]) of one RV_PCA_MOMENTS call whose ws held ws_fill"""
    L_ = _lib()
    T, L = x.shape
    xg = G.guarded(T, L, L, F32, x)
    n = _call(L_.PCA_WORKSPACE, T=T, L=L).ws_bytes
    assert n > 0 and n % 8 == 0
    ws, centre, cov = _out(n // 8, F64, ws_fill), _out(L), _out(L * L)
    _call(L_.PCA_MOMENTS, T=T, L=L, q=xg.ptr, ws=ws.ptr, ws_bytes=n, centre=centre.ptr, basis=cov.ptr)
    _untouched(ws=ws, centre=centre, covariance=cov)
    return _values(centre, (L,)), _values(cov, (L, L))


@pytest.mark.parametrize("T,L", M.MOMENT_CASES)
def test_moments_are_the_blocked_mean_and_the_ranges_chains(T, L):
    x = M.moment_input(T, L)
    rows = M.compared_rows(T, L)
    centre, cov = _moments(x, 0.0)
    what = "T %d L %d" % (T, L)
    _same(centre, PO.blocked_mean(x), "centre " + what)
    _same(cov[rows], M.covariance_bits(x, rows), "covariance " + what)
    _same(cov, cov.T.copy(), "C == C^T " + what)
    for fill, why in ((0.0, "a second run"), (NAN, "ws full of NaN: a partial tile read before it is written")):
        c2, cov2 = _moments(x, fill)
        _same(c2, centre, "centre, %s, %s" % (why, what))
        _same(cov2, cov, "covariance, %s, %s" % (why, what))


# ---- RV_PCA_LAGCOV ----------------------------------------------------------------------------------------------------

def _lagcov(x, rs, centre, ws_fill):
    L_ = _lib()
    T, L = x.shape
    xg, cg, rg = G.guarded(T, L, L, F32, x), _in(centre), _in(rs, I64)
    n = _call(L_.WALK_WORKSPACE, T=T, k=0, L=L).ws_bytes
    assert n > 0 and n % 8 == 0
    ws, c1 = _out(n // 8, F64, ws_fill), _out(L * L)              # the keep bytes are the head of ws
    _call(L_.PCA_LAGCOV, T=T, L=L, n_rows=len(rs) - 1, q=xg.ptr, row_start=rg.ptr, ws=ws.ptr, ws_bytes=n,
          centre=cg.ptr, basis=c1.ptr)
    _untouched(ws=ws, C1=c1)
    return _values(c1, (L, L))


@pytest.mark.parametrize("lengths,L", M.LAG_CASES)
def test_lagcov_is_the_ranges_chains_over_the_kept_pairs(lengths, L):
    x, rs, centre = M.lag_input(lengths, L)
    T = x.shape[0]
    rows = M.compared_rows(T, L)
    c1 = _lagcov(x, rs, centre, 0.0)
    what = "%s L %d" % (lengths, L)
    _same(c1[rows], M.lagcov_bits(x, rs, centre, rows), "C1 " + what)
    for fill, why in ((0.0, "a second run"), (NAN, "ws full of NaN")):
        _same(_lagcov(x, rs, centre, fill), c1, "C1, %s, %s" % (why, what))


# ---- RV_PCA_APPLY -----------------------------------------------------------------------------------------------------

def _apply(mode, q, width, k, L, comp, centre, lam=None, g=None, h=None):
    """out [T, width] of one RV_PCA_APPLY call on the rows q, with a row pitch of width + 3 between sentinels"""
    T = q.shape[0]
    qg = G.guarded(T, q.shape[1], q.shape[1], F32, q)
    out = G.guarded(T, width, width + 3, F32)
    extra = {} if lam is None else dict(eigenvalues=lam.ptr, gains=g.ptr, shifts=h.ptr)
    _call(_lib().PCA_APPLY, mode=mode, T=T, L=L, k=k, q=qg.ptr, out=out.ptr, ldo=width + 3, centre=centre.ptr,
          basis=comp.ptr, **extra)
    _untouched(out=out)
    return _np(out.payload())


@pytest.mark.parametrize("L", (3, 70, 256, 257, 320, 512))
def test_apply_is_the_headers_chains_rounded_once(L):
    x, centre, lam, g, h = M.apply_input(L)
    cg = _in(centre)
    for k in [k for k in APPLY_K if k < L] + [L]:
        comp = M.rotation(L)[:k]
        coords = M.project_chain(x, comp, centre)
        y = M.apply_bits(M.PROJECT, x, comp, centre, coords=coords)
        one, zero = np.ones(k, np.float32), np.zeros(k, np.float32)
        bent = lam[:k].copy()
        bent[0] = -1e-17                                  # a slightly negative eigenvalue: its shift counts as zero
        edits = (("g = 1, h = 0", lam[:k], one, zero), ("a mixed edit", lam[:k], g[:k], h[:k]),
                 ("a negative eigenvalue", bent, g[:k], h[:k]))
        want = [M.apply_bits(M.EDIT, x, comp, centre, lm, gg, hh, coords) for _, lm, gg, hh in edits]
        assert np.array_equal(want[0].view(np.int32), x.view(np.int32))
        assert not np.array_equal(want[1], want[2]) and not np.array_equal(want[1], x)
        rec = M.apply_bits(M.RECONSTRUCT, y, comp, centre)
        vg = _in(comp)
        dev = [(_in(lm), _in(gg, F32), _in(hh, F32)) for _, lm, gg, hh in edits]
        for T in APPLY_T:
            what = "L %d k %d T %d" % (L, k, T)
            _same(_apply(M.PROJECT, x[:T], k, k, L, vg, cg), y[:T], "project " + what)
            _same(_apply(M.RECONSTRUCT, y[:T], L, k, L, vg, cg), rec[:T], "reconstruct " + what)
            for (name, _, _, _), w, (lg, gg, hg) in zip(edits, want, dev):
                _same(_apply(M.EDIT, x[:T], L, k, L, vg, cg, lg, gg, hg), w[:T], "edit, %s, %s" % (name, what))


# ---- RV_PCA_EIG -------------------------------------------------------------------------------------------------------

def _eig(cov):
    """(eigenvalues, components, sweeps, converged) of one RV_PCA_EIG call on a copy of cov between guards"""
    L_ = _lib()
    L = cov.shape[0]
    n = _call(L_.PCA_WORKSPACE, T=0, L=L).ws_bytes
    assert n == 8 * L * L
    basis, ws, lam, info = _out(L * L), _out(L * L), _out(L), _out(2, I32, G.INT_FILL)
    basis.view.copy_(torch.from_numpy(np.array(cov).reshape(1, -1)))
    _call(L_.PCA_EIG, L=L, ws=ws.ptr, ws_bytes=n, basis=basis.ptr, eigenvalues=lam.ptr, info=info.ptr)
    _untouched(basis=basis, ws=ws, eigenvalues=lam, info=info)
    sweeps, converged = (int(v) for v in _values(info, (2,)))
    return _values(lam, (L,)), _values(basis, (L, L)), sweeps, converged


@pytest.mark.parametrize("N,L", EIG_CASES)
def test_eig_past_128_pairs_within_the_bounds_and_the_same_twice(N, L):
    cov = PO.covariance(N, L)
    lam, V, sweeps, converged = _eig(cov)
    ref = np.linalg.eigvalsh(cov)[::-1]
    F, U = np.linalg.norm(cov), PO.U
    r = (np.abs(lam - ref).max() / (L * U * F), np.linalg.norm(cov @ V.T - V.T * lam) / (L * U * F),
         np.linalg.norm(V @ V.T - np.eye(L)) / (L * U))
    print("eig", (N, L), "sweeps", sweeps, "ratios to L u ||C||, L u ||C||, L u: %.3g %.3g %.3g (bounds 8, 16, 128)" % r)
    assert converged == 1 and 1 <= sweeps <= PO.MAX_SWEEPS
    assert np.all(np.diff(lam) <= 0)
    assert r[0] <= 8 and r[1] <= 16 and r[2] <= 128
    assert np.all(V[np.arange(L), np.argmax(np.abs(V), axis=1)] > 0)           # the sign rule
    lam2, V2, sweeps2, converged2 = _eig(cov)
    _same(lam2, lam, "eigenvalues of a second run"), _same(V2, V, "components of a second run")
    assert (sweeps2, converged2) == (sweeps, converged)


# ---- RV_WALK_FIT ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,L", FIT_CASES)
def test_walk_fit_is_the_headers_chains(k, L):
    L_ = _lib()
    V, lam, C1 = M.fit_input(k, L)
    n = _call(L_.WALK_WORKSPACE, T=0, k=k, L=L).ws_bytes
    assert n == 8 * k * L
    vg, lg, mg = _in(V), _in(lam), _in(C1)
    ws, res = _out(k * L), _out(2 * k * k + 2 * k * L)
    _call(L_.WALK_FIT, mode=L_.WALK_DYNAMICS, k=k, L=L, ws=ws.ptr, ws_bytes=n, basis=vg.ptr, eigenvalues=lg.ptr,
          moment=mg.ptr, result=res.ptr)
    _untouched(ws=ws, result=res)
    want = M.walk_fit_bits(V, lam, C1, k)
    got = _values(res, (-1,))
    at = 0
    for name in ("A", "Q", "P", "R"):
        _same(got[at:at + want[name].size], want[name].ravel(), "%s k %d L %d" % (name, k, L))
        at += want[name].size
    A, U, q = M.noise_input(k)
    ag, ug, qg = _in(A), _in(U), _in(q)
    for mode, extra, ref in ((L_.WALK_NOISE, dict(moment=ug.ptr, eigenvalues=qg.ptr), M.walk_noise_bits(A, U, q)),
                             (L_.WALK_DIAGONAL, {}, M.walk_diagonal_bits(A))):
        dyn = _out(2 * k * k)
        _call(L_.WALK_FIT, mode=mode, k=k, L=L, basis=ag.ptr, result=dyn.ptr, **extra)
        _untouched(dyn=dyn)
        _same(_values(dyn, (2, k, k)), ref, "mode %d k %d" % (mode, k))


# ---- RV_WALK_STEP -----------------------------------------------------------------------------------------------------

def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


@functools.lru_cache(maxsize=None)
def _walk(L, k):
    """(the smallest model a stream takes at L: one sample a frame, one hidden unit; a LatentWalk holding
    moment_oracle.step_input's dynamics and R, set directly)"""
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd import walk as W
    dyn, R, c = M.step_input(L, k)[:3]
    torch.manual_seed(L + k)
    model = VAE(1, 1, L).cuda().eval()
    walk = W.LatentWalk(k)._set(mean=_dev(c), components=_dev(R), variances=torch.ones(k, dtype=F64, device="cuda"),
                                dyn=_dev(dyn), P=_dev(R), R=_dev(R), rank=k, n_frames=2, n_files=1)
    return model, walk


def _generator(L, k):
    from rawaudiovae_kelsey_amd import walk as W
    model, walk = _walk(L, k)
    offset, temperature = M.step_input(L, k)[3:5]
    gen = W.StreamingWalk(model, walk, 3, 4)           # hop = S = 1: four frames a block
    gen.temperature.copy_(_dev(temperature))
    gen.offset.copy_(_dev(offset))
    return gen


@pytest.mark.parametrize("L,k", STEP_CASES)
def test_walk_step_is_the_headers_chains_unprimed_then_primed(L, k):
    L_ = _lib()
    dyn, R, c, offset, temperature, eps = M.step_input(L, k)
    assert eps.shape == (3, 8, k)
    want_w, want_z = M.walk_step_bits(dyn, R, c, offset, temperature, eps, np.full((3, k), NAN), np.zeros(3, bool))
    gen = _generator(L, k)
    dg, rg, cg = _in(dyn), _in(R), _in(c)
    state, primed = _out(3 * k), _out(3, I32, G.INT_FILL)
    state.view.fill_(NAN)                                # a stream that is not primed does not use its state
    primed.view.zero_()
    y = torch.empty((3, 4), dtype=F32, device="cuda")
    for call in range(2):
        e = np.ascontiguousarray(eps[:, 4 * call:4 * call + 4])
        eg = _in(e, F32)
        out = G.guarded(12, L, L + 3, F32)
        sd = gen.stream.desc(gen._silence, y, eg.view)
        _call(L_.WALK_STEP, live=C.pointer(sd), k=k, L=L, ldo=L + 3, centre=cg.ptr, basis=rg.ptr, moment=dg.ptr, out=out.ptr,
              state=state.ptr, primed=primed.ptr)
        _untouched(out=out, state=state, primed=primed)
        what = "L %d k %d call %d" % (L, k, call)
        _same(_np(out.payload()).reshape(3, 4, L), want_z[:, 4 * call:4 * call + 4], "out " + what)
        _same(_values(state, (3, k)), want_w[:, 4 * call + 3], "state " + what)
        assert _values(primed, (3,)).tolist() == [1, 1, 1]
    # the generator's own buffers: last_latents and state
    own = _generator(L, k)
    for call in range(2):
        own.generate(_dev(eps[:, 4 * call:4 * call + 4]))
        _same(own.last_latents(), want_z[:, 4 * call:4 * call + 4], "last_latents L %d k %d call %d" % (L, k, call))
        _same(own.state, want_w[:, 4 * call + 3], "the generator's state L %d k %d call %d" % (L, k, call))
