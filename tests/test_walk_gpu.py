"""The latent walk on the GPU (RV_PCA_LAGCOV, RV_WALK_FIT, RV_WALK_STEP, walk.py, generate.py) against
tests/walk_oracle.py.  u = 2^-53.

Bounds.
  lag moment  |C1 - oracle|_ij <= (T + 8) u sqrt(C_ii C_jj): the fp64 dot-product bound with Cauchy-Schwarz, the form of
              the moments test.  Two runs bit-equal; every row its own file: exactly zero.
  fit         every element of A within (2 L + 4) u sum |terms| of numpy's P C1 P^T from the GPU's own centre, axes and
              variances (two chains of L terms, and a square root and a division in each of the two P factors);
              ||A||_2 <= 1 + 1e-9; Q == Q^T bit for bit.
              ||A A^T + B B^T - I||_F <= 2.4e-13 = 8 x 2.98e-14, the largest value the numpy oracle (numpy.linalg.eigh
              for Q) reaches over the corpora and k of tests/test_walk_cpu.py (at k = 256), with the 8 x headroom
              test_pca_gpu.py takes over its numpy restatement of the Jacobi solver.  The kernels' value is evaluated in
              long double, so the evaluation adds nothing.
              Diagonal mode: B exactly diagonal, |a^2 + b^2 - 1| <= 4 u.
  step        ||w - w_oracle||_2 <= n (2 k + 2) u max_f || |A| |w_f| + |B| |e_f| ||_2 after n frames (||A||_2 <= 1: the
              errors of earlier frames do not grow); z within one fp32 ulp + (k + 3) u sum |terms| + sum_j |R_jl| x the
              state bound.  The oracle steps in long double.
Each test prints the figures it asserts on."""
import copy
import ctypes as C
import functools
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import stream_oracle as SO  # noqa: E402
import walk_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

U = O.U
CLOSURE_BOUND = 8 * 2.98e-14
FIT_CASES = [(lengths, L, k) for lengths, L in O.CORPORA for k in (1, 2, 16, 64) if k <= min(L, sum(lengths) - 1)]
STEP_MODELS = {17: (32, 40, 17, 16, (100, 1, 156)), 256: (64, 96, 256, 64, (2500, 3000, 3500))}   # L: S, H, L, k, corpus
N_FRAMES = 40


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))     # a copy: the oracle's arrays are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _bits(t):
    a = np.ascontiguousarray(_np(t))
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


@functools.lru_cache(maxsize=None)
def _corpus(lengths, L):
    """(x on the device, row_start, the fitted LatentPCA with every axis) of one oracle corpus, shared by the tests."""
    from rawaudiovae_kelsey_amd import pca as P
    xd = _dev(O.make_corpus(lengths, L))
    return xd, O.row_start(lengths), P.LatentPCA().fit(xd)


# ---- lag moment ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lengths,L", O.CORPORA)
def test_lagcov_equals_the_oracle_within_the_dot_product_bound(lengths, L):
    from rawaudiovae_kelsey_amd import walk as W
    x = O.make_corpus(lengths, L)
    xd, rs, pca = _corpus(lengths, L)
    T = x.shape[0]
    centre = pca.mean_
    c1, again = W.lagcov(xd, rs, centre), W.lagcov(xd, rs, centre)
    assert c1.shape == (L, L) and c1.dtype == torch.float64
    assert np.array_equal(_bits(c1), _bits(again))                              # two runs bit-equal
    c = _np(centre)
    sd = np.sqrt(np.diag(O.moments(x)[1]))
    bound = (T + 8) * U * np.outer(sd, sd)
    for what, starts in (("files", rs), ("one file", np.array([0, T]))):
        got = _np(W.lagcov(xd, starts, centre))
        err = np.abs(got - O.lagcov(x, starts, c))
        print("lagcov", lengths, L, what, "worst |C1 - oracle| / bound %.3g" % (err / bound).max())
        assert np.all(err <= bound)
    d = x.astype(np.float64) - c
    assert np.all(np.abs(got - d[1:].T @ d[:-1] / (T - 1)) <= bound)            # a single file: the unmasked product
    if len(lengths) > 1 and L > 1:
        assert not np.array_equal(_np(c1), got) and not np.array_equal(_np(c1), _np(c1).T)
    assert not _np(W.lagcov(xd, np.arange(T + 1), centre)).any()                # every row its own file: exactly zero


def test_lagcov_of_a_strided_slice_equals_that_of_its_copy():
    from rawaudiovae_kelsey_amd import walk as W
    lengths, L = (100, 1, 156), 17
    xd, rs, pca = _corpus(lengths, L)
    big = torch.full((257, 40), 9.0, device="cuda")
    big[:, 11:28] = xd
    view = big[:, 11:28]
    assert not view.is_contiguous()
    assert np.array_equal(_bits(W.lagcov(view, rs, pca.mean_)), _bits(W.lagcov(xd, rs, pca.mean_)))
    assert bool((big[:, :11] == 9.0).all()) and bool((big[:, 28:] == 9.0).all()) and torch.equal(big[:, 11:28], xd)


# ---- fit ----------------------------------------------------------------------------------------------------------

def _closure(A, B):
    A, B = A.astype(np.longdouble), B.astype(np.longdouble)
    return float(np.sqrt(((A @ A.T + B @ B.T - np.eye(A.shape[0])) ** 2).sum()))


@pytest.mark.parametrize("lengths,L,k", FIT_CASES)
def test_fit_against_the_oracle_and_its_invariants(lengths, L, k):
    from rawaudiovae_kelsey_amd import walk as W
    x = O.make_corpus(lengths, L)
    xd, rs, pca = _corpus(lengths, L)
    walk = W.LatentWalk(k).fit(xd, rs, pca)
    assert walk.rank_ >= k and (walk.n_frames_, walk.n_files_) == (x.shape[0], len(lengths))
    A, B, Q = _np(walk.A_), _np(walk.B_), _np(walk.Q_)
    c, V, lam = _np(pca.mean_), _np(pca.components_), _np(pca.explained_variance_)
    ref = O.dynamics(O.lagcov(x, rs, c), V, lam, k)
    tol = (2 * L + 4) * U * ref["terms"]
    err = np.abs(A - ref["A"])
    norm, closure = np.linalg.norm(A, 2), _closure(A, B)
    print("fit", lengths, L, "k", k, "worst |A - oracle| / bound %.3g, ||A||_2 %.6f, closure %.3g (bound %.3g)"
          % ((err / tol).max(), norm, closure, CLOSURE_BOUND))
    assert np.all(err <= tol)
    assert norm <= 1 + 1e-9
    assert np.array_equal(Q, Q.T)
    assert closure <= CLOSURE_BOUND
    assert np.array_equal(walk.persistence_, np.diag(A)) and walk.predictability_ == pytest.approx((A * A).sum() / k, rel=1e-14)
    s = np.sqrt(lam[:k])
    assert np.allclose(_np(walk.P_), V[:k] / s[:, None], rtol=4 * U, atol=0)
    assert np.allclose(_np(walk.R_), V[:k] * s[:, None], rtol=4 * U, atol=0)
    # diagonal mode: the diagonal of the same A, B exactly diagonal, a^2 + b^2 = 1 to 4 u
    dia = W.LatentWalk(k, "diagonal").fit(xd, rs, pca)
    Ad, Bd = _np(dia.A_), _np(dia.B_)
    assert np.array_equal(Ad, np.diag(np.diag(A))) and np.array_equal(Bd, np.diag(np.diag(Bd))) and dia.Q_ is None
    a, b = np.diag(Ad).astype(np.longdouble), np.diag(Bd).astype(np.longdouble)
    worst = float(np.abs(a * a + b * b - 1).max())
    print("fit", lengths, L, "k", k, "diagonal: worst |a^2 + b^2 - 1| / u %.3g" % (worst / U))
    assert worst <= 4 * U and np.all(np.abs(a) <= 1)


def test_fit_refuses_more_axes_than_the_rank_and_fits_its_own_pca():
    from rawaudiovae_kelsey_amd import walk as W
    xd, rs, pca = _corpus((1, 2, 5), 3)
    with pytest.raises(ValueError, match="n_components=4 must be in \\[1, r\\], r = 3"):
        W.LatentWalk(4).fit(xd, rs, pca)
    own, given = W.LatentWalk(2).fit(xd, rs), W.LatentWalk(2).fit(xd, rs, pca)
    assert torch.equal(own.dyn_, given.dyn_) and torch.equal(own.R_, given.R_)
    flat = torch.cat([xd[:, :2], xd[:, :1]], 1).contiguous()                    # an exactly duplicated column: rank 2
    with pytest.raises(ValueError, match="r = 2 the rank"):
        W.LatentWalk(3).fit(flat, rs)
    assert W.LatentWalk().fit(flat, rs).n_components == 2


# ---- step ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _setup(L):
    """(model, fitted walk) of STEP_MODELS[L], shared and left unchanged."""
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd import walk as W
    S, H, _, k, lengths = STEP_MODELS[L]
    torch.manual_seed(100 + L)
    model = VAE(S, H, L).cuda().eval()
    xd, rs, pca = _corpus(lengths, L)
    return model, W.LatentWalk(k).fit(xd, rs, pca)


def _eps(n_streams, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n_streams, n, k), generator=g).cuda()


def _run(gen, n_blocks, eps=None):
    F = gen.frames_per_block
    out = []
    for b in range(n_blocks):
        out.append(gen.generate(None if eps is None else eps[:, b * F:(b + 1) * F]).clone())
    return torch.cat(out, 1)


def _small(x, layer, act):
    from rawaudiovae_kelsey_amd._lib import lib, ptr, stream_ptr
    w, b = layer.weight.detach(), layer.bias.detach()
    M, K = x.shape
    y = torch.empty((M, w.shape[0]), dtype=torch.float32, device=x.device)
    lib().rv_small_linear_f32(ptr(x), K, ptr(w), K, ptr(b), M, w.shape[0], K, act, ptr(y), w.shape[0], stream_ptr())
    return y


def _decode(model, z):
    return _small(_small(z.contiguous(), model.fc3, 1), model.fc4, 2)


@pytest.mark.parametrize("L", sorted(STEP_MODELS))
def test_state_and_latents_within_the_bounds(L):
    from rawaudiovae_kelsey_amd import walk as W
    model, walk = _setup(L)
    S, k = STEP_MODELS[L][0], STEP_MODELS[L][3]
    E = _eps(2, N_FRAMES, k, 5)
    gen = W.StreamingWalk(model, walk, 2, S)
    gen.temperature.copy_(torch.tensor([1.0, 0.7]))
    off = torch.linspace(-0.5, 0.5, L).cuda()
    gen.offset[1] = off
    states, lat = [], []
    for f in range(N_FRAMES):
        gen.generate(E[:, f:f + 1])
        states.append(_np(gen.state).copy())
        lat.append(_np(gen.last_latents())[:, 0].copy())
    states, lat = np.array(states), np.array(lat)                               # [n, streams, ...]
    A, B, R, c = _np(walk.A_), _np(walk.B_), _np(walk.R_), _np(walk.mean_)
    for s, temp, offset in ((0, 1.0, None), (1, 0.7, _np(off))):
        w, z, drive, zterms = O.run(A, B, R, c, _np(E[s]), temp, offset)
        n = np.arange(1, N_FRAMES + 1)
        sbound = n * (2 * k + 2) * U * np.maximum.accumulate(drive)
        serr = np.linalg.norm(states[:, s] - w, axis=1)
        zbound = (np.spacing(np.abs(z).astype(np.float32)).astype(np.float64) + (k + 3) * U * zterms
                  + np.abs(R).sum(0)[None, :] * sbound[:, None])
        zerr = np.abs(lat[:, s].astype(np.float64) - z)
        print("step L=%d stream %d: worst state error / bound %.3g, worst latent error / bound %.3g"
              % (L, s, (serr / sbound).max(), (zerr / zbound).max()))
        assert np.all(serr <= sbound) and np.all(zerr <= zbound)
    assert np.linalg.norm(states[-1, 0]) > 0.1 * np.sqrt(k)                     # a walk, not a decay


def _randn(n, seed, offset):
    from rawaudiovae_kelsey_amd._lib import lib, ptr, stream_ptr
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    lib().rv_randn(ptr(out), n, seed, offset, stream_ptr())
    return out


def test_philox_noise_block_size_streams_and_seed():
    from rawaudiovae_kelsey_amd import walk as W
    model, walk = _setup(17)
    S, k = 32, 16
    hop = S // 4
    make = lambda n_streams, block, seed=77: W.StreamingWalk(model, walk, n_streams, block, hop, "hann", seed)  # noqa: E731
    a = make(2, hop)
    ya = _run(a, N_FRAMES)
    # the Philox path is the explicit path fed rv_randn(seed, offset = stream)
    E = torch.stack([_randn(N_FRAMES * k, 77, s).view(N_FRAMES, k) for s in range(2)])
    b = make(2, hop)
    assert torch.equal(_run(b, N_FRAMES, E), ya) and torch.equal(b.state, a.state)
    # block = hop and block = 4 hop: the same audio and state
    c = make(2, 4 * hop)
    assert torch.equal(_run(c, N_FRAMES // 4), ya) and torch.equal(c.state, a.state)
    # stream 0 alone is stream 0 of two; the two streams differ; the seed decides
    one = make(1, 4 * hop)
    assert torch.equal(_run(one, N_FRAMES // 4)[0], ya[0]) and torch.equal(one.state[0], a.state[0])
    assert not torch.equal(ya[0], ya[1])
    assert torch.equal(_run(make(2, 4 * hop), N_FRAMES // 4), ya)
    assert not torch.equal(_run(make(2, 4 * hop, seed=78), N_FRAMES // 4), ya)
    assert bool(torch.isfinite(ya).all()) and float(ya.abs().max()) > 0


def test_reset_and_set_state():
    from rawaudiovae_kelsey_amd import walk as W
    model, walk = _setup(17)
    S, k = 32, 16
    hop = S // 4
    make = lambda: W.StreamingWalk(model, walk, 2, 2 * hop, hop, "hann", 3)   # noqa: E731
    whole = _run(make(), 3)
    g = make()
    first = _run(g, 2)
    g.reset(1)
    assert int(g._primed[1]) == 0 and int(g._primed[0]) == 1 and not g.state[1].any()
    third = g.generate()
    assert torch.equal(first, whole[:, :4 * hop])
    assert torch.equal(third[0], whole[0, 4 * hop:])                            # stream 0 goes on
    assert torch.equal(third[1], whole[1, :2 * hop])                            # stream 1 starts again
    # a set state: the next frame at temperature 0 is A w
    xd = _corpus((100, 1, 156), 17)[0]
    w0 = walk.whiten(xd[40:42].contiguous())
    assert w0.shape == (2, k) and w0.dtype == torch.float32
    g = W.StreamingWalk(model, walk, 2, S)
    g.temperature.zero_()
    g.set_state(w0)
    assert int(g._primed.sum()) == 2 and torch.equal(g.state, w0.double())
    g.generate()
    A = _np(walk.A_).astype(np.longdouble)
    w = _np(w0).astype(np.longdouble)
    ref = (w @ A.T).astype(np.float64)
    bound = (2 * k + 2) * U * np.linalg.norm((np.abs(w) @ np.abs(A).T).astype(np.float64), axis=1)
    err = np.linalg.norm(_np(g.state) - ref, axis=1)
    print("set_state: |state - A w| / bound", err / bound)
    assert np.all(err <= bound) and np.all(np.linalg.norm(ref, axis=1) > 0)
    g.set_state(w0[1], 0)
    assert torch.equal(g.state[0], w0[1].double())
    with pytest.raises(ValueError, match="w has shape"):
        g.set_state(w0[:, :3])
    with pytest.raises(ValueError, match="stream 2 of 2"):
        g.reset(2)


@pytest.mark.parametrize("L", sorted(STEP_MODELS))
def test_audio_is_the_decode_of_the_latents(L):
    from rawaudiovae_kelsey_amd import walk as W
    from rawaudiovae_kelsey_amd.stream import window_values
    model, walk = _setup(L)
    S = STEP_MODELS[L][0]
    # hop == S, no window: the decoded frames themselves, byte for byte
    g = W.StreamingWalk(model, walk, 2, 2 * S, seed=9)
    for _ in range(3):
        y = g.generate()
        z = g.last_latents()
        assert z.shape == (2, 2, L)
        assert torch.equal(y, _decode(model, z.reshape(-1, L)).view(2, 2 * S))
    # hop = S / 4 and Hann: the weighted overlap-add of the decoded frames
    hop = S // 4
    g = W.StreamingWalk(model, walk, 2, 4 * hop, hop, "hann", 9)
    ys, zs = [], []
    for _ in range(N_FRAMES // 4):
        ys.append(g.generate().clone())
        zs.append(g.last_latents().clone())
    y, z = _np(torch.cat(ys, 1)).astype(np.float64), torch.cat(zs, 1)
    w = window_values(S, "hann").astype(np.float64)
    for s in range(2):
        dec = _np(_decode(model, z[s])).astype(np.float64)
        err = np.abs(y[s] - SO.wola(dec, w, hop, y.shape[1])).max()
        print("audio L=%d stream %d: worst |y - wola(decoded)| %.3g (bound 1e-6)" % (L, s, err))
        assert err <= 1e-6 and np.abs(y[s]).max() > 0


def test_graph_replay_equals_eager_and_sees_the_controls():
    from rawaudiovae_kelsey_amd import walk as W
    from rawaudiovae_kelsey_amd._lib import RvError
    model, walk = _setup(17)
    mine = copy.deepcopy(model)
    S, hop = 32, 8
    eager = W.StreamingWalk(model, walk, 2, 2 * hop, hop, "hann", 21)
    graph = W.StreamingWalk(mine, walk, 2, 2 * hop, hop, "hann", 21)
    with pytest.raises(RvError, match="before capture"):
        graph.replay()
    graph.capture()
    for step in range(4):
        if step == 2:                                                           # controls written in place
            for g in (eager, graph):
                g.temperature[1] = 0.25
                g.offset[0] = torch.linspace(-1, 1, 17).cuda()
        assert torch.equal(graph.replay(), eager.generate()), step
        assert torch.equal(graph.state, eager.state) and torch.equal(graph.last_latents(), eager.last_latents())
    mine.fc3.weight = torch.nn.Parameter(mine.fc3.weight.detach().clone())
    with pytest.raises(RvError, match="replaced after capture"):
        graph.replay()
    torch.cuda.synchronize()


def test_argument_errors_name_the_field_and_touch_nothing():
    from rawaudiovae_kelsey_amd import _lib
    from rawaudiovae_kelsey_amd import walk as W
    from rawaudiovae_kelsey_amd._lib import MosaicDesc, RvError, lib, ptr, stream_ptr
    model, walk = _setup(17)
    g = W.StreamingWalk(model, walk, 2, 16, 8, "hann", 1)
    g.generate()
    torch.cuda.synchronize()
    before = (g.stream._ws.clone(), g.state.clone(), g._primed.clone(), g._z.clone())
    y = torch.zeros((2, 16), device="cuda")

    def step(**change):
        sd = g.stream.desc(g._silence, y, None)
        for name in [n for n in change if n.startswith("live_")]:
            setattr(sd, name[5:], change.pop(name))
        f = dict(live=C.pointer(sd), k=16, L=17, ldo=17, centre=ptr(walk.mean_), basis=ptr(walk.R_), moment=ptr(walk.dyn_),
                 out=ptr(g._z), state=ptr(g._state), primed=ptr(g._primed))
        f.update(change)
        lib().rv_mosaic(_lib.WALK_STEP, C.byref(MosaicDesc(**f)), stream_ptr())

    for change, msg in ((dict(k=0), "k=0 outside"), (dict(k=18), "k=18 outside"), (dict(L=16), "L=16, the stream's model has L=17"),
                        (dict(L=513), "L=513 outside"), (dict(centre=None), "centre is null"),
                        (dict(basis=None), "basis \\(R\\) is null"), (dict(moment=None), "moment .* is null"),
                        (dict(state=None), "the state is null"), (dict(primed=None), "the primed flags are null"),
                        (dict(ldo=16), "ldo=16 holds no row"), (dict(live=None), "\\(live\\) is null"),
                        (dict(live_temperature=None), "live->temperature is null"), (dict(live_y=None), "null buffer")):
        with pytest.raises(RvError, match=msg):
            step(**change)
    with pytest.raises(ValueError, match="eps has shape"):
        g.generate(torch.zeros((2, 2, 17), device="cuda"))
    torch.cuda.synchronize()
    for a, b in zip(before, (g.stream._ws, g.state, g._primed, g._z)):
        assert torch.equal(a, b)
    assert not y.any()
    # the fit's ops
    xd, rs, pca = _corpus((100, 1, 156), 17)
    rsd = torch.from_numpy(rs).cuda()
    c1 = torch.full((17, 17), 7.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(W._workspace(257, 16, 17, "cuda")[1], dtype=torch.uint8, device="cuda")
    good = dict(T=257, L=17, n_rows=3, q=ptr(xd), row_start=ptr(rsd), ws=ptr(ws), ws_bytes=ws.numel(),
                centre=ptr(pca.mean_), basis=ptr(c1))
    for change, msg in ((dict(T=1), "T=1 outside"), (dict(L=513), "L=513 outside"), (dict(n_rows=0), "n_rows=0"),
                        (dict(q=None), "q is null"), (dict(row_start=None), "row_start is null"),
                        (dict(centre=None), "centre is null"), (dict(basis=None), "basis .* is null"),
                        (dict(ws_bytes=8), "ws_bytes=8"), (dict(ws=None), "ws is null")):
        with pytest.raises(RvError, match="PCA_LAGCOV.*" + msg):
            lib().rv_mosaic(_lib.PCA_LAGCOV, C.byref(MosaicDesc(**dict(good, **change))), stream_ptr())
    for change, msg in ((dict(mode=3), "mode=3"), (dict(k=0), "k=0 outside"), (dict(result=None), "result is null"),
                        (dict(moment=None), "moment .* is null"), (dict(ws_bytes=0), "ws_bytes=0")):
        f = dict(mode=_lib.WALK_DYNAMICS, k=16, L=17, ws=ptr(ws), ws_bytes=ws.numel(), basis=ptr(pca.components_),
                 eigenvalues=ptr(pca.explained_variance_), moment=ptr(c1), result=ptr(c1))
        with pytest.raises(RvError, match="WALK_FIT.*" + msg):
            lib().rv_mosaic(_lib.WALK_FIT, C.byref(MosaicDesc(**dict(f, **change))), stream_ptr())
    with pytest.raises(RvError, match="WALK_WORKSPACE.*T=1 "):
        lib().rv_mosaic(_lib.WALK_WORKSPACE, C.byref(MosaicDesc(T=1, L=17)), None)
    torch.cuda.synchronize()
    assert bool((c1 == 7.0).all()) and not ws.any()
    with pytest.raises(ValueError, match="ascending"):
        W.lagcov(xd, [0, 100, 100, 257], pca.mean_)


# ---- the tool -----------------------------------------------------------------------------------------------------

S, H, LAT, SR = 64, 32, 8, 8000


def _model():
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.synth import make_params
    m = VAE(S, H, LAT).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(S, H, LAT, 0).items()})
    return m


def _waves():
    rng = np.random.default_rng(11)
    t = np.arange(2100) / SR
    return [(0.5 * np.sin(2 * np.pi * 330 * t) + 0.2 * rng.standard_normal(t.size)).astype(np.float32),
            (0.7 * rng.uniform(-1, 1, 1333)).astype(np.float32)]


def test_generate_py_fit_then_run(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import json
    import generate as cli
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import walk as W
    (tmp_path / "audio").mkdir()
    for i, w in enumerate(_waves()):
        D.write_wav(tmp_path / "audio" / ("%d.wav" % i), w, SR)
    ini = tmp_path / "m.ini"
    ini.write_text("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n"
                   % (SR, S, H, LAT))
    ck = tmp_path / "ckpt"
    torch.save({"epoch": 0, "state_dict": _model().state_dict(), "optimizer": {}}, ck)
    npz = tmp_path / "walk.npz"
    common = ["--config", str(ini), "--checkpoint", str(ck), "--hop", "16"]
    rep = cli.main(["fit"] + common + ["--data", str(tmp_path / "audio"), "--keep", "4", "--out", str(npz)])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == rep
    model = _model()
    waves = [D.load_audio_mono(tmp_path / "audio" / ("%d.wav" % i), SR) for i in range(2)]
    want = W.fit_corpus(model, waves, 16, 4)
    assert (rep["keep"], rep["n_files"], rep["n_frames"], rep["rank"]) == (4, 2, want.n_frames_, want.rank_)
    assert rep["predictability"] == want.predictability_ and rep["persistence"] == [float(v) for v in want.persistence_]
    assert 0 < rep["predictability"] <= 1 and want.row_start_.tolist() == [0, want.row_start_[1], want.n_frames_]
    walk, meta = W.read_walk(npz)
    assert meta == dict(segment_length=S, latent_dim=LAT, hop=16, n_frames=want.n_frames_, n_files=2)
    assert torch.equal(walk.dyn_, want.dyn_) and torch.equal(walk.R_, want.R_) and torch.equal(walk.mean_, want.mean_)
    run = ["run"] + common + ["--walk", str(npz), "--seconds", "0.25", "--window", "hann", "--seed", "5"]
    y = cli.main(run + ["--out", str(tmp_path / "a.wav")])
    n = 2000
    assert y.shape == (1, n) and np.isfinite(y).all() and np.abs(y).max() > 0
    assert D.load_audio_mono(tmp_path / "a.wav", SR).shape == (n,)
    gen = W.StreamingWalk(model, walk, 1, 16, 16, "hann", 5)                    # by hand, one frame per block
    ref = _np(torch.cat([gen.generate() for _ in range(n // 16)], 1))
    assert np.array_equal(y, ref)
    again = cli.main(run + ["--out", str(tmp_path / "b.wav")])
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "b.wav").read_bytes() and np.array_equal(again, y)
    # --start: another first block, the same determinism
    start = run + ["--start", str(tmp_path / "audio" / "0.wav")]
    s1, s2 = cli.main(start + ["--out", str(tmp_path / "c.wav")]), cli.main(start + ["--out", str(tmp_path / "d.wav")])
    assert np.array_equal(s1, s2) and not np.array_equal(s1[:, :256], y[:, :256])
    # --streams 2 and a shift along axis 1: two files, the first stream moved by exactly LatentPCA.offset's vector
    two = cli.main(run + ["--streams", "2", "--pca-shift", "1:2", "--out", str(tmp_path / "e.wav")])
    assert two.shape == (2, n) and (tmp_path / "e_0.wav").exists() and (tmp_path / "e_1.wav").exists()
    assert not np.array_equal(two[0], two[1]) and not np.array_equal(two[0], y[0])
    with pytest.raises(ValueError, match="--hop: hop 32: the walk was fitted at hop 16"):
        cli.main(["run", "--config", str(ini), "--checkpoint", str(ck), "--hop", "32", "--walk", str(npz), "--seconds", "1",
                  "--out", str(tmp_path / "x.wav")])
    with pytest.raises(ValueError, match="--pca-shift: axis 5: the PCA file holds 4 axes"):
        cli.main(run + ["--pca-shift", "5:1", "--out", str(tmp_path / "x.wav")])
    with pytest.raises(ValueError, match="--keep 9: .*r = "):
        cli.main(["fit"] + common + ["--data", str(tmp_path / "audio"), "--keep", "9", "--out", str(npz)])
