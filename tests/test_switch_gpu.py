"""The switching walk on the GPU (RV_SWITCH_*, csrc/switch.hip, rawaudiovae_kelsey_amd/switching.py, compose.py) against
tests/switch_oracle.py.  u = 2^-53.

Bit for bit, inputs between NaN guards, outputs and ws between sentinel guards, x with a row pitch of L + 3: the residual and
the observed flags; the moments N, D', D and C1 at the range edges, with file ends and unobserved frames on either side of a
pair; the dynamics and Q on moments set directly; the guard and [A^T | B^T] given the device's own eigenvectors; the step's
state, state numbers, path and latents on supplied draws, and the audio as the decode of the latents.

Bounded: the closure ||A A^T + B B^T - I||_F of every state within 8 x the worst the oracle (numpy.linalg.eigh for Q) reaches
over the same shapes, the headroom test_walk_gpu.py takes; g = 1 / 1.5 within 4 u where C1 = 1.5 D; the fitted phi within 1e-9
of the oracle's fit of the planted data.

Statistics of one seed over 4096 frames: forced to state j, the mean and variance of y within 5 standard errors of m_j and
v_j, the standard errors those of a stationary Gaussian VAR(1) with autocovariance A_j^h (Bartlett's sums over the lags);
free-running, the transition counts within 5 binomial standard errors of A_hmm.  Each test prints the figures it asserts on."""
import copy
import ctypes as C
import functools
import json
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import guarded as G  # noqa: E402
import states_oracle as SO  # noqa: E402
import stream_oracle as STO  # noqa: E402
import switch_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

U = O.U
FIT_SHAPES = ((1, 1), (3, 16), (64, 64))
STEP_SHAPES = ((7, 1, 1), (17, 16, 3), (70, 64, 64))     # (L, k, S)
SEG, HID = 32, 24                                          # the decoder of the step tests


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))     # a copy: the oracle's arrays are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if torch.is_tensor(a) else a)
    return a.view({8: np.int64, 4: np.int32, 1: np.uint8}[a.dtype.itemsize])


def _same(got, want, what):
    got, want = _bits(got), _bits(want if torch.is_tensor(want) else np.asarray(want))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d elements differ, the first at %d" % (what, bad.size, got.size, bad[0])


def _in64(a):
    """a float64 input between NaN guards, as a device tensor of a's shape"""
    a = np.asarray(a, np.float64)
    g = G.guarded_flat(a.size, torch.float64, a.reshape(-1))
    return g.view.view(a.shape)


def _out(shape, dtype=torch.float64, fill=G.SENTINEL):
    n = int(np.prod(shape))
    g = G.guarded_flat(n, dtype, fill)
    return g, g.view.view(shape)


def _rows(x, pad=3):
    """x [T, L] fp32 with a row pitch of L + pad, NaN in the gaps and guards"""
    return G.guarded(x.shape[0], x.shape[1], x.shape[1] + pad, torch.float32, x).view


class _Block:
    """n bytes on a 256-byte boundary between two guards of `fill` bytes"""

    def __init__(self, n, fill):
        self.n, self.fill, self.front = n, fill, 512
        self.flat = torch.full((self.front + n + 512 + n,), fill, dtype=torch.uint8, device="cuda")
        assert self.flat.data_ptr() % 256 == 0
        self.view = self.flat[self.front:self.front + n]

    def assert_untouched(self, name):
        bad = int((self.flat[:self.front] != self.fill).sum()) + int((self.flat[self.front + self.n:] != self.fill).sum())
        assert bad == 0, "%s: %d guard bytes were written" % (name, bad)


def _law(T, S, seed):
    rng = np.random.default_rng(seed)
    g = rng.uniform(0, 1, (T, S)) * np.geomspace(1, 1e-4, S)
    return g / g.sum(axis=1, keepdims=True)


# ---- RV_SWITCH_RESIDUAL -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,L", ((1, 1), (3, 7), (64, 70)))
def test_residual_equals_the_oracle_bit_for_bit(k, L):
    from rawaudiovae_kelsey_amd import switching as SW
    c, P = SO.basis(k, L)
    cd, Pd = _in64(c), _in64(P)
    for T in (1, 63, 64, 65, 257):
        x = SO.latents(T, L)
        if T > 1:
            x[T // 2, L - 1] = np.nan                                           # one unobserved frame
        xd = _rows(x)
        for S in (1, 2, 17, 64):
            th, gamma = SO.random_theta(S, k), _law(T, S, T + S)
            n = SW.residual_bytes(T, k)
            blk = _Block(n, 0x5A)
            SW.residual(xd, cd, Pd, _in64(th), _in64(gamma), S, out=blk.view)
            torch.cuda.synchronize()
            blk.assert_untouched("the residual block")
            r, obs = SW.split_residual(blk.view, T, k)
            want_r, want_obs = O.residual(x, c, P, th, gamma, S, k)
            what = "k %d L %d T %d S %d" % (k, L, T, S)
            _same(r, want_r, "r " + what)
            assert np.array_equal(_np(obs), want_obs), what
            pad = _np(blk.view[8 * T * k:n - T])                                # between r and the flags: not written
            assert (pad == 0x5A).all(), what
            if T > 1:
                assert want_obs.sum() == T - 1 and not want_r[T // 2].any() and want_r[0].any()


# ---- RV_SWITCH_MOMENTS ------------------------------------------------------------------------------------------------------

def _moments_case(T, S, k, holes, seed=0):
    rng = np.random.default_rng(1000 * S + k + T + seed)
    r = rng.standard_normal((T, k))
    obs = np.ones(T, np.uint8)
    obs[[h for h in holes if h < T]] = 0
    r[obs == 0] = 0.0                                                           # as RV_SWITCH_RESIDUAL leaves it
    return r, obs, _law(T, S, T + 3 * S)


def _gpu_moments(r, obs, gamma, rs, S, k, ws_fill=0xFF):
    from rawaudiovae_kelsey_amd import switching as SW
    T = r.shape[0]
    blk = _Block(SW.residual_bytes(T, k), 0xFF)                                 # 0xFF..: NaN to a double that is read past r
    rv, ov = SW.split_residual(blk.view, T, k)
    rv.copy_(_dev(r))
    ov.copy_(_dev(obs))
    nb = SW.workspace(T, S, k, "cuda")[1]
    ws = _Block(nb, ws_fill)
    g, mo = _out((SW.moments_size(S, k),))
    SW.moments(blk.view, _in64(gamma), rs, S, k, out=mo, ws=(ws.view, nb))
    torch.cuda.synchronize()
    g.assert_untouched("the moments"), ws.assert_untouched("ws")
    return mo


def _check_moments(T, S, k, lengths, holes):
    r, obs, gamma = _moments_case(T, S, k, holes)
    rs = SO.starts(lengths)
    assert rs[-1] == T
    got = _gpu_moments(r, obs, gamma, rs, S, k)
    keep = O.keep_mask(rs, obs, T)
    want = O.moments(r, gamma, keep)
    what = "T %d S %d k %d files %s" % (T, S, k, lengths)
    _same(got, O.pack_moments(want), what)
    _same(_gpu_moments(r, obs, gamma, rs, S, k, 0x00), got, what + ": a ws of zeros and a ws of NaN")
    return keep, want


@pytest.mark.parametrize("T,lengths,holes", (
    (2, (2,), ()), (2, (1, 1), ()), (4, (1, 1, 2), ()), (4096, (4096,), (7,)), (4097, (4097,), (4096,)),
    (4098, (4098,), (4095, 4097)), (4398, (4096, 2, 300), (4200,)), (4098, (4095, 3), (4096,)), (4102, (4097, 5), (0, 4101))))
def test_moments_at_the_range_edges_with_file_ends_and_unobserved_frames(T, lengths, holes):
    keep, want = _check_moments(T, 3, 3, lengths, holes)
    cuts = np.cumsum(lengths)[:-1] - 1
    assert not keep[cuts].any() and not keep[[p for h in holes for p in (h - 1, h) if 0 <= p < T - 1]].any()
    assert keep.sum() == T - 1 - len(set(cuts) | {p for h in holes for p in (h - 1, h) if 0 <= p < T - 1})
    if lengths == (1, 1):
        assert not O.pack_moments(want).any()


@pytest.mark.parametrize("S,k", ((64, 64), (17, 33)))
def test_moments_at_the_tile_edges(S, k):
    _check_moments(300, S, k, (100, 0, 200), (150, 299))


# ---- RV_SWITCH_FIT ----------------------------------------------------------------------------------------------------------

def _direct_moments(S, k, seed=0):
    """moments set directly: N with thin states, D' and D with zeros, negatives, inf and NaN among them"""
    rng = np.random.default_rng(100 * S + k + seed)
    mo = dict(N=rng.uniform(0, 40, S), Dn=rng.uniform(0.5, 2, (S, k)), Dt=rng.uniform(0.5, 2, (S, k)),
              C1=rng.standard_normal((S, k, k)))
    mo["N"][S // 2] = 1.5
    if S > 2:
        mo["N"][0], mo["N"][S - 1] = 2.0, np.nan
    mo["Dn"][0, 0] = 0.0
    if k > 3:
        mo["Dt"][0, 1], mo["Dn"][S - 1, 2], mo["Dt"][S // 3, 3], mo["Dn"][S // 3, k - 1] = -1.0, np.inf, np.nan, 0.0
    return mo


def _gpu_dynamics(mo, S, k):
    from rawaudiovae_kelsey_amd import switching as SW
    g, res = _out((2 * S * k * k,))
    gi, info = _out((S,), torch.int32, G.INT_FILL)
    A, Q, info = SW.dynamics(_in64(O.pack_moments(mo)), S, k, out=(res, info))
    torch.cuda.synchronize()
    g.assert_untouched("[A | Q]"), gi.assert_untouched("info")
    return A, Q, info


@pytest.mark.parametrize("S,k", FIT_SHAPES)
def test_dynamics_and_q_are_bit_for_bit_on_moments_set_directly(S, k):
    mo = _direct_moments(S, k)
    A, Q, info = _gpu_dynamics(mo, S, k)
    wA, wQ, winfo = O.dynamics(mo)
    _same(A, wA, "A"), _same(Q, wQ, "Q")
    assert np.array_equal(_np(info), winfo) and winfo[S // 2] == 1 and np.isfinite(wA).all()
    assert not wA[S // 2].any() and not wA[0, 0].any() and np.array_equal(_np(Q), np.swapaxes(_np(Q), 1, 2))
    if S > 2:
        assert winfo[0] == 0 and winfo[S - 1] == 1 and wA[0].any()


@functools.lru_cache(maxsize=None)
def _oracle_closure():
    """the worst closure the oracle (eigh for Q) reaches over FIT_SHAPES on the moments of _direct_moments"""
    worst = 0.0
    for S, k in FIT_SHAPES:
        A, Q, _ = O.dynamics(_direct_moments(S, k))
        q, Uv = O.eigh_desc(Q)
        worst = max(worst, O.closure(O.noise(A, Uv, q)[0]))
    return worst


@pytest.mark.parametrize("S,k", FIT_SHAPES)
def test_noise_given_the_devices_eigenvectors_and_the_closure(S, k):
    from rawaudiovae_kelsey_amd import switching as SW
    mo = _direct_moments(S, k)
    A, Q, _ = _gpu_dynamics(mo, S, k)
    q, Uv, einfo = SW.eig_states(Q)
    assert _np(einfo)[:, 1].all()
    g, res = _out((2 * S * k * k + S,))
    dyn, shrink = SW.noise(_in64(_np(A)), _in64(_np(Uv)), _in64(_np(q)), out=res)
    torch.cuda.synchronize()
    g.assert_untouched("[dyn | g]")
    wdyn, wg = O.noise(_np(A), _np(Uv), _np(q))
    _same(dyn, wdyn, "dyn"), _same(shrink, wg, "g")
    closure, bound = O.closure(_np(dyn)), 8 * _oracle_closure()
    norms = [np.linalg.norm(d[0], 2) for d in _np(dyn)]
    print("S %d k %d: closure %.3g (bound %.3g = 8 x the oracle's worst), ||A||_2 up to %.9f, g from %.4g" % (
        S, k, closure, bound, max(norms), wg.min()))
    assert closure <= bound and max(norms) <= 1 + 1e-9 and (wg <= 1).all()
    assert (wg < 1).any() or k == 1


def test_the_guard_where_c1_is_one_and_a_half_d():
    from rawaudiovae_kelsey_amd import switching as SW
    S, k = 2, 3
    D = np.array([[4.0, 16.0, 0.25], [1.0, 64.0, 0.0625]])
    mo = dict(N=np.array([50.0, 60.0]), Dn=D, Dt=D, C1=np.stack([1.5 * np.diag(d) for d in D]))
    A, Q, _ = _gpu_dynamics(mo, S, k)
    assert np.array_equal(_np(A), np.stack([1.5 * np.eye(k)] * S))
    q, Uv, _ = SW.eig_states(Q)
    dyn, g = SW.noise(A, Uv, q)
    err = np.abs(_np(g) - 1 / 1.5)
    print("guard: g %s, |g - 1 / 1.5| / u %s, closure %.3g" % (_np(g), err / U, O.closure(_np(dyn))))
    assert (err <= 4 * U).all() and O.closure(_np(dyn)) <= 8 * _oracle_closure()
    assert np.allclose(_np(dyn)[:, 0], np.eye(k), atol=4 * U) and not _np(dyn)[:, 1].any()     # A = I, B = 0


@functools.lru_cache(maxsize=None)
def _planted_gpu():
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd import switching as SW
    x, rs, th, labels, At = O.planted()
    S, k = At.shape[0], At.shape[1]
    st = ST.LatentStates(S, k)._set(_dev(th), _dev(np.zeros(k)), _dev(np.eye(k)), x.shape[0], len(rs) - 1)
    return SW.SwitchingWalk(st).fit(_rows(x), rs)


def test_fit_of_the_planted_data_follows_the_oracles():
    sw = _planted_gpu()
    x, rs, th, labels, At = O.planted()
    f = O.planted_fit()
    S, k = At.shape[0], At.shape[1]
    got, want = _np(sw.phi_), f["phi"]
    err = np.abs(got - want).max()
    A = np.swapaxes(_np(sw.dyn_)[:, 0], 1, 2)
    rec = np.abs(A - At).max(axis=(1, 2))
    print("planted: |phi - oracle| %.3g (bound 1e-9); pairs %s; |A_j - planted| %s (gate %s); closure %.3g" % (
        err, sw.pairs_, rec, 8 / np.sqrt(sw.pairs_), O.closure(_np(sw.dyn_))))
    assert err <= 1e-9
    assert (rec <= 8 / np.sqrt(sw.pairs_)).all() and not sw.info_.any() and (sw.shrink_ == 1).all()
    assert np.allclose(sw.pairs_, f["mo"]["N"], rtol=1e-9) and np.allclose(sw.predictability_, (A * A).sum(axis=(1, 2)) / k)
    assert np.allclose(_np(sw.R_), np.eye(k)) and (sw.n_frames_, sw.n_files_) == (12000, 4)


# ---- RV_SWITCH_STEP ---------------------------------------------------------------------------------------------------------

def _small(x, layer, act):
    from rawaudiovae_kelsey_amd._lib import lib, ptr, stream_ptr
    w, b = layer.weight.detach(), layer.bias.detach()
    M, K = x.shape
    y = torch.empty((M, w.shape[0]), dtype=torch.float32, device=x.device)
    lib().rv_small_linear_f32(ptr(x), K, ptr(w), K, ptr(b), M, w.shape[0], K, act, ptr(y), w.shape[0], stream_ptr())
    return y


def _decode(model, z):
    return _small(_small(z.contiguous(), model.fc3, 1), model.fc4, 2)


@functools.lru_cache(maxsize=None)
def _setup(L, k, S):
    """(model, SwitchingWalk on the device, phi, R, c) of one step shape, shared and left unchanged.  At S = 3 the laws are
    binary fractions, so that a uniform can sit exactly on a cumulative edge, with zeros among them."""
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd import switching as SW
    torch.manual_seed(200 + L)
    model = VAE(SEG, HID, L).cuda().eval()
    c, P = SO.basis(k, L)
    phi = O.random_phi(S, k, zeros=True)
    if S == 3:
        o = O.phi_layout(S, k)
        phi[o["pi"]] = [0.5, 0.25, 0.25]
        phi[o["A"]] = np.array([[0.25, 0.25, 0.5], [0.5, 0.0, 0.5], [0.0, 1.0, 0.0]]).ravel()
    R = np.linalg.solve(P @ P.T, P)
    p = O.unpack_phi(phi, S, k)
    st = ST.LatentStates(S, k)._set(_dev(SO.pack(p["m"], p["sd"] ** 2, p["pi"], p["A"])), _dev(c), _dev(P), 10, 1)
    z = np.zeros(S)
    sw = SW.SwitchingWalk(st)._set(_dev(phi), st.mean_, st.P_, _dev(R), z, z + 1, z, 10, 1)
    return model, sw, phi, R, c


def _draws(n_streams, F, k, S, seed):
    g = torch.Generator().manual_seed(seed)
    eps = torch.randn((n_streams, F, k), generator=g)
    un = torch.rand((n_streams, F), generator=g)
    forced = torch.randint(-1, S + 1, (n_streams, F), generator=g).to(torch.int32)      # -1 and S: free
    forced[torch.rand((n_streams, F), generator=g) < 0.5] = -1
    return eps, un, forced


@pytest.mark.parametrize("L,k,S", STEP_SHAPES)
def test_step_is_bit_for_bit_and_the_audio_is_the_decode_of_the_latents(L, k, S):
    from rawaudiovae_kelsey_amd import switching as SW
    model, sw, phi, R, c = _setup(L, k, S)
    n, F = 3, 4
    gen = SW.StreamingSwitchingWalk(model, sw, n, F * SEG)
    temps = [1.0, 0.7, 1.3]
    gen.temperature.copy_(torch.tensor(temps))
    off = torch.linspace(-0.5, 0.5, L)
    gen.offset[1] = off.cuda()
    u = [np.zeros(k)] * n
    cur, primed = [0] * n, False
    for call in range(2):
        eps, un, forced = _draws(n, F, k, S, 10 * L + call)
        forced[0] = -1                                                          # stream 0 runs free ...
        if S == 3:                                                              # ... along the laws' edges
            un[0] = torch.tensor([0.5, 0.5, 0.99999994, 0.25] if call == 0 else [0.25, 0.75, 0.5, 0.5])
        y = gen.generate(eps.cuda(), un.cuda(), forced.cuda())
        z = gen.last_latents()
        assert torch.equal(y, _decode(model, z.reshape(-1, L)).view(n, F * SEG))                # hop == S, no window
        for s in range(n):
            u[s], cur[s], path, wz = O.step(phi, R, c, S, k, u[s], primed, cur[s], eps[s].numpy(), un[s].numpy(),
                                             forced[s].numpy(), temps[s], off.numpy() if s == 1 else None)
            what = "L %d k %d S %d call %d stream %d" % (L, k, S, call, s)
            _same(gen.state[s], u[s], "u " + what), _same(z[s], wz, "z " + what)
            assert np.array_equal(_np(gen.last_states()[s]), path) and int(gen.current_states()[s]) == cur[s], what
            if S == 3 and s == 0:
                assert path.tolist() == ([1, 2, 1, 0] if call == 0 else [1, 2, 1, 2]), path
            taken = (forced[s].numpy() >= 0) & (forced[s].numpy() < S)
            assert np.array_equal(path[taken], forced[s].numpy()[taken])
        primed = True
    assert int(gen._primed.sum()) == n and float(y.abs().max()) > 0 and bool(torch.isfinite(y).all())


def _randn(n, seed, offset):
    from rawaudiovae_kelsey_amd._lib import lib, ptr, stream_ptr
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    lib().rv_randn(ptr(out), n, seed, offset, stream_ptr())
    return out


def test_philox_draws_block_size_streams_and_seed():
    from rawaudiovae_kelsey_amd import switching as SW
    L, k, S = 17, 16, 3
    model, sw, phi, R, c = _setup(L, k, S)
    hop = SEG // 4
    make = lambda n, F, seed=77: SW.StreamingSwitchingWalk(model, sw, n, F * hop, hop, "hann", seed)   # noqa: E731

    def run(gen, calls, **draws):
        F = gen.frames_per_block
        ys, ps = [], []
        for b in range(calls):
            cut = {n: t[:, b * F:(b + 1) * F].contiguous() for n, t in draws.items()}
            ys.append(gen.generate(**cut).clone())
            ps.append(gen.last_states().clone())
        return torch.cat(ys, 1), torch.cat(ps, 1)

    a = make(3, 8)
    ya, pa = run(a, 1)
    b = make(3, 4)
    yb, pb = run(b, 2)
    assert torch.equal(ya, yb) and torch.equal(pa, pb) and torch.equal(a.state, b.state)       # 8 frames = two calls of 4
    assert torch.equal(a.current_states(), b.current_states())
    one = make(1, 4)
    y1, p1 = run(one, 2)
    assert torch.equal(y1[0], ya[0]) and torch.equal(p1[0], pa[0]) and torch.equal(one.state[0], a.state[0])   # alone = among three
    assert not torch.equal(ya[0], ya[1]) and not torch.equal(run(make(3, 8, 78), 1)[0], ya)
    # the Philox path is the explicit path fed rv_randn(seed, offset = stream) and the oracle's uniforms
    eps = torch.stack([_randn(8 * k, 77, s).view(8, k) for s in range(3)])
    un = torch.tensor([[O.state_uniform(77, f, s) for f in range(8)] for s in range(3)], dtype=torch.float32).cuda()
    ye, pe = run(make(3, 8), 1, eps=eps, uniforms=un)
    assert torch.equal(ye, ya) and torch.equal(pe, pa)
    assert len(set(_np(pa).ravel().tolist())) > 1 and bool(torch.isfinite(ya).all())


def test_graph_replay_equals_eager_and_sees_the_forced_states():
    from rawaudiovae_kelsey_amd import switching as SW
    from rawaudiovae_kelsey_amd._lib import RvError
    L, k, S = 17, 16, 3
    model, sw, _, _, _ = _setup(L, k, S)
    mine = copy.deepcopy(model)
    hop = SEG // 4
    eager = SW.StreamingSwitchingWalk(model, sw, 2, 2 * hop, hop, "hann", 21)
    graph = SW.StreamingSwitchingWalk(mine, sw, 2, 2 * hop, hop, "hann", 21)
    with pytest.raises(RvError, match="before capture"):
        graph.replay()
    graph.capture()
    for step in range(5):
        if step == 2:                                                           # written in place between replays
            for g in (eager, graph):
                g.forced.copy_(torch.tensor([[2, 2], [-1, 0]], dtype=torch.int32))
                g.temperature[1] = 0.25
        if step == 4:
            for g in (eager, graph):
                g.forced.fill_(-1)
        assert torch.equal(graph.replay(), eager.generate()), step
        assert torch.equal(graph.state, eager.state) and torch.equal(graph.last_latents(), eager.last_latents())
        assert torch.equal(graph.last_states(), eager.last_states())
        if step in (2, 3):
            assert _np(graph.last_states())[0].tolist() == [2, 2] and int(graph.last_states()[1, 1]) == 0
    mine.fc3.weight = torch.nn.Parameter(mine.fc3.weight.detach().clone())
    with pytest.raises(RvError, match="replaced after capture"):
        graph.replay()
    torch.cuda.synchronize()


def test_reset_set_state_and_prime():
    from rawaudiovae_kelsey_amd import switching as SW
    L, k, S = 17, 16, 3
    model, sw, phi, R, c = _setup(L, k, S)
    g = SW.StreamingSwitchingWalk(model, sw, 2, SEG)
    g.generate()
    g.reset(1)
    assert int(g._primed[1]) == 0 and int(g._primed[0]) == 1 and not g.state[1].any()
    u0 = torch.randn((2, k), generator=torch.Generator().manual_seed(1)).cuda()
    g.set_state(u0, [2, 0])
    assert torch.equal(g.state, u0.double()) and _np(g.current_states()).tolist() == [2, 0] and int(g._primed.sum()) == 2
    with pytest.raises(ValueError, match="u has shape"):
        g.set_state(u0[:, :3], [0, 0])
    with pytest.raises(ValueError, match="expected 2 states in \\[0, 3\\)"):
        g.set_state(u0, [0, 3])
    # prime: a latent row that sits on state 1's mean starts there with u = 0
    p = O.unpack_phi(phi, S, k)
    x = (c + p["m"][1] @ R).astype(np.float32)
    s = g.prime(torch.from_numpy(x).cuda())
    assert s == 1 and _np(g.current_states()).tolist() == [1, 1] and int(g._primed.sum()) == 2
    assert np.abs(_np(g.state)).max() <= 1e-4                                   # x is rounded to fp32, nothing else
    # ... and one standard deviation out along axis 0 has u = e_0
    x = (c + (p["m"][1] + p["sd"][1] * np.eye(k)[0]) @ R).astype(np.float32)
    assert g.prime(torch.from_numpy(x).cuda(), 0) == 1
    assert np.abs(_np(g.state[0]) - np.eye(k)[0]).max() <= 1e-4


def test_argument_errors_name_the_field_and_touch_nothing():
    from rawaudiovae_kelsey_amd import _lib
    from rawaudiovae_kelsey_amd import switching as SW
    from rawaudiovae_kelsey_amd._lib import MosaicDesc, RvError, lib, ptr, stream_ptr
    L, k, S = 17, 16, 3
    model, sw, _, _, _ = _setup(L, k, S)
    g = SW.StreamingSwitchingWalk(model, sw, 2, 16, 8, "hann", 1)
    g.generate()
    torch.cuda.synchronize()
    held = (g.stream._ws, g.state, g._primed, g._current, g._path, g._z)
    before = [t.clone() for t in held]
    y = torch.zeros((2, 16), device="cuda")

    def step(**change):
        sd = g.stream.desc(g._silence, y, None)
        for name in [n for n in change if n.startswith("live_")]:
            setattr(sd, name[5:], change.pop(name))
        f = dict(live=C.pointer(sd), S=S, k=k, L=L, ldo=L, centre=ptr(sw.mean_), basis=ptr(sw.R_), moment=ptr(sw.phi_),
                 out=ptr(g._z), state=ptr(g._state), primed=ptr(g._primed), idx=ptr(g._current), path=ptr(g._path))
        f.update(change)
        lib().rv_mosaic(_lib.SWITCH_STEP, C.byref(MosaicDesc(**f)), stream_ptr())

    for change, msg in ((dict(k=0), "k=0 \\(the axes\\) outside"), (dict(k=65), "k=65 \\(the axes\\) outside"),
                        (dict(S=0), "S=0 \\(the states\\) outside"), (dict(S=65), "S=65 \\(the states\\) outside"),
                        (dict(L=15), "L=15 outside \\[k=16, 512\\]"), (dict(L=18), "L=18, the stream's model has L=17"),
                        (dict(L=513), "L=513 outside"), (dict(centre=None), "centre is null"),
                        (dict(basis=None), "basis \\(R\\) is null"), (dict(moment=None), "moment \\(phi\\) is null"),
                        (dict(state=None), "the state is null"), (dict(primed=None), "the primed flags are null"),
                        (dict(idx=None), "idx \\(the current states\\) is null"), (dict(path=None), "path \\(the states out\\) is null"),
                        (dict(ldo=16), "ldo=16 holds no row"), (dict(live=None), "\\(live\\) is null"),
                        (dict(live_temperature=None), "live->temperature is null"), (dict(live_y=None), "null buffer")):
        with pytest.raises(RvError, match="SWITCH_STEP.*" + msg if "null buffer" not in msg else msg):
            step(**change)
    for what, shape in (("eps", (2, 2, 17)), ("uniforms", (2, 3))):
        with pytest.raises(ValueError, match=what + " has shape"):
            g.generate(**{what: torch.zeros(shape, device="cuda")})
    with pytest.raises(ValueError, match="states has shape"):
        g.generate(states=torch.zeros((2, 2), device="cuda"))
    torch.cuda.synchronize()
    for t, b in zip(held, before):
        assert torch.equal(t, b)


# ---- statistics -------------------------------------------------------------------------------------------------------------

def _standard_errors(At, v, n, lags=512):
    """(se of the mean, se of the variance) [k] of n frames of y = m + sd o u, u a stationary Gaussian VAR(1) with Cov I and
    autocovariance A^h: se_mean^2 = (v / n) (1 + 2 sum_h (1 - h / n) rho_h), se_var^2 = (2 v^2 / n) (1 + 2 sum_h (1 - h / n)
    rho_h^2), rho_h = (A^h)_ii (Bartlett)."""
    A = At.T
    k = A.shape[0]
    s1, s2, M = np.ones(k), np.ones(k), np.eye(k)
    for h in range(1, lags):
        M = A @ M
        rho = np.diag(M)
        s1, s2 = s1 + 2 * (1 - h / n) * rho, s2 + 2 * (1 - h / n) * rho * rho
    return np.sqrt(v / n * s1), np.sqrt(2 * v * v / n * s2)


def test_statistics_of_4096_frames():
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd import switching as SW
    S, k, n = 3, 3, 4096
    torch.manual_seed(5)
    model = VAE(16, 8, k).cuda().eval()
    phi = O.random_phi(S, k, seed=3)
    p = O.unpack_phi(phi, S, k)
    st = ST.LatentStates(S, k)._set(_dev(SO.random_theta(S, k)), _dev(np.zeros(k)), _dev(np.eye(k)), 10, 1)
    z = np.zeros(S)
    sw = SW.SwitchingWalk(st)._set(_dev(phi), st.mean_, st.P_, _dev(np.eye(k)), z, z + 1, z, 10, 1)    # L = k, R = I: z = y
    F = 1024
    gen = SW.StreamingSwitchingWalk(model, sw, S + 1, F * 16, seed=2024)
    forced = torch.full((S + 1, F), -1, dtype=torch.int32)
    for j in range(S):
        forced[j] = j                                                           # stream j is held in state j; the last runs free
    ys, paths = [], []
    for _ in range(n // F):
        gen.generate(states=forced.cuda())
        ys.append(_np(gen.last_latents()).astype(np.float64))
        paths.append(_np(gen.last_states()))
    y, path = np.concatenate(ys, 1), np.concatenate(paths, 1)
    for j in range(S):
        assert (path[j] == j).all()
        v = p["sd"][j] ** 2
        se_m, se_v = _standard_errors(p["dyn"][j, 0], v, n)
        dm, dv = np.abs(y[j].mean(0) - p["m"][j]) / se_m, np.abs(y[j].var(0) - v) / se_v
        print("state %d: |mean - m| / se %s, |var - v| / se %s" % (j, dm, dv))
        assert (dm <= 5).all() and (dv <= 5).all()
    free = path[S]
    counts = np.zeros((S, S))
    np.add.at(counts, (free[:-1], free[1:]), 1)
    rows = counts.sum(1)
    se = np.sqrt(p["A"] * (1 - p["A"]) / rows[:, None])
    dev = np.abs(counts / rows[:, None] - p["A"]) / se
    print("free: transitions from each state %s, worst |share - A_hmm| / se %.3g" % (rows, dev.max()))
    assert (rows > 200).all() and (dev <= 5).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------

def test_compose_py_fit_then_run_with_a_form_and_segment_py_split(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import compose as cli
    import segment
    import states as states_cli
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd.synth import make_params
    S, H, LAT, SR, hop = 64, 32, 8, 8000, 16
    model = VAE(S, H, LAT).cuda().eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(S, H, LAT, 0).items()})
    rng = np.random.default_rng(11)
    t = np.arange(2100) / SR
    waves = [(0.5 * np.sin(2 * np.pi * 330 * t) + 0.2 * rng.standard_normal(t.size)).astype(np.float32),
             (0.7 * rng.uniform(-1, 1, 1333)).astype(np.float32)]
    (tmp_path / "audio").mkdir()
    for i, w in enumerate(waves):
        D.write_wav(tmp_path / "audio" / ("%d.wav" % i), w, SR)
    ini = tmp_path / "m.ini"
    ini.write_text("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n" % (SR, S, H, LAT))
    ck = tmp_path / "ckpt"
    torch.save({"epoch": 0, "state_dict": model.state_dict(), "optimizer": {}}, ck)
    common = ["--config", str(ini), "--checkpoint", str(ck), "--hop", str(hop)]
    npz, form = tmp_path / "states.npz", tmp_path / "form.npz"
    states_cli.main(["fit"] + common + ["--data", str(tmp_path / "audio"), "--states", "3", "--keep", "4", "--iters", "8",
                                        "--out", str(npz)])
    capsys.readouterr()
    rep = cli.main(["fit"] + common + ["--data", str(tmp_path / "audio"), "--states", str(npz), "--out", str(form)])
    out = capsys.readouterr().out.strip().splitlines()
    assert json.loads(out[-1]) == rep and rep["n_files"] == 2 and rep["keep"] == 4
    assert [s["letter"] for s in rep["states"]] == ["A", "B", "C"]
    for s in rep["states"]:
        assert 0 < s["shrink"] <= 1 and 0 <= s["predictability"] <= 1 + 1e-9 and s["flag"] in (0, 1) and s["pairs"] >= 0
    assert abs(sum(s["pairs"] for s in rep["states"]) - (rep["n_frames"] - 2)) < 1e-6
    # 0.1 s = 50 frames at hop 16: A, then C, then free, then A again; the rest of the second free
    wav, lab = tmp_path / "out.wav", tmp_path / "labels.json"
    y, played = cli.main(["run"] + common + ["--model", str(form), "--seconds", "0.5", "--out", str(wav), "--window", "hann",
                                             "--form", "A:0.1,C:0.1,*:0.1,A:0.1", "--labels", str(lab), "--seed", "3"])
    assert y.shape == (1, 4000) and played.shape == (1, 250) and np.isfinite(y).all() and np.abs(y).max() > 0
    assert (played[0, :50] == 0).all() and (played[0, 50:100] == 2).all() and (played[0, 150:200] == 0).all()
    assert set(played[0].tolist()) <= {0, 1, 2}
    report = json.loads(lab.read_text())
    assert report["labels"][:2] == [0, 2] and report["boundary_frames"][0] == 50 and report["states"] == 3
    assert report["samples"] == 4000 and report["hop"] == hop and report["form"].startswith("A C")
    assert np.array_equal(D.load_audio_mono(str(wav), SR), y[0])
    names = segment.main(["split", "--segments", str(lab), "--in", str(wav), "--out-dir", str(tmp_path / "cut")])
    assert len(names) == report["segments"]
    assert np.array_equal(np.concatenate([D.load_audio_mono(n, SR) for n in names]), y[0])
    # the same seed gives the same file; two streams under one form; a start from a wav
    again, _ = cli.main(["run"] + common + ["--model", str(form), "--seconds", "0.5", "--out", str(wav), "--window", "hann",
                                            "--form", "A:0.1,C:0.1,*:0.1,A:0.1", "--seed", "3"])
    assert np.array_equal(again, y)
    two, p2 = cli.main(["run"] + common + ["--model", str(form), "--seconds", "0.1", "--out", str(wav), "--streams", "2",
                                           "--form", "B:1", "--start", str(tmp_path / "audio" / "0.wav"),
                                           "--labels", str(lab)])
    assert two.shape == (2, 800) and (p2 == 1).all() and not np.array_equal(two[0], two[1])
    assert (tmp_path / "out_1.wav").exists() and json.loads((tmp_path / "labels_1.json").read_text())["labels"] == [1]
    with pytest.raises(ValueError, match="--form 'A:1,D:2': unknown letter D: the model has 3 states"):
        cli.main(["run"] + common + ["--model", str(form), "--seconds", "0.1", "--out", str(wav), "--form", "A:1,D:2"])
    with pytest.raises(ValueError, match="--hop: hop 32: the switching walk was fitted at hop 16"):
        cli.main(["run", "--config", str(ini), "--checkpoint", str(ck), "--hop", "32", "--model", str(form), "--seconds", "0.1",
                  "--out", str(wav)])
    with pytest.raises(ValueError, match="--model: .*not a latent-switching file"):
        cli.main(["run"] + common + ["--model", str(npz), "--seconds", "0.1", "--out", str(wav)])
