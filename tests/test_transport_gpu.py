"""Latent transport on the GPU (RV_OT_*, csrc/transport.hip, rawaudiovae_kelsey_amd/transport.py, transfer.py) against
tests/transport_oracle.py.

Inputs between NaN guards and outputs between sentinel guards (tests/guarded.py), x with a row pitch of L + 3 and NaN in the
gaps.  Bit for bit: WHITEN against the float64 chain; the exact limit (lattice points, eps = 2^-11: every other weight is an
exact 0) for every row; a row alone, in blocks of 4 and among 130; two runs; alpha = 0; a row that is not finite.  Gated
against the longdouble oracle: SOFTMIN and MAP, each error as a fraction of its derived ceiling (the oracle's module doc),
each gate 4 x the largest fraction measured on the MI355X and never above the ceiling itself.  Every test prints what it
measures before it asserts.

The tool on a tiny model (S 64, H 32, L 8, k 4): the fit reaches its tolerance and follows the oracle's loop, the live path
equals the offline one bit for bit, eagerly and through a captured graph, and transfer.py writes the same file either way."""
import json
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import guarded as G  # noqa: E402
import states_oracle as SO  # noqa: E402
import transport_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

sys.path.insert(0, REPO)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if torch.is_tensor(a) else a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


def _same(got, want, what):
    got, want = _bits(got), _bits(want if torch.is_tensor(want) else np.asarray(want))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d elements differ, the first at %d" % (what, bad.size, got.size, bad[0])


def _in64(a):
    """a float64 input between NaN guards, as a device tensor of a's shape"""
    a = np.asarray(a, np.float64)
    return G.guarded_flat(a.size, torch.float64, a.reshape(-1)).view.view(a.shape)


def _out(shape, dtype=torch.float64, fill=G.SENTINEL):
    g = G.guarded_flat(int(np.prod(shape)), dtype, fill)
    return g, g.view.view(shape)


def _rows(x, pad=3):
    """x [T, L] fp32 with a row pitch of L + pad, NaN in the gaps and guards"""
    return G.guarded(x.shape[0], x.shape[1], x.shape[1] + pad, torch.float32, x).view


def _TR():
    from rawaudiovae_kelsey_amd import transport as TR
    return TR


# ---- kernel level -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", O.WHITEN_L)
def test_whiten_equals_the_oracle_chain_bit_for_bit(L):
    TR = _TR()
    for k in (k for k in O.WHITEN_K if k <= L):
        c, P = SO.basis(k, L)
        cd, Pd = _in64(c), _in64(P)
        for T in O.WHITEN_T:
            x = SO.latents(T, L)
            x[T // 2, L - 1] = np.nan                      # one row that is not finite
            if T > 2:
                x[T - 1, 0] = np.inf
            gy, y = _out((T, k))
            gi, info = _out((T,), torch.int32, G.INT_FILL)
            TR.whiten(_rows(x), cd, Pd, out=(y, info))
            torch.cuda.synchronize()
            gy.assert_untouched("y")
            gi.assert_untouched("info")
            want_y, want_obs = O.whiten(x, c, P)
            _same(y, want_y, "y L %d k %d T %d" % (L, k, T))
            assert np.array_equal(_np(info), want_obs) and want_obs[T // 2] == 0 and (_np(y)[T // 2] == 0).all()
            assert not np.signbit(_np(y)[T // 2]).any()


def _lw(mask):
    with np.errstate(divide="ignore"):
        return np.where(mask, -np.log(float(mask.sum())), -np.inf)


@pytest.mark.parametrize("k,N,T", O.CASES)
def test_softmin_stays_within_its_gate_of_the_oracle(k, N, T):
    TR = _TR()
    A, B, h, cost = O.case(k, N, T)
    Ad, Bd = _in64(A), _in64(B)
    worst = 0.0
    for rel in O.EPSILONS:
        eps = O.eps32(rel * cost)
        ds, _ = O.delta_s(A, B, eps, k)
        for name, mask in O.masks(N).items():
            lw = _lw(mask)
            g, f = _out((T,))
            TR.softmin(Ad, Bd, _in64(np.concatenate([h, lw])), eps, out=f)
            torch.cuda.synchronize()
            g.assert_untouched("f")
            want = O.softmin(A, B, h, lw, eps)
            got = _np(f)
            assert np.isfinite(got).all() and np.isfinite(want).all()
            frac = float((np.abs(got - want) / eps / ds).max())
            print("softmin k %d N %d T %d eps %g x cost, mask %s: |df| / eps = %.3g of its ceiling" % (k, N, T, rel, name, frac))
            worst = max(worst, frac)
    print("softmin k %d N %d T %d: worst %.4g of the ceiling (gate %.4g)" % (k, N, T, worst, O.GATE_F))
    assert worst <= O.GATE_F <= 1.0


def test_softmin_of_a_row_with_no_column_of_finite_weight_is_plus_infinity():
    TR = _TR()
    A, B, h, cost = O.case(3, 257, 17)
    f = TR.softmin(_in64(A), _in64(B), _in64(np.concatenate([h, np.full(257, -np.inf)])), cost)
    assert np.isposinf(_np(f)).all()


def _map_once(TR, x, c, P, W, V, gl, eps, k, alpha, pad=3):
    T, L = x.shape
    go = G.guarded(T, L, L + 2, torch.float32)
    gs, state = _out((T, 3 + k))
    block = _in64(np.concatenate([c, P.reshape(-1), W.reshape(-1)]))
    amount = None if alpha is None else torch.full((1,), alpha, dtype=torch.float32, device="cuda")
    TR.transport_map(_rows(x, pad), block, _in64(V), _in64(gl), eps, k, amount=amount, out=go.view, state=state)
    torch.cuda.synchronize()
    go.assert_untouched("out")
    gs.assert_untouched("state")
    return _np(go.payload()), _np(state)


@pytest.mark.parametrize("k,N,T", O.CASES)
def test_map_stays_within_its_gates_of_the_oracle(k, N, T):
    TR = _TR()
    x, c, P, W, V, g, cost = O.map_case(k, N, T)
    y, obs = O.whiten(x, c, P)
    assert obs.all()
    worst = dict(f=0.0, T=0.0, support=0.0, cbar=0.0)
    vmax = np.abs(V).max()
    for rel, alpha in zip(O.EPSILONS, O.AMOUNTS):
        eps = O.eps32(rel * cost)
        ds, C = O.delta_s(y, V, eps, k)
        for name, mask in O.masks(N).items():
            lw = _lw(mask)
            out, state = _map_once(TR, x, c, P, W, V, np.concatenate([g, lw]), eps, k, alpha)
            want = O.transport_map(y, V, g, lw, eps)
            assert np.isfinite(state).all()
            cmax = want["c"][:, mask].max(axis=1).astype(np.float64)
            frac = dict(f=np.abs(state[:, 0] - want["f"]) / eps / ds,
                        T=np.abs(state[:, 3:] - want["T"]).max(axis=1) / (4 * ds * vmax),
                        support=np.abs(state[:, 1] / want["support"] - 1) / (8 * ds),
                        cbar=np.abs(state[:, 2] - want["cbar"]) / (4 * ds * cmax + 8 * (k + 8) * O.U * C))
            frac = {n: float(v.max()) for n, v in frac.items()}
            print("map k %d N %d T %d eps %g x cost, alpha %g, mask %s: of the ceilings %s" % (
                k, N, T, rel, alpha, name, " ".join("%s %.3g" % kv for kv in frac.items())))
            worst = {n: max(worst[n], frac[n]) for n in worst}
            # the latent rows: the oracle's x' rounded to float32, give or take what the ceiling of T moves it by
            exact = O.moved(x, y, want["T_ld"], W, alpha)
            slack = abs(alpha) * (4 * ds * vmax)[:, None] * np.abs(W).sum(axis=1)[None, :] + 4 * O.U * np.abs(exact).astype(np.float64)
            half_ulp = 0.5 * np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
            assert (np.abs(out.astype(np.float64) - exact.astype(np.float64)) <= half_ulp * (1 + 1e-6) + slack).all()
            if alpha == 0:
                _same(out, x, "out at alpha 0")
        if alpha != 0:         # alpha = 0 at this epsilon too: the input's bits whatever the weights look like
            lw = _lw(np.ones(N, bool))
            _same(_map_once(TR, x, c, P, W, V, np.concatenate([g, lw]), eps, k, 0.0)[0], x, "out at alpha 0, eps %g x cost" % rel)
    print("map k %d N %d T %d: worst of the ceilings %s (gates f %.3g T %.3g support %.3g cbar %.3g)" % (
        k, N, T, " ".join("%s %.4g" % kv for kv in worst.items()), O.GATE_F, O.GATE_T, O.GATE_SUPPORT, O.GATE_CBAR))
    assert worst["f"] <= O.GATE_F <= 1 and worst["T"] <= O.GATE_T <= 1
    assert worst["support"] <= O.GATE_SUPPORT <= 1 and worst["cbar"] <= O.GATE_CBAR <= 1


def test_map_in_place_equals_the_map_into_another_buffer():
    TR = _TR()
    k, N, T = 17, 515, 65
    x, c, P, W, V, g, cost = O.map_case(k, N, T)
    gl = np.concatenate([g, _lw(np.ones(N, bool))])
    want, want_state = _map_once(TR, x, c, P, W, V, gl, cost, k, 0.5)
    L = x.shape[1]
    buf = G.guarded(T, L, L + 3, torch.float32)
    buf.view.copy_(torch.from_numpy(x).cuda())
    gs, state = _out((T, 3 + k))
    block = _in64(np.concatenate([c, P.reshape(-1), W.reshape(-1)]))
    TR.transport_map(buf.view, block, _in64(V), _in64(gl), cost, k, amount=0.5, out=buf.view, state=state)
    torch.cuda.synchronize()
    buf.assert_untouched("x = out")
    gs.assert_untouched("state")
    _same(buf.payload(), want, "out written over x")
    _same(state, want_state, "state")
    assert not np.array_equal(want, x)


def test_map_without_an_amount_moves_every_row_all_the_way():
    TR = _TR()
    x, c, P, W, V, g, cost = O.map_case(3, 15, 15)
    gl = np.concatenate([g, _lw(np.ones(15, bool))])
    one, s1 = _map_once(TR, x, c, P, W, V, gl, cost, 3, 1.0)
    none, s2 = _map_once(TR, x, c, P, W, V, gl, cost, 3, None)
    _same(none, one, "out")
    _same(s2, s1, "state")
    assert not np.array_equal(one, x)


@pytest.mark.parametrize("k,N,T", [(1, 17, 33), (3, 515, 130), (64, 300, 65)])
def test_the_exact_limit_every_row_lands_on_its_nearest_lattice_point(k, N, T):
    TR = _TR()
    Q, V, near = O.lattice_case(k, N, T)
    x = Q.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), Q)
    c, P = np.zeros(k), np.eye(k)
    gl = np.concatenate([np.zeros(N), _lw(np.ones(N, bool))])
    out, state = _map_once(TR, x, c, P, np.eye(k), V, gl, 2.0 ** -11, k, 1.0)
    _same(state[:, 3:], V[near], "the coordinates")
    assert (state[:, 1] == 1.0).all()
    _same(out, V[near].astype(np.float32), "the latent rows")
    assert np.allclose(state[:, 2], ((Q - V[near]) ** 2).sum(axis=1), rtol=0, atol=1e-9)


def test_a_row_is_the_same_alone_in_blocks_of_four_and_among_130_and_two_runs_are_bit_equal():
    TR = _TR()
    k, N, T = 17, 515, 130
    x, c, P, W, V, g, cost = O.map_case(k, N, T)
    mask = np.ones(N, bool)
    mask[::7] = False
    gl = np.concatenate([g, _lw(mask)])
    eps = O.eps32(cost)
    out, state = _map_once(TR, x, c, P, W, V, gl, eps, k, 0.5)
    again = _map_once(TR, x, c, P, W, V, gl, eps, k, 0.5)
    _same(again[0], out, "out, the second run")
    _same(again[1], state, "state, the second run")
    for rows in (1, 4):       # every row alone; every block of 4, the last one of 2 rows
        for r0 in range(0, T, rows):
            o, s = _map_once(TR, x[r0:r0 + rows], c, P, W, V, gl, eps, k, 0.5)
            _same(o, out[r0:r0 + rows], "out rows %d..%d alone" % (r0, r0 + rows))
            _same(s, state[r0:r0 + rows], "state rows %d..%d alone" % (r0, r0 + rows))
    y, _ = O.whiten(x, c, P)
    hl = _in64(np.concatenate([g, _lw(mask)]))
    f1, f2 = (TR.softmin(_in64(y), _in64(V), hl, eps) for _ in range(2))
    _same(f1, f2, "softmin, the second run")


def test_a_row_that_is_not_finite_passes_through_and_changes_no_other_row():
    TR = _TR()
    k, N, T = 3, 257, 130
    x, c, P, W, V, g, cost = O.map_case(k, N, T)
    gl = np.concatenate([g, _lw(np.ones(N, bool))])
    clean = _map_once(TR, x, c, P, W, V, gl, cost, k, 1.0)
    holes = x.copy()
    holes[0, 2], holes[63, 4], holes[64], holes[129, 0] = np.nan, np.inf, np.nan, -np.inf
    out, state = _map_once(TR, holes, c, P, W, V, gl, cost, k, 1.0)
    gone = np.zeros(T, bool)
    gone[[0, 63, 64, 129]] = True
    _same(out[gone], holes[gone], "the rows that are not finite")
    assert np.isnan(state[gone][:, 0]).all() and (state[gone][:, 1] == 0).all() and np.isnan(state[gone][:, 2:]).all()
    _same(out[~gone], clean[0][~gone], "the other rows")
    _same(state[~gone], clean[1][~gone], "the other rows' diagnostics")
    # a finite row with no column of finite weight passes through too
    none = _map_once(TR, x[:5], c, P, W, V, np.concatenate([g, np.full(N, -np.inf)]), cost, k, 1.0)
    _same(none[0], x[:5], "rows with nowhere to go")
    assert np.isposinf(none[1][:, 0]).all() and (none[1][:, 1] == 0).all() and np.isnan(none[1][:, 2:]).all()


# ---- tool level ---------------------------------------------------------------------------------------------------------

S, H, LAT, K, SR = 64, 32, 8, 4, 8000


def _model():
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.synth import make_params
    m = VAE(S, H, LAT).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(S, H, LAT, 0).items()})
    return m


def _waves():
    """(source, target, a recording to transfer): a second or so each"""
    rng = np.random.default_rng(21)
    t = np.arange(9000) / SR
    src = 0.5 * np.sin(2 * np.pi * 220 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.05 * rng.standard_normal(t.size)
    tgt = 0.4 * np.sign(np.sin(2 * np.pi * 330 * t)) * (0.5 + 0.5 * np.cos(2 * np.pi * 2 * t)) + 0.1 * rng.standard_normal(t.size)
    t2 = np.arange(2500) / SR
    rec = 0.5 * np.sin(2 * np.pi * 180 * t2 + 3 * np.sin(2 * np.pi * 5 * t2)) + 0.05 * rng.standard_normal(t2.size)
    return src.astype(np.float32), tgt.astype(np.float32), rec.astype(np.float32)


def _planted_clouds(n=200, L=LAT, seed=8):
    """Latent rows of two planted clouds: the target a few blobs, the source the same blobs moved and stretched"""
    rng = np.random.default_rng(seed)
    blobs = rng.standard_normal((4, L)) * 2
    xt = blobs[rng.integers(0, 4, n)] + 0.3 * rng.standard_normal((n, L))
    xs = 1.3 * (blobs[rng.integers(0, 4, n + 30)] + 0.3 * rng.standard_normal((n + 30, L))) + 1.5
    xs[5] = np.nan
    return xs.astype(np.float32), xt.astype(np.float32)


def test_fit_reaches_its_tolerance_and_follows_the_oracles_loop():
    TR = _TR()
    xs, xt = _planted_clouds()
    both = np.concatenate([xs[np.isfinite(xs).all(axis=1)], xt]).astype(np.float64)
    c = both.mean(axis=0)
    lam, vec = np.linalg.eigh(np.cov((both - c).T))
    P = (vec[:, ::-1][:, :K] / np.sqrt(lam[::-1][:K])).T.copy()
    tr = TR.LatentTransport(K, epsilon=0.05, iters=500, tol=1e-3)
    hist = tr.fit(torch.from_numpy(xs).cuda(), torch.from_numpy(xt).cuda(), (c, P))
    ys, obs_s = O.whiten(xs, c, P)
    yt, obs_t = O.whiten(xt, c, P)
    _same(tr.ys_, ys, "the source cloud")
    _same(tr.yt_, yt, "the target cloud")
    lws, lwt = O.log_weights(obs_s), O.log_weights(obs_t)
    assert np.array_equal(_np(tr.lws_), lws) and np.array_equal(_np(tr.lwt_), lwt) and np.isneginf(lws[5])
    ref = O.sinkhorn(ys, lws, yt, lwt, 0.05, 500, 1e-3)
    print("fit: %d iterations, error %.3g (oracle %d, %.3g), epsilon %.6g, cost %.6g" % (
        tr.n_iter_, tr.err_, ref["n_iter"], ref["err"], tr.epsilon_, tr.cost_))
    assert tr.err_ <= 1e-3 and hist[-1][1] == tr.err_ and tr.n_iter_ == ref["n_iter"] and tr.epsilon_ == ref["epsilon"]
    assert abs(tr.mean_cost_ - ref["cost"]) <= 1e-12 * ref["cost"]
    seen = lws > -np.inf
    ds = max(O.delta_s(ys[seen], yt, tr.epsilon_, K)[0].max(), O.delta_s(yt, ys[seen], tr.epsilon_, K)[0].max())
    df = np.abs(_np(tr.f_) - ref["f"])[seen].max() / tr.epsilon_ / ds
    dg = np.abs(_np(tr.g_) - ref["g"]).max() / tr.epsilon_ / ds
    print("potentials after %d iterations: |df| / eps %.3g, |dg| / eps %.3g of the ceiling (gate %d x %.3g)" % (
        tr.n_iter_, df, dg, tr.n_iter_, O.GATE_F))
    assert max(df, dg) <= tr.n_iter_ * O.GATE_F
    want = O.transport_map(ys, yt, ref["g"], lwt, ref["epsilon"])
    cost = float((np.exp(lws)[seen] * want["cbar"][seen]).sum())
    dsm, C = O.delta_s(ys[seen], yt, tr.epsilon_, K)
    ceiling = float((4 * (tr.n_iter_ * O.GATE_F + O.GATE_CBAR) * dsm * want["c"][seen].max(axis=1).astype(np.float64)).max()
                    + 8 * (K + 8) * O.U * C.max())
    print("cost %.9g, the oracle's %.9g, apart by %.3g (ceiling %.3g); distance %.6g" % (
        tr.cost_, cost, abs(tr.cost_ - cost), ceiling, np.sqrt(tr.cost_)))
    assert abs(tr.cost_ - cost) <= ceiling
    # the map carries the source's mass onto the target: the images' mean is the target's mean to the marginal error
    _, diag = tr.map(torch.from_numpy(xs).cuda())
    img = _np(diag["coords"])[seen]
    assert np.abs(img.mean(axis=0) - yt.mean(axis=0)).max() <= 1e-3 * np.abs(yt).max() * 2
    back, _ = tr.map(tr.map(torch.from_numpy(xt).cuda(), reverse=True)[0])
    assert np.isfinite(_np(back)).all()


def _fitted(model, hop):
    TR = _TR()
    from rawaudiovae_kelsey_amd.corpus import encode_corpus
    src, tgt, _ = _waves()
    xs, _ = encode_corpus(model, [src], hop)
    xt, _ = encode_corpus(model, [tgt], hop)
    tr = TR.LatentTransport(K, epsilon=0.1, iters=100, tol=1e-3)
    tr.fit(xs[::4].contiguous(), xt[::4].contiguous(), None)
    return tr


def _run(st, x, replay=False, before_block=None):
    ys, sup = [], []
    for b in range(x.shape[1] // st.block):
        if before_block is not None:
            before_block(b)
        xb = x[:, b * st.block:(b + 1) * st.block]
        ys.append((st.replay(xb) if replay else st.process(xb)).clone())
        sup.append(st.last_diagnostics()["support"].clone())
    return torch.cat(ys, 1), torch.cat(sup, 1)


@pytest.mark.parametrize("n_streams", [1, 3])
def test_live_equals_the_offline_transfer_of_the_zero_prefixed_recording(n_streams):
    TR = _TR()
    model, hop, window = _model(), 16, "hann"
    tr = _fitted(model, hop)
    rng = np.random.default_rng(n_streams)
    n = 4 * 256
    t = np.arange(n)
    x = np.stack([0.5 * np.sin(t * (0.05 + 0.03 * s)) for s in range(n_streams)]) + 0.1 * rng.standard_normal((n_streams, n))
    x = torch.from_numpy(x.astype(np.float32)).cuda()
    amounts = [1.0, 0.5, 0.0][:n_streams]
    refs = []
    for s in range(n_streams):
        w = torch.cat([torch.zeros(S - hop, device="cuda"), x[s]])
        y, diag = TR.transfer(model, w, tr, hop, window, amounts[s])
        refs.append((y[:n], diag["support"][:n // hop]))
    for block, replay in ((64, False), (256, False), (64, True)):
        st = TR.StreamingTransport(model, tr, n_streams, block, hop, window)
        st.amount.copy_(torch.tensor(amounts))
        assert st.latency == S - hop and st.frames_per_block == block // hop
        if replay:
            st.capture()
        y, sup = _run(st, x, replay)
        for s in range(n_streams):
            _same(y[s], refs[s][0], "stream %d, blocks of %d%s" % (s, block, ", replayed" if replay else ""))
            _same(sup[s], refs[s][1], "support of stream %d" % s)
        mu, _ = st.last_latents()
        assert mu.shape == (n_streams, block // hop, LAT)
    # amount, written in place, changes a replayed block; reset() starts over
    st.reset()
    first = st.replay(x[:, :64]).clone()
    st.reset()
    st.amount.zero_()
    plain = st.replay(x[:, :64]).clone()
    st.reset()
    st.amount.copy_(torch.tensor(amounts))
    assert not torch.equal(first[0], plain[0])
    _same(st.replay(x[:, :64]), first, "the first block after a reset")


def test_transfer_py_fit_then_apply_offline_and_live_write_the_same_file(tmp_path, capsys):
    import transfer as cli
    from rawaudiovae_kelsey_amd import data as D
    src, tgt, rec = _waves()
    (tmp_path / "src").mkdir()
    D.write_wav(tmp_path / "src" / "a.wav", src[:5000], SR)
    D.write_wav(tmp_path / "src" / "b.wav", src[5000:], SR)
    D.write_wav(tmp_path / "tgt.wav", tgt, SR)
    D.write_wav(tmp_path / "in.wav", rec, SR)
    ini = tmp_path / "m.ini"
    ini.write_text("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n" % (SR, S, H, LAT))
    ck = tmp_path / "ckpt"
    torch.save({"epoch": 0, "state_dict": _model().state_dict(), "optimizer": {}}, ck)
    common = ["--config", str(ini), "--checkpoint", str(ck), "--hop", "16"]
    npz = tmp_path / "transport.npz"
    rep = cli.main(["fit"] + common + ["--source", str(tmp_path / "src"), "--target", str(tmp_path / "tgt.wav"), "--keep", str(K),
                                       "--epsilon", "0.1", "--iters", "100", "--max-frames", "150", "--out", str(npz)])
    out = capsys.readouterr().out.strip().splitlines()
    assert json.loads(out[-1]) == rep and out[0].startswith("source: %d of %d frames (every %d)" % (
        rep["source_frames"], rep["source_frames_read"], rep["source_stride"]))
    assert rep["source_frames"] <= 150 and rep["target_frames"] <= 150 and rep["source_stride"] == -(-rep["source_frames_read"] // 150)
    assert rep["marginal_error"] <= 1e-3 and rep["distance"] == np.sqrt(rep["cost_per_frame"]) and rep["median_support"] >= 1
    apply = ["apply"] + common + ["--transport", str(npz), "--in", str(tmp_path / "in.wav"), "--window", "hann"]
    off = cli.main(apply + ["--out", str(tmp_path / "off.wav")])
    live = cli.main(apply + ["--out", str(tmp_path / "live.wav"), "--live-block", "256"])
    a, b = D.load_audio_mono(str(tmp_path / "off.wav"), SR), D.load_audio_mono(str(tmp_path / "live.wav"), SR)
    assert a.size == rec.size and np.array_equal(a, b) and (tmp_path / "off.wav").read_bytes() == (tmp_path / "live.wav").read_bytes()
    assert off["mean_support"] >= 1 and off["mean_squared_displacement"] > 0 and live["live_block"] == 256
    rev = cli.main(apply + ["--out", str(tmp_path / "rev.wav"), "--reverse", "--amount", "0.5"])
    c = D.load_audio_mono(str(tmp_path / "rev.wav"), SR)
    assert rev["reverse"] and c.size == rec.size and np.isfinite(c).all() and not np.array_equal(a, c)
    with pytest.raises(ValueError, match="--hop: hop 32: the transport was fitted at hop 16"):
        cli.main(["apply", "--config", str(ini), "--checkpoint", str(ck), "--hop", "32", "--transport", str(npz), "--in",
                  str(tmp_path / "in.wav"), "--out", str(tmp_path / "x.wav")])
    with pytest.raises(ValueError, match="--live-block 100: not a multiple of the hop 16"):
        cli.main(apply + ["--out", str(tmp_path / "x.wav"), "--live-block", "100"])
