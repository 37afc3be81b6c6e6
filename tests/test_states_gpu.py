"""Latent states on the GPU (RV_HMM_*, csrc/hmm.hip, rawaudiovae_kelsey_amd/states.py, states.py) against
tests/states_oracle.py.

Bit for bit, inputs between NaN guards and outputs between sentinel guards (tests/guarded.py), x with a row pitch of
L + 3: EMIT against the float64 oracle given the same theta; VITERBI's path and score on small-integer logb with -inf in
log A; the moments N, M1 and M2 of MSTEP at the range edge and at the tile's edges, and what MSTEP derives from them by
sums and divisions alone (m, w, pi, A, info); a sequence alone and inside a batch; an unobserved frame among observed ones.

Gated against the longdouble oracle (exp and log on the device are not numpy's): gamma relative to 1, xi relative to the
sequence's pairs, ll relative to sum_t |log c_t + M_t|, g relative to k log(2 pi) + sum_j |log v_sj|, log pi and log A
relative to max(1, |.|).  Each gate is 4 x the distance of the float64 oracle from the longdouble one at these shapes
(states_oracle.GATE_*, measured by tests/test_states_cpu.py).  Each test prints the distances it measures.

End to end: 20 EM iterations on planted data recover the planted states, the log-likelihood never drops by more than
its gate, and the parameters stay within the gates, times the iterations, of the oracle's own fit."""
import functools
import json
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import guarded as G  # noqa: E402
import states_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

STATES = (1, 2, 16, 17, 63, 64)
EMIT_SHAPES = ((1, 1), (3, 7), (64, 64), (64, 70), (64, 512), (1, 257))
EMIT_FRAMES = (1, 2, 255, 256, 257, O.EMIT_FRAMES + 1)
VITERBI_LENGTHS = (5, 0, 1, 257, 2, 3, 0)      # the sequence of 3 frames holds a frame every state is -inf at


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
    g = G.guarded_flat(a.size, torch.float64, a.reshape(-1))
    return g.view.view(a.shape)


def _out(shape, dtype=torch.float64, fill=G.SENTINEL):
    n = int(np.prod(shape))
    g = G.guarded_flat(n, dtype, fill)
    return g, g.view.view(shape)


def _rows(x, pad=3):
    """x [T, L] fp32 with a row pitch of L + pad, NaN in the gaps and guards"""
    return G.guarded(x.shape[0], x.shape[1], x.shape[1] + pad, torch.float32, x).view


def _seqs(rs):
    return torch.from_numpy(np.array(rs, np.int64)).cuda(), len(rs) - 1     # a copy: the oracle's arrays are read-only


@pytest.mark.parametrize("k,L", EMIT_SHAPES)
def test_emit_equals_the_oracle_bit_for_bit(k, L):
    from rawaudiovae_kelsey_amd import states as ST
    c, P = O.basis(k, L)
    cd, Pd = _in64(c), _in64(P)
    for T in EMIT_FRAMES:
        x = O.latents(T, L)
        xd = _rows(x)
        for S in STATES:
            th = O.random_theta(S, k)
            g, logb = _out((T, S))
            ST.emit(xd, cd, Pd, _in64(th), S, out=logb)
            torch.cuda.synchronize()
            g.assert_untouched("logb")
            _same(logb, O.emit(x, c, P, th, S, k), "logb k %d L %d T %d S %d" % (k, L, T, S))


def test_an_unobserved_frame_is_a_row_of_nan_and_changes_no_other_row():
    from rawaudiovae_kelsey_amd import states as ST
    k, L, S, T = 3, 7, 17, 130
    c, P = O.basis(k, L)
    th = O.random_theta(S, k)
    x = O.latents(T, L)
    clean = _np(ST.emit(_rows(x), _in64(c), _in64(P), _in64(th), S))
    holes = x.copy()
    holes[0, 2], holes[63, 6], holes[64], holes[129, 0] = np.nan, np.inf, np.nan, -np.inf
    got = _np(ST.emit(_rows(holes), _in64(c), _in64(P), _in64(th), S))
    gone = np.zeros(T, bool)
    gone[[0, 63, 64, 129]] = True
    assert np.isnan(got[gone]).all() and np.isfinite(clean).all()
    _same(got[~gone], clean[~gone], "the observed rows")
    _same(got, O.emit(holes, c, P, th, S, k), "logb with holes")


def _viterbi_case(S):
    """small-integer logb (ties abound), a log A with -inf entries, a sequence with a frame no state reaches, NaN in the
    parts of theta the op has no business reading"""
    rng = np.random.default_rng(100 + S)
    rs = O.starts(VITERBI_LENGTHS)
    T = int(rs[-1])
    logb = rng.integers(-3, 4, (T, S)).astype(np.float64)
    logb[rs[5] + 1] = -np.inf
    logb[rs[3] + 100] = np.nan                                  # an unobserved frame inside the long sequence
    o = O.layout(S, 2)
    th = np.full(o["doubles"], np.nan)
    th[o["logpi"]] = rng.integers(-2, 3, S)
    la = rng.integers(-2, 3, (S, S)).astype(np.float64)
    la[rng.uniform(size=(S, S)) < 0.4] = -np.inf
    th[o["logA"]] = la.ravel()
    return logb, rs, th


@pytest.mark.parametrize("S", STATES)
def test_viterbi_path_and_score_are_exact(S):
    from rawaudiovae_kelsey_amd import states as ST
    logb, rs, th = _viterbi_case(S)
    T = logb.shape[0]
    gp, path = _out((T,), torch.int32, G.INT_FILL)
    gs, score = _out((len(rs) - 1,))
    ST.viterbi(_in64(logb), _seqs(rs), _in64(th), S, 2, out=(path, score))
    torch.cuda.synchronize()
    gp.assert_untouched("path"), gs.assert_untouched("score")
    want_path, want_score = O.viterbi(logb, rs, th, S, 2)
    assert np.array_equal(_np(path), want_path), np.flatnonzero(_np(path) != want_path)[:8]
    _same(score, want_score, "score S %d" % S)
    assert (want_path[rs[5]:rs[6]] == -1).all() and want_score[5] == -np.inf and want_score[1] == 0
    assert S == 1 or len(set(want_path[rs[3]:rs[4]].tolist())) > 1


def _mstep(S, k, T, floor=1e-3, lengths=None, L=None):
    """RV_HMM_MSTEP at O.mstep_case between guards -> (theta', info, moments) as numpy arrays and the oracle's result"""
    from rawaudiovae_kelsey_amd import states as ST
    x, c, P, gamma, xi, rs, th = O.mstep_case(S, k, T, lengths, L)
    n_theta = O.layout(S, k)["doubles"]
    gt, new = _out((n_theta + S * (1 + 2 * k),))
    gi, info = _out((S,), torch.int32, G.INT_FILL)
    block = np.concatenate([gamma.ravel(), xi.ravel(), np.full(len(rs) - 1, np.nan)])       # ll is not the M-step's business
    new, info, mom = ST.mstep(_rows(x), _in64(c), _in64(P), _in64(block), _seqs(rs), _in64(th), S, floor, out=(new, info),
                              moments=True)
    torch.cuda.synchronize()
    gt.assert_untouched("theta and moments"), gi.assert_untouched("info")
    lean, _, none = ST.mstep(_rows(x), _in64(c), _in64(P), _in64(block), _seqs(rs), _in64(th), S, floor)
    assert none is None
    _same(lean, new, "theta without the moments")
    return _np(new), _np(info), _np(mom), O.mstep(x, c, P, gamma, xi, rs, th, S, k, floor), th


def _check_mstep(S, k, T, floor=1e-3, lengths=None, L=None):
    new, info, mom, res, old = _mstep(S, k, T, floor, lengths, L)
    what = "S %d k %d T %d" % (S, k, T)
    _same(mom[:, 0], res["N"], "N " + what)
    _same(mom[:, 1:1 + k], res["M1"], "M1 " + what)
    _same(mom[:, 1 + k:], res["M2"], "M2 " + what)
    assert np.array_equal(info, res["info"])
    o = O.layout(S, k)
    for part in ("m", "w", "pi", "A"):
        _same(new[o[part]], res["theta"][o[part]], part + " " + what)
    dg, dpi, da = O.mstep_distances(new, res, S, k)
    print("measured %s: dead %d, g %.3g log pi %.3g log A %.3g" % (what, info.sum(), dg, dpi, da))
    assert dg <= O.GATE_G and dpi <= O.GATE_LOG_A and da <= O.GATE_LOG_A
    dead = info == 1
    got, was = O.unpack(new, S, k), O.unpack(old, S, k)
    for part in ("m", "w", "g"):                                # a dead state keeps its emission, bit for bit
        _same(got[part][dead], was[part][dead], "dead " + part)
    return got, was, res, dead


@pytest.mark.parametrize("T", (1, 4095, 4096, 4097, 8193))
def test_mstep_moments_at_the_range_edge(T):
    got, was, res, dead = _check_mstep(3, 3, T, lengths=(T - T // 2, 0, T // 2))
    assert dead.all() if T == 1 else not dead[0]


@pytest.mark.parametrize("S,k", ((64, 64), (17, 33)))
def test_mstep_moments_at_the_tile_edges(S, k):
    got, was, res, dead = _check_mstep(S, k, 300)
    assert dead.any() and not dead.all()
    _same(got["A"][S - 1], was["A"][S - 1], "the row of A without mass")
    assert np.isneginf(got["logA"]).any() and np.isneginf(got["logpi"]).sum() == 0


def test_mstep_moments_of_the_widest_latents():
    got, was, res, dead = _check_mstep(17, 33, 300, L=512)
    assert dead.any() and not dead.all()


def test_mstep_takes_the_variance_floor():
    S, k = 3, 3
    got, was, res, dead = _check_mstep(S, k, 300, floor=50.0)
    live = ~dead
    assert live.any() and (1 / res["v"][live] == 1 / 50.0).all() and (got["w"][live] == 1 / 50.0).all()
    got, was, res, dead = _check_mstep(S, k, 300, floor=1e-3)
    assert (res["v"][~dead] > 1e-3).all()


def _forward_backward(logb, rs, th, S, k):
    from rawaudiovae_kelsey_amd import states as ST
    T, n = logb.shape[0], len(rs) - 1
    g, block = _out((ST.posteriors_size(T, S, n),))
    ST.forward_backward(_in64(logb), _seqs(rs), _in64(th), S, k, out=block)
    torch.cuda.synchronize()
    g.assert_untouched("the posteriors")
    return tuple(_np(t) for t in ST.split_posteriors(block, T, S, n))


@pytest.mark.parametrize("outlier", (False, True))
@pytest.mark.parametrize("S", O.GATED_STATES)
def test_forward_backward_within_the_gates_of_the_longdouble_oracle(S, outlier):
    logb, rs, th, k = O.gated_case(S, outlier)
    got = _forward_backward(logb, rs, th, S, k)
    dg, dx, dl = O.gated_distances(got, S, outlier)
    print("measured S %d outlier %d: gamma %.3g xi %.3g ll %.3g" % (S, outlier, dg, dx, dl))
    assert dg <= O.GATE_GAMMA and dx <= O.GATE_XI and dl <= O.GATE_LL
    assert not got[1][0].any() and got[1][1].sum() > 0.999                 # one frame: no pair; two frames: one


def test_a_sequence_alone_and_inside_a_batch_has_the_same_bits():
    from rawaudiovae_kelsey_amd import states as ST
    S = 17
    logb, rs, th, k = O.gated_case(S, True)
    gamma, xi, ll = _forward_backward(logb, rs, th, S, k)
    thv = np.array(th)
    o = O.layout(S, k)
    with np.errstate(divide="ignore"):
        thv[o["logA"]] = np.where(np.arange(S * S) % 5 == 0, -np.inf, thv[o["logA"]])
    path, score = (_np(t) for t in ST.viterbi(_in64(logb), _seqs(rs), _in64(thv), S, k))
    a, b = int(rs[2]), int(rs[3])
    for lead in (0, 7):                                                    # alone; behind an empty and a short sequence
        part = np.concatenate([logb[:lead], logb[a:b]])
        prs = [0, b - a] if lead == 0 else [0, 0, lead, lead + b - a]
        g1, x1, l1 = _forward_backward(part, prs, th, S, k)
        _same(g1[lead:], gamma[a:b], "gamma"), _same(x1[-1], xi[2], "xi"), _same(l1[-1:], ll[2:3], "ll")
        p1, s1 = (_np(t) for t in ST.viterbi(_in64(part), _seqs(prs), _in64(thv), S, k))
        assert np.array_equal(p1[lead:], path[a:b])
        _same(s1[-1:], score[2:3], "score")


def test_graph_replay_of_one_em_iteration_and_viterbi_gives_the_eager_bits():
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd.engine import Graph
    S, k = 17, 33
    x, c, P, _, _, rs, th = O.mstep_case(S, k)
    T, n = x.shape[0], len(rs) - 1
    xd, cd, Pd, thd, seqs = _rows(x), _in64(c), _in64(P), _in64(th), _seqs(rs)
    ws = ST.workspace(T, S, k, xd.device)

    def outputs():
        f64 = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device="cuda")  # noqa: E731
        i32 = lambda m: torch.full((m,), -77, dtype=torch.int32, device="cuda")  # noqa: E731
        return [f64(T, S), f64(ST.posteriors_size(T, S, n)), f64(thd.numel()), i32(S), i32(T), f64(n)]

    def iteration(o):
        ST.emit(xd, cd, Pd, thd, S, out=o[0])
        ST.forward_backward(o[0], seqs, thd, S, k, out=o[1], ws=ws)
        ST.mstep(xd, cd, Pd, o[1], seqs, thd, S, 1e-3, out=(o[2], o[3]), ws=ws)
        ST.viterbi(o[0], seqs, o[2], S, k, out=(o[4], o[5]), ws=ws)

    eager = outputs()
    iteration(eager)
    torch.cuda.synchronize()
    held = outputs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = Graph(side)
    with torch.cuda.stream(side):          # the ops launch on the current stream
        with g:
            iteration(held)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for t, fresh in zip(held, outputs()):
            t.copy_(fresh)
        g.launch(torch.cuda.current_stream())
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(held, eager)):
            _same(a, b, "output %d" % i)
    assert np.isnan(_np(eager[0])).any() and (_np(eager[4]) != -77).all()      # an unobserved frame; every frame labelled


@functools.lru_cache(maxsize=None)
def _planted_fit():
    from rawaudiovae_kelsey_amd import states as ST
    x, rs, labels, c, P = O.planted()
    S, k, iters = O.PLANT["S"], O.PLANT["k"], O.PLANT["iters"]
    st = ST.LatentStates(S, k)
    xd = torch.from_numpy(np.array(x)).cuda()
    hist = st.fit(xd, rs, (torch.from_numpy(np.array(c)).cuda(), torch.from_numpy(np.array(P)).cuda()), iters, 0, O.PLANT_SEED)
    return st, xd, hist


def test_fit_recovers_planted_states_and_follows_the_oracles_fit():
    st, xd, hist = _planted_fit()
    x, rs, labels, c, P = O.planted()
    S, k, iters = O.PLANT["S"], O.PLANT["k"], O.PLANT["iters"]
    want, want_hist, scales = O.planted_fit()
    assert len(hist) == iters == st.n_iter_
    step = np.diff(hist) / scales[1:]
    path, score = st.label(xd, rs)
    agree = O.agreement(_np(path), labels, S)
    print("measured: ll %.6f -> %.6f, least step %.3g of its scale, agreement %.4f" % (hist[0], hist[-1], step.min(), agree))
    assert (step >= -O.GATE_LL).all() and agree >= 0.99
    got, ref = O.unpack(_np(st.theta_), S, k), O.unpack(want, S, k)
    worst = {p: float((np.abs(got[p] - ref[p]) / np.maximum(1, np.abs(ref[p]))).max()) for p in ("m", "w", "pi", "A", "g")}
    print("measured after %d iterations, relative to max(1, |.|): %s" % (iters, " ".join("%s %.3g" % kv for kv in worst.items())))
    assert max(worst["m"], worst["w"], worst["pi"]) <= iters * O.GATE_GAMMA and worst["A"] <= iters * O.GATE_XI
    assert worst["g"] <= iters * max(O.GATE_GAMMA, O.GATE_G)
    assert not _np(st.info_).any() and ((st.durations_ > 10) & (st.durations_ < 40)).all()      # planted: 20 frames
    # the other faces of the model agree with one another
    gamma = _np(st.posteriors(xd, rs))
    assert np.mean(gamma.argmax(axis=1) == _np(path)) > 0.99
    ll = _np(st.loglik(xd, rs))
    assert ll.shape == (3,) and (_np(score) <= ll).all() and ll.sum() >= hist[-1] - 1e-6


def test_states_py_fit_label_score_and_segment_py_split(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import segment
    import states as cli
    import test_walk_gpu as TW
    from rawaudiovae_kelsey_amd import data as D
    (tmp_path / "audio").mkdir()
    for i, w in enumerate(TW._waves()):
        D.write_wav(tmp_path / "audio" / ("%d.wav" % i), w, TW.SR)
    ini = tmp_path / "m.ini"
    ini.write_text("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n"
                   % (TW.SR, TW.S, TW.H, TW.LAT))
    ck = tmp_path / "ckpt"
    torch.save({"epoch": 0, "state_dict": TW._model().state_dict(), "optimizer": {}}, ck)
    common = ["--config", str(ini), "--checkpoint", str(ck), "--hop", "16"]
    npz = tmp_path / "states.npz"
    rep = cli.main(["fit"] + common + ["--data", str(tmp_path / "audio"), "--states", "3", "--keep", "4", "--iters", "8",
                                       "--out", str(npz)])
    out = capsys.readouterr().out.strip().splitlines()
    assert json.loads(out[-1]) == rep and out[0].startswith("%d iterations, log-likelihood per frame" % rep["iterations"])
    assert [ln.split(":")[0] for ln in out[1:4]] == ["state A", "state B", "state C"]
    assert rep["n_files"] == 2 and rep["states"] == 3 and rep["keep"] == 4 and 1 <= rep["iterations"] <= 8
    assert abs(sum(rep["occupancy"]) - 1) < 1e-9 and all(d >= 1 for d in rep["duration"])
    wav = str(tmp_path / "audio" / "0.wav")
    seg = tmp_path / "segments.json"
    lab = cli.main(["label"] + common + ["--states", str(npz), "--in", wav, "--out", str(seg)])
    assert json.loads(seg.read_text()) == lab and set(lab["labels"]) <= {0, 1, 2} and lab["states"] == 3
    assert lab["frames"] == sum(np.diff([0] + lab["boundary_frames"] + [lab["frames"]])) and lab["hop"] == 16
    names = segment.main(["split", "--segments", str(seg), "--in", wav, "--out-dir", str(tmp_path / "cut")])
    assert len(names) == lab["segments"]
    assert np.array_equal(np.concatenate([D.load_audio_mono(n, TW.SR) for n in names]), D.load_audio_mono(wav, TW.SR))
    capsys.readouterr()
    sc = cli.main(["score"] + common + ["--states", str(npz), "--in", wav])
    out = capsys.readouterr().out.strip().splitlines()
    assert json.loads(out[-1]) == sc and sc["frames"] == lab["frames"] and np.isfinite(sc["loglik_per_frame"])
    assert abs(sum(sc["occupancy"]) - 1) < 1e-9 and lab["score"] <= sc["loglik"]
    with pytest.raises(ValueError, match="--hop: hop 32: the states were fitted at hop 16"):
        cli.main(["score", "--config", str(ini), "--checkpoint", str(ck), "--hop", "32", "--states", str(npz), "--in", wav])
    with pytest.raises(ValueError, match="--states 9 / --keep 4: 4 frames are fewer than the 9 states"):
        short = tmp_path / "short.wav"
        D.write_wav(short, TW._waves()[0][:TW.S + 16 * 3], TW.SR)
        cli.main(["fit"] + common + ["--data", str(short), "--states", "9", "--keep", "4", "--out", str(npz)])
