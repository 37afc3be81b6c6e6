"""Latent restoration on the GPU (RV_SMOOTH_*, csrc/smooth.hip, rawaudiovae_kelsey_amd/smooth.py, restore.py) against
tests/smooth_oracle.py: the textbook filter and a Rauch-Tung-Striebel smoother in longdouble, another algorithm than
the kernels' Cholesky-Crout filter and Bryson-Frazier pass.

Gates (smooth_oracle.GATE_*): 8 x the largest error measured over every case below; state errors normalised by
max(1, ||y||_inf) of the sequence, nis by its value, logdet by sum_j |log eig_j(S)|.  The latent rows are held to
0.5 ulp32(|z|) + GATE_SMOOTHED (|c_l| + sum_j |R_jl| + |rho_l|).  Bit-for-bit: a sequence alone and in a batch, causality
of the filter, a sequence with no observation, NaN rows at missing frames, the guard bands, the splice where g is 0 or 1,
graph replay.  Each test prints the figures it asserts on."""
import functools
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import guarded as G  # noqa: E402
import smooth_oracle as O  # noqa: E402
import walk_oracle as WO  # noqa: E402

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if torch.is_tensor(a) else a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _smoother(k, L, diagonal, r):
    from rawaudiovae_kelsey_amd import smooth as SM, walk as W
    m = O.model(k, L, diagonal)
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64)).cuda()  # noqa: E731
    walk = W.LatentWalk(k, "diagonal" if diagonal else "full")._set(
        t(m["centre"]), t(m["V"]), t(m["lam"]), t(np.stack([m["A"].T, m["B"].T])), t(m["P"]), t(m["R"]), m["rank"], 300, 1)
    return SM.LatentSmoother(walk, r)


def _run(sm, x, rs, weight, mode=None):
    """FILTER and BACKWARD on guarded, wider-than-needed outputs -> (result [T, k + 2], state [T, k], out [T, L]) as
    numpy arrays, the guard bands and the gap columns checked."""
    T = x.shape[0]
    xd = torch.from_numpy(np.array(x)).cuda()
    wd = None if weight is None else torch.from_numpy(np.array(weight)).cuda()
    _, fields, held = sm.operands(xd, rs, wd)
    if mode is not None:
        from rawaudiovae_kelsey_amd import smooth as SM
        need = SM.workspace_bytes(T, sm.L, sm.k, mode)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        fields = dict(fields, mode=mode, ws=ws.data_ptr(), ws_bytes=need)
    res = G.guarded(T, sm.k + 2, sm.k + 5, torch.float64)
    out = G.guarded(T, sm.L, sm.L + 3, torch.float32)
    state = G.guarded_flat(T * sm.k, torch.float64)
    sm.run_filter(fields, res.view)
    sm.run_backward(fields, out.view, state.view)
    torch.cuda.synchronize()
    res.assert_untouched("result"), out.assert_untouched("out"), state.assert_untouched("state")
    return _np(res.payload()), _np(state.payload()).reshape(T, sm.k), _np(out.payload())


def _errors(c, res, state, k):
    """The four normalised errors of one batch against its oracle case."""
    obs = c["obs"]
    wp = float((np.abs(res[:, :k] - c["wp"]).max(1) / c["ynorm"]).max())
    wh = float((np.abs(state - c["wh"]).max(1) / c["ynorm"]).max())
    nis = logdet = 0.0
    if obs.any():
        nis = float((np.abs(res[obs, k] - c["nis"][obs]) / c["nis"][obs]).max()) if (c["nis"][obs] > 0).all() else np.inf
        logdet = float((np.abs(res[obs, k + 1] - c["logdet"][obs]) / c["logabs"][obs]).max())
    return wp, wh, nis, logdet


@pytest.mark.parametrize("mask", O.MASKS)
@pytest.mark.parametrize("r", O.NOISES)
@pytest.mark.parametrize("k,L,diagonal", O.SHAPES)
def test_filter_and_smoother_against_the_textbook_oracle(k, L, diagonal, r, mask):
    sm = _smoother(k, L, diagonal, r)
    worst = np.zeros(4)
    for lengths in O.LENGTHS:
        c = O.case(k, L, diagonal, lengths, mask, r)
        res, state, out = _run(sm, c["x"], c["row_start"], None if mask == "none" else c["weight"])
        obs, rs = c["obs"], c["row_start"]
        # NaN rows of x at missing frames leave every output finite
        assert np.isfinite(res).all() and np.isfinite(state).all() and np.isfinite(out).all(), (lengths, mask)
        assert (res[~obs, k] == -1).all() and (res[~obs, k + 1] == 0).all()
        worst = np.maximum(worst, _errors(c, res, state, k))
        # the latent rows
        z = c["z"].astype(np.float64)
        bound = 0.5 * np.spacing(np.abs(z).astype(np.float32)).astype(np.float64) + O.GATE_SMOOTHED * c["terms"].astype(np.float64)
        excess = float((np.abs(out.astype(np.float64) - z) / bound).max())
        assert excess <= 1.0, ("out", lengths, mask, excess)
        for a, b in zip(rs[:-1], rs[1:]):
            # nothing follows the last frame: its smoothed state is the filtered one, within the gate
            assert np.abs(state[b - 1] - res[b - 1, :k]).max() <= (O.GATE_SMOOTHED + O.GATE_FILTERED) * c["ynorm"][a]
            if not obs[a:b].any():                                   # no observation: the prior, exactly
                assert not state[a:b].any() and not res[a:b, :k].any()
                assert np.array_equal(_bits(out[a:b]), _bits(np.tile(c["model"]["centre"].astype(np.float32), (b - a, 1))))
    print("measured k %d L %d %s r %g %s: w+ %.3g  w-hat %.3g  nis %.3g  logdet %.3g" % (
        k, L, "diagonal" if diagonal else "dense", r, mask, *worst))
    assert (worst <= O.CEILING).all(), worst                             # above 1e-8 the kernel is defective
    assert worst[0] <= O.GATE_FILTERED and worst[1] <= O.GATE_SMOOTHED and worst[2] <= O.GATE_NIS and worst[3] <= O.GATE_LOGDET


@pytest.mark.parametrize("k,L,diagonal", [(17, 70, False), (64, 64, False), (70, 70, True)])
def test_a_sequence_has_the_same_bits_alone_and_in_a_batch_and_the_filter_is_causal(k, L, diagonal):
    sm = _smoother(k, L, diagonal, 1e-2)
    for mask in ("alternating", "weights", "gap30"):
        c = O.case(k, L, diagonal, (37, 1, 90), mask, 1e-2)
        rs = c["row_start"]
        res, state, out = _run(sm, c["x"], rs, c["weight"])
        for a, b in zip(rs[:-1], rs[1:]):
            r1, s1, o1 = _run(sm, c["x"][a:b], np.array([0, b - a]), c["weight"][a:b])
            assert np.array_equal(_bits(r1), _bits(res[a:b])) and np.array_equal(_bits(s1), _bits(state[a:b]))
            assert np.array_equal(_bits(o1), _bits(out[a:b]))
        # the same rows as one sequence fewer and shifted: where the sequence lies in x does not matter
        r2, s2, o2 = _run(sm, c["x"][37:], np.array([0, 1, 91]), c["weight"][37:])
        assert np.array_equal(_bits(r2), _bits(res[37:])) and np.array_equal(_bits(s2), _bits(state[37:]))
        assert np.array_equal(_bits(o2), _bits(out[37:]))
        # causality: w+[t] of the run cut at t + 1
        for t in (0, 1, 21, 88):
            rc, _, _ = _run(sm, c["x"][38:38 + t + 1], np.array([0, t + 1]), c["weight"][38:38 + t + 1])
            assert np.array_equal(_bits(rc[t]), _bits(res[38 + t])), (mask, t)


def test_dense_mode_on_a_diagonal_model_equals_diagonal_mode():
    from rawaudiovae_kelsey_amd import _lib
    sm = _smoother(17, 17, True, 1e-2)
    assert sm.mode == _lib.SMOOTH_DIAGONAL
    worst = np.zeros(4)
    for mask in ("none", "alternating", "gap30", "weights"):
        c = O.case(17, 17, True, (37, 1, 90), mask, 1e-2)
        diag = _run(sm, c["x"], c["row_start"], c["weight"])
        dense = _run(sm, c["x"], c["row_start"], c["weight"], mode=_lib.SMOOTH_DENSE)
        for got in (diag, dense):
            worst = np.maximum(worst, _errors(c, got[0], got[1], 17))
        obs = c["obs"]
        assert np.abs((dense[0][:, :17] - diag[0][:, :17]) / c["ynorm"][:, None]).max() <= 2 * O.GATE_FILTERED
        assert np.abs((dense[1] - diag[1]) / c["ynorm"][:, None]).max() <= 2 * O.GATE_SMOOTHED
        assert np.abs(dense[0][obs, 17] - diag[0][obs, 17]).max() <= 2 * O.GATE_NIS * np.abs(c["nis"][obs]).max()
        assert (np.abs(dense[0][obs, 18] - diag[0][obs, 18]) / c["logabs"][obs]).max() <= 2 * O.GATE_LOGDET
    print("measured dense on a diagonal model: w+ %.3g  w-hat %.3g  nis %.3g  logdet %.3g" % tuple(worst))
    assert worst[0] <= O.GATE_FILTERED and worst[1] <= O.GATE_SMOOTHED and worst[2] <= O.GATE_NIS and worst[3] <= O.GATE_LOGDET


@pytest.mark.parametrize("n,ranges,fade", [(300, [(100, 140)], 0), (300, [(0, 10), (200, 201)], 16), (300, [(290, 300)], 16),
                                             (300, [(0, 300)], 8), (300, [(100, 110), (120, 130)], 16), (1000, [(5, 6), (11, 12), (600, 700)], 4),
                                             (70000, [(0, 1), (65535, 65537), (69999, 70000)], 64)])
def test_splice_is_bit_exact_where_the_gain_is_0_or_1(n, ranges, fade):
    from rawaudiovae_kelsey_amd import _lib
    rng = np.random.default_rng(n + fade)
    src, frames = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    want, g = O.splice(src, frames, ranges, fade)
    out = G.guarded_flat(n, torch.float32)
    sd, fd = torch.from_numpy(src).cuda(), torch.from_numpy(frames).cuda()
    room = torch.from_numpy(np.asarray(ranges, np.int32)).cuda()
    _lib.mosaic_call(_lib.SMOOTH_SPLICE, src=sd.data_ptr(), frames=fd.data_ptr(), room=room.data_ptr(), n_rows=len(ranges),
                     width=fade, n_out=n, out=out.ptr)
    torch.cuda.synchronize()
    out.assert_untouched("out")
    got = _np(out.payload()).reshape(-1)
    assert np.array_equal(_bits(got[g == 0]), _bits(src[g == 0])) and np.array_equal(_bits(got[g == 1]), _bits(frames[g == 1]))
    ramp = (g > 0) & (g < 1)
    assert bool(ramp.any()) == (fade > 0 and ranges != [(0, n)])
    err = np.abs(got.astype(np.float64) - want)
    bound = 0.5 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 4 * WO.U * (np.abs(src) + np.abs(frames))
    print("splice n %d fade %d: %d ramp samples, worst error / bound %.3g" % (n, fade, ramp.sum(), (err / bound).max()))
    assert (err <= bound).all()
    # the library's wrapper gives the same bits
    from rawaudiovae_kelsey_amd import smooth as SM
    assert np.array_equal(_bits(SM.splice(sd, fd, ranges, fade)), _bits(got))


# ---- the tool --------------------------------------------------------------------------------------------------------

S, H, LAT, SR, HOP = 64, 32, 8, 8000, 16


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


def test_restore_end_to_end_and_restore_py(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import restore as cli
    from rawaudiovae_kelsey_amd import data as D, smooth as SM, walk as W
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    from rawaudiovae_kelsey_amd.mosaic import ola
    from rawaudiovae_kelsey_amd.stream import window_values
    model = _model()
    walk = W.fit_corpus(model, _waves(), HOP, 4)
    wave = _waves()[0].copy()
    wave[wave == 0] = 1e-3
    s, e, fade, context = 700, 792, 24, 8
    wave[s:e] = 0
    got = _np(SM.restore(model, walk, wave, [(s, e)], HOP, "hann", 1e-2, context, fade, fitted_hop=HOP))
    assert got.shape == wave.shape and got.dtype == np.float32 and np.isfinite(got).all()
    keep = np.ones(wave.size, bool)
    keep[s - fade:e + fade] = False
    assert np.array_equal(_bits(got[keep]), _bits(wave[keep]))                  # untouched outside [s - fade, e + fade)
    assert np.abs(got[s:e]).max() > 0                                           # the gap is filled
    # by hand: encode, smooth the region, decode, overlap-add, splice
    codec = FrameCodec(model)
    w = codec.wave(wave)
    padded, n_frames = codec.pad(w, w.numel(), HOP)
    mu, _ = codec.encode(padded, n_frames, HOP)
    mask = SM.frame_mask(wave.size, S, HOP, [(s, e)])
    assert np.array_equal(mask, O.frame_mask(wave.size, S, HOP, [(s, e)]))
    (f0, f1), = SM.regions(mask, context)
    weight = torch.from_numpy((~mask[f0:f1]).astype(np.float32)).cuda()
    z, _ = SM.LatentSmoother(walk, 1e-2).smooth(mu[f0:f1].contiguous(), [0, f1 - f0], weight)
    win = torch.from_numpy(window_values(S, "hann")).cuda()
    y = ola(codec.decode(z), HOP, (f1 - f0 - 1) * HOP + S, win)
    assert np.array_equal(_bits(got[s:e]), _bits(y[s - f0 * HOP:e - f0 * HOP]))
    full = torch.zeros_like(padded)
    full[f0 * HOP:f0 * HOP + y.numel()] = y
    assert np.array_equal(_bits(SM.splice(w, full[:w.numel()], [(s, e)], fade)), _bits(got))
    with pytest.raises(ValueError, match="context=5 frames is too short for segment_length 64, fade=24 and hop 16: it must be at least 6"):
        SM.restore(model, walk, wave, [(s, e)], HOP, "hann", 1e-2, 5, fade)
    with pytest.raises(ValueError, match="hop 32: the walk was fitted at hop 16"):
        SM.restore(model, walk, wave, [(s, e)], 32, None, 1e-2, context, fade, fitted_hop=HOP)
    with pytest.raises(ValueError, match=r"workspace for \d+ frames of 4 axes is \d+ bytes, more than max_workspace_bytes=1000: use a smaller context"):
        SM.restore(model, walk, wave, [(s, e)], HOP, "hann", 1e-2, context, fade, max_workspace_bytes=1000)
    # the surprise of the damaged take peaks in the damaged frames
    sur = _np(SM.surprise(model, walk, wave, HOP, 1e-2))
    assert sur.shape == (n_frames,) and np.isfinite(sur).all() and (sur >= 0).all()
    # restore.py: fill --detect-zeros finds the same span and writes the same samples; surprise writes its .npy
    ini = tmp_path / "m.ini"
    ini.write_text("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n" % (SR, S, H, LAT))
    ck, npz, wav = tmp_path / "ckpt", tmp_path / "walk.npz", tmp_path / "in.wav"
    torch.save({"epoch": 0, "state_dict": model.state_dict(), "optimizer": {}}, ck)
    W.write_walk(npz, walk, S, HOP)
    D.write_wav(wav, wave, SR)
    common = ["--config", str(ini), "--checkpoint", str(ck), "--walk", str(npz), "--in", str(wav), "--hop", str(HOP)]
    out, report = cli.main(["fill"] + common + ["--out", str(tmp_path / "out.wav"), "--window", "hann", "--detect-zeros", "64",
                                                "--context", str(context), "--fade", str(fade)])
    text = capsys.readouterr().out
    assert [g["samples"] for g in report] == [[s, e]] and report[0]["frames"] == [int(np.flatnonzero(mask)[0]), int(np.flatnonzero(mask)[-1]) + 1]
    assert "repaired 0.0875 s .. 0.0990 s (samples 700 .. 792, frames %d .. %d)" % tuple(report[0]["frames"]) in text
    assert np.array_equal(_bits(out), _bits(got))
    assert np.array_equal(_bits(D.load_audio_mono(tmp_path / "out.wav", SR)), _bits(got))
    by_gaps, _ = cli.main(["fill"] + common + ["--out", str(tmp_path / "out2.wav"), "--window", "hann",
                                               "--gaps", "%r:%r" % (s / SR, e / SR), "--context", str(context), "--fade", str(fade)])
    assert np.array_equal(_bits(by_gaps), _bits(got))
    sur_cli = cli.main(["surprise"] + common + ["--out", str(tmp_path / "surprise.npy"), "--threshold", "4"])
    assert np.array_equal(_bits(np.load(tmp_path / "surprise.npy")), _bits(sur)) and np.array_equal(_bits(sur_cli), _bits(sur))
    assert "wrote %s: %d frames" % (tmp_path / "surprise.npy", n_frames) in capsys.readouterr().out
    smoothed = cli.main(["smooth"] + common + ["--out", str(tmp_path / "smooth.wav"), "--window", "hann", "--noise", "0.5"])
    assert smoothed.shape == wave.shape and np.isfinite(smoothed).all() and (tmp_path / "smooth.wav").exists()
    with pytest.raises(ValueError, match="--hop: hop 32: the walk was fitted at hop 16"):
        cli.main(["fill", "--config", str(ini), "--checkpoint", str(ck), "--walk", str(npz), "--in", str(wav), "--hop", "32",
                  "--out", str(tmp_path / "x.wav"), "--gaps", "0.01:0.02"])
    with pytest.raises(ValueError, match="--context 2 / --fade 24 / --window hann: context=2 frames is too short"):
        cli.main(["fill"] + common + ["--out", str(tmp_path / "x.wav"), "--window", "hann", "--detect-zeros", "64",
                                      "--context", "2", "--fade", "24"])


@pytest.mark.parametrize("k,L,diagonal", [(17, 70, False), (70, 70, True)])
def test_graph_replay_of_filter_then_backward_gives_the_eager_bits(k, L, diagonal):
    from rawaudiovae_kelsey_amd.engine import Graph
    sm = _smoother(k, L, diagonal, 1e-2)
    c = O.case(k, L, diagonal, (37, 1, 90), "gap30", 1e-2)
    T = c["x"].shape[0]
    eager = _run(sm, c["x"], c["row_start"], c["weight"])
    xd, wd = torch.from_numpy(np.array(c["x"])).cuda(), torch.from_numpy(np.array(c["weight"])).cuda()
    _, fields, held = sm.operands(xd, c["row_start"], wd)
    res = torch.full((T, k + 2), 7.0, dtype=torch.float64, device="cuda")
    state = torch.full((T, k), 7.0, dtype=torch.float64, device="cuda")
    out = torch.full((T, L), 7.0, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = Graph(side)
    with g:
        sm.run_filter(fields, res, side.cuda_stream)
        sm.run_backward(fields, out, state, side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        res.fill_(7.0), state.fill_(7.0), out.fill_(7.0)
        g.launch(torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert np.array_equal(_bits(res), _bits(eager[0])) and np.array_equal(_bits(state), _bits(eager[1]))
        assert np.array_equal(_bits(out), _bits(eager[2]))
