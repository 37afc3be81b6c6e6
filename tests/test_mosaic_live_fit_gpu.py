"""Live grain fitting on the GPU (RV_MOSAIC_LIVE / LIVE_DRAIN with a fit in csrc/mosaic_live.hip and csrc/grain.hip,
StreamingMosaic(fit=R, gain_max=g), mosaic.py --live-fit / --live-gain-max).  Everything is compared bit for bit: the
audio and the gains as int32 views, the scores as int64 views.  Without unit selection and at lag 0 the reference is
the offline mosaic of the zero-prefixed input; with a lag, drains and resets it is tests/live_fit_oracle.py on the
device's own candidates."""
import csv
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from conftest import REPO  # noqa: E402
import live_fit_oracle as LF  # noqa: E402
from guarded import guarded_flat  # noqa: E402

S, HOP = 64, 16
FITS = [(5, 0.0), (0, 4.0), (16, 4.0), (70, 2.0)]


def _M():
    from rawaudiovae_kelsey_amd import mosaic
    return mosaic


def _model(S=64, H=96, L=8, seed=0):
    from rawvae.model import VAE
    torch.manual_seed(seed)
    return VAE(S, H, L).cuda().eval()


def _waves(rng, lengths, sr=8000.0):
    out = []
    for i, n in enumerate(lengths):
        t = np.arange(n) / sr
        w = 0.6 * np.sin(2 * np.pi * (150 + 170 * i) * t) + 0.2 * rng.standard_normal(n)
        w[: n // 5] = 0                                          # leading silence: duplicate all-zero frames
        out.append(w.astype(np.float32))
    return out


def _index(model, hop, lengths=(700, 1000, 513, 1290), seed=9):
    index = _M().LatentIndex(model, hop=hop)
    for i, w in enumerate(_waves(np.random.default_rng(seed), lengths)):
        index.add(w, "f%d" % i)
    return index


def _signal(rng, n_streams, n):
    t = np.arange(n)
    x = np.stack([0.5 * np.sin(t * (0.05 + 0.03 * s)) for s in range(n_streams)]) + 0.1 * rng.standard_normal(
        (n_streams, n))
    x[:, n // 2:n // 2 + 40] = 0                                 # a silent stretch: target frames of zero energy
    return torch.from_numpy(x.astype(np.float32)).cuda()


@pytest.fixture(scope="module")
def index():
    return _index(_model(seed=5), HOP)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _run(sm, x, calls=None, replay=False, before_call=None):
    """`calls`: 'p' = the next block of x through process, 'd' = drain; None: every block of x, then drain_blocks drains
    -> dict of y [ns, len(calls) * block], idx / dist [ns, T, k] of the frames fed, choice [ns, n_out], the fits
    shift / gain / score [ns, n_out, kf] (as emitted, call after call), calls."""
    if calls is None:
        calls = "p" * (x.shape[1] // sm.block) + "d" * (sm.drain_blocks if sm.lag else 0)
    out = dict(y=[], idx=[], dist=[], choice=[], shift=[], gain=[], score=[])
    b = 0
    for n, c in enumerate(calls):
        if before_call is not None:
            before_call(n)
        if c == "p":
            xb = x[:, b * sm.block:(b + 1) * sm.block]
            b += 1
            out["y"].append((sm.replay(xb) if replay else sm.process(xb)).clone())
            i, d, _ = sm.last_matches()
            out["idx"].append(i.clone()), out["dist"].append(d.clone())
        else:
            out["y"].append((sm.drain_replay() if replay else sm.drain()).clone())
        out["choice"].append(sm.last_matches()[2].clone())
        if sm.last_fit() is not None:
            for name, t in zip(("shift", "gain", "score"), sm.last_fit()):
                out[name].append(t.clone())
    res = {k: torch.cat(v, 1) for k, v in out.items() if v}
    res["calls"] = calls
    return res


def _same(a, b, keys=("y", "idx", "dist", "choice", "shift", "gain", "score")):
    for k in keys:
        assert (k in a) == (k in b), k
        if k in a:
            assert _eq(a[k], b[k]), (k, torch.nonzero(_bits(a[k]) != _bits(b[k]))[:5].tolist())


def _against_offline(index, x, block, k, window, R, g, continuity=0.0, hop=HOP):
    """equalities 1 and 2: the live outputs and fits of every stream are the offline call's on cat([zeros, x])"""
    M = _M()
    ns, n = x.shape
    sm = M.StreamingMosaic(index, ns, block, hop=hop, k=k, mode="grains", window=window, continuity=continuity, fit=R,
                           gain_max=g)
    assert (sm.fit, sm.gain_max, sm.lag) == (R, g, 0)
    got = _run(sm, x)
    kf = k if continuity == 0 else 1
    assert got["shift"].shape == (ns, n // hop, kf) and got["shift"].dtype == torch.int32
    assert got["gain"].dtype == torch.float32 and got["score"].dtype == torch.float64
    for s in range(ns):
        target = torch.cat([torch.zeros(sm.latency, device="cuda"), x[s]])
        ref = index.mosaic(target, k=k, hop=hop, mode="grains", window=window, return_matches=True,
                           continuity=continuity, return_path=True, fit=R, gain_max=g, return_fit=True)
        y, idx, dist, path, fits = ref
        assert _eq(got["idx"][s], idx) and _eq(got["dist"][s], dist)
        if continuity > 0:
            assert torch.equal(got["choice"][s], path[1])
        else:
            assert torch.all(got["choice"][s] == -1)
        for name, want in zip(("shift", "gain", "score"), fits):
            bad = torch.nonzero(_bits(got[name][s]) != _bits(want))
            assert bad.numel() == 0, (name, s, block, k, bad[:5].tolist())
        bad = torch.nonzero(_bits(got["y"][s]) != _bits(y[:n]))
        assert bad.numel() == 0, (s, block, k, bad[:5].flatten().tolist(), float((got["y"][s] - y[:n]).abs().max()))
    return got


@pytest.mark.parametrize("R,g", FITS)
@pytest.mark.parametrize("window", [None, "hann"])
def test_without_selection_live_equals_the_offline_fitted_mosaic(index, window, R, g):
    """12 blocks of 64, 24 of 32, 48 of 16 samples: the ring of P + block = 112, 80, 64 floats wraps many times"""
    x = _signal(np.random.default_rng(R + 1), 3, 64 * 12)
    moved = scaled = 0
    for k in (1, 4):
        for block in (16, 32, 64):
            for ns in (1, 3):
                got = _against_offline(index, x[:ns], block, k, window, R, g)
                moved += int((got["shift"] != 0).sum())
                scaled += int(((got["gain"] != 1) & (got["gain"] != 0)).sum())
    assert (moved > 0) == (R > 0) and (scaled > 0) == (g > 0)


@pytest.mark.parametrize("R,g", [(16, 4.0), (70, 0.0)])
def test_k1_with_selection_at_lag_zero_equals_the_offline_fitted_mosaic(index, R, g):
    x = _signal(np.random.default_rng(3), 2, 64 * 12)
    for block in (16, 64):
        _against_offline(index, x, block, 1, "hann", R, g, continuity=0.5)


def _oracle_check(index, sm, x, got, weight_at, window):
    """choices, fits and audio of every stream against live_fit_oracle on the device's own candidates"""
    from rawaudiovae_kelsey_amd.stream import window_values
    w = None if window is None else window_values(sm.S, window)
    audio, mu = index.audio.cpu().numpy(), index.mu.cpu().numpy()
    played = 0
    for s in range(x.shape[0]):
        r = LF.run(x[s].cpu().numpy(), got["calls"], sm.block, sm.S, sm.hop, got["idx"][s].cpu().numpy(),
                   got["dist"][s].cpu().numpy(), audio, index.row_start, index.room, sm.fit, sm.gain_max, w, mu,
                   index.successor(sm.hop // index.step), lambda c: weight_at(c)[s], sm.lag)
        assert np.array_equal(got["choice"][s].cpu().numpy(), r["choice"]), (s, "choice")
        assert np.array_equal(got["shift"][s, :, 0].cpu().numpy(), r["shift"][:, 0]), (s, "shift")
        assert np.array_equal(got["gain"][s, :, 0].cpu().numpy().view(np.int32), r["gain"][:, 0].view(np.int32)), (s, "gain")
        assert np.array_equal(got["score"][s, :, 0].cpu().numpy().view(np.int64), r["score"][:, 0].view(np.int64)), (s, "score")
        y = got["y"][s].cpu().numpy()
        bad = np.argwhere(y.view(np.int32) != r["y"].view(np.int32))
        assert bad.size == 0, (s, bad[:5].ravel().tolist(), float(np.abs(y - r["y"]).max()))
        played += int((r["choice"] >= 0).sum())
        none = r["choice"] < 0
        assert np.all(r["shift"][none] == 0) and np.all(r["gain"][none] == 0) and np.all(r["score"][none] == 0)
    return played


@pytest.mark.parametrize("lag,calls,n_blocks", [(1, None, 6), (3, None, 6), (3, "ppdppdd", 4), (5, None, 2), (0, None, 6)])
def test_with_a_lag_every_committed_frame_is_fitted_to_the_frame_it_arrived_with(index, lag, calls, n_blocks):
    M = _M()
    block, k, R, g = 32, 4, 16, 4.0
    sm = M.StreamingMosaic(index, 2, block, hop=HOP, k=k, mode="grains", window="hann", continuity=0.5, lag=lag, fit=R,
                           gain_max=g)
    x = _signal(np.random.default_rng(10 + lag), 2, n_blocks * block)

    def weight_at(call):                                         # a weight change between calls
        return (0.5, 0.5) if call < 3 else (3.0, 0.0)

    def before(call):
        sm.weight.copy_(torch.tensor(weight_at(call), device="cuda"))

    got = _run(sm, x, calls=calls, before_call=before)
    if lag == 5:
        assert got["calls"] == "pp" + "d" * 4 and torch.all(got["choice"][:, :4] == -1)   # more lag than frames fed
    played = _oracle_check(index, sm, x, got, weight_at, "hann")
    assert played == 2 * n_blocks * (block // HOP)              # every frame fed was played
    assert int((got["shift"] != 0).sum()) > 0 and float(got["y"].abs().max()) > 0


def test_reset_of_one_stream_restarts_its_target_history_only(index):
    M = _M()
    kw = dict(hop=HOP, k=4, mode="grains", window="hann", continuity=0.4, lag=3, fit=16, gain_max=4.0)
    x = _signal(np.random.default_rng(21), 3, 32 * 6)
    sm = M.StreamingMosaic(index, 3, 32, **kw)
    whole = _run(sm, x)
    calls = whole["calls"]
    sm = M.StreamingMosaic(index, 3, 32, **kw)
    first = _run(sm, x[:, :96], calls="ppp")
    sm.reset(1)
    second = _run(sm, x[:, 96:], calls=calls[3:])
    for s in (0, 2):                                             # the other streams' bits are unchanged
        for key in ("y", "choice", "shift", "gain", "score"):
            assert _eq(torch.cat([first[key][s], second[key][s]]), whole[key][s]), (s, key)
    # stream 1 from the reset on: the oracle restarted, i.e. a zero-prefixed history and no pending rows
    one = {k: (v[1:2] if torch.is_tensor(v) else v) for k, v in second.items()}
    _oracle_check(index, sm, x[1:2, 96:], one, lambda c: (0.4,), "hann")
    fresh = _run(M.StreamingMosaic(index, 1, 32, **kw), x[1:2, 96:], calls=calls[3:])
    _same(one, fresh)
    assert torch.all(second["choice"][1, :3] == -1) and torch.all(second["choice"][0, :3] >= 0)
    assert not _eq(second["y"][1], whole["y"][1, 96:])
    sm.reset()
    _same(_run(sm, x), whole)


def test_graph_replay_and_drain_replay_give_the_eager_bits(index):
    M = _M()
    kw = dict(hop=HOP, k=4, mode="grains", window="hann", continuity=0.5, lag=2, fit=16, gain_max=4.0)
    x = _signal(np.random.default_rng(22), 2, 32 * 8)
    eager, graph = M.StreamingMosaic(index, 2, 32, **kw), M.StreamingMosaic(index, 2, 32, **kw)
    graph.capture()
    graph.reset()
    calls = "pppdppddpppdd"
    a, b = _run(eager, x, calls=calls), _run(graph, x, calls=calls, replay=True)
    _same(a, b)
    _oracle_check(index, graph, x, b, lambda c: (0.5, 0.5), "hann")
    plain, cap = M.StreamingMosaic(index, 2, 32, hop=HOP, k=4, fit=5, gain_max=2.0), M.StreamingMosaic(
        index, 2, 32, hop=HOP, k=4, fit=5, gain_max=2.0)
    cap.capture()
    cap.reset()
    _same(_run(plain, x), _run(cap, x, replay=True))


def test_fit_zero_given_explicitly_is_the_default_construction(index):
    M = _M()
    x = _signal(np.random.default_rng(23), 2, 32 * 6)
    for cont, lag in ((0.0, 0), (0.5, 0), (0.5, 3)):
        kw = dict(hop=HOP, k=4, mode="grains", window="hann", continuity=cont, lag=lag)
        a, b = M.StreamingMosaic(index, 2, 32, **kw), M.StreamingMosaic(index, 2, 32, fit=0, gain_max=0.0, **kw)
        assert b.last_fit() is None and a.last_fit() is None and (b.fit, b.gain_max) == (0, 0.0)
        assert a._ws.numel() == b._ws.numel()
        fitted = M.StreamingMosaic(index, 2, 32, fit=0, gain_max=1.0, **kw)
        assert fitted._ws.numel() > a._ws.numel() and fitted.last_fit() is not None
        ra, rb = _run(a, x), _run(b, x)
        assert "shift" not in rb
        _same(ra, rb)
        assert all(_eq(p, q) for p, q in zip(a.last_matches(), b.last_matches()))
    b = M.StreamingMosaic(index, 2, 32, hop=HOP, k=4, mode="decode", fit=0, gain_max=0.0)
    assert b.last_fit() is None
    with pytest.raises(ValueError, match="fit"):
        M.StreamingMosaic(index, 2, 32, hop=HOP, k=4, mode="decode", fit=8)
    with pytest.raises(ValueError, match="gain_max"):
        M.StreamingMosaic(index, 2, 32, hop=HOP, k=4, mode="decode", gain_max=2.0)
    with pytest.raises(ValueError, match="fit"):
        M.StreamingMosaic(index, 2, 32, hop=HOP, k=4, fit=1025)


def test_a_frame_longer_than_a_staged_chunk_equals_offline():
    """S = 1280: the fit stages the frame in chunks of 1024 samples, and the ring of P + block = 1280 floats wraps inside
    a frame of every block after the first"""
    index = _index(_model(1280, 32, 8, seed=6), 320, lengths=(3000, 5000, 2600))
    x = _signal(np.random.default_rng(24), 2, 320 * 5)
    got = _against_offline(index, x, 320, 2, "hann", 9, 2.0, hop=320)
    assert int((got["shift"] != 0).sum()) > 0


def test_guard_bands_around_the_workspace_and_the_fit_outputs_stay_intact(index):
    M = _M()
    x = _signal(np.random.default_rng(25), 2, 32 * 5)
    for cont, lag in ((0.0, 0), (0.5, 3)):
        kw = dict(hop=HOP, k=4, mode="grains", window="hann", continuity=cont, lag=lag, fit=70, gain_max=2.0)
        ref = _run(M.StreamingMosaic(index, 2, 32, **kw), x)
        sm = M.StreamingMosaic(index, 2, 32, **kw)
        n, kf = sm._ws.numel(), sm._fit[0].shape[1]
        rows = sm.n_streams * sm.frames_per_block
        assert n % 256 == 0
        gws = guarded_flat(n // 4, torch.float32)
        gsh, ggn = guarded_flat(rows * kf, torch.float32), guarded_flat(rows * kf, torch.float32)
        gsc = guarded_flat(2 * rows * kf, torch.float32)
        sm._ws = gws.view.view(torch.uint8).reshape(-1)
        assert sm._ws.numel() == n and sm._ws.data_ptr() == gws.ptr and gws.ptr % 256 == 0
        sm._fit = (gsh.view.view(torch.int32).reshape(rows, kf), ggn.view.reshape(rows, kf),
                   gsc.view.view(torch.float64).reshape(rows, kf))
        sm.reset()
        got = _run(sm, x)
        sm.reset(1)
        sm.reset()
        for name, gd in (("workspace", gws), ("shift", gsh), ("gain", ggn), ("score", gsc)):
            gd.assert_untouched(name)
        _same(got, ref)
        assert _eq(_run(sm, x)["y"], ref["y"])


def test_cli_live_fit_writes_what_the_api_gives(tmp_path, capsys):
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd import data as D
    sys.path.insert(0, REPO)
    import mosaic as cli
    from rawaudiovae_kelsey_amd import frontend as interp_cli
    S_, H, L, sr = 64, 128, 8, 8000
    torch.manual_seed(3)
    torch.save({"epoch": 1, "state_dict": VAE(S_, H, L).state_dict(), "optimizer": {}}, tmp_path / "ckpt_00001")
    (tmp_path / "tiny.ini").write_text("[audio]\nsampling_rate = %d\nhop_length = 8\nsegment_length = %d\n"
                                       "[VAE]\nlatent_dim = %d\nn_units = %d\n" % (sr, S_, L, H))
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    rng = np.random.default_rng(4)
    for i, w in enumerate(_waves(rng, [400, 777, 1024])):
        D.write_wav(corpus / ("c%d.wav" % i), w, sr)
    D.write_wav(tmp_path / "t.wav", (0.3 * rng.standard_normal(999)).astype(np.float32), sr)
    argv = ["--config", str(tmp_path / "tiny.ini"), "--checkpoint", str(tmp_path / "ckpt_00001"), "--corpus", str(corpus),
            "--target", str(tmp_path / "t.wav"), "--out", str(tmp_path / "out.wav"), "--hop", "16", "--k", "3", "--window",
            "hann", "--matches", str(tmp_path / "m.csv"), "--live-block", "64"]
    y = cli.main(argv + ["--live-fit", "16", "--live-gain-max", "4"])
    said = capsys.readouterr().out
    assert ", live, block 64, streams 1, fit 16, gain-max 4" in said
    cfg = interp_cli.read_model_config(str(tmp_path / "tiny.ini"))
    index = _M().LatentIndex(interp_cli.load_model(str(tmp_path / "ckpt_00001"), cfg), hop=16)
    for f in sorted(os.listdir(corpus)):
        index.add(interp_cli.load_wav(str(corpus / f), sr), f)
    target = interp_cli.load_wav(str(tmp_path / "t.wav"), sr)
    want, idx, dist, choice, fits = cli.live_mosaic(index, target, 64, 16, 1, k=3, mode="grains", window="hann", fit=16,
                                                    gain_max=4.0)
    assert np.array_equal(y, want) and y.size == target.size and len(fits) == 3
    # ... which is the offline fitted mosaic where both have the whole target under their frames
    off = index.mosaic(torch.cat([torch.zeros(48), torch.from_numpy(target)]), k=3, hop=16, window="hann", fit=16,
                       gain_max=4.0)
    n = target.size // 16 * 16 - 64
    assert np.array_equal(y[:n].view(np.int32), off[48:48 + n].cpu().numpy().view(np.int32))
    D.write_wav(tmp_path / "ref.wav", want, sr)
    assert (tmp_path / "out.wav").read_bytes() == (tmp_path / "ref.wav").read_bytes()
    rows = list(csv.reader(open(tmp_path / "m.csv")))
    assert len(rows) == fits[0].shape[0] and all(len(r) == 15 for r in rows)
    assert [[int(r[3]), int(r[8]), int(r[13])] for r in rows] == fits[0].tolist()
    assert [[float(r[4]), float(r[9]), float(r[14])] for r in rows] == fits[1].astype(np.float64).tolist()
    plain = cli.main(argv)
    assert ", fit " not in capsys.readouterr().out and not np.array_equal(plain, y)
    assert all(len(r) == 9 for r in csv.reader(open(tmp_path / "m.csv")))
    # with selection and a lag: the slot, then the committed frame's shift and gain, aligned with its own candidates
    cli.main(argv + ["--live-fit", "16", "--continuity", "0.5", "--lag", "3"])
    assert ", live, lag 3, block 64, streams 1, fit 16, gain-max 0, continuity 0.5" in capsys.readouterr().out
    _, idx, _, choice, fits = cli.live_mosaic(index, target, 64, 16, 1, k=3, mode="grains", window="hann", continuity=0.5,
                                              lag=3, fit=16)
    rows = list(csv.reader(open(tmp_path / "m.csv")))
    assert len(rows) == len(choice) and all(len(r) == 12 for r in rows)
    assert [int(r[10]) for r in rows] == fits[0][:, 0].tolist() and np.all(fits[1][choice >= 0, 0] == 1.0)
    assert [int(r[9]) for r in rows] == [int((idx[t] == choice[t]).argmax()) if choice[t] >= 0 else -1
                                          for t in range(len(choice))]
