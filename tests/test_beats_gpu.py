"""The three beat ops on the device against tests/beat_oracle.py, exactly: every fp64 output bit for bit, every index
equal.  Inputs are read from between NaN guards and outputs written between sentinel guards (tests/guarded.py), so a
read or a write outside an operand fails the comparison or assert_untouched.  The shapes are the smallest at which the
kernels take each of their paths: the 256-frame blocks of the onset sum, the 64-term tiles and the 256-lag workgroups of
the tempogram, windows cut by the end of the curve, and for the tracker every number of lanes per frame from a whole wave
(dlo = 1) to one lane and two passes (dlo > 1024).  Then the whole chain on the tiny model against the oracle chain on
the device's own mu rows, beats.py's two commands, and a captured replay."""
import functools
import json
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import align_oracle as AO  # noqa: E402
import beat_oracle as O  # noqa: E402
import structure_oracle as SO  # noqa: E402
from guarded import INT_FILL, guarded, guarded_flat  # noqa: E402

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _same(got, want, what):
    got, want = _np(got) if torch.is_tensor(got) else np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(_bits(got), _bits(want)), (what, np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())[:8])


def _between_nans(values):
    """A float64 device vector between two guards of 64 NaN: reading a guard poisons the result."""
    values = np.asarray(values, np.float64)
    flat = torch.full((values.size + 128,), float("nan"), dtype=torch.float64, device="cuda")
    flat[64:64 + values.size] = torch.from_numpy(values).cuda()
    return flat[64:64 + values.size]


def _f64(n):
    return guarded_flat(n, torch.float64)


def _i32(n):
    return guarded_flat(n, torch.int32, fill=INT_FILL)


def _flat(g):
    return g.view.view(-1)


def _onset(nov):
    from rawaudiovae_kelsey_amd import beats as B
    T = len(nov)
    go, gs, gc = _f64(T), _i32(4), _f64(2)
    ws = torch.full((B.workspace_bytes(T),), 7, dtype=torch.uint8, device="cuda")
    B.onset(_between_nans(nov), ws, out=(_flat(go), _flat(gs), _flat(gc)))
    for g, name in ((go, "o"), (gs, "summary"), (gc, "cost")):
        g.assert_untouched(name)
    return _np(_flat(go)).copy(), _np(_flat(gs)).copy(), _np(_flat(gc)).copy()


def _tempogram(o, Wn, Hw, lo, hi, win, prior, ldo=None):
    from rawaudiovae_kelsey_amd import beats as B
    T, nlag = len(o), hi - lo + 1
    nW = -(-T // Hw)
    ga = guarded(nW, nlag, nlag if ldo is None else ldo, torch.float64)
    gg, gp, gi, gc = _f64(nlag), _i32(nW), _i32(4), _f64(2)
    table = _between_nans(np.concatenate([win, prior]))
    B.tempogram(_between_nans(o), Wn, Hw, lo, hi, table=table, out=(ga.view, _flat(gg), _flat(gp), _flat(gi), _flat(gc)))
    for g, name in ((ga, "A"), (gg, "G"), (gp, "period"), (gi, "info"), (gc, "cost")):
        g.assert_untouched(name)
    return tuple(_np(x).copy() for x in (ga.view, _flat(gg), _flat(gp), _flat(gi), _flat(gc)))


def _track(o, P, pen, dlo, dhi, extra=0):
    from rawaudiovae_kelsey_amd import beats as B
    T = len(o)
    n_out = (T - 1) // dlo + 1 + extra
    gC, gb, gp, gs, gc = _f64(T), _i32(T), _i32(n_out), _i32(4), _f64(2)
    B.track(_between_nans(o), P, _between_nans(pen), dlo, dhi, out=(_flat(gC), _flat(gb), _flat(gp), _flat(gs), _flat(gc)))
    for g, name in ((gC, "C"), (gb, "back"), (gp, "beats"), (gs, "summary"), (gc, "cost")):
        g.assert_untouched(name)
    return tuple(_np(_flat(g)).copy() for g in (gC, gb, gp, gs, gc))


NAMES_TG = ("A", "G", "period", "info", "cost")
NAMES_TR = ("C", "back", "beats", "summary", "cost")


# ---- onset -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 513, 1000])
def test_onset_equals_the_oracle_bit_for_bit(T):
    rs = np.random.RandomState(T)
    plain = rs.randn(T)
    mixed = rs.randn(T)
    for k, v in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0, -3.0)):
        mixed[(k * 37) % T] = v
    for name, nov in (("plain", plain), ("mixed", mixed), ("huge", plain * 1e200), ("tiny", plain * 1e-200)):
        got, want = _onset(nov), O.onset(nov)
        for g, w, what in zip(got, want, ("o", "summary", "cost")):
            _same(g, w, "%s %s" % (name, what))
        assert not np.signbit(got[0]).any() and not np.isnan(got[0]).any()
    # nothing above 0: s = 0 and every entry +0
    dull = -np.abs(plain)
    dull[0], dull[T // 2] = -0.0, np.nan
    o, summary, cost = _onset(dull)
    assert not _bits(o).any() and cost.tolist() == [0.0, 0.0] and summary[0] == 0 and summary[1] == np.isfinite(dull).sum()


# ---- tempogram ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Wn", [1, 63, 64, 65, 200])
def test_tempogram_equals_the_oracle_bit_for_bit(Wn):
    lo, hi, Hw = 3, 20, 7
    rs = np.random.RandomState(Wn)
    win, prior = O.window_values(Wn), O.tempo_prior(lo, hi, 9.0)
    for T in sorted({lo, lo + 1, Wn + hi - 1, Wn + hi, 3 * Hw + 5}):
        for kind in ("signed", "positive", "nan"):
            o = rs.randn(T) if kind != "positive" else np.abs(rs.randn(T))
            if kind == "nan":
                o[T // 2] = np.nan
            for hop in (Hw, max(1, T // 2), T + 3):
                got, want = _tempogram(o, Wn, hop, lo, hi, win, prior), O.tempogram(o, Wn, hop, lo, hi, win, prior)
                for g, w, what in zip(got, want, NAMES_TG):
                    _same(g, w, "T %d %s hop %d %s" % (T, kind, hop, what))


def test_tempogram_at_one_lag_at_the_largest_lag_and_with_a_row_pitch():
    rs = np.random.RandomState(5)
    o = np.abs(rs.randn(300))
    for lo, hi, Wn, Hw, ldo in ((17, 17, 70, 40, None), (17, 17, 70, 40, 5), (5, 40, 130, 64, 50), (250, 520, 33, 100, 300)):
        win, prior = O.window_values(Wn), O.tempo_prior(lo, hi, 0.6 * (lo + hi))
        got, want = _tempogram(o, Wn, Hw, lo, hi, win, prior, ldo), O.tempogram(o, Wn, Hw, lo, hi, win, prior)
        for g, w, what in zip(got, want, NAMES_TG):
            _same(g, w, (lo, hi, what))
    o = np.abs(rs.randn(1100))
    o[::700] += 9.0
    win, prior = O.window_values(64), O.tempo_prior(1, 1024, 700.0, 2.0)
    got, want = _tempogram(o, 64, 300, 1, 1024, win, prior), O.tempogram(o, 64, 300, 1, 1024, win, prior)
    for g, w, what in zip(got, want, NAMES_TG):
        _same(g, w, ("hi 1024", what))
    assert got[3][0] > 513 and got[3][1] == 4                       # a lag of the third workgroup of lags wins


def test_tempogram_ties_go_to_the_smaller_lag_and_silence_has_no_period():
    lo, hi, Wn = 4, 300, 16
    ones, flat = np.ones(Wn), np.ones(hi - lo + 1)
    o = np.full(Wn + hi + 40, 0.5)
    # one whole window: every lag sums the same 16 terms
    A, G, period, info, cost = _tempogram(o, Wn, o.size + 1, lo, hi, ones, flat)
    assert (A == 4.0).all() and info.tolist() == [lo, 1, 0, 0] and period.tolist() == [lo] and cost.tolist() == [4.0, 4.0]
    got, want = _tempogram(o, Wn, 50, lo, hi, ones, flat), O.tempogram(o, Wn, 50, lo, hi, ones, flat)
    for g, w, what in zip(got, want, NAMES_TG):
        _same(g, w, what)
    assert got[2][0] == lo
    # a tie between two lags 256 apart (two workgroups of lags, two rounds of the argmax)
    prior = np.zeros(hi - lo + 1)
    prior[[260 - lo, 5 - lo]] = 1.0
    assert _tempogram(o, Wn, o.size + 1, lo, hi, ones, prior)[3][0] == 5
    # silence, and a curve whose every score is negative or NaN
    for curve, pr in ((np.zeros(200), flat), (np.full(400, 0.5), -flat), (np.full(400, np.nan), flat)):
        A, G, period, info, cost = _tempogram(curve, Wn, 32, lo, hi, ones, pr)
        want = O.tempogram(curve, Wn, 32, lo, hi, ones, pr)
        assert info.tolist() == [0, -(-curve.size // 32), 0, 0] == want[3].tolist() and not period.any()
        assert not _bits(cost).any() and np.array_equal(np.isnan(A), np.isnan(want[0]))
        assert np.array_equal(_bits(A[~np.isnan(A)]), _bits(want[0][~np.isnan(A)]))


# ---- tracker -----------------------------------------------------------------------------------------------------------

def _check_track(o, P, pen, dlo, dhi, what, extra=0):
    got = _track(o, P, pen, dlo, dhi, extra)
    want = O.track(o, dlo, dhi, P, pen, (len(o) - 1) // dlo + 1 + extra)
    for g, w, name in zip(got, want, NAMES_TR):
        _same(g, w, (what, name))
    return got


@pytest.mark.parametrize("P", [1, 2, 3, 7, 37, 512, 1024])
def test_track_equals_the_oracle_bit_for_bit(P):
    dlo, dhi, pen = O.penalty_table(P)
    rs = np.random.RandomState(P)
    for T in sorted({1, max(1, dlo - 1), dlo, dlo + 1, dhi, dhi + 1, 3 * dhi + 5}):
        o = np.abs(rs.randn(T))
        o[::max(2, P)] += 3.0
        C, back, beats, summary, cost = _check_track(o, P, pen, dlo, dhi, ("noise", T), extra=T % 3)
        n = summary[0]
        assert n >= 1 and (beats[n:] == -1).all() and (np.diff(beats[:n]) >= dlo).all()
        poisoned = o.copy()
        poisoned[T // 2], poisoned[T // 3] = np.nan, np.inf
        _check_track(poisoned, P, pen, dlo, dhi, ("nan", T))
    T = 3 * dhi + 5
    _check_track(np.zeros(T), P, pen, dlo, dhi, "zero")
    # a flat table on a silent curve: every candidate ties and the nearer predecessor wins
    C, back, beats, summary, cost = _check_track(np.zeros(T), P, np.zeros(dhi - dlo + 1), dlo, dhi, "ties")
    assert (back[dlo:] == np.arange(dlo, T) - dlo).all() and (back[:dlo] == -1).all() and not _bits(C).any()
    assert summary[1] == max(0, T - P)                              # equal ends: the earlier frame


def test_track_with_one_lane_per_frame_two_passes_and_tables_that_hold_nan_and_inf():
    rs = np.random.RandomState(11)
    for dlo, dhi, P, T in ((600, 700, 100, 2300), (1500, 2048, 2048, 5000), (1025, 1025, 1, 3100), (1, 2048, 5, 2200),
                           (1, 1, 1, 70), (33, 64, 2048, 500)):
        pen = -np.abs(rs.randn(dhi - dlo + 1))
        o = np.abs(rs.randn(T))
        _check_track(o, P, pen, dlo, dhi, (dlo, dhi))
        pen[::5] = np.nan
        pen[1::7] = -np.inf
        _check_track(o, P, pen, dlo, dhi, (dlo, dhi, "nan"))
    # no admissible step at all: every frame starts a path of its own
    C, back, beats, summary, cost = _check_track(np.abs(rs.randn(50)), 4, np.full(3, np.nan), 2, 4, "all nan")
    assert (back == -1).all() and summary[0] == 1


# ---- errors ------------------------------------------------------------------------------------------------------------

def test_a_refused_call_leaves_every_output_untouched():
    from rawaudiovae_kelsey_amd import _lib, beats as B
    T = 100
    o = _between_nans(np.abs(np.random.RandomState(0).randn(T)))
    table = _between_nans(np.ones(32 + 17))
    ws = torch.full((B.workspace_bytes(T),), 7, dtype=torch.uint8, device="cuda")
    outs = dict(o=_f64(T), A=guarded(13, 17, 17, torch.float64), G=_f64(17), period=_i32(13), info=_i32(4), cost=_f64(2),
                C=_f64(T), back=_i32(T), beats=_i32(25), summary=_i32(4))
    ons = dict(T=T, moment=o.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel(), result=outs["o"].ptr, summary=outs["summary"].ptr,
               cost=outs["cost"].ptr)
    tg = dict(T=T, moment=o.data_ptr(), width=32, hop=8, lag=4, N=20, basis=table.data_ptr(), result=outs["A"].ptr, ldo=17,
              centre=outs["G"].ptr, path=outs["period"].ptr, info=outs["info"].ptr, cost=outs["cost"].ptr)
    tr = dict(T=T, moment=o.data_ptr(), lag=4, width=16, N=8, basis=table.data_ptr(), result=outs["C"].ptr, idx=outs["back"].ptr,
              path=outs["beats"].ptr, n_out=25, summary=outs["summary"].ptr, cost=outs["cost"].ptr)
    bad = [(_lib.BEAT_ONSET, ons, dict(T=0), "T=0"), (_lib.BEAT_ONSET, ons, dict(ws_bytes=8), "ws_bytes=8"),
           (_lib.BEAT_ONSET, ons, dict(cost=None), "cost is null"), (_lib.BEAT_TEMPOGRAM, tg, dict(width=8193), "width=8193"),
           (_lib.BEAT_TEMPOGRAM, tg, dict(N=1025), "N=1025"), (_lib.BEAT_TEMPOGRAM, tg, dict(ldo=16), "ldo=16"),
           (_lib.BEAT_TEMPOGRAM, tg, dict(info=None), "info is null"), (_lib.BEAT_TRACK, tr, dict(width=2049), "width=2049"),
           (_lib.BEAT_TRACK, tr, dict(n_out=24), "n_out=24"), (_lib.BEAT_TRACK, tr, dict(idx=None), "idx (the predecessors) is null")]
    for op, ok, change, what in bad:
        with pytest.raises(_lib.RvError) as e:
            _lib.lib().rv_mosaic(op, _lib.C.byref(_lib.MosaicDesc(**dict(ok, **change))), _lib.stream_ptr())
        assert what in str(e.value) and "rv_mosaic(BEAT_" in str(e.value), (what, str(e.value))
    torch.cuda.synchronize()
    for name, g in outs.items():
        g.assert_untouched(name)
        assert (_np(g.view) == g.fill).all(), name
    assert (_np(ws) == 7).all()
    for op, ok in ((_lib.BEAT_ONSET, ons), (_lib.BEAT_TEMPOGRAM, tg), (_lib.BEAT_TRACK, tr)):      # unchanged, they run
        _lib.lib().rv_mosaic(op, _lib.C.byref(_lib.MosaicDesc(**ok)), _lib.stream_ptr())
    torch.cuda.synchronize()
    for name, g in outs.items():
        assert not (_np(g.view) == g.fill).all(), name


# ---- end to end ----------------------------------------------------------------------------------------------------

SEG, H, LAT, SR, HOP = 64, 32, 8, 8000, 16        # the tiny model of tests/test_align_gpu.py
P0, BURSTS, BURST, KERNEL = 20, 20, 96, 8
LAGS, WINDOW, WINDOW_HOP = (8, 64), 128, 16


def _model():
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.synth import make_params
    m = VAE(SEG, H, LAT).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(SEG, H, LAT, 0).items()})
    return m


@functools.lru_cache(maxsize=None)
def _wave():
    """(wave, the burst onsets in samples): BURSTS bursts of noise, BURST samples long, one in the middle of every
    P0 * HOP samples, over a floor of faint noise."""
    rng = np.random.default_rng(0)
    w = 0.01 * rng.uniform(-1, 1, BURSTS * P0 * HOP)
    at = []
    for k in range(BURSTS):
        a = k * P0 * HOP + (P0 * HOP) // 2
        w[a:a + BURST] += 0.6 * rng.uniform(-1, 1, BURST)
        at.append(a)
    w = w.astype(np.float32)
    w.setflags(write=False)
    return w, np.array(at)


def _oracle_chain(mu, lags, window, window_hop, centre):
    T = mu.shape[0]
    r = 2 * KERNEL - 1 if T >= 2 * (2 * KERNEL - 1) + 1 else 0
    nov = SO.novelty(AO.local_costs(mu, mu, r)[1], KERNEL, SO.taper(KERNEL, 0.5))
    return O.chain(nov, lags[0], lags[1], window, window_hop, centre)


def test_the_tracker_equals_the_oracle_chain_on_the_devices_own_latents_and_finds_the_bursts():
    from rawaudiovae_kelsey_amd import beats as B
    wave, at = _wave()
    b = B.BeatTracker(_model()).track(np.array(wave), HOP, KERNEL, 0.5, LAGS, WINDOW, WINDOW_HOP, None, 1.0, 100.0, SR)
    P, beats, on, tg, tr = _oracle_chain(_np(b.mu), LAGS, WINDOW, WINDOW_HOP, None)
    assert b.period == P == P0 and not b.silent and b.T == b.mu.shape[0] == wave.size // HOP - SEG // HOP + 1
    _same(b.onset, on[0], "onset")
    _same(b.tempogram, tg[0], "tempogram")
    _same(b.window_periods, tg[2], "periods")
    for g, w, name in zip(b._tracked, tr, NAMES_TR):
        _same(g, w, name)
    assert b.beat_frames.tolist() == beats.tolist() and b.n_beats == tr[3][0] and b.score == tr[4][0]
    assert b.bpm == 60.0 * SR / (HOP * P0) and b.beat_samples.tolist() == (beats * HOP).tolist()
    # a frame sees SEG / HOP hops of sound and the kernel KERNEL frames: no beat is further from a burst's onset
    bound = SEG // HOP + KERNEL
    dist = [np.abs(at / HOP - t).min() for t in beats]
    print("period %d, %d beats for %d bursts, furthest from an onset: %.1f frames (bound %d)" % (P, beats.size, BURSTS, max(dist), bound))
    assert max(dist) <= bound and abs(beats.size - BURSTS) <= 1
    mean, std = b.intervals
    assert abs(mean - P0) <= 1 and std <= 2


def test_beats_py_find_split_and_click(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import beats as cli
    import segment
    from rawaudiovae_kelsey_amd import beats as B, data as D
    wave, _ = _wave()
    D.write_wav(tmp_path / "in.wav", wave, SR)
    ini = tmp_path / "m.ini"
    ini.write_text("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n" % (SR, SEG, H, LAT))
    ck = tmp_path / "ckpt"
    torch.save({"epoch": 0, "state_dict": _model().state_dict(), "optimizer": {}}, ck)
    rep = cli.main(["find", "--config", str(ini), "--checkpoint", str(ck), "--in", str(tmp_path / "in.wav"), "--hop", str(HOP),
                    "--bpm", "none", "--bpm-min", "468.75", "--bpm-max", "3750", "--window-seconds", "0.256", "--meter", "4",
                    "--onset", str(tmp_path / "o.npy"), "--tempogram", str(tmp_path / "tg.npy"), "--out", str(tmp_path / "b.json")])
    lines = capsys.readouterr().out.strip().splitlines()
    assert json.loads(lines[-1]) == rep == json.loads((tmp_path / "b.json").read_text())
    a = D.load_audio_mono(tmp_path / "in.wav", SR)
    b = B.BeatTracker(_model()).track(a, HOP, 8, 0.5, LAGS, WINDOW, SR // HOP, None, 1.0, 100.0, SR)
    assert rep["lags"] == list(LAGS) and rep["window_hop"] == SR // HOP and rep["period"] == b.period == P0
    assert rep["beat_frames"] == b.beat_frames.tolist() and rep["beats"] == b.n_beats >= BURSTS - 1
    assert rep["beat_samples"] == [HOP * f for f in rep["beat_frames"]] and rep["bpm"] == 60.0 * SR / (HOP * P0)
    assert rep["bpm_over_time"] == b.bpm_over_time.tolist() and len(rep["bpm_over_time"]) == -(-b.T // (SR // HOP))
    _same(np.load(tmp_path / "o.npy"), _np(b.onset), "onset file")
    _same(np.load(tmp_path / "tg.npy"), _np(b.tempogram), "tempogram file")
    assert lines[-2] == "%.6g bpm (period %d frames), %d beats, interval %.6g +- %.6g frames" % (
        rep["bpm"], P0, b.n_beats, b.intervals[0], b.intervals[1])
    first = [0] if rep["beat_samples"][0] > 0 else []
    assert rep["sample_offsets"] == first + rep["beat_samples"] + [a.size]
    assert rep["labels"] == [4] * len(first) + [k % 4 for k in range(b.n_beats)]
    names = segment.main(["split", "--segments", str(tmp_path / "b.json"), "--in", str(tmp_path / "in.wav"),
                          "--out-dir", str(tmp_path / "parts")])
    parts = [D.load_audio_mono(n, SR) for n in names]
    assert [p.size for p in parts] == np.diff(rep["sample_offsets"]).tolist() and np.array_equal(np.concatenate(parts), a)
    out = cli.main(["click", "--beats", str(tmp_path / "b.json"), "--in", str(tmp_path / "in.wav"), "--out", str(tmp_path / "c.wav")])
    got = D.load_audio_mono(tmp_path / "c.wav", SR)
    assert got.size == a.size == out.size and not np.array_equal(got, a)


def test_a_captured_replay_of_onset_and_tempogram_equals_the_eager_bits():
    from rawaudiovae_kelsey_amd import beats as B
    from rawaudiovae_kelsey_amd.engine import Graph
    T, Wn, Hw, lo, hi = 700, 130, 32, 5, 300
    curve, _ = O.pulse_curve(37, T, 1)
    nov = torch.from_numpy(curve).cuda()
    table = B.tempogram_table(O.window_values(Wn), O.tempo_prior(lo, hi, 40.0), Wn, lo, hi, nov.device)
    eager_o = B.onset(nov)
    eager = B.tempogram(eager_o[0], Wn, Hw, lo, hi, table=table)
    want_o = O.onset(curve)
    want = O.tempogram(want_o[0], Wn, Hw, lo, hi, O.window_values(Wn), O.tempo_prior(lo, hi, 40.0))
    static = nov.clone()
    ws = B.workspace(T, nov.device)
    out_o = tuple(torch.empty_like(t) for t in eager_o)
    out = tuple(torch.empty_like(t) for t in eager)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = Graph(side)
    with g:
        B.onset(static, ws, out=out_o, stream=side.cuda_stream)
        B.tempogram(out_o[0], Wn, Hw, lo, hi, table=table, out=out, stream=side.cuda_stream)
    torch.cuda.current_stream().wait_stream(side)
    static.copy_(torch.flip(nov, (0,)))                                 # other operands first: the replay reads the buffers
    g.launch(torch.cuda.current_stream())
    static.copy_(nov)
    g.launch(torch.cuda.current_stream())
    torch.cuda.synchronize()
    for got, e, w, name in zip(out_o + out, eager_o + eager, want_o + want, ("o", "summary", "cost") + NAMES_TG):
        _same(got, _np(e), "replay against eager " + name)
        _same(got, w, "replay against the oracle " + name)
    assert int(out[3][0]) > 0 and int(out[3][1]) == -(-T // Hw)
