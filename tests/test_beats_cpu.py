"""The beat rules without a device: the header's op codes and field names, the library's argument checks (all made on the
host), the workspace sizes, the host helpers against their formulas, the numpy oracle (tests/beat_oracle.py) against
brute-force loops written on their own and its block-parallel tracker against the sequential one, the musical property on
planted pulses, and beats.py's flags and JSON."""
import ctypes as C
import json
import math
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import beat_oracle as O  # noqa: E402

sys.path.insert(0, REPO)

FAKE = 0x7000_0000_0000      # a non-null, 256-byte aligned address no check dereferences


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def test_op_codes_and_field_names_follow_the_header():
    from rawaudiovae_kelsey_amd import _lib
    text = open(REPO + "/include/rawvae_hip.h").read()
    codes = dict(re.findall(r"#define (RV_BEAT_\w+) (\d+)", text))
    assert codes == dict(RV_BEAT_ONSET="63", RV_BEAT_TEMPOGRAM="64", RV_BEAT_TRACK="65", RV_BEAT_WORKSPACE="66")
    assert (_lib.BEAT_ONSET, _lib.BEAT_TEMPOGRAM, _lib.BEAT_TRACK, _lib.BEAT_WORKSPACE) == (63, 64, 65, 66)
    assert _lib.BEAT_WORKSPACE in _lib._HOST_ONLY_OPS
    assert not {_lib.BEAT_ONSET, _lib.BEAT_TEMPOGRAM, _lib.BEAT_TRACK} & _lib._HOST_ONLY_OPS
    para = text[text.index("/* Latent beats"):text.index("#define RV_BEAT_ONSET")]
    types = {n: ctype for slot in abi_slots.header_slots() for n, ctype in slot}
    paragraphs = {op: para[para.index(" * RV_BEAT_%s:" % op):] for op in ("ONSET", "TEMPOGRAM", "TRACK", "WORKSPACE")}
    ends = [para.index(" * RV_BEAT_%s:" % op) for op in ("TEMPOGRAM", "TRACK", "WORKSPACE")] + [len(para)]
    for (op, p), end in zip(list(paragraphs.items()), ends):
        paragraphs[op] = para[para.index(" * RV_BEAT_%s:" % op):end]
    fields = dict(ONSET=(("T", "long"), ("moment", "const double*"), ("ws", "void*"), ("ws_bytes", "long"), ("result", "double*"),
                         ("summary", "int*"), ("cost", "double*")),
                  TEMPOGRAM=(("T", "long"), ("moment", "const double*"), ("width", "long"), ("hop", "long"), ("lag", "long"),
                             ("N", "long"), ("basis", "double*"), ("result", "double*"), ("ldo", "long"), ("centre", "double*"),
                             ("path", "int*"), ("info", "int*"), ("cost", "double*")),
                  TRACK=(("T", "long"), ("moment", "const double*"), ("lag", "long"), ("width", "long"), ("N", "long"),
                         ("basis", "double*"), ("result", "double*"), ("idx", "int*"), ("path", "int*"), ("n_out", "long"),
                         ("summary", "int*"), ("cost", "double*")),
                  WORKSPACE=(("T", "long"), ("ws_bytes", "long")))
    for op, want in fields.items():
        for field, ctype in want:
            assert re.search(r"\b%s\b" % field, paragraphs[op]), (op, field)
            assert hasattr(_lib.MosaicDesc, field) and types[field] == ctype, (field, types.get(field))
    # the ops of one call use distinct slots
    for op in ("ONSET", "TEMPOGRAM", "TRACK"):
        at = [getattr(_lib.MosaicDesc, f).offset for f, _ in fields[op]]
        assert len(set(at)) == len(at), op


def test_the_descriptor_the_version_the_exports_and_the_unassigned_codes_stay():
    from rawaudiovae_kelsey_amd import _lib
    assert len(abi_slots.check_layout()) == 37 and C.sizeof(_lib.MosaicDesc) == 37 * 8
    assert _lib.lib().rv_version() == 100
    assert not [n for n in _lib.EXPORTED if "beat" in n or "tempo" in n or "onset" in n]
    assert (_lib.MOSAIC_KNN, _lib.STRUCT_NOVELTY, _lib.OT_WORKSPACE) == (0, 31, 62)
    for op in (38, 39, 42, 48, 57, 67):
        with pytest.raises(_lib.RvError, match="unknown op %d" % op):
            _lib.lib().rv_mosaic(op, C.byref(_lib.MosaicDesc()), None)
    text = open(REPO + "/include/rawvae_hip.h").read()
    assert "The codes 38, 39, 42, 48 and 57 stay unassigned." in text


def _err(op, text, **fields):
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError) as e:
        _lib.lib().rv_mosaic(op, C.byref(_lib.MosaicDesc(**fields)), None)
    assert text in str(e.value), str(e.value)


def test_workspace_sizes_and_every_argument_error_names_its_field():
    from rawaudiovae_kelsey_amd import _lib, beats as B
    up = lambda n: -(-n // 256) * 256  # noqa: E731
    for T in (1, 256, 257, 5000, 52000):
        nb = -(-T // 256)
        assert B.workspace_bytes(T) == up(8 * nb) + 2 * up(4 * nb) + 256
    ons = dict(T=100, moment=FAKE, ws=FAKE, ws_bytes=B.workspace_bytes(100), result=FAKE + 4096, summary=FAKE, cost=FAKE)
    tg = dict(T=100, moment=FAKE, width=32, hop=8, lag=4, N=20, basis=FAKE, result=FAKE, ldo=17, centre=FAKE, path=FAKE,
              info=FAKE, cost=FAKE)
    tr = dict(T=100, moment=FAKE, lag=4, width=16, N=8, basis=FAKE, result=FAKE, idx=FAKE, path=FAKE, n_out=25, summary=FAKE,
              cost=FAKE)
    for name, op, ok in (("BEAT_ONSET", _lib.BEAT_ONSET, ons), ("BEAT_TEMPOGRAM", _lib.BEAT_TEMPOGRAM, tg),
                         ("BEAT_TRACK", _lib.BEAT_TRACK, tr), ("BEAT_WORKSPACE", _lib.BEAT_WORKSPACE, dict(T=100))):
        for T in (0, -3, 1 << 31):
            _err(op, "rv_mosaic(%s): T=%d outside [1, 2^31)" % (name, T), **dict(ok, T=T))
    need = ons["ws_bytes"]
    for change, what in ((dict(moment=None), "moment (the novelty curve) is null"), (dict(result=None), "result (the onset curve) is null"),
                         (dict(result=FAKE), "result may not be moment"), (dict(summary=None), "the summary is null"),
                         (dict(cost=None), "cost is null"), (dict(ws=None), "ws is null, T=100 needs %d bytes" % need),
                         (dict(ws=FAKE + 8), "ws is not 256-byte aligned"),
                         (dict(ws_bytes=need - 1), "ws_bytes=%d, T=100 needs %d" % (need - 1, need))):
        _err(_lib.BEAT_ONSET, "rv_mosaic(BEAT_ONSET): " + what, **dict(ons, **change))
    for change, what in ((dict(width=0), "width=0 (the window) outside [1, 8192]"), (dict(width=8193), "width=8193 (the window) outside"),
                         (dict(hop=0), "hop=0 (the frames between two windows) outside [1, 2^31)"),
                         (dict(lag=0), "lag=0 (the least lag) outside [1, 1024]"), (dict(lag=1025, N=1025), "lag=1025 (the least lag)"),
                         (dict(N=3), "N=3 (the largest lag) outside [lag=4, 1024]"), (dict(N=1025), "N=1025 (the largest lag) outside"),
                         (dict(T=1 << 23, hop=1), "hop=1 cuts T=8388608 frames into 8388608 windows, more than 2^22"),
                         (dict(ldo=16), "ldo=16 holds no row of 17 lags"),
                         (dict(moment=None), "moment (the onset curve) is null"),
                         (dict(basis=None), "basis (the window and the prior) is null"),
                         (dict(result=None), "result (the tempogram) is null"),
                         (dict(centre=None), "centre (the sum over the windows) is null"),
                         (dict(path=None), "the path (the windows' periods) is null"), (dict(info=None), "info is null"),
                         (dict(cost=None), "cost is null")):
        _err(_lib.BEAT_TEMPOGRAM, "rv_mosaic(BEAT_TEMPOGRAM): " + what, **dict(tg, **change))
    for change, what in ((dict(lag=0), "lag=0 (the nearest predecessor) outside [1, 2048]"), (dict(lag=2049, width=2049), "lag=2049"),
                         (dict(width=3), "width=3 (the furthest predecessor) outside [lag=4, 2048]"),
                         (dict(width=2049), "width=2049 (the furthest predecessor)"),
                         (dict(N=0), "N=0 (the end window) outside [1, 2048]"), (dict(N=2049), "N=2049 (the end window)"),
                         (dict(n_out=24), "n_out=24, T=100 frames at least lag=4 apart need 25"),
                         (dict(moment=None), "moment (the onset curve) is null"),
                         (dict(basis=None), "basis (the transition scores) is null"),
                         (dict(result=None), "result (the scores C) is null"), (dict(idx=None), "idx (the predecessors) is null"),
                         (dict(path=None), "the path (the beats) is null"), (dict(summary=None), "the summary is null"),
                         (dict(cost=None), "cost is null")):
        _err(_lib.BEAT_TRACK, "rv_mosaic(BEAT_TRACK): " + what, **dict(tr, **change))


def test_the_host_helpers_follow_their_formulas_and_refuse_by_name():
    from rawaudiovae_kelsey_amd import beats as B
    assert B.lag_range(40, 240, 44100, 256) == (math.ceil(60 * 44100 / (256 * 240)), math.floor(60 * 44100 / (256 * 40))) == (44, 258)
    assert B.lag_range(60, 60, 8000, 16) == (500, 500) and B.lag_range(40, 240, 22050, 256) == (22, 129)
    with pytest.raises(ValueError, match="bpm_min=40.0 is a period of 1033 frames"):
        B.lag_range(40, 240, 44100, 64)
    with pytest.raises(ValueError, match="bpm_max=50.0 leaves no period"):
        B.lag_range(60, 50, 44100, 256)
    for bad in (dict(bpm_min=0), dict(bpm_max=float("nan")), dict(sampling_rate=-1), dict(step="x")):
        with pytest.raises(ValueError, match=list(bad)[0] + "="):
            B.lag_range(**dict(dict(bpm_min=40, bpm_max=240, sampling_rate=44100, step=256), **bad))
    tau = np.arange(16, 129, dtype=np.float64)
    for centre, octaves in ((40.7, 1.0), (64.0, 0.5)):
        want = np.exp(-0.5 * (np.log2(tau / centre) / octaves) ** 2)
        assert np.array_equal(_bits(B.tempo_prior(16, 128, centre, octaves)), _bits(want))
        assert np.array_equal(_bits(want), _bits(O.tempo_prior(16, 128, centre, octaves)))
    assert B.tempo_prior(16, 128, 64.0)[48] == 1.0 and np.array_equal(B.tempo_prior(3, 9, None), np.ones(7))
    for call, msg in ((lambda: B.tempo_prior(0, 5, None), "lo=0"), (lambda: B.tempo_prior(6, 5, None), "hi=5"),
                      (lambda: B.tempo_prior(1, 1025, None), "hi=1025"), (lambda: B.tempo_prior(1, 5, 0.0), "centre=0.0"),
                      (lambda: B.tempo_prior(1, 5, 3.0, -1), "octaves=-1"), (lambda: B.window_values(0), "Wn=0"),
                      (lambda: B.window_values(8193), "Wn=8193"), (lambda: B.penalty_table(0), "P=0"),
                      (lambda: B.penalty_table(1025), "P=1025"), (lambda: B.penalty_table(8, -1.0), "tightness=-1.0"),
                      (lambda: B.penalty_table(True), "P=True")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            call()
    for Wn in (1, 2, 63, 512):
        w = B.window_values(Wn)
        n = np.arange(Wn)
        assert w.dtype == np.float64 and np.array_equal(w, 0.5 - 0.5 * np.cos(2 * np.pi * (n + 0.5) / Wn))
        assert np.array_equal(_bits(w), _bits(O.window_values(Wn))) and (w > 0).all() and np.allclose(w, w[::-1])
    assert B.window_values(1)[0] == 1.0
    for P, tight in ((1, 100.0), (2, 100.0), (37, 100.0), (1024, 400.0)):
        dlo, dhi, pen = B.penalty_table(P, tight)
        d = np.arange(dlo, dhi + 1, dtype=np.float64)
        assert (dlo, dhi) == ((P + 1) // 2, 2 * P) and np.array_equal(_bits(pen), _bits(-tight * np.log(d / P) ** 2))
        assert pen[P - dlo] == 0 and (pen <= 0).all() and np.array_equal(_bits(pen), _bits(O.penalty_table(P, tight)[2]))
    for call in (lambda: B.onset(torch.zeros(4, dtype=torch.float64)), lambda: B.onset(None),
                 lambda: B.tempogram(torch.zeros(4), 4, 1, 1, 2), lambda: B.track(torch.zeros(4, dtype=torch.float64), 2, [0.0], 1, 1)):
        with pytest.raises(ValueError, match="1-D float64 device tensor"):
            call()


def _brute_tempogram(o, Wn, Hw, lo, hi, win):
    """The header's rule term by term, sharing nothing with the oracle."""
    T = len(o)
    nW = -(-T // Hw)
    A = np.zeros((nW, hi - lo + 1))
    for n in range(nW):
        for tau in range(lo, hi + 1):
            acc = 0.0
            for i0 in range(0, Wn, 64):
                tile = 0.0
                for i in range(i0, min(Wn, i0 + 64)):
                    a = n * Hw + i
                    if a + tau >= T:
                        continue
                    tile = tile + float(win[i]) * (float(o[a]) * float(o[a + tau]))
                acc = acc + tile
            A[n, tau - lo] = acc
    return A


def test_the_oracle_equals_brute_force_loops():
    rs = np.random.RandomState(1)
    for T, Wn, Hw, lo, hi in ((40, 9, 5, 1, 6), (150, 70, 33, 3, 20), (130, 65, 64, 7, 7), (5, 3, 2, 5, 9)):
        o = np.abs(rs.randn(T))
        o[rs.randint(0, T, 3)] = 0.0
        win, prior = O.window_values(Wn), O.tempo_prior(lo, hi, 0.5 * (lo + hi))
        A, G, period, info, cost = O.tempogram(o, Wn, Hw, lo, hi, win, prior)
        assert np.array_equal(_bits(A), _bits(_brute_tempogram(o, Wn, Hw, lo, hi, win)))
        g = np.zeros(hi - lo + 1)
        for n in range(A.shape[0]):
            g = g + A[n]
        assert np.array_equal(_bits(G), _bits(g)) and info.tolist() == [info[0], -(-T // Hw), 0, 0]
        score = prior * G
        best = [t for t in range(lo, hi + 1) if score[t - lo] > 0 and score[t - lo] == score[score > 0].max()] if (score > 0).any() else [0]
        assert info[0] == best[0] and period.shape == (A.shape[0],)
    # the onset rule on a curve with every kind of entry
    nov = np.array([1.0, -2.0, np.nan, np.inf, -np.inf, -0.0, 0.0, 3.0] * 40)
    o, summary, cost = O.onset(nov)
    h = np.where(np.isfinite(nov) & (nov > 0), nov, 0.0)
    q = 0.0
    for b in range(0, 320, 256):
        part = 0.0
        for x in h[b:b + 256]:
            part += x * x
        q += part
    assert cost[0] == math.sqrt(q / 320) and summary.tolist() == [80, 200, 0, 0] and not np.signbit(o).any()
    assert np.array_equal(_bits(o), _bits(h / cost[0]))
    o, summary, cost = O.onset(np.array([-1.0, 0.0, np.nan]))
    assert not o.any() and not np.signbit(o).any() and summary.tolist() == [0, 2, 0, 0] and cost.tolist() == [0.0, 0.0]


@pytest.mark.parametrize("P", [2, 3, 37])
def test_the_block_parallel_tracker_equals_the_sequential_one_bit_for_bit(P):
    dlo, dhi, pen = O.penalty_table(P)
    rs = np.random.RandomState(P)
    for T in sorted({1, max(1, dlo - 1), dlo, dlo + 1, dhi, dhi + 1, 3 * dhi + 5, 400}):
        for kind in ("noise", "zero", "nan"):
            o = np.abs(rs.randn(T)) if kind != "zero" else np.zeros(T)
            if kind == "nan":
                o[T // 2] = np.nan
            seq, blk = O.track(o, dlo, dhi, P, pen), O.track_blocks(o, dlo, dhi, P, pen)
            assert np.array_equal(_bits(seq[0]), _bits(blk[0])) and np.array_equal(_bits(seq[4]), _bits(blk[4]))
            for a, b in zip(seq[1:4], blk[1:4]):
                assert np.array_equal(a, b)
            C, back, path, summary, cost = seq
            n, tstar = int(summary[0]), int(summary[1])
            beats = path[:n]
            assert n >= 1 and beats[-1] == tstar >= max(0, T - P) and (path[n:] == -1).all() and path.size == (T - 1) // dlo + 1
            assert (np.diff(beats) >= dlo).all() and (np.diff(beats) <= dhi).all() and back[beats[0]] == -1
            assert (back[:dlo] == -1).all() and (back[dlo:] >= 0).all() and not np.isnan(C).any()
            if kind == "zero":
                flat = O.track(o, dlo, dhi, P, np.zeros(dhi - dlo + 1))      # a flat table: every candidate ties, the nearest wins
                assert (flat[1][dlo:] == np.arange(dlo, T) - dlo).all() and not flat[0].any()
                assert np.array_equal(flat[1], O.track_blocks(o, dlo, dhi, P, np.zeros(dhi - dlo + 1))[1])


CASES = ((37, 900, 1), (60, 1500, 2), (23, 700, 0), (100, 2400, 3))


@pytest.mark.parametrize("P0,T,j", CASES)
def test_planted_pulses_are_found_at_their_tempo(P0, T, j):
    """Noise of N(0, 0.3) (seed 0) with a pulse of +3, and +1 on the next frame, every P0 frames, jittered by +-j
    (beat_oracle.pulse_curve).  lo, hi = 16, 128; Wn, Hw = 512, 128; the prior centred at 1.1 P0; tightness 100."""
    curve, pulses = O.pulse_curve(P0, T, j)
    P, beats, on, tg, tr = O.chain(curve, 16, 128, 512, 128, 1.1 * P0)
    print("P0 %d: P %d, %d beats for %d pulses" % (P0, P, beats.size, pulses.size))
    assert abs(P - P0) <= 2
    assert all(np.abs(beats - p).min() <= max(1, j) for p in pulses)
    assert abs(beats.size - pulses.size) <= 1
    assert np.isclose(np.sqrt(np.mean(on[0] ** 2)), 1.0) and (on[0] >= 0).all()      # the onset curve has an RMS of 1


def test_a_flat_prior_shows_the_octave_ambiguity_the_prior_is_there_for():
    """Without a prior the same curves prefer a multiple of the period in two of the four cases (a train of pulses
    correlates with itself at every multiple of its period and the window weighs them alike): pinned as the reason for
    the prior, not as a failure."""
    flat = [O.chain(O.pulse_curve(P0, T, j)[0], 16, 128, 512, 128, None)[0] for P0, T, j in CASES]
    print("flat prior:", flat)
    multiple = [round(P / P0) for P, (P0, _, _) in zip(flat, CASES)]
    assert all(abs(P - m * P0) <= 2 * m for P, m, (P0, _, _) in zip(flat, multiple, CASES))
    assert sum(m >= 2 for m in multiple) == 2 and sum(m == 1 for m in multiple) == 2


def test_silence_has_no_period_and_no_beats():
    from rawaudiovae_kelsey_amd import beats as B
    P, beats, on, tg, tr = O.chain(np.zeros(300), 16, 128, 64, 16, 40.0)
    assert P == 0 and beats.size == 0 and not tg[2].any() and tg[4].tolist() == [0.0, 0.0] and tr is None
    b = B.Beats(torch.zeros(300, dtype=torch.float64), torch.zeros(19, 113, dtype=torch.float64),
                torch.zeros(19, dtype=torch.int32), 0, (16, 128), 16, None, step=16, n_samples=4800, sampling_rate=8000)
    assert b.silent and b.n_beats == 0 and b.bpm == 0.0 and b.score == 0.0 and b.intervals == (0.0, 0.0)
    assert not b.bpm_over_time.any() and b.beat_seconds.size == 0
    offsets, labels = b.segments(4)
    assert offsets.tolist() == [0, 4800] and labels.tolist() == [4]


def _host_beats(frames, T=200, step=16, n=3203, sr=8000, P=25):
    from rawaudiovae_kelsey_amd import beats as B
    path = torch.full((T,), -1, dtype=torch.int32)
    path[:len(frames)] = torch.tensor(frames, dtype=torch.int32)
    tracked = (torch.zeros(T, dtype=torch.float64), torch.zeros(T, dtype=torch.int32), path,
               torch.tensor([len(frames), frames[-1], 0, 0], dtype=torch.int32), torch.tensor([12.5, 3.0], dtype=torch.float64))
    return B.Beats(torch.zeros(T, dtype=torch.float64), torch.zeros(4, 10, dtype=torch.float64),
                   torch.tensor([25, 0, 24, 50], dtype=torch.int32), P, (16, 128), 50, tracked, kernel=8, band=15,
                   step=step, n_samples=n, sampling_rate=sr)


def test_beats_py_flags_and_a_json_that_segment_py_split_takes(tmp_path):
    import beats as cli
    import segment
    from rawaudiovae_kelsey_amd import data as D
    find = ["find", "--checkpoint", "c", "--in", "a.wav", "--out", "b.json"]
    args = cli.parse_args(find + ["--hop", "256"])
    assert (args.command, args.hop, args.bpm, args.octaves, args.bpm_min, args.bpm_max) == ("find", 256, 120.0, 1.0, 40.0, 240.0)
    assert (args.kernel, args.tightness, args.window_seconds, args.meter, args.onset, args.tempogram) == (8, 100.0, 8.0, 4, None, None)
    assert cli.parse_args(find + ["--bpm", "none"]).bpm is None
    args = cli.parse_args(["click", "--beats", "b.json", "--in", "a.wav", "--out", "o.wav"])
    assert (args.command, args.beats, args.wav, args.out) == ("click", "b.json", "a.wav", "o.wav")
    for argv, msg in ((find + ["--hop", "0"], "--hop '0'"), (find + ["--kernel", "0"], "--kernel '0'"),
                      (find + ["--kernel", "513"], "--kernel 513: at most 512"), (find + ["--bpm", "0"], "--bpm '0'"),
                      (find + ["--bpm", "x"], "--bpm 'x'"), (find + ["--octaves", "0"], "--octaves '0'"),
                      (find + ["--bpm-min", "-1"], "--bpm-min '-1'"), (find + ["--bpm-max", "inf"], "--bpm-max 'inf'"),
                      (find + ["--bpm-min", "300"], "--bpm-min 300: above --bpm-max 240"),
                      (find + ["--tightness", "-1"], "--tightness '-1'"), (find + ["--window-seconds", "0"], "--window-seconds '0'"),
                      (find + ["--meter", "0"], "--meter '0'"), ([], "expected a command: find or click")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            cli.parse_args(argv)
    with pytest.raises(SystemExit):
        cli.parse_args(["find", "--checkpoint", "c", "--out", "b.json"])            # no --in
    args = cli.parse_args(find + ["--hop", "256"])
    assert cli.tempogram_plan(args, 44100, 256) == ((44, 258), 1378, 172, 60.0 * 44100 / 256 / 120)
    with pytest.raises(ValueError, match="--bpm-min 40 --bpm-max 240: bpm_min=40.0 is a period of 1033 frames"):
        cli.tempogram_plan(args, 44100, 64)
    with pytest.raises(ValueError, match="--window-seconds 60: 10336 frames, at most 8192"):
        cli.tempogram_plan(cli.parse_args(find + ["--window-seconds", "60"]), 44100, 256)
    # the report of beats at frames 10, 35, 60, ..: what segment.py split checks, and what it cuts
    frames = list(range(10, 200, 25))
    b = _host_beats(frames)
    assert b.n_beats == 8 and b.beat_frames.tolist() == frames and b.score == 12.5 and b.intervals == (25.0, 0.0)
    assert b.bpm == 60.0 * 8000 / (16 * 25) and b.bpm_over_time.tolist() == [1200.0, 0.0, 1250.0, 600.0]
    rep = cli.report_of(b, 3, 16)
    assert rep["beat_samples"] == [16 * f for f in frames] and rep["beat_seconds"] == [16 * f / 8000 for f in frames]
    assert rep["sample_offsets"] == [0] + rep["beat_samples"] + [3203] and rep["labels"] == [3, 0, 1, 2, 0, 1, 2, 0, 1]
    assert (rep["period"], rep["bpm"], rep["beats"], rep["meter"], rep["silent"]) == (25, 1200.0, 8, 3, False)
    assert _host_beats([0, 25, 50]).segments(4)[0].tolist() == [0, 400, 800, 3203]          # a beat at 0: no piece before it
    assert _host_beats([0, 25, 50]).segments(4)[1].tolist() == [0, 1, 2]
    wave = (0.1 * np.random.RandomState(0).randn(3203)).astype(np.float32)
    D.write_wav(tmp_path / "in.wav", wave, 8000)
    (tmp_path / "b.json").write_text(json.dumps(rep))
    names = segment.main(["split", "--segments", str(tmp_path / "b.json"), "--in", str(tmp_path / "in.wav"),
                          "--out-dir", str(tmp_path / "parts")])
    parts = [D.load_audio_mono(n, 8000) for n in names]
    assert len(names) == 9 and [p.size for p in parts] == np.diff(rep["sample_offsets"]).tolist()
    assert np.array_equal(np.concatenate(parts), wave)
    out = cli.main(["click", "--beats", str(tmp_path / "b.json"), "--in", str(tmp_path / "in.wav"), "--out", str(tmp_path / "o.wav")])
    got = D.load_audio_mono(tmp_path / "o.wav", 8000)
    assert got.size == wave.size and np.array_equal(got, out)
    changed = np.flatnonzero(got != wave)
    m = int(round(cli.CLICK_SECONDS * 8000))
    assert changed.size and all(any(s <= c < s + m for s in rep["beat_samples"]) for c in changed)
    assert all(np.abs(got[s:s + m] - wave[s:s + m]).max() > 0.1 for s in rep["beat_samples"])
    D.write_wav(tmp_path / "short.wav", wave[:-5], 8000)
    with pytest.raises(ValueError, match="--beats"):
        cli.main(["click", "--beats", str(tmp_path / "b.json"), "--in", str(tmp_path / "short.wav"), "--out", str(tmp_path / "x.wav")])
