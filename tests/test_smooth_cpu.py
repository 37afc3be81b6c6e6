"""Latent restoration without a device: the oracle's two smoothers against one another (tests/smooth_oracle.py: the
textbook filter with a Rauch-Tung-Striebel pass, and the kernels' Bryson-Frazier recursion in longdouble), the host
integer logic at its edges against brute-force forms, the op codes and the descriptor's unchanged layout, every argument
error of the four ops (all made on the host, before any launch), the Python checks and restore.py's parser."""
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import smooth_oracle as O  # noqa: E402

FAKE = 0x7000_0000_0000      # a non-null, 256-byte aligned address no check dereferences
AGREE = 1e-13                # RTS against Bryson-Frazier, both in longdouble (2^-64 = 5.4e-20 times the conditioning)


@pytest.mark.parametrize("k,L,diagonal", [(1, 1, False), (2, 3, False), (17, 17, False), (17, 70, False), (17, 17, True)])
def test_the_oracles_rts_and_a_longdouble_bryson_frazier_agree(k, L, diagonal):
    worst = 0.0
    for lengths in O.LENGTHS:
        for mask in O.MASKS:
            for r in O.NOISES:
                c = O.case(k, L, diagonal, lengths, mask, r)
                m = c["model"]
                rt = O.noise_of(r, c["weight"])
                for a, b in zip(c["row_start"][:-1], c["row_start"][1:]):
                    wp, wh = O.bryson_frazier(c["y"][a:b], c["obs"][a:b], rt[a:b], m["A"], m["B"])
                    scale = c["ynorm"][a]
                    worst = max(worst, float(np.abs(wp - c["wp"][a:b]).max() / scale),
                                float(np.abs(wh - c["wh"][a:b]).max() / scale))
                    assert np.array_equal(c["wh"][b - 1], c["wp"][b - 1])           # nothing follows the last frame
                    if not c["obs"][a:b].any():
                        assert not c["wh"][a:b].any() and not wh.any()                # no observation: the prior mean
                assert np.isfinite(c["z"].astype(np.float64)).all() and np.isnan(c["x"][~c["obs"]]).all()
    print("k %d L %d %s: RTS against Bryson-Frazier, worst normalised difference %.3g" % (
        k, L, "diagonal" if diagonal else "dense", worst))
    assert worst <= AGREE


def test_the_oracles_dense_and_scalar_forms_agree_on_a_diagonal_model():
    c = O.case(17, 17, True, (37, 1, 90), "alternating", 1e-2)
    m = c["model"]
    rt = O.noise_of(1e-2, c["weight"])
    dense = O.kalman_rts(c["y"][:37], c["obs"][:37], rt[:37], m["A"], m["B"], diagonal=False)
    for key in ("wp", "wh", "nis", "logdet"):
        got, want = np.asarray(dense[key], np.float64), np.asarray(c[key][:37], np.float64)
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), key


def test_frame_mask_and_regions_at_their_edges():
    from rawaudiovae_kelsey_amd import smooth as SM
    S = 64
    for n, hop in ((1000, 16), (1000, 64), (1000, None), (64, 16), (130, 32)):
        for ranges in ([(0, 1)], [(n - 1, n)], [(0, 5), (n - 3, n)], [(500 % n, 500 % n + 1)], [(63, 64)], [(64, 65)],
                       [(100 % n, 117 % n + 1), (120 % n + 1, 125 % n + 2)], [(0, n)]):
            got = SM.frame_mask(n, S, hop, ranges)
            want = O.frame_mask(n, S, hop, ranges)
            assert got.dtype == bool and np.array_equal(got, want), (n, hop, ranges)
            assert got.any() or ranges[0][0] >= n                                      # (64, 65) of 64 samples: outside
            for context in (0, 1, 4, 40):
                regs = SM.regions(got, context)
                assert regs == O.regions(want, context), (n, hop, ranges, context)
                assert all(0 <= a < b <= got.size for a, b in regs)
                assert all(b < c for (_, b), (c, _) in zip(regs, regs[1:]))            # merged where they touch
                covered = np.zeros(got.size, bool)
                for a, b in regs:
                    covered[a:b] = True
                assert covered[got].all()
        assert not SM.frame_mask(n, S, hop, []).any() and SM.regions(SM.frame_mask(n, S, hop, []), 4) == []
    # a gap at sample 0 and one at the last sample, hop 16: frames [0, 1) and the last frame; context clipped to the file
    mask = SM.frame_mask(1000, S, 16, [(0, 1), (999, 1000)])
    assert np.flatnonzero(mask).tolist() == [0, 59] and mask.size == 60
    assert SM.regions(mask, 8) == [(0, 9), (51, 60)]
    # gaps closer than 2 x context merge, further apart they do not; exactly touching regions merge
    mask = np.zeros(100, bool)
    mask[[20, 30]] = True
    assert SM.regions(mask, 5) == [(15, 36)] and SM.regions(mask, 4) == [(16, 25), (26, 35)]
    mask[[30, 31]] = [False, True]
    assert SM.regions(mask, 5) == [(15, 37)]                                            # [15, 26) touches [26, 37)
    # hop == S: a range of one sample is one frame
    assert np.flatnonzero(SM.frame_mask(640, 64, 64, [(128, 129)])).tolist() == [2]
    assert np.flatnonzero(SM.frame_mask(640, 64, None, [(127, 129)])).tolist() == [1, 2]
    with pytest.raises(ValueError, match="context=-1"):
        SM.regions(mask, -1)


def test_parse_ranges_check_ranges_and_zero_runs():
    from rawaudiovae_kelsey_amd import smooth as SM
    assert SM.parse_ranges("1.20:1.35,4.0:4.1", 8000) == [(9600, 10800), (32000, 32800)]
    assert SM.parse_ranges("0:0.000125", 8000) == [(0, 1)]
    for text, msg in (("1.2", "range '1.2': expected START:END"), ("a:b", "range 'a:b'"), ("2:1", "range '2:1': expected 0 <= START < END"),
                      ("-1:1", "range '-1:1'"), ("1:inf", "range '1:inf'"), ("1:2,,3:4", "range ''"),
                      ("1:1.00001", "range '1:1.00001': no sample at 8000 Hz")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            SM.parse_ranges(text, 8000)
    assert SM.check_ranges([(50, 60), (0, 10), (10, 20), (55, 70), (990, 2000)], 1000).tolist() == [[0, 20], [50, 70], [990, 1000]]
    assert SM.check_ranges([(-5, 1)], 10).tolist() == [[0, 1]] and SM.check_ranges([], 10).shape == (0, 2)
    for bad, msg in (([(5, 5)], "range [5, 5) is empty"), ([(10, 12)], "range [10, 12) lies outside the 10 samples"),
                     ([(-3, 0)], "lies outside")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            SM.check_ranges(bad, 10)
    w = np.array([0, 0, 1, 0, 0, 0, 2, -0.0, 0, 3, 0], np.float32)
    assert SM.zero_runs(w, 1) == [(0, 2), (3, 6), (7, 9), (10, 11)] and SM.zero_runs(w, 2) == [(0, 2), (3, 6), (7, 9)]
    assert SM.zero_runs(w, 3) == [(3, 6)] and SM.zero_runs(w, 4) == [] and SM.zero_runs(np.zeros(5), 5) == [(0, 5)]
    with pytest.raises(ValueError, match="min_run=0"):
        SM.zero_runs(w, 0)
    assert SM.check_context(5, 16, 64, 16) == 5
    with pytest.raises(ValueError, match="context=4 frames is too short for segment_length 64, fade=16 and hop 16: it must be at least 5"):
        SM.check_context(4, 16, 64, 16)
    for bad in (0, 1e-9, 1e9, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="noise="):
            SM.check_noise(bad)
    assert SM.check_noise("0.5") == 0.5


def test_the_splice_gain_of_the_oracle():
    g = O.splice_gain(40, [(10, 12), (20, 21)], 3)
    assert (g[10:12] == 1).all() and g[20] == 1 and (g[:7] == 0).all() and (g[24:] == 0).all()
    ramp = 0.5 + 0.5 * np.cos(np.pi * np.arange(1, 4) / 4)
    assert np.allclose(g[7:10], ramp[::-1], rtol=0, atol=1e-16) and np.allclose(g[12:15], ramp, rtol=0, atol=1e-16)
    assert (np.diff(g[12:16]) < 0).all() and 0 < g[14] < g[13] < g[12] < 1
    # where ramps meet the larger wins: ranges 5 apart with a fade of 4
    g = O.splice_gain(30, [(5, 6), (11, 12)], 4)
    assert np.array_equal(g[6:11], np.maximum(O.splice_gain(30, [(5, 6)], 4), O.splice_gain(30, [(11, 12)], 4))[6:11])
    assert np.array_equal(g[6:11], g[6:11][::-1]) and (g[6:11] > 0).all()
    assert np.array_equal(O.splice_gain(9, [(0, 2), (8, 9)], 0), [1, 1, 0, 0, 0, 0, 0, 0, 1])


def test_op_codes_follow_the_header_and_the_descriptor_is_unchanged():
    from rawaudiovae_kelsey_amd import _lib
    text = open(REPO + "/include/rawvae_hip.h").read()
    codes = dict(re.findall(r"#define (RV_SMOOTH_\w+) (\d+)", text))
    assert codes == dict(RV_SMOOTH_FILTER="34", RV_SMOOTH_BACKWARD="35", RV_SMOOTH_SPLICE="36", RV_SMOOTH_WORKSPACE="37",
                         RV_SMOOTH_DENSE="0", RV_SMOOTH_DIAGONAL="1")
    assert (_lib.SMOOTH_FILTER, _lib.SMOOTH_BACKWARD, _lib.SMOOTH_SPLICE, _lib.SMOOTH_WORKSPACE) == (34, 35, 36, 37)
    assert (_lib.SMOOTH_DENSE, _lib.SMOOTH_DIAGONAL) == (0, 1)
    assert _lib.SMOOTH_WORKSPACE in _lib._HOST_ONLY_OPS
    assert not {_lib.SMOOTH_FILTER, _lib.SMOOTH_BACKWARD, _lib.SMOOTH_SPLICE} & _lib._HOST_ONLY_OPS
    para = text[text.index("/* Latent restoration"):text.index("#define RV_SMOOTH_FILTER")]
    types = {n: ctype for slot in abi_slots.header_slots() for n, ctype in slot}
    for field, ctype in (("q", "const float*"), ("weight", "const float*"), ("lam", "float"), ("centre", "double*"),
                         ("basis", "double*"), ("moment", "const double*"), ("T", "long"), ("L", "long"), ("k", "long"),
                         ("n_rows", "long"), ("row_start", "const long long*"), ("mode", "long"), ("ws", "void*"),
                         ("ws_bytes", "long"), ("result", "double*"), ("out", "float*"), ("state", "double*"), ("ldo", "long"),
                         ("src", "const float*"), ("frames", "const float*"), ("room", "const int*"), ("width", "long"),
                         ("n_out", "long")):
        assert re.search(r"\b%s\b" % field, para), field
        assert hasattr(_lib.MosaicDesc, field) and types[field] == ctype, (field, types.get(field))
    # no new member, no new role: 37 slots of 8 bytes, the earlier ops' numbers, the version, no new export
    assert len(abi_slots.check_layout()) == 37 and _lib.C.sizeof(_lib.MosaicDesc) == 37 * 8
    assert (_lib.MOSAIC_KNN, _lib.WALK_WORKSPACE, _lib.ALIGN_WORKSPACE, _lib.STRUCT_WORKSPACE) == (0, 25, 30, 33)
    assert _lib.lib().rv_version() == 100
    assert "smooth" not in " ".join(_lib.EXPORTED)
    with pytest.raises(_lib.RvError, match="unknown op 38"):
        _lib.lib().rv_mosaic(38, _lib.C.byref(_lib.MosaicDesc()), None)


def _err(op, text, **fields):
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError) as e:
        _lib.lib().rv_mosaic(op, _lib.C.byref(_lib.MosaicDesc(**fields)), None)
    assert text in str(e.value), str(e.value)


def test_workspace_query_and_every_argument_error_names_its_field():
    from rawaudiovae_kelsey_amd import _lib, smooth as SM
    up = lambda n: -(-n // 256) * 256  # noqa: E731
    for T, k in ((1, 1), (100, 17), (4096, 64), (7, 3)):
        assert SM.workspace_bytes(T, max(k, 70), k, _lib.SMOOTH_DENSE) == up(up(8 * k * k) + 8 * T * k * (k + 5))
        assert SM.workspace_bytes(T, max(k, 70), k, _lib.SMOOTH_DIAGONAL) == up(64 * T * k)
    assert SM.workspace_bytes(10, 512, 300, _lib.SMOOTH_DIAGONAL) == up(64 * 10 * 300)
    shape = dict(T=100, L=70, k=17, mode=0)
    shape_errors = ((dict(mode=2), "mode=2 is neither RV_SMOOTH_DENSE nor RV_SMOOTH_DIAGONAL"), (dict(mode=-1), "mode=-1"),
                    (dict(T=0), "T=0 outside [1, 2^31)"), (dict(T=1 << 31), "T=2147483648 outside"),
                    (dict(L=0), "L=0 outside [1, 512]"), (dict(L=513), "L=513 outside [1, 512]"),
                    (dict(k=0), "k=0 outside [1, L=70]"), (dict(k=71), "k=71 outside [1, L=70]"),
                    (dict(k=65), "k=65 exceeds the dense mode's limit of 64 axes"))
    for op, name in ((_lib.SMOOTH_WORKSPACE, "SMOOTH_WORKSPACE"), (_lib.SMOOTH_FILTER, "SMOOTH_FILTER"),
                     (_lib.SMOOTH_BACKWARD, "SMOOTH_BACKWARD")):
        for change, what in shape_errors:
            _err(op, "rv_mosaic(%s): %s" % (name, what), **dict(shape, **change))
    assert SM.workspace_bytes(100, 70, 65, _lib.SMOOTH_DIAGONAL) > 0                  # the limit is the dense mode's
    for mode in (0, 1):
        need = SM.workspace_bytes(100, 70, 17, mode)
        ok = dict(shape, mode=mode, n_rows=3, lam=1e-2, q=FAKE, row_start=FAKE, centre=FAKE, basis=FAKE, moment=FAKE,
                  ws=FAKE, ws_bytes=need, result=FAKE, out=FAKE, ldo=70)
        common = ((dict(n_rows=0), "n_rows=0 (the sequences) outside [1, T=100]"), (dict(n_rows=101), "n_rows=101"),
                  (dict(lam=0.0), "lam=0 (the observation noise r) must be finite and in [1e-8, 1e8]"),
                  (dict(lam=0.9e-8), "lam=9e-09"), (dict(lam=1.1e8), "lam=1.1e+08"), (dict(lam=-1.0), "lam=-1"),
                  (dict(lam=float("nan")), "lam=nan"), (dict(lam=float("inf")), "lam=inf"),
                  (dict(q=None), "q (the latent rows x) is null"), (dict(row_start=None), "row_start is null"),
                  (dict(centre=None), "centre is null"), (dict(moment=None), "moment (the dynamics [A^T | B^T]) is null"),
                  (dict(ws_bytes=need - 1), "ws_bytes=%d, T=100 frames of k=17 (mode=%d) need %d" % (need - 1, mode, need)),
                  (dict(ws=None), "ws is null"), (dict(ws=FAKE + 64), "ws is not 256-byte aligned"))
        for change, what in common + ((dict(basis=None), "basis (P) is null"),
                                      (dict(ldo=18), "ldo=18 holds no row of k + 2 = 19 values")):
            _err(_lib.SMOOTH_FILTER, "rv_mosaic(SMOOTH_FILTER): " + what, **dict(ok, **change))
        for change, what in common + ((dict(basis=None), "basis (R) is null"), (dict(out=None), "out is null"),
                                      (dict(ldo=69), "ldo=69 holds no row of L=70 values")):
            _err(_lib.SMOOTH_BACKWARD, "rv_mosaic(SMOOTH_BACKWARD): " + what, **dict(ok, **change))
    ok = dict(src=FAKE, frames=FAKE, room=FAKE, out=FAKE, n_rows=2, width=64, n_out=1000)
    for change, what in ((dict(n_out=0), "n_out=0 outside [1, 2^31)"), (dict(n_out=1 << 31), "n_out=2147483648 outside [1, 2^31)"),
                         (dict(n_rows=0), "n_rows=0 (the ranges) outside"), (dict(width=-1), "width=-1 (the fade) outside"),
                         (dict(src=None), "src is null"), (dict(frames=None), "frames is null"),
                         (dict(room=None), "room (the ranges) is null"), (dict(out=None), "out is null")):
        _err(_lib.SMOOTH_SPLICE, "rv_mosaic(SMOOTH_SPLICE): " + what, **dict(ok, **change))


def _cpu_walk(k, L, diagonal=False):
    from rawaudiovae_kelsey_amd import walk as W
    m = O.model(k, L, diagonal)
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))  # noqa: E731
    return W.LatentWalk(k, "diagonal" if diagonal else "full")._set(
        t(m["centre"]), t(m["V"]), t(m["lam"]), t(np.stack([m["A"].T, m["B"].T])), t(m["P"]), t(m["R"]), m["rank"], 300, 1)


def test_python_argument_checks_without_a_device():
    from rawaudiovae_kelsey_amd import smooth as SM, walk as W
    with pytest.raises(TypeError, match="fitted LatentWalk"):
        SM.LatentSmoother(object())
    with pytest.raises(RuntimeError, match="has not been fitted"):
        SM.LatentSmoother(W.LatentWalk(3))
    with pytest.raises(ValueError, match=r"keeps 70 axes in full mode .* at most 64: refit with --keep <= 64 or --mode diagonal"):
        SM.LatentSmoother(_cpu_walk(70, 70))
    assert SM.LatentSmoother(_cpu_walk(70, 70, True)).mode == 1
    sm = SM.LatentSmoother(_cpu_walk(17, 70), 0.5)
    assert (sm.k, sm.L, sm.mode, sm.noise) == (17, 70, 0, 0.5)
    with pytest.raises(ValueError, match="noise=0 must be finite"):
        SM.LatentSmoother(_cpu_walk(17, 70), 0)
    with pytest.raises(ValueError, match="2-D float32 device tensor"):
        sm.filter(torch.zeros(4, 70), [0, 4])
    with pytest.raises(ValueError, match="ranges must be at least one"):
        SM.splice(torch.zeros(8), torch.zeros(8), [(4, 2)], 1)
    with pytest.raises(ValueError, match="ranges must be at least one"):
        SM.splice(torch.zeros(8), torch.zeros(8), [(0, 4), (3, 6)], 1)
    with pytest.raises(ValueError, match="fade=-1"):
        SM.splice(torch.zeros(8), torch.zeros(8), [(0, 4)], -1)


def test_restore_py_parser_errors():
    sys.path.insert(0, REPO)
    import restore as cli
    base = ["--checkpoint", "c", "--walk", "w.npz", "--in", "a.wav", "--out", "o.wav"]
    args = cli.parse_args(["fill"] + base + ["--hop", "256", "--window", "hann", "--gaps", "1.2:1.35", "--noise", "1e-3",
                                             "--context", "40", "--fade", "0"])
    assert (args.command, args.hop, args.window, args.gaps, args.noise, args.context, args.fade) == (
        "fill", 256, "hann", "1.2:1.35", 1e-3, 40, 0)
    args = cli.parse_args(["fill"] + base + ["--detect-zeros", "64"])
    assert (args.detect_zeros, args.gaps, args.gaps_json, args.noise, args.context, args.fade, args.window) == (
        64, None, None, 1e-2, 32, 64, None)
    assert cli.parse_args(["smooth"] + base).noise == 0.5
    args = cli.parse_args(["surprise"] + base + ["--threshold", "6"])
    assert (args.command, args.threshold, args.noise, args.wav, args.out) == ("surprise", 6.0, 1e-2, "a.wav", "o.wav")
    fill = ["fill"] + base
    for argv, msg in ((fill, "expected exactly one of --gaps, --gaps-json and --detect-zeros, got none"),
                      (fill + ["--gaps", "1:2", "--detect-zeros", "4"], "exactly one of --gaps, --gaps-json and --detect-zeros, got --gaps, --detect-zeros"),
                      (fill + ["--detect-zeros", "0"], "--detect-zeros '0'"), (fill + ["--gaps", "1:2", "--hop", "0"], "--hop '0'"),
                      (fill + ["--gaps", "1:2", "--noise", "0"], "--noise '0': expected a finite number in [1e-8, 1e8]"),
                      (fill + ["--gaps", "1:2", "--noise", "nan"], "--noise 'nan'"), (fill + ["--gaps", "1:2", "--noise", "x"], "--noise 'x'"),
                      (fill + ["--gaps", "1:2", "--context", "0"], "--context '0'"), (fill + ["--gaps", "1:2", "--fade", "-1"], "--fade '-1'"),
                      (fill + ["--gaps", "1:2", "--window", "hamming"], "--window 'hamming'"),
                      (["smooth"] + base + ["--noise", "1e9"], "--noise '1e9'"),
                      (["surprise"] + base + ["--threshold", "-1"], "--threshold '-1'"), ([], "expected a command: fill, smooth or surprise")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            cli.parse_args(argv)
    with pytest.raises(SystemExit):
        cli.parse_args(["fill", "--checkpoint", "c", "--in", "a.wav", "--out", "o.wav", "--gaps", "1:2"])       # no --walk
    with pytest.raises(SystemExit):
        cli.parse_args(["smooth"] + base + ["--gaps", "1:2"])                                                   # fill's flag
    # the gaps of a fill: parsed, read from JSON, detected; each error names its flag
    args = cli.parse_args(fill + ["--gaps", "0.5:0.25"])
    with pytest.raises(ValueError, match=re.escape("--gaps: range '0.5:0.25'")):
        cli.gap_ranges(args, np.zeros(10), 8000)
    wave = np.ones(400, np.float32)
    wave[100:180] = 0
    assert cli.gap_ranges(cli.parse_args(fill + ["--detect-zeros", "64"]), wave, 8000) == [(100, 180)]
    with pytest.raises(ValueError, match="--detect-zeros 81: 'a.wav' holds no run of 81 zero samples"):
        cli.gap_ranges(cli.parse_args(fill + ["--detect-zeros", "81"]), wave, 8000)
    with pytest.raises(ValueError, match="--gaps-json 'nowhere.json'"):
        cli.gap_ranges(cli.parse_args(fill + ["--gaps-json", "nowhere.json"]), wave, 8000)
