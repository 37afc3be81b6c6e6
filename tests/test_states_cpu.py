"""Latent states without a GPU: the oracle against itself (tests/states_oracle.py: its fma against exact rationals, its
Viterbi against every path, its scaled recursion against the log-domain one in longdouble, which is where the gates of
tests/test_states_gpu.py come from, and its fit on the planted data), the op codes and descriptor roles, every argument
check of the five ops (they run before anything is launched), and the host side of rawaudiovae_kelsey_amd/states.py and
states.py: argument checks, the .npz round trip, the hop check and the segments file that segment.py split reads."""
import ctypes as C
import itertools
import json
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import states_oracle as O  # noqa: E402

sys.path.insert(0, REPO)


def test_fma_is_the_correctly_rounded_one():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(1500), rng.standard_normal(1500)
    c = -(a * b) * (1 + rng.choice([0, 1e-16, 1e-9, 1.0], 1500))      # cancellation down to the product's last bits
    got = O.fma(a, b, c)
    want = [float(Fraction(float(p)) * Fraction(float(q)) + Fraction(float(r))) for p, q, r in zip(a, b, c)]
    assert np.array_equal(got, np.array(want))
    assert np.isnan(O.fma(np.nan, 1.0, 1.0)) and O.fma(np.inf, 1.0, 1.0) == np.inf and O.fma(2.0, 3.0, -np.inf) == -np.inf


def test_viterbi_takes_the_best_of_every_path_and_the_lower_state_on_ties():
    S, k, T = 3, 1, 5
    rng = np.random.default_rng(3)
    for trial in range(20):
        th = O.random_theta(S, k, trial)
        o = O.layout(S, k)
        th[o["logpi"]] = rng.integers(-2, 2, S)
        la = rng.integers(-2, 2, (S, S)).astype(np.float64)
        la[rng.uniform(size=(S, S)) < 0.3] = -np.inf
        th[o["logA"]] = la.ravel()
        logb = rng.integers(-2, 2, (T, S)).astype(np.float64)
        path, score = O.viterbi(logb, [0, T], th, S, k)
        with np.errstate(all="ignore"):
            best = max(th[o["logpi"]][p[0]] + logb[0, p[0]] + sum(la[p[t - 1], p[t]] + logb[t, p[t]] for t in range(1, T))
                       for p in itertools.product(range(S), repeat=T))
        assert score[0] == best
        if np.isfinite(best):
            p = path
            assert best == th[o["logpi"]][p[0]] + logb[0, p[0]] + sum(la[p[t - 1], p[t]] + logb[t, p[t]] for t in range(1, T))
        else:
            assert (path == -1).all()
    # ties: everything equal, so state 0 throughout; an unobserved frame adds nothing
    th = O.pack(np.zeros((S, k)), np.ones((S, k)), np.full(S, 1 / 3), np.full((S, S), 1 / 3))
    logb = np.zeros((4, S))
    logb[2] = np.nan
    path, score = O.viterbi(logb, [0, 0, 4], th, S, k)
    assert path.tolist() == [0, 0, 0, 0] and score[0] == 0 and score[1] == np.log(1 / 3) * 4


@pytest.mark.parametrize("S", O.GATED_STATES)
def test_gates_hold_on_the_cpu(S):
    """The float64 recursion against the longdouble one at the GPU test's shapes: within the measured distances the gates
    are 4 times of (a quarter of each gate, and half again for another libm)."""
    for outlier in (False, True):
        logb, rs, th, k = O.gated_case(S, outlier)
        gamma, xi, ll, scale = O.forward_backward(logb, rs, th, S, k)
        dg, dx, dl = O.gated_distances((gamma, xi, ll), S, outlier)
        print("S %d outlier %d: gamma %.3g xi %.3g ll %.3g" % (S, outlier, dg, dx, dl))
        assert dg <= 1.5 * O.GATE_GAMMA / 4 and dx <= 1.5 * O.GATE_XI / 4 and dl <= 1.5 * O.GATE_LL / 4
        assert np.abs(gamma.sum(axis=1) - 1).max() < 1e-13
        pairs = np.maximum(0, np.diff(rs) - 1)
        assert np.abs(xi.sum(axis=(1, 2)) - pairs).max() < 1e-11 and (xi[pairs == 0] == 0).all()
        assert np.isnan(logb).any() == outlier


@pytest.mark.parametrize("S,k", O.MSTEP_SHAPES)
def test_mstep_oracle_and_its_log_gates(S, k):
    x, c, P, gamma, xi, rs, th = O.mstep_case(S, k)
    res = O.mstep(x, c, P, gamma, xi, rs, th, S, k, 1e-3)
    p, old = O.unpack(res["theta"], S, k), O.unpack(th, S, k)
    dg, dpi, da = O.mstep_distances(res["theta"], res, S, k)
    print("S %d k %d: dead %d, g %.3g log pi %.3g log A %.3g" % (S, k, res["info"].sum(), dg, dpi, da))
    assert dg <= 1.5 * O.GATE_G / 4 and max(dpi, da) <= 1.5 * O.GATE_LOG_A / 4
    dead = res["info"] == 1
    assert dead.any() and np.array_equal(dead, ~(res["N"] >= 1))
    assert np.array_equal(p["m"][dead], old["m"][dead]) and np.array_equal(p["w"][dead], old["w"][dead])
    assert np.array_equal(p["g"][dead], old["g"][dead])
    # against plain numpy sums: the same numbers up to rounding
    y, obs = O.whiten(x, c, P), O.observed(x)
    assert not obs.all()
    gn = gamma * obs[:, None]
    assert np.allclose(res["N"], gn.sum(0), rtol=1e-12) and np.allclose(res["M1"], gn.T @ y, rtol=0, atol=1e-10)
    assert np.allclose(res["M2"], gn.T @ (y * y), rtol=0, atol=1e-9)
    assert np.array_equal(p["A"][S - 1], old["A"][S - 1]) and np.isneginf(p["logA"]).any()
    live = ~dead
    assert np.allclose(p["A"].sum(axis=1), 1) and abs(p["pi"].sum() - 1) < 1e-12
    assert (1 / p["w"][live] >= np.float64(np.float32(1e-3))).all()


def test_the_oracles_fit_recovers_the_planted_states():
    """The end-to-end conditions on the oracle alone, at the seed the GPU test fits with."""
    x, rs, labels, c, P = O.planted()
    S, k = O.PLANT["S"], O.PLANT["k"]
    th, hist, scales = O.planted_fit()
    drop = np.diff(hist) / scales[1:]
    path, _ = O.viterbi(O.emit(x, c, P, th, S, k), rs, th, S, k)
    agree = O.agreement(path, labels, S)
    print("ll %.6f -> %.6f, least step %.3g of its scale, agreement %.4f" % (hist[0], hist[-1], drop.min(), agree))
    assert (drop >= -O.GATE_LL).all() and agree >= 0.99


def test_op_codes_roles_and_limits():
    from rawaudiovae_kelsey_amd import _lib
    text = open(REPO + "/include/rawvae_hip.h").read()
    codes = dict(re.findall(r"#define (RV_HMM_\w+) (\d+)", text))
    assert codes == dict(RV_HMM_EMIT="43", RV_HMM_FORWARD_BACKWARD="44", RV_HMM_MSTEP="45", RV_HMM_VITERBI="46",
                         RV_HMM_WORKSPACE="47", RV_HMM_MOMENTS="1")
    assert (_lib.HMM_EMIT, _lib.HMM_FORWARD_BACKWARD, _lib.HMM_MSTEP, _lib.HMM_VITERBI, _lib.HMM_WORKSPACE) == (43, 44, 45, 46, 47)
    assert _lib.HMM_MOMENTS == 1
    assert _lib.HMM_WORKSPACE in _lib._HOST_ONLY_OPS and _lib.HMM_EMIT not in _lib._HOST_ONLY_OPS
    para = text[text.index("/* Latent states"):text.index("#define RV_HMM_EMIT")]
    types = {n: ctype for slot in abi_slots.header_slots() for n, ctype in slot}
    for field, ctype in (("moment", "const double*"), ("result", "double*"), ("state", "double*"), ("info", "int*"),
                         ("path", "int*"), ("score", "double*"), ("centre", "double*"), ("basis", "double*"), ("q", "const float*"),
                         ("S", "long"), ("k", "long"), ("L", "long"), ("T", "long"), ("stride", "long"), ("n_rows", "long"),
                         ("lam", "float"), ("mode", "long"), ("ws_bytes", "long")):
        assert re.search(r"\b%s\b" % field, para), field
        assert hasattr(_lib.MosaicDesc, field) and types[field] == ctype, (field, types.get(field))
    assert len(abi_slots.check_layout()) == 37 and C.sizeof(_lib.MosaicDesc) == 37 * 8
    assert _lib.lib().rv_version() == 100 and "hmm" not in " ".join(_lib.EXPORTED)
    for op in (42, 48):
        with pytest.raises(_lib.RvError, match="unknown op %d" % op):
            _lib.lib().rv_mosaic(op, C.byref(_lib.MosaicDesc()), None)
    d = _lib.mosaic_call(_lib.HMM_WORKSPACE, T=5000, S=17, k=33)
    up = lambda n: -(-n // 256) * 256   # noqa: E731
    fb = up(5000 * 17 * 8) + up(5000 * 8)
    ms = up(5000 * 33 * 8) + up(5000) + up(20 * 17 * 8) + 2 * 2 * 64 * 64 * 8
    assert d.ws_bytes == max(fb, ms, up(5000 * 17))


def _err(op, text, **fields):
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError) as e:
        _lib.lib().rv_mosaic(op, C.byref(_lib.MosaicDesc(**fields)), None)
    assert text in str(e.value), str(e.value)


def test_every_op_names_the_offending_field_before_it_launches():
    from rawaudiovae_kelsey_amd import _lib
    p = 0x1000     # never dereferenced: every call here fails a check
    rows = dict(T=10, S=3, k=2, L=4, stride=4, q=p, centre=p, basis=p)
    emit = dict(rows, moment=p, result=p)
    seqs = dict(T=10, S=3, k=2, n_rows=2, row_start=p, ws=p, ws_bytes=1 << 20, moment=p, result=p)
    fb = dict(seqs, state=p)
    vit = dict(seqs, path=p, score=p)
    ms = dict(rows, n_rows=2, row_start=p, ws=p, ws_bytes=1 << 20, moment=p, state=p, lam=1e-3, result=2 * p, info=p)
    ops = (("HMM_EMIT", _lib.HMM_EMIT, emit), ("HMM_FORWARD_BACKWARD", _lib.HMM_FORWARD_BACKWARD, fb),
           ("HMM_VITERBI", _lib.HMM_VITERBI, vit), ("HMM_MSTEP", _lib.HMM_MSTEP, ms),
           ("HMM_WORKSPACE", _lib.HMM_WORKSPACE, dict(T=10, S=3, k=2)))
    for name, op, ok in ops:
        for change, text in ((dict(T=0), "T=0 outside [1, 2^31)"), (dict(T=1 << 31), "T=2147483648 outside [1, 2^31)"),
                             (dict(S=0), "S=0 (the states) outside [1, 64]"), (dict(S=65), "S=65 (the states) outside [1, 64]"),
                             (dict(k=0), "k=0 (the axes) outside [1, 64]"), (dict(k=65), "k=65 (the axes) outside [1, 64]")):
            _err(op, "rv_mosaic(%s): %s" % (name, text), **dict(ok, **change))
    for name, op, ok in (ops[0], ops[3]):
        for change, text in ((dict(L=1), "L=1 outside [k=2, 512]"), (dict(L=513, stride=513), "L=513 outside [k=2, 512]"),
                             (dict(stride=3), "stride=3 (the row pitch of x) holds no row of L=4 values"),
                             (dict(q=None), "q (the latent rows x) is null"), (dict(centre=None), "centre is null"),
                             (dict(basis=None), "basis (P) is null")):
            _err(op, "rv_mosaic(%s): %s" % (name, text), **dict(ok, **change))
    for name, op, ok in ops[1:4]:
        for change, text in ((dict(n_rows=0), "n_rows=0 (the sequences) outside [1, 2^31)"), (dict(row_start=None), "row_start is null"),
                             (dict(ws_bytes=8), "ws_bytes=8, T=10 frames of S=3 states and k=2 axes need"),
                             (dict(ws=None), "ws is null, T=10 frames"), (dict(ws=p + 8), "ws is not 256-byte aligned"),
                             (dict(moment=None), "moment (")):
            _err(op, "rv_mosaic(%s): %s" % (name, text), **dict(ok, **change))
    for name, op, ok, outs in (("HMM_EMIT", _lib.HMM_EMIT, emit, ("moment", "result")),
                               ("HMM_FORWARD_BACKWARD", _lib.HMM_FORWARD_BACKWARD, fb, ("result", "state")),
                               ("HMM_VITERBI", _lib.HMM_VITERBI, vit, ("result", "path", "score")),
                               ("HMM_MSTEP", _lib.HMM_MSTEP, ms, ("state", "result", "info"))):
        for field in outs:
            _err(op, "rv_mosaic(%s): %s" % (name, field), **dict(ok, **{field: None}))
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        _err(_lib.HMM_MSTEP, "(the variance floor) must be finite and positive", **dict(ms, lam=lam))
    _err(_lib.HMM_MSTEP, "result and moment are the same block", **dict(ms, result=p))
    _err(_lib.HMM_MSTEP, "mode=2 is neither 0 nor RV_HMM_MOMENTS", **dict(ms, mode=2))


def test_latent_states_checks_its_arguments():
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd.corpus import check_row_start
    for bad in (0, 65, 2.0, True, None):
        with pytest.raises(ValueError, match="n_states=.* must be an integer in \\[1, 64\\]"):
            ST.LatentStates(bad, 4)
        with pytest.raises(ValueError, match="n_components=.* must be an integer in \\[1, 64\\]"):
            ST.LatentStates(3, bad)
    for bad in (0, -1e-3, float("nan"), float("inf"), "x", 1e-60):
        with pytest.raises(ValueError, match="var_floor=.* must be a finite positive number"):
            ST.LatentStates(3, 4, bad)
    st = ST.LatentStates(5, 2)
    with pytest.raises(RuntimeError, match="has not been fitted"):
        st.means_
    with pytest.raises(ValueError, match="4 frames are fewer than the 5 states"):
        st.fit(torch.zeros(4, 8), [0, 4], (np.zeros(8), np.eye(8)[:2]), 3, 0, 0)
    with pytest.raises(ValueError, match="x must be a 2-D float32 device tensor"):
        st.fit(torch.zeros(9, 8), [0, 9], (np.zeros(8), np.eye(8)[:2]), 3, 0, 0)
    for rs, text in (([0, 5, 3, 9], "must not descend: file 1 is \\[5, 3\\)"), ([1, 9], "must run from 0 to T=9"),
                     ([0, 8], "must run from 0 to T=9"), ([0.0, 9.0], "1-D integer sequence"), ([9], "1-D integer sequence")):
        with pytest.raises(ValueError, match=text):
            check_row_start(rs, 9, empty_files=True)
    assert check_row_start([0, 0, 4, 4, 9], 9, empty_files=True).tolist() == [0, 0, 4, 4, 9]       # empty files are legal
    with pytest.raises(TypeError, match="expected a fitted LatentPCA, a fitted LatentWalk or a \\(centre, P\\) pair"):
        ST.whitening("pca.npz", 2)
    with pytest.raises(ValueError, match="n_components=3: the basis holds P \\(2, 8\\)"):
        ST.whitening((np.zeros(8), np.eye(8)[:2]), 3)
    offsets, labels = ST.runs([2, 2, 0, 0, 0, 2])
    assert offsets.tolist() == [0, 2, 5, 6] and labels.tolist() == [2, 0, 2]
    assert [a.tolist() for a in ST.runs([1])] == [[0, 1], [1]]


def _fitted(S=3, k=2, L=5):
    from rawaudiovae_kelsey_amd import states as ST
    th = O.random_theta(S, k, zeros=True)
    c, P = O.basis(k, L)
    return ST.LatentStates(S, k, 2e-3)._set(torch.from_numpy(th.copy()), torch.from_numpy(c.copy()), torch.from_numpy(P.copy()),
                                            1200, 3, [-10.5, -9.25]), th


def test_npz_round_trip_and_the_hop_check(tmp_path):
    import states as cli
    from rawaudiovae_kelsey_amd import corpus as C_
    from rawaudiovae_kelsey_amd import states as ST
    st, th = _fitted()
    p = O.unpack(th, 3, 2)
    assert np.array_equal(st.means_, p["m"]) and np.array_equal(st.variances_, 1 / p["w"])
    assert np.array_equal(st.startprob_, p["pi"]) and np.array_equal(st.transmat_, p["A"])
    assert np.array_equal(st.durations_, 1 / (1 - np.diag(p["A"])))
    path = str(tmp_path / "states.npz")
    ST.write_states(path, st, 64, 16)
    back, meta = ST.read_states(path, "cpu")
    assert meta == dict(segment_length=64, latent_dim=5, hop=16, n_frames=1200, n_files=3, n_iter=2)
    assert (back.n_states, back.n_components, back.var_floor, back.ll_history_) == (3, 2, 2e-3, [-10.5, -9.25])
    for a, b in ((back.theta_, st.theta_), (back.mean_, st.mean_), (back.P_, st.P_)):
        assert a.dtype == torch.float64 and torch.equal(a, b)
    ST.write_states(path, st, 64)
    assert ST.read_states(path, "cpu")[1]["hop"] is None
    check_hop = lambda *a: C_.check_hop(*a, *cli.HOP_PHRASES)     # noqa: E731
    assert check_hop(16, 16, 64) == 16 and check_hop(None, None, 64) == 64 and check_hop(None, 64, 64) == 64
    with pytest.raises(ValueError, match="hop 32: the states were fitted at hop 16"):
        check_hop(16, 32, 64)
    with pytest.raises(ValueError, match="hop 64: the states were fitted at hop 16"):
        check_hop(16, None, 64)
    with np.load(path) as z:
        arrays = {n: z[n] for n in z.files}
    np.savez(path, **{n: v for n, v in arrays.items() if n != "whiten"})
    with pytest.raises(ValueError, match="not a latent-states file, it lacks whiten"):
        ST.read_states(path, "cpu")
    np.savez(path, **dict(arrays, theta=arrays["theta"][:-1]))
    with pytest.raises(ValueError, match="do not fit 3 states, 2 components and latent_dim 5"):
        ST.read_states(path, "cpu")


def test_the_segments_of_label_are_what_segment_py_split_reads(tmp_path):
    import segment
    import states as cli
    from rawaudiovae_kelsey_amd import data as D
    sr, step = 8000, 16
    wave = np.random.default_rng(5).uniform(-0.5, 0.5, 16 * 40 + 7).astype(np.float32)
    path = np.repeat([2, 0, 2, 1], [7, 20, 3, 8])          # 38 frames of 64 samples at hop 16
    rep = cli.segments_report(path, -123.5, wave.size, sr, step, 3)
    assert rep["labels"] == [2, 0, 2, 1] and rep["form"] == "C A C B" and rep["segments"] == 4 and rep["states"] == 3
    assert rep["boundary_frames"] == [7, 27, 30] and rep["sample_offsets"] == [0, 112, 432, 480, wave.size]
    assert rep["boundary_seconds"] == [112 / sr, 432 / sr, 480 / sr] and rep["score"] == -123.5
    find_keys = {"segments", "frames", "samples", "sampling_rate", "hop", "boundary_frames", "boundary_samples",
                 "boundary_seconds", "sample_offsets", "labels", "form"}
    assert find_keys <= set(rep)
    D.write_wav(tmp_path / "in.wav", wave, sr)
    (tmp_path / "seg.json").write_text(json.dumps(rep))
    names = segment.main(["split", "--segments", str(tmp_path / "seg.json"), "--in", str(tmp_path / "in.wav"),
                          "--out-dir", str(tmp_path / "cut")])
    assert [n.rsplit("/", 1)[1] for n in names] == ["seg_000_C.wav", "seg_001_A.wav", "seg_002_C.wav", "seg_003_B.wav"]
    parts = [D.load_audio_mono(n, sr) for n in names]
    assert np.array_equal(np.concatenate(parts), D.load_audio_mono(tmp_path / "in.wav", sr))
    one = cli.segments_report(np.zeros(5, np.int32), 0.0, 100, sr, step, 2)
    assert one["labels"] == [0] and one["sample_offsets"] == [0, 100] and one["boundary_frames"] == []


def test_states_py_names_the_bad_flag():
    import states as cli
    fit = ["fit", "--checkpoint", "c", "--data", "d", "--out", "o"]
    for extra, text in ((["--states", "0"], "--states '0': expected a positive integer"),
                        (["--states", "65"], "--states 65: at most 64"), (["--keep", "65"], "--keep 65: at most 64"),
                        (["--keep", "x"], "--keep 'x'"), (["--hop", "0"], "--hop '0'"), (["--iters", "0"], "--iters '0'"),
                        (["--tol", "-1"], "--tol '-1': expected a finite number >= 0"),
                        (["--floor", "0"], "--floor '0': expected a finite number > 0"), (["--seed", "-1"], "--seed '-1'")):
        with pytest.raises(ValueError) as e:
            cli.parse_args(fit + extra)
        assert text in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="expected a command: fit, label or score"):
        cli.parse_args([])
    a = cli.parse_args(fit + ["--states", "5", "--keep", "3", "--hop", "16", "--tol", "0"])
    assert (a.states, a.keep, a.hop, a.tol, a.iters, a.floor, a.seed, a.pca) == (5, 3, 16, 0.0, 50, 1e-3, 0, None)
    a = cli.parse_args(["label", "--checkpoint", "c", "--states", "s.npz", "--in", "a.wav", "--out", "o.json"])
    assert (a.states, a.wav, a.out, a.hop) == ("s.npz", "a.wav", "o.json", None)
    with pytest.raises(ValueError, match="--states 'none.npz': no such file"):
        cli.main(["score", "--checkpoint", "c", "--states", "none.npz", "--in", "a.wav"])
