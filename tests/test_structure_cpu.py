"""The structure rules without a device: the numpy oracle (tests/structure_oracle.py) against a brute-force triple loop
written on its own, planted boundaries recovered exactly, the properties of the peak rule, the header's op codes and
field names, the library's argument checks (all made on the host), the label rule and segment.py's parser."""
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import align_oracle as AO  # noqa: E402
import structure_oracle as O  # noqa: E402

FAKE = 0x7000_0000_0000      # a non-null, 256-byte aligned address no check dereferences


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _brute_novelty(full, R, w):
    """The header's rule term by term, sharing nothing with the oracle."""
    T = full.shape[0]
    out = []
    for t in range(T):
        Cross = Wc = Within = Ww = 0.0
        for u in range(-R, R):
            cross = wc = within = ww = 0.0
            for v in range(-R, R):
                i, j = t + u, t + v
                if i < 0 or i >= T or j < 0 or j >= T:
                    continue
                c = float(w[u + R]) * float(w[v + R])
                d = float(full[i, j])
                if (u < 0) != (v < 0):
                    cross, wc = cross + c * d, wc + c
                else:
                    within, ww = within + c * d, ww + c
            Cross, Wc, Within, Ww = Cross + cross, Wc + wc, Within + within, Ww + ww
        out.append(Cross / Wc - Within / Ww if Wc > 0 and Ww > 0 else 0.0)
    return np.array(out)


@pytest.mark.parametrize("R", [1, 2, 3])
def test_the_oracle_equals_a_brute_force_triple_loop(R):
    for T in range(1, 13):
        for sigma in (None, 0.5):
            mu = AO.random_latents(T, 3, 10 * T + R)
            _, full = AO.local_costs(mu, mu, 0)
            w = O.taper(R, sigma)
            got, want = O.novelty(full, R, w), _brute_novelty(full, R, w)
            assert np.array_equal(_bits(got), _bits(want)), (T, R, sigma)
            assert got[0] == 0.0 and not np.signbit(got[0])                     # no past
            # the band's +inf slots are never read: the banded matrix gives the same bits
            r = 2 * R - 1
            _, banded_full = AO.local_costs(mu, mu, r)
            assert np.array_equal(_bits(O.novelty(banded_full, R, w)), _bits(want))
            # a NaN row: exactly the frames whose window holds it
            bad = mu.copy()
            row = T // 2
            bad[row] = np.nan
            _, fb = AO.local_costs(bad, bad, 0)
            nb = O.novelty(fb, R, w)
            hit = np.array([t >= 1 and t - R <= row < t + R for t in range(T)])   # frame 0 has no past: +0
            assert np.array_equal(np.isnan(nb), hit), (T, R)
            assert np.array_equal(_bits(nb[~hit]), _bits(got[~hit]))
            assert np.array_equal(_bits(nb), _bits(_brute_novelty(fb, R, w)))


@pytest.mark.parametrize("R", [4, 8])
def test_planted_boundaries_are_recovered_exactly(R):
    mu, starts = O.planted()
    assert mu.shape == (140, 8) and starts == [23, 41, 80, 97]
    for r in (0, 2 * R - 1):
        _, full = AO.local_costs(mu, mu, r)
        nov = O.novelty(full, R, O.taper(R, 0.5))
        path, summary = O.peaks(nov, 8, 16, 0.5)
        assert summary.tolist() == [5, 140, 0, 0]
        assert path[:6].tolist() == [0, 23, 41, 80, 97, 140] and (path[6:] == -1).all()


def test_peaks_of_a_constant_signal_ties_nan_and_the_gap():
    # a constant signal: every distance 0, nov == 0, one segment
    mu = np.ones((40, 3), np.float32)
    _, full = AO.local_costs(mu, mu, 0)
    nov = O.novelty(full, 4, O.taper(4, 0.5))
    assert (nov == 0).all() and not np.signbit(nov).any()
    path, summary = O.peaks(nov, 4, 8, 0.0)
    assert summary.tolist() == [1, 40, 0, 0] and path[:2].tolist() == [0, 40] and (path[2:] == -1).all()
    # ties go to the earlier frame
    curve = np.zeros(30)
    curve[[10, 11, 12, 20]] = 1.0
    path, summary = O.peaks(curve, 3, 30, 0.0)
    assert path[:summary[0] + 1].tolist() == [0, 10, 20, 30]
    path, summary = O.peaks(curve, 1, 30, 0.0)
    assert path[:summary[0] + 1].tolist() == [0, 10, 20, 30]              # 11 loses to 10 and 12 to 11: a plateau's first
    path, summary = O.peaks(curve, 0, 30, 0.0)
    assert path[:summary[0] + 1].tolist() == [0, 10, 11, 12, 20, 30]      # no gap: every frame above the threshold
    # NaN is never a boundary and never suppresses a neighbour
    curve = np.zeros(30)
    curve[[10, 20]] = 1.0
    withnan = curve.copy()
    withnan[[9, 11, 21]] = np.nan
    p0, s0 = O.peaks(curve, 3, 30, 0.0)
    p1, s1 = O.peaks(withnan, 3, 30, 0.0)
    assert p1[:s1[0] + 1].tolist() == p0[:s0[0] + 1].tolist() == [0, 10, 20, 30] and s1.tolist() == [3, 27, 0, 0]
    assert O.peaks(np.full(12, np.nan), 2, 4, 0.0)[1].tolist() == [1, 0, 0, 0]
    # the minimum gap, and non-empty first and last segments, on random curves
    rs = np.random.RandomState(3)
    for T, g, m, delta in ((1, 0, 0, 0.0), (2, 0, 0, 0.0), (2, 1, 1, 0.0), (50, 0, 3, 0.0), (300, 1, 16, 0.5),
                           (300, 8, 16, 0.0), (300, 8, 0, 0.5), (40, 60, 5, 0.0)):
        for kind in ("random", "binary"):
            curve = rs.randn(T) if kind == "random" else rs.randint(0, 2, T).astype(np.float64)
            path, summary = O.peaks(curve, g, m, delta)
            F = int(summary[0])
            off = path[:F + 1]
            assert F >= 1 and off[0] == 0 and off[-1] == T and (path[F + 1:] == -1).all() and path.shape == (T + 1,)
            assert (np.diff(off) >= 1).all()
            assert (np.diff(off[1:-1]) > g).all()
            if F > 1:
                assert off[1] >= max(g, 1) and off[-2] <= T - max(g, 1)
            if g >= T:
                assert F == 1
            if m == 0 and delta > 0:
                assert F == 1 or (np.abs(curve).mean() == 0)    # nothing exceeds itself plus a positive margin


def test_op_codes_and_field_names_follow_the_header():
    from rawaudiovae_kelsey_amd import _lib
    text = open(REPO + "/include/rawvae_hip.h").read()
    codes = dict(re.findall(r"#define (RV_STRUCT_\w+) (\d+)", text))
    assert codes == dict(RV_STRUCT_NOVELTY="31", RV_STRUCT_PEAKS="32", RV_STRUCT_WORKSPACE="33")
    assert (_lib.STRUCT_NOVELTY, _lib.STRUCT_PEAKS, _lib.STRUCT_WORKSPACE) == (31, 32, 33)
    assert _lib.STRUCT_WORKSPACE in _lib._HOST_ONLY_OPS and _lib.STRUCT_PEAKS not in _lib._HOST_ONLY_OPS
    para = text[text.index("/* Latent structure"):text.index("#define RV_STRUCT_NOVELTY")]
    types = {n: ctype for slot in abi_slots.header_slots() for n, ctype in slot}
    for field, ctype in (("T", "long"), ("local_costs", "float*"), ("band", "long"), ("k", "long"), ("moment", "const double*"),
                         ("result", "double*"), ("lag", "long"), ("width", "long"), ("lam", "float"), ("ws", "void*"),
                         ("ws_bytes", "long"), ("path", "int*"), ("summary", "int*")):
        assert re.search(r"\b%s\b" % field, para), field
        assert hasattr(_lib.MosaicDesc, field) and types[field] == ctype, (field, types.get(field))
    # the ops before them keep their numbers, the descriptor its 37 eight-byte slots, the library its version
    assert (_lib.MOSAIC_KNN, _lib.EVAL_DIMS, _lib.WALK_WORKSPACE, _lib.ALIGN_WORKSPACE) == (0, 17, 25, 30)
    assert len(abi_slots.check_layout()) == 37 and _lib.C.sizeof(_lib.MosaicDesc) == 37 * 8
    assert _lib.lib().rv_version() == 100
    assert "rv_struct" not in " ".join(_lib.EXPORTED)                       # no new export


def _err(op, text, **fields):
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError) as e:
        _lib.lib().rv_mosaic(op, _lib.C.byref(_lib.MosaicDesc(**fields)), None)
    assert text in str(e.value), str(e.value)


def test_workspace_query_and_every_argument_error_names_its_field():
    from rawaudiovae_kelsey_amd import _lib, structure as S
    up = lambda n: -(-n // 256) * 256  # noqa: E731
    for T in (1, 256, 257, 5000):
        nb = -(-T // 256)
        assert S.workspace_bytes(T) == up(8 * nb) + 3 * up(4 * nb) + 256 + up(4 * T)
    for T, what in ((0, "T=0 outside"), (-3, "T=-3 outside"), ((1 << 31) - 1, "T=2147483647 outside")):
        _err(_lib.STRUCT_WORKSPACE, "rv_mosaic(STRUCT_WORKSPACE): " + what, T=T)
    ok = dict(T=100, k=8, band=15, local_costs=FAKE, moment=FAKE, result=FAKE)
    for change, what in ((dict(T=0), "T=0 outside [1, 2^31)"), (dict(k=0), "k=0 outside [1, 512]"),
                         (dict(k=513), "k=513 outside [1, 512]"), (dict(band=-1), "band=-1 outside"),
                         (dict(band=14), "band=14 does not hold the window of k=8; the least band that does is 15"),
                         (dict(band=1), "band=1 does not hold the window of k=8; the least band that does is 15"),
                         (dict(T=1 << 16, band=0), "T=65536 rows of 65536 band slots (band=0) reach 2^31"),
                         (dict(T=1 << 21, k=512, band=1023), "T=2097152 rows of 2047 band slots (band=1023) reach 2^31"),
                         (dict(local_costs=None), "local_costs is null"), (dict(moment=None), "moment is null"),
                         (dict(result=None), "result is null")):
        _err(_lib.STRUCT_NOVELTY, "rv_mosaic(STRUCT_NOVELTY): " + what, **dict(ok, **change))
    need = S.workspace_bytes(100)
    ok = dict(T=100, moment=FAKE, lag=8, width=16, lam=0.5, ws=FAKE, ws_bytes=need, path=FAKE, summary=FAKE)
    for change, what in ((dict(T=0), "T=0 outside"), (dict(lag=-1), "lag=-1 outside [0, 65536]"),
                         (dict(lag=65537), "lag=65537 outside [0, 65536]"), (dict(width=-1), "width=-1 outside [0, 65536]"),
                         (dict(width=65537), "width=65537 outside"), (dict(lam=-0.5), "lam=-0.5 must be finite and not negative"),
                         (dict(lam=float("inf")), "lam=inf"), (dict(lam=float("nan")), "lam=nan"),
                         (dict(moment=None), "moment is null"), (dict(path=None), "the path is null"),
                         (dict(summary=None), "the summary is null"), (dict(ws=None), "ws is null"),
                         (dict(ws=FAKE + 8), "ws is not 256-byte aligned"),
                         (dict(ws_bytes=need - 1), "ws_bytes=%d, T=100 needs %d" % (need - 1, need))):
        _err(_lib.STRUCT_PEAKS, "rv_mosaic(STRUCT_PEAKS): " + what, **dict(ok, **change))


def test_python_argument_checks_and_helpers_without_a_device():
    from rawaudiovae_kelsey_amd import structure as S
    assert np.array_equal(S.taper(3, None), np.ones(6)) and S.taper(3, None).dtype == np.float64
    for R, sigma in ((1, 0.5), (7, 0.5), (32, 0.25)):
        assert np.array_equal(_bits(S.taper(R, sigma)), _bits(O.taper(R, sigma)))
        n = np.arange(2 * R)
        assert np.array_equal(S.taper(R, sigma), np.exp(-((n - R + 0.5) ** 2) / (2 * (sigma * R) ** 2)))
        assert np.array_equal(S.taper(R, sigma), S.taper(R, sigma)[::-1])
    assert S.pick_band(1000, 8) == 15 and S.pick_band(31, 8) == 15 and S.pick_band(30, 8) == 0 and S.pick_band(1, 1) == 0
    assert S.pick_band(3, 1) == 1 and S.pick_band(2, 1) == 0
    for bad in (0, 513, 2.0, True):
        with pytest.raises(ValueError, match="kernel="):
            S.check_kernel(bad)
    with pytest.raises(ValueError, match="sigma=0"):
        S.taper(4, 0)
    with pytest.raises(ValueError, match="gap=-1"):
        S.check_peaks(-1, 0, 0.0)
    with pytest.raises(ValueError, match="mean_radius=65537"):
        S.check_peaks(0, 65537, 0.0)
    for d in (-0.5, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="delta="):
            S.check_peaks(0, 0, d)
    with pytest.raises(ValueError, match="band=14 does not hold the window of kernel=8: the least band that does is 15"):
        S.check_struct_band(100, 14, 8)
    assert S.check_struct_band(100, None, 8) == 15 and S.check_struct_band(20, None, 8) == 0
    with pytest.raises(ValueError, match="1-D float64 device tensor"):
        S.peaks(torch.zeros(4, dtype=torch.float64), 0, 0, 0.0)
    with pytest.raises(ValueError, match="2-D float32 device tensor"):
        S.self_costs(torch.zeros(4, 3))
    assert S.form([0, 1, 0, 2]) == "A B A C" and S.form([0]) == "A" and S.form([25, 26]) == "Z 26"


def test_the_label_rule_on_a_hand_made_matrix():
    from rawaudiovae_kelsey_amd.structure import labels_from_distances as lab
    D = np.array([[0, 10, 1, 9],
                  [10, 0, 10, 12],
                  [1, 10, 0, 11],
                  [9, 12, 11, 0]], np.float64)
    # adjacent distances 10, 10, 11: the limit is 0.5 * 31 / 3; 2 is within it of 0, 3 of nothing
    assert lab(D).tolist() == [0, 1, 0, 2]
    assert lab(D, similar=0.05).tolist() == [0, 1, 2, 3]
    assert lab(D, similar=2.0).tolist() == [0, 0, 0, 0]
    assert lab(np.zeros((1, 1))).tolist() == [0]
    # the nearest earlier segment decides, ties to the lower one: 2 is equally near 0 and 1
    D = np.array([[0, 8, 2], [8, 0, 2], [2, 2, 0]], np.float64)
    assert lab(D, similar=0.5).tolist() == [0, 1, 0]                          # the limit is 0.5 * (8 + 2) / 2 = 2.5
    D[2, 0] = 3.0
    assert lab(D, similar=0.5).tolist() == [0, 1, 1]
    with pytest.raises(ValueError, match="square"):
        lab(np.zeros((2, 3)))


def test_segment_py_parser_errors():
    sys.path.insert(0, REPO)
    import segment as cli
    find = ["find", "--checkpoint", "c", "--in", "a.wav", "--out", "s.json"]
    args = cli.parse_args(find + ["--hop", "256", "--kernel", "32", "--gap", "16", "--delta", "0.5", "--novelty", "n.npy"])
    assert (args.command, args.hop, args.kernel, args.gap, args.delta, args.novelty) == ("find", 256, 32, 16, 0.5, "n.npy")
    assert (args.sigma, args.mean_radius, args.similar) == (0.5, None, 0.5)
    assert cli.parse_args(find + ["--sigma", "none"]).sigma is None
    args = cli.parse_args(["split", "--segments", "s.json", "--in", "a.wav", "--out-dir", "d"])
    assert (args.command, args.segments, args.wav, args.out_dir) == ("split", "s.json", "a.wav", "d")
    for argv, msg in ((find + ["--hop", "0"], "--hop '0'"), (find + ["--kernel", "0"], "--kernel '0'"),
                      (find + ["--kernel", "513"], "--kernel 513: at most 512"), (find + ["--kernel", "x"], "--kernel 'x'"),
                      (find + ["--gap", "-1"], "--gap '-1'"), (find + ["--gap", "65537"], "--gap 65537: at most 65536"),
                      (find + ["--mean-radius", "-2"], "--mean-radius '-2'"), (find + ["--delta", "-1"], "--delta '-1'"),
                      (find + ["--delta", "inf"], "--delta 'inf'"), (find + ["--delta", "x"], "--delta 'x'"),
                      (find + ["--sigma", "0"], "--sigma '0'"), (find + ["--similar", "nan"], "--similar 'nan'"),
                      ([], "expected a command: find or split")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            cli.parse_args(argv)
    with pytest.raises(SystemExit):
        cli.parse_args(["find", "--checkpoint", "c", "--out", "s.json"])            # no --in
    with pytest.raises(SystemExit):
        cli.parse_args(["split", "--segments", "s.json", "--in", "a.wav"])           # no --out-dir
