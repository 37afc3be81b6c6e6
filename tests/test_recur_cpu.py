"""The recurrence rules without a device: the numpy oracle (tests/recur_oracle.py) against a brute-force triple loop, the
pick rules on P and I (ties, masking, no finite entry), the plan of the looped rows, the header's op codes and field
names, the library's argument checks (all made on the host, reached with fake pointers) and recur.py's parser."""
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import align_oracle as AO  # noqa: E402
import recur_oracle as O  # noqa: E402

FAKE = 0x7000_0000_0000      # a non-null, 256-byte aligned address no check dereferences
BI, BJ = 16, 256             # csrc/recur.hip: REC_BI rows to a workgroup, REC_BJ diagonals to a tile
FULL = 2 ** 31 - 1


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- the oracle ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 3, 5])
def test_the_oracle_equals_a_brute_force_triple_loop(m):
    for Ta, Tb, seed in ((m, m, 0), (m + 1, m + 3, 1), (9, 7, 2), (12, 12, 3)):
        if Ta < m or Tb < m:
            continue
        a, b = AO.binary_latents(Ta, 3, seed), AO.binary_latents(Tb, 3, seed + 50)      # small integers: many exact ties
        dm = AO.local_costs(a, b, 0)[0]
        for row0, lo, hi, mirror in ((0, -FULL, FULL, 0), (0, 2, FULL, 1), (3, 1, 4, 0), (5, -3, -1, 0), (0, 0, 0, 1),
                                     (2, 0, 0, 0), (0, 40, 50, 1)):
            P, I = O.profile(dm, m, row0, lo, hi, mirror)
            bP, bI = O.brute_profile(dm, m, row0, lo, hi, mirror)
            assert np.array_equal(_bits(P), _bits(bP)) and np.array_equal(I, bI), (m, Ta, Tb, row0, lo, hi, mirror)
            assert I.dtype == np.int32 and ((I == -1) == np.isinf(P)).all()
        # a NaN and a +inf cell: exactly the windows that hold them lose
        for bad in (np.nan, np.inf):
            d2 = dm.copy()
            d2[Ta // 2, Tb // 2] = bad
            P, I = O.profile(d2, m)
            bP, bI = O.brute_profile(d2, m, 0, -FULL, FULL, 0)
            assert np.array_equal(_bits(P), _bits(bP)) and np.array_equal(I, bI)
            W = O.window_sums(d2, m)
            hit = ~np.isfinite(W)
            assert hit.any() and all(not hit[i, I[i]] for i in range(len(I)) if I[i] >= 0)


def test_the_self_join_of_a_periodic_trajectory_is_exactly_zero_at_the_lowest_period():
    p, T, m = 5, 23, 4
    mu = AO.random_latents(p, 3, 7)[np.arange(T) % p]
    dm = AO.local_costs(mu, mu, 0)[0]
    P, I = O.profile(dm, m, 0, m, FULL, O.MIRROR)
    assert (P == 0).all() and not np.signbit(P).any()
    want = [min(j for j in range(T - m + 1) if (j - i) % p == 0 and abs(j - i) >= m) for i in range(T - m + 1)]
    assert I.tolist() == want
    # slabs with their row0 give the rows of the whole-matrix call
    for rows in (1, 3, 20):
        for i0 in range(0, T - m + 1, rows):
            n = min(rows, T - m + 1 - i0)
            sP, sI = O.profile(dm[i0:i0 + n + m - 1], m, i0, m, FULL, O.MIRROR)
            assert np.array_equal(_bits(sP), _bits(P[i0:i0 + n])) and np.array_equal(sI, I[i0:i0 + n])


# ---- the pick rules --------------------------------------------------------------------------------------------------

def test_motifs_discords_and_best_loop_ties_masking_and_no_finite_entry():
    from rawaudiovae_kelsey_amd import recur as R
    P = np.array([3.0, 1.0, 1.0, 5.0, np.inf, 0.5, 9.0, np.nan, 1.0, 5.0])
    I = np.array([5, 8, 9, 0, -1, 0, 2, -1, 1, 3])
    for pick, orc in ((R.pick_motifs, O.motifs), (R.pick_discords, O.discords)):
        for ex in (0, 1, 2, 20):
            for K in (0, 1, 3, 20):
                assert pick(P, I, ex, K) == orc(P, I, ex, K), (ex, K)
    assert R.pick_motifs(P, I, 0, 3) == [(5, 0, 0.5), (1, 8, 1.0), (2, 9, 1.0)]          # ties: the lower i; row 0 masked by I[5]
    assert R.pick_motifs(P, I, 1, 9) == [(5, 0, 0.5), (2, 9, 1.0)]                       # 4..6, 0..1, then 1..3, 8..9: 7 is NaN
    assert R.pick_discords(P, I, 0, 2) == [(6, 2, 9.0), (3, 0, 5.0)]                     # 5.0 twice: the lower i
    assert R.pick_discords(P, I, 20, 5) == [(6, 2, 9.0)]
    assert R.pick_best_loop(P, I) == O.best_loop(P, I) == (5, 0, 0.5)
    none = np.array([np.inf, np.nan, -np.inf])
    assert R.pick_motifs(none, [-1, -1, -1], 1, 3) == [] == R.pick_discords(none, [-1, -1, -1], 1, 3)
    assert R.pick_best_loop(none, [-1, -1, -1]) is None and O.best_loop(none, [-1, -1, -1]) is None
    rs = np.random.RandomState(4)
    for _ in range(20):
        P = rs.randint(0, 6, 40).astype(np.float64)
        P[rs.rand(40) < 0.2] = np.inf
        I = rs.randint(0, 40, 40)
        ex, K = int(rs.randint(0, 6)), int(rs.randint(1, 8))
        got = R.pick_motifs(P, I, ex, K)
        assert got == O.motifs(P, I, ex, K) and R.pick_discords(P, I, ex, K) == O.discords(P, I, ex, K)
        for (i, _, _), (i2, _, _) in zip(got, got[1:]):
            assert abs(i - i2) > ex and P[i] <= P[i2]
    with pytest.raises(ValueError, match="exclude=-1"):
        R.pick_motifs(P, I, -1, 1)
    with pytest.raises(ValueError, match="K=-1"):
        R.pick_motifs(P, I, 1, -1)


def test_loop_rows_lengths_indices_and_the_two_value_errors():
    from rawaudiovae_kelsey_amd import recur as R
    for T, start, end, m, repeats in ((20, 3, 9, 2, 1), (20, 3, 9, 2, 3), (32, 0, 16, 16, 2), (12, 4, 8, 4, 4), (9, 2, 5, 3, 2)):
        src, other, g = R.loop_rows(T, start, end, m, repeats)
        plan = O.loop_plan(T, start, end, m, repeats)
        assert src.tolist() == [p[0] for p in plan] and other.tolist() == [p[1] for p in plan]
        assert np.array_equal(g.view(np.int32), np.array([p[2] for p in plan], np.float32).view(np.int32))
        assert src.dtype == other.dtype == np.int64 and g.dtype == np.float32
        assert len(src) == T + (repeats - 1) * (end - start)
        seam = other >= 0
        assert seam.sum() == m * repeats and (g[~seam] == 0).all()
        assert src[:end].tolist() == list(range(end)) and src[len(src) - (T - end - m):].tolist() == list(range(end + m, T))
        want = np.float32(np.arange(1, m + 1, dtype=np.float64) / (m + 1))
        assert np.array_equal(g[seam][:m], want) and 0 < g[seam].min() and g[seam].max() < 1
        # the last seam leaves the loop: from the rows at start to the rows at end
        last = np.nonzero(seam)[0][-m:]
        assert src[last].tolist() == list(range(start, start + m)) and other[last].tolist() == list(range(end, end + m))
        if repeats > 1:
            first = np.nonzero(seam)[0][:m]
            assert src[first].tolist() == list(range(end, end + m)) and other[first].tolist() == list(range(start, start + m))
    mu = AO.random_latents(12, 3, 0)
    rows = O.loop_rows(mu, 4, 8, 2, 2)
    assert rows.shape == (16, 3) and np.array_equal(rows[:8], mu[:8]) and np.array_equal(rows[-2:], mu[10:])
    with pytest.raises(ValueError, match="end=9"):
        R.loop_rows(12, 2, 9, 4, 2)                 # end + m > T
    with pytest.raises(ValueError, match="start=6 and end=9"):
        R.loop_rows(20, 6, 9, 4, 2)                 # end - start < m
    with pytest.raises(ValueError, match="repeats=0"):
        R.loop_rows(20, 2, 9, 4, 0)
    for fn in (lambda: O.loop_plan(12, 2, 9, 4, 2), lambda: O.loop_plan(20, 6, 9, 4, 2)):
        with pytest.raises(ValueError):
            fn()


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def test_op_codes_and_field_names_follow_the_header():
    from rawaudiovae_kelsey_amd import _lib
    text = open(REPO + "/include/rawvae_hip.h").read()
    codes = dict(re.findall(r"#define (RV_RECUR_\w+) (\d+)", text))
    assert codes == dict(RV_RECUR_PROFILE="40", RV_RECUR_WORKSPACE="41", RV_RECUR_MIRROR="1")
    assert (_lib.RECUR_PROFILE, _lib.RECUR_WORKSPACE, _lib.RECUR_MIRROR) == (40, 41, 1)
    assert _lib.RECUR_WORKSPACE in _lib._HOST_ONLY_OPS and _lib.RECUR_PROFILE not in _lib._HOST_ONLY_OPS
    para = text[text.index("/* Latent recurrence"):text.index("#define RV_RECUR_PROFILE")]
    types = {n: ctype for slot in abi_slots.header_slots() for n, ctype in slot}
    for field, ctype in (("local_costs", "float*"), ("stride", "long"), ("n_rows", "long"), ("N", "long"), ("k", "long"),
                         ("T", "long"), ("row0", "long"), ("lag", "long"), ("width", "long"), ("mode", "long"),
                         ("splits", "long"), ("ws", "void*"), ("ws_bytes", "long"), ("result", "double*"), ("idx", "int*")):
        assert re.search(r"\b%s\b" % field, para), field
        assert hasattr(_lib.MosaicDesc, field) and types[field] == ctype, (field, types.get(field))
    assert "38 and 39 are unassigned" in para
    # no new member, no new role: 37 slots of 8 bytes, the earlier ops' numbers, the version, no new export
    assert len(abi_slots.check_layout()) == 37 and _lib.C.sizeof(_lib.MosaicDesc) == 37 * 8
    assert (_lib.MOSAIC_KNN, _lib.ALIGN_COST, _lib.STRUCT_WORKSPACE, _lib.SMOOTH_WORKSPACE) == (0, 26, 33, 37)
    assert _lib.lib().rv_version() == 100
    assert "recur" not in " ".join(_lib.EXPORTED)
    for op in (38, 39, 42):
        with pytest.raises(_lib.RvError, match="unknown op %d" % op):
            _lib.lib().rv_mosaic(op, _lib.C.byref(_lib.MosaicDesc()), None)


def _err(op, text, **fields):
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError) as e:
        _lib.lib().rv_mosaic(op, _lib.C.byref(_lib.MosaicDesc(**fields)), None)
    assert text in str(e.value), str(e.value)


def test_workspace_query_and_every_argument_error_names_its_field():
    from rawaudiovae_kelsey_amd import _lib, recur as R
    up = lambda n: -(-n // 256) * 256  # noqa: E731
    for T, N, m in ((1, 1, 1), (100, 131, 32), (5000, 5031, 32), (40000, 300, 256)):
        assert R.workspace_bytes(T, N, m, 1) == 0
        for S in (2, 3, 1024):
            assert R.workspace_bytes(T, N, m, S) == up(8 * S * T) + up(4 * S * T)
        nb, nt = -(-T // BI), -(-(N - m + BI) // BJ)
        S = min(-(-8192 // nb), nt)                   # the library's choice: about 8192 workgroups, at most one per tile
        assert R.workspace_bytes(T, N, m, 0) == (up(8 * S * T) + up(4 * S * T) if S > 1 else 0)
    for change, what in ((dict(k=0), "k=0 outside [1, 256]"), (dict(k=257), "k=257 outside [1, 256]"), (dict(T=0), "T=0 outside"),
                         (dict(N=7), "N=7 outside [k=8"), (dict(splits=-1), "splits=-1 outside [0, 1024]"),
                         (dict(splits=1025), "splits=1025 outside")):
        _err(_lib.RECUR_WORKSPACE, "rv_mosaic(RECUR_WORKSPACE): " + what, **dict(dict(T=10, N=20, k=8, splits=0), **change))
    need = R.workspace_bytes(23, 40, 8, 2)
    ok = dict(local_costs=FAKE, stride=43, n_rows=30, N=40, k=8, T=23, row0=0, lag=8, width=FULL, mode=1, splits=2, ws=FAKE,
              ws_bytes=need, result=FAKE, idx=FAKE)
    for change, what in ((dict(k=0), "k=0 outside [1, 256]"), (dict(k=257), "k=257 outside [1, 256]"),
                         (dict(T=22), "T=22 is not n_rows=30 - k + 1"), (dict(T=24), "T=24 is not n_rows=30 - k + 1"),
                         (dict(n_rows=7, T=1), "T=1 is not n_rows=7 - k + 1"),
                         (dict(N=7, stride=7), "N=7 outside [k=8"), (dict(stride=39), "stride=39 below N=40"),
                         (dict(stride=1 << 27), "n_rows=30 rows of stride=134217728 reach 2^31"),
                         (dict(row0=-1), "row0=-1 outside"), (dict(lag=9, width=8), "lag=9 above width=8"),
                         (dict(lag=-(1 << 31)), "lag=-2147483648 outside"), (dict(width=1 << 31), "width=2147483648 outside"),
                         (dict(mode=2), "mode=2 is neither 0 nor RV_RECUR_MIRROR"), (dict(mode=-1), "mode=-1"),
                         (dict(splits=1025), "splits=1025 outside [0, 1024]"),
                         (dict(local_costs=None), "local_costs is null"), (dict(result=None), "result is null"),
                         (dict(idx=None), "idx is null"), (dict(ws=None), "ws is null"),
                         (dict(ws_bytes=need - 1), "ws_bytes=%d, T=23 with splits=2 needs %d" % (need - 1, need)),
                         (dict(ws=FAKE + 8), "ws is not 256-byte aligned")):
        _err(_lib.RECUR_PROFILE, "rv_mosaic(RECUR_PROFILE): " + what, **dict(ok, **change))


def test_python_argument_checks_without_a_device():
    from rawaudiovae_kelsey_amd import recur as R
    for bad in (0, 257, 2.0, True):
        with pytest.raises(ValueError, match="m="):
            R.check_m(bad)
    with pytest.raises(ValueError, match="lo=5 is above hi=4"):
        R.check_range(5, 4)
    with pytest.raises(ValueError, match="hi="):
        R.check_range(0, 1 << 31)
    with pytest.raises(ValueError, match="lo="):
        R.check_range(1.5, 4)
    with pytest.raises(ValueError, match="splits=1025"):
        R.check_splits(1025)
    with pytest.raises(ValueError, match="2-D float32 device tensor"):
        R.profile(torch.zeros(4, 4), 2)
    with pytest.raises(ValueError, match="2-D float32 device tensor"):
        R.recurrence(torch.zeros(4, 3), m=2)
    assert R.join_range(True, 8) == (8, FULL, True, 8) and R.join_range(True, 8, exclude=0) == (0, FULL, True, 0)
    assert R.join_range(False, 8) == (-FULL, FULL, False, 8) and R.join_range(True, 8, None, 20, 90) == (20, 90, False, 8)
    with pytest.raises(ValueError, match="give both or neither"):
        R.join_range(True, 8, None, 3, None)
    with pytest.raises(ValueError, match="exclude=-2"):
        R.join_range(True, 8, -2)
    loop = R.Loop(10, 42, 0.25, 4, 16, 8000)
    assert (loop.frames, loop.samples, loop.start_sample, loop.end_sample) == (32, 512, 160, 672)
    assert (loop.start_seconds, loop.end_seconds, loop.seconds) == (0.02, 0.084, 0.064)
    with pytest.raises(ValueError, match="sampling_rate"):
        R.Loop(1, 9, 0.0, 4, 16).seconds


def test_recur_py_parser_errors():
    sys.path.insert(0, REPO)
    import recur as cli
    mot = ["motifs", "--checkpoint", "c", "--in", "a.wav", "--out", "m.json"]
    args = cli.parse_args(mot + ["--hop", "256", "--window-frames", "32", "--top", "5", "--against", "b.wav", "--profile", "p.npy"])
    assert (args.command, args.hop, args.window_frames, args.top, args.against, args.profile, args.exclude) == (
        "motifs", 256, 32, 5, "b.wav", "p.npy", None)
    assert cli.parse_args(["discords"] + mot[1:]).command == "discords"
    loop = ["loop", "--checkpoint", "c", "--in", "a.wav", "--out", "o.wav"]
    args = cli.parse_args(loop + ["--hop", "256", "--window-frames", "16", "--min-seconds", "1", "--max-seconds", "8", "--repeats", "4"])
    assert (args.command, args.hop, args.window_frames, args.min_seconds, args.max_seconds, args.repeats, args.window) == (
        "loop", 256, 16, 1.0, 8.0, 4, None)
    assert cli.parse_args(loop).window_frames == 16 and cli.parse_args(mot).window_frames == 32
    for argv, msg in ((mot + ["--hop", "0"], "--hop '0'"), (mot + ["--window-frames", "0"], "--window-frames '0'"),
                      (mot + ["--window-frames", "257"], "--window-frames 257: at most 256"), (mot + ["--top", "0"], "--top '0'"),
                      (mot + ["--exclude", "-1"], "--exclude '-1'"), (loop + ["--min-seconds", "0"], "--min-seconds '0'"),
                      (loop + ["--max-seconds", "inf"], "--max-seconds 'inf'"), (loop + ["--min-seconds", "x"], "--min-seconds 'x'"),
                      (loop + ["--min-seconds", "9"], "--min-seconds 9: above --max-seconds 8"),
                      (loop + ["--repeats", "0"], "--repeats '0'"), (loop + ["--window", "hamming"], "--window 'hamming'"),
                      (loop + ["--window", "hann"], "--window hann: needs --hop"), ([], "expected a command: motifs, discords or loop")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            cli.parse_args(argv)
    with pytest.raises(SystemExit):
        cli.parse_args(["motifs", "--checkpoint", "c", "--out", "m.json"])            # no --in
    with pytest.raises(SystemExit):
        cli.parse_args(loop + ["--top", "3"])                                          # --top belongs to motifs / discords
