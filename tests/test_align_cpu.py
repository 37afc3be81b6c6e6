"""The alignment without a device: the numpy oracle (tests/align_oracle.py) against an exhaustive enumeration of every
monotone path and against a planted warp -- two checks that rest on no DP --, the band rule against brute-force
reachability, the header's op codes, the library's argument checks (all made on the host) and align.py's parser."""
import itertools
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import align_oracle as O  # noqa: E402

FAKE = 0x7000_0000_0000      # a non-null, 256-byte aligned address no check dereferences
PENALTIES = (0.0, 0.5, 1e30)


def _paths(Ta, Tb, ok, mode):
    """Every monotone path through the cells where ok[i, j], as (cells, steps): global paths run from (0, 0) to
    (Ta - 1, Tb - 1); subsequence paths start at any (0, j), end at any (Ta - 1, j) and never move left in row 0."""
    starts = [(0, 0)] if mode == O.GLOBAL else [(0, j) for j in range(Tb)]
    out = []

    def walk(cells, steps):
        i, j = cells[-1]
        if i == Ta - 1 and (mode == O.SUBSEQUENCE or j == Tb - 1):
            out.append((list(cells), list(steps)))
        for k, (di, dj) in enumerate(((1, 1), (1, 0), (0, 1))):
            ni, nj = i + di, j + dj
            if ni < Ta and nj < Tb and ok[ni, nj] and not (mode == O.SUBSEQUENCE and k == 2 and i == 0):
                walk(cells + [(ni, nj)], steps + [k])

    for s in starts:
        if ok[s]:
            walk([s], [])
    return out


def _path_cost(full, cells, steps, p):
    """The path's cost in the DP's own order: C = dd at the start, then C = fl(dd + fl(C + p)) (no p on a diagonal)."""
    c = float(full[cells[0]])
    for cell, k in zip(cells[1:], steps):
        c = float(full[cell]) + (c if k == 0 else c + p)
    return c


def _enumerated(full, mode, p):
    """(optimum, the optimal path the tie order picks) over all paths; rounding is monotone, so the DP's optimum is the
    minimum of the paths' costs in the DP's order, bit for bit.  Ties: the lowest end j, then, read from the end
    backwards, diag before up before left."""
    Ta, Tb = full.shape
    ok = full < np.inf
    best = None
    for cells, steps in _paths(Ta, Tb, ok, mode):
        key = (_path_cost(full, cells, steps, p), cells[-1][1], steps[::-1])
        if best is None or key < best[0]:
            best = (key, cells)
    return (np.inf, None) if best is None else (best[0][0], best[1])


@pytest.mark.parametrize("maker", ["random", "binary"])
def test_the_oracle_equals_exhaustive_enumeration_up_to_five_by_five(maker):
    make = O.random_latents if maker == "random" else O.binary_latents
    checked = 0
    for Ta, Tb in itertools.product(range(1, 6), repeat=2):
        a, b = make(Ta, 3, 10 * Ta + Tb), make(Tb, 3, 100 + 10 * Ta + Tb)
        for r, penalty, mode in itertools.product((0, 1, 2), PENALTIES, (O.GLOBAL, O.SUBSEQUENCE)):
            if not O.admits(Ta, Tb, r) or (mode == O.SUBSEQUENCE and r):
                continue
            got = O.align(a, b, r, mode, penalty)
            want, cells = _enumerated(got["full"], mode, float(np.float32(penalty)))
            assert got["cost"][0] == want, (Ta, Tb, r, penalty, mode)
            assert got["choice"][3] == 1 and (got["path"][got["P"]:] == -1).all()
            # The path and, on the binary inputs, the tie order: wherever the sums are exact.  At p = 1e30 a sum that
            # holds a penalty absorbs every local cost, so equal totals no longer mean equal prefixes; that penalty is
            # checked where it forces the diagonal (Ta = Tb).
            if penalty < 1e30 or (Ta == Tb and mode == O.GLOBAL):
                assert got["P"] == len(cells) and got["path"][:got["P"]].tolist() == [list(c) for c in cells], (
                    Ta, Tb, r, penalty, mode)
                assert got["choice"].tolist() == [len(cells), cells[0][1], cells[-1][1], 1]
            checked += 1
    assert checked >= 250


def test_a_huge_penalty_forces_the_diagonal_and_a_blocked_row_blocks_everything():
    a, b = O.random_latents(6, 4, 1), O.random_latents(6, 4, 2)
    got = O.align(a, b, 0, O.GLOBAL, 1e30)
    assert got["path"][:got["P"]].tolist() == [[i, i] for i in range(6)]
    a[3] = np.nan
    for mode in (O.GLOBAL, O.SUBSEQUENCE):
        got = O.align(a, b, 0, mode, 0.0)
        assert got["P"] == 0 and got["choice"].tolist() == [0, -1, -1, 0] and (got["path"] == -1).all()
        assert got["cost"].tolist() == [np.inf, 0.0]


def test_the_band_rule_equals_brute_force_reachability_up_to_twelve():
    from rawaudiovae_kelsey_amd import align as A
    for Ta, Tb, r in itertools.product(range(1, 13), range(1, 13), range(1, 13)):
        ok = O.in_band(Ta, Tb, r)
        reach = np.zeros((Ta, Tb), bool)
        reach[0, 0] = ok[0, 0]
        for i in range(Ta):
            for j in range(Tb):
                if ok[i, j] and ((i and reach[i - 1, j]) or (j and reach[i, j - 1]) or (i and j and reach[i - 1, j - 1])):
                    reach[i, j] = True
        assert bool(reach[Ta - 1, Tb - 1]) == O.admits(Ta, Tb, r) == A.band_admits(Ta, Tb, r), (Ta, Tb, r)
        least = A.least_band(Ta, Tb)
        assert A.band_admits(Ta, Tb, least) and (least == 1 or not A.band_admits(Ta, Tb, least - 1)), (Ta, Tb)


@pytest.mark.parametrize("Ta,L,seed", [(1, 3, 0), (7, 3, 1), (40, 8, 2), (150, 5, 3)])
def test_the_planted_warp_is_recovered_at_cost_zero(Ta, L, seed):
    a, b, path = O.planted_warp(Ta, L, seed)
    for r in (0, b.shape[0]):
        got = O.align(a, b, r, O.GLOBAL, 0.0)
        assert got["P"] == path.shape[0] and np.array_equal(got["path"][:got["P"]], path)
        assert got["cost"].tolist() == [0.0, 0.0]
    # the three timelines of the planted path
    P = path.shape[0]
    full = np.full((Ta + b.shape[0] - 1, 2), -1, np.int32)
    full[:P] = path
    on_a, on_b = O.warp(full, P, Ta, b.shape[0], O.ON_A), O.warp(full, P, Ta, b.shape[0], O.ON_B)
    assert np.array_equal(on_b, path) and np.array_equal(on_a[:, 0], np.arange(Ta))
    assert np.array_equal(on_a[:, 1], np.searchsorted(path[:, 0], np.arange(Ta)))      # the first copy of every row
    assert np.array_equal(O.warp(full, P, Ta, b.shape[0], O.ON_PATH), full)


@pytest.mark.parametrize("Ta,Tb,L,r", [(9, 13, 5, 0), (30, 41, 40, 3), (25, 25, 33, 0)])
def test_without_a_penalty_the_two_costs_are_the_same_bits(Ta, Tb, L, r):
    got = O.align(O.random_latents(Ta, L, 5), O.random_latents(Tb, L, 6), r, O.GLOBAL, 0.0)
    assert got["choice"][3] == 1 and got["cost"][0].tobytes() == got["cost"][1].tobytes()
    # the band layout: every slot outside [0, Tb) is +inf, the others are the full matrix's
    dm, full = got["dm"], got["full"]
    assert dm.shape == (Ta, O.band_width(Tb, r)) and dm.dtype == np.float32
    for i in range(Ta):
        for col in range(dm.shape[1]):
            j = col if not r else col - r + int(O.centre(i, Ta, Tb))
            assert dm[i, col] == (full[i, j] if 0 <= j < Tb else np.inf)


def test_op_codes_and_field_roles_follow_the_header():
    from rawaudiovae_kelsey_amd import _lib
    text = open(REPO + "/include/rawvae_hip.h").read()
    codes = dict(re.findall(r"#define (RV_ALIGN_\w+) (\d+)", text))
    assert codes == dict(RV_ALIGN_COST="26", RV_ALIGN_FORWARD="27", RV_ALIGN_BACKTRACK="28", RV_ALIGN_WARP="29",
                         RV_ALIGN_WORKSPACE="30", RV_ALIGN_GLOBAL="0", RV_ALIGN_SUBSEQUENCE="1", RV_ALIGN_ON_A="0",
                         RV_ALIGN_ON_B="1", RV_ALIGN_ON_PATH="2")
    assert (_lib.ALIGN_COST, _lib.ALIGN_FORWARD, _lib.ALIGN_BACKTRACK, _lib.ALIGN_WARP, _lib.ALIGN_WORKSPACE) == (
        26, 27, 28, 29, 30)
    assert (_lib.ALIGN_GLOBAL, _lib.ALIGN_SUBSEQUENCE) == (0, 1)
    assert (_lib.ALIGN_ON_A, _lib.ALIGN_ON_B, _lib.ALIGN_ON_PATH) == (0, 1, 2)
    assert (O.GLOBAL, O.SUBSEQUENCE, O.ON_A, O.ON_B, O.ON_PATH) == (0, 1, 0, 1, 2)
    # the ops before them keep their numbers, the descriptor its 37 eight-byte slots, the library its version
    assert (_lib.MOSAIC_KNN, _lib.EVAL_DIMS, _lib.PCA_WORKSPACE, _lib.WALK_WORKSPACE) == (0, 17, 21, 25)
    assert re.search(r"#define RV_WALK_WORKSPACE 25\b", text) and re.search(r"#define RV_MOSAIC_KNN 0\b", text)
    assert len(abi_slots.check_layout()) == 37 and _lib.C.sizeof(_lib.MosaicDesc) == 37 * 8
    assert _lib.lib().rv_version() == 100
    # the roles' slots and element types: the table of test_audio_tools_cpu.py


def _err(op, text, **fields):
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError) as e:
        _lib.lib().rv_mosaic(op, _lib.C.byref(_lib.MosaicDesc(**fields)), None)
    assert text in str(e.value), str(e.value)


def test_workspace_query_and_every_argument_error_names_its_field():
    from rawaudiovae_kelsey_amd import _lib, align as A
    up = lambda n: -(-n // 256) * 256  # noqa: E731
    # the back table, the end-cost row, the walk and the end record; beyond 2048 cells per diagonal also three diagonals
    assert A.workspace_bytes(1, 1) == up(1) + up(8) + up(8) + 256
    assert A.workspace_bytes(300, 257) == up(300 * 257) + up(8 * 257) + up(8 * 556) + 256
    assert A.workspace_bytes(1000, 1500, 40) == up(1000 * 81) + up(8 * 1500) + up(8 * 2499) + 256
    assert A.workspace_bytes(2048, 2048) == up(2048 * 2048) + up(8 * 2048) + up(8 * 4095) + 256
    assert A.workspace_bytes(2049, 2049) == up(2049 * 2049) + up(3 * 8 * 2049) + up(8 * 2049) + up(8 * 4097) + 256
    assert A.workspace_bytes(5000, 5000, 1024) == up(5000 * 2049) + up(3 * 8 * 5000) + up(8 * 5000) + up(8 * 9999) + 256
    shape = (("T", dict(T=0), "T=0 outside [1, 2^31)"), ("T", dict(T=1 << 31), "T=2147483648"),
             ("N", dict(N=0), "N=0 outside [1, 2^31)"), ("width", dict(width=-1), "band=-1 outside"),
             ("width", dict(T=5, N=40, width=3), "band=3: the band admits no path through T=5 by N=40; the least band "
                                                 "that does is 5"),
             ("width", dict(T=1, N=9, width=2), "band=2: the band admits no path through T=1 by N=9; the least band that does is 8"),
             ("cells", dict(T=1 << 20, N=1 << 20, width=0), "T=1048576 rows of 1048576 band slots (band=0) reach 2^31"))
    for op, name in ((_lib.ALIGN_WORKSPACE, "ALIGN_WORKSPACE"), (_lib.ALIGN_COST, "ALIGN_COST"),
                     (_lib.ALIGN_FORWARD, "ALIGN_FORWARD"), (_lib.ALIGN_BACKTRACK, "ALIGN_BACKTRACK")):
        ok = dict(T=20, N=30, L=8, width=4, q=FAKE, c=FAKE, dist=FAKE, ws=FAKE, ws_bytes=1 << 30, slot=FAKE, choice=FAKE,
                  cost=FAKE)
        for _, change, what in shape:
            _err(op, "rv_mosaic(%s): %s" % (name, what), **dict(ok, **change))
    ok = dict(T=20, N=30, L=8, width=4, q=FAKE, c=FAKE, dist=FAKE)
    for change, what in ((dict(L=0), "L=0 outside [1, 4096]"), (dict(L=4097), "L=4097 outside [1, 4096]"),
                         (dict(q=None), "a is null"), (dict(c=None), "b is null"),
                         (dict(dist=None), "local_costs is null")):
        _err(_lib.ALIGN_COST, "rv_mosaic(ALIGN_COST): " + what, **dict(ok, **change))
    need = A.workspace_bytes(20, 30, 4)
    ok = dict(T=20, N=30, width=4, dist=FAKE, ws=FAKE, ws_bytes=need, mode=_lib.ALIGN_GLOBAL, lam=0.5)
    for change, what in ((dict(mode=2), "mode=2 is neither"), (dict(mode=-1), "mode=-1"),
                         (dict(mode=_lib.ALIGN_SUBSEQUENCE), "band=4: RV_ALIGN_SUBSEQUENCE (mode) runs on the whole matrix"),
                         (dict(lam=-1.0), "penalty=-1 must be finite and not negative"), (dict(lam=float("inf")), "penalty=inf"),
                         (dict(lam=float("nan")), "penalty=nan"), (dict(dist=None), "local_costs is null"),
                         (dict(ws=None), "ws is null"), (dict(ws=FAKE + 8), "ws is not 256-byte aligned"),
                         (dict(ws_bytes=need - 1), "ws_bytes=%d, T=20 by N=30 at band=4 need %d" % (need - 1, need))):
        _err(_lib.ALIGN_FORWARD, "rv_mosaic(ALIGN_FORWARD): " + what, **dict(ok, **change))
    ok = dict(T=20, N=30, width=4, dist=FAKE, ws=FAKE, ws_bytes=need, slot=FAKE, choice=FAKE, cost=FAKE)
    for change, what in ((dict(dist=None), "local_costs is null"), (dict(slot=None), "the path is null"),
                         (dict(choice=None), "the summary is null"), (dict(cost=None), "path_costs is null"),
                         (dict(ws=None), "ws is null"), (dict(ws_bytes=need - 1), "ws_bytes=%d" % (need - 1))):
        _err(_lib.ALIGN_BACKTRACK, "rv_mosaic(ALIGN_BACKTRACK): " + what, **dict(ok, **change))
    ok = dict(T=20, N=30, slot=FAKE, choice=FAKE, idx=FAKE, mode=_lib.ALIGN_ON_B)
    for change, what in ((dict(T=0), "T=0"), (dict(N=0), "N=0"), (dict(mode=3), "mode=3 is none of"),
                         (dict(slot=None), "the path is null"), (dict(choice=None), "the summary is null"),
                         (dict(idx=None), "warp_table is null")):
        _err(_lib.ALIGN_WARP, "rv_mosaic(ALIGN_WARP): " + what, **dict(ok, **change))


def test_python_argument_checks_without_a_device():
    from rawaudiovae_kelsey_amd import align as A
    assert A.check_band(10, 20, None) == 0 and A.check_band(10, 20, 0) == 0 and A.check_band(10, 20, 5) == 5
    for band, msg in ((-1, "band=-1 must be"), (1.5, "band=1.5 must be"), (True, "band=True must be")):
        with pytest.raises(ValueError, match=msg):
            A.check_band(10, 20, band)
    with pytest.raises(ValueError, match="band=3 admits no path through 5 x 40 frames: the least band that does is 5"):
        A.check_band(5, 40, 3)
    # the cell limit names the least band that admits a path and the widest that fits
    with pytest.raises(ValueError, match=r"band=None: 100000 x 100000 cells exceed the limit of 2147483647; the least band "
                                         r"that admits a path is 1, the widest that fits is 10736"):
        A.check_band(100000, 100000, None)
    assert A.check_band(100000, 100000, 10736) == 10736
    with pytest.raises(ValueError, match="band=10737: 100000 x 21475 cells exceed"):
        A.check_band(100000, 100000, 10737)
    with pytest.raises(ValueError, match="at every band that admits a path"):
        A.check_band(10, 1000, None, cell_limit=500)
    for p in (-0.5, float("inf"), float("nan"), 1e39):
        with pytest.raises(ValueError, match="penalty="):
            A.check_penalty(p)
    assert A.check_penalty(1e30) == 1e30
    with pytest.raises(ValueError, match="2-D float32 device tensor"):
        A.local_costs(torch.zeros(4, 3), torch.zeros(5, 3))
    with pytest.raises(ValueError, match="2-D float32 device tensor"):
        A.align_latents(torch.zeros(4, 3), torch.zeros(5, 3))
    with pytest.raises(ValueError, match="timeline='c'"):
        A.warp(torch.zeros(3, 2), torch.zeros(4), 2, 2, "c")
    with pytest.raises(ValueError, match="mode='local'"):
        A.forward(torch.zeros(3, 3), 3, 3, 0, "local")


def test_align_py_parser_errors():
    sys.path.insert(0, REPO)
    import align as cli
    two = ["--checkpoint", "c", "--a", "a.wav", "--b", "b.wav", "--out", "o"]
    args = cli.parse_args(["path"] + two + ["--hop", "256", "--band", "200", "--penalty", "0.25"])
    assert (args.command, args.hop, args.band, args.penalty) == ("path", 256, 200, 0.25)
    args = cli.parse_args(["morph"] + two + ["--hop", "16", "--window", "hann", "--alpha", "0:1", "--timeline", "path"])
    assert (args.window, args.timeline, args.band, args.seed) == ("hann", "path", None, 0)
    assert args.curve_values.dtype == np.float64 and args.curve_values.tolist() == [0.0, 1.0]
    args = cli.parse_args(["find", "--checkpoint", "c", "--query", "q.wav", "--in", "l.wav", "--out", "m.json"])
    assert (args.query, args.recording, args.hop, args.penalty) == ("q.wav", "l.wav", None, 0.0)
    for argv, msg in ((["path"] + two + ["--hop", "0"], "--hop '0'"), (["path"] + two + ["--band", "-1"], "--band '-1'"),
                      (["path"] + two + ["--band", "x"], "--band 'x'"), (["path"] + two + ["--penalty", "-1"], "--penalty '-1'"),
                      (["path"] + two + ["--penalty", "inf"], "--penalty 'inf'"),
                      (["morph"] + two, "--alpha / --curve: expected exactly one"),
                      (["morph"] + two + ["--alpha", "0:1", "--curve", "c.npy"], "--alpha / --curve: expected exactly one"),
                      (["morph"] + two + ["--alpha", "0"], "--alpha '0': expected START:END"),
                      (["morph"] + two + ["--alpha", "0:nan"], "--alpha '0:nan'"),
                      (["morph"] + two + ["--alpha", "0:1", "--timeline", "c"], "--timeline 'c'"),
                      (["morph"] + two + ["--alpha", "0:1", "--window", "hamming"], "--window 'hamming'"),
                      (["morph"] + two + ["--alpha", "0:1", "--window", "hann"], "--window hann: needs --hop"),
                      (["morph"] + two + ["--alpha", "0:1", "--seed", "-1"], "--seed '-1'"),
                      ([], "expected a command: path, morph or find")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            cli.parse_args(argv)
    with pytest.raises(SystemExit):
        cli.parse_args(["find", "--checkpoint", "c", "--query", "q.wav", "--out", "m.json"])      # no --in
    with pytest.raises(SystemExit):
        cli.parse_args(["find", "--checkpoint", "c", "--query", "q.wav", "--in", "l.wav", "--band", "3", "--out", "m"])
