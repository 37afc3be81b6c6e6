"""Live mosaicing without a GPU: the header's new ops and fields, the workspace queries, the device-free validator, the
command line's flags, the greedy oracle against the Viterbi oracle, and the blockwise overlap-add against the offline
one (rawaudiovae_kelsey_amd/mosaic.py, mosaic.py, tests/live_mosaic_oracle.py)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import live_mosaic_oracle as LO  # noqa: E402
import mosaic_oracle as O  # noqa: E402
import mosaic_path_oracle as P  # noqa: E402

# rv_mosaic_desc as the parent commit declared it: new fields go behind these
FIELDS_33 = ["T", "k", "idx", "q", "c", "N", "L", "splits", "dist", "ws", "ws_bytes", "src", "src_len", "row_start",
             "stride", "n_rows", "width", "out", "ldo", "frames", "F", "S", "hop", "window", "n_out", "next_of", "row0",
             "rows", "trans", "lam", "slot", "choice", "cost"]
NEW_OPS = {"KNN_SMALL": 8, "KNN_SMALL_WORKSPACE": 9, "LIVE": 10, "LIVE_WORKSPACE": 11, "LIVE_RESET": 12}


def _header():
    with open(os.path.join(REPO, "include", "rawvae_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_appends_ops_and_fields_and_no_entry_point(tmp_path):
    from rawaudiovae_kelsey_amd import _lib
    src = _header()
    names = sorted(set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", src)))
    assert len(names) <= 70 and set(_lib.EXPORTED) >= {"rv_mosaic", "rv_stream_process"}
    for name, num in NEW_OPS.items():
        assert re.search(r"#define RV_MOSAIC_%s %d\b" % (name, num), src), name
        assert getattr(_lib, "MOSAIC_" + name) == num
    assert (_lib.LIVE_GRAINS, _lib.LIVE_DECODE) == (0, 1) and "#define RV_LIVE_DECODE 1" in src
    fields = abi_slots.check_layout()    # the slots' first names, the same in the header and in _lib
    assert fields[:33] == FIELDS_33 and fields[33:] == ["live", "mode", "weight", "which"]
    c = tmp_path / "c.c"
    c.write_text('#include "rawvae_hip.h"\nint main(void) { rv_stream_desc s = {0}; rv_mosaic_desc d = {0}; d.live = &s; '
                 'd.mode = RV_LIVE_DECODE; d.weight = 0; d.which = -1; d.k = RV_MOSAIC_KNN_SMALL + RV_MOSAIC_LIVE_RESET;'
                 ' return (int)sizeof(d) > 0 && d.live->S == 0 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(c), "-o",
                    str(tmp_path / "c.o")], check=True)
    assert C.sizeof(_lib.MosaicDesc) == 33 * 8 + 4 * 8     # 8-byte slots throughout (lam is padded to one)


def test_small_knn_workspace_query_touches_no_device():
    from rawaudiovae_kelsey_amd import _lib, mosaic
    assert mosaic.SMALL_T_MAX == 64
    assert mosaic.knn_workspace_bytes(16, 1240000, 256, 4, small=True) > 0
    assert mosaic.knn_workspace_bytes(16, 5000, 64, 1, splits=1, small=True) == 0
    assert mosaic.knn_workspace_bytes(5, 5000, 64, 2, splits=3, small=True) == 3 * 5 * 2 * 8
    # the grid fills the chip for any N: the workspace is that of ~1024 splits once N has that many runs of 256 rows
    per_split = mosaic.knn_workspace_bytes(1, 1240000, 256, 1, small=True) // 8
    assert 512 <= per_split <= 1024
    for bad in ((65, 1000, 8, 1), (0, 10, 8, 1), (4, 10, 8, 0), (4, 10, 8, 17), (4, 3, 8, 4), (4, 10, (1 << 24) + 4, 1)):
        with pytest.raises(_lib.RvError):
            mosaic.knn_workspace_bytes(*bad, small=True)


def _live_ws_bytes(n_streams=1, block=256, hop=256, S=1024, L=256, N=1240000, k=4, corpus_L=None, live=True):
    from rawaudiovae_kelsey_amd import _lib
    sd = _lib.StreamDesc(S=S, H=2048, L=L, n_streams=n_streams, block=block, hop=hop)
    d = _lib.MosaicDesc(k=k, N=N, L=L if corpus_L is None else corpus_L, live=C.pointer(sd) if live else None)
    _lib.lib().rv_mosaic(_lib.MOSAIC_LIVE_WORKSPACE, C.byref(d), None)
    return d.ws_bytes


def test_live_workspace_query_touches_no_device_and_rejects_bad_extents():
    from rawaudiovae_kelsey_amd import _lib
    one = _live_ws_bytes()
    assert one > 0 and one % 256 == 0
    assert _live_ws_bytes(n_streams=16, block=1024) > one                 # 64 rows: four passes of partials
    assert _live_ws_bytes(n_streams=32, block=1024) > one                 # 128 rows: the tile search's partials
    assert _live_ws_bytes(N=100, k=1) >= 256 + 1024                       # prev, then one query row of 256 floats
    for bad in (dict(block=100), dict(hop=0), dict(n_streams=0), dict(k=0), dict(k=17), dict(N=3), dict(corpus_L=8),
                dict(block=128), dict(live=False)):
        with pytest.raises(_lib.RvError):
            _live_ws_bytes(**bad)


def test_validator_names_the_argument():
    from rawaudiovae_kelsey_amd.mosaic import check_live_args
    ok = dict(segment_length=64, index_step=16, n_corpus=100, n_streams=2, block=32, hop=16, k=4, mode="grains",
              window="hann", continuity=0.5)
    assert check_live_args(**ok) == (16, 48, 2, 1)
    assert check_live_args(**dict(ok, hop=32, block=64)) == (32, 32, 2, 2)
    assert check_live_args(**dict(ok, hop=None, block=128, window=None, index_step=64)) == (64, 0, 2, 1)
    assert check_live_args(**dict(ok, hop=8, block=8, window=None, continuity=0)) == (8, 56, 1, 1)
    for change, name in ((dict(block=40), "block"), (dict(block=0), "block"), (dict(block=8), "block"),
                         (dict(hop=24, block=48), "hop"), (dict(hop=8, block=8), "hop"),
                         (dict(hop=64, block=64), "window"), (dict(window="hamming"), "window"), (dict(k=0), "k="),
                         (dict(k=17), "k="), (dict(k=5, n_corpus=4), "k="), (dict(n_corpus=0), "index"),
                         (dict(mode="blend"), "mode"), (dict(n_streams=0), "n_streams"),
                         (dict(continuity=-1.0), "continuity"), (dict(continuity=float("nan")), "continuity")):
        with pytest.raises(ValueError, match=name):
            check_live_args(**dict(ok, **change))


def test_cli_live_flags(tmp_path):
    sys.path.insert(0, REPO)
    import mosaic as cli
    from rawaudiovae_kelsey_amd import data as D
    r = subprocess.run([sys.executable, os.path.join(REPO, "mosaic.py"), "--help"], capture_output=True, text=True,
                       cwd=REPO)
    assert r.returncode == 0 and "--live-block" in r.stdout and "--streams" in r.stdout
    ini = tmp_path / "tiny.ini"
    ini.write_text("[audio]\nsampling_rate = 8000\nhop_length = 8\nsegment_length = 64\n[VAE]\nlatent_dim = 8\n"
                   "n_units = 96\n")
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    D.write_wav(corpus / "a.wav", np.zeros(640, np.float32), 8000)
    D.write_wav(tmp_path / "t.wav", np.zeros(300, np.float32), 8000)
    base = ["--config", str(ini), "--checkpoint", "none.pt", "--target", str(tmp_path / "t.wav"), "--out",
            str(tmp_path / "o.wav"), "--corpus", str(corpus)]
    for extra, flag in ((["--live-block", "0"], "--live-block"), (["--live-block", "x"], "--live-block"),
                        (["--live-block", "40", "--hop", "16"], "--live-block"), (["--live-block", "100"], "--live-block"),
                        (["--live-block", "64", "--streams", "0"], "--streams"), (["--streams", "2"], "--streams"),
                        (["--live-block", "64", "--continuity", "-1"], "--continuity")):
        with pytest.raises(ValueError, match=flag):
            cli.main(base + extra)
    args = cli.parse_args(base + ["--live-block", "128", "--streams", "3", "--hop", "16"])
    assert (args.live_block, args.streams, args.hop) == (128, 3, 16)
    assert cli.parse_args(base).live_block is None and cli.parse_args(base).streams == 1


def test_greedy_first_row_takes_the_lowest_valid_slot_and_k1_is_viterbi():
    rng = np.random.default_rng(0)
    N, L, T = 60, 8, 40
    mu = rng.standard_normal((N, L)).astype(np.float32)
    next_of = np.minimum(np.arange(N) + 1, N - 1).astype(np.int32)
    q = rng.standard_normal((T, L)).astype(np.float32)
    idx, dist = O.knn(q, mu, 1)
    slot, choice, prev, _ = LO.greedy(idx, dist, mu, next_of, 0.7)
    assert slot[0] == 0 and np.all(slot == 0) and np.array_equal(choice, idx[:, 0]) and prev == idx[-1, 0]
    idx[[3, 4, 17]], dist[[3, 4, 17]] = -1, np.inf                        # rows without a candidate
    for w in (0.0, 0.7, 100.0):
        slot, choice, prev, _ = LO.greedy(idx, dist, mu, next_of, w)
        vs, vc, _ = P.best_path(idx, dist, mu, next_of, w)
        assert np.array_equal(slot, vs) and np.array_equal(choice, vc)
        assert np.all(slot[[3, 4, 17]] == -1) and np.all(choice[[3, 4, 17]] == -1)
    # k = 4, prev < 0: the lowest valid j, whatever the weight; a weight that is not finite and >= 0 counts as 0
    idx4, dist4 = O.knn(q, mu, 4)
    idx4[0, 0], dist4[0, 0] = -1, np.inf
    s4 = LO.greedy(idx4, dist4, mu, next_of, 5.0)[0]
    assert s4[0] == 1
    for w in (-1.0, np.nan, np.inf):
        assert np.array_equal(LO.greedy(idx4, dist4, mu, next_of, w)[0], LO.greedy(idx4, dist4, mu, next_of, 0.0)[0])
    assert np.all(LO.greedy(idx4, dist4, mu, next_of, 0.0)[0][1:] == 0)   # w = 0: the nearest candidate


@pytest.mark.parametrize("lam", [1 / 16, 1 / 4, 1.0, 2.0])
def test_greedy_never_beats_viterbi_on_exact_cases(lam):
    for seed in range(4):
        mu, q, next_of = P.two_file_case(F=40, L=8, seed=seed)
        idx, dist = O.knn(q, mu, 2)
        gs, gc, _, gcost = LO.greedy(idx, dist, mu, next_of, lam)
        vs, vc, vcost = P.best_path(idx, dist, mu, next_of, lam)
        jg, jv = gcost[0] + lam * gcost[1], vcost[0] + lam * vcost[1]
        assert jg >= jv, (seed, jg, jv)
        if lam >= 1.0:      # a jump costs lam >= 1 > 1/4: the greedy path stays in file A, which is optimal
            assert jg == jv and np.all(gc < 40)


def test_greedy_follows_a_corpus_file_played_straight_through():
    sys.path.insert(0, REPO)
    from mosaic import continuing_share
    mu, _, next_of = P.two_file_case(F=50, L=8, seed=3)
    for which in (0, 1):
        q = mu[which * 50:(which + 1) * 50]
        idx, dist = O.knn(q, mu, 2)
        slot, choice, _, cost = LO.greedy(idx, dist, mu, next_of, 0.5)
        assert np.array_equal(choice, which * 50 + np.arange(50)) and np.all(cost == 0)
        assert continuing_share(choice, next_of) == 1.0


@pytest.mark.parametrize("S,hop,block,window", [(64, 16, 32, "hann"), (64, 64, 64, None), (64, 8, 40, None),
                                                (64, 32, 32, "hann"), (64, 16, 16, None)])
def test_blockwise_overlap_add_equals_the_offline_one(S, hop, block, window):
    from rawaudiovae_kelsey_amd.stream import window_norm, window_values
    rng = np.random.default_rng(S + hop + block)
    F = 6 * (block // hop)
    frames = rng.uniform(-1, 1, (F, S)).astype(np.float32)
    w = window_values(S, window)
    got = LO.block_ola(frames, hop, block, w, window_norm(w, hop))
    ref = O.ola(frames, hop, F * hop, None if window is None else w)
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))
