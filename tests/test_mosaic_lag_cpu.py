"""Live mosaicing with a lag, without a GPU: the numpy oracle of the fixed-lag rule against the greedy rule, brute force
and the offline Viterbi search, the header's new op, the workspace query, the device-free validator and the command
line's flag (tests/live_lag_oracle.py, include/rawvae_hip.h, rawaudiovae_kelsey_amd/mosaic.py, mosaic.py)."""
import ctypes as C
import itertools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import live_lag_oracle as G  # noqa: E402
import live_mosaic_oracle as LO  # noqa: E402
import mosaic_oracle as O  # noqa: E402
import mosaic_path_oracle as P  # noqa: E402

OPS = {"KNN": 0, "KNN_WORKSPACE": 1, "GATHER_MEAN": 2, "OLA": 3, "TRANSITION": 4, "PATH_FORWARD": 5, "PATH_BACKTRACK": 6,
       "PATH_WORKSPACE": 7, "KNN_SMALL": 8, "KNN_SMALL_WORKSPACE": 9, "LIVE": 10, "LIVE_WORKSPACE": 11, "LIVE_RESET": 12,
       "LIVE_DRAIN": 13}


def _random_case(rng, T=25, k=4, N=60, L=8):
    mu = rng.standard_normal((N, L)).astype(np.float32)
    q = rng.standard_normal((T, L)).astype(np.float32)
    next_of = np.minimum(np.arange(N) + 1, N - 1).astype(np.int32)
    idx, dist = O.knn(q, mu, k)
    return mu, next_of, idx, dist


def _dyadic_case(rng, T, k=3, N=30, L=8):
    """test_mosaic_path_cpu's exact-arithmetic generator: half-integer latents, every fp32 operation exact"""
    mu = (rng.integers(-4, 5, (N, L)) / 2).astype(np.float32)
    q = (rng.integers(-4, 5, (T, L)) / 2).astype(np.float32)
    next_of = np.minimum(np.arange(N) + 1, N - 1).astype(np.int32)
    idx, dist = O.knn(q, mu, k)
    return mu, next_of, idx, dist


def test_lag_zero_is_the_greedy_rule():
    rng = np.random.default_rng(0)
    for trial in range(40):
        mu, next_of, idx, dist = _random_case(rng)
        if trial % 4 == 0:
            idx[[5, 6]], dist[[5, 6]] = -1, np.inf              # rows without a candidate
        w = [0.0, 0.3, 1.0, 7.0][trial % 4]
        gs, gc, _, gcost = LO.greedy(idx, dist, mu, next_of, w)
        slot, choice, cost = G.fixed_lag(idx, dist, mu, next_of, w, 0)
        assert np.array_equal(slot, gs) and np.array_equal(choice, gc), trial
        assert np.array_equal(cost, gcost), trial
    mu, q, next_of = P.two_file_case(40, 8, 0)
    idx, dist = O.knn(q, mu, 2)
    gs, gc, _, gcost = LO.greedy(idx, dist, mu, next_of, 3 / 16)
    slot, choice, cost = G.fixed_lag(idx, dist, mu, next_of, 3 / 16, 0)
    assert np.array_equal(slot, gs) and np.array_equal(choice, gc) and np.array_equal(cost, gcost)


def test_the_committed_slot_is_the_first_step_of_a_brute_force_optimum():
    """Exact-integer windows of R <= 4 rows, k = 3: the slot a window solve commits starts one of the k^R paths of least
    cost (entry cost from prev included).  Optima tie, so membership is what holds."""
    rng = np.random.default_rng(1)
    k, tied = 3, 0
    for trial in range(300):
        R = 1 + trial % 4
        mu, next_of, idx, dist = _dyadic_case(rng, R, k)
        if trial % 7 == 0 and R > 1:
            idx[R - 1, 2], dist[R - 1, 2] = -1, np.inf          # a short row
        lam = [0.0, 0.25, 2.0][trial % 3]
        prev = int(rng.integers(-1, mu.shape[0]))
        tr = P.transitions(mu, idx, next_of)
        slot, _ = G.solve(idx, dist, tr, mu, next_of, 0, R - 1, lam, prev)
        entry, _ = G.entry_scores(idx[0], dist[0], mu, next_of, lam, prev)
        paths = np.array(list(itertools.product(range(k), repeat=R)))
        u = np.arange(R)
        J = entry[paths[:, 0]].astype(np.float64) + dist[u[None, 1:], paths[:, 1:]].astype(np.float64).sum(1)
        if R > 1:
            trs = tr[u[None, 1:], paths[:, :-1], paths[:, 1:]].astype(np.float64).sum(1)
            J = J + np.where(np.isinf(trs), np.inf, lam * np.where(np.isinf(trs), 0, trs))
        assert np.isfinite(J.min())
        firsts = set(paths[J == J.min(), 0].tolist())
        assert slot in firsts, (trial, slot, firsts)
        tied += len(firsts) > 1
    assert tied > 0


@pytest.mark.parametrize("lag", [39, 64])
def test_a_lag_of_the_whole_target_is_the_offline_search(lag):
    for seed in range(3):
        mu, q, next_of = P.two_file_case(40, 8, seed)
        idx, dist = O.knn(q, mu, 2)
        for lam in (1 / 16, 3 / 16, 1.0):
            vs, vc, vcost = P.best_path(idx, dist, mu, next_of, lam)
            slot, choice, cost = G.fixed_lag(idx, dist, mu, next_of, lam, lag)
            assert np.array_equal(slot, vs) and np.array_equal(choice, vc) and np.array_equal(cost, vcost)
    rng = np.random.default_rng(2)
    for trial in range(30):
        mu, next_of, idx, dist = _dyadic_case(rng, 7)
        if trial % 3 == 0:
            r = rng.integers(0, 7)
            idx[r], dist[r] = -1, np.inf                        # a closed row
        for lam in (0.0, 0.25, 2.0):
            vs, vc, vcost = P.best_path(idx, dist, mu, next_of, lam)
            slot, choice, cost = G.fixed_lag(idx, dist, mu, next_of, lam, lag)
            assert np.array_equal(slot, vs) and np.array_equal(choice, vc) and np.array_equal(cost, vcost), (trial, lam)


def test_one_frame_of_look_ahead_finds_the_two_file_path():
    mu, q, next_of = P.two_file_case(40, 8, 0)
    idx, dist = O.knn(q, mu, 2)
    w = 3 / 16
    _, gc, _, gcost = LO.greedy(idx, dist, mu, next_of, w)
    assert gcost[0] + w * gcost[1] == 12.9375 and G.switches(gc, 40) == 39     # a file switch at every frame
    vs, vc, vcost = P.best_path(idx, dist, mu, next_of, w)
    assert vcost[0] + w * vcost[1] == 10.5625
    for lag in (1, 2, 3, 8, 39, 64):
        slot, choice, cost = G.fixed_lag(idx, dist, mu, next_of, w, lag)
        assert cost[0] + w * cost[1] == 10.5625, lag
        assert G.switches(choice, 40) == 1, lag


def test_schedule_orders_commits_and_drains():
    last, emit, T = G.schedule("pppdd", 2, 3)
    assert T == 6 and emit.tolist() == [-1, -1, -1, 0, 1, 2, 3, 4, 5, -1]
    assert last.tolist() == [3, 4, 5, 5, 5, 5]
    last, emit, T = G.schedule("pdp", 2, 1)                      # drained dry, then fed again
    assert emit.tolist() == [-1, 0, 1, -1, -1, 2] and last.tolist() == [1, 1, 3, 3]
    last, emit, T = G.schedule("pp", 1, 0)
    assert emit.tolist() == [0, 1] and last.tolist() == [0, 1]


def _header():
    with open(os.path.join(REPO, "include", "rawvae_hip.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def test_header_adds_the_drain_op_and_nothing_else(tmp_path):
    from rawaudiovae_kelsey_amd import _lib
    src = _header()
    names = sorted(set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", src)))
    assert len(names) <= 70
    for name, num in OPS.items():
        assert re.search(r"#define RV_MOSAIC_%s %d\b" % (name, num), src), name
        assert getattr(_lib, "MOSAIC_" + name) == num
    assert len(re.findall(r"#define RV_MOSAIC_[A-Z_]+ \d+", src)) == len(OPS)
    assert len(abi_slots.check_layout()) == 37 and C.sizeof(_lib.MosaicDesc) == 37 * 8
    c = tmp_path / "c.c"
    c.write_text('#include "rawvae_hip.h"\nint main(void) { rv_stream_desc s = {0}; rv_mosaic_desc d = {0}; d.live = &s; '
                 'd.rows = 8; return rv_mosaic(RV_MOSAIC_LIVE_DRAIN, &d, 0) + (int)sizeof(d) - 37 * 8; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(c), "-o",
                    str(tmp_path / "c.o")], check=True)


def _live_ws_bytes(lag, weight=True, n_streams=1, block=256, hop=256, S=1024, L=256, N=1240000, k=4):
    from rawaudiovae_kelsey_amd import _lib
    sd = _lib.StreamDesc(S=S, H=2048, L=L, n_streams=n_streams, block=block, hop=hop)
    d = _lib.MosaicDesc(k=k, N=N, L=L, live=C.pointer(sd), rows=lag, weight=0x1000 if weight else None)
    _lib.lib().rv_mosaic(_lib.MOSAIC_LIVE_WORKSPACE, C.byref(d), None)   # the pointer is not read: no device is touched
    return d.ws_bytes


def test_live_workspace_grows_with_the_lag_and_rejects_bad_lags():
    from rawaudiovae_kelsey_amd import _lib
    base = _live_ws_bytes(0)
    assert base == _live_ws_bytes(0, weight=False) and base % 256 == 0
    sizes = [_live_ws_bytes(D) for D in (0, 1, 4, 16, 64)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and all(s % 256 == 0 for s in sizes)
    # the ring of D + 1 rows of idx[k], dist[k] and trans[k, k] per stream, each part rounded up to 256 bytes, + (head, count)
    k, D = 16, 64
    ring = (D + 1) * k * (k + 2) * 4
    grown = _live_ws_bytes(D, k=k) - _live_ws_bytes(0, k=k)
    assert ring + 8 <= grown <= ring + 4 * 256
    assert _live_ws_bytes(D, k=k, n_streams=16, block=1024) - _live_ws_bytes(0, k=k, n_streams=16, block=1024) >= 16 * ring
    for bad in (65, -1, 1 << 40):
        with pytest.raises(_lib.RvError, match="lag"):
            _live_ws_bytes(bad)
    with pytest.raises(_lib.RvError, match="lag"):
        _live_ws_bytes(3, weight=False)


def test_validator_names_the_lag():
    from rawaudiovae_kelsey_amd.mosaic import LAG_MAX, check_live_args
    ok = dict(segment_length=64, index_step=16, n_corpus=100, n_streams=2, block=32, hop=16, k=4, mode="grains",
              window="hann", continuity=0.5)
    assert LAG_MAX == 64
    assert check_live_args(**ok) == check_live_args(**dict(ok, lag=0)) == check_live_args(**dict(ok, lag=64)) == (16, 48, 2, 1)
    assert check_live_args(**dict(ok, continuity=0.0, lag=0)) == (16, 48, 2, 1)
    for bad in (-1, 65, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="lag"):
            check_live_args(**dict(ok, lag=bad))
    with pytest.raises(ValueError, match="lag"):
        check_live_args(**dict(ok, continuity=0.0, lag=2))


def test_cli_lag_flag(tmp_path):
    sys.path.insert(0, REPO)
    import mosaic as cli
    from rawaudiovae_kelsey_amd import data as D
    r = subprocess.run([sys.executable, os.path.join(REPO, "mosaic.py"), "--help"], capture_output=True, text=True, cwd=REPO)
    assert r.returncode == 0 and "--lag" in r.stdout
    assert "--lag" in cli.__doc__
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    D.write_wav(corpus / "a.wav", np.zeros(640, np.float32), 8000)
    base = ["--config", "none.ini", "--checkpoint", "none.pt", "--target", "t.wav", "--out", "o.wav", "--corpus", str(corpus)]
    live = ["--live-block", "64", "--continuity", "0.5"]
    for extra in (["--lag", "2"], ["--lag", "2", "--continuity", "0.5"], ["--live-block", "64", "--lag", "2"],
                  ["--live-block", "64", "--continuity", "0", "--lag", "1"], live + ["--lag", "65"], live + ["--lag", "-1"],
                  live + ["--lag", "x"]):
        with pytest.raises(ValueError, match="--lag"):
            cli.parse_args(base + extra)
    assert cli.parse_args(base + live + ["--lag", "8"]).lag == 8
    assert cli.parse_args(base + live).lag == 0 and cli.parse_args(base).lag == 0
    assert cli.parse_args(base + ["--live-block", "64", "--lag", "0"]).lag == 0
