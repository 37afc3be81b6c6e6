"""Continuity-aware mosaicing without a GPU: the numpy oracle of the Viterbi unit selection against brute force and on
a construction with a known answer, the header's new ops and fields, the successor table and the command line's flag
(tests/mosaic_path_oracle.py, include/rawvae_hip.h, rawaudiovae_kelsey_amd/mosaic.py, mosaic.py)."""
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
import mosaic_oracle as O  # noqa: E402
import mosaic_path_oracle as P  # noqa: E402


def test_oracle_path_is_the_brute_force_optimum():
    """T = 7, k = 3, dyadic latents (every fp32 operation is exact), closed rows, short rows, lambda in {0, 1/4, 2}:
    on every maximal run of open rows the oracle's path costs exactly the minimum over all k^len paths."""
    rng = np.random.default_rng(3)
    T, k, N, L = 7, 3, 30, 8
    n = 0
    for trial in range(300):
        mu = (rng.integers(-4, 5, (N, L)) / 2).astype(np.float32)
        q = (rng.integers(-4, 5, (T, L)) / 2).astype(np.float32)
        idx, dist = O.knn(q, mu, k)
        if trial % 3 == 0:
            r = rng.integers(0, T)
            idx[r], dist[r] = -1, np.inf                       # a closed row
        if trial % 5 == 0:
            r = rng.integers(0, T)
            idx[r, 2], dist[r, 2] = -1, np.inf                 # a short row
        next_of = np.minimum(np.arange(N) + 1, N - 1).astype(np.int32)
        tr = P.transitions(mu, idx, next_of)
        closed = (idx < 0).all(1)
        for lam in (0.0, 0.25, 2.0):
            slot, choice, cost = P.best_path(idx, dist, mu, next_of, lam, tr=tr)
            assert np.array_equal(slot < 0, closed)
            assert np.array_equal(choice, np.where(closed, -1, idx[np.arange(T), np.maximum(slot, 0)]))
            if lam == 0:
                assert np.all(slot[~closed] == 0)
            total = 0.0
            t0 = 0
            while t0 < T:
                if closed[t0]:
                    t0 += 1
                    continue
                t1 = t0
                while t1 < T and not closed[t1]:
                    t1 += 1
                paths = np.array(list(itertools.product(range(k), repeat=t1 - t0)))
                u = np.arange(t0, t1)
                J = dist[u[None, :], paths].astype(np.float64).sum(1)
                if t1 - t0 > 1:
                    trs = tr[u[None, 1:], paths[:, :-1], paths[:, 1:]].astype(np.float64).sum(1)
                    J = J + np.where(np.isinf(trs), np.inf, lam * np.where(np.isinf(trs), 0, trs))   # no 0 * inf
                got = P.path_cost(slot[t0:t1], dist[t0:t1], tr[t0:t1], lam)
                assert np.isfinite(got) and got == J.min(), (trial, lam, t0, t1)
                total += got
                t0 = t1
            assert cost[0] + lam * cost[1] == total            # the reported sums are the path's own
            n += 1
    assert n == 900


def test_two_file_construction_jumps_below_and_stays_above_the_break_even_weight():
    F = 40
    mu, q, next_of = P.two_file_case(F)
    idx, dist = O.knn(q, mu, 2)
    assert np.array_equal(np.sort(idx, 1), np.stack([np.arange(F), np.arange(F) + F], 1))
    assert np.array_equal(idx[:, 0] >= F, np.arange(F) % 2 == 1)      # the nearer file alternates
    tr = P.transitions(mu, idx, next_of)
    for lam, jumps in ((0.0, 39), (1 / 32, 39), (1.0, 0)):
        slot, choice, cost = P.best_path(idx, dist, mu, next_of, lam, tr=tr)
        assert int((choice[1:] != next_of[choice[:-1]]).sum()) == jumps, lam
        assert cost[1] == jumps                                        # every jump costs |e_0|^2 = 1
        near, far = F * (3 / 8) ** 2, (F // 2) * ((3 / 8) ** 2 + (5 / 8) ** 2)
        assert cost[0] == (near if jumps else far)


def test_oracle_chosen_successor_costs_exactly_zero_and_missing_is_inf():
    rng = np.random.default_rng(4)
    mu = rng.standard_normal((20, 37)).astype(np.float32)
    mu[7] = np.nan
    next_of = np.minimum(np.arange(20) + 1, 19).astype(np.int32)
    idx = np.array([[3, 5, -1], [4, 7, 9], [8, 5, 10], [-1, -1, -1], [2, 3, 4]])
    tr = P.transitions(mu, idx, next_of)
    assert np.all(tr[0] == 0)
    assert tr[1, 0, 0] == 0 and tr[2, 0, 1] == 0 and tr[2, 2, 2] == 0     # 3 -> 4, 4 -> 5, 9 -> 10 play on: exactly 0
    assert tr[2, 1, 0] == 0                                              # the successor of the NaN row 7 is row 8
    assert np.all(np.isinf(tr[1, 2])) and np.all(np.isinf(tr[1, :, 1]))  # a -1 predecessor; a NaN corpus row
    assert np.isfinite(tr[2]).all() and (tr[2] > 0).sum() == 6
    assert np.all(np.isinf(tr[3])) and np.all(np.isinf(tr[4]))           # into and out of a closed row


def _header():
    with open(os.path.join(REPO, "include", "rawvae_hip.h")) as f:
        return f.read()


def test_header_adds_ops_and_fields_but_no_entry_point(tmp_path):
    from rawaudiovae_kelsey_amd import _lib, mosaic
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert len(set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", src))) <= 70
    c = tmp_path / "c.c"
    c.write_text('#include "rawvae_hip.h"\n'
                 'int main(void) { rv_mosaic_desc d = {0}; int nx[2] = {1, 1}; int s[2]; double cost[2]; float tr[4];\n'
                 '  d.next_of = nx; d.row0 = 0; d.rows = 2; d.trans = tr; d.lam = 0.5f; d.slot = s; d.choice = s;\n'
                 '  d.cost = cost;\n'
                 '  return RV_MOSAIC_TRANSITION + RV_MOSAIC_PATH_FORWARD + RV_MOSAIC_PATH_BACKTRACK\n'
                 '         + RV_MOSAIC_PATH_WORKSPACE + (int)sizeof(d) > 0 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(c), "-o",
                    str(tmp_path / "c.o")], check=True)
    # _lib mirrors the header: the constants' values, and the struct's field names in order
    for name in ("KNN", "KNN_WORKSPACE", "GATHER_MEAN", "OLA", "TRANSITION", "PATH_FORWARD", "PATH_BACKTRACK",
                 "PATH_WORKSPACE"):
        assert int(re.search(r"#define RV_MOSAIC_%s (\d+)" % name, src).group(1)) == getattr(_lib, "MOSAIC_" + name)
    fields = abi_slots.check_layout()    # the slots' first names, the same in the header and in _lib
    assert fields[:25] == ["T", "k", "idx", "q", "c", "N", "L", "splits", "dist", "ws", "ws_bytes", "src", "src_len",
                           "row_start", "stride", "n_rows", "width", "out", "ldo", "frames", "F", "S", "hop", "window",
                           "n_out"]                                      # the existing fields stay where they were
    # the workspace query touches no device: it covers back and the met transition per (t, j), end per t, the scores
    for T, k in ((1, 1), (20700, 16), (4097, 3)):
        n = mosaic.path_workspace_bytes(T, k)
        assert n >= T * k * 5 + T + 4 * k and n <= T * k * 5 + T + 256 and n % 16 == 0
    for bad in ((0, 4), (10, 0), (10, 17), (-3, 2)):
        with pytest.raises(_lib.RvError):
            mosaic.path_workspace_bytes(*bad)


def test_successor_table_on_a_three_file_layout():
    from rawaudiovae_kelsey_amd.mosaic import frame_tables, successor_table
    n_frames, _, _, file_of, _ = frame_tables([64 * 3, 64 * 1, 64 * 4 + 5], 64, None)
    assert list(n_frames) == [3, 1, 5]
    nxt = successor_table(file_of)
    assert nxt.dtype == np.int32 and list(nxt) == [1, 2, 2, 3, 5, 6, 7, 8, 8]
    assert list(successor_table(file_of, 2)) == [2, 1, 2, 3, 6, 7, 8, 7, 8]
    assert list(successor_table(file_of, 2.0)) == [2, 1, 2, 3, 6, 7, 8, 7, 8]
    for bad in (1.5, 0, -1, 0.5, float("nan")):
        with pytest.raises(ValueError, match="hop"):
            successor_table(file_of, bad)


def test_cli_continuity_flag(tmp_path):
    sys.path.insert(0, REPO)
    import mosaic as cli
    r = subprocess.run([sys.executable, os.path.join(REPO, "mosaic.py"), "--help"], capture_output=True, text=True,
                       cwd=REPO)
    assert r.returncode == 0 and "--continuity" in r.stdout
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    base = ["--config", "none.ini", "--checkpoint", "none.pt", "--target", "t.wav", "--out", str(tmp_path / "o.wav"),
            "--corpus", str(corpus)]
    for bad in ("-1", "nan", "abc", "inf", "-0.5"):
        with pytest.raises(ValueError, match="--continuity"):
            cli.parse_args(base + ["--continuity", bad])
    assert cli.parse_args(base).continuity == 0.0
    assert cli.parse_args(base + ["--continuity", "0.25"]).continuity == 0.25
    assert cli.continuing_share(np.array([4, 5, 6, 2, 3, -1, 9]), np.minimum(np.arange(10) + 1, 9)) == 3 / 6
