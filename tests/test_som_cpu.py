"""SOM of a corpus's latents without a GPU: the float64 numpy SOM (tests/som_oracle.py) itself, the som/ files and the
notebook's way of reading them (tutorial.ipynb:725-756), the flags of som.py and interpolate.py, and the C header."""
import json
import os
import pathlib
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from conftest import REPO

import interpolate as icli  # noqa: E402  (entry points at the repository root)
import som as scli  # noqa: E402
import som_oracle as O  # noqa: E402
from rawaudiovae_kelsey_amd import _lib, frontend  # noqa: E402
from rawaudiovae_kelsey_amd import som as S  # noqa: E402

torch = pytest.importorskip("torch")

CENTERS = [[0, 0, 0, 0], [8, 0, 0, 0], [0, 8, 0, 0], [0, 0, 8, 0], [0, 0, 0, 8], [8, 8, 8, 8]]


def test_oracle_recovers_separated_clusters():
    x, lab = O.blobs(40, CENTERS, 0.2, seed=3)
    w, best = O.fit(x, 2, 3, sigma1=0.1, epochs=20, seed=1)
    nodes = [np.unique(best[lab == k]) for k in range(len(CENTERS))]
    assert all(n.size == 1 for n in nodes)                        # each cluster on one node
    assert len({int(n[0]) for n in nodes}) == len(CENTERS)       # distinct nodes
    for k, n in enumerate(nodes):
        np.testing.assert_allclose(w[n[0]], x[lab == k].mean(0), atol=1e-6)


def test_sigma_to_zero_is_a_kmeans_step():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((500, 5))
    w0 = rng.standard_normal((12, 5))
    w0[11] = 100.0                                               # a node nobody picks keeps its weights
    best = O.bmu(x, w0)[0]
    sums, counts = O.node_sums(x, best, 12)
    w1 = O.update(sums, counts, w0, 3, 4, 1e-3)
    for m in range(12):
        ref = x[best == m].mean(0) if (best == m).any() else w0[m]
        np.testing.assert_allclose(w1[m], ref, rtol=1e-12, atol=1e-12)
    assert counts[11] == 0 and counts.sum() == 500


def test_oracle_bmu_ties_and_order():
    w = np.array([[1.0, 2.0], [3.0, 4.0], [1.0, 2.0], [0.0, 0.0]])
    best, second, d1, d2 = O.bmu(np.array([[1.0, 2.0], [0.1, 0.1]]), w)
    assert best.tolist() == [0, 3] and second.tolist() == [2, 0]
    assert d1[0] == 0 and d2[0] == 0


def test_sigma_schedule():
    np.testing.assert_allclose(S.sigma_schedule(4.0, 0.5, 5), 4.0 * (0.125 ** (np.arange(5) / 4)), rtol=0, atol=0)
    assert S.sigma_schedule(3.0, 0.5, 1).tolist() == [3.0]
    som = S.LatentSOM(4, 6)
    assert som.sigma0 == 3.0 and som.sigma1 == 0.5 and som.epochs == 50 and som.M == 24
    for bad in (dict(rows=1, cols=1), dict(rows=2, cols=2, sigma0=0), dict(rows=2, cols=2, epochs=0)):
        with pytest.raises(ValueError):
            S.LatentSOM(**bad)


def _stub_som(rows, cols, L):
    return types.SimpleNamespace(rows=rows, cols=cols, M=rows * cols, weights=torch.zeros(rows, cols, L),
                                 sigmas=S.sigma_schedule(2.0, 0.5, 3), sigma0=2.0, sigma1=0.5, seed=7, epochs=3)


def notebook_concat_paths(audio_files, cluster_idx, som_clusters_dict, som_data_dict):
    """tutorial.ipynb:743-756, concat_audio_som, with librosa.load replaced by a recorder of the paths it loads."""
    loaded = []
    librosa = types.SimpleNamespace(load=lambda path, sr=None: (loaded.append(str(path)) or np.zeros(1), sr))
    init = True
    cluster = som_clusters_dict[str(cluster_idx)]
    for index in cluster:
        path = som_data_dict[str(index)][1]
        path = audio_files.joinpath(path)
        y, fs = librosa.load(path, sr=None)
        if init:
            audio = y
        else:
            audio = np.concatenate((audio, y), 0)
        init = False
    return loaded


def test_write_read_round_trip_and_the_notebooks_reader(tmp_path):
    files = ["a.wav", "b.wav", "c.wav", "d.wav", "e.wav"]
    assign = np.array([3, 0, 3, 5, 0])
    S.write_som(str(tmp_path), files, assign, _stub_som(2, 3, 4))
    clusters, data = S.read_som(str(tmp_path))
    assert clusters == {"0": [1, 4], "1": [], "2": [], "3": [0, 2], "4": [], "5": [3]}   # every node, ascending
    assert data == {str(i): [int(assign[i]), f] for i, f in enumerate(files)}
    # the notebook's own loading code (tutorial.ipynb:725-732) on the written files
    with open(tmp_path / "clusters.json", "r") as f:
        som_clusters_dict = json.load(f)
    with open(tmp_path / "data-concatenated.json", "r") as f:
        som_data_dict = json.load(f)
    audio = pathlib.Path(tmp_path / "audio")
    for k in range(6):
        assert notebook_concat_paths(audio, k, som_clusters_dict, som_data_dict) == \
            S.cluster_paths(clusters, data, str(audio), k)
    z = np.load(tmp_path / "som.npz")
    assert z["grid"].tolist() == [2, 3] and z["weights"].shape == (2, 3, 4) and int(z["seed"]) == 7
    assert z["sigmas"].size == 3 and int(z["hop"]) == -1 and z["assignment"].tolist() == assign.tolist()


def test_read_som_accepts_an_outside_trainers_files(tmp_path):
    """Sparse clusters (empty nodes left out), extra fields per entry, subfolders in the relative paths."""
    (tmp_path / "clusters.json").write_text(json.dumps({"18": [2, 0], "24": [1]}))
    (tmp_path / "data-concatenated.json").write_text(json.dumps(
        {"0": [18, "x/one.wav", 0.5], "1": [24, "two.wav", 0.1], "2": [18, "x/three.wav", 0.7]}))
    clusters, data = S.read_som(str(tmp_path))
    assert S.cluster_paths(clusters, data, "/au", 18) == ["/au/x/three.wav", "/au/x/one.wav"]   # list order kept
    assert notebook_concat_paths(pathlib.Path("/au"), 18, clusters, data) == S.cluster_paths(clusters, data, "/au", 18)
    with pytest.raises(KeyError):
        S.cluster_paths(clusters, data, "/au", 3)


def test_som_cli_flags_are_validated(tmp_path):
    base = ["--checkpoint", "c", "--audio", str(tmp_path), "--out", str(tmp_path / "som")]
    a = scli.parse_args(base)
    assert (a.rows, a.cols, a.epochs, a.seed, a.hop, a.sigma0, a.sigma1, a.max_rows) == (8, 8, 50, 0, None, None, 0.5,
                                                                                          16384)
    a = scli.parse_args(base + ["--grid", "3x5", "--epochs", "7", "--sigma0", "2.5", "--hop", "128", "--seed", "4"])
    assert (a.rows, a.cols, a.epochs, a.sigma0, a.hop, a.seed) == (3, 5, 7, 2.5, 128, 4)
    for flags, name in ((["--grid", "8"], "--grid"), (["--grid", "1x1"], "--grid"), (["--grid", "axb"], "--grid"),
                        (["--epochs", "0"], "--epochs"), (["--epochs", "x"], "--epochs"), (["--sigma0", "0"], "--sigma0"),
                        (["--sigma1", "-1"], "--sigma1"), (["--sigma1", "nan"], "--sigma1"), (["--seed", "-2"], "--seed"),
                        (["--hop", "0"], "--hop"), (["--max-rows", "0"], "--max-rows")):
        with pytest.raises(ValueError, match=re.escape(name)):
            scli.parse_args(base + flags)
    with pytest.raises(ValueError, match="--audio"):
        scli.parse_args(["--checkpoint", "c", "--audio", str(tmp_path / "nope"), "--out", "o"])
    with pytest.raises(ValueError, match="--audio"):
        scli.corpus_files(str(tmp_path))


def test_som_cli_names_bad_wavs(tmp_path):
    from rawaudiovae_kelsey_amd import data as D
    D.write_wav(tmp_path / "empty.wav", np.zeros(0, np.float32), 8000)
    (tmp_path / "junk.wav").write_bytes(b"not a wav at all")
    D.write_wav(tmp_path / "ok.wav", np.ones(10, np.float32), 8000)
    assert scli.corpus_files(str(tmp_path)) == ["empty.wav", "junk.wav", "ok.wav"]
    for name in ("empty.wav", "junk.wav"):
        with pytest.raises(ValueError, match=re.escape(name)):
            frontend.load_wav(str(tmp_path / name), 8000)
    assert frontend.load_wav(str(tmp_path / "ok.wav"), 8000).size == 10


def test_interpolate_cluster_flags_are_validated(tmp_path):
    out = ["--checkpoint", "c", "--out", "o.wav"]
    som = ["--som", str(tmp_path), "--audio", str(tmp_path)]
    a = icli.parse_args(out + som + ["--a-cluster", "3", "--b", "b.wav"])
    assert a.a_cluster == 3 and a.a is None and a.b == "b.wav" and a.b_cluster is None
    a = icli.parse_args(out + ["--a", "a.wav", "--b", "b.wav"])
    assert a.a_cluster is None and a.som is None
    for flags, name in (([ "--b", "b.wav"], "--a"), (["--a", "a.wav", "--a-cluster", "1", "--b", "b.wav"] + som, "--a"),
                        (["--a", "a.wav"], "--b"), (["--a", "a.wav", "--b-cluster", "1"], "--b-cluster"),
                        (["--a-cluster", "1", "--b", "b.wav", "--som", str(tmp_path)], "--a-cluster"),
                        (["--a-cluster", "x", "--b", "b.wav"] + som, "--a-cluster"),
                        (["--a-cluster", "-1", "--b", "b.wav"] + som, "--a-cluster")):
        with pytest.raises(ValueError, match=re.escape(name)):
            icli.parse_args(out + flags)


def test_cluster_audio_is_concat_audio_som(tmp_path):
    from rawaudiovae_kelsey_amd import data as D
    rng = np.random.default_rng(5)
    waves = [rng.uniform(-1, 1, n).astype(np.float32) for n in (100, 37, 260)]
    for i, w in enumerate(waves):
        D.write_wav(tmp_path / ("f%d.wav" % i), w, 8000)
    S.write_som(str(tmp_path / "som"), ["f0.wav", "f1.wav", "f2.wav"], [1, 0, 1], _stub_som(1, 3, 2))
    got = icli.cluster_audio(str(tmp_path / "som"), str(tmp_path), 1, 8000, "--a-cluster")
    np.testing.assert_array_equal(got, np.concatenate([waves[0], waves[2]]))
    with pytest.raises(ValueError, match="--b-cluster 2"):
        icli.cluster_audio(str(tmp_path / "som"), str(tmp_path), 2, 8000, "--b-cluster")   # empty node
    with pytest.raises(ValueError, match="--a-cluster 9"):
        icli.cluster_audio(str(tmp_path / "som"), str(tmp_path), 9, 8000, "--a-cluster")   # missing node


def test_som_header_entries_compile_as_c(tmp_path):
    if not shutil.which("gcc"):
        pytest.skip("gcc not available")
    src = tmp_path / "som.c"
    src.write_text('#include "rawvae_hip.h"\n'
                   'int main(void) {\n'
                   '  int (*a)(const float*, long, long, const long long*, const long long*, long, float*, void*) =\n'
                   '      rv_segment_mean;\n'
                   '  int (*b)(const float*, long, const float*, long, long, int*, int*, float*, float*, void*) =\n'
                   '      rv_som_bmu;\n'
                   '  int (*c)(const float*, long, long, const int*, long, double*, long long*, void*) =\n'
                   '      rv_som_node_sums;\n'
                   '  int (*d)(const double*, const long long*, const float*, long, long, long, double, float*,\n'
                   '           void*) = rv_som_update;\n'
                   '  return (a != 0) + (b != 0) + (c != 0) + (d != 0) == 4 ? 0 : 1;\n}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(REPO, "include"), str(src), "-o",
                    str(tmp_path / "som.o")], check=True)
    assert {"rv_segment_mean", "rv_som_bmu", "rv_som_node_sums", "rv_som_update"} <= set(_lib.EXPORTED)


def test_node_sums_oracle_adds_in_ascending_row_order_bit_for_bit():
    rng = np.random.default_rng(21)
    N, L, M = 97, 5, 6
    x = (rng.standard_normal((N, L)) * 10.0 ** rng.integers(-6, 7, (N, L))).astype(np.float32)   # order matters
    best = rng.integers(-1, M + 2, N).astype(np.int32)           # -1, M and M + 1 belong to no node
    best[best == 3] = 2                                           # node 3 stays empty
    sums, counts = O.node_sums(x, best, M)
    ref = np.zeros((M, L), np.float64)
    n = [0] * M
    for r in range(N):
        if 0 <= best[r] < M:
            for l in range(L):
                ref[best[r], l] = ref[best[r], l] + float(x[r, l])
            n[best[r]] += 1
    assert np.array_equal(sums.view(np.int64), ref.view(np.int64)) and counts.tolist() == n and counts.dtype == np.int64
    assert n[3] == 0 and np.array_equal(sums[3].view(np.int64), np.zeros(L, np.int64))          # +0, not -0
    rev = np.zeros((M, L), np.float64)
    for r in range(N - 1, -1, -1):
        if 0 <= best[r] < M:
            rev[best[r]] += x[r].astype(np.float64)
    assert not np.array_equal(rev, ref)                           # the case does tell the orders apart
    inside = (best >= 0) & (best < M)                             # entries inside [0, M) alone: the result from before
    s2, c2 = O.node_sums(x[inside], best[inside], M)
    assert np.array_equal(s2.view(np.int64), sums.view(np.int64)) and np.array_equal(c2, counts)


def test_bmu_exact_agrees_with_the_float64_bmu_where_the_margin_is_clear():
    rng = np.random.default_rng(22)
    x = rng.standard_normal((200, 33)).astype(np.float32)
    w = rng.standard_normal((65, 33)).astype(np.float32)
    w[40] = w[7]                                                  # an exact tie: the lower index is best
    x[:2] = w[7]
    best, second, d1, d2 = O.bmu_exact(x, w)
    ob, os_, od1, od2 = O.bmu(x, w)
    assert best.dtype == second.dtype == np.int32 and d1.dtype == d2.dtype == np.float32
    assert best[0] == 7 and second[0] == 40 and d1[0] == 0 and d2[0] == 0
    # fp32 sums of 33 squares: each distance within 33 * 2^-24 relative of the float64 one
    clear = (od2 - od1) > 1e-5 * od2
    assert clear.sum() > 150 and np.array_equal(best[clear], ob[clear])
    np.testing.assert_allclose(d1, od1, rtol=1e-5, atol=0)
    np.testing.assert_allclose(d2, O.direct_dist(x, w, second), rtol=1e-5, atol=0)
    assert np.all(d1 <= d2) and np.all(best != second)
    wn, xn = w[:2].copy(), x[:5].copy()
    wn[1] = np.nan
    xn[3] = np.nan
    best, second, d1, d2 = O.bmu_exact(xn, wn)
    assert best.tolist() == [0, 0, 0, -1, 0] and second.tolist() == [-1] * 5
    assert np.isinf(d2).all() and np.isinf(d1[3]) and np.isfinite(np.delete(d1, 3)).all()


def test_segment_mean_oracle_is_the_float64_mean_rounded_once():
    rng = np.random.default_rng(23)
    lens = [1, 5, 1, 30, 2]
    x = (rng.standard_normal((sum(lens), 7)) * 10 + 3).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(lens)])
    got = O.segment_mean(x, off)
    assert got.dtype == np.float32 and got.shape == (5, 7)
    assert np.array_equal(got[0], x[0]) and np.array_equal(got[2], x[6])
    for f in range(5):
        s = [sum((float(v) for v in x[off[f]:off[f + 1], l]), 0.0) for l in range(7)]            # ascending, from +0
        assert np.array_equal(got[f], (np.array(s) / lens[f]).astype(np.float32))
