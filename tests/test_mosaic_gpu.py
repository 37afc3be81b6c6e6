"""Latent mosaicing on the GPU (csrc/mosaic*.hip, rawaudiovae_kelsey_amd/mosaic.py, mosaic.py) against the numpy
restatement in tests/mosaic_oracle.py."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from conftest import REPO  # noqa: E402
import mosaic_oracle as O  # noqa: E402
import stream_oracle as SO  # noqa: E402


def _M():
    from rawaudiovae_kelsey_amd import mosaic
    return mosaic


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _check_knn(q, c, k, splits=0):
    idx, dist = _M().knn_topk(_dev(q), _dev(c), k, splits=splits)
    ri, rd = O.knn(q, c, k)
    gi, gd = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(gi, ri), np.argwhere(gi != ri)[:5]
    assert np.array_equal(gd.view(np.int32), rd.view(np.int32))
    return gi, gd


@pytest.mark.parametrize("T,N,L,k", [(1, 70001, 256, 16), (300, 5000, 64, 1), (1000, 1000, 100, 16), (4097, 33, 7, 4)])
def test_knn_matches_the_oracle_exactly(T, N, L, k):
    rng = np.random.default_rng(T + N)
    c = rng.standard_normal((N, L)).astype(np.float32)
    q = rng.standard_normal((T, L)).astype(np.float32)
    q[: min(T, 3)] = c[[N // 2, 0, N - 1][: min(T, 3)]]        # exact hits: distance 0
    gi, gd = _check_knn(q, c, k)
    assert gi[0, 0] == N // 2 and gd[0, 0] == 0


def test_knn_ties_go_to_the_lower_index_and_nan_never_wins():
    rng = np.random.default_rng(5)
    base = rng.standard_normal((50, 24)).astype(np.float32)
    c = np.concatenate([base, base[::-1], base[:10]])            # every row two or three times
    q = np.concatenate([base[:20], rng.standard_normal((30, 24)).astype(np.float32)])
    for splits in (0, 1, 3):
        gi, gd = _check_knn(q, c, 8, splits)
    assert np.all(gi[:10, 0] == np.arange(10)) and np.all(gi[:10, 1] == 99 - np.arange(10))
    assert np.all(gi[:10, 2] == 100 + np.arange(10)) and np.all(gd[:10, :3] == 0)
    cn = c.copy()
    cn[::2, 5] = np.nan                                          # half the corpus is NaN
    qn = q.copy()
    qn[7] = np.nan                                               # a query with no candidate at all
    gi, gd = _check_knn(qn, cn, 16, 3)
    assert np.all(np.delete(gi, 7, axis=0)[:, 0] % 2 == 1)   # only the odd (finite) corpus rows are taken
    assert np.all(gi[7] == -1) and np.all(np.isinf(gd[7]))


def test_knn_pads_rows_with_fewer_finite_candidates():
    rng = np.random.default_rng(6)
    c = np.full((40, 9), np.nan, np.float32)
    c[[3, 17, 38]] = rng.standard_normal((3, 9))
    q = rng.standard_normal((130, 9)).astype(np.float32)
    for splits in (0, 1, 3):
        gi, gd = _check_knn(q, c, 5, splits)
        assert np.array_equal(np.sort(gi[:, :3], axis=1), np.tile([3, 17, 38], (130, 1)))
        assert np.all(gi[:, 3:] == -1) and np.all(np.isinf(gd[:, 3:]))


@pytest.mark.parametrize("N,M,L", [(1000, 700, 64), (300, 5000, 33), (5, 2, 256),
                                   (129, 65, 33),     # one past a row block, a column tile and a K tile at once
                                   (128, 64, 32)])    # exactly one full tile: no padding path at all
def test_knn_k_le_2_is_som_bmu_bit_for_bit(N, M, L):
    from rawaudiovae_kelsey_amd import som
    rng = np.random.default_rng(N + M)
    x = _dev(rng.standard_normal((N, L)))
    w = _dev(rng.standard_normal((M, L)))
    best, second, d_best, d_second = som.bmu(x, w)
    for k in (1, 2):
        idx, dist = _M().knn_topk(x, w, k)
        assert torch.equal(idx[:, 0], best) and torch.equal(dist[:, 0].view(torch.int32), d_best.view(torch.int32))
        if k == 2:
            assert torch.equal(idx[:, 1], second)
            assert torch.equal(dist[:, 1].view(torch.int32), d_second.view(torch.int32))


@pytest.mark.parametrize("T,N,L,k", [(1, 70001, 256, 16), (344, 20000, 64, 4), (1000, 1000, 100, 3)])
def test_knn_does_not_depend_on_the_split_count(T, N, L, k):
    rng = np.random.default_rng(11)
    q = _dev(rng.standard_normal((T, L)))
    c = _dev(rng.standard_normal((N, L)))
    ref = _M().knn_topk(q, c, k, splits=1)
    for s in (3, 0, 7):
        got = _M().knn_topk(q, c, k, splits=s)
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))


def test_gather_mean_and_ola_match_the_oracle_bit_for_bit():
    from rawaudiovae_kelsey_amd.stream import window_values
    M = _M()
    rng = np.random.default_rng(8)
    src = rng.standard_normal(20000).astype(np.float32)
    starts = np.sort(rng.choice(20000 - 96, 300, replace=False)).astype(np.int64)
    idx = rng.integers(-1, 300, (257, 7)).astype(np.int32)
    got = M.gather_mean(_dev(src), torch.from_numpy(idx).cuda(), 96, row_start=torch.from_numpy(starts).cuda())
    assert np.array_equal(got.cpu().numpy(), O.gather_mean(src, starts, idx, 96))
    mu = rng.standard_normal((300, 24)).astype(np.float32)
    got = M.gather_mean(_dev(mu), torch.from_numpy(idx).cuda(), 24, stride=24)
    assert np.array_equal(got.cpu().numpy(), O.gather_mean(mu.reshape(-1), np.arange(300) * 24, idx, 24))
    frames = rng.standard_normal((41, 64)).astype(np.float32)
    for hop, win, n_out in ((64, None, 41 * 64), (64, None, 41 * 64 - 9), (16, "hann", 40 * 16 + 64), (32, "hann", 1000),
                            (8, None, 40 * 8 + 64 + 50)):
        w = None if win is None else window_values(64, win)
        got = M.ola(_dev(frames), hop, n_out, None if w is None else _dev(w)).cpu().numpy()
        assert np.array_equal(got, O.ola(frames, hop, n_out, w)), (hop, win, n_out)


def _model(S=64, H=96, L=8, seed=0):
    from rawvae.model import VAE
    torch.manual_seed(seed)
    return VAE(S, H, L).cuda().eval()


def _corpus(rng, lengths):
    out = []
    for i, n in enumerate(lengths):
        t = np.arange(n) / 8000.0
        w = 0.6 * np.sin(2 * np.pi * (150 + 170 * i) * t) + 0.2 * rng.standard_normal(n)
        w[: n // 5] = 0                                          # leading silence: duplicate all-zero frames
        out.append(w.astype(np.float32))
    return out


def test_identity_the_target_is_a_corpus_file():
    M = _M()
    m = _model()
    rng = np.random.default_rng(9)
    waves = _corpus(rng, [700, 1000, 513, 1290])
    for hop, win, exact in ((None, None, True), (64, None, True), (16, "hann", False)):
        index = M.LatentIndex(m, hop=hop)
        for i, w in enumerate(waves):
            index.add(w, "f%d" % i)
        target = waves[2]
        y, idx, dist = index.mosaic(target, k=1, mode="grains", window=win, return_matches=True)
        y = y.cpu().numpy()
        assert y.shape == target.shape and np.all(dist.cpu().numpy() == 0)
        if exact:
            assert np.array_equal(y, target), np.abs(y - target).max()
        else:
            assert y[0] == 0                                      # Hann: the window sum is 0 at t = 0 only
            assert np.abs(y[1:] - target[1:]).max() <= 1e-6
        names = index.locate(idx)
        assert all(n in ("f0", "f1", "f2", "f3") for row in names for n, _ in row)


def test_grains_and_decode_follow_the_oracle_and_not_max_rows():
    from rawaudiovae_kelsey_amd.interpolate import LatentInterpolator
    from rawaudiovae_kelsey_amd.stream import window_values
    M = _M()
    m = _model(seed=2)
    rng = np.random.default_rng(10)
    waves = _corpus(rng, [900, 333, 1500])
    target = (0.5 * np.sin(np.arange(1111) * 0.07) + 0.1 * rng.standard_normal(1111)).astype(np.float32)
    p = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}
    enc = LatentInterpolator(m)
    for hop, win, k in ((16, "hann", 3), (None, None, 2), (32, None, 4)):
        outs = {}
        for max_rows in (16384, 7, 1):
            index = M.LatentIndex(m, hop=hop, max_rows=max_rows)
            for i, w in enumerate(waves):
                index.add(w, "w%d" % i)
            for mode in ("grains", "decode"):
                outs[(max_rows, mode)] = index.mosaic(target, k=k, mode=mode, window=win,
                                                      return_matches=True)
        for mode in ("grains", "decode"):
            y, idx, dist = [t.cpu().numpy() for t in outs[(16384, mode)]]
            for mr in (7, 1):
                assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(outs[(mr, mode)], (y, idx, dist)))
        # the search is the oracle's on the encoder's own mu
        mu_t = enc.encode_audio(target, hop=hop)[0].cpu().numpy()
        ri, rd = O.knn(mu_t, index.mu.cpu().numpy(), k)
        assert np.array_equal(idx, ri) and np.array_equal(dist, rd)
        step = 64 if hop is None else hop
        w = None if win is None else window_values(64, win)
        y_g = outs[(16384, "grains")][0].cpu().numpy()
        grains = O.gather_mean(index.audio.cpu().numpy(), index.row_start, idx, 64)
        assert np.array_equal(y_g, O.ola(grains, step, target.size, w))
        # decode: the mean of the neighbours' mu through a float64 decoder, overlap-added in float64
        z = index.mu.cpu().numpy().astype(np.float64)[idx].mean(1)
        h3 = np.maximum(z @ p["fc3.weight"].T + p["fc3.bias"], 0.0)
        dec = np.tanh(h3 @ p["fc4.weight"].T + p["fc4.bias"])
        ref = SO.wola(dec, np.ones(64) if w is None else w, step, target.size)
        y_d = outs[(16384, "decode")][0].cpu().numpy()
        assert np.abs(y_d - ref).max() <= 2e-6, np.abs(y_d - ref).max()


def test_cli_writes_the_mosaic_and_the_matches(tmp_path):
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd import data as D
    S_, H, L, sr = 64, 128, 8, 8000
    torch.manual_seed(3)
    torch.save({"epoch": 1, "state_dict": VAE(S_, H, L).state_dict(), "optimizer": {}}, tmp_path / "ckpt_00001")
    (tmp_path / "tiny.ini").write_text("[audio]\nsampling_rate = %d\nhop_length = 8\nsegment_length = %d\n"
                                       "[VAE]\nlatent_dim = %d\nn_units = %d\n" % (sr, S_, L, H))
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    rng = np.random.default_rng(4)
    for i, w in enumerate(_corpus(rng, [400, 777, 1024])):
        D.write_wav(corpus / ("c%d.wav" % i), w, sr)
    target = (0.3 * rng.standard_normal(999)).astype(np.float32)
    D.write_wav(tmp_path / "t.wav", target, sr)
    run = [sys.executable, os.path.join(REPO, "mosaic.py"), "--config", str(tmp_path / "tiny.ini"), "--checkpoint",
           str(tmp_path / "ckpt_00001"), "--corpus", str(corpus), "--target", str(tmp_path / "t.wav"), "--out",
           str(tmp_path / "out.wav"), "--hop", "16", "--k", "3", "--mode", "grains", "--window", "hann", "--matches",
           str(tmp_path / "m.csv")]
    subprocess.run(run, check=True, timeout=300, cwd=str(tmp_path))
    y, got_sr = D.read_wav(tmp_path / "out.wav")
    assert got_sr == sr and y.size == target.size and np.all(np.isfinite(y))
    rows = list(csv.reader(open(tmp_path / "m.csv")))
    T = (-(-target.size // 16) * 16) // 16 - 64 // 16 + 1
    assert len(rows) == T and all(len(r) == 9 for r in rows)
    assert all(r[0] in ("c0.wav", "c1.wav", "c2.wav") and int(r[1]) % 16 == 0 for r in rows)
    assert all(float(r[2]) <= float(r[5]) <= float(r[8]) for r in rows)
    subprocess.run(run[:-2] + ["--mode", "decode", "--window", "none", "--hop", "64"], check=True, timeout=300,
                   cwd=str(tmp_path))
    y, _ = D.read_wav(tmp_path / "out.wav")
    assert y.size == target.size and np.all(np.isfinite(y))
