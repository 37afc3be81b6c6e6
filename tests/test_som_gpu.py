"""SOM kernels and API on the GPU (csrc/som.hip, rawaudiovae_kelsey_amd/som.py, som.py, interpolate.py --a-cluster)
against the float64 numpy SOM of tests/som_oracle.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from conftest import REPO  # noqa: E402
import som_oracle as O  # noqa: E402


def _S():
    from rawaudiovae_kelsey_amd import som
    return som


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def test_segment_mean_is_the_float64_mean_rounded():
    S = _S()
    rng = np.random.default_rng(0)
    lens = [1, 5, 1, 300, 2, 1, 77]
    x = (rng.standard_normal((sum(lens), 37)) * 10 + 3).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(lens)])
    got = S.segment_mean(_dev(x), off).cpu().numpy()
    for f in range(len(lens)):
        ref = x[off[f]:off[f + 1]].astype(np.float64).mean(0)
        ulp = np.spacing(np.abs(ref).astype(np.float32))
        assert np.all(np.abs(got[f].astype(np.float64) - ref) <= ulp), f
        if lens[f] == 1:
            np.testing.assert_array_equal(got[f], x[off[f]])
    from rawaudiovae_kelsey_amd._lib import RvError
    with pytest.raises(RvError, match="empty"):
        S.segment_mean(_dev(x), [0, 3, 3, 10])


def _check_bmu(x, w):
    S = _S()
    best, second, d1, d2 = (t.cpu().numpy() for t in S.bmu(_dev(x), _dev(w)))
    ob, os_, od1, od2 = O.bmu(x, w)
    # distances of the nodes the kernel chose, and the oracle's own, within 1e-5 relative
    np.testing.assert_allclose(d1, O.direct_dist(x, w, best), rtol=1e-5, atol=1e-30)
    np.testing.assert_allclose(d2, O.direct_dist(x, w, second), rtol=1e-5, atol=1e-30)
    np.testing.assert_allclose(d1, od1, rtol=1e-5, atol=1e-30)
    clear = (od2 - od1) > 1e-5 * od1
    assert np.array_equal(best[clear], ob[clear])
    assert np.all((best == ob) | (best == os_))
    assert np.all(best != second) and best.min() >= 0 and best.max() < w.shape[0]


@pytest.mark.parametrize("L", [1, 3, 64, 256, 300])
@pytest.mark.parametrize("M", [2, 64, 1000])
@pytest.mark.parametrize("N", [1, 333, 70001])
def test_bmu_matches_float64(N, M, L):
    rng = np.random.default_rng(N * 7 + M * 3 + L)
    x = rng.standard_normal((N, L)).astype(np.float32)
    w = rng.standard_normal((M, L)).astype(np.float32)
    _check_bmu(x, w)


@pytest.mark.parametrize("M,dups", [(64, (7, 40, 63)), (1000, (10, 500, 999)), (2, (0, 1))])
def test_bmu_exact_ties_pick_the_lower_index(M, dups):
    S = _S()
    rng = np.random.default_rng(M)
    L = 19
    w = rng.standard_normal((M, L)).astype(np.float32)
    for d in dups[1:]:
        w[d] = w[dups[0]]
    x = (w[dups[0]][None, :] + 0.01 * rng.standard_normal((500, L))).astype(np.float32)
    x[:3] = w[dups[0]]                                   # distance 0 to every copy
    best, second, d1, d2 = (t.cpu().numpy() for t in S.bmu(_dev(x), _dev(w)))
    assert np.all(best == dups[0]) and np.all(second == dups[1])
    np.testing.assert_array_equal(d1, d2)
    assert np.all(d1[:3] == 0)


def test_node_sums_and_update_match_float64_and_are_deterministic():
    S = _S()
    rng = np.random.default_rng(4)
    N, L, rows, cols = 50001, 70, 6, 7
    M = rows * cols
    x = rng.standard_normal((N, L)).astype(np.float32)
    best = rng.integers(0, M - 3, N).astype(np.int32)     # the last nodes stay empty
    xd, bd = _dev(x), torch.from_numpy(best).cuda()
    sums, counts = S.node_sums(xd, bd, M)
    sums2, counts2 = S.node_sums(xd, bd, M)
    assert torch.equal(sums, sums2) and torch.equal(counts, counts2)
    osums, ocounts = O.node_sums(x, best, M)
    np.testing.assert_array_equal(counts.cpu().numpy(), ocounts)
    np.testing.assert_allclose(sums.cpu().numpy(), osums, rtol=1e-6, atol=1e-9)
    w_old = rng.standard_normal((M, L)).astype(np.float32)
    for sigma in (3.0, 0.7, 1e-3):
        wn = S.update(sums, counts, _dev(w_old), rows, cols, sigma)
        wn2 = S.update(sums, counts, _dev(w_old), rows, cols, sigma)
        assert torch.equal(wn, wn2)
        ref = O.update(osums, ocounts, w_old, rows, cols, sigma)
        np.testing.assert_allclose(wn.cpu().numpy(), ref, rtol=1e-6, atol=1e-7)
    # sigma -> 0 keeps the empty nodes' weights bit for bit
    np.testing.assert_array_equal(wn.cpu().numpy()[M - 3:], w_old[M - 3:])


def test_fit_matches_the_oracle_on_separated_data():
    S = _S()
    rng = np.random.default_rng(9)
    centers = rng.uniform(-20, 20, (12, 16))
    x, lab = O.blobs(300, centers, 0.5, seed=2)
    som = S.LatentSOM(3, 4, epochs=25, seed=5).fit(_dev(x))
    w_ref, best_ref = O.fit(x, 3, 4, epochs=25, seed=5)
    best, second, dist = som.assign(_dev(x))
    np.testing.assert_array_equal(best.cpu().numpy(), best_ref)
    np.testing.assert_allclose(som.weights.cpu().numpy().reshape(12, 16), w_ref, rtol=1e-4, atol=1e-4)
    qe = som.quantization_error(_dev(x))
    assert abs(qe - np.sqrt(O.direct_dist(x, w_ref, best_ref)).mean()) <= 1e-4 * qe
    te = som.topographic_error(_dev(x))
    nb = S.grid_neighbours(best.long(), second.long(), 4).double().mean().item()
    assert 0.0 <= te <= 1.0 and abs(te - (1 - nb)) < 1e-12


def test_latent_map_is_one_mean_per_file_and_leaves_the_model():
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.interpolate import LatentInterpolator
    S = _S()
    torch.manual_seed(0)
    m = VAE(64, 96, 8).cuda().eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(1)
    waves = [rng.uniform(-1, 1, n).astype(np.float32) for n in (64, 1000, 257, 30)]
    for hop, ws in ((None, waves), (16, waves[:3])):   # 30 samples make no AudioDataset frame of 64
        desc = S.LatentMap(m, hop=hop).describe(ws).cpu().numpy()
        it = LatentInterpolator(m)
        for f, wv in enumerate(ws):
            mu = it.encode_audio(wv, hop=hop)[0].cpu().numpy().astype(np.float64)
            ref = mu.mean(0)
            assert np.all(np.abs(desc[f] - ref) <= np.spacing(np.abs(ref).astype(np.float32)))
    with pytest.raises(ValueError, match="waveform 3"):
        S.LatentMap(m, hop=16).describe(waves)
    assert all(torch.equal(before[k], v) for k, v in m.state_dict().items())


def test_cli_som_then_interpolate_by_cluster(tmp_path):
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd import data as D
    S_, H, L, sr = 64, 128, 8, 8000
    torch.manual_seed(3)
    m = VAE(S_, H, L)
    torch.save({"epoch": 1, "state_dict": m.state_dict(), "optimizer": {}}, tmp_path / "ckpt_00001")
    (tmp_path / "tiny.ini").write_text("[audio]\nsampling_rate = %d\nhop_length = 8\nsegment_length = %d\n"
                                       "[VAE]\nlatent_dim = %d\nn_units = %d\n" % (sr, S_, L, H))
    audio = tmp_path / "audio"
    audio.mkdir()
    rng = np.random.default_rng(7)
    for i in range(8):
        t = np.arange(200 + 97 * i) / sr
        D.write_wav(audio / ("s%02d.wav" % i), (0.8 * np.sin(2 * np.pi * (100 + 400 * (i % 4)) * t)
                                                + 0.05 * rng.standard_normal(t.size)).astype(np.float32), sr)
    run = [sys.executable, os.path.join(REPO, "som.py"), "--config", str(tmp_path / "tiny.ini"), "--checkpoint",
           str(tmp_path / "ckpt_00001"), "--audio", str(audio), "--out", str(tmp_path / "som"), "--grid", "2x2",
           "--epochs", "10"]
    subprocess.run(run, check=True, timeout=300, cwd=str(tmp_path))
    clusters = json.loads((tmp_path / "som" / "clusters.json").read_text())
    data = json.loads((tmp_path / "som" / "data-concatenated.json").read_text())
    assert sorted(clusters) == ["0", "1", "2", "3"] and sorted(sum(clusters.values(), [])) == list(range(8))
    assert [data[str(i)][1] for i in range(8)] == ["s%02d.wav" % i for i in range(8)]
    z = np.load(tmp_path / "som" / "som.npz")
    assert z["weights"].shape == (2, 2, L) and z["descriptors"].shape == (8, L) and np.isfinite(z["quantization_error"])
    full = [k for k in sorted(clusters, key=int) if clusters[k]]
    ka, kb = full[0], full[-1]
    for k, name in ((ka, "cat_a.wav"), (kb, "cat_b.wav")):
        D.write_wav(tmp_path / name, np.concatenate([D.load_audio_mono(audio / data[str(i)][1], sr)
                                                     for i in clusters[k]]), sr)
    common = [sys.executable, os.path.join(REPO, "interpolate.py"), "--config", str(tmp_path / "tiny.ini"),
              "--checkpoint", str(tmp_path / "ckpt_00001"), "--alphas", "0:1.1:0.5", "--seed", "2"]
    subprocess.run(common + ["--som", str(tmp_path / "som"), "--audio", str(audio), "--a-cluster", ka, "--b-cluster", kb,
                             "--out", str(tmp_path / "by_cluster.wav")], check=True, timeout=300, cwd=str(tmp_path))
    subprocess.run(common + ["--a", str(tmp_path / "cat_a.wav"), "--b", str(tmp_path / "cat_b.wav"),
                             "--out", str(tmp_path / "by_hand.wav")], check=True, timeout=300, cwd=str(tmp_path))
    y1, _ = D.read_wav(tmp_path / "by_cluster.wav")
    y2, _ = D.read_wav(tmp_path / "by_hand.wav")
    assert y1.size > 0
    np.testing.assert_array_equal(y1, y2)
