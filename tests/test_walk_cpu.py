"""The latent walk without a device: the numpy oracle's own guarantees on every test corpus (they are what makes the
model safe to run without a guard), the .npz round trip, the host-side argument checks and generate.py's parser.

The closure figure ||A A^T + B B^T - I||_F printed by test_the_oracle_is_stable_and_closed is the yardstick of the GPU
test: tests/test_walk_gpu.py holds the kernels to 8 x the largest value reached here."""
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import walk_oracle as O  # noqa: E402

CLOSURE_CEILING = 2.98e-14      # the largest closure the oracle reached when the GPU bound was set (k = 256)


@pytest.mark.parametrize("lengths,L", O.CORPORA)
def test_the_oracle_is_stable_and_closed(lengths, L):
    x, rs = O.make_corpus(lengths, L), O.row_start(lengths)
    T = x.shape[0]
    assert T == sum(lengths) and x.dtype == np.float32
    full = O.fit(x, rs)
    worst = 0.0
    for k in sorted({full["rank"]} | {k for k in (1, 2, 16, 64) if k <= full["rank"]}):
        for diagonal in (False, True):
            m = O.fit(x, rs, k, diagonal)
            norm, diag, closure = np.linalg.norm(m["Afull"], 2), np.abs(np.diag(m["Afull"])).max(), O.closure(m["A"], m["B"])
            print("oracle", lengths, L, "k", k, "diagonal" if diagonal else "full", "||A||_2 %.6f max|a_jj| %.6f closure %.3g"
                  % (norm, diag, closure))
            assert norm <= 1 + 1e-12 and diag <= 1
            worst = max(worst, closure)
    assert worst <= 2 * CLOSURE_CEILING      # the figure the GPU bound rests on still stands on this machine's LAPACK
    # every row its own file: no pair, C1 exactly zero
    assert not O.lagcov(x, np.arange(T + 1), full["centre"]).any()
    # one file: the unmasked product
    d = x.astype(np.float64) - full["centre"]
    assert np.array_equal(O.lagcov(x, np.array([0, T]), full["centre"]), d[1:].T @ d[:-1] / (T - 1))


def _cpu_walk(lengths=(100, 1, 156), L=17, k=5, diagonal=False):
    from rawaudiovae_kelsey_amd import walk as W
    m = O.fit(O.make_corpus(lengths, L), O.row_start(lengths), k, diagonal)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    walk = W.LatentWalk(k, "diagonal" if diagonal else "full")._set(
        t(m["centre"]), t(m["V"]), t(m["lam"]), t(np.stack([m["A"].T, m["B"].T])), t(m["P"]), t(m["R"]), m["rank"],
        sum(lengths), len(lengths))
    return walk, m


@pytest.mark.parametrize("diagonal", [False, True])
def test_npz_round_trip_and_a_refused_mismatch(tmp_path, diagonal):
    from rawaudiovae_kelsey_amd import walk as W
    walk, m = _cpu_walk(diagonal=diagonal)
    assert np.array_equal(walk.A_.numpy(), m["A"]) and np.array_equal(walk.B_.numpy(), m["B"])
    assert np.array_equal(walk.persistence_, np.diag(m["A"]))
    assert walk.predictability_ == pytest.approx((m["A"] ** 2).sum() / 5, rel=1e-15)
    path = tmp_path / "walk.npz"
    W.write_walk(path, walk, 64, 16)
    back, meta = W.read_walk(path, "cpu")
    assert meta == dict(segment_length=64, latent_dim=17, hop=16, n_frames=257, n_files=3)
    assert back.mode == walk.mode and back.rank_ == walk.rank_ == 17 and back.n_components == 5
    for name in ("mean_", "components_", "explained_variance_", "dyn_", "P_", "R_", "A_", "B_"):
        assert torch.equal(getattr(back, name), getattr(walk, name)), name
    W.write_walk(path, walk, 64)
    assert W.read_walk(path, "cpu")[1]["hop"] is None
    with np.load(path) as z:
        arrays = {n: z[n] for n in z.files}
    bad = dict(arrays, dynamics=arrays["dynamics"][:, :4, :4])
    np.savez(tmp_path / "bad.npz", **bad)
    with pytest.raises(ValueError, match=r"dynamics \(2, 4, 4\).*do not fit latent_dim 17"):
        W.read_walk(tmp_path / "bad.npz", "cpu")
    del arrays["unwhiten"]
    np.savez(tmp_path / "short.npz", **arrays)
    with pytest.raises(ValueError, match="not a latent-walk file, it lacks unwhiten"):
        W.read_walk(tmp_path / "short.npz", "cpu")


def test_argument_checks_without_a_device():
    from rawaudiovae_kelsey_amd import walk as W
    from rawaudiovae_kelsey_amd.corpus import check_hop
    assert W.check_row_start([0, 3, 4, 9], 9).dtype == np.int64
    assert np.array_equal(W.check_row_start(torch.tensor([0, 9]), 9), [0, 9])
    for rs, msg in (([0, 3, 3, 9], "ascending: file 1 is \\[3, 3\\)"), ([1, 9], "from 0 to T=9"), ([0, 8], "from 0 to T=9"),
                    ([0, 5, 4, 9], "ascending: file 1"), ([9], "n_files \\+ 1 entries"), ([0.0, 9.0], "integer sequence")):
        with pytest.raises(ValueError, match=msg):
            W.check_row_start(rs, 9)
    assert W.rank_of([4.0, 1.0, 1e-11, 3e-12, 0.0, -1e-18]) == 3 and W.rank_of([0.0, 0.0]) == 0
    assert W.check_components(None, 7) == 7 and W.check_components(7, 7) == 7
    for k in (0, 8, True, 2.0):
        with pytest.raises(ValueError, match="must be in \\[1, r\\], r = 7 the rank"):
            W.check_components(k, 7)
    with pytest.raises(ValueError, match="mode='ar2'"):
        W.LatentWalk(3, "ar2")
    with pytest.raises(ValueError, match="n_components=0"):
        W.LatentWalk(0)
    with pytest.raises(RuntimeError, match="has not been fitted"):
        W.LatentWalk(3).whiten(torch.zeros(1, 3))
    with pytest.raises(ValueError, match="2-D float32 device tensor"):
        W.lagcov(torch.zeros(4, 3), [0, 4], torch.zeros(3, dtype=torch.float64))
    with pytest.raises(TypeError, match="fitted LatentWalk"):
        W.StreamingWalk(None, object(), 1, 64)
    with pytest.raises(RuntimeError, match="has not been fitted"):
        W.StreamingWalk(None, W.LatentWalk(2), 1, 64)
    assert check_hop(16, 16, 64) == 16 and check_hop(None, 64, 64) == 64 and check_hop(None, None, 64) == 64
    with pytest.raises(ValueError, match="hop 32: the walk was fitted at hop 16"):
        check_hop(16, 32, 64)
    with pytest.raises(ValueError, match="hop 64: the walk was fitted at hop 16"):
        check_hop(16, None, 64)


def test_op_codes_and_field_roles_follow_the_header():
    from rawaudiovae_kelsey_amd import _lib
    text = open(REPO + "/include/rawvae_hip.h").read()
    codes = dict(re.findall(r"#define (RV_(?:PCA_LAGCOV|WALK_\w+)) (\d+)", text))
    assert codes == dict(RV_PCA_LAGCOV="22", RV_WALK_FIT="23", RV_WALK_STEP="24", RV_WALK_WORKSPACE="25",
                         RV_WALK_DYNAMICS="0", RV_WALK_NOISE="1", RV_WALK_DIAGONAL="2")
    assert (_lib.PCA_LAGCOV, _lib.WALK_FIT, _lib.WALK_STEP, _lib.WALK_WORKSPACE) == (22, 23, 24, 25)
    assert (_lib.WALK_DYNAMICS, _lib.WALK_NOISE, _lib.WALK_DIAGONAL) == (0, 1, 2)
    assert _lib.PCA_WORKSPACE == 21                                            # the ops before it keep their numbers
    # the roles' slots and element types: the table of test_audio_tools_cpu.py


def test_generate_py_parser_errors_and_hop_mismatch(tmp_path):
    sys.path.insert(0, REPO)
    import generate as cli
    run = ["run", "--checkpoint", "c", "--walk", "w.npz", "--out", "o.wav"]
    args = cli.parse_args(run + ["--seconds", "1.5", "--hop", "16", "--window", "hann", "--pca-shift", "2:1.5",
                                 "--streams", "3", "--seed", "7", "--temperature", "0"])
    assert (args.seconds, args.hop, args.window, args.pca_shift, args.streams, args.seed, args.temperature) == (
        1.5, 16, "hann", {1: 1.5}, 3, 7, 0.0)
    assert cli.out_paths("a/o.wav", 1) == ["a/o.wav"] and cli.out_paths("a/o.wav", 2) == ["a/o_0.wav", "a/o_1.wav"]
    for extra, msg in ((["--seconds", "0"], "--seconds '0': expected a finite positive"),
                       (["--seconds", "x"], "--seconds 'x'"),
                       (["--seconds", "1", "--temperature", "-1"], "--temperature '-1': expected a finite non-negative"),
                       (["--seconds", "1", "--window", "hamming"], "--window 'hamming'"),
                       (["--seconds", "1", "--streams", "0"], "--streams '0': expected a positive integer"),
                       (["--seconds", "1", "--hop", "-4"], "--hop '-4'"),
                       (["--seconds", "1", "--seed", "-1"], "--seed '-1': expected a non-negative integer"),
                       (["--seconds", "1", "--pca-shift", "0:1"], "--pca-shift '0:1': axis 0: axes are numbered from 1")):
        with pytest.raises(ValueError, match=msg):
            cli.parse_args(run + extra)
    with pytest.raises(ValueError, match="--keep '0': expected a positive integer"):
        cli.parse_args(["fit", "--checkpoint", "c", "--data", "d", "--out", "w.npz", "--keep", "0"])
    with pytest.raises(ValueError, match="expected a command: fit or run"):
        cli.parse_args([])
    with pytest.raises(SystemExit):
        cli.parse_args(["run", "--checkpoint", "c", "--out", "o.wav", "--seconds", "1"])     # no --walk
    # --hop must be the hop of the fit: refused naming both, before anything touches a device
    from rawaudiovae_kelsey_amd import walk as W
    walk, _ = _cpu_walk()
    W.write_walk(tmp_path / "w.npz", walk, 64, 16)
    _, meta = W.read_walk(tmp_path / "w.npz", "cpu")
    args = cli.parse_args(run + ["--seconds", "1", "--hop", "32"])
    from rawaudiovae_kelsey_amd.frontend import check_fitted
    cfg = dict(segment_length=64, latent_dim=meta["latent_dim"])
    with pytest.raises(ValueError, match="--hop: hop 32: the walk was fitted at hop 16"):
        check_fitted("walk", args.walk, meta, cfg, args.hop)
    assert check_fitted("walk", args.walk, meta, cfg, cli.parse_args(run + ["--seconds", "1", "--hop", "16"]).hop) == 16
