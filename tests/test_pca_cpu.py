"""Latent PCA without a GPU: the numpy oracle against numpy.linalg.eigh and numpy's mean, the .npz round trip, the
flag parsers, the header mirrored in _lib, and every argument error of the RV_PCA_* ops (each is raised before
anything is launched and without reading a device pointer, so made-up addresses stand in for device buffers).

Bounds of the Jacobi (u = 2^-52; the same as the GPU test's): max |lambda - eigvalsh| <= 8 L u ||C||_F,
||C V - V Lambda||_F <= 16 L u ||C||_F, ||V^T V - I||_F <= 128 L u."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import REPO
import abi_slots
import pca_oracle as O

U = O.U
FAKE = 4096     # a non-null address that is never dereferenced


def _header():
    with open(os.path.join(REPO, "include", "rawvae_hip.h")) as f:
        return f.read()


@pytest.mark.parametrize("N,L", [(7, 3), (1000, 64), (333, 70)])
def test_oracle_jacobi_equals_eigh_within_the_bounds(N, L):
    C = O.covariance(N, L)
    lam, V, sweeps, converged = O.jacobi(C)
    ref, Vref = O.eigh_descending(C)
    F = np.linalg.norm(C)
    print("sweeps", sweeps, "ratios", np.abs(lam - ref).max() / (L * U * F),
          np.linalg.norm(C @ V.T - V.T * lam) / (L * U * F), np.linalg.norm(V @ V.T - np.eye(L)) / (L * U))
    assert converged and 1 <= sweeps < O.MAX_SWEEPS
    assert np.all(np.diff(lam) <= 0)
    assert np.abs(lam - ref).max() <= 8 * L * U * F
    assert np.linalg.norm(C @ V.T - V.T * lam) <= 16 * L * U * F
    assert np.linalg.norm(V @ V.T - np.eye(L)) <= 128 * L * U
    lead = np.argmax(np.abs(V), axis=1)
    assert np.all(V[np.arange(L), lead] > 0)
    if L >= 64:
        gaps = np.minimum(np.r_[np.inf, ref[:7] - ref[1:8]], ref[:8] - ref[1:9])
        assert gaps.min() >= 0.018 * ref[0]
        assert np.all(np.abs((V[:8] * Vref[:8]).sum(1)) >= 1 - 1e-9)


def test_oracle_jacobi_on_one_by_one_diagonal_and_unconverged_input():
    lam, V, sweeps, converged = O.jacobi(np.array([[2.5]]))
    assert (lam[0], V[0, 0], sweeps, converged) == (2.5, 1.0, 0, True)
    lam, V, sweeps, converged = O.jacobi(np.diag([1.0, 3.0, 2.0]))
    assert list(lam) == [3.0, 2.0, 1.0] and sweeps == 0 and converged
    assert np.array_equal(V, np.eye(3)[[1, 2, 0]])
    _, _, sweeps, converged = O.jacobi(O.covariance(333, 70), max_sweeps=2)
    assert sweeps == 2 and not converged
    assert np.array_equal(O.apply_sign_rule([[1.0, -1.0], [-2.0, 2.0], [0.5, -3.0]]),
                          [[1.0, -1.0], [2.0, -2.0], [-0.5, 3.0]])            # ties: the lowest index decides


def test_round_robin_order_visits_every_pair_once_per_sweep():
    for n in (2, 4, 18, 70):
        seen = set()
        for s in range(n - 1):
            p, q = O.pair_order(n, s)
            assert np.all(p < q) and len(set(p) | set(q)) == n          # disjoint: every index once per step
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == n * (n - 1) // 2


@pytest.mark.parametrize("N,L", [(2, 1), (255, 16), (257, 70), (70001, 70)])
def test_oracle_blocked_mean_is_within_two_ulp_of_numpys(N, L):
    x = O.make_latents(N, L)
    got, ref = O.blocked_mean(x), x.astype(np.float64).mean(0)
    assert np.all(np.abs(got - ref) <= 2 * np.spacing(np.abs(ref)))
    if L >= 3:
        assert got[1] == 0.25 and O.covariance(N, L)[1, 1] == 0 and not O.covariance(N, L)[1].any()


def test_npz_round_trip(tmp_path):
    torch = pytest.importorskip("torch")
    from rawaudiovae_kelsey_amd import pca as P
    C = O.covariance(333, 70)
    lam, V = O.eigh_descending(C)
    mean = O.blocked_mean(O.make_latents(333, 70))
    fitted = P.LatentPCA(5)._set(torch.from_numpy(mean), torch.from_numpy(V), torch.from_numpy(lam), 333, 14, 5)
    path = tmp_path / "p.npz"
    P.write_pca(path, fitted, 1024, 256)
    z = np.load(path)
    assert sorted(z.files) == ["components", "hop", "latent_dim", "mean", "n_frames", "segment_length", "sweeps",
                               "variances"]
    assert all(z[n].dtype == np.float64 for n in ("mean", "components", "variances"))
    back, meta = P.read_pca(path, "cpu")
    assert meta == dict(segment_length=1024, latent_dim=70, hop=256, n_frames=333)
    assert np.array_equal(back.mean_.numpy(), mean) and np.array_equal(back.components_.numpy(), V[:5])
    assert np.array_equal(back.explained_variance_.numpy(), lam[:5]) and np.array_equal(back.all_variances_.numpy(), lam)
    assert back.n_frames_ == 333 and back.sweeps_ == 14 and back.n_components == 5
    clamped = np.maximum(lam, 0)
    assert back.effective_dim_ == pytest.approx(clamped.sum() ** 2 / (clamped ** 2).sum(), rel=1e-12)
    assert np.allclose(back.explained_variance_ratio_.numpy(), clamped[:5] / clamped.sum(), rtol=1e-12, atol=0)
    cum = np.cumsum(clamped) / clamped.sum()
    for frac in (0.9, 0.99, 0.999):
        m = back.components_needed(frac)
        assert cum[m - 1] >= frac and (m == 1 or cum[m - 2] < frac)
    P.write_pca(path, fitted, 1024, None)
    assert P.read_pca(path, "cpu")[1]["hop"] is None
    np.savez(tmp_path / "bad.npz", mean=mean)
    with pytest.raises(ValueError, match="lacks components"):
        P.read_pca(tmp_path / "bad.npz", "cpu")
    np.savez(tmp_path / "bad2.npz", mean=mean[:3], components=V, variances=lam, segment_length=1, latent_dim=70, hop=-1,
             n_frames=2, sweeps=1)
    with pytest.raises(ValueError, match="do not fit latent_dim 70"):
        P.read_pca(tmp_path / "bad2.npz", "cpu")
    with pytest.raises(RuntimeError, match="not been fitted"):
        P.write_pca(path, P.LatentPCA(), 1024)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="n_components"):
            P.LatentPCA(bad)


def test_wrappers_refuse_wrong_shapes_dtypes_and_devices():
    torch = pytest.importorskip("torch")
    from rawaudiovae_kelsey_amd import pca as P
    x = torch.zeros(4, 3)
    for call in (lambda: P.moments(x), lambda: P.moments(np.zeros((4, 3), np.float32)), lambda: P.eig(x.double()),
                 lambda: P.project(x, x.double(), x[0].double()), lambda: P.LatentPCA().fit(x)):
        with pytest.raises(ValueError, match="must be a 2-D float(32|64) device tensor"):
            call()
    with pytest.raises(RuntimeError, match="not been fitted"):
        P.LatentPCA().transform(x)


def test_flag_errors_name_the_flag():
    sys.path.insert(0, REPO)
    import latent_pca as cli
    import resynth
    from rawaudiovae_kelsey_amd import frontend
    assert frontend.parse_axis_values("1:2,3:-0.5", "shift") == {0: 2.0, 2: -0.5}
    for text, what in (("2", "expected J:VALUE"), ("a:1", "expected J:VALUE"), ("1:x", "expected J:VALUE"),
                       ("0:1", "numbered from 1"), ("1:nan", "must be finite"), ("1:inf", "must be finite"),
                       ("2:1,2:3", "given twice"), ("", "expected J:VALUE")):
        with pytest.raises(ValueError, match="--shift .*" + what):
            frontend.parse_axis_values(text, "shift")
    with pytest.raises(ValueError, match="--gain: axis 9: the PCA file holds 8 axes"):
        frontend.check_axes({8: 1.0}, 8, "gain")
    base = ["--checkpoint", "c", "--out", "o"]
    edit = ["edit"] + base + ["--pca", "p.npz", "--in", "i.wav"]
    for argv, what in ((["fit"] + base + ["--data", "d", "--hop", "0"], "--hop '0'"),
                       (["fit"] + base + ["--data", "d", "--hop", "x"], "--hop 'x'"),
                       (edit + ["--window", "hamming"], "--window 'hamming'"),
                       (edit + ["--keep", "-1"], "--keep '-1'"),
                       (edit + ["--gain", "1"], "--gain '1'"),
                       (edit + ["--shift", "0:1"], "--shift '0:1'"),
                       ([], "expected a command")):
        with pytest.raises(ValueError, match=what):
            cli.parse_args(argv)
    args = cli.parse_args(edit + ["--hop", "16", "--window", "hann", "--keep", "3", "--gain", "4:2", "--shift", "1:1.5"])
    assert (args.hop, args.window, args.keep, args.gain, args.shift) == (16, "hann", 3, {3: 2.0}, {0: 1.5})
    g, h = cli.controls(args, 8)
    assert list(g) == [1, 1, 1, 2, 0, 0, 0, 0] and list(h) == [1.5, 0, 0, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="--keep 3: the PCA file holds 2 axes"):
        cli.controls(args, 2)
    assert cli.check_framing(args, 64) == 16
    with pytest.raises(ValueError, match="--window hann"):
        cli.check_framing(cli.parse_args(edit + ["--hop", "64", "--window", "hann"]), 64)
    with pytest.raises(ValueError, match="--hop 48"):
        cli.check_framing(cli.parse_args(edit + ["--hop", "48"]), 64)
    rs = ["--checkpoint", "c", "--in", "i.wav", "--out", "o.wav"]
    with pytest.raises(ValueError, match="--pc-shift: --pca and --pc-shift come together"):
        resynth.parse_args(rs + ["--pca", "p.npz"])
    with pytest.raises(ValueError, match="--pca: --pca and --pc-shift come together"):
        resynth.parse_args(rs + ["--pc-shift", "1:2"])
    with pytest.raises(ValueError, match="--pc-shift '1;2'"):
        resynth.parse_args(rs + ["--pca", "p.npz", "--pc-shift", "1;2"])
    assert resynth.parse_args(rs + ["--pca", "p.npz", "--pc-shift", "2:0.5"]).pc_shift == {1: 0.5}
    assert resynth.parse_args(rs).pca is None


def test_header_ops_and_fields_are_mirrored_and_no_entry_point_is_added():
    from rawaudiovae_kelsey_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert len(set(re.findall(r"\b(rv_[a-z0-9_]+)\s*\(", src))) <= 70
    for name, value in (("MOMENTS", 18), ("EIG", 19), ("APPLY", 20), ("WORKSPACE", 21), ("PROJECT", 0),
                        ("RECONSTRUCT", 1), ("EDIT", 2)):
        assert int(re.search(r"#define RV_PCA_%s (\d+)" % name, src).group(1)) == value == getattr(_lib, "PCA_" + name)
    # no slot is added: the fp64 operands are members of the slots they share (test_audio_tools_cpu.py holds the table)
    assert len(abi_slots.check_layout()) == 37
    head = _header()
    assert head.index("Latent PCA (csrc/pca.hip") > head.index("#define RV_EVAL_DIMS 17")


def _err(op, text, **fields):
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError) as e:
        _lib.lib().rv_mosaic(op, _lib.C.byref(_lib.MosaicDesc(**fields)), None)
    assert text in str(e.value), str(e.value)


def test_workspace_query_and_its_errors():
    from rawaudiovae_kelsey_amd import _lib, pca as P
    assert P.workspace_bytes(0, 1) == 8 and P.workspace_bytes(0, 512) == 8 * 512 * 512
    # moments: the block sums of the mean and one 64 x 64 partial per (range of 4096 rows, tile on or above the diagonal)
    assert P.workspace_bytes(2, 1) == 8 * (1 + 4096)
    assert P.workspace_bytes(4097, 70) == 8 * (17 * 70 + 2 * 3 * 4096)
    assert P.workspace_bytes(3000, 256) == max(8 * (12 * 256 + 10 * 4096), 8 * 256 * 256)
    for T, L, what in ((1, 8, "T=1"), (-1, 8, "T=-1"), (1 << 31, 8, "T=2147483648"), (0, 0, "L=0"), (0, 513, "L=513")):
        _err(_lib.PCA_WORKSPACE, "rv_mosaic(PCA_WORKSPACE): " + what, T=T, L=L)


def test_every_argument_error_names_its_field():
    from rawaudiovae_kelsey_amd import _lib
    ok = dict(T=100, L=16, q=FAKE, trans=FAKE, dist=FAKE, ws=FAKE, ws_bytes=1 << 30)
    for change, what in ((dict(T=1), "T=1 outside [2, 2^31)"), (dict(T=1 << 31), "T=2147483648"), (dict(L=0), "L=0"),
                         (dict(L=513), "L=513 outside [1, 512]"), (dict(q=None), "q is null"),
                         (dict(trans=None), "centre is null"), (dict(dist=None), "basis is null"),
                         (dict(ws=None), "ws is null"), (dict(ws_bytes=8 * (16 + 4096) - 1), "ws_bytes=32895")):
        _err(_lib.PCA_MOMENTS, "rv_mosaic(PCA_MOMENTS): " + what, **dict(ok, **change))
    ok = dict(L=16, dist=FAKE, cost=FAKE, choice=FAKE, ws=FAKE, ws_bytes=8 * 256)
    for change, what in ((dict(L=0), "L=0"), (dict(L=513), "L=513 outside [1, 512]"), (dict(dist=None), "basis is null"),
                         (dict(cost=None), "the eigenvalues are null"), (dict(choice=None), "info is null"),
                         (dict(ws=None), "ws is null"), (dict(ws_bytes=8 * 256 - 1), "ws_bytes=2047")):
        _err(_lib.PCA_EIG, "rv_mosaic(PCA_EIG): " + what, **dict(ok, **change))
    ok = dict(T=5, L=16, k=4, q=FAKE, out=FAKE, trans=FAKE, dist=FAKE, cost=FAKE, weight=FAKE, c=FAKE)
    for mode, width in ((_lib.PCA_PROJECT, 4), (_lib.PCA_RECONSTRUCT, 16), (_lib.PCA_EDIT, 16)):
        base = dict(ok, mode=mode, ldo=width)
        for change, what in ((dict(T=0), "T=0 outside [1, 2^31)"), (dict(L=513, k=513), "L=513 outside [1, 512]"),
                             (dict(k=0), "k=0 outside [1, L=16]"), (dict(k=17), "k=17 outside [1, L=16]"),
                             (dict(q=None), "q is null"), (dict(out=None), "out is null"),
                             (dict(trans=None), "centre is null"), (dict(dist=None), "basis is null"),
                             (dict(ldo=width - 1), "ldo=%d holds no row of %d values" % (width - 1, width))):
            _err(_lib.PCA_APPLY, "rv_mosaic(PCA_APPLY): " + what, **dict(base, **change))
    edit = dict(ok, mode=_lib.PCA_EDIT, ldo=16)
    for change, what in ((dict(cost=None), "the eigenvalues are null"), (dict(weight=None), "the gains are null"),
                         (dict(c=None), "the shifts are null")):
        _err(_lib.PCA_APPLY, "rv_mosaic(PCA_APPLY): " + what, **dict(edit, **change))
    _err(_lib.PCA_APPLY, "rv_mosaic(PCA_APPLY): mode=3", **dict(ok, mode=3, ldo=16))
