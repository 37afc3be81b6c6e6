"""The RV_PCA_* ops, LatentPCA and the two command-line tools on the GPU against tests/pca_oracle.py.

Bounds (u = 2^-52).
  moments   centre: bit-equal to the oracle's blocked sum.  |C - numpy.cov|_ij <= (N + 8) 2^-53 sqrt(C_ii C_jj): the
            fp64 dot-product bound with Cauchy-Schwarz (a reordered fp64 accumulation stays under 0.13 of it on these
            inputs).  C == C^T exactly; two runs bit-equal.
  eig       max |lambda - eigvalsh| <= 8 L u ||C||_F, ||C V - V Lambda||_F <= 16 L u ||C||_F, ||V^T V - I||_F <= 128 L u
            (the numpy restatement of the algorithm reaches 0.54, 1.5 and 22 in the units of the coefficients); each of
            the top 8 eigenvectors of the L >= 64 cases within 1 - 1e-9 of eigh's, their gaps asserted >= 0.018 lambda_max.
  apply     every output within 1 fp32 ulp of the float64 value plus (L + 2) 2^-53 sum |terms|.
Each test prints the figures it asserts on.
"""
import functools
import json
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import pca_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

U = O.U
MOMENT_SHAPES = [(2, 1), (7, 3), (255, 16), (256, 17), (257, 70), (1000, 64), (70001, 70), (3000, 256)]
EIG_CASES = [(7, 3), (1000, 64), (333, 70), (3000, 256)]
APPLY_CASE = {3: (7, 3), 70: (333, 70), 256: (3000, 256)}     # the corpus whose axes an L is applied with


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))     # a copy: the oracle's arrays are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


# ---- moments ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,L", MOMENT_SHAPES)
def test_moments_equal_the_blocked_mean_and_numpy_cov(N, L):
    from rawaudiovae_kelsey_amd import pca as P
    x = O.make_latents(N, L)
    xd = _dev(x)
    centre, C = P.moments(xd)
    centre2, C2 = P.moments(xd)
    assert np.array_equal(_bits(centre), O.blocked_mean(x).view(np.int64))
    ref = O.covariance(N, L)
    sd = np.sqrt(np.diag(ref))
    bound = (N + 8) * 2.0 ** -53 * np.outer(sd, sd)
    got = C.cpu().numpy()
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("moments", (N, L), "worst |C - cov| / bound", np.nanmax(np.where(bound > 0, err / bound, 0.0)))
    assert np.all(err <= bound)
    assert np.array_equal(got, got.T)
    assert np.array_equal(_bits(centre), _bits(centre2)) and np.array_equal(_bits(C), _bits(C2))
    if L >= 3:
        assert not got[1].any()                        # the collapsed dimension: exactly 0 on both sides


def test_moments_of_a_strided_slice_equal_those_of_its_copy():
    from rawaudiovae_kelsey_amd import pca as P
    x = _dev(O.make_latents(257, 70))
    big = torch.full((257, 150), 9.0, device="cuda")
    big[:, 40:110] = x
    view = big[:, 40:110]
    assert not view.is_contiguous()
    for a, b in zip(P.moments(view), P.moments(x)):
        assert np.array_equal(_bits(a), _bits(b))
    assert bool((big[:, :40] == 9.0).all()) and bool((big[:, 110:] == 9.0).all())


# ---- eig ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _eig(N, L):
    from rawaudiovae_kelsey_amd import pca as P
    C = _dev(O.covariance(N, L))
    runs = [P.eig(C) for _ in range(2)]
    assert np.array_equal(C.cpu().numpy(), O.covariance(N, L))                 # the wrapper works on a copy
    for a, b in zip(*runs):
        assert (torch.equal(a, b) if torch.is_tensor(a) else a == b)           # two runs bit-equal
    lam, V, sweeps, converged = runs[0]
    return lam.cpu().numpy(), V.cpu().numpy(), sweeps, converged


@pytest.mark.parametrize("N,L", EIG_CASES)
def test_eig_equals_eigh_within_the_bounds(N, L):
    C = O.covariance(N, L)
    lam, V, sweeps, converged = _eig(N, L)
    ref, Vref = O.eigh_descending(C)
    F = np.linalg.norm(C)
    r = (np.abs(lam - ref).max() / (L * U * F), np.linalg.norm(C @ V.T - V.T * lam) / (L * U * F),
         np.linalg.norm(V @ V.T - np.eye(L)) / (L * U))
    print("eig", (N, L), "sweeps", sweeps, "ratios to L u ||C||, L u ||C||, L u: %.3g %.3g %.3g (bounds 8, 16, 128)" % r)
    assert converged and 1 <= sweeps <= O.MAX_SWEEPS
    assert np.all(np.diff(lam) <= 0)
    assert r[0] <= 8 and r[1] <= 16 and r[2] <= 128
    lead = np.argmax(np.abs(V), axis=1)
    assert np.all(V[np.arange(L), lead] > 0)                                   # the sign rule
    if L >= 64:
        gaps = np.minimum(np.r_[np.inf, ref[:7] - ref[1:8]], ref[:8] - ref[1:9])
        assert gaps.min() >= 0.018 * ref[0]                                    # the condition of the next line
        dots = np.abs((V[:8] * Vref[:8]).sum(1))
        print("eig", (N, L), "1 - |<v, v_eigh>| of the top 8:", 1 - dots)
        assert np.all(dots >= 1 - 1e-9)


def test_eig_of_one_by_one_and_of_a_diagonal_matrix():
    from rawaudiovae_kelsey_amd import pca as P
    lam, V, sweeps, converged = P.eig(_dev(np.array([[2.5]])))
    assert (float(lam[0]), float(V[0, 0]), sweeps, converged) == (2.5, 1.0, 0, True)
    lam, V, sweeps, converged = P.eig(_dev(np.diag([1.0, -3.0, 2.0, 2.0, 0.0])))
    assert lam.tolist() == [2.0, 2.0, 1.0, 0.0, -3.0] and sweeps == 0 and converged   # negative values as computed
    assert np.array_equal(V.cpu().numpy(), np.eye(5)[[2, 3, 0, 4, 1]])                # ties: the lower index first


# ---- apply --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _axes(L):
    """(centre [L], components [L, L], eigenvalues [L]) float64 of the corpus of APPLY_CASE[L], by numpy."""
    N, _ = APPLY_CASE[L]
    lam, V = O.eigh_descending(O.covariance(N, L))
    return O.blocked_mean(O.make_latents(N, L)), V, lam


def _tol(ref, terms, L):
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + (L + 2) * 2.0 ** -53 * terms


@pytest.mark.parametrize("T", [1, 300])
@pytest.mark.parametrize("L", [3, 70, 256])
def test_project_and_reconstruct_within_one_ulp(L, T):
    from rawaudiovae_kelsey_amd import pca as P
    centre, V, _ = _axes(L)
    x = O.make_latents(300, L)[:T]
    for k in (1, 2, L):
        comp = V[:k]
        yref, yterms = O.project(x, comp, centre)
        y = P.project(_dev(x), _dev(comp), _dev(centre))
        assert y.shape == (T, k) and y.dtype == torch.float32
        err = np.abs(y.cpu().numpy().astype(np.float64) - yref)
        assert np.all(err <= _tol(yref, yterms, L)), ("project", L, k, (err / _tol(yref, yterms, L)).max())
        y32 = yref.astype(np.float32)
        xref, xterms = O.reconstruct(y32, comp, centre)
        xh = P.reconstruct(_dev(y32), _dev(comp), _dev(centre))
        assert xh.shape == (T, L)
        err = np.abs(xh.cpu().numpy().astype(np.float64) - xref)
        assert np.all(err <= _tol(xref, xterms, L)), ("reconstruct", L, k, (err / _tol(xref, xterms, L)).max())


@pytest.mark.parametrize("L", [3, 70, 256])
def test_edit_identity_full_removal_and_a_mixed_edit(L):
    from rawaudiovae_kelsey_amd import pca as P
    centre, V, lam = _axes(L)
    x = O.make_latents(300, L)
    xd, cd = _dev(x), _dev(centre)
    for k in (1, 2, L):
        ones, zeros = torch.ones(k, device="cuda"), torch.zeros(k, device="cuda")
        same = P.edit(xd, _dev(V[:k]), cd, _dev(lam[:k]), ones, zeros)
        assert np.array_equal(_bits(same), x.view(np.int32)), k                # g = 1, h = 0: x bit for bit
    Vd, ld = _dev(V), _dev(lam)
    gone = P.edit(xd, Vd, cd, ld, torch.zeros(L, device="cuda"), torch.zeros(L, device="cuda"))
    ref, terms = O.edit(x, V, centre, lam, np.zeros(L), np.zeros(L))
    assert np.all(np.abs(gone.cpu().numpy() - ref) <= _tol(ref, terms, L))
    assert np.all(np.abs(gone.cpu().numpy() - centre) <= _tol(centre, terms, L))   # k = L, g = 0: the centre, rounded
    rng = np.random.default_rng(L)
    k = min(L, 5)
    g, h = rng.uniform(0, 2, k).astype(np.float32), rng.uniform(-2, 2, k).astype(np.float32)
    ref, terms = O.edit(x, V[:k], centre, lam[:k], g, h)
    got = P.edit(xd, _dev(V[:k]), cd, _dev(lam[:k]), _dev(g), _dev(h))
    assert np.all(np.abs(got.cpu().numpy() - ref) <= _tol(ref, terms, L))
    assert not np.array_equal(got.cpu().numpy(), x)


@pytest.mark.parametrize("L", [3, 256])
def test_a_row_alone_equals_the_row_among_others_and_padding_is_untouched(L):
    from rawaudiovae_kelsey_amd import pca as P
    centre, V, lam = _axes(L)
    k = min(L, 7)
    x = _dev(O.make_latents(300, L))
    comp, cd, ld = _dev(V[:k]), _dev(centre), _dev(lam[:k])
    g, h = torch.linspace(0, 2, k, device="cuda"), torch.linspace(-1, 1, k, device="cuda")
    y = P.project(x, comp, cd)
    forms = ((lambda r: P.project(r, comp, cd), x, k), (lambda r: P.reconstruct(r, comp, cd), y, L),
             (lambda r: P.edit(r, comp, cd, ld, g, h), x, L))
    for f, rows, width in forms:
        whole = f(rows)
        for t in (0, 137, 299):
            assert torch.equal(f(rows[t:t + 1]), whole[t:t + 1]), (width, t)
    for f, rows, width in ((P.project, x, k), (P.reconstruct, y, L)):
        out = torch.full((300, width + 3), float("nan"), device="cuda")
        assert f(rows, comp, cd, out=out) is out
        assert torch.equal(out[:, :width], f(rows, comp, cd)) and bool(out[:, width:].isnan().all())
    out = torch.full((300, L + 5), float("nan"), device="cuda")
    P.edit(x, comp, cd, ld, g, h, out=out)
    assert torch.equal(out[:, :L], P.edit(x, comp, cd, ld, g, h)) and bool(out[:, L:].isnan().all())
    assert P.project(x, comp, cd, ldo=k + 2).shape == (300, k + 2)


def test_a_captured_edit_replays_with_updated_gains():
    from rawaudiovae_kelsey_amd import pca as P
    from rawaudiovae_kelsey_amd.engine import Graph
    L = 70
    centre, V, lam = _axes(L)
    x = _dev(O.make_latents(300, L))
    comp, cd, ld = _dev(V), _dev(centre), _dev(lam)
    g, h = torch.ones(L, device="cuda"), torch.zeros(L, device="cuda")
    out = torch.zeros((300, L), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = Graph(side)
    with torch.cuda.stream(side), graph:
        P.edit(x, comp, cd, ld, g, h, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph.launch(torch.cuda.current_stream())
    assert torch.equal(out, x)
    g[3:] = 0
    h[0] = 1.5
    graph.launch(torch.cuda.current_stream())
    assert torch.equal(out, P.edit(x, comp, cd, ld, g, h)) and not torch.equal(out, x)
    torch.cuda.synchronize()


# ---- the class, the corpus helper and the command-line tools ---------------------------------------------------------

S, H, LAT, SR = 64, 32, 8, 8000


def _model(seed=0):
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.synth import make_params
    m = VAE(S, H, LAT).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(S, H, LAT, seed).items()})
    return m


def _waves():
    rng = np.random.default_rng(11)
    t = np.arange(2100) / SR
    return [(0.5 * np.sin(2 * np.pi * 330 * t) + 0.2 * rng.standard_normal(t.size)).astype(np.float32),
            (0.7 * rng.uniform(-1, 1, 1333)).astype(np.float32)]


def test_latent_pca_class_and_fit_corpus():
    from rawaudiovae_kelsey_amd import pca as P
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    model = _model()
    codec = FrameCodec(model)
    mus = []
    for w in _waves():
        w = codec.wave(w)
        padded, n = codec.pad(w, w.numel(), 16)
        mus.append(codec.encode(padded, n, 16)[0])
    mu = torch.cat(mus)
    a, b = P.fit_corpus(model, _waves(), 16), P.LatentPCA().fit(mu)
    for name in ("mean_", "components_", "explained_variance_", "explained_variance_ratio_"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert (a.n_frames_, a.sweeps_, a.effective_dim_) == (b.n_frames_, b.sweeps_, b.effective_dim_)
    assert a.n_frames_ == mu.shape[0] and 1 <= a.sweeps_ <= 40
    lam = b.explained_variance_.cpu().numpy()
    ref = np.linalg.eigvalsh(np.cov(mu.cpu().numpy().astype(np.float64), rowvar=False))[::-1]
    # Weyl: the covariance's own error, at most (N + 8) 2^-53 trace in Frobenius norm, plus the solver's bound
    N = mu.shape[0]
    assert np.abs(lam - ref).max() <= (N + 8) * 2.0 ** -53 * ref.clip(0).sum() + 8 * LAT * U * np.linalg.norm(ref)
    c = np.maximum(lam, 0)
    assert b.effective_dim_ == pytest.approx(c.sum() ** 2 / (c ** 2).sum(), rel=1e-12)
    assert float(b.explained_variance_ratio_.sum()) == pytest.approx(1.0, abs=1e-12)
    y = b.transform(mu)
    assert y.shape == (mu.shape[0], LAT)
    assert float((b.inverse_transform(y) - mu).abs().max()) < 1e-5             # all L axes: the rows come back
    small = P.LatentPCA(3).fit(mu)
    assert small.components_.shape == (3, LAT) and torch.equal(small.components_, b.components_[:3])
    assert small.transform(mu).shape == (mu.shape[0], 3)
    assert torch.equal(b.edit(mu), mu)
    off = b.offset([2] + [0] * (LAT - 1))
    want = (2 * np.sqrt(c[0]) * b.components_[0].cpu().numpy()).astype(np.float32)
    assert off.shape == (LAT,) and off.dtype == torch.float32
    assert np.all(np.abs(off.cpu().numpy() - want) <= np.spacing(np.abs(want)))
    assert torch.equal(off, b.offset({0: 2}))
    with pytest.raises(ValueError, match="n_components=9"):
        P.LatentPCA(9).fit(mu)
    with pytest.raises(ValueError, match="shifts: 3 values for 8 components"):
        b.offset([1, 2, 3])


def _files(tmp_path):
    from rawaudiovae_kelsey_amd import data as D
    (tmp_path / "audio").mkdir()
    for i, w in enumerate(_waves()):
        D.write_wav(tmp_path / "audio" / ("%d.wav" % i), w, SR)
    ini = tmp_path / "m.ini"
    ini.write_text("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n"
                   % (SR, S, H, LAT))
    ck = tmp_path / "ckpt"
    torch.save({"epoch": 0, "state_dict": _model().state_dict(), "optimizer": {}}, ck)
    return ini, ck


def test_latent_pca_py_fit_then_edit(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import latent_pca as cli
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import pca as P
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    from rawaudiovae_kelsey_amd.mosaic import ola
    from rawaudiovae_kelsey_amd.stream import window_values
    ini, ck = _files(tmp_path)
    npz = tmp_path / "pca.npz"
    common = ["--config", str(ini), "--checkpoint", str(ck), "--hop", "16"]
    rep = cli.main(["fit"] + common + ["--data", str(tmp_path / "audio"), "--out", str(npz)])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert json.loads(line) == rep and sorted(rep) == ["components_90", "components_99", "components_99_9",
                                                      "effective_dim", "n_frames", "sweeps"]
    model = _model()
    codec = FrameCodec(model)
    waves = [D.load_audio_mono(tmp_path / "audio" / ("%d.wav" % i), SR) for i in range(2)]
    want = P.fit_corpus(model, waves, 16)
    pca, meta = P.read_pca(npz)
    assert meta == dict(segment_length=S, latent_dim=LAT, hop=16, n_frames=want.n_frames_) and rep["n_frames"] == want.n_frames_
    assert torch.equal(pca.components_, want.components_) and torch.equal(pca.mean_, want.mean_)
    assert 1 <= rep["components_90"] <= rep["components_99"] <= rep["components_99_9"] <= LAT
    # no --gain, --shift or --keep: the temperature-0 reconstruction, bit for bit
    src = tmp_path / "audio" / "0.wav"
    edit = ["edit"] + common + ["--pca", str(npz), "--in", str(src), "--window", "hann"]
    plain = cli.main(edit + ["--out", str(tmp_path / "plain.wav")])
    w = codec.wave(waves[0])
    padded, T = codec.pad(w, w.numel(), 16)
    mu, _ = codec.encode(padded, T, 16)
    ref = ola(codec.decode(mu), 16, w.numel(), torch.from_numpy(window_values(S, "hann")).cuda()).cpu().numpy()
    assert plain.shape == ref.shape == waves[0].shape and np.array_equal(plain.view(np.int32), ref.view(np.int32))
    D.write_wav(tmp_path / "ref.wav", ref, SR)
    assert (tmp_path / "plain.wav").read_bytes() == (tmp_path / "ref.wav").read_bytes()
    kept = cli.main(edit + ["--keep", str(LAT), "--out", str(tmp_path / "kept.wav")])
    assert np.array_equal(kept.view(np.int32), ref.view(np.int32))
    # an edit is what LatentPCA.edit of the same mu decodes to
    moved = cli.main(edit + ["--keep", "3", "--gain", "2:0.5", "--shift", "1:1.5", "--out", str(tmp_path / "moved.wav")])
    g, h = np.ones(LAT, np.float32), np.zeros(LAT, np.float32)
    g[3:], g[1], h[0] = 0, 0.5, 1.5
    ref2 = ola(codec.decode(pca.edit(mu, g, h)), 16, w.numel(), torch.from_numpy(window_values(S, "hann")).cuda())
    assert np.array_equal(moved.view(np.int32), _bits(ref2)) and not np.array_equal(moved, ref)
    with pytest.raises(ValueError, match="--shift: axis 9: the PCA file holds 8 axes"):
        cli.main(edit + ["--shift", "9:1", "--out", str(tmp_path / "x.wav")])
    with pytest.raises(ValueError, match="--pca .*no such file"):
        cli.main(["edit"] + common + ["--pca", str(tmp_path / "none.npz"), "--in", str(src), "--out", str(tmp_path / "x.wav")])


def test_resynth_py_pc_shift(tmp_path):
    sys.path.insert(0, REPO)
    import latent_pca as cli
    import resynth
    from rawaudiovae_kelsey_amd.frontend import read_model_config
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import pca as P
    ini, ck = _files(tmp_path)
    npz = tmp_path / "pca.npz"
    cli.main(["fit", "--config", str(ini), "--checkpoint", str(ck), "--hop", "16", "--data", str(tmp_path / "audio"),
              "--out", str(npz)])
    base = ["--config", str(ini), "--checkpoint", str(ck), "--in", str(tmp_path / "audio" / "0.wav"), "--hop", "16",
            "--window", "hann", "--seed", "5"]
    before = resynth.main(base + ["--out", str(tmp_path / "a.wav")])
    zero = resynth.main(base + ["--out", str(tmp_path / "b.wav"), "--pca", str(npz), "--pc-shift", "1:0"])
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "b.wav").read_bytes() and np.array_equal(before, zero)
    # --pc-shift 1:2 moves StreamingVAE.offset by exactly LatentPCA.offset([2, 0, ...]), onto --offset when there is one
    cfg = read_model_config(str(ini))
    pca, _ = P.read_pca(npz)
    want = pca.offset([2] + [0] * (LAT - 1)).cpu().numpy()
    args = resynth.parse_args(base + ["--out", "x", "--pca", str(npz), "--pc-shift", "1:2"])
    assert np.array_equal(resynth.pc_offset(args, cfg, None), want) and np.abs(want).max() > 0
    off = np.linspace(-1, 1, LAT).astype(np.float32)
    assert np.array_equal(resynth.pc_offset(args, cfg, off), off + want)
    np.save(tmp_path / "off.npy", off)
    audio = D.load_audio_mono(tmp_path / "audio" / "0.wav", SR)
    from rawaudiovae_kelsey_amd.frontend import load_model
    ref = resynth.resynthesize(load_model(str(ck), cfg), audio, 16, S, "hann", 1.0, off + want, 5)
    got = resynth.main(base + ["--out", str(tmp_path / "c.wav"), "--offset", str(tmp_path / "off.npy"), "--pca", str(npz),
                               "--pc-shift", "1:2"])
    assert np.array_equal(got, ref) and not np.array_equal(got, before)
    with pytest.raises(ValueError, match="--pc-shift: axis 9"):
        resynth.main(base + ["--out", str(tmp_path / "d.wav"), "--pca", str(npz), "--pc-shift", "9:1"])
