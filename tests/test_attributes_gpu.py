"""RV_ATTR_DESCRIBE / RV_ATTR_FIT and attributes.py on the GPU against tests/attr_oracle.py; every output between guard bands.

Tolerances.  DESCRIBE's columns 0..2 (an fp64 sum and one library logarithm): 1e-12 * max(1, |value|) against the float64
oracle, RV_EVAL_DIMS' bound.  Columns 3 and 4: the oracle's float32 restatement of the kernel's algorithm is run on the same
inputs; its worst disagreement with the float64 oracle, per column and per S over both layouts, is the yardstick, and the
kernel may disagree with float64 by 4 times that (tests/test_evaluate_gpu.py's rule; the values measured on the CPU are in
tests/test_attributes_cpu.py's docstring, the test recomputes and prints them).  Column 3's error is in cycles/sample,
column 4's in dB.
FIT: the oracle's cond(Cyy + lam I) <= 100 is asserted; then B, Cdd and the means are held to 1e-9 * max abs of the block
(n 2^-53 cond with n <= 4133 is about 5e-11, and a margin of 20 for the other summation order), r2 to 1e-9.
"""
import functools
import json
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import attr_oracle as O  # noqa: E402
import eval_oracle as E  # noqa: E402
from guarded import INT_FILL, guarded, guarded_flat  # noqa: E402

pytestmark = pytest.mark.gpu

sys.path.insert(0, REPO)

SIZES = (32, 1024, 4096)
T_ALL = 37
R_DB = 60.0
LAYOUTS = ("side by side", "overlap")
N_KINDS = len(O.KINDS)


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()       # (a copy: the cached inputs are read-only)


@functools.lru_cache(maxsize=None)
def _case(S, layout):
    """The inputs of one DESCRIBE case and both oracle runs, computed once"""
    hop = S if layout == "side by side" else S // 4
    wave, hop = O.signals(S, T_ALL, 1000 + S, hop)
    w = E.hann(S)
    f64 = O.describe(wave, hop, T_ALL, S, w, R_DB)
    f32 = O.describe(wave, hop, T_ALL, S, w, R_DB, dtype=np.float32)
    for a in (wave, f64, f32):
        a.setflags(write=False)
    return dict(x=wave, hop=hop, w=w, f64=f64, f32=f32, ldo=5 if layout == "side by side" else 8)


@functools.lru_cache(maxsize=None)
def _yardstick(S):
    worst = np.zeros(2)
    for layout in LAYOUTS:
        c = _case(S, layout)
        worst = np.maximum(worst, np.nanmax(O.spectral_errors(c["f32"], c["f64"]), axis=0))
    assert np.all(worst > 0) and worst[0] < 1e-6 and worst[1] < 1e-3, worst
    return worst


def _run(c, S, T=T_ALL, row0=0, ldo=None, x=None, window=True):
    """RV_ATTR_DESCRIBE on rows [row0, row0 + T) of case c into a guarded [T, ldo] output -> numpy [T, 5 or 3]"""
    from rawaudiovae_kelsey_amd import attributes as A
    from rawaudiovae_kelsey_amd.evaluate import twiddle_table
    ldo = c["ldo"] if ldo is None else ldo
    cols = 5 if window else 3
    xd = _dev(c["x"] if x is None else x)
    win, tab = (_dev(c["w"]), _dev(twiddle_table(S))) if window else (None, None)
    out = guarded(T, cols, ldo, torch.float64)
    view = out.view if T > 1 else out.flat[out.front:out.front + ldo].view(1, ldo)
    A.describe(xd[row0 * c["hop"]:], T, S, c["hop"], win, R_DB, out=view, table=tab)
    torch.cuda.synchronize()
    out.assert_untouched("desc")
    return out.payload().cpu().numpy()


def _check(got, f64, S, yard=None):
    for col in (0, 1, 2):
        fin = np.isfinite(f64[:, col])
        err = np.abs(got[fin, col] - f64[fin, col])
        tol = 1e-12 * np.maximum(1.0, np.abs(f64[fin, col]))
        print("S %d column %d: worst error / allowed %.3g" % (S, col, np.max(err / tol) if fin.any() else 0))
        assert np.all(err <= tol), (col, err.max())
        assert np.array_equal(got[~fin, col], f64[~fin, col], equal_nan=True), col     # -inf and NaN exactly
    if got.shape[1] == 3:
        return
    err = O.spectral_errors(got, f64)
    assert np.array_equal(np.isnan(got[:, 3:]), np.isnan(f64[:, 3:]))
    print("S %d: kernel's worst errors %s, yardstick %s" % (S, np.nanmax(err, axis=0), yard))
    for j in range(2):
        scaled = ~np.isnan(err[:, j])
        assert np.all(err[scaled, j] <= 4 * yard[j]), (3 + j, np.nanmax(err[:, j]), yard[j])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("S", SIZES)
def test_describe_against_the_oracle(S, layout):
    c = _case(S, layout)
    got = _run(c, S)
    _check(got, c["f64"], S, _yardstick(S))
    again = _run(c, S)
    assert np.array_equal(_bits(got), _bits(again))                                        # run to run
    # a row described alone, two rows, another ldo: the same bits as inside the batch
    for row0, T in ((0, 1), (T_ALL - 1, 1), (8, 1), (30, 2)):
        part = _run(c, S, T=T, row0=row0, ldo=13 - c["ldo"])
        assert np.array_equal(_bits(part), _bits(got[row0:row0 + T])), (row0, T)
    if layout == "side by side":
        silent = [t for t in range(T_ALL) if t % N_KINDS == 6]
        assert np.all(np.isneginf(got[silent, 0])) and np.all(got[silent, 1] == 0) and np.all(np.isnan(got[silent, 2:]))
        dc = [t for t in range(T_ALL) if t % N_KINDS == 3]
        assert np.all(got[dc, 1] == 0) and np.all(got[dc, 2] == 0)
        imp = [t for t in range(T_ALL) if t % N_KINDS == 4]
        assert np.all(np.abs(got[imp, 2] - 10 * np.log10(S)) <= 1e-12 * 10 * np.log10(S))
        assert np.all(np.isfinite(np.delete(got, silent, axis=0)))


@pytest.mark.parametrize("hop", [1000, 250])
def test_describe_without_a_window_takes_any_length(hop):
    S = 1000
    wave, hop = O.signals(S, T_ALL, 77, hop)
    c = dict(x=wave, hop=hop, w=None, ldo=5)
    got = _run(c, S, window=False)              # three columns of a guarded ldo = 5 buffer: columns 3.. are gap columns
    assert got.shape == (T_ALL, 3)
    _check(got, O.describe(wave, hop, T_ALL, S), S)
    assert np.array_equal(_bits(_run(c, S, T=1, row0=20, ldo=3, window=False)), _bits(got[20:21]))
    one = dict(x=np.array([-0.25], dtype=np.float32), hop=1, w=None, ldo=3)
    assert _run(one, 1, T=1, window=False).tolist() == [[10 * np.log10(0.0625), 0.0, 0.0]]        # S = 1: no pair


@pytest.mark.parametrize("S", [32, 1024])
def test_a_nan_sample_changes_only_its_own_row(S):
    c = _case(S, "side by side")
    clean = _run(c, S)
    x = c["x"].copy()
    x[2 * S + 5] = np.nan          # an off-bin sine
    x[8 * S + S - 1] = np.inf      # an on-bin sine
    got = _run(c, S, x=x)
    assert np.all(np.isnan(got[2][[0, 2, 3, 4]])) and np.isfinite(got[2, 1])
    assert got[8, 0] == np.inf and np.all(np.isnan(got[8, 2:])) and np.isfinite(got[8, 1])
    keep = [t for t in range(T_ALL) if t not in (2, 8)]
    assert np.array_equal(_bits(got[keep]), _bits(clean[keep]))
    want = O.describe(x, S, T_ALL, S, c["w"], R_DB)
    assert np.array_equal(np.isnan(want), np.isnan(got)) and np.array_equal(got[:, 1], want[:, 1])


# ---- the fit ---------------------------------------------------------------------------------------------------------

def _fit(x, ldx, c, P, D, lam=0.0):
    """RV_ATTR_FIT with x [T, L] at row pitch ldx, result and info between guard bands and ws inside a painted block ->
    (dict of numpy parts, info [2]); the call is repeated and must give the same bits."""
    from rawaudiovae_kelsey_amd import _lib
    T, L = x.shape
    k, N = P.shape[0], D.shape[1]
    parts, n_res = O.layout(k, N)
    need = _lib.mosaic_call(_lib.ATTR_WORKSPACE, T=T, k=k, N=N).ws_bytes
    xg = guarded(T, L, ldx, torch.float32, fill=x)
    Dg = guarded(T, N, N, torch.float64, fill=D)
    cd, Pd = _dev(np.asarray(c, dtype=np.float64)), _dev(np.asarray(P, dtype=np.float64))
    outs = []
    for _ in range(2):
        res = guarded_flat(n_res, torch.float64)
        info = guarded_flat(2, torch.int32, INT_FILL)
        block = torch.full((need + 1024,), 0x5A, dtype=torch.uint8, device="cuda")
        at = (-block.data_ptr()) % 256 + 256
        _lib.mosaic_call(_lib.ATTR_FIT, T=T, L=L, k=k, N=N, q=xg.ptr, stride=ldx, centre=cd.data_ptr(), basis=Pd.data_ptr(),
                         moment=Dg.ptr, lam=float(lam), result=res.ptr, info=info.ptr, ws=block.data_ptr() + at, ws_bytes=need)
        torch.cuda.synchronize()
        res.assert_untouched("result")
        info.assert_untouched("info")
        assert bool((block[:at] == 0x5A).all()) and bool((block[at + need:] == 0x5A).all()), "ws was overrun"
        outs.append((res.payload().view(-1).cpu().numpy(), info.payload().view(-1).cpu().numpy()))
    assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(outs[0][1], outs[1][1])      # run to run
    flat, info = outs[0]
    got = {name: flat[s] for name, s in parts.items()}
    got["Cdd"], got["B"] = got["Cdd"].reshape(N, N), got["B"].reshape(N, k)
    return got, info


def _axes_of(x, k):
    """(c [L], P [k, L]) numpy float64 of x's own LatentPCA on the GPU"""
    from rawaudiovae_kelsey_amd import attributes as A
    from rawaudiovae_kelsey_amd.pca import LatentPCA
    c, P, _ = A.axes(LatentPCA().fit(_dev(x)), k)
    return c.cpu().numpy(), P.cpu().numpy()


def _targets(x, c, P, N, seed):
    """D [T, N]: column a < N - 1 a random direction of y plus noise of a growing share plus an offset; the last column is
    independent of x"""
    rng = np.random.default_rng(seed)
    Y = (x.astype(np.float64) - c) @ P.T
    k = P.shape[0]
    D = np.empty((x.shape[0], N))
    for a in range(N):
        D[:, a] = (Y @ rng.standard_normal(k)) / np.sqrt(k) + (0.2 + a) * 0.1 * rng.standard_normal(x.shape[0]) + 3.0 * (a + 1)
    D[:, N - 1] = rng.standard_normal(x.shape[0]) - 2.0
    return D


def _compare(got, info, want, lam_cond=100.0):
    assert want["status"] == 0 and want["cond"] <= lam_cond, want["cond"]
    assert info.tolist() == [0, want["n"]] and got["n"][0] == want["n"]
    means, wmeans = np.concatenate([got["ybar"], got["dbar"]]), np.concatenate([want["ybar"], want["dbar"]])
    for name, a, b in (("means", means, wmeans), ("Cdd", got["Cdd"], want["Cdd"]), ("B", got["B"], want["B"])):
        err, scale = np.abs(a - b).max(), np.abs(b).max()
        print("%s: worst error %.3g of max abs %.3g (allowed 1e-9)" % (name, err, scale))
        assert err <= 1e-9 * scale, (name, err, scale)
    err = np.abs(got["r2"] - want["r2"]).max()
    print("r2: worst error %.3g (allowed 1e-9)" % err)
    assert err <= 1e-9


@pytest.mark.parametrize("T,L,k,N,pitch", [(4133, 70, 64, 16, 0), (33, 5, 1, 1, 0), (300, 512, 17, 5, 3)])
def test_fit_against_the_oracle(T, L, k, N, pitch):
    x = O.latents(T, L, T + L)
    c, P = _axes_of(x, k)
    D = _targets(x, c, P, N, 5 * T)
    if pitch:
        rng = np.random.default_rng(9)
        x, D = x.copy(), D.copy()
        x[:32, 7] = np.nan                                   # the whole first 32-row chunk
        x[rng.choice(np.arange(32, T), 3, replace=False), rng.integers(0, L, 3)] = np.inf
        D[rng.choice(np.arange(32, T), 4, replace=False), rng.integers(0, N, 4)] = np.nan
        D[T - 1, 0] = -np.inf                                # a silent frame's level
        assert 0.08 * T <= (~O.observed(x, D)).sum() <= 0.14 * T
    want = O.fit(x, c, P, D)
    got, info = _fit(x, L + pitch, c, P, D)
    _compare(got, info, want)
    # the independent column: at most three times its null mean k / (n - 1), on the oracle and on the device
    bound = 3.0 * k / (want["n"] - 1)
    print("independent target: r2 %.4g (oracle %.4g), bound %.4g" % (got["r2"][N - 1], want["r2"][N - 1], bound))
    assert want["r2"][N - 1] <= bound and got["r2"][N - 1] <= bound
    if N > 1:
        assert want["r2"][0] > 0.9 and got["r2"][0] > 0.9


def test_fit_recovers_a_planted_model_and_takes_a_ridge():
    T, L, k, N = 700, 24, 9, 4
    x = O.latents(T, L, 3)
    c, P = _axes_of(x, k)
    rng = np.random.default_rng(8)
    b = rng.standard_normal((N, k))
    Y = (x.astype(np.float64) - c) @ P.T
    D = Y @ b.T + rng.standard_normal(N)
    D[:, N - 1] = 4.5                                        # a constant target: Cdd[a, a] == 0
    got, info = _fit(x, L, c, P, D)
    assert info.tolist() == [0, T]
    assert np.all(got["r2"][:N - 1] >= 1 - 1e-10) and np.abs(got["B"][:N - 1] - b[:N - 1]).max() <= 1e-9 * np.abs(b).max()
    assert not got["B"][N - 1].any() and got["r2"][N - 1] == 0 and got["Cdd"][N - 1, N - 1] == 0
    D = _targets(x, c, P, N, 2)
    for lam in (0.5, 1e-3):
        want = O.fit(x, c, P, D, lam)
        got, info = _fit(x, L, c, P, D, lam)
        _compare(got, info, want)
    assert np.abs(O.fit(x, c, P, D, 0.5)["B"] - O.fit(x, c, P, D)["B"]).max() > 1e-2     # the ridge is felt


def test_fit_says_when_it_cannot_solve():
    T, L, k, N = 20, 8, 6, 2
    x = O.latents(200, L, 6)
    c, P = _axes_of(x, k)
    D = _targets(x, c, P, N, 1)
    xs, Ds = x[:T].copy(), D[:T].copy()
    xs[:9, 0] = np.nan
    Ds[15:19, 1] = np.inf                                    # 7 observed frames are fewer than k + 2 = 8
    got, info = _fit(xs, L, c, P, Ds)
    assert info.tolist() == [1, 7] and got["n"][0] == 7 and not got["B"].any() and not got["r2"].any()
    assert O.fit(xs, c, P, Ds)["status"] == 1
    xs[8, 0] = x[8, 0]                                       # the eighth frame: solvable again
    got, info = _fit(xs, L, c, P, Ds)
    assert info.tolist() == [0, 8] and O.fit(xs, c, P, Ds)["status"] == 0 and got["B"].any()
    # a duplicated axis: rank-deficient P
    P2 = np.concatenate([P[:3], P[1:2], P[3:]])
    want = O.fit(x, c, P2, D)
    got, info = _fit(x, L, c, P2, D)
    assert want["status"] == 2 and info.tolist() == [2, 200] and not got["B"].any() and not got["r2"].any()
    assert np.abs(got["Cdd"] - want["Cdd"]).max() <= 1e-9 * np.abs(want["Cdd"]).max()
    want = O.fit(x, c, P2, D, 1e-3)
    got, info = _fit(x, L, c, P2, D, 1e-3)
    assert want["status"] == 0 and info.tolist() == [0, 200]
    tol = 20 * 200 * 2.0 ** -53 * want["cond"]               # the module doc's bound at this condition number
    print("ridge 1e-3 on a duplicated axis: cond %.3g, B error %.3g (allowed %.3g of max abs)" % (
        want["cond"], np.abs(got["B"] - want["B"]).max(), tol))
    assert np.abs(got["B"] - want["B"]).max() <= tol * np.abs(want["B"]).max()
    assert np.abs(got["r2"] - want["r2"]).max() <= tol


# ---- the whole path --------------------------------------------------------------------------------------------------

def test_one_graph_replay_of_describe_then_fit_gives_the_eager_bits():
    from rawaudiovae_kelsey_amd import attributes as A
    from rawaudiovae_kelsey_amd.evaluate import twiddle_table
    from rawaudiovae_kelsey_amd.pca import LatentPCA
    from rawaudiovae_kelsey_amd.stream import GraphReplay
    S, hop, T, L, k = 64, 16, 300, 12, 5
    wave, _ = O.signals(S, T, 21, hop)
    x = _dev(O.latents(T, L, 4))
    ax = A.axes(LatentPCA().fit(x), k)

    class Captured(GraphReplay):
        n_streams, block, device = 1, 1, torch.device("cuda")

        def __init__(self):
            self.wave = torch.zeros(wave.size, dtype=torch.float32, device="cuda")
            self.win, self.tab = _dev(E.hann(S)), _dev(twiddle_table(S))
            self.desc = torch.full((T, 5), 7.0, dtype=torch.float64, device="cuda")
            self.out = (torch.full((A.result_layout(k, 5)[1],), 7.0, dtype=torch.float64, device="cuda"),
                        torch.full((2,), INT_FILL, dtype=torch.int32, device="cuda"))
            self.ws = A.workspace(T, k, 5, "cuda")

        def parameters(self):
            return []

        def launch(self, st):
            A.describe(self.wave, T, S, hop, self.win, R_DB, out=self.desc, table=self.tab, stream=st)
            A.fit_targets(x, self.desc, ax, out=self.out, ws=self.ws, stream=st)

    cap = Captured()
    cap.wave.copy_(_dev(wave))
    cap.launch(None)
    torch.cuda.synchronize()
    eager = [t.clone() for t in (cap.desc, *cap.out)]
    assert eager[2].tolist()[0] == 0 and 0 < eager[2].tolist()[1] < T          # the silent frames are unobserved
    cap._capture(cap.launch)
    for t in (cap.desc, *cap.out):
        t.fill_(3)
    cap.ws[0].fill_(0x33)
    cap._replay(0, "replay()")
    torch.cuda.synchronize()
    for a, b in zip(eager, (cap.desc, *cap.out)):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))
    want = O.describe(wave, hop, T, S, E.hann(S), R_DB)
    res = O.fit(x.cpu().numpy(), ax[0].cpu().numpy(), ax[1].cpu().numpy(), want)
    assert eager[2].tolist() == [0, res["n"]]


SR, S_M, H_M, LAT = 8000, 64, 96, 8


def _model(seed=0):
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.synth import make_params
    m = VAE(S_M, H_M, LAT).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(S_M, H_M, LAT, seed).items()})
    return m


def _files(tmp_path):
    from rawaudiovae_kelsey_amd import data as D
    rng = np.random.default_rng(12)
    n = np.arange(2100)
    waves = [(0.5 * np.sin(2 * np.pi * (0.01 + 0.00002 * n) * n) * (0.3 + 0.7 * np.abs(np.sin(0.004 * n)))).astype(np.float32),
             (0.4 * rng.uniform(-1, 1, 1700) * np.linspace(0.05, 1, 1700)).astype(np.float32)]
    (tmp_path / "audio").mkdir()
    for i, w in enumerate(waves):
        D.write_wav(tmp_path / "audio" / ("%d.wav" % i), w, SR)
    ini = tmp_path / "m.ini"
    ini.write_text("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n" % (SR, S_M, H_M, LAT))
    ck = tmp_path / "ckpt"
    torch.save({"epoch": 0, "state_dict": _model().state_dict(), "optimizer": {}}, ck)
    return ini, ck, waves


def test_attributes_py_measure_fit_move_and_edit(tmp_path, capsys):
    import attributes as cli
    import latent_pca
    from rawaudiovae_kelsey_amd import attributes as A
    from rawaudiovae_kelsey_amd import data as D
    ini, ck, waves = _files(tmp_path)
    src = tmp_path / "audio" / "0.wav"
    # measure: the descriptors of the wav's frames, as describe gives them
    rep = cli.main(["measure", "--in", str(src), "--segment-length", "64", "--hop", "16", "--out", str(tmp_path / "d.npy")])
    desc = np.load(tmp_path / "d.npy")
    w0 = D.load_audio_mono(src, SR)
    T0 = rep["frames"]
    padded = np.zeros((T0 - 1) * 16 + 64, dtype=np.float32)
    padded[:w0.size] = w0
    assert desc.shape == (T0, 5) and rep["sampling_rate"] == SR and rep["silent_frames"] == 0
    assert np.array_equal(_bits(desc), _bits(A.describe(_dev(padded), T0, 64, 16).cpu().numpy()))
    f64 = O.describe(padded, 16, T0, 64, E.hann(64))
    _check(desc, f64, 64, np.nanmax(O.spectral_errors(O.describe(padded, 16, T0, 64, E.hann(64), dtype=np.float32), f64), axis=0))
    capsys.readouterr()
    # fit
    common = ["--config", str(ini), "--checkpoint", str(ck), "--hop", "16"]
    npz = tmp_path / "attrs.npz"
    rep = cli.main(["fit"] + common + ["--data", str(tmp_path / "audio"), "--keep", "4", "--out", str(npz)])
    out = capsys.readouterr().out
    assert json.loads(out.strip().splitlines()[-1]) == rep and rep["names"] == list(A.NAMES) and rep["keep"] == 4
    assert "R2" in out and "cross-talk" in out
    at, meta = A.read_attributes(npz)
    want, x, targets = A.fit_corpus(_model(), [D.load_audio_mono(tmp_path / "audio" / ("%d.wav" % i), SR) for i in range(2)], 16,
                                    n_components=4)
    assert meta == dict(segment_length=64, latent_dim=LAT, hop=16, n_frames=x.shape[0], n_observed=want.n_observed_)
    assert np.array_equal(at.B_, want.B_) and np.array_equal(at.R_, want.R_) and np.array_equal(at.r2_, want.r2_)
    assert np.all(at.r2_ <= 1 + 1e-12) and np.all(np.abs(np.diag(at.corr_) - 1) <= 1e-12)
    # move: the offset file is LatentAttributes.move's, the printed prediction is B w
    moves = {"level": -3.0, "centroid": 0.02}
    rep = cli.main(["move", "--attrs", str(npz), "--move", "centroid:+0.02,level:-3", "--out", str(tmp_path / "off.npy")])
    off, pred, norm = at.move(moves)
    _, want_pred, want_norm = O.move(at.B_, at.R_, [0, 3], [-3.0, 0.02])
    assert np.array_equal(np.load(tmp_path / "off.npy"), off.cpu().numpy()) and np.load(tmp_path / "off.npy").dtype == np.float32
    assert rep["predicted"] == [float(v) for v in pred] and np.abs(pred - want_pred).max() <= 1e-9 and rep["norm"] == norm
    assert abs(norm - want_norm) <= 1e-9 * want_norm
    # edit with no move: latent_pca.py edit without edits, bit for bit
    latent_pca.main(["fit"] + common + ["--data", str(tmp_path / "audio"), "--out", str(tmp_path / "pca.npz")])
    ref = latent_pca.main(["edit"] + common + ["--pca", str(tmp_path / "pca.npz"), "--in", str(src), "--window", "hann",
                                               "--out", str(tmp_path / "ref.wav")])
    plain = cli.main(["edit"] + common + ["--attrs", str(npz), "--in", str(src), "--window", "hann", "--out", str(tmp_path / "p.wav")])
    assert np.array_equal(plain.view(np.int32), ref.view(np.int32))
    assert (tmp_path / "p.wav").read_bytes() == (tmp_path / "ref.wav").read_bytes()
    capsys.readouterr()
    moved = cli.main(["edit"] + common + ["--attrs", str(npz), "--in", str(src), "--window", "hann", "--move", "level:-3",
                                          "--out", str(tmp_path / "m.wav")])
    out = capsys.readouterr().out
    print(out)                                               # requested, predicted, achieved: printed, not gated
    last = json.loads(out.strip().splitlines()[-1])
    assert moved.shape == plain.shape and not np.array_equal(moved, plain)
    assert last["requested"][0] == -3.0 and abs(last["predicted"][0] + 3.0) <= 1e-9 and "achieved" in out
    assert last["achieved"][0] is not None and last["frames_compared"] > 0
    with pytest.raises(ValueError, match="--hop: hop 32: the attributes were fitted at hop 16"):
        cli.main(["edit", "--config", str(ini), "--checkpoint", str(ck), "--hop", "32", "--attrs", str(npz), "--in", str(src),
                  "--out", str(tmp_path / "x.wav")])
    # the user's own targets
    np.save(tmp_path / "t.npy", targets.cpu().numpy()[:, :2])
    rep = cli.main(["fit"] + common + ["--data", str(tmp_path / "audio"), "--keep", "4", "--targets", str(tmp_path / "t.npy"),
                                       "--names", "loud,cross", "--out", str(tmp_path / "own.npz")])
    own, _ = A.read_attributes(tmp_path / "own.npz")
    assert own.names == ("loud", "cross") and rep["names"] == ["loud", "cross"]
    assert np.abs(own.B_ - at.B_[:2]).max() <= 1e-9 * np.abs(at.B_[:2]).max()
