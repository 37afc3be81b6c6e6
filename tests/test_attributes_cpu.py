"""Latent attributes without a GPU: the oracle (tests/attr_oracle.py) on signals whose descriptors are known, the op codes
and the descriptor's layout, every argument check of the three ops (they run before anything is launched), the algebra of
LatentAttributes.move on a planted B, the .npz round trip, the hop check and the flags of attributes.py.

The float32 restatement's worst disagreement with float64 on the inputs of tests/test_attributes_gpu.py (Hann window,
R = 60 dB, 37 frames cycling through the seven kinds, hop = S and hop = S / 4), measured on the CPU; the GPU test
recomputes them and allows the kernel 4 times as much:

    S       centroid (cycles/sample)    flatness (dB)
    32      1.3e-08                     2.6e-05
    1024    2.1e-09                     1.5e-06
    4096    3.9e-09                     5.2e-07
"""
import ctypes as C
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import attr_oracle as O  # noqa: E402
import eval_oracle as E  # noqa: E402

sys.path.insert(0, REPO)


def test_the_oracle_on_signals_whose_descriptors_are_known():
    S = 1024
    w = E.hann(S)
    for b in (3, 40, 200):
        d = O.describe(O.bin_of_sine(S, b), S, 1, S, w)[0]
        assert abs(d[3] - b / S) <= 1e-6, (b, d[3])
        # the floor fl = max Pa 10^(-R/10) bounds the flatness of a pure tone from below: three bins of a Hann window
        # hold the power and the other S/2 - 3 sit at the floor, so it is about -R + 10 log10(S / 3) dB: -34.7 dB at
        # S = 1024 under the default R = 60, and below -40 dB with a floor of 80 dB or a frame of 64 samples
        assert abs(d[4] - (-60 + 10 * np.log10(S / 3))) < 0.5, (b, d[4])
        assert O.describe(O.bin_of_sine(S, b), S, 1, S, w, R=80.0)[0, 4] < -40
    for b in (2, 9, 20):
        d = O.describe(O.bin_of_sine(64, b), 64, 1, 64, E.hann(64))[0]
        assert abs(d[3] - b / 64) <= 1e-6 and d[4] < -40, (b, d)
    noise = np.random.default_rng(0).uniform(-1, 1, S).astype(np.float32)
    assert O.describe(noise, S, 1, S, w)[0, 4] > -6 and O.describe(noise[:64], 64, 1, 64, E.hann(64))[0, 4] > -6
    alt = np.where(np.arange(S) % 2 == 0, 1.0, -1.0).astype(np.float32)
    assert O.describe(alt, S, 1, S)[0, 1] == 1.0
    const = np.full(S, 0.5, dtype=np.float32)
    d = O.describe(const, S, 1, S, w)[0]
    assert d[1] == 0.0 and d[2] == 0.0 and d[0] == 10 * np.log10(0.25)
    imp = np.zeros(S, dtype=np.float32)
    imp[17] = 1.0
    d = O.describe(imp, S, 1, S)[0]
    assert abs(d[2] - 10 * np.log10(S)) <= 1e-12 and abs(d[0] + 10 * np.log10(S)) <= 1e-12
    d = O.describe(np.zeros(S, dtype=np.float32), S, 1, S, w)[0]
    assert np.isneginf(d[0]) and d[1] == 0.0 and np.isnan(d[2]) and np.isnan(d[3]) and np.isnan(d[4])
    # a NaN compares as not negative; S = 1 has no pair
    x = np.array([1, np.nan, -1, -1, np.nan, 2], dtype=np.float32)
    assert O.describe(x, 6, 1, 6)[0, 1] == 2 / 5 and O.describe(x[:1], 1, 1, 1)[0, 1] == 0.0
    # both precisions agree on the three columns that are float64 in both, and nearly on the spectral ones
    wave, hop = O.signals(64, 15, 3)
    f64, f32 = O.describe(wave, hop, 15, 64, E.hann(64)), O.describe(wave, hop, 15, 64, E.hann(64), dtype=np.float32)
    assert np.array_equal(f64[:, :3], f32[:, :3], equal_nan=True) and np.array_equal(np.isnan(f64), np.isnan(f32))
    err = O.spectral_errors(f32, f64)
    assert np.nanmax(err[:, 0]) < 1e-6 and np.nanmax(err[:, 1]) < 1e-3 and np.nanmax(err) > 0


@pytest.mark.parametrize("S", [32, 1024, 4096])
def test_the_yardsticks_of_the_gpu_test(S):
    worst = np.zeros(2)
    for hop in (S, S // 4):
        wave, hop = O.signals(S, 37, 1000 + S, hop)
        f64 = O.describe(wave, hop, 37, S, E.hann(S))
        f32 = O.describe(wave, hop, 37, S, E.hann(S), dtype=np.float32)
        worst = np.maximum(worst, np.nanmax(O.spectral_errors(f32, f64), axis=0))
    print("S %d: centroid %.3g cycles/sample, flatness %.3g dB" % (S, worst[0], worst[1]))
    assert 0 < worst[0] < 1e-6 and 0 < worst[1] < 1e-3


def test_the_fit_oracle_recovers_a_planted_model():
    T, L, k, N = 500, 12, 5, 3
    x = O.latents(T, L, 2)
    c, P, lam, V = O.whitening(x, k)
    rng = np.random.default_rng(4)
    b = rng.standard_normal((N, k))
    Y = (x.astype(np.float64) - c) @ P.T
    D = Y @ b.T + rng.standard_normal(N)
    res = O.fit(x, c, P, D)
    assert res["status"] == 0 and res["n"] == T and res["cond"] <= 1 + 1e-9
    assert np.abs(res["B"] - b).max() <= 1e-10 and (res["r2"] >= 1 - 1e-10).all()
    assert np.abs(res["Cyy"] - np.eye(k)).max() <= 1e-10          # whitened by its own PCA
    D[::7, 1] = np.nan
    x2 = x.copy()
    x2[3, 2] = np.inf
    res = O.fit(x2, c, P, D)
    assert res["n"] == T - len(range(0, T, 7)) - 1 + (1 if 3 % 7 == 0 else 0) and np.abs(res["B"] - b).max() <= 1e-9
    assert O.fit(x[:k + 1], c, P, D[:k + 1] * 0 + 1.0)["status"] == 1
    P2 = np.concatenate([P, P[:1]])
    assert O.fit(x, c, P2, Y @ b.T)["status"] == 2 and O.fit(x, c, P2, Y @ b.T, 1e-3)["status"] == 0
    flat = O.fit(x, c, P, np.ones((T, 1)))
    assert flat["status"] == 0 and flat["B"].tolist() == [[0.0] * k] and flat["r2"].tolist() == [0.0]
    assert O.pack(res).size == O.layout(k, N)[1] == 1 + k + N + N * N + N * k + N


def test_op_codes_roles_and_limits():
    from rawaudiovae_kelsey_amd import _lib
    from rawaudiovae_kelsey_amd import attributes as A
    text = open(REPO + "/include/rawvae_hip.h").read()
    codes = dict(re.findall(r"#define (RV_ATTR_\w+) (\d+)", text))
    assert codes == dict(RV_ATTR_DESCRIBE="49", RV_ATTR_FIT="50", RV_ATTR_WORKSPACE="51")
    assert (_lib.ATTR_DESCRIBE, _lib.ATTR_FIT, _lib.ATTR_WORKSPACE) == (49, 50, 51)
    assert _lib.ATTR_WORKSPACE in _lib._HOST_ONLY_OPS and _lib.ATTR_FIT not in _lib._HOST_ONLY_OPS
    assert _lib.ATTR_DESCRIBE not in _lib._HOST_ONLY_OPS
    para = text[text.index("/* Latent attributes"):text.index("#define RV_ATTR_DESCRIBE")]
    types = {n: ctype for slot in abi_slots.header_slots() for n, ctype in slot}
    for field, ctype in (("frames", "const float*"), ("n_out", "long"), ("T", "long"), ("S", "long"), ("hop", "long"),
                         ("window", "const float*"), ("twiddles", "const float*"), ("dynamic_range", "float"),
                         ("result", "double*"), ("ldo", "long"), ("q", "const float*"), ("stride", "long"), ("centre", "double*"),
                         ("basis", "double*"), ("moment", "const double*"), ("lam", "float"), ("ws", "void*"), ("ws_bytes", "long"),
                         ("L", "long"), ("k", "long"), ("N", "long"), ("info", "int*")):
        assert re.search(r"\b%s\b" % field, para), field
        assert hasattr(_lib.MosaicDesc, field) and types[field] == ctype, (field, types.get(field))
    assert len(abi_slots.check_layout()) == 37 and C.sizeof(_lib.MosaicDesc) == 37 * 8
    assert _lib.lib().rv_version() == 100 and "attr" not in " ".join(_lib.EXPORTED)
    for op in (38, 39, 42, 48):     # still unassigned
        with pytest.raises(_lib.RvError, match="unknown op %d" % op):
            _lib.lib().rv_mosaic(op, C.byref(_lib.MosaicDesc()), None)
    up = lambda n: -(-n // 256) * 256   # noqa: E731
    sizes = []
    for T in (2, 5000, 9000):
        d = _lib.mosaic_call(_lib.ATTR_WORKSPACE, T=T, k=33, N=5)
        nb, nr = -(-T // 256), -(-T // 4096)
        assert d.ws_bytes == up(T * 33 * 8) + up(T * 5 * 8) + up(T) + up(nb * 39 * 8) + nr * 3 * 64 * 64 * 8
        sizes.append(d.ws_bytes)
    assert sizes[0] < sizes[1] < sizes[2]
    assert (A.K_MAX, A.N_MAX, A.L_MAX) == (64, 64, 512) and A.NAMES == O.NAMES
    assert A.result_layout(7, 3) == O.layout(7, 3)


def _err(op, text, **fields):
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError) as e:
        _lib.lib().rv_mosaic(op, C.byref(_lib.MosaicDesc(**fields)), None)
    assert text in str(e.value), str(e.value)


def test_every_op_names_the_offending_field_before_it_launches():
    from rawaudiovae_kelsey_amd import _lib
    p = 0x1000     # never dereferenced: every call here fails a check
    desc = dict(T=10, S=64, hop=16, frames=p, n_out=9 * 16 + 64, window=p, twiddles=p, dynamic_range=60.0, result=p, ldo=5)
    for change, text in ((dict(T=0), "T=0 outside [1, 2^31)"), (dict(T=1 << 31), "T=2147483648 outside [1, 2^31)"),
                         (dict(S=0), "S=0 outside [1, 2^31)"), (dict(hop=0), "hop=0 outside [1, 2^31)"),
                         (dict(frames=None), "frames is null"), (dict(result=None), "result (desc) is null"),
                         (dict(n_out=9 * 16 + 63), "T=10 frames of S=64 at hop=16 overrun n_out=207"),
                         (dict(T=11), "T=11 frames of S=64 at hop=16 overrun n_out=208"),
                         (dict(dynamic_range=0.0), "dynamic_range=0 dB must be in (0, 120]"),
                         (dict(dynamic_range=121.0), "dynamic_range=121 dB must be in (0, 120]"),
                         (dict(dynamic_range=float("nan")), "dynamic_range=nan dB must be in (0, 120]"),
                         (dict(ldo=4), "ldo=4 holds no row of 5 descriptors"),
                         (dict(ldo=2, window=None), "ldo=2 holds no row of 3 descriptors"),
                         (dict(S=48, n_out=1000), "S=48: the spectral columns (window given) need a power of two in [32, 4096]"),
                         (dict(S=16, n_out=1000), "S=16: the spectral columns"), (dict(S=8192, n_out=100000), "S=8192: the spectral columns"),
                         (dict(twiddles=None), "window given but twiddles is null")):
        _err(_lib.ATTR_DESCRIBE, "rv_mosaic(ATTR_DESCRIBE): " + text, **dict(desc, **change))
    need = _lib.mosaic_call(_lib.ATTR_WORKSPACE, T=300, k=4, N=3).ws_bytes
    fit = dict(T=300, L=6, k=4, N=3, q=p, stride=6, centre=p, basis=p, moment=p, lam=0.0, result=p, info=p, ws=p,
               ws_bytes=need)
    for name, op, ok in (("ATTR_FIT", _lib.ATTR_FIT, fit), ("ATTR_WORKSPACE", _lib.ATTR_WORKSPACE, dict(T=300, k=4, N=3))):
        for change, text in ((dict(T=1), "T=1 outside [2, 2^31)"), (dict(T=1 << 31), "T=2147483648 outside [2, 2^31)"),
                             (dict(k=0), "k=0 (the axes) outside [1, 64]"), (dict(k=65, L=70, stride=70), "k=65 (the axes) outside [1, 64]"),
                             (dict(N=0), "N=0 (the targets) outside [1, 64]"), (dict(N=65), "N=65 (the targets) outside [1, 64]")):
            _err(op, "rv_mosaic(%s): %s" % (name, text), **dict(ok, **change))
    for change, text in ((dict(L=3), "L=3 outside [k=4, 512]"), (dict(L=513, stride=513), "L=513 outside [k=4, 512]"),
                         (dict(stride=5), "stride=5 (the row pitch of x) holds no row of L=6 values"),
                         (dict(q=None), "q (the latent rows x) is null"), (dict(centre=None), "centre is null"),
                         (dict(basis=None), "basis (P) is null"), (dict(moment=None), "moment (the targets D) is null"),
                         (dict(lam=-1e-3), "lam=-0.001 (the ridge) must be finite and >= 0"),
                         (dict(lam=float("nan")), "lam=nan (the ridge) must be finite and >= 0"),
                         (dict(lam=float("inf")), "lam=inf (the ridge) must be finite and >= 0"),
                         (dict(result=None), "result is null"), (dict(info=None), "info is null"),
                         (dict(ws_bytes=need - 1), "ws_bytes=%d, T=300 frames of k=4 axes and N=3 targets need %d" % (need - 1, need)),
                         (dict(ws=None), "ws is null, T=300 frames"), (dict(ws=p + 8), "ws is not 256-byte aligned")):
        _err(_lib.ATTR_FIT, "rv_mosaic(ATTR_FIT): " + text, **dict(fit, **change))


def _planted(N=4, k=6, L=9, seed=0):
    from rawaudiovae_kelsey_amd import attributes as A
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((N, k))
    V = np.linalg.qr(rng.standard_normal((L, L)))[0][:k]
    R = V * np.sqrt(np.linspace(2.0, 0.5, k))[:, None]
    std = np.abs(rng.standard_normal(N)) + 0.5
    names = ("level", "zcr", "crest", "centroid", "flatness")[:N]
    corr = np.eye(N)
    return A.LatentAttributes(names)._set(B, rng.standard_normal(N), std, rng.uniform(0, 1, N), corr, R, 900, 1000, 0.25), B, R


def test_move_on_a_planted_B():
    from rawaudiovae_kelsey_amd import attributes as A
    at, B, R = _planted()
    off, pred, norm = at.move({"centroid": 0.02, "level": -3.0})
    assert off.dtype == torch.float32 and off.shape == (9,) and off.device.type == "cpu"
    assert abs(pred[3] - 0.02) <= 1e-12 and abs(pred[0] + 3.0) <= 1e-12
    want_off, want_pred, want_norm = O.move(B, R, [0, 3], [-3.0, 0.02])
    assert np.array_equal(off.numpy(), want_off.astype(np.float32)) and np.allclose(pred, want_pred, rtol=0, atol=1e-12)
    assert abs(norm - want_norm) <= 1e-12 * want_norm
    # the least-norm step: any other w with the same two changes is longer
    w = np.linalg.lstsq(R.T, want_off, rcond=None)[0]
    assert abs(np.sqrt(w @ w) - norm) <= 1e-9
    off_h, pred_h, norm_h = at.move({"centroid": 0.02, "level": -3.0}, hold=True)
    assert abs(pred_h[3] - 0.02) <= 1e-12 and abs(pred_h[0] + 3.0) <= 1e-12 and np.abs(pred_h[[1, 2]]).max() <= 1e-12
    assert norm_h > norm
    off0, pred0, norm0 = at.move({})
    assert not off0.any() and not pred0.any() and norm0 == 0.0
    off0h, pred0h, norm0h = at.move({}, hold=True)
    assert not off0h.any() and norm0h == 0.0
    # two parallel rows cannot be set apart
    B2 = B.copy()
    B2[2] = 2.0 * B2[1]
    par = A.LatentAttributes(at.names)._set(B2, at.mean_, at.std_, at.r2_, at.corr_, R, 900, 1000)
    with pytest.raises(ValueError, match="the directions of zcr, crest cannot be set apart: M M\\^T has condition number"):
        par.move({"zcr": 1.0, "crest": 1.0})
    with pytest.raises(ValueError, match="level, zcr, crest, centroid cannot be set apart"):
        par.move({"level": 1.0}, hold=True)
    assert abs(par.move({"zcr": 1.0})[1][2] - 2.0) <= 1e-12      # alone it moves, and drags its parallel along
    with pytest.raises(ValueError, match="unknown descriptor 'pitch': the fit holds level, zcr, crest, centroid"):
        at.move({"pitch": 1.0})
    with pytest.raises(ValueError, match="descriptor 'zcr': the move must be finite"):
        at.move({"zcr": float("nan")})
    with pytest.raises(RuntimeError, match="has not been fitted"):
        A.LatentAttributes().move({})
    for bad in ((), ("a", "a"), ("a,b",), ("a:b",), ("",)):
        with pytest.raises(ValueError, match="names="):
            A.LatentAttributes(bad)
    with pytest.raises(ValueError, match="x must be a 2-D float32 device tensor with at least two rows"):
        A.LatentAttributes().fit(torch.zeros(9, 8), torch.zeros(9, 5, dtype=torch.float64), (np.zeros(8), np.eye(8)[:2]))
    with pytest.raises(ValueError, match="targets has 4 columns for the 5 names"):
        A.LatentAttributes().fit(torch.zeros(9, 8), torch.zeros(9, 4, dtype=torch.float64), (np.zeros(8), np.eye(8)[:2]))
    with pytest.raises(ValueError, match="padded must be a contiguous float32 device tensor"):
        A.describe(torch.zeros(100), 1, 64, 64)
    with pytest.raises(TypeError, match="expected a fitted LatentPCA or a \\(centre, P\\) pair"):
        A.axes("pca.npz")
    with pytest.raises(ValueError, match="n_components=3: the basis holds 2 axes and the attribute fit takes at most 64"):
        A.axes((np.zeros(8), np.eye(8)[:2]), 3)
    c, P, R2 = A.axes((np.zeros(3), np.diag([2.0, 4.0, 5.0])[:2]))
    assert np.allclose(R2, np.diag([0.5, 0.25, 0.2])[:2]) and P.dtype == torch.float64


def test_npz_round_trip_and_the_hop_check(tmp_path):
    import attributes as cli
    from rawaudiovae_kelsey_amd import attributes as A
    from rawaudiovae_kelsey_amd import corpus as C_
    at, B, R = _planted()
    path = str(tmp_path / "attrs.npz")
    A.write_attributes(path, at, 64, 16)
    back, meta = A.read_attributes(path, "cpu")
    assert meta == dict(segment_length=64, latent_dim=9, hop=16, n_frames=1000, n_observed=900)
    assert back.names == at.names and back.ridge == 0.25 and (back.n_observed_, back.n_frames_) == (900, 1000)
    for a, b in ((back.B_, at.B_), (back.mean_, at.mean_), (back.std_, at.std_), (back.r2_, at.r2_), (back.corr_, at.corr_),
                 (back.R_, at.R_)):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    m = {"level": -3.0, "zcr": 0.01}
    assert torch.equal(back.move(m, True)[0], at.move(m, True)[0])
    A.write_attributes(path, at, 64)
    assert A.read_attributes(path, "cpu")[1]["hop"] is None
    check_hop = lambda *a: C_.check_hop(*a, *cli.HOP_PHRASES)     # noqa: E731
    assert check_hop(16, 16, 64) == 16 and check_hop(None, None, 64) == 64
    with pytest.raises(ValueError, match="hop 32: the attributes were fitted at hop 16"):
        check_hop(16, 32, 64)
    with np.load(path) as z:
        arrays = {n: z[n] for n in z.files}
    np.savez(path, **{n: v for n, v in arrays.items() if n != "R"})
    with pytest.raises(ValueError, match="not a latent-attributes file, it lacks R"):
        A.read_attributes(path, "cpu")
    np.savez(path, **dict(arrays, B=arrays["B"][:-1]))
    with pytest.raises(ValueError, match="do not fit 4 descriptors, 6 components and latent_dim 9"):
        A.read_attributes(path, "cpu")
    np.savez(path, **dict(arrays, std=arrays["std"][:-1]))
    with pytest.raises(ValueError, match="attrs.npz: B .* do not fit 4 descriptors"):
        A.read_attributes(path, "cpu")


def test_attributes_py_names_the_bad_flag(tmp_path):
    import attributes as cli
    fit = ["fit", "--checkpoint", "c", "--data", "d", "--out", "o"]
    for extra, text in ((["--keep", "65"], "--keep 65: at most 64"), (["--keep", "x"], "--keep 'x'"),
                        (["--keep", "0"], "--keep '0': expected a positive integer"), (["--hop", "0"], "--hop '0'"),
                        (["--ridge", "-1"], "--ridge '-1': expected a finite number >= 0"),
                        (["--ridge", "nan"], "--ridge 'nan'"),
                        (["--targets", "t.npy"], "--targets and --names come together: --names is missing"),
                        (["--names", "a,b"], "--targets and --names come together: --targets is missing"),
                        (["--targets", "t.npy", "--names", "a,a"], "--names 'a,a': expected distinct non-empty names")):
        with pytest.raises(ValueError) as e:
            cli.parse_args(fit + extra)
        assert text in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="expected a command: measure, fit, move or edit"):
        cli.parse_args([])
    a = cli.parse_args(fit + ["--keep", "3", "--hop", "16", "--ridge", "1e-3"])
    assert (a.keep, a.hop, a.ridge, a.pca, a.targets, a.names) == (3, 16, 1e-3, None, None, None)
    meas = ["measure", "--in", "a.wav", "--out", "d.npy"]
    for extra, text in ((["--segment-length", "1000"], "--segment-length 1000: --window hann needs a power of two in [32, 4096]"),
                        (["--segment-length", "0"], "--segment-length '0'"),
                        (["--segment-length", "64", "--hop", "24"], "--hop 24: does not divide --segment-length 64"),
                        (["--segment-length", "64", "--window", "blackman"], "--window 'blackman': expected none or hann")):
        with pytest.raises(ValueError) as e:
            cli.parse_args(meas + extra)
        assert text in str(e.value), str(e.value)
    a = cli.parse_args(meas + ["--segment-length", "1000", "--window", "none", "--hop", "250"])
    assert (a.segment_length, a.window, a.hop) == (1000, None, 250)
    mv = ["move", "--attrs", "a.npz", "--out", "o.npy"]
    for text_in, text in (("centroid", "--move 'centroid': expected NAME:DELTA,..., got 'centroid'"),
                          ("centroid:x", "expected NAME:DELTA,..., got 'centroid:x'"), (":1", "expected NAME:DELTA"),
                          ("level:inf", "level: the change must be finite"), ("level:1,level:2", "level is given twice")):
        with pytest.raises(ValueError) as e:
            cli.parse_args(mv + ["--move", text_in])
        assert text in str(e.value), str(e.value)
    a = cli.parse_args(mv + ["--move", "centroid:+0.02,level:-3", "--hold"])
    assert a.move == {"centroid": 0.02, "level": -3.0} and a.hold is True
    assert cli.parse_args(mv).move == {} and cli.parse_args(mv).hold is False
    with pytest.raises(ValueError, match="--attrs 'none.npz': no such file"):
        cli.main(mv[:1] + ["--attrs", "none.npz", "--out", "o.npy", "--move", "level:1"])
    # move needs no GPU: the offset file is LatentAttributes.move's
    from rawaudiovae_kelsey_amd import attributes as A
    at, B, R = _planted()
    npz, out = str(tmp_path / "a.npz"), str(tmp_path / "o.npy")
    A.write_attributes(npz, at, 64, 16)
    rep = cli.main(["move", "--attrs", npz, "--out", out, "--move", "centroid:+0.02,level:-3", "--hold"])
    off, pred, norm = at.move({"centroid": 0.02, "level": -3.0}, hold=True)
    assert np.array_equal(np.load(out), off.numpy()) and rep["predicted"] == [float(v) for v in pred] and rep["norm"] == norm
    assert rep["requested"] == [-3.0, None, None, 0.02]
    with pytest.raises(ValueError, match="--move: unknown descriptor 'pitch'"):
        cli.main(["move", "--attrs", npz, "--out", out, "--move", "pitch:1"])
    with pytest.raises(ValueError, match="--attrs: .*not a latent-attributes file"):
        np.savez(str(tmp_path / "b.npz"), B=B)
        cli.main(["move", "--attrs", str(tmp_path / "b.npz"), "--out", out])
    ed = ["edit", "--checkpoint", "c", "--attrs", "a.npz", "--in", "a.wav", "--out", "b.wav"]
    with pytest.raises(ValueError, match="--window 'x': expected none or hann"):
        cli.parse_args(ed + ["--window", "x"])
    a = cli.parse_args(ed + ["--hop", "16", "--window", "hann", "--move", "zcr:0.1"])
    assert (a.hop, a.window, a.move, a.hold) == (16, "hann", {"zcr": 0.1}, False)
