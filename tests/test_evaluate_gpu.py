"""RV_EVAL_FRAMES / RV_EVAL_DIMS and the Evaluator on the GPU against tests/eval_oracle.py.

Tolerances.  Columns 0..2 (fp64 sums rounded once to fp32): relative error at most 2^-22 against the float64 oracle;
RV_EVAL_DIMS' fp64 cost: 1e-12.  Columns 3..5: the oracle's float32 restatement of the kernel's algorithm is run on the
same inputs; its worst disagreement with the float64 oracle, per column and per S over every case of that S, is the
yardstick, and the kernel may disagree with float64 by 4 times that (another butterfly order, the GPU's log10 / sqrt).
The error measures: column 3 the difference in dB; column 4 the difference over max(spec_err, spec_ref) of the float64
row (its natural scale: (sqrt Pa - sqrt Pb)^2 <= max(Pa, Pb)); column 5 the relative difference.  A row whose float64
scale is 0 (silence) must be exactly 0, a NaN row NaN.

Yardstick values of the float32 restatement on these inputs (R = 60 dB), measured on the CPU:

    S       lsd (dB)    spec_err    spec_ref
    32      3.1e-05     1.7e-07     1.4e-07
    64      1.2e-05     1.3e-07     1.7e-07
    1024    3.1e-06     1.5e-07     2.1e-07
    4096    3.4e-06     1.0e-07     2.2e-07

(the test recomputes them; it does not read this table).
"""
import ctypes as C
import configparser
import functools
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import eval_oracle as O  # noqa: E402
from guarded import guarded, guarded_flat  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (32, 64, 1024, 4096)
L_OF = {32: 1, 64: 8, 1024: 100, 4096: 256, 1000: 8}
T_ALL = 67
R_DB = 60.0
EPS32 = 2.0 ** -22
LAYOUTS = ("packed", "padded", "overlap")


def _rows(S, seed):
    """T_ALL frame pairs [T, S]: noise, on-bin and off-bin sines, a pair 80 dB apart (both ways), silence on either
    side and on both, identical pairs, in turn."""
    rng = np.random.default_rng(seed)
    n = np.arange(S)
    X, Y = np.empty((T_ALL, S)), np.empty((T_ALL, S))
    for t in range(T_ALL):
        kind = t % 9
        x = rng.uniform(-1, 1, S)
        y = np.tanh(x + 0.3 * rng.standard_normal(S))
        if kind == 1:
            x = np.sin(2 * np.pi * rng.integers(1, S // 4) * n / S)
            y = 0.7 * np.sin(2 * np.pi * rng.integers(1, S // 4) * n / S + 1)
        elif kind == 2:
            x = np.sin(2 * np.pi * rng.uniform(1, S / 4) * n / S) + 1e-3 * rng.standard_normal(S)
            y = 0.5 * x + 1e-3 * rng.standard_normal(S)
        elif kind == 3:
            x = 1e-4 * x
        elif kind == 4:
            y = 1e-4 * y
        elif kind == 5:
            y = np.zeros(S)
        elif kind == 6:
            x = np.zeros(S)
        elif kind == 7:
            x = y = np.zeros(S)
        elif kind == 8:
            y = x
        X[t], Y[t] = x, y
    return X.astype(np.float32), Y.astype(np.float32)


def _waves(S, seed):
    """Two waveforms framed at hop = S / 4 (overlapping rows): noise, a tone, silence and a stretch where they agree."""
    rng = np.random.default_rng(seed)
    hop = S // 4
    n = (T_ALL - 1) * hop + S
    x = rng.uniform(-1, 1, n)
    x[n // 5:2 * n // 5] = np.sin(2 * np.pi * 3.37 * np.arange(n // 5, 2 * n // 5) / S)
    y = np.tanh(x + 0.2 * rng.standard_normal(n))
    y[3 * n // 5:4 * n // 5] = x[3 * n // 5:4 * n // 5]
    x[9 * n // 10:] = 0
    y[17 * n // 20:] = 0
    return x.astype(np.float32), y.astype(np.float32)


def _latents(T, L, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, L)).astype(np.float32), (0.7 * rng.standard_normal((T, L))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(S, layout):
    """The inputs of one case and both oracle runs, computed once: dict(x, y flat waves, hop, stride, ldo, mu, lv,
    f64, f32)."""
    L = L_OF[S]
    seed = 100 * SIZES.index(S) + LAYOUTS.index(layout) if S in SIZES else 999
    if layout == "overlap":
        x, y = _waves(S, seed)
        hop = stride = S // 4
        mu = lv = None
        ldo = 6
    else:
        X, Y = _rows(S, seed)
        hop = S
        stride = S if layout == "packed" else S + 3
        x = X.reshape(-1)
        yy = np.full((T_ALL, stride), np.nan, dtype=np.float32)      # the gap of a padded row is never read
        yy[:, :S] = Y
        y = yy.reshape(-1)[:(T_ALL - 1) * stride + S]
        mu, lv = _latents(T_ALL, L, seed + 7)
        ldo = 6 if layout == "packed" else 9
    w = O.hann(S) if S in SIZES else None
    f64 = O.frame_scores(x, hop, y, stride, T_ALL, S, mu, lv, w, R_DB)
    f32 = O.frame_scores(x, hop, y, stride, T_ALL, S, mu, lv, w, R_DB, dtype=np.float32) if w is not None else f64
    for a in (x, y, f64, f32):
        a.setflags(write=False)
    return dict(x=x, y=y, hop=hop, stride=stride, ldo=ldo, mu=mu, lv=lv, w=w, f64=f64, f32=f32)


def _spectral_errors(got, f64):
    """[T, 3] error measures of columns 3..5 (see the module doc); rows without a scale are left out (NaN)."""
    err = np.full((f64.shape[0], 3), np.nan)
    with np.errstate(all="ignore"):
        err[:, 0] = np.abs(got[:, 3] - f64[:, 3])
        s4 = np.maximum(f64[:, 4], f64[:, 5])
        err[:, 1] = np.where(s4 > 0, np.abs(got[:, 4] - f64[:, 4]) / s4, np.nan)
        err[:, 2] = np.where(f64[:, 5] > 0, np.abs(got[:, 5] - f64[:, 5]) / f64[:, 5], np.nan)
    return err


@functools.lru_cache(maxsize=None)
def _yardstick(S):
    """[3]: the float32 restatement's worst error per column over every case of S"""
    worst = np.zeros(3)
    for layout in LAYOUTS:
        c = _case(S, layout)
        worst = np.maximum(worst, np.nanmax(_spectral_errors(c["f32"], c["f64"]), axis=0))
    assert np.all(worst > 0) and worst[0] < 1e-4 and np.all(worst[1:] < 1e-6), worst
    return worst


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()       # (a copy: the cached inputs are read-only)


def _spec(S, w):
    from rawaudiovae_kelsey_amd.evaluate import twiddle_table
    return (None, None) if w is None else (_dev(w), _dev(twiddle_table(S)))


def _run(c, S, T=T_ALL, row0=0, ldo=None, x=None, y=None):
    """RV_EVAL_FRAMES on rows [row0, row0 + T) of case c into a guarded [T, ldo] output -> numpy [T, 6]"""
    from rawaudiovae_kelsey_amd.evaluate import frame_scores
    ldo = c["ldo"] if ldo is None else ldo
    xd, yd = _dev(c["x"] if x is None else x), _dev(c["y"] if y is None else y)
    mu, lv = (None, None) if c["mu"] is None else (_dev(c["mu"][row0:row0 + T]), _dev(c["lv"][row0:row0 + T]))
    win, tab = _spec(S, c["w"])
    out = guarded(T, 6, ldo, torch.float32)
    view = out.view if T > 1 else out.flat[out.front:out.front + ldo].view(1, ldo)
    frame_scores(xd[row0 * c["hop"]:], yd[row0 * c["stride"]:], T, S, c["hop"], c["stride"], mu, lv, win, tab, R_DB, out=view)
    torch.cuda.synchronize()
    out.assert_untouched("scores")
    return out.payload().cpu().numpy()


def _check(got, c, S, rows=slice(None)):
    f64 = c["f64"][rows]
    for col in (0, 1, 2):
        err = np.abs(got[:, col].astype(np.float64) - f64[:, col])
        print("S %d column %d: worst relative error %.3g (allowed %.3g)" % (S, col, np.max(err / np.maximum(f64[:, col], 1e-300)), EPS32))
        assert np.all(err <= EPS32 * f64[:, col]), (col, err.max())
    if c["w"] is None:
        assert np.all(got[:, 3:] == 0)
        return
    yard = _yardstick(S)
    err = _spectral_errors(got.astype(np.float64), f64)
    print("S %d: kernel's worst errors %s, yardstick %s" % (S, np.nanmax(err, axis=0), yard))
    for j in range(3):
        scaled = ~np.isnan(err[:, j])
        assert np.all(err[scaled, j] <= 4 * yard[j]), (3 + j, np.nanmax(err[:, j]), yard[j])
        assert np.all(got[~scaled, 3 + j] == 0) and np.all(f64[~scaled, 3 + j] == 0)      # silence: exactly 0


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("S", SIZES)
def test_frame_scores_against_the_oracle(S, layout):
    c = _case(S, layout)
    got = _run(c, S)
    assert np.all(np.isfinite(got))
    _check(got, c, S)
    again = _run(c, S)
    assert np.array_equal(got.view(np.int32), again.view(np.int32))                       # run to run
    # a row scored alone, two rows, another ldo: the same bits as inside the batch
    for row0, T in ((0, 1), (T_ALL - 1, 1), (8, 1), (30, 2)):
        part = _run(c, S, T=T, row0=row0, ldo=15 - c["ldo"])
        assert np.array_equal(part.view(np.int32), got[row0:row0 + T].view(np.int32)), (row0, T)
    if layout != "overlap":
        same = [t for t in range(T_ALL) if t % 9 in (7, 8)]
        assert np.all(got[same][:, [0, 3, 4]].view(np.int32) == 0)                        # identical pairs: +0


@pytest.mark.parametrize("hop", [1000, 250])
def test_frame_scores_without_a_window_take_any_length(hop):
    S = 1000
    X, Y = _rows(S, 5)
    if hop == S:
        x, y = X.reshape(-1), Y.reshape(-1)
    else:
        x, y = _waves(S, 6)
    mu, lv = _latents(T_ALL, 8, 9)
    c = dict(x=x, y=y, hop=hop, stride=hop, ldo=6, mu=mu, lv=lv, w=None,
             f64=O.frame_scores(x, hop, y, hop, T_ALL, S, mu, lv))
    got = _run(c, S)
    _check(got, c, S)
    assert np.array_equal(_run(c, S, T=1, row0=40, ldo=9), got[40:41])


@pytest.mark.parametrize("S", [64, 1024])
def test_a_nan_row_touches_no_other_row(S):
    c = _case(S, "packed")
    clean = _run(c, S)
    x, y = c["x"].copy(), c["y"].copy()
    x[3 * S + 5] = np.nan
    y[10 * S + S - 1] = np.inf
    got = _run(c, S, x=x, y=y)
    assert np.all(np.isnan(got[3][[0, 1, 3, 4, 5]])) and got[3, 2] == clean[3, 2]
    assert not np.isfinite(got[10, 0]) and got[10, 1] == clean[10, 1] and np.all(np.isnan(got[10, 3:5]))
    assert got[10, 5] == clean[10, 5]
    keep = [t for t in range(T_ALL) if t not in (3, 10)]
    assert np.array_equal(got[keep].view(np.int32), clean[keep].view(np.int32))
    want = O.frame_scores(x, S, y, S, T_ALL, S, c["mu"], c["lv"], c["w"], R_DB)
    assert np.array_equal(np.isnan(want), np.isnan(got))


def _dims(mu, lv):
    """RV_EVAL_DIMS with cost and ws between guard bands -> (cost [L] float64, the call repeated: the same bits)"""
    from rawaudiovae_kelsey_amd import _lib
    T, L = mu.shape
    nb = -(-T // 256)
    nbytes = 8 * nb * L if nb > 1 else 0
    md, ld = _dev(mu), _dev(lv)
    outs = []
    for _ in range(2):
        cost = guarded_flat(2 * L, torch.float32)                 # fp64 values in a guarded fp32 buffer (16-byte aligned)
        ws = guarded_flat(max(2 * nb * L, 2), torch.float32)
        d = _lib.MosaicDesc(T=T, L=L, q=md.data_ptr(), c=ld.data_ptr(), cost=cost.ptr, ws=ws.ptr if nbytes else None,
                            ws_bytes=nbytes)
        _lib.lib().rv_mosaic(_lib.EVAL_DIMS, C.byref(d), None)
        torch.cuda.synchronize()
        cost.assert_untouched("cost")
        ws.assert_untouched("ws")
        if not nbytes:
            assert np.all(ws.payload().cpu().numpy() == 7.0)      # up to one block the scratch is not used
        outs.append(cost.payload().view(-1).view(torch.float64).cpu().numpy())
    assert np.array_equal(outs[0].view(np.int64), outs[1].view(np.int64))
    return outs[0]


@pytest.mark.parametrize("T", [1, 255, 257, 3 * 256 + 5, 9 * 256 + 5])   # ten blocks: the total's group of eight, then two
@pytest.mark.parametrize("L", [1, 8, 100, 256])
def test_kl_dims_against_the_oracle(T, L):
    from rawaudiovae_kelsey_amd.evaluate import kl_dims
    mu, lv = _latents(T, L, 11 * T + L)
    want = O.kl_dims(mu, lv)
    got = _dims(mu, lv)
    err = np.abs(got - want) / want
    print("T %d L %d: worst relative error %.3g" % (T, L, err.max()))
    assert np.all(err <= 1e-12)
    assert np.array_equal(kl_dims(_dev(mu), _dev(lv)).cpu().numpy().view(np.int64), got.view(np.int64))


# ---- the Evaluator ------------------------------------------------------------------------------------------------

def _model(S=64, H=96, L=8, seed=0):
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.synth import make_params
    m = VAE(S, H, L).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(S, H, L, seed).items()})
    return m


def _close(a, b, rtol):
    return abs(a - b) <= rtol * abs(b)


@pytest.mark.parametrize("hop", [None, 16])
def test_evaluator_report_equals_the_oracle_and_the_reference_loss(hop):
    from rawvae.model import loss_function
    from rawaudiovae_kelsey_amd.evaluate import Evaluator
    from rawaudiovae_kelsey_amd.interpolate import frame_layout
    from rawaudiovae_kelsey_amd.synth import make_eps
    S, L, kl_beta = 64, 8, 0.05
    model = _model()
    rng = np.random.default_rng(4)
    waves = [("a", (0.6 * rng.uniform(-1, 1, 700)).astype(np.float32)), ("b", np.sin(0.05 * np.arange(1290)).astype(np.float32))]
    step = S if hop is None else hop
    calls = model._rng_calls
    ev = {m: Evaluator(model, hop=hop, max_rows=m) for m in (3, 16384)}
    files, tensors = [], []
    for i, (name, w) in enumerate(waves):
        T, padded = frame_layout(w.size, S, hop)
        eps = make_eps(T, L, 50 + i)
        for e in ev.values():
            assert e.add(w, name, eps=eps) == T
        wp = np.zeros(padded, np.float32)
        wp[:w.size] = w
        x = torch.from_numpy(O.rows_of(wp, step, T, S)).cuda()
        with torch.no_grad():
            mu, lv = model.encode(x)
            z = model.reparameterize(mu, lv, torch.from_numpy(eps).cuda())
            recon = model.decode(z)
        tensors.append((recon, x, mu, lv))
        sc = O.frame_scores(wp, step, recon.cpu().numpy().reshape(-1), S, T, S, mu.cpu().numpy(), lv.cpu().numpy(),
                            O.hann(S), 60.0)
        files.append((name, sc, O.kl_dims(mu.cpu().numpy(), lv.cpu().numpy())))
    model._rng_calls = calls
    want = O.report(files, S, L, kl_beta)
    got = ev[16384].report(kl_beta)
    assert np.array_equal(ev[3].scores.cpu().numpy().view(np.int32), ev[16384].scores.cpu().numpy().view(np.int32))
    assert json.dumps(ev[3].report(kl_beta)) == json.dumps(got)                   # max_rows changes nothing

    def same(g, w):
        assert g["frames"] == w["frames"] and g["active_units"] == w["active_units"]
        for key in ("mse", "kld", "loss", "spectral_convergence"):
            assert _close(g[key], w[key], 1e-6), (key, g[key], w[key])
        assert abs(g["snr_db"] - w["snr_db"]) < 1e-5 and abs(g["lsd_db"] - w["lsd_db"]) < 1e-4
        assert np.allclose(g["kl_per_dim"], w["kl_per_dim"], rtol=1e-12, atol=0)
    same(got, want)
    for g, w in zip(got["files"], want["files"]):
        assert g["name"] == w["name"]
        same(g, w)
    cat = [torch.cat(t) for t in zip(*tensors)]
    ref = float(loss_function(cat[0], cat[1], cat[2], cat[3], kl_beta, S))
    assert _close(got["loss"], ref, 1e-6), (got["loss"], ref)
    # z = mu by default, deterministic; the seeded draw is another z and repeats
    a, ka = ev[3].score(waves[0][1])
    b, kb = ev[16384].score(waves[0][1])
    assert torch.equal(a, b) and torch.equal(ka, kb)
    s1, _ = ev[3].score(waves[0][1], seed=5)
    s2, _ = ev[16384].score(waves[0][1], seed=5)
    assert torch.equal(s1, s2) and not torch.equal(s1[:, 0], a[:, 0]) and torch.equal(s1[:, 1:3], a[:, 1:3])
    assert model._rng_calls == calls


def test_compare_of_a_wave_with_itself_and_with_its_half_gain_copy():
    from rawaudiovae_kelsey_amd.evaluate import compare
    rng = np.random.default_rng(8)
    w = rng.uniform(-1, 1, 5000).astype(np.float32)
    r, sc = compare(w, w, 1024, 256, return_scores=True)
    assert r["frames"] == sc.shape[0] == (5120 - 1024) // 256 + 1
    assert r["mse"] == 0 and r["lsd_db"] == 0 and r["spectral_convergence"] == 0 and r["snr_db"] == float("inf")
    assert np.all(sc.cpu().numpy()[:, [0, 2, 3, 4]].view(np.int32) == 0)
    r = compare(w, (np.float32(0.5) * w)[:4000], 1024, 256)                       # the shorter one is zero-padded
    assert r["frames"] == 17
    r = compare(torch.from_numpy(w).cuda(), np.float32(0.5) * w, 1024, 256, dynamic_range=120.0)
    db = 20 * np.log10(2.0)
    assert abs(r["snr_db"] - db) < 1e-4 and abs(r["spectral_convergence"] - 0.5) < 1e-6
    # white noise under a Hann window: every bin lies far above a floor 120 dB below the peak bin, so D = 6.02 dB
    # in every bin up to the floor's lift, (Pa + f) / (Pa / 4 + f) with f <= 1e-12 max Pa
    assert abs(r["lsd_db"] - db) < 1e-3
    r60 = compare(w, np.float32(0.5) * w, 1024, 256)
    assert r60["snr_db"] == r["snr_db"] and db - 0.5 < r60["lsd_db"] < db        # a 60 dB floor lifts the weakest bins
    r = compare(w, np.float32(0.5) * w, 1000, 250, window=None)
    assert abs(r["snr_db"] - db) < 1e-4 and r["lsd_db"] == 0 and r["spectral_convergence"] == 0


# ---- end to end ---------------------------------------------------------------------------------------------------

def test_evaluate_py_end_to_end(tmp_path):
    sys.path.insert(0, REPO)
    import evaluate as cli
    import test_train_entry as TE
    from rawaudiovae_kelsey_amd.frontend import load_model, read_model_config
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd.evaluate import Evaluator
    from rawvae.model import VAE
    ds = TE._dataset(tmp_path / "ds")
    ini = TE._ini(ds)
    torch.manual_seed(3)
    model = VAE(256, 128, 8).cuda()
    ck = tmp_path / "ckpt"
    torch.save({"epoch": 0, "state_dict": model.state_dict(), "optimizer": {}}, ck)
    out, npz = tmp_path / "r.json", tmp_path / "s.npz"
    rep = cli.main(["--config", str(ini), "--checkpoint", str(ck), "--data", str(ds / "audio"), "--out", str(out),
                    "--hop", "64", "--per-frame", str(npz), "--kl-beta", "0.25"])
    cfg = read_model_config(str(ini))
    ev = Evaluator(load_model(str(ck), cfg), hop=64)
    for name in ("a.wav", "b.wav"):
        ev.add(D.load_audio_mono(ds / "audio" / name, 8000), name)
    want = ev.report(0.25)
    on_disk = json.loads(out.read_text())
    for key, v in want.items():
        assert rep[key] == v and on_disk[key] == v, key
    assert [f["name"] for f in on_disk["files"]] == ["a.wav", "b.wav"] and on_disk["hop"] == 64
    z = np.load(npz)
    assert np.array_equal(z["scores"], ev.scores.cpu().numpy()) and list(z["offsets"]) == list(ev.offsets)
    assert list(z["names"]) == ["a.wav", "b.wav"]
    pair = cli.main(["--ref", str(ds / "audio" / "a.wav"), "--test", str(ds / "test_audio" / "t.wav"),
                     "--segment-length", "256", "--hop", "64", "--out", str(tmp_path / "p.json")])
    assert pair["frames"] == (int(1.3 * 8000) + 63) // 64 - 3 and np.isfinite(pair["snr_db"]) and pair["lsd_db"] > 0


def test_train_py_validation_is_opt_in_and_does_not_perturb_training(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import test_train_entry as TE
    import train as T
    plain = T.main(["--config", str(TE._ini(TE._dataset(tmp_path / "plain")))])
    out_plain = capsys.readouterr().out
    ds = TE._dataset(tmp_path / "val")
    valid = T.main(["--config", str(TE._ini(ds, mi355x__validate="True", mi355x__best_by="validation"))])
    out = capsys.readouterr().out
    assert "Validation" not in out_plain
    lines = [l for l in out.splitlines() if "Validation loss:" in l]
    assert len(lines) == 4 and all(l.startswith("====> Epoch: %d - Validation loss: " % i) for i, l in enumerate(lines))
    assert all(k in lines[0] for k in ("mse ", "kld ", "snr ", "lsd ", " dB"))
    losses = [float(l.split("Validation loss: ")[1].split(" ")[0]) for l in lines]
    cfg = configparser.ConfigParser(allow_no_value=True)
    cfg.read(valid / "config.ini")
    assert abs(float(cfg["training"]["validation_loss"]) - min(losses)) < 1e-8      # printed with nine decimals
    assert int(cfg["training"]["best_validation_epoch"]) == int(np.argmin(losses))
    plain_cfg = configparser.ConfigParser(allow_no_value=True)
    plain_cfg.read(plain / "config.ini")
    assert "validation_loss" not in plain_cfg["training"] and "best_validation_epoch" not in plain_cfg["training"]
    totals = lambda text: [l for l in text.splitlines() if l.startswith("====> Epoch") and "Total loss" in l]  # noqa: E731
    assert len(totals(out)) == 4 and totals(out) == totals(out_plain)      # the training lines: unchanged, bit for bit
    for name in ("ckpt_00002", "ckpt_00004"):
        a = torch.load(plain / "model/checkpoints" / name, weights_only=False)
        b = torch.load(valid / "model/checkpoints" / name, weights_only=False)
        for k in a["state_dict"]:
            assert torch.equal(a["state_dict"][k], b["state_dict"][k]), (name, k)
    assert (valid / "model/best_model.pt").exists()
    assert len(set(losses)) == 4          # the figures move from epoch to epoch: the live Parameters are read


def test_best_model_is_chosen_by_the_validation_loss(tmp_path, capsys, monkeypatch):
    """A planted validation loss that does not follow the training loss: checkpoints at epochs 1, 2, 3 see 3, 5, 4, so
    best_by = validation saves best_model.pt at epoch 1 alone, where the falling training loss would save at all three."""
    sys.path.insert(0, REPO)
    import test_train_entry as TE
    import train as T
    from rawaudiovae_kelsey_amd import evaluate as E
    planted = iter([9.0, 3.0, 5.0, 4.0])
    real = E.Evaluator.report

    def report(self, kl_beta, active_threshold=None):
        r = real(self, kl_beta, active_threshold)
        assert np.isfinite(r["loss"]) and r["frames"] > 0
        return dict(r, loss=next(planted))
    monkeypatch.setattr(E.Evaluator, "report", report)
    over = dict(training__checkpoint_interval="1", training__save_best_model_after="0")
    by_val = T.main(["--config", str(TE._ini(TE._dataset(tmp_path / "v"), mi355x__validate="True",
                                             mi355x__best_by="validation", **over))])
    out = capsys.readouterr().out
    cfg = configparser.ConfigParser(allow_no_value=True)
    cfg.read(by_val / "config.ini")
    saved = [l for l in out.splitlines() if l.startswith("Epoch 0") and ": Saved " in l]
    assert cfg["training"]["best_epoch"] == "1" and len(saved) == 1 and saved[0].startswith("Epoch 00001: Saved")
    assert out.count("Loss did not improve.") == 2 and "Final loss was not better than the last best model." in out
    assert float(cfg["training"]["validation_loss"]) == 3.0 and cfg["training"]["best_validation_epoch"] == "1"
    planted = iter([9.0, 3.0, 5.0, 4.0])
    by_train = T.main(["--config", str(TE._ini(TE._dataset(tmp_path / "t"), mi355x__validate="True", **over))])
    out = capsys.readouterr().out
    cfg = configparser.ConfigParser(allow_no_value=True)
    cfg.read(by_train / "config.ini")
    totals = [float(l.split("Total loss: ")[1].split(" - ")[0]) for l in out.splitlines() if "Total loss" in l]
    want = [e for e in (1, 2, 3) if totals[e] < min([float("inf")] + totals[1:e])]
    assert cfg["training"]["best_epoch"] == str(want[-1])      # the default rule: the training loss, whatever validation says
    assert cfg["training"]["best_validation_epoch"] == "1"
