"""The structure ops on the GPU (RV_STRUCT_*, csrc/structure.hip, rawaudiovae_kelsey_amd/structure.py, segment.py)
against tests/structure_oracle.py.  Everything is compared exactly: the novelty is fp64 with every product rounded before
it is added and every sum in a fixed order, the peak rule is comparisons of those values, so the curve's bits, the offsets
and the summary are the oracle's own.

Shapes.  T in {1, 2, R, 2R - 1, 2R, 2R + 1, 4R, 4R + 3, 300}: no past, windows cut at one or both ends, the first T with
a whole window, and more.  The kernel has one form: NOV_THREADS = 1024 threads take 1024 // 2R consecutive frames and
stage their shared window once, so what changes with R is that number of frames: R in {1, 2, 7, 32} (512, 256, 73, 16
frames) and the R on either side of 16 / 15 frames, of 4 / 3 and of 2 / 1, the last also where the staged window passes
64 KiB of LDS; R = 512 at T = 40 and T = 1100.  Every novelty and peaks call of this file reads its inputs from between
NaN guards and writes its outputs between sentinel guards.

R = 512 at T = 1100 is compared on 170 of its frames -- both ends, every frame whose window is whole (512 .. 588) and its
neighbours -- not on all 1100: the oracle's 1.15e9 terms take ten seconds in numpy, and every frame runs the same code."""
import functools
import json
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import align_oracle as AO  # noqa: E402
import structure_oracle as O  # noqa: E402
from guarded import SENTINEL, guarded, guarded_flat  # noqa: E402

pytestmark = pytest.mark.gpu

NOV_THREADS = 1024                   # csrc/structure.hip: a workgroup takes NOV_THREADS // 2R frames
THRESHOLD_RS = tuple(R + d for R in (NOV_THREADS // 32, NOV_THREADS // 8, NOV_THREADS // 4) for d in (0, 1))
LS = (1, 33, 64)
SIGMAS = (None, 0.5)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()     # a copy: the cached inputs are read-only


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def _between_nans(values):
    """A float64 device vector between two guards of 64 NaN: reading a guard poisons the result."""
    values = np.asarray(values, np.float64)
    flat = torch.full((values.size + 128,), float("nan"), dtype=torch.float64, device="cuda")
    flat[64:64 + values.size] = torch.from_numpy(values).cuda()
    return flat[64:64 + values.size]


def _Ts(R):
    return sorted({1, 2, R, 2 * R - 1, 2 * R, 2 * R + 1, 4 * R, 4 * R + 3, 300})


@functools.lru_cache(maxsize=None)
def _latents(T, L):
    mu = AO.random_latents(T, L, 31 * T + L)
    mu.setflags(write=False)
    return mu


@functools.lru_cache(maxsize=None)
def _full(T, L):
    """The oracle's full self-distance matrix [T, T] fp32, computed once and left unchanged."""
    mu = _latents(T, L)
    full = AO.local_costs(mu, mu, 0)[1]
    full.setflags(write=False)
    return full


def _device_costs(mu, r):
    """self_costs on the device, copied between NaN guards -> (the guarded [T, W] view, its numpy copy)."""
    from rawaudiovae_kelsey_amd import structure as S
    m = _dev(mu)
    dm = _np(S.self_costs(m, r))
    return guarded(dm.shape[0], dm.shape[1], dm.shape[1], torch.float32, fill=dm).view, dm


def _novelty(dmv, T, r, R, w):
    """RV_STRUCT_NOVELTY on a guarded Dm and taper into a guarded output -> nov as numpy."""
    from rawaudiovae_kelsey_amd import structure as S
    g = guarded_flat(2 * T, torch.float32)
    out = g.view.view(torch.float64).view(T)
    wv = _between_nans(w)
    got = S.novelty(dmv, T, r, R, wv, out=out)
    assert got.data_ptr() == out.data_ptr()
    g.assert_untouched("nov")
    return _np(out).copy()


def _peaks(curve, gap, m, delta):
    from rawaudiovae_kelsey_amd import structure as S
    T = len(curve)
    gp, gs = guarded_flat(T + 1, torch.float32), guarded_flat(4, torch.float32)
    out = (gp.view.view(torch.int32).view(T + 1), gs.view.view(torch.int32).view(4))
    S.peaks(_between_nans(curve), gap, m, delta, out=out)
    gp.assert_untouched("path")
    gs.assert_untouched("summary")
    return _np(out[0]).copy(), _np(out[1]).copy()


# ---- self costs ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,L,r", [(1, 3, 0), (1, 3, 1), (9, 1, 3), (130, 33, 0), (300, 64, 13), (300, 64, 69)])
def test_self_costs_have_a_zero_diagonal_and_are_the_searchs_distance(T, L, r):
    from rawaudiovae_kelsey_amd import align as A, structure as S
    mu = _latents(T, L)
    m = _dev(mu)
    got = _np(S.self_costs(m, r))
    want = AO.local_costs(mu, mu, r)[0]                  # mosaic_oracle.sq_dist in the band layout
    assert np.array_equal(_bits(got), _bits(want))
    diag = got[:, r] if r else np.diagonal(got)
    assert (diag == 0).all() and not np.signbit(diag).any()
    assert np.array_equal(_bits(_np(A.local_costs(m, m, r))), _bits(got))       # a and b the same pointer


# ---- novelty ---------------------------------------------------------------------------------------------------------

def _check_novelty(T, L, R, sigma, frames=None):
    mu, w = _latents(T, L), O.taper(R, sigma)
    want = O.novelty(_full(T, L), R, w, frames)
    sel = slice(None) if frames is None else np.asarray(frames)
    first = None
    for r in (0, 2 * R - 1, 2 * R + 5):
        if T * (2 * r + 1) >= 1 << 31:
            continue
        dmv, dm = _device_costs(mu, r)
        got = _novelty(dmv, T, r, R, w)
        assert np.array_equal(_bits(got[sel]), _bits(want)), (T, L, R, sigma, r, got[sel][:4], want[:4])
        if r:
            assert np.isinf(dm).any()                   # the band's +inf slots were there and were not read
        if first is None:
            first = got
        assert np.array_equal(_bits(got), _bits(first)), (T, L, R, sigma, r, "the band changed the bits")
    assert first[0] == 0.0 and not np.signbit(first[0])
    assert np.isfinite(first).all()
    return first


@pytest.mark.parametrize("R", [1, 2, 7])
def test_novelty_equals_the_oracle_bit_for_bit_every_combination(R):
    for T in _Ts(R):
        for L in LS:
            for sigma in SIGMAS:
                _check_novelty(T, L, R, sigma)


@pytest.mark.parametrize("R,n,T", [(R, n, T) for R in THRESHOLD_RS for n, T in enumerate(_Ts(R))])
def test_novelty_equals_the_oracle_bit_for_bit_across_the_thresholds(R, n, T):
    # L and sigma take turns over the T: each value of each meets small, cut and whole windows
    _check_novelty(T, LS[n % 3], R, SIGMAS[n % 2])
    if T == 300:
        _check_novelty(T, LS[(n + 1) % 3], R, SIGMAS[(n + 1) % 2])


def test_novelty_at_the_largest_kernel():
    R = 512
    nov = _check_novelty(40, 8, R, 0.5)
    assert (nov[1:] != 0).any()
    T = 1100
    frames = sorted(set(range(0, 40)) | set(range(500, 600)) | set(range(T - 30, T)))
    _check_novelty(T, 8, R, None, frames)


@pytest.mark.parametrize("T,L,R,row", [(60, 8, 7, 30), (60, 8, 7, 0), (60, 8, 7, 59), (200, 4, 33, 90), (300, 4, 129, 150),
                                       (600, 4, 257, 300)])
def test_a_nan_row_poisons_exactly_the_frames_whose_window_holds_it(T, L, R, row):
    mu, w = _latents(T, L), O.taper(R, 0.5)
    bad = mu.copy()
    bad[row] = np.nan
    want = O.novelty(AO.local_costs(bad, bad, 0)[1], R, w)
    hit = np.isnan(want)                                            # the exact window, from the oracle
    assert hit.any() and not hit.all() and (np.abs(np.nonzero(hit)[0] - row) <= R).all()
    assert hit[[t for t in range(1, T) if abs(t - row) < R]].all()
    clean = None
    for r in (0, 2 * R - 1):
        clean = _novelty(_device_costs(mu, r)[0], T, r, R, w)
        got = _novelty(_device_costs(bad, r)[0], T, r, R, w)
        assert np.array_equal(np.isnan(got), hit), (r, np.nonzero(np.isnan(got))[0], np.nonzero(hit)[0])
        assert np.array_equal(_bits(got[~hit]), _bits(clean[~hit])) and np.array_equal(_bits(got[~hit]), _bits(want[~hit]))


# ---- peaks -----------------------------------------------------------------------------------------------------------

def _curves(T, seed):
    rs = np.random.RandomState(seed)
    rnd = rs.randn(T)
    binary = rs.randint(0, 2, T).astype(np.float64)
    holes = rs.randn(T)
    holes[rs.rand(T) < 0.2] = np.nan
    holes[rs.rand(T) < 0.02] = np.inf
    return (("random", rnd), ("binary", binary), ("nan", holes))


@pytest.mark.parametrize("T", [1, 2, 255, 256, 257, 5000])
def test_peaks_are_exactly_the_oracles_offsets_and_summary(T):
    if T < 5000:
        combos = [(g, m, d) for g in (0, 1, 8, T + 3) for m in (0, 16) for d in (0.0, 0.5)]
    else:       # the oracle is a Python loop: every value of g, m and delta, not every combination
        combos = [(0, 16, 0.5), (1, 0, 0.0), (8, 16, 0.0), (8, 16, 0.5), (T, 16, 0.0)]
    some = 0
    for kind, curve in _curves(T, T):
        for g, m, d in combos:
            path, summary = _peaks(curve, g, m, d)
            wp, ws = O.peaks(curve, g, m, d)
            assert summary.tolist() == ws.tolist(), (T, kind, g, m, d, summary, ws)
            assert np.array_equal(path, wp), (T, kind, g, m, d)
            F = int(summary[0])
            assert path[0] == 0 and path[F] == T and (path[F + 1:] == -1).all() and (np.diff(path[:F + 1]) >= 1).all()
            assert (np.diff(path[1:F]) > g).all()
            if g >= T:
                assert F == 1
            some += F > 1
    assert some or T <= 2
    if T == 5000:
        assert _peaks(np.full(T, np.nan), 8, 16, 0.5)[1].tolist() == [1, 0, 0, 0]


def test_peaks_of_ties_and_nan_entries():
    curve = np.zeros(30)
    curve[[10, 11, 12, 20]] = 1.0
    for g, want in ((3, [0, 10, 20, 30]), (1, [0, 10, 20, 30]), (0, [0, 10, 11, 12, 20, 30])):
        path, summary = _peaks(curve, g, 30, 0.0)
        assert path[:summary[0] + 1].tolist() == want and summary.tolist() == [len(want) - 1, 30, 0, 0]
    curve = np.zeros(30)
    curve[[10, 20]] = 1.0
    curve[[9, 11, 21]] = np.nan
    path, summary = _peaks(curve, 3, 30, 0.0)
    assert path[:4].tolist() == [0, 10, 20, 30] and summary.tolist() == [3, 27, 0, 0]
    path, summary = _peaks(np.zeros(40), 4, 8, 0.0)               # a constant curve: one segment
    assert path[:2].tolist() == [0, 40] and (path[2:] == -1).all() and summary.tolist() == [1, 40, 0, 0]


# ---- planted structure, end to end -----------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [4, 8])
def test_planted_boundaries_means_and_labels(R):
    from rawaudiovae_kelsey_amd import som, structure as S
    mu, starts = O.planted()
    seg = S.segment_latents(_dev(mu), R, 0.5, 8, 16, 0.5)
    want_nov = O.novelty(AO.local_costs(mu, mu, 0)[1], R, O.taper(R, 0.5))
    want_path, want_summary = O.peaks(want_nov, 8, 16, 0.5)
    assert np.array_equal(_bits(_np(seg.novelty)), _bits(want_nov))
    assert np.array_equal(_np(seg.path), want_path) and _np(seg.summary).tolist() == want_summary.tolist()
    assert seg.F == 5 and seg.finite == 140 and seg.band == S.pick_band(140, R) == 2 * R - 1
    assert _np(seg.offsets).tolist() == [0] + starts + [140] and seg.boundary_frames.tolist() == starts
    means = som.segment_mean(_dev(mu), want_path[:6])
    assert torch.equal(seg.means, means) and seg.means.shape == (5, 8)
    assert np.array_equal(_bits(_np(seg.distances)), _bits(AO.local_costs(_np(means), _np(means), 0)[0]))
    assert seg.labels.tolist() == S.labels_from_distances(_np(seg.distances)).tolist() and seg.labels[:4].tolist() == [0, 1, 2, 3]
    # a planted A B A C
    mu, starts = O.planted(T=140, starts=(30, 70, 100), seed=1, centres=(0, 1, 0, 2))
    seg = S.segment_latents(_dev(mu), R, 0.5, 8, 16, 0.5)
    assert _np(seg.offsets).tolist() == [0, 30, 70, 100, 140]
    assert seg.labels.tolist() == [0, 1, 0, 2] and seg.form == "A B A C"


# ---- determinism, capture ----------------------------------------------------------------------------------------------

def test_two_runs_and_a_captured_replay_are_bit_equal():
    from rawaudiovae_kelsey_amd import structure as S
    for T, L, R in ((300, 33, 7), (700, 8, 40), (600, 8, 130), (700, 8, 300)):
        mu = _dev(_latents(T, L))
        runs = [S.segment_latents(mu, R, 0.5, 8, 16, 0.5) for _ in range(2)]
        cap = S.CapturedSegmentation(T, L, R, 0.5, 8, 16, 0.5).capture()
        other = cap.replay(torch.flip(mu, (0,)))                     # other operands first: the replay reads the buffers
        assert other.F >= 1
        runs.append(cap.replay(mu))
        ref = runs[0]
        assert ref.F > 1 and ref.F == int(ref.summary[0]) and ref.offsets.shape == (ref.F + 1,)
        for seg in runs[1:]:
            assert np.array_equal(_bits(_np(seg.novelty)), _bits(_np(ref.novelty)))
            assert torch.equal(seg.path, ref.path) and torch.equal(seg.summary, ref.summary)


# ---- errors ----------------------------------------------------------------------------------------------------------

def test_every_error_names_its_field_and_leaves_the_outputs_untouched():
    from rawaudiovae_kelsey_amd import _lib, structure as S
    T, R = 100, 8
    r = 2 * R - 1
    dm = S.self_costs(_dev(_latents(T, 8)), r)
    w = _dev(O.taper(R, 0.5))
    gn, gp, gs = guarded_flat(2 * T, torch.float32), guarded_flat(T + 1, torch.float32), guarded_flat(4, torch.float32)
    curve = _dev(np.random.RandomState(0).randn(T))
    ws = torch.full((S.workspace_bytes(T),), 7, dtype=torch.uint8, device="cuda")
    nov = dict(T=T, k=R, band=r, local_costs=dm.data_ptr(), moment=w.data_ptr(), result=gn.ptr)
    pk = dict(T=T, moment=curve.data_ptr(), lag=8, width=16, lam=0.5, ws=ws.data_ptr(), ws_bytes=ws.numel(), path=gp.ptr,
              summary=gs.ptr)
    bad = [(_lib.STRUCT_NOVELTY, nov, dict(T=0), "T=0"), (_lib.STRUCT_NOVELTY, nov, dict(k=0), "k=0"),
           (_lib.STRUCT_NOVELTY, nov, dict(k=513), "k=513"), (_lib.STRUCT_NOVELTY, nov, dict(band=-1), "band=-1"),
           (_lib.STRUCT_NOVELTY, nov, dict(band=r - 1), "band=%d does not hold the window of k=8; the least band that does is %d" % (r - 1, r)),
           (_lib.STRUCT_NOVELTY, nov, dict(T=1 << 16, band=0), "T=65536 rows of 65536 band slots"),
           (_lib.STRUCT_NOVELTY, nov, dict(local_costs=None), "local_costs is null"),
           (_lib.STRUCT_NOVELTY, nov, dict(moment=None), "moment is null"),
           (_lib.STRUCT_NOVELTY, nov, dict(result=None), "result is null"),
           (_lib.STRUCT_PEAKS, pk, dict(T=0), "T=0"), (_lib.STRUCT_PEAKS, pk, dict(lag=-1), "lag=-1"),
           (_lib.STRUCT_PEAKS, pk, dict(lag=65537), "lag=65537"), (_lib.STRUCT_PEAKS, pk, dict(width=-1), "width=-1"),
           (_lib.STRUCT_PEAKS, pk, dict(width=65537), "width=65537"), (_lib.STRUCT_PEAKS, pk, dict(lam=-1.0), "lam=-1"),
           (_lib.STRUCT_PEAKS, pk, dict(lam=float("nan")), "lam=nan"), (_lib.STRUCT_PEAKS, pk, dict(lam=float("inf")), "lam=inf"),
           (_lib.STRUCT_PEAKS, pk, dict(moment=None), "moment is null"), (_lib.STRUCT_PEAKS, pk, dict(path=None), "the path is null"),
           (_lib.STRUCT_PEAKS, pk, dict(summary=None), "the summary is null"), (_lib.STRUCT_PEAKS, pk, dict(ws=None), "ws is null"),
           (_lib.STRUCT_PEAKS, pk, dict(ws_bytes=ws.numel() - 1), "ws_bytes=%d" % (ws.numel() - 1))]
    for op, ok, change, what in bad:
        with pytest.raises(_lib.RvError) as e:
            _lib.lib().rv_mosaic(op, _lib.C.byref(_lib.MosaicDesc(**dict(ok, **change))), _lib.stream_ptr())
        assert what in str(e.value), (what, str(e.value))
        assert ("rv_mosaic(STRUCT_NOVELTY)" if op == _lib.STRUCT_NOVELTY else "rv_mosaic(STRUCT_PEAKS)") in str(e.value)
    torch.cuda.synchronize()
    for g, name in ((gn, "nov"), (gp, "path"), (gs, "summary")):
        g.assert_untouched(name)
        assert (_np(g.view) == SENTINEL).all(), name
    assert (_np(ws) == 7).all()
    # the same descriptors unchanged do run
    for op, ok in ((_lib.STRUCT_NOVELTY, nov), (_lib.STRUCT_PEAKS, pk)):
        _lib.lib().rv_mosaic(op, _lib.C.byref(_lib.MosaicDesc(**ok)), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert not (_np(gn.view) == SENTINEL).any() and int(_np(gs.view.view(torch.int32))[0, 0]) >= 1


# ---- end to end ----------------------------------------------------------------------------------------------------

SEG, H, LAT, SR = 64, 32, 8, 8000        # the tiny model of tests/test_align_gpu.py


def _model():
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.synth import make_params
    m = VAE(SEG, H, LAT).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(SEG, H, LAT, 0).items()})
    return m


def _wave():
    """Four events: a low tone, noise, the low tone again, a high tone."""
    rng = np.random.default_rng(5)
    t = np.arange(1600) / SR
    low, high = 0.6 * np.sin(2 * np.pi * 220 * t), 0.6 * np.sin(2 * np.pi * 1900 * t)
    return np.concatenate([low, 0.5 * rng.uniform(-1, 1, 1400), low[:1500], high[:1233]]).astype(np.float32)


def test_segment_py_writes_what_it_prints_and_the_split_files_concatenate_to_the_input(tmp_path, capsys):
    sys.path.insert(0, REPO)
    import segment as cli
    from rawaudiovae_kelsey_amd import data as D, structure as S
    wave = _wave()
    D.write_wav(tmp_path / "in.wav", wave, SR)
    ini = tmp_path / "m.ini"
    ini.write_text("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n" % (SR, SEG, H, LAT))
    ck = tmp_path / "ckpt"
    torch.save({"epoch": 0, "state_dict": _model().state_dict(), "optimizer": {}}, ck)
    rep = cli.main(["find", "--config", str(ini), "--checkpoint", str(ck), "--in", str(tmp_path / "in.wav"), "--hop", "16",
                    "--kernel", "12", "--gap", "8", "--delta", "0.5", "--out", str(tmp_path / "s.json"),
                    "--novelty", str(tmp_path / "nov.npy")])
    lines = capsys.readouterr().out.strip().splitlines()
    assert json.loads(lines[-1]) == rep == json.loads((tmp_path / "s.json").read_text())
    a = D.load_audio_mono(tmp_path / "in.wav", SR)
    seg = S.LatentSegmenter(_model()).segment(a, 16, 12, 0.5, 8, None, 0.5, 0.5, SR)
    assert rep["segments"] == seg.F and rep["frames"] == seg.T and rep["samples"] == a.size == wave.size
    assert rep["boundary_frames"] == seg.boundary_frames.tolist() and rep["labels"] == seg.labels.tolist()
    assert rep["boundary_samples"] == [16 * f for f in rep["boundary_frames"]]
    assert rep["boundary_seconds"] == [s / SR for s in rep["boundary_samples"]] and rep["form"] == seg.form
    assert rep["sample_offsets"] == [0] + rep["boundary_samples"] + [a.size] and len(rep["labels"]) == seg.F
    assert np.array_equal(_bits(np.load(tmp_path / "nov.npy")), _bits(_np(seg.novelty)))
    assert lines[-2] == "%d segments, boundaries at %s s, form %s" % (
        seg.F, " ".join("%.6g" % v for v in rep["boundary_seconds"]) or "-", seg.form)
    print("segment.py find: %s" % lines[-2])
    assert seg.F >= 2                                               # four events: at least one change is found
    # the oracle on the same latents finds the same offsets
    mu = _np(seg.mu)
    r = S.pick_band(seg.T, 12)
    want = O.peaks(O.novelty(AO.local_costs(mu, mu, r)[1], 12, O.taper(12, 0.5)), 8, 24, 0.5)
    assert np.array_equal(_np(seg.path), want[0]) and _np(seg.summary).tolist() == want[1].tolist()
    # split
    names = cli.main(["split", "--segments", str(tmp_path / "s.json"), "--in", str(tmp_path / "in.wav"),
                      "--out-dir", str(tmp_path / "parts")])
    assert ("wrote %d segments to %s" % (seg.F, tmp_path / "parts")) in capsys.readouterr().out
    assert len(names) == seg.F and names == sorted(names)
    parts = [D.load_audio_mono(n, SR) for n in names]
    assert [p.size for p in parts] == np.diff(rep["sample_offsets"]).tolist()
    assert np.array_equal(np.concatenate(parts), a)
    # a segments file that does not fit the wav is refused, naming the flag
    D.write_wav(tmp_path / "short.wav", wave[:-5], SR)
    with pytest.raises(ValueError, match="--segments"):
        cli.main(["split", "--segments", str(tmp_path / "s.json"), "--in", str(tmp_path / "short.wav"),
                  "--out-dir", str(tmp_path / "parts2")])
