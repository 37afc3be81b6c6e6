"""The recurrence ops on the GPU (RV_RECUR_*, csrc/recur.hip, rawaudiovae_kelsey_amd/recur.py, recur.py) against
tests/recur_oracle.py.  Everything is compared exactly: a window sum is one fp64 chain in a fixed order and the winner
is chosen by comparisons of those sums under a total order, so P's bits and I are the oracle's own.  No tolerance.

Shapes.  The kernel has one form: a workgroup takes BI = 16 rows and walks the diagonals j - i' in tiles of BJ = 256, so
what changes is how the extents fall on those two: n_rows in {m, m + 1, m + BI - 1, m + BI, m + BI + 1} (1, 2, BI, BI + 1
and BI + 2 windows) and N - m + 1 in {1, 2, BJ - 1, BJ, BJ + 1, 2 BJ + 3} columns, for m in {1, 2, 7, 32, 33, 256}: below,
at and above BI (the chains' ramp), and the longest window.  Every profile call of this file reads Dm from between NaN
guards with a row pitch of N + 3 (NaN in the padding) and writes P and I between sentinel guards."""
import functools
import json
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import align_oracle as AO  # noqa: E402
import recur_oracle as O  # noqa: E402
from guarded import guarded, guarded_flat  # noqa: E402

pytestmark = pytest.mark.gpu

BI, BJ = 16, 256                     # csrc/recur.hip: REC_BI, REC_BJ
FULL = 2 ** 31 - 1
MS = (1, 2, 7, 32, 33, 256)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()     # a copy: the cached inputs are read-only


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def _costs(n_rows, N, seed, binary=False):
    """The oracle's Dm [n_rows, N] fp32 of two seeded trajectories, computed once and left unchanged."""
    make = AO.binary_latents if binary else AO.random_latents
    dm = AO.local_costs(make(n_rows, 3, seed), make(N, 3, seed + 1000), 0)[0]
    dm.setflags(write=False)
    return dm


def _profile(dm, m, row0=0, lo=-FULL, hi=FULL, mirror=False, splits=0):
    """RV_RECUR_PROFILE on a guarded Dm of pitch N + 3 into guarded outputs -> (P, I) as numpy."""
    from rawaudiovae_kelsey_amd import recur as R
    n_rows, N = dm.shape
    T = n_rows - m + 1
    gd = guarded(n_rows, N, N + 3, torch.float32, fill=dm)
    gp, gi = guarded_flat(2 * T, torch.float32), guarded_flat(T, torch.float32)
    out = (gp.view.view(torch.float64).view(T), gi.view.view(torch.int32).view(T))
    P, I = R.profile(gd.view, m, row0, lo, hi, mirror, splits, out=out)
    assert P.data_ptr() == out[0].data_ptr() and I.data_ptr() == out[1].data_ptr()
    gp.assert_untouched("P")
    gi.assert_untouched("I")
    return _np(P).copy(), _np(I).copy()


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, got[1][:8], want[1][:8])
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (what, got[0][:4], want[0][:4])


# ---- windows and extents ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", MS)
def test_profile_equals_the_oracle_bit_for_bit_at_every_extent(m):
    n = 0
    for n_rows in (m, m + 1, m + BI - 1, m + BI, m + BI + 1):
        for J in (1, 2, BJ - 1, BJ, BJ + 1, 2 * BJ + 3):
            N = J + m - 1
            dm = _costs(n_rows, N, 7 * m + J, binary=n % 2 == 1)          # every other case: small integers, many ties
            # the admission and the split count take turns: each meets every kind of extent
            row0, lo, hi, mirror = ((0, -FULL, FULL, False), (0, 1, FULL, True), (5, 3, 40, False), (2, m, FULL, True))[n % 4]
            splits = (1, 2, 3, 0)[(n // 4) % 4]
            got = _profile(dm, m, row0, lo, hi, mirror, splits)
            _same(got, O.profile(dm, m, row0, lo, hi, mirror), (m, n_rows, N, row0, lo, hi, mirror, splits))
            n += 1
    assert n == 30


def test_the_largest_case_finds_finite_neighbours_everywhere():
    m = 256
    dm = _costs(m + BI + 1 + 300, 2 * BJ + 3 + m - 1 - 170, 99)          # 573 x 600: 318 windows against 345
    got = _profile(dm, m)
    _same(got, O.profile(dm, m), "largest")
    assert np.isfinite(got[0]).all() and (got[1] >= 0).all() and got[1].max() <= dm.shape[1] - m


# ---- splits ----------------------------------------------------------------------------------------------------------

def test_every_split_count_gives_the_same_bits():
    from rawaudiovae_kelsey_amd import recur as R
    m = 7
    dm = _costs(m + 40, 2 * BJ + 3 + m - 1, 3, binary=True)              # 3 tiles of diagonals, ties everywhere
    want = O.profile(dm, m, 0, 1, FULL, True)
    for splits in (1, 2, 3, 0, 5, 64):                                    # 5 and 64: more splits than tiles
        _same(_profile(dm, m, 0, 1, FULL, True, splits), want, splits)
    assert R.workspace_bytes(41, dm.shape[1], m, 1) == 0 and R.workspace_bytes(41, dm.shape[1], m, 5) > 0
    # a workspace with room to spare, and one split without any
    ws = torch.full((R.workspace_bytes(41, dm.shape[1], m, 3) + 512,), 7, dtype=torch.uint8, device="cuda")
    P, I = R.profile(_dev(dm), m, 0, 1, FULL, True, 3, ws=ws)
    _same((_np(P), _np(I)), want, "ws")
    P, I = R.profile(_dev(dm), m, 0, 1, FULL, True, 1, ws=torch.empty(0, dtype=torch.uint8, device="cuda"))
    _same((_np(P), _np(I)), want, "no ws")


# ---- admission -------------------------------------------------------------------------------------------------------

def test_admission_ranges():
    m = 7
    dm = _costs(m + 40, 2 * BJ + 3 + m - 1, 11)
    T = 41
    P, I = _profile(dm, m, 0, 10 ** 6, 10 ** 6 + 5, False)                # an empty range
    assert np.isposinf(P).all() and (I == -1).all()
    P, I = _profile(dm, m, 10 ** 6, -5, 5, True)                          # ... and one emptied by row0
    assert np.isposinf(P).all() and (I == -1).all()
    for row0, lo, hi, mirror in ((0, 3, 3, False), (4, 0, 0, False), (30, -20, -5, False), (30, -20, -5, True), (0, 0, FULL, True),
                                 (0, 1, FULL, True), (0, m, FULL, True), (20, m, FULL, True),
                                 (0, 100, 300, False),                    # diagonals 100 .. 300: the tile edge at 241 cuts it
                                 (0, 240, 241, False), (3, 238, 238, False), (0, BJ - BI, BJ - BI + 1, True),
                                 (0, -FULL, -FULL, False), (0, FULL, FULL, True), (0, -FULL, 0, False)):
        for splits in (1, 0):
            got = _profile(dm, m, row0, lo, hi, mirror, splits)
            _same(got, O.profile(dm, m, row0, lo, hi, mirror), (row0, lo, hi, mirror, splits))
    P, I = _profile(dm, m, 0, 3, 3, False)
    assert I.tolist() == [i + 3 for i in range(T)]                        # lo = hi: the one admitted window


# ---- slabs -----------------------------------------------------------------------------------------------------------

def test_slabs_with_their_row0_equal_the_whole_matrix_call():
    from rawaudiovae_kelsey_amd import align as A, recur as R
    Tf, L, m = 300, 8, 16
    mu = AO.random_latents(Tf, L, 17)
    dmu = _dev(mu)
    dm = _np(A.local_costs(dmu, dmu, 0))
    assert np.array_equal(_bits(dm), _bits(AO.local_costs(mu, mu, 0)[0]))
    T = Tf - m + 1
    for lo, hi, mirror in ((m, FULL, True), (20, 120, False)):
        want = O.profile(dm, m, 0, lo, hi, mirror)
        _same(_profile(dm, m, 0, lo, hi, mirror), want, "whole")
        for rows in (1, 37, 128):
            P, I = np.empty(T), np.empty(T, np.int32)
            for i0 in range(0, T, rows):
                n = min(rows, T - i0)
                P[i0:i0 + n], I[i0:i0 + n] = _profile(dm[i0:i0 + n + m - 1], m, i0, lo, hi, mirror)
            _same((P, I), want, ("slabs of", rows))
            # ... and recurrence() walking the trajectory in slabs of that many windows
            kw = dict(exclude=m) if mirror else dict(lo=lo, hi=hi)
            rec = R.recurrence(dmu, None, m, slab_rows=rows, **kw)
            _same((rec.P, rec.I.astype(np.int32)), want, ("recurrence, slabs of", rows))
    rec = R.recurrence(dmu, None, m)
    want = O.profile(dm, m, 0, m, FULL, True)
    assert (rec.m, rec.exclude, rec.mirror, rec.T) == (m, m, True, T)
    assert rec.motifs(3) == O.motifs(want[0], want[1], m, 3) and rec.discords(3) == O.discords(want[0], want[1], m, 3)
    # against another recording: the full range
    other = AO.random_latents(90, L, 18)
    rec = R.recurrence(dmu, _dev(other), m, slab_rows=100)
    _same((rec.P, rec.I.astype(np.int32)), O.profile(AO.local_costs(mu, other, 0)[0], m), "join")


# ---- ties and specials -----------------------------------------------------------------------------------------------

def test_a_periodic_trajectory_has_exact_zeros_and_the_lowest_j_wins():
    from rawaudiovae_kelsey_amd import recur as R
    p, Tf, m = 13, 330, 8
    mu = AO.random_latents(p, 5, 23)[np.arange(Tf) % p]
    rec = R.recurrence(_dev(mu), None, m)
    P, I = rec.P, rec.I
    assert (P == 0).all() and not np.signbit(P).any()
    T = Tf - m + 1
    want = [min(j for j in range(i % p, T, p) if abs(j - i) >= m) for i in range(T)]
    assert I.tolist() == want
    dm = AO.local_costs(mu, mu, 0)[0]
    for splits in (1, 2, 0):
        _same(_profile(dm, m, 0, m, FULL, True, splits), O.profile(dm, m, 0, m, FULL, True), splits)


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_nan_or_inf_cell_poisons_exactly_the_windows_that_hold_it(bad):
    m, r, c = 7, 30, 290
    clean = _costs(60, 2 * BJ + 3, 31)
    dm = clean.copy()
    dm[r, c] = bad
    want = O.profile(dm, m)
    got = _profile(dm, m)
    _same(got, want, "planted")
    W = O.window_sums(dm, m)
    hit = ~np.isfinite(W)
    assert hit.sum() == m and all(hit[r - u, c - u] for u in range(m))    # exactly the windows on its diagonal
    assert all(not hit[i, got[1][i]] for i in range(len(got[1])))
    # where the poisoned window was the winner another one wins now; every other row is untouched
    was = _profile(clean, m)
    rows = np.array([was[1][i] == i + (c - r) and r - m < i <= r for i in range(len(was[1]))])
    assert np.array_equal(_bits(got[0][~rows]), _bits(was[0][~rows])) and np.array_equal(got[1][~rows], was[1][~rows])
    # one admitted window per row (lo = hi): the rows whose window holds the cell read -1 / +inf, the others their window
    d = c - r
    P, I = _profile(dm, m, 0, d, d, False)
    _same((P, I), O.profile(dm, m, 0, d, d, False), "lo = hi")
    lost = np.array([r - m < i <= r for i in range(len(I))])
    assert np.isposinf(P[lost]).all() and (I[lost] == -1).all() and lost.sum() == m
    assert np.isfinite(P[~lost]).all() and I[~lost].tolist() == [i + d for i in np.nonzero(~lost)[0]]


# ---- capture ---------------------------------------------------------------------------------------------------------

def test_a_captured_replay_equals_the_eager_pair():
    from rawaudiovae_kelsey_amd import recur as R
    Tf, L, m = 200, 8, 16
    mu = _dev(AO.random_latents(Tf, L, 41))
    other = _dev(AO.random_latents(150, L, 42))
    for b, kw in ((None, {}), (None, dict(lo=20, hi=90)), (other, {})):
        eager = R.recurrence(mu, b, m, **kw)
        cap = R.CapturedRecurrence(Tf, Tf if b is None else 150, L, m, self_join=b is None, **kw).capture()
        first = cap.replay(torch.flip(mu, (0,)), b)                       # other operands first: the replay reads the buffers
        assert first.P.shape == (Tf - m + 1,)
        rec = cap.replay(mu, b)
        assert np.array_equal(_bits(rec.P), _bits(eager.P)) and np.array_equal(rec.I, eager.I)
        assert (rec.lo, rec.hi, rec.mirror) == (eager.lo, eager.hi, eager.mirror)
    with pytest.raises(R._lib.RvError, match="before capture"):
        R.CapturedRecurrence(Tf, Tf, L, m).replay(mu)


# ---- end to end ------------------------------------------------------------------------------------------------------

SEG, H, LAT, SR, HOP, M = 64, 96, 8, 8000, 16, 8


def _model():
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.synth import make_params
    m = VAE(SEG, H, LAT).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(SEG, H, LAT, 0).items()})
    return m


def _wave():
    """A B A C from hop-aligned blocks of noise: 40, 30, 40 and 25 hops.  The second A starts at frame 70."""
    rng = np.random.default_rng(9)
    a, b, c = (0.5 * rng.uniform(-1, 1, n * HOP) for n in (40, 30, 25))
    return np.concatenate([a, b, a, c]).astype(np.float32)


def test_find_render_and_the_command_line_on_a_b_a_c(tmp_path):
    from rawaudiovae_kelsey_amd import data as D, recur as R
    from rawaudiovae_kelsey_amd.mosaic import ola
    D.write_wav(tmp_path / "in.wav", _wave(), SR)
    wave = D.load_audio_mono(tmp_path / "in.wav", SR)                     # what the command line reads
    n = wave.size
    assert n == 135 * HOP
    model = _model()
    looper = R.LatentLooper(model)
    loop = looper.find(wave, HOP, M, 25, 100, SR)
    assert (loop.start_frame, loop.end_frame, loop.distance) == (0, 70, 0.0)
    assert (loop.frames, loop.samples, loop.start_sample, loop.end_sample) == (70, 70 * HOP, 0, 70 * HOP)
    assert (loop.start_seconds, loop.end_seconds, loop.seconds) == (0.0, 70 * HOP / SR, 70 * HOP / SR)
    mu, _, _ = looper.encode(wave, HOP)
    T = mu.shape[0]
    assert T == n // HOP - SEG // HOP + 1
    mu_np = _np(mu)
    want = O.profile(AO.local_costs(mu_np, mu_np, 0)[0], M, 0, 25, 100, False)
    rec = loop.recurrence
    assert np.array_equal(_bits(rec.P), _bits(want[0])) and np.array_equal(rec.I, want[1])
    assert O.best_loop(want[0], want[1]) == (0, 70, 0.0)
    # render: the planned length, the oracle's rows, the codec's samples
    repeats = 3
    y = looper.render(wave, loop, repeats, HOP, "hann")
    assert y.shape == (n + (repeats - 1) * 70 * HOP,)
    z = looper.loop_latents(mu, loop, repeats)
    rows = O.loop_rows(mu_np, 0, 70, M, repeats)
    assert z.shape == rows.shape == (T + (repeats - 1) * 70, LAT) and np.array_equal(_bits(_np(z)), _bits(rows))
    frames = looper.codec.decode(_dev(rows))
    win = torch.from_numpy(R.window_values(SEG, "hann")).cuda()
    full = ola(frames, HOP, (rows.shape[0] - 1) * HOP + SEG, win)
    assert torch.equal(y, full[:y.numel()])
    # before the loop's end and after the last seam: the plain resynthesis of the input
    plain = ola(looper.codec.decode(mu), HOP, (T - 1) * HOP + SEG, win)
    assert torch.equal(y[:70 * HOP], plain[:70 * HOP])
    tail = (T - 70 - M) * HOP - SEG                                       # samples that only frames after the seam cover
    assert tail > 0 and torch.equal(y[-tail:], plain[n - tail:n])
    # the command line, as processes of their own
    ini = tmp_path / "m.ini"
    ini.write_text("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n" % (SR, SEG, H, LAT))
    ck = tmp_path / "ckpt"
    torch.save({"epoch": 0, "state_dict": model.state_dict(), "optimizer": {}}, ck)
    common = ["--config", str(ini), "--checkpoint", str(ck), "--in", str(tmp_path / "in.wav"), "--hop", str(HOP),
              "--window-frames", str(M)]

    def run(*argv):
        r = subprocess.run([sys.executable, REPO + "/recur.py"] + list(argv), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.strip().splitlines()

    lines = run("loop", *common, "--min-seconds", str(25 * HOP / SR), "--max-seconds", str(100 * HOP / SR), "--repeats", "3",
                "--window", "hann", "--out", str(tmp_path / "out.wav"), "--profile", str(tmp_path / "p.npy"))
    rep = json.loads(lines[-1])
    assert (rep["start_frame"], rep["end_frame"], rep["distance"], rep["repeats"]) == (0, 70, 0.0, 3)
    assert (rep["start_seconds"], rep["end_seconds"], rep["seconds"]) == (loop.start_seconds, loop.end_seconds, loop.seconds)
    assert rep["samples"] == y.numel() and lines[-2].startswith("loop from 0 s to %.6g s" % loop.end_seconds)
    D.write_wav(tmp_path / "want.wav", _np(y), SR)
    assert np.array_equal(D.load_audio_mono(tmp_path / "out.wav", SR), D.load_audio_mono(tmp_path / "want.wav", SR))
    assert np.array_equal(_bits(np.load(tmp_path / "p.npy")), _bits(rec.P))
    print("recur.py loop: %s" % lines[-2])
    lines = run("motifs", *common, "--top", "3", "--out", str(tmp_path / "m.json"))
    rep = json.loads(lines[-1])
    assert rep == json.loads((tmp_path / "m.json").read_text())
    selfrec = looper.profile(wave, HOP, M, sampling_rate=SR)
    found = selfrec.motifs(3)
    assert found[0] == (0, 70, 0.0) and len(found) == 3
    assert [(e["frame"], e["match_frame"], e["distance"]) for e in rep["found"]] == found
    assert [e["distance_per_frame"] for e in rep["found"]] == [d / M for _, _, d in found]
    assert [(e["seconds"], e["match_seconds"]) for e in rep["found"]] == [(i * HOP / SR, j * HOP / SR) for i, j, _ in found]
    assert (rep["windows"], rep["window_frames"], rep["hop"], rep["exclude"]) == (T - M + 1, M, HOP, M)
