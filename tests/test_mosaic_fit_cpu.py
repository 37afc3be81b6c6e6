"""Grain fitting without a GPU: the numpy oracle of the rule on planted cases, the room table, the header's two ops and
their host-side error returns, and the command line's flags (tests/grain_fit_oracle.py, include/rawvae_hip.h,
rawaudiovae_kelsey_amd/mosaic.py, mosaic.py)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import grain_fit_oracle as F  # noqa: E402
import mosaic_oracle as O  # noqa: E402


def test_header_and_lib_agree_on_the_two_ops():
    from rawaudiovae_kelsey_amd import _lib
    with open(os.path.join(REPO, "include", "rawvae_hip.h")) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert re.search(r"#define RV_GRAIN_FIT 14\b", src) and re.search(r"#define RV_GRAIN_GATHER 15\b", src)
    assert _lib.GRAIN_FIT == 14 and _lib.GRAIN_GATHER == 15
    assert len(abi_slots.check_layout()) == 37 and C.sizeof(_lib.MosaicDesc) == 37 * 8


def test_fma_emulation_is_the_fused_operation():
    """against exact rational arithmetic: fmaf(a, b, c) is a * b + c rounded once"""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.standard_normal(400).astype(np.float32)
    b = rng.standard_normal(400).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32)      # heavy cancellation
    c[::2] = rng.standard_normal(200).astype(np.float32)
    # midpoints: a * b = 2^-24 (half an ulp of 1) + something tiny, c = 1
    a[:4] = np.float32(2.0 ** -12)
    b[:4] = [np.float32(2.0 ** -12), np.nextafter(np.float32(2.0 ** -12), np.float32(1)), np.float32(2.0 ** -12), 0]
    c[:4] = [1, 1, np.nextafter(np.float32(1), np.float32(2)), 1]
    got = F._fma(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        err = abs(Fraction(float(g)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):   # a tie: to even
            assert int(np.float32(g).view(np.int32)) % 2 == 0
    d = rng.standard_normal(100).astype(np.float32)
    acc = rng.standard_normal(100).astype(np.float32)
    assert np.array_equal(F._fma(d, d, acc), O._fma_sq(d, acc))


def _smoothed_noise(n, seed):
    w = np.random.default_rng(seed).standard_normal(n + 4)
    return np.convolve(w, np.ones(5) / 5, mode="valid").astype(np.float32)


def test_the_oracle_recovers_a_planted_shift_and_gain():
    S, hop, R = 64, 16, 24
    wave = _smoothed_noise(768, 1)
    room = F.shift_room([768], S, hop)
    row_start = np.arange(room.shape[0], dtype=np.int64) * hop
    target = np.zeros(768, np.float32)
    target[:768 - 13] = np.float32(0.5) * wave[13:]
    T = room.shape[0]
    idx = np.arange(T)[:, None]
    shift, gain, score = F.fit(target, hop, S, idx, wave, row_start, room, R, 1e3)
    free = room[:, 1] >= 13
    assert free.sum() == 44
    assert np.all(shift[free, 0] == 13)
    assert np.all(np.abs(gain[free, 0] - 0.5) < 1e-6)
    assert np.all(score[free, 0] > 0)
    assert np.all(shift[~free, 0] <= room[~free, 1])
    only, one, _ = F.fit(target, hop, S, idx, wave, row_start, room, R, 0.0)     # shift only
    assert np.array_equal(only, shift) and np.all(one == 1)
    y = F.gather(wave, row_start, idx, shift, gain, S)
    x = np.stack([target[t * hop:t * hop + S] for t in range(T)])
    assert np.abs(y[free] - x[free]).max() < 1e-6


def test_the_oracle_breaks_a_periodic_tie_towards_the_smaller_then_the_negative_shift():
    S, R = 32, 12
    pattern = np.array([3, -1, 4, 1, -5, 9, 2, -6], np.float32)                   # small integers: every sum is exact
    wave = np.tile(pattern, 16)                                                   # 128 samples, period 8
    row_start = np.array([0, 48], np.int64)
    room = np.array([[0, 96], [48, 48]], np.int32)
    target = wave[48 + 5:48 + 5 + S].copy()                                       # frame 1, 5 samples off the grid
    shift, gain, score = F.fit(target, S, S, np.array([[1, 0]]), wave, row_start, room, R, 4.0)
    assert shift[0, 0] == -3 and gain[0, 0] == 1 and score[0, 0] == float((target.astype(np.float64) ** 2).sum())
    assert shift[0, 1] == 5 and gain[0, 1] == 1                                   # no room backwards: +5 is the nearest
    wave4 = np.tile(pattern[:4], 32)                                              # period 4, queried 2 off: -2 and +2 tie
    shift, _, _ = F.fit(wave4[48 + 2:48 + 2 + S], S, S, np.array([[1]]), wave4, row_start, room, R, 4.0)
    assert shift[0, 0] == -2
    zeros, gz, sz = F.fit(np.zeros(S, np.float32), S, S, np.array([[1, -1, 2]]), wave, row_start, room, R, 4.0)
    assert np.all(zeros == 0) and np.all(gz == 0) and np.all(sz == 0)             # nothing scores: shift 0, gain 0
    _, g1, _ = F.fit(np.zeros(S, np.float32), S, S, np.array([[1, -1, 2]]), wave, row_start, room, R, 0.0)
    assert g1.tolist() == [[1, 0, 0]]                                             # shift only; no candidate: gain 0


@pytest.mark.parametrize("hop", [None, 16, 64])
def test_shift_room_keeps_every_permitted_grain_inside_its_file(hop):
    from rawaudiovae_kelsey_amd.mosaic import frame_tables, shift_room
    S, lengths = 64, (700, 1000, 513, 1290)
    before = frame_tables(lengths, S, hop)
    room = shift_room(lengths, S, hop)
    after = frame_tables(lengths, S, hop)
    assert len(after) == 5 and all(np.array_equal(a, b) for a, b in zip(before, after))
    n_frames, padded, row_start, file_of, offset_of = after
    assert room.dtype == np.int32 and room.shape == (row_start.size, 2) and np.all(room >= 0)
    assert np.array_equal(room, F.shift_room(lengths, S, hop))
    base = np.concatenate([[0], np.cumsum(padded)[:-1]])
    first, last = base[file_of], base[file_of] + padded[file_of]
    assert np.all(row_start - room[:, 0] >= first) and np.all(row_start + room[:, 1] + S <= last)
    assert np.all(row_start - (room[:, 0] + 1) < first) and np.all(row_start + room[:, 1] + 1 + S > last)
    starts = np.concatenate([[0], np.cumsum(n_frames)[:-1]])
    assert np.all(room[starts, 0] == 0) and np.all(room[starts + n_frames - 1, 1] == 0)


def _fit_desc(**over):
    from rawaudiovae_kelsey_amd import _lib
    f = dict(T=4, k=2, idx=0x1000, frames=0x2000, n_out=4096, hop=16, S=64, src=0x3000, src_len=8192, row_start=0x4000,
             n_rows=100, next_of=0x5000, width=24, lam=2.0, slot=0x6000, trans=0x7000, cost=0x8000)
    f.update(over)
    return _lib.MosaicDesc(**f)


def _gather_desc(**over):
    from rawaudiovae_kelsey_amd import _lib
    f = dict(T=4, k=2, idx=0x1000, src=0x3000, src_len=8192, row_start=0x4000, n_rows=100, width=64, out=0x9000, ldo=64,
             slot=0x6000, trans=0x7000)
    f.update(over)
    return _lib.MosaicDesc(**f)


def test_bad_arguments_are_refused_by_name_before_any_launch():
    """every case fails a host-side check: the pointers are never read and no device is touched"""
    from rawaudiovae_kelsey_amd import _lib
    L = _lib.lib()
    bad_fit = [(dict(width=1025), "fit_radius=1025"), (dict(width=-1), "fit_radius=-1"), (dict(T=0), "T="), (dict(k=0), "k="),
               (dict(k=17), "k="), (dict(idx=None), "idx"), (dict(frames=None), "frames"), (dict(src=None), "src"),
               (dict(row_start=None), "row_start"), (dict(next_of=None), "room"), (dict(slot=None), "shift"),
               (dict(trans=None), "gain"), (dict(cost=None), "score"), (dict(n_out=3 * 16 + 63), "n_out"),
               (dict(T=1, n_out=63), "n_out"), (dict(lam=-1.0), "gain_max"), (dict(lam=float("inf")), "gain_max"),
               (dict(lam=float("nan")), "gain_max"), (dict(S=0), "S="), (dict(hop=0), "hop="), (dict(n_rows=0), "n_rows"),
               (dict(src_len=63), "src_len")]
    for over, name in bad_fit:
        with pytest.raises(_lib.RvError, match=r"GRAIN_FIT\): .*" + name):
            L.rv_mosaic(_lib.GRAIN_FIT, C.byref(_fit_desc(**over)), None)
    bad_gather = [(dict(T=0), "T="), (dict(k=17), "k="), (dict(idx=None), "idx"), (dict(src=None), "src"),
                  (dict(out=None), "out"), (dict(slot=None), "shift"), (dict(trans=None), "gain"),
                  (dict(width=0), "width"), (dict(ldo=63), "ldo"), (dict(src_len=63), "src_len")]
    for over, name in bad_gather:
        with pytest.raises(_lib.RvError, match=r"GRAIN_GATHER\): .*" + name):
            L.rv_mosaic(_lib.GRAIN_GATHER, C.byref(_gather_desc(**over)), None)


def test_python_validators_name_the_argument():
    from rawaudiovae_kelsey_amd.mosaic import FIT_MAX, check_fit
    assert FIT_MAX == 1024
    assert check_fit(0, 0) == (0, 0.0) and check_fit(1024, 2.5) == (1024, 2.5) and check_fit(np.int64(7), 0.0) == (7, 0.0)
    for bad in (-1, 1025, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="fit"):
            check_fit(bad, 0.0)
    for bad in (-0.5, float("inf"), float("nan"), "x", None):
        with pytest.raises(ValueError, match="gain_max"):
            check_fit(0, bad)


def test_cli_fit_flags(tmp_path):
    sys.path.insert(0, REPO)
    import mosaic as cli
    from rawaudiovae_kelsey_amd import data as D
    assert "--fit" in cli.__doc__ and "--gain-max" in cli.__doc__
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    D.write_wav(corpus / "a.wav", np.zeros(640, np.float32), 8000)
    base = ["--config", "none.ini", "--checkpoint", "none.pt", "--target", "t.wav", "--out", "o.wav", "--corpus", str(corpus)]
    for extra in (["--fit", "8", "--live-block", "64"], ["--fit", "8", "--mode", "decode"], ["--fit", "-1"],
                  ["--fit", "1025"], ["--fit", "x"], ["--fit", "1.5"]):
        with pytest.raises(ValueError, match="--fit"):
            cli.parse_args(base + extra)
    for extra in (["--gain-max", "2", "--live-block", "64"], ["--gain-max", "2", "--mode", "decode"], ["--gain-max", "-1"],
                  ["--gain-max", "inf"], ["--gain-max", "nan"], ["--gain-max", "x"]):
        with pytest.raises(ValueError, match="--gain-max"):
            cli.parse_args(base + extra)
    a = cli.parse_args(base)
    assert a.fit == 0 and a.gain_max == 0.0 and not a.fitted
    a = cli.parse_args(base + ["--fit", "16", "--gain-max", "4"])
    assert a.fit == 16 and a.gain_max == 4.0 and a.fitted
    a = cli.parse_args(base + ["--gain-max", "0.5", "--continuity", "1"])
    assert a.fit == 0 and a.gain_max == 0.5 and a.fitted
    path = tmp_path / "m.csv"
    cli.write_matches(path, [[("a.wav", 0), ("a.wav", 64)]], [[0.5, 1.5]], None,
                      (np.array([[3, -2]]), np.array([[0.25, 1.0]], np.float32)))
    assert path.read_text().strip() == "a.wav,0,0.5,3,0.25,a.wav,64,1.5,-2,1.0"
    cli.write_matches(path, [[("a.wav", 0), ("a.wav", 64)]], [[0.5, 1.5]], [1], (np.array([[-7]]), np.array([[2.0]])))
    assert path.read_text().strip() == "a.wav,0,0.5,a.wav,64,1.5,1,-7,2.0"
    cli.write_matches(path, [[("a.wav", 0)]], [[0.5]], [0])
    assert path.read_text().strip() == "a.wav,0,0.5,0"
