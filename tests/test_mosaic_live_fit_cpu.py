"""Live grain fitting without a GPU: the numpy oracle on planted cases, the header's text, the workspace query, the
host-side checks, the device-free validator and the command line's flags (tests/live_fit_oracle.py,
include/rawvae_hip.h, csrc/mosaic_live.hip, rawaudiovae_kelsey_amd/mosaic.py, mosaic.py)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import REPO  # noqa: E402
import abi_slots  # noqa: E402
import grain_fit_oracle as GF  # noqa: E402
import live_fit_oracle as LF  # noqa: E402


def _planted(rng, S, hop, n_blocks, block, d, g):
    """A one-file corpus framed at `hop` and a stream whose target frame n is g times corpus frame n moved by d samples
    (once the P zeros of the start have left the frame): x[t] = g * src[P + d + t]."""
    P = S - hop
    n = n_blocks * block
    src = rng.standard_normal(P + n + S + 64).astype(np.float32)
    src = np.concatenate([np.zeros(40, np.float32), src])       # corpus frame 0 is not the first sample: room to go back
    row_start = 40 + np.arange((src.size - 40 - S) // hop + 1, dtype=np.int64) * hop
    room = np.stack([row_start, src.size - S - row_start], 1).astype(np.int32)
    x = (np.float32(g) * src[40 + P + d:40 + P + d + n]).astype(np.float32)
    return src, row_start, room, x


@pytest.mark.parametrize("lag,calls", [(0, "pppp"), (2, "ppppd"), (3, "ppdppdd"), (5, "ppddd")])
def test_a_shifted_scaled_copy_is_found_through_a_lag(lag, calls):
    """k = 1 and the candidate of frame n is corpus frame n: whenever that row is played, at once or `lag` frames and a
    drain later, its fit is the planted shift and gain, because it is fitted to the frame that was new when it arrived"""
    rng = np.random.default_rng(lag)
    S, hop, block, d, g = 32, 8, 16, -5, 0.5
    F, first = block // hop, (S - hop) // hop                    # frames from `first` on hold no zero of the start
    src, row_start, room, x = _planted(rng, S, hop, calls.count("p"), block, d, g)
    arr = LF.arrival(calls, F)
    T = arr.size
    idx = np.arange(T, dtype=np.int32).reshape(-1, 1)           # row a of the input lines up with corpus frame a
    dist = np.zeros((T, 1), np.float32)
    mu = rng.standard_normal((row_start.size, 4)).astype(np.float32)
    next_of = np.minimum(np.arange(row_start.size) + 1, row_start.size - 1).astype(np.int32)
    r = LF.run(x, calls, block, S, hop, idx, dist, src, row_start, room, 8, 4.0, None, mu, next_of, lambda c: 0.5, lag)
    assert r["choice"].size == len(calls) * F
    fed = np.array([c == "p" for c in calls]).repeat(F)          # absolute frames that hold input, not a drain's zeros
    seen = 0
    for pos, a in enumerate(r["emit"]):
        if a < 0:
            assert r["choice"][pos] == -1
            assert (r["shift"][pos, 0], r["gain"][pos, 0], r["score"][pos, 0]) == (0, 0.0, 0.0)
            continue
        assert r["tf"][pos] == arr[a] and r["choice"][pos] == a
        # the target frame must hold input alone: past the zeros of the start, no drained block under it
        whole = arr[a] >= first and fed[arr[a] - first:arr[a] + 1].all()
        if whole:
            assert (r["shift"][pos, 0], r["gain"][pos, 0]) == (d, np.float32(g)), (pos, a)
            seen += 1
    assert seen >= 1
    if lag:
        assert np.all(r["choice"][:min(lag, T)] == -1)           # the warm-up plays nothing and fits nothing
    if calls == "ppdppdd":
        assert (r["emit"] >= 0).sum() == T and (np.arange(len(r["emit"])) - r["tf"])[r["emit"] >= 0].max() > lag


def test_without_selection_every_candidate_is_fitted_and_a_missing_one_gets_zeros():
    rng = np.random.default_rng(7)
    S, hop, block, d, g = 32, 8, 16, 3, 2.0
    src, row_start, room, x = _planted(rng, S, hop, 4, block, d, g)
    T = 4 * block // hop
    idx = np.stack([np.arange(T), np.full(T, -1), np.arange(T) + 1], 1).astype(np.int32)
    r = LF.run(x, "pppp", block, S, hop, idx, np.zeros((T, 3), np.float32), src, row_start, room, 8, 4.0)
    assert r["shift"].shape == (T, 3) and np.all(r["choice"] == -1)
    assert np.all(r["shift"][:, 1] == 0) and np.all(r["gain"][:, 1] == 0) and np.all(r["score"][:, 1] == 0)
    assert np.all(r["shift"][3:, 0] == d) and np.all(r["gain"][3:, 0] == np.float32(g))
    assert np.all(r["shift"][3:, 2] == d - hop)                  # the next corpus frame lines up one hop earlier
    # the audio is the overlap-add of the mean of the fitted grains: frame by frame grain_fit_oracle's gather
    frames = GF.gather(src, row_start, idx, r["shift"], r["gain"], S)
    import mosaic_oracle as O
    assert np.array_equal(r["y"], O.ola(frames, hop, T * hop, None))


@pytest.mark.parametrize("S,hop,block", [(64, 16, 16), (64, 16, 32), (64, 16, 128), (64, 64, 64), (1280, 320, 320)])
def test_the_headers_ring_layout_holds_every_target_frame_a_committed_row_stands_for(S, hop, block):
    """The state the header describes, stepped on the host: the block written at ring[(count hop + i) mod C] with
    C = P + 2 D hop + block, pending rows stamped with their arrival frame, a committed row's frame read back from
    ring[(n hop - P + m) mod C].  Every frame read equals the oracle's target frame and no row is older than 2 D."""
    import live_lag_oracle as G
    rng = np.random.default_rng(S + block)
    F, P = block // hop, S - hop
    oldest = {}
    for lag, calls in ((0, "pppppp"), (1, "ppppdd"), (3, "ppdppdd"), (3, "pdpdpdpdpddd"), (5, "ppdddd"),
                       (8, "ppppdppdpppddddddddd"), (2, "pdddpppdd")):
        C, R = P + 2 * lag * hop + block, lag + 1
        x = rng.standard_normal(calls.count("p") * block).astype(np.float32)
        frames = LF.target_frames(LF.timeline(x, calls, block), S, hop)
        arr, emit = LF.arrival(calls, F), G.schedule(calls, F, lag)[1]
        ring, stamp = np.zeros(C, np.float32), np.zeros(R, np.int64)
        count = head = pending = b = pos = 0
        for c in calls:
            xb = x[b * block:(b + 1) * block] if c == "p" else np.zeros(block, np.float32)
            b += c == "p"
            ring[(count * hop + np.arange(block)) % C] = xb
            for f in range(F):
                if c == "p":
                    stamp[(head + pending) % R] = count + f
                    pending += 1
                if (pending == R) if c == "p" else (pending > 0):
                    n = stamp[head]
                    head, pending = (head + 1) % R, pending - 1
                    assert emit[pos] >= 0 and n == arr[emit[pos]]
                    assert 0 <= count + f - n <= 2 * lag
                    oldest[lag] = max(oldest.get(lag, 0), count + f - n)
                    assert np.array_equal(ring[(n * hop - P + np.arange(S)) % C], frames[n]), (lag, calls, pos)
                else:
                    assert emit[pos] < 0
                pos += 1
            count += F
    if F == 2:
        assert oldest[3] == 5 and oldest[8] > 8                  # a row that waited through a drain is older than D


def _header():
    with open(os.path.join(REPO, "include", "rawvae_hip.h")) as f:
        return f.read()


def test_header_keeps_its_ops_and_fields_and_states_the_fields_of_the_live_fit():
    from rawaudiovae_kelsey_amd import _lib
    text = _header()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert len(re.findall(r"#define RV_MOSAIC_[A-Z_]+ \d+", code)) == 14
    assert len(abi_slots.check_layout()) == 37 and C.sizeof(_lib.MosaicDesc) == 37 * 8
    m = re.search(r"Live grain fitting.*?\n \*\n", text, flags=re.S)
    assert m, "the header has no 'Live grain fitting' paragraph"
    para = m.group(0)
    for word in ("fit_radius = R", "gain_max > 0", "shift [M, kf]", "gain [M, kf]", "score [M, kf]", "[3 N]", "room [N, 2]",
                 "LIVE_WORKSPACE", "LIVE_RESET", "LIVE_DRAIN", "RV_LIVE_DECODE", "TARGET RING", "P + 2 D hop + block"):
        assert word in para, word


def _live_desc(fit=0, gain_max=0.0, lag=0, weight=True, mode=0, n_streams=1, block=256, hop=256, S=1024, L=256,
               N=1240000, k=4, **over):
    from rawaudiovae_kelsey_amd import _lib
    sd = _lib.StreamDesc(S=S, H=2048, L=L, n_streams=n_streams, block=block, hop=hop)
    f = dict(k=k, N=N, L=L, live=C.pointer(sd), rows=lag, weight=0x1000 if weight else None, width=fit, lam=gain_max,
             mode=mode)
    f.update(over)
    return _lib.MosaicDesc(**f), sd


def _ws(**kw):
    from rawaudiovae_kelsey_amd import _lib
    d, sd = _live_desc(**kw)
    _lib.lib().rv_mosaic(_lib.MOSAIC_LIVE_WORKSPACE, C.byref(d), None)   # pointers are not read: no device is touched
    return d.ws_bytes


def test_live_workspace_is_unchanged_without_a_fit_and_grows_by_the_ring_with_one():
    """the byte counts without a fit are the ones the library gave before it knew a fit"""
    up = lambda n: (n + 255) // 256 * 256
    assert _ws() == _ws(fit=0, gain_max=0.0) == 32512
    assert _ws(lag=8) == 34048 and _ws(lag=64, n_streams=8, block=1024, k=16) == 2618880
    assert _ws(N=1000, n_streams=3, block=512, k=1, weight=False) == 6656
    assert _ws(N=1000, n_streams=5, block=4096) == 92416
    S, hop = 1024, 256
    for lag, block, ns in ((0, 256, 1), (0, 1024, 3), (8, 256, 1), (64, 2048, 2)):
        kw = dict(lag=lag, block=block, n_streams=ns, N=1000, k=4)
        plain = _ws(**kw)
        ring = up(ns * (S - hop + 2 * lag * hop + block) * 4)
        extra = 0 if lag == 0 else up(ns * (lag + 1) * 8) + up(ns * (block // hop) * 8)
        for fit, g in ((5, 0.0), (0, 4.0), (1024, 2.0)):
            assert _ws(fit=fit, gain_max=g, **kw) == plain + ring + extra, (lag, block, ns, fit, g)
        assert _ws(fit=5, weight=(lag > 0), **kw) == _ws(fit=5, **kw)


def test_live_ops_refuse_a_bad_fit_by_name_before_any_launch():
    """every case fails a host-side check: the pointers are never read and no device is touched"""
    from rawaudiovae_kelsey_amd import _lib
    L = _lib.lib()
    for bad in (1025, -1, 1 << 40):
        with pytest.raises(_lib.RvError, match=r"LIVE_WORKSPACE\): fit_radius="):
            _ws(fit=bad)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(_lib.RvError, match=r"LIVE_WORKSPACE\): gain_max="):
            _ws(gain_max=bad)
        with pytest.raises(_lib.RvError, match="gain_max="):
            _ws(fit=8, gain_max=bad)
    for kw in (dict(fit=8), dict(gain_max=2.0), dict(fit=8, gain_max=2.0)):
        with pytest.raises(_lib.RvError, match=r"LIVE_WORKSPACE\): a fit .*fit_radius=.*gain_max=.*RV_LIVE_GRAINS"):
            _ws(mode=1, **kw)
    assert _ws(mode=1) == _ws()
    # LIVE, LIVE_DRAIN and LIVE_RESET read the two fields as LIVE_WORKSPACE does
    for op, name in ((_lib.MOSAIC_LIVE, "LIVE"), (_lib.MOSAIC_LIVE_DRAIN, "LIVE_DRAIN"), (_lib.MOSAIC_LIVE_RESET, "LIVE_RESET")):
        for kw, what in ((dict(fit=1025), "fit_radius=1025"), (dict(gain_max=float("nan")), "gain_max="),
                         (dict(fit=8, mode=1), "RV_LIVE_GRAINS")):
            d, sd = _live_desc(lag=2, **kw)
            with pytest.raises(_lib.RvError, match=r"\(%s\): .*%s" % (name, what)):
                L.rv_mosaic(op, C.byref(d), None)
    # a null table or output, and a workspace that is too small, of a call that would otherwise launch
    ok = dict(fit=8, gain_max=2.0, lag=2, N=1000, idx=0x1000, dist=0x2000, c=0x3000, src=0x4000, src_len=1 << 20,
              row_start=0x5000, next_of=0x6000, choice=0x7000, slot=0x8000, trans=0x9000, cost=0xa000, ws=0x10000)
    need = _ws(fit=8, gain_max=2.0, lag=2, N=1000)
    for op, name in ((_lib.MOSAIC_LIVE, "LIVE"), (_lib.MOSAIC_LIVE_DRAIN, "LIVE_DRAIN")):
        for over, what in ((dict(next_of=None), "next_of"), (dict(slot=None), "shift is null"),
                           (dict(trans=None), "gain is null"), (dict(cost=None), "score is null"),
                           (dict(ws_bytes=need - 256), "workspace of %d bytes" % (need - 256))):
            d, sd = _live_desc(**dict(dict(ok, ws_bytes=need), **over))
            with pytest.raises(_lib.RvError, match=r"\(%s\): .*%s" % (name, what)):
                L.rv_mosaic(op, C.byref(d), None)
    d, sd = _live_desc(**dict(ok, ws_bytes=need - 256))
    with pytest.raises(_lib.RvError, match=r"LIVE_RESET\): workspace of %d bytes, %d needed" % (need - 256, need)):
        L.rv_mosaic(_lib.MOSAIC_LIVE_RESET, C.byref(d), None)


def test_validator_names_fit_and_gain_max():
    from rawaudiovae_kelsey_amd.mosaic import check_live_args
    ok = dict(segment_length=64, index_step=16, n_corpus=100, n_streams=2, block=32, hop=16, k=4, mode="grains",
              window="hann", continuity=0.5)
    want = (16, 48, 2, 1)
    assert check_live_args(**ok) == check_live_args(**dict(ok, fit=0, gain_max=0.0)) == want
    assert check_live_args(**dict(ok, fit=1024, gain_max=2.5, lag=3)) == want
    assert check_live_args(**dict(ok, mode="decode", fit=0, gain_max=0)) == want
    for bad in (-1, 1025, 1.5, "3", None, True):
        with pytest.raises(ValueError, match="fit"):
            check_live_args(**dict(ok, fit=bad))
    for bad in (-0.5, float("inf"), float("nan"), "x", None):
        with pytest.raises(ValueError, match="gain_max"):
            check_live_args(**dict(ok, gain_max=bad))
    with pytest.raises(ValueError, match="fit=8"):
        check_live_args(**dict(ok, mode="decode", fit=8))
    with pytest.raises(ValueError, match="gain_max=2"):
        check_live_args(**dict(ok, mode="decode", gain_max=2.0))


def test_cli_live_fit_flags(tmp_path):
    sys.path.insert(0, REPO)
    import mosaic as cli
    from rawaudiovae_kelsey_amd import data as D
    assert "--live-fit" in cli.__doc__ and "--live-gain-max" in cli.__doc__
    with open(os.path.join(REPO, "README.md")) as f:
        assert "--live-fit" in f.read()
    corpus = tmp_path / "corpus"
    corpus.mkdir()
    D.write_wav(corpus / "a.wav", np.zeros(640, np.float32), 8000)
    base = ["--config", "none.ini", "--checkpoint", "none.pt", "--target", "t.wav", "--out", "o.wav", "--corpus", str(corpus)]
    live = ["--live-block", "64"]
    for extra in (["--live-fit", "8"], live + ["--live-fit", "8", "--mode", "decode"], live + ["--live-fit", "1025"],
                  live + ["--live-fit", "-1"], live + ["--live-fit", "x"], live + ["--live-fit", "1.5"]):
        with pytest.raises(ValueError, match="^--live-fit"):
            cli.parse_args(base + extra)
    for extra in (["--live-gain-max", "2"], live + ["--live-gain-max", "2", "--mode", "decode"],
                  live + ["--live-gain-max", "-1"], live + ["--live-gain-max", "inf"], live + ["--live-gain-max", "nan"],
                  live + ["--live-gain-max", "x"]):
        with pytest.raises(ValueError, match="^--live-gain-max"):
            cli.parse_args(base + extra)
    # the offline flags still refuse the live path, by their own name first, and now say where to go
    with pytest.raises(ValueError, match="^--fit 8.*--live-fit"):
        cli.parse_args(base + ["--fit", "8", "--live-block", "64"])
    with pytest.raises(ValueError, match="^--gain-max 2.*--live-gain-max"):
        cli.parse_args(base + ["--gain-max", "2", "--live-block", "64"])
    a = cli.parse_args(base + live)
    assert a.live_fit == 0 and a.live_gain_max == 0.0 and not a.live_fitted and not a.fitted
    a = cli.parse_args(base + live + ["--live-fit", "16", "--live-gain-max", "4"])
    assert a.live_fit == 16 and a.live_gain_max == 4.0 and a.live_fitted and not a.fitted and a.fit == 0
    a = cli.parse_args(base + live + ["--live-gain-max", "0.5", "--continuity", "1", "--lag", "3"])
    assert a.live_fit == 0 and a.live_gain_max == 0.5 and a.live_fitted
    assert not cli.parse_args(base).live_fitted
    # the layout of --matches for live fits is offline's: per candidate behind its distance, or behind the slot
    path = tmp_path / "m.csv"
    fits = (np.array([[3, -2], [0, 0]], np.int32), np.array([[0.25, 1.0], [0.0, 0.0]], np.float32))
    cli.write_matches(path, [[("a.wav", 0), ("a.wav", 64)], [(None, -1), (None, -1)]], [[0.5, 1.5], [np.inf, np.inf]],
                      None, fits)
    assert path.read_text().strip().split("\n") == ["a.wav,0,0.5,3,0.25,a.wav,64,1.5,-2,1.0", ",-1,inf,0,0.0,,-1,inf,0,0.0"]
    cli.write_matches(path, [[("a.wav", 0), ("a.wav", 64)]], [[0.5, 1.5]], [1],
                      (np.array([[-7]], np.int32), np.array([[2.0]], np.float32)))
    assert path.read_text().strip() == "a.wav,0,0.5,a.wav,64,1.5,1,-7,2.0"
