#!/usr/bin/env python3
"""Time the mosaicing kNN search (rv_mosaic RV_MOSAIC_KNN, csrc/mosaic_knn.hip) and one whole LatentIndex.mosaic() call.

    python tools/mosaic_bench.py [--reps 5] [--path] [--out build/mosaic_bench.json]
    python tools/mosaic_bench.py --live [--reps 30] [--summary profiles/mosaic_live_summary.txt]
    python tools/mosaic_bench.py --live --lag [--reps 30] [--summary profiles/mosaic_live_lag_summary.txt]
    python tools/mosaic_bench.py --fit [--reps 5] [--summary profiles/mosaic_fit_summary.txt]
    python tools/mosaic_bench.py --live --fit [--reps 30] [--summary profiles/mosaic_live_fit_summary.txt]

Search shapes (T, N, L, k): one minute of target at hop 128 (20 700 frames) and one second (344 frames), both against
one hour of corpus at hop 128 (1.24 M frames), latent_dim 256, k = 4.  Per shape: device time (events around `reps`
back-to-back calls after a warm-up), the workgroups of the search launch, and the rate in distance terms/s, T N L per
call.  A term is one subtract and one fma: against the 157.3 TFLOP/s fp32 spec of the MI355X (78.6 T fma/s with packed
math) the bound is about 39 T terms/s packed and 20 T terms/s unpacked -- spec-sheet arithmetic, not a measurement.

--path: the three steps of the unit selection (mosaic.best_path) for one minute of target (T = 20 700, N = 1.24 M,
L = 256, k = 16) beside the search of the same shape: the transition costs (RV_MOSAIC_TRANSITION, judged against HBM
rate: 2 k L 4 bytes of gathered latent rows per target row), the forward pass and the backtrack (one wave each; the
time per row is the length of the dependent chain).  The candidates are the search's own, on random data.

--live (alone: nothing else is timed): the live path, every figure from HIP events around `reps` replays of a captured
graph after a warm-up.  (1) The few-query search (RV_MOSAIC_KNN_SMALL) against RV_MOSAIC_KNN, alternating in one
process, for T in {1, 4, 16, 64}, N in {124 000, 1 240 000}, L = 256, k in {4, 16}; the best of three rounds each, and
the corpus bytes (N L 4) per second of the few-query kernel.  (2) One StreamingMosaic.replay() per block for
n_streams x hop x block in {1x128x128, 1x256x256, 1x256x1024, 16x256x1024}, grains and decode, k = 4, continuity 0.5,
against corpora of 6 872, 124 000 and 1 240 000 frames (random audio in 8 files, indexed at hop 128 by a
VAE(1024, 2048, 256) with random weights), beside the block's duration at 44.1 kHz.

--live --lag (nothing else is timed): the live path's unit selection with look-ahead.  One StreamingMosaic.replay()
per block, grains, continuity 0.5, for lag 0 (k_live_select, the greedy rule) and lag in {1, 4, 16, 64} (k_live_lag),
alternating in one process, the best of three rounds each, every window full before the clock starts; k in {4, 16},
N in {124 000, 1 240 000}, n_streams x hop x block in {1x128x128, 16x256x1024}.  Beside each time: the block's duration
at 44.1 kHz, and for lag > 0 the time over lag 0 per frame and window row (the length of the forward pass's chain).

--fit (alone: nothing else is timed): grain fitting (RV_GRAIN_FIT, csrc/grain.hip) at the search's minute shape -- one
minute of target at hop 128 (T = 20 700), k = 4, S = 1024, R = 256, the candidates the search's own over one hour of
corpus audio (1.24 M frames at hop 128 in 8 files, random samples) -- beside the search and the fitted gather
(RV_GRAIN_GATHER), alternating in one process, HIP events around `reps` calls, the best of three rounds each.  The rate
is in fmas/s, 2 T k (2R + 1) S per call (the c and the e chain), against 78.6 T fma/s (the fp32 vector spec, unpacked
fmas: 39.3 T/s).

--live --fit (nothing else is timed): live grain fitting, StreamingMosaic(fit=R, gain_max=4).  One replay() per block,
grains, k = 4, hop = block = 256, S = 1024 (one frame per block and stream), n_streams in {1, 8}, against the 124 000
frame corpus of the --live --lag table; once at continuity 0 (k fits per frame) and once at continuity 0.5 with lag 8
(one fit per frame); R in {0 (the gain alone), 64, 256, 1024}.  Each fitted replay alternates in one process with the
unfitted replay of the same configuration, the best of three rounds each, every window full before the clock starts.
Beside each time: the time over the unfitted replay (the ring update, the fit and the fitted gather in place of the
plain one: with a handful of workgroups per block this is the latency of one workgroup's 2R + 1 shifts, not a
throughput) and the block's duration at 44.1 kHz.

mosaic(): a VAE(1024, 2048, 256) with random weights, a 40 s corpus in 8 files and a 5 s target at hop 256, k = 4,
grains and decode, wall time of the call including the target's encoder pass (the corpus is indexed beforehand).
"""
import argparse
import json
import os
import platform
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd import mosaic as M  # noqa: E402

PACKED_TERMS, UNPACKED_TERMS = 157.3e12 / 2 / 2, 157.3e12 / 2 / 4
SHAPES = (("minute_target", 20700, 1240000, 256, 4), ("second_target", 344, 1240000, 256, 4))


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def bench_search(name, T, N, L, k, reps):
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(T, L, device="cuda", generator=g)
    c = torch.randn(N, L, device="cuda", generator=g)
    ms = timed(lambda: M.knn_topk(q, c, k), reps)
    splits = max(1, M.knn_workspace_bytes(T, N, L, k) // (T * k * 8))
    terms = float(T) * N * L / (ms * 1e-3)
    return dict(shape=name, T=T, N=N, L=L, k=k, ms=round(ms, 3), splits=int(splits),
                workgroups=int(-(-T // 128) * splits), terms_per_s=terms,
                of_packed_bound=round(terms / PACKED_TERMS, 4), of_unpacked_bound=round(terms / UNPACKED_TERMS, 4))


def bench_path(T, N, L, k, reps):
    from rawaudiovae_kelsey_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(T, L, device="cuda", generator=g)
    c = torch.randn(N, L, device="cuda", generator=g)
    search_ms = timed(lambda: M.knn_topk(q, c, k), reps)
    idx, dist = M.knn_topk(q, c, k)
    next_of = torch.from_numpy(M.successor_table(torch.arange(N).div(20000, rounding_mode="floor").numpy())).cuda()
    trans = torch.empty((T, k, k), dtype=torch.float32, device="cuda")
    trans_ms = timed(lambda: M.transition_costs(c, idx, next_of, out=trans), reps)
    nbytes = M.path_workspace_bytes(T, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    slot = torch.empty(T, dtype=torch.int32, device="cuda")
    choice = torch.empty(T, dtype=torch.int32, device="cuda")
    cost = torch.empty(2, dtype=torch.float64, device="cuda")
    common = dict(T=T, k=k, idx=M.ptr(idx), dist=M.ptr(dist), ws=M.ptr(ws), ws_bytes=nbytes)
    fwd_ms = timed(lambda: M._call(_lib.MOSAIC_PATH_FORWARD, row0=0, rows=T, trans=M.ptr(trans), lam=1.0, **common),
                   reps)
    back_ms = timed(lambda: M._call(_lib.MOSAIC_PATH_BACKTRACK, slot=M.ptr(slot), choice=M.ptr(choice),
                                    cost=M.ptr(cost), **common), reps)
    whole_ms = timed(lambda: M.best_path(idx, dist, c, next_of, 1.0), reps)
    gathered = 2.0 * k * L * 4 * T + 4.0 * k * k * T
    return dict(T=T, N=N, L=L, k=k, search_ms=round(search_ms, 3), transition_ms=round(trans_ms, 4),
                transition_gb_per_s=round(gathered / (trans_ms * 1e-3) / 1e9, 1), forward_ms=round(fwd_ms, 4),
                forward_ns_per_row=round(fwd_ms * 1e6 / T, 1), backtrack_ms=round(back_ms, 4),
                backtrack_ns_per_row=round(back_ms * 1e6 / T, 1), best_path_ms=round(whole_ms, 4),
                continuing=float((choice[1:] == next_of[choice[:-1].clamp(min=0).long()]).float().mean()),
                cost=[float(v) for v in cost.cpu()])


def bench_mosaic(reps):
    from rawvae.model import VAE
    torch.manual_seed(0)
    m = VAE(1024, 2048, 256).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    sr = 44100
    index = M.LatentIndex(m, hop=256)
    for i in range(8):
        index.add(torch.randn(5 * sr, device="cuda", generator=g) * 0.3, "c%d" % i)
    target = torch.randn(5 * sr, device="cuda", generator=g) * 0.3
    out = {}
    for mode in ("grains", "decode"):
        index.mosaic(target, k=4, mode=mode, window="hann")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            index.mosaic(target, k=4, mode=mode, window="hann")
        torch.cuda.synchronize()
        out[mode + "_ms"] = round((time.perf_counter() - t0) * 1e3 / reps, 3)
    out.update(corpus_frames=len(index), target_samples=int(target.numel()))
    return out


def bench_fit(reps, T=20700, N=1240000, L=256, k=4, S=1024, hop=128, R=256, gain_max=4.0):
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(T, L, device="cuda", generator=g)
    c = torch.randn(N, L, device="cuda", generator=g)
    per_file = N // 8
    lengths = [((per_file + (N - 8 * per_file if i == 7 else 0)) - 1) * hop + S for i in range(8)]
    _, padded, row_start, _, _ = M.frame_tables(lengths, S, hop)
    assert row_start.size == N
    room = torch.from_numpy(M.shift_room(lengths, S, hop)).cuda()
    row_start = torch.from_numpy(row_start).cuda()
    audio = torch.randn(int(padded.sum()), device="cuda", generator=g) * 0.3
    target = torch.randn((T - 1) * hop + S, device="cuda", generator=g) * 0.3
    idx, _ = M.knn_topk(q, c, k)
    shift, gain, _ = M.fit_grains(target, idx, hop, S, audio, row_start, room, R, gain_max)
    out = torch.empty((T, S), dtype=torch.float32, device="cuda")
    calls = dict(search=lambda: M.knn_topk(q, c, k),
                 fit=lambda: M.fit_grains(target, idx, hop, S, audio, row_start, room, R, gain_max),
                 gather=lambda: M.gather_fitted(audio, idx, shift, gain, S, row_start, out=out),
                 gather_mean=lambda: M.gather_mean(audio, idx, S, row_start=row_start, out=out))
    ms = dict.fromkeys(calls, float("inf"))
    for _ in range(3):                                            # alternating
        for name, fn in calls.items():
            ms[name] = min(ms[name], timed(fn, reps))
    fmas = 2.0 * T * k * (2 * R + 1) * S
    return dict(T=T, N=N, L=L, k=k, S=S, hop=hop, R=R, reps=reps, search_ms=round(ms["search"], 3),
                fit_ms=round(ms["fit"], 3), gather_ms=round(ms["gather"], 4), gather_mean_ms=round(ms["gather_mean"], 4),
                fit_over_search=round(ms["fit"] / ms["search"], 4), fit_fmas=fmas,
                fit_fmas_per_s=fmas / (ms["fit"] * 1e-3), of_unpacked_bound=round(fmas / (ms["fit"] * 1e-3) / 39.3e12, 4),
                moved=float((shift != 0).float().mean()), clamped=float((gain >= gain_max).float().mean()))


def fit_report(r, device):
    return "\n".join([
        "grain fitting on %s (tools/mosaic_bench.py --fit): HIP events around %d calls after a warm-up, alternating in "
        "one process," % (device, r["reps"]),
        "best of three rounds", "",
        "T = %d target frames at hop %d, k = %d, S = %d, R = %d; corpus N = %d frames at hop %d in 8 files, L = %d"
        % (r["T"], r["hop"], r["k"], r["S"], r["R"], r["N"], r["hop"], r["L"]),
        "search   (RV_MOSAIC_KNN)          %10.3f ms" % r["search_ms"],
        "fit      (RV_GRAIN_FIT)           %10.3f ms   = %.4f of the search; %.3g fmas -> %.3g fma/s = %.3f of 39.3 T/s"
        % (r["fit_ms"], r["fit_over_search"], r["fit_fmas"], r["fit_fmas_per_s"], r["of_unpacked_bound"]),
        "gather   (RV_GRAIN_GATHER)        %10.4f ms" % r["gather_ms"],
        "gather   (RV_MOSAIC_GATHER_MEAN)  %10.4f ms" % r["gather_mean_ms"],
        "grains moved off the grid: %.4f; gains at gain_max: %.4f (random data)" % (r["moved"], r["clamped"])]) + "\n"


def replay_ms(launch, reps, rounds=3):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(rounds):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            launch()
        t1.record()
        t1.synchronize()
        best = min(best, t0.elapsed_time(t1) / reps)
    return best


def captured(fn):
    """fn() (which enqueues on the current stream) as a graph -> a callable that replays it on the current stream."""
    from rawaudiovae_kelsey_amd.engine import Graph
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = Graph(side)
    with torch.cuda.stream(side):
        with g:
            fn()
    torch.cuda.current_stream().wait_stream(side)
    return lambda: g.launch(torch.cuda.current_stream())


def bench_live_search(reps):
    from rawaudiovae_kelsey_amd import _lib
    rows = []
    g = torch.Generator(device="cuda").manual_seed(0)
    for N in (124000, 1240000):
        c = torch.randn(N, 256, device="cuda", generator=g)
        for k in (4, 16):
            for T in (1, 4, 16, 64):
                q = torch.randn(T, 256, device="cuda", generator=g)
                launches, outs = {}, {}
                for name, op, small in (("small", _lib.MOSAIC_KNN_SMALL, True), ("tile", _lib.MOSAIC_KNN, False)):
                    idx = torch.empty((T, k), dtype=torch.int32, device="cuda")
                    dist = torch.empty((T, k), dtype=torch.float32, device="cuda")
                    nbytes = M.knn_workspace_bytes(T, N, 256, k, small=small)
                    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
                    outs[name] = (idx, dist, ws)
                    launches[name] = captured(lambda op=op, idx=idx, dist=dist, ws=ws, nbytes=nbytes: M._call(
                        op, T=T, N=N, L=256, k=k, q=M.ptr(q), c=M.ptr(c), idx=M.ptr(idx), dist=M.ptr(dist), ws=M.ptr(ws),
                        ws_bytes=nbytes))
                ms = {"small": float("inf"), "tile": float("inf")}
                for _ in range(3):                                # alternating
                    for name in ("small", "tile"):
                        ms[name] = min(ms[name], replay_ms(launches[name], reps, rounds=1))
                same = bool(torch.equal(outs["small"][0], outs["tile"][0])
                            and torch.equal(outs["small"][1].view(torch.int32), outs["tile"][1].view(torch.int32)))
                rows.append(dict(N=N, k=k, T=T, small_ms=round(ms["small"], 4), tile_ms=round(ms["tile"], 4),
                                 small_tb_per_s=round(N * 256 * 4 * -(-T // 16) / (ms["small"] * 1e-3) / 1e12, 3),
                                 same_bits=same))
        del c
    return rows


def bench_live_blocks(reps):
    from rawvae.model import VAE
    torch.manual_seed(0)
    m = VAE(1024, 2048, 256).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for n_frames in (6872, 124000, 1240000):
        index = M.LatentIndex(m, hop=128)
        per_file = n_frames // 8
        for i in range(8):
            frames = per_file + (n_frames - 8 * per_file if i == 7 else 0)
            index.add(torch.randn((frames - 1) * 128 + 1024, device="cuda", generator=g) * 0.3, "c%d" % i)
        assert len(index) == n_frames
        for n_streams, hop, block in ((1, 128, 128), (1, 256, 256), (1, 256, 1024), (16, 256, 1024)):
            for mode in ("grains", "decode"):
                sm = M.StreamingMosaic(index, n_streams, block, hop=hop, k=4, mode=mode, window="hann",
                                       continuity=0.5).capture()
                sm.graph_input.copy_(torch.randn(n_streams, block, device="cuda", generator=g) * 0.3)
                ms = replay_ms(sm.replay, reps)
                budget = block / 44100.0 * 1e3
                rows.append(dict(N=n_frames, n_streams=n_streams, hop=hop, block=block, mode=mode,
                                 rows=n_streams * block // hop, ms=round(ms, 4), block_ms=round(budget, 3),
                                 meets=bool(ms < budget)))
                del sm
        del index
        torch.cuda.empty_cache()
    return rows


LAGS = (0, 1, 4, 16, 64)


def bench_live_lag(reps):
    from rawvae.model import VAE
    torch.manual_seed(0)
    m = VAE(1024, 2048, 256).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for n_frames in (124000, 1240000):
        index = M.LatentIndex(m, hop=128)
        per_file = n_frames // 8
        for i in range(8):
            frames = per_file + (n_frames - 8 * per_file if i == 7 else 0)
            index.add(torch.randn((frames - 1) * 128 + 1024, device="cuda", generator=g) * 0.3, "c%d" % i)
        assert len(index) == n_frames
        for k in (4, 16):
            for n_streams, hop, block in ((1, 128, 128), (16, 256, 1024)):
                x = torch.randn(n_streams, block, device="cuda", generator=g) * 0.3
                sms = {}
                for lag in LAGS:
                    sm = M.StreamingMosaic(index, n_streams, block, hop=hop, k=k, mode="grains", window="hann",
                                           continuity=0.5, lag=lag).capture()
                    sm.graph_input.copy_(x)
                    for _ in range(-(-(lag + 1) // sm.frames_per_block)):   # fill the window: steady state
                        sm.replay()
                    sms[lag] = sm
                ms = dict.fromkeys(LAGS, float("inf"))
                for _ in range(3):                                # alternating
                    for lag in LAGS:
                        ms[lag] = min(ms[lag], replay_ms(sms[lag].replay, reps, rounds=1))
                budget = block / 44100.0 * 1e3
                for lag in LAGS:
                    per_row = (ms[lag] - ms[0]) * 1e6 / ((block // hop) * (lag + 1)) if lag else 0.0
                    rows.append(dict(N=n_frames, k=k, n_streams=n_streams, hop=hop, block=block, lag=lag,
                                     ms=round(ms[lag], 4), block_ms=round(budget, 3), meets=bool(ms[lag] < budget),
                                     over_lag0_ns_per_frame_row=round(per_row, 1)))
                del sms
        del index
        torch.cuda.empty_cache()
    return rows


FIT_RS = (0, 64, 256, 1024)


def bench_live_fit(reps, n_frames=124000, k=4, hop=256, block=256, gain_max=4.0):
    from rawvae.model import VAE
    torch.manual_seed(0)
    m = VAE(1024, 2048, 256).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    index = M.LatentIndex(m, hop=128)
    per_file = n_frames // 8
    for i in range(8):
        frames = per_file + (n_frames - 8 * per_file if i == 7 else 0)
        index.add(torch.randn((frames - 1) * 128 + 1024, device="cuda", generator=g) * 0.3, "c%d" % i)
    assert len(index) == n_frames
    rows = []
    for continuity, lag in ((0.0, 0), (0.5, 8)):
        for n_streams in (1, 8):
            x = torch.randn(n_streams, block, device="cuda", generator=g) * 0.3
            sms = {}
            for R in (None,) + FIT_RS:                            # None: no fit
                kw = {} if R is None else dict(fit=R, gain_max=gain_max)
                sm = M.StreamingMosaic(index, n_streams, block, hop=hop, k=k, mode="grains", window="hann",
                                       continuity=continuity, lag=lag, **kw).capture()
                sm.graph_input.copy_(x)
                for _ in range(lag + 4):                          # fill the window and the target ring: steady state
                    sm.replay()
                sms[R] = sm
            ms = dict.fromkeys(sms, float("inf"))
            for _ in range(3):                                    # alternating
                for R in sms:
                    ms[R] = min(ms[R], replay_ms(sms[R].replay, reps, rounds=1))
            budget = block / 44100.0 * 1e3
            for R in FIT_RS:
                shift = sms[R].last_fit()[0]
                rows.append(dict(N=n_frames, k=k, n_streams=n_streams, hop=hop, block=block, continuity=continuity,
                                 lag=lag, R=R, gain_max=gain_max, fits_per_block=int(shift.numel()),
                                 ms=round(ms[R], 4), unfitted_ms=round(ms[None], 4), over_ms=round(ms[R] - ms[None], 4),
                                 block_ms=round(budget, 3), meets=bool(ms[R] < budget),
                                 moved=float((shift != 0).float().mean())))
            del sms
    return rows


def live_fit_report(rows, device):
    out = ["live grain fitting on %s (tools/mosaic_bench.py --live --fit): HIP events around graph replays after a "
           "warm-up that fills" % device, "every window and target ring", "",
           "one StreamingMosaic.replay() per block, grains, k = %d, hop = block = %d, S = 1024, Hann window, gain_max %g, "
           "VAE(1024, 2048, 256)," % (rows[0]["k"], rows[0]["block"], rows[0]["gain_max"]),
           "N = %d corpus frames; fitted and unfitted replays alternate in one process, best of three rounds; over = ms - "
           "unfitted ms" % rows[0]["N"],
           "%8s %5s %4s %5s %5s %10s %12s %10s %10s %6s" % ("streams", "cont", "lag", "R", "fits", "ms/block", "unfitted ms",
                                                           "over ms", "block ms", "meets")]
    for r in rows:
        out.append("%8d %5g %4d %5d %5d %10.4f %12.4f %10.4f %10.3f %6s" % (
            r["n_streams"], r["continuity"], r["lag"], r["R"], r["fits_per_block"], r["ms"], r["unfitted_ms"],
            r["over_ms"], r["block_ms"], "yes" if r["meets"] else "NO"))
    return "\n".join(out) + "\n"


def live_lag_report(rows, device):
    out = ["live mosaicing with a lag on %s (tools/mosaic_bench.py --live --lag): HIP events around graph replays after a "
           "warm-up that fills every window" % device, "",
           "one StreamingMosaic.replay() per block, grains, continuity 0.5, Hann window, VAE(1024, 2048, 256); lag 0 is "
           "k_live_select,", "lag > 0 is k_live_lag; alternating in one process, best of three rounds; ns/row = (ms - ms "
           "at lag 0) per frame of the block", "and row of the window (lag + 1)",
           "%9s %3s %8s %5s %6s %4s %10s %10s %6s %8s" % ("N", "k", "streams", "hop", "block", "lag", "ms/block", "block ms",
                                                          "meets", "ns/row")]
    for r in rows:
        out.append("%9d %3d %8d %5d %6d %4d %10.4f %10.3f %6s %8s" % (
            r["N"], r["k"], r["n_streams"], r["hop"], r["block"], r["lag"], r["ms"], r["block_ms"],
            "yes" if r["meets"] else "NO", "%.1f" % r["over_lag0_ns_per_frame_row"] if r["lag"] else "-"))
    return "\n".join(out) + "\n"


def live_report(search, blocks, device):
    out = ["live mosaicing on %s (tools/mosaic_bench.py --live): HIP events around graph replays after a warm-up" % device,
           "", "few-query search (RV_MOSAIC_KNN_SMALL) against RV_MOSAIC_KNN, L = 256, best of three alternating rounds",
           "%9s %3s %3s %10s %10s %8s %14s %5s" % ("N", "k", "T", "small ms", "tile ms", "tile/sm", "small TB/s read",
                                                    "bits")]
    for r in search:
        out.append("%9d %3d %3d %10.4f %10.4f %8.2f %14.3f %5s" % (
            r["N"], r["k"], r["T"], r["small_ms"], r["tile_ms"], r["tile_ms"] / r["small_ms"], r["small_tb_per_s"],
            "same" if r["same_bits"] else "DIFF"))
    out += ["", "one StreamingMosaic.replay() per block, k = 4, continuity 0.5, Hann window, VAE(1024, 2048, 256)",
            "%9s %8s %5s %6s %5s %7s %10s %10s %6s" % ("N", "streams", "hop", "block", "rows", "mode", "ms/block",
                                                      "block ms", "meets")]
    for r in blocks:
        out.append("%9d %8d %5d %6d %5d %7s %10.4f %10.3f %6s" % (
            r["N"], r["n_streams"], r["hop"], r["block"], r["rows"], r["mode"], r["ms"], r["block_ms"],
            "yes" if r["meets"] else "NO"))
    return "\n".join(out) + "\n"


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=None)
    p.add_argument("--live", action="store_true", help="time the live path only (few-query search, replay per block)")
    p.add_argument("--summary", default=None, help="--live / --fit: also write the tables to this text file")
    p.add_argument("--out", default=None)
    p.add_argument("--path", action="store_true", help="also time the unit selection beside the search at k = 16")
    p.add_argument("--lag", action="store_true", help="with --live: time the lagged unit selection against lag 0 instead")
    p.add_argument("--fit", action="store_true", help="time the grain fit beside the search (nothing else is timed); with --live: the live fit")
    a = p.parse_args(argv)
    if a.fit and a.live:
        if a.lag:
            raise ValueError("--lag: --live --fit times lag 0 and lag 8 itself")
        res = dict(device=torch.cuda.get_device_name(0), host=platform.node(), live_fit=bench_live_fit(a.reps or 30))
        text = live_fit_report(res["live_fit"], res["device"])
        print(text, end="")
        for path, body in ((a.summary, text), (a.out, json.dumps(res, indent=1))):
            if path:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "w") as f:
                    f.write(body)
        return res
    if a.fit:
        res = dict(device=torch.cuda.get_device_name(0), host=platform.node(), fit=bench_fit(a.reps or 5))
        text = fit_report(res["fit"], res["device"])
        print(text, end="")
        for path, body in ((a.summary, text), (a.out, json.dumps(res, indent=1))):
            if path:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "w") as f:
                    f.write(body)
        return res
    if a.lag and not a.live:
        raise ValueError("--lag: needs --live")
    if a.lag:
        res = dict(device=torch.cuda.get_device_name(0), host=platform.node(), live_lag=bench_live_lag(a.reps or 30))
        text = live_lag_report(res["live_lag"], res["device"])
        print(text, end="")
        for path, body in ((a.summary, text), (a.out, json.dumps(res, indent=1))):
            if path:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "w") as f:
                    f.write(body)
        return res
    if a.live:
        reps = a.reps or 30
        res = dict(device=torch.cuda.get_device_name(0), host=platform.node(), live_search=bench_live_search(reps),
                   live_blocks=bench_live_blocks(reps))
        text = live_report(res["live_search"], res["live_blocks"], res["device"])
        print(text, end="")
        for path, body in ((a.summary, text), (a.out, json.dumps(res, indent=1))):
            if path:
                os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
                with open(path, "w") as f:
                    f.write(body)
        return res
    a.reps = a.reps or 5
    res = dict(device=torch.cuda.get_device_name(0), host=platform.node(),
               search=[bench_search(*s, a.reps) for s in SHAPES], mosaic=bench_mosaic(a.reps))
    if a.path:
        res["path"] = r = bench_path(20700, 1240000, 256, 16, a.reps)
        print("path T=%d N=%d L=%d k=%d: search %.3f ms; transition %.4f ms (%.1f GB/s of gathered rows), forward "
              "%.4f ms (%.1f ns/row), backtrack %.4f ms (%.1f ns/row), best_path() %.4f ms; continuing %.4f"
              % (r["T"], r["N"], r["L"], r["k"], r["search_ms"], r["transition_ms"], r["transition_gb_per_s"],
                 r["forward_ms"], r["forward_ns_per_row"], r["backtrack_ms"], r["backtrack_ns_per_row"],
                 r["best_path_ms"], r["continuing"]))
    for r in res["search"]:
        print("%-14s T=%-6d N=%d L=%d k=%d: %9.3f ms, %d splits, %d workgroups, %.3g terms/s = %.3f of the packed "
              "bound (%.3f of the unpacked)" % (r["shape"], r["T"], r["N"], r["L"], r["k"], r["ms"], r["splits"],
                                                 r["workgroups"], r["terms_per_s"], r["of_packed_bound"],
                                                 r["of_unpacked_bound"]))
    print("mosaic(): %s" % json.dumps(res["mosaic"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
