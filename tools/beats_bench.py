#!/usr/bin/env python3
"""Time the beat ops (csrc/beat.hip) at a 5-minute file beside their numpy oracle and write profiles/beats_summary.txt.

    python tools/beats_bench.py [--runs 9] [--out build/beats_bench.json] [--summary profiles/beats_summary.txt]

The curve is tests/beat_oracle.py's planted pulses: T = 52000 frames (5 minutes at 44.1 kHz, hop 256), a pulse every 86
frames (120 bpm) jittered by 2; lags 43 .. 258 (40 to 240 bpm), windows of 1378 frames (8 s) every 172 (1 s), the prior
centred on 120 bpm, tightness 100.  Every device figure is the median [min, max] of `runs` timed calls after two warm-up
calls, device events around one call (operands and outputs allocated before).  The oracle runs once on this box's CPU
and its outputs are compared with the device's bit for bit.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

T, P0, JITTER = 52000, 86, 2
LO, HI, WN, HW = 43, 258, 1378, 172


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def timed(fn, runs):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1))
    return out


def ms(s):
    return "%.4g [%.4g, %.4g]" % (s["median"], s["min"], s["max"])


def same(got, want):
    got = [g.cpu().numpy() for g in got]
    return bool(all(g.shape == w.shape and np.array_equal(g.view(np.uint8), np.ascontiguousarray(w).view(np.uint8))
                    for g, w in zip(got, want)))


def summary_text(rep):
    o, g, k = rep["onset"], rep["tempogram"], rep["track"]
    chain = o["ms"]["median"] + g["ms"]["median"] + k["ms"]["median"]
    return "\n".join([
        "Latent beats (csrc/beat.hip), one MI355X (%s), `python tools/beats_bench.py --runs %d` (raw JSON written under" % (
            rep["device"], rep["runs"]),
        "build/; this file is written by the tool from it).  Planted pulses (tests/beat_oracle.py): T = %d frames, a pulse" % T,
        "every %d frames jittered by %d; lags %d .. %d, windows of %d frames every %d (%d windows), the prior centred on" % (
            P0, JITTER, LO, HI, WN, HW, g["windows"]),
        "%d frames, tightness 100.  Every device figure: two warm-up calls, then the median [min, max] of repeated timed" % P0,
        "calls, device events around one call.  The oracle: one run on this box's CPU, numpy %s." % rep["numpy"], "",
        "RV_BEAT_ONSET      three launches   %s ms   the oracle %.4g s   bit-equal: %s" % (ms(o["ms"]), o["oracle_s"], o["bit_equal"]),
        "RV_BEAT_TEMPOGRAM  three launches   %s ms   the oracle %.4g s   bit-equal: %s" % (ms(g["ms"]), g["oracle_s"], g["bit_equal"]),
        "                   %.4g window terms (two multiplies and an add each), %.3g a second; %d workgroups of 256 lags, %d"
        % (g["terms"], g["terms"] / (g["ms"]["median"] * 1e-3), g["workgroups"], g["lds_bytes"]),
        "                   bytes of LDS each; period %d" % g["period"],
        "RV_BEAT_TRACK      one workgroup    %s ms   the oracle %.4g s   bit-equal: %s" % (ms(k["ms"]), k["oracle_s"], k["bit_equal"]),
        "                   dlo %d, dhi %d: %d blocks of %d frames, %d lanes per frame; %d beats walked back by one thread"
        % (k["dlo"], k["dhi"], k["blocks"], k["dlo"], k["lanes"], k["beats"]),
        "", "The chain of the three ops: %.4g ms; the tracker's share of it %.0f %%." % (chain, 100.0 * k["ms"]["median"] / chain)]) + "\n"


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=9)
    p.add_argument("--out", default=os.path.join(REPO, "build", "beats_bench.json"))
    p.add_argument("--summary", default=os.path.join(REPO, "profiles", "beats_summary.txt"))
    args = p.parse_args(argv)
    import torch
    import beat_oracle as O
    from rawaudiovae_kelsey_amd import beats as B
    curve, _ = O.pulse_curve(P0, T, JITTER)
    win, prior = B.window_values(WN), B.tempo_prior(LO, HI, float(P0))
    report = dict(device=torch.cuda.get_device_name(0), host=os.uname().nodename, numpy=np.__version__, runs=args.runs)

    nov = torch.from_numpy(curve).cuda()
    ws = B.workspace(T, nov.device)
    on = B.onset(nov, ws)
    t_on = stats(timed(lambda: B.onset(nov, ws, on), args.runs))
    t0 = time.perf_counter()
    want_on = O.onset(curve)
    report["onset"] = dict(ms=t_on, oracle_s=time.perf_counter() - t0, bit_equal=same(on, want_on))
    print("onset", json.dumps(report["onset"]), flush=True)

    table = B.tempogram_table(win, prior, WN, LO, HI, nov.device)
    tg = B.tempogram(on[0], WN, HW, LO, HI, table=table)
    t_tg = stats(timed(lambda: B.tempogram(on[0], WN, HW, LO, HI, table=table, out=tg), args.runs))
    t0 = time.perf_counter()
    want_tg = O.tempogram(want_on[0], WN, HW, LO, HI, win, prior)
    nW, nlag = tg[0].shape
    terms = float(sum(max(0, min(WN, T - n * HW - tau)) for n in range(nW) for tau in range(LO, HI + 1)))
    P = int(tg[3][0])
    report["tempogram"] = dict(ms=t_tg, oracle_s=time.perf_counter() - t0, bit_equal=same(tg, want_tg), windows=nW, lags=nlag,
                               terms=terms, workgroups=nW * -(-nlag // 256), lds_bytes=(2 * WN + HI) * 8, period=P)
    print("tempogram", json.dumps(report["tempogram"]), flush=True)

    dlo, dhi, pen = B.penalty_table(P)
    pen_d = torch.from_numpy(pen).cuda()
    tr = B.track(on[0], P, pen_d, dlo, dhi)
    t_tr = stats(timed(lambda: B.track(on[0], P, pen_d, dlo, dhi, tr), args.runs))
    t0 = time.perf_counter()
    want_tr = O.track(want_on[0], dlo, dhi, P, pen)
    lanes = 1
    while lanes < 64 and 2 * lanes * dlo <= 1024:
        lanes *= 2
    report["track"] = dict(ms=t_tr, oracle_s=time.perf_counter() - t0, bit_equal=same(tr, want_tr), dlo=dlo, dhi=dhi,
                           blocks=-(-T // dlo), lanes=lanes, beats=int(tr[3][0]))
    print("track", json.dumps(report["track"]), flush=True)
    for path, text in ((args.out, json.dumps(report, indent=1)), (args.summary, summary_text(report))):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    print(summary_text(report))
    return report


if __name__ == "__main__":
    main()
