#!/usr/bin/env python3
"""Time the structure ops (csrc/structure.hip) beside their yardsticks and write profiles/segment_summary.txt.

    python tools/segment_bench.py [--runs 9] [--skip-cli] [--out build/segment_bench.json]
                                  [--summary profiles/segment_summary.txt]

Random fp32 latents.  Every device figure is the median [min, max] of `runs` timed calls after two warm-up calls, device
events around one call.

  NOVELTY    T = 20000, L = 256, R in {16, 64, 256}, band 2R - 1, beside RV_ALIGN_COST of the same band on the same
             operands in the same process, the two taking turns.  The band is read at least once: T W 4 bytes at the HBM
             rate is the floor stated beside it; the kernel itself stages, per workgroup of TB = 1024 // 2R frames, the
             (2R + TB - 1)^2 window those frames share, from L2 into LDS.
  oracle     RV_STRUCT_NOVELTY at T = 2000, L = 64, R in {16, 64} beside tests/structure_oracle.py's numpy form on this
             box's CPU (one run), from the same self-distance matrix.
  PEAKS      T = 20000 on the R = 64 curve, gap 16, mean radius 128, delta 0.5.
  find       `segment.py find` end to end (wav in, JSON out, the model loaded from a checkpoint) on a 2-minute sound at
             44.1 kHz, (S, H, L) = (1024, 2048, 256), hop 256, kernel 32: wall-clock seconds of the second call.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

T_BIG, L_BIG, KERNELS = 20000, 256, (16, 64, 256)
T_SMALL, L_SMALL, KERNELS_SMALL = 2000, 64, (16, 64)
HBM_BYTES_PER_S = 8.0e12        # MI355X


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


def find_seconds():
    import torch
    import segment as cli
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd import data as D
    S, H, L, SR = 1024, 2048, 256, 44100
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        ini, ck, wav = os.path.join(tmp, "m.ini"), os.path.join(tmp, "ckpt"), os.path.join(tmp, "in.wav")
        with open(ini, "w") as f:
            f.write("[audio]\nsampling_rate = %d\nsegment_length = %d\n[VAE]\nn_units = %d\nlatent_dim = %d\n" % (SR, S, H, L))
        torch.save({"epoch": 0, "state_dict": VAE(S, H, L).state_dict(), "optimizer": {}}, ck)
        rng = np.random.default_rng(0)
        t = np.arange(5 * SR) / SR
        events = [0.4 * np.sin(2 * np.pi * f0 * t) + 0.05 * rng.standard_normal(t.size) for f0 in rng.uniform(110, 3000, 24)]
        D.write_wav(wav, np.concatenate(events).astype(np.float32), SR)          # 24 events of 5 s: 2 minutes
        argv = ["find", "--config", ini, "--checkpoint", ck, "--in", wav, "--hop", "256", "--kernel", "32", "--gap", "16",
                "--delta", "0.5", "--out", os.path.join(tmp, "s.json")]
        out = []
        for _ in range(2):
            t0 = time.perf_counter()
            rep = cli.main(argv)
            torch.cuda.synchronize()
            out.append(time.perf_counter() - t0)
        return dict(first_call_s=out[0], second_call_s=out[1], samples=rep["samples"], frames=rep["frames"],
                    segments=rep["segments"], band=rep["band"])


def ms(s):
    return "%.4g [%.4g, %.4g]" % (s["median"], s["min"], s["max"])


def summary_text(rep):
    lines = ["Latent structure (csrc/structure.hip), one MI355X (%s), `python tools/segment_bench.py --runs %d` (raw JSON" % (
        rep["device"], rep["runs"]),
        "written under build/; this file is written by the tool from it).  Random fp32 latents.  Every device figure: two",
        "warm-up calls, then the median [min, max] of repeated timed calls, device events around one call (NOVELTY and COST:",
        "the two taking turns in one process).", "",
        "T = %d, L = %d, band 2R - 1" % (T_BIG, L_BIG)]
    for R in KERNELS:
        n = rep["novelty"][str(R)]
        lines += ["R = %-3d W = %-4d  RV_STRUCT_NOVELTY %s ms   RV_ALIGN_COST of the same band %s ms   NOVELTY / COST %.2f" % (
            R, n["W"], ms(n["novelty_ms"]), ms(n["cost_ms"]), n["novelty_over_cost"]),
            "                  the band read once at %.0f TB/s (the floor): %.4g ms; window terms per second %.3g; %d frames per"
            % (HBM_BYTES_PER_S / 1e12, n["floor_ms"], n["terms_per_s"], n["frames_per_workgroup"]),
            "                  workgroup, %.4g MB staged into LDS, %.3g bytes per second" % (n["staged_bytes"] / 1e6, n["staged_bytes_per_s"])]
    lines += ["", "Beside the numpy oracle (tests/structure_oracle.py, one run on this box's CPU, numpy %s), T = %d, L = %d:" % (
        rep["numpy"], T_SMALL, L_SMALL)]
    for R in KERNELS_SMALL:
        o = rep["oracle"][str(R)]
        lines += ["R = %-3d RV_STRUCT_NOVELTY %s ms   the oracle %.4g s   (%.0f x)   bit-equal: %s" % (
            R, ms(o["novelty_ms"]), o["oracle_s"], o["oracle_s"] * 1e3 / o["novelty_ms"]["median"], o["bit_equal"])]
    p = rep["peaks"]
    lines += ["", "RV_STRUCT_PEAKS, T = %d (the R = 64 curve, gap %d, mean radius %d, delta %g), five launches: %s ms, %d segments" % (
        T_BIG, p["gap"], p["mean_radius"], p["delta"], ms(p["peaks_ms"]), p["segments"])]
    if "find" in rep:
        f = rep["find"]
        lines += ["", "`segment.py find` end to end (a 2-minute sound at 44.1 kHz read from wav, (S, H, L) = (1024, 2048, 256) loaded",
                  "from a checkpoint, hop 256, kernel 32, gap 16, delta 0.5: %d samples, %d frames, band %d, %d segments, JSON"
                  % (f["samples"], f["frames"], f["band"], f["segments"]),
                  "written), wall clock, one process: first call %.3f s, second call %.3f s." % (f["first_call_s"], f["second_call_s"])]
    return "\n".join(lines) + "\n"


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=9)
    p.add_argument("--skip-cli", action="store_true")
    p.add_argument("--out", default=os.path.join(REPO, "build", "segment_bench.json"))
    p.add_argument("--summary", default=os.path.join(REPO, "profiles", "segment_summary.txt"))
    args = p.parse_args(argv)
    import torch
    import structure_oracle as O
    from rawaudiovae_kelsey_amd import align as A
    from rawaudiovae_kelsey_amd import structure as S
    report = dict(device=torch.cuda.get_device_name(0), host=os.uname().nodename, numpy=np.__version__, runs=args.runs,
                  novelty={}, oracle={})
    g = torch.Generator().manual_seed(1)
    mu = torch.randn((T_BIG, L_BIG), generator=g).cuda()
    curve = None
    for R in KERNELS:
        r = 2 * R - 1
        W = 2 * r + 1
        dm = torch.empty((T_BIG, W), dtype=torch.float32, device="cuda")
        w = S.taper_tensor(S.taper(R, 0.5), R, "cuda")
        nov = torch.empty(T_BIG, dtype=torch.float64, device="cuda")
        t_nov, t_cost = [], []
        for _ in range(3):                                   # the two take turns
            t_cost += timed(lambda: A.local_costs(mu, mu, r, out=dm), args.runs // 3 + 1)
            t_nov += timed(lambda: S.novelty(dm, T_BIG, r, R, w, out=nov), args.runs // 3 + 1)
        n, c = stats(t_nov), stats(t_cost)
        terms = float(T_BIG) * (2 * R) ** 2
        tb = 1024 // (2 * R)
        staged = 4.0 * -(-T_BIG // tb) * (2 * R + tb - 1) ** 2
        report["novelty"][str(R)] = dict(
            T=T_BIG, L=L_BIG, R=R, band=r, W=W, novelty_ms=n, cost_ms=c, novelty_over_cost=n["median"] / c["median"],
            floor_ms=4.0 * T_BIG * W / HBM_BYTES_PER_S * 1e3, terms_per_s=terms / (n["median"] * 1e-3),
            frames_per_workgroup=tb, staged_bytes=staged, staged_bytes_per_s=staged / (n["median"] * 1e-3))
        print(R, json.dumps(report["novelty"][str(R)]), flush=True)
        if R == 64:
            curve = nov.clone()
        del dm
    gap, radius, delta = 16, 128, 0.5
    ws = S.workspace(T_BIG, "cuda")
    outs = S.peaks(curve, gap, radius, delta, ws)
    report["peaks"] = dict(T=T_BIG, gap=gap, mean_radius=radius, delta=delta, segments=int(outs[1][0]),
                           peaks_ms=stats(timed(lambda: S.peaks(curve, gap, radius, delta, ws, outs), args.runs)))
    print("peaks", json.dumps(report["peaks"]), flush=True)
    small = torch.randn((T_SMALL, L_SMALL), generator=g)
    for R in KERNELS_SMALL:
        r = 2 * R - 1
        dm = S.self_costs(small.cuda(), r)
        w = S.taper(R, 0.5)
        wd = S.taper_tensor(w, R, "cuda")
        nov = torch.empty(T_SMALL, dtype=torch.float64, device="cuda")
        t_nov = stats(timed(lambda: S.novelty(dm, T_SMALL, r, R, wd, out=nov), args.runs))
        full = S.self_costs(small.cuda(), 0).cpu().numpy()
        t0 = time.perf_counter()
        want = O.novelty(full, R, w)
        sec = time.perf_counter() - t0
        report["oracle"][str(R)] = dict(T=T_SMALL, L=L_SMALL, R=R, novelty_ms=t_nov, oracle_s=sec,
                                        bit_equal=bool(np.array_equal(want.view(np.int64), nov.cpu().numpy().view(np.int64))))
        print("oracle", R, json.dumps(report["oracle"][str(R)]), flush=True)
    if not args.skip_cli:
        report["find"] = find_seconds()
    for path, text in ((args.out, json.dumps(report, indent=1)), (args.summary, summary_text(report))):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
