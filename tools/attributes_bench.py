#!/usr/bin/env python3
"""Time the latent-attribute ops (csrc/attr.hip) and write profiles/attributes_summary.txt.

    python tools/attributes_bench.py [--runs 9] [--out build/attributes_bench.json]
                                     [--summary profiles/attributes_summary.txt]

Seeded inputs.  Every figure is the median [min, max] of `runs` timed windows after two warm-up windows; a window is
`calls` back-to-back calls between two device events (so that it lasts tens of milliseconds), and the figure is the window
over `calls`.

  DESCRIBE   S = 1024, hop = 256, Hann window, three minutes of noise at 44.1 kHz.  The bytes the op needs are the waveform
             read once and the [T, 5] fp64 output written once; over the call time that is its achieved bandwidth, stated
             beside the HBM rate.  (Every sample is read by the S / hop = 4 frames that cover it; three of the four reads are
             served by the caches.)  Also without a window (three columns, no spectrum) for the share the transform takes.
  FIT        T = 2^18, L = 256, k = 64, N = 5: the five launches of one call, and its floor: x read once (T L 4 bytes) at
             the HBM rate.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

S_DESC, HOP_DESC, SR, SECONDS = 1024, 256, 44100, 180
T_FIT, L_FIT, K_FIT, N_FIT = 1 << 18, 256, 64, 5
HBM_BYTES_PER_S = 8.0e12        # MI355X


def stats(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def timed(fn, runs, calls):
    """ms per call: `runs` windows of `calls` calls each, after two warm-up windows"""
    import torch
    for _ in range(2 * calls):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / calls)
    return out


def ms(s):
    return "%.4g [%.4g, %.4g]" % (s["median"], s["min"], s["max"])


def summary_text(rep):
    d, w, f = rep["describe"], rep["describe_no_window"], rep["fit"]
    return "\n".join([
        "Latent attributes (csrc/attr.hip), one MI355X (%s), `python tools/attributes_bench.py --runs %d` (raw JSON written" % (
            rep["device"], rep["runs"]),
        "under build/; this file is written by the tool from it).  Seeded inputs.  Every figure: two warm-up windows, then the",
        "median [min, max] of repeated timed windows of back-to-back calls between two device events, per call.", "",
        "RV_ATTR_DESCRIBE, S = %d, hop = %d, Hann window, %d s of noise at %d Hz: %d samples, T = %d frames, one launch" % (
            S_DESC, HOP_DESC, SECONDS, SR, d["samples"], d["T"]),
        "  %s ms per call (%d calls per window); %.4g frames per second, %.0f times real time" % (
            ms(d["ms"]), d["calls"], d["frames_per_s"], d["times_real_time"]),
        "  needed bytes (the waveform once, the output once): %.4g MB; achieved %.4g GB/s = %.3g %% of the HBM rate (%.0f TB/s)" % (
            d["bytes"] / 1e6, d["bytes_per_s"] / 1e9, 100 * d["hbm_fraction"], HBM_BYTES_PER_S / 1e12),
        "  without a window (level, zcr, crest only): %s ms per call, %.3g %% of the HBM rate" % (ms(w["ms"]), 100 * w["hbm_fraction"]),
        "",
        "RV_ATTR_FIT, T = %d, L = %d, k = %d, N = %d, five launches, ws %.4g MB" % (T_FIT, L_FIT, K_FIT, N_FIT, f["ws_bytes"] / 1e6),
        "  %s ms per call (%d calls per window); x read once at the HBM rate (the floor): %.4g ms; status %d, n = %d" % (
            ms(f["ms"]), f["calls"], f["floor_ms"], f["status"], f["n"]),
        "  bit-identical from call to call: %s" % f["bit_identical"]]) + "\n"


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--runs", type=int, default=9)
    p.add_argument("--out", default=os.path.join(REPO, "build", "attributes_bench.json"))
    p.add_argument("--summary", default=os.path.join(REPO, "profiles", "attributes_summary.txt"))
    args = p.parse_args(argv)
    import torch
    from rawaudiovae_kelsey_amd import attributes as A
    from rawaudiovae_kelsey_amd.codec import frame_layout
    from rawaudiovae_kelsey_amd.pca import LatentPCA
    if not torch.cuda.is_available():
        raise SystemExit("attributes_bench.py measures on the GPU: no device found")
    report = dict(device=torch.cuda.get_device_name(0), host=os.uname().nodename, runs=args.runs)
    g = torch.Generator().manual_seed(1)
    n = SR * SECONDS
    T, padded = frame_layout(n, S_DESC, HOP_DESC)
    wave = torch.zeros(padded)
    wave[:n] = torch.rand(n, generator=g) * 2 - 1
    wave = wave.cuda()
    win, tab = A.tables(S_DESC, "hann", "cuda")
    for name, window, cols in (("describe", win, 5), ("describe_no_window", None, 3)):
        out = torch.empty((T, cols), dtype=torch.float64, device="cuda")
        calls = 40
        t = stats(timed(lambda: A.describe(wave, T, S_DESC, HOP_DESC, window, out=out, table=tab), args.runs, calls))
        nbytes = 4.0 * padded + 8.0 * cols * T
        report[name] = dict(T=T, samples=padded, calls=calls, ms=t, bytes=nbytes, bytes_per_s=nbytes / (t["median"] * 1e-3),
                            hbm_fraction=nbytes / (t["median"] * 1e-3) / HBM_BYTES_PER_S, frames_per_s=T / (t["median"] * 1e-3),
                            times_real_time=SECONDS / (t["median"] * 1e-3))
        print(name, json.dumps(report[name]), flush=True)
    x = torch.randn((T_FIT, L_FIT), generator=g).cuda()
    x = x * torch.linspace(1.0, 0.1, L_FIT, device="cuda") + 0.5
    ax = A.axes(LatentPCA().fit(x), K_FIT)
    D = (torch.randn((T_FIT, N_FIT), generator=g, dtype=torch.float64).cuda()
         + (x[:, :N_FIT].double() - 0.5) * torch.arange(1, N_FIT + 1, device="cuda"))
    D[::1000, 0] = float("-inf")          # silent frames
    res = (torch.empty(A.result_layout(K_FIT, N_FIT)[1], dtype=torch.float64, device="cuda"),
           torch.empty(2, dtype=torch.int32, device="cuda"))
    ws = A.workspace(T_FIT, K_FIT, N_FIT, "cuda")
    A.fit_targets(x, D, ax, out=res, ws=ws)
    first = res[0].clone()
    calls = 10
    t = stats(timed(lambda: A.fit_targets(x, D, ax, out=res, ws=ws), args.runs, calls))
    status, n_obs = (int(v) for v in res[1].cpu().numpy())
    report["fit"] = dict(T=T_FIT, L=L_FIT, k=K_FIT, N=N_FIT, calls=calls, ms=t, ws_bytes=ws[1],
                         floor_ms=4.0 * T_FIT * L_FIT / HBM_BYTES_PER_S * 1e3, status=status, n=n_obs,
                         bit_identical=bool(torch.equal(first.view(torch.int64), res[0].view(torch.int64))))
    print("fit", json.dumps(report["fit"]), flush=True)
    for path, text in ((args.out, json.dumps(report, indent=1)), (args.summary, summary_text(report))):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
