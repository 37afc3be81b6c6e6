#!/usr/bin/env python3
"""Streaming ingest on the MI355X: the device ingest kernels' rates and the frames/s of the train_iterable loop.

  python tools/ingest_bench.py --out DIR            # everything below; writes DIR/ingest_bench.json + a text summary

1. Kernel rates: rv_resample_sinc_hann at 48000->44100 and 96000->44100 and rv_pcm_to_f32 on int16 mono / stereo
   payloads, 60 s of audio per launch, timed by `rocprofv3 --kernel-trace --stats` (a child run of this script with
   --kernels), as output samples per second of kernel time.
2. Loop throughput: frames/s of train_iterable.py's loop (StreamingFrames.batches -> TrainEngine.step, losses drained
   every `loss_ring` batches) at kelsey_iterable.ini's shape (segment 1024, hop 128, 2048 units, latent 256, batch
   4096) over synthetic on-disk int16 corpora (mono / stereo, 44.1 kHz / 48 kHz, 6 files of 30 s), with a cache
   (16 MiB) smaller than every corpus, so that every file is ingested again on every pass:
     ingest = host, ingest = device, the corpus fully cached (a warm pass first), and the step alone (one batch).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

S, HOP, H, L, B, SR = 1024, 128, 2048, 256, 4096, 44100
KERNEL_REPS = 20
KERNEL_CASES = [("resample 48000->44100", 48000), ("resample 96000->44100", 96000),
                ("pcm_to_f32 int16 mono", 1), ("pcm_to_f32 int16 stereo", 2)]


def kernels():
    """The launches the profiler times (in this order, KERNEL_REPS each); prints the outputs per launch."""
    import torch
    from rawaudiovae_kelsey_amd import data as D
    counts = {}
    for name, sr_in in KERNEL_CASES[:2]:
        x = torch.randn(60 * sr_in, device="cuda")
        D.resample_sinc_hann_device(x, sr_in, SR)       # bank upload outside the timed launches
        torch.cuda.synchronize()
        for _ in range(KERNEL_REPS):
            _, n = D.resample_sinc_hann_device(x, sr_in, SR)
        counts[name] = n
    for name, ch in KERNEL_CASES[2:]:
        h = D.WavHeader(1, ch, SR, 16, 2 * ch, 2, 44, 60 * SR * 2 * ch)
        payload = torch.randint(0, 256, (h.data_bytes,), dtype=torch.uint8, device="cuda")
        for _ in range(KERNEL_REPS):
            _, n = D.pcm_to_f32_device(payload, h, HOP)
        counts[name] = n
    torch.cuda.synchronize()
    print("KERNEL_COUNTS " + json.dumps(counts))


def kernel_rates(out):
    d = os.path.join(out, "ingest_kernels")
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "ingest", "--",
           sys.executable, os.path.abspath(__file__), "--kernels"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("KERNEL_COUNTS ")]
    if r.returncode != 0 or not line:
        raise RuntimeError("rocprofv3 run failed (%d): %s" % (r.returncode, (r.stdout + r.stderr)[-3000:]))
    counts = json.loads(line[0].split(" ", 1)[1])
    trace = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = [r for r in csv.DictReader(open(trace)) if "k_resample_sinc_hann" in r["Kernel_Name"]
            or "k_pcm_to_f32" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # the launches of each kernel, in launch order, are KERNEL_REPS per case (the first resampler launch per pair
    # is the warm-up one)
    rs = [r for r in rows if "k_resample_sinc_hann" in r["Kernel_Name"]]
    pc = [r for r in rows if "k_pcm_to_f32" in r["Kernel_Name"]]
    groups = {KERNEL_CASES[0][0]: rs[1:1 + KERNEL_REPS], KERNEL_CASES[1][0]: rs[2 + KERNEL_REPS:2 + 2 * KERNEL_REPS],
              KERNEL_CASES[2][0]: pc[:KERNEL_REPS], KERNEL_CASES[3][0]: pc[KERNEL_REPS:2 * KERNEL_REPS]}
    res = {}
    for name, g in groups.items():
        ns = sorted(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in g)
        med = ns[len(ns) // 2]
        res[name] = {"launches": len(ns), "outputs_per_launch": counts[name], "median_us": med / 1e3,
                     "min_us": ns[0] / 1e3, "G_samples_per_s": counts[name] / med}
    stats = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
    res["stats_csv"] = [dict(r) for r in csv.DictReader(open(stats[0]))
                        if "k_resample" in r["Name"] or "k_pcm" in r["Name"]] if stats else []
    return res


def write_corpus(root, sr, channels, n_files=6, seconds=30):
    from scipy.io import wavfile
    os.makedirs(root, exist_ok=True)
    rng = np.random.default_rng(sr + channels)
    files = []
    t = np.arange(seconds * sr) / sr
    for i in range(n_files):
        a = 0.3 * np.sin(2 * np.pi * (100 + 37 * i) * t) + 0.05 * rng.standard_normal(len(t))
        pcm = (np.clip(a, -1, 1) * 32767).astype(np.int16)
        if channels == 2:
            pcm = np.stack([pcm, pcm[::-1]], axis=1)
        p = os.path.join(root, "f%02d.wav" % i)
        wavfile.write(p, sr, pcm)
        files.append(p)
    return files


def loop_rate(engine, batches, warm, timed):
    """frames/s of `timed` steps after `warm` steps of the train_iterable loop."""
    import torch
    ring = engine.ring if hasattr(engine, "ring") else 64
    t0 = None
    for i, data in enumerate(batches):
        if i == warm:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        engine.step(data)
        if (i + 1) % ring == 0:
            engine.drain_losses()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    engine.drain_losses()
    return timed * B / dt


def loops(tmp, host_batches, device_batches):
    import torch
    import train as T
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd.engine import TrainEngine
    engine = TrainEngine(S, H, L, B, device="cuda", kl_beta=1e-4, lr=1e-4, seed=0, ring=64, **T.engine_options({}))
    small = 16 << 20
    res = {}
    corpora = {}
    for sr in (44100, 48000):
        for ch in (1, 2):
            name = "%dHz_%s" % (sr, "mono" if ch == 1 else "stereo")
            corpora[name] = write_corpus(os.path.join(tmp, name), sr, ch)
    for name, files in corpora.items():
        for ingest, nb in (("host", host_batches), ("device", device_batches)):
            st = D.StreamingFrames(files, SR, HOP, S, "cuda", shuffle=True, seed=0, cache_bytes=small, ingest=ingest)
            warm = 4
            fps = loop_rate(engine, st.batches(B, warm + nb), warm, nb)
            res["%s_%s" % (name, ingest)] = fps
            print("%-24s ingest=%-6s %12.0f frames/s" % (name, ingest, fps), flush=True)
    for name in ("44100Hz_mono", "48000Hz_mono"):
        files = corpora[name]
        st = D.StreamingFrames(files, SR, HOP, S, "cuda", shuffle=True, seed=0, cache_bytes=8 << 30, ingest="device")
        per_pass = sum(len(st._dataset(f)) for f in files) // B
        fps = loop_rate(engine, st.batches(B, 4 + device_batches), 4, device_batches)
        res["%s_cached" % name] = fps
        print("%-24s cached       %12.0f frames/s (%d batches per pass)" % (name, fps, per_pass), flush=True)
    x = torch.randn(B, S, device="cuda") * 0.3
    fps = loop_rate(engine, (x for _ in range(20 + 400)), 20, 400)
    res["step_alone"] = fps
    print("%-24s              %12.0f frames/s" % ("step alone", fps), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true", help="(child of the profiler run) launch the timed kernels")
    ap.add_argument("--out", default="build/ingest_bench")
    ap.add_argument("--host-batches", type=int, default=12)
    ap.add_argument("--device-batches", type=int, default=200)
    ap.add_argument("--no-profile", action="store_true")
    a = ap.parse_args()
    if a.kernels:
        return kernels()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ingest_bench needs a GPU")
    os.makedirs(a.out, exist_ok=True)
    result = {"shape": {"segment_length": S, "hop": HOP, "n_units": H, "latent": L, "batch": B, "sampling_rate": SR},
              "device": torch.cuda.get_device_name()}
    if not a.no_profile:
        result["kernels"] = kernel_rates(a.out)
        for k, v in result["kernels"].items():
            if k != "stats_csv":
                print("%-26s %8.1f us per launch  %7.2f G samples/s" % (k, v["median_us"], v["G_samples_per_s"]),
                      flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        lp = loops(tmp, a.host_batches, a.device_batches)
    result["loop_frames_per_s"] = lp
    ratios = {}
    for sr in ("44100Hz", "48000Hz"):
        for ch in ("mono", "stereo"):
            k = "%s_%s" % (sr, ch)
            ratios[k + "_device_over_host"] = lp[k + "_device"] / lp[k + "_host"]
        ratios[sr + "_mono_device_over_cached"] = lp[sr + "_mono_device"] / lp[sr + "_mono_cached"]
    result["ratios"] = ratios
    for k, v in ratios.items():
        print("%-40s %8.2f" % (k, v))
    with open(os.path.join(a.out, "ingest_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "kernels"}))


if __name__ == "__main__":
    main()
