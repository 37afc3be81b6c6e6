#!/usr/bin/env python3
"""Time the SOM kernels (csrc/som.hip) at the frame-level shape N = 2^20 rows, M = 1024 nodes (32 x 32), L = 256 and
at the file-level shape N = 2000, M = 64 (8 x 8), L = 256.

    python tools/som_bench.py [--reps 20] [--out build/som_bench.json]

Per shape: device time (events around `reps` back-to-back launches, after a warm-up) of rv_som_bmu, rv_som_node_sums,
rv_som_update and of one whole epoch (the three in a row, as LatentSOM.fit issues them), and rv_som_bmu's rate in
FLOP/s counting 3 N M L (subtract, multiply, add per term) against the 157.3 TFLOP/s fp32 peak of the MI355X.
"""
import argparse
import json
import os
import platform
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd._lib import lib, ptr, stream_ptr  # noqa: E402

FP32_PEAK = 157.3e12
SHAPES = (("frame_level", 1 << 20, 32, 32, 256), ("file_level", 2000, 8, 8, 256))


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


def bench_shape(name, N, rows, cols, L, reps):
    M = rows * cols
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(N, L, device="cuda", generator=g)
    w = torch.randn(M, L, device="cuda", generator=g)
    w2 = torch.empty_like(w)
    best, second = (torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(2))
    d1, d2 = (torch.empty(N, device="cuda") for _ in range(2))
    sums = torch.empty(M, L, dtype=torch.float64, device="cuda")
    counts = torch.empty(M, dtype=torch.int64, device="cuda")
    R, st = lib(), stream_ptr()

    def bmu():
        R.rv_som_bmu(ptr(x), N, ptr(w), M, L, ptr(best), ptr(second), ptr(d1), ptr(d2), st)

    def node_sums():
        R.rv_som_node_sums(ptr(x), N, L, ptr(best), M, ptr(sums), ptr(counts), st)

    def update():
        R.rv_som_update(ptr(sums), ptr(counts), ptr(w), rows, cols, L, 2.0, ptr(w2), st)

    def epoch():
        bmu()
        node_sums()
        update()

    out = dict(shape=name, N=N, M=M, grid=[rows, cols], L=L, reps=reps)
    for k, fn in (("bmu", bmu), ("node_sums", node_sums), ("update", update), ("epoch", epoch)):
        out[k + "_ms"] = timed(fn, reps)
    flops = 3.0 * N * M * L
    out["bmu_tflops"] = flops / (out["bmu_ms"] * 1e-3) / 1e12
    out["bmu_frac_fp32_peak"] = out["bmu_tflops"] * 1e12 / FP32_PEAK
    out["epoch_frac_fp32_peak"] = flops / (out["epoch_ms"] * 1e-3) / FP32_PEAK
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=os.path.join(REPO, "build", "som_bench.json"))
    a = p.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), host=platform.node(), torch=torch.__version__,
               hip=torch.version.hip, fp32_peak_tflops=FP32_PEAK / 1e12,
               shapes=[bench_shape(*s, reps=a.reps) for s in SHAPES])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for s in res["shapes"]:
        print("%-12s N=%-8d M=%-5d L=%d  bmu %.3f ms (%.1f TF, %.2f of fp32 peak)  node_sums %.3f ms  update %.3f ms  "
              "epoch %.3f ms" % (s["shape"], s["N"], s["M"], s["L"], s["bmu_ms"], s["bmu_tflops"],
                                 s["bmu_frac_fp32_peak"], s["node_sums_ms"], s["update_ms"], s["epoch_ms"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
