#!/usr/bin/env python3
"""Time the restoration kernels (csrc/smooth.hip): RV_SMOOTH_FILTER and RV_SMOOTH_BACKWARD in dense mode at L = 64 on
one sequence of T = 4096 frames at k = 16 and at k = 64, and on 64 sequences of 64 frames at k = 16.

    python tools/smooth_bench.py [--reps 5] [--windows 5] [--out build/smooth_bench.json]

Per case: device time of each op (events around `reps` back-to-back calls after a warm-up; the median and the spread of
`windows` such windows), the time per frame of the longest sequence (the sequential part: one workgroup per sequence)
and the filter's fp64 rate counting 5 k^3 flops per frame.  The model is synthetic and exact: A = 0.9 Q with Q
orthogonal, B = sqrt(1 - 0.81) I, so A A^T + B B^T = I; one frame in eight is missing.
"""
import argparse
import json
import os
import platform
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd import smooth as SM  # noqa: E402
from rawaudiovae_kelsey_amd.walk import LatentWalk  # noqa: E402

L = 64
CASES = (("one_long_k16", 1, 4096, 16), ("one_long_k64", 1, 4096, 64), ("batch_k16", 64, 64, 16))


def synthetic_walk(k, seed=0):
    rng = np.random.default_rng(seed)
    V = np.linalg.qr(rng.standard_normal((L, L)))[0][:k]
    lam = np.geomspace(3.0, 0.3, k)
    A = 0.9 * np.linalg.qr(rng.standard_normal((k, k)))[0]
    B = np.sqrt(1 - 0.81) * np.eye(k)
    s = np.sqrt(lam)[:, None]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()  # noqa: E731
    return LatentWalk(k)._set(t(rng.uniform(-1, 1, L)), t(V), t(lam), t(np.stack([A.T, B.T])), t(V / s), t(V * s), k, 1, 1)


def windows(fn, reps, n):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        out.append(t0.elapsed_time(t1) / reps)
    return out


def bench_case(name, n_seq, frames, k, reps, n_windows):
    T = n_seq * frames
    sm = SM.LatentSmoother(synthetic_walk(k), 1e-2)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(T, L, device="cuda", generator=g)
    weight = torch.ones(T, device="cuda")
    weight[3::8] = 0
    rs = np.arange(n_seq + 1, dtype=np.int64) * frames
    x, fields, held = sm.operands(x, rs, weight)
    res = torch.empty(T, k + 2, dtype=torch.float64, device="cuda")
    z = torch.empty(T, L, device="cuda")
    state = torch.empty(T, k, dtype=torch.float64, device="cuda")
    out = dict(case=name, sequences=n_seq, frames=frames, T=T, k=k, L=L, reps=reps, ws_bytes=fields["ws_bytes"])
    for op, fn in (("filter", lambda: sm.run_filter(fields, res)), ("backward", lambda: sm.run_backward(fields, z, state))):
        w = windows(fn, reps, n_windows)
        out[op + "_ms"] = float(np.median(w))
        out[op + "_ms_min_max"] = [min(w), max(w)]
        out[op + "_us_per_frame"] = 1e3 * out[op + "_ms"] / frames
    out["filter_gflops"] = 5.0 * k ** 3 * T / (out["filter_ms"] * 1e-3) / 1e9
    assert bool(torch.isfinite(res).all()) and bool(torch.isfinite(z).all())
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--out", default=os.path.join(REPO, "build", "smooth_bench.json"))
    a = p.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), host=platform.node(), torch=torch.__version__, hip=torch.version.hip,
               cases=[bench_case(*c, reps=a.reps, n_windows=a.windows) for c in CASES])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for c in res["cases"]:
        print("%-13s %2d x %4d frames k=%-2d  filter %8.3f ms [%.3f, %.3f] (%.2f us/frame, %.1f GFLOP/s fp64)  backward %8.3f ms "
              "[%.3f, %.3f] (%.2f us/frame)  ws %.1f MB" % (
                  c["case"], c["sequences"], c["frames"], c["k"], c["filter_ms"], *c["filter_ms_min_max"],
                  c["filter_us_per_frame"], c["filter_gflops"], c["backward_ms"], *c["backward_ms_min_max"],
                  c["backward_us_per_frame"], c["ws_bytes"] / 1e6))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
