#!/usr/bin/env python3
"""Time the recurrence kernels (csrc/recur.hip): the self-join of one trajectory of T frames at L = 64, the costs launch
(RV_ALIGN_COST, band 0) and the profile launch (RV_RECUR_PROFILE, exclusion zone m, mirrored, the library's split count)
at T = 4096, 16384 and 32768 with m = 16, 64 and 256.

    python tools/recur_bench.py [--reps 3] [--windows 5] [--sizes 4096,16384,32768] [--out build/recur_bench.json]

Per case: device time of each launch (events around `reps` back-to-back calls after a warm-up; the median and the spread
of `windows` such windows), and what the profile launch moves, computed from the shapes:
  dm_bytes     the bytes of Dm, which HBM delivers once
  load_bytes   the bytes the workgroups load: a block of 16 rows reads 16 + m - 1 rows of Dm, so Dm goes through the
               caches (16 + m - 1) / 16 times
  adds         the fp64 adds of the window sums, T (N - m + 1) m
and the least time each of the three could take alone: dm_bytes at 6.3 TB/s (HBM, achievable), load_bytes at 34.5 TB/s (the
L2s' aggregate) and adds at 39.3e12 per second (256 CUs x 64 fp64 adds per clock x 2.4 GHz).  The largest of the three
names the bound; the measured time over it is the distance from that bound.
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

from rawaudiovae_kelsey_amd import align as A, recur as R  # noqa: E402

L = 64
MS = (16, 64, 256)
BI = 16                                   # csrc/recur.hip: REC_BI
HBM, L2, ADDS = 6.3e12, 34.5e12, 256 * 64 * 2.4e9


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


def counts(T_frames, m):
    """What the profile launch of a self-join of T_frames frames moves (see the module doc)."""
    N, T = T_frames, T_frames - m + 1
    nb = -(-T // BI)
    dm_bytes, load_bytes, adds = 4 * T_frames * N, 4 * nb * (BI + m - 1) * N, T * (N - m + 1) * m
    est = dict(hbm_ms=1e3 * dm_bytes / HBM, l2_ms=1e3 * load_bytes / L2, add_ms=1e3 * adds / ADDS)
    return dict(dm_bytes=dm_bytes, load_bytes=load_bytes, adds=adds, bound=max(est, key=est.get)[:-3], **est)


def bench_size(T_frames, reps, n_windows):
    g = torch.Generator(device="cuda").manual_seed(T_frames)
    mu = torch.randn(T_frames, L, device="cuda", generator=g)
    dm = torch.empty(T_frames, T_frames, device="cuda")
    w = windows(lambda: A.local_costs(mu, mu, 0, dm), reps, n_windows)
    costs = dict(costs_ms=float(np.median(w)), costs_ms_min_max=[min(w), max(w)])
    out = []
    for m in MS:
        T = T_frames - m + 1
        ws = R.workspace(T, T_frames, m, 0, "cuda")
        res = (torch.empty(T, dtype=torch.float64, device="cuda"), torch.empty(T, dtype=torch.int32, device="cuda"))
        w = windows(lambda: R.profile(dm, m, 0, m, R.RANGE_MAX, True, 0, ws, res), reps, n_windows)
        c = dict(frames=T_frames, m=m, L=L, reps=reps, ws_bytes=ws.numel(), profile_ms=float(np.median(w)),
                 profile_ms_min_max=[min(w), max(w)], **costs, **counts(T_frames, m))
        c["over_bound"] = c["profile_ms"] / c[c["bound"] + "_ms"]
        assert bool(torch.isfinite(res[0]).all()) and int(res[1].min()) >= 0
        out.append(c)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--sizes", default="4096,16384,32768")
    p.add_argument("--out", default=os.path.join(REPO, "build", "recur_bench.json"))
    a = p.parse_args()
    cases = [c for T in (int(v) for v in a.sizes.split(",")) for c in bench_size(T, a.reps, a.windows)]
    res = dict(device=torch.cuda.get_device_name(0), host=platform.node(), torch=torch.__version__, hip=torch.version.hip,
               cases=cases)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for c in cases:
        print("T=%-5d m=%-3d costs %8.3f ms [%.3f, %.3f]  profile %8.3f ms [%.3f, %.3f]  Dm %.2f GB, loaded %.2f GB, "
              "%.3g fp64 adds; least: HBM %.3f ms, L2 %.3f ms, adds %.3f ms -> %s-bound, measured %.2fx that" % (
                  c["frames"], c["m"], c["costs_ms"], *c["costs_ms_min_max"], c["profile_ms"], *c["profile_ms_min_max"],
                  c["dm_bytes"] / 1e9, c["load_bytes"] / 1e9, c["adds"], c["hbm_ms"], c["l2_ms"], c["add_ms"], c["bound"],
                  c["over_bound"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
