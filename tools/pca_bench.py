#!/usr/bin/env python3
"""Time the latent PCA (csrc/pca.hip) on synthetic latents at (N, L) = (2^20, 256) and (2^18, 64).

    python tools/pca_bench.py [--reps 5] [--trials 3] [--out build/pca_bench.json]

Per shape and trial (after a warm-up of every timed call; the figures are the median over the trials, with the spread),
device events around `reps` back-to-back calls:
  moments   RV_PCA_MOMENTS (4 launches): ms, and the fp64 flop/s of the covariance pass it achieves, N L (L + 1) flops
            (the tiles on and above the diagonal), against the fp64 matrix peak
  eig       RV_PCA_EIG on that covariance (one workgroup), with its sweeps and, against numpy.linalg.eigh, the three
            error ratios the tests bound (max |lambda - eigvalsh| and ||C V - V Lambda||_F over L u ||C||_F,
            ||V^T V - I||_F over L u)
  edit      RV_PCA_EDIT with all L axes, random gains and shifts
and beside them what the machine offers for the same job: torch.cov on the fp64 copy of x and torch.linalg.eigh, both on
the device (if they fail there: numpy.cov and numpy.linalg.eigh on the host, named so in the output), and for edit
the two fp64 torch.matmul it amounts to.
"""
import argparse
import json
import os
import platform
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd import pca as P  # noqa: E402

FP64_MATRIX_PEAK = 78.6e12    # flop/s (MI355X)
SHAPES = ((1 << 20, 256), (1 << 18, 64))
U = 2.0 ** -52


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


def host_timed(fn, reps):
    import time
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) * 1e3 / reps


def latents(N, L):
    """[N, L] fp32 on the device: a geometric spectrum 3 .. 1e-3 in a random rotation about means in [-3, 3]."""
    g = torch.Generator(device="cuda").manual_seed(L)
    sig = torch.from_numpy(np.geomspace(3, 1e-3, L)).float().cuda()
    Q = torch.linalg.qr(torch.randn(L, L, generator=g, device="cuda"))[0]
    return ((torch.randn(N, L, generator=g, device="cuda") * sig) @ Q
            + (torch.rand(L, generator=g, device="cuda") * 6 - 3)).contiguous()


def yardsticks(x, cov):
    """{name: (callable, timer)} of the device's own routines, or numpy's where the device refuses."""
    out = {}
    try:
        torch.cov(x[:1024].double().T)
        out["cov_torch_fp64_device"] = (lambda: torch.cov(x.double().T), timed)
    except Exception as e:   # noqa: BLE001
        print("torch.cov in fp64 does not run on the device (%s): numpy on the host" % e)
        xh = x.cpu().numpy()
        out["cov_numpy_host"] = (lambda: np.cov(xh.astype(np.float64), rowvar=False), host_timed)
    try:
        torch.linalg.eigh(cov)
        torch.cuda.synchronize()
        out["eigh_torch_device"] = (lambda: torch.linalg.eigh(cov), timed)
    except Exception as e:   # noqa: BLE001
        print("torch.linalg.eigh does not run on the device (%s): numpy on the host" % e)
        ch = cov.cpu().numpy()
        out["eigh_numpy_host"] = (lambda: np.linalg.eigh(ch), host_timed)
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--trials", type=int, default=3)
    p.add_argument("--out", default=os.path.join(REPO, "build", "pca_bench.json"))
    a = p.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), host=platform.node(), torch=torch.__version__, hip=torch.version.hip,
               host_threads=torch.get_num_threads(), reps=a.reps, trials=a.trials, shapes=[])
    for N, L in SHAPES:
        x = latents(N, L)
        centre, cov = P.moments(x)
        lam, comp, sweeps, converged = P.eig(cov)
        g = torch.Generator(device="cuda").manual_seed(1)
        gains = torch.rand(L, generator=g, device="cuda") * 2
        shifts = torch.rand(L, generator=g, device="cuda") * 2 - 1
        out = torch.empty_like(x)
        C, V, lm = cov.cpu().numpy(), comp.cpu().numpy(), lam.cpu().numpy()
        F = np.linalg.norm(C)
        ref = np.linalg.eigvalsh(C)[::-1]
        row = dict(N=N, L=L, sweeps=sweeps, converged=converged,
                   eigenvalue_ratio=float(np.abs(lm - ref).max() / (L * U * F)),
                   residual_ratio=float(np.linalg.norm(C @ V.T - V.T * lm) / (L * U * F)),
                   orthogonality_ratio=float(np.linalg.norm(V @ V.T - np.eye(L)) / (L * U)),
                   workspace_bytes=P.workspace_bytes(N, L))
        xd = x.double()
        calls = {"moments": (lambda: P.moments(x), timed), "eig": (lambda: P.eig(cov), timed),
                 "edit": (lambda: P.edit(x, comp, centre, lam, gains, shifts, out=out), timed),
                 "edit_torch_fp64_device": (lambda: ((xd - centre) @ comp.T) @ comp, timed)}
        calls.update(yardsticks(x, cov))
        ms = {k: [] for k in calls}
        for _ in range(a.trials):
            for k, (fn, timer) in calls.items():
                ms[k].append(timer(fn, a.reps))
        for k, v in ms.items():
            row[k + "_ms"] = statistics.median(v)
            row[k + "_ms_spread"] = [min(v), max(v)]
        row["moments_flops"] = N * L * (L + 1)
        row["moments_frac_fp64_matrix_peak"] = row["moments_flops"] / (row["moments_ms"] * 1e-3) / FP64_MATRIX_PEAK
        res["shapes"].append(row)
        print("N=%d L=%d: " % (N, L) + "; ".join("%s %.3f ms [%.3f, %.3f]" % (k, row[k + "_ms"], *row[k + "_ms_spread"])
                                                  for k in ms))
        print("   eig: %d sweeps, ratios %.3g %.3g %.3g (bounds 8, 16, 128); moments at %.3f of the fp64 matrix peak"
              % (sweeps, row["eigenvalue_ratio"], row["residual_ratio"], row["orthogonality_ratio"],
                 row["moments_frac_fp64_matrix_peak"]))
        del x, xd, out, calls
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
