#!/usr/bin/env python3
"""Time the curve interpolation pipeline (LatentInterpolator.curve) on 120 s of synthetic 44.1 kHz audio at the
reference model's shape (S, H, L) = (1024, 2048, 256), at hop 1024 (TestDataset framing, the meso-scale variant) and
hop 128 (AudioDataset framing, "with extensions").

    python tools/interp_bench.py [--reps 5] [--max-rows 16384] [--out build/interp_bench.json]

Reports, per hop: the whole call (host to host, device-synchronised), frames/s of output, and per launch kind the
device time of the same launches issued one at a time between events (rv_match_pad, fc1 / fc21 / fc22 / fc3 / fc4 on
rv_linear_fp32, rv_latent_mix) with each GEMM's TFLOP/s against the 157.3 TFLOP/s fp32 MFMA peak of the MI355X.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd._lib import ACT_NONE, ACT_RELU, ACT_TANH, ALPHA_CURVE, lib, ptr, stream_ptr  # noqa: E402
from rawaudiovae_kelsey_amd.interpolate import LatentInterpolator, frame_layout  # noqa: E402
from rawvae.model import VAE  # noqa: E402

FP32_MFMA_PEAK = 157.3e12
S, H, L, SR = 1024, 2048, 256, 44100


def launches(it, a, b, curve, hop, eps):
    """The pipeline of LatentInterpolator.curve as (kind, flops, thunk) launches, operands preallocated."""
    dev = it.device
    n = max(a.numel(), b.numel())
    N, padded = frame_layout(n, S, hop)
    step = hop or S
    R = it.max_rows
    pa, pb = (torch.empty(padded, device=dev) for _ in range(2))
    mus = [torch.empty(N, L, device=dev) for _ in range(4)]
    h = torch.empty(min(R, N), H, device=dev)
    z = torch.empty(min(R, N), L, device=dev)
    out = torch.empty(N * S, device=dev)
    c = torch.from_numpy(curve).to(dev)
    W = {k: it.codec.weights(k) for k in ("fc1", "fc21", "fc22", "fc3", "fc4")}
    st = stream_ptr()
    L_ = lib()

    def lin(name, x, ldx, rows, act, y, ldy):
        w, bias = W[name]
        return lambda: L_.rv_linear_fp32(x, ldx, ptr(w), w.shape[1], ptr(bias), rows, w.shape[0], w.shape[1], act, y, ldy,
                                         st)
    ops = [("match_pad", 0, lambda: L_.rv_match_pad(ptr(a), a.numel(), n, ptr(pa), padded, st)),
           ("match_pad", 0, lambda: L_.rv_match_pad(ptr(b), b.numel(), n, ptr(pb), padded, st))]
    for wave, (mu, lv) in ((pa, mus[:2]), (pb, mus[2:])):
        for f0 in range(0, N, R):
            r = min(R, N - f0)
            ops.append(("fc1", 2 * r * S * H, lin("fc1", wave.data_ptr() + 4 * f0 * step, step, r, ACT_RELU, ptr(h), H)))
            ops.append(("fc21", 2 * r * H * L, lin("fc21", ptr(h), H, r, ACT_NONE, ptr(mu) + 4 * f0 * L, L)))
            ops.append(("fc22", 2 * r * H * L, lin("fc22", ptr(h), H, r, ACT_NONE, ptr(lv) + 4 * f0 * L, L)))
    for r0 in range(0, N, R):
        r = min(R, N - r0)
        e = eps.data_ptr() + 4 * r0 * L

        def mix(r0=r0, r=r, e=e):
            L_.rv_latent_mix(*[ptr(t) for t in mus], N, L, ALPHA_CURVE, ptr(c), c.numel(), r0, r, e, None, 0, 0, ptr(z),
                             None, None, None, st)
        ops.append(("latent_mix", 0, mix))
        ops.append(("fc3", 2 * r * L * H, lin("fc3", ptr(z), L, r, ACT_RELU, ptr(h), H)))
        ops.append(("fc4", 2 * r * H * S, lin("fc4", ptr(h), H, r, ACT_TANH, out.data_ptr() + 4 * r0 * S, S)))
    return N, ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-rows", type=int, default=16384)
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--out", default=os.path.join(REPO, "build", "interp_bench.json"))
    args = ap.parse_args()
    torch.manual_seed(0)
    model = VAE(S, H, L).cuda()
    it = LatentInterpolator(model, max_rows=args.max_rows)
    rng = np.random.default_rng(0)
    n = int(args.seconds * SR)
    t = np.arange(n) / SR
    a = torch.from_numpy((0.5 * np.sin(2 * np.pi * 220 * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)).cuda()
    b = torch.from_numpy((0.3 * rng.standard_normal(n * 3 // 4)).astype(np.float32)).cuda()   # repeated to a's length
    curve = np.sin(np.linspace(-500 * np.pi, 500 * np.pi, 20000))
    results = []
    for hop in (1024, 128):
        N, _ = frame_layout(n, S, hop)
        eps = torch.randn(N, L, device="cuda")
        y = it.curve(a, b, curve, hop=hop, eps=eps)          # warm-up (and the output checked below)
        torch.cuda.synchronize()
        walls = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            it.curve(a, b, curve, hop=hop, eps=eps)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - t0)
        N, ops = launches(it, a, b, curve, hop, eps)
        per = {}
        for rep in range(args.reps + 1):
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(ops) + 1)]
            evs[0].record()
            for i, (_, _, f) in enumerate(ops):
                f()
                evs[i + 1].record()
            torch.cuda.synchronize()
            if rep == 0:
                continue                                       # warm-up pass
            for i, (kind, flops, _) in enumerate(ops):
                d = per.setdefault(kind, {"launches": 0, "ms": [], "flops": 0})
                if rep == 1:
                    d["launches"] += 1
                    d["flops"] += flops
                d["ms"].append(evs[i].elapsed_time(evs[i + 1]))
        kinds = {}
        for kind, d in per.items():
            ms = float(np.sum(d["ms"]) / args.reps)            # device ms of all launches of this kind, one pass
            k = {"launches": d["launches"], "ms_per_pass": round(ms, 4),
                 "us_per_launch": round(1000 * ms / d["launches"], 2)}
            if d["flops"]:
                tf = d["flops"] / (ms * 1e-3)
                k["tflops"] = round(tf / 1e12, 2)
                k["pct_fp32_mfma_peak"] = round(100 * tf / FP32_MFMA_PEAK, 1)
            kinds[kind] = k
        wall = float(np.median(walls))
        r = {"hop": hop, "frames": N, "output_samples": N * S, "max_rows": args.max_rows, "wall_ms_median": round(
            1000 * wall, 3), "wall_ms_min": round(1000 * min(walls), 3), "frames_per_s": round(N / wall, 1),
            "device_ms_sum": round(sum(k["ms_per_pass"] for k in kinds.values()), 3), "kinds": kinds,
            "finite": bool(torch.isfinite(y).all().item())}
        results.append(r)
        print(json.dumps(r))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"shape": [S, H, L], "seconds": args.seconds, "sr": SR, "runs": results,
                   "device": torch.cuda.get_device_name(0)}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
