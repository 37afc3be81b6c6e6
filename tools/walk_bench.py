#!/usr/bin/env python3
"""Time one replayed block of the latent walk (StreamingWalk.replay) beside one replayed block of streaming
resynthesis (StreamingVAE.replay) at the same extents, and the fit that precedes a walk.

    python tools/walk_bench.py [--only walk|resynth] [--streams 1,16] [--windows 21] [--replays 200] [--out build/walk_bench.json]

(S, H, L) = (1024, 2048, 256), k = 64, hop = block = 256, a randomly initialised model and a walk fitted on 8192
synthetic AR(1) latents in 4 files.  Per stream count, after a warm-up of 100 replays: `windows` windows of `replays`
back-to-back graph replays each, device events around a window, the two engines taking turns window by window; the
figure is the median window's microseconds per block with [min, max].  `--only resynth` needs nothing of the walk, so
it also runs on a tree that has none.  The fit is timed once per op after one warm-up call.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

S, H, L, K, HOP = 1024, 2048, 256, 64, 256
T_FIT, FILES = 8192, 4


def window_us(fn, replays):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(replays):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / replays


def latents():
    """[T_FIT, L] fp32 on the device: per file and axis an AR(1) process, persistences 0.995 .. -0.5, a geometric
    spectrum 3 .. 3e-2 in a random rotation."""
    g = torch.Generator().manual_seed(0)
    rho = torch.linspace(0.995, -0.5, L, dtype=torch.float64)
    e = torch.randn((T_FIT, L), generator=g, dtype=torch.float64)
    s = torch.empty_like(e)
    per = T_FIT // FILES
    for t in range(T_FIT):
        s[t] = e[t] if t % per == 0 else rho * s[t - 1] + (1 - rho * rho).sqrt() * e[t]
    rot = torch.linalg.qr(torch.randn((L, L), generator=g, dtype=torch.float64))[0]
    x = (s * torch.from_numpy(np.geomspace(3, 3e-2, L))) @ rot
    return x.float().cuda(), np.arange(0, T_FIT + 1, per)


def once_ms(fn):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--only", default=None, choices=("walk", "resynth"))
    p.add_argument("--streams", default="1,16")
    p.add_argument("--windows", type=int, default=21)
    p.add_argument("--replays", type=int, default=200)
    p.add_argument("--out", default=os.path.join(REPO, "build", "walk_bench.json"))
    args = p.parse_args(argv)
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.stream import StreamingVAE
    torch.manual_seed(0)
    model = VAE(S, H, L).cuda().eval()
    report = dict(device=torch.cuda.get_device_name(0), extents=dict(S=S, H=H, L=L, k=K, hop=HOP, block=HOP),
                  windows=args.windows, replays=args.replays, blocks={})
    walk = None
    if args.only != "resynth":
        from rawaudiovae_kelsey_amd import pca as P
        from rawaudiovae_kelsey_amd import walk as W
        x, rs = latents()
        pca = P.LatentPCA().fit(x)
        walk = W.LatentWalk(K).fit(x, rs, pca)
        report["fit_ms"] = dict(lagcov=once_ms(lambda: W.lagcov(x, rs, pca.mean_)),
                                fit_given_the_pca=once_ms(lambda: W.LatentWalk(K).fit(x, rs, pca)),
                                pca=once_ms(lambda: P.LatentPCA().fit(x)))
        report["fit"] = dict(T=T_FIT, files=FILES, predictability=walk.predictability_,
                             norm_A=float(np.linalg.norm(walk.A_.cpu().numpy(), 2)))
    for ns in (int(v) for v in args.streams.split(",")):
        engines = {}
        if args.only != "walk":
            vae = StreamingVAE(model, ns, HOP, HOP, "hann").capture()
            engines["resynth"] = vae.replay
        if walk is not None:
            gen = W.StreamingWalk(model, walk, ns, HOP, HOP, "hann").capture()
            engines["walk"] = gen.replay
        for fn in engines.values():
            for _ in range(100):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in engines}
        for _ in range(args.windows):
            for name, fn in engines.items():
                times[name].append(window_us(fn, args.replays))
        report["blocks"][str(ns)] = {name: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v))
                                     for name, v in times.items()}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
