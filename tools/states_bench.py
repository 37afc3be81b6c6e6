#!/usr/bin/env python3
"""Time the latent-state kernels (csrc/hmm.hip): RV_HMM_EMIT, RV_HMM_FORWARD_BACKWARD, RV_HMM_MSTEP and RV_HMM_VITERBI on
a corpus of T = 262144 frames of L = 64 latents, as 64 files of 4096 frames and as 1024 files of 256 frames, with
S = 8 states over k = 16 axes and with S = 64 states over k = 64 axes.

    python tools/states_bench.py [--reps 10]

Per case and op: device time of one call (events around it, after three warm-up calls): the median, the least and the
largest of `reps` calls.  The latents, the axes and the parameters are synthetic and seeded; every frame is observed.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd import states as ST  # noqa: E402

L = 64
CORPORA = ((64, 4096), (1024, 256))       # files x frames
MODELS = ((8, 16), (64, 64))              # states, axes


def synthetic(S, k, seed=0):
    """(centre [L], P [k, L], theta) on the device: whitening rows over scales 0.5 .. 2, means a few units apart,
    variances in 0.25 .. 4, a random transition matrix with a heavy diagonal"""
    rng = np.random.default_rng(seed + 7 * S + k)
    P = np.linalg.qr(rng.standard_normal((L, L)))[0][:k] / np.geomspace(0.5, 2.0, k)[:, None]
    A = rng.uniform(0.05, 1, (S, S)) + 4 * np.eye(S)
    pi = rng.uniform(0.2, 1, S)
    theta = ST.pack_theta(rng.normal(0, 2, (S, k)), rng.uniform(0.25, 4, (S, k)), pi / pi.sum(), A / A.sum(axis=1, keepdims=True))
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda() for a in (rng.uniform(-1, 1, L), P, theta))


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=10)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("states_bench.py measures on the GPU; none is available")
    for files, length in CORPORA:
        T = files * length
        x = torch.from_numpy(np.random.default_rng(0).normal(0, 1.5, (T, L)).astype(np.float32)).cuda()
        seqs = (torch.from_numpy(np.arange(files + 1, dtype=np.int64) * length).cuda(), files)
        for S, k in MODELS:
            c, P, th = synthetic(S, k)
            ws = ST.workspace(T, S, k, x.device)
            logb = ST.emit(x, c, P, th, S)
            post = ST.forward_backward(logb, seqs, th, S, k, ws=ws)
            new = (torch.empty_like(th), torch.empty(S, dtype=torch.int32, device="cuda"))
            vit = (torch.empty(T, dtype=torch.int32, device="cuda"), torch.empty(files, dtype=torch.float64, device="cuda"))
            ops = (("EMIT", lambda: ST.emit(x, c, P, th, S, out=logb)),
                   ("FORWARD_BACKWARD", lambda: ST.forward_backward(logb, seqs, th, S, k, out=post, ws=ws)),
                   ("MSTEP", lambda: ST.mstep(x, c, P, post, seqs, th, S, 1e-3, out=new, ws=ws)),
                   ("VITERBI", lambda: ST.viterbi(logb, seqs, th, S, k, out=vit, ws=ws)))
            for name, fn in ops:
                print("%d files x %d frames, L %d, S %d, k %d, %-16s median %.3f ms [%.3f, %.3f], ws %.1f MB" % (
                    (files, length, L, S, k, name) + timed(fn, args.reps) + (ws[1] / 1e6,)), flush=True)


if __name__ == "__main__":
    main()
