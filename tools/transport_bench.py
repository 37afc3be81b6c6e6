#!/usr/bin/env python3
"""Time the latent-transport kernels (csrc/transport.hip): RV_OT_SOFTMIN and RV_OT_MAP at T = N = 32768 rows with k = 16 and
k = 64 axes, RV_OT_MAP on T = 4 rows (a live block) against the same N, a whole LatentTransport.fit at that size, and one
replayed block of StreamingTransport beside StreamingVAE.replay at (S, H, L) = (1024, 2048, 256), hop = block = 256, 1 and
16 streams.  The yardstick of the two ops is a chunked torch fp64 cdist^2 + logsumexp (softmax @ V for the map) on the same GPU.

    python tools/transport_bench.py [--reps 10] [--summary FILE]

Per op: device time of one call (events around it, after three warm-up calls): the median, the least and the largest of
`reps` calls; then what the shapes say the call needs -- score elements, fp64 exp per element, f64 MFMA FLOP -- over the
median.  The live engines take turns window by window in one process.  Everything is synthetic and seeded.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd import transport as TR  # noqa: E402

N = 32768
L = 64
AXES = (16, 64)
LIVE_ROWS = 4
CHUNK = 2048          # rows of the torch yardstick's chunks: a [2048, 32768] fp64 block is 512 MB
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


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


def clouds(k, seed=0):
    rng = np.random.default_rng(seed + k)
    A = torch.from_numpy(rng.standard_normal((N, k))).cuda()
    B = torch.from_numpy(rng.standard_normal((N, k)) * 0.7 + 1.5 / np.sqrt(k)).cuda()
    hl = torch.cat([torch.from_numpy(rng.standard_normal(N) * 0.2 * k).cuda(),
                    torch.full((N,), -np.log(N), dtype=torch.float64, device="cuda")])
    return A, B, hl


def torch_softmin(A, B, hl, eps):
    h, lw = hl[:B.shape[0]], hl[B.shape[0]:]
    out = torch.empty(A.shape[0], dtype=torch.float64, device=A.device)
    for r in range(0, A.shape[0], CHUNK):
        s = lw[None, :] + (h[None, :] - torch.cdist(A[r:r + CHUNK], B).square_()) / eps
        out[r:r + CHUNK] = -eps * torch.logsumexp(s, dim=1)
    return out


def torch_map(A, B, hl, eps):
    h, lw = hl[:B.shape[0]], hl[B.shape[0]:]
    out = torch.empty_like(A)
    for r in range(0, A.shape[0], CHUNK):
        s = lw[None, :] + (h[None, :] - torch.cdist(A[r:r + CHUNK], B).square_()) / eps
        out[r:r + CHUNK] = torch.softmax(s, dim=1) @ B
    return out


def ops(reps):
    for k in AXES:
        A, B, hl = clouds(k)
        eps = float(np.float32(0.05 * 2.0 * k))     # the float32 the device reads, widened: the same epsilon on both sides
        ws = TR.workspace(N, N, k, A.device)
        f = torch.empty(N, dtype=torch.float64, device="cuda")
        pairs = float(N) * N
        kp = -(-k // 16) * 16
        med, lo, hi = timed(lambda: TR.softmin(A, B, hl, eps, out=f, ws=ws), reps)
        ref = timed(lambda: torch_softmin(A, B, hl, eps), max(3, reps // 3), 1)
        err = float((f - torch_softmin(A, B, hl, eps)).abs().max())
        say("SOFTMIN T %d N %d k %d: median %.3f ms [%.3f, %.3f]; %.3g score elements/s, %.3g fp64 exp/s (5 per 4 elements), "
            "%.2f TFLOP/s on the f64 MFMA (2 T N %d); torch cdist^2 + logsumexp in chunks of %d rows %.3f ms: %.2fx; "
            "max |f - torch's| %.3g" % (N, N, k, med, lo, hi, pairs / med * 1e3, 1.25 * pairs / med * 1e3,
                                        2 * pairs * kp / med * 1e-9, kp, CHUNK, ref[0], ref[0] / med, err))
        # the map: x = centre + y W^T with P = I on the first k axes, so the whitened rows are A
        c, P = np.zeros(L), np.eye(L)[:k]
        block = TR.basis_block(torch.from_numpy(c).cuda(), torch.from_numpy(P.copy()).cuda(), torch.from_numpy(P.T.copy()).cuda())
        x = torch.zeros((N, L), dtype=torch.float32, device="cuda")
        x[:, :k] = A.float()
        out, state = torch.empty_like(x), torch.empty((N, 3 + k), dtype=torch.float64, device="cuda")
        med, lo, hi = timed(lambda: TR.transport_map(x, block, B, hl, eps, k, out=out, state=state, ws=ws), reps)
        ref = timed(lambda: torch_map(A, B, hl, eps), max(3, reps // 3), 1)
        say("MAP     T %d N %d k %d: median %.3f ms [%.3f, %.3f]; %.3g score elements/s, %.2f TFLOP/s on the f64 MFMA "
            "(4 T N %d); torch cdist^2 + softmax @ V %.3f ms: %.2fx; ws %.1f MB" % (
                N, N, k, med, lo, hi, pairs / med * 1e3, 4 * pairs * kp / med * 1e-9, kp, ref[0], ref[0] / med, ws[1] / 1e6))
        xs, outs, sts = x[:LIVE_ROWS].contiguous(), out[:LIVE_ROWS].contiguous(), state[:LIVE_ROWS].contiguous()
        med, lo, hi = timed(lambda: TR.transport_map(xs, block, B, hl, eps, k, out=outs, state=sts, ws=ws), 5 * reps)
        say("MAP     T %d N %d k %d (a live block's rows): median %.3f ms [%.3f, %.3f]" % (LIVE_ROWS, N, k, med, lo, hi))


def fit(k=16):
    rng = np.random.default_rng(5)
    blobs = rng.standard_normal((8, L)) * 2
    xt = (blobs[rng.integers(0, 8, N)] + 0.5 * rng.standard_normal((N, L))).astype(np.float32)
    xs = (1.2 * (blobs[rng.integers(0, 8, N)] + 0.5 * rng.standard_normal((N, L))) + 1.0).astype(np.float32)
    xs, xt = torch.from_numpy(xs).cuda(), torch.from_numpy(xt).cuda()
    for run in range(2):       # the first run warms every shape up
        tr = TR.LatentTransport(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.fit(xs, xt, None)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    say("FIT     Ns = Nt = %d, L %d, k %d, epsilon 0.05, tol 1e-3: %.3f s wall for %d iterations (%.3f ms each), marginal error "
        "%.3g, cost per frame %.6g" % (N, L, k, dt, tr.n_iter_, dt / tr.n_iter_ * 1e3, tr.err_, tr.cost_))
    return tr


def live(tr, reps, S=1024, H=2048, Lm=256, block=256, windows=6):
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd.stream import StreamingVAE
    from rawaudiovae_kelsey_amd.synth import make_params
    model = VAE(S, H, Lm).cuda().eval()
    model.load_state_dict({n: torch.from_numpy(v) for n, v in make_params(S, H, Lm, 0).items()})
    k = tr.n_components
    rng = np.random.default_rng(9)
    big = TR.LatentTransport(k)._set(
        torch.zeros(Lm, dtype=torch.float64, device="cuda"), torch.eye(Lm, dtype=torch.float64, device="cuda")[:k].contiguous(),
        torch.eye(Lm, dtype=torch.float64, device="cuda")[:, :k].contiguous(), tr.ys_, tr.yt_, tr.f_, tr.g_, tr.lws_, tr.lwt_,
        tr.epsilon_)
    for n_streams in (1, 16):
        x = torch.from_numpy((0.3 * rng.standard_normal((n_streams, block))).astype(np.float32)).cuda()
        engines = (("StreamingTransport", TR.StreamingTransport(model, big, n_streams, block, block).capture()),
                   ("StreamingVAE", StreamingVAE(model, n_streams, block, block).capture()))
        ms = {name: [] for name, _ in engines}
        for _ in range(windows):
            for name, eng in engines:
                ms[name].append(timed(lambda: eng.replay(x), reps)[0])
        t, v = (float(np.median(ms[name])) for name, _ in engines)
        say("LIVE    %d stream%s, block = hop = %d, (S, H, L) = (%d, %d, %d), k %d, N %d: StreamingTransport.replay %.3f ms "
            "[%.3f, %.3f], StreamingVAE.replay %.3f ms [%.3f, %.3f] (medians of %d alternating windows of %d): +%.3f ms" % (
                n_streams, "" if n_streams == 1 else "s", block, S, H, Lm, k, big.yt_.shape[0], t, min(ms["StreamingTransport"]),
                max(ms["StreamingTransport"]), v, min(ms["StreamingVAE"]), max(ms["StreamingVAE"]), windows, reps, t - v))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--summary", default=None, help="also write the lines to this file")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("transport_bench.py measures on the GPU; none is available")
    say("device: %s; torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    ops(args.reps)
    live(fit(), args.reps)
    if args.summary:
        with open(args.summary, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
