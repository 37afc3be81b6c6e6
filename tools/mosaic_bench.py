#!/usr/bin/env python3
"""Time the mosaicing kNN search (rv_mosaic RV_MOSAIC_KNN, csrc/mosaic.hip) and one whole LatentIndex.mosaic() call.

    python tools/mosaic_bench.py [--reps 5] [--path] [--out build/mosaic_bench.json]

Search shapes (T, N, L, k): one minute of target at hop 128 (20 700 frames) and one second (344 frames), both against
one hour of corpus at hop 128 (1.24 M frames), latent_dim 256, k = 4.  Per shape: device time (events around `reps`
back-to-back calls after a warm-up), the workgroups of the search launch, and the rate in distance terms/s, T N L per
call.  A term is one subtract and one fma: against the 157.3 TFLOP/s fp32 spec of the MI355X (78.6 T fma/s with packed
math) the bound is about 39 T terms/s packed and 20 T terms/s unpacked -- spec-sheet arithmetic, not a measurement.

--path: the three steps of the unit selection (mosaic.best_path) for one minute of target (T = 20 700, N = 1.24 M,
L = 256, k = 16) beside the search of the same shape: the transition costs (RV_MOSAIC_TRANSITION, judged against HBM
rate: 2 k L 4 bytes of gathered latent rows per target row), the forward pass and the backtrack (one wave each; the
time per row is the length of the dependent chain).  The candidates are the search's own, on random data.

mosaic(): a VAE(1024, 2048, 256) with random weights, a 40 s corpus in 8 files and a 5 s target at hop 256, k = 4,
grains and decode, wall time of the call including the target's encoder pass (the corpus is indexed beforehand).
"""
import argparse
import json
import os
import platform
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd import mosaic as M  # noqa: E402

PACKED_TERMS, UNPACKED_TERMS = 157.3e12 / 2 / 2, 157.3e12 / 2 / 4
SHAPES = (("minute_target", 20700, 1240000, 256, 4), ("second_target", 344, 1240000, 256, 4))


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


def bench_search(name, T, N, L, k, reps):
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(T, L, device="cuda", generator=g)
    c = torch.randn(N, L, device="cuda", generator=g)
    ms = timed(lambda: M.knn_topk(q, c, k), reps)
    splits = max(1, M.knn_workspace_bytes(T, N, L, k) // (T * k * 8))
    terms = float(T) * N * L / (ms * 1e-3)
    return dict(shape=name, T=T, N=N, L=L, k=k, ms=round(ms, 3), splits=int(splits),
                workgroups=int(-(-T // 128) * splits), terms_per_s=terms,
                of_packed_bound=round(terms / PACKED_TERMS, 4), of_unpacked_bound=round(terms / UNPACKED_TERMS, 4))


def bench_path(T, N, L, k, reps):
    from rawaudiovae_kelsey_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(T, L, device="cuda", generator=g)
    c = torch.randn(N, L, device="cuda", generator=g)
    search_ms = timed(lambda: M.knn_topk(q, c, k), reps)
    idx, dist = M.knn_topk(q, c, k)
    next_of = torch.from_numpy(M.successor_table(torch.arange(N).div(20000, rounding_mode="floor").numpy())).cuda()
    trans = torch.empty((T, k, k), dtype=torch.float32, device="cuda")
    trans_ms = timed(lambda: M.transition_costs(c, idx, next_of, out=trans), reps)
    nbytes = M.path_workspace_bytes(T, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    slot = torch.empty(T, dtype=torch.int32, device="cuda")
    choice = torch.empty(T, dtype=torch.int32, device="cuda")
    cost = torch.empty(2, dtype=torch.float64, device="cuda")
    common = dict(T=T, k=k, idx=M.ptr(idx), dist=M.ptr(dist), ws=M.ptr(ws), ws_bytes=nbytes)
    fwd_ms = timed(lambda: M._call(_lib.MOSAIC_PATH_FORWARD, row0=0, rows=T, trans=M.ptr(trans), lam=1.0, **common),
                   reps)
    back_ms = timed(lambda: M._call(_lib.MOSAIC_PATH_BACKTRACK, slot=M.ptr(slot), choice=M.ptr(choice),
                                    cost=M.ptr(cost), **common), reps)
    whole_ms = timed(lambda: M.best_path(idx, dist, c, next_of, 1.0), reps)
    gathered = 2.0 * k * L * 4 * T + 4.0 * k * k * T
    return dict(T=T, N=N, L=L, k=k, search_ms=round(search_ms, 3), transition_ms=round(trans_ms, 4),
                transition_gb_per_s=round(gathered / (trans_ms * 1e-3) / 1e9, 1), forward_ms=round(fwd_ms, 4),
                forward_ns_per_row=round(fwd_ms * 1e6 / T, 1), backtrack_ms=round(back_ms, 4),
                backtrack_ns_per_row=round(back_ms * 1e6 / T, 1), best_path_ms=round(whole_ms, 4),
                continuing=float((choice[1:] == next_of[choice[:-1].clamp(min=0).long()]).float().mean()),
                cost=[float(v) for v in cost.cpu()])


def bench_mosaic(reps):
    from rawvae.model import VAE
    torch.manual_seed(0)
    m = VAE(1024, 2048, 256).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    sr = 44100
    index = M.LatentIndex(m, hop=256)
    for i in range(8):
        index.add(torch.randn(5 * sr, device="cuda", generator=g) * 0.3, "c%d" % i)
    target = torch.randn(5 * sr, device="cuda", generator=g) * 0.3
    out = {}
    for mode in ("grains", "decode"):
        index.mosaic(target, k=4, mode=mode, window="hann")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            index.mosaic(target, k=4, mode=mode, window="hann")
        torch.cuda.synchronize()
        out[mode + "_ms"] = round((time.perf_counter() - t0) * 1e3 / reps, 3)
    out.update(corpus_frames=len(index), target_samples=int(target.numel()))
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    p.add_argument("--path", action="store_true", help="also time the unit selection beside the search at k = 16")
    a = p.parse_args(argv)
    res = dict(device=torch.cuda.get_device_name(0), host=platform.node(),
               search=[bench_search(*s, a.reps) for s in SHAPES], mosaic=bench_mosaic(a.reps))
    if a.path:
        res["path"] = r = bench_path(20700, 1240000, 256, 16, a.reps)
        print("path T=%d N=%d L=%d k=%d: search %.3f ms; transition %.4f ms (%.1f GB/s of gathered rows), forward "
              "%.4f ms (%.1f ns/row), backtrack %.4f ms (%.1f ns/row), best_path() %.4f ms; continuing %.4f"
              % (r["T"], r["N"], r["L"], r["k"], r["search_ms"], r["transition_ms"], r["transition_gb_per_s"],
                 r["forward_ms"], r["forward_ns_per_row"], r["backtrack_ms"], r["backtrack_ns_per_row"],
                 r["best_path_ms"], r["continuing"]))
    for r in res["search"]:
        print("%-14s T=%-6d N=%d L=%d k=%d: %9.3f ms, %d splits, %d workgroups, %.3g terms/s = %.3f of the packed "
              "bound (%.3f of the unpacked)" % (r["shape"], r["T"], r["N"], r["L"], r["k"], r["ms"], r["splits"],
                                                 r["workgroups"], r["terms_per_s"], r["of_packed_bound"],
                                                 r["of_unpacked_bound"]))
    print("mosaic(): %s" % json.dumps(res["mosaic"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
