"""Device time per block of the streaming engine (graph replay, HIP events) against the existing chain on the same
rows (five rv_linear_fp32 launches + rv_reparameterize), alternating in one process; host wall per replay.

    python tools/stream_bench.py [--iters 200] [--out profiles/stream_summary.txt]

Grid: n_streams in {1, 16, 64} x hop in {1024, 256}, block 1024, (S, H, L) = (1024, 2048, 256)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from rawvae.model import VAE
    from rawaudiovae_kelsey_amd import _lib
    from rawaudiovae_kelsey_amd._lib import lib, ptr
    from rawaudiovae_kelsey_amd.engine import Graph
    from rawaudiovae_kelsey_amd.stream import StreamingVAE
    assert torch.cuda.is_available(), "stream_bench needs a GPU"
    S, H, L, block = 1024, 2048, 256, 1024
    torch.manual_seed(0)
    model = VAE(S, H, L).cuda().eval()
    rows = []
    for ns in (1, 16, 64):
        for hop in (1024, 256):
            eng = StreamingVAE(model, ns, block, hop=hop, window="hann" if hop < S else None).capture()
            eng.graph_input.copy_(torch.rand((ns, block)).cuda() - 0.5)
            M = ns * (block // hop)
            # the existing chain on the same rows, captured the same way
            fr = torch.rand((M, S)).cuda() - 0.5
            h1, h3 = torch.empty((M, H)).cuda(), torch.empty((M, H)).cuda()
            mu, lv, z, eps = (torch.empty((M, L)).cuda() for _ in range(4))
            dec = torch.empty((M, S)).cuda()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            g = Graph(side)

            def lin(x, K, name, act, y, N):
                m = getattr(model, name)
                lib().rv_linear_fp32(ptr(x), K, ptr(m.weight), K, ptr(m.bias), M, N, K, act, ptr(y), N, side.cuda_stream)
            with g:
                lin(fr, S, "fc1", 1, h1, H)
                lin(h1, H, "fc21", 0, mu, L)
                lin(h1, H, "fc22", 0, lv, L)
                lib().rv_reparameterize(ptr(mu), ptr(lv), M * L, None, ptr(eps), 1, 0, ptr(z), side.cuda_stream)
                lin(z, L, "fc3", 1, h3, H)
                lin(h3, H, "fc4", 2, dec, S)
            torch.cuda.current_stream().wait_stream(side)
            cur = torch.cuda.current_stream()

            def new():
                eng.replay()

            def old():
                g.launch(cur)
            res = {"new": [], "old": [], "new_wall": []}
            for f in (new, old):
                for _ in range(20):
                    f()
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for name, f in (("new", new), ("old", old)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    for _ in range(a.iters):
                        f()
                    e1.record()
                    t_host = time.perf_counter() - t0
                    torch.cuda.synchronize()
                    res[name].append(e0.elapsed_time(e1) * 1000.0 / a.iters)
                    if name == "new":
                        res["new_wall"].append(t_host * 1e6 / a.iters)
            row = {"n_streams": ns, "hop": hop, "block": block, "rows": M,
                   "new_us_per_block": round(min(res["new"]), 2), "new_us_median": round(sorted(res["new"])[len(res["new"]) // 2], 2),
                   "old_us_per_block": round(min(res["old"]), 2), "old_us_median": round(sorted(res["old"])[len(res["old"]) // 2], 2),
                   "host_wall_us_per_replay": round(sorted(res["new_wall"])[len(res["new_wall"]) // 2], 2)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            f.write("# tools/stream_bench.py: device us per block (graph replay, HIP events; min and median of %d rounds "
                    "of %d replays), new engine vs the existing chain (5 x rv_linear_fp32 + rv_reparameterize) on the "
                    "same rows, alternating in one process; host wall per replay of the new graph (enqueue only)\n"
                    % (a.rounds, a.iters))
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
