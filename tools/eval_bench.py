#!/usr/bin/env python3
"""Time the evaluation scoring (csrc/eval.hip) at the reference's shape S = 1024, H = 2048, L = 256 on synthetic frames.

    python tools/eval_bench.py [--frames 65536] [--reps 50] [--trials 5] [--out build/eval_bench.json]

Per trial (after a warm-up of every timed call; the figures are the median over the trials, with the spread):
  frame_scores   one RV_EVAL_FRAMES launch over `frames` non-overlapping frames with the KL and spectral columns, device
                 events around `reps` back-to-back launches: frames/s, and the bytes/s it achieves against the bytes it
                 must read (x and y, 2 * 4 S = 8 KB per frame, plus mu and logvar, 8 L) over the HBM peak
  kl_dims        RV_EVAL_DIMS over the same latents
  encode+decode  the exact-fp32 inference path of the same frames (fc1, fc21, fc22, fc3, fc4: rv_linear_fp32)
  score          Evaluator.score of the waveform, whole (framing, encode, decode, both ops)
and the scoring launch's share of score()'s time.  At the default 65 536 frames one launch reads 672 MB, more than
twice the 256 MiB Infinity Cache, so back-to-back launches over the same buffers are served from HBM and the bytes/s
is an HBM rate; with fewer frames (under about 25 000) the buffers stay in the cache and it is a cache rate.
"""
import argparse
import json
import os
import platform
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd import evaluate as E  # noqa: E402
from rawaudiovae_kelsey_amd.synth import make_params  # noqa: E402

HBM_PEAK = 8.0e12    # bytes/s (MI355X)
S, H, L = 1024, 2048, 256


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


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--frames", type=int, default=65536)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--trials", type=int, default=5)
    p.add_argument("--out", default=os.path.join(REPO, "build", "eval_bench.json"))
    a = p.parse_args()
    from rawvae.model import VAE
    model = VAE(S, H, L).cuda().eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_params(S, H, L, 0).items()})
    T = a.frames
    g = torch.Generator(device="cuda").manual_seed(0)
    wave = torch.rand(T * S, device="cuda", generator=g) * 2 - 1
    ev = E.Evaluator(model, max_rows=T)
    with torch.no_grad():
        mu, lv = model.encode(wave.view(T, S))
        recon = model.decode(mu)
    out = torch.empty((T, 6), device="cuda")

    def scores():
        E.frame_scores(wave, recon, T, S, S, S, mu, lv, ev._spec.window, ev._spec.table, 60.0, out=out)

    def scores_time_only():
        E.frame_scores(wave, recon, T, S, S, S, mu, lv, dynamic_range=60.0, out=out)

    def dims():
        E.kl_dims(mu, lv)

    def codec():
        with torch.no_grad():
            model.decode(model.encode(wave.view(T, S))[0])

    def whole():
        ev.score(wave)

    calls = (("frame_scores", scores, a.reps), ("frame_scores_no_spectrum", scores_time_only, a.reps),
             ("kl_dims", dims, a.reps), ("encode_decode", codec, max(a.reps // 10, 3)), ("score", whole, max(a.reps // 10, 3)))
    ms = {k: [] for k, _, _ in calls}
    for _ in range(a.trials):
        for k, fn, reps in calls:
            ms[k].append(timed(fn, reps))
    res = dict(device=torch.cuda.get_device_name(0), host=platform.node(), torch=torch.__version__, hip=torch.version.hip,
               S=S, H=H, L=L, frames=T, reps=a.reps, trials=a.trials)
    for k, v in ms.items():
        res[k + "_ms"] = statistics.median(v)
        res[k + "_ms_spread"] = [min(v), max(v)]
    sec = res["frame_scores_ms"] * 1e-3
    must_read = T * (2 * 4 * S + 2 * 4 * L)
    res.update(frames_per_s=T / sec, bytes_read=must_read, bytes_per_s=must_read / sec,
               frac_hbm_peak=must_read / sec / HBM_PEAK, share_of_score=res["frame_scores_ms"] / res["score_ms"],
               encode_decode_share_of_score=res["encode_decode_ms"] / res["score_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("S=%d H=%d L=%d frames=%d: frame_scores %.3f ms [%.3f, %.3f] = %.3g frames/s, %.3g B/s (%.3f of HBM peak); "
          "without the spectrum %.3f ms; kl_dims %.3f ms; encode+decode %.3f ms; score() %.3f ms: scoring is %.3f of it"
          % (S, H, L, T, res["frame_scores_ms"], *res["frame_scores_ms_spread"], res["frames_per_s"], res["bytes_per_s"],
             res["frac_hbm_peak"], res["frame_scores_no_spectrum_ms"], res["kl_dims_ms"], res["encode_decode_ms"],
             res["score_ms"], res["share_of_score"]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
