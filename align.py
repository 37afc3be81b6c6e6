"""`python align.py path  --checkpoint C --a a.wav --b b.wav --hop 256 [--band 200] [--penalty 0] --out align.npz`
`python align.py morph --checkpoint C --a a.wav --b b.wav --hop 256 --window hann --alpha 0:1 | --curve file.npy
        --timeline a --out out.wav`
`python align.py find  --checkpoint C --query q.wav --in long.wav --hop 256 --out match.json`

Time alignment of two recordings in the latent space (rawaudiovae_kelsey_amd.align): dynamic time warping over the
encoder's mu rows, on the GPU.

path   aligns a.wav and b.wav and writes one .npz: path [P, 2] int32 (frame of a, frame of b), cost, path_cost, band,
       hop, segment_length.  It prints P, the cost and the cost per step.
morph  interpolates between the two sounds ALONG the warping path, so that event k of a meets event k of b:
  --alpha A0:A1      alpha runs linearly from A0 at the first output frame to A1 at the last (a two-point curve)
  --curve file.npy   a float64 control curve of >= 2 points, stretched to the output frames
  --timeline a|b|path   one output frame per frame of a (default), of b, or per step of the path
  --window none|hann overlap-add window at --hop
find   subsequence search: where in --in the whole of --query occurs.  It writes and prints one JSON object: start / end
       in frames, samples and seconds, and the cost.

  --band N           keep the cells within N frames of the straight line (default: the whole matrix)
  --penalty P        cost added to every non-diagonal step (default 0)

Bad flag values raise ValueError naming the flag.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, flagged, int_at_least, load_model, load_wav,  # noqa: E402
                                             model_config, nonneg_real, window_flag)

COMMANDS = ("path", "morph", "find")


def parse_alpha(spec):
    """'A0:A1' -> the float64 two-point curve [A0, A1]; ValueError naming --alpha."""
    try:
        a0, a1 = (float(v) for v in spec.split(":"))
        if not (np.isfinite(a0) and np.isfinite(a1)):
            raise ValueError
    except ValueError:
        raise ValueError("--alpha %r: expected START:END, two finite numbers" % (spec,))
    return np.array([a0, a1], dtype=np.float64)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Time-aligned latent morphing: DTW of two recordings on the GPU")
    sub = p.add_subparsers(dest="command")
    for name in COMMANDS:
        s = sub.add_parser(name)
        add_model_flags(s)
        s.add_argument("--penalty", default="0", help="cost of a non-diagonal step (default 0)")
        s.add_argument("--out", required=True, help="path: the .npz; morph: the wav; find: the .json")
        if name == "find":
            s.add_argument("--query", required=True, help="the wav to look for")
            s.add_argument("--in", dest="recording", required=True, help="the wav to look in")
        else:
            s.add_argument("--a", required=True, help="first wav")
            s.add_argument("--b", required=True, help="second wav")
            s.add_argument("--band", default=None, help="band half-width in frames (default: the whole matrix)")
        if name == "morph":
            s.add_argument("--alpha", default=None, help="START:END, alpha from the first to the last output frame")
            s.add_argument("--curve", default=None, help=".npy float64 control curve")
            s.add_argument("--timeline", default="a", help="a | b | path")
            s.add_argument("--window", default="none", help="none | hann")
            s.add_argument("--seed", default="0", help="Philox seed of the reparameterisation")
    args = p.parse_args(argv)
    if args.command is None:
        raise ValueError("expected a command: path, morph or find")
    int_at_least(args, "hop", 1)
    nonneg_real(args, "penalty")
    if args.command != "find":
        int_at_least(args, "band", 0)
    if args.command == "morph":
        if (args.alpha is None) == (args.curve is None):
            raise ValueError("--alpha / --curve: expected exactly one of the two")
        if args.timeline not in ("a", "b", "path"):
            raise ValueError("--timeline %r: expected a, b or path" % args.timeline)
        window_flag(args)
        if args.window is not None and args.hop is None:
            raise ValueError("--window %s: needs --hop (without one the frames are concatenated)" % args.window)
        int_at_least(args, "seed", 0)
        args.curve_values = parse_alpha(args.alpha) if args.alpha is not None else None
    return args


def load_curve(path):
    """The float64 control curve of --curve; ValueError naming the flag."""
    try:
        c = np.load(path)
    except Exception as e:
        raise ValueError("--curve %r: unreadable .npy (%s)" % (path, e))
    if c.ndim != 1 or c.size < 2 or c.dtype.kind != "f":
        raise ValueError("--curve %r: expected a 1-D float array of at least 2 points, got %s %s" % (path, c.dtype, c.shape))
    return np.ascontiguousarray(c, dtype=np.float64)


def run_path(args):
    from rawaudiovae_kelsey_amd.align import LatentAligner
    cfg, _ = model_config(args)
    a, b = load_wav(args.a, cfg["sampling_rate"]), load_wav(args.b, cfg["sampling_rate"])
    aligner = LatentAligner(load_model(args.checkpoint, cfg))
    al = flagged("--a / --b / --band", lambda: aligner.align(a, b, args.hop, args.band, args.penalty))
    path = al.path.cpu().numpy()
    with open(args.out, "wb") as f:
        np.savez(f, path=path, cost=al.cost, path_cost=al.path_cost, band=-1 if al.band is None else al.band,
                 hop=-1 if args.hop is None else args.hop, segment_length=cfg["segment_length"], frames_a=al.Ta, frames_b=al.Tb)
    print("wrote %s: %d steps through %d x %d frames, cost %.9g, cost per step %.9g, band %s, penalty %g"
          % (args.out, al.P, al.Ta, al.Tb, al.cost, al.normalised_cost, al.band, args.penalty))
    return al


def run_morph(args):
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd.align import AlignedInterpolator
    from rawaudiovae_kelsey_amd.mosaic import check_window
    cfg, step = model_config(args)
    flagged("--window %s" % args.window, lambda: check_window(cfg["segment_length"], step, args.window))
    curve = args.curve_values if args.curve is None else load_curve(args.curve)
    a, b = load_wav(args.a, cfg["sampling_rate"]), load_wav(args.b, cfg["sampling_rate"])
    it = AlignedInterpolator(load_model(args.checkpoint, cfg))
    y = flagged("--a / --b / --band", lambda: it.curve(a, b, curve, hop=args.hop, window=args.window,
                                                         timeline=args.timeline, band=args.band, penalty=args.penalty,
                                                         seed=args.seed))
    y = y.cpu().numpy()
    D.write_wav(args.out, y, cfg["sampling_rate"])
    al = it.last_alignment
    print("wrote %s: %d samples on timeline %s, %d steps through %d x %d frames, cost %.9g, hop %s, window %s"
          % (args.out, y.size, args.timeline, al.P, al.Ta, al.Tb, al.cost, args.hop, args.window or "none"))
    return y


def run_find(args):
    from rawaudiovae_kelsey_amd.align import LatentAligner
    cfg, _ = model_config(args)
    sr = cfg["sampling_rate"]
    q, rec = load_wav(args.query, sr), load_wav(args.recording, sr)
    aligner = LatentAligner(load_model(args.checkpoint, cfg))
    m = flagged("--query / --in", lambda: aligner.find(q, rec, args.hop, args.penalty))
    report = dict(found=m.found, start_frame=m.start_frame, end_frame=m.end_frame, start_sample=m.start_sample,
                  end_sample=m.end_sample, start_seconds=m.start_sample / sr if m.found else None,
                  end_seconds=m.end_sample / sr if m.found else None, cost=m.cost if m.found else None,
                  steps=m.alignment.P)
    with open(args.out, "w") as f:
        json.dump(report, f)
    print(json.dumps(report))
    return report


def main(argv=None):
    args = parse_args(argv)
    return {"path": run_path, "morph": run_morph, "find": run_find}[args.command](args)


if __name__ == "__main__":
    main()
