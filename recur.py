"""`python recur.py motifs   --checkpoint C --in in.wav --hop 256 --window-frames 32 --top 5 --out motifs.json
        [--against other.wav] [--profile p.npy]`
`python recur.py discords --checkpoint C --in in.wav --hop 256 --window-frames 32 --top 5 --out discords.json`
`python recur.py loop     --checkpoint C --in in.wav --hop 256 --window-frames 16 --min-seconds 1 --max-seconds 8
        --repeats 4 --out out.wav`

What repeats in a recording, in the latent space (rawaudiovae_kelsey_amd.recur): the matrix profile of its mu rows on the
GPU.

motifs    the stretches of --window-frames frames that occur again, nearest pair first: for each both positions in
          seconds, the distance (the sum of the frame distances along the window) and the distance per frame, printed
          and written to one JSON object.  --against other.wav looks for the stretches of in.wav in other.wav instead of
          in in.wav itself.
discords  the same form for the stretches that have no counterpart: the greatest distance first.
loop      finds where the recording can be cut so that it loops without a seam -- the window at the loop's start recurs
          at its end, --min-seconds to --max-seconds later -- prints the loop points and writes the recording with the
          loop played --repeats times, the seams mixed in the latent space and resynthesised.
  --window-frames M  the window in frames (1 to 256; default 32, loop: 16)
  --top K            how many to report (default 5)
  --exclude E        frames around a match that cannot match again (default: the window)
  --window W         the synthesis window of loop: none | hann (default none)
  --profile F.npy    also write the profile P [windows] float64

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

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, flagged, int_at_least, load_wav, number_flag,  # noqa: E402
                                             open_model, positive, window_flag)

COMMANDS = ("motifs", "discords", "loop")


def parse_args(argv=None):
    from rawaudiovae_kelsey_amd.recur import M_MAX
    p = argparse.ArgumentParser(description="Latent recurrence: motifs, discords and loop points on the GPU")
    sub = p.add_subparsers(dest="command")
    for name in COMMANDS:
        s = sub.add_parser(name)
        add_model_flags(s)
        s.add_argument("--in", dest="wav", required=True, help="the wav to search")
        s.add_argument("--window-frames", default="16" if name == "loop" else "32", help="the window in frames")
        s.add_argument("--out", required=True, help="motifs, discords: the .json; loop: the wav")
        s.add_argument("--profile", default=None, help="also write the profile as .npy")
        if name == "loop":
            s.add_argument("--min-seconds", default="1", help="the shortest loop (default 1)")
            s.add_argument("--max-seconds", default="8", help="the longest loop (default 8)")
            s.add_argument("--repeats", default="4", help="how often the loop is played (default 4)")
            s.add_argument("--window", default="none", help="none | hann")
        else:
            s.add_argument("--top", default="5", help="how many to report (default 5)")
            s.add_argument("--exclude", default=None, help="frames around a match that cannot match again")
            s.add_argument("--against", default=None, help="search this wav for the stretches of --in")
    args = p.parse_args(argv)
    if args.command is None:
        raise ValueError("expected a command: motifs, discords or loop")
    int_at_least(args, "hop", 1)
    int_at_least(args, "window-frames", 1)
    if args.window_frames > M_MAX:
        raise ValueError("--window-frames %d: at most %d frames" % (args.window_frames, M_MAX))
    if args.command == "loop":
        for flag in ("min-seconds", "max-seconds"):
            number_flag(args, flag, float, positive, "a finite number of seconds > 0")
        if args.min_seconds > args.max_seconds:
            raise ValueError("--min-seconds %g: above --max-seconds %g" % (args.min_seconds, args.max_seconds))
        int_at_least(args, "repeats", 1)
        window_flag(args)
        if args.window is not None and args.hop is None:
            raise ValueError("--window %s: needs --hop (without one the frames are concatenated)" % args.window)
    else:
        int_at_least(args, "top", 1)
        int_at_least(args, "exclude", 0)
    return args


def _setup(args):
    from rawaudiovae_kelsey_amd.recur import LatentLooper
    cfg, model, step = open_model(args)
    return cfg, step, LatentLooper(model)


def _save_profile(args, rec):
    if args.profile is not None:
        np.save(args.profile, rec.P)


def run_picks(args):
    cfg, step, looper = _setup(args)
    sr, m = cfg["sampling_rate"], args.window_frames
    wave = load_wav(args.wav, sr)
    other = None if args.against is None else load_wav(args.against, sr)
    rec = flagged("--in / --against / --window-frames",
                   lambda: looper.profile(wave, args.hop, m, other, args.exclude, sampling_rate=sr))
    found = rec.motifs(args.top) if args.command == "motifs" else rec.discords(args.top)
    report = dict(command=args.command, windows=rec.T, window_frames=m, hop=step, sampling_rate=sr, exclude=rec.exclude,
                  against=args.against,
                  found=[dict(frame=i, match_frame=j, seconds=rec.seconds(i), match_seconds=rec.seconds(j), distance=d,
                              distance_per_frame=d / m) for i, j, d in found])
    with open(args.out, "w") as f:
        json.dump(report, f)
    _save_profile(args, rec)
    for e in report["found"]:
        print("%s at %.6g s, nearest at %.6g s: distance %.9g, per frame %.9g"
              % (args.command[:-1], e["seconds"], e["match_seconds"], e["distance"], e["distance_per_frame"]))
    print(json.dumps(report))
    return report


def run_loop(args):
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd.mosaic import check_window
    cfg, step, looper = _setup(args)
    sr, m = cfg["sampling_rate"], args.window_frames
    flagged("--window %s" % args.window, lambda: check_window(cfg["segment_length"], step, args.window))
    # whole frames inside [min, max] seconds; the 1e-9 keeps a bound that is a whole number of frames on its frame
    lo, hi = int(np.ceil(args.min_seconds * sr / step - 1e-9)), int(np.floor(args.max_seconds * sr / step + 1e-9))
    if lo < m:
        raise ValueError("--min-seconds %g: %d frames, shorter than the seam of --window-frames %d" % (args.min_seconds, lo, m))
    if hi < lo:
        raise ValueError("--max-seconds %g: no whole number of frames between it and --min-seconds %g"
                         % (args.max_seconds, args.min_seconds))
    wave = load_wav(args.wav, sr)
    loop = flagged("--in / --window-frames", lambda: looper.find(wave, args.hop, m, lo, hi, sr))
    if loop is None:
        raise ValueError("--in %r: no loop of %g to %g seconds (the recording is too short or holds NaN)"
                         % (args.wav, args.min_seconds, args.max_seconds))
    y = looper.render(wave, loop, args.repeats, args.hop, args.window).cpu().numpy()
    D.write_wav(args.out, y, sr)
    _save_profile(args, loop.recurrence)
    report = dict(command="loop", start_frame=loop.start_frame, end_frame=loop.end_frame, start_sample=loop.start_sample,
                  end_sample=loop.end_sample, start_seconds=loop.start_seconds, end_seconds=loop.end_seconds,
                  seconds=loop.seconds, distance=loop.distance, distance_per_frame=loop.distance / m, window_frames=m,
                  hop=step, repeats=args.repeats, samples=int(y.size), sampling_rate=sr)
    print("loop from %.6g s to %.6g s (%.6g s), distance %.9g; wrote %s: %d samples, the loop %d times"
          % (loop.start_seconds, loop.end_seconds, loop.seconds, loop.distance, args.out, y.size, args.repeats))
    print(json.dumps(report))
    return report


def main(argv=None):
    args = parse_args(argv)
    return (run_loop if args.command == "loop" else run_picks)(args)


if __name__ == "__main__":
    main()
