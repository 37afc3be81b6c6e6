"""`python restore.py fill --checkpoint ckpt_00500 --walk walk.npz --in in.wav --out out.wav --hop 256 --window hann
        (--gaps 1.20:1.35,4.0:4.1 | --gaps-json F | --detect-zeros 64) [--noise 1e-2 --context 32 --fade 64]`
`python restore.py smooth --checkpoint ckpt_00500 --walk walk.npz --in in.wav --out out.wav --hop 256 --window hann --noise 0.5`
`python restore.py surprise --checkpoint ckpt_00500 --walk walk.npz --in in.wav --hop 256 --out surprise.npy [--threshold 4]`

Repair a damaged recording with the corpus model of generate.py (rawaudiovae_kelsey_amd.smooth), on the GPU.

fill replaces the damaged spans of the wav by the most probable latent trajectory under the walk, given the frames
around them (a Kalman filter and a fixed-interval smoother), decoded, overlap-added and cross-faded into the original:
everything further than --fade samples from a gap is the input bit for bit.  It prints the gaps it repaired, in seconds
and frames, and warns when a gap is longer than --context frames: across a long gap the posterior mean relaxes to the
corpus centre, so the fill grows bland.

  --gaps S:E,...     the damaged spans in seconds
  --gaps-json F      the same from a JSON list of [start, end] pairs in seconds
  --detect-zeros N   every run of at least N exactly-zero samples is a gap (dropouts, lost packets)
  --noise R          observation noise of a good frame in whitened units (default 1e-2; 1e-8 .. 1e8)
  --context N        good frames on each side of a gap that take part (default 32)
  --fade N           cross-fade samples on either side of a gap (default 64)

smooth treats every frame as a noisy observation (--noise is then the strength of the smoothing) and resynthesises the
whole file from the smoothed latents.  surprise writes nis / k per frame from the filter alone (about 1 where the
recording moves as the corpus does) as a .npy and prints the frames above --threshold: damaged frames nobody marked.

--hop must be the hop the walk was fitted at.  Bad flag values raise ValueError naming the flag.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, check_exists, check_fitted, finite, load_model,  # noqa: E402
                                             load_wav, nonneg_int, number_flag, positive_int, read_model_config,
                                             window_flag)

COMMANDS = ("fill", "smooth", "surprise")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Restore damaged audio with a fitted latent walk on the GPU")
    sub = p.add_subparsers(dest="command")
    for name in COMMANDS:
        s = sub.add_parser(name)
        add_model_flags(s, hop_help="frame hop: the hop the walk was fitted at")
        s.add_argument("--walk", required=True, help="the .npz written by generate.py fit")
        s.add_argument("--in", dest="wav", required=True, help="the damaged wav")
        s.add_argument("--out", required=True, help="fill, smooth: the output wav; surprise: the .npy")
        s.add_argument("--noise", default="0.5" if name == "smooth" else "1e-2", help="observation noise, 1e-8 .. 1e8")
        if name != "surprise":
            s.add_argument("--window", default="none", help="none | hann")
        if name == "fill":
            s.add_argument("--gaps", default=None, help="S:E,... in seconds")
            s.add_argument("--gaps-json", dest="gaps_json", default=None, help="a JSON list of [start, end] in seconds")
            s.add_argument("--detect-zeros", dest="detect_zeros", default=None, help="minimum run of zero samples")
            s.add_argument("--context", default="32", help="good frames on each side of a gap")
            s.add_argument("--fade", default="64", help="cross-fade samples on either side of a gap")
        if name == "surprise":
            s.add_argument("--threshold", default="4", help="print the frames whose nis / k exceeds it")
    args = p.parse_args(argv)
    if args.command is None:
        raise ValueError("expected a command: fill, smooth or surprise")
    positive_int(args, "hop")
    number_flag(args, "noise", float, finite(1e-8, 1e8), "a finite number in [1e-8, 1e8]")
    if args.command != "surprise":
        window_flag(args)
    if args.command == "fill":
        given = [f for f in ("gaps", "gaps_json", "detect_zeros") if getattr(args, f) is not None]
        if len(given) != 1:
            raise ValueError("expected exactly one of --gaps, --gaps-json and --detect-zeros, got %s" % (
                ", ".join("--" + f.replace("_", "-") for f in given) or "none"))
        positive_int(args, "detect-zeros")
        positive_int(args, "context")
        nonneg_int(args, "fade")
    if args.command == "surprise":
        number_flag(args, "threshold", float, finite(0.0, float("inf")), "a non-negative number")
    return args


def gap_ranges(args, wave, sampling_rate):
    """The damaged sample ranges of a fill: --gaps, --gaps-json or --detect-zeros; ValueError naming the flag."""
    from rawaudiovae_kelsey_amd import smooth as SM
    if args.detect_zeros is not None:
        runs = SM.zero_runs(wave, args.detect_zeros)
        if not runs:
            raise ValueError("--detect-zeros %d: %r holds no run of %d zero samples" % (
                args.detect_zeros, args.wav, args.detect_zeros))
        return runs
    if args.gaps is not None:
        try:
            return SM.parse_ranges(args.gaps, sampling_rate)
        except ValueError as e:
            raise ValueError("--gaps: %s" % e)
    try:
        with open(args.gaps_json) as f:
            pairs = json.load(f)
        return SM.parse_ranges(",".join("%r:%r" % (float(a), float(b)) for a, b in pairs), sampling_rate)
    except (OSError, TypeError, ValueError) as e:
        raise ValueError("--gaps-json %r: %s" % (args.gaps_json, e))


def _load(args):
    from rawaudiovae_kelsey_amd import walk as W
    cfg = read_model_config(args.config)
    for flag, path in (("walk", args.walk), ("in", args.wav)):
        check_exists(flag, path)
    model = load_model(args.checkpoint, cfg)
    walk, meta = W.read_walk(args.walk, model.fc1.weight.device)
    hop = check_fitted("walk", args.walk, meta, cfg, args.hop)
    return cfg, model, walk, load_wav(args.wav, cfg["sampling_rate"]), hop


def fill(args):
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import smooth as SM
    cfg, model, walk, wave, hop = _load(args)
    sr, S = cfg["sampling_rate"], cfg["segment_length"]
    try:
        rg = SM.check_ranges(gap_ranges(args, wave, sr), len(wave))
    except ValueError as e:
        raise ValueError(str(e) if str(e).startswith("--") else "--gaps: %s" % e)
    try:
        out = SM.restore(model, walk, wave, rg, hop, args.window, args.noise, args.context, args.fade)
    except ValueError as e:
        raise ValueError("--context %d / --fade %d / --window %s: %s" % (args.context, args.fade, args.window or "none", e))
    out = out.cpu().numpy()
    D.write_wav(args.out, out, sr)
    report = []
    for s, e in rg.tolist():
        mask = SM.frame_mask(len(wave), S, hop, [(s, e)])
        frames = np.flatnonzero(mask)
        f0, f1 = int(frames[0]), int(frames[-1]) + 1
        report.append(dict(start=s / sr, end=e / sr, samples=[s, e], frames=[f0, f1]))
        print("repaired %.4f s .. %.4f s (samples %d .. %d, frames %d .. %d)" % (s / sr, e / sr, s, e, f0, f1))
        if f1 - f0 > args.context:
            print("warning: this gap spans %d frames, more than --context %d: across a long gap the fill relaxes to the "
                  "corpus centre and grows bland" % (f1 - f0, args.context), file=sys.stderr)
    print("wrote %s: %d samples, %d gaps, hop %d, window %s, noise %g" % (args.out, out.size, len(report), hop,
                                                                       args.window or "none", args.noise))
    return out, report


def smooth(args):
    import torch
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import smooth as SM
    from rawaudiovae_kelsey_amd.mosaic import check_window, ola
    from rawaudiovae_kelsey_amd.stream import window_values
    cfg, model, walk, wave, hop = _load(args)
    S = cfg["segment_length"]
    try:
        check_window(S, hop, args.window)
    except ValueError as e:
        raise ValueError("--window %s: %s" % (args.window or "none", e))
    with torch.no_grad():
        codec, w, mu, n_frames, n_padded = SM._encode(model, walk, wave, hop)
        z, _ = SM.LatentSmoother(walk, args.noise).smooth(mu, np.asarray([0, n_frames], dtype=np.int64))
        win = None if args.window is None else torch.from_numpy(window_values(S, args.window)).to(mu.device)
        out = ola(codec.decode(z), hop, n_padded, win)[:w.numel()].cpu().numpy()
    D.write_wav(args.out, out, cfg["sampling_rate"])
    print("wrote %s: %d samples, %d frames smoothed, hop %d, window %s, noise %g" % (
        args.out, out.size, n_frames, hop, args.window or "none", args.noise))
    return out


def surprise(args):
    from rawaudiovae_kelsey_amd import smooth as SM
    cfg, model, walk, wave, hop = _load(args)
    s = SM.surprise(model, walk, wave, hop, args.noise).cpu().numpy()
    np.save(args.out, s)
    sr = cfg["sampling_rate"]
    for f in np.flatnonzero(s > args.threshold):
        print("frame %d (%.4f s): %.3f" % (f, f * hop / sr, s[f]))
    print("wrote %s: %d frames, %d above %g" % (args.out, s.size, int((s > args.threshold).sum()), args.threshold))
    return s


def main(argv=None):
    args = parse_args(argv)
    return dict(fill=fill, smooth=smooth, surprise=surprise)[args.command](args)


if __name__ == "__main__":
    main()
