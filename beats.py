"""`python beats.py find  --checkpoint C --in in.wav --hop 256 [--bpm 120|none --bpm-min 40 --bpm-max 240 --kernel 8
        --tightness 100 --octaves 1 --window-seconds 8 --meter 4 --onset o.npy --tempogram tg.npy] --out beats.json`
`python beats.py click --beats beats.json --in in.wav --out out.wav`

Beats of a recording in the latent space (rawaudiovae_kelsey_amd.beats): where its pulse falls and how fast it is, on the
GPU.

find   encodes in.wav, takes the novelty of its mu rows under a small kernel as an onset-strength curve, finds the period
       its windowed autocorrelation prefers and places the beats by dynamic programming.  It prints the tempo, the number of
       beats and how regular their intervals are, and writes one JSON object: the beats in frames, samples and seconds,
       `period`, `bpm` and `bpm_over_time` (one value per tempogram window), and `sample_offsets` with `labels` (the beat's
       index mod --meter; the stretch before the first beat a piece of its own), which `segment.py split --segments
       beats.json` takes as they are to cut the recording at its beats.
  --bpm B            the tempo the prior is centred on (default 120; none: no prior, every period weighs the same)
  --octaves X        width of the prior in octaves (default 1)
  --bpm-min, --bpm-max   the tempi looked at (default 40 to 240); a --bpm-min whose period is over 1024 frames is refused
  --kernel R         half-width of the novelty kernel in frames (default 8, at most 512)
  --tightness X      how strongly the tracker holds the beats to the period (default 100)
  --window-seconds S length of a tempogram window (default 8; windows start every second)
  --meter M          beats to a bar, for the labels (default 4)
  --onset F.npy      also write the onset curve [frames] float64
  --tempogram F.npy  also write the tempogram [windows, periods] float64
click  mixes a short decaying burst into in.wav at every beat of beats.json, on the host; out.wav has in.wav's length.

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

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, int_at_least, load_model, load_wav, model_config,  # noqa: E402
                                             nonneg_real, positive_real)

COMMANDS = ("find", "click")
CLICK_HZ, CLICK_SECONDS, CLICK_GAIN = 1000.0, 0.03, 0.5


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Latent beat tracking: onset curve, tempo and beats on the GPU")
    sub = p.add_subparsers(dest="command")
    s = sub.add_parser("find")
    add_model_flags(s)
    s.add_argument("--in", dest="wav", required=True, help="the wav to track")
    s.add_argument("--bpm", default="120", help="centre of the tempo prior, or none (default 120)")
    s.add_argument("--octaves", default="1", help="width of the tempo prior in octaves (default 1)")
    s.add_argument("--bpm-min", default="40", help="slowest tempo looked at (default 40)")
    s.add_argument("--bpm-max", default="240", help="fastest tempo looked at (default 240)")
    s.add_argument("--kernel", default="8", help="half-width of the novelty kernel in frames (default 8)")
    s.add_argument("--tightness", default="100", help="weight of the tracker's transition scores (default 100)")
    s.add_argument("--window-seconds", default="8", help="length of a tempogram window (default 8)")
    s.add_argument("--meter", default="4", help="beats to a bar, for the labels (default 4)")
    s.add_argument("--out", required=True, help="the .json")
    s.add_argument("--onset", default=None, help="also write the onset curve as .npy")
    s.add_argument("--tempogram", default=None, help="also write the tempogram as .npy")
    s = sub.add_parser("click")
    s.add_argument("--beats", required=True, help="the .json of find")
    s.add_argument("--in", dest="wav", required=True, help="the wav it was made from")
    s.add_argument("--out", required=True, help="the wav with the clicks")
    args = p.parse_args(argv)
    if args.command is None:
        raise ValueError("expected a command: find or click")
    if args.command == "find":
        from rawaudiovae_kelsey_amd.structure import R_MAX
        int_at_least(args, "hop", 1)
        int_at_least(args, "kernel", 1)
        if args.kernel > R_MAX:
            raise ValueError("--kernel %d: at most %d frames" % (args.kernel, R_MAX))
        args.bpm = None if args.bpm.lower() == "none" else args.bpm
        for flag in ("bpm", "octaves", "bpm-min", "bpm-max", "window-seconds"):
            positive_real(args, flag)
        if args.bpm_min > args.bpm_max:
            raise ValueError("--bpm-min %g: above --bpm-max %g" % (args.bpm_min, args.bpm_max))
        nonneg_real(args, "tightness")
        int_at_least(args, "meter", 1)
    return args


def tempogram_plan(args, sr, step):
    """(lags, window, window_hop, centre) in frames from the flags, the sampling rate and the frame step; ValueError
    naming the flag."""
    from rawaudiovae_kelsey_amd import beats as B
    try:
        lags = B.lag_range(args.bpm_min, args.bpm_max, sr, step)
    except ValueError as e:
        raise ValueError("--bpm-min %g --bpm-max %g: %s" % (args.bpm_min, args.bpm_max, e))
    fps = float(sr) / float(step)
    window = max(1, int(round(args.window_seconds * fps)))
    if window > B.W_MAX:
        raise ValueError("--window-seconds %g: %d frames, at most %d (%.6g s at this hop)" % (
            args.window_seconds, window, B.W_MAX, B.W_MAX / fps))
    centre = None if args.bpm is None else 60.0 * fps / args.bpm
    return lags, window, max(1, int(round(fps))), centre


def report_of(beats, meter, hop):
    """The JSON object of find from a Beats with its framing."""
    offsets, labels = beats.segments(meter)
    mean, std = beats.intervals
    return dict(beats=beats.n_beats, frames=beats.T, samples=int(beats.n_samples), sampling_rate=beats.sampling_rate, hop=hop,
                kernel=beats.kernel, band=beats.band, meter=meter, period=beats.period, bpm=beats.bpm, silent=beats.silent,
                lags=list(beats.lags), window_hop=beats.window_hop, bpm_over_time=[float(v) for v in beats.bpm_over_time],
                beat_frames=[int(v) for v in beats.beat_frames], beat_samples=[int(v) for v in beats.beat_samples],
                beat_seconds=[float(v) for v in beats.beat_seconds], score=beats.score, interval_mean=mean, interval_std=std,
                sample_offsets=[int(v) for v in offsets], labels=[int(v) for v in labels])


def run_find(args):
    from rawaudiovae_kelsey_amd.beats import BeatTracker
    cfg, step = model_config(args)
    sr = cfg["sampling_rate"]
    lags, window, window_hop, centre = tempogram_plan(args, sr, step)
    wave = load_wav(args.wav, sr)
    beats = BeatTracker(load_model(args.checkpoint, cfg)).track(
        wave, args.hop, args.kernel, 0.5, lags, window, window_hop, centre, args.octaves, args.tightness, sr)
    report = report_of(beats, args.meter, step)
    with open(args.out, "w") as f:
        json.dump(report, f)
    if args.onset is not None:
        np.save(args.onset, beats.onset.cpu().numpy())
    if args.tempogram is not None:
        np.save(args.tempogram, beats.tempogram.cpu().numpy())
    if beats.silent:
        print("no pulse found: no period between %d and %d frames has a positive score; 0 beats" % lags)
    else:
        print("%.6g bpm (period %d frames), %d beats, interval %.6g +- %.6g frames" % (
            report["bpm"], beats.period, beats.n_beats, report["interval_mean"], report["interval_std"]))
    print(json.dumps(report))
    return report


def click_track(wave, beat_samples, sr):
    """wave [n] float32 with a burst of CLICK_HZ, CLICK_SECONDS long and decaying by 60 dB, added at every beat; the same
    length, clipped to [-1, 1]."""
    out = np.array(wave, dtype=np.float32)
    m = max(1, int(round(CLICK_SECONDS * sr)))
    t = np.arange(m) / float(sr)
    burst = (CLICK_GAIN * np.sin(2.0 * np.pi * CLICK_HZ * t) * np.exp(-t * (np.log(1000.0) / CLICK_SECONDS))).astype(np.float32)
    for b in beat_samples:
        if 0 <= b < out.size:
            k = min(m, out.size - b)
            out[b:b + k] += burst[:k]
    return np.clip(out, -1.0, 1.0)


def run_click(args):
    from rawaudiovae_kelsey_amd import data as D
    try:
        with open(args.beats) as f:
            report = json.load(f)
        at, sr, n = [int(v) for v in report["beat_samples"]], int(report["sampling_rate"]), int(report["samples"])
    except (OSError, ValueError, KeyError, TypeError) as e:
        raise ValueError("--beats %r: not a beats file of find (%s)" % (args.beats, e))
    wave = load_wav(args.wav, sr)
    if wave.size != n:
        raise ValueError("--beats %r: made from %d samples, --in %r has %d" % (args.beats, n, args.wav, wave.size))
    out = click_track(wave, at, sr)
    D.write_wav(args.out, out, sr)
    print("wrote %d clicks to %s" % (len(at), args.out))
    return out


def main(argv=None):
    args = parse_args(argv)
    return {"find": run_find, "click": run_click}[args.command](args)


if __name__ == "__main__":
    main()
