"""`python segment.py find  --checkpoint C --in in.wav --hop 256 --kernel 32 --gap 16 --delta 0.5 --out segments.json
        [--novelty nov.npy]`
`python segment.py split --segments segments.json --in in.wav --out-dir DIR`

Structure of a recording in the latent space (rawaudiovae_kelsey_amd.structure): where the sound changes, on the GPU.

find   encodes in.wav, slides a checkerboard kernel of half-width --kernel frames along the diagonal of the banded
       self-distance matrix of its mu rows and picks the boundaries from the novelty curve.  It prints the number of
       segments, every boundary in seconds and the form (for example A B A C: segments with the same letter resemble
       each other) and writes the same to one JSON object: boundaries in frames, samples and seconds, the segments'
       sample offsets and the labels.
  --kernel R         half-width of the kernel in frames (default 32, at most 512)
  --sigma X          width of the kernel's Gaussian taper as a fraction of R (default 0.5; none: no taper)
  --gap G            minimum gap between two boundaries in frames (default 16)
  --mean-radius M    radius of the local mean a boundary has to exceed (default 2 R)
  --delta D          ... by D times the mean |novelty| (default 0.5)
  --similar X        a segment takes the label of its nearest earlier segment when their distance is at most X times
                     the mean distance of adjacent segments (default 0.5)
  --novelty F.npy    also write the novelty curve [frames] float64
split  writes one wav per segment of segments.json into DIR (seg_000_A.wav, ...), cut at the boundaries' sample
       offsets, on the host; the files concatenate to in.wav.

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

COMMANDS = ("find", "split")


def parse_args(argv=None):
    from rawaudiovae_kelsey_amd.structure import PEAK_MAX, R_MAX
    p = argparse.ArgumentParser(description="Latent structure analysis: novelty, boundaries and segments on the GPU")
    sub = p.add_subparsers(dest="command")
    s = sub.add_parser("find")
    add_model_flags(s)
    s.add_argument("--in", dest="wav", required=True, help="the wav to segment")
    s.add_argument("--kernel", default="32", help="half-width of the kernel in frames (default 32)")
    s.add_argument("--sigma", default="0.5", help="taper width as a fraction of the kernel, or none (default 0.5)")
    s.add_argument("--gap", default="16", help="minimum gap between boundaries in frames (default 16)")
    s.add_argument("--mean-radius", default=None, help="radius of the local mean in frames (default: two kernels)")
    s.add_argument("--delta", default="0.5", help="threshold above the local mean, in mean |novelty| (default 0.5)")
    s.add_argument("--similar", default="0.5", help="label threshold, in mean adjacent distances (default 0.5)")
    s.add_argument("--out", required=True, help="the .json")
    s.add_argument("--novelty", default=None, help="also write the novelty curve as .npy")
    s = sub.add_parser("split")
    s.add_argument("--segments", required=True, help="the .json of find")
    s.add_argument("--in", dest="wav", required=True, help="the wav it was made from")
    s.add_argument("--out-dir", required=True, help="directory of the segment wavs")
    args = p.parse_args(argv)
    if args.command is None:
        raise ValueError("expected a command: find or split")
    if args.command == "find":
        int_at_least(args, "hop", 1)
        int_at_least(args, "kernel", 1)
        if args.kernel > R_MAX:
            raise ValueError("--kernel %d: at most %d frames" % (args.kernel, R_MAX))
        int_at_least(args, "gap", 0)
        int_at_least(args, "mean-radius", 0)
        for name, v in (("gap", args.gap), ("mean-radius", args.mean_radius)):
            if v is not None and v > PEAK_MAX:
                raise ValueError("--%s %d: at most %d frames" % (name, v, PEAK_MAX))
        args.sigma = None if args.sigma.lower() == "none" else args.sigma
        positive_real(args, "sigma")
        nonneg_real(args, "delta")
        nonneg_real(args, "similar")
    return args


def run_find(args):
    from rawaudiovae_kelsey_amd.structure import LatentSegmenter
    cfg, step = model_config(args)
    sr = cfg["sampling_rate"]
    wave = load_wav(args.wav, sr)
    seg = LatentSegmenter(load_model(args.checkpoint, cfg)).segment(
        wave, args.hop, args.kernel, args.sigma, args.gap, args.mean_radius, args.delta, args.similar, sr)
    frames, samples = seg.boundary_frames, seg.boundary_samples
    report = dict(segments=seg.F, frames=seg.T, samples=int(wave.size), sampling_rate=sr,
                  hop=step, kernel=args.kernel, band=seg.band,
                  boundary_frames=[int(v) for v in frames], boundary_samples=[int(v) for v in samples],
                  boundary_seconds=[float(v) for v in seg.boundary_seconds],
                  sample_offsets=[int(v) for v in seg.sample_offsets], labels=[int(v) for v in seg.labels], form=seg.form)
    with open(args.out, "w") as f:
        json.dump(report, f)
    if args.novelty is not None:
        np.save(args.novelty, seg.novelty.cpu().numpy())
    print("%d segments, boundaries at %s s, form %s" % (
        seg.F, " ".join("%.6g" % v for v in report["boundary_seconds"]) or "-", seg.form))
    print(json.dumps(report))
    return report


def run_split(args):
    from rawaudiovae_kelsey_amd import data as D
    try:
        with open(args.segments) as f:
            report = json.load(f)
        offsets, labels, sr = report["sample_offsets"], report["labels"], int(report["sampling_rate"])
    except (OSError, ValueError, KeyError, TypeError) as e:
        raise ValueError("--segments %r: not a segments file of find (%s)" % (args.segments, e))
    wave = load_wav(args.wav, sr)
    if (len(offsets) != len(labels) + 1 or offsets[0] != 0 or offsets[-1] != wave.size
            or any(b <= a for a, b in zip(offsets, offsets[1:]))):
        raise ValueError("--segments %r: its offsets do not cut the %d samples of --in %r" % (args.segments, wave.size, args.wav))
    os.makedirs(args.out_dir, exist_ok=True)
    from rawaudiovae_kelsey_amd.structure import form
    names = []
    for f, (a, b) in enumerate(zip(offsets, offsets[1:])):
        name = os.path.join(args.out_dir, "seg_%03d_%s.wav" % (f, form([labels[f]])))
        D.write_wav(name, wave[a:b], sr)
        names.append(name)
    print("wrote %d segments to %s" % (len(names), args.out_dir))
    return names


def main(argv=None):
    args = parse_args(argv)
    return {"find": run_find, "split": run_split}[args.command](args)


if __name__ == "__main__":
    main()
