"""`python evaluate.py --config default.ini --checkpoint ckpt_00500 --data DIR_OR_WAV --out report.json`
`python evaluate.py --ref target.wav --test mosaic.wav --segment-length 1024 --hop 256 --out report.json`

Held-out evaluation on the GPU (rawaudiovae_kelsey_amd.evaluate).  The first form scores a checkpoint on a wav or on
every *.wav of a folder (sorted by name): each frame against its reconstruction through the exact-fp32 inference path.
The second scores one wav against another without a model (a mosaic or a resynthesis against its target).

  --hop N              frame hop (default: non-overlapping frames, the tail zero-padded, as the test set is framed)
  --window hann|none   window of the spectral figures (default hann; none: no spectral figures)
  --dynamic-range R    dB below the louder frame's peak bin at which the log-spectral distance floors (default 60)
  --sample             z = mu + eps * exp(logvar / 2) drawn on the device from --seed (default: z = mu, deterministic)
  --seed S             seed of the draw (default 0)
  --kl-beta B          weight of the KL term in `loss` (default: the .ini's kl_beta)
  --active-threshold X mean KL above which a latent dimension counts as active (default 0.01)
  --per-frame F.npz    also write the score matrix: scores [T, 6], columns, offsets [files + 1], names
  --sampling-rate SR   (second form) rate both wavs are read at (default: the reference wav's own)

The JSON is Evaluator.report's dict (first form) or compare's (second).  A figure that is infinite or undefined
(snr_db of identical waves, of silence) is written as Python's json module writes it, Infinity / NaN, which Python
reads back but strict JSON parsers refuse.  Bad flag values raise ValueError naming the flag.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd.frontend import (check_exists, data_files, load_model, load_wav, nonneg_int,  # noqa: E402
                                             nonneg_real, number_flag, positive_int, read_model_config, window_flag)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Score a checkpoint on held-out audio, or one wav against another, on the GPU")
    p.add_argument("--config", default=None, help="the training .ini (model shape, sampling_rate, kl_beta)")
    p.add_argument("--checkpoint", default=None, help="checkpoint dict (ckpt_NNNNN) or whole-module pickle (.pt)")
    p.add_argument("--data", default=None, help="a wav, or a folder whose *.wav are scored")
    p.add_argument("--ref", default=None, help="reference wav (model-free form)")
    p.add_argument("--test", default=None, help="wav scored against --ref")
    p.add_argument("--segment-length", default=None, help="frame length of the model-free form")
    p.add_argument("--out", required=True, help="the JSON report")
    p.add_argument("--hop", default=None)
    p.add_argument("--window", default="hann")
    p.add_argument("--dynamic-range", default="60")
    p.add_argument("--sample", action="store_true")
    p.add_argument("--seed", default=None)
    p.add_argument("--kl-beta", default=None)
    p.add_argument("--active-threshold", default="0.01")
    p.add_argument("--per-frame", default=None)
    p.add_argument("--sampling-rate", default=None)
    args = p.parse_args(argv)
    args.pair = args.ref is not None or args.test is not None
    if args.pair:
        for flag in ("ref", "test"):
            if getattr(args, flag) is None:
                raise ValueError("--%s: --ref and --test come together" % flag)
        for flag in ("checkpoint", "data", "config"):
            if getattr(args, flag) is not None:
                raise ValueError("--%s: not used when --ref / --test compare two wavs" % flag)
        if args.segment_length is None:
            raise ValueError("--segment-length: required with --ref / --test")
        if args.sample or args.seed is not None:
            raise ValueError("--%s: nothing is sampled when --ref / --test compare two wavs"
                             % ("sample" if args.sample else "seed"))
        if args.kl_beta is not None:
            raise ValueError("--kl-beta: two wavs have no KL term")
    else:
        for flag in ("checkpoint", "data"):
            if getattr(args, flag) is None:
                raise ValueError("--%s: required (or give --ref and --test)" % flag)
        for flag in ("segment_length", "sampling_rate"):
            if getattr(args, flag) is not None:
                raise ValueError("--%s: the model's .ini sets it; the flag belongs to --ref / --test"
                                 % flag.replace("_", "-"))
        if args.seed is not None and not args.sample:
            raise ValueError("--seed: only read with --sample")
        if args.config is None:
            args.config = "./default.ini"
    for flag in ("segment-length", "hop", "sampling-rate"):
        positive_int(args, flag)
    nonneg_int(args, "seed")
    number_flag(args, "dynamic-range", float, lambda x: 0 < x <= 120, "a number of dB in (0, 120]")
    nonneg_real(args, "kl-beta")
    nonneg_real(args, "active-threshold")
    window_flag(args)
    if args.sample and args.seed is None:
        args.seed = 0
    if args.pair:
        check_frames(args, args.segment_length)
    return args


def check_frames(args, segment_length):
    """The framing flags against the frame length; ValueError naming the flag."""
    from rawaudiovae_kelsey_amd.evaluate import SPECTRAL_S, check_args
    S = int(segment_length)
    if args.hop is not None and S % args.hop != 0:
        raise ValueError("--hop %d: must divide the frame length %d" % (args.hop, S))
    if args.window is not None and not (SPECTRAL_S[0] <= S <= SPECTRAL_S[1] and S & (S - 1) == 0):
        raise ValueError("--window %s: the spectral figures need a frame length that is a power of two in [%d, %d], "
                         "got %d (--window none scores without them)" % (args.window, SPECTRAL_S[0], SPECTRAL_S[1], S))
    check_args(S, args.hop, args.window, args.dynamic_range, 16384, args.active_threshold)


def write_per_frame(path, scores, offsets, names):
    from rawaudiovae_kelsey_amd.evaluate import COLUMNS
    np.savez(path, scores=np.asarray(scores, dtype=np.float32), columns=np.array(COLUMNS),
             offsets=np.asarray(offsets, dtype=np.int64), names=np.array([str(n) for n in names]))


def main(argv=None):
    args = parse_args(argv)
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import evaluate as E
    if args.pair:
        for flag in ("ref", "test"):
            check_exists(flag, getattr(args, flag))
        sr = args.sampling_rate or D.read_wav(args.ref)[1]
        ref, test = load_wav(args.ref, sr), load_wav(args.test, sr)
        report, scores = E.compare(ref, test, args.segment_length, args.hop, args.window, args.dynamic_range,
                                   return_scores=True)
        report.update(ref=str(args.ref), test=str(args.test), sampling_rate=int(sr))
        offsets, names = [0, report["frames"]], [str(args.test)]
    else:
        import configparser
        cfg = read_model_config(args.config)
        check_frames(args, cfg["segment_length"])
        files = data_files(args.data)
        if args.kl_beta is None:
            ini = configparser.ConfigParser(allow_no_value=True)
            ini.read(args.config)
            args.kl_beta = ini["VAE"].getfloat("kl_beta")
        model = load_model(args.checkpoint, cfg)
        ev = E.Evaluator(model, hop=args.hop, window=args.window, dynamic_range=args.dynamic_range,
                         active_threshold=args.active_threshold)
        for i, f in enumerate(files):
            ev.add(load_wav(f, cfg["sampling_rate"]), os.path.basename(f),
                   seed=None if not args.sample else args.seed + i)
        report = ev.report(args.kl_beta)
        report.update(checkpoint=str(args.checkpoint), sampling_rate=cfg["sampling_rate"], hop=args.hop,
                      sampled=bool(args.sample), seed=args.seed)
        scores, offsets, names = ev.scores, ev.offsets, ev.names
    report.update(segment_length=int(args.segment_length if args.pair else cfg["segment_length"]),
                  window=args.window or "none", dynamic_range=args.dynamic_range)
    with open(args.out, "w") as f:
        f.write(json.dumps(report, indent=1) + "\n")
    if args.per_frame is not None:
        write_per_frame(args.per_frame, scores.cpu().numpy(), offsets, names)
    print("wrote %s: %d frames, mse %.6g, snr %.2f dB, lsd %.2f dB" % (args.out, report["frames"], report["mse"],
                                                                       report["snr_db"], report["lsd_db"]))
    return report


if __name__ == "__main__":
    main()
