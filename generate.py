"""`python generate.py fit --config default.ini --checkpoint ckpt_00500 --data DIR_OR_WAV --hop 256 --keep 16 --out walk.npz`
`python generate.py run --config default.ini --checkpoint ckpt_00500 --walk walk.npz --seconds 10 --out out.wav
        --hop 256 --window hann --temperature 1 --seed 0`

New audio in the manner of a corpus: a fitted walk through the latent space (rawaudiovae_kelsey_amd.walk), on the GPU.

fit encodes every frame of a wav, or of every *.wav of a folder (sorted by name), to its mu, fits the principal axes and
the frame-to-frame dynamics on the first K of them (files are kept apart: no pair of frames spans two files) and writes
one .npz (walk.write_walk).  It prints one JSON line: n_frames, n_files, rank, keep, predictability (the share of the
whitened variance one step explains) and the leading persistences (diag A).

  --keep K           axes the walk keeps (default: every axis of the rank)
  --diagonal         every axis its own AR(1) process instead of the full k x k dynamics

run generates --seconds of audio block by block (walk.StreamingWalk):

  --hop N            frame hop; it must be the hop the walk was fitted at (one step of the walk is one frame)
  --window hann|none overlap-add window (default none: rectangular)
  --temperature T    scale of the noise that drives the walk (default 1: the corpus's own spread; 0 decays to its mean)
  --seed N           Philox seed; the same seed gives the same file
  --streams N        N independent walks, written as OUT_0.wav .. OUT_{N-1}.wav
  --start in.wav     start every stream from the state of the wav's last frame instead of a stationary draw
  --pca-shift J:H,.. move along principal axis J (1-based) by H standard deviations of the corpus

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

from latent_pca import _positive, check_axes, parse_axis_values  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Generate audio from a corpus: a fitted latent walk on the GPU")
    sub = p.add_subparsers(dest="command")
    for name in ("fit", "run"):
        s = sub.add_parser(name)
        s.add_argument("--config", default="./default.ini", help="the training .ini (model shape, sampling_rate)")
        s.add_argument("--checkpoint", required=True, help="checkpoint dict (ckpt_NNNNN) or whole-module pickle (.pt)")
        s.add_argument("--hop", default=None, help="frame hop (default: non-overlapping frames)")
        s.add_argument("--out", required=True, help="fit: the .npz; run: the output wav")
        if name == "fit":
            s.add_argument("--data", required=True, help="a wav, or a folder whose *.wav are encoded")
            s.add_argument("--keep", default=None, help="axes the walk keeps (default: the rank)")
            s.add_argument("--diagonal", action="store_true", help="independent AR(1) axes")
        else:
            s.add_argument("--walk", required=True, help="the .npz written by fit")
            s.add_argument("--seconds", required=True, help="length of the output")
            s.add_argument("--window", default="none", help="none | hann")
            s.add_argument("--temperature", default="1", help="scale of the driving noise")
            s.add_argument("--seed", default="0", help="Philox seed")
            s.add_argument("--streams", default="1", help="independent walks, one file each")
            s.add_argument("--start", default=None, help="a wav whose last frame seeds the state")
            s.add_argument("--pca-shift", dest="pca_shift", default=None, help="J:H,...: move along axis J by H sigma")
    args = p.parse_args(argv)
    if args.command is None:
        raise ValueError("expected a command: fit or run")
    _positive(args, "hop")
    if args.command == "fit":
        _positive(args, "keep")
        return args
    _positive(args, "streams")
    _positive(args, "seed", allow_zero=True)
    for flag in ("seconds", "temperature"):
        try:
            v = float(getattr(args, flag))
        except ValueError:
            v = float("nan")
        if not (v == v and abs(v) != float("inf") and (v > 0 if flag == "seconds" else v >= 0)):
            raise ValueError("--%s %r: expected a finite %s number" % (
                flag, getattr(args, flag), "positive" if flag == "seconds" else "non-negative"))
        setattr(args, flag, v)
    if args.window not in ("none", "hann"):
        raise ValueError("--window %r: expected none or hann" % args.window)
    args.window = None if args.window == "none" else args.window
    args.pca_shift = {} if args.pca_shift is None else parse_axis_values(args.pca_shift, "pca-shift")
    return args


def check_hop(args, meta):
    """--hop against the hop the walk file was fitted at; ValueError naming both."""
    from rawaudiovae_kelsey_amd.walk import check_hop as same_hop
    try:
        return same_hop(meta["hop"], args.hop, meta["segment_length"])
    except ValueError as e:
        raise ValueError("--hop: %s (--walk %r)" % (e, args.walk))


def out_paths(out, n_streams):
    """The files of a run: `out` itself, or OUT_0.wav .. with --streams N > 1."""
    if n_streams == 1:
        return [out]
    stem, ext = os.path.splitext(out)
    return ["%s_%d%s" % (stem, s, ext) for s in range(n_streams)]


def fit(args):
    from evaluate import data_files
    from interpolate import load_model, read_model_config
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import walk as W
    from rawaudiovae_kelsey_amd.codec import frame_layout
    cfg = read_model_config(args.config)
    try:
        frame_layout(cfg["segment_length"], cfg["segment_length"], args.hop)
    except ValueError as e:
        raise ValueError("--hop %s: %s" % (args.hop, e))
    files = data_files(args.data)
    model = load_model(args.checkpoint, cfg)
    waves = [D.load_audio_mono(f, cfg["sampling_rate"]) for f in files]
    try:
        walk = W.fit_corpus(model, waves, args.hop, args.keep, "diagonal" if args.diagonal else "full")
    except ValueError as e:
        raise ValueError("--data %r / --keep %s: %s" % (args.data, args.keep, e))
    W.write_walk(args.out, walk, cfg["segment_length"], args.hop)
    report = dict(n_frames=walk.n_frames_, n_files=walk.n_files_, rank=walk.rank_, keep=walk.n_components,
                  predictability=walk.predictability_, persistence=[float(v) for v in walk.persistence_[:8]])
    print(json.dumps(report))
    return report


def start_state(model, walk, path, sampling_rate, hop):
    """The whitened state [1, k] of the last frame of the wav at `path`."""
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    codec = FrameCodec(model)
    w = codec.wave(D.load_audio_mono(path, sampling_rate))
    try:
        padded, T = codec.pad(w, w.numel(), hop)
    except ValueError as e:
        raise ValueError("--start %r: %s" % (path, e))
    mu, _ = codec.encode(padded, T, hop)
    return walk.whiten(mu[T - 1:T].contiguous())


def run(args):
    import torch
    from interpolate import load_model, read_model_config
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import walk as W
    from rawaudiovae_kelsey_amd.pca import LatentPCA
    from rawaudiovae_kelsey_amd.stream import check_args
    cfg = read_model_config(args.config)
    S = cfg["segment_length"]
    for flag, path in (("walk", args.walk), ("start", args.start)):
        if path is not None and not os.path.exists(path):
            raise ValueError("--%s %r: no such file" % (flag, path))
    model = load_model(args.checkpoint, cfg)
    walk, meta = W.read_walk(args.walk, model.fc1.weight.device)
    if meta["segment_length"] != S or meta["latent_dim"] != cfg["latent_dim"]:
        raise ValueError("--walk %r: fitted for segment_length %d and latent_dim %d, the model has %d and %d" % (
            args.walk, meta["segment_length"], meta["latent_dim"], S, cfg["latent_dim"]))
    hop = check_hop(args, meta)
    try:
        check_args(S, hop, hop, args.window)
    except ValueError as e:
        raise ValueError("--window %s: %s" % (args.window or "none", e))
    k = walk.n_components
    shifts = check_axes(args.pca_shift, k, "pca-shift")
    n = int(round(args.seconds * cfg["sampling_rate"]))
    if n < 1:
        raise ValueError("--seconds %r: no sample at %d Hz" % (args.seconds, cfg["sampling_rate"]))
    # blocks of up to 16 frames: the audio does not depend on the block length
    frames = -(-n // hop)
    per = min(16, frames)
    gen = W.StreamingWalk(model, walk, args.streams, per * hop, hop, args.window, args.seed)
    gen.temperature.fill_(args.temperature)
    if shifts:
        axes = LatentPCA(k)._set(walk.mean_, walk.components_, walk.explained_variance_, walk.n_frames_, 0, k)
        gen.offset.copy_(axes.offset(shifts).expand_as(gen.offset))
    if args.start is not None:
        w0 = start_state(model, walk, args.start, cfg["sampling_rate"], args.hop)
        gen.set_state(w0.expand(args.streams, k))
    with torch.no_grad():
        y = torch.cat([gen.generate() for _ in range(-(-frames // per))], 1)[:, :n].cpu().numpy()
    paths = out_paths(args.out, args.streams)
    for path, row in zip(paths, y):
        D.write_wav(path, row, cfg["sampling_rate"])
    print("wrote %s: %d samples per stream, hop %d, window %s, %d axes, temperature %g, seed %d"
          % (", ".join(paths), n, hop, args.window or "none", k, args.temperature, args.seed))
    return y


def main(argv=None):
    args = parse_args(argv)
    return fit(args) if args.command == "fit" else run(args)


if __name__ == "__main__":
    main()
