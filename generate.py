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

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, check_axes, check_exists, check_fitted, data_files,  # noqa: E402
                                             encode_wav, load_model, load_wav, model_config, nonneg, nonneg_int,
                                             number_flag, parse_axis_values, positive, positive_int, read_model_config,
                                             window_flag)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Generate audio from a corpus: a fitted latent walk on the GPU")
    sub = p.add_subparsers(dest="command")
    for name in ("fit", "run"):
        s = sub.add_parser(name)
        add_model_flags(s)
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
    positive_int(args, "hop")
    if args.command == "fit":
        positive_int(args, "keep")
        return args
    positive_int(args, "streams")
    nonneg_int(args, "seed")
    number_flag(args, "seconds", float, positive, "a finite positive number")
    number_flag(args, "temperature", float, nonneg, "a finite non-negative number")
    window_flag(args)
    args.pca_shift = {} if args.pca_shift is None else parse_axis_values(args.pca_shift, "pca-shift")
    return args


def out_paths(out, n_streams):
    """The files of a run: `out` itself, or OUT_0.wav .. with --streams N > 1."""
    if n_streams == 1:
        return [out]
    stem, ext = os.path.splitext(out)
    return ["%s_%d%s" % (stem, s, ext) for s in range(n_streams)]


def fit(args):
    from rawaudiovae_kelsey_amd import walk as W
    cfg, _ = model_config(args)
    files = data_files(args.data)
    model = load_model(args.checkpoint, cfg)
    waves = [load_wav(f, cfg["sampling_rate"]) for f in files]
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
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    _, mu, _, T = encode_wav(FrameCodec(model), load_wav(path, sampling_rate), hop, "start", path)
    return walk.whiten(mu[T - 1:T].contiguous())


def run(args):
    import torch
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import walk as W
    from rawaudiovae_kelsey_amd.pca import LatentPCA
    from rawaudiovae_kelsey_amd.stream import check_args
    cfg = read_model_config(args.config)
    S = cfg["segment_length"]
    for flag, path in (("walk", args.walk), ("start", args.start)):
        if path is not None:
            check_exists(flag, path)
    model = load_model(args.checkpoint, cfg)
    walk, meta = W.read_walk(args.walk, model.fc1.weight.device)
    hop = check_fitted("walk", args.walk, meta, cfg, args.hop)
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
