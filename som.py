"""`python som.py --config default.ini --checkpoint ckpt_00500 --audio DIR --out DIR`

Train a self-organising map of a corpus's files in a trained VAE's latent space and write the two files the reference's
tutorial.ipynb reads to pick its sources (725-805, 1078-1146): som/clusters.json and som/data-concatenated.json, plus
som.npz (weights, grid, sigma schedule, descriptors, errors).  `interpolate.py --som DIR --audio DIR --a-cluster K
--b-cluster J` then interpolates between two nodes' concatenated files.

  --grid 8x8        rows x cols of the map
  --epochs 50       batch-SOM epochs; sigma runs from --sigma0 (default max(rows, cols) / 2) to --sigma1 (0.5)
  --seed N          seed of the initial nodes (numpy.random.default_rng)
  --hop N           frame like AudioDataset at hop N (default: TestDataset framing)
  --max-rows N      frames per encoder chunk

The files are the sorted *.wav in --audio, loaded at the .ini's sampling_rate; each is described by the mean encoder
mu over its frames.  Bad flag values, empty or unreadable wavs raise ValueError naming the flag or the file.
"""
import argparse
import glob
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, int_at_least, load_model, load_wav, number_flag,  # noqa: E402
                                             positive, read_model_config)


def parse_grid(spec):
    parts = str(spec).lower().split("x")
    try:
        if len(parts) != 2:
            raise ValueError
        rows, cols = int(parts[0]), int(parts[1])
    except ValueError:
        raise ValueError("--grid %r: expected ROWSxCOLS, e.g. 8x8" % spec)
    if rows < 1 or cols < 1 or rows * cols < 2:
        raise ValueError("--grid %r: needs at least 2 nodes" % spec)
    return rows, cols


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Self-organising map of a corpus's latents (writes the tutorial's som/ files)")
    add_model_flags(p, hop_help="AudioDataset hop (default: TestDataset framing)")
    p.add_argument("--audio", required=True, help="folder of the corpus's .wav files")
    p.add_argument("--out", required=True, help="output folder for clusters.json, data-concatenated.json, som.npz")
    p.add_argument("--grid", default="8x8", help="ROWSxCOLS")
    p.add_argument("--epochs", default="50")
    p.add_argument("--sigma0", default=None, help="initial neighbourhood width (default max(rows, cols) / 2)")
    p.add_argument("--sigma1", default="0.5", help="final neighbourhood width")
    p.add_argument("--seed", default="0")
    p.add_argument("--max-rows", default="16384", help="frames per encoder chunk")
    args = p.parse_args(argv)
    args.rows, args.cols = parse_grid(args.grid)
    for flag, minimum in (("epochs", 1), ("seed", 0), ("max-rows", 1), ("hop", 1)):
        int_at_least(args, flag, minimum)
    for flag in ("sigma0", "sigma1"):
        number_flag(args, flag, float, positive, "a positive number")
    if not os.path.isdir(args.audio):
        raise ValueError("--audio %r: not a folder" % args.audio)
    return args


def corpus_files(audio_dir):
    """Sorted *.wav of audio_dir, as paths relative to it; ValueError when there are none."""
    files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(audio_dir, "*.wav")))
    if not files:
        raise ValueError("--audio %r: no .wav files" % audio_dir)
    return files


def main(argv=None):
    args = parse_args(argv)
    cfg = read_model_config(args.config)
    files = corpus_files(args.audio)
    waves = [load_wav(os.path.join(args.audio, f), cfg["sampling_rate"]) for f in files]
    from rawaudiovae_kelsey_amd.som import LatentMap, LatentSOM, write_som
    model = load_model(args.checkpoint, cfg)
    desc = LatentMap(model, hop=args.hop, max_rows=args.max_rows).describe(waves)
    som = LatentSOM(args.rows, args.cols, sigma0=args.sigma0, sigma1=args.sigma1, epochs=args.epochs,
                    seed=args.seed).fit(desc)
    best, _, _ = som.assign(desc)
    qe, te = write_som(args.out, files, best, som, descriptors=desc, hop=args.hop)
    print("wrote %s: %d files on a %dx%d map, QE %.6g, TE %.4f" % (args.out, len(files), args.rows, args.cols, qe, te))
    return qe, te


if __name__ == "__main__":
    main()
