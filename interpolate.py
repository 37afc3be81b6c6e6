"""`python interpolate.py --config default.ini --checkpoint ckpt_00500 --a a.wav --b b.wav --out out.wav`

Latent interpolation between two sounds with a trained model: the workflow of the reference's tutorial.ipynb
(stepwise 456-530, meso-scale curve 834-925, with extensions 1200-1279) as one command, computed on the GPU by
rawaudiovae_kelsey_amd.interpolate.LatentInterpolator.

  --mode stepwise --alphas 0:1.1:0.2       numpy.arange(start, stop, step), or a comma list 0,0.5,1
  --mode curve --curve sin:-500:500:20000  sin(linspace(-500 pi, 500 pi, 20000)), stretched to the frame count
  --mode curve --curve file.npy            a float64 curve from a .npy file
  --hop N                                  frame like AudioDataset at hop N (default: TestDataset framing)
  --match repeat|crop                      repeat the shorter source (default) or crop the longer one
  --seed S                                 seed of the on-device eps draw
  --som DIR --audio DIR --a-cluster K      source a is node K of a SOM (som.py): its files concatenated in list
                                           order, as the notebook's concat_audio_som (743-756); likewise --b-cluster

The model shape (segment_length, n_units, latent_dim) and sampling_rate come from the .ini as in train.py.  The
checkpoint is a training checkpoint dict (its 'state_dict', as tutorial.ipynb:292-298 loads it) or a whole-module
pickle (best_model.pt / last_model.pt).  Bad flag values raise ValueError naming the flag.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, load_model, load_wav, nonneg_int, number_flag,  # noqa: E402
                                             positive_int, read_model_config)


def parse_alphas(spec):
    """'start:stop:step' -> numpy.arange(start, stop, step); 'a,b,c' -> [a, b, c] (float64)."""
    try:
        if ":" in spec:
            parts = [float(p) for p in spec.split(":")]
            if len(parts) != 3 or parts[2] == 0:
                raise ValueError
            out = np.arange(parts[0], parts[1], parts[2])
        else:
            out = np.array([float(p) for p in spec.split(",")], dtype=np.float64)
    except ValueError:
        raise ValueError("--alphas %r: expected start:stop:step (nonzero step) or a comma list of numbers" % spec)
    if out.size == 0:
        raise ValueError("--alphas %r gives no values" % spec)
    return out.astype(np.float64)


def parse_curve(spec):
    """'sin:lo:hi:n' -> sin(linspace(lo pi, hi pi, n)); a path ending in .npy -> its 1-D float64 array."""
    if spec.endswith(".npy"):
        if not os.path.exists(spec):
            raise ValueError("--curve %r: no such file" % spec)
        c = np.load(spec)
        if c.ndim != 1 or c.size < 2 or not np.issubdtype(c.dtype, np.floating):
            raise ValueError("--curve %r: expected a 1-D float array of at least 2 points, got %s %s"
                             % (spec, c.dtype, c.shape))
        return c.astype(np.float64)
    parts = spec.split(":")
    try:
        if len(parts) != 4 or parts[0] != "sin":
            raise ValueError
        lo, hi, n = float(parts[1]), float(parts[2]), int(parts[3])
    except ValueError:
        raise ValueError("--curve %r: expected sin:lo:hi:n (multiples of pi, n points) or a .npy file" % spec)
    if n < 2:
        raise ValueError("--curve %r: a curve needs at least 2 points" % spec)
    return np.sin(np.linspace(lo * np.pi, hi * np.pi, n))


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Latent interpolation between two sounds (tutorial.ipynb on the GPU)")
    add_model_flags(p, hop_help="AudioDataset hop (default: TestDataset framing)")
    p.add_argument("--a", default=None, help="first sound (wav); or --a-cluster")
    p.add_argument("--b", default=None, help="second sound (wav); or --b-cluster")
    p.add_argument("--som", default=None, help="folder with clusters.json and data-concatenated.json (som.py)")
    p.add_argument("--audio", default=None, help="the folder the SOM's relative paths start from")
    p.add_argument("--a-cluster", default=None, help="first sound: the files of this SOM node, concatenated")
    p.add_argument("--b-cluster", default=None, help="second sound: the files of this SOM node, concatenated")
    p.add_argument("--out", required=True, help="output wav")
    p.add_argument("--mode", default="stepwise", help="stepwise | curve")
    p.add_argument("--alphas", default="0:1.1:0.2", help="stepwise: start:stop:step or a comma list")
    p.add_argument("--curve", default="sin:-500:500:20000", help="curve: sin:lo:hi:n or file.npy")
    p.add_argument("--match", default="repeat", help="repeat | crop")
    p.add_argument("--seed", default="0", help="seed of the eps draw")
    p.add_argument("--max-rows", default="16384", help="frames per chunk")
    args = p.parse_args(argv)
    if args.mode not in ("stepwise", "curve"):
        raise ValueError("--mode %r: expected stepwise or curve" % args.mode)
    if args.match not in ("repeat", "crop"):
        raise ValueError("--match %r: expected repeat or crop" % args.match)
    positive_int(args, "hop")
    nonneg_int(args, "seed")
    positive_int(args, "max-rows")
    for s in ("a", "b"):
        wav, node = getattr(args, s), getattr(args, s + "_cluster")
        if (wav is None) == (node is None):
            raise ValueError("--%s / --%s-cluster: give exactly one of them" % (s, s))
        if node is not None:
            number_flag(args, s + "-cluster", int, lambda k: k >= 0, "a non-negative node index")
            if args.som is None or args.audio is None:
                raise ValueError("--%s-cluster needs --som and --audio" % s)
    args.alpha_values = parse_alphas(args.alphas) if args.mode == "stepwise" else None
    args.curve_values = parse_curve(args.curve) if args.mode == "curve" else None
    return args


def cluster_audio(som_dir, audio_dir, node, sampling_rate, flag):
    """concat_audio_som (tutorial.ipynb:743-756): the node's files in list order, each loaded at sampling_rate, joined
    into one waveform.  A missing or empty node raises ValueError naming `flag`."""
    from rawaudiovae_kelsey_amd.som import cluster_paths, read_som
    clusters, data = read_som(som_dir)
    try:
        paths = cluster_paths(clusters, data, audio_dir, node)
    except KeyError:
        raise ValueError("%s %d: no such node in %s" % (flag, node, os.path.join(som_dir, "clusters.json")))
    if not paths:
        raise ValueError("%s %d: the node has no files" % (flag, node))
    return np.concatenate([load_wav(p, sampling_rate) for p in paths], 0)


def main(argv=None):
    args = parse_args(argv)
    cfg = read_model_config(args.config)
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd.interpolate import LatentInterpolator
    model = load_model(args.checkpoint, cfg)
    sr = cfg["sampling_rate"]
    a = (load_wav(args.a, sr) if args.a is not None
         else cluster_audio(args.som, args.audio, args.a_cluster, sr, "--a-cluster"))
    b = (load_wav(args.b, sr) if args.b is not None
         else cluster_audio(args.som, args.audio, args.b_cluster, sr, "--b-cluster"))
    it = LatentInterpolator(model, max_rows=args.max_rows)
    if args.mode == "stepwise":
        out = it.stepwise(a, b, args.alpha_values, hop=args.hop, seed=args.seed, match=args.match)
    else:
        out = it.curve(a, b, args.curve_values, hop=args.hop, seed=args.seed, match=args.match)
    y = out.cpu().numpy()
    D.write_wav(args.out, y, cfg["sampling_rate"])
    print("wrote %s: %d samples (%.2f s at %d Hz)" % (args.out, y.size, y.size / cfg["sampling_rate"],
                                                      cfg["sampling_rate"]))
    return y


if __name__ == "__main__":
    main()
