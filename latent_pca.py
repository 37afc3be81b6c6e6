"""`python latent_pca.py fit --config default.ini --checkpoint ckpt_00500 --data DIR_OR_WAV --hop 256 --out pca.npz`
`python latent_pca.py edit --config default.ini --checkpoint ckpt_00500 --pca pca.npz --in in.wav --out out.wav
        --hop 256 --window hann --shift 2:1.5`

Principal axes of a corpus's latents on the GPU (rawaudiovae_kelsey_amd.pca), and offline edits along them.

fit encodes every frame of a wav, or of every *.wav of a folder (sorted by name), to its mu, fits the axes on all of
them and writes one .npz (pca.write_pca).  It prints one JSON line: n_frames, sweeps, effective_dim and the number of
axes that carry 90, 99 and 99.9 % of the variance.

edit encodes a wav to mu, moves every frame along the axes, decodes z = mu' (no eps) and overlap-adds the frames:

  --hop N            frame hop (default: non-overlapping frames of segment_length)
  --window hann|none overlap-add window (default none: rectangular)
  --keep K           keep the first K axes and drop the rest (gain 0): the rank-K resynthesis about the corpus mean
  --gain J:G,...     scale coordinate J (1-based) about the mean by G
  --shift J:H,...    move along axis J (1-based) by H standard deviations of the corpus
                     (--gain overrides --keep on the axes it names)

Without --keep, --gain and --shift the output is the plain temperature-0 reconstruction, bit for bit.  Bad flag values
raise ValueError naming the flag.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, check_axes, check_exists, check_fitted, data_files,  # noqa: E402
                                             encode_wav, frame_step, load_model, load_wav, nonneg_int,
                                             parse_axis_values, positive_int, read_model_config, window_flag)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Principal axes of a corpus's latents on the GPU, and edits along them")
    sub = p.add_subparsers(dest="command")
    for name in ("fit", "edit"):
        s = sub.add_parser(name)
        add_model_flags(s)
        s.add_argument("--out", required=True, help="fit: the .npz; edit: the output wav")
        if name == "fit":
            s.add_argument("--data", required=True, help="a wav, or a folder whose *.wav are encoded")
        else:
            s.add_argument("--pca", required=True, help="the .npz written by fit")
            s.add_argument("--in", dest="inp", required=True, help="input wav")
            s.add_argument("--window", default="none", help="none | hann")
            s.add_argument("--keep", default=None, help="keep the first K axes, drop the rest")
            s.add_argument("--gain", default=None, help="J:G,...: scale coordinate J (1-based) about the mean")
            s.add_argument("--shift", default=None, help="J:H,...: move along axis J by H standard deviations")
    args = p.parse_args(argv)
    if args.command is None:
        raise ValueError("expected a command: fit or edit")
    positive_int(args, "hop")
    if args.command == "edit":
        nonneg_int(args, "keep")
        window_flag(args)
        args.gain = {} if args.gain is None else parse_axis_values(args.gain, "gain")
        args.shift = {} if args.shift is None else parse_axis_values(args.shift, "shift")
    return args


def check_framing(args, segment_length):
    """The framing flags against the model's frame length -> the frame step; ValueError naming the flag."""
    from rawaudiovae_kelsey_amd.mosaic import check_window
    step = frame_step(args, segment_length)
    if args.command == "edit":
        try:
            check_window(int(segment_length), step, args.window)
        except ValueError as e:
            raise ValueError("--window %s: %s" % (args.window or "none", e))
    return step


def controls(args, n_axes):
    """(gains, shifts) [n_axes] float32 of the edit flags; ValueError naming the flag."""
    gains, shifts = np.ones(n_axes, dtype=np.float32), np.zeros(n_axes, dtype=np.float32)
    if args.keep is not None:
        if args.keep > n_axes:
            raise ValueError("--keep %d: the PCA file holds %d axes" % (args.keep, n_axes))
        gains[args.keep:] = 0
    for j, g in check_axes(args.gain, n_axes, "gain").items():
        gains[j] = g
    for j, h in check_axes(args.shift, n_axes, "shift").items():
        shifts[j] = h
    return gains, shifts


def fit(args):
    from rawaudiovae_kelsey_amd import pca as P
    cfg = read_model_config(args.config)
    check_framing(args, cfg["segment_length"])
    files = data_files(args.data)
    model = load_model(args.checkpoint, cfg)
    waves = [load_wav(f, cfg["sampling_rate"]) for f in files]
    try:
        pca = P.fit_corpus(model, waves, args.hop)
    except ValueError as e:
        raise ValueError("--data %r: %s" % (args.data, e))
    P.write_pca(args.out, pca, cfg["segment_length"], args.hop)
    report = dict(n_frames=pca.n_frames_, sweeps=pca.sweeps_, effective_dim=pca.effective_dim_,
                  components_90=pca.components_needed(0.9), components_99=pca.components_needed(0.99),
                  components_99_9=pca.components_needed(0.999))
    print(json.dumps(report))
    return report


def edit(args):
    import torch
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import pca as P
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    from rawaudiovae_kelsey_amd.mosaic import ola
    from rawaudiovae_kelsey_amd.stream import window_values
    cfg = read_model_config(args.config)
    S = cfg["segment_length"]
    step = check_framing(args, S)
    for flag, path in (("pca", args.pca), ("in", args.inp)):
        check_exists(flag, path)
    model = load_model(args.checkpoint, cfg)
    codec = FrameCodec(model)
    pca, meta = P.read_pca(args.pca, codec.device)
    check_fitted("pca", args.pca, meta, cfg)
    gains, shifts = controls(args, pca.components_.shape[0])
    with torch.no_grad():
        w, mu, _, T = encode_wav(codec, load_wav(args.inp, cfg["sampling_rate"]), args.hop, "in", args.inp)
        frames = codec.decode(pca.edit(mu, gains, shifts))
        win = None if args.window is None else torch.from_numpy(window_values(S, args.window)).to(codec.device)
        y = ola(frames, step, w.numel(), win).cpu().numpy()
    D.write_wav(args.out, y, cfg["sampling_rate"])
    print("wrote %s: %d samples from %d frames, hop %d, window %s, %d axes edited"
          % (args.out, y.size, T, step, args.window or "none", int(((gains != 1) | (shifts != 0)).sum())))
    return y


def main(argv=None):
    args = parse_args(argv)
    return fit(args) if args.command == "fit" else edit(args)


if __name__ == "__main__":
    main()
