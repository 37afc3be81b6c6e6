"""`python attributes.py measure --in a.wav --segment-length 1024 --hop 256 --window hann --out desc.npy`
`python attributes.py fit  --config default.ini --checkpoint ckpt_00500 --data DIR_OR_WAV --pca pca.npz --keep 16 --hop 256
        --out attrs.npz`
`python attributes.py move --attrs attrs.npz --move centroid:+0.02,level:-3 --hold --out offset.npy`
`python attributes.py edit --config default.ini --checkpoint ckpt_00500 --attrs attrs.npz --in a.wav --out b.wav --hop 256
        --window hann --move centroid:+0.02,level:-3 --hold`

Latent attributes (rawaudiovae_kelsey_amd.attributes), on the GPU: audio descriptors of every frame -- level (dB), zcr,
crest (dB), centroid (cycles/sample), flatness (dB) -- and the latent directions that move them.

measure  describes every frame of a wav and writes desc [frames, 5] float64 (.npy); needs no checkpoint.  Prints every
         descriptor's mean and standard deviation over the frames where it is finite, and the silent frames.
  --segment-length S   frame length; with --window hann a power of two in [32, 4096]
  --hop N              frame hop (default: non-overlapping frames)
  --window hann|none   none: level, zcr and crest only (any frame length)
fit      encodes every frame of a wav, or of every *.wav of a folder (sorted by name), to its mu, describes the same
         frames, and regresses the descriptors on the first K whitened principal coordinates.  Prints per descriptor its
         mean, standard deviation and R^2 (how much of it the latents explain linearly) and the predicted cross-talk matrix
         (row a: what a move of descriptor a alone by one of its standard deviations does to every descriptor, in theirs),
         then one JSON line; writes one .npz (attributes.write_attributes).
  --pca F.npz          the axes: a file of `latent_pca.py fit` at the same hop (default: the corpus's own)
  --keep K             whitened axes (default 16, at most 64 and the rank)
  --ridge X            ridge on the whitened covariance (default 0)
  --targets T.npy --names a,b    the user's own [frames, N] targets in place of the built-in descriptors
move     turns moves into the latent offset `resynth.py --offset` takes (.npy, latent_dim float32 values) and prints the
         predicted change of every descriptor and the size of the step in corpus standard deviations.
  --move NAME:DELTA,...   the change of each named descriptor in its own unit
  --hold               hold every descriptor that is not named at change 0
edit     encodes a wav to mu, adds the offset to every frame, decodes z = mu + offset (no eps) and overlap-adds; prints,
         per descriptor, the requested, the predicted and the achieved change (the decoder's actual response).

--hop must be the hop the attributes were fitted at.  Bad flag values raise ValueError naming the flag.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, check_exists, check_fitted, data_files, encode_wav,  # noqa: E402
                                             flagged, frame_step, load_model, load_wav, nonneg_real, positive_int,
                                             read_model_config, window_flag)

COMMANDS = ("measure", "fit", "move", "edit")
HOP_PHRASES = ("the attributes were", "a descriptor is of one frame at that hop")
K_MAX = 64      # rawaudiovae_kelsey_amd.attributes.K_MAX (not imported here: a bad flag needs no torch)


def parse_moves(text, flag="move"):
    """{name: delta} of "NAME:DELTA,..." ("" -> {}); ValueError naming `flag` for anything else, a delta that is not finite
    or a name given twice."""
    out = {}
    for item in [s for s in str(text).split(",") if s.strip()]:
        name, sep, v = item.partition(":")
        name = name.strip()
        try:
            if not sep or not name:
                raise ValueError
            value = float(v)
        except ValueError:
            raise ValueError("--%s %r: expected NAME:DELTA,..., got %r" % (flag, text, item))
        if value != value or abs(value) == float("inf"):
            raise ValueError("--%s %r: %s: the change must be finite" % (flag, text, name))
        if name in out:
            raise ValueError("--%s %r: %s is given twice" % (flag, text, name))
        out[name] = value
    return out


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Latent attributes: audio descriptors and the latent directions that move them")
    sub = p.add_subparsers(dest="command")
    for name in COMMANDS:
        s = sub.add_parser(name)
        if name in ("fit", "edit"):
            add_model_flags(s)
        if name == "measure":
            s.add_argument("--in", dest="wav", required=True, help="the wav")
            s.add_argument("--segment-length", dest="segment_length", required=True, help="frame length")
            s.add_argument("--hop", default=None, help="frame hop (default: non-overlapping frames)")
            s.add_argument("--window", default="hann", help="hann | none")
        if name == "fit":
            s.add_argument("--data", required=True, help="a wav, or a folder whose *.wav are encoded")
            s.add_argument("--pca", default=None, help="the .npz of latent_pca.py fit")
            s.add_argument("--keep", default="16", help="whitened axes (default 16)")
            s.add_argument("--ridge", default="0", help="ridge on the whitened covariance (default 0)")
            s.add_argument("--targets", default=None, help="a .npy of [frames, N] targets of your own")
            s.add_argument("--names", default=None, help="their names, a,b,...")
        if name in ("move", "edit"):
            s.add_argument("--attrs", required=True, help="the .npz written by fit")
            s.add_argument("--move", default="", help="NAME:DELTA,...")
            s.add_argument("--hold", action="store_true", help="hold the descriptors that are not named")
        if name == "edit":
            s.add_argument("--in", dest="wav", required=True, help="input wav")
            s.add_argument("--window", default="none", help="none | hann (the overlap-add window)")
        s.add_argument("--out", required=True, help="measure: the .npy; fit: the .npz; move: the .npy; edit: the wav")
    args = p.parse_args(argv)
    if args.command is None:
        raise ValueError("expected a command: measure, fit, move or edit")
    if args.command != "move":
        positive_int(args, "hop")
    if args.command == "measure":
        positive_int(args, "segment-length")
        window_flag(args)
        S = args.segment_length
        if args.window is not None and not (32 <= S <= 4096 and S & (S - 1) == 0):
            raise ValueError("--segment-length %d: --window %s needs a power of two in [32, 4096] (--window none describes "
                             "without the spectrum)" % (S, args.window))
        if args.hop is not None and S % args.hop != 0:
            raise ValueError("--hop %d: does not divide --segment-length %d" % (args.hop, S))
    if args.command == "fit":
        if positive_int(args, "keep") > K_MAX:
            raise ValueError("--keep %d: at most %d" % (args.keep, K_MAX))
        nonneg_real(args, "ridge")
        if (args.targets is None) != (args.names is None):
            raise ValueError("--targets and --names come together: %s is missing" % ("--names" if args.names is None else "--targets"))
        if args.names is not None:
            args.names = [n.strip() for n in args.names.split(",")]
            if not all(args.names) or len(set(args.names)) != len(args.names) or any(":" in n for n in args.names):
                raise ValueError("--names %r: expected distinct non-empty names a,b,... without ':'" % ",".join(args.names))
    if args.command in ("move", "edit"):
        args.move = parse_moves(args.move)
    if args.command == "edit":
        window_flag(args)
    return args


def measure(args):
    import torch
    from rawaudiovae_kelsey_amd import attributes as A
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd.codec import frame_layout
    check_exists("in", args.wav)
    try:
        wave, sr = D.read_wav(args.wav)          # at the file's own rate: nothing here depends on a model's
    except Exception as e:
        raise ValueError("--in %r: unreadable wav (%s)" % (args.wav, e))
    wave = wave.mean(axis=1) if wave.ndim == 2 else wave
    S = args.segment_length
    T, padded = frame_layout(wave.size, S, args.hop)
    if T < 1:
        raise ValueError("--in %r: %d samples make no frame of %d samples at hop %s" % (args.wav, wave.size, S, args.hop))
    buf = np.zeros(padded, dtype=np.float32)
    buf[:wave.size] = wave
    desc = A.describe(torch.from_numpy(buf).cuda(), T, S, S if args.hop is None else args.hop, args.window).cpu().numpy()
    np.save(args.out, desc)
    report = _describe_report(desc, A.NAMES[:desc.shape[1]])
    report.update(frames=int(T), sampling_rate=int(sr), segment_length=S, hop=S if args.hop is None else args.hop)
    print(json.dumps(report))
    return report


def _describe_report(desc, names):
    """Print and return every descriptor's mean and std over its finite frames, and the silent frames (level -inf)."""
    silent = int(np.isneginf(desc[:, 0]).sum())
    report = dict(silent_frames=silent, mean={}, std={})
    for j, name in enumerate(names):
        col = desc[:, j][np.isfinite(desc[:, j])]
        m, s = (float(col.mean()), float(col.std())) if col.size else (None, None)
        report["mean"][name], report["std"][name] = m, s
        print("%-9s mean %s  std %s  (%d frames)" % (name, "-" if m is None else "%.6g" % m, "-" if s is None else "%.6g" % s, col.size))
    print("%d silent frames of %d" % (silent, desc.shape[0]))
    return report


def crosstalk(attrs):
    """[N, N]: row a = the predicted change of every descriptor, in its own standard deviations, when descriptor a alone is
    moved by one of its standard deviations (NaN where a direction is degenerate)"""
    N = len(attrs.names)
    out = np.full((N, N), np.nan)
    for a, name in enumerate(attrs.names):
        try:
            out[a] = attrs.move({name: attrs.std_[a]})[1] / attrs.std_
        except ValueError:
            pass
    return out


def fit(args):
    from rawaudiovae_kelsey_amd import attributes as A
    from rawaudiovae_kelsey_amd import pca as P
    cfg = read_model_config(args.config)
    frame_step(args, cfg["segment_length"])
    files = data_files(args.data)
    targets = None
    if args.targets is not None:
        check_exists("targets", args.targets)
        targets = np.load(args.targets)
        if targets.ndim != 2 or targets.shape[1] != len(args.names):
            raise ValueError("--targets %r: shape %s does not hold one column for each of the %d --names" % (
                args.targets, targets.shape, len(args.names)))
    pca = None
    if args.pca is not None:
        check_exists("pca", args.pca)
    model = load_model(args.checkpoint, cfg)
    if args.pca is not None:
        pca, meta = flagged("--pca", lambda: P.read_pca(args.pca, model.fc1.weight.device))
        check_fitted("pca", args.pca, meta, cfg, args.hop, "the axes were", HOP_PHRASES[1])
    waves = [load_wav(f, cfg["sampling_rate"]) for f in files]
    S = cfg["segment_length"]
    window = "hann" if 32 <= S <= 4096 and S & (S - 1) == 0 else None     # another frame length: level, zcr and crest
    try:
        attrs, x, desc = A.fit_corpus(model, waves, args.hop, pca, args.keep, args.ridge, window, targets=targets,
                                      names=args.names)
    except (ValueError, A.RvError) as e:
        raise ValueError("--data %r / --keep %s / --ridge %s: %s" % (args.data, args.keep, args.ridge, e))
    A.write_attributes(args.out, attrs, S, args.hop)
    cross = crosstalk(attrs)
    report = dict(n_frames=attrs.n_frames_, n_observed=attrs.n_observed_, keep=int(attrs.B_.shape[1]), names=list(attrs.names),
                  mean=[float(v) for v in attrs.mean_], std=[float(v) for v in attrs.std_], r2=[float(v) for v in attrs.r2_],
                  crosstalk=[[None if v != v else float(v) for v in row] for row in cross])
    print("%d of %d frames observed, %d axes" % (attrs.n_observed_, attrs.n_frames_, attrs.B_.shape[1]))
    for a, name in enumerate(attrs.names):
        print("%-9s mean %.6g  std %.6g  R2 %.4f  cross-talk %s" % (
            name, attrs.mean_[a], attrs.std_[a], attrs.r2_[a], " ".join("%+.3f" % v for v in cross[a])))
    print(json.dumps(report))
    return report


def _read_attrs(args, device):
    from rawaudiovae_kelsey_amd import attributes as A
    check_exists("attrs", args.attrs)
    attrs, meta = flagged("--attrs", lambda: A.read_attributes(args.attrs, device))
    offset, predicted, norm = flagged("--move", lambda: attrs.move(args.move, args.hold))
    return attrs, meta, offset, predicted, norm


def move(args):
    attrs, _, offset, predicted, norm = _read_attrs(args, "cpu")
    np.save(args.out, offset.numpy())
    report = dict(names=list(attrs.names), requested=[args.move.get(n) for n in attrs.names],
                  predicted=[float(v) for v in predicted], norm=norm, hold=bool(args.hold))
    for n, v in zip(attrs.names, predicted):
        print("%-9s requested %s  predicted %+.6g" % (n, "-" if n not in args.move else "%+.6g" % args.move[n], v))
    print("norm %.6g corpus standard deviations" % norm)
    print(json.dumps(report))
    return report


def edit(args):
    import torch
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    from rawaudiovae_kelsey_amd.mosaic import check_window, ola
    from rawaudiovae_kelsey_amd.stream import window_values
    cfg = read_model_config(args.config)
    S = cfg["segment_length"]
    step = frame_step(args, S)
    try:
        check_window(S, step, args.window)
    except ValueError as e:
        raise ValueError("--window %s: %s" % (args.window or "none", e))
    check_exists("in", args.wav)
    check_exists("attrs", args.attrs)
    model = load_model(args.checkpoint, cfg)
    codec = FrameCodec(model)
    attrs, meta, offset, predicted, norm = _read_attrs(args, codec.device)
    check_fitted("attrs", args.attrs, meta, cfg, args.hop, *HOP_PHRASES)
    spectral = 32 <= S <= 4096 and S & (S - 1) == 0
    with torch.no_grad():
        w, mu, _, T = encode_wav(codec, load_wav(args.wav, cfg["sampling_rate"]), args.hop, "in", args.wav)
        z = mu + offset if args.move else mu        # no move: the temperature-0 reconstruction, bit for bit
        win = None if args.window is None else torch.from_numpy(window_values(S, args.window)).to(codec.device)
        y = ola(codec.decode(z), step, w.numel(), win).cpu().numpy()
        achieved, n = attrs.response(codec, mu, offset, S, "hann" if spectral else None)
    D.write_wav(args.out, y, cfg["sampling_rate"])
    from rawaudiovae_kelsey_amd.attributes import NAMES
    got = dict(zip(NAMES, achieved))       # the decoder's response is measured on the built-in descriptors
    report = dict(names=list(attrs.names), requested=[args.move.get(nm) for nm in attrs.names],
                  predicted=[float(v) for v in predicted], achieved=[None if nm not in got or got[nm] != got[nm] else float(got[nm])
                                                                     for nm in attrs.names],
                  norm=norm, frames=int(T), frames_compared=int(n), hold=bool(args.hold))
    print("wrote %s: %d samples from %d frames, hop %d, window %s" % (args.out, y.size, T, step, args.window or "none"))
    for i, nm in enumerate(attrs.names):
        a = report["achieved"][i]
        print("%-9s requested %s  predicted %+.6g  achieved %s" % (
            nm, "-" if nm not in args.move else "%+.6g" % args.move[nm], predicted[i], "-" if a is None else "%+.6g" % a))
    print("norm %.6g corpus standard deviations; achieved over %d of %d frames" % (norm, n, T))
    print(json.dumps(report))
    return y


def main(argv=None):
    args = parse_args(argv)
    return {"measure": measure, "fit": fit, "move": move, "edit": edit}[args.command](args)


if __name__ == "__main__":
    main()
