"""`python mosaic.py --config default.ini --checkpoint ckpt_00500 --corpus DIR --target in.wav --out out.wav`

Latent audio mosaicing (rawaudiovae_kelsey_amd.mosaic.LatentIndex): every frame of the target is replaced by its
nearest corpus frames in the model's latent space, and the result is overlap-added into a wav of the target's length.

  --hop N            frame hop of the corpus and the target (default: segment_length, TestDataset framing)
  --k N              neighbours per target frame, 1..16 (default 1)
  --mode grains      the mean of the neighbours' audio; `decode`: the decoded mean of their mu
  --window hann|none overlap-add window (default none: rectangular; hann needs hop <= segment_length / 2)
  --continuity X     weight (float >= 0, default 0) of the concatenation cost: with X > 0 one of the k candidates per
                     frame is chosen by a Viterbi search that prefers corpus frames which follow each other
  --matches FILE     one CSV line per target frame: the k (file, sample offset, distance) triples; with --continuity
                     a last column holds the chosen slot (0-based, -1: none)
  --max-rows N       target frames per encoder / search / decoder chunk (the output does not depend on it)
  --live-block N     run the target through the live path instead (StreamingMosaic): blocks of N samples (a multiple of
                     the hop), the tail zero-padded to a whole block; the output drops the S - hop samples of latency
                     and is cut to the target's length, so it lines up with the offline result.  With --continuity X
                     one candidate per frame is chosen by the greedy rule (against the previous choice only), not by
                     the Viterbi search over the whole target; --lag buys look-ahead
  --streams M        with --live-block: cut the target into M consecutive parts and run them as M parallel streams,
                     each starting from silence (default 1)
  --lag N            with --live-block and --continuity X > 0: N frames of look-ahead, 0..64 (default 0: the greedy
                     rule).  Every frame is chosen by a Viterbi search over itself and the N frames after it; the live
                     output comes N * hop samples later, which the file drops as well

  --fit N            grains mode, offline: move every selected grain by up to N samples (0..1024) to where it lines up
                     best with its target frame (the shift of the least-squares fit; a grain stays inside its file)
  --gain-max X       grains mode, offline: scale every selected grain by the gain of that fit, at most X (float >= 0;
                     0: leave the corpus's level).  With either flag the summary line names both values, and --matches
                     holds (file, sample offset, distance, shift, gain) per candidate, or with --continuity the chosen
                     frame's shift and gain after the slot
  --live-fit N       with --live-block, grains mode: --fit for the live path.  Every corpus frame a block plays is
                     first moved by up to N samples (0..1024) to where it lines up best with the target frame it stands
                     for (with --lag L that frame is L frames old; the stream's input is kept on the device for it)
  --live-gain-max X  with --live-block, grains mode: --gain-max for the live path (float >= 0; 0: the corpus's level).
                     With either flag the summary line ends its live part with `, fit N, gain-max X` and --matches
                     gains the shift and gain columns in the offline layout

The corpus is the sorted *.wav in --corpus, each loaded at the .ini's sampling_rate and framed on its own.  Bad flag
values, an empty corpus, unreadable wavs or a --k above the number of corpus frames raise ValueError naming the flag or
the file.
"""
import argparse
import csv
import os
import sys

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, int_at_least, load_model, load_wav, nonneg_real,  # noqa: E402
                                             read_model_config, window_flag)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Latent audio mosaicing: resynthesise a target from a corpus's frames")
    add_model_flags(p, hop_help="frame hop (default: segment_length)")
    p.add_argument("--corpus", required=True, help="folder of the corpus's .wav files")
    p.add_argument("--target", required=True, help="the wav to resynthesise")
    p.add_argument("--out", required=True, help="output wav")
    p.add_argument("--k", default="1", help="neighbours per target frame (1..16)")
    p.add_argument("--mode", default="grains", help="grains | decode")
    p.add_argument("--window", default="none", help="none | hann")
    p.add_argument("--continuity", default="0", help="weight >= 0 of the concatenation cost (0: off)")
    p.add_argument("--matches", default=None, help="CSV of the k (file, offset, distance) triples per target frame")
    p.add_argument("--max-rows", default="16384", help="target frames per chunk")
    p.add_argument("--live-block", default=None, help="samples per block of the live path (default: offline)")
    p.add_argument("--streams", default=None, help="parallel streams of the live path (default 1)")
    p.add_argument("--lag", default=None, help="frames of look-ahead of the live path's unit selection (0..64, default 0)")
    p.add_argument("--fit", default=None, help="samples a grain may be shifted to fit its target frame (0..1024)")
    p.add_argument("--gain-max", default=None, help="largest gain of the fit (float >= 0; 0: no gain)")
    p.add_argument("--live-fit", default=None, help="--fit for the live path (0..1024; needs --live-block)")
    p.add_argument("--live-gain-max", default=None, help="--gain-max for the live path (needs --live-block)")
    args = p.parse_args(argv)
    int_at_least(args, "live-block", 1)
    if args.streams is not None and args.live_block is None:
        raise ValueError("--streams %s: needs --live-block" % args.streams)
    args.streams = int_at_least(args, "streams", 1) or 1
    int_at_least(args, "k", 1)
    if args.k > 16:
        raise ValueError("--k %d: at most 16" % args.k)
    nonneg_real(args, "continuity")
    if args.lag is not None:
        if args.live_block is None:
            raise ValueError("--lag %s: needs --live-block" % args.lag)
        int_at_least(args, "lag", 0)
        if args.lag > 64:
            raise ValueError("--lag %d: at most 64" % args.lag)
        if args.lag > 0 and args.continuity == 0:
            raise ValueError("--lag %d: needs --continuity > 0" % args.lag)
    args.lag = args.lag or 0
    int_at_least(args, "hop", 1)
    int_at_least(args, "max-rows", 1)
    if args.mode not in ("grains", "decode"):
        raise ValueError("--mode %r: expected grains or decode" % args.mode)
    window_flag(args)
    for flag, value in (("fit", args.fit), ("gain-max", args.gain_max)):
        if value is None:
            continue
        if args.live_block is not None:
            raise ValueError("--%s %s: fits the offline path only; with --live-block use --live-%s" % (flag, value, flag))
        if args.mode == "decode":
            raise ValueError("--%s %s: needs --mode grains, --mode decode plays no corpus audio" % (flag, value))
    args.fitted = args.fit is not None or args.gain_max is not None
    args.fit = int_at_least(args, "fit", 0) or 0
    if args.fit > 1024:
        raise ValueError("--fit %d: at most 1024" % args.fit)
    args.gain_max = nonneg_real(args, "gain-max") or 0.0
    for flag, value in (("live-fit", args.live_fit), ("live-gain-max", args.live_gain_max)):
        if value is None:
            continue
        if args.live_block is None:
            raise ValueError("--%s %s: needs --live-block" % (flag, value))
        if args.mode == "decode":
            raise ValueError("--%s %s: needs --mode grains, --mode decode plays no corpus audio" % (flag, value))
    args.live_fitted = args.live_fit is not None or args.live_gain_max is not None
    args.live_fit = int_at_least(args, "live-fit", 0) or 0
    if args.live_fit > 1024:
        raise ValueError("--live-fit %d: at most 1024" % args.live_fit)
    args.live_gain_max = nonneg_real(args, "live-gain-max") or 0.0
    if not os.path.isdir(args.corpus):
        raise ValueError("--corpus %r: not a folder" % args.corpus)
    return args


def check_framing(args, S):
    """--hop / --window against the model's segment_length; ValueError naming the flag."""
    from rawaudiovae_kelsey_amd.mosaic import check_window
    hop = S if args.hop is None else args.hop
    if S % hop != 0:
        raise ValueError("--hop %d: does not divide segment_length %d" % (hop, S))
    try:
        check_window(S, hop, args.window)
    except ValueError as e:
        raise ValueError("--window %s: %s" % (args.window, e))
    if args.live_block is not None and args.live_block % hop != 0:
        raise ValueError("--live-block %d: not a multiple of the hop %d" % (args.live_block, hop))
    return hop


def corpus_files(corpus_dir):
    """Sorted *.wav of corpus_dir (basenames); ValueError naming --corpus when there are none."""
    import glob
    files = sorted(os.path.basename(p) for p in glob.glob(os.path.join(corpus_dir, "*.wav")))
    if not files:
        raise ValueError("--corpus %r: no .wav files" % corpus_dir)
    return files


def write_matches(path, names_offsets, dist, slot=None, fit=None):
    """One line per target frame: file_1, offset_1, distance_1, ..., file_k, offset_k, distance_k[, chosen slot].
    fit = (shift, gain): [T, k] adds each candidate's shift and gain behind its distance; [T, 1] (the chosen frame's)
    adds the two behind the slot."""
    per_candidate = fit is not None and slot is None
    with open(path, "w", newline="") as f:
        wr = csv.writer(f)
        for t, (row, drow) in enumerate(zip(names_offsets, dist)):
            line = []
            for j, ((name, off), d) in enumerate(zip(row, drow)):
                line += [name if name is not None else "", off, repr(float(d))]
                if per_candidate:
                    line += [int(fit[0][t][j]), repr(float(fit[1][t][j]))]
            if slot is not None:
                line.append(int(slot[t]))
                if fit is not None:
                    line += [int(fit[0][t][0]), repr(float(fit[1][t][0]))]
            wr.writerow(line)


def main(argv=None):
    args = parse_args(argv)
    cfg = read_model_config(args.config)
    S, sr = cfg["segment_length"], cfg["sampling_rate"]
    hop = check_framing(args, S)
    files = corpus_files(args.corpus)
    waves = [load_wav(os.path.join(args.corpus, f), sr) for f in files]
    target = load_wav(args.target, sr)
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd.interpolate import frame_layout
    from rawaudiovae_kelsey_amd.mosaic import LatentIndex
    framing = None if args.hop is None else hop
    for f, w in zip(files, waves):
        if frame_layout(w.size, S, framing)[0] < 1:
            raise ValueError("%s: %d samples make no frame of %d samples at hop %d" % (
                os.path.join(args.corpus, f), w.size, S, hop))
    n_corpus = sum(frame_layout(w.size, S, framing)[0] for w in waves)
    if args.k > n_corpus:
        raise ValueError("--k %d: the corpus has only %d frames" % (args.k, n_corpus))
    if frame_layout(target.size, S, framing)[0] < 1:
        raise ValueError("--target %r: %d samples make no frame of %d samples at hop %d" % (args.target, target.size,
                                                                                           S, hop))
    model = load_model(args.checkpoint, cfg)
    index = LatentIndex(model, hop=framing, max_rows=args.max_rows)
    for f, w in zip(files, waves):
        index.add(w, f)
    if args.live_block is not None:
        return run_live(args, index, target, hop, sr, len(files))
    y, idx, dist, path, fits = index.mosaic(target, k=args.k, mode=args.mode, window=args.window, return_matches=True,
                                            continuity=args.continuity, return_path=True, fit=args.fit,
                                            gain_max=args.gain_max, return_fit=True)
    y = y.cpu().numpy()
    D.write_wav(args.out, y, sr)
    slot = None if path is None else path[0].cpu().numpy()
    if args.fitted and fits is not None:
        fits = (fits[0].cpu().numpy(), fits[1].cpu().numpy())
    if args.matches:
        write_matches(args.matches, index.locate(idx), dist.cpu().numpy(), slot, fits if args.fitted else None)
    line = ("wrote %s: %d samples from %d target frames, %d corpus frames in %d files, k %d, mode %s, window %s"
            % (args.out, y.size, idx.shape[0], len(index), len(files), args.k, args.mode, args.window or "none"))
    if args.fitted:
        line += ", fit %d, gain-max %g" % (args.fit, args.gain_max)
    if path is not None:
        choice, cost = path[1].cpu().numpy(), path[2].cpu().numpy()
        line += (", continuity %g, continuing %.4f, target cost %.6g, transition cost %.6g"
                 % (args.continuity, continuing_share(choice, index.successor()), cost[0], cost[1]))
    print(line)
    return y


def live_mosaic(index, target, block, hop, n_streams=1, **kw):
    """The target through StreamingMosaic in blocks of `block` -> (y [target.size] numpy, idx [T, k], dist [T, k],
    choice [T]) with T the frames of all streams, stream after stream.  The target is cut into n_streams consecutive
    parts; every part is zero-padded to whole blocks that also flush the S - hop samples of latency.  With lag=N the
    frames still held back are drained, the output is cut N * hop samples later, and choice[t] is the frame committed
    for frame t (N frames after its candidates were found).  With fit= / gain_max= (StreamingMosaic's) a fifth element
    holds the fits (shift, gain, score), each [T, kf] numpy and aligned with choice: row t is frame t's fit."""
    import numpy as np
    import torch
    from rawaudiovae_kelsey_amd.mosaic import StreamingMosaic
    sm = StreamingMosaic(index, n_streams, block, hop=hop, **kw)
    n = target.size
    part = -(-n // n_streams)
    n_blocks = -(-(part + sm.latency) // block)
    x = np.zeros((n_streams, n_blocks * block), np.float32)
    for s in range(n_streams):
        seg = target[s * part:(s + 1) * part]
        x[s, :seg.size] = seg
    x = torch.from_numpy(x).to(sm.device)
    ys, idxs, dists, choices, fits = [], [], [], [], []
    for b in range(n_blocks):
        ys.append(sm.process(x[:, b * block:(b + 1) * block]))
        i, d, c = sm.last_matches()
        idxs.append(i.clone()), dists.append(d.clone()), choices.append(c.clone())
        if sm.fitted:
            fits.append([t.clone() for t in sm.last_fit()])
    for b in range(-(-sm.lag_samples // block)):                 # every frame fed is committed and played
        ys.append(sm.drain())
        choices.append(sm.last_matches()[2].clone())
        if sm.fitted:
            fits.append([t.clone() for t in sm.last_fit()])
    late = sm.latency + sm.lag_samples
    y = torch.cat(ys, 1)[:, late:late + part].reshape(-1)[:n].cpu().numpy()
    k = idxs[0].shape[-1]
    frames = n_blocks * sm.frames_per_block
    choice = torch.cat(choices, 1)[:, sm.lag:sm.lag + frames]
    res = (y, torch.cat(idxs, 1).reshape(-1, k).cpu().numpy(), torch.cat(dists, 1).reshape(-1, k).cpu().numpy(),
           choice.reshape(-1).cpu().numpy())
    if sm.fitted:
        parts = [torch.cat(p, 1)[:, sm.lag:sm.lag + frames] for p in zip(*fits)]
        res += (tuple(p.reshape(-1, p.shape[-1]).cpu().numpy() for p in parts),)
    return res


def _live_rule(args):
    if args.continuity > 0:
        return "live, lag %d" % args.lag if args.lag > 0 else "live, greedy"
    return "live"


def run_live(args, index, target, hop, sr, n_files):
    from rawaudiovae_kelsey_amd import data as D
    fits = None
    kw = dict(k=args.k, mode=args.mode, window=args.window, continuity=args.continuity, lag=args.lag)
    if args.live_fitted:
        kw.update(fit=args.live_fit, gain_max=args.live_gain_max)
    y, idx, dist, choice, *rest = live_mosaic(index, target, args.live_block, hop, args.streams, **kw)
    if rest:                                                     # fitted: fit 0 with gain-max 0 fits nothing
        fits = rest[0][:2]
    D.write_wav(args.out, y, sr)
    slot = None
    if args.continuity > 0:
        slot = [int((idx[t] == choice[t]).argmax()) if choice[t] >= 0 else -1 for t in range(len(choice))]
    if args.matches:
        write_matches(args.matches, index.locate(idx), dist, slot, fits)
    line = ("wrote %s: %d samples from %d target frames, %d corpus frames in %d files, k %d, mode %s, window %s, %s, "
            "block %d, streams %d" % (args.out, y.size, idx.shape[0], len(index), n_files, args.k, args.mode,
                                      args.window or "none", _live_rule(args),
                                      args.live_block, args.streams))
    if args.live_fitted:
        line += ", fit %d, gain-max %g" % (args.live_fit, args.live_gain_max)
    if args.continuity > 0:
        line += ", continuity %g, continuing %.4f" % (
            args.continuity, continuing_share(choice, index.successor(hop // index.step)))
    print(line)
    return y


def continuing_share(choice, next_of):
    """The share of frames t >= 1 whose corpus frame is the successor of frame t - 1's (1.0 for a single frame)."""
    if len(choice) < 2:
        return 1.0
    prev, cur = choice[:-1], choice[1:]
    ok = (prev >= 0) & (cur >= 0)
    hit = ok & (cur == next_of[prev.clip(min=0)])
    return float(hit.sum()) / (len(choice) - 1)


if __name__ == "__main__":
    main()
