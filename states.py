"""`python states.py fit   --config default.ini --checkpoint ckpt_00500 --data DIR_OR_WAV --pca pca.npz --states 8 --keep 16
        --hop 256 --out states.npz`
`python states.py label --config default.ini --checkpoint ckpt_00500 --states states.npz --in in.wav --out segments.json`
`python states.py score --config default.ini --checkpoint ckpt_00500 --states states.npz --in in.wav`

Latent states: a hidden Markov model of a corpus (rawaudiovae_kelsey_amd.states), on the GPU.  Its states are kinds of
sound that mean the same in every file, its transition matrix says what follows what and for how long.

fit    encodes every frame of a wav, or of every *.wav of a folder (sorted by name), to its mu and fits S Gaussian states
       over the first K whitened principal axes by EM, the files kept apart.  It prints the iterations, the final
       log-likelihood per frame and every state's occupancy and mean duration 1 / (1 - A_ss) in frames, then the same as
       one JSON line, and writes one .npz (states.write_states).
  --pca F.npz        the axes: a file of `latent_pca.py fit` or `generate.py fit` at the same hop (default: the corpus's own)
  --states S         states (default 8, at most 64)
  --keep K           whitened axes the states see (default 16, at most 64 and the rank)
  --iters N          EM iterations at most (default 50)
  --tol X            stop once an iteration gains less than X per frame (default 1e-4; 0: never)
  --floor V          variance floor in whitened units (default 1e-3)
  --seed N           the seed of the initial means
label  writes the Viterbi path of in.wav as the JSON object `segment.py find` writes (boundaries in frames, samples and
       seconds, the segments' sample offsets, the labels and the form), so `segment.py split` cuts it unchanged.  The
       letters are the model's states: A is the same kind of sound in every file.
score  prints the log-likelihood of in.wav per frame and, for every state, its share of the frames and the mean
       log-density of the frames it explains.

--hop must be the hop the states were fitted at.  Bad flag values raise ValueError naming the flag.
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
                                             load_wav, nonneg_int, nonneg_real, open_model, positive_int, positive_real)

COMMANDS = ("fit", "label", "score")
HOP_PHRASES = ("the states were", "a transition is one frame at that hop")


def parse_args(argv=None):
    from rawaudiovae_kelsey_amd.states import K_MAX, S_MAX
    p = argparse.ArgumentParser(description="Latent states: a Gaussian hidden Markov model of a corpus on the GPU")
    sub = p.add_subparsers(dest="command")
    for name in COMMANDS:
        s = sub.add_parser(name)
        add_model_flags(s)
        if name == "fit":
            s.add_argument("--data", required=True, help="a wav, or a folder whose *.wav are encoded")
            s.add_argument("--pca", default=None, help="the .npz of latent_pca.py fit or generate.py fit")
            s.add_argument("--states", default="8", help="states (default 8)")
            s.add_argument("--keep", default="16", help="whitened axes the states see (default 16)")
            s.add_argument("--iters", default="50", help="EM iterations at most (default 50)")
            s.add_argument("--tol", default="1e-4", help="stop below this gain per frame (default 1e-4)")
            s.add_argument("--floor", default="1e-3", help="variance floor (default 1e-3)")
            s.add_argument("--seed", default="0", help="seed of the initial means")
            s.add_argument("--out", required=True, help="the .npz")
        else:
            s.add_argument("--states", required=True, help="the .npz written by fit")
            s.add_argument("--in", dest="wav", required=True, help="the wav")
            if name == "label":
                s.add_argument("--out", required=True, help="the .json")
    args = p.parse_args(argv)
    if args.command is None:
        raise ValueError("expected a command: fit, label or score")
    positive_int(args, "hop")
    if args.command == "fit":
        for flag, hi in (("states", S_MAX), ("keep", K_MAX)):
            if positive_int(args, flag) > hi:
                raise ValueError("--%s %d: at most %d" % (flag, getattr(args, flag), hi))
        positive_int(args, "iters")
        nonneg_int(args, "seed")
        nonneg_real(args, "tol")
        positive_real(args, "floor")
    return args


def read_axes(path, cfg, hop, device):
    """The fitted axes of --pca: a latent-walk file or a latent-PCA file, at this model's shape and this hop."""
    from rawaudiovae_kelsey_amd import pca as P
    from rawaudiovae_kelsey_amd import walk as W
    check_exists("pca", path)
    with np.load(path) as z:
        is_walk = "dynamics" in z.files
    try:
        axes, meta = (W.read_walk if is_walk else P.read_pca)(path, device)
    except ValueError as e:
        raise ValueError("--pca: %s" % e)
    check_fitted("pca", path, meta, cfg, hop, "the axes were", HOP_PHRASES[1])
    return axes


def fit(args):
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd.corpus import encode_corpus
    cfg, model, _ = open_model(args)
    files = data_files(args.data)
    axes = None if args.pca is None else read_axes(args.pca, cfg, args.hop, model.fc1.weight.device)
    waves = [load_wav(f, cfg["sampling_rate"]) for f in files]
    try:
        x, starts = encode_corpus(model, waves, args.hop)
        st = ST.LatentStates(args.states, args.keep, args.floor)
        st.fit(x, starts, axes, args.iters, args.tol, args.seed)
    except ValueError as e:
        raise ValueError("--data %r / --states %s / --keep %s: %s" % (args.data, args.states, args.keep, e))
    ST.write_states(args.out, st, cfg["segment_length"], args.hop)
    occupancy = st.posteriors(x, starts).sum(dim=0).cpu().numpy() / x.shape[0]
    report = dict(n_frames=st.n_frames_, n_files=st.n_files_, states=st.n_states, keep=st.n_components,
                  iterations=st.n_iter_, loglik_per_frame=st.ll_history_[-1] / st.n_frames_,
                  occupancy=[float(v) for v in occupancy], duration=[float(v) for v in st.durations_],
                  kept_emission=[int(v) for v in st.info_.cpu().numpy()])
    print("%d iterations, log-likelihood per frame %.6g" % (report["iterations"], report["loglik_per_frame"]))
    for s in range(st.n_states):
        print("state %s: occupancy %.4f, mean duration %.4g frames" % (_letter(s), occupancy[s], report["duration"][s]))
    print(json.dumps(report))
    return report


def _letter(s):
    from rawaudiovae_kelsey_amd.structure import form
    return form([s])


def _encode(args):
    """(states, cfg, the wav, its mu [T, L], row_start, the frame step in samples)"""
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    check_exists("states", args.states)
    cfg, model, _ = open_model(args)
    try:
        st, meta = ST.read_states(args.states, model.fc1.weight.device)
    except ValueError as e:
        raise ValueError("--states: %s" % e)
    step = check_fitted("states", args.states, meta, cfg, args.hop, *HOP_PHRASES)
    wave = load_wav(args.wav, cfg["sampling_rate"])
    _, mu, _, T = encode_wav(FrameCodec(model), wave, args.hop, "in", args.wav)
    return st, cfg, wave, mu, np.asarray([0, T], dtype=np.int64), step


def segments_report(path, score, n_samples, sampling_rate, step, n_states):
    """The object `segment.py find` writes, of a state path [frames]: a segment is a maximal run of one state, its label
    the state's number (so its letter is the same in every file); also the states and the path's score."""
    from rawaudiovae_kelsey_amd.states import runs
    from rawaudiovae_kelsey_amd.structure import form
    offsets, labels = runs(path)
    frames = offsets[1:-1]
    samples = frames * int(step)
    return dict(segments=int(labels.size), frames=int(np.asarray(path).size), samples=int(n_samples),
                sampling_rate=int(sampling_rate), hop=int(step), states=int(n_states), score=float(score),
                boundary_frames=[int(v) for v in frames], boundary_samples=[int(v) for v in samples],
                boundary_seconds=[float(v) / sampling_rate for v in samples],
                sample_offsets=[0] + [int(v) for v in samples] + [int(n_samples)], labels=[int(v) for v in labels],
                form=form(labels))


def label(args):
    st, cfg, wave, mu, rs, step = _encode(args)
    path, score = st.label(mu, rs)
    path, score = path.cpu().numpy(), float(score.cpu().numpy()[0])
    if (path < 0).any():
        raise ValueError("--in %r: no state sequence of the model explains the recording" % args.wav)
    report = segments_report(path, score, int(wave.size), cfg["sampling_rate"], step, st.n_states)
    with open(args.out, "w") as f:
        json.dump(report, f)
    print("%d segments, boundaries at %s s, form %s" % (
        report["segments"], " ".join("%.6g" % v for v in report["boundary_seconds"]) or "-", report["form"]))
    print(json.dumps(report))
    return report


def score(args):
    from rawaudiovae_kelsey_amd import states as ST
    st, cfg, wave, mu, rs, step = _encode(args)
    T = mu.shape[0]
    ll = float(st.loglik(mu, rs).cpu().numpy()[0])
    gamma = st.posteriors(mu, rs)
    logb = ST.emit(mu, st.mean_, st.P_, st.theta_, st.n_states)
    occ = gamma.sum(dim=0)
    dens = ((gamma * logb).sum(dim=0) / occ).cpu().numpy()
    occ = occ.cpu().numpy() / T
    report = dict(frames=int(T), loglik=ll, loglik_per_frame=ll / T, occupancy=[float(v) for v in occ],
                  state_loglik=[float(v) if np.isfinite(v) else None for v in dens])
    print("%d frames, log-likelihood per frame %.6g" % (T, report["loglik_per_frame"]))
    for s in range(st.n_states):
        print("state %s: share %.4f, mean log-density %s" % (
            _letter(s), occ[s], "-" if report["state_loglik"][s] is None else "%.6g" % report["state_loglik"][s]))
    print(json.dumps(report))
    return report


def main(argv=None):
    args = parse_args(argv)
    return {"fit": fit, "label": label, "score": score}[args.command](args)


if __name__ == "__main__":
    main()
