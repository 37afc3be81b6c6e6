"""`python compose.py fit --config default.ini --checkpoint ckpt_00500 --data DIR_OR_WAV --states states.npz --hop 256 --out form.npz`
`python compose.py run --config default.ini --checkpoint ckpt_00500 --model form.npz --seconds 10 --out out.wav --hop 256
        --window hann --form A:2,B:1.5,*:4,A:2 --labels labels.json`

Audio with form: a switching walk (rawaudiovae_kelsey_amd.switching), on the GPU.  The states of `states.py fit` are kinds
of sound; here every state gets its own frame-to-frame dynamics, and a form says which state plays when.

fit encodes every frame of a wav, or of every *.wav of a folder (sorted by name), to its mu, computes the states' posteriors
and fits one linear-Gaussian law per state under them, the files kept apart.  It writes one .npz
(switching.write_switching) and prints one JSON line: per state its letter, pairs (the weight of frame pairs it was fitted
on), predictability (the share of the standardised variance one step explains), shrink (the contraction guard's factor, 1
where it did not act) and flag (1: fewer than two pairs, the state has no dynamics of its own).

run generates --seconds of audio block by block (switching.StreamingSwitchingWalk):

  --form L:SEC,...   the plan: state L (a letter of `states.py label`: A the first state; beyond Z the state's number) for SEC
                     seconds, rounded to frames; * runs free (the states follow the transition matrix).  A form shorter than
                     --seconds continues free; without --form everything runs free
  --hop N            frame hop; it must be the hop the model was fitted at
  --window hann|none overlap-add window (default none: rectangular)
  --temperature T    scale of the noise that drives the walk (default 1)
  --seed N           Philox seed; the same seed gives the same file
  --streams N        N independent walks under the same form, written as OUT_0.wav .. OUT_{N-1}.wav
  --start in.wav     start every stream from the wav's last frame: its likeliest state and its residual there
  --labels F.json    write the states that played as the object `states.py label` writes (with --streams N > 1:
                     F_0.json ..), so `segment.py split` cuts the result

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

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, check_exists, check_fitted, data_files, encode_wav,  # noqa: E402
                                             load_wav, nonneg, nonneg_int, number_flag, open_model, positive, positive_int,
                                             window_flag)

HOP_PHRASES = ("the switching walk was", "one step of the walk is one frame at that hop")
FREE = -1


def parse_form(text, flag="form"):
    """[(state or FREE, seconds)] of "A:2,B:1.5,*:4": a letter A..Z is state 0..25, a number >= 26 that state, * free;
    ValueError naming the flag for anything else, or a duration that is not finite and positive."""
    out = []
    for item in str(text).split(","):
        name, sep, sec = item.strip().partition(":")
        name = name.strip()
        try:
            if not sep:
                raise ValueError
            seconds = float(sec)
        except ValueError:
            raise ValueError("--%s %r: expected LETTER:SECONDS,... (* runs free), got %r" % (flag, text, item))
        if not 0 < seconds < float("inf"):
            raise ValueError("--%s %r: %r: the duration must be a finite number of seconds > 0" % (flag, text, item))
        if name == "*":
            state = FREE
        elif len(name) == 1 and "A" <= name <= "Z":
            state = ord(name) - ord("A")
        elif name.isdigit() and int(name) >= 26:
            state = int(name)
        else:
            raise ValueError("--%s %r: unknown letter %r: expected A..Z, a state number >= 26 or *" % (flag, text, name))
        out.append((state, seconds))
    return out


def check_form(form, n_states, text, flag="form"):
    """The form's states against the model's; ValueError naming the flag and the letter."""
    from rawaudiovae_kelsey_amd.structure import form as letters
    for state, _ in form:
        if state >= n_states:
            raise ValueError("--%s %r: unknown letter %s: the model has %d states (%s)" % (
                flag, text, letters([state]), n_states, letters([0]) + (" .. " + letters([n_states - 1]) if n_states > 1 else "")))
    return form


def form_frames(form, frames, sampling_rate, hop):
    """forced [frames] int32: every part's seconds rounded to frames (at least one), cut at `frames`; FREE beyond the form"""
    forced = np.full(frames, FREE, dtype=np.int32)
    at = 0
    for state, seconds in form:
        n = max(1, int(round(seconds * sampling_rate / hop)))
        forced[at:at + n] = state
        at += n
        if at >= frames:
            break
    return forced


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Audio with form: a switching walk over a corpus's latent states on the GPU")
    sub = p.add_subparsers(dest="command")
    for name in ("fit", "run"):
        s = sub.add_parser(name)
        add_model_flags(s)
        s.add_argument("--out", required=True, help="fit: the .npz; run: the output wav")
        if name == "fit":
            s.add_argument("--data", required=True, help="a wav, or a folder whose *.wav are encoded")
            s.add_argument("--states", required=True, help="the .npz of states.py fit")
        else:
            s.add_argument("--model", required=True, help="the .npz written by fit")
            s.add_argument("--seconds", required=True, help="length of the output")
            s.add_argument("--window", default="none", help="none | hann")
            s.add_argument("--temperature", default="1", help="scale of the driving noise")
            s.add_argument("--seed", default="0", help="Philox seed")
            s.add_argument("--streams", default="1", help="independent walks, one file each")
            s.add_argument("--start", default=None, help="a wav whose last frame seeds the state")
            s.add_argument("--form", default=None, help="LETTER:SECONDS,...; * runs free")
            s.add_argument("--labels", default=None, help="write the states that played as a segments .json")
    args = p.parse_args(argv)
    if args.command is None:
        raise ValueError("expected a command: fit or run")
    positive_int(args, "hop")
    if args.command == "fit":
        return args
    positive_int(args, "streams")
    nonneg_int(args, "seed")
    number_flag(args, "seconds", float, positive, "a finite positive number")
    number_flag(args, "temperature", float, nonneg, "a finite non-negative number")
    window_flag(args)
    args.form_text = args.form
    args.form = [] if args.form is None else parse_form(args.form)
    return args


def out_paths(out, n_streams):
    """The files of a run: `out` itself, or OUT_0.ext .. with --streams N > 1."""
    if n_streams == 1:
        return [out]
    stem, ext = os.path.splitext(out)
    return ["%s_%d%s" % (stem, s, ext) for s in range(n_streams)]


def fit(args):
    from rawaudiovae_kelsey_amd import states as ST
    from rawaudiovae_kelsey_amd import switching as SW
    from rawaudiovae_kelsey_amd.structure import form as letters
    check_exists("states", args.states)
    files = data_files(args.data)
    cfg, model, _ = open_model(args)
    try:
        st, meta = ST.read_states(args.states, model.fc1.weight.device)
    except ValueError as e:
        raise ValueError("--states: %s" % e)
    check_fitted("states", args.states, meta, cfg, args.hop, "the states were", "a transition is one frame at that hop")
    waves = [load_wav(f, cfg["sampling_rate"]) for f in files]
    try:
        sw = SW.fit_corpus(model, waves, st, args.hop)
    except ValueError as e:
        raise ValueError("--data %r: %s" % (args.data, e))
    SW.write_switching(args.out, sw, cfg["segment_length"], args.hop)
    report = dict(n_frames=sw.n_frames_, n_files=sw.n_files_, keep=sw.n_components,
                  states=[dict(letter=letters([s]), pairs=float(sw.pairs_[s]), predictability=float(sw.predictability_[s]),
                               shrink=float(sw.shrink_[s]), flag=int(sw.info_[s])) for s in range(sw.n_states)])
    print(json.dumps(report))
    return report


def run(args):
    import torch
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import switching as SW
    from rawaudiovae_kelsey_amd.codec import FrameCodec
    from rawaudiovae_kelsey_amd.stream import check_args
    from states import segments_report
    for flag, path in (("model", args.model), ("start", args.start)):
        if path is not None:
            check_exists(flag, path)
    cfg, model, _ = open_model(args)
    S, sr = cfg["segment_length"], cfg["sampling_rate"]
    try:
        sw, meta = SW.read_switching(args.model, model.fc1.weight.device)
    except ValueError as e:
        raise ValueError("--model: %s" % e)
    hop = check_fitted("model", args.model, meta, cfg, args.hop, *HOP_PHRASES)
    check_form(args.form, sw.n_states, args.form_text)
    try:
        check_args(S, hop, hop, args.window)
    except ValueError as e:
        raise ValueError("--window %s: %s" % (args.window or "none", e))
    n = int(round(args.seconds * sr))
    if n < 1:
        raise ValueError("--seconds %r: no sample at %d Hz" % (args.seconds, sr))
    # blocks of up to 16 frames: the audio does not depend on the block length
    frames = -(-n // hop)
    per = min(16, frames)
    blocks = -(-frames // per)
    forced = np.full(blocks * per, FREE, dtype=np.int32)
    forced[:frames] = form_frames(args.form, frames, sr, hop)
    gen = SW.StreamingSwitchingWalk(model, sw, args.streams, per * hop, hop, args.window, args.seed)
    gen.temperature.fill_(args.temperature)
    if args.start is not None:
        _, mu, _, T = encode_wav(FrameCodec(model), load_wav(args.start, sr), args.hop, "start", args.start)
        gen.prime(mu[T - 1])
    ys, paths_played = [], []
    with torch.no_grad():
        for b in range(blocks):
            plan = torch.from_numpy(forced[b * per:(b + 1) * per]).to(gen.device)
            ys.append(gen.generate(states=plan.view(1, per).expand(args.streams, per).contiguous()))
            paths_played.append(gen.last_states().clone())
    y = torch.cat(ys, 1)[:, :n].cpu().numpy()
    played = torch.cat(paths_played, 1)[:, :frames].cpu().numpy()
    paths = out_paths(args.out, args.streams)
    for path, row in zip(paths, y):
        D.write_wav(path, row, sr)
    if args.labels is not None:
        for path, row in zip(out_paths(args.labels, args.streams), played):
            with open(path, "w") as f:
                json.dump(segments_report(row, 0.0, n, sr, hop, sw.n_states), f)
    print("wrote %s: %d samples per stream, hop %d, window %s, %d states on %d axes, temperature %g, seed %d"
          % (", ".join(paths), n, hop, args.window or "none", sw.n_states, sw.n_components, args.temperature, args.seed))
    return y, played


def main(argv=None):
    args = parse_args(argv)
    return fit(args) if args.command == "fit" else run(args)


if __name__ == "__main__":
    main()
