"""`python transfer.py fit   --config default.ini --checkpoint ckpt_00500 --source DIR_OR_WAV --target DIR_OR_WAV [--pca pca.npz]
        --keep 16 --hop 256 --epsilon 0.05 --iters 500 --tol 1e-3 [--max-frames 65536] --out transport.npz`
`python transfer.py apply --config default.ini --checkpoint ckpt_00500 --transport transport.npz --in in.wav --out out.wav
        --hop 256 --window hann --amount 1.0 [--reverse] [--live-block 256]`

Latent timbre transfer (rawaudiovae_kelsey_amd.transport), on the GPU: play a recording with the sound of another corpus,
keeping its gestures.  An entropic optimal-transport plan between the two corpora's latent clouds sends the source
distribution onto the target distribution as a whole; its barycentric map moves every frame of a new recording.

fit    encodes every frame of --source and of --target (a wav, or every *.wav of a folder sorted by name) to its mu, whitens
       both into the first K principal axes and runs Sinkhorn between the two clouds.  It prints the frames on each side,
       epsilon, the iterations, the marginal error, the transport cost per frame with its square root (the distance between
       the two corpora in whitened units) and the median support, then the same as one JSON line, and writes one .npz
       (transport.write_transport).
  --pca F.npz        the axes: a file of `latent_pca.py fit` or `generate.py fit` at the same hop (default: the PCA of both
                     corpora together)
  --keep K           whitened axes the transport sees (default 16, at most 64 and the rank)
  --epsilon X        the entropic regularisation as a fraction of the mean cost between the clouds (default 0.05)
  --iters N          Sinkhorn iterations at the target epsilon at most (default 500)
  --tol X            stop once the L1 violation of the target's marginal is at most X (default 1e-3; 0: never)
  --max-frames N     at most N frames per side: every ceil(T / N)-th frame is kept (deterministic, printed; default 65536)
apply  maps every frame of in.wav and writes the resynthesis.  It prints the mean support (the effective number of target
       frames behind a frame) and the mean squared displacement in whitened units.
  --amount A         how far every frame moves towards its image (default 1; 0: the plain resynthesis)
  --reverse          turn the target's material into the source's manner with the same file
  --live-block N     run through the live path instead (StreamingTransport): blocks of N samples (a multiple of the hop); the
                     file is the same as the offline path's, bit for bit
  Both paths frame the recording from S - hop samples of silence before it to as many after it, so that every sample is
  covered by its full set of frames.

--hop must be the hop the transport was fitted at.  Bad flag values raise ValueError naming the flag.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from rawaudiovae_kelsey_amd.frontend import (add_model_flags, check_exists, check_fitted, data_files, flagged,  # noqa: E402
                                             int_at_least, load_wav, nonneg_real, number_flag, open_model, positive_int,
                                             positive_real, window_flag)

COMMANDS = ("fit", "apply")
HOP_PHRASES = ("the transport was", "the map moves one frame at that hop")


def parse_args(argv=None):
    from rawaudiovae_kelsey_amd.transport import K_MAX
    p = argparse.ArgumentParser(description="Latent timbre transfer: entropic optimal transport between two corpora on the GPU")
    sub = p.add_subparsers(dest="command")
    for name in COMMANDS:
        s = sub.add_parser(name)
        add_model_flags(s)
        if name == "fit":
            s.add_argument("--source", required=True, help="a wav, or a folder whose *.wav are the source corpus")
            s.add_argument("--target", required=True, help="a wav, or a folder whose *.wav are the target corpus")
            s.add_argument("--pca", default=None, help="the .npz of latent_pca.py fit or generate.py fit")
            s.add_argument("--keep", default="16", help="whitened axes the transport sees (default 16)")
            s.add_argument("--epsilon", default="0.05", help="regularisation as a fraction of the mean cost (default 0.05)")
            s.add_argument("--iters", default="500", help="Sinkhorn iterations at the target epsilon at most (default 500)")
            s.add_argument("--tol", default="1e-3", help="stop at this marginal error (default 1e-3)")
            s.add_argument("--max-frames", default="65536", help="frames per side at most (default 65536)")
            s.add_argument("--out", required=True, help="the .npz")
        else:
            s.add_argument("--transport", required=True, help="the .npz written by fit")
            s.add_argument("--in", dest="wav", required=True, help="the wav")
            s.add_argument("--out", required=True, help="the wav to write")
            s.add_argument("--window", default="none", help="none | hann")
            s.add_argument("--amount", default="1.0", help="how far every frame moves towards its image (default 1)")
            s.add_argument("--reverse", action="store_true", help="map the target's material into the source's manner")
            s.add_argument("--live-block", default=None, help="samples per block of the live path (default: offline)")
    args = p.parse_args(argv)
    if args.command is None:
        raise ValueError("expected a command: fit or apply")
    positive_int(args, "hop")
    if args.command == "fit":
        if positive_int(args, "keep") > K_MAX:
            raise ValueError("--keep %d: at most %d" % (args.keep, K_MAX))
        positive_real(args, "epsilon")
        positive_int(args, "iters")
        nonneg_real(args, "tol")
        positive_int(args, "max-frames")
    else:
        window_flag(args)
        number_flag(args, "amount", float, lambda x: abs(x) < float("inf"), "a finite number")
        int_at_least(args, "live-block", 1)
    return args


def thin(T, max_frames):
    """The stride ceil(T / max_frames) that keeps at most max_frames of T frames"""
    return -(-int(T) // int(max_frames))


def _corpus(flag, path, model, cfg, hop, max_frames):
    """(mu of every `stride`-th frame, frames before thinning, stride) of the wavs --flag names"""
    from rawaudiovae_kelsey_amd.corpus import encode_corpus
    try:
        files = data_files(path)
    except ValueError as e:
        raise ValueError(str(e).replace("--data", "--" + flag))
    waves = [load_wav(f, cfg["sampling_rate"]) for f in files]
    x, _ = flagged("--%s %r" % (flag, path), lambda: encode_corpus(model, waves, hop))
    stride = thin(x.shape[0], max_frames)
    return x[::stride].contiguous(), x.shape[0], stride


def fit(args):
    from rawaudiovae_kelsey_amd import transport as TR
    from states import read_axes
    cfg, model, _ = open_model(args)
    axes = None if args.pca is None else read_axes(args.pca, cfg, args.hop, model.fc1.weight.device)
    xs, Ts, ss = _corpus("source", args.source, model, cfg, args.hop, args.max_frames)
    xt, Tt, st = _corpus("target", args.target, model, cfg, args.hop, args.max_frames)
    tr = TR.LatentTransport(args.keep, args.epsilon, args.iters, args.tol)
    flagged("--source %r / --target %r / --keep %s" % (args.source, args.target, args.keep), lambda: tr.fit(xs, xt, axes))
    TR.write_transport(args.out, tr, cfg["segment_length"], args.hop)
    support = tr.map(xs, 0.0)[1]["support"].cpu().numpy()
    report = dict(source_frames=int(xs.shape[0]), target_frames=int(xt.shape[0]), source_stride=ss, target_stride=st,
                  source_frames_read=int(Ts), target_frames_read=int(Tt), keep=tr.n_components, epsilon=tr.epsilon_,
                  mean_cost=tr.mean_cost_, iterations=tr.n_iter_, marginal_error=tr.err_, cost_per_frame=tr.cost_,
                  distance=float(np.sqrt(max(tr.cost_, 0.0))), median_support=float(np.median(support[support > 0])))
    print("source: %d of %d frames (every %d), target: %d of %d frames (every %d)" % (xs.shape[0], Ts, ss, xt.shape[0], Tt, st))
    print("epsilon %.6g (%.4g x the mean cost %.6g), %d iterations, marginal error %.3g" % (
        tr.epsilon_, tr.epsilon, tr.mean_cost_, tr.n_iter_, tr.err_))
    print("transport cost per frame %.6g, distance between the corpora %.6g, median support %.4g target frames" % (
        report["cost_per_frame"], report["distance"], report["median_support"]))
    print(json.dumps(report))
    return report


def live_transfer(model, x, transport, block, hop, window, amount, reverse):
    """x (numpy, 1-D) through StreamingTransport in blocks -> (y [len(x)] numpy, support, displacement per frame): the
    recording followed by S - hop samples of silence, zero-padded to whole blocks; the latency is dropped"""
    import torch
    from rawaudiovae_kelsey_amd import transport as TR
    st = TR.StreamingTransport(model, transport, 1, block, hop, window, amount, reverse)
    n = x.size
    m = -(-(n + st.latency) // block) * block
    fed = np.zeros(m, np.float32)
    fed[:n] = x
    fed = torch.from_numpy(fed).to(st.device)
    ys, sup, dis = [], [], []
    for b in range(m // block):
        ys.append(st.process(fed[b * block:(b + 1) * block]).clone())
        d = st.last_diagnostics()
        sup.append(d["support"].reshape(-1).clone())
        dis.append(TR.displacement(transport, st.last_latents()[0].reshape(-1, st.L), d["coords"], amount))
    y = torch.cat(ys, 1)[0, st.latency:st.latency + n]
    return y.cpu().numpy(), torch.cat(sup).cpu().numpy(), torch.cat(dis).cpu().numpy()


def offline_transfer(model, x, transport, hop, window, amount, reverse):
    """x (numpy, 1-D) through transport.transfer between S - hop samples of silence on either side, which are dropped"""
    from rawaudiovae_kelsey_amd import transport as TR
    S = int(model.segment_length)
    lat = S - (S if hop is None else int(hop))
    w = np.concatenate([np.zeros(lat, np.float32), np.asarray(x, np.float32), np.zeros(lat, np.float32)])
    y, diag = TR.transfer(model, w, transport, hop, window, amount, reverse)
    moved = TR.displacement(transport, diag["mu"], diag["coords"], amount)
    return y[lat:lat + x.size].cpu().numpy(), diag["support"].cpu().numpy(), moved.cpu().numpy()


def apply(args):
    from rawaudiovae_kelsey_amd import data as D
    from rawaudiovae_kelsey_amd import transport as TR
    from rawaudiovae_kelsey_amd.mosaic import check_window
    check_exists("transport", args.transport)
    cfg, model, step = open_model(args)
    try:
        tr, meta = TR.read_transport(args.transport, model.fc1.weight.device)
    except ValueError as e:
        raise ValueError("--transport: %s" % e)
    check_fitted("transport", args.transport, meta, cfg, args.hop, *HOP_PHRASES)
    flagged("--window %s" % (args.window or "none"), lambda: check_window(cfg["segment_length"], step, args.window))
    if args.live_block is not None and args.live_block % step != 0:
        raise ValueError("--live-block %d: not a multiple of the hop %d" % (args.live_block, step))
    x = load_wav(args.wav, cfg["sampling_rate"])
    if args.live_block is not None:
        y, support, moved = live_transfer(model, x, tr, args.live_block, args.hop, args.window, args.amount, args.reverse)
    else:
        y, support, moved = offline_transfer(model, x, tr, args.hop, args.window, args.amount, args.reverse)
    D.write_wav(args.out, y, cfg["sampling_rate"])
    ok = support > 0
    report = dict(samples=int(y.size), frames=int(support.size), mapped_frames=int(ok.sum()), amount=args.amount,
                  reverse=bool(args.reverse), live_block=args.live_block,
                  mean_support=float(support[ok].mean()) if ok.any() else 0.0,
                  mean_squared_displacement=float(moved[ok].mean()) if ok.any() else 0.0)
    print("wrote %s: %d samples, %d frames, amount %g%s%s, mean support %.4g target frames, mean squared displacement %.6g" % (
        args.out, y.size, support.size, args.amount, ", reversed" if args.reverse else "",
        "" if args.live_block is None else ", live blocks of %d" % args.live_block, report["mean_support"],
        report["mean_squared_displacement"]))
    print(json.dumps(report))
    return report


def main(argv=None):
    args = parse_args(argv)
    return {"fit": fit, "apply": apply}[args.command](args)


if __name__ == "__main__":
    main()
