"""What the command-line front ends at the repository's root share: flag parsing, the model's setup, the user's wavs and
the checks of a fitted file against the model.  Every error is a ValueError that names the flag or the file.

  number_flag(args, flag, kind, ok, what)    one numeric flag, checked and set on args; positive_int, nonneg_int,
                                             int_at_least, positive_real, nonneg_real: its recurring phrases
  window_flag(args), add_model_flags(parser), parse_axis_values / check_axes, flagged(flags, fn)
  read_model_config(path), frame_step(args, S), model_config(args), load_model(path, cfg), open_model(args)
  load_wav(path, sr), data_files(path), check_exists(flag, path), encode_wav(codec, wave, hop, flag, path)
  check_fitted(flag, path, meta, cfg, hop)   a fitted .npz against the model's shape and the hop

torch, the model and the audio reader are imported inside the functions that need them: --help and a bad flag need no GPU.
"""
import configparser
import math
import os


def number_flag(args, flag, kind, ok, what, none_ok=True):
    """args' value of --flag (spelled with dashes) as kind(value), which ok() must accept: set on args and returned.
    None stays None when none_ok.  ValueError "--flag 'value': expected <what>"."""
    name = flag.replace("-", "_")
    v = getattr(args, name)
    if v is None and none_ok:
        return None
    try:
        x = kind(v)
    except (TypeError, ValueError):
        x = None
    if x is None or not ok(x):
        raise ValueError("--%s %r: expected %s" % (flag, v, what))
    setattr(args, name, x)
    return x


def positive(x):
    return 0 < x < float("inf")


def nonneg(x):
    return 0 <= x < float("inf")


def finite(lo, hi):
    """The test of a finite number in [lo, hi]."""
    return lambda x: math.isfinite(x) and lo <= x <= hi


def positive_int(args, flag):
    return number_flag(args, flag, int, lambda x: x > 0, "a positive integer")


def nonneg_int(args, flag):
    return number_flag(args, flag, int, lambda x: x >= 0, "a non-negative integer")


def int_at_least(args, flag, minimum):
    return number_flag(args, flag, int, lambda x: x >= minimum, "an integer >= %d" % minimum)


def positive_real(args, flag):
    return number_flag(args, flag, float, positive, "a finite number > 0")


def nonneg_real(args, flag):
    return number_flag(args, flag, float, nonneg, "a finite number >= 0")


def window_flag(args):
    """--window none|hann -> args.window None | "hann"."""
    if args.window not in ("none", "hann"):
        raise ValueError("--window %r: expected none or hann" % args.window)
    args.window = None if args.window == "none" else args.window
    return args.window


def add_model_flags(parser, hop_help="frame hop (default: non-overlapping frames)"):
    parser.add_argument("--config", default="./default.ini", help="the training .ini (model shape, sampling_rate)")
    parser.add_argument("--checkpoint", required=True, help="checkpoint dict (ckpt_NNNNN) or whole-module pickle (.pt)")
    parser.add_argument("--hop", default=None, help=hop_help)


def parse_axis_values(text, flag):
    """{0-based axis: value} of "J:V,J:V,..." with 1-based J; ValueError naming `flag` for anything else, a J < 1, a
    value that is not finite or an axis given twice."""
    out = {}
    for item in str(text).split(","):
        j, sep, v = item.partition(":")
        try:
            if not sep:
                raise ValueError
            axis, value = int(j), float(v)
        except ValueError:
            raise ValueError("--%s %r: expected J:VALUE,... with J a 1-based axis number, got %r" % (flag, text, item))
        if axis < 1:
            raise ValueError("--%s %r: axis %d: axes are numbered from 1" % (flag, text, axis))
        if value != value or abs(value) == float("inf"):
            raise ValueError("--%s %r: axis %d: the value must be finite" % (flag, text, axis))
        if axis - 1 in out:
            raise ValueError("--%s %r: axis %d is given twice" % (flag, text, axis))
        out[axis - 1] = value
    return out


def check_axes(values, n_axes, flag):
    """`values` of parse_axis_values against the number of axes of the .npz; ValueError naming `flag`."""
    for j in values:
        if j >= n_axes:
            raise ValueError("--%s: axis %d: the PCA file holds %d axes" % (flag, j + 1, n_axes))
    return values


def flagged(flags, fn):
    """fn(), its ValueError re-raised behind the flags it belongs to."""
    try:
        return fn()
    except ValueError as e:
        raise ValueError("%s: %s" % (flags, e))


def read_model_config(path):
    config = configparser.ConfigParser(allow_no_value=True)
    if not config.read(path):
        raise ValueError("--config %r: file not found" % path)
    return dict(sampling_rate=config["audio"].getint("sampling_rate"),
                segment_length=config["audio"].getint("segment_length"),
                n_units=config["VAE"].getint("n_units"), latent_dim=config["VAE"].getint("latent_dim"))


def frame_step(args, segment_length):
    """--hop against the model's frame length -> the frame step in samples; ValueError naming --hop."""
    from .codec import frame_layout
    S = int(segment_length)
    try:
        frame_layout(S, S, args.hop)
    except ValueError as e:
        raise ValueError("--hop %s: %s" % (args.hop, e))
    return S if args.hop is None else args.hop


def model_config(args):
    """(cfg of --config, frame_step of --hop): what a front end knows before it loads the checkpoint."""
    cfg = read_model_config(args.config)
    return cfg, frame_step(args, cfg["segment_length"])


def load_model(path, cfg, device="cuda"):
    """VAE of the .ini's shape with the checkpoint's parameters."""
    import torch
    from rawvae.model import VAE
    state = torch.load(path, map_location=device, weights_only=False)
    model = VAE(cfg["segment_length"], cfg["n_units"], cfg["latent_dim"]).to(device)
    if isinstance(state, dict):
        sd = state.get("state_dict", state)
    elif isinstance(state, torch.nn.Module):
        sd = state.state_dict()
    else:
        raise ValueError("--checkpoint %r: neither a checkpoint dict nor a module pickle" % path)
    model.load_state_dict(sd)
    return model.eval()


def open_model(args):
    """(cfg, model, step): model_config, then the checkpoint."""
    cfg, step = model_config(args)
    return cfg, load_model(args.checkpoint, cfg), step


def load_wav(path, sr):
    """data.load_audio_mono with errors that name the file: unreadable or zero-length wavs raise ValueError."""
    from . import data as D
    try:
        a = D.load_audio_mono(path, sr)
    except Exception as e:   # scipy raises ValueError / OSError / struct.error on malformed files
        raise ValueError("%s: unreadable wav (%s)" % (path, e))
    if a.size == 0:
        raise ValueError("%s: zero-length wav" % path)
    return a


def data_files(path):
    """The wavs --data names: the file itself, or the folder's *.wav sorted by name."""
    if os.path.isdir(path):
        files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.lower().endswith(".wav"))
        if not files:
            raise ValueError("--data %r: no .wav files in the folder" % path)
        return files
    if not os.path.exists(path):
        raise ValueError("--data %r: no such file or folder" % path)
    return [path]


def check_exists(flag, path):
    """The file --flag names exists; checked before the model loads, so before a fitted file's meta can be read."""
    if not os.path.exists(path):
        raise ValueError("--%s %r: no such file" % (flag, path))


def check_fitted(flag, path, meta, cfg, hop=Ellipsis, fitted="the walk was", unit="one step of the walk is one frame at that hop"):
    """The meta of the fitted file --flag against the model's shape and, when `hop` is given, --hop against the hop of
    the fit (corpus.check_hop with its two phrases) -> the frame step in samples."""
    from .corpus import check_hop
    if meta["segment_length"] != cfg["segment_length"] or meta["latent_dim"] != cfg["latent_dim"]:
        raise ValueError("--%s %r: fitted for segment_length %d and latent_dim %d, the model has %d and %d" % (
            flag, path, meta["segment_length"], meta["latent_dim"], cfg["segment_length"], cfg["latent_dim"]))
    if hop is Ellipsis:
        return None
    try:
        return check_hop(meta["hop"], hop, meta["segment_length"], fitted, unit)
    except ValueError as e:
        raise ValueError("--hop: %s (--%s %r)" % (e, flag, path))


def encode_wav(codec, wave, hop, flag, path):
    """(w, mu, logvar, frames) of one wav through a FrameCodec; a wav too short to frame raises naming --flag."""
    w = codec.wave(wave)
    try:
        padded, T = codec.pad(w, w.numel(), hop)
    except ValueError as e:
        raise ValueError("--%s %r: %s" % (flag, path, e))
    mu, logvar = codec.encode(padded, T, hop)
    return w, mu, logvar, T
