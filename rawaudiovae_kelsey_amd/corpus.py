"""What the corpus models (pca, walk, states) and the row-wise ops share on the host: the argument checks of their rows
and file boundaries, the encoding of a corpus, the hop check and the .npz codec of a fitted model.

  rows(x, what, dtype, cols, empty_ok, wording)      x as a contiguous 2-D device tensor (ValueError)
  check_row_start(row_start, T, empty_files)         the files' first rows as a fresh [n + 1] int64 numpy array
  encode_corpus(model, waves, hop, max_rows)         (mu [T, L], row_start [n + 1]) through codec.FrameCodec
  check_hop(fitted_hop, hop, segment_length, ...)    the hop a fitted model is used at against the hop of its fit
  write_fitted(path, arrays, meta, **extra) / read_fitted(path, kind, arrays, meta, extra)
                                                     one .npz of fp64 arrays, integers and whatever else a model keeps
"""
import numpy as np
import torch

from .codec import FrameCodec

_DTYPES = {torch.float32: "float32", torch.float64: "float64"}


def rows(x, what="x", dtype=torch.float32, cols=None, empty_ok=False, wording="a 2-D"):
    """x as a contiguous 2-D `dtype` device tensor (of `cols` columns, with at least one row and one column unless
    empty_ok); ValueError naming `what`.  wording: how the message describes the shape."""
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype != dtype or x.device.type != "cuda":
        raise ValueError("%s must be %s %s device tensor, got %s" % (
            what, wording, _DTYPES[dtype],
            "%s %s on %s" % (x.dtype, tuple(x.shape), x.device) if torch.is_tensor(x) else type(x).__name__))
    if not empty_ok and (x.shape[0] < 1 or x.shape[1] < 1):
        raise ValueError("%s is empty: shape %s" % (what, tuple(x.shape)))
    if cols is not None and x.shape[1] != cols:
        raise ValueError("%s has %d columns, expected %d" % (what, x.shape[1], cols))
    return x.contiguous()


def check_row_start(row_start, T, empty_files=False):
    """row_start as a fresh [n_files + 1] int64 numpy array, checked on the host: from 0 to T and ascending, or with
    empty_files never descending (ValueError)."""
    if torch.is_tensor(row_start):
        row_start = row_start.cpu().numpy()
    rs = np.asarray(row_start)
    if rs.ndim != 1 or rs.size < 2 or rs.dtype.kind not in "iu":
        raise ValueError("row_start must be a 1-D integer sequence of n_files + 1 entries, got %s %s" % (rs.dtype, rs.shape))
    rs = np.array(rs, dtype=np.int64)     # a copy: the caller's array may be read-only
    if rs[0] != 0 or rs[-1] != int(T):
        raise ValueError("row_start must run from 0 to T=%d, got %d .. %d" % (int(T), rs[0], rs[-1]))
    bad = np.diff(rs) < 0 if empty_files else np.diff(rs) <= 0
    if np.any(bad):
        f = int(np.argmax(bad))
        raise ValueError("row_start %s: file %d is [%d, %d)" % (
            "must not descend" if empty_files else "must be ascending", f, rs[f], rs[f + 1]))
    return rs


def encode_corpus(model, waves, hop=None, max_rows=16384):
    """(mu [T, L] of every frame of every waveform, row_start [n + 1] int64) through codec.FrameCodec, framed like
    TestDataset (hop=None) or AudioDataset (hop=int)."""
    codec = FrameCodec(model, max_rows=max_rows)
    waves = list(waves)
    if not waves:
        raise ValueError("fit_corpus needs at least one waveform")
    mus, starts = [], [0]
    for f, w in enumerate(waves):
        try:
            w = codec.wave(w)
            padded, n_frames = codec.pad(w, w.numel(), hop)
            mus.append(codec.encode(padded, n_frames, hop)[0])
        except ValueError as e:
            raise ValueError("waveform %d: %s" % (f, e))
        starts.append(starts[-1] + n_frames)
    return (torch.cat(mus, 0) if len(mus) > 1 else mus[0]), np.asarray(starts, dtype=np.int64)


def check_hop(fitted_hop, hop, segment_length, fitted="the walk was", unit="one step of the walk is one frame at that hop"):
    """The hop a fitted model is used at against the hop it was fitted at (None: non-overlapping frames of
    segment_length) -> the hop in samples; ValueError naming both when they differ."""
    a = int(segment_length) if fitted_hop is None else int(fitted_hop)
    b = int(segment_length) if hop is None else int(hop)
    if a != b:
        raise ValueError("hop %d: %s fitted at hop %d; %s" % (b, fitted, a, unit))
    return b


def write_fitted(path, arrays, meta, **extra):
    """One .npz: the tensors of `arrays` as they are, the integers of `meta` (hop None: -1) and `extra` as given."""
    meta = dict(meta, hop=-1 if meta["hop"] is None else meta["hop"])
    with open(path, "wb") as f:
        np.savez(f, **{n: t.cpu().numpy() for n, t in arrays.items()}, **{n: int(v) for n, v in meta.items()}, **extra)


def read_fitted(path, kind, arrays, meta, extra=()):
    """({name: contiguous fp64 array}, {name: int} with hop -1 -> None, {name: array}) of write_fitted's file; ValueError
    naming the keys a latent-`kind` file lacks."""
    with np.load(path) as z:
        missing = [n for n in tuple(arrays) + tuple(meta) + tuple(extra) if n not in z.files]
        if missing:
            raise ValueError("%s: not a latent-%s file, it lacks %s" % (path, kind, ", ".join(missing)))
        a = {n: np.ascontiguousarray(z[n], dtype=np.float64) for n in arrays}
        m = {n: int(z[n]) for n in meta}
        x = {n: z[n] for n in extra}
    m["hop"] = None if m["hop"] < 0 else m["hop"]
    return a, m, x
