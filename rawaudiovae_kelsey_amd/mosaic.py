"""Latent audio mosaicing: resynthesise a target from the frames of a corpus that sound like it in the model's latent
space (corpus-based concatenative synthesis with the VAE's encoder as the descriptor).

  index = LatentIndex(model, hop=None)    frames each corpus file on its own (TestDataset at hop=None, AudioDataset at
  index.add(wave, name)                   an int hop: interpolate.frame_layout) and encodes the frames with the
                                          exact-fp32 encoder path; no frame straddles two files
  index.search(mu, k)                     (idx [T, k] int32, dist [T, k] fp32): the k nearest corpus frames of every
                                          row of mu, rv_mosaic(RV_MOSAIC_KNN)
  index.locate(idx)                       (file name, sample offset) of corpus frames
  index.mosaic(target, k, hop, mode, window)
      the target is framed at `hop` and encoded; each frame is replaced by its k nearest corpus frames, either
      "grains": the mean of their audio (S samples each, RV_MOSAIC_GATHER_MEAN over the corpus waveform), or
      "decode": the mean of their mu decoded through fc3 and fc4 + tanh (rv_linear_fp32);
      then an offline weighted overlap-add (RV_MOSAIC_OLA) with stream.py's window and normaliser rules.  The output
      has the target's length.
  index.mosaic(..., continuity=w)         w > 0: unit selection.  The k candidates are searched as above, then one per
                                          frame is chosen by a Viterbi search (best_path) that minimises
                                          sum_t dist[t, p_t] + w * sum_t trans[t, p_{t-1}, p_t], where trans is the
                                          distance between the corpus frame that FOLLOWS the previous choice
                                          (index.successor) and this candidate: 0 when the corpus simply plays on.
                                          Grains / decode then run on the one chosen frame.  w = 0 is the call above.
  transition_costs, best_path             the two steps on their own (RV_MOSAIC_TRANSITION, RV_MOSAIC_PATH_*)
  index.mosaic(..., fit=R, gain_max=g)    grain fitting ("grains" mode): every selected grain is moved by the shift in
                                          [-R, R] samples and scaled by the gain of its least-squares fit to the target
                                          frame before the overlap-add (the rule: include/rawvae_hip.h, "Grain
                                          fitting").  g = 0: shift only; g > 0: the gain, at most g.  A shifted grain
                                          stays inside its own file (index.room).  With k candidates each is fitted on
                                          its own and the k fitted grains are averaged; with continuity > 0 the one
                                          chosen frame is fitted.  fit=0, gain_max=0 is the call without them.
  shift_room, fit_grains, gather_fitted   the steps on their own (RV_GRAIN_FIT, RV_GRAIN_GATHER)
  check_mosaic_args                       the rules for k, mode, continuity, fit and gain_max that index.mosaic and
                                          check_live_args share, each in its own order
  knn_topk_small(q, c, k)                 knn_topk for at most SMALL_T_MAX query rows by the few-query kernel
                                          (RV_MOSAIC_KNN_SMALL): the same bits
  StreamingMosaic(index, n_streams, block, hop, k, mode, window, continuity, lag)
      live mosaicing: process(x) takes one block of samples per stream and returns the block built from the nearest
      corpus frames, `S - hop` samples late -- StreamingVAE's framing, history and overlap-add around the search
      (RV_MOSAIC_LIVE), state on the device, capture() / replay(x) as one graph.  continuity > 0 selects one candidate
      per frame, weighted by the device tensor `weight` [n_streams].  lag = 0: the GREEDY rule (each frame against the
      previous choice only; not best_path's Viterbi search, which needs the whole target; the two agree for k = 1).
      lag = D in [1, 64]: fixed-lag Viterbi.  The last D + 1 searched frames wait in a window; every new frame runs
      best_path's forward rule over the window, entered from the last committed choice, and commits the window's
      oldest frame, so each choice has seen D frames of its future and the audio comes `lag_samples` = D * hop samples
      later still (the first D frames of a stream are silent in grains mode).  drain() plays out what the window
      still holds, one block per call (drain_replay() after capture()).  The rule: include/rawvae_hip.h.
  StreamingMosaic(..., fit=R, gain_max=g)
      live grain fitting ("grains" mode): every corpus frame the block is about to play is first fitted, by the rule of
      index.mosaic(fit=, gain_max=), to the target frame it stands for -- the frame of the stream's own input that the
      encoder saw, which with a lag is `lag` frames old (older still for a frame that drain() plays out).  The input
      is kept per stream in a ring on the device; nothing syncs, capture() / replay() / drain() / reset() work as
      before, and last_fit() returns the block's (shift, gain, score).  At continuity 0 the output equals
      index.mosaic(..., fit=R, gain_max=g) of the same input bit for bit.  fit=0, gain_max=0 is the class without them.

The kNN distance is rv_som_bmu's direct fp32 form (identical frames are at distance exactly 0), ties go to the lower
corpus index and NaN never wins.  Every row's arithmetic is independent of `max_rows` (the chunk of target frames per
encoder, search, gather and decoder step), so the output is bit-identical for any chunking.  Framing, encoder and
decoder are codec.FrameCodec's (`index.codec`); the graphs of the live path are stream.GraphReplay's; every rv_mosaic
call passes the member names rv_mosaic_desc declares for the op's roles (_lib.mosaic_call).
"""
import functools

import numpy as np
import torch

from . import _lib
from ._lib import mosaic_call as _call, ptr
from .codec import FrameCodec, frame_layout
from .corpus import rows
from .stream import WINDOWS, GraphReplay, StreamingVAE, check_args, each_stream, window_values

MODES = ("grains", "decode")
K_MAX = 16
FIT_MAX = 1024     # samples a grain may be shifted at most (csrc/grain.hip)
SMALL_T_MAX = 64   # query rows of knn_topk_small (csrc/internal.h, csrc/mosaic_knn.hip)


def live_fit_table(successors, room):
    """RV_MOSAIC_LIVE with a fit reads ONE next_of table [3 N] int32: the successors [N] (None: zeros, unread without
    unit selection), then room [N, 2]"""
    if successors is None:
        successors = torch.zeros(room.shape[0], dtype=torch.int32, device=room.device)
    return torch.cat([successors, room.reshape(-1)]).contiguous()


_rows = functools.partial(rows, empty_ok=True)


def knn_workspace_bytes(T, N, L, k, splits=0, small=False):
    """Bytes of device workspace knn_topk (small: knn_topk_small) needs for these extents (0 when the corpus is not
    split)."""
    op = _lib.MOSAIC_KNN_SMALL_WORKSPACE if small else _lib.MOSAIC_KNN_WORKSPACE
    return _call(op, T=int(T), N=int(N), L=int(L), k=int(k), splits=int(splits)).ws_bytes


def knn_topk(q, c, k, splits=0):
    """(idx [T, k] int32, dist [T, k] fp32): the k nearest rows of c [N, L] to each row of q [T, L] under the squared
    distance, in ascending (distance, index) order; -1 / +inf where a row has fewer than k candidates.  `splits` pins
    the number of corpus splits (0: the library's choice); the result does not depend on it."""
    return _knn(q, c, k, splits, False)


def knn_topk_small(q, c, k, splits=0):
    """knn_topk by the kernel built for few query rows (at most SMALL_T_MAX; more raises RvError): the same result,
    bit for bit, for any `splits`."""
    return _knn(q, c, k, splits, True)


def _knn(q, c, k, splits, small):
    q, c = _rows(q, "q"), _rows(c, "c")
    if q.shape[1] != c.shape[1] or q.device != c.device:
        raise ValueError("q %s and c %s must share L and device" % (tuple(q.shape), tuple(c.shape)))
    T, N, L, k = q.shape[0], c.shape[0], q.shape[1], int(k)
    if not 1 <= k <= min(K_MAX, N):
        raise ValueError("k=%d must be in [1, %d] and at most the %d corpus rows" % (k, K_MAX, N))
    idx = torch.empty((T, k), dtype=torch.int32, device=q.device)
    dist = torch.empty((T, k), dtype=torch.float32, device=q.device)
    nbytes = knn_workspace_bytes(T, N, L, k, splits, small)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=q.device)
    _call(_lib.MOSAIC_KNN_SMALL if small else _lib.MOSAIC_KNN, T=T, N=N, L=L, k=k, splits=int(splits), q=ptr(q), c=ptr(c), idx=ptr(idx), dist=ptr(dist),
          ws=ptr(ws), ws_bytes=nbytes)
    return idx, dist


def path_workspace_bytes(T, k):
    """Bytes of device workspace best_path's forward and backtrack steps share for T rows of k candidates."""
    return _call(_lib.MOSAIC_PATH_WORKSPACE, T=int(T), k=int(k)).ws_bytes


def successor_table(file_of, adv=1):
    """next_of [N] int32 for corpus frames laid out file by file (frame_tables' file_of): i + adv when that frame exists
    and lies in the same file, else i (a file's last frames continue as themselves).  adv = target step / index step;
    ValueError naming `hop` unless it is a positive integer."""
    a = float(adv)
    if not (a >= 1 and a == int(a)):
        raise ValueError("hop: the target's frame step must be a positive integer multiple of the index's "
                         "(target step / index step = %r)" % (adv,))
    a = int(a)
    file_of = np.asarray(file_of)
    N = file_of.size
    i = np.arange(N, dtype=np.int64)
    nxt = i + a
    same = nxt < N
    same[same] = file_of[nxt[same]] == file_of[i[same]]
    return np.where(same, nxt, i).astype(np.int32)


def _candidates(idx, dist):
    if (not torch.is_tensor(idx) or idx.dim() != 2 or idx.dtype != torch.int32 or idx.device.type != "cuda"
            or idx.shape[0] < 1 or not 1 <= idx.shape[1] <= K_MAX):
        raise ValueError("idx must be a [T, k] int32 device tensor with T >= 1 and 1 <= k <= %d" % K_MAX)
    if dist is not None and (not torch.is_tensor(dist) or dist.dtype != torch.float32 or dist.shape != idx.shape
                             or dist.device != idx.device):
        raise ValueError("dist must be a float32 device tensor of idx's shape %s" % (tuple(idx.shape),))
    return idx.contiguous(), None if dist is None else dist.contiguous()


def _successors(next_of, N, device):
    if not torch.is_tensor(next_of):
        next_of = torch.from_numpy(np.ascontiguousarray(next_of, dtype=np.int32))
    next_of = next_of.to(device=device, dtype=torch.int32).contiguous()
    if next_of.dim() != 1 or next_of.numel() != N:
        raise ValueError("next_of must hold one successor for each of the %d corpus rows" % N)
    return next_of


def transition_costs(mu, idx, next_of, row0=0, rows=None, out=None):
    """trans [rows, k, k] fp32 for rows [row0, row0 + rows) of the candidates idx [T, k] (the whole table: row row0
    needs row row0 - 1): trans[t - row0, i, j] = the search's distance between mu[next_of[idx[t-1, i]]] and
    mu[idx[t, j]]; +inf where a candidate is -1 or the value is NaN; row 0 is all 0."""
    mu = _rows(mu, "mu")
    idx, _ = _candidates(idx, None)
    N, L = mu.shape
    next_of = _successors(next_of, N, mu.device)
    T, k = idx.shape
    row0 = int(row0)
    rows = T - row0 if rows is None else int(rows)
    if not (0 <= row0 and 1 <= rows <= T - row0):
        raise ValueError("rows [%d, %d + %d) outside the %d rows of idx" % (row0, row0, rows, T))
    if out is None:
        out = torch.empty((rows, k, k), dtype=torch.float32, device=mu.device)
    _call(_lib.MOSAIC_TRANSITION, T=T, k=k, idx=ptr(idx), c=ptr(mu), N=N, L=L, next_of=ptr(next_of), row0=row0,
          rows=rows, trans=ptr(out))
    return out


def best_path(idx, dist, mu, next_of, weight, max_rows=4096):
    """Viterbi unit selection over the candidates (idx, dist) [T, k] of knn_topk -> (slot [T] int32, choice [T] int32,
    cost [2] fp64), device tensors: the path p that minimises sum_t dist[t, p_t] + weight * sum_t trans[t, p_{t-1}, p_t]
    (transition_costs) under the forward rule of include/rawvae_hip.h; choice[t] = idx[t, slot[t]], both -1 for a row
    without candidates; cost = the two sums along the path.  The forward pass runs in chunks of max_rows rows, each
    over its own chunk of trans, carrying the scores on the device; the result does not depend on max_rows."""
    idx, dist = _candidates(idx, dist)
    mu = _rows(mu, "mu")
    weight, max_rows = float(weight), int(max_rows)
    if not 0 <= weight < float("inf"):
        raise ValueError("weight=%r must be a finite number >= 0" % (weight,))
    if max_rows < 1:
        raise ValueError("max_rows=%d must be at least 1" % max_rows)
    T, k = idx.shape
    next_of = _successors(next_of, mu.shape[0], mu.device)
    nbytes = path_workspace_bytes(T, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=idx.device)
    trans = torch.empty((min(max_rows, T), k, k), dtype=torch.float32, device=idx.device)
    for r0 in range(0, T, max_rows):
        rows = min(max_rows, T - r0)
        transition_costs(mu, idx, next_of, r0, rows, out=trans)
        _call(_lib.MOSAIC_PATH_FORWARD, T=T, k=k, idx=ptr(idx), dist=ptr(dist), row0=r0, rows=rows, trans=ptr(trans),
              lam=weight, ws=ptr(ws), ws_bytes=nbytes)
    slot = torch.empty(T, dtype=torch.int32, device=idx.device)
    choice = torch.empty(T, dtype=torch.int32, device=idx.device)
    cost = torch.empty(2, dtype=torch.float64, device=idx.device)
    _call(_lib.MOSAIC_PATH_BACKTRACK, T=T, k=k, idx=ptr(idx), dist=ptr(dist), ws=ptr(ws), ws_bytes=nbytes,
          slot=ptr(slot), choice=ptr(choice), cost=ptr(cost))
    return slot, choice, cost


def gather_mean(src, idx, width, row_start=None, stride=None, n_rows=None, out=None, ldo=None):
    """out [T, width] fp32: row t is (1/k) sum_j src[start(idx[t, j]) : + width], the sum in ascending j from +0.
    start(i) = row_start[i] (int64 device tensor) or i * stride.  Indices outside [0, n_rows) add nothing."""
    src = src.contiguous().view(-1)
    idx = idx.to(torch.int32).contiguous()
    T, k = idx.shape
    width = int(width)
    if row_start is None:
        stride = int(stride)
        n_rows = (src.numel() - width) // stride + 1 if n_rows is None else int(n_rows)
    else:
        row_start = row_start.to(torch.int64).contiguous()
        n_rows = row_start.numel() if n_rows is None else int(n_rows)
        stride = 0
    ldo = width if ldo is None else int(ldo)
    if out is None:
        out = torch.empty((T, ldo), dtype=torch.float32, device=src.device)
    _call(_lib.MOSAIC_GATHER_MEAN, T=T, k=k, idx=ptr(idx), src=ptr(src), src_len=src.numel(), row_start=ptr(row_start),
          stride=stride, n_rows=n_rows, width=width, out=ptr(out), ldo=ldo)
    return out


def check_fit(fit, gain_max):
    """(R, gain_max) of a grain fit: ValueError naming `fit` unless it is an integer in [0, FIT_MAX], naming `gain_max`
    unless it is a finite number >= 0."""
    if isinstance(fit, bool) or not isinstance(fit, (int, np.integer)) or not 0 <= int(fit) <= FIT_MAX:
        raise ValueError("fit=%r must be an integer number of samples in [0, %d]" % (fit, FIT_MAX))
    try:
        g = float(gain_max)
    except (TypeError, ValueError):
        g = float("nan")
    if not 0 <= g < float("inf"):
        raise ValueError("gain_max=%r must be a finite number >= 0" % (gain_max,))
    return int(fit), g


def check_mosaic_args(k, n_corpus, mode, continuity, fit, gain_max, rules=("fit_mode", "continuity", "mode", "k")):
    """The argument rules LatentIndex.mosaic and check_live_args share -> (k, continuity, fit, gain_max) as int, float,
    int, float.  ValueError naming the argument: check_fit's first, then those of `rules` in its order, which is what
    decides the error of a call that breaks several (the default is LatentIndex.mosaic's order)."""
    fit, gain_max = check_fit(fit, gain_max)
    for rule in rules:
        if rule == "fit_mode":
            if (fit > 0 or gain_max > 0) and mode == "decode":
                raise ValueError("fit=%d, gain_max=%g: grains are fitted in mode 'grains' only, mode 'decode' plays no "
                                 "corpus audio" % (fit, gain_max))
        elif rule == "continuity":
            continuity = float(continuity)
            if not 0 <= continuity < float("inf"):
                raise ValueError("continuity=%r must be a finite number >= 0" % (continuity,))
        elif rule == "mode":
            if mode not in MODES:
                raise ValueError("mode %r: expected one of %s" % (mode, ", ".join(MODES)))
        elif rule == "k":
            k = int(k)
            if not 1 <= k <= min(K_MAX, int(n_corpus)):
                raise ValueError("k=%d must be in [1, %d] and at most the %d corpus frames" % (k, K_MAX, int(n_corpus)))
    return k, continuity, fit, gain_max


def fit_buffers(rows, kf, device, alloc=torch.empty):
    """(shift int32, gain fp32, score fp64), each [rows, kf], of a grain fit: kf = k fits per row, or 1 where unit
    selection leaves one frame per row to fit."""
    return tuple(alloc((rows, kf), dtype=t, device=device) for t in (torch.int32, torch.float32, torch.float64))


def shift_room(lengths, segment_length, hop=None):
    """room [N, 2] int32 for the corpus layout of frame_tables: how many samples frame i's start may move back
    (room[i, 0]) and forward (room[i, 1]) while its segment_length samples stay inside its own file's padded
    waveform."""
    _, padded, _, file_of, offset_of = frame_tables(lengths, segment_length, hop)
    room = np.empty((file_of.size, 2), dtype=np.int32)
    room[:, 0] = offset_of
    room[:, 1] = padded[file_of] - int(segment_length) - offset_of
    return room


def fit_grains(target, idx, hop, segment_length, src, row_start, room, fit, gain_max=0.0):
    """(shift [T, k] int32, gain [T, k] fp32, score [T, k] fp64): the shift-and-gain fit (RV_GRAIN_FIT; the rule:
    include/rawvae_hip.h) of corpus grain idx[t, j] to target frame t = target[t * hop : t * hop + segment_length].
    target: 1-D fp32 device tensor holding all T frames; src: the corpus audio; row_start [N] int64 and room [N, 2]
    int32 device tensors (frame_tables, shift_room); fit = R samples; gain_max = 0: shift only (gain 1)."""
    R, g = check_fit(fit, gain_max)
    idx, _ = _candidates(idx, None)
    T, k = idx.shape
    S, hop = int(segment_length), int(hop)
    if (not torch.is_tensor(target) or target.dim() != 1 or target.dtype != torch.float32
            or target.device != idx.device or not target.is_contiguous()):
        raise ValueError("target must be a contiguous 1-D float32 tensor on idx's device")
    if hop < 1 or S < 1 or (T - 1) * hop + S > target.numel():
        raise ValueError("target: %d frames of %d samples at hop %d overrun its %d samples" % (T, S, hop, target.numel()))
    src = src.contiguous().view(-1)
    row_start = row_start.to(torch.int64).contiguous()
    N = row_start.numel()
    if (not torch.is_tensor(room) or room.dtype != torch.int32 or tuple(room.shape) != (N, 2)
            or room.device != idx.device):
        raise ValueError("room must be an int32 device tensor of shape [%d, 2] (shift_room)" % N)
    room = room.contiguous()
    shift, gain, score = fit_buffers(T, k, idx.device)
    _call(_lib.GRAIN_FIT, T=T, k=k, idx=ptr(idx), frames=ptr(target), n_out=target.numel(), hop=hop, S=S, src=ptr(src),
          src_len=src.numel(), row_start=ptr(row_start), n_rows=N, room=ptr(room), fit_radius=R, gain_max=g,
          shift=ptr(shift), gain=ptr(gain), score=ptr(score))
    return shift, gain, score


def gather_fitted(src, idx, shift, gain, width, row_start, out=None, ldo=None):
    """out [T, width] fp32: gather_mean with candidate j of row t read shift[t, j] samples later and scaled by
    gain[t, j] (RV_GRAIN_GATHER): (1/k) sum_j fl(gain * src[row_start[idx[t, j]] + shift[t, j] : + width]), ascending
    j from +0.  Shift 0 and gain 1 give gather_mean's bits."""
    src = src.contiguous().view(-1)
    idx, _ = _candidates(idx, None)
    T, k = idx.shape
    if (not torch.is_tensor(shift) or shift.dtype != torch.int32 or shift.shape != idx.shape
            or shift.device != idx.device):
        raise ValueError("shift must be an int32 device tensor of idx's shape %s" % (tuple(idx.shape),))
    if not torch.is_tensor(gain) or gain.dtype != torch.float32 or gain.shape != idx.shape or gain.device != idx.device:
        raise ValueError("gain must be a float32 device tensor of idx's shape %s" % (tuple(idx.shape),))
    shift, gain = shift.contiguous(), gain.contiguous()
    width = int(width)
    row_start = row_start.to(torch.int64).contiguous()
    ldo = width if ldo is None else int(ldo)
    if out is None:
        out = torch.empty((T, ldo), dtype=torch.float32, device=src.device)
    _call(_lib.GRAIN_GATHER, T=T, k=k, idx=ptr(idx), src=ptr(src), src_len=src.numel(), row_start=ptr(row_start),
          n_rows=row_start.numel(), width=width, out=ptr(out), ldo=ldo, shift=ptr(shift), gain=ptr(gain))
    return out


def ola(frames, hop, n_out, window=None, out=None):
    """[n_out] fp32 weighted overlap-add of frames [F, S] at `hop` (window: [S] fp32 device tensor or None)."""
    frames = frames.contiguous()
    F, S = frames.shape
    if out is None:
        out = torch.empty(int(n_out), dtype=torch.float32, device=frames.device)
    w = None if window is None else window.to(device=frames.device, dtype=torch.float32).contiguous()
    if w is not None and w.numel() != S:
        raise ValueError("window has %d values for frames of %d samples" % (w.numel(), S))
    _call(_lib.MOSAIC_OLA, frames=ptr(frames), F=F, S=S, hop=int(hop), window=ptr(w), n_out=int(n_out), out=ptr(out))
    return out


def check_window(segment_length, hop, window):
    """stream.py's window rules for a synthesis hop: ValueError for an unknown window or a Hann window whose sum is zero
    at frame starts (hop > segment_length / 2)."""
    if window not in WINDOWS:
        raise ValueError("window %r: expected None (rectangular) or 'hann'" % (window,))
    if window == "hann" and 2 * int(hop) > int(segment_length):
        raise ValueError("a Hann window needs hop <= segment_length / 2 (got hop %d, segment_length %d)"
                         % (hop, segment_length))


def frame_tables(lengths, segment_length, hop=None):
    """The corpus tables of files of `lengths` samples, each framed on its own (frame_layout) and stored padded, one
    after the other -> (n_frames [F], padded [F], row_start [N] int64, file_of [N] int32, offset_of [N] int64):
    frame i is samples [row_start[i], row_start[i] + segment_length) of the concatenation, which lie inside its file's
    padded waveform at offset_of[i]."""
    S = int(segment_length)
    step = S if hop is None else int(hop)
    lay = [frame_layout(n, S, hop) for n in lengths]
    n_frames = np.array([max(f, 0) for f, _ in lay], dtype=np.int64)
    padded = np.array([p for _, p in lay], dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64)
    file_of = np.repeat(np.arange(len(lay), dtype=np.int32), n_frames)
    offset_of = np.concatenate([np.arange(n, dtype=np.int64) * step for n in n_frames] or [np.zeros(0, np.int64)])
    return n_frames, padded, base[file_of] + offset_of, file_of, offset_of


class LatentIndex:
    """Frames of a corpus, their latents and their audio on the device (see the module doc).

    Corpus frame i of file f at frame position p starts at sample p * hop of f's padded waveform; the padded waveforms
    of all files are concatenated into one device buffer, and `row_start[i]` (int64) is frame i's sample offset in it.
    `file_of[i]` and `offset_of[i]` (numpy) give the file and the sample offset within the file."""

    def __init__(self, model, hop=None, max_rows=16384):
        self.codec = c = FrameCodec(model, max_rows=max_rows)
        self.model, self.max_rows, self.device = model, c.max_rows, c.device
        self.S, self.H, self.L = c.S, c.H, c.L
        self.hop = None if hop is None else int(hop)
        frame_layout(self.S, self.S, self.hop)   # ValueError for a hop that does not divide segment_length
        self.names = []
        self._lengths, self._waves, self._mus, self._n_frames = [], [], [], []
        self._built = None

    @property
    def step(self):
        return self.S if self.hop is None else self.hop

    def __len__(self):
        return int(sum(self._n_frames))

    @torch.no_grad()
    def add(self, wave, name):
        """Frame, encode and append one corpus file.  ValueError naming `name` when it makes no frame."""
        w = self.codec.wave(wave)
        n_frames, _ = frame_layout(w.numel(), self.S, self.hop)
        if n_frames < 1:
            raise ValueError("%s: %d samples make no frame of %d samples at hop %s" % (name, w.numel(), self.S,
                                                                                       self.hop))
        padded, n_frames = self.codec.pad(w, w.numel(), self.hop)
        mu, _ = self.codec.encode(padded, n_frames, self.hop)
        self.names.append(str(name))
        self._lengths.append(w.numel())
        self._waves.append(padded)
        self._mus.append(mu)
        self._n_frames.append(n_frames)
        self._built = None
        return n_frames

    def _tables(self):
        if self._built is None:
            if not self.names:
                raise ValueError("the index is empty: add() corpus files first")
            _, _, row_start, file_of, offset_of = frame_tables(self._lengths, self.S, self.hop)
            self._built = dict(audio=torch.cat(self._waves), mu=torch.cat(self._mus), file_of=file_of,
                               offset_of=offset_of, row_start_host=row_start,
                               row_start=torch.from_numpy(row_start).to(self.device))
        return self._built

    @property
    def audio(self):
        """All files' padded waveforms, concatenated: [sum of padded lengths] fp32 on the device."""
        return self._tables()["audio"]

    @property
    def mu(self):
        """[N, L] fp32 encoder mu of every corpus frame, file by file."""
        return self._tables()["mu"]

    @property
    def row_start(self):
        return self._tables()["row_start_host"]

    @property
    def file_of(self):
        return self._tables()["file_of"]

    @property
    def offset_of(self):
        return self._tables()["offset_of"]

    @property
    def room(self):
        """[N, 2] int32 (numpy): how far each corpus frame may be shifted back / forward inside its file (shift_room)."""
        return self._room()[0]

    def _room(self):
        t = self._tables()
        if "room" not in t:
            host = shift_room(self._lengths, self.S, self.hop)
            t["room"] = (host, torch.from_numpy(host).to(self.device))
        return t["room"]

    def successor(self, adv=1):
        """next_of [N] int32 (numpy, cached): the corpus frame `adv` index steps after frame i in the same file, or i
        itself at a file's end (successor_table)."""
        return self._successor(adv)[0]

    def _successor(self, adv):
        cache = self._tables().setdefault("next_of", {})
        if adv not in cache:
            host = successor_table(self.file_of, adv)
            cache[adv] = (host, torch.from_numpy(host).to(self.device))
        return cache[adv]

    @torch.no_grad()
    def search(self, mu, k, splits=0):
        """(idx [T, k] int32, dist [T, k] fp32) of the k nearest corpus frames of each row of mu [T, L]."""
        return knn_topk(mu, self.mu, k, splits)

    def locate(self, idx):
        """(name, sample offset within the file) of each corpus frame index in idx (any shape; -1 -> (None, -1)),
        as a nested list of idx's shape."""
        a = idx.cpu().numpy() if torch.is_tensor(idx) else np.asarray(idx)
        t = self._tables()
        N = len(self)

        def one(i):
            i = int(i)
            if not 0 <= i < N:
                return (None, -1)
            return (self.names[t["file_of"][i]], int(t["offset_of"][i]))
        if a.ndim == 0:
            return one(a)
        return [self.locate(r) if a.ndim > 1 else one(r) for r in a]

    @torch.no_grad()
    def mosaic(self, target, k=1, hop=None, mode="grains", window=None, return_matches=False, continuity=0.0,
               return_path=False, fit=0, gain_max=0.0, return_fit=False):
        """The target resynthesised from the corpus (see the module doc) -> 1-D fp32 device tensor of the target's
        length; with return_matches also (idx [T, k], dist [T, k]).  hop=None: the index's framing.
        continuity > 0 chooses one of the k candidates per frame by best_path with that weight; return_path then
        appends (slot, choice, cost) to the result (None at continuity 0, where no path is searched).
        fit = R > 0 or gain_max > 0 ("grains" mode only): every grain is fitted to its target frame by a shift of at
        most R samples and, with gain_max > 0, a gain of at most gain_max (fit_grains) before the overlap-add;
        return_fit then appends (shift, gain, score), each [T, k], or [T, 1] with continuity > 0 (None when nothing
        is fitted)."""
        k, continuity, fit, gain_max = check_mosaic_args(k, len(self), mode, continuity, fit, gain_max)
        hop = self.hop if hop is None else int(hop)
        step = self.S if hop is None else hop
        check_window(self.S, step, window)
        if continuity > 0:
            next_of = self._successor(step / self.step)[1]   # ValueError naming hop unless a whole number of steps
        w = self.codec.wave(target)
        padded, T = self.codec.pad(w, w.numel(), hop)
        mu, _ = self.codec.encode(padded, T, hop)
        synth = _Synthesis(self, padded, T, step, mode, fit, gain_max, k if continuity == 0 else 1)
        idx = torch.empty((T, k), dtype=torch.int32, device=self.device)
        dist = torch.empty((T, k), dtype=torch.float32, device=self.device)
        for r0, rows in self.codec.chunks(T):          # search; without unit selection each chunk is synthesised at once
            i, d = knn_topk(mu[r0:r0 + rows], self.mu, k)
            idx[r0:r0 + rows], dist[r0:r0 + rows] = i, d
            if continuity == 0:
                synth.chunk(i, r0, rows)
        path = None
        if continuity > 0:                             # select, then synthesise from the one chosen frame of each row
            path = best_path(idx, dist, self.mu, next_of, continuity, max_rows=self.max_rows)
            one = path[1].view(T, 1)   # the chosen corpus frame: a gather-mean of one is that frame, bit for bit
            for r0, rows in self.codec.chunks(T):
                synth.chunk(one[r0:r0 + rows], r0, rows)
        win = None if window is None else torch.from_numpy(window_values(self.S, window)).to(self.device)
        out = ola(synth.frames, step, w.numel(), win)
        res = (out, idx, dist) if return_matches else (out,)
        if return_path:
            res += (path,)
        if return_fit:
            res += (synth.fits,)
        return res if len(res) > 1 else out


class _Synthesis:
    """The frames [T, S] of one LatentIndex.mosaic call, `chunk(i, r0, rows)` at a time: rows [r0, r0 + rows) from the
    corpus frames i [rows, any k] chosen for them -- their mean audio, each fitted to its target frame first when a fit
    is asked for (`fits`: the (shift, gain, score) of every row, else None), or their mean mu decoded."""

    def __init__(self, index, padded, T, step, mode, fit, gain_max, kf):
        self.index, self.padded, self.step, self.fit, self.gain_max = index, padded, step, fit, gain_max
        self.tables = index._tables()
        self.frames = torch.empty((T, index.S), dtype=torch.float32, device=index.device)
        self.fits, self.chunk = None, self._mean_grains
        if fit > 0 or gain_max > 0:
            self.room, self.fits, self.chunk = index._room()[1], fit_buffers(T, kf, index.device), self._fitted_grains
        elif mode == "decode":
            self.z = torch.empty((min(index.max_rows, T), index.L), dtype=torch.float32, device=index.device)
            self.h, self.chunk = index.codec.hidden(T), self._decoded_mean

    def _fitted_grains(self, i, r0, rows):
        t, S, i = self.tables, self.index.S, i.contiguous()
        sh, gn, sc = fit_grains(self.padded[r0 * self.step:], i, self.step, S, t["audio"], t["row_start"], self.room,
                                self.fit, self.gain_max)
        for dst, part in zip(self.fits, (sh, gn, sc)):
            dst[r0:r0 + rows] = part
        gather_fitted(t["audio"], i, sh, gn, S, t["row_start"], out=self.frames[r0:r0 + rows])

    def _mean_grains(self, i, r0, rows):
        t = self.tables
        gather_mean(t["audio"], i, self.index.S, row_start=t["row_start"], out=self.frames[r0:r0 + rows])

    def _decoded_mean(self, i, r0, rows):
        L = self.index.L
        gather_mean(self.tables["mu"], i, L, stride=L, n_rows=len(self.index), out=self.z[:rows])
        self.index.codec.decode_chunk(self.z[:rows], self.h, self.frames[r0:r0 + rows])


LAG_MAX = 64       # frames of look-ahead of the live selection at most (csrc/mosaic_live.hip)


def check_live_args(segment_length, index_step, n_corpus, n_streams, block, hop=None, k=1, mode="grains", window=None,
                    continuity=0.0, lag=0, fit=0, gain_max=0.0):
    """Validate a StreamingMosaic configuration without a device -> (hop, latency, frames per block, successor
    advance).  ValueError naming the argument (`fit` / `gain_max`: check_fit's ranges, and mode "grains" only)."""
    S = int(segment_length)
    fit, gain_max = check_fit(fit, gain_max)
    if int(n_corpus) < 1:
        raise ValueError("index: the index is empty, add() corpus files first")
    if int(n_streams) <= 0:
        raise ValueError("n_streams must be positive, got %d" % int(n_streams))
    _, continuity, _, _ = check_mosaic_args(k, n_corpus, mode, continuity, fit, gain_max, ("mode", "k", "continuity"))
    if isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not 0 <= int(lag) <= LAG_MAX:
        raise ValueError("lag=%r must be an integer in [0, %d]" % (lag, LAG_MAX))
    if int(lag) > 0 and continuity == 0:
        raise ValueError("lag=%d needs continuity > 0: without unit selection there is nothing to look ahead for"
                         % int(lag))
    check_mosaic_args(k, n_corpus, mode, continuity, fit, gain_max, ("fit_mode",))
    hop, latency, frames = check_args(S, block, hop, window)   # ValueError naming hop, block or window
    adv = 1
    if continuity > 0:
        if hop % int(index_step) != 0:
            raise ValueError("hop %d must be a whole multiple of the index's frame step %d when continuity > 0"
                             % (hop, int(index_step)))
        adv = hop // int(index_step)
    return hop, latency, frames, adv


class StreamingMosaic(GraphReplay):
    """Live mosaicing of `n_streams` streams against a LatentIndex (see the module doc).

    `process(x)` -> y [n_streams, block], the input `latency` = S - hop samples late; the concatenated outputs equal
    `index.mosaic(cat([zeros(latency), x]), k, hop, mode, window)` bit for bit at continuity 0.  Device tensors that
    may be written in place between calls: `scale`, `offset` [n_streams, L] (the query is mu * scale + offset) and,
    with continuity > 0, `weight` [n_streams] (starts at `continuity`; a value that is not finite and >= 0 counts
    as 0).  The index must not change after construction.

    `lag` > 0 (needs continuity > 0): fixed-lag Viterbi selection.  The choices, and with them the audio, come
    `lag_samples` = lag * hop samples later on top of `latency`; `drain()` plays out the frames still held back.

    `fit` = R > 0 or `gain_max` > 0 (mode "grains"): every frame played is fitted to the target frame it stands for
    (see the module doc); with them the equality above holds against `index.mosaic(..., fit=R, gain_max=gain_max)`,
    and `last_fit()` returns the block's shifts, gains and scores."""

    def __init__(self, index, n_streams, block, hop=None, k=1, mode="grains", window=None, continuity=0.0, lag=0,
                 fit=0, gain_max=0.0):
        self.index = index
        N = len(index)
        self.hop, self.latency, self.frames_per_block, adv = check_live_args(
            index.S, index.step, N, n_streams, block, hop, k, mode, window, continuity, lag, fit, gain_max)
        self.fit, self.gain_max = check_fit(fit, gain_max)
        self.fitted = self.fit > 0 or self.gain_max > 0
        self.lag = int(lag)
        self.lag_samples = self.lag * self.hop
        # the framing, history, window tables and stream workspace are StreamingVAE's
        self._sv = StreamingVAE(index.model, n_streams, block, self.hop, window)
        self.n_streams, self.block, self.k, self.mode, self.window = int(n_streams), int(block), int(k), mode, window
        self.S, self.L, self.device = index.S, index.L, self._sv.device
        self.scale, self.offset = self._sv.scale, self._sv.offset
        self.selects = float(continuity) > 0
        t = index._tables()
        self._mu, self._audio, self._row_start = t["mu"], t["audio"], t["row_start"]
        self._next_of = index._successor(adv)[1] if self.selects else None
        self.weight = (torch.full((self.n_streams,), float(continuity), dtype=torch.float32, device=self.device)
                       if self.selects else None)
        M = self.n_streams * self.frames_per_block
        self._idx = torch.full((M, self.k), -1, dtype=torch.int32, device=self.device)
        self._dist = torch.full((M, self.k), float("inf"), dtype=torch.float32, device=self.device)
        self._choice = torch.full((M,), -1, dtype=torch.int32, device=self.device)
        self._fit = None
        if self.fitted:
            self._next_of = live_fit_table(self._next_of, index._room()[1])
            self._fit = fit_buffers(M, 1 if self.selects else self.k, self.device, torch.zeros)
        self._ws = None
        nbytes = self._call(_lib.MOSAIC_LIVE_WORKSPACE, None, None).ws_bytes
        self._ws = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self._zeros = None
        self.reset()

    def _call(self, op, x, y, which=-1, stream=None):
        sd = self._sv.desc(x, y, None)
        shift, gain, score = self._fit or (None, None, None)
        return _call(op, stream, k=self.k, idx=ptr(self._idx), dist=ptr(self._dist), c=ptr(self._mu), N=self._mu.shape[0],
                     L=self.L, src=ptr(self._audio), src_len=self._audio.numel(), row_start=ptr(self._row_start),
                     choice=ptr(self._choice), ws=ptr(self._ws), ws_bytes=0 if self._ws is None else self._ws.numel(),
                     live=_lib.C.pointer(sd), mode=_lib.LIVE_DECODE if self.mode == "decode" else _lib.LIVE_GRAINS,
                     weight=ptr(self.weight), which=int(which), lag=self.lag, next_of=ptr(self._next_of),
                     fit_radius=self.fit, gain_max=self.gain_max, shift=ptr(shift), gain=ptr(gain), score=ptr(score))

    @torch.no_grad()
    def process(self, x):
        """One block: x [n_streams, block] fp32 on the device -> [n_streams, block]."""
        x = self.check_input(x)
        y = torch.empty((self.n_streams, self.block), dtype=torch.float32, device=self.device)
        self._call(_lib.MOSAIC_LIVE, x, y)
        return y

    def _zero_block(self):
        if self.lag == 0:
            raise ValueError("lag=0: nothing is held back, there is nothing to drain")
        if self._zeros is None:
            self._zeros = torch.zeros((self.n_streams, self.block), dtype=torch.float32, device=self.device)
        return self._zeros

    @torch.no_grad()
    def drain(self):
        """One block [n_streams, block] that plays out frames the lag still holds back (RV_MOSAIC_LIVE_DRAIN): no input,
        no search; the history, the frame counter and the overlap-add move on as for a block of silence.  After
        `drain_blocks` calls everything fed so far has been played; process() may follow.  ValueError at lag 0."""
        x = self._zero_block()
        y = torch.empty((self.n_streams, self.block), dtype=torch.float32, device=self.device)
        self._call(_lib.MOSAIC_LIVE_DRAIN, x, y)
        return y

    @property
    def drain_blocks(self):
        """drain() calls after the last process() until every frame fed has left the overlap-add."""
        frames = self.lag + (self.S - self.hop) // self.hop
        return -(-frames // self.frames_per_block)

    @torch.no_grad()
    def reset(self, streams=None):
        """Zero the history, the overlap-add tail and the frame counter of `streams` (an index or a list; None = all)
        and forget their last chosen corpus frame and the frames their lag holds back; with a fit their target
        history is silence again."""
        for s in each_stream(streams, self.n_streams):
            self._call(_lib.MOSAIC_LIVE_RESET, None, None, s)

    def last_matches(self):
        """(idx [n_streams, F, k] int32, dist [n_streams, F, k] fp32, choice [n_streams, F] int32) of the last block's
        frames, as views of static buffers; choice is the selected corpus frame, -1 everywhere at continuity 0.
        With a lag, choice is `lag` frames behind idx / dist: choice[s, f] is the frame committed when the block's
        frame f arrived, chosen among the candidates of the frame `lag` frames earlier (-1 for the first `lag` frames
        after a reset); after drain() idx / dist still hold the last process() call's frames."""
        F = self.frames_per_block
        return (self._idx.view(self.n_streams, F, self.k), self._dist.view(self.n_streams, F, self.k),
                self._choice.view(self.n_streams, F))

    def last_fit(self):
        """(shift [n_streams, F, kf] int32, gain [n_streams, F, kf] fp32, score [n_streams, F, kf] fp64) of the last
        block's frames as views of static buffers, or None when nothing is fitted; kf = k at continuity 0 (one fit per
        candidate), 1 with unit selection (the chosen or committed frame's fit; (0, 0, 0) where choice is -1)."""
        if self._fit is None:
            return None
        F = self.frames_per_block
        return tuple(t.view(self.n_streams, F, -1) for t in self._fit)

    def last_latents(self):
        """(mu, logvar) of the last block's frames as views [n_streams, F, L], before `scale` and `offset`."""
        return self._sv.last_latents()

    @torch.no_grad()
    def capture(self):
        """Capture one call as a graph on static buffers `graph_input` / `graph_output` [n_streams, block];
        `replay(x)` then runs one block per call.  With a lag a second graph holds one drain() call for
        `drain_replay()`, writing `graph_output` too.  The graphs hold the Parameters' pointers: replaying after a
        Parameter was replaced raises."""
        launches = [lambda st: self._call(_lib.MOSAIC_LIVE, self.graph_input, self.graph_output, stream=st)]
        if self.lag > 0:
            zeros = self._zero_block()
            launches.append(lambda st: self._call(_lib.MOSAIC_LIVE_DRAIN, zeros, self.graph_output, stream=st))
        return self._capture(*launches)

    def parameters(self):
        return self._sv.parameters()

    def check_input(self, x):
        return self._sv.check_input(x)

    @torch.no_grad()
    def replay(self, x=None):
        """One block through the captured graph on the current stream; x (optional) is copied into `graph_input`
        first.  Returns `graph_output` (overwritten by the next replay)."""
        return self._replay(0, "replay()", x)

    @torch.no_grad()
    def drain_replay(self):
        """drain() through its captured graph on the current stream.  Returns `graph_output`."""
        self._zero_block()   # ValueError at lag 0
        return self._replay(1, "drain_replay()")
