"""Latent restoration: inference with the fitted walk (walk.LatentWalk) -- a Kalman filter and a fixed-interval smoother
over latent trajectories whose frames are partly missing, and gap filling of waveforms with them (the RV_SMOOTH_* ops of
rv_mosaic; the rules: include/rawvae_hip.h, "Latent restoration").

The walk is w' = A w + B e in whitened principal coordinates, A A^T + B B^T = I.  A frame's latent row x_t is observed as
y_t = P (x_t - c) with noise r_t I, r_t = noise / weight[t]; a frame with weight <= 0 (or NaN) is missing.

Host integer logic (no device):
  frame_mask(n_samples, segment_length, hop, ranges)   bool [frames]: the frame's samples overlap a damaged range
  regions(mask, context)                               [(f0, f1)]: every run of missing frames with `context` frames on
                                                       each side, merged where they touch, clipped to the file
  parse_ranges("1.20:1.35,...", sampling_rate)          [(s, e)] in samples
  check_ranges(ranges, n_samples)                       sorted, merged where they touch, clipped -> int64 [n, 2]
  zero_runs(wave, min_run)                              [(s, e)]: runs of exactly-zero samples of at least min_run
On the device:
  LatentSmoother(walk, noise=1e-2, max_workspace_bytes=2 GiB)
    .filter(x, row_start, weight=None)  -> w+ [T, k], nis [T], logdet [T]   (fp64; nis -1 and logdet 0 at missing frames)
    .smooth(x, row_start, weight=None)  -> z [T, L] fp32, w_hat [T, k] fp64
  splice(src, resynthesis, ranges, fade)               RV_SMOOTH_SPLICE
  restore(model, walk, wave, ranges, hop, window, noise, context=32, fade=64) -> the repaired waveform [n] fp32
  surprise(model, walk, wave, hop, noise)              nis / k per frame, from the filter alone

Nothing syncs; every op may run under graph capture (the tensors are then the caller's to keep alive).
"""
import math

import numpy as np
import torch

from . import _lib
from ._lib import mosaic_call as _call, ptr
from .codec import FrameCodec, frame_layout
from .corpus import check_hop, check_row_start, rows as _rows
from .mosaic import check_window, ola
from .stream import window_values
from .walk import LatentWalk

K_DENSE = 64                 # csrc/smooth.hip: the dense mode's axes
NOISE_MIN, NOISE_MAX = 1e-8, 1e8
MAX_WORKSPACE = 2 << 30


def check_noise(noise):
    """The observation noise r as a float, finite and in [1e-8, 1e8] (ValueError)."""
    try:
        r = float(noise)
    except (TypeError, ValueError):
        r = float("nan")
    if not (math.isfinite(r) and NOISE_MIN <= r <= NOISE_MAX):
        raise ValueError("noise=%r must be finite and in [1e-8, 1e8]" % (noise,))
    return r


def check_ranges(ranges, n_samples):
    """Damaged sample ranges [s, e) as int64 [n, 2]: sorted, merged where they overlap or touch, clipped to
    [0, n_samples).  ValueError for an empty or reversed range or one that lies outside the file."""
    n = int(n_samples)
    out = []
    for r in ranges:
        s, e = int(r[0]), int(r[1])
        if e <= s:
            raise ValueError("range [%d, %d) is empty" % (s, e))
        if e <= 0 or s >= n:
            raise ValueError("range [%d, %d) lies outside the %d samples" % (s, e, n))
        out.append((max(s, 0), min(e, n)))
    out.sort()
    merged = []
    for s, e in out:
        if merged and s <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], e)
        else:
            merged.append([s, e])
    return np.asarray(merged, dtype=np.int64).reshape(-1, 2)


def frame_mask(n_samples, segment_length, hop, ranges):
    """bool [frames of frame_layout(n_samples)]: frame f = samples [f hop, f hop + S) overlaps a range [s, e)."""
    S = int(segment_length)
    step = S if hop is None else int(hop)
    n_frames, _ = frame_layout(n_samples, S, hop)
    mask = np.zeros(max(n_frames, 0), dtype=bool)
    for s, e in np.asarray(ranges, dtype=np.int64).reshape(-1, 2):
        if e <= s:
            continue
        # f hop < e and f hop + S > s
        lo = max(0, (int(s) - S) // step + 1)
        hi = min(n_frames, -(-int(e) // step))
        if hi > lo:
            mask[lo:hi] = True
    return mask


def regions(mask, context):
    """[(f0, f1)]: every run of True in mask extended by `context` frames on each side, merged where two touch or
    overlap, clipped to [0, len(mask))."""
    mask = np.asarray(mask, dtype=bool)
    context = int(context)
    if context < 0:
        raise ValueError("context=%d must not be negative" % context)
    n = mask.size
    edge = np.diff(np.concatenate([[0], mask.astype(np.int8), [0]]))
    out = []
    for a, b in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)):
        f0, f1 = max(0, int(a) - context), min(n, int(b) + context)
        if out and f0 <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], f1))
        else:
            out.append((f0, f1))
    return out


def parse_ranges(text, sampling_rate):
    """'1.20:1.35,4.0:4.1' (seconds) -> [(s, e)] in samples at sampling_rate, each rounded to the nearest sample;
    ValueError naming the piece that does not parse, is negative or is empty."""
    sr = float(sampling_rate)
    out = []
    for piece in str(text).split(","):
        try:
            a, b = piece.split(":")
            a, b = float(a), float(b)
        except ValueError:
            raise ValueError("range %r: expected START:END in seconds" % piece)
        if not (math.isfinite(a) and math.isfinite(b) and 0 <= a < b):
            raise ValueError("range %r: expected 0 <= START < END" % piece)
        s, e = int(round(a * sr)), int(round(b * sr))
        if e <= s:
            raise ValueError("range %r: no sample at %g Hz" % (piece, sr))
        out.append((s, e))
    return out


def zero_runs(wave, min_run):
    """[(s, e)] of the runs of exactly-zero samples of a 1-D array that are at least min_run long."""
    min_run = int(min_run)
    if min_run < 1:
        raise ValueError("min_run=%d must be positive" % min_run)
    z = (np.asarray(wave).reshape(-1) == 0).astype(np.int8)
    edge = np.diff(np.concatenate([[0], z, [0]]))
    return [(int(a), int(b)) for a, b in zip(np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)) if b - a >= min_run]


def workspace_bytes(T, L, k, mode):
    """Bytes of ws of RV_SMOOTH_FILTER / _BACKWARD (launches nothing)."""
    return _call(_lib.SMOOTH_WORKSPACE, T=int(T), L=int(L), k=int(k), mode=int(mode)).ws_bytes


class LatentSmoother:
    """The filter and the smoother of a fitted LatentWalk on its device (see the module doc).  `mode` follows the
    walk's: dense for "full" (k <= 64), diagonal otherwise."""

    def __init__(self, walk, noise=1e-2, max_workspace_bytes=MAX_WORKSPACE):
        if not isinstance(walk, LatentWalk):
            raise TypeError("LatentSmoother needs a fitted LatentWalk, got %s" % type(walk).__name__)
        walk._fitted()
        self.walk, self.noise = walk, check_noise(noise)
        self.k, self.L = (int(v) for v in walk.R_.shape)
        self.mode = _lib.SMOOTH_DIAGONAL if walk.mode == "diagonal" else _lib.SMOOTH_DENSE
        if self.mode == _lib.SMOOTH_DENSE and self.k > K_DENSE:
            raise ValueError("the walk keeps %d axes in full mode and the dense smoother takes at most %d: refit with "
                             "--keep <= %d or --mode diagonal" % (self.k, K_DENSE, K_DENSE))
        self.max_workspace_bytes = int(max_workspace_bytes)

    def operands(self, x, row_start, weight=None):
        """(x made contiguous, the descriptor members both passes share, the tensors they point to): the checks and the
        workspace of one batch; the caller keeps the third alive until the launches have run."""
        x = _rows(x, cols=self.L)
        T = x.shape[0]
        if x.device != self.walk.mean_.device:
            raise _lib.RvError("x is on %s; the walk is on %s" % (x.device, self.walk.mean_.device))
        rs = check_row_start(row_start, T)
        if weight is not None:
            if (not torch.is_tensor(weight) or weight.dtype != torch.float32 or weight.device != x.device
                    or tuple(weight.shape) != (T,)):
                raise ValueError("weight must be a float32 device tensor of %d values on %s, got %s" % (
                    T, x.device, "%s %s on %s" % (weight.dtype, tuple(weight.shape), weight.device)
                    if torch.is_tensor(weight) else type(weight).__name__))
            weight = weight.contiguous()
        need = workspace_bytes(T, self.L, self.k, self.mode)
        if need > self.max_workspace_bytes:
            raise ValueError("the smoother's workspace for %d frames of %d axes is %d bytes, more than "
                             "max_workspace_bytes=%d: use a smaller context (fewer frames per region) or fewer axes"
                             % (T, self.k, need, self.max_workspace_bytes))
        ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        rs_dev = torch.from_numpy(rs.copy()).to(x.device)
        w = self.walk
        fields = dict(T=T, L=self.L, k=self.k, n_rows=rs.size - 1, mode=self.mode, lam=self.noise, q=ptr(x),
                      weight=ptr(weight), row_start=ptr(rs_dev), centre=ptr(w.mean_),
                      moment=ptr(w.dyn_), ws=ptr(ws), ws_bytes=need)
        return x, fields, (ws, rs_dev, weight)

    def run_filter(self, fields, result, stream=None):
        """RV_SMOOTH_FILTER on the operands `fields` (a dict of descriptor members) into result [T, ldo] or None, on the
        raw hipStream_t `stream` (None: the current stream)."""
        _call(_lib.SMOOTH_FILTER, stream, basis=ptr(self.walk.P_), result=ptr(result),
              ldo=0 if result is None else result.stride(0), **fields)

    def run_backward(self, fields, out, state, stream=None):
        """RV_SMOOTH_BACKWARD behind run_filter on the same operands."""
        _call(_lib.SMOOTH_BACKWARD, stream, basis=ptr(self.walk.R_), out=ptr(out), ldo=out.stride(0), state=ptr(state), **fields)

    @torch.no_grad()
    def filter(self, x, row_start, weight=None):
        """-> (w+ [T, k], nis [T], logdet [T]) fp64, views of one [T, k + 2] tensor."""
        x, fields, held = self.operands(x, row_start, weight)
        res = torch.empty((x.shape[0], self.k + 2), dtype=torch.float64, device=x.device)
        self.run_filter(fields, res)
        return res[:, :self.k], res[:, self.k], res[:, self.k + 1]

    @torch.no_grad()
    def smooth(self, x, row_start, weight=None):
        """-> (z [T, L] fp32, the smoothed latent rows; w_hat [T, k] fp64, the smoothed states)."""
        x, fields, held = self.operands(x, row_start, weight)
        T = x.shape[0]
        z = torch.empty((T, self.L), dtype=torch.float32, device=x.device)
        w_hat = torch.empty((T, self.k), dtype=torch.float64, device=x.device)
        self.run_filter(fields, None)
        self.run_backward(fields, z, w_hat)
        return z, w_hat


@torch.no_grad()
def splice(src, resynthesis, ranges, fade):
    """RV_SMOOTH_SPLICE: src [n] fp32 with resynthesis [n] fp32 faded in over `ranges` (check_ranges' array, at least
    one) and `fade` samples on either side of each -> [n] fp32."""
    n = src.numel()
    rg = np.ascontiguousarray(ranges, dtype=np.int64).reshape(-1, 2)
    if rg.shape[0] < 1 or (rg[:, 1] <= rg[:, 0]).any() or (rg[1:, 0] < rg[:-1, 1]).any() or rg[0, 0] < 0 or rg[-1, 1] > n:
        raise ValueError("ranges must be at least one [s, e), ascending and disjoint inside [0, %d)" % n)
    if int(fade) < 0:
        raise ValueError("fade=%d must not be negative" % int(fade))
    if (src.dtype != torch.float32 or resynthesis.dtype != torch.float32 or resynthesis.numel() != n or src.dim() != 1
            or resynthesis.dim() != 1 or src.device != resynthesis.device):
        raise ValueError("src and the resynthesis must be 1-D float32 tensors of one length on one device")
    room = torch.from_numpy(rg.astype(np.int32)).to(src.device)
    out = torch.empty_like(src)
    _call(_lib.SMOOTH_SPLICE, src=ptr(src.contiguous()), frames=ptr(resynthesis.contiguous()), room=ptr(room),
          n_rows=rg.shape[0], width=int(fade), n_out=n, out=ptr(out))
    return out


def check_context(context, fade, segment_length, hop):
    """context >= ceil((S + fade) / hop): every replaced sample then has its full set of overlapping frames inside the
    region; ValueError naming both."""
    need = -(-(int(segment_length) + int(fade)) // int(hop))
    if int(context) < need:
        raise ValueError("context=%d frames is too short for segment_length %d, fade=%d and hop %d: it must be at least "
                         "%d" % (int(context), int(segment_length), int(fade), int(hop), need))
    return int(context)


def _encode(model, walk, wave, hop):
    codec = FrameCodec(model)
    if walk.mean_.numel() != codec.L:
        raise ValueError("the walk was fitted on %d-dimensional latents, the model has latent_dim %d" % (
            walk.mean_.numel(), codec.L))
    w = codec.wave(wave)
    padded, n_frames = codec.pad(w, w.numel(), hop)
    mu, _ = codec.encode(padded, n_frames, hop)
    return codec, w, mu, n_frames, padded.numel()


@torch.no_grad()
def restore(model, walk, wave, ranges, hop=None, window=None, noise=1e-2, context=32, fade=64, fitted_hop=Ellipsis,
            max_workspace_bytes=MAX_WORKSPACE):
    """The waveform with the damaged sample `ranges` filled from the walk's posterior mean -> [n] fp32 on the model's
    device.  Everything outside [s - fade, e + fade) of every range is the input bit for bit.  fitted_hop: the hop the
    walk was fitted at (read_walk's meta["hop"]; None: non-overlapping frames), checked against `hop` when given."""
    S = int(model.segment_length)
    step = S if hop is None else int(hop)
    if fitted_hop is not Ellipsis:
        check_hop(fitted_hop, hop, S)
    check_window(S, step, window)
    check_context(context, fade, S, step)
    smoother = LatentSmoother(walk, noise, max_workspace_bytes)
    codec, w, mu, n_frames, n_padded = _encode(model, walk, wave, hop)
    n = w.numel()
    rg = check_ranges(ranges, n)
    if rg.shape[0] == 0:
        return w.clone()
    mask = frame_mask(n, S, hop, rg)
    regs = regions(mask, context)
    rows = np.concatenate([np.arange(f0, f1) for f0, f1 in regs])
    rs = np.concatenate([[0], np.cumsum([f1 - f0 for f0, f1 in regs])]).astype(np.int64)
    x = mu[torch.from_numpy(rows).to(mu.device)].contiguous()
    weight = torch.from_numpy((~mask[rows]).astype(np.float32)).to(mu.device)
    z, _ = smoother.smooth(x, rs, weight)
    frames = codec.decode(z)
    win = None if window is None else torch.from_numpy(window_values(S, window)).to(mu.device)
    y = torch.zeros(n_padded, dtype=torch.float32, device=mu.device)
    for r, (f0, f1) in enumerate(regs):
        span = (f1 - f0 - 1) * step + S
        ola(frames[rs[r]:rs[r + 1]], step, span, win, out=y[f0 * step:f0 * step + span])
    return splice(w, y[:n], rg, fade)


@torch.no_grad()
def surprise(model, walk, wave, hop=None, noise=1e-2, fitted_hop=Ellipsis, max_workspace_bytes=MAX_WORKSPACE):
    """nis / k per frame of the waveform, from the filter alone over all frames as one sequence: about 1 where the frame
    moves as the corpus does, large where it does not -> [frames] fp64."""
    S = int(model.segment_length)
    if fitted_hop is not Ellipsis:
        check_hop(fitted_hop, hop, S)
    smoother = LatentSmoother(walk, noise, max_workspace_bytes)
    _, _, mu, n_frames, _ = _encode(model, walk, wave, hop)
    _, nis, _ = smoother.filter(mu, np.asarray([0, n_frames], dtype=np.int64))
    return nis / smoother.k
