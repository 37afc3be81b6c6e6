"""Time alignment of two recordings in the latent space: banded dynamic time warping over the encoder's mu rows, and the
morph, distance and search built on it (the RV_ALIGN_* ops of rv_mosaic; the rules: include/rawvae_hip.h, "Latent
alignment"; csrc/align.hip).

  local_costs(a, b, band)            Dm [Ta, W] fp32: the search's squared distance of every pair of rows in the band
  forward(dm, Ta, Tb, band, ...)     the DP over the anti-diagonals in fp64 (one workgroup), the back table into ws
  backtrack(dm, Ta, Tb, band, ws)    (path [Ta + Tb - 1, 2] int32, summary [4] int32, costs [2] fp64)
  warp(path, summary, Ta, Tb, timeline)   index table [n, 2] int32 = (ia, ib) on A's, B's or the path's timeline
  workspace_bytes(Ta, Tb, band)
  align_latents(a, b, band, penalty, mode)   the first three on two latent trajectories -> Alignment
  CapturedAlignment(Ta, Tb, L, band, ...)    the same three launches captured as one graph on static buffers
  LatentAligner(model, max_rows)     align(a, b, hop, band, penalty) of two waveforms -> Alignment (path, cost,
                                     path_cost, normalised_cost, band, mu / logvar of both sounds);
                                     find(query, recording, hop, penalty): where the query occurs (subsequence DTW)
  AlignedInterpolator(model)         curve(...) / stepwise(...): LatentInterpolator's mixes along the warping path,
                                     overlap-added at `hop` with `window`

`band` is in frames: cell (i, j) is kept iff |j - floor(i (Tb - 1) / max(Ta - 1, 1))| <= band; None (or 0) is the whole
matrix.  Nothing here syncs except reading the path length P (Alignment.P and what follows from it).
"""
import functools

import numpy as np
import torch

from . import _lib
from ._lib import RvError, mosaic_call as _call, ptr
from .codec import FrameCodec
from .corpus import rows
from .interpolate import LatentInterpolator
from .stream import GraphReplay, window_values

MODES = {"global": _lib.ALIGN_GLOBAL, "subsequence": _lib.ALIGN_SUBSEQUENCE}
TIMELINES = {"a": _lib.ALIGN_ON_A, "b": _lib.ALIGN_ON_B, "path": _lib.ALIGN_ON_PATH}
L_MAX = 4096
CELL_LIMIT = (1 << 31) - 1     # Ta * W, the band slots of one alignment (the library's own limit)


def band_admits(Ta, Tb, band):
    """Whether the band holds a monotone path from (0, 0) to (Ta - 1, Tb - 1) (the header's rule)."""
    Ta, Tb, r = int(Ta), int(Tb), int(band or 0)
    if r == 0:
        return True
    if Ta == 1:
        return Tb - 1 <= r
    return -(-(Tb - 1) // (Ta - 1)) <= 2 * r + 1


def least_band(Ta, Tb):
    """The least band >= 1 that admits a path."""
    Ta, Tb = int(Ta), int(Tb)
    if Ta == 1:
        return max(1, Tb - 1)
    return max(1, -(-(Tb - 1) // (Ta - 1)) // 2)


def check_band(Ta, Tb, band, cell_limit=CELL_LIMIT):
    """`band` (None: the whole matrix) as the library's band for Ta x Tb frames; ValueError naming `band` when it is
    not a non-negative integer, admits no path, or the cells exceed `cell_limit` (then naming the least band that
    admits a path and the widest that fits)."""
    Ta, Tb = int(Ta), int(Tb)
    if Ta < 1 or Tb < 1:
        raise ValueError("an alignment needs at least one frame of each sound, got %d and %d" % (Ta, Tb))
    if band is None:
        band = 0
    if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or band < 0:
        raise ValueError("band=%r must be a non-negative number of frames or None" % (band,))
    band = int(band)
    if not band_admits(Ta, Tb, band):
        raise ValueError("band=%d admits no path through %d x %d frames: the least band that does is %d"
                         % (band, Ta, Tb, least_band(Ta, Tb)))
    W = 2 * band + 1 if band else Tb
    if Ta * W > cell_limit:
        least, widest = least_band(Ta, Tb), (cell_limit // Ta - 1) // 2
        if widest < least:
            raise ValueError("band=%s: %d x %d frames exceed the limit of %d cells at every band that admits a path "
                             "(the least is %d)" % (band or None, Ta, Tb, cell_limit, least))
        raise ValueError("band=%s: %d x %d cells exceed the limit of %d; the least band that admits a path is %d, the "
                         "widest that fits is %d" % (band or None, Ta, W, cell_limit, least, widest))
    return band


def check_penalty(penalty):
    p = float(penalty)
    if not 0 <= p <= float(np.finfo(np.float32).max):
        raise ValueError("penalty=%r must be a finite fp32 number >= 0" % (penalty,))
    return p


_rows = functools.partial(rows, empty_ok=True)


def band_slots(Tb, band):
    return 2 * int(band) + 1 if band else int(Tb)


def workspace_bytes(Ta, Tb, band=0):
    """Bytes of device workspace forward and backtrack share for these extents."""
    return _call(_lib.ALIGN_WORKSPACE, T=int(Ta), N=int(Tb), band=int(band or 0)).ws_bytes


def workspace(Ta, Tb, band, device):
    n = workspace_bytes(Ta, Tb, band)
    return torch.empty(n, dtype=torch.uint8, device=device)


def local_costs(a, b, band=0, out=None, stream=None):
    """Dm [Ta, W] fp32 of a [Ta, L] and b [Tb, L]: RV_ALIGN_COST."""
    a, b = _rows(a, "a"), _rows(b, "b")
    if a.shape[1] != b.shape[1] or a.device != b.device:
        raise ValueError("a %s and b %s must share L and device" % (tuple(a.shape), tuple(b.shape)))
    Ta, Tb, L = a.shape[0], b.shape[0], a.shape[1]
    r = check_band(Ta, Tb, band)
    if out is None:
        out = torch.empty((Ta, band_slots(Tb, r)), dtype=torch.float32, device=a.device)
    _call(_lib.ALIGN_COST, stream, T=Ta, N=Tb, L=L, band=r, a=ptr(a), b=ptr(b), local_costs=ptr(out))
    return out


def forward(dm, Ta, Tb, band=0, mode="global", penalty=0.0, ws=None, end_costs=None, stream=None):
    """RV_ALIGN_FORWARD over dm [Ta, W] -> ws (the back table and the end cell); end_costs [Tb] fp64 receives
    C[Ta - 1, .] in mode "subsequence"."""
    if mode not in MODES:
        raise ValueError("mode=%r: expected 'global' or 'subsequence'" % (mode,))
    r = check_band(Ta, Tb, band)
    if ws is None:
        ws = workspace(Ta, Tb, r, dm.device)
    _call(_lib.ALIGN_FORWARD, stream, T=int(Ta), N=int(Tb), band=r, mode=MODES[mode], penalty=check_penalty(penalty),
          ws=ptr(ws), ws_bytes=ws.numel(), local_costs=ptr(dm), end_costs=ptr(end_costs))
    return ws


def backtrack(dm, Ta, Tb, band, ws, out=None, stream=None):
    """RV_ALIGN_BACKTRACK -> (path [Ta + Tb - 1, 2] int32, summary [4] int32 = {P, first j, last j, reached},
    costs [2] fp64 = {C at the end, the path's own sum}); out: the three tensors to write into."""
    r = check_band(Ta, Tb, band)
    if out is None:
        dev = dm.device
        out = (torch.empty((Ta + Tb - 1, 2), dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev),
               torch.empty(2, dtype=torch.float64, device=dev))
    path, summary, costs = out
    _call(_lib.ALIGN_BACKTRACK, stream, T=int(Ta), N=int(Tb), band=r, ws=ptr(ws), ws_bytes=ws.numel(),
          local_costs=ptr(dm), path=ptr(path), summary=ptr(summary), path_costs=ptr(costs))
    return path, summary, costs


def warp(path, summary, Ta, Tb, timeline="a", out=None, stream=None):
    """RV_ALIGN_WARP -> idx [n, 2] int32 = (ia, ib), n = Ta ("a"), Tb ("b") or Ta + Tb - 1 ("path", -1 beyond P)."""
    if timeline not in TIMELINES:
        raise ValueError("timeline=%r: expected 'a', 'b' or 'path'" % (timeline,))
    n = {"a": Ta, "b": Tb, "path": Ta + Tb - 1}[timeline]
    if out is None:
        out = torch.empty((n, 2), dtype=torch.int32, device=path.device)
    _call(_lib.ALIGN_WARP, stream, T=int(Ta), N=int(Tb), mode=TIMELINES[timeline],
          path=ptr(path), summary=ptr(summary), warp_table=ptr(out))
    return out


class Alignment:
    """The result of one alignment; everything stays on the device until a host value (P, cost, ...) is asked for."""

    def __init__(self, Ta, Tb, band, mode, penalty, path_rows, summary, costs, end_costs=None, dists=None):
        self.Ta, self.Tb, self.band, self.mode, self.penalty = Ta, Tb, band or None, mode, penalty
        self.path_rows, self.summary, self.costs, self.end_costs = path_rows, summary, costs, end_costs
        self.mu_a, self.logvar_a, self.mu_b, self.logvar_b = dists if dists is not None else (None,) * 4
        self._host = None

    def _read(self):
        if self._host is None:
            s, c = self.summary.cpu().numpy(), self.costs.cpu().numpy()     # the one sync
            self._host = (int(s[0]), int(s[1]), int(s[2]), bool(s[3]), float(c[0]), float(c[1]))
        return self._host

    P = property(lambda self: self._read()[0])
    first_b = property(lambda self: self._read()[1])
    last_b = property(lambda self: self._read()[2])
    reached = property(lambda self: self._read()[3])
    cost = property(lambda self: self._read()[4])
    path_cost = property(lambda self: self._read()[5])

    @property
    def normalised_cost(self):
        return self.path_cost / self.P if self.P else float("inf")

    @property
    def path(self):
        """The path [P, 2] int32 on the device."""
        return self.path_rows[:self.P]

    def warp(self, timeline="a"):
        """The index table of `timeline`; "path" is cut to its P rows."""
        idx = warp(self.path_rows, self.summary, self.Ta, self.Tb, timeline)
        return idx[:self.P] if timeline == "path" else idx


def align_latents(a, b, band=None, penalty=0.0, mode="global", dists=None):
    """DTW of two latent trajectories a [Ta, L], b [Tb, L] (fp32 device tensors) -> Alignment.  Three launches."""
    a, b = _rows(a, "a"), _rows(b, "b")
    Ta, Tb = a.shape[0], b.shape[0]
    if a.shape[1] > L_MAX:
        raise ValueError("rows of %d values: at most %d" % (a.shape[1], L_MAX))
    r = check_band(Ta, Tb, band)
    if mode == "subsequence" and r:
        raise ValueError("band=%d: a subsequence search runs on the whole matrix (band None)" % r)
    dm = local_costs(a, b, r)
    end_costs = torch.empty(Tb, dtype=torch.float64, device=a.device) if mode == "subsequence" else None
    ws = forward(dm, Ta, Tb, r, mode, penalty, end_costs=end_costs)
    path, summary, costs = backtrack(dm, Ta, Tb, r, ws)
    return Alignment(Ta, Tb, r, mode, penalty, path, summary, costs, end_costs, dists)


class CapturedAlignment(GraphReplay):
    """local_costs, forward and backtrack of fixed extents captured as one graph: replay(a, b) copies the two
    trajectories into static buffers and launches it -> the Alignment on static output tensors (overwritten by the
    next replay)."""
    n_streams, block = 1, 1     # GraphReplay's block buffers are not used: the operands have their own static tensors

    def __init__(self, Ta, Tb, L, band=None, penalty=0.0, mode="global", device="cuda"):
        self.device = torch.device(device)
        self.Ta, self.Tb, self.L, self.mode, self.penalty = int(Ta), int(Tb), int(L), mode, check_penalty(penalty)
        self.r = check_band(Ta, Tb, band)
        dev = self.device
        self.a = torch.zeros((self.Ta, self.L), dtype=torch.float32, device=dev)
        self.b = torch.zeros((self.Tb, self.L), dtype=torch.float32, device=dev)
        self.dm = torch.empty((self.Ta, band_slots(Tb, self.r)), dtype=torch.float32, device=dev)
        self.ws = workspace(Ta, Tb, self.r, dev)
        self.end_costs = torch.empty(self.Tb, dtype=torch.float64, device=dev) if mode == "subsequence" else None
        self.out = (torch.empty((self.Ta + self.Tb - 1, 2), dtype=torch.int32, device=dev),
                    torch.empty(4, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.float64, device=dev))

    def parameters(self):
        return []

    def _launch(self, st):
        local_costs(self.a, self.b, self.r, self.dm, st)
        forward(self.dm, self.Ta, self.Tb, self.r, self.mode, self.penalty, self.ws, self.end_costs, st)
        backtrack(self.dm, self.Ta, self.Tb, self.r, self.ws, self.out, st)

    def capture(self):
        return self._capture(self._launch)

    def replay(self, a, b):
        self.a.copy_(a)
        self.b.copy_(b)
        self._replay(0, "replay()")
        return Alignment(self.Ta, self.Tb, self.r, self.mode, self.penalty, *self.out, self.end_costs)


class Match:
    """Where a query occurs in a recording (LatentAligner.find): frames [start_frame, end_frame], samples
    [start_sample, end_sample), cost (the accumulated cost of the best path; +inf: none), end_costs [Tb] fp64 on the
    device (the cost of the best path ending at every frame of the recording) and the Alignment itself."""

    def __init__(self, alignment, step, S, n_samples):
        self.alignment, self.end_costs = alignment, alignment.end_costs
        self.found, self.cost = alignment.reached, alignment.cost
        self.start_frame, self.end_frame = (alignment.first_b, alignment.last_b) if self.found else (-1, -1)
        self.start_sample = self.start_frame * step if self.found else -1
        self.end_sample = min(self.end_frame * step + S, int(n_samples)) if self.found else -1


class LatentAligner:
    """Align two waveforms frame by frame in a `VAE`'s latent space (see the module doc).  `codec` is the FrameCodec
    that frames and encodes; the model's parameters are read, never written."""

    def __init__(self, model, max_rows=16384, cell_limit=CELL_LIMIT):
        self.codec = c = FrameCodec(model, max_rows)
        self.model, self.device, self.S, self.L = model, c.device, c.S, c.L
        self.cell_limit = int(cell_limit)

    def encode(self, wave, hop=None):
        """(mu, logvar, samples) of a waveform at its own length."""
        w = self.codec.wave(wave)
        padded, n_frames = self.codec.pad(w, w.numel(), hop)
        return self.codec.encode(padded, n_frames, hop) + (w.numel(),)

    @torch.no_grad()
    def align(self, a, b, hop=None, band=None, penalty=0.0):
        """Global DTW of the mu rows of two waveforms -> Alignment."""
        penalty = check_penalty(penalty)
        mu_a, lv_a, _ = self.encode(a, hop)
        mu_b, lv_b, _ = self.encode(b, hop)
        r = check_band(mu_a.shape[0], mu_b.shape[0], band, self.cell_limit)
        return align_latents(mu_a, mu_b, r, penalty, "global", (mu_a, lv_a, mu_b, lv_b))

    @torch.no_grad()
    def find(self, query, recording, hop=None, penalty=0.0):
        """Subsequence DTW: the stretch of `recording` that the whole of `query` aligns with best -> Match."""
        penalty = check_penalty(penalty)
        mu_q, lv_q, _ = self.encode(query, hop)
        mu_r, lv_r, n = self.encode(recording, hop)
        check_band(mu_q.shape[0], mu_r.shape[0], None, self.cell_limit)
        al = align_latents(mu_q, mu_r, None, penalty, "subsequence", (mu_q, lv_q, mu_r, lv_r))
        return Match(al, self.S if hop is None else int(hop), self.S, n)


class AlignedInterpolator(LatentInterpolator):
    """LatentInterpolator's mixes along the warping path of the two sounds: frame n of the output mixes the frame of A
    and the frame of B that the alignment pairs on the chosen timeline ("a": one output frame per frame of A, "b": per
    frame of B, "path": per step of the path), then the frames are overlap-added at `hop` with `window` (hop None: the
    frames concatenated).  The alpha conventions, eps and seed are LatentInterpolator.curve's / .stepwise's; the output
    frames n take their place in them.  `last_alignment` is the Alignment of the last call."""

    def __init__(self, model, max_rows=16384, cell_limit=CELL_LIMIT):
        super().__init__(model, max_rows)
        self.aligner = LatentAligner(model, max_rows, cell_limit)
        self._request, self.last_alignment = ("a", None, 0.0), None

    def _sources(self, a, b, hop, match):
        timeline, band, penalty = self._request
        self.last_alignment = al = self.aligner.align(a, b, hop, band, penalty)
        if not al.reached:      # reads the summary: the one sync; it also sizes the "path" timeline
            raise RvError("the two sounds cannot be aligned: no path of finite cost (a NaN frame?)")
        idx = al.warp(timeline).long()
        ia, ib = idx[:, 0].contiguous(), idx[:, 1].contiguous()
        rows = (al.mu_a.index_select(0, ia), al.logvar_a.index_select(0, ia), al.mu_b.index_select(0, ib),
                al.logvar_b.index_select(0, ib))
        return rows, idx.shape[0]

    def _overlap(self, flat, hop, window):
        if hop is None:
            return flat
        from .mosaic import ola
        frames = flat.view(-1, self.S)
        w = None if window is None else torch.from_numpy(window_values(self.S, window)).to(self.device)
        return ola(frames, int(hop), (frames.shape[0] - 1) * int(hop) + self.S, w)

    def _check(self, hop, window, timeline, band, penalty):
        from .mosaic import check_window
        if timeline not in TIMELINES:
            raise ValueError("timeline=%r: expected 'a', 'b' or 'path'" % (timeline,))
        check_window(self.S, self.S if hop is None else hop, window)
        if window is not None and hop is None:
            raise ValueError("window %r needs a hop: without one the frames are concatenated" % (window,))
        self._request = (timeline, band, check_penalty(penalty))

    @torch.no_grad()
    def curve(self, a, b, curve_or_alpha, hop=None, window=None, timeline="a", band=None, penalty=0.0, eps=None, seed=0):
        """LatentInterpolator.curve along the warping path -> 1-D fp32 waveform."""
        self._check(hop, window, timeline, band, penalty)
        return self._overlap(LatentInterpolator.curve(self, a, b, curve_or_alpha, hop, eps, seed), hop, window)

    @torch.no_grad()
    def stepwise(self, a, b, alphas, hop=None, window=None, timeline="a", band=None, penalty=0.0, eps=None, seed=0):
        """LatentInterpolator.stepwise along the warping path: the K blocks of n frames, each block overlap-added on
        its own, concatenated in the order of `alphas`."""
        self._check(hop, window, timeline, band, penalty)
        flat = LatentInterpolator.stepwise(self, a, b, alphas, hop, eps, seed)
        K = np.asarray(alphas).size
        return torch.cat([self._overlap(blk.contiguous(), hop, window) for blk in flat.view(K, -1)])
