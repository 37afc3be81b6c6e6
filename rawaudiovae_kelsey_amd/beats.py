"""The pulse of a recording in the latent space: onset strength, tempo and beats (the RV_BEAT_* ops of rv_mosaic; the
rules: include/rawvae_hip.h, "Latent beats"; csrc/beat.hip).

  lag_range(bpm_min, bpm_max, sampling_rate, step)   (lo, hi): the periods in frames the tempogram looks at
  tempo_prior(lo, hi, centre, octaves)   the log-normal weight of every period, on the host (centre None: all ones)
  window_values(Wn)                  the tempogram's Hann window [Wn] float64, on the host
  penalty_table(P, tightness)        (dlo, dhi, pen): the tracker's transition scores for the period P, on the host
  onset(nov)                         (o [T] fp64, summary [4] int32, cost [2] fp64): the novelty curve rectified, over its RMS
  tempogram(o, Wn, Hw, lo, hi, win, prior)   (A [nW, lags], G [lags], period [nW] int32, info [4] int32, cost [2] fp64)
  track(o, P, pen, dlo, dhi)         (C [T], back [T] int32, beats [n_out] int32, summary [4] int32, cost [2] fp64)
  workspace_bytes(T)                 the bytes of device workspace onset needs
  track_latents(mu, kernel, ...)     self_costs, novelty, onset, tempogram, (read P), track on a latent trajectory -> Beats
  BeatTracker(model, max_rows)       track(wave, hop, ...) -> Beats

Two syncs, and no other: track_latents reads the period P between the tempogram and the tracker (the tracker's window
and its table depend on it), and Beats reads the number of beats n when a host value (beat_frames, ...) is asked for.
"""
import math

import numpy as np
import torch

from . import _lib
from . import align as _align
from . import structure as _struct
from ._lib import mosaic_call as _call, ptr
from .codec import FrameCodec

W_MAX = 8192        # the longest tempogram window in frames
LAG_MAX = 1024      # the largest period the tempogram looks at
D_MAX = 2048        # the furthest predecessor of the tracker, and its longest end window


def _whole(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError("%s=%r must be a whole number in [%d, %d]" % (name, v, lo, hi))
    return int(v)


def _real(name, v, positive=True):
    try:
        x = float(v)
    except (TypeError, ValueError):
        x = float("nan")
    if not math.isfinite(x) or x < 0 or (positive and x == 0):
        raise ValueError("%s=%r must be a finite number %s 0" % (name, v, ">" if positive else ">="))
    return x


def lag_range(bpm_min, bpm_max, sampling_rate, step):
    """(lo, hi) = (ceil(60 sr / (step bpm_max)), floor(60 sr / (step bpm_min))): the periods in frames of the tempi
    [bpm_min, bpm_max] at `step` samples a frame.  ValueError naming the argument when no period is left or hi > 1024."""
    bpm_min, bpm_max = _real("bpm_min", bpm_min), _real("bpm_max", bpm_max)
    sr, step = _real("sampling_rate", sampling_rate), _real("step", step)
    lo, hi = math.ceil(60.0 * sr / (step * bpm_max)), math.floor(60.0 * sr / (step * bpm_min))
    lo = max(lo, 1)
    if hi > LAG_MAX:
        raise ValueError("bpm_min=%r is a period of %d frames of %g samples: at most %d (a larger hop or a faster "
                         "bpm_min)" % (bpm_min, hi, step, LAG_MAX))
    if lo > hi:
        raise ValueError("bpm_max=%r leaves no period between bpm_min=%r and it: %d > %d frames" % (bpm_max, bpm_min, lo, hi))
    return lo, hi


def check_lags(lo, hi):
    lo = _whole("lo", lo, 1, LAG_MAX)
    return lo, _whole("hi", hi, lo, LAG_MAX)


def tempo_prior(lo, hi, centre, octaves=1.0):
    """prior [hi - lo + 1] float64 = exp(-1/2 (log2(tau / centre) / octaves)^2) for tau = lo .. hi; centre None: ones."""
    lo, hi = check_lags(lo, hi)
    tau = np.arange(lo, hi + 1, dtype=np.float64)
    if centre is None:
        return np.ones(tau.size, dtype=np.float64)
    centre, octaves = _real("centre", centre), _real("octaves", octaves)
    return np.exp(-0.5 * (np.log2(tau / centre) / octaves) ** 2)


def window_values(Wn):
    """The Hann window on Wn points taken between the samples, w[i] = 1/2 - 1/2 cos(2 pi (i + 1/2) / Wn): no point is 0
    and Wn = 1 gives 1."""
    Wn = _whole("Wn", Wn, 1, W_MAX)
    n = np.arange(Wn, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (n + 0.5) / Wn)


def penalty_table(P, tightness=100.0):
    """(dlo, dhi, pen) = ((P + 1) // 2, 2 P, -tightness ln(delta / P)^2 for delta = dlo .. dhi): Ellis' transition
    score between two beats delta frames apart when the period is P."""
    P = _whole("P", P, 1, D_MAX // 2)
    tightness = _real("tightness", tightness, positive=False)
    dlo, dhi = (P + 1) // 2, 2 * P
    d = np.arange(dlo, dhi + 1, dtype=np.float64)
    return dlo, dhi, -tightness * np.log(d / P) ** 2


def workspace_bytes(T):
    """Bytes of device workspace onset needs for T frames."""
    return _call(_lib.BEAT_WORKSPACE, T=int(T)).ws_bytes


def workspace(T, device):
    return torch.empty(workspace_bytes(T), dtype=torch.uint8, device=device)


def _curve(x, name):
    if not torch.is_tensor(x) or x.dtype != torch.float64 or x.dim() != 1 or x.device.type != "cuda" or x.numel() < 1:
        raise ValueError("%s must be a 1-D float64 device tensor of at least one frame" % name)
    return x.contiguous()


def _table(x, n, name, device):
    """A host or device table as the [n] fp64 device tensor the ops read."""
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    if x.dtype != torch.float64 or x.dim() != 1 or x.numel() != n:
        raise ValueError("%s must hold %d float64 values, got %s %s" % (name, n, x.dtype, tuple(x.shape)))
    return x.to(device).contiguous()


def onset(nov, ws=None, out=None, stream=None):
    """RV_BEAT_ONSET over nov [T] fp64 -> (o [T] fp64, summary [4] int32 = {entries > 0, finite entries, 0, 0}, cost [2]
    fp64 = {the RMS s, 0}); out: the three tensors to write into."""
    nov = _curve(nov, "nov")
    T, dev = nov.numel(), nov.device
    if ws is None:
        ws = workspace(T, dev)
    if out is None:
        out = (torch.empty(T, dtype=torch.float64, device=dev), torch.empty(4, dtype=torch.int32, device=dev),
               torch.empty(2, dtype=torch.float64, device=dev))
    o, summary, cost = out
    _call(_lib.BEAT_ONSET, stream, T=T, moment=ptr(nov), ws=ptr(ws), ws_bytes=ws.numel(), result=ptr(o), summary=ptr(summary),
          cost=ptr(cost))
    return o, summary, cost


def n_windows(T, Hw):
    return -(-int(T) // int(Hw))


def tempogram_table(win, prior, Wn, lo, hi, device):
    """[ win (Wn) | prior (hi - lo + 1) ] as the fp64 device tensor RV_BEAT_TEMPOGRAM reads."""
    return torch.cat([_table(win, Wn, "win", device), _table(prior, hi - lo + 1, "prior", device)])


def tempogram(o, Wn, Hw, lo, hi, win=None, prior=None, table=None, out=None, stream=None):
    """RV_BEAT_TEMPOGRAM over o [T] fp64 -> (A [nW, hi - lo + 1], G [hi - lo + 1], period [nW] int32, info [4] int32 =
    {P, nW, 0, 0}, cost [2] = {score[P], G[P]}).  win None: window_values(Wn); prior None: all ones; table: the tensor
    tempogram_table made of the two; out: the five tensors to write into (A may have a row pitch above the lags)."""
    o = _curve(o, "o")
    T, dev = o.numel(), o.device
    Wn, Hw = _whole("Wn", Wn, 1, W_MAX), _whole("Hw", Hw, 1, (1 << 31) - 1)
    lo, hi = check_lags(lo, hi)
    nlag, nW = hi - lo + 1, n_windows(T, Hw)
    if table is None:
        table = tempogram_table(window_values(Wn) if win is None else win, np.ones(nlag) if prior is None else prior,
                                Wn, lo, hi, dev)
    if table.dtype != torch.float64 or table.numel() != Wn + nlag or not table.is_contiguous():
        raise ValueError("table must hold Wn + lags = %d contiguous float64 values" % (Wn + nlag))
    if out is None:
        out = (torch.empty((nW, nlag), dtype=torch.float64, device=dev), torch.empty(nlag, dtype=torch.float64, device=dev),
               torch.empty(nW, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev),
               torch.empty(2, dtype=torch.float64, device=dev))
    A, G, period, info, cost = out
    if A.dim() != 2 or A.shape != (nW, nlag) or A.stride(1) != 1 or A.stride(0) < nlag:
        raise ValueError("A must be [%d, %d] with unit column stride, got %s" % (nW, nlag, tuple(A.shape)))
    _call(_lib.BEAT_TEMPOGRAM, stream, T=T, moment=ptr(o), width=Wn, hop=Hw, lag=lo, N=hi, basis=ptr(table), result=ptr(A),
          ldo=A.stride(0) if nW > 1 else max(A.stride(0), nlag), centre=ptr(G), path=ptr(period), info=ptr(info), cost=ptr(cost))
    return A, G, period, info, cost


def track(o, P, pen, dlo, dhi, out=None, stream=None):
    """RV_BEAT_TRACK over o [T] fp64 with the end window P and the transition scores pen [dhi - dlo + 1] (numpy or device
    tensor) -> (C [T], back [T] int32, beats [(T - 1) // dlo + 1] int32: the beats ascending, then -1, summary [4] int32 =
    {n, t*, 0, 0}, cost [2] = {C[t*], the onset strength summed over the beats})."""
    o = _curve(o, "o")
    T, dev = o.numel(), o.device
    P = _whole("P", P, 1, D_MAX)
    dlo = _whole("dlo", dlo, 1, D_MAX)
    dhi = _whole("dhi", dhi, dlo, D_MAX)
    pen = _table(pen, dhi - dlo + 1, "pen", dev)
    if out is None:
        out = (torch.empty(T, dtype=torch.float64, device=dev), torch.empty(T, dtype=torch.int32, device=dev),
               torch.empty((T - 1) // dlo + 1, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev),
               torch.empty(2, dtype=torch.float64, device=dev))
    C, back, beats, summary, cost = out
    _call(_lib.BEAT_TRACK, stream, T=T, moment=ptr(o), lag=dlo, width=dhi, N=P, basis=ptr(pen), result=ptr(C), idx=ptr(back),
          path=ptr(beats), n_out=beats.numel(), summary=ptr(summary), cost=ptr(cost))
    return C, back, beats, summary, cost


class Beats:
    """The result of one beat tracking; the tensors stay on the device.  `period` (frames, 0: silence, no pulse found) was
    read when the result was made; the number of beats is read when a host value is first asked for.  `step` is the hop
    between frames in samples, `n_samples` the length of the sound."""

    def __init__(self, onset, tempogram, window_periods, period, lags, window_hop, tracked=None, kernel=None, band=None,
                 mu=None, step=None, n_samples=None, sampling_rate=None):
        self.onset, self.tempogram, self.window_periods = onset, tempogram, window_periods
        self.period, self.lags, self.window_hop = int(period), tuple(lags), int(window_hop)
        self.T, self.kernel, self.band, self.mu = onset.numel(), kernel, band, mu
        self.step, self.n_samples, self.sampling_rate = step, n_samples, sampling_rate
        self._tracked, self._host = tracked, None

    silent = property(lambda self: self.period == 0, doc="no period had a positive score: there are no beats")

    def _read(self):
        if self._host is None:
            if self._tracked is None:
                self._host = np.zeros(0, np.int64)
            else:
                n = int(self._tracked[3][0])                         # the sync
                self._host = self._tracked[2][:n].cpu().numpy().astype(np.int64)
        return self._host

    beat_frames = property(lambda self: self._read(), doc="the beats in frames, ascending, as a numpy int64 array")
    n_beats = property(lambda self: self._read().size)

    @property
    def score(self):
        """C[t*], the tracker's score of the whole path; 0 without beats."""
        return 0.0 if self._tracked is None else float(self._tracked[4][0])

    def _framed(self, what):
        if what is None:
            raise ValueError("these beats have no framing: they were made from latents, not from a waveform")
        return what

    @property
    def beat_samples(self):
        return self.beat_frames * int(self._framed(self.step))

    @property
    def beat_seconds(self):
        if self.sampling_rate is None:
            raise ValueError("these beats have no sampling_rate")
        return self.beat_samples / float(self.sampling_rate)

    def _bpm(self, period):
        sr, step = self.sampling_rate, self._framed(self.step)
        if sr is None:
            raise ValueError("these beats have no sampling_rate")
        period = np.asarray(period, np.float64)
        with np.errstate(divide="ignore"):
            return np.where(period > 0, 60.0 * float(sr) / (float(step) * np.where(period > 0, period, 1.0)), 0.0)

    bpm = property(lambda self: float(self._bpm(self.period)), doc="60 sr / (step period); 0 when silent")

    @property
    def bpm_over_time(self):
        """[nW] float64: the tempo every tempogram window prefers (0 where it holds no pulse)."""
        return self._bpm(self.window_periods.cpu().numpy())

    @property
    def intervals(self):
        """(mean, standard deviation) of the inter-beat interval in frames; (0, 0) with fewer than two beats."""
        d = np.diff(self.beat_frames).astype(np.float64)
        return (float(d.mean()), float(d.std())) if d.size else (0.0, 0.0)

    def segments(self, meter=4):
        """(sample_offsets, labels) that cut the sound at its beats: 0, the beats in samples, the length; the label of a
        piece is its beat's index mod `meter`, and the stretch before the first beat (if any) is a piece of its own,
        labelled `meter`."""
        meter = _whole("meter", meter, 1, 1 << 20)
        n = int(self._framed(self.n_samples))
        at = [int(v) for v in self.beat_samples if 0 <= v < n]
        labels = [k % meter for k in range(len(at))]
        if not at or at[0] > 0:
            at, labels = [0] + at, [meter] + labels
        return np.array(at + [n], np.int64), np.array(labels, np.int64)


def track_latents(mu, kernel=8, sigma=0.5, lags=(16, 128), window=512, window_hop=None, centre=None, octaves=1.0,
                  tightness=100.0, band=None, **about):
    """Onset curve, tempo and beats of a latent trajectory mu [T, L] (fp32 device tensor) -> Beats.  self_costs and
    novelty with a kernel of half-width `kernel` frames (structure.py), onset, tempogram over the periods lags = (lo, hi)
    in windows of `window` frames every `window_hop` (None: an eighth of a window) under tempo_prior(centre, octaves), then --
    after reading P, the first sync -- track with penalty_table(P, tightness)."""
    mu = _align._rows(mu, "mu")
    T, R = mu.shape[0], _struct.check_kernel(kernel)
    lo, hi = check_lags(*lags)
    Wn = _whole("window", window, 1, W_MAX)
    Hw = max(1, Wn // 8) if window_hop is None else _whole("window_hop", window_hop, 1, (1 << 31) - 1)
    prior = tempo_prior(lo, hi, centre, octaves)
    r = _struct.check_struct_band(T, band, R)
    dm = _struct.self_costs(mu, r)
    nov = _struct.novelty(dm, T, r, R, _struct.taper(R, sigma))
    o, _, _ = onset(nov)
    A, _, period, info, _ = tempogram(o, Wn, Hw, lo, hi, None, prior)
    P = int(info[0])                                                # the sync
    tracked = None
    if P:
        dlo, dhi, pen = penalty_table(P, tightness)
        tracked = track(o, P, pen, dlo, dhi)
    return Beats(o, A, period, P, (lo, hi), Hw, tracked, R, r, mu, **about)


class BeatTracker:
    """Find the beats of a waveform from its trajectory in a `VAE`'s latent space (see the module doc).  `codec` is the
    FrameCodec that frames and encodes; the model's parameters are read, never written."""

    def __init__(self, model, max_rows=16384, cell_limit=_align.CELL_LIMIT):
        self.codec = c = FrameCodec(model, max_rows)
        self.model, self.device, self.S, self.L = model, c.device, c.S, c.L
        self.cell_limit = int(cell_limit)

    @torch.no_grad()
    def track(self, wave, hop=None, kernel=8, sigma=0.5, lags=(16, 128), window=512, window_hop=None, centre=None,
              octaves=1.0, tightness=100.0, sampling_rate=None):
        """The mu rows of `wave` at `hop`, then track_latents -> Beats with the framing (step, n_samples, sampling_rate)."""
        R = _struct.check_kernel(kernel)
        w = self.codec.wave(wave)
        padded, n_frames = self.codec.pad(w, w.numel(), hop)
        r = _align.check_band(n_frames, n_frames, _struct.pick_band(n_frames, R), self.cell_limit)
        mu, _ = self.codec.encode(padded, n_frames, hop)
        return track_latents(mu, R, sigma, lags, window, window_hop, centre, octaves, tightness, r,
                             step=self.S if hop is None else int(hop), n_samples=w.numel(), sampling_rate=sampling_rate)
