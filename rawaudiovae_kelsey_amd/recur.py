"""What repeats in a recording, in the latent space: the matrix profile of the encoder's mu rows, the motifs, discords
and loop points picked from it, and the looped resynthesis (the RV_RECUR_* ops of rv_mosaic; the rules:
include/rawvae_hip.h, "Latent recurrence"; csrc/recur.hip).

  workspace_bytes(T, N, m, splits)   the bytes of device workspace profile needs (0 with one split)
  profile(dm, m, row0, lo, hi, mirror, ...)   (P [T] fp64, I [T] int32): for every window of m rows of the slab dm the
                                     nearest admitted window of the columns and its window sum
  recurrence(a, b, m, exclude, lo, hi, slab_rows)   the profile of a whole trajectory, slab by slab -> Recurrence
  pick_motifs / pick_discords / pick_best_loop      the host rules on P and I (float64 numpy)
  loop_rows(T, start, end, m, repeats)               the plan of the looped row sequence -> (src, other, g)
  CapturedRecurrence(T, N, L, m, ...)   local_costs + profile of fixed extents captured as one graph
  LatentLooper(model, max_rows)      find(wave, hop, m, min_len, max_len) -> Loop; render(wave, loop, repeats, hop, window)

The admitted windows.  With g the row's frame in the whole recording, window j is admitted iff lo <= j - g <= hi, and with
`mirror` also iff lo <= g - j <= hi.  A self-join with an exclusion zone of e frames is (e, RANGE_MAX, mirror); loop
candidates are (shortest loop, longest loop, no mirror): the window at `end` = I[start] then lies lo..hi frames after the
window at `start`; a join against another recording is the full range.

Nothing here syncs except reading P and I on the host (Recurrence.P, .I and what follows from them).
"""
import numpy as np
import torch

from . import _lib
from . import align as _align
from ._lib import mosaic_call as _call, ptr
from .codec import FrameCodec
from .stream import GraphReplay, window_values

M_MAX = 256                     # the longest window in frames
SPLITS_MAX = 1024
RANGE_MAX = (1 << 31) - 1       # |lo|, |hi| at most
SLAB_ROWS = 4096                # windows per slab of recurrence(): 4096 x N fp32 of distances at a time


def check_m(m):
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= M_MAX:
        raise ValueError("m=%r must be a window of 1 to %d frames" % (m, M_MAX))
    return int(m)


def check_range(lo, hi):
    """(lo, hi) as the library takes them; ValueError naming the argument."""
    for name, v in (("lo", lo), ("hi", hi)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or abs(int(v)) > RANGE_MAX:
            raise ValueError("%s=%r must be a number of frames in [-%d, %d]" % (name, v, RANGE_MAX, RANGE_MAX))
    if lo > hi:
        raise ValueError("lo=%d is above hi=%d" % (lo, hi))
    return int(lo), int(hi)


def check_splits(splits):
    if isinstance(splits, bool) or not isinstance(splits, (int, np.integer)) or not 0 <= splits <= SPLITS_MAX:
        raise ValueError("splits=%r must be in [0, %d] (0: the library's choice)" % (splits, SPLITS_MAX))
    return int(splits)


def workspace_bytes(T, N, m, splits=0):
    """Bytes of device workspace profile needs for T windows against N columns (0 with one split)."""
    return _call(_lib.RECUR_WORKSPACE, T=int(T), N=int(N), k=check_m(m), splits=check_splits(splits)).ws_bytes


def workspace(T, N, m, splits, device):
    return torch.empty(workspace_bytes(T, N, m, splits), dtype=torch.uint8, device=device)


def profile(dm, m, row0=0, lo=-RANGE_MAX, hi=RANGE_MAX, mirror=False, splits=0, ws=None, out=None, stream=None):
    """RV_RECUR_PROFILE over the slab dm [n_rows, N] fp32 (rows of unit stride, any row pitch >= N), whose row r is frame
    row0 + r of the recording -> (P [T] fp64, I [T] int32), T = n_rows - m + 1; out: the two tensors to write into."""
    if not torch.is_tensor(dm) or dm.dim() != 2 or dm.dtype != torch.float32 or dm.device.type != "cuda":
        raise ValueError("dm must be a 2-D float32 device tensor")
    n_rows, N = dm.shape
    if N < 1 or n_rows < 1 or dm.stride(1) != 1 or (n_rows > 1 and dm.stride(0) < N):
        raise ValueError("dm must have rows of unit stride that do not overlap, got shape %s strides %s"
                         % (tuple(dm.shape), tuple(dm.stride())))
    m, splits = check_m(m), check_splits(splits)
    lo, hi = check_range(lo, hi)
    if isinstance(row0, bool) or not isinstance(row0, (int, np.integer)) or not 0 <= row0 <= RANGE_MAX:
        raise ValueError("row0=%r must be a frame index >= 0" % (row0,))
    T = n_rows - m + 1
    if T < 1 or N < m:
        raise ValueError("m=%d: dm %s holds no window of that many frames" % (m, tuple(dm.shape)))
    if ws is None:
        ws = workspace(T, N, m, splits, dm.device)
    if out is None:
        out = (torch.empty(T, dtype=torch.float64, device=dm.device), torch.empty(T, dtype=torch.int32, device=dm.device))
    P, I = out
    _call(_lib.RECUR_PROFILE, stream, local_costs=ptr(dm), stride=dm.stride(0) if n_rows > 1 else N, n_rows=n_rows, N=N, k=m,
          T=T, row0=int(row0), lag=lo, width=hi, mode=_lib.RECUR_MIRROR if mirror else 0, splits=splits,
          ws=ptr(ws) if ws.numel() else None, ws_bytes=ws.numel(), result=ptr(P), idx=ptr(I))
    return P, I


# ---- the host rules on P and I ------------------------------------------------------------------------------------------

def _pick(P, I, exclude, K, sign):
    P, I = np.asarray(P, dtype=np.float64), np.asarray(I, dtype=np.int64)
    if isinstance(exclude, bool) or not isinstance(exclude, (int, np.integer)) or exclude < 0:
        raise ValueError("exclude=%r must be a number of frames >= 0" % (exclude,))
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 0:
        raise ValueError("K=%r must be a count >= 0" % (K,))
    open_ = np.isfinite(P)
    rows = np.arange(P.size)
    found = []
    while len(found) < K and open_.any():
        key = np.where(open_, sign * P, np.inf)
        i = int(np.argmin(key))                 # the first of equal values: ties go to the lower i
        j = int(I[i])
        found.append((i, j, float(P[i])))
        open_ &= (np.abs(rows - i) > exclude) & (np.abs(rows - j) > exclude)
    return found


def pick_motifs(P, I, exclude, K):
    """Up to K motifs [(i, I[i], P[i])], in float64 on the host: repeatedly the least finite P among the rows not yet
    masked (ties: the lower i), after which every row r with |r - i| <= exclude or |r - I[i]| <= exclude is masked."""
    return _pick(P, I, exclude, K, 1.0)


def pick_discords(P, I, exclude, K):
    """pick_motifs with the GREATEST finite P (ties: the lower i) and the same masking."""
    return _pick(P, I, exclude, K, -1.0)


def pick_best_loop(P, I):
    """(start, end, P[start]) = (i, I[i], P[i]) of the least (P, i) over the finite P; None when there is none."""
    found = _pick(P, I, 0, 1, 1.0)
    return found[0] if found else None


def loop_rows(T, start, end, m, repeats):
    """The plan of the looped row sequence of T rows whose window of m rows at `start` recurs at `end`, the stretch
    [start, end) played `repeats` >= 1 times -> (src, other, g): int64, int64 and float32 arrays, one entry per output
    row.  other < 0: the row is row src, copied.  Otherwise it is (1 - g) row src + g row other, mixed by rv_latent_mix
    under RV_ALPHA_F32.  With g_u = fp32((u + 1) / (m + 1)):
      rows 0 .. end - 1;
      for each of the repeats - 1 further passes: m seam rows, seam row u = (1 - g_u) row end + u + g_u row start + u,
        then rows start + m .. end - 1;
      m seam rows again, row u = (1 - g_u) row start + u + g_u row end + u, then rows end + m .. T - 1.
    T + (repeats - 1) (end - start) rows in all.  ValueError unless end + m <= T and end - start >= m."""
    T, start, end, m, repeats = int(T), int(start), int(end), check_m(m), int(repeats)
    if repeats < 1:
        raise ValueError("repeats=%d must be at least 1" % repeats)
    if start < 0 or end + m > T:
        raise ValueError("end=%d: the seam of m=%d rows after it leaves the %d rows (start=%d)" % (end, m, T, start))
    if end - start < m:
        raise ValueError("start=%d and end=%d are closer than the seam of m=%d rows" % (start, end, m))
    u = np.arange(m, dtype=np.int64)
    gu = ((u + 1).astype(np.float64) / (m + 1)).astype(np.float32)

    def plain(a, b):
        r = np.arange(a, b, dtype=np.int64)
        return r, np.full(r.size, -1, np.int64), np.zeros(r.size, np.float32)

    parts = [plain(0, end)]
    for _ in range(repeats - 1):
        parts += [(end + u, start + u, gu), plain(start + m, end)]
    parts += [(start + u, end + u, gu), plain(end + m, T)]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


# ---- the profile of a whole trajectory ----------------------------------------------------------------------------------

class Recurrence:
    """The matrix profile of one trajectory: P [T] fp64 and I [T] int32 on the device, T windows of m frames; they are
    read once, when a host value is asked for.  `exclude` is the radius motifs and discords mask with; `step` the hop
    between frames in samples."""

    def __init__(self, P, I, m, exclude, lo, hi, mirror, step=None, sampling_rate=None):
        self.P_dev, self.I_dev, self.m, self.exclude = P, I, int(m), int(exclude)
        self.lo, self.hi, self.mirror, self.T = lo, hi, bool(mirror), P.numel()
        self.step, self.sampling_rate = step, sampling_rate
        self._host = None

    def _read(self):
        if self._host is None:
            self._host = (self.P_dev.cpu().numpy(), self.I_dev.cpu().numpy().astype(np.int64))     # the one sync
        return self._host

    P = property(lambda self: self._read()[0], doc="[T] float64 on the host")
    I = property(lambda self: self._read()[1], doc="[T] int64 on the host")

    def motifs(self, K=1):
        return pick_motifs(self.P, self.I, self.exclude, K)

    def discords(self, K=1):
        return pick_discords(self.P, self.I, self.exclude, K)

    def best_loop(self):
        if self.mirror:
            raise ValueError("best_loop needs a profile without mirror: its I must lie after its row (lo > 0)")
        return pick_best_loop(self.P, self.I)

    def seconds(self, frame):
        if self.step is None or self.sampling_rate is None:
            raise ValueError("this profile has no framing: it was made from latents, not from a waveform")
        return int(frame) * int(self.step) / float(self.sampling_rate)


def join_range(self_join, m, exclude=None, lo=None, hi=None):
    """(lo, hi, mirror, exclude) of a join: lo / hi given: that range, no mirror; a self-join otherwise: the exclusion zone
    (default m) mirrored; a join against another recording: everything."""
    if (lo is None) != (hi is None):
        raise ValueError("lo=%r and hi=%r: give both or neither" % (lo, hi))
    if exclude is not None and (isinstance(exclude, bool) or not isinstance(exclude, (int, np.integer))
                                or not 0 <= exclude <= RANGE_MAX):
        raise ValueError("exclude=%r must be a number of frames >= 0" % (exclude,))
    if lo is not None:
        return check_range(lo, hi) + (False, m if exclude is None else int(exclude))
    if not self_join:
        return -RANGE_MAX, RANGE_MAX, False, m if exclude is None else int(exclude)
    e = m if exclude is None else int(exclude)
    return e, RANGE_MAX, True, e


def recurrence(a, b=None, m=16, exclude=None, lo=None, hi=None, slab_rows=SLAB_ROWS, splits=0, **about):
    """The matrix profile of the trajectory a [Ta, L] (fp32 device tensor) against b [N, L] (None: against itself) for
    windows of m frames -> Recurrence of Ta - m + 1 windows.  It walks a in slabs of `slab_rows` windows: each slab's
    distances by align.local_costs(a[i0 : i0 + rows + m - 1], b, 0), then profile with row0 = i0, so the memory is
    (slab_rows + m - 1) x N distances, not Ta x N.  The result does not depend on slab_rows."""
    a = _align._rows(a, "a")
    self_join = b is None
    b = a if self_join else _align._rows(b, "b")
    m = check_m(m)
    Ta, N = a.shape[0], b.shape[0]
    if Ta < m or N < m:
        raise ValueError("m=%d: %d and %d frames hold no window of that many" % (m, Ta, N))
    lo, hi, mirror, exclude = join_range(self_join, m, exclude, lo, hi)
    if isinstance(slab_rows, bool) or not isinstance(slab_rows, (int, np.integer)) or slab_rows < 1:
        raise ValueError("slab_rows=%r must be a number of windows >= 1" % (slab_rows,))
    T = Ta - m + 1
    rows_max = min(int(slab_rows), T, _align.CELL_LIMIT // N - (m - 1))
    if rows_max < 1:
        raise ValueError("slab_rows: one window of m=%d rows against %d frames exceeds the limit of %d cells"
                         % (m, N, _align.CELL_LIMIT))
    dev = a.device
    P = torch.empty(T, dtype=torch.float64, device=dev)
    I = torch.empty(T, dtype=torch.int32, device=dev)
    dm = torch.empty((rows_max + m - 1, N), dtype=torch.float32, device=dev)
    ws = workspace(rows_max, N, m, splits, dev)       # the largest slab's: a smaller one needs no more
    for i0 in range(0, T, rows_max):
        rows = min(rows_max, T - i0)
        if workspace_bytes(rows, N, m, splits) > ws.numel():
            ws = workspace(rows, N, m, splits, dev)
        slab = _align.local_costs(a[i0:i0 + rows + m - 1], b, 0, dm[:rows + m - 1])
        profile(slab, m, i0, lo, hi, mirror, splits, ws, (P[i0:i0 + rows], I[i0:i0 + rows]))
    return Recurrence(P, I, m, exclude, lo, hi, mirror, **about)


class CapturedRecurrence(GraphReplay):
    """local_costs and profile of fixed extents captured as one graph: a [T, L] against b [N, L] (self_join: b is a and N
    must be T), windows of m frames.  replay(a, b) copies the trajectories into static buffers and launches it -> the
    Recurrence on static tensors (overwritten by the next replay)."""
    n_streams, block = 1, 1     # GraphReplay's block buffers are not used: the operands have their own static tensors

    def __init__(self, T, N, L, m, exclude=None, lo=None, hi=None, self_join=True, splits=0, device="cuda"):
        self.device = dev = torch.device(device)
        self.T, self.N, self.L, self.m, self.self_join = int(T), int(N), int(L), check_m(m), bool(self_join)
        if self.self_join and self.N != self.T:
            raise ValueError("N=%d: a self-join has N = T = %d" % (self.N, self.T))
        if self.T < self.m or self.N < self.m:
            raise ValueError("m=%d: %d and %d frames hold no window of that many" % (self.m, self.T, self.N))
        self.lo, self.hi, self.mirror, self.exclude = join_range(self.self_join, self.m, exclude, lo, hi)
        self.splits = check_splits(splits)
        _align.check_band(self.T, self.N, 0)
        W = self.T - self.m + 1
        self.a = torch.zeros((self.T, self.L), dtype=torch.float32, device=dev)
        self.b = self.a if self.self_join else torch.zeros((self.N, self.L), dtype=torch.float32, device=dev)
        self.dm = torch.empty((self.T, self.N), dtype=torch.float32, device=dev)
        self.ws = workspace(W, self.N, self.m, self.splits, dev)
        self.out = (torch.empty(W, dtype=torch.float64, device=dev), torch.empty(W, dtype=torch.int32, device=dev))

    def parameters(self):
        return []

    def _launch(self, st):
        _align.local_costs(self.a, self.b, 0, self.dm, st)
        profile(self.dm, self.m, 0, self.lo, self.hi, self.mirror, self.splits, self.ws, self.out, st)

    def capture(self):
        self._launch(None)      # once eagerly, as CapturedSegmentation does: a kernel's first launch stays outside the capture
        return self._capture(self._launch)

    def replay(self, a, b=None, **about):
        self.a.copy_(a)
        if not self.self_join:
            self.b.copy_(b)
        self._replay(0, "replay()")
        return Recurrence(*self.out, self.m, self.exclude, self.lo, self.hi, self.mirror, **about)


# ---- loops of a waveform ------------------------------------------------------------------------------------------------

class Loop:
    """A loop of a recording: the window of m frames at `start_frame` recurs at `end_frame`, `distance` is their window
    sum (0: the same latents); the stretch [start_sample, end_sample) repeats without a seam."""

    def __init__(self, start, end, distance, m, step, sampling_rate=None, recurrence=None):
        self.start_frame, self.end_frame, self.distance, self.m, self.step = int(start), int(end), float(distance), int(m), int(step)
        self.start_sample, self.end_sample = self.start_frame * self.step, self.end_frame * self.step
        self.sampling_rate, self.recurrence = sampling_rate, recurrence
        self.frames, self.samples = self.end_frame - self.start_frame, self.end_sample - self.start_sample

    def _seconds(self, samples):
        if self.sampling_rate is None:
            raise ValueError("this loop has no sampling_rate")
        return samples / float(self.sampling_rate)

    start_seconds = property(lambda self: self._seconds(self.start_sample))
    end_seconds = property(lambda self: self._seconds(self.end_sample))
    seconds = property(lambda self: self._seconds(self.samples))


class LatentLooper:
    """Find where a waveform loops without a seam in a `VAE`'s latent space and render the loop (see the module doc).
    `codec` is the FrameCodec that frames, encodes and decodes; the model's parameters are read, never written."""

    def __init__(self, model, max_rows=16384, slab_rows=SLAB_ROWS):
        self.codec = c = FrameCodec(model, max_rows)
        self.model, self.device, self.S, self.L = model, c.device, c.S, c.L
        self.slab_rows = slab_rows

    def encode(self, wave, hop=None):
        """(mu, logvar, samples) of a waveform at its own length."""
        w = self.codec.wave(wave)
        padded, n_frames = self.codec.pad(w, w.numel(), hop)
        return self.codec.encode(padded, n_frames, hop) + (w.numel(),)

    @torch.no_grad()
    def profile(self, wave, hop=None, m=16, against=None, exclude=None, lo=None, hi=None, sampling_rate=None):
        """recurrence() of the mu rows of `wave` (against those of the waveform `against`, or itself) -> Recurrence."""
        mu, _, _ = self.encode(wave, hop)
        other = None if against is None else self.encode(against, hop)[0]
        return recurrence(mu, other, m, exclude, lo, hi, self.slab_rows, step=self.S if hop is None else int(hop),
                          sampling_rate=sampling_rate)

    @torch.no_grad()
    def find(self, wave, hop=None, m=16, min_len=None, max_len=None, sampling_rate=None):
        """The best loop of min_len .. max_len frames (default: m .. everything): the profile with lo = min_len,
        hi = max_len and no mirror, then the least (P, start) -> Loop, or None when no candidate is finite."""
        m = check_m(m)
        min_len = m if min_len is None else min_len
        max_len = RANGE_MAX if max_len is None else max_len
        lo, hi = check_range(min_len, max_len)
        if lo < m:
            raise ValueError("min_len=%d is shorter than the seam of m=%d frames" % (lo, m))
        rec = self.profile(wave, hop, m, None, None, lo, hi, sampling_rate)
        best = rec.best_loop()
        if best is None:
            return None
        return Loop(best[0], best[1], best[2], m, rec.step, sampling_rate, rec)

    def loop_latents(self, mu, loop, repeats):
        """The rows of loop_rows' plan from mu [T, L]: plain rows copied, seam rows by ONE rv_latent_mix launch
        (RV_ALPHA_F32, eps 0: its mixed mu) -> [rows, L] fp32."""
        from .interpolate import latent_mix
        src, other, g = loop_rows(mu.shape[0], loop.start_frame, loop.end_frame, loop.m, repeats)
        dev = mu.device
        z = mu.index_select(0, torch.from_numpy(src).to(dev))
        seam = np.nonzero(other >= 0)[0]
        ma = mu.index_select(0, torch.from_numpy(src[seam]).to(dev))
        mb = mu.index_select(0, torch.from_numpy(other[seam]).to(dev))
        mixed = latent_mix(ma, ma, mb, mb, g[seam], "f32", eps=torch.zeros_like(ma))["mu"]
        z[torch.from_numpy(seam).to(dev)] = mixed
        return z

    @torch.no_grad()
    def render(self, wave, loop, repeats=2, hop=None, window=None):
        """The waveform with the loop played `repeats` times -> 1-D fp32 of n + (repeats - 1) loop.samples samples:
        FrameCodec.encode, the rows of loop_rows' plan, FrameCodec.decode and the overlap-add at `hop` with `window`.
        Everything before frame loop.start_frame and after the last seam is the plain resynthesis of the input."""
        from .mosaic import check_window, ola
        step = self.S if hop is None else int(hop)
        if step != loop.step:
            raise ValueError("hop: the loop was found at a step of %d samples, not %d" % (loop.step, step))
        check_window(self.S, step, window)
        mu, _, n = self.encode(wave, hop)
        z = self.loop_latents(mu, loop, repeats)
        frames = self.codec.decode(z)
        win = None if window is None else torch.from_numpy(window_values(self.S, window)).to(self.device)
        out = ola(frames, step, (z.shape[0] - 1) * step + self.S, win)
        return out[:n + (int(repeats) - 1) * loop.samples]
