"""Structure of a recording in the latent space: where it changes, and which stretches resemble each other (the
RV_STRUCT_* ops of rv_mosaic; the rules: include/rawvae_hip.h, "Latent structure"; csrc/structure.hip).

  taper(R, sigma)                    the kernel's taper w [2R] float64, on the host (sigma None: all ones)
  self_costs(mu, band)               Dm [T, W] fp32: align.local_costs of a trajectory against itself
  novelty(dm, T, band, R, w)         nov [T] fp64: the checkerboard kernel slid along the diagonal of Dm
  peaks(nov, gap, mean_radius, delta)   (offsets [T + 1] int32, summary [4] int32 = {F, finite entries, 0, 0})
  workspace_bytes(T)                 the bytes of device workspace peaks needs
  pick_band(T, R)                    the narrowest band that holds the kernel, or 0 where the whole matrix is smaller
  segment_latents(mu, ...)           the three launches on a latent trajectory -> Segmentation
  CapturedSegmentation(T, L, R, ...) the same three launches captured as one graph on static buffers
  LatentSegmenter(model, max_rows)   segment(wave, hop, kernel, sigma, gap, mean_radius, delta) -> Segmentation
  labels_from_distances(D, similar)  the form (0 1 0 2 = A B A C) from the segments' self-distance matrix, on the host

Nothing here syncs except reading the number of segments F (Segmentation.F and what follows from it).
"""
import numpy as np
import torch

from . import _lib
from . import align as _align
from ._lib import mosaic_call as _call, ptr
from .codec import FrameCodec
from .stream import GraphReplay

R_MAX = 512
PEAK_MAX = 65536          # the largest gap and mean radius


def check_kernel(R):
    if isinstance(R, bool) or not isinstance(R, (int, np.integer)) or not 1 <= R <= R_MAX:
        raise ValueError("kernel=%r must be a half-width of 1 to %d frames" % (R, R_MAX))
    return int(R)


def check_peaks(gap, mean_radius, delta):
    """(gap, mean_radius, delta) as the library takes them; ValueError naming the argument."""
    for name, v in (("gap", gap), ("mean_radius", mean_radius)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= PEAK_MAX:
            raise ValueError("%s=%r must be a number of frames in [0, %d]" % (name, v, PEAK_MAX))
    d = float(delta)
    if not 0 <= d <= float(np.finfo(np.float32).max):
        raise ValueError("delta=%r must be a finite fp32 number >= 0" % (delta,))
    return int(gap), int(mean_radius), d


def taper(R, sigma=0.5):
    """w [2R] float64: w[n] = exp(-((n - R + 0.5)^2) / (2 (sigma R)^2)); sigma None: ones."""
    R = check_kernel(R)
    if sigma is None:
        return np.ones(2 * R, dtype=np.float64)
    sigma = float(sigma)
    if not 0 < sigma < float("inf"):
        raise ValueError("sigma=%r must be a finite number > 0 or None" % (sigma,))
    n = np.arange(2 * R, dtype=np.float64)
    return np.exp(-((n - R + 0.5) ** 2) / (2.0 * (sigma * R) ** 2))


def pick_band(T, R):
    """2R - 1, the least band that holds the kernel's window, or 0 (the whole matrix) where T rows of T slots are
    fewer than T rows of that band."""
    r = 2 * check_kernel(R) - 1
    return 0 if int(T) < 2 * r + 1 else r


def check_struct_band(T, band, R):
    """`band` (None: pick_band) for a kernel of half-width R; ValueError naming `band`."""
    if band is None:
        band = pick_band(T, R)
    r = _align.check_band(T, T, band)
    if r and r < 2 * R - 1:
        raise ValueError("band=%d does not hold the window of kernel=%d: the least band that does is %d (0: the whole "
                         "matrix)" % (r, R, 2 * R - 1))
    return r


def workspace_bytes(T):
    """Bytes of device workspace peaks needs for T frames."""
    return _call(_lib.STRUCT_WORKSPACE, T=int(T)).ws_bytes


def workspace(T, device):
    return torch.empty(workspace_bytes(T), dtype=torch.uint8, device=device)


def self_costs(mu, band=0, out=None, stream=None):
    """Dm [T, W] fp32 of a trajectory mu [T, L] against itself: RV_ALIGN_COST with a = b."""
    return _align.local_costs(mu, mu, band, out, stream)


def taper_tensor(w, R, device):
    """The taper as the [2R] fp64 device tensor RV_STRUCT_NOVELTY reads."""
    if not torch.is_tensor(w):
        w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float64))
    if w.dtype != torch.float64 or w.dim() != 1 or w.numel() != 2 * R:
        raise ValueError("w must hold 2 R = %d float64 values, got %s %s" % (2 * R, w.dtype, tuple(w.shape)))
    return w.to(device).contiguous()


def novelty(dm, T, band, R, w, out=None, stream=None):
    """RV_STRUCT_NOVELTY over dm [T, W] fp32 -> nov [T] fp64; w: the taper [2R] float64 (numpy or device tensor)."""
    T, R = int(T), check_kernel(R)
    r = check_struct_band(T, band or 0, R)
    w = taper_tensor(w, R, dm.device)
    if out is None:
        out = torch.empty(T, dtype=torch.float64, device=dm.device)
    _call(_lib.STRUCT_NOVELTY, stream, T=T, k=R, band=r, local_costs=ptr(dm), moment=ptr(w), result=ptr(out))
    return out


def peaks(nov, gap, mean_radius, delta, ws=None, out=None, stream=None):
    """RV_STRUCT_PEAKS over nov [T] fp64 -> (offsets [T + 1] int32: 0, the boundaries, T, then -1; summary [4] int32 =
    {F, finite entries, 0, 0}); out: the two tensors to write into."""
    if not torch.is_tensor(nov) or nov.dtype != torch.float64 or nov.dim() != 1 or nov.device.type != "cuda":
        raise ValueError("nov must be a 1-D float64 device tensor")
    gap, mean_radius, delta = check_peaks(gap, mean_radius, delta)
    nov = nov.contiguous()
    T = nov.numel()
    if ws is None:
        ws = workspace(T, nov.device)
    if out is None:
        out = (torch.empty(T + 1, dtype=torch.int32, device=nov.device), torch.empty(4, dtype=torch.int32, device=nov.device))
    path, summary = out
    _call(_lib.STRUCT_PEAKS, stream, T=T, moment=ptr(nov), lag=gap, width=mean_radius, lam=delta, ws=ptr(ws),
          ws_bytes=ws.numel(), path=ptr(path), summary=ptr(summary))
    return path, summary


def labels_from_distances(D, similar=0.5):
    """labels [F] int64 from the segments' self-distance matrix D [F, F], in float64 on the host: label[0] = 0; segment
    f >= 1 takes the label of its nearest earlier segment h (ties: the lower h) when D[f, h] <= similar * the mean of
    D[f, f - 1] over f >= 1, a new label otherwise."""
    D = np.asarray(D, dtype=np.float64)
    F = D.shape[0]
    if D.shape != (F, F) or F < 1:
        raise ValueError("D must be a square matrix of at least one segment, got %s" % (D.shape,))
    labels = np.zeros(F, dtype=np.int64)
    if F == 1:
        return labels
    acc = 0.0
    for f in range(1, F):
        acc = acc + D[f, f - 1]
    limit = float(similar) * (acc / (F - 1))
    fresh = 1
    for f in range(1, F):
        h = int(np.argmin(D[f, :f]))          # the first of equal minima
        if D[f, h] <= limit:
            labels[f] = labels[h]
        else:
            labels[f] = fresh
            fresh += 1
    return labels


def form(labels):
    """'A B A C' of labels [0, 1, 0, 2] (beyond Z: the label's number)."""
    return " ".join(chr(ord("A") + int(v)) if v < 26 else str(int(v)) for v in labels)


class Segmentation:
    """The result of one segmentation; everything stays on the device until a host value (F, offsets, ...) is asked
    for.  `step` is the hop between frames in samples, `n_samples` the length of the sound."""

    def __init__(self, mu, novelty, path, summary, kernel, band, step=None, n_samples=None, sampling_rate=None, similar=0.5):
        self.mu, self.novelty, self.path, self.summary = mu, novelty, path, summary
        self.T, self.kernel, self.band = novelty.numel(), kernel, band
        self.step, self.n_samples, self.sampling_rate, self.similar = step, n_samples, sampling_rate, similar
        self._host = self._parts = None

    def _read(self):
        if self._host is None:
            s = self.summary.cpu().numpy()      # the one sync
            self._host = (int(s[0]), int(s[1]))
        return self._host

    F = property(lambda self: self._read()[0])
    finite = property(lambda self: self._read()[1])

    @property
    def offsets(self):
        """[F + 1] int32 on the device: 0, the boundaries, T."""
        return self.path[:self.F + 1]

    @property
    def boundary_frames(self):
        """The F - 1 boundaries as a numpy int64 array."""
        return self.offsets.cpu().numpy().astype(np.int64)[1:-1]

    @property
    def boundary_samples(self):
        if self.step is None:
            raise ValueError("this segmentation has no framing: it was made from latents, not from a waveform")
        return self.boundary_frames * int(self.step)

    @property
    def boundary_seconds(self):
        if self.sampling_rate is None:
            raise ValueError("this segmentation has no sampling_rate")
        return self.boundary_samples / float(self.sampling_rate)

    @property
    def sample_offsets(self):
        """[F + 1] int64: 0, the boundaries in samples, the length of the sound."""
        return np.concatenate([[0], self.boundary_samples, [int(self.n_samples)]]).astype(np.int64)

    def _structure(self):
        if self._parts is None:
            from .som import segment_mean
            means = segment_mean(self.mu, self.offsets.cpu().numpy())
            dist = self_costs(means, 0)
            self._parts = (means, dist, labels_from_distances(dist.cpu().numpy(), self.similar))
        return self._parts

    means = property(lambda self: self._structure()[0], doc="[F, L] fp32: rv_segment_mean of mu on the offsets")
    distances = property(lambda self: self._structure()[1], doc="[F, F] fp32: self_costs(means, 0)")
    labels = property(lambda self: self._structure()[2], doc="[F] int64 on the host: labels_from_distances")
    form = property(lambda self: form(self.labels))


def segment_latents(mu, kernel=32, sigma=0.5, gap=16, mean_radius=None, delta=0.5, band=None, **about):
    """Novelty and boundaries of a latent trajectory mu [T, L] (fp32 device tensor) -> Segmentation.  Three library
    calls: self_costs, novelty, peaks.  mean_radius None: two kernels."""
    mu = _align._rows(mu, "mu")
    T, R = mu.shape[0], check_kernel(kernel)
    mean_radius = min(2 * R, PEAK_MAX) if mean_radius is None else mean_radius
    check_peaks(gap, mean_radius, delta)
    r = check_struct_band(T, band, R)
    dm = self_costs(mu, r)
    nov = novelty(dm, T, r, R, taper(R, sigma))
    path, summary = peaks(nov, gap, mean_radius, delta)
    return Segmentation(mu, nov, path, summary, R, r, **about)


class CapturedSegmentation(GraphReplay):
    """self_costs, novelty and peaks of fixed extents captured as one graph: replay(mu) copies the trajectory into a
    static buffer and launches it -> the Segmentation on static tensors (overwritten by the next replay)."""
    n_streams, block = 1, 1     # GraphReplay's block buffers are not used: the operands have their own static tensors

    def __init__(self, T, L, R, sigma=0.5, gap=16, mean_radius=None, delta=0.5, band=None, device="cuda"):
        self.device = dev = torch.device(device)
        self.T, self.L, self.R = int(T), int(L), check_kernel(R)
        mean_radius = min(2 * self.R, PEAK_MAX) if mean_radius is None else mean_radius
        self.gap, self.mean_radius, self.delta = check_peaks(gap, mean_radius, delta)
        self.r = check_struct_band(self.T, band, self.R)
        self.mu = torch.zeros((self.T, self.L), dtype=torch.float32, device=dev)
        self.dm = torch.empty((self.T, _align.band_slots(self.T, self.r)), dtype=torch.float32, device=dev)
        self.w = taper_tensor(taper(self.R, sigma), self.R, dev)
        self.nov = torch.empty(self.T, dtype=torch.float64, device=dev)
        self.ws = workspace(self.T, dev)
        self.out = (torch.empty(self.T + 1, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev))

    def parameters(self):
        return []

    def _launch(self, st):
        self_costs(self.mu, self.r, self.dm, st)
        novelty(self.dm, self.T, self.r, self.R, self.w, self.nov, st)
        peaks(self.nov, self.gap, self.mean_radius, self.delta, self.ws, self.out, st)

    def capture(self):
        self._launch(None)      # once eagerly: a kernel's first launch on a device sets its LDS attribute, outside the capture
        return self._capture(self._launch)

    def replay(self, mu, **about):
        self.mu.copy_(mu)
        self._replay(0, "replay()")
        return Segmentation(self.mu, self.nov, *self.out, self.R, self.r, **about)


class LatentSegmenter:
    """Cut a waveform where its trajectory in a `VAE`'s latent space changes (see the module doc).  `codec` is the
    FrameCodec that frames and encodes; the model's parameters are read, never written."""

    def __init__(self, model, max_rows=16384, cell_limit=_align.CELL_LIMIT):
        self.codec = c = FrameCodec(model, max_rows)
        self.model, self.device, self.S, self.L = model, c.device, c.S, c.L
        self.cell_limit = int(cell_limit)

    @torch.no_grad()
    def segment(self, wave, hop=None, kernel=32, sigma=0.5, gap=16, mean_radius=None, delta=0.5, similar=0.5,
                sampling_rate=None):
        """The mu rows of `wave` at `hop`, their novelty under a kernel of half-width `kernel` frames and the
        boundaries picked from it -> Segmentation."""
        R = check_kernel(kernel)
        w = self.codec.wave(wave)
        padded, n_frames = self.codec.pad(w, w.numel(), hop)
        r = _align.check_band(n_frames, n_frames, pick_band(n_frames, R), self.cell_limit)
        mu, _ = self.codec.encode(padded, n_frames, hop)
        return segment_latents(mu, R, sigma, gap, mean_radius, delta, r, step=self.S if hop is None else int(hop),
                               n_samples=w.numel(), sampling_rate=sampling_rate, similar=similar)
