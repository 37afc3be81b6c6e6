"""Held-out evaluation on the device: how well a model reconstructs audio it did not train on, and how close one
waveform is to another.

  frame_scores(ref, test, T, S, hop, stride, ...)   RV_EVAL_FRAMES: [T, 6] fp32 scores of T frame pairs, the columns
                                        COLUMNS = sse, energy, kl, lsd, spec_err, spec_ref (include/rawvae_hip.h)
  kl_dims(mu, logvar)                   RV_EVAL_DIMS: [L] fp64 KL sums per latent dimension
  ev = Evaluator(model, hop=None, window="hann", dynamic_range=60.0, max_rows=16384)
  ev.score(wave, eps=None, seed=None)   frames the waveform as TestDataset does (hop=None: non-overlapping, the tail
                                        zero-padded) or as AudioDataset does at `hop`, runs the exact-fp32 inference
                                        path (VAE.encode / decode under no_grad: rv_linear_fp32) in chunks of max_rows
                                        frames and scores every frame against its reconstruction.  z = mu (default,
                                        deterministic), mu + eps * exp(logvar / 2) with an explicit eps [T, L], or the
                                        on-device draw from `seed`.  -> (scores [T, 6] fp32, kl sums [L] fp64), on the
                                        device, nothing read back.
  ev.add(wave, name); ev.report(kl_beta)
                                        scores files one by one, then the whole-set and per-file figures as a dict:
                                        frames, mse = sum sse / (T S), kld = sum kl / (T L), loss = mse + kl_beta * kld
                                        (the reference's loss_function on the whole set as one batch), snr_db =
                                        10 log10(sum energy / sum sse), lsd_db = the mean over frames,
                                        spectral_convergence = sqrt(sum spec_err / sum spec_ref), kl_per_dim (mean KL
                                        of each dimension over the frames) and active_units (dimensions whose mean KL
                                        exceeds active_threshold).  The means are rv_segment_mean's (fp64, ascending
                                        rows, rounded once).
  compare(ref_wave, test_wave, segment_length, hop, ...)
                                        model-free: the same figures (without the KL ones) of two waveforms framed at
                                        `hop`, the shorter one zero-padded: what scores a mosaic or a resynthesis
                                        against its target.
  check_args(...)                       the argument rules without a device; ValueError naming the argument.

Every row's scores depend on that row alone, so the result is bit-identical for any max_rows.  Framing, encoder and
decoder are codec.FrameCodec's (`ev.codec`).
"""
import numpy as np
import torch

from . import _lib
from ._lib import lib, mosaic_call, ptr, stream_ptr
from .codec import MAX_GEMM_ROWS, FrameCodec, frame_layout
from .som import segment_mean
from .stream import WINDOWS, window_values

COLUMNS = ("sse", "energy", "kl", "lsd", "spec_err", "spec_ref")
SPECTRAL_S = (32, 4096)      # frame lengths (powers of two) the spectral columns take (csrc/eval.hip)
DIMS_ROWS = 256              # rows of one summation block of kl_dims (the header fixes it)
R_MAX = 120.0


def twiddle_table(segment_length):
    """The table RV_EVAL_FRAMES reads: [S] fp32, (cos, -sin)(2 pi j / S) for j < S / 2, float64 rounded once."""
    S = int(segment_length)
    a = 2.0 * np.pi * np.arange(S // 2, dtype=np.float64) / S
    t = np.empty(S, dtype=np.float64)
    t[0::2], t[1::2] = np.cos(a), -np.sin(a)
    return t.astype(np.float32)


def _spectral_ok(S):
    return SPECTRAL_S[0] <= S <= SPECTRAL_S[1] and S & (S - 1) == 0


def check_args(segment_length, hop=None, window="hann", dynamic_range=60.0, max_rows=16384, active_threshold=0.01):
    """Validate an evaluation's arguments without a device -> (frame step, dynamic range).  ValueError naming the
    argument."""
    try:
        S = int(segment_length)
    except (TypeError, ValueError):
        S = 0
    if S < 1:
        raise ValueError("segment_length=%r must be a positive integer" % (segment_length,))
    step = S
    if hop is not None:
        if isinstance(hop, bool) or not isinstance(hop, (int, np.integer)) or int(hop) < 1 or S % int(hop) != 0:
            raise ValueError("hop=%r must be a positive integer that divides segment_length %d" % (hop, S))
        step = int(hop)
    if window not in WINDOWS:
        raise ValueError("window %r: expected None (no spectral figures) or 'hann'" % (window,))
    if window is not None and not _spectral_ok(S):
        raise ValueError("window %r: the spectral figures need segment_length a power of two in [%d, %d], got %d "
                         "(window=None scores without them)" % (window, SPECTRAL_S[0], SPECTRAL_S[1], S))
    try:
        R = float(dynamic_range)
    except (TypeError, ValueError):
        R = float("nan")
    if not 0 < R <= R_MAX:
        raise ValueError("dynamic_range=%r must be a number of dB in (0, %g]" % (dynamic_range, R_MAX))
    if isinstance(max_rows, bool) or not isinstance(max_rows, (int, np.integer)) or not 1 <= int(max_rows) <= MAX_GEMM_ROWS:
        raise ValueError("max_rows=%r must be an integer in [1, %d]" % (max_rows, MAX_GEMM_ROWS))
    try:
        thr = float(active_threshold)
    except (TypeError, ValueError):
        thr = float("nan")
    if not 0 <= thr < float("inf"):
        raise ValueError("active_threshold=%r must be a finite number >= 0" % (active_threshold,))
    return step, R


def _flat(x, what, device=None):
    if (not torch.is_tensor(x) or x.dtype != torch.float32 or x.device.type != "cuda" or not x.is_contiguous()
            or (device is not None and x.device != device)):
        raise ValueError("%s must be a contiguous float32 device tensor%s" % (
            what, "" if device is None else " on %s" % device))
    return x.view(-1)


def frame_scores(ref, test, T, segment_length, hop, stride, mu=None, logvar=None, window=None, table=None,
                 dynamic_range=60.0, out=None):
    """[T, 6] fp32 (COLUMNS) of the frame pairs x = ref[t * hop : + S], y = test[t * stride : + S] (RV_EVAL_FRAMES; the
    arithmetic: include/rawvae_hip.h).  ref / test: contiguous fp32 device tensors read flat; mu / logvar [T, L] or
    both None (kl = 0); window [S] with its twiddle `table` [S] (twiddle_table) or None (columns 3..5 = 0).  `out`: a
    [T, ldo >= 6] fp32 tensor (or a row slice of one) to write into; only its columns 0..5 are written."""
    ref = _flat(ref, "ref")
    test = _flat(test, "test", ref.device)
    T, S = int(T), int(segment_length)
    L = 0
    if mu is not None or logvar is not None:
        if mu is None or logvar is None or mu.shape != logvar.shape or mu.dim() != 2 or mu.shape[0] != T:
            raise ValueError("mu and logvar must both be [%d, L] tensors" % T)
        mu, logvar = _flat(mu, "mu", ref.device), _flat(logvar, "logvar", ref.device)
        L = mu.numel() // T
    if window is not None:
        window = _flat(window, "window", ref.device)
        if table is None or window.numel() != S:
            raise ValueError("window must hold %d values and come with its twiddle table" % S)
        table = _flat(table, "table", ref.device)
        if table.numel() != S:
            raise ValueError("table must hold %d values (twiddle_table), got %d" % (S, table.numel()))
    if out is None:
        out = torch.empty((T, 6), dtype=torch.float32, device=ref.device)
    if (not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != ref.device or out.dim() != 2
            or out.shape[0] != T or out.shape[1] < 6 or out.stride(1) != 1):
        raise ValueError("out must be a [%d, >= 6] float32 tensor on %s with unit column stride" % (T, ref.device))
    mosaic_call(_lib.EVAL_FRAMES, T=T, S=S, hop=int(hop), frames=ptr(ref), n_out=ref.numel(), src=ptr(test),
                stride=int(stride), src_len=test.numel(), L=L, window=ptr(window), out=ptr(out),
                ldo=out.stride(0) if T > 1 else max(out.shape[1], 6), mu=ptr(mu), logvar=ptr(logvar), twiddles=ptr(table),
                dynamic_range=float(dynamic_range))
    return out


def kl_dims(mu, logvar):
    """[L] fp64: sum_t -0.5 (1 + logvar - mu^2 - exp(logvar)) of every latent dimension (RV_EVAL_DIMS): rows in blocks
    of DIMS_ROWS, each block in ascending t, the blocks in ascending order; bit-identical from run to run."""
    if not torch.is_tensor(mu) or mu.dim() != 2 or not torch.is_tensor(logvar) or logvar.shape != mu.shape:
        raise ValueError("mu and logvar must be [T, L] tensors of one shape")
    T, L = mu.shape
    mu = _flat(mu, "mu")
    logvar = _flat(logvar, "logvar", mu.device)
    cost = torch.empty(L, dtype=torch.float64, device=mu.device)
    nb = -(-T // DIMS_ROWS)
    nbytes = 8 * nb * L if nb > 1 else 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=mu.device) if nbytes else None
    mosaic_call(_lib.EVAL_DIMS, T=T, L=L, cost=ptr(cost), ws=ptr(ws), ws_bytes=nbytes, mu=ptr(mu), logvar=ptr(logvar))
    return cost


def _figures(mean, T, S, L, kl_beta, kl_dim, threshold):
    """The figures from the fp64 means of the six columns over T frames."""
    sse, energy, kl, lsd, serr, sref = (float(v) for v in mean)
    with np.errstate(all="ignore"):
        snr = float(10.0 * np.log10(np.float64(energy) / np.float64(sse))) if sse > 0 else (
            float("inf") if energy > 0 else float("nan"))
        out = {"frames": int(T), "mse": sse / S, "snr_db": snr, "lsd_db": lsd,
               "spectral_convergence": float(np.sqrt(serr / sref)) if sref > 0 else 0.0}
    if L:
        out["kld"] = kl / L
        out["loss"] = out["mse"] + float(kl_beta) * out["kld"]
    if kl_dim is not None:
        per = np.asarray(kl_dim, dtype=np.float64) / T
        out["kl_per_dim"] = per.tolist()
        out["active_units"] = int((per > threshold).sum())
    return out


class _Spectral:
    """The window and its table on a device (None, None without a window)."""

    def __init__(self, S, window, device):
        self.window = self.table = None
        if window is not None:
            self.window = torch.from_numpy(window_values(S, window)).to(device)
            self.table = torch.from_numpy(twiddle_table(S)).to(device)


class Evaluator:
    """Scores a `rawvae.model.VAE` on the GPU against waveforms (see the module doc).  The model's parameters are read
    in place on every call and never written; `_rng_calls` stays as it was."""

    def __init__(self, model, hop=None, window="hann", dynamic_range=60.0, max_rows=16384, active_threshold=0.01):
        from .model import VAE
        if not isinstance(model, VAE):
            raise TypeError("Evaluator needs a rawvae.model.VAE (the one-hidden-layer model), got %s"
                            % type(model).__name__)
        self.step, self.dynamic_range = check_args(model.segment_length, hop, window, dynamic_range, max_rows,
                                                   active_threshold)
        self.codec = c = FrameCodec(model, max_rows=int(max_rows))   # RvError for a model that is not on the GPU
        self.model, self.max_rows, self.device = model, c.max_rows, c.device
        self.S, self.H, self.L = c.S, c.H, c.L
        self.hop = None if hop is None else int(hop)
        self.window, self.active_threshold = window, float(active_threshold)
        self._spec = _Spectral(self.S, window, self.device)
        self.reset()

    def reset(self):
        """Forget the files added so far."""
        self.names, self._scores, self._kl = [], [], []

    @torch.no_grad()
    def score(self, wave, eps=None, seed=None):
        """(scores [T, 6] fp32, kl sums [L] fp64) of one waveform, device tensors (see the module doc)."""
        if eps is not None and seed is not None:
            raise ValueError("eps and seed: give at most one of them")
        w = self.codec.wave(wave)
        padded, T = self.codec.pad(w, w.numel(), self.hop)
        mu, lv = self.codec.encode(padded, T, self.hop)
        if eps is None and seed is None:
            z = mu
        else:
            z = torch.empty_like(mu)
            if eps is not None:
                if not torch.is_tensor(eps):
                    eps = torch.from_numpy(np.ascontiguousarray(eps, dtype=np.float32))
                eps = eps.to(device=self.device, dtype=torch.float32).contiguous()
                if tuple(eps.shape) != (T, self.L):
                    raise ValueError("eps has shape %s, expected [%d, %d]" % (tuple(eps.shape), T, self.L))
                lib().rv_reparameterize(ptr(mu), ptr(lv), mu.numel(), ptr(eps), None, 0, 0, ptr(z), stream_ptr())
            else:
                drawn = torch.empty_like(mu)
                lib().rv_reparameterize(ptr(mu), ptr(lv), mu.numel(), None, ptr(drawn), int(seed), 0, ptr(z),
                                        stream_ptr())
        scores = torch.empty((T, 6), dtype=torch.float32, device=self.device)
        h = self.codec.hidden(T)
        recon = torch.empty((min(self.max_rows, T), self.S), dtype=torch.float32, device=self.device)
        for r0, rows in self.codec.chunks(T):
            self.codec.decode_chunk(z[r0:r0 + rows], h, recon)
            frame_scores(padded[r0 * self.step:], recon[:rows], rows, self.S, self.step, self.S, mu[r0:r0 + rows],
                         lv[r0:r0 + rows], self._spec.window, self._spec.table, self.dynamic_range,
                         out=scores[r0:r0 + rows])
        return scores, kl_dims(mu, lv)

    def add(self, wave, name, eps=None, seed=None):
        """Score one file and keep its rows for report().  ValueError naming `name` when it makes no frame."""
        try:
            scores, kl = self.score(wave, eps, seed)
        except ValueError as e:
            raise ValueError("%s: %s" % (name, e))
        self.names.append(str(name))
        self._scores.append(scores)
        self._kl.append(kl)
        return scores.shape[0]

    @property
    def scores(self):
        """[sum of frames, 6] fp32: the score matrix of every file added, in order."""
        if not self._scores:
            raise ValueError("nothing to report: add() files first")
        return torch.cat(self._scores) if len(self._scores) > 1 else self._scores[0]

    @property
    def offsets(self):
        """[files + 1] int64 (numpy): file f's rows of `scores` are [offsets[f], offsets[f + 1])."""
        return np.concatenate([[0], np.cumsum([s.shape[0] for s in self._scores])]).astype(np.int64)

    def report(self, kl_beta, active_threshold=None):
        """The whole-set figures and, under "files", every file's (see the module doc)."""
        thr = self.active_threshold
        if active_threshold is not None:
            check_args(self.S, self.hop, self.window, self.dynamic_range, self.max_rows, active_threshold)
            thr = float(active_threshold)
        allrows, off = self.scores, self.offsets
        whole = segment_mean(allrows, [0, int(off[-1])]).double().cpu().numpy()[0]
        per = segment_mean(allrows, off).double().cpu().numpy()
        kls = torch.stack(self._kl).cpu().numpy()
        out = _figures(whole, int(off[-1]), self.S, self.L, kl_beta, kls.sum(axis=0), thr)
        out["kl_beta"] = float(kl_beta)
        out["files"] = [dict(_figures(per[f], int(off[f + 1] - off[f]), self.S, self.L, kl_beta, kls[f], thr), name=n)
                        for f, n in enumerate(self.names)]
        return out


@torch.no_grad()
def compare(ref_wave, test_wave, segment_length, hop=None, window="hann", dynamic_range=60.0, device=None,
            return_scores=False):
    """Figures of `test_wave` against `ref_wave` without a model: both framed at `hop` (None: segment_length) after
    the shorter one is zero-padded to the longer one's length -> dict with frames, mse, snr_db, lsd_db and
    spectral_convergence; with return_scores also the [T, 6] device tensor."""
    step, R = check_args(segment_length, hop, window, dynamic_range)
    S = int(segment_length)
    waves = []
    for what, w in (("ref_wave", ref_wave), ("test_wave", test_wave)):
        if isinstance(w, np.ndarray):
            w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
        if not torch.is_tensor(w) or w.dim() != 1 or w.numel() == 0:
            raise ValueError("%s must be a non-empty 1-D tensor or numpy array" % what)
        if device is None and w.device.type == "cuda":
            device = w.device
        waves.append(w)
    device = torch.device("cuda") if device is None else torch.device(device)
    n = max(w.numel() for w in waves)
    T, total = frame_layout(n, S, None if hop is None else step)
    if T < 1:
        raise ValueError("%d samples make no frame of %d samples at hop %s" % (n, S, hop))
    padded = []
    for w in waves:
        w = w.to(device=device, dtype=torch.float32).contiguous()
        dst = torch.empty(total, dtype=torch.float32, device=device)
        lib().rv_match_pad(ptr(w), w.numel(), w.numel(), ptr(dst), total, stream_ptr())   # w, then zeros
        padded.append(dst)
    spec = _Spectral(S, window, device)
    scores = frame_scores(padded[0], padded[1], T, S, step, step, window=spec.window, table=spec.table, dynamic_range=R)
    mean = segment_mean(scores, [0, T]).double().cpu().numpy()[0]
    out = _figures(mean, T, S, 0, 0.0, None, 0.0)
    return (out, scores) if return_scores else out
