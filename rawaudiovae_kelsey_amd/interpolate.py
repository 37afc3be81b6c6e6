"""Latent interpolation and resynthesis of whole waveforms: the reference's `tutorial.ipynb` workflow on the device.

The notebook encodes two sounds, mixes their latent distributions and decodes the mix back into audio, in three
variants (tutorial.ipynb:456-530 stepwise, 834-925 meso-scale curve, 1200-1279 the curve "with extensions" at
hop_length 128).  Here each variant is a handful of launches per chunk of frames on the caller's current stream:

  rv_match_pad    repeat-the-shorter / crop and the framing's zero padding, straight into a device waveform
  rv_linear_fp32  fc1 reading its frames from that waveform through the leading dimension (ldx = hop), then fc21, fc22
  rv_latent_mix   the mix of (mu, logvar) and the reparameterisation, alpha from a list, a per-frame array or a curve
                  stretched in the kernel (scipy.interpolate.interp1d at numpy.linspace)
  rv_linear_fp32  fc3, then fc4 + tanh written into the output waveform's slice

Arithmetic follows torch's promotion in the notebook: scalar or fp32 alpha -> fp32 throughout; fp64 alpha or curve
-> fp64 mix and reparameterisation, z rounded once to fp32 (the notebook's `.float()` before `decode`).  The GEMMs are
the exact-fp32 inference kernels of `VAE.encode` / `VAE.decode` under `torch.no_grad()`.

Memory: mu / logvar of both sources are kept whole ([N, L] fp32 each); per chunk of at most `max_rows` frames one
h [rows, H] and one z [rows, L] buffer.  Every row's arithmetic is independent of the chunking, so the output is
bit-identical for any `max_rows`.
"""
import numpy as np
import torch

from . import _lib
from ._lib import ACT_NONE, ACT_RELU, ACT_TANH, ALPHA_CURVE, ALPHA_F32, ALPHA_F64, ALPHA_LIST, lib, ptr, stream_ptr

MAX_GEMM_ROWS = 65535 * 64    # rv_linear_fp32's launch grid


def matched_length(n_a, n_b, mode="repeat"):
    """Length both sources have after the notebook's match_audio_size (tutorial.ipynb:423-437): "repeat" repeats the
    shorter one up to the longer one's length, "crop" cuts the longer one to the shorter one's."""
    if mode == "repeat":
        return max(int(n_a), int(n_b))
    if mode == "crop":
        return min(int(n_a), int(n_b))
    raise ValueError("match mode %r: expected 'repeat' or 'crop'" % (mode,))


def frame_layout(n_samples, segment_length, hop=None):
    """(frames, padded length) of a waveform of n_samples.  hop=None: TestDataset (non-overlapping frames, the tail
    zero-padded to a whole frame, dataset.py:141-160); an int: AudioDataset (padded to a multiple of hop, frame i starts
    at i * hop, dataset.py:99-121, ValueError when segment_length is not a multiple of hop)."""
    S = int(segment_length)
    n = int(n_samples)
    if hop is None:
        padded = -(-n // S) * S
        return padded // S, padded
    hop = int(hop)
    if hop <= 0:
        raise ValueError("hop must be positive, got %d" % hop)
    if S % hop != 0:
        raise ValueError("segment_length {} is not a multiple of hop_size {}".format(S, hop))
    padded = -(-n // hop) * hop
    return padded // hop - S // hop + 1, padded


class LatentInterpolator:
    """Encode two sounds, mix their latent distributions, decode the mix into one waveform (see the module doc).

    `model` is a `VAE` on the GPU; its parameters are read, never written (the model's parameters, `_rng_calls` and
    operand shadows stay as they were).  eps is either given ([rows, L] fp32, rows = the output frames) or drawn on
    the device from `seed` with the Philox stream of `VAE.reparameterize` (offset 0)."""

    def __init__(self, model, max_rows=16384):
        max_rows = int(max_rows)
        if not 1 <= max_rows <= MAX_GEMM_ROWS:
            raise ValueError("max_rows must be in [1, %d], got %d" % (MAX_GEMM_ROWS, max_rows))
        self.model = model
        self.max_rows = max_rows
        self.S, self.H, self.L = int(model.segment_length), int(model.n_units), int(model.latent_dim)
        self.device = model.fc1.weight.device
        if self.device.type != "cuda":
            raise _lib.RvError("LatentInterpolator computes on the GPU only: the model is on %s" % self.device)

    # -- helpers ---------------------------------------------------------------------------------------------------
    def _w(self, name):
        t = getattr(self.model, name)
        return t.weight.detach().contiguous(), t.bias.detach().contiguous()

    def _wave(self, w):
        """1-D fp32 device tensor of a waveform given as a device tensor or a numpy array."""
        if isinstance(w, np.ndarray):
            w = torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32))
        if not torch.is_tensor(w):
            raise TypeError("waveform must be a torch tensor or a numpy array, got %s" % type(w).__name__)
        if w.dim() != 1:
            raise ValueError("waveform must be 1-D, got shape %s" % (tuple(w.shape),))
        if w.numel() == 0:
            raise ValueError("empty waveform")
        return w.to(device=self.device, dtype=torch.float32).contiguous()

    def _padded(self, w, n_valid, hop):
        """rv_match_pad: w repeated or cropped to n_valid samples, zeros up to the framing's padded length."""
        n_frames, padded = frame_layout(n_valid, self.S, hop)
        if n_frames < 1:
            raise ValueError("%d samples make no frame of %d samples at hop %s" % (n_valid, self.S, hop))
        dst = torch.empty(padded, dtype=torch.float32, device=self.device)
        lib().rv_match_pad(ptr(w), w.numel(), n_valid, ptr(dst), padded, stream_ptr())
        return dst, n_frames

    def _linear(self, x, ldx, rows, name, act, y, ldy):
        W, b = self._w(name)
        N, K = W.shape
        lib().rv_linear_fp32(x, ldx, ptr(W), K, ptr(b), rows, N, K, act, y, ldy, stream_ptr())

    def _encode_padded(self, wave, n_frames, hop):
        """fc1 -> (fc21, fc22) over the frames of a padded waveform, max_rows frames at a time."""
        step = self.S if hop is None else int(hop)
        mu = torch.empty((n_frames, self.L), dtype=torch.float32, device=self.device)
        lv = torch.empty_like(mu)
        h = torch.empty((min(self.max_rows, n_frames), self.H), dtype=torch.float32, device=self.device)
        for f0 in range(0, n_frames, self.max_rows):
            rows = min(self.max_rows, n_frames - f0)
            self._linear(wave.data_ptr() + 4 * f0 * step, step, rows, "fc1", ACT_RELU, ptr(h), self.H)
            self._linear(ptr(h), self.H, rows, "fc21", ACT_NONE, ptr(mu) + 4 * f0 * self.L, self.L)
            self._linear(ptr(h), self.H, rows, "fc22", ACT_NONE, ptr(lv) + 4 * f0 * self.L, self.L)
        return mu, lv

    def _mix_decode(self, dists, n_frames, mode, alpha, n_alpha, rows_total, eps, seed):
        mu_a, lv_a, mu_b, lv_b = dists
        if eps is not None:
            eps = eps.to(device=self.device, dtype=torch.float32).contiguous()
            if eps.numel() != rows_total * self.L:
                raise ValueError("eps has %d elements, expected [%d, %d]" % (eps.numel(), rows_total, self.L))
        out = torch.empty(rows_total * self.S, dtype=torch.float32, device=self.device)
        cap = min(self.max_rows, rows_total)
        z = torch.empty((cap, self.L), dtype=torch.float32, device=self.device)
        h = torch.empty((cap, self.H), dtype=torch.float32, device=self.device)
        for r0 in range(0, rows_total, self.max_rows):
            rows = min(self.max_rows, rows_total - r0)
            e = None if eps is None else eps.data_ptr() + 4 * r0 * self.L
            lib().rv_latent_mix(ptr(mu_a), ptr(lv_a), ptr(mu_b), ptr(lv_b), n_frames, self.L, mode, ptr(alpha), n_alpha,
                                r0, rows, e, None, int(seed), 0, ptr(z), None, None, None, stream_ptr())
            self._linear(ptr(z), self.L, rows, "fc3", ACT_RELU, ptr(h), self.H)
            self._linear(ptr(h), self.H, rows, "fc4", ACT_TANH, out.data_ptr() + 4 * r0 * self.S, self.S)
        return out

    def _sources(self, a, b, hop, match):
        a, b = self._wave(a), self._wave(b)
        n = matched_length(a.numel(), b.numel(), match)
        (pa, n_frames), (pb, _) = self._padded(a, n, hop), self._padded(b, n, hop)
        return self._encode_padded(pa, n_frames, hop) + self._encode_padded(pb, n_frames, hop), n_frames

    # -- public surface --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_audio(self, wave, hop=None):
        """(mu, logvar) [frames, L] of a waveform framed like TestDataset (hop=None) or AudioDataset (hop=int):
        the notebook's raw_to_z_dist (tutorial.ipynb:456-470) in exact fp32."""
        w = self._wave(wave)
        padded, n_frames = self._padded(w, w.numel(), hop)
        return self._encode_padded(padded, n_frames, hop)

    @torch.no_grad()
    def match_length(self, a, b, mode="repeat"):
        """Both waveforms at matched_length(len(a), len(b), mode), as device tensors (rv_match_pad)."""
        a, b = self._wave(a), self._wave(b)
        n = matched_length(a.numel(), b.numel(), mode)
        out = []
        for w in (a, b):
            d = torch.empty(n, dtype=torch.float32, device=self.device)
            lib().rv_match_pad(ptr(w), w.numel(), n, ptr(d), n, stream_ptr())
            out.append(d)
        return tuple(out)

    @torch.no_grad()
    def stepwise(self, a, b, alphas, hop=None, eps=None, seed=0, match="repeat"):
        """The stepwise interpolation (tutorial.ipynb:496-530): for each alpha in `alphas` every frame of the mix
        mu_a (1 - alpha) + mu_b alpha (logvar likewise) is reparameterised and decoded; the K blocks of N frames are
        concatenated in the order of `alphas` -> 1-D fp32 waveform of K * N * segment_length samples.  fp32 arithmetic
        (alpha a float64 scalar, as the notebook's numpy values are).  eps: [K * N, L] fp32 or None (Philox, `seed`)."""
        al = np.asarray(alphas, dtype=np.float64).reshape(-1)
        if al.size == 0:
            raise ValueError("alphas is empty")
        dists, n_frames = self._sources(a, b, hop, match)
        alpha = torch.from_numpy(al).to(self.device)
        return self._mix_decode(dists, n_frames, ALPHA_LIST, alpha, al.size, al.size * n_frames, eps, seed)

    @torch.no_grad()
    def curve(self, a, b, curve_or_alpha, hop=None, eps=None, seed=0, match="repeat", stretch=None):
        """The meso-scale interpolation (tutorial.ipynb:905-925; with hop=128 the "with extensions" variant): frame n
        of the output decodes the mix at its own alpha_n -> 1-D fp32 waveform of N * segment_length samples.

        `curve_or_alpha` (numpy array or tensor):
          * float64 and stretch in (None, True): a control curve of C >= 2 points stretched to the N frames as
            interp1d(arange(C), curve)(linspace(0, C - 1, N)); fp64 mix and reparameterisation;
          * float64 and stretch=False: one alpha per frame ([N]), fp64 arithmetic;
          * float32 ([N], stretch None or False): one alpha per frame, fp32 arithmetic.
        eps: [N, L] fp32 or None (Philox, `seed`)."""
        c = curve_or_alpha
        if torch.is_tensor(c):
            c = c.detach().cpu().numpy()
        c = np.asarray(c)
        if c.dtype not in (np.float32, np.float64) or c.ndim != 1:
            raise ValueError("curve / alpha must be a 1-D float32 or float64 array, got %s %s" % (c.dtype, c.shape))
        if stretch is None:
            stretch = c.dtype == np.float64
        if stretch and c.dtype != np.float64:
            raise ValueError("a curve to stretch must be float64 (the notebook's numpy curve)")
        dists, n_frames = self._sources(a, b, hop, match)
        if stretch:
            if c.size < 2:
                raise ValueError("a curve needs at least 2 points, got %d" % c.size)
            mode = ALPHA_CURVE
        else:
            if c.size != n_frames:
                raise ValueError("%d per-frame alpha values for %d frames" % (c.size, n_frames))
            mode = ALPHA_F64 if c.dtype == np.float64 else ALPHA_F32
        alpha = torch.from_numpy(np.ascontiguousarray(c)).to(self.device)
        return self._mix_decode(dists, n_frames, mode, alpha, c.size, n_frames, eps, seed)


def latent_mix(mu_a, lv_a, mu_b, lv_b, alpha, mode, row0=0, rows=None, eps=None, seed=0, offset=0):
    """One rv_latent_mix launch on device tensors (tests and users who inspect the mix).  mode: "list" (alpha = K
    float64 scalars, K * N rows), "f32" / "f64" (alpha [N]), "curve" (alpha [C] float64).  -> dict with z, eps, mu,
    logvar ([rows, L] fp32) and alpha ([rows] float64: the alpha each row used)."""
    modes = {"list": ALPHA_LIST, "f32": ALPHA_F32, "f64": ALPHA_F64, "curve": ALPHA_CURVE}
    m = modes[mode]
    N, L = mu_a.shape
    dev = mu_a.device
    a = alpha if torch.is_tensor(alpha) else torch.from_numpy(np.ascontiguousarray(alpha))
    a = a.to(device=dev, dtype=torch.float32 if m == ALPHA_F32 else torch.float64).contiguous()
    total = a.numel() * N if m == ALPHA_LIST else N
    rows = total - row0 if rows is None else rows
    out = {k: torch.empty((rows, L), dtype=torch.float32, device=dev) for k in ("z", "mu", "logvar")}
    out["alpha"] = torch.empty(rows, dtype=torch.float64, device=dev)
    if eps is None:
        out["eps"] = torch.empty((rows, L), dtype=torch.float32, device=dev)
        e_in, e_out = None, ptr(out["eps"])
    else:
        out["eps"] = eps.to(device=dev, dtype=torch.float32).contiguous()
        e_in, e_out = ptr(out["eps"]), None
    t = [x.to(device=dev, dtype=torch.float32).contiguous() for x in (mu_a, lv_a, mu_b, lv_b)]
    lib().rv_latent_mix(*[ptr(x) for x in t], N, L, m, ptr(a), a.numel(), row0, rows, e_in, e_out, int(seed),
                        int(offset), ptr(out["z"]), ptr(out["mu"]), ptr(out["logvar"]), ptr(out["alpha"]), stream_ptr())
    return out
