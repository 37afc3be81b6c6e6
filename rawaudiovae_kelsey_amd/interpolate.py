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
the exact-fp32 inference kernels of `VAE.encode` / `VAE.decode` under `torch.no_grad()`; the framing, the encoder and
the decoder launches are `codec.FrameCodec`'s, which the SOM, mosaicing and evaluation share.

Memory: mu / logvar of both sources are kept whole ([N, L] fp32 each); per chunk of at most `max_rows` frames one
h [rows, H] and one z [rows, L] buffer.  Every row's arithmetic is independent of the chunking, so the output is
bit-identical for any `max_rows`.
"""
import numpy as np
import torch

from ._lib import ALPHA_CURVE, ALPHA_F32, ALPHA_F64, ALPHA_LIST, lib, ptr, stream_ptr
from .codec import MAX_GEMM_ROWS, FrameCodec, frame_layout  # noqa: F401  (both names are part of this module's surface)


def matched_length(n_a, n_b, mode="repeat"):
    """Length both sources have after the notebook's match_audio_size (tutorial.ipynb:423-437): "repeat" repeats the
    shorter one up to the longer one's length, "crop" cuts the longer one to the shorter one's."""
    if mode == "repeat":
        return max(int(n_a), int(n_b))
    if mode == "crop":
        return min(int(n_a), int(n_b))
    raise ValueError("match mode %r: expected 'repeat' or 'crop'" % (mode,))


class LatentInterpolator:
    """Encode two sounds, mix their latent distributions, decode the mix into one waveform (see the module doc).

    `model` is a `VAE` on the GPU; its parameters are read, never written (the model's parameters, `_rng_calls` and
    operand shadows stay as they were).  eps is either given ([rows, L] fp32, rows = the output frames) or drawn on
    the device from `seed` with the Philox stream of `VAE.reparameterize` (offset 0).  `codec` is the FrameCodec that
    frames, encodes and decodes."""

    def __init__(self, model, max_rows=16384):
        self.codec = c = FrameCodec(model, max_rows)
        self.model, self.max_rows, self.device = model, c.max_rows, c.device
        self.S, self.H, self.L = c.S, c.H, c.L

    # -- helpers ---------------------------------------------------------------------------------------------------
    def _mix_decode(self, dists, n_frames, mode, alpha, n_alpha, rows_total, eps, seed):
        mu_a, lv_a, mu_b, lv_b = dists
        if eps is not None:
            eps = eps.to(device=self.device, dtype=torch.float32).contiguous()
            if eps.numel() != rows_total * self.L:
                raise ValueError("eps has %d elements, expected [%d, %d]" % (eps.numel(), rows_total, self.L))
        out = torch.empty(rows_total * self.S, dtype=torch.float32, device=self.device)
        z = torch.empty((min(self.max_rows, rows_total), self.L), dtype=torch.float32, device=self.device)
        h = self.codec.hidden(rows_total)
        for r0, rows in self.codec.chunks(rows_total):
            e = None if eps is None else eps.data_ptr() + 4 * r0 * self.L
            lib().rv_latent_mix(ptr(mu_a), ptr(lv_a), ptr(mu_b), ptr(lv_b), n_frames, self.L, mode, ptr(alpha), n_alpha,
                                r0, rows, e, None, int(seed), 0, ptr(z), None, None, None, stream_ptr())
            self.codec.decode_chunk(z[:rows], h, out[r0 * self.S:])
        return out

    def _sources(self, a, b, hop, match):
        c = self.codec
        a, b = c.wave(a), c.wave(b)
        n = matched_length(a.numel(), b.numel(), match)
        (pa, n_frames), (pb, _) = c.pad(a, n, hop), c.pad(b, n, hop)
        return c.encode(pa, n_frames, hop) + c.encode(pb, n_frames, hop), n_frames

    # -- public surface --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_audio(self, wave, hop=None):
        """(mu, logvar) [frames, L] of a waveform framed like TestDataset (hop=None) or AudioDataset (hop=int):
        the notebook's raw_to_z_dist (tutorial.ipynb:456-470) in exact fp32."""
        w = self.codec.wave(wave)
        padded, n_frames = self.codec.pad(w, w.numel(), hop)
        return self.codec.encode(padded, n_frames, hop)

    @torch.no_grad()
    def match_length(self, a, b, mode="repeat"):
        """Both waveforms at matched_length(len(a), len(b), mode), as device tensors (rv_match_pad)."""
        a, b = self.codec.wave(a), self.codec.wave(b)
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
