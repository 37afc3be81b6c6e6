"""The frame codec: waveforms to latent distributions and latents back to frames, by the exact-fp32 inference kernels
of `VAE.encode` / `VAE.decode` under `torch.no_grad()` (rv_linear_fp32), on the caller's current stream.

  codec = FrameCodec(model, max_rows)
  codec.wave(w)                    a waveform (device tensor or numpy array) as a 1-D fp32 device tensor
  codec.pad(w, n_valid, hop)       rv_match_pad: repeated or cropped to n_valid samples, zero-padded to the framing's
                                   length (frame_layout) -> (padded waveform, frames)
  codec.encode(padded, n, hop)     fc1 reading its frames from the waveform through the leading dimension (ldx = hop),
                                   then fc21, fc22 -> (mu, logvar) [n, L]
  codec.decode(z, out=None)        fc3, then fc4 + tanh -> [T, S], or written into `out`
  codec.chunks(T), codec.hidden(T), codec.decode_chunk(z, h, out)
                                   what decode is made of, for callers that produce z chunk by chunk into one buffer
  codec.linear(...), codec.weights(name)
                                   one rv_linear_fp32 launch on raw pointers; a layer's (weight, bias)

Interpolation, the SOM's descriptors, mosaicing and evaluation all frame, encode and decode through this class.

Memory: per chunk of at most `max_rows` frames one h [rows, H] buffer (and, at the callers that mix or gather latents,
one z [rows, L]).  Every row's arithmetic is independent of the chunking, so the result is bit-identical for any
`max_rows`.
"""
import numpy as np
import torch

from . import _lib
from ._lib import ACT_NONE, ACT_RELU, ACT_TANH, lib, ptr, stream_ptr

MAX_GEMM_ROWS = 65535 * 64    # rv_linear_fp32's launch grid


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


class FrameCodec:
    """The encoder and decoder of a `VAE` on the GPU over whole waveforms, `max_rows` frames per launch (see the
    module doc).  The model's parameters are read, never written (`_rng_calls` and operand shadows stay as they
    were)."""

    def __init__(self, model, max_rows=16384):
        max_rows = int(max_rows)
        if not 1 <= max_rows <= MAX_GEMM_ROWS:
            raise ValueError("max_rows must be in [1, %d], got %d" % (MAX_GEMM_ROWS, max_rows))
        self.model = model
        self.max_rows = max_rows
        self.S, self.H, self.L = int(model.segment_length), int(model.n_units), int(model.latent_dim)
        self.device = model.fc1.weight.device
        if self.device.type != "cuda":
            # the text every user of the codec has raised since it was LatentInterpolator's own check
            raise _lib.RvError("LatentInterpolator computes on the GPU only: the model is on %s" % self.device)

    def weights(self, name):
        """(weight, bias) of layer `name`, detached and contiguous."""
        t = getattr(self.model, name)
        return t.weight.detach().contiguous(), t.bias.detach().contiguous()

    def wave(self, w):
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

    def pad(self, w, n_valid, hop):
        """rv_match_pad: w repeated or cropped to n_valid samples, zeros up to the framing's padded length
        -> (padded waveform, frames)."""
        n_frames, padded = frame_layout(n_valid, self.S, hop)
        if n_frames < 1:
            raise ValueError("%d samples make no frame of %d samples at hop %s" % (n_valid, self.S, hop))
        dst = torch.empty(padded, dtype=torch.float32, device=self.device)
        lib().rv_match_pad(ptr(w), w.numel(), n_valid, ptr(dst), padded, stream_ptr())
        return dst, n_frames

    def linear(self, x, ldx, rows, name, act, y, ldy):
        """One rv_linear_fp32 launch of layer `name`: x, y are device addresses, ldx, ldy their row pitches."""
        W, b = self.weights(name)
        N, K = W.shape
        lib().rv_linear_fp32(x, ldx, ptr(W), K, ptr(b), rows, N, K, act, y, ldy, stream_ptr())

    def chunks(self, T):
        """(r0, rows) of the chunks of at most max_rows rows that cover T rows."""
        for r0 in range(0, T, self.max_rows):
            yield r0, min(self.max_rows, T - r0)

    def hidden(self, T):
        """The h [min(max_rows, T), H] buffer the chunks of T rows share."""
        return torch.empty((min(self.max_rows, T), self.H), dtype=torch.float32, device=self.device)

    def encode(self, padded, n_frames, hop):
        """fc1 -> (fc21, fc22) over the frames of a padded waveform, max_rows frames at a time -> (mu, logvar)."""
        step = self.S if hop is None else int(hop)
        mu = torch.empty((n_frames, self.L), dtype=torch.float32, device=self.device)
        lv = torch.empty_like(mu)
        h = self.hidden(n_frames)
        for f0, rows in self.chunks(n_frames):
            self.linear(padded.data_ptr() + 4 * f0 * step, step, rows, "fc1", ACT_RELU, ptr(h), self.H)
            self.linear(ptr(h), self.H, rows, "fc21", ACT_NONE, ptr(mu[f0:]), self.L)
            self.linear(ptr(h), self.H, rows, "fc22", ACT_NONE, ptr(lv[f0:]), self.L)
        return mu, lv

    def decode_chunk(self, z, h, out):
        """fc3 + ReLU into h, then fc4 + tanh: the rows of z [rows <= max_rows, L] (contiguous) decoded into the
        rows * S contiguous floats that `out` (a tensor or a slice of one, of any shape) starts with."""
        rows = z.shape[0]
        self.linear(ptr(z), self.L, rows, "fc3", ACT_RELU, ptr(h), self.H)
        self.linear(ptr(h), self.H, rows, "fc4", ACT_TANH, ptr(out), self.S)

    def decode(self, z, out=None):
        """z [T, L] fp32 decoded into [T, S], or into `out`: a contiguous [T, S] tensor or a slice of T * S samples of
        the output waveform.  Returns the [T, S] tensor or `out`."""
        T = z.shape[0]
        z = z.contiguous()
        if out is None:
            out = torch.empty((T, self.S), dtype=torch.float32, device=self.device)
        if out.numel() != T * self.S or not out.is_contiguous():
            raise ValueError("out must hold %d x %d contiguous samples, got shape %s" % (T, self.S, tuple(out.shape)))
        h, flat = self.hidden(T), out.view(-1)
        for r0, rows in self.chunks(T):
            self.decode_chunk(z[r0:r0 + rows], h, flat[r0 * self.S:])
        return out
