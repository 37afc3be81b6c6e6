"""Block-by-block streaming resynthesis: audio in, decoded audio out, one block of samples per stream per call.

`StreamingVAE(model, n_streams, block, hop=None, window=None, seed=0)` keeps, per stream, the last P = S - hop input
samples, the overlap-add tail and a frame counter, all on the device.  One `process(x)` consumes `block` samples of
every stream and decodes the block // hop frames that became complete:

  frames    Xp = [0] * P + X (X: every sample fed since the last reset); frame f = Xp[f * hop : f * hop + S]
  latent    mu' = mu * scale + offset;  z = mu' + (temperature * eps) * exp(logvar / 2)   (controls per stream, held in
            device tensors, so a captured graph sees updates); eps from Philox(seed) keyed by (stream, frame, latent
            index) or given explicitly
  output    Yp[t] = sum_f w[t - f hop] D_f[t - f hop] / sum_f w[t - f hop] over the frames f >= 0 that cover t; call k
            returns Yp[k * block : (k + 1) * block], i.e. the input delayed by `latency` = P samples

The numerator is accumulated in ascending frame order from +0 and the normaliser is a function of the position alone,
so the output is byte-identical for any block size.  With hop == S and no window the output is the decoded frames
themselves (the reference's non-overlapping reconstruction).

Five launches per call (csrc/stream.hip): fc1 reading its frames from the history and the new block in place, the two
heads with the controls and the reparameterisation, fc3, fc4, then overlap-add + history update.  Every GEMM is
`rv_small_linear_f32`'s k-ordered fmaf chain, the arithmetic of the exact-fp32 inference path (`VAE.encode` /
`decode` under `torch.no_grad()`).  `capture()` / `replay(x)` run the same call as a captured graph; the capture, the
check that the model's Parameters are still the captured ones and the replay are `GraphReplay`'s, which live mosaicing
(mosaic.StreamingMosaic) mixes in too.  What that class needs of a StreamingVAE is public: `desc(x, y, eps)`,
`check_input(x)`, `parameters()`; `each_stream` is the walk of a `reset(streams)`.
"""
import numpy as np
import torch

from . import _lib
from ._lib import StreamDesc, lib, ptr, stream_ptr

WINDOWS = (None, "hann")
_LAYERS = ("fc1", "fc21", "fc22", "fc3", "fc4")


def check_args(segment_length, block, hop=None, window=None):
    """Validate a stream configuration without a device -> (hop, latency, frames per block).  Raises ValueError."""
    S = int(segment_length)
    hop = S if hop is None else int(hop)
    block = int(block)
    if S <= 0 or hop <= 0 or block <= 0:
        raise ValueError("segment_length, hop and block must be positive (got %d, %d, %d)" % (S, hop, block))
    if S % hop != 0:
        raise ValueError("hop %d does not divide segment_length %d" % (hop, S))
    if block % hop != 0 or block < hop:
        raise ValueError("block %d must be a positive multiple of hop %d" % (block, hop))
    if window not in WINDOWS:
        raise ValueError("window %r: expected None (rectangular) or 'hann'" % (window,))
    if window == "hann" and 2 * hop > S:
        raise ValueError("a Hann window needs hop <= segment_length / 2 (got hop %d, segment_length %d): "
                         "its window sum is zero at frame starts" % (hop, S))
    return hop, S - hop, block // hop


def window_values(segment_length, window=None):
    """The fp32 window: ones, or the periodic Hann window 0.5 - 0.5 cos(2 pi n / S) in float64, rounded once."""
    S = int(segment_length)
    if window is None:
        return np.ones(S, dtype=np.float32)
    if window == "hann":
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(S, dtype=np.float64) / S)).astype(np.float32)
    raise ValueError("window %r: expected None (rectangular) or 'hann'" % (window,))


def window_norm(w, hop):
    """Normaliser table [P + hop] fp32: entry t is the sum of w[t - f hop] over the frames f >= 0 that cover
    position t, added in ascending f from +0 in fp32; positions t >= P use entry P + t % hop."""
    w = np.asarray(w, dtype=np.float32)
    S = w.size
    P = S - hop
    out = np.zeros(P + hop, dtype=np.float32)
    for t in range(P + hop):
        acc = np.float32(0.0)
        for f in range(max(0, (t - S) // hop + 1), t // hop + 1):
            acc = np.float32(acc + w[t - f * hop])
        out[t] = acc
    return out


def each_stream(streams, n_streams):
    """The stream indices a reset(streams) walks: -1 (all of them at once) for None, else the int or every entry of
    the iterable, each checked against n_streams as it comes up (ValueError)."""
    if streams is None:
        yield -1
        return
    for s in ([streams] if isinstance(streams, int) else list(streams)):
        s = int(s)
        if not 0 <= s < n_streams:
            raise ValueError("stream %d of %d" % (s, n_streams))
        yield s


class GraphReplay:
    """capture() / replay() of a block processor as graphs on static buffers `graph_input` / `graph_output`
    [n_streams, block].  The class that mixes this in has n_streams, block and device, parameters() (the model
    Parameters its launches read) and check_input(x).  The graphs hold the Parameters' pointers: replaying after a
    Parameter was replaced raises."""
    _graphs = ()

    def _capture(self, *launches):
        """Allocate the static buffers, note the Parameters' pointers and capture each launch(raw stream) as a graph
        of its own on a side stream."""
        from .engine import Graph
        self.graph_input = torch.zeros((self.n_streams, self.block), dtype=torch.float32, device=self.device)
        self.graph_output = torch.zeros_like(self.graph_input)
        self._held = [(p, p.data_ptr()) for p in self.parameters()]
        side = torch.cuda.Stream(self.device)
        graphs = []
        for launch in launches:
            side.wait_stream(torch.cuda.current_stream(self.device))
            g = Graph(side)
            with g:
                launch(side.cuda_stream)
            torch.cuda.current_stream(self.device).wait_stream(side)
            graphs.append(g)
        self._graphs = graphs
        return self

    def _replay(self, which, what, x=None):
        """Graph `which` on the current stream, x (optional) copied into `graph_input` first -> `graph_output`.
        `what` names the caller in the error raised before capture()."""
        if not self._graphs:
            raise _lib.RvError("%s before capture()" % what)
        if any(p is not q or p.data_ptr() != a for p, (q, a) in zip(self.parameters(), self._held)):
            raise _lib.RvError("a Parameter of the model was replaced after capture(): capture again")
        if x is not None:
            self.graph_input.copy_(self.check_input(x))
        self._graphs[which].launch(torch.cuda.current_stream(self.device))
        return self.graph_output


class StreamingVAE(GraphReplay):
    """Stateful streaming resynthesis of `n_streams` streams through a `VAE` on the GPU (see the module doc).

    The model's Parameters are read in place on every eager call.  Control tensors (`scale` [n_streams, L],
    `offset` [n_streams, L], `temperature` [n_streams]) may be written in place between calls."""

    def __init__(self, model, n_streams, block, hop=None, window=None, seed=0):
        from .model import VAE
        if not isinstance(model, VAE):
            raise TypeError("StreamingVAE needs a rawvae.model.VAE (the one-hidden-layer model), got %s"
                            % type(model).__name__)
        self.model = model
        self.S, self.H, self.L = int(model.segment_length), int(model.n_units), int(model.latent_dim)
        n_streams = int(n_streams)
        if n_streams <= 0:
            raise ValueError("n_streams must be positive, got %d" % n_streams)
        self.hop, self.latency, self.frames_per_block = check_args(self.S, block, hop, window)
        self.n_streams, self.block, self.window = n_streams, int(block), window
        self.seed = int(seed)
        self.device = model.fc1.weight.device
        if self.device.type != "cuda":
            raise _lib.RvError("StreamingVAE computes on the GPU only: the model is on %s" % self.device)
        self.parameters()                                # raises on a non-fp32 / non-contiguous parameter
        dev, F, L = self.device, self.frames_per_block, self.L
        w = window_values(self.S, window)
        self._window = torch.from_numpy(w).to(dev)
        self._norm = torch.from_numpy(window_norm(w, self.hop)).to(dev)
        self.scale = torch.ones((n_streams, L), dtype=torch.float32, device=dev)
        self.offset = torch.zeros((n_streams, L), dtype=torch.float32, device=dev)
        self.temperature = torch.ones(n_streams, dtype=torch.float32, device=dev)
        self._mu = torch.zeros((n_streams * F, L), dtype=torch.float32, device=dev)
        self._logvar = torch.zeros_like(self._mu)
        nbytes = lib().rv_stream_workspace_bytes(self.S, self.H, L, n_streams, self.block, self.hop)
        if nbytes <= 0:
            raise ValueError("rv_stream_workspace_bytes rejected the extents")
        self._ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)

    # -- helpers ---------------------------------------------------------------------------------------------------
    def parameters(self):
        """The model's ten Parameters in the descriptor's order, checked: RvError unless contiguous fp32 on the device."""
        out = []
        for name in _LAYERS:
            layer = getattr(self.model, name)
            for p in (layer.weight, layer.bias):
                if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device:
                    raise _lib.RvError("%s: parameters must be contiguous fp32 on %s" % (name, self.device))
                out.append(p)
        return out

    def desc(self, x, y, eps):
        """The rv_stream_desc of one call on x, y [n_streams, block] (None: no block, as for a reset) and eps."""
        d = StreamDesc()
        d.S, d.H, d.L, d.n_streams, d.block, d.hop = self.S, self.H, self.L, self.n_streams, self.block, self.hop
        for (name, p) in zip(("w1", "b1", "w21", "b21", "w22", "b22", "w3", "b3", "w4", "b4"), self.parameters()):
            setattr(d, name, p.data_ptr())
        d.x, d.ld_x = (ptr(x), x.stride(0)) if x is not None else (None, self.block)
        d.y, d.ld_y = (ptr(y), y.stride(0)) if y is not None else (None, self.block)
        d.mu, d.logvar, d.eps_in, d.seed = ptr(self._mu), ptr(self._logvar), ptr(eps), self.seed
        d.scale, d.offset, d.temperature = ptr(self.scale), ptr(self.offset), ptr(self.temperature)
        d.window, d.norm, d.workspace = ptr(self._window), ptr(self._norm), ptr(self._ws)
        return d

    def _check(self, t, shape, what):
        if not torch.is_tensor(t):
            raise TypeError("%s must be a torch tensor, got %s" % (what, type(t).__name__))
        if t.device != self.device:
            raise _lib.RvError("%s is on %s; the stream computes on %s (no CPU path)" % (what, t.device, self.device))
        if t.dtype != torch.float32:
            raise TypeError("%s must be float32, got %s" % (what, t.dtype))
        if tuple(t.shape) != shape:
            raise ValueError("%s has shape %s, expected %s" % (what, tuple(t.shape), shape))

    def check_input(self, x):
        """x as the [n_streams, block] fp32 device tensor a call reads (TypeError, ValueError or RvError otherwise)."""
        if torch.is_tensor(x) and x.dim() == 1 and self.n_streams == 1:
            x = x.view(1, -1)
        self._check(x, (self.n_streams, self.block), "x")
        if x.stride(1) != 1 or x.stride(0) < self.block:
            x = x.contiguous()
        return x

    # -- public surface --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def process(self, x, eps=None):
        """One block: x [n_streams, block] fp32 on the device -> output [n_streams, block] (the input `latency`
        samples late).  eps: None (Philox) or [n_streams, block // hop, L] fp32."""
        x = self.check_input(x)
        if eps is not None:
            self._check(eps, (self.n_streams, self.frames_per_block, self.L), "eps")
            eps = eps.contiguous()
        y = torch.empty((self.n_streams, self.block), dtype=torch.float32, device=self.device)
        lib().rv_stream_process(self.desc(x, y, eps), stream_ptr())
        return y

    @torch.no_grad()
    def reset(self, streams=None):
        """Zero the history, the overlap-add tail and the frame counter of `streams` (an index or a list; None = all)."""
        d = self.desc(None, None, None)
        for s in each_stream(streams, self.n_streams):
            lib().rv_stream_reset(d, s, stream_ptr())

    def last_latents(self):
        """(mu, logvar) of the last call's frames as views [n_streams, block // hop, L] (before the controls)."""
        shape = (self.n_streams, self.frames_per_block, self.L)
        return self._mu.view(shape), self._logvar.view(shape)

    @torch.no_grad()
    def capture(self):
        """Capture one call (eps from Philox) as a graph on static buffers `graph_input` / `graph_output`
        [n_streams, block]; `replay(x)` then runs one block per call.  The graph holds the Parameters' pointers:
        replaying after a Parameter was replaced raises."""
        return self._capture(lambda st: lib().rv_stream_process(self.desc(self.graph_input, self.graph_output, None), st))

    @torch.no_grad()
    def replay(self, x=None):
        """One block through the captured graph on the current stream; x (optional) is copied into `graph_input`
        first.  Returns `graph_output` (overwritten by the next replay)."""
        return self._replay(0, "replay()", x)
