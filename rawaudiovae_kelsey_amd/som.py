"""Self-organising map of a corpus's latents on the device: the SOM that chooses the two sources of the reference's
tutorial.ipynb "Interpolations in Meso-scale" (725-805) and "Interpolations with Extensions" (1078-1146).

  LatentMap(model).describe(waves)   one descriptor per file: the mean mu over its frames (rv_segment_mean)
  LatentSOM(rows, cols).fit(x)       batch SOM on any [N, L] fp32 device tensor; each epoch is three launches on the
                                     current stream -- rv_som_bmu, rv_som_node_sums, rv_som_update -- and no host sync
  write_som(dir, ...)                clusters.json, data-concatenated.json (the notebook's two files) and som.npz
  read_som(dir)                      the two JSON files, read the way the notebook reads them

The epoch is the batch SOM: every row's best-matching unit (BMU) under the squared distance, per-node sums of member
rows, then w[m] = sum_b h(m, b) sums[b] / sum_b h(m, b) counts[b] with the Gaussian neighbourhood
h = exp(-|grid(m) - grid(b)|^2 / (2 sigma_t^2)), sigma_t = sigma0 (sigma1 / sigma0)^(t / (E - 1)).
"""
import functools
import json
import os

import numpy as np
import torch

from . import _lib
from ._lib import lib, ptr, stream_ptr
from .codec import FrameCodec
from .corpus import rows


def sigma_schedule(sigma0, sigma1, epochs):
    """[epochs] float64: sigma0 (sigma1 / sigma0)^(t / (E - 1)), or [sigma0] when E = 1."""
    E = int(epochs)
    if E == 1:
        return np.array([float(sigma0)])
    t = np.arange(E, dtype=np.float64)
    return float(sigma0) * (float(sigma1) / float(sigma0)) ** (t / (E - 1))


_rows = functools.partial(rows, wording="an [N, L]")


def bmu(x, w):
    """rv_som_bmu: (best int32 [N], second int32 [N], d_best fp32 [N], d_second fp32 [N]) of rows x against nodes w."""
    x, w = _rows(x), _rows(w, "w")
    if x.shape[1] != w.shape[1] or x.device != w.device:
        raise ValueError("x %s and w %s must share L and device" % (tuple(x.shape), tuple(w.shape)))
    N, M, L = x.shape[0], w.shape[0], x.shape[1]
    out = [torch.empty(N, dtype=t, device=x.device) for t in (torch.int32, torch.int32, torch.float32, torch.float32)]
    lib().rv_som_bmu(ptr(x), N, ptr(w), M, L, *[ptr(t) for t in out], stream_ptr())
    return tuple(out)


def node_sums(x, best, M):
    """rv_som_node_sums: (sums fp64 [M, L], counts int64 [M]) of the rows of x per node."""
    x = _rows(x)
    best = best.to(dtype=torch.int32).contiguous()
    if best.numel() != x.shape[0]:
        raise ValueError("%d BMUs for %d rows" % (best.numel(), x.shape[0]))
    sums = torch.empty((M, x.shape[1]), dtype=torch.float64, device=x.device)
    counts = torch.empty(M, dtype=torch.int64, device=x.device)
    lib().rv_som_node_sums(ptr(x), x.shape[0], x.shape[1], ptr(best), M, ptr(sums), ptr(counts), stream_ptr())
    return sums, counts


def update(sums, counts, w_old, rows, cols, sigma, out=None):
    """rv_som_update: the batch-SOM weights [M, L] fp32 from node sums and counts at neighbourhood width sigma."""
    w_old = _rows(w_old, "w_old")
    M, L = w_old.shape
    if M != rows * cols or tuple(sums.shape) != (M, L) or counts.numel() != M:
        raise ValueError("sums %s / counts %s / w_old %s do not fit a %dx%d grid" % (
            tuple(sums.shape), tuple(counts.shape), tuple(w_old.shape), rows, cols))
    w_new = torch.empty_like(w_old) if out is None else out
    lib().rv_som_update(ptr(sums.to(torch.float64).contiguous()), ptr(counts.to(torch.int64).contiguous()), ptr(w_old),
                        rows, cols, L, float(sigma), ptr(w_new), stream_ptr())
    return w_new


def segment_mean(x, offsets):
    """rv_segment_mean: [F, L] fp32 means of x[offsets[f] : offsets[f + 1]] (offsets: F + 1 ascending ints)."""
    x = _rows(x)
    off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
    if off.size < 2:
        raise ValueError("offsets needs at least 2 entries, got %d" % off.size)
    F = off.size - 1
    off_dev = torch.from_numpy(off).to(x.device)
    out = torch.empty((F, x.shape[1]), dtype=torch.float32, device=x.device)
    host = off.ctypes.data_as(_lib.C.POINTER(_lib.c_i64))
    lib().rv_segment_mean(ptr(x), x.shape[0], x.shape[1], ptr(off_dev), host, F, ptr(out), stream_ptr())
    return out


def grid_neighbours(a, b, cols):
    """True where nodes a and b (int arrays or tensors) are 8-neighbours (or equal) on a grid of `cols` columns."""
    return ((a // cols - b // cols).abs() <= 1) & ((a % cols - b % cols).abs() <= 1)


class LatentSOM:
    """Batch SOM on a rows x cols grid (node m at (m // cols, m % cols)); see the module doc for one epoch.

    fit(x) initialises w = x[numpy.random.default_rng(seed).choice(N, M, replace=N < M)] and runs `epochs` epochs.
    Afterwards `weights` is [rows, cols, L] fp32 on x's device and `sigmas` the schedule used."""

    def __init__(self, rows, cols, sigma0=None, sigma1=0.5, epochs=50, seed=0):
        self.rows, self.cols = int(rows), int(cols)
        if self.rows < 1 or self.cols < 1 or self.rows * self.cols < 2:
            raise ValueError("grid %sx%s: needs at least 2 nodes" % (rows, cols))
        self.sigma0 = float(max(self.rows, self.cols) / 2.0 if sigma0 is None else sigma0)
        self.sigma1 = float(sigma1)
        if not (np.isfinite(self.sigma0) and self.sigma0 > 0 and np.isfinite(self.sigma1) and self.sigma1 > 0):
            raise ValueError("sigma0 %r and sigma1 %r must be positive and finite" % (sigma0, sigma1))
        self.epochs = int(epochs)
        if self.epochs < 1:
            raise ValueError("epochs must be at least 1, got %d" % self.epochs)
        self.seed = int(seed)
        self.sigmas = sigma_schedule(self.sigma0, self.sigma1, self.epochs)
        self._w = None

    @property
    def M(self):
        return self.rows * self.cols

    @property
    def weights(self):
        if self._w is None:
            raise RuntimeError("LatentSOM has not been fitted")
        return self._w.view(self.rows, self.cols, -1)

    @torch.no_grad()
    def fit(self, x):
        x = _rows(x)
        N, L = x.shape
        M = self.M
        pick = np.random.default_rng(self.seed).choice(N, M, replace=N < M)
        w = x[torch.from_numpy(pick).to(x.device)].contiguous()
        w_next = torch.empty_like(w)
        best, second = (torch.empty(N, dtype=torch.int32, device=x.device) for _ in range(2))
        d1, d2 = (torch.empty(N, dtype=torch.float32, device=x.device) for _ in range(2))
        sums = torch.empty((M, L), dtype=torch.float64, device=x.device)
        counts = torch.empty(M, dtype=torch.int64, device=x.device)
        L_ = lib()
        st = stream_ptr()
        for sigma in self.sigmas:
            L_.rv_som_bmu(ptr(x), N, ptr(w), M, L, ptr(best), ptr(second), ptr(d1), ptr(d2), st)
            L_.rv_som_node_sums(ptr(x), N, L, ptr(best), M, ptr(sums), ptr(counts), st)
            L_.rv_som_update(ptr(sums), ptr(counts), ptr(w), self.rows, self.cols, L, float(sigma), ptr(w_next), st)
            w, w_next = w_next, w
        self._w = w
        return self

    @torch.no_grad()
    def assign(self, x):
        """(best, second, dist): int32 [N] node indices and fp32 [N] squared distance to the best node."""
        best, second, d1, _ = bmu(x, self.weights.view(self.M, -1))
        return best, second, d1

    @torch.no_grad()
    def quantization_error(self, x):
        """Mean distance (not squared) of each row to its best node."""
        _, _, d = self.assign(x)
        return float(d.double().sqrt().mean())

    @torch.no_grad()
    def topographic_error(self, x):
        """Fraction of rows whose best and second nodes are not 8-neighbours on the grid."""
        best, second, _ = self.assign(x)
        return float((~grid_neighbours(best.long(), second.long(), self.cols)).double().mean())


class LatentMap:
    """File descriptors for the SOM: the mean encoder mu of each file's frames, framed like TestDataset (hop=None) or
    AudioDataset (hop=int), through `codec.FrameCodec`.  The model is read, never written."""

    def __init__(self, model, hop=None, max_rows=16384):
        self.hop = None if hop is None else int(hop)
        self.codec = FrameCodec(model, max_rows=max_rows)

    @torch.no_grad()
    def describe(self, waves):
        """[F, L] fp32 device tensor: row f = mean mu over the frames of waves[f] (one rv_segment_mean launch)."""
        waves = list(waves)
        if not waves:
            raise ValueError("describe needs at least one waveform")
        mus, offsets = [], [0]
        for f, w in enumerate(waves):
            try:
                w = self.codec.wave(w)
                padded, n_frames = self.codec.pad(w, w.numel(), self.hop)
                mu, _ = self.codec.encode(padded, n_frames, self.hop)
            except ValueError as e:
                raise ValueError("waveform %d: %s" % (f, e))
            mus.append(mu)
            offsets.append(offsets[-1] + mu.shape[0])
        return segment_mean(torch.cat(mus, 0) if len(mus) > 1 else mus[0], offsets)


def write_som(out_dir, files_rel, assignment, som, descriptors=None, hop=None, x=None):
    """Write clusters.json ({node: [file indices ascending]} for every node), data-concatenated.json ({i: [node,
    path relative to the audio folder]}) and som.npz (weights, grid, sigma schedule, seed, epochs, hop, descriptors,
    quantisation and topographic error) into out_dir.  `assignment` is each file's node (int [F]); the errors are
    measured on `x` (default: descriptors) when given."""
    os.makedirs(out_dir, exist_ok=True)
    a = np.asarray(assignment.cpu() if torch.is_tensor(assignment) else assignment).astype(np.int64).reshape(-1)
    if a.size != len(files_rel):
        raise ValueError("%d assignments for %d files" % (a.size, len(files_rel)))
    clusters = {str(m): [int(i) for i in np.flatnonzero(a == m)] for m in range(som.M)}
    data = {str(i): [int(a[i]), str(p)] for i, p in enumerate(files_rel)}
    with open(os.path.join(out_dir, "clusters.json"), "w") as f:
        json.dump(clusters, f, indent=1)
    with open(os.path.join(out_dir, "data-concatenated.json"), "w") as f:
        json.dump(data, f, indent=1)
    x = descriptors if x is None else x
    qe = som.quantization_error(x) if x is not None else np.nan
    te = som.topographic_error(x) if x is not None else np.nan
    desc = np.zeros((0, som.weights.shape[-1]), np.float32) if descriptors is None else descriptors.cpu().numpy()
    np.savez(os.path.join(out_dir, "som.npz"), weights=som.weights.cpu().numpy(), grid=np.array([som.rows, som.cols]),
             sigmas=som.sigmas, sigma0=som.sigma0, sigma1=som.sigma1, seed=som.seed, epochs=som.epochs,
             hop=-1 if hop is None else int(hop), descriptors=desc, assignment=a, quantization_error=qe,
             topographic_error=te)
    return qe, te


def read_som(som_dir):
    """(clusters, data): the two JSON files as the notebook loads them (tutorial.ipynb:725-732), from write_som or from
    an outside trainer: clusters[str(node)] -> file indices, data[str(index)][1] -> path relative to the audio folder."""
    with open(os.path.join(som_dir, "clusters.json")) as f:
        clusters = json.load(f)
    with open(os.path.join(som_dir, "data-concatenated.json")) as f:
        data = json.load(f)
    return clusters, data


def cluster_paths(clusters, data, audio_dir, node):
    """Paths of node's files in list order, as concat_audio_som walks them (tutorial.ipynb:743-756).  KeyError when the
    node is missing; an empty list when it has no files."""
    return [os.path.join(str(audio_dir), data[str(i)][1]) for i in clusters[str(node)]]
