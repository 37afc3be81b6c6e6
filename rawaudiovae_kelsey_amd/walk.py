"""New audio in the manner of a corpus: a fitted walk through the latent space, offline and block by block (the
RV_PCA_LAGCOV and RV_WALK_* ops of rv_mosaic; the rules: include/rawvae_hip.h, "Latent walk").

The model is first-order and linear-Gaussian in whitened principal coordinates.  With c, v_j, lambda_j the corpus's
centre, principal axes and variances (pca.LatentPCA), P the rows v_j / sqrt(lambda_j) and C1 the lag-1 moment of the
centred latents over the frame pairs of one file, divided by T - 1 like the covariance:

  A = P C1 P^T,   Q = I - A A^T = U diag(q) U^T,   B = U diag(sqrt(max(q, 0)))
  w' = A w + B e,  e ~ temperature * N(0, I);   z = c + offset + R^T w,  R = diag(sqrt(lambda)) V_k

||A||_2 <= 1 by construction (no guard, no knob) and A A^T + B B^T = I, so the stationary latents have exactly the
corpus's mean and its covariance on the kept axes.

  lagcov(x, row_start, centre)       C1 [L, L] fp64 of x [T, L] fp32, bit-identical from run to run
  LatentWalk(k, mode).fit(x, row_start, pca=None)
                                     mode "full" or "diagonal" (A and B diagonal: every axis its own AR(1));
                                     A_, B_, R_, P_, persistence_ = diag(A), predictability_ = ||A||_F^2 / k, rank_
  LatentWalk.whiten(x)               the state of given latents: P (x - c), [N, k] fp32
  fit_corpus(model, waves, hop)      every waveform's mu through codec.FrameCodec, the files kept apart
  write_walk(path, walk, ...) / read_walk(path)   one .npz of fp64 arrays and the framing they were fitted at
  StreamingWalk(model, walk, n_streams, block, hop, window, seed)
                                     generate(eps=None) -> [n_streams, block]; reset, set_state, state, last_latents,
                                     temperature [n_streams] and offset [n_streams, L] (device tensors a captured graph
                                     sees), capture() / replay()

Four launches per block (csrc/walk.hip, csrc/stream.hip): the step of every frame of the block, fc3, fc4 and the
overlap-add of streaming resynthesis.  Nothing syncs.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from . import pca as P_
from ._lib import RvError, mosaic_call as _call, ptr
from .corpus import check_row_start, encode_corpus, read_fitted, rows as _rows, write_fitted
from .pca import L_MAX, LatentPCA, _vector
from .stream import GraphReplay, StreamingVAE, each_stream

MODES = ("full", "diagonal")
RANK_TOL = 1e-12     # an axis counts while lambda_j > RANK_TOL * lambda_0


def rank_of(variances):
    """The number of eigenvalues (descending) with lambda_j > 1e-12 lambda_0."""
    lam = np.asarray(variances, dtype=np.float64)
    return int(np.count_nonzero(lam > RANK_TOL * lam[0])) if lam.size and lam[0] > 0 else 0


def check_components(k, rank):
    """k (None: the rank) as the number of kept axes, 1 <= k <= rank; ValueError naming the rank."""
    if k is None:
        k = rank
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= rank:
        raise ValueError("n_components=%r must be in [1, r], r = %d the rank of the corpus's covariance "
                         "(the eigenvalues above 1e-12 of the largest)" % (k, rank))
    return int(k)


def _workspace(T, k, L, device):
    n = _call(_lib.WALK_WORKSPACE, T=int(T), k=int(k), L=int(L)).ws_bytes
    return torch.empty(max(n, 1), dtype=torch.uint8, device=device), n


def lagcov(x, row_start, centre):
    """C1 [L, L] fp64 of x [T, L] fp32 (T >= 2), row_start the host's [n_files + 1] file boundaries and centre [L] fp64:
    RV_PCA_LAGCOV."""
    x = _rows(x)
    T, L = x.shape
    if T < 2 or L > L_MAX:
        raise ValueError("x %s: needs at least 2 rows and at most %d columns" % (tuple(x.shape), L_MAX))
    rs = check_row_start(row_start, T)
    centre = _vector(centre, "centre", L, torch.float64, x.device)
    rs_dev = torch.from_numpy(rs).to(x.device)
    c1 = torch.empty((L, L), dtype=torch.float64, device=x.device)
    ws, n = _workspace(T, 0, L, x.device)
    _call(_lib.PCA_LAGCOV, T=T, L=L, n_rows=rs.size - 1, q=ptr(x), row_start=ptr(rs_dev), ws=ptr(ws), ws_bytes=n,
          centre=ptr(centre), basis=ptr(c1))
    return c1


class LatentWalk:
    """The fitted walk (see the module doc), all on x's device.

    After fit: mean_ [L], components_ [k, L], explained_variance_ [k], A_ and B_ [k, k], P_ and R_ [k, L], all fp64;
    Q_ [k, k] (mode "full"); dyn_ [2, k, k] = A^T and B^T as the step reads them; persistence_ [k] (numpy) and
    predictability_ of the model in use; rank_, n_frames_, n_files_."""

    def __init__(self, n_components=None, mode="full"):
        if n_components is not None:
            if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or n_components < 1:
                raise ValueError("n_components=%r must be a positive integer or None" % (n_components,))
            n_components = int(n_components)
        if mode not in MODES:
            raise ValueError("mode=%r: expected 'full' or 'diagonal'" % (mode,))
        self.n_components, self.mode = n_components, mode
        self.mean_ = None

    def _set(self, mean, components, variances, dyn, P, R, rank, n_frames, n_files, Q=None):
        k, L = components.shape
        for t, shape, what in ((mean, (L,), "mean"), (variances, (k,), "variances"), (dyn, (2, k, k), "dynamics"),
                               (P, (k, L), "P"), (R, (k, L), "R")):
            if tuple(t.shape) != shape or t.dtype != torch.float64:
                raise ValueError("%s is %s %s, expected float64 %s" % (what, t.dtype, tuple(t.shape), shape))
        self.mean_, self.components_, self.explained_variance_ = mean, components, variances
        self.dyn_, self.P_, self.R_, self.Q_ = dyn.contiguous(), P.contiguous(), R.contiguous(), Q
        self.A_, self.B_ = self.dyn_[0].t(), self.dyn_[1].t()
        a = self.dyn_[0].cpu().numpy()
        self.persistence_ = np.diag(a).copy()
        self.predictability_ = float((a * a).sum() / k)
        self.rank_, self.n_frames_, self.n_files_ = int(rank), int(n_frames), int(n_files)
        self.n_components = k
        return self

    @torch.no_grad()
    def fit(self, x, row_start, pca=None):
        x = _rows(x)
        T, L = x.shape
        rs = check_row_start(row_start, T)
        if pca is None:
            pca = LatentPCA().fit(x)
        pca._fitted()
        if pca.mean_.numel() != L or pca.mean_.device != x.device:
            raise ValueError("the PCA was fitted on %d-dimensional latents on %s, x is %s on %s" % (
                pca.mean_.numel(), pca.mean_.device, tuple(x.shape), x.device))
        rank = rank_of(pca.all_variances_.cpu().numpy())
        k = check_components(self.n_components, rank)
        if k > pca.components_.shape[0]:
            raise ValueError("n_components=%d: the PCA holds %d components" % (k, pca.components_.shape[0]))
        comp = pca.components_[:k].contiguous()
        lam = pca.explained_variance_[:k].contiguous()
        c1 = lagcov(x, rs, pca.mean_)
        dev = x.device
        res = torch.empty(2 * k * k + 2 * k * L, dtype=torch.float64, device=dev)
        ws, n = _workspace(0, k, L, dev)
        _call(_lib.WALK_FIT, mode=_lib.WALK_DYNAMICS, k=k, L=L, ws=ptr(ws), ws_bytes=n, basis=ptr(comp),
              eigenvalues=ptr(lam), moment=ptr(c1), result=ptr(res))
        A, Q = res[:k * k].view(k, k), res[k * k:2 * k * k].view(k, k)
        Pm, R = res[2 * k * k:2 * k * k + k * L].view(k, L), res[2 * k * k + k * L:].view(k, L)
        dyn = torch.empty((2, k, k), dtype=torch.float64, device=dev)
        if self.mode == "diagonal":
            _call(_lib.WALK_FIT, mode=_lib.WALK_DIAGONAL, k=k, L=L, basis=ptr(A), result=ptr(dyn))
            Q = None
        else:
            q, U, sweeps, converged = P_.eig(Q)
            if not converged:
                raise RvError("LatentWalk.fit: the Jacobi eigensolver did not converge on Q in %d sweeps" % sweeps)
            _call(_lib.WALK_FIT, mode=_lib.WALK_NOISE, k=k, L=L, basis=ptr(A), eigenvalues=ptr(q), moment=ptr(U),
                  result=ptr(dyn))
        self.lagcov_ = c1
        return self._set(pca.mean_, comp, lam, dyn, Pm.clone(), R.clone(), rank, T, rs.size - 1,
                         None if Q is None else Q.clone())

    def _fitted(self):
        if self.mean_ is None:
            raise RuntimeError("LatentWalk has not been fitted")

    @torch.no_grad()
    def whiten(self, x, out=None):
        """The state of latents x [N, L] fp32: P (x - c), [N, k] fp32 (RV_PCA_APPLY's projection on the rows of P)."""
        self._fitted()
        return P_.project(x, self.P_, self.mean_, out)


@torch.no_grad()
def fit_corpus(model, waves, hop=None, n_components=None, mode="full", max_rows=16384):
    """LatentWalk fitted on the encoder's mu of every frame of every waveform, framed like pca.fit_corpus; the files'
    frame counts are kept (row_start_), so no pair of frames spans two files."""
    walk = LatentWalk(n_components, mode)
    x, starts = encode_corpus(model, waves, hop, max_rows)
    if starts[-1] < 2:
        raise ValueError("fit_corpus needs at least 2 frames, the waveforms make %d" % starts[-1])
    walk.fit(x, starts)
    walk.row_start_ = starts
    return walk


_ARRAYS = ("mean", "components", "variances", "dynamics", "whiten", "unwhiten")
_META = ("segment_length", "latent_dim", "hop", "n_frames", "n_files", "rank", "diagonal")


def write_walk(path, walk, segment_length, hop=None):
    """One .npz: mean [L], components [k, L], variances [k], dynamics [2, k, k] (A^T, B^T), whiten = P [k, L] and
    unwhiten = R [k, L], all fp64, and segment_length, latent_dim, hop (-1: non-overlapping frames), n_frames,
    n_files, rank, diagonal."""
    walk._fitted()
    arrays = dict(zip(_ARRAYS, (walk.mean_, walk.components_, walk.explained_variance_, walk.dyn_, walk.P_, walk.R_)))
    write_fitted(path, arrays,
                 dict(segment_length=segment_length, latent_dim=walk.mean_.numel(), hop=hop, n_frames=walk.n_frames_,
                      n_files=walk.n_files_, rank=walk.rank_, diagonal=walk.mode == "diagonal"))


def read_walk(path, device="cuda"):
    """(LatentWalk on `device`, {segment_length, latent_dim, hop (None: non-overlapping), n_frames, n_files}) of
    write_walk's file; ValueError when the arrays do not fit one another."""
    arrays, meta, _ = read_fitted(path, "walk", _ARRAYS, _META)
    arrays = list(arrays.values())
    mean, comp, lam, dyn, Pm, R = arrays
    L = meta["latent_dim"]
    k = comp.shape[0] if comp.ndim == 2 else -1
    if (mean.shape != (L,) or not 1 <= k <= L or comp.shape != (k, L) or lam.shape != (k,) or dyn.shape != (2, k, k)
            or Pm.shape != (k, L) or R.shape != (k, L) or not k <= meta["rank"] <= L):
        raise ValueError("%s: mean %s, components %s, variances %s, dynamics %s, whiten %s and unwhiten %s do not fit "
                         "latent_dim %d and rank %d" % (path, mean.shape, comp.shape, lam.shape, dyn.shape, Pm.shape,
                                                        R.shape, L, meta["rank"]))
    dev = torch.device(device)
    walk = LatentWalk(k, "diagonal" if meta.pop("diagonal") else "full")._set(
        *(torch.from_numpy(a).to(dev) for a in arrays), meta.pop("rank"), meta["n_frames"], meta["n_files"])
    return walk, meta


class StreamingWalk(GraphReplay):
    """`n_streams` independent walks decoded block by block through a `VAE` on the GPU (see the module doc).

    `temperature` [n_streams] and `offset` [n_streams, L] (LatentPCA.offset makes one) may be written in place between
    calls; `state` [n_streams, k] fp64 is the whitened state w.  A stream that is not primed (after construction or a
    reset) draws its first state from the stationary distribution: w = e."""

    def __init__(self, model, walk, n_streams, block, hop=None, window=None, seed=0):
        if not isinstance(walk, LatentWalk):
            raise TypeError("StreamingWalk needs a fitted LatentWalk, got %s" % type(walk).__name__)
        walk._fitted()
        # the decoder's descriptor, window, overlap-add state and the temperature / offset controls are the streaming
        # engine's; its encoder half is never launched
        self.stream = sv = StreamingVAE(model, n_streams, block, hop, window, seed)
        self.model, self.walk = model, walk
        self.S, self.H, self.L, self.hop, self.device = sv.S, sv.H, sv.L, sv.hop, sv.device
        self.n_streams, self.block, self.window, self.seed = sv.n_streams, sv.block, window, sv.seed
        self.frames_per_block = sv.frames_per_block
        self.k = walk.components_.shape[0]
        if walk.mean_.numel() != self.L:
            raise ValueError("the walk was fitted on %d-dimensional latents, the model has latent_dim %d" % (
                walk.mean_.numel(), self.L))
        if walk.mean_.device != self.device:
            raise RvError("the walk is on %s; the model computes on %s" % (walk.mean_.device, self.device))
        self.temperature, self.offset = sv.temperature, sv.offset
        self._state = torch.zeros((self.n_streams, self.k), dtype=torch.float64, device=self.device)
        self._primed = torch.zeros(self.n_streams, dtype=torch.int32, device=self.device)
        self._z = torch.zeros((self.n_streams * self.frames_per_block, self.L), dtype=torch.float32, device=self.device)
        self._silence = torch.zeros((self.n_streams, self.block), dtype=torch.float32, device=self.device)

    def parameters(self):
        return self.stream.parameters()

    def _step(self, x, y, eps, stream):
        sd = self.stream.desc(x, y, eps)
        w = self.walk
        _call(_lib.WALK_STEP, stream, live=C.pointer(sd), k=self.k, L=self.L, ldo=self.L, centre=ptr(w.mean_),
              basis=ptr(w.R_), moment=ptr(w.dyn_), out=ptr(self._z), state=ptr(self._state), primed=ptr(self._primed))

    @torch.no_grad()
    def generate(self, eps=None):
        """One block of every stream -> [n_streams, block] fp32.  eps: None (Philox keyed by seed, stream, frame and
        axis) or [n_streams, block // hop, k] fp32 standard-normal draws."""
        if eps is not None:
            shape = (self.n_streams, self.frames_per_block, self.k)
            if (not torch.is_tensor(eps) or eps.dtype != torch.float32 or eps.device != self.device
                    or tuple(eps.shape) != shape):
                raise ValueError("eps has shape %s, expected a float32 tensor %s on %s" % (
                    "%s %s on %s" % (eps.dtype, tuple(eps.shape), eps.device) if torch.is_tensor(eps) else type(eps).__name__,
                    shape, self.device))
            eps = eps.contiguous()
        y = torch.empty((self.n_streams, self.block), dtype=torch.float32, device=self.device)
        self._step(self._silence, y, eps, None)
        return y

    @torch.no_grad()
    def reset(self, streams=None):
        """Zero the overlap-add tail, the frame counter and the state of `streams` (an index or a list; None = all) and
        clear their primed flags: the next frame starts from a fresh draw."""
        self.stream.reset(streams)
        for s in each_stream(streams, self.n_streams):
            sel = slice(None) if s < 0 else s
            self._state[sel] = 0
            self._primed[sel] = 0

    @torch.no_grad()
    def set_state(self, w, streams=None):
        """Set the state of `streams` (None = all, in order) to the rows of w [len(streams), k] (LatentWalk.whiten
        makes them) and set their primed flags: the next frame is A w + B e."""
        which = list(range(self.n_streams)) if streams is None else [s for s in each_stream(streams, self.n_streams)]
        if not torch.is_tensor(w) or w.device != self.device or not w.is_floating_point():
            raise ValueError("w must be a floating-point tensor on %s" % self.device)
        if w.dim() == 1:
            w = w.view(1, -1)
        if tuple(w.shape) != (len(which), self.k):
            raise ValueError("w has shape %s, expected %s" % (tuple(w.shape), (len(which), self.k)))
        for row, s in enumerate(which):
            self._state[s] = w[row].to(torch.float64)
            self._primed[s] = 1

    @property
    def state(self):
        """The whitened state w [n_streams, k] fp64 after the last frame (the tensor the launches read and write)."""
        return self._state

    def last_latents(self):
        """The latent rows z of the last call's frames as a view [n_streams, block // hop, L]."""
        return self._z.view(self.n_streams, self.frames_per_block, self.L)

    @torch.no_grad()
    def capture(self):
        """Capture one block (eps from Philox) as a graph; `replay()` then generates one block per call into
        `graph_output` [n_streams, block].  The graph holds the Parameters' pointers: replaying after a Parameter was
        replaced raises."""
        return self._capture(lambda st: self._step(self.graph_input, self.graph_output, None, st))

    @torch.no_grad()
    def replay(self):
        """One block through the captured graph on the current stream.  Returns `graph_output` (overwritten by the next
        replay)."""
        return self._replay(0, "replay()")
