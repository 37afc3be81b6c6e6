"""Latent states: a hidden Markov model of a corpus, a shared temporal vocabulary for its recordings (the RV_HMM_* ops of
rv_mosaic; the rules: include/rawvae_hip.h, "Latent states").

S states over the first k whitened principal coordinates y = P (x - c) of the encoder's mu rows; state s emits
N(m_s, diag(v_s)), pi is the initial law and A the transition matrix.  Fitted by EM (Baum-Welch) over every file of a
corpus at once: the states mean the same in every recording, A says what follows what and for how long, the Viterbi
path labels any recording in that vocabulary and the log-likelihood says how well a recording belongs to the corpus.

  emit(x, centre, P, theta, S)                logb [T, S] fp64                                      RV_HMM_EMIT
  forward_backward(logb, row_start, theta, S, k)    the posteriors, one block [gamma | xi | ll]     RV_HMM_FORWARD_BACKWARD
  split_posteriors(block, T, S, n)            its views gamma [T, S], xi [n, S, S], ll [n]
  mstep(x, centre, P, block, row_start, theta, S, floor)       theta', info [S], moments [S, 1 + 2 k]    RV_HMM_MSTEP
  viterbi(logb, row_start, theta, S, k)       path [T] int32, score [n] fp64                        RV_HMM_VITERBI
  LatentStates(n_states, n_components, var_floor).fit(x, row_start, pca_or_walk, iters, tol, seed) -> the ll history
      .posteriors(x, row_start), .label(x, row_start) -> (path, score), .loglik(x, row_start)
      means_, variances_ [S, k], startprob_ [S], transmat_ [S, S], durations_ = 1 / (1 - A_ss) (numpy)
  fit_corpus(model, waves, hop, n_states, n_components, pca)   every waveform's mu through codec.FrameCodec, files apart
  write_states(path, states, ...) / read_states(path)          one .npz of fp64 arrays and the framing they were fitted at

x [T, L] fp32 on the device; its rows may have a pitch (x.stride(0) >= L).  A row that holds a value that is not finite is
an unobserved frame: it takes part in the chain but says nothing about the state.  row_start [n + 1] are the files' first
rows, 0 .. T, non-decreasing: an empty file is legal.  One EM iteration is three ops on one stream with no host sync
between them; only ll [n] is read back, once per iteration, for the stopping rule.
"""
import numpy as np
import torch

from . import _lib
from ._lib import mosaic_call as _call, ptr
from .corpus import check_row_start, encode_corpus, read_fitted, write_fitted
from .pca import LatentPCA
from .walk import LatentWalk, rank_of

S_MAX, K_MAX, L_MAX = 64, 64, 512    # csrc/hmm.hip


def theta_layout(S, k):
    """{part: slice} of theta = [m (S k) | w (S k) | g (S) | pi (S) | A (S S) | log pi (S) | log A (S S)] and its length"""
    o, at = {}, 0
    for name, n in (("m", S * k), ("w", S * k), ("g", S), ("pi", S), ("A", S * S), ("logpi", S), ("logA", S * S)):
        o[name] = slice(at, at + n)
        at += n
    return o, at


def pack_theta(m, v, pi, A):
    """theta (numpy fp64) of means m [S, k], variances v [S, k], pi [S] and A [S, S]; g's logarithms are added in
    ascending j from +0"""
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    pi, A = np.asarray(pi, np.float64), np.asarray(A, np.float64)
    S, k = m.shape
    o, n = theta_layout(S, k)
    acc = np.zeros(S)
    for j in range(k):
        acc = acc + np.log(v[:, j])
    th = np.empty(n)
    th[o["m"]], th[o["w"]], th[o["g"]] = m.ravel(), (1.0 / v).ravel(), -0.5 * (k * 1.8378770664093453 + acc)
    th[o["pi"]], th[o["A"]] = pi, A.ravel()
    with np.errstate(divide="ignore"):
        th[o["logpi"]], th[o["logA"]] = np.log(pi), np.log(A).ravel()
    return th


def _count(value, what, hi):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= value <= hi:
        raise ValueError("%s=%r must be an integer in [1, %d]" % (what, value, hi))
    return int(value)


def _latents(x):
    if (not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32 or x.device.type != "cuda" or x.shape[0] < 1
            or x.shape[1] < 1):
        raise ValueError("x must be a 2-D float32 device tensor with at least one row, got %s" % (
            "%s %s on %s" % (x.dtype, tuple(x.shape), x.device) if torch.is_tensor(x) else type(x).__name__))
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return x, (x.stride(0) if x.shape[0] > 1 else x.shape[1])


def _f64(t, what, shape, device="cuda"):
    if (not torch.is_tensor(t) or t.dtype != torch.float64 or (device and t.device.type != device)
            or tuple(t.shape) != tuple(shape)):
        raise ValueError("%s must be a float64 device tensor of shape %s, got %s" % (
            what, tuple(shape), "%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__))
    return t if t.is_contiguous() else t.contiguous()


def _rs_dev(row_start, T, device):
    rs = check_row_start(row_start, T, empty_files=True)
    return torch.from_numpy(rs).to(device), rs.size - 1


def workspace(T, S, k, device):
    """(ws, bytes): one workspace that serves FORWARD_BACKWARD, MSTEP and VITERBI at (T, S, k)"""
    n = _call(_lib.HMM_WORKSPACE, T=int(T), S=int(S), k=int(k)).ws_bytes
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device), n


def emit(x, centre, P, theta, S, out=None):
    """logb [T, S] fp64 of x [T, L] under theta: RV_HMM_EMIT.  centre [L] and P [k, L] fp64 on the device."""
    x, ldx = _latents(x)
    T, L = x.shape
    k = P.shape[0]
    P, centre = _f64(P, "P", (k, L)), _f64(centre, "centre", (L,))
    theta = _f64(theta, "theta", (theta_layout(S, k)[1],))
    logb = torch.empty((T, S), dtype=torch.float64, device=x.device) if out is None else out
    _call(_lib.HMM_EMIT, T=T, L=L, k=k, S=S, q=ptr(x), stride=ldx, centre=ptr(centre), basis=ptr(P), moment=ptr(theta),
          result=ptr(logb))
    return logb


def posteriors_size(T, S, n):
    """doubles of the posteriors of T frames in n sequences: gamma [T, S], xi [n, S, S] and ll [n] in one block"""
    return T * S + n * S * S + n


def split_posteriors(block, T, S, n):
    """(gamma [T, S], xi [n, S, S], ll [n]) as views of the block forward_backward writes"""
    return block[:T * S].view(T, S), block[T * S:T * S + n * S * S].view(n, S, S), block[T * S + n * S * S:]


def forward_backward(logb, row_start, theta, S, k, out=None, ws=None):
    """The posteriors of logb [T, S] over the sequences of row_start (host), one fp64 block [gamma | xi | ll]
    (split_posteriors): RV_HMM_FORWARD_BACKWARD.  out: the block to write into."""
    T = logb.shape[0]
    logb = _f64(logb, "logb", (T, S))
    theta = _f64(theta, "theta", (theta_layout(S, k)[1],))
    rs, n = row_start if isinstance(row_start, tuple) else _rs_dev(row_start, T, logb.device)
    dev = logb.device
    block = torch.empty(posteriors_size(T, S, n), dtype=torch.float64, device=dev) if out is None else out
    block = _f64(block, "the posteriors", (posteriors_size(T, S, n),))
    ws, nb = workspace(T, S, k, dev) if ws is None else ws
    _call(_lib.HMM_FORWARD_BACKWARD, T=T, S=S, k=k, n_rows=n, row_start=ptr(rs), result=ptr(logb), moment=ptr(theta),
          state=ptr(block), ws=ptr(ws), ws_bytes=nb)
    return block


def mstep(x, centre, P, block, row_start, theta, S, floor, out=None, ws=None, moments=False):
    """(theta', info [S] int32, moments [S, 1 + 2 k] or None) of the posteriors forward_backward left in `block`:
    RV_HMM_MSTEP.  floor: the variance floor (taken as float32).  out: (theta', info) to write into; with moments, theta'
    has S (1 + 2 k) doubles of room behind the parameters and the moments are that part of it."""
    x, ldx = _latents(x)
    T, L = x.shape
    k = P.shape[0]
    P, centre = _f64(P, "P", (k, L)), _f64(centre, "centre", (L,))
    n_theta = theta_layout(S, k)[1]
    theta = _f64(theta, "theta", (n_theta,))
    rs, n = row_start if isinstance(row_start, tuple) else _rs_dev(row_start, T, x.device)
    block = _f64(block, "the posteriors", (posteriors_size(T, S, n),))
    dev = x.device
    n_new = n_theta + (S * (1 + 2 * k) if moments else 0)
    new, info = out if out is not None else (torch.empty(n_new, dtype=torch.float64, device=dev),
                                             torch.empty(S, dtype=torch.int32, device=dev))
    new = _f64(new, "the new theta", (n_new,))
    ws, nb = workspace(T, S, k, dev) if ws is None else ws
    _call(_lib.HMM_MSTEP, T=T, L=L, k=k, S=S, q=ptr(x), stride=ldx, centre=ptr(centre), basis=ptr(P), state=ptr(block),
          n_rows=n, row_start=ptr(rs), moment=ptr(theta), lam=float(floor), mode=_lib.HMM_MOMENTS if moments else 0,
          result=ptr(new), info=ptr(info), ws=ptr(ws), ws_bytes=nb)
    return new[:n_theta], info, (new[n_theta:].view(S, 1 + 2 * k) if moments else None)


def viterbi(logb, row_start, theta, S, k, out=None, ws=None):
    """(path [T] int32, score [n] fp64): the best state sequence of every sequence of row_start: RV_HMM_VITERBI.  -1 along
    a sequence no path of which has a score above -inf."""
    T = logb.shape[0]
    logb = _f64(logb, "logb", (T, S))
    theta = _f64(theta, "theta", (theta_layout(S, k)[1],))
    rs, n = row_start if isinstance(row_start, tuple) else _rs_dev(row_start, T, logb.device)
    dev = logb.device
    path, score = out if out is not None else (torch.empty(T, dtype=torch.int32, device=dev),
                                               torch.empty(n, dtype=torch.float64, device=dev))
    ws, nb = workspace(T, S, k, dev) if ws is None else ws
    _call(_lib.HMM_VITERBI, T=T, S=S, k=k, n_rows=n, row_start=ptr(rs), result=ptr(logb), moment=ptr(theta), path=ptr(path),
          score=ptr(score), ws=ptr(ws), ws_bytes=nb)
    return path, score


def whitening(basis, k, device=None):
    """(centre [L], P [k, L]) fp64 on the device of a fitted LatentWalk (its P), a fitted LatentPCA (rows v_j / sqrt(lambda_j))
    or a (centre, P) pair; ValueError when it holds fewer than k usable axes."""
    if isinstance(basis, LatentWalk):
        basis._fitted()
        centre, P = basis.mean_, basis.P_
    elif isinstance(basis, LatentPCA):
        basis._fitted()
        lam = basis.explained_variance_.cpu().numpy()
        rank = min(rank_of(basis.all_variances_.cpu().numpy()), lam.size)
        if k > rank:
            raise ValueError("n_components=%d: the PCA holds %d axes of positive variance" % (k, rank))
        centre = basis.mean_
        P = torch.from_numpy(basis.components_[:k].cpu().numpy() / np.sqrt(lam[:k])[:, None]).to(centre.device)
    elif isinstance(basis, (tuple, list)) and len(basis) == 2:
        centre, P = (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)) for t in basis)
        if device is not None:
            centre, P = centre.to(device), P.to(device)
    else:
        raise TypeError("expected a fitted LatentPCA, a fitted LatentWalk or a (centre, P) pair, got %s" % type(basis).__name__)
    if P.dim() != 2 or P.shape[0] < k or centre.dim() != 1 or P.shape[1] != centre.numel():
        raise ValueError("n_components=%d: the basis holds P %s and centre %s" % (k, tuple(P.shape), tuple(centre.shape)))
    return centre.to(torch.float64).contiguous(), P[:k].to(torch.float64).contiguous()


class LatentStates:
    """The fitted model (see the module doc), all on x's device.

    After fit: theta_ (the parameter block), mean_ [L] and P_ [k, L] (the whitening), info_ [S] (1: the state held fewer
    than one frame in the last iteration and kept its emission), ll_history_, n_iter_, n_frames_, n_files_."""

    def __init__(self, n_states, n_components, var_floor=1e-3):
        self.n_states = _count(n_states, "n_states", S_MAX)
        self.n_components = _count(n_components, "n_components", K_MAX)
        try:
            ok = 0 < float(var_floor) < float("inf") and np.float32(var_floor) > 0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("var_floor=%r must be a finite positive number" % (var_floor,))
        self.var_floor = float(var_floor)
        self.theta_ = None

    def _set(self, theta, centre, P, n_frames, n_files, history=(), info=None):
        S, k = self.n_states, self.n_components
        L = centre.numel()
        if not k <= L <= L_MAX:
            raise ValueError("n_components=%d: the latents have %d dimensions (at most %d)" % (k, L, L_MAX))
        # (a model read onto the host can be inspected and written; every op checks for the device again)
        self.theta_ = _f64(theta, "theta", (theta_layout(S, k)[1],), None)
        self.mean_, self.P_ = _f64(centre, "centre", (L,), None), _f64(P, "P", (k, L), None)
        self.n_frames_, self.n_files_ = int(n_frames), int(n_files)
        self.ll_history_ = [float(v) for v in history]
        self.n_iter_ = len(self.ll_history_)
        self.info_ = info
        return self

    def _fitted(self):
        if self.theta_ is None:
            raise RuntimeError("LatentStates has not been fitted")

    def _part(self, name, shape):
        self._fitted()
        return self.theta_.cpu().numpy()[theta_layout(self.n_states, self.n_components)[0][name]].reshape(shape)

    @property
    def means_(self):
        return self._part("m", (self.n_states, self.n_components))

    @property
    def variances_(self):
        return 1.0 / self._part("w", (self.n_states, self.n_components))

    @property
    def startprob_(self):
        return self._part("pi", (self.n_states,))

    @property
    def transmat_(self):
        return self._part("A", (self.n_states, self.n_states))

    @property
    def durations_(self):
        """The mean stay in every state in frames, 1 / (1 - A_ss) (inf for an absorbing state)"""
        with np.errstate(divide="ignore"):
            return 1.0 / (1.0 - np.diag(self.transmat_))

    def initial_theta(self, x, centre, P, seed):
        """The start of EM, made on the host: S distinct observed frames chosen by numpy.random.RandomState(seed) as
        means (in ascending frame order), v = 1, pi uniform, A = 0.9 I + 0.1 / S."""
        S, k = self.n_states, self.n_components
        ok = np.flatnonzero(torch.isfinite(x).all(dim=1).cpu().numpy())
        if ok.size < S:
            raise ValueError("%d observed frames are fewer than the %d states" % (ok.size, S))
        pick = np.sort(np.random.RandomState(seed).choice(ok.size, S, replace=False))
        rows = x[torch.from_numpy(ok[pick]).to(x.device)].cpu().numpy()
        m = (np.asarray(rows, np.float64) - centre.cpu().numpy()) @ P.cpu().numpy()[:k].T
        return pack_theta(m, np.ones((S, k)), np.full(S, 1.0 / S), 0.9 * np.eye(S) + 0.1 / S)

    @torch.no_grad()
    def fit(self, x, row_start, pca_or_walk, iters=50, tol=1e-4, seed=0):
        """EM from initial_theta(seed) in the axes of a fitted LatentPCA or LatentWalk, of a (centre, P) pair or -- None -- of
        x's own principal axes: at most `iters` iterations, stopped early once an iteration gains less than `tol`
        per frame (tol = 0: never).  Returns the history: the log-likelihood of the corpus under the parameters each
        iteration started from, the sequences' ll added in ascending order."""
        S, k = self.n_states, self.n_components
        if torch.is_tensor(x) and x.dim() == 2 and x.shape[0] < S:
            raise ValueError("%d frames are fewer than the %d states" % (x.shape[0], S))
        x, _ = _latents(x)
        T, L = x.shape
        rs = check_row_start(row_start, T, empty_files=True)
        iters = _count(iters, "iters", 1 << 30)
        if not (isinstance(tol, (int, float)) and 0 <= tol < float("inf")):
            raise ValueError("tol=%r must be a finite number >= 0" % (tol,))
        centre, P = whitening(LatentPCA().fit(x.contiguous()) if pca_or_walk is None else pca_or_walk, k, x.device)
        if centre.numel() != L or centre.device != x.device:
            raise ValueError("the basis was fitted on %d-dimensional latents on %s, x is %s on %s" % (
                centre.numel(), centre.device, tuple(x.shape), x.device))
        if not k <= L <= L_MAX:
            raise ValueError("n_components=%d: the latents have %d dimensions (at most %d)" % (k, L, L_MAX))
        dev = x.device
        theta = torch.from_numpy(self.initial_theta(x, centre, P, seed)).to(dev)
        spare = torch.empty_like(theta)
        seqs = (torch.from_numpy(rs).to(dev), rs.size - 1)
        n = seqs[1]
        logb = torch.empty((T, S), dtype=torch.float64, device=dev)
        post = torch.empty(posteriors_size(T, S, n), dtype=torch.float64, device=dev)
        ll = split_posteriors(post, T, S, n)[2]
        info = torch.empty(S, dtype=torch.int32, device=dev)
        ws = workspace(T, S, k, dev)
        history = []
        for _ in range(iters):
            emit(x, centre, P, theta, S, out=logb)
            forward_backward(logb, seqs, theta, S, k, out=post, ws=ws)
            mstep(x, centre, P, post, seqs, theta, S, self.var_floor, out=(spare, info), ws=ws)
            theta, spare = spare, theta
            total = 0.0
            for v in ll.cpu().numpy():     # the one read of the iteration
                total = total + v
            history.append(float(total))
            if tol > 0 and len(history) > 1 and history[-1] - history[-2] < tol * T:
                break
        self._set(theta, centre, P, T, n, history, info)
        return list(self.ll_history_)

    def _logb(self, x, row_start):
        self._fitted()
        x, _ = _latents(x)
        if x.shape[1] != self.mean_.numel() or x.device != self.mean_.device:
            raise ValueError("the states were fitted on %d-dimensional latents on %s, x is %s on %s" % (
                self.mean_.numel(), self.mean_.device, tuple(x.shape), x.device))
        seqs = _rs_dev(row_start, x.shape[0], x.device)
        return emit(x, self.mean_, self.P_, self.theta_, self.n_states), seqs

    @torch.no_grad()
    def posteriors(self, x, row_start):
        """gamma [T, S] fp64: the probability of every state at every frame given its whole sequence"""
        logb, seqs = self._logb(x, row_start)
        block = forward_backward(logb, seqs, self.theta_, self.n_states, self.n_components)
        return split_posteriors(block, logb.shape[0], self.n_states, seqs[1])[0]

    @torch.no_grad()
    def loglik(self, x, row_start):
        """ll [n] fp64: the log-likelihood of every sequence"""
        logb, seqs = self._logb(x, row_start)
        block = forward_backward(logb, seqs, self.theta_, self.n_states, self.n_components)
        return split_posteriors(block, logb.shape[0], self.n_states, seqs[1])[2]

    @torch.no_grad()
    def label(self, x, row_start):
        """(path [T] int32, score [n] fp64): the Viterbi path of every sequence and its log-probability"""
        logb, seqs = self._logb(x, row_start)
        return viterbi(logb, seqs, self.theta_, self.n_states, self.n_components)


@torch.no_grad()
def fit_corpus(model, waves, hop=None, n_states=8, n_components=16, pca=None, iters=50, tol=1e-4, seed=0, var_floor=1e-3,
               max_rows=16384):
    """LatentStates fitted on the encoder's mu of every frame of every waveform, the files kept apart (row_start_);
    pca: a fitted LatentPCA or LatentWalk of the same model (None: the corpus's own principal axes)."""
    states = LatentStates(n_states, n_components, var_floor)
    x, starts = encode_corpus(model, waves, hop, max_rows)
    states.fit(x, starts, pca, iters, tol, seed)
    states.row_start_ = starts
    return states


_ARRAYS = ("theta", "mean", "whiten")
_META = ("segment_length", "latent_dim", "hop", "n_frames", "n_files", "n_states", "n_components", "n_iter")


def write_states(path, states, segment_length, hop=None):
    """One .npz: theta, mean [L] and whiten = P [k, L], all fp64, var_floor, ll_history, and segment_length, latent_dim,
    hop (-1: non-overlapping frames), n_frames, n_files, n_states, n_components, n_iter."""
    states._fitted()
    write_fitted(path, dict(theta=states.theta_, mean=states.mean_, whiten=states.P_),
                 dict(segment_length=segment_length, latent_dim=states.mean_.numel(), hop=hop, n_frames=states.n_frames_,
                      n_files=states.n_files_, n_states=states.n_states, n_components=states.n_components,
                      n_iter=states.n_iter_),
                 var_floor=float(states.var_floor), ll_history=np.asarray(states.ll_history_, dtype=np.float64))


def read_states(path, device="cuda"):
    """(LatentStates on `device`, {segment_length, latent_dim, hop (None: non-overlapping), n_frames, n_files, n_iter}) of
    write_states' file; ValueError when the arrays do not fit one another."""
    arrays, meta, extra = read_fitted(path, "states", _ARRAYS, _META, ("var_floor", "ll_history"))
    theta, mean, P = arrays.values()
    floor, history = float(extra["var_floor"]), np.asarray(extra["ll_history"], dtype=np.float64).reshape(-1)
    S, k, L = meta.pop("n_states"), meta.pop("n_components"), meta["latent_dim"]
    if (not 1 <= S <= S_MAX or not 1 <= k <= K_MAX or not k <= L <= L_MAX or theta.shape != (theta_layout(S, k)[1],)
            or mean.shape != (L,) or P.shape != (k, L)):
        raise ValueError("%s: theta %s, mean %s and whiten %s do not fit %d states, %d components and latent_dim %d" % (
            path, theta.shape, mean.shape, P.shape, S, k, L))
    dev = torch.device(device)
    states = LatentStates(S, k, floor)._set(*(torch.from_numpy(a).to(dev) for a in (theta, mean, P)), meta["n_frames"],
                                            meta["n_files"], history)
    return states, meta


def runs(path):
    """(offsets [F + 1], labels [F]) of a label sequence: its maximal runs of one state, as segment boundaries in frames"""
    path = np.asarray(path).reshape(-1)
    cuts = np.flatnonzero(np.diff(path) != 0) + 1
    offsets = np.concatenate([[0], cuts, [path.size]]).astype(np.int64)
    return offsets, path[offsets[:-1]].astype(np.int64)
