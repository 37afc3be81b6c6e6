"""Switching walk: one linear-Gaussian law per state of a fitted hidden Markov model, so that generated audio has parts,
returns and contrast (the RV_SWITCH_* ops of rv_mosaic; the rules: include/rawvae_hip.h, "Switching walk"; the
derivation: DESIGN.md section 7.18).

In the HMM's whitened coordinates y = P (x - c), state s emitting N(m_s, diag(v_s)):

  r_t = sum_i gamma_t(i) (y_t - m_i) / sd_i                      the standardised residual of a frame under its posterior
  A_j[a, b] = C1_j[a, b] / (sqrt(D'_j[a]) sqrt(D_j[b]))          a cross-correlation of r over the pairs weighted by gamma'(j)
  Q_j = I - A_j A_j^T = U diag(q) U^T; q_min < 0: A_j <- g A_j   the contraction guard, g = 1 / sqrt(1 - q_min)
  B_j = U diag(sqrt(q))                                          so that A_j A_j^T + B_j B_j^T = I for every state
  s' ~ A_hmm[s, .] (or forced);  u' = A_s' u + B_s' e;  y = m_s' + sd_s' o u';  z = c + offset + R^T y

Every step maps covariance I to I whatever the state sequence: given its state, a generated frame has exactly the HMM's
emission law, and the frames are continuous in time.

  residual(x, centre, P, theta, gamma, S)         the residual block [r (T k) | observed (T)]             RV_SWITCH_RESIDUAL
  split_residual(block, T, k)                     its views r [T, k] fp64 and observed [T] uint8
  moments(block, gamma, row_start, S, k)          [N | D' | D | C1] fp64                                  RV_SWITCH_MOMENTS
  split_moments(mo, S, k)                         its views N [S], D' [S, k], D [S, k], C1 [S, k, k]
  dynamics(mo, S, k)                              A [S, k, k], Q [S, k, k], info [S]                      RV_SWITCH_FIT
  noise(A, U, q)                                  dyn [S, 2, k, k], g [S]                                 RV_SWITCH_FIT
  SwitchingWalk(states).fit(x, row_start)         pairs_, predictability_, shrink_, info_ (numpy), phi_, R_
  fit_corpus(model, waves, states, hop)
  write_switching(path, sw, ...) / read_switching(path)
  StreamingSwitchingWalk(model, sw, n_streams, block, hop, window, seed)
      generate(eps=None, uniforms=None, states=None) -> [n_streams, block]; last_states, last_latents, reset, set_state,
      prime, temperature, offset, forced (the tensor a captured graph reads), capture() / replay()
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import RvError, mosaic_call as _call, ptr
from .corpus import check_row_start, encode_corpus, read_fitted, write_fitted
from .states import (K_MAX, L_MAX, S_MAX, LatentStates, _f64, _latents, emit, forward_backward, posteriors_size,
                     split_posteriors, theta_layout, workspace as hmm_workspace)
from .stream import GraphReplay, StreamingVAE, each_stream


def _up256(n):
    return (n + 255) // 256 * 256


def phi_layout(S, k):
    """{part: slice} of phi = [m (S k) | sd (S k) | pi (S) | A (S S) | dyn (S 2 k k)] and its length"""
    o, at = {}, 0
    for name, n in (("m", S * k), ("sd", S * k), ("pi", S), ("A", S * S), ("dyn", S * 2 * k * k)):
        o[name] = slice(at, at + n)
        at += n
    return o, at


def residual_bytes(T, k):
    """bytes of the residual block: r [T, k] fp64, then observed [T] bytes on a 256-byte boundary"""
    return _up256(8 * T * k) + T


def split_residual(block, T, k):
    """(r [T, k] fp64, observed [T] uint8) as views of the block residual() writes"""
    return block[:8 * T * k].view(torch.float64).view(T, k), block[_up256(8 * T * k):_up256(8 * T * k) + T]


def moments_size(S, k):
    return S + 2 * S * k + S * k * k


def split_moments(mo, S, k):
    """(N [S], D' [S, k], D [S, k], C1 [S, k, k]) as views of the block moments() writes"""
    a, b = S + S * k, S + 2 * S * k
    return mo[:S], mo[S:a].view(S, k), mo[a:b].view(S, k), mo[b:].view(S, k, k)


def _aligned_bytes(n, device):
    t = torch.empty(max(n, 256), dtype=torch.uint8, device=device)
    if t.data_ptr() % 256:
        raise RvError("the allocator returned a block that is not 256-byte aligned")
    return t


def workspace(T, S, k, device):
    """(ws, bytes) of RV_SWITCH_MOMENTS at (T, S, k)"""
    n = _call(_lib.SWITCH_WORKSPACE, T=int(T), S=int(S), k=int(k)).ws_bytes
    return _aligned_bytes(n, device), n


def residual(x, centre, P, theta, gamma, S, out=None):
    """The residual block of x [T, L] under theta and the posteriors gamma [T, S]: RV_SWITCH_RESIDUAL."""
    x, ldx = _latents(x)
    T, L = x.shape
    k = P.shape[0]
    P, centre = _f64(P, "P", (k, L)), _f64(centre, "centre", (L,))
    theta = _f64(theta, "theta", (theta_layout(S, k)[1],))
    gamma = _f64(gamma, "gamma", (T, S))
    block = _aligned_bytes(residual_bytes(T, k), x.device) if out is None else out
    _call(_lib.SWITCH_RESIDUAL, T=T, L=L, k=k, S=S, q=ptr(x), stride=ldx, centre=ptr(centre), basis=ptr(P), moment=ptr(theta),
          state=ptr(gamma), result=ptr(block))
    return block


def moments(block, gamma, row_start, S, k, out=None, ws=None):
    """[N | D' | D | C1] of the residual block and gamma [T, S] over the pairs inside the files of row_start (the host's
    boundaries, or the checked (device tensor, n_files) pair): RV_SWITCH_MOMENTS."""
    T = gamma.shape[0]
    gamma = _f64(gamma, "gamma", (T, S))
    if T < 2:
        raise ValueError("%d frame makes no pair" % T)
    dev = gamma.device
    if isinstance(row_start, tuple):
        rs_dev, n = row_start
    else:
        rs = check_row_start(row_start, T, empty_files=True)
        rs_dev, n = torch.from_numpy(rs).to(dev), rs.size - 1
    mo = torch.empty(moments_size(S, k), dtype=torch.float64, device=dev) if out is None else out
    ws, nb = workspace(T, S, k, dev) if ws is None else ws
    _call(_lib.SWITCH_MOMENTS, T=T, S=S, k=k, n_rows=n, row_start=ptr(rs_dev), moment=ptr(block), state=ptr(gamma),
          result=ptr(mo), ws=ptr(ws), ws_bytes=nb)
    return mo


def dynamics(mo, S, k, out=None):
    """(A [S, k, k], Q [S, k, k], info [S] int32) of the moments block: RV_SWITCH_FIT, mode RV_SWITCH_DYNAMICS."""
    mo = _f64(mo, "the moments", (moments_size(S, k),))
    res, info = out if out is not None else (torch.empty(2 * S * k * k, dtype=torch.float64, device=mo.device),
                                             torch.empty(S, dtype=torch.int32, device=mo.device))
    _call(_lib.SWITCH_FIT, mode=_lib.SWITCH_DYNAMICS, S=S, k=k, moment=ptr(mo), result=ptr(res), info=ptr(info))
    return res[:S * k * k].view(S, k, k), res[S * k * k:].view(S, k, k), info


def eig_states(Q):
    """(q [S, k], U [S, k, k], info [S, 2] int32) of the symmetric Q [S, k, k]: RV_PCA_EIG once per state on a copy, the S
    launches enqueued back to back without a read."""
    S, k, _ = Q.shape
    U = Q.clone()
    q = torch.empty((S, k), dtype=torch.float64, device=Q.device)
    info = torch.empty((S, 2), dtype=torch.int32, device=Q.device)
    n = _call(_lib.PCA_WORKSPACE, T=0, L=k).ws_bytes
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=Q.device)
    for j in range(S):
        _call(_lib.PCA_EIG, L=k, ws=ptr(ws), ws_bytes=n, basis=U[j].data_ptr(), eigenvalues=q[j].data_ptr(),
              info=info[j].data_ptr())
    return q, U, info


def noise(A, U, q, out=None):
    """(dyn [S, 2, k, k] = [A_j^T | B_j^T], g [S]) after the contraction guard: RV_SWITCH_FIT, mode RV_SWITCH_NOISE."""
    S, k, _ = A.shape
    A, U, q = _f64(A, "A", (S, k, k)), _f64(U, "U", (S, k, k)), _f64(q, "q", (S, k))
    res = torch.empty(2 * S * k * k + S, dtype=torch.float64, device=A.device) if out is None else out
    _call(_lib.SWITCH_FIT, mode=_lib.SWITCH_NOISE, S=S, k=k, basis=ptr(A), moment=ptr(U), eigenvalues=ptr(q), result=ptr(res))
    return res[:2 * S * k * k].view(S, 2, k, k), res[2 * S * k * k:]


def unwhitening(P):
    """R [k, L] with R P^T = I: solve(P P^T, P) in numpy float64 on the host (sqrt(lambda) v for a PCA's P)"""
    Pn = P.cpu().numpy()
    return torch.from_numpy(np.ascontiguousarray(np.linalg.solve(Pn @ Pn.T, Pn))).to(P.device)


def pack_phi(m, sd, pi, A, dyn):
    """phi (numpy fp64) of its parts"""
    S, k = m.shape
    o, n = phi_layout(S, k)
    phi = np.empty(n)
    for name, a in (("m", m), ("sd", sd), ("pi", pi), ("A", A), ("dyn", dyn)):
        phi[o[name]] = np.asarray(a, np.float64).ravel()
    return phi


class SwitchingWalk:
    """The fitted switching model over a fitted LatentStates, all on its device.

    After fit: phi_ (the model block RV_SWITCH_STEP reads), mean_ [L], P_ and R_ [k, L], dyn_ [S, 2, k, k]; numpy: pairs_ [S]
    (N_j), predictability_ [S] = ||A_j||_F^2 / k, shrink_ [S] (the guard's g, 1 where it did not act), info_ [S] (1: fewer than
    two pairs, A_j = 0); n_frames_, n_files_."""

    def __init__(self, states):
        if not isinstance(states, LatentStates):
            raise TypeError("SwitchingWalk needs a fitted LatentStates, got %s" % type(states).__name__)
        states._fitted()
        self.states = states
        self.n_states, self.n_components = states.n_states, states.n_components
        self.phi_ = None

    def _set(self, phi, mean, P, R, pairs, shrink, info, n_frames, n_files):
        S, k = self.n_states, self.n_components
        L = mean.numel()
        o, n = phi_layout(S, k)
        for t, shape, what in ((phi, (n,), "phi"), (mean, (L,), "mean"), (P, (k, L), "whiten"), (R, (k, L), "unwhiten")):
            if tuple(t.shape) != shape or t.dtype != torch.float64:
                raise ValueError("%s is %s %s, expected float64 %s" % (what, t.dtype, tuple(t.shape), shape))
        self.phi_, self.mean_, self.P_, self.R_ = phi.contiguous(), mean.contiguous(), P.contiguous(), R.contiguous()
        self.dyn_ = self.phi_[o["dyn"]].view(S, 2, k, k)
        a = self.dyn_[:, 0].cpu().numpy()
        self.predictability_ = (a * a).sum(axis=(1, 2)) / k
        self.pairs_ = np.asarray(pairs, np.float64).reshape(S)
        self.shrink_ = np.asarray(shrink, np.float64).reshape(S)
        self.info_ = np.asarray(info, np.int64).reshape(S)
        self.n_frames_, self.n_files_ = int(n_frames), int(n_files)
        return self

    def _fitted(self):
        if self.phi_ is None:
            raise RuntimeError("SwitchingWalk has not been fitted")

    def _part(self, name, shape):
        self._fitted()
        return self.phi_.cpu().numpy()[phi_layout(self.n_states, self.n_components)[0][name]].reshape(shape)

    @property
    def means_(self):
        return self._part("m", (self.n_states, self.n_components))

    @property
    def scales_(self):
        return self._part("sd", (self.n_states, self.n_components))

    @property
    def transmat_(self):
        return self._part("A", (self.n_states, self.n_states))

    @torch.no_grad()
    def fit(self, x, row_start):
        """The per-state dynamics of x [T, L] (T >= 2) under the states' posteriors: emit, forward_backward, then RESIDUAL,
        MOMENTS, FIT (dynamics), S eigensolves, FIT (noise) on one stream; one read of the eigensolvers' info at the end."""
        st = self.states
        S, k = self.n_states, self.n_components
        x, _ = _latents(x)
        T, L = x.shape
        if T < 2:
            raise ValueError("%d frame makes no pair" % T)
        if L != st.mean_.numel() or x.device != st.mean_.device:
            raise ValueError("the states were fitted on %d-dimensional latents on %s, x is %s on %s" % (
                st.mean_.numel(), st.mean_.device, tuple(x.shape), x.device))
        rs = check_row_start(row_start, T, empty_files=True)
        dev = x.device
        seqs = (torch.from_numpy(rs).to(dev), rs.size - 1)
        logb = emit(x, st.mean_, st.P_, st.theta_, S)
        post = forward_backward(logb, seqs, st.theta_, S, k, ws=hmm_workspace(T, S, k, dev))
        gamma = split_posteriors(post, T, S, seqs[1])[0].contiguous()
        block = residual(x, st.mean_, st.P_, st.theta_, gamma, S)
        mo = moments(block, gamma, seqs, S, k)
        A, Q, info = dynamics(mo, S, k)
        q, U, einfo = eig_states(Q)
        dyn, g = noise(A, U, q)
        einfo = einfo.cpu().numpy()                     # the one read
        if not einfo[:, 1].all():
            raise RvError("SwitchingWalk.fit: the Jacobi eigensolver did not converge on Q of state %d in %d sweeps" % (
                int(np.argmin(einfo[:, 1])), int(einfo[np.argmin(einfo[:, 1]), 0])))
        o, n = theta_layout(S, k)
        th = st.theta_
        phi = torch.cat([th[o["m"]], torch.sqrt(1.0 / th[o["w"]]), th[o["pi"]], th[o["A"]], dyn.reshape(-1)])
        self.moments_ = mo
        return self._set(phi, st.mean_, st.P_, unwhitening(st.P_), split_moments(mo, S, k)[0].cpu().numpy(), g.cpu().numpy(),
                         info.cpu().numpy(), T, rs.size - 1)


@torch.no_grad()
def fit_corpus(model, waves, states, hop=None, max_rows=16384):
    """SwitchingWalk fitted on the encoder's mu of every frame of every waveform, the files kept apart (row_start_)."""
    sw = SwitchingWalk(states)
    x, starts = encode_corpus(model, waves, hop, max_rows)
    if starts[-1] < 2:
        raise ValueError("fit_corpus needs at least 2 frames, the waveforms make %d" % starts[-1])
    sw.fit(x, starts)
    sw.row_start_ = starts
    return sw


_ARRAYS = ("phi", "mean", "whiten", "unwhiten", "theta")
_META = ("segment_length", "latent_dim", "hop", "n_frames", "n_files", "n_states", "n_components")
_EXTRA = ("pairs", "shrink", "flags", "var_floor")


def write_switching(path, sw, segment_length, hop=None):
    """One .npz: phi, mean [L], whiten = P [k, L], unwhiten = R [k, L] and the states' theta, all fp64; pairs, shrink, flags [S]
    and var_floor; segment_length, latent_dim, hop (-1: non-overlapping frames), n_frames, n_files, n_states, n_components."""
    sw._fitted()
    write_fitted(path, dict(phi=sw.phi_, mean=sw.mean_, whiten=sw.P_, unwhiten=sw.R_, theta=sw.states.theta_),
                 dict(segment_length=segment_length, latent_dim=sw.mean_.numel(), hop=hop, n_frames=sw.n_frames_,
                      n_files=sw.n_files_, n_states=sw.n_states, n_components=sw.n_components),
                 pairs=sw.pairs_, shrink=sw.shrink_, flags=sw.info_, var_floor=float(sw.states.var_floor))


def read_switching(path, device="cuda"):
    """(SwitchingWalk on `device`, {segment_length, latent_dim, hop (None: non-overlapping), n_frames, n_files}) of
    write_switching's file; ValueError when the arrays do not fit one another."""
    arrays, meta, extra = read_fitted(path, "switching", _ARRAYS, _META, _EXTRA)
    phi, mean, P, R, theta = arrays.values()
    S, k, L = meta.pop("n_states"), meta.pop("n_components"), meta["latent_dim"]
    ok = 1 <= S <= S_MAX and 1 <= k <= K_MAX and k <= L <= L_MAX
    if (not ok or phi.shape != (phi_layout(S, k)[1],) or theta.shape != (theta_layout(S, k)[1],) or mean.shape != (L,)
            or P.shape != (k, L) or R.shape != (k, L) or any(np.asarray(extra[n]).shape != (S,) for n in _EXTRA[:3])):
        raise ValueError("%s: phi %s, theta %s, mean %s, whiten %s and unwhiten %s do not fit %d states, %d components and "
                         "latent_dim %d" % (path, phi.shape, theta.shape, mean.shape, P.shape, R.shape, S, k, L))
    dev = torch.device(device)
    phi, mean, P, R, theta = (torch.from_numpy(a).to(dev) for a in (phi, mean, P, R, theta))
    states = LatentStates(S, k, float(extra["var_floor"]))._set(theta, mean, P, meta["n_frames"], meta["n_files"])
    sw = SwitchingWalk(states)._set(phi, mean, P, R, extra["pairs"], extra["shrink"], extra["flags"], meta["n_frames"],
                                    meta["n_files"])
    return sw, meta


class StreamingSwitchingWalk(GraphReplay):
    """`n_streams` independent switching walks decoded block by block through a `VAE` on the GPU (see the module doc).

    `temperature` [n_streams], `offset` [n_streams, L] and `forced` [n_streams, block // hop] int32 (-1: free) may be
    written in place between calls; a captured graph reads them.  A stream that is not primed draws its first state from
    pi and its first u from N(0, I)."""

    def __init__(self, model, sw, n_streams, block, hop=None, window=None, seed=0):
        if not isinstance(sw, SwitchingWalk):
            raise TypeError("StreamingSwitchingWalk needs a fitted SwitchingWalk, got %s" % type(sw).__name__)
        sw._fitted()
        self.stream = sv = StreamingVAE(model, n_streams, block, hop, window, seed)
        self.model, self.sw = model, sw
        self.S, self.H, self.L, self.hop, self.device = sv.S, sv.H, sv.L, sv.hop, sv.device
        self.n_streams, self.block, self.window, self.seed = sv.n_streams, sv.block, window, sv.seed
        self.frames_per_block = F = sv.frames_per_block
        self.k, self.n_states = sw.n_components, sw.n_states
        if sw.mean_.numel() != self.L:
            raise ValueError("the switching walk was fitted on %d-dimensional latents, the model has latent_dim %d" % (
                sw.mean_.numel(), self.L))
        if sw.mean_.device != self.device:
            raise RvError("the switching walk is on %s; the model computes on %s" % (sw.mean_.device, self.device))
        self.temperature, self.offset = sv.temperature, sv.offset
        dev = self.device
        self._state = torch.zeros((self.n_streams, self.k), dtype=torch.float64, device=dev)
        self._primed = torch.zeros(self.n_streams, dtype=torch.int32, device=dev)
        self._current = torch.zeros(self.n_streams, dtype=torch.int32, device=dev)
        self._path = torch.full((self.n_streams, F), -1, dtype=torch.int32, device=dev)
        self.forced = torch.full((self.n_streams, F), -1, dtype=torch.int32, device=dev)
        self._z = torch.zeros((self.n_streams * F, self.L), dtype=torch.float32, device=dev)
        self._silence = torch.zeros((self.n_streams, self.block), dtype=torch.float32, device=dev)

    def parameters(self):
        return self.stream.parameters()

    def _step(self, x, y, eps, uniforms, forced, stream):
        sd = self.stream.desc(x, y, eps)
        w = self.sw
        _call(_lib.SWITCH_STEP, stream, live=C.pointer(sd), S=self.n_states, k=self.k, L=self.L, ldo=self.L, centre=ptr(w.mean_),
              basis=ptr(w.R_), moment=ptr(w.phi_), out=ptr(self._z), state=ptr(self._state), primed=ptr(self._primed),
              idx=ptr(self._current), path=ptr(self._path), next_of=ptr(forced), weight=ptr(uniforms))

    def _check(self, t, dtype, shape, what):
        if not torch.is_tensor(t) or t.dtype != dtype or t.device != self.device or tuple(t.shape) != shape:
            raise ValueError("%s has shape %s, expected a %s tensor %s on %s" % (
                what, "%s %s on %s" % (t.dtype, tuple(t.shape), t.device) if torch.is_tensor(t) else type(t).__name__,
                str(dtype).replace("torch.", ""), shape, self.device))
        return t.contiguous()

    @torch.no_grad()
    def generate(self, eps=None, uniforms=None, states=None):
        """One block of every stream -> [n_streams, block] fp32.  eps: None (Philox) or [n_streams, F, k] fp32 standard-normal
        draws; uniforms: None (Philox) or [n_streams, F] fp32 in [0, 1); states: None (the `forced` tensor as it stands) or
        [n_streams, F] int32 forced states, -1 = free, copied into `forced`.  F = block // hop."""
        F = self.frames_per_block
        if eps is not None:
            eps = self._check(eps, torch.float32, (self.n_streams, F, self.k), "eps")
        if uniforms is not None:
            uniforms = self._check(uniforms, torch.float32, (self.n_streams, F), "uniforms")
        if states is not None:
            self.forced.copy_(self._check(states, torch.int32, (self.n_streams, F), "states"))
        y = torch.empty((self.n_streams, self.block), dtype=torch.float32, device=self.device)
        self._step(self._silence, y, eps, uniforms, self.forced, None)
        return y

    @torch.no_grad()
    def reset(self, streams=None):
        """Zero the overlap-add tail, the frame counter and the state of `streams` (an index or a list; None = all) and clear
        their primed flags: the next frame draws its state from pi and u from N(0, I)."""
        self.stream.reset(streams)
        for s in each_stream(streams, self.n_streams):
            sel = slice(None) if s < 0 else s
            self._state[sel] = 0
            self._primed[sel] = 0
            self._current[sel] = 0

    @torch.no_grad()
    def set_state(self, u, s, streams=None):
        """Set the standardised state of `streams` (None = all, in order) to the rows of u [len(streams), k] and their HMM
        state to s [len(streams)] (integers in [0, S)), and set their primed flags."""
        which = list(range(self.n_streams)) if streams is None else [i for i in each_stream(streams, self.n_streams)]
        if not torch.is_tensor(u) or u.device != self.device or not u.is_floating_point():
            raise ValueError("u must be a floating-point tensor on %s" % self.device)
        if u.dim() == 1:
            u = u.view(1, -1)
        if tuple(u.shape) != (len(which), self.k):
            raise ValueError("u has shape %s, expected %s" % (tuple(u.shape), (len(which), self.k)))
        s = [int(v) for v in (s.reshape(-1).tolist() if torch.is_tensor(s) else np.asarray(s).reshape(-1))]
        if len(s) != len(which) or any(not 0 <= v < self.n_states for v in s):
            raise ValueError("s=%r: expected %d states in [0, %d)" % (s, len(which), self.n_states))
        for row, i in enumerate(which):
            self._state[i] = u[row].to(torch.float64)
            self._current[i] = s[row]
            self._primed[i] = 1

    @torch.no_grad()
    def prime(self, x_row, streams=None):
        """Start `streams` from a latent row x [L] fp32: s = the argmax of the frame's emission, u = (y - m_s) / sd_s.
        Returns s."""
        sw = self.sw
        x = torch.as_tensor(x_row, dtype=torch.float32, device=self.device).reshape(1, self.L).contiguous()
        logb = emit(x, sw.mean_, sw.P_, sw.states.theta_, self.n_states)
        s = int(torch.argmax(logb[0]))
        y = (sw.P_ @ (x[0].double() - sw.mean_))
        o, _ = phi_layout(self.n_states, self.k)
        m, sd = sw.phi_[o["m"]].view(-1, self.k)[s], sw.phi_[o["sd"]].view(-1, self.k)[s]
        n = self.n_streams if streams is None else len(list(each_stream(streams, self.n_streams)))
        self.set_state(((y - m) / sd).view(1, -1).expand(n, -1), [s] * n, streams)
        return s

    @property
    def state(self):
        """The standardised state u [n_streams, k] fp64 after the last frame (the tensor the launches read and write)."""
        return self._state

    def current_states(self):
        """The HMM state of every stream after the last frame [n_streams] int32"""
        return self._current

    def last_states(self):
        """The states of the last call's frames [n_streams, block // hop] int32"""
        return self._path

    def last_latents(self):
        """The latent rows z of the last call's frames as a view [n_streams, block // hop, L]."""
        return self._z.view(self.n_streams, self.frames_per_block, self.L)

    @torch.no_grad()
    def capture(self):
        """Capture one block (eps and uniforms from Philox, the forced states read from `forced`) as a graph; `replay()`
        then generates one block per call into `graph_output` [n_streams, block]."""
        return self._capture(lambda st: self._step(self.graph_input, self.graph_output, None, None, self.forced, st))

    @torch.no_grad()
    def replay(self):
        """One block through the captured graph on the current stream.  Returns `graph_output` (overwritten by the next
        replay)."""
        return self._replay(0, "replay()")
