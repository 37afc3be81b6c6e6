"""Latent timbre transfer: entropic optimal transport between the latent clouds of two corpora (the RV_OT_* ops of
rv_mosaic; the rules: include/rawvae_hip.h, "Latent transport").

Both corpora are whitened into the first k principal coordinates y = P (x - c).  A Sinkhorn iteration finds the two dual
potentials f (source) and g (target) of the entropic plan between the clouds; the plan's barycentric map
T(y) = softmax_j(lw_j + (g_j - |y - v_j|^2) / eps) . V sends the source distribution onto the target distribution as a
whole, where a nearest-neighbour mosaic would collapse it onto the target's near edge.  The map needs the target cloud and
its potential only, so it runs on any new frame, offline or block by block between the stream's encoder and decoder.

  whiten(x, centre, P)                          (y [T, k] fp64, observed [T] int32)                    RV_OT_WHITEN
  softmin(A, B, hl, epsilon)                    one Sinkhorn half-step, [T] fp64                       RV_OT_SOFTMIN
  transport_map(x, block, V, gl, epsilon, k, amount)   (x' [T, L] fp32, state [T, 3 + k] fp64)         RV_OT_MAP
  workspace(T, N, k, device)                    (ws, bytes) that serves both at (T, N, k)              RV_OT_WORKSPACE
  displacement(transport, mu, coords, amount)   how far every row moved, squared, in whitened units
  LatentTransport(n_components, epsilon, iters, tol, level_iters, check_every).fit(xs, xt, basis)
      .map(x, amount, reverse) -> (x', diagnostics); f_, g_, epsilon_, err_history_, n_iter_, cost_
  write_transport(path, transport, segment_length, hop) / read_transport(path, device)
  transfer(model, wave, transport, hop, window, amount, reverse)      the offline path -> (waveform, diagnostics)
  StreamingTransport(model, transport, n_streams, block, hop, window, amount, reverse)   the live path (RV_OT_LIVE)

x [T, L] fp32 on the device; its rows may have a pitch.  A row that holds a value that is not finite is unobserved: it has
no weight in a fit and passes through a map unchanged.  epsilon is taken as float32 and widened once, here and on the
device.  One Sinkhorn iteration is two ops on one stream with no host sync; the error is read back every `check_every`
iterations, which is the iteration's one read-back.
"""
import numpy as np
import torch

from . import _lib
from ._lib import mosaic_call as _call, ptr
from .codec import FrameCodec
from .corpus import read_fitted, write_fitted
from .states import _count, _f64, _latents, whitening
from .stream import GraphReplay, StreamingVAE

K_MAX, L_MAX = 64, 512    # csrc/transport.hip


def _epsilon(value, what="epsilon"):
    """epsilon as the float32 the device reads, widened (ValueError unless finite and positive as a float32)"""
    try:
        with np.errstate(over="ignore"):
            e = float(np.float32(value))
    except (TypeError, ValueError):
        e = float("nan")
    if isinstance(value, bool) or not 0 < e < float("inf"):
        raise ValueError("%s=%r must be a finite positive number (as float32)" % (what, value))
    return e


def _latents_of(x, L):
    """_latents(x) of x with L columns"""
    x, ldx = _latents(x)
    if x.shape[1] != L:
        raise ValueError("x has %d columns, the basis was fitted on %d-dimensional latents" % (x.shape[1], L))
    return x, ldx


def _cloud(t, what, k=None):
    if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] < 1 or not 1 <= t.shape[1] <= K_MAX:
        raise ValueError("%s must be a float64 device tensor [rows >= 1, 1 <= k <= %d], got %s" % (
            what, K_MAX, tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))
    if k is not None and t.shape[1] != k:
        raise ValueError("%s has %d axes, expected %d" % (what, t.shape[1], k))
    return _f64(t, what, t.shape)


def workspace(T, N, k, device):
    """(ws, bytes): one workspace that serves softmin and transport_map at (T rows, N columns, k axes)"""
    n = _call(_lib.OT_WORKSPACE, T=_count(T, "T", (1 << 31) - 1), N=_count(N, "N", (1 << 31) - 1), k=_count(k, "k", K_MAX)).ws_bytes
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device), n


def basis_block(centre, P, W=None):
    """[centre (L) | P (k L)] or, with W [L, k], [centre | P | W] as one fp64 device tensor: the ops' `basis`"""
    k, L = P.shape
    P, centre = _f64(P, "P", (k, L)), _f64(centre, "centre", (L,))
    if not 1 <= k <= K_MAX or not k <= L <= L_MAX:
        raise ValueError("P %s: 1 <= k <= %d and k <= L <= %d" % (tuple(P.shape), K_MAX, L_MAX))
    parts = [centre, P.reshape(-1)]
    if W is not None:
        parts.append(_f64(W, "W", (L, k)).reshape(-1))
    return torch.cat(parts)


def whiten(x, centre, P, out=None):
    """(y [T, k] fp64, observed [T] int32) of x [T, L]: RV_OT_WHITEN.  centre [L] and P [k, L] fp64 on the device."""
    x, ldx = _latents(x)
    T, L = x.shape
    if not torch.is_tensor(P) or P.dim() != 2:
        raise ValueError("P must be a 2-D float64 device tensor")
    k = P.shape[0]
    block = basis_block(centre, _f64(P, "P", (k, L)))
    y, info = out if out is not None else (torch.empty((T, k), dtype=torch.float64, device=x.device),
                                           torch.empty(T, dtype=torch.int32, device=x.device))
    _call(_lib.OT_WHITEN, T=T, L=L, k=k, a=ptr(x), stride=ldx, basis=ptr(block), result=ptr(y), info=ptr(info))
    return y, info


def softmin(A, B, hl, epsilon, out=None, ws=None):
    """f [T] fp64 = -eps log sum_j exp(lw_j + (h_j - |A_i - B_j|^2) / eps): RV_OT_SOFTMIN.  A [T, k], B [N, k] and
    hl = [h (N) | lw (N)] fp64 on the device."""
    A = _cloud(A, "A")
    T, k = A.shape
    B = _cloud(B, "B", k)
    N = B.shape[0]
    hl = _f64(hl, "hl = [h | lw]", (2 * N,))
    eps = _epsilon(epsilon)
    f = torch.empty(T, dtype=torch.float64, device=A.device) if out is None else _f64(out, "out", (T,))
    ws, nb = workspace(T, N, k, A.device) if ws is None else ws
    _call(_lib.OT_SOFTMIN, T=T, N=N, k=k, basis=ptr(A), moment=ptr(B), centre=ptr(hl), lam=eps, result=ptr(f), ws=ptr(ws),
          ws_bytes=nb)
    return f


def _amount(amount, n, device, what="amount"):
    """amount as a float32 device tensor [n]: a finite number or such a tensor (ValueError / TypeError otherwise)"""
    if torch.is_tensor(amount):
        if amount.dtype != torch.float32 or amount.device.type != "cuda" or tuple(amount.shape) != (n,):
            raise ValueError("%s must be a float32 device tensor [%d], got %s %s on %s" % (
                what, n, amount.dtype, tuple(amount.shape), amount.device))
        return amount.contiguous()
    if isinstance(amount, bool) or not isinstance(amount, (int, float, np.integer, np.floating)):
        raise TypeError("%s must be a number or a float32 device tensor, got %s" % (what, type(amount).__name__))
    if not np.isfinite(float(amount)):
        raise ValueError("%s=%r must be finite" % (what, amount))
    return torch.full((n,), float(amount), dtype=torch.float32, device=device)


def transport_map(x, block, V, gl, epsilon, k, amount=None, out=None, state=None, ws=None):
    """(x' [T, L] fp32, state [T, 3 + k] fp64) of x [T, L]: RV_OT_MAP.  block = basis_block(centre, P, W), V [N, k] the
    target cloud, gl = [g (N) | lw (N)], amount: None (1), a number or a float32 device tensor [1].  A state row is
    [f, support, cbar, T_0 .. T_k-1]."""
    x, ldx = _latents(x)
    T, L = x.shape
    k = _count(k, "k", K_MAX)
    V = _cloud(V, "V", k)
    N = V.shape[0]
    block = _f64(block, "the basis block [centre | P | W]", (L + 2 * k * L,))
    gl = _f64(gl, "gl = [g | lw]", (2 * N,))
    eps = _epsilon(epsilon)
    alpha = None if amount is None else _amount(amount, 1, x.device)
    dev = x.device
    out = torch.empty((T, L), dtype=torch.float32, device=dev) if out is None else out
    if (not torch.is_tensor(out) or out.dtype != torch.float32 or out.device != dev or tuple(out.shape) != (T, L)
            or out.stride(1) != 1 or (T > 1 and out.stride(0) < L)):
        raise ValueError("out must be a float32 device tensor of shape %s with unit column stride" % ((T, L),))
    state = torch.empty((T, 3 + k), dtype=torch.float64, device=dev) if state is None else _f64(state, "state", (T, 3 + k))
    ws, nb = workspace(T, N, k, dev) if ws is None else ws
    _call(_lib.OT_MAP, T=T, N=N, L=L, k=k, a=ptr(x), stride=ldx, basis=ptr(block), moment=ptr(V), centre=ptr(gl), lam=eps,
          weight=ptr(alpha), out=ptr(out), ldo=out.stride(0) if T > 1 else L, state=ptr(state), ws=ptr(ws), ws_bytes=nb)
    return out, state


def diagnostics(state):
    """The columns of a state block as a dict of views: f, support, cbar [..] and coords [.., k]"""
    return dict(f=state[..., 0], support=state[..., 1], cbar=state[..., 2], coords=state[..., 3:])


def displacement(transport, mu, coords, amount=1.0):
    """[T] fp64: the squared distance every row of mu [T, L] moves in whitened units, |amount (T_i - y_i)|^2 (NaN for a row
    that was not mapped)"""
    y, _ = whiten(mu, transport.mean_, transport.P_)
    d = (coords.reshape(y.shape) - y) * float(amount)
    return (d * d).sum(dim=1)


def mean_cost(ys, obs_s, yt, obs_t):
    """The mean of |a_i - b_j|^2 over the observed pairs, on the host in float64 from the clouds' first and second moments"""
    a = np.asarray(ys, np.float64)[np.asarray(obs_s) != 0]
    b = np.asarray(yt, np.float64)[np.asarray(obs_t) != 0]
    return float((a * a).sum(axis=1).mean() + (b * b).sum(axis=1).mean() - 2.0 * (a.mean(axis=0) * b.mean(axis=0)).sum())


def schedule(epsilon, cost, level_iters):
    """[(eps_l as float32 widened, iterations)] of the epsilon-scaling levels above the target eps = epsilon * cost:
    eps_l = cost 2^-l while that exceeds the target"""
    target = _epsilon(epsilon * cost, "epsilon x the mean cost")
    levels, l = [], 0
    while cost * 2.0 ** -l > target and l < 64:
        levels.append((_epsilon(cost * 2.0 ** -l), int(level_iters)))
        l += 1
    return levels, target


def log_weights(obs):
    """lw [N] float64 (numpy): -log(the observed frames) on them, -inf elsewhere"""
    obs = np.asarray(obs) != 0
    n = int(obs.sum())
    if n < 1:
        raise ValueError("no frame of the cloud is observed (every row holds a value that is not finite)")
    return np.where(obs, -np.log(float(n)), -np.inf)


def unwhitening(P):
    """W [L, k] (numpy): the pseudo-inverse of P [k, L] on the kept axes, P^T (P P^T)^-1 -- for a PCA's P the columns
    v_d sqrt(lambda_d)"""
    P = np.asarray(P, np.float64)
    return np.ascontiguousarray(np.linalg.solve(P @ P.T, P).T)


class LatentTransport:
    """The fitted plan between a source and a target corpus (see the module doc), all on the clouds' device.

    After fit: mean_ [L], P_ [k, L], W_ [L, k]; ys_ [Ns, k] and yt_ [Nt, k] (the clouds); f_ [Ns] and g_ [Nt] (the
    potentials); lws_ and lwt_ (the log-weights); epsilon_ (the target epsilon as the device reads it), mean_cost_,
    err_history_ [(iteration, error)], err_, n_iter_, cost_ (the transport cost per frame in whitened units)."""

    def __init__(self, n_components, epsilon=0.05, iters=500, tol=1e-3, level_iters=10, check_every=10):
        self.n_components = _count(n_components, "n_components", K_MAX)
        if isinstance(epsilon, bool) or not isinstance(epsilon, (int, float)) or not 0 < epsilon < float("inf"):
            raise ValueError("epsilon=%r must be a finite positive number" % (epsilon,))
        if isinstance(tol, bool) or not isinstance(tol, (int, float)) or not 0 <= tol < float("inf"):
            raise ValueError("tol=%r must be a finite number >= 0" % (tol,))
        self.epsilon, self.tol = float(epsilon), float(tol)
        self.iters, self.check_every = _count(iters, "iters", 1 << 30), _count(check_every, "check_every", 1 << 30)
        if isinstance(level_iters, bool) or not isinstance(level_iters, (int, np.integer)) or level_iters < 0:
            raise ValueError("level_iters=%r must be an integer >= 0" % (level_iters,))
        self.level_iters = int(level_iters)
        self.f_ = None

    def _fitted(self):
        if self.f_ is None:
            raise RuntimeError("LatentTransport has not been fitted")

    def _set(self, mean, P, W, ys, yt, f, g, lws, lwt, epsilon, n_iter=0, err=float("nan"), history=(), cost=float("nan"),
             mean_cost=float("nan")):
        k = self.n_components
        L, Ns, Nt = mean.numel(), ys.shape[0], yt.shape[0]
        if not k <= L <= L_MAX:
            raise ValueError("n_components=%d: the latents have %d dimensions (at most %d)" % (k, L, L_MAX))
        self.mean_, self.P_, self.W_ = _f64(mean, "mean", (L,), None), _f64(P, "whiten", (k, L), None), _f64(W, "unwhiten", (L, k), None)
        self.ys_, self.yt_ = _f64(ys, "the source cloud", (Ns, k), None), _f64(yt, "the target cloud", (Nt, k), None)
        self.f_, self.g_ = _f64(f, "f", (Ns,), None), _f64(g, "g", (Nt,), None)
        self.lws_, self.lwt_ = _f64(lws, "the source log-weights", (Ns,), None), _f64(lwt, "the target log-weights", (Nt,), None)
        self.epsilon_ = _epsilon(epsilon)
        self.n_iter_, self.err_, self.cost_, self.mean_cost_ = int(n_iter), float(err), float(cost), float(mean_cost)
        self.err_history_ = [(int(i), float(e)) for i, e in history]
        self._block = self._fl = self._gl = None
        return self

    def _blocks(self):
        if self._block is None:
            self._block = basis_block(self.mean_, self.P_, self.W_)
            self._fl, self._gl = torch.cat([self.f_, self.lws_]), torch.cat([self.g_, self.lwt_])
        return self._block, self._fl, self._gl

    @torch.no_grad()
    def fit(self, xs, xt, basis=None):
        """Sinkhorn between the latent rows xs [Ns, L] (source) and xt [Nt, L] (target) in the axes of `basis`: a fitted
        LatentPCA or LatentWalk, a (centre, P) pair, or None, the PCA of the two clouds' union.  Returns err_history_."""
        from .pca import LatentPCA
        k = self.n_components
        xs, _ = _latents(xs)
        xt, _ = _latents_of(xt, xs.shape[1])
        if xt.device != xs.device:
            raise ValueError("xs is on %s, xt on %s" % (xs.device, xt.device))
        dev, L = xs.device, xs.shape[1]
        if not k <= L <= L_MAX:
            raise ValueError("n_components=%d: the latents have %d dimensions (at most %d)" % (k, L, L_MAX))
        if basis is None:
            both = torch.cat([xs, xt], 0)
            basis = LatentPCA().fit(both[torch.isfinite(both).all(dim=1)].contiguous())
        centre, P = whitening(basis, k, dev)
        if centre.numel() != L or centre.device != dev:
            raise ValueError("the basis was fitted on %d-dimensional latents on %s, x is %s on %s" % (
                centre.numel(), centre.device, tuple(xs.shape), dev))
        W = torch.from_numpy(unwhitening(P.cpu().numpy())).to(dev)
        ys, obs_s = whiten(xs, centre, P)
        yt, obs_t = whiten(xt, centre, P)
        lws, lwt = log_weights(obs_s.cpu().numpy()), log_weights(obs_t.cpu().numpy())
        cost = mean_cost(ys.cpu().numpy(), obs_s.cpu().numpy(), yt.cpu().numpy(), obs_t.cpu().numpy())
        if not 0 < cost < float("inf"):
            raise ValueError("the mean cost between the two clouds is %r: nothing to transport" % cost)
        levels, target = schedule(self.epsilon, cost, self.level_iters)
        Ns, Nt = ys.shape[0], yt.shape[0]
        fl = torch.cat([torch.zeros(Ns, dtype=torch.float64, device=dev), torch.from_numpy(lws).to(dev)])
        gl = torch.cat([torch.zeros(Nt, dtype=torch.float64, device=dev), torch.from_numpy(lwt).to(dev)])
        f, g = fl[:Ns], gl[:Nt]
        ws = workspace(max(Ns, Nt), max(Ns, Nt), k, dev)
        bt = np.exp(lwt)
        n_iter, history, err = 0, [], float("inf")

        def iterate(eps, check):
            prev = g.clone() if check else None
            softmin(ys, yt, gl, eps, out=f, ws=ws)
            softmin(yt, ys, fl, eps, out=g, ws=ws)
            if not check:
                return None
            with np.errstate(over="ignore", invalid="ignore"):
                d = np.where(bt > 0, np.abs(np.exp((prev.cpu().numpy() - g.cpu().numpy()) / eps) - 1.0), 0.0)
            return float((bt * d).sum())

        for eps, n in levels:
            for _ in range(n):
                iterate(eps, False)
                n_iter += 1
        for i in range(1, self.iters + 1):
            check = i % self.check_every == 0 or i == self.iters
            e = iterate(target, check)
            n_iter += 1
            if check:
                err = e
                history.append((n_iter, e))
                if e <= self.tol:
                    break
        self._set(centre, P, W, ys, yt, f.clone(), g.clone(), fl[Ns:].clone(), gl[Nt:].clone(), target, n_iter, err, history,
                  mean_cost=cost)
        state = transport_map(xs, self._blocks()[0], self.yt_, self._gl, target, k, amount=0.0)[1]
        cbar, a = state[:, 2].cpu().numpy(), np.exp(lws)
        self.cost_ = float((a[a > 0] * cbar[a > 0]).sum())
        return list(self.err_history_)

    @torch.no_grad()
    def map(self, x, amount=1.0, reverse=False, out=None):
        """(x' [T, L] fp32, diagnostics) of latent rows x: every row moved by `amount` of the way to its barycentric image
        in the target's cloud (reverse: in the source's, under the source's potential).  diagnostics: f, support, cbar
        [T] and coords [T, k], fp64 on the device."""
        self._fitted()
        x, _ = _latents_of(x, self.mean_.numel())
        if x.device != self.mean_.device:
            raise ValueError("the transport lives on %s, x is on %s" % (self.mean_.device, x.device))
        block, fl, gl = self._blocks()
        V, hl = (self.ys_, fl) if reverse else (self.yt_, gl)
        out, state = transport_map(x, block, V, hl, self.epsilon_, self.n_components, amount, out=out)
        return out, diagnostics(state)


_ARRAYS = ("mean", "whiten", "unwhiten", "source_cloud", "target_cloud", "source_potential", "target_potential",
           "source_logweight", "target_logweight")
_META = ("segment_length", "latent_dim", "hop", "n_components", "n_source", "n_target", "n_iter")


def write_transport(path, transport, segment_length, hop=None):
    """One .npz: the nine fp64 arrays of the plan, epsilon (the target, as the device reads it), rel_epsilon, err, cost,
    mean_cost, err_history, and segment_length, latent_dim, hop (-1: non-overlapping frames), n_components, n_source,
    n_target, n_iter."""
    t = transport
    t._fitted()
    write_fitted(path, dict(mean=t.mean_, whiten=t.P_, unwhiten=t.W_, source_cloud=t.ys_, target_cloud=t.yt_,
                            source_potential=t.f_, target_potential=t.g_, source_logweight=t.lws_, target_logweight=t.lwt_),
                 dict(segment_length=segment_length, latent_dim=t.mean_.numel(), hop=hop, n_components=t.n_components,
                      n_source=t.ys_.shape[0], n_target=t.yt_.shape[0], n_iter=t.n_iter_),
                 epsilon=float(t.epsilon_), rel_epsilon=float(t.epsilon), err=float(t.err_), cost=float(t.cost_),
                 mean_cost=float(t.mean_cost_), err_history=np.asarray(t.err_history_, dtype=np.float64).reshape(-1, 2))


def read_transport(path, device="cuda"):
    """(LatentTransport on `device`, {segment_length, latent_dim, hop (None: non-overlapping), n_source, n_target,
    n_iter}) of write_transport's file; ValueError when the arrays do not fit one another."""
    arrays, meta, extra = read_fitted(path, "transport", _ARRAYS, _META, ("epsilon", "rel_epsilon", "err", "cost", "mean_cost",
                                                                          "err_history"))
    k, L, Ns, Nt = meta.pop("n_components"), meta["latent_dim"], meta["n_source"], meta["n_target"]
    want = dict(mean=(L,), whiten=(k, L), unwhiten=(L, k), source_cloud=(Ns, k), target_cloud=(Nt, k), source_potential=(Ns,),
                target_potential=(Nt,), source_logweight=(Ns,), target_logweight=(Nt,))
    bad = [n for n in _ARRAYS if arrays[n].shape != want[n]]
    if not 1 <= k <= K_MAX or not k <= L <= L_MAX or Ns < 1 or Nt < 1 or bad:
        raise ValueError("%s: %s do not fit %d components, latent_dim %d and %d + %d frames" % (
            path, ", ".join("%s %s" % (n, arrays[n].shape) for n in bad) or "the counts", k, L, Ns, Nt))
    dev = torch.device(device)
    t = LatentTransport(k, float(extra["rel_epsilon"]))
    t._set(*(torch.from_numpy(arrays[n]).to(dev) for n in _ARRAYS), float(extra["epsilon"]), meta["n_iter"], float(extra["err"]),
           np.asarray(extra["err_history"], np.float64).reshape(-1, 2), float(extra["cost"]), float(extra["mean_cost"]))
    return t, meta


@torch.no_grad()
def transfer(model, wave, transport, hop=None, window=None, amount=1.0, reverse=False, max_rows=16384):
    """The offline path: the waveform framed and encoded (codec.FrameCodec), every latent row mapped, decoded and
    overlap-added (RV_MOSAIC_OLA) -> (1-D fp32 device tensor of the waveform's length, diagnostics); the diagnostics also
    hold the frames' latent rows before the map as `mu`."""
    from .mosaic import check_window, ola
    from .stream import window_values
    codec = FrameCodec(model, max_rows=max_rows)
    step = codec.S if hop is None else int(hop)
    w = codec.wave(wave)
    padded, T = codec.pad(w, w.numel(), hop)
    check_window(codec.S, step, window)
    mu, _ = codec.encode(padded, T, hop)
    z, diag = transport.map(mu, amount, reverse)
    frames = codec.decode(z)
    win = None if window is None else torch.from_numpy(window_values(codec.S, window)).to(codec.device)
    return ola(frames, step, w.numel(), win), dict(diag, mu=mu)


class StreamingTransport(GraphReplay):
    """Live timbre transfer of `n_streams` streams through a fitted LatentTransport (RV_OT_LIVE).

    `process(x)` -> y [n_streams, block], the input `latency` = S - hop samples late; the concatenated outputs equal
    `transfer(model, cat([zeros(latency), x]), transport, hop, window, amount, reverse)` bit for bit.  Device tensors that
    may be written in place between calls, also between replays of a captured graph: `amount` [n_streams], `scale` and
    `offset` [n_streams, L] (the mapped row is mu * scale + offset)."""

    def __init__(self, model, transport, n_streams, block, hop=None, window=None, amount=1.0, reverse=False):
        transport._fitted()
        # the framing, history, window tables and stream workspace are StreamingVAE's
        self._sv = StreamingVAE(model, n_streams, block, hop, window)
        self.transport, self.reverse = transport, bool(reverse)
        self.n_streams, self.block, self.window = self._sv.n_streams, self._sv.block, window
        self.hop, self.latency, self.frames_per_block = self._sv.hop, self._sv.latency, self._sv.frames_per_block
        self.S, self.L, self.device = self._sv.S, self._sv.L, self._sv.device
        if transport.mean_.numel() != self.L or transport.mean_.device != self.device:
            raise ValueError("the transport was fitted on %d-dimensional latents on %s, the model has %d on %s" % (
                transport.mean_.numel(), transport.mean_.device, self.L, self.device))
        self.scale, self.offset = self._sv.scale, self._sv.offset
        self.amount = _amount(amount, self.n_streams, self.device)
        self.k = transport.n_components
        block_, fl, gl = transport._blocks()
        self._basis, (self._V, self._hl) = block_, ((transport.ys_, fl) if self.reverse else (transport.yt_, gl))
        M = self.n_streams * self.frames_per_block
        self._state = torch.zeros((M, 3 + self.k), dtype=torch.float64, device=self.device)
        self._ws = None
        nbytes = self._call(_lib.OT_WORKSPACE, None, None).ws_bytes
        self._ws = torch.zeros(max(nbytes, 256), dtype=torch.uint8, device=self.device)
        self.reset()

    def _call(self, op, x, y, stream=None):
        sd = self._sv.desc(x, y, None)
        return _call(op, stream, N=self._V.shape[0], k=self.k, L=self.L, basis=ptr(self._basis), moment=ptr(self._V),
                     centre=ptr(self._hl), lam=self.transport.epsilon_, weight=ptr(self.amount), state=ptr(self._state),
                     ws=ptr(self._ws), ws_bytes=0 if self._ws is None else self._ws.numel(), live=_lib.C.pointer(sd))

    @torch.no_grad()
    def process(self, x):
        """One block: x [n_streams, block] fp32 on the device -> [n_streams, block]."""
        x = self.check_input(x)
        y = torch.empty((self.n_streams, self.block), dtype=torch.float32, device=self.device)
        self._call(_lib.OT_LIVE, x, y)
        return y

    @torch.no_grad()
    def reset(self, streams=None):
        """Zero the history, the overlap-add tail and the frame counter of `streams` (an index or a list; None = all)."""
        self._sv.reset(streams)

    def last_latents(self):
        """(mu, logvar) of the last block's frames as views [n_streams, F, L], before `scale`, `offset` and the map."""
        return self._sv.last_latents()

    def last_diagnostics(self):
        """f, support, cbar [n_streams, F] and coords [n_streams, F, k] of the last block's frames, views of a static buffer"""
        return diagnostics(self._state.view(self.n_streams, self.frames_per_block, 3 + self.k))

    @torch.no_grad()
    def capture(self):
        """Capture one call as a graph on static buffers `graph_input` / `graph_output` [n_streams, block]; `replay(x)`
        then runs one block per call.  The graph reads `amount`, `scale` and `offset` where they are: writing them in place
        changes the next replay."""
        return self._capture(lambda st: self._call(_lib.OT_LIVE, self.graph_input, self.graph_output, stream=st))

    def parameters(self):
        return self._sv.parameters()

    def check_input(self, x):
        return self._sv.check_input(x)

    @torch.no_grad()
    def replay(self, x=None):
        """One block through the captured graph on the current stream; x (optional) is copied into `graph_input` first.
        Returns `graph_output` (overwritten by the next replay)."""
        return self._replay(0, "replay()", x)
