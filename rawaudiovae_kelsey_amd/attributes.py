"""Latent attributes: audio descriptors of every frame, and the latent directions that move them (the RV_ATTR_* ops of
rv_mosaic; the rules: include/rawvae_hip.h, "Latent attributes").

A descriptor is a property of the sound of one frame: its level, zero-crossing rate, crest factor, spectral centroid and
spectral flatness.  Regressed on the whitened principal coordinates y = P (x - c) of a corpus's latents, each becomes a
direction of the latent space, and "centroid +0.02, level -3 dB, hold the rest" becomes one offset [L] that
StreamingVAE.offset and `resynth.py --offset` take.  The model is linear and may fit a raw-waveform latent badly: R^2 says
how well the latents explain a descriptor, `response` what the decoder actually did with an offset.

  describe(padded, T, S, hop, window, dynamic_range, out)      desc [T, 5 or 3] fp64                     RV_ATTR_DESCRIBE
  fit_targets(x, targets, pca, n_components, ridge)            the raw fit: (parts of the result, info)  RV_ATTR_FIT
  LatentAttributes(names).fit(x, targets, pca, n_components, ridge)
      B_ [N, k], mean_, std_, r2_ [N], corr_ [N, N], R_ [k, L] (rows sqrt(lambda_j) v_j), n_observed_, n_frames_ (numpy)
      .move(moves, hold) -> (offset [L] fp32 device tensor, predicted [N], norm)
      .response(codec, mu, offset, S, window) -> the mean achieved change of every descriptor
  fit_corpus(model, waves, hop, pca, ...)                      the built-in descriptors of a corpus against its mu
  write_attributes(path, attrs, segment_length, hop) / read_attributes(path)      one .npz

x [T, L] fp32 on the device; its rows may have a pitch.  targets [T, N] fp64 on the device.  A frame whose x row or
target row holds a value that is not finite (a silent frame's level is -inf) is unobserved and takes no part in the fit.
"""
import numpy as np
import torch

from . import _lib
from ._lib import RvError, mosaic_call as _call, ptr
from .corpus import encode_corpus, read_fitted, write_fitted
from .evaluate import R_MAX, SPECTRAL_S, _spectral_ok, twiddle_table
from .pca import LatentPCA
from .stream import window_values
from .walk import check_components, rank_of

NAMES = ("level", "zcr", "crest", "centroid", "flatness")
K_MAX, N_MAX, L_MAX = 64, 64, 512    # csrc/attr.hip
COND_MAX = 1e12                      # of M M^T in move
_STATUS = {1: "fewer than n_components + 2 frames are observed (finite in x and in the targets)",
           2: "the covariance of the whitened latents is not positive definite: a pivot of its Cholesky factor was not "
              "positive (keep fewer components or give a ridge > 0)"}


def tables(S, window, device):
    """(window [S], twiddles [S]) fp32 on the device for describe, or (None, None) without a window."""
    if window is None:
        return None, None
    if not _spectral_ok(int(S)):
        raise ValueError("window %r: the spectral descriptors need segment_length a power of two in [%d, %d], got %d "
                         "(window=None describes without them)" % (window, SPECTRAL_S[0], SPECTRAL_S[1], S))
    return (torch.from_numpy(window_values(S, window)).to(device), torch.from_numpy(twiddle_table(S)).to(device))


def describe(padded, T, S, hop, window="hann", dynamic_range=60.0, out=None, table=None, stream=None):
    """desc [T, 5] fp64 (NAMES) of the frames padded[t * hop : t * hop + S], or [T, 3] (level, zcr, crest) with
    window=None: RV_ATTR_DESCRIBE.  padded: a contiguous fp32 device tensor read flat.  window: None, "hann" or a [S] fp32
    device tensor that comes with its twiddle `table` (evaluate.twiddle_table).  out: a [T, ldo] fp64 tensor (or a row
    slice of one) to write into; only its first 5 (3) columns are written.  stream: the raw hipStream_t (None: the current
    stream); with window and table tensors and `out` given the call allocates and copies nothing, so it may be captured."""
    if (not torch.is_tensor(padded) or padded.dtype != torch.float32 or padded.device.type != "cuda"
            or not padded.is_contiguous()):
        raise ValueError("padded must be a contiguous float32 device tensor")
    flat = padded.view(-1)
    T, S, hop = int(T), int(S), int(hop)
    if T < 1 or S < 1 or hop < 1 or (T - 1) * hop + S > flat.numel():
        raise ValueError("%d frames of %d samples at hop %d do not fit the %d samples given" % (T, S, hop, flat.numel()))
    if not 0 < float(dynamic_range) <= R_MAX:
        raise ValueError("dynamic_range=%r must be a number of dB in (0, %g]" % (dynamic_range, R_MAX))
    if torch.is_tensor(window):
        if table is None or window.numel() != S or table.numel() != S or not _spectral_ok(S):
            raise ValueError("a window tensor must hold %d values, a power of two in [%d, %d], and come with its twiddle "
                             "table" % (S, SPECTRAL_S[0], SPECTRAL_S[1]))
        win, tw = window.contiguous(), table.contiguous()
    else:
        win, tw = tables(S, window, flat.device)
    cols = 3 if win is None else 5
    if out is None:
        out = torch.empty((T, cols), dtype=torch.float64, device=flat.device)
    if (not torch.is_tensor(out) or out.dtype != torch.float64 or out.device != flat.device or out.dim() != 2
            or out.shape[0] != T or out.shape[1] < cols or out.stride(1) != 1):
        raise ValueError("out must be a [%d, >= %d] float64 tensor on %s with unit column stride" % (T, cols, flat.device))
    _call(_lib.ATTR_DESCRIBE, stream, T=T, S=S, hop=hop, frames=ptr(flat), n_out=flat.numel(), window=ptr(win), twiddles=ptr(tw),
          dynamic_range=float(dynamic_range), result=ptr(out), ldo=out.stride(0) if T > 1 else max(out.shape[1], cols))
    return out


def result_layout(k, N):
    """{part: slice} of result = [n | ybar (k) | dbar (N) | Cdd (N N) | B (N k) | r2 (N)] and its length"""
    o, at = {}, 0
    for name, n in (("n", 1), ("ybar", k), ("dbar", N), ("Cdd", N * N), ("B", N * k), ("r2", N)):
        o[name] = slice(at, at + n)
        at += n
    return o, at


def workspace(T, k, N, device):
    """(ws, bytes) of RV_ATTR_FIT at (T, k, N)"""
    n = _call(_lib.ATTR_WORKSPACE, T=int(T), k=int(k), N=int(N)).ws_bytes
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device), n


def axes(pca, n_components=None, device=None):
    """(centre [L], P [k, L] fp64 on the device, R [k, L] numpy) of a fitted LatentPCA -- P's rows v_j / sqrt(lambda_j), R's
    sqrt(lambda_j) v_j, k = n_components or every axis of positive variance, 64 at most -- or of a (centre, P) pair, whose
    R = pinv(P)^T.  ValueError naming n_components."""
    if isinstance(pca, LatentPCA):
        pca._fitted()
        lam = pca.explained_variance_.cpu().numpy()
        rank = min(rank_of(pca.all_variances_.cpu().numpy()), lam.size)
        k = check_components(n_components, rank)
        if k > K_MAX:
            if n_components is not None:
                raise ValueError("n_components=%d: the attribute fit takes at most %d axes" % (k, K_MAX))
            k = K_MAX      # the corpus has more usable axes than the fit takes: the leading 64
        comp = pca.components_[:k].cpu().numpy()
        root = np.sqrt(lam[:k])[:, None]
        centre, P, R = pca.mean_, torch.from_numpy(comp / root).to(pca.mean_.device), comp * root
    elif isinstance(pca, (tuple, list)) and len(pca) == 2:
        centre, P = (t if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)) for t in pca)
        if P.dim() != 2 or centre.dim() != 1 or P.shape[1] != centre.numel():
            raise ValueError("the basis holds P %s and centre %s" % (tuple(P.shape), tuple(centre.shape)))
        k = P.shape[0] if n_components is None else int(n_components)
        if not 1 <= k <= min(P.shape[0], K_MAX):
            raise ValueError("n_components=%d: the basis holds %d axes and the attribute fit takes at most %d" % (
                k, P.shape[0], K_MAX))
        P = P[:k]
        R = np.linalg.pinv(P.cpu().numpy().astype(np.float64)).T
        if device is not None:
            centre, P = centre.to(device), P.to(device)
    else:
        raise TypeError("expected a fitted LatentPCA or a (centre, P) pair, got %s" % type(pca).__name__)
    return centre.to(torch.float64).contiguous(), P.to(torch.float64).contiguous(), np.ascontiguousarray(R)


def _latents(x):
    if (not torch.is_tensor(x) or x.dim() != 2 or x.dtype != torch.float32 or x.device.type != "cuda" or x.shape[0] < 2
            or x.shape[1] < 1):
        raise ValueError("x must be a 2-D float32 device tensor with at least two rows, got %s" % (
            "%s %s on %s" % (x.dtype, tuple(x.shape), x.device) if torch.is_tensor(x) else type(x).__name__))
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    return x, x.stride(0)


def fit_targets(x, targets, pca, n_components=None, ridge=0.0, out=None, ws=None, stream=None):
    """The regression of targets [T, N] fp64 on y = P (x - c): RV_ATTR_FIT.  Returns ({n, ybar, dbar, Cdd [N, N], B [N, k],
    r2}: fp64 device views of the result block, info [2] int32 = {status, n}, R [k, L] numpy).  Nothing is read back: the
    caller looks at info.  out: (result, info) to write into; ws: workspace()'s pair.  pca: a fitted LatentPCA, a (centre, P)
    pair or the triple axes() returned; with that triple, out and ws given the call allocates and copies nothing, so it may be
    captured on `stream` (the raw hipStream_t; None: the current stream)."""
    x, ldx = _latents(x)
    T, L = x.shape
    if (not torch.is_tensor(targets) or targets.dim() != 2 or targets.dtype != torch.float64 or targets.device != x.device
            or targets.shape[0] != T or not 1 <= targets.shape[1] <= N_MAX):
        raise ValueError("targets must be a [%d, 1..%d] float64 tensor on %s, got %s" % (
            T, N_MAX, x.device, "%s %s on %s" % (targets.dtype, tuple(targets.shape), targets.device)
            if torch.is_tensor(targets) else type(targets).__name__))
    targets = targets.contiguous()
    N = targets.shape[1]
    if not (isinstance(ridge, (int, float)) and 0 <= ridge < float("inf")):
        raise ValueError("ridge=%r must be a finite number >= 0" % (ridge,))
    centre, P, R = pca if isinstance(pca, tuple) and len(pca) == 3 else axes(pca, n_components, x.device)
    k = P.shape[0]
    if centre.numel() != L or centre.device != x.device:
        raise ValueError("the basis was fitted on %d-dimensional latents on %s, x is %s on %s" % (
            centre.numel(), centre.device, tuple(x.shape), x.device))
    if not k <= L <= L_MAX:
        raise ValueError("n_components=%d: the latents have %d dimensions (at most %d)" % (k, L, L_MAX))
    parts, n_res = result_layout(k, N)
    res, info = out if out is not None else (torch.empty(n_res, dtype=torch.float64, device=x.device),
                                             torch.empty(2, dtype=torch.int32, device=x.device))
    if res.dtype != torch.float64 or res.numel() != n_res or not res.is_contiguous():
        raise ValueError("the result must be %d contiguous float64 values" % n_res)
    ws, nb = workspace(T, k, N, x.device) if ws is None else ws
    _call(_lib.ATTR_FIT, stream, T=T, L=L, k=k, N=N, q=ptr(x), stride=ldx, centre=ptr(centre), basis=ptr(P), moment=ptr(targets),
          lam=float(ridge), result=ptr(res), info=ptr(info), ws=ptr(ws), ws_bytes=nb)
    flat = res.view(-1)
    views = {name: flat[s] for name, s in parts.items()}
    views["Cdd"], views["B"] = views["Cdd"].view(N, N), views["B"].view(N, k)
    return views, info, R


def parse_moves(moves, names):
    """{index: delta} of {name: delta}; ValueError naming an unknown descriptor or a delta that is not finite."""
    out = {}
    for name, delta in dict(moves).items():
        if name not in names:
            raise ValueError("unknown descriptor %r: the fit holds %s" % (name, ", ".join(names)))
        delta = float(delta)
        if not np.isfinite(delta):
            raise ValueError("descriptor %r: the move must be finite, got %r" % (name, delta))
        out[names.index(name)] = delta
    return out


class LatentAttributes:
    """The fitted directions (see the module doc).  The fit runs on the device; what it leaves is small and lives on the
    host as float64 numpy arrays, and move() solves its N x N system there."""

    def __init__(self, names=NAMES):
        names = tuple(str(n) for n in names)
        if not 1 <= len(names) <= N_MAX or len(set(names)) != len(names) or any(not n or "," in n or ":" in n for n in names):
            raise ValueError("names=%r: expected 1 to %d distinct names without ',' or ':'" % (names, N_MAX))
        self.names = names
        self.B_ = None

    def _set(self, B, mean, std, r2, corr, R, n_observed, n_frames, ridge=0.0, device="cpu"):
        N = len(self.names)
        B, R = np.asarray(B, dtype=np.float64), np.asarray(R, dtype=np.float64)
        mean, std, r2 = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (mean, std, r2))
        corr = np.asarray(corr, dtype=np.float64)
        if (B.ndim != 2 or B.shape[0] != N or R.ndim != 2 or R.shape[0] != B.shape[1] or mean.shape != (N,)
                or std.shape != (N,) or r2.shape != (N,) or corr.shape != (N, N)):
            raise ValueError("B %s, mean %s, std %s, r2 %s, corr %s and R %s do not fit %d descriptors" % (
                B.shape, mean.shape, std.shape, r2.shape, corr.shape, R.shape, N))
        self.B_, self.mean_, self.std_, self.r2_, self.corr_, self.R_ = B, mean, std, r2, corr, R
        self.n_observed_, self.n_frames_, self.ridge, self.device_ = int(n_observed), int(n_frames), float(ridge), torch.device(device)
        return self

    def _fitted(self):
        if self.B_ is None:
            raise RuntimeError("LatentAttributes has not been fitted")

    @torch.no_grad()
    def fit(self, x, targets, pca, n_components=None, ridge=0.0):
        """Fit on x [T, L] and targets [T, N] (N = len(names)) in the axes of a fitted LatentPCA (or a (centre, P) pair).
        RvError naming the cause when too few frames are observed or the covariance is singular."""
        if torch.is_tensor(targets) and targets.dim() == 2 and targets.shape[1] != len(self.names):
            raise ValueError("targets has %d columns for the %d names %s" % (targets.shape[1], len(self.names), ", ".join(self.names)))
        parts, info, R = fit_targets(x, targets, pca, n_components, ridge)
        status, n = (int(v) for v in info.cpu().numpy())      # the one read of the fit
        if status:
            raise RvError("LatentAttributes.fit: %s (%d of %d frames observed, %d components)" % (
                _STATUS.get(status, "status %d" % status), n, x.shape[0], R.shape[0]))
        host = {name: t.cpu().numpy() for name, t in parts.items()}
        std = np.sqrt(np.diag(host["Cdd"]))
        with np.errstate(all="ignore"):
            corr = host["Cdd"] / np.outer(std, std)
        return self._set(host["B"], host["dbar"], std, host["r2"], corr, R, n, x.shape[0], ridge, x.device)

    def move(self, moves, hold=False):
        """(offset [L] fp32 on the fit's device, predicted [N], norm) of `moves` = {name: change}.  The smallest step w in
        whitened coordinates (|w| = norm, in corpus standard deviations) with M w = delta, M = the rows of B_ of the moved
        descriptors and -- hold -- of all the others at change 0: w = M^T (M M^T)^-1 delta, offset = R_^T w, predicted =
        B_ w.  ValueError naming the descriptors when M M^T has a condition number above 1e12."""
        self._fitted()
        wanted = parse_moves(moves, self.names)
        rows = sorted(wanted) + ([i for i in range(len(self.names)) if i not in wanted] if hold else [])
        k = self.B_.shape[1]
        w = np.zeros(k)
        if rows:
            M = self.B_[rows]
            delta = np.array([wanted.get(i, 0.0) for i in rows])
            gram = M @ M.T
            with np.errstate(all="ignore"):
                cond = np.linalg.cond(gram) if np.isfinite(gram).all() else np.inf
            if not cond <= COND_MAX:
                raise ValueError("the directions of %s cannot be set apart: M M^T has condition number %.3g (above %g); "
                                 "move fewer of them together or drop hold" % (
                                     ", ".join(self.names[i] for i in rows), cond, COND_MAX))
            w = M.T @ np.linalg.solve(gram, delta)
        offset = torch.from_numpy((self.R_.T @ w).astype(np.float32)).to(self.device_)
        return offset, self.B_ @ w, float(np.sqrt(w @ w))

    @torch.no_grad()
    def response(self, codec, mu, offset, S, window="hann", dynamic_range=60.0):
        """What the decoder did with `offset`: mu and mu + offset decoded, both sets of frames described (hop = S), and
        the mean change of every descriptor over the frames whose descriptors are finite in both -> ([5 or 3] numpy,
        the number of those frames)."""
        S = int(S)
        T = mu.shape[0]
        base = describe(codec.decode(mu).view(-1), T, S, S, window, dynamic_range)
        moved = describe(codec.decode(mu + offset.to(mu.device, torch.float32)).view(-1), T, S, S, window, dynamic_range)
        both = torch.isfinite(base).all(dim=1) & torch.isfinite(moved).all(dim=1)
        n = int(both.sum())
        if n == 0:
            return np.full(base.shape[1], np.nan), 0
        return (moved[both] - base[both]).mean(dim=0).cpu().numpy(), n


@torch.no_grad()
def describe_corpus(codec, waves, hop=None, window="hann", dynamic_range=60.0):
    """desc [T, 5 or 3] fp64 of every frame of every waveform, padded and framed as corpus.encode_corpus frames them."""
    step = codec.S if hop is None else int(hop)
    out = []
    for w in waves:
        w = codec.wave(w)
        padded, T = codec.pad(w, w.numel(), hop)
        out.append(describe(padded, T, codec.S, step, window, dynamic_range))
    return torch.cat(out, 0) if len(out) > 1 else out[0]


@torch.no_grad()
def fit_corpus(model, waves, hop=None, pca=None, n_components=None, ridge=0.0, window="hann", dynamic_range=60.0,
               targets=None, names=None, max_rows=16384):
    """LatentAttributes of a corpus: the encoder's mu of every frame of every waveform (corpus.encode_corpus) against the
    descriptors of the same padded frames, or against the caller's `targets` [T, N] under `names`.  pca: a fitted LatentPCA
    of the same model (None: the corpus's own principal axes).  Returns (attrs, x, targets)."""
    from .codec import FrameCodec
    waves = list(waves)
    x, _ = encode_corpus(model, waves, hop, max_rows)
    if targets is None:
        targets = describe_corpus(FrameCodec(model, max_rows=max_rows), waves, hop, window, dynamic_range)
        names = NAMES[:targets.shape[1]] if names is None else names
    else:
        if not torch.is_tensor(targets):
            targets = torch.from_numpy(np.ascontiguousarray(targets, dtype=np.float64))
        targets = targets.to(x.device, torch.float64)
        if targets.dim() != 2 or targets.shape[0] != x.shape[0]:
            raise ValueError("targets %s: expected one row for each of the corpus's %d frames" % (tuple(targets.shape), x.shape[0]))
        names = tuple("t%d" % i for i in range(targets.shape[1])) if names is None else names
    attrs = LatentAttributes(names)
    attrs.fit(x, targets, LatentPCA().fit(x.contiguous()) if pca is None else pca, n_components, ridge)
    return attrs, x, targets


_ARRAYS = ("B", "mean", "std", "r2", "corr", "R")
_META = ("segment_length", "latent_dim", "hop", "n_frames", "n_observed", "n_components", "n_targets")


def write_attributes(path, attrs, segment_length, hop=None):
    """One .npz: B [N, k], mean, std, r2 [N], corr [N, N] and R [k, L], all fp64, names (an array of strings), ridge, and
    segment_length, latent_dim, hop (-1: non-overlapping frames), n_frames, n_observed, n_components, n_targets."""
    attrs._fitted()
    write_fitted(path, {n: torch.from_numpy(np.ascontiguousarray(a)) for n, a in zip(
        _ARRAYS, (attrs.B_, attrs.mean_, attrs.std_, attrs.r2_, attrs.corr_, attrs.R_))},
                 dict(segment_length=segment_length, latent_dim=attrs.R_.shape[1], hop=hop, n_frames=attrs.n_frames_,
                      n_observed=attrs.n_observed_, n_components=attrs.B_.shape[1], n_targets=attrs.B_.shape[0]),
                 names=np.asarray(attrs.names), ridge=float(attrs.ridge))


def read_attributes(path, device="cuda"):
    """(LatentAttributes whose offsets go to `device`, {segment_length, latent_dim, hop (None: non-overlapping), n_frames,
    n_observed}) of write_attributes' file; ValueError when the arrays do not fit one another."""
    arrays, meta, extra = read_fitted(path, "attributes", _ARRAYS, _META, ("names", "ridge"))
    names = tuple(str(n) for n in np.asarray(extra["names"]).reshape(-1))
    k, N, L = meta.pop("n_components"), meta.pop("n_targets"), meta["latent_dim"]
    B, R = arrays["B"], arrays["R"]
    if len(names) != N or B.shape != (N, k) or R.shape != (k, L) or not 1 <= k <= K_MAX or not k <= L <= L_MAX:
        raise ValueError("%s: %d names, B %s and R %s do not fit %d descriptors, %d components and latent_dim %d" % (
            path, len(names), B.shape, R.shape, N, k, L))
    try:
        attrs = LatentAttributes(names)._set(B, arrays["mean"], arrays["std"], arrays["r2"], arrays["corr"], R,
                                             meta["n_observed"], meta["n_frames"], float(extra["ridge"]), device)
    except ValueError as e:
        raise ValueError("%s: %s" % (path, e))
    return attrs, meta
