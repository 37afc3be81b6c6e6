"""Principal axes of a corpus's latents on the device, and edits along them (the RV_PCA_* ops of rv_mosaic; the rules:
include/rawvae_hip.h, "Latent PCA").

  moments(x)                        (centre [L], cov [L, L]) fp64 of x [N, L] fp32: column means and the sample
                                    covariance with ddof = 1, bit-identical from run to run
  eig(cov)                          (eigenvalues [L] descending, components [L, L] with row j the j-th unit eigenvector,
                                    sweeps, converged) by the one-workgroup cyclic Jacobi
  project / reconstruct / edit      rows to coordinates, coordinates to rows, and x + sum_j ((g_j - 1) y_j +
                                    h_j sqrt(lambda_j)) v_j with gains g and shifts h (in standard deviations) on the device
  LatentPCA(n_components).fit(x)    the two ops above, then mean_, components_, explained_variance_, ... and
                                    transform / inverse_transform / edit / offset
  fit_corpus(model, waves, hop)     every waveform's mu through codec.FrameCodec, fitted on all frames
  write_pca(path, pca, ...) / read_pca(path)   one .npz of fp64 arrays and the framing they were fitted at

Everything is computed by the library's kernels in fp64; nothing syncs, and the three apply forms may be captured in a
graph (the gains and shifts are device tensors, so a replay sees their updates).
"""
import numpy as np
import torch

from . import _lib
from ._lib import RvError, mosaic_call as _call, ptr
from .corpus import encode_corpus, read_fitted, rows as _rows, write_fitted

L_MAX = 512     # csrc/pca.hip


def _vector(v, what, n, dtype, device):
    name = {torch.float32: "float32", torch.float64: "float64"}[dtype]
    if not torch.is_tensor(v) or v.dim() != 1 or v.dtype != dtype or v.device != device or v.numel() != n:
        raise ValueError("%s must be a %s device tensor of %d values on %s, got %s" % (
            what, name, n, device,
            "%s %s on %s" % (v.dtype, tuple(v.shape), v.device) if torch.is_tensor(v) else type(v).__name__))
    return v.contiguous()


def workspace_bytes(N, L):
    """Bytes of device workspace of eig at L and, with N >= 2, of moments at (N, L) (N = 0: eig only)."""
    return _call(_lib.PCA_WORKSPACE, T=int(N), L=int(L)).ws_bytes


def _workspace(N, L, device):
    n = workspace_bytes(N, L)
    return torch.empty(max(n, 1), dtype=torch.uint8, device=device), n


def moments(x):
    """(centre [L] fp64, cov [L, L] fp64) of x [N, L] fp32, N >= 2: RV_PCA_MOMENTS."""
    x = _rows(x)
    N, L = x.shape
    if N < 2 or L > L_MAX:
        raise ValueError("x %s: needs at least 2 rows and at most %d columns" % (tuple(x.shape), L_MAX))
    centre = torch.empty(L, dtype=torch.float64, device=x.device)
    cov = torch.empty((L, L), dtype=torch.float64, device=x.device)
    ws, n = _workspace(N, L, x.device)
    _call(_lib.PCA_MOMENTS, T=N, L=L, q=ptr(x), ws=ptr(ws), ws_bytes=n, centre=ptr(centre), basis=ptr(cov))
    return centre, cov


def eig(cov):
    """(eigenvalues [L] fp64 descending, components [L, L] fp64 with row j the j-th unit eigenvector, sweeps,
    converged) of a symmetric cov [L, L] fp64: RV_PCA_EIG on a copy.  Reading sweeps and converged syncs."""
    cov = _rows(cov, "cov", torch.float64)
    L = cov.shape[0]
    if cov.shape[1] != L or L > L_MAX:
        raise ValueError("cov %s: expected a square matrix of at most %d rows" % (tuple(cov.shape), L_MAX))
    comp = cov.clone()
    lam = torch.empty(L, dtype=torch.float64, device=cov.device)
    info = torch.empty(2, dtype=torch.int32, device=cov.device)
    ws, n = _workspace(0, L, cov.device)
    _call(_lib.PCA_EIG, L=L, ws=ptr(ws), ws_bytes=n, basis=ptr(comp), eigenvalues=ptr(lam), info=ptr(info))
    sweeps, converged = (int(v) for v in info.cpu())
    return lam, comp, sweeps, bool(converged)


def _basis(components, centre, eigenvalues=None):
    comp = _rows(components, "components", torch.float64)
    k, L = comp.shape
    if k > L or L > L_MAX:
        raise ValueError("components %s: expected [k, L] with k <= L <= %d" % (tuple(comp.shape), L_MAX))
    centre = _vector(centre, "centre", L, torch.float64, comp.device)
    if eigenvalues is not None:
        eigenvalues = _vector(eigenvalues, "eigenvalues", k, torch.float64, comp.device)
    return comp, centre, eigenvalues, k, L


def _apply(mode, x, width, k, L, out, ldo, **roles):
    if x.device.index != roles["basis"].device.index:
        raise ValueError("the rows are on %s, the components on %s" % (x.device, roles["basis"].device))
    T = x.shape[0]
    if out is None:
        ldo = width if ldo is None else int(ldo)
        out = torch.empty((T, ldo), dtype=torch.float32, device=x.device)
    else:
        if (not torch.is_tensor(out) or out.dim() != 2 or out.dtype != torch.float32 or out.device != x.device
                or out.shape[0] != T or out.stride(1) != 1 or out.shape[1] < width):
            raise ValueError("out must be a float32 device tensor of %d rows of at least %d contiguous values" % (T, width))
        ldo = out.stride(0) if T > 1 else out.shape[1]
    _call(_lib.PCA_APPLY, mode=mode, T=T, L=L, k=k, q=ptr(x), out=ptr(out), ldo=ldo,
          **{role: ptr(t) for role, t in roles.items()})
    return out


def project(x, components, centre, out=None, ldo=None):
    """y [N, k] fp32 (or `out` / rows of pitch ldo >= k): y_j = sum_l (x_l - centre_l) v_jl: RV_PCA_PROJECT."""
    comp, centre, _, k, L = _basis(components, centre)
    x = _rows(x, "x", cols=L)
    return _apply(_lib.PCA_PROJECT, x, k, k, L, out, ldo, centre=centre, basis=comp)


def reconstruct(y, components, centre, out=None, ldo=None):
    """x^ [N, L] fp32 from coordinates y [N, k] fp32: centre_l + sum_j y_j v_jl: RV_PCA_RECONSTRUCT."""
    comp, centre, _, k, L = _basis(components, centre)
    y = _rows(y, "y", cols=k)
    return _apply(_lib.PCA_RECONSTRUCT, y, L, k, L, out, ldo, centre=centre, basis=comp)


def edit(x, components, centre, eigenvalues, gains, shifts, out=None, ldo=None):
    """x' [N, L] fp32: x_l + sum_j ((g_j - 1) y_j + h_j sqrt(max(lambda_j, 0))) v_jl with gains g and shifts h [k] fp32
    device tensors (read when the launch runs): RV_PCA_EDIT.  g = 1 and h = 0 return x bit for bit."""
    comp, centre, lam, k, L = _basis(components, centre, eigenvalues)
    x = _rows(x, "x", cols=L)
    gains = _vector(gains, "gains", k, torch.float32, comp.device)
    shifts = _vector(shifts, "shifts", k, torch.float32, comp.device)
    return _apply(_lib.PCA_EDIT, x, L, k, L, out, ldo, centre=centre, basis=comp, eigenvalues=lam, gains=gains,
                  shifts=shifts)


class LatentPCA:
    """Principal axes of rows x [N, L] (fit), all on x's device.

    After fit: mean_ [L], components_ [k, L] (row j = the j-th axis, its entry of largest magnitude positive),
    explained_variance_ [k] and explained_variance_ratio_ [k] (of the total variance over all L axes), all fp64;
    all_variances_ [L]; n_frames_, sweeps_; effective_dim_ = (sum lambda)^2 / sum lambda^2 over lambda clamped at 0.
    k = n_components, or L when it is None."""

    def __init__(self, n_components=None):
        if n_components is not None:
            if isinstance(n_components, bool) or not isinstance(n_components, (int, np.integer)) or n_components < 1:
                raise ValueError("n_components=%r must be a positive integer or None" % (n_components,))
            n_components = int(n_components)
        self.n_components = n_components
        self.mean_ = None

    def _set(self, mean, components, variances, n_frames, sweeps, k=None):
        L = mean.numel()
        k = L if k is None else k
        if not 1 <= k <= L:
            raise ValueError("n_components=%d must be in [1, %d], the latent dimension" % (k, L))
        self.mean_, self.all_variances_ = mean, variances
        self.components_ = components[:k].contiguous()
        self.explained_variance_ = variances[:k].contiguous()
        lam = variances.clamp(min=0).cpu().numpy()
        total = float(lam.sum())
        self.explained_variance_ratio_ = (variances[:k].clamp(min=0) / total if total > 0
                                          else torch.zeros_like(variances[:k]))
        self.effective_dim_ = float(total * total / float((lam * lam).sum())) if total > 0 else 0.0
        self.n_frames_, self.sweeps_ = int(n_frames), int(sweeps)
        return self

    @torch.no_grad()
    def fit(self, x):
        x = _rows(x)
        if self.n_components is not None and self.n_components > x.shape[1]:
            raise ValueError("n_components=%d must be in [1, %d], the latent dimension" % (self.n_components, x.shape[1]))
        mean, cov = moments(x)
        lam, comp, sweeps, converged = eig(cov)
        if not converged:
            raise RvError("LatentPCA.fit: the Jacobi eigensolver did not converge in %d sweeps" % sweeps)
        return self._set(mean, comp, lam, x.shape[0], sweeps, self.n_components)

    def _fitted(self):
        if self.mean_ is None:
            raise RuntimeError("LatentPCA has not been fitted")

    def components_needed(self, fraction):
        """The fewest leading axes whose variances (clamped at 0) sum to at least `fraction` of the total."""
        self._fitted()
        lam = self.all_variances_.clamp(min=0).cpu().numpy()
        if lam.sum() <= 0:
            return 0
        return int(min(np.searchsorted(np.cumsum(lam) / lam.sum(), float(fraction)) + 1, lam.size))

    @torch.no_grad()
    def transform(self, x, out=None):
        self._fitted()
        return project(x, self.components_, self.mean_, out)

    @torch.no_grad()
    def inverse_transform(self, y, out=None):
        self._fitted()
        return reconstruct(y, self.components_, self.mean_, out)

    def controls(self, gains=None, shifts=None):
        """(gains, shifts) as [k] fp32 device tensors: a sequence of k values, a {0-based axis: value} dict over the
        defaults (gain 1, shift 0), None for the defaults, or a device tensor (taken as it is)."""
        self._fitted()
        k, dev = self.components_.shape[0], self.mean_.device
        out = []
        for v, default, what in ((gains, 1.0, "gains"), (shifts, 0.0, "shifts")):
            if torch.is_tensor(v):
                out.append(_vector(v, what, k, torch.float32, dev))
                continue
            a = np.full(k, default, dtype=np.float32)
            if isinstance(v, dict):
                for j, val in v.items():
                    if not 0 <= int(j) < k:
                        raise ValueError("%s: axis %d outside the %d components" % (what, int(j), k))
                    a[int(j)] = val
            elif v is not None:
                v = np.asarray(v, dtype=np.float32).reshape(-1)
                if v.size != k:
                    raise ValueError("%s: %d values for %d components" % (what, v.size, k))
                a = v
            out.append(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
        return tuple(out)

    @torch.no_grad()
    def edit(self, x, gains=None, shifts=None, out=None):
        """x moved along the axes: coordinate j scaled by gains[j] about the mean and shifted by shifts[j] standard
        deviations (see `controls` for the forms gains and shifts may take)."""
        g, h = self.controls(gains, shifts)
        return edit(x, self.components_, self.mean_, self.explained_variance_, g, h, out)

    @torch.no_grad()
    def offset(self, shifts):
        """[L] fp32 device tensor sum_j h_j sqrt(lambda_j) v_j: what StreamingVAE.offset takes for `shifts`."""
        g, h = self.controls(None, shifts)
        zero = torch.zeros((1, self.mean_.numel()), dtype=torch.float32, device=self.mean_.device)
        return self.edit(zero, g, h)[0]


@torch.no_grad()
def fit_corpus(model, waves, hop=None, n_components=None, max_rows=16384):
    """LatentPCA fitted on the encoder's mu of every frame of every waveform, framed like TestDataset (hop=None) or
    AudioDataset (hop=int) through codec.FrameCodec."""
    return LatentPCA(n_components).fit(encode_corpus(model, waves, hop, max_rows)[0])


def write_pca(path, pca, segment_length, hop=None):
    """One .npz: mean [L], components [k, L], variances [L] (every eigenvalue), all fp64, and segment_length,
    latent_dim, hop (-1: non-overlapping frames), n_frames, sweeps."""
    pca._fitted()
    write_fitted(path, dict(mean=pca.mean_, components=pca.components_, variances=pca.all_variances_),
                 dict(segment_length=segment_length, latent_dim=pca.mean_.numel(), hop=hop, n_frames=pca.n_frames_,
                      sweeps=pca.sweeps_))


def read_pca(path, device="cuda"):
    """(LatentPCA on `device`, {segment_length, latent_dim, hop (None: non-overlapping), n_frames}) of write_pca's file;
    ValueError when the arrays do not fit one another."""
    arrays, meta, _ = read_fitted(path, "PCA", ("mean", "components", "variances"),
                                  ("segment_length", "latent_dim", "hop", "n_frames", "sweeps"))
    mean, comp, lam = arrays.values()
    L = meta["latent_dim"]
    if mean.shape != (L,) or lam.shape != (L,) or comp.ndim != 2 or comp.shape[1] != L or not 1 <= comp.shape[0] <= L:
        raise ValueError("%s: mean %s, components %s and variances %s do not fit latent_dim %d" % (
            path, mean.shape, comp.shape, lam.shape, L))
    dev = torch.device(device)
    pca = LatentPCA(comp.shape[0])._set(torch.from_numpy(mean).to(dev), torch.from_numpy(comp).to(dev),
                                        torch.from_numpy(lam).to(dev), meta["n_frames"], meta.pop("sweeps"),
                                        comp.shape[0])
    return pca, meta
