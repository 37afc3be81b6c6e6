#!/usr/bin/env python3
"""Generate tests/golden/interp_f32.npz: latent interpolation computed by the REFERENCE model itself (rawvae/model.py
imported by path as tools/make_golden.py does, CPU PyTorch fp32) on seeded inputs.  Needs the reference checkout; the
tests read only the committed fixture.

    python tools/make_interp_golden.py

Case (S, H, L) = (64, 96, 8), parameters oracle.inputs.make_params(S, H, L, 0), two synthetic sources of 1000 and
2345 samples (neither a multiple of S).  The shorter source is repeated to the longer one's length (the notebook's
match_size = 1), then three runs of the reference's encode / reparameterize / decode, with eps injected in place of
torch.randn_like (as tools/make_golden.py does):

  step   TestDataset framing, alphas numpy.arange(0, 1.1, 0.2), fp32 mix per alpha, the K decoded blocks concatenated
  curve  TestDataset framing, curve sin(linspace(-3 pi, 3 pi, 50)) stretched by scipy interp1d at linspace(0, C-1, N),
         fp64 mix and reparameterisation (torch's promotion of the float64 alpha), decode(z.float())
  ext    the curve run with AudioDataset framing at hop S / 8

The mix is restated from its semantics: mu = mu_a * (1 - alpha) + mu_b * alpha, logvar likewise.
Stored: a, b, the ten parameters (p/<name>), alphas, curve, eps_<run>, out_<run>, mu_<run>_a / _b (encoder outputs).
"""
import os
import sys
from contextlib import contextmanager

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from make_golden import load_reference  # noqa: E402
from oracle.inputs import make_eps, make_params  # noqa: E402

S, H, L = 64, 96, 8
N_A, N_B = 1000, 2345
OUT = os.path.join(REPO, "tests", "golden", "interp_f32.npz")


@contextmanager
def fixed_eps(eps_t):
    orig = torch.randn_like

    def _eps(t, *a, **k):
        assert t.shape == eps_t.shape, (t.shape, eps_t.shape)
        return eps_t.to(t.dtype)
    torch.randn_like = _eps
    try:
        yield
    finally:
        torch.randn_like = orig


def repeat_to(x, n):
    return x[np.arange(n) % len(x)]


def frames(x, hop):
    """TestDataset (hop None) / AudioDataset framing of a waveform."""
    step = S if hop is None else hop
    padded = -(-len(x) // step) * step
    buf = np.zeros(padded, np.float32)
    buf[:len(x)] = x
    n = padded // step - S // step + 1
    return buf[np.arange(n)[:, None] * step + np.arange(S)[None, :]]


def main():
    import scipy.interpolate
    ref = load_reference("model")
    model = ref.VAE(S, H, L)
    params = make_params(S, H, L, 0)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model.eval()
    rng = np.random.default_rng(2024)
    t = np.arange(N_B)
    a = (0.6 * np.sin(2 * np.pi * 0.013 * np.arange(N_A)) + 0.1 * rng.standard_normal(N_A)).astype(np.float32)
    b = (0.5 * np.sign(np.sin(2 * np.pi * 0.004 * t)) * np.exp(-t / 3000.0) + 0.05 * rng.standard_normal(N_B))
    b = b.astype(np.float32)
    n = max(N_A, N_B)
    am, bm = repeat_to(a, n), repeat_to(b, n)
    out = {"a": a, "b": b, "shape": np.array([S, H, L])}
    out.update({"p/" + k: v for k, v in params.items()})
    alphas = np.arange(0, 1.1, 0.2)
    curve = np.sin(np.linspace(-3 * np.pi, 3 * np.pi, 50))
    out["alphas"], out["curve"] = alphas, curve
    with torch.no_grad():
        for run, hop in (("step", None), ("curve", None), ("ext", S // 8)):
            mu_a, lv_a = model.encode(torch.from_numpy(frames(am, hop)))
            mu_b, lv_b = model.encode(torch.from_numpy(frames(bm, hop)))
            N = mu_a.shape[0]
            out["mu_%s_a" % run], out["mu_%s_b" % run] = mu_a.numpy(), mu_b.numpy()
            if run == "step":
                eps = make_eps(len(alphas) * N, L, 77)
                pieces = []
                for k, al in enumerate(alphas):
                    mu = torch.add(torch.mul(mu_a, 1 - al), torch.mul(mu_b, al))
                    lv = torch.add(torch.mul(lv_a, 1 - al), torch.mul(lv_b, al))
                    with fixed_eps(torch.from_numpy(eps[k * N:(k + 1) * N])):
                        z = model.reparameterize(mu, lv)
                    pieces.append(model.decode(z))
                y = torch.cat(pieces, 0)
            else:
                eps = make_eps(N, L, 78 if run == "curve" else 79)
                f = scipy.interpolate.interp1d(np.arange(0, len(curve)), curve)
                al = torch.from_numpy(f(np.linspace(0.0, len(curve) - 1, N)))[:, None]
                mu = torch.add(torch.mul(mu_a, 1 - al), torch.mul(mu_b, al))
                lv = torch.add(torch.mul(lv_a, 1 - al), torch.mul(lv_b, al))
                assert mu.dtype == torch.float64
                with fixed_eps(torch.from_numpy(eps)):
                    z = model.reparameterize(mu, lv)
                y = model.decode(z.float())
            out["eps_" + run] = eps
            out["out_" + run] = y.reshape(-1).numpy()
            print(run, "frames", N, "output samples", out["out_" + run].size)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
