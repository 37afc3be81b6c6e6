"""Float64 restatement of the streaming resynthesis contract (rawaudiovae_kelsey_amd/stream.py) for the tests:
framing with P = S - hop zeros in front, the one-hidden-layer forward, and weighted overlap-add normalised by the
window sum."""
import numpy as np


def frames(x, S, hop):
    """Every complete frame of Xp = [0] * (S - hop) + x: [n, S] (frame f = Xp[f hop : f hop + S])."""
    xp = np.concatenate([np.zeros(S - hop, dtype=np.float64), np.asarray(x, dtype=np.float64)])
    n = (xp.size - S) // hop + 1
    return np.stack([xp[f * hop:f * hop + S] for f in range(n)]) if n > 0 else np.zeros((0, S))


def wola(dec, w, hop, n_out):
    """Yp[t] = sum_f w[t - f hop] D_f[t - f hop] / sum_f w[t - f hop] over the frames f that cover t (0 where the
    sum of weights is 0), for t < n_out."""
    dec = np.asarray(dec, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    S = w.size
    num = np.zeros(max(n_out, dec.shape[0] * hop + S))
    den = np.zeros_like(num)
    for f in range(dec.shape[0]):
        num[f * hop:f * hop + S] += w * dec[f]
        den[f * hop:f * hop + S] += w
    num, den = num[:n_out], den[:n_out]
    out = np.zeros(n_out)
    nz = den != 0
    out[nz] = num[nz] / den[nz]
    return out


def forward(p, x, eps, scale=None, offset=None, temperature=1.0):
    """Float64 forward of frames x [n, S] with eps [n, L]: (decoded [n, S], mu, logvar).  p: name -> array."""
    g = {k: np.asarray(v, dtype=np.float64) for k, v in p.items()}
    h1 = np.maximum(x @ g["fc1.weight"].T + g["fc1.bias"], 0.0)
    mu = h1 @ g["fc21.weight"].T + g["fc21.bias"]
    lv = h1 @ g["fc22.weight"].T + g["fc22.bias"]
    m = mu if scale is None else mu * scale
    m = m if offset is None else m + offset
    z = m + temperature * eps * np.exp(0.5 * lv)
    h3 = np.maximum(z @ g["fc3.weight"].T + g["fc3.bias"], 0.0)
    return np.tanh(h3 @ g["fc4.weight"].T + g["fc4.bias"]), mu, lv
