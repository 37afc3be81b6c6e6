"""tests/ingest_oracle.py against independent statements of the same rules: the host resampler, oracle.vae_oracle's
framing, scipy's interp1d over numpy's linspace, and torch-CPU's mix (the expressions of tests/test_interpolate_gpu.py)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ingest_oracle as IO  # noqa: E402
from test_ingest_gpu import PAIRS  # noqa: E402


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@pytest.mark.parametrize("sr_in,sr_out", [PAIRS[0], PAIRS[2], PAIRS[4]])     # 160 -> 147, 1 -> 2, 441 -> 160
def test_resample_chain_is_the_host_resampler(sr_in, sr_out):
    from rawaudiovae_kelsey_amd import data as D
    orig, new, width, bank = D._sinc_hann_bank(sr_in, sr_out)
    rng = np.random.default_rng(sr_in + sr_out)
    for n in (1, width, 3 * orig + 1, 1500):
        a = rng.standard_normal(n).astype(np.float32)
        y = IO.resample_chain(a, orig, new, width, bank)
        ref = D._resample_sinc_hann(a, sr_in, sr_out)
        assert y.dtype == np.float32 and y.shape == ref.shape == (IO.resample_target(n, orig, new),)
        err = np.abs(y.astype(np.float64) - ref).max()
        print("resample_chain %d -> %d, n %d: max |chain - host| = %.3e (bound 1e-5)" % (orig, new, n, err))
        assert err <= 1e-5
    # the padding to n_out is +0
    y = IO.resample_chain(a, orig, new, width, bank, n_out=len(ref) + 2 * new + 1)
    assert np.array_equal(_bits(y[:len(ref)]), _bits(IO.resample_chain(a, orig, new, width, bank)))
    assert not _bits(y[len(ref):]).any()


def test_resample_chain_sees_a_dropped_tap():
    """The bank's very last tap sits where the window is clipped and is 0 in every phase of every bank, so the tap dropped
    here is the last one that holds a value: 1.2e-6 at 2 -> 1, which moves no output by 1e-5 and still changes bits."""
    from rawaudiovae_kelsey_amd import data as D
    orig, new, width, bank = D._sinc_hann_bank(2, 1)
    rng = np.random.default_rng(5)
    a = rng.standard_normal(500).astype(np.float32)
    y = IO.resample_chain(a, orig, new, width, bank)
    assert not bank[:, -1].any()
    k = int(np.flatnonzero(bank.any(axis=0))[-1])
    cut = bank.copy()
    cut[:, k] = 0
    last = np.abs(bank[:, k])
    assert 0 < last.max() < 1e-5 / np.abs(a).max()         # the existing 1e-5 check cannot see this tap
    z = IO.resample_chain(a, orig, new, width, cut)
    changed = int((_bits(y) != _bits(z)).sum())
    print("tap %d of %d at 2 -> 1: largest |value| %.3e; zeroing it changes %d of %d outputs, by at most %.3e"
          % (k, bank.shape[1], last.max(), changed, y.size, np.abs(y.astype(np.float64) - z).max()))
    assert changed > y.size // 2 and np.abs(y.astype(np.float64) - z).max() < 1e-5


@pytest.mark.parametrize("S,hop", [(1, 1), (4, 4), (100, 100), (256, 64), (6, 2)])
def test_gather_is_the_oracles_framing(S, hop):
    from oracle import vae_oracle as O
    rng = np.random.default_rng(S + hop)
    for n_samples in (S, 5 * S + 1, 7 * S + hop - 1):
        audio = rng.standard_normal(n_samples).astype(np.float32)
        n, _ = O.frame_count(n_samples, S, hop)
        idx = rng.permutation(n)
        assert np.array_equal(_bits(IO.gather(audio, n_samples, idx, 0, n, S, hop)), _bits(O.hop_frames(audio, S, hop, idx)))
        first = n // 2
        got = IO.gather(audio, n_samples, None, first, n - first, S, hop)
        assert np.array_equal(_bits(got), _bits(O.hop_frames(audio, S, hop, np.arange(first, n))))
    # outside the framing's domain: zeros before the waveform and past its end, whatever the buffer holds there
    audio = np.arange(1, 11, dtype=np.float32)
    got = IO.gather(audio, 7, np.array([-1, 3, 9]), 0, 3, 3, 2)
    assert np.array_equal(got, np.array([[0, 0, 1], [7, 0, 0], [0, 0, 0]], dtype=np.float32))
    assert np.array_equal(IO.match_pad(audio, 3, 7, 9), np.array([1, 2, 3, 1, 2, 3, 1, 0, 0], dtype=np.float32))
    assert np.array_equal(IO.match_pad(audio, 10, 0, 2), np.zeros(2, dtype=np.float32))


@pytest.mark.parametrize("C", [2, 3, 7])
def test_curve_alpha_is_scipy_over_linspace(C):
    import scipy.interpolate
    rng = np.random.default_rng(C)
    y = rng.uniform(-1, 2, C)
    for N in (1, 2, C, 2 * C - 1, 50):
        ref = scipy.interpolate.interp1d(np.arange(C), y)(np.linspace(0, C - 1, N))
        got = IO.curve_alpha(y, N)
        assert got.dtype == np.float64 and np.array_equal(_bits(got), _bits(ref)), (C, N)
        if N == 2 * C - 1:                      # every second point lies on the grid and is y[j] itself
            assert np.array_equal(_bits(got[::2]), _bits(y))
        out = IO.latent_mix(*np.zeros((4, N, 1), np.float32), IO.CURVE, y)
        assert np.array_equal(_bits(out["alpha"]), _bits(ref))


def test_fp32_mix_is_torch_cpu():
    N, L = 37, 24
    g = torch.Generator().manual_seed(1)
    mu_a, lv_a, mu_b, lv_b = (torch.randn(N, L, generator=g) * s for s in (1.0, 0.7, 1.3, 0.5))
    d = [t.numpy() for t in (mu_a, lv_a, mu_b, lv_b)]
    alphas = np.arange(0, 1.1, 0.2)             # test_mix_fp32_list_explicit_eps_vs_torch_cpu's
    out = IO.latent_mix(*d, IO.LIST, alphas)
    mu_ref = torch.cat([torch.add(torch.mul(mu_a, 1 - al), torch.mul(mu_b, al)) for al in alphas])
    lv_ref = torch.cat([torch.add(torch.mul(lv_a, 1 - al), torch.mul(lv_b, al)) for al in alphas])
    assert np.array_equal(_bits(out["mu"]), _bits(mu_ref.numpy()))
    assert np.array_equal(_bits(out["logvar"]), _bits(lv_ref.numpy()))
    assert np.array_equal(out["alpha"], np.repeat(alphas.astype(np.float32), N).astype(np.float64))
    part = IO.latent_mix(*d, IO.LIST, alphas, row0=29, rows=101)       # rows wrap over the frames
    assert np.array_equal(_bits(part["mu"]), _bits(mu_ref.numpy()[29:130]))
    al = torch.rand(N, generator=torch.Generator().manual_seed(4))     # test_mix_fp32_per_frame_alpha_vs_torch_cpu's
    out = IO.latent_mix(*d, IO.F32, al.numpy())
    a2 = al[:, None]
    assert np.array_equal(_bits(out["mu"]), _bits(torch.add(torch.mul(mu_a, 1 - a2), torch.mul(mu_b, a2)).numpy()))
    assert np.array_equal(_bits(out["logvar"]), _bits(torch.add(torch.mul(lv_a, 1 - a2), torch.mul(lv_b, a2)).numpy()))
    # the float64 modes against torch-CPU's float64 expression (test_curve_stretch_and_fp64_mix's)
    a64 = torch.rand(N, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    eps = torch.randn(N, L, generator=torch.Generator().manual_seed(6))
    out = IO.latent_mix(*d, IO.F64, a64.numpy(), eps=eps.numpy())
    a2 = a64[:, None]
    mu = torch.add(torch.mul(mu_a, 1 - a2), torch.mul(mu_b, a2))
    lv = torch.add(torch.mul(lv_a, 1 - a2), torch.mul(lv_b, a2))
    assert mu.dtype == torch.float64 and np.array_equal(_bits(out["mu"]), _bits(mu.float().numpy()))
    assert np.array_equal(_bits(out["logvar"]), _bits(lv.float().numpy()))
    z = (mu + eps.double() * torch.exp(0.5 * lv)).float().numpy()
    err = np.abs(out["z"].astype(np.float64) - z)
    assert (err <= np.spacing(np.abs(z))).all()             # numpy's exp and torch's may differ in the last float64 bit
    print("float64 z: numpy == torch-CPU at %.2f %% of %d elements" % (100.0 * (_bits(out["z"]) == _bits(z)).mean(), z.size))
