"""The device RNG (csrc/philox.h) bit for bit: every consumer's draws against the numpy oracle (tests/rng_oracle.py).

Philox's words and the fp32 uniforms are reproduced exactly by the oracle, so a device value differs from the oracle's
float64 Box-Muller value only by the device's own log / sqrt / sin / cos arithmetic.  The bounds below are four times the
largest difference measured on an MI355X over the runs of this file (profiles/rng_summary.txt; the margin is for libm
differences between ROCm releases), and by rule never above 1e-5 -- a permuted lane, a swapped sin / cos, a wrong counter
word or a missing key bump moves a draw by O(1).

  accurate form (normal4: logf, sqrtf, sincospif)   measured 7.08e-07 (bulk), 4.40e-07 (the four edge counters) -> ACC_BOUND       = 2.83e-06
  fast form (normal4_fast: __logf, __sinf, __cosf)  measured 1.79e-06 (bulk, every forward form)         -> FAST_BOUND      = 7.17e-06
  fast form, the draws of the four edge counters    measured 3.23e-07 (9.3e-08 at the smallest radius)   -> FAST_EDGE_BOUND = 1.29e-06
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import rng_oracle as R  # noqa: E402
from guarded import SENTINEL, guarded_flat  # noqa: E402

ACC_BOUND = 4 * 7.080e-7
FAST_BOUND = 4 * 1.793e-6
FAST_EDGE_BOUND = 4 * 3.231e-7
CAP = 1e-5
assert max(ACC_BOUND, FAST_BOUND, FAST_EDGE_BOUND) <= CAP

SEED = 0x9E3779B97F4A7C15          # a non-zero high half: both key words count
HI = (1 << 32) + 5                 # an offset / step whose high word counts (counter word c3)
N_TAIL = 4099                      # a ragged tail
N_STRIDE = 4 * 2048 * 256 + 7      # one more than the 2048-block grid cap covers in one trip, and a ragged tail


@pytest.fixture(scope="module")
def L():
    from rawaudiovae_kelsey_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.lib()


def sp():
    return torch.cuda.current_stream().cuda_stream or None


def _randn(L, n, seed, offset):
    g = guarded_flat(n, torch.float32)
    L.rv_randn(g.ptr, n, seed, offset, sp())
    g.assert_untouched("rv_randn")
    return g.payload().view(-1)


def _err(got, ref, what):
    """max |got - ref| (device fp32 against the oracle's float64), printed: the figure behind the bounds above."""
    a = got.detach().cpu().numpy().astype(np.float64).reshape(-1)
    assert np.isfinite(a).all(), what
    e = float(np.abs(a - np.asarray(ref).reshape(-1)).max())
    print("rng max |device - float64|: %-58s %.3e" % (what, e))
    return e


# ------------------------------------------------------------------------------------------------ accurate form
@pytest.mark.parametrize("n", [N_TAIL, N_STRIDE])
@pytest.mark.parametrize("seed,offset", [(SEED, 0), (SEED, 5), (SEED, HI), (1234, 5)])
def test_randn_draws_the_oracles_values(L, n, seed, offset):
    got = _randn(L, n, seed, offset)
    assert _err(got, R.randn_ref(n, seed, offset), "rv_randn n=%d seed=%#x offset=%d" % (n, seed, offset)) <= ACC_BOUND


@pytest.mark.parametrize("edge", range(4), ids=["x_high", "x_low", "z_high", "z_low"])
def test_randn_at_the_edges_of_the_uniforms(L, edge):
    """One counter whose word x (z) rounds to u = 1.0 and is clamped -- the smallest radius, 3.45e-4 -- and one whose word
    is below 0x100 -- a radius of 5.8: finite, and as close to float64 as everywhere else."""
    hi, _ = R.EDGES[edge]
    got = _randn(L, 4, R.EDGE_SEED, hi)
    ref = R.randn_ref(4, R.EDGE_SEED, hi)
    assert _err(got, ref, "rv_randn edge counter %d" % hi) <= ACC_BOUND
    pair = got.cpu().numpy().astype(np.float64)[2 * (edge // 2):2 * (edge // 2) + 2]
    r = float(np.hypot(pair[0], pair[1]))
    assert abs(r - 3.4527e-4) < 1e-6 if edge % 2 == 0 else 5.8 < r < 5.95


@pytest.mark.parametrize("seed,offset", [(SEED, 0), (SEED, HI), (9, 1)])
def test_reparameterize_draws_rv_randn(L, seed, offset):
    """eps_out of rv_reparameterize(seed, offset) is rv_randn(n, seed, offset) bit for bit, over a second grid-stride trip."""
    n = 2048 * 256 + 5
    g = torch.Generator().manual_seed(3)
    mu, lv = torch.randn(n, generator=g).cuda(), (0.3 * torch.randn(n, generator=g)).cuda()
    eps, z = guarded_flat(n, torch.float32), guarded_flat(n, torch.float32)
    L.rv_reparameterize(mu.data_ptr(), lv.data_ptr(), n, None, eps.ptr, seed, offset, z.ptr, sp())
    eps.assert_untouched("eps_out")
    z.assert_untouched("z")
    e = eps.payload().view(-1)
    assert torch.equal(e, _randn(L, n, seed, offset))
    # ... and z is built from that eps
    zr = mu.double() + e.double() * torch.exp(0.5 * lv.double())
    assert float((z.payload().view(-1).double() - zr).abs().max()) <= 2e-6 * float(zr.abs().max()) + 1e-6


def test_streaming_engine_draws_rv_randn_per_stream():
    """The streaming engine's Philox run is its explicit-eps run fed rv_randn(seed, offset = stream) laid out
    [frame, latent]: element f * L + l of stream s's draw, f the stream's absolute frame number (it runs on over the
    blocks)."""
    from rawaudiovae_kelsey_amd._lib import lib
    from rawaudiovae_kelsey_amd.stream import StreamingVAE
    from rawvae.model import VAE
    S_, H_, L_, hop, n_streams, n_blocks = 256, 128, 22, 64, 2, 3
    torch.manual_seed(5)
    model = VAE(S_, H_, L_).cuda().eval()
    block = 2 * hop
    F = block // hop
    nf = n_blocks * F
    g = torch.Generator().manual_seed(6)
    x = (torch.rand((n_streams, n_blocks * block), generator=g) - 0.5).cuda()
    E = torch.stack([_randn(lib(), nf * L_, SEED, s).view(nf, L_) for s in range(n_streams)])

    def run(eng, eps):
        out = []
        for k in range(n_blocks):
            e = None if eps is None else eps[:, k * F:(k + 1) * F].contiguous()
            out.append(eng.process(x[:, k * block:(k + 1) * block].contiguous(), eps=e).clone())
        return torch.cat(out, 1)
    ya = run(StreamingVAE(model, n_streams, block, hop=hop, window="hann", seed=SEED), None)
    yb = run(StreamingVAE(model, n_streams, block, hop=hop, window="hann", seed=SEED), E)
    assert torch.equal(ya, yb) and bool(torch.isfinite(ya).all()) and float(ya.abs().max()) > 0
    assert not torch.equal(ya[0], ya[1])
    # the draw matters: another seed, or the streams' draws swapped, gives other audio
    assert not torch.equal(run(StreamingVAE(model, n_streams, block, hop=hop, window="hann", seed=SEED + 1), None), ya)
    assert not torch.equal(run(StreamingVAE(model, n_streams, block, hop=hop, window="hann", seed=SEED), E.flip(0)), ya)


# ------------------------------------------------------------------------------------------------ fast form
def _reparam_fwd(L, B, Lt, Lp, Bp, seed, step, splits=1):
    """rv_reparam_fwd with generated eps -> eps_out [B, Lt] (guarded), mulv, z."""
    g = torch.Generator().manual_seed(B * 131 + Lt)
    slabs = (0.3 * torch.randn((splits, Bp, 2 * Lp), generator=g)).cuda()
    mulv = torch.empty(Bp, 2 * Lp, device="cuda")
    z = torch.empty(Bp, Lp, device="cuda", dtype=torch.bfloat16)
    klp = torch.zeros(Bp * Lp // 1024, device="cuda")
    ctr = torch.tensor([step], dtype=torch.int64, device="cuda")      # (2^32 + 5 only fits a device int64)
    eps = guarded_flat(B * Lt, torch.float32)
    L.rv_reparam_fwd(slabs.data_ptr(), splits, Bp, Lp, B, Lt, None, eps.ptr, seed, ctr.data_ptr(), mulv.data_ptr(), z.data_ptr(),
                     klp.data_ptr(), sp())
    eps.assert_untouched("eps_out")
    assert int(ctr.item()) == step                                     # read, never written
    return eps.payload().view(B, Lt), mulv, z


FAST_SHAPES = [(100, 3, 64, 128), (16, 64, 64, 16), (130, 129, 256, 256), (1, 1, 64, 16)]   # (B, L, Lp, Bp)


@pytest.mark.parametrize("B,Lt,Lp,Bp", FAST_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("step", [0, 1, HI])
def test_training_eps_draws_the_oracles_grid(L, B, Lt, Lp, Bp, step):
    """rv_reparam_fwd with eps_in = NULL: element (b, l) is lane l & 3 of counter (b * (Lp / 4) + l / 4, *step_counter)."""
    eps, mulv, z = _reparam_fwd(L, B, Lt, Lp, Bp, SEED, step)
    ref = R.eps_grid_ref(B, Lt, Lp, SEED, step)
    assert _err(eps, ref, "rv_reparam_fwd (B, L, Lp)=(%d, %d, %d) step=%d" % (B, Lt, Lp, step)) <= FAST_BOUND
    # z = mu + eps * exp(logvar / 2) on that eps
    mv = mulv.double()
    zr = mv[:B, :Lt] + eps.double() * torch.exp(0.5 * mv[:B, Lp:Lp + Lt])
    assert float((z[:B, :Lt].double() - zr).abs().max()) <= 2.0 ** -8 * float(zr.abs().max()) + 1e-6


@pytest.mark.parametrize("edge", range(4), ids=["x_high", "x_low", "z_high", "z_low"])
def test_training_eps_at_the_edges_of_the_uniforms(L, edge):
    """The edge counters as *step_counter (seed 1234): elements (0, 0..3) are the draw of counter (0, step)."""
    hi, _ = R.EDGES[edge]
    eps, _, _ = _reparam_fwd(L, 16, 64, 64, 16, R.EDGE_SEED, hi)
    ref = R.eps_grid_ref(16, 64, 64, R.EDGE_SEED, hi)
    e_edge = _err(eps[0, :4], ref[0, :4], "rv_reparam_fwd edge counter %d (4 values)" % hi)
    assert e_edge <= FAST_EDGE_BOUND
    assert _err(eps, ref, "rv_reparam_fwd (16, 64, 64) step=%d" % hi) <= FAST_BOUND


# (B, L, H) -> the form of rv_latent_fwd: row-local (Lp = 64, Hp % 512 == 0, Bp <= 8192), 64 x 128 GEMM tiles,
# 256 x 128 at a large batch and Lp = 64 (Bp = 65792 = 257 * 256), 256 x 256 ping-pong at a large batch and Lp >= 128
FORMS = {"rowlocal": (200, 64, 512), "gemm64x128": (300, 100, 256), "big256x128": (65700, 64, 256), "pp256x256": (16600, 256, 256)}


@pytest.mark.parametrize("variant", ["vector", "ragged_L", "unaligned_base"])
@pytest.mark.parametrize("form", list(FORMS))
def test_every_forward_form_draws_the_same_bits(L, form, variant):
    """eps_out of rv_latent_fwd in each of its kernel forms == rv_reparam_fwd's for the same (B, L, Lp, seed, step), with
    L % 4 == 0 (16-byte eps stores in the GEMM epilogue), L % 4 != 0 and a base that is not 16-byte aligned (its scalar
    stores); the last rows of the batch against the oracle as well (b * (Lp / 4) at the large batch)."""
    B, Lt, H = FORMS[form]
    if variant == "ragged_L":
        Lt -= 3
    step = {"vector": HI, "ragged_L": 1, "unaligned_base": 0}[variant]
    off = 1 if variant == "unaligned_base" else 0
    Bp, Lp, Hp = -(-B // 128) * 128, 64 if Lt <= 64 else 128 if Lt <= 128 else 256, H
    g = torch.Generator(device="cuda").manual_seed(7)
    h = (0.5 * torch.randn((Bp, Hp), generator=g, device="cuda")).clamp_min(0).to(torch.bfloat16)
    wh = (0.05 * torch.randn((2 * Lp, Hp), generator=g, device="cuda")).to(torch.bfloat16)
    bh = torch.zeros(2 * Lp, device="cuda")
    mulv = torch.empty(Bp, 2 * Lp, device="cuda")
    z = torch.empty(Bp, Lp, device="cuda", dtype=torch.bfloat16)
    klp = torch.zeros(Bp * Lp // 1024, device="cuda")
    ctr = torch.tensor([step], dtype=torch.int64, device="cuda")
    n = B * Lt
    e1, e2 = guarded_flat(n + 4, torch.float32), guarded_flat(n + 4, torch.float32)
    assert (e1.ptr + 4 * off) % 16 == (4 if off else 0)
    # (w3 = NULL: heads + reparameterisation only, in every form)
    L.rv_latent_fwd(h.data_ptr(), Hp, wh.data_ptr(), Hp, bh.data_ptr(), None, 0, None, Bp, Hp, Lp, B, Lt, None, e1.ptr + 4 * off,
                    SEED, ctr.data_ptr(), mulv.data_ptr(), z.data_ptr(), klp.data_ptr(), None, 0, sp())
    # the form that ran, read off the KL partials it left: one per 16 rows (row-local), or one per tile and zeros beside it
    k = klp.cpu().numpy()
    bm, tiles_n = {"rowlocal": (16, 1), "gemm64x128": (64, Lp // 64), "big256x128": (256, 1), "pp256x256": (256, Lp // 128)}[form]
    kk = k.reshape(Bp // bm * tiles_n, -1)          # [tile, slots of the tile]: 1, 4, 16, 32 slots
    assert kk.shape[1] == {"rowlocal": 1, "gemm64x128": 4, "big256x128": 16, "pp256x256": 32}[form]
    live = -(-B // bm) * tiles_n                    # tiles that hold rows of the batch
    assert kk[:live, 0].all() and not kk[live:, 0].any() and not kk[:, 1:].any(), form
    slabs = torch.zeros(1, Bp, 2 * Lp, device="cuda")
    L.rv_reparam_fwd(slabs.data_ptr(), 1, Bp, Lp, B, Lt, None, e2.ptr + 4 * off, SEED, ctr.data_ptr(), mulv.data_ptr(), z.data_ptr(),
                     klp.data_ptr(), sp())
    for e in (e1, e2):
        e.assert_untouched("eps_out")
        p = e.payload().view(-1)
        assert bool((p[:off] == SENTINEL).all()) and bool((p[off + n:] == SENTINEL).all())
    a, b = e1.payload().view(-1)[off:off + n], e2.payload().view(-1)[off:off + n]
    assert torch.equal(a, b)
    row0 = max(0, B - 300)
    ref = R.eps_grid_ref(B, Lt, Lp, SEED, step, row0=row0)
    assert _err(a.view(B, Lt)[row0:], ref, "rv_latent_fwd %s %s rows %d..%d" % (form, variant, row0, B)) <= FAST_BOUND


def test_fast_form_statistics(L):
    """2^20 draws of the training step's eps on a [16384, 64] grid: rv_randn's thresholds (test_kernels_gpu.py
    test_randn_statistics), and no correlation between consecutive steps or between lanes 0 and 1 of the counters."""
    from scipy import stats
    B = 16384
    e3, _, _ = _reparam_fwd(L, B, 64, 64, B, SEED, 3)
    e4, _, _ = _reparam_fwd(L, B, 64, 64, B, SEED, 4)
    a3, a4 = e3.cpu().numpy().astype(np.float64), e4.cpu().numpy().astype(np.float64)
    a = a3.reshape(-1)
    assert a.size == 1 << 20 and np.isfinite(a).all()
    assert abs(a.mean()) < 5e-3 and abs(a.std() - 1) < 5e-3
    assert abs(stats.skew(a)) < 2e-2 and abs(stats.kurtosis(a)) < 5e-2
    assert stats.kstest(a[:200000], "norm").pvalue > 1e-3
    assert abs(np.corrcoef(a, a4.reshape(-1))[0, 1]) < 5e-3
    assert abs(np.corrcoef(a3[:, 0::4].reshape(-1), a3[:, 1::4].reshape(-1))[0, 1]) < 5e-3


# ------------------------------------------------------------------------------------------------ the step keys the draw
def test_the_step_counter_keys_the_draw_eagerly_and_under_replay():
    """Three eager steps and three replays of one captured step: after each, the engine's eps buffer is the oracle's grid for
    the device step counter at that step (a replay must read the counter from memory, not carry a captured value), and
    differs from the step before."""
    from oracle.inputs import make_frames
    from rawaudiovae_kelsey_amd.engine import Graph
    from test_engine_gpu import _engine
    S_, H_, L_, B = 256, 256, 16, 64
    seed = SEED
    x = torch.from_numpy(make_frames(B, S_, 1)).cuda()

    def eps_of(e):
        torch.cuda.synchronize()
        Bp, _, _, Lp = e.padded()
        return e.buffer("eps", torch.float32, (Bp * Lp,))[:B * L_].clone().view(B, L_), int(e.step_counter.item()), Lp

    def check(e, t_want, prev, what):
        eps, t, Lp = eps_of(e)
        assert t == t_want
        assert _err(eps, R.eps_grid_ref(B, L_, Lp, seed, t), "%s step %d" % (what, t)) <= FAST_BOUND
        if prev is not None:
            assert float((eps - prev).abs().max()) > 1.0       # another draw, not the last one again
        return eps
    a = _engine(S_, H_, L_, B, seed=seed)
    prev = None
    for t in (1, 2, 3):
        a.step(x)
        prev = check(a, t, prev, "eager")
    b = _engine(S_, H_, L_, B, seed=seed)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with Graph(st) as g:
            b.step(x, stream=st)
        prev = None
        for t in (1, 2, 3):
            g.launch()
            prev = check(b, t, prev, "replay")
    torch.cuda.synchronize()
