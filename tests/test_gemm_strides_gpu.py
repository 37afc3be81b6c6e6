"""Leading dimensions of the bf16 GEMM family (GPU): every entry point of include/rawvae_hip.h that takes an `ld*`
argument, called with EVERY leading dimension different from its row width and from every other one in the call, on
buffers cut from the inside of guarded allocations (tests/guarded.py).  Each case asserts

  1. bit equality with the packed call (same entry point, data and forced tile): a leading dimension changes no
     arithmetic and no summation order, so no tolerance applies;
  2. the float64 reference, with the tolerance the neighbouring packed test of tests/test_kernels_gpu.py states for the
     same operation;
  3. guards, gap columns [width, ld) and side tables bit-equal to the sentinel they were filled with (inputs carry NaN
     there: a read poisons the result);
  4. for split outputs, slab s at element offset s * rows * ld (the slabs are read back through that stride).

Every case runs at two sets of leading dimensions: the width plus small distinct odd multiples of 8 (of 4 for fp32 slabs,
whose rule is ld % 4), and the width plus 264 and up (no power of two)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import vae_oracle as O  # noqa: E402
from guarded import PACKED_FILL, guarded, guarded_flat  # noqa: E402
from test_kernels_gpu import dev, rand_bf16, sp  # noqa: E402

BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
TILES = [-1, 0, 1, 2, 3, 4, 5, 7]
TILE_IDS = ["auto", "t64", "t128w4", "t256x128w8", "t256x128w4", "t128w8", "t256x256", "t256x256pp"]
# pads[8]: for bf16 tensors and fp16 slabs (ld % 8 == 0), pads[4]: for fp32 slabs (ld % 4 == 0; 4 * odd, so never equal to
# a pads[8] value), pads[1]: for the exact-shape fp32 tensors that take any leading dimension
PADS = {"small": {8: (8, 24, 40, 56, 72, 88), 4: (12, 20, 28, 36), 1: (9, 3)},
        "large": {8: (264, 280, 296, 312, 328, 344), 4: (268, 276, 284, 292), 1: (262, 268)}}


@pytest.fixture(scope="module")
def L():
    from rawaudiovae_kelsey_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.lib()


@pytest.fixture(params=TILES, ids=TILE_IDS)
def tile(request, L):
    """Pin each block-tile configuration in turn through the test hook of include/rawvae_hip_diag.h."""
    L.rv_gemm_force_tile(request.param)
    yield request.param
    L.rv_gemm_force_tile(-1)


@pytest.fixture(params=["small", "large"])
def pads(request):
    return PADS[request.param]


def f64(a):
    return np.asarray(a, dtype=np.float64)


def host(t):
    return t.float().cpu().numpy()


def packed(shape, dtype):
    return torch.full(shape, PACKED_FILL, dtype=dtype, device="cuda")


def same_bits(a, b, name):
    """Bit equality of two tensors of one shape and dtype (through an integer view: -0 != +0, NaN compares by its bits)."""
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape)
    bad = int((a.contiguous().view(it) != b.contiguous().view(it)).sum())
    assert bad == 0, "%s: %d of %d payload elements differ from the packed call" % (name, bad, a.numel())


def distinct(lds, widths):
    """Every leading dimension of a call differs from every other one and from every row width of that call."""
    assert len(set(lds)) == len(lds) and not set(lds) & set(widths), (lds, widths)


# ------------------------------------------------------------------------------------------------ forward GEMMs

def _linear_fwd_case(L, pads, M, N, K):
    rng = np.random.default_rng(M + N + K)
    x, w = rand_bf16(rng, (M, K)), rand_bf16(rng, (N, K))
    b = rng.standard_normal(N).astype(np.float32)
    ldx, ldw, ldy = K + pads[8][0], K + pads[8][1], N + pads[8][2]
    distinct((ldx, ldw, ldy), (K, N))
    X, W = guarded(M, K, ldx, BF, x), guarded(N, K, ldw, BF, w)
    xd, wd, bd = dev(x, BF), dev(w, BF), dev(b)
    for act in (0, 1):
        Y, yp = guarded(M, N, ldy, BF), packed((M, N), BF)
        L.rv_linear_fwd(X.ptr, ldx, W.ptr, ldw, bd.data_ptr(), M, N, K, act, Y.ptr, ldy, sp())
        L.rv_linear_fwd(xd.data_ptr(), K, wd.data_ptr(), K, bd.data_ptr(), M, N, K, act, yp.data_ptr(), N, sp())
        same_bits(Y.payload(), yp, "y (act %d)" % act)
        ref = f64(x) @ f64(w).T + b
        if act:
            ref = np.maximum(ref, 0)
        assert np.abs(host(Y.payload()) - ref).max() <= 2 ** -7 * np.abs(ref).max()
        Y.assert_untouched("y (act %d)" % act)


def test_linear_fwd(L, tile, pads):
    """rv_linear_fwd, bias with and without ReLU, under every forced tile; K = 128 keeps tile 7 on its ping-pong loop."""
    _linear_fwd_case(L, pads, 256, 256, 128)


def test_linear_fwd_odd_k_tiles(L, pads):
    """Tile 7 with an odd number of K tiles (K = 192) falls back from the ping-pong loop to the two-slot ring."""
    L.rv_gemm_force_tile(7)
    try:
        _linear_fwd_case(L, pads, 256, 256, 192)
    finally:
        L.rv_gemm_force_tile(-1)


def _linear_fwd_f32_case(L, pads, M, N, K, splits):
    rng = np.random.default_rng(7)
    x, w = rand_bf16(rng, (M, K)), rand_bf16(rng, (N, K))
    b = rng.standard_normal(N).astype(np.float32)
    ldx, ldw, ldy = K + pads[8][0], K + pads[8][1], N + pads[4][0]
    distinct((ldx, ldw, ldy), (K, N))
    X, W = guarded(M, K, ldx, BF, x), guarded(N, K, ldw, BF, w)
    xd, wd, bd = dev(x, BF), dev(w, BF), dev(b)
    slabs = {}
    for bias in (bd, None):
        Y, yp = guarded(splits * M, N, ldy, F32), packed((splits, M, N), F32)
        bp = None if bias is None else bias.data_ptr()
        L.rv_linear_fwd_f32(X.ptr, ldx, W.ptr, ldw, bp, M, N, K, splits, Y.ptr, ldy, sp())
        L.rv_linear_fwd_f32(xd.data_ptr(), K, wd.data_ptr(), K, bp, M, N, K, splits, yp.data_ptr(), N, sp())
        got = Y.slabs(splits)                      # slab s read from element offset s * M * ldy
        same_bits(got, yp, "y slabs")
        ref = f64(x) @ f64(w).T + (b if bias is not None else 0)
        np.testing.assert_allclose(got.sum(0).cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
        Y.assert_untouched("y slabs")
        slabs[bias is not None] = got
    # the bias is added in slab 0 only: every later slab is the same with and without it, slab 0 is not
    for s in range(1, splits):
        same_bits(slabs[True][s], slabs[False][s], "slab %d with / without bias" % s)
    assert not torch.equal(slabs[True][0], slabs[False][0])


@pytest.mark.parametrize("splits", [1, 2])
def test_linear_fwd_f32(L, tile, pads, splits):
    """rv_linear_fwd_f32: fp32 split-K slabs Mp * ldy apart, with and without bias, under every forced tile."""
    _linear_fwd_f32_case(L, pads, 256, 256, 128, splits)


def test_linear_fwd_f32_odd_k_tiles(L, pads):
    L.rv_gemm_force_tile(7)
    try:
        _linear_fwd_f32_case(L, pads, 256, 256, 192, 1)
    finally:
        L.rv_gemm_force_tile(-1)


def test_forward_tile_lists(L, pads):
    """The tile-list path (gemm_pp_persist_kernel: at least 512 tiles of 256 x 256) with all three leading dimensions
    strided: the same bits as the packed 128 x 128 tiles, the float64 reference on 64 sampled rows, gaps and guards of the
    whole output."""
    M, N, K = 16384, 2048, 128
    rng = np.random.default_rng(31)
    x, w = rand_bf16(rng, (M, K), 0.5), rand_bf16(rng, (N, K), 0.1)
    b = (rng.standard_normal(N) * 0.1).astype(np.float32)
    ldx, ldw, ldy = K + pads[8][0], K + pads[8][1], N + pads[8][2]
    distinct((ldx, ldw, ldy), (K, N))
    X, W, Y = guarded(M, K, ldx, BF, x), guarded(N, K, ldw, BF, w), guarded(M, N, ldy, BF)
    xd, wd, bd, yp = dev(x, BF), dev(w, BF), dev(b), packed((M, N), BF)
    L.rv_linear_fwd(X.ptr, ldx, W.ptr, ldw, bd.data_ptr(), M, N, K, 1, Y.ptr, ldy, sp())
    L.rv_gemm_force_tile(4)
    try:
        L.rv_linear_fwd(xd.data_ptr(), K, wd.data_ptr(), K, bd.data_ptr(), M, N, K, 1, yp.data_ptr(), N, sp())
    finally:
        L.rv_gemm_force_tile(-1)
    same_bits(Y.payload(), yp, "y")
    rows = rng.choice(M, 64, replace=False)
    ref = np.maximum(f64(x[rows]) @ f64(w).T + b, 0)
    np.testing.assert_allclose(host(Y.view[torch.from_numpy(rows).cuda()]), ref, rtol=1e-2, atol=1e-3)
    Y.assert_untouched("y")


def test_decode_out_loss_fwd(L, tile, pads):
    """rv_decode_out_loss_fwd with ragged valid extents: strided ldh, ldw, ldx, ld_recon, ld_dp4.  Rows [Bv, M) and columns
    [Sv, N) of recon stay sentinel, the padding of dP4 is zero, its gap stays sentinel, the partial tables are guarded."""
    from rawaudiovae_kelsey_amd._lib import gemm_tile
    M, N, K = 512, 256, 128
    Bv, Sv = M - 37, N - 5
    rng = np.random.default_rng(22)
    a, w = rand_bf16(rng, (M, K)), rand_bf16(rng, (N, K), 0.1)
    b = rng.standard_normal(N).astype(np.float32)
    x = rng.uniform(-1, 1, (Bv, Sv)).astype(np.float32)
    bm, bn = gemm_tile(M, N, 1)
    ldh, ldw, ld_dp4 = K + pads[8][0], K + pads[8][1], N + pads[8][2]
    ldx, ld_recon = Sv + pads[1][0], N + pads[1][1]     # fp32 at their exact shapes: any leading dimension
    distinct((ldh, ldw, ld_dp4, ldx, ld_recon), (K, N, Sv))
    A, W, X = guarded(M, K, ldh, BF, a), guarded(N, K, ldw, BF, w), guarded(Bv, Sv, ldx, F32, x)
    ad, wd, bd, xd = dev(a, BF), dev(w, BF), dev(b), dev(x)
    n_mse = (M // bm) * (N // bn)
    R, D = guarded(M, N, ld_recon, F32), guarded(M, N, ld_dp4, BF)
    MS, CS = guarded_flat(n_mse, F32), guarded_flat((M // bm) * N, F32)
    rp, dp, msp, csp = packed((Bv, Sv), F32), packed((M, N), BF), packed((n_mse,), F32), packed((M // bm, N), F32)
    L.rv_decode_out_loss_fwd(A.ptr, ldh, W.ptr, ldw, bd.data_ptr(), M, N, K, Bv, Sv, X.ptr, ldx, R.ptr, ld_recon, D.ptr, ld_dp4,
                             MS.ptr, CS.ptr, sp())
    L.rv_decode_out_loss_fwd(ad.data_ptr(), K, wd.data_ptr(), K, bd.data_ptr(), M, N, K, Bv, Sv, xd.data_ptr(), Sv,
                             rp.data_ptr(), Sv, dp.data_ptr(), N, msp.data_ptr(), csp.data_ptr(), sp())
    recon = R.payload()
    same_bits(recon[:Bv, :Sv], rp, "recon")
    same_bits(D.payload(), dp, "dP4")
    same_bits(MS.payload().view(-1), msp, "mse partials")
    same_bits(CS.payload().view(M // bm, N), csp, "db4 partials")
    # the rows and columns of recon beyond the valid extents belong to nobody: still the sentinel
    assert bool((recon[Bv:] == R.fill).all()) and bool((recon[:, Sv:] == R.fill).all())
    rec = np.tanh(f64(a) @ f64(w).T + b)[:Bv, :Sv]
    np.testing.assert_allclose(host(recon[:Bv, :Sv]), rec, atol=2e-6)
    mse = ((rec - x) ** 2).sum()
    assert abs(float(MS.payload().double().sum()) - mse) <= 1e-5 * mse
    g = np.zeros((M, N))
    g[:Bv, :Sv] = 2.0 / (Bv * Sv) * (rec - x) * (1 - rec ** 2)
    got = host(D.payload())
    assert np.abs(got - g).max() <= 2 ** -7 * np.abs(g).max()
    assert not got[Bv:].any() and not got[:, Sv:].any()
    cs = CS.payload().view(M // bm, N).sum(0).cpu().numpy()
    np.testing.assert_allclose(cs, g.sum(0), rtol=2e-3, atol=2e-3 * np.abs(g.sum(0)).max())
    for t, name in ((R, "recon"), (D, "dP4"), (MS, "mse partials"), (CS, "db4 partials")):
        t.assert_untouched(name)


# ------------------------------------------------------------------------------------------------ backward GEMMs

@pytest.mark.parametrize("splits", [1, 2])
def test_linear_dgrad_f32(L, tile, pads, splits):
    """rv_linear_dgrad, the fp32 slab form: dX[M,N] = dY[M,K] @ W[K,N], slabs Mp * lddx32 apart."""
    M, N, K = 256, 256, 128
    rng = np.random.default_rng(11)
    dy, w = rand_bf16(rng, (M, K)), rand_bf16(rng, (K, N))
    lddy, ldw, lddx = K + pads[8][0], N + pads[8][1], N + pads[4][0]
    distinct((lddy, ldw, lddx), (K, N))
    DY, W, DX = guarded(M, K, lddy, BF, dy), guarded(K, N, ldw, BF, w), guarded(splits * M, N, lddx, F32)
    dyd, wd, dxp = dev(dy, BF), dev(w, BF), packed((splits, M, N), F32)
    L.rv_linear_dgrad(DY.ptr, lddy, W.ptr, ldw, M, N, K, None, 0, None, 0, None, DX.ptr, lddx, splits, sp())
    L.rv_linear_dgrad(dyd.data_ptr(), K, wd.data_ptr(), N, M, N, K, None, 0, None, 0, None, dxp.data_ptr(), N, splits, sp())
    got = DX.slabs(splits)
    same_bits(got, dxp, "dx slabs")
    ref = f64(dy) @ f64(w)
    np.testing.assert_allclose(got.sum(0).cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    DX.assert_untouched("dx slabs")


def test_linear_dgrad_mask_colsum(L, tile, pads):
    """rv_linear_dgrad, the ReLU-mask + column-sum form: strided lddy, ldw, ldmask, lddx, the partials guarded."""
    from rawaudiovae_kelsey_amd._lib import gemm_tile
    M, N, K = 256, 256, 128
    rng = np.random.default_rng(12)
    dy, w = rand_bf16(rng, (M, K)), rand_bf16(rng, (K, N))
    h = O.bf16_round(np.maximum(rng.standard_normal((M, N)), 0).astype(np.float32))
    bm = gemm_tile(M, N, 1)[0]
    lddy, ldw, ldmask, lddx = K + pads[8][0], N + pads[8][1], N + pads[8][2], N + pads[8][3]
    distinct((lddy, ldw, ldmask, lddx), (K, N))
    DY, W, H = guarded(M, K, lddy, BF, dy), guarded(K, N, ldw, BF, w), guarded(M, N, ldmask, BF, h)
    DX, CS = guarded(M, N, lddx, BF), guarded_flat((M // bm) * N, F32)
    dyd, wd, hd, dxp, csp = dev(dy, BF), dev(w, BF), dev(h, BF), packed((M, N), BF), packed((M // bm, N), F32)
    L.rv_linear_dgrad(DY.ptr, lddy, W.ptr, ldw, M, N, K, H.ptr, ldmask, DX.ptr, lddx, CS.ptr, None, 0, 1, sp())
    L.rv_linear_dgrad(dyd.data_ptr(), K, wd.data_ptr(), N, M, N, K, hd.data_ptr(), N, dxp.data_ptr(), N, csp.data_ptr(), None, 0, 1,
                      sp())
    same_bits(DX.payload(), dxp, "dx")
    same_bits(CS.payload().view(M // bm, N), csp, "column sums")
    ref = (f64(dy) @ f64(w)) * (h > 0)
    assert np.abs(host(DX.payload()) - ref).max() <= 2 ** -7 * np.abs(ref).max()
    np.testing.assert_allclose(CS.payload().view(M // bm, N).sum(0).cpu().numpy(), ref.sum(0), rtol=1e-4,
                               atol=1e-4 * np.abs(ref.sum(0)).max())
    DX.assert_untouched("dx")
    CS.assert_untouched("column sums")


@pytest.mark.parametrize("splits", [1, 2])
def test_linear_wgrad_f32(L, tile, pads, splits):
    """rv_linear_wgrad, fp32 slabs: dW[M,N] = dY[K,M]^T @ X[K,N] (K the batch), slabs Mp * lddw apart."""
    M, N, K = 256, 256, 128
    rng = np.random.default_rng(13)
    dy, x = rand_bf16(rng, (K, M)), rand_bf16(rng, (K, N))
    lddy, ldx, lddw = M + pads[8][0], N + pads[8][1], N + pads[4][0]
    distinct((lddy, ldx, lddw), (M, N))
    DY, X, DW = guarded(K, M, lddy, BF, dy), guarded(K, N, ldx, BF, x), guarded(splits * M, N, lddw, F32)
    dyd, xd, dwp = dev(dy, BF), dev(x, BF), packed((splits, M, N), F32)
    L.rv_linear_wgrad(DY.ptr, lddy, X.ptr, ldx, M, N, K, splits, -1, DW.ptr, lddw, 0, None, sp())
    L.rv_linear_wgrad(dyd.data_ptr(), M, xd.data_ptr(), N, M, N, K, splits, -1, dwp.data_ptr(), N, 0, None, sp())
    got = DW.slabs(splits)
    same_bits(got, dwp, "dw slabs")
    ref = f64(dy).T @ f64(x)
    np.testing.assert_allclose(got.sum(0).cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    DW.assert_untouched("dw slabs")


@pytest.mark.parametrize("named_tile", [0, 4, 2, 7], ids=["64x64", "128x128", "256x128", "256x256"])
def test_linear_wgrad_f16_slabs(L, pads, named_tile):
    """rv_linear_wgrad with RV_SLAB_F16, one case per tile family: the fp16 slabs are Mp * lddw fp16 elements apart, the
    table of unscale factors is packed and guarded.  Each dequantised slab against the float64 product of its own K range
    (test_fp16_gradient_slabs_track_the_gradients_magnitude's bound: 1e-3 of the norm of every 128-row block)."""
    M, N, K, splits = 256, 256, 256, 2
    rng = np.random.default_rng(17)
    dy, x = rand_bf16(rng, (K, M), 1e-3), rand_bf16(rng, (K, N), 0.5)
    lddy, ldx, lddw = M + pads[8][0], N + pads[8][1], N + pads[8][2]
    distinct((lddy, ldx, lddw), (M, N))
    DY, X, DW = guarded(K, M, lddy, BF, dy), guarded(K, N, ldx, BF, x), guarded(splits * M, N, lddw, F16)
    n_us = splits * (M // 32) * (N // 32)
    US = guarded_flat(n_us, F32)
    dyd, xd, dwp, usp = dev(dy, BF), dev(x, BF), packed((splits, M, N), F16), packed((n_us,), F32)
    L.rv_linear_wgrad(DY.ptr, lddy, X.ptr, ldx, M, N, K, splits, named_tile, DW.ptr, lddw, 1, US.ptr, sp())
    L.rv_linear_wgrad(dyd.data_ptr(), M, xd.data_ptr(), N, M, N, K, splits, named_tile, dwp.data_ptr(), N, 1, usp.data_ptr(), sp())
    got = DW.slabs(splits)
    same_bits(got, dwp, "fp16 dw slabs")
    same_bits(US.payload().view(-1), usp, "unscale table")
    us = US.payload().view(splits, M // 32, N // 32).cpu().numpy()
    assert np.all(us > 0) and np.all(np.log2(us) == np.round(np.log2(us)))   # exact powers of two
    deq = host(got) * np.repeat(np.repeat(us, 32, axis=1), 32, axis=2)
    ks = K // splits
    for s in range(splits):
        ref = f64(dy[s * ks:(s + 1) * ks]).T @ f64(x[s * ks:(s + 1) * ks])
        for r0 in range(0, M, 128):
            a, b = deq[s, r0:r0 + 128], ref[r0:r0 + 128]
            assert np.linalg.norm(a - b) <= 1e-3 * np.linalg.norm(b), (s, r0)
    DW.assert_untouched("fp16 dw slabs")
    US.assert_untouched("unscale table")


def _dgrad_wgrad_case(L, pads, M, N, K, want_paired, want_bm=None):
    from rawaudiovae_kelsey_amd._lib import dgrad_wgrad_pick
    rng = np.random.default_rng(41)
    dy, w = rand_bf16(rng, (M, K)), rand_bf16(rng, (K, N), 0.1)
    x = O.bf16_round(np.maximum(rng.standard_normal((M, N)), 0).astype(np.float32))
    paired, bm, splits = dgrad_wgrad_pick(M, N, K)
    assert paired == want_paired and (want_bm is None or bm == want_bm), (paired, bm, splits)
    lddy, ldw, ldx, lddx, lddw = K + pads[8][0], N + pads[8][1], N + pads[8][2], N + pads[8][3], N + pads[4][0]
    distinct((lddy, ldw, ldx, lddx, lddw), (M, N, K))
    DY, W, X = guarded(M, K, lddy, BF, dy), guarded(K, N, ldw, BF, w), guarded(M, N, ldx, BF, x)
    DX, CS, DW = guarded(M, N, lddx, BF), guarded_flat((M // bm) * N, F32), guarded(splits * K, N, lddw, F32)
    dyd, wd, xd = dev(dy, BF), dev(w, BF), dev(x, BF)
    dxp, csp, dwp = packed((M, N), BF), packed((M // bm, N), F32), packed((splits, K, N), F32)
    L.rv_linear_dgrad_wgrad(DY.ptr, lddy, W.ptr, ldw, X.ptr, ldx, M, N, K, DX.ptr, lddx, CS.ptr, DW.ptr, lddw, splits, 0, None, sp())
    L.rv_linear_dgrad_wgrad(dyd.data_ptr(), K, wd.data_ptr(), N, xd.data_ptr(), N, M, N, K, dxp.data_ptr(), N, csp.data_ptr(),
                            dwp.data_ptr(), N, splits, 0, None, sp())
    cs, dw = CS.payload().view(M // bm, N), DW.slabs(splits)     # dw slab s read from element offset s * K * lddw
    same_bits(DX.payload(), dxp, "dx")
    same_bits(cs, csp, "column sums")
    same_bits(dw, dwp, "dw slabs")
    ref_dx = (f64(dy) @ f64(w)) * (x > 0)
    ref_dw = f64(dy).T @ f64(x)
    assert np.abs(host(DX.payload()) - ref_dx).max() <= 2 ** -7 * np.abs(ref_dx).max()
    np.testing.assert_allclose(cs.sum(0).cpu().numpy(), ref_dx.sum(0), rtol=1e-4, atol=1e-4 * np.abs(ref_dx.sum(0)).max())
    np.testing.assert_allclose(dw.sum(0).cpu().numpy(), ref_dw, rtol=1e-5, atol=1e-5 * np.abs(ref_dw).max())
    for t, name in ((DX, "dx"), (CS, "column sums"), (DW, "dw slabs")):
        t.assert_untouched(name)


@pytest.mark.parametrize("force,loop", [(5, 102), (5, 108), (-1, 102)], ids=["paired-ring", "paired-pingpong", "unpaired"])
def test_linear_dgrad_wgrad(L, pads, force, loop):
    """rv_linear_dgrad_wgrad: the paired 256 x 256 launch with both main loops (forced) and the unpaired fallback, with
    lddy, ldw, ldx (mask AND wgrad operand), lddx and lddw strided; dW slabs Kp * lddw apart."""
    L.rv_gemm_force_tile(force)
    L.rv_gemm_force_tile(loop)       # 102: two-slot ring main loop, 108: ping-pong main loop
    try:
        _dgrad_wgrad_case(L, pads, 512, 256, 256, 1 if force == 5 else 0)
    finally:
        L.rv_gemm_force_tile(-1)
        L.rv_gemm_force_tile(108)    # the default


def test_linear_dgrad_wgrad_dual_launch(L, pads):
    """The heads' extents (K = 128): dgrad and wgrad share the 128 x 128 tile and go out in one dual launch."""
    _dgrad_wgrad_case(L, pads, 1024, 512, 128, 0, 128)


@pytest.mark.parametrize("M,N,K,ds,ws", [(512, 64, 256, 2, 4), (256, 256, 512, 1, 2)])
def test_linear_dgrad_wgrad_f32(L, pads, M, N, K, ds, ws):
    """rv_linear_dgrad_wgrad_f32: dX slabs Mp * lddx apart and dW slabs Kp * lddw apart, on the shared 64 x 64 tile (N = 64)
    and on 128 x 128 tiles (N = 256), with lddy, ldw, ldx, lddx and lddw strided."""
    rng = np.random.default_rng(43)
    dy, w, x = rand_bf16(rng, (M, K)), rand_bf16(rng, (K, N), 0.1), rand_bf16(rng, (M, N))
    lddy, ldw, ldx, lddx, lddw = K + pads[8][0], N + pads[8][1], N + pads[8][2], N + pads[4][0], N + pads[4][1]
    distinct((lddy, ldw, ldx, lddx, lddw), (M, N, K))
    DY, W, X = guarded(M, K, lddy, BF, dy), guarded(K, N, ldw, BF, w), guarded(M, N, ldx, BF, x)
    DX, DW = guarded(ds * M, N, lddx, F32), guarded(ws * K, N, lddw, F32)
    dyd, wd, xd, dxp, dwp = dev(dy, BF), dev(w, BF), dev(x, BF), packed((ds, M, N), F32), packed((ws, K, N), F32)
    L.rv_linear_dgrad_wgrad_f32(DY.ptr, lddy, W.ptr, ldw, X.ptr, ldx, M, N, K, DX.ptr, lddx, ds, DW.ptr, lddw, ws, sp())
    L.rv_linear_dgrad_wgrad_f32(dyd.data_ptr(), K, wd.data_ptr(), N, xd.data_ptr(), N, M, N, K, dxp.data_ptr(), N, ds,
                                dwp.data_ptr(), N, ws, sp())
    dx, dw = DX.slabs(ds), DW.slabs(ws)
    same_bits(dx, dxp, "dx slabs")
    same_bits(dw, dwp, "dw slabs")
    ref_dx, ref_dw = f64(dy) @ f64(w), f64(dy).T @ f64(x)
    np.testing.assert_allclose(dx.sum(0).cpu().numpy(), ref_dx, rtol=1e-5, atol=1e-5 * np.abs(ref_dx).max())
    np.testing.assert_allclose(dw.sum(0).cpu().numpy(), ref_dw, rtol=1e-5, atol=1e-5 * np.abs(ref_dw).max())
    DX.assert_untouched("dx slabs")
    DW.assert_untouched("dw slabs")


# ------------------------------------------------------------------------------------------------ the latent block

def _lp_of(Lt):
    return 64 if Lt <= 64 else 128 if Lt <= 128 else 256


@pytest.mark.parametrize("explicit_eps", [True, False], ids=["eps-given", "eps-generated"])
def test_heads_reparam_fwd(L, pads, explicit_eps):
    """rv_heads_reparam_fwd with strided ldh and ldw; the slab workspace, mu | logvar, z, the KL partials and eps_out have
    no leading dimension and sit between guards."""
    B, Lt, K, splits = 100, 3, 256, 2
    rng = np.random.default_rng(8)
    Bp, Lp = -(-B // 128) * 128, -(-Lt // 64) * 64
    h = np.zeros((Bp, K), np.float32); h[:B] = rand_bf16(rng, (B, K), 0.5)
    w = np.zeros((2 * Lp, K), np.float32)
    w[:Lt] = rand_bf16(rng, (Lt, K), 0.05); w[Lp:Lp + Lt] = rand_bf16(rng, (Lt, K), 0.05)
    bias = np.zeros(2 * Lp, np.float32)
    bias[:Lt] = rng.standard_normal(Lt) * 0.1; bias[Lp:Lp + Lt] = rng.standard_normal(Lt) * 0.1
    eps = rng.standard_normal((B, Lt)).astype(np.float32)
    ldh, ldw = K + pads[8][0], K + pads[8][1]
    distinct((ldh, ldw), (K, 2 * Lp))
    H, W = guarded(Bp, K, ldh, BF, h), guarded(2 * Lp, K, ldw, BF, w)
    hd, wd, bd, ed = dev(h, BF), dev(w, BF), dev(bias), dev(eps)
    E = guarded_flat(B * Lt, F32, eps)                 # eps_in between NaN guards
    ctr = torch.ones(1, dtype=torch.int64, device="cuda")
    n_kl = Bp * Lp // 1024
    sizes = (("slabs", splits * Bp * 2 * Lp, F32), ("mulv", Bp * 2 * Lp, F32), ("z", Bp * Lp, BF), ("kl", n_kl, F32),
             ("eps_out", B * Lt, F32))
    G = {n: guarded_flat(c, d) for n, c, d in sizes}
    P = {n: packed((c,), d) for n, c, d in sizes}
    if explicit_eps:
        L.rv_heads_reparam_fwd(H.ptr, ldh, W.ptr, ldw, bd.data_ptr(), Bp, Lp, K, B, Lt, splits, G["slabs"].ptr, E.ptr, None, 0,
                               ctr.data_ptr(), G["mulv"].ptr, G["z"].ptr, G["kl"].ptr, sp())
        L.rv_heads_reparam_fwd(hd.data_ptr(), K, wd.data_ptr(), K, bd.data_ptr(), Bp, Lp, K, B, Lt, splits, P["slabs"].data_ptr(),
                               ed.data_ptr(), None, 0, ctr.data_ptr(), P["mulv"].data_ptr(), P["z"].data_ptr(), P["kl"].data_ptr(), sp())
    else:
        L.rv_heads_reparam_fwd(H.ptr, ldh, W.ptr, ldw, bd.data_ptr(), Bp, Lp, K, B, Lt, splits, G["slabs"].ptr, None,
                               G["eps_out"].ptr, 77, ctr.data_ptr(), G["mulv"].ptr, G["z"].ptr, G["kl"].ptr, sp())
        L.rv_heads_reparam_fwd(hd.data_ptr(), K, wd.data_ptr(), K, bd.data_ptr(), Bp, Lp, K, B, Lt, splits, P["slabs"].data_ptr(),
                               None, P["eps_out"].data_ptr(), 77, ctr.data_ptr(), P["mulv"].data_ptr(), P["z"].data_ptr(),
                               P["kl"].data_ptr(), sp())
    for n in G:
        if n != "eps_out" or not explicit_eps:
            same_bits(G[n].payload().view(-1), P[n], n)
        G[n].assert_untouched(n)                       # (eps_out with eps given: not written at all)
    if explicit_eps:
        assert bool((G["eps_out"].payload() == G["eps_out"].fill).all())
    ref = f64(h[:B]) @ f64(w).T + bias
    mu, lv = ref[:, :Lt], ref[:, Lp:Lp + Lt]
    got = G["mulv"].payload().view(Bp, 2 * Lp).cpu().numpy()
    np.testing.assert_allclose(got[:B, :Lt], mu, rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(got[:B, Lp:Lp + Lt], lv, rtol=1e-5, atol=2e-5)
    assert not got[B:].any() and not got[:, Lt:Lp].any() and not got[:, Lp + Lt:].any()
    zg = host(G["z"].payload().view(Bp, Lp))
    if explicit_eps:
        zr = O.bf16_round((mu + eps * np.exp(0.5 * lv)).astype(np.float32))
        assert np.mean(zg[:B, :Lt] != zr) < 2e-3      # a last-bit fp32 difference may cross a bf16 rounding boundary
        np.testing.assert_allclose(zg[:B, :Lt], zr, rtol=1e-2, atol=1e-6)
    else:
        e2 = G["eps_out"].payload().view(B, Lt).cpu().numpy()
        assert abs(e2.mean()) < 0.05 + 2.0 / np.sqrt(e2.size) and abs(e2.std() - 1) < 0.1
        mv = got.astype(np.float64)
        z2 = O.bf16_round((mv[:B, :Lt] + e2 * np.exp(0.5 * mv[:B, Lp:Lp + Lt])).astype(np.float32))
        np.testing.assert_allclose(zg[:B, :Lt], z2, rtol=1e-2, atol=1e-6)
    kl_ref = float(np.sum(1 + lv - mu ** 2 - np.exp(lv)))
    assert abs(float(G["kl"].payload().double().sum()) - kl_ref) <= 1e-5 * abs(kl_ref) + 1e-4


LATENT_SHAPES = [(100, 3, 512), (100, 100, 512), (100, 200, 512)]
LATENT_IDS = ["row-local", "gemm-Lp128", "gemm-Lp256"]


@pytest.mark.parametrize("explicit_eps", [True, False], ids=["eps-given", "eps-generated"])
@pytest.mark.parametrize("B,Lt,H", LATENT_SHAPES, ids=LATENT_IDS)
def test_latent_fwd(L, pads, B, Lt, H, explicit_eps):
    """rv_latent_fwd in its row-local form and its GEMM forms at Lp = 128 / 256, with ldh, ldwh, ldw3, ldh3 strided; mu |
    logvar, z, the KL partials and eps_out between guards."""
    rng = np.random.default_rng(9)
    Bp, Lp, Hp = -(-B // 128) * 128, _lp_of(Lt), -(-H // 512) * 512
    h = np.zeros((Bp, Hp), np.float32); h[:B, :H] = np.maximum(rand_bf16(rng, (B, H), 0.5), 0)
    wh = np.zeros((2 * Lp, Hp), np.float32)
    wh[:Lt, :H] = rand_bf16(rng, (Lt, H), 0.05); wh[Lp:Lp + Lt, :H] = rand_bf16(rng, (Lt, H), 0.05)
    bh = np.zeros(2 * Lp, np.float32)
    bh[:Lt] = rng.standard_normal(Lt) * 0.1; bh[Lp:Lp + Lt] = rng.standard_normal(Lt) * 0.1
    w3 = np.zeros((Hp, Lp), np.float32); w3[:H, :Lt] = rand_bf16(rng, (H, Lt), 0.2)
    b3 = np.zeros(Hp, np.float32); b3[:H] = rng.standard_normal(H) * 0.1
    eps = rng.standard_normal((B, Lt)).astype(np.float32)
    ldh, ldwh, ldw3, ldh3 = Hp + pads[8][0], Hp + pads[8][1], Lp + pads[8][2], Hp + pads[8][3]
    distinct((ldh, ldwh, ldw3, ldh3), (Hp, Lp, 2 * Lp))
    Hh, WH, W3 = guarded(Bp, Hp, ldh, BF, h), guarded(2 * Lp, Hp, ldwh, BF, wh), guarded(Hp, Lp, ldw3, BF, w3)
    hd, whd, w3d, bhd, b3d, ed = dev(h, BF), dev(wh, BF), dev(w3, BF), dev(bh), dev(b3), dev(eps)
    E = guarded_flat(B * Lt, F32, eps)
    ctr = torch.ones(1, dtype=torch.int64, device="cuda")
    sizes = (("mulv", Bp * 2 * Lp, F32), ("z", Bp * Lp, BF), ("kl", Bp * Lp // 1024, F32), ("eps_out", B * Lt, F32))
    G = {n: guarded_flat(c, d) for n, c, d in sizes}
    P = {n: packed((c,), d) for n, c, d in sizes}
    H3, h3p = guarded(Bp, Hp, ldh3, BF), packed((Bp, Hp), BF)
    ein = (E.ptr, ed.data_ptr()) if explicit_eps else (None, None)
    eout = (None, None) if explicit_eps else (G["eps_out"].ptr, P["eps_out"].data_ptr())
    L.rv_latent_fwd(Hh.ptr, ldh, WH.ptr, ldwh, bhd.data_ptr(), W3.ptr, ldw3, b3d.data_ptr(), Bp, Hp, Lp, B, Lt, ein[0], eout[0], 77,
                    ctr.data_ptr(), G["mulv"].ptr, G["z"].ptr, G["kl"].ptr, H3.ptr, ldh3, sp())
    L.rv_latent_fwd(hd.data_ptr(), Hp, whd.data_ptr(), Hp, bhd.data_ptr(), w3d.data_ptr(), Lp, b3d.data_ptr(), Bp, Hp, Lp, B, Lt,
                    ein[1], eout[1], 77, ctr.data_ptr(), P["mulv"].data_ptr(), P["z"].data_ptr(), P["kl"].data_ptr(),
                    h3p.data_ptr(), Hp, sp())
    for n in G:
        if n != "eps_out" or not explicit_eps:
            same_bits(G[n].payload().view(-1), P[n], n)
        G[n].assert_untouched(n)
    same_bits(H3.payload(), h3p, "h3")
    H3.assert_untouched("h3")
    ref = f64(h[:B]) @ f64(wh).T + bh
    mu, lv = ref[:, :Lt], ref[:, Lp:Lp + Lt]
    got = G["mulv"].payload().view(Bp, 2 * Lp).cpu().numpy()
    np.testing.assert_allclose(got[:B, :Lt], mu, rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(got[:B, Lp:Lp + Lt], lv, rtol=1e-5, atol=2e-5)
    assert not got[B:].any() and not got[:, Lt:Lp].any() and not got[:, Lp + Lt:].any()
    e = eps if explicit_eps else G["eps_out"].payload().view(B, Lt).cpu().numpy()
    if not explicit_eps:
        assert abs(e.mean()) < 0.05 + 2.0 / np.sqrt(e.size) and abs(e.std() - 1) < 0.1
    za = host(G["z"].payload().view(Bp, Lp))
    zr = O.bf16_round((mu + e * np.exp(0.5 * lv)).astype(np.float32))
    assert np.mean(za[:B, :Lt] != zr) < 2e-3 and not za[B:].any() and not za[:, Lt:].any()
    np.testing.assert_allclose(za[:B, :Lt], zr, rtol=1e-2, atol=1e-6)
    kl_ref = float(np.sum(1 + lv - mu ** 2 - np.exp(lv)))
    assert abs(float(G["kl"].payload().double().sum()) - kl_ref) <= 1e-5 * abs(kl_ref) + 1e-4
    # fc3 on the kernel's own z (bf16) against float64: only the fp32 accumulation and the output rounding differ
    h3ref = np.maximum(f64(za[:B]) @ f64(w3).T + b3, 0)
    np.testing.assert_allclose(host(H3.payload())[:B], h3ref, rtol=1e-2, atol=1e-3)


@pytest.mark.parametrize("B,Lt,H", LATENT_SHAPES, ids=LATENT_IDS)
def test_latent_bwd(L, pads, B, Lt, H):
    """rv_latent_bwd in its three forms with z given (dW3 is produced): lddp, ldw3, ldz, lddw3 strided, dW3 slabs
    Hp * lddw3 apart; dmulv, the bias partials and the loss ring between guards.  Bounds: those of
    test_latent_bwd_one_launch_equals_two."""
    rng = np.random.default_rng(19)
    Bp, Lp, Hp, S = -(-B // 128) * 128, _lp_of(Lt), -(-H // 512) * 512, 512
    dp3 = np.zeros((Bp, Hp), np.float32); dp3[:B, :H] = rand_bf16(rng, (B, H), 1e-3)
    w3 = np.zeros((Hp, Lp), np.float32); w3[:H, :Lt] = rand_bf16(rng, (H, Lt), 0.2)
    mulv = np.zeros((Bp, 2 * Lp), np.float32)
    mulv[:B, :Lt] = rng.standard_normal((B, Lt)) * 0.5; mulv[:B, Lp:Lp + Lt] = rng.standard_normal((B, Lt)) * 0.3
    eps = rng.standard_normal((B, Lt)).astype(np.float32)
    n_mse, n_kl, kl_beta, w3s = 37, Bp // 16, 1e-2, 2
    msep = rng.random(n_mse).astype(np.float32); klp = -rng.random(n_kl).astype(np.float32)
    zz = np.zeros((Bp, Lp), np.float32); zz[:B, :Lt] = rand_bf16(rng, (B, Lt), 1.0)
    lddp, ldw3, ldz, lddw3 = Hp + pads[8][0], Lp + pads[8][1], Lp + pads[8][2], Lp + pads[4][0]
    distinct((lddp, ldw3, ldz, lddw3), (Hp, Lp, 2 * Lp))
    DP, W3, Z = guarded(Bp, Hp, lddp, BF, dp3), guarded(Hp, Lp, ldw3, BF, w3), guarded(Bp, Lp, ldz, BF, zz)
    MV, E = guarded_flat(Bp * 2 * Lp, F32, mulv), guarded_flat(B * Lt, F32, eps)
    MS, KL = guarded_flat(n_mse, F32, msep), guarded_flat(n_kl, F32, klp)
    dpd, w3d, zd, mvd, ed, msd, kld = dev(dp3, BF), dev(w3, BF), dev(zz, BF), dev(mulv), dev(eps), dev(msep), dev(klp)
    ctr = torch.full((1,), 3, dtype=torch.int64, device="cuda")
    sizes = (("dmulv", Bp * 2 * Lp, BF), ("dbh", (Bp // 16) * 2 * Lp, F32), ("loss", 16, F32))
    G = {n: guarded_flat(c, d) for n, c, d in sizes}
    P = {n: packed((c,), d) for n, c, d in sizes}
    DW, dwp = guarded(w3s * Hp, Lp, lddw3, F32), packed((w3s, Hp, Lp), F32)
    L.rv_latent_bwd(DP.ptr, lddp, W3.ptr, ldw3, Bp, Hp, Lp, B, Lt, S, MV.ptr, E.ptr, kl_beta, None, None, G["dmulv"].ptr,
                    G["dbh"].ptr, MS.ptr, n_mse, KL.ptr, n_kl, G["loss"].ptr, ctr.data_ptr(), 4, Z.ptr, ldz, DW.ptr, lddw3, w3s, sp())
    L.rv_latent_bwd(dpd.data_ptr(), Hp, w3d.data_ptr(), Lp, Bp, Hp, Lp, B, Lt, S, mvd.data_ptr(), ed.data_ptr(), kl_beta, None, None,
                    P["dmulv"].data_ptr(), P["dbh"].data_ptr(), msd.data_ptr(), n_mse, kld.data_ptr(), n_kl, P["loss"].data_ptr(),
                    ctr.data_ptr(), 4, zd.data_ptr(), Lp, dwp.data_ptr(), Lp, w3s, sp())
    same_bits(G["dmulv"].payload().view(-1), P["dmulv"], "dmulv")
    same_bits(G["dbh"].payload().view(-1), P["dbh"], "bias partials")
    # the loss ring [4][4]: slot (3 - 1) % 4 holds (total, mse, kld); nothing else of the ring is written
    loss, lossp = G["loss"].payload().view(4, 4), P["loss"].view(4, 4)
    same_bits(loss[2, :3], lossp[2, :3], "loss")
    assert bool((loss[[0, 1, 3]] == G["loss"].fill).all()) and float(loss[2, 0]) != G["loss"].fill
    dw = DW.slabs(w3s)                                  # slab s read from element offset s * Hp * lddw3
    same_bits(dw, dwp, "dW3 slabs")
    for n in G:
        G[n].assert_untouched(n)
    DW.assert_untouched("dW3 slabs")
    # float64 reference
    dz = f64(dp3[:B]) @ f64(w3[:, :Lt])
    mu, lv = f64(mulv[:B, :Lt]), f64(mulv[:B, Lp:Lp + Lt])
    sd = np.exp(0.5 * lv); ink = 1.0 / (B * Lt)
    dmu = dz + kl_beta * mu * ink
    dlv = dz * eps * 0.5 * sd + kl_beta * 0.5 * (sd * sd - 1) * ink
    g1 = host(G["dmulv"].payload().view(Bp, 2 * Lp))
    scale = f64(np.abs(dp3[:B])) @ f64(np.abs(w3[:, :Lt]))
    tol = 2.0 ** -8 * np.abs(dmu) + 1e-5 * scale + 1e-12   # one bf16 rounding + the fp32 accumulation
    assert (np.abs(g1[:B, :Lt] - dmu) <= tol).all()
    tol_v = 2.0 ** -8 * np.abs(dlv) + 1e-5 * scale * np.abs(eps) * sd + 1e-12
    assert (np.abs(g1[:B, Lp:Lp + Lt] - dlv) <= tol_v).all()
    assert not g1[B:].any() and not g1[:, Lt:Lp].any() and not g1[:, Lp + Lt:].any()
    ref_db = np.zeros((Bp, 2 * Lp)); ref_db[:B, :Lt] = dmu; ref_db[:B, Lp:Lp + Lt] = dlv
    ref_db = ref_db.reshape(Bp // 16, 16, 2 * Lp).sum(1)
    d1 = G["dbh"].payload().view(Bp // 16, 2 * Lp).cpu().numpy()
    if Lp > 64:   # the GEMM form: one partial row per 64-row tile in row 4 t of the table, zeros in rows 4 t + 1 .. + 3
        assert not d1.reshape(-1, 4, 2 * Lp)[:, 1:].any()
        d1, ref_db = d1.reshape(-1, 4, 2 * Lp).sum(1), ref_db.reshape(-1, 4, 2 * Lp).sum(1)
    np.testing.assert_allclose(d1, ref_db, rtol=1e-4, atol=1e-4 * np.abs(ref_db).max())
    ref_w3 = f64(dp3).T @ f64(zz)
    np.testing.assert_allclose(dw.double().sum(0).cpu().numpy(), ref_w3, rtol=1e-4, atol=1e-5 * np.abs(ref_w3).max())


@pytest.mark.parametrize("B,Lt,H", [(512, 64, 128), (1024, 17, 900)])
def test_heads_bwd(L, pads, B, Lt, H):
    """rv_heads_bwd with ldw, ldh, ldp, lddw strided: dWh slabs 128 * lddw apart, the bias partials between guards.  Bounds:
    those of test_heads_bwd_streaming_equals_the_dual_launch."""
    rng = np.random.default_rng(23)
    Bp, Lp, Hp = -(-B // 512) * 512, 64, -(-H // 128) * 128
    G_ = Bp // 512
    dm = np.zeros((Bp, 2 * Lp), np.float32)
    dm[:B, :Lt] = rand_bf16(rng, (B, Lt), 1e-3); dm[:B, Lp:Lp + Lt] = rand_bf16(rng, (B, Lt), 1e-3)
    wh = np.zeros((2 * Lp, Hp), np.float32)
    wh[:Lt, :H] = rand_bf16(rng, (Lt, H), 0.05); wh[Lp:Lp + Lt, :H] = rand_bf16(rng, (Lt, H), 0.05)
    h1 = np.zeros((Bp, Hp), np.float32); h1[:B, :H] = np.maximum(rand_bf16(rng, (B, H), 0.5), 0)
    ldw, ldh, ldp, lddw = Hp + pads[8][0], Hp + pads[8][1], Hp + pads[8][2], Hp + pads[4][0]
    distinct((ldw, ldh, ldp, lddw), (Hp, 2 * Lp))
    DM, WH, H1 = guarded_flat(Bp * 2 * Lp, BF, dm), guarded(2 * Lp, Hp, ldw, BF, wh), guarded(Bp, Hp, ldh, BF, h1)
    DP, DB, DW = guarded(Bp, Hp, ldp, BF), guarded_flat(G_ * Hp, F32), guarded(G_ * 2 * Lp, Hp, lddw, F32)
    dmd, whd, h1d = dev(dm, BF), dev(wh, BF), dev(h1, BF)
    dpp, dbp, dwp = packed((Bp, Hp), BF), packed((G_, Hp), F32), packed((G_, 2 * Lp, Hp), F32)
    L.rv_heads_bwd(DM.ptr, WH.ptr, ldw, H1.ptr, ldh, Bp, Hp, Lp, DP.ptr, ldp, DB.ptr, DW.ptr, lddw, sp())
    L.rv_heads_bwd(dmd.data_ptr(), whd.data_ptr(), Hp, h1d.data_ptr(), Hp, Bp, Hp, Lp, dpp.data_ptr(), Hp, dbp.data_ptr(),
                   dwp.data_ptr(), Hp, sp())
    db, dw = DB.payload().view(G_, Hp), DW.slabs(G_)       # slab g read from element offset g * 128 * lddw
    same_bits(DP.payload(), dpp, "dP1")
    same_bits(db, dbp, "db1 partials")
    same_bits(dw, dwp, "dWh slabs")
    for t, name in ((DP, "dP1"), (DB, "db1 partials"), (DW, "dWh slabs")):
        t.assert_untouched(name)
    ref = (f64(dm) @ f64(wh)) * (h1 > 0)
    got = host(DP.payload())
    np.testing.assert_allclose(got, ref, rtol=2.0 ** -7, atol=1e-5 * float(np.abs(ref).max()))
    assert not got[B:].any() and not got[:, H:].any()
    refw = f64(dm).T @ f64(h1)
    scale_w = float((f64(np.abs(dm)).T @ f64(np.abs(h1))).max())
    np.testing.assert_allclose(dw.double().sum(0).cpu().numpy(), refw, rtol=1e-4, atol=1e-5 * scale_w)
    np.testing.assert_allclose(db.double().sum(0).cpu().numpy(), ref.sum(0), rtol=1e-4,
                               atol=1e-5 * float(np.abs(ref).sum(0).max()) + 1e-12)


# ------------------------------------------------------------------------------------------------ cast

def test_cast_pad(L, pads):
    """rv_cast_pad_bf16 with ld_src > cols and ld_dst > cols_p at the shapes of test_cast_pad: exact bf16 rounding, zero
    padding, the gap of the destination and the guards untouched, the gap of the source not read."""
    rng = np.random.default_rng(3)
    for rows, cols, rp, cp in [(16, 64, 128, 128), (37, 100, 128, 128), (128, 256, 128, 256), (5, 7, 128, 128)]:
        a = rng.standard_normal((rows, cols)).astype(np.float32)
        ld_src, ld_dst = cols + pads[1][0], cp + pads[8][0]
        distinct((ld_src, ld_dst), (cols, cp))
        A, ad = guarded(rows, cols, ld_src, F32, a), dev(a)
        D, dp = guarded(rp, cp, ld_dst, BF, 9.0), packed((rp, cp), BF)
        ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
        L.rv_cast_pad_bf16(A.ptr, rows, cols, ld_src, D.ptr, rp, cp, ld_dst, ctr.data_ptr(), sp())
        L.rv_cast_pad_bf16(ad.data_ptr(), rows, cols, cols, dp.data_ptr(), rp, cp, cp, None, sp())
        same_bits(D.payload(), dp, "dst")
        got = host(D.payload())
        np.testing.assert_array_equal(got[:rows, :cols], O.bf16_round(a))
        assert np.all(got[rows:] == 0) and np.all(got[:, cols:] == 0)
        assert int(ctr.item()) == 1
        D.assert_untouched("dst")


# ------------------------------------------------------------------------------------------------ rejections

def test_leading_dimension_below_the_row_width_is_rejected(L):
    """A leading dimension smaller than the row it strides (rows would overlap) is RV_ERR_SHAPE before any launch, for every
    operand and output of the entry points that used to check `ld % 8` only.  Each call below is valid as written (and is
    first made that way); one leading dimension at a time is then lowered by one alignment unit below its width."""
    from rawaudiovae_kelsey_amd._lib import RvError, dgrad_wgrad_pick
    M, N, K = 256, 256, 512
    bf = torch.zeros(4 * 512 * 512, dtype=BF, device="cuda")       # every call stays inside these, valid or not
    f32 = torch.zeros(4 * 512 * 512, dtype=F32, device="cuda")
    b, f, s = bf.data_ptr(), f32.data_ptr(), sp()
    ob, f2, f3 = b + 2 * 2 * 512 * 512, f + 4 * 512 * 512, f + 4 * 2 * 512 * 512   # outputs apart from what is read
    _, _, psp = dgrad_wgrad_pick(M, N, K)
    # (function, arguments, {position of a leading dimension: its alignment unit})
    calls = [
        (L.rv_linear_fwd, [b, K, b, K, None, M, N, K, 1, ob, N, s], {1: 8, 3: 8, 10: 8}),
        (L.rv_linear_fwd_f32, [b, K, b, K, None, M, N, K, 2, f, N, s], {1: 8, 3: 8, 10: 4}),
        (L.rv_decode_out_loss_fwd, [b, K, b, K, None, M, N, K, M - 3, N - 5, f, N - 5, f2, N - 5, ob, N, f3, None, s],
         {1: 8, 3: 8, 11: 1, 13: 1, 15: 8}),
        (L.rv_linear_dgrad, [b, K, b, N, M, N, K, None, 0, None, 0, None, f, N, 2, s], {1: 8, 3: 8, 13: 4}),
        (L.rv_linear_dgrad, [b, K, b, N, M, N, K, b, N, ob, N, None, None, 0, 1, s], {1: 8, 3: 8, 8: 8, 10: 8}),
        (L.rv_linear_wgrad, [b, M, b, N, M, N, K, 2, -1, f, N, 0, None, s], {1: 8, 3: 8, 10: 4}),
        (L.rv_linear_wgrad, [b, M, b, N, M, N, K, 2, -1, ob, N, 1, f, s], {1: 8, 3: 8, 10: 8}),
        (L.rv_linear_dgrad_wgrad, [b, K, b, N, b, N, M, N, K, ob, N, None, f, N, psp, 0, None, s], {1: 8, 3: 8, 5: 8, 10: 8, 13: 4}),
        (L.rv_linear_dgrad_wgrad_f32, [b, K, b, N, b, N, M, N, K, f, N, 1, f2, N, 2, s], {1: 8, 3: 8, 5: 8, 10: 4, 13: 4}),
    ]
    for fn, args, lds in calls:
        fn(*args)
        for pos, unit in lds.items():
            bad = list(args)
            bad[pos] -= unit
            with pytest.raises(RvError, match="leading dim"):
                fn(*bad)
    # a packed per-split K share is not a row: the widths are those of the whole operand
    with pytest.raises(RvError, match="leading dim"):
        L.rv_linear_fwd_f32(b, K // 2, b, K, None, M, N, K, 2, f, N, s)
    torch.cuda.synchronize()
