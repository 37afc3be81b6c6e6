"""Every fp8 (e4m3) GEMM launch of the training step against float64 on ITS OWN operand images.

tests/test_fp8_gpu.py holds the fp8 weight path to the oracle statistically, because the oracle recomputes the whole chain.
Here each launch is compared element by element with a float64 product of the very bytes it read out of the plan's
workspace (`xq`, `W1q`, `h3q`, `W4q`, `dP4q`, `dP1q`, the dequantisation scalars of `fp8_state`): what remains is fp32
accumulation order and the final rounding (tests/fp8_oracle.py).  Where a test can also WRITE those buffers, images of small
integers make the comparison bit exact.

Tolerances, per element, never a norm or a share (other than the boundary-zone rule of `assert_image`, capped at 1 %):
  bf16 outputs   2^-8 |ref| (bf16 rounding, ties included) + ACC[kind] * dq sum|a||b|
  recon          2e-6 (the tanh tolerance of test_gemm_strides_gpu.py::test_decode_out_loss_fwd) + ACC["fc4"] * dq sum|a||b|
  fp32 gradients ACC[kind] * dq sum|a||b| (+ 2^-11 of the 32 x 32 granule's maximum per fp16 slab: block-floating fp16
                 keeps 11 significant bits of the largest value of a granule)
  fp8 images     `assert_image`: equal to fp8(ref * scale) except within delta of a rounding boundary, there a neighbour
ACC (tests/fp8_oracle.py) is 4 x the largest accumulation error measured on an MI355X per launch kind, in 2^-24 units:
fc1 273 (68.2 measured), fc4 434 (108.3), dgrad 138 (34.4), fc4's wgrad 263 (65.6), fc1's wgrad 107 (26.6), the bf16 fc3 1
(0.22); profiles/fp8_images_summary.txt has every shape and tile.  Every test prints what it measured (`pytest -s`) and
requires it to stay under its ACC and under the any-order fp32 ceiling K * 2^-24; ACC itself stays under the ceiling of the
smallest K tested except for fc1 at K = 256 and fc4 at K = 384, where the f8f6f4 MFMA's own block sum -- not fp32
round-to-nearest steps -- already takes a quarter of the ceiling (fp8_oracle.ABOVE_CEILING: reported, not widened).

Which test runs which fp8 instantiation of csrc/gemm_launch.hip:
  launch_tile_fp8<EPI_BIAS_ACT_BF16>  64 x 64, 128 x 128, 256 x 128   test_forward_images[*-t0 / t1 / t2], test_integer_forward
                                      256 x 256 (forced)               test_fc1_forward_on_256x256_tiles (2 shapes), test_integer_forward[t7]
                                      256 x 256 (the picker's choice)  test_large_batch_fc1_takes_the_256x256_tile
  launch_tile_fp8<EPI_TANH_LOSS>      64 x 64, 128 x 128, 256 x 128   test_forward_images[*-t0 / t1 / t2], test_integer_forward
                                      (256 x 256 is never chosen for it: rv_gemm_tile_fp8_loss; a forced 7 is kept from it)
  launch_pair<8, true>                bf16 mask                        test_pair_backward (3 shapes x 2 slab types),
                                                                       test_integer_backward (2 shapes)
                                      fp8 mask (no_h3)                 test_full_step_fc1_weight_gradient (C2)
  gemm_wgrad_adam_kernel<8, true>                                      test_full_step_fc1_weight_gradient (C2)
fc1's fp8 weight gradient needs the single-call full step, so its operands cannot be planted between phases: it stays on the
operand-image check.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import fp8_oracle as F  # noqa: E402
from oracle.inputs import make_eps, make_frames, make_params  # noqa: E402

KL, LR = 1e-4, 1e-4
U = F.U
BF16_REL = 2.0 ** -8
TANH_TOL = 2e-6
ZONE_CAP = 0.01
TILE_IDS = {-1: "auto", 0: "t0", 1: "t1", 2: "t2", 7: "t7"}
TILE_DIMS = {0: (64, 64), 1: (128, 128), 2: (256, 128), 7: (256, 256)}

FWD_SHAPES = [(256, 384, 100, 130), (256, 512, 16, 1024), (512, 1024, 64, 2048)]
C2 = (1024, 2048, 64, 4096)
BWD_SHAPES = [(512, 2048, 64, 4096), (1024, 4096, 64, 2048), (1024, 2048, 64, 6144)]


def _lib():
    from rawaudiovae_kelsey_amd._lib import lib
    return lib()


def _engine(shape, fp8, params=None, **kw):
    """An engine created -- like every launch it then enqueues -- under the pinned tile: the plan sizes its partial-sum
    tables from the tiles the picker reports."""
    from rawaudiovae_kelsey_amd.engine import TrainEngine
    S, H, L, B = shape
    e = TrainEngine(S, H, L, B, kl_beta=KL, lr=LR, fp8=fp8, **kw)
    e.load_params(params if params is not None else make_params(S, H, L, 0))
    return e


def _inputs(shape):
    S, H, L, B = shape
    return torch.from_numpy(make_frames(B, S, 1234)).cuda(), torch.from_numpy(make_eps(B, L, 4321)).cuda()


def _fits(tile, M, N):
    bm, bn = TILE_DIMS[tile]
    return M % bm == 0 and N % bn == 0


def _note(kind, shape, tile, K, value):
    print("MEASURED %-6s shape %-28s tile %-4s K %5d: %8.3f x 2^-24 (asserted %.2f, ceiling %d)"
          % (kind, shape, TILE_IDS.get(tile, tile), K, value / U, F.ACC[kind] / U, K))
    assert value <= F.ACC[kind], "%s: measured accumulation error %.3f x 2^-24 units exceeds the asserted %.3f" % (
        kind, value / U, F.ACC[kind] / U)
    # the any-order fp32 ceiling: what was measured stays under it everywhere; the asserted 4 x does except where
    # F.ABOVE_CEILING says why not
    assert value <= F.ceiling(K), (kind, K, value / U)
    assert F.ACC[kind] <= F.ceiling(K) or K in F.ABOVE_CEILING.get(kind, ()), (kind, K)


def _spot(ref, rows, a, b, dq, what):
    """The device's float64 matmul against numpy on a few rows of the same product (a [M, K], b [K, N] decoded images)."""
    want = float(dq) * (a[rows].cpu().numpy() @ b.cpu().numpy())
    np.testing.assert_allclose(ref[rows].cpu().numpy(), want, rtol=1e-12, atol=1e-300, err_msg=what)


def _tile_max(a, bm, bn):
    M, N = a.shape
    return a.view(M // bm, bm, N // bn, bn).amax(dim=(1, 3)).flatten()


# ------------------------------------------------------------------------------------------------ forward, random data

def _check_cast(e, x):
    S, H, L, B = e.S, e.H, e.L, e.B
    Bp, Sp, Hp, Lp = e.padded()
    st = e.fp8_state()
    xq = e.buffer("xq", torch.uint8, (Bp, Sp))
    # x * s_x is exact in fp32 for the power-of-two scale of the frames, so the float64 rounding is the device's
    assert np.log2(st[0]) == round(np.log2(st[0]))
    assert torch.equal(F.decode(xq[:B, :S]), F.e4m3_round(x.double() * st[0])), "xq != fp8(x * s_x)"
    assert not xq[B:].any() and not xq[:, S:].any()
    # [5] = 1 / ([0][1]), [6] = 1 / ([3][2]): one fp32 product and one reciprocal (1 ulp) away from exact
    assert abs(st[5] * (st[0] * st[1]) - 1.0) <= 4 * U and abs(st[6] * (st[3] * st[2]) - 1.0) <= 4 * U, st


def _check_fc1(e, tile):
    S, H, L, B = e.S, e.H, e.L, e.B
    Bp, Sp, Hp, Lp = e.padded()
    st = e.fp8_state()
    xq, w1q = e.buffer("xq", torch.uint8, (Bp, Sp)), e.buffer("W1q", torch.uint8, (Hp, Sp))
    b1 = e.buffer("b1p", torch.float32, (Hp,))
    h1 = e.buffer("h1", torch.bfloat16, (Bp, Hp))
    ref = F.fwd(xq, w1q, st[5], b1, relu=True)
    unit = F.abs_fwd(xq, w1q, st[5])
    _spot(F.fwd(xq, w1q, st[5]), [0, B - 1, Bp - 1], F.decode(xq), F.decode(w1q).T.contiguous(), st[5], "fc1 reference")
    F.assert_close(h1, ref, BF16_REL * ref.abs() + F.ACC["fc1"] * unit, "h1")
    # padding: columns H.. have zero weights and bias -> 0; rows B.. read the zero frames -> relu(b1), as on the bf16 path
    assert not h1[:, H:].any()
    if Bp > B:
        assert torch.equal(h1[B:], b1.clamp(min=0).to(torch.bfloat16).expand(Bp - B, Hp))
    got = F.accumulation_excess(h1, ref, unit, F.bf16_half_ulp(h1) + U * ref.abs())
    _note("fc1", (S, H, L, B), tile, Sp, got)


def _rowlocal(e):
    """csrc/latent.hip, rv_latent_rowlocal: fc3 inside the row-local latent launch (else it is a GEMM of its own).  Copied by
    hand, as is the layout of "h3_amax" below: the plan decides in csrc/plan.hip, fwd_decide (8 maxima per 16 batch rows in
    the row-local form, else one per fc3 tile; the engines here leave RV_OPT_LATENT_FUSED at its default, and
    test_fc3_gemm_form_by_products, which does not, passes gemm_form itself).  If those conditions change, an h3_amax
    failure here means this copy is stale."""
    Bp, Sp, Hp, Lp = e.padded()
    return Lp == 64 and Hp % 512 == 0 and Hp <= 2048 and Bp <= 8192


def _check_fc3(e, tile, gemm_form, fc3_tile=None):
    S, H, L, B = e.S, e.H, e.L, e.B
    Bp, Sp, Hp, Lp = e.padded()
    st = e.fp8_state()
    z, w3 = e.buffer("z", torch.bfloat16, (Bp, Lp)).double(), e.buffer("W3b", torch.bfloat16, (Hp, Lp)).double()
    b3 = e.buffer("b3p", torch.float32, (Hp,)).double()
    h3, h3q = e.buffer("h3", torch.bfloat16, (Bp, Hp)), e.buffer("h3q", torch.uint8, (Bp, Hp))
    ref = (z @ w3.T + b3).clamp(min=0)
    unit = z.abs() @ w3.abs().T + b3.abs()
    delta = F.ACC["fc3"] * unit + 2 * U * ref                   # accumulation; bias add and the product with the scale
    F.assert_close(h3, ref, BF16_REL * ref + delta, "h3")
    # fp8_keep_positive: the image is the ReLU mask of fc4's fp8 backward
    img = F.decode(h3q)
    assert bool((img >= 0).all()) and torch.equal(img != 0, h3 > 0), "(h3q != 0) != (h3 > 0)"
    share = F.assert_image(h3q, ref, st[3], delta, floor=h3 > 0, what="h3q")
    assert share < ZONE_CAP, share
    # the maxima behind delayed scaling: per block of the GEMM form (in whatever order the blocks are numbered), per 16
    # rows -- 8 waves -- of the row-local form
    amax = e.buffer("h3_amax", torch.float32, (-1,)).double()
    if gemm_form:
        from rawaudiovae_kelsey_amd._lib import gemm_tile
        bm, bn = fc3_tile or gemm_tile(Bp, Hp, 1)
        n = (Bp // bm) * (Hp // bn)
        want, got = _tile_max(ref, bm, bn).sort().values, amax[:n].sort().values
    else:
        n = Bp // 16 * 8
        want, got = ref.view(Bp // 16, 16 * Hp).amax(1), amax[:n].view(Bp // 16, 8).amax(1)
    assert not amax[n:].any()
    tol = float(delta.max())
    assert float((got - want).abs().max()) <= tol, ("h3_amax", float((got - want).abs().max()), tol)
    assert abs(float(amax[:n].max()) - float(ref.max())) <= tol
    excess = F.accumulation_excess(h3, ref, unit, F.bf16_half_ulp(h3) + 2 * U * ref)
    _note("fc3", (S, H, L, B), tile, Lp, excess)
    print("ZONE h3q %s: %.2e" % ((S, H, L, B), share))


def _check_fc4(e, tile, x, recon, f8_bwd=False):
    S, H, L, B = e.S, e.H, e.L, e.B
    Bp, Sp, Hp, Lp = e.padded()
    st = e.fp8_state()
    h3q, w4q = e.buffer("h3q", torch.uint8, (Bp, Hp)), e.buffer("W4q", torch.uint8, (Sp, Hp))
    b4 = e.buffer("b4p", torch.float32, (Sp,))
    pre = F.fwd(h3q[:B], w4q[:S], st[6], b4[:S])
    unit = F.abs_fwd(h3q[:B], w4q[:S], st[6])
    _spot(F.fwd(h3q, w4q, st[6]), [0, B - 1], F.decode(h3q), F.decode(w4q).T.contiguous(), st[6], "fc4 reference")
    ref = torch.tanh(pre)
    F.assert_close(recon, ref, TANH_TOL + F.ACC["fc4"] * unit, "recon")
    # ... and everything behind recon on the device's own recon
    r, xd = recon.double(), x.double()
    d = r - xd
    mse = float(e.buffer("mse_part", torch.float32, (-1,)).double().sum())
    want = float((d * d).sum())
    # (per thread a few dozen fp32 additions, then a tree: 128 * 2^-24 relative covers the longest chain of the largest tile)
    assert abs(mse - want) <= 1e-5 * want, (mse, want)
    g = torch.zeros(Bp, Sp, dtype=torch.float64, device="cuda")
    g[:B, :S] = 2.0 / (B * S) * d * (1.0 - r * r)
    g_tol = 8 * U * 2.0 / (B * S)        # a few fp32 ulps of the largest possible |recon - x| * scale
    db4 = e.buffer("db4p", torch.float32, (-1, Sp)).double().sum(0)
    # column sums: at most 256 sequential fp32 additions per block (the row tile), partial rows added here in float64
    # (and every g carries the fp32 evaluation's error: 4 ulps of its own, 2 of scale * |recon - x| from 1 - recon^2)
    dpad = torch.zeros_like(g)
    dpad[:B, :S] = d.abs()
    F.assert_close(db4, g.sum(0), (256 + 8) * U * g.abs().sum(0) + 2 * U * 2.0 / (B * S) * dpad.sum(0), "db4 partials")
    dp4, dp4q = e.buffer("dP4", torch.bfloat16, (Bp, Sp)), e.buffer("dP4q", torch.uint8, (Bp, Sp))
    if f8_bwd:
        assert not dp4.any(), "the fp8 backward's forward wrote the bf16 dP4"
        share = F.assert_image(dp4q, g, st[12], g_tol, what="dP4q")
        assert share < ZONE_CAP, share
        assert not dp4q[B:].any() and not dp4q[:, S:].any()
        print("ZONE dP4q %s: %.2e" % ((S, H, L, B), share))
    else:
        assert not dp4q.any()
        F.assert_close(dp4, g, BF16_REL * g.abs() + g_tol, "dP4")
        assert not dp4[B:].any() and not dp4[:, S:].any()
    got = F.accumulation_excess(recon, ref, unit, torch.full_like(ref, TANH_TOL))
    _note("fc4", (S, H, L, B), tile, Hp, got)


def _forward(shape, tile, fused=True, mode="fwd"):
    from rawaudiovae_kelsey_amd import engine as E
    L_ = _lib()
    L_.rv_gemm_force_tile(tile)
    try:
        e = _engine(shape, mode)
        if not fused:
            e.set_latent_fused(False)
        e.set_fp8_scales(h3=32.0, freeze_h3=True)
        x, eps = _inputs(shape)
        recon = torch.zeros(shape[3], shape[0], device="cuda")
        e.step(x, eps, recon, phases=E.PHASE_FWD)
        torch.cuda.synchronize()
        from rawaudiovae_kelsey_amd._lib import gemm_tile
        fc3_tile = gemm_tile(e.padded()[0], e.padded()[2], 1)        # (under the pinned tile, as the launch chose it)
    finally:
        L_.rv_gemm_force_tile(-1)
    return e, x, recon, fc3_tile


def _forward_cases():
    from itertools import product
    out = []
    for (S, H, L, B), t in product(FWD_SHAPES, (-1, 0, 1, 2)):
        Bp, Sp, Hp = -(-B // 128) * 128, -(-S // 128) * 128, -(-H // 128) * 128
        # a pinned tile applies where it divides the extents of fc1 (Bp x Hp) or of fc4 (Bp x Sp)
        if t < 0 or _fits(t, Bp, Hp) or _fits(t, Bp, Sp):
            out.append(pytest.param((S, H, L, B), t, id="%dx%dx%dx%d-%s" % (S, H, L, B, TILE_IDS[t])))
    return out


@pytest.mark.parametrize("shape,tile", _forward_cases())
def test_forward_images(shape, tile):
    """One forward (`fp8="fwd"`, scales frozen at the refresh's values and a power of two for h3) under each tile
    `launch_tile_fp8` instantiates below 256 x 256: the cast, fc1, fc3's fp8 by-products and fc4 + loss, each against the
    device's own inputs to that launch."""
    e, x, recon, fc3_tile = _forward(shape, tile)
    assert tuple(e.padded()[:3]) == tuple(-(-v // 128) * 128 for v in (shape[3], shape[0], shape[1]))
    _check_cast(e, x)
    _check_fc1(e, tile)
    _check_fc3(e, tile, gemm_form=not _rowlocal(e), fc3_tile=fc3_tile)
    _check_fc4(e, tile, x, recon)


def test_fc3_gemm_form_by_products():
    """fc3 as a GEMM of its own (the fused latent launch switched off): the bias + ReLU epilogue writes h3's fp8 image and
    the per-block maxima (the row-local form is what test_forward_images runs at a padded latent width of 64)."""
    shape = (256, 512, 16, 1024)
    e, x, recon, fc3_tile = _forward(shape, -1, fused=False)
    _check_fc3(e, -1, gemm_form=True, fc3_tile=fc3_tile)
    _check_fc4(e, -1, x, recon)


@pytest.mark.parametrize("shape", [s for s in FWD_SHAPES if _fits(7, -(-s[3] // 128) * 128, -(-s[1] // 128) * 128)],
                         ids=lambda s: "%dx%dx%dx%d" % s)
def test_fc1_forward_on_256x256_tiles(shape):
    """`launch_tile_fp8` case 5 / 7, pinned at every forward shape whose fc1 extents it divides: the cast and fc1 alone (the
    fused loss has no 256 x 256 form on fp8 operands and the plan never sends it there, so the two launches behind fc1 are
    left out of this forward)."""
    from rawaudiovae_kelsey_amd import engine as E
    assert shape in FWD_SHAPES[1:]
    L_ = _lib()
    L_.rv_gemm_force_tile(7)
    try:
        e = _engine(shape, "fwd")
        e.set_fp8_scales(h3=32.0, freeze_h3=True)
        x, eps = _inputs(shape)
        L_.rv_plan_diag_skip(e._plan, 0b1100)          # slots 2 (latent forward) and 3 (fc4 + loss)
        e.step(x, eps, phases=E.PHASE_FWD)
        torch.cuda.synchronize()
    finally:
        L_.rv_gemm_force_tile(-1)
    _check_cast(e, x)
    _check_fc1(e, 7)


def test_large_batch_fc1_takes_the_256x256_tile():
    """The smallest batch at which the picker itself sends fc1's fp8 forward to 256 x 256 tiles (S = 256, H = 512), read
    from the picker: the whole forward there."""
    from rawaudiovae_kelsey_amd._lib import gemm_tile
    S, H, L = 256, 512, 16
    B = next(b for b in range(256, 1 << 20, 256) if gemm_tile(b, H, 1) == (256, 256))
    assert gemm_tile(B - 256, H, 1) != (256, 256) and B == 65536, B
    e, x, recon, _ = _forward((S, H, L, B), -1)
    _check_cast(e, x)
    _check_fc1(e, "t7*")
    _check_fc4(e, -1, x, recon)


# ------------------------------------------------------------------------------------------------ backward, random data

def _fp8_pair_fits(e):
    """rv_dgrad_wgrad_fp8_fits, from the picker and the conditions of plan.hip's fp8_bwd."""
    from rawaudiovae_kelsey_amd._lib import dgrad_wgrad_pick
    Bp, Sp, Hp, Lp = e.padded()
    paired, _, sp = dgrad_wgrad_pick(Bp, Hp, Sp)
    ok = bool(paired and Bp % 256 == 0 and Hp % 256 == 0 and Sp % 256 == 0 and (Sp // 128) % 2 == 0 and Bp % (128 * sp) == 0
              and (Bp // 128 // sp) % 2 == 0 and Bp // 128 // sp >= 2)
    return ok, sp


def _check_dgrad(e, w4q, mask, kind_shape):
    Bp, Sp, Hp, Lp = e.padded()
    st = e.fp8_state()
    dp4q = e.buffer("dP4q", torch.uint8, (Bp, Sp))
    dp3 = e.buffer("dP3", torch.bfloat16, (Bp, Hp))
    full = F.dgrad(dp4q, w4q, st[10], 1.0)
    _spot(full, [0, 257, Bp - 1], F.decode(dp4q), F.decode(w4q), st[10], "dgrad reference")
    ref, unit = full * mask, F.abs_dgrad(dp4q, w4q, st[10]) * mask
    assert not dp3[~mask].any(), "dP3 is not exactly zero where the mask is"
    F.assert_close(dp3, ref, BF16_REL * ref.abs() + F.ACC["dgrad"] * unit, "dP3")
    _note("dgrad", kind_shape, -1, Sp, F.accumulation_excess(dp3, ref, unit, F.bf16_half_ulp(dp3)))
    return ref, unit


@pytest.mark.parametrize("slab", ["fp32", "fp16"])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_pair_backward(shape, slab):
    """fc4's backward as the fp8 pair (`launch_pair<8, true>`), bf16 ReLU mask: dP3 against (h3 > 0) * dq[10] dP4q W4q, the
    finalized gradient of fc4.weight against dq[11] dP4q^T h3q (split-K slabs in fp32 and in block-floating fp16), fc3.bias
    against the column sums -- and the forward's own fp8 by-products at these shapes (dP4q through `assert_image`)."""
    from rawaudiovae_kelsey_amd import engine as E
    S, H, L, B = shape
    e = _engine(shape, "full", slab_dtype=slab)
    fits, sp = _fp8_pair_fits(e)
    assert fits, "the picker does not pair this shape on fp8 operands"
    e.set_fp8_scales(h3=32.0, freeze_h3=True)
    x, eps = _inputs(shape)
    recon = torch.zeros(B, S, device="cuda")
    e.step(x, eps, recon, phases=E.PHASE_FWD | E.PHASE_BWD_A | E.PHASE_FINALIZE_A)
    torch.cuda.synchronize()
    Bp, Sp, Hp, Lp = e.padded()
    st = e.fp8_state()
    assert abs(st[10] * (st[12] * st[2]) - 1.0) <= 4 * U and abs(st[11] * (st[12] * st[3]) - 1.0) <= 4 * U, st
    if slab == "fp32":
        _check_fc3(e, -1, gemm_form=not _rowlocal(e))
    _check_fc4(e, -1, x, recon, f8_bwd=True)            # asserts that dP4q was written and the bf16 dP4 left untouched
    # the loss ring's mse term (written by the latent backward from the forward's partials) on the device's own recon
    mse = float(((recon.double() - x.double()) ** 2).mean())
    assert abs(e.last_loss()[1] - mse) <= 1e-5 * mse, (e.last_loss(), mse)
    h3 = e.buffer("h3", torch.bfloat16, (Bp, Hp))
    h3q, w4q = e.buffer("h3q", torch.uint8, (Bp, Hp)), e.buffer("W4q", torch.uint8, (Sp, Hp))
    ref3, unit3 = _check_dgrad(e, w4q, h3 > 0, shape)
    gv = e.grad_views()
    # fc3.bias: column sums of the fp32 dP3 (before its bf16 rounding) -- 256 sequential additions per row tile
    F.assert_close(gv["fc3.bias"], ref3.sum(0)[:H], (F.ACC["dgrad"] * unit3.sum(0) + (256 + 8) * U * ref3.abs().sum(0))[:H], "db3")
    # fc4.weight
    dp4q = e.buffer("dP4q", torch.uint8, (Bp, Sp))
    parts = F.wgrad(dp4q, h3q, st[11], splits=sp, summed=False)
    ref, unit = parts.sum(0), F.abs_wgrad(dp4q, h3q, st[11])
    _spot(ref, [0, 129, Sp - 1], F.decode(dp4q).T.contiguous(), F.decode(h3q), st[11], "wgrad reference")
    tol = F.ACC["wgrad4"] * unit
    slab_tol = torch.zeros_like(unit)
    if slab == "fp16":
        gmax = parts.abs().view(sp, Sp // 32, 32, Hp // 32, 32).amax(dim=(2, 4))          # per slab and 32 x 32 granule
        slab_tol = (2.0 ** -11 * gmax.sum(0)).repeat_interleave(32, 0).repeat_interleave(32, 1)
    got = gv["fc4.weight"]
    F.assert_close(got, ref[:S, :H], (tol + slab_tol)[:S, :H], "fc4.weight gradient")
    _note("wgrad4", "%s %s" % (shape, slab), -1, Bp, F.accumulation_excess(got, ref[:S, :H], unit[:S, :H], slab_tol[:S, :H] + U * ref[:S, :H].abs()))


def test_full_step_fc1_weight_gradient():
    """The single-call full step at C2 (zero moments: exp_avg = 0.1f * g): fc1's weight gradient on fp8 operands
    (`gemm_wgrad_adam_kernel<8, true>`) against dq[15] dP1q^T xq, dP1's image against the heads' backward on the device's own
    dmu | dlogvar and head weights, its maxima behind h3's, fc4's dgrad with the ReLU mask read from h3's fp8 image (the bf16
    h3 is never written) against the weight image as it was BEFORE this step's update -- and, after a second, unfrozen step,
    the delayed scale of dP1.  fc1's operands cannot be planted (one call), so this launch stays on the image check."""
    shape = C2
    S, H, L, B = shape
    e = _engine(shape, "full", slab_dtype="fp32")
    assert _fp8_pair_fits(e)[0]
    s_dp1 = 2.0 ** 26          # about 56 B S / 4, as test_fp8_gpu.py: dP1's image then uses the format's range
    e.set_fp8_scales(h3=32.0, freeze_h3=True, dp1=s_dp1)
    Bp, Sp, Hp, Lp = e.padded()
    # (the optimizer riders of this very call rewrite the weight shadows: the images the backward read are today's)
    w4q_before = e.buffer("W4q", torch.uint8, (Sp, Hp)).clone()
    whb_before = e.buffer("Whb", torch.bfloat16, (2 * Lp, Hp)).double()
    x, eps = _inputs(shape)
    e.step(x, eps)
    torch.cuda.synchronize()
    st = e.fp8_state()
    assert st[13] == s_dp1 and abs(st[15] * (st[13] * st[0]) - 1.0) <= 4 * U
    # the fp8 forms ran: no bf16 dP4, h3, dP1 and no bf16 copy of the frames
    for name in ("dP4", "h3", "dP1", "xb"):
        assert not e.buffer(name, torch.bfloat16, (-1,)).any(), name
    h3q = e.buffer("h3q", torch.uint8, (Bp, Hp))
    _check_dgrad(e, w4q_before, F.decode(h3q) > 0, "C2 fp8 mask")
    # dP1's image
    dmulv, whb = e.buffer("dmulv", torch.bfloat16, (Bp, 2 * Lp)).double(), whb_before
    mask = e.buffer("h1", torch.bfloat16, (Bp, Hp)) > 0
    ref1, unit1 = (dmulv @ whb) * mask, (dmulv.abs() @ whb.abs()) * mask
    delta = F.ACC["dp1"] * unit1 + U * ref1.abs()
    dp1q = e.buffer("dP1q", torch.uint8, (Bp, Hp))
    share = F.assert_image(dp1q, ref1, st[13], delta, what="dP1q")
    assert share < ZONE_CAP, share
    assert 8.0 < float(F.decode(dp1q).abs().max()) <= 448.0
    print("ZONE dP1q: %.2e" % share)
    # its maxima: 8 waves per block of 512 rows x 64 columns (csrc/latent.hip, rv_heads_bwd_ex; the count is plan.hip's
    # n_amax_dp1), behind h3's 8 per 16 rows (plan.hip, fwd_decide) -- hand copies, like _rowlocal
    n3, n1 = Bp // 16 * 8, 8 * (Bp // 512) * (Hp // 64)
    amax = e.buffer("h3_amax", torch.float32, (-1,)).double()[n3:n3 + n1]
    got, want = amax.view(-1, 8).amax(1).sort().values, _tile_max(ref1.abs(), 512, 64).sort().values
    assert float((got - want).abs().max()) <= float(delta.max()), float((got - want).abs().max())
    # fc1.weight's gradient
    xq = e.buffer("xq", torch.uint8, (Bp, Sp))
    ref, unit = F.wgrad(dp1q, xq, st[15]), F.abs_wgrad(dp1q, xq, st[15])
    _spot(ref, [0, 1023, Hp - 1], F.decode(dp1q).T.contiguous(), F.decode(xq), st[15], "fc1 wgrad reference")
    got = e.view(e.exp_avg, "fc1.weight").double() / float(np.float32(0.1))
    F.assert_close(got, ref[:H, :S], F.ACC["wgrad1"] * unit[:H, :S] + 2 * U * ref[:H, :S].abs(), "fc1.weight gradient")
    _note("wgrad1", shape, -1, Bp, F.accumulation_excess(got, ref[:H, :S], unit[:H, :S], 3 * U * ref[:H, :S].abs()))
    # delayed scaling: the next step's first kernel turns the maxima above into dP1's scale
    e.set_fp8_scales(freeze_h3=False)
    e.step(torch.from_numpy(make_frames(B, S, 77)).cuda(), torch.from_numpy(make_eps(B, L, 78)).cuda())
    st2 = e.fp8_state()
    assert abs(st2[14] - float(ref1.abs().max())) <= float(delta.max()), (st2[14], float(ref1.abs().max()))
    assert abs(st2[13] * st2[14] / 224.0 - 1.0) <= 4 * U and abs(st2[15] * (st2[13] * st2[0]) - 1.0) <= 4 * U, st2
    assert np.isfinite(e.last_loss()[0])


# ------------------------------------------------------------------------------------------------ small-integer images: exact

def _ints(shape, seed, zero_rows=(), zero_cols=()):
    """e4m3 codes of random integers in {0, +-1, +-2, +-3} with some all-zero rows and columns (not aligned to 16)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-3, 4, shape, generator=g).double()
    for a, b in zero_rows:
        v[a:b] = 0
    for a, b in zero_cols:
        v[:, a:b] = 0
    return v.cuda()


@pytest.mark.parametrize("shape", BWD_SHAPES[:2], ids=lambda s: "%dx%dx%dx%d" % s)
def test_integer_backward(shape):
    """A forward takes the plan's decisions; then dP4q, W4q, h3q and the bf16 mask h3 are overwritten with small integers,
    [10] and [11] with powers of two, and fc4's backward runs alone (fp32 slabs).  Every partial sum is an integer far below
    2^24, so the result depends neither on the order of summation nor on the MFMA's internals: dP3 is the bf16 rounding of
    the exact product, the gradients of fc4.weight and fc3.bias are the exact ones -- bit for bit."""
    from rawaudiovae_kelsey_amd import engine as E
    from rawaudiovae_kelsey_amd._lib import PHASE_BWD_FC4, PHASE_FIN_FC4
    S, H, L, B = shape
    e = _engine(shape, "full", slab_dtype="fp32")
    assert _fp8_pair_fits(e)[0]
    x, eps = _inputs(shape)
    e.step(x, eps, phases=E.PHASE_FWD)
    Bp, Sp, Hp, Lp = e.padded()
    dy = _ints((Bp, Sp), 1, zero_rows=[(5, 23), (Bp - 301, Bp - 290)], zero_cols=[(100, 117)])
    w = _ints((Sp, Hp), 2, zero_rows=[(250, 263)], zero_cols=[(7, 9), (Hp - 133, Hp - 120)])
    a = _ints((Bp, Hp), 3, zero_rows=[(1000, 1037)], zero_cols=[(31, 50)])
    e.buffer("dP4q", torch.uint8, (Bp, Sp)).copy_(F.encode(dy))
    e.buffer("W4q", torch.uint8, (Sp, Hp)).copy_(F.encode(w))
    e.buffer("h3q", torch.uint8, (Bp, Hp)).copy_(F.encode(a))
    e.buffer("h3", torch.bfloat16, (Bp, Hp)).copy_(a)
    dq_d, dq_w = 2.0 ** -4, 2.0 ** -9
    st = e.buffer("fp8_state", torch.float32, (-1,))
    st[10], st[11] = dq_d, dq_w
    for name in ("dP3", "dW4", "db3p"):
        e.buffer(name, torch.uint8, (-1,)).fill_(0xFF)
    e.step(x, eps, phases=PHASE_BWD_FC4 | PHASE_FIN_FC4)
    torch.cuda.synchronize()
    assert e.fp8_state()[10] == dq_d and e.fp8_state()[11] == dq_w
    exact3 = torch.where(a > 0, dq_d * (dy @ w), torch.zeros_like(a))        # (the masked elements are +0)
    assert float(exact3.abs().max()) * 2 ** 4 < 2 ** 24
    dp3 = e.buffer("dP3", torch.bfloat16, (Bp, Hp))
    assert torch.equal(dp3.view(torch.int16), exact3.float().to(torch.bfloat16).view(torch.int16)), "dP3"
    db3 = e.buffer("db3p", torch.float32, (-1, Hp))[:Bp // 256]
    assert torch.equal(db3.double().sum(0), exact3.sum(0)) and torch.equal(db3.double(), exact3.view(Bp // 256, 256, Hp).sum(1)), "db3"
    exact_w = dq_w * (dy.T @ a)
    assert torch.equal(e.grad_views()["fc4.weight"].double(), exact_w[:S, :H]), "fc4.weight gradient"


@pytest.mark.parametrize("tile", [-1, 0, 1, 2, 7], ids=lambda t: TILE_IDS[t])
def test_integer_forward(tile):
    """Integer frames (x s_x in {0, +-1, +-2, +-3}), W1q and W4q written directly, scales frozen at powers of two: h1 must be
    the bf16 rounding of the exact dq sum + b1 bit for bit (b1 a multiple of dq, so the fp32 sum is exact too), and recon --
    on an h3q of integers, the three launches before fc4 left out of a second forward -- float64 tanh of the exact
    pre-activation within the tanh tolerance alone.  A pinned 256 x 256 tile is kept from the fused loss, which has no such
    form on fp8 operands."""
    from rawaudiovae_kelsey_amd import engine as E
    shape = (512, 1024, 64, 2048)
    S, H, L, B = shape
    rng = np.random.default_rng(5)
    p = make_params(S, H, L, 0)
    s_x, s_w, dq1 = 256.0, 64.0, 2.0 ** -14
    p["fc1.bias"] = (rng.integers(-40, 41, H) * dq1).astype(np.float32)
    L_ = _lib()
    L_.rv_gemm_force_tile(tile)
    try:
        e = _engine(shape, "fwd", params=p)
        e.set_fp8_scales(x=s_x, w1=s_w, w4=s_w, h3=32.0, freeze_h3=True)
        Bp, Sp, Hp, Lp = e.padded()
        assert (Bp, Sp, Hp) == (B, S, H)
        xi = _ints((B, S), 11, zero_rows=[(3, 20)], zero_cols=[(200, 231)])
        w1 = _ints((H, S), 12, zero_rows=[(77, 90)], zero_cols=[(5, 6)])
        e.buffer("W1q", torch.uint8, (Hp, Sp)).copy_(F.encode(w1))
        x = (xi / s_x).float()
        eps = _inputs(shape)[1]
        L_.rv_plan_diag_skip(e._plan, 0b1100 if tile == 7 else 0)
        e.step(x, eps, phases=E.PHASE_FWD)
        torch.cuda.synchronize()
        assert e.fp8_state()[5] == dq1
        assert torch.equal(F.decode(e.buffer("xq", torch.uint8, (Bp, Sp))), xi)
        exact = (dq1 * (xi @ w1.T) + torch.from_numpy(p["fc1.bias"]).cuda().double()).clamp(min=0)
        h1 = e.buffer("h1", torch.bfloat16, (Bp, Hp))
        assert torch.equal(h1.view(torch.int16), exact.float().to(torch.bfloat16).view(torch.int16)), "h1"
        if tile != 7:
            a = _ints((B, H), 13, zero_rows=[(500, 519)], zero_cols=[(1000, 1011)]).abs()
            w4 = _ints((S, H), 14, zero_rows=[(130, 141)], zero_cols=[(64, 81)])
            e.buffer("h3q", torch.uint8, (Bp, Hp)).copy_(F.encode(a))
            e.buffer("W4q", torch.uint8, (Sp, Hp)).copy_(F.encode(w4))
            dq4 = 2.0 ** -7
            e.buffer("fp8_state", torch.float32, (-1,))[6] = dq4       # (its writer, the cast launch, is left out below)
            recon = torch.zeros(B, S, device="cuda")
            L_.rv_plan_diag_skip(e._plan, 0b0111)                      # only slot 3: fc4 + tanh + loss
            e.step(x, eps, recon, phases=E.PHASE_FWD)
            torch.cuda.synchronize()
            pre = dq4 * (a @ w4.T) + e.buffer("b4p", torch.float32, (Sp,)).double()
            assert 0.5 < float(pre.std()) < 4.0
            F.assert_close(recon, torch.tanh(pre), TANH_TOL, "recon")
    finally:
        L_.rv_gemm_force_tile(-1)
