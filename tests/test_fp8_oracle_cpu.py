"""tests/fp8_oracle.py itself: the e4m3 decoder and rounding against torch and the build's oracle, the float64 GEMM forms
against plain numpy, and -- the point of the helper -- planted errors in synthetic kernel outputs, each of which it must
flag, beside values that genuinely sit on a rounding boundary, which it must accept.  Also the reference-only check that the
boundary zones of `assert_image` stay under the 1 % cap at every shape tests/test_fp8_images_gpu.py runs."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import fp8_oracle as F  # noqa: E402
from oracle import vae_oracle as O  # noqa: E402
from oracle.inputs import make_eps, make_frames, make_params  # noqa: E402

ALL = torch.arange(256, dtype=torch.uint8)
FINITE = ALL[(ALL & 0x7F) != 0x7F]


def test_decoder_matches_torch_for_all_256_codes():
    want = ALL.view(torch.float8_e4m3fn).to(torch.float64)
    got = F.decode(ALL)
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(got).sum()) == 2
    assert torch.equal(got[FINITE.long()], want[FINITE.long()])
    assert float(got.nan_to_num().max()) == 448.0 and float(got[1]) == 2.0 ** -9


def test_every_code_is_a_fixed_point_of_both_roundings():
    v = F.decode(FINITE)
    assert torch.equal(F.e4m3_round(v), v)
    np.testing.assert_array_equal(O.fp8_e4m3_round(v.numpy().astype(np.float32)).astype(np.float64), v.numpy())
    back = F.encode(v)
    nz = v != 0
    assert torch.equal(back[nz], FINITE[nz]) and not back[~nz].any()


def test_rounding_matches_torch_and_the_oracle_between_the_codes():
    rng = np.random.default_rng(0)
    pos = F.decode(torch.arange(0, 127, dtype=torch.uint8)).numpy()
    mids = (pos[1:] + pos[:-1]) / 2                      # every rounding boundary, subnormal steps and 432 included
    y = np.concatenate([mids, np.nextafter(mids, 0), np.nextafter(mids, 1e9), rng.normal(0, 60, 20000),
                        rng.uniform(-0.05, 0.05, 20000), [448.0, 463.9, 500.0, 1e6, 0.0, 2.0 ** -10, 2.0 ** -10 * 1.0001]])
    y = np.concatenate([y, -y])
    got = F.e4m3_round(torch.from_numpy(y)).numpy()
    # (float32 inputs for the two others: the midpoints and their float64 neighbours are not all float32 values)
    y32 = y.astype(np.float32)
    got32 = F.e4m3_round(torch.from_numpy(y32.astype(np.float64))).numpy()
    np.testing.assert_array_equal(got32, O.fp8_e4m3_round(y32).astype(np.float64))
    t = torch.from_numpy(np.clip(y32, -448, 448)).to(torch.float8_e4m3fn).to(torch.float64).numpy()
    np.testing.assert_array_equal(got32, t)
    # ties go to the even code, and the float64 neighbours of a midpoint to either side of it
    n = len(mids)
    even = np.where((np.arange(n) % 2) == 0, pos[:-1], pos[1:])
    np.testing.assert_array_equal(got[:n], even)
    np.testing.assert_array_equal(got[n:2 * n], pos[:-1])
    np.testing.assert_array_equal(got[2 * n:3 * n], pos[1:])


def _images(seed=1, M=48, N=40, K=256):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: FINITE[torch.randint(0, len(FINITE), s, generator=g)]  # noqa: E731
    return r(M, K), r(N, K), r(K, N), r(M, N)


def test_gemm_forms_match_numpy():
    a, b, w, x = _images()
    A, B, W, X = (F.TABLE[t.numpy()] for t in (a, b, w, x))
    bias = torch.linspace(-3, 3, b.shape[0])
    np.testing.assert_allclose(F.fwd(a, b, 0.5, bias, relu=True).numpy(), np.maximum(0.5 * A @ B.T + bias.numpy().astype(np.float64), 0), rtol=1e-13)
    mask = torch.from_numpy(X > 0)
    np.testing.assert_allclose(F.dgrad(a, w, 0.25, mask).numpy(), 0.25 * (A @ W) * (X > 0), rtol=1e-13)
    parts = F.wgrad(a, x, 2.0, splits=4, summed=False)
    assert parts.shape == (4, a.shape[1], x.shape[1])
    np.testing.assert_allclose(parts.sum(0).numpy(), 2.0 * A.T @ X, rtol=1e-12)
    np.testing.assert_allclose(parts[1].numpy(), 2.0 * A[12:24].T @ X[12:24], rtol=1e-13)
    np.testing.assert_allclose(F.wgrad(a, x, 2.0).numpy(), 2.0 * A.T @ X, rtol=1e-12)
    np.testing.assert_allclose(F.abs_fwd(a, b, 0.5).numpy(), 0.5 * np.abs(A) @ np.abs(B).T, rtol=1e-13)
    np.testing.assert_allclose(F.abs_dgrad(a, w, 0.25).numpy(), 0.25 * np.abs(A) @ np.abs(W), rtol=1e-13)
    np.testing.assert_allclose(F.abs_wgrad(a, x, 2.0).numpy(), 2.0 * np.abs(A).T @ np.abs(X), rtol=1e-13)


# ---- planted errors: a synthetic "kernel output" is the float64 reference pushed through the output rounding

def _small_case():
    g = torch.Generator().manual_seed(7)
    ints = lambda *s: F.encode(torch.randint(-3, 4, s, generator=g).double())  # noqa: E731
    a, b = ints(64, 256), ints(32, 256)
    return a, b, F.fwd(a, b, 2.0 ** -6), F.abs_fwd(a, b, 2.0 ** -6)


K_BOUND = 4 * 2.0 ** -24      # the planted-error tests' accumulation allowance, in units of dq sum|a||b|


def test_one_dropped_product_is_flagged():
    a, b, ref, unit = _small_case()
    tol = K_BOUND * unit
    F.assert_close(ref.float(), ref, tol, "clean")
    r, c = 17, 5
    k = int((F.decode(a[r]) * F.decode(b[c])).abs().argmax())
    bad = ref.clone()
    bad[r, c] -= 2.0 ** -6 * float(F.decode(a[r, k]) * F.decode(b[c, k]))      # the kernel left product k out
    assert bad[r, c] != ref[r, c]
    with pytest.raises(AssertionError, match=r"1 of 2048 .*\(17, 5\)"):
        F.assert_close(bad.float(), ref, tol, "dropped product")
    assert F.accumulation_excess(bad.float(), ref, unit, torch.zeros_like(ref)) > 100 * K_BOUND


def test_one_zeroed_row_is_flagged():
    a, b, ref, unit = _small_case()
    bad = ref.float()
    bad[33] = 0
    with pytest.raises(AssertionError, match=r"\(33, "):
        F.assert_close(bad, ref, K_BOUND * unit, "zeroed row")
    # ... also through an fp8 image of the same output
    img = F.encode(ref * 4.3)        # (a scale off the dyadic grid: the integers of this case would all be ties)
    assert F.assert_image(img, ref, 4.3, K_BOUND * unit) < 0.01
    img[33] = 0
    with pytest.raises(AssertionError, match="neither rounding"):
        F.assert_image(img, ref, 4.3, K_BOUND * unit)


def test_one_code_off_away_from_a_boundary_is_flagged_and_a_value_on_a_boundary_is_accepted():
    # values in the middle of their rounding interval, one exactly on a boundary (a tie), one within delta of one
    ref = torch.tensor([[1.0, 1.06, 20.1, -0.011, 300.0, 1.0625, 1.0625 + 1e-7, 440.0, 1000.0, 0.0, 2.0 ** -10]], dtype=torch.float64)
    img = F.encode(ref)
    delta = 1e-5 * ref.abs()
    share = F.assert_image(img, ref, 1.0, delta)
    assert share == pytest.approx(3 / 11)                   # the tie, its neighbour, and the tie between 0 and 2^-9
    # the tie may have gone either way on the device: both neighbouring codes pass, and so does the near-tie's other side
    for j in (5, 6):
        other = img.clone()
        other[0, j] = int(img[0, j]) + (1 if F.decode(img[0, j]) < 1.09 else -1)
        assert float(F.decode(other[0, j])) in (1.0, 1.125)
        F.assert_image(other, ref, 1.0, delta)
    flip = img.clone(); flip[0, 10] = 1                    # 2^-10 is the tie between 0 and the first subnormal
    F.assert_image(flip, ref, 1.0, delta)
    # ... but two codes away does not, and nowhere else may a single code differ by one
    far = img.clone(); far[0, 5] = int(img[0, 5]) + 2
    with pytest.raises(AssertionError, match="neither rounding"):
        F.assert_image(far, ref, 1.0, delta)
    for j in (0, 1, 2, 3, 4, 7, 8, 9):
        for d in (1, -1):
            if (j in (8,) and d == 1) or (j == 9 and d == -1):
                continue                                    # past 448 lies the NaN code; below +0 there is no code
            up = img.clone()
            up[0, j] = int(img[0, j]) + d
            with pytest.raises(AssertionError):
                F.assert_image(up, ref, 1.0, delta)
    # saturation: everything beyond 448 is 448 and undecided about nothing; 440 is 8 above the boundary 432
    assert float(F.decode(img[0, 8])) == 448.0 and float(F.decode(img[0, 7])) == 448.0
    # a NaN code is never an image
    nan = img.clone(); nan[0, 0] = 0x7F
    with pytest.raises(AssertionError, match="NaN"):
        F.assert_image(nan, ref, 1.0, delta)
    # a delta wider than an e4m3 step is the caller's mistake, not an allowance
    with pytest.raises(AssertionError, match="more than one"):
        F.assert_image(img, ref, 1.0, 0.2 * ref.abs())


def test_keep_positive_floor():
    """A positive activation whose scaled value rounds to zero is held at 2^-9 (common.h, fp8_keep_positive)."""
    ref = torch.tensor([[1e-5, 0.0, 3e-3, 0.5]], dtype=torch.float64)
    pos = ref > 0
    img = torch.tensor([[1, 0, 2, 0x30]], dtype=torch.uint8)
    assert float(F.decode(img[0, 2])) == 2.0 ** -8 and float(F.decode(img[0, 3])) == 0.5
    F.assert_image(img, ref, 1.0, 1e-9, floor=pos)
    with pytest.raises(AssertionError):
        F.assert_image(img, ref, 1.0, 1e-9)                # without the floor 1e-5 rounds to zero
    lost = img.clone(); lost[0, 0] = 0
    with pytest.raises(AssertionError):
        F.assert_image(lost, ref, 1.0, 1e-9, floor=pos)


# ---- the reference alone: boundary zones at the shapes of tests/test_fp8_images_gpu.py

KL = 1e-4
C2 = (1024, 2048, 64, 4096)
# the three forward shapes, the picked large-batch shape, the backward shapes and C2 (there also dP1's image)
SHAPES = [(256, 384, 100, 130), (256, 512, 16, 1024), (512, 1024, 64, 2048), (256, 512, 16, 65536),
          (512, 2048, 64, 4096), (1024, 4096, 64, 2048), (1024, 2048, 64, 6144), C2]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_boundary_zone_share_of_the_reference_stays_under_the_cap(shape):
    """`assert_image` lets an element differ only inside a zone of width delta around a rounding boundary; its callers
    require that fewer than 1 % of the elements lie in such a zone.  With the deltas the device tests use -- the
    asserted accumulation bound of fc3 for h3 (in units of sum|z||w| + |b|), a few fp32 ulps for dP4 -- the oracle's own h3
    and dP4 at the test shapes (seeds 1234 / 4321, as there) are far below it: the estimate is 3e-4 at a delta of 1e-5.
    At C2, where the full step writes dP1 as fp8, also dP1 from the oracle's backward with the fp8 rounding points (scale
    2^26 and the reasoned bound of the heads' backward, as the device test)."""
    S, H, L, B = shape
    p = O.cast_params(make_params(S, H, L, 0), np.float32)
    x, eps = make_frames(B, S, 1234), make_eps(B, L, 4321)
    s_h3, s_dp4 = 32.0, 56.0 * B * S
    scales = {"x": 256.0, "w1": 224.0 / np.abs(p["fc1.weight"]).max(), "w4": 224.0 / np.abs(p["fc4.weight"]).max(), "h3": s_h3}
    c = O.forward(p, x, eps, quant="fp8", fp8_scales=scales)
    z, w3 = c["z"].astype(np.float64), O.bf16_round(p["fc3.weight"]).astype(np.float64)
    b3 = p["fc3.bias"].astype(np.float64)
    h3 = torch.from_numpy(np.maximum(z @ w3.T + b3, 0))
    unit = torch.from_numpy(np.abs(z) @ np.abs(w3).T + np.abs(b3))
    img = F.encode(torch.where(h3 > 0, (h3 * s_h3).clamp(min=F.E4M3_TINY), h3 * s_h3))      # (fp8_keep_positive)
    share = F.assert_image(img, h3, s_h3, F.ACC["fc3"] * unit + 2 * F.U * h3, floor=h3 > 0)
    assert share < 0.01, share
    rec = c["recon"].astype(np.float64)
    dp4 = torch.from_numpy(2.0 / (B * S) * (rec - x) * (1.0 - rec * rec))
    share4 = F.assert_image(F.encode(dp4 * s_dp4), dp4, s_dp4, 8 * 2.0 ** -24 * 2.0 / (B * S))
    assert share4 < 0.01, share4
    print("zone shares at %s: h3 %.2e, dP4 %.2e" % (shape, share, share4))
    if shape != C2:
        return
    # dP1 = (dmu W21 + dlv W22) * (h1 > 0) on the bf16 dmu | dlogvar of the fp8 backward (oracle/vae_oracle.py, backward)
    q, n_k, s_dp1 = O.bf16_round, B * L, 2.0 ** 26
    dP4 = O._q8(dp4.numpy().astype(np.float32), s_dp4)
    dP3 = q((dP4 @ O._q8(p["fc4.weight"], scales["w4"])) * (c["h3"] > 0))
    dz = dP3 @ q(p["fc3.weight"])
    dmu = q(dz + KL * c["mu"] / n_k).astype(np.float64)
    dlv = q(dz * c["eps"] * 0.5 * c["std"] + KL * 0.5 * (np.exp(c["logvar"]) - 1.0) / n_k).astype(np.float64)
    W21, W22 = q(p["fc21.weight"]).astype(np.float64), q(p["fc22.weight"]).astype(np.float64)
    mask = c["h1"] > 0
    dp1 = torch.from_numpy((dmu @ W21 + dlv @ W22) * mask)
    unit1 = torch.from_numpy((np.abs(dmu) @ np.abs(W21) + np.abs(dlv) @ np.abs(W22)) * mask)
    assert 8.0 < float(dp1.abs().max()) * s_dp1 <= 448.0
    share1 = F.assert_image(F.encode(dp1 * s_dp1), dp1, s_dp1, F.ACC["dp1"] * unit1 + F.U * dp1.abs())
    assert share1 < 0.01, share1
    print("zone share of dP1 at C2: %.2e" % share1)
