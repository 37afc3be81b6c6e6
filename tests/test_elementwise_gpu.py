"""The small entry points of csrc/elementwise.hip on their own, against float64 / exact fp32 numpy: until now they were
reached only through ops.py / strict.py and compared with other HIP routes.  Outputs sit between guard bands
(tests/guarded.py); sizes take in a ragged tail and a second trip of the grid-stride loops (the launchers cap the grid at
2048 blocks of 256 threads, 4096 for rv_tanh_bwd_pack)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from guarded import SENTINEL, guarded, guarded_flat  # noqa: E402
from oracle import vae_oracle as O  # noqa: E402

N_SIZES = [1, 1000, 2048 * 256 + 5]     # one thread, a ragged block, one element past a full first trip of the capped grid


@pytest.fixture(scope="module")
def L():
    from rawaudiovae_kelsey_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.lib()


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(dtype) if dtype is not None else t


def sp():
    return torch.cuda.current_stream().cuda_stream or None


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def flat_out(n):
    return guarded_flat(n, torch.float32)


def got_of(g):
    return g.payload().view(-1).cpu().numpy()


# ------------------------------------------------------------------------------------------------ rv_colsum_partial
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_colsum_partial(L, dtype, rows):
    """out[ry][col] = sum of rows [256 ry, 256 ry + 256) of column col, for strided sources (NaN in the gap columns) and
    strided outputs (guards), against the float64 sum of the block within 1e-5 of its term scale sum |x|."""
    rng = np.random.default_rng(rows)
    nblk = -(-rows // 256)
    for cols in (1, 63, 64, 65, 200):
        a = rng.standard_normal((rows, cols)).astype(np.float32)
        for ld, ld_out in ((cols, cols), (cols + 5, cols + 3)):
            src = guarded(rows, cols, ld, dtype, a)
            out = guarded(nblk, cols, ld_out, torch.float32)
            L.rv_colsum_partial(src.ptr, int(dtype == torch.bfloat16), rows, cols, ld, out.ptr, ld_out, sp())
            out.assert_untouched("colsum partials")
            x = src.payload().double().cpu().numpy()                       # the values as stored (bf16-rounded)
            pad = np.zeros((nblk * 256, cols)); pad[:rows] = x
            ref, scale = pad.reshape(nblk, 256, cols).sum(1), np.abs(pad).reshape(nblk, 256, cols).sum(1)
            got = out.payload().cpu().numpy().astype(np.float64)
            assert (np.abs(got - ref) <= 1e-5 * scale).all(), (rows, cols, ld, float(np.abs(got - ref).max()))
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError):
        L.rv_colsum_partial(src.ptr, 0, rows, cols, cols - 1, out.ptr, ld_out, sp())
    with pytest.raises(_lib.RvError):
        L.rv_colsum_partial(src.ptr, 0, rows, cols, ld, out.ptr, cols - 1, sp())


# ------------------------------------------------------------------------------------------------ rv_tanh_bwd_pack
@pytest.mark.parametrize("B,S,Bp,Sp", [(100, 1000, 128, 1024), (1, 1, 128, 128), (1152, 1024, 1152, 1024)])
def test_tanh_bwd_pack(L, B, S, Bp, Sp):
    """dP4 = d_recon * (1 - recon^2) as zero-padded bf16 [Bp, Sp]: within one bf16 rounding of float64 (2^-8 |ref|, plus
    2^-22 |d_recon| for the three fp32 roundings in front of it), recon = +-1 exactly included, padding exactly zero.  The
    last shape has more elements than the capped grid covers in one trip."""
    rng = np.random.default_rng(B + S)
    recon = np.tanh(2 * rng.standard_normal((B, S))).astype(np.float32)
    recon.reshape(-1)[::7] = 1.0
    recon.reshape(-1)[3::11] = -1.0
    d = (rng.standard_normal((B, S)) * 1e-3).astype(np.float32)
    dd, rd = dev(d), dev(recon)
    out = guarded_flat(Bp * Sp, torch.bfloat16)
    L.rv_tanh_bwd_pack(dd.data_ptr(), rd.data_ptr(), B, S, out.ptr, Bp, Sp, sp())
    out.assert_untouched("dP4")
    got = out.payload().view(Bp, Sp).float().cpu().numpy().astype(np.float64)
    ref = d.astype(np.float64) * (1.0 - recon.astype(np.float64) ** 2)
    assert (np.abs(got[:B, :S] - ref) <= 2.0 ** -8 * np.abs(ref) + 2.0 ** -22 * np.abs(d)).all()
    assert not got[B:].any() and not got[:, S:].any()
    assert not got[:B, :S][np.abs(recon) == 1.0].any()            # 1 - 1 * 1 is exact
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError):
        L.rv_tanh_bwd_pack(dd.data_ptr(), rd.data_ptr(), B, S, out.ptr, B - 1, Sp, sp())


# ------------------------------------------------------------------------------------------------ rv_ew_f32
@pytest.mark.parametrize("n", N_SIZES)
def test_ew_f32(L, n):
    """op 0: a (1 - b^2) within 2^-22 |a| of float64 (|b| <= 1 as a tanh output; the compiler may contract 1 - b * b);
    op 1: b > 0 ? a : 0 and op 2: a + b, bit-equal to numpy's fp32 -- -0.0, NaN and denormals in b (and a) for op 1."""
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    ad = dev(a)
    out = flat_out(n)
    # op 0
    y = np.tanh(b).astype(np.float32)
    yd = dev(y)
    L.rv_ew_f32(0, ad.data_ptr(), yd.data_ptr(), n, out.ptr, sp())
    out.assert_untouched("op 0")
    ref = a.astype(np.float64) * (1.0 - y.astype(np.float64) ** 2)
    assert (np.abs(got_of(out).astype(np.float64) - ref) <= 2.0 ** -22 * np.abs(a)).all()
    # op 1: special values at both ends and spread through the array
    b1, a1 = b.copy(), a.copy()
    special = np.array([-0.0, 0.0, np.nan, 1e-45, -1e-45, 1e-39, -1e-39, np.inf, -np.inf], dtype=np.float32)
    for k, v in enumerate(special):
        b1[k % n::max(1, n // 9) + 13] = v
    a1[::5] = np.float32(1e-40)        # a denormal gradient passes through unchanged
    a1[1::17] = np.float32(-0.0)
    out = flat_out(n)
    a1d, b1d = dev(a1), dev(b1)
    L.rv_ew_f32(1, a1d.data_ptr(), b1d.data_ptr(), n, out.ptr, sp())
    out.assert_untouched("op 1")
    with np.errstate(invalid="ignore"):
        ref1 = np.where(b1 > 0, a1, np.float32(0.0)).astype(np.float32)
    np.testing.assert_array_equal(bits(got_of(out)), bits(ref1))
    # op 2
    out = flat_out(n)
    bd = dev(b)
    L.rv_ew_f32(2, ad.data_ptr(), bd.data_ptr(), n, out.ptr, sp())
    out.assert_untouched("op 2")
    np.testing.assert_array_equal(bits(got_of(out)), bits(a + b))
    from rawaudiovae_kelsey_amd import _lib
    with pytest.raises(_lib.RvError):
        L.rv_ew_f32(3, ad.data_ptr(), bd.data_ptr(), n, out.ptr, sp())


# ------------------------------------------------------------------------------------------------ rv_reparameterize_bwd
@pytest.mark.parametrize("n", N_SIZES)
def test_reparameterize_bwd(L, n):
    """dmu = dz bit for bit; dlv = dz eps exp(logvar / 2) / 2 against float64 at test_reparameterize's bound for the same
    __expf expression (rtol 2e-6, atol 1e-6); a NULL output leaves the other one's call complete and its guards alone."""
    rng = np.random.default_rng(n + 1)
    dz, eps, lv = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    dzd, ed, lvd = dev(dz), dev(eps), dev(lv)
    ref = dz.astype(np.float64) * eps.astype(np.float64) * 0.5 * np.exp(0.5 * lv.astype(np.float64))
    for want_mu, want_lv in ((True, True), (True, False), (False, True)):
        dmu, dlv = flat_out(n), flat_out(n)
        L.rv_reparameterize_bwd(dzd.data_ptr(), ed.data_ptr(), lvd.data_ptr(), n, dmu.ptr if want_mu else None,
                                dlv.ptr if want_lv else None, sp())
        dmu.assert_untouched("dmu")
        dlv.assert_untouched("dlv")
        if want_mu:
            np.testing.assert_array_equal(bits(got_of(dmu)), bits(dz))
        else:
            assert (got_of(dmu) == SENTINEL).all()
        if want_lv:
            np.testing.assert_allclose(got_of(dlv), ref, rtol=2e-6, atol=1e-6)
        else:
            assert (got_of(dlv) == SENTINEL).all()


# ------------------------------------------------------------------------------------------------ rv_scale_by
@pytest.mark.parametrize("n", N_SIZES)
def test_scale_by(L, n):
    rng = np.random.default_rng(n + 2)
    a = rng.standard_normal(n).astype(np.float32)
    ad = dev(a)
    for g in (np.float32(0.37), np.float32(-3.0), np.float32(1.0)):
        gd = dev(np.array([g, 99.0], dtype=np.float32))           # (only scalar[0] is read)
        out = flat_out(n)
        L.rv_scale_by(ad.data_ptr(), gd.data_ptr(), n, out.ptr, sp())
        out.assert_untouched("scale_by")
        np.testing.assert_array_equal(bits(got_of(out)), bits(a * g))


# ------------------------------------------------------------------------------------------------ rv_reparam_fwd
@pytest.mark.parametrize("B,Lt,Lp,Bp", [(1000, 3, 64, 1024), (130, 129, 256, 256)], ids=lambda v: str(v))
@pytest.mark.parametrize("splits", [1, 3, 4, 5, 9])
def test_reparam_fwd_sums_its_slabs(L, splits, B, Lt, Lp, Bp):
    """rv_reparam_fwd on its own, with slab counts that run only the unrolled-by-four loop (4), only the remainder loop
    (1, 3) and both in one call (5, 9): mulv against the float64 sum of the slabs within splits * 2^-24 of the term scale,
    z and the KL partials by test_heads_reparam_fwd's checks."""
    rng = np.random.default_rng(splits * 1000 + B)
    slabs = (rng.standard_normal((splits, Bp, 2 * Lp)) * 0.3).astype(np.float32)
    eps = rng.standard_normal((B, Lt)).astype(np.float32)
    sd, ed = dev(slabs), dev(eps)
    mulv, z = guarded_flat(Bp * 2 * Lp, torch.float32), guarded_flat(Bp * Lp, torch.bfloat16)
    klp = guarded_flat(Bp * Lp // 1024, torch.float32)
    ctr = torch.ones(1, dtype=torch.int64, device="cuda")
    L.rv_reparam_fwd(sd.data_ptr(), splits, Bp, Lp, B, Lt, ed.data_ptr(), None, 0, ctr.data_ptr(), mulv.ptr, z.ptr, klp.ptr, sp())
    for g, name in ((mulv, "mulv"), (z, "z"), (klp, "kl_partial")):
        g.assert_untouched(name)
    s64 = slabs.astype(np.float64)
    ref, scale = s64.sum(0), np.abs(s64).sum(0)
    got = mulv.payload().view(Bp, 2 * Lp).cpu().numpy().astype(np.float64)
    mu, lv = ref[:B, :Lt], ref[:B, Lp:Lp + Lt]
    tol = splits * 2.0 ** -24 * scale
    assert (np.abs(got[:B, :Lt] - mu) <= tol[:B, :Lt]).all() and (np.abs(got[:B, Lp:Lp + Lt] - lv) <= tol[:B, Lp:Lp + Lt]).all()
    assert not got[B:].any() and not got[:, Lt:Lp].any() and not got[:, Lp + Lt:].any()
    zr = O.bf16_round((mu + eps * np.exp(0.5 * lv)).astype(np.float32))
    zg = z.payload().view(Bp, Lp).float().cpu().numpy()
    assert np.mean(zg[:B, :Lt] != zr) < 2e-3            # a last-bit fp32 difference may cross a bf16 rounding boundary
    np.testing.assert_allclose(zg[:B, :Lt], zr, rtol=1e-2, atol=1e-6)
    assert not zg[B:].any() and not zg[:, Lt:].any()
    kl = float(klp.payload().double().sum())
    kl_ref = float(np.sum(1 + lv - mu ** 2 - np.exp(lv)))
    assert abs(kl - kl_ref) <= 1e-5 * abs(kl_ref) + 1e-4


# ------------------------------------------------------------------------------------------------ the loss ring's slot
@pytest.mark.parametrize("route", ["reparam_bwd", "latent_bwd_rowlocal", "latent_bwd_gemm"])
@pytest.mark.parametrize("counter,slot", [(0, 3), (1, 0), (4, 3), (5, 0)])
def test_loss_ring_slot(L, route, counter, slot):
    """The loss scalar goes to slot ((*step_counter - 1) mod ring) of loss_out [ring][4], also for a counter of 0 -- C's
    `%` gave -1 there, a write 16 bytes in front of loss_out: slot ring - 1 = 3, guards untouched."""
    rng = np.random.default_rng(5)
    B, Lt, Lp, Bp, S, ring, kl_beta = 100, 3, 64, 128, 512, 4, 1e-2
    Hp = 512 if route == "latent_bwd_rowlocal" else 128
    mulv = np.zeros((Bp, 2 * Lp), np.float32)
    mulv[:B, :Lt] = rng.standard_normal((B, Lt)) * 0.5; mulv[:B, Lp:Lp + Lt] = rng.standard_normal((B, Lt)) * 0.3
    eps = rng.standard_normal((B, Lt)).astype(np.float32)
    n_mse, n_kl = 37, Bp // 16
    msep, klp = rng.random(n_mse).astype(np.float32), -rng.random(n_kl).astype(np.float32)
    mvd, ed, msed, kld = dev(mulv), dev(eps), dev(msep), dev(klp)
    dmulv = torch.empty(Bp, 2 * Lp, device="cuda", dtype=torch.bfloat16)
    dbh = torch.zeros(Bp // 16, 2 * Lp, device="cuda")
    ctr = torch.tensor([counter], dtype=torch.int64, device="cuda")
    loss = guarded_flat(4 * ring, torch.float32)
    if route == "reparam_bwd":
        slabs = dev((rng.standard_normal((1, Bp, Lp)) * 1e-3).astype(np.float32))
        L.rv_reparam_bwd(slabs.data_ptr(), 1, Bp, Lp, B, Lt, S, mvd.data_ptr(), ed.data_ptr(), kl_beta, None, None, dmulv.data_ptr(),
                         dbh.data_ptr(), msed.data_ptr(), n_mse, kld.data_ptr(), n_kl, loss.ptr, ctr.data_ptr(), ring, sp())
    else:
        dp3 = dev((rng.standard_normal((Bp, Hp)) * 1e-3).astype(np.float32), torch.bfloat16)
        w3 = dev((rng.standard_normal((Hp, Lp)) * 0.2).astype(np.float32), torch.bfloat16)
        L.rv_latent_bwd(dp3.data_ptr(), Hp, w3.data_ptr(), Lp, Bp, Hp, Lp, B, Lt, S, mvd.data_ptr(), ed.data_ptr(), kl_beta, None, None,
                        dmulv.data_ptr(), dbh.data_ptr(), msed.data_ptr(), n_mse, kld.data_ptr(), n_kl, loss.ptr, ctr.data_ptr(), ring,
                        None, 0, None, 0, 0, sp())
    loss.assert_untouched("loss_out")
    got = got_of(loss).reshape(ring, 4)
    others = [r for r in range(ring) if r != slot]
    assert (got[others] == SENTINEL).all() and got[slot, 3] == SENTINEL
    mse = msep.astype(np.float64).sum() / (B * S)
    kld_ = -0.5 * klp.astype(np.float64).sum() / (B * Lt)
    np.testing.assert_allclose(got[slot, :3], [mse + kl_beta * kld_, mse, kld_], rtol=1e-5)
    assert int(ctr.item()) == counter


def test_loss_finish_is_one_rule(L):
    """The three backward routes finish the loss scalar by one rule (csrc/reparam.h, loss_finish): on the same partial
    sums the three words they write to the ring's slot are equal as bits -- rv_reparam_bwd's extra block, the row-local
    rv_latent_bwd (Hp = 512) and its GEMM form (Hp = 128, the 512-thread k_dz_reparam_gemm<0>), at a counter of 0 (slot
    ring - 1) and of 5 (slot 0).  The guards around the ring and its other slots stay untouched."""
    rng = np.random.default_rng(5)
    B, Lt, Lp, Bp, S, ring, kl_beta = 100, 3, 64, 128, 512, 4, 1e-2
    mulv = np.zeros((Bp, 2 * Lp), np.float32)
    mulv[:B, :Lt] = rng.standard_normal((B, Lt)) * 0.5; mulv[:B, Lp:Lp + Lt] = rng.standard_normal((B, Lt)) * 0.3
    eps = rng.standard_normal((B, Lt)).astype(np.float32)
    n_mse, n_kl = 37, Bp // 16
    msep, klp = rng.random(n_mse).astype(np.float32), -rng.random(n_kl).astype(np.float32)
    mvd, ed, msed, kld = dev(mulv), dev(eps), dev(msep), dev(klp)
    slabs = dev((rng.standard_normal((1, Bp, Lp)) * 1e-3).astype(np.float32))
    dmulv = torch.empty(Bp, 2 * Lp, device="cuda", dtype=torch.bfloat16)
    dbh = torch.zeros(Bp // 16, 2 * Lp, device="cuda")

    def run(route, counter):
        ctr = torch.tensor([counter], dtype=torch.int64, device="cuda")
        loss = guarded_flat(4 * ring, torch.float32)
        if route == "reparam_bwd":
            L.rv_reparam_bwd(slabs.data_ptr(), 1, Bp, Lp, B, Lt, S, mvd.data_ptr(), ed.data_ptr(), kl_beta, None, None,
                             dmulv.data_ptr(), dbh.data_ptr(), msed.data_ptr(), n_mse, kld.data_ptr(), n_kl, loss.ptr,
                             ctr.data_ptr(), ring, sp())
        else:
            Hp = 512 if route == "latent_bwd_rowlocal" else 128
            dp3 = dev((rng.standard_normal((Bp, Hp)) * 1e-3).astype(np.float32), torch.bfloat16)
            w3 = dev((rng.standard_normal((Hp, Lp)) * 0.2).astype(np.float32), torch.bfloat16)
            L.rv_latent_bwd(dp3.data_ptr(), Hp, w3.data_ptr(), Lp, Bp, Hp, Lp, B, Lt, S, mvd.data_ptr(), ed.data_ptr(), kl_beta,
                            None, None, dmulv.data_ptr(), dbh.data_ptr(), msed.data_ptr(), n_mse, kld.data_ptr(), n_kl, loss.ptr,
                            ctr.data_ptr(), ring, None, 0, None, 0, 0, sp())
        loss.assert_untouched("loss_out (%s, counter %d)" % (route, counter))
        return got_of(loss).reshape(ring, 4)

    for counter, slot in ((0, 3), (5, 0)):
        got = {r: run(r, counter) for r in ("reparam_bwd", "latent_bwd_rowlocal", "latent_bwd_gemm")}
        first = got["reparam_bwd"]
        assert (first[slot, :3] != SENTINEL).all()
        for r, g in got.items():
            others = [s for s in range(ring) if s != slot]
            assert (g[others] == SENTINEL).all() and g[slot, 3] == SENTINEL, r
            np.testing.assert_array_equal(bits(g[slot, :3]), bits(first[slot, :3]), err_msg="%s, counter %d" % (r, counter))
