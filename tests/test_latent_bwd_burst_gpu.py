"""The streaming loops of the two backward latent launches (csrc/latent.hip: k_heads_bwd's tile loop, k_latent_bwd's dz
ring) run on COUNTED vmcnt waits: their transposing LDS reads are issued from assembly, so no full wait of the
compiler's stands between a slot's request and the tile two steps earlier.  A count that is one too loose then reads a
slot before it has landed, which shows as run-to-run differences before it shows as a wrong sum: every case runs twice
and must give the same bits, and is held to float64 numpy with the bounds of tests/test_kernels_gpu.py
(test_heads_bwd_streaming_equals_the_dual_launch, test_latent_bwd_one_launch_equals_two) at the smallest shapes that
reach every path: one, two and three row groups and column strips, every tile of every group on its own; 2, 4, 6 and 8
steps per wave; both row-group maps.

The fp16-slab instantiations of k_heads_bwd are reachable only through the step plan (rv_heads_bwd_ex is not exported):
tests/test_engine_gpu.py and tests/test_fp8_gpu.py hold them."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from guarded import guarded  # noqa: E402
from test_kernels_gpu import dev, rand_bf16, sp  # noqa: E402


@pytest.fixture(scope="module")
def L():
    from rawaudiovae_kelsey_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.lib()


# ---- rv_heads_bwd ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,Bp,Hp,pad", [(512, 512, 64, 0), (1024, 1024, 128, 0), (1536, 1536, 192, 0),
                                         (1000, 1024, 128, 0), (1024, 1024, 128, 64)],
                         ids=["1group-1strip", "2groups-2strips", "3groups-3strips", "padded-batch", "strided-guarded"])
def test_heads_bwd_every_tile_of_every_group(L, B, Bp, Hp, pad):
    """dP1, the fp32 dWh slab and the bias partial of EVERY 512-row group against float64 (an image or stage mix-up shows
    per tile and per group, so nothing is summed over groups first); padded rows are zero; with pad, h1 / dP1 / the
    slabs are strided views between guard bands (NaN around the input, a sentinel around the outputs)."""
    rng = np.random.default_rng(23 + Bp + Hp + pad)
    Lp, Lt, H, G = 64, 64, Hp, Bp // 512
    dm = np.zeros((Bp, 2 * Lp), np.float32)
    dm[:B, :Lt] = rand_bf16(rng, (B, Lt), 1e-3); dm[:B, Lp:Lp + Lt] = rand_bf16(rng, (B, Lt), 1e-3)
    wh = rand_bf16(rng, (2 * Lp, Hp), 0.05)
    h1 = np.zeros((Bp, Hp), np.float32); h1[:B, :H] = np.maximum(rand_bf16(rng, (B, H), 0.5), 0)
    ld = Hp + pad
    dmd, whd = dev(dm, torch.bfloat16), dev(wh, torch.bfloat16)
    H1 = guarded(Bp, Hp, ld, torch.bfloat16, h1)

    def run():
        DP = guarded(Bp, Hp, ld, torch.bfloat16)
        DB = guarded(G, Hp, Hp, torch.float32)
        DW = guarded(G * 2 * Lp, Hp, ld, torch.float32)
        L.rv_heads_bwd(dmd.data_ptr(), whd.data_ptr(), Hp, H1.ptr, ld, Bp, Hp, Lp, DP.ptr, ld, DB.ptr, DW.ptr, ld, sp())
        torch.cuda.synchronize()
        for o, name in ((DP, "dP1"), (DB, "db1_partial"), (DW, "dWh slabs")):
            o.assert_untouched(name)
        return DP.payload(), DB.payload(), DW.payload().view(G, 2 * Lp, Hp)
    dp1, db1, dwh = run()
    dp1b, db1b, dwhb = run()
    assert torch.equal(dp1, dp1b) and torch.equal(db1, db1b) and torch.equal(dwh, dwhb)   # run to run: the same bits

    d64, h64 = dm.astype(np.float64), h1.astype(np.float64)
    ref = (d64 @ wh.astype(np.float64)) * (h1 > 0)
    got = dp1.float().cpu().numpy()
    atol = 1e-5 * float(np.abs(ref).max())
    for t in range(Bp // 64):   # tile t % 8 of group t // 8
        rows = slice(64 * t, 64 * t + 64)
        np.testing.assert_allclose(got[rows], ref[rows], rtol=2.0 ** -7, atol=atol, err_msg="dP1, group %d tile %d" % (t // 8, t % 8))
    assert not got[B:].any()
    for g in range(G):
        rows = slice(512 * g, 512 * g + 512)
        refw = d64[rows].T @ h64[rows]
        scale_w = float((np.abs(d64[rows]).T @ np.abs(h64[rows])).max())
        np.testing.assert_allclose(dwh[g].double().cpu().numpy(), refw, rtol=1e-4, atol=1e-5 * scale_w, err_msg="dWh slab %d" % g)
        np.testing.assert_allclose(db1[g].double().cpu().numpy(), ref[rows].sum(0), rtol=1e-4,
                                   atol=1e-5 * float(np.abs(ref[rows]).sum(0).max()) + 1e-12, err_msg="db1 partial %d" % g)


# ---- rv_latent_bwd, row-local form ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,Bp,Hp,Lt,with_w3,ext", [
    (64, 64, 512, 64, True, False),      # 2 steps per wave: nothing is issued inside the loop; 4 row groups, the plain map
    (64, 64, 1024, 17, False, True),     # 4 steps
    (128, 128, 1536, 64, True, True),    # 6 steps; 8 row groups: the XCD placement map
    (128, 128, 2048, 64, True, False),   # 8 steps
    (128, 128, 2048, 17, False, False),
    (192, 192, 2048, 64, True, True),    # 12 row groups: not a power of two, the plain map
    (192, 192, 1024, 17, True, False),
    (100, 128, 1024, 64, True, True),    # B < Bp
    (50, 64, 2048, 17, False, True),
    (192, 192, 512, 64, False, False),
], ids=lambda v: str(v))
def test_latent_bwd_rowlocal(L, B, Bp, Hp, Lt, with_w3, ext):
    """dmulv, the head-bias partials, the dW3 slabs and the loss slot against float64 and the two-launch route, twice."""
    rng = np.random.default_rng(19 + Bp + Hp + Lt)
    Lp, S, H = 64, 512, Hp
    dp3 = np.zeros((Bp, Hp), np.float32); dp3[:B, :H] = rand_bf16(rng, (B, H), 1e-3)
    w3 = np.zeros((Hp, Lp), np.float32); w3[:H, :Lt] = rand_bf16(rng, (H, Lt), 0.2)
    mulv = np.zeros((Bp, 2 * Lp), np.float32)
    mulv[:B, :Lt] = rng.standard_normal((B, Lt)) * 0.5; mulv[:B, Lp:Lp + Lt] = rng.standard_normal((B, Lt)) * 0.3
    eps = rng.standard_normal((B, Lt)).astype(np.float32)
    xm = (rng.standard_normal((B, Lt)) * 1e-3).astype(np.float32) if ext else None
    xv = (rng.standard_normal((B, Lt)) * 1e-3).astype(np.float32) if ext else None
    n_mse, n_kl, kl_beta = 37, Bp // 16, 1e-2
    msep = rng.random(n_mse).astype(np.float32); klp = -rng.random(n_kl).astype(np.float32)
    dpd, w3d, mvd, ed = dev(dp3, torch.bfloat16), dev(w3, torch.bfloat16), dev(mulv), dev(eps)
    xmd, xvd = (dev(xm), dev(xv)) if ext else (None, None)
    msed, kld = dev(msep), dev(klp)
    ctr = torch.full((1,), 3, dtype=torch.int64, device="cuda")
    P = lambda t: None if t is None else t.data_ptr()
    zz = np.zeros((Bp, Lp), np.float32); zz[:B, :Lt] = rand_bf16(rng, (B, Lt), 1.0)
    zd = dev(zz, torch.bfloat16)
    w3s = 2 if Bp % 128 == 0 else 1

    def run():
        dm = torch.full((Bp, 2 * Lp), 7.0, device="cuda", dtype=torch.bfloat16)
        db = torch.zeros(Bp // 16, 2 * Lp, device="cuda")
        loss = torch.zeros(4, 4, device="cuda")
        dw3 = torch.full((w3s, Hp, Lp), 7.0, device="cuda")
        L.rv_latent_bwd(dpd.data_ptr(), Hp, w3d.data_ptr(), Lp, Bp, Hp, Lp, B, Lt, S, mvd.data_ptr(), ed.data_ptr(), kl_beta,
                        P(xmd), P(xvd), dm.data_ptr(), db.data_ptr(), msed.data_ptr(), n_mse, kld.data_ptr(), n_kl,
                        loss.data_ptr(), ctr.data_ptr(), 4, P(zd) if with_w3 else None, Lp, dw3.data_ptr() if with_w3 else None,
                        Lp, w3s if with_w3 else 0, sp())
        torch.cuda.synchronize()
        return dm, db, loss, dw3
    dm1, db1, loss1, dw3a = run()
    dmb, dbb, lossb, dw3c = run()
    assert torch.equal(dm1.view(torch.int16), dmb.view(torch.int16)) and torch.equal(db1, dbb)   # run to run: the same bits
    assert torch.equal(loss1, lossb) and torch.equal(dw3a, dw3c)
    # the two-launch route
    dm2 = torch.full((Bp, 2 * Lp), 7.0, device="cuda", dtype=torch.bfloat16)
    db2, loss2 = torch.zeros(Bp // 16, 2 * Lp, device="cuda"), torch.zeros(4, 4, device="cuda")
    slabs = torch.empty(4, Bp, Lp, device="cuda")
    L.rv_linear_dgrad(dpd.data_ptr(), Hp, w3d.data_ptr(), Lp, Bp, Lp, Hp, None, 0, None, 0, None, slabs.data_ptr(), Lp, 4, sp())
    L.rv_reparam_bwd(slabs.data_ptr(), 4, Bp, Lp, B, Lt, S, mvd.data_ptr(), ed.data_ptr(), kl_beta, P(xmd), P(xvd),
                     dm2.data_ptr(), db2.data_ptr(), msed.data_ptr(), n_mse, kld.data_ptr(), n_kl, loss2.data_ptr(),
                     ctr.data_ptr(), 4, sp())
    # float64
    dz = dp3[:B].astype(np.float64) @ w3[:, :Lt].astype(np.float64)
    mu, lv = mulv[:B, :Lt].astype(np.float64), mulv[:B, Lp:Lp + Lt].astype(np.float64)
    sd = np.exp(0.5 * lv); ink = 1.0 / (B * Lt)
    dmu = dz + kl_beta * mu * ink + (xm if ext else 0)
    dlv = dz * eps * 0.5 * sd + kl_beta * 0.5 * (sd * sd - 1) * ink + (xv if ext else 0)
    g1, g2 = dm1.float().cpu().numpy(), dm2.float().cpu().numpy()
    scale = np.abs(dp3[:B]).astype(np.float64) @ np.abs(w3[:, :Lt]).astype(np.float64)
    tol = 2.0 ** -8 * np.abs(dmu) + 1e-5 * scale + 1e-12   # one bf16 rounding + the fp32 accumulation
    assert (np.abs(g1[:B, :Lt] - dmu) <= tol).all()
    tol_v = 2.0 ** -8 * np.abs(dlv) + 1e-5 * scale * np.abs(eps) * sd + 1e-12
    assert (np.abs(g1[:B, Lp:Lp + Lt] - dlv) <= tol_v).all()
    assert not g1[B:].any() and not g1[:, Lt:Lp].any() and not g1[:, Lp + Lt:].any()
    assert np.mean(g1 != g2) < 0.05
    np.testing.assert_allclose(g1, g2, rtol=2.0 ** -7, atol=1e-5 * float(scale.max()))
    ref_db = np.zeros((Bp, 2 * Lp)); ref_db[:B, :Lt] = dmu; ref_db[:B, Lp:Lp + Lt] = dlv
    ref_db = ref_db.reshape(Bp // 16, 16, 2 * Lp).sum(1)
    np.testing.assert_allclose(db1.cpu().numpy(), ref_db, rtol=1e-4, atol=1e-4 * np.abs(ref_db).max())
    np.testing.assert_allclose(db1.cpu().numpy(), db2.cpu().numpy(), rtol=1e-4, atol=1e-4 * np.abs(ref_db).max())
    if with_w3:
        dw3b = torch.empty(w3s, Hp, Lp, device="cuda")
        L.rv_linear_wgrad(dpd.data_ptr(), Hp, zd.data_ptr(), Lp, Hp, Lp, Bp, w3s, -1, dw3b.data_ptr(), Lp, 0, None, sp())
        assert torch.equal(dw3a, dw3b)
        ref_w3 = dp3.astype(np.float64).T @ zz.astype(np.float64)
        np.testing.assert_allclose(dw3a.double().sum(0).cpu().numpy(), ref_w3, rtol=1e-4, atol=1e-5 * np.abs(ref_w3).max())
    else:
        assert bool((dw3a == 7.0).all())
    assert torch.equal(loss1, loss2) and float(loss1[2, 0]) != 0.0 and not loss1[[0, 1, 3]].any()


# ---- the counted waits under contention ----------------------------------------------------------------------------------

def test_both_launches_on_four_streams_beside_a_copy_give_the_serial_bits(L):
    """Counts that only hold at the latencies of an idle chip would pass everything above.  Here both launches run at the
    C2 widths on four streams at once, beside a device-to-device copy that keeps HBM busy, eight rounds; every output of
    every stream must equal the bits of one launch alone on an idle chip."""
    rng = np.random.default_rng(5)
    Lp, Hp, Bp, S = 64, 2048, 1024, 512
    G = Bp // 512
    dm = np.concatenate([rand_bf16(rng, (Bp, Lp), 1e-3), rand_bf16(rng, (Bp, Lp), 1e-3)], 1)
    dmd, whd = dev(dm, torch.bfloat16), dev(rand_bf16(rng, (2 * Lp, Hp), 0.05), torch.bfloat16)
    h1d = dev(np.maximum(rand_bf16(rng, (Bp, Hp), 0.5), 0), torch.bfloat16)
    dpd, w3d = dev(rand_bf16(rng, (Bp, Hp), 1e-3), torch.bfloat16), dev(rand_bf16(rng, (Hp, Lp), 0.2), torch.bfloat16)
    mvd = dev((rng.standard_normal((Bp, 2 * Lp)) * 0.4).astype(np.float32))
    ed = dev(rng.standard_normal((Bp, Lp)).astype(np.float32))
    zd = dev(rand_bf16(rng, (Bp, Lp), 1.0), torch.bfloat16)

    def launch(stream):
        o = dict(dp1=torch.full((Bp, Hp), 7.0, device="cuda", dtype=torch.bfloat16), db1=torch.full((G, Hp), 7.0, device="cuda"),
                 dwh=torch.full((G, 2 * Lp, Hp), 7.0, device="cuda"),
                 dmulv=torch.full((Bp, 2 * Lp), 7.0, device="cuda", dtype=torch.bfloat16),
                 dbh=torch.zeros(Bp // 16, 2 * Lp, device="cuda"), dw3=torch.full((2, Hp, Lp), 7.0, device="cuda"))
        stream.wait_stream(torch.cuda.current_stream())   # (the fills above ran on the current stream)
        s = stream.cuda_stream
        L.rv_heads_bwd(dmd.data_ptr(), whd.data_ptr(), Hp, h1d.data_ptr(), Hp, Bp, Hp, Lp, o["dp1"].data_ptr(), Hp,
                       o["db1"].data_ptr(), o["dwh"].data_ptr(), Hp, s)
        L.rv_latent_bwd(dpd.data_ptr(), Hp, w3d.data_ptr(), Lp, Bp, Hp, Lp, Bp, Lp, S, mvd.data_ptr(), ed.data_ptr(), 1e-2, None, None,
                        o["dmulv"].data_ptr(), o["dbh"].data_ptr(), None, 0, None, 0, None, None, 0, zd.data_ptr(), Lp,
                        o["dw3"].data_ptr(), Lp, 2, s)
        return o
    streams = [torch.cuda.Stream() for _ in range(4)]
    ref = launch(streams[0])
    torch.cuda.synchronize()
    big, hog = torch.empty(2, 64 << 20, device="cuda", dtype=torch.uint8), torch.cuda.Stream()
    for rnd in range(8):
        with torch.cuda.stream(hog):
            hog.wait_stream(torch.cuda.current_stream())
            for _ in range(4):
                big[1].copy_(big[0], non_blocking=True)
        outs = [launch(st) for st in streams]
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            for k, v in o.items():
                a, b = v.view(torch.int16 if v.dtype == torch.bfloat16 else torch.int32), ref[k].view(torch.int16 if v.dtype == torch.bfloat16 else torch.int32)
                assert torch.equal(a, b), "round %d stream %d: %s differs from the serial launch" % (rnd, i, k)
