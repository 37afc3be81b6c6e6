"""Whole-step parity (GPU): rv_plan_step against the CPU oracle and the golden
vectors captured from the reference.

Tolerances (stated, bf16 MFMA inputs with fp32 accumulation):
  * vs the bf16-quantised oracle (same rounding points): loss 2e-5 rel, activations
    to ~1 bf16 ulp of the tensor scale, gradients 2e-3 rel-L2.
  * vs the fp32 reference golden: loss 1e-4 rel at the smoke and benchmark shapes
    (5e-4 at the 16x64 toy shape, where 1k elements do not average the rounding),
    recon/mu/logvar 1e-2 abs, gradients 6e-2 rel-L2 (ReLU-mask flips dominate).
"""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from conftest import GOLDEN  # noqa: E402
from oracle import vae_oracle as O  # noqa: E402
from oracle.inputs import PARAM_NAMES, make_eps, make_frames, make_params  # noqa: E402

KL, LR = 1e-4, 1e-4


def _engine(S, H, L, B, **kw):
    from rawaudiovae_kelsey_amd.engine import TrainEngine
    e = TrainEngine(S, H, L, B, kl_beta=KL, lr=LR, **kw)
    e.load_params(make_params(S, H, L, 0))
    return e


def _rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / (np.linalg.norm(b) + 1e-300))


@pytest.mark.parametrize("shape", [(64, 96, 8, 16), (512, 2048, 8, 32), (100, 200, 5, 37), (256, 384, 100, 130)])
def test_fwd_bwd_vs_quantised_oracle(shape):
    from rawaudiovae_kelsey_amd import engine as E
    S, H, L, B = shape
    e = _engine(S, H, L, B)
    x, eps = make_frames(B, S, 1234), make_eps(B, L, 4321)
    xd, ed = torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda()
    recon = torch.zeros(B, S, device="cuda")
    e.step(xd, ed, recon, phases=E.PHASE_FWD | E.PHASE_BWD_A | E.PHASE_BWD_B | E.PHASE_FINALIZE_A | E.PHASE_FINALIZE_B)
    torch.cuda.synchronize()
    p = O.cast_params(make_params(S, H, L, 0), np.float32)
    c = O.forward(p, x, eps, quant="bf16")
    loss, mse, kld = O.loss_function(c["recon"].astype(np.float64), x.astype(np.float64),
                                     c["mu"].astype(np.float64), c["logvar"].astype(np.float64), KL)
    g = O.backward(p, c, KL, quant="bf16")
    got = e.last_loss()
    assert abs(got[0] - loss) <= 2e-5 * abs(loss), (got, loss)
    assert abs(got[1] - mse) <= 2e-5 * abs(mse) and abs(got[2] - kld) <= 1e-4 * abs(kld)
    mu, lv = e.outputs()
    np.testing.assert_allclose(mu.cpu().numpy(), c["mu"], atol=2e-4 * max(1, np.abs(c["mu"]).max()))
    np.testing.assert_allclose(lv.cpu().numpy(), c["logvar"], atol=2e-4 * max(1, np.abs(c["logvar"]).max()))
    np.testing.assert_allclose(recon.cpu().numpy(), c["recon"], atol=5e-4)
    gv = e.grad_views()
    for k in PARAM_NAMES:
        assert _rel_l2(gv[k].cpu().numpy(), g[k]) < 5e-3, k
    # padding of every internal operand stays zero / finite
    Bp, Sp, Hp, Lp = e.padded()
    z = e.buffer("z", torch.bfloat16, (Bp, Lp)).float().cpu().numpy()
    assert np.all(z[B:] == 0) and np.all(z[:, L:] == 0)
    dP4 = e.buffer("dP4", torch.bfloat16, (Bp, Sp)).float().cpu().numpy()
    assert np.all(dP4[B:] == 0) and np.all(dP4[:, S:] == 0)


def test_small_vs_reference_golden():
    from rawaudiovae_kelsey_amd import engine as E
    g = np.load(os.path.join(GOLDEN, "small_f32.npz"))
    S, H, L, B = (int(v) for v in g["shape"])
    e = _engine(S, H, L, B)
    x, eps = make_frames(B, S, 1234), make_eps(B, L, 4321)
    recon = torch.zeros(B, S, device="cuda")
    e.step(torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda(), recon,
           phases=E.PHASE_FWD | E.PHASE_BWD_A | E.PHASE_BWD_B | E.PHASE_FINALIZE_A | E.PHASE_FINALIZE_B)
    got = e.last_loss()[0]
    assert abs(got - float(g["loss"])) <= 5e-4 * float(g["loss"])
    mu, lv = e.outputs()
    np.testing.assert_allclose(recon.cpu().numpy(), g["recon"], atol=1e-2)
    np.testing.assert_allclose(mu.cpu().numpy(), g["mu"], atol=1e-2)
    np.testing.assert_allclose(lv.cpu().numpy(), g["logvar"], atol=1e-2)
    gv = e.grad_views()
    for k in PARAM_NAMES:
        assert _rel_l2(gv[k].cpu().numpy(), g["grad/" + k].astype(np.float64)) < 6e-2, k


@pytest.mark.parametrize("case", ["smoke_f32", "c2_f32", "refini_f32"])
def test_trajectory_vs_reference_golden(case):
    """20 full steps (fwd+bwd+Adam): loss trajectory against the reference's."""
    with open(os.path.join(GOLDEN, "summary.json")) as f:
        cs = json.load(f)["cases"][case]
    S, H, L, B = cs["shape"]
    e = _engine(S, H, L, B)
    for i in range(20):
        x = torch.from_numpy(make_frames(B, S, 1234 + i)).cuda()
        eps = torch.from_numpy(make_eps(B, L, 4321 + i)).cuda()
        e.step(x, eps)
    got = np.array(e.losses(20))
    ref = np.array(cs["traj"])
    rel = np.abs(got - ref) / ref
    assert rel[0] <= 1e-4, rel
    assert rel.max() <= 1e-3, rel
    assert int(e.step_counter.item()) == 20
    # sampled outputs of the last forward are not in the fixture; check parameters moved like Adam moves them
    assert torch.isfinite(e.param).all()


def test_adam_three_steps_vs_quantised_oracle():
    S, H, L, B = 64, 96, 8, 16
    e = _engine(S, H, L, B)
    p = O.cast_params(make_params(S, H, L, 0), np.float32)
    st = O.adam_init(p)
    for i in range(3):
        x, eps = make_frames(B, S, 1234 + i), make_eps(B, L, 4321 + i)
        e.step(torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda())
        O.train_step(p, st, x, eps, KL, LR, quant="bf16")
    pv = e.param_views()
    for k in PARAM_NAMES:
        # each Adam step moves a weight by ~lr; sign disagreements on near-zero grads bound the error by 2*lr*steps
        assert np.abs(pv[k].cpu().numpy() - p[k]).max() <= 2.5 * LR * 3, k
        assert np.abs(pv[k].cpu().numpy() - p[k]).mean() <= 0.05 * LR * 3, k


def test_on_device_rng_path_and_determinism():
    S, H, L, B = 256, 256, 16, 64
    a, b = _engine(S, H, L, B, seed=7), _engine(S, H, L, B, seed=7)
    x = torch.from_numpy(make_frames(B, S, 1)).cuda()
    for _ in range(3):
        a.step(x)
        b.step(x)
    torch.cuda.synchronize()
    assert torch.equal(a.param, b.param) and a.losses(3) == b.losses(3)
    Bp, Sp, Hp, Lp = a.padded()
    eps = a.buffer("eps", torch.float32, (Bp * Lp,))[:B * L].cpu().numpy()
    assert abs(eps.mean()) < 0.1 and abs(eps.std() - 1) < 0.1
    c = _engine(S, H, L, B, seed=8)
    c.step(x)
    assert c.last_loss()[0] != a.losses(3)[0]


def test_graph_replay_matches_eager():
    from rawaudiovae_kelsey_amd.engine import Graph
    S, H, L, B = 256, 256, 16, 128
    a, b = _engine(S, H, L, B, seed=3), _engine(S, H, L, B, seed=3)
    x = torch.from_numpy(make_frames(B, S, 1)).cuda()
    for _ in range(4):
        a.step(x)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with Graph(st) as g:
            b.step(x, stream=st)
        b.host_steps = 0
        for _ in range(4):
            g.launch()
            b.host_steps += 1
    torch.cuda.synchronize()
    assert torch.equal(a.param, b.param)
    assert a.losses(4) == b.losses(4)


def test_ddp_phased_step_equals_local_step_single_rank():
    """FWD|BWD_A|FINALIZE_A -> (all-reduce) -> BWD_B|FINALIZE_B -> (all-reduce) -> Adam-from-flat
    is the same arithmetic as the fused local step when world == 1."""
    from rawaudiovae_kelsey_amd import ddp
    S, H, L, B = 256, 384, 16, 256
    a, b = _engine(S, H, L, B, seed=9), _engine(S, H, L, B, seed=9)
    sync = ddp.GradSync(b.grad, ddp.engine_buckets(b))
    xs = [torch.from_numpy(make_frames(B, S, 70 + i)).cuda() for i in range(3)]
    for i in range(4):
        a.step(xs[i % 3])
        ddp.ddp_step(b, sync, xs[i % 3])
    torch.cuda.synchronize()
    assert torch.equal(a.param, b.param) and a.losses(4) == b.losses(4)


@pytest.mark.parametrize("shape", [(8, 16, 1, 1), (1000, 130, 256, 3), (64, 64, 129, 300), (1024, 2048, 64, 2137)])
def test_edge_shapes_single_frame_wide_latent_ragged_batch(shape):
    """B=1, L=1, L=256 (widest supported latent), S not a multiple of 8, and the ragged last batch
    of the reference's 30 s example (2137 frames) -- each a full step against the oracle."""
    from rawaudiovae_kelsey_amd import engine as E
    S, H, L, B = shape
    e = _engine(S, H, L, B)
    x, eps = make_frames(B, S, 11), make_eps(B, L, 12)
    recon = torch.zeros(B, S, device="cuda")
    e.step(torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda(), recon,
           phases=E.PHASE_FWD | E.PHASE_BWD_A | E.PHASE_BWD_B | E.PHASE_FINALIZE_A | E.PHASE_FINALIZE_B)
    p = O.cast_params(make_params(S, H, L, 0), np.float32)
    c = O.forward(p, x, eps, quant="bf16")
    loss, _, _ = O.loss_function(c["recon"].astype(np.float64), x.astype(np.float64), c["mu"].astype(np.float64),
                                 c["logvar"].astype(np.float64), KL)
    g = O.backward(p, c, KL, quant="bf16")
    assert abs(e.last_loss()[0] - loss) <= 5e-5 * abs(loss)
    # a bf16-ulp flip of one hidden unit (different fp32 summation order) moves a few outputs by ~2e-3
    np.testing.assert_allclose(recon.cpu().numpy(), c["recon"], atol=4e-3)
    assert (np.abs(recon.cpu().numpy() - c["recon"]) > 1e-3).mean() < 1e-3
    gv = e.grad_views()
    for k in PARAM_NAMES:
        assert _rel_l2(gv[k].cpu().numpy(), g[k]) < 1e-2, k


def test_unsupported_latent_is_rejected_loudly():
    from rawaudiovae_kelsey_amd._lib import RvError
    from rawaudiovae_kelsey_amd.engine import TrainEngine
    with pytest.raises(RvError, match="latent_dim"):
        TrainEngine(64, 64, 300, 8)
    e = _engine(64, 64, 8, 8)
    with pytest.raises(RvError):
        e.step(torch.zeros(7, 64, device="cuda"))          # wrong batch size
    with pytest.raises(RvError):
        e.step(torch.zeros(8, 64, device="cuda", dtype=torch.float64))


def test_ddp_runner_graph_segments_equal_eager():
    from rawaudiovae_kelsey_amd import ddp
    S, H, L, B = 256, 384, 16, 256
    a, b = _engine(S, H, L, B, seed=4), _engine(S, H, L, B, seed=4)
    st = torch.cuda.Stream()
    xs = [torch.from_numpy(make_frames(B, S, 90 + i)).cuda() for i in range(2)]
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        a.step(xs[0], stream=st)   # warm-up outside capture (kernel attributes)
        b.step(xs[0], stream=st)
        ra = ddp.DdpRunner(a, ddp.GradSync(a.grad, ddp.engine_buckets(a)), st, use_graphs=False)
        rb = ddp.DdpRunner(b, ddp.GradSync(b.grad, ddp.engine_buckets(b)), st, use_graphs=True)
        for i in range(5):
            ra.step(xs[i % 2])
            rb.step(xs[i % 2])
    torch.cuda.synchronize()
    assert torch.equal(a.param, b.param) and a.losses(5) == b.losses(5)


def test_long_trajectory_tracks_fp32_cpu_training():
    """400 Adam steps at lr 1e-3 on cycling batches: the bf16-MFMA engine must track stock fp32 PyTorch
    training (oracle/torch_port.py, the reference's arithmetic) on the same frames and eps -- no slow drift
    from stale bf16 shadows, bias-correction at large t, or the device step counter.  Tolerances: the first
    100 losses within 2e-3 relative; later the two trajectories decorrelate (bf16 rounding perturbs the
    path of a loss that has fallen by >2x; measured up to 3 % on single batches), so every step within 6 %
    and the mean of the last 50 within 2 %."""
    from oracle.torch_port import PortVAE, port_loss
    S, H, L, B, steps, lr = 128, 256, 16, 128, 400, 1e-3
    p = make_params(S, H, L, 0)
    xs = [make_frames(B, S, 100 + i) * (0.3 + 0.1 * i) for i in range(4)]     # batches of different scale
    es = [make_eps(B, L, 200 + i) for i in range(4)]
    from rawaudiovae_kelsey_amd.engine import TrainEngine
    e = TrainEngine(S, H, L, B, kl_beta=KL, lr=lr, ring=512)
    e.load_params(p)
    xd = [torch.from_numpy(x.astype(np.float32)).cuda() for x in xs]
    ed = [torch.from_numpy(v).cuda() for v in es]
    for t in range(steps):
        e.step(xd[t % 4], ed[t % 4])
    got = np.array(e.losses(steps))
    m = PortVAE(S, H, L)
    m.load_numpy(p)
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    ref = []
    torch.set_num_threads(4)
    for t in range(steps):
        x, eps = torch.from_numpy(xs[t % 4].astype(np.float32)), torch.from_numpy(es[t % 4])
        opt.zero_grad()
        recon, mu, lv = m(x, eps)
        loss = port_loss(recon, x, mu, lv, KL, S)
        loss.backward()
        opt.step()
        ref.append(loss.item())
    ref = np.array(ref)
    assert ref[-1] < 0.5 * ref[0]                       # it actually trains
    rel = np.abs(got - ref) / ref
    assert rel[:100].max() < 2e-3, (rel[:100].max(), int(rel[:100].argmax()))
    assert rel.max() < 6e-2, (rel.max(), int(rel.argmax()))
    assert abs(got[-50:].mean() - ref[-50:].mean()) / ref[-50:].mean() < 2e-2


@pytest.mark.parametrize("shape", [(1024, 2048, 64, 4096), (256, 512, 16, 384)])
def test_full_step_equals_its_phases(shape):
    """The default schedule of the full step (the fc1 weight-gradient launch also carries the Adam update of fc3 / fc4
    on the CUs its GEMM leaves idle, rv_linear_wgrad_adam) gives bit for bit what the same step gives when it is
    issued phase by phase (forward, backward, then Adam as launches of its own from the same slabs): same kernels'
    arithmetic, different launch grouping."""
    from rawaudiovae_kelsey_amd import engine as E
    S, H, L, B = shape
    x = [torch.from_numpy(make_frames(B, S, 7 + i)).cuda() for i in range(3)]
    out = []
    for phased in (False, True):
        e = _engine(S, H, L, B, seed=11)
        for i in range(3):
            if phased:
                e.step(x[i], phases=E.PHASE_FWD | E.PHASE_BWD_A | E.PHASE_BWD_B)
                e.step(x[i], phases=E.PHASE_ADAM)
            else:
                e.step(x[i])
        torch.cuda.synchronize()
        out.append((e.param.clone(), e.exp_avg.clone(), e.exp_avg_sq.clone(), e.losses(3)))
    assert out[0][3] == out[1][3]
    for a, b in zip(out[0][:3], out[1][:3]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [(1024, 2048, 64, 4096), (256, 512, 16, 384)])
def test_backward_in_one_go_equals_the_finer_phases(shape):
    """The latent-sized backward as the full step issues it (rv_latent_bwd with fc3's weight gradient on extra
    workgroups of its launch, then the heads' backward) against the same backward issued phase by phase (BWD_FC4,
    BWD_CHAIN, BWD_REST: fc3's weight gradient then is a launch of its own): every gradient bit for bit."""
    from rawaudiovae_kelsey_amd import engine as E
    S, H, L, B = shape
    x, eps = torch.from_numpy(make_frames(B, S, 31)).cuda(), torch.from_numpy(make_eps(B, L, 32)).cuda()
    fin = E.PHASE_FINALIZE_A | E.PHASE_FINALIZE_B
    out = []
    for fine in (False, True):
        e = _engine(S, H, L, B)
        if fine:
            for ph in (E.PHASE_FWD, E.PHASE_BWD_FC4, E.PHASE_BWD_CHAIN, E.PHASE_BWD_REST, fin):
                e.step(x, eps, phases=ph)
        else:
            e.step(x, eps, phases=E.PHASE_FWD | E.PHASE_BWD_A | E.PHASE_BWD_B | fin)
        torch.cuda.synchronize()
        out.append(({k: v.clone() for k, v in e.grad_views().items()}, e.last_loss()))
    assert out[0][1] == out[1][1]
    for k in PARAM_NAMES:
        assert torch.equal(out[0][0][k], out[1][0][k]), k
        assert float(out[0][0][k].abs().max()) > 0, k


def test_latent_forward_one_launch_vs_three_in_the_step():
    """The step with heads + reparam + fc3 as one launch and dz + reparam backward as one launch
    (`set_latent_fused(True)`, the default where it applies) against the step with the three + three launches: same eps, losses equal to fp32 summation order, parameters after 5 steps
    agree like two summation orders do."""
    from oracle.inputs import make_frames, make_params
    from rawaudiovae_kelsey_amd.engine import TrainEngine
    S, H, L, B = 1024, 2048, 64, 4096
    engs = []
    for fused in (True, False):
        e = TrainEngine(S, H, L, B, kl_beta=1e-2, lr=1e-3, seed=5)
        e.load_params(make_params(S, H, L, 0))
        e.set_latent_fused(fused)
        for i in range(5):
            e.step(torch.from_numpy(make_frames(B, S, 10 + i)).cuda())
        engs.append(e)
    la, lb = engs[0].losses(5), engs[1].losses(5)
    np.testing.assert_allclose(la, lb, rtol=2e-5)
    d = (engs[0].param - engs[1].param).abs()
    assert float(d.mean()) < 2e-5 and float(d.max()) <= 5 * 2 * 1e-3 + 1e-6


@pytest.mark.parametrize("shape", [(1024, 2048, 64, 4096), (256, 384, 100, 130), (1024, 2048, 256, 4096)])
def test_fp16_split_k_slabs_vs_fp32_slabs(shape):
    """slab_dtype="fp16" (the default): the split-K partials of dW1 / dW4 -- and, where the streaming heads' backward
    runs (C2), the eight row-group partials of the two heads' weight gradients -- are stored as block-floating-point fp16
    (one power-of-two scale per 32 x 32 granule and slab) and summed in fp32.  Forward and every other gradient are
    untouched (bit-equal to slab_dtype="fp32"); those weight gradients move by the rounding of their fp16 partials
    (stated bound 1e-3 rel-L2, 3e-4 expected) and still meet the oracle bound of the bf16 path."""
    from rawaudiovae_kelsey_amd import engine as E
    S, H, L, B = shape
    x, eps = make_frames(B, S, 1234), make_eps(B, L, 4321)
    xd, ed = torch.from_numpy(x).cuda(), torch.from_numpy(eps).cuda()
    ph = E.PHASE_FWD | E.PHASE_BWD_A | E.PHASE_BWD_B | E.PHASE_FINALIZE_A | E.PHASE_FINALIZE_B
    out = {}
    for dt in ("fp32", "fp16"):
        e = _engine(S, H, L, B, slab_dtype=dt)
        e.step(xd, ed, phases=ph)
        torch.cuda.synchronize()
        out[dt] = ({k: v.clone() for k, v in e.grad_views().items()}, e.last_loss())
    assert out["fp16"][1] == out["fp32"][1]
    # the streaming heads' backward (batch a multiple of 512, latent width 64), or -- the reference's own latent width -- the
    # heads' backward as the paired 256 x 256 launch: the heads' slabs are fp16 as well
    heads16 = shape in ((1024, 2048, 64, 4096), (1024, 2048, 256, 4096))
    for k in PARAM_NAMES:
        a, b = out["fp16"][0][k], out["fp32"][0][k]
        if k in ("fc1.weight", "fc4.weight") or (heads16 and k in ("fc21.weight", "fc22.weight")):
            rel = float((a - b).norm() / b.norm())
            assert 0 < rel < 1e-3, (k, rel)
        else:
            assert torch.equal(a, b), k
    p = O.cast_params(make_params(S, H, L, 0), np.float32)
    c = O.forward(p, x, eps, quant="bf16")
    g = O.backward(p, c, KL, quant="bf16")
    for k in ("fc1.weight", "fc4.weight", "fc21.weight", "fc22.weight"):
        assert _rel_l2(out["fp16"][0][k].cpu().numpy(), g[k]) < 5e-3, k
    # full steps (Adam reading the fp16 slabs, the default schedule's optimizer blocks included) stay on the
    # reference trajectory
    e = _engine(S, H, L, B, slab_dtype="fp16")
    r = _engine(S, H, L, B, slab_dtype="fp32")
    for i in range(6):
        xi = torch.from_numpy(make_frames(B, S, 50 + i)).cuda()
        ei = torch.from_numpy(make_eps(B, L, 60 + i)).cuda()
        e.step(xi, ei)
        r.step(xi, ei)
    la, lb = np.array(e.losses(6)), np.array(r.losses(6))
    assert np.abs(la - lb).max() <= 1e-4 * lb.max(), (la, lb)


def test_full_local_step_with_external_grads_is_refused_before_any_launch():
    """A full local step (backward + ADAM in one call) cannot take gradients from outside.  The call is refused before its
    forward goes out: the device step counter and recon_out are as they were."""
    from rawaudiovae_kelsey_amd._lib import RvError, lib, ptr
    S, H, L, B = 64, 96, 8, 16
    e = _engine(S, H, L, B)
    x = torch.from_numpy(make_frames(B, S, 1234)).cuda()
    eps = torch.from_numpy(make_eps(B, L, 4321)).cuda()
    e.step(x, eps)
    recon = torch.full((B, S), 7.0, device="cuda")
    d_recon = torch.ones(B, S, device="cuda")
    torch.cuda.synchronize()
    steps = e.step_counter.clone()
    lib().rv_plan_set_external_grads(e._plan, ptr(d_recon), ptr(recon), None, None, None)
    try:
        with pytest.raises(RvError, match="external gradients"):
            e.step(x, eps, recon)
    finally:
        lib().rv_plan_set_external_grads(e._plan, None, None, None, None, None)
    torch.cuda.synchronize()
    assert torch.equal(e.step_counter, steps)
    assert (recon == 7.0).all()
