"""Every path of the fused Adam and of the shadow refresh (csrc/adam.h) against the float64 oracle of the descriptor
contract (tests/optimizer_oracle.py), on two bags of small tensors that force each path by construction -- the table
is in DESIGN.md, "optimizer test matrix", and beside the specs in optimizer_oracle.py.

What is compared, per entry point (u = 2^-24; the bounds and the operation counts behind them are in
optimizer_oracle.py's docstring, and tests/test_optimizer_oracle_cpu.py shows that an fp32 model of adam_update with its
approximate operations an ulp off either way stays inside them):
  * the summed gradient (rv_grad_finalize, rv_adam_multi's grad_out): bit for bit -- the slabs hold exactly representable
    values whose sums are exact in any order; the bf16 payload is bf16_round of that;
  * exp_avg, exp_avg_sq and the parameters: |m - m_ref| <= 4u (0.9|m0| + 0.1|g|), |v - v_ref| <= 5u v_ref,
    |w - w_ref| <= 2u|w_ref| + 32u|dw_ref| + (step/denom)_ref tol_m -- nothing but the last subtraction's rounding is
    relative to |w|, so the UPDATE is what is held, at step counters 1, 2, 1000 and 10^6;
  * the shadows: bit for bit what optimizer_oracle.shadow_values derives from the kernel's own new parameters;
  * everything a call must not write -- arena elements between the tensors, gap columns and padding rows of the shadows,
    every guard band -- still holds its sentinel.

Worst observed |error| / bound on an MI355X (m, v, w), printed by every test (run with -s):
  rv_adam_multi, random state         t = 1: 0.53 0.64 0.49   t = 2: 0.53 0.64 0.49   t = 1000: 0.53 0.64 0.50   t = 10^6: 0.53 0.64 0.48
  rv_adam_multi, zero state           t = 1: 0.30 0.52 0.47
  rv_adam_multi, consecutive steps    t = 1: 0.30 0.53 0.46   t = 2: 0.45 0.53 0.46   t = 3: 0.42 0.45 0.46
  rv_adam_multi, bf16 flat gradient   t = 5: 0.55 0.43 0.50   (8-byte aligned and one element further alike)
  rv_linear_wgrad_adam                t = 4: 0.53 0.50 0.49 on the LDS-DMA ring, 0.53 0.70 0.50 on the plain-load walk
                                      (K = 128 and 192, 1 / 3 / 24 optimizer blocks alike)
The fp32 numpy model of adam_update (optimizer_oracle.adam_model_f32, unperturbed) gives the same figures on the same
inputs.  The whole file takes under 3 s on the GPU.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import optimizer_oracle as OO  # noqa: E402
from guarded import guarded, guarded_flat  # noqa: E402
from test_kernels_gpu import dev, rand_bf16, sp  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def L():
    from rawaudiovae_kelsey_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.lib()


@pytest.fixture(scope="module")
def bags():
    """The two bags on the device: slabs and tables are uploaded once and never written."""
    return {name: OO.DeviceBag(OO.bag(name)) for name in ("f32", "f16")}


@pytest.fixture(scope="module")
def zero_bags():
    return {name: OO.DeviceBag(OO.bag(name, 0.25)) for name in ("f32", "f16")}


def counter(t):
    return torch.full((1,), t, dtype=torch.int64, device="cuda")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def arenas(D, state):
    return [D.arena(a) for a in state]


def assert_gradient(D, G, g64, name, as_bf16=False):
    """A flat gradient arena is the oracle's sum (cast to fp32, or bf16_round of that) bit for bit inside the tensors and
    untouched outside."""
    mask = D.bag.mask
    got = D.read(G)[mask]
    want = g64.astype(np.float32)[mask]
    assert np.array_equal(want.astype(np.float64), g64[mask])
    if as_bf16:
        assert np.array_equal(bits(got), bits(OO.O.bf16_round(want))), name
    else:
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, "%s: %d gradient elements differ, first %d: %r != %r" % (name, bad.size, bad[0], got[bad[0]], want[bad[0]])
    D.assert_arena_outside_untouched(G, name)


def assert_update(D, g64, state, t, M, V, W, name):
    """The arenas M, V, W after one step from `state` with gradient g64 (flat float64, grad_scale applied) are inside the
    bounds; the shadows are derived from W; nothing else was written.  Returns (and prints) the worst error / bound."""
    mask = D.bag.mask
    ref = OO.adam_reference(g64[mask], *(a[mask] for a in state), t)
    m, v, w = D.read(M), D.read(V), D.read(W)
    r = OO.worst_ratios(ref, m[mask], v[mask], w[mask])
    print("ratio %-44s t=%-8d m %.3f  v %.3f  w %.3f" % (name, t, r["m"], r["v"], r["w"]))
    for k, got in (("m", m), ("v", v), ("w", w)):
        err = np.abs(got[mask].astype(np.float64) - ref[k])
        bad = np.flatnonzero(err > ref["tol_" + k])
        assert bad.size == 0, "%s, t = %d: %s misses its bound at %d elements (worst %.2f of it); first: arena index %d, got %r, reference %r" % (
            name, t, k, bad.size, r[k], np.flatnonzero(mask)[bad[0]], got[mask][bad[0]], ref[k][bad[0]])
    for G, what in ((M, "exp_avg"), (V, "exp_avg_sq"), (W, "param")):
        D.assert_arena_outside_untouched(G, "%s: %s" % (name, what))
    D.assert_shadows(w, name)
    return r


# ------------------------------------------------------------------------------------------------ rv_grad_finalize
@pytest.mark.parametrize("name", ["f32", "f16"])
@pytest.mark.parametrize("out_bf16", [0, 1], ids=["fp32", "bf16"])
def test_grad_finalize(L, bags, name, out_bf16):
    D = bags[name]
    D.reset_outputs()
    G = D.arena(dtype=BF if out_bf16 else F32)
    L.rv_grad_finalize(D.descs, D.n_desc, G.ptr, out_bf16, sp())
    torch.cuda.synchronize()
    assert_gradient(D, G, D.bag.grad_flat(), "rv_grad_finalize(%s)" % name, as_bf16=bool(out_bf16))
    for sh in D.shadows:     # a finalize refreshes no shadow
        for kind, S in sh.items():
            S.assert_untouched("rv_grad_finalize: %s shadow" % kind)
            assert int((S.payload() != S.fill).sum()) == 0


# ------------------------------------------------------------------------------------------------ rv_adam_multi
@pytest.mark.parametrize("name", ["f32", "f16"])
@pytest.mark.parametrize("with_grad_out", [False, True], ids=["", "grad_out"])
@pytest.mark.parametrize("t", OO.STEPS)
def test_adam_multi(L, bags, name, with_grad_out, t):
    D = bags[name]
    D.reset_outputs()
    state = OO.random_state(D.bag.n, 11)
    M, V, W = arenas(D, state)
    GO = D.arena() if with_grad_out else None
    ctr = counter(t)
    L.rv_adam_multi(D.descs, D.n_desc, W.ptr, M.ptr, V.ptr, GO.ptr if GO else None, None, OO.LR, OO.GRAD_SCALE,
                    ctr.data_ptr(), sp())
    torch.cuda.synchronize()
    g = D.bag.grad_flat(OO.GRAD_SCALE)
    if GO:
        assert_gradient(D, GO, g, "rv_adam_multi(%s) grad_out" % name)
    assert_update(D, g, state, t, M, V, W, "rv_adam_multi(%s)" % name)


@pytest.mark.parametrize("name", ["f32", "f16"])
def test_adam_multi_zero_gradient_from_zero_state(L, zero_bags, name):
    """m = v = 0 and a gradient that is exactly 0: the element keeps its parameter bit for bit (0 * rcp(eps) = 0) and
    its moments stay 0; the others move by about lr."""
    D = zero_bags[name]
    D.reset_outputs()
    z = np.zeros(D.bag.n, dtype=np.float32)
    state = (z, z, OO.random_state(D.bag.n, 11)[2])
    M, V, W = arenas(D, state)
    ctr = counter(1)
    L.rv_adam_multi(D.descs, D.n_desc, W.ptr, M.ptr, V.ptr, None, None, OO.LR, OO.GRAD_SCALE, ctr.data_ptr(), sp())
    torch.cuda.synchronize()
    g = D.bag.grad_flat(OO.GRAD_SCALE)
    assert_update(D, g, state, 1, M, V, W, "rv_adam_multi(%s) zero state" % name)
    still = D.bag.mask & (g == 0)
    assert still.sum() > 0.1 * D.bag.mask.sum()
    assert np.array_equal(bits(D.read(W)[still]), bits(state[2][still]))
    assert not np.any(bits(D.read(M)[still])) and not np.any(bits(D.read(V)[still]))
    go = D.bag.mask & (g != 0)
    step = np.abs(D.read(W)[go].astype(np.float64) - state[2][go])
    assert np.all(step > 0.5 * OO.LR) and np.all(step < 1.5 * OO.LR)


@pytest.mark.parametrize("name", ["f32", "f16"])
def test_adam_multi_three_consecutive_steps(L, bags, name):
    """The counter at 1, 2, 3 on one state: before each step the oracle restarts from the kernel's own fp32 state, so the
    bounds stay those of a single step."""
    D = bags[name]
    z = np.zeros(D.bag.n, dtype=np.float32)
    M, V, W = arenas(D, (z, z, OO.random_state(D.bag.n, 13)[2]))
    g = D.bag.grad_flat(OO.GRAD_SCALE)
    ctr = counter(0)
    for t in (1, 2, 3):
        D.reset_outputs()
        state = tuple(D.read(A) for A in (M, V, W))
        ctr.fill_(t)
        L.rv_adam_multi(D.descs, D.n_desc, W.ptr, M.ptr, V.ptr, None, None, OO.LR, OO.GRAD_SCALE, ctr.data_ptr(), sp())
        torch.cuda.synchronize()
        assert_update(D, g, state, t, M, V, W, "rv_adam_multi(%s) consecutive" % name)


@pytest.mark.parametrize("name", ["f32", "f16"])
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset_by_one"])
def test_adam_multi_from_bf16_gradient(L, bags, name, shift):
    """grad_bf16: the gradient comes from a flat bf16 arena, the slabs are not read.  8-byte aligned the 4-wide tensors take
    the bf16x4 load, one element further the scalar one; ragged tensors and wave-summed rows are in both bags.  The "f16"
    bag's descriptors include fp16-slab tensors laid out 8 elements per thread when the slabs are read (adam_wide): with
    a flat gradient every element must still be updated -- or the call must fail before it launches anything."""
    D = bags[name]
    D.reset_outputs()
    n, mask = D.bag.n, D.bag.mask
    gb = OO.bf16_gradient(n, 12)
    assert np.array_equal(OO.O.bf16_round(gb.astype(np.float32)).astype(np.float64), gb)
    src = np.full(n + 1, np.nan, dtype=np.float32)
    src[shift:shift + n][mask] = gb[mask]             # NaN between the tensors: reading it poisons the state
    GB = guarded_flat(n + 1, BF, src)
    ptr = GB.ptr + 2 * shift
    assert ptr % 8 == (0 if shift == 0 else 2)
    state = OO.random_state(n, 11)
    M, V, W = arenas(D, state)
    from rawaudiovae_kelsey_amd._lib import RvError
    ctr = counter(5)
    try:
        L.rv_adam_multi(D.descs, D.n_desc, W.ptr, M.ptr, V.ptr, None, ptr, OO.LR, OO.GRAD_SCALE, ctr.data_ptr(), sp())
    except RvError:
        torch.cuda.synchronize()
        for A, a in zip((M, V, W), state):   # rejected: nothing may have run
            assert np.array_equal(bits(D.read(A)[mask]), bits(a[mask]))
            D.assert_arena_outside_untouched(A, "rejected rv_adam_multi")
        return
    torch.cuda.synchronize()
    assert_update(D, gb * OO.GRAD_SCALE, state, 5, M, V, W, "rv_adam_multi(%s) grad_bf16 %s" % (name, "aligned" if shift == 0 else "offset"))


# ------------------------------------------------------------------------------------------------ rv_linear_wgrad_adam
@pytest.fixture(scope="module")
def gemm_inputs():
    out = {}
    for K in (128, 192):
        rng = np.random.default_rng(13 + K)
        dy, x = rand_bf16(rng, (K, 256)), rand_bf16(rng, (K, 256))
        out[K] = (dev(dy, BF), dev(x, BF), dy.astype(np.float64).T @ x.astype(np.float64))
    return out


@pytest.mark.parametrize("name", ["f32", "f16"], ids=["lds_dma_ring", "plain_loads"])
@pytest.mark.parametrize("K", [128, 192], ids=["8stage", "2stage"])
@pytest.mark.parametrize("n_blocks", [1, 3, 24])
def test_wgrad_adam_riders(L, bags, gemm_inputs, name, K, n_blocks):
    """The optimizer blocks of rv_linear_wgrad_adam against the oracle: a bag of fp32 slabs rides on the per-wave LDS-DMA
    rings (adam_stream), a bag with fp16 slabs on the plain-load walk (adam_group<2>); one optimizer block makes every
    wave's ring wrap many times, with 24 many waves start past the end of the table.  The GEMM beside them (an even count
    of K tiles takes the 8-stage kernel, an odd one the 2-stage) against the float64 product."""
    D = bags[name]
    D.reset_outputs()
    Mg = Ng = 256
    dy, x, ref = gemm_inputs[K]
    DW = guarded(Mg, Ng, Ng, F32)
    state = OO.random_state(D.bag.n, 17)
    M, V, W = arenas(D, state)
    t = 4
    ctr = counter(t)
    L.rv_linear_wgrad_adam(dy.data_ptr(), Mg, x.data_ptr(), Ng, Mg, Ng, K, 1, DW.ptr, Ng, 0, None, D.descs, D.n_desc,
                           W.ptr, M.ptr, V.ptr, OO.LR, OO.GRAD_SCALE, ctr.data_ptr(), n_blocks, sp())
    torch.cuda.synchronize()
    assert_update(D, D.bag.grad_flat(OO.GRAD_SCALE), state, t, M, V, W,
                  "rv_linear_wgrad_adam(%s, K=%d, %d blocks)" % (name, K, n_blocks))
    np.testing.assert_allclose(DW.payload().cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    DW.assert_untouched("dW")


# ------------------------------------------------------------------------------------------------ rv_params_from_flat
@pytest.mark.parametrize("name", ["f32", "f16"])
@pytest.mark.parametrize("case", ["base4", "base6", "shadows_only", "arena_itself"])
def test_params_from_flat(L, bags, name, case):
    """refresh_block: parameters (unless param is NULL) and every shadow from a flat fp32 source whose element 0 is arena
    element flat_base.  base4 keeps the 4-wide copy for the aligned tensors and sends the tensor at offset % 4 == 1
    down the scalar one; base6 misaligns o - flat_base for every aligned tensor; the "f16" bag has the two-halves layout
    of adam_wide tensors, both bags wave-per-group rows and ragged tensors."""
    D = bags[name]
    D.reset_outputs()
    n, mask = D.bag.n, D.bag.mask
    w = OO.random_state(n, 19)[2]
    label = "rv_params_from_flat(%s, %s)" % (name, case)
    if case == "arena_itself":
        W = D.arena(w)
        before = W.flat.clone()
        L.rv_params_from_flat(D.descs, D.n_desc, W.ptr, 0, None, sp())
        torch.cuda.synchronize()
        assert torch.equal(W.flat.view(torch.int32), before.view(torch.int32))
    else:
        base = {"base4": 4, "base6": 6, "shadows_only": 0}[case]
        src = np.where(mask, w, np.float32(np.nan)).astype(np.float32)[base:]   # NaN between the tensors and in the guards
        SRC = guarded_flat(n - base, F32, src)
        W = D.arena() if case != "shadows_only" else None
        L.rv_params_from_flat(D.descs, D.n_desc, SRC.ptr, base, W.ptr if W else None, sp())
        torch.cuda.synchronize()
        if W:
            assert np.array_equal(bits(D.read(W)[mask]), bits(w[mask])), label
            D.assert_arena_outside_untouched(W, label)
    D.assert_shadows(w, label)
