"""The optimizer oracle (tests/optimizer_oracle.py) on its own, without a GPU: it agrees with torch.optim.Adam in
float64, the gradients of its bags are exact in fp32 in any order, and an fp32 model of csrc/adam.h's adam_update with
its approximate operations moved by an ulp either way stays inside the bounds that tests/test_optimizer_gpu.py holds
the kernels to -- so a kernel that misses a bound does something the model does not."""
import itertools

import numpy as np
import pytest

import optimizer_oracle as OO

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("steps", [1, 3])
def test_oracle_matches_torch_adam_float64(steps):
    rng = np.random.default_rng(5)
    n = 257
    w0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 1, n) for _ in range(steps)]
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.Adam([p], lr=OO.LR, foreach=False)
    m, v, w = np.zeros(n), np.zeros(n), w0.copy()
    for t, g in enumerate(grads, 1):
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        ref = OO.adam_reference(g, m, v, w, t)
        m, v, w = ref["m"], ref["v"], ref["w"]
        st = opt.state[p]
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(w, p.detach().numpy(), rtol=1e-12, atol=0)
        # the update itself, not only the parameter it is subtracted from
        np.testing.assert_allclose(w - w0, p.detach().numpy() - w0, rtol=1e-9, atol=0)


@pytest.mark.parametrize("name,zero_frac", [("f32", 0.0), ("f16", 0.0), ("f32", 0.25), ("f16", 0.25)])
def test_gradients_are_exact_in_any_order(name, zero_frac):
    """The fp32 sum of every tensor's slabs is the same forwards, backwards and in the kernels' (a+b)+(c+d) grouping,
    and equals the float64 sum: the GPU tests compare gradients bit for bit."""
    b = OO.bag(name, zero_frac)
    for t in b.tensors:
        terms = t.terms()
        t32 = terms.astype(np.float32)
        assert np.array_equal(t32.astype(np.float64), terms), t.spec.name     # every term is an fp32 number
        if t.spec.half:
            assert np.array_equal(t.slabs.astype(np.float16).astype(np.float64), t.slabs)
        exact = terms.sum(0)
        fwd, rev, grp = (np.zeros(exact.shape, dtype=np.float32) for _ in range(3))
        for s in range(t.spec.splits):
            fwd = fwd + t32[s]
            rev = rev + t32[t.spec.splits - 1 - s]
        s = 0
        while s + 4 <= t.spec.splits:
            grp = grp + ((t32[s] + t32[s + 1]) + (t32[s + 2] + t32[s + 3]))
            s += 4
        for s in range(s, t.spec.splits):
            grp = grp + t32[s]
        for got in (fwd, rev, grp):
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), exact), t.spec.name
        scaled = (exact * OO.GRAD_SCALE).astype(np.float32)
        assert np.array_equal(scaled.astype(np.float64), exact * OO.GRAD_SCALE)
        if zero_frac:
            assert (exact == 0).mean() > 0.1, t.spec.name


def test_bags_cover_the_paths_they_are_named_for():
    """The layout properties the path table relies on ('optimizer test matrix')."""
    for name in ("f32", "f16"):
        b = OO.bag(name)
        end = 0
        for t in b.tensors:
            assert t.offset >= end + 8 and t.offset % 8 == t.spec.off_rem, t.spec.name
            end = t.offset + t.spec.rows * t.spec.cols
        assert b.n >= end + 8
    by = {t.spec.name: t for name in ("f32", "f16") for t in OO.bag(name).tensors}

    def wide(t):   # csrc/adam.h: adam_wide (the slab pointers are 16-byte aligned by construction)
        s = t.spec
        return (s.half and s.rows > 1 and "f32" not in s.shadows and s.splits <= 8
                and (s.cols | s.grad_ld | s.split_stride | t.offset | s.shadow_ld) % 8 == 0)

    def vec(t):
        s = t.spec
        return (s.cols | s.grad_ld | s.split_stride | t.offset) % 4 == 0

    assert [n for n, t in by.items() if wide(t)] == ["h_wide4", "h_wide8", "h_wide3"]
    for n in ("w4", "w3", "w2", "w1", "s5", "s9", "h_36", "h_s9", "h_off4", "f_w4", "f_w3", "f_w2", "f_w1"):
        assert vec(by[n]) and not wide(by[n]), n
    for n in ("rag3", "rag6", "off1", "ld2", "tiny", "bias3", "h_ld2", "f_rag"):
        assert not vec(by[n]), n
    assert by["off1"].offset % 4 == 1 and by["ld2"].spec.grad_ld % 4 == 2 and by["h_off4"].offset % 8 == 4
    assert by["w4"].spec.rows * by["w4"].spec.cols // 4 > 256          # spans two virtual blocks
    assert by["rag6"].spec.shadow_ld % 4 != 0 and by["w4"].spec.shadow_ld % 4 == 0
    for n in ("coop16", "coop70", "h_coop", "f_coop"):
        assert by[n].spec.rows == 1 and by[n].spec.splits >= 16


def test_e4m3_bits_round_trip():
    codes = np.array([c for c in range(256) if c & 0x7f != 0x7f], dtype=np.uint8)
    vals = torch.from_numpy(codes).view(torch.float8_e4m3fn).float().numpy()
    assert np.array_equal(OO.e4m3_bits(vals), codes)
    w = np.array([0.0, -0.0, 1e-5, -1e-5, 0.3, -27.9, 28.1, 100.0, -3e4], dtype=np.float32)
    want = torch.from_numpy(np.clip(w * 16, -448, 448)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(OO.shadow_values("fp8", w), want)


PERTURB = [(0, 0, 0, 0)] + list(itertools.product((-1, 1), repeat=4))
MODEL_T = (1, 2, 3, 10, 1000, 10 ** 5, 10 ** 7)


def _model_ratios(g, m0, v0, w0, t):
    ref = OO.adam_reference(g, m0, v0, w0, t)
    worst = {"m": 0.0, "v": 0.0, "w": 0.0}
    for ks in PERTURB:
        m, v, w = OO.adam_model_f32(g, m0, v0, w0, t, OO.LR, *ks)
        r = OO.worst_ratios(ref, m, v, w)
        worst = {k: max(worst[k], r[k]) for k in worst}
    return worst


def test_fp32_model_stays_inside_the_bounds_on_hard_inputs():
    """Typical values, zero state, m0 ~ -g/9 (the first moment cancels), |g| ~ 2^-27 and |w| ~ 1000, at small and very
    large step counters."""
    rng = np.random.default_rng(3)
    n = 4096
    f = np.float32
    g = (rng.integers(-1024, 1025, n) * 2.0 ** -12).astype(f)
    m0, v0, w0 = OO.random_state(n, 4)
    tiny = (rng.integers(-1024, 1025, n) * 2.0 ** -37).astype(f)
    cases = {"typical": (g, m0, v0, w0),
             "zero state": (g, np.zeros(n, f), np.zeros(n, f), w0),
             "cancellation": (g, (-g / 9 * (1 + 1e-6 * rng.standard_normal(n))).astype(f), v0, w0),
             "tiny gradient": (tiny, np.zeros(n, f), np.zeros(n, f), w0),
             "large weights": (g, m0, v0, (1000 * w0).astype(f)),
             "zero weights": (g, m0, v0, np.zeros(n, f))}
    for name, (g_, m_, v_, w_) in cases.items():
        for t in MODEL_T:
            r = _model_ratios(g_, m_, v_, w_, t)
            assert max(r.values()) <= 1.0, (name, t, r)


@pytest.mark.parametrize("name", ["f32", "f16"])
def test_fp32_model_stays_inside_the_bounds_on_the_gpu_tests_inputs(name):
    b = OO.bag(name)
    g = b.grad_flat(OO.GRAD_SCALE)
    m0, v0, w0 = OO.random_state(b.n, 11)
    for t in OO.STEPS + (3,):
        r = _model_ratios(g, m0, v0, w0, t)
        assert max(r.values()) <= 1.0, ("slabs", t, r)
    r = _model_ratios(OO.bf16_gradient(b.n, 12) * OO.GRAD_SCALE, m0, v0, w0, 5)
    assert max(r.values()) <= 1.0, ("bf16 payload", r)
    bz = OO.bag(name, 0.25)
    z = np.zeros(bz.n, np.float32)
    r = _model_ratios(bz.grad_flat(OO.GRAD_SCALE), z, z, OO.random_state(bz.n, 11)[2], 1)
    assert max(r.values()) <= 1.0, ("zero state", r)
