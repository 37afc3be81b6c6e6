"""A float64 oracle of the fused optimizer's descriptor contract (include/rawvae_hip.h: rv_param_desc), and the bags of
small tensors that tests/test_optimizer_gpu.py and tests/test_optimizer_oracle_cpu.py share.

A Spec names one tensor as a descriptor sees it: exact shape, the split-K gradient slabs (leading dimension, split
stride, count, fp32 or block-floating-point fp16 with one power-of-two factor per 32 x 32 granule and slab), its place
in the flat arenas and the operand shadows the update refreshes.  make_bag() lays a list of specs out in an arena (a
gap of at least 8 elements between tensors) and draws the slabs; everything in it is numpy, so the CPU tests see
exactly what the GPU tests upload.  DeviceBag (GPU only) cuts every buffer from tests/guarded.py allocations and fills
the rv_param_desc array from the same specs.

Gradients are exactly representable: fp32 slabs hold integers in [-1024, 1024] times 2^-12, fp16 slabs integers in
[-1024, 1024] whose factors are 2^-e, e in [4, 12].  A sum of up to 70 such terms is an integer below 2^24 times
2^-12, so it is exact in fp32 in ANY order (test_optimizer_oracle_cpu.py checks that premise) and the kernels'
gradient is compared bit for bit; grad_scale is a power of two.

The update is O.adam_step's formula (oracle/vae_oracle.py; torch.optim.Adam's single-tensor form) in float64:
    m = 0.9 m0 + 0.1 g;  v = 0.999 v0 + 0.001 g^2;  denom = sqrt(v) / sqrt(1 - 0.999^t) + 1e-8
    w = w0 - lr / (1 - 0.9^t) * m / denom
Bounds on the kernels' fp32 results (u = 2^-24, one half ulp relative):
    |m - m_ref| <= 4u (0.9 |m0| + 0.1 |g|)          constant, product, constant, product, sum: 1u each, 3u in all
    |v - v_ref| <= 5u v_ref                         0.999f and its product; 0.001f and two products; the sum: 4u
    |w - w_ref| <= 2u |w_ref| + 32u |dw_ref| + (step / denom)_ref tol_m
with dw = step m / denom: the fp32 constants are 1u each, every product and sum 1u, v_sqrt_f32 and v_rcp_f32 2u each
(1 ulp), expm1f and the division behind step_size and inv_bc2s about 4u each -- under 20u on dw, 32u leaves room; the
error of m enters through step / denom, and only the final subtraction's rounding is relative to |w|.
"""
from dataclasses import dataclass

import numpy as np

from oracle import vae_oracle as O

U = 2.0 ** -24
LR = 1e-3            # the learning rate the kernel tests step with
GRAD_SCALE = 0.25    # a power of two: the scaled gradient stays exact
FP8_SCALE = 16.0
SENTINEL = 7.0
FP8_SENTINEL = 127   # 0x7f is e4m3's NaN: a saturating conversion never writes it


@dataclass(frozen=True)
class Spec:
    name: str
    rows: int
    cols: int
    grad_ld: int
    splits: int
    half: bool = False          # fp16 slabs with unscale tables
    shadows: tuple = ()         # of "bf16", "f32", "fp8"
    shadow_ld: int = 0
    off_rem: int = 0            # arena offset % 8
    slab_rows: int = 0          # rows of one slab (split stride = slab_rows * grad_ld); 0: rows + 1

    @property
    def split_stride(self):
        return (self.slab_rows or self.rows + 1) * self.grad_ld


# ------------------------------------------------------------------------------------------------ the bags
# One spec per path of csrc/adam.h ("optimizer test matrix").  BAG_F32 holds fp32 slabs only, so that the
# optimizer blocks of rv_linear_wgrad_adam take the LDS-DMA ring (adam_stream); BAG_F16 has fp16-slab tensors in it
# and takes the plain-load walk (adam_group<2>).
BAG_F32 = (
    Spec("w4", 24, 64, 72, 4, shadows=("bf16", "fp8"), shadow_ld=64),      # 4-wide, (a+b)+(c+d); fp8 word store
    Spec("w3", 24, 64, 72, 3, shadows=("bf16",), shadow_ld=72),            # the s_ < 3 loops
    Spec("w2", 24, 64, 72, 2),
    Spec("w1", 24, 64, 72, 1, shadows=("bf16",), shadow_ld=64),
    Spec("s5", 16, 32, 32, 5, shadows=("bf16",), shadow_ld=32),            # slab_sum4<true>: a block of four + 1
    Spec("s9", 16, 32, 40, 9, shadows=("fp8",), shadow_ld=32),             # two blocks of four + 1
    Spec("rag3", 50, 37, 44, 3, shadows=("bf16", "fp8"), shadow_ld=40),    # slab_sum4<false>, remainder loop only
    Spec("rag6", 50, 37, 44, 6, shadows=("bf16", "fp8"), shadow_ld=39),    # both loops; byte-wise fp8 stores
    Spec("off1", 8, 16, 16, 2, shadows=("bf16",), shadow_ld=16, off_rem=1),   # aligned shape, offset % 4 == 1
    Spec("ld2", 8, 16, 18, 2, shadows=("bf16",), shadow_ld=16),               # grad_ld % 4 == 2
    Spec("tiny", 7, 3, 4, 2, shadows=("bf16",), shadow_ld=8),                 # cols < 4
    Spec("coop16", 1, 200, 208, 16, shadows=("f32",), shadow_ld=208, slab_rows=2),   # one wave per group
    Spec("coop70", 1, 77, 80, 70, shadows=("f32",), shadow_ld=80, slab_rows=2),      # second trip of s += 64; ragged
    Spec("bias3", 1, 77, 80, 3, shadows=("f32",), shadow_ld=80, slab_rows=2),        # a bias row with few partials
)
BAG_F16 = (
    Spec("h_wide4", 40, 64, 64, 4, half=True, shadows=("bf16",), shadow_ld=64, slab_rows=40),   # adam_block_wide, ld == cols
    Spec("h_wide8", 40, 64, 72, 8, half=True, shadows=("bf16", "fp8"), shadow_ld=72),           # two blocks of four, ld > cols
    Spec("h_wide3", 40, 64, 64, 3, half=True, shadows=("fp8",), shadow_ld=64),                  # remainder loop only
    Spec("h_36", 40, 36, 40, 4, half=True, shadows=("bf16",), shadow_ld=40),      # cols % 8 != 0: 4-wide, half load_slab4
    Spec("h_s9", 40, 64, 64, 9, half=True, shadows=("bf16",), shadow_ld=64),      # more than 8 slabs: not wide
    Spec("h_off4", 40, 64, 64, 4, half=True, shadows=("bf16",), shadow_ld=64, off_rem=4),   # offset % 8 == 4: not wide
    Spec("h_ld2", 12, 36, 38, 5, half=True, shadows=("bf16",), shadow_ld=36),     # scalar: half load_slab1, both loops
    Spec("h_coop", 1, 64, 64, 16, half=True, shadows=("f32",), shadow_ld=64, slab_rows=2),
    Spec("f_w4", 24, 64, 72, 4, shadows=("bf16", "fp8"), shadow_ld=64),           # adam_group's own 4-wide form
    Spec("f_w3", 24, 64, 72, 3, shadows=("bf16",), shadow_ld=64),
    Spec("f_w2", 24, 64, 72, 2),
    Spec("f_w1", 24, 64, 72, 1, shadows=("bf16",), shadow_ld=72),
    Spec("f_rag", 50, 37, 44, 3, shadows=("bf16", "fp8"), shadow_ld=39),
    Spec("f_coop", 1, 200, 208, 16, shadows=("f32",), shadow_ld=208, slab_rows=2),
)
BAGS = {"f32": BAG_F32, "f16": BAG_F16}
STEPS = (1, 2, 1000, 10 ** 6)   # the step counters rv_adam_multi is checked at


class Tensor:
    """Host data of one spec: stored slab values [splits, rows, cols], unscale factors [splits, gr, gc] or None."""

    def __init__(self, spec, offset, slabs, unscale):
        self.spec, self.offset, self.slabs, self.unscale = spec, offset, slabs, unscale

    def terms(self):
        """The slabs as the values they stand for, float64 [splits, rows, cols]."""
        if self.unscale is None:
            return self.slabs
        s = self.spec
        return self.slabs * np.repeat(np.repeat(self.unscale, 32, axis=1), 32, axis=2)[:, :s.rows, :s.cols]

    def grad(self):
        return self.terms().sum(0)


class Bag:
    def __init__(self, specs, tensors, n):
        self.specs, self.tensors, self.n = specs, tensors, n
        self.mask = np.zeros(n, dtype=bool)
        for t in tensors:
            self.mask[t.offset:t.offset + t.spec.rows * t.spec.cols] = True

    def flat(self, per_tensor, fill=0.0):
        """Per-tensor [rows, cols] arrays -> one flat arena array (`fill` outside the tensors)."""
        out = np.full(self.n, fill, dtype=np.float64)
        for t, a in zip(self.tensors, per_tensor):
            out[t.offset:t.offset + a.size] = np.asarray(a, dtype=np.float64).reshape(-1)
        return out

    def grad_flat(self, grad_scale=1.0):
        """The oracle's summed gradient times grad_scale, flat float64."""
        return self.flat([t.grad() for t in self.tensors]) * grad_scale


def make_bag(specs, seed, zero_frac=0.0):
    """Lay `specs` out in an arena and draw their slabs.  zero_frac: that share of every tensor's elements is 0 in
    every slab (an exactly zero gradient)."""
    assert len(specs) <= 16
    rng = np.random.default_rng(seed)
    tensors, cur = [], 0
    for s in specs:
        off = -(-(cur + 8) // 8) * 8 + s.off_rem      # a gap of at least 8 elements in front of every tensor
        slabs = rng.integers(-1024, 1025, size=(s.splits, s.rows, s.cols)).astype(np.float64)
        if zero_frac:
            slabs *= rng.random((s.rows, s.cols)) >= zero_frac
        unscale = None
        if s.half:
            gr, gc = -(-s.rows // 32), -(-s.cols // 32)
            unscale = np.exp2(-rng.integers(4, 13, size=(s.splits, gr, gc)).astype(np.float64))
        else:
            slabs *= 2.0 ** -12
        tensors.append(Tensor(s, off, slabs, unscale))
        cur = off + s.rows * s.cols
    return Bag(tuple(specs), tensors, cur + 8)


def bag(name, zero_frac=0.0):
    return make_bag(BAGS[name], {"f32": 101, "f16": 202}[name] + (7 if zero_frac else 0), zero_frac)


def random_state(n, seed):
    """(m0, v0, w0) as fp32 arrays of a run that starts 'from a random state'."""
    rng = np.random.default_rng(seed)
    return ((0.01 * rng.standard_normal(n)).astype(np.float32), (1e-4 * rng.random(n)).astype(np.float32),
            rng.standard_normal(n).astype(np.float32))


def bf16_gradient(n, seed):
    """A flat gradient of bf16-representable values (the data-parallel payload after its all-reduce)."""
    rng = np.random.default_rng(seed)
    return rng.integers(-128, 129, size=n).astype(np.float64) * 2.0 ** -10


# ------------------------------------------------------------------------------------------------ the update
def adam_reference(g, m0, v0, w0, t, lr=LR):
    """One Adam step in float64 (O.adam_step's formula).  Returns a dict: m, v, w and the terms the bounds need."""
    g, m0, v0, w0 = (np.asarray(a, dtype=np.float64) for a in (g, m0, v0, w0))
    bc1 = 1.0 - O.ADAM_BETA1 ** t
    bc2 = 1.0 - O.ADAM_BETA2 ** t
    m = O.ADAM_BETA1 * m0 + (1.0 - O.ADAM_BETA1) * g
    v = O.ADAM_BETA2 * v0 + (1.0 - O.ADAM_BETA2) * g * g
    denom = np.sqrt(v) / np.sqrt(bc2) + O.ADAM_EPS
    step = lr / bc1
    dw = step * (m / denom)
    tol_m = 4 * U * (0.9 * np.abs(m0) + 0.1 * np.abs(g))
    w = w0 - dw
    return {"m": m, "v": v, "w": w, "dw": dw, "tol_m": tol_m, "tol_v": 5 * U * v,
            "tol_w": 2 * U * np.abs(w) + 32 * U * np.abs(dw) + step / denom * tol_m}


def worst_ratios(ref, m, v, w):
    """max |error| / bound of m, v and w (an error where the bound is 0 counts as infinite)."""
    out = {}
    for k, got in (("m", m), ("v", v), ("w", w)):
        err, tol = np.abs(np.asarray(got, dtype=np.float64) - ref[k]), ref["tol_" + k]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / tol)
        out[k] = float(r.max()) if r.size else 0.0
    return out


def shadow_values(kind, w32, scale=FP8_SCALE):
    """What a shadow holds for the fp32 parameters w32, as an array of bit patterns: bf16 (uint16), f32 (uint32), fp8
    (uint8: e4m3 of clip(fp32(w * scale), -448, 448))."""
    w32 = np.ascontiguousarray(w32, dtype=np.float32)
    if kind == "f32":
        return w32.view(np.uint32)
    if kind == "bf16":
        return (O.bf16_round(w32).view(np.uint32) >> 16).astype(np.uint16)
    x = np.clip(w32 * np.float32(scale), np.float32(-448), np.float32(448))
    return e4m3_bits(np.copysign(O.fp8_e4m3_round(x), x))   # (the sign of a zero is the operand's, as in IEEE conversions)


def e4m3_bits(q):
    """Bit patterns of exactly representable e4m3 values (sign of zero kept)."""
    q = np.asarray(q, dtype=np.float64)
    mag = np.abs(q)
    e = np.floor(np.log2(np.where(mag > 0, mag, 1.0)))
    sub = (mag < 2.0 ** -6)
    field = np.where(sub, 0, e + 7).astype(np.int64)
    mant = np.where(sub, mag * 2.0 ** 9, (mag / np.exp2(e) - 1.0) * 8.0)
    assert np.all(mant == np.rint(mant)) and np.all(mant < 8) and np.all(field < 16)
    return ((np.signbit(q).astype(np.int64) << 7) | (field << 3) | mant.astype(np.int64)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ an fp32 model
def _ulp(x, k):
    x = np.asarray(x, dtype=np.float32)
    if k == 0:
        return x
    return np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)


def adam_model_f32(g, m0, v0, w0, t, lr=LR, k_sqrt=0, k_rcp=0, k_e1=0, k_e2=0):
    """csrc/adam.h's adam_update and adam_step_consts in numpy fp32 (every product and sum rounded once, no
    contraction), with the hardware's square root and reciprocal and the two expm1f results each moved by k ulp."""
    f = np.float32
    g, m, v, w = (np.asarray(a, dtype=f) for a in (g, m0, v0, w0))
    tt = f(t)
    e1 = _ulp(f(np.expm1(np.float64(tt * f(-0.10536051565782628)))), k_e1)
    e2 = _ulp(f(np.expm1(np.float64(tt * f(-0.0010005003335835344)))), k_e2)
    step_size = f(lr) / -e1
    inv_bc2s = f(1.0) / np.sqrt(-e2, dtype=f)
    m = f(0.9) * m + f(0.1) * g
    v = f(0.999) * v + (f(0.001) * g) * g
    denom = _ulp(np.sqrt(v, dtype=f), k_sqrt) * inv_bc2s + f(1e-8)
    w = w - step_size * (m * _ulp(f(1.0) / denom, k_rcp))
    return m, v, w


# ------------------------------------------------------------------------------------------------ device side
class DeviceBag:
    """A bag's device buffers, every one cut from a tests/guarded.py allocation, and its rv_param_desc array.

    Slabs and unscale tables are inputs: gap columns [cols, ld), the extra rows between slabs and the guards hold NaN.
    Shadows are outputs: sentinel-filled with guards (reset_outputs() refills them).  arena() makes a sentinel-filled
    flat arena with guards and the given values inside the tensors."""

    def __init__(self, bag_):
        import torch
        from guarded import guarded
        from rawaudiovae_kelsey_amd._lib import ParamDesc
        self.bag, self.torch = bag_, torch
        self.fp8_scale = torch.full((1,), FP8_SCALE, dtype=torch.float32, device="cuda")
        self.slabs, self.unscale, self.shadows = [], [], []
        self.descs = (ParamDesc * len(bag_.tensors))()
        dt = {"bf16": torch.bfloat16, "f32": torch.float32, "fp8": torch.uint8}
        for i, t in enumerate(bag_.tensors):
            s = t.spec
            sr = s.slab_rows or s.rows + 1
            rows_all = (s.splits - 1) * sr + s.rows
            a = np.full((rows_all, s.cols), np.nan, dtype=np.float32)
            for k in range(s.splits):
                a[k * sr:k * sr + s.rows] = t.slabs[k]
            G = guarded(rows_all, s.cols, s.grad_ld, torch.float16 if s.half else torch.float32, a)
            self.slabs.append(G)
            us = None
            if s.half:
                _, gr, gc = t.unscale.shape
                us = guarded(s.splits * gr, gc, gc + 1, torch.float32, t.unscale.reshape(s.splits * gr, gc))
            self.unscale.append(us)
            sh = {k: guarded(s.rows, s.cols, s.shadow_ld, dt[k], FP8_SENTINEL if k == "fp8" else SENTINEL) for k in s.shadows}
            self.shadows.append(sh)
            self.descs[i] = ParamDesc(
                t.offset, s.rows, s.cols, G.ptr, s.grad_ld, s.split_stride, s.splits,
                sh["bf16"].ptr if "bf16" in sh else None, sh["f32"].ptr if "f32" in sh else None, s.shadow_ld,
                sh["fp8"].ptr if "fp8" in sh else None, self.fp8_scale.data_ptr() if "fp8" in sh else None,
                int(s.half), us.ptr if us else None, us.ld if us else 0, us.rows // s.splits * us.ld if us else 0)

    @property
    def n_desc(self):
        return len(self.bag.tensors)

    def reset_outputs(self):
        for sh in self.shadows:
            for G in sh.values():
                G.flat.fill_(G.fill)

    def arena(self, values=None, dtype=None):
        """A guarded, sentinel-filled flat arena; `values` (flat, bag.n long) go inside the tensors."""
        from guarded import guarded_flat
        torch = self.torch
        G = guarded_flat(self.bag.n, dtype or torch.float32, SENTINEL)
        if values is not None:
            mask = torch.from_numpy(self.bag.mask).cuda()
            G.view[0, mask] = torch.from_numpy(np.asarray(values, dtype=np.float32)[self.bag.mask]).cuda().to(G.dtype)
        return G

    def read(self, G):
        """An arena's payload as a flat fp32 numpy array."""
        return G.view[0].float().cpu().numpy().copy()

    def assert_arena_outside_untouched(self, G, name):
        """The guards and every arena element outside the tensors still hold the sentinel, bit for bit."""
        torch = self.torch
        G.assert_untouched(name)
        it = {torch.float32: torch.int32, torch.bfloat16: torch.int16}[G.dtype]
        want = torch.full((1,), SENTINEL, dtype=G.dtype, device="cuda").view(it)
        outside = G.view[0].view(it)[torch.from_numpy(~self.bag.mask).cuda()]
        bad = int((outside != want).sum())
        assert bad == 0, "%s: %d arena elements between the tensors were written" % (name, bad)

    def assert_shadows(self, w32, name):
        """Every shadow's payload is what shadow_values() derives from the fp32 parameters w32 (flat), bit for bit;
        its gap columns, padding rows and guards still hold the sentinel."""
        torch = self.torch
        it = {"bf16": (torch.int16, np.uint16), "f32": (torch.int32, np.uint32), "fp8": (torch.uint8, np.uint8)}
        for t, sh in zip(self.bag.tensors, self.shadows):
            s = t.spec
            w = w32[t.offset:t.offset + s.rows * s.cols].reshape(s.rows, s.cols)
            for kind, G in sh.items():
                got = G.payload().view(it[kind][0]).cpu().numpy().view(it[kind][1])
                want = shadow_values(kind, w)
                bad = np.argwhere(got != want)
                assert bad.size == 0, "%s: %s shadow of %s differs at %d elements, first (r, c) = %s: %#x, expected %#x" % (
                    name, kind, s.name, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])
                G.assert_untouched("%s: %s shadow of %s" % (name, kind, s.name))
