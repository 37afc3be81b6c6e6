"""Float64 references for ONE fp8 (e4m3) GEMM launch on the very operand images that launch read (tests only).

The fp8 weight path is held to `oracle/vae_oracle.py` only statistically (tests/test_fp8_gpu.py): the oracle recomputes the
whole chain, and a last-bit difference upstream flips an e4m3 rounding downstream.  Here nothing is recomputed: the operand
bytes come from the plan's workspace, are decoded exactly and multiplied in float64, so that what remains between a kernel
and its reference is the fp32 accumulation order and the final rounding.

Everything works on torch tensors (CPU or device) and returns float64 tensors on the operands' device.

  decode(bytes)                     e4m3 bytes -> float64 (exact; the two NaN codes decode to NaN)
  e4m3_round(y) / encode(y)         float64 -> nearest e4m3 value / its byte (ties to even, saturating at +-448)
  fwd / dgrad / wgrad               the four GEMM forms (wgrad per split or summed) on decoded images
  abs_fwd / abs_dgrad / abs_wgrad   sum_k |a_k| |b_k| of every output element: the unit of the accumulation bound
  assert_image                      boundary-aware comparison of an fp8 image with fp8(ref * scale)
"""
import numpy as np
import torch

E4M3_MAX = 448.0
E4M3_TINY = 2.0 ** -9          # the smallest subnormal; every subnormal step is this wide


def _table():
    t = np.zeros(256, np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        if e == 15 and m == 7:
            v = np.nan
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[c] = -v if c & 0x80 else v
    return t


TABLE = _table()
_POS = torch.from_numpy(TABLE[:127].copy())      # codes 0x00..0x7E: increasing values 0 .. 448


def decode(q):
    """uint8 (or float8_e4m3fn) tensor -> float64, exactly."""
    q = q.view(torch.uint8) if q.dtype != torch.uint8 else q
    return torch.from_numpy(TABLE).to(q.device)[q.long()]


def e4m3_round(y):
    """Nearest e4m3 value of float64 `y`: ties to even, subnormal steps of 2^-9 below 2^-6, saturating at +-448 (what the
    device's conversions do; torch's own cast agrees below 464)."""
    y = torch.as_tensor(y, dtype=torch.float64)
    a = y.abs().clamp(max=E4M3_MAX)
    e = torch.floor(torch.log2(a.clamp(min=2.0 ** -6)))
    # log2 of a value just below a power of two may round up to the integer: step back where it did
    e = torch.where(torch.exp2(e) > a.clamp(min=2.0 ** -6), e - 1, e)
    step = torch.exp2(e - 3)
    r = (torch.round(a / step) * step).clamp(max=E4M3_MAX)      # torch.round: half to even; a / step is exact
    return torch.where(y < 0, -r, r)


def encode(y):
    """float64 -> e4m3 byte of `e4m3_round(y)` (zero is 0x00 whatever its sign)."""
    r = e4m3_round(y)
    code = torch.searchsorted(_POS.to(r.device), r.abs().contiguous())
    return (code + 128 * ((r < 0) & (code > 0))).to(torch.uint8)


def f64(t):
    return t.to(torch.float64)


def fwd(aq, bq, dq, bias=None, relu=False):
    """dq * A B^T + bias (optionally ReLU): A [M, K] and B [N, K] e4m3 images, both K-major."""
    y = float(dq) * (decode(aq) @ decode(bq).T)
    if bias is not None:
        y = y + f64(bias)
    return y.clamp(min=0) if relu else y


def abs_fwd(aq, bq, dq):
    return float(dq) * (decode(aq).abs() @ decode(bq).abs().T)


def dgrad(dyq, wq, dq, mask):
    """mask * (dq * dY W): dY [M, K], W [K, N] e4m3 images, mask a boolean [M, N]."""
    return float(dq) * (decode(dyq) @ decode(wq)) * mask


def abs_dgrad(dyq, wq, dq):
    return float(dq) * (decode(dyq).abs() @ decode(wq).abs())


def wgrad(dyq, xq, dq, splits=1, summed=True):
    """dq * dY^T X over the batch: dY [M, K], X [M, N] e4m3 images -> [K, N], or the `splits` partial products over
    consecutive batch slices [splits, K, N] (the split-K slabs of the kernel)."""
    dy, x = decode(dyq), decode(xq)
    m = dy.shape[0] // splits
    parts = torch.stack([float(dq) * (dy[s * m:(s + 1) * m].T @ x[s * m:(s + 1) * m]) for s in range(splits)])
    return parts.sum(0) if summed else parts


def abs_wgrad(dyq, xq, dq):
    return float(dq) * (decode(dyq).abs().T @ decode(xq).abs())


def assert_image(got, ref, scale, delta, floor=None, what="fp8 image"):
    """`got` (e4m3 bytes) against fp8(ref * scale), knowing where a rounding is undecided.

    `delta` bounds |device value - ref| before the scale (a float or a tensor like `ref`, in ref's units; the caller adds what
    the fp32 multiplication by the scale may add).  y = ref * scale then lies in [y - w, y + w] with w = delta * scale, and:
      * where both ends round to the same e4m3 value -- no rounding boundary (a midpoint between two codes, subnormal steps
        and the step to 448 included; beyond 448 everything saturates and nothing is undecided) within w of y -- the image
        must hold exactly that value;
      * elsewhere it may hold either end's value, which must be neighbouring codes: w has to stay below one e4m3 step.
    `floor`: a boolean tensor; where set, the device raises a scaled value to at least 2^-9 before converting (the ReLU
    mask read from an fp8 image must not lose a positive activation: common.h, fp8_keep_positive).
    Values are compared, not bytes: +0 and -0 are the same image.  Returns the share of elements in a boundary zone; callers
    cap it (1 %), which keeps the undecided set from growing into an allowance."""
    got = got.view(torch.uint8) if got.dtype != torch.uint8 else got
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    g = decode(got)
    assert not bool(torch.isnan(g).any()), "%s: NaN codes" % what
    y = f64(ref) * float(scale)
    w = torch.as_tensor(delta, dtype=torch.float64, device=y.device) * abs(float(scale))
    lo, hi = y - w, y + w
    if floor is not None:
        lo = torch.where(floor, lo.clamp(min=E4M3_TINY), lo)
        hi = torch.where(floor, hi.clamp(min=E4M3_TINY), hi)
    lo, hi = e4m3_round(lo), e4m3_round(hi)
    zone = lo != hi
    # neighbouring codes: no e4m3 value strictly between the two ends
    mid = e4m3_round((lo + hi) / 2)
    assert bool(((mid == lo) | (mid == hi)).all()), "%s: delta spans more than one e4m3 step" % what
    bad = (g != lo) & (g != hi)
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements are neither rounding of the reference; first at %s: got %r, ref * scale %r "
                             "(+- %r) rounds to %r / %r" % (what, int(bad.sum()), bad.numel(), i, float(g[i]), float(y[i]),
                                                           float(w[i]) if w.dim() else float(w), float(lo[i]), float(hi[i])))
    return float(zone.double().mean())


def assert_close(got, ref, tol, what):
    """Per element |got - ref| <= tol (tensors of one shape); the message names the worst element."""
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err = (f64(got) - ref).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64, device=err.device).expand_as(err)
    bad = ~(err <= tol)          # (a NaN is out of tolerance)
    if bool(bad.any()):
        i = tuple(int(v) for v in np.unravel_index(int(torch.nan_to_num(err - tol, nan=float("inf")).argmax()), err.shape))
        raise AssertionError("%s: %d of %d elements out of tolerance; worst at %s: got %r, ref %r, |diff| %.3e > tol %.3e"
                             % (what, int(bad.sum()), bad.numel(), i, float(f64(got)[i]), float(ref[i]), float(err[i]),
                                float(tol[i])))


def bf16_half_ulp(v):
    """Half the spacing of bf16 at the (bf16) values `v`, as float64: what rounding to nearest may have moved them by."""
    a = f64(v).abs().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 8)


def accumulation_excess(got, ref, unit, rounding):
    """The largest |got - ref| that `rounding` (per element) does not explain, in units of `unit` = dq sum|a||b|: the
    accumulation error a launch is measured by.  Elements whose unit is zero (all products zero) must be exact."""
    err = ((f64(got) - ref).abs() - rounding).clamp(min=0)
    assert not bool(((unit == 0) & (err > 0)).any()), "an element without a single non-zero product differs from its reference"
    return float((err / unit.clamp(min=1e-300)).max())


# ---- accumulation bounds, in units of dq * sum_k |a_k||b_k| per output element
# The ceiling: fp32 round-to-nearest accumulation of K products in ANY order errs by at most K * 2^-24 units.
U = 2.0 ** -24


def ceiling(K):
    return K * U


# Asserted bounds per launch kind ("dp1" excepted, see there): 4 x the largest |got - ref| / unit that the launch showed against the float64 reference
# on an MI355X (profiles/fp8_images_summary.txt lists the maxima per shape and tile; the margin is the one the RNG tests
# took: the maximum over a few million elements is not the maximum over all inputs).  bf16 outputs show it where the
# reference lies next to a bf16 rounding boundary (the part of |got - ref| that half a bf16 ulp does not explain).
ACC = {
    "fc1": 273 * U,      # fp8 forward, bias + ReLU epilogue: 68.2 measured (K = 256; 34.8 and 29.7 at the other shapes)
    "fc4": 434 * U,      # fp8 forward, tanh + loss epilogue: 108.3 measured beyond the tanh tolerance (K = 512, B = 65536)
    "fc3": 1 * U,        # bf16 fc3 inside the latent forward / as a GEMM (K = Lp): 0.22 measured; h3's fp8 image and maxima
    "dgrad": 138 * U,    # fp8 pair, dgrad blocks: 34.4 measured (K = 512; 23.9 - 28.4 at K = 1024)
    "wgrad4": 263 * U,   # fp8 pair, wgrad blocks, fp32 slabs summed: 65.6 measured (K = 2048; 29.0, 22.7 at 4096, 6144)
    "wgrad1": 107 * U,   # fc1's fp8 weight gradient beside the optimizer riders: 26.6 measured (K = 4096)
    # the heads' backward has no fp32 or bf16 output to measure it on in this form: the bf16 MFMA chain rounds once per
    # 32-deep instruction and once per reduction level behind it, (K / 32 + 2) times in all at K = 2 Lp = 128
    "dp1": 6 * U,
}
# Every bound above stays under the ceiling of the smallest K its launch is tested at, and every MEASURED value under the
# ceiling of its own K (tests/test_fp8_images_gpu.py asserts both) -- except, for the 4 x margin only, the two forward
# kinds at these K.  At K = 256 -- two f8f6f4 MFMA instructions per output -- fc1 is already 68 units off, a quarter of
# the any-order ceiling, where the bf16 GEMMs stay far below one unit, and the error does not grow with K (it is 30 at
# K = 512 and 17 - 40 for fc4 at K = 1024 - 4096).  That is consistent with products aligned to the block's largest
# exponent inside the instruction rather than added in fp32 round-to-nearest steps; the measurements do not prove it (every
# one of them is under the any-order ceiling).  With a 4 x margin on such a measurement the ceiling cannot hold at the
# smallest K; the measured maxima are reported, not widened.
ABOVE_CEILING = {"fc1": (256,), "fc4": (384,)}
