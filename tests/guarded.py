"""Strided views with guard bands for the leading-dimension tests (tests/test_gemm_strides_gpu.py).

guarded(rows, cols, ld, dtype, fill) cuts a [rows, cols] view with row stride `ld` from the inside of one flat
allocation the test owns:

    | front guard | row 0: cols payload, ld - cols gap | row 1: ... | ... | back guard |

  - both guards are multiples of 64 elements, so the view's base keeps the 16-byte alignment of the allocation;
  - the back guard is at least as large as the payload (rows * ld elements): a kernel that walks the view with a wrong
    stride of up to twice the right one still stays inside memory the test owns, and the test fails on a comparison;
  - an OUTPUT (fill = a number, SENTINEL by default) is filled with that number everywhere -- guards, gap columns
    [cols, ld) of every row and payload.  After the call assert_untouched() compares guards and gaps with the fill bit for
    bit (through an integer view), naming the region that was hit.  That every payload element was written follows from
    the bit comparison with the packed call's output, which the tests fill with ANOTHER number (PACKED_FILL): an element
    neither call wrote differs, and an element only one of them skipped differs unless the value the other one wrote IS
    the fill, i.e. the skipped store would have changed nothing;
  - an INPUT (fill = an array [rows, cols]) has NaN in its guards and gap columns: any read of them poisons the result
    and fails the value check;
  - an INPUT with `guard` = an array of rows has those rows, flattened and repeated, in its guards and gap columns
    instead of NaN.  The back guard's copy starts at its first element and the front guard's ends at its last, so with
    ld == cols == the guard rows' width the view's row `rows + i` IS guard row i (mod their number) and row -1 the
    last one.  Two uses.  An ATTRACTIVE guard: in a nearest-neighbour search NaN never wins, so a corpus or node row
    read past the end would lose silently behind NaN guards; with copies of the query rows there it is at distance 0,
    wins, and the exact comparison with the oracle fails on an index >= rows.  And integer inputs, which have no NaN:
    their guards hold values the kernel must not act on (indices past the table, for instance).

Dtypes: the 16- and 32-bit floats and uint8 of the GEMM tests, and float64, int32 and int64 (sums, counts, indices).
An integer or fp64 output is checked like any other: its guards against the bits of the fill.  INT_FILL is a fill for
index outputs that no kernel writes (-1 is "no candidate", 7 a valid index).
"""
import numpy as np
import torch

SENTINEL = 7.0       # what the existing kernel tests fill outputs with
PACKED_FILL = -3.0   # fill of the packed twin of an output (see above)
INT_FILL = -77       # fill of an int32 / int64 output

_INT_OF = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32,
           torch.uint8: torch.uint8,   # (uint8: fp8 images, tests/optimizer_oracle.py)
           torch.float64: torch.int64, torch.int32: torch.int32, torch.int64: torch.int64}
# what an input array is staged as on the host: float32 (then cast on the device) unless that would lose bits
_STAGE_OF = {torch.float64: np.float64, torch.int32: np.int32, torch.int64: np.int64}


def _round64(n):
    return -(-int(n) // 64) * 64


class Guarded:
    def __init__(self, rows, cols, ld, dtype, fill, guard=None):
        assert ld >= cols and rows >= 1 and cols >= 1
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.front = _round64(max(ld, 64))
        self.back = _round64(rows * ld) + 64
        n = self.front + rows * ld + self.back
        self.is_output = np.isscalar(fill)
        stage = _STAGE_OF.get(dtype, np.float32)
        if self.is_output:
            assert guard is None
            self.fill = fill if dtype in (torch.int32, torch.int64) else float(fill)
            self.flat = torch.full((n,), self.fill, dtype=dtype, device="cuda")
        else:
            a = np.array(fill, dtype=stage, order="C")               # a copy: the caller's array may be read-only
            assert a.shape == (rows, cols), (a.shape, rows, cols)
            if guard is None:
                assert dtype.is_floating_point or dtype == torch.uint8, "an integer input needs a guard fill"
                self.flat = torch.full((n,), float("nan"), dtype=dtype, device="cuda")
            else:
                g = np.ascontiguousarray(guard, dtype=stage).reshape(-1)
                assert g.size >= 1
                body = np.resize(g, rows * ld)                           # gap columns; the payload is written below
                front = np.resize(g, -(-self.front // g.size) * g.size)[-self.front:]   # ends on the pattern's end
                host = np.concatenate([front, body, np.resize(g, self.back)])
                self.flat = torch.from_numpy(host).cuda().to(dtype)
            self._body()[:, :cols] = torch.from_numpy(a).cuda().to(dtype)
        self.view = torch.as_strided(self.flat, (rows, cols), (ld, 1), self.front)
        assert self.view.data_ptr() % 16 == 0

    def _body(self):
        return self.flat[self.front:self.front + self.rows * self.ld].view(self.rows, self.ld)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def payload(self):
        """A packed copy of the [rows, cols] payload."""
        return self.view.contiguous()

    def slabs(self, n):
        """The payload as [n, rows / n, cols]: slab s starts at element s * (rows / n) * ld of the view."""
        assert self.rows % n == 0
        return self.payload().view(n, self.rows // n, self.cols)

    def assert_untouched(self, name="output"):
        """Guards and gap columns still hold the fill, bit for bit."""
        assert self.is_output
        it = _INT_OF[self.dtype]
        want = torch.full((1,), self.fill, dtype=self.dtype, device="cuda").view(it)
        bits = self.flat.view(it)
        front, back = bits[:self.front], bits[self.front + self.rows * self.ld:]
        gap = bits[self.front:self.front + self.rows * self.ld].view(self.rows, self.ld)[:, self.cols:]
        for region, t in (("front guard", front), ("gap columns [cols, ld)", gap), ("back guard", back)):
            bad = int((t != want).sum())
            assert bad == 0, "%s: %d elements of the %s were written (rows %d cols %d ld %d)" % (
                name, bad, region, self.rows, self.cols, self.ld)


def guarded(rows, cols, ld, dtype, fill=SENTINEL, guard=None):
    return Guarded(rows, cols, ld, dtype, fill, guard)


def guarded_flat(n, dtype, fill=SENTINEL, guard=None):
    """An output (or input) without a leading dimension: n packed elements between two guards."""
    stage = _STAGE_OF.get(dtype, np.float32)
    return Guarded(1, n, n, dtype, fill if np.isscalar(fill) else np.asarray(fill, dtype=stage).reshape(1, n), guard)
