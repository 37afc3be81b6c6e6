"""tests/moment_oracle.py on the CPU: that its bit-for-bit restatements are the operations the existing GPU tests hold
the kernels to (each stays inside the bound those tests use against numpy.cov, walk_oracle.lagcov, pca_oracle's apply
forms, walk_oracle.dynamics and the longdouble step), that states_oracle.fma is the exact fma on operands drawn from
the test inputs, and that the inputs of every RV_PCA_MOMENTS and RV_PCA_LAGCOV case of tests/test_moment_edges_gpu.py
tell a wrong kernel from a right one.

The wrong restatements.  Each changes which rows enter a range's chain, or in which order:
  swap    two adjacent rows added in swapped order: rows 0 | 1, the rows on either side of the edge between two MFMAs
          (four rows each) and between two chunks nearest the middle of the first range, the last two of every range
  groups  every MFMA's four rows added in reverse
  drop    a chunk's last row dropped (row 31, the last row of the last full chunk, the last row of all)
  edge    a range's last row added first in the next range, or the next range's first row added last in this one
  keep    a pair that crosses a file end counted all the same (RV_PCA_LAGCOV), every file end in turn
Each is evaluated on every element the GPU test compares.  An instance applies to a case when the rows it moves exist
and, for the lag-1 moment, are pairs of one file (a dropped pair enters as +0 wherever it is added, so moving it changes
nothing).  Every instance that applies must differ in bits in at least one compared element; every case has one that
applies, and every case of more than one range has an `edge` instance that does.  Two instances cannot show and are
asserted EQUAL instead: the swap at T = 2 of the covariance (the mean of two fp32 values is exact, so d_0 = -d_1 and the
two products are the same number), and the covariance's mirror recomputed in the other operand order (fma(a, b, c) =
fma(b, a, c)).

How much shows.  A dropped row, a moved edge and reversed groups change a large share of the elements.  One swapped pair
inside a chain of thousands changes one rounding; on the correlated corpora that reaches the result in 1 to 16 elements
of a few thousand (and in hundreds at T = 300), and in none for some swaps of five cases,
which therefore use moment_oracle.white_rows.  The test prints
the count per instance (-s).
"""
from fractions import Fraction

import numpy as np
import pytest

import moment_oracle as M
import pca_oracle as PO
import walk_oracle as WO
from states_oracle import RANGE, fma

U53 = 2.0 ** -53


def _differs(a, b):
    return not np.array_equal(a.view(np.int64), b.view(np.int64))


def _count(a, b):
    return int(np.count_nonzero(a.view(np.int64) != b.view(np.int64)))


def _instances(n, kept):
    """(name, schedule) of every wrong schedule that applies to n rows of which kept [n] (bool) count"""
    base = M.default_schedule(n)
    out = []
    for p in M.swap_positions(n):
        if kept[p] and kept[p + 1]:
            out.append(("swap %d|%d" % (p, p + 1), M.swapped(base, p)))
    if n >= 4:
        out.append(("groups", M.reversed_groups(base)))
    for p in M.drop_positions(n):
        if kept[p]:
            out.append(("drop %d" % p, M.dropped(base, p)))
    for r in range(len(base) - 1):
        if kept[(r + 1) * RANGE - 1]:
            out.append(("edge %d back" % r, M.edge_moved(base, r, True)))
        if kept[(r + 1) * RANGE]:
            out.append(("edge %d forward" % r, M.edge_moved(base, r, False)))
    return base, out


def _check_instances(name, n, kept, operands, shape, divisor):
    base, wrong = _instances(n, kept)
    right_parts = M.range_partials(operands, shape, base)
    right = M.range_total(right_parts, shape, divisor)
    kinds, counts = set(), []
    for what, schedule in wrong:
        got = M.range_total(M.range_partials(operands, shape, schedule, (base, right_parts)), shape, divisor)
        counts.append("%s: %d" % (what, _count(got, right)))
        assert _differs(got, right), "%s: '%s' gives the right bits: the case cannot tell it apart" % (name, what)
        kinds.add(what.split()[0])
    print("%s, elements of %d that differ: %s" % (name, right.size, ", ".join(counts)))
    assert wrong, "%s: no wrong restatement applies" % name
    assert len(base) == 1 or "edge" in kinds, "%s: no range edge is tested" % name
    return right, kinds


@pytest.mark.parametrize("T,L", M.MOMENT_CASES)
def test_every_moments_case_tells_the_wrong_covariances_apart(T, L):
    x = M.moment_input(T, L)
    rows = M.compared_rows(T, L)
    operands, shape = M.covariance_operands(x, rows)
    name = "moments (%d, %d)" % (T, L)
    if T == 2:
        # d_0 = -d_1 exactly: the swap cannot show (asserted equal); the dropped last row does, so one instance applies.
        # L = 1: there is no mirrored element, so the mirror's operand order has nothing to be checked on.
        base = M.default_schedule(T)
        right = M.covariance_bits(x, rows)
        assert not _differs(M.covariance_bits(x, rows, M.swapped(base, 0)), right)
        assert _differs(M.covariance_bits(x, rows, M.dropped(base, 1)), right)
        return
    right, kinds = _check_instances(name, T, np.ones(T, bool), operands, shape, float(T - 1))
    assert {"swap", "groups", "drop"} <= kinds
    assert not _differs(right, M.covariance_bits(x, rows))
    # the mirror in the other operand order: EXPECTED EQUAL, fma(a, b, c) = fma(b, a, c) and d is the same on both sides
    assert not _differs(M.covariance_bits(x, rows, mirror=False), right)
    assert rows[-1] == 0 or np.any(np.arange(L)[None, :] < rows[:, None])       # there is a mirrored element to compare


@pytest.mark.parametrize("lengths,L", M.LAG_CASES)
def test_every_lagcov_case_tells_the_wrong_moments_apart(lengths, L):
    x, rs, c = M.lag_input(lengths, L)
    T = x.shape[0]
    rows = M.compared_rows(T, L)
    keep = WO.pair_mask(rs, T)
    operands, shape = M.lagcov_operands(x, rs, c, rows)
    name = "lagcov %s L %d" % (lengths, L)
    right, kinds = _check_instances(name, T - 1, keep, operands, shape, float(T - 1))
    assert not _differs(right, M.lagcov_bits(x, rs, c, rows))
    # a keep flag ignored: every dropped pair in turn, the ones at a range edge among them
    ends = np.flatnonzero(~keep)
    assert ends.size == len(lengths) - 1
    for p in ends:
        forgot = keep.copy()
        forgot[p] = True
        got = M.lagcov_bits(x, rs, c, rows, keep=forgot)
        assert _differs(got, right), "%s: the file end at pair %d cannot show" % (name, p)


def test_the_cases_put_a_file_end_on_before_and_after_a_range_edge():
    at = {lengths: set(np.flatnonzero(~WO.pair_mask(WO.row_start(lengths), sum(lengths))).tolist())
          for lengths, _ in M.LAG_CASES}
    assert RANGE - 1 in at[(4096, 2, 300)]          # the last pair of range 0
    assert RANGE - 2 in at[(4095, 3)]               # one before
    assert RANGE in at[(4097, 1, 4095)] and RANGE + 1 in at[(4097, 1, 4095)]     # the first pairs of range 1
    assert sum((4097, 1, 4095)) - 1 == 2 * RANGE and sum((8194,)) - 1 == 2 * RANGE + 1   # a full last range; one pair over
    assert {L for _, L in M.LAG_CASES} == {3, 65, 70, 129, 321, 512}
    assert all(sum(lengths) <= 700 and len(lengths) > 1 for lengths, L in M.LAG_CASES if L > 256)


def test_fma_is_the_exact_fma_on_operands_of_the_test_inputs():
    x = M.moment_input(4097, 129)
    d = x.astype(np.float64) - PO.blocked_mean(x)
    a, b = d[:80, :50].ravel(), d[80:160, 50:100].ravel()
    c = np.cumsum(a * b)                                  # accumulators of the size the chains reach
    c[::7] = 0.0
    c[1::11] *= 2.0 ** -30                                # and ones far below the product
    got = fma(a, b, c)
    want = np.array([float(Fraction(float(p)) * Fraction(float(q)) + Fraction(float(r))) for p, q, r in zip(a, b, c)])
    assert a.size == 4000 and np.array_equal(got.view(np.int64), want.view(np.int64))
    assert np.count_nonzero(got != a * b + c) > 50      # the two roundings of a * b + c are not the same thing


# ---- the restatements are the operations the GPU tests bound -------------------------------------------------------------

@pytest.mark.parametrize("T,L", [(2, 1), (33, 63), (4097, 129), (300, 512)])
def test_covariance_bits_within_the_dot_product_bound_of_numpy_cov(T, L):
    x = M.moment_input(T, L)
    rows = M.compared_rows(T, L)
    ref = np.atleast_2d(np.cov(x.astype(np.float64), rowvar=False))
    sd = np.sqrt(np.diag(ref))
    bound = (T + 8) * U53 * np.outer(sd, sd)[rows]
    err = np.abs(M.covariance_bits(x, rows) - ref[rows])
    assert np.all(err <= bound)


@pytest.mark.parametrize("lengths,L", [((1, 1, 2), 65), ((4095, 3), 65), ((257, 443), 512)])
def test_lagcov_bits_within_the_dot_product_bound_of_the_oracle(lengths, L):
    x, rs, c = M.lag_input(lengths, L)
    T = x.shape[0]
    rows = M.compared_rows(T, L)
    sd = np.sqrt(np.diag(WO.moments(x)[1]))
    bound = (T + 8) * WO.U * np.outer(sd, sd)[rows]
    err = np.abs(M.lagcov_bits(x, rs, c, rows) - WO.lagcov(x, rs, c)[rows])
    assert np.all(err <= bound)


def _tol(ref, terms, L):
    return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + (L + 2) * U53 * terms


@pytest.mark.parametrize("L,k", [(3, 3), (70, 9), (257, 257)])
def test_apply_bits_within_one_ulp_of_the_float64_forms(L, k):
    x, centre, lam, g, h = M.apply_input(L)
    comp = M.rotation(L)[:k]
    y = M.apply_bits(M.PROJECT, x, comp, centre)
    ref, terms = PO.project(x, comp, centre)
    assert y.dtype == np.float32 and np.all(np.abs(y - ref) <= _tol(ref, terms, L))
    ref, terms = PO.reconstruct(y, comp, centre)
    assert np.all(np.abs(M.apply_bits(M.RECONSTRUCT, y, comp, centre) - ref) <= _tol(ref, terms, L))
    ref, terms = PO.edit(x, comp, centre, lam[:k], g[:k], h[:k])
    got = M.apply_bits(M.EDIT, x, comp, centre, lam[:k], g[:k], h[:k])
    assert np.all(np.abs(got - ref) <= _tol(ref, terms, L)) and not np.array_equal(got, x)
    same = M.apply_bits(M.EDIT, x, comp, centre, lam[:k], np.ones(k, np.float32), np.zeros(k, np.float32))
    assert np.array_equal(same.view(np.int32), x.view(np.int32))


@pytest.mark.parametrize("k,L", [(1, 1), (16, 17), (64, 70)])
def test_walk_fit_bits_within_the_bound_of_the_oracles_dynamics(k, L):
    V, lam, C1 = M.fit_input(k, L)
    res = M.walk_fit_bits(V, lam, C1, k)
    ref = WO.dynamics(C1, V, lam, k)
    assert np.all(np.abs(res["A"] - ref["A"]) <= (2 * L + 4) * WO.U * ref["terms"])
    assert np.array_equal(res["Q"], res["Q"].T) and np.allclose(res["Q"], ref["Q"], rtol=0, atol=1e-13)
    assert np.allclose(res["P"], ref["P"], rtol=4 * WO.U, atol=0) and np.allclose(res["R"], ref["R"], rtol=4 * WO.U, atol=0)
    A, Uq, q = M.noise_input(k)
    dyn = M.walk_noise_bits(A, Uq, q)
    assert np.array_equal(dyn[0], A.T) and np.array_equal(dyn[1][q <= 0], np.zeros_like(dyn[1][q <= 0])) and (q <= 0).any()
    dia = M.walk_diagonal_bits(A)
    a, b = np.diag(dia[0]).astype(np.longdouble), np.diag(dia[1]).astype(np.longdouble)
    inside = np.abs(a) <= 1
    assert np.all(np.abs(a * a + b * b - 1)[inside] <= 4 * WO.U) and np.all(b[~inside] == 0) and b[0] == 0


@pytest.mark.parametrize("L,k", [(17, 16), (70, 64)])
def test_walk_step_bits_within_the_bounds_of_the_longdouble_step(L, k):
    dyn, R, c, offset, temperature, eps = M.step_input(L, k)
    n = eps.shape[1]
    w, z = M.walk_step_bits(dyn, R, c, offset, temperature, eps, np.full((3, k), np.nan), np.zeros(3, bool))
    A, B = dyn[0].T, dyn[1].T
    assert np.linalg.norm(A, 2) < 1
    for s in range(3):
        rw, rz, drive, zterms = WO.run(A, B, R, c, eps[s], temperature[s], offset[s])
        sbound = np.arange(1, n + 1) * (2 * k + 2) * WO.U * np.maximum.accumulate(drive)
        assert np.all(np.linalg.norm(w[s] - rw, axis=1) <= sbound)
        zbound = (np.spacing(np.abs(rz).astype(np.float32)).astype(np.float64) + (k + 3) * WO.U * zterms
                  + np.abs(R).sum(0)[None, :] * sbound[:, None])
        assert np.all(np.abs(z[s].astype(np.float64) - rz) <= zbound)
    # two calls of four frames are one call of eight: the second starts primed from the first's state
    w1, z1 = M.walk_step_bits(dyn, R, c, offset, temperature, eps[:, :4], np.zeros((3, k)), np.zeros(3, bool))
    w2, z2 = M.walk_step_bits(dyn, R, c, offset, temperature, eps[:, 4:], w1[:, -1], np.ones(3, bool))
    assert np.array_equal(np.concatenate([w1, w2], 1), w) and np.array_equal(np.concatenate([z1, z2], 1), z)
