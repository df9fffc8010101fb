"""The dense operator sets of operator_dense_util.py on the host (no GPU): what test_gpu_operator_dense.py leans on.

  * a float64 product of the normal set (NumPy's, pairwise sums and BLAS blocks: one more order of summation) sits within the derived bound
    2 (K + 3) 2^-53 of the absolute-term sum at every shape and batch -- the bound is no tighter than float64 itself;
  * the integer set is exactly representable: the largest partial sum, K x 64, is below 2^53 by the shape alone, and a float64 product
    returns the int64 product bit for bit;
  * the faults the sets are there for show: ONE zeroed operator entry, ONE entry read at the neighbouring k and an operator rounded to
    float32 each move the normal set by more than 1e6 (float32: 1e4) times the bound on the outputs the entry feeds, and nowhere else;
    the integer set then differs in bits.

Measured here: float64 against longdouble 1e-16 ... 5e-16 of the abs-sum (bounds 1.8e-15 at K = 5 ... 2.0e-13 at K = 900); one dropped term
moves its worst output by 1.6e-4 ... 0.76 of the abs-sum (entries picked by position, not by size), one moved term by 7.7e-4 ... 1.9, a
float32 operator by 4.8e-9 ... 3.5e-8."""
import numpy as np
import pytest

import operator_dense_util as OD

CASES = [(s, B) for s in OD.SHAPES for B in OD.BATCHES]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def test_shape_table():
    """every shape fits the stage-alone engine, sits on the side of the 128-column switch its list says, and the lists reach the edges named"""
    assert len(set(OD.SHAPES)) == len(OD.SHAPES) == 13
    for s in OD.SHAPES:
        assert OD.K_of(s) <= OD.K_MAX and s[2] * s[3] <= OD.K_MAX
    assert all(OD.kernel_of(s) == "rows" for s in OD.ROWS_SHAPES) and all(OD.kernel_of(s) == "narrow" for s in OD.NARROW_SHAPES)
    ncols = lambda s: s[2] * s[3]
    assert min(map(ncols, OD.ROWS_SHAPES)) == 129 and max(map(ncols, OD.NARROW_SHAPES)) == 128   # both sides of the switch
    assert max(map(OD.K_of, OD.SHAPES)) == OD.K_MAX
    assert any(s[1] > 256 and s[1] % 256 == 1 for s in OD.ROWS_SHAPES) and any(s[1] == 256 for s in OD.ROWS_SHAPES)
    assert any(OD.K_of(s) < 8 for s in OD.NARROW_SHAPES)                                           # waves without any k


@pytest.mark.parametrize("shape,B", CASES, ids=_ids)
def test_float64_product_within_the_bound(shape, B):
    pb = OD.normal_problem(shape, B)
    d = OD.distance(OD.product(pb.op, pb.templ, np.float64), pb.ref, pb.abssum)
    e = OD.distance(np.einsum("alxk,blrk->barx", pb.op, pb.templ), pb.ref, pb.abssum)
    print("%-18s B %d K %3d: float64 matmul %.1e einsum %.1e of the abs-sum, bound %.1e" % (shape, B, OD.K_of(shape), d, e, pb.bound))
    assert pb.bound == 2.0 * (OD.K_of(shape) + 3) * 2.0**-53
    assert d < pb.bound and e < pb.bound


@pytest.mark.parametrize("shape,B", CASES, ids=_ids)
def test_integer_products_are_exact(shape, B):
    K = OD.K_of(shape)
    assert K <= 900 and K * OD.INT_MAX**2 < 2**53          # every partial sum of every order, from the shape alone
    pb = OD.integer_problem(shape, B)
    for a in (pb.op, pb.templ, pb.want):
        assert np.array_equal(a, np.rint(a))
    assert np.max(np.abs(pb.op)) == OD.INT_MAX and np.max(np.abs(pb.templ)) <= OD.INT_MAX
    assert np.array_equal(OD.product(pb.op, pb.templ, np.float64), pb.want)
    assert np.array_equal(np.einsum("alxk,blrk->barx", pb.op, pb.templ), pb.want)
    assert np.array_equal(OD.product(pb.op, pb.templ, np.longdouble).astype(np.float64), pb.want)
    # the operator is the same at every batch size (the GPU tests register it once per shape)
    assert np.array_equal(pb.op, OD.integer_problem(shape, 5 - B).op)


def _entries(shape):
    """three operator entries per shape: the first, the last, and one in the middle of the last segment and column group"""
    nl_out, nl_in, nx_out, nx_in = OD.op_shape(shape)
    return [(0, 0, 0, 0), (nl_out - 1, nl_in - 1, nx_out - 1, nx_in - 1), (nl_out - 1, nl_in - 1, nx_out // 2, nx_in // 2)]


@pytest.mark.parametrize("shape", OD.SHAPES, ids=_ids)
def test_single_faults_stand_out(shape):
    B = 3
    pb = OD.normal_problem(shape, B)
    ip = OD.integer_problem(shape, B)
    for (a, l, x, k) in _entries(shape):
        for name, fault in (("zeroed", OD.zeroed_entry), ("moved", OD.moved_entry)):
            if name == "moved" and shape[1] == 1:
                continue
            bad = OD.product(fault(pb.op, a, l, x, k), pb.templ, np.float64)
            err = np.abs(bad.astype(np.longdouble) - pb.ref) / pb.abssum
            touched = np.zeros(err.shape, dtype=bool)
            touched[:, a, :, x] = True
            print("%-18s %s (%d, %d, %d, %d): touched outputs %.1e ... %.1e of the abs-sum, the rest %.1e, bound %.1e" %
                  (shape, name, a, l, x, k, err[touched].min(), err[touched].max(), err[~touched].max() if (~touched).any() else 0.0, pb.bound))
            assert err[touched].max() > 1e6 * pb.bound
            assert np.median(err[touched]) > 1e4 * pb.bound                  # not one lucky output: the typical one
            if (~touched).any():
                assert err[~touched].max() < pb.bound
            # the integer set: any output whose two factors are non-zero differs in bits
            bad = OD.product(fault(ip.op, a, l, x, k), ip.templ, np.float64)
            if name == "zeroed":
                differs = ip.op[a, l, x, k] != 0 and np.any(ip.templ[:, l, :, k] != 0)
            else:
                k2 = (k + 1) % shape[1]
                differs = np.any((ip.op[a, l, x, k] - ip.op[a, l, x, k2]) * (ip.templ[:, l, :, k] - ip.templ[:, l, :, k2]) != 0)
            assert np.array_equal(bad, ip.want) != bool(differs)
            assert np.array_equal(bad[~touched], ip.want[~touched])
    # a precision downgrade, which the integer set cannot see
    op32 = pb.op.astype(np.float32).astype(np.float64)
    d32 = OD.distance(OD.product(op32, pb.templ, np.float64), pb.ref, pb.abssum)
    print("%-18s operator rounded to float32: %.1e of the abs-sum, bound %.1e" % (shape, d32, pb.bound))
    assert d32 > 1e4 * pb.bound
    assert np.array_equal(OD.product(ip.op.astype(np.float32).astype(np.float64), ip.templ, np.float64), ip.want)


def test_split_and_tracer_references():
    """split_rows and per_tracer, the references of the stochastic split and of the per-tracer operators, against plain loops"""
    shape, B = (3, 7, 2, 9), 6
    ops = [OD.integer_operator(shape, seed=s) for s in range(3)]
    assert not np.array_equal(ops[0], ops[1]) and not np.array_equal(ops[1], ops[2])
    pb = OD.integer_problem(shape, B)
    full = [OD.product(o, pb.templ, np.int64) for o in ops]
    sp = OD.split_rows(full[0], full[1])
    assert np.array_equal(sp[:, :, :21], full[0][:, :, :21]) and np.array_equal(sp[:, :, 21:], full[1][:, :, 21:])
    pt = OD.per_tracer(full)
    for b in range(B):
        assert np.array_equal(pt[b], full[b % 3][b])
        assert not np.array_equal(pt[b], full[(b + 1) % 3][b])      # a swapped tracer is unmistakable
