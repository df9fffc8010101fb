"""Seeded dense operators and template blocks for the two projection GEMMs, gemm_rows_kernel and gemm_narrow_kernel (shared by
test_operator_dense.py and test_gpu_operator_dense.py; NumPy only, no GPU).

The window, binning, chained and fibre operators are banded in k and block-sparse in l: on caseC (Nk = 50, physical templates, relerr's row
scaling) 46 % of the (l, k) -> (a, x) terms of the window product, 34 % of window o binning and 83 % of binning alone contribute less than
the suite's 1e-8 of their output row's maximum.  A term dropped, misplaced or read with a wrong stride there passes every test.  Here every
entry of the operator and of the block is of order one, so every term counts, in two problem kinds:

  integer_problem   entries are integers in [-8, 8]: every product and every partial sum of K = nl_in nx_in <= 900 of them is an integer
                    below 900 x 64 < 2^53, exact in float64 in any order of summation, fused or not.  The expected output is the int64
                    product and the device has to return it bit for bit: a wrong index, stride, mask or tile shows without a tolerance.
  normal_problem    standard-normal entries, the reference is the same product in np.longdouble, beside it the absolute-term sum
                    sum |op| |T| of every output point; the distance is max |device - ref| / abs-sum (loop_synth_util.distance).  This is
                    what catches a precision downgrade: integers survive float32.

bound(K) is derived, not measured: a float64 sum of K products in any order is within K u of its absolute-term sum (u = 2^-53, first order;
each product rounds once, each of the K - 1 adds once, and a term passes through at most K - 1 adds), the narrow kernel adds its four K
quarters with three more adds -> (K + 3) u; the tests assert twice that.

Shapes are (nl_in, nx_in, nl_out, nx_out), as launch_operator reads them: K = nl_in nx_in in nl_in segments of nx_in, ncols = nl_out nx_out
output columns in nl_out groups of nx_out inside a leading dimension padded to 16.  Rows are B x 24 (21 + 3 under a stochastic split)."""
import types

import numpy as np

NROW = 24
U53 = 2.0**-53
K_MAX = 900            # nl nx of the stage-alone engine (Nl = 3, Nk = 300): what eftb_add_operator allows there
INT_MAX = 8            # |entries| of the integer set

# gemm_rows_kernel (ncols > 128): 64 rows x 256 columns per workgroup, wave q owns columns 64 q ... 64 q + 63, K in chunks of 256 padded to 4
ROWS_SHAPES = [
    (3, 257, 3, 43),   # ncols 129: wave 2 owns ONE column, wave 3 is dead; multipole boundaries 43 | 86 inside 16-column tiles; K chunk 2 holds one k, three zero-padded
    (2, 77, 3, 87),    # ncols 261: the second column workgroup has 5 columns; kseg = 77 = 1 mod 4 (an odd chunk: the v1 half of the last pair is masked)
    (3, 258, 1, 300),  # K tail of 2 in the second chunk; nl_out = 1 (one column group: c_colgroup never used); ncols 300 = 256 + 44
    (1, 256, 3, 86),   # K exactly one full chunk, one segment; ncols 258: two columns in the second workgroup
    (3, 50, 3, 50),    # the fixture's own shape (caseC before binning), dense
]
# gemm_narrow_kernel (ncols <= 128): 16 rows per workgroup, the four waves take a quarter of K each (kq = 4 ceil(K / 16)) in trips of 16 k
NARROW_SHAPES = [
    (1, 5, 1, 1),      # K 5: kq 4, wave 1 gets one k, waves 2 and 3 none; one column of one tile
    (3, 7, 2, 9),      # K 21: kq 8, segment ends (7 | 14) fall inside a trip and inside a quarter; ncols 18, the group boundary 9 inside tile 0
    (1, 16, 1, 16),    # K 16 and ncols 16: exactly one k-step of 4 per wave, exactly one column tile
    (1, 17, 1, 17),    # one past both: kq 8, wave 2 gets one k and wave 3 none; a second tile of one column
    (3, 50, 3, 18),    # the fixture's shape (caseC binned to 18)
    (3, 256, 2, 64),   # ncols 128 = 16 GN_MAXT: the last width the narrow kernel takes (129 goes to the rows kernel); K 768, kq 192
    (2, 129, 3, 42),   # ncols 126: the eighth tile ragged by two; K 258, kq 68: quarters end inside a segment and off a trip
    (3, 300, 1, 127),  # the largest K there is (900), kq 228 = 14 trips + 4; ncols 127
]
SHAPES = ROWS_SHAPES + NARROW_SHAPES
BATCHES = (1, 3)       # 24 rows: one ragged 64-row tile / one full and one half 16-row workgroup; 72 rows: a batch group ends inside a tile


def kernel_of(shape):
    return "narrow" if shape[2] * shape[3] <= 128 else "rows"


def K_of(shape):
    return shape[0] * shape[1]


def bound(K):
    """twice the first-order bound of a float64 sum of K products in any order plus the three adds of the quarter reduction, per abs-sum"""
    return 2.0 * (K + 3) * U53


def op_shape(shape):
    """(nl_in, nx_in, nl_out, nx_out) -> the shape of the array Engine.add_operator takes, [nl_out, nl_in, nx_out, nx_in]"""
    nl_in, nx_in, nl_out, nx_out = shape
    return (nl_out, nl_in, nx_out, nx_in)


def product(op, templ, dtype):
    """out[b, a, r, x] = sum_{l, k} op[a, l, x, k] templ[b, l, r, k], every operation in dtype (one matrix product, no BLAS for int64 / longdouble)"""
    nl_out, nl_in, nx_out, nx_in = op.shape
    B, _, R, _ = templ.shape
    assert templ.shape == (B, nl_in, R, nx_in)
    A = np.ascontiguousarray(np.asarray(templ).transpose(0, 2, 1, 3)).reshape(B * R, nl_in * nx_in).astype(dtype)
    M = np.ascontiguousarray(np.asarray(op).transpose(1, 3, 0, 2)).reshape(nl_in * nx_in, nl_out * nx_out).astype(dtype)
    return np.ascontiguousarray((A @ M).reshape(B, R, nl_out, nx_out).transpose(0, 2, 1, 3))


def reference(op, templ):
    """-> (the product in np.longdouble, its absolute-term sum sum |op| |templ| per output point)"""
    return product(op, templ, np.longdouble), product(np.abs(op), np.abs(templ), np.float64)


def distance(got, want, abssum):
    """max over points of |got - want| / (absolute-term sum of that point), as loop_synth_util.distance"""
    got, want, abssum = np.asarray(got), np.asarray(want), np.asarray(abssum)
    assert got.shape == want.shape == abssum.shape and np.all(abssum > 0)
    return float(np.max(np.abs(got.astype(np.longdouble) - want) / abssum))


def _rng(shape, seed, kind):
    return np.random.default_rng([seed, kind, *shape])


def integer_operator(shape, seed=0):
    return _rng(shape, seed, 1).integers(-INT_MAX, INT_MAX + 1, size=op_shape(shape)).astype(np.float64)


def normal_operator(shape, seed=0):
    return _rng(shape, seed, 2).standard_normal(op_shape(shape))


def integer_problem(shape, B, seed=0, rows=NROW):
    """-> op [nl_out, nl_in, nx_out, nx_in], templ [B, nl_in, rows, nx_in] (float64 arrays of integers in [-8, 8]) and want
    [B, nl_out, rows, nx_out]: the int64 product as float64 (exact), to be met bit for bit.  The operator depends on (shape, seed) only."""
    assert K_of(shape) <= K_MAX
    op = integer_operator(shape, seed)
    templ = _rng(shape, seed, 3 + 16 * B).integers(-INT_MAX, INT_MAX + 1, size=(B, shape[0], rows, shape[1])).astype(np.float64)
    want = product(op, templ, np.int64)
    assert np.max(np.abs(want)) <= K_of(shape) * INT_MAX**2 < 2**53
    return types.SimpleNamespace(shape=shape, B=B, op=op, templ=templ, want=want.astype(np.float64))


def normal_problem(shape, B, seed=0, rows=NROW):
    """-> op, templ (standard normal), ref (np.longdouble) and abssum (float64) [B, nl_out, rows, nx_out], bound.  The operator depends
    on (shape, seed) only."""
    op = normal_operator(shape, seed)
    templ = _rng(shape, seed, 4 + 16 * B).standard_normal((B, shape[0], rows, shape[1]))
    ref, abssum = reference(op, templ)
    return types.SimpleNamespace(shape=shape, B=B, op=op, templ=templ, ref=ref, abssum=abssum, bound=bound(K_of(shape)))


def split_rows(main, stochastic):
    """the output of add_operator(op, stochastic=op2): rows 0-20 (P11l, Pctl, Ploopl) of the product with op, rows 21-23 (Pstl) of that with op2"""
    out = np.array(main)
    out[:, :, NROW - 3 :] = stochastic[:, :, NROW - 3 :]
    return out


def per_tracer(products):
    """products[t] [B, ...]: the whole batch through tracer t's matrix -> entry b takes products[b % ntr][b] (batch entry = walker x ntr + tracer)"""
    ntr = len(products)
    out = np.array(products[0])
    for t in range(1, ntr):
        out[t::ntr] = products[t][t::ntr]
    return out


def zeroed_entry(op, a, l, x, k):
    """a kernel that drops one term: the operator with entry (a, l, x, k) zeroed"""
    out = np.array(op)
    out[a, l, x, k] = 0.0
    return out


def moved_entry(op, a, l, x, k):
    """a kernel that reads one term at the neighbouring k: entries (a, l, x, k) and (a, l, x, k + 1) exchanged (cyclic in k)"""
    out = np.array(op)
    k2 = (k + 1) % op.shape[3]
    out[a, l, x, k], out[a, l, x, k2] = op[a, l, x, k2], op[a, l, x, k]
    return out
