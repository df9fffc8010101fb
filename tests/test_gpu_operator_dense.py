"""GPU: the two projection GEMMs, gemm_rows_kernel and gemm_narrow_kernel, on the dense operator sets of operator_dense_util.py.  The
suite's physical operators (window, binning, chained, fibre) are banded in k and block-sparse in l: a third to four fifths of the terms of
their products sit below the suite's 1e-8 (46 % window, 34 % window o binning, 83 % binning alone on caseC), so a dropped, misplaced or
mis-strided term passes there.  Here every term is of order one.

Stage-alone cases (Engine(Nl = 3, Nk = 300), max_batch 4; set_template_dims -> put TEMPL -> apply_operator -> get TEMPL), per shape of
operator_dense_util.SHAPES at B = 1 and B = 3:
  * the integer set has to come back bit for bit, the normal set within 2 (K + 3) 2^-53 of the absolute-term sum of every output point;
  * NaN poison: everything of the input block behind the B live entries (the batch slots B ... max_batch - 1 and the tail of the buffer)
    is NaN -- a read past d.rows multiplied by an operator zero, or by a masked lane, would leak it;
  * sentinels: launch_operator writes the OTHER template block and swaps.  A 1 x 1 operator is applied first to a block that holds a
    sentinel everywhere, so that the operator under test writes into the block that still holds the sentinels; every element behind
    B nl_out 24 nx_out must still hold its sentinel.
Then the stochastic split (21 + 3 rows through two matrices), the per-tracer forms through run(S_PROJECT) (tracers as blockIdx.z, strided
per-tracer launches of either kernel), REDUCE behind three of the cases, and whole-pipeline runs on survey_kgrid(129) with resummation and
AP: direct-P_l runs (PLK0 -> PLK, one row per group, a_row = 0) and templates-first eval_batch runs through a dense random operator, one,
three and nine tracers, against the longdouble product of what the same engine returns with no operator set.  (The AP stage of a direct
run writes P_l to PLK without a PROJECT stage and to PLK0 with one: one kernel, one set of bits, so the un-projected PLK is what the
projection reads; test_direct_projection_reads_the_unprojected_bits asserts that through the identity operator.)

Measured on an MI355X (worst distance per abs-sum; bounds 1.8e-15 at K = 5 ... 2.0e-13 at K = 900):
    stage alone      gemm_rows_kernel 4.9e-16    gemm_narrow_kernel 2.3e-16    stochastic split 4.4e-16 / 1.4e-16 (rows / narrow)
    three tracers    rows, strided    4.9e-16    narrow, z launch and strided 1.6e-16         REDUCE 1.7e-16 (bound 6.0e-15)
    whole pipeline   direct P_l 4.3e-16 (narrow) 7.1e-16 (wide)    templates first 4.6e-16 (narrow) 1.2e-15 (wide)    bound 8.7e-14
Every integer case came back bit for bit, no NaN leaked, every sentinel was intact, the poisoned and the zero-padded block gave the same
bits: no fault was found in either kernel.  The distances are those of float64 itself (the host's own product: 1e-16 ... 5e-16), two to
three decades below the bound and six below the smallest fault of test_operator_dense.py (an operator rounded to float32, 4.8e-9).
Every figure is printed before it is asserted."""
import numpy as np
import pytest

import operator_dense_util as OD
from conftest import relerr
from eftpipe_amd import synth

pytestmark = pytest.mark.gpu
SENTINEL = -12345.678
NK_ALONE, MAX_BATCH = 300, 4
Z = 0.7
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)
WORST = {}


def _note(key, d):
    WORST[key] = max(WORST.get(key, 0.0), d)


def _alone(max_batch):
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.tables import EngineConfig

    eng = Engine(EngineConfig(Nl=3, k=synth.survey_kgrid(NK_ALONE)), max_batch=max_batch)
    eng.unit_op = eng.add_operator(np.ones((1, 1, 1, 1)))
    eng.op_cache = {}
    return eng


@pytest.fixture(scope="module")
def eng4():
    eng = _alone(MAX_BATCH)
    yield eng
    eng.close()
    print("worst distances:", ", ".join("%s %.1e" % kv for kv in sorted(WORST.items())))


@pytest.fixture(scope="module")
def eng6():
    eng = _alone(6)
    yield eng
    eng.close()


def _op(eng, shape, kind, seed=0, stochastic=None):
    """the operator of (shape, kind, seed), registered once per engine -> (id, host array [, host array of the stochastic matrix])"""
    key = (shape, kind, seed, stochastic)
    if key not in eng.op_cache:
        make = OD.integer_operator if kind == "integer" else OD.normal_operator
        op = make(shape, seed)
        op2 = None if stochastic is None else make(shape, stochastic)
        eng.op_cache[key] = (eng.add_operator(op, stochastic=op2), op, op2)
    return eng.op_cache[key]


def _through(eng, shape, templ, launch):
    """templ [B, nl_in, 24, nx_in] through launch(B) with the input block poisoned behind it and the output block full of sentinels
    -> the B live outputs [B, nl_out, 24, nx_out]; the sentinels behind them are asserted here"""
    nl_in, nx_in, nl_out, nx_out = shape
    B = templ.shape[0]
    size = eng.max_batch * eng.Nl * 24 * eng.Nk
    eng.set_template_dims(1, 1)
    eng.put("TEMPL", np.full(size, SENTINEL))
    eng.apply_operator(eng.unit_op, 1)            # writes 24 elements of the other block and swaps: the sentinel block is the next output
    eng.set_template_dims(nl_in, nx_in)
    block = np.full(size, np.nan)
    block[: templ.size] = templ.ravel()
    eng.put("TEMPL", block)
    launch(B)
    out = eng.get("TEMPL", (size,))
    live = B * nl_out * 24 * nx_out
    assert eng.dims == (nl_out, nx_out)
    stray = np.nonzero(out[live:] != SENTINEL)[0]
    assert stray.size == 0, ("written behind the live block", shape, B, live + stray[:8], out[live + stray[:8]])
    got = out[:live].reshape(B, nl_out, 24, nx_out)
    assert np.all(np.isfinite(got)), ("NaN leaked from behind the live rows", shape, B)
    return got


def _check_integer(tag, got, want):
    bad = np.argwhere(got != want)
    print("%s integer: %d of %d outputs differ" % (tag, len(bad), want.size))
    assert np.array_equal(got, want), (tag, bad[:8].tolist())


def _check_normal(tag, key, got, ref, abssum, bound):
    d = OD.distance(got, ref, abssum)
    print("%s normal: %.2e of the abs-sum, bound %.2e" % (tag, d, bound))
    _note(key, d)
    assert d < bound, (tag, d, bound)


def _reduce(eng, tag, got, B, kind, seed):
    """S_REDUCE on the block the operator left: PLK = sum_r bias[b, r] TEMPL[b, a, r, x] against the longdouble contraction of the device's own block"""
    from eftpipe_amd import _lib as L

    rng = np.random.default_rng(seed)
    bias = rng.integers(-8, 9, size=(B, 24)).astype(np.float64) if kind == "integer" else rng.standard_normal((B, 24))
    eng.put("BIAS", bias)
    eng.run(L.S_REDUCE, B)
    plk = eng.get("PLK", (B,) + eng.dims)
    ld = np.longdouble
    ref = np.einsum("br,barx->bax", bias.astype(ld), got.astype(ld))
    abssum = np.einsum("br,barx->bax", np.abs(bias), np.abs(got))
    if kind == "integer":
        assert np.max(abssum) < 2**53
        _check_integer(tag + " REDUCE", plk, ref.astype(np.float64))
    else:
        _check_normal(tag + " REDUCE", "reduce", plk, ref, abssum, 2.0 * 27 * 2.0**-53)


REDUCE_BEHIND = {((3, 257, 3, 43), 3), ((3, 7, 2, 9), 3), ((1, 5, 1, 1), 3)}


@pytest.mark.parametrize("B", OD.BATCHES)
@pytest.mark.parametrize("shape", OD.SHAPES, ids=_ids)
def test_stage_alone(eng4, shape, B):
    kern = OD.kernel_of(shape)
    tag = "%-6s %-18s B %d" % (kern, shape, B)
    ip = OD.integer_problem(shape, B)
    oid, op, _ = _op(eng4, shape, "integer")
    assert np.array_equal(op, ip.op)
    got = _through(eng4, shape, ip.templ, lambda n: eng4.apply_operator(oid, n))
    _check_integer(tag, got, ip.want)
    if (shape, B) in REDUCE_BEHIND:
        _reduce(eng4, tag, got, B, "integer", 11)
    pb = OD.normal_problem(shape, B)
    oid, op, _ = _op(eng4, shape, "normal")
    assert np.array_equal(op, pb.op)
    got = _through(eng4, shape, pb.templ, lambda n: eng4.apply_operator(oid, n))
    _check_normal(tag, kern, got, pb.ref, pb.abssum, pb.bound)
    if (shape, B) in REDUCE_BEHIND:
        _reduce(eng4, tag, got, B, "normal", 12)
    # the poison changes nothing: the same call on a block that is zero behind the live entries returns the same bits
    eng4.set_template_dims(shape[0], shape[1])
    clean = np.zeros(MAX_BATCH * 3 * 24 * NK_ALONE)
    clean[: pb.templ.size] = pb.templ.ravel()
    eng4.put("TEMPL", clean)
    eng4.apply_operator(oid, B)
    assert np.array_equal(eng4.get("TEMPL", got.shape), got)


@pytest.mark.parametrize("B", OD.BATCHES)
@pytest.mark.parametrize("shape", [(2, 77, 3, 87), (2, 129, 3, 42)], ids=_ids)
def test_stochastic_split(eng4, shape, B):
    """add_operator(op, stochastic=op2), two independent matrices: rows 0-20 follow op (B x 21 rows in groups of 21), rows 21-23 op2 (B x 3)"""
    kern = OD.kernel_of(shape)
    tag = "%-6s %-18s B %d split" % (kern, shape, B)
    ip = OD.integer_problem(shape, B)
    oid, op, op2 = _op(eng4, shape, "integer", stochastic=7)
    assert not np.array_equal(op, op2)
    got = _through(eng4, shape, ip.templ, lambda n: eng4.apply_operator(oid, n))
    _check_integer(tag, got, OD.split_rows(ip.want, OD.product(op2, ip.templ, np.int64)).astype(np.float64))
    pb = OD.normal_problem(shape, B)
    oid, op, op2 = _op(eng4, shape, "normal", stochastic=7)
    got = _through(eng4, shape, pb.templ, lambda n: eng4.apply_operator(oid, n))
    ref2, abs2 = OD.reference(op2, pb.templ)
    _check_normal(tag, kern + " split", got, OD.split_rows(pb.ref, ref2), OD.split_rows(pb.abssum, abs2), pb.bound)


@pytest.mark.parametrize("shape,stochastic", [((2, 129, 3, 42), False), ((2, 129, 3, 42), True), ((2, 77, 3, 87), False)],
                         ids=["narrow-z", "narrow-strided", "rows-strided"])
def test_three_tracers(eng6, shape, stochastic):
    """set_tracers(3, operators=...) with three independent matrices, B = 6, through run(S_PROJECT): a narrow shape without a stochastic
    matrix is ONE launch with the tracers as blockIdx.z, with one it is three strided launches per row set, and a rows shape is strided;
    every entry has to match the product with its own tracer's matrix"""
    from eftpipe_amd import _lib as L

    B, ntr = 6, 3
    kern = OD.kernel_of(shape)
    tag = "%-6s %-18s tracers%s" % (kern, shape, " split" if stochastic else "")
    launch = lambda n: eng6.run(L.S_PROJECT, n)
    try:
        for kind in ("integer", "normal"):
            ops = [_op(eng6, shape, kind, seed=20 + t, stochastic=(30 + t) if stochastic else None) for t in range(ntr)]
            eng6.set_tracers(ntr, operators=[o[0] for o in ops])
            pb = (OD.integer_problem if kind == "integer" else OD.normal_problem)(shape, B)
            got = _through(eng6, shape, pb.templ, launch)
            if kind == "integer":
                full = [OD.product(o[1], pb.templ, np.int64) for o in ops]
                if stochastic:
                    full = [OD.split_rows(m, OD.product(o[2], pb.templ, np.int64)) for m, o in zip(full, ops)]
                _check_integer(tag, got, OD.per_tracer(full).astype(np.float64))
            else:
                refs = [OD.reference(o[1], pb.templ) for o in ops]
                if stochastic:
                    st = [OD.reference(o[2], pb.templ) for o in ops]
                    refs = [(OD.split_rows(r[0], s[0]), OD.split_rows(r[1], s[1])) for r, s in zip(refs, st)]
                _check_normal(tag, kern + " tracers", got, OD.per_tracer([r[0] for r in refs]), OD.per_tracer([r[1] for r in refs]), pb.bound)
    finally:
        eng6.set_tracers(1)


# ------------------------------------------------------------------------------------------------ whole-pipeline runs
NK_PIPE = 129
PIPE_OPS = {"narrow": (3, NK_PIPE, 3, 20), "wide": (3, NK_PIPE, 3, 60)}
BS, ES = [2.14, 0.55, 0.77, 0.55, -1.84, -1.89, -1.49], (0.26, 0.0, -0.93)


@pytest.fixture(scope="module")
def pipe():
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.tables import EngineConfig

    cfg = EngineConfig(Nl=3, k=synth.survey_kgrid(NK_PIPE), with_resum=True, with_ap=True, DA_AP=float(synth.da_func(synth.OM_AP, Z)),
                       H_AP=float(synth.hubble(synth.OM_AP, Z)))
    eng = Engine(cfg, max_batch=9)
    eng.op_cache = {}
    yield eng
    eng.close()


def _draws(B):
    from eftpipe_amd.parambasis import bias_row

    d = synth.draw_batch(B, z=Z, seed=6100 + B)
    rng = np.random.default_rng(61)
    bs = np.asarray(BS)
    d["bias"] = np.stack([bias_row(float(f), list(bs * (1.0 + 0.2 * rng.standard_normal(bs.size))), None, ES, kmA=0.7, krA=0.25, ndA=4.5e-5) for f in d["f"]])
    return d


def _set_ops(eng, ntr, ids):
    eng.set_tracers(ntr, operators=ids if ntr > 1 else None)
    eng.set_pipeline_operator(ids[0] if ntr == 1 and ids else -1)


def _distance0(got, ref, abssum):
    """operator_dense_util.distance where template rows may vanish identically: such outputs have to be exact zeros"""
    dead = abssum == 0
    assert np.all(got[dead] == 0.0)
    return OD.distance(np.where(dead, 0.0, got), np.where(dead, 0.0, ref), np.where(dead, 1.0, abssum))


@pytest.mark.parametrize("ntr,B", [(1, 3), (3, 6), (9, 9)])
@pytest.mark.parametrize("width", ["narrow", "wide"])
def test_pipeline_through_a_dense_operator(pipe, width, ntr, B):
    """Direct-P_l and templates-first runs with one random dense matrix per tracer.  The direct projection takes the z launch (narrow, up to
    eight tracers), the per-tracer narrow launches (narrow, nine tracers) and the per-tracer rows launches (wide); the templates-first one
    the z launch or the strided launches of launch_operator.  Input to the reference: what the same engine returns with no operator set."""
    eng, shape = pipe, PIPE_OPS[width]
    assert OD.kernel_of(shape) == ("narrow" if width == "narrow" else "rows")
    bound = OD.bound(OD.K_of(shape))
    d = _draws(B)
    args = (d["Pin"], d["f"], d["DA"], d["H"])
    ops = [_op(eng, shape, "normal", seed=40 + t) for t in range(ntr)]
    tag = "pipeline %-6s %d tracer(s) B %d" % (width, ntr, B)
    try:
        # ---- what the projection reads
        _set_ops(eng, 1, [])
        eng.set_plk_direct(False)
        T0, P0t = eng.eval_batch(*args, bias=d["bias"])
        eng.set_plk_direct(True)
        P0 = eng.eval_batch(*args, bias=d["bias"], templates=False)
        assert np.isfinite(T0).all() and np.isfinite(P0).all()
        assert relerr(P0, P0t) < 1e-9 and not np.array_equal(P0, P0t)     # (identical bits would mean the direct option did nothing)
        # ---- direct P_l through the operators
        _set_ops(eng, ntr, [o[0] for o in ops])
        P1 = eng.eval_batch(*args, bias=d["bias"], templates=False)
        assert P1.shape == (B, shape[2], shape[3])
        refs = [OD.reference(o[1], P0[:, :, None, :]) for o in ops]
        dd = _distance0(P1[:, :, None, :], OD.per_tracer([r[0] for r in refs]), OD.per_tracer([r[1] for r in refs]))
        print("%s direct: %.2e of the abs-sum, bound %.2e" % (tag, dd, bound))
        _note("pipeline direct " + width, dd)
        # ---- templates first through the same operators
        eng.set_plk_direct(False)
        T1 = eng.eval_batch(*args)
        assert T1.shape == (B, shape[2], 24, shape[3])
        refs = [OD.reference(o[1], T0) for o in ops]
        dt = _distance0(T1, OD.per_tracer([r[0] for r in refs]), OD.per_tracer([r[1] for r in refs]))
        print("%s templates first: %.2e of the abs-sum, bound %.2e" % (tag, dt, bound))
        _note("pipeline templates " + width, dt)
        assert dd < bound and dt < bound, (tag, dd, dt, bound)
    finally:
        eng.set_plk_direct(False)
        _set_ops(eng, 1, [])


def test_direct_projection_reads_the_unprojected_bits(pipe):
    """The identity as the pipeline operator of a direct-P_l run (K = 387 with one non-zero term per output: an exact product) returns the
    bits of the run without an operator: PLK0, which the projection reads, holds what PLK holds when no PROJECT stage follows"""
    eng = pipe
    d = _draws(3)
    args = (d["Pin"], d["f"], d["DA"], d["H"])
    key = ("identity",)
    if key not in eng.op_cache:
        eye = np.zeros((3, 3, NK_PIPE, NK_PIPE))
        for a in range(3):
            eye[a, a] = np.eye(NK_PIPE)
        eng.op_cache[key] = eng.add_operator(eye)
    try:
        _set_ops(eng, 1, [])
        eng.set_plk_direct(True)
        P0 = eng.eval_batch(*args, bias=d["bias"], templates=False)
        _set_ops(eng, 1, [eng.op_cache[key]])
        P1 = eng.eval_batch(*args, bias=d["bias"], templates=False)
        assert np.array_equal(P1, P0)
    finally:
        eng.set_plk_direct(False)
        _set_ops(eng, 1, [])
