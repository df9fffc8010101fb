"""The draw kernels on the synthetic likelihoods of synth_like_util.py: every workgroup shape of draws_logp_shape and every nG edge of
draws_solve, which the fixture likelihoods never reach (they all run at four waves).  The cases (synth_like_util.CASES; the wave counts are
those of the launcher's formula when the table was written, for the reader):

    case ntr NNLO nG  J1  nl x nx ndata P   reaches
    A    1   no   1   25  3 x 4   9     1   the smallest of everything
    B    1   no   3   25  1 x 11  11    2   nl = 1, nG < ADJ_KB
    C    2   no   5   49  3 x 3   5     3   ntr = 2, ndata < 16
    D    2   yes  4   55  3 x 5   17    3   the NNLO columns of two tracers
    E    1   yes  24  28  3 x 6   16    4   nG max at even J1
    F    3   no   23  73  3 x 5   33    5   TWO, nG odd
    G    4   no   24  97  3 x 5   17    5   nw = 2
    H    4   yes  16  109 3 x 5   53    6   the rows kernel at nw = 4 beside the params kernels at nw = 2
    I    5   no   24  121 3 x 7   53    8   nw = 1; the largest footprint there is
    J    5   no   8   121 3 x 7   53    8   nw = 4 on 154568 (rows) to 163048 (sample) of 163840 bytes; chain and Hessian at nw = 2
    Gf   4   no   24  97  3 x 5   31    5   G with ndata >= nG: a proper flat prior at nw = 2 (the failing-draw tests)
    Ef   1   yes  24  28  3 x 10  27    4   E with ndata >= nG: the same at nw = 4

(The tempering call chooses its own wave count, one per rung: the rungs that fit at each case are temper_util.TEMPER_RUNGS, and its ladders
on these likelihoods are in test_gpu_draw_temper.py.)

Three walkers own 9, 0 and 5 draws: one has none, one more than twice the widest workgroup's waves.  Yardsticks: the data-space ones of
grad_util, hess_util and sample_util around oracle.marginal, pinned on the host by test_draw_synthetic.py; bars: hess_util.device_bar of
synth_like_util.SYNTH_FLOOR.  What the calls promise to share they are asked to share bit for bit, and a draw's bits must not depend on
the wave, or the trip of a wave's loop, that computed it.  The draws reversed within each walker, and split into two calls, return the
same bits: that moves a draw to another workgroup and wave, not to a later trip, because the launcher spreads a walker's draws over up to
2048 / C workgroups and nine draws leave every wave with one.  test_every_wave_loops gives a walker 5463 draws, more than twice what
those workgroups take at four waves, so that every wave of every kernel loops at least twice, failing draws among them.
synth_like_util.CASES states per call whether a shape runs or is refused; nothing passes because everything refused."""
import ctypes as C

import numpy as np
import pytest

import sample_util as SU
import synth_like_util as SY
from hess_util import device_bar
from test_draw_datasets import datasets
from test_gpu_draw_chains import _compare, _records, _stored_records_are_the_draw_call

pytestmark = pytest.mark.gpu

MAIN = [c for c in SY.CASES if c not in ("Gf", "Ef")]
FITS = "does not fit the LDS"


def _engine(pb, entries):
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.tables import EngineConfig

    eng = Engine(EngineConfig(Nl=3, with_NNLO=pb.nnlo), max_batch=entries)
    if pb.ntr > 1:
        eng.set_tracers(pb.ntr)
    eng.set_template_dims(pb.nl, pb.nx)
    return eng


def _put(eng, pb, walker=None):
    """the walkers' templates, or (the LOGP stage) those of walker[d] duplicated per draw"""
    pick = lambda a: a if walker is None else a.reshape((len(pb.counts), pb.ntr) + a.shape[1:])[walker].reshape((-1,) + a.shape[1:])
    eng.put("TEMPL", pick(pb.templ))
    if pb.nnlo:
        eng.put("TEMPLN", pick(pb.templn))


def _like(eng, pb, jeff, rec=None, invcov=None):
    from eftpipe_amd.marginal import MarginalLikelihood

    like = MarginalLikelihood(eng, pb.index, pb.D, pb.invcov if invcov is None else invcov, pb.loc, pb.scale, jeffreys=jeff)
    like.set_draw_recipe(pb.rec if rec is None else rec)
    return like


def _raw_grad(like, theta, off, f):
    """eftb_draws_logp_grad_params itself (the wrapper raises where ln P is NaN) -> logp, grad, full, best"""
    from eftpipe_amd import _lib as L

    theta, off, f = np.ascontiguousarray(theta), np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(f)
    N, P = theta.shape
    logp, grad, full, best = np.empty(N), np.empty((N, P)), np.empty(N), np.empty((N, like.nG))
    L.check(like.eng.lib.eftb_draws_logp_grad_params(like.eng._h, off.size - 1, N, off.ctypes.data_as(C.POINTER(C.c_int64)), L.dptr(theta), L.dptr(f),
                                                     L.dptr(logp), L.dptr(grad), L.dptr(full), L.dptr(best)))
    return logp, grad, full, best


def _param_calls(like, theta, off, f, z, hess, groups=None):
    """the params, gradient, Hessian (where the shape runs) and sample calls, NaN where a draw fails -> a dict of arrays [N, ...]; what the
    calls promise to share is asserted to be shared bit for bit"""
    from eftpipe_amd.engine import _params_args
    from eftpipe_amd.marginal import _groups_args

    if groups is None:
        lp, full, best = _records(like, off, f)(theta)
        lg, grad, fg, bg = _raw_grad(like, theta, off, f)
    else:
        th, o, ff, wk, ds = _groups_args(like._recipe, theta, off, f, like.eng.ntracers, groups)
        lp, _, _, full, best = like._draws_groups_raw(th, o, ff, wk, ds, grad=False, hess=False)
        lg, grad, _, fg, bg = like._draws_groups_raw(th, o, ff, wk, ds, grad=True, hess=False)
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    assert same(lg, lp) and same(fg, full) and same(bg, best)
    out = dict(logp=lp, full=full, best=best, grad=grad)
    if hess:
        if groups is None:
            lh, gh, hh, fh, bh = like._draws_hess_raw(*_params_args(like._recipe, theta, off, f, like.eng.ntracers))
        else:
            lh, gh, hh, fh, bh = like._draws_groups_raw(th, o, ff, wk, ds, grad=True, hess=True)
        assert same(lh, lp) and same(fh, full) and same(bh, best) and same(gh, grad)
        assert same(hh, hh.transpose(0, 2, 1))
        out["hess"] = hh
    r = like._sample_raw(theta, off, f, z, groups=groups)
    assert same(r.logp, lp) and same(r.fullchi2, full) and same(r.best, best)
    out["b"], out["chi2"] = r.b, r.chi2
    return out


def _report(tag, call, worst, floors):
    print(tag, call + ":", ", ".join("%s %.1e (bar %.1e)" % (k, v, device_bar(floors[k])) for k, v in worst.items()))
    for k, v in worst.items():
        assert v < device_bar(floors[k]), (tag, call, k, v, device_bar(floors[k]))


def _reorder_and_split(like, pb, off, z, base, hess):
    """the draws reversed within each walker, and each walker's draws split over two calls: the same bits draw for draw (every draw lands
    in another workgroup or on another wave; no wave takes a second draw here: test_every_wave_loops)"""
    counts = np.array(pb.counts)
    perm = np.concatenate([np.arange(off[c], off[c + 1])[::-1] for c in range(len(counts))])
    got = _param_calls(like, pb.theta[perm], off, pb.f, z[perm], hess)
    for k, a in got.items():
        assert np.array_equal(a, base[k][perm]), ("reversed", k)
    cut = (counts + 1) // 2 - (counts > 6)  # 9 -> 4 + 5, 5 -> 3 + 2: the second halves start on other workgroups and waves than in the whole
    sel_a = np.concatenate([np.arange(off[c], off[c] + cut[c]) for c in range(len(counts))])
    sel_b = np.concatenate([np.arange(off[c] + cut[c], off[c + 1]) for c in range(len(counts))])
    for sel, cnt in ((sel_a, cut), (sel_b, counts - cut)):
        got = _param_calls(like, pb.theta[sel], SY.offsets(cnt), pb.f, z[sel], hess)
        for k, a in got.items():
            assert np.array_equal(a, base[k][sel]), ("split", k)


@pytest.mark.parametrize("case", MAIN)
def test_every_call_at_every_shape(case):
    from eftpipe_amd import _lib as L

    runs = SY.CASES[case]["runs"]
    # (every call below but the Hessian's is made outright, so a refusal fails the test; a table that expects one needs a test of it)
    assert all(runs[k] for k in ("rows", "stage", "params", "grad", "sample", "chain"))
    pb0 = SY.case_problem(case)
    N, nG, ntr, P = pb0.theta.shape[0], pb0.nG, pb0.ntr, pb0.P
    off, walker = SY.offsets(pb0.counts), pb0.walker
    eng = _engine(pb0, max(N, len(pb0.counts)) * ntr)
    _put(eng, pb0)
    z = SY.normals(N, SY.S5, nG)
    fd = pb0.f[walker]
    rng = np.random.default_rng(61)
    chain_in = dict(theta0=pb0.theta, step=0.02 * rng.standard_normal((N, 6, P)), lnu=np.log(rng.uniform(size=(N, 6))))
    for kind in SY.kinds(case):
        pb = SY.case_problem(case, kind)
        floors = SY.SYNTH_FLOOR[case][kind]
        for jeff in SY.jeffreys_of(case, kind):
            tag = "%s %s%s" % (case, kind, " jeffreys" if jeff else "")
            ref = SY.reference(case, kind, jeff)
            like = _like(eng, pb, jeff)
            hess = runs["hess_jeffreys" if jeff else "hess"]
            # ---- the params, gradient, Hessian and sample calls: shared bits, then the yardsticks
            base = _param_calls(like, pb.theta, off, pb.f, z, hess)
            assert all(np.all(np.isfinite(a)) for a in base.values())
            if not hess:
                with pytest.raises(L.EftbError, match="the Hessian of P = %d parameters with nG = %d and J \\+ 1 = 121 columns %s" % (P, nG, FITS)):
                    like.logp_draws_params(pb.theta, off, pb.f, grad=True, hess=True)
            r5 = like.sample_gaussian_params(pb.theta, off, pb.f, z)
            assert np.array_equal(r5.b, base["b"]) and np.array_equal(r5.chi2, base["chi2"])
            r1 = like.sample_gaussian_params(pb.theta, off, pb.f, z[:, 2])  # S = 1: sample 2 of the S = 5 call alone
            assert np.array_equal(r1.b[:, 0], r5.b[:, 2]) and np.array_equal(r1.chi2[:, 0], r5.chi2[:, 2]) and np.array_equal(r1.logp, r5.logp)
            r0 = like.sample_gaussian_params(pb.theta, off, pb.f, np.zeros((N, 1, nG)))  # z = 0: the best fit and its chi2
            assert np.array_equal(r0.b[:, 0], r5.best) and np.array_equal(r0.chi2[:, 0], r5.fullchi2)
            rn = like.sample_gaussian_params(pb.theta, off, pb.f, np.tile(np.eye(nG), (N, 1, 1)))  # S = nG, z = 1: the covariance
            errs = [SY.errors(pb, d, ref[d], z[d], base["logp"][d], base["full"][d], base["best"][d], base["grad"][d], base["hess"][d] if hess else None,
                              r5.b[d], r5.chi2[d], rn.b[d] - rn.best[d]) for d in range(N)]
            _report(tag, "params / grad / hess / sample", SY.worst(errs), floors)
            for d in range(N):
                ff, tw, tn = SY.of_walker(pb, walker[d])
                assert np.allclose(r5.chi2[d], SU.chi2_at(pb.rec, pb.theta[d], ff, tw, pb.index, pb.D, pb.invcov, r5.b[d], tn), rtol=1e-9, atol=0)
            _reorder_and_split(like, pb, off, z, base, hess)
            # ---- the chain call: T = 6 steps under Gaussian theta priors are the host loop around logp_draws_params, every state's record included
            got, _ = _compare(like, off, pb.f, chain_in, 1, prior_loc=np.ones(P), prior_scale=np.full(P, 0.5))
            assert np.all(np.isfinite(got.logp)) and np.any(got.naccept > 0)
            _stored_records_are_the_draw_call(like, off, pb.f, got)
            assert np.array_equal(like.logp_draws_params(pb.theta, off, pb.f), base["logp"])
            # ---- the rows call on DrawRecipe.rows
            rows, rn_ = pb.rec.rows(pb.theta, fd), pb.rec.rows_nnlo(pb.theta, fd) if pb.nnlo else None
            lr, fr, br = like.logp_draws(rows, off, return_best=True, rows_nnlo=rn_)
            _report(tag, "rows", SY.worst([SY.errors(pb, d, ref[d], None, lr[d], fr[d], br[d], None, None, None, None, None) for d in range(N)]), floors)
            # ---- the LOGP stage on the walkers' templates duplicated per draw
            _put(eng, pb, walker)
            ls, fs, bs = like.logp(rows.reshape(N * ntr, nG + 1, 24), return_best=True, rows_nnlo=None if rn_ is None else rn_.reshape(N * ntr, nG + 1, 3))
            _report(tag, "stage", SY.worst([SY.errors(pb, d, ref[d], None, ls[d], fs[d], bs[d], None, None, None, None, None) for d in range(N)]), floors)
            _put(eng, pb)
            assert np.array_equal(like.logp_draws_params(pb.theta, off, pb.f), base["logp"])  # the Gram block rebuilt: the same bits
    eng.close()


@pytest.mark.parametrize("ndata", list(SY.WIDE))
def test_logp_stage_past_one_column_group(ndata):
    """U = V C^-1 of the LOGP stage (launch_times_invcov: gemm_narrow_kernel over column groups of 128, the one launch with blockIdx.y > 0)
    at ndata = 128 (exactly one group), 129 (one column in a second group) and 257 (three groups): 14 walkers x 4 rows = 56 rows, three
    and a half 16-row workgroups, K = ndata.  The stage call alone, against the oracle.marginal yardstick as test_every_call_at_every_shape
    compares its stage call; bars: hess_util.device_bar of synth_like_util.WIDE_FLOOR (measured on the host by test_draw_synthetic.py)."""
    from eftpipe_amd.marginal import MarginalLikelihood

    pb = SY.wide_problem(ndata)
    N, nG, ntr = pb.theta.shape[0], pb.nG, pb.ntr
    eng = _engine(pb, N * ntr)
    rows = pb.rec.rows(pb.theta, pb.f[pb.walker])
    _put(eng, pb, pb.walker)
    for jeff in (False, True):
        ref = SY.wide_reference(ndata, jeff)
        like = MarginalLikelihood(eng, pb.index, pb.D, pb.invcov, pb.loc, pb.scale, jeffreys=jeff)
        ls, fs, bs = like.logp(rows.reshape(N * ntr, nG + 1, 24), return_best=True)
        assert ls.shape == (N,) and np.all(np.isfinite(ls)) and np.all(np.isfinite(bs))
        _report("ndata %d%s" % (ndata, " jeffreys" if jeff else ""), "stage",
                SY.worst([SY.errors(pb, d, ref[d], None, ls[d], fs[d], bs[d], None, None, None, None, None) for d in range(N)]), SY.WIDE_FLOOR[ndata])
    eng.close()


@pytest.mark.parametrize("case", ["Ef", "Gf", "I"])
def test_failing_draw_between_regular_ones(case):
    """nG = 24 at four, two and one waves: one draw with an exactly zero row and column of F2 (test_draw_synthetic.py) in the middle of
    walker 0's nine is NaN throughout, and every other draw has the bits of the call without it; then F2 negative definite (the negated
    inverse covariance, nG even, flat prior): det F2 > 0, ln P finite, the samples NaN"""
    nG = SY.CASES[case]["nG"]
    pb = SY.case_problem(case, "flat", singular=nG // 2 + 1)
    N = pb.theta.shape[0]
    eng = _engine(pb, len(pb.counts) * pb.ntr)
    _put(eng, pb)
    z = SY.normals(N, SY.S5, nG)
    bad = 4
    keep = np.arange(N) != bad
    theta = pb.theta.copy()
    theta[bad, 0] = 0.0
    off = SY.offsets(pb.counts)
    for jeff in (False, True):
        hess = SY.CASES[case]["runs"]["hess_jeffreys" if jeff else "hess"]
        like = _like(eng, pb, jeff)
        got = _param_calls(like, theta, off, pb.f, z, hess)
        want = _param_calls(like, pb.theta[keep], SY.offsets([pb.counts[0] - 1] + pb.counts[1:]), pb.f, z[keep], hess)
        for k, a in got.items():
            assert k in ("full", "best") or np.all(np.isnan(a[bad])), k
            assert np.all(np.isfinite(a[keep])) and np.array_equal(a[keep], want[k]), k
        with pytest.raises(RuntimeError, match="det of F2ij"):
            like.logp_draws_params(theta, off, pb.f, grad=True)
        with pytest.raises(RuntimeError, match="det of F2ij"):
            like.sample_gaussian_params(theta, off, pb.f, z)
    # ---- the negated inverse covariance at the regular recipe
    pb = SY.case_problem(case, "flat")
    neg = _like(eng, pb, False, invcov=-pb.invcov)
    lp = neg.logp_draws_params(pb.theta, off, pb.f)
    raw = neg._sample_raw(pb.theta, off, pb.f, z)
    assert np.all(np.isfinite(lp)) and np.array_equal(raw.logp, lp) and np.all(np.isfinite(raw.best))
    assert np.all(np.isnan(raw.b)) and np.all(np.isnan(raw.chi2))
    with pytest.raises(RuntimeError, match="F2ij is not positive definite"):
        neg.sample_gaussian_params(pb.theta, off, pb.f, z)
    pos = _like(eng, pb, False)
    assert np.all(np.isfinite(pos.sample_gaussian_params(pb.theta, off, pb.f, z).b))
    eng.close()


def _raw_rows(like, rows, off, rows_nnlo):
    """eftb_draws_logp itself (the wrapper raises where ln P is NaN) -> logp, full, best"""
    from eftpipe_amd import _lib as L

    rows, off = np.ascontiguousarray(rows), np.ascontiguousarray(off, dtype=np.int64)
    rn = None if rows_nnlo is None else np.ascontiguousarray(rows_nnlo)
    N = rows.shape[0]
    logp, full, best = np.empty(N), np.empty(N), np.empty((N, like.nG))
    L.check(like.eng.lib.eftb_draws_logp(like.eng._h, off.size - 1, N, off.ctypes.data_as(C.POINTER(C.c_int64)), L.dptr(rows), L.dptr(rn), L.dptr(logp),
                                         L.dptr(full), L.dptr(best)))
    return dict(logp=logp, full=full, best=best)


@pytest.mark.parametrize("case", ["Ef", "Gf", "I"])
def test_every_wave_loops(case):
    """nG = 24 at four, two and one waves, every wave on several trips of its draw loop.  The launcher gives a walker's draws to at most
    2048 / C = 682 workgroups of at most four waves and strides a wave by workgroups x waves; walker 0 owns its nine theta tiled 607 times,
    5463 > 2 x 682 x 4 draws, so every wave of the rows, params, gradient, Hessian and sample kernels takes at least two draws (eight and
    more at one wave).  Draw 4 of the nine is the singular one (an exactly zero pivot): the stride is 682 nw = 7, 5, 1 mod 9, so the waves
    meet failing draws between regular ones, in the same buffers.  Every copy must have the bits of the nine-draw call: NaN where that
    call is NaN, and nothing of a failed draw, or of any earlier draw, left in the next one."""
    nG = SY.CASES[case]["nG"]
    pb = SY.case_problem(case, "flat", singular=nG // 2 + 1)
    eng = _engine(pb, len(pb.counts) * pb.ntr)
    _put(eng, pb)
    counts = SY.long_counts()
    n0, tile = pb.counts[0], -(-counts[0] // pb.counts[0])
    assert counts[0] > 2 * 4 * (2048 // len(counts)) and tile * n0 >= counts[0]
    counts[0] = tile * n0
    theta9 = pb.theta.copy()
    theta9[4, 0] = 0.0
    pick = np.concatenate([np.tile(np.arange(n0), tile), np.arange(n0, len(theta9))])  # draw of the short call behind each draw of the long one
    z9 = SY.normals(len(theta9), SY.S5, nG)
    off9, off = SY.offsets(pb.counts), SY.offsets(counts)
    fd = pb.f[pb.walker]
    rows9, rn9 = pb.rec.rows(theta9, fd), pb.rec.rows_nnlo(theta9, fd) if pb.nnlo else None
    for jeff in (False, True):
        hess = SY.CASES[case]["runs"]["hess_jeffreys" if jeff else "hess"]
        like = _like(eng, pb, jeff)
        short = _param_calls(like, theta9, off9, pb.f, z9, hess)
        short_rows = _raw_rows(like, rows9, off9, rn9)
        bad = np.isnan(short["logp"])
        assert np.array_equal(np.nonzero(bad)[0], [4]) and np.all(np.isnan(short["grad"][4])) and np.all(np.isnan(short["b"][4]))
        assert all(np.all(np.isfinite(a[~bad])) for a in short.values()) and np.array_equal(np.isnan(short_rows["logp"]), bad)
        long = _param_calls(like, theta9[pick], off, pb.f, z9[pick], hess)
        for k, a in long.items():
            assert np.array_equal(a, short[k][pick], equal_nan=True), (jeff, k)
        long_rows = _raw_rows(like, rows9[pick], off, None if rn9 is None else rn9[pick])
        for k, a in long_rows.items():
            assert np.array_equal(a, short_rows[k][pick], equal_nan=True), (jeff, "rows", k)
    eng.close()


@pytest.mark.parametrize("case", ["C", "I"])
def test_groups_at_other_shapes(case):
    """groups= with two data sets and groups that repeat a walker: a group on data set 0 returns the bits of the call without groups, a
    group on data set 1 matches the yardstick evaluated with that data vector"""
    pb = SY.case_problem(case)
    nG = pb.nG
    eng = _engine(pb, len(pb.counts) * pb.ntr)
    _put(eng, pb)
    Ds = datasets(pb.D, pb.invcov, 2)
    off0 = SY.offsets(pb.counts)
    w0, w2 = np.arange(off0[0], off0[1]), np.arange(off0[2], off0[3])
    groups = [(2, 1), (0, 0), (0, 1), (2, 0)]
    members = [w2, w0, w0[:3], w2]  # the draws of the case each group repeats
    src = np.concatenate(members)
    gof = np.repeat(np.arange(4), [len(m) for m in members])
    off = SY.offsets([len(m) for m in members])
    wk, ds = np.array([g[0] for g in groups]), np.array([g[1] for g in groups])
    theta = pb.theta[src]
    z = SY.normals(theta.shape[0], SY.S5, nG, seed=29)
    floors = SY.SYNTH_FLOOR[case]["gauss"]
    for jeff in (False, True):
        hess = SY.CASES[case]["runs"]["hess_jeffreys" if jeff else "hess"]
        like = _like(eng, pb, jeff)
        like.set_datasets(Ds)
        got = _param_calls(like, theta, off, pb.f, z, hess, groups=(wk, ds))
        assert all(np.all(np.isfinite(a)) for a in got.values())
        own = np.isin(gof, [1, 3])  # groups (0, 0) and (2, 0), in walker order: the call without groups
        plain = _param_calls(like, theta[own], off0, pb.f, z[own], hess)
        for k, a in plain.items():
            assert np.array_equal(a, got[k][own]), k
        errs = []
        for q in np.nonzero(~own)[0]:
            y = SY.yardstick(pb, src[q], z[q], jeff, D=Ds[1], hess=hess)
            errs.append(SY.errors(pb, src[q], y, z[q], got["logp"][q], got["full"][q], got["best"][q], got["grad"][q], got["hess"][q] if hess else None,
                                  got["b"][q], got["chi2"][q], None))
        _report("%s groups%s" % (case, " jeffreys" if jeff else ""), "data set 1", SY.worst(errs), floors)
    eng.close()


def test_five_tracers_with_nnlo_are_refused():
    """J + 1 = 136 columns: every draw call refuses, and names the limit"""
    from eftpipe_amd import _lib as L

    assert not any(SY.TOO_WIDE["runs"][k] for k in SY.CALLS if k != "stage")
    pb = SY.problem(seed=77, **SY.shape_of(SY.TOO_WIDE))
    N, P = pb.theta.shape
    eng = _engine(pb, len(pb.counts) * pb.ntr)
    _put(eng, pb)
    like = _like(eng, pb, False)
    off, fd = SY.offsets(pb.counts), pb.f[pb.walker]
    z = SY.normals(N, 2, pb.nG)
    calls = dict(rows=lambda: like.logp_draws(pb.rec.rows(pb.theta, fd), off, rows_nnlo=pb.rec.rows_nnlo(pb.theta, fd)),
                 params=lambda: like.logp_draws_params(pb.theta, off, pb.f),
                 grad=lambda: like.logp_draws_params(pb.theta, off, pb.f, grad=True),
                 hess=lambda: like.logp_draws_params(pb.theta, off, pb.f, grad=True, hess=True),
                 sample=lambda: like.sample_gaussian_params(pb.theta, off, pb.f, z),
                 chain=lambda: like.metropolis_draws_params(pb.theta, off, pb.f, np.zeros((N, 2, P)), np.full((N, 2), -1.0)))
    for name, call in calls.items():
        with pytest.raises(L.EftbError, match="135 template columns per walker, at most 127"):
            call()
    eng.close()


def _padded_recipe(rec, entries):
    """rec with single-term entries added at free (tracer, row, column) slots until it has `entries` of them"""
    from eftpipe_amd.parambasis import DrawRecipe

    have = set(zip(rec.tracer.tolist(), rec.row.tolist(), rec.col.tolist()))
    free = [(t, g, c) for g in range(1, rec.ng1) for t in range(rec.ntr) for c in range(24) if (t, g, c) not in have][: entries - len(have)]
    assert len(have) + len(free) == entries
    cat = lambda a, extra: np.concatenate([a, np.asarray(extra, dtype=a.dtype).reshape((-1,) + a.shape[1:])])
    n = len(free)
    out = DrawRecipe(rec.param_names, rec.ntr, rec.ng1, cat(rec.tracer, [s[0] for s in free]), cat(rec.row, [s[1] for s in free]), cat(rec.col, [s[2] for s in free]),
                     cat(rec.coef, [1e-3 * (1 + q % 7) for q in range(n)]), cat(rec.fpow, [q % 7 for q in range(n)]), cat(rec.idx, [[q % len(rec.param_names), -1, -1] for q in range(n)]))
    assert len(set(zip(out.tracer.tolist(), out.row.tolist(), out.col.tolist()))) == entries and out.nterms <= 1024
    return out


def test_sample_call_lds_refusal():
    """The one LDS refusal of draws_logp_shape's callers that can be reached: the sample call at five tracers and nG = 24 with a recipe of
    at least 1001 entries (147816 + 16 nnzp bytes at one wave, nnzp the entry count rounded up to even, against 163840).  1000 entries run,
    1001 are refused with the call's own message while the params, gradient and chain calls still run; the engine then serves the case's
    ordinary recipe with the bits it returned before."""
    from eftpipe_amd import _lib as L

    pb = SY.case_problem("I")
    N, P = pb.theta.shape
    eng = _engine(pb, len(pb.counts) * pb.ntr)
    _put(eng, pb)
    off = SY.offsets(pb.counts)
    z = SY.normals(N, SY.S5, pb.nG)
    like = _like(eng, pb, False)
    before = like.sample_gaussian_params(pb.theta, off, pb.f, z)
    like = _like(eng, pb, False, rec=_padded_recipe(pb.rec, 1000))
    r = like.sample_gaussian_params(pb.theta, off, pb.f, z)
    want = like.logp_draws_params(pb.theta, off, pb.f, return_best=True)
    assert all(np.array_equal(a, b) for a, b in zip((r.logp, r.fullchi2, r.best), want)) and np.all(np.isfinite(r.b))
    assert not np.array_equal(r.logp, before.logp)  # the added entries count
    like = _like(eng, pb, False, rec=_padded_recipe(pb.rec, 1001))
    with pytest.raises(L.EftbError, match="eftb_draws_sample_params: the samples of nG = 24 parameters with J \\+ 1 = 121 columns do not fit the LDS"):
        like.sample_gaussian_params(pb.theta, off, pb.f, z)
    lp, full, best = like.logp_draws_params(pb.theta, off, pb.f, return_best=True)
    lg, _, fg, bg = like.logp_draws_params(pb.theta, off, pb.f, grad=True, return_best=True)
    assert np.all(np.isfinite(lp)) and np.array_equal(lg, lp) and np.array_equal(fg, full) and np.array_equal(bg, best)
    ch = like.metropolis_draws_params(pb.theta, off, pb.f, np.zeros((N, 1, P)), np.full((N, 1), -1.0))
    assert np.array_equal(ch.logp[:, 0], lp)
    like = _like(eng, pb, False, rec=_padded_recipe(pb.rec, 1024))  # the longest recipe there is: the same answers
    with pytest.raises(L.EftbError, match="the samples of nG = 24 parameters"):
        like.sample_gaussian_params(pb.theta, off, pb.f, z)
    assert np.all(np.isfinite(like.logp_draws_params(pb.theta, off, pb.f, grad=True)[1]))
    assert np.all(np.isfinite(like.metropolis_draws_params(pb.theta, off, pb.f, np.zeros((N, 1, P)), np.full((N, 1), -1.0)).logp))
    like = _like(eng, pb, False)
    after = like.sample_gaussian_params(pb.theta, off, pb.f, z)
    for a, b in zip(after[:5], before[:5]):
        assert np.array_equal(a, b)
    eng.close()
