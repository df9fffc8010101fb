"""Metropolis chains over the draw parameters on the device (eftb_draws_chain_params; MarginalLikelihood.metropolis_draws_params).
Yardstick: the project's own synchronous route -- a host loop that forms every proposal in NumPy, asks eftb_draws_logp_params for its
record and applies chain_util.host_chain's acceptance rule (pinned to the mathematics by test_draw_chains.py).  Everything is compared bit
for bit: the states, ln P, full chi2, the best fits, the last state and the accept counts.  The inputs are those test_draw_chains.py has
checked to move and to be refused on every chain; the replayed chains are asked again."""
import ctypes as C

import numpy as np
import pytest

import chain_util as CU
from test_draw_chains import T37, THIN, chain_case, long_inputs
from test_draw_datasets import datasets
from test_gpu_draws import _marg, _offsets
from test_gpu_draws_grad import _nnlo_problem
from test_gpu_draws_params import _cfg3_engine, _marg_case

pytestmark = pytest.mark.gpu

FIELDS = ("theta", "logp", "fullchi2", "best", "last", "naccept")


def _records(like, off, f, groups=None):
    """theta [N, P] -> (ln P, full chi2, best) of eftb_draws_logp_params (eftb_draws_logp_params_datasets), NaN where det F2 <= 0"""
    from eftpipe_amd import _lib as L
    from eftpipe_amd.engine import _params_args
    from eftpipe_amd.marginal import _groups_args

    eng = like.eng

    def fun(theta):
        if groups is not None:
            th, o, ff, wk, ds = _groups_args(like._recipe, theta, off, f, eng.ntracers, groups)
            logp, _, _, full, best = like._draws_groups_raw(th, o, ff, wk, ds, grad=False, hess=False)
            return logp, full, best
        th, o, ff = _params_args(like._recipe, theta, off, f, eng.ntracers)
        N = th.shape[0]
        logp, full, best = np.empty(N), np.empty(N), np.empty((N, like.nG))
        L.check(eng.lib.eftb_draws_logp_params(eng._h, o.size - 1, N, o.ctypes.data_as(C.POINTER(C.c_int64)), L.dptr(th), L.dptr(ff), L.dptr(logp),
                                               L.dptr(full), L.dptr(best)))
        return logp, full, best

    return fun


def _same(got, want):
    """a DrawChains of the device against host_chain's dict around the device's records"""
    for name, a, b in zip(FIELDS, (got.theta, got.logp, got.fullchi2, got.best, got.last, got.naccept),
                          (want["theta"], want["logp"], want["extras"][0], want["extras"][1], want["last"], want["naccept"])):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), name


def _compare(like, off, f, inp, thin, groups=None, raw=False, **prior):
    """the device call against the host loop -> (DrawChains, host_chain's dict)"""
    box = {k: inp[k] for k in ("lower", "upper") if k in inp}
    want = CU.host_chain(_records(like, off, f, groups), inp["theta0"], inp["step"], inp["lnu"], thin, box.get("lower"), box.get("upper"),
                         prior.get("prior_loc"), prior.get("prior_scale"))
    call = like._chains_raw if raw else like.metropolis_draws_params
    got = call(inp["theta0"], off, f, inp["step"], inp["lnu"], thin=thin, groups=groups, return_best=True, **box, **prior)
    _same(got, want)
    return got, want


def _stored_records_are_the_draw_call(like, off, f, got, groups=None):
    fun = _records(like, off, f, groups)
    for k in range(got.theta.shape[1]):
        for a, b in zip(fun(got.theta[:, k]), (got.logp[:, k], got.fullchi2[:, k], got.best[:, k])):
            assert np.array_equal(a, b)


def _engine(golden, tag, case):
    """the engine of a case of test_draw_chains.chain_case with its templates put -> eng"""
    if tag in ("auto", "cross"):
        _, eng, _, index = _marg(golden, tag)
        eng.put("TEMPL", case["templ"])
    elif tag == "full":
        eng, templ, index = _cfg3_engine(golden("cfg3"), len(case["counts"]), 3 * len(case["counts"]))
        assert np.array_equal(templ, case["templ"])
    else:
        eng, _, theta, f, counts, T, TN, index, D, Ci, _ = _nnlo_problem()
        assert np.array_equal(T, case["templ"]) and np.array_equal(TN, case["templn"]) and np.array_equal(D, case["D"]) and np.array_equal(f, case["f"])
    assert np.array_equal(index, case["index"])
    return eng


def _like(eng, case, i):
    from eftpipe_amd.marginal import MarginalLikelihood

    loc, scale, jeff = case["priors"][i]
    like = MarginalLikelihood(eng, case["index"], case["D"], case["Ci"], loc, scale, jeffreys=jeff)
    like.set_draw_recipe(case["rec"])
    return like


@pytest.mark.parametrize("tag", ["auto", "cross", "full", "nnlo"])
def test_chains_are_the_host_loop_bit_for_bit(golden, tag):
    """T = 37, thin = 5, a box that refuses proposals, walkers with their own templates (one without a chain), under every prior of the case"""
    case = chain_case(tag)
    eng = _engine(golden, tag, case)
    inp, off, f = case["inp"], _offsets(case["counts"]), case["f"]
    N, P, nG = inp["theta0"].shape[0], inp["theta0"].shape[1], case["rec"].ng1 - 1
    for i in range(len(case["priors"])):
        like = _like(eng, case, i)
        before = like.logp_draws_params(inp["theta0"], off, f, return_best=True)
        got, want = _compare(like, off, f, inp, THIN)
        K = T37 // THIN
        assert got.theta.shape == (N, K, P) and got.logp.shape == (N, K) and got.best.shape == (N, K, nG) and got.naccept.dtype == np.int64
        print(tag, i, "naccept", got.naccept, "outside the box", want["outside"])
        assert np.all(got.naccept > 0) and np.all(got.naccept < T37) and np.all(want["outside"] > 0)
        assert np.all(np.isfinite(got.theta)) and np.all(np.isfinite(got.logp))
        _stored_records_are_the_draw_call(like, off, f, got)
        for a, b in zip(before, like.logp_draws_params(inp["theta0"], off, f, return_best=True)):  # the Gram cache and the records are not disturbed
            assert np.array_equal(a, b)
        if i:
            continue
        # thin = 1: the thinned chain is a subsequence, `last` and the accept counts are the same
        full, _ = _compare(like, off, f, inp, 1)
        assert np.array_equal(full.theta[:, THIN - 1 :: THIN][:, :K], got.theta) and np.array_equal(full.logp[:, THIN - 1 :: THIN][:, :K], got.logp)
        assert np.array_equal(full.last, got.last) and np.array_equal(full.naccept, got.naccept) and np.array_equal(full.last, full.theta[:, -1])
        # without return_best the same chain, and no records
        lean = like.metropolis_draws_params(inp["theta0"], off, f, inp["step"], inp["lnu"], thin=THIN, lower=inp["lower"], upper=inp["upper"])
        assert lean.fullchi2 is None and lean.best is None and np.array_equal(lean.theta, got.theta) and np.array_equal(lean.logp, got.logp)
    eng.close()


def test_long_chain_crosses_the_launch_boundary(golden):
    """T = 300 > 256: two launches.  The call equals the host loop, and a 100-step call followed by a 200-step call from `last`"""
    case, inp = long_inputs()
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    off, f = _offsets([3, 0, 0, 0]), case["f"]
    got, want = _compare(like, off, f, inp, 7)
    one, want = _compare(like, off, f, inp, 1)
    assert np.all(one.naccept > 0) and np.all(one.naccept < 300) and np.all(want["outside"] > 0) and np.array_equal(got.naccept, one.naccept)
    assert np.array_equal(got.theta, one.theta[:, 6::7]) and np.array_equal(got.last, one.last)
    cut = lambda a, b: dict(inp, step=np.ascontiguousarray(inp["step"][:, a:b]), lnu=np.ascontiguousarray(inp["lnu"][:, a:b]))
    first, _ = _compare(like, off, f, cut(0, 100), 1)
    second, _ = _compare(like, off, f, dict(cut(100, 300), theta0=first.last), 1)
    for name in ("theta", "logp", "fullchi2", "best"):
        assert np.array_equal(np.concatenate([getattr(first, name), getattr(second, name)], axis=1), getattr(one, name)), name
    assert np.array_equal(second.last, one.last) and np.array_equal(first.naccept + second.naccept, one.naccept)
    _stored_records_are_the_draw_call(like, off, f, got)
    eng.close()


def test_a_launch_that_stores_nothing_before_one_that_does(golden):
    """T = 300, thin = 299: the launch of steps 1 ... 256 stores no state and brings nothing back, the second stores the one state there is.
    The state, its record, `last` and the accept counts are the host loop's."""
    case, inp = long_inputs()
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    got, _ = _compare(like, _offsets([3, 0, 0, 0]), case["f"], inp, 299)
    assert got.theta.shape == (3, 1, inp["theta0"].shape[1]) and np.all(got.naccept > 0)
    eng.close()


def test_split_batches_and_theta_priors(golden):
    case = chain_case("auto")
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    inp, counts, f = case["inp"], np.array(case["counts"]), case["f"]
    off = _offsets(counts)
    whole, _ = _compare(like, off, f, inp, THIN)
    # a batch split over two calls with other offsets: the same bits per chain
    cutc = np.array([1, 0, 2, 0])
    sel_a = np.concatenate([np.arange(off[c], off[c] + cutc[c]) for c in range(4)])
    sel_b = np.concatenate([np.arange(off[c] + cutc[c], off[c + 1]) for c in range(4)])
    for sel, cnt in ((sel_a, cutc), (sel_b, counts - cutc)):
        part, _ = _compare(like, _offsets(cnt), f, dict(inp, theta0=inp["theta0"][sel], step=inp["step"][sel], lnu=inp["lnu"][sel]), THIN)
        for name in FIELDS:
            assert np.array_equal(getattr(part, name), getattr(whole, name)[sel]), name
    none = like.metropolis_draws_params(np.zeros((0, 3)), [0, 0, 0, 0, 0], f, np.zeros((0, 4, 3)), np.zeros((0, 4)), thin=2, return_best=True)
    assert none.theta.shape == (0, 2, 3) and none.naccept.shape == (0,) and none.best.shape == (0, 2, like.nG)
    # no bounds and no priors on theta: the call with infinite ones
    free = {k: v for k, v in inp.items() if k not in ("lower", "upper")}
    a, _ = _compare(like, off, f, free, THIN)
    inf = np.full(3, np.inf)
    b, _ = _compare(like, off, f, dict(free, lower=-inf, upper=inf), THIN, prior_loc=np.array([1.0, 2.0, 3.0]), prior_scale=inf)
    for name in FIELDS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert not np.array_equal(a.theta, whole.theta)  # (the box had refused proposals)
    # Gaussian priors on theta, on all parameters and on one: the chain changes as the host loop says
    mid, wid = 0.5 * (inp["lower"] + inp["upper"]), 0.1 * (inp["upper"] - inp["lower"])
    for scale in (wid, np.array([np.inf, wid[1], np.inf])):
        c, want = _compare(like, off, f, inp, THIN, prior_loc=mid, prior_scale=scale)
        assert not np.array_equal(c.theta, whole.theta) and np.all(want["naccept"] > 0)
    c, _ = _compare(like, off, f, free, THIN, prior_loc=mid, prior_scale=wid)
    assert not np.array_equal(c.theta, a.theta)
    eng.close()


def test_groups_chain_against_their_own_data(golden):
    """groups= after set_datasets (M = 3) against the host loop through logp_draws_params(groups=); the groups of data set 0 are the call
    without groups bit for bit"""
    case = chain_case("auto")
    eng = _engine(golden, "auto", case)
    inp, f = case["inp"], case["f"]
    groups = [(3, 2), (0, 0), (2, 0), (0, 1), (2, 1)]
    counts = [2, 2, 1, 0, 3]
    wk, ds = np.array([w for w, _ in groups]), np.array([m for _, m in groups])
    off = _offsets(counts)
    Ds = datasets(case["D"], case["Ci"], 3)
    assert np.array_equal(Ds[0], case["D"])
    for i in (0, 1):
        like = _like(eng, case, i)
        like.set_datasets(Ds)
        got, want = _compare(like, off, f, inp, THIN, groups=(wk, ds))
        print("groups", i, "naccept", got.naccept, "outside the box", want["outside"])
        assert np.all(got.naccept > 0) and np.all(got.naccept < T37)
        _stored_records_are_the_draw_call(like, off, f, got, groups=(wk, ds))
        own = sorted((q for q, (w, m) in enumerate(groups) if m == 0), key=lambda q: groups[q][0])
        sel = np.concatenate([np.arange(off[q], off[q + 1]) for q in own])
        cnt = np.zeros(4, dtype=int)
        for q in own:
            cnt[groups[q][0]] = counts[q]
        plain, _ = _compare(like, _offsets(cnt), f, dict(inp, theta0=inp["theta0"][sel], step=inp["step"][sel], lnu=inp["lnu"][sel]), THIN)
        for name in FIELDS:
            assert np.array_equal(getattr(plain, name), getattr(got, name)[sel]), name
    eng.close()


def test_failed_starts_nan_proposals_and_refusals(golden):
    from eftpipe_amd import _lib as L
    from eftpipe_amd.marginal import MarginalLikelihood
    from eftpipe_amd.parambasis import DrawRecipe

    g, eng, T, index = _marg(golden, "auto", max_batch=4)
    rec, theta, _, _, f = _marg_case(g, "auto", [2, 2])
    D, Ci = g["auto_D"], g["auto_invcov"]
    nG = len(g["auto_loc"])
    eng.put("TEMPL", np.stack([T, T]))
    off = [0, 2, 4]
    N, P, Tn = 4, 3, 9
    rng = np.random.default_rng(6)
    step, lnu = rng.standard_normal((N, Tn, P)) * [0.02, 0.1, 0.1], np.log(rng.random((N, Tn)))
    # ---- det F2 <= 0 where theta_2 = 0: Gaussian row 3 times theta_2 under a flat prior (test_gpu_draws_hess.py)
    flat = MarginalLikelihood(eng, index, D, Ci, np.zeros(nG), np.full(nG, np.inf))
    idx3 = rec.idx.copy()
    idx3[rec.row == 3, 2] = 2
    flat.set_draw_recipe(DrawRecipe(rec.param_names, 1, nG + 1, rec.tracer, rec.row, rec.col, rec.coef, rec.fpow, idx3))
    th0 = theta.copy()
    th0[1, 2] = 0.0  # chain 1 starts on the singular plane
    step[0, 0] = [0.0, 0.0, -th0[0, 2]]  # chain 0 is sent there by its first proposal, with lnu = -inf: any finite ln P would be accepted
    lnu[0, 0] = -np.inf
    inp = dict(theta0=th0, step=step, lnu=lnu)
    with pytest.raises(RuntimeError, match="det of F2ij"):
        flat.metropolis_draws_params(th0, off, f, step, lnu)
    raw, want = _compare(flat, off, f, inp, 2, raw=True)
    assert raw.naccept[1] == -1 and all(np.all(np.isnan(a[1])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last))
    ok = [0, 2, 3]
    assert all(np.all(np.isfinite(a[ok])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last)) and np.all(raw.naccept[ok] > 0)
    one, _ = _compare(flat, off, f, inp, 1, raw=True)
    assert np.array_equal(one.theta[0, 0], th0[0]) and np.any(one.theta[0] != th0[0])  # the NaN proposal was rejected and the chain went on
    # ---- refusals
    like = MarginalLikelihood(eng, index, D, Ci, g["auto_loc"], g["auto_scale"])
    with pytest.raises(L.EftbError, match="eftb_draws_chain_params: no draw recipe"):
        like.metropolis_draws_params(theta, off, f, step, lnu)
    like.set_draw_recipe(rec)
    want = like.metropolis_draws_params(theta, off, f, step, lnu)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    th, fo, o64 = np.ascontiguousarray(theta), np.ascontiguousarray(f), np.asarray(off, dtype=np.int64)
    out = [np.zeros((N, Tn, P)), np.zeros((N, Tn)), np.zeros((N, Tn)), np.zeros((N, Tn, nG)), np.zeros((N, P))]
    nacc = np.zeros(N, dtype=np.int64)

    def call(Tc, thin, st=step, lu=lnu, pri=(None, None, None, None)):
        rc = eng.lib.eftb_draws_chain_params(eng._h, 2, N, Tc, thin, i64(o64), dp(th), dp(fo), dp(st), dp(lu), *[dp(a) for a in pri], *[dp(a) for a in out], i64(nacc))
        return rc, eng.lib.eftb_last_error().decode()

    for Tc, thin, msg in ((0, 1, "T = 0 steps"), (Tn, 0, "thin = 0 outside"), (Tn, Tn + 1, "thin = 10 outside")):
        rc, err = call(Tc, thin)
        assert rc != 0 and msg in err, err
    assert call(Tn, 1)[0] == 0 and np.array_equal(out[0], want.theta) and np.array_equal(out[4], want.last) and np.array_equal(nacc, want.naccept)
    for v in (np.nan, np.inf):
        bad = step.copy()
        bad[2, 5, 1] = v
        with pytest.raises(L.EftbError, match="step\\[2\\]\\[5\\]\\[1\\] is not finite"):
            like.metropolis_draws_params(theta, off, f, bad, lnu)
    for v in (np.nan, 1e-3):
        bad = lnu.copy()
        bad[3, 4] = v
        with pytest.raises(L.EftbError, match="lnu\\[3\\]\\[4\\]"):
            like.metropolis_draws_params(theta, off, f, step, bad)
    lo, hi = theta.min(0) - 1.0, theta.max(0) + 1.0
    with pytest.raises(L.EftbError, match="lower\\[1\\] = .* > upper\\[1\\]"):
        like.metropolis_draws_params(theta, off, f, step, lnu, lower=[lo[0], hi[1], lo[2]], upper=[hi[0], lo[1], hi[2]])
    with pytest.raises(L.EftbError, match="a bound of parameter 2 is NaN"):
        like.metropolis_draws_params(theta, off, f, step, lnu, lower=[lo[0], lo[1], np.nan])
    for v in (0.0, -1.0, np.nan):
        with pytest.raises(L.EftbError, match="prior_scale\\[0\\]"):
            like.metropolis_draws_params(theta, off, f, step, lnu, prior_scale=[v, 1.0, 1.0])
    j = int(np.argmin(theta[:, 1]))  # the one chain below a bound just above it
    with pytest.raises(L.EftbError, match="theta0\\[%d\\]\\[1\\] = .* outside" % j):
        like.metropolis_draws_params(theta, off, f, step, lnu, lower=[lo[0], np.nextafter(theta[j, 1], np.inf), lo[2]])
    bad = theta.copy()
    bad[1, 2] = np.inf
    with pytest.raises(L.EftbError, match="theta\\[1\\]\\[2\\] is not finite"):
        like.metropolis_draws_params(bad, off, f, step, lnu)
    with pytest.raises(L.EftbError, match="offsets"):
        like.metropolis_draws_params(theta, [0, 2, 5], f, step, lnu)
    with pytest.raises(L.EftbError, match="eftb_draws_chain_params_datasets: no data sets"):
        like.metropolis_draws_params(theta, off, f, step, lnu, groups=([0, 1], [0, 0]))
    assert np.array_equal(like.metropolis_draws_params(theta, off, f, step, lnu).theta, want.theta)
    eng.set_tracers(1)  # drops the recipe (and the likelihood)
    with pytest.raises(L.EftbError, match="eftb_set_likelihood"):
        like.metropolis_draws_params(theta, off, f, step, lnu)
    like = MarginalLikelihood(eng, index, D, Ci, g["auto_loc"], g["auto_scale"])
    with pytest.raises(L.EftbError, match="no draw recipe"):
        like.metropolis_draws_params(theta, off, f, step, lnu)
    like.set_draw_recipe(rec)
    assert np.array_equal(like.metropolis_draws_params(theta, off, f, step, lnu).theta, want.theta)
    eng.close()
