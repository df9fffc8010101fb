"""Hamiltonian Monte Carlo over the draw parameters on the device (eftb_draws_hmc_params; MarginalLikelihood.hmc_draws_params).
Yardstick: the project's own synchronous route -- hmc_util.host_hmc (pinned to the mathematics by test_draw_hmc.py) around
eftb_draws_logp_grad_params, what logp_draws_params(..., grad=True, return_best=True) returns, one call per leapfrog step.  Everything is
compared bit for bit: the states, ln P, full chi2, the best fits, the last state, the accept counts and the ratios.  The inputs are those
test_draw_hmc.py has checked to move, to be refused and to leave the box; the device's chains are asked again."""
import ctypes as C

import numpy as np
import pytest

import hmc_util as HM
import synth_like_util as SY
from test_draw_datasets import datasets
from test_draw_hmc import HMC_WAVES, NLEAP, T11, THIN, hmc_case, hmc_shape, hmc_waves, mixed
from test_gpu_draw_chains import _engine, _like, _records
from test_gpu_draws import _marg, _offsets
from test_gpu_draws_params import _marg_case

pytestmark = pytest.mark.gpu

FIELDS = ("theta", "logp", "fullchi2", "best", "last", "naccept", "log_ratio")


def _grad_records(like, off, f, groups=None):
    """theta [N, P] -> (ln P, grad, full chi2, best) of eftb_draws_logp_grad_params (eftb_draws_logp_params_datasets): the arrays of
    logp_draws_params(theta, off, f, grad=True, return_best=True, groups=groups) without its RuntimeError, NaN where det F2 <= 0"""
    from eftpipe_amd import _lib as L
    from eftpipe_amd.engine import _params_args
    from eftpipe_amd.marginal import _groups_args

    eng = like.eng

    def fun(theta):
        if groups is not None:
            th, o, ff, wk, ds = _groups_args(like._recipe, theta, off, f, eng.ntracers, groups)
            logp, grad, _, full, best = like._draws_groups_raw(th, o, ff, wk, ds, grad=True, hess=False)
            return logp, grad, full, best
        th, o, ff = _params_args(like._recipe, theta, off, f, eng.ntracers)
        N, P = th.shape
        logp, grad, full, best = np.empty(N), np.empty((N, P)), np.empty(N), np.empty((N, like.nG))
        L.check(eng.lib.eftb_draws_logp_grad_params(eng._h, o.size - 1, N, o.ctypes.data_as(C.POINTER(C.c_int64)), L.dptr(th), L.dptr(ff), L.dptr(logp),
                                                    L.dptr(grad), L.dptr(full), L.dptr(best)))
        return logp, grad, full, best

    return fun


def _same(got, want):
    """a DrawTrajectories of the device against host_hmc's dict around the device's records and gradients"""
    for name, a, b in zip(FIELDS, (got.theta, got.logp, got.fullchi2, got.best, got.last, got.naccept, got.log_ratio),
                          (want["theta"], want["logp"], want["extras"][0], want["extras"][1], want["last"], want["naccept"], want["log_ratio"])):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), name


def _compare(like, off, f, inp, eps, nleap, factor, thin, groups=None, raw=False):
    """the device call against the host loop -> (DrawTrajectories, host_hmc's dict); inp: theta0, mom, lnu and, where given, lower, upper,
    prior_loc, prior_scale"""
    opt = {k: inp[k] for k in ("lower", "upper", "prior_loc", "prior_scale") if k in inp}
    want = HM.host_hmc(_grad_records(like, off, f, groups), inp["theta0"], inp["mom"], inp["lnu"], eps, nleap, factor, thin, opt.get("lower"), opt.get("upper"),
                       opt.get("prior_loc"), opt.get("prior_scale"))
    call = like._hmc_raw if raw else like.hmc_draws_params
    got = call(inp["theta0"], off, f, inp["mom"], inp["lnu"], eps, nleap, factor=factor, thin=thin, groups=groups, return_best=True, return_ratio=True, **opt)
    _same(got, want)
    return got, want


def _stored_records_are_the_draw_call(like, off, f, got, groups=None):
    fun = _records(like, off, f, groups)
    for k in range(got.theta.shape[1]):
        for a, b in zip(fun(got.theta[:, k]), (got.logp[:, k], got.fullchi2[:, k], got.best[:, k])):
            assert np.array_equal(a, b)


def _inputs(hc, sel=slice(None)):
    return dict({k: hc[k][sel] for k in ("theta0", "mom", "lnu")}, **{k: hc[k] for k in ("lower", "upper", "prior_loc", "prior_scale")})


@pytest.mark.parametrize("tag", ["auto", "cross", "full", "nnlo"])
def test_trajectories_are_the_host_loop_bit_for_bit(golden, tag):
    """T = 11, nleap = 4, thin = 3, a box that trajectories leave and a Gaussian prior on the bounded parameter, walkers with their own
    templates (one without a chain), under every prior of the case, with a factor and without"""
    hc = hmc_case(tag)
    case = hc["case"]
    eng = _engine(golden, tag, case)
    inp, off, f = _inputs(hc), _offsets(case["counts"]), case["f"]
    N, P, nG = inp["theta0"].shape[0], inp["theta0"].shape[1], case["rec"].ng1 - 1
    K = T11 // THIN
    for i in range(len(case["priors"])):
        like = _like(eng, case, i)
        before = like.logp_draws_params(inp["theta0"], off, f, return_best=True)
        step, lnu = 0.01 * inp["mom"], inp["lnu"]
        walk = like.metropolis_draws_params(inp["theta0"], off, f, step, lnu, return_best=True)
        for name, F, eps in hc["variants"]:
            got, want = _compare(like, off, f, inp, eps, NLEAP, F, THIN)
            assert got.theta.shape == (N, K, P) and got.logp.shape == (N, K) and got.best.shape == (N, K, nG) and got.log_ratio.shape == (N, T11)
            assert got.naccept.dtype == np.int64
            print(tag, i, name, "naccept", got.naccept, "outside", want["outside"], "aborted", want["aborted"], "refused", want["refused"])
            assert mixed(want, T11)  # every chain moved and was refused; the box was met; a trajectory was refused inside it
            assert np.all(np.isfinite(got.theta)) and np.all(np.isfinite(got.logp))
            assert np.array_equal(np.isnan(got.log_ratio).sum(1), want["aborted"])
            _stored_records_are_the_draw_call(like, off, f, got)
            if i == 0 and name == "factor":
                # thin = 1: the thinned trajectory is a subsequence, `last`, the accept counts and the ratios are the same
                full, _ = _compare(like, off, f, inp, eps, NLEAP, F, 1)
                assert np.array_equal(full.theta[:, THIN - 1 :: THIN][:, :K], got.theta) and np.array_equal(full.logp[:, THIN - 1 :: THIN][:, :K], got.logp)
                assert np.array_equal(full.last, got.last) and np.array_equal(full.naccept, got.naccept) and np.array_equal(full.last, full.theta[:, -1])
                assert np.array_equal(full.log_ratio, got.log_ratio, equal_nan=True)
                # without return_best and return_ratio the same chain, and neither
                opt = {k: inp[k] for k in ("lower", "upper", "prior_loc", "prior_scale")}
                lean = like.hmc_draws_params(inp["theta0"], off, f, inp["mom"], inp["lnu"], eps, NLEAP, factor=F, thin=THIN, **opt)
                assert lean.fullchi2 is None and lean.best is None and lean.log_ratio is None
                assert np.array_equal(lean.theta, got.theta) and np.array_equal(lean.logp, got.logp) and np.array_equal(lean.naccept, got.naccept)
        # the Gram cache, the records and the chain call's buffers are not disturbed
        for a, b in zip(before, like.logp_draws_params(inp["theta0"], off, f, return_best=True)):
            assert np.array_equal(a, b)
        again = like.metropolis_draws_params(inp["theta0"], off, f, step, lnu, return_best=True)
        for a, b in zip(walk, again):
            assert np.array_equal(a, b)
    eng.close()


def test_launch_boundaries(golden):
    """nleap = 4 and T = 70: launches of 64 trajectories, two of them.  The call equals the host loop and a 30- and a 40-trajectory call from
    `last`.  nleap = 200 and T = 3: one trajectory per launch."""
    hc = hmc_case("auto", 70, 6)
    case = hc["case"]
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    sel = slice(0, 3)
    inp, off, f = _inputs(hc, sel), _offsets([3, 0, 0, 0]), case["f"]
    name, F, eps = hc["variants"][1]
    F, eps = F[sel], eps[sel]
    got, want = _compare(like, off, f, inp, eps, NLEAP, F, 7)
    one, want = _compare(like, off, f, inp, eps, NLEAP, F, 1)
    acc = ~np.isnan(one.log_ratio) & (inp["lnu"] < np.nan_to_num(one.log_ratio, nan=-np.inf))
    print("naccept", one.naccept, "before / after the boundary", acc[:, :64].sum(1), acc[:, 64:].sum(1), "aborted", want["aborted"])
    assert np.all(acc[:, :64].sum(1) > 0) and np.all(acc[:, 64:].sum(1) > 0) and np.all(one.naccept < 70) and np.array_equal(acc.sum(1), one.naccept)
    assert np.array_equal(got.theta, one.theta[:, 6::7]) and np.array_equal(got.last, one.last) and np.array_equal(got.naccept, one.naccept)
    cut = lambda a, b: dict(inp, mom=np.ascontiguousarray(inp["mom"][:, a:b]), lnu=np.ascontiguousarray(inp["lnu"][:, a:b]))
    first, _ = _compare(like, off, f, cut(0, 30), eps[:, :30], NLEAP, F, 1)
    second, _ = _compare(like, off, f, dict(cut(30, 70), theta0=first.last), eps[:, 30:], NLEAP, F, 1)
    for name in ("theta", "logp", "fullchi2", "best", "log_ratio"):
        assert np.array_equal(np.concatenate([getattr(first, name), getattr(second, name)], axis=1), getattr(one, name), equal_nan=True), name
    assert np.array_equal(second.last, one.last) and np.array_equal(first.naccept + second.naccept, one.naccept)
    _stored_records_are_the_draw_call(like, off, f, got)
    # one trajectory per launch; short steps, so that 200 of them stay a trajectory that can be accepted
    long, want = _compare(like, off, f, cut(0, 3), 0.02 * eps[:, :3], 200, F, 2)
    print("nleap = 200: naccept", long.naccept, "aborted", want["aborted"])
    assert long.theta.shape[1] == 1 and np.any(long.naccept > 0)
    eng.close()


def test_launches_that_store_nothing_before_one_that_does(golden):
    """nleap = 128, T = 5, thin = 5: two trajectories per launch, so three launches, of which the first two store no state.  With
    return_ratio they still bring their ratios back, all five of every chain; without it they bring nothing back.  The chain is the host
    loop's and the same in both runs.  The step sizes are those of the nleap = 4 runs over 32: trajectories of the same length."""
    hc = hmc_case("auto", 70, 6)
    case = hc["case"]
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    sel = slice(0, 3)
    inp, off, f = _inputs(hc, sel), _offsets([3, 0, 0, 0]), case["f"]
    inp = dict(inp, mom=np.ascontiguousarray(inp["mom"][:, :5]), lnu=np.ascontiguousarray(inp["lnu"][:, :5]))
    name, F, eps = hc["variants"][1]
    F, eps = F[sel], eps[sel, :5] / 32.0
    got, want = _compare(like, off, f, inp, eps, 128, F, 5)
    print("nleap = 128: naccept", got.naccept, "aborted", want["aborted"], "log_ratio", got.log_ratio)
    assert got.theta.shape[1] == 1 and got.log_ratio.shape == (3, 5) and np.any(got.naccept > 0) and np.any(np.isfinite(got.log_ratio[:, :4]))
    opt = {k: inp[k] for k in ("lower", "upper", "prior_loc", "prior_scale")}
    lean = like.hmc_draws_params(inp["theta0"], off, f, inp["mom"], inp["lnu"], eps, 128, factor=F, thin=5, return_best=True, **opt)
    assert lean.log_ratio is None
    for name in FIELDS[:-1]:
        assert np.array_equal(getattr(lean, name), getattr(got, name)), name
    eng.close()


def test_split_batches(golden):
    """a batch split over two calls with other offsets: the same bits per chain; no chains at all; eps as a scalar and per chain"""
    hc = hmc_case("auto")
    case = hc["case"]
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    inp, counts, f = _inputs(hc), np.array(case["counts"]), case["f"]
    off = _offsets(counts)
    name, F, eps = hc["variants"][1]
    whole, _ = _compare(like, off, f, inp, eps, NLEAP, F, THIN)
    cutc = np.array([1, 0, 2, 0])
    sel_a = np.concatenate([np.arange(off[c], off[c] + cutc[c]) for c in range(4)])
    sel_b = np.concatenate([np.arange(off[c] + cutc[c], off[c + 1]) for c in range(4)])
    for sel, cnt in ((sel_a, cutc), (sel_b, counts - cutc)):
        part, _ = _compare(like, _offsets(cnt), f, _inputs(hc, sel), eps[sel], NLEAP, F[sel], THIN)
        for name in FIELDS:
            assert np.array_equal(getattr(part, name), getattr(whole, name)[sel], equal_nan=True), name
    none = like.hmc_draws_params(np.zeros((0, 3)), [0, 0, 0, 0, 0], f, np.zeros((0, 4, 3)), np.zeros((0, 4)), 0.1, 2, thin=2, return_best=True, return_ratio=True)
    assert none.theta.shape == (0, 2, 3) and none.naccept.shape == (0,) and none.best.shape == (0, 2, like.nG) and none.log_ratio.shape == (0, 4)
    # eps as a scalar and per chain are the broadcast arrays; one factor for all chains is that factor per chain; None is the identity
    N = inp["theta0"].shape[0]
    for e in (0.3, eps[:, 0]):
        a, _ = _compare(like, off, f, inp, e, NLEAP, F[0], THIN)
        b, _ = _compare(like, off, f, inp, np.broadcast_to(e if np.ndim(e) == 0 else e[:, None], (N, T11)), NLEAP, np.tile(F[0], (N, 1, 1)), THIN)
        for name in FIELDS:
            assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    name, _, eps0 = hc["variants"][0]
    a, _ = _compare(like, off, f, inp, eps0, NLEAP, None, THIN)
    b, _ = _compare(like, off, f, inp, eps0, NLEAP, np.eye(3), THIN)
    for name in FIELDS:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    # no box and no prior on theta: the call with infinite ones
    free = {k: inp[k] for k in ("theta0", "mom", "lnu")}
    inf = np.full(3, np.inf)
    a, _ = _compare(like, off, f, free, eps0, NLEAP, None, THIN)
    b, _ = _compare(like, off, f, dict(free, lower=-inf, upper=inf, prior_loc=np.array([1.0, 2.0, 3.0]), prior_scale=inf), eps0, NLEAP, None, THIN)
    for name in FIELDS:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    eng.close()


def test_groups_against_their_own_data(golden):
    """groups= after set_datasets (M = 3) against the host loop through the groups gradient call; the groups of data set 0 are the call
    without groups bit for bit"""
    hc = hmc_case("auto")
    case = hc["case"]
    eng = _engine(golden, "auto", case)
    inp, f = _inputs(hc), case["f"]
    name, F, eps = hc["variants"][1]
    groups = [(3, 2), (0, 0), (2, 0), (0, 1), (2, 1)]
    counts = [2, 2, 1, 0, 3]
    wk, ds = np.array([w for w, _ in groups]), np.array([m for _, m in groups])
    off = _offsets(counts)
    Ds = datasets(case["D"], case["Ci"], 3)
    assert np.array_equal(Ds[0], case["D"])
    like = _like(eng, case, 0)
    like.set_datasets(Ds)
    got, want = _compare(like, off, f, inp, eps, NLEAP, F, THIN, groups=(wk, ds))
    print("groups: naccept", got.naccept, "aborted", want["aborted"], "refused", want["refused"])
    assert np.all(got.naccept > 0) and np.all(got.naccept < T11)
    _stored_records_are_the_draw_call(like, off, f, got, groups=(wk, ds))
    own = sorted((q for q, (w, m) in enumerate(groups) if m == 0), key=lambda q: groups[q][0])
    sel = np.concatenate([np.arange(off[q], off[q + 1]) for q in own])
    cnt = np.zeros(4, dtype=int)
    for q in own:
        cnt[groups[q][0]] = counts[q]
    plain, _ = _compare(like, _offsets(cnt), f, _inputs(hc, sel), eps[sel], NLEAP, F[sel], THIN)
    for name in FIELDS:
        assert np.array_equal(getattr(plain, name), getattr(got, name)[sel], equal_nan=True), name
    eng.close()


def test_failed_starts_and_refusals(golden):
    from eftpipe_amd import _lib as L
    from eftpipe_amd.marginal import MarginalLikelihood
    from eftpipe_amd.parambasis import DrawRecipe

    g, eng, T, index = _marg(golden, "auto", max_batch=4)
    rec, theta, _, _, f = _marg_case(g, "auto", [2, 2])
    D, Ci = g["auto_D"], g["auto_invcov"]
    nG = len(g["auto_loc"])
    eng.put("TEMPL", np.stack([T, T]))
    off = [0, 2, 4]
    N, P, Tn = 4, 3, 5
    rng = np.random.default_rng(6)
    mom, lnu, eps = rng.standard_normal((N, Tn, P)), np.log(rng.random((N, Tn))), 0.004
    # ---- det F2 <= 0 where theta_2 = 0: Gaussian row 3 times theta_2 under a flat prior (test_gpu_draw_chains.py)
    flat = MarginalLikelihood(eng, index, D, Ci, np.zeros(nG), np.full(nG, np.inf))
    idx3 = rec.idx.copy()
    idx3[rec.row == 3, 2] = 2
    flat.set_draw_recipe(DrawRecipe(rec.param_names, 1, nG + 1, rec.tracer, rec.row, rec.col, rec.coef, rec.fpow, idx3))
    th0 = theta.copy()
    th0[1, 2] = 0.0  # chain 1 starts on the singular plane
    inp = dict(theta0=th0, mom=mom, lnu=lnu)
    with pytest.raises(RuntimeError, match="det of F2ij"):
        flat.hmc_draws_params(th0, off, f, mom, lnu, eps, 3)
    raw, want = _compare(flat, off, f, inp, eps, 3, None, 2, raw=True)
    assert raw.naccept[1] == -1 and all(np.all(np.isnan(a[1])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last, raw.log_ratio))
    ok = [0, 2, 3]
    assert all(np.all(np.isfinite(a[ok])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last)) and np.all(raw.naccept[ok] > 0)
    # ---- refusals
    like = MarginalLikelihood(eng, index, D, Ci, g["auto_loc"], g["auto_scale"])
    with pytest.raises(L.EftbError, match="eftb_draws_hmc_params: no draw recipe"):
        like.hmc_draws_params(theta, off, f, mom, lnu, eps, 3)
    like.set_draw_recipe(rec)
    want = like.hmc_draws_params(theta, off, f, mom, lnu, eps, 3)
    call = lambda **kw: like.hmc_draws_params(**dict(dict(theta0=theta, offsets=off, f=f, momentum=mom, lnu=lnu, eps=eps, nleap=3), **kw))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    th, fo, o64, ep = np.ascontiguousarray(theta), np.ascontiguousarray(f), np.asarray(off, dtype=np.int64), np.full((N, Tn), eps)
    out = [np.zeros((N, Tn, P)), np.zeros((N, Tn)), np.zeros((N, Tn)), np.zeros((N, Tn, nG)), np.zeros((N, P))]
    nacc = np.zeros(N, dtype=np.int64)

    def ccall(Tc, nleap, thin):
        rc = eng.lib.eftb_draws_hmc_params(eng._h, 2, N, Tc, nleap, thin, i64(o64), dp(th), dp(fo), dp(mom), dp(lnu), dp(ep), None, None, None, None, None,
                                           *[dp(a) for a in out], i64(nacc), None)
        return rc, eng.lib.eftb_last_error().decode()

    for Tc, nleap, thin, msg in ((0, 3, 1, "T = 0 steps"), (Tn, 3, 0, "thin = 0 outside"), (Tn, 3, Tn + 1, "thin = 6 outside"), (Tn, 0, 1, "nleap = 0 leapfrog steps outside [1, 256]"),
                                 (Tn, 257, 1, "nleap = 257 leapfrog steps outside [1, 256]")):
        rc, err = ccall(Tc, nleap, thin)
        assert rc != 0 and msg in err, err
    assert ccall(Tn, 3, 1)[0] == 0 and np.array_equal(out[0], want.theta) and np.array_equal(out[4], want.last) and np.array_equal(nacc, want.naccept)
    for v in (np.nan, np.inf, -np.inf):
        bad = mom.copy()
        bad[2, 4, 1] = v
        with pytest.raises(L.EftbError, match="mom\\[2\\]\\[4\\]\\[1\\] is not finite"):
            call(momentum=bad)
    for v in (np.nan, 1e-3):
        bad = lnu.copy()
        bad[3, 4] = v
        with pytest.raises(L.EftbError, match="lnu\\[3\\]\\[4\\]"):
            call(lnu=bad)
    for v in (np.nan, np.inf, 0.0, -0.1):
        bad = np.full((N, Tn), eps)
        bad[1, 2] = v
        with pytest.raises(L.EftbError, match="eps\\[1\\]\\[2\\] = .* is not a finite step size > 0"):
            call(eps=bad)
    for v, msg in ((np.nan, "factor\\[3\\]\\[2\\]\\[1\\] is not finite"), (np.inf, "factor\\[3\\]\\[2\\]\\[1\\] is not finite")):
        bad = np.tile(np.eye(P), (N, 1, 1))
        bad[3, 2, 1] = v
        with pytest.raises(L.EftbError, match=msg):
            call(factor=bad)
    for v in (0.0, -1.0):
        bad = np.tile(np.eye(P), (N, 1, 1))
        bad[2, 1, 1] = v
        with pytest.raises(L.EftbError, match="factor\\[2\\]\\[1\\]\\[1\\] = .*, the diagonal must be > 0"):
            call(factor=bad)
    upper_junk = np.tile(np.eye(P), (N, 1, 1))
    upper_junk[:, 0, 2] = np.nan  # above the diagonal: not read
    assert np.array_equal(call(factor=upper_junk).theta, want.theta)
    lo, hi = theta.min(0) - 1.0, theta.max(0) + 1.0
    with pytest.raises(L.EftbError, match="lower\\[1\\] = .* > upper\\[1\\]"):
        call(lower=[lo[0], hi[1], lo[2]], upper=[hi[0], lo[1], hi[2]])
    with pytest.raises(L.EftbError, match="a bound of parameter 2 is NaN"):
        call(lower=[lo[0], lo[1], np.nan])
    for v in (0.0, -1.0, np.nan):
        with pytest.raises(L.EftbError, match="prior_scale\\[0\\]"):
            call(prior_scale=[v, 1.0, 1.0])
    j = int(np.argmin(theta[:, 1]))  # the one chain below a bound just above it
    with pytest.raises(L.EftbError, match="theta0\\[%d\\]\\[1\\] = .* outside" % j):
        call(lower=[lo[0], np.nextafter(theta[j, 1], np.inf), lo[2]])
    bad = theta.copy()
    bad[1, 2] = np.inf
    with pytest.raises(L.EftbError, match="theta\\[1\\]\\[2\\] is not finite"):
        call(theta0=bad)
    with pytest.raises(L.EftbError, match="offsets"):
        call(offsets=[0, 2, 5])
    with pytest.raises(L.EftbError, match="eftb_draws_hmc_params_datasets: no data sets"):
        call(groups=([0, 1], [0, 0]))
    assert np.array_equal(call().theta, want.theta)
    eng.close()


# ----------------------------------------------------------------------------- synthetic shapes
@pytest.mark.parametrize("case", list(HMC_WAVES))
def test_synthetic_shapes(case):
    """T = 4 trajectories of nleap = 3 steps under Gaussian theta priors at the smallest shapes that reach four waves, nG = 24, TWO, two
    waves, the tightest fits and the largest footprint: the host loop around the gradient call, every state's record included"""
    from test_gpu_draw_synthetic import _engine as s_engine, _like as s_like, _put

    pb = SY.case_problem(case)
    N, P = pb.theta.shape
    eng = s_engine(pb, len(pb.counts) * pb.ntr)
    _put(eng, pb)
    off = SY.offsets(pb.counts)
    rng = np.random.default_rng(31)
    inp = dict(theta0=pb.theta, mom=rng.standard_normal((N, 4, P)), lnu=np.log(rng.random((N, 4))), prior_loc=np.ones(P), prior_scale=np.full(P, 0.5))
    F = np.tril(0.05 * rng.standard_normal((N, P, P))) + np.eye(P)
    for jeff in (False, True):
        like = s_like(eng, pb, jeff)
        got, want = _compare(like, off, pb.f, inp, np.exp(rng.uniform(np.log(0.003), np.log(0.1), (N, 4))), 3, F, 1)
        print(case, jeff, "naccept", got.naccept, "aborted", want["aborted"], "refused", want["refused"])
        assert np.all(np.isfinite(got.logp)) and np.any(got.naccept > 0)
        _stored_records_are_the_draw_call(like, off, pb.f, got)
    eng.close()


def test_lds_refusal():
    """The LDS refusal is reachable at five tracers and nG = 24 (case I) with a padded recipe: every entry costs 8 bytes per workgroup and 8
    per wave.  The longest recipe that fits runs, one entry pair more is refused by message, while the gradient and chain calls still run."""
    from eftpipe_amd import _lib as L
    from test_gpu_draw_synthetic import _engine as s_engine, _like as s_like, _padded_recipe, _put

    pb = SY.case_problem("I")
    N, P = pb.theta.shape
    J1, nG, nnz, _ = hmc_shape("I")
    fits = max(n for n in range(nnz, 1025) if hmc_waves(J1, nG, n, P) == 1)
    assert nnz < fits < 1022 and hmc_waves(J1, nG, fits + 1, P) == 0
    eng = s_engine(pb, len(pb.counts) * pb.ntr)
    _put(eng, pb)
    off = SY.offsets(pb.counts)
    rng = np.random.default_rng(32)
    inp = dict(theta0=pb.theta, mom=rng.standard_normal((N, 2, P)), lnu=np.log(rng.random((N, 2))))
    like = s_like(eng, pb, False, rec=_padded_recipe(pb.rec, fits))
    got, _ = _compare(like, off, pb.f, inp, 0.003, 2, None, 1)
    assert np.all(np.isfinite(got.logp))
    like = s_like(eng, pb, False, rec=_padded_recipe(pb.rec, fits + 1))
    with pytest.raises(L.EftbError, match="eftb_draws_hmc_params: the trajectories of P = 8 parameters with nG = 24 and J \\+ 1 = 121 columns do not fit the LDS"):
        like.hmc_draws_params(pb.theta, off, pb.f, inp["mom"], inp["lnu"], 0.003, 2)
    assert np.all(np.isfinite(like.logp_draws_params(pb.theta, off, pb.f, grad=True)[1]))
    assert np.all(np.isfinite(like.metropolis_draws_params(pb.theta, off, pb.f, np.zeros((N, 1, P)), np.full((N, 1), -1.0)).logp))
    like = s_like(eng, pb, False)
    again, _ = _compare(like, off, pb.f, inp, 0.003, 2, None, 1)
    assert np.all(np.isfinite(again.logp))
    eng.close()
