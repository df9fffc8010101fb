"""Draw calls against many data vectors sharing one covariance on the device (eftb_set_likelihood_datasets, eftb_draws_logp_params_datasets;
MarginalLikelihood.set_datasets and ``groups=`` of logp_draws_params / maximize_draws_params).  Yardsticks: the oracle
(oracle/marginal.py), the data-space adjoint (grad_util.py) and the data-space Hessian (hess_util.py), each evaluated with the group's own
data vector D_m, at the tolerances test_gpu_draws_params.py, test_gpu_draws_grad.py and test_gpu_draws_hess.py use for the same
quantities; the Hessian bar is hess_util.device_bar of the floors test_draw_datasets.py measures on the host.  A group whose data set is
the likelihood's own vector returns the bits of the call without groups."""
import numpy as np
import pytest

import cfg3_util as U
import grad_util as GU
import hess_util as HU
from oracle import marginal as M
from test_draw_datasets import DATASET_FLOOR, datasets
from test_draw_hessian import TOL
from test_gpu_draws import _caseC_engine, _marg, _offsets
from test_gpu_draws_grad import BAR, _nnlo_problem
from test_gpu_draws_params import _cfg3_draws, _cfg3_engine, _marg_case

pytestmark = pytest.mark.gpu

GROUPS = [(1, 2), (0, 0), (1, 0), (0, 1), (1, 1)]  # (walker, data set): an empty group, repeats of both, not sorted by walker
GCOUNTS = [3, 0, 2, 4, 1]


def _table(groups):
    return np.array([w for w, _ in groups]), np.array([m for _, m in groups])


def _marg_groups(golden, tag, nwalk=2, M_=3, groups=GROUPS, counts=GCOUNTS):
    """engine with nwalk scaled walkers (as test_params_draws_match_oracle_and_fixture), recipe, theta, f [nwalk], the data sets, and per
    draw its walker and data set"""
    g, eng, T, index = _marg(golden, tag, max_batch=4)
    templ = np.stack([T * (1.0 + 0.1 * c) for c in range(nwalk)])
    eng.put("TEMPL", templ)
    rec, theta, _, _, f = _marg_case(g, tag, [int(np.sum(counts))])
    f = f[0] * (1.0 + 0.02 * np.arange(nwalk))
    Ds = datasets(g[tag + "_D"], g[tag + "_invcov"], M_)
    wk, ds = _table(groups)
    return g, eng, templ, index, rec, theta, f, Ds, np.repeat(wk, counts), np.repeat(ds, counts)


def _like(eng, rec, index, lk, jeffreys, Ds):
    from eftpipe_amd.marginal import MarginalLikelihood

    like = MarginalLikelihood(eng, index, *lk, jeffreys=jeffreys)
    like.set_draw_recipe(rec)
    if Ds is not None:
        like.set_datasets(Ds)
    return like


def _oracle(rec, th, ff, templ, index, d, lk, jeffreys, templn=None):
    """the oracle on the recipe's rows with data vector d -> ln P, full chi2, best fit"""
    V = GU.recipe_vectors(rec, th, ff, templ, index, templn)[0]
    return M.marginalized_logp(V[1:], V[0], d, lk[1], lk[2], lk[3], jeffreys=jeffreys, return_best=True)[:3]


def _relerr(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _check_oracle(out, rec, theta, f, templ, index, Ds, lk, jeffreys, dw, dm, rtol=1e-10, ntr=1):
    """every draw against the oracle with its group's D_m: ln P at rtol (1e-10; the flat prior 1e-9), full chi2 at 1e-9, best fit at 1e-8"""
    logp, full, best = out
    want = [_oracle(rec, theta[d], np.reshape(f, (-1, ntr))[dw[d]], templ[dw[d] * ntr : (dw[d] + 1) * ntr], index, Ds[dm[d]], lk, jeffreys) for d in range(theta.shape[0])]
    print("worst against the oracle: ln P %.2e, full chi2 %.2e relative, best fit %.2e" % (
        max(abs(logp[d] / w[0] - 1.0) for d, w in enumerate(want)), max(abs(full[d] / w[1] - 1.0) for d, w in enumerate(want)),
        max(_relerr(best[d], w[2]) for d, w in enumerate(want))))
    for d, w in enumerate(want):
        assert np.isclose(logp[d], w[0], rtol=rtol), (d, logp[d], w[0])
        assert np.isclose(full[d], w[1], rtol=1e-9), d
        assert _relerr(best[d], w[2]) < 1e-8, d


def _check_derivatives(tag, floor, like, rec, theta, off, f, groups, templ, index, Ds, lk, jeffreys, dw, dm, ntr=1, templn=None, hess=True):
    """gradient and Hessian of a groups call against the yardsticks evaluated with D_m, and the bits the three calls share"""
    fw = like.logp_draws_params(theta, off, f, return_best=True, groups=groups)
    lp, gr, full, best = like.logp_draws_params(theta, off, f, return_best=True, grad=True, groups=groups)
    for a, b in zip((lp, full, best), fw):
        assert np.array_equal(a, b)
    assert gr.shape == theta.shape and np.all(np.isfinite(gr))
    if hess:
        lph, grh, he, fullh, besth = like.logp_draws_params(theta, off, f, return_best=True, grad=True, hess=True, groups=groups)
        for a, b in zip((lph, grh, fullh, besth), (lp, gr, full, best)):
            assert np.array_equal(a, b)  # record and gradient of the Hessian call: the gradient call's bits
        assert np.array_equal(he, he.transpose(0, 2, 1)) and np.all(np.isfinite(he))
    worst_g = worst_h = 0.0
    for d in range(theta.shape[0]):
        w, m = dw[d], dm[d]
        args = (rec, theta[d], np.reshape(f, (-1, ntr))[w], templ[w * ntr : (w + 1) * ntr], index, Ds[m], lk[1], lk[2], lk[3])
        tn = None if templn is None else templn[w * ntr : (w + 1) * ntr]
        lpy, gy, gmag = GU.adjoint_of_draw(*args, jeffreys=jeffreys, templn=tn)
        assert np.isclose(lp[d], lpy, rtol=1e-9), d
        worst_g = max(worst_g, float(np.max(np.abs(gr[d] - gy) / gmag)))
        if hess:
            _, hy, hmag = HU.hessian_of_draw(*args, jeffreys=jeffreys, templn=tn)
            worst_h = max(worst_h, float(np.max(np.abs(he[d] - hy) / hmag)))
    bar = HU.device_bar(floor)
    print(tag, "jeffreys" if jeffreys else "", "groups: worst |grad - adjoint| / mag = %.2e (bar %.1e), |hess - yardstick| / mag = %.2e (bar %.1e)" % (worst_g, BAR, worst_h, bar))
    assert worst_g < BAR, (tag, jeffreys, worst_g)
    assert worst_h < bar, (tag, jeffreys, worst_h)
    return lp, gr


# ----------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("tag", ["auto", "cross"])
def test_groups_match_oracle(golden, tag):
    g, eng, templ, index, rec, theta, f, Ds, dw, dm = _marg_groups(golden, tag)
    off, groups = _offsets(GCOUNTS), _table(GROUPS)
    loc, scale = g[tag + "_loc"], g[tag + "_scale"]
    nG = len(loc)
    priors = [(loc, scale, False, 1e-10), (loc, scale, True, 1e-10)] + ([(np.zeros(nG), np.full(nG, np.inf), False, 1e-9)] if tag == "auto" else [])
    seen = []
    for lo, sc, jeff, rtol in priors:
        lk = (Ds[0], g[tag + "_invcov"], lo, sc)
        like = _like(eng, rec, index, lk, jeff, Ds)
        out = like.logp_draws_params(theta, off, f, return_best=True, groups=groups)
        N = theta.shape[0]
        assert out[0].shape == out[1].shape == (N,) and out[2].shape == (N, nG)
        _check_oracle(out, rec, theta, f, templ, index, Ds, lk, jeff, dw, dm, rtol=rtol)
        assert np.array_equal(like.logp_draws_params(theta, off, f, groups=groups), out[0])
        seen.append(out[0])
    assert not np.allclose(seen[0], seen[1], rtol=1e-6)
    eng.close()


# ----------------------------------------------------------------------------- 2. bit identity with the call without groups
@pytest.mark.parametrize("tag", ["auto", "cross"])
def test_own_vector_groups_are_the_plain_call_bit_for_bit(golden, tag):
    counts = [3, 4]
    g, eng, templ, index, rec, theta, f, Ds, dw, dm = _marg_groups(golden, tag, groups=[(0, 0), (1, 0)], counts=counts)
    off = _offsets(counts)
    lk = (Ds[0], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"])
    for jeff in (False, True):
        like = _like(eng, rec, index, lk, jeff, Ds)
        kw = dict(return_best=True, grad=True, hess=True)
        plain = like.logp_draws_params(theta, off, f, **kw)
        groups = ([0, 1], [0, 0])
        got = like.logp_draws_params(theta, off, f, groups=groups, **kw)
        assert all(np.array_equal(a, b) for a, b in zip(got, plain))
        again = like.logp_draws_params(theta, off, f, groups=groups, **kw)  # the cached Wg
        assert all(np.array_equal(a, b) for a, b in zip(again, plain))
        for a, b in zip(like.logp_draws_params(theta, off, f, groups=groups, return_best=True), like.logp_draws_params(theta, off, f, return_best=True)):
            assert np.array_equal(a, b)
        # the same groups split over two calls, in the other order, with other tables
        a = like.logp_draws_params(theta[off[1] :], [0, counts[1]], f, groups=([1], [0]), **kw)
        b = like.logp_draws_params(theta[: off[1]], [0, 0, counts[0]], f, groups=([1, 0], [0, 0]), **kw)
        assert all(np.array_equal(np.concatenate([y, x]), z) for x, y, z in zip(a, b, plain))
        # beside other data sets in one call
        mixed = like.logp_draws_params(np.concatenate([theta, theta]), _offsets(counts + counts), f, groups=([0, 1, 0, 1], [0, 0, 2, 1]), **kw)
        assert all(np.array_equal(x[: theta.shape[0]], z) for x, z in zip(mixed, plain))
        assert not np.allclose(mixed[0][theta.shape[0] :], plain[0], rtol=1e-6)
    eng.close()


# ----------------------------------------------------------------------------- 3. derivatives against the yardsticks
@pytest.mark.parametrize("tag", ["auto", "cross"])
def test_groups_derivatives_match_yardsticks(golden, tag):
    g, eng, templ, index, rec, theta, f, Ds, dw, dm = _marg_groups(golden, tag)
    off, groups = _offsets(GCOUNTS), _table(GROUPS)
    lk = (Ds[0], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"])
    grads = []
    for jeff in (False, True):
        like = _like(eng, rec, index, lk, jeff, Ds)
        grads.append(_check_derivatives(tag, DATASET_FLOOR[tag], like, rec, theta, off, f, groups, templ, index, Ds, lk, jeff, dw, dm)[1])
    assert not np.allclose(grads[0], grads[1], rtol=1e-6)  # the trace term is there
    eng.close()


# ----------------------------------------------------------------------------- 4. cfg 3: three tracers, J + 1 = 73, the two-column-half kernels
def test_cfg3_xnost_groups(golden):
    from eftpipe_amd.marginal import joint_draw_recipe

    g = golden("cfg3")
    groups_l, counts = [(0, 1), (1, 0), (1, 1)], [3, 2, 2]
    eng, templ, index = _cfg3_engine(g, 2, 6)
    names = [str(n) for n in g["xnost_names"]]
    nG = len(names)
    pn, theta, f = _cfg3_draws(g, [sum(counts)], 9)
    f = f[0] * (1.0 + 0.01 * np.arange(2)[:, None] * [1.0, 2.0, 3.0])
    rec = joint_draw_recipe(U.bases(), names, U.scales(g), param_names=pn)
    lk = (g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf))
    Ds = datasets(lk[0], lk[1], 2)
    off, groups = _offsets(counts), _table(groups_l)
    dw, dm = np.repeat(groups[0], counts), np.repeat(groups[1], counts)
    for jeff in (True, False):
        like = _like(eng, rec, index, lk, jeff, Ds)
        out = like.logp_draws_params(theta, off, f, return_best=True, groups=groups)
        for d in range(theta.shape[0]):  # (_cfg3_oracle's formula on the recipe's rows, with D_m: its tolerances)
            want = _oracle(rec, theta[d], f[dw[d]], templ[3 * dw[d] : 3 * dw[d] + 3], index, Ds[dm[d]], lk, jeff)
            assert np.isclose(out[0][d], want[0], rtol=1e-9), d
            assert np.isclose(out[1][d], want[1], rtol=1e-8), d
        _check_derivatives("cfg3 xnost", DATASET_FLOOR["xnost"], like, rec, theta, off, f, groups, templ, index, Ds, lk, jeff, dw, dm, ntr=3)
        kw = dict(return_best=True, grad=True, hess=True)
        got = like.logp_draws_params(theta, off, f, groups=groups, **kw)
        sel = slice(off[1], off[2])  # group (1, 0): the likelihood's own vector on walker 1
        plain = like.logp_draws_params(theta[sel], [0, 0, counts[1]], f, **kw)
        assert all(np.array_equal(x[sel], z) for x, z in zip(got, plain))
    eng.close()


# ----------------------------------------------------------------------------- 5. NNLO columns in the border
def test_nnlo_groups():
    eng, rec, theta, f, _, T, TN, index, D, Ci, nG = _nnlo_problem()
    counts = [2, 3]
    theta, f = theta[:5], f[:1]
    lk = (D, Ci, np.zeros(nG), np.full(nG, 2.0))
    Ds = datasets(D, Ci, 2)
    groups = ([0, 0], [0, 1])
    dw, dm = np.zeros(5, dtype=int), np.repeat([0, 1], counts)
    for jeff in (False, True):
        like = _like(eng, rec, index, lk, jeff, Ds)
        lp, gr = _check_derivatives("nnlo", 0.0, like, rec, theta, _offsets(counts), f, groups, T, index, Ds, lk, jeff, dw, dm, templn=TN, hess=False)
        plain = like.logp_draws_params(theta[:2], [0, 2], f, grad=True)
        assert np.array_equal(lp[:2], plain[0]) and np.array_equal(gr[:2], plain[1])
        # without the NNLO columns in the border the other data set could not come out right: they carry weight here
        no_nnlo = GU.adjoint_of_draw(rec, theta[4], f[0], T[:1], index, Ds[1], *lk[1:], jeffreys=jeff, templn=0.0 * TN[:1])[0]
        assert abs(no_nnlo - lp[4]) > 1e-6 * abs(lp[4])
    eng.close()


# ----------------------------------------------------------------------------- 6. state
def test_groups_follow_data_sets_templates_and_likelihood(golden):
    from eftpipe_amd import _lib as L

    tag = "auto"
    g, eng, templ, index, rec, theta, f, Ds, dw, dm = _marg_groups(golden, tag)
    off, groups = _offsets(GCOUNTS), _table(GROUPS)
    lk = (Ds[0], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"])
    like = _like(eng, rec, index, lk, False, Ds)
    kw = dict(return_best=True, groups=groups)
    first = like.logp_draws_params(theta, off, f, **kw)
    # other data
    Ds2 = Ds[::-1] + 0.0
    like.set_datasets(Ds2)
    out = like.logp_draws_params(theta, off, f, **kw)
    assert not np.allclose(out[0], first[0], rtol=1e-6)
    _check_oracle(out, rec, theta, f, templ, index, Ds2, lk, False, dw, dm)
    # other templates
    templ2 = templ * np.array([1.05, 0.97])[:, None, None, None]
    eng.put("TEMPL", templ2)
    out2 = like.logp_draws_params(theta, off, f, **kw)
    assert not np.allclose(out2[0], out[0], rtol=1e-6)
    _check_oracle(out2, rec, theta, f, templ2, index, Ds2, lk, False, dw, dm)
    eng.put("TEMPL", templ)
    like.set_datasets(Ds)
    assert all(np.array_equal(a, b) for a, b in zip(like.logp_draws_params(theta, off, f, **kw), first))
    # withdrawn, and dropped by a new likelihood
    like.set_datasets(None)
    with pytest.raises(L.EftbError, match="eftb_draws_logp_params_datasets: no data sets"):
        like.logp_draws_params(theta, off, f, **kw)
    like.set_datasets(Ds)
    like = _like(eng, rec, index, lk, False, None)
    with pytest.raises(L.EftbError, match="no data sets \\(eftb_set_likelihood_datasets; eftb_set_likelihood and eftb_set_tracers drop them\\)"):
        like.logp_draws_params(theta, off, f, **kw)
    like.set_datasets(Ds)
    assert all(np.array_equal(a, b) for a, b in zip(like.logp_draws_params(theta, off, f, **kw), first))
    eng.close()


def test_other_calls_are_untouched_by_groups_calls(golden):
    """eval_logp (slow step), plain draw calls, eval_logp again: with groups calls in between, every one gives the bits it gives without"""
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe
    from eftpipe_amd.parambasis import WestCoastBasis, gaussian_params, gaussian_rows

    B = 2
    g, eng, index, nb = _caseC_engine(golden, 4)
    rng = np.random.default_rng(31)
    sc = dict(kmA=0.7, krA=0.25, ndA=4.5e-5)
    Pin = g["Pin"][None] * (1.0 + 0.1 * rng.uniform(-1, 1, (B, 1)))
    fs = float(g["f"]) * (1.0 + 0.03 * rng.uniform(-1, 1, B))
    DA, H = np.full(B, float(g["DA"])), np.full(B, float(g["H"]))
    ng = np.array([[2.0, 0.5, 0.3], [2.1, 0.4, 0.2]])
    rows = np.stack([gaussian_rows(fi, tuple(p), None, **sc) for fi, p in zip(fs, ng)])
    templ = eng.eval_batch(Pin, fs, DA, H)
    model = np.einsum("r,lrx->lx", rows[0, 0], templ[0]).reshape(-1)[index]
    lk = (model * 1.02, np.diag(1.0 / (0.05 * np.abs(model) + 10.0) ** 2), np.zeros(7), np.full(7, 3.0))
    like = MarginalLikelihood(eng, index, *lk)
    like.set_draw_recipe(joint_draw_recipe([WestCoastBasis(prefix="")], gaussian_params(""), [sc]))
    like.set_datasets(datasets(lk[0], lk[1], 3))
    theta = np.concatenate([ng, ng + 0.05])
    off = [0, 2, 4]

    def sequence(with_groups):
        gc = lambda: like.logp_draws_params(theta, [0, 1, 3, 4], fs, grad=True, hess=True, groups=([1, 0, 1], [2, 1, 0])) if with_groups else None
        lp0 = like.eval_logp(Pin, fs, DA, H, rows)
        gc()
        a = like.logp_draws_params(theta, off, fs, return_best=True, grad=True, hess=True)
        gc()
        b = like.logp_draws_params(theta, off, fs)
        gc()
        lp1 = like.eval_logp(Pin[::-1].copy(), fs[::-1].copy(), DA, H, rows[::-1].copy())
        gc()
        return (lp0, lp1, b) + tuple(a)

    x, y = sequence(False), sequence(True)
    assert all(np.array_equal(p, q) for p, q in zip(x, y))
    eng.close()


# ----------------------------------------------------------------------------- 7. refusals
def test_groups_refusals(golden):
    from eftpipe_amd import _lib as L

    tag = "auto"
    g, eng, templ, index, rec, theta, f, Ds, dw, dm = _marg_groups(golden, tag)
    off, groups = _offsets(GCOUNTS), _table(GROUPS)
    lk = (Ds[0], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"])
    like = _like(eng, rec, index, lk, False, None)
    who = "eftb_draws_logp_params_datasets: "
    with pytest.raises(L.EftbError, match=who + "no data sets"):
        like.logp_draws_params(theta, off, f, groups=groups)
    bad = Ds.copy()
    bad[1, 5] = np.nan
    with pytest.raises(L.EftbError, match="eftb_set_likelihood_datasets: data\\[1\\]\\[5\\] is not finite"):
        like.set_datasets(bad)
    with pytest.raises(L.EftbError, match=who + "no data sets"):  # nothing was copied
        like.logp_draws_params(theta, off, f, groups=groups)
    like.set_datasets(Ds)
    want = like.logp_draws_params(theta, off, f, groups=groups, grad=True, hess=True)
    bad[1, 5] = np.inf
    with pytest.raises(L.EftbError, match="data\\[1\\]\\[5\\] is not finite"):
        like.set_datasets(bad)
    assert all(np.array_equal(a, b) for a, b in zip(like.logp_draws_params(theta, off, f, groups=groups, grad=True, hess=True), want))  # the old sets stand
    wk, ds = groups
    for w_bad, name in ((2, "walker"), (-1, "walker")):
        w2 = wk.copy()
        w2[3] = w_bad
        with pytest.raises(L.EftbError, match=who + "walker\\[3\\] = %d outside \\[0, 2\\)" % w_bad):
            like.logp_draws_params(theta, off, f, groups=(w2, ds))
    w2 = wk.copy()
    w2[4] = 2  # inside [0, C) of a three-walker f, beyond the two walkers of the block
    with pytest.raises(L.EftbError, match=who + "walker\\[4\\] = 2 with 1 tracers, but the template block holds 2 entries"):
        like.logp_draws_params(theta, off, np.append(f, f[0]), groups=(w2, ds))
    for m_bad in (3, -2):
        d2 = ds.copy()
        d2[2] = m_bad
        with pytest.raises(L.EftbError, match=who + "dataset\\[2\\] = %d outside \\[0, 3\\)" % m_bad):
            like.logp_draws_params(theta, off, f, groups=(wk, d2))
    for o_bad, msg in (([1, 3, 3, 5, 9, 10], "offsets\\[0\\] = 1, not 0"), ([0, 3, 2, 5, 9, 10], "offsets decrease at group 1"), ([0, 3, 3, 5, 9, 11], "offsets\\[5\\] = 11, not the 10 draws")):
        with pytest.raises(L.EftbError, match=who + msg):
            like.logp_draws_params(theta, o_bad, f, groups=groups)
    th_bad = theta.copy()
    th_bad[7, 1] = np.nan
    with pytest.raises(L.EftbError, match=who + "theta\\[7\\]\\[1\\] is not finite"):
        like.logp_draws_params(th_bad, off, f, groups=groups)
    with pytest.raises(L.EftbError, match=who + "f\\[1\\]\\[0\\] is not finite"):
        like.logp_draws_params(theta, off, [f[0], np.inf], groups=groups)
    with pytest.raises(ValueError, match="hess=True needs grad=True"):
        like.logp_draws_params(theta, off, f, groups=groups, hess=True)
    # the library's own refusal of hess without grad
    import ctypes as C

    dp, i32p = (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), C.POINTER(C.c_int32)
    N, P = theta.shape
    lp, he = np.zeros(N), np.zeros((N, P, P))
    w32, d32 = wk.astype(np.int32), ds.astype(np.int32)
    rc = eng.lib.eftb_draws_logp_params_datasets(eng._h, 2, 5, w32.ctypes.data_as(i32p), d32.ctypes.data_as(i32p), N, off.ctypes.data_as(C.POINTER(C.c_int64)),
                                                 dp(np.ascontiguousarray(theta)), dp(np.ascontiguousarray(f)), dp(lp), None, dp(he), None, None)
    assert rc != 0 and "hess needs grad" in eng.lib.eftb_last_error().decode()
    like.set_draw_recipe(None)
    with pytest.raises(L.EftbError, match=who + "no draw recipe"):
        like.logp_draws_params(theta, off, f, groups=groups)
    like.set_draw_recipe(rec)
    # the engine still answers: the groups call, and a plain call against the oracle
    assert all(np.array_equal(a, b) for a, b in zip(like.logp_draws_params(theta, off, f, groups=groups, grad=True, hess=True), want))
    counts = [6, 4]
    out = like.logp_draws_params(theta, _offsets(counts), f, return_best=True)
    _check_oracle(out, rec, theta, f, templ, index, Ds, lk, False, np.repeat([0, 1], counts), np.zeros(10, dtype=int))
    eng.set_tracers(1)
    with pytest.raises(L.EftbError, match="eftb_set_likelihood"):
        like.logp_draws_params(theta, off, f, groups=groups)
    with pytest.raises(L.EftbError, match="eftb_set_likelihood_datasets: the data sets share a likelihood's index, covariance and priors: needs eftb_set_likelihood first"):
        like.set_datasets(Ds)
    eng.close()


# ----------------------------------------------------------------------------- 8. best fits of several data sets in one call
_BESTFITS = {}


def _bestfits(golden):
    """marg.npz auto, 1 walker, M = 3, two starts per group (the fixture's point scaled by 0.95 and 1.05), run once for the tests below"""
    if not _BESTFITS:
        tag = "auto"
        g, eng, T, index = _marg(golden, tag, max_batch=4)
        eng.put("TEMPL", T[None])
        rec, theta, _, _, f = _marg_case(g, tag, [1])
        f = f[:1]
        lk = (g[tag + "_D"], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"])
        Ds = datasets(lk[0], lk[1], 3)
        like = _like(eng, rec, index, lk, False, Ds)
        starts = np.concatenate([theta[:1] * s for _ in range(3) for s in (0.95, 1.05)])
        out = like.maximize_draws_params(starts, [0, 2, 4, 6], f, groups=([0, 0, 0], [0, 1, 2]), tol=TOL)
        plain = like.maximize_draws_params(starts[:2], [0, 2], f, tol=TOL)
        eng.close()
        print("iterations", out[4].tolist(), "ln P", out[1].tolist())
        _BESTFITS.update(out=out, plain=plain, rec=rec, f=f, T=T, index=index, lk=lk, Ds=Ds)
    return _BESTFITS


def test_maximize_draws_params_groups(golden):
    """all starts converge; the yardstick's Newton decrement at each result, evaluated with the group's D_m, is <= 10 tol; the
    best fits of data sets 1 and 2 are not set 0's"""
    b = _bestfits(golden)
    th, logp, grad, hess, n_iter, converged = b["out"]
    assert th.shape == (6, 3) and hess.shape == (6, 3, 3) and np.all(converged)
    worst = 0.0
    for d in range(6):
        args = (b["rec"], th[d], b["f"][0], b["T"][None], b["index"], b["Ds"][d // 2], *b["lk"][1:])
        gy, hy = GU.adjoint_of_draw(*args)[1], HU.hessian_of_draw(*args)[1]
        dec = float(gy @ np.linalg.solve(-hy, gy))
        worst = max(worst, dec)
        assert 0.0 <= dec <= 10 * TOL, (d, dec)
    print("worst yardstick decrement at the results: %.2e" % worst)
    for m in (1, 2):
        for s in (0, 1):
            assert np.max(np.abs(th[2 * m + s] - th[s])) > 1e-3 * np.max(np.abs(th[s])) and abs(logp[2 * m + s] - logp[s]) > 1e-6 * abs(logp[s])
    # set 0 in a groups call climbs as the call without groups does
    assert all(np.array_equal(x[:2], y) for x, y in zip(b["out"], b["plain"]))


@pytest.mark.parametrize("m", [0, 1, 2])
def test_maximize_groups_starts_agree(golden, m):
    """the two starts of a group agree in ln P to 1e-9 relative.

    Data set 0 (the fixture's own vector) sits close to a watershed: ln P of ``marg.npz`` auto has two maxima along the b2 - b4 degeneracy
    (-19.1168 and -19.1783 with the Gaussian prior), and which one the start scaled by 0.95 reaches depends on the last bits
    of W.  On the NumPy evaluator (hess_util.gram_hessian, the same newton_maximize) both starts end at -19.11683044 with
    grad_util.gram_matrix's own W, and the 0.95 start ends at -19.17825537 once the border of set 0 is summed again in another order
    (test_draw_datasets.bordered_gram), which moves W by 1e-16 of its scale.  On the device Wg of set 0 has the bits of W_c, so the groups
    call climbs as the call without groups does (test_maximize_draws_params_groups asserts those bits).  Sets 1 and 2 are not sensitive:
    -35.33075901 and -41.28508711 from both starts on the host."""
    logp = _bestfits(golden)["out"][1]
    print("data set", m, "ln P of the two starts", logp[2 * m], logp[2 * m + 1])
    assert abs(logp[2 * m] - logp[2 * m + 1]) <= 1e-9 * abs(logp[2 * m])
