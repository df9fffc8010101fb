"""d2 ln P / d theta d theta of the params draws on the device (eftb_draws_logp_hess_params; MarginalLikelihood.logp_draws_params(grad=True,
hess=True)) and the Newton best fits built on it (MarginalLikelihood.maximize_draws_params).  Yardstick: the data-space Hessian of
hess_util.py (pinned on the host by test_draw_hessian.py), draw for draw, in units of mag_pq.  Bar (hess_util.device_bar): 1e-10 of mag
where the NumPy restatement of the Gram route sits at <= 1e-12 of it (auto, xnost, NNLO), 100 times that floor elsewhere (cross 1.6e-10,
cfg 3 full 9.8e-10).  ln P, the gradient, full chi2 and the best fit of the Hessian call are the bits of the gradient call."""
import ctypes as C

import numpy as np
import pytest

import cfg3_util as U
import grad_util as GU
import hess_util as HU
from test_draw_hessian import TOL, newton_problem, yardstick_decrement
from test_gpu_draws import COUNTS, _caseC_engine, _marg, _offsets
from test_gpu_draws_grad import _nnlo_problem
from test_gpu_draws_params import _cfg3_draws, _cfg3_engine, _marg_case

pytestmark = pytest.mark.gpu


def _check(tag, key, like, rec, theta, off, f, walker, templ, index, lk, jeffreys, templn=None, ntr=1, sample=None):
    """the Hessian call against the gradient call (bits) and against the yardstick; -> hess, worst error / mag"""
    want = like.logp_draws_params(theta, off, f, return_best=True, grad=True)
    logp, grad, hess, full, best = like.logp_draws_params(theta, off, f, return_best=True, grad=True, hess=True)
    P = theta.shape[1]
    assert hess.shape == (theta.shape[0], P, P) and np.all(np.isfinite(hess))
    for a, b in zip((logp, grad, full, best), want):
        assert np.array_equal(a, b)
    assert np.array_equal(hess, hess.transpose(0, 2, 1))
    lp2, g2, h2 = like.logp_draws_params(theta, off, f, grad=True, hess=True)
    assert np.array_equal(h2, hess) and np.array_equal(g2, grad) and np.array_equal(lp2, logp)  # a repeat call: the same bits
    worst = 0.0
    for d in range(theta.shape[0]) if sample is None else sample:
        w = walker[d]
        _, h, mag = HU.hessian_of_draw(rec, theta[d], np.reshape(f, (len(off) - 1, ntr))[w], templ[w * ntr : (w + 1) * ntr], index, *lk, jeffreys=jeffreys,
                                       templn=None if templn is None else templn[w * ntr : (w + 1) * ntr])
        worst = max(worst, float(np.max(np.abs(hess[d] - h) / mag)))
    bar = HU.device_bar(HU.GRAM_FLOOR[key] if isinstance(key, str) else key)
    print(tag, "jeffreys" if jeffreys else "", "worst |hess - yardstick| / mag = %.2e (bar %.1e)" % (worst, bar))
    assert worst < bar, (tag, jeffreys, worst)
    return hess, worst


@pytest.mark.parametrize("tag", ["auto", "cross"])
def test_hess_matches_data_space_hessian(golden, tag):
    from eftpipe_amd.marginal import MarginalLikelihood

    g, eng, T, index = _marg(golden, tag)
    nC = len(COUNTS)
    templ = np.stack([T * (1.0 + 0.1 * c) for c in range(nC)])
    eng.put("TEMPL", templ)
    rec, theta, _, walker, f = _marg_case(g, tag, COUNTS)
    off = _offsets(COUNTS)  # (walker 1 owns no draw)
    D, Ci, loc, scale = g[tag + "_D"], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"]
    nG = len(loc)
    priors = [(loc, scale, False), (loc, scale, True)] + ([(np.zeros(nG), np.full(nG, np.inf), False), (np.zeros(nG), np.full(nG, np.inf), True)] if tag == "auto" else [])
    hs = []
    for lo, sc, jeff in priors:  # (flat prior: auto only, the cross fixture's 11 parameters are degenerate without one)
        like = MarginalLikelihood(eng, index, D, Ci, lo, sc, jeffreys=jeff)
        like.set_draw_recipe(rec)
        hs.append(_check(tag, tag, like, rec, theta, off, f, walker, templ, index, (D, Ci, lo, sc), jeff)[0])
    assert not np.allclose(hs[0], hs[1], rtol=1e-6)  # the trace term is there
    with pytest.raises(ValueError, match="hess=True needs grad=True"):
        like.logp_draws_params(theta, off, f, hess=True)
    eng.close()


@pytest.mark.parametrize("tag", ["full", "xnost"])
def test_cfg3_joint_hess(golden, tag):
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe

    g = golden("cfg3")
    counts = [150, 0, 1, 196]  # (a few hundred draws over 4 walkers, one empty, one with a single draw)
    eng, templ, index = _cfg3_engine(g, 4, 12)
    names = [str(n) for n in g[tag + "_names"]]
    nG = len(names)
    pn, theta, f = _cfg3_draws(g, counts, 9)
    rec = joint_draw_recipe(U.bases(), names, U.scales(g), param_names=pn)
    walker = np.repeat(np.arange(4), counts)
    lk = (g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf))
    sample = np.sort(np.random.default_rng(2).choice(theta.shape[0], 12, replace=False))
    for jeff in (True, False):
        like = MarginalLikelihood(eng, index, *lk, jeffreys=jeff)
        like.set_draw_recipe(rec)
        _check("cfg3 " + tag, tag, like, rec, theta, _offsets(counts), f, walker, templ, index, lk, jeff, ntr=3, sample=sample)
    eng.close()


def test_nnlo_hess():
    from eftpipe_amd.marginal import MarginalLikelihood

    eng, rec, theta, f, counts, T, TN, index, D, Ci, nG = _nnlo_problem()
    walker = np.repeat(np.arange(len(counts)), counts)
    for jeff in (False, True):
        lk = (D, Ci, np.zeros(nG), np.full(nG, 2.0))
        like = MarginalLikelihood(eng, index, *lk, jeffreys=jeff)
        like.set_draw_recipe(rec)
        floor = 0.0  # the Gram route in NumPy against the yardstick on these draws: what the device bar follows from
        for d in range(theta.shape[0]):
            w = walker[d]
            _, h, mag = HU.hessian_of_draw(rec, theta[d], f[w], T[w : w + 1], index, *lk, jeffreys=jeff, templn=TN[w : w + 1])
            hg = HU.gram_hessian(rec, theta[d], f[w], GU.gram_matrix(T[w : w + 1], index, D, Ci, TN[w : w + 1]), lk[2], lk[3], jeffreys=jeff)[2]
            floor = max(floor, float(np.max(np.abs(hg - h) / mag)))
        print("nnlo: floor of the Gram route on the host %.2e" % floor)
        assert floor <= 1e-12
        _check("nnlo", floor, like, rec, theta, _offsets(counts), f, walker, T, index, lk, jeff, templn=TN)
    eng.close()


def test_split_calls_single_draws_and_empty_walkers(golden):
    """one batch submitted whole, and split into two calls with other offsets, gives the same bits per draw; so does one draw alone; walkers
    without draws and N = 0 are in order"""
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe

    g = golden("cfg3")
    nC = 4
    rng = np.random.default_rng(5)
    counts = np.array([700, 0, 1, 1500])  # (more draws than one pass of a workgroup's waves)
    eng, templ, index = _cfg3_engine(g, nC, 3 * nC)
    names = [str(n) for n in g["full_names"]]
    nG = len(names)
    pn, theta, f = _cfg3_draws(g, counts, 79)
    rec = joint_draw_recipe(U.bases(), names, U.scales(g), param_names=pn)
    for jeff in (False, True):
        like = MarginalLikelihood(eng, index, g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf), jeffreys=jeff)
        like.set_draw_recipe(rec)
        off = _offsets(counts)
        logp, grad, hess, full, best = like.logp_draws_params(theta, off, f, return_best=True, grad=True, hess=True)
        assert np.all(np.isfinite(hess)) and np.array_equal(hess, hess.transpose(0, 2, 1))
        cut = np.array([rng.integers(0, c + 1) for c in counts])
        sel_a = np.concatenate([np.arange(off[c], off[c] + cut[c]) for c in range(nC)])
        sel_b = np.concatenate([np.arange(off[c] + cut[c], off[c + 1]) for c in range(nC)])
        for sel, cnt in ((sel_a, cut), (sel_b, counts - cut)):
            lp, gr, he, fu, be = like.logp_draws_params(theta[sel], _offsets(cnt), f, return_best=True, grad=True, hess=True)
            assert np.array_equal(he, hess[sel]) and np.array_equal(gr, grad[sel]) and np.array_equal(lp, logp[sel])
            assert np.array_equal(fu, full[sel]) and np.array_equal(be, best[sel])
        d = int(off[3]) + 11
        lp, gr, he = like.logp_draws_params(theta[d : d + 1], [0, 0, 0, 0, 1], f, grad=True, hess=True)
        assert he.shape == (1, 6, 6) and np.array_equal(he[0], hess[d]) and np.array_equal(gr[0], grad[d]) and lp[0] == logp[d]
        lp, gr, he = like.logp_draws_params(np.zeros((0, 6)), [0, 0, 0, 0, 0], f, grad=True, hess=True)
        assert lp.shape == (0,) and gr.shape == (0, 6) and he.shape == (0, 6, 6)
    eng.close()


def _raw_hess(eng, theta, off, f, grad=True, hess=True):
    """the library call itself (the Python wrapper raises where ln P is NaN) -> rc, logp, grad, hess"""
    theta, off, f = np.ascontiguousarray(theta, dtype=np.float64), np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(f, dtype=np.float64)
    N, P = theta.shape
    logp, gr, he = np.zeros(N), np.zeros((N, P)), np.zeros((N, P, P))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = eng.lib.eftb_draws_logp_hess_params(eng._h, off.size - 1, N, off.ctypes.data_as(C.POINTER(C.c_int64)), dp(theta), dp(f), dp(logp), dp(gr) if grad else None,
                                             dp(he) if hess else None, None, None)
    return rc, logp, gr, he


def test_hess_refusals_and_nan_rows(golden):
    from eftpipe_amd import _lib as L
    from eftpipe_amd import synth
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.marginal import MarginalLikelihood, data_index, joint_draw_recipe
    from eftpipe_amd.parambasis import DrawRecipe, WestCoastBasis, bias_row, gaussian_params
    from eftpipe_amd.tables import EngineConfig

    g, eng, T, index = _marg(golden, "auto", max_batch=4)
    rec, theta, _, _, f = _marg_case(g, "auto", [2, 2])
    nG = len(g["auto_loc"])
    eng.put("TEMPL", np.stack([T, T]))
    mk = lambda: MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], g["auto_loc"], g["auto_scale"])
    like = mk()
    off = [0, 2, 4]
    kw = dict(grad=True, hess=True)
    with pytest.raises(L.EftbError, match="eftb_draws_logp_hess_params: no draw recipe"):
        like.logp_draws_params(theta, off, f, **kw)
    like.set_draw_recipe(rec)
    lp, gr, want = like.logp_draws_params(theta, off, f, **kw)
    rc, lp_raw, g_raw, h_raw = _raw_hess(eng, theta, off, f)
    assert rc == 0 and np.array_equal(h_raw, want) and np.array_equal(g_raw, gr) and np.array_equal(lp_raw, lp)
    assert _raw_hess(eng, theta, off, f, grad=False)[0] != 0 and "grad == NULL" in eng.lib.eftb_last_error().decode()
    assert _raw_hess(eng, theta, off, f, hess=False)[0] != 0 and "hess == NULL" in eng.lib.eftb_last_error().decode()
    bad = theta.copy()
    bad[1, 2] = np.inf
    with pytest.raises(L.EftbError, match="theta\\[1\\]\\[2\\] is not finite"):
        like.logp_draws_params(bad, off, f, **kw)
    with pytest.raises(L.EftbError, match="offsets"):
        like.logp_draws_params(theta, [0, 2, 5], f, **kw)
    assert np.array_equal(like.logp_draws_params(theta, off, f, **kw)[2], want)
    # singular draw sets: zeroed and duplicated Gaussian rows under a flat prior fail draw by draw, a recipe of row 0 only fails everywhere
    like_f = MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], np.zeros(nG), np.full(nG, np.inf))
    with pytest.raises(L.EftbError, match="no draw recipe"):  # eftb_set_likelihood dropped the recipe and both derivative tables
        like_f.logp_draws_params(theta, off, f, **kw)
    like_f.set_draw_recipe(rec)
    ok_lp, ok_g, ok_h = like_f.logp_draws_params(theta, off, f, **kw)
    # row 3 times theta_2: draws 1 and 2 (theta_2 = 0) have a zeroed Gaussian row; with the terms of row 2 added, a duplicated one
    r3, r2 = rec.row == 3, rec.row == 2
    idx3 = rec.idx.copy()
    assert np.all(idx3[r3, 2] == -1)
    idx3[r3, 2] = 2
    th0 = theta.copy()
    th0[1:3, 2] = 0.0
    sing = np.array([False, True, True, False])
    cat = lambda a, extra: np.concatenate([a, extra])
    for dup in (False, True):
        ex = r2 if dup else np.zeros_like(r2)
        like_f.set_draw_recipe(DrawRecipe(rec.param_names, 1, nG + 1, cat(rec.tracer, rec.tracer[ex]), cat(rec.row, np.full(ex.sum(), 3)), cat(rec.col, rec.col[ex]),
                                          cat(rec.coef, rec.coef[ex]), cat(rec.fpow, rec.fpow[ex]), cat(idx3, rec.idx[ex])))
        rc, lp_raw, g_raw, h_raw = _raw_hess(eng, th0, off, f)
        bad = np.isnan(lp_raw)
        assert rc == 0 and not np.any(bad[~sing]) and (dup or np.all(bad[sing]))  # (duplicated: det F2 is 0 up to rounding, of either sign)
        assert np.all(np.isnan(g_raw[bad])) and np.all(np.isnan(h_raw[bad])) and np.all(np.isfinite(g_raw[~sing])) and np.all(np.isfinite(h_raw[~sing]))
    keep = rec.row == 0
    like_f.set_draw_recipe(DrawRecipe(rec.param_names, 1, nG + 1, rec.tracer[keep], rec.row[keep], rec.col[keep], rec.coef[keep], rec.fpow[keep], rec.idx[keep]))
    with pytest.raises(RuntimeError, match="det of F2ij"):
        like_f.logp_draws_params(theta, off, f, **kw)
    rc, lp_raw, g_raw, h_raw = _raw_hess(eng, theta, off, f)
    assert rc == 0 and np.all(np.isnan(lp_raw)) and np.all(np.isnan(g_raw)) and np.all(np.isnan(h_raw)) and h_raw.shape == (4, 3, 3)
    like_f.set_draw_recipe(rec)
    assert np.array_equal(like_f.logp_draws_params(theta, off, f, **kw)[2], ok_h)
    like = mk()
    like.set_draw_recipe(rec)
    assert np.array_equal(like.logp_draws_params(theta, off, f, **kw)[2], want)
    # a shape whose working set does not fit: 32 parameters against 24 marginalised ones without Jeffreys (2 P nG^2 doubles per wave)
    big = MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], np.zeros(24), np.full(24, 3.0))
    big.set_draw_recipe(DrawRecipe(["p%d" % i for i in range(32)], 1, 25, [0] * 32, list(range(1, 25)) + [0] * 8, [i % 24 for i in range(32)], [1.0] * 32, [0] * 32,
                                   [[i, -1, -1] for i in range(32)]))
    th32 = np.ones((4, 32))
    assert np.all(np.isfinite(big.logp_draws_params(th32, off, f, grad=True)[1]))  # (the gradient call fits)
    with pytest.raises(L.EftbError, match="eftb_draws_logp_hess_params: the Hessian of P = 32 parameters with nG = 24 and J \\+ 1 = 25 columns does not fit the LDS"):
        big.logp_draws_params(th32, off, f, **kw)
    # eftb_set_tracers drops the recipe (and the likelihood)
    eng.set_tracers(1)
    with pytest.raises(L.EftbError, match="eftb_set_likelihood"):
        like.logp_draws_params(theta, off, f, **kw)
    like = mk()
    with pytest.raises(L.EftbError, match="no draw recipe"):
        like.logp_draws_params(theta, off, f, **kw)
    like.set_draw_recipe(rec)
    assert np.array_equal(like.logp_draws_params(theta, off, f, **kw)[2], want)
    like.set_draw_recipe(None)
    with pytest.raises(L.EftbError, match="no draw recipe"):
        like.logp_draws_params(theta, off, f, **kw)
    eng.close()
    # after a direct-P_l run the block holds no templates
    z = 0.7
    cos = synth.cosmology(z=z, Om=0.3, h=0.68)
    DA_AP, H_AP = float(synth.da_func(synth.OM_AP, z)), float(synth.hubble(synth.OM_AP, z))
    eng = Engine(EngineConfig(Nl=3, with_resum=True, with_ap=True, DA_AP=DA_AP, H_AP=H_AP), max_batch=2)
    sc = dict(kmA=0.7, krA=0.25, ndA=4.5e-5)
    bias = np.stack([bias_row(float(cos["f"]), [2.14, 0.55, 0.77, 0.55, -1.84, -1.89, -1.49], None, (0.26, 0.0, -0.93), **sc)] * 2)
    Pin = np.stack([cos["Pin"], 1.1 * cos["Pin"]])
    templ = eng.eval_batch(Pin, cos["f"], cos["DA"], cos["H"])
    nx = templ.shape[-1]
    index = data_index([0, 2], None, nx)[::7].copy()
    model = np.einsum("r,lrx->lx", bias[0], templ[0]).reshape(-1)[index]
    like = MarginalLikelihood(eng, index, 1.02 * model, np.diag(1.0 / (0.05 * np.abs(model) + 10.0) ** 2), np.zeros(7), np.full(7, 3.0))
    like.set_draw_recipe(joint_draw_recipe([WestCoastBasis(prefix="")], gaussian_params(""), [sc]))
    th = np.array([[2.14, 0.55, 0.55], [2.0, 0.5, 0.3]])
    ff = np.full(2, float(cos["f"]))
    assert np.all(np.isfinite(like.logp_draws_params(th, [0, 1, 2], ff, **kw)[2]))
    eng.set_plk_direct(True)
    eng.eval_batch(Pin, cos["f"], cos["DA"], cos["H"], bias=bias, templates=False)
    with pytest.raises(L.EftbError, match="eftb_draws_logp_hess_params: the current block holds no templates"):
        like.logp_draws_params(th, [0, 1, 2], ff, **kw)
    eng.close()


def test_workflow_is_untouched_by_hessian_calls(golden):
    """eval_logp (slow step), the three existing draw calls, staged steps, eval_logp: with Hessian calls in between, every other call gives
    the bits it gives without them"""
    from eftpipe_amd import _lib as L
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe
    from eftpipe_amd.parambasis import WestCoastBasis, gaussian_params, gaussian_rows, gaussian_rows_many

    B = 3
    g, eng, index, nb = _caseC_engine(golden, 16)
    rng = np.random.default_rng(31)
    f0, DA0, H0 = float(g["f"]), float(g["DA"]), float(g["H"])
    sc = dict(kmA=0.7, krA=0.25, ndA=4.5e-5)
    mk = lambda: dict(Pin=g["Pin"][None] * (1.0 + 0.1 * rng.uniform(-1, 1, (B, 1))), f=f0 * (1.0 + 0.03 * rng.uniform(-1, 1, B)),
                      DA=DA0 * (1.0 + 0.02 * rng.uniform(-1, 1, B)), H=H0 * (1.0 + 0.02 * rng.uniform(-1, 1, B)))
    steps = [mk() for _ in range(3)]
    for st in steps:
        st["ng"] = np.stack([[2.0 + 0.1 * rng.uniform(), 0.5, 0.3] for _ in range(B)])
        st["rows"] = np.stack([gaussian_rows(fi, tuple(ng), None, **sc) for fi, ng in zip(st["f"], st["ng"])])
    templ = eng.eval_batch(steps[0]["Pin"], steps[0]["f"], steps[0]["DA"], steps[0]["H"])
    model = np.einsum("r,lrx->lx", steps[0]["rows"][0, 0], templ[0]).reshape(-1)[index]
    sig = 0.05 * np.abs(model) + 10.0
    lk = (model * 1.02, np.diag(1.0 / sig**2), np.zeros(7), np.full(7, 3.0))
    like = MarginalLikelihood(eng, index, *lk)
    like.set_draw_recipe(joint_draw_recipe([WestCoastBasis(prefix="")], gaussian_params(""), [sc]))
    counts = [3, 2, 4]
    off = _offsets(counts)
    first = off[:-1]
    walker = np.repeat(np.arange(3), counts)
    extra = rng.normal(0, 0.1, (sum(counts), 3))

    def sequence(with_hess):
        s0 = steps[0]
        lp0 = like.eval_logp(s0["Pin"], s0["f"], s0["DA"], s0["H"], s0["rows"])
        theta = np.tile([2.0, 0.5, 0.3], (sum(counts), 1)) + extra
        theta[first] = s0["ng"]
        rows = gaussian_rows_many(s0["f"][walker], theta, None, sc["kmA"], sc["krA"], sc["ndA"])
        hs = lambda: like.logp_draws_params(theta, off, s0["f"], grad=True, hess=True) if with_hess else None
        hs()
        lpr = like.logp_draws(rows, off)
        hs()
        lpd = like.logp_draws_params(theta, off, s0["f"])
        hs()
        lpg, gr = like.logp_draws_params(theta, off, s0["f"], grad=True)
        if with_hess:
            lph, gh, he = hs()
            assert np.array_equal(lph, lpd) and np.array_equal(gh, gr) and np.all(np.isfinite(he))
        staged = [r.copy() for r in eng.pipeline(steps[1:], fetch="LOGP")]
        if with_hess:
            with pytest.raises(L.EftbError, match="no templates"):  # a staged step has rotated the blocks
                hs()
        s2 = steps[2]
        return lp0, staged, like.eval_logp(s2["Pin"], s2["f"], s2["DA"], s2["H"], s2["rows"]), lpr, lpd, lpg, gr

    a = sequence(False)
    b = sequence(True)
    assert all(np.array_equal(a[k], b[k]) for k in (0, 2, 3, 4, 5, 6))
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    eng.close()


@pytest.mark.parametrize("jeffreys", [False, True])
def test_maximize_draws_params(golden, jeffreys):
    """the 8 starts of test_draw_hessian.py through the device call: all converge, ln P within 1e-10 |ln P| of the run on the NumPy
    evaluator, the yardstick's Newton decrement at the result <= 10 tol"""
    from eftpipe_amd.marginal import MarginalLikelihood, newton_maximize

    g, eng, T, index = _marg(golden, "auto")
    eng.put("TEMPL", T[None])
    rec, _, _, _, f = _marg_case(g, "auto", [1])
    like = MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], g["auto_loc"], g["auto_scale"], jeffreys=jeffreys)
    like.set_draw_recipe(rec)
    starts, fun, yardstick = newton_problem(jeffreys)
    ref = newton_maximize(fun, starts, tol=TOL)
    theta, logp, grad, hess, n_iter, converged = like.maximize_draws_params(starts, [0, len(starts)], f[:1], tol=TOL)
    print("jeffreys" if jeffreys else "", "iterations", n_iter.tolist(), "on the NumPy evaluator", ref[4].tolist())
    assert np.all(converged) and np.all(ref[5])
    rel = float(np.max(np.abs(logp - ref[1]) / np.abs(ref[1])))
    dec = max(yardstick_decrement(yardstick, t) for t in theta)
    print("jeffreys" if jeffreys else "", "worst |ln P - NumPy run| / |ln P| = %.2e, worst yardstick decrement %.2e" % (rel, dec))
    assert rel < 1e-10
    assert 0.0 <= dec <= 10 * TOL
    # a start where det F2 <= 0 is no error: it stays where it is, unconverged (a recipe of row 0 only)
    keep = rec.row == 0
    from eftpipe_amd.parambasis import DrawRecipe

    flat = MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], np.zeros(7), np.full(7, np.inf))
    flat.set_draw_recipe(DrawRecipe(rec.param_names, 1, 8, rec.tracer[keep], rec.row[keep], rec.col[keep], rec.coef[keep], rec.fpow[keep], rec.idx[keep]))
    out = flat.maximize_draws_params(starts[:2], [0, 2], f[:1])
    assert not np.any(out[5]) and np.array_equal(out[0], starts[:2]) and np.all(np.isnan(out[1]))
    eng.close()
