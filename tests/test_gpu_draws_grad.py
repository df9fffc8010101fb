"""d ln P / d theta of the params draws on the device (eftb_draws_logp_grad_params; MarginalLikelihood.logp_draws_params(grad=True)).
Yardstick: the data-space adjoint of grad_util.py (the oracle's b and F2, dV / d theta from DrawRecipe.jacobian; pinned on the host
against Richardson differences of the oracle by test_draw_gradient.py), draw for draw, at 1e-10 of the component's magnitude
mag_p = 1/2 sum |Rbar_V . dV_p| -- the bar test_gpu_draws*.py hold ln P of the same draws to.  The NumPy restatement of the kernel's
Gram-space route sits at 1.5e-13 of that magnitude (test_draw_gradient.py), a factor 700 under the bar.  ln P, full chi2 and the best fit
of the gradient call are the bits of the call without it."""
import ctypes as C

import numpy as np
import pytest

import cfg3_util as U
import grad_util as GU
from test_gpu_draws import COUNTS, _caseC_engine, _marg, _offsets
from test_gpu_draws_params import _cfg3_draws, _cfg3_engine, _marg_case

pytestmark = pytest.mark.gpu

BAR = 1e-10


def _check(tag, like, rec, theta, off, f, walker, templ, index, lk, jeffreys, templn=None, ntr=1):
    """the gradient call against the yardstick and against the call without the gradient; -> grad, worst error / mag"""
    want = like.logp_draws_params(theta, off, f, return_best=True)
    logp, grad, full, best = like.logp_draws_params(theta, off, f, return_best=True, grad=True)
    assert grad.shape == theta.shape and np.all(np.isfinite(grad))
    for a, b in zip((logp, full, best), want):
        assert np.array_equal(a, b)
    lp2, g2 = like.logp_draws_params(theta, off, f, grad=True)
    assert np.array_equal(g2, grad) and np.array_equal(lp2, logp)  # a repeat call: the same bits
    worst = 0.0
    for d in range(theta.shape[0]):
        w = walker[d]
        lp, g, mag = GU.adjoint_of_draw(rec, theta[d], np.reshape(f, (len(off) - 1, ntr))[w], templ[w * ntr : (w + 1) * ntr], index, *lk, jeffreys=jeffreys,
                                        templn=None if templn is None else templn[w * ntr : (w + 1) * ntr])
        assert np.isclose(logp[d], lp, rtol=1e-9)
        worst = max(worst, float(np.max(np.abs(grad[d] - g) / mag)))
    print(tag, "jeffreys" if jeffreys else "", "worst |grad - adjoint| / mag = %.2e" % worst)
    assert worst < BAR, (tag, jeffreys, worst)
    return grad, worst


@pytest.mark.parametrize("tag", ["auto", "cross"])
def test_grad_matches_data_space_adjoint(golden, tag):
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
    grads = []
    for lo, sc, jeff in priors:  # (flat prior: auto only, the cross fixture's 11 parameters are degenerate without one)
        like = MarginalLikelihood(eng, index, D, Ci, lo, sc, jeffreys=jeff)
        like.set_draw_recipe(rec)
        grads.append(_check(tag, like, rec, theta, off, f, walker, templ, index, (D, Ci, lo, sc), jeff)[0])
    assert not np.allclose(grads[0], grads[1], rtol=1e-6)  # the trace term is there
    eng.close()


@pytest.mark.parametrize("tag", ["full", "xnost"])
def test_cfg3_joint_grad(golden, tag):
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe

    g = golden("cfg3")
    counts = [4, 3]
    eng, templ, index = _cfg3_engine(g, 2, 24)
    names = [str(n) for n in g[tag + "_names"]]
    nG = len(names)
    pn, theta, f = _cfg3_draws(g, counts, 9)
    rec = joint_draw_recipe(U.bases(), names, U.scales(g), param_names=pn)
    walker = np.repeat([0, 1], counts)
    lk = (g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf))
    for jeff in (True, False):
        like = MarginalLikelihood(eng, index, *lk, jeffreys=jeff)
        like.set_draw_recipe(rec)
        _check("cfg3 " + tag, like, rec, theta, _offsets(counts), f, walker, templ, index, lk, jeff, ntr=3)
    eng.close()


def _nnlo_problem():
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.marginal import joint_draw_recipe
    from eftpipe_amd.parambasis import WestCoastBasis, gaussian_params
    from eftpipe_amd.tables import EngineConfig

    rng = np.random.default_rng(4)
    nx, nC, counts = 20, 3, [2, 5, 3]
    N = sum(counts)
    eng = Engine(EngineConfig(Nl=3, with_resum=True, with_ap=True, DA_AP=1.0, H_AP=1.0, with_NNLO=True), max_batch=N)
    eng.set_template_dims(3, nx)
    sc = dict(kmA=0.7, krA=0.25, ndA=4.5e-5)
    T = rng.normal(0, 1, (nC, 3, 24, nx)) * np.logspace(0, 3, 24)[:, None] / np.array([1.0] * 21 + [1e4, 1e7, 1e7])[:, None]
    TN = rng.normal(0, 1, (nC, 3, 24, nx)) * 0.3
    index = np.sort(rng.choice(3 * nx, 40, replace=False)).astype(np.int32)
    D = rng.normal(0, 50, 40)
    Ci = np.diag(1.0 / rng.uniform(5, 20, 40) ** 2)
    basis = WestCoastBasis(prefix="")
    names = gaussian_params("") + basis.cnnloA()
    rec = joint_draw_recipe([basis], names, [sc], with_NNLO=True)
    theta = np.array([2.0, 0.5, 0.3]) + 0.2 * rng.normal(size=(N, 3))
    f = rng.uniform(0.6, 0.9, nC)
    eng.put("TEMPL", T)
    eng.put("TEMPLN", TN)
    return eng, rec, theta, f, counts, T, TN, index, D, Ci, len(names)


def test_nnlo_grad():
    from eftpipe_amd.marginal import MarginalLikelihood

    eng, rec, theta, f, counts, T, TN, index, D, Ci, nG = _nnlo_problem()
    walker = np.repeat(np.arange(len(counts)), counts)
    for jeff in (False, True):
        lk = (D, Ci, np.zeros(nG), np.full(nG, 2.0))
        like = MarginalLikelihood(eng, index, *lk, jeffreys=jeff)
        like.set_draw_recipe(rec)
        grad, _ = _check("nnlo", like, rec, theta, _offsets(counts), f, walker, T, index, lk, jeff, templn=TN)
        assert np.all(np.abs(grad[:, 0]) > 0)
    eng.close()


def test_split_calls_single_draws_and_empty_walkers(golden):
    """one batch of draws submitted whole, and split into two calls with other offsets, gives the same bits per draw; so do draws sent
    one at a time; walkers without draws and N = 0 are in order"""
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe

    g = golden("cfg3")
    nC = 4
    rng = np.random.default_rng(5)
    counts = np.array([700, 0, 37, 1500])  # (more draws than one pass of a workgroup's waves)
    eng, templ, index = _cfg3_engine(g, nC, 3 * nC)
    names = [str(n) for n in g["full_names"]]
    nG = len(names)
    pn, theta, f = _cfg3_draws(g, counts, 79)
    rec = joint_draw_recipe(U.bases(), names, U.scales(g), param_names=pn)
    like = MarginalLikelihood(eng, index, g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf))
    like.set_draw_recipe(rec)
    off = _offsets(counts)
    logp, grad, full, best = like.logp_draws_params(theta, off, f, return_best=True, grad=True)
    assert np.all(np.isfinite(grad)) and np.array_equal(logp, like.logp_draws_params(theta, off, f))
    # the same draws in two calls: every walker's draws cut at a random place
    cut = np.array([rng.integers(0, c + 1) for c in counts])
    sel_a = np.concatenate([np.arange(off[c], off[c] + cut[c]) for c in range(nC)])
    sel_b = np.concatenate([np.arange(off[c] + cut[c], off[c + 1]) for c in range(nC)])
    for sel, cnt in ((sel_a, cut), (sel_b, counts - cut)):
        lp, gr, fu, be = like.logp_draws_params(theta[sel], _offsets(cnt), f, return_best=True, grad=True)
        assert np.array_equal(gr, grad[sel]) and np.array_equal(lp, logp[sel]) and np.array_equal(fu, full[sel]) and np.array_equal(be, best[sel])
    # one draw, of the last walker alone (walkers 0 ... 2 own none)
    d = int(off[3]) + 11
    lp, gr = like.logp_draws_params(theta[d : d + 1], [0, 0, 0, 0, 1], f, grad=True)
    assert gr.shape == (1, 6) and np.array_equal(gr[0], grad[d]) and lp[0] == logp[d]
    # N = 0
    lp, gr = like.logp_draws_params(np.zeros((0, 6)), [0, 0, 0, 0, 0], f, grad=True)
    assert lp.shape == (0,) and gr.shape == (0, 6)
    # a sample against the yardstick
    walker = np.repeat(np.arange(nC), counts)
    worst = 0.0
    for d in np.sort(rng.choice(theta.shape[0], 24, replace=False)):
        w = walker[d]
        _, gw, mag = GU.adjoint_of_draw(rec, theta[d], f[w], templ[3 * w : 3 * w + 3], index, g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf))
        worst = max(worst, float(np.max(np.abs(grad[d] - gw) / mag)))
    print("cfg3 full, many draws: worst |grad - adjoint| / mag = %.2e" % worst)
    assert worst < BAR
    eng.close()


def _raw_grad(eng, theta, off, f, grad=True):
    """the library call itself (the Python wrapper raises where ln P is NaN) -> rc, logp, grad"""
    theta, off, f = np.ascontiguousarray(theta, dtype=np.float64), np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(f, dtype=np.float64)
    N, P = theta.shape
    logp, gr = np.zeros(N), np.zeros((N, P))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = eng.lib.eftb_draws_logp_grad_params(eng._h, off.size - 1, N, off.ctypes.data_as(C.POINTER(C.c_int64)), dp(theta), dp(f), dp(logp), dp(gr) if grad else None,
                                             None, None)
    return rc, logp, gr


def test_grad_refusals_and_nan_rows(golden):
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
    with pytest.raises(L.EftbError, match="eftb_draws_logp_grad_params: no draw recipe"):
        like.logp_draws_params(theta, off, f, grad=True)
    like.set_draw_recipe(rec)
    lp, want = like.logp_draws_params(theta, off, f, grad=True)
    rc, lp_raw, g_raw = _raw_grad(eng, theta, off, f)
    assert rc == 0 and np.array_equal(g_raw, want) and np.array_equal(lp_raw, lp)
    assert _raw_grad(eng, theta, off, f, grad=False)[0] != 0 and "grad == NULL" in eng.lib.eftb_last_error().decode()
    bad = theta.copy()
    bad[1, 2] = np.inf
    with pytest.raises(L.EftbError, match="theta\\[1\\]\\[2\\] is not finite"):
        like.logp_draws_params(bad, off, f, grad=True)
    with pytest.raises(L.EftbError, match="f\\[1\\]\\[0\\] is not finite"):
        like.logp_draws_params(theta, off, np.array([f[0], np.nan]), grad=True)
    with pytest.raises(L.EftbError, match="offsets"):
        like.logp_draws_params(theta, [0, 2, 5], f, grad=True)
    with pytest.raises(ValueError, match="theta"):
        like.logp_draws_params(theta[:, :2], off, f, grad=True)
    assert np.array_equal(like.logp_draws_params(theta, off, f, grad=True)[1], want)
    # det F2 <= 0 (flat prior, a recipe without derivative rows): an all-NaN row, as ln P; the likelihood beside it is unaffected afterwards
    like_f = MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], np.zeros(nG), np.full(nG, np.inf))
    with pytest.raises(L.EftbError, match="no draw recipe"):  # eftb_set_likelihood dropped the recipe, and the derivative table with it
        like_f.logp_draws_params(theta, off, f, grad=True)
    keep = rec.row == 0
    like_f.set_draw_recipe(DrawRecipe(rec.param_names, 1, nG + 1, rec.tracer[keep], rec.row[keep], rec.col[keep], rec.coef[keep], rec.fpow[keep], rec.idx[keep]))
    with pytest.raises(RuntimeError, match="det of F2ij"):
        like_f.logp_draws_params(theta, off, f, grad=True)
    rc, lp_raw, g_raw = _raw_grad(eng, theta, off, f)
    assert rc == 0 and np.all(np.isnan(lp_raw)) and np.all(np.isnan(g_raw)) and g_raw.shape == (4, 3)
    like = mk()
    like.set_draw_recipe(rec)
    assert np.array_equal(like.logp_draws_params(theta, off, f, grad=True)[1], want)
    # eftb_set_tracers drops the recipe (and the likelihood)
    eng.set_tracers(1)
    with pytest.raises(L.EftbError, match="eftb_set_likelihood"):
        like.logp_draws_params(theta, off, f, grad=True)
    like = mk()
    with pytest.raises(L.EftbError, match="no draw recipe"):
        like.logp_draws_params(theta, off, f, grad=True)
    like.set_draw_recipe(rec)
    assert np.array_equal(like.logp_draws_params(theta, off, f, grad=True)[1], want)  # the engine works afterwards
    like.set_draw_recipe(None)  # withdrawn
    with pytest.raises(L.EftbError, match="no draw recipe"):
        like.logp_draws_params(theta, off, f, grad=True)
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
    lp, gr = like.logp_draws_params(th, [0, 1, 2], ff, grad=True)
    assert np.all(np.isfinite(gr))
    eng.set_plk_direct(True)
    eng.eval_batch(Pin, cos["f"], cos["DA"], cos["H"], bias=bias, templates=False)
    with pytest.raises(L.EftbError, match="eftb_draws_logp_grad_params: the current block holds no templates"):
        like.logp_draws_params(th, [0, 1, 2], ff, grad=True)
    eng.close()


def test_workflow_is_untouched_by_gradient_calls(golden):
    """eval_logp (slow step), draws, staged steps, eval_logp: with gradient calls in between, every other call gives the bits it gives
    without them"""
    from eftpipe_amd import _lib as L
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe
    from eftpipe_amd.parambasis import WestCoastBasis, gaussian_params, gaussian_rows

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
    rec = joint_draw_recipe([WestCoastBasis(prefix="")], gaussian_params(""), [sc])
    like.set_draw_recipe(rec)
    counts = [3, 2, 4]
    off = _offsets(counts)
    first = off[:-1]
    extra = rng.normal(0, 0.1, (sum(counts), 3))

    def sequence(with_grad):
        s0 = steps[0]
        lp0 = like.eval_logp(s0["Pin"], s0["f"], s0["DA"], s0["H"], s0["rows"])
        theta = np.tile([2.0, 0.5, 0.3], (sum(counts), 1)) + extra
        theta[first] = s0["ng"]
        lpd = like.logp_draws_params(theta, off, s0["f"])
        if with_grad:
            lpg, gr = like.logp_draws_params(theta, off, s0["f"], grad=True)
            assert np.array_equal(lpg, lpd) and np.allclose(lpg[first], lp0, rtol=1e-10, atol=0)
            assert np.all(np.isfinite(gr))
            assert np.array_equal(like.logp_draws_params(theta, off, s0["f"]), lpd)
        staged = [r.copy() for r in eng.pipeline(steps[1:], fetch="LOGP")]
        if with_grad:
            with pytest.raises(L.EftbError, match="no templates"):  # a staged step has rotated the blocks
                like.logp_draws_params(theta, off, s0["f"], grad=True)
        s2 = steps[2]
        return lp0, staged, like.eval_logp(s2["Pin"], s2["f"], s2["DA"], s2["H"], s2["rows"]), lpd

    a = sequence(False)
    b = sequence(True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    eng.close()
