"""Draw calls fed with EFT parameter values (eftb_draws_logp_params / eftb_draws_reduce_params): the rows are built on the device from a
draw recipe.  Yardsticks: the oracle (oracle/marginal.py) on rows from the existing scalar / many-draw builders, the reference's fixture
values, the LOGP stage, and np.einsum of the scalar bias_row -- with the tolerances test_gpu_draws.py uses for the same quantities."""
import numpy as np
import pytest

import cfg3_util as U
from conftest import relerr
from test_gpu_draws import COUNTS, _caseC_engine, _cfg3_block, _marg, _offsets, _oracle

pytestmark = pytest.mark.gpu


def _marg_case(g, tag, counts, seed=7):
    """recipe, theta [N, P], the builders' rows [N, nG + 1, 24], walker of each draw, f [C] (a growth rate per walker; walker 0: the fixture's)"""
    from eftpipe_amd.marginal import joint_draw_recipe
    from eftpipe_amd.parambasis import WestCoastBasis, gaussian_params, gaussian_rows_many

    co = [float(x) for x in g[tag + "_co"]]
    ng = dict(zip((str(n) for n in g[tag + "_ng_names"]), (float(v) for v in g[tag + "_ng_values"])))
    N, C = int(np.sum(counts)), len(counts)
    rng = np.random.default_rng(seed)
    walker = np.repeat(np.arange(C), counts)
    f = float(g["f"]) * (1.0 + 0.02 * np.arange(C))
    if tag == "auto":
        basis, sc = WestCoastBasis(prefix=""), dict(kmA=co[0], krA=co[1], ndA=co[2])
        rec = joint_draw_recipe([basis], gaussian_params(""), [sc])
        theta = np.array([ng["b1"], ng["b2"], ng["b4"]]) + rng.normal(0.0, 1.0, (N, 3)) * [0.05, 0.3, 0.3]
        theta[0] = [ng["b1"], ng["b2"], ng["b4"]]
        rows = gaussian_rows_many(f[walker], theta, None, *co[:3])
    else:
        basis = WestCoastBasis(prefix="", cross_prefix=["A_", "B_"])
        sc = dict(zip(("kmA", "krA", "ndA", "kmB", "krB", "ndB"), co))
        rec = joint_draw_recipe([basis], gaussian_params("", ("A_", "B_")), [sc])
        p0 = np.array([ng[x + p] for x in ("A_", "B_") for p in ("b1", "b2", "b4")])
        theta = p0 + rng.normal(0.0, 1.0, (N, 6)) * [0.05, 0.3, 0.3, 0.05, 0.3, 0.3]
        theta[0] = p0
        rows = gaussian_rows_many(f[walker], theta[:, :3], theta[:, 3:], *co)
    return rec, theta, rows, walker, f


@pytest.mark.parametrize("tag", ["auto", "cross"])
def test_params_draws_match_oracle_and_fixture(golden, tag):
    from eftpipe_amd.marginal import MarginalLikelihood

    g, eng, T, index = _marg(golden, tag)
    C = len(COUNTS)
    templ = np.stack([T * (1.0 + 0.1 * c) for c in range(C)])
    eng.put("TEMPL", templ)
    rec, theta, rows, walker, f = _marg_case(g, tag, COUNTS)
    assert np.allclose(rec.rows(theta, f[walker])[:, 0], rows, rtol=1e-14, atol=0)
    off = _offsets(COUNTS)
    like = MarginalLikelihood(eng, index, g[tag + "_D"], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"])
    like.set_draw_recipe(rec)
    logp, full, best = like.logp_draws_params(theta, off, f, return_best=True)
    N = theta.shape[0]
    assert logp.shape == full.shape == (N,) and best.shape == (N, len(g[tag + "_loc"]))
    print(tag, "draw 0:", logp[0], g[tag + "_logp"], full[0], g[tag + "_fullchi2"])
    assert np.isclose(logp[0], g[tag + "_logp"], rtol=1e-10) and np.isclose(full[0], g[tag + "_fullchi2"], rtol=1e-9)
    assert relerr(best[0][None], g[tag + "_best"][None]) < 1e-8
    for d in range(N):
        want = _oracle(g, tag, rows[d], templ[walker[d]], index)
        assert np.isclose(logp[d], want[0], rtol=1e-10), d
        assert np.isclose(full[d], want[1], rtol=1e-9), d
        assert relerr(best[d][None], want[2][None]) < 1e-8, d
    assert np.array_equal(like.logp_draws_params(theta, off, f), logp)  # Gram cache, fixed summation order: the same bits
    # the rows path on the builders' rows agrees (different summation order: not the same bits)
    assert np.allclose(like.logp_draws(rows, off), logp, rtol=1e-10, atol=0)
    like_j = MarginalLikelihood(eng, index, g[tag + "_D"], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"], jeffreys=True)
    like_j.set_draw_recipe(rec)
    lj = like_j.logp_draws_params(theta, off, f)
    assert np.isclose(lj[0], g[tag + "_logp_jeffreys"], rtol=1e-10)
    for d in range(N):
        assert np.isclose(lj[d], _oracle(g, tag, rows[d], templ[walker[d]], index, jeffreys=True)[0], rtol=1e-10), d
    if tag == "auto":
        nG = len(g[tag + "_loc"])
        like_f = MarginalLikelihood(eng, index, g[tag + "_D"], g[tag + "_invcov"], np.zeros(nG), np.full(nG, np.inf))
        like_f.set_draw_recipe(rec)
        lf = like_f.logp_draws_params(theta, off, f)
        assert np.isclose(lf[0], g[tag + "_logp_flat"], rtol=1e-9)
        for d in range(N):
            want = _oracle(g, tag, rows[d], templ[walker[d]], index, loc=np.zeros(nG), scale=np.full(nG, np.inf))[0]
            assert np.isclose(lf[d], want, rtol=1e-9), d
    eng.close()


def _cfg3_engine(g, nwalkers, max_batch):
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.marginal import data_index
    from eftpipe_amd.tables import EngineConfig

    block, nb = _cfg3_block(g)
    eng = Engine(EngineConfig(Nl=3), max_batch=max_batch)
    eng.set_tracers(3)
    eng.set_template_dims(3, nb)
    templ = np.concatenate([(1.0 + 0.02 * c) * block for c in range(nwalkers)])
    eng.put("TEMPL", templ)
    index = np.concatenate([data_index([int(l) for l in g[t + "_ls"]], U.masks(g, t), nb, tracer=i, nl=3) for i, t in enumerate(U.TRACERS)])
    return eng, templ, index


def _cfg3_draws(g, counts, seed, spread=0.05):
    """theta [N, 6] (LRG b1 b2 b4, ELG b1 b2 b4; draw 0: the fixture's point), f [C, 3] (walker 0: the fixture's growth rates)"""
    p = U.params(g)
    names = [t + q for t in ("LRG_NGC_", "ELG_NGC_") for q in ("b1", "b2", "b4")]
    N, C = int(np.sum(counts)), len(counts)
    rng = np.random.default_rng(seed)
    theta = np.array([p[n] for n in names]) + spread * rng.normal(size=(N, 6))
    theta[0] = [p[n] for n in names]
    f = np.array([float(g[t + "_f"]) for t in U.TRACERS]) * (1.0 + 0.01 * np.arange(C)[:, None] * [1.0, 2.0, 3.0])
    return names, theta, f


def _cfg3_oracle(g, rows_d, templ, w, index, nG, jeff):
    from oracle import marginal as M

    V = np.concatenate([np.einsum("gr,lrx->glx", rows_d[t], templ[3 * w + t]) for t in range(3)], axis=1).reshape(nG + 1, -1)[:, index]
    return M.marginalized_logp(V[1:], V[0], g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf), jeffreys=jeff, return_best=True)


@pytest.mark.parametrize("tag", ["full", "xnost"])
def test_cfg3_joint_params_draws(golden, tag):
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe, joint_gaussian_rows_many

    g = golden("cfg3")
    counts = [4, 3]
    eng, templ, index = _cfg3_engine(g, 2, 24)
    names = [str(n) for n in g[tag + "_names"]]
    nG = len(names)
    pn, theta, f = _cfg3_draws(g, counts, 9)
    rec = joint_draw_recipe(U.bases(), names, U.scales(g), param_names=pn)
    walker = np.repeat([0, 1], counts)
    rows = joint_gaussian_rows_many(U.bases(), list(f[walker].T), {n: theta[:, i] for i, n in enumerate(pn)}, names, U.scales(g))
    for jeff, key in ((True, "_logp"), (False, "_logp_nojeffreys")):
        like = MarginalLikelihood(eng, index, g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf), jeffreys=jeff)
        like.set_draw_recipe(rec)
        logp, full, best = like.logp_draws_params(theta, _offsets(counts), f, return_best=True)
        print(tag, jeff, "draw 0:", logp[0], g[tag + key])
        assert np.isclose(logp[0], g[tag + key], rtol=1e-9), (logp[0], g[tag + key])
        for d in range(theta.shape[0]):
            want = _cfg3_oracle(g, rows[d], templ, walker[d], index, nG, jeff)
            assert np.isclose(logp[d], want[0], rtol=1e-9), d
            assert np.isclose(full[d], want[1], rtol=1e-8), d
    eng.close()


def test_plain_chi2_params_draws(golden):
    """nG = 0: -chi2 / 2 of the full parameter set through a one-row recipe."""
    from eftpipe_amd.marginal import MarginalLikelihood
    from eftpipe_amd.parambasis import WestCoastBasis, bias_draw_recipe, bias_rows_many

    g, eng, T, index = _marg(golden, "auto", max_batch=4)
    D, Ci = g["auto_D"], g["auto_invcov"]
    like = MarginalLikelihood(eng, index, D, Ci, np.zeros(0), np.zeros(0))
    eng.put("TEMPL", np.stack([T, 1.1 * T]))
    sc = dict(kmA=0.7, krA=0.25, ndA=4.5e-5)
    like.set_draw_recipe(bias_draw_recipe(WestCoastBasis(prefix=""), sc))
    N = 5
    theta = np.tile([2.1, 0.5, 0.3, 0.2, -1.0, -2.0, 0.5, 0.3, 0.1, -0.4], (N, 1)) + 0.1 * np.arange(N)[:, None]
    walker = np.array([0, 0, 1, 1, 1])
    f = np.array([float(g["f"]), 1.03 * float(g["f"])])
    rows = bias_rows_many(f[walker], theta[:, :7], None, theta[:, 7:], **sc)
    logp = like.logp_draws_params(theta, _offsets([2, 3]), f)
    for d in range(N):
        r = np.einsum("r,lrx->lx", rows[d], (1.1 if walker[d] else 1.0) * T).reshape(-1)[index] - D
        assert np.isclose(logp[d], -0.5 * r @ Ci @ r, rtol=1e-10), d
    eng.close()


def test_nnlo_params_draws_match_logp_stage():
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe
    from eftpipe_amd.parambasis import WestCoastBasis, gaussian_params, gaussian_rows_many, nnlo_vector
    from eftpipe_amd.tables import EngineConfig

    rng = np.random.default_rng(4)
    nx, C, counts = 20, 3, [2, 5, 3]
    N = sum(counts)
    eng = Engine(EngineConfig(Nl=3, with_resum=True, with_ap=True, DA_AP=1.0, H_AP=1.0, with_NNLO=True), max_batch=N)
    eng.set_template_dims(3, nx)
    sc = dict(kmA=0.7, krA=0.25, ndA=4.5e-5)
    T = rng.normal(0, 1, (C, 3, 24, nx)) * np.logspace(0, 3, 24)[:, None] / np.array([1.0] * 21 + [1e4, 1e7, 1e7])[:, None]
    TN = rng.normal(0, 1, (C, 3, 24, nx)) * 0.3
    index = np.sort(rng.choice(3 * nx, 40, replace=False)).astype(np.int32)
    D = rng.normal(0, 50, 40)
    Ci = np.diag(1.0 / rng.uniform(5, 20, 40) ** 2)
    basis = WestCoastBasis(prefix="")
    names = gaussian_params("") + basis.cnnloA()
    nG = len(names)
    like = MarginalLikelihood(eng, index, D, Ci, np.zeros(nG), np.full(nG, 2.0))
    like.set_draw_recipe(joint_draw_recipe([basis], names, [sc], with_NNLO=True))
    theta = np.array([2.0, 0.5, 0.3]) + 0.2 * rng.normal(size=(N, 3))
    f = rng.uniform(0.6, 0.9, C)
    walker = np.repeat(np.arange(C), counts)
    rows, rn = np.zeros((N, nG + 1, 24)), np.zeros((N, nG + 1, 3))
    rows[:, :8] = gaussian_rows_many(f[walker], theta, None, **sc)
    for d in range(N):
        rn[d, 8] = nnlo_vector(f[walker[d]], theta[d, 0], (1.0, 0.0), sc["krA"])
        rn[d, 9] = nnlo_vector(f[walker[d]], theta[d, 0], (0.0, 1.0), sc["krA"])
    eng.put("TEMPL", T)
    eng.put("TEMPLN", TN)
    logp = like.logp_draws_params(theta, _offsets(counts), f)
    eng.put("TEMPL", T[walker])
    eng.put("TEMPLN", TN[walker])
    assert np.allclose(logp, like.logp(rows, rows_nnlo=rn), rtol=1e-10, atol=0)
    eng.close()


@pytest.mark.parametrize("kind", ["ap", "ap_stochastic", "nnlo", "tracers"])
def test_reduce_draws_params(kind):
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.parambasis import WestCoastBasis, bias_draw_recipe, bias_row, nnlo_vector
    from eftpipe_amd.tables import EngineConfig

    rng = np.random.default_rng(12)
    nnlo = kind == "nnlo"
    ntr = 2 if kind == "tracers" else 1
    counts = [4, 0, 6]
    C, N, nx = len(counts), sum(counts), 37
    cfg = EngineConfig(Nl=3, with_resum=True, with_ap=True, DA_AP=1.0, H_AP=1.0, with_NNLO=nnlo) if kind != "tracers" else EngineConfig(Nl=3)
    eng = Engine(cfg, max_batch=N * ntr)
    if kind == "ap_stochastic":
        eng.set_ap_stochastic(True)
    if ntr > 1:
        eng.set_tracers(ntr)
    eng.set_template_dims(3, nx)
    T = rng.normal(0, 1, (C * ntr, 3, 24, nx)) * np.logspace(0, 4, 24)[:, None]
    TN = rng.normal(0, 1, (C * ntr, 3, 24, nx)) * 100.0
    eng.put("TEMPL", T)
    if nnlo:
        eng.put("TEMPLN", TN)
    bases = [WestCoastBasis(prefix="T%d_" % t) for t in range(ntr)]
    scales = [dict(kmA=0.7, krA=0.25, ndA=4.5e-5), dict(kmA=0.45, krA=0.35, ndA=3e-4)][:ntr]
    rec = bias_draw_recipe(bases, scales, with_NNLO=nnlo)
    per = 12 if nnlo else 10
    assert len(rec.param_names) == per * ntr
    theta = rng.normal(0.5, 1.0, (N, per * ntr))
    f = rng.uniform(0.6, 0.9, (C, ntr))
    eng.set_reduce_recipe(rec)
    plk = eng.reduce_draws_params(theta, _offsets(counts), f if ntr > 1 else f[:, 0])
    assert plk.shape == ((N, ntr, 3, nx) if ntr > 1 else (N, 3, nx))
    plk = plk.reshape(N, ntr, 3, nx)
    walker = np.repeat(np.arange(C), counts)
    for d in range(N):
        for t in range(ntr):
            th = [float(v) for v in theta[d, per * t : per * (t + 1)]]
            want = np.einsum("r,lrx->lx", bias_row(float(f[walker[d], t]), th[:7], None, th[7:10], **scales[t]), T[walker[d] * ntr + t])
            if nnlo:
                want = want + np.einsum("j,ljx->lx", nnlo_vector(float(f[walker[d], t]), th[0], th[10:12], scales[t]["krA"]), TN[walker[d] * ntr + t][:, 3:6])
            assert relerr(plk[d, t], want) < 1e-13, (d, t)
    # the rows path on the recipe's own rows: the contraction is the same kernel
    rows = rec.rows(theta, f[walker])
    bn = rec.rows_nnlo(theta, f[walker])[:, :, 0] if nnlo else None
    got = eng.reduce_draws(rows[:, :, 0] if ntr > 1 else rows[:, 0, 0], _offsets(counts), bias_nnlo=(bn if ntr > 1 else bn[:, 0]) if nnlo else None)
    assert relerr(got.reshape(N, ntr, 3, nx), plk) < 1e-13
    eng.close()


def test_workflow_slow_step_then_params_draws(golden):
    """eval_logp (slow step) then params draws whose first draw per walker repeats the walker's parameters; put("TEMPL") is seen by the next
    call; after a staged step the call refuses; logp_draws with rows, staged steps and eval_logp give the bits they give without params calls."""
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
    like = MarginalLikelihood(eng, index, model * 1.02, np.diag(1.0 / sig**2), np.zeros(7), np.full(7, 3.0))
    rec = joint_draw_recipe([WestCoastBasis(prefix="")], gaussian_params(""), [sc])
    counts = [3, 2, 4]
    off = _offsets(counts)
    first = off[:-1]
    extra = rng.normal(0, 0.1, (sum(counts), 3))

    def sequence(with_params):
        s0 = steps[0]
        lp0 = like.eval_logp(s0["Pin"], s0["f"], s0["DA"], s0["H"], s0["rows"])
        theta = np.tile([2.0, 0.5, 0.3], (sum(counts), 1)) + extra
        theta[first] = s0["ng"]  # the first draw of each walker repeats the walker's parameters
        rows = gaussian_rows_many(np.repeat(s0["f"], counts), theta, None, **sc)
        lpr = like.logp_draws(rows, off)
        if with_params:
            like.set_draw_recipe(rec)
            lpd = like.logp_draws_params(theta, off, s0["f"])
            assert np.allclose(lpd[first], lp0, rtol=1e-10, atol=0)
            assert np.allclose(lpd, lpr, rtol=1e-10, atol=0)
            assert np.array_equal(like.logp_draws_params(theta, off, s0["f"]), lpd)
            eng.put("TEMPL", 1.05 * templ)  # new templates through put: the next params call sees them
            lpn = like.logp_draws_params(theta, off, s0["f"])
            assert not np.allclose(lpn[first], lp0, rtol=1e-6)
            assert np.allclose(lpn[first], like.logp(s0["rows"]), rtol=1e-10, atol=0)
        staged = [r.copy() for r in eng.pipeline(steps[1:], fetch="LOGP")]
        if with_params:
            with pytest.raises(L.EftbError, match="no templates"):  # a staged step has rotated the blocks
                like.logp_draws_params(theta, off, s0["f"])
        s2 = steps[2]
        return lp0, staged, like.eval_logp(s2["Pin"], s2["f"], s2["DA"], s2["H"], s2["rows"]), lpr

    a = sequence(False)
    b = sequence(True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    eng.close()


def test_params_error_paths(golden):
    import ctypes as C

    from eftpipe_amd import _lib as L
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe
    from eftpipe_amd.parambasis import WestCoastBasis, bias_draw_recipe, gaussian_params

    g, eng, T, index = _marg(golden, "auto", max_batch=4)
    rec, theta, rows, walker, f = _marg_case(g, "auto", [2, 2])
    nG = len(g["auto_loc"])
    eng.put("TEMPL", np.stack([T, T]))
    mk = lambda: MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], g["auto_loc"], g["auto_scale"])
    like = mk()
    off = [0, 2, 4]
    with pytest.raises(L.EftbError, match="no draw recipe"):
        like.logp_draws_params(theta, off, f)
    with pytest.raises(L.EftbError, match="no draw recipe"):
        eng.reduce_draws_params(np.ones((4, 10)), off, f)
    like.set_draw_recipe(rec)
    want = like.logp_draws_params(theta, off, f)
    # a recipe for another nG
    with pytest.raises(ValueError, match="rows"):
        like.set_draw_recipe(joint_draw_recipe([WestCoastBasis(prefix="")], gaussian_params("")[:5], [dict(kmA=0.7, krA=0.25, ndA=4.5e-5)]))
    terms = rec.terms()
    with pytest.raises(L.EftbError, match="ng1"):
        L.check(eng.lib.eftb_set_draw_recipe(eng._h, L.RECIPE_LOGP, 3, nG, terms.size, terms.ctypes.data))
    # terms out of range handed straight to the library
    for field, bad, msg in (("i", 3, "parameter index"), ("k", -2, "parameter index"), ("tracer", 1, "tracer"), ("row", nG + 1, "row"), ("col", 24, "column"),
                            ("fpow", 7, "f\\^7")):
        t2 = terms.copy()
        t2[field][-1] = bad
        with pytest.raises(L.EftbError, match=msg):
            L.check(eng.lib.eftb_set_draw_recipe(eng._h, L.RECIPE_LOGP, 3, nG + 1, t2.size, t2.ctypes.data))
    assert np.array_equal(like.logp_draws_params(theta, off, f), want)  # the refused recipes left the one in place
    # shapes: Python refuses before the library is called
    with pytest.raises(ValueError, match="theta"):
        like.logp_draws_params(theta[:, :2], off, f)
    with pytest.raises(ValueError, match="f must be"):
        like.logp_draws_params(theta, off, np.ones(3))
    with pytest.raises(ValueError, match="offsets"):
        like.logp_draws_params(theta, [4], f)
    bad = theta.copy()
    bad[1, 2] = np.nan
    with pytest.raises(L.EftbError, match="theta\\[1\\]\\[2\\] is not finite"):
        like.logp_draws_params(bad, off, f)
    with pytest.raises(L.EftbError, match="f\\[1\\]\\[0\\] is not finite"):
        like.logp_draws_params(theta, off, np.array([f[0], np.inf]))
    for bo in ([1, 2, 4], [0, 3, 2, 4], [0, 2, 5]):
        with pytest.raises((L.EftbError, ValueError), match="offsets|f must be"):
            like.logp_draws_params(theta, bo, f if len(bo) == 3 else np.ones(3))
    with pytest.raises(L.EftbError, match="entries"):  # three walkers, two template entries
        like.logp_draws_params(theta, [0, 2, 3, 4], np.ones(3))
    assert np.array_equal(like.logp_draws_params(theta, off, f), want)
    # det F2 <= 0 (flat prior, a recipe without derivative rows)
    like_f = MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], np.zeros(nG), np.full(nG, np.inf))
    with pytest.raises(L.EftbError, match="no draw recipe"):  # eftb_set_likelihood dropped it
        like_f.logp_draws_params(theta, off, f)
    row0 = joint_draw_recipe([WestCoastBasis(prefix="")], gaussian_params(""), [dict(kmA=0.7, krA=0.25, ndA=4.5e-5)])
    keep = row0.row == 0
    from eftpipe_amd.parambasis import DrawRecipe

    like_f.set_draw_recipe(DrawRecipe(row0.param_names, 1, nG + 1, row0.tracer[keep], row0.row[keep], row0.col[keep], row0.coef[keep], row0.fpow[keep], row0.idx[keep]))
    with pytest.raises(RuntimeError, match="det of F2ij"):
        like_f.logp_draws_params(theta, off, f)
    # eftb_set_tracers drops both recipes (and the likelihood)
    eng.set_reduce_recipe(bias_draw_recipe(WestCoastBasis(prefix=""), dict(kmA=0.7, krA=0.25, ndA=4.5e-5)))
    eng.reduce_draws_params(np.ones((4, 10)), off, f)
    eng.set_tracers(1)
    with pytest.raises(L.EftbError, match="no draw recipe"):
        eng.reduce_draws_params(np.ones((4, 10)), off, f)
    like = mk()
    like.set_draw_recipe(rec)
    assert np.array_equal(like.logp_draws_params(theta, off, f), want)  # the engine works afterwards
    eng.close()


@pytest.mark.parametrize("shape", ["one_tracer", "cfg3"])
def test_many_params_draws(golden, shape):
    """More draws than one pass of a workgroup's waves, both column-half variants (J + 1 = 25 and 73): a seeded sample against the oracle."""
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe, joint_gaussian_rows_many

    C = 8
    rng = np.random.default_rng(77)
    counts = rng.multinomial(5200, np.ones(C) / C)
    counts[3] += 3000  # one walker owns more draws than a workgroup's share
    N, off = int(counts.sum()), _offsets(counts)
    walker = np.repeat(np.arange(C), counts)
    sample = np.sort(rng.choice(N, 200, replace=False))
    if shape == "one_tracer":
        g, eng, T, index = _marg(golden, "auto")
        templ = np.stack([T * (1.0 + 0.1 * c) for c in range(C)])
        eng.put("TEMPL", templ)
        rec, theta, rows, walker, f = _marg_case(g, "auto", counts, seed=78)
        like = MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], g["auto_loc"], g["auto_scale"])
        like.set_draw_recipe(rec)
        logp, full, best = like.logp_draws_params(theta, off, f, return_best=True)
        assert np.all(np.isfinite(logp)) and np.all(np.isfinite(full)) and np.all(np.isfinite(best))
        for d in sample:
            want = _oracle(g, "auto", rows[d], templ[walker[d]], index)
            assert np.isclose(logp[d], want[0], rtol=1e-10), d
            assert np.isclose(full[d], want[1], rtol=1e-9), d
            assert relerr(best[d][None], want[2][None]) < 1e-8, d
    else:
        g = golden("cfg3")
        eng, templ, index = _cfg3_engine(g, C, 3 * C)
        names = [str(n) for n in g["full_names"]]
        nG = len(names)
        pn, theta, f = _cfg3_draws(g, counts, 79)
        like = MarginalLikelihood(eng, index, g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf), jeffreys=True)
        like.set_draw_recipe(joint_draw_recipe(U.bases(), names, U.scales(g), param_names=pn))
        logp, full, best = like.logp_draws_params(theta, off, f, return_best=True)
        assert np.all(np.isfinite(logp)) and np.all(np.isfinite(full)) and np.all(np.isfinite(best))
        rows = joint_gaussian_rows_many(U.bases(), list(f[walker[sample]].T), {n: theta[sample, i] for i, n in enumerate(pn)}, names, U.scales(g))
        for q, d in enumerate(sample):
            want = _cfg3_oracle(g, rows[q], templ, walker[d], index, nG, True)
            assert np.isclose(logp[d], want[0], rtol=1e-9), d
            assert np.isclose(full[d], want[1], rtol=1e-8), d
    eng.close()
