"""d2 ln P / d theta d theta of the params draws on the host (no GPU): the second derivative of a draw recipe (DrawRecipe.second_derivative /
hessian) against stencils of DrawRecipe.jacobian, the data-space Hessian (hess_util.data_space_hessian, the yardstick of the GPU tests)
against Richardson differences of the data-space adjoint the parent already pins (grad_util.adjoint_of_draw), the kernel's Gram-space
route restated in NumPy (hess_util.gram_hessian) against that yardstick, and the Newton ascent built on it (marginal.newton_maximize).

Stencil.  The entries of the jacobian are quadratic in theta at most, so the five-point stencil is exact for any h and what remains is the
rounding of ``jacobian`` at the four points; steps and draws as test_draw_gradient.py (h the power of two next to |theta_q|, |theta| in
[0.5, 2.5] with both signs).  Bar: 64 unit roundoffs of hessian_magnitude, the bar ``jacobian`` is held to.  Measured: 1.0 (west auto,
west cross, NNLO: the second derivatives there are single monomials), 42 (east coast)."""
import numpy as np
import pytest

import grad_util as GU
import hess_util as HU
from conftest import load_golden
from test_draw_gradient import N, _cfg3_problem, _marg_problem, _recipe


@pytest.mark.parametrize("case", ["west_auto", "west_cross", "east", "nnlo"])
def test_hessian_matches_stencil_of_jacobian(case):
    rec = _recipe(case)
    P = len(rec.param_names)
    rng = np.random.default_rng(21)
    theta = rng.uniform(0.5, 2.5, (N, P)) * rng.choice([-1.0, 1.0], (N, P))
    f = rng.uniform(0.6, 0.9, (N, rec.ntr))
    u = 2.0**-53
    worst = 0.0
    for fun, hes, mag in ((rec.jacobian, rec.hessian(theta, f), rec.hessian_magnitude(theta, f)),) + (
            ((rec.jacobian_nnlo, rec.hessian_nnlo(theta, f), rec._hess(theta, f, 24, 27, magnitude=True)),) if rec.has_nnlo else ()):
        assert hes.shape == fun(theta, f).shape + (P,) and mag.shape == hes.shape
        assert np.count_nonzero(hes) > 0 and np.all(np.abs(hes) <= mag * (1 + 8 * u))
        assert np.array_equal(hes, hes.swapaxes(-1, -2))
        for q in range(P):
            h = 2.0 ** np.round(np.log2(np.abs(theta[:, q])))
            r = []
            for k in (2.0, 1.0, -1.0, -2.0):
                t = theta.copy()
                t[:, q] += k * h
                r.append(fun(t, f))
            fd = (8.0 * (r[1] - r[2]) - (r[0] - r[3])) / (12.0 * h)[:, None, None, None, None]
            err = np.abs(fd - hes[..., q])
            m = mag[..., q]
            flat = m == 0.0  # no record: the jacobian's entry does not move with theta_q at all
            assert np.all(hes[..., q][flat] == 0.0) and all(np.array_equal(r[0][flat], x[flat]) for x in r[1:])
            worst = max(worst, float(np.max(err / np.where(flat, 1.0, m))) / u)
            assert np.all(err <= 64 * u * m), (case, q, worst)
    print(case, "worst |stencil - hessian| in unit roundoffs of hessian_magnitude: %.1f" % worst)


def test_second_derivative_records():
    from eftpipe_amd.parambasis import DrawRecipe

    # entry (0, 0, 0): 3 f a a b - 2 a + 5;  entry (0, 1, 2): b b b
    rec = DrawRecipe(["a", "b"], 1, 2, [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 2], [3.0, -2.0, 5.0, 1.0], [1, 0, 0, 0],
                     [[0, 0, 1], [0, -1, -1], [-1, -1, -1], [1, 1, 1]])
    d = rec.second_derivative()
    got = [(int(x["p"]), int(x["q"]), int(x["row"]), int(x["col"]), float(x["coef"]), int(x["fpow"]), int(x["idx"][0])) for x in d]
    assert got == [(0, 0, 0, 0, 6.0, 1, 1), (0, 1, 0, 0, 6.0, 1, 0), (1, 1, 1, 2, 6.0, 0, 1)]
    h = rec.hessian(np.array([[2.0, 3.0]]), np.array([0.5]))
    assert h.shape == (1, 1, 2, 24, 2, 2)
    assert h[0, 0, 0, 0, 0, 0] == 6.0 * 0.5 * 3.0 and h[0, 0, 0, 0, 0, 1] == 6.0 * 0.5 * 2.0 == h[0, 0, 0, 0, 1, 0] and h[0, 0, 1, 2, 1, 1] == 18.0
    assert np.count_nonzero(h) == 4


@pytest.mark.parametrize("case", ["west_cross", "cfg3_joint", "nnlo"])
def test_second_derivative_is_order_independent(case):
    """a shuffled term list, with the indices of every term permuted, gives the same table, sorted by (p, q, entry, parent term)"""
    from eftpipe_amd.parambasis import DrawRecipe

    rec = _recipe(case)
    rng = np.random.default_rng(3)
    want = rec.second_derivative()
    assert want.size > 0
    entry = (want["row"].astype(np.int64) * rec.ntr + want["tracer"]) * 32 + want["col"]
    key = list(zip(want["p"].tolist(), want["q"].tolist(), entry.tolist()))
    assert key == sorted(key) and np.all(want["p"] <= want["q"])
    for _ in range(3):
        o = rng.permutation(rec.nterms)
        idx = np.stack([rng.permutation(r) for r in rec.idx[o]])
        got = DrawRecipe(rec.param_names, rec.ntr, rec.ng1, rec.tracer[o], rec.row[o], rec.col[o], rec.coef[o], rec.fpow[o], idx).second_derivative()
        assert got.tobytes() == want.tobytes()
    dup = lambda o: DrawRecipe(["a"], 1, 1, [0, 0], [0, 0], [0, 0], np.array([2.0, -1.0])[o], [0, 0], [[0, 0, -1]] * 2).second_derivative()
    assert dup([0, 1]).tobytes() == dup([1, 0]).tobytes() and list(dup([0, 1])["coef"]) == [-2.0, 4.0]


# ----------------------------------------------------------------------------- the yardstick against differences of the pinned adjoint
def _problem(tag):
    return _marg_problem(tag) if tag in ("auto", "cross") else _cfg3_problem(tag)


# Richardson differences (h = 2e-3 max(1, |theta_q|), one step) of the data-space adjoint's gradient against the data-space Hessian, worst
# |fd - hess| / mag over 12 draws.  Measured floor of that difference, Jeffreys off / on: FD_FLOOR below; the bar is 30 times the
# floor, as DESIGN 10.2 did for the gradient: the excess is the finite difference's own error, which moves with the draw.
FD_FLOOR = {("auto", False): 3.4e-12, ("auto", True): 3.4e-12, ("cross", False): 4.9e-12, ("cross", True): 4.9e-12,
            ("full", False): 1.2e-11, ("full", True): 1.9e-11, ("xnost", False): 7.1e-12, ("xnost", True): 7.8e-12}
# (bars: 1.0e-10, 1.5e-10, 3.6e-10 / 5.7e-10, 2.1e-10 / 2.3e-10; the yardstick's own two triangles differ by 1.2e-13 (auto), 1.0e-12 (cross),
# 4.3e-12 (full) and 1.0e-12 (xnost) of mag: F2 of the flat-prior cfg 3 likelihoods is ill-conditioned and K = F2^-1 enters squared)


@pytest.mark.parametrize("jeffreys", [False, True])
@pytest.mark.parametrize("tag", ["auto", "cross", "full", "xnost"])
def test_hessian_matches_richardson_differences_of_the_adjoint(tag, jeffreys):
    rec, theta, f, templ, index, like = _problem(tag)
    worst = asym = 0.0
    for th, ff in zip(theta, f):
        _, hess, mag = HU.hessian_of_draw(rec, th, ff, templ, index, *like, jeffreys=jeffreys)
        fd = HU.richardson_hess(lambda t: GU.adjoint_of_draw(rec, t, ff, templ, index, *like, jeffreys=jeffreys)[1], th)
        worst = max(worst, float(np.max(np.abs(fd - hess) / mag)))
        asym = max(asym, float(np.max(np.abs(hess - hess.T) / mag)))
    print(tag, "jeffreys" if jeffreys else "", "worst |fd - hess| / mag = %.2e, asymmetry of the yardstick %.2e" % (worst, asym))
    assert asym < 1e-10  # (its two triangles are rounded differently; the bar every route here is held to)
    assert worst < 30 * FD_FLOOR[(tag, jeffreys)]


# ----------------------------------------------------------------------------- the kernel's Gram-space route in NumPy
@pytest.mark.parametrize("jeffreys", [False, True])
@pytest.mark.parametrize("tag", ["auto", "cross", "full", "xnost"])
def test_gram_route_matches_data_space_hessian(tag, jeffreys):
    """the rounding floor of the Gram route; bar: 1e-10 of the entry's magnitude, the project's bar for the Gram route.  Measured, Jeffreys
    on and off alike: 1.1e-13 (auto), 1.5e-12 (cross), 9.7e-12 (full), 9.7e-13 (xnost) -- hess_util.GRAM_FLOOR, from which the GPU tests
    take their bar"""
    rec, theta, f, templ, index, like = _problem(tag)
    W = GU.gram_matrix(templ, index, like[0], like[1])
    worst = worst_g = 0.0
    for th, ff in zip(theta, f):
        lp, hess, mag = HU.hessian_of_draw(rec, th, ff, templ, index, *like, jeffreys=jeffreys)
        _, grad, gmag = GU.adjoint_of_draw(rec, th, ff, templ, index, *like, jeffreys=jeffreys)
        lpg, gg, hg = HU.gram_hessian(rec, th, ff, W, like[2], like[3], jeffreys=jeffreys)
        assert np.array_equal(hg, hg.T)
        lpa, ga = GU.gram_adjoint(rec, th, ff, W, like[2], like[3], jeffreys=jeffreys)
        assert np.isclose(lpg, lpa, rtol=1e-12, atol=0) and np.allclose(gg, ga, rtol=0, atol=1e-12 * np.max(gmag))
        assert abs(lpg - lp) < 1e-10 * abs(lp)
        worst = max(worst, float(np.max(np.abs(hg - hess) / mag)))
        worst_g = max(worst_g, float(np.max(np.abs(gg - grad) / gmag)))
    print(tag, "jeffreys" if jeffreys else "", "Gram route: worst |hess - yardstick| / mag = %.2e (gradient %.2e)" % (worst, worst_g))
    assert worst < 1e-10 and worst_g < 1e-10
    assert worst <= 1.5 * HU.GRAM_FLOOR[tag]  # (the recorded floor the device bars are taken from; 1.5: another NumPy / BLAS rounds differently)


# ----------------------------------------------------------------------------- Newton ascent on the NumPy evaluator
TOL = 1e-8


def newton_problem(jeffreys, nstart=8):
    """marg.npz auto: the starts (the fixture's parameters scaled by seeded factors in [0.9, 1.1]), the NumPy evaluator of the Gram route as
    ``fun`` and the yardstick's (ln P, grad, hess) at one point"""
    g = load_golden("marg")
    rec, theta, f, templ, index, like = _marg_problem("auto", 1)
    ff = f[0]
    W = GU.gram_matrix(templ, index, like[0], like[1])
    rng = np.random.default_rng(17)
    ng = dict(zip((str(n) for n in g["auto_ng_names"]), (float(v) for v in g["auto_ng_values"])))
    starts = np.array([ng["b1"], ng["b2"], ng["b4"]]) * rng.uniform(0.9, 1.1, (nstart, 3))

    def fun(th):
        out = [HU.gram_hessian(rec, t, ff, W, like[2], like[3], jeffreys=jeffreys) for t in th]
        return np.array([o[0] for o in out]), np.stack([o[1] for o in out]), np.stack([o[2] for o in out])

    def yardstick(t):
        lp, grad, _ = GU.adjoint_of_draw(rec, t, ff, templ, index, *like, jeffreys=jeffreys)
        return lp, grad, HU.hessian_of_draw(rec, t, ff, templ, index, *like, jeffreys=jeffreys)[1]

    return starts, fun, yardstick


def yardstick_decrement(yardstick, t):
    _, g, H = yardstick(t)
    return float(g @ np.linalg.solve(-H, g))


@pytest.mark.parametrize("jeffreys", [False, True])
def test_newton_maximize_reaches_the_best_fit(jeffreys):
    from scipy.optimize import minimize

    from eftpipe_amd.marginal import newton_maximize

    starts, fun, yardstick = newton_problem(jeffreys)
    theta, logp, grad, hess, n_iter, converged = newton_maximize(fun, starts, tol=TOL)
    assert theta.shape == starts.shape and hess.shape == (8, 3, 3) and converged.dtype == bool
    print("jeffreys" if jeffreys else "", "iterations", n_iter.tolist())
    assert np.all(converged)
    lp2, g2, h2 = fun(theta)
    assert np.array_equal(lp2, logp) and np.array_equal(g2, grad) and np.array_equal(h2, hess)  # what it returns belongs to theta
    worst = 0.0
    for t0, t, lp in zip(starts, theta, logp):
        dec = yardstick_decrement(yardstick, t)
        worst = max(worst, dec)
        assert 0.0 <= dec <= 10 * TOL  # (10: the two routes differ in rounding)
        res = minimize(lambda x: -yardstick(x)[0], t0, jac=lambda x: -yardstick(x)[1], method="BFGS")
        assert lp >= -res.fun - 1e-10 * abs(lp), (lp, -res.fun)
    print("jeffreys" if jeffreys else "", "worst Newton decrement of the yardstick at the result: %.2e" % worst)


def test_newton_maximize_leaves_nan_points_alone():
    """a start whose first trial gives NaN keeps its point and ends unconverged; so does a start that is NaN itself; the others converge
    as they do without them"""
    from eftpipe_amd.marginal import newton_maximize

    starts, fun, _ = newton_problem(False, 4)
    want = newton_maximize(fun, starts, tol=TOL)

    def holed(th):
        lp, g, H = fun(th)
        moved = np.any(th[1] != starts[1])
        if moved:  # every trial of point 1
            lp[1], g[1], H[1] = np.nan, np.nan, np.nan
        lp[3], g[3], H[3] = np.nan, np.nan, np.nan  # point 3: NaN from the start
        return lp, g, H

    theta, logp, grad, hess, n_iter, converged = newton_maximize(holed, starts, max_iter=12, tol=TOL)
    assert converged.tolist() == [True, False, True, False]
    assert np.array_equal(theta[1], starts[1]) and np.array_equal(theta[3], starts[3])
    assert np.isfinite(logp[1]) and np.isnan(logp[3]) and n_iter[3] == 0 and 1 <= n_iter[1] <= 12
    for k in (0, 2):
        assert np.array_equal(theta[k], want[0][k]) and logp[k] == want[1][k] and n_iter[k] == want[4][k]


def test_newton_maximize_on_a_saddle_and_a_quadratic():
    """-H indefinite at the start: the damping carries the point to the maximum; an exact quadratic takes one step and the confirming one"""
    from eftpipe_amd.marginal import newton_maximize

    def fun(th):  # ln P = -(x^2 - 1)^2 - y^2: maxima at x = +-1, a saddle at 0
        x, y = th[:, 0], th[:, 1]
        lp = -((x * x - 1.0) ** 2) - y * y
        g = np.stack([-4.0 * x * (x * x - 1.0), -2.0 * y], axis=1)
        H = np.zeros((th.shape[0], 2, 2))
        H[:, 0, 0], H[:, 1, 1] = -12.0 * x * x + 4.0, -2.0
        return lp, g, H

    theta, logp, _, _, _, conv = newton_maximize(fun, np.array([[0.2, 0.5], [-0.3, 1.0], [1.5, -2.0]]))
    assert np.all(conv) and np.allclose(np.abs(theta[:, 0]), 1.0, atol=1e-5) and np.allclose(theta[:, 1], 0.0, atol=1e-5) and np.all(logp > -1e-9)
    A = np.array([[2.0, 0.3], [0.3, 1.0]])
    quad = lambda th: (-0.5 * np.einsum("mi,ij,mj->m", th, A, th), -th @ A, np.broadcast_to(-A, (th.shape[0], 2, 2)).copy())
    theta, _, _, _, n_iter, conv = newton_maximize(quad, np.array([[3.0, -4.0]]))
    assert conv[0] and n_iter[0] == 2 and np.allclose(theta, 0.0, atol=1e-12)
