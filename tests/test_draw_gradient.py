"""d ln P / d theta of the params draws on the host (no GPU): the derivative of a draw recipe (DrawRecipe.derivative / jacobian) against
stencils of DrawRecipe.rows, the data-space adjoint (grad_util.data_space_adjoint, the yardstick of the GPU tests) against Richardson
differences of the oracle's ln P, and the kernel's Gram-space formula restated in NumPy (grad_util.gram_adjoint) against that yardstick.

Stencil.  The rows are cubic in theta at most, so the five-point stencil (8 (r(+h) - r(-h)) - (r(+2h) - r(-2h))) / 12h is exact for any h
and what remains is the rounding of ``rows`` at the four points, 18 / 12h times a few unit roundoffs of rows_magnitude there.  That is
compared in units of jacobian_magnitude at theta (bar: 64 unit roundoffs, the bar test_draw_recipe.py holds ``rows`` to against
rows_magnitude).  The monomials of an entry that do not hold theta_p add their rounding to the stencil and nothing to the derivative, so
the step is long: h is the power of two next to |theta_p| per draw and parameter (theta_p +- h, +- 2h are exact; a monomial theta_p^m
grows by at most 3^m at the stencil points, against m / |theta_p| times itself in the derivative), and the draws keep |theta_p| in
[0.5, 2.5] with both signs, so no monomial of the derivative is small against the others of its entry only because theta_p is.
Measured: 23 unit roundoffs at worst (east coast), 4 to 10 for the west-coast recipes; with h next to |theta_p| / 2 the east-coast
case reaches 76: the stencil's rounding, not the table's."""
import numpy as np
import pytest

import cfg3_util as U
import grad_util as GU
from conftest import load_golden

N = 48
WEST = dict(kmA=0.7, krA=0.25, ndA=4.5e-5)
CROSS = dict(kmA=0.7, krA=0.25, ndA=4.5e-5, kmB=0.45, krB=0.35, ndB=3.1e-4)


def _recipe(case):
    from eftpipe_amd.marginal import joint_draw_recipe
    from eftpipe_amd.parambasis import EastCoastBasis, WestCoastBasis, gaussian_params

    if case == "west_auto":
        return joint_draw_recipe([WestCoastBasis(prefix="A_")], gaussian_params("A_"), [WEST])
    if case == "west_cross":
        return joint_draw_recipe([WestCoastBasis(prefix="X_", cross_prefix=["A_", "B_"])], gaussian_params("X_", ("A_", "B_")), [CROSS])
    if case == "east":
        basis = EastCoastBasis(prefix="E_")
        return joint_draw_recipe([basis], basis.gaussian_params()[:7], [WEST])
    if case == "nnlo":
        basis = WestCoastBasis(prefix="A_")
        return joint_draw_recipe([basis], gaussian_params("A_") + basis.cnnloA(), [WEST], with_NNLO=True)
    g = load_golden("cfg3")
    return joint_draw_recipe(U.bases(), [str(n) for n in g["full_names"]], U.scales(g))


@pytest.mark.parametrize("case", ["west_auto", "west_cross", "east", "cfg3_joint", "nnlo"])
def test_jacobian_matches_stencil(case):
    rec = _recipe(case)
    P = len(rec.param_names)
    rng = np.random.default_rng(21)
    theta = rng.uniform(0.5, 2.5, (N, P)) * rng.choice([-1.0, 1.0], (N, P))
    f = rng.uniform(0.6, 0.9, (N, rec.ntr))
    u = 2.0**-53
    worst = 0.0
    for fun, jac, mag in ((rec.rows, rec.jacobian(theta, f), rec.jacobian_magnitude(theta, f)),) + (
            ((rec.rows_nnlo, rec.jacobian_nnlo(theta, f), rec._jac(theta, f, 24, 27, magnitude=True)),) if rec.has_nnlo else ()):
        assert jac.shape == fun(theta, f).shape + (P,) and mag.shape == jac.shape
        assert np.count_nonzero(jac) > 0 and np.all(np.abs(jac) <= mag * (1 + 8 * u))
        for p in range(P):
            h = 2.0 ** np.round(np.log2(np.abs(theta[:, p])))
            r = []
            for k in (2.0, 1.0, -1.0, -2.0):
                t = theta.copy()
                t[:, p] += k * h
                r.append(fun(t, f))
            fd = (8.0 * (r[1] - r[2]) - (r[0] - r[3])) / (12.0 * h)[:, None, None, None]
            err = np.abs(fd - jac[..., p])
            flat = mag[..., p] == 0.0  # no derivative record: the entry does not move with theta_p at all
            assert np.all(jac[..., p][flat] == 0.0) and all(np.array_equal(r[0][flat], x[flat]) for x in r[1:])
            worst = max(worst, float(np.max(err / np.where(mag[..., p] == 0.0, 1.0, mag[..., p]))) / u)
            assert np.all(err <= 64 * u * mag[..., p]), (case, p, worst)
    print(case, "worst |stencil - jacobian| in unit roundoffs of jacobian_magnitude: %.1f" % worst)


def test_derivative_records():
    from eftpipe_amd.parambasis import DrawRecipe

    # entry (0, 0, 0): 3 f a a b - 2 a + 5;  entry (0, 1, 2): b b b
    rec = DrawRecipe(["a", "b"], 1, 2, [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 2], [3.0, -2.0, 5.0, 1.0], [1, 0, 0, 0],
                     [[0, 0, 1], [0, -1, -1], [-1, -1, -1], [1, 1, 1]])
    d = rec.derivative()
    got = [(int(x["p"]), int(x["row"]), int(x["col"]), float(x["coef"]), int(x["fpow"]), tuple(int(i) for i in x["idx"])) for x in d]
    assert got == [(0, 0, 0, -2.0, 0, (-1, -1)), (0, 0, 0, 6.0, 1, (1, 0)), (1, 0, 0, 3.0, 1, (0, 0)), (1, 1, 2, 3.0, 0, (1, 1))]
    j = rec.jacobian(np.array([[2.0, 3.0]]), np.array([0.5]))
    assert j.shape == (1, 1, 2, 24, 2)
    assert j[0, 0, 0, 0, 0] == 6.0 * 0.5 * 3.0 * 2.0 - 2.0 and j[0, 0, 0, 0, 1] == 3.0 * 0.5 * 4.0 and j[0, 0, 1, 2, 1] == 27.0
    assert np.count_nonzero(j) == 3


@pytest.mark.parametrize("case", ["west_cross", "cfg3_joint", "nnlo"])
def test_derivative_is_order_independent(case):
    """a shuffled term list, with the indices of every term permuted, gives the same table: the order of every sum is the table's"""
    from eftpipe_amd.parambasis import DrawRecipe

    rec = _recipe(case)
    rng = np.random.default_rng(3)
    want = rec.derivative()
    assert want.size > rec.nterms / 2 and np.all(np.diff(want["p"]) >= 0)
    for _ in range(3):
        o = rng.permutation(rec.nterms)
        idx = np.stack([rng.permutation(r) for r in rec.idx[o]])
        got = DrawRecipe(rec.param_names, rec.ntr, rec.ng1, rec.tracer[o], rec.row[o], rec.col[o], rec.coef[o], rec.fpow[o], idx).derivative()
        assert got.tobytes() == want.tobytes()
    # one monomial given twice with two coefficients: the table orders the pair by coefficient, as the library does
    dup = lambda o: DrawRecipe(["a"], 1, 1, [0, 0], [0, 0], [0, 0], np.array([2.0, -1.0])[o], [0, 0], [[0, -1, -1]] * 2).derivative()
    assert dup([0, 1]).tobytes() == dup([1, 0]).tobytes() and list(dup([0, 1])["coef"]) == [-1.0, 2.0]


# ----------------------------------------------------------------------------- the yardstick against finite differences of the oracle
def _marg_problem(tag, ndraws=12):
    from test_gpu_draws_params import _marg_case

    g = load_golden("marg")
    templ, index = GU.marg_templates(g)
    rec, theta, _, _, f = _marg_case(g, tag, [ndraws])
    like = (g[tag + "_D"], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"])
    return rec, theta, np.tile(f[:1], (ndraws, 1)), templ, index, like


def _cfg3_problem(tag, ndraws=12):
    from test_gpu_draws import _cfg3_block
    from test_gpu_draws_params import _cfg3_draws
    from eftpipe_amd.marginal import joint_draw_recipe

    g = load_golden("cfg3")
    block, nb = _cfg3_block(g)
    names = [str(n) for n in g[tag + "_names"]]
    pn, theta, f = _cfg3_draws(g, [ndraws], 9)
    rec = joint_draw_recipe(U.bases(), names, U.scales(g), param_names=pn)
    nG = len(names)
    like = (g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf))
    return rec, theta, np.tile(f[:1], (ndraws, 1)), block, GU.cfg3_index(g, nb), like


def _worst_fd(problem, jeffreys):
    rec, theta, f, templ, index, like = problem
    worst = 0.0
    for th, ff in zip(theta, f):
        _, grad, mag = GU.adjoint_of_draw(rec, th, ff, templ, index, *like, jeffreys=jeffreys)
        fd = GU.richardson_grad(lambda t: GU.oracle_logp(rec, t, ff, templ, index, *like, jeffreys=jeffreys), th)
        worst = max(worst, float(np.max(np.abs(fd - grad) / mag)))
    return worst


# Richardson differences of the oracle's ln P (h = 2e-3 max(1, |theta_p|), one step) against the data-space adjoint, worst
# |fd - adjoint| / mag over 12 draws, Jeffreys on and off (the same figures: the trace term is smooth).  marg.npz: 1.6e-11 (auto) and
# 7.3e-11 (cross) here, 2.2e-11 and 3.2e-11 when the formula was derived; bar 1e-9, about 30 times that: the excess is the finite
# difference's own error, which moves with the draw.  cfg3.npz (ln P of -160 to -280): measured 1.2e-10 (full) and 5.6e-11 (xnost) with
# the oracle and the adjoint alone, before any device code ran; bars 30 times those.
FD_BAR = {"auto": 1e-9, "cross": 1e-9, "full": 3.5e-9, "xnost": 1.7e-9}


@pytest.mark.parametrize("jeffreys", [False, True])
@pytest.mark.parametrize("tag", ["auto", "cross", "full", "xnost"])
def test_adjoint_matches_richardson_differences_of_the_oracle(tag, jeffreys):
    worst = _worst_fd(_marg_problem(tag) if tag in ("auto", "cross") else _cfg3_problem(tag), jeffreys)
    print(tag, "jeffreys" if jeffreys else "", "worst |fd - adjoint| / mag = %.2e" % worst)
    assert worst < FD_BAR[tag]


def test_jeffreys_drops_the_trace_term():
    """a parameter that enters through F2 only (here: through the rows of the Gaussian parameters) keeps a gradient under Jeffreys, and
    the two priors' gradients differ by the trace term"""
    rec, theta, f, templ, index, like = _marg_problem("cross", 2)
    V, dV = GU.recipe_vectors(rec, theta[1], f[1], templ, index)
    _, g0, _ = GU.data_space_adjoint(V, dV, *like, jeffreys=False)
    _, g1, _ = GU.data_space_adjoint(V, dV, *like, jeffreys=True)
    F2 = np.einsum("ia,ab,jb->ij", V[1:], like[1], V[1:]) + np.diag(1.0 / np.asarray(like[3]) ** 2)
    dF2 = np.einsum("iap,ab,jb->ijp", dV[1:], like[1], V[1:])
    trace = np.einsum("ij,jip->p", np.linalg.inv(F2), dF2 + dF2.transpose(1, 0, 2))
    assert np.all(np.abs(g1) > 0) and np.allclose(g0 - g1, -0.5 * trace, rtol=1e-9, atol=0)


# ----------------------------------------------------------------------------- the kernel's Gram-space route in NumPy
@pytest.mark.parametrize("jeffreys", [False, True])
@pytest.mark.parametrize("tag", ["auto", "cross", "full", "xnost"])
def test_gram_route_matches_data_space_adjoint(tag, jeffreys):
    """The Gram route cancels where the data-space route does not (G = R^ W R^^T against V C^-1 V^T: DESIGN 10), so this is its rounding
    floor; the bar is the one the GPU tests hold the kernel to, 1e-10 of the component's magnitude."""
    rec, theta, f, templ, index, like = _marg_problem(tag) if tag in ("auto", "cross") else _cfg3_problem(tag)
    W = GU.gram_matrix(templ, index, like[0], like[1])
    worst = worst_lp = 0.0
    for th, ff in zip(theta, f):
        lp, grad, mag = GU.adjoint_of_draw(rec, th, ff, templ, index, *like, jeffreys=jeffreys)
        lpg, gg = GU.gram_adjoint(rec, th, ff, W, like[2], like[3], jeffreys=jeffreys)
        worst = max(worst, float(np.max(np.abs(gg - grad) / mag)))
        worst_lp = max(worst_lp, abs(lpg - lp) / abs(lp))
    print(tag, "jeffreys" if jeffreys else "", "Gram route: worst |grad - adjoint| / mag = %.2e, ln P relative %.2e" % (worst, worst_lp))
    assert worst_lp < 1e-10 and worst < 1e-10
