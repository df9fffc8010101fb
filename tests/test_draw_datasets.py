"""Draw calls against many data vectors sharing one covariance, on the host (no GPU): the border route of DESIGN 10.6 restated in NumPy --
the template block of grad_util.gram_matrix plus the last row and column from a data set D_m, as draws_gram_groups_kernel builds Wg -- and
taken through the Gram-space evaluators (grad_util.gram_adjoint, hess_util.gram_hessian) against the data-space yardsticks evaluated with
D_m (grad_util.adjoint_of_draw, hess_util.hessian_of_draw).  The worst Hessian error per case is that case's floor (DATASET_FLOOR), from
which test_gpu_draws_datasets.py takes its bar (hess_util.device_bar).  Also the argument checks of MarginalLikelihood.set_datasets and of
``groups=``, which need no device.

Data sets: set 0 is the fixture's own vector D; set m >= 1 is D + chol(C) z_m with z_m standard normal from default_rng(100 + m): a mock
scattered by the covariance itself.  F2 does not depend on the data, so no data set brings a det F2 <= 0 the fixture's draws did not have."""
from types import SimpleNamespace

import numpy as np
import pytest

import grad_util as GU
import hess_util as HU
from test_draw_gradient import _cfg3_problem, _marg_problem

NDRAWS = 6
NSETS = {"auto": 3, "cross": 3, "xnost": 2}

# worst |gram_hessian on the bordered W - data_space_hessian with D_m| / mag over NDRAWS draws x the data sets of the case, Jeffreys on and
# off, measured on the host (test_border_route_matches_data_space_yardsticks asserts them); the device bar is hess_util.device_bar(floor)
DATASET_FLOOR = {"auto": 1.3e-13, "cross": 1.7e-12, "xnost": 9.8e-13}


def datasets(D, invcov, M):
    """[M, ndata]: the fixture's vector, then M - 1 mocks D + chol(inv(invcov)) z_m"""
    chol = np.linalg.cholesky(np.linalg.inv(invcov))
    return np.stack([np.asarray(D, dtype=np.float64)] + [D + chol @ np.random.default_rng(100 + m).standard_normal(len(D)) for m in range(1, M)])


def template_columns(templ, index, templn=None):
    """A [J, ndata]: the template rows of grad_util.gram_matrix's A (everything but the data row), in its column order"""
    ntr, nl, _, nx = templ.shape
    cols = []
    for tau in range(ntr):
        for r in range(24):
            z = np.zeros((ntr, nl, nx))
            z[tau] = templ[tau, :, r]
            cols.append(z.reshape(-1)[index])
    if templn is not None:
        for tau in range(ntr):
            for j in range(3):
                z = np.zeros((ntr, nl, nx))
                z[tau] = templn[tau, :, 3 + j]
                cols.append(z.reshape(-1)[index])
    return np.stack(cols)


def bordered_gram(W, A, invcov, d):
    """Wg of one group: the template block of the walker's W, and the border of data set d as the device computes it --
    Wg[j][J] = Wg[J][j] = -(A_j . Ud + U_j . d) / 2 with U = A C^-1, Ud = d C^-1, and Wg[J][J] = d . Ud"""
    J = A.shape[0]
    U, Ud = A @ invcov, d @ invcov
    Wg = np.array(W, dtype=np.float64)
    Wg[:J, J] = Wg[J, :J] = -0.5 * (A @ Ud + U @ d)
    Wg[J, J] = d @ Ud
    return Wg


def problem(tag, ndraws=NDRAWS):
    return _marg_problem(tag, ndraws) if tag in ("auto", "cross") else _cfg3_problem(tag, ndraws)


def test_datasets_are_the_fixture_then_covariance_scatter():
    rec, theta, f, templ, index, like = problem("auto", 1)
    Ds = datasets(like[0], like[1], 3)
    assert Ds.shape == (3, len(like[0])) and np.array_equal(Ds[0], like[0])
    chi2 = [(d - like[0]) @ like[1] @ (d - like[0]) for d in Ds[1:]]
    n = len(like[0])
    assert all(n - 5 * np.sqrt(2 * n) < c < n + 5 * np.sqrt(2 * n) for c in chi2) and not np.allclose(Ds[1], Ds[2])


def test_border_of_the_own_vector_is_the_gram_matrix():
    """set 0 through the border route is grad_util.gram_matrix itself, up to the rounding of a differently ordered sum"""
    for tag in ("auto", "xnost"):
        rec, theta, f, templ, index, like = problem(tag, 1)
        W = GU.gram_matrix(templ, index, like[0], like[1])
        Wg = bordered_gram(W, template_columns(templ, index), like[1], np.asarray(like[0], dtype=np.float64))
        scale = np.sqrt(np.outer(np.diag(W), np.diag(W)))
        assert np.array_equal(Wg[:-1, :-1], W[:-1, :-1]) and np.array_equal(Wg, Wg.T)
        assert np.max(np.abs(Wg - W) / scale) < 1e-14


@pytest.mark.parametrize("tag", ["auto", "cross", "xnost"])
def test_border_route_matches_data_space_yardsticks(tag):
    """ln P, gradient and Hessian of the bordered W against the yardsticks evaluated with D_m.  Bars: ln P 1e-10 relative and 1e-10 of mag
    for the derivatives, the bars test_draw_gradient.py / test_draw_hessian.py hold the Gram route to; the worst Hessian error is the
    case's floor.  Measured, Jeffreys on and off alike: 1.29e-13 (auto), 1.61e-12 (cross), 9.75e-13 (xnost; gradient 1.1e-13, 1.3e-13,
    8.9e-14; ln P 8.8e-13, 1.1e-12, 1.0e-12 relative) -- the floors of the one-vector route (hess_util.GRAM_FLOOR: 1.2e-13, 1.6e-12,
    9.7e-13), as they should be: the border is two more dot products of the same length."""
    rec, theta, f, templ, index, like = problem(tag)
    D0, Ci, loc, scale = like
    Ds = datasets(D0, Ci, NSETS[tag])
    W = GU.gram_matrix(templ, index, D0, Ci)
    A = template_columns(templ, index)
    for jeffreys in (False, True):
        worst = worst_g = worst_lp = 0.0
        for m, d in enumerate(Ds):
            Wg = bordered_gram(W, A, Ci, d)
            for th, ff in zip(theta, f):
                lp, hess, mag = HU.hessian_of_draw(rec, th, ff, templ, index, d, Ci, loc, scale, jeffreys=jeffreys)
                lp2, grad, gmag = GU.adjoint_of_draw(rec, th, ff, templ, index, d, Ci, loc, scale, jeffreys=jeffreys)
                assert lp2 == lp and lp == GU.oracle_logp(rec, th, ff, templ, index, d, Ci, loc, scale, jeffreys=jeffreys)
                lpg, gg, hg = HU.gram_hessian(rec, th, ff, Wg, loc, scale, jeffreys=jeffreys)
                lpa, ga = GU.gram_adjoint(rec, th, ff, Wg, loc, scale, jeffreys=jeffreys)
                assert np.isclose(lpg, lpa, rtol=1e-12, atol=0) and np.allclose(gg, ga, rtol=0, atol=1e-12 * np.max(gmag))
                assert np.array_equal(hg, hg.T)
                worst_lp = max(worst_lp, abs(lpg - lp) / abs(lp))
                worst_g = max(worst_g, float(np.max(np.abs(gg - grad) / gmag)))
                worst = max(worst, float(np.max(np.abs(hg - hess) / mag)))
            if m:  # another data vector is another posterior
                assert abs(lp - GU.oracle_logp(rec, theta[-1], f[-1], templ, index, D0, Ci, loc, scale, jeffreys=jeffreys)) > 1e-3 * abs(lp)
        print(tag, "jeffreys" if jeffreys else "", "border route: worst |hess - yardstick| / mag = %.2e (gradient %.2e, ln P relative %.2e)" % (worst, worst_g, worst_lp))
        assert worst_lp < 1e-10 and worst_g < 1e-10 and worst < 1e-10
        assert worst <= 1.5 * DATASET_FLOOR[tag]  # (the recorded floor; 1.5: another NumPy / BLAS rounds differently)


# ----------------------------------------------------------------------------- argument checks (no device)
class _Lib:
    """stands in for the library: records the calls, reports success"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append((name, a))
            if name == "eftb_draws_logp_params_datasets":
                for d in range(a[5]):
                    a[9][d] = -1.0  # logp [N]: the wrapper raises where it finds NaN
            return 0

        return call


def _like(ntr=1, nG=7, ndata=36):
    from eftpipe_amd.marginal import MarginalLikelihood

    eng = SimpleNamespace(lib=_Lib(), _h=None, ntracers=ntr, cfg=SimpleNamespace(with_NNLO=False))
    like = MarginalLikelihood(eng, np.arange(ndata), np.zeros(ndata), np.eye(ndata), np.zeros(nG), np.ones(nG))
    eng.lib.calls.clear()
    return like, eng.lib


def test_set_datasets_arguments():
    like, lib = _like()
    like.set_datasets(np.zeros((3, 36)))
    like.set_datasets([[0.0] * 36])
    like.set_datasets(None)
    assert [(n, a[1]) for n, a in lib.calls] == [("eftb_set_likelihood_datasets", 3), ("eftb_set_likelihood_datasets", 1), ("eftb_set_likelihood_datasets", 0)]
    assert lib.calls[2][1][2] is None
    for bad in (np.zeros(36), np.zeros((2, 35)), np.zeros((0, 36)), np.zeros((2, 36, 1))):
        with pytest.raises(ValueError, match=r"data must be \[M, 36\]"):
            like.set_datasets(bad)
    assert len(lib.calls) == 3


def test_groups_arguments():
    like, lib = _like()
    theta = np.zeros((5, 3))
    g = ([0, 0, 1], [2, 0, 1])
    off = [0, 2, 2, 5]
    f = [0.7, 0.8]
    out = like.logp_draws_params(theta, off, f, groups=g)
    assert out.shape == (5,)
    name, a = lib.calls[-1]
    assert name == "eftb_draws_logp_params_datasets" and a[1] == 2 and a[2] == 3 and a[5] == 5  # C walkers from f, G groups, N draws
    assert a[10] is None and a[11] is None  # no gradient, no Hessian asked for
    lp, gr, he, full, best = like.logp_draws_params(theta, off, f, groups=g, grad=True, hess=True, return_best=True)
    assert gr.shape == (5, 3) and he.shape == (5, 3, 3) and full.shape == (5,) and best.shape == (5, 7)
    assert lib.calls[-1][1][10] is not None and lib.calls[-1][1][11] is not None
    assert [x.shape for x in like.logp_draws_params(theta, off, f, groups=g, grad=True)] == [(5,), (5, 3)]
    assert [x.shape for x in like.logp_draws_params(theta, off, f, groups=g, return_best=True)] == [(5,), (5,), (5, 7)]
    n = len(lib.calls)
    with pytest.raises(ValueError, match="hess=True needs grad=True"):
        like.logp_draws_params(theta, off, f, groups=g, hess=True)
    for bad in (([0, 0, 1],), ([0, 0, 1], [2, 0]), ([[0, 0, 1]], [[2, 0, 1]]), ([], []), 3):
        with pytest.raises(ValueError, match=r"groups must be \(walker \[G\], dataset \[G\]\)"):
            like.logp_draws_params(theta, off, f, groups=bad)
    for bad in (([0.0, 0.0, 1.0], [2, 0, 1]), ([0, 0, 1], [2, 0, 2**40])):
        with pytest.raises(ValueError, match="integers"):
            like.logp_draws_params(theta, off, f, groups=bad)
    with pytest.raises(ValueError, match=r"offsets must be \[4\]"):
        like.logp_draws_params(theta, [0, 2, 5], f, groups=g)
    with pytest.raises(ValueError, match=r"f must be \[C, 1\]"):
        like.logp_draws_params(theta, off, np.zeros((2, 2)), groups=g)
    with pytest.raises(ValueError, match=r"theta must be \[N, P\]"):
        like.logp_draws_params(np.zeros(5), off, f, groups=g)
    with pytest.raises(ValueError, match=r"groups must be"):
        like.maximize_draws_params(theta, off, f, groups=([0], [0], [0]))
    assert len(lib.calls) == n  # nothing reached the library
    like3, _ = _like(ntr=3)
    with pytest.raises(ValueError, match=r"f must be \[C, 3\]"):
        like3.logp_draws_params(theta, off, [0.7, 0.8], groups=g)
