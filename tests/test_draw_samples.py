"""Samples of the marginalised parameters on the host (no GPU): the data-space yardstick of the GPU tests (sample_util.data_space_samples)
against the identities it must obey, the kernel's Gram-space route restated in NumPy (sample_util.gram_samples) against that yardstick --
the rounding floor the device bars are taken from -- and DrawRecipe.coefficients against an einsum of ``rows`` and b."""
import numpy as np
import pytest

import grad_util as GU
import sample_util as SU
from test_draw_gradient import _cfg3_problem, _marg_problem, _recipe

S = 5  # samples per draw (no multiple of the kernel's chunk of 4)


def _problem(tag):
    return _marg_problem(tag) if tag in ("auto", "cross") else _cfg3_problem(tag)


def _normals(n, s, nG, seed=11):
    return np.random.default_rng(seed).standard_normal((n, s, nG))


@pytest.mark.parametrize("tag", ["auto", "cross", "full", "xnost"])
def test_yardstick_obeys_the_gaussian_identities(tag):
    """b^ minimises chi2 + prior and 2 F2 is its Hessian there: chi2(b) + prior(b) - [chi2(b^) + prior(b^)] = z^T z exactly; z = 0 gives b^ and
    the oracle's full chi2; X^T X of the identity call is F2^-1.  Bars: 1e-9, the relative accuracy the suite pins the oracle's full chi2 to
    (the identity subtracts two chi2 of ~1e2..1e3 for a difference of ~nG); measured <= 2e-12 everywhere"""
    rec, theta, f, templ, index, like = _problem(tag)
    nG = rec.ng1 - 1
    z = _normals(theta.shape[0], S, nG)
    worst = worst_c = 0.0
    for d, (th, ff) in enumerate(zip(theta, f)):
        y = SU.samples_of_draw(rec, th, ff, templ, index, *like, z[d])
        assert np.allclose(y["L"] @ y["L"].T, y["F2"], rtol=1e-12, atol=0)
        worst = max(worst, SU.identity_error(y["chi2"], y["b"], y["fullchi2"], y["best"], like[2], like[3], z[d]))
        y0 = SU.samples_of_draw(rec, th, ff, templ, index, *like, np.zeros((1, nG)))
        assert np.array_equal(y0["b"][0], y["best"]) and np.isclose(y0["chi2"][0], y["fullchi2"], rtol=1e-12, atol=0)
        yi = SU.samples_of_draw(rec, th, ff, templ, index, *like, np.eye(nG))
        worst_c = max(worst_c, SU.covariance_error(y["F2"], yi["b"] - yi["best"]))
    print(tag, "yardstick: identity %.2e, covariance %.2e" % (worst, worst_c))
    assert worst < 1e-9 and worst_c < 1e-9


def test_cholesky_rows():
    rng = np.random.default_rng(2)
    A = rng.standard_normal((6, 9))
    F2 = A @ A.T
    U, ok = SU.cholesky_rows(F2)
    assert ok and np.array_equal(U, np.triu(U)) and np.all(np.diag(U) > 0)
    assert np.allclose(U.T @ U, F2, rtol=1e-13, atol=1e-13) and np.allclose(U, np.linalg.cholesky(F2).T, rtol=1e-12, atol=1e-13)
    assert not SU.cholesky_rows(-F2)[1]  # negative definite, det > 0: an even dimension
    assert not SU.cholesky_rows(np.diag([1.0, 0.0, 1.0]))[1]
    assert not SU.cholesky_rows(np.diag([1.0, np.nan]))[1]


@pytest.mark.parametrize("jeffreys", [False, True])
@pytest.mark.parametrize("tag", ["auto", "cross", "full", "xnost"])
def test_gram_route_matches_data_space_samples(tag, jeffreys):
    """the rounding floor of the Gram route over 12 draws x S = 5 (the covariance over the S = nG identity call); recorded in
    sample_util.SAMPLE_FLOOR, from which the GPU tests take their bars.  Jeffreys only drops ln det F2 from ln P: the samples do not move."""
    rec, theta, f, templ, index, like = _problem(tag)
    nG = rec.ng1 - 1
    W = GU.gram_matrix(templ, index, like[0], like[1])
    z = _normals(theta.shape[0], S, nG)
    worst = dict(samples=0.0, covariance=0.0, identity=0.0)
    for d, (th, ff) in enumerate(zip(theta, f)):
        y = SU.samples_of_draw(rec, th, ff, templ, index, *like, z[d], jeffreys=jeffreys)
        best, b, chi2, full = SU.gram_samples(rec, th, ff, W, like[2], like[3], z[d])
        assert np.all(np.isfinite(b))  # (Cholesky succeeds on every draw: none is skipped)
        worst["samples"] = max(worst["samples"], SU.whitened_error(y["L"], b, y["b"]))
        worst["identity"] = max(worst["identity"], SU.identity_error(chi2, b, full, best, like[2], like[3], z[d]))
        assert np.allclose(chi2, SU.chi2_at(rec, th, ff, templ, index, like[0], like[1], b), rtol=1e-9, atol=0)  # chi2 at the route's own b
        bi = SU.gram_samples(rec, th, ff, W, like[2], like[3], np.eye(nG))
        worst["covariance"] = max(worst["covariance"], SU.covariance_error(y["F2"], bi[1] - bi[0]))
    print(tag, "jeffreys" if jeffreys else "", "Gram route: " + ", ".join("%s %.2e" % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v < 1e-10, (tag, k, v)
        assert v <= 1.5 * SU.SAMPLE_FLOOR[tag][k], (tag, k, v)  # (1.5: another NumPy / BLAS rounds differently)


def test_gram_samples_fail_where_f2_is_not_positive_definite():
    rec, theta, f, templ, index, like = _problem("auto")
    nG = rec.ng1 - 1
    W = GU.gram_matrix(templ, index, like[0], -like[1])  # the negated inverse covariance: F2 negative definite under a flat prior
    _, b, chi2, _ = SU.gram_samples(rec, theta[0], f[0], W, np.zeros(nG), np.full(nG, np.inf), np.ones((2, nG)))
    assert np.all(np.isnan(b)) and np.all(np.isnan(chi2))


@pytest.mark.parametrize("case", ["west_auto", "west_cross", "east", "cfg3_joint", "nnlo"])
def test_coefficients_match_einsum_of_rows(case):
    """coefficients = rows[0] + sum_g b[g - 1] rows[g]: a sum of at most nG + 1 products per coefficient, so any order of it lies within
    (nG + 2) unit roundoffs of the sum of the terms' magnitudes"""
    rec = _recipe(case)
    P, nG = len(rec.param_names), rec.ng1 - 1
    rng = np.random.default_rng(5)
    N = 6
    theta = rng.uniform(0.5, 2.5, (N, P)) * rng.choice([-1.0, 1.0], (N, P))
    f = rng.uniform(0.6, 0.9, (N, rec.ntr))
    b = rng.standard_normal((N, S, nG)) * 3.0
    v = np.concatenate([np.ones((N, S, 1)), b], axis=2)
    u = 2.0**-53
    for fun, rows in ((rec.coefficients, rec.rows(theta, f)),) + (((rec.coefficients_nnlo, rec.rows_nnlo(theta, f)),) if rec.has_nnlo else ()):
        got = fun(theta, f, b)
        assert got.shape == (N, S, rec.ntr, rows.shape[-1]) and np.count_nonzero(got) > 0
        want = np.einsum("nsg,ntgr->nstr", v, rows)
        mag = np.einsum("nsg,ntgr->nstr", np.abs(v), np.abs(rows))
        assert np.all(np.abs(got - want) <= (nG + 2) * u * mag)
        assert np.array_equal(fun(theta, f, b[:, 0]), got[:, :1])  # [N, nG]: one sample per draw
        assert np.array_equal(fun(theta, f, np.zeros((N, 1, nG)))[:, 0], rows[:, :, 0])
    with pytest.raises(ValueError, match="b must be"):
        rec.coefficients(theta, f, b[:, :, :-1])
