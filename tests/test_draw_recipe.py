"""Draw recipes (parambasis.DrawRecipe, bias_draw_recipe, marginal.joint_draw_recipe): the rows a recipe evaluates from parameter values
against the existing row builders, draw for draw, and the compile-time refusals.  The two are the same few products in another order:
rtol 1e-14, and exactly zero wherever the builder's entry is zero.

Where the draws come from.  rtol 1e-14 of an entry asks the builder -- the yardstick -- to be that accurate itself.  The west-coast builders
are: every entry is a product, or a sum of two products that differ in sign only where the parameters do, and the west-coast cases draw
generic parameters of both signs.  The east-coast builders first map the parameters (eastcoast_to_bs: b1 + 7/2 bG2, b1 + 15 bG2 +
6 bGamma3, b2 / 2 - 7/2 bG2, c0 - f / 3 c2 + 3/35 f^2 c4, c2 - 6/7 f c4) and then multiply the mapped values.  Where such a sum cancels by
a factor A, the builder's own value carries a relative rounding error of about A 2^-53, before anything is compared with it: at A of a few
tens, which generic draws reach many times in 96, the yardstick is no longer good to 1e-14 and no evaluation of the same polynomial in
another order can agree with it to that.  The east-coast cases therefore draw from the orthant in which every sum of the mapping adds terms
of one sign (b2, c2 < 0, all other parameters > 0; magnitudes uniform in [0.3, 2.5]): there the builder is accurate to a few ulp and the
1e-14 measures the recipe.  Generic east-coast draws are checked too (test_eastcoast_generic_draws), against the bound that floating
point gives for a sum of monomials: a number of roundings times the sum of the monomials' magnitudes (DrawRecipe.rows_magnitude)."""
import numpy as np
import pytest

import cfg3_util as U
from conftest import load_golden

N = 96
WEST = dict(kmA=0.7, krA=0.25, ndA=4.5e-5)
CROSS = dict(kmA=0.7, krA=0.25, ndA=4.5e-5, kmB=0.45, krB=0.35, ndB=3.1e-4)


def _same(got, want):
    assert got.shape == want.shape
    assert np.all(got[want == 0.0] == 0.0)
    assert np.allclose(got, want, rtol=1e-14, atol=0)
    assert np.count_nonzero(want) > 0


def _draws(P, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 1.0, (N, P)) + 1.5, rng.uniform(0.6, 0.9, N)


EAST_SIGN = {"b2": -1.0, "c2": -1.0}  # the orthant in which every sum of eastcoast_to_bs adds terms of one sign (module docstring)


def _east_draws(names, seed):
    """theta [N, len(names)] in that orthant (names without prefix), f [N]"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.3, 2.5, (N, len(names))) * [EAST_SIGN.get(n, 1.0) for n in names], rng.uniform(0.6, 0.9, N)


EAST_FULL = ("b1", "b2", "bG2", "bGamma3", "c0", "c2", "c4", "Pshot", "a0", "a2")


def test_westcoast_auto_rows():
    from eftpipe_amd.marginal import joint_draw_recipe
    from eftpipe_amd.parambasis import WestCoastBasis, gaussian_params, gaussian_rows_many

    basis = WestCoastBasis(prefix="A_")
    rec = joint_draw_recipe([basis], gaussian_params("A_"), [WEST])
    assert rec.param_names == ["A_b1", "A_b2", "A_b4"] and (rec.ntr, rec.ng1) == (1, 8) and not rec.has_nnlo
    theta, f = _draws(3, 1)
    _same(rec.rows(theta, f)[:, 0], gaussian_rows_many(f, theta, None, **WEST))
    assert not np.any(rec.rows_nnlo(theta, f))
    assert rec.terms().dtype.itemsize == 40 and rec.terms().size == rec.nterms


def test_westcoast_cross_rows():
    from eftpipe_amd.marginal import joint_draw_recipe
    from eftpipe_amd.parambasis import WestCoastBasis, gaussian_params, gaussian_rows_many

    basis = WestCoastBasis(prefix="X_", cross_prefix=["A_", "B_"])
    rec = joint_draw_recipe([basis], gaussian_params("X_", ("A_", "B_")), [CROSS])
    assert rec.param_names == ["A_b1", "A_b2", "A_b4", "B_b1", "B_b2", "B_b4"] and rec.ng1 == 12
    theta, f = _draws(6, 2)
    _same(rec.rows(theta, f)[:, 0], gaussian_rows_many(f, theta[:, :3], theta[:, 3:], **CROSS))
    # theta in another order
    order = ["B_b4", "A_b1", "B_b1", "A_b4", "A_b2", "B_b2"]
    rec2 = joint_draw_recipe([basis], gaussian_params("X_", ("A_", "B_")), [CROSS], param_names=order)
    perm = [rec.param_names.index(n) for n in order]
    assert np.array_equal(rec2.rows(theta[:, perm], f), rec.rows(theta, f))


def test_eastcoast_rows():
    from eftpipe_amd.marginal import joint_draw_recipe
    from eftpipe_amd.parambasis import EastCoastBasis, gaussian_rows_many

    basis = EastCoastBasis(prefix="E_")
    rec = joint_draw_recipe([basis], basis.gaussian_params()[:7], [WEST])
    assert rec.param_names == ["E_b1", "E_b2", "E_bG2"] and rec.ng1 == 8
    theta, f = _east_draws(("b1", "b2", "bG2"), 3)
    _same(rec.rows(theta, f)[:, 0], gaussian_rows_many(f, theta, basis="eastcoast", **WEST))


def test_eastcoast_generic_draws():
    """East-coast recipes at generic parameters of both signs, where the mapped parameters cancel (module docstring).  Bound: the recipe and
    the builder each evaluate the entry as a sum of at most 9 monomials; a monomial's value carries at most 16 roundings (its coefficient
    at most 6, f^e at most 5, the products 4, one to spare) and the summation at most 8 more, for both sides 2 (16 + 8) = 48, taken as
    64 unit roundoffs 2^-53 of the sum of the monomials' magnitudes.  Measured: 4 of them at worst; relative to the entry itself the same
    differences reach 9.4e-14 (Gaussian rows) and 5.6e-13 (bias rows) where the entry cancels."""
    from eftpipe_amd.marginal import joint_draw_recipe
    from eftpipe_amd.parambasis import EastCoastBasis, bias_draw_recipe, eastcoast_bias_row, gaussian_rows_many

    basis = EastCoastBasis(prefix="E_")
    u = 2.0**-53
    rec = joint_draw_recipe([basis], basis.gaussian_params()[:7], [WEST])
    theta, f = _draws(3, 3)
    got, want, mag = rec.rows(theta, f)[:, 0], gaussian_rows_many(f, theta, basis="eastcoast", **WEST), rec.rows_magnitude(theta, f)[:, 0]
    assert np.all(got[want == 0.0] == 0.0) and np.all(np.abs(got - want) <= 64 * u * mag)
    assert np.max(mag / np.where(got == 0.0, np.inf, np.abs(got))) > 30.0  # (the draws do reach cancelling entries)
    rec = bias_draw_recipe(basis, WEST)
    rng = np.random.default_rng(6)
    f, theta = rng.uniform(0.6, 0.9, N), rng.normal(0.0, 1.0, (N, 10)) + 0.5
    want = np.stack([eastcoast_bias_row(float(fi), *[float(v) for v in th], **WEST) for fi, th in zip(f, theta)])
    got, mag = rec.rows(theta, f)[:, 0, 0], rec.rows_magnitude(theta, f)[:, 0, 0]
    assert np.all(got[want == 0.0] == 0.0) and np.all(np.abs(got - want) <= 64 * u * mag)


@pytest.mark.parametrize("tag", ["full", "xnost"])
def test_cfg3_joint_rows(tag):
    from eftpipe_amd.marginal import joint_draw_recipe, joint_gaussian_rows_many

    g = load_golden("cfg3")
    names = [str(n) for n in g[tag + "_names"]]
    rec = joint_draw_recipe(U.bases(), names, U.scales(g))
    assert rec.param_names == [t + p for t in ("LRG_NGC_", "ELG_NGC_") for p in ("b1", "b2", "b4")]
    assert (rec.ntr, rec.ng1) == (3, len(names) + 1)
    rng = np.random.default_rng(5)
    theta = rng.normal(0.0, 1.0, (N, 6)) + 1.5
    f = rng.uniform(0.6, 0.9, (N, 3))  # a growth rate per draw's walker and tracer
    params = {n: theta[:, i] for i, n in enumerate(rec.param_names)}
    _same(rec.rows(theta, f), joint_gaussian_rows_many(U.bases(), list(f.T), params, names, U.scales(g)))


@pytest.mark.parametrize("form", ["westcoast", "westcoast_cross", "eastcoast"])
def test_bias_recipe_rows(form):
    from eftpipe_amd.parambasis import EastCoastBasis, WestCoastBasis, bias_draw_recipe, bias_rows_many, eastcoast_bias_row

    rng = np.random.default_rng(6)
    f = rng.uniform(0.6, 0.9, N)
    if form == "eastcoast":
        basis = EastCoastBasis(prefix="E_")
        rec = bias_draw_recipe(basis, WEST)
        assert rec.param_names == basis.bsA() + basis.es() == ["E_" + n for n in EAST_FULL]
        theta, f = _east_draws(EAST_FULL, 6)
        want = np.stack([eastcoast_bias_row(float(fi), *[float(v) for v in th], **WEST) for fi, th in zip(f, theta)])
    elif form == "westcoast":
        basis = WestCoastBasis(prefix="A_")
        rec = bias_draw_recipe(basis, WEST)
        assert rec.param_names == basis.bsA() + basis.es()
        theta = rng.normal(0.0, 1.0, (N, 10)) + 0.5
        want = bias_rows_many(f, theta[:, :7], None, theta[:, 7:], **WEST)
    else:
        basis = WestCoastBasis(prefix="X_", cross_prefix=["A_", "B_"])
        rec = bias_draw_recipe(basis, CROSS)
        assert rec.param_names == basis.bsA() + basis.bsB() + basis.es()
        theta = rng.normal(0.0, 1.0, (N, 17)) + 0.5
        want = bias_rows_many(f, theta[:, :7], theta[:, 7:14], theta[:, 14:], **CROSS)
    assert (rec.ntr, rec.ng1) == (1, 1)
    _same(rec.rows(theta, f)[:, 0, 0], want)


def test_bias_recipe_eastcoast_counterform_matches_bias_rows_many():
    """the east-coast counter-term form of bias_rows_many (its bsA are the mapped parameters) through the east-coast recipe"""
    from eftpipe_amd.parambasis import EastCoastBasis, bias_draw_recipe, bias_rows_many, eastcoast_to_bs

    theta, f = _east_draws(EAST_FULL, 8)
    mapped = [eastcoast_to_bs(float(fi), *[float(v) for v in th]) for fi, th in zip(f, theta)]
    want = bias_rows_many(f, np.array([m[0] for m in mapped]), None, np.array([m[1] for m in mapped]), counterform="eastcoast", **WEST)
    _same(bias_draw_recipe(EastCoastBasis(prefix="E_"), WEST).rows(theta, f)[:, 0, 0], want)


@pytest.mark.parametrize("form", ["westcoast", "eastcoast"])
def test_nnlo_columns(form):
    from eftpipe_amd.marginal import joint_draw_recipe
    from eftpipe_amd.parambasis import EastCoastBasis, WestCoastBasis, bias_draw_recipe, gaussian_params, nnlo_vector

    rng = np.random.default_rng(10)
    f = rng.uniform(0.6, 0.9, N)
    basis = WestCoastBasis(prefix="A_") if form == "westcoast" else EastCoastBasis(prefix="E_")
    rec = bias_draw_recipe(basis, WEST, with_NNLO=True)
    assert rec.has_nnlo and rec.param_names == basis.bsA() + basis.es() + basis.cnnloA()
    P = len(rec.param_names)
    theta = rng.normal(0.0, 1.0, (N, P)) + 0.5
    cn = theta[:, 10:] if form == "westcoast" else np.stack([theta[:, 10], np.zeros(N)], axis=1)
    want = np.stack([nnlo_vector(float(fi), float(th[0]), [float(v) for v in c], WEST["krA"], form) for fi, th, c in zip(f, theta, cn)])
    _same(rec.rows_nnlo(theta, f)[:, 0, 0], want)
    _same(rec.rows(theta, f), bias_draw_recipe(basis, WEST).rows(theta[:, :10], f))
    # a likelihood recipe that marginalises the NNLO parameters: their rows are the derivatives of nnlo_vector
    own = gaussian_params("A_") if form == "westcoast" else basis.gaussian_params()[:7]
    names = own + basis.cnnloA()
    jr = joint_draw_recipe([basis], names, [WEST], with_NNLO=True)
    th3 = theta[:, :3]
    rn = jr.rows_nnlo(th3, f)[:, 0]
    assert not np.any(rn[:, : 1 + len(own)])
    for q in range(len(basis.cnnloA())):
        unit = [1.0 if m == q else 0.0 for m in range(2)]
        _same(rn[:, 1 + len(own) + q], np.stack([nnlo_vector(float(fi), float(b1), unit, WEST["krA"], form) for fi, b1 in zip(f, th3[:, 0])]))
    assert np.array_equal(jr.rows(th3, f)[:, 0, : 1 + len(own)], joint_draw_recipe([basis], own, [WEST]).rows(th3, f)[:, 0])


def test_compile_time_refusals():
    from eftpipe_amd.marginal import joint_draw_recipe
    from eftpipe_amd.parambasis import (RECIPE_MAXP, RECIPE_MAXTERMS, DrawRecipe, EastCoastBasis, WestCoastBasis, _compile_recipe, _poly_theta, _POLY_F,
                                        bias_draw_recipe, gaussian_params, gaussian_rows)

    with pytest.raises(NotImplementedError, match="cross"):  # east-coast cross: as the reference
        EastCoastBasis(prefix="X_", cross_prefix=["A_", "B_"])
    with pytest.raises(NotImplementedError, match="cross"):
        gaussian_rows(_POLY_F, [_poly_theta(0)] * 3, [_poly_theta(1)] * 3, basis="eastcoast")
    # P: five auto tracers' full parameter sets are 50 names
    bases = [WestCoastBasis(prefix="T%d_" % t) for t in range(5)]
    with pytest.raises(ValueError, match=f"at most {RECIPE_MAXP} parameters"):
        bias_draw_recipe(bases, [WEST] * 5)
    with pytest.raises(ValueError, match=f"at most {RECIPE_MAXP} parameters"):
        DrawRecipe(["p%d" % i for i in range(RECIPE_MAXP + 1)], 1, 1, [0], [0], [0], [1.0], [0], [[0, -1, -1]])
    # term count
    n = RECIPE_MAXTERMS + 1
    with pytest.raises(ValueError, match=f"at most {RECIPE_MAXTERMS} terms"):
        DrawRecipe(["a"], 1, 1, [0] * n, [0] * n, [0] * n, [1.0] * n, [0] * n, [[0, -1, -1]] * n)
    # degree in theta, power of f
    x = _poly_theta(0)
    with pytest.raises(ValueError, match="degree 4"):
        _compile_recipe(["a"], [[[x * x * x * x] + [0.0] * 23]], 1)
    with pytest.raises(ValueError, match="f\\^7"):
        _compile_recipe(["a"], [[[x * _POLY_F**7] + [0.0] * 23]], 1)
    with pytest.raises(ValueError, match="divide by a parameter"):
        1.0 / x
    # entries and indices out of range, names
    for bad in (dict(tracer=[1]), dict(row=[1]), dict(col=[27]), dict(fpow=[7]), dict(idx=[[1, -1, -1]]), dict(idx=[[-2, -1, -1]]), dict(coef=[np.inf])):
        kw = dict(tracer=[0], row=[0], col=[0], coef=[1.0], fpow=[0], idx=[[0, -1, -1]])
        kw.update(bad)
        with pytest.raises(ValueError):
            DrawRecipe(["a"], 1, 1, **kw)
    basis = WestCoastBasis(prefix="A_")
    with pytest.raises(ValueError, match="lacks"):
        joint_draw_recipe([basis], gaussian_params("A_"), [WEST], param_names=["A_b1", "A_b2"])
    with pytest.raises(ValueError, match="repeats"):
        joint_draw_recipe([basis], gaussian_params("A_"), [WEST], param_names=["A_b1", "A_b2", "A_b4", "A_b1"])
    with pytest.raises(ValueError, match="theta must be"):
        joint_draw_recipe([basis], gaussian_params("A_"), [WEST]).rows(np.zeros((4, 2)), 0.7)


def test_scalar_builders_keep_their_bits():
    """the row helper shared with the recipe compiler returns float rows for float input, as before"""
    from eftpipe_amd.parambasis import gaussian_rows, gaussian_rows_many

    for kw in (dict(), dict(basis="eastcoast")):
        r = gaussian_rows(0.78, (2.1, 0.4, -0.3), None, **WEST, **kw)
        assert r.dtype == np.float64
        assert np.array_equal(r, gaussian_rows_many(0.78, np.array([[2.1, 0.4, -0.3]]), None, **WEST, **kw)[0])
