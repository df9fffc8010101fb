"""Samples of the marginalised parameters on the device (eftb_draws_sample_params; MarginalLikelihood.sample_gaussian_params).  Yardstick:
sample_util.data_space_samples (the oracle's b^ and F2 in data space and NumPy's Cholesky factor; pinned on the host by
test_draw_samples.py), sample by sample, in the whitened units of sample_util.py.  Bars (hess_util.device_bar): 1e-10 where the NumPy
restatement of the Gram route sits at <= 1e-12, 100 times that floor elsewhere; the floors are sample_util.SAMPLE_FLOOR for the fixture
likelihoods and measured on the host, on the draws at hand, for the others (flat prior on auto, NNLO) before anything is asked of the device.
ln P, full chi2 and the best fit are the bits of logp_draws_params; a sample's bits depend neither on S nor on the split into calls."""
import numpy as np
import pytest

import cfg3_util as U
import grad_util as GU
import sample_util as SU
from hess_util import device_bar
from test_draw_datasets import datasets
from test_gpu_draws import COUNTS, _marg, _offsets
from test_gpu_draws_grad import _nnlo_problem
from test_gpu_draws_params import _cfg3_draws, _cfg3_engine, _marg_case

pytestmark = pytest.mark.gpu

S5 = 5  # no multiple of the kernel's chunk of 4 samples


def _normals(N, S, nG, seed=23):
    return np.random.default_rng(seed).standard_normal((N, S, nG))


def _per_draw(f, nC, ntr, walker, templ, templn, d):
    w = walker[d]
    return np.reshape(f, (nC, ntr))[w], templ[w * ntr : (w + 1) * ntr], None if templn is None else templn[w * ntr : (w + 1) * ntr]


def _host_floor(rec, theta, f, nC, walker, templ, index, lk, z, templn, ntr, draws):
    """the NumPy restatement of the Gram route against the yardstick on these draws: what a device bar follows from where no floor is recorded"""
    worst = dict(samples=0.0, covariance=0.0, identity=0.0)
    nG = rec.ng1 - 1
    Wc = {}
    for d in draws:
        ff, tw, tn = _per_draw(f, nC, ntr, walker, templ, templn, d)
        if walker[d] not in Wc:
            Wc[walker[d]] = GU.gram_matrix(tw, index, lk[0], lk[1], tn)
        y = SU.samples_of_draw(rec, theta[d], ff, tw, index, *lk, z[d], templn=tn)
        best, b, chi2, full = SU.gram_samples(rec, theta[d], ff, Wc[walker[d]], lk[2], lk[3], z[d])
        bi = SU.gram_samples(rec, theta[d], ff, Wc[walker[d]], lk[2], lk[3], np.eye(nG))
        worst["samples"] = max(worst["samples"], SU.whitened_error(y["L"], b, y["b"]))
        worst["identity"] = max(worst["identity"], SU.identity_error(chi2, b, full, best, lk[2], lk[3], z[d]))
        worst["covariance"] = max(worst["covariance"], SU.covariance_error(y["F2"], bi[1] - bi[0]))
    return worst


def _check(tag, floors, like, rec, theta, off, f, walker, templ, index, lk, jeffreys, templn=None, ntr=1, draws=None):
    """the sample call against logp_draws_params (bits), against itself at other S (bits) and against the yardstick -> the S = 5 result"""
    N, nG, nC = theta.shape[0], rec.ng1 - 1, len(off) - 1
    draws = range(N) if draws is None else draws
    z = _normals(N, S5, nG)
    if floors is None:
        floors = _host_floor(rec, theta, f, nC, walker, templ, index, lk, z, templn, ntr, draws)
        print(tag, "floors of the Gram route on the host:", ", ".join("%s %.2e" % kv for kv in floors.items()))
    want = like.logp_draws_params(theta, off, f, return_best=True)
    r5 = like.sample_gaussian_params(theta, off, f, z)
    assert r5.b.shape == (N, S5, nG) and r5.chi2.shape == (N, S5) and r5.coef is None and r5.coef_nnlo is None and r5.plk is None
    assert np.all(np.isfinite(r5.b)) and np.all(np.isfinite(r5.chi2))
    for a, b in zip((r5.logp, r5.fullchi2, r5.best), want):
        assert np.array_equal(a, b)
    r1 = like.sample_gaussian_params(theta, off, f, z[:, 2])  # [N, nG]: S = 1; sample 2 of the S = 5 call alone
    assert r1.b.shape == (N, 1, nG) and np.array_equal(r1.b[:, 0], r5.b[:, 2]) and np.array_equal(r1.chi2[:, 0], r5.chi2[:, 2])
    assert np.array_equal(r1.logp, r5.logp) and np.array_equal(r1.best, r5.best)
    r0 = like.sample_gaussian_params(theta, off, f, np.zeros((N, 1, nG)))  # z = 0: the best fit and its chi2
    assert np.array_equal(r0.b[:, 0], r5.best) and np.array_equal(r0.chi2[:, 0], r5.fullchi2)
    zi = np.concatenate([z[:, :3], np.tile(np.eye(nG), (N, 1, 1))], axis=1)  # S = 3 + nG: the identity behind three of the samples
    ri = like.sample_gaussian_params(theta, off, f, zi)
    assert np.array_equal(ri.b[:, :3], r5.b[:, :3]) and np.array_equal(ri.chi2[:, :3], r5.chi2[:, :3])
    rn = like.sample_gaussian_params(theta, off, f, zi[:, 3:])  # S = nG
    assert np.array_equal(rn.b, ri.b[:, 3:]) and np.array_equal(rn.chi2, ri.chi2[:, 3:])
    worst = dict(samples=0.0, covariance=0.0, identity=0.0)
    for d in draws:
        ff, tw, tn = _per_draw(f, nC, ntr, walker, templ, templn, d)
        y = SU.samples_of_draw(rec, theta[d], ff, tw, index, *lk, z[d], jeffreys=jeffreys, templn=tn)
        worst["samples"] = max(worst["samples"], SU.whitened_error(y["L"], r5.b[d], y["b"]))
        worst["covariance"] = max(worst["covariance"], SU.covariance_error(y["F2"], rn.b[d] - rn.best[d]))
        worst["identity"] = max(worst["identity"], SU.identity_error(r5.chi2[d], r5.b[d], r5.fullchi2[d], r5.best[d], lk[2], lk[3], z[d]))
        assert np.allclose(r5.chi2[d], SU.chi2_at(rec, theta[d], ff, tw, index, lk[0], lk[1], r5.b[d], tn), rtol=1e-9, atol=0)
    print(tag, "jeffreys" if jeffreys else "", ", ".join("%s %.2e (bar %.1e)" % (k, v, device_bar(floors[k])) for k, v in worst.items()))
    for k, v in worst.items():
        assert v < device_bar(floors[k]), (tag, jeffreys, k, v)
    return r5, z


def _check_predict(eng, like, rec, theta, off, f, walker, z, ntr, nn):
    """predict=True: P_l is reduce_draws fed with coef bit for bit; coef is DrawRecipe.coefficients at the device's b to (nG + 2) unit
    roundoffs of the sum of the magnitudes of its at most nG + 1 products"""
    N, S, nG = z.shape
    r = like.sample_gaussian_params(theta, off, f, z, predict=True, return_coef=True)
    nl, nx = eng.dims
    tr = () if ntr == 1 else (ntr,)
    assert r.coef.shape == (N, S) + tr + (24,) and r.plk.shape == (N, S) + tr + (nl, nx)
    assert (r.coef_nnlo is not None) == nn and (not nn or r.coef_nnlo.shape == (N, S) + tr + (3,))
    base = like.sample_gaussian_params(theta, off, f, z)
    assert np.array_equal(r.b, base.b) and np.array_equal(r.chi2, base.chi2) and np.array_equal(r.logp, base.logp)
    only = like.sample_gaussian_params(theta, off, f, z, predict=True)
    assert only.coef is None and only.coef_nnlo is None and np.array_equal(only.plk, r.plk)
    plk = eng.reduce_draws(r.coef.reshape((N * S,) + tr + (24,)), np.asarray(off) * S, bias_nnlo=r.coef_nnlo.reshape((N * S,) + tr + (3,)) if nn else None)
    assert np.array_equal(plk.reshape(r.plk.shape), r.plk) and np.count_nonzero(r.plk) > 0
    fd = np.reshape(f, (len(off) - 1, ntr))[walker]
    u = 2.0**-53
    v = np.concatenate([np.ones((N, S, 1)), r.b], axis=2)
    worst = 0.0
    for got, fun, rows in ((r.coef, rec.coefficients, rec.rows),) + (((r.coef_nnlo, rec.coefficients_nnlo, rec.rows_nnlo),) if nn else ()):
        got = got.reshape(N, S, ntr, -1)
        want = fun(theta, fd, r.b)
        mag = np.einsum("nsg,ntgr->nstr", np.abs(v), np.abs(rows(theta, fd)))
        assert np.array_equal(got == 0.0, mag == 0.0)  # slots without an entry are written, with zero
        worst = max(worst, float(np.max(np.abs(got - want) / np.where(mag == 0.0, 1.0, mag))) / u)
        assert np.all(np.abs(got - want) <= (nG + 2) * u * mag), worst
    print("coefficients: worst |device - host| = %.1f unit roundoffs of the magnitudes (bar %d)" % (worst, nG + 2))
    return r


@pytest.mark.parametrize("tag", ["auto", "cross"])
def test_samples_match_data_space_yardstick(golden, tag):
    from eftpipe_amd.marginal import MarginalLikelihood

    g, eng, T, index = _marg(golden, tag)
    nC = len(COUNTS)
    templ = np.stack([T * (1.0 + 0.1 * c) for c in range(nC)])
    eng.put("TEMPL", templ)
    rec, theta, _, walker, f = _marg_case(g, tag, COUNTS)
    off = _offsets(COUNTS)  # (walker 1 owns no draw)
    D, Ci, loc, scale = g[tag + "_D"], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"]
    nG = len(loc)
    priors = [(loc, scale, False, SU.SAMPLE_FLOOR[tag]), (loc, scale, True, SU.SAMPLE_FLOOR[tag])]
    if tag == "auto":  # (flat prior: auto only, the cross fixture's 11 parameters are degenerate without one)
        priors.append((np.zeros(nG), np.full(nG, np.inf), False, None))
    bs = []
    for lo, sc, jeff, floors in priors:
        like = MarginalLikelihood(eng, index, D, Ci, lo, sc, jeffreys=jeff)
        like.set_draw_recipe(rec)
        r5, z = _check(tag, floors, like, rec, theta, off, f, walker, templ, index, (D, Ci, lo, sc), jeff)
        bs.append(r5.b)
    assert np.array_equal(bs[0], bs[1])  # Jeffreys only drops ln det F2 from ln P
    _check_predict(eng, like, rec, theta, off, f, walker, z, 1, False)
    eng.close()


@pytest.mark.parametrize("tag", ["full", "xnost"])
def test_cfg3_joint_samples(golden, tag):
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe

    g = golden("cfg3")
    counts = [9, 0, 1, 14]  # (4 walkers, one empty, one with a single draw)
    eng, templ, index = _cfg3_engine(g, 4, 12)
    names = [str(n) for n in g[tag + "_names"]]
    nG = len(names)
    pn, theta, f = _cfg3_draws(g, counts, 9)
    rec = joint_draw_recipe(U.bases(), names, U.scales(g), param_names=pn)
    walker = np.repeat(np.arange(4), counts)
    lk = (g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf))
    draws = np.sort(np.random.default_rng(2).choice(theta.shape[0], 12, replace=False))
    off = _offsets(counts)
    for jeff in (True, False):
        like = MarginalLikelihood(eng, index, *lk, jeffreys=jeff)
        like.set_draw_recipe(rec)
        _, z = _check("cfg3 " + tag, SU.SAMPLE_FLOOR[tag], like, rec, theta, off, f, walker, templ, index, lk, jeff, ntr=3, draws=draws)
    _check_predict(eng, like, rec, theta, off, f, walker, z, 3, False)
    eng.close()


def test_nnlo_samples():
    from eftpipe_amd.marginal import MarginalLikelihood

    eng, rec, theta, f, counts, T, TN, index, D, Ci, nG = _nnlo_problem()
    walker = np.repeat(np.arange(len(counts)), counts)
    off = _offsets(counts)
    for jeff in (False, True):
        lk = (D, Ci, np.zeros(nG), np.full(nG, 2.0))
        like = MarginalLikelihood(eng, index, *lk, jeffreys=jeff)
        like.set_draw_recipe(rec)
        _, z = _check("nnlo", None, like, rec, theta, off, f, walker, T, index, lk, jeff, templn=TN)
    r = _check_predict(eng, like, rec, theta, off, f, walker, z, 1, True)
    assert np.count_nonzero(r.coef_nnlo) > 0
    eng.close()


def test_split_calls_give_the_same_bits(golden):
    """one batch submitted whole, and split into two calls with other offsets and another S, gives the same bits per sample"""
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe

    g = golden("cfg3")
    nC = 4
    rng = np.random.default_rng(5)
    counts = np.array([40, 0, 1, 90])  # (more draws than one pass of a workgroup's waves)
    eng, templ, index = _cfg3_engine(g, nC, 3 * nC)
    names = [str(n) for n in g["full_names"]]
    nG = len(names)
    pn, theta, f = _cfg3_draws(g, counts, 79)
    rec = joint_draw_recipe(U.bases(), names, U.scales(g), param_names=pn)
    like = MarginalLikelihood(eng, index, g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf))
    like.set_draw_recipe(rec)
    off = _offsets(counts)
    z = _normals(theta.shape[0], 6, nG)
    whole = like.sample_gaussian_params(theta, off, f, z, predict=True, return_coef=True)
    cut = np.array([rng.integers(0, c + 1) for c in counts])
    sel_a = np.concatenate([np.arange(off[c], off[c] + cut[c]) for c in range(nC)])
    sel_b = np.concatenate([np.arange(off[c] + cut[c], off[c + 1]) for c in range(nC)])
    for sel, cnt, ss in ((sel_a, cut, slice(0, 6)), (sel_b, counts - cut, slice(1, 4))):
        part = like.sample_gaussian_params(theta[sel], _offsets(cnt), f, z[sel][:, ss], predict=True, return_coef=True)
        for a, b in zip(part[:3], whole[:3]):
            assert np.array_equal(a, b[sel])
        for a, b in zip(part[3:], whole[3:]):
            assert (a is None and b is None) or np.array_equal(a, b[sel][:, ss])
    d = int(off[3]) + 11
    one = like.sample_gaussian_params(theta[d : d + 1], [0, 0, 0, 0, 1], f, z[d : d + 1, 4])
    assert np.array_equal(one.b[0, 0], whole.b[d, 4]) and one.chi2[0, 0] == whole.chi2[d, 4]
    none = like.sample_gaussian_params(np.zeros((0, 6)), [0, 0, 0, 0, 0], f, np.zeros((0, 2, nG)))
    assert none.b.shape == (0, 2, nG) and none.logp.shape == (0,)
    eng.close()


def test_groups_sample_against_their_own_data(golden):
    """groups= after set_datasets (M = 3): every group against the yardstick evaluated with its own D_m; groups (c, 0) are the call
    without groups bit for bit"""
    from eftpipe_amd.marginal import MarginalLikelihood

    tag = "auto"
    g, eng, T, index = _marg(golden, tag, max_batch=4)
    templ = np.stack([T, T * 1.1])
    eng.put("TEMPL", templ)
    groups = [(1, 2), (0, 0), (1, 0), (0, 1), (1, 1)]
    counts = [3, 0, 2, 4, 1]
    wk, ds = np.array([w for w, _ in groups]), np.array([m for _, m in groups])
    rec, theta, _, _, f = _marg_case(g, tag, [sum(counts)])
    f = f[0] * (1.0 + 0.02 * np.arange(2))
    D, Ci, loc, scale = g[tag + "_D"], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"]
    Ds = datasets(D, Ci, 3)
    assert np.array_equal(Ds[0], D)
    nG = len(loc)
    off = _offsets(counts)
    dw, dm = np.repeat(wk, counts), np.repeat(ds, counts)
    z = _normals(theta.shape[0], S5, nG)
    for jeff in (False, True):
        like = MarginalLikelihood(eng, index, D, Ci, loc, scale, jeffreys=jeff)
        like.set_draw_recipe(rec)
        like.set_datasets(Ds)
        want = like.logp_draws_params(theta, off, f, return_best=True, groups=(wk, ds))
        r = like.sample_gaussian_params(theta, off, f, z, groups=(wk, ds), return_coef=True)
        for a, b in zip(r[:3], want):
            assert np.array_equal(a, b)
        assert r.plk is None and r.coef.shape == (theta.shape[0], S5, 24)
        worst = dict(samples=0.0, identity=0.0)
        for d in range(theta.shape[0]):
            lk = (Ds[dm[d]], Ci, loc, scale)
            y = SU.samples_of_draw(rec, theta[d], f[dw[d]], templ[dw[d] : dw[d] + 1], index, *lk, z[d], jeffreys=jeff)
            worst["samples"] = max(worst["samples"], SU.whitened_error(y["L"], r.b[d], y["b"]))
            worst["identity"] = max(worst["identity"], SU.identity_error(r.chi2[d], r.b[d], r.fullchi2[d], r.best[d], loc, scale, z[d]))
            assert np.allclose(r.chi2[d], SU.chi2_at(rec, theta[d], f[dw[d]], templ[dw[d] : dw[d] + 1], index, lk[0], Ci, r.b[d]), rtol=1e-9, atol=0)
        print("groups", "jeffreys" if jeff else "", ", ".join("%s %.2e" % kv for kv in worst.items()))
        for k, v in worst.items():
            assert v < device_bar(SU.SAMPLE_FLOOR[tag][k]), (k, v)
        # the groups of data set 0, in walker order, are the call without groups
        own = [q for q, (w, m) in enumerate(groups) if m == 0]
        own.sort(key=lambda q: groups[q][0])
        sel = np.concatenate([np.arange(off[q], off[q + 1]) for q in own])
        plain = like.sample_gaussian_params(theta[sel], _offsets([counts[q] for q in own]), f, z[sel], return_coef=True)
        for a, b in zip(plain, r):
            assert (a is None and b is None) or np.array_equal(a, b[sel])
        with pytest.raises(ValueError, match="predict=True does not go with groups"):
            like.sample_gaussian_params(theta, off, f, z, groups=(wk, ds), predict=True)
    eng.close()


def test_failures_and_refusals(golden):
    from eftpipe_amd import _lib as L
    from eftpipe_amd.marginal import MarginalLikelihood, joint_draw_recipe
    from eftpipe_amd.parambasis import DrawRecipe, WestCoastBasis

    g, eng, T, index = _marg(golden, "auto", max_batch=4)
    rec, theta, _, _, f = _marg_case(g, "auto", [2, 2])
    D, Ci = g["auto_D"], g["auto_invcov"]
    nG = len(g["auto_loc"])
    eng.put("TEMPL", np.stack([T, T]))
    off = [0, 2, 4]
    # ---- F2 negative definite with det F2 > 0: two marginalised parameters, a flat prior and the negated inverse covariance
    co = [float(x) for x in g["auto_co"]]
    rec2 = joint_draw_recipe([WestCoastBasis(prefix="")], ["cct", "cr1"], [dict(kmA=co[0], krA=co[1], ndA=co[2])])
    neg = MarginalLikelihood(eng, index, D, -Ci, np.zeros(2), np.full(2, np.inf))
    neg.set_draw_recipe(rec2)
    z2 = _normals(4, 3, 2)
    assert np.all(np.isfinite(neg.logp_draws_params(theta, off, f)))
    raw = neg._sample_raw(theta, off, f, z2, return_coef=True, predict=True)
    assert np.all(np.isfinite(raw.logp)) and np.all(np.isfinite(raw.best)) and np.array_equal(raw.logp, neg.logp_draws_params(theta, off, f))
    assert all(np.all(np.isnan(a)) for a in (raw.b, raw.chi2, raw.coef, raw.plk)) and raw.b.shape == (4, 3, 2)
    with pytest.raises(RuntimeError, match="F2ij is not positive definite"):
        neg.sample_gaussian_params(theta, off, f, z2)
    pos = MarginalLikelihood(eng, index, D, Ci, np.zeros(2), np.full(2, np.inf))  # the same likelihood the right way up
    pos.set_draw_recipe(rec2)
    assert np.all(np.isfinite(pos.sample_gaussian_params(theta, off, f, z2).b))
    # ---- det F2 <= 0 raises as its siblings do: a recipe of row 0 only under a flat prior
    keep = rec.row == 0
    flat = MarginalLikelihood(eng, index, D, Ci, np.zeros(nG), np.full(nG, np.inf))
    flat.set_draw_recipe(DrawRecipe(rec.param_names, 1, nG + 1, rec.tracer[keep], rec.row[keep], rec.col[keep], rec.coef[keep], rec.fpow[keep], rec.idx[keep]))
    z = _normals(4, 3, nG)
    with pytest.raises(RuntimeError, match="det of F2ij"):
        flat.sample_gaussian_params(theta, off, f, z)
    raw = flat._sample_raw(theta, off, f, z)
    assert np.all(np.isnan(raw.logp)) and np.all(np.isnan(raw.b)) and np.all(np.isnan(raw.chi2))
    # ---- refusals
    like = MarginalLikelihood(eng, index, D, Ci, g["auto_loc"], g["auto_scale"])
    with pytest.raises(L.EftbError, match="eftb_draws_sample_params: no draw recipe"):
        like.sample_gaussian_params(theta, off, f, z)
    like.set_draw_recipe(rec)
    want = like.sample_gaussian_params(theta, off, f, z)
    with pytest.raises(ValueError, match="S >= 1 samples per draw"):
        like.sample_gaussian_params(theta, off, f, np.zeros((4, 0, nG)))
    import ctypes as C

    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    th, fo, o64 = np.ascontiguousarray(theta), np.ascontiguousarray(f), np.asarray(off, dtype=np.int64)
    out = [np.zeros(4), np.zeros(4), np.zeros((4, nG)), np.zeros((4, 3, nG)), np.zeros((4, 3))]
    call = lambda S, cn=None: eng.lib.eftb_draws_sample_params(eng._h, 2, 4, S, o64.ctypes.data_as(C.POINTER(C.c_int64)), dp(th), dp(fo), dp(z), *[dp(a) for a in out],
                                                               None, cn, None)
    assert call(0) != 0 and "S = 0" in eng.lib.eftb_last_error().decode()
    cn = np.zeros((4, 3, 1, 3))
    assert call(3, dp(cn)) != 0 and "coefn needs an engine built with with_nnlo" in eng.lib.eftb_last_error().decode()
    assert call(3) == 0 and np.array_equal(out[3], want.b)
    for bad in (np.zeros((4, 3, nG + 1)), np.zeros((3, 3, nG)), np.zeros((4, nG, 3, 1))):
        with pytest.raises(ValueError, match="z must be"):
            like.sample_gaussian_params(theta, off, f, bad)
    zb = z.copy()
    zb[2, 1, 4] = np.nan
    with pytest.raises(L.EftbError, match="z\\[2\\]\\[1\\]\\[4\\] is not finite"):
        like.sample_gaussian_params(theta, off, f, zb)
    with pytest.raises(ValueError, match="predict=True does not go with groups"):
        like.sample_gaussian_params(theta, off, f, z, groups=([0, 1], [0, 0]), predict=True)
    with pytest.raises(L.EftbError, match="eftb_draws_sample_params_datasets: no data sets"):
        like.sample_gaussian_params(theta, off, f, z, groups=([0, 1], [0, 0]))
    assert np.array_equal(like.sample_gaussian_params(theta, off, f, z).b, want.b)
    eng.set_tracers(1)  # drops the recipe (and the likelihood)
    with pytest.raises(L.EftbError, match="eftb_set_likelihood"):
        like.sample_gaussian_params(theta, off, f, z)
    like = MarginalLikelihood(eng, index, D, Ci, g["auto_loc"], g["auto_scale"])
    with pytest.raises(L.EftbError, match="no draw recipe"):
        like.sample_gaussian_params(theta, off, f, z)
    like.set_draw_recipe(rec)
    assert np.array_equal(like.sample_gaussian_params(theta, off, f, z).b, want.b)
    eng.close()
