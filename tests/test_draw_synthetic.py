"""The synthetic likelihoods of synth_like_util.py on the host (no GPU): what the GPU tests (test_gpu_draw_synthetic.py) lean on.

  * the oracle (oracle.marginal.marginalized_logp on grad_util.recipe_vectors) against an evaluation of F0, F1, F2, b = F2^-1 F1 and
    ln det (F2 / 2 pi) with mpmath at 50 digits: ln P, the full chi2 and the best fit
  * the floors: the NumPy restatements of the kernels' Gram route against the data-space yardsticks, asserted against
    synth_like_util.SYNTH_FLOOR, from which the device's bars follow
  * the input conditions that keep the GPU tests from hiding a failure: every regular draw is positive definite, the LU of F2 exchanges
    rows, a deliberately singular draw has an exactly zero row and column of F2"""
import numpy as np
import pytest

import grad_util as GU
import sample_util as SU
import synth_like_util as SY
from hess_util import device_bar

ALL = [(c, k) for c in SY.CASES for k in SY.kinds(c)]
MP_DRAWS = (0, 8, 13)  # walker 0's first and last draw and walker 2's last: the 50-digit evaluation is slow


def _mp_evaluation(V, D, invcov, loc, scale, jeffreys):
    """ln P, full chi2 and best from the doubles V, D, invcov, loc, scale taken as exact, every operation at 50 digits"""
    import mpmath as mp

    mp.mp.dps = 50
    tomp = np.vectorize(lambda x: mp.mpf(float(x)), otypes=[object])
    Vm, Cm = tomp(V), tomp(invcov)
    Vm[0] = Vm[0] - tomp(D)
    nG = V.shape[0] - 1
    G = Vm.dot(Cm).dot(Vm.T)
    flat = bool(np.any(np.isinf(scale)))
    sinv = [mp.mpf(0) if flat else 1 / mp.mpf(float(s)) ** 2 for s in scale]
    mu = [mp.mpf(float(m)) for m in loc]
    F2 = mp.matrix(nG, nG)
    for i in range(nG):
        for j in range(nG):
            F2[i, j] = G[1 + i, 1 + j] + (sinv[i] if i == j else 0)
    F1 = mp.matrix([-G[1 + i, 0] + sinv[i] * mu[i] for i in range(nG)])
    F0 = G[0, 0] + sum(m * m * s for m, s in zip(mu, sinv))
    b = mp.lu_solve(F2, F1)
    f1b = sum(F1[i] * b[i] for i in range(nG))
    logdet = mp.log(mp.det(F2 / (2 * mp.pi)))
    v = np.array([mp.mpf(1)] + [b[i] for i in range(nG)], dtype=object)
    full = v.dot(G).dot(v)
    return float(-(F0 - f1b + (0 if jeffreys else logdet)) / 2), float(full), np.array([float(b[i]) for i in range(nG)])


@pytest.mark.parametrize("case,kind", ALL)
def test_oracle_against_fifty_digits(case, kind):
    """The yardstick of ln P, full chi2 and best is right to a tenth of the bar the device is held to (hess_util.device_bar of the recorded
    floor), the usual ratio between a reference's uncertainty and the tolerance it checks.  ln P and the full chi2 sit four orders below
    it; best, in whitened units, carries the rounding of the oracle's own solve, a few thousand unit roundoffs at nG = 24, which is also
    most of what the recorded floor of best is."""
    pb = SY.case_problem(case, kind)
    worst = dict(logp=0.0, fullchi2=0.0, best=0.0, gram=0.0)
    for jeff in SY.jeffreys_of(case, kind):
        ref = SY.reference(case, kind, jeff)
        for d in MP_DRAWS:
            y = ref[d]
            logp, full, best = _mp_evaluation(y["V"], pb.D, pb.invcov, pb.loc, pb.scale, jeff)
            worst["logp"] = max(worst["logp"], abs(y["logp"] - logp) / y["scale"])
            worst["fullchi2"] = max(worst["fullchi2"], abs(y["fullchi2"] - full) / y["chi2scale"])
            worst["best"] = max(worst["best"], SU.whitened_error(y["L"], y["best"], best))
            ff, tw, tn = SY.of_walker(pb, pb.walker[d])
            W = GU.gram_matrix(tw, pb.index, pb.D, pb.invcov, tn)
            worst["gram"] = max(worst["gram"], abs(SY.CU.gram_record(pb.rec, pb.theta[d], ff, W, pb.loc, pb.scale, jeff) - logp) / y["scale"])
    print(case, kind, "oracle against 50 digits:", ", ".join("%s %.1e" % kv for kv in worst.items()), "(gram: chain_util.gram_record)")
    for k in ("logp", "fullchi2", "best"):
        assert worst[k] < 0.1 * device_bar(SY.floor_of(case, kind, k)), (k, worst[k])


@pytest.mark.parametrize("case,kind", ALL)
def test_gram_route_floors(case, kind):
    """gram_record, gram_samples, gram_adjoint and gram_hessian against the data-space yardsticks on every draw, Jeffreys off and on: the
    worst values are those recorded in SYNTH_FLOOR, which is this test's print-out (at most 1.5 times them, the margin the sibling floor
    tests leave for another NumPy / BLAS, and not more than tenfold below)"""
    pb = SY.case_problem(case, kind)
    z = SY.normals(pb.theta.shape[0], SY.S5, pb.nG)
    errs = []
    for jeff in SY.jeffreys_of(case, kind):
        ref = SY.reference(case, kind, jeff)
        errs += [SY.errors(pb, d, ref[d], z[d], *SY.gram_route(pb, d, z[d], jeff)) for d in range(pb.theta.shape[0])]
    got = SY.worst(errs)
    print(case, kind, "floors:", "dict(" + ", ".join("%s=%.1e" % (k, got[k]) for k in SY.QUANTITIES) + ")")
    for k in SY.QUANTITIES:
        rec = SY.floor_of(case, kind, k)
        assert got[k] <= 1.5 * rec, (k, got[k], rec)  # (1.5: another NumPy / BLAS rounds differently)
        assert rec <= max(10.0 * got[k], 1e-13), (k, got[k], rec)  # (below 1e-13 every floor gives the same bar: not pinned further)
        assert device_bar(rec) < 1e-6, (k, rec)  # a benign construction: the bars that follow stay meaningful


@pytest.mark.parametrize("ndata", list(SY.WIDE))
def test_wide_logp_floors(ndata):
    """The likelihoods past one column group of the U = V C^-1 product (ndata = 128, 129, 257; the LOGP stage alone): ln P, full chi2 and
    best of the Gram route against the data-space yardstick on every draw, Jeffreys off and on -- the worst values are those recorded in
    WIDE_FLOOR (pinned as test_gram_route_floors pins SYNTH_FLOOR), and every draw is positive definite"""
    pb = SY.wide_problem(ndata)
    assert pb.ndata == ndata and pb.index.size == ndata and np.array_equal(pb.invcov, pb.invcov.T)
    assert set(pb.index // (pb.nl * pb.nx)) == set(range(pb.ntr))
    errs = []
    for jeff in (False, True):
        ref = SY.wide_reference(ndata, jeff)
        for d, y in enumerate(ref):
            assert np.isfinite(y["logp"]) and np.all(np.linalg.eigvalsh(y["F2"]) > 0)
            ff, tw, tn = SY.of_walker(pb, pb.walker[d])
            W = GU.gram_matrix(tw, pb.index, pb.D, pb.invcov, tn)
            logp = SY.CU.gram_record(pb.rec, pb.theta[d], ff, W, pb.loc, pb.scale, jeff)
            best, _, _, full = SU.gram_samples(pb.rec, pb.theta[d], ff, W, pb.loc, pb.scale, np.zeros((1, pb.nG)))
            errs.append(SY.errors(pb, d, y, None, logp, full, best, None, None, None, None, None))
    got = SY.worst(errs)
    print("ndata %d floors:" % ndata, "dict(" + ", ".join("%s=%.1e" % kv for kv in got.items()) + ")")
    for k in ("logp", "fullchi2", "best"):
        rec = SY.WIDE_FLOOR[ndata][k]
        assert got[k] <= 1.5 * rec, (k, got[k], rec)
        assert rec <= max(10.0 * got[k], 1e-13), (k, got[k], rec)
        assert device_bar(rec) < 1e-6, (k, rec)


@pytest.mark.parametrize("case,kind", ALL)
def test_input_conditions(case, kind):
    """every draw has a finite ln P and finite samples (F2 positive definite: the yardsticks' Cholesky factor exists), all theta are
    distinct, the index touches every tracer, and from nG = 3 on the partially pivoted LU of F2 exchanges rows on some draw"""
    from scipy.linalg import lu

    pb = SY.case_problem(case, kind)
    assert pb.counts == SY.COUNTS and np.unique(pb.theta, axis=0).shape[0] == pb.theta.shape[0]
    if pb.ndata >= pb.ntr:
        assert set(pb.index // (pb.nl * pb.nx)) == set(range(pb.ntr))
    assert np.array_equal(pb.invcov, pb.invcov.T) and 5e2 < np.linalg.cond(pb.invcov) < 2e3
    exchanged = 0
    for y in SY.reference(case, kind):
        assert np.isfinite(y["logp"]) and np.all(np.isfinite(y["b"])) and np.all(np.isfinite(y["chi2"])) and np.all(np.linalg.eigvalsh(y["F2"]) > 0)
        perm = lu(y["F2"])[0]
        exchanged = max(exchanged, int(np.sum(np.argmax(perm, axis=0) != np.arange(pb.nG))))
    print(case, kind, "rows the LU of F2 moves, at most:", exchanged)
    if pb.nG >= 3:
        assert exchanged > 0


@pytest.mark.parametrize("case", ["Ef", "Gf", "I"])
def test_singular_draw_is_exactly_singular(case):
    """the deliberately singular draw of the GPU tests: Gaussian row g carries a factor theta_0 in every term, the draw has theta_0 = 0 and
    the prior is flat -> row g of the model is exactly zero, and so are row and column g of F2 by either route: the pivot is 0, not noise"""
    g = SY.CASES[case]["nG"] // 2 + 1
    pb = SY.case_problem(case, "flat", singular=g)
    d = 4
    th = pb.theta[d].copy()
    th[0] = 0.0
    ff, tw, tn = SY.of_walker(pb, pb.walker[d])
    V, _ = GU.recipe_vectors(pb.rec, th, ff, tw, pb.index, tn)
    assert not np.any(V[g]) and np.count_nonzero(V) > 0
    F2 = V[1:] @ pb.invcov @ V[1:].T
    assert not np.any(F2[g - 1]) and not np.any(F2[:, g - 1])
    _, G = SU.gram_G(pb.rec, th, ff, GU.gram_matrix(tw, pb.index, pb.D, pb.invcov, tn))
    assert not np.any(G[g]) and not np.any(G[:, g])
    # the same recipe at the draw's own theta_0 is regular
    V, _ = GU.recipe_vectors(pb.rec, pb.theta[d], ff, tw, pb.index, tn)
    assert np.all(np.linalg.eigvalsh(V[1:] @ pb.invcov @ V[1:].T) > 0)
