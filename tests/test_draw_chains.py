"""Metropolis chains over the draw parameters on the host (no GPU): chain_util.host_chain, the NumPy restatement of
eftb_draws_chain_params, against an analytic target and on its edge cases; the helpers proposal_factor and metropolis_proposals; the
inputs of the GPU tests (test_gpu_draw_chains.py), checked here to move and to be refused on every chain; and the argument errors
MarginalLikelihood.metropolis_draws_params raises before it touches the library."""
import numpy as np
import pytest

import cfg3_util as U
import chain_util as CU
import grad_util as GU
from conftest import load_golden

T37, THIN = 37, 5  # a multiple of neither the thinning nor the launch's 256 steps
SEED = 3
DIAG_SCALE, DIAG_BOX = 0.5, 1.0  # cases without a best fit: proposals of half the fixture's dispersion d per parameter, box d beyond the starts


# ----------------------------------------------------------------------------- the acceptance rule against the mathematics
def test_chains_sample_an_analytic_gaussian():
    """256 chains x 400 steps on N(mu, Sigma) in two dimensions from a start dispersed three times as wide, proposals from
    proposal_factor of the exact Hessian, the first half discarded.  The pooled mean and variances agree with the target within 5 Monte-Carlo
    errors, the error taken from the scatter of the per-chain estimates (256 independent chains: their standard deviation / 16).
    Measured with this seed: the means off by 0.5 and 0.2 errors, the variances by 1.2 and 1.8, the covariance by 1.7 (margin: a factor 2.7)."""
    from eftpipe_amd.marginal import metropolis_proposals, proposal_factor

    mu = np.array([1.0, -2.0])
    Sigma = np.array([[2.0, 0.9], [0.9, 0.8]])
    Si = np.linalg.inv(Sigma)
    logp = lambda th: -0.5 * np.einsum("ni,ij,nj->n", th - mu, Si, th - mu)
    N, T = 256, 400
    rng = np.random.default_rng(12)
    theta0 = mu + 3.0 * rng.standard_normal((N, 2)) @ np.linalg.cholesky(Sigma).T
    step, lnu = metropolis_proposals(rng, N, T, proposal_factor(-Si))
    r = CU.host_chain(logp, theta0, step, lnu)
    assert r["theta"].shape == (N, T, 2) and np.all(r["naccept"] > 0.2 * T) and np.all(r["naccept"] < 0.6 * T)
    x = r["theta"][:, T // 2 :] - mu
    est = dict(mean0=x[:, :, 0].mean(1), mean1=x[:, :, 1].mean(1), var0=(x[:, :, 0] ** 2).mean(1) - Sigma[0, 0],
               var1=(x[:, :, 1] ** 2).mean(1) - Sigma[1, 1], cov=(x[:, :, 0] * x[:, :, 1]).mean(1) - Sigma[0, 1])
    for k, v in est.items():
        err = v.std(ddof=1) / np.sqrt(N)
        print("%s: off by %.2e = %.2f Monte-Carlo errors" % (k, v.mean(), abs(v.mean()) / err))
        assert abs(v.mean()) < 5.0 * err, k


# ----------------------------------------------------------------------------- bounds, thinning, NaN
def _walk(N=4, T=23, P=2, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, P)) * 0.1, rng.standard_normal((N, T, P)) * 0.4, np.log(rng.random((N, T)))


def test_thinning_stores_every_thin_th_step_and_last_is_step_T():
    theta0, step, lnu = _walk()
    logp = lambda th: -0.5 * np.sum(th**2, axis=1)
    full = CU.host_chain(logp, theta0, step, lnu)
    thin = CU.host_chain(logp, theta0, step, lnu, thin=5)
    assert thin["theta"].shape == (4, 4, 2) and np.array_equal(thin["theta"], full["theta"][:, 4::5][:, :4])
    assert np.array_equal(thin["logp"], full["logp"][:, 4::5][:, :4]) and np.array_equal(thin["logp"], logp(thin["theta"].reshape(-1, 2)).reshape(4, 4))
    assert np.array_equal(thin["last"], full["theta"][:, -1]) and np.array_equal(thin["naccept"], full["naccept"])
    assert np.all(full["naccept"] > 0) and np.all(full["naccept"] < 23)
    # a chain continued from `last` is the chain run in one piece
    a = CU.host_chain(logp, theta0, step[:, :10], lnu[:, :10])
    b = CU.host_chain(logp, a["last"], step[:, 10:], lnu[:, 10:])
    assert np.array_equal(np.concatenate([a["theta"], b["theta"]], axis=1), full["theta"]) and np.array_equal(a["naccept"] + b["naccept"], full["naccept"])


def test_box_rejects_without_an_evaluation():
    theta0, step, lnu = _walk()
    lower, upper = np.array([-0.5, -np.inf]), np.array([0.5, 0.3])
    theta0 = np.clip(theta0, lower, upper)

    def logp(th):
        assert np.all(th >= lower) and np.all(th <= upper)  # never asked for a point outside the box
        return -0.5 * np.sum(th**2, axis=1)

    r = CU.host_chain(logp, theta0, step, lnu, lower=lower, upper=upper)
    assert np.all(r["outside"] > 0) and np.all(r["theta"] >= lower) and np.all(r["theta"] <= upper)
    plain = lambda th: -0.5 * np.sum(th**2, axis=1)
    free = CU.host_chain(plain, theta0, step, lnu)
    assert not np.array_equal(free["theta"], r["theta"])
    # lnu = -inf accepts every finite proposal inside the box
    r = CU.host_chain(logp, theta0, step, np.full(lnu.shape, -np.inf), lower=lower, upper=upper)
    assert np.array_equal(r["naccept"] + r["outside"], np.full(4, 23))
    # a Gaussian prior on theta moves the chain, one of infinite width does not
    pr = CU.host_chain(logp, theta0, step, lnu, lower=lower, upper=upper, loc=[0.2, 0.0], scale=[0.1, np.inf])
    assert not np.array_equal(pr["theta"], CU.host_chain(logp, theta0, step, lnu, lower=lower, upper=upper)["theta"])
    wide = CU.host_chain(plain, theta0, step, lnu, loc=[0.2, 5.0], scale=[np.inf, np.inf])
    assert np.array_equal(wide["theta"], free["theta"])
    assert np.array_equal(CU.prior_term(np.array([[0.3, 7.0]]), *CU.prior_arrays(2, loc=[0.2, 0.0], scale=[0.1, np.inf])[2:]), [-0.5 * ((0.3 - 0.2) * (1.0 / 0.1)) ** 2])


def test_nan_rejects_a_proposal_and_fails_a_start():
    theta0, step, lnu = _walk()
    theta0[2] = [0.9, 0.0]

    def logp(th):
        return np.where(th[:, 0] > 0.5, np.nan, -0.5 * np.sum(th**2, axis=1))

    r = CU.host_chain(logp, theta0, step, np.full(lnu.shape, -np.inf), thin=2)
    assert r["naccept"][2] == -1 and np.all(np.isnan(r["theta"][2])) and np.all(np.isnan(r["logp"][2])) and np.all(np.isnan(r["last"][2]))
    ok = [0, 1, 3]
    assert np.all(np.isfinite(r["theta"][ok])) and np.all(r["theta"][ok][:, :, 0] <= 0.5)
    assert np.all(r["naccept"][ok] > 0) and np.any(r["naccept"][ok] < 23)  # lnu = -inf: only the NaN proposals were rejected


# ----------------------------------------------------------------------------- the helpers
def test_proposal_factor():
    from eftpipe_amd.marginal import proposal_factor

    rng = np.random.default_rng(0)
    A = rng.standard_normal((5, 4, 6))
    H = -np.einsum("nij,nkj->nik", A, A)
    for hess, scale in ((H, None), (H[0], None), (H, 0.7)):
        L = proposal_factor(hess, scale)
        s2 = (2.38 / 2.0) ** 2 if scale is None else scale**2
        assert L.shape == hess.shape and np.array_equal(L, np.tril(L))
        assert np.allclose(L @ np.swapaxes(L, -1, -2) @ -hess, s2 * np.eye(4), rtol=0, atol=1e-12 * s2)
    bad = H.copy()
    bad[3] = np.diag([-1.0, -1.0, 0.5, -1.0])
    for hess in (bad, -H[0], np.full((2, 2), np.nan)):
        with pytest.raises(ValueError, match="not positive definite"):
            proposal_factor(hess)
    with pytest.raises(ValueError, match="hess must be"):
        proposal_factor(np.zeros((3, 2)))


def test_metropolis_proposals():
    from eftpipe_amd.marginal import metropolis_proposals

    F = np.tril(np.random.default_rng(1).standard_normal((3, 3)))
    step, lnu = metropolis_proposals(np.random.default_rng(5), 7, 11, F)
    assert step.shape == (7, 11, 3) and lnu.shape == (7, 11) and np.all(lnu <= 0.0) and step.flags["C_CONTIGUOUS"]
    rng = np.random.default_rng(5)
    z = rng.standard_normal((7, 11, 3))
    assert np.allclose(step, z @ F.T, rtol=1e-14, atol=1e-15) and np.array_equal(lnu, np.log(rng.random((7, 11))))
    Fn = np.stack([F * (1.0 + n) for n in range(7)])
    sn, _ = metropolis_proposals(np.random.default_rng(5), 7, 11, Fn)
    assert np.allclose(sn, step * (1.0 + np.arange(7))[:, None, None], rtol=1e-14, atol=1e-15)
    big, _ = metropolis_proposals(np.random.default_rng(8), 2, 20000, F)
    assert np.allclose(np.einsum("ntp,ntq->pq", big, big) / 40000, F @ F.T, atol=0.05)
    with pytest.raises(ValueError, match="factor must be"):
        metropolis_proposals(np.random.default_rng(5), 7, 11, Fn[:3])


# ----------------------------------------------------------------------------- the inputs of the device tests
def chain_case(tag):
    """A likelihood of the GPU tests without its engine -> dict(rec, f, counts, walker, ntr, templ [C ntr, nl, 24, nx], templn, index, D, Ci,
    priors [(loc, scale, jeffreys), ...], inp (chain_util.chain_inputs, from the first of the priors), Ws (the walkers' Gram matrices)).
    auto / cross: tests/golden/marg.npz (J + 1 = 25, nG = 7 / 11), walkers with templates scaled by 1 + 0.02 c, one without a chain; auto
    also under a flat prior.  full: tests/golden/cfg3.npz, three tracers (J + 1 = 73, nG = 14).  nnlo: test_gpu_draws_grad._nnlo_problem
    (J + 1 = 28, nG = 9).  auto takes its proposals from the Hessian at the best fits; the others, whose posteriors are too far from
    Gaussian for that, from the dispersion of the fixture's draws."""
    from test_gpu_draws_params import _cfg3_draws, _marg_case

    from eftpipe_amd.marginal import joint_draw_recipe

    templn, ntr = None, 1
    if tag in ("auto", "cross"):
        g = load_golden("marg")
        T, index = GU.marg_templates(g)
        counts = [3, 0, 2, 3]
        templ = np.concatenate([T * (1.0 + 0.02 * c) for c in range(len(counts))])
        rec, center, _, _, f = _marg_case(g, tag, counts)
        D, Ci, loc, scale = g[tag + "_D"], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"]
        nG = len(loc)
        priors = [(loc, scale, False), (loc, scale, True)] + ([(np.zeros(nG), np.full(nG, np.inf), False)] if tag == "auto" else [])
        d = np.array([0.05, 0.3, 0.3] * (1 if tag == "auto" else 2))
    elif tag == "full":
        from test_gpu_draws import _cfg3_block

        g = load_golden("cfg3")
        block, nb = _cfg3_block(g)
        counts, ntr = [2, 0, 1, 3], 3
        templ = np.concatenate([(1.0 + 0.02 * c) * block for c in range(len(counts))])
        names = [str(n) for n in g["full_names"]]
        pn, center, f = _cfg3_draws(g, counts, 9)
        rec = joint_draw_recipe(U.bases(), names, U.scales(g), param_names=pn)
        index, D, Ci, nG = GU.cfg3_index(g, nb), g["data_vector"], g["invcov"], len(names)
        priors = [(np.zeros(nG), np.full(nG, np.inf), True), (np.zeros(nG), np.full(nG, np.inf), False)]
        d = np.full(6, 0.05)
    else:
        from eftpipe_amd.parambasis import WestCoastBasis, gaussian_params

        templ, templn, index, D, Ci, center, f, counts = CU.nnlo_arrays()
        basis = WestCoastBasis(prefix="")
        names = gaussian_params("") + basis.cnnloA()
        rec = joint_draw_recipe([basis], names, [dict(kmA=0.7, krA=0.25, ndA=4.5e-5)], with_NNLO=True)
        nG = len(names)
        priors = [(np.zeros(nG), np.full(nG, 2.0), False), (np.zeros(nG), np.full(nG, 2.0), True)]
        d = np.full(3, 0.2)
    walker = np.repeat(np.arange(len(counts)), counts)
    fw = np.reshape(f, (len(counts), ntr))
    Ws = [GU.gram_matrix(templ[c * ntr : (c + 1) * ntr], index, D, Ci, None if templn is None else templn[c * ntr : (c + 1) * ntr]) for c in range(len(counts))]
    case = dict(rec=rec, f=f, counts=counts, walker=walker, ntr=ntr, templ=templ, templn=templn, index=index, D=D, Ci=Ci, priors=priors, Ws=Ws, fw=fw)
    if tag == "auto":
        case["inp"] = CU.best_fit_inputs(host_target(case, 0).hess, np.tile(center[0], (len(walker), 1)), SEED, T37)
    else:
        case["inp"] = CU.chain_inputs(center, np.diag(d) * DIAG_SCALE, np.tile(d, (len(walker), 1)), SEED, T37, box=DIAG_BOX)
    return case


def host_target(case, i):
    """the target of prior i of a case on the host (the Gram route in NumPy)"""
    w = case["walker"]
    return CU.HostTarget(case["rec"], case["fw"][w], [case["Ws"][c] for c in w], *case["priors"][i])


def mixed(r, T):
    """every chain moved, was refused, and met the box"""
    return bool(np.all(r["naccept"] > 0) and np.all(r["naccept"] < T) and np.all(r["outside"] > 0))


@pytest.mark.parametrize("tag", ["auto", "cross", "full", "nnlo"])
def test_device_inputs_move_and_are_refused_on_every_chain(tag):
    """the inputs the GPU tests feed to the device give every chain 0 < naccept < T and at least one proposal outside the box, under every
    prior of the case: a device test cannot pass on a chain that never moves or never refuses.  ln P here is the Gram route in NumPy."""
    case = chain_case(tag)
    inp = case["inp"]
    N = len(case["walker"])
    assert 6 <= N <= 12 and inp["theta0"].shape == (N, len(case["rec"].param_names)) and inp["step"].shape[:2] == (N, T37)
    assert np.all(inp["theta0"] >= inp["lower"]) and np.all(inp["theta0"] <= inp["upper"])
    for i in range(len(case["priors"])):
        r = CU.host_chain(host_target(case, i).logp, inp["theta0"], inp["step"], inp["lnu"], THIN, inp["lower"], inp["upper"])
        print(tag, i, "naccept", r["naccept"], "outside the box", r["outside"])
        assert mixed(r, T37) and r["theta"].shape[1] == T37 // THIN


def long_inputs():
    """the T = 300 call of the GPU tests (auto, the first 3 chains): it crosses the launch boundary at 256 steps"""
    case = chain_case("auto")
    inp = CU.best_fit_inputs(host_target(case, 0).hess, case["inp"]["theta0"], SEED + 1, 300)
    return case, {k: (v[:3] if k in ("theta0", "step", "lnu") else v) for k, v in inp.items()}


def test_long_inputs_move_on_both_sides_of_the_launch_boundary():
    case, inp = long_inputs()
    tg = host_target(case, 0)
    tg.fs, tg.Ws = tg.fs[:3], tg.Ws[:3]
    r = CU.host_chain(tg.logp, inp["theta0"], inp["step"], inp["lnu"], 1, inp["lower"], inp["upper"])
    moved = np.any(np.diff(r["theta"], axis=1) != 0.0, axis=2)  # [3, 299]: step t + 1 was accepted
    assert mixed(r, 300) and np.all(moved[:, :255].sum(1) > 0) and np.all(moved[:, 256:].sum(1) > 0)


# ----------------------------------------------------------------------------- argument errors raised before the library is touched
class _NoLib:
    def __getattr__(self, name):
        raise AssertionError("the library was touched: " + name)


def _like(P=3, nG=7):
    from eftpipe_amd.marginal import MarginalLikelihood

    like = MarginalLikelihood.__new__(MarginalLikelihood)
    like.eng = type("E", (), dict(ntracers=1, lib=_NoLib(), _h=None))()
    like.nG = nG
    like._recipe = type("R", (), dict(param_names=["a", "b", "c"][:P]))()
    return like


def test_argument_errors_before_the_library():
    like = _like()
    N, T = 4, 6
    theta0, off, f = np.zeros((N, 3)), [0, 2, 4], [0.7, 0.8]
    step, lnu = np.zeros((N, T, 3)), np.zeros((N, T))
    for bad in (np.zeros((N, T, 2)), np.zeros((N + 1, T, 3)), np.zeros((N, 3)), np.zeros((N, 0, 3))):
        with pytest.raises(ValueError, match="step must be"):
            like.metropolis_draws_params(theta0, off, f, bad, lnu)
    for bad in (np.zeros((N, T + 1)), np.zeros(N), np.zeros((N, T, 1))):
        with pytest.raises(ValueError, match="lnu must be"):
            like.metropolis_draws_params(theta0, off, f, step, bad)
    for bad in (0, T + 1, -1, 2.5):
        with pytest.raises(ValueError, match="thin must be"):
            like.metropolis_draws_params(theta0, off, f, step, lnu, thin=bad)
    for name in ("lower", "upper", "prior_loc", "prior_scale"):
        with pytest.raises(ValueError, match=name + " must be"):
            like.metropolis_draws_params(theta0, off, f, step, lnu, **{name: np.zeros(2)})
    with pytest.raises(ValueError, match="theta must be"):
        like.metropolis_draws_params(np.zeros((N, 2)), off, f, step, lnu)
    with pytest.raises(AssertionError, match="the library was touched"):
        like.metropolis_draws_params(theta0, off, f, step, lnu)
    import eftpipe_amd.marginal as M

    assert all(n in M.__all__ for n in ("DrawChains", "metropolis_proposals", "proposal_factor"))
