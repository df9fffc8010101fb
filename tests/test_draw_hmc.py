"""Hamiltonian Monte Carlo over the draw parameters on the host (no GPU): hmc_util.host_hmc, the NumPy restatement of eftb_draws_hmc_params,
against an analytic target, its reversibility and the order of its energy error, and on its edge cases; the helper hmc_momenta; the inputs
of the GPU tests (test_gpu_draw_hmc.py), checked here to move, to be refused and to leave the box; and the argument errors
MarginalLikelihood.hmc_draws_params raises before it touches the library."""
import functools

import numpy as np
import pytest

import grad_util as GU
import hmc_util as HM
import synth_like_util as SY
from test_draw_chains import _like, chain_case, host_target

T11, NLEAP, THIN = 11, 4, 3
SEED = 5
# the step size of trajectory (n, t) is EPS[variant] times a log-uniform factor in [JIT_LO, JIT_HI]: wide enough for every chain to meet steps it accepts and
# steps it refuses within 11 trajectories
JIT_LO, JIT_HI = 0.2, 3.0


def _gauss(mu, Sigma):
    Si = np.linalg.inv(Sigma)
    return lambda th: (-0.5 * np.einsum("ni,ij,nj->n", th - mu, Si, th - mu), -(th - mu) @ Si)


# ----------------------------------------------------------------------------- the algorithm against the mathematics
def test_trajectories_sample_an_analytic_gaussian():
    """256 chains x 200 trajectories of 5 leapfrog steps on N(mu, Sigma) in two dimensions from a start dispersed three times as wide, F the
    Cholesky factor of Sigma, the step size jittered around 0.8, the first half discarded.  The pooled means, variances and covariance agree
    with the target within 5 Monte-Carlo errors, the error taken from the scatter of the per-chain estimates (the criterion of
    test_draw_chains.test_chains_sample_an_analytic_gaussian)."""
    from eftpipe_amd.marginal import hmc_momenta

    mu = np.array([1.0, -2.0])
    Sigma = np.array([[2.0, 0.9], [0.9, 0.8]])
    N, T = 256, 200
    rng = np.random.default_rng(12)
    F = np.linalg.cholesky(Sigma)
    theta0 = mu + 3.0 * rng.standard_normal((N, 2)) @ F.T
    mom, lnu = hmc_momenta(rng, N, T, 2)
    eps = 0.8 * rng.uniform(0.8, 1.2, (N, T))
    r = HM.host_hmc(_gauss(mu, Sigma), theta0, mom, lnu, eps, 5, factor=F)
    print("acceptance", r["naccept"].mean() / T)
    assert r["theta"].shape == (N, T, 2) and np.all(r["naccept"] > 0.7 * T) and np.all(r["naccept"] < T) and np.all(r["refused"] > 0) and not np.any(r["aborted"])
    x = r["theta"][:, T // 2 :] - mu
    est = dict(mean0=x[:, :, 0].mean(1), mean1=x[:, :, 1].mean(1), var0=(x[:, :, 0] ** 2).mean(1) - Sigma[0, 0],
               var1=(x[:, :, 1] ** 2).mean(1) - Sigma[1, 1], cov=(x[:, :, 0] * x[:, :, 1]).mean(1) - Sigma[0, 1])
    for k, v in est.items():
        err = v.std(ddof=1) / np.sqrt(N)
        print("%s: off by %.2e = %.2f Monte-Carlo errors" % (k, v.mean(), abs(v.mean()) / err))
        assert abs(v.mean()) < 5.0 * err, k


def _one(fun, theta, r, eps, nleap, F):
    N, P = theta.shape
    inf = np.full(P, np.inf)
    g = HM.target_grad(fun(theta)[1], theta, np.zeros(P), np.zeros(P))
    return HM.trajectory(fun, theta, g, r, np.full(N, eps), nleap, HM.factors(F, N, P), -inf, inf, np.zeros(P), np.zeros(P), theta)


def test_a_trajectory_is_reversible():
    """the momentum negated after a trajectory and the trajectory run again: the start comes back to a few ulp of the path length (every
    leapfrog step is undone by the same operations up to their rounding, 2 nleap of them here)"""
    rng = np.random.default_rng(3)
    mu, Sigma = np.array([1.0, -2.0]), np.array([[2.0, 0.9], [0.9, 0.8]])
    fun, F = _gauss(mu, Sigma), np.linalg.cholesky(Sigma)
    theta, r = mu + rng.standard_normal((16, 2)) @ F.T, rng.standard_normal((16, 2))
    nleap, eps = 20, 0.2
    t1, r1, *_ = _one(fun, theta, r, eps, nleap, F)
    t2, r2, *_ = _one(fun, t1, -r1, eps, nleap, F)
    path = eps * nleap * np.abs(F).sum()
    assert np.max(np.abs(t1 - theta)) > 0.1
    print("returned to", np.max(np.abs(t2 - theta)), "of", path)
    assert np.max(np.abs(t2 - theta)) <= 2 * nleap * 4 * np.finfo(float).eps * path and np.max(np.abs(r2 + r)) <= 2 * nleap * 4 * np.finfo(float).eps * np.max(np.abs(r)) * 4


def test_the_energy_error_is_second_order():
    """at fixed path length eps nleap the energy error of a trajectory falls by about 4 when eps halves (a non-Gaussian target: a quartic well)"""
    fun = lambda th: (-0.25 * np.sum(th**4, axis=1) - 0.5 * np.sum(th**2, axis=1), -(th**3) - th)
    rng = np.random.default_rng(4)
    theta, r = rng.standard_normal((32, 3)), rng.standard_normal((32, 3))
    err = []
    for nleap in (8, 16, 32):
        t1, r1, lp1, *_ = _one(fun, theta, r, 0.4 / nleap, nleap, None)
        err.append(np.abs((lp1 - HM.kinetic(r1)) - (fun(theta)[0] - HM.kinetic(r))))
    ratios = [np.median(err[0] / err[1]), np.median(err[1] / err[2])]
    print("energy error ratios", ratios)
    assert all(3.0 < q < 5.0 for q in ratios)


# ----------------------------------------------------------------------------- thinning, the box, NaN, the factor
def _walk(N=4, T=23, P=2, seed=1):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, P)) * 0.3, rng.standard_normal((N, T, P)), np.log(rng.random((N, T))), rng.uniform(0.9, 1.98, (N, T))


_quad = lambda th: (-0.5 * np.sum(th**2, axis=1), -th)


def test_thinning_last_and_continuation():
    theta0, mom, lnu, eps = _walk()
    full = HM.host_hmc(_quad, theta0, mom, lnu, eps, 3)
    thin = HM.host_hmc(_quad, theta0, mom, lnu, eps, 3, thin=5)
    assert thin["theta"].shape == (4, 4, 2) and np.array_equal(thin["theta"], full["theta"][:, 4::5][:, :4])
    assert np.array_equal(thin["logp"], full["logp"][:, 4::5][:, :4]) and np.array_equal(thin["logp"], _quad(thin["theta"].reshape(-1, 2))[0].reshape(4, 4))
    assert np.array_equal(thin["last"], full["theta"][:, -1]) and np.array_equal(thin["naccept"], full["naccept"])
    assert np.array_equal(thin["log_ratio"], full["log_ratio"]) and np.all(np.isfinite(full["log_ratio"]))
    assert np.all(full["naccept"] > 0) and np.all(full["naccept"] < 23)
    # accepted iff lnu < log_ratio
    assert np.array_equal(full["naccept"], np.sum(lnu < full["log_ratio"], axis=1))
    # a chain continued from `last` is the chain run in one piece
    a = HM.host_hmc(_quad, theta0, mom[:, :10], lnu[:, :10], eps[:, :10], 3)
    b = HM.host_hmc(_quad, a["last"], mom[:, 10:], lnu[:, 10:], eps[:, 10:], 3)
    assert np.array_equal(np.concatenate([a["theta"], b["theta"]], axis=1), full["theta"]) and np.array_equal(a["naccept"] + b["naccept"], full["naccept"])
    assert np.array_equal(np.concatenate([a["log_ratio"], b["log_ratio"]], axis=1), full["log_ratio"])
    # eps as a scalar and per chain
    assert np.array_equal(HM.host_hmc(_quad, theta0, mom, lnu, 0.7, 3)["theta"], HM.host_hmc(_quad, theta0, mom, lnu, np.full((4, 23), 0.7), 3)["theta"])
    assert np.array_equal(HM.host_hmc(_quad, theta0, mom, lnu, eps[:, 0], 3)["theta"], HM.host_hmc(_quad, theta0, mom, lnu, np.tile(eps[:, :1], (1, 23)), 3)["theta"])


def test_box_aborts_without_an_evaluation_outside():
    theta0, mom, lnu, eps = _walk()
    lower, upper = np.array([-0.8, -np.inf]), np.array([0.8, 0.6])
    theta0 = np.clip(theta0, lower, upper)

    def fun(th):
        assert np.all(th >= lower) and np.all(th <= upper)  # never asked for a point outside the box
        return _quad(th)

    r = HM.host_hmc(fun, theta0, mom, lnu, eps, 3, lower=lower, upper=upper)
    assert np.all(r["outside"] > 0) and np.all(r["theta"] >= lower) and np.all(r["theta"] <= upper) and np.array_equal(r["outside"], r["aborted"])
    assert np.array_equal(np.isnan(r["log_ratio"]).sum(1), r["outside"])
    assert not np.array_equal(HM.host_hmc(_quad, theta0, mom, lnu, eps, 3)["theta"], r["theta"])
    # lnu = -inf accepts every trajectory that is not aborted
    r = HM.host_hmc(fun, theta0, mom, np.full(lnu.shape, -np.inf), eps, 3, lower=lower, upper=upper)
    assert np.array_equal(r["naccept"] + r["outside"], np.full(4, 23)) and not np.any(r["refused"])
    # a Gaussian prior on theta moves the chain through value and gradient, one of infinite width does not
    pr = HM.host_hmc(fun, theta0, mom, lnu, eps, 3, lower=lower, upper=upper, loc=[0.2, 0.0], scale=[0.3, np.inf])
    assert not np.array_equal(pr["theta"], HM.host_hmc(fun, theta0, mom, lnu, eps, 3, lower=lower, upper=upper)["theta"])
    wide = HM.host_hmc(_quad, theta0, mom, lnu, eps, 3, loc=[0.2, 5.0], scale=[np.inf, np.inf])
    assert np.array_equal(wide["theta"], HM.host_hmc(_quad, theta0, mom, lnu, eps, 3)["theta"])
    # the prior as part of the target: the same chain up to rounding as the function with the prior folded in
    s = np.array([0.3, 0.5])
    both = lambda th: (_quad(th)[0] - 0.5 * np.sum(((th - 0.2) / s) ** 2, axis=1), -th - (th - 0.2) / s**2)
    a = HM.host_hmc(_quad, theta0, mom[:, :1], lnu[:, :1], 0.1, 3, loc=[0.2, 0.2], scale=s)
    b = HM.host_hmc(both, theta0, mom[:, :1], lnu[:, :1], 0.1, 3)
    assert np.allclose(a["log_ratio"], b["log_ratio"], rtol=0, atol=1e-12) and np.allclose(a["last"], b["last"], rtol=0, atol=1e-13)


def test_nan_aborts_a_trajectory_and_fails_a_start():
    theta0, mom, lnu, eps = _walk()
    theta0[2] = [0.9, 0.0]

    def fun(th):
        bad = th[:, 0] > 0.5
        return np.where(bad, np.nan, _quad(th)[0]), np.where(bad[:, None], np.nan, _quad(th)[1])

    r = HM.host_hmc(fun, theta0, mom, np.full(lnu.shape, -np.inf), eps, 3, thin=2)
    assert r["naccept"][2] == -1 and all(np.all(np.isnan(r[k][2])) for k in ("theta", "logp", "last", "log_ratio"))
    ok = [0, 1, 3]
    assert np.all(np.isfinite(r["theta"][ok])) and np.all(r["theta"][ok][:, :, 0] <= 0.5)
    assert np.all(r["naccept"][ok] > 0) and np.any(r["naccept"][ok] < 23) and np.array_equal(r["naccept"][ok] + r["aborted"][ok], [23] * 3)
    assert not np.any(r["outside"])
    # a gradient component that is not finite aborts as well
    gnan = lambda th: (_quad(th)[0], np.where((th[:, 0] > 0.5)[:, None], np.inf, _quad(th)[1]))
    r2 = HM.host_hmc(gnan, np.delete(theta0, 2, 0), np.delete(mom, 2, 0), np.full((3, 23), -np.inf), np.delete(eps, 2, 0), 3)
    assert np.any(r2["aborted"] > 0) and np.all(r2["theta"][:, :, 0] <= 0.5)


def test_no_factor_is_the_identity():
    theta0, mom, lnu, eps = _walk()
    a, b = HM.host_hmc(_quad, theta0, mom, lnu, eps, 3), HM.host_hmc(_quad, theta0, mom, lnu, eps, 3, factor=np.eye(2))
    for k in ("theta", "logp", "last", "naccept", "log_ratio"):
        assert np.array_equal(a[k], b[k]), k
    # what lies above the diagonal is not read
    F = np.array([[0.7, 123.0], [0.2, 1.1]])
    assert np.array_equal(HM.host_hmc(_quad, theta0, mom, lnu, eps, 3, factor=F)["theta"], HM.host_hmc(_quad, theta0, mom, lnu, eps, 3, factor=np.tril(F))["theta"])


def test_hmc_momenta():
    from eftpipe_amd.marginal import hmc_momenta

    mom, lnu = hmc_momenta(np.random.default_rng(5), 7, 11, 3)
    rng = np.random.default_rng(5)
    assert np.array_equal(mom, rng.standard_normal((7, 11, 3))) and np.array_equal(lnu, np.log(rng.random((7, 11)))) and np.all(lnu <= 0.0)
    with pytest.raises(ValueError, match="T must be"):
        hmc_momenta(rng, 7, 0, 3)


# ----------------------------------------------------------------------------- the inputs of the device tests
class GradTarget:
    """ln P and its gradient of N chains on the host by the Gram route (grad_util.gram_adjoint), NaN where det F2 <= 0 (chain_util.gram_record)"""

    def __init__(self, tg):
        self.tg = tg

    def __call__(self, theta):
        tg = self.tg
        out = [GU.gram_adjoint(tg.rec, th, f, W, *tg.lk) for th, f, W in zip(theta, tg.fs, tg.Ws)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])


# per case: the box reaches BOX dispersions d beyond the outermost starts (wider than the Metropolis tests' box: a trajectory follows the
# gradient, and from a start off the mode it runs a long way), then the leapfrog step size without a factor (in units of theta) and with one
# (in units of the whitened space)
DISP = dict(auto=[0.05, 0.3, 0.3], cross=[0.05, 0.3, 0.3] * 2, full=[0.05] * 6, nnlo=[0.2] * 3)
BOUND = dict(auto=0, cross=0, full=2, nnlo=2)
BOX = dict(auto=3.0, cross=3.0, full=3.0, nnlo=3.0)
EPS = dict(auto=(0.08, 1.5), cross=(0.055, 0.85), full=(0.065, 1.2), nnlo=(0.012, 0.06))
# the step size of a chain relative to the case's, as a caller's adaptation would leave it: the starts of the NNLO case lie on slopes of very
# different curvature
CHAIN_EPS = dict(nnlo=[1.0, 1.0, 1.0, 1.0, 1.6, 1.0, 1.0, 1.0, 2.5, 1.0])


@functools.lru_cache(maxsize=None)
def hmc_case(tag, T=T11, seed=SEED, box=None, eps=None, bound=None):
    """The inputs of the device tests on a case of test_draw_chains.chain_case -> dict(case, theta0, lower, upper, prior_loc, prior_scale (a
    Gaussian prior on theta: the middle of the box, half its width), mom, lnu, variants = [(name, factor, eps [N, T]), ...]): without a
    factor, and with one -- auto: proposal_factor(H, scale=1.0) of each chain's best fit; the others, whose posteriors are too far from
    Gaussian for that, the diagonal of the dispersions their Metropolis proposals use."""
    from eftpipe_amd.marginal import hmc_momenta, newton_maximize, proposal_factor

    case = chain_case(tag)
    theta0 = case["inp"]["theta0"]
    N, P = theta0.shape
    d = np.array(DISP[tag])
    box = BOX[tag] if box is None else box
    lower, upper = theta0.min(0) - box * d, theta0.max(0) + box * d
    free = np.arange(P) != (BOUND[tag] if bound is None else bound)
    lower[free], upper[free] = -np.inf, np.inf  # (one parameter alone is bounded: along the others a trajectory that runs away is refused for its energy)
    if tag == "auto":
        _, _, _, H, _, conv = newton_maximize(host_target(case, 0).hess, theta0)
        assert np.all(conv)
        F = proposal_factor(H, scale=1.0)
    else:
        F = np.diag(d)
    rng = np.random.default_rng(seed)
    mom, lnu = hmc_momenta(rng, N, T, P)
    jit = np.exp(rng.uniform(np.log(JIT_LO), np.log(JIT_HI), (N, T))) * np.array(CHAIN_EPS.get(tag, [1.0] * N))[:, None]
    e0, e1 = EPS[tag] if eps is None else eps
    ploc, pscale = np.where(free, 0.0, 0.5 * (np.where(free, 0.0, lower) + np.where(free, 0.0, upper))), 0.5 * (upper - lower)  # (scale inf: no prior on that parameter)
    return dict(case=case, theta0=theta0, lower=lower, upper=upper, prior_loc=ploc, prior_scale=pscale, mom=mom, lnu=lnu,
                variants=[("none", None, e0 * jit), ("factor", F, e1 * jit)])


def mixed(r, T):
    """every chain moved and was refused; some trajectory left the box and some was refused without leaving it"""
    return bool(np.all(r["naccept"] > 0) and np.all(r["naccept"] < T) and r["outside"].sum() > 0 and r["refused"].sum() > 0)


@pytest.mark.parametrize("tag", ["auto", "cross", "full", "nnlo"])
def test_device_inputs_move_abort_and_are_refused(tag):
    """the inputs the GPU tests feed to the device give every chain 0 < naccept < T, at least one trajectory aborted at the box and at least
    one rejected without aborting, under every prior of the case and with and without a factor: a device test cannot pass on a chain that
    never moves, never leaves or is never refused.  ln P and its gradient here are the Gram route in NumPy."""
    hc = hmc_case(tag)
    case = hc["case"]
    N = len(case["walker"])
    assert 6 <= N <= 10 and hc["mom"].shape == (N, T11, len(case["rec"].param_names))
    for i in range(len(case["priors"])):
        fun = GradTarget(host_target(case, i))
        for name, F, eps in hc["variants"]:
            r = HM.host_hmc(fun, hc["theta0"], hc["mom"], hc["lnu"], eps, NLEAP, F, THIN, hc["lower"], hc["upper"], hc["prior_loc"], hc["prior_scale"])
            print(tag, i, name, "naccept", r["naccept"], "outside", r["outside"], "aborted", r["aborted"], "refused", r["refused"])
            assert mixed(r, T11) and r["theta"].shape[1] == T11 // THIN, (tag, i, name)


def test_long_inputs_move_on_both_sides_of_the_launch_boundary():
    """the T = 70 call of the GPU tests (auto, the first 3 chains, nleap = 4: launches of 64 trajectories) accepts and refuses on both sides
    of the boundary"""
    hc = hmc_case("auto", 70, 6)
    tg = host_target(hc["case"], 0)
    tg.fs, tg.Ws = tg.fs[:3], tg.Ws[:3]
    name, F, eps = hc["variants"][1]
    lnu = hc["lnu"][:3]
    r = HM.host_hmc(GradTarget(tg), hc["theta0"][:3], hc["mom"][:3], lnu, eps[:3], NLEAP, F[:3], 1, hc["lower"], hc["upper"], hc["prior_loc"], hc["prior_scale"])
    acc = lnu < np.nan_to_num(r["log_ratio"], nan=-np.inf)
    assert np.array_equal(acc.sum(1), r["naccept"]) and np.all(acc[:, :64].sum(1) > 0) and np.all(acc[:, 64:].sum(1) > 0) and np.all((~acc)[:, 64:].sum(1) > 0)
    assert mixed(r, 70)


# ----------------------------------------------------------------------------- the LDS footprint at the synthetic shapes
def hmc_lds_bytes(J1, nG, nnz, P, nw):
    """DrawLds of the DRAW_HMC kind in bytes: per workgroup W_c, the powers of f, col and erow and the prior table; per wave th, val, H, G,
    the two thetas, two records, two gradients, the momentum and F"""
    nnzp, ng1 = (nnz + 1) & ~1, nG + 1
    return 8 * (J1 * J1 + 56 + nnzp + 128) + nw * 8 * (34 + nnzp + ng1 * J1 + ng1 * ng1 + 2 * 32 + 2 * 26 + 2 * 32 + 32 + P * P)


def hmc_waves(J1, nG, nnz, P):
    return next((nw for nw in (4, 2, 1) if hmc_lds_bytes(J1, nG, nnz, P, nw) <= 160 * 1024), 0)


def _nnz(rec):
    return len(set(zip(rec.tracer.tolist(), rec.row.tolist(), rec.col.tolist())))


def hmc_shape(case):
    c = SY.CASES[case]
    pb = SY.case_problem(case)
    return (27 if c["nnlo"] else 24) * c["ntr"] + 1, c["nG"], _nnz(pb.rec), c["P"]


# the waves of a workgroup of the HMC call at each case, from hmc_lds_bytes on the case's own recipe: every case of the table runs, case I
# (the largest footprint there is) at one wave beside a W_c of 117 KB
HMC_WAVES = dict(A=4, E=4, F=4, G=2, J=2, I=1)


def test_lds_table():
    for case, nw in HMC_WAVES.items():
        assert hmc_waves(*hmc_shape(case)) == nw, (case, hmc_shape(case))
    assert hmc_lds_bytes(109, 24, 1024, 32, 1) == 149864 and hmc_waves(121, 24, 1024, 1) == 0  # the figures the library pins


# ----------------------------------------------------------------------------- argument errors raised before the library is touched
def test_argument_errors_before_the_library():
    like = _like()
    N, T = 4, 6
    theta0, off, f = np.zeros((N, 3)), [0, 2, 4], [0.7, 0.8]
    mom, lnu = np.zeros((N, T, 3)), np.zeros((N, T))
    call = lambda **kw: like.hmc_draws_params(**dict(dict(theta0=theta0, offsets=off, f=f, momentum=mom, lnu=lnu, eps=0.1, nleap=3), **kw))
    for bad in (np.zeros((N, T, 2)), np.zeros((N + 1, T, 3)), np.zeros((N, 3)), np.zeros((N, 0, 3))):
        with pytest.raises(ValueError, match="momentum must be"):
            call(momentum=bad)
    for bad in (np.zeros((N, T + 1)), np.zeros(N), np.zeros((N, T, 1))):
        with pytest.raises(ValueError, match="lnu must be"):
            call(lnu=bad)
    for bad in (np.zeros(N + 1), np.zeros((T, N)), np.zeros((N, T, 1))):
        with pytest.raises(ValueError, match="eps must be"):
            call(eps=bad)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="nleap must be"):
            call(nleap=bad)
    for bad in (np.eye(2), np.zeros((N + 1, 3, 3)), np.zeros(3)):
        with pytest.raises(ValueError, match="factor must be"):
            call(factor=bad)
    for bad in (0, T + 1, -1, 2.5):
        with pytest.raises(ValueError, match="thin must be"):
            call(thin=bad)
    for name in ("lower", "upper", "prior_loc", "prior_scale"):
        with pytest.raises(ValueError, match=name + " must be"):
            call(**{name: np.zeros(2)})
    with pytest.raises(ValueError, match="theta must be"):
        call(theta0=np.zeros((N, 2)))
    for kw in (dict(), dict(eps=np.full(N, 0.1)), dict(eps=np.full((N, T), 0.1), factor=np.eye(3)), dict(factor=np.tile(np.eye(3), (N, 1, 1)))):
        with pytest.raises(AssertionError, match="the library was touched"):
            call(**kw)
    import eftpipe_amd.marginal as M

    assert all(n in M.__all__ for n in ("DrawTrajectories", "hmc_momenta")) and M.DrawTrajectories._fields == M.DrawChains._fields + ("log_ratio",)
