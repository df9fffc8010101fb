"""The affine-invariant ensembles of the device call on the host (no GPU): ensemble_util.host_ensemble is pinned to the mathematics on a
badly conditioned Gaussian, then its mechanics, the helper stretch_proposals, the shape errors of the Python call, the wave table and the
inputs of the device tests (test_gpu_draw_ensemble.py)."""
import numpy as np
import pytest

import chain_util as CU
import ensemble_util as EU
import synth_like_util as SY

P4 = 4
SIG = np.array([1.0, 0.3, 0.05, 0.01])  # the dispersions along the principal axes: the covariance has the condition number 1e4
NENS, K8, T400 = 400, 8, 400


def _gauss():
    """a Gaussian in four dimensions, rotated off the axes -> mu, cov, precision"""
    Q = 0.5 * np.array([[1.0, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]])  # (every principal axis is a diagonal of the cube)
    assert np.allclose(Q @ Q.T, np.eye(P4))
    return np.array([0.5, -1.0, 2.0, 0.25]), (Q * SIG**2) @ Q.T, (Q / SIG**2) @ Q.T


def _moments(theta, mu, groups):
    """theta [N, Kt, P] in `groups` independent groups of chains -> the pooled means [P], variances [P] and the covariance of parameters
    0 and 1 about mu, and their Monte-Carlo errors from the scatter between the groups"""
    d = (theta - mu).reshape(groups, -1, theta.shape[-1])
    s = np.concatenate([d.mean(1), (d * d).mean(1), (d[..., 0] * d[..., 1]).mean(1)[:, None]], axis=1)
    return s.mean(0), s.std(0, ddof=1) / np.sqrt(groups)


_RUNS = {}


def _run(exponent):
    """400 ensembles of 8 members, 400 sweeps from starts three times too wide, the first half discarded -> deviations from the target in
    Monte-Carlo errors [9], the errors, the acceptance rate"""
    if exponent not in _RUNS:
        from eftpipe_amd.marginal import stretch_proposals

        mu, cov, prec = _gauss()
        rng = np.random.default_rng(5)
        th0 = mu + 3.0 * rng.standard_normal((NENS * K8, P4)) @ np.linalg.cholesky(cov).T
        z, pick, lnq = stretch_proposals(rng, NENS, K8, T400, P4)
        lnu = lnq + (P4 - 1) * np.log(z)
        logp = lambda th: -0.5 * np.einsum("ni,ij,nj->n", th - mu, prec, th - mu)
        r = EU.host_ensemble(logp, th0, K8, z, pick, lnu=lnu, exponent=exponent)
        got, err = _moments(r["theta"][:, T400 // 2 :], mu, NENS)
        if exponent == P4 - 1:
            _RUNS["kept"] = r["theta"][:, T400 // 2 :] - mu
        want = np.concatenate([np.zeros(P4), np.diag(cov), [cov[0, 1]]])
        _RUNS[exponent] = ((got - want) / err, err / np.concatenate([np.sqrt(np.diag(cov)), np.diag(cov), [abs(cov[0, 1])]]), r["naccept"].mean() / T400)
    return _RUNS[exponent]


def _ensemble_long_axis(axis):
    """the second moment along `axis` per ensemble of the run with the right exponent [NENS]"""
    _run(P4 - 1)
    return ((_RUNS["kept"] @ axis) ** 2).reshape(NENS, -1).mean(1)


def test_ensembles_sample_a_badly_conditioned_gaussian():
    """means, variances and a covariance within 5 Monte-Carlo errors of a Gaussian whose covariance has the condition number 1e4 and no axis
    along a coordinate, with no proposal matrix.  Measured: 1.7 errors at most, the errors 1 % of a dispersion and of a variance."""
    dev, rel, acc = _run(P4 - 1)
    print("deviations in Monte-Carlo errors", np.round(dev, 2), "relative errors", np.round(rel, 4), "acceptance %.2f" % acc)
    assert np.max(np.abs(dev)) < 5.0 and 0.2 < acc < 0.9


@pytest.mark.parametrize("exponent", [P4, 0])
def test_the_jacobian_exponent_is_P_minus_one(exponent):
    """the same run with z^P or z^0 in the place of z^(P - 1) misses the variances by far more than 5 errors (measured: 21 and 39; the first sizes tried separated them)"""
    dev, _, _ = _run(exponent)
    print("exponent", exponent, "deviations in Monte-Carlo errors", np.round(dev, 1))
    assert np.max(np.abs(dev[P4 : 2 * P4])) > 10.0


def test_a_lone_isotropic_chain_misses_the_long_axis():
    """the reason the call exists: one Metropolis chain per ensemble with the same number of evaluations (K T steps) and an isotropic
    proposal of the size the shortest axis allows (2.38 / sqrt(P) of its dispersion) does not reach the long axis's variance from the
    same starts (measured: 7.0 against 1, 12 Monte-Carlo errors, at an acceptance of 0.64)"""
    mu, cov, prec = _gauss()
    rng = np.random.default_rng(5)
    th0 = (mu + 3.0 * rng.standard_normal((NENS * K8, P4)) @ np.linalg.cholesky(cov).T)[::K8]
    T = K8 * T400
    step = 2.38 / np.sqrt(P4) * SIG.min() * rng.standard_normal((NENS, T, P4))
    lnu = np.log(rng.random((NENS, T)))
    logp = lambda th: -0.5 * np.einsum("ni,ij,nj->n", th - mu, prec, th - mu)
    r = CU.host_chain(logp, th0, step, lnu)
    w, V = np.linalg.eigh(cov)
    along = (r["theta"][:, T // 2 :] - mu) @ V[:, -1]  # [NENS, T / 2]: the coordinate along the long axis
    v = (along**2).mean(1)
    dev = (v.mean() - w[-1]) / (v.std(ddof=1) / np.sqrt(NENS))
    print("long-axis variance %.3f against %.3f: %.1f Monte-Carlo errors; acceptance %.2f" % (v.mean(), w[-1], dev, r["naccept"].mean() / T))
    assert abs(dev) > 5.0 and 0.1 < r["naccept"].mean() / T < 0.9
    # ... which the ensembles of _run reach from those starts with those evaluations, along that very axis
    e = _ensemble_long_axis(V[:, -1])
    edev = (e.mean() - w[-1]) / (e.std(ddof=1) / np.sqrt(NENS))
    print("the ensembles: %.3f, %.1f Monte-Carlo errors" % (e.mean(), edev))
    assert abs(edev) < 5.0


# ----------------------------------------------------------------------------- mechanics
def _toy(nens=3, K=4, T=23, P=2, seed=1, a=2.0):
    from eftpipe_amd.marginal import stretch_proposals

    rng = np.random.default_rng(seed)
    th0 = rng.standard_normal((nens * K, P))
    return (th0,) + stretch_proposals(rng, nens, K, T, P, a)


_quad = lambda th: -0.5 * np.sum(th * th, axis=1)


def test_two_members_one_per_half():
    th0, z, pick, lnq = _toy(K=2)
    assert np.all(pick == 0)
    r = EU.host_ensemble(_quad, th0, 2, z, pick, lnq)
    # by hand: member 0 against member 1, then member 1 against the new member 0
    cur = th0.copy()
    na = np.zeros(len(cur), dtype=int)
    for t in range(z.shape[1]):
        for k, j in ((0, 1), (1, 0)):
            for e in range(len(cur) // 2):
                a, b = 2 * e + k, 2 * e + j
                trial = cur[b] + z[a, t] * (cur[a] - cur[b])
                if lnq[a, t] < _quad(trial[None])[0] - _quad(cur[a][None])[0]:
                    cur[a] = trial
                    na[a] += 1
    assert np.array_equal(r["last"], cur) and np.array_equal(r["naccept"], na) and 0 < na.sum() < na.size * z.shape[1]


def test_half_one_sees_the_new_half_zero():
    th0, z, pick, lnq = _toy()
    r, s = EU.host_ensemble(_quad, th0, 4, z, pick, lnq), EU.host_ensemble(_quad, th0, 4, z, pick, lnq, stale=True)
    assert not np.array_equal(r["theta"], s["theta"])
    # the first half-sweep is the same; in the second, exactly the members of half 1 whose partner has moved propose from another point
    assert np.array_equal(r["asked"][0], s["asked"][0])
    one = EU.host_ensemble(_quad, th0, 4, z[:, :1], pick[:, :1], np.full_like(lnq[:, :1], -np.inf))
    stale = EU.host_ensemble(_quad, th0, 4, z[:, :1], pick[:, :1], np.full_like(lnq[:, :1], -np.inf), stale=True)
    n = np.arange(len(th0))
    half1, partner = n % 4 >= 2, n // 4 * 4 + pick[:, 0]
    assert np.all(one["naccept"] == 1)  # (lnq = -inf: everyone moved, so every partner has)
    differs = np.any(one["asked"][1] != stale["asked"][1], axis=1)
    assert np.array_equal(differs, half1)
    assert np.array_equal(one["asked"][1][half1], one["asked"][0][partner[half1]] + z[half1, 0, None] * (th0[half1] - one["asked"][0][partner[half1]]))


def test_thinning_last_and_continuation():
    th0, z, pick, lnq = _toy(T=23)
    one = EU.host_ensemble(_quad, th0, 4, z, pick, lnq)
    thin = EU.host_ensemble(_quad, th0, 4, z, pick, lnq, thin=5)
    assert thin["theta"].shape == (12, 4, 2) and np.array_equal(thin["theta"], one["theta"][:, 4::5]) and np.array_equal(thin["logp"], one["logp"][:, 4::5])
    assert np.array_equal(thin["last"], one["theta"][:, -1]) and np.array_equal(thin["naccept"], one["naccept"])
    for T1 in (1, 7, 22):
        a = EU.host_ensemble(_quad, th0, 4, z[:, :T1], pick[:, :T1], lnq[:, :T1])
        b = EU.host_ensemble(_quad, a["last"], 4, z[:, T1:], pick[:, T1:], lnq[:, T1:])
        assert np.array_equal(np.concatenate([a["theta"], b["theta"]], axis=1), one["theta"]) and np.array_equal(a["naccept"] + b["naccept"], one["naccept"])
        assert np.array_equal(b["last"], one["last"])


def test_box_rejects_without_an_evaluation():
    th0, z, pick, lnq = _toy(seed=3)
    lower, upper = th0.min(0) - 0.05, th0.max(0) + 0.05
    seen = []

    def logp(th):
        seen.append(th.copy())
        return _quad(th)

    r = EU.host_ensemble(logp, th0, 4, z, pick, lnq, lower=lower, upper=upper)
    assert np.all(r["outside"] > 0)
    for th in seen:
        assert np.all(th >= lower) and np.all(th <= upper)
    assert np.all(r["theta"] >= lower) and np.all(r["theta"] <= upper)
    free = EU.host_ensemble(_quad, th0, 4, z, pick, lnq)
    assert not np.array_equal(free["theta"], r["theta"]) and np.all(free["outside"] == 0)


def test_lnq_minus_infinity_and_positive():
    th0, z, pick, lnq = _toy()
    T = z.shape[1]
    r = EU.host_ensemble(_quad, th0, 4, z, pick, np.full_like(lnq, -np.inf))
    assert np.all(r["naccept"] == T)
    # a positive lnq is a legitimate value (u close to 1, z < 1): it refuses unless ln pi rises by more
    big = EU.host_ensemble(_quad, th0, 4, z, pick, np.full_like(lnq, 50.0))
    assert np.all(big["naccept"] == 0) and np.array_equal(big["last"], th0)
    small = EU.host_ensemble(_quad, th0, 4, z, pick, np.full_like(lnq, 1e-3))
    assert 0 < small["naccept"].sum() < r["naccept"].sum()
    assert np.any(lnq > 0)  # (stretch_proposals gives some: u' close to 1 and z < 1)


def test_nan_rejects_a_proposal_and_fails_a_start():
    th0, z, pick, lnq = _toy()
    wall = lambda th: np.where(th[:, 0] > 0.8, np.nan, _quad(th))  # (ln P is NaN beyond a wall)
    th0 = np.where(th0[:, :1] > 0.8, 0.5, th0)
    r = EU.host_ensemble(wall, th0, 4, z, pick, np.full_like(lnq, -np.inf))
    assert np.all(r["naccept"] >= 0) and np.any(r["naccept"] < z.shape[1]) and np.all(r["theta"][..., 0] <= 0.8) and np.all(np.isfinite(r["logp"]))
    assert np.any(r["asked"][..., 0] > 0.8)  # (the wall was met, and the chains went on)
    bad = th0.copy()
    bad[5, 0] = 0.9  # member 1 of ensemble 1
    f = EU.host_ensemble(wall, bad, 4, z, pick, np.full_like(lnq, -np.inf))
    assert np.all(f["naccept"][4:8] == -1) and np.all(np.isnan(f["theta"][4:8])) and np.all(np.isnan(f["last"][4:8])) and np.all(np.isnan(f["logp"][4:8]))
    ok = np.r_[0:4, 8:12]
    for name in ("theta", "logp", "last", "naccept"):
        assert np.array_equal(f[name][ok], r[name][ok]), name


def test_stretch_proposals():
    from eftpipe_amd.marginal import stretch_proposals

    for a in (2.0, 1.3, 5.0):
        z, pick, lnq = stretch_proposals(np.random.default_rng(4), 5, 6, 200, 3, a)
        assert z.shape == pick.shape == lnq.shape == (30, 200) and z.dtype == np.float64 and pick.dtype == np.int32 and lnq.dtype == np.float64
        assert np.all(z >= 1 / a) and np.all(z <= a) and z.min() < 1 / a + 0.05 * (a - 1 / a) and z.max() > a - 0.05 * (a - 1 / a)
        assert pick.min() == 0 and pick.max() == 2
        rng = np.random.default_rng(4)
        u = rng.random((30, 200))
        assert np.array_equal(z, ((a - 1.0) * u + 1.0) ** 2 / a)
        assert np.array_equal(pick, rng.integers(3, size=(30, 200)))
        assert np.array_equal(lnq, np.log(rng.random((30, 200))) - 2 * np.log(z))
        # g(z) ~ 1 / sqrt(z): the mean of sqrt(z) is (sqrt(a) + 1 / sqrt(a)) / 2
        assert abs(np.sqrt(z).mean() - 0.5 * (np.sqrt(a) + 1 / np.sqrt(a))) < 0.01 * a
    for a in (1.0, 0.5, -2.0, np.nan):
        with pytest.raises(ValueError, match="a must be > 1"):
            stretch_proposals(np.random.default_rng(4), 5, 6, 20, 3, a)
    with pytest.raises(ValueError, match="K must be even"):
        stretch_proposals(np.random.default_rng(4), 5, 5, 20, 3)
    with pytest.raises(ValueError, match="K must be an integer >= 2"):
        stretch_proposals(np.random.default_rng(4), 5, 0, 20, 3)
    assert stretch_proposals(np.random.default_rng(4), 0, 4, 7, 3)[0].shape == (0, 7)


def test_argument_errors_before_the_library():
    from test_draw_chains import _like

    import eftpipe_amd.marginal as M

    like = _like()
    N, T, K = 8, 6, 4
    theta0, off, f = np.zeros((N, 3)), [0, 4, 8], [0.7, 0.8]
    z, pick, lnq = np.ones((N, T)), np.zeros((N, T), dtype=np.int32), np.zeros((N, T))
    for bad in (np.ones((N, T, 3)), np.ones((N + 1, T)), np.ones(N), np.ones((N, 0))):
        with pytest.raises(ValueError, match="z must be \\[8, T\\] stretch factors"):
            like.ensemble_draws_params(theta0, off, f, K, bad, pick, lnq)
    for bad in (np.zeros((N, T + 1)), np.zeros(N), np.zeros((N, T, 1))):
        with pytest.raises(ValueError, match="lnq must be \\[8, 6\\]"):
            like.ensemble_draws_params(theta0, off, f, K, z, pick, bad)
    for bad in (np.zeros((N, T + 1), dtype=np.int32), np.zeros(N, dtype=np.int32), np.zeros((N, T)), np.zeros((N, T), dtype=bool)):
        with pytest.raises(ValueError, match="pick must be \\[8, 6\\] integers"):
            like.ensemble_draws_params(theta0, off, f, K, z, bad, lnq)
    for bad in (3, 2.5, 16):
        with pytest.raises(ValueError, match="K must be an integer|not a multiple of the K"):
            like.ensemble_draws_params(theta0, off, f, bad, z, pick, lnq)
    for bad in (0, T + 1, 2.5):
        with pytest.raises(ValueError, match="thin must be"):
            like.ensemble_draws_params(theta0, off, f, K, z, pick, lnq, thin=bad)
    for name in ("lower", "upper", "prior_loc", "prior_scale"):
        with pytest.raises(ValueError, match=name + " must be"):
            like.ensemble_draws_params(theta0, off, f, K, z, pick, lnq, **{name: np.zeros(2)})
    with pytest.raises(ValueError, match="theta must be"):
        like.ensemble_draws_params(np.zeros((N, 2)), off, f, K, z, pick, lnq)
    with pytest.raises(AssertionError, match="the library was touched"):
        like.ensemble_draws_params(theta0, off, f, K, z, pick.astype(np.int64), lnq)
    assert "stretch_proposals" in M.__all__


# ----------------------------------------------------------------------------- the waves of an ensemble's workgroup
def test_wave_table():
    """W = min(8, K / 2, the waves that fit beside W_c and 61 doubles per member) at K = 16 and K = 64, and the most members that leave
    room for one wave, for every synthetic case"""
    import os
    import re

    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eftpipe_amd", "csrc", "eftb_kernels.hpp")) as fh:
        m = re.search(r"constexpr int ENS_MAXK = (\d+), ENS_MAXW = (\d+), ENS_REC = RECIPE_MAXP, ENS_LP = ENS_REC \+ MARG_OUT, ENS_PRI = ENS_LP \+ 1, "
                      r"ENS_NA = ENS_PRI \+ 1, ENS_SLOT = ENS_NA \+ 1;", fh.read())
    assert m and (int(m.group(1)), int(m.group(2))) == (EU.ENS_MAXK, 8) and EU.ENS_SLOT == 32 + 26 + 3  # (the library's constants are the formula's)
    assert sorted(EU.ENSEMBLE_WAVES) == sorted(SY.CASES)
    for case, (w16, w64, most) in EU.ENSEMBLE_WAVES.items():
        assert (EU.case_waves(case, 16), EU.case_waves(case, EU.ENS_MAXK), EU.most_members(case)) == (w16, w64, most), case
    # the fixtures (J + 1 = 25, nG = 7) hold eight waves beside 64 members; at case G, K = 8 runs on three waves, two passes a half-sweep
    assert EU.ens_waves(25, 7, 40, 64) == 8 and EU.ens_waves(25, 7, 40, 6) == 3 and EU.case_waves("G", 8) == 3
    # the largest shape there is: four members beside one wave
    assert EU.ens_waves(121, 24, 1024, 4) == 1 and EU.ens_waves(121, 24, 1024, 6) == 0
    assert EU.case_waves("I", 24) == 1 and EU.case_waves("I", 26) == 0


# ----------------------------------------------------------------------------- the inputs of the device tests
def _replay(case, ein, T, thin=EU.THIN):
    for i in range(len(case["priors"])):
        r = EU.host_ensemble(EU.ensemble_target(case, ein, i).logp, ein["theta0"], ein["K"], ein["z"], ein["pick"], ein["lnq"], thin, ein["lower"], ein["upper"])
        print("K", ein["K"], "prior", i, "naccept", r["naccept"].min(), "...", r["naccept"].max(), "outside the box", r["outside"])
        assert EU.mixed(r, T) and r["theta"].shape[1] == T // thin


@pytest.mark.parametrize("tag", ["auto", "cross", "full", "nnlo"])
def test_device_inputs_move_and_are_refused(tag):
    """the inputs the GPU tests feed to the device give every member 0 < naccept < T and every ensemble a proposal outside the box, under
    every prior of the case: a device test cannot pass on an ensemble that never moves or never refuses.  ln P is the Gram route in NumPy."""
    case, ein = EU.ensemble_case(tag)
    assert ein["theta0"].shape == (4 * sum(EU.ENSEMBLES[tag]), len(case["rec"].param_names)) and 0 in ein["counts"] and 4 in ein["counts"] and 12 in ein["counts"]
    assert np.all(ein["theta0"] >= ein["lower"]) and np.all(ein["theta0"] <= ein["upper"])
    _replay(case, ein, EU.T_ENS)


def test_device_inputs_at_the_other_sizes():
    from test_draw_chains import chain_case

    case = chain_case("auto")
    for K in EU.SIZES:
        _replay(case, EU.size_case(K, case)[1], EU.T_ENS)


@pytest.mark.parametrize("name", ["G", "I", "Gf"])
def test_synthetic_inputs_mix(name):
    """the synthetic inputs of the device tests on the host (temper_util.SyntheticTarget: ln P by the Gram route), under the Gaussian theta
    priors they run with, without and with Jeffreys: G (K = 8) and I (K = 24) meet mixed(), every member 0 < naccept < T and every ensemble a
    proposal outside the box; Gf, at T = 4 and 61 + 1 ensembles of K = 2, meets it summed over the ensembles (mixed_in_sum)"""
    import temper_util as TU

    pb = SY.case_problem(name)
    ein = EU.synthetic_inputs(name, [61, 0, 1] if name == "Gf" else None)
    K, T = ein["K"], ein["z"].shape[1]
    assert (K, T) == {"G": (8, 20), "I": (24, 24), "Gf": (2, 4)}[name] and np.all(ein["theta0"] >= ein["lower"]) and np.all(ein["theta0"] <= ein["upper"])
    prior = EU.theta_prior(pb.P)
    for jeff in (False, True):
        r = EU.host_ensemble(TU.SyntheticTarget(pb, ein["walker"], jeff).logp, ein["theta0"], K, ein["z"], ein["pick"], ein["lnq"], 1, ein["lower"], ein["upper"],
                             prior["prior_loc"], prior["prior_scale"])
        print(name, jeff, "naccept", r["naccept"].min(), "...", r["naccept"].max(), "outside the box", r["outside"][:8])
        assert EU.mixed_in_sum(r, T) if name == "Gf" else EU.mixed(r, T)


def test_long_inputs_move_on_both_sides_of_the_launch_boundary():
    case, ein = EU.long_case()
    r = EU.host_ensemble(EU.ensemble_target(case, ein, 0).logp, ein["theta0"], 4, ein["z"], ein["pick"], ein["lnq"], 1, ein["lower"], ein["upper"])
    moved = np.any(np.diff(r["theta"], axis=1) != 0.0, axis=2)
    assert EU.mixed(r, 300) and np.all(moved[:, :255].sum(1) > 0) and np.all(moved[:, 256:].sum(1) > 0)
