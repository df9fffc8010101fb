"""Dragging chains between two cosmologies on the host (no GPU): drag_util.host_drag, the NumPy restatement of eftb_draws_drag_params,
against chain_util.host_chain at the two ends of the schedule and against an analytic target through a whole dragging sampler; the inputs
of the GPU tests (test_gpu_draw_drag.py), checked here to move, to be refused and to feel the end walker on every chain; the helpers
drag_fractions and drag_accept; and the argument errors MarginalLikelihood.drag_draws_params raises before it touches the library."""
import numpy as np
import pytest

import chain_util as CU
import drag_util as DU
from drag_util import T37

from eftpipe_amd.marginal import DragChains, drag_accept, drag_fractions  # (the feature: without it nothing in this file runs)

RHO = 0.8  # correlation of the slow and the fast parameter of the analytic target


# ----------------------------------------------------------------------------- the two ends of the schedule are the chain call
def _walk(N=6, T=29, P=2, seed=2):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, P)) * 0.1, rng.standard_normal((N, T, P)) * 0.4, np.log(rng.random((N, T)))


def test_frac_zero_and_one_are_host_chain_on_one_target():
    """frac = 0 everywhere is host_chain on the start target, frac = 1 on the end target, bit for bit wherever the other end is finite:
    u a1 + 0 b1 = a1 and 0 a1 + 1 b1 = b1 exactly.  Each target has a region without a finite ln P of its own, which rejects; under a box
    and a Gaussian prior on theta, thinned and not"""
    theta0, step, lnu = _walk()
    fa = lambda th: np.where(th[:, 0] > 0.45, np.nan, -0.5 * np.sum(th**2, axis=1) / 0.3)
    fb = lambda th: np.where(th[:, 1] < -0.4, np.nan, -0.5 * np.sum((th - [0.3, -0.1]) ** 2, axis=1) / 0.2)
    finite_a = lambda th: -0.5 * np.sum(th**2, axis=1) / 0.3
    finite_b = lambda th: -0.5 * np.sum((th - [0.3, -0.1]) ** 2, axis=1) / 0.2
    kw = dict(lower=[-0.6, -0.5], upper=[0.5, np.inf], loc=[0.1, 0.0], scale=[0.3, np.inf])
    T = step.shape[1]
    for thin in (1, 4):
        for lam, own, other, key in ((0.0, fa, finite_b, "start"), (1.0, fb, finite_a, "end")):
            want = CU.host_chain(own, theta0, step, lnu, thin, **kw)
            args = (own, other) if key == "start" else (other, own)
            got = DU.host_drag(*args, theta0, step, lnu, np.zeros_like(drag_fractions(T)) + lam, thin, **kw)
            assert np.all(want["naccept"] > 0) and np.all(want["naccept"] < T) and np.all(want["outside"] > 0)
            assert np.array_equal(got["theta"], want["theta"]) and np.array_equal(got["logp_" + key], want["logp"])
            assert np.array_equal(got["last"], want["last"]) and np.array_equal(got["naccept"], want["naccept"]) and np.array_equal(got["outside"], want["outside"])
            assert np.all(np.isfinite(got["logp_start"])) and np.all(np.isfinite(got["logp_end"]))  # (the other end was finite throughout)
    # the interpolated rule is neither
    mid = DU.host_drag(finite_a, finite_b, theta0, step, lnu, np.full_like(drag_fractions(T), 0.5), 1, **kw)
    assert all(not np.array_equal(mid["theta"], CU.host_chain(f, theta0, step, lnu, 1, **kw)["theta"]) for f in (finite_a, finite_b))
    assert np.sum(mid["differ"] > 0) >= 4


def test_sums_thinning_and_failures():
    theta0, step, lnu = _walk()
    T = step.shape[1]
    frac = drag_fractions(T)
    fa = lambda th: (-0.5 * np.sum(th**2, axis=1) / 0.3, th[:, :1] * 2.0)  # (an extra carried with the state)
    fb = lambda th: np.where(th[:, 0] > 0.6, np.nan, -0.5 * np.sum((th - [0.3, -0.1]) ** 2, axis=1) / 0.2)
    kw = dict(lower=[-0.7, -0.6], upper=[0.9, 0.8], loc=[0.1, 0.0], scale=[0.3, np.inf])
    theta0[4] = [0.8, 0.0]  # fails at the end walker only
    one = DU.host_drag(fa, fb, theta0, step, lnu, frac, 1, **kw)
    ok = np.arange(6) != 4
    assert one["naccept"][4] == -1 and all(np.all(np.isnan(one[k][4])) for k in ("theta", "logp_start", "logp_end", "last", "sum_start", "sum_end", "last_logp_start"))
    assert all(np.all(np.isfinite(one[k][ok])) for k in ("theta", "logp_start", "logp_end", "last", "sum_start", "sum_end")) and np.all(one["naccept"][ok] > 0)
    assert np.array_equal(one["extras_start"][0][ok], one["theta"][ok][:, :, :1] * 2.0) and np.array_equal(one["last_extras_start"][0][ok], one["last"][ok][:, :1] * 2.0)
    # the sums are the T + 1 terms of the states, the starting one included, added in step order
    _, _, loc, sinv = CU.prior_arrays(2, **kw)
    for key, f in (("start", lambda th: fa(th)[0]), ("end", fb)):
        s = f(theta0[ok]) + CU.prior_term(theta0[ok], loc, sinv)
        for k in range(T):
            s = s + (one["logp_" + key][ok][:, k] + CU.prior_term(one["theta"][ok][:, k], loc, sinv))
        assert np.array_equal(s, one["sum_" + key][ok])
    # thinned: a subsequence; thin = 0: no trajectory, the same end
    for thin in (5, 0):
        r = DU.host_drag(fa, fb, theta0, step, lnu, frac, thin, **kw)
        K = T // thin if thin else 0
        assert r["theta"].shape == (6, K, 2) and r["logp_end"].shape == (6, K) and r["extras_start"][0].shape == (6, K, 1)
        if thin:
            assert np.array_equal(r["theta"], one["theta"][:, thin - 1 :: thin][:, :K], equal_nan=True) and np.array_equal(r["logp_end"], one["logp_end"][:, thin - 1 :: thin][:, :K], equal_nan=True)
        for k in ("last", "naccept", "sum_start", "sum_end", "last_logp_start", "last_logp_end", "outside"):
            assert np.array_equal(r[k], one[k], equal_nan=True), k
    assert np.array_equal(one["last"][ok], one["theta"][ok][:, -1]) and np.array_equal(one["last_logp_end"][ok], one["logp_end"][ok][:, -1])


# ----------------------------------------------------------------------------- the rule against the mathematics
def _result(r, T):
    """host_drag's dict as the DragChains a device call returns, as far as drag_accept looks"""
    vals = dict(sum_start=r["sum_start"], sum_end=r["sum_end"], log_ratio=(r["sum_end"] - r["sum_start"]) / (T + 1), last=r["last"], naccept=r["naccept"])
    return DragChains(*[vals.get(k) for k in DragChains._fields])


def _rule(lnu_slow, r, T, start_term):
    return drag_accept(lnu_slow, _result(r, T))


def _drag_sampler(decide, n_iter, N=256, T=4, seed=21):
    """A dragging sampler on N(0, [[1, RHO], [RHO, 1]]) over (slow s, fast theta): per iteration a slow proposal s' = s + 1.5 z, host_drag
    with T fast steps from (s, theta) towards (s', .) on drag_fractions(T), and the whole move accepted where decide(lnu_slow, result, T,
    start term) says so; a rejected chain returns to (s, theta).  The chains start on exact draws.  -> s, theta [N, n_iter]"""
    Sigma = np.array([[1.0, RHO], [RHO, 1.0]])
    Si = np.linalg.inv(Sigma)
    lnpi = lambda s, th: -0.5 * (Si[0, 0] * s * s + 2.0 * Si[0, 1] * s * th + Si[1, 1] * th * th)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, 2)) @ np.linalg.cholesky(Sigma).T
    s, th = x[:, 0].copy(), x[:, 1].copy()
    out_s, out_t = np.empty((N, n_iter)), np.empty((N, n_iter))
    frac = drag_fractions(T)
    for it in range(n_iter):
        s1 = s + 1.5 * rng.standard_normal(N)
        step, lnu = 0.8 * rng.standard_normal((N, T, 1)), np.log(rng.random((N, T)))
        r = DU.host_drag(lambda t: lnpi(s, t[:, 0]), lambda t: lnpi(s1, t[:, 0]), th[:, None], step, lnu, frac)
        acc = decide(np.log(rng.random(N)), r, T, lnpi(s1, th) - lnpi(s, th))
        s, th = np.where(acc, s1, s), np.where(acc, r["last"][:, 0], th)
        out_s[:, it], out_t[:, it] = s, th
    return out_s, out_t


def _misses(s, th):
    """the pooled moments of the chains against the target, in Monte-Carlo errors taken from the between-chain scatter"""
    N = s.shape[0]
    est = dict(mean_s=s.mean(1), mean_t=th.mean(1), var_s=(s * s).mean(1) - 1.0, var_t=(th * th).mean(1) - 1.0, cov=(s * th).mean(1) - RHO)
    return {k: abs(v.mean()) / (v.std(ddof=1) / np.sqrt(N)) for k, v in est.items()}


N_ITER = 300
# two deliberately wrong decisions on the whole move: the sums without their start term, and division by T instead of T + 1.  Not run by the
# suite; the figures in the docstring below are measured again with: python -c "import test_draw_drag as t; t.measure()"
WRONG = dict(no_start_term=lambda lnu, r, T, st: lnu < ((r["sum_end"] - r["sum_start"]) - st) / (T + 1),
             divide_by_T=lambda lnu, r, T, st: lnu < (r["sum_end"] - r["sum_start"]) / T)


def measure():
    for name, decide in dict(rule=_rule, **WRONG).items():
        print(name, {k: round(v, 2) for k, v in _misses(*_drag_sampler(decide, N_ITER)).items()})


def test_dragging_sampler_samples_an_analytic_gaussian():
    """256 chains x 300 dragging iterations of T = 4 fast steps on a two-dimensional Gaussian over (slow, fast) with correlation 0.8, the
    whole move decided by drag_accept on log_ratio = (sum_end - sum_start) / (T + 1).  Mean, variances and covariance agree with the
    target within 5 Monte-Carlo errors, the error taken from the scatter of the per-chain estimates (the criterion of test_draw_chains.py).
    Measured with this seed (0.4 s): the means off by 0.59 and 0.47 errors, the variances by 1.15 and 1.70, the covariance by 1.54 (margin: a
    factor 2.9).  At this run length the two wrong decisions of WRONG miss: the sums without their start term by 15.8 and 11.1 errors in
    the variances and 12.9 in the covariance; division by T instead of T + 1 by 9.1 errors in the variance of the slow parameter (3.3 and 5.0
    in the other two)."""
    s, th = _drag_sampler(_rule, N_ITER)
    for k, v in _misses(s, th).items():
        print("%s: off by %.2f Monte-Carlo errors" % (k, v))
        assert v < 5.0, k


# ----------------------------------------------------------------------------- the inputs of the device tests
@pytest.mark.parametrize("tag", ["auto", "full", "nnlo"])
def test_device_inputs_move_are_refused_and_feel_the_end_walker(tag):
    """the inputs the GPU tests feed to the device, under every prior of the case and with both ends' ln P by the Gram route in NumPy: every
    chain has 0 < naccept < T and a proposal outside the box, and every pair of two different walkers meets a step that the start target
    alone would have decided otherwise -- a device test cannot pass on chains that never move or on a kernel that ignores the end
    walker.  One pair has one walker twice, one has no chain, and the end walkers have their own growth rates."""
    case = DU.drag_case(tag)
    inp, N = case["inp"], len(case["pair"])
    C = len(case["counts"])
    assert inp["step"].shape[:2] == (N, T37) and np.any(case["pcounts"] == 0) and np.any(case["wstart"] == case["wend"]) and len(case["Ws"]) == 2 * C
    two = case["a"] != case["b"]
    assert np.any(two) and np.all(np.any(case["fw"][case["a"][two]] != case["fw"][case["b"][two]], axis=1))
    for i in range(len(case["priors"])):
        ta, tb = DU.host_targets(case, i)
        r = DU.host_drag(ta.logp, tb.logp, inp["theta0"], inp["step"], inp["lnu"], drag_fractions(T37), 5, inp["lower"], inp["upper"])
        print(tag, i, "naccept", r["naccept"], "outside the box", r["outside"], "decided otherwise", r["differ"])
        assert DU.moves(r, case, T37) and r["theta"].shape[1] == T37 // 5


# ----------------------------------------------------------------------------- the helpers, and argument errors before the library
def test_drag_fractions_and_drag_accept():
    assert np.array_equal(drag_fractions(4), np.array([1.0, 2.0, 3.0, 4.0]) / 5.0) and drag_fractions(1).tolist() == [0.5]
    fr = drag_fractions(T37)
    assert fr.shape == (T37,) and np.array_equal(fr, np.arange(1, T37 + 1) / (T37 + 1)) and fr[0] > 0.0 and fr[-1] < 1.0
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError, match="T must be"):
            drag_fractions(bad)
    res = DragChains(*([None] * 9), np.array([-0.5, 0.2, -np.inf, np.nan]), *([None] * 8))
    assert drag_accept(np.array([-0.6, -0.1, -1e300, -1.0]), res).tolist() == [True, True, False, False]
    assert drag_accept(np.array([-0.5, 0.0, -np.inf, -np.inf]), res).tolist() == [False, True, False, False]
    with pytest.raises(ValueError, match="lnu_slow must be"):
        drag_accept(np.zeros(3), res)
    assert DragChains._fields[:10] == ("theta", "logp_start", "logp_end", "last", "naccept", "last_logp_start", "last_logp_end", "sum_start", "sum_end", "log_ratio")


def test_argument_errors_before_the_library():
    from test_draw_chains import _like

    import eftpipe_amd.marginal as M

    like = _like()
    N, T = 4, 6
    theta0, off, f, pairs = np.zeros((N, 3)), [0, 2, 4], [0.7, 0.8], ([0, 1], [1, 1])
    step, lnu = np.zeros((N, T, 3)), np.zeros((N, T))
    for bad in (np.zeros((N, T, 2)), np.zeros((N + 1, T, 3)), np.zeros((N, 3)), np.zeros((N, 0, 3))):
        with pytest.raises(ValueError, match="step must be"):
            like.drag_draws_params(theta0, off, f, pairs, bad, lnu)
    for bad in (np.zeros((N, T + 1)), np.zeros(N)):
        with pytest.raises(ValueError, match="lnu must be"):
            like.drag_draws_params(theta0, off, f, pairs, step, bad)
    for bad in (np.zeros(T + 1), np.zeros((T, 1)), 0.5):
        with pytest.raises(ValueError, match="frac must be"):
            like.drag_draws_params(theta0, off, f, pairs, step, lnu, frac=bad)
    for bad in (T + 1, -1, 2.5):
        with pytest.raises(ValueError, match="thin must be"):
            like.drag_draws_params(theta0, off, f, pairs, step, lnu, thin=bad)
    for name in ("lower", "upper", "prior_loc", "prior_scale"):
        with pytest.raises(ValueError, match=name + " must be"):
            like.drag_draws_params(theta0, off, f, pairs, step, lnu, **{name: np.zeros(2)})
    for bad in (([0, 1], [1]), [0, 1], ([0.5, 1.0], [1.0, 1.0]), ([], []), 3):
        with pytest.raises(ValueError, match="pairs must be"):
            like.drag_draws_params(theta0, off, f, bad, step, lnu)
    with pytest.raises(ValueError, match="offsets must be \\[3\\]: pair g"):
        like.drag_draws_params(theta0, [0, 1, 2, 4], f, pairs, step, lnu)
    with pytest.raises(ValueError, match="theta must be"):
        like.drag_draws_params(np.zeros((N, 2)), off, f, pairs, step, lnu)
    for thin in (0, 1, T):  # thin = 0 is a sampler's normal use: it reaches the library
        with pytest.raises(AssertionError, match="the library was touched"):
            like.drag_draws_params(theta0, off, f, pairs, step, lnu, thin=thin)
    assert all(n in M.__all__ for n in ("DragChains", "drag_fractions", "drag_accept"))
