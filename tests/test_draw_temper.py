"""Parallel tempering over the draw parameters on the host (no GPU): temper_util.host_ladder, the NumPy restatement of
eftb_draws_temper_params, against a bimodal target with known tempered distributions and on its edge cases; the helpers temper_ladder and
temper_proposals; the inputs of the GPU tests (test_gpu_draw_temper.py), checked here to move, to swap and to be refused on every rung, pair
and ladder; the rungs that fit the LDS at the synthetic likelihoods and the ladders the GPU tests run there, checked to mix in sum; and the
argument errors MarginalLikelihood.temper_draws_params raises before it touches the library."""
import numpy as np
import pytest

import chain_util as CU
import grad_util as GU
import synth_like_util as SY
import temper_util as TU
from test_draw_chains import _like, _walk, chain_case


# ----------------------------------------------------------------------------- the swap rule against the mathematics
MODE = 6.0


def _bimodal(th):
    return np.logaddexp(-0.5 * (th[:, 0] - MODE) ** 2, -0.5 * (th[:, 0] + MODE) ** 2)


def test_ladders_sample_every_tempered_distribution_of_a_bimodal_target():
    """ln P(x) = logaddexp(-(x - m)^2 / 2, -(x + m)^2 / 2) in the box [-12, 12]; 256 ladders of R = 4 (temper_ladder(4, 1/16)) x 2000 steps with a
    swap event every 5, every rung started in the left mode at x = -m, unit proposals widened by 1 / sqrt(beta), the first half discarded.
    For every rung the pooled E[x^2] and the occupancy of x > 0 agree with quadrature of exp(beta_r ln P) on the box within 5 Monte-Carlo
    errors, the error taken from the scatter of the per-ladder estimates (256 independent ladders: their standard deviation / 16).  A wrong
    sign of the swap ratio, or temperatures that travel with the states, fail this.  The same proposals for rung 0 run as a lone chain
    (R = 1) must not leave the left mode: occupancy of x > 0 below 0.05.  With m = 4 the ladders agreed (at most 1.0 error) but the lone
    chains' occupancy was 0.24 (unit proposals cross an e^-8 barrier within 2000 steps), so the modes stand at m = MODE = 6.
    Measured with this seed, in Monte-Carlo errors: E[x^2] 0.23, 2.57, 0.50, 0.09 on rungs 0 ... 3, the occupancy 0.57, 0.20, 0.12, 0.39
    (margin: a factor 1.9); the lone chains' occupancy is 0.0000."""
    from eftpipe_amd.marginal import temper_ladder, temper_proposals

    R, nlad, T, S = 4, 256, 2000, 5
    beta = temper_ladder(R, 1.0 / 16.0)
    assert np.allclose(beta, [1.0, 16.0 ** (-1.0 / 3.0), 16.0 ** (-2.0 / 3.0), 1.0 / 16.0], rtol=1e-15)
    step, lnu, swaps = temper_proposals(np.random.default_rng(21), nlad, beta, T, np.eye(1), S)
    theta0 = np.full((nlad * R, 1), -MODE)
    box = dict(lower=[-12.0], upper=[12.0])
    r = TU.host_ladder(_bimodal, theta0, beta, step, lnu, swaps, S, **box)
    assert np.all(r["nswap"] > 0) and np.all(r["nswap"] < r["tried"]) and np.all(r["tried"] == 200)
    x = r["theta"][:, T // 2 :, 0].reshape(nlad, R, -1)
    grid = np.linspace(-12.0, 12.0, 48001)
    lp = _bimodal(grid[:, None])
    for q in range(R):
        w = np.exp(beta[q] * (lp - lp.max()))
        w[0] *= 0.5
        w[-1] *= 0.5
        x2, occ = np.sum(w * grid**2) / np.sum(w), np.sum(w[grid > 0]) / np.sum(w)
        assert abs(occ - 0.5) < 1e-4
        for name, est, want in (("E[x^2]", (x[:, q] ** 2).mean(1), x2), ("occupancy of x > 0", (x[:, q] > 0).mean(1), occ)):
            err = est.std(ddof=1) / np.sqrt(nlad)
            print("rung %d (beta = %.4f) %s: %.4f against %.4f = %.2f Monte-Carlo errors" % (q, beta[q], name, est.mean(), want, abs(est.mean() - want) / err))
            assert abs(est.mean() - want) < 5.0 * err, (q, name)
    lone = TU.host_ladder(_bimodal, theta0[::R], [1.0], step[::R], lnu[::R], None, 0, **box)
    occ = (lone["theta"][:, T // 2 :, 0] > 0).mean()
    print("the lone chains' occupancy of x > 0: %.4f" % occ)
    assert occ < 0.05
    # <ln P> per temperature falls along the ladder: what thermodynamic integration integrates
    mean_lp = (r["sum_logp"] / T).reshape(nlad, R).mean(0)
    assert np.all(np.diff(mean_lp) < 0)


# ----------------------------------------------------------------------------- mechanics
def _quad(th):
    return -0.5 * np.sum(th**2, axis=1)


def _ladder(R, nlad=3, T=23, S=2, seed=1, P=2):
    rng = np.random.default_rng(seed)
    N = nlad * R
    beta = np.linspace(1.0, 0.2, R) if R > 1 else np.ones(1)
    return dict(theta0=rng.standard_normal((N, P)) * 0.5, beta=beta, step=rng.standard_normal((N, T, P)) * 0.6, lnu=np.log(rng.random((N, T))),
                swaps=np.log(rng.random((nlad, T // S if S else 0, max(R - 1, 0)))))


def _run(d, S=2, first_step=0, thin=1, logp=_quad, **kw):
    return TU.host_ladder(logp, d["theta0"], d["beta"], d["step"], d["lnu"], d["swaps"], S, first_step, thin, **kw)


def test_one_rung_and_no_swaps_are_the_chain():
    theta0, step, lnu = _walk()
    want = CU.host_chain(_quad, theta0, step, lnu, thin=5, lower=[-0.5, -np.inf], upper=[0.5, 0.6])
    swaps = np.zeros((4, 23 // 3, 0))
    for S, sw in ((0, None), (3, swaps)):  # R = 1 and S = 0; beta = (1,) with swap events that have no pair
        r = TU.host_ladder(_quad, theta0, [1.0], step, lnu, sw, S, thin=5, lower=[-0.5, -np.inf], upper=[0.5, 0.6])
        for name in ("theta", "logp", "naccept", "last"):
            assert np.array_equal(r[name], want[name]), name
        assert np.array_equal(r["outside"], want["outside"]) and np.all(r["nswap"] == 0) and r["nswap"].shape == (4, 1)
    # S = 0 at R = 3: every rung is a chain on beta_r ln P
    d = _ladder(3)
    r = _run(d, S=0)
    for q in range(3):
        ch = CU.host_chain(lambda th: d["beta"][q] * _quad(th), d["theta0"][q::3], d["step"][q::3], d["lnu"][q::3])
        assert np.array_equal(ch["theta"], r["theta"][q::3]) and np.array_equal(ch["naccept"], r["naccept"][q::3])
    assert np.all(r["nswap"] == 0) and np.array_equal(r["logp"], _quad(r["theta"].reshape(-1, 2)).reshape(9, 23))  # ln P comes back untempered


def test_thinning_last_and_continuation_with_first_step():
    d = _ladder(4, T=23, S=2)
    full = _run(d)
    thin = _run(d, thin=5)
    assert thin["theta"].shape == (12, 4, 2) and np.array_equal(thin["theta"], full["theta"][:, 4::5][:, :4]) and np.array_equal(thin["logp"], full["logp"][:, 4::5][:, :4])
    for name in ("last", "naccept", "nswap", "sum_logp"):
        assert np.array_equal(thin[name], full[name]), name
    assert np.array_equal(full["last"], full["theta"][:, -1]) and np.all(full["nswap"].sum(0) > 0)
    assert np.array_equal(full["sum_logp"], np.cumsum(full["logp"], axis=1)[:, -1])  # (a sequential sum)
    # T1 = 10 is even in units of S = 2, T1 = 7 ends between two events and T1 = 6 after an odd number of them: the parity of the next event
    # comes from first_step alone
    for T1 in (10, 7, 6):
        cut = lambda a, b: dict(d, step=d["step"][:, a:b], lnu=d["lnu"][:, a:b], swaps=d["swaps"][:, a // 2 : b // 2])
        a = _run(cut(0, T1))
        b = _run(dict(cut(T1, 23), theta0=a["last"]), first_step=T1)
        assert np.array_equal(np.concatenate([a["theta"], b["theta"]], axis=1), full["theta"]), T1
        assert np.array_equal(a["naccept"] + b["naccept"], full["naccept"]) and np.array_equal(a["nswap"] + b["nswap"], full["nswap"])
        assert np.array_equal(b["last"], full["last"])
        wrong = _run(dict(cut(T1, 23), theta0=a["last"]), first_step=0 if T1 != 6 else 8)[("theta")]
        assert T1 == 10 or not np.array_equal(np.concatenate([a["theta"], wrong], axis=1), full["theta"])
    # thin counts from the call's start whatever first_step is
    b = _run(dict(d, step=d["step"][:, 7:], lnu=d["lnu"][:, 7:], swaps=d["swaps"][:, 3:]), first_step=7, thin=5)
    assert b["theta"].shape[1] == 16 // 5


def test_a_swap_event_on_the_last_step():
    d = _ladder(2, T=6, S=3, seed=4)
    d["swaps"][:] = -np.inf  # (accepted whatever x is)
    r = _run(d, S=3)
    assert np.all(r["tried"] == 1) and np.all(r["nswap"] == 1)  # event 0 on step 2; event 1, on the last step, is odd and tries nothing at R = 2
    d5 = dict(d, step=d["step"][:, :3], lnu=d["lnu"][:, :3], swaps=d["swaps"][:, :1])
    r5 = _run(d5, S=3)  # T = 3: the event is on the last step, and `last` is the swapped state
    noswap = _run(dict(d5, swaps=None), S=0)
    assert np.array_equal(r5["last"][0::2], noswap["last"][1::2]) and np.array_equal(r5["last"][1::2], noswap["last"][0::2])
    assert np.array_equal(r5["theta"][:, -1], r5["last"]) and np.array_equal(r5["logp"][:, -1], _quad(r5["last"]))
    assert np.array_equal(r5["naccept"], noswap["naccept"])  # the counts stay with the rung


def test_parity_of_the_events():
    # R = 2: odd events try nothing
    d = _ladder(2, T=12, S=2)
    r = _run(d)
    assert np.all(r["tried"] == 3)
    poisoned = d["swaps"].copy()
    poisoned[:, 1::2] = np.nan  # (not read)
    assert np.array_equal(_run(dict(d, swaps=poisoned))["theta"], r["theta"])
    # R = 3: pair (0, 1) on even events, pair (1, 2) on odd ones, one rung idle per event
    d = _ladder(3, T=12, S=2)
    r = _run(d)
    assert np.all(r["tried"] == [3, 3])
    poisoned = d["swaps"].copy()
    poisoned[:, 0::2, 1] = np.nan
    poisoned[:, 1::2, 0] = np.nan
    assert np.array_equal(_run(dict(d, swaps=poisoned))["theta"], r["theta"])
    # first_step = 2 starts with event 1
    r = _run(d, first_step=2)
    assert np.all(r["tried"] == [3, 3]) and not np.array_equal(r["theta"], _run(d)["theta"])
    # R = 4: pairs (0, 1) and (2, 3) together, then (1, 2)
    assert np.all(_run(_ladder(4, T=12, S=2))["tried"] == [3, 3, 3])


def test_swap_uniforms_at_their_ends():
    """lnu_swap = -inf is ln of u = 0: below every finite x, so every tried pair is exchanged (as lnu = -inf accepts every finite proposal of the
    chain call).  A swap is never accepted where x <= lnu_swap = 0: with equal ln P on both rungs x = 0 and nothing moves."""
    d = _ladder(3, T=12, S=2)
    r = _run(dict(d, swaps=np.full(d["swaps"].shape, -np.inf)))
    assert np.array_equal(r["nswap"], r["tried"])
    flat = lambda th: np.zeros(th.shape[0])
    r = _run(dict(d, swaps=np.zeros(d["swaps"].shape)), logp=flat)
    assert np.all(r["nswap"] == 0) and np.all(r["tried"] > 0)
    # the sign of the ratio: with lnu_swap just below 0 the colder rung takes the better state and never gives it back
    d = _ladder(2, nlad=50, T=2, S=1, seed=9)
    d["step"][:] = 0.0
    r = _run(dict(d, swaps=np.full(d["swaps"].shape, -1e-300)), S=1)
    lp0 = _quad(d["theta0"])
    assert np.array_equal(r["logp"][0::2, -1], np.maximum(lp0[0::2], lp0[1::2])) and 0 < r["nswap"].sum() < 50


def test_a_failed_ladder_fails_whole_and_alone():
    d = _ladder(3, nlad=3, T=9, S=2)
    d["theta0"][4] = [0.9, 0.0]  # rung 1 of ladder 1

    def logp(th):
        return np.where(th[:, 0] > 0.85, np.nan, _quad(th))

    d["theta0"][[0, 1, 2, 3, 5, 6, 7, 8], 0] = np.minimum(d["theta0"][[0, 1, 2, 3, 5, 6, 7, 8], 0], 0.5)
    r = _run(d, logp=logp, thin=2)
    bad, ok = [3, 4, 5], [0, 1, 2, 6, 7, 8]
    assert np.all(r["naccept"][bad] == -1) and np.all(r["nswap"][1] == -1) and np.all(np.isnan(r["sum_logp"][bad]))
    assert all(np.all(np.isnan(r[k][bad])) for k in ("theta", "logp", "last"))
    assert all(np.all(np.isfinite(r[k][ok])) for k in ("theta", "logp", "last", "sum_logp")) and np.all(r["nswap"][[0, 2]] >= 0)
    # the other ladders are those of a call without the failed one
    keep = dict(d, theta0=d["theta0"][ok], step=d["step"][ok], lnu=d["lnu"][ok], swaps=d["swaps"][[0, 2]])
    alone = _run(keep, logp=logp, thin=2)
    assert np.array_equal(alone["theta"], r["theta"][ok]) and np.array_equal(alone["nswap"], r["nswap"][[0, 2]])


# ----------------------------------------------------------------------------- the helpers
def test_temper_ladder_and_proposals():
    from eftpipe_amd.marginal import metropolis_proposals, temper_ladder, temper_proposals

    assert np.array_equal(temper_ladder(1, 0.3), [1.0]) and np.array_equal(temper_ladder(2, 0.25), [1.0, 0.25])
    b = temper_ladder(5, 1.0 / 81.0)
    assert b[0] == 1.0 and b[-1] == 1.0 / 81.0 and np.all(np.diff(b) < 0) and np.allclose(b[1:] / b[:-1], 1.0 / 3.0, rtol=1e-14)
    for R, bmin in ((0, 0.5), (2.5, 0.5), (3, 0.0), (3, 1.0), (3, -0.1)):
        with pytest.raises(ValueError):
            temper_ladder(R, bmin)
    F = np.tril(np.random.default_rng(1).standard_normal((3, 3)))
    beta = temper_ladder(4, 0.1)
    step, lnu, swaps = temper_proposals(np.random.default_rng(5), 3, beta, 11, F, 3, first_step=4)
    assert step.shape == (12, 11, 3) and lnu.shape == (12, 11) and swaps.shape == (3, 15 // 3 - 4 // 3, 3) and step.flags["C_CONTIGUOUS"]
    assert np.all(lnu <= 0) and np.all(swaps <= 0)
    rng = np.random.default_rng(5)
    s0, l0 = metropolis_proposals(rng, 12, 11, F)
    assert np.array_equal(step, s0 * np.tile(1.0 / np.sqrt(beta), 3)[:, None, None]) and np.array_equal(lnu, l0)
    assert np.array_equal(swaps, np.log(rng.random((3, 4, 3))))
    wide, _, none = temper_proposals(np.random.default_rng(5), 3, beta, 11, F, 0, widen=[1.0, 2.0, 3.0, 4.0])
    assert np.array_equal(wide, s0 * np.tile([1.0, 2.0, 3.0, 4.0], 3)[:, None, None]) and none.shape == (3, 0, 3)
    assert temper_proposals(np.random.default_rng(5), 2, [1.0], 5, F, 2)[2].shape == (2, 2, 0)
    with pytest.raises(ValueError, match="beta = 0"):
        temper_proposals(np.random.default_rng(5), 3, [1.0, 0.5, 0.0], 11, F, 3)
    assert temper_proposals(np.random.default_rng(5), 3, [1.0, 0.5, 0.0], 11, F, 3, widen=[1.0, 1.5, 4.0])[0].shape == (9, 11, 3)
    with pytest.raises(ValueError, match="widen must be"):
        temper_proposals(np.random.default_rng(5), 3, beta, 11, F, 3, widen=[1.0, 2.0])
    for kw in (dict(nlad=-1), dict(T=0), dict(swap_every=-1), dict(first_step=-2), dict(swap_every=2.5)):
        with pytest.raises(ValueError, match="must be an integer"):
            temper_proposals(np.random.default_rng(5), **dict(dict(nlad=3, beta=beta, T=11, factor=F, swap_every=3), **kw))


def test_lds_waves_at_the_published_figures():
    """the chain call's figure at the largest shape (J + 1 = 121, nG = 24, 1024 recipe entries: 161288 bytes at one wave) leaves room for the
    exchange's 320 bytes and for no second wave; the fixtures' shapes hold all eight"""
    assert 8 * (121 * 121 + 56 + 512 + 128) + 8 * (34 + 1024 + 25 * 121 + 625 + 116) == 161288
    assert TU.lds_waves(121, 24, 1024) == 1 and TU.lds_waves(25, 7, 40) == 8 and TU.lds_waves(73, 14, 300) == 8


# ----------------------------------------------------------------------------- the inputs of the device tests
@pytest.mark.parametrize("tag", ["auto", "cross", "full", "nnlo"])
def test_device_inputs_move_swap_and_are_refused(tag):
    """the ladders the GPU tests feed to the device give every rung 0 < naccept < T, every adjacent pair of every ladder at least one accepted
    and one refused swap, and every ladder a proposal outside the box, under every prior of the case.  ln P here is the Gram route in NumPy."""
    case, lin = TU.ladder_case(tag)
    T = lin["step"].shape[1]
    nlad = len(lin["walker"]) // 4
    per_walker = np.array(lin["counts"]) // 4
    assert T <= 128 and nlad == sum(TU.LADDERS[tag]) >= 4 and 0 in per_walker and 1 in per_walker and per_walker.max() >= 3
    assert np.all(lin["theta0"] >= lin["lower"]) and np.all(lin["theta0"] <= lin["upper"]) and lin["lnu_swap"].shape == (nlad, T // TU.S_LADDER, 3)
    for i in range(len(case["priors"])):
        r = TU.host_ladder(TU.ladder_target(case, lin, i).logp, lin["theta0"], lin["beta"], lin["step"], lin["lnu"], lin["lnu_swap"], TU.S_LADDER, 0, TU.THIN,
                           lin["lower"], lin["upper"])
        print(tag, i, "naccept", r["naccept"], "nswap", r["nswap"].tolist(), "of", r["tried"][0], "outside the box", r["outside"])
        assert TU.mixed(r, T) and r["theta"].shape[1] == T // TU.THIN


@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_other_lengths_move(R):
    case = chain_case("auto")
    lin = TU.other_length(case, R)
    r = TU.host_ladder(TU.ladder_target(case, lin, 0).logp, lin["theta0"], lin["beta"], lin["step"], lin["lnu"], lin["lnu_swap"], TU.S_LADDER, 0, TU.THIN,
                       lin["lower"], lin["upper"])
    print("R", R, "naccept", r["naccept"], "nswap", r["nswap"].tolist(), "outside the box", r["outside"])
    assert TU.other_length_moves(r, R)


def test_long_ladder_swaps_on_both_sides_of_the_launch_boundary():
    case, lin = TU.long_ladder()
    assert lin["step"].shape[:2] == (8, 300) and lin["lnu_swap"].shape == (2, 75, 3) and 256 % 4 == 0
    run = lambda a, b, th0, first: TU.host_ladder(TU.ladder_target(case, lin, 0).logp, th0, lin["beta"], lin["step"][:, a:b], lin["lnu"][:, a:b],
                                                  lin["lnu_swap"][:, a // 4 : b // 4], 4, first, 1, lin["lower"], lin["upper"])
    head = run(0, 256, lin["theta0"], 0)
    tail = run(256, 300, head["last"], 256)
    for r in (head, tail):  # (the tail has 44 steps: not every rung moves there)
        print("naccept", r["naccept"], "nswap", r["nswap"].tolist(), "of", r["tried"][0])
        assert np.all(r["naccept"] > 0 if r is head else r["naccept"].reshape(2, 4).sum(1) > 0) and np.all(r["nswap"].sum(0) > 0)
    assert np.all(head["nswap"] + tail["nswap"] < head["tried"] + tail["tried"]) and np.all(head["nswap"] + tail["nswap"] > 0)


# ----------------------------------------------------------------------------- the ladders on the synthetic likelihoods
def test_rung_table():
    """TEMPER_RUNGS is lds_waves on each case's own recipe and TEMPER_RUNGS_PADDED at 1024 entries, the shapes taken as test_draw_hmc.hmc_shape
    takes them; the ladders of the GPU tests fit, and stand at the limit wherever the LDS sets one below eight"""
    from test_draw_hmc import hmc_shape
    from test_gpu_draw_synthetic import _padded_recipe

    assert set(TU.TEMPER_RUNGS) == set(TU.TEMPER_RUNGS_PADDED) == set(SY.CASES)
    for case in SY.CASES:
        J1, nG, nnz = TU.case_shape(case)
        assert (J1, nG, nnz) == hmc_shape(case)[:3]
        assert TU.lds_waves(J1, nG, nnz) == TU.TEMPER_RUNGS[case] and TU.lds_waves(J1, nG, TU.PADDED) == TU.TEMPER_RUNGS_PADDED[case], case
    for case, R in TU.SYNTH_R.items():
        assert R <= TU.TEMPER_RUNGS[case] and (R == TU.TEMPER_RUNGS[case] or TU.TEMPER_RUNGS[case] == 8), case
    # the padded recipe the device meets holds its 1024 entries; no recipe of one tracer can (25 rows x 27 columns)
    assert TU.case_shape("F", _padded_recipe(SY.case_problem("F").rec, TU.PADDED))[2] == TU.PADDED
    assert all(TU.lds_waves(28, 24, n) == 8 for n in range(107, 25 * 27 + 1))


def _synthetic_target(name, lin, jeff):
    from test_gpu_draw_synthetic import _padded_recipe

    pb = SY.case_problem(name.split("/")[0])
    rec = _padded_recipe(pb.rec, TU.PADDED) if name.endswith("/1024") else None
    return pb, TU.SyntheticTarget(pb, lin["walker"], jeff, rec=rec, Ds=lin.get("Ds"), dataset=lin.get("dataset"))


def _mixes(name, lin, S, thin):
    T = lin["step"].shape[1]
    for jeff in (False, True):
        pb, target = _synthetic_target(name, lin, jeff)
        assert np.all(lin["theta0"] >= lin["lower"]) and np.all(lin["theta0"] <= lin["upper"])
        r = TU.host_ladder(target.records, lin["theta0"], lin["beta"], lin["step"], lin["lnu"], lin["lnu_swap"], S, 0, thin, lin["lower"], lin["upper"],
                           np.full(pb.P, TU.PRIOR_LOC), np.full(pb.P, TU.PRIOR_SCALE))
        print(name, "R", lin["beta"].size, "jeffreys", jeff, {k: np.asarray(v).tolist() for k, v in TU.mixing_counts(r, T).items()})
        assert TU.mixed_in_sum(r, T) and np.all(np.isfinite(r["logp"])) and len(r["extras"]) == 2 and r["extras"][1].shape == r["theta"].shape[:2] + (pb.nG,)


@pytest.mark.parametrize("name", list(TU.SYNTH_TUNING))
def test_synthetic_inputs_mix(name):
    """the ladders the GPU tests run on the synthetic likelihoods meet the mixing condition (temper_util.mixed_in_sum) on the host target, without
    and with Jeffreys, under the Gaussian theta priors: every case at its rungs, case F under the padded recipe at four, Gf at three, and the
    T = 260 ladders of case G"""
    if name == "G/long":
        case, lin = TU.synthetic_inputs(name, TU.LONG_LADDERS, S=TU.LONG_S)
        assert lin["step"].shape[:2] == (6, 260) and lin["lnu_swap"].shape == (2, 86, 2)
        return _mixes(name, lin, TU.LONG_S, TU.LONG_THIN)
    case, lin = TU.synthetic_inputs(name)
    R = lin["beta"].size
    assert lin["step"].shape[1] <= 96 and lin["counts"] == [2 * R, 0, R]
    _mixes(name, lin, TU.SYNTH_S, TU.SYNTH_THIN)


@pytest.mark.parametrize("n0, kw", [(60, dict()), (300, dict(kind="flat", singular=SY.CASES["Gf"]["nG"] // 2 + 1))], ids=["gauss", "flat-singular"])
def test_three_wave_inputs_mix(n0, kw):
    """the three-wave GPU tests run case Gf at T = 4, S = 2 (each pair tried once per ladder) with 690 and 1372 ladders on walker 0, under the
    Gaussian prior and under the flat prior with the singular recipe.  The ladders come from one generator, so fewer of them are other
    ladders, not a subset: here 60 (Gaussian prior) and 300 (flat prior, singular recipe) on walker 0 and one on walker 2, the same recipe of
    inputs at sizes the host evaluates in seconds, already meet the condition in sum; the device tests assert it on their own ladders.  Under
    the flat prior the hottest pair keeps its states in one event of 27 (51 of 1373 at the device's size, 0 of 61), hence the 300"""
    pb = SY.case_problem("Gf", **kw)
    _, lin = TU.synthetic_inputs("Gf", [n0, 0, 1], T=4, S=2, **kw)
    assert lin["beta"].size == 3 and lin["step"].shape[:2] == (3 * n0 + 3, 4)
    r = TU.host_ladder(TU.SyntheticTarget(pb, lin["walker"]).records, lin["theta0"], lin["beta"], lin["step"], lin["lnu"], lin["lnu_swap"], 2, 0, 2, lin["lower"],
                       lin["upper"], np.full(pb.P, TU.PRIOR_LOC), np.full(pb.P, TU.PRIOR_SCALE))
    print("Gf T = 4", kw, {k: np.asarray(v).tolist() for k, v in TU.mixing_counts(r, 4).items()})
    assert TU.mixed_in_sum(r, 4) and np.all(np.isfinite(r["logp"]))


def test_groups_inputs_mix():
    """the ladders of the groups test (case C, two data sets): the whole call mixes on the host, every chain against its group's data vector"""
    from test_draw_datasets import datasets

    pb = SY.case_problem("C")
    whole, counts, plain, own = TU.groups_inputs("C")
    assert counts == [4, 8, 4, 4] and own.tolist() == list(range(4, 12)) + list(range(16, 20))
    for k in ("theta0", "step", "lnu"):
        assert np.array_equal(whole[k][own], plain[k])
    assert np.array_equal(whole["lnu_swap"][own[::4] // 4], plain["lnu_swap"])
    _mixes("C", dict(whole, Ds=datasets(pb.D, pb.invcov, 2)), TU.SYNTH_S, TU.SYNTH_THIN)


def test_synthetic_target_is_the_gram_route():
    """SyntheticTarget returns chain_util.gram_record's ln P and sample_util.gram_samples' full chi2 and best fit bit for bit: the same statements"""
    import sample_util as SU

    for case, jeff in (("C", False), ("E", True)):
        pb = SY.case_problem(case)
        lp, full, best = TU.SyntheticTarget(pb, pb.walker, jeff).records(pb.theta)
        for d in (0, 3, 11):
            ff, tw, tn = SY.of_walker(pb, pb.walker[d])
            W = GU.gram_matrix(tw, pb.index, pb.D, pb.invcov, tn)
            assert lp[d] == CU.gram_record(pb.rec, pb.theta[d], ff, W, pb.loc, pb.scale, jeff)
            b, _, _, f0 = SU.gram_samples(pb.rec, pb.theta[d], ff, W, pb.loc, pb.scale, np.zeros((1, pb.nG)))
            assert np.array_equal(best[d], b) and full[d] == f0


# ----------------------------------------------------------------------------- argument errors raised before the library is touched
def test_argument_errors_before_the_library():
    like = _like()
    N, T, R = 8, 6, 4
    theta0, off, f, beta = np.zeros((N, 3)), [0, 4, 8], [0.7, 0.8], [1.0, 0.5, 0.25, 0.125]
    step, lnu, swaps = np.zeros((N, T, 3)), np.zeros((N, T)), np.zeros((2, 3, 3))
    call = lambda **kw: like.temper_draws_params(**dict(dict(theta0=theta0, offsets=off, f=f, beta=beta, step=step, lnu=lnu, lnu_swap=swaps, swap_every=2), **kw))
    for bad in (np.zeros((N, T, 2)), np.zeros((N + 1, T, 3)), np.zeros((N, 3))):
        with pytest.raises(ValueError, match="step must be"):
            call(step=bad)
    with pytest.raises(ValueError, match="lnu must be"):
        call(lnu=np.zeros((N, T + 1)))
    with pytest.raises(ValueError, match="thin must be"):
        call(thin=0)
    with pytest.raises(ValueError, match="lower must be"):
        call(lower=np.zeros(2))
    for bad in (np.zeros((2, 2)), [], 1.0):
        with pytest.raises(ValueError, match="beta must be"):
            call(beta=bad)
    with pytest.raises(ValueError, match="8 chains, not a multiple of the R = 3 rungs"):
        call(beta=[1.0, 0.5, 0.25])
    for bad in (np.zeros((2, 3, 2)), np.zeros((2, 2, 3)), np.zeros((1, 3, 3)), np.zeros(18)):
        with pytest.raises(ValueError, match="lnu_swap must be \\[2, 3, 3\\]"):
            call(lnu_swap=bad)
    with pytest.raises(ValueError, match="lnu_swap must be \\[2, 2, 3\\]"):  # S = 4: steps 2 ... 7 hold events 0 and 1, steps 0 ... 5 event 0 alone
        call(swap_every=4, first_step=2, lnu_swap=np.zeros((2, 1, 3)))
    with pytest.raises(ValueError, match="lnu_swap must be .* holds 3 swap events"):
        call(lnu_swap=None)
    for name in ("swap_every", "first_step"):
        for bad in (-1, 1.5):
            with pytest.raises(ValueError, match=name + " must be an integer >= 0"):
                call(**{name: bad})
    for kw in (dict(), dict(swap_every=4, lnu_swap=np.zeros((2, 1, 3))), dict(lnu_swap=None, swap_every=0), dict(lnu_swap=np.zeros((2, 0, 3)), swap_every=0)):
        with pytest.raises(AssertionError, match="the library was touched"):
            call(**kw)
    import eftpipe_amd.marginal as M

    assert all(n in M.__all__ for n in ("TemperedChains", "temper_ladder", "temper_proposals"))
