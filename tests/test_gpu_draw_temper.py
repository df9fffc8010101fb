"""Parallel tempering over the draw parameters on the device (eftb_draws_temper_params; MarginalLikelihood.temper_draws_params).
Yardstick: the project's own synchronous route -- temper_util.host_ladder (pinned to the mathematics by test_draw_temper.py) around the records
of eftb_draws_logp_params, as test_gpu_draw_chains._records asks for them.  Everything is compared bit for bit: the states, ln P, full chi2,
the best fits, the last state, the accept counts, the swap counts and the sums of ln P.  The inputs are those test_draw_temper.py has checked
to move, to swap and to be refused on every rung and pair; the replayed ladders are asked again.  The fixtures reach nG = 14, P = 6, three
tracers and eight rungs; the tests of the last section run the ladders on synth_like_util's likelihoods, up to nG = 24, P = 8, five tracers
and the rung counts the LDS limits (temper_util.TEMPER_RUNGS)."""
import ctypes as C

import numpy as np
import pytest

import synth_like_util as SY
import temper_util as TU
from test_draw_datasets import datasets
from test_gpu_draw_chains import _engine, _like, _records, _stored_records_are_the_draw_call
from test_gpu_draws import _marg, _offsets
from test_gpu_draws_params import _marg_case

pytestmark = pytest.mark.gpu

FIELDS = ("theta", "logp", "fullchi2", "best", "last", "naccept", "nswap", "sum_logp")


def _same(got, want):
    """a TemperedChains of the device against host_ladder's dict around the device's records"""
    for name, b in zip(FIELDS, (want["theta"], want["logp"], want["extras"][0], want["extras"][1], want["last"], want["naccept"], want["nswap"], want["sum_logp"])):
        a = getattr(got, name)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), name


def _compare(like, off, f, lin, thin, S=TU.S_LADDER, first_step=0, groups=None, raw=False, **prior):
    """the device call against the host loop -> (TemperedChains, host_ladder's dict)"""
    box = {k: lin[k] for k in ("lower", "upper") if k in lin}
    want = TU.host_ladder(_records(like, off, f, groups), lin["theta0"], lin["beta"], lin["step"], lin["lnu"], lin.get("lnu_swap"), S, first_step, thin,
                          box.get("lower"), box.get("upper"), prior.get("prior_loc"), prior.get("prior_scale"))
    call = like._temper_raw if raw else like.temper_draws_params
    got = call(lin["theta0"], off, f, lin["beta"], lin["step"], lin["lnu"], lin.get("lnu_swap"), swap_every=S, first_step=first_step, thin=thin, groups=groups,
               return_best=True, **box, **prior)
    _same(got, want)
    return got, want


def _pick(lin, sel):
    """the chains sel (whole ladders) of ladder inputs"""
    R = lin["beta"].size
    return dict(lin, theta0=lin["theta0"][sel], step=lin["step"][sel], lnu=lin["lnu"][sel], lnu_swap=lin["lnu_swap"][sel[::R] // R])


@pytest.mark.parametrize("tag", ["auto", "cross", "full", "nnlo"])
def test_ladders_are_the_host_loop_bit_for_bit(golden, tag):
    """R = 4, thin = 5, S = 3, walkers with 0, 1 and 3 ladders, under every prior of the case"""
    case, lin = TU.ladder_case(tag)
    eng = _engine(golden, tag, case)
    off, f, T = _offsets(lin["counts"]), case["f"], lin["step"].shape[1]
    N, P, nG = lin["theta0"].shape[0], lin["theta0"].shape[1], case["rec"].ng1 - 1
    for i in range(len(case["priors"])):
        like = _like(eng, case, i)
        before = like.logp_draws_params(lin["theta0"], off, f, return_best=True)
        chains = like.metropolis_draws_params(lin["theta0"], off, f, lin["step"], lin["lnu"], thin=TU.THIN, lower=lin["lower"], upper=lin["upper"], return_best=True)
        got, want = _compare(like, off, f, lin, TU.THIN)
        K = T // TU.THIN
        assert got.theta.shape == (N, K, P) and got.best.shape == (N, K, nG) and got.nswap.shape == (N // 4, 3) and got.sum_logp.shape == (N,)
        print(tag, i, "naccept", got.naccept, "nswap", got.nswap.tolist(), "tried", want["tried"][0], "outside the box", want["outside"])
        assert TU.mixed(want, T) and np.all(np.isfinite(got.theta)) and np.all(np.isfinite(got.logp)) and np.all(np.isfinite(got.sum_logp))
        _stored_records_are_the_draw_call(like, off, f, got)
        # the draw call and the chain call are not disturbed: the Gram cache, the records, the chain buffers
        for a, b in zip(before, like.logp_draws_params(lin["theta0"], off, f, return_best=True)):
            assert np.array_equal(a, b)
        again = like.metropolis_draws_params(lin["theta0"], off, f, lin["step"], lin["lnu"], thin=TU.THIN, lower=lin["lower"], upper=lin["upper"], return_best=True)
        for a, b in zip(chains, again):
            assert np.array_equal(a, b)
        if i:
            continue
        lean = like.temper_draws_params(lin["theta0"], off, f, lin["beta"], lin["step"], lin["lnu"], lin["lnu_swap"], swap_every=TU.S_LADDER, thin=TU.THIN,
                                        lower=lin["lower"], upper=lin["upper"])
        assert lean.fullchi2 is None and lean.best is None and np.array_equal(lean.theta, got.theta) and np.array_equal(lean.nswap, got.nswap)
    eng.close()


@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_other_ladder_lengths(golden, R):
    """R = 1, 2, 3 and 8 on marg.npz auto; R = 1, and beta = (1,) with swap events, are the chain call bit for bit"""
    from test_draw_chains import chain_case

    case = chain_case("auto")
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    lin = TU.other_length(case, R)
    off, f = _offsets(lin["counts"]), case["f"]
    got, want = _compare(like, off, f, lin, TU.THIN)
    print("R", R, "naccept", got.naccept, "nswap", got.nswap.tolist())
    assert got.nswap.shape == (len(lin["walker"]) // R, max(R - 1, 1)) and TU.other_length_moves(want, R)
    if R == 1:
        for S, swaps in ((0, None), (3, lin["lnu_swap"])):
            one = like.temper_draws_params(lin["theta0"], off, f, [1.0], lin["step"], lin["lnu"], swaps, swap_every=S, thin=TU.THIN, lower=lin["lower"],
                                           upper=lin["upper"])
            ch = like.metropolis_draws_params(lin["theta0"], off, f, lin["step"], lin["lnu"], thin=TU.THIN, lower=lin["lower"], upper=lin["upper"])
            for name in ("theta", "logp", "last", "naccept"):
                assert np.array_equal(getattr(one, name), getattr(ch, name)), name
    eng.close()


def test_every_workgroup_takes_a_second_ladder(golden):
    """the launcher spreads a walker's ladders over up to 2048 / C workgroups (draw_shares), so three ladders on a walker go to three
    workgroups; 520 ladders of R = 2 on one of four walkers make the first eight workgroups loop.  T = 6, S = 2"""
    from eftpipe_amd.marginal import temper_ladder
    from test_draw_chains import chain_case

    case = chain_case("auto")
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    lin = TU.ladder_inputs(case, [2048 // 4 + 8, 0, 0, 1], 2, 6, temper_ladder(2, 0.3), 41, S=2)
    got, want = _compare(like, _offsets(lin["counts"]), case["f"], lin, 2, S=2)
    assert got.nswap.shape == (521, 1) and 0 < want["nswap"].sum() < want["tried"].sum() and np.any(got.naccept > 0)
    eng.close()


def test_long_ladder_crosses_the_launch_boundary(golden):
    """T = 300 > 256 with S = 4: two launches and a swap event on the last step of the first.  The call equals the host loop, a 100 + 200
    split from `last` with first_step = 100, and a 99 + 201 split, whose first part is odd in units of S"""
    case, lin = TU.long_ladder()
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    off, f, S = _offsets(lin["counts"]), case["f"], 4
    got, _ = _compare(like, off, f, lin, 7, S=S)
    one, want = _compare(like, off, f, lin, 1, S=S)
    assert np.all(one.naccept > 0) and np.all(one.nswap > 0) and np.all(one.nswap < want["tried"])
    assert np.array_equal(got.theta, one.theta[:, 6::7]) and np.array_equal(got.last, one.last) and np.array_equal(got.nswap, one.nswap)
    assert np.array_equal(got.sum_logp, one.sum_logp)
    for T1 in (100, 99):
        cut = lambda a, b: dict(lin, step=np.ascontiguousarray(lin["step"][:, a:b]), lnu=np.ascontiguousarray(lin["lnu"][:, a:b]),
                                lnu_swap=np.ascontiguousarray(lin["lnu_swap"][:, a // S : b // S]))
        first, _ = _compare(like, off, f, cut(0, T1), 1, S=S)
        second, _ = _compare(like, off, f, dict(cut(T1, 300), theta0=first.last), 1, S=S, first_step=T1)
        for name in ("theta", "logp", "fullchi2", "best"):
            assert np.array_equal(np.concatenate([getattr(first, name), getattr(second, name)], axis=1), getattr(one, name)), (T1, name)
        assert np.array_equal(second.last, one.last) and np.array_equal(first.naccept + second.naccept, one.naccept)
        assert np.array_equal(first.nswap + second.nswap, one.nswap)
    eng.close()


def test_a_launch_that_stores_nothing_before_one_that_does(golden):
    """T = 300, thin = 299, S = 4, R = 4: the launch of steps 1 ... 256 stores no state and brings nothing back, the second stores the one
    state there is.  The state, its record, `last`, the accept and swap counts and the sums of ln P are the host loop's."""
    case, lin = TU.long_ladder()
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    got, _ = _compare(like, _offsets(lin["counts"]), case["f"], lin, 299, S=4)
    assert lin["beta"].size == 4 and got.theta.shape[:2] == (lin["theta0"].shape[0], 1) and np.all(got.naccept > 0) and np.all(got.nswap > 0)
    eng.close()


def test_order_and_split_of_the_ladders(golden):
    """the same ladders in another order, and split over two calls with other offsets, give the same bits per ladder"""
    case, lin = TU.ladder_case("auto")
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    f, counts, R = case["f"], np.array(lin["counts"]), 4
    off = _offsets(counts)
    whole, _ = _compare(like, off, f, lin, TU.THIN)
    per_ladder = lambda a, name: a.reshape((-1, R) + a.shape[1:]) if name != "nswap" else a

    def check(part, sel, note):
        for name in FIELDS:
            assert np.array_equal(per_ladder(getattr(part, name), name), per_ladder(getattr(whole, name), name)[sel[::R] // R]), (note, name)

    # walker 0's three ladders in the order 2, 0, 1
    order = np.concatenate([np.arange(8, 12), np.arange(0, 8), np.arange(12, counts.sum())])
    part, _ = _compare(like, off, f, _pick(lin, order), TU.THIN)
    check(part, order, "order")
    cutc = np.array([R, 0, R, 0])
    sel_a = np.concatenate([np.arange(off[c], off[c] + cutc[c]) for c in range(4)])
    sel_b = np.concatenate([np.arange(off[c] + cutc[c], off[c + 1]) for c in range(4)])
    for sel, cnt in ((sel_a, cutc), (sel_b, counts - cutc)):
        part, _ = _compare(like, _offsets(cnt), f, _pick(lin, sel), TU.THIN)
        check(part, sel, "split")
    none = like.temper_draws_params(np.zeros((0, 3)), [0, 0, 0, 0, 0], f, lin["beta"], np.zeros((0, 4, 3)), np.zeros((0, 4)), np.zeros((0, 1, 3)), swap_every=3,
                                    thin=2, return_best=True)
    assert none.theta.shape == (0, 2, 3) and none.nswap.shape == (0, 3) and none.sum_logp.shape == (0,)
    # a Gaussian prior on theta is not tempered: the ladders change as the host loop says
    mid, wid = 0.5 * (lin["lower"] + lin["upper"]), 0.1 * (lin["upper"] - lin["lower"])
    c, _ = _compare(like, off, f, lin, TU.THIN, prior_loc=mid, prior_scale=wid)
    assert not np.array_equal(c.theta, whole.theta)
    eng.close()


def test_groups_ladders_against_their_own_data(golden):
    """groups= after set_datasets (M = 3) against the host loop through logp_draws_params(groups=); the groups of data set 0 are the call
    without groups bit for bit"""
    case, lin = TU.ladder_case("auto")
    eng = _engine(golden, "auto", case)
    f, R = case["f"], 4
    groups = [(3, 2), (0, 0), (2, 0), (0, 1), (2, 1)]
    counts = [4, 8, 4, 0, 4]  # 20 chains: the case's five ladders
    assert sum(counts) == lin["theta0"].shape[0]
    wk, ds = np.array([w for w, _ in groups]), np.array([m for _, m in groups])
    off = _offsets(counts)
    Ds = datasets(case["D"], case["Ci"], 3)
    assert np.array_equal(Ds[0], case["D"])
    for i in (0, 1):
        like = _like(eng, case, i)
        like.set_datasets(Ds)
        got, want = _compare(like, off, f, lin, TU.THIN, groups=(wk, ds))
        print("groups", i, "naccept", got.naccept, "nswap", got.nswap.tolist())
        assert np.all(got.naccept >= 0) and np.all(np.isfinite(got.logp))
        _stored_records_are_the_draw_call(like, off, f, got, groups=(wk, ds))
        own = sorted((q for q, (w, m) in enumerate(groups) if m == 0), key=lambda q: groups[q][0])
        sel = np.concatenate([np.arange(off[q], off[q + 1]) for q in own])
        cnt = np.zeros(4, dtype=int)
        for q in own:
            cnt[groups[q][0]] = counts[q]
        plain, _ = _compare(like, _offsets(cnt), f, _pick(lin, sel), TU.THIN)
        for name in FIELDS:
            a, b = getattr(plain, name), getattr(got, name)
            assert np.array_equal(a, b[sel] if name != "nswap" else b[sel[::R] // R]), name
    eng.close()


def test_failed_ladder_and_refusals(golden):
    from eftpipe_amd import _lib as L
    from eftpipe_amd.marginal import MarginalLikelihood, temper_ladder
    from eftpipe_amd.parambasis import DrawRecipe

    g, eng, T, index = _marg(golden, "auto", max_batch=4)
    rec, theta, _, _, f = _marg_case(g, "auto", [4, 4])
    D, Ci = g["auto_D"], g["auto_invcov"]
    nG = len(g["auto_loc"])
    eng.put("TEMPL", np.stack([T, T]))
    off = [0, 4, 8]
    N, P, Tn, R, S = 8, 3, 9, 2, 2
    beta = temper_ladder(R, 0.5)
    rng = np.random.default_rng(6)
    step, lnu = rng.standard_normal((N, Tn, P)) * [0.02, 0.1, 0.1], np.log(rng.random((N, Tn)))
    swaps = np.log(rng.random((N // R, Tn // S, R - 1)))
    # ---- det F2 <= 0 where theta_2 = 0 (test_gpu_draw_chains.py): rung 1 of ladder 1 starts on the singular plane
    flat = MarginalLikelihood(eng, index, D, Ci, np.zeros(nG), np.full(nG, np.inf))
    idx3 = rec.idx.copy()
    idx3[rec.row == 3, 2] = 2
    flat.set_draw_recipe(DrawRecipe(rec.param_names, 1, nG + 1, rec.tracer, rec.row, rec.col, rec.coef, rec.fpow, idx3))
    th0 = theta.copy()
    th0[3, 2] = 0.0
    lin = dict(theta0=th0, step=step, lnu=lnu, lnu_swap=swaps, beta=beta)
    with pytest.raises(RuntimeError, match="det of F2ij"):
        flat.temper_draws_params(th0, off, f, beta, step, lnu, swaps, swap_every=S)
    raw, want = _compare(flat, off, f, lin, 2, S=S, raw=True)
    bad, ok = [2, 3], [0, 1, 4, 5, 6, 7]
    assert np.all(raw.naccept[bad] == -1) and np.all(raw.nswap[1] == -1) and np.all(np.isnan(raw.sum_logp[bad]))
    assert all(np.all(np.isnan(a[bad])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last))
    assert all(np.all(np.isfinite(a[ok])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last, raw.sum_logp)) and np.all(raw.naccept[ok] > 0)
    assert np.all(raw.nswap[[0, 2, 3]] >= 0)
    # ---- refusals
    like = MarginalLikelihood(eng, index, D, Ci, g["auto_loc"], g["auto_scale"])
    with pytest.raises(L.EftbError, match="eftb_draws_temper_params: no draw recipe"):
        like.temper_draws_params(theta, off, f, beta, step, lnu, swaps, swap_every=S)
    like.set_draw_recipe(rec)
    want = like.temper_draws_params(theta, off, f, beta, step, lnu, swaps, swap_every=S)
    call = lambda **kw: like.temper_draws_params(**dict(dict(theta0=theta, offsets=off, f=f, beta=beta, step=step, lnu=lnu, lnu_swap=swaps, swap_every=S), **kw))
    # (what the chain call refuses, through the same checks)
    b = step.copy()
    b[2, 5, 1] = np.nan
    with pytest.raises(L.EftbError, match="eftb_draws_temper_params: step\\[2\\]\\[5\\]\\[1\\] is not finite"):
        call(step=b)
    b = lnu.copy()
    b[3, 4] = 1e-3
    with pytest.raises(L.EftbError, match="lnu\\[3\\]\\[4\\]"):
        call(lnu=b)
    with pytest.raises(L.EftbError, match="prior_scale\\[0\\]"):
        call(prior_scale=[0.0, 1.0, 1.0])
    j = int(np.argmin(theta[:, 1]))
    with pytest.raises(L.EftbError, match="theta0\\[%d\\]\\[1\\] = .* outside" % j):
        call(lower=[-np.inf, np.nextafter(theta[j, 1], np.inf), -np.inf])
    with pytest.raises(L.EftbError, match="eftb_draws_temper_params_datasets: no data sets"):
        call(groups=([0, 1], [0, 0]))
    # (its own)
    nine = temper_ladder(9, 0.1)
    with pytest.raises(L.EftbError, match="R = 9 rungs outside \\[1, 8\\]"):
        like.temper_draws_params(np.zeros((9, P)), [0, 9, 9], f, nine, np.zeros((9, Tn, P)), np.zeros((9, Tn)), np.zeros((1, Tn // S, 8)), swap_every=S)
    with pytest.raises(L.EftbError, match="walker 0 owns 3 chains, not a multiple of R = 2"):
        call(offsets=[0, 3, 8])
    for bb, msg in (([1.0, np.nan], "beta\\[1\\] = nan outside"), ([1.5, 0.5], "beta\\[0\\] = 1.5 outside"), ([0.5, -0.1], "beta\\[1\\] = -0.1 outside"),
                    ([0.5, 0.5], "beta\\[1\\] = 0.5 is not below beta\\[0\\]"), ([0.25, 0.5], "beta\\[1\\] = 0.5 is not below beta\\[0\\]")):
        with pytest.raises(L.EftbError, match=msg):
            call(beta=bb)
    for v in (np.nan, 1e-3):
        b = swaps.copy()
        b[2, 1, 0] = v  # (event 1 is odd and tries no pair of R = 2: not read)
        assert np.array_equal(call(lnu_swap=b).theta, want.theta)
        b[2, 2, 0] = v
        with pytest.raises(L.EftbError, match="lnu_swap\\[2\\]\\[2\\]\\[0\\]"):
            call(lnu_swap=b)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    th, fo, o64 = np.ascontiguousarray(theta), np.ascontiguousarray(f), np.asarray(off, dtype=np.int64)
    out = [np.zeros((N, Tn, P)), np.zeros((N, Tn)), np.zeros((N, Tn)), np.zeros((N, Tn, nG)), np.zeros((N, P))]
    nacc, nswap, sums = np.zeros(N, dtype=np.int64), np.zeros((N // R, 1), dtype=np.int64), np.zeros(N)

    def direct(Sc, first, sw):
        rc = eng.lib.eftb_draws_temper_params(eng._h, 2, N, R, Tn, Sc, first, 1, i64(o64), dp(th), dp(fo), dp(beta), dp(step), dp(lnu), dp(sw), None, None, None,
                                              None, *[dp(a) for a in out], i64(nacc), i64(nswap), dp(sums))
        return rc, eng.lib.eftb_last_error().decode()

    for Sc, first, sw, msg in ((-1, 0, swaps, "S = -1"), (S, -1, swaps, "first_step = -1"), (S, 0, None, "lnu_swap is NULL with 4 swap events")):
        rc, err = direct(Sc, first, sw)
        assert rc != 0 and msg in err, err
    assert direct(0, 0, None)[0] == 0 and np.all(nswap == 0)
    assert direct(S, 0, swaps)[0] == 0 and np.array_equal(out[4], want.last) and np.array_equal(nswap, want.nswap) and np.array_equal(sums, want.sum_logp)
    assert np.array_equal(call().theta, want.theta)
    eng.close()


def test_ladder_that_does_not_fit_the_lds():
    """synth_like_util's case G (J + 1 = 97, nG = 24: the TWO instantiation): three waves fit beside W_c.  R = 4 is refused by a message that
    names R, the waves that fit, J + 1, nG and P; R = 3 runs and is the host loop"""
    import synth_like_util as SY
    from test_gpu_draw_synthetic import _engine as synth_engine
    from test_gpu_draw_synthetic import _like as synth_like
    from test_gpu_draw_synthetic import _put

    from eftpipe_amd import _lib as L
    from eftpipe_amd.marginal import temper_ladder, temper_proposals

    pb = SY.case_problem("G")
    J1, fit = 24 * pb.ntr + 1, TU.lds_waves(24 * pb.ntr + 1, pb.nG, len(pb.rec.coef))
    assert fit == 3
    eng = synth_engine(pb, len(pb.counts) * pb.ntr)
    _put(eng, pb)
    like = synth_like(eng, pb, False)
    for R in (fit, fit + 1):
        beta = temper_ladder(R, 0.25)
        step, lnu, swaps = temper_proposals(np.random.default_rng(31), 2, beta, 6, 0.02 * np.eye(pb.P), 2)
        theta0 = np.concatenate([pb.theta[:R], pb.theta[9 : 9 + R]])  # walkers 0 and 2
        lin, off = dict(theta0=theta0, step=step, lnu=lnu, lnu_swap=swaps, beta=beta), _offsets([R, 0, R])
        if R == fit:
            got, _ = _compare(like, off, pb.f, lin, 2, S=2, prior_loc=np.ones(pb.P), prior_scale=np.full(pb.P, 0.5))
            assert np.all(got.naccept >= 0) and np.all(np.isfinite(got.sum_logp))
        else:
            with pytest.raises(L.EftbError, match="R = %d rungs needs %d waves in one workgroup, but %d fit the LDS .* J \\+ 1 = %d columns with nG = %d and P = %d" %
                               (R, R, fit, J1, pb.nG, pb.P)):
                like.temper_draws_params(theta0, off, pb.f, beta, step, lnu, swaps, swap_every=2)
    eng.close()


# ----------------------------------------------------------------------------- the synthetic likelihoods (synth_like_util.CASES)
def _synthetic(name, kind="gauss", singular=None):
    """the engine of a synthetic case with its templates put: name as the entries of temper_util.SYNTH_TUNING ("F/1024": case F under the
    recipe padded to 1024 entries) -> pb, rec (None: the case's own), eng, like(jeffreys).  A likelihood sets the engine's Jeffreys switch,
    recipe and data sets when it is built, so like(...) is called where the likelihood is used, one at a time."""
    from test_gpu_draw_synthetic import _engine as s_engine, _like as s_like, _padded_recipe, _put

    pb = SY.case_problem(name.split("/")[0], kind, singular)
    rec = _padded_recipe(pb.rec, TU.PADDED) if name.endswith("/1024") else None
    eng = s_engine(pb, len(pb.counts) * pb.ntr)
    _put(eng, pb)
    return pb, rec, eng, lambda jeffreys=False: s_like(eng, pb, jeffreys, rec=rec)


def _fields_equal(a, b, note):
    for name in FIELDS:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), (note, name)


def _join(first, second, whole, note):
    """two calls, the second continued from the first's `last`, are the one call"""
    for name in ("theta", "logp", "fullchi2", "best"):
        assert np.array_equal(np.concatenate([getattr(first, name), getattr(second, name)], axis=1), getattr(whole, name)), (note, name)
    assert np.array_equal(second.last, whole.last) and np.array_equal(first.naccept + second.naccept, whole.naccept), note
    assert np.array_equal(first.nswap + second.nswap, whole.nswap), note


@pytest.mark.parametrize("case", list(TU.SYNTH_R))
def test_synthetic_shapes(case):
    """Ladders at every shape the fixtures do not reach (temper_util.SYNTH_R: eight rungs at the smallest shape and at nG = 24, where all 26
    record slots are live in every exchange; nl = 1; two tracers with ndata < 16; NNLO columns of two and of four tracers; the most rungs
    that fit at three, four and five tracers, five of them at TWO with nG odd; P = 8; one rung, with swap uniforms supplied, behind the
    largest footprint).  S = 3, thin = 5, a box and Gaussian theta priors, without and with Jeffreys, two ladders on walker 0, none on 1,
    one on 2: the host loop around the device's own records, bit for bit.  The inputs meet temper_util.mixed_in_sum on the device's ln P as
    they do on the host (test_draw_temper.py); the draw call returns the same bits before and after."""
    pb, _, eng, make = _synthetic(case)
    _, lin = TU.synthetic_inputs(case)
    R, (N, T, P) = lin["beta"].size, lin["step"].shape
    assert R == TU.SYNTH_R[case] and lin["counts"] == [2 * R, 0, R]
    off, prior, K = SY.offsets(lin["counts"]), TU.theta_prior(P), T // TU.SYNTH_THIN
    plain = None
    for jeff in (False, True):
        like = make(jeff)
        before = like.logp_draws_params(lin["theta0"], off, pb.f, return_best=True)
        if jeff:  # the second pass is another target: ln P without ln det F2, the same best fits
            assert np.all(before[0] != plain[0]) and np.array_equal(before[2], plain[2])
        plain = before
        got, want = _compare(like, off, pb.f, lin, TU.SYNTH_THIN, S=TU.SYNTH_S, **prior)
        print(case, "R", R, {k: np.asarray(v).tolist() for k, v in TU.mixing_counts(want, T).items()})
        assert TU.mixed_in_sum(want, T)
        assert got.theta.shape == (N, K, P) and got.best.shape == (N, K, pb.nG) and got.nswap.shape == (3, max(R - 1, 1)) and got.sum_logp.shape == (N,)
        assert all(np.all(np.isfinite(a)) for a in (got.theta, got.logp, got.fullchi2, got.best, got.last, got.sum_logp)) and np.all(got.nswap >= 0)
        _stored_records_are_the_draw_call(like, off, pb.f, got)
        for a, b in zip(before, like.logp_draws_params(lin["theta0"], off, pb.f, return_best=True)):  # the Gram cache and the buffers are not disturbed
            assert np.array_equal(a, b)
        if R == 1:  # one rung with S = 3 and swap uniforms supplied (there is no pair to read them) is the chain call
            assert lin["lnu_swap"].shape == (3, T // TU.SYNTH_S, 0) and np.all(got.nswap == 0)
            ch = like.metropolis_draws_params(lin["theta0"], off, pb.f, lin["step"], lin["lnu"], thin=TU.SYNTH_THIN, lower=lin["lower"], upper=lin["upper"], **prior)
            for name in ("theta", "logp", "last", "naccept"):
                assert np.array_equal(getattr(got, name), getattr(ch, name)), name
    eng.close()


@pytest.mark.parametrize("name", ["F", "H", "J", "F/1024"])
def test_rungs_at_the_lds_limit(name):
    """The most rungs that fit (temper_util.TEMPER_RUNGS: five at case F, three at H and J; four at F under the recipe padded to 1024 entries,
    whose own five no longer fit) run and are the host loop; one rung more is refused by a message that names R, the rungs that fit, J + 1,
    nG and P; after the refusal the chain call and the call at the limit return their earlier bits.  (Case E has no such limit: a recipe of
    one tracer holds at most 675 entries, and eight rungs fit beside every one of them.)"""
    from eftpipe_amd import _lib as L

    pb, rec, eng, make = _synthetic(name)
    like = make()
    case = name.split("/")[0]
    J1, nG, nnz = TU.case_shape(case, rec)
    fit = (TU.TEMPER_RUNGS_PADDED if rec is not None else TU.TEMPER_RUNGS)[case]
    assert TU.lds_waves(J1, nG, nnz) == fit < 8 and nnz == (TU.PADDED if rec is not None else nnz)
    _, lin = TU.synthetic_inputs(name)
    T, P = lin["step"].shape[1], pb.P
    assert lin["beta"].size == fit
    off, prior = SY.offsets(lin["counts"]), TU.theta_prior(P)
    chain = lambda: like.metropolis_draws_params(lin["theta0"], off, pb.f, lin["step"], lin["lnu"], thin=TU.SYNTH_THIN, lower=lin["lower"], upper=lin["upper"],
                                                 return_best=True, **prior)
    ch = chain()
    got, want = _compare(like, off, pb.f, lin, TU.SYNTH_THIN, S=TU.SYNTH_S, **prior)
    print(name, "R", fit, {k: np.asarray(v).tolist() for k, v in TU.mixing_counts(want, T).items()})
    assert TU.mixed_in_sum(want, T) and np.all(np.isfinite(got.logp))
    _stored_records_are_the_draw_call(like, off, pb.f, got)
    _, more = TU.synthetic_inputs(name, T=6, R=fit + 1)
    with pytest.raises(L.EftbError, match="R = %d rungs needs %d waves in one workgroup, but %d fit the LDS .* J \\+ 1 = %d columns with nG = %d and P = %d" %
                       (fit + 1, fit + 1, fit, J1, nG, P)):
        like.temper_draws_params(more["theta0"], SY.offsets(more["counts"]), pb.f, more["beta"], more["step"], more["lnu"], more["lnu_swap"], swap_every=TU.SYNTH_S,
                                 lower=more["lower"], upper=more["upper"], **prior)
    for a, b in zip(ch, chain()):
        assert np.array_equal(a, b)
    again, _ = _compare(like, off, pb.f, lin, TU.SYNTH_THIN, S=TU.SYNTH_S, **prior)
    _fields_equal(again, got, "after the refusal")
    eng.close()


def test_odd_ladder_across_the_launch_boundary():
    """Case G at its three rungs, T = 260 > 256, S = 3, thin = 7, one ladder on each of two walkers.  The first launch holds the 85 events
    0 ... 84, the last on step 254 (counted from 0), and ends on step 255 between two events: the second launch starts one step into an
    interval (two steps to its first event) and on the odd pair (1, 2), which the first launch started on (0, 1); at R = 3 one rung idles in
    every event.  The call is the host loop, and equals the continuations from `last` after 100 steps (one step past event 32), after 98
    (two steps before it) and after 99 (on it) with first_step set."""
    pb, _, eng, make = _synthetic("G")
    like = make()
    _, lin = TU.synthetic_inputs("G/long", TU.LONG_LADDERS, S=TU.LONG_S)
    S, T, prior = TU.LONG_S, 260, TU.theta_prior(pb.P)
    assert lin["beta"].size == 3 and lin["step"].shape[:2] == (6, T) and (256 // S) % 2 == 1 and 256 % S == 1
    off = SY.offsets(lin["counts"])
    got, _ = _compare(like, off, pb.f, lin, TU.LONG_THIN, S=S, **prior)
    one, want = _compare(like, off, pb.f, lin, 1, S=S, **prior)
    print("G/long", {k: np.asarray(v).tolist() for k, v in TU.mixing_counts(want, T).items()})
    assert TU.mixed_in_sum(want, T)
    assert np.array_equal(got.theta, one.theta[:, 6::7]) and np.array_equal(got.best, one.best[:, 6::7]) and np.array_equal(got.last, one.last)
    assert np.array_equal(got.nswap, one.nswap) and np.array_equal(got.naccept, one.naccept) and np.array_equal(got.sum_logp, one.sum_logp)
    for T1 in (100, 98, 99):
        cut = lambda a, b: dict(lin, step=np.ascontiguousarray(lin["step"][:, a:b]), lnu=np.ascontiguousarray(lin["lnu"][:, a:b]),
                                lnu_swap=np.ascontiguousarray(lin["lnu_swap"][:, a // S : b // S]))
        first, _ = _compare(like, off, pb.f, cut(0, T1), 1, S=S, **prior)
        second, _ = _compare(like, off, pb.f, dict(cut(T1, T), theta0=first.last), 1, S=S, first_step=T1, **prior)
        _join(first, second, one, T1)
    eng.close()


def _many_ladders(n0, **kw):
    """case Gf at its three rungs with n0 ladders on walker 0 and one on walker 2, T = 4, S = 2: events 0 and 1 try each pair once"""
    _, lin = TU.synthetic_inputs("Gf", [n0, 0, 1], T=4, S=2, **kw)
    assert lin["beta"].size == 3
    return lin


def test_every_workgroup_loops_at_three_waves():
    """nG = 24 at three waves (case Gf): the launcher spreads a walker's ladders over up to 2048 / C workgroups (draw_shares), 682 with the C = 3
    walkers of the case, so with 690 ladders on walker 0 the first eight workgroups take a second ladder in the same LDS.  The host loop, bit
    for bit"""
    pb, _, eng, make = _synthetic("Gf")
    like = make()
    n0 = 2048 // len(pb.counts) + 8  # (2048 / C workgroups per walker, C walkers: not the rung count, which is 3 as well)
    lin = _many_ladders(n0)
    got, want = _compare(like, SY.offsets(lin["counts"]), pb.f, lin, 2, S=2, **TU.theta_prior(pb.P))
    print("Gf", n0 + 1, "ladders", {k: np.asarray(v).tolist() for k, v in TU.mixing_counts(want, 4).items()})
    assert got.nswap.shape == (n0 + 1, 2) and TU.mixed_in_sum(want, 4) and np.all(np.isfinite(got.logp))
    eng.close()


def test_failed_ladder_at_three_waves():
    """Case Gf under its flat prior with the singular recipe of test_failing_draw_between_regular_ones (theta_0 = 0: an exactly zero row and
    column of F2).  A walker's ladders go to 2048 / C = 682 workgroups (C = 3 walkers); walker 0 owns 2 x 682 + 8 ladders, so workgroup 3
    works the ladders 3, 685 and 1367; rung 1 of ladder 685 starts on the singular plane.  That ladder is NaN in every field with naccept = nswap = -1, and every other ladder, those before and after it in
    the same workgroup's LDS included, has the bits of the call without it."""
    nG = SY.CASES["Gf"]["nG"]
    kw = dict(kind="flat", singular=nG // 2 + 1)
    pb, _, eng, make = _synthetic("Gf", **kw)
    like = make()
    wgs, R = 2048 // len(pb.counts), 3  # the workgroups of a walker (2048 / C at C = 3 walkers) and the rungs
    assert wgs == 682
    n0, bad = 2 * wgs + 8, wgs + 3
    lin = _many_ladders(n0, **kw)
    lin["theta0"][bad * R + 1, 0] = 0.0
    lin["lower"][0] = -0.1  # (the box holds the singular start)
    off, prior = SY.offsets(lin["counts"]), TU.theta_prior(pb.P)
    with pytest.raises(RuntimeError, match="det of F2ij"):
        like.temper_draws_params(lin["theta0"], off, pb.f, lin["beta"], lin["step"], lin["lnu"], lin["lnu_swap"], swap_every=2, lower=lin["lower"], upper=lin["upper"],
                                 **prior)
    raw, want = _compare(like, off, pb.f, lin, 2, S=2, raw=True, **prior)
    print("Gf flat, singular", n0 + 1, "ladders", {k: np.asarray(v).tolist() for k, v in TU.mixing_counts(want, 4).items()})
    chains = np.arange(bad * R, bad * R + R)
    keep = np.setdiff1d(np.arange(lin["theta0"].shape[0]), chains)
    assert np.all(raw.naccept[chains] == -1) and np.all(raw.nswap[bad] == -1) and np.all(np.isnan(raw.sum_logp[chains]))
    assert all(np.all(np.isnan(a[chains])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last))
    assert all(np.all(np.isfinite(a[keep])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last, raw.sum_logp))
    assert np.all(raw.naccept[keep] >= 0) and np.all(np.delete(raw.nswap, bad, axis=0) >= 0) and TU.mixed_in_sum(want, 4)
    rest = dict(_pick(lin, keep), counts=[(n0 - 1) * R, 0, R])
    alone, _ = _compare(like, SY.offsets(rest["counts"]), pb.f, rest, 2, S=2, **prior)
    for name in FIELDS:
        a, b = getattr(alone, name), getattr(raw, name)
        assert np.array_equal(a, np.delete(b, bad, axis=0) if name == "nswap" else b[keep]), name
    eng.close()


def test_groups_at_two_tracers():
    """groups= at two tracers (case C, ndata < 16) with two data vectors and groups that repeat a walker, four rungs: the call is the host
    loop around logp_draws_params(groups=) on every group's own data, and the groups on data set 0 return the bits of the call without groups"""
    pb, _, eng, make = _synthetic("C")
    whole, counts, plain, own = TU.groups_inputs("C")
    wk, ds = np.array([g[0] for g in TU.GROUPS]), np.array([g[1] for g in TU.GROUPS])
    off, prior, T, R = SY.offsets(counts), TU.theta_prior(pb.P), whole["step"].shape[1], whole["beta"].size
    Ds = datasets(pb.D, pb.invcov, 2)
    assert np.array_equal(Ds[0], pb.D) and R == 4
    first = None
    for jeff in (False, True):
        like = make(jeff)
        like.set_datasets(Ds)
        start = _records(like, off, pb.f, (wk, ds))(whole["theta0"])[0]
        assert first is None or np.all(start != first)  # (the second pass is another target: ln P without ln det F2)
        first = start
        got, want = _compare(like, off, pb.f, whole, TU.SYNTH_THIN, S=TU.SYNTH_S, groups=(wk, ds), **prior)
        print("C groups", {k: np.asarray(v).tolist() for k, v in TU.mixing_counts(want, T).items()})
        assert TU.mixed_in_sum(want, T) and np.all(np.isfinite(got.logp))
        _stored_records_are_the_draw_call(like, off, pb.f, got, groups=(wk, ds))
        base, _ = _compare(like, SY.offsets(plain["counts"]), pb.f, plain, TU.SYNTH_THIN, S=TU.SYNTH_S, **prior)
        for name in FIELDS:
            a, b = getattr(base, name), getattr(got, name)
            assert np.array_equal(a, b[own[::R] // R] if name == "nswap" else b[own]), name
        # the groups on data set 1 are fitted to another vector: other bits than the same ladders would have on data set 0
        lp1, lp0 = _records(like, off, pb.f, (wk, ds))(whole["theta0"])[0][:R], _records(like, SY.offsets([0, 0, R]), pb.f)(whole["theta0"][:R])[0]
        assert np.all(lp1 != lp0)
    eng.close()
