"""Affine-invariant ensembles over the draw parameters on the device (eftb_draws_ensemble_params; MarginalLikelihood.ensemble_draws_params).
Yardstick: the project's own synchronous route -- ensemble_util.host_ensemble (pinned to the mathematics by test_draw_ensemble.py) around the
records of eftb_draws_logp_params, as test_gpu_draw_chains._records asks for them.  Everything is compared bit for bit: the states, ln P, full
chi2, the best fits, the last state and the accept counts.  The inputs are those test_draw_ensemble.py has checked to move, to be refused and to
meet the box; the replayed ensembles are asked again."""
import ctypes as C

import numpy as np
import pytest

import ensemble_util as EU
import synth_like_util as SY
import temper_util as TU
from test_draw_datasets import datasets
from test_gpu_draw_chains import _engine, _like, _records, _stored_records_are_the_draw_call
from test_gpu_draws import _marg, _offsets
from test_gpu_draws_params import _marg_case

pytestmark = pytest.mark.gpu

FIELDS = ("theta", "logp", "fullchi2", "best", "last", "naccept")


def _same(got, want):
    """a DrawChains of the device against host_ensemble's dict around the device's records"""
    for name, b in zip(FIELDS, (want["theta"], want["logp"], want["extras"][0], want["extras"][1], want["last"], want["naccept"])):
        a = getattr(got, name)
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), name


def _compare(like, off, f, ein, thin, groups=None, raw=False, **prior):
    """the device call against the host loop -> (DrawChains, host_ensemble's dict)"""
    box = {k: ein[k] for k in ("lower", "upper") if k in ein}
    want = EU.host_ensemble(_records(like, off, f, groups), ein["theta0"], ein["K"], ein["z"], ein["pick"], ein["lnq"], thin, box.get("lower"), box.get("upper"),
                            prior.get("prior_loc"), prior.get("prior_scale"))
    call = like._ensemble_raw if raw else like.ensemble_draws_params
    got = call(ein["theta0"], off, f, ein["K"], ein["z"], ein["pick"], ein["lnq"], thin=thin, groups=groups, return_best=True, **box, **prior)
    _same(got, want)
    return got, want


def _fields_equal(a, b, note, sel=None):
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert np.array_equal(x, y if sel is None else y[sel], equal_nan=True), (note, name)


@pytest.mark.parametrize("tag", ["auto", "cross", "full", "nnlo"])
def test_ensembles_are_the_host_loop_bit_for_bit(golden, tag):
    """K = 4, T = 37, thin = 5, walkers with 0, 1 and 3 ensembles, under every prior of the case (Gaussian, Jeffreys and, on auto, flat);
    full is the TWO instantiation.  The draw call, the chain call and the tempering call return the same bits before and after."""
    from eftpipe_amd.marginal import temper_ladder

    case, ein = EU.ensemble_case(tag)
    eng = _engine(golden, tag, case)
    off, f, T = _offsets(ein["counts"]), case["f"], EU.T_ENS
    N, P, nG = ein["theta0"].shape[0], ein["theta0"].shape[1], case["rec"].ng1 - 1
    inp, coff = case["inp"], _offsets(case["counts"])
    for i in range(len(case["priors"])):
        like = _like(eng, case, i)
        before = like.logp_draws_params(ein["theta0"], off, f, return_best=True)
        chain = lambda: like.metropolis_draws_params(inp["theta0"], coff, f, inp["step"], inp["lnu"], thin=EU.THIN, lower=inp["lower"], upper=inp["upper"],
                                                     return_best=True)
        ladder = lambda: like._temper_raw(ein["theta0"], off, f, temper_ladder(2, 0.5), np.zeros((N, 3, P)) + inp["step"][0, :3], np.full((N, 3), -1.0),
                                          np.full((N // 2, 1, 1), -0.5), swap_every=2, return_best=True)
        ch, lad = chain(), ladder()
        got, want = _compare(like, off, f, ein, EU.THIN)
        Kt = T // EU.THIN
        assert got.theta.shape == (N, Kt, P) and got.logp.shape == (N, Kt) and got.best.shape == (N, Kt, nG) and got.naccept.dtype == np.int64
        print(tag, i, "naccept", got.naccept, "outside the box", want["outside"])
        assert EU.mixed(want, T) and np.all(np.isfinite(got.theta)) and np.all(np.isfinite(got.logp))
        _stored_records_are_the_draw_call(like, off, f, got)
        for a, b in zip(before, like.logp_draws_params(ein["theta0"], off, f, return_best=True)):
            assert np.array_equal(a, b)
        for a, b in zip(ch, chain()):
            assert np.array_equal(a, b)
        for a, b in zip(lad, ladder()):
            assert np.array_equal(a, b, equal_nan=True)
        if i:
            continue
        lean = like.ensemble_draws_params(ein["theta0"], off, f, 4, ein["z"], ein["pick"], ein["lnq"], thin=EU.THIN, lower=ein["lower"], upper=ein["upper"])
        assert lean.fullchi2 is None and lean.best is None and np.array_equal(lean.theta, got.theta) and np.array_equal(lean.naccept, got.naccept)
        # a Gaussian prior on theta changes the ensembles as the host loop says
        mid, wid = 0.5 * (ein["lower"] + ein["upper"]), 0.1 * (ein["upper"] - ein["lower"])
        c, _ = _compare(like, off, f, ein, EU.THIN, prior_loc=mid, prior_scale=wid)
        assert not np.array_equal(c.theta, got.theta)
    eng.close()


@pytest.mark.parametrize("K", list(EU.SIZES))
def test_other_ensemble_sizes(golden, K):
    """marg.npz auto under its three priors: K = 2 (one wave, one member per half), 6 (three waves: an odd half), 16 (eight waves, one pass),
    20 (eight waves, two passes, the second with two members) and ENS_MAXK = 64 (four passes)"""
    case, ein = EU.size_case(K)
    eng = _engine(golden, "auto", case)
    off, f = _offsets(ein["counts"]), case["f"]
    for i in range(len(case["priors"])):
        like = _like(eng, case, i)
        got, want = _compare(like, off, f, ein, EU.THIN)
        print("K", K, i, "naccept", got.naccept.min(), "...", got.naccept.max(), "outside the box", want["outside"])
        assert EU.mixed(want, EU.T_ENS) and got.theta.shape[0] == K * sum(EU.SIZES[K][0])
        if i == 0:
            _stored_records_are_the_draw_call(like, off, f, got)
    eng.close()


def test_long_call_crosses_the_launch_boundary(golden):
    """T = 300 > 256: two launches.  The call equals the host loop, a 100 + 200 split from `last` and a 99 + 201 split; at thin = 299 the
    first launch stores nothing and the second the one state there is"""
    case, ein = EU.long_case()
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    off, f = _offsets(ein["counts"]), case["f"]
    got, _ = _compare(like, off, f, ein, 7)
    one, want = _compare(like, off, f, ein, 1)
    assert EU.mixed(want, 300)
    assert np.array_equal(got.theta, one.theta[:, 6::7]) and np.array_equal(got.best, one.best[:, 6::7]) and np.array_equal(got.last, one.last)
    assert np.array_equal(got.naccept, one.naccept)
    for T1 in (100, 99):
        first, _ = _compare(like, off, f, EU.cut(ein, 0, T1), 1)
        second, _ = _compare(like, off, f, dict(EU.cut(ein, T1, 300), theta0=first.last), 1)
        for name in ("theta", "logp", "fullchi2", "best"):
            assert np.array_equal(np.concatenate([getattr(first, name), getattr(second, name)], axis=1), getattr(one, name)), (T1, name)
        assert np.array_equal(second.last, one.last) and np.array_equal(first.naccept + second.naccept, one.naccept)
    rare, _ = _compare(like, off, f, ein, 299)
    assert rare.theta.shape[:2] == (8, 1) and np.array_equal(rare.theta[:, 0], one.theta[:, 298]) and np.array_equal(rare.last, one.last)
    eng.close()


def test_order_and_split_of_the_ensembles(golden):
    """the same ensembles in another order, and split over two calls with other offsets, give the same bits per ensemble"""
    case, ein = EU.ensemble_case("auto")
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    f, counts, K = case["f"], np.array(ein["counts"]), 4
    off = _offsets(counts)
    whole, _ = _compare(like, off, f, ein, EU.THIN)
    # walker 0's three ensembles in the order 2, 0, 1
    order = np.concatenate([np.arange(8, 12), np.arange(0, 8), np.arange(12, counts.sum())])
    part, _ = _compare(like, off, f, EU.take(ein, order), EU.THIN)
    _fields_equal(part, whole, "order", order)
    cutc = np.array([K, 0, K, 0])
    sel_a = np.concatenate([np.arange(off[c], off[c] + cutc[c]) for c in range(4)])
    sel_b = np.concatenate([np.arange(off[c] + cutc[c], off[c + 1]) for c in range(4)])
    for sel, cnt in ((sel_a, cutc), (sel_b, counts - cutc)):
        part, _ = _compare(like, _offsets(cnt), f, EU.take(ein, sel), EU.THIN)
        _fields_equal(part, whole, "split", sel)
    none = like.ensemble_draws_params(np.zeros((0, 3)), [0, 0, 0, 0, 0], f, 4, np.ones((0, 4)), np.zeros((0, 4), dtype=np.int32), np.zeros((0, 4)), thin=2,
                                      return_best=True)
    assert none.theta.shape == (0, 2, 3) and none.naccept.shape == (0,)
    eng.close()


def test_groups_ensembles_against_their_own_data(golden):
    """groups= after set_datasets (M = 3) against the host loop through logp_draws_params(groups=); the groups of data set 0 are the call
    without groups bit for bit"""
    case, ein = EU.ensemble_case("auto")
    eng = _engine(golden, "auto", case)
    f = case["f"]
    groups = [(3, 2), (0, 0), (2, 0), (0, 1), (2, 1)]
    counts = [4, 8, 4, 0, 4]  # 20 chains: the case's five ensembles
    assert sum(counts) == ein["theta0"].shape[0]
    wk, ds = np.array([w for w, _ in groups]), np.array([m for _, m in groups])
    off = _offsets(counts)
    Ds = datasets(case["D"], case["Ci"], 3)
    assert np.array_equal(Ds[0], case["D"])
    for i in (0, 1):
        like = _like(eng, case, i)
        like.set_datasets(Ds)
        got, want = _compare(like, off, f, ein, EU.THIN, groups=(wk, ds))
        print("groups", i, "naccept", got.naccept)
        assert np.all(got.naccept >= 0) and np.all(np.isfinite(got.logp)) and 0 < got.naccept.sum() < got.naccept.size * EU.T_ENS
        _stored_records_are_the_draw_call(like, off, f, got, groups=(wk, ds))
        own = sorted((q for q, (w, m) in enumerate(groups) if m == 0), key=lambda q: groups[q][0])
        sel = np.concatenate([np.arange(off[q], off[q + 1]) for q in own])
        cnt = np.zeros(4, dtype=int)
        for q in own:
            cnt[groups[q][0]] = counts[q]
        plain, _ = _compare(like, _offsets(cnt), f, EU.take(ein, sel), EU.THIN)
        _fields_equal(plain, got, "groups", sel)
    eng.close()


# ----------------------------------------------------------------------------- the synthetic likelihoods (synth_like_util.CASES)
def _synthetic(name, kind="gauss", singular=None):
    from test_gpu_draw_synthetic import _engine as s_engine, _like as s_like, _put

    pb = SY.case_problem(name, kind, singular)
    eng = s_engine(pb, len(pb.counts) * pb.ntr)
    _put(eng, pb)
    return pb, eng, lambda jeffreys=False: s_like(eng, pb, jeffreys)


def test_passes_from_the_lds_limit():
    """Case G (J + 1 = 97, nG = 24: the TWO instantiation) holds three waves beside eight members, so the four members of a half take two
    passes, the second with one wave at work.  A box and Gaussian theta priors, without and with Jeffreys: the host loop, bit for bit"""
    pb, eng, make = _synthetic("G")
    ein = EU.synthetic_inputs("G")
    K, T = ein["K"], ein["z"].shape[1]
    assert K == 8 and EU.case_waves("G", K) == 3
    off, prior = SY.offsets(ein["counts"]), EU.theta_prior(pb.P)
    for jeff in (False, True):
        like = make(jeff)
        before = like.logp_draws_params(ein["theta0"], off, pb.f, return_best=True)
        got, want = _compare(like, off, pb.f, ein, EU.THIN, **prior)
        print("G", jeff, "naccept", got.naccept, "outside the box", want["outside"])
        assert EU.mixed(want, T) and all(np.all(np.isfinite(a)) for a in (got.theta, got.logp, got.fullchi2, got.best, got.last))
        _stored_records_are_the_draw_call(like, off, pb.f, got)
        for a, b in zip(before, like.logp_draws_params(ein["theta0"], off, pb.f, return_best=True)):
            assert np.array_equal(a, b)
    eng.close()


def test_members_at_the_lds_limit():
    """Case I (J + 1 = 121, nG = 24) holds 24 members beside one wave, which takes all twelve of a half in turn; two members more are refused
    by a message that names K, J + 1, nG and P, and the call at the limit then returns its earlier bits"""
    from eftpipe_amd import _lib as L

    pb, eng, make = _synthetic("I")
    like = make()
    most = EU.most_members("I")
    ein = EU.synthetic_inputs("I")
    J1, nG, _ = TU.case_shape("I")
    assert most == ein["K"] == 24 and EU.case_waves("I", most) == 1 and EU.case_waves("I", most + 2) == 0
    off, prior, T = SY.offsets(ein["counts"]), EU.theta_prior(pb.P), ein["z"].shape[1]
    got, want = _compare(like, off, pb.f, ein, 2, **prior)
    print("I", "naccept", got.naccept, "outside the box", want["outside"])
    assert EU.mixed(want, T) and np.all(np.isfinite(got.logp))
    more = EU.synthetic_ensemble("I", most + 2, [1, 0, 1], 6, 3, 0.01)
    with pytest.raises(L.EftbError, match="K = %d members needs .* no room for one wave .* J \\+ 1 = %d columns with nG = %d and P = %d" % (most + 2, J1, nG, pb.P)):
        like.ensemble_draws_params(more["theta0"], SY.offsets(more["counts"]), pb.f, most + 2, more["z"], more["pick"], more["lnq"], **prior)
    again, _ = _compare(like, off, pb.f, ein, 2, **prior)
    _fields_equal(again, got, "after the refusal")
    eng.close()


def test_a_workgroup_takes_a_second_ensemble_and_one_fails():
    """Case Gf under its flat prior with the singular recipe of test_failing_draw_between_regular_ones (theta_0 = 0: an exactly zero row and
    column of F2), K = 2, T = 4.  A walker's ensembles go to 2048 / C = 682 workgroups (C = 3 walkers); walker 0 owns 2 x 682 + 8 ensembles,
    so workgroup 3 works the ensembles 3, 685 and 1367; member 1 of ensemble 685 starts on the singular plane.  That ensemble is NaN in
    every field with naccept = -1, and every other ensemble, those before and after it in the same workgroup's LDS included, has the bits of
    the call without it."""
    nG = SY.CASES["Gf"]["nG"]
    kw = dict(kind="flat", singular=nG // 2 + 1)
    pb, eng, make = _synthetic("Gf", **kw)
    like = make()
    wgs, K = 2048 // len(pb.counts), 2
    assert wgs == 682
    n0, bad = 2 * wgs + 8, wgs + 3
    ein = EU.synthetic_inputs("Gf", [n0, 0, 1], **kw)
    ein["theta0"][bad * K + 1, 0] = 0.0
    ein["lower"][0] = -0.1  # (the box holds the singular start)
    off, prior = SY.offsets(ein["counts"]), EU.theta_prior(pb.P)
    with pytest.raises(RuntimeError, match="det of F2ij"):
        like.ensemble_draws_params(ein["theta0"], off, pb.f, K, ein["z"], ein["pick"], ein["lnq"], lower=ein["lower"], upper=ein["upper"], **prior)
    raw, want = _compare(like, off, pb.f, ein, 2, raw=True, **prior)
    chains = np.arange(bad * K, bad * K + K)
    keep = np.setdiff1d(np.arange(ein["theta0"].shape[0]), chains)
    assert np.all(raw.naccept[chains] == -1) and all(np.all(np.isnan(a[chains])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last))
    assert all(np.all(np.isfinite(a[keep])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last)) and np.all(raw.naccept[keep] >= 0)
    assert EU.mixed_in_sum(want, 4)  # (T = 4: the condition summed over the ensembles, as the host checks these inputs)
    rest = dict(EU.take(ein, keep), counts=[(n0 - 1) * K, 0, K])
    alone, _ = _compare(like, SY.offsets(rest["counts"]), pb.f, rest, 2, **prior)
    _fields_equal(alone, raw, "without the failed ensemble", keep)
    eng.close()


# ----------------------------------------------------------------------------- refusals
def test_failed_ensemble_and_refusals(golden):
    from eftpipe_amd import _lib as L
    from eftpipe_amd.marginal import MarginalLikelihood, stretch_proposals
    from eftpipe_amd.parambasis import DrawRecipe

    g, eng, T, index = _marg(golden, "auto", max_batch=4)
    rec, theta, _, _, f = _marg_case(g, "auto", [4, 4])
    D, Ci = g["auto_D"], g["auto_invcov"]
    nG = len(g["auto_loc"])
    eng.put("TEMPL", np.stack([T, T]))
    off = [0, 4, 8]
    N, P, Tn, K = 8, 3, 9, 4
    z, pick, lnq = stretch_proposals(np.random.default_rng(6), N // K, K, Tn, P)
    # ---- det F2 <= 0 where theta_2 = 0 (test_gpu_draw_chains.py): member 3 of ensemble 0 starts on the singular plane
    flat = MarginalLikelihood(eng, index, D, Ci, np.zeros(nG), np.full(nG, np.inf))
    idx3 = rec.idx.copy()
    idx3[rec.row == 3, 2] = 2
    flat.set_draw_recipe(DrawRecipe(rec.param_names, 1, nG + 1, rec.tracer, rec.row, rec.col, rec.coef, rec.fpow, idx3))
    th0 = theta.copy()
    th0[3, 2] = 0.0
    ein = dict(theta0=th0, z=z, pick=pick, lnq=lnq, K=K)
    with pytest.raises(RuntimeError, match="det of F2ij"):
        flat.ensemble_draws_params(th0, off, f, K, z, pick, lnq)
    raw, _ = _compare(flat, off, f, ein, 2, raw=True)
    bad, ok = [0, 1, 2, 3], [4, 5, 6, 7]
    assert np.all(raw.naccept[bad] == -1) and all(np.all(np.isnan(a[bad])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last))
    assert all(np.all(np.isfinite(a[ok])) for a in (raw.theta, raw.logp, raw.fullchi2, raw.best, raw.last)) and np.all(raw.naccept[ok] >= 0)
    # ---- refusals
    like = MarginalLikelihood(eng, index, D, Ci, g["auto_loc"], g["auto_scale"])
    with pytest.raises(L.EftbError, match="eftb_draws_ensemble_params: no draw recipe"):
        like.ensemble_draws_params(theta, off, f, K, z, pick, lnq)
    like.set_draw_recipe(rec)
    want = like.ensemble_draws_params(theta, off, f, K, z, pick, lnq)
    call = lambda **kw: like.ensemble_draws_params(**dict(dict(starts=theta, offsets=off, f=f, K=K, z=z, pick=pick, lnq=lnq), **kw))
    # (what the chain call refuses, through the same checks)
    with pytest.raises(L.EftbError, match="prior_scale\\[0\\]"):
        call(prior_scale=[0.0, 1.0, 1.0])
    with pytest.raises(L.EftbError, match="lower\\[1\\] = 2 > upper\\[1\\] = 1"):
        call(lower=[0.0, 2.0, 0.0], upper=[1.0, 1.0, 1.0])
    j = int(np.argmin(theta[:, 1]))
    with pytest.raises(L.EftbError, match="theta0\\[%d\\]\\[1\\] = .* outside" % j):
        call(lower=[-np.inf, np.nextafter(theta[j, 1], np.inf), -np.inf])
    with pytest.raises(L.EftbError, match="eftb_draws_ensemble_params_datasets: no data sets"):
        call(groups=([0, 1], [0, 0]))
    # (its own)
    for Kb, n in ((3, 6), (66, 66), (0, 0)):
        with pytest.raises((L.EftbError, ValueError), match="K = %d members, not an even number in \\[2, 64\\]|not a multiple of the K" % Kb):
            like.ensemble_draws_params(np.zeros((n, P)), [0, n, n], f, Kb, np.ones((n, Tn)), np.zeros((n, Tn), dtype=np.int32), np.zeros((n, Tn)))
    with pytest.raises(L.EftbError, match="K = 66 members, not an even number in \\[2, 64\\]"):
        like.ensemble_draws_params(np.zeros((66, P)), [0, 66, 66], f, 66, np.ones((66, Tn)), np.zeros((66, Tn), dtype=np.int32), np.zeros((66, Tn)))
    with pytest.raises(L.EftbError, match="K = 1 members, not an even number"):
        call(K=1)
    with pytest.raises(L.EftbError, match="walker 0 owns 2 chains, not a multiple of K = 4 members"):
        call(offsets=[0, 2, 8])
    for v in (np.nan, np.inf, -np.inf, 0.0, -0.5):
        b = z.copy()
        b[6, 5] = v
        with pytest.raises(L.EftbError, match="z\\[6\\]\\[5\\] = .* \\(ensemble 1, member 2, sweep 5\\) is not a finite stretch factor > 0"):
            call(z=b)
    for v in (-1, 2, 100):
        b = pick.copy()
        b[5, 8] = v
        with pytest.raises(L.EftbError, match="pick\\[5\\]\\[8\\] = %d \\(ensemble 1, member 1, sweep 8\\) outside \\[0, K / 2 = 2\\)" % v):
            call(pick=b)
    for v in (np.nan, np.inf):
        b = lnq.copy()
        b[2, 0] = v
        with pytest.raises(L.EftbError, match="lnq\\[2\\]\\[0\\] = .* \\(ensemble 0, member 2, sweep 0\\) is NaN or \\+inf"):
            call(lnq=b)
    # lnq > 0 and lnq = -inf are not refused: the host loop says what they do
    b = lnq.copy()
    b[:, ::2], b[:, 1::3] = 0.75, -np.inf
    free, _ = _compare(like, off, f, dict(theta0=theta, z=z, pick=pick, lnq=b, K=K), 1)
    assert not np.array_equal(free.theta, want.theta)
    # the raw entry point with NULL optional arguments
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    th, fo, o64 = np.ascontiguousarray(theta), np.ascontiguousarray(f), np.asarray(off, dtype=np.int64)
    out = [np.zeros((N, Tn, P)), np.zeros((N, Tn)), np.zeros((N, Tn)), np.zeros((N, Tn, nG)), np.zeros((N, P))]
    nacc = np.zeros(N, dtype=np.int64)
    rc = eng.lib.eftb_draws_ensemble_params(eng._h, 2, N, K, Tn, 1, i64(o64), dp(th), dp(fo), dp(z), pick.ctypes.data_as(C.POINTER(C.c_int32)), dp(lnq), None, None,
                                            None, None, *[dp(a) for a in out], i64(nacc))
    assert rc == 0 and np.array_equal(out[0], want.theta) and np.array_equal(out[4], want.last) and np.array_equal(nacc, want.naccept)
    rc = eng.lib.eftb_draws_ensemble_params(eng._h, 2, N, K, Tn, 1, i64(o64), dp(th), dp(fo), None, pick.ctypes.data_as(C.POINTER(C.c_int32)), dp(lnq), None, None,
                                            None, None, *[dp(a) for a in out], i64(nacc))
    assert rc != 0 and "null argument" in eng.lib.eftb_last_error().decode()
    assert np.array_equal(call().theta, want.theta)
    eng.close()
