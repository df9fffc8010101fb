"""Dragging chains between two walkers on the device (eftb_draws_drag_params; MarginalLikelihood.drag_draws_params).
Yardstick: the project's own synchronous route -- a host loop that forms every proposal in NumPy, asks eftb_draws_logp_params for its
record at the start walker and at the end walker (the chains reordered by walker, as that call needs) and applies drag_util.host_drag's
rule (pinned to the mathematics by test_draw_drag.py).  Everything is compared bit for bit: the states, both ln P, both full chi2, both best
fits, the last state, the accept counts and the two sums.  The inputs are those test_draw_drag.py has checked to move, to be refused and to
feel the end walker; the replayed chains are asked again."""
import numpy as np
import pytest

import chain_util as CU
import drag_util as DU
import synth_like_util as SY
from drag_util import T37
from test_draw_chains import long_inputs
from test_gpu_draw_chains import _records
from test_gpu_draws import _marg, _offsets
from test_gpu_draws_grad import _nnlo_problem
from test_gpu_draws_params import _cfg3_engine

from eftpipe_amd.marginal import drag_fractions  # (the feature: without it nothing in this file runs)

pytestmark = pytest.mark.gpu

THIN = 5
PAIRED = ("logp", "fullchi2", "best")
FIELDS = ("theta", "logp_start", "logp_end", "fullchi2_start", "fullchi2_end", "best_start", "best_end", "last", "naccept", "last_logp_start", "last_logp_end",
          "last_fullchi2_start", "last_fullchi2_end", "last_best_start", "last_best_end", "sum_start", "sum_end", "log_ratio")


def _walker_records(like, f, C, w):
    """theta [N, P] -> (ln P, full chi2, best) of eftb_draws_logp_params with chain n at walker w[n]: the chains are handed over sorted by
    walker and the records put back in the caller's order"""
    w = np.asarray(w)
    order = np.argsort(w, kind="stable")
    fun = _records(like, _offsets(np.bincount(w, minlength=C)), f)

    def ask(theta):
        out = []
        for x in fun(np.ascontiguousarray(np.asarray(theta)[order])):
            y = np.empty_like(x)
            y[order] = x
            out.append(y)
        return tuple(out)

    return ask


def _want_fields(want, T):
    ea, eb, la, lb = want["extras_start"], want["extras_end"], want["last_extras_start"], want["last_extras_end"]
    return dict(theta=want["theta"], logp_start=want["logp_start"], logp_end=want["logp_end"], fullchi2_start=ea[0], fullchi2_end=eb[0], best_start=ea[1],
                best_end=eb[1], last=want["last"], naccept=want["naccept"], last_logp_start=want["last_logp_start"], last_logp_end=want["last_logp_end"],
                last_fullchi2_start=la[0], last_fullchi2_end=lb[0], last_best_start=la[1], last_best_end=lb[1], sum_start=want["sum_start"],
                sum_end=want["sum_end"], log_ratio=(want["sum_end"] - want["sum_start"]) / (T + 1))


def _compare(like, f, pairs, pcounts, inp, thin, frac=None, raw=False, **prior):
    """the device call against the host loop -> (DragChains, host_drag's dict)"""
    wa, wb = (np.asarray(p) for p in pairs)
    pair = np.repeat(np.arange(len(pcounts)), pcounts)
    C = np.reshape(f, (-1, like.eng.ntracers)).shape[0]
    box = {k: inp[k] for k in ("lower", "upper") if k in inp}
    T = inp["step"].shape[1]
    want = DU.host_drag(_walker_records(like, f, C, wa[pair]), _walker_records(like, f, C, wb[pair]), inp["theta0"], inp["step"], inp["lnu"],
                        drag_fractions(T) if frac is None else frac, thin, box.get("lower"), box.get("upper"), prior.get("prior_loc"), prior.get("prior_scale"))
    call = like._drag_raw if raw else like.drag_draws_params
    got = call(inp["theta0"], _offsets(pcounts), f, (wa, wb), inp["step"], inp["lnu"], frac=frac, thin=thin, return_best=True, **box, **prior)
    for name, b in _want_fields(want, T).items():
        a = getattr(got, name)
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), name
    return got, want


def _stored_records_are_the_draw_call(like, f, C, a, b, got):
    """every stored record, and the final one, is logp_draws_params' at the stored theta for its walker"""
    for w, end in ((a, "_start"), (b, "_end")):
        fun = _walker_records(like, f, C, w)
        for k in range(got.theta.shape[1]):
            for x, name in zip(fun(got.theta[:, k]), PAIRED):
                assert np.array_equal(x, getattr(got, name + end)[:, k]), (name + end, k)
        for x, name in zip(fun(got.last), PAIRED):
            assert np.array_equal(x, getattr(got, "last_" + name + end)), "last_" + name + end


def _engine(golden, tag, case):
    """the engine of a drag_util.drag_case with the templates of its 2 C walkers put -> eng"""
    C2 = len(case["Ws"])
    if tag == "auto":
        _, eng, _, index = _marg(golden, tag)
    elif tag == "full":
        eng, _, index = _cfg3_engine(golden("cfg3"), C2 // 2, 3 * C2)
    else:
        eng, _, _, _, _, _, _, index, D, _, _ = _nnlo_problem()
        assert np.array_equal(D, case["D"])
    assert np.array_equal(index, case["index"])
    eng.put("TEMPL", case["templ"])
    if case["templn"] is not None:
        eng.put("TEMPLN", case["templn"])
    return eng


def _like(eng, case, i):
    from eftpipe_amd.marginal import MarginalLikelihood

    loc, scale, jeff = case["priors"][i]
    like = MarginalLikelihood(eng, case["index"], case["D"], case["Ci"], loc, scale, jeffreys=jeff)
    like.set_draw_recipe(case["rec"])
    return like


@pytest.mark.parametrize("tag", ["auto", "full", "nnlo"])
def test_drag_is_the_host_loop_bit_for_bit(golden, tag):
    """T = 37 on drag_fractions, a box that refuses proposals, pairs of two walkers with their own templates and growth rates, a pair of one
    walker twice and a pair without a chain, under every prior of the case (Gaussian, Jeffreys, flat) and under box + Gaussian priors on theta;
    thin = 5, 1 and 0.  auto: J + 1 = 25; full: J + 1 = 73, the TWO instantiation, nG = 14; nnlo: J + 1 = 28.  Every stored record is the draw
    call's, and the draw and chain calls return the same bits before and after."""
    case = DU.drag_case(tag)
    eng = _engine(golden, tag, case)
    inp, f, pairs, pc = case["inp"], case["f"], (case["wstart"], case["wend"]), case["pcounts"]
    N, P, nG, C = inp["theta0"].shape[0], inp["theta0"].shape[1], case["rec"].ng1 - 1, len(case["Ws"])
    K = T37 // THIN
    woff = _offsets(np.bincount(case["a"], minlength=C))
    for i in range(len(case["priors"])):
        like = _like(eng, case, i)
        before = like.logp_draws_params(inp["theta0"], woff, f, return_best=True)
        chain_before = like.metropolis_draws_params(inp["theta0"], woff, f, inp["step"], inp["lnu"], thin=THIN, lower=inp["lower"], upper=inp["upper"], return_best=True)
        got, want = _compare(like, f, pairs, pc, inp, THIN)
        assert got.theta.shape == (N, K, P) and got.logp_end.shape == (N, K) and got.best_end.shape == (N, K, nG) and got.last_best_start.shape == (N, nG)
        assert got.naccept.dtype == np.int64 and got.sum_start.shape == (N,) and got.log_ratio.shape == (N,)
        print(tag, i, "naccept", got.naccept, "outside the box", want["outside"], "decided otherwise", want["differ"], "log ratio", got.log_ratio)
        assert DU.moves(want, case, T37)  # the condition of test_draw_drag.py on the replayed chains
        assert all(np.all(np.isfinite(getattr(got, k))) for k in FIELDS)
        _stored_records_are_the_draw_call(like, f, C, case["a"], case["b"], got)
        for a, b in zip(before, like.logp_draws_params(inp["theta0"], woff, f, return_best=True)):  # the Gram cache and the records are not disturbed
            assert np.array_equal(a, b)
        chain_after = like.metropolis_draws_params(inp["theta0"], woff, f, inp["step"], inp["lnu"], thin=THIN, lower=inp["lower"], upper=inp["upper"], return_best=True)
        for a, b in zip(chain_before, chain_after):
            assert np.array_equal(a, b)
        assert not np.array_equal(chain_after.theta, got.theta)  # (the end walker was felt)
        if i:
            continue
        # thin = 1: the thinned chain is a subsequence with the same end
        full, _ = _compare(like, f, pairs, pc, inp, 1)
        for k in ("theta", "logp_start", "logp_end", "fullchi2_start", "fullchi2_end", "best_start", "best_end"):
            assert np.array_equal(getattr(full, k)[:, THIN - 1 :: THIN][:, :K], getattr(got, k)), k
        for k in FIELDS[7:]:
            assert np.array_equal(getattr(full, k), getattr(got, k)), k
        assert np.array_equal(full.last, full.theta[:, -1]) and np.array_equal(full.last_logp_end, full.logp_end[:, -1])
        # thin = 0: no trajectory, the same end
        none, _ = _compare(like, f, pairs, pc, inp, 0)
        assert none.theta.shape == (N, 0, P) and none.logp_start.shape == (N, 0) and none.best_end.shape == (N, 0, nG)
        for k in FIELDS[7:]:
            assert np.array_equal(getattr(none, k), getattr(got, k)), k
        # without return_best the same chains, and no chi2 or best fits
        lean = like.drag_draws_params(inp["theta0"], _offsets(pc), f, pairs, inp["step"], inp["lnu"], thin=THIN, lower=inp["lower"], upper=inp["upper"])
        assert lean.fullchi2_start is None and lean.best_end is None and lean.last_best_start is None
        for k in ("theta", "logp_start", "logp_end", "last", "naccept", "last_logp_end", "sum_start", "sum_end", "log_ratio"):
            assert np.array_equal(getattr(lean, k), getattr(got, k)), k
        # box + Gaussian priors on theta, on all parameters and on one: the chains change as the host loop says
        mid, wid = 0.5 * (inp["lower"] + inp["upper"]), 0.1 * (inp["upper"] - inp["lower"])
        for scale in (wid, np.where(np.arange(P) == 1, wid, np.inf)):
            c, w = _compare(like, f, pairs, pc, inp, THIN, prior_loc=mid, prior_scale=scale)
            assert np.all(w["naccept"] > 0) and not np.array_equal(c.sum_start, got.sum_start)  # (pri is a part of every term of the sums)
            assert tag != "auto" or not np.array_equal(c.theta, got.theta)  # (the other two walk where ln P moves by hundreds per step: a prior this wide turns no decision)
    eng.close()


def test_frac_zero_and_one_are_the_chain_call(golden):
    """frac = 0 everywhere: metropolis_draws_params on the start walkers in theta, logp, last and naccept; frac = 1: on the end walkers; on
    inputs where the other end is finite throughout (asserted on the thin = 1 run)"""
    case = DU.drag_case("auto")
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    inp, f, pairs, pc, C = case["inp"], case["f"], (case["wstart"], case["wend"]), case["pcounts"], len(case["Ws"])
    box = dict(lower=inp["lower"], upper=inp["upper"])
    for lam, w, own, other in ((0.0, case["a"], "_start", "_end"), (1.0, case["b"], "_end", "_start")):
        got, _ = _compare(like, f, pairs, pc, inp, 1, frac=np.full(T37, lam))
        assert np.all(np.isfinite(getattr(got, "logp" + other))) and np.all(np.isfinite(getattr(got, "last_logp" + other)))
        order = np.argsort(w, kind="stable")
        ch = like.metropolis_draws_params(inp["theta0"][order], _offsets(np.bincount(w, minlength=C)), f, inp["step"][order], inp["lnu"][order], thin=1, return_best=True, **box)
        assert np.all(ch.naccept > 0) and np.all(ch.naccept < T37)
        for a, b in ((got.theta, ch.theta), (getattr(got, "logp" + own), ch.logp), (getattr(got, "fullchi2" + own), ch.fullchi2), (getattr(got, "best" + own), ch.best),
                     (got.last, ch.last), (got.naccept, ch.naccept)):
            assert np.array_equal(a[order], b)
    eng.close()


def test_long_drag_crosses_the_launch_boundary(golden):
    """T = 300 > 256: two launches, with theta, the accept counts and the sums kept on the device between them.  The call equals the host
    loop, sums included, and a 100-step call followed by a 200-step call from `last` on the matching slices of frac in states, records,
    `last` and the summed accept counts.  The second call's sums restart from its own start term, so its additions are grouped otherwise:
    sum(T) against sum(T1) + sum(T2) - the start term of the second differs by rounding alone, at most T 2^-53 sum |terms| (T + 1 terms
    added in two orders, each addition rounding a partial sum no larger than sum |terms| by at most 2^-53 of it)."""
    _, inp = long_inputs()  # the first 3 chains of auto, walker 0
    case = DU.drag_case("auto")
    C = len(case["Ws"])
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    f, pairs, pc = case["f"], ([0, 0], [C // 2, 0]), [2, 1]
    T, T1 = 300, 100
    frac = drag_fractions(T)
    got, _ = _compare(like, f, pairs, pc, inp, 7)
    one, want = _compare(like, f, pairs, pc, inp, 1)
    assert np.all(one.naccept > 0) and np.all(one.naccept < T) and np.all(want["outside"] > 0) and np.all(want["differ"][:2] > 0)
    moved = np.any(np.diff(one.theta, axis=1) != 0.0, axis=2)
    assert np.all(moved[:, :255].sum(1) > 0) and np.all(moved[:, 256:].sum(1) > 0)  # on both sides of the boundary
    assert np.array_equal(got.theta, one.theta[:, 6::7]) and np.array_equal(got.logp_end, one.logp_end[:, 6::7])
    for k in FIELDS[7:]:
        assert np.array_equal(getattr(got, k), getattr(one, k)), k
    cut = lambda a, b: dict(inp, step=np.ascontiguousarray(inp["step"][:, a:b]), lnu=np.ascontiguousarray(inp["lnu"][:, a:b]))
    first, _ = _compare(like, f, pairs, pc, cut(0, T1), 1, frac=frac[:T1])
    second, _ = _compare(like, f, pairs, pc, dict(cut(T1, T), theta0=first.last), 1, frac=frac[T1:])
    for name in FIELDS[:7]:
        assert np.array_equal(np.concatenate([getattr(first, name), getattr(second, name)], axis=1), getattr(one, name)), name
    for name in FIELDS[7:15]:
        if name != "naccept":
            assert np.array_equal(getattr(second, name), getattr(one, name)), name
    assert np.array_equal(first.naccept + second.naccept, one.naccept)
    theta0_lp = {"_start": _walker_records(like, f, C, [0, 0, 0])(inp["theta0"])[0], "_end": _walker_records(like, f, C, [C // 2, C // 2, 0])(inp["theta0"])[0]}
    for end in ("_start", "_end"):  # (no Gaussian prior on theta here: pri = 0 and a term is ln P alone)
        whole, parts = getattr(one, "sum" + end), getattr(first, "sum" + end) + getattr(second, "sum" + end) - getattr(first, "last_logp" + end)
        bound = T * 2.0**-53 * (np.abs(theta0_lp[end]) + np.sum(np.abs(getattr(one, "logp" + end)), axis=1))
        print("sum" + end, "whole - parts", whole - parts, "bound", bound)
        assert np.all(np.abs(whole - parts) <= bound)
    eng.close()


def test_a_launch_that_stores_nothing_before_one_that_does(golden):
    """T = 300, thin = 299: the launch of steps 1 ... 256 stores no state and brings nothing back, the second stores the one state there is.
    The record arrays have K + 1 = 2 slots: the stored one and, from the copy at the end of the call, the one after step T.  All of it,
    `last`, the accept counts and the sums are the host loop's."""
    _, inp = long_inputs()  # the first 3 chains of auto, walker 0
    case = DU.drag_case("auto")
    C = len(case["Ws"])
    eng = _engine(golden, "auto", case)
    like = _like(eng, case, 0)
    got, _ = _compare(like, case["f"], ([0, 0], [C // 2, 0]), [2, 1], inp, 299)
    assert got.theta.shape[:2] == (3, 1) and got.logp_end.shape == (3, 1) and got.last_logp_end.shape == (3,) and np.all(got.naccept > 0)
    eng.close()


def test_chains_do_not_depend_on_the_batch(golden):
    """the batch split over two calls with other offsets and the pairs in another order: the same bits per chain"""
    case = DU.drag_case("full")
    eng = _engine(golden, "full", case)
    like = _like(eng, case, 0)
    inp, f, pc = case["inp"], case["f"], case["pcounts"]
    whole, _ = _compare(like, f, (case["wstart"], case["wend"]), pc, inp, THIN)
    G = len(pc)
    poff = _offsets(pc)
    cutc = np.minimum(pc, 1)  # the first chain of every pair, then the others
    rev = np.arange(G)[::-1]
    for lo, hi in ((np.zeros(G, dtype=int), cutc), (cutc, pc)):
        sel = np.concatenate([np.arange(poff[g] + lo[g], poff[g] + hi[g]) for g in rev]).astype(int)
        part, _ = _compare(like, f, (case["wstart"][rev], case["wend"][rev]), (hi - lo)[rev], dict(inp, theta0=inp["theta0"][sel], step=inp["step"][sel], lnu=inp["lnu"][sel]), THIN)
        assert len(sel) > 0
        for name in FIELDS:
            assert np.array_equal(getattr(part, name), getattr(whole, name)[sel]), name
    none = like.drag_draws_params(np.zeros((0, inp["theta0"].shape[1])), [0, 0], f, ([0], [1]), np.zeros((0, 4, inp["theta0"].shape[1])), np.zeros((0, 4)), thin=2, return_best=True)
    assert none.theta.shape == (0, 2, 6) and none.naccept.shape == (0,) and none.best_end.shape == (0, 2, like.nG) and none.log_ratio.shape == (0,)
    eng.close()


def test_failed_starts_nan_proposals_and_refusals(golden):
    """Failures.  Under a flat prior a Gaussian row whose model vanishes gives det F2 = 0.  Row 5 of the recipe, one term c on one column,
    becomes the two terms c theta_2 - c f: it vanishes, exactly, on the plane theta_2 = f of each walker, and the walkers have different f,
    so a point on the plane of the end walker has a finite ln P at the start walker.  Chain 1 starts on the plane of its end walker: the
    public call raises; the raw call returns NaN and -1 for that chain and finite results for the others.  Chain 0 is sent onto the plane
    of its end walker by its first proposal with lnu = -inf (f - 1/2 + 1/2 = f exactly): la1 is finite, lb1 is not, the kernel evaluates
    both, rejects, and the chain goes on.  Then the refusals, by their messages, and the chain call at work afterwards."""
    import ctypes as C

    from eftpipe_amd import _lib as L
    from eftpipe_amd.marginal import MarginalLikelihood
    from eftpipe_amd.parambasis import DrawRecipe
    from test_gpu_draws_params import _marg_case

    g, eng, T, index = _marg(golden, "auto", max_batch=4)
    rec, theta, _, _, f = _marg_case(g, "auto", [2, 2, 0])
    D, Ci = g["auto_D"], g["auto_invcov"]
    nG = len(g["auto_loc"])
    eng.put("TEMPL", np.stack([T, 1.01 * T, 1.02 * T]))
    N, P, Tn = 4, 3, 9
    rng = np.random.default_rng(6)
    step, lnu = rng.standard_normal((N, Tn, P)) * [0.02, 0.1, 0.1], np.log(rng.random((N, Tn)))
    m = rec.row == 5
    assert m.sum() == 1 and rec.fpow[m][0] == 0 and np.all(rec.idx[m] == -1) and len(set(f)) == 3 and np.all((f > 0.5) & (f < 1.0))
    two = lambda a, x, y: np.concatenate([a[~m], np.array([x, y], dtype=a.dtype).reshape((2,) + a.shape[1:])])
    c5 = rec.coef[m][0]
    plane = DrawRecipe(rec.param_names, 1, nG + 1, two(rec.tracer, 0, 0), two(rec.row, 5, 5), two(rec.col, rec.col[m][0], rec.col[m][0]), two(rec.coef, c5, -c5),
                       two(rec.fpow, 0, 1), two(rec.idx, [2, -1, -1], [-1, -1, -1]))
    flat = MarginalLikelihood(eng, index, D, Ci, np.zeros(nG), np.full(nG, np.inf))
    flat.set_draw_recipe(plane)
    pairs, pc = ([0, 0, 1], [1, 2, 0]), [1, 1, 2]
    a, b = np.array([0, 0, 1, 1]), np.array([1, 2, 0, 0])
    th0 = theta.copy()
    th0[1, 2] = f[2]  # chain 1 starts on the plane of its end walker
    th0[0, 2] = f[1] - 0.5  # chain 0 is sent onto the plane of its end walker by its first proposal: any finite pair would be accepted
    step[0, 0] = [0.0, 0.0, 0.5]
    lnu[0, 0] = -np.inf
    assert th0[0, 2] + step[0, 0, 2] == f[1]
    at_a, at_b = _walker_records(flat, f, 3, a), _walker_records(flat, f, 3, b)
    assert np.all(np.isfinite(at_a(th0)[0])) and np.array_equal(np.isnan(at_b(th0)[0]), [False, True, False, False])
    trial = th0 + step[:, 0]
    assert np.isfinite(at_a(trial)[0][0]) and np.isnan(at_b(trial)[0][0])  # la1 finite, lb1 not: the step that is rejected after both evaluations
    inp = dict(theta0=th0, step=step, lnu=lnu)
    with pytest.raises(RuntimeError, match="det of F2ij"):
        flat.drag_draws_params(th0, _offsets(pc), f, pairs, step, lnu)
    raw, _ = _compare(flat, f, pairs, pc, inp, 1, raw=True)
    assert raw.naccept[1] == -1 and all(np.all(np.isnan(getattr(raw, k)[1])) for k in FIELDS if k != "naccept")
    ok = [0, 2, 3]
    assert all(np.all(np.isfinite(getattr(raw, k)[ok])) for k in FIELDS) and np.all(raw.naccept[ok] > 0)
    assert np.array_equal(raw.theta[0, 0], th0[0]) and np.any(raw.theta[0] != th0[0])  # the proposal was rejected and the chain went on
    thinned, _ = _compare(flat, f, pairs, pc, inp, 2, raw=True)
    assert np.array_equal(thinned.last, raw.last, equal_nan=True) and np.array_equal(thinned.naccept, raw.naccept)
    # ---- refusals
    like = MarginalLikelihood(eng, index, D, Ci, g["auto_loc"], g["auto_scale"])
    pairs, pc = ([0, 1], [1, 0]), [2, 2]
    off = _offsets(pc)
    with pytest.raises(L.EftbError, match="eftb_draws_drag_params: no draw recipe"):
        like.drag_draws_params(theta, off, f, pairs, step, lnu)
    like.set_draw_recipe(rec)
    chain_before = like.metropolis_draws_params(theta, [0, 2, 4, 4], f, step, lnu)
    draws_before = like.logp_draws_params(theta, [0, 2, 4, 4], f)
    want = like.drag_draws_params(theta, off, f, pairs, step, lnu, thin=1)
    for bad, msg in ((([0, 3], [1, 0]), "wstart\\[1\\] = 3 outside \\[0, 3\\)"), (([0, 1], [-1, 0]), "wend\\[0\\] = -1 outside \\[0, 3\\).*pair 0")):
        with pytest.raises(L.EftbError, match=msg):
            like.drag_draws_params(theta, off, f, bad, step, lnu)
    for v in (np.nan, -1e-3, 1.0 + 1e-9):
        fr = drag_fractions(Tn)
        fr[4] = v
        with pytest.raises(L.EftbError, match="frac\\[4\\] = .* outside \\[0, 1\\]"):
            like.drag_draws_params(theta, off, f, pairs, step, lnu, frac=fr)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    i64, i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    th, fo, fr = np.ascontiguousarray(theta), np.ascontiguousarray(f), drag_fractions(Tn)
    wa, wb = np.array(pairs[0], dtype=np.int32), np.array(pairs[1], dtype=np.int32)
    out = [np.zeros((N, Tn, P))] + [np.zeros((N, Tn + 1)) for _ in range(4)] + [np.zeros((N, Tn + 1, nG)) for _ in range(2)] + [np.zeros((N, P))]
    nacc, sums = np.zeros(N, dtype=np.int64), np.zeros((N, 2))

    def call(Tc, thin):
        rc = eng.lib.eftb_draws_drag_params(eng._h, 3, 2, i32(wa), i32(wb), N, Tc, thin, i64(off), dp(th), dp(fo), dp(fr), dp(step), dp(lnu), None, None, None, None,
                                            *[dp(a) for a in out], i64(nacc), dp(sums))
        return rc, eng.lib.eftb_last_error().decode()

    for Tc, thin, msg in ((0, 1, "T = 0 steps"), (Tn, -1, "thin = -1 outside [0, T = 9]"), (Tn, Tn + 1, "thin = 10 outside [0, T = 9]")):
        rc, err = call(Tc, thin)
        assert rc != 0 and msg in err, err
    assert call(Tn, 1)[0] == 0 and np.array_equal(out[0], want.theta) and np.array_equal(out[1][:, :Tn], want.logp_start) and np.array_equal(out[2][:, Tn], want.last_logp_end)
    assert np.array_equal(nacc, want.naccept) and np.array_equal(sums[:, 1], want.sum_end)
    bad = step.copy()
    bad[2, 5, 1] = np.inf
    with pytest.raises(L.EftbError, match="eftb_draws_drag_params: step\\[2\\]\\[5\\]\\[1\\] is not finite"):
        like.drag_draws_params(theta, off, f, pairs, bad, lnu)
    bad = lnu.copy()
    bad[3, 4] = 1e-3
    with pytest.raises(L.EftbError, match="lnu\\[3\\]\\[4\\]"):
        like.drag_draws_params(theta, off, f, pairs, step, bad)
    lo, hi = theta.min(0) - 1.0, theta.max(0) + 1.0
    with pytest.raises(L.EftbError, match="lower\\[1\\] = .* > upper\\[1\\]"):
        like.drag_draws_params(theta, off, f, pairs, step, lnu, lower=[lo[0], hi[1], lo[2]], upper=[hi[0], lo[1], hi[2]])
    with pytest.raises(L.EftbError, match="prior_scale\\[0\\]"):
        like.drag_draws_params(theta, off, f, pairs, step, lnu, prior_scale=[0.0, 1.0, 1.0])
    j = int(np.argmin(theta[:, 1]))
    with pytest.raises(L.EftbError, match="theta0\\[%d\\]\\[1\\] = .* outside" % j):
        like.drag_draws_params(theta, off, f, pairs, step, lnu, lower=[lo[0], np.nextafter(theta[j, 1], np.inf), lo[2]])
    with pytest.raises(L.EftbError, match="offsets\\[2\\] = 5, not the 4 draws"):
        like.drag_draws_params(theta, [0, 2, 5], f, pairs, step, lnu)
    with pytest.raises(L.EftbError, match="offsets decrease at pair 1"):
        like.drag_draws_params(theta, [0, 3, 2], f, pairs, step, lnu)
    again = like.drag_draws_params(theta, off, f, pairs, step, lnu, thin=1)
    for k in FIELDS[:3] + FIELDS[7:11] + FIELDS[15:]:
        assert np.array_equal(getattr(again, k), getattr(want, k)), k
    for a, b in zip(chain_before[:4], like.metropolis_draws_params(theta, [0, 2, 4, 4], f, step, lnu)[:4]):
        assert np.array_equal(a, b)
    assert np.array_equal(draws_before, like.logp_draws_params(theta, [0, 2, 4, 4], f))
    eng.close()


# ----------------------------------------------------------------------------- the workgroup shapes of the drag layout, on synthetic likelihoods
def drag_lds_bytes(J1, nG, nnz, nw):
    """DrawLds::drag(...).bytes(nw) on the host: per workgroup two Gram matrices, two tables of powers of f [8][7], col (two ints to a double)
    and the prior table [4][32]; per wave th [34], val, H, G, the two theta [32] and four records [26]"""
    nnzp, ng1 = (nnz + 1) & ~1, nG + 1
    wg = 2 * J1 * J1 + 2 * 8 * 7 + nnzp // 2 + 4 * 32
    wave = 34 + nnzp + ng1 * J1 + ng1 * ng1 + 2 * 32 + 4 * 26
    return 8 * (wg + nw * wave)


def drag_lds_waves(J1, nG, nnz, limit=160 * 1024):
    """DrawLds::fit: waves per workgroup, 0: refused"""
    return next((nw for nw in (4, 2, 1) if drag_lds_bytes(J1, nG, nnz, nw) <= limit), 0)


# this copy is held to the figures that the library's static_assert pins on DrawLds::drag at every build
assert drag_lds_bytes(82, 24, 1024, 1) == 144808 and drag_lds_waves(82, 24, 1024) == 1 and drag_lds_waves(97, 24, 0) == 0


# the waves per workgroup are computed from the layout and asserted; W: case F at nG = 5 (TWO at four waves), F: case F (3 tracers, nG = 23),
# N: three tracers with NNLO at nG = 24 and a recipe of 600 entries, G: case G (4 tracers, nG = 24)
DRAG_SHAPES = {
    "W": (dict(ntr=3, nnlo=False, nG=5, nl=3, nx=5, ndata=33, P=5), None, 4),
    "F": (SY.shape_of("F"), None, 2),
    "N": (dict(ntr=3, nnlo=True, nG=24, nl=3, nx=5, ndata=33, P=5), 600, 1),
    "G": (SY.shape_of("G"), None, 0),
}


def _synthetic(name):
    from test_gpu_draw_synthetic import _engine as synth_engine
    from test_gpu_draw_synthetic import _like as synth_like
    from test_gpu_draw_synthetic import _padded_recipe, _put

    shape, entries, nw = DRAG_SHAPES[name]
    pb = SY.problem(seed=2000 + sorted(DRAG_SHAPES).index(name), **shape)
    rec = pb.rec if entries is None else _padded_recipe(pb.rec, entries)
    nnz = len(set(zip(rec.tracer.tolist(), rec.row.tolist(), rec.col.tolist())))
    J1 = (27 if pb.nnlo else 24) * pb.ntr + 1
    assert drag_lds_waves(J1, pb.nG, nnz) == nw, (J1, pb.nG, nnz)
    eng = synth_engine(pb, len(pb.counts) * pb.ntr)
    _put(eng, pb)
    return pb, eng, synth_like(eng, pb, False, rec=rec), J1


@pytest.mark.parametrize("name", ["W", "F", "N"])
def test_workgroup_shapes(name):
    """four, two and one waves per workgroup of the drag layout (J + 1 = 73 at nG = 5 and 23: TWO; J + 1 = 82 at nG = 24 with 600 recipe
    entries): T = 6 steps of 9 + 5 chains on two pairs of different walkers, one pair without a chain, bitwise against the host loop"""
    pb, eng, like, J1 = _synthetic(name)
    N, P = pb.theta.shape
    rng = np.random.default_rng(61)
    inp = dict(theta0=pb.theta, step=0.02 * rng.standard_normal((N, 6, P)), lnu=np.log(rng.uniform(size=(N, 6))))
    assert pb.counts == [9, 0, 5]
    got, want = _compare(like, pb.f, ([0, 1, 2], [2, 1, 0]), [9, 0, 5], inp, 1, prior_loc=np.ones(P), prior_scale=np.full(P, 0.5))
    print(name, "J1", J1, "naccept", got.naccept, "decided otherwise", want["differ"])
    assert np.all(np.isfinite(got.logp_end)) and np.any(got.naccept > 0) and np.any(got.naccept < 6)
    _stored_records_are_the_draw_call(like, pb.f, 3, np.repeat([0, 2], [9, 5]), np.repeat([2, 0], [9, 5]), got)
    eng.close()


def test_four_tracers_at_nG_24_are_refused():
    """case G's shape: two Gram matrices of 97 columns leave no room for a wave.  The call refuses before anything is copied, by a message that
    names J + 1 and nG and says that it stages two Gram matrices; metropolis_draws_params still runs at that shape afterwards"""
    from eftpipe_amd import _lib as L

    pb, eng, like, J1 = _synthetic("G")
    N, P = pb.theta.shape
    step, lnu = np.zeros((N, 2, P)), np.full((N, 2), -1.0)
    before = like.metropolis_draws_params(pb.theta, SY.offsets(pb.counts), pb.f, step, lnu)
    with pytest.raises(L.EftbError, match="eftb_draws_drag_params: the call stages two Gram matrices of J \\+ 1 = 97 columns per workgroup; with nG = 24 they do not fit the LDS"):
        like.drag_draws_params(pb.theta, [0, 9, 9, 14], pb.f, ([0, 1, 2], [2, 1, 0]), step, lnu)
    after = like.metropolis_draws_params(pb.theta, SY.offsets(pb.counts), pb.f, step, lnu)
    assert np.all(np.isfinite(after.logp)) and all(np.array_equal(a, b) for a, b in zip(before[:4], after[:4]))
    eng.close()
