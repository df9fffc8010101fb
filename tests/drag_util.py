"""The dragging chains of eftb_draws_drag_params restated in NumPy, beside chain_util.py; shared by the CPU tests (test_draw_drag.py) and
the GPU tests (test_gpu_draw_drag.py).

host_drag    the algorithm of the device call, vectorised over the chains with a loop over the steps, around any two ln P: per step
             theta' = theta + step, a proposal outside the box rejected without an evaluation, otherwise with u = 1 - frac[t]
                 a1 = la1 + pri1, b1 = lb1 + pri1, a0 = la0 + pri0, b0 = lb0 + pri0, w1 = u a1 + frac[t] b1, w0 = u a0 + frac[t] b0,
                 accepted iff la1 and lb1 are finite and lnu < w1 - w0,
             then sa = sa + (la0 + pri0), sb = sb + (lb0 + pri0) with the current values; the sums start at the starting state's terms.
             pri is chain_util.prior_term.  NumPy rounds every operation on its own, as the kernel does, so fed with the device's ln P the
             chains and the sums are the device's bit for bit.
drag_case    the inputs of the device tests: a case of test_draw_chains.chain_case with every walker doubled by an end walker (templates
             scaled, another growth rate) and its chains dealt to pairs of walkers."""
import numpy as np

import chain_util as CU

T37 = 37
# templates of the end walkers over those of their start walkers, even and odd rows: scaled until the end walker changes decisions on every pair
# (test_draw_drag.py).  auto walks around its best fits, where one per cent is enough; the other two walk where ln P changes by hundreds
# per step and only a landscape of another shape turns a decision
END_SCALE = dict(auto=(1.01, 1.01), full=(0.3, 0.3), nnlo=(2.0, 0.5))
END_F = 1.05  # and their growth rates


def end_templates(tag, templ):
    """the end walkers' templates [.., rows, nx] from the start walkers': the even rows times END_SCALE[tag][0], the odd ones times [1]"""
    even, odd = END_SCALE[tag]
    return templ * np.where(np.arange(templ.shape[-2]) % 2 == 0, even, odd)[:, None]


def host_drag(logp_start_fun, logp_end_fun, theta0, step, lnu, frac, thin=0, lower=None, upper=None, loc=None, scale=None):
    """logp_x_fun(theta [N, P]) -> ln P [N] at the chains' start (end) walkers, or a tuple (ln P [N], extra [N, ...], ...) whose extras are
    carried with the state.  Each is called once for the start and once per step with all N chains; a chain whose proposal lies outside
    the box (or that has failed) is passed its current (starting) theta instead and the value is not used: neither is ever asked for a point
    outside the box.
    -> dict(theta [N, K, P], logp_start, logp_end [N, K], extras_start, extras_end (lists of [N, K, ...]), last [N, P], naccept [N],
    last_logp_start, last_logp_end [N], last_extras_start, last_extras_end, sum_start, sum_end [N], outside [N] (proposals refused for
    the box), differ [N] (steps at which the rule of the start target alone, lnu < a1 - a0, decides otherwise)) with K = T // thin, 0 for
    thin = 0.  A chain whose starting ln P is not finite at either walker has failed: NaN everywhere, naccept -1."""
    theta0 = np.array(theta0, dtype=np.float64)
    step, lnu, frac = (np.asarray(a, dtype=np.float64) for a in (step, lnu, frac))
    N, P = theta0.shape
    T = step.shape[1]
    assert step.shape == (N, T, P) and lnu.shape == (N, T) and frac.shape == (T,) and 0 <= thin <= T
    lower, upper, loc, sinv = CU.prior_arrays(P, lower, upper, loc, scale)
    split = lambda r: (np.array(r[0], dtype=np.float64), [np.array(x, dtype=np.float64) for x in r[1:]]) if isinstance(r, tuple) else (np.array(r, dtype=np.float64), [])
    cur = theta0.copy()
    la, exa = split(logp_start_fun(cur.copy()))
    lb, exb = split(logp_end_fun(cur.copy()))
    pri = CU.prior_term(cur, loc, sinv)
    failed = ~(np.isfinite(la) & np.isfinite(lb))
    K = T // thin if thin else 0
    out_t, out_a, out_b = np.empty((N, K, P)), np.empty((N, K)), np.empty((N, K))
    out_ea, out_eb = [np.empty((N, K) + x.shape[1:]) for x in exa], [np.empty((N, K) + x.shape[1:]) for x in exb]
    nacc, outside, differ = (np.zeros(N, dtype=np.int64) for _ in range(3))
    with np.errstate(invalid="ignore"):
        sa, sb = la + pri, lb + pri
    for t in range(T):
        trial = cur + step[:, t]
        inbox = np.all((trial >= lower) & (trial <= upper), axis=1) & ~failed
        outside += ~inbox & ~failed
        ask = np.where(inbox[:, None], trial, np.where(failed[:, None], theta0, cur))
        la1, exa1 = split(logp_start_fun(ask))
        lb1, exb1 = split(logp_end_fun(ask))
        pri1 = CU.prior_term(ask, loc, sinv)
        lam = frac[t]
        with np.errstate(invalid="ignore"):
            u = 1.0 - lam
            a1, b1, a0, b0 = la1 + pri1, lb1 + pri1, la + pri, lb + pri
            w1, w0 = u * a1 + lam * b1, u * a0 + lam * b0
            acc = inbox & np.isfinite(la1) & np.isfinite(lb1) & (lnu[:, t] < w1 - w0)
            differ += (inbox & np.isfinite(la1) & (lnu[:, t] < a1 - a0)) != acc
        cur[acc], la[acc], lb[acc], pri[acc] = trial[acc], la1[acc], lb1[acc], pri1[acc]
        for xs, x1s in ((exa, exa1), (exb, exb1)):
            for x, x1 in zip(xs, x1s):
                x[acc] = x1[acc]
        nacc += acc
        with np.errstate(invalid="ignore"):
            sa = sa + (la + pri)
            sb = sb + (lb + pri)
        if thin and (t + 1) % thin == 0:
            k = (t + 1) // thin - 1
            out_t[:, k], out_a[:, k], out_b[:, k] = cur, la, lb
            for os, xs in ((out_ea, exa), (out_eb, exb)):
                for o, x in zip(os, xs):
                    o[:, k] = x
    last = cur.copy()
    for a in [out_t, out_a, out_b, last, la, lb, sa, sb] + out_ea + out_eb + exa + exb:
        a[failed] = np.nan
    nacc[failed] = -1
    return dict(theta=out_t, logp_start=out_a, logp_end=out_b, extras_start=out_ea, extras_end=out_eb, last=last, naccept=nacc, last_logp_start=la,
                last_logp_end=lb, last_extras_start=exa, last_extras_end=exb, sum_start=sa, sum_end=sb, outside=outside, differ=differ)


# ----------------------------------------------------------------------------- the inputs of the device tests
def drag_case(tag):
    """test_draw_chains.chain_case(tag) for dragging: the C walkers of that case are the start walkers, walker C + c is the end walker of
    walker c -- its templates times END_SCALE[tag], its growth rates times END_F -- and the chains keep their order, theta0, step and lnu
    (T = 37).  The chains of walker c go to the pair (c, C + c); the last chain of the first walker with two chains goes to the pair (c, c)
    instead, followed by a pair (C + c, c) without a chain.
    -> the case with templ, templn, fw, f and Ws for the 2 C walkers, and wstart, wend [G], pcounts [G], pair [N], a [N], b [N] (the pair
    and the two walkers of every chain)."""
    import grad_util as GU
    from test_draw_chains import chain_case

    case = dict(chain_case(tag))
    counts, ntr = list(case["counts"]), case["ntr"]
    C = len(counts)
    case["templ"] = np.concatenate([case["templ"], end_templates(tag, case["templ"])])
    if case["templn"] is not None:
        case["templn"] = np.concatenate([case["templn"], end_templates(tag, case["templn"])])
    case["fw"] = np.concatenate([case["fw"], END_F * case["fw"]])
    case["f"] = case["fw"] if ntr > 1 else case["fw"][:, 0]
    tn = case["templn"]
    case["Ws"] = list(case["Ws"]) + [GU.gram_matrix(case["templ"][c * ntr : (c + 1) * ntr], case["index"], case["D"], case["Ci"], None if tn is None else tn[c * ntr : (c + 1) * ntr])
                                     for c in range(C, 2 * C)]
    first = next(c for c in range(C) if counts[c] >= 2)
    wstart, wend, pcounts = [], [], []
    for c in range(C):
        if counts[c] == 0:
            continue
        own = counts[c] - (c == first)
        wstart, wend, pcounts = wstart + [c], wend + [C + c], pcounts + [own]
        if c == first:
            wstart, wend, pcounts = wstart + [c, C + c], wend + [c, c], pcounts + [1, 0]
    case["wstart"], case["wend"], case["pcounts"] = np.array(wstart), np.array(wend), np.array(pcounts)
    case["pair"] = np.repeat(np.arange(len(pcounts)), pcounts)
    case["a"], case["b"] = case["wstart"][case["pair"]], case["wend"][case["pair"]]
    assert np.array_equal(case["a"], case["walker"]) and case["inp"]["step"].shape[1] == T37
    return case


def host_targets(case, i, sel=slice(None)):
    """the start and the end target of prior i of a drag case on the host (the Gram route in NumPy), for the chains sel"""
    return tuple(CU.HostTarget(case["rec"], case["fw"][w[sel]], [case["Ws"][c] for c in w[sel]], *case["priors"][i]) for w in (case["a"], case["b"]))


def moves(r, case, T):
    """the condition on the inputs: every chain moved, was refused and met the box, and every pair of two different walkers met a step that
    the start target alone would have decided otherwise"""
    two = np.flatnonzero((case["wstart"] != case["wend"]) & (case["pcounts"] > 0))
    felt = [np.sum(r["differ"][case["pair"] == g]) > 0 for g in two]
    return bool(np.all(r["naccept"] > 0) and np.all(r["naccept"] < T) and np.all(r["outside"] > 0) and len(two) >= 2 and all(felt))
