"""The parallel tempering of eftb_draws_temper_params restated in NumPy, beside chain_util.py; shared by the CPU tests (test_draw_temper.py)
and the GPU tests (test_gpu_draw_temper.py).

host_ladder   the algorithm of the device call, vectorised over the chains, around any ln P.  Chain n is rung n % R of ladder n // R and
              targets beta_r ln P + pri (chain_util.prior_term: not tempered).  Step i is global step g = first_step + i: the step of
              chain_util.host_chain with lnu < (beta_r ln P' + pri') - (beta_r ln P + pri); then, if (g + 1) % S == 0, event
              j = (g + 1) // S - 1 tries the pairs (r, r + 1), r = j mod 2: x = (beta_r - beta_{r+1}) (ln P_{r+1} - ln P_r), accepted iff
              lnu_swap[ladder, j - first_step // S, r] < x, and the two rungs exchange theta, ln P, the extras and pri; then
              sum_logp = sum_logp + ln P and the store after every thin-th step of the call.  NumPy rounds every operation on its own, as
              the kernel does, so fed with the device's ln P the ladders are the device's bit for bit.
ladder_case   the inputs of the device tests from a case of test_draw_chains.chain_case: ladders of R = 4 on walkers that carry 0, 1 and 3
              of them, starts and diagonal proposals from the case's own chains, its box.
lds_waves     the rungs that fit one workgroup's LDS, from the documented layout."""
import numpy as np

import chain_util as CU


def host_ladder(logp_fun, theta0, beta, step, lnu, lnu_swap=None, swap_every=0, first_step=0, thin=1, lower=None, upper=None, loc=None, scale=None):
    """logp_fun as chain_util.host_chain's (ln P [N], or a tuple with extras that are carried -- and swapped -- with the state).
    -> dict(theta [N, K, P], logp [N, K], extras, naccept [N], last [N, P], nswap [nlad, max(R - 1, 1)], sum_logp [N], outside [nlad]
    (proposals refused for the box, per ladder), tried [nlad, max(R - 1, 1)] (swaps tried per pair)).  A ladder one of whose rungs starts
    without a finite ln P has failed: NaN everywhere, naccept = nswap = -1."""
    theta0 = np.array(theta0, dtype=np.float64)
    beta = np.asarray(beta, dtype=np.float64)
    step, lnu = np.asarray(step, dtype=np.float64), np.asarray(lnu, dtype=np.float64)
    (N, P), R, T, S = theta0.shape, beta.size, step.shape[1], int(swap_every)
    assert N % R == 0 and step.shape == (N, T, P) and lnu.shape == (N, T) and 1 <= thin <= T and S >= 0 and first_step >= 0
    nlad, npair = N // R, max(R - 1, 1)
    nsw = (first_step + T) // S - first_step // S if S else 0
    if nsw and R > 1:
        lnu_swap = np.asarray(lnu_swap, dtype=np.float64)
        assert lnu_swap.shape == (nlad, nsw, R - 1)
    lower, upper, loc, sinv = CU.prior_arrays(P, lower, upper, loc, scale)
    split = lambda r: (np.asarray(r[0], dtype=np.float64), [np.asarray(x, dtype=np.float64) for x in r[1:]]) if isinstance(r, tuple) else (np.asarray(r, dtype=np.float64), [])
    bt = np.tile(beta, nlad)
    cur = theta0.copy()
    lp, ex = split(logp_fun(cur.copy()))
    lp, ex = lp.copy(), [x.copy() for x in ex]
    pri = CU.prior_term(cur, loc, sinv)
    lad_failed = np.any(~np.isfinite(lp).reshape(nlad, R), axis=1)
    failed = np.repeat(lad_failed, R)
    K = T // thin
    out_t, out_l = np.empty((N, K, P)), np.empty((N, K))
    out_e = [np.empty((N, K) + x.shape[1:]) for x in ex]
    nacc, outside, sums = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64), np.zeros(N)
    nswap, tried = np.zeros((nlad, npair), dtype=np.int64), np.zeros((nlad, npair), dtype=np.int64)
    base = np.arange(nlad) * R
    for t in range(T):
        trial = cur + step[:, t]
        inbox = np.all((trial >= lower) & (trial <= upper), axis=1) & ~failed
        outside += ~inbox & ~failed
        ask = np.where(inbox[:, None], trial, np.where(failed[:, None], theta0, cur))
        lp1, ex1 = split(logp_fun(ask))
        pri1 = CU.prior_term(ask, loc, sinv)
        with np.errstate(invalid="ignore"):
            acc = inbox & np.isfinite(lp1) & (lnu[:, t] < (bt * lp1 + pri1) - (bt * lp + pri))
        cur[acc], lp[acc], pri[acc] = trial[acc], lp1[acc], pri1[acc]
        for x, x1 in zip(ex, ex1):
            x[acc] = x1[acc]
        nacc += acc
        g = first_step + t
        if S and (g + 1) % S == 0:
            j = (g + 1) // S - 1
            for r in range(j % 2, R - 1, 2):
                lo, hi = base + r, base + r + 1
                with np.errstate(invalid="ignore"):
                    x = (beta[r] - beta[r + 1]) * (lp[hi] - lp[lo])
                    sw = (lnu_swap[:, j - first_step // S, r] < x) & ~lad_failed
                a, b = lo[sw], hi[sw]
                for arr in [cur, lp, pri] + ex:
                    arr[a], arr[b] = arr[b].copy(), arr[a].copy()
                nswap[:, r] += sw
                tried[:, r] += ~lad_failed
        sums = sums + lp
        if (t + 1) % thin == 0:
            k = (t + 1) // thin - 1
            out_t[:, k], out_l[:, k] = cur, lp
            for o, x in zip(out_e, ex):
                o[:, k] = x
    last = cur.copy()
    for a in [out_t, out_l, last, sums] + out_e:
        a[failed] = np.nan
    nacc[failed] = -1
    nswap[lad_failed] = -1
    return dict(theta=out_t, logp=out_l, extras=out_e, naccept=nacc, last=last, nswap=nswap, sum_logp=sums, outside=outside.reshape(nlad, R).sum(1),
                tried=tried)


# ----------------------------------------------------------------------------- the inputs of the device tests
R4, T_LADDER, THIN, S_LADDER = 4, 37, 5, 3
LADDERS = dict(auto=[3, 0, 1, 1], cross=[3, 0, 1, 1], full=[1, 0, 1, 3], nnlo=[1, 0, 3])  # per walker: none, one, and enough for a loop
# (T, seed) per case.  At T = 37 every pair is tried six times, and marg.npz auto and cross did not both accept and refuse a swap on every
# pair of every ladder under every prior with any ladder or seed tried: they run 64 steps.  Checked by test_draw_temper.py on the host.
TUNING = dict(auto=(64, 13), cross=(64, 11), full=(T_LADDER, 11), nnlo=(T_LADDER, 11))
BETA_MIN, SCALE = 0.1, 0.5  # the ladders reach beta = 0.1; the proposals have half the dispersion of the chain tests' increments


def ladder_inputs(case, ladders, R, T, beta, seed, S=S_LADDER, first_step=0, scale=SCALE):
    """Ladders on the walkers of a chain_case: every rung starts half a proposal step off the mean start of the case's chains on its walker
    (a walker without chains there carries no ladder here either); the proposals are diagonal with the per-parameter dispersion of the
    case's own increments, widened by 1 / sqrt(beta_r); the box is the case's.
    -> dict(theta0 [N, P], step [N, T, P], lnu [N, T], lnu_swap, lower, upper, beta, counts (chains per walker), walker [N])"""
    from eftpipe_amd.marginal import temper_proposals

    inp, w0 = case["inp"], case["walker"]
    sd = scale * inp["step"].std(axis=(0, 1))
    counts = [R * n for n in ladders]
    walker = np.repeat(np.arange(len(counts)), counts)
    assert all(n == 0 or np.any(w0 == c) for c, n in enumerate(ladders))
    center = np.stack([inp["theta0"][w0 == c].mean(0) for c in walker])
    rng = np.random.default_rng(seed)
    theta0 = np.clip(center + 0.5 * sd * rng.standard_normal(center.shape), inp["lower"], inp["upper"])
    step, lnu, lnu_swap = temper_proposals(rng, len(walker) // R, beta, T, np.diag(sd), S, first_step)
    return dict(theta0=theta0, step=step, lnu=lnu, lnu_swap=lnu_swap, lower=inp["lower"], upper=inp["upper"], beta=np.asarray(beta), counts=counts,
                walker=walker)


def ladder_case(tag):
    """-> (case of test_draw_chains.chain_case, ladder_inputs for it at the case's T and beta_min)"""
    from test_draw_chains import chain_case

    from eftpipe_amd.marginal import temper_ladder

    case = chain_case(tag)
    T, seed = TUNING[tag]
    return case, ladder_inputs(case, LADDERS[tag], R4, T, temper_ladder(R4, BETA_MIN), seed)


def long_ladder():
    """the T = 300 call of the GPU tests (auto, one ladder on each of two walkers, to be run with S = 4): it crosses the launch boundary at 256
    steps with swap event 63 on step 255, the first launch's last"""
    from test_draw_chains import chain_case

    from eftpipe_amd.marginal import temper_ladder

    case = chain_case("auto")
    return case, ladder_inputs(case, [1, 0, 0, 1], R4, 300, temper_ladder(R4, BETA_MIN), 17, S=4)


def other_length(case, R):
    """the ladders of the GPU tests at R = 1, 2, 3 and 8 (auto, T = 37, S = 3)"""
    from eftpipe_amd.marginal import temper_ladder

    return ladder_inputs(case, [1, 0, 0, 1] if R == 8 else [2, 0, 1, 1], R, T_LADDER, temper_ladder(R, 0.1 if R > 2 else 0.3), 20 + R)


def other_length_moves(r, R):
    """at the other lengths: every ladder has a rung that moved and met the box, and every pair swapped somewhere"""
    return bool(np.all(r["naccept"].reshape(-1, R).sum(1) > 0) and np.all(r["outside"] > 0) and (np.all(r["nswap"] == 0) if R == 1 else np.all(r["nswap"].sum(0) > 0)))


def lds_waves(J1, nG, nnz, limit=160 * 1024):
    """the rungs of a ladder that fit one workgroup, from the layout the header of the library documents: per workgroup W_c [J1][J1], the
    powers of f [8][7], col (two ints to a double) and the prior table [4][32]; per wave th [34], val, H [nG + 1][J1], G [nG + 1][nG + 1],
    two theta of 32 and two records of 26; then 40 doubles for the exchange.  At most 8."""
    nnzp = (nnz + 1) // 2 * 2
    wg, wave = J1 * J1 + 56 + nnzp // 2 + 128, 34 + nnzp + (nG + 1) * J1 + (nG + 1) ** 2 + 116
    return int(min(8, (limit - 8 * (wg + 40)) // (8 * wave)))


def ladder_target(case, lin, i):
    """the target of prior i of a case for the chains of ladder_inputs, on the host (the Gram route in NumPy)"""
    w = lin["walker"]
    return CU.HostTarget(case["rec"], case["fw"][w], [case["Ws"][c] for c in w], *case["priors"][i])


def mixed(r, T):
    """every rung moved and was refused, every adjacent pair of every ladder swapped and refused a swap, every ladder met the box"""
    return bool(np.all(r["naccept"] > 0) and np.all(r["naccept"] < T) and np.all(r["nswap"] > 0) and np.all(r["nswap"] < r["tried"])
                and np.all(r["outside"] > 0))
