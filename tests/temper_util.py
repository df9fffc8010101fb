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
lds_waves     the rungs that fit one workgroup's LDS, from the documented layout.
TEMPER_RUNGS  lds_waves at every case of synth_like_util.CASES (test_draw_temper.py pins the table); synthetic_ladder, SyntheticTarget and
              mixed_in_sum are the inputs, the host target and the mixing condition of the ladders on those likelihoods."""
import numpy as np

import chain_util as CU
import grad_util as GU
import sample_util as SU
import synth_like_util as SY


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


# ----------------------------------------------------------------------------- ladders on the synthetic likelihoods
# The rungs that fit one workgroup at each case of synth_like_util.CASES: lds_waves on the case's own recipe, and on the recipe padded to its
# 1024 entries (test_gpu_draw_synthetic._padded_recipe).  Pinned by test_draw_temper.py::test_rung_table; the library's refusal names the
# same numbers (test_gpu_draw_temper.py::test_rungs_at_the_lds_limit).  The padded column is lds_waves at 1024 entries, whether or not a
# recipe of the case can hold them: an entry is a distinct (tracer, row, column), so one tracer has at most 25 x 27 = 675 (cases E, Ef: eight
# rungs at every recipe there is; the 7 is the formula's alone), and the padded recipe the device meets is case F's (four rungs).
TEMPER_RUNGS = dict(A=8, B=8, C=8, D=8, E=8, F=5, G=3, H=3, I=1, J=3, Gf=3, Ef=8)
TEMPER_RUNGS_PADDED = dict(A=8, B=8, C=8, D=8, E=7, F=4, G=2, H=2, I=1, J=2, Gf=2, Ef=7)
PADDED = 1024
# the rungs of the GPU tests' ladders per case: all eight at the smallest shape and at nG = 24, the most that fit where the LDS limits them,
# four elsewhere
SYNTH_R = dict(A=8, B=4, C=4, D=4, E=8, F=5, G=3, H=3, J=3, I=1)
SYNTH_LADDERS = [2, 0, 1]  # per walker: two, none, one
SYNTH_S, SYNTH_THIN = 3, 5
PRIOR_LOC, PRIOR_SCALE = 1.0, 0.5  # the Gaussian theta priors of test_gpu_draw_hmc.test_synthetic_shapes


def case_shape(case, rec=None):
    """J + 1, nG and the recipe's entries (distinct (tracer, row, column)) of a synthetic case: the arguments of lds_waves"""
    pb = SY.case_problem(case)
    rec = pb.rec if rec is None else rec
    return (27 if pb.nnlo else 24) * pb.ntr + 1, pb.nG, len(set(zip(rec.tracer.tolist(), rec.row.tolist(), rec.col.tolist())))


def theta_prior(P):
    return dict(prior_loc=np.full(P, PRIOR_LOC), prior_scale=np.full(P, PRIOR_SCALE))


def synthetic_ladder(case, R, ladders, T, S, seed, scale, beta_min, first_step=0, kind="gauss", singular=None, box=1.0):
    """Ladders of R rungs on the walkers of synth_like_util.case_problem(case, kind, singular): chain i of a walker starts half a proposal step
    off row i (mod the walker's rows) of the case's own theta; the proposals are isotropic with dispersion `scale`, widened by
    1 / sqrt(beta_r) (temper_proposals); the box reaches `box` proposal steps beyond the outermost starts, so that every wall has a chain one
    step away.  -> what ladder_inputs returns"""
    from eftpipe_amd.marginal import temper_ladder, temper_proposals

    pb = SY.case_problem(case, kind, singular)
    counts = [R * n for n in ladders]
    walker = np.repeat(np.arange(len(counts)), counts)
    assert len(counts) == len(pb.counts) and all(n == 0 or m > 0 for n, m in zip(counts, pb.counts))
    rows = [pb.theta[pb.walker == w] for w in range(len(counts))]
    base = np.stack([rows[w][i % len(rows[w])] for w, n in enumerate(counts) for i in range(n)])
    beta = temper_ladder(R, beta_min)
    sd = np.full(pb.P, float(scale))
    rng = np.random.default_rng(seed)
    theta0 = base + 0.5 * sd * rng.standard_normal(base.shape)
    step, lnu, lnu_swap = temper_proposals(rng, len(walker) // R, beta, T, np.diag(sd), S, first_step)
    return dict(theta0=theta0, step=step, lnu=lnu, lnu_swap=lnu_swap, lower=theta0.min(0) - box * sd, upper=theta0.max(0) + box * sd, beta=beta, counts=counts,
                walker=walker)


# (proposal dispersion, beta_min, T, seed) per ladder of the GPU tests.  ln P of the synthetic likelihoods changes by 1e2 to 1e3 between two
# of a case's own theta rows, and by another amount at every case, so every case has its own dispersion; tuned on the host
# (test_draw_temper.py::test_synthetic_inputs_mix) until mixed_in_sum held without and with Jeffreys with every count it asks for at seven
# or more (the device's ln P differs from the host's in rounding, and a ladder can then take another path).  F/1024 is case F under the
# recipe padded to 1024 entries at its four rungs; G/long the ladders across the launch boundary.  Gf is the case of the three-wave tests:
# its entry, run at [2, 0, 1] ladders and T = 60, shows the tuning only; the device runs Gf at T = 4, S = 2 with hundreds of ladders, which
# test_draw_temper.py::test_three_wave_inputs_mix checks at 61 and 301 ladders on the host.
SYNTH_TUNING = {
    "A": (0.003, 0.02, 60, 1), "B": (0.03, 0.1, 60, 1), "C": (0.1, 0.02, 60, 1), "D": (0.03, 0.1, 60, 1), "E": (0.005, 0.2, 60, 3), "F": (0.1, 0.1, 60, 1),
    "G": (0.01, 0.1, 60, 1), "H": (0.01, 0.02, 60, 2), "J": (0.03, 0.1, 60, 2), "I": (0.01, 0.5, 60, 2), "F/1024": (0.01, 0.1, 60, 2), "Gf": (0.03, 0.02, 60, 1),
    "G/long": (0.01, 0.1, 260, 5),
}
LONG_LADDERS, LONG_S, LONG_THIN = [1, 0, 1], 3, 7  # G/long: one ladder on each of two walkers across the launch boundary at 256 steps


def synthetic_inputs(name, ladders=SYNTH_LADDERS, T=None, S=SYNTH_S, first_step=0, R=None, **kw):
    """synthetic_ladder at an entry of SYNTH_TUNING -> (case, lin)"""
    scale, beta_min, T0, seed = SYNTH_TUNING[name]
    case = name.split("/")[0]
    if R is None:
        R = TEMPER_RUNGS_PADDED[case] if name.endswith("/1024") else SYNTH_R.get(case, TEMPER_RUNGS[case])
    return case, synthetic_ladder(case, R, ladders, T0 if T is None else T, S, seed, scale, beta_min, first_step, **kw)


GROUPS = [(2, 1), (0, 0), (0, 1), (2, 0)]  # (walker, data set) per group: both walkers twice, data set 1 first


def groups_inputs(case="C"):
    """The ladders of the groups test at two data sets: the groups on data set 0 own the ladders of synthetic_inputs(case) (two on walker 0,
    one on walker 2), those on data set 1 one ladder each from another seed; one box holds both.
    -> (lin of the whole call in group order, counts per group, lin of the call without groups, own: the chains of the whole call that the
    call without groups repeats, in its order)"""
    scale, beta_min, T, seed = SYNTH_TUNING[case]
    _, plain = synthetic_inputs(case)
    other = synthetic_ladder(case, SYNTH_R[case], [1, 0, 1], T, SYNTH_S, seed + 100, scale, beta_min)
    R = SYNTH_R[case]
    box = dict(lower=np.minimum(plain["lower"], other["lower"]), upper=np.maximum(plain["upper"], other["upper"]))
    part = {(0, 0): (plain, np.arange(0, 2 * R)), (2, 0): (plain, np.arange(2 * R, 3 * R)), (0, 1): (other, np.arange(0, R)), (2, 1): (other, np.arange(R, 2 * R))}
    take = lambda lin, sel, k: lin[k][sel[::R] // R] if k == "lnu_swap" else lin[k][sel]  # (lnu_swap is per ladder)
    whole = dict({k: np.concatenate([take(*part[g], k) for g in GROUPS]) for k in ("theta0", "step", "lnu", "lnu_swap")}, beta=plain["beta"], **box)
    counts = [len(part[g][1]) for g in GROUPS]
    whole["walker"], whole["dataset"] = np.repeat([g[0] for g in GROUPS], counts), np.repeat([g[1] for g in GROUPS], counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    own = np.concatenate([np.arange(off[q], off[q + 1]) for q in sorted((q for q, g in enumerate(GROUPS) if g[1] == 0), key=lambda q: GROUPS[q][0])])
    return whole, counts, dict(plain, **box), own


def gram_records(rec, theta, f, W, loc, scale, jeffreys=False):
    """ln P_marg (chain_util.gram_record's statements), the full chi2 at the best fit and the best fit (sample_util.gram_samples') of one theta
    by the Gram route; ln P is NaN where det F2 <= 0"""
    _, G = SU.gram_G(rec, theta, f, W)
    nG = rec.ng1 - 1
    sinv, mu = SU._sinv(scale, nG), np.asarray(loc, dtype=np.float64)
    F2 = 0.5 * (G[1:, 1:] + G[1:, 1:].T) + np.diag(sinv)
    F1 = -G[1:, 0] + sinv * mu
    F0 = G[0, 0] + mu @ (sinv * mu)
    sign, logdet = np.linalg.slogdet(F2 / (2 * np.pi))
    if not sign > 0:
        return np.nan, np.nan, np.full(nG, np.nan)
    best = np.linalg.solve(F2, F1)
    full = G[0, 0] + 2.0 * (best @ G[1:, 0]) + np.einsum("...i,ij,...j->...", best, G[1:, 1:], best)
    return -0.5 * (F0 - F1 @ best + (0.0 if jeffreys else logdet)), full, best


class SyntheticTarget(CU.HostTarget):
    """ln P_marg of a synthetic problem at any theta on the host: chain n on the Gram matrix (grad_util.gram_matrix) and growth rates of
    walker[n].  records(theta) -> (ln P [N], full chi2 [N], best [N, nG]): what host_ladder carries as ln P and its two extras"""

    def __init__(self, pb, walker, jeffreys=False, rec=None, Ds=None, dataset=None):
        """Ds [M, ndata] and dataset [N]: chain n is fitted to Ds[dataset[n]] (the groups of the device call); neither: to pb.D"""
        walker = np.asarray(walker).tolist()
        dataset = [None] * len(walker) if dataset is None else np.asarray(dataset).tolist()
        Wc = {}
        for key in set(zip(walker, dataset)):
            _, tw, tn = SY.of_walker(pb, key[0])
            Wc[key] = GU.gram_matrix(tw, pb.index, pb.D if key[1] is None else Ds[key[1]], pb.invcov, tn)
        super().__init__(pb.rec if rec is None else rec, pb.f[walker], [Wc[key] for key in zip(walker, dataset)], pb.loc, pb.scale, jeffreys)

    def records(self, theta):
        out = [gram_records(self.rec, th, f, W, *self.lk) for th, f, W in zip(theta, self.fs, self.Ws)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out])


def mixing_counts(r, T):
    """of a host_ladder result, summed over its ladders that have not failed -> dict(accepted [R], refused [R] (moves per rung index), swapped,
    kept [max(R - 1, 1)] (swaps per adjacent pair), outside (proposals beyond the box))"""
    ok = r["nswap"][:, 0] >= 0
    R = r["naccept"].size // ok.size
    na = r["naccept"].reshape(-1, R)[ok]
    return dict(accepted=na.sum(0), refused=(T - na).sum(0), swapped=r["nswap"][ok].sum(0), kept=(r["tried"] - r["nswap"])[ok].sum(0), outside=int(r["outside"][ok].sum()))


def mixed_in_sum(r, T):
    """the mixing condition of the synthetic ladders, weaker than mixed(), which asks it of every ladder: summed over the ladders of the call,
    every rung index has an accepted and a refused move, every adjacent pair an accepted and a refused swap, and a proposal left the box"""
    c = mixing_counts(r, T)
    R = c["accepted"].size
    return bool(np.all(c["accepted"] > 0) and np.all(c["refused"] > 0) and (R == 1 or (np.all(c["swapped"] > 0) and np.all(c["kept"] > 0))) and c["outside"] > 0)
