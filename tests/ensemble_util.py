"""The affine-invariant ensembles of eftb_draws_ensemble_params restated in NumPy, beside chain_util.py and temper_util.py; shared by the CPU
tests (test_draw_ensemble.py) and the GPU tests (test_gpu_draw_ensemble.py).

host_ensemble   the algorithm of the device call, vectorised over the chains, around any ln P.  Chain n is member n % K of ensemble n // K;
                members 0 ... K/2 - 1 are half 0, the rest half 1.  Sweep t: half 0 moves against the current half 1, then half 1 against the
                new half 0.  Member k with partner j = member pick[n, t] of the other half: d = theta_k - theta_j, theta' = theta_j + z[n, t] d;
                outside the box: rejected without an evaluation; otherwise accepted iff ln P' is finite and
                lnq[n, t] < (ln P' + pri') - (ln P + pri) (chain_util.prior_term).  NumPy rounds every operation on its own, as the kernel
                does, so fed with the device's ln P the ensembles are the device's bit for bit.  Instead of lnq the caller may pass lnu and
                the exponent of the Jacobian: lnq = lnu - exponent ln z (the move's own is P - 1).
ens_waves       the waves of an ensemble's workgroup, from the documented layout.
ENSEMBLE_WAVES  ens_waves at every case of synth_like_util.CASES (test_draw_ensemble.py pins the table).
ensemble_case   the inputs of the device tests from a case of test_draw_chains.chain_case."""
import numpy as np

import chain_util as CU

ENS_MAXK, ENS_SLOT = 64, 61


def host_ensemble(logp_fun, theta0, K, z, pick, lnq=None, thin=1, lower=None, upper=None, loc=None, scale=None, lnu=None, exponent=None, stale=False):
    """logp_fun as chain_util.host_chain's (ln P [N], or a tuple with extras that are carried with the state): called once for the start
    and once per half-sweep with all N chains; a chain that does not move in that half-sweep, whose proposal lies outside the box, or that
    has failed is passed its current (starting) theta instead and the value is not used, so logp_fun is never asked for a point outside the
    box.  stale: half 1 moves against the positions half 0 had before the sweep -- not the algorithm, for the test that tells the two apart.
    -> dict(theta [N, Kt, P], logp [N, Kt], extras, naccept [N], last [N, P], outside [nens] (proposals refused for the box, per ensemble),
    asked (every theta logp_fun was given after the start, [2 T, N, P])) with Kt = T // thin.  An ensemble one of whose members starts
    without a finite ln P has failed: NaN everywhere, naccept = -1."""
    theta0 = np.array(theta0, dtype=np.float64)
    z, pick = np.asarray(z, dtype=np.float64), np.asarray(pick)
    (N, P), T = theta0.shape, z.shape[1]
    if lnq is None:
        lnq = np.asarray(lnu, dtype=np.float64) - exponent * np.log(z)
    lnq = np.asarray(lnq, dtype=np.float64)
    assert K % 2 == 0 and K >= 2 and N % K == 0 and z.shape == pick.shape == lnq.shape == (N, T) and 1 <= thin <= T
    assert np.all(pick >= 0) and np.all(pick < K // 2)
    nens, half = N // K, K // 2
    lower, upper, loc, sinv = CU.prior_arrays(P, lower, upper, loc, scale)
    split = lambda r: (np.asarray(r[0], dtype=np.float64), [np.asarray(x, dtype=np.float64) for x in r[1:]]) if isinstance(r, tuple) else (np.asarray(r, dtype=np.float64), [])
    cur = theta0.copy()
    lp, ex = split(logp_fun(cur.copy()))
    lp, ex = lp.copy(), [x.copy() for x in ex]
    pri = CU.prior_term(cur, loc, sinv)
    ens_failed = np.any(~np.isfinite(lp).reshape(nens, K), axis=1)
    failed = np.repeat(ens_failed, K)
    Kt = T // thin
    out_t, out_l = np.empty((N, Kt, P)), np.empty((N, Kt))
    out_e = [np.empty((N, Kt) + x.shape[1:]) for x in ex]
    nacc, outside = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    member, base = np.arange(N) % K, np.arange(N) // K * K
    asked = []
    for t in range(T):
        before = cur.copy()
        for h in range(2):
            active = (member // half == h) & ~failed
            partner = base + (1 - h) * half + pick[:, t]
            tj = (before if stale and h == 1 else cur)[partner]
            d = cur - tj
            trial = tj + z[:, t, None] * d
            inbox = np.all((trial >= lower) & (trial <= upper), axis=1) & active
            outside += active & ~inbox
            ask = np.where(inbox[:, None], trial, np.where(failed[:, None], theta0, cur))
            asked.append(ask.copy())
            lp1, ex1 = split(logp_fun(ask))
            pri1 = CU.prior_term(ask, loc, sinv)
            with np.errstate(invalid="ignore"):
                acc = inbox & np.isfinite(lp1) & (lnq[:, t] < (lp1 + pri1) - (lp + pri))
            cur[acc], lp[acc], pri[acc] = trial[acc], lp1[acc], pri1[acc]
            for x, x1 in zip(ex, ex1):
                x[acc] = x1[acc]
            nacc += acc
        if (t + 1) % thin == 0:
            k = (t + 1) // thin - 1
            out_t[:, k], out_l[:, k] = cur, lp
            for o, x in zip(out_e, ex):
                o[:, k] = x
    last = cur.copy()
    for a in [out_t, out_l, last] + out_e:
        a[failed] = np.nan
    nacc[failed] = -1
    return dict(theta=out_t, logp=out_l, extras=out_e, naccept=nacc, last=last, outside=outside.reshape(nens, K).sum(1), asked=np.array(asked))


# ----------------------------------------------------------------------------- the LDS of an ensemble's workgroup
def ens_waves(J1, nG, nnz, K, limit=160 * 1024):
    """W = min(8, K / 2, the waves that fit): per workgroup W_c [J1][J1], the powers of f [8][7], col (two ints to a double) and the prior
    table [4][32]; per wave th [34], val, H [nG + 1][J1], G [nG + 1][nG + 1], two theta of 32 and two records of 26; then 61 doubles per
    member (theta [32], record [26], ln P, pri, accept count).  0: the members leave no room for one wave."""
    nnzp = (nnz + 1) // 2 * 2
    wg, wave = J1 * J1 + 56 + nnzp // 2 + 128, 34 + nnzp + (nG + 1) * J1 + (nG + 1) ** 2 + 116
    return int(max(0, min(8, K // 2, (limit - 8 * (wg + ENS_SLOT * K)) // (8 * wave))))


def case_waves(case, K):
    import temper_util as TU

    return ens_waves(*TU.case_shape(case), K)


# W at K = 16 and at K = ENS_MAXK for every case of synth_like_util.CASES, and the largest even K that leaves room for one wave (at most
# ENS_MAXK); pinned by test_draw_ensemble.py::test_wave_table, and the library's refusal names the same shapes
ENSEMBLE_WAVES = dict(A=(8, 8, 64), B=(8, 8, 64), C=(8, 8, 64), D=(8, 8, 64), E=(8, 8, 64), F=(5, 4, 64), G=(2, 2, 64), H=(2, 1, 64), I=(1, 0, 24), J=(3, 1, 64),
                      Gf=(2, 2, 64), Ef=(8, 8, 64))
# (case G at K = 8: three waves for four members of a half, so its passes come from the LDS limit; case I holds 24 members and refuses 26)


def most_members(case):
    K = ENS_MAXK
    while K >= 2 and not case_waves(case, K):
        K -= 2
    return K


# ----------------------------------------------------------------------------- the inputs of the device tests
T_ENS, THIN = 37, 5
ENSEMBLES = dict(auto=[3, 0, 1, 1], cross=[3, 0, 1, 1], full=[1, 0, 1, 3], nnlo=[1, 0, 3])  # per walker: none, one and three
# (K, seed, spread, box) per case: the members start `spread` dispersions of the case's own increments around the mean start of the case's
# chains on their walker, and the box reaches `box` dispersions beyond the outermost start.  Tuned on the host
# (test_draw_ensemble.py::test_device_inputs_move_and_are_refused) until every member had 0 < naccept < T and every ensemble a proposal
# outside the box under every prior of the case.
TUNING = dict(auto=(4, 2, 1.0, 0.5), cross=(4, 1, 1.0, 0.5), full=(4, 1, 1.0, 0.5), nnlo=(4, 1, 1.0, 0.5))
# the other sizes on marg.npz auto: K -> (ensembles per walker, seed, spread, box)
SIZES = {2: ([2, 0, 1, 1], 3, 1.0, 0.5), 6: ([2, 0, 1, 1], 2, 1.0, 0.5), 16: ([1, 0, 0, 1], 1, 1.0, 0.5), 20: ([1, 0, 0, 1], 1, 1.0, 0.5),
         ENS_MAXK: ([1, 0, 0, 1], 1, 1.0, 0.5)}


def ensemble_inputs(case, ensembles, K, T, seed, spread=1.0, box=0.5):
    """Ensembles of K members on the walkers of a chain_case -> dict(theta0 [N, P], z, pick, lnq [N, T], lower, upper [P], counts (chains per
    walker), walker [N], K)"""
    from eftpipe_amd.marginal import stretch_proposals

    inp, w0 = case["inp"], case["walker"]
    sd = inp["step"].std(axis=(0, 1))
    counts = [K * n for n in ensembles]
    walker = np.repeat(np.arange(len(counts)), counts)
    assert all(n == 0 or np.any(w0 == c) for c, n in enumerate(ensembles))
    center = np.stack([inp["theta0"][w0 == c].mean(0) for c in walker])
    rng = np.random.default_rng(seed)
    theta0 = center + spread * sd * rng.standard_normal(center.shape)
    z, pick, lnq = stretch_proposals(rng, len(walker) // K, K, T, theta0.shape[1])
    return dict(theta0=theta0, z=z, pick=pick, lnq=lnq, lower=theta0.min(0) - box * sd, upper=theta0.max(0) + box * sd, counts=counts, walker=walker, K=K)


def ensemble_case(tag):
    """-> (case of test_draw_chains.chain_case, ensemble_inputs for it)"""
    from test_draw_chains import chain_case

    case = chain_case(tag)
    K, seed, spread, box = TUNING[tag]
    return case, ensemble_inputs(case, ENSEMBLES[tag], K, T_ENS, seed, spread, box)


def size_case(K, case=None):
    """the ensembles of the GPU tests at the other sizes (marg.npz auto, T = 37)"""
    from test_draw_chains import chain_case

    case = chain_case("auto") if case is None else case
    ensembles, seed, spread, box = SIZES[K]
    return case, ensemble_inputs(case, ensembles, K, T_ENS, seed, spread, box)


def long_case():
    """the T = 300 call of the GPU tests (auto, K = 4, one ensemble on each of two walkers): it crosses the launch boundary at 256 sweeps"""
    from test_draw_chains import chain_case

    case = chain_case("auto")
    return case, ensemble_inputs(case, [1, 0, 0, 1], 4, 300, 18, 1.0, 0.5)


def ensemble_target(case, ein, i):
    """the target of prior i of a case for the chains of ensemble_inputs, on the host (the Gram route in NumPy)"""
    w = ein["walker"]
    return CU.HostTarget(case["rec"], case["fw"][w], [case["Ws"][c] for c in w], *case["priors"][i])


def mixed(r, T):
    """every member moved and was refused, every ensemble met the box"""
    return bool(np.all(r["naccept"] > 0) and np.all(r["naccept"] < T) and np.all(r["outside"] > 0))


def cut(ein, a, b):
    """sweeps a ... b - 1 of ensemble inputs"""
    return dict(ein, z=np.ascontiguousarray(ein["z"][:, a:b]), pick=np.ascontiguousarray(ein["pick"][:, a:b]), lnq=np.ascontiguousarray(ein["lnq"][:, a:b]))


def take(ein, sel):
    """the chains sel (whole ensembles) of ensemble inputs"""
    return dict(ein, theta0=ein["theta0"][sel], z=ein["z"][sel], pick=ein["pick"][sel], lnq=ein["lnq"][sel])


# ----------------------------------------------------------------------------- ensembles on the synthetic likelihoods
PRIOR_LOC, PRIOR_SCALE = 1.0, 0.5  # the Gaussian theta priors of the synthetic device tests (temper_util.theta_prior)
# (K, ensembles per walker, T, seed, spread) per synthetic call of the GPU tests: the members of ensemble i of a walker start `spread` around
# row i (mod the walker's rows) of the case's own theta, and the box reaches half a spread beyond the outermost start.  ln P of these
# likelihoods changes by 1e2 to 1e3 between two of a case's rows, so every case has its own spread; tuned on the host
# (test_draw_ensemble.py::test_synthetic_inputs_mix), without and with Jeffreys, until G and I met mixed() -- every member moved and was
# refused, every ensemble met the box -- as the fixtures' inputs do.  Gf runs T = 4 sweeps, in which a member cannot be asked to do both:
# it meets mixed_in_sum, the condition summed over the call's ensembles, checked on the host at 61 ensembles on walker 0.
#   G      three waves for the four members of a half: two passes a half-sweep, the second ragged, from the LDS limit
#   I      the most members that fit beside one wave (24, twelve passes); 26 are refused
#   Gf     K = 2, T = 4 with enough ensembles on walker 0 that the first workgroups take a second one (test_gpu_draw_ensemble.py)
SYNTH_TUNING = {"G": (8, [2, 0, 1], 20, 1, 0.01), "I": (24, [1, 0, 1], 24, 1, 0.01), "Gf": (2, [2, 0, 1], 4, 1, 0.03)}


def synthetic_ensemble(case, K, ensembles, T, seed, spread, kind="gauss", singular=None, box=0.5):
    """-> what ensemble_inputs returns, on the walkers of synth_like_util.case_problem(case, kind, singular)"""
    import synth_like_util as SY

    from eftpipe_amd.marginal import stretch_proposals

    pb = SY.case_problem(case, kind, singular)
    counts = [K * n for n in ensembles]
    walker = np.repeat(np.arange(len(counts)), counts)
    assert len(counts) == len(pb.counts) and all(n == 0 or m > 0 for n, m in zip(counts, pb.counts))
    rows = [pb.theta[pb.walker == w] for w in range(len(counts))]
    base = np.stack([rows[w][(i // K) % len(rows[w])] for w, n in enumerate(counts) for i in range(n)])
    rng = np.random.default_rng(seed)
    theta0 = base + spread * rng.standard_normal(base.shape)
    z, pick, lnq = stretch_proposals(rng, len(walker) // K, K, T, pb.P)
    return dict(theta0=theta0, z=z, pick=pick, lnq=lnq, lower=theta0.min(0) - box * spread, upper=theta0.max(0) + box * spread, counts=counts, walker=walker, K=K)


def synthetic_inputs(name, ensembles=None, **kw):
    K, ens, T, seed, spread = SYNTH_TUNING[name]
    return synthetic_ensemble(name, K, ens if ensembles is None else ensembles, T, seed, spread, **kw)


def theta_prior(P):
    return dict(prior_loc=np.full(P, PRIOR_LOC), prior_scale=np.full(P, PRIOR_SCALE))


def mixed_in_sum(r, T):
    """the mixing condition of the synthetic ensembles, weaker than mixed(), which asks it of every member: summed over the ensembles of the
    call that have not failed, every member index has an accepted and a refused move, and a proposal left the box"""
    K = r["naccept"].size // r["outside"].size
    na = r["naccept"].reshape(-1, K)
    na = na[na[:, 0] >= 0]
    return bool(np.all(na.sum(0) > 0) and np.all((T - na).sum(0) > 0) and r["outside"].sum() > 0)
