"""The Metropolis chains of eftb_draws_chain_params restated in NumPy, beside grad_util.py, hess_util.py and sample_util.py; shared by the
CPU tests (test_draw_chains.py) and the GPU tests (test_gpu_draw_chains.py).

host_chain   the algorithm of the device call, vectorised over the chains, around any ln P: per step theta' = theta + step, a proposal
             outside the box rejected without an evaluation, otherwise accepted iff ln P' is finite and
             lnu < (ln P' + pri') - (ln P + pri).  prior_term is the kernel's pri: parameter order, q = (theta_p - loc_p) sinv_p,
             acc = acc + q q, -acc / 2, sinv_p = 1 / scale_p, parameters with sinv_p = 0 skipped.  NumPy rounds every operation on its own,
             as the kernel does, so fed with the device's ln P the chain is the device's bit for bit.
HostTarget   ln P_marg, its gradient and Hessian by the Gram route in NumPy (grad_util.gram_matrix, sample_util.gram_G, hess_util.gram_hessian):
             the target of the fixture likelihoods on the host, from which chain_inputs / best_fit_inputs build what the device is fed."""
import numpy as np


def prior_term(theta, loc, sinv):
    """pri [N] of theta [N, P]"""
    theta = np.asarray(theta, dtype=np.float64)
    acc = np.zeros(theta.shape[0])
    for p in range(theta.shape[1]):
        if sinv[p] == 0.0:
            continue
        q = (theta[:, p] - loc[p]) * sinv[p]
        acc = acc + q * q
    return -0.5 * acc


def prior_arrays(P, lower=None, upper=None, loc=None, scale=None):
    """lower, upper, loc, sinv [P] as the library forms them from its optional arguments"""
    lower = np.full(P, -np.inf) if lower is None else np.asarray(lower, dtype=np.float64)
    upper = np.full(P, np.inf) if upper is None else np.asarray(upper, dtype=np.float64)
    scale = np.full(P, np.inf) if scale is None else np.asarray(scale, dtype=np.float64)
    loc = np.zeros(P) if loc is None else np.asarray(loc, dtype=np.float64)
    return lower, upper, np.where(np.isfinite(scale), loc, 0.0), 1.0 / scale


def host_chain(logp_fun, theta0, step, lnu, thin=1, lower=None, upper=None, loc=None, scale=None):
    """logp_fun(theta [N, P]) -> ln P [N], or a tuple (ln P [N], extra [N, ...], ...) whose extras are carried with the state.  It is
    called once for the start and once per step with all N chains; a chain whose proposal lies outside the box (or that has failed) is
    passed its current (starting) theta instead and the value is not used, so logp_fun is never asked for a point outside the box.
    -> dict(theta [N, K, P], logp [N, K], extras (a list of [N, K, ...]), naccept [N], last [N, P], outside [N] (proposals refused for the
    box)) with K = T // thin.  A chain whose starting ln P is not finite has failed: NaN states and ln P, naccept -1."""
    theta0 = np.array(theta0, dtype=np.float64)
    step, lnu = np.asarray(step, dtype=np.float64), np.asarray(lnu, dtype=np.float64)
    N, P = theta0.shape
    T = step.shape[1]
    assert step.shape == (N, T, P) and lnu.shape == (N, T) and 1 <= thin <= T
    lower, upper, loc, sinv = prior_arrays(P, lower, upper, loc, scale)
    split = lambda r: (np.asarray(r[0], dtype=np.float64), [np.asarray(x, dtype=np.float64) for x in r[1:]]) if isinstance(r, tuple) else (np.asarray(r, dtype=np.float64), [])
    cur = theta0.copy()
    lp, ex = split(logp_fun(cur.copy()))
    lp, ex = lp.copy(), [x.copy() for x in ex]
    pri = prior_term(cur, loc, sinv)
    failed = ~np.isfinite(lp)
    K = T // thin
    out_t, out_l = np.empty((N, K, P)), np.empty((N, K))
    out_e = [np.empty((N, K) + x.shape[1:]) for x in ex]
    nacc, outside = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
    for t in range(T):
        trial = cur + step[:, t]
        inbox = np.all((trial >= lower) & (trial <= upper), axis=1) & ~failed
        outside += ~inbox & ~failed
        ask = np.where(inbox[:, None], trial, np.where(failed[:, None], theta0, cur))
        lp1, ex1 = split(logp_fun(ask))
        pri1 = prior_term(ask, loc, sinv)
        with np.errstate(invalid="ignore"):
            acc = inbox & np.isfinite(lp1) & (lnu[:, t] < (lp1 + pri1) - (lp + pri))
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
    return dict(theta=out_t, logp=out_l, extras=out_e, naccept=nacc, last=last, outside=outside)


# ----------------------------------------------------------------------------- the targets of the device tests on the host
def gram_record(rec, theta, f, W, loc, scale, jeffreys=False):
    """ln P_marg of one theta by the Gram route (sample_util.gram_G, then F2 / F1 / F0 as draws_solve forms them); NaN where det F2 <= 0"""
    import sample_util as SU

    _, G = SU.gram_G(rec, theta, f, W)
    nG = rec.ng1 - 1
    sinv, mu = SU._sinv(scale, nG), np.asarray(loc, dtype=np.float64)
    F2 = 0.5 * (G[1:, 1:] + G[1:, 1:].T) + np.diag(sinv)
    F1 = -G[1:, 0] + sinv * mu
    F0 = G[0, 0] + mu @ (sinv * mu)
    sign, logdet = np.linalg.slogdet(F2 / (2 * np.pi))
    if not sign > 0:
        return np.nan
    return -0.5 * (F0 - F1 @ np.linalg.solve(F2, F1) + (0.0 if jeffreys else logdet))


class HostTarget:
    """ln P_marg of N chains on the host: chain n against the Gram matrix Ws[n] and growth rates fs[n] of its walker"""

    def __init__(self, rec, fs, Ws, loc, scale, jeffreys=False):
        self.rec, self.fs, self.Ws, self.lk = rec, fs, Ws, (loc, scale, jeffreys)

    def logp(self, theta):
        return np.array([gram_record(self.rec, th, f, W, *self.lk) for th, f, W in zip(theta, self.fs, self.Ws)])

    def hess(self, theta):
        """-> ln P [N], grad [N, P], hess [N, P, P] (hess_util.gram_hessian): what newton_maximize asks for"""
        import hess_util as HU

        out = [HU.gram_hessian(self.rec, th, f, W, *self.lk) for th, f, W in zip(theta, self.fs, self.Ws)]
        return tuple(np.array([o[i] for o in out]) for i in range(3))


def chain_inputs(center, factor, sig, seed, T, box=1.5, spread=0.5):
    """The inputs of a chain test: chain n starts spread proposal steps (factor [P, P] or [N, P, P]) off center[n]; the box, shared by the
    chains, reaches box * sig [N, P] beyond the outermost centers, close enough for proposals to leave it.
    -> dict(theta0 [N, P], step [N, T, P], lnu [N, T], lower [P], upper [P])"""
    from eftpipe_amd.marginal import metropolis_proposals

    center = np.asarray(center, dtype=np.float64)
    N, P = center.shape
    L = np.broadcast_to(np.asarray(factor, dtype=np.float64), (N, P, P))
    rng = np.random.default_rng(seed)
    theta0 = center + spread * np.einsum("npq,nq->np", L, rng.standard_normal((N, P)))
    step, lnu = metropolis_proposals(rng, N, T, factor)
    lower, upper = np.min(center - box * sig, axis=0), np.max(center + box * sig, axis=0)
    return dict(theta0=np.clip(theta0, lower, upper), step=step, lnu=lnu, lower=lower, upper=upper)


def best_fit_inputs(hessfun, start, seed, T, **kw):
    """chain_inputs around the best fits: every chain climbs from start [N, P] (newton_maximize on hessfun -> ln P, grad, hess), its
    proposal factor is proposal_factor of the Hessian there and sig the posterior standard deviations (-H)^-1 gives"""
    from eftpipe_amd.marginal import newton_maximize, proposal_factor

    best, _, _, H, _, conv = newton_maximize(hessfun, start)
    assert np.all(conv), "a start of the chain inputs did not reach its best fit"
    sig = np.sqrt(np.diagonal(np.linalg.inv(-H), axis1=1, axis2=2))
    return chain_inputs(best, proposal_factor(H), sig, seed, T, **kw)


def nnlo_arrays():
    """the arrays of test_gpu_draws_grad._nnlo_problem without its engine (the same generator, asked in the same order): T, TN
    [3, 3, 24, 20], index, D, Ci, theta [10, 3], f [3], counts"""
    rng = np.random.default_rng(4)
    nx, nC, counts = 20, 3, [2, 5, 3]
    N = sum(counts)
    T = rng.normal(0, 1, (nC, 3, 24, nx)) * np.logspace(0, 3, 24)[:, None] / np.array([1.0] * 21 + [1e4, 1e7, 1e7])[:, None]
    TN = rng.normal(0, 1, (nC, 3, 24, nx)) * 0.3
    index = np.sort(rng.choice(3 * nx, 40, replace=False)).astype(np.int32)
    D = rng.normal(0, 50, 40)
    Ci = np.diag(1.0 / rng.uniform(5, 20, 40) ** 2)
    theta = np.array([2.0, 0.5, 0.3]) + 0.2 * rng.normal(size=(N, 3))
    f = rng.uniform(0.6, 0.9, nC)
    return T, TN, index, D, Ci, theta, f, counts
