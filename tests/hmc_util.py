"""The leapfrog trajectories of eftb_draws_hmc_params restated in NumPy, beside chain_util.py; shared by the CPU tests (test_draw_hmc.py) and
the GPU tests (test_gpu_draw_hmc.py).

host_hmc     the algorithm of the device call, vectorised over the chains, around any fun(theta [N, P]) -> (ln P [N], grad [N, P], extras...).
             Target ln pi = ln P + pri with chain_util.prior_term; g = grad ln P + grad pri, (grad pri)_p = -((theta_p - loc_p) sinv_p) sinv_p,
             parameters with sinv_p = 0 skipped.  Momenta in the whitened space of the lower-triangular F (M^-1 = F F^T; None: the identity,
             multiplied through like any other F):
                 k = 1/2 sum_p r_p r_p;  h = 0.5 eps;  r = r + h u,  u_p = sum_{q >= p} F[q][p] g_q
                 nleap times: theta_p = theta_p + eps v_p, v_p = sum_{q <= p} F[p][q] r_q; box test; ln P and g at theta; r = r + (eps | h last) u
                 ratio = ((ln P' + pri') - k') - ((ln P + pri) - k);  accept iff not aborted and lnu < ratio
             every sum with the index ascending from 0 as acc = acc + x y.  NumPy rounds every operation on its own, as the kernel does, so fed
             with the device's ln P and gradient the chains are the device's bit for bit.  A trajectory is aborted when a position leaves the
             box or ln P or a component of g is not finite; fun is never asked for a point outside the box (an aborted or failed chain is
             passed its starting theta instead and the values are not used).
trajectory   one leapfrog trajectory of every chain, the piece host_hmc is built from: the reversibility and energy tests call it directly."""
import numpy as np

import chain_util as CU


def _split(r):
    return np.array(r[0], dtype=np.float64), np.array(r[1], dtype=np.float64), [np.array(x, dtype=np.float64) for x in r[2:]]


def target_grad(gl, theta, loc, sinv):
    """g [N, P] of the target from grad ln P [N, P]"""
    g = np.array(gl, dtype=np.float64)
    for p in range(g.shape[1]):
        if sinv[p] == 0.0:
            continue
        q = (theta[:, p] - loc[p]) * sinv[p]
        g[:, p] = g[:, p] + -(q * sinv[p])
    return g


def kinetic(r):
    acc = np.zeros(r.shape[0])
    for p in range(r.shape[1]):
        acc = acc + r[:, p] * r[:, p]
    return 0.5 * acc


def ft_times(F, g):
    """u [N, P], u_p = sum_{q >= p} F[q][p] g_q with q ascending"""
    acc = np.zeros_like(g)
    for q in range(g.shape[1]):
        acc[:, : q + 1] = acc[:, : q + 1] + F[:, q, : q + 1] * g[:, q : q + 1]
    return acc


def f_times(F, r):
    """v [N, P], v_p = sum_{q <= p} F[p][q] r_q with q ascending"""
    acc = np.zeros_like(r)
    for q in range(r.shape[1]):
        acc[:, q:] = acc[:, q:] + F[:, q:, q] * r[:, q : q + 1]
    return acc


def factors(factor, N, P):
    """F [N, P, P] of the optional argument: None is the identity; what lies above the diagonal is not read"""
    F = np.eye(P) if factor is None else np.asarray(factor, dtype=np.float64)
    return np.tril(np.broadcast_to(F, (N, P, P)))


def trajectory(fun, theta, g, r, eps, nleap, F, lower, upper, loc, sinv, safe, skip=None):
    """nleap leapfrog steps of every chain from (theta, r) with g the target's gradient at theta; eps [N]; safe [N, P]: the point asked for in
    the place of an aborted chain's (or of a chain in skip [N]).  -> theta', r', ln P', g', extras', box [N], bad [N] (aborted; box: at the box)"""
    N, P = theta.shape
    skip = np.zeros(N, dtype=bool) if skip is None else skip
    theta, r = theta.copy(), r.copy()
    h = 0.5 * eps
    box, bad = np.zeros(N, dtype=bool), skip.copy()
    lp, ex = np.full(N, np.nan), None
    with np.errstate(invalid="ignore", over="ignore"):
        r = r + h[:, None] * ft_times(F, g)
        for s in range(nleap):
            theta = np.where(bad[:, None], theta, theta + eps[:, None] * f_times(F, r))
            out = ~bad & ~np.all((theta >= lower) & (theta <= upper), axis=1)
            box |= out
            bad |= out
            lp1, gl1, ex1 = _split(fun(np.where(bad[:, None], safe, theta)))
            g1 = target_grad(gl1, theta, loc, sinv)
            bad |= ~bad & ~(np.isfinite(lp1) & np.all(np.isfinite(g1), axis=1))
            lp, g, ex = lp1, g1, ex1
            r = np.where(bad[:, None], r, r + np.where(s == nleap - 1, h, eps)[:, None] * ft_times(F, g))
    return theta, r, lp, g, ex, box, bad & ~skip


def host_hmc(fun, theta0, mom, lnu, eps, nleap, factor=None, thin=1, lower=None, upper=None, loc=None, scale=None):
    """-> dict(theta [N, K, P], logp [N, K], extras (a list of [N, K, ...]), naccept [N], last [N, P], log_ratio [N, T], outside [N]
    (trajectories aborted at the box), aborted [N] (all aborted ones), refused [N] (rejected without aborting)) with K = T // thin.  A chain
    whose starting ln P is not finite has failed: NaN states, ln P and ratios, naccept -1."""
    theta0 = np.array(theta0, dtype=np.float64)
    mom, lnu = np.asarray(mom, dtype=np.float64), np.asarray(lnu, dtype=np.float64)
    N, P = theta0.shape
    T = mom.shape[1]
    assert mom.shape == (N, T, P) and lnu.shape == (N, T) and 1 <= thin <= T and nleap >= 1
    eps = np.asarray(eps, dtype=np.float64)
    eps = np.broadcast_to(eps if eps.ndim != 1 else eps[:, None], (N, T))
    F = factors(factor, N, P)
    lower, upper, loc, sinv = CU.prior_arrays(P, lower, upper, loc, scale)
    cur = theta0.copy()
    lp, gl, ex = _split(fun(cur.copy()))
    g = target_grad(gl, cur, loc, sinv)
    pri = CU.prior_term(cur, loc, sinv)
    failed = ~np.isfinite(lp)
    K = T // thin
    out_t, out_l = np.empty((N, K, P)), np.empty((N, K))
    out_e = [np.empty((N, K) + x.shape[1:]) for x in ex]
    ratio = np.full((N, T), np.nan)
    nacc, outside, aborted, refused = (np.zeros(N, dtype=np.int64) for _ in range(4))
    for t in range(T):
        r0 = mom[:, t]
        k0 = kinetic(r0)
        trial, r1, lp1, g1, ex1, box, bad = trajectory(fun, cur, g, r0, eps[:, t], nleap, F, lower, upper, loc, sinv, theta0, skip=failed)
        pri1 = CU.prior_term(trial, loc, sinv)
        with np.errstate(invalid="ignore", over="ignore"):
            lr = ((lp1 + pri1) - kinetic(r1)) - ((lp + pri) - k0)
            lr[bad | failed] = np.nan
            acc = ~bad & ~failed & (lnu[:, t] < lr)
        ratio[:, t] = lr
        cur[acc], lp[acc], pri[acc], g[acc] = trial[acc], lp1[acc], pri1[acc], g1[acc]
        for x, x1 in zip(ex, ex1):
            x[acc] = x1[acc]
        nacc += acc
        outside += box
        aborted += bad
        refused += ~acc & ~bad & ~failed
        if (t + 1) % thin == 0:
            k = (t + 1) // thin - 1
            out_t[:, k], out_l[:, k] = cur, lp
            for o, x in zip(out_e, ex):
                o[:, k] = x
    last = cur.copy()
    for a in [out_t, out_l, last, ratio] + out_e:
        a[failed] = np.nan
    nacc[failed] = -1
    return dict(theta=out_t, logp=out_l, extras=out_e, naccept=nacc, last=last, log_ratio=ratio, outside=outside, aborted=aborted, refused=refused)
