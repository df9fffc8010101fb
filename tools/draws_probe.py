#!/usr/bin/env python3
"""Fast / slow split on one GPU: parameter draws per second through MarginalLikelihood.logp_draws (eftb_draws_logp) against the templates of
one set of walkers, for two shapes -- the single-tracer marg.npz likelihood and the cfg 3 joint likelihood (3 tracers, 142 data points,
14 marginalised parameters, tests/golden/cfg3.npz) -- split into

    rows    host row building (parambasis.gaussian_rows_many / marginal.joint_gaussian_rows_many) for all draws
    h2d     the rows' bytes host -> device, pageable as the call takes them (one hipMemcpy of the same array)
    gram    first call after put("TEMPL") minus a cached call: gather + A C^-1 + A U^T of every walker
    draws   a cached call minus h2d: draw kernel + the [N][26] records back + unpacking

the same draws through MarginalLikelihood.logp_draws_params (eftb_draws_logp_params: theta [N, P] in, the rows built on the device from the
draw recipe) -- per call, and end to end with theta stacked from the sampler's per-parameter arrays -- with the bytes per draw over PCIe;
the same call with d ln P / d theta (logp_draws_params(grad=True), eftb_draws_logp_grad_params), per call and end to end, and its cost in
forward calls (the 2 P central differences it replaces are the yardstick); the same call with d2 ln P / d theta d theta
(logp_draws_params(grad=True, hess=True), eftb_draws_logp_hess_params), per call, and its cost in gradient calls (the 2 P gradient calls of
a central difference are the yardstick);
and, for comparison, the same number of evaluations through eval_logp (theory + likelihood per walker; Nk = 512, resummation + AP, an
interpolation onto the data k instead of the window: a lower bound on the cost of the real thing).  GPU box.

    python tools/draws_probe.py [--draws N] [--walkers C]

--datasets M: many data vectors sharing one covariance (MarginalLikelihood.set_datasets, ``groups=``) instead, for both
shapes, 1 walker x M data sets x --draws draws per group (default 1024 in this mode), Hessian calls, medians of cached calls:

    (a) groups   one logp_draws_params(grad=True, hess=True, groups=...) call over the M groups
    (b) loop     the same job without data sets: per data vector a new MarginalLikelihood, set_draw_recipe, one call
    (c) plain    one call without groups with the same total draws on the one walker: the ceiling

On a tree without set_datasets (a) is skipped, so that the same file times (b) and (c) on the parent commit.

    python tools/draws_probe.py --datasets M [--draws N]

--samples [S,S,...]: samples of the marginalised parameters (MarginalLikelihood.sample_gaussian_params) instead, for both
shapes, 1 walker x --draws draws (default 4096), medians of 9 cached calls with [min, max]:

    (a) samples  the sample call at each S (default 1, 8, 64), with and without predict
    (b) floor    logp_draws_params(return_best=True) on the same draws, the S = 0 floor; and the gradient and Hessian calls
    (c) numpy    the NumPy route of tests/sample_util.data_space_samples on templates fetched to the host (timed on 32 draws, scaled)

On a tree without sample_gaussian_params only (b) runs, so that the same file times the existing calls on the parent commit.

    python tools/draws_probe.py --samples [--draws N]

--chains [n,n,...]: Metropolis chains over theta (MarginalLikelihood.metropolis_draws_params) instead, for both shapes,
--walkers walkers (default 128 in this mode) x n chains each (default 1 and 8), --steps T steps (default 256), medians of 9 cached calls
with [min, max], on the same proposals:

    (a) chains   one metropolis_draws_params call: all T steps of all chains in the kernel
    (b) loop     the host loop: per step the proposals formed in NumPy, one logp_draws_params call, the acceptance rule in NumPy
    (c) ceiling  one logp_draws_params call on N T independent draws: the throughput a Markov chain cannot reach

On a tree without metropolis_draws_params (a) is skipped, so that the same file times (b) and (c) on the parent commit.

    python tools/draws_probe.py --chains [--walkers C] [--steps T]

--drag [n,n,...]: dragging chains between two walkers (MarginalLikelihood.drag_draws_params) instead, for both shapes,
--walkers pairs (default 128; pair g drags from walker g to walker pairs + g, twice as many walkers are resident) x n chains each (default
1 and 8), --steps T steps (default 256) on drag_fractions(T), medians of 9 cached calls with [min, max], on the same proposals:

    (a) drag     one drag_draws_params call (thin = 0): all T steps of all chains in the kernel, both walkers' ln P per step
    (b) loop     the host loop: per step the proposals formed in NumPy, two logp_draws_params calls (the start and the end walkers), the
                 interpolated acceptance rule and the two sums in NumPy

(a) and (b) are asserted to return the same chains, accept counts and sums.  On a tree without drag_draws_params (a) is skipped, so that the
same file times (b) on the parent commit.

    python tools/draws_probe.py --drag [--walkers G] [--steps T]

--hmc [n,n,...]: Hamiltonian Monte Carlo over theta (MarginalLikelihood.hmc_draws_params) instead, for both shapes, --walkers
walkers (default 128) x n chains each (default 1 and 8), --steps gradient evaluations per chain (default 256: one launch) as --steps / --leap
trajectories of --leap leapfrog steps (default 8), medians of 9 cached calls with [min, max], on the same momenta, uniforms and step sizes:

    (a) hmc      one hmc_draws_params call: all trajectories of all chains in the kernel
    (b) loop     the host loop (tests/hmc_util.host_hmc): per leapfrog step one gradient call (eftb_draws_logp_grad_params), the integrator and the
                 acceptance rule in NumPy
    (c) ceiling  one logp_draws_params(grad=True) call on as many independent draws as (a) evaluates gradients

(a) and (b) are asserted to return the same chains, accept counts and ratios.  On a tree without hmc_draws_params (a) is skipped, so that
the same file (with tests/hmc_util.py beside it) times (b) and (c) on the parent commit.

    python tools/draws_probe.py --hmc [--walkers C] [--steps E] [--leap L]

--temper [n,n,...]: parallel tempering over theta (MarginalLikelihood.temper_draws_params) instead, for both shapes, --walkers
walkers (default 128) x n ladders each (default 1 and 4) of R = 4 rungs on the geometric ladder from 1 to 0.1, --steps T steps (default 256)
with a swap event every fourth, medians of 9 cached calls with [min, max], on the same proposals and uniforms:

    (a) temper   one temper_draws_params call: all T steps of all rungs and every swap in the kernel
    (b) loop     T / 4 metropolis_draws_params calls of four steps with the swaps in NumPy between them: the only route without (a)
    (c) chains   one metropolis_draws_params call of the same N T steps, without swaps: (a) / (c) is the price of the barriers

(a) and (b) are asserted to return the same ladders and swap counts.  On a tree without temper_draws_params (a) is skipped, so that the same
file times (b) and (c) on the parent commit.

    python tools/draws_probe.py --temper [--walkers C] [--steps T]

--ensemble [n,n,...]: affine-invariant ensembles over theta (MarginalLikelihood.ensemble_draws_params) instead, for both shapes,
--walkers walkers (default 128) x n ensembles each (default 1 and 4) of K = 8 members, --steps T sweeps (default 256), medians of 9 cached
calls with [min, max], on the same stretch factors, partners and uniforms:

    (a) ensemble  one ensemble_draws_params call: all T sweeps of all ensembles in the kernel
    (b) loop      2 T logp_draws_params calls, one per half-sweep on the half that moves, with the rule in NumPy: the only route without (a)
    (c) chains    one metropolis_draws_params call of the same N T evaluations: (a) / (c) is the price of the two barriers per sweep

(a) and (b) are asserted to return the same ensembles.  On a tree without ensemble_draws_params (a) is skipped, so that the same file times (b)
and (c) on the parent commit.

    python tools/draws_probe.py --ensemble [--walkers C] [--steps T]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cfg3_util as U  # noqa: E402
from eftpipe_amd import synth  # noqa: E402
from eftpipe_amd import tables as TB  # noqa: E402
from eftpipe_amd.engine import Engine  # noqa: E402
from eftpipe_amd.marginal import MarginalLikelihood, data_index, joint_draw_recipe, joint_gaussian_rows_many  # noqa: E402
from eftpipe_amd.parambasis import WestCoastBasis, gaussian_params, gaussian_rows, gaussian_rows_many  # noqa: E402
from eftpipe_amd.tables import EngineConfig  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def times(fn, n=5):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def med(fn, n=5):
    return float(np.median(times(fn, n)))


def h2d_seconds(a):
    """one synchronous hipMemcpy of the array (pageable, as the draw call takes it) into a device buffer of its size"""
    import ctypes as C

    hip = C.CDLL("libamdhip64.so")
    dev = C.c_void_p()
    if hip.hipMalloc(C.byref(dev), C.c_size_t(a.nbytes)) != 0:
        raise RuntimeError("hipMalloc failed")
    one = lambda: hip.hipMemcpy(dev, C.c_void_p(a.ctypes.data), C.c_size_t(a.nbytes), 1)  # hipMemcpyHostToDevice
    one()
    t = med(one)
    hip.hipFree(dev)
    return t


def marg_setup(C, N, rng):
    g = dict(np.load(os.path.join(GOLD, "marg.npz")))
    nx = g["binned_P11l"].shape[-1]
    eng = Engine(EngineConfig(Nl=3), max_batch=C)
    eng.set_template_dims(3, nx)
    T = np.concatenate([g["binned_P11l"], g["binned_Pctl"], g["binned_Ploopl"], g["binned_Pstl"]], axis=1)
    ls = list(g["ls"])
    index = data_index(ls, {l: slice(a, b) for l, (a, b) in zip(ls, g["masks"])}, nx)
    like = MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], g["auto_loc"], g["auto_scale"])
    templ = np.stack([T * (1.0 + 0.01 * c) for c in range(C)])
    f, co = float(g["f"]), g["auto_co"]
    ng = dict(zip(g["auto_ng_names"], g["auto_ng_values"]))
    ngv = np.array([ng["b1"], ng["b2"], ng["b4"]]) + rng.normal(0, 1, (N, 3)) * [0.05, 0.3, 0.3]
    build = lambda: gaussian_rows_many(f, ngv, None, *co[:3])
    rec = joint_draw_recipe([WestCoastBasis(prefix="")], gaussian_params(""), [dict(kmA=float(co[0]), krA=float(co[1]), ndA=float(co[2]))])
    cols = [np.ascontiguousarray(ngv[:, i]) for i in range(3)]  # (a sampler holds one array per parameter)
    lk = (g["auto_D"], g["auto_invcov"], g["auto_loc"], g["auto_scale"], False)  # (data, invcov, loc, scale, jeffreys: the likelihood's own arguments)
    return eng, like, templ, build, index.size, len(g["auto_loc"]), (rec, lambda: np.stack(cols, axis=1), np.full(C, f)), lk


def cfg3_setup(C, N, rng):
    g = dict(np.load(os.path.join(GOLD, "cfg3.npz")))
    nb = max(U.final_templates(g, t)["P11l"].shape[-1] for t in U.TRACERS)
    block = np.zeros((3, 3, 24, nb))
    for i, t in enumerate(U.TRACERS):
        ft = U.final_templates(g, t)
        T = np.concatenate([ft[n] for n in U.NAMES], axis=1)
        block[i, : T.shape[0], :, : T.shape[-1]] = T
    eng = Engine(EngineConfig(Nl=3), max_batch=3 * C)
    eng.set_tracers(3)
    eng.set_template_dims(3, nb)
    index = np.concatenate([data_index([int(l) for l in g[t + "_ls"]], U.masks(g, t), nb, tracer=i, nl=3) for i, t in enumerate(U.TRACERS)])
    names = [str(n) for n in g["full_names"]]
    like = MarginalLikelihood(eng, index, g["data_vector"], g["invcov"], np.zeros(len(names)), np.full(len(names), np.inf), jeffreys=True)
    templ = np.concatenate([block * (1.0 + 0.01 * c) for c in range(C)])
    p = U.params(g)
    draws = {k: np.full(N, v) for k, v in p.items()}
    for k in ("LRG_NGC_b1", "ELG_NGC_b1", "LRG_NGC_c2", "LRG_NGC_c4", "ELG_NGC_c2", "ELG_NGC_c4"):
        draws[k] = p[k] + 0.05 * rng.normal(size=N)
    for t in ("LRG_NGC_", "ELG_NGC_"):
        draws[t + "b2"] = (draws[t + "c2"] + draws[t + "c4"]) / np.sqrt(2.0)
        draws[t + "b4"] = (draws[t + "c2"] - draws[t + "c4"]) / np.sqrt(2.0)
    f = [float(g[t + "_f"]) for t in U.TRACERS]
    build = lambda: joint_gaussian_rows_many(U.bases(), f, draws, names, U.scales(g))
    rec = joint_draw_recipe(U.bases(), names, U.scales(g))
    lk = (g["data_vector"], g["invcov"], np.zeros(len(names)), np.full(len(names), np.inf), True)
    return eng, like, templ, build, index.size, len(names), (rec, lambda: np.stack([draws[n] for n in rec.param_names], axis=1), np.tile(f, (C, 1))), lk


def eval_logp_rate(ntr, ndata_per_tracer, nG, walkers=42):
    """eval_logp walkers / s on the production grid (Nk = 512, resummation + AP), data vector of the same length per tracer"""
    k = synth.survey_kgrid(512)
    cfg = EngineConfig(Nl=3, k=k, with_resum=True, with_ap=True, APst=True, DA_AP=float(synth.da_func(synth.OM_AP, 0.7)), H_AP=float(synth.hubble(synth.OM_AP, 0.7)))
    eng = Engine(cfg, max_batch=walkers * ntr)
    nd = (ndata_per_tracer + 2) // 3
    kdata = np.linspace(0.02, 0.2, nd)
    op = eng.add_operator(TB.compose_operator(3, 512, binning=TB.interp_operator(k, kdata)))
    if ntr > 1:
        eng.set_tracers(ntr, [op] * ntr)
    else:
        eng.set_pipeline_operator(op)
    index = np.concatenate([data_index([0, 2, 4], {}, nd, tracer=t, nl=3) for t in range(ntr)])
    cos = synth.cosmology(z=0.7, Om=0.3, h=0.68)
    B = walkers * ntr
    Pin, f, DA, H = np.stack([cos["Pin"]] * B), np.full(B, cos["f"]), np.full(B, cos["DA"]), np.full(B, cos["H"])
    rng = np.random.default_rng(0)
    data = rng.normal(0, 1, index.size)
    like = MarginalLikelihood(eng, index, data, np.eye(index.size), np.zeros(nG), np.full(nG, 2.0))
    rows = np.zeros((B, nG + 1, 24))
    rows[:, : min(nG, 7) + 1] = gaussian_rows(float(cos["f"]), (2.0, 0.5, 0.3), None, 0.7, 0.25, 4.5e-5)[: min(nG, 7) + 1]
    like.eval_logp(Pin, f, DA, H, rows)
    t = med(lambda: like.eval_logp(Pin, f, DA, H, rows), 10)
    eng.close()
    return walkers / t


def probe(name, setup, C, N, ntr):
    rng = np.random.default_rng(1)
    eng, like, templ, build, ndata, nG, (rec, theta_build, fC), _ = setup(C, N, rng)
    rows = build()
    t_rows = med(build, 3)
    counts = np.full(C, N // C)
    counts[: N % C] += 1
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    t_h2d = h2d_seconds(rows)
    eng.put("TEMPL", templ)
    like.logp_draws(rows[:64], off * 0 + np.minimum(off, 64))  # (first launch of the kernels: code objects loaded)
    eng.put("TEMPL", templ)
    t0 = time.perf_counter()
    like.logp_draws(rows, off)
    t_first = time.perf_counter() - t0
    ts_cached = times(lambda: like.logp_draws(rows, off), 9)
    t_cached = float(np.median(ts_cached))
    # the params path: the same draws as theta [N, P]
    like.set_draw_recipe(rec)
    theta = theta_build()
    t_theta = med(theta_build, 5)
    lp = like.logp_draws_params(theta, off, fC)
    agree = float(np.max(np.abs(lp / like.logp_draws(rows, off) - 1.0)))
    ts_params = times(lambda: like.logp_draws_params(theta, off, fC), 9)
    t_params = float(np.median(ts_params))
    # the gradient call on the same draws
    lpg, grad = like.logp_draws_params(theta, off, fC, grad=True)
    assert np.array_equal(lpg, lp) and grad.shape == theta.shape
    ts_grad = times(lambda: like.logp_draws_params(theta, off, fC, grad=True), 9)
    t_grad = float(np.median(ts_grad))
    # the Hessian call on the same draws
    lph, gradh, hess = like.logp_draws_params(theta, off, fC, grad=True, hess=True)
    assert np.array_equal(lph, lp) and np.array_equal(gradh, grad) and hess.shape == theta.shape + theta.shape[1:]
    ts_hess = times(lambda: like.logp_draws_params(theta, off, fC, grad=True, hess=True), 9)
    t_hess = float(np.median(ts_hess))
    rate_eval = eval_logp_rate(ntr, ndata // ntr, nG)
    out = {
        "shape": name, "walkers": C, "draws": N, "tracers": ntr, "ndata": ndata, "nG": nG, "row_bytes_per_draw": rows[0].nbytes,
        "host_rows_us_per_draw": 1e6 * t_rows / N, "h2d_us_per_draw": 1e6 * t_h2d / N, "gram_ms": 1e3 * (t_first - t_cached),
        "draws_us_per_draw": 1e6 * (t_cached - t_h2d) / N, "call_us_per_draw": 1e6 * t_cached / N,
        "draws_per_s_device_call": N / t_cached, "draws_per_s_end_to_end": N / (t_cached + t_rows),
        "call_us_per_draw_spread": [1e6 * min(ts_cached) / N, 1e6 * max(ts_cached) / N],
        "params_bytes_per_draw": theta[0].nbytes, "params_terms": rec.nterms, "params_theta_us_per_draw": 1e6 * t_theta / N,
        "params_call_us_per_draw": 1e6 * t_params / N, "params_call_us_per_draw_spread": [1e6 * min(ts_params) / N, 1e6 * max(ts_params) / N],
        "params_draws_per_s_device_call": N / t_params, "params_draws_per_s_end_to_end": N / (t_params + t_theta),
        "params_vs_rows_max_rel_diff": agree,
        "grad_bytes_back_per_draw": grad[0].nbytes, "grad_call_us_per_draw": 1e6 * t_grad / N,
        "grad_call_us_per_draw_spread": [1e6 * min(ts_grad) / N, 1e6 * max(ts_grad) / N],
        "grad_draws_per_s_device_call": N / t_grad, "grad_draws_per_s_end_to_end": N / (t_grad + t_theta),
        "grad_cost_in_forward_calls": t_grad / t_params, "central_difference_cost_in_forward_calls": 2 * theta.shape[1],
        "hess_bytes_back_per_draw": hess[0].nbytes, "hess_call_us_per_draw": 1e6 * t_hess / N,
        "hess_call_us_per_draw_spread": [1e6 * min(ts_hess) / N, 1e6 * max(ts_hess) / N],
        "hess_draws_per_s_device_call": N / t_hess, "hess_cost_in_gradient_calls": t_hess / t_grad,
        "central_difference_cost_in_gradient_calls": 2 * theta.shape[1],
        "eval_logp_per_s": rate_eval,
    }
    out["speedup_end_to_end"] = out["draws_per_s_end_to_end"] / rate_eval
    eng.close()
    print(json.dumps(out), flush=True)
    return out


def probe_datasets(name, setup, M, n, repeats=9):
    """(a), (b), (c) of the module docstring for one shape; n draws per group"""
    rng = np.random.default_rng(1)
    eng, like, templ, _, ndata, nG, (rec, theta_build, fC), (data, invcov, loc, scale, jeff) = setup(1, M * n, rng)
    eng.put("TEMPL", templ)
    theta = theta_build()
    chol = np.linalg.cholesky(np.linalg.inv(invcov))
    Ds = np.stack([data] + [data + chol @ np.random.default_rng(100 + m).standard_normal(ndata) for m in range(1, M)])
    off = n * np.arange(M + 1, dtype=np.int64)
    kw = dict(grad=True, hess=True)
    like.set_draw_recipe(rec)
    plain = lambda: like.logp_draws_params(theta, [0, M * n], fC, **kw)
    plain()
    ts_c = times(plain, repeats)
    out = {"shape": name, "datasets": M, "draws_per_group": n, "ndata": ndata, "nG": nG, "P": theta.shape[1],
           "plain_ms": 1e3 * float(np.median(ts_c)), "plain_ms_spread": [1e3 * min(ts_c), 1e3 * max(ts_c)]}
    if hasattr(like, "set_datasets"):
        groups = (np.zeros(M, dtype=np.int32), np.arange(M, dtype=np.int32))
        like.set_datasets(Ds)
        call = lambda: like.logp_draws_params(theta, off, fC, groups=groups, **kw)
        t0 = time.perf_counter()
        got = call()
        t_first = time.perf_counter() - t0
        ts_a = times(call, repeats)
        out.update({"groups_ms": 1e3 * float(np.median(ts_a)), "groups_ms_spread": [1e3 * min(ts_a), 1e3 * max(ts_a)],
                    "groups_first_call_ms": 1e3 * t_first, "groups_Wg_bytes": 8 * M * (eng.ntracers * 24 + 1) ** 2})
        t0 = time.perf_counter()
        like.set_datasets(Ds)
        out["set_datasets_ms"] = 1e3 * (time.perf_counter() - t0)

    def loop():
        res = []
        for m in range(M):
            lk = MarginalLikelihood(eng, like.index, Ds[m], invcov, loc, scale, jeffreys=jeff)
            lk.set_draw_recipe(rec)
            res.append(lk.logp_draws_params(theta[off[m] : off[m + 1]], [0, n], fC, **kw))
        return res

    res = loop()
    if "groups_ms" in out:
        assert all(np.allclose(np.concatenate([r[i] for r in res]), got[i], rtol=1e-9, atol=0) for i in (0,))
    ts_b = times(loop, repeats)
    out.update({"loop_ms": 1e3 * float(np.median(ts_b)), "loop_ms_spread": [1e3 * min(ts_b), 1e3 * max(ts_b)]})
    eng.close()
    print(json.dumps(out), flush=True)
    return out


def probe_samples(name, setup, S_list, N=4096, repeats=9, host_draws=32):
    """(a), (b), (c) of --samples for one shape: one walker x N draws, medians of `repeats` cached calls with [min, max]"""
    rng = np.random.default_rng(1)
    eng, like, templ, _, ndata, nG, (rec, theta_build, fC), (data, invcov, loc, scale, jeff) = setup(1, N, rng)
    eng.put("TEMPL", templ)
    theta = theta_build()
    off = [0, N]
    like.set_draw_recipe(rec)
    stat = lambda ts: {"ms": 1e3 * float(np.median(ts)), "ms_spread": [1e3 * min(ts), 1e3 * max(ts)]}
    out = {"shape": name, "draws": N, "ndata": ndata, "nG": nG, "P": theta.shape[1]}
    for key, kw in (("floor", dict(return_best=True)), ("grad", dict(grad=True)), ("hess", dict(grad=True, hess=True))):
        call = lambda: like.logp_draws_params(theta, off, fC, **kw)
        call()
        out[key] = stat(times(call, repeats))
    if hasattr(like, "sample_gaussian_params"):
        import grad_util as GU
        import sample_util as SU

        for S in S_list:
            z = np.random.default_rng(S).standard_normal((N, S, nG))
            for predict in (False, True):
                call = lambda: like.sample_gaussian_params(theta, off, fC, z, predict=predict)
                call()
                r = stat(times(call, repeats))
                r["over_floor"] = r["ms"] / out["floor"]["ms"]
                out["samples_S%d%s" % (S, "_predict" if predict else "")] = r
        # what a user has today: the templates on the host, and per draw V, F2, a Cholesky factor and the samples in NumPy
        ntr = eng.ntracers
        nl, nx = eng.dims
        th = eng.get("TEMPL", (ntr, nl, 24, nx))
        S = S_list[-1] if len(S_list) < 2 else S_list[1]
        z = np.random.default_rng(S).standard_normal((host_draws, S, nG))
        ff = np.reshape(fC, (1, ntr))[0]
        t0 = time.perf_counter()
        for d in range(host_draws):
            SU.data_space_samples(GU.model_vectors(rec.rows(theta[d : d + 1], ff[None])[0], th, like.index), data, invcov, loc, scale, z[d], jeffreys=jeff)
        t = (time.perf_counter() - t0) / host_draws * N
        out["numpy_S%d" % S] = {"ms": 1e3 * t, "timed_draws": host_draws, "device_call_speedup": 1e3 * t / out["samples_S%d" % S]["ms"]}
    eng.close()
    print(json.dumps(out), flush=True)
    return out


def probe_chains(name, setup, C, n, T, repeats=9):
    """(a), (b), (c) of --chains for one shape: C walkers x n chains x T steps, medians of `repeats` cached calls with [min, max]"""
    rng = np.random.default_rng(1)
    N = C * n
    eng, like, templ, _, ndata, nG, (rec, theta_build, fC), _ = setup(C, N, rng)
    eng.put("TEMPL", templ)
    theta0 = theta_build()
    P = theta0.shape[1]
    off = np.arange(C + 1) * n
    like.set_draw_recipe(rec)
    step = 0.3 * (theta_build() - np.median(theta0, axis=0))[:, None, :] * rng.standard_normal((N, T, 1)) + 0.01 * rng.standard_normal((N, T, P))
    lnu = np.log(rng.random((N, T)))
    stat = lambda ts: {"ms": 1e3 * float(np.median(ts)), "ms_spread": [1e3 * min(ts), 1e3 * max(ts)]}
    out = {"shape": name, "walkers": C, "chains": N, "steps": T, "ndata": ndata, "nG": nG, "P": P}

    def loop():
        cur = theta0.copy()
        lp = like.logp_draws_params(cur, off, fC)
        nacc = np.zeros(N, dtype=np.int64)
        for t in range(T):
            trial = cur + step[:, t]
            try:
                lp1 = like.logp_draws_params(trial, off, fC)
            except RuntimeError:  # det F2 <= 0 at a proposal: the public call has no NaN to give, the step is lost for all chains
                lp1, out["loop_hit_nan"] = np.full(N, np.nan), True
            acc = np.isfinite(lp1) & (lnu[:, t] < lp1 - lp)
            cur[acc], lp[acc] = trial[acc], lp1[acc]
            nacc += acc
        return cur, nacc

    last, nacc = loop()
    out["accept_rate"] = float(np.mean(nacc)) / T
    out["loop"] = stat(times(loop, repeats))
    many = np.ascontiguousarray((theta0[:, None, :] + step).reshape(N * T, P))
    ceiling = lambda: like.logp_draws_params(many, off * T, fC)
    ceiling()
    out["ceiling"] = stat(times(ceiling, repeats))
    if hasattr(like, "metropolis_draws_params"):
        call = lambda: like.metropolis_draws_params(theta0, off, fC, step, lnu)
        r = call()
        assert "loop_hit_nan" in out or (np.array_equal(r.last, last) and np.array_equal(r.naccept, nacc))  # the same chains as the loop
        out["chains"] = stat(times(call, repeats))
        out["loop_over_chains"] = out["loop"]["ms"] / out["chains"]["ms"]
        out["chains_over_ceiling"] = out["chains"]["ms"] / out["ceiling"]["ms"]
        out["steps_per_s"] = N * T / (1e-3 * out["chains"]["ms"])
    eng.close()
    print(json.dumps(out), flush=True)
    return out


def probe_drag(name, setup, G, n, T, repeats=9):
    """(a) and (b) of --drag for one shape: G pairs x n chains x T steps, medians of `repeats` cached calls with [min, max]"""
    rng = np.random.default_rng(1)
    N, C = G * n, 2 * G
    eng, like, templ, _, ndata, nG, (rec, theta_build, fC), _ = setup(C, N, rng)
    eng.put("TEMPL", templ)
    theta0 = theta_build()
    P = theta0.shape[1]
    counts = np.repeat([n, 0], G)
    off_a, off_b = np.concatenate([[0], np.cumsum(counts)]), np.concatenate([[0], np.cumsum(counts[::-1])])  # the chains at their start and at their end walkers
    fC = np.ascontiguousarray(fC * (1.0 + 0.02 * (np.arange(C) >= G)).reshape((C,) + (1,) * (np.ndim(fC) - 1)))  # the end walkers have their own growth rates
    like.set_draw_recipe(rec)
    step = 0.3 * (theta_build() - np.median(theta0, axis=0))[:, None, :] * rng.standard_normal((N, T, 1)) + 0.01 * rng.standard_normal((N, T, P))
    lnu = np.log(rng.random((N, T)))
    frac = np.arange(1, T + 1) / (T + 1)
    stat = lambda ts: {"ms": 1e3 * float(np.median(ts)), "ms_spread": [1e3 * min(ts), 1e3 * max(ts)]}
    out = {"shape": name, "pairs": G, "chains": N, "steps": T, "ndata": ndata, "nG": nG, "P": P}

    def both(theta):
        try:
            return like.logp_draws_params(theta, off_a, fC), like.logp_draws_params(theta, off_b, fC)
        except RuntimeError:  # det F2 <= 0 at a proposal: the public call has no NaN to give, the step is lost for all chains
            out["loop_hit_nan"] = True
            return np.full(N, np.nan), np.full(N, np.nan)

    def loop():
        cur = theta0.copy()
        la, lb = both(cur)
        sa, sb = la + 0.0, lb + 0.0
        nacc = np.zeros(N, dtype=np.int64)
        for t in range(T):
            trial = cur + step[:, t]
            la1, lb1 = both(trial)
            u = 1.0 - frac[t]
            acc = np.isfinite(la1) & np.isfinite(lb1) & (lnu[:, t] < (u * la1 + frac[t] * lb1) - (u * la + frac[t] * lb))
            cur[acc], la[acc], lb[acc] = trial[acc], la1[acc], lb1[acc]
            nacc += acc
            sa, sb = sa + la, sb + lb
        return cur, nacc, sa, sb

    last, nacc, sa, sb = loop()
    out["accept_rate"] = float(np.mean(nacc)) / T
    out["loop"] = stat(times(loop, repeats))
    if hasattr(like, "drag_draws_params"):
        pairs = (np.arange(G), G + np.arange(G))
        call = lambda: like.drag_draws_params(theta0, np.arange(G + 1) * n, fC, pairs, step, lnu)
        r = call()
        if "loop_hit_nan" not in out:  # the same chains as the loop
            assert np.array_equal(r.last, last) and np.array_equal(r.naccept, nacc) and np.array_equal(r.sum_start, sa) and np.array_equal(r.sum_end, sb)
        out["drag"] = stat(times(call, repeats))
        out["loop_over_drag"] = out["loop"]["ms"] / out["drag"]["ms"]
        out["steps_per_s"] = N * T / (1e-3 * out["drag"]["ms"])
        out["mean_log_ratio"] = float(np.mean(r.log_ratio))
    eng.close()
    print(json.dumps(out), flush=True)
    return out


def probe_hmc(name, setup, C, n, evals, nleap, eps, repeats=9):
    """(a), (b), (c) of --hmc for one shape: C walkers x n chains x evals / nleap trajectories of nleap steps, medians with [min, max]"""
    import hmc_util as HM

    rng = np.random.default_rng(1)
    N, T = C * n, max(1, evals // nleap)
    eng, like, templ, _, ndata, nG, (rec, theta_build, fC), _ = setup(C, N, rng)
    eng.put("TEMPL", templ)
    theta0 = theta_build()
    P = theta0.shape[1]
    off = np.arange(C + 1) * n
    like.set_draw_recipe(rec)
    mom, lnu = rng.standard_normal((N, T, P)), np.log(rng.random((N, T)))
    epsa = eps * rng.uniform(0.8, 1.2, (N, T))
    stat = lambda ts: {"ms": 1e3 * float(np.median(ts)), "ms_spread": [1e3 * min(ts), 1e3 * max(ts)]}
    out = {"shape": name, "walkers": C, "chains": N, "trajectories": T, "nleap": nleap, "eps": eps, "ndata": ndata, "nG": nG, "P": P}

    import ctypes as ct

    from eftpipe_amd import _lib as L

    o64, fo = np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(fC, dtype=np.float64)
    lp, gr = np.empty(N), np.empty((N, P))

    def grad(theta):  # eftb_draws_logp_grad_params itself: logp_draws_params(grad=True) raises where a draw has det F2 <= 0, the library returns NaN there
        L.check(eng.lib.eftb_draws_logp_grad_params(eng._h, C, N, o64.ctypes.data_as(ct.POINTER(ct.c_int64)), L.dptr(np.ascontiguousarray(theta)), L.dptr(fo),
                                                    L.dptr(lp), L.dptr(gr), None, None))
        return lp.copy(), gr.copy()

    loop = lambda: HM.host_hmc(grad, theta0, mom, lnu, epsa, nleap)
    want = loop()
    out["accept_rate"] = float(np.mean(want["naccept"])) / T
    out["aborted"] = int(np.sum(want["aborted"]))
    out["loop"] = stat(times(loop, repeats))
    many = np.ascontiguousarray(np.repeat(theta0, T * nleap, axis=0))
    ceiling = lambda: like.logp_draws_params(many, off * T * nleap, fC, grad=True)
    ceiling()
    out["ceiling"] = stat(times(ceiling, repeats))
    if hasattr(like, "hmc_draws_params"):
        call = lambda: like.hmc_draws_params(theta0, off, fC, mom, lnu, epsa, nleap, return_ratio=True)
        r = call()
        assert np.array_equal(r.last, want["last"]) and np.array_equal(r.naccept, want["naccept"])  # the same chains as the loop
        assert np.array_equal(r.theta, want["theta"]) and np.array_equal(r.log_ratio, want["log_ratio"], equal_nan=True)
        out["hmc"] = stat(times(call, repeats))
        out["loop_over_hmc"] = out["loop"]["ms"] / out["hmc"]["ms"]
        out["hmc_over_ceiling"] = out["hmc"]["ms"] / out["ceiling"]["ms"]
        out["evaluations_per_s"] = N * T * nleap / (1e-3 * out["hmc"]["ms"])
        out["us_per_evaluation_per_wave"] = 1e3 * out["hmc"]["ms"] / (T * nleap + 1) if n == 1 else None  # (one chain per workgroup: its wave runs alone)
    eng.close()
    print(json.dumps(out), flush=True)
    return out


def probe_temper(name, setup, C, nlad, R=4, T=256, S=4, repeats=9):
    """(a), (b), (c) of --temper for one shape: C walkers x nlad ladders of R rungs x T steps with a swap event every S, medians of `repeats`
    cached calls with [min, max].  (b), the only route without the tempering call, runs on a tree that lacks it too"""
    rng = np.random.default_rng(1)
    N = C * nlad * R
    eng, like, templ, _, ndata, nG, (rec, theta_build, fC), _ = setup(C, N, rng)
    eng.put("TEMPL", templ)
    theta0 = theta_build()
    P = theta0.shape[1]
    off = np.arange(C + 1) * nlad * R
    like.set_draw_recipe(rec)
    beta = 0.1 ** (np.arange(R) / max(R - 1, 1))  # (temper_ladder(R, 0.1), spelled out for the tree without it)
    bt = np.tile(beta, N // R)
    step = 0.3 * (theta_build() - np.median(theta0, axis=0))[:, None, :] * rng.standard_normal((N, T, 1)) + 0.01 * rng.standard_normal((N, T, P))
    step = np.ascontiguousarray(step / np.sqrt(bt)[:, None, None])
    lnu = np.log(rng.random((N, T)))
    lnus = np.log(rng.random((N // R, T // S, R - 1)))
    stat = lambda ts: {"ms": 1e3 * float(np.median(ts)), "ms_spread": [1e3 * min(ts), 1e3 * max(ts)]}
    out = {"shape": name, "walkers": C, "ladders": N // R, "rungs": R, "steps": T, "swap_every": S, "ndata": ndata, "nG": nG, "P": P}
    # (b) T / S chain calls of S steps, the swaps in NumPy between them.  The chain call has no temperature: without a Gaussian prior on theta,
    # lnu / beta < ln P' - ln P is the tempered rule up to the rounding of one product
    lnu_b = lnu / bt[:, None]
    base = np.arange(N // R) * R

    def loop():
        cur, nswap = theta0, np.zeros((N // R, R - 1), dtype=np.int64)
        for j in range(T // S):
            r = like.metropolis_draws_params(cur, off, fC, np.ascontiguousarray(step[:, j * S : (j + 1) * S]), np.ascontiguousarray(lnu_b[:, j * S : (j + 1) * S]))
            cur, lp = r.last, r.logp[:, -1]
            for q in range(j % 2, R - 1, 2):
                lo, hi = base + q, base + q + 1
                sw = lnus[:, j, q] < (beta[q] - beta[q + 1]) * (lp[hi] - lp[lo])
                a, b = lo[sw], hi[sw]
                cur[a], cur[b] = cur[b].copy(), cur[a].copy()
                nswap[:, q] += sw
        return cur, nswap

    last, nswap = loop()
    out["swap_rate"] = (nswap.sum(0) / ((T // S + 1 - np.arange(R - 1) % 2) // 2 * (N // R))).tolist()
    out["loop"] = stat(times(loop, repeats))
    plain = lambda: like.metropolis_draws_params(theta0, off, fC, step, lnu)  # (c) the same N T steps without a swap or a barrier
    plain()
    out["chains"] = stat(times(plain, repeats))
    if hasattr(like, "temper_draws_params"):
        call = lambda: like.temper_draws_params(theta0, off, fC, beta, step, lnu, lnus, swap_every=S)
        r = call()
        assert np.array_equal(r.last, last) and np.array_equal(r.nswap, nswap)  # the same ladders as the loop
        out["accept_rate"] = (r.naccept.reshape(-1, R).mean(0) / T).tolist()
        out["temper"] = stat(times(call, repeats))
        out["loop_over_temper"] = out["loop"]["ms"] / out["temper"]["ms"]
        out["temper_over_chains"] = out["temper"]["ms"] / out["chains"]["ms"]
        out["steps_per_s"] = N * T / (1e-3 * out["temper"]["ms"])
    eng.close()
    print(json.dumps(out), flush=True)
    return out


def probe_ensemble(name, setup, C, nens, K=8, T=256, a=2.0, repeats=9):
    """(a), (b), (c) of --ensemble for one shape: C walkers x nens ensembles of K members x T sweeps, medians of `repeats` cached calls with
    [min, max].  (b), the only route without the ensemble call, runs on a tree that lacks it too"""
    rng = np.random.default_rng(1)
    N, half = C * nens * K, K // 2
    eng, like, templ, _, ndata, nG, (rec, theta_build, fC), _ = setup(C, N, rng)
    eng.put("TEMPL", templ)
    theta0 = theta_build()
    P = theta0.shape[1]
    off = np.arange(C + 1) * nens * K
    like.set_draw_recipe(rec)
    # (stretch_proposals(rng, C nens, K, T, P, a), spelled out for the tree without it)
    z = ((a - 1.0) * rng.random((N, T)) + 1.0) ** 2 / a
    pick = rng.integers(half, size=(N, T)).astype(np.int32)
    lnq = np.log(rng.random((N, T))) - (P - 1) * np.log(z)
    stat = lambda ts: {"ms": 1e3 * float(np.median(ts)), "ms_spread": [1e3 * min(ts), 1e3 * max(ts)]}
    out = {"shape": name, "walkers": C, "ensembles": N // K, "members": K, "sweeps": T, "ndata": ndata, "nG": nG, "P": P}
    n = np.arange(N)
    halves = [n[n % K // half == h] for h in (0, 1)]  # the chains of each half, in chain order: half the chains of every walker
    base = n // K * K

    def loop():
        cur = theta0.copy()
        lp = like.logp_draws_params(cur, off, fC)
        nacc = np.zeros(N, dtype=np.int64)
        for t in range(T):
            for h in (0, 1):
                act = halves[h]
                tj = cur[base[act] + (1 - h) * half + pick[act, t]]
                d = cur[act] - tj
                trial = tj + z[act, t, None] * d
                try:
                    lp1 = like.logp_draws_params(trial, off // 2, fC)
                except RuntimeError:  # det F2 <= 0 at a proposal: the public call has no NaN to give, the half-sweep is lost for all chains
                    lp1, out["loop_hit_nan"] = np.full(act.size, np.nan), True
                acc = np.isfinite(lp1) & (lnq[act, t] < lp1 - lp[act])
                cur[act[acc]], lp[act[acc]] = trial[acc], lp1[acc]
                nacc[act] += acc
        return cur, nacc

    last, nacc = loop()
    out["accept_rate"] = float(np.mean(nacc)) / T
    out["loop"] = stat(times(loop, repeats))
    step = 0.01 * rng.standard_normal((N, T, P))
    lnu = np.log(rng.random((N, T)))
    plain = lambda: like.metropolis_draws_params(theta0, off, fC, step, lnu)  # (c) the same N T evaluations without a barrier
    plain()
    out["chains"] = stat(times(plain, repeats))
    if hasattr(like, "ensemble_draws_params"):
        call = lambda: like.ensemble_draws_params(theta0, off, fC, K, z, pick, lnq)
        r = call()
        # the same ensembles as the loop -- unless the loop lost a half-sweep to a NaN proposal, which the result then says
        out["same_as_loop"] = None if "loop_hit_nan" in out else bool(np.array_equal(r.last, last) and np.array_equal(r.naccept, nacc))
        assert out["same_as_loop"] is not False
        if out["same_as_loop"] is None:
            print("draws_probe: the loop met det F2 <= 0 at a proposal; (a) was NOT compared with (b) at this shape", flush=True)
        out["ensemble"] = stat(times(call, repeats))
        out["loop_over_ensemble"] = out["loop"]["ms"] / out["ensemble"]["ms"]
        out["ensemble_over_chains"] = out["ensemble"]["ms"] / out["chains"]["ms"]
        out["evaluations_per_s"] = N * T / (1e-3 * out["ensemble"]["ms"])
    eng.close()
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ensemble", nargs="?", const="1,4", default=None,
                    help="n[,n...] ensembles of eight members per walker (default 1,4): time ensemble_draws_params, the loop of 2 x steps "
                         "logp_draws_params calls with the rule in NumPy on the same inputs, and one chain call of as many evaluations")
    ap.add_argument("--temper", nargs="?", const="1,4", default=None,
                    help="n[,n...] ladders of four rungs per walker (default 1,4), a swap event every fourth step: time temper_draws_params, the loop of "
                         "steps / 4 metropolis_draws_params calls with the swaps in NumPy on the same inputs, and one chain call of as many steps")
    ap.add_argument("--chains", nargs="?", const="1,8", default=None,
                    help="n[,n...] chains per walker (default 1,8): time metropolis_draws_params, the host loop of logp_draws_params calls on the same "
                         "proposals and one logp_draws_params call on as many independent draws")
    ap.add_argument("--drag", nargs="?", const="1,8", default=None,
                    help="n[,n...] chains per pair of walkers (default 1,8): time drag_draws_params and the host loop of two logp_draws_params calls per step "
                         "on the same proposals")
    ap.add_argument("--hmc", nargs="?", const="1,8", default=None,
                    help="n[,n...] chains per walker (default 1,8): time hmc_draws_params, the host loop of logp_draws_params(grad=True) calls on the same "
                         "inputs and one gradient call on as many independent draws")
    ap.add_argument("--leap", type=int, default=8, help="leapfrog steps per trajectory of --hmc")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--samples", nargs="?", const="1,8,64", default=None,
                    help="S[,S...] samples of the marginalised parameters per draw (default 1,8,64): time sample_gaussian_params with and without predict, the "
                         "logp / gradient / Hessian calls on the same draws and the NumPy route on fetched templates")
    ap.add_argument("--draws", type=int, default=None)
    ap.add_argument("--walkers", type=int, default=None)
    ap.add_argument("--datasets", type=int, default=0, help="M data vectors sharing the covariance: time the groups call, the per-vector loop and the plain call")
    a = ap.parse_args()
    if a.ensemble:
        for n in (int(x) for x in a.ensemble.split(",")):
            probe_ensemble("marg", marg_setup, a.walkers or 128, n, T=a.steps)
            probe_ensemble("cfg3", cfg3_setup, a.walkers or 128, n, T=a.steps)
    elif a.temper:
        for n in (int(x) for x in a.temper.split(",")):
            probe_temper("marg", marg_setup, a.walkers or 128, n, T=a.steps)
            probe_temper("cfg3", cfg3_setup, a.walkers or 128, n, T=a.steps)
    elif a.hmc:
        for n in (int(x) for x in a.hmc.split(",")):
            probe_hmc("marg", marg_setup, a.walkers or 128, n, a.steps, a.leap, 0.01)
            probe_hmc("cfg3", cfg3_setup, a.walkers or 128, n, a.steps, a.leap, 0.01)
    elif a.drag:
        for n in (int(x) for x in a.drag.split(",")):
            probe_drag("marg", marg_setup, a.walkers or 128, n, a.steps)
            probe_drag("cfg3", cfg3_setup, a.walkers or 128, n, a.steps)
    elif a.chains:
        for n in (int(x) for x in a.chains.split(",")):
            probe_chains("marg", marg_setup, a.walkers or 128, n, a.steps)
            probe_chains("cfg3", cfg3_setup, a.walkers or 128, n, a.steps)
    elif a.samples:
        S_list = [int(s) for s in a.samples.split(",")]
        probe_samples("marg", marg_setup, S_list, a.draws or 4096)
        probe_samples("cfg3", cfg3_setup, S_list, a.draws or 4096)
    elif a.datasets:
        probe_datasets("marg", marg_setup, a.datasets, a.draws or 1024)
        probe_datasets("cfg3", cfg3_setup, a.datasets, a.draws or 1024)
    else:
        probe("marg", marg_setup, a.walkers or 32, a.draws or 32768, 1)
        probe("cfg3", cfg3_setup, a.walkers or 32, a.draws or 32768, 3)
