"""Bit-for-bit A/B of two builds of the library (GPU box), beside ab_lib.sh which compares their speed.

    EFTB_LIB=other.so python3 tools/ab_bits.py dump OUT.npz    every output array of a fixed list of small seeded cases, on the library EFTB_LIB names
    python3 tools/ab_bits.py cmp A.npz B.npz                   exit status 1 unless both hold the same arrays, array_equal each

One dump per process: _lib.py reads EFTB_LIB once, when it is loaded.  The kernels use integer atomics only (status flags, a min / max in
ap_weights_kernel), so a build must reproduce itself, and a host-side refactor its parent, in every case.  Each case names the arm it is there
for -- of the stage launcher (launch_stages_impl) or of the staged launch around it (issue_group: every value of PlkExit,
both completion rules, both issuing threads, both upload streams, per-step destinations, the GROWS upload), or the
buffers an engine replaces while it lives; shapes are the smallest that reach the arm."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from eftpipe_amd import _lib as L  # noqa: E402
from eftpipe_amd import synth  # noqa: E402
from eftpipe_amd.engine import Engine  # noqa: E402
from eftpipe_amd.parambasis import bias_row  # noqa: E402
from eftpipe_amd.tables import EngineConfig  # noqa: E402

Z = 0.7
BS, ES = [2.14, 0.55, 0.77, 0.55, -1.84, -1.89, -1.49], (0.26, 0.0, -0.93)


def cfg(**kw):
    base = dict(Nl=3, with_resum=True, with_ap=True, DA_AP=float(synth.da_func(synth.OM_AP, Z)), H_AP=float(synth.hubble(synth.OM_AP, Z)))
    base.update(kw)
    return EngineConfig(**base)


def draws(B, seed, kin=None):
    d = synth.draw_batch(B, z=Z, seed=seed)
    rng = np.random.default_rng(seed)
    if kin is not None:  # another input grid: the same shapes of P_lin on it
        d["Pin"] = np.stack([(1.0 + 0.1 * rng.uniform(-1, 1)) * synth.plin(kin) for _ in range(B)])
    d["bias"] = np.stack([bias_row(float(f), list(np.asarray(BS) * (1.0 + 0.2 * rng.standard_normal(7))), None, ES, kmA=0.7, krA=0.25, ndA=4.5e-5)
                          for f in d["f"]])
    d["biasn"] = 0.1 * rng.standard_normal((B, 3))
    return d


def thin(eng, step, nl_out=3):  # an operator that keeps every step-th k (and the first nl_out multipoles)
    return np.einsum("al,xk->alxk", np.eye(3)[:nl_out, :eng.Nl], np.eye(eng.Nk)[::step])


def sync_eval(B, max_batch, direct=False, ops=None, tracers=0, nnlo=False, **kw):
    """eval_batch on a fresh engine -> templates (templates-first runs), P_l, the NNLO block"""
    def run():
        eng, d = Engine(cfg(with_NNLO=nnlo, **kw), max_batch=max_batch), draws(B, 7, kw.get("kin"))
        ids = [eng.add_operator(o(eng)) if callable(o) else eng.add_operator(o[0](eng), stochastic=o[1](eng)) for o in (ops or [])]
        if tracers:
            eng.set_tracers(tracers, ids)
        elif ids:
            eng.set_pipeline_operator(ids[0])
        eng.set_plk_direct(direct)
        out = eng.eval_batch(d["Pin"], d["f"], d["DA"], d["H"], bias=d["bias"], templates=not direct, bias_nnlo=d["biasn"] if nnlo else None)
        out = [out] if direct else list(out)
        if nnlo:
            nl, nx = eng.out_dims()
            out.append(eng.get("TEMPLN", (B, nl, 24, nx)))
        eng.close()
        return out
    return run


def async_runs(B, nrun=4, direct=False, nnlo=False, **kw):
    """back-to-back run(mask, sync=False) on settled inputs -> P_l, templates, the NNLO block"""
    def run():
        eng, d = Engine(cfg(with_NNLO=nnlo, **kw), max_batch=B), draws(B, 11, kw.get("kin"))
        eng.set_plk_direct(direct)
        eng.load_inputs(d["Pin"], d["f"], d["DA"], d["H"], d["bias"])
        if nnlo:
            eng.put("BIASN", d["biasn"])
        for _ in range(nrun):
            eng.run(eng.full_mask(reduce=True), B, sync=False)
        out = [eng.get("PLK", (B, 3, eng.Nk))] + ([] if direct else [eng.get("TEMPL", (B, 3, 24, eng.Nk))])
        if nnlo:
            out.append(eng.get("TEMPLN", (B, 3, 24, eng.Nk)))
        eng.close()
        return out
    return run


def staged_direct():
    """the loop of test_staged_direct_loop_under_each_switch: B = 16, K = 14, depth 6, coalesce 3, then one latency-mode step"""
    import bench
    B, K, depth, shape = 16, 14, 6, (16, bench.NL, bench.NK)
    eng = Engine(cfg(k=synth.survey_kgrid(bench.NK)), max_batch=B, coalesce=3)
    eng.set_plk_direct(True)
    eng.set_latency_mode(False)
    mask, sets, got = eng.full_mask(reduce=True), [draws(B, 820 + i) for i in range(3)], []
    for i in range(K):
        s = sets[i % 3]
        view = eng.step(mask, s["Pin"], s["f"], s["DA"], s["H"], bias=s["bias"], back=depth if i >= depth else -1, shape=shape)
        if i >= depth:
            got.append(view.copy())
    got += [eng.fetch_previous("PLK", shape, back=back) for back in range(depth - 1, -1, -1)]
    eng.set_latency_mode(True)
    eng.sync()
    s = sets[0]
    eng.stage_inputs(s["Pin"], s["f"], s["DA"], s["H"], bias=s["bias"])
    eng.run_staged(mask, B)
    got.append(eng.fetch_previous("PLK", shape, back=0))
    eng.close()
    return got


def staged_engine(B, nk=None, direct=True):
    import bench
    eng = Engine(cfg(k=synth.survey_kgrid(nk or bench.NK)), max_batch=B, coalesce=3)
    eng.set_plk_direct(direct)
    eng.set_latency_mode(False)
    return eng, eng.full_mask(reduce=True), (B, bench.NL, nk or bench.NK)


def held_launch(eng, mask, steps, outs):
    """the steps leave as ONE launch (the submission thread is held while they are queued), step i into outs[i] (None: the set's own block)"""
    eng.set_submit_thread(2)
    eng.hold_submissions(True)
    for s, out in zip(steps, outs):
        eng.step(mask, s["Pin"], s["f"], s["DA"], s["H"], bias=s["bias"], out=out)
    eng.hold_submissions(False)


def staged_outputs():
    """eftb_set_step_output: launches of three steps whose destinations follow each other in memory (one transfer), leave a gap (one each),
    have a step without a destination between them; then a free-running loop, every step into its own slice"""
    B, K, depth = 16, 12, 4
    eng, mask, shape = staged_engine(B)
    sets, dest, got = [draws(B, 830 + i) for i in range(3)], eng.pinned_empty((K,) + shape), []
    for slots in ((0, 1, 2), (3, 5, 7), (8, None, 9)):
        dest.fill(-1.0)
        held_launch(eng, mask, sets, [None if j is None else dest[j] for j in slots])
        got += [eng.fetch_previous("PLK", shape, back=2 - i) for i in range(3)] + [dest.copy()]
    dest.fill(-1.0)
    eng.set_submit_thread(1)
    for i in range(K):
        s = sets[i % 3]
        eng.step(mask, s["Pin"], s["f"], s["DA"], s["H"], bias=s["bias"], back=depth if i >= depth else -1, shape=shape, out=dest[i])
    for back in range(depth - 1, -1, -1):
        eng.fetch_previous("PLK", shape, back=back, copy=False)
    got.append(dest.copy())
    eng.close()
    return got


def staged_odd():
    """odd nx and an odd batch: the later steps of a launch start at addresses that are only 8-byte aligned (EFTB_PLK_DMA=0: copy8_kernel)"""
    import bench
    B, K, depth = 5, 12, 4
    eng, mask, shape = staged_engine(B, nk=bench.NK - 1)
    sets, dest, got = [draws(B, 840 + i) for i in range(3)], eng.pinned_empty((3,) + shape), []
    held_launch(eng, mask, sets, [None] * 3)
    got += [eng.fetch_previous("PLK", shape, back=2 - i) for i in range(3)]
    dest.fill(-1.0)
    held_launch(eng, mask, sets, [dest[2], dest[0], dest[1]])
    got += [eng.fetch_previous("PLK", shape, back=2 - i) for i in range(3)] + [dest.copy()]
    eng.set_submit_thread(1)
    for i in range(K):
        s = sets[i % 3]
        view = eng.step(mask, s["Pin"], s["f"], s["DA"], s["H"], bias=s["bias"], back=depth if i >= depth else -1, shape=shape)
        if i >= depth:
            got.append(view.copy())
    got += [eng.fetch_previous("PLK", shape, back=back) for back in range(depth - 1, -1, -1)]
    eng.close()
    return got


def staged_templates_first():
    """the staged loop with set_plk_direct(False): P_l leaves through the copy behind the back half, which the next join waits for"""
    B, K, depth = 16, 12, 4
    eng, mask, shape = staged_engine(B, direct=False)
    sets, got = [draws(B, 850 + i) for i in range(3)], []
    for i in range(K):
        s = sets[i % 3]
        view = eng.step(mask, s["Pin"], s["f"], s["DA"], s["H"], bias=s["bias"], back=depth if i >= depth else -1, shape=shape)
        if i >= depth:
            got.append(view.copy())
    got += [eng.fetch_previous("PLK", shape, back=back) for back in range(depth - 1, -1, -1)]
    eng.close()
    return got


def staged_logp():
    """a staged LOGP loop: every step brings its likelihood rows (the GROWS segment of the upload), ln P fetched from the set's mapped block"""
    from eftpipe_amd.marginal import MarginalLikelihood
    B, K, depth, nG = 4, 12, 3, 5
    eng, rng = Engine(cfg(), max_batch=B, coalesce=3), np.random.default_rng(23)
    eng.set_pipeline_operator(eng.add_operator(thin(eng, 2)))
    index = np.arange(0, 3 * eng.out_dims()[1], 4)
    A = 0.03 * rng.standard_normal((index.size, index.size))
    MarginalLikelihood(eng, index, 1e3 * rng.standard_normal(index.size), 1e-6 * (np.eye(index.size) + A @ A.T), np.zeros(nG), np.full(nG, 2.0))
    sets = [draws(n, 860 + n) for n in (4, 3, 1)]
    for s in sets:
        s["rows"] = np.concatenate([s["bias"][:, None, :], 0.1 * rng.standard_normal((s["bias"].shape[0], nG, 24))], axis=1)
    mask, got = eng.full_mask() | L.S_LOGP, []
    eng.set_latency_mode(False)
    eng.set_submit_thread(2)
    eng.hold_submissions(True)
    for s in sets:
        eng.step(mask, s["Pin"], s["f"], s["DA"], s["H"], rows=s["rows"])
    eng.hold_submissions(False)
    got += [eng.fetch_previous("LOGP", (sets[i]["f"].size, 26), back=2 - i) for i in range(3)]
    eng.set_submit_thread(1)
    size = lambda i: sets[i % 3]["f"].size
    for i in range(K):
        s = sets[i % 3]
        view = eng.step(mask, s["Pin"], s["f"], s["DA"], s["H"], rows=s["rows"], back=depth if i >= depth else -1, fetch="LOGP", shape=(size(i - depth), 26))
        if i >= depth:
            got.append(view.copy())
    got += [eng.fetch_previous("LOGP", (size(K - 1 - back), 26), back=back) for back in range(depth - 1, -1, -1)]
    eng.close()
    return got


def logp_tracers():
    """eval_logp with two tracers per walker (marg_build, U = V C^-1, marg_solve)"""
    from eftpipe_amd.marginal import MarginalLikelihood
    B, ntr, nG = 4, 2, 5
    eng, d, rng = Engine(cfg(), max_batch=B), draws(B, 13), np.random.default_rng(13)
    eng.set_tracers(ntr, [eng.add_operator(thin(eng, 2)), eng.add_operator(thin(eng, 2) * 0.9)])
    nx = eng.out_dims()[1]
    index = np.arange(0, ntr * 3 * nx, 4)
    rows = np.concatenate([d["bias"][:, None, :], 0.1 * rng.standard_normal((B, nG, 24))], axis=1)
    A = 0.03 * rng.standard_normal((index.size, index.size))
    like = MarginalLikelihood(eng, index, 1e3 * rng.standard_normal(index.size), 1e-6 * (np.eye(index.size) + A @ A.T), np.zeros(nG), np.full(nG, 2.0))
    out = list(like.eval_logp(d["Pin"], d["f"], d["DA"], d["H"], rows, return_best=True))
    eng.close()
    return out


def draws_engine(B=4, nG=3, step=4, seed=31):
    """templates of B seeded cosmologies in the block, and a likelihood over every step-th point of it with nG marginalised parameters"""
    from eftpipe_amd.marginal import MarginalLikelihood
    eng, d, rng = Engine(cfg(), max_batch=B), draws(B, seed), np.random.default_rng(seed)
    eng.eval_batch(d["Pin"], d["f"], d["DA"], d["H"])

    def likelihood(step):
        index = np.arange(0, 3 * eng.Nk, step)
        A = 0.03 * rng.standard_normal((index.size, index.size))
        return MarginalLikelihood(eng, index, 1e3 * rng.standard_normal(index.size), 1e-6 * (np.eye(index.size) + A @ A.T), np.zeros(nG), np.full(nG, 2.0))
    return eng, d, rng, likelihood, likelihood(step)


def recipe(names=("cct", "cr1", "cr2"), kmA=0.7):
    from eftpipe_amd.marginal import joint_draw_recipe
    from eftpipe_amd.parambasis import WestCoastBasis
    return joint_draw_recipe([WestCoastBasis(prefix="")], list(names), [dict(kmA=kmA, krA=0.25, ndA=4.5e-5)])


def theta_of(rng, N):  # (b1, b2, b4) per draw
    return np.array([2.0, 0.5, 0.3]) + rng.standard_normal((N, 3)) * [0.05, 0.3, 0.3]


def even_offsets(N, C):
    return np.arange(C + 1) * (N // C)


def relike():
    """eftb_set_likelihood twice on one engine (the second replaces the first's device arrays, of other sizes), a rows call after each"""
    B, nG, N = 4, 3, 8
    eng, d, rng, likelihood, like = draws_engine(B, nG)
    rows = np.concatenate([np.repeat(d["bias"], N // B, axis=0)[:, None, :], 0.1 * rng.standard_normal((N, nG, 24))], axis=1)
    out = list(like.logp_draws(rows, even_offsets(N, B), return_best=True))
    like = likelihood(3)
    out += list(like.logp_draws(rows, even_offsets(N, B), return_best=True))
    eng.close()
    return out


def regrow():
    """grow_dev: a params call of 8 draws, one of 4096 (every draw buffer is replaced by a larger one), 8 again (nothing grows)"""
    B = 4
    eng, d, rng, _, like = draws_engine(B)
    like.set_draw_recipe(recipe())
    out = []
    for N in (8, 4096, 8):
        out += list(like.logp_draws_params(theta_of(rng, N), even_offsets(N, B), d["f"], return_best=True, grad=True, hess=True))
    eng.close()
    return out


def rerecipe():
    """eftb_set_draw_recipe twice with recipes of other sizes (the second replaces the first's tables), a params call after each"""
    B, N = 4, 8
    eng, d, rng, _, like = draws_engine(B)
    theta, out = theta_of(rng, N), []
    for rec in (recipe(), recipe(("b3", "ce0", "cr1"), kmA=0.45)):
        like.set_draw_recipe(rec)
        out += list(like.logp_draws_params(theta, even_offsets(N, B), d["f"], return_best=True, grad=True, hess=True))
    eng.close()
    return out


def redatasets():
    """eftb_set_likelihood_datasets with 2 data sets, with 5 (the blocks grow), withdrawn; a groups call after each of the first two"""
    B, N = 4, 12
    eng, d, rng, _, like = draws_engine(B)
    like.set_draw_recipe(recipe())
    theta, out = theta_of(rng, N), []
    for M in (2, 5):
        like.set_datasets(1e3 * rng.standard_normal((M, like.index.size)))
        groups = (np.arange(6) % B, np.arange(6) % M)
        out += list(like.logp_draws_params(theta, even_offsets(N, 6), d["f"], return_best=True, grad=True, hess=True, groups=groups))
    like.set_datasets(None)
    out += list(like.logp_draws_params(theta, even_offsets(N, B), d["f"], return_best=True))
    eng.close()
    return out


def gather_single():
    """eftb_gather_plk on one rank without a communicator: the lazily created blocks and events of two exchange slots"""
    B = 3
    eng, d = Engine(cfg(), max_batch=B), draws(B, 37)
    out = []
    for scale in (1.0, 1.1):
        eng.eval_batch(scale * d["Pin"], d["f"], d["DA"], d["H"], bias=d["bias"])
        out.append(eng.gather_plk(B, to_host=True))
    eng.close()
    return out


def partial_masks():
    """REGROUP without RESUM; EFTB_K_RESUM alone after a full run; EFTB_K_IRFILTER alone; a direct engine split in front of REGROUP"""
    B = 3
    eng, d, out = Engine(cfg(), max_batch=B), draws(B, 17), []
    eng.load_inputs(d["Pin"], d["f"], d["DA"], d["H"], d["bias"])
    templ = lambda: eng.get("TEMPL", (B, 3, 24, eng.Nk))
    eng.run(L.S_PREP | L.S_LOOPS | L.S_CF | L.S_REGROUP, B)
    out.append(templ())
    eng.run(eng.full_mask(), B)
    eng.run(L.K_RESUM, B)
    out.append(templ())
    eng.run(L.K_IRFILTER, B)
    out += [eng.get(n, (B, eng.lib.eftb_buffer_size(eng._h, L.B[n]) // B)) for n in ("XY", "Q")]
    eng.set_plk_direct(True)
    eng.run(L.S_PREP | L.S_LOOPS | L.S_CF, B)
    eng.run(L.S_REGROUP | L.S_RESUM | L.S_AP | L.S_REDUCE, B)
    out += [eng.get("PLK", (B, 3, eng.Nk)), templ()]
    eng.close()
    return out


def graph_replay():
    """EFTB_GRAPH=1: the capture of either parity of the template blocks, then a replay of each"""
    eng, d = Engine(cfg(), max_batch=3), draws(3, 19)
    out = [eng.eval_batch(d["Pin"], d["f"], d["DA"], d["H"]) for _ in range(4)]
    eng.close()
    return out


LO = dict(NFFT=512, kin=np.logspace(-4, 0, 200))
# name: (arm of the launcher, environment, case)
CASES = {
    "sync_nl3_split": ("side-stream fork without look-ahead; resum_splits = 8: split s sums, resum_sum_kernel", {}, sync_eval(2, 2)),
    "sync_nl2_split": ("... resum_prep_kernel<2>, resum_mfma2_kernel", {}, sync_eval(2, 2, Nl=2)),
    "sync_nl3_unsplit": ("... the unsplit form", {}, sync_eval(16, 16)),
    "sync_nl2_unsplit": ("... the unsplit form, Nl = 2", {}, sync_eval(16, 16, Nl=2)),
    "async": ("three-stream layout: pre_side, ap_side, ahead, as_side", {}, async_runs(5)),
    "async_no_ap_overlap": ("pre_side without ap_side: the join in front of REGROUP", {"EFTB_AP_OVERLAP": "0"}, async_runs(5)),
    "async_no_prep_overlap": ("asynchronous runs on one stream and the side stream", {"EFTB_PREP_OVERLAP": "0"}, async_runs(5)),
    "staged_direct": ("front_side, coalesced launches, host-written P_l; AP form ap_plk_fused", {}, staged_direct),
    "staged_direct_mom": ("... AP form ap_prefix + ap_plk_mom", {"EFTB_AP_PLK_FUSED": "0"}, staged_direct),
    "staged_direct_nodes": ("... AP form ap_plk (node quadrature)", {"EFTB_AP_PLK_NODES": "1"}, staged_direct),
    # the arms of the staged launch (issue_group)
    "staged_copy_kernel": ("P_l leaves through copy16_kernel", {"EFTB_PLK_DMA": "0"}, staged_direct),
    "staged_event_completion": ("no completion words: the set's event answers 'finished?'", {"EFTB_DONE_WORDS": "0"}, staged_direct),
    "staged_by_caller": ("every launch issued by the calling thread", {"EFTB_SUBMIT_THREAD": "0"}, staged_direct),
    "staged_upload_on_copy": ("uploads on the copy stream: three streams wait for them", {"EFTB_UPLOAD_ON_SIDE": "0"}, staged_direct),
    "staged_outputs": ("per-step destinations: contiguous (merged), with a gap, around a step without one", {}, staged_outputs),
    "staged_odd_copy8": ("odd nx, odd batch: copy8_kernel for the later steps of a launch", {"EFTB_PLK_DMA": "0"}, staged_odd),
    "staged_templates_first": ("templates-first launches: the DMA copy behind the back half, evBack recorded again", {}, staged_templates_first),
    "staged_logp": ("LOGP steps with likelihood rows: the GROWS segments of the upload, ln P from the mapped block", {}, staged_logp),
    "direct_project": ("direct_proj, one operator", {}, sync_eval(4, 4, direct=True, ops=[lambda e: thin(e, 2)])),
    "direct_project_tracers": ("direct_proj, per-tracer operators", {}, sync_eval(4, 4, direct=True, tracers=2, ops=[lambda e: thin(e, 2), lambda e: 0.9 * thin(e, 2)])),
    "project_st_op": ("templates-first PROJECT, stochastic companion (st_op)", {}, sync_eval(3, 3, APst=True, ops=[(lambda e: thin(e, 2), lambda e: 0.5 * thin(e, 2))])),
    "logp_tracers": ("LOGP stage, two tracers", {}, logp_tracers),
    "nnlo_two_pass": ("with_nnlo with PROJECT: the two-pass form, fused accumulator", {}, sync_eval(16, 16, nnlo=True, ops=[lambda e: thin(e, 2)])),
    "nnlo_inline": ("with_nnlo, whole-pipeline asynchronous steps at max_batch 16: the in-line three-stream form", {}, async_runs(16, nnlo=True)),
    "nnlo_unfused": ("with_nnlo at max_batch < 16: the second resummation", {}, sync_eval(2, 2, nnlo=True)),
    "optiresum": ("extract_bao_kernel, no fuse_cf", {}, sync_eval(3, 3, optiresum=True)),
    "dual_coef": ("IRcutoff: the second coefficient set, two anti-diagonal passes", {}, sync_eval(3, 3, IRcutoff="resum", kIR=0.004)),
    "ap_mode1": ("ap_moments_kernel", {"EFTB_AP_MODE": "1"}, sync_eval(3, 3)),
    "ap_mode2": ("ap_direct_kernel on every tile", {"EFTB_AP_MODE": "2"}, sync_eval(3, 3)),
    "ap_stochastic": ("24 AP rows: the 12-row window of ap_rows_kernel, msplit 12", {}, sync_eval(3, 3, APst=True)),
    "nfft512_lo": ("NFFT 512 with low-k tails: prep_rows_lo_kernel, the _nh entry points", {}, sync_eval(3, 3, **LO)),
    "nfft512_lo_direct": ("... on the front of three-stream direct runs: prep_rows_qf_lo_kernel", {}, async_runs(5, direct=True, **LO)),
    "graph": ("captured graph, replayed", {"EFTB_GRAPH": "1"}, graph_replay),
    # what an engine replaces while it lives: the release-then-acquire paths
    "relike": ("eftb_set_likelihood twice, a draws call after each", {}, relike),
    "regrow": ("grow_dev: 8 draws, 4096, 8", {}, regrow),
    "rerecipe": ("eftb_set_draw_recipe twice, a params call after each", {}, rerecipe),
    "redatasets": ("eftb_set_likelihood_datasets: 2 data sets, 5, none; groups calls", {}, redatasets),
    "gather_single": ("eftb_gather_plk without a communicator", {}, gather_single),
    "partial_masks": ("stand-alone REGROUP, EFTB_K_RESUM, EFTB_K_IRFILTER, a split direct run", {}, partial_masks),
}


def dump(path):
    arrays = {}
    for name, (arm, env, case) in CASES.items():
        os.environ.update(env)  # (the switches are read when an engine is created)
        out = case()
        for key in env:
            del os.environ[key]
        for i, a in enumerate(out):
            arrays[f"{name}/{i}"] = np.asarray(a)
        print(f"{name:24s} {len(out)} arrays  [{arm}]", flush=True)
    np.savez(path, **arrays)
    print("library", L.LIB_PATH, "sources", L.load().eftb_source_hash().decode(), "->", path)


def cmp(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files)) + [k for k in A.files if k in B.files and not np.array_equal(A[k], B[k])]
    for k in bad:
        both = k in A.files and k in B.files and A[k].shape == B[k].shape
        print("DIFFERS", k, "max |a - b| / max |a| = %.3e" % (np.max(np.abs(A[k] - B[k])) / np.max(np.abs(A[k]))) if both else "(missing or another shape)")
    print(f"{a} vs {b}: {len(A.files)} arrays, {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
