"""Many EFT parameter draws against one cosmology's templates (eftb_draws_logp / eftb_draws_reduce; the fast / slow split of reference
theory.py:829-874): the marginalised ln P of every draw against the oracle (oracle/marginal.py) and the LOGP stage, P_l of every draw
against the REDUCE stage, the Gram cache across template / likelihood changes, and the refusals."""
import numpy as np
import pytest

import cfg3_util as U
from conftest import relerr

pytestmark = pytest.mark.gpu

COUNTS = [3, 0, 7, 1, 4]  # draws per walker (walker 1 owns none)


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _marg(golden, tag, max_batch=16):
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.marginal import data_index
    from eftpipe_amd.tables import EngineConfig

    g = golden("marg")
    nx = g["binned_P11l"].shape[-1]
    eng = Engine(EngineConfig(Nl=3), max_batch=max_batch)
    eng.set_template_dims(3, nx)
    T = np.concatenate([g["binned_P11l"], g["binned_Pctl"], g["binned_Ploopl"], g["binned_Pstl"]], axis=1)
    ls = list(g["ls"])
    index = data_index(ls, {l: slice(a, b) for l, (a, b) in zip(ls, g["masks"])}, nx)
    return g, eng, T, index


def _marg_draws(g, tag, counts, seed=7):
    """rows [N, nG + 1, 24] of draws varying b1 / b2 / b4 (draw 0: the fixture's point), walker of each draw"""
    from eftpipe_amd.parambasis import gaussian_rows_many

    f, co = float(g["f"]), g[tag + "_co"]
    ng = dict(zip(g[tag + "_ng_names"], g[tag + "_ng_values"]))
    N = int(np.sum(counts))
    rng = np.random.default_rng(seed)
    d = rng.normal(0.0, 1.0, (N, 3)) * [0.05, 0.3, 0.3]
    d[0] = 0.0
    if tag == "auto":
        rows = gaussian_rows_many(f, np.array([ng["b1"], ng["b2"], ng["b4"]]) + d, None, *co[:3])
    else:
        rows = gaussian_rows_many(f, np.array([ng["A_b1"], ng["A_b2"], ng["A_b4"]]) + d, np.tile([ng["B_b1"], ng["B_b2"], ng["B_b4"]], (N, 1)), *co)
    return rows, np.repeat(np.arange(len(counts)), counts)


def _oracle(g, tag, rows, templ, index, jeffreys=False, loc=None, scale=None):
    from oracle import marginal as M

    V = np.einsum("gr,lrx->glx", rows, templ).reshape(rows.shape[0], -1)[:, index]
    loc = g[tag + "_loc"] if loc is None else loc
    scale = g[tag + "_scale"] if scale is None else scale
    return M.marginalized_logp(V[1:], V[0], g[tag + "_D"], g[tag + "_invcov"], loc, scale, jeffreys=jeffreys, return_best=True)


@pytest.mark.parametrize("tag", ["auto", "cross"])
def test_draws_match_oracle_and_logp_stage(golden, tag):
    from eftpipe_amd.marginal import MarginalLikelihood

    g, eng, T, index = _marg(golden, tag)
    C = len(COUNTS)
    templ = np.stack([T * (1.0 + 0.1 * c) for c in range(C)])
    eng.put("TEMPL", templ)
    rows, walker = _marg_draws(g, tag, COUNTS)
    off = _offsets(COUNTS)
    like = MarginalLikelihood(eng, index, g[tag + "_D"], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"])
    logp, full, best = like.logp_draws(rows, off, return_best=True)
    assert logp.shape == full.shape == (rows.shape[0],) and best.shape == (rows.shape[0], len(g[tag + "_loc"]))
    assert np.isclose(logp[0], g[tag + "_logp"], rtol=1e-10) and np.isclose(full[0], g[tag + "_fullchi2"], rtol=1e-9)
    assert relerr(best[0][None], g[tag + "_best"][None]) < 1e-8
    for d in range(rows.shape[0]):
        want = _oracle(g, tag, rows[d], templ[walker[d]], index)
        assert np.isclose(logp[d], want[0], rtol=1e-10), d
        assert np.isclose(full[d], want[1], rtol=1e-9), d
        assert relerr(best[d][None], want[2][None]) < 1e-8, d
    # a second call reuses the Gram block: the same bits
    assert np.array_equal(like.logp_draws(rows, off), logp)
    # Jeffreys: the fixture's own value, the oracle for the others
    like_j = MarginalLikelihood(eng, index, g[tag + "_D"], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"], jeffreys=True)
    lj = like_j.logp_draws(rows, off)
    assert np.isclose(lj[0], g[tag + "_logp_jeffreys"], rtol=1e-10)
    for d in range(rows.shape[0]):
        assert np.isclose(lj[d], _oracle(g, tag, rows[d], templ[walker[d]], index, jeffreys=True)[0], rtol=1e-10), d
    if tag == "auto":  # flat prior (the cross fixture's 11 parameters are degenerate without one: see test_gpu_marginal)
        nG = len(g[tag + "_loc"])
        like_f = MarginalLikelihood(eng, index, g[tag + "_D"], g[tag + "_invcov"], np.zeros(nG), np.full(nG, np.inf))
        lf = like_f.logp_draws(rows, off)
        assert np.isclose(lf[0], g[tag + "_logp_flat"], rtol=1e-9)
        for d in range(rows.shape[0]):
            want = _oracle(g, tag, rows[d], templ[walker[d]], index, loc=np.zeros(nG), scale=np.full(nG, np.inf))[0]
            assert np.isclose(lf[d], want, rtol=1e-9), d
    # the same draws through the LOGP stage: the walker's templates duplicated per draw (the engine holds one likelihood: set it again)
    like = MarginalLikelihood(eng, index, g[tag + "_D"], g[tag + "_invcov"], g[tag + "_loc"], g[tag + "_scale"])
    assert np.array_equal(like.logp_draws(rows, off), logp)
    eng.put("TEMPL", templ[walker])
    lp_stage, full_stage, best_stage = like.logp(rows, return_best=True)
    assert np.allclose(logp, lp_stage, rtol=1e-10, atol=0)
    assert np.allclose(full, full_stage, rtol=1e-9, atol=0)
    assert relerr(best, best_stage) < 1e-8
    eng.close()


def test_plain_chi2_draws():
    """nG = 0: -chi2 / 2 of row 0 per draw."""
    from conftest import load_golden
    from eftpipe_amd.marginal import MarginalLikelihood
    from eftpipe_amd.parambasis import bias_rows_many

    g = load_golden("marg")
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.marginal import data_index
    from eftpipe_amd.tables import EngineConfig

    nx = g["binned_P11l"].shape[-1]
    eng = Engine(EngineConfig(Nl=3), max_batch=4)
    eng.set_template_dims(3, nx)
    T = np.concatenate([g["binned_P11l"], g["binned_Pctl"], g["binned_Ploopl"], g["binned_Pstl"]], axis=1)
    ls = list(g["ls"])
    index = data_index(ls, {l: slice(a, b) for l, (a, b) in zip(ls, g["masks"])}, nx)
    D, Ci = g["auto_D"], g["auto_invcov"]
    like = MarginalLikelihood(eng, index, D, Ci, np.zeros(0), np.zeros(0))
    eng.put("TEMPL", np.stack([T, 1.1 * T]))
    N = 5
    bs = np.tile([2.1, 0.5, 0.3, 0.2, -1.0, -2.0, 0.5], (N, 1)) + 0.1 * np.arange(N)[:, None]
    rows = bias_rows_many(float(g["f"]), bs, None, (0.3, 0.1, -0.4), kmA=0.7, krA=0.25, ndA=4.5e-5)
    walker = np.array([0, 0, 1, 1, 1])
    logp = like.logp_draws(rows[:, None, :], _offsets([2, 3]))
    for d in range(N):
        r = np.einsum("r,lrx->lx", rows[d], (1.1 if walker[d] else 1.0) * T).reshape(-1)[index] - D
        assert np.isclose(logp[d], -0.5 * r @ Ci @ r, rtol=1e-10), d
    eng.close()


def _cfg3_block(g):
    """the likelihood's templates of one cfg 3 point [3 tracers, 3, 24, nb]: binned LRG / X, chained ELG padded with a zero multipole"""
    nb = max(U.final_templates(g, t)["P11l"].shape[-1] for t in U.TRACERS)
    out = np.zeros((3, 3, 24, nb))
    for i, t in enumerate(U.TRACERS):
        ft = U.final_templates(g, t)
        T = np.concatenate([ft[n] for n in U.NAMES], axis=1)
        out[i, : T.shape[0], :, : T.shape[-1]] = T
    return out, nb


@pytest.mark.parametrize("tag", ["full", "xnost"])
def test_cfg3_joint_draws(golden, tag):
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.marginal import MarginalLikelihood, data_index, joint_gaussian_rows_many
    from eftpipe_amd.tables import EngineConfig
    from oracle import marginal as M

    g = golden("cfg3")
    block, nb = _cfg3_block(g)
    eng = Engine(EngineConfig(Nl=3), max_batch=24)
    eng.set_tracers(3)
    eng.set_template_dims(3, nb)
    templ = np.concatenate([block, 1.02 * block])  # walker 0: the fixture's point, walker 1: rescaled templates
    eng.put("TEMPL", templ)
    index = np.concatenate([data_index([int(l) for l in g[t + "_ls"]], U.masks(g, t), nb, tracer=i, nl=3) for i, t in enumerate(U.TRACERS)])
    names = [str(n) for n in g[tag + "_names"]]
    nG = len(names)
    counts = [4, 3]
    N = sum(counts)
    p = U.params(g)
    rng = np.random.default_rng(9)
    draws = {k: np.full(N, v) for k, v in p.items()}
    for k in ("LRG_NGC_b1", "ELG_NGC_b1", "LRG_NGC_c2", "ELG_NGC_c4"):
        draws[k] = p[k] + np.where(np.arange(N) == 0, 0.0, 0.05 * rng.normal(size=N))
    for t in ("LRG_NGC_", "ELG_NGC_"):
        draws[t + "b2"] = (draws[t + "c2"] + draws[t + "c4"]) / np.sqrt(2.0)
        draws[t + "b4"] = (draws[t + "c2"] - draws[t + "c4"]) / np.sqrt(2.0)
    f = [float(g[t + "_f"]) for t in U.TRACERS]
    rows = joint_gaussian_rows_many(U.bases(), f, draws, names, U.scales(g))
    assert rows.shape == (N, 3, nG + 1, 24)
    walker = np.repeat([0, 1], counts)
    for jeff, key in ((True, "_logp"), (False, "_logp_nojeffreys")):
        like = MarginalLikelihood(eng, index, g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf), jeffreys=jeff)
        logp, full, best = like.logp_draws(rows, _offsets(counts), return_best=True)
        assert np.isclose(logp[0], g[tag + key], rtol=1e-9), (logp[0], g[tag + key])
        if jeff:
            assert relerr(best[0][None], g[tag + "_best"][None]) < 1e-7
        for d in range(N):
            V = np.concatenate([np.einsum("gr,lrx->glx", rows[d, t], templ[3 * walker[d] + t]) for t in range(3)], axis=1).reshape(nG + 1, -1)[:, index]
            want = M.marginalized_logp(V[1:], V[0], g["data_vector"], g["invcov"], np.zeros(nG), np.full(nG, np.inf), jeffreys=jeff, return_best=True)
            assert np.isclose(logp[d], want[0], rtol=1e-9), d
            assert np.isclose(full[d], want[1], rtol=1e-8), d
        # the LOGP stage on the walkers' templates duplicated per draw
        eng.put("TEMPL", templ.reshape(2, 3, 3, 24, nb)[walker].reshape(3 * N, 3, 24, nb))
        assert np.allclose(like.logp(rows.reshape(3 * N, nG + 1, 24)), logp, rtol=1e-10, atol=0)
        eng.put("TEMPL", templ)
    eng.close()


def _caseC_engine(golden, B):
    from eftpipe_amd import tables as TB
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.marginal import data_index
    from eftpipe_amd.tables import EngineConfig

    g = golden("caseC")
    k = g["k"]
    Bm, _, _, _ = TB.binning_operator(k, g["kout"])
    nb = len(g["kout"])
    eng = Engine(EngineConfig(Nl=3, with_resum=True, with_ap=True, DA_AP=float(g["DA_AP"]), H_AP=float(g["H_AP"])), max_batch=B)
    eng.set_pipeline_operator(eng.add_operator(TB.compose_operator(3, k.size, binning=Bm)))
    index = data_index([0, 2], {0: slice(0, nb), 2: slice(1, nb - 1)}, nb)
    return g, eng, index, nb


def test_workflow_slow_step_then_fast_draws(golden):
    """eval_logp (slow step) then draws: a draw that repeats a walker's rows gives the walker's ln P; put("TEMPL") invalidates the Gram
    block; staged steps and eval_logp after the draws give the bits they give without them."""
    from eftpipe_amd import _lib as L
    from eftpipe_amd.marginal import MarginalLikelihood
    from eftpipe_amd.parambasis import gaussian_rows, gaussian_rows_many

    B = 3
    g, eng, index, nb = _caseC_engine(golden, 16)
    rng = np.random.default_rng(31)
    f0, DA0, H0 = float(g["f"]), float(g["DA"]), float(g["H"])
    mk = lambda: dict(Pin=g["Pin"][None] * (1.0 + 0.1 * rng.uniform(-1, 1, (B, 1))), f=f0 * (1.0 + 0.03 * rng.uniform(-1, 1, B)),
                      DA=DA0 * (1.0 + 0.02 * rng.uniform(-1, 1, B)), H=H0 * (1.0 + 0.02 * rng.uniform(-1, 1, B)))
    steps = [mk() for _ in range(3)]
    for st in steps:
        st["rows"] = np.stack([gaussian_rows(fi, (2.0 + 0.1 * rng.uniform(), 0.5, 0.3), None, 0.7, 0.25, 4.5e-5) for fi in st["f"]])
    templ = eng.eval_batch(steps[0]["Pin"], steps[0]["f"], steps[0]["DA"], steps[0]["H"])
    model = np.einsum("r,lrx->lx", steps[0]["rows"][0, 0], templ[0]).reshape(-1)[index]
    sig = 0.05 * np.abs(model) + 10.0
    like = MarginalLikelihood(eng, index, model * 1.02, np.diag(1.0 / sig**2), np.zeros(7), np.full(7, 3.0))

    def sequence(with_draws):
        s0 = steps[0]
        lp0 = like.eval_logp(s0["Pin"], s0["f"], s0["DA"], s0["H"], s0["rows"])
        if with_draws:
            counts = [3, 2, 4]
            ng = np.concatenate([np.tile([2.0, 0.5, 0.3], (n, 1)) + rng.normal(0, 0.1, (n, 3)) for n in counts])
            fw = np.repeat(s0["f"], counts)
            rows = gaussian_rows_many(fw, ng, None, 0.7, 0.25, 4.5e-5)
            first = _offsets(counts)[:-1]
            rows[first] = s0["rows"]  # the first draw of each walker repeats the walker's rows
            lpd = like.logp_draws(rows, _offsets(counts))
            assert np.allclose(lpd[first], lp0, rtol=1e-10, atol=0)
            # new templates through put: the next draw call sees them (the Gram block is rebuilt)
            eng.put("TEMPL", 1.05 * templ)
            lpn = like.logp_draws(rows, _offsets(counts))
            assert not np.allclose(lpn[first], lp0, rtol=1e-6)
            assert np.allclose(lpn[first], like.logp(s0["rows"]), rtol=1e-10, atol=0)
        staged = [r.copy() for r in eng.pipeline(steps[1:], fetch="LOGP")]
        with pytest.raises(L.EftbError, match="no templates"):  # a staged step has rotated the blocks
            like.logp_draws(s0["rows"], _offsets([1, 1, 1]))
        s2 = steps[2]
        return lp0, staged, like.eval_logp(s2["Pin"], s2["f"], s2["DA"], s2["H"], s2["rows"])

    a = sequence(False)
    b = sequence(True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
    eng.close()


def test_nnlo_draws_match_logp_stage():
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.marginal import MarginalLikelihood
    from eftpipe_amd.tables import EngineConfig

    rng = np.random.default_rng(4)
    nx, C, counts = 20, 3, [2, 5, 3]
    N = sum(counts)
    eng = Engine(EngineConfig(Nl=3, with_resum=True, with_ap=True, DA_AP=1.0, H_AP=1.0, with_NNLO=True), max_batch=N)
    eng.set_template_dims(3, nx)
    T = rng.normal(0, 1, (C, 3, 24, nx)) * np.logspace(0, 3, 24)[:, None]
    TN = rng.normal(0, 1, (C, 3, 24, nx)) * 30.0
    index = np.sort(rng.choice(3 * nx, 40, replace=False)).astype(np.int32)
    D = rng.normal(0, 50, 40)
    Ci = np.diag(1.0 / rng.uniform(5, 20, 40) ** 2)
    nG = 5
    like = MarginalLikelihood(eng, index, D, Ci, np.zeros(nG), np.full(nG, 2.0))
    rows = rng.normal(0, 1, (N, nG + 1, 24))
    rn = rng.normal(0, 1, (N, nG + 1, 3))
    eng.put("TEMPL", T)
    eng.put("TEMPLN", TN)
    logp = like.logp_draws(rows, _offsets(counts), rows_nnlo=rn)
    walker = np.repeat(np.arange(C), counts)
    eng.put("TEMPL", T[walker])
    eng.put("TEMPLN", TN[walker])
    assert np.allclose(logp, like.logp(rows, rows_nnlo=rn), rtol=1e-10, atol=0)
    eng.close()


@pytest.mark.parametrize("kind", ["ap", "ap_stochastic", "nnlo", "tracers"])
def test_reduce_draws_bits_of_reduce_stage(kind):
    from eftpipe_amd import _lib as L
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.tables import EngineConfig

    rng = np.random.default_rng(12)
    nnlo = kind == "nnlo"
    ntr = 2 if kind == "tracers" else 1
    counts = [4, 0, 6]
    C, N, nx = len(counts), sum(counts), 37
    cfg = EngineConfig(Nl=3, with_resum=True, with_ap=True, DA_AP=1.0, H_AP=1.0, with_NNLO=nnlo) if kind != "tracers" else EngineConfig(Nl=3)
    eng = Engine(cfg, max_batch=N * ntr)
    if kind == "ap_stochastic":
        eng.set_ap_stochastic(True)
    if ntr > 1:
        eng.set_tracers(ntr)
    eng.set_template_dims(3, nx)
    T = rng.normal(0, 1, (C * ntr, 3, 24, nx)) * np.logspace(0, 4, 24)[:, None]
    TN = rng.normal(0, 1, (C * ntr, 3, 24, nx)) * 100.0
    bias = rng.normal(1, 1, (N, ntr, 24))
    bn = rng.normal(0, 1, (N, ntr, 3)) if nnlo else None
    eng.put("TEMPL", T)
    if nnlo:
        eng.put("TEMPLN", TN)
    plk = eng.reduce_draws(bias if ntr > 1 else bias[:, 0], _offsets(counts), bias_nnlo=bn)
    assert plk.shape == ((N, ntr, 3, nx) if ntr > 1 else (N, 3, nx))
    # the REDUCE stage on the walkers' entries duplicated per draw
    walker = np.repeat(np.arange(C), counts)
    ent = (walker[:, None] * ntr + np.arange(ntr)).reshape(-1)
    eng.put("TEMPL", T[ent])
    if nnlo:
        eng.put("TEMPLN", TN[ent])
        eng.put("BIASN", bn.reshape(-1, 3))
    eng.put("BIAS", bias.reshape(-1, 24))
    eng.run(L.S_REDUCE, N * ntr)
    want = eng.get("PLK", (N * ntr, 3, nx))
    assert np.array_equal(plk.reshape(N * ntr, 3, nx), want)
    eng.close()


def test_draws_error_paths(golden):
    from eftpipe_amd import _lib as L
    from eftpipe_amd import synth
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.marginal import MarginalLikelihood
    from eftpipe_amd.parambasis import bias_row
    from eftpipe_amd.tables import EngineConfig

    g, eng, T, index = _marg(golden, "auto", max_batch=4)
    rows, _ = _marg_draws(g, "auto", [2, 2])
    nG = len(g["auto_loc"])
    eng.put("TEMPL", np.stack([T, T]))
    like = MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], g["auto_loc"], g["auto_scale"])
    like.logp_draws(rows, [0, 2, 4])
    for bad in ([1, 2, 4], [0, 3, 2, 4], [0, 2, 5]):  # offsets[0] != 0, decreasing, offsets[C] != N
        with pytest.raises(L.EftbError, match="offsets"):
            like.logp_draws(rows, bad)
    with pytest.raises(ValueError, match="offsets"):
        like.logp_draws(rows, [4])
    with pytest.raises(L.EftbError, match="entries"):  # three walkers, two template entries
        like.logp_draws(rows, [0, 2, 3, 4])
    with pytest.raises(L.EftbError, match="entries"):
        eng.reduce_draws(np.ones((4, 24)), [0, 1, 2, 3, 4])
    with pytest.raises(ValueError, match="rows"):
        like.logp_draws(rows[:, :-1], [0, 2, 4])
    # a block of another shape than the likelihood's
    eng.set_template_dims(2, T.shape[-1])
    with pytest.raises(L.EftbError, match="addresses templates"):
        like.logp_draws(rows, [0, 2, 4])
    eng.set_template_dims(3, T.shape[-1])
    # det F2 <= 0 (flat prior, no derivative rows)
    like_f = MarginalLikelihood(eng, index, g["auto_D"], g["auto_invcov"], np.zeros(nG), np.full(nG, np.inf))
    with pytest.raises(RuntimeError, match="det of F2ij"):
        like_f.logp_draws(np.zeros((2, nG + 1, 24)), [0, 1, 2])
    # no likelihood (eftb_set_tracers drops it)
    eng.set_tracers(1)
    with pytest.raises(L.EftbError, match="eftb_set_likelihood"):
        like.logp_draws(rows, [0, 2, 4])
    eng.close()
    # after a direct-P_l run the block holds no templates
    z = 0.7
    cos = synth.cosmology(z=z, Om=0.3, h=0.68)
    DA_AP, H_AP = float(synth.da_func(synth.OM_AP, z)), float(synth.hubble(synth.OM_AP, z))
    eng = Engine(EngineConfig(Nl=3, with_resum=True, with_ap=True, DA_AP=DA_AP, H_AP=H_AP), max_batch=2)
    bias = np.stack([bias_row(float(cos["f"]), [2.14, 0.55, 0.77, 0.55, -1.84, -1.89, -1.49], None, (0.26, 0.0, -0.93), kmA=0.7, krA=0.25, ndA=4.5e-5)] * 2)
    Pin = np.stack([cos["Pin"], 1.1 * cos["Pin"]])
    eng.eval_batch(Pin, cos["f"], cos["DA"], cos["H"])
    plk = eng.reduce_draws(bias, [0, 1, 2])  # a template-producing run: the draws see its templates
    eng.set_plk_direct(True)
    want = eng.eval_batch(Pin, cos["f"], cos["DA"], cos["H"], bias=bias, templates=False)
    assert relerr(plk, want) < 1e-9
    with pytest.raises(L.EftbError, match="no templates"):
        eng.reduce_draws(bias, [0, 1, 2])
    eng.close()
