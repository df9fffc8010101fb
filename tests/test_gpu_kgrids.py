"""GPU parity on k grids off the usual outline (tests/golden/kgrid_<name>.npz, written by the REAL reference: tools/make_fixtures.py kgrids).

Every other grid the engine is tested on has k[0] = 0.001, k[-1] = 0.3 and 7 points below 0.02; the launcher and the kernels branch on exactly
that (tests/test_kgrids.py lists the edge each grid sits on and checks the stored k against it): Nklow = 0 / 20 / 23 / 31, odd Nk, Nk = 8, more
than one 256-k tile with a ragged last one, kmax = 0.25 ... 0.5, the switch between the two forms of the templates-first AP stage and the LDS
budget of the fused direct-P_l AP kernel.  Bars: the suite's 1e-8 row-scaled (conftest.relerr) against the reference's outputs and the oracle,
1e-9 between the direct-P_l and the template path of one engine, bits where a run-time switch must (or must not) change the arm that runs.
Every figure is printed before it is asserted (pytest -s shows them).
"""
import functools

import numpy as np
import pytest

from conftest import load_golden, relerr
from eftpipe_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-8
ROWS = dict(P11l=slice(0, 3), Pctl=slice(3, 9), Ploopl=slice(9, 21), Pstl=slice(21, 24))
GRIDS = ["kmax04", "kmax05", "from002", "odd77", "lowdense", "finetail", "densemid", "s753", "s754", "s755", "nk8"]
SMALL = ["kmax04", "kmax05", "from002", "odd77", "finetail", "nk8"]  # Nk <= 104: the fixture also holds Nl = 2, and the oracle is cheap
Z = 0.7
SCALES = dict(kmA=0.7, krA=0.25, ndA=4.5e-5)


def check(name, what, got, want, bar=TOL):
    err = relerr(got, want)
    print(f"KGRID {name:9s} {what:44s} err {err:.3e} bar {bar:.0e}")
    assert err < bar, (name, what, err)
    return err


def check_pointwise(name, what, got, want, bar=1e-6):
    big = np.abs(want) > 1e-3 * np.abs(want).max(axis=-1, keepdims=True)
    err = float(np.max(np.abs(got - want)[big] / np.abs(want)[big]))
    print(f"KGRID {name:9s} {what:44s} err {err:.3e} bar {bar:.0e}")
    assert err < bar, (name, what, err)


def make_engine(g, Nl=3, max_batch=3, **kw):
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.tables import EngineConfig

    opts = {k: kw.pop(k) for k in ("with_NNLO",) if k in kw}
    cfg = EngineConfig(Nl=Nl, k=g["k"], with_resum=True, with_ap=True, DA_AP=float(synth.da_func(synth.OM_AP, Z)),
                       H_AP=float(synth.hubble(synth.OM_AP, Z)), **opts)
    return Engine(cfg, max_batch=max_batch, **kw)


def batch(g, B, slots, seed):
    """B cosmologies: the fixture's own in `slots`, seeded draws (synth.draw_batch) everywhere else."""
    d = synth.draw_batch(B, z=Z, seed=seed)
    for i in slots:
        d["Pin"][i], d["f"][i], d["DA"][i], d["H"][i] = g["Pin"], float(g["f"]), float(g["DA"]), float(g["H"])
    return d


def with_bias(g, d, slots, seed):
    """One bias vector per cosmology: the fixture's (bsA, es) in `slots`, seeded perturbations of it elsewhere."""
    from eftpipe_amd.parambasis import bias_row

    rng = np.random.default_rng(seed)
    bsA, es = np.asarray(g["bsA"]), tuple(g["es"])
    d["bs"] = [list(bsA if i in slots else bsA * (1.0 + 0.2 * rng.standard_normal(bsA.size))) for i in range(len(d["f"]))]
    d["bias"] = np.stack([bias_row(float(f), bs, None, es, **SCALES) for f, bs in zip(d["f"], d["bs"])])
    return d


@functools.lru_cache(maxsize=None)
def oracle(name, Nl, nnlo=False):
    from oracle import OracleConfig, OracleEngine

    g = load_golden("kgrid_" + name)
    return OracleEngine(OracleConfig(Nl=Nl, k=g["k"], with_resum=True, with_ap=True, Om_AP=synth.OM_AP, z_AP=Z, with_NNLO=nnlo, **SCALES))


@functools.lru_cache(maxsize=None)
def oracle_draw(name, Nl, B, seed, i, nnlo=False):
    """The oracle on draw i of synth.draw_batch(B, seed): computed once, shared by the tests that run the same draw."""
    d = synth.draw_batch(B, z=Z, seed=seed)
    return oracle(name, Nl, nnlo).evaluate(d["kin"], d["Pin"][i], float(d["f"][i]), float(d["DA"][i]), float(d["H"][i]))


def templates_first(name, g, Nl, pre, max_batch, slots, seed, oracle_slots):
    """eval_batch against the fixture in `slots` and against the oracle in `oracle_slots`; then the same batch stopped in front of the AP stage
    against the fixture's resum_* (a failure is then placed in front of or behind the AP stage)."""
    from eftpipe_amd import _lib as L

    Nk, B = g["k"].size, max_batch
    eng = make_engine(g, Nl, max_batch)
    d = batch(g, B, slots, seed)
    templ = eng.eval_batch(d["Pin"], d["f"], d["DA"], d["H"])
    assert templ.shape == (B, Nl, 24, Nk) and np.isfinite(templ).all()
    tag = f"Nl={Nl} B={B}"
    for i in slots:
        for n, sl in ROWS.items():
            check(name, f"templates {tag} slot {i} ap_{n}", templ[i][:, sl], g[pre + "ap_" + n])
    for i in oracle_slots:
        st = oracle_draw(name, Nl, B, seed, i)
        for n, sl in ROWS.items():
            check(name, f"templates {tag} slot {i} oracle {n}", templ[i][:, sl], st[n])
    eng.load_inputs(d["Pin"], d["f"], d["DA"], d["H"])
    eng.run(eng.full_mask() & ~L.S_AP, B)
    T = eng.get("TEMPL", (B, Nl, 24, Nk))
    for i in slots:
        for n in ("P11l", "Pctl", "Ploopl"):
            check(name, f"in front of AP {tag} slot {i} resum_{n}", T[i][:, ROWS[n]], g[pre + "resum_" + n])
    eng.close()


# ----------------------------------------------------------------------------- (a) templates first, every grid, split s sums
@pytest.mark.parametrize("name", GRIDS)
def test_templates_first_split_sums(golden, name):
    """Nl = 3, max_batch = 3: at this batch size the s sums of the resummation are split (resum_mfma_kernel<false> + resum_sum_kernel)."""
    g = golden("kgrid_" + name)
    templates_first(name, g, 3, "", 3, (1,), 4100, (0, 2) if name in SMALL else ())


# ----------------------------------------------------------------------------- (b) unsplit s sums, NNLO
@pytest.mark.parametrize("name", ["odd77", "lowdense"])
def test_templates_first_unsplit_sums(golden, name):
    """max_batch = 16: one pass over s per k tile, the results added into the template block by the resummation kernel itself; k tiles that
    start at Nklow & ~15 = 16 with idle lanes below Nklow = 20 / 23."""
    g = golden("kgrid_" + name)
    slots = (0, 7, 15)
    templates_first(name, g, 3, "", 16, slots, 4200, [i for i in range(16) if i not in slots] if name in SMALL else ())


@pytest.mark.parametrize("B", [16, 2])
def test_nnlo_odd77(golden, B):
    """with_NNLO on the odd grid against the oracle: B = 16 reaches the fused accumulator resum_mfma_kernel<true>, B = 2 the second
    resummation pass over the NNLO block (split sums have no slot for it)."""
    name = "odd77"
    g = golden("kgrid_" + name)
    Nk = g["k"].size
    slots = (0, 7, 15) if B == 16 else (1,)
    others = (1, 14) if B == 16 else (0,)
    eng = make_engine(g, 3, B, with_NNLO=True)
    d = batch(g, B, slots, 4300)
    templ = eng.eval_batch(d["Pin"], d["f"], d["DA"], d["H"])
    tn = eng.get("TEMPLN", (B, 3, 24, Nk))
    fix = oracle(name, 3, True).evaluate(g["kin"], g["Pin"], float(g["f"]), float(g["DA"]), float(g["H"]))
    for i in slots + others:
        st = fix if i in slots else oracle_draw(name, 3, B, 4300, i, True)
        for n, sl in ROWS.items():
            check(name, f"NNLO B={B} slot {i} oracle {n}", templ[i][:, sl], st[n])
        check(name, f"NNLO B={B} slot {i} oracle PctNNLOl", tn[i][:, 3:6], st["PctNNLOl"])
    for i in slots:  # the block beside it is the fixture's
        for n in ("P11l", "Pctl", "Ploopl"):
            check(name, f"NNLO B={B} slot {i} ap_{n}", templ[i][:, ROWS[n]], g["ap_" + n])
    eng.close()


# ----------------------------------------------------------------------------- (c) Nl = 2
@pytest.mark.parametrize("name", SMALL)
def test_nl2(golden, name):
    """resum_prep_kernel<2> and resum_mfma2_kernel, whose k tiles start at Nklow itself."""
    g = golden("kgrid_" + name)
    templates_first(name, g, 2, "nl2_", 3, (1,), 4400, (0, 2))


# ----------------------------------------------------------------------------- (d) direct P_l, every grid
def plk_run(eng, d, B, direct):
    eng.set_plk_direct(direct)
    eng.load_inputs(d["Pin"], d["f"], d["DA"], d["H"], d["bias"])
    eng.run(eng.full_mask(reduce=True), B, sync=True)
    nl, nx = eng.out_dims()
    return eng.get("PLK", (B, nl, nx)).copy()


@pytest.mark.parametrize("name", GRIDS)
def test_direct_plk(golden, name):
    """set_plk_direct(True), one bias vector per cosmology: against the reference's reduce_Plk of its own AP-stage templates, and against the
    template path of the same engine (another order of summation: identical bits would mean the option did nothing)."""
    g = golden("kgrid_" + name)
    B = 3
    eng = make_engine(g, 3, B)
    d = with_bias(g, batch(g, B, (1,), 4100), (1,), 45)  # (the draws of test_templates_first_split_sums: one oracle run serves both)
    tm = plk_run(eng, d, B, False)
    dr = plk_run(eng, d, B, True)
    assert np.isfinite(dr).all() and np.isfinite(tm).all()
    for what, got in (("direct", dr), ("template path", tm)):
        check(name, f"P_l {what} slot 1 plk_auto", got[1], g["plk_auto"])
        check_pointwise(name, f"P_l {what} slot 1 plk_auto pointwise", got[1], g["plk_auto"])
    check(name, "P_l direct against the template path", dr, tm, 1e-9)
    assert not np.array_equal(dr, tm)
    if name in SMALL:
        for i in (0, 2):
            st = oracle_draw(name, 3, B, 4100, i)
            check(name, f"P_l direct slot {i} oracle", dr[i], oracle(name, 3).reduce_plk(float(d["f"][i]), st, d["bs"][i], es=tuple(g["es"])))
    eng.close()


# ----------------------------------------------------------------------------- (e) the arm that ran, by bits
def run_under(monkeypatch, g, env, direct, B=2):
    """A fresh engine created with `env` set: the switches are read when the engine is created."""
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        eng = make_engine(g, 3, B)
    d = with_bias(g, batch(g, B, (1,), 4600), (1,), 46)
    if direct:
        out = plk_run(eng, d, B, True)
    else:
        out = eng.eval_batch(d["Pin"], d["f"], d["DA"], d["H"])
    eng.close()
    return out


@pytest.mark.parametrize("name,fused", [("s753", True), ("s754", False)])
def test_fused_direct_ap_switches_at_its_lds_budget(golden, monkeypatch, name, fused):
    """Nk = 753 is the last grid whose tables fit the 150 KB of ap_plk_fused_kernel (the largest footprint it can be launched with): turning
    the fused form off changes the bits there, and changes nothing at Nk = 754, which never had it."""
    g = golden("kgrid_" + name)
    default = run_under(monkeypatch, g, {}, True)
    off = run_under(monkeypatch, g, {"EFTB_AP_PLK_FUSED": "0"}, True)
    check(name, "P_l direct, EFTB_AP_PLK_FUSED=0, plk_auto", off[1], g["plk_auto"])
    assert np.array_equal(default, off) == (not fused)


@pytest.mark.parametrize("name,mode", [("s754", "0"), ("s755", "1"), ("finetail", "1"), ("densemid", "0")])
def test_ap_form_follows_the_last_spacing(golden, monkeypatch, name, mode):
    """The templates-first AP stage takes the interval-moment form (EFTB_AP_MODE=1) when 0.02 k[-1] / (k[-1] - k[-2]) > 16 and the knot-weight
    form (0) otherwise: 15.99 at Nk = 754, 16.007 at 755; finetail and densemid are grids whose interior disagrees with their last spacing."""
    g = golden("kgrid_" + name)
    default = run_under(monkeypatch, g, {}, False)
    forced = {m: run_under(monkeypatch, g, {"EFTB_AP_MODE": m}, False) for m in ("0", "1")}
    other = "1" if mode == "0" else "0"
    for m in ("0", "1"):
        for n, sl in ROWS.items():
            check(name, f"templates EFTB_AP_MODE={m} ap_{n}", forced[m][1][:, sl], g["ap_" + n])
    assert np.array_equal(default, forced[mode])
    assert not np.array_equal(default, forced[other])


@pytest.mark.parametrize("env", [{"EFTB_AP_MODE": "0"}, {"EFTB_AP_MODE": "1"}, {"EFTB_AP_MODE": "2"}, {"EFTB_AP_PLK_NODES": "1"},
                                 {"EFTB_AP_PLK_FUSED": "0"}], ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_forced_ap_forms_odd77(golden, monkeypatch, env):
    """Every form of the AP stage on the odd grid (rows of 77 doubles, LDS tables behind an odd number of knots) against the fixture."""
    name = "odd77"
    g = golden("kgrid_" + name)
    direct = "EFTB_AP_MODE" not in env
    out = run_under(monkeypatch, g, env, direct)
    tag = "-".join(f"{k}={v}" for k, v in env.items())
    if direct:
        check(name, f"P_l direct {tag} plk_auto", out[1], g["plk_auto"])
        check_pointwise(name, f"P_l direct {tag} plk_auto pointwise", out[1], g["plk_auto"])
    else:
        for n, sl in ROWS.items():
            check(name, f"templates {tag} ap_{n}", out[1][:, sl], g["ap_" + n])


def test_grid_of_seven_points_is_refused():
    """Nk = 8 (kgrid_nk8) is the smallest grid the library serves; one point fewer is refused by eftb_create with a message, not served wrongly."""
    from eftpipe_amd import _lib as L

    with pytest.raises(L.EftbError, match="bad dimensions Nk=7"):
        make_engine(dict(k=np.linspace(0.01, 0.2, 7)), 3, 1)


# ----------------------------------------------------------------------------- (g) drop-in
@pytest.mark.parametrize("Nl", [3, 2])
def test_dropin_kmax04(golden, Nl):
    """pybird.Common(kmax=0.4) builds its own grid (Nk = 84): Bird -> PsCf -> setPsCfl -> Resum.Ps -> AP as reference theory.py:557-585 drives
    them, against the reference on the same Common."""
    from eftpipe_amd import pybird
    from eftpipe_amd.parambasis import reduce_Plk

    name, pre = "kmax04", "" if Nl == 3 else "nl2_"
    g = golden("kgrid_" + name)
    co = pybird.Common(Nl=Nl, kmax=0.4, **SCALES)
    assert np.array_equal(co.k, g["k"]) and co.Nklow == 7
    nonlinear = pybird.NonLinear(load=False, save=False, co=co)
    resum = pybird.Resum(co=co)
    ap = pybird.APeffect(Om_AP=synth.OM_AP, z_AP=Z, co=co)
    assert np.isclose(ap.DA, g["DA_AP"], rtol=1e-13) and np.isclose(ap.H, g["H_AP"], rtol=1e-15)
    bird = pybird.Bird(g["kin"], g["Pin"], float(g["f"]), float(g["DA"]), float(g["H"]), Z, co=co)
    nonlinear.PsCf(bird)
    bird.setPsCfl()
    resum.Ps(bird)
    for n in ("P11l", "Pctl", "Ploopl"):
        check(name, f"drop-in Nl={Nl} resum_{n}", getattr(bird, n), g[pre + "resum_" + n])
    ap.AP(bird)
    for n in ("P11l", "Pctl", "Ploopl", "Pstl"):
        check(name, f"drop-in Nl={Nl} ap_{n}", getattr(bird, n), g[pre + "ap_" + n])
    plk = reduce_Plk(bird, list(g["bsA"]), es=tuple(g["es"])).sum()
    check(name, f"drop-in Nl={Nl} plk_auto", plk, g[pre + "plk_auto"])
    check_pointwise(name, f"drop-in Nl={Nl} plk_auto pointwise", plk, g[pre + "plk_auto"])


# ----------------------------------------------------------------------------- (h) PROJECT on an odd grid
@pytest.mark.parametrize("nx_out", [13, 67])
@pytest.mark.parametrize("name", ["odd77", "lowdense"])
def test_project_odd_grid(golden, name, nx_out):
    """A dense seeded operator [nl_out = 2][3][nx_out][Nk] behind the AP stage, K = 3 Nk odd: 26 output columns go through gemm_narrow_kernel,
    134 through gemm_rows_kernel with one ragged column tile; templates first and direct (direct_proj: the operator on one row per
    cosmology).  Against NumPy on the engine's own unprojected output, within 4 K 2^-53 (|T| contracted with |Op|): K products summed in
    another order on each side, twice the worst-case rounding of each."""
    g = golden("kgrid_" + name)
    Nk, B = g["k"].size, 3
    rng = np.random.default_rng(7000 + nx_out)
    op = rng.standard_normal((2, 3, nx_out, Nk)) / np.sqrt(3 * Nk)
    K = 3 * Nk
    eng = make_engine(g, 3, B)
    d = with_bias(g, batch(g, B, (1,), 4700), (1,), 47)
    T = eng.eval_batch(d["Pin"], d["f"], d["DA"], d["H"])            # unprojected: templates and the direct run's P_l
    P = plk_run(eng, d, B, True)
    eng.set_plk_direct(False)
    eng.set_pipeline_operator(eng.add_operator(op))
    assert eng.out_dims() == (2, nx_out)
    got = eng.eval_batch(d["Pin"], d["f"], d["DA"], d["H"])
    want = np.einsum("alxk,blrk->barx", op, T)
    bound = 4 * K * 2.0**-53 * np.einsum("alxk,blrk->barx", np.abs(op), np.abs(T))
    assert got.shape == want.shape == (B, 2, 24, nx_out)
    worst = float(np.max(np.abs(got - want) / np.where(bound > 0, bound, 1.0)))
    print(f"KGRID {name:9s} PROJECT nx_out={nx_out} templates: max |err| / bound = {worst:.3f}")
    assert np.all(np.abs(got - want) <= bound)
    gotp = plk_run(eng, d, B, True)
    wantp = np.einsum("alxk,blk->bax", op, P)
    boundp = 4 * K * 2.0**-53 * np.einsum("alxk,blk->bax", np.abs(op), np.abs(P))
    assert gotp.shape == wantp.shape == (B, 2, nx_out)
    worst = float(np.max(np.abs(gotp - wantp) / np.where(boundp > 0, boundp, 1.0)))
    print(f"KGRID {name:9s} PROJECT nx_out={nx_out} direct: max |err| / bound = {worst:.3f}")
    assert np.all(np.abs(gotp - wantp) <= boundp)
    eng.close()


# ----------------------------------------------------------------------------- (i) pipelined steps on an odd row length
@pytest.mark.parametrize("dma", ["1", "0"])
def test_pipelined_steps_odd77(golden, monkeypatch, dma):
    """odd77, direct, Engine(coalesce=3), B = 5: a row of P_l is 3 x 77 = 231 doubles, so the second step of a coalesced launch starts 1155
    doubles into the device block and an odd slot of the results array 1155 k doubles into page-locked memory -- addresses that are only
    8-byte aligned.  Nine steps over three input sets, four kept queued, delivered into pinned_empty memory: every step returns the bits of its
    synchronous run, with the DMA engine and with the copy kernel (EFTB_PLK_DMA=0), in launches of three queued steps whose destinations do
    not follow each other (one copy per step) and in a free-running loop."""
    name = "odd77"
    g = golden("kgrid_" + name)
    Nk, B, K, depth = g["k"].size, 5, 9, 4
    if dma == "0":
        monkeypatch.setenv("EFTB_PLK_DMA", "0")
    eng = make_engine(g, 3, B, coalesce=3)
    sets = [with_bias(g, batch(g, B, (i,), 4800 + i), (i,), 48 + i) for i in range(3)]
    ref = [plk_run(eng, s, B, True) for s in sets]
    for i in range(3):
        check(name, f"P_l direct B=5 set {i} plk_auto", ref[i][i], g["plk_auto"])
    eng.set_plk_direct(True)
    eng.set_latency_mode(False)
    mask = eng.full_mask(reduce=True)
    shape = (B, 3, Nk)
    dest = eng.pinned_empty((K,) + shape)
    # launches of three queued steps; step i delivers into slot perm[i]: no two neighbours in one launch, odd and even slots in each
    perm = [0, 3, 6, 1, 4, 7, 2, 5, 8]
    dest.fill(-1.0)
    eng.set_submit_thread(2)
    eng.submit_stats(enable=True, reset=True)
    for a in (0, 3, 6):
        eng.hold_submissions(True)
        for i in range(a, a + 3):
            s = sets[i % 3]
            eng.step(mask, s["Pin"], s["f"], s["DA"], s["H"], bias=s["bias"], out=dest[perm[i]])
        eng.hold_submissions(False)
        for i in range(a, a + 3):
            eng.fetch_previous("PLK", shape, back=a + 2 - i, copy=False)
            assert np.array_equal(dest[perm[i]], ref[i % 3]), (dma, i)
    st = eng.submit_stats(enable=False)
    assert st["steps"] == K and st["launches"] == 3, st
    # free-running: whatever grouping the timing produces
    dest.fill(-1.0)
    eng.set_submit_thread(1)
    for i in range(K):
        s = sets[i % 3]
        eng.step(mask, s["Pin"], s["f"], s["DA"], s["H"], bias=s["bias"], back=depth if i >= depth else -1, shape=shape, out=dest[i])
        if i >= depth:
            assert np.array_equal(dest[i - depth], ref[(i - depth) % 3]), (dma, i - depth)
    for back in range(depth - 1, -1, -1):
        j = K - 1 - back
        eng.fetch_previous("PLK", shape, back=back, copy=False)
        assert np.array_equal(dest[j], ref[j % 3]), (dma, j)
    eng.close()
