"""GPU: the direct-P_l resummation in the closed-form basis (resum_plk_kernel<2,8>, back_prep_plk_kernel, Q_e(f)) against the templates-first
path of the same engine -- the project's bar for the two paths, relerr < 1e-9 (they sum in different orders and through different bases; they
agree to about 6e-10), and finite everywhere.

Shapes: the smallest at which the kernel can go wrong.  A workgroup owns 128 k (two per lane) of one cosmology and its eight waves split the
80 s, so: 129 points = one full tile and a ragged tile of one point; an odd grid below 64 points = one tile, Nklow inside it, the second k of
every lane clamped; 512 points with five cosmologies = the bench's tiles with more cosmologies than the small cases; eight cosmologies = the
XCD-aware decoding of the workgroup index.  One case takes the highest-amplitude draws, where z = k^2 X(s) is largest, and asserts on the host
that z stays inside the range in which tests/test_resum_plk_basis.py checks the basis.  Every figure is printed before it is asserted."""
import functools

import numpy as np
import pytest

from conftest import relerr
from eftpipe_amd import synth

pytestmark = pytest.mark.gpu
Z = 0.7
BAR = 1e-9
KPL = 2                       # k per lane of the kernel (RSD_KPL)
Z_LO, Z_HI = -0.05, 8.0        # the z range of the host test (Z_SMALL, Z_POINTS)
BS, ES = [2.14, 0.55, 0.77, 0.55, -1.84, -1.89, -1.49], (0.26, 0.0, -0.93)
GRIDS = {"tile+1": 64 * KPL + 1, "odd45": 45, "bench512": 512}


@functools.lru_cache(maxsize=None)
def engine(grid, max_batch):
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.tables import EngineConfig

    cfg = EngineConfig(Nl=3, k=synth.survey_kgrid(GRIDS[grid]), with_resum=True, with_ap=True, DA_AP=float(synth.da_func(synth.OM_AP, Z)),
                       H_AP=float(synth.hubble(synth.OM_AP, Z)))
    return Engine(cfg, max_batch=max_batch)


@pytest.fixture(scope="module", autouse=True)
def close_engines():
    yield
    for args in (("tile+1", 8), ("odd45", 3), ("bench512", 5)):
        engine(*args).close()
    engine.cache_clear()


def with_bias(d, seed):
    from eftpipe_amd.parambasis import bias_row

    rng = np.random.default_rng(seed)
    bs = np.asarray(BS)
    d["bias"] = np.stack([bias_row(float(f), list(bs * (1.0 + 0.2 * rng.standard_normal(bs.size))), None, ES, kmA=0.7, krA=0.25, ndA=4.5e-5) for f in d["f"]])
    return d


def plk_run(eng, d, B, direct):
    eng.set_plk_direct(direct)
    eng.load_inputs(d["Pin"], d["f"], d["DA"], d["H"], d["bias"])
    eng.run(eng.full_mask(reduce=True), B, sync=True)
    nl, nx = eng.out_dims()
    return eng.get("PLK", (B, nl, nx)).copy()


def both_paths(tag, eng, d, B):
    tm = plk_run(eng, d, B, False)
    dr = plk_run(eng, d, B, True)
    assert np.isfinite(dr).all() and np.isfinite(tm).all()
    err = relerr(dr, tm)
    print(f"RESUM_PLK {tag:32s} direct against templates first: err {err:.3e} bar {BAR:.0e}")
    assert err < BAR, (tag, err)
    assert not np.array_equal(dr, tm)   # (another order of summation: identical bits would mean the option did nothing)
    again = plk_run(eng, d, B, True)    # the option switched back and forth: each run evaluates the Q(f) block that its own resummation reads
    assert np.array_equal(again, dr)


@pytest.mark.parametrize("grid,B", [("tile+1", 1), ("tile+1", 3), ("tile+1", 8), ("odd45", 1), ("odd45", 3), ("bench512", 5)])
def test_direct_against_templates_first(grid, B):
    eng = engine(grid, 8 if grid == "tile+1" else (3 if grid == "odd45" else 5))
    Nk = GRIDS[grid]
    assert eng.tables["k"].size == Nk
    if grid == "odd45":
        nklow = int(np.sum(eng.tables["k"] < 0.02))
        assert 0 < nklow < Nk < 64 and Nk % 2 == 1
    d = with_bias(synth.draw_batch(B, z=Z, seed=5200 + B), 52)
    both_paths(f"{grid} Nk={Nk} B={B}", eng, d, B)


def test_largest_z():
    """The two highest-amplitude draws of 64: z = k^2 X(s) at its largest.  X is linear in P_in, so the draws are ranked on the host by max z itself."""
    import emulate as E

    eng = engine("tile+1", 8)
    t = eng.tables
    d = synth.draw_batch(64, z=Z, seed=5300)
    zmax = np.array([float(np.max(t["k"][:, None] ** 2 * E.ir_filters(t, P)[0][None, :])) for P in d["Pin"]])
    zmin = np.array([float(np.min(t["k"][:, None] ** 2 * E.ir_filters(t, P)[0][None, :])) for P in d["Pin"]])
    top = np.argsort(zmax)[-2:]
    print(f"RESUM_PLK largest z = k^2 X(s) over 64 draws: {zmax.max():.3f} (draws {top.tolist()}), median {np.median(zmax):.3f}; the host test covers [{Z_LO}, {Z_HI}]")
    assert zmax.max() <= Z_HI, zmax.max()
    assert zmax.max() > 4.0            # (the fiducial cosmology reaches 4.08 on this grid: these draws are above it)
    assert zmin.min() >= Z_LO, zmin.min()
    sub = {k: (v[top] if k != "kin" else v) for k, v in d.items()}
    both_paths("largest z, B=2", eng, with_bias(sub, 53), 2)
