"""What the k grids of tests/golden/kgrid_<name>.npz are there for (tools/make_fixtures.py kgrids), checked on the stored `k` itself, so that
a regenerated file cannot drift away from the edge it was made for.  CPU only; the GPU tests on these grids are tests/test_gpu_kgrids.py.

Every other fixture, the native grid and synth.survey_kgrid share one outline: k[0] = 0.001, k[-1] = 0.3 and exactly 7 points below 0.02.  The
launcher and the kernels branch on what that outline never varies:
  * Nklow = #(k < 0.02): the Nl = 3 resummation starts its k tiles at Nklow & ~15, the Nl = 2 one at Nklow, the direct-P_l one clamps its lanes;
  * Nk against the tiles of 16 / 64 / 256 k, and its parity (LDS layouts rounded to pairs, rows of 3 Nk doubles in the copy-out);
  * the last spacing: eftb_finalize takes the interval-moment form of the templates-first AP stage when 0.02 k[-1] / (k[-1] - k[-2]) > 16
    (APW_DCAP / 2), the knot-weight form otherwise;
  * the LDS footprint of ap_plk_fused_kernel against 150 KB: beyond it direct-P_l runs take ap_prefix + ap_plk_mom_kernel.
"""
import numpy as np
import pytest

NMU = 200  # EngineConfig.nbinsmu

# name: (Nk, Nklow, interval-moment form chosen from the last spacing, tables of the fused direct AP stage fit)
PURPOSE = {
    "kmax04": (84, 7, False, True),      # the drop-in's own grid for kmax = 0.4; first tile of 64 full, second ragged
    "kmax05": (104, 7, False, True),     # largest k^2 X(s) of the resummation polynomials
    "from002": (100, 0, False, True),    # no k below 0.02
    "lowdense": (301, 23, False, True),  # Nklow & ~15 = 16: neither 0 nor Nklow; odd Nk; two 256-k tiles, the second ragged; kmax < 0.3
    "odd77": (77, 20, False, True),      # odd, small, Nklow between 16 and 32
    "nk8": (8, 1, False, True),          # the smallest Nk eftb_create accepts: below every tile size
    "densemid": (405, 31, False, True),  # coarse last spacing over a dense interior: many fallback tiles of the knot-weight form
    "finetail": (60, 4, True, True),     # fine last spacing over a coarse grid: moment form; 50 : 1 neighbouring knot spacings
    "s753": (753, 7, False, True),       # last Nk whose fused-AP tables fit
    "s754": (754, 7, False, False),      # first Nk without the fused form, still the knot-weight form
    "s755": (755, 7, True, False),       # first moment-form survey grid
}


def fused_ap_lds_bytes(Nk, nmu=NMU):
    """eftb_finalize's expression for the dynamic LDS of ap_plk_fused_kernel<3, 8>, restated."""
    return 8 * (((Nk + 1) & ~1) + nmu * 8 + 36 * 16 + (nmu + 1) * 36 + (Nk - 1) * 12)


@pytest.mark.parametrize("name", list(PURPOSE))
def test_fixture_grid_sits_on_its_edge(golden, name):
    g = golden("kgrid_" + name)
    k = g["k"]
    Nk, Nklow, moments, fused = PURPOSE[name]
    assert k.ndim == 1 and k.dtype == np.float64 and np.all(np.diff(k) > 0)
    assert k.size == Nk
    assert int(np.sum(k < 0.02)) == Nklow
    ratio = 0.02 * k[-1] / (k[-1] - k[-2])
    assert (ratio > 16) == moments, ratio
    assert (fused_ap_lds_bytes(Nk) <= 150 * 1024) == fused, fused_ap_lds_bytes(Nk)
    # the templates of every file belong to its own grid; the Nl = 2 set exists exactly for the grids with Nk <= 104
    assert g["ap_Ploopl"].shape == (3, 12, Nk) and g["resum_Pctl"].shape == (3, 6, Nk) and g["plk_auto"].shape == (3, Nk)
    assert ("nl2_plk_auto" in g) == (Nk <= 104)
    if Nk <= 104:
        assert g["nl2_ap_P11l"].shape == (2, 3, Nk) and g["nl2_plk_auto"].shape == (2, Nk)


def test_what_the_grids_cover_between_them(golden):
    ks = {n: golden("kgrid_" + n)["k"] for n in PURPOSE}
    nklow = {n: int(np.sum(k < 0.02)) for n, k in ks.items()}
    assert {v & ~15 for v in nklow.values()} == {0, 16}
    assert any(v & ~15 not in (0, v) for v in nklow.values())               # a tile start that is neither 0 nor Nklow
    assert min(nklow.values()) == 0
    assert any(k.size % 2 for k in ks.values()) and any(k.size < 16 for k in ks.values())
    assert any(256 < k.size < 512 and k.size % 256 for k in ks.values())     # more than one 256-k tile, the last one ragged
    assert max(k[-1] for k in ks.values()) >= 0.5 and min(k[-1] for k in ks.values()) < 0.3
    assert fused_ap_lds_bytes(753) <= 150 * 1024 < fused_ap_lds_bytes(754)   # the switch lies between these two at 200 mu nodes
    # a grid whose interior disagrees with its last spacing, in both directions
    d, f = ks["densemid"], ks["finetail"]
    assert 40 * np.median(np.diff(d)) < d[-1] - d[-2] and 0.02 * d[-1] / (d[-1] - d[-2]) < 16
    assert np.median(np.diff(f)) > 40 * (f[-1] - f[-2]) and 0.02 * f[-1] / (f[-1] - f[-2]) > 16
