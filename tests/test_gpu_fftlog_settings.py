"""GPU: the loop FFTLog at NFFT = 384 / 512 and input grids that start above its xmin = 1.5e-5 (low-k power-law tails), through the drop-in
classes and the batched engine, against the REAL reference (tests/golden/fftlog.npz, tools/make_fixtures.py fftlog)."""
import os

import numpy as np
import pytest

from conftest import relerr
from eftpipe_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-8
ROWS = dict(P11l=slice(0, 3), Pctl=slice(3, 9), Ploopl=slice(9, 21), Pstl=slice(21, 24))

CASES = {  # fixture prefix: (NFFT, Nl, low-k grid, AP, Common options)
    "n384": (384, 3, False, True, {}), "n512": (512, 3, False, True, {}), "n512l2": (512, 2, False, False, {}),
    "n512cut": (512, 3, False, True, dict(IRcutoff="all", kIR=0.004)), "n512nnlo": (512, 3, False, True, dict(with_NNLO=True)),
    "lo256": (256, 3, True, True, {}), "lo512": (512, 3, True, True, {}), "lo512loop": (512, 3, True, True, dict(IRcutoff="loop", kIR=0.004)),
}


def _common(Nl, **opts):
    from eftpipe_amd import pybird

    return pybird.Common(Nl=Nl, kmax=0.3, kmA=0.7, krA=0.25, ndA=4.5e-5, **opts)


def _check(g, bird, prefix, names):
    hit = 0
    for n in names:
        key = f"{prefix}_{n}"
        if key in g:
            assert relerr(getattr(bird, n), g[key]) < TOL, key
            hit += 1
    return hit


@pytest.mark.parametrize("case", list(CASES))
def test_dropin_sequence(golden, case):
    from eftpipe_amd import pybird

    g = golden("fftlog")
    NFFT, Nl, lo, ap_on, opts = CASES[case]
    z = float(g["z"])
    co = _common(Nl, **opts)
    nl = pybird.NonLinear(load=False, save=False, NFFT=NFFT, co=co)
    rs = pybird.Resum(co=co)
    ap = pybird.APeffect(Om_AP=synth.OM_AP, z_AP=z, co=co) if ap_on else None
    kin, Pin = (g["kin_lo"], g["Pin_lo"]) if lo else (g["kin"], g["Pin"])
    bird = pybird.Bird(kin, Pin, float(g["f"]), float(g["DA"]), float(g["H"]), z, co=co)
    nl.PsCf(bird)
    assert nl.engine.cfg.NFFT == NFFT
    hit = _check(g, bird, case + "_pscf", ("P11", "P22", "P13", "C11", "Cct"))
    if case + "_pscf_C22_l0" in g:
        assert relerr(bird.C22[0], g[case + "_pscf_C22_l0"]) < TOL and relerr(bird.C13[1], g[case + "_pscf_C13_l2"]) < TOL
    bird.setPsCfl()
    hit += _check(g, bird, case + "_setpscfl", ROWS)
    if lo:
        X, Y = rs.IRFilters(bird)
        assert relerr(X, g[case + "_X"]) < 1e-10 and relerr(Y, g[case + "_Y"]) < 1e-10
    rs.Ps(bird)
    hit += _check(g, bird, case + "_resum", ("P11l", "Pctl", "Ploopl") + (("PctNNLOl",) if opts.get("with_NNLO") else ()))
    if ap is not None:
        ap.AP(bird)
        hit += _check(g, bird, case + "_ap", ROWS)
    assert hit >= 3


def _batch_engine(B, NFFT=512):
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.tables import EngineConfig

    z = 0.7
    cfg = EngineConfig(Nl=3, NFFT=NFFT, kin=np.logspace(-4, 0, 200), with_resum=True, with_ap=True,
                       DA_AP=float(synth.da_func(synth.OM_AP, z)), H_AP=float(synth.hubble(synth.OM_AP, z)))
    return Engine(cfg, max_batch=B)


def _batch_inputs(g, B):
    from eftpipe_amd.parambasis import bias_row

    idx = np.arange(B) % 4
    f = g["batch_f"][idx]
    bias = np.stack([bias_row(float(fi), list(g["bsA"]), None, tuple(g["es"]), kmA=0.7, krA=0.25, ndA=4.5e-5) for fi in f])
    return idx, np.ascontiguousarray(g["batch_Pin"][idx]), f, g["batch_DA"][idx], g["batch_H"][idx], bias


def test_eval_batch_nfft512_low_k_grid(golden):
    g = golden("fftlog")
    B = 128
    eng = _batch_engine(B)
    idx, Pin, f, DA, H, bias = _batch_inputs(g, B)
    templ, plk = eng.eval_batch(Pin, f, DA, H, bias=bias)
    for i in range(B):
        assert relerr(templ[i], g["batch_templ"][idx[i]]) < TOL, i
        assert relerr(plk[i], g["batch_plk"][idx[i]]) < TOL, i
    eng.set_plk_direct(True)
    plk_d = eng.eval_batch(Pin, f, DA, H, bias=bias, templates=False)
    for i in range(B):
        assert relerr(plk_d[i], g["batch_plk"][idx[i]]) < TOL, i
    eng.close()


def test_direct_plk_matches_template_path_nfft384(golden):
    """Direct P_l at NFFT = 384, the size between the compiled-in 256 and the tested 512: nh = 192 gives the row builders a ragged last block
    of lanes (385 harmonics in 7 blocks of 64), and B = 3 leaves 61 of the 64 lanes of the anti-diagonal pass's cosmology group on the
    clamped index.  Held to the engine's own template path at the bar of test_gpu_direct (another order of summation: 1e-9)."""
    g = golden("fftlog")
    B = 3
    eng = _batch_engine(B, NFFT=384)
    _, Pin, f, DA, H, bias = _batch_inputs(g, B)
    _, plk = eng.eval_batch(Pin, f, DA, H, bias=bias)
    eng.set_plk_direct(True)
    plk_d = eng.eval_batch(Pin, f, DA, H, bias=bias, templates=False)
    print("NFFT 384 direct vs templates-first P_l: relerr %.3e" % relerr(plk_d, plk))
    assert np.isfinite(plk_d).all()
    assert relerr(plk_d, plk) < 1e-9
    eng.close()


def test_pipelined_steps_are_bit_identical_nfft512_low_k_grid(golden):
    g = golden("fftlog")
    B, K = 128, 7
    eng = _batch_engine(B)
    _, Pin, f, DA, H, bias = _batch_inputs(g, B)
    sets = [(Pin * s, f, DA, H, bias) for s in (1.0, 1.05, 0.95)]
    mask = eng.full_mask(reduce=True)
    for direct in (True, False):
        eng.set_plk_direct(direct)
        want = []
        for s in sets:
            eng.load_inputs(*s)
            eng.run(mask, B, sync=True)
            want.append(eng.get("PLK", (B, 3, eng.Nk)).copy())
        eng.set_latency_mode(False)
        out = np.zeros((K, B, 3, eng.Nk))
        for i in range(K):
            s = sets[i % 3]
            eng.stage_inputs(s[0], s[1], s[2], s[3], bias=s[4])
            eng.run_staged(mask, B)
            if i >= 3:
                eng.fetch_previous("PLK", (B, 3, eng.Nk), out=out[i - 3], back=3)
        for back in (2, 1, 0):
            eng.fetch_previous("PLK", (B, 3, eng.Nk), out=out[K - 1 - back], back=back)
        eng.sync()
        for i in range(K):
            assert np.array_equal(out[i], want[i % 3]), (direct, i)
        eng.set_latency_mode(True)
    eng.close()


def test_pyegg512_round_trip(golden, tmp_path):
    from eftpipe_amd import pybird

    g = golden("fftlog")
    z = float(g["z"])

    def run(load, save):
        co = _common(3)
        nl = pybird.NonLinear(load=load, save=save, path=str(tmp_path), NFFT=512, co=co)
        bird = pybird.Bird(g["kin_lo"], g["Pin_lo"], float(g["f"]), float(g["DA"]), float(g["H"]), z, co=co)
        nl.PsCf(bird)
        bird.setPsCfl()
        pybird.Resum(co=co).Ps(bird)
        return nl, {n: np.array(getattr(bird, n), copy=True) for n in ("P22", "P13", "C11", "Ploopl", "Pctl")}

    nl1, out1 = run(load=False, save=True)
    path = os.path.join(str(tmp_path), "pyegg512_Nl3.npz")
    assert os.path.exists(path) and not nl1.loaded
    with np.load(path) as zf:
        assert set(zf.files) == {"Pow", "M22", "M13", "Mcf11", "Mcf22", "Mcf13", "Mcfct", "McfctNNLO"}
        assert zf["Pow"].shape == (513,) and zf["M22"].shape == (28, 513, 513) and zf["M13"].shape == (10, 513)
        assert zf["Mcf11"].shape == (3, 513) and zf["Mcf22"].shape == (28, 3, 513, 513)
    nl2, out2 = run(load=True, save=False)
    assert nl2.loaded
    for n in out1:
        assert np.array_equal(out1[n], out2[n]), n
    assert relerr(out2["Ploopl"], g["lo512_resum_Ploopl"]) < TOL
