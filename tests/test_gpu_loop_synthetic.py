"""GPU: the loop stages (anti-diagonal pass, row builders, the syntheses of P22 / P13 / C11 / Cct / C22 / C13 and their direct-P_l forms) on
whitened FFTLog coefficients (loop_synth_util): every pair (n, m) and every harmonic carries weight, where on a physical spectrum the edge pair
of each anti-diagonal multiplies an exact zero and the upper half of the synthesis columns sits below the suite's 1e-8.

Stage-wise cases: the operator rows of the engine's tables are rescaled before upload (build_tables wrapped in eftpipe_amd.engine), the taps COEF,
P22, P13, C11, CCT, CC (CCTN) are compared
  * for four cosmologies of the batch (first, last, and the two either side of the lane-group boundary 63 | 64) with the oracle's un-regrouped
    sums on the expected coefficients c' (OracleEngine.pscf, 0.2 - 0.7 s per cosmology), as max over points of |device - oracle| / (absolute-term
    sum of the piece at that point), bound BOUND[NFFT] = min(100 x host floor, 1e-12) (floors: test_loop_synthetic.py, column 2b at "flat");
  * for EVERY cosmology with the NumPy emulation of the same regrouping on float64 coefficients (3 ms per cosmology), per absolute-term sum on
    the scale the device sums at (loop_synth_util.emulated_scale), same bound.
A single dropped pair moves P22 by 1e-5 of its absolute-term sum, a flipped Im above harmonic 192 by as much: seven decades above the bound.

Measured on an MI355X (worst piece; device vs oracle / device vs emulation):
    256 flat B = 70            6.1e-14 (C22) / 1.6e-14 (Cct)        256 edge      7.4e-13 (C22) / 2.0e-13 (C22)
    256 flat B = 3, no resum   9.3e-15 (P22) / 1.6e-15              256 centre    2.7e-15 (P22) / 9.3e-16 (P13)
    258 flat B = 65            7.4e-14 (C22) / 2.9e-14 (Cct)        256 even      3.1e-14 (C22) / 1.6e-14 (Cct)
    512 flat B = 65            5.0e-14 (Cct) / 7.5e-14 (Cct)        256 odd       3.1e-14 (C22) / 1.6e-14 (Cct)
    256 IRcutoff "loop"        3.5e-14 (C22) / 1.1e-14 (Cct)        256 NNLO      4.6e-14 (C22) / 1.4e-14 (CctNNLO)
    direct P_l vs the oracle, row-scaled: 256: 5.1e-14 (templates-first 5.7e-12), 258: 1.1e-13 (4.8e-12); direct vs templates-first 1.5e-11, 1.6e-11
The edge band is the closest to its bound: it weighs only the matrix entries at which rows of M22 are 3000 times smaller than the basis matrices they are
expanded from (test_loop_synthetic.py) -- before the combination of tables.loop_basis was refined it stood at 2.7e-11 and failed.
"""
import numpy as np
import pytest

import emulate as E
import loop_synth_util as U
from conftest import relerr
from eftpipe_amd import synth

pytestmark = pytest.mark.gpu
TOL = 1e-8
FLOOR = {256: 5e-14, 258: 7e-14, 512: 7e-14}                       # host emulation against the oracle on the flat set (test_loop_synthetic.py)
BOUND = {n: min(100.0 * f, 1e-12) for n, f in FLOOR.items()}


def _whiten(g, name="flat", ramp2=False):
    def whiten(t0):
        nch = t0["Gc"].shape[1]
        s1 = U.flat_scale(t0, g["Pin"]) * U.mask(name, nch)
        s2 = U.flat_scale(t0, g["Pin"], xi=True) * U.mask(name, nch) * ((1.0 + np.arange(nch) / nch) if ramp2 else 1.0)
        return U.whitened_tables(t0, s1, s2)

    return whiten


def _stagewise(monkeypatch, golden, B, NFFT=256, name="flat", with_resum=True, ramp2=False, **opts):
    """one engine, one batch -> per piece (worst distance to the oracle over the checked cosmologies, worst distance to the emulation over all)"""
    from eftpipe_amd import _lib as L
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.tables import EngineConfig

    g = golden("caseE")
    Nl = 3
    U.patch_build_tables(monkeypatch, _whiten(g, name, ramp2))
    eng = Engine(EngineConfig(Nl=Nl, NFFT=NFFT, with_resum=with_resum, fft_window=None, **opts), max_batch=B)
    t = eng.tables
    nch, Nk = t["Gc"].shape[1], eng.Nk
    d = U.draw_set(NFFT, B, g["Pin"])
    eng.load_inputs(d["Pin"], d["f"])
    eng.run(L.S_PREP | L.S_LOOPS, B)
    got = dict(COEF=eng.get("COEF", (B, 2, nch)), P22=eng.get("P22", (B, 28, Nk)), P13=eng.get("P13", (B, 10, Nk)))
    names = ["P22", "P13"]
    if with_resum:
        eng.run(L.S_CF, B)
        got.update(C11=eng.get("C11", (B, Nl, 80)), Cct=eng.get("CCT", (B, Nl, 80)))
        cc = eng.get("CC", (B, Nl * 38, 80))
        got.update(C22=cc[:, : Nl * 28].reshape(B, Nl, 28, 80), C13=cc[:, Nl * 28 :].reshape(B, Nl, 10, 80))
        names += ["C11", "Cct", "C22", "C13"]
        if opts.get("with_NNLO"):
            got["CctNNLO"] = eng.get("CCTN", (B, Nl, 80))
            names.append("CctNNLO")
    eng.close()
    for n in names:
        assert np.all(np.isfinite(got[n])), n
    # the operator swap first: COEF against c', within the a-priori bound of a float64 product summed in any order
    for b in range(B):
        c = got["COEF"][b, 0] + 1j * got["COEF"][b, 1]
        assert np.all(np.abs(c - U.coef_half_ld(t, d["Pin"][b])) <= U.coef_bound(t, d["Pin"][b])), ("COEF", b)
    orc = U.oracle_for(Nl, NFFT, **{k: v for k, v in opts.items() if k in ("with_NNLO", "IRcutoff", "kIR")})
    d_orc, d_emu = dict.fromkeys(names, 0.0), dict.fromkeys(names, 0.0)
    for b in sorted({0, min(63, B - 1), min(64, B - 1), B - 1}):
        o = U.oracle_pieces(orc, t, d["Pin"][b])
        for n in names:
            d_orc[n] = max(d_orc[n], U.distance(got[n][b], o["ref"][n], o["abs"][n]))
    for b in range(B):
        ck, cs = E.coef_half(t, d["Pin"][b]), E.coef_half(t, d["Pin"][b], xi=True)
        st = E.pscf(t, d["Pin"][b], with_cf=with_resum, coef=(ck, cs))
        sc = U.emulated_scale(t, d["Pin"][b], (ck, cs), with_cf=with_resum)
        for n in names:
            d_emu[n] = max(d_emu[n], U.distance(got[n][b], st[n], sc[n]))
    print("NFFT %d %-6s B %2d %s: " % (NFFT, name, B, ",".join(f"{k}={v}" for k, v in opts.items()) or ("resum" if with_resum else "no resum"))
          + "  ".join("%s %.1e/%.1e" % (n, d_orc[n], d_emu[n]) for n in names))
    return names, d_orc, d_emu


def _assert(names, d_orc, d_emu, NFFT):
    for n in names:
        assert d_orc[n] < BOUND[NFFT], (n, "oracle", d_orc[n])
        assert d_emu[n] < BOUND[NFFT], (n, "emulation", d_emu[n])


def test_flat_resum_two_lane_groups(monkeypatch, golden):
    """antidiag_kernel<9,2> and build_rows_kernel<9>: 70 draws, two lane groups with a ragged second one, the odd group walking j' backwards"""
    _assert(*_stagewise(monkeypatch, golden, 70), 256)


def test_flat_without_resum(monkeypatch, golden):
    """antidiag_kernel<7,2> and build_rows_kernel<7>: P22 / P13 only, 3 of 64 lanes in use"""
    _assert(*_stagewise(monkeypatch, golden, 3, with_resum=False), 256)


@pytest.mark.parametrize("NFFT", [258, 512])
def test_flat_other_sizes(monkeypatch, golden, NFFT):
    """antidiag_nh_kernel, build_rows_nh_kernel, run-time ksyn / klin: odd nh = 129, and the largest size"""
    _assert(*_stagewise(monkeypatch, golden, 65, NFFT=NFFT), NFFT)


@pytest.mark.parametrize("name", U.MASKS)
def test_masked_bands(monkeypatch, golden, name):
    """One band of coefficients at a time: a failure here names the pairs / harmonics at fault (edge: m in {0, 1, 2}, the anti-diagonals
    j' in {0, 1, 2} and {N - 4 ... N} alone; centre: j' <= 4; even / odd: the harmonics of the other parity stay empty)"""
    _assert(*_stagewise(monkeypatch, golden, 2, name=name), 256)


def test_two_coefficient_sets(monkeypatch, golden):
    """IRcutoff = "loop": Gc (cut) flat, Gc2 flat x (1 + m / NCH) -- the k-space pieces must follow the first set, the xi-space pieces the second"""
    kIR = float(golden("ircut")["kIR"])
    _assert(*_stagewise(monkeypatch, golden, 2, ramp2=True, IRcutoff="loop", kIR=kIR), 256)


def test_nnlo_row_set(monkeypatch, golden):
    """with_NNLO: the third linear row set (nlc = 3) and its synthesis into CCTN"""
    names, d_orc, d_emu = _stagewise(monkeypatch, golden, 2, with_NNLO=True)
    assert "CctNNLO" in names
    _assert(names, d_orc, d_emu, 256)


@pytest.mark.parametrize("NFFT", [256, 258])
def test_direct_plk_on_the_flat_set(monkeypatch, golden, NFFT):
    """Direct P_l (build_rows_plk_kernel<9> / build_rows_plk_nh_kernel<9>): flat set, Nl = 3, resum + AP, 70 draws, a random 24-vector of bias
    coefficients per cosmology -- P_l against the oracle's whole path on the expected coefficients contracted with the same vector (four
    cosmologies; 0.4 s each), and against the templates-first run of the same engine (all).  The stages behind the loops are linear: the unphysical
    templates do them no harm.  A front-end fault of relative size 1e-4 reaches this output; the bounds are the suite's own (1e-8 row-scaled to the
    oracle, 1e-9 between the two orders of contraction: test_gpu_direct.py)."""
    from eftpipe_amd.engine import Engine
    from eftpipe_amd.tables import EngineConfig
    from oracle import OracleConfig, OracleEngine

    g = golden("caseE")
    B, z = 70, float(g["z"])
    U.patch_build_tables(monkeypatch, _whiten(g))
    eng = Engine(EngineConfig(Nl=3, NFFT=NFFT, with_resum=True, with_ap=True, fft_window=None, DA_AP=float(synth.da_func(synth.OM_AP, z)),
                              H_AP=float(synth.hubble(synth.OM_AP, z))), max_batch=B)
    t = eng.tables
    d = U.draw_set(NFFT, B, g["Pin"])
    bias = np.random.default_rng(NFFT).normal(size=(B, 24))
    _, tm = eng.eval_batch(d["Pin"], d["f"], d["DA"], d["H"], bias=bias)
    eng.set_plk_direct(True)
    dr = eng.eval_batch(d["Pin"], d["f"], d["DA"], d["H"], bias=bias, templates=False)
    eng.close()
    assert np.isfinite(dr).all() and not np.array_equal(dr, tm)      # (identical bits would mean the option did nothing)
    print("NFFT %d direct P_l vs templates-first: %.1e" % (NFFT, relerr(dr, tm)))
    assert relerr(dr, tm) < 1e-9
    orc = OracleEngine(OracleConfig(Nl=3, NFFT=NFFT, kmA=0.7, krA=0.25, ndA=4.5e-5, with_resum=True, with_ap=True, Om_AP=synth.OM_AP, z_AP=z))
    for b in (0, 63, 64, B - 1):
        orc.loop_coef = U._Injected(U.mirror(U.coef_half_ld(t, d["Pin"][b])).astype(np.complex128), None, False)
        v = bias[b]
        orc.bias_vectors = lambda *a, v=v, **k: (v[0:3], v[9:21], v[3:9], v[21:24])    # the device's row order: b11, bct, bloop, bst
        st = orc.evaluate(d["kin"], d["Pin"][b], float(d["f"][b]), float(d["DA"][b]), float(d["H"][b]))
        ref = orc.reduce_plk(float(d["f"][b]), st, None)
        print("  cosmology %2d: direct %.1e  templates-first %.1e of the oracle's row maximum" % (b, relerr(dr[b], ref), relerr(tm[b], ref)))
        assert relerr(dr[b], ref) < TOL and relerr(tm[b], ref) < TOL, b
