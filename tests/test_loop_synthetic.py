"""Loop stages on whitened FFTLog coefficients, on the host (no GPU): the reference and the floor of test_gpu_loop_synthetic.py.

On every coefficient set of loop_synth_util (flat, and the four masks) and at NFFT = 256, 258 (odd nh = 129) and 512, as max over output
points and pieces of |a - b| / (absolute-term sum of the point):
  (1) the float64 oracle (OracleEngine.pscf on injected coefficients) against the same sums in np.longdouble (every 9th k and s);
  (2) the NumPy emulation of the device regrouping (emulate.py: `ad` table -> anti-diagonal sums -> rows -> synthesis) against the oracle,
      (a) fed the same coefficients -- the regrouping alone -- and (b) forming its own, [Pin | tail] . (Gc' ; Ec') in float64, as the device does.
Measured (caseE's Pin, Nl = 3, native grids; the worst piece in brackets; "2a" per absolute-term sum on the scale the device sums at,
loop_synth_util.expansion_scale, the others per the piece's own):

    NFFT  set      (1) oracle vs longdouble   (2a) regrouping alone   (2b) emulation vs oracle
    256   flat     5.3e-16 (P13)              2.9e-15 (Cct)           5.1e-14 (C22)
    256   edge     3.1e-16 (C22)              3.6e-14 (C13)           9.5e-13 (C22)
    256   centre   3.8e-16 (C22)              1.4e-15 (P22)           3.8e-15 (C22)
    256   even     5.3e-16 (P13)              7.5e-15 (Cct)           2.0e-14 (C22)
    256   odd      4.2e-16 (P22)              5.6e-15 (Cct)           3.3e-14 (C22)
    258   flat     4.0e-16 (P13)              3.2e-15 (Cct)           6.4e-14 (C22)
    258   edge     3.4e-16 (C22)              3.1e-14 (C22)           1.1e-12 (C22)
    258   centre   2.9e-16 (C22)              1.4e-15 (P22)           4.4e-15 (C22)
    258   even     6.5e-16 (P13)              5.1e-15 (Cct)           5.1e-14 (C22)
    258   odd      3.8e-16 (P13)              4.8e-15 (Cct)           4.0e-14 (C22)
    512   flat     5.3e-16 (P13)              3.7e-15 (P13)           7.0e-14 (Cct)
    512   edge     2.1e-16 (C22)              6.3e-14 (C22)           2.2e-12 (C22)
    512   centre   3.5e-16 (P22)              1.6e-15 (P22)           3.6e-15 (C22)
    512   even     6.0e-16 (P13)              6.1e-15 (Cct)           1.1e-13 (Cct)
    512   odd      4.3e-16 (P22)              7.3e-15 (Cct)           7.0e-14 (Cct)
    256   flat, IRcutoff "loop" + NNLO: 6.7e-16, 3.8e-15, 3.9e-14 (C22)

Column (2b) at "flat" is the floor the GPU tolerance is set against (100 x, capped at 1e-12): 5e-14, 7e-14, 7e-14 (it moves by a few 1e-14 with the
BLAS threading of the oracle's einsums).  The regrouping itself sits at (2a).  What lifts (2b) above it: P22, C22 and C13 are expanded from 7 + 2 basis pieces
(tables.loop_basis), and where a matrix is small against the basis it is combined from -- by 3000 at the entries the edge band weighs -- the rounding of the
basis pieces is that much larger against the piece's own sum; and the whitened edge coefficients are good to 1e-13 in float64 (loop_synth_util.coef_bound).
The edge band at 258 and 512 is recorded, not asserted, at the cap: the GPU runs the masks at 256.
Fitness of the batches: min over the cosmologies of min|c'| / max|c'| = 0.557 (256, 70 draws), 0.547 (258, 65 draws), 0.654 (512, 65 draws pulled to an eighth
of their distance from the fixture; the draws themselves reach 0.088, whitened by their geometric mean 0.087).

Teeth, with the fault put into emulate.py by hand (not committed): the t = 0 pair of anti-diagonal j' = 40 dropped moves the flat set's P22 by 1.9e-5 and C22 by
5.5e-5 of the absolute-term sum; Im of harmonic 250 negated, by 2.1e-5 and 1.2e-4.  The physical-input comparison of test_tables.py stays at 1.8e-14 and 3.9e-11.
"""
import numpy as np
import pytest

import emulate as E
import loop_synth_util as U
from eftpipe_amd.tables import EngineConfig, build_tables

LD_TOL = 1e-14        # the float64 oracle as a reference: a hundredth of the tightest bound it serves
REGROUP_TOL = 1e-13   # the regrouping alone, per absolute-term sum on the scale the device sums at (loop_synth_util.expansion_scale): two float64
                      # summation orders of 66 049 (263 169 at NFFT = 512) terms per point
CAP = 1e-12           # the cap of the GPU tolerance: what the emulation with its own coefficients must stay under wherever the GPU test asserts it


@pytest.fixture(scope="module", params=U.NFFTS)
def setup(request, golden):
    NFFT = request.param
    g = golden("caseE")
    t = build_tables(EngineConfig(Nl=3, NFFT=NFFT, with_resum=True, fft_window=None))
    return dict(NFFT=NFFT, g=g, t=t, orc=U.oracle_for(3, NFFT), flat=U.flat_scale(t, g["Pin"]))


def _halves(c):
    return np.stack([c.real, c.imag])


def _distances(t, orc, Pin, ld_every):
    o = U.oracle_pieces(orc, t, Pin, ld_every=ld_every)
    e = ld_every
    d_ld = {n: U.distance(o["ref"][n][..., ::e], o["ld"][n], o["ld_abs"][n]) for n in o["ref"]}
    st = E.pscf(t, Pin, with_cf=True, coef=(_halves(o["coef_k"]), _halves(o["coef_s"])))
    dev = U.expansion_scale(t, o["abs"])
    d_rg = {n: U.distance(st[n], o["ref"][n], dev[n]) for n in o["ref"]}
    d_rg_own = {n: U.distance(st[n], o["ref"][n], o["abs"][n]) for n in o["ref"]}
    st = E.pscf(t, Pin, with_cf=True)
    d_emu = {n: U.distance(st[n], o["ref"][n], o["abs"][n]) for n in o["ref"]}
    for xi, want in ((False, o["coef_k"]), (True, o["coef_s"])):
        c = E.coef_half(t, Pin, xi)
        assert np.all(np.abs(c[0] + 1j * c[1] - want) <= U.coef_bound(t, Pin, xi))
    return d_ld, d_rg, d_rg_own, d_emu, o


def _worst(d):
    n = max(d, key=d.get)
    return "%.1e (%s)" % (d[n], n)


@pytest.mark.parametrize("name", ("flat",) + U.MASKS)
def test_oracle_and_emulation_on_whitened_coefficients(setup, name):
    t0, orc, g = setup["t"], setup["orc"], setup["g"]
    nch = t0["Gc"].shape[1]
    t = U.whitened_tables(t0, setup["flat"] * U.mask(name, nch))
    d_ld, d_rg, d_own, d_emu, o = _distances(t, orc, g["Pin"], ld_every=9 if setup["NFFT"] < 512 else 27)
    print("NFFT %d %-6s  (1) %-14s  (2a) %-14s  (2a, own sum) %-14s  (2b) %-14s" % (setup["NFFT"], name, _worst(d_ld), _worst(d_rg), _worst(d_own), _worst(d_emu)))
    a = np.abs(o["coef_k"])
    keep = U.mask(name, nch) > 0
    assert np.all(np.abs(a[keep] - 1.0) < 1e-11) and not np.any(a[~keep])          # modulus one on the band (the operator's entries are rounded), nothing off it
    assert o["coef_k"][-1].imag == 0.0                                            # the DC coefficient stays real
    for n in d_ld:
        assert d_ld[n] < LD_TOL, (n, d_ld[n])
        assert d_rg[n] < REGROUP_TOL, (n, d_rg[n])
        if name == "flat" or setup["NFFT"] == 256:   # the sets and sizes the GPU test runs
            assert d_emu[n] < CAP, (n, d_emu[n])
    S = E.antidiagonal_sums(t, _halves(o["coef_k"]))
    N = 2 * (nch - 1)
    if name in ("even", "odd"):
        # n and N - n have the same parity: pairs within one parity have n + m even, the anti-diagonals of odd j' are empty
        # (and j' = N is the pair (N, N) alone, which the odd set does not hold)
        assert not np.any(S[:, 1::2]) and np.all(np.any(S[:, 0 : N - 1 : 2] != 0, axis=0)) and np.any(S[:, N] != 0) == (name == "even")
    if name == "edge":
        # the full set is nonzero at n in {0, 1, 2, N - 2, N - 1, N}: n + m = N + j' has solutions for j' in {0, 1, 2} and {N - 4 ... N} only
        assert not np.any(S[:, 3 : N - 4]) and np.all(np.any(S[:, :3] != 0, axis=0)) and np.all(np.any(S[:, N - 4 :] != 0, axis=0))
    if name == "centre":
        # n in {nh - 2 ... nh + 2}: j' = n + m - N in {0 ... 4}
        assert not np.any(S[:, 5:]) and np.all(np.any(S[:, :5] != 0, axis=0))


def test_basis_combination_is_good_to_rounding_on_the_edge_band(golden):
    """Regression: tables.loop_basis took comb22 from a float64 least-squares fit, good to 5e-15.  Row 12 of M22 is 3000 times smaller than the
    basis matrices it is combined from at the entries (n, m) near (0, N), the only ones the edge band {0, 1, 2} weighs: P22[12] was off by
    2.7e-11 of its absolute-term sum there (1.7e-10 at NFFT = 512), on the host and on the device alike, and by nothing visible on any physical
    input.  With the refined combination the regrouped sums on exact coefficients agree with the oracle to the rounding of the basis pieces."""
    g = golden("caseE")
    t0 = build_tables(EngineConfig(Nl=3, with_resum=True, fft_window=None))
    nch = t0["Gc"].shape[1]
    t = U.whitened_tables(t0, U.flat_scale(t0, g["Pin"]) * U.mask("edge", nch))
    orc = U.oracle_for(3, 256)
    o = U.oracle_pieces(orc, t, g["Pin"])
    st = E.pscf(t, g["Pin"], with_cf=True, coef=(_halves(o["coef_k"]), _halves(o["coef_s"])))
    amp = U.expansion_scale(t, o["abs"])["P22"] / o["abs"]["P22"]
    assert amp[12].max() > 1e3                                   # the row the fit hurt most
    d = np.abs(st["P22"] - o["ref"]["P22"]) / o["abs"]["P22"]
    print("edge band, exact coefficients: P22 row 12 %.1e, every row %.1e of the absolute-term sum" % (d[12].max(), d.max()))
    # what is left is rounding of the basis pieces, magnified by the cancellation of the expansion: a few ulp (the product of two coefficients
    # and a matrix entry, the short sum of the band) times the magnification, 2e-12 at row 12
    assert np.all(d <= 6 * 2.0**-53 * amp.max()), d.max()


def test_batches_are_flat_enough(setup):
    """Fitness of the fixture for the GPU batches: every cosmology's whitened coefficients stay within a factor of two of each other"""
    t0, g, NFFT = setup["t"], setup["g"], setup["NFFT"]
    tw = U.whitened_tables(t0, setup["flat"])
    d = U.draw_set(NFFT, 70 if NFFT == 256 else 65, g["Pin"])
    worst = min(U.flatness(tw, P) for P in d["Pin"])
    print("NFFT %d: min over the batch of min|c'| / max|c'| = %.3f (pull %.3f)" % (NFFT, worst, U.PULL[NFFT]))
    assert worst >= U.FLAT_MIN
    assert U.flatness(tw, g["Pin"]) > 1.0 - 1e-11


def test_two_coefficient_sets_and_nnlo(golden):
    """IRcutoff = "loop" (k-space pieces from the cut set Gc, xi-space pieces from Gc2) with a different scale on each, and the NNLO row set"""
    g, gi = golden("caseE"), golden("ircut")
    kIR = float(gi["kIR"])
    t0 = build_tables(EngineConfig(Nl=3, with_resum=True, with_NNLO=True, fft_window=None, IRcutoff="loop", kIR=kIR))
    nch = t0["Gc"].shape[1]
    ramp = 1.0 + np.arange(nch) / nch
    s1, s2 = U.flat_scale(t0, g["Pin"]), U.flat_scale(t0, g["Pin"], xi=True)
    t = U.whitened_tables(t0, s1, s2 * ramp)
    orc = U.oracle_for(3, 256, with_NNLO=True, IRcutoff="loop", kIR=kIR)
    d_ld, d_rg, d_own, d_emu, o = _distances(t, orc, g["Pin"], ld_every=9)
    print("IRcutoff loop + NNLO  (1) %-14s  (2a) %-14s  (2a, own sum) %-14s  (2b) %-14s" % (_worst(d_ld), _worst(d_rg), _worst(d_own), _worst(d_emu)))
    assert "CctNNLO" in d_emu and np.max(np.abs(np.abs(o["coef_s"]) - ramp)) < 1e-11 and np.max(np.abs(np.abs(o["coef_k"]) - 1.0)) < 1e-11
    for n in d_ld:
        assert d_ld[n] < LD_TOL and d_rg[n] < REGROUP_TOL and d_emu[n] < CAP, (n, d_ld[n], d_rg[n], d_emu[n])
    # the pieces follow their own set: with the two scales swapped every piece is off by far more than rounding
    sw = E.pscf(U.whitened_tables(t0, s1 * ramp, s2), g["Pin"], with_cf=True)
    for n in d_emu:
        assert U.distance(sw[n], o["ref"][n], o["abs"][n]) > 1e-3, n
    tw = U.whitened_tables(t0, s1, s2)
    assert min(U.flatness(tw, P) for P in U.draw_set(256, 2, g["Pin"])["Pin"]) >= U.FLAT_MIN
