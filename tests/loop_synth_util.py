"""Whitened FFTLog coefficients for the loop stages (shared by test_loop_synthetic.py and test_gpu_loop_synthetic.py; no GPU).

On a physical P_lin the coefficients c_m fall by five to seven decades from the centre of the band (m = NCH - 1, the real DC term) to its edge
(m = 0), and the default edge window makes c_0 exactly zero: most of the pairs and harmonics the loop kernels sum carry no weight.  The
coefficients are linear in the input, c = [Pin | tail] . (Gc ; Ec), so multiplying ROW m of the operator by a real factor scale[m] multiplies
c_m by it and touches nothing else (P_lin, P11, the tails and the IR filters keep their physical values).  With scale = 1 / |c_m| of one
fixture spectrum every coefficient of that spectrum has modulus one (the "flat" set) and every pair (n, m) of the double sums counts.

The reference of a loop piece is the oracle's own, un-regrouped sum (OracleEngine.pscf, its einsums untouched) with loop_coef returning the
whitened coefficients c', which are formed here in np.longdouble; next to each piece comes its absolute-term sum at every output point
(the same einsums over |c' x| and |M|): errors are measured pointwise against that, so that both ends of k^-0.2 and of s^-2.8 are tested.
"""
import copy

import numpy as np

PIECES = ("P22", "P13", "C11", "Cct", "C22", "C13")
MASKS = ("edge", "centre", "even", "odd")
_MATS = ("M22", "M13", "Mcf11", "Mcfct", "McfctNNLO", "Mcf22", "Mcf13")


# ----------------------------------------------------------------------------- the operator swap
def whitened_tables(t, scale, scale2=None):
    """A copy of a build_tables dict whose Gc / Ec rows m = 0 ... NCH - 1 are multiplied by scale[m] (real), and Gc2 / Ec2 -- the operator of the
    xi-space pieces under IRcutoff = "loop" | "resum" -- by scale2[m] (default: scale).  Everything else is the same object as in t."""
    out = dict(t)
    for G, E, sc in (("Gc", "Ec", scale), ("Gc2", "Ec2", scale if scale2 is None else scale2)):
        if G in t:
            sc = np.asarray(sc, dtype=np.float64)
            assert sc.shape == (t[G].shape[1],) and np.all(np.isfinite(sc))
            out[G] = np.ascontiguousarray(t[G] * sc[None, :, None])
            out[E] = np.ascontiguousarray(t[E] * sc[None, :, None])
    return out


def patch_build_tables(monkeypatch, whiten):
    """Engines created from now on (until monkeypatch undoes it) upload whiten(tables): wraps the build_tables that eftpipe_amd.engine imported.
    whiten: physical tables dict -> whitened one (whitened_tables with scales taken from those very tables); Engine.tables is its result."""
    import eftpipe_amd.engine as engine_mod

    real = engine_mod.build_tables
    monkeypatch.setattr(engine_mod, "build_tables", lambda cfg, loop_cache=None: whiten(real(cfg, loop_cache)))


def coef_half_ld(t, Pin, xi=False):
    """c = (Gc ; Ec) . [Pin | tail] in np.longdouble -> complex [NCH] (xi: Gc2 / Ec2 where the tables carry them).  The tails follow the
    reference formula (fftlog.py:140-151): a power law through the last two samples above the grid, through the first two below it."""
    ld = np.longdouble
    lnk, P = np.log(t["kin"].astype(ld)), np.asarray(Pin).astype(ld)
    lnx, nlo = t["lnx_tail"].astype(ld), int(t["ntail_lo"])
    nhi = lnx.size - nlo
    slope = (np.log(P[-1]) - np.log(P[-2])) / (lnk[-1] - lnk[-2])
    tail = P[-1] * np.exp(slope * (lnx[:nhi] - lnk[-1]))
    if nlo:
        slope = (np.log(P[1]) - np.log(P[0])) / (lnk[1] - lnk[0])
        tail = np.concatenate([tail, P[0] * np.exp(slope * (lnx[nhi:] - lnk[0]))])
    G, E = ("Gc2", "Ec2") if xi and "Gc2" in t else ("Gc", "Ec")
    v = t[G].astype(ld) @ P + t[E].astype(ld) @ tail
    return v[0] + 1j * v[1]


def coef_bound(t, Pin, xi=False):
    """The a-priori bound of a float64 evaluation of the same product in any order of summation: n u sum_j |G_mj| |x_j| per coefficient
    (n terms, u = 2^-53; re and im together).  The whitened edge rows are sums with 1e4-fold cancellation scaled up to modulus one, so their
    float64 value is good to 1e-13 only -- that, not the loop stages, is the floor of every comparison that starts from the operator."""
    lnk = np.log(t["kin"])
    lnx, nlo = t["lnx_tail"], int(t["ntail_lo"])
    nhi = lnx.size - nlo
    slope = (np.log(Pin[-1]) - np.log(Pin[-2])) / (lnk[-1] - lnk[-2])
    tail = Pin[-1] * np.exp(slope * (lnx[:nhi] - lnk[-1]))
    if nlo:
        slope = (np.log(Pin[1]) - np.log(Pin[0])) / (lnk[1] - lnk[0])
        tail = np.concatenate([tail, Pin[0] * np.exp(slope * (lnx[nhi:] - lnk[0]))])
    G, E = ("Gc2", "Ec2") if xi and "Gc2" in t else ("Gc", "Ec")
    a = np.abs(t[G]) @ np.abs(Pin) + np.abs(t[E]) @ np.abs(tail)
    return (Pin.size + tail.size) * 2.0**-53 * (a[0] + a[1])


def mirror(ch):
    """independent half [..., NCH] -> all NPOW = 2 NCH - 1 coefficients, c[NPOW - 1 - n] = conj c[n]"""
    return np.concatenate([ch, np.conj(ch[..., :-1][..., ::-1])], axis=-1)


def flat_scale(t, Pin, xi=False):
    """scale[m] = 1 / |c_m| of the spectrum Pin under the tables' operator: the whitened coefficients of Pin have modulus one for every m"""
    a = np.abs(coef_half_ld(t, Pin, xi))
    assert np.all(a > 0), "a coefficient of the fixture vanishes (edge window on? build with fft_window=None)"
    return np.asarray(1.0 / a, dtype=np.float64)


def mask(name, nch):
    """0 / 1 factors over m = 0 ... NCH - 1: the band of pairs / harmonics a masked set keeps"""
    m = np.arange(nch)
    return {"flat": np.ones(nch), "edge": (m <= 2) * 1.0, "centre": (m >= nch - 3) * 1.0, "even": (m % 2 == 0) * 1.0, "odd": (m % 2 == 1) * 1.0}[name]


def flatness(tw, Pin):
    """min_m |c'_m| / max_m |c'_m| over the rows a whitened operator keeps, of one spectrum (both coefficient sets where there are two)"""
    worst = 1.0
    for xi in (False, True):
        a = np.abs(coef_half_ld(tw, Pin, xi))
        a = a[a > 0]
        worst = min(worst, float(a.min() / a.max()))
    return worst


def near_fixture(draws, Pin0, lam):
    """The draws pulled towards the fixture spectrum along the geometric line, Pin0^(1 - lam) Pin^lam (lam = 1: the draws themselves).
    The high harmonics of P_lin are small differences of large terms: at NFFT = 512 a 10 % change of shape moves single coefficients by a
    factor of ten against the fixture's, and no common scale whitens such a batch; an eighth of the way keeps every draw within a factor of two."""
    out = dict(draws)
    out["Pin"] = np.ascontiguousarray(Pin0[None, :] ** (1.0 - lam) * draws["Pin"] ** lam)
    return out


NFFTS = (256, 258, 512)                      # the compiled-in size, an odd nh = 129 off the default ksyn / klin, the largest the engine runs
PULL = {256: 1.0, 258: 1.0, 512: 0.125}      # near_fixture's lam per size: the seeded draws themselves where they stay flat enough
FLAT_MIN = 0.5                               # a batch is fit for purpose if min_m |c'_m| / max_m |c'_m| >= FLAT_MIN for each of its cosmologies


def draw_set(NFFT, B, Pin0):
    """The first B of one seeded set of 70 draws (synth.draw_batch, z = 0.7), pulled towards the fixture spectrum Pin0 by PULL[NFFT]"""
    from eftpipe_amd import synth

    d = synth.draw_batch(70, z=0.7)
    d = {n: (v if n == "kin" else np.ascontiguousarray(v[:B])) for n, v in d.items()}
    return near_fixture(d, Pin0, PULL[NFFT])


# ----------------------------------------------------------------------------- the oracle on injected coefficients
class _Injected:
    """loop_coef of an OracleEngine variant: hands out the injected coefficient set the call asks for (pscf decides by IRcut which one)"""

    def __init__(self, ck, cs, k_is_cut):
        self.ck, self.cs, self.k_is_cut = ck, cs, k_is_cut

    def __call__(self, kin, Pin, window=0.2, IRcut=False):
        return self.ck if bool(IRcut) == self.k_is_cut else self.cs


def _variant(orc, fn, ck, cs, every=1, offset=0, cache=None):
    """A shallow copy of an OracleEngine whose loop matrices and power tables went through fn and whose loop_coef returns fn(ck) / fn(cs);
    every > 1: only the k and s of index offset, offset + every, ... (pscf evaluates its einsums on the engine's own grids).
    cache: a name under which the transformed matrices are kept on orc for the next call."""
    v = copy.copy(orc)
    v.cfg = copy.copy(orc.cfg)
    store = orc.__dict__.setdefault("_loop_synth_mats", {})
    mats = store.get(cache) or {n: fn(getattr(orc, n)) for n in _MATS}
    if cache is not None:
        store[cache] = mats
    for n in _MATS:
        setattr(v, n, mats[n])
    v.k, v.s = orc.k[offset::every], orc.s[offset::every]
    v.kPow, v.sPow = fn(orc.kPow[:, offset::every]), fn(orc.sPow[:, offset::every])
    mode = orc._ircutoff()
    v.loop_coef = _Injected(fn(ck), fn(ck if mode in ("all", False) else cs), mode in ("all", "loop"))
    return v


def oracle_pieces(orc, t, Pin, ld_every=0, every=1, offset=0):
    """The loop pieces of one spectrum under the (whitened) tables t, from the oracle's own pscf.
    -> dict(coef_k, coef_s: complex128 [NCH], the expected independent halves;  ref: {piece: float64 array};  abs: {piece: absolute-term sum};
            ld, ld_abs (ld_every > 0): the same sums in np.longdouble on every ld_every-th k and s)
    every, offset: ref and abs on the output points offset, offset + every, ... only (the cost of the oracle is per output point)."""
    ck, cs = coef_half_ld(t, Pin), coef_half_ld(t, Pin, xi=True)
    fk, fs = mirror(ck), mirror(cs)
    names = PIECES + (("CctNNLO",) if orc.cfg.with_NNLO else ())
    c128 = lambda a: np.asarray(a, dtype=np.complex128 if np.iscomplexobj(a) else np.float64)
    st = _variant(orc, c128, fk, fs, every, offset, cache="f64").pscf(t["kin"], Pin)
    ab = _variant(orc, lambda a: np.abs(c128(a)), fk, fs, every, offset, cache="abs").pscf(t["kin"], Pin)
    out = dict(coef_k=c128(ck), coef_s=c128(cs), ref={n: st[n] for n in names}, abs={n: ab[n] for n in names})
    if ld_every:
        cld = lambda a: np.asarray(a, dtype=np.clongdouble if np.iscomplexobj(a) else np.longdouble)
        st = _variant(orc, cld, fk, fs, ld_every).pscf(t["kin"], Pin)
        ab = _variant(orc, lambda a: np.abs(cld(a)), fk, fs, ld_every).pscf(t["kin"], Pin)
        out.update(ld={n: st[n] for n in names}, ld_abs={n: ab[n] for n in names}, ld_every=ld_every)
    return out


def expansion_scale(t, ab):
    """The absolute-term sums on the scale the DEVICE sums at.  P22, C22 and C13 are not summed from their own matrices: the 28 (10) loop matrices
    span 7 (2) dimensions (tables.loop_basis), the kernels sum the basis pieces and expand, piece_b = sum_c comb[b, c] basis_c.  Where a matrix
    is small against the basis matrices it is combined from -- rows 12, 20, 25 of M22 by a factor of 3000 to 5000 at the corner entries (n, m)
    near (0, N) -- rounding of the basis pieces and of comb itself (a least-squares fit, good to 1e-14) is that much larger against the
    piece's own absolute-term sum.  -> a copy of ab with sum_c |comb[b, c]| ab[basis_c] in the place of those three (>= ab, equal on basis rows)."""
    out = dict(ab)
    c22, b22 = np.abs(t["comb22"]), np.asarray(t["basis22"])
    out["P22"] = c22 @ ab["P22"][b22]
    if "comb13" in t:
        c13 = np.abs(t["comb13"])
        b13 = [int(np.argmin(np.abs(t["comb13"] - np.eye(c13.shape[1])[c][None, :]).max(axis=1))) for c in range(c13.shape[1])]
        assert np.allclose(t["comb13"][b13], np.eye(c13.shape[1]), atol=1e-12) and np.allclose(t["comb22"][b22], np.eye(c22.shape[1]), atol=1e-12)
        out["C22"] = np.einsum("bc,lcs->lbs", c22, ab["C22"][:, b22])
        out["C13"] = np.einsum("bc,lcs->lbs", c13, ab["C13"][:, b13])
    return out


def emulated_scale(t, Pin, coef, with_cf=True):
    """expansion_scale without the oracle (3 ms instead of 100 per cosmology): the device's own regrouping (emulate.pscf) run on absolute values --
    |ad|, |mlj|, |linvec|, |comb|, the synthesis bases with every phase at zero, |c'|.  coef: (k-space, xi-space) halves [2, NCH] as emulate
    takes them; Pin enters through P11 > 0 alone (P13 is a multiple of it)."""
    import emulate as E

    ta = dict(t)
    for n in ("ad", "mlj", "linvec", "comb22", "comb13", "expand_c"):
        if n in t:
            ta[n] = np.abs(t[n])
    for n in ("syn_k", "lin_k", "syn_s", "lin_s"):
        if n in t:
            K = (4 if n.startswith("syn") else 2) * (t["Gc"].shape[1] - 1) + 1
            a = np.zeros_like(t[n])
            a[0] = t[n][0]                  # row 0 is the amplitude x^power (tables.synthesis_table)
            a[1:K:2] = 2.0 * t[n][0]        # cos rows with the phase at zero; the sin rows stay empty
            ta[n] = a
    mod = tuple(np.stack([np.hypot(c[0], c[1]), np.zeros_like(c[0])]) for c in coef)
    return E.pscf(ta, Pin, with_cf, coef=mod)


def distance(got, want, abssum):
    """max over points of |got - want| / (absolute-term sum of that point)"""
    got, want, abssum = np.asarray(got), np.asarray(want), np.asarray(abssum)
    assert got.shape == want.shape == abssum.shape and np.all(abssum > 0)
    return float(np.max(np.abs(got - want) / abssum))


def oracle_for(Nl=3, NFFT=256, **over):
    """OracleEngine on the native k grid for the loop pieces (resummation tables are not needed for pscf)"""
    from oracle import OracleConfig, OracleEngine

    return OracleEngine(OracleConfig(Nl=Nl, NFFT=NFFT, **over))
