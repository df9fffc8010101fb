"""Loop FFTLog sizes other than 256 and input grids that start above the FFTLog's xmin = 1.5e-5, on the host (no GPU):
the tables the device consumes at NFFT = 384 / 512, the anti-diagonal regrouping at a size other than 256, the low-k power-law tails
against the REAL reference (tests/golden/fftlog.npz, tools/make_fixtures.py fftlog), and the refusals of the sizes the engine does not run."""
import numpy as np
import pytest

from conftest import relerr
from eftpipe_amd import loopmath as lm
from eftpipe_amd.tables import EngineConfig, antidiagonal_tables, build_tables, loop_basis

KIN_LO = np.logspace(-4, 0, 200)


def kpad(n, m=48):
    return (n + m - 1) // m * m


@pytest.mark.parametrize("NFFT", [384, 512])
def test_build_tables_shapes(NFFT):
    nh, npow, nch = NFFT // 2, NFFT + 1, NFFT // 2 + 1
    for kin in (None, KIN_LO):
        cfg = EngineConfig(Nl=3, NFFT=NFFT, kin=kin, with_resum=True, with_ap=True, DA_AP=1.0, H_AP=1.0, with_NNLO=True)
        t = build_tables(cfg)
        Nk, Nkin, ntail = t["k"].size, t["kin"].size, t["lnx_tail"].size
        assert t["Gc"].shape == (2, nch, Nkin) and t["Ec"].shape == (2, nch, ntail)
        assert t["ad"].shape == (t["comb22"].shape[1] + t["comb13"].shape[1], npow, nh + 2)
        assert t["mlj"].shape == (3, npow) and t["linvec"].shape == (10 + 3 * 3, nch)
        assert t["syn_k"].shape == (kpad(4 * nh + 1), Nk) and t["lin_k"].shape == (kpad(2 * nh + 1), Nk)
        assert t["syn_s"].shape == (kpad(4 * nh + 1), 80) and t["lin_s"].shape == (kpad(2 * nh + 1), 80)
        assert t["comb22"].shape[1] == 7
        lo = kin is not None
        assert (t["ntail_lo"] > 0) == lo and (t["nxtail_lo"] > 0) == lo
        assert t["wq_last2"].shape == ((4,) if lo else (2,))
        assert t["TX"].shape == (80, t["lnx_xtail"].size)


def test_default_tables_keep_their_shapes():
    t = build_tables(EngineConfig(Nl=3, with_resum=True, with_ap=True, DA_AP=1.0, H_AP=1.0))
    assert t["Gc"].shape[1] == 129 and t["ad"].shape[1:] == (257, 130) and t["syn_k"].shape[0] == 528 and t["lin_k"].shape[0] == 288
    assert t["ntail_lo"] == 0 and t["nxtail_lo"] == 0 and t["wq_last2"].shape == (2,)


def test_antidiagonal_tables_match_the_double_sum_at_384():
    N = 384
    dx = np.log(1000.0 / 1.5e-5) / (N - 1.0)
    Pow = -1.6 + 1j * 2.0 * np.pi / (N * dx) * (np.arange(N + 1) - N / 2.0)
    M22 = lm.matrices_22(-0.5 * Pow)
    basis, _ = loop_basis(M22)
    M = M22[basis[:3]]
    V = lm.vectors_13(-0.5 * Pow)[:2]
    AD = antidiagonal_tables(M, V)
    rng = np.random.default_rng(7)
    half = rng.normal(size=N // 2 + 1) + 1j * rng.normal(size=N // 2 + 1)
    half[-1] = half[-1].real
    c = np.concatenate([half, np.conj(half[:-1][::-1])])     # c_{N - n} = conj(c_n), as the FFTLog of a real function
    k = np.array([0.01, 0.1, 0.25])
    x = c[None, :] * np.exp(np.outer(np.log(k), Pow))          # x_n(k) = c_n k^Pow_n
    mats = list(M) + [v[:, None] * np.ones((1, N + 1)) for v in V]
    for q, Mq in enumerate(mats):
        direct = np.real(np.einsum("kn,nm,km->k", x, Mq, x))
        # S[j'] = sum_t c_{j'+t} c_{N-t} AD[q, j', t]; the sum over j' = -N..N of k^{2 bias + i dpow j'} S[j'] is real: 2 Re (j' > 0) + j' = 0
        S = np.array([np.sum(c[jp + np.arange(AD.shape[2])[: (N + jp) // 2 - jp + 1]] *
                             c[N - np.arange((N + jp) // 2 - jp + 1)] * AD[q, jp, : (N + jp) // 2 - jp + 1]) for jp in range(N + 1)])
        dpow = 2.0 * np.pi / (N * dx)
        kp = np.exp(np.outer(np.log(k), 2.0 * -1.6 + 1j * dpow * np.arange(N + 1)))
        regrouped = np.real(kp[:, 0] * S[0]) + 2.0 * np.real(kp[:, 1:] @ S[1:])
        assert np.max(np.abs(regrouped - direct)) <= 1e-13 * np.max(np.abs(direct)), q


def host_tail(vals, lnk, lnx, end):
    """power law through the first (end = 0) or last (end = -1) two samples of `vals`, evaluated at exp(lnx) (reference fftlog.py:140-151)"""
    i0, i1 = (0, 1) if end == 0 else (-2, -1)
    slope = (np.log(vals[i1]) - np.log(vals[i0])) / (lnk[i1] - lnk[i0])
    return vals[i1] * np.exp(slope * (lnx - lnk[i1]))


def host_coef(t, Pin):
    """the device's first-stage product [Pin | high tail | low tail] . (Gc ; Ec) -> the NFFT/2 + 1 independent coefficients"""
    lnk, nlo = np.log(t["kin"]), t["ntail_lo"]
    lnx = t["lnx_tail"]
    nhi = lnx.size - nlo
    tail = np.concatenate([host_tail(Pin, lnk, lnx[:nhi], -1), host_tail(Pin, lnk, lnx[nhi:], 0)])
    G = t["Gc"][0] + 1j * t["Gc"][1]
    E = t["Ec"][0] + 1j * t["Ec"][1]
    return G @ Pin + E @ tail


def host_xy(t, Pin):
    lnk = np.log(t["kin"])
    wq = np.exp(-(t["kin"] ** 2) / 0.2**2) / t["kin"] ** 2
    q = Pin * wq
    lnx, nlo = t["lnx_xtail"], t["nxtail_lo"]
    nhi = lnx.size - nlo
    tail = np.concatenate([host_tail(q, lnk, lnx[:nhi], -1), host_tail(q, lnk, lnx[nhi:], 0)])
    return t["BX"] @ Pin + t["TX"] @ tail, t["BY"] @ Pin + t["TY"] @ tail


@pytest.mark.parametrize("case,NFFT,ircut", [("lo256", 256, False), ("lo512", 512, False), ("lo512loop", 512, "loop")])
def test_low_k_tails_match_the_reference(golden, case, NFFT, ircut):
    g = golden("fftlog")
    cfg = EngineConfig(Nl=3, NFFT=NFFT, kin=g["kin_lo"], with_resum=True, IRcutoff=ircut, kIR=float(g["kIR"]) if ircut else None)
    t = build_tables(cfg)
    assert t["ntail_lo"] > 0 and t["nxtail_lo"] > 0
    want = g[case + "_coef"]
    nch = NFFT // 2 + 1
    # Coef without IR cut: the first coefficient set ("loop" cuts the k-space set, the xi-space set Gc2 is the plain one)
    if ircut == "loop":
        t = dict(t, Gc=t["Gc2"], Ec=t["Ec2"])
    assert relerr(host_coef(t, g["Pin_lo"]), want[:nch]) < 1e-12
    X, Y = host_xy(t, g["Pin_lo"])
    assert relerr(X, g[case + "_X"]) < 1e-12 and relerr(Y, g[case + "_Y"]) < 1e-12


def test_ir_cut_coefficient_set_pads_the_low_end():
    # IRcutoff="loop": the k-space set is the cut one, ("padding", "extrap"); the xi-space set continues P_lin below kin[0] (pybird.py:1127-1160)
    t = build_tables(EngineConfig(Nl=3, with_resum=True, IRcutoff="loop", kIR=0.004, kin=KIN_LO))
    assert t["ntail_lo"] > 0
    assert np.all(t["Ec"][:, :, -t["ntail_lo"]:] == 0.0)
    assert np.any(t["Ec2"][:, :, -t["ntail_lo"]:] != 0.0)


def test_refusals():
    from eftpipe_amd import pybird

    co = pybird.Common(Nl=3)
    with pytest.raises(NotImplementedError):
        pybird.NonLinear(load=False, save=False, NFFT=128, co=co)
    for bad in (257, 1024, 514):
        with pytest.raises(ValueError, match="256 to 512"):
            pybird.NonLinear(load=False, save=False, NFFT=bad, co=co)
    for bad in (255, 600):
        with pytest.raises(ValueError, match="256 to 512"):
            build_tables(EngineConfig(Nl=2, NFFT=bad))
    with pytest.raises(ValueError, match="above the first k"):
        build_tables(EngineConfig(Nl=2, kin=np.logspace(-1.5, 0, 200)))
