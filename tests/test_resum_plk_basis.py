"""Host checks of the closed-form basis of the direct-P_l resummation (tables.resum_plk_tables / resum_basis; device: resum_plk_kernel).

Every nonzero row of the coordinate table, for every power of f, is evaluated as the kernel does it -- -1/2 sum_j c_j b_j(-z/2) in float64 by the
kernel's recurrence -- and compared with the table polynomial sum_p q_p z^p evaluated in rationals.  The bar is 1e-13 of sum_p |q_p| z^p: the basis
form measured <= 1.6e-15 on a sample of rows at z <= 8 (Horner in float64: 2e-16), so the bar sits about 60 times above the method's own error and
four orders below the 1e-9 at which the direct path is compared with the templates-first one."""
from fractions import Fraction

import numpy as np
import pytest

from eftpipe_amd import loopmath as lm
from eftpipe_amd import tables as T

Z_POINTS = (0.05, 0.5, 1.0, 2.0, 3.0, 4.5, 6.0, 8.0)   # z = k^2 X(s): the GPU tests assert that their inputs stay below the largest of them
# ... and these are the small z of the lowest k (0.001: z near 1e-5) and of the few s where X(s) is slightly negative.  Near z = 0 a polynomial that
# starts at a higher power tends to zero while the rounding of its basis form does not, so there the error is measured against sum_p |q_p|: the rows
# are summed with weights of one order, and what counts is the error against the rows a row is summed with
Z_SMALL = (-0.05, 1e-8, 1e-5, 1e-3)
BAR = 1e-13
NIR, Na, Nl, NB = 16, 3, 3, 8


@pytest.fixture(scope="module")
def tabs():
    Qpoly = lm.q_polynomials(Nl)
    return Qpoly, T.resum_plk_tables(Qpoly, NIR, Na)


def _rows(Qpoly, QE):
    nf = Qpoly.shape[-1]
    q = Qpoly.reshape(2, Nl, Nl, 2, NIR, Na, nf).transpose(0, 1, 2, 3, 5, 6, 4).reshape(-1, NIR)   # (table, l, l', half, v, f-power) x p
    c = QE.reshape(2, Nl, Nl, 2, NB, Na, nf).transpose(0, 1, 2, 3, 5, 6, 4).reshape(-1, NB)        # the same rows x j
    return q, c


def test_basis_form_matches_table_polynomials(tabs):
    Qpoly, t = tabs
    q, c = _rows(Qpoly, t["QEpoly"])
    assert t["QEpoly"].shape == (2, Nl * Nl * 2 * NB * Na, Qpoly.shape[-1])
    nz = np.abs(q).max(axis=1) > 0
    assert nz.sum() > 100
    assert not np.any(c[~nz]), "a zero polynomial must keep zero coordinates"
    assert np.all(np.abs(c[nz]).max(axis=1) > 0)
    z = np.array(Z_POINTS)
    b = T.resum_basis(-0.5 * z)                                    # [8, nz]: the kernel's recurrence in float64
    got = -0.5 * np.einsum("rj,jz->rz", c[nz], b)                  # (the kernel folds the -1/2 into its coefficient record)
    worst = 0.0
    zf = [Fraction(float(x)) for x in z]
    for i, row in enumerate(q[nz]):
        qf = [Fraction(float(x)) for x in row]
        for iz, zz in enumerate(zf):
            exact, scale, zp = Fraction(0), Fraction(0), Fraction(1)
            for p in range(NIR):
                exact += qf[p] * zp
                scale += abs(qf[p]) * zp
                zp *= zz
            worst = max(worst, abs(float((Fraction(float(got[i, iz])) - exact) / scale)))
    print(f"basis form vs exact table polynomial: worst {worst:.3e} of sum_p |q_p| z^p over {int(nz.sum())} rows x {len(z)} z")
    assert worst < BAR, worst


def test_basis_form_at_small_z(tabs):
    Qpoly, t = tabs
    q, c = _rows(Qpoly, t["QEpoly"])
    nz = np.abs(q).max(axis=1) > 0
    z = np.array(Z_SMALL)
    got = -0.5 * np.einsum("rj,jz->rz", c[nz], T.resum_basis(-0.5 * z))
    worst = 0.0
    for i, row in enumerate(q[nz]):
        qf = [Fraction(float(x)) for x in row]
        scale = sum(abs(x) for x in qf)
        for iz, zz in enumerate(z):
            zz = Fraction(float(zz))
            exact = sum(qf[p] * zz**p for p in range(NIR))
            worst = max(worst, abs(float((Fraction(float(got[i, iz])) - exact) / scale)))
    print(f"basis form vs exact table polynomial at small z: worst {worst:.3e} of sum_p |q_p|")
    assert worst < BAR, worst


def test_reconstruction_bound_is_enforced(tabs):
    Qpoly, t = tabs
    assert 0.0 <= float(t["rse_worst"][0]) <= T.RSE_TOL
    bad = Qpoly.copy()
    i = np.argmax(np.abs(bad.reshape(2, Nl, Nl, 2, NIR, Na, -1)[..., 12, :, :]).reshape(-1))   # some nonzero coefficient of power 12 ...
    view = bad.reshape(2, Nl, Nl, 2, NIR, Na, -1)[..., 12, :, :]
    idx = np.unravel_index(i, view.shape)
    view[idx] *= 1.0 + 1e-6                                                                     # ... pushed out of the 8-dimensional space
    with pytest.raises(ValueError):
        T.resum_plk_tables(bad, NIR, Na)


# sha256 (first 16 hex digits) of the tables as the commit before the closed-form basis built them.  Exact data: the Q polynomials come from a
# data file, the Nl = 2 basis is the identity scaled by powers of 8, the row tables are integers.  (The Nl = 3 basis of the matrix-core kernel is an
# SVD, whose last bits belong to the LAPACK build: it is compared with what resum_mfma_tables returns on its own.)
DIGESTS = {(2, "Qpoly"): "7ed50fa565dd25d3", (2, "rs_basis"): "b2d8a2cb31d9a5b8", (2, "rs_basis_scaled"): "a56937ac17f8edd4", (2, "rs_rows"): "d8c36ab87e59348b",
           (3, "Qpoly"): "f34692f896f284ae", (3, "rs_rows"): "9af983dd3c3d4e85"}


def test_other_tables_unchanged():
    import hashlib

    digest = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]
    for nl, nir, na in ((2, 8, 2), (3, NIR, Na)):
        t = T.build_tables(T.EngineConfig(Nl=nl, with_resum=True))
        alone = T.resum_mfma_tables(lm.q_polynomials(nl), nir, na)
        assert set(alone) == {"rs_basis", "rs_basis_scaled", "rs_rows"}
        for name in alone:   # what the engine uploads is what the untouched function returns: nothing of the new table leaks into them
            assert t[name].dtype == alone[name].dtype and t[name].tobytes() == alone[name].tobytes(), (nl, name)
        for (n, name), want in DIGESTS.items():
            if n == nl:
                assert digest(t[name]) == want, (nl, name)
        assert ("QEpoly" in t) == (nl == 3)   # Nl = 2 has no direct path: no coordinate table
    with pytest.raises(ValueError):
        T.resum_plk_tables(lm.q_polynomials(2), 8, 2)
