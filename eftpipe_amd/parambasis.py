"""Bias contraction onto P_l(k): host mirror of reference eftpipe/parambasis.py:42-136 and of its two parameter
bases (WestCoastBasis :166-316, EastCoastBasis :320-454).

``bias_vectors`` builds the 3 + 6 + 12 + 3 coefficient vectors; the
contraction itself runs on the device (``reduce_kernel``) when driven through ``Engine`` and is a
24-term dot product per (l, k).  ``reduce_Plk`` keeps the reference signature for BirdLike objects.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np


@dataclass
class BirdComponent:
    """Same record as reference parambasis.py:30-39."""

    Plin: np.ndarray
    Ploop: np.ndarray
    Pct: np.ndarray
    Pst: np.ndarray
    Picc: np.ndarray

    def sum(self):
        return self.Plin + self.Ploop + self.Pct + self.Pst + self.Picc


def bias_vectors(f, bsA, bsB=None, es=(0.0, 0.0, 0.0), kmA=0.7, krA=0.25, ndA=3e-4, kmB=None, krB=None, ndB=None,
                 counterform="westcoast"):
    """-> b11[3], bct[6], bloop[12], bst[3] (reference parambasis.py:69-126; counterform 'eastcoast' reads the last
    three entries of bsA/bsB as ctilde_0, ctilde_2, ctilde_4, :93-102)."""
    kmB = kmA if kmB is None else kmB
    krB = krA if krB is None else krB
    ndB = ndA if ndB is None else ndB
    b1A, b2A, b3A, b4A, cctA, cr1A, cr2A = bsA
    b1B, b2B, b3B, b4B, cctB, cr1B, cr2B = bsB if bsB is not None else bsA
    ce0, cemono, cequad = es
    b11 = np.array([b1A * b1B, (b1A + b1B) * f, f * f])
    if counterform not in ("westcoast", "eastcoast"):
        raise ValueError(f"unexpected counterform: {counterform}")
    bct = np.array([-cctA - cctB, -(cr1A + cr1B) * f, -(cr2A + cr2B) * f**2, 0.0, 0.0, 0.0]) if counterform == "eastcoast" else np.array([
        b1A * cctB / kmB**2 + b1B * cctA / kmA**2,
        b1B * cr1A / krA**2 + b1A * cr1B / krB**2,
        b1B * cr2A / krA**2 + b1A * cr2B / krB**2,
        (cctA / kmA**2 + cctB / kmB**2) * f,
        (cr1A / krA**2 + cr1B / krB**2) * f,
        (cr2A / krA**2 + cr2B / krB**2) * f,
    ])
    bloop = np.array([
        1.0, 0.5 * (b1A + b1B), 0.5 * (b2A + b2B), 0.5 * (b3A + b3B), 0.5 * (b4A + b4B), b1A * b1B,
        0.5 * (b1A * b2B + b1B * b2A), 0.5 * (b1A * b3B + b1B * b3A), 0.5 * (b1A * b4B + b1B * b4A),
        b2A * b2B, 0.5 * (b2A * b4B + b2B * b4A), b4A * b4B,
    ])
    x1 = 0.5 * (1.0 / ndA + 1.0 / ndB)
    x2 = 0.5 * (1.0 / ndA / kmA**2 + 1.0 / ndB / kmB**2)
    bst = np.array([ce0 * x1, cemono * x2, cequad * x2])
    return b11, bct, bloop, bst


def bias_row(f, bsA, bsB=None, es=(0.0, 0.0, 0.0), **scales):
    """The 24 coefficients in template-row order (P11l, Pctl, Ploopl, Pstl) for the device reduce."""
    return np.concatenate(bias_vectors(f, bsA, bsB, es, **scales))


def nnlo_vector(f, b1A, cnnloA, krA=0.25, counterform="westcoast"):
    """bctNNLOAB[3] (reference parambasis.py:96-106): west coast cnnloA = (cr4, cr6); east coast (ctilde, _).
    These are the EFTB_B_BIASN coefficients of the device reduce."""
    if counterform == "westcoast":
        cr4, cr6 = cnnloA
        return np.array([1 / 4 * b1A**2 / krA**4 * cr4, 1 / 4 * b1A / krA**4 * cr6, 0.0])
    ctilde = cnnloA[0]
    return ctilde * np.array([-(b1A**2) * f**4, -2 * b1A * f**5, -(f**6)])


def reduce_Plk(bird, bsA, bsB=None, es=(0.0, 0.0, 0.0), cnnloA=(0.0, 0.0), cnnloB=None):
    """BirdLike -> BirdComponent (reference parambasis.py:42-136; the counter-term form is bird.co.counterform; with
    bird.co.with_NNLO the k^4 counter-terms bctNNLO . PctNNLOl are added to Pct)."""
    co = bird.co
    b11, bct, bloop, bst = bias_vectors(bird.f, list(bsA), None if bsB is None else list(bsB), tuple(es),
                                        kmA=co.kmA, krA=co.krA, ndA=co.ndA, kmB=co.kmB, krB=co.krB, ndB=co.ndB,
                                        counterform=getattr(co, "counterform", "westcoast"))
    No = co.No
    return BirdComponent(
        Plin=np.einsum("b,lbx->lx", b11, bird.P11l[:No]),
        Ploop=np.einsum("b,lbx->lx", bloop, bird.Ploopl[:No]),
        Pct=np.einsum("b,lbx->lx", bct, bird.Pctl[:No])
        + (np.einsum("b,lbx->lx", nnlo_vector(bird.f, list(bsA)[0], tuple(cnnloA), co.krA, getattr(co, "counterform", "westcoast")),
                     bird.PctNNLOl[:No]) if getattr(co, "with_NNLO", False) else 0.0),
        Pst=np.einsum("b,lbx->lx", bst, bird.Pstl[:No]),
        Picc=bird.Picc[:No],
    )


# ----------------------------------------------------------------------------- Gaussian table
GAUSSIAN = ("b3", "cct", "cr1", "cr2")
STOCHASTIC = ("ce0", "cemono", "cequad")


def gaussian_params(prefix="", cross_prefix=()):
    """Names of the analytically marginalisable parameters, in table order (reference parambasis.py:209-223)."""
    if cross_prefix:
        return [x + p for x in cross_prefix for p in GAUSSIAN] + [prefix + p for p in STOCHASTIC]
    return [prefix + p for p in GAUSSIAN + STOCHASTIC]


def _sparse_row(pairs):
    """24 coefficients, zero but for the (index, value) pairs; the values are floats, or the polynomials of the recipe compiler"""
    r = np.zeros(24, dtype=object if any(isinstance(c, _Poly) for _, c in pairs) else np.float64)
    for i, c in pairs:
        r[i] = c
    return r


def gaussian_rows(f, ngA, ngB=None, kmA=0.7, krA=0.25, ndA=3e-4, kmB=None, krB=None, ndB=None, basis="westcoast"):
    """Coefficient rows over the 24 template rows (P11l[3], Pctl[6], Ploopl[12], Pstl[3]) of

        row 0        P_NG: the model with every Gaussian parameter at 0 (reference likelihood.py:524-549 via reduce_Plk)
        rows 1..nG   dP/d(gaussian parameter) in the order of ``gaussian_params`` (reference parambasis.py:249-316)

    for the non-Gaussian parameters ngA = (b1, b2, b4) [and ngB for a cross spectrum].  Everything downstream of the
    templates is linear in these rows, so the device builds P_NG and P_G with one small contraction per walker.
    basis="eastcoast": ngA = (b1, b2, bG2), rows in the order of EastCoastBasis.gaussian_params (reference :413-444)."""
    if basis == "eastcoast":
        if ngB is not None:
            raise NotImplementedError("EastCoastBasis does not support cross yet")
        return _eastcoast_rows(f, ngA, kmA, krA, ndA)
    if basis != "westcoast":
        raise ValueError(f"unexpected basis: {basis}")
    cross = ngB is not None
    kmB = kmA if kmB is None else kmB
    krB = krA if krB is None else krB
    ndB = ndA if ndB is None else ndB
    b1A, b2A, b4A = ngA
    b1B, b2B, b4B = ngB if cross else ngA
    bsA = [b1A, b2A, 0.0, b4A, 0.0, 0.0, 0.0]
    bsB = [b1B, b2B, 0.0, b4B, 0.0, 0.0, 0.0] if cross else None
    rows = [bias_row(f, bsA, bsB, (0.0, 0.0, 0.0), kmA=kmA, krA=krA, ndA=ndA, kmB=kmB, krB=krB, ndB=ndB)]
    row = _sparse_row
    if cross:
        for b1o, km, kr in ((b1B, kmA, krA), (b1A, kmB, krB)):
            rows.append(row([(LOOP + 3, 0.5), (LOOP + 7, 0.5 * b1o)]))
            rows.append(row([(CT + 0, b1o / km**2), (CT + 3, f / km**2)]))
            rows.append(row([(CT + 1, b1o / kr**2), (CT + 4, f / kr**2)]))
            rows.append(row([(CT + 2, b1o / kr**2), (CT + 5, f / kr**2)]))
    else:
        rows.append(row([(LOOP + 3, 1.0), (LOOP + 7, b1A)]))
        rows.append(row([(CT + 0, 2.0 * b1A / kmA**2), (CT + 3, 2.0 * f / kmA**2)]))
        rows.append(row([(CT + 1, 2.0 * b1A / krA**2), (CT + 4, 2.0 * f / krA**2)]))
        rows.append(row([(CT + 2, 2.0 * b1A / krA**2), (CT + 5, 2.0 * f / krA**2)]))
    x1 = 0.5 * (1.0 / ndA + 1.0 / ndB)
    x2 = 0.5 * (1.0 / ndA / kmA**2 + 1.0 / ndB / kmB**2)
    rows += [row([(ST + 0, x1)]), row([(ST + 1, x2)]), row([(ST + 2, x2)])]
    return np.stack(rows)


# ----------------------------------------------------------------------------- many draws at once (Engine.reduce_draws, MarginalLikelihood.logp_draws)
# The same arithmetic as bias_vectors / gaussian_rows, element by element over N parameter draws: draw i of a *_many builder has the bits
# of the scalar builder called with Python floats for draw i.  Per-draw powers go through _powu: numpy's array power (a square, or its own
# vector pow) and libm's pow, which a Python float uses, differ in the last bit for some arguments.


def _draws(x, N, name, width=None):
    """x as float64 [N] (or [N, width]); a scalar / one row is shared by every draw"""
    a = np.asarray(x, dtype=np.float64)
    shape = (N,) if width is None else (N, width)
    try:
        return np.broadcast_to(a, shape)
    except ValueError:
        raise ValueError(f"{name} must be {'[N]' if width is None else f'[N, {width}]'} (N = {N}), got {a.shape}") from None


def _powu(x, p):
    """x ** p per element with the arithmetic of a Python float; evaluated once per distinct value (draws of one walker share its growth rate)"""
    u, inv = np.unique(x, return_inverse=True)
    return np.array([float(v) ** p for v in u.tolist()])[inv].reshape(x.shape)


def _ndraws(*arrays):
    sizes = {np.asarray(a).shape[0] for a in arrays if a is not None and np.ndim(a) >= 1}
    if len(sizes) != 1:
        raise ValueError(f"the per-draw arrays disagree on the number of draws: {sorted(sizes)}")
    return sizes.pop()


def bias_rows_many(f, bsA, bsB=None, es=(0.0, 0.0, 0.0), kmA=0.7, krA=0.25, ndA=3e-4, kmB=None, krB=None, ndB=None, counterform="westcoast"):
    """bias_row for N draws: f [N] (or one value), bsA [N, 7], bsB [N, 7] or None, es [N, 3] or one triple -> [N, 24]."""
    if np.ndim(bsA) != 2 or (bsB is not None and np.ndim(bsB) != 2):
        raise ValueError("bsA / bsB must be [N, 7]")
    N = _ndraws(bsA)
    f = _draws(f, N, "f")
    bsA = _draws(bsA, N, "bsA", 7)
    bsB = bsA if bsB is None else _draws(bsB, N, "bsB", 7)
    es = _draws(es, N, "es", 3)
    kmB = kmA if kmB is None else kmB
    krB = krA if krB is None else krB
    ndB = ndA if ndB is None else ndB
    b1A, b2A, b3A, b4A, cctA, cr1A, cr2A = bsA.T
    b1B, b2B, b3B, b4B, cctB, cr1B, cr2B = bsB.T
    ce0, cemono, cequad = es.T
    b11 = [b1A * b1B, (b1A + b1B) * f, f * f]
    if counterform not in ("westcoast", "eastcoast"):
        raise ValueError(f"unexpected counterform: {counterform}")
    bct = [-cctA - cctB, -(cr1A + cr1B) * f, -(cr2A + cr2B) * _powu(f, 2), 0.0, 0.0, 0.0] if counterform == "eastcoast" else [
        b1A * cctB / kmB**2 + b1B * cctA / kmA**2,
        b1B * cr1A / krA**2 + b1A * cr1B / krB**2,
        b1B * cr2A / krA**2 + b1A * cr2B / krB**2,
        (cctA / kmA**2 + cctB / kmB**2) * f,
        (cr1A / krA**2 + cr1B / krB**2) * f,
        (cr2A / krA**2 + cr2B / krB**2) * f,
    ]
    bloop = [
        1.0, 0.5 * (b1A + b1B), 0.5 * (b2A + b2B), 0.5 * (b3A + b3B), 0.5 * (b4A + b4B), b1A * b1B,
        0.5 * (b1A * b2B + b1B * b2A), 0.5 * (b1A * b3B + b1B * b3A), 0.5 * (b1A * b4B + b1B * b4A),
        b2A * b2B, 0.5 * (b2A * b4B + b2B * b4A), b4A * b4B,
    ]
    x1 = 0.5 * (1.0 / ndA + 1.0 / ndB)
    x2 = 0.5 * (1.0 / ndA / kmA**2 + 1.0 / ndB / kmB**2)
    bst = [ce0 * x1, cemono * x2, cequad * x2]
    out = np.empty((N, 24))
    for r, v in enumerate(b11 + bct + bloop + bst):
        out[:, r] = v
    return out


def gaussian_rows_many(f, ngA, ngB=None, kmA=0.7, krA=0.25, ndA=3e-4, kmB=None, krB=None, ndB=None, basis="westcoast"):
    """gaussian_rows for N draws: f [N] (or one value), ngA [N, 3] (and ngB [N, 3] for a cross spectrum) -> [N, nG + 1, 24]."""
    if np.ndim(ngA) != 2 or (ngB is not None and np.ndim(ngB) != 2):
        raise ValueError("ngA / ngB must be [N, 3]")
    N = _ndraws(ngA, ngB)
    f = _draws(f, N, "f")
    ngA = _draws(ngA, N, "ngA", 3)
    zero = np.zeros(N)
    if basis == "eastcoast":
        if ngB is not None:
            raise NotImplementedError("EastCoastBasis does not support cross yet")
        b1, b2, bG2 = ngA.T
        f2 = _powu(f, 2)
        c0 = c2 = c4 = bGamma3 = 0.0
        bsA = np.stack([b1, b1 + 7 / 2 * bG2, b1 + 15 * bG2 + 6 * bGamma3, 1 / 2 * b2 - 7 / 2 * bG2,
                        c0 - f / 3 * c2 + 3 / 35 * f2 * c4, c2 - 6 / 7 * f * c4, c4 + zero], axis=1)  # eastcoast_to_bs
        Pshot = a0 = a2 = 0.0
        es = np.stack([Pshot + zero, a0 + 1 / 3 * a2 + zero, 2 / 3 * a2 + zero], axis=1)
        out = np.zeros((N, 8, 24))
        out[:, 0] = bias_rows_many(f, bsA, None, es, counterform="eastcoast", kmA=kmA, krA=krA, ndA=ndA)
        out[:, 1, LOOP + 3], out[:, 1, LOOP + 7] = 6.0, 6.0 * b1                                        # bGamma3
        out[:, 2, CT + 0] = -2.0                                                                       # c0
        out[:, 3, CT + 0], out[:, 3, CT + 1] = 2 / 3 * f, -2.0 * f                                     # c2
        out[:, 4, CT + 0], out[:, 4, CT + 1], out[:, 4, CT + 2] = -6 / 35 * f2, 12 / 7 * f2, -2.0 * f2  # c4
        x1 = 1.0 / ndA
        x2 = 1.0 / ndA / kmA**2
        out[:, 5, ST + 0] = x1                                                                         # Pshot
        out[:, 6, ST + 1] = x2                                                                         # a0
        out[:, 7, ST + 1], out[:, 7, ST + 2] = x2 / 3, 2 * x2 / 3                                      # a2
        return out
    if basis != "westcoast":
        raise ValueError(f"unexpected basis: {basis}")
    cross = ngB is not None
    kmB = kmA if kmB is None else kmB
    krB = krA if krB is None else krB
    ndB = ndA if ndB is None else ndB
    b1A, b2A, b4A = ngA.T
    b1B, b2B, b4B = _draws(ngB, N, "ngB", 3).T if cross else (b1A, b2A, b4A)
    bsA = np.stack([b1A, b2A, zero, b4A, zero, zero, zero], axis=1)
    bsB = np.stack([b1B, b2B, zero, b4B, zero, zero, zero], axis=1) if cross else None
    out = np.zeros((N, 12 if cross else 8, 24))
    out[:, 0] = bias_rows_many(f, bsA, bsB, (0.0, 0.0, 0.0), kmA=kmA, krA=krA, ndA=ndA, kmB=kmB, krB=krB, ndB=ndB)
    g = 1
    if cross:
        for b1o, km, kr in ((b1B, kmA, krA), (b1A, kmB, krB)):
            out[:, g, LOOP + 3], out[:, g, LOOP + 7] = 0.5, 0.5 * b1o
            out[:, g + 1, CT + 0], out[:, g + 1, CT + 3] = b1o / km**2, f / km**2
            out[:, g + 2, CT + 1], out[:, g + 2, CT + 4] = b1o / kr**2, f / kr**2
            out[:, g + 3, CT + 2], out[:, g + 3, CT + 5] = b1o / kr**2, f / kr**2
            g += 4
    else:
        out[:, 1, LOOP + 3], out[:, 1, LOOP + 7] = 1.0, b1A
        out[:, 2, CT + 0], out[:, 2, CT + 3] = 2.0 * b1A / kmA**2, 2.0 * f / kmA**2
        out[:, 3, CT + 1], out[:, 3, CT + 4] = 2.0 * b1A / krA**2, 2.0 * f / krA**2
        out[:, 4, CT + 2], out[:, 4, CT + 5] = 2.0 * b1A / krA**2, 2.0 * f / krA**2
        g = 5
    x1 = 0.5 * (1.0 / ndA + 1.0 / ndB)
    x2 = 0.5 * (1.0 / ndA / kmA**2 + 1.0 / ndB / kmB**2)
    out[:, g, ST + 0], out[:, g + 1, ST + 1], out[:, g + 2, ST + 2] = x1, x2, x2
    return out


# ----------------------------------------------------------------------------- parameter bases
CT, LOOP, ST = 3, 9, 21  # first template row of Pctl, Ploopl, Pstl in the 24-row order


def eastcoast_to_bs(f, b1, b2, bG2, bGamma3, c0, c2, c4, Pshot=0.0, a0=0.0, a2=0.0):
    """East-coast parameters -> (bsA, es) of reduce_Plk with counterform='eastcoast' (reference parambasis.py:378-397)."""
    bsA = [b1, b1 + 7 / 2 * bG2, b1 + 15 * bG2 + 6 * bGamma3, 1 / 2 * b2 - 7 / 2 * bG2,
           c0 - f / 3 * c2 + 3 / 35 * f**2 * c4, c2 - 6 / 7 * f * c4, c4]
    es = [Pshot, a0 + 1 / 3 * a2, 2 / 3 * a2]
    return bsA, es


def eastcoast_bias_row(f, b1, b2, bG2, bGamma3=0.0, c0=0.0, c2=0.0, c4=0.0, Pshot=0.0, a0=0.0, a2=0.0, **scales):
    """The 24 device-reduce coefficients for east-coast parameters (arxiv 2106.12580 convention of the reference)."""
    bsA, es = eastcoast_to_bs(f, b1, b2, bG2, bGamma3, c0, c2, c4, Pshot, a0, a2)
    return bias_row(f, bsA, None, es, counterform="eastcoast", **scales)


def _eastcoast_rows(f, ng, kmA, krA, ndA):
    b1, b2, bG2 = ng
    rows = [eastcoast_bias_row(f, b1, b2, bG2, kmA=kmA, krA=krA, ndA=ndA)]
    row = _sparse_row
    rows.append(row([(LOOP + 3, 6.0), (LOOP + 7, 6.0 * b1)]))                                      # bGamma3
    rows.append(row([(CT + 0, -2.0)]))                                                             # c0
    rows.append(row([(CT + 0, 2 / 3 * f), (CT + 1, -2.0 * f)]))                                    # c2
    rows.append(row([(CT + 0, -6 / 35 * f**2), (CT + 1, 12 / 7 * f**2), (CT + 2, -2.0 * f**2)]))   # c4
    x1 = 1.0 / ndA
    x2 = 1.0 / ndA / kmA**2
    rows.append(row([(ST + 0, x1)]))                                                               # Pshot
    rows.append(row([(ST + 1, x2)]))                                                               # a0
    rows.append(row([(ST + 1, x2 / 3), (ST + 2, 2 * x2 / 3)]))                                     # a2
    return np.stack(rows)


def _table_from_rows(bird, rows, names, requires):
    No = bird.co.No
    T = np.concatenate([bird.P11l[:No], bird.Pctl[:No], bird.Ploopl[:No], bird.Pstl[:No]], axis=1)  # [No, 24, nx]
    return {p: np.einsum("b,lbx->lx", r, T) for p, r in zip(names, rows) if requires is None or p in requires}


@dataclass(frozen=True)
class WestCoastBasis:
    """Same surface as reference parambasis.py:166-316 (b1 b2 b3 b4 cct cr1 cr2 | ce0 cemono cequad)."""

    prefix: str = ""
    cross_prefix: list = field(default_factory=list)

    def default(self):
        return {p: 0.0 for p in self.gaussian_params()}

    def bsA(self):
        prefix = self.cross_prefix[0] if self.is_cross() else self.prefix
        return [prefix + p for p in ("b1", "b2", "b3", "b4", "cct", "cr1", "cr2")]

    def bsB(self):
        return [self.cross_prefix[1] + p for p in ("b1", "b2", "b3", "b4", "cct", "cr1", "cr2")] if self.is_cross() else []

    def es(self):
        return [self.prefix + p for p in STOCHASTIC]

    def cnnloA(self):
        return [self.prefix + p for p in ("cr4", "cr6")]

    def is_cross(self):
        return bool(self.cross_prefix)

    @classmethod
    def get_name(cls):
        return "westcoast"

    @classmethod
    def counterform(cls):
        return "westcoast"

    def non_gaussian_params(self):
        names = ("b1", "b2", "b4")
        if self.is_cross():
            return [x + p for x in self.cross_prefix for p in names]
        return [self.prefix + p for p in names]

    def gaussian_params(self):
        if self.is_cross():
            return gaussian_params(self.prefix, self.cross_prefix)
        return gaussian_params(self.prefix) + self.cnnloA()  # the NNLO names never enter the table (as the reference)

    def reduce_Plk(self, bird, params_values_dict):
        v = self.default()
        v.update(params_values_dict)
        cnnloA = [v[p] for p in self.cnnloA()] if getattr(bird.co, "with_NNLO", False) else (0.0, 0.0)
        return reduce_Plk(bird, [v[p] for p in self.bsA()], [v[p] for p in self.bsB()] or None, [v[p] for p in self.es()], cnnloA)

    def nnlo_row(self, f, params_values_dict, krA=0.25):
        """EFTB_B_BIASN coefficients (cr4, cr6) for one walker"""
        v = self.default()
        v.update(params_values_dict)
        return nnlo_vector(f, v[self.bsA()[0]], [v[p] for p in self.cnnloA()], krA, "westcoast")

    def bias_row(self, f, params_values_dict, **scales):
        """Device-reduce coefficients for one walker (the batched counterpart of reduce_Plk)."""
        v = self.default()
        v.update(params_values_dict)
        return bias_row(f, [v[p] for p in self.bsA()], [v[p] for p in self.bsB()] or None, [v[p] for p in self.es()], **scales)

    def gaussian_rows(self, f, params_values_dict, **scales):
        ng = [[params_values_dict[x + p] for p in ("b1", "b2", "b4")] for x in (self.cross_prefix or [self.prefix])]
        return gaussian_rows(f, ng[0], ng[1] if self.is_cross() else None, **scales)

    def reduce_Plk_gaussian_table(self, bird, params_values_dict, requires=None):
        co = bird.co
        rows = self.gaussian_rows(bird.f, params_values_dict, kmA=co.kmA, krA=co.krA, ndA=co.ndA, kmB=co.kmB, krB=co.krB, ndB=co.ndB)
        PG = _table_from_rows(bird, rows[1:], gaussian_params(self.prefix, self.cross_prefix), requires)
        if getattr(co, "with_NNLO", False) and not self.is_cross():  # reference parambasis.py:303-307
            b1, No, st = params_values_dict[self.prefix + "b1"], co.No, PG.pop(self.prefix + "ce0", None)
            extra = {self.prefix + "cr4": 1 / 4 * b1**2 / co.krA**4 * bird.PctNNLOl[:No, 0], self.prefix + "cr6": 1 / 4 * b1 / co.krA**4 * bird.PctNNLOl[:No, 1]}
            PG.update({p: v for p, v in extra.items() if requires is None or p in requires})
            if st is not None:  # keep the reference's insertion order: ..., cr4, cr6, ce0, cemono, cequad
                rest = {p: PG.pop(p) for p in (self.prefix + "cemono", self.prefix + "cequad") if p in PG}
                PG[self.prefix + "ce0"] = st
                PG.update(rest)
        return PG


@dataclass(frozen=True)
class EastCoastBasis:
    """Same surface as reference parambasis.py:320-454 (b1 b2 bG2 bGamma3 c0 c2 c4 | Pshot a0 a2; auto spectra only)."""

    prefix: str = ""
    cross_prefix: list = field(default_factory=list)

    def __post_init__(self):
        if self.cross_prefix:
            raise NotImplementedError("EastCoastBasis does not support cross yet")

    def default(self):
        return {p: 0.0 for p in self.gaussian_params()}

    def bsA(self):
        return [self.prefix + p for p in ("b1", "b2", "bG2", "bGamma3", "c0", "c2", "c4")]

    def es(self):
        return [self.prefix + p for p in ("Pshot", "a0", "a2")]

    def cnnloA(self):
        return [self.prefix + "ctilde"]

    def is_cross(self):
        return False

    @classmethod
    def get_name(cls):
        return "eastcoast"

    @classmethod
    def counterform(cls):
        return "eastcoast"

    def non_gaussian_params(self):
        return [self.prefix + p for p in ("b1", "b2", "bG2")]

    def gaussian_params(self):
        return [self.prefix + p for p in ("bGamma3", "c0", "c2", "c4", "Pshot", "a0", "a2")] + self.cnnloA()

    def _values(self, params_values_dict):
        v = self.default()
        v.update(params_values_dict)
        return [v[p] for p in self.bsA() + self.es()]

    def reduce_Plk(self, bird, params_values_dict):
        bsA, es = eastcoast_to_bs(bird.f, *self._values(params_values_dict))
        v = self.default()
        v.update(params_values_dict)
        cnnloA = [v[self.prefix + "ctilde"], 0.0] if getattr(bird.co, "with_NNLO", False) else (0.0, 0.0)
        return reduce_Plk(bird, bsA, None, es, cnnloA)  # bird.co.counterform must be 'eastcoast', as in the reference

    def nnlo_row(self, f, params_values_dict, krA=0.25):
        """EFTB_B_BIASN coefficients (ctilde) for one walker"""
        v = self.default()
        v.update(params_values_dict)
        return nnlo_vector(f, v[self.prefix + "b1"], [v[self.prefix + "ctilde"], 0.0], krA, "eastcoast")

    def bias_row(self, f, params_values_dict, **scales):
        return eastcoast_bias_row(f, *self._values(params_values_dict), **scales)

    def gaussian_rows(self, f, params_values_dict, **scales):
        return gaussian_rows(f, [params_values_dict[self.prefix + p] for p in ("b1", "b2", "bG2")], basis="eastcoast", **scales)

    def reduce_Plk_gaussian_table(self, bird, params_values_dict, requires=None):
        co = bird.co
        rows = self.gaussian_rows(bird.f, params_values_dict, kmA=co.kmA, krA=co.krA, ndA=co.ndA)
        PG = _table_from_rows(bird, rows[1:], self.gaussian_params()[:7], requires)
        p = self.prefix + "ctilde"
        if getattr(co, "with_NNLO", False) and (requires is None or p in requires):  # reference parambasis.py:429-435
            b1, f, Pn = params_values_dict[self.prefix + "b1"], bird.f, bird.PctNNLOl[: co.No]
            ct = -(b1**2) * f**4 * Pn[:, 0] - 2.0 * b1 * f**5 * Pn[:, 1] - f**6 * Pn[:, 2]
            keys = list(PG)
            st = {q: PG.pop(q) for q in keys if q in (self.prefix + "Pshot", self.prefix + "a0", self.prefix + "a2")}
            PG[p] = ct  # reference order: bGamma3, c0, c2, c4, ctilde, Pshot, a0, a2
            PG.update(st)
        return PG


def find_param_basis(name):
    """reference parambasis.py:457-466"""
    if name == "westcoast":
        return WestCoastBasis
    if name == "eastcoast":
        return EastCoastBasis
    import importlib

    module_name, class_name = name.rsplit(".", 1)
    return getattr(importlib.import_module(module_name), class_name)


# ----------------------------------------------------------------------------- draw recipes (rows built on the device from parameter values)
# A recipe is the compiled form of "how the coefficient rows follow from the parameters": every entry is a sum of monomials
#     coef * f^e * theta[i] * theta[j] * theta[k]        (index -1: the factor 1)
# of the per-draw parameter vector theta and the growth rate f of the (walker, tracer) entry.  The monomials are not typed a second time:
# the scalar builders above (bias_vectors, gaussian_rows, _eastcoast_rows, nnlo_vector) only use + - * / and integer powers, so calling them
# with _Poly values in place of floats yields the polynomials they compute (eftb_set_draw_recipe, Engine.reduce_draws_params,
# MarginalLikelihood.logp_draws_params).
RECIPE_MAXP, RECIPE_MAXTERMS, RECIPE_MAXDEG, RECIPE_MAXFPOW = 32, 1024, 3, 6


class _Poly:
    """polynomial in f and theta with float coefficients: {(e, (i, j, ...) ascending): coef}"""

    __slots__ = ("m",)

    def __init__(self, m=None):
        self.m = {k: v for k, v in (m or {}).items() if v != 0.0}

    @staticmethod
    def _of(x):
        if isinstance(x, _Poly):
            return x
        if isinstance(x, (int, float, np.integer, np.floating)):
            return _Poly({(0, ()): float(x)})
        return None

    def __add__(self, o):
        o = _Poly._of(o)
        if o is None:
            return NotImplemented
        m = dict(self.m)
        for k, v in o.m.items():
            m[k] = m.get(k, 0.0) + v
        return _Poly(m)

    __radd__ = __add__

    def __neg__(self):
        return _Poly({k: -v for k, v in self.m.items()})

    def __sub__(self, o):
        o = _Poly._of(o)
        return NotImplemented if o is None else self + (-o)

    def __rsub__(self, o):
        o = _Poly._of(o)
        return NotImplemented if o is None else o + (-self)

    def __mul__(self, o):
        o = _Poly._of(o)
        if o is None:
            return NotImplemented
        m = {}
        for (e1, i1), v1 in self.m.items():
            for (e2, i2), v2 in o.m.items():
                k = (e1 + e2, tuple(sorted(i1 + i2)))
                m[k] = m.get(k, 0.0) + v1 * v2
        return _Poly(m)

    __rmul__ = __mul__

    def __truediv__(self, o):
        if isinstance(o, _Poly):
            if set(o.m) - {(0, ())} or not o.m:
                raise ValueError("a draw recipe cannot divide by a parameter")
            o = o.m[(0, ())]
        if not isinstance(o, (int, float, np.integer, np.floating)):
            return NotImplemented
        return _Poly({k: v / float(o) for k, v in self.m.items()})

    def __rtruediv__(self, o):
        return _Poly._of(o) / self

    def __pow__(self, p):
        if not isinstance(p, (int, np.integer)) or p < 0:
            raise ValueError("a draw recipe only takes non-negative integer powers of a parameter")
        out = _Poly({(0, ()): 1.0})
        for _ in range(int(p)):
            out = out * self
        return out


_POLY_F = _Poly({(1, ()): 1.0})


def _poly_theta(i):
    return _Poly({(0, (i,)): 1.0})


class DrawRecipe:
    """Terms (tracer, row g, column r, coef, e, i, j, k) of the coefficient rows [ntr, ng1, 24 (+ 3 NNLO columns 24..26)]: entry
    (tracer, g, r) is the sum of coef * f[tracer]^e * theta[i] * theta[j] * theta[k] over its terms (an index of -1: the factor 1).
    The terms are kept sorted by (g, tracer, r, e, i, j, k) -- the order the device sums them in.  ``rows`` / ``rows_nnlo`` evaluate the
    recipe with NumPy: the host statement of what the device computes from theta."""

    def __init__(self, param_names, ntr, ng1, tracer, row, col, coef, fpow, idx):
        self.param_names = [str(n) for n in param_names]
        self.ntr, self.ng1 = int(ntr), int(ng1)
        tracer, row, col, fpow = (np.asarray(a, dtype=np.int32).reshape(-1) for a in (tracer, row, col, fpow))
        coef = np.asarray(coef, dtype=np.float64).reshape(-1)
        idx = np.sort(np.asarray(idx, dtype=np.int32).reshape(-1, RECIPE_MAXDEG), axis=1)[:, ::-1]  # (the -1 entries last)
        P, n = len(self.param_names), coef.size
        if P > RECIPE_MAXP:
            raise ValueError(f"a draw recipe takes at most {RECIPE_MAXP} parameters, got {P}")
        if n > RECIPE_MAXTERMS:
            raise ValueError(f"a draw recipe holds at most {RECIPE_MAXTERMS} terms, got {n}")
        if not (tracer.size == row.size == col.size == fpow.size == idx.shape[0] == n):
            raise ValueError("the term arrays of a draw recipe disagree on the number of terms")
        if n and (tracer.min() < 0 or tracer.max() >= self.ntr or row.min() < 0 or row.max() >= self.ng1 or col.min() < 0 or col.max() >= 27):
            raise ValueError("a term of the draw recipe addresses an entry outside [ntr, ng1, 27]")
        if n and (fpow.min() < 0 or fpow.max() > RECIPE_MAXFPOW):
            raise ValueError(f"a draw recipe takes powers of f up to {RECIPE_MAXFPOW}")
        if n and (idx.min() < -1 or idx.max() >= P):
            raise ValueError("a term of the draw recipe names a parameter outside theta")
        if not np.all(np.isfinite(coef)):
            raise ValueError("a draw recipe needs finite coefficients")
        order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0], fpow, col, tracer, row))
        self.tracer, self.row, self.col, self.coef, self.fpow, self.idx = tracer[order], row[order], col[order], coef[order], fpow[order], idx[order]

    @property
    def nterms(self):
        return self.coef.size

    @property
    def has_nnlo(self):
        return bool(np.any(self.col >= 24))

    def _eval(self, theta, f, lo, hi, magnitude=False):
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim != 2 or theta.shape[1] != len(self.param_names):
            raise ValueError(f"theta must be [N, {len(self.param_names)}]")
        N = theta.shape[0]
        f = np.asarray(f, dtype=np.float64)
        f = np.broadcast_to(f[:, None] if f.ndim == 1 and self.ntr == 1 else f, (N, self.ntr))
        fp = [np.ones((N, self.ntr))]
        for _ in range(RECIPE_MAXFPOW):
            fp.append(fp[-1] * f)
        th = np.concatenate([theta, np.ones((N, 1))], axis=1)  # (index -1: the factor 1)
        out = np.zeros((N, self.ntr, self.ng1, hi - lo))
        for t, g, r, c, e, ix in zip(self.tracer, self.row, self.col, self.coef, self.fpow, self.idx):
            if lo <= r < hi:
                v = c * fp[e][:, t] * th[:, ix[0]] * th[:, ix[1]] * th[:, ix[2]]
                out[:, t, g, r - lo] += np.abs(v) if magnitude else v
        return out

    def rows(self, theta, f):
        """theta [N, P], f [N, ntr] (the growth rate of each draw's walker per tracer; [N] with one tracer) -> rows [N, ntr, ng1, 24]"""
        return self._eval(theta, f, 0, 24)

    def rows_magnitude(self, theta, f):
        """-> the sum of the magnitudes of each entry's monomials [N, ntr, ng1, 24]: the scale of the rounding error of ``rows``.  An
        entry far below it is a cancelling sum (the east-coast mapping enters squared: (b1 + 7/2 bG2)^2 is three monomials), whose
        relative error, on the device as in the scalar builders, grows by that ratio."""
        return self._eval(theta, f, 0, 24, magnitude=True)

    def rows_nnlo(self, theta, f):
        """-> the NNLO columns [N, ntr, ng1, 3]"""
        return self._eval(theta, f, 24, 27)

    def _coefficients(self, rows, b):
        b = np.asarray(b, dtype=np.float64)
        N = rows.shape[0]
        if b.shape == (N, self.ng1 - 1):
            b = b[:, None]
        if b.ndim != 3 or b.shape[0] != N or b.shape[2] != self.ng1 - 1:
            raise ValueError(f"b must be [{N}, S, {self.ng1 - 1}]: S sets of the linear parameters per draw")
        out = np.repeat(rows[:, None, :, 0], b.shape[1], axis=1)  # row 0, then the rows g >= 1 in their order
        for g in range(1, self.ng1):
            out = out + b[:, :, None, g - 1, None] * rows[:, None, :, g]
        return out

    def coefficients(self, theta, f, b):
        """theta [N, P], f as ``rows``, b [N, S, ng1 - 1] ([N, ng1 - 1]: S = 1) values of the linear parameters -> the coefficient rows
        rows[0] + sum_g b[g - 1] rows[g] [N, S, ntr, 24] that ``Engine.reduce_draws`` contracts with the templates: the host counterpart of
        the coefficients ``MarginalLikelihood.sample_gaussian_params`` builds on the device"""
        return self._coefficients(self.rows(theta, f), b)

    def coefficients_nnlo(self, theta, f, b):
        """-> the NNLO columns of ``coefficients`` [N, S, ntr, 3]"""
        return self._coefficients(self.rows_nnlo(theta, f), b)

    def derivative(self):
        """The terms of d rows / d theta: for each term and each distinct theta index p in it one record (p, tracer, row, col, coef *
        multiplicity of p in the term, fpow, idx [2]: the two remaining indices, -1 last), sorted by (p, row, tracer, col) and, inside an
        entry, by the order the library gives the parent terms (fpow, i, j, k, coef) -- the table eftb_set_draw_recipe builds for
        eftb_draws_logp_grad_params, whatever order the terms were handed over in."""
        order = np.lexsort((self.coef, self.idx[:, 2], self.idx[:, 1], self.idx[:, 0], self.fpow, self.col, self.tracer, self.row))
        rec = []
        for p in range(len(self.param_names)):
            for t in order:
                ix = [int(v) for v in self.idx[t]]
                m = ix.count(p)
                if m:
                    ix.remove(p)
                    rec.append((p, self.tracer[t], self.row[t], self.col[t], self.coef[t] * m, self.fpow[t], ix))
        out = np.zeros(len(rec), dtype=[("p", "<i4"), ("tracer", "<i4"), ("row", "<i4"), ("col", "<i4"), ("coef", "<f8"), ("fpow", "<i4"), ("idx", "<i4", (2,))])
        for q, r in enumerate(rec):
            out[q] = r
        return out

    def _jac(self, theta, f, lo, hi, magnitude=False):
        theta = np.asarray(theta, dtype=np.float64)
        P = len(self.param_names)
        if theta.ndim != 2 or theta.shape[1] != P:
            raise ValueError(f"theta must be [N, {P}]")
        N = theta.shape[0]
        f = np.asarray(f, dtype=np.float64)
        f = np.broadcast_to(f[:, None] if f.ndim == 1 and self.ntr == 1 else f, (N, self.ntr))
        fp = [np.ones((N, self.ntr))]
        for _ in range(RECIPE_MAXFPOW):
            fp.append(fp[-1] * f)
        th = np.concatenate([theta, np.ones((N, 1))], axis=1)  # (index -1: the factor 1)
        out = np.zeros((N, self.ntr, self.ng1, hi - lo, P))
        for d in self.derivative():
            if lo <= d["col"] < hi:
                v = d["coef"] * fp[d["fpow"]][:, d["tracer"]] * th[:, d["idx"][0]] * th[:, d["idx"][1]]
                out[:, d["tracer"], d["row"], d["col"] - lo, d["p"]] += np.abs(v) if magnitude else v
        return out

    def jacobian(self, theta, f):
        """d rows / d theta [N, ntr, ng1, 24, P] (theta, f as ``rows``): the terms of ``derivative`` summed in their order"""
        return self._jac(theta, f, 0, 24)

    def jacobian_nnlo(self, theta, f):
        """-> d rows_nnlo / d theta [N, ntr, ng1, 3, P]"""
        return self._jac(theta, f, 24, 27)

    def jacobian_magnitude(self, theta, f):
        """-> the sum of the magnitudes of the monomials of each entry of ``jacobian``: the scale of its rounding error, as
        ``rows_magnitude`` is of ``rows``"""
        return self._jac(theta, f, 0, 24, magnitude=True)

    def second_derivative(self):
        """The terms of d2 rows / d theta_p d theta_q: for each term and each unordered pair p <= q of theta indices in it one record (p, q,
        tracer, row, col, coef * multiplicity, fpow, idx [1]: the one remaining index or -1), the multiplicity being m_p m_q for p < q and
        m_p (m_p - 1) for p = q (m: how often the index occurs in the term).  Sorted by (p, q, row, tracer, col) and, inside an entry, by
        the order the library gives the parent terms, as ``derivative`` -- the table eftb_set_draw_recipe builds for
        eftb_draws_logp_hess_params."""
        order = np.lexsort((self.coef, self.idx[:, 2], self.idx[:, 1], self.idx[:, 0], self.fpow, self.col, self.tracer, self.row))
        P = len(self.param_names)
        rec = []
        for p in range(P):
            for q in range(p, P):
                for t in order:
                    ix = [int(v) for v in self.idx[t]]
                    m = ix.count(p) * (ix.count(p) - 1) if p == q else ix.count(p) * ix.count(q)
                    if m:
                        ix.remove(p)
                        ix.remove(q)
                        rec.append((p, q, self.tracer[t], self.row[t], self.col[t], self.coef[t] * m, self.fpow[t], ix))
        out = np.zeros(len(rec), dtype=[("p", "<i4"), ("q", "<i4"), ("tracer", "<i4"), ("row", "<i4"), ("col", "<i4"), ("coef", "<f8"), ("fpow", "<i4"),
                                        ("idx", "<i4", (1,))])
        for n, r in enumerate(rec):
            out[n] = r
        return out

    def _hess(self, theta, f, lo, hi, magnitude=False):
        theta = np.asarray(theta, dtype=np.float64)
        P = len(self.param_names)
        if theta.ndim != 2 or theta.shape[1] != P:
            raise ValueError(f"theta must be [N, {P}]")
        N = theta.shape[0]
        f = np.asarray(f, dtype=np.float64)
        f = np.broadcast_to(f[:, None] if f.ndim == 1 and self.ntr == 1 else f, (N, self.ntr))
        fp = [np.ones((N, self.ntr))]
        for _ in range(RECIPE_MAXFPOW):
            fp.append(fp[-1] * f)
        th = np.concatenate([theta, np.ones((N, 1))], axis=1)  # (index -1: the factor 1)
        out = np.zeros((N, self.ntr, self.ng1, hi - lo, P, P))
        for d in self.second_derivative():
            if lo <= d["col"] < hi:
                v = d["coef"] * fp[d["fpow"]][:, d["tracer"]] * th[:, d["idx"][0]]
                out[:, d["tracer"], d["row"], d["col"] - lo, d["p"], d["q"]] += np.abs(v) if magnitude else v
        iu = np.triu_indices(P, 1)
        out[..., iu[1], iu[0]] = out[..., iu[0], iu[1]]  # entry (q, p) is a copy of (p, q)
        return out

    def hessian(self, theta, f):
        """d2 rows / d theta d theta [N, ntr, ng1, 24, P, P] (theta, f as ``rows``): the terms of ``second_derivative`` summed in their order"""
        return self._hess(theta, f, 0, 24)

    def hessian_nnlo(self, theta, f):
        """-> d2 rows_nnlo / d theta d theta [N, ntr, ng1, 3, P, P]"""
        return self._hess(theta, f, 24, 27)

    def hessian_magnitude(self, theta, f):
        """-> the sum of the magnitudes of the monomials of each entry of ``hessian``: the scale of its rounding error, as
        ``jacobian_magnitude`` is of ``jacobian``"""
        return self._hess(theta, f, 0, 24, magnitude=True)

    def terms(self):
        """the records of eftb_set_draw_recipe"""
        from . import _lib as L

        out = np.zeros(self.nterms, dtype=L.DRAW_TERM)
        out["tracer"], out["row"], out["col"], out["fpow"], out["coef"] = self.tracer, self.row, self.col, self.fpow, self.coef
        out["i"], out["j"], out["k"] = self.idx.T
        return out


def _compile_recipe(param_names, poly_rows, ng1):
    """poly_rows[tracer][g]: 24 (or 27) entries, floats or _Poly -> DrawRecipe"""
    tr, row, col, coef, fpow, idx = [], [], [], [], [], []
    for t, rows_t in enumerate(poly_rows):
        for g, rw in enumerate(rows_t):
            for r, v in enumerate(rw):
                p = _Poly._of(v)
                if p is None:
                    raise ValueError(f"entry ({t}, {g}, {r}) of the rows is neither a number nor a polynomial: {type(v).__name__}")
                for (e, ix), c in sorted(p.m.items()):
                    if len(ix) > RECIPE_MAXDEG:
                        raise ValueError(f"entry ({t}, {g}, {r}) is of degree {len(ix)} in the parameters, a draw recipe takes up to {RECIPE_MAXDEG}")
                    if e > RECIPE_MAXFPOW:
                        raise ValueError(f"entry ({t}, {g}, {r}) holds f^{e}, a draw recipe takes powers of f up to {RECIPE_MAXFPOW}")
                    tr.append(t); row.append(g); col.append(r); coef.append(c); fpow.append(e)
                    idx.append(list(ix) + [-1] * (RECIPE_MAXDEG - len(ix)))
    return DrawRecipe(param_names, len(poly_rows), ng1, tr, row, col, coef, fpow, idx)


def _recipe_names(param_names, needed):
    """theta's order: the caller's, or every needed name once in order of first appearance"""
    if param_names is None:
        param_names = list(dict.fromkeys(needed))
    param_names = [str(n) for n in param_names]
    if len(set(param_names)) != len(param_names):
        raise ValueError("param_names repeats a name")
    missing = [n for n in needed if n not in param_names]
    if missing:
        raise ValueError(f"param_names lacks {sorted(set(missing))}")
    if len(param_names) > RECIPE_MAXP:
        raise ValueError(f"a draw recipe takes at most {RECIPE_MAXP} parameters, got {len(param_names)}")
    return param_names


def bias_draw_recipe(bases, scales, with_NNLO=False, param_names=None):
    """The recipe of ``basis.bias_row`` (``bias_rows_many``) per tracer, and of ``basis.nnlo_row`` (``nnlo_vector``) in the NNLO columns
    with ``with_NNLO``: theta holds the full parameter set bsA() + bsB() + es() (+ cnnloA()) of every basis, each name once; one row.
    bases / scales: one basis and one dict(kmA=, krA=, ndA=[, kmB=, ...]) per tracer (a single basis / dict: one tracer)."""
    if not isinstance(bases, (list, tuple)):
        bases, scales = [bases], [scales]
    if len(scales) != len(bases):
        raise ValueError("one scale dict per tracer")
    own = [b.bsA() + (b.bsB() if b.is_cross() else []) + b.es() + (b.cnnloA() if with_NNLO else []) for b in bases]
    names = _recipe_names(param_names, [n for o in own for n in o])
    rows = []
    for basis, sc, o in zip(bases, scales, own):
        v = {n: _poly_theta(names.index(n)) for n in o}
        r = list(basis.bias_row(_POLY_F, v, **sc))
        if with_NNLO:
            if basis.is_cross():
                raise NotImplementedError("the NNLO counter-terms of a cross spectrum are not supported (as the reference)")
            r += list(basis.nnlo_row(_POLY_F, v, sc.get("krA", 0.25)))
        rows.append([r])
    return _compile_recipe(names, rows, 1)
