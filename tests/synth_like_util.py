"""A seeded synthetic likelihood of any shape for the draw calls, NumPy only, beside grad_util.py, hess_util.py, sample_util.py and
chain_util.py; shared by the CPU tests (test_draw_synthetic.py) and the GPU tests (test_gpu_draw_synthetic.py).

The fixture likelihoods (marg.npz, cfg3.npz) put every draw kernel at one workgroup shape: four waves, J + 1 in {25, 28, 73, 82} columns,
nG in {0, 2, 7, 11, 12, 14}, ndata in {36, 142}.  problem() builds a likelihood with any number of tracers, NNLO or not, any nG up to 24, any
template block and data-vector length, with a hand-built DrawRecipe whose Gaussian rows depend on theta (F2 moves with theta, the Hessian has
second-derivative terms).  It plugs into the yardsticks the suite already has (grad_util, hess_util, sample_util, chain_util and
oracle.marginal); nothing is restated here.

CASES      the shapes, the smallest that reach each path of the launcher (draws_logp_shape: the wave count that fits the LDS, the TWO
           instantiation beyond 64 columns) and of draws_solve (nG = 1, nG below and off the multiples of ADJ_KB = 4, nG = 23 and 24);
           `runs` states per call whether the library serves the shape or refuses it
SYNTH_FLOOR  the worst error of the NumPy Gram-route restatements against the data-space yardsticks per case and prior, measured on the
           host (test_draw_synthetic.py asserts them); the device is held to hess_util.device_bar of each
reference() the yardsticks of every draw of a case, computed once and shared"""
import functools
import types

import numpy as np

import chain_util as CU
import grad_util as GU
import hess_util as HU
import sample_util as SU

# draws per walker: one walker owns none, one more than twice the four waves of the largest workgroup.  (That alone gives no wave a second
# draw: the launcher spreads a walker's draws over up to 2048 / C workgroups.  long_counts() is what makes the waves loop.)
COUNTS = [9, 0, 5]
S5 = 5  # samples per draw: no multiple of the kernel's chunk of ADJ_KB = 4
CALLS = ("rows", "stage", "params", "grad", "hess", "hess_jeffreys", "sample", "chain")

# the wave counts (rows kernel / params kernels) are those of draws_logp_shape at the commit that added this table: for the reader, not asserted
CASES = {
    "A": dict(ntr=1, nnlo=False, nG=1, nl=3, nx=4, ndata=9, P=1),  # J1 25, nw 4: the smallest of everything
    "B": dict(ntr=1, nnlo=False, nG=3, nl=1, nx=11, ndata=11, P=2),  # J1 25, nw 4: nl = 1, nG < ADJ_KB
    "C": dict(ntr=2, nnlo=False, nG=5, nl=3, nx=3, ndata=5, P=3),  # J1 49, nw 4: two tracers, ndata < 16
    "D": dict(ntr=2, nnlo=True, nG=4, nl=3, nx=5, ndata=17, P=3),  # J1 55, nw 4: the NNLO columns of two tracers, ndata = 1 mod 4
    "E": dict(ntr=1, nnlo=True, nG=24, nl=3, nx=6, ndata=16, P=4),  # J1 28, nw 4: nG max at even J1
    "F": dict(ntr=3, nnlo=False, nG=23, nl=3, nx=5, ndata=33, P=5),  # J1 73, nw 4: TWO, nG odd
    "G": dict(ntr=4, nnlo=False, nG=24, nl=3, nx=5, ndata=17, P=5),  # J1 97, nw 2
    "H": dict(ntr=4, nnlo=True, nG=16, nl=3, nx=5, ndata=53, P=6),  # J1 109: the rows kernel at nw 4 beside the params kernels at nw 2
    "I": dict(ntr=5, nnlo=False, nG=24, nl=3, nx=7, ndata=53, P=8),  # J1 121, nw 1: the largest footprint there is
    # J1 121: the rows kernel at nw 4 on 154568 of 163840 bytes, the params, gradient and sample kernels at nw 4 on 161432, 162024 and
    # 163048; the chain and Hessian kernels, with more words per wave, at nw 2
    "J": dict(ntr=5, nnlo=False, nG=8, nl=3, nx=7, ndata=53, P=8),
    # case G with a data vector longer than nG, so that a flat prior is proper: the shape of the failing-draw test at nw 2 (G itself has
    # ndata = 17 < nG = 24: under a flat prior every one of its draws is singular)
    "Gf": dict(ntr=4, nnlo=False, nG=24, nl=3, nx=5, ndata=31, P=5),
    # case E likewise (its 3 x 6 block holds 18 points: nx = 10 here): nG = 24 at nw 4 and even J1 under a proper flat prior
    "Ef": dict(ntr=1, nnlo=True, nG=24, nl=3, nx=10, ndata=27, P=4),
}
# what the library does with each call at each case: True runs, False refuses.  The Hessian call of case I keeps 2 P nG^2 doubles per wave
# beside a W_c of 117 KB without Jeffreys and fits with it.
for _c in CASES.values():
    _c["runs"] = dict.fromkeys(CALLS, True)
CASES["I"]["runs"]["hess"] = False
# five tracers with NNLO: J + 1 = 136 columns; every draw call refuses ("at most 127"); the LOGP stage is no draw call and is not asked
TOO_WIDE = dict(ntr=5, nnlo=True, nG=4, nl=3, nx=4, ndata=20, P=3, runs=dict(dict.fromkeys(CALLS, False), stage=True))
SEEDS = {c: 1000 + i for i, c in enumerate(CASES)}


def kinds(case):
    """the priors a case is checked under: Gaussian always, flat where ndata >= nG"""
    c = CASES[case]
    return ("gauss", "flat") if c["ndata"] >= c["nG"] else ("gauss",)


def jeffreys_of(case, kind):
    """Jeffreys off and on, but off alone under a flat prior with ndata = nG (case C): there the best fit interpolates the data, the
    minimum chi2 and with it Jeffreys' ln P are identically zero, and the magnitudes that scale a gradient error are rounding noise"""
    c = CASES[case]
    return (False,) if kind == "flat" and c["ndata"] == c["nG"] else (False, True)


# worst error of the NumPy Gram route (chain_util.gram_record, sample_util.gram_samples, grad_util.gram_adjoint, hess_util.gram_hessian)
# against the data-space yardsticks over the 14 draws of each case, Jeffreys on and off alike, as
# test_draw_synthetic.py::test_gram_route_floors prints them on the host (it holds the measurement to 1.5 times these entries: another
# NumPy / BLAS rounds differently).  logp is scaled by 1/2 (|F0| + |F1 . b| + |ln det|), fullchi2 by
# |F0| + |F1 . b|, best and samples are in whitened units, grad and hess are scaled by mag, covariance and identity as in sample_util.py.
# (case C under its flat prior has ndata = nG: F2 = V C^-1 V^T of a square V carries the square of V's condition number)
_F = lambda *v: dict(zip(("logp", "fullchi2", "best", "grad", "hess", "samples", "covariance", "identity"), v))
SYNTH_FLOOR = {
    "A": dict(gauss=_F(1.2e-13, 1.3e-13, 6.1e-14, 2.3e-15, 4.4e-16, 6.1e-14, 4.4e-15, 8.2e-12),
              flat=_F(1.2e-13, 1.2e-13, 6.1e-14, 2.2e-15, 3.7e-16, 6.5e-14, 8.6e-15, 6.3e-12)),
    "B": dict(gauss=_F(7.6e-16, 7.2e-16, 6.7e-14, 4.3e-15, 1.0e-15, 6.7e-14, 7.6e-15, 4.2e-12),
              flat=_F(7.1e-16, 7.1e-16, 1.4e-13, 2.7e-14, 3.5e-15, 1.4e-13, 5.3e-15, 3.0e-12)),
    "C": dict(gauss=_F(1.1e-15, 6.0e-16, 2.1e-13, 4.9e-14, 6.4e-15, 2.1e-13, 1.6e-14, 6.3e-12),
              flat=_F(6.8e-14, 3.7e-14, 1.8e-10, 8.9e-10, 4.1e-15, 3.0e-10, 2.1e-10, 1.6e-09)),
    "D": dict(gauss=_F(2.8e-15, 2.7e-15, 4.5e-14, 1.5e-14, 5.8e-16, 4.6e-14, 5.8e-15, 3.7e-12),
              flat=_F(2.4e-15, 2.5e-15, 7.9e-14, 1.6e-14, 7.8e-16, 9.2e-14, 1.1e-14, 6.5e-12)),
    "E": dict(gauss=_F(9.3e-16, 1.6e-15, 2.8e-12, 1.5e-13, 1.8e-13, 3.0e-12, 1.5e-12, 1.8e-11)),
    "F": dict(gauss=_F(5.8e-16, 6.6e-16, 4.0e-13, 1.3e-14, 5.9e-15, 4.0e-13, 3.7e-14, 9.2e-12),
              flat=_F(1.4e-15, 9.4e-16, 3.7e-12, 1.5e-13, 1.1e-13, 3.8e-12, 5.1e-13, 8.4e-12)),
    "G": dict(gauss=_F(8.3e-15, 8.8e-15, 1.5e-12, 8.8e-14, 1.6e-14, 1.6e-12, 6.2e-14, 5.2e-12)),
    "H": dict(gauss=_F(7.3e-16, 7.2e-16, 2.9e-13, 1.2e-14, 2.0e-15, 2.9e-13, 1.1e-14, 1.9e-12),
              flat=_F(6.5e-16, 8.9e-16, 2.5e-13, 2.7e-14, 2.0e-15, 2.5e-13, 9.3e-15, 1.4e-12)),
    "I": dict(gauss=_F(3.3e-15, 3.2e-15, 1.5e-12, 3.6e-14, 3.1e-14, 1.6e-12, 1.5e-13, 1.1e-11),
              flat=_F(5.7e-15, 4.4e-15, 1.5e-11, 1.2e-13, 1.3e-13, 1.5e-11, 7.9e-13, 1.2e-11)),
    "J": dict(gauss=_F(2.7e-15, 2.6e-15, 2.6e-13, 3.7e-15, 1.3e-15, 2.6e-13, 1.7e-14, 5.9e-12),
              flat=_F(2.7e-15, 2.7e-15, 1.8e-13, 5.2e-15, 1.8e-15, 1.8e-13, 1.7e-14, 1.2e-11)),
    "Gf": dict(gauss=_F(1.1e-15, 1.1e-15, 1.4e-12, 1.4e-14, 3.2e-14, 1.4e-12, 8.4e-14, 1.8e-12),
               flat=_F(1.9e-15, 2.0e-15, 2.6e-12, 2.5e-13, 3.1e-13, 2.6e-12, 4.1e-13, 5.3e-12)),
    "Ef": dict(gauss=_F(1.1e-15, 1.6e-15, 3.1e-12, 5.8e-14, 6.4e-14, 3.1e-12, 3.1e-13, 7.1e-12),
               flat=_F(8.1e-15, 5.9e-15, 4.7e-11, 4.7e-13, 2.0e-12, 5.0e-11, 1.7e-11, 2.7e-11)),
}


def floor_of(case, kind, quantity):
    return SYNTH_FLOOR[case][kind][quantity]


# The LOGP stage's product U = V C^-1 (launch_times_invcov, the one caller of gemm_narrow_kernel with blockIdx.y > 0) past one column group
# of 128 data points: exactly one group, one column in a second group, three groups with one column in the last.  Two tracers on 3 x 50
# blocks; the LOGP stage alone is asked (the draw calls may refuse such footprints).  WIDE_FLOOR: the Gram route against the data-space
# yardstick, Jeffreys on and off, as test_draw_synthetic.py::test_wide_logp_floors prints it; the device's stage call is held to
# hess_util.device_bar of each.
WIDE = {n: dict(ntr=2, nnlo=False, nG=3, nl=3, nx=50, ndata=n, P=2) for n in (128, 129, 257)}
WIDE_SEEDS = {128: 2128, 129: 2129, 257: 2257}
WIDE_FLOOR = {
    128: dict(logp=4.4e-15, fullchi2=4.6e-15, best=1.4e-13),
    129: dict(logp=3.1e-15, fullchi2=3.1e-15, best=1.1e-13),
    257: dict(logp=1.0e-14, fullchi2=1.0e-14, best=1.9e-13),
}


@functools.lru_cache(maxsize=None)
def wide_problem(ndata):
    return problem(seed=WIDE_SEEDS[ndata], **WIDE[ndata])


@functools.lru_cache(maxsize=None)
def wide_reference(ndata, jeffreys=False):
    """yardstick() of every draw of a WIDE likelihood (ln P, full chi2 and best are what the stage call is compared with)"""
    pb = wide_problem(ndata)
    z = normals(pb.theta.shape[0], 1, pb.nG)
    return [yardstick(pb, d, z[d], jeffreys, hess=False) for d in range(pb.theta.shape[0])]


def problem(ntr, nnlo, nG, nl, nx, ndata, P, seed, flat=False, counts=COUNTS, singular=None):
    """-> a namespace of templ [C ntr, nl, 24, nx], templn (or None), index [ndata], D, invcov, loc, scale, rec (a DrawRecipe), theta [N, P],
    f [C, ntr], counts, walker [N].  singular = g: every term of Gaussian row g carries a factor theta_0, so that a draw with theta_0 = 0
    has an exactly zero row g of the model and, under a flat prior, an exactly zero row and column of F2."""
    from eftpipe_amd.parambasis import DrawRecipe

    rng = np.random.default_rng(seed)
    C, N = len(counts), int(sum(counts))
    wscale = np.repeat(1.0 + 0.2 * np.arange(C), ntr)[:, None, None, None]
    templ = rng.standard_normal((C * ntr, nl, 24, nx)) * np.logspace(-1, 1, 24)[rng.permutation(24)][:, None] * wscale
    templn = rng.standard_normal((C * ntr, nl, 24, nx)) * np.logspace(-1, 1, 24)[rng.permutation(24)][:, None] * wscale if nnlo else None
    block = nl * nx
    first = [t * block + int(rng.integers(block)) for t in range(ntr)] if ndata >= ntr else []
    rest = rng.permutation(np.setdiff1d(np.arange(ntr * block), first))[: ndata - len(first)]
    index = np.sort(np.concatenate([first, rest])).astype(np.int32)
    assert index.size == ndata and np.unique(index).size == ndata
    Q, _ = np.linalg.qr(rng.standard_normal((ndata, ndata)))
    invcov = (Q * np.logspace(-1.5, 1.5, ndata)[rng.permutation(ndata)]) @ Q.T
    invcov = 0.5 * (invcov + invcov.T)
    # ---- the recipe
    ncol = 27 if nnlo else 24
    terms = []  # (tracer, row, col, coef, fpow, idx)
    u = lambda: float(rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0]))
    for t in range(ntr):
        for c in range(ncol):
            terms.append((t, 0, c, u(), (t * ncol + c) % 7, [(t + c) % P, -1, -1]))
    for g in range(1, nG + 1):
        s = [0] if singular == g else [-1]
        lin = 24 + g % 3 if nnlo and g % 2 == 0 else (5 * g + 7) % 24
        quad = 24 + (g + 1) % 3 if nnlo and g % 3 == 0 else (5 * g + 13) % 24
        terms.append(((g - 1) % ntr, g, (5 * g + 1) % 24, u(), 0, s + [-1, -1]))
        terms.append((g % ntr, g, lin, 0.3 * u(), g % 7, [g % P] + s + [-1]))
        terms.append(((g + 1) % ntr, g, quad, 0.2 * u(), (g + 3) % 7, [(g + 1) % P, (2 * g) % P] + s))
        if g % 3 == 1:
            terms.append(((g + 2) % ntr, g, (5 * g + 19) % 24, 0.1 * u(), (g + 5) % 7, [(g + 2) % P, (g + 2) % P] + s))
    rec = DrawRecipe(["p%d" % i for i in range(P)], ntr, nG + 1, *[[t[k] for t in terms] for k in range(6)])
    assert set(rec.fpow) == set(range(7)) and rec.has_nnlo == bool(nnlo)
    # ---- the draws, the data and the prior
    theta = 1.0 + 0.3 * rng.standard_normal((N, P))
    assert np.unique(theta, axis=0).shape[0] == N
    f = rng.uniform(0.6, 0.9, (C, ntr))
    V, _ = GU.recipe_vectors(rec, np.ones(P), f[0], templ[:ntr], index, None if templn is None else templn[:ntr])
    D = V[0] + 0.5 * rng.standard_normal(nG) @ V[1:] + np.linalg.cholesky(np.linalg.inv(invcov)) @ rng.standard_normal(ndata)
    loc = 0.5 * rng.standard_normal(nG)
    scale = np.full(nG, np.inf) if flat else np.logspace(-1, 1, nG)[rng.permutation(nG)] if nG > 1 else np.ones(1)
    return types.SimpleNamespace(ntr=ntr, nnlo=bool(nnlo), nG=nG, nl=nl, nx=nx, ndata=ndata, P=P, templ=templ, templn=templn, index=index, D=D,
                                 invcov=invcov, loc=loc, scale=scale, rec=rec, theta=theta, f=f, counts=list(counts),
                                 walker=np.repeat(np.arange(C), counts))


def shape_of(case):
    c = CASES[case] if isinstance(case, str) else case
    return {k: c[k] for k in ("ntr", "nnlo", "nG", "nl", "nx", "ndata", "P")}


@functools.lru_cache(maxsize=None)
def case_problem(case, kind="gauss", singular=None):
    """the problem of a case of the table under its Gaussian or its flat prior (the same seed: everything but the prior is shared)"""
    return problem(seed=SEEDS[case], flat=kind == "flat", singular=singular, **shape_of(case))


def long_counts(C=len(COUNTS)):
    """draws per walker that make every wave of every draw kernel loop: a walker's draws go to at most 2048 / C workgroups of at most four
    waves (draw_shares in the library), so with more than twice that many draws every wave takes a second one, whatever the wave count"""
    return [2 * 4 * (2048 // C) + 7] + [0] * (C - 2) + [5]


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def of_walker(pb, w):
    """f [ntr], templ [ntr, nl, 24, nx] and templn of walker w"""
    n = pb.ntr
    return pb.f[w], pb.templ[w * n : (w + 1) * n], None if pb.templn is None else pb.templn[w * n : (w + 1) * n]


def normals(N, S, nG, seed=23):
    return np.random.default_rng(seed).standard_normal((N, S, nG))


def logp_scale(F, best, jeffreys):
    """1/2 of the magnitudes that ln P adds up: |F0| + |F1 . b| and, without Jeffreys, |ln det F2 / 2 pi|"""
    logdet = 0.0 if jeffreys else abs(np.linalg.slogdet(F["F2"] / (2 * np.pi))[1])
    return 0.5 * (abs(F["F0"]) + abs(F["F1"] @ best) + logdet)


def yardstick(pb, d, z, jeffreys=False, D=None, hess=True):
    """the data-space yardsticks of draw d -> dict(logp, fullchi2, best, scale, L, F2, grad, gmag, hess, hmag, b [S, nG])"""
    from oracle import marginal as M

    ff, tw, tn = of_walker(pb, pb.walker[d])
    D = pb.D if D is None else D
    V, dV, d2V = HU.recipe_vectors2(pb.rec, pb.theta[d], ff, tw, pb.index, tn)
    logp, full, best, F = M.marginalized_logp(V[1:], V[0], D, pb.invcov, pb.loc, pb.scale, jeffreys=jeffreys, return_best=True)
    y = SU.data_space_samples(V, D, pb.invcov, pb.loc, pb.scale, z, jeffreys)
    _, grad, gmag = GU.data_space_adjoint(V, dV, D, pb.invcov, pb.loc, pb.scale, jeffreys)
    out = dict(logp=logp, fullchi2=full, best=best, scale=logp_scale(F, best, jeffreys), chi2scale=abs(F["F0"]) + abs(F["F1"] @ best), L=y["L"],
               F2=y["F2"], grad=grad, gmag=gmag, b=y["b"], chi2=y["chi2"], V=V)
    if hess:
        _, out["hess"], out["hmag"] = HU.data_space_hessian(V, dV, d2V, D, pb.invcov, pb.loc, pb.scale, jeffreys)
    return out


@functools.lru_cache(maxsize=None)
def reference(case, kind, jeffreys=False):
    """the yardsticks of every draw of a case (a list of yardstick()'s dicts), computed once; z is normals(N, S5, nG)"""
    pb = case_problem(case, kind)
    z = normals(pb.theta.shape[0], S5, pb.nG)
    return [yardstick(pb, d, z[d], jeffreys) for d in range(pb.theta.shape[0])]


QUANTITIES = ("logp", "fullchi2", "best", "grad", "hess", "samples", "covariance", "identity")


def errors(pb, d, y, z, logp, full, best, grad, hess, b, chi2, X):
    """the error measures of one draw's results (a device call's or the Gram route's) against yardstick() y; X [nG, nG]: b - best of the
    call with z = 1; entries that are None are left out"""
    e = dict(logp=abs(logp - y["logp"]) / y["scale"], fullchi2=abs(full - y["fullchi2"]) / y["chi2scale"], best=SU.whitened_error(y["L"], best, y["best"]))
    if grad is not None:
        e["grad"] = float(np.max(np.abs(grad - y["grad"]) / y["gmag"]))
    if hess is not None:
        e["hess"] = float(np.max(np.abs(hess - y["hess"]) / y["hmag"]))
    if b is not None:
        e["samples"] = SU.whitened_error(y["L"], b, y["b"])
        e["identity"] = SU.identity_error(chi2, b, full, best, pb.loc, pb.scale, z)
    if X is not None:
        e["covariance"] = SU.covariance_error(y["F2"], X)
    return e


def gram_route(pb, d, z, jeffreys=False):
    """the results of draw d by the NumPy restatements of the kernels' Gram route, in the argument order of errors()"""
    ff, tw, tn = of_walker(pb, pb.walker[d])
    W = GU.gram_matrix(tw, pb.index, pb.D, pb.invcov, tn)
    th = pb.theta[d]
    logp = CU.gram_record(pb.rec, th, ff, W, pb.loc, pb.scale, jeffreys)
    best, b, chi2, full = SU.gram_samples(pb.rec, th, ff, W, pb.loc, pb.scale, z)
    bi = SU.gram_samples(pb.rec, th, ff, W, pb.loc, pb.scale, np.eye(pb.nG))
    _, grad = GU.gram_adjoint(pb.rec, th, ff, W, pb.loc, pb.scale, jeffreys)
    _, _, hess = HU.gram_hessian(pb.rec, th, ff, W, pb.loc, pb.scale, jeffreys)
    return logp, full, best, grad, hess, b, chi2, bi[1] - bi[0]


def worst(dicts):
    out = {}
    for e in dicts:
        for k, v in e.items():
            out[k] = max(out.get(k, 0.0), float(v))
    return out
