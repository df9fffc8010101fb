"""Yardsticks of the samples of the marginalised parameters (eftb_draws_sample_params), NumPy only, beside grad_util.py and hess_util.py;
shared by the CPU tests (test_draw_samples.py) and the GPU tests (test_gpu_draw_samples.py).

data_space_samples   the yardstick: b^ and F2 of the oracle on the masked data vector (oracle/marginal.py marginalized_logp, pinned to the
                     reference by marg.npz / cfg3.npz), NumPy's Cholesky factor F2 = L L^T, b = b^ + solve(L^T, z) and chi2(b) from the
                     residual in data space.  It never forms a Gram matrix of the templates.  The factor with a positive diagonal is
                     unique, so another route to it agrees sample by sample.
gram_samples         the kernel's route restated: grad_util.gram_matrix, G = R^ W R^^T, F2, then the elimination of
                     draws_sample_params_kernel in its own order (no pivoting, the pivot row divided by sqrt(pivot)), the back substitution
                     and the Gram-space chi2.  Isolates the algebra from the device and gives the rounding floor of the Gram route.

Error measures, scaled so that the conditioning of F2 does not enter:
    samples      max |L^T (b - b_ref)|: the error in units of the conditional standard deviation along the whitened axes
    covariance   the call with S = nG and z = 1: X = b - b^ holds the columns of U^-1 as its rows, so X^T X = F2^-1 = K;
                 max |X^T X - K|_ij / sqrt(K_ii K_jj)
    identity     chi2(b) + prior(b) - [chi2(b^) + prior(b^)] = z^T z (b^ minimises the quadratic form whose Hessian is 2 F2), relative to
                 max(1, z^T z)"""
import numpy as np

import grad_util as GU
from oracle import marginal as M

# worst error of gram_samples against data_space_samples over the 12 draws x S = 5 of test_draw_samples.py (samples, identity) and the
# S = nG identity call (covariance), measured on the host, Jeffreys on and off alike (test_gram_route_matches_data_space_samples asserts
# them).  The device is held to hess_util.device_bar of each: 1e-10 where the floor is <= 1e-12, 100 times the floor elsewhere.
# (the identity subtracts two Gram-space chi2, each a cancelling sum of G's entries: its floor is the largest)
SAMPLE_FLOOR = {"auto": dict(samples=1.4e-12, covariance=2.1e-13, identity=1.1e-11),
                "cross": dict(samples=7.3e-12, covariance=1.8e-12, identity=4.0e-12),
                "full": dict(samples=1.6e-11, covariance=9.6e-13, identity=5.1e-11),
                "xnost": dict(samples=1.8e-11, covariance=3.8e-13, identity=4.1e-11)}


def _sinv(scale, nG):
    scale = np.asarray(scale, dtype=np.float64)
    return np.zeros(nG) if np.any(np.isinf(scale)) else 1.0 / scale**2


def prior_chi2(b, loc, scale):
    """(b - mu)^T sigma^-2 (b - mu) over the last axis of b (0 under a flat prior)"""
    b = np.asarray(b, dtype=np.float64)
    return np.sum((b - np.asarray(loc, dtype=np.float64)) ** 2 * _sinv(scale, b.shape[-1]), axis=-1)


def data_space_samples(V, D, invcov, loc, scale, z, jeffreys=False):
    """V [nG + 1, ndata] (row 0: the model at zero Gaussian parameters; grad_util.recipe_vectors), z [S, nG]
    -> dict(logp, fullchi2, best [nG], F2, L, b [S, nG], chi2 [S])"""
    logp, full, best, F = M.marginalized_logp(V[1:], V[0], D, invcov, loc, scale, jeffreys=jeffreys, return_best=True)
    F2 = 0.5 * (F["F2"] + F["F2"].T)
    L = np.linalg.cholesky(F2)
    z = np.asarray(z, dtype=np.float64)
    b = best + np.linalg.solve(L.T, z.T).T
    res = V[0] + b @ V[1:] - D
    chi2 = np.einsum("sa,ab,sb->s", res, invcov, res)
    return dict(logp=logp, fullchi2=full, best=best, F2=F2, L=L, b=b, chi2=chi2)


def samples_of_draw(rec, theta, f, templ, index, D, invcov, loc, scale, z, jeffreys=False, templn=None):
    """the yardstick for one draw"""
    V, _ = GU.recipe_vectors(rec, theta, f, templ, index, templn)
    return data_space_samples(V, D, invcov, loc, scale, z, jeffreys)


def chi2_at(rec, theta, f, templ, index, D, invcov, b, templn=None):
    """the yardstick's chi2 at given b [S, nG] (the device's own samples)"""
    V, _ = GU.recipe_vectors(rec, theta, f, templ, index, templn)
    res = V[0] + np.asarray(b, dtype=np.float64) @ V[1:] - D
    return np.einsum("sa,ab,sb->s", res, invcov, res)


def whitened_error(L, b, b_ref):
    return float(np.max(np.abs((np.asarray(b) - np.asarray(b_ref)) @ L))) if np.size(b) else 0.0


def covariance_error(F2, X):
    """X [nG, nG]: b - b^ of the call with z = 1 (row s: U^-1 e_s)"""
    K = np.linalg.inv(F2)
    s = np.sqrt(np.diag(K))
    return float(np.max(np.abs(X.T @ X - K) / np.outer(s, s)))


def identity_error(chi2, b, fullchi2, best, loc, scale, z):
    zz = np.sum(np.asarray(z, dtype=np.float64) ** 2, axis=-1)
    lhs = chi2 + prior_chi2(b, loc, scale) - (fullchi2 + prior_chi2(best, loc, scale))
    return float(np.max(np.abs(lhs - zz) / np.maximum(1.0, zz)))


# ----------------------------------------------------------------------------- the kernel's route
def gram_G(rec, theta, f, W):
    """R^ [ng1, J + 1] of one draw and G = R^ W R^^T (as grad_util.gram_adjoint)"""
    theta = np.asarray(theta, dtype=np.float64)
    ff = np.reshape(np.asarray(f, dtype=np.float64), (rec.ntr,))
    ntr, ng1, J1 = rec.ntr, rec.ng1, W.shape[0]
    R = np.zeros((ng1, J1))
    rows = rec.rows(theta[None], ff[None])[0]
    for t in range(ntr):
        R[:, 24 * t : 24 * t + 24] = rows[t]
    if J1 - 1 > 24 * ntr:
        rn = rec.rows_nnlo(theta[None], ff[None])[0]
        for t in range(ntr):
            R[:, 24 * ntr + 3 * t : 24 * ntr + 3 * t + 3] = rn[t]
    R[0, J1 - 1] = 1.0
    return R, (R @ W) @ R.T


def cholesky_rows(F2):
    """the elimination of draws_sample_params_kernel: column c, pivot a[c][c], r = sqrt(pivot); the rows i > c take m = a[i][c] / pivot and
    a[i][j] -= m a[c][j] (j > c); row c becomes a[c][j] / r (j >= c) -> U (upper, F2 = U^T U), ok (every pivot > 0)"""
    a = np.array(F2, dtype=np.float64)
    n = a.shape[0]
    ok = True
    for c in range(n):
        piv = a[c, c]
        if not piv > 0.0:
            ok = False
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.sqrt(piv)
            for i in range(c + 1, n):
                m = a[i, c] / piv
                a[i, c + 1 :] = a[i, c + 1 :] - m * a[c, c + 1 :]
            a[c, c:] = a[c, c:] / r
    return np.triu(a), ok


def gram_samples(rec, theta, f, W, loc, scale, z):
    """best [nG], b [S, nG] and chi2 [S] of one draw by the statements of draws_sample_params_kernel (NaN samples where a pivot is <= 0),
    and the full chi2 at best"""
    _, G = gram_G(rec, theta, f, W)
    nG = rec.ng1 - 1
    sinv, mu = _sinv(scale, nG), np.asarray(loc, dtype=np.float64)
    F2 = 0.5 * (G[1:, 1:] + G[1:, 1:].T) + np.diag(sinv)
    F1 = -G[1:, 0] + sinv * mu
    best = np.linalg.solve(F2, F1)
    U, ok = cholesky_rows(F2)
    z = np.asarray(z, dtype=np.float64)
    x = np.zeros_like(z)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(z.shape[0]):
            y = z[s].copy()
            for c in range(nG - 1, -1, -1):
                xc = y[c] / U[c, c]
                y[:c] = y[:c] - U[:c, c] * xc
                y[c] = xc
            x[s] = y
    b = best + x if ok else np.full_like(z, np.nan)
    full = lambda v: G[0, 0] + 2.0 * (v @ G[1:, 0]) + np.einsum("...i,ij,...j->...", v, G[1:, 1:], v)
    return best, b, full(b), full(best)
