"""Yardsticks of d ln P / d theta of the params draws (eftb_draws_logp_grad_params), NumPy only; shared by the CPU tests
(test_draw_gradient.py) and the GPU tests (test_gpu_draws_grad.py).

data_space_adjoint   the yardstick: the adjoint of the marginalised ln P taken on the masked data vector, from the oracle's own b and F2
                     (oracle/marginal.py marginalized_logp) and dV / d theta of DrawRecipe.jacobian.  It never forms a Gram matrix of the
                     templates: it shares nothing with the kernel's route.
richardson_grad      central differences of any ln P(theta) with one Richardson step: what pins the yardstick itself.
gram_adjoint         the kernel's Gram-space formula restated (S, (S + S^T) H at the non-zeros, the derivative table), in the style of
                     emulate.py: isolates the algebra from the device and gives the rounding floor of the Gram route.

Errors of a gradient component are scaled by its magnitude mag_p = 1/2 sum |Rbar_V . dV_p| (the sum of the magnitudes of what is added
up), not by |grad_p|, which vanishes at a best fit."""
import numpy as np

from oracle import marginal as M


def model_vectors(rows, templ, index, rows_nnlo=None, templn=None):
    """rows [ntr, ng1, 24, ...] (trailing axes, e.g. P of a jacobian, ride along), templ [ntr, nl, 24, nx] of one walker, index of the
    data vector (l counts the ntr * nl multipoles of the walker's entries) -> V [ng1, ndata, ...]; rows_nnlo [ntr, ng1, 3, ...] act on
    rows 3 ... 5 of templn"""
    v = np.einsum("tgr...,tlrx->gtlx...", rows, templ)
    if rows_nnlo is not None:
        v = v + np.einsum("tgj...,tljx->gtlx...", rows_nnlo, templn[:, :, 3:6])
    ntr, nl, nx = templ.shape[0], templ.shape[1], templ.shape[3]
    return v.reshape((v.shape[0], ntr * nl * nx) + v.shape[4:])[:, index]


def data_space_adjoint(V, dV, D, invcov, loc, scale, jeffreys=False):
    """V [nG + 1, ndata] (row 0: the model at zero Gaussian parameters), dV [nG + 1, ndata, P] -> ln P, grad [P], mag [P].
    With v = (1, b): d chi2 = sum S dG, S = v v^T + [not Jeffreys] blockdiag(0, F2^-1), G = (V - [D; 0]) C^-1 (V - [D; 0])^T, so
    Rbar_V = d chi2 / d V = S (V - [D; 0]) (C^-1 + C^-T) and grad_p = -1/2 sum Rbar_V dV_p."""
    logp, _, b, F = M.marginalized_logp(V[1:], V[0], D, invcov, loc, scale, jeffreys=jeffreys, return_best=True)
    v = np.concatenate([[1.0], b])
    S = np.outer(v, v)
    if not jeffreys:
        S[1:, 1:] += np.linalg.inv(F["F2"])
    Vc = V.copy()
    Vc[0] -= D
    Rbar = S @ Vc @ (invcov + invcov.T)
    prod = Rbar[:, :, None] * dV
    return logp, -0.5 * prod.sum(axis=(0, 1)), 0.5 * np.abs(prod).sum(axis=(0, 1))


def richardson_grad(fun, theta, rel=2e-3):
    """d fun / d theta [P] by central differences at h = rel max(1, |theta_p|) and h / 2, combined in one Richardson step (error O(h^4))"""
    theta = np.asarray(theta, dtype=np.float64)
    out = np.zeros(theta.size)
    for p in range(theta.size):
        h = rel * max(1.0, abs(theta[p]))
        d = []
        for hh in (h, 0.5 * h):
            up, dn = theta.copy(), theta.copy()
            up[p] += hh
            dn[p] -= hh
            d.append((fun(up) - fun(dn)) / ((up[p] - dn[p])))
        out[p] = (4.0 * d[1] - d[0]) / 3.0
    return out


def recipe_vectors(rec, theta, f, templ, index, templn=None):
    """V [ng1, ndata] and dV [ng1, ndata, P] of one draw: theta [P], f [ntr] (a float with one tracer)"""
    th, ff = np.asarray(theta, dtype=np.float64)[None], np.reshape(np.asarray(f, dtype=np.float64), (1, rec.ntr))
    nn = templn is not None
    V = model_vectors(rec.rows(th, ff)[0], templ, index, rec.rows_nnlo(th, ff)[0] if nn else None, templn)
    dV = model_vectors(rec.jacobian(th, ff)[0], templ, index, rec.jacobian_nnlo(th, ff)[0] if nn else None, templn)
    return V, dV


def oracle_logp(rec, theta, f, templ, index, D, invcov, loc, scale, jeffreys=False, templn=None):
    th, ff = np.asarray(theta, dtype=np.float64)[None], np.reshape(np.asarray(f, dtype=np.float64), (1, rec.ntr))
    V = model_vectors(rec.rows(th, ff)[0], templ, index, rec.rows_nnlo(th, ff)[0] if templn is not None else None, templn)
    return M.marginalized_logp(V[1:], V[0], D, invcov, loc, scale, jeffreys=jeffreys)


def adjoint_of_draw(rec, theta, f, templ, index, D, invcov, loc, scale, jeffreys=False, templn=None):
    """the yardstick for one draw -> ln P, grad [P], mag [P]"""
    V, dV = recipe_vectors(rec, theta, f, templ, index, templn)
    return data_space_adjoint(V, dV, D, invcov, loc, scale, jeffreys)


# ----------------------------------------------------------------------------- the kernel's route
def gram_matrix(templ, index, D, invcov, templn=None):
    """W_c = A C^-1 A^T [J + 1, J + 1] of one walker as draws_gather_kernel / draws_gram_kernel build it: column (tau, r) at tau * 24 + r,
    the NNLO columns (tau, j) at ntr * 24 + 3 tau + j, the data row -D last; symmetrised"""
    ntr, nl, _, nx = templ.shape
    cols = []
    for tau in range(ntr):
        for r in range(24):
            z = np.zeros((ntr, nl, nx))
            z[tau] = templ[tau, :, r]
            cols.append(z.reshape(-1)[index])
    if templn is not None:
        for tau in range(ntr):
            for j in range(3):
                z = np.zeros((ntr, nl, nx))
                z[tau] = templn[tau, :, 3 + j]
                cols.append(z.reshape(-1)[index])
    A = np.stack(cols + [-np.asarray(D, dtype=np.float64)])
    W = A @ invcov @ A.T
    return 0.5 * (W + W.T)


def gram_adjoint(rec, theta, f, W, loc, scale, jeffreys=False):
    """ln P and grad [P] of one draw by the statements of draws_logp_grad_params_kernel: R^ from the recipe, H = R^ W, G = H R^^T, F2 / F1 /
    F0, b, S = v v^T + [not Jeffreys] blockdiag(0, F2^-1), Rbar = (S + S^T) H read at the entries the derivative records name, and the P
    sums over DrawRecipe.derivative() in table order"""
    theta = np.asarray(theta, dtype=np.float64)
    ff = np.reshape(np.asarray(f, dtype=np.float64), (rec.ntr,))
    ntr, ng1, nG = rec.ntr, rec.ng1, rec.ng1 - 1
    J1 = W.shape[0]
    nn = J1 - 1 > 24 * ntr
    R = np.zeros((ng1, J1))
    rows = rec.rows(theta[None], ff[None])[0]
    for t in range(ntr):
        R[:, 24 * t : 24 * t + 24] = rows[t]
    if nn:
        rn = rec.rows_nnlo(theta[None], ff[None])[0]
        for t in range(ntr):
            R[:, 24 * ntr + 3 * t : 24 * ntr + 3 * t + 3] = rn[t]
    R[0, J1 - 1] = 1.0
    H = R @ W
    G = H @ R.T
    scale = np.asarray(scale, dtype=np.float64)
    sinv = np.zeros(nG) if np.any(np.isinf(scale)) else 1.0 / scale**2
    mu = np.asarray(loc, dtype=np.float64)
    F2 = 0.5 * (G[1:, 1:] + G[1:, 1:].T) + np.diag(sinv)
    F1 = -G[1:, 0] + sinv * mu
    F0 = G[0, 0] + mu @ (sinv * mu)
    b = np.linalg.solve(F2, F1) if nG else np.zeros(0)
    chi2 = F0 - F1 @ b + (0.0 if jeffreys or not nG else np.linalg.slogdet(F2 / (2 * np.pi))[1])
    v = np.concatenate([[1.0], b])
    S = np.outer(v, v)
    if not jeffreys and nG:
        S[1:, 1:] += np.linalg.inv(F2)
    Rbar = (S + S.T) @ H
    th = np.concatenate([theta, [1.0]])
    grad = np.zeros(theta.size)
    for d in rec.derivative():
        col = 24 * d["tracer"] + d["col"] if d["col"] < 24 else 24 * ntr + 3 * d["tracer"] + d["col"] - 24
        grad[d["p"]] += d["coef"] * ff[d["tracer"]] ** d["fpow"] * th[d["idx"][0]] * th[d["idx"][1]] * Rbar[d["row"], col]
    return -0.5 * chi2, -0.5 * grad


# ----------------------------------------------------------------------------- the cases (tests/golden only)
def marg_templates(g):
    """templates [1, 3, 24, nx] and data index of tests/golden/marg.npz (as test_gpu_draws._marg, without an engine)"""
    from eftpipe_amd.marginal import data_index

    nx = g["binned_P11l"].shape[-1]
    T = np.concatenate([g["binned_P11l"], g["binned_Pctl"], g["binned_Ploopl"], g["binned_Pstl"]], axis=1)
    ls = list(g["ls"])
    return T[None], data_index(ls, {l: slice(a, b) for l, (a, b) in zip(ls, g["masks"])}, nx)


def cfg3_index(g, nb):
    import cfg3_util as U
    from eftpipe_amd.marginal import data_index

    return np.concatenate([data_index([int(l) for l in g[t + "_ls"]], U.masks(g, t), nb, tracer=i, nl=3) for i, t in enumerate(U.TRACERS)])
