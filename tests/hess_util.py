"""Yardsticks of d2 ln P / d theta d theta of the params draws (eftb_draws_logp_hess_params), NumPy only, beside grad_util.py; shared by the
CPU tests (test_draw_hessian.py) and the GPU tests (test_gpu_draws_hess.py).

data_space_hessian   the yardstick: the second derivative of the marginalised ln P taken on the masked data vector, from the oracle's own b
                     and F2 (oracle/marginal.py marginalized_logp), dV / d theta of DrawRecipe.jacobian and d2V of DrawRecipe.hessian.  It
                     never forms a Gram matrix of the templates: it shares nothing with the kernel's route.
richardson_hess      central differences of any gradient(theta) with one Richardson step: what pins the yardstick itself.
gram_hessian         the kernel's Gram-space route restated from DrawRecipe.derivative() / second_derivative(), in the style of
                     grad_util.gram_adjoint.

With V' = V - [D; 0], H = V' C^-1 (C^-1 symmetrised), v = (1, b), K = F2^-1, S = v v^T + [not Jeffreys] blockdiag(0, K) and
G_p = dV_p H^T + H dV_p^T:

    d2 chi2 / d theta_p d theta_q = sum ((S + S^T) H) . d2V_pq  +  sum (S + S^T)[g][h] dV_p[g] C^-1 dV_q[h]
                                    - 2 u_p^T K u_q  -  [not Jeffreys] tr(K G_p[1:,1:] K G_q[1:,1:]),       u_p = (G_p v)[1:]

Errors of an entry are scaled by mag_pq = 1/2 of the sum of the magnitudes of every product added up, not by |hess_pq|."""
import numpy as np

import grad_util as GU
from oracle import marginal as M


# worst |gram_hessian - data_space_hessian| / mag over the 12 draws of test_draw_hessian.py, measured on the host, Jeffreys on and off alike
# (test_gram_route_matches_data_space_hessian asserts them).  The device is held to 1e-10 of mag where this floor is <= 1e-12, to 100
# times the floor elsewhere.  The NNLO likelihood of the GPU tests measures its own floor on the host before it asks 1e-10 of the device.
GRAM_FLOOR = {"auto": 1.2e-13, "cross": 1.6e-12, "full": 9.8e-12, "xnost": 9.7e-13}


def device_bar(floor):
    return 1e-10 if floor <= 1e-12 else 100.0 * floor


def data_space_hessian(V, dV, d2V, D, invcov, loc, scale, jeffreys=False):
    """V [nG + 1, ndata], dV [nG + 1, ndata, P], d2V [nG + 1, ndata, P, P] -> ln P, hess [P, P], mag [P, P]"""
    logp, _, b, F = M.marginalized_logp(V[1:], V[0], D, invcov, loc, scale, jeffreys=jeffreys, return_best=True)
    K = np.linalg.inv(F["F2"])
    v = np.concatenate([[1.0], b])
    S = np.outer(v, v)
    if not jeffreys:
        S[1:, 1:] += K
    S2 = S + S.T
    Cs = 0.5 * (invcov + invcov.T)
    Vc = V.copy()
    Vc[0] -= D
    H = Vc @ Cs
    t1 = (S2 @ H)[:, :, None, None] * d2V  # [g, a, p, q]
    E = np.einsum("gh,ab,hbq->gaq", S2, Cs, dV, optimize=True)
    t2 = dV[:, :, :, None] * E[:, :, None, :]
    Gp = np.einsum("gap,ha->ghp", dV, H)
    Gp = Gp + Gp.transpose(1, 0, 2)
    u = np.einsum("ghp,h->gp", Gp, v)[1:]  # [nG, P]
    t3 = -2.0 * u[:, :, None] * (K @ u)[:, None, :]  # [i, p, q]
    hess = t1.sum(axis=(0, 1)) + t2.sum(axis=(0, 1)) + t3.sum(axis=0)
    mag = np.abs(t1).sum(axis=(0, 1)) + np.abs(t2).sum(axis=(0, 1)) + np.abs(t3).sum(axis=0)
    if not jeffreys:
        Mp = np.einsum("ik,kjp->ijp", K, Gp[1:, 1:])
        t4 = -Mp[:, :, :, None] * Mp.transpose(1, 0, 2)[:, :, None, :]  # [i, j, p, q]: M_p[i][j] M_q[j][i]
        hess = hess + t4.sum(axis=(0, 1))
        mag = mag + np.abs(t4).sum(axis=(0, 1))
    return logp, -0.5 * hess, 0.5 * mag


def recipe_vectors2(rec, theta, f, templ, index, templn=None):
    """V [ng1, ndata], dV [ng1, ndata, P] and d2V [ng1, ndata, P, P] of one draw"""
    th, ff = np.asarray(theta, dtype=np.float64)[None], np.reshape(np.asarray(f, dtype=np.float64), (1, rec.ntr))
    V, dV = GU.recipe_vectors(rec, theta, f, templ, index, templn)
    d2V = GU.model_vectors(rec.hessian(th, ff)[0], templ, index, rec.hessian_nnlo(th, ff)[0] if templn is not None else None, templn)
    return V, dV, d2V


def hessian_of_draw(rec, theta, f, templ, index, D, invcov, loc, scale, jeffreys=False, templn=None):
    """the yardstick for one draw -> ln P, hess [P, P], mag [P, P]"""
    V, dV, d2V = recipe_vectors2(rec, theta, f, templ, index, templn)
    return data_space_hessian(V, dV, d2V, D, invcov, loc, scale, jeffreys)


def richardson_hess(gradfun, theta, rel=2e-3):
    """d gradfun / d theta [P, P] (column p: the derivative along theta_p) by central differences at h = rel max(1, |theta_p|) and h / 2,
    combined in one Richardson step, as grad_util.richardson_grad"""
    theta = np.asarray(theta, dtype=np.float64)
    out = np.zeros((theta.size, theta.size))
    for p in range(theta.size):
        h = rel * max(1.0, abs(theta[p]))
        d = []
        for hh in (h, 0.5 * h):
            up, dn = theta.copy(), theta.copy()
            up[p] += hh
            dn[p] -= hh
            d.append((gradfun(up) - gradfun(dn)) / (up[p] - dn[p]))
        out[:, p] = (4.0 * d[1] - d[0]) / 3.0
    return out


def gram_hessian(rec, theta, f, W, loc, scale, jeffreys=False):
    """ln P, grad [P] and hess [P, P] of one draw by the statements of draws_logp_hess_params_kernel: the forward pass and S of
    grad_util.gram_adjoint, K = F2^-1 also under Jeffreys, Rbar = (S + S^T) H, then per pair p <= q
        t1  the records of DrawRecipe.second_derivative() against Rbar
        t2  the double sum over the derivative records of p and q: (S + S^T)[g_n][g_m] W[col_n][col_m]
        t3  -2 u_p . (K u_q), u_p and G_p[1:,1:] accumulated record by record from H and H^T v
        t4  -sum_ij M_p[i][j] M_q[j][i], M_p = K G_p[1:,1:]   (not under Jeffreys)
    and entry (q, p) a copy of (p, q)"""
    theta = np.asarray(theta, dtype=np.float64)
    ff = np.reshape(np.asarray(f, dtype=np.float64), (rec.ntr,))
    ntr, ng1, nG, P = rec.ntr, rec.ng1, rec.ng1 - 1, theta.size
    J1 = W.shape[0]
    R = np.zeros((ng1, J1))
    rows = rec.rows(theta[None], ff[None])[0]
    for t in range(ntr):
        R[:, 24 * t : 24 * t + 24] = rows[t]
    if J1 - 1 > 24 * ntr:
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
    b = np.linalg.solve(F2, F1)
    chi2 = F0 - F1 @ b + (0.0 if jeffreys else np.linalg.slogdet(F2 / (2 * np.pi))[1])
    K = np.linalg.inv(F2)
    v = np.concatenate([[1.0], b])
    S = np.outer(v, v)
    if not jeffreys:
        S[1:, 1:] += K
    S2 = S + S.T
    Rbar = S2 @ H
    hv = v @ H
    th = np.concatenate([theta, [1.0]])
    colof = lambda d: 24 * d["tracer"] + d["col"] if d["col"] < 24 else 24 * ntr + 3 * d["tracer"] + d["col"] - 24
    der = rec.derivative()
    dval = np.array([d["coef"] * ff[d["tracer"]] ** d["fpow"] * th[d["idx"][0]] * th[d["idx"][1]] for d in der])
    dcol = np.array([colof(d) for d in der], dtype=int)
    drow = np.array([d["row"] for d in der], dtype=int)
    grad = np.zeros(P)
    u = np.zeros((P, ng1))
    Gp = np.zeros((P, ng1, ng1))
    for n, d in enumerate(der):
        p, g, c = d["p"], drow[n], dcol[n]
        grad[p] += dval[n] * Rbar[g, c]
        u[p] += dval[n] * v[g] * H[:, c]
        u[p, g] += dval[n] * hv[c]
        Gp[p, g, :] += dval[n] * H[:, c]
        Gp[p, :, g] += dval[n] * H[:, c]
    hess = np.zeros((P, P))
    for d in rec.second_derivative():
        hess[d["p"], d["q"]] += d["coef"] * ff[d["tracer"]] ** d["fpow"] * th[d["idx"][0]] * Rbar[d["row"], colof(d)]
    Ku = u[:, 1:] @ K.T  # [q, i]: (K u_q)[i]
    Mp = np.einsum("ik,pkj->pij", K, Gp[:, 1:, 1:])
    for p in range(P):
        ip = np.nonzero(der["p"] == p)[0]
        for q in range(p, P):
            iq = np.nonzero(der["p"] == q)[0]
            t2 = np.sum(dval[ip][:, None] * dval[iq][None, :] * S2[np.ix_(drow[ip], drow[iq])] * W[np.ix_(dcol[ip], dcol[iq])])
            t3 = -2.0 * (u[p, 1:] @ Ku[q])
            t4 = 0.0 if jeffreys else -np.sum(Mp[p] * Mp[q].T)
            hess[p, q] = hess[q, p] = -0.5 * (hess[p, q] + t2 + t3 + t4)
    return -0.5 * chi2, -0.5 * grad, hess
