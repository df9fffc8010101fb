"""Analytically marginalised log-posterior on the device.

Host mirror of what ``EFTLike`` + ``Marginalizable`` do per likelihood call in the reference
(eftpipe/likelihood.py:483-549 ``PNG``/``PG`` -> eftpipe/marginal.py:79-140 ``marginalized_logp``), for a whole batch
of walkers whose templates are already resident on the GPU: only ``B`` log-posteriors (and, on request, the best-fit
Gaussian parameters) cross PCIe instead of 0.3 MB of templates per walker.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib as L
from .parambasis import _ndraws, gaussian_params, gaussian_rows, gaussian_rows_many

MAXG = 24

# what MarginalLikelihood.sample_gaussian_params returns; fields that were not asked for are None
GaussianSamples = collections.namedtuple("GaussianSamples", "logp fullchi2 best b chi2 coef coef_nnlo plk")

# what MarginalLikelihood.metropolis_draws_params returns; fullchi2 and best are None unless return_best is set
DrawChains = collections.namedtuple("DrawChains", "theta logp naccept last fullchi2 best")
# what MarginalLikelihood.hmc_draws_params returns: the fields of DrawChains, then log_ratio (None unless return_ratio is set)
DrawTrajectories = collections.namedtuple("DrawTrajectories", "theta logp naccept last fullchi2 best log_ratio")
# what MarginalLikelihood.temper_draws_params returns; fullchi2 and best are None unless return_best is set
TemperedChains = collections.namedtuple("TemperedChains", "theta logp fullchi2 best last naccept nswap sum_logp beta")
DragChains = collections.namedtuple("DragChains", "theta logp_start logp_end last naccept last_logp_start last_logp_end sum_start sum_end log_ratio "
                                    "fullchi2_start fullchi2_end best_start best_end last_fullchi2_start last_fullchi2_end last_best_start last_best_end")


def data_index(ls, masks, nx, tracer=0, nl=None):
    """Flat indices l * nx + x of the data vector in the order of reference likelihood.py:167-195 (``flatten``):
    multipoles ``ls`` (even), each restricted to ``masks[ell]`` (a slice, or None for all bins).  With several tracers per
    likelihood point (``Engine.set_tracers``) the block of tracer t starts at multipole t * nl: pass ``tracer`` and ``nl`` (the
    multipoles per entry of the template block) and concatenate the tracers' indices in data-vector order."""
    out = []
    for ell in ls:
        sl = masks[ell] if masks and masks.get(ell) is not None else slice(0, nx)
        out.append((tracer * (nl or 0) + ell // 2) * nx + np.arange(nx)[sl])
    return np.concatenate(out).astype(np.int32)


def joint_gaussian_rows(bases, fs, params, names, scales):
    """Coefficient rows of a joint likelihood over several tracers (the device form of ``EFTLike.PNG`` / ``EFTLike.PG``, reference
    likelihood.py:430-530): tracer t contributes to marginalised parameter ``names[i]`` iff its basis lists that parameter.
    bases   one ``WestCoastBasis`` / ``EastCoastBasis`` per tracer (a cross spectrum's basis carries ``cross_prefix``)
    fs      growth rate per tracer entry; params: the non-Gaussian parameter values by name; scales: per tracer dict(kmA=, krA=, ndA=[, kmB=, ...])
    -> rows [ntr, len(names) + 1, 24] for one walker (row 0: the model at zero Gaussian parameters)."""
    out = np.zeros((len(bases), len(names) + 1, 24))
    for t, (basis, f, sc) in enumerate(zip(bases, fs, scales)):
        r = basis.gaussian_rows(float(f), params, **sc)
        own = gaussian_params(basis.prefix, tuple(basis.cross_prefix)) if basis.get_name() == "westcoast" else basis.gaussian_params()
        out[t, 0] = r[0]
        for i, n in enumerate(names):
            if n in own:
                out[t, 1 + i] = r[1 + own.index(n)]
    return out


def joint_gaussian_rows_many(bases, fs, params, names, scales):
    """joint_gaussian_rows for N draws: params maps each non-Gaussian parameter name to its values [N] (or one value shared by every
    draw); fs: growth rate per tracer, one value or [N] each -> rows [N, ntr, len(names) + 1, 24], the bits of joint_gaussian_rows draw
    for draw (the rows of MarginalLikelihood.logp_draws)."""
    per = [np.asarray(v) for v in params.values() if np.ndim(v) >= 1] + [np.asarray(f) for f in fs if np.ndim(f) >= 1]
    if not per:
        raise ValueError("no per-draw values: pass arrays [N]")
    N = _ndraws(*per)
    if len(fs) != len(bases) or len(scales) != len(bases):
        raise ValueError("one growth rate and one scale dict per tracer")
    out = np.zeros((N, len(bases), len(names) + 1, 24))
    for t, (basis, f, sc) in enumerate(zip(bases, fs, scales)):
        if basis.get_name() == "westcoast":
            ng = [np.stack([np.broadcast_to(np.asarray(params[x + p], dtype=np.float64), (N,)) for p in ("b1", "b2", "b4")], axis=1)
                  for x in (basis.cross_prefix or [basis.prefix])]
            r = gaussian_rows_many(f, ng[0], ng[1] if basis.is_cross() else None, **sc)
            own = gaussian_params(basis.prefix, tuple(basis.cross_prefix))
        else:
            ng = np.stack([np.broadcast_to(np.asarray(params[basis.prefix + p], dtype=np.float64), (N,)) for p in ("b1", "b2", "bG2")], axis=1)
            r = gaussian_rows_many(f, ng, basis="eastcoast", **sc)
            own = basis.gaussian_params()
        out[:, t, 0] = r[:, 0]
        for i, n in enumerate(names):
            if n in own:
                out[:, t, 1 + i] = r[:, 1 + own.index(n)]
    return out


def joint_draw_recipe(bases, names, scales, param_names=None, with_NNLO=False):
    """The recipe (``parambasis.DrawRecipe``) of ``joint_gaussian_rows_many(bases, fs, params, names, scales)``: theta holds the
    non-Gaussian parameters of all tracers, each name once (a cross basis reuses its parents' entries), in the order of ``param_names``
    (default: first appearance over the bases); f is [walkers, ntr].  Parameters a yaml derives from others stay the caller's business.
    with_NNLO: a marginalised NNLO parameter in ``names`` (``basis.cnnloA()``) gets its row in the NNLO columns, the derivative of
    ``nnlo_vector`` (reference parambasis.py:303-307, :429-435)."""
    from .parambasis import _POLY_F, _compile_recipe, _poly_theta, _recipe_names, nnlo_vector

    if len(scales) != len(bases):
        raise ValueError("one scale dict per tracer")
    names = [str(n) for n in names]
    pn = _recipe_names(param_names, [n for b in bases for n in b.non_gaussian_params()])
    rows = []
    for basis, sc in zip(bases, scales):
        v = {n: _poly_theta(pn.index(n)) for n in basis.non_gaussian_params()}
        r = basis.gaussian_rows(_POLY_F, v, **sc)
        west = basis.get_name() == "westcoast"
        own = gaussian_params(basis.prefix, tuple(basis.cross_prefix)) if west else basis.gaussian_params()[:7]
        nn = basis.cnnloA() if with_NNLO and not basis.is_cross() else []
        out = [list(r[0]) + [0.0] * 3]
        for n in names:
            main = list(r[1 + own.index(n)]) if n in own else [0.0] * 24
            unit = [1.0 if m == n else 0.0 for m in nn] + [0.0] * (2 - len(nn))
            tail = list(nnlo_vector(_POLY_F, v[basis.prefix + "b1"], unit, sc.get("krA", 0.25), basis.counterform())) if n in nn else [0.0] * 3
            out.append(main + tail)
        rows.append(out)
    return _compile_recipe(pn, rows, len(names) + 1)


class MarginalLikelihood:
    """Gaussian likelihood of one data vector with the linear bias parameters marginalised analytically.

    engine        an ``Engine`` whose template block has the shape the data were measured on (set the pipeline operator
                  -- window / binning / chained -- before constructing this object)
    index         ``data_index(...)`` or any int array of l * nx + x
    data, invcov  data vector [ndata] and inverse covariance [ndata, ndata]
    loc, scale    Gaussian prior of the marginalised parameters (scale = inf for all of them: flat prior)
    """

    def __init__(self, engine, index, data, invcov, loc, scale, jeffreys=False):
        self.eng = engine
        self.index = np.ascontiguousarray(index, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.float64)
        invcov = np.ascontiguousarray(invcov, dtype=np.float64)
        loc = np.ascontiguousarray(loc, dtype=np.float64)
        scale = np.asarray(scale, dtype=np.float64)
        self.nG = loc.size
        if self.nG > MAXG:
            raise ValueError(f"at most {MAXG} marginalised parameters")
        if np.any(np.isinf(scale)) and not np.all(np.isinf(scale)):
            raise ValueError("only support setting infinite scale for all parameters")  # reference marginal.py:222-226
        sinv = np.ascontiguousarray(np.zeros(self.nG) if np.all(np.isinf(scale)) else 1.0 / scale**2)
        if invcov.shape != (data.size, data.size) or self.index.size != data.size:
            raise ValueError("index, data and invcov disagree on the data-vector length")
        L.check(engine.lib.eftb_set_likelihood(engine._h, data.size, self.index.ctypes.data_as(C.POINTER(C.c_int32)), L.dptr(data),
                                               L.dptr(invcov), self.nG, L.dptr(loc), L.dptr(sinv)))
        L.check(engine.lib.eftb_set_option(engine._h, 1, int(bool(jeffreys))))

    def logp(self, rows, return_best=False, rows_nnlo=None):
        """rows [B, nG + 1, 24] (``parambasis.gaussian_rows`` per walker) -> ln P_marg [B]
        (+ full chi2 [B] and best-fit Gaussian parameters [B, nG]).  Raises like the reference when det F2 <= 0.
        With ``Engine.set_tracers(ntr)``: B = walkers * ntr entries (each tracer its own rows, zero rows for parameters that do
        not act on it) -> results per walker [B / ntr]."""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        B = rows.shape[0]
        if rows.shape[1:] != (self.nG + 1, 24):
            raise ValueError(f"rows must be [B, {self.nG + 1}, 24]")
        buf = np.zeros((B, MAXG + 1, 24))
        buf[:, : self.nG + 1] = rows
        self.eng.put("GROWS", buf)
        if self.eng.cfg.with_NNLO:  # coefficients of PctNNLOl per row (zeros unless given): [B, nG + 1, 3]
            bn = np.zeros((B, MAXG + 1, 3))
            if rows_nnlo is not None:
                bn[:, : self.nG + 1] = np.asarray(rows_nnlo, dtype=np.float64).reshape(B, self.nG + 1, 3)
            self.eng.put("GROWSN", bn)
        elif rows_nnlo is not None:
            raise ValueError("rows_nnlo needs an engine built with with_NNLO")
        self.eng.run(L.S_LOGP, B)
        out = self.eng.get("LOGP", (B // self.eng.ntracers, 2 + MAXG))
        if np.any(np.isnan(out[:, 0])):
            raise RuntimeError("det of F2ij <= 0")
        if return_best:
            return out[:, 0], out[:, 1], out[:, 2 : 2 + self.nG]
        return out[:, 0]


    def logp_draws(self, rows, offsets, return_best=False, rows_nnlo=None):
        """Many parameter draws against the current template block (``eftb_draws_logp``; the fast / slow split of reference
        theory.py:829-874): walker c (template entries c * ntr ... c * ntr + ntr - 1, left by eval_logp / eval_batch / put("TEMPL")) owns
        draws offsets[c] ... offsets[c + 1] - 1.  rows [N, ntr, nG + 1, 24] ([N, nG + 1, 24] with one tracer; ``joint_gaussian_rows_many``,
        ``parambasis.gaussian_rows_many``), rows_nnlo [N, ntr, nG + 1, 3] (with_NNLO engines) -> ln P_marg [N] (+ full chi2 [N] and
        best-fit Gaussian parameters [N, nG]).  Raises like the reference when det F2 <= 0."""
        ntr, ng1 = self.eng.ntracers, self.nG + 1
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        N = rows.shape[0] if rows.ndim else 0
        if rows.shape not in ((N, ntr, ng1, 24),) + (((N, ng1, 24),) if ntr == 1 else ()):
            raise ValueError(f"rows must be [N, {ntr}, {ng1}, 24]")
        rn = None
        if rows_nnlo is not None:
            if not self.eng.cfg.with_NNLO:
                raise ValueError("rows_nnlo needs an engine built with with_NNLO")
            rn = np.ascontiguousarray(rows_nnlo, dtype=np.float64)
            if rn.shape not in ((N, ntr, ng1, 3),) + (((N, ng1, 3),) if ntr == 1 else ()):
                raise ValueError(f"rows_nnlo must be [N, {ntr}, {ng1}, 3]")
        off = _offsets(offsets)
        logp, full, best = np.empty(N), np.empty(N), np.empty((N, self.nG))
        L.check(self.eng.lib.eftb_draws_logp(self.eng._h, off.size - 1, N, off.ctypes.data_as(C.POINTER(C.c_int64)), L.dptr(rows), L.dptr(rn),
                                             L.dptr(logp), L.dptr(full), L.dptr(best)))
        if np.any(np.isnan(logp)):
            raise RuntimeError("det of F2ij <= 0")
        return (logp, full, best) if return_best else logp

    def set_draw_recipe(self, recipe):
        """The draw recipe of ``logp_draws_params`` (``eftb_set_draw_recipe`` kind 0; ``joint_draw_recipe``): nG + 1 rows per tracer.  It
        belongs to this likelihood: constructing another ``MarginalLikelihood`` on the engine, or ``Engine.set_tracers``, drops it."""
        from .engine import _set_recipe

        self._recipe = _set_recipe(self.eng, L.RECIPE_LOGP, recipe, self.nG + 1)

    def set_datasets(self, data):
        """Data vectors that share this likelihood's index, covariance, priors and Jeffreys switch (``eftb_set_likelihood_datasets``): data
        [M, ndata], e.g. mock realisations; ``None`` withdraws them.  ``logp_draws_params`` and ``maximize_draws_params`` score draws
        against them through ``groups=``.  They belong to this likelihood: constructing another ``MarginalLikelihood`` on the engine, or
        ``Engine.set_tracers``, drops them.  Every other call keeps the one data vector the likelihood was constructed with."""
        if data is None:
            L.check(self.eng.lib.eftb_set_likelihood_datasets(self.eng._h, 0, None))
            return
        data = np.ascontiguousarray(data, dtype=np.float64)
        if data.ndim != 2 or data.shape[0] < 1 or data.shape[1] != self.index.size:
            raise ValueError(f"data must be [M, {self.index.size}]: M >= 1 data vectors of the likelihood's length")
        L.check(self.eng.lib.eftb_set_likelihood_datasets(self.eng._h, data.shape[0], L.dptr(data)))

    def logp_draws_params(self, theta, offsets, f, return_best=False, grad=False, hess=False, groups=None):
        """``logp_draws`` with the rows built on the device from parameter values (``eftb_draws_logp_params``): theta [N, P] in the order of
        the recipe's ``param_names``, f [C, ntr] ([C] with one tracer) the growth rate of each walker's entries -> ln P_marg [N] (+ full
        chi2 [N] and best-fit Gaussian parameters [N, nG]).  8 P bytes per draw cross PCIe instead of the rows.  Raises like the
        reference when det F2 <= 0.
        grad=True (``eftb_draws_logp_grad_params``): d ln P_marg / d theta [N, P] in ``param_names`` order from an adjoint pass on the device
        -> (logp, grad) or (logp, grad, full, best); ln P, full chi2 and the best fit are the bits of the call without it.
        grad=True, hess=True (``eftb_draws_logp_hess_params``): also d2 ln P_marg / d theta d theta [N, P, P], each draw's block equal to its
        transpose bit for bit -> (logp, grad, hess) or (logp, grad, hess, full, best); ln P, the gradient, full chi2 and the best fit are
        the gradient call's bits.  hess=True without grad raises ValueError.
        groups=(walker [G], dataset [G]) (``eftb_draws_logp_params_datasets``; ``set_datasets`` first): group g scores its draws
        offsets[g] ... offsets[g + 1] - 1 against the templates of walker[g] and data set dataset[g]; offsets is then [G + 1], f stays
        [C, ntr] per walker.  Groups come in any order and may repeat a walker or a data set.  Returns as without it; a group whose data set
        is the likelihood's own vector returns the bits of the call without ``groups``."""
        from .engine import _params_args

        if hess and not grad:
            raise ValueError("hess=True needs grad=True: the Hessian call returns the gradient too")
        if groups is not None:
            theta, off, f, wk, ds = _groups_args(getattr(self, "_recipe", None), theta, offsets, f, self.eng.ntracers, groups)
            logp, dlogp, d2logp, full, best = self._draws_groups_raw(theta, off, f, wk, ds, grad, hess)
            if np.any(np.isnan(logp)):
                raise RuntimeError("det of F2ij <= 0")
            out = (logp,) + ((dlogp,) if grad else ()) + ((d2logp,) if hess else ()) + ((full, best) if return_best else ())
            return out if len(out) > 1 else logp
        theta, off, f = _params_args(getattr(self, "_recipe", None), theta, offsets, f, self.eng.ntracers)
        N = theta.shape[0]
        if hess:
            logp, dlogp, d2logp, full, best = self._draws_hess_raw(theta, off, f)
            if np.any(np.isnan(logp)):
                raise RuntimeError("det of F2ij <= 0")
            return (logp, dlogp, d2logp, full, best) if return_best else (logp, dlogp, d2logp)
        logp, full, best = np.empty(N), np.empty(N), np.empty((N, self.nG))
        if grad:
            dlogp = np.empty((N, theta.shape[1]))
            L.check(self.eng.lib.eftb_draws_logp_grad_params(self.eng._h, off.size - 1, N, off.ctypes.data_as(C.POINTER(C.c_int64)), L.dptr(theta), L.dptr(f),
                                                             L.dptr(logp), L.dptr(dlogp), L.dptr(full), L.dptr(best)))
        else:
            L.check(self.eng.lib.eftb_draws_logp_params(self.eng._h, off.size - 1, N, off.ctypes.data_as(C.POINTER(C.c_int64)), L.dptr(theta), L.dptr(f),
                                                        L.dptr(logp), L.dptr(full), L.dptr(best)))
        if np.any(np.isnan(logp)):
            raise RuntimeError("det of F2ij <= 0")
        if grad:
            return (logp, dlogp, full, best) if return_best else (logp, dlogp)
        return (logp, full, best) if return_best else logp

    def _draws_hess_raw(self, theta, off, f):
        """``eftb_draws_logp_hess_params`` on checked arguments -> logp, grad, hess, full, best; NaN where det F2 <= 0, nothing raised for it"""
        N, P = theta.shape
        logp, full, best, dlogp, d2logp = np.empty(N), np.empty(N), np.empty((N, self.nG)), np.empty((N, P)), np.empty((N, P, P))
        L.check(self.eng.lib.eftb_draws_logp_hess_params(self.eng._h, off.size - 1, N, off.ctypes.data_as(C.POINTER(C.c_int64)), L.dptr(theta), L.dptr(f),
                                                         L.dptr(logp), L.dptr(dlogp), L.dptr(d2logp), L.dptr(full), L.dptr(best)))
        return logp, dlogp, d2logp, full, best

    def _draws_groups_raw(self, theta, off, f, wk, ds, grad=True, hess=True):
        """``eftb_draws_logp_params_datasets`` on checked arguments -> logp, grad (or None), hess (or None), full, best; NaN where det F2 <= 0,
        nothing raised for it"""
        N, P = theta.shape
        logp, full, best = np.empty(N), np.empty(N), np.empty((N, self.nG))
        dlogp = np.empty((N, P)) if grad else None
        d2logp = np.empty((N, P, P)) if hess else None
        i32p = C.POINTER(C.c_int32)
        nC = f.shape[0]
        L.check(self.eng.lib.eftb_draws_logp_params_datasets(self.eng._h, nC, wk.size, wk.ctypes.data_as(i32p), ds.ctypes.data_as(i32p), N,
                                                             off.ctypes.data_as(C.POINTER(C.c_int64)), L.dptr(theta), L.dptr(f), L.dptr(logp), L.dptr(dlogp),
                                                             L.dptr(d2logp), L.dptr(full), L.dptr(best)))
        return logp, dlogp, d2logp, full, best

    def sample_gaussian_params(self, theta, offsets, f, z, groups=None, predict=False, return_coef=False):
        """Samples of the marginalised parameters of params draws (``eftb_draws_sample_params``).  Given theta they are exactly Gaussian,
        b | theta, data ~ N(best, F2^-1), with and without Jeffreys; the device takes the Cholesky factor F2 = U^T U per draw and returns
        b = best + U^-1 z for the caller's standard normals z [N, S, nG] ([N, nG]: one sample per draw) -- the posterior of the
        counter-terms, stochastic terms and b3 behind a marginalised chain or the best fits of ``maximize_draws_params``.
        theta, offsets, f and ``groups`` as ``logp_draws_params``.  -> ``GaussianSamples(logp, fullchi2, best, b, chi2, coef, coef_nnlo,
        plk)``: logp [N], fullchi2 [N] and best [N, nG] are the bits of ``logp_draws_params(return_best=True)``; b [N, S, nG]; chi2
        [N, S] the full chi2 at each sample (z = 0 gives best and fullchi2 bit for bit); with ``return_coef`` coef [N, S, ntr, 24]
        ([N, S, 24] with one tracer) and, on with_NNLO engines, coef_nnlo [N, S, ntr, 3]: the rows ``Engine.reduce_draws`` takes; with
        ``predict`` plk [N, S, ntr, nl, nx] ([N, S, nl, nx]), the posterior-predictive P_l of every sample, the bits of
        ``reduce_draws(coef, offsets * S, bias_nnlo=coef_nnlo)``.  Fields not asked for are None.  A sample's bits depend neither on S
        nor on how the draws are split into calls.
        Raises RuntimeError("det of F2ij <= 0") where ln P is NaN, like its siblings, and RuntimeError("F2ij is not positive definite")
        where only the samples are (det F2 > 0 with an even number of negative eigenvalues); ValueError for ``predict`` with
        ``groups`` (the P_l kernel addresses templates by walker: feed coef to ``reduce_draws``)."""
        out = self._sample_raw(theta, offsets, f, z, groups, predict, return_coef)
        if np.any(np.isnan(out.logp)):
            raise RuntimeError("det of F2ij <= 0")
        if np.any(np.isnan(out.b)) or np.any(np.isnan(out.chi2)):
            raise RuntimeError("F2ij is not positive definite")
        return out

    def _sample_raw(self, theta, offsets, f, z, groups=None, predict=False, return_coef=False):
        """``sample_gaussian_params`` without the two RuntimeErrors: NaN where det F2 <= 0 or F2 is not positive definite"""
        from .engine import _params_args

        ntr, nG = self.eng.ntracers, self.nG
        if predict and groups is not None:
            raise ValueError("predict=True does not go with groups: P_l is reduced against a walker's templates (reduce_draws takes coef)")
        rec = getattr(self, "_recipe", None)
        wk = ds = None
        if groups is not None:
            theta, off, f, wk, ds = _groups_args(rec, theta, offsets, f, ntr, groups)
        else:
            theta, off, f = _params_args(rec, theta, offsets, f, ntr)
        N = theta.shape[0]
        z = np.ascontiguousarray(z, dtype=np.float64)
        if z.shape == (N, nG):
            z = z.reshape(N, 1, nG)
        if z.ndim != 3 or z.shape[0] != N or z.shape[2] != nG:
            raise ValueError(f"z must be [{N}, S, {nG}] standard normals ([{N}, {nG}] for one sample per draw)")
        S = z.shape[1]
        if S < 1:
            raise ValueError("z must be [N, S, nG] with S >= 1 samples per draw")
        nn = self.eng.cfg.with_NNLO
        logp, full, best = np.empty(N), np.empty(N), np.empty((N, nG))
        b, chi2 = np.empty((N, S, nG)), np.empty((N, S))
        coef = np.empty((N, S, ntr, 24)) if return_coef else None
        coefn = np.empty((N, S, ntr, 3)) if return_coef and nn else None
        i64p = C.POINTER(C.c_int64)
        if groups is not None:
            i32p = C.POINTER(C.c_int32)
            L.check(self.eng.lib.eftb_draws_sample_params_datasets(self.eng._h, f.shape[0], wk.size, wk.ctypes.data_as(i32p), ds.ctypes.data_as(i32p), N, S,
                                                                   off.ctypes.data_as(i64p), L.dptr(theta), L.dptr(f), L.dptr(z), L.dptr(logp), L.dptr(full),
                                                                   L.dptr(best), L.dptr(b), L.dptr(chi2), L.dptr(coef), L.dptr(coefn)))
            plk = None
        else:
            nl, nx = self.eng.dims
            plk = np.empty((N, S, ntr, nl, nx)) if predict else None
            L.check(self.eng.lib.eftb_draws_sample_params(self.eng._h, off.size - 1, N, S, off.ctypes.data_as(i64p), L.dptr(theta), L.dptr(f), L.dptr(z),
                                                          L.dptr(logp), L.dptr(full), L.dptr(best), L.dptr(b), L.dptr(chi2), L.dptr(coef), L.dptr(coefn),
                                                          L.dptr(plk)))
        if ntr == 1:  # (as reduce_draws: no tracer axis)
            coef, coefn, plk = (None if a is None else a.reshape(a.shape[:2] + a.shape[3:]) for a in (coef, coefn, plk))
        return GaussianSamples(logp, full, best, b, chi2, coef, coefn, plk)

    def metropolis_draws_params(self, theta0, offsets, f, step, lnu, thin=1, lower=None, upper=None, prior_loc=None, prior_scale=None, groups=None,
                                return_best=False):
        """Metropolis chains over theta at fixed templates, all T steps of all N chains in one device call (``eftb_draws_chain_params``): the
        fast steps of a dragging or oversampling sampler behind one slow step.  theta0 [N, P], offsets, f and ``groups`` as
        ``logp_draws_params``: chain n starts at theta0[n] and belongs to the walker (group) that owns draw n.  The target is
        ln P_marg(theta) + ln prior(theta) with the prior on theta given by box bounds ``lower`` / ``upper`` [P] (None or -inf / inf: none)
        and independent Gaussians ``prior_loc`` / ``prior_scale`` [P] (None or scale inf: none).  The caller supplies the randomness
        (``metropolis_proposals``): step [N, T, P], the proposal increments, and lnu [N, T], the logarithms of its uniforms; step t
        proposes theta + step[n, t], rejects it without an evaluation outside the box, and accepts iff ln P' is finite and
        lnu[n, t] < (ln P' + pri') - (ln P + pri).  A proposal with det F2 <= 0 is rejected, not an error.
        -> ``DrawChains(theta [N, K, P], logp [N, K], naccept [N], last [N, P], fullchi2, best)`` with K = T // thin: the state after steps
        thin, 2 thin, ..., its ln P_marg (the bits of ``logp_draws_params`` there) and, with ``return_best``, full chi2 [N, K] and best
        [N, K, nG]; ``last`` is the state after step T, the theta0 that continues the chains: a T-step call equals a T1-step call and a
        T2-step call from ``last`` bit for bit.  A chain's bits depend neither on the other chains nor on the split into calls.
        Raises RuntimeError("det of F2ij <= 0") where a chain's starting point has no finite ln P."""
        out = self._chains_raw(theta0, offsets, f, step, lnu, thin, lower, upper, prior_loc, prior_scale, groups, return_best)
        if np.any(out.naccept < 0):
            raise RuntimeError("det of F2ij <= 0")
        return out

    def _chains_raw(self, theta0, offsets, f, step, lnu, thin=1, lower=None, upper=None, prior_loc=None, prior_scale=None, groups=None, return_best=False):
        """``metropolis_draws_params`` without the RuntimeError: a chain that failed at its start has NaN states and naccept = -1"""
        theta0, off, f, wk, ds, step, lnu, thin, pri = self._chain_args(theta0, offsets, f, step, lnu, thin, lower, upper, prior_loc, prior_scale, groups)
        N, T, P = step.shape
        theta, logp, last, nacc, full, best = self._chain_out(N, T // thin, P, return_best)
        i64p = C.POINTER(C.c_int64)
        tail = (off.ctypes.data_as(i64p), L.dptr(theta0), L.dptr(f), L.dptr(step), L.dptr(lnu)) + tuple(L.dptr(a) for a in pri) + (
            L.dptr(theta), L.dptr(logp), L.dptr(full), L.dptr(best), L.dptr(last), nacc.ctypes.data_as(i64p))
        if groups is not None:
            i32p = C.POINTER(C.c_int32)
            L.check(self.eng.lib.eftb_draws_chain_params_datasets(self.eng._h, f.shape[0], wk.size, wk.ctypes.data_as(i32p), ds.ctypes.data_as(i32p), N, T,
                                                                  thin, *tail))
        else:
            L.check(self.eng.lib.eftb_draws_chain_params(self.eng._h, off.size - 1, N, T, thin, *tail))
        return DrawChains(theta, logp, nacc, last, full, best)

    def _chain_args(self, theta0, offsets, f, moves, lnu, thin, lower, upper, prior_loc, prior_scale, groups, name="step", kind="proposal increments",
                    unit="steps", per="step", thin_min=1, pair_words=(), flat=False):
        """the arguments the four sampler calls share as the library takes them, shape errors raised here -> theta0, off, f, walker, dataset (None
        without groups), moves, lnu, thin, [lower, upper, prior_loc, prior_scale].  The caller words its moves [N, T, P] (``name``, what ``kind`` of
        numbers they are, the ``unit`` T counts and the one lnu holds a uniform ``per``), says how small thin may be and, with ``pair_words``, that
        ``groups`` are the pairs of ``drag_draws_params`` in the wording of ``_groups_args``; ``flat``: the moves are one number per chain and
        step, [N, T] (the stretch factors of ``ensemble_draws_params``, whose lnu may be of either sign)"""
        from .engine import _params_args

        ntr = self.eng.ntracers
        rec = getattr(self, "_recipe", None)
        wk = ds = None
        if groups is not None or pair_words:
            theta0, off, f, wk, ds = _groups_args(rec, theta0, offsets, f, ntr, groups, *pair_words)
        else:
            theta0, off, f = _params_args(rec, theta0, offsets, f, ntr)
        N, P = theta0.shape
        moves = np.ascontiguousarray(moves, dtype=np.float64)
        if flat:
            if moves.ndim != 2 or moves.shape[0] != N or moves.shape[1] < 1:
                raise ValueError(f"{name} must be [{N}, T] {kind} with T >= 1 {unit}")
        elif moves.ndim != 3 or moves.shape[0] != N or moves.shape[2] != P or moves.shape[1] < 1:
            raise ValueError(f"{name} must be [{N}, T, {P}] {kind} with T >= 1 {unit}")
        T = moves.shape[1]
        lnu = np.ascontiguousarray(lnu, dtype=np.float64)
        if lnu.shape != (N, T):
            raise ValueError(f"{'lnq' if flat else 'lnu'} must be [{N}, {T}]: the logarithm of a uniform per chain and {per}")
        if thin != int(thin) or not thin_min <= thin <= T:
            raise ValueError(f"thin must be an integer in [{thin_min}, T = {T}]")
        thin = int(thin)
        pri = []
        for key, a in (("lower", lower), ("upper", upper), ("prior_loc", prior_loc), ("prior_scale", prior_scale)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape != (P,):
                    raise ValueError(f"{key} must be [{P}], one value per parameter")
            pri.append(a)
        return theta0, off, f, wk, ds, moves, lnu, thin, pri

    def _chain_out(self, N, K, P, return_best, slots=None):
        """the arrays a sampler call fills -> theta [N, K, P], logp [N, slots], last [N, P], naccept [N], and with ``return_best`` fullchi2
        [N, slots] and best [N, slots, nG], else None; slots = K unless the call keeps more records than states"""
        slots = K if slots is None else slots
        full = np.empty((N, slots)) if return_best else None
        best = np.empty((N, slots, self.nG)) if return_best else None
        return np.empty((N, K, P)), np.empty((N, slots)), np.empty((N, P)), np.empty(N, dtype=np.int64), full, best

    def temper_draws_params(self, theta0, offsets, f, beta, step, lnu, lnu_swap=None, swap_every=0, first_step=0, thin=1, lower=None, upper=None,
                            prior_loc=None, prior_scale=None, groups=None, return_best=False):
        """Parallel tempering over theta at fixed templates, all T steps and every swap of all ladders in one device call
        (``eftb_draws_temper_params``) instead of one chain call per swap interval.  beta [R] (``temper_ladder``) are the inverse temperatures,
        1 >= beta[0] > ... > beta[R - 1] >= 0, R <= 8; theta0 [N, P], offsets, f, ``groups``, the box and the Gaussian prior on theta are those of
        ``metropolis_draws_params`` with N = nlad R: chain n is rung n % R of ladder n // R, and every walker (group) owns a multiple of R
        chains.  Rung r targets beta[r] ln P_marg(theta) + ln prior(theta): ln P_marg is tempered as a whole, the Gaussian priors of the
        marginalised parameters with it; the prior on theta is not.  The caller supplies the randomness (``temper_proposals``): step [N, T, P],
        lnu [N, T] and lnu_swap [nlad, nsw, R - 1] with nsw = (first_step + T) // S - first_step // S, S = ``swap_every`` (0: no swaps).  Step i
        is global step g = first_step + i: the Metropolis step of ``metropolis_draws_params`` against the rung's target, then, if
        (g + 1) % S == 0, swap event j = (g + 1) // S - 1: the pairs (r, r + 1) with r = j mod 2 are exchanged iff
        lnu_swap[ladder, j_local, r] < (beta[r] - beta[r + 1]) (ln P[r + 1] - ln P[r]).  States move, temperatures stay: chain n is always at
        beta[n % R].
        -> ``TemperedChains(theta [N, K, P], logp [N, K], fullchi2, best, last [N, P], naccept [N], nswap [nlad, max(R - 1, 1)], sum_logp [N],
        beta [R])`` with K = T // thin: the states as ``DrawChains``, ln P untempered (the bits of ``logp_draws_params`` there), the accepted swaps
        per adjacent pair, and the sum of ln P over the call's T steps per rung (sum_logp / T is <ln P> at beta[r], the integrand of
        thermodynamic integration).  A call continues from ``last`` with first_step advanced by T, bit for bit.
        Raises RuntimeError("det of F2ij <= 0") where a rung's starting point has no finite ln P (its whole ladder fails)."""
        out = self._temper_raw(theta0, offsets, f, beta, step, lnu, lnu_swap, swap_every, first_step, thin, lower, upper, prior_loc, prior_scale, groups,
                               return_best)
        if np.any(out.naccept < 0):
            raise RuntimeError("det of F2ij <= 0")
        return out

    def _temper_raw(self, theta0, offsets, f, beta, step, lnu, lnu_swap=None, swap_every=0, first_step=0, thin=1, lower=None, upper=None, prior_loc=None,
                    prior_scale=None, groups=None, return_best=False):
        """``temper_draws_params`` without the RuntimeError: a ladder that failed at its start has NaN states and naccept = nswap = -1"""
        theta0, off, f, wk, ds, step, lnu, thin, pri = self._chain_args(theta0, offsets, f, step, lnu, thin, lower, upper, prior_loc, prior_scale, groups)
        N, T, P = step.shape
        beta = np.asarray(beta, dtype=np.float64)
        if beta.ndim != 1 or beta.size < 1:
            raise ValueError("beta must be [R]: the inverse temperatures of the rungs, R >= 1")
        beta = np.ascontiguousarray(beta)
        R = beta.size
        if N % R:
            raise ValueError(f"theta0 holds {N} chains, not a multiple of the R = {R} rungs of beta")
        for name, v in (("swap_every", swap_every), ("first_step", first_step)):
            if v != int(v) or v < 0:
                raise ValueError(f"{name} must be an integer >= 0")
        S, first = int(swap_every), int(first_step)
        nlad, nsw = N // R, ((first + T) // S - first // S if S else 0)
        if lnu_swap is not None:
            lnu_swap = np.ascontiguousarray(lnu_swap, dtype=np.float64)
            if lnu_swap.shape != (nlad, nsw, R - 1):
                raise ValueError(f"lnu_swap must be [{nlad}, {nsw}, {R - 1}]: the logarithm of a uniform per ladder, swap event and adjacent pair")
        elif nsw and R > 1 and nlad:
            raise ValueError(f"lnu_swap must be [{nlad}, {nsw}, {R - 1}]: the call holds {nsw} swap events")
        theta, logp, last, nacc, full, best = self._chain_out(N, T // thin, P, return_best)
        nswap, sums = np.empty((nlad, max(R - 1, 1)), dtype=np.int64), np.empty(N)
        i64p = C.POINTER(C.c_int64)
        head = (N, R, T, S, first, thin, off.ctypes.data_as(i64p), L.dptr(theta0), L.dptr(f), L.dptr(beta), L.dptr(step), L.dptr(lnu), L.dptr(lnu_swap))
        tail = tuple(L.dptr(a) for a in pri) + (L.dptr(theta), L.dptr(logp), L.dptr(full), L.dptr(best), L.dptr(last), nacc.ctypes.data_as(i64p),
                                                nswap.ctypes.data_as(i64p), L.dptr(sums))
        if groups is not None:
            i32p = C.POINTER(C.c_int32)
            L.check(self.eng.lib.eftb_draws_temper_params_datasets(self.eng._h, f.shape[0], wk.size, wk.ctypes.data_as(i32p), ds.ctypes.data_as(i32p), *head,
                                                                   *tail))
        else:
            L.check(self.eng.lib.eftb_draws_temper_params(self.eng._h, off.size - 1, *head, *tail))
        return TemperedChains(theta, logp, full, best, last, nacc, nswap, sums, beta)

    def ensemble_draws_params(self, starts, offsets, f, K, z, pick, lnq, thin=1, lower=None, upper=None, prior_loc=None, prior_scale=None, groups=None,
                              return_best=False):
        """Affine-invariant ensembles over theta at fixed templates (the stretch move of Goodman & Weare, as in emcee), all T sweeps of all
        ensembles in one device call (``eftb_draws_ensemble_params``) instead of 2 T ``logp_draws_params`` calls with the rule in NumPy
        between them.  An ensemble takes the scale and orientation of its proposals from its own members: the call needs no proposal matrix.
        starts [N, P], offsets, f, ``groups``, the box and the Gaussian prior on theta are those of ``metropolis_draws_params`` with
        N = nens K: chain n is member n % K of ensemble n // K, K even with 2 <= K <= 64, and every walker (group) owns a multiple of K
        chains.  Members 0 ... K/2 - 1 are half 0, the rest half 1.  The caller supplies the randomness (``stretch_proposals``): z [N, T] > 0,
        pick [N, T] in [0, K/2) and lnq [N, T].  Sweep t moves half 0 against the current half 1, then half 1 against the new half 0: member
        k proposes theta_j + z[n, t] (theta_k - theta_j) with j = member pick[n, t] of the other half, rejects it without an evaluation
        outside the box, and accepts iff ln P' is finite and lnq[n, t] < (ln P' + pri') - (ln P + pri).  lnq = ln u - (P - 1) ln z carries the
        Jacobian of the stretch, so it may be positive.
        -> ``DrawChains(theta [N, Kt, P], logp [N, Kt], naccept [N], last [N, P], fullchi2, best)`` with Kt = T // thin, as
        ``metropolis_draws_params``; a T-sweep call equals a T1-sweep call and a T2-sweep call from ``last`` bit for bit.
        Raises RuntimeError("det of F2ij <= 0") where a member's starting point has no finite ln P (its whole ensemble fails)."""
        out = self._ensemble_raw(starts, offsets, f, K, z, pick, lnq, thin, lower, upper, prior_loc, prior_scale, groups, return_best)
        if np.any(out.naccept < 0):
            raise RuntimeError("det of F2ij <= 0")
        return out

    def _ensemble_raw(self, starts, offsets, f, K, z, pick, lnq, thin=1, lower=None, upper=None, prior_loc=None, prior_scale=None, groups=None,
                      return_best=False):
        """``ensemble_draws_params`` without the RuntimeError: an ensemble that failed at its start has NaN states and naccept = -1"""
        theta0, off, f, wk, ds, z, lnq, thin, pri = self._chain_args(starts, offsets, f, z, lnq, thin, lower, upper, prior_loc, prior_scale, groups,
                                                                     name="z", kind="stretch factors", unit="sweeps", per="sweep", flat=True)
        (N, T), P = z.shape, theta0.shape[1]
        if K != int(K):
            raise ValueError("K must be an integer: the members of an ensemble")
        K = int(K)
        if K < 1 or N % K:
            raise ValueError(f"starts holds {N} chains, not a multiple of the K = {K} members of an ensemble")
        pick = np.asarray(pick)
        if pick.shape != (N, T) or pick.dtype.kind not in "iu":
            raise ValueError(f"pick must be [{N}, {T}] integers: the partner of every member in every sweep")
        pick = np.ascontiguousarray(pick, dtype=np.int32)
        theta, logp, last, nacc, full, best = self._chain_out(N, T // thin, P, return_best)
        i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        tail = (N, K, T, thin, off.ctypes.data_as(i64p), L.dptr(theta0), L.dptr(f), L.dptr(z), pick.ctypes.data_as(i32p), L.dptr(lnq)) + tuple(
            L.dptr(a) for a in pri) + (L.dptr(theta), L.dptr(logp), L.dptr(full), L.dptr(best), L.dptr(last), nacc.ctypes.data_as(i64p))
        if groups is not None:
            L.check(self.eng.lib.eftb_draws_ensemble_params_datasets(self.eng._h, f.shape[0], wk.size, wk.ctypes.data_as(i32p), ds.ctypes.data_as(i32p),
                                                                     *tail))
        else:
            L.check(self.eng.lib.eftb_draws_ensemble_params(self.eng._h, off.size - 1, *tail))
        return DrawChains(theta, logp, nacc, last, full, best)

    def hmc_draws_params(self, theta0, offsets, f, momentum, lnu, eps, nleap, factor=None, thin=1, lower=None, upper=None, prior_loc=None, prior_scale=None,
                         groups=None, return_best=False, return_ratio=False):
        """Hamiltonian Monte Carlo over theta at fixed templates, all T trajectories of nleap leapfrog steps of all N chains in one device call
        (``eftb_draws_hmc_params``) instead of one gradient call per leapfrog step.  theta0, offsets, f, ``groups``, the box and the Gaussian
        prior on theta are those of ``metropolis_draws_params``; the target is ln P_marg(theta) + ln prior(theta) and its gradient the bits of
        ``logp_draws_params(..., grad=True)`` plus the prior's.  The caller supplies the randomness (``hmc_momenta``) and the tuning:
        momentum [N, T, P] standard normals, lnu [N, T] logarithms of uniforms, eps the leapfrog step size (a scalar, [N] or [N, T]: jitter and
        adapt it between calls), nleap the steps per trajectory and factor a lower-triangular F [P, P] or [N, P, P] with mass matrix
        M^-1 = F F^T (``proposal_factor(H, scale=1.0)`` at a best fit; None: the identity).  A trajectory that leaves the box or meets a
        ln P or gradient that is not finite is aborted and rejected (no reflection); otherwise it is accepted iff
        lnu[n, t] < log_ratio[n, t], the change of ln pi - |r|^2 / 2 along it.
        -> ``DrawTrajectories(theta [N, K, P], logp [N, K], naccept [N], last [N, P], fullchi2, best, log_ratio)`` with K = T // thin as
        ``DrawChains``; with ``return_ratio`` log_ratio [N, T] (NaN where the trajectory was aborted), what a dual-averaging step-size
        adaptation needs.  A T-trajectory call equals a T1 and a T2 call from ``last`` bit for bit.
        Raises RuntimeError("det of F2ij <= 0") where a chain's starting point has no finite ln P."""
        out = self._hmc_raw(theta0, offsets, f, momentum, lnu, eps, nleap, factor, thin, lower, upper, prior_loc, prior_scale, groups, return_best, return_ratio)
        if np.any(out.naccept < 0):
            raise RuntimeError("det of F2ij <= 0")
        return out

    def _hmc_raw(self, theta0, offsets, f, momentum, lnu, eps, nleap, factor=None, thin=1, lower=None, upper=None, prior_loc=None, prior_scale=None,
                 groups=None, return_best=False, return_ratio=False):
        """``hmc_draws_params`` without the RuntimeError: a chain that failed at its start has NaN states and ratios and naccept = -1"""
        theta0, off, f, wk, ds, mom, lnu, thin, pri = self._chain_args(theta0, offsets, f, momentum, lnu, thin, lower, upper, prior_loc, prior_scale, groups,
                                                                       "momentum", "standard normals", "trajectories", "trajectory")
        N, T, P = mom.shape
        eps = np.asarray(eps, dtype=np.float64)
        if eps.shape not in ((), (N,), (N, T)):
            raise ValueError(f"eps must be a scalar, [{N}] or [{N}, {T}]: the leapfrog step size")
        eps = np.ascontiguousarray(np.broadcast_to(eps if eps.ndim != 1 else eps[:, None], (N, T)))
        if isinstance(nleap, bool) or nleap != int(nleap) or int(nleap) < 1:
            raise ValueError("nleap must be an integer >= 1: the leapfrog steps of a trajectory")
        nleap = int(nleap)
        if factor is not None:
            factor = np.asarray(factor, dtype=np.float64)
            if factor.shape not in ((P, P), (N, P, P)):
                raise ValueError(f"factor must be [{P}, {P}] or [{N}, {P}, {P}]: a lower-triangular F with M^-1 = F F^T")
            factor = np.ascontiguousarray(np.broadcast_to(factor, (N, P, P)))
        theta, logp, last, nacc, full, best = self._chain_out(N, T // thin, P, return_best)
        ratio = np.empty((N, T)) if return_ratio else None
        i64p = C.POINTER(C.c_int64)
        tail = (off.ctypes.data_as(i64p), L.dptr(theta0), L.dptr(f), L.dptr(mom), L.dptr(lnu), L.dptr(eps), L.dptr(factor)) + tuple(L.dptr(a) for a in pri) + (
            L.dptr(theta), L.dptr(logp), L.dptr(full), L.dptr(best), L.dptr(last), nacc.ctypes.data_as(i64p), L.dptr(ratio))
        if groups is not None:
            i32p = C.POINTER(C.c_int32)
            L.check(self.eng.lib.eftb_draws_hmc_params_datasets(self.eng._h, f.shape[0], wk.size, wk.ctypes.data_as(i32p), ds.ctypes.data_as(i32p), N, T,
                                                                nleap, thin, *tail))
        else:
            L.check(self.eng.lib.eftb_draws_hmc_params(self.eng._h, off.size - 1, N, T, nleap, thin, *tail))
        return DrawTrajectories(theta, logp, nacc, last, full, best, ratio)

    def drag_draws_params(self, theta0, offsets, f, pairs, step, lnu, frac=None, thin=0, lower=None, upper=None, prior_loc=None, prior_scale=None,
                          return_best=False):
        """The fast steps of a dragging sampler (cobaya's ``drag: true``) between two slow points, all T steps of all N chains in one device
        call (``eftb_draws_drag_params``).  The C walkers of the resident template block are the slow points, f [C, ntr] their growth
        rates; pairs = (start [G], end [G]) names the walkers each pair drags between (repeats and start = end allowed) and pair g owns the
        chains offsets[g] ... offsets[g + 1] - 1 (offsets [G + 1]).  theta0, step, lnu, the box and the Gaussian prior on theta are those of
        ``metropolis_draws_params``.  Step t of a chain targets
            (1 - frac[t]) ln pi_start(theta) + frac[t] ln pi_end(theta),      ln pi_x = ln P_marg of walker x + ln prior(theta),
        with frac [T] in [0, 1]; ``None`` is ``drag_fractions(T)``, cobaya's schedule.  Along the way the call sums ln pi_start and ln pi_end
        of the current state, the starting state included: T + 1 terms each.
        -> ``DragChains``: theta [N, K, P], logp_start and logp_end [N, K] after steps thin, 2 thin, ... (K = T // thin; thin = 0, a
        sampler's normal use, stores no trajectory); last [N, P], naccept [N], last_logp_start and last_logp_end [N] after step T; sum_start,
        sum_end [N] and log_ratio = (sum_end - sum_start) / (T + 1), the logarithm of the acceptance ratio of the whole slow + fast move
        (``drag_accept``).  With ``return_best`` the fields fullchi2_* and best_* [.., nG] of both walkers are filled too, else None.
        Every ln P, chi2 and best fit is the bit pattern ``logp_draws_params`` returns for that walker at that theta, and a chain's bits
        depend neither on the other chains nor on the order of the pairs.
        Raises RuntimeError("det of F2ij <= 0") where a chain's starting point has no finite ln P at either walker."""
        out = self._drag_raw(theta0, offsets, f, pairs, step, lnu, frac, thin, lower, upper, prior_loc, prior_scale, return_best)
        if np.any(out.naccept < 0):
            raise RuntimeError("det of F2ij <= 0")
        return out

    def _drag_raw(self, theta0, offsets, f, pairs, step, lnu, frac=None, thin=0, lower=None, upper=None, prior_loc=None, prior_scale=None, return_best=False):
        """``drag_draws_params`` without the RuntimeError: a chain that failed at its start has NaN states, records and sums and naccept = -1"""
        theta0, off, f, wa, wb, step, lnu, thin, pri = self._chain_args(theta0, offsets, f, step, lnu, thin, lower, upper, prior_loc, prior_scale, pairs,
                                                                        thin_min=0, pair_words=("pairs must be (start [G], end [G])", "pair"))
        N, T, P = step.shape
        frac = drag_fractions(T) if frac is None else np.ascontiguousarray(frac, dtype=np.float64)
        if frac.shape != (T,):
            raise ValueError(f"frac must be [{T}]: the weight of the end point at every step")
        K = T // thin if thin else 0
        theta, la, last, nacc, fa, ba = self._chain_out(N, K, P, return_best, slots=K + 1)  # (the record of the state after step T in the last slot)
        lb, fb, bb = (None if a is None else np.empty_like(a) for a in (la, fa, ba))
        sums = np.empty((N, 2))
        i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
        L.check(self.eng.lib.eftb_draws_drag_params(self.eng._h, f.shape[0], wa.size, wa.ctypes.data_as(i32p), wb.ctypes.data_as(i32p), N, T, thin,
                                                    off.ctypes.data_as(i64p), L.dptr(theta0), L.dptr(f), L.dptr(frac), L.dptr(step), L.dptr(lnu),
                                                    *[L.dptr(a) for a in pri], L.dptr(theta), L.dptr(la), L.dptr(lb), L.dptr(fa), L.dptr(fb), L.dptr(ba),
                                                    L.dptr(bb), L.dptr(last), nacc.ctypes.data_as(i64p), L.dptr(sums)))
        sa, sb = sums[:, 0].copy(), sums[:, 1].copy()
        cut = lambda a: (None, None) if a is None else (a[:, :K], a[:, K])
        (fak, fal), (fbk, fbl), (bak, bal), (bbk, bbl) = cut(fa), cut(fb), cut(ba), cut(bb)
        return DragChains(theta, la[:, :K], lb[:, :K], last, nacc, la[:, K], lb[:, K], sa, sb, (sb - sa) / (T + 1), fak, fbk, bak, bbk, fal, fbl, bal, bbl)

    def maximize_draws_params(self, theta0, offsets, f, groups=None, **kw):
        """Best fits over the recipe's parameters at fixed cosmology: ``newton_maximize`` fed with the Hessian call, all starts of all
        walkers at once (theta0 [N, P], offsets and f as ``logp_draws_params``; kw: max_iter, tol) -> theta, logp, grad, hess, n_iter,
        converged.  A point whose ln P is NaN (det F2 <= 0) is not an error here: a trial there is rejected, a start there is left where it
        is with converged False.  Priors and bounds on theta are the sampler's business, not this call's.
        groups=(walker [G], dataset [G]) as in ``logp_draws_params``: the starts of group g climb the posterior of data set dataset[g] --
        the best fits of many mocks in one call."""
        from .engine import _params_args

        if groups is not None:
            theta0, off, f, wk, ds = _groups_args(getattr(self, "_recipe", None), theta0, offsets, f, self.eng.ntracers, groups)
            return newton_maximize(lambda th: self._draws_groups_raw(np.ascontiguousarray(th), off, f, wk, ds)[:3], theta0, **kw)
        theta0, off, f = _params_args(getattr(self, "_recipe", None), theta0, offsets, f, self.eng.ntracers)
        return newton_maximize(lambda th: self._draws_hess_raw(np.ascontiguousarray(th), off, f)[:3], theta0, **kw)

    def eval_logp(self, Pin, f, DA, H, rows, return_best=False):
        """Theory + likelihood in one call (``eftb_eval_logp_batch``): Pin [B, Nkin], f/DA/H [B], rows [B, nG + 1, 24] ->
        ln P_marg [B]; only the inputs and B floats cross PCIe.  The engine's pipeline operator must bring the templates to
        the shape the data index refers to."""
        B, Pin, f, DA, H = self.eng._inputs(Pin, f, DA, H)
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        if rows.shape != (B, self.nG + 1, 24):
            raise ValueError(f"rows must be [{B}, {self.nG + 1}, 24]")
        nw = B // self.eng.ntracers
        logp, full, best = np.empty(nw), np.empty(nw), np.empty((nw, self.nG))
        L.check(self.eng.lib.eftb_eval_logp_batch(self.eng._h, B, L.dptr(Pin), L.dptr(f), L.dptr(DA), L.dptr(H), L.dptr(rows),
                                                  L.dptr(logp), L.dptr(full), L.dptr(best)))
        self.eng.dims = self.eng.out_dims()  # (the shape of the template block this run leaves)
        if np.any(np.isnan(logp)):
            raise RuntimeError("det of F2ij <= 0")
        return (logp, full, best) if return_best else logp


def _offsets(offsets):
    """walker boundaries of a draw call as int64 [C + 1] (the library checks their values)"""
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    if off.ndim != 1 or off.size < 2:
        raise ValueError("offsets must be [C + 1]: walker c owns draws offsets[c] ... offsets[c + 1] - 1")
    return off


def _groups_args(recipe, theta, offsets, f, ntr, groups, what="groups must be (walker [G], dataset [G])", unit="group"):
    """theta [N, P], offsets [G + 1], f [C, ntr] and groups = (walker [G], dataset [G]) of a groups call as the library takes them; shape
    errors are raised here, the values (a walker or data set out of range) are the library's to refuse.  ``drag_draws_params`` passes its
    pairs (start [G], end [G]) through here with its own wording."""
    try:
        wk, ds = groups
    except (TypeError, ValueError):
        raise ValueError(what) from None
    wk, ds = np.asarray(wk), np.asarray(ds)
    if wk.ndim != 1 or wk.shape != ds.shape or wk.size < 1:
        raise ValueError(what + ": two integer arrays of one length G >= 1")
    for a in (wk, ds):
        if a.dtype.kind not in "iu" or np.any(a != a.astype(np.int32)):
            raise ValueError(what + ": integers")
    from .engine import _theta_f_args

    theta, f = _theta_f_args(recipe, theta, f, ntr)
    off = np.ascontiguousarray(offsets, dtype=np.int64)
    if off.ndim != 1 or off.size != wk.size + 1:
        raise ValueError(f"offsets must be [{wk.size + 1}]: {unit} g owns draws offsets[g] ... offsets[g + 1] - 1")
    return theta, off, f.reshape(-1, ntr), np.ascontiguousarray(wk, dtype=np.int32), np.ascontiguousarray(ds, dtype=np.int32)


def newton_maximize(fun, theta0, max_iter=50, tol=1e-8):
    """Maximise ln P from M starting points at once by a Levenberg-damped Newton ascent, in NumPy.

    fun(theta [M, P]) -> (logp [M], grad [M, P], hess [M, P, P]).  It is always called with all M points, the frozen ones at their
    place and their results unused, so a device call with fixed walker offsets can stand behind it.
    -> theta [M, P], logp [M], grad [M, P], hess [M, P, P], n_iter [M], converged [M]; n_iter counts the trial steps of a point, each
    one evaluation of fun.

    Per point and iteration (-H + lam I) delta = g is solved; lam starts at its floor 0, the pure Newton step.
    - The trial theta + delta is accepted where ln P rises; lam then falls by 10, to 0 once below lam0 / 10.
    - Elsewhere (ln P not higher, or ln P or a derivative NaN at the trial) the point stays and lam grows by 10, from 0 to lam0.
      lam0 is three times the smallest |eigenvalue| of -H: the first damped step is a quarter of the Newton step along the flattest
      direction.  Where -H + lam I is not positive definite no trial is made and lam grows to at least twice the most negative
      eigenvalue's size.
    - A point is converged, and frozen, when lam is 0, -H is positive definite and the Newton decrement g^T (-H)^-1 g <= tol.  That
      last step is still taken where ln P rises by it, so ln P at the result is short of the maximum by the decrement's square, not
      by tol / 2.  The default tol is the absolute accuracy ln P itself is pinned to (1e-10 relative at chi2 ~ 1e2).
    - A start whose ln P or derivatives are not finite is left where it is, unconverged.
    It is a local method: where ln P has several maxima, the one a start ends in depends on the damping.
    Priors and bounds on theta are out of scope: they are the sampler's business."""
    theta = np.array(theta0, dtype=np.float64)
    if theta.ndim != 2:
        raise ValueError("theta0 must be [M, P]")
    M, P = theta.shape
    finite = lambda lp, g, H: np.isfinite(lp) & np.all(np.isfinite(g), axis=1) & np.all(np.isfinite(H), axis=(1, 2))
    logp, grad, hess = (np.array(a, dtype=np.float64) for a in fun(theta))
    alive = finite(logp, grad, hess)
    lam, n_iter, converged = np.zeros(M), np.zeros(M, dtype=np.int64), np.zeros(M, dtype=bool)
    eye = np.eye(P)
    for _ in range(max_iter):
        act = np.nonzero(alive & ~converged)[0]
        if act.size == 0:
            break
        A = -hess[act] + lam[act, None, None] * eye
        A = 0.5 * (A + A.transpose(0, 2, 1))
        w = np.linalg.eigvalsh(A) if P else np.ones((act.size, 1))
        pd = w[:, 0] > 0.0
        wh = w - lam[act, None]  # (the eigenvalues of -H)
        lam0 = 3.0 * np.min(np.abs(wh), axis=1)
        lam0 = np.where(lam0 > 0.0, lam0, 1e-3 * np.max(np.abs(wh), axis=1) + 1e-300)
        delta = np.zeros((act.size, P))
        if P and np.any(pd):
            delta[pd] = np.linalg.solve(A[pd], grad[act][pd][:, :, None])[:, :, 0]
        dec = np.sum(grad[act] * delta, axis=1)
        done = pd & (lam[act] == 0.0) & (dec <= tol)
        converged[act[done]] = True  # (after this last step, if ln P still rises by it: it halves what the decrement leaves of ln P)
        go = pd
        ok = np.zeros(act.size, dtype=bool)
        if np.any(go):
            trial = theta.copy()
            trial[act[go]] += delta[go]
            lp_t, g_t, H_t = (np.asarray(a, dtype=np.float64) for a in fun(trial))
            n_iter[act[go]] += 1
            with np.errstate(invalid="ignore"):
                ok = go & finite(lp_t, g_t, H_t)[act] & (lp_t[act] > logp[act])
            acc = act[ok]
            theta[acc], logp[acc], grad[acc], hess[acc] = trial[acc], lp_t[acc], g_t[acc], H_t[acc]
            lam[acc] = np.where(lam[acc] * 0.1 < 0.1 * lam0[ok], 0.0, lam[acc] * 0.1)
        rej = ~ok & ~done
        grown = np.where(lam[act] == 0.0, lam0, lam[act] * 10.0)
        lam[act[rej]] = np.where(pd, grown, np.maximum(grown, -2.0 * wh[:, 0]))[rej]
    return theta, logp, grad, hess, n_iter, converged


def proposal_factor(hess, scale=None):
    """Lower Cholesky factor L of the Gaussian proposal covariance scale^2 (-H)^-1 at a maximum: hess [P, P] or [N, P, P], the Hessian of
    ln P from ``logp_draws_params(..., hess=True)`` or ``maximize_draws_params`` -> L [P, P] or [N, P, P] with L L^T (-H) = scale^2 I.
    scale defaults to 2.38 / sqrt(P), the optimal random-walk scaling of a Gaussian target.  ValueError where -H is not positive definite
    (no maximum: a proposal cannot be taken from the curvature there)."""
    H = np.asarray(hess, dtype=np.float64)
    if H.ndim not in (2, 3) or H.shape[-1] != H.shape[-2] or H.shape[-1] < 1:
        raise ValueError("hess must be [P, P] or [N, P, P]")
    P = H.shape[-1]
    scale = 2.38 / np.sqrt(P) if scale is None else float(scale)
    A = -0.5 * (H + np.swapaxes(H, -1, -2))
    if not np.all(np.isfinite(A)):
        raise ValueError("-H is not positive definite (not finite)")
    try:
        np.linalg.cholesky(A)  # (raises where -H is not positive definite)
        cov = np.linalg.inv(A)
        return scale * np.linalg.cholesky(0.5 * (cov + np.swapaxes(cov, -1, -2)))
    except np.linalg.LinAlgError:
        raise ValueError("-H is not positive definite") from None


def metropolis_proposals(rng, N, T, factor):
    """The randomness of ``MarginalLikelihood.metropolis_draws_params`` from a ``numpy.random.Generator``: -> (step [N, T, P], lnu [N, T]) with
    step = z @ factor^T for standard normals z [N, T, P] and lnu = log(rng.random((N, T))).  factor is [P, P] (``proposal_factor``), one
    for all chains, or [N, P, P], one per chain."""
    F = np.asarray(factor, dtype=np.float64)
    if F.ndim not in (2, 3) or F.shape[-1] != F.shape[-2] or (F.ndim == 3 and F.shape[0] != N):
        raise ValueError(f"factor must be [P, P] or [{N}, P, P]")
    P = F.shape[-1]
    z = rng.standard_normal((N, T, P))
    step = np.einsum("ntq,pq->ntp", z, F) if F.ndim == 2 else np.einsum("ntq,npq->ntp", z, F)
    with np.errstate(divide="ignore"):
        lnu = np.log(rng.random((N, T)))
    return np.ascontiguousarray(step), lnu


def temper_ladder(R, beta_min):
    """The inverse temperatures of ``MarginalLikelihood.temper_draws_params``: a geometric ladder beta [R] from 1 down to beta_min,
    beta[r] = beta_min^(r / (R - 1)) (R = 1: [1]), with 0 < beta_min < 1 for R > 1."""
    if R != int(R) or R < 1:
        raise ValueError("R must be an integer >= 1")
    R = int(R)
    if R == 1:
        return np.ones(1)
    if not 0.0 < beta_min < 1.0:
        raise ValueError("beta_min must lie in (0, 1): a geometric ladder does not reach 0")
    beta = float(beta_min) ** (np.arange(R) / (R - 1))
    beta[0], beta[-1] = 1.0, float(beta_min)
    return beta


def temper_proposals(rng, nlad, beta, T, factor, swap_every, first_step=0, widen=None):
    """The randomness of ``MarginalLikelihood.temper_draws_params`` from a ``numpy.random.Generator``: -> (step [nlad R, T, P], lnu [nlad R, T],
    lnu_swap [nlad, nsw, R - 1]) with nsw = (first_step + T) // swap_every - first_step // swap_every (swap_every = 0: nsw = 0).  step and lnu are
    ``metropolis_proposals`` for the nlad R chains (factor [P, P] or [nlad R, P, P]), the increments of rung r multiplied by widen[r]; the
    default 1 / sqrt(beta[r]) keeps the acceptance of a Gaussian target level along the ladder and needs every beta > 0 (ValueError otherwise)."""
    beta = np.asarray(beta, dtype=np.float64)
    if beta.ndim != 1 or beta.size < 1:
        raise ValueError("beta must be [R]")
    R = beta.size
    for name, v, lo in (("nlad", nlad, 0), ("T", T, 1), ("swap_every", swap_every, 0), ("first_step", first_step, 0)):
        if v != int(v) or v < lo:
            raise ValueError(f"{name} must be an integer >= {lo}")
    nlad, T, S, first = int(nlad), int(T), int(swap_every), int(first_step)
    if widen is None:
        if np.any(beta <= 0.0):
            raise ValueError("a rung at beta = 0 has no default widening 1 / sqrt(beta): pass widen [R]")
        widen = 1.0 / np.sqrt(beta)
    widen = np.asarray(widen, dtype=np.float64)
    if widen.shape != (R,):
        raise ValueError(f"widen must be [{R}], one factor per rung")
    step, lnu = metropolis_proposals(rng, nlad * R, T, factor)
    step = step * np.tile(widen, nlad)[:, None, None]
    nsw = (first + T) // S - first // S if S else 0
    with np.errstate(divide="ignore"):
        lnu_swap = np.log(rng.random((nlad, nsw, max(R - 1, 0))))
    return np.ascontiguousarray(step), lnu, lnu_swap


def stretch_proposals(rng, nens, K, T, P, a=2.0):
    """The randomness of ``MarginalLikelihood.ensemble_draws_params`` from a ``numpy.random.Generator``: -> (z [nens K, T], pick [nens K, T]
    (int32), lnq [nens K, T]).  z = ((a - 1) u + 1)^2 / a with u uniform has the density g(z) ~ 1 / sqrt(z) on [1 / a, a] of Goodman &
    Weare's stretch move, pick = rng.integers(K / 2) is the partner in the other half, and lnq = ln u' - (P - 1) ln z carries the move's
    Jacobian z^(P - 1) to the uniform's side.  a > 1 (ValueError otherwise); 2 is emcee's default."""
    for name, v, lo in (("nens", nens, 0), ("K", K, 2), ("T", T, 1), ("P", P, 1)):
        if v != int(v) or v < lo:
            raise ValueError(f"{name} must be an integer >= {lo}")
    nens, K, T, P = int(nens), int(K), int(T), int(P)
    if K % 2:
        raise ValueError("K must be even: an ensemble moves half against half")
    if not a > 1.0:
        raise ValueError("a must be > 1: the stretch factors lie in [1 / a, a]")
    N = nens * K
    z = ((a - 1.0) * rng.random((N, T)) + 1.0) ** 2 / a
    pick = rng.integers(K // 2, size=(N, T)).astype(np.int32)
    with np.errstate(divide="ignore"):
        lnq = np.log(rng.random((N, T))) - (P - 1) * np.log(z)
    return z, pick, lnq


def hmc_momenta(rng, N, T, P):
    """The randomness of ``MarginalLikelihood.hmc_draws_params`` from a ``numpy.random.Generator``: -> (momentum [N, T, P], lnu [N, T]) with
    momentum = rng.standard_normal((N, T, P)) and lnu = log(rng.random((N, T)))."""
    for name, v in (("N", N), ("T", T), ("P", P)):
        if v != int(v) or v < (0 if name == "N" else 1):
            raise ValueError(f"{name} must be an integer >= {0 if name == 'N' else 1}")
    mom = rng.standard_normal((int(N), int(T), int(P)))
    with np.errstate(divide="ignore"):
        lnu = np.log(rng.random((int(N), int(T))))
    return mom, lnu


def drag_fractions(T):
    """The schedule of a dragging step of T fast steps (cobaya's ``drag: true``; Neal 2005): the weight of the end point at fast step
    t = 1 ... T is t / (T + 1) -> frac [T].  The default of ``drag_draws_params``."""
    if T != int(T) or T < 1:
        raise ValueError("T must be an integer >= 1")
    return np.arange(1, int(T) + 1) / (int(T) + 1)


def drag_accept(lnu_slow, result):
    """The decision on the whole slow + fast move of every chain of a ``DragChains``: lnu_slow [N], the logarithms of the caller's uniforms
    -> accepted [N] = lnu_slow < result.log_ratio.  An accepted chain goes on from (end walker, result.last), a rejected one returns to
    (start walker, its theta0).  The ratio is that of ln pi alone: a prior on the slow parameters and an asymmetric slow proposal are the
    caller's to add to lnu_slow's side."""
    lnu_slow = np.asarray(lnu_slow, dtype=np.float64)
    if lnu_slow.shape != np.shape(result.log_ratio):
        raise ValueError(f"lnu_slow must be {list(np.shape(result.log_ratio))}: the logarithm of a uniform per chain")
    return lnu_slow < result.log_ratio


__all__ = ["MarginalLikelihood", "DrawChains", "DrawTrajectories", "TemperedChains", "temper_ladder", "temper_proposals", "stretch_proposals", "hmc_momenta", "DragChains", "drag_fractions", "drag_accept", "metropolis_proposals", "proposal_factor", "data_index", "newton_maximize", "gaussian_params", "gaussian_rows", "gaussian_rows_many", "joint_draw_recipe", "joint_gaussian_rows", "joint_gaussian_rows_many"]
