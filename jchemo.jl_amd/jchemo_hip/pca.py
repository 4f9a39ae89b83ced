"""PCA and principal component regression — host-side mirror of the reference's src/pcasvd.jl, src/pcaeigen.jl and src/pcr.jl over
jch_pca_fit, jch_transform and jch_predict (include/jchemo_hip.h).

numpy in gives numpy out; a device torch tensor in leaves what is n-sized (`T`, `weights`, `contr_ind`, the predictions) on the device.
The p- and nlv-sized results are host arrays either way.

Deviations from the reference: `pcasvd`, `pcaeigen` and `pcaeigenk` run one algorithm (the leading eigenpairs of
Xc'D Xc by block subspace iteration: the same T, P and sv up to rounding); `sv` and `eig` hold the nlv leading values, not min(n, p);
`summary` is computed from the stored quantities and does not read X; the `!` forms do not leave a centred X behind.  The iteration needs a
gap in the spectrum behind the block: on pure-noise data it stops at `eig_maxit` with `converged = False` and a warning."""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .plsr import _addr_ld, _as_colmajor_copy, _is_torch, _model_vec, _np, _x_out, colmajor_empty, ensure_mat

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


@dataclass
class Pca:
    """The reference's `Pca` (src/pcasvd.jl:100: T, P, sv, xmeans, xscales, weights, niter, conv), then what the eigen route knows: eig = sv^2,
    sstot = trace(Xs'D Xs), colvar = the weighted variances of the columns of X (before scaling), resid = the residual norms
    |G p_i - eig_i p_i| and converged.  T (n x nlv) and weights (n, normalised) live where X lives; niter counts the subspace iterations and
    conv repeats converged (the reference stores `nothing` in both for the SVD route)."""
    T: object
    P: np.ndarray
    sv: np.ndarray
    xmeans: np.ndarray
    xscales: np.ndarray
    weights: object
    niter: int
    conv: bool
    eig: np.ndarray
    sstot: float
    colvar: np.ndarray
    resid: np.ndarray
    converged: bool


@dataclass
class Pcr:
    """The reference's `Pcr` (src/pcr.jl:96): fm_pca, T, R = P, C = beta', xmeans, xscales, ymeans, yscales (ones), weights.  R and C have the
    shapes of a `Plsr`, so `transform`, `coef` and `predict` take it through the same code."""
    fm_pca: Pca
    T: object
    R: np.ndarray
    C: np.ndarray
    xmeans: np.ndarray
    xscales: np.ndarray
    ymeans: np.ndarray
    yscales: np.ndarray
    weights: object

    @property
    def P(self):
        return self.R


def _weights_arg(weights, n, dev, device):
    if weights is None:
        return None, None
    if dev:
        w = (weights if _is_torch(weights) else torch.as_tensor(np.asarray(weights, dtype=np.float64), device=device)).to(torch.float64).reshape(-1).contiguous()
        addr = w.data_ptr()
    else:
        w = np.ascontiguousarray(np.asarray(weights.cpu() if _is_torch(weights) else weights, dtype=np.float64).reshape(-1))
        addr = w.ctypes.data
    if w.shape[0] != n:
        raise ValueError(f"DimensionMismatch: weights has {w.shape[0]} entries, X has {n} rows")
    return w, addr


def _colmajor(A):
    A = ensure_mat(A)
    if not _is_torch(A):
        A = np.asarray(A)
    try:
        _addr_ld(A)
    except (ValueError, TypeError):
        A = _as_colmajor_copy(A)
    return A


def _fit(who, X, Y, weights, nlv, scal, eig_tol, eig_maxit, ctx):
    if isinstance(nlv, bool) or int(nlv) != nlv or int(nlv) < 1:
        raise ValueError(f"nlv = {nlv} must be an integer >= 1")
    if int(eig_maxit) < 1:
        raise ValueError(f"eig_maxit = {eig_maxit} must be >= 1")
    if not float(eig_tol) > 0.0:
        raise ValueError(f"eig_tol = {eig_tol} must be > 0")
    X = _colmajor(X)
    dev = _is_torch(X)
    if dev and not X.is_cuda:
        raise TypeError("torch inputs must live on the GPU (host data: pass numpy arrays)")
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be a matrix with at least one row and one column")
    n, p = X.shape
    q = 0
    if Y is not None:
        if _is_torch(Y) != dev:
            raise TypeError("X and Y must both be host arrays or both device tensors")
        Y = _colmajor(Y)
        if Y.shape[0] != n:
            raise ValueError(f"DimensionMismatch: X has {n} rows, Y has {Y.shape[0]}")
        q = Y.shape[1]
    w_arr, w_addr = _weights_arg(weights, n, dev, X.device if dev else None)
    ctx = ctx or default_context((X.device.index or 0) if dev else 0)
    a = min(int(nlv), n, p)                                                  # src/pcasvd.jl:82
    if dev:
        T = colmajor_empty(n, a, X.device)
        wn = torch.empty(n, dtype=torch.float64, device=X.device)
        ta, wa = T.data_ptr(), wn.data_ptr()
        torch.cuda.current_stream(X.device).synchronize()
    else:
        T = np.empty((n, a), order="F")
        wn = np.empty(n)
        ta, wa = T.ctypes.data, wn.ctypes.data
    P = np.empty((p, a), order="F")
    sv, eig, res = np.empty(a), np.empty(a), np.empty(a)
    xm, xs, cvar = np.empty(p), np.empty(p), np.empty(p)
    ym, K = np.empty(q), np.empty((p, q), order="F")
    sst = C.c_double(0.0); nit = C.c_int32(0); got = C.c_int32(0); cvg = C.c_int32(0)
    xa, ldx = _addr_ld(X)
    ya, ldy = _addr_ld(Y) if q else (None, 0)
    ctx.check(_lib.load().jch_pca_fit(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, xa, n, p, ldx, w_addr, ya, q, ldy, int(nlv), int(bool(scal)),
                                      float(eig_tol), int(eig_maxit), ta, P.ctypes.data, sv.ctypes.data, eig.ctypes.data, xm.ctypes.data, xs.ctypes.data, wa,
                                      C.addressof(sst), cvar.ctypes.data, _np(ym) if q else None, K.ctypes.data if q else None, C.byref(nit), res.ctypes.data,
                                      C.byref(got), C.byref(cvg)))
    conv = bool(cvg.value)                                                   # decided by the iteration itself
    if not conv:
        warnings.warn(f"{who}: the subspace iteration did not converge in {nit.value} iterations (max residual {float(res.max()):.3g}, "
                      f"tolerance {float(eig_tol) * eig[0]:.3g})", RuntimeWarning, stacklevel=3)
    fm = Pca(T, P, sv, xm, xs, wn, int(nit.value), conv, eig, float(sst.value), cvar, res, conv)
    return fm, ym, K


def pcasvd(X, weights=None, *, nlv, scal: bool = False, eig_tol: float = 1e-10, eig_maxit: int = 300, ctx: Optional[Context] = None) -> Pca:
    """`pcasvd(X, weights; nlv, scal = false)` — src/pcasvd.jl:73-101 through jch_pca_fit.  X is only read.  eig_tol / eig_maxit control the
    subspace iteration; a fit that did not converge warns and returns what it has."""
    return _fit("pcasvd", X, None, weights, nlv, scal, eig_tol, eig_maxit, ctx)[0]


def pcaeigen(X, weights=None, *, nlv, scal: bool = False, eig_tol: float = 1e-10, eig_maxit: int = 300, ctx: Optional[Context] = None) -> Pca:
    """`pcaeigen(X, weights; nlv, scal = false)` — src/pcaeigen.jl: the eigen-decomposition of X'DX, which is what every fit here runs."""
    return _fit("pcaeigen", X, None, weights, nlv, scal, eig_tol, eig_maxit, ctx)[0]


def pcaeigenk(X, weights=None, *, nlv, scal: bool = False, eig_tol: float = 1e-10, eig_maxit: int = 300, ctx: Optional[Context] = None) -> Pca:
    """`pcaeigenk(X, weights; nlv, scal = false)` — src/pcaeigenk.jl (the n x n route for n < p): the same T, P and sv; here the p x p Gram costs
    2 n p^2 flops at such shapes, so the one algorithm serves."""
    return _fit("pcaeigenk", X, None, weights, nlv, scal, eig_tol, eig_maxit, ctx)[0]


# The reference's `!` forms centre (and scale) X in place as a side effect of the SVD.  The fit here never writes X: the `!` names are aliases.
pcasvd_, pcaeigen_, pcaeigenk_ = pcasvd, pcaeigen, pcaeigenk


def pca_transform(fm: Pca, X, *, nlv: Optional[int] = None, ctx: Optional[Context] = None):
    """`transform(object::Pca, X; nlv)` — src/pcasvd.jl:110-115: cscale(X, xmeans, xscales) * P[:, 1:nlv] through jch_transform with R = P."""
    a = fm.P.shape[1]
    k = a if nlv is None else min(int(nlv), a)
    if k < 1:
        raise ValueError("transform needs nlv >= 1")
    X, out, oa, ctx, loc = _x_out(X, k, ctx)
    m, p = X.shape
    if fm.P.shape[0] != p:
        raise ValueError(f"DimensionMismatch: X has {p} columns, the model has {fm.P.shape[0]}")
    R = np.asfortranarray(fm.P[:, :k], dtype=np.float64)
    xm, xs = _model_vec(fm.xmeans), _model_vec(fm.xscales)
    xa, ldx = _addr_ld(X)
    ctx.check(_lib.load().jch_transform(ctx._h, loc, xa, m, p, ldx, _np(xm), _np(xs), R.ctypes.data, k, oa, max(m, 1)))
    return out


def pca_summary(fm: Pca, X):
    """`summary(object::Pca, X)` — src/pcasvd.jl:123-146 from the stored quantities; X is only checked for its shape.  With G = Xs'D Xs,
    G P = P diag(eig): sstot = trace(G) (:128); tt = eig (:130-133); coord_var = Xs'D T / sqrt(tt) = P diag(sv) (:140); cor_circle =
    coord_var ./ colstd(Xs) (:139; colstd(Xs) = sqrt(colvar) / xscales); contr_var = coord_var.^2 scaled by its column sums (:142-144);
    contr_ind = D T.^2 ./ tt (:129, :138), which stays where T lives.  explvarx is a dict of columns (lv, var, pvar, cumpvar)."""
    X = ensure_mat(X)
    n, p = fm.T.shape[0], fm.P.shape[0]
    if tuple(X.shape) != (n, p):
        raise ValueError(f"DimensionMismatch: X is {X.shape[0]} x {X.shape[1]}, the model was fitted on {n} x {p}")
    a = fm.P.shape[1]
    tt = fm.eig[:a]
    pvar = tt / fm.sstot
    explvarx = dict(lv=np.arange(1, a + 1), var=tt, pvar=pvar, cumpvar=np.cumsum(pvar))
    if _is_torch(fm.T):
        w = fm.weights if _is_torch(fm.weights) else torch.as_tensor(np.asarray(fm.weights), device=fm.T.device)
        contr_ind = w[:, None] * fm.T ** 2 / torch.as_tensor(tt, device=fm.T.device)[None, :]
    else:
        contr_ind = np.asarray(fm.weights)[:, None] * fm.T ** 2 / tt[None, :]
    coord_var = fm.P * fm.sv[None, :a]
    cor_circle = coord_var / (np.sqrt(fm.colvar) / fm.xscales)[:, None]
    cc = coord_var ** 2
    contr_var = cc / cc.sum(axis=0, keepdims=True)
    return dict(explvarx=explvarx, contr_ind=contr_ind, contr_var=contr_var, coord_var=coord_var, cor_circle=cor_circle)


def pcr(X, Y, weights=None, *, nlv, scal: bool = False, eig_tol: float = 1e-10, eig_maxit: int = 300, ctx: Optional[Context] = None) -> Pcr:
    """`pcr(X, Y, weights; nlv, scal = false)` — src/pcr.jl:76-97: the PCA fit plus one pass Xs'D Yc over X; beta = diag(1 / sv^2) P' Xs'D Yc
    (:93-94: T is D-orthogonal and T'D Y = T'D Yc because T is centred), nlv x q host work.  `coef` and `predict` (a single nlv or a range,
    0 = intercept only) are the `Plsr` ones."""
    if Y is None:
        raise ValueError("pcr needs Y")
    fm, ym, K = _fit("pcr", X, Y, weights, nlv, scal, eig_tol, eig_maxit, ctx)
    beta = (fm.P.T @ K) / fm.eig[:, None]
    return Pcr(fm, fm.T, fm.P, np.asfortranarray(beta.T), fm.xmeans, fm.xscales, ym, np.ones(ym.shape[0]), fm.weights)


pcr_ = pcr   # `pcr!` (src/pcr.jl:82): X and Y are not written here
