"""Gaussian discrimination on raw X — host-side mirror of the reference's src/dmnorm.jl, src/lda.jl, src/qda.jl, src/matW.jl and `mahsqchol` of
src/distances.jl over jch_class_cov, jch_gauss_factor and jch_mahsq_chol (include/jchemo_hip.h).

numpy in gives numpy out; a device torch tensor in keeps the matrices (W, Wi, Uinv, dens, posterior, distances) on the device.  Class labels,
class means, priors and determinants are host arrays, as everywhere else.

The densities are the reference's plain products (2 pi)^(-p/2) / sqrt(detS) * exp(-d / 2): beyond roughly p = 130 they leave the float64 range for
all but well-conditioned data, and the reference then gives densities of 0, a NaN posterior and the first level; so does this mirror.  The
distances (`mahsqchol`, `mahsq_chol`) have no such limit."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context
from .kde import _colmajor, _ctx_for, _group_by_class, _labels, _posterior, _wprior
from .plsr import _addr_ld, _is_torch, ensure_mat

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


@dataclass
class Dmnorm:
    """src/dmnorm.jl:1-5 — same fields: mu (p, host), Uinv (p x p upper triangular, where the data lives), detS."""
    mu: np.ndarray
    Uinv: object
    detS: float


@dataclass
class Lda:
    """src/lda.jl:1-8 — same fields: fm (one Dmnorm per level, all sharing ONE Uinv object), W, ct, wprior, lev, ni."""
    fm: list
    W: object
    ct: np.ndarray
    wprior: np.ndarray
    lev: np.ndarray
    ni: np.ndarray


@dataclass
class Qda:
    """src/qda.jl:1-8 — same fields: fm (one Dmnorm per level), Wi ((nlev, p, p)), ct, wprior, lev, ni."""
    fm: list
    Wi: object
    ct: np.ndarray
    wprior: np.ndarray
    lev: np.ndarray
    ni: np.ndarray


# ---------------------------------------------------------------------------------- the three primitives
def _loc(dev):
    return _lib.LOC_DEVICE if dev else _lib.LOC_HOST


def _stack_empty(k, p, like):
    """(k, p, p) float64 storage where `like` lives; slice f is the p x p matrix f at stride p * p."""
    if _is_torch(like):
        return torch.empty((k, p, p), dtype=torch.float64, device=like.device)
    return np.empty((k, p, p), dtype=np.float64)


def _ptr(a):
    return a.data_ptr() if _is_torch(a) else a.ctypes.data


def _sync_torch(a):
    if _is_torch(a):
        torch.cuda.current_stream(a.device).synchronize()


def class_cov(Z, cls_start, *, want_Wi: bool = True, want_W: bool = True, ctx: Optional[Context] = None):
    """jch_class_cov on the rows of Z grouped by class (class c in rows cls_start[c] .. cls_start[c + 1] - 1): (Wi, W, ct).  Wi (ncls, p, p) and
    W (p, p) live where Z does (None when not wanted; every matrix is bitwise symmetric), ct (ncls, p) is a host array.  Wi[c] is the uncorrected
    covariance of class c — of ALL rows for a class of one row (src/matW.jl:54-65) — and W = sum_c n_c / n Wi[c]."""
    Z = _colmajor(Z)
    n, p = Z.shape
    cs = np.ascontiguousarray(cls_start, dtype=np.int64).reshape(-1)
    ncls = cs.shape[0] - 1
    Wi = _stack_empty(ncls, p, Z) if want_Wi else None
    W = _stack_empty(1, p, Z)[0] if want_W else None
    ct = np.empty((ncls, p), dtype=np.float64, order="F")
    ctx = _ctx_for(Z, ctx)
    _sync_torch(Z)
    za, ldz = _addr_ld(Z)
    ctx.check(_lib.load().jch_class_cov(ctx._h, _loc(_is_torch(Z)), za, n, p, ldz, cs.ctypes.data, ncls, _ptr(Wi) if want_Wi else None,
                                        _ptr(W) if want_W else None, ct.ctypes.data))
    return Wi, W, ct


def gauss_factor(S, *, ctx: Optional[Context] = None):
    """jch_gauss_factor: S (p, p) or (nfac, p, p), symmetric (one triangle is read), host array or device tensor -> (Uinv, diagU, info).  Uinv has
    S's shape and lives where S does: Uinv[f] = L_f^-T, upper triangular with exact zeros below the diagonal, column-major; diagU (p, nfac) and
    info (nfac) are host arrays; info[f] != 0 (the 1-based column of the first pivot that is not > 0) marks a factor that failed."""
    single = S.dim() == 2 if _is_torch(S) else np.ndim(S) == 2
    if _is_torch(S):
        S3 = (S[None] if single else S).to(torch.float64).contiguous()
    else:
        S3 = np.ascontiguousarray(S[None] if single else S, dtype=np.float64)
    if S3.ndim != 3 or S3.shape[1] != S3.shape[2]:
        raise ValueError(f"gauss_factor: S must be (p, p) or (nfac, p, p), got {tuple(S3.shape)}")
    nfac, p = S3.shape[0], S3.shape[1]
    store = _stack_empty(nfac, p, S3)
    diagU = np.empty((p, nfac), dtype=np.float64, order="F")
    info = np.zeros(nfac, dtype=np.int32)
    ctx = _ctx_for(S3, ctx)
    _sync_torch(S3)
    ctx.check(_lib.load().jch_gauss_factor(ctx._h, _loc(_is_torch(S3)), _ptr(S3), p, p, p * p, nfac, _ptr(store), p, p * p, diagU.ctypes.data,
                                           info.ctypes.data))
    Uinv = store.transpose(1, 2) if _is_torch(store) else store.transpose(0, 2, 1)   # slice f column-major in the storage
    return (Uinv[0] if single else Uinv), diagU, info


def _factor_layout(Uinv, p):
    """(array to keep alive, address, ldu, ustride, nfac) of one column-major p x p factor or of a (nfac, p, p) stack as gauss_factor returns it."""
    nd = Uinv.dim() if _is_torch(Uinv) else np.ndim(Uinv)
    if nd == 3:
        nfac = Uinv.shape[0]
        T = Uinv.transpose(1, 2) if _is_torch(Uinv) else np.transpose(Uinv, (0, 2, 1))
        ok = T.is_contiguous() and T.dtype == torch.float64 if _is_torch(T) else (T.flags.c_contiguous and T.dtype == np.float64)
        if not ok:
            T = T.to(torch.float64).contiguous() if _is_torch(T) else np.ascontiguousarray(T, dtype=np.float64)
        if tuple(T.shape[1:]) != (p, p):
            raise ValueError(f"DimensionMismatch: Uinv is {tuple(Uinv.shape)}, the data has {p} columns")
        return T, _ptr(T), p, p * p, nfac
    U = _colmajor(Uinv)
    if tuple(U.shape) != (p, p):
        raise ValueError(f"DimensionMismatch: Uinv is {tuple(U.shape)}, the data has {p} columns")
    ua, ldu = _addr_ld(U)
    return U, ua, ldu, p * p, 1


def mahsq_chol(Xq, Mu, Uinv, *, ctx: Optional[Context] = None):
    """jch_mahsq_chol: out[i, c] = |(Xq[i, :] - Mu[c, :]) Uinv_f|^2, f = 0 for one factor (Uinv p x p) or c for one per centre (Uinv (ncen, p, p)).
    Xq (m x p) and Uinv both host arrays or both device tensors; Mu (ncen x p) is taken to the host; out (m x ncen) lives where Xq does.  The
    difference is taken before the product; the strictly lower triangle of Uinv is never read."""
    Xq = _colmajor(Xq)
    m, p = Xq.shape
    dev = _is_torch(Xq)
    if dev != _is_torch(Uinv):
        raise TypeError("Xq and Uinv must both be host arrays or both device tensors")
    Mu = np.asfortranarray(ensure_mat(np.asarray(Mu.cpu() if _is_torch(Mu) else Mu, dtype=np.float64)))
    if Mu.shape[1] != p:
        raise ValueError(f"DimensionMismatch: Xq has {p} columns, Mu has {Mu.shape[1]}")
    ncen = Mu.shape[0]
    keep, ua, ldu, ustride, nfac = _factor_layout(Uinv, p)
    if nfac != 1 and nfac != ncen:
        raise ValueError(f"mahsq_chol: {nfac} factors for {ncen} centres (one, or one per centre)")
    if dev:
        out = torch.empty((ncen, m), dtype=torch.float64, device=Xq.device).t()
    else:
        out = np.empty((m, ncen), dtype=np.float64, order="F")
    ctx = _ctx_for(Xq, ctx)
    _sync_torch(Xq)
    qa, ldq = _addr_ld(Xq)
    ctx.check(_lib.load().jch_mahsq_chol(ctx._h, _loc(dev), qa, m, p, ldq, Mu.ctypes.data, ncen, ua, ldu, ustride, nfac, _ptr(out), max(m, 1)))
    return out


# ---------------------------------------------------------------------------------- dmnorm
def _posdef(info, what):
    j = int(info)
    if j != 0:
        raise ValueError(f"PosDefException: {what}: matrix is not positive definite; Cholesky factorization failed at column {j}")


def _det_s(diag):
    """det(U)^2 with det(U) the product of the diagonal in order; 0 -> 1e-20 (src/dmnorm.jl:121-122)."""
    d = 1.0
    for v in diag:
        d *= float(v)
    detS = d ** 2
    return 1e-20 if detS == 0 else detS


def dmnorm(X=None, *, mu=None, S=None, ctx: Optional[Context] = None) -> Dmnorm:
    """`dmnorm(X = nothing; mu = nothing, S = nothing)` — src/dmnorm.jl:107-128.  mu defaults to the column means of X, S to `cov(X)` (corrected):
    one jch_class_cov call with one class.  The factor and its inverse come from jch_gauss_factor; a matrix that is not positive definite (one row
    of X among them) raises ValueError("PosDefException: ...") as the reference's `cholesky!` throws."""
    if X is None and (mu is None or S is None):
        raise ValueError("dmnorm: give X, or both mu and S")
    if X is not None and (mu is None or S is None):
        X = ensure_mat(X)
        n = X.shape[0]
        Wi, _, ct = class_cov(X, [0, n], want_Wi=S is None, want_W=False, ctx=ctx)
        if mu is None:
            mu = ct[0]
        if S is None:
            S = Wi[0] * (n / (n - 1) if n > 1 else math.nan)
    mu = np.array(mu.cpu() if _is_torch(mu) else mu, dtype=np.float64).reshape(-1)
    S = ensure_mat(S)
    if S.shape[0] != S.shape[1] or S.shape[0] != mu.shape[0]:
        raise ValueError(f"DimensionMismatch: mu has {mu.shape[0]} entries, S is {tuple(S.shape)}")
    Uinv, diagU, info = gauss_factor(S, ctx=ctx)
    _posdef(info[0], "dmnorm")
    return Dmnorm(mu, Uinv, _det_s(diagU[:, 0]))


def _coef(p, detS):
    """(2 * pi)^(-p / 2) * (1 / sqrt(detS)), in the reference's order (src/dmnorm.jl:141)."""
    return (2 * math.pi) ** (-p / 2) * (1 / math.sqrt(detS))


def _exp_half(d):
    return torch.exp(-.5 * d) if _is_torch(d) else np.exp(-.5 * d)


def dmnorm_predict(obj: Dmnorm, X, *, ctx: Optional[Context] = None):
    """`predict(object::Dmnorm, X)` — src/dmnorm.jl:136-143: pred (m x 1) where X lives, one jch_mahsq_chol call."""
    X = ensure_mat(X)
    p = X.shape[1]
    if p != obj.mu.shape[0]:
        raise ValueError(f"DimensionMismatch: X has {p} columns, the model has {obj.mu.shape[0]}")
    d = mahsq_chol(X, obj.mu.reshape(1, -1), obj.Uinv, ctx=ctx)
    return _coef(p, obj.detS) * _exp_half(d)


# ---------------------------------------------------------------------------------- lda, qda
def _da_prepare(X, y, prior):
    """What `lda`, `qda`, `matW` and `matB` share ahead of any device work: the checks of y and prior; labels, levels, counts, class offsets."""
    yv = _labels(y)
    n = X.shape[0]
    if yv.shape[0] != n:
        raise ValueError(f"DimensionMismatch: X has {n} rows, y has {yv.shape[0]}")
    lev, ni = np.unique(yv, return_counts=True)
    wprior = _wprior(prior, ni)
    return yv, lev, ni, wprior, np.concatenate([[0], np.cumsum(ni)]).astype(np.int64)


def lda(X, y, *, prior: str = "unif", ctx: Optional[Context] = None) -> Lda:
    """`lda(X, y; prior = "unif")` — src/lda.jl:56-77: W of `matW` times n / (n - nlev), ONE factor, and nlev Dmnorm records that share its Uinv."""
    X = ensure_mat(X)
    n = X.shape[0]
    yv, lev, ni, wprior, cs = _da_prepare(X, y, prior)
    nlev = len(lev)
    _, W, ct = class_cov(_group_by_class(X, yv, lev), cs, want_Wi=False, ctx=ctx)
    W = W * (n / (n - nlev) if n > nlev else math.inf)              # unbiased estimate (:65; Julia's n / 0 is Inf)
    Uinv, diagU, info = gauss_factor(W, ctx=ctx)
    _posdef(info[0], f"lda: the pooled W of {n} rows in {nlev} classes")
    detS = _det_s(diagU[:, 0])
    return Lda([Dmnorm(np.array(ct[i]), Uinv, detS) for i in range(nlev)], W, ct, wprior, lev, ni)


def qda(X, y, *, prior: str = "unif", ctx: Optional[Context] = None) -> Qda:
    """`qda(X, y; prior = "unif")` — src/qda.jl:55-79: S_i = Wi[i] n_i / (n_i - 1) (Wi[i] itself for a class of one row), nlev factors in one
    jch_gauss_factor call."""
    X = ensure_mat(X)
    yv, lev, ni, wprior, cs = _da_prepare(X, y, prior)
    nlev = len(lev)
    Wi, _, ct = class_cov(_group_by_class(X, yv, lev), cs, want_W=False, ctx=ctx)
    f = np.array([1.0 if k == 1 else k / (k - 1) for k in ni])
    S = Wi * (torch.as_tensor(f, device=Wi.device) if _is_torch(Wi) else f)[:, None, None]
    Uinv, diagU, info = gauss_factor(S, ctx=ctx)
    for i in range(nlev):
        _posdef(info[i], f"qda: class {np.asarray(lev[i]).item()!r} ({int(ni[i])} rows)")
    obj = Qda([Dmnorm(np.array(ct[i]), Uinv[i], _det_s(diagU[:, i])) for i in range(nlev)], Wi, ct, wprior, lev, ni)
    obj._Uinv = Uinv                                           # the stack the records' Uinv are views of
    return obj


def _da_predict(obj, X, ctx):
    X = ensure_mat(X)
    p = X.shape[1]
    if p != obj.ct.shape[1]:
        raise ValueError(f"DimensionMismatch: X has {p} columns, the model has {obj.ct.shape[1]}")
    fm = obj.fm
    if all(f.Uinv is fm[0].Uinv for f in fm):
        U = fm[0].Uinv                                         # one shared factor: nfac = 1
    else:
        U = getattr(obj, "_Uinv", None)
        if U is None:                                          # a record put together by hand
            U = torch.stack([f.Uinv for f in fm]) if _is_torch(fm[0].Uinv) else np.stack([f.Uinv for f in fm])
    d = mahsq_chol(X, np.stack([f.mu for f in fm]), U, ctx=ctx)
    coef = np.array([_coef(p, f.detS) for f in fm])
    dens = (torch.as_tensor(coef, device=d.device) if _is_torch(d) else coef)[None, :] * _exp_half(d)
    post, z = _posterior(np.asarray(obj.wprior, dtype=np.float64), dens)
    return np.asarray(obj.lev)[z].reshape(-1, 1), dens, post


def lda_predict(obj: Lda, X, *, ctx: Optional[Context] = None):
    """`predict(object::Lda, X)` — src/lda.jl:85-101: (pred, dens, posterior); pred m x 1 host labels, dens and posterior m x nlev where X lives.
    One jch_mahsq_chol call for all classes, with nfac = 1: the records share one Uinv."""
    return _da_predict(obj, X, ctx)


def qda_predict(obj: Qda, X, *, ctx: Optional[Context] = None):
    """`predict(object::Qda, X)` — src/qda.jl:87-104: as `lda_predict`, one factor per class."""
    return _da_predict(obj, X, ctx)


# ---------------------------------------------------------------------------------- matW, matB, mahsqchol
def matW(X, y, *, ctx: Optional[Context] = None):
    """`matW(X, y)` — src/matW.jl:44-75: (W, Wi, lev, ni); Wi (nlev, p, p) and W where X lives."""
    X = ensure_mat(X)
    yv, lev, ni, _, cs = _da_prepare(X, y, "unif")
    Wi, W, _ = class_cov(_group_by_class(X, yv, lev), cs, ctx=ctx)
    return W, Wi, lev, ni


def matB(X, y, *, ctx: Optional[Context] = None):
    """`matB(X, y)` — src/matW.jl:23-29: (B, ct, lev, ni); the class centres come from the device (jch_class_cov without a covariance), B, the
    weighted covariance of the nlev centres (`covm(ct, mweight(ni))`, src/utility.jl:439-446), is host work."""
    X = ensure_mat(X)
    yv, lev, ni, _, cs = _da_prepare(X, y, "unif")
    _, _, ct = class_cov(_group_by_class(X, yv, lev), cs, want_Wi=False, want_W=False, ctx=ctx)
    w = ni / ni.sum()
    z = np.sqrt(w)[:, None] * (ct - w @ ct)
    return z.T @ z, ct, lev, ni


def mahsqchol(X, Y, Uinv=None, *, ctx: Optional[Context] = None):
    """`mahsqchol(X, Y[, Uinv])` — src/distances.jl:104-126: the squared Mahalanobis distances between the rows of X (n x p) and of Y (k x p, the
    centres: k small), n x k where X lives.  Without Uinv: from the uncorrected covariance of X, factored on the device.  The difference x - y is
    taken before the product with Uinv (the reference multiplies first and expands the square)."""
    X, Y = ensure_mat(X), ensure_mat(Y)
    if X.shape[1] != Y.shape[1]:
        raise ValueError(f"DimensionMismatch: X has {X.shape[1]} columns, Y has {Y.shape[1]}")
    if Uinv is None:
        Wi, _, _ = class_cov(X, [0, X.shape[0]], want_W=False, ctx=ctx)
        Uinv, _, info = gauss_factor(Wi[0], ctx=ctx)
        _posdef(info[0], "mahsqchol")
    else:
        Uinv = ensure_mat(Uinv)
    return mahsq_chol(X, Y, Uinv, ctx=ctx)
