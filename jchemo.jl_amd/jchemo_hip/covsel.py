"""Covsel variable selection and the MLR on the selected variables — host-side mirror of the reference's src/covsel.jl and
src/covselr.jl over jch_covsel_fit and jch_affine_gemm (include/jchemo_hip.h).

numpy in gives numpy out; device torch tensors in leave what is n-sized (`Q`, the predictions, the deflated X and Y of `covsel_`) on the
device.  The p- and nlv-sized results are host arrays either way.  `sel` is 0-based here (the Julia mirror gives 1-based indices).

Deviations from the reference: a column whose deflated sum of squares fell to 1e-10 of its original one is exhausted — `cor`
gives it z = 0, and a selection that lands on one stops, so a rank-deficient X returns fewer than `nlv` steps (`nlv` of the record).
`typ = "aic"` (marked "not useful" in the reference) is not provided."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .plsr import _addr_ld, _affine, _as_colmajor_copy, _as_colmajor_view, _is_torch, colmajor_empty, ensure_mat

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

COVSEL_COV, COVSEL_COR = 0, 1   # include/jchemo_hip.h JCH_COVSEL_*
_TYPS = {"cov": COVSEL_COV, "cor": COVSEL_COR}


@dataclass
class Covsel:
    """What the reference's `covsel` returns (src/covsel.jl:119-121): `sel` is the table with the columns sel, cov2, cumpvarx, cumpvary
    (a dict of arrays, one entry per completed step), then `cov2` (p) and `C` (p x nlv).  Beyond the reference: `nlv` = the completed
    steps, xmeans, ymeans, yscales, G = Xc'Q (p x nlv), QtY = Q'Yc (nlv x q, in the units of the scaled Y) and Q (n x nlv, an orthonormal
    basis of the deflated selected columns, where X lives) — what `covselr` is computed from."""
    sel: dict
    cov2: np.ndarray
    C: np.ndarray
    nlv: int
    xmeans: np.ndarray
    ymeans: np.ndarray
    yscales: np.ndarray
    G: np.ndarray
    QtY: np.ndarray
    Q: object


@dataclass
class Mlr:
    """The reference's `Mlr` (src/mlr.jl:1-5): B (p x q) and int (1 x q) in the units of the raw Y, and the normalised weights (None in
    the record `covselr` builds, which never had any)."""
    B: np.ndarray
    int: np.ndarray
    weights: Optional[np.ndarray] = None


@dataclass
class Covselr:
    """The reference's `Covselr` (src/covselr.jl:1-5): fm::Mlr on the selected columns, the `sel` table and cov2."""
    fm: Mlr
    sel: dict
    cov2: np.ndarray


def _check_args(X, Y, nlv, typ):
    """Everything that can be refused before any device work.  Returns (n, p, q, nlv, typ code)."""
    if typ not in _TYPS:
        raise ValueError(f'typ = {typ!r}: "cov" or "cor" ("aic" is marked not useful in the reference and is not provided)')
    if _is_torch(X) != _is_torch(Y):
        raise TypeError("X and Y must both be host arrays or both device tensors")
    if _is_torch(X) and not (X.is_cuda and Y.is_cuda):
        raise TypeError("torch inputs must live on the GPU (host data: pass numpy arrays)")
    if X.ndim != 2 or Y.ndim != 2:
        raise ValueError("X and Y must be matrices (or vectors)")
    n, p = X.shape
    q = Y.shape[1]
    if Y.shape[0] != n:
        raise ValueError(f"DimensionMismatch: X has {n} rows, Y has {Y.shape[0]}")
    if n < 1 or p < 1 or q < 1:
        raise ValueError(f"X is {n} x {p}, Y is {n} x {q}: at least one row and one column each")
    if nlv is None:
        nlv = p                                               # src/covsel.jl:63
    if isinstance(nlv, bool) or int(nlv) != nlv or int(nlv) < 1:
        raise ValueError(f"nlv = {nlv} must be an integer >= 1")
    return n, p, q, min(int(nlv), p), _TYPS[typ]


def _fit(X, Y, nlv, typ, ctx, inplace) -> Covsel:
    X, Y = ensure_mat(X), ensure_mat(Y)
    if not _is_torch(X):
        X = np.asarray(X)
    if not _is_torch(Y):
        Y = np.asarray(Y)
    n, p, q, a, code = _check_args(X, Y, nlv, typ)
    if inplace:
        X, Y = _as_colmajor_view(X), _as_colmajor_view(Y)
    else:
        try:
            _addr_ld(X)
        except (ValueError, TypeError):
            X = _as_colmajor_copy(X)
        try:
            _addr_ld(Y)
        except (ValueError, TypeError):
            Y = _as_colmajor_copy(Y)
    dev = _is_torch(X)
    ctx = ctx or default_context((X.device.index or 0) if dev else 0)
    sel = np.zeros(a, dtype=np.int32)
    selcov, cpx, cpy = np.zeros(a), np.zeros(a), np.zeros(a)
    cov2, xm, ym, ys = np.zeros(p), np.zeros(p), np.zeros(q), np.zeros(q)
    Cm, G, QtY = np.zeros((p, a), order="F"), np.zeros((p, a), order="F"), np.zeros((a, q), order="F")
    if dev:
        Q = colmajor_empty(n, a, X.device)
        qa = Q.data_ptr()
        torch.cuda.current_stream(X.device).synchronize()
    else:
        Q = np.empty((n, a), order="F")
        qa = Q.ctypes.data
    done = C.c_int32(0)
    xa, ldx = _addr_ld(X)
    ya, ldy = _addr_ld(Y)
    ctx.check(_lib.load().jch_covsel_fit(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, xa, n, p, ldx, ya, q, ldy, a, code, int(bool(inplace)),
                                         sel.ctypes.data, selcov.ctypes.data, cov2.ctypes.data, Cm.ctypes.data, cpx.ctypes.data, cpy.ctypes.data,
                                         xm.ctypes.data, ym.ctypes.data, ys.ctypes.data, G.ctypes.data, QtY.ctypes.data, qa, C.byref(done)))
    k = int(done.value)
    tab = dict(sel=sel[:k].astype(np.int64), cov2=selcov[:k], cumpvarx=cpx[:k], cumpvary=cpy[:k])
    return Covsel(tab, cov2, Cm[:, :k], k, xm, ym, ys, G[:, :k], QtY[:k], Q[:, :k])


def covsel(X, Y, nlv: Optional[int] = None, typ: str = "cov", ctx: Optional[Context] = None) -> Covsel:
    """`covsel(X, Y; nlv = nothing, typ = "cov")` — src/covsel.jl:54-57: X and Y are left untouched (and, unlike the reference, not
    copied: the selection only reads X).  nlv = None selects p variables (:63)."""
    return _fit(X, Y, nlv, typ, ctx, False)


def covsel_(X, Y, nlv: Optional[int] = None, typ: str = "cov", ctx: Optional[Context] = None) -> Covsel:
    """`covsel!(X::Matrix, Y::Matrix; nlv = nothing, typ = "cov")` — src/covsel.jl:59-122: the caller's column-major float64 X and Y end
    up centred (Y scaled when q > 1) and orthogonalised to every selected column, as the reference leaves them (:112-113)."""
    return _fit(X, Y, nlv, typ, ctx, True)


def _back_substitute(R, Z):
    """R^-1 Z for an upper triangular R (nlv x nlv): the whole of covselr's regression once Q and G are there."""
    k = R.shape[0]
    B = np.array(Z, dtype=np.float64, copy=True)
    for i in range(k - 1, -1, -1):
        B[i] = (B[i] - R[i, i + 1:] @ B[i + 1:]) / R[i, i]
    return B


def covselr(X, Y, nlv, typ: str = "cov", ctx: Optional[Context] = None) -> Covselr:
    """`covselr(X, Y; nlv, typ = "cov")` — src/covselr.jl:48-53: `covsel`, then the MLR of Y on the selected columns.  With
    Xc[:, sel] = Q R and R[k, i] = G[sel_i, k] the least-squares coefficients are B = R^-1 Q'Yc: a nlv x nlv triangular solve on the
    host, rescaled by yscales to the raw Y; int = ymeans - xmeans[sel]' B."""
    if nlv is None:
        raise ValueError("covselr needs nlv (src/covselr.jl:48)")
    res = covsel(X, Y, nlv, typ, ctx)
    s = res.sel["sel"]
    R = np.triu(res.G[s, :].T)
    B = _back_substitute(R, res.QtY) * res.yscales[None, :]
    intercept = res.ymeans[None, :] - res.xmeans[s][None, :] @ B
    return Covselr(Mlr(B, intercept), res.sel, res.cov2)


def covselr_coef(fm: Covselr):
    """`coef(object.fm)` of the reference's Mlr: (B nlv x q, int 1 x q)."""
    return fm.fm.B, fm.fm.int


def covselr_predict(fm: Covselr, X, ctx: Optional[Context] = None):
    """`predict(object::Covselr, X)` — src/covselr.jl:61-64: int + X[:, sel] B through jch_affine_gemm on the gathered columns."""
    X = ensure_mat(X)
    s = fm.sel["sel"]
    if s.size and X.shape[1] <= int(s.max()):
        raise ValueError(f"DimensionMismatch: X has {X.shape[1]} columns, the model selected column {int(s.max())}")
    if _is_torch(X):
        Xs = X[:, torch.as_tensor(s, device=X.device)]
    else:
        Xs = np.asarray(X)[:, s]
    return _affine(Xs, None, None, fm.fm.B, fm.fm.int.reshape(-1), ctx)
