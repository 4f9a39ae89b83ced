"""Calibration transfer and the plain linear models it defaults to — host-side mirror of the reference's src/calds.jl, src/calpds.jl,
src/eposvd.jl, src/difmean.jl and src/mlr.jl (include/jchemo_hip.h).

The fits are tiny (n standards times a window) and run on the host; the hot path is `predict(::CalPds, X)` on a spectral library: every
per-column model with a `coef` predicts int_j + sum_t B_j[t] x[i, j - zm_j + t], so the whole transform is ONE banded map with taps
of its own per output column — one `jch_rows_fir` call in mode JCH_FIR_SAME | JCH_FIR_PER_COLUMN (one read and one write of X) where the
reference runs p predictions on gathered windows.

numpy in gives numpy out; a device torch tensor in gives a device tensor out.

Departures from the reference: `mlr` factors with the unpivoted Householder QR (LAPACK geqrf; the reference's `\\` pivots
the columns) and raises on a numerically rank-deficient X instead of returning a basic solution — `mlrpinv` is the function for those;
beyond HOST_ROUTE_MAX elements only the normal-equations functions run (`mlrchol`, `mlrpinvn`, `mlrvec` with an intercept); the `_`
forms centre X and Y in place on the host route only; a window that leaves the matrix raises ValueError (the reference: BoundsError)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .covsel import Mlr
from .plsr import _addr_ld, _affine, _as_colmajor_copy, _col_stats, _is_torch, colmajor_empty, ensure_mat
from .preproc import FIR_SAME, _call, _in_out

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

FIR_PER_COLUMN = 4            # include/jchemo_hip.h JCH_FIR_PER_COLUMN
HOST_ROUTE_MAX = 1 << 22      # n (p + q) up to which every mlr function runs on the host in numpy
EPOSVD_MAX = 1 << 24          # elements of D up to which eposvd takes its host SVD
_RTOL = math.sqrt(np.finfo(np.float64).eps)   # the reference's pinv(...; rtol = sqrt(eps))
_COEF_TYPES = ("Mlr", "Plsr", "Pcr", "Covselr")   # per-column models whose `coef` is (B, int): the five PLS fits all return a Plsr


@dataclass
class CalDs:
    """The reference's `CalDs` (src/calds.jl:1-3)."""
    fm: object


@dataclass
class CalPds:
    """The reference's `CalPds` (src/calpds.jl:1-4): the p per-column models and their windows `s` (0-based column indices here)."""
    fm: list
    s: list


# ---------------------------------------------------------------------------------- the mlr family (src/mlr.jl)
def _host(A):
    return A.detach().cpu().numpy() if _is_torch(A) else np.asarray(A)


def _mweight(weights, n):
    if weights is None:
        return np.full(n, 1.0 / n)
    w = np.asarray(_host(weights), dtype=np.float64).reshape(-1)
    if w.shape[0] != n:
        raise ValueError(f"DimensionMismatch: weights has {w.shape[0]} entries, X has {n} rows")
    return w / w.sum()


def _back_substitute(R, Z):
    B = np.array(Z, dtype=np.float64, copy=True)
    for i in range(R.shape[0] - 1, -1, -1):
        B[i] = (B[i] - R[i, i + 1:] @ B[i + 1:]) / R[i, i]
    return B


def _solve(kind, Xc, Yc, w):
    """B of the weighted least-squares problem on already centred (or, noint, raw) data, by the routine the reference's function uses."""
    if kind in ("mlr", "mlrpinv"):
        sq = np.sqrt(w)[:, None]
        A, Z = sq * Xc, sq * Yc
        if kind == "mlrpinv":
            return np.linalg.pinv(A, rcond=_RTOL) @ Z                        # src/mlr.jl:170-172, 178-180
        Q, R = np.linalg.qr(A)                                               # :84, :91 (geqrf; the reference pivots)
        d = np.abs(np.diag(R))
        if A.shape[0] < A.shape[1] or d.min() <= A.shape[1] * np.finfo(np.float64).eps * d.max():
            raise np.linalg.LinAlgError("mlr: X is numerically rank deficient for the unpivoted QR (use mlrpinv)")
        return _back_substitute(R, Q.T @ Z)
    XtD = Xc.T * w[None, :]
    return _solve_normal(kind, XtD @ Xc, XtD @ Yc)


def _solve_normal(kind, G, K):
    """B from G = Xc'D Xc and K = Xc'D Yc: the whole of mlrchol, mlrpinvn and mlrvec after the moments."""
    if kind == "mlrchol":
        L = np.linalg.cholesky(G)                                            # src/mlr.jl:127 (LinAlgError when not positive definite)
        return np.linalg.solve(L.T, np.linalg.solve(L, K))
    if kind == "mlrpinvn":
        return np.linalg.pinv(G, rcond=_RTOL) @ K                            # :213-215
    return K / G                                                             # mlrvec :253, :261: the scalar ratio


def _check_xy(X, Y, kind):
    X, Y = ensure_mat(X), ensure_mat(Y)
    if _is_torch(X) != _is_torch(Y):
        raise TypeError("X and Y must both be host arrays or both device tensors")
    if X.ndim != 2 or Y.ndim != 2:
        raise ValueError("X and Y must be matrices (or vectors)")
    if Y.shape[0] != X.shape[0]:
        raise ValueError(f"DimensionMismatch: X has {X.shape[0]} rows, Y has {Y.shape[0]}")
    if X.shape[0] < 1 or X.shape[1] < 1 or Y.shape[1] < 1:
        raise ValueError("X and Y need at least one row and one column each")
    if kind == "mlrchol" and X.shape[1] < 2:
        raise ValueError("Method only working for X with > 1 column.")      # src/mlr.jl:119
    if kind == "mlrvec" and X.shape[1] != 1:
        raise ValueError("Method only working for univariate x.")           # :246
    return X, Y


def _fit_host(kind, X, Y, weights, noint, inplace):
    n = X.shape[0]
    w = _mweight(weights, n)
    Xh, Yh = np.asarray(_host(X), dtype=np.float64), np.asarray(_host(Y), dtype=np.float64)
    q = Yh.shape[1]
    if noint:
        return Mlr(_solve(kind, Xh, Yh, w), np.zeros((1, q)), w)
    xmeans, ymeans = w @ Xh, w @ Yh
    Xc, Yc = Xh - xmeans[None, :], Yh - ymeans[None, :]
    if inplace:                                                              # the reference's `!`: center!(X, xmeans), center!(Y, ymeans)
        for A, Ac in ((X, Xc), (Y, Yc)):
            if _is_torch(A):
                A.copy_(torch.as_tensor(Ac, dtype=A.dtype))
            else:
                A[...] = Ac
    B = _solve(kind, Xc, Yc, w)
    return Mlr(B, ymeans[None, :] - xmeans[None, :] @ B, w)


def _fit_moments(kind, X, Y, weights, ctx):
    """The device route of mlrchol / mlrpinvn / mlrvec: G = Xc'D Xc and xmeans from jch_xtdx, Xc'D Yc from jch_covsel_pass with the panel
    V = D Yc (as pcr takes its Xs'D Yc), then the p x p system on the host.  X and Y are only read."""
    X, Y = (A if _is_torch(A) else torch.as_tensor(np.asarray(A, dtype=np.float64), device="cuda") for A in (X, Y))
    if not (X.is_cuda and Y.is_cuda):
        raise TypeError("torch inputs must live on the GPU (host data: pass numpy arrays)")
    try:
        _addr_ld(X)
    except (ValueError, TypeError):
        X = _as_colmajor_copy(X)
    n, p = X.shape
    q = Y.shape[1]
    ctx = ctx or default_context(X.device.index or 0)
    w = None if weights is None else (weights if _is_torch(weights) else torch.as_tensor(np.asarray(weights, dtype=np.float64))).to(X.device, torch.float64).reshape(-1).contiguous()
    if w is not None and w.shape[0] != n:
        raise ValueError(f"DimensionMismatch: weights has {w.shape[0]} entries, X has {n} rows")
    wn = torch.full((n,), 1.0 / n, dtype=torch.float64, device=X.device) if w is None else w / w.sum()
    ymeans, _ = _col_stats(Y, w, False, ctx)
    G = np.empty((p, p), order="F")
    xmeans = np.empty(p)
    mu = torch.empty(p, dtype=torch.float64, device=X.device)
    V = colmajor_empty(n, q, X.device)
    V.copy_((Y.to(torch.float64) - torch.as_tensor(ymeans, device=X.device)[None, :]) * wn[:, None])
    K = colmajor_empty(p, q, X.device)
    xa, ldx = _addr_ld(X)
    torch.cuda.current_stream(X.device).synchronize()
    L = _lib.load()
    ctx.check(L.jch_xtdx(ctx._h, _lib.LOC_DEVICE, xa, n, p, ldx, None if w is None else w.data_ptr(), None, p, mu.data_ptr(), G.ctypes.data,
                         xmeans.ctypes.data))
    ctx.check(L.jch_covsel_pass(ctx._h, xa, n, p, ldx, mu.data_ptr(), V.data_ptr(), q, n, K.data_ptr()))
    ctx.check(L.jch_ctx_synchronize(ctx._h))
    B = _solve_normal(kind, G, K.cpu().numpy())
    return Mlr(B, ymeans[None, :] - xmeans[None, :] @ B, wn.cpu().numpy())


def _fit(kind, X, Y, weights, noint, inplace, ctx):
    X, Y = _check_xy(X, Y, kind)
    n, p = X.shape
    if n * (p + Y.shape[1]) <= HOST_ROUTE_MAX:
        return _fit_host(kind, X, Y, weights, bool(noint), inplace)
    if kind in ("mlr", "mlrpinv") or noint:
        raise NotImplementedError(f"{kind}{'(noint)' if noint else ''}: beyond n (p + q) = {HOST_ROUTE_MAX} only the normal-equations functions "
                                  "mlrchol / mlrpinvn (with an intercept) run, from one Gram pass on the device; a tall QR or SVD is not provided")
    return _fit_moments(kind, X, Y, weights, ctx)


def mlr(X, Y, weights=None, *, noint: bool = False, ctx: Optional[Context] = None) -> Mlr:
    """`mlr(X, Y, weights; noint = false)` — src/mlr.jl:68-95: least squares of sqrtD Xc by QR.  X and Y are only read."""
    return _fit("mlr", X, Y, weights, noint, False, ctx)


def mlr_(X, Y, weights=None, *, noint: bool = False, ctx: Optional[Context] = None) -> Mlr:
    """`mlr!` — src/mlr.jl:74-95.  On the host route X and Y end up centred in place, as the reference leaves them (not with noint); there is
    no device route for this function."""
    return _fit("mlr", X, Y, weights, noint, True, ctx)


def mlrchol(X, Y, weights=None, *, ctx: Optional[Context] = None) -> Mlr:
    """`mlrchol(X, Y, weights)` — src/mlr.jl:114-130: Cholesky of Xc'D Xc; X needs more than one column; a matrix that is not positive
    definite raises numpy's LinAlgError.  Beyond HOST_ROUTE_MAX elements the moments come from the device (jch_xtdx, jch_covsel_pass)."""
    return _fit("mlrchol", X, Y, weights, False, False, ctx)


def mlrchol_(X, Y, weights=None, *, ctx: Optional[Context] = None) -> Mlr:
    """`mlrchol!` — src/mlr.jl:118-130.  On the host route X and Y end up centred in place; on the device route they are left alone."""
    return _fit("mlrchol", X, Y, weights, False, True, ctx)


def mlrpinv(X, Y, weights=None, *, noint: bool = False, ctx: Optional[Context] = None) -> Mlr:
    """`mlrpinv(X, Y, weights; noint = false)` — src/mlr.jl:151-182: pinv(sqrtD Xc, rtol = sqrt(eps)) sqrtD Yc, the minimum-norm solution
    on a rank-deficient X.  X and Y are only read."""
    return _fit("mlrpinv", X, Y, weights, noint, False, ctx)


def mlrpinv_(X, Y, weights=None, *, noint: bool = False, ctx: Optional[Context] = None) -> Mlr:
    """`mlrpinv!` — src/mlr.jl:157-182.  On the host route X and Y end up centred in place (not with noint); there is no device route."""
    return _fit("mlrpinv", X, Y, weights, noint, True, ctx)


def mlrpinvn(X, Y, weights=None, *, ctx: Optional[Context] = None) -> Mlr:
    """`mlrpinvn(X, Y, weights)` — src/mlr.jl:201-217: pinv(Xc'D Xc, rtol = sqrt(eps)) Xc'D Yc.  Beyond HOST_ROUTE_MAX elements the moments
    come from the device (jch_xtdx, jch_covsel_pass) and the p x p pseudo-inverse is taken on the host."""
    return _fit("mlrpinvn", X, Y, weights, False, False, ctx)


def mlrpinvn_(X, Y, weights=None, *, ctx: Optional[Context] = None) -> Mlr:
    """`mlrpinvn!` — src/mlr.jl:205-217.  On the host route X and Y end up centred in place; on the device route they are left alone."""
    return _fit("mlrpinvn", X, Y, weights, False, True, ctx)


def mlrvec(x, Y, weights=None, *, noint: bool = False, ctx: Optional[Context] = None) -> Mlr:
    """`mlrvec(x, Y, weights; noint = false)` — src/mlr.jl:237-265: univariate x, B = (x'D Y) ./ (x'D x)."""
    return _fit("mlrvec", x, Y, weights, noint, False, ctx)


def mlrvec_(x, Y, weights=None, *, noint: bool = False, ctx: Optional[Context] = None) -> Mlr:
    """`mlrvec!` — src/mlr.jl:243-265.  On the host route x and Y end up centred in place (not with noint); on the device route (intercept
    only) they are left alone."""
    return _fit("mlrvec", x, Y, weights, noint, True, ctx)


def mlr_coef(fm: Mlr):
    """`coef(object::Mlr)` — src/mlr.jl:275-277: (B p x q, int 1 x q)."""
    return fm.B, fm.int


def mlr_predict(fm: Mlr, X, ctx: Optional[Context] = None):
    """`predict(object::Mlr, X)` — src/mlr.jl:287-292: int + X B, one jch_affine_gemm."""
    return _affine(X, None, None, fm.B, np.asarray(fm.int).reshape(-1), ctx)


# ---------------------------------------------------------------------------------- calds (src/calds.jl)
def _resolve(fun):
    """`fun` may be a string naming a mirror function (the reference evals the name, src/calds.jl:61-63)."""
    if isinstance(fun, str):
        import jchemo_hip
        if not callable(getattr(jchemo_hip, fun, None)):
            raise ValueError(f"fun = {fun!r} names no function of jchemo_hip")
        return getattr(jchemo_hip, fun)
    return fun


def _predict(fm, X, **kwargs):
    """`predict` of whatever `fun` returned: the models `plsr.predict` dispatches, and Krr."""
    if type(fm).__name__ == "Krr":
        from .krr import krr_predict
        return krr_predict(fm, X, **kwargs)
    from .plsr import predict
    return predict(fm, X, **kwargs)


def calds(X, Xt, *, fun=mlrpinv, **kwargs) -> CalDs:
    """`calds(X, Xt; fun = mlrpinv, kwargs...)` — src/calds.jl:59-66: direct standardization, one model `fun(X, Xt; kwargs...)` that
    predicts the target spectra Xt from X (the same n standards on both instruments)."""
    return CalDs(_resolve(fun)(X, Xt, **kwargs))


def calds_predict(obj: CalDs, X, **kwargs):
    """`predict(object::CalDs, X; kwargs...)` — src/calds.jl:74-76."""
    return _predict(obj.fm, X, **kwargs)


# ---------------------------------------------------------------------------------- calpds (src/calpds.jl)
def pds_windows(p: int, m: int):
    """The half-widths zm and the windows s of src/calpds.jl:70-77, built literally: all m, then zm[0:m] = 0..m-1, then zm[p-m:p] = m-1..0
    (the second assignment overrides the first where they overlap).  0-based.  p < m, or a window that leaves the matrix, raises
    ValueError (the reference: BoundsError)."""
    p, m = int(p), int(m)
    if p < 1 or m < 0:
        raise ValueError(f"calpds: p = {p} must be >= 1 and m = {m} >= 0")
    if p < m:
        raise ValueError(f"calpds: p = {p} columns cannot hold the half-window m = {m}")
    zm = np.full(p, m, dtype=np.int64)
    zm[0:m] = np.arange(m)
    zm[p - m:p] = np.arange(m - 1, -1, -1)
    s = [np.arange(i - zm[i], i + zm[i] + 1) for i in range(p)]
    for i, si in enumerate(s):
        if si[0] < 0 or si[-1] > p - 1:
            raise ValueError(f"calpds: the window of column {i} ({si[0]}..{si[-1]}) leaves the matrix (p = {p}, m = {m})")
    return zm, s


def pds_table(coefs, s, m: int):
    """The jch_rows_fir per-column table of a PDS model: ((f + 1) x p column-major table, f = 2m + 1, lo = -m).  coefs[i] = (B_i, int_i) of
    the model of column i on the window s[i] (0-based, contiguous, centred on i).  Column i of the table holds B_i at the rows
    m - zm_i ... m + zm_i, exact 0.0 elsewhere (the kernel skips those taps: a shrunken border window never reads a clamped column), and
    int_i in row f."""
    p, m = len(s), int(m)
    f = 2 * m + 1
    tab = np.zeros((f + 1, p), order="F")
    for i, ((B, c), si) in enumerate(zip(coefs, s)):
        B = np.asarray(B, dtype=np.float64).reshape(-1)
        zm = (len(si) - 1) // 2
        if len(si) != 2 * zm + 1 or zm > m or si[0] != i - zm or si[-1] != i + zm or B.shape[0] != len(si):
            raise ValueError(f"pds_table: column {i}: {B.shape[0]} coefficients on the window {si[0]}..{si[-1]} (half-width at most {m} around {i})")
        tab[m - zm:m + zm + 1, i] = B
        tab[f, i] = float(np.asarray(c).reshape(-1)[0])
    return tab, f, -m


def _window(A, lo, hi):
    """Columns lo..hi of A as a view (no copy): a column-major X keeps its leading dimension."""
    return A[:, lo:hi + 1]


def calpds(X, Xt, *, fun=mlrpinv, m: int = 5, **kwargs) -> CalPds:
    """`calpds(X, Xt; fun = mlrpinv, m = 5, kwargs...)` — src/calpds.jl:66-83: piecewise direct standardization, column i of Xt is predicted
    from the window i - zm_i ... i + zm_i of X by its own model `fun(X[:, s_i], Xt[:, i]; kwargs...)` (zm = m away from the borders).  The
    windows are column views.  Example of the reference: calpds(Xcal, Xtcal, fun=plskern, nlv=1, m=2)."""
    X, Xt = ensure_mat(X), ensure_mat(Xt)
    if tuple(X.shape) != tuple(Xt.shape):
        raise ValueError(f"DimensionMismatch: X is {tuple(X.shape)}, Xt is {tuple(Xt.shape)} (the same standards on both instruments)")
    fun = _resolve(fun)
    _, s = pds_windows(Xt.shape[1], m)
    fm = [fun(_window(X, si[0], si[-1]), _window(Xt, i, i), **kwargs) for i, si in enumerate(s)]
    return CalPds(fm, s)


def calpds_predict(obj: CalPds, X, *, ctx: Optional[Context] = None, inplace: bool = False, **kwargs):
    """`predict(object::CalPds, X; kwargs...)` — src/calpds.jl:91-99.  Where every per-column model has a `coef` (Mlr, the five PLS fits,
    Pcr, Covselr) the coefficients `coef(fm_i; kwargs...)` are assembled into the per-column table (`pds_table`) and the whole transform is
    ONE jch_rows_fir call (one read and one write of X; `inplace = True` overwrites the caller's column-major X).  Any other model runs the
    reference's per-column loop.  `nlv` given as a collection raises (the reference would fail to assign a list to a column)."""
    X = ensure_mat(X)
    p = len(obj.fm)
    if X.shape[1] != p:
        raise ValueError(f"DimensionMismatch: X has {X.shape[1]} columns, the model has {p}")
    if "nlv" in kwargs and kwargs["nlv"] is not None and np.ndim(kwargs["nlv"]) != 0:
        raise ValueError("predict(CalPds): nlv must be one value (each model predicts one column)")
    if all(type(f).__name__ in _COEF_TYPES for f in obj.fm):
        from .plsr import coef
        coefs = []
        for f in obj.fm:
            B, c = coef(f, **kwargs)
            if type(f).__name__ == "Covselr":                                # its B lives on the selected columns of the window
                full = np.zeros((len(obj.s[len(coefs)]), B.shape[1]))
                full[f.sel["sel"]] = B
                B = full
            coefs.append((B, c))
        m = max((len(si) - 1) // 2 for si in obj.s)
        tab, f, lo = pds_table(coefs, obj.s, m)
        Xin, out = _in_out(X, inplace, p)
        return _call("jch_rows_fir", Xin, out, ctx, tab.ctypes.data, f, lo, FIR_SAME | FIR_PER_COLUMN)
    if inplace:
        raise ValueError("predict(CalPds): in place needs models with a coef")
    dev = _is_torch(X)
    pred = colmajor_empty(X.shape[0], p, X.device) if dev else np.empty((X.shape[0], p), order="F")
    kw = dict(kwargs) if ctx is None else dict(kwargs, ctx=ctx)
    for i, si in enumerate(obj.s):
        col = _predict(obj.fm[i], _window(X, si[0], si[-1]), **kw)[:, 0]
        if dev != _is_torch(col):                                            # (a model fitted on host arrays may answer on the host)
            col = torch.as_tensor(np.asarray(col), device=X.device) if dev else col.cpu().numpy()
        pred[:, i] = col
    return pred


# ---------------------------------------------------------------------------------- eposvd, difmean
def eposvd(D, *, nlv):
    """`eposvd(D; nlv)` — src/eposvd.jl:87-98: (M, P) with P (p x nlv) the first right singular vectors of the UNcentred D (host SVD; D is a
    handful of difference or mean spectra), nlv = min(nlv, n, p), and M = I - P P' (p x p) the matrix that orthogonalises spectra to them:
    X_corrected = X M.  For nlv <= 8 that product is jch_rows_project_out with A = P', V = P, in place (preproc.detrend_ is the same
    call): no p x p matrix and one read of X.  Beyond EPOSVD_MAX elements of D: NotImplementedError."""
    D = np.asarray(_host(ensure_mat(D)), dtype=np.float64)
    n, p = D.shape
    if n * p > EPOSVD_MAX:
        raise NotImplementedError(f"eposvd: D is {n} x {p}; beyond {EPOSVD_MAX} elements no SVD is provided (D is a few difference or mean spectra)")
    if isinstance(nlv, bool) or int(nlv) != nlv or int(nlv) < 1:
        raise ValueError(f"nlv = {nlv} must be an integer >= 1")
    nlv = min(int(nlv), n, p)
    P = np.asfortranarray(np.linalg.svd(D, full_matrices=False)[2][:nlv].T)
    return np.eye(p) - P @ P.T, P


def difmean(X1, X2, *, normx: bool = False, ctx: Optional[Context] = None):
    """`difmean(X1, X2; normx = false)` — src/difmean.jl:41-50: (D 1 x p, xmeans1, xmeans2), D the difference of the two mean spectra
    (each normed first with normx).  The column means of a device tensor come from jch_col_stats, those of a host array from numpy."""
    X1, X2 = ensure_mat(X1), ensure_mat(X2)
    if X1.shape[1] != X2.shape[1]:
        raise ValueError(f"DimensionMismatch: X1 has {X1.shape[1]} columns, X2 has {X2.shape[1]}")
    means = [_col_stats(A, None, False, ctx)[0] if _is_torch(A) else np.asarray(A, dtype=np.float64).mean(axis=0) for A in (X1, X2)]
    if normx:
        means = [v / np.linalg.norm(v) for v in means]
    return (means[0] - means[1])[None, :], means[0], means[1]
