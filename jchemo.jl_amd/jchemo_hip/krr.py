"""Kernel ridge regression (LS-SVM) — host-side mirror of the reference's src/krr.jl, src/krrda.jl and `gridscorelb`
(src/gridscore.jl:235-284) over jch_krr_fit / jch_krr_solve / jch_kplsr_transform (include/jchemo_hip.h).

Deviation from the reference: the fit keeps Kd = sqrtD Kc sqrtD on the device and every lb is one Cholesky factorisation of
Kd + lb^2 I there, so the record has no `U`, `UtDY` and `sv` fields (the reference keeps the full svd(Kd)); A, the predictions and
df are the same quantities."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Optional, Sequence, Union

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .plsr import (_addr_ld, _affine, _as_colmajor_copy, _as_colmajor_view, _grid_table, _is_torch, _kern_args, _model_vec, _np, _np_host,
                   _pars_rows, _same_kind, _score_from_sums, _score_sums, _x_out, colmajor_empty, dummy, ensure_mat)

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


@dataclass
class Krr:
    """The reference's `Krr` (src/krr.jl:1-17) without `U`, `UtDY`, `sv` (no SVD is taken) and with `Kd`, `B` in their place.  `X`
    is the (scaled) training X the predictions are built on; `Kd` = sqrtD Kc sqrtD (n x n) always stays on the device; `B` =
    sqrtD Y (n x q), `vtot` (1 x n) and `weights` live where X lives; xscales and ymeans are host arrays.  `solved` caches, per
    lb, what `krr_coef` computed (A, alpha = sqrtD A, df)."""
    X: object
    Kd: object
    B: object
    vtot: object
    lb: float
    xscales: np.ndarray
    ymeans: np.ndarray
    weights: object
    kern: str
    dots: dict
    solved: dict = field(default_factory=dict, repr=False)


def _check_lb(lb, what="lb"):
    v = float(lb)
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"{what} = {lb} must be finite and > 0 (Kd is singular by construction; the reference returns Inf / NaN at 0)")
    return v


def _lb_list(fm: Krr, lb):
    if lb is None:
        return [fm.lb], False
    if np.ndim(lb) == 0:
        return [_check_lb(lb)], False
    vals = [_check_lb(v) for v in np.asarray(lb).reshape(-1)]
    if not vals:
        raise ValueError("lb is empty")
    return vals, len(vals) > 1


def _krr_fit(X, Y, weights, lb, kern, scal, ctx, kwargs) -> Krr:
    kind, gamma, coef0, degree = _kern_args(kern, kwargs)
    lb = _check_lb(lb)
    dev = _is_torch(X)
    if dev != _is_torch(Y):
        raise TypeError("X and Y must both be host arrays or both device tensors")
    n, p = X.shape
    q = Y.shape[1]
    if Y.shape[0] != n:
        raise ValueError(f"DimensionMismatch: X has {n} rows, Y has {Y.shape[0]}")
    if weights is None:
        w_arr, w_addr = None, None
    elif dev:
        w_arr = (weights if _is_torch(weights) else torch.as_tensor(np.asarray(weights, dtype=np.float64), device=X.device)).to(torch.float64).reshape(-1).contiguous()
        w_addr = w_arr.data_ptr()
    else:
        w_arr = np.ascontiguousarray(np.asarray(weights.cpu() if _is_torch(weights) else weights, dtype=np.float64).reshape(-1))
        w_addr = w_arr.ctypes.data
    if w_arr is not None and w_arr.shape[0] != n:
        raise ValueError(f"DimensionMismatch: weights has {w_arr.shape[0]} entries, X has {n} rows")
    if torch is None:
        raise TypeError("krr needs torch (Kd stays on the device)")
    ctx = ctx or default_context((X.device.index or 0) if dev else 0)
    Kd = colmajor_empty(n, n, X.device if dev else f"cuda:{ctx.device}")
    if dev:
        B = colmajor_empty(n, q, X.device)
        vt = torch.empty((1, n), dtype=torch.float64, device=X.device)
        wn = torch.empty(n, dtype=torch.float64, device=X.device)
        addrs = [B.data_ptr(), vt.data_ptr(), wn.data_ptr()]
    else:
        B = np.empty((n, q), order="F"); vt = np.empty((1, n)); wn = np.empty(n)
        addrs = [B.ctypes.data, vt.ctypes.data, wn.ctypes.data]
    xs = np.empty(p); ym = np.empty(q)
    xa, ldx = _addr_ld(X)
    ya, ldy = _addr_ld(Y)
    torch.cuda.current_stream(Kd.device).synchronize()
    ctx.check(_lib.load().jch_krr_fit(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, kind, gamma, coef0, degree, xa, n, p, ldx, ya, q, ldy,
                                      w_addr, int(bool(scal)), Kd.data_ptr(), None, *addrs, xs.ctypes.data, ym.ctypes.data))
    return Krr(X, Kd, B, vt, lb, xs, ym, wn, kern, dict(kwargs))


def _y_mat(Y):
    Y = ensure_mat(Y)
    try:
        _addr_ld(Y)
    except (ValueError, TypeError):
        Y = _as_colmajor_copy(Y)
    return Y


def krr(X, Y, weights=None, *, lb, kern: str = "krbf", scal: bool = False, ctx: Optional[Context] = None, **kwargs) -> Krr:
    """`krr(X, Y, weights; lb, kern = "krbf", scal = false, kwargs...)` — src/krr.jl:122-126: the fit on a copy of X (X and Y are left
    untouched; the model keeps its own, scaled when `scal`, copy of X).  `kwargs` are the kernel's keywords (krbf: gamma; kpol:
    degree, gamma, coef0).  No SVD: the record keeps Kd on the device instead of U, UtDY and sv; `krr_coef` solves per lb."""
    _kern_args(kern, kwargs)
    _check_lb(lb)
    return _krr_fit(_as_colmajor_copy(X), _y_mat(Y), weights, lb, kern, scal, ctx, kwargs)


def krr_(X, Y, weights=None, *, lb, kern: str = "krbf", scal: bool = False, ctx: Optional[Context] = None, **kwargs) -> Krr:
    """`krr!(X::Matrix, Y::Matrix, ...)` — src/krr.jl:128-159: with `scal`, X is divided by its column stds in place; Y is not
    touched.  The model refers to the caller's X."""
    _kern_args(kern, kwargs)
    _check_lb(lb)
    return _krr_fit(_as_colmajor_view(X), _y_mat(Y), weights, lb, kern, scal, ctx, kwargs)


def _solve(fm: Krr, lb: float, want_df: bool, ctx: Optional[Context]):
    hit = fm.solved.get(lb)
    if hit is not None and (hit["df"] is not None or not want_df):
        return hit
    dev = _is_torch(fm.X)
    n, q = fm.B.shape
    ctx = ctx or default_context(fm.Kd.device.index or 0)
    if dev:
        A, al = colmajor_empty(n, q, fm.X.device), colmajor_empty(n, q, fm.X.device)
        addrs = (fm.B.data_ptr(), fm.weights.data_ptr(), A.data_ptr(), al.data_ptr())
    else:
        A, al = np.empty((n, q), order="F"), np.empty((n, q), order="F")
        addrs = (fm.B.ctypes.data, fm.weights.ctypes.data, A.ctypes.data, al.ctypes.data)
    df = C.c_double(float("nan")); info = C.c_int32(0)
    torch.cuda.current_stream(fm.Kd.device).synchronize()
    ctx.check(_lib.load().jch_krr_solve(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, fm.Kd.data_ptr(), n, addrs[0], q, addrs[1], lb,
                                        int(want_df), addrs[2], addrs[3], C.addressof(df), C.byref(info)))
    hit = dict(A=A, alpha=al, df=float(df.value) if want_df else None)
    fm.solved[lb] = hit
    return hit


def krr_coef(fm: Krr, *, lb=None, df: bool = True, ctx: Optional[Context] = None):
    """`coef(object::Krr; lb = nothing)` — src/krr.jl:168-177: (A, int, df) with A = (Kd + lb^2 I)^-1 sqrtD Y (n x q, where the
    model's X lives), int = ymeans' (1 x q) and df = 1 + sum eig / (eig + lb^2), computed as 1 + n - lb^2 |L^-1|_F^2 from the
    Cholesky factor (`df=False` skips that pass and returns None for it).  Solved values are cached per lb."""
    lb = fm.lb if lb is None else _check_lb(lb)
    hit = _solve(fm, lb, bool(df), ctx)
    return hit["A"], fm.ymeans.reshape(1, -1), (hit["df"] if df else None)


def krr_predict(fm: Krr, X, *, lb: Union[None, float, Sequence[float]] = None, ctx: Optional[Context] = None):
    """`predict(object::Krr, X; lb = nothing)` — src/krr.jl:187-202: ymeans + Kc_new sqrtD A(lb) with Kc_new the centred Gram of
    the new rows against the training rows; one lb gives a matrix, a collection a list of matrices.  All lb share ONE pass over
    the Gram blocks of the new rows (jch_kplsr_transform with the alphas side by side); the constant of the centring is
    weights . vtot."""
    lbs, many = _lb_list(fm, lb)
    kind, gamma, coef0, degree = _kern_args(fm.kern, fm.dots)
    X = _same_kind(X, fm.X)
    if X.shape[1] != fm.X.shape[1]:
        raise ValueError(f"DimensionMismatch: X has {X.shape[1]} columns, the model has {fm.X.shape[1]}")
    q = fm.B.shape[1]
    R = np.asfortranarray(np.hstack([_np_host(_solve(fm, v, False, ctx)["alpha"]) for v in lbs]), dtype=np.float64)
    k = R.shape[1]
    X, T, oa, ctx, loc = _x_out(X, k, ctx)
    xa, ldx = _addr_ld(X)
    ta, ldt = _addr_ld(fm.X)
    xs, w, vt = _model_vec(fm.xscales), _model_vec(_np_host(fm.weights)), _model_vec(_np_host(fm.vtot).reshape(-1))
    ctx.check(_lib.load().jch_kplsr_transform(ctx._h, loc, kind, gamma, coef0, degree, xa, X.shape[0], X.shape[1], ldx, xs.ctypes.data, ta,
                                              fm.X.shape[0], ldt, w.ctypes.data, vt.ctypes.data, R.ctypes.data, k, oa, max(X.shape[0], 1)))
    out = _affine(T, None, None, np.eye(k), np.tile(fm.ymeans, len(lbs)), ctx)   # + ymeans (src/krr.jl:198), on the device
    preds = [out[:, i * q:(i + 1) * q] for i in range(len(lbs))]
    return preds if many else preds[0]


def gridscorelb(Xtrain, Ytrain, X, Y, *, score, fun, lb, pars=None, verbose: bool = False, ctx: Optional[Context] = None, **kwargs):
    """`gridscorelb(Xtrain, Ytrain, X, Y; score, fun, lb, pars, verbose)` — src/gridscore.jl:235-284: per parameter combination one
    fit (at max(lb)) and ONE predict over all lb (`mlev(lb)`: the sorted distinct values), scores from device-side sums.
    `pars` must not contain `lb`.  Returns dict(lb=[...], <one list per pars key>, res=(ncomb * le_lb, q)), rows combination-major."""
    if pars is not None and "lb" in pars:
        raise ValueError("Argument `pars` must not contain `lb` (src/gridscore.jl:231)")
    lbs = sorted({_check_lb(v) for v in np.atleast_1d(np.asarray(lb)).reshape(-1)})   # mlev
    rows = _pars_rows(pars)
    name = getattr(score, "_jch_name", None)
    predict_fun = krr_predict
    if verbose:
        print("-- Nb. combinations = 0." if pars is None else f"-- Nb. combinations = {len(rows)}")
    blocks = []
    for kw in rows:
        if verbose and pars is not None:
            print("".join(f"{k_} => {v_}" for k_, v_ in kw.items()))
        fm = fun(Xtrain, Ytrain, lb=max(lbs), ctx=ctx, **kwargs, **kw)
        pred = predict_fun(fm, X, lb=lbs, ctx=ctx)
        pred = pred if isinstance(pred, list) else [pred]
        if name is None:
            blocks.append(np.vstack([np.asarray(score(pr, Y)).reshape(1, -1) for pr in pred]))
        else:
            Yk = _same_kind(ensure_mat(Y), pred[0])
            blocks.append(np.vstack([_score_from_sums(name, _score_sums(pr, Yk, None, ctx)) for pr in pred]))
    if verbose:
        print("-- End.")
    tab = _grid_table(pars, lbs, np.vstack(blocks))
    out = dict(lb=tab.pop("nlv"))   # the level column is `lb` here (src/gridscore.jl:249, 277)
    out.update(tab)
    return out


@dataclass
class Krrda:
    """What the reference's `krrda` returns (its `Rrda`, src/krrda.jl:65): fm::Krr on the dummy table, lev, ni."""
    fm: Krr
    lev: np.ndarray
    ni: np.ndarray


def krrda(X, y, weights=None, *, lb, kern: str = "krbf", scal: bool = False, ctx: Optional[Context] = None, **kwargs) -> Krrda:
    """`krrda(X, y, weights; lb, kern = "krbf", scal = false, kwargs...)` — src/krrda.jl:59-66: krr on `dummy(y)`."""
    _kern_args(kern, kwargs)
    _check_lb(lb)
    Yd, lev = dummy(y)
    yv = np.asarray(y.cpu() if _is_torch(y) else y).reshape(-1)
    ni = np.array([(yv == l).sum() for l in lev])
    X = ensure_mat(X)
    if _is_torch(X):
        Yt = colmajor_empty(Yd.shape[0], Yd.shape[1], X.device); Yt.copy_(torch.from_numpy(Yd)); Yd = Yt
    return Krrda(krr(X, Yd, weights, lb=lb, kern=kern, scal=scal, ctx=ctx, **kwargs), lev, ni)


def krrda_predict(obj: Krrda, X, *, lb=None, ctx: Optional[Context] = None):
    """`predict(object::Rrda, X; lb)` — src/rrda.jl:79-97: (pred, posterior) with pred the level of the largest posterior (the first
    one on ties, as `argmax`); lists when several lb."""
    post = krr_predict(obj.fm, X, lb=lb, ctx=ctx)
    many = isinstance(post, list)
    posts = post if many else [post]
    preds = [obj.lev[np.argmax(_np_host(z), axis=1)].reshape(-1, 1) for z in posts]
    return (preds, posts) if many else (preds[0], posts[0])
