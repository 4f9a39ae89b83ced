"""Variable importance by permutation and interval selection — host-side mirror of the reference's src/viperm.jl and src/isel.jl over
jch_perm_fill, jch_perm_score_sums and jch_score_sums (include/jchemo_hip.h).

The reference shuffles one column of a copy of the held-out block, predicts and scores, p times per replication.  Every model here that has
`coef` predicts as int + X B, so the p shuffled predictions differ from the unshuffled one by a rank-one term and their scores come from ONE
read of X per replication (`route="fast"`).  Any other `fun`, or a callable `score`, runs the reference's loop literally (`route="loop"`) on
the same permutations: slower, never absent.

numpy in gives numpy out; device torch tensors stay on the device.  `imp`, `res` and the `isel` tables are host arrays either way.  Row and
column numbers are 0-based here (the Julia mirror gives 1-based ones)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .plsr import (_addr_ld, _as_colmajor_copy, _is_torch, _score_from_sums, _score_sums, coef, colmajor_empty, ensure_mat, plskern, plsnipals, plsrosa,
                   plssimp, plswold, predict, rmsep)
from .pca import pcr
from .covsel import covselr

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

PERM_SLICE_ROWS = 2048   # csrc/viperm.hip VP_SLICE: held-out rows per work item of the pass
PERM_QGROUP = 4          # csrc/viperm.hip VP_QG: response columns whose sums a thread holds in registers at a time

_REUSE_FUNS = (plskern, plsnipals, plssimp, plsrosa, plswold)   # fits that take weights and `reuse_x`
_WEIGHT_FUNS = _REUSE_FUNS + (pcr,)                             # fits that take weights: a split is ONE fit with weight 0 on the held-out rows
_FAST_FUNS = _WEIGHT_FUNS + (covselr,)                          # models that predict as int + X B


@dataclass
class Viperm:
    """What the reference's `viperm` returns (src/viperm.jl:108-109): imp (p x q) = the mean of res over the replications, res (p x q x perm)."""
    imp: np.ndarray
    res: np.ndarray


@dataclass
class Isel:
    """What the reference's `isel` returns (src/isel.jl:118-128): `res` = the table lo, up, mid, y1 .. yq (a dict of columns, one entry per
    interval; lo / up / mid are `wl` at the interval's bounds), `res0` = the table y1 .. yq of the fit on all columns, res_rep (nint x q x rep),
    res0_rep (1 x q x rep) and `int` (nint x 3: first column, last column, middle column of every interval, 0-based)."""
    res: dict
    res0: dict
    res_rep: np.ndarray
    res0_rep: np.ndarray
    int: np.ndarray


# ---------------------------------------------------------------------------------- the two entries
def _mat_addr_ld(a, dtype_np, dtype_t):
    """(address, leading dimension) of a column-major matrix view; a host view may have a leading dimension beyond its row count."""
    if _is_torch(a):
        if a.dtype != dtype_t:
            raise TypeError(f"expected a {dtype_t} tensor")
        n = a.shape[0]
        if n > 1 and a.stride(0) != 1:
            raise ValueError("device matrix must be column-major (stride(0) == 1); see colmajor_empty()")
        ld = a.stride(1) if a.shape[1] > 1 else max(n, 1)
        if ld < n:
            raise ValueError("bad leading dimension")
        return a.data_ptr(), ld
    if a.dtype != dtype_np:
        raise TypeError(f"expected a {np.dtype(dtype_np).name} array")
    n, item = a.shape[0], a.itemsize
    if n > 1 and a.strides[0] != item:
        raise ValueError("host matrix must be column-major (unit row stride)")
    ld = a.strides[1] // item if a.shape[1] > 1 else max(n, 1)
    if a.shape[1] > 1 and (a.strides[1] % item or ld < n):
        raise ValueError("bad leading dimension")
    return a.ctypes.data, ld


def _f64(a):
    return _mat_addr_ld(a, np.float64, torch.float64 if torch is not None else None)


def _colmajor_f64(a):
    a = ensure_mat(a)
    if not _is_torch(a):
        a = np.asarray(a)
    try:
        _f64(a)
    except (ValueError, TypeError):
        a = _as_colmajor_copy(a)
    return a


def _seed64(seed) -> int:
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed = {seed} must fit an unsigned 64-bit integer")
    return seed


def perm_fill(m: int, ncols: int, seed: int, *, device=None, ctx: Optional[Context] = None):
    """jch_perm_fill: the m x ncols int32 matrix whose column j is the permutation of 0 .. m - 1 the library generates for (seed, j)
    (include/jchemo_hip.h has the definition).  device = None gives a numpy array (Fortran order), else a column-major tensor there."""
    m, ncols, seed = int(m), int(ncols), _seed64(seed)
    if m < 1 or m >= 2 ** 31 or ncols < 1:
        raise ValueError(f"perm_fill: m = {m} (1 <= m < 2^31), ncols = {ncols} (>= 1)")
    if device is None:
        ctx = ctx or default_context(0)
        out = np.empty((m, ncols), dtype=np.int32, order="F")
        ctx.check(_lib.load().jch_perm_fill(ctx._h, _lib.LOC_HOST, out.ctypes.data, m, ncols, m, seed))
        return out
    device = torch.device(device)
    ctx = ctx or default_context(device.index or 0)
    out = torch.empty((ncols, m), dtype=torch.int32, device=device).t()
    torch.cuda.current_stream(device).synchronize()
    ctx.check(_lib.load().jch_perm_fill(ctx._h, _lib.LOC_DEVICE, out.data_ptr(), m, ncols, m, seed))
    return out


def perm_score_sums(X, Pred, Y, B, *, rows=None, m: Optional[int] = None, perm=None, seed: int = 0, ctx: Optional[Context] = None) -> np.ndarray:
    """jch_perm_score_sums: ((p + 1), q, 6) host array — rows j < p the six sums of `_score_sums` for the prediction in which column j of the
    held-out block was shuffled, row p the unshuffled ones.  X (n x p), Pred and Y (n x q) are column-major host arrays or device tensors (all
    alike); B (p x q) is a host array; rows (the held-out row numbers; None = the first `m` rows, all n when m is None too) and perm (m x p
    int32, None = generated from `seed`) live where X lives (host lists are moved there)."""
    X, Pred, Y = ensure_mat(X), ensure_mat(Pred), ensure_mat(Y)
    dev = _is_torch(X)
    if _is_torch(Pred) != dev or _is_torch(Y) != dev:
        raise TypeError("X, Pred and Y must all be host arrays or all device tensors")
    if dev and not X.is_cuda:
        raise TypeError("torch inputs must live on the GPU (host data: pass numpy arrays)")
    n, p = X.shape
    q = Y.shape[1]
    if Pred.shape != (n, q) or Y.shape[0] != n:
        raise ValueError(f"DimensionMismatch: X is {n} x {p}, Pred {tuple(Pred.shape)}, Y {tuple(Y.shape)}")
    B = np.asfortranarray(np.asarray(B, dtype=np.float64).reshape(p, -1) if np.ndim(B) == 1 else np.asarray(B, dtype=np.float64))
    if B.shape != (p, q):
        raise ValueError(f"DimensionMismatch: B is {B.shape}, expected ({p}, {q})")
    if n < 1 or p < 1 or q < 1:
        raise ValueError("perm_score_sums: at least one row and one column each")
    seed = _seed64(seed)
    if rows is not None and m is not None:
        raise ValueError("perm_score_sums: rows or m, not both")
    ra, m = None, (n if m is None else int(m))
    if rows is not None:
        if dev:
            rows = (rows if _is_torch(rows) else torch.as_tensor(np.asarray(rows, dtype=np.int64))).to(device=X.device, dtype=torch.int64).contiguous()
            ra = rows.data_ptr()
        else:
            rows = np.ascontiguousarray(rows.cpu().numpy() if _is_torch(rows) else rows, dtype=np.int64).reshape(-1)
            ra = rows.ctypes.data
        m = int(rows.shape[0])
    if m < 1 or m >= 2 ** 31 or (rows is None and m > n):
        raise ValueError(f"perm_score_sums: m = {m} held-out rows (1 <= m < 2^31; m <= n without rows)")
    pa, ldperm = None, m
    if perm is not None:
        if tuple(perm.shape) != (m, p):
            raise ValueError(f"DimensionMismatch: perm is {tuple(perm.shape)}, expected ({m}, {p})")
        if dev and not _is_torch(perm):
            t = torch.empty((p, m), dtype=torch.int32, device=X.device).t()
            t.copy_(torch.as_tensor(np.asarray(perm, dtype=np.int32)))
            perm = t
        elif not dev and _is_torch(perm):
            perm = np.asfortranarray(perm.cpu().numpy())
        try:
            pa, ldperm = _mat_addr_ld(perm, np.int32, torch.int32 if torch is not None else None)
        except (ValueError, TypeError):   # layout / integer width conversion only
            if dev:
                t = torch.empty((p, m), dtype=torch.int32, device=X.device).t()
                t.copy_(perm)
                perm = t
            else:
                perm = np.asfortranarray(perm, dtype=np.int32)
            pa, ldperm = _mat_addr_ld(perm, np.int32, torch.int32 if torch is not None else None)
    xa, ldx = _f64(X)
    pra, ldp = _f64(Pred)
    ya, ldy = _f64(Y)
    ctx = ctx or default_context((X.device.index or 0) if dev else 0)
    sums = np.empty((p + 1, q, 6))
    if dev:
        torch.cuda.current_stream(X.device).synchronize()
    ctx.check(_lib.load().jch_perm_score_sums(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, xa, n, p, ldx, ra, m, pra, ldp, ya, q, ldy, B.ctypes.data, p, pa,
                                              ldperm, seed, sums.ctypes.data))
    return sums


# ---------------------------------------------------------------------------------- the split both functions share
def _nval(psamp, n) -> int:
    nval = int(round(float(psamp) * n))   # half to even, as Julia's `round` (src/viperm.jl:81)
    if not 1 <= nval < n:
        raise ValueError(f"psamp = {psamp} leaves {nval} of {n} rows for the test set: at least one row on each side")
    return nval


def _count_arg(name, v) -> int:
    if isinstance(v, bool) or int(v) != v or int(v) < 1:
        raise ValueError(f"{name} = {v} must be an integer >= 1")
    return int(v)


def _check_xy(X, Y):
    X, Y = ensure_mat(X), ensure_mat(Y)
    if _is_torch(X) != _is_torch(Y):
        raise TypeError("X and Y must both be host arrays or both device tensors")
    if _is_torch(X) and not (X.is_cuda and Y.is_cuda):
        raise TypeError("torch inputs must live on the GPU (host data: pass numpy arrays)")
    if X.ndim != 2 or Y.ndim != 2:
        raise ValueError("X and Y must be matrices (or vectors)")
    if Y.shape[0] != X.shape[0]:
        raise ValueError(f"DimensionMismatch: X has {X.shape[0]} rows, Y has {Y.shape[0]}")
    if X.shape[0] < 2 or X.shape[1] < 1 or Y.shape[1] < 1:
        raise ValueError("at least two rows and one column each")
    return X, Y


def _splits(n, nval, nrep, seed, s):
    """Per replication (held-out rows, 64-bit permutation seed), both from numpy.random.default_rng(seed): the `nrep` seeds first, then the
    rows replication by replication.  `s` (a list of `nrep` index arrays) pins the rows and leaves the seeds what they were."""
    if s is not None:
        s = [np.asarray(si, dtype=np.int64).reshape(-1) for si in s]
        if len(s) != nrep:
            raise ValueError(f"s has {len(s)} index arrays for {nrep} replications")
        for si in s:
            if si.size < 1 or si.size >= n or si.min() < 0 or si.max() >= n or np.unique(si).size != si.size:
                raise ValueError("every entry of s: between 1 and n - 1 distinct row numbers in 0 .. n - 1")
    rng = np.random.default_rng(seed)
    pseeds = rng.integers(0, 2 ** 64, size=nrep, dtype=np.uint64)
    return [(s[i] if s is not None else np.sort(rng.choice(n, size=nval, replace=False)).astype(np.int64), int(pseeds[i])) for i in range(nrep)]


def _held(n, rows, like):
    """(held, w): the 0/1 vector of the held-out rows and its complement, made where X lives."""
    if _is_torch(like):
        held = torch.zeros(n, dtype=torch.float64, device=like.device)
        held[torch.as_tensor(rows, dtype=torch.int64).to(like.device)] = 1.0
    else:
        held = np.zeros(n)
        held[rows] = 1.0
    return held, 1.0 - held


def _take_rows(A, rows):
    """A[rows, :] as a column-major copy."""
    if _is_torch(A):
        return _as_colmajor_copy(A[torch.as_tensor(rows, dtype=torch.int64).to(A.device)])
    return np.asfortranarray(A[rows])


def _split_copies(X, Y, rows):
    keep = np.setdiff1d(np.arange(X.shape[0]), rows)   # rmrow (src/utility.jl): the other rows in their order
    return _take_rows(X, keep), _take_rows(Y, keep), _take_rows(X, rows), _take_rows(Y, rows)


def _pred_of(fm, X, ctx):
    pred = predict(fm, X, ctx=ctx)
    return getattr(pred, "pred", pred)


def _score_row(score, pred, Y):
    v = score(pred, Y)
    return np.asarray(v.cpu().numpy() if _is_torch(v) else v, dtype=np.float64).reshape(-1)


def _full_B(fm, p):
    """`coef(fm).B` in the units of the raw X, p x q: a Covselr model's coefficients sit in the rows of its selected columns."""
    B = np.asarray(coef(fm)[0], dtype=np.float64)
    if type(fm).__name__ == "Covselr":
        full = np.zeros((p, B.shape[1]))
        full[fm.sel["sel"]] = B
        return full
    return B


# ---------------------------------------------------------------------------------- viperm
def _loop_replication(X, Y, rows, pseed, score, fun, ctx, kwargs, cols=None):
    """One replication of src/viperm.jl:90-106 taken literally, with the library's permutations: (p or len(cols)) x q differences."""
    Xcal, Ycal, Xval, Yval = _split_copies(X, Y, rows)
    m, p = Xval.shape
    fm = fun(Xcal, Ycal, ctx=ctx, **kwargs)
    score0 = _score_row(score, _pred_of(fm, Xval, ctx), Yval)
    perm = perm_fill(m, p, pseed, ctx=ctx)
    cols = range(p) if cols is None else cols
    out = np.empty((len(cols), score0.size))
    for o, j in enumerate(cols):
        pj = perm[:, j].astype(np.int64)
        col = Xval[:, j].clone() if _is_torch(Xval) else Xval[:, j].copy()
        Xval[:, j] = col[torch.as_tensor(pj).to(Xval.device)] if _is_torch(Xval) else col[pj]
        out[o] = _score_row(score, _pred_of(fm, Xval, ctx), Yval) - score0
        Xval[:, j] = col
    return out


def _fast_replication(X, Y, rows, pseed, name, fun, ctx, kwargs, same_x):
    """One replication by the rank-one route: one fit, one predict over X, one jch_perm_score_sums.  p x q differences."""
    n, p = X.shape
    if fun in _WEIGHT_FUNS:
        _, w = _held(n, rows, X)
        extra = dict(reuse_x=same_x) if fun in _REUSE_FUNS else {}
        fm = fun(X, Y, w, ctx=ctx, **extra, **kwargs)
    else:   # no weights to give: the training rows are gathered
        keep = np.setdiff1d(np.arange(n), rows)
        fm = fun(_take_rows(X, keep), _take_rows(Y, keep), ctx=ctx, **kwargs)
    pred = _pred_of(fm, X, ctx)
    S = perm_score_sums(X, pred, Y, _full_B(fm, p), rows=rows, seed=pseed, ctx=ctx)
    return _score_from_sums(name, S[:p]) - _score_from_sums(name, S[p:])


def viperm(X, Y, *, perm: int = 50, psamp: float = 1 / 3, score=rmsep, fun, seed=None, s=None, route: str = "auto", ctx: Optional[Context] = None,
           **kwargs) -> Viperm:
    """`viperm(X, Y; perm = 50, psamp = 1/3, score = rmsep, fun, kwargs...)` — src/viperm.jl:74-110.  nval = round(psamp n) rows are held
    out per replication, drawn from numpy.random.default_rng(seed) together with one 64-bit permutation seed (the reference's own stream is
    not reproduced); `s`, a list of `perm` index arrays, pins the rows.  Column j of a replication is shuffled by the permutation
    jch_perm_fill gives for (that seed, j) on either route.
    route = "fast": `fun` one of plskern / plsnipals / plssimp / plsrosa / plswold / pcr / covselr and `score` one of msep / rmsep / ssr /
    bias / r2 / cor2 — one fit with weight 0 on the held-out rows (X is never copied; covselr, which takes no weights, gets gathered rows),
    one predict over X and one jch_perm_score_sums per replication.  route = "loop": the reference's loop.  "auto": fast where it applies."""
    if route not in ("auto", "fast", "loop"):
        raise ValueError(f'route = {route!r}: "auto", "fast" or "loop"')
    nrep = _count_arg("perm", perm)
    X, Y = _check_xy(X, Y)
    n, p = X.shape
    q = Y.shape[1]
    nval = _nval(psamp, n)
    if not callable(fun) or not callable(score):
        raise TypeError("fun and score must be callable")
    name = getattr(score, "_jch_name", None)
    fast_ok = name is not None and any(fun is f for f in _FAST_FUNS)
    if route == "fast" and not fast_ok:
        raise ValueError('route = "fast" needs fun in plskern / plsnipals / plssimp / plsrosa / plswold / pcr / covselr and a named score')
    splits = _splits(n, nval, nrep, seed, s)
    fast = fast_ok and route != "loop"
    if fast:
        X, Y = _colmajor_f64(X), _colmajor_f64(Y)
    ctx = ctx or default_context((X.device.index or 0) if _is_torch(X) else 0)
    res = np.empty((p, q, nrep))
    for i, (rows, pseed) in enumerate(splits):
        if fast:
            res[:, :, i] = _fast_replication(X, Y, rows, pseed, name, fun, ctx, kwargs, i > 0)
        else:
            res[:, :, i] = _loop_replication(X, Y, rows, pseed, score, fun, ctx, kwargs)
    return Viperm(res.mean(axis=2), res)


# ---------------------------------------------------------------------------------- isel
def isel_intervals(p: int, nint: int) -> np.ndarray:
    """src/isel.jl:84-87: nint x 3 (first column, last column, middle column), 1-based as in the reference; `round` is half to even."""
    z = np.rint(np.linspace(1, p + 1, nint + 1))
    lo, up = z[:nint], z[1:] - 1
    return np.stack([lo, up, np.rint((lo + up) / 2)], axis=1).astype(np.int64)


def isel(X, Y, wl=None, *, rep: int = 1, nint: int = 5, psamp: float = 1 / 3, score=rmsep, fun, seed=None, s=None, ctx: Optional[Context] = None,
         **kwargs) -> Isel:
    """`isel(X, Y, wl = 1:nco(X); rep = 1, nint = 5, psamp = 1/3, score = rmsep, fun, kwargs...)` — src/isel.jl:76-129 (wl = None: the
    0-based column numbers).  The split works as in `viperm`.  Where `fun` takes weights and `score` is a named one, a replication is one fit
    with weight 0 on the held-out rows per column range, on a VIEW of the column-major X (same leading dimension, no copy), and the scores come
    from jch_score_sums with the held-out mask; otherwise the training and test rows are gathered once per replication."""
    nrep, nint = _count_arg("rep", rep), _count_arg("nint", nint)
    X, Y = _check_xy(X, Y)
    n, p = X.shape
    q = Y.shape[1]
    if nint > p:
        raise ValueError(f"nint = {nint} intervals for {p} columns")
    nval = _nval(psamp, n)
    if not callable(fun) or not callable(score):
        raise TypeError("fun and score must be callable")
    wl = np.arange(p) if wl is None else np.asarray(wl).reshape(-1)
    if wl.shape[0] != p:
        raise ValueError(f"DimensionMismatch: wl has {wl.shape[0]} entries, X has {p} columns")
    ints = isel_intervals(p, nint) - 1
    splits = _splits(n, nval, nrep, seed, s)
    name = getattr(score, "_jch_name", None)
    masked = name is not None and any(fun is f for f in _WEIGHT_FUNS)
    if masked:
        X, Y = _colmajor_f64(X), _colmajor_f64(Y)
    ctx = ctx or default_context((X.device.index or 0) if _is_torch(X) else 0)
    res_rep, res0_rep = np.zeros((nint, q, nrep)), np.zeros((1, q, nrep))
    for i, (rows, _) in enumerate(splits):
        if masked:
            held, w = _held(n, rows, X)

            def one(lo, up):
                Xu = X[:, lo:up + 1]
                fm = fun(Xu, Y, w, ctx=ctx, **kwargs)
                return _score_from_sums(name, _score_sums(_pred_of(fm, Xu, ctx), Y, held, ctx))[0]
        else:
            Xcal, Ycal, Xval, Yval = _split_copies(X, Y, rows)

            def one(lo, up):
                fm = fun(Xcal[:, lo:up + 1], Ycal, ctx=ctx, **kwargs)
                return _score_row(score, _pred_of(fm, Xval[:, lo:up + 1], ctx), Yval)
        res0_rep[0, :, i] = one(0, p - 1)
        for j in range(nint):
            res_rep[j, :, i] = one(int(ints[j, 0]), int(ints[j, 1]))
    res = dict(lo=wl[ints[:, 0]], up=wl[ints[:, 1]], mid=wl[ints[:, 2]])
    zres, zres0 = res_rep.mean(axis=2), res0_rep.mean(axis=2)
    res0 = {}
    for k in range(q):
        res[f"y{k + 1}"] = zres[:, k]
        res0[f"y{k + 1}"] = zres0[:, k]
    return Isel(res, res0, res_rep, res0_rep, ints)
