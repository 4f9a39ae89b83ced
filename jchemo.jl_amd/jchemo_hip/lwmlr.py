"""Locally weighted multiple linear regression and discrimination — host-side mirror of the reference's src/lwmlr.jl, src/lwmlr_s.jl,
src/lwmlrda.jl and src/lwmlrda_s.jl (through src/locw.jl, src/mlr.jl and src/mlrda.jl) over jch_knn_search and jch_knn_wls
(include/jchemo_hip.h).

A predict is one neighbour search on a handle cached per model (the space of `getknn`: the model's coordinates, whitened for "mahal") and one
jch_knn_wls: per query a weighted Householder least-squares fit of the neighbours' responses on their UN-whitened coordinates, as
`locw(object.X, ...)` does, and the prediction of the query's row.  numpy in gives numpy out; device tensors keep the m-sized results on the device.
Neighbour lists are int32 and 0-based, m x k row-major.

Rank-deficient neighbourhoods (k <= d, collinear coordinates) give NaN rows and one RuntimeWarning with their count — the reference returns
LAPACK's minimum-norm solution there.  The discrimination models give such a query the weighted-vote class of jch_knn_vote.

`samp = "random"` draws from `numpy.random.default_rng(seed)`: Julia's `sample` draws from a stream that cannot be matched.  `psamp = 1` takes every
row, in order, whatever `samp` is."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context
from .knn import (KnnPred, _check_knn_args, _ctx_for, _done, _dummy_like, _empty, _labels, _lists_like, _loc_sync, _prepared, _ptr, _rows, knn_prepare,
                  knn_search, knn_vote)
from .occ import _colmajor_x
from .pca import Pca, pca_transform, pcasvd
from .plsr import (Dkplsr, Plsrda, _addr_ld, _is_torch, _knn_train_space, colmajor_empty, dkplsr, dkplsr_transform, ensure_mat, plskern, plsrda,
                   transform)
from .samp import sampcla, sampsys

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

WLS_LDS_MAX = 150 * 1024   # csrc/lwmlr.hip: the largest slab that lives in LDS


def knn_wls_lds_bytes(k: int, d: int, q: int) -> int:
    """Bytes of one workgroup's slab and vectors in jch_knn_wls (csrc/lwmlr.hip `wls_slab_doubles`): in LDS up to WLS_LDS_MAX, else in the workspace."""
    k, d, q = int(k), int(d), int(q)
    return 8 * ((d + q) * (k | 1) + 2 * k + (d + q) + 2 * d + (k + 1) // 2)


@dataclass
class Lwmlr:
    """src/lwmlr.jl:1-9 — same fields."""
    X: object
    Y: object
    metric: str
    h: float
    k: int
    tol: float
    verbose: bool


@dataclass
class LwmlrS:
    """src/lwmlr_s.jl:1-10 — same fields (T: the scores of all training rows, fm: the global reduction)."""
    T: object
    Y: object
    fm: object
    metric: str
    h: float
    k: int
    tol: float
    verbose: bool


@dataclass
class Lwmlrda:
    """src/lwmlrda.jl:1-9 — same fields (y: the labels as given)."""
    X: object
    y: object
    metric: str
    h: float
    k: int
    tol: float
    verbose: bool


@dataclass
class LwmlrdaS:
    """src/lwmlrda_s.jl:1-10 — same fields."""
    T: object
    y: object
    fm: object
    metric: str
    h: float
    k: int
    tol: float
    verbose: bool


# ---------------------------------------------------------------------------------- the primitive
def knn_wls(X, Y, Xq, ind, w, *, info: bool = False, ctx: Optional[Context] = None):
    """jch_knn_wls: pred (m x q, where X lives) — per query the weighted least-squares fit (Householder QR) of Y[ind_i, :] on X[ind_i, :] with the
    weights w_i / sum(w_i), evaluated at Xq[i, :].  With `info=True` also the m int32 flags: 0 fitted, 1 rank-deficient (the row is NaN), 2 the
    constant-response shortcut of src/locw.jl:33-34 (q == 1)."""
    X = _colmajor_x(X); Y = _colmajor_x(Y); Xq = _colmajor_x(Xq)
    dev = _is_torch(X)
    if _is_torch(Y) != dev or _is_torch(Xq) != dev:
        raise TypeError("X, Y and Xq must all be host arrays or all device tensors")
    n, d = X.shape
    q = Y.shape[1]
    if Y.shape[0] != n:
        raise ValueError(f"DimensionMismatch: X has {n} rows, Y has {Y.shape[0]}")
    if Xq.shape[1] != d:
        raise ValueError(f"DimensionMismatch: X has {d} columns, Xq has {Xq.shape[1]}")
    ind, w = _lists_like(ind, w, X)
    m, k = ind.shape
    if w is None or m != Xq.shape[0]:
        raise ValueError(f"ind and w must be {Xq.shape[0]} x k arrays")
    if min(n, d, q, m, k) < 1:
        raise ValueError("knn_wls: n, d, q, m and k must be >= 1")
    ctx = _ctx_for(X, ctx)
    pred = colmajor_empty(m, q, X.device) if dev else np.empty((m, q), order="F")
    flags = _empty((m,), np.int32, X) if info else None
    xa, ldx = _addr_ld(X); ya, ldy = _addr_ld(Y); qa, ldq = _addr_ld(Xq)
    ctx.check(_lib.load().jch_knn_wls(ctx._h, _loc_sync(X), xa, n, d, ldx, ya, q, ldy, qa, m, ldq, _ptr(ind), _ptr(w), k, _ptr(pred), _ptr(flags)))
    _done(ctx, dev)
    return (pred, flags) if info else pred


# ---------------------------------------------------------------------------------- the models
_REDUC = ("pca", "pls", "dkpls")


def _check_rows(X, Y, what="Y"):
    if Y.shape[0] != X.shape[0]:
        raise ValueError(f"DimensionMismatch: X has {X.shape[0]} rows, {what} has {Y.shape[0]}")
    if _is_torch(X) and not X.is_cuda:
        raise TypeError("torch inputs must live on the GPU (host data: pass numpy arrays)")


def lwmlr(X, Y, *, metric: str = "eucl", h, k, tol: float = 1e-4, verbose: bool = False, ctx: Optional[Context] = None) -> Lwmlr:
    """`lwmlr(X, Y; metric = "eucl", h, k, tol = 1e-4, verbose = false)` — src/lwmlr.jl:64-70: stores the data.  (`ctx` is accepted for symmetry; the
    constructor does no device work.)"""
    X = ensure_mat(X); Y = ensure_mat(Y)
    _check_knn_args(metric, h, k, tol)
    _check_rows(X, Y)
    if _is_torch(X) != _is_torch(Y):
        raise TypeError("X and Y must both be host arrays or both device tensors")
    return Lwmlr(X, Y, metric, h, int(k), tol, bool(verbose))


def lwmlrda(X, y, *, metric: str = "eucl", h, k, tol: float = 1e-4, verbose: bool = False, ctx: Optional[Context] = None) -> Lwmlrda:
    """`lwmlrda(X, y; metric = "eucl", h, k, tol = 1e-4, verbose = false)` — src/lwmlrda.jl:58-64: stores the data."""
    X = ensure_mat(X)
    _check_knn_args(metric, h, k, tol)
    _check_rows(X, _labels(y), "y")
    return Lwmlrda(X, y, metric, h, int(k), tol, bool(verbose))


def _check_s_args(reduc, samp, allowed, psamp, nlv):
    if reduc not in _REDUC:
        raise ValueError(f"reduc must be one of {_REDUC}, got {reduc!r}")
    if samp not in allowed:
        raise ValueError(f"samp must be one of {allowed}, got {samp!r}")
    if not 0.0 < float(psamp) <= 1.0:
        raise ValueError(f"psamp = {psamp} must be in (0, 1]")
    if isinstance(nlv, bool) or int(nlv) != nlv or int(nlv) < 1:
        raise ValueError(f"nlv = {nlv} must be an integer >= 1")


def _reduce(X, Yfit, yv, s, nlv, reduc, gamma, scal, ctx):
    """The global reduction fitted on the rows s (None: all rows), and the scores of ALL rows (src/lwmlr_s.jl:84-95)."""
    zX = X if s is None else _rows(X, s)
    if reduc == "pca":
        fm = pcasvd(zX, nlv=nlv, scal=scal, ctx=ctx)
    elif yv is not None and reduc == "pls":
        fm = plsrda(zX, yv if s is None else yv[s], nlv=nlv, scal=scal, ctx=ctx)
    else:
        zY = Yfit if s is None else _rows(Yfit, s)
        fm = plskern(zX, zY, nlv=nlv, scal=scal, ctx=ctx) if reduc == "pls" else dkplsr(zX, zY, nlv=nlv, kern="krbf", gamma=gamma, scal=scal, ctx=ctx)
    return fm, _transform(fm, X, ctx)


def _transform(fm, X, ctx):
    if isinstance(fm, Pca):
        return pca_transform(fm, X, ctx=ctx)
    if isinstance(fm, Dkplsr):
        return dkplsr_transform(fm, X, ctx=ctx)
    if isinstance(fm, Plsrda):
        return transform(fm.fm, X, ctx=ctx)
    return transform(fm, X, ctx=ctx)


def lwmlr_s(X, Y, *, nlv, reduc: str = "pls", metric: str = "eucl", h, k, gamma=1, psamp=1, samp: str = "sys", tol: float = 1e-4, scal: bool = False,
            verbose: bool = False, seed=None, ctx: Optional[Context] = None) -> LwmlrS:
    """`lwmlr_s(X, Y; nlv, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "sys", tol = 1e-4, scal = false, verbose = false)` —
    src/lwmlr_s.jl:73-98: a global reduction (`pcasvd`, `plskern`, or `dkplsr` with `krbf`) fitted on a sample of round(psamp n) rows (`sampsys` on
    the row sums of Y, or `seed`ed random), then LWMLR on the scores of all rows.  reduc = "pca" is the LWR of Naes et al."""
    X = _colmajor_x(X); Y = _colmajor_x(Y)
    _check_knn_args(metric, h, k, tol)
    _check_s_args(reduc, samp, ("sys", "random"), psamp, nlv)
    _check_rows(X, Y)
    if _is_torch(X) != _is_torch(Y):
        raise TypeError("X and Y must both be host arrays or both device tensors")
    n = X.shape[0]
    ms = int(round(psamp * n))
    s = None
    if ms < n:
        if samp == "sys":
            rs = Y.sum(dim=1).cpu().numpy() if _is_torch(Y) else np.asarray(Y).sum(axis=1)
            s = np.asarray(sampsys(rs, ms).train, dtype=np.int64)
        else:
            s = np.random.default_rng(seed).choice(n, size=ms, replace=False)
    fm, T = _reduce(X, Y, None, s, int(nlv), reduc, gamma, scal, ctx)
    return LwmlrS(T, Y, fm, metric, h, int(k), tol, bool(verbose))


def lwmlrda_s(X, y, *, nlv, reduc: str = "pls", metric: str = "eucl", h, k, gamma=1, psamp=1, samp: str = "cla", tol: float = 1e-4,
              scal: bool = False, verbose: bool = False, seed=None, ctx: Optional[Context] = None) -> LwmlrdaS:
    """`lwmlrda_s(X, y; nlv, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "cla", tol = 1e-4, scal = false, verbose = false)` —
    src/lwmlrda_s.jl:77-106.  reduc = "pls" is `plsrda`; "dkpls" is `dkplsr` on `dummy(y)`, which is what the reference's `dkplsrda` fits.
    samp = "cla": `sampcla` with round(round(psamp n) / nlev) rows per class (random within a class, from `seed`)."""
    X = _colmajor_x(X)
    _check_knn_args(metric, h, k, tol)
    _check_s_args(reduc, samp, ("cla", "random"), psamp, nlv)
    yv = _labels(y)
    _check_rows(X, yv, "y")
    n = X.shape[0]
    ms = int(round(psamp * n))
    s = None
    if ms < n:
        if samp == "cla":
            nlev = np.unique(yv).shape[0]
            s = np.asarray(sampcla(yv, k=max(int(round(ms / nlev)), 1), seed=seed).train, dtype=np.int64)
        else:
            s = np.random.default_rng(seed).choice(n, size=ms, replace=False)
    Yd = None if reduc != "dkpls" else _dummy_like(yv, X)
    fm, T = _reduce(X, Yd, yv, s, int(nlv), reduc, gamma, scal, ctx)
    return LwmlrdaS(T, y, fm, metric, h, int(k), tol, bool(verbose))


# ---------------------------------------------------------------------------------- predict
def _coords(obj):
    return obj.T if isinstance(obj, (LwmlrS, LwmlrdaS)) else obj.X


def _lw_prepared(obj, ctx, dev):
    """The handle on the search space of the model (`getknn(object.X, ...)`: its coordinates, whitened for "mahal") and the query map into it."""
    Z = _coords(obj)
    key = (id(ctx), ctx._h.value, dev, id(Z), obj.metric)

    def build():
        Zt, qmap, _ = _knn_train_space(SimpleNamespace(X=Z, Y=None, fm=None, metric=obj.metric, scal=False), ctx)
        return {"handle": knn_prepare(Zt, ctx), "qmap": qmap, "n": Zt.shape[0]}
    return _prepared(obj, key, build)


def _lw_search(obj, X, ctx):
    """The queries in the model's coordinates, the search, and the cached state."""
    from .knn import _check_metric
    _check_metric(obj.metric)
    X = _colmajor_x(X)
    Z = _coords(obj)
    dev = _is_torch(X)
    if dev != _is_torch(Z):
        raise TypeError("training data and queries must both be host arrays or both device tensors")
    fm = getattr(obj, "fm", None)
    if fm is None and X.shape[1] != Z.shape[1]:
        raise ValueError(f"DimensionMismatch: X has {X.shape[1]} columns, the model has {Z.shape[1]}")
    ctx = _ctx_for(X, ctx)
    Q = X if fm is None else _transform(fm, X, ctx)
    st = _lw_prepared(obj, ctx, dev)
    res = knn_search(st["handle"], st["n"], st["qmap"](Q), obj.k, h=obj.h, tol=obj.tol, want=("ind", "dist", "w"), ctx=ctx)
    return Q, res, st, ctx


def _warn_deficient(info, who):
    flags = info.cpu().numpy() if _is_torch(info) else info
    bad = flags == 1
    if bad.any():
        warnings.warn(f"{who}: {int(bad.sum())} of {flags.shape[0]} neighbourhoods are rank-deficient; their predictions are NaN", RuntimeWarning, stacklevel=3)
    return bad


def _verbose(obj, m):
    if getattr(obj, "verbose", False):                            # src/locw.jl:27,45
        print("".join(f"{i} " for i in range(1, m + 1)))


def _lw_reg_predict(obj, X, ctx, who):
    Q, res, st, ctx = _lw_search(obj, X, ctx)
    pred, info = knn_wls(_coords(obj), obj.Y, Q, res["ind"], res["w"], info=True, ctx=ctx)
    _warn_deficient(info, who)
    _verbose(obj, Q.shape[0])
    return KnnPred(pred, res["ind"], res["dist"], res["w"])


def _lw_da_predict(obj, X, ctx, who):
    Q, res, st, ctx = _lw_search(obj, X, ctx)
    yv = _labels(obj.y)
    if "Yd" not in st:
        lev = np.unique(yv)
        codes = np.searchsorted(lev, yv).astype(np.int32)
        st["lev"] = lev
        st["Yd"] = _dummy_like(yv, Q)
        st["cls"] = torch.as_tensor(codes, device=Q.device) if _is_torch(Q) else codes
    post, info = knn_wls(_coords(obj), st["Yd"], Q, res["ind"], res["w"], info=True, ctx=ctx)
    bad = _warn_deficient(info, who)
    post = post.cpu().numpy() if _is_torch(post) else post
    code = np.argmax(np.where(np.isnan(post), -np.inf, post), axis=1)          # the first maximum in sorted-level order (`argmax`, src/mlrda.jl:51)
    if bad.any():                                                              # no fit there: the weighted vote of knnda
        vote = knn_vote(st["cls"], len(st["lev"]), res["ind"], res["w"], ctx=ctx)
        vote = vote.cpu().numpy() if _is_torch(vote) else vote
        code = np.where(bad, vote, code)
    _verbose(obj, Q.shape[0])
    return KnnPred(np.asarray(st["lev"])[code].reshape(-1, 1), res["ind"], res["dist"], res["w"])


def lwmlr_predict(obj: Lwmlr, X, *, ctx: Optional[Context] = None) -> KnnPred:
    """`predict(object::Lwmlr, X)` — src/lwmlr.jl:78-97: one jch_knn_search (neighbours, distances, `wdist` weights clamped to tol), one jch_knn_wls."""
    return _lw_reg_predict(obj, X, ctx, "lwmlr_predict")


def lwmlr_s_predict(obj: LwmlrS, X, *, ctx: Optional[Context] = None) -> KnnPred:
    """`predict(object::LwmlrS, X)` — src/lwmlr_s.jl:106-125: the scores of X under the global reduction, then as `lwmlr_predict` on the scores."""
    return _lw_reg_predict(obj, X, ctx, "lwmlr_s_predict")


def lwmlrda_predict(obj: Lwmlrda, X, *, ctx: Optional[Context] = None) -> KnnPred:
    """`predict(object::Lwmlrda, X)` — src/lwmlrda.jl:72-91: the search, jch_knn_wls on the GLOBAL dummy table, the row argmax on the host (the
    reference's local `mlrda` on the local levels gives the same label: DESIGN.md §23).  pred: an m x 1 host array of labels; a rank-deficient
    neighbourhood gets the weighted-vote class of jch_knn_vote."""
    return _lw_da_predict(obj, X, ctx, "lwmlrda_predict")


def lwmlrda_s_predict(obj: LwmlrdaS, X, *, ctx: Optional[Context] = None) -> KnnPred:
    """`predict(object::LwmlrdaS, X)` — src/lwmlrda_s.jl:114-133: as `lwmlrda_predict` on the scores of the global reduction."""
    return _lw_da_predict(obj, X, ctx, "lwmlrda_s_predict")
