"""Locally weighted PLS discrimination, and the locally weighted PLS models on global scores — host-side mirror of the reference's src/lwplsrda.jl,
src/lwplslda.jl, src/lwplsqda.jl, src/lwplsr_s.jl and src/lwplsrda_s.jl (through src/locwlv.jl, src/plsrda.jl, src/plslda.jl, src/plsqda.jl) over
jch_lwplsda_predict_prepared and jch_knn_gda (include/jchemo_hip.h).

A predict is ONE library call on the handle cached per model (`Lwplsr`'s handle, built on the dummy table of the labels): the neighbour search, the
`wdist` weights, one weighted `plskern` per query on the dummy columns and, for the Gaussian models, the nested discriminants of the local scores
for the whole nlv range from one factorisation per covariance.  Results are `LwplsrPred`-shaped with two more fields: `pred` is an m x 1 array of
labels (a list of them for several nlv), `posterior` the m x nlev posteriors in sorted-level order (kind "rda": the dummy predictions), `info` the
m (x le) flags: 0 fitted, 1 unanimous neighbourhood (the label is that class, the posterior one-hot), 2 a covariance not positive definite in these
score columns (label: the weighted vote of the neighbourhood, posterior NaN, one RuntimeWarning per call), 3 a non-finite local fit (posterior NaN,
the first local level).  Neighbour lists are int32 and 0-based, m x k row-major."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context
from .knn import _check_knn_args, _dummy_like, _labels, _lists_like, _ptr, _rows
from .lwmlr import _check_rows, _check_s_args, _reduce, _transform
from .occ import _colmajor_x
from .plsr import (Lwplsr, LwplsrPred, _addr_ld, _as_colmajor_copy, _is_torch, _lwplsr_prepared, _np, default_context, ensure_mat, lwplsr_predict,
                   plskern)
from .samp import sampcla, sampsys

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

GDA_LDS_MAX = 150 * 1024   # csrc/lwplsda.hip: the largest slab that lives in LDS
_KIND = {"rda": 0, "lda": 1, "qda": 2}
_PRIOR = {"unif": 0, "prop": 1}


def knn_gda_lds_bytes(k: int, a: int, nlev: int) -> int:
    """Bytes of one workgroup's slab in jch_knn_gda (csrc/lwplsda.hip `jch_knn_gda_slab_doubles`, rounded to 256 B): in LDS up to GDA_LDS_MAX, else in
    the workspace."""
    k, a, nlev = int(k), int(a), int(nlev)
    d = k * a + a * (a | 1) + 2 * a + (nlev + 1) * a + 4 * a + a + (nlev + k + 1) // 2 + 2
    return 8 * ((d + 31) // 32 * 32)


def locw_pspace_lds_bytes(k: int, p: int, nlev: int) -> int:
    """Bytes of dynamic LDS of the p-space local-fit kernel for k neighbours, p columns and nlev responses (csrc/lwplsr.hip `locw_pspace_lds`).  With
    p <= 2048, nlev <= 16 and nlv <= 48, a predict takes that kernel — the one that hands out its local scores — while this is <= 150 KiB, and one fit
    per query beyond."""
    k, ldr = int(k), (int(p) + 1) & ~1
    KC = 1 if ldr <= 128 else 2 if ldr <= 256 else 4 if ldr <= 512 else 8 if ldr <= 1024 else 16
    Q = 1 if nlev <= 1 else 2 if nlev <= 2 else 4 if nlev <= 4 else 8 if nlev <= 8 else 16
    return 8 * ((1 + Q) * k + (5 + Q) * ldr + 4 * KC * 128 + 128 + 4 * Q + 16 + 5 * Q * (Q + 2) + 2 * (Q + 2) + 8 + 4 * (Q * (Q + 1) // 2 + Q + 1)) + 4 * k + 64


@dataclass
class Lwplsrda:
    """src/lwplsrda.jl:1-14 — same fields."""
    X: object
    y: object
    fm: object
    metric: str
    h: float
    k: int
    nlv: int
    tol: float
    scal: bool
    verbose: bool
    lev: object
    ni: object


@dataclass
class LwplsLda:
    """src/lwplslda.jl:1-15 — same fields."""
    X: object
    y: object
    fm: object
    metric: str
    h: float
    k: int
    nlv: int
    prior: str
    tol: float
    scal: bool
    verbose: bool
    lev: object
    ni: object


@dataclass
class LwplsQda(LwplsLda):
    """src/lwplsqda.jl:1-15 — same fields."""


@dataclass
class LwplsrS:
    """src/lwplsr_s.jl:1-12 — same fields (T: the scores of all training rows, fm: the global reduction)."""
    T: object
    Y: object
    fm: object
    metric: str
    h: float
    k: int
    nlv: int
    tol: float
    scal: bool
    verbose: bool


@dataclass
class LwplsrdaS:
    """src/lwplsrda_s.jl:1-12 — same fields."""
    T: object
    y: object
    fm: object
    metric: str
    h: float
    k: int
    nlv: int
    tol: float
    scal: bool
    verbose: bool


@dataclass
class LwplsdaPred(LwplsrPred):
    """`LwplsrPred` (pred, listnn, listd, listw) with the posteriors and the per-(query, nlv) flags."""
    posterior: object = None
    info: object = None


# ---------------------------------------------------------------------------------- the primitive
def knn_gda(T, tq, cls_nb, nlev: int, *, kind: str = "lda", prior: str = "unif", nlv=None, ctx: Optional[Context] = None):
    """jch_knn_gda: T (m x k x a_hi scores of the neighbours), tq (m x a_hi, the queries' scores), cls_nb (m x k int32 codes in 0 .. nlev - 1), all
    C-contiguous host arrays or device tensors -> (post m x le x nlev, code m x le int32, info m x le int32) where the inputs live.  nlv: an int or a
    collection, the models min .. max within 1 .. a_hi (default a_hi)."""
    if kind not in ("lda", "qda"):
        raise ValueError(f"kind must be 'lda' or 'qda', got {kind!r}")
    if prior not in _PRIOR:
        raise ValueError(f"prior must be 'unif' or 'prop', got {prior!r}")
    dev = _is_torch(T)
    if _is_torch(tq) != dev or _is_torch(cls_nb) != dev:
        raise TypeError("T, tq and cls_nb must all be host arrays or all device tensors")
    if T.ndim != 3 or tq.ndim != 2 or cls_nb.ndim != 2:
        raise ValueError("knn_gda: T must be m x k x a, tq m x a and cls_nb m x k")
    m, k, a_hi = (int(v) for v in T.shape)
    if tuple(tq.shape) != (m, a_hi) or tuple(cls_nb.shape) != (m, k):
        raise ValueError(f"DimensionMismatch: T is {m} x {k} x {a_hi}, tq {tuple(tq.shape)}, cls_nb {tuple(cls_nb.shape)}")
    if min(m, k, a_hi, int(nlev)) < 1:
        raise ValueError("knn_gda: m, k, a and nlev must be >= 1")
    vals = np.atleast_1d(np.asarray(a_hi if nlv is None else nlv))
    lo, hi = int(vals.min()), int(vals.max())
    if lo < 1 or hi > a_hi:
        raise ValueError(f"nlv = {lo} .. {hi} must lie in 1 .. {a_hi}")
    le = hi - lo + 1
    if dev:
        if not T.is_cuda:
            raise TypeError("torch inputs must live on the GPU (host data: pass numpy arrays)")
        T = T.contiguous().double(); tq = tq.contiguous().double(); cls_nb = cls_nb.contiguous().to(torch.int32)
        ctx = ctx or default_context(T.device.index or 0)
        post = torch.empty((m, le, int(nlev)), dtype=torch.float64, device=T.device)
        code = torch.empty((m, le), dtype=torch.int32, device=T.device)
        info = torch.empty((m, le), dtype=torch.int32, device=T.device)
        torch.cuda.current_stream(T.device).synchronize()
    else:
        T = np.ascontiguousarray(T, dtype=np.float64); tq = np.ascontiguousarray(tq, dtype=np.float64); cls_nb = np.ascontiguousarray(cls_nb, dtype=np.int32)
        ctx = ctx or default_context(0)
        post = np.empty((m, le, int(nlev))); code = np.empty((m, le), dtype=np.int32); info = np.empty((m, le), dtype=np.int32)
    ctx.check(_lib.load().jch_knn_gda(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, _ptr(T), m, k, a_hi, _ptr(tq), _ptr(cls_nb), int(nlev), _KIND[kind],
                                      _PRIOR[prior], lo, hi, _ptr(post), _ptr(code), _ptr(info)))
    if dev:
        ctx.synchronize()
    return post, code, info


# ---------------------------------------------------------------------------------- the models
def _check_da(X, y, metric, h, k, tol, nlv, nlvdis, prior="unif"):
    _check_knn_args(metric, h, k, tol)
    if prior not in _PRIOR:
        raise ValueError(f"prior must be 'unif' or 'prop', got {prior!r}")
    for nm, v, lo in (("nlv", nlv, 0), ("nlvdis", nlvdis, 0)):
        if isinstance(v, bool) or int(v) != v or int(v) < lo:
            raise ValueError(f"{nm} = {v} must be an integer >= {lo}")
    yv = _labels(y)
    _check_rows(X, yv, "y")
    return yv


def _fit_da(cls, X, y, nlvdis, metric, h, k, nlv, prior, tol, scal, verbose, ctx):
    X = ensure_mat(X)
    yv = _check_da(X, y, metric, h, k, tol, nlv, nlvdis, "unif" if prior is None else prior)
    lev, ni = np.unique(yv, return_counts=True)
    fm = None if nlvdis == 0 else plskern(X, _dummy_like(yv, X), nlv=int(nlvdis), scal=scal, ctx=ctx)   # src/lwplsrda.jl:89
    if prior is None:
        return cls(X, y, fm, metric, h, int(k), int(nlv), tol, bool(scal), bool(verbose), lev, ni)
    return cls(X, y, fm, metric, h, int(k), int(nlv), prior, tol, bool(scal), bool(verbose), lev, ni)


def lwplsrda(X, y, *, nlvdis, metric, h, k, nlv, tol: float = 1e-4, scal: bool = False, verbose: bool = False, ctx: Optional[Context] = None) -> Lwplsrda:
    """`lwplsrda(X, y; nlvdis, metric, h, k, nlv, tol = 1e-4, scal = false, verbose = false)` — src/lwplsrda.jl:81-94: stores the data and (nlvdis > 0) a
    global plskern fit on `dummy(y)` whose scores define the neighbourhood space."""
    return _fit_da(Lwplsrda, X, y, nlvdis, metric, h, k, nlv, None, tol, scal, verbose, ctx)


def lwplslda(X, y, *, nlvdis, metric, h, k, nlv, prior: str = "unif", tol: float = 1e-4, scal: bool = False, verbose: bool = False,
             ctx: Optional[Context] = None) -> LwplsLda:
    """`lwplslda(X, y; nlvdis, metric, h, k, nlv, prior = "unif", tol = 1e-4, scal = false, verbose = false)` — src/lwplslda.jl:84-97."""
    return _fit_da(LwplsLda, X, y, nlvdis, metric, h, k, nlv, prior, tol, scal, verbose, ctx)


def lwplsqda(X, y, *, nlvdis, metric, h, k, nlv, prior: str = "unif", tol: float = 1e-4, scal: bool = False, verbose: bool = False,
             ctx: Optional[Context] = None) -> LwplsQda:
    """`lwplsqda(X, y; nlvdis, metric, h, k, nlv, prior = "unif", tol = 1e-4, scal = false, verbose = false)` — src/lwplsqda.jl:89-102."""
    return _fit_da(LwplsQda, X, y, nlvdis, metric, h, k, nlv, prior, tol, scal, verbose, ctx)


def _sample(n, psamp, samp, rowkey, yv, seed):
    """The rows the global reduction is fitted on (None: all of them) — src/lwplsr_s.jl:120-128, src/lwplsrda_s.jl:82-92."""
    ms = int(round(psamp * n))
    if ms >= n:
        return None
    if samp == "sys":
        return np.asarray(sampsys(rowkey(), ms).train, dtype=np.int64)
    if samp == "cla":
        nlev = np.unique(yv).shape[0]
        return np.asarray(sampcla(yv, k=max(int(round(ms / nlev)), 1), seed=seed).train, dtype=np.int64)
    return np.random.default_rng(seed).choice(n, size=ms, replace=False)


def _check_nlv_local(nlv):
    if isinstance(nlv, bool) or int(nlv) != nlv or int(nlv) < 0:
        raise ValueError(f"nlv = {nlv} must be an integer >= 0")


def lwplsr_s(X, Y, *, nlv0, reduc: str = "pls", metric: str = "eucl", h, k, gamma=1, psamp=1, samp: str = "sys", nlv, tol: float = 1e-4,
             scal: bool = False, verbose: bool = False, seed=None, ctx: Optional[Context] = None) -> LwplsrS:
    """`lwplsr_s(X, Y; nlv0, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "sys", nlv, tol = 1e-4, scal = false, verbose = false)` —
    src/lwplsr_s.jl:115-141: a global reduction to nlv0 scores (`pcasvd`, `plskern`, or `dkplsr` with `krbf`) fitted on a sample of the rows, then kNN-LWPLSR
    on the n x nlv0 score table with nlv = min(nlv0, nlv) local LVs."""
    X = _colmajor_x(X); Y = _colmajor_x(Y)
    _check_knn_args(metric, h, k, tol)
    _check_s_args(reduc, samp, ("sys", "random"), psamp, nlv0)
    _check_nlv_local(nlv)
    _check_rows(X, Y)
    if _is_torch(X) != _is_torch(Y):
        raise TypeError("X and Y must both be host arrays or both device tensors")
    s = _sample(X.shape[0], psamp, samp, lambda: Y.sum(dim=1).cpu().numpy() if _is_torch(Y) else np.asarray(Y).sum(axis=1), None, seed)
    fm, T = _reduce(X, Y, None, s, int(nlv0), reduc, gamma, scal, ctx)
    return LwplsrS(T, Y, fm, metric, h, int(k), min(int(nlv0), int(nlv)), tol, bool(scal), bool(verbose))


def lwplsrda_s(X, y, *, nlv0, reduc: str = "pls", metric: str = "eucl", h, k, gamma=1, psamp=1, samp: str = "cla", nlv, tol: float = 1e-4,
               scal: bool = False, verbose: bool = False, seed=None, ctx: Optional[Context] = None) -> LwplsrdaS:
    """`lwplsrda_s(X, y; nlv0, reduc = "pls", metric = "eucl", h, k, gamma = 1, psamp = 1, samp = "cla", nlv, tol = 1e-4, scal = false, verbose = false)` —
    src/lwplsrda_s.jl:77-105.  reduc = "pls" is `plsrda`; "dkpls" is `dkplsr` on `dummy(y)`, which is what the reference's `dkplsrda` fits."""
    X = _colmajor_x(X)
    _check_knn_args(metric, h, k, tol)
    _check_s_args(reduc, samp, ("cla", "random"), psamp, nlv0)
    _check_nlv_local(nlv)
    yv = _labels(y)
    _check_rows(X, yv, "y")
    s = _sample(X.shape[0], psamp, samp, None, yv, seed)
    Yd = None if reduc != "dkpls" else _dummy_like(yv, X)
    fm, T = _reduce(X, Yd, yv, s, int(nlv0), reduc, gamma, scal, ctx)
    return LwplsrdaS(T, y, fm, metric, h, int(k), min(int(nlv0), int(nlv)), tol, bool(scal), bool(verbose))


# ---------------------------------------------------------------------------------- predict
def _engine(obj, coords, yv=None, Y=None):
    """The `Lwplsr` this model predicts through (its handle cache, query maps and host / device rules: plsr.py) — on the dummy table of the labels for
    the discrimination models.  Kept with the object; rebuilt when its data were re-assigned."""
    key = (id(coords), id(getattr(obj, "y", None)), id(getattr(obj, "Y", None)), id(obj.fm), obj.metric, bool(obj.scal))
    st = obj.__dict__.get("_lw_engine")
    if st is not None and st["key"] == key:
        return st
    st = {"key": key}
    if yv is not None:
        lev = np.unique(yv)
        codes = np.searchsorted(lev, yv).astype(np.int32)
        st["lev"] = lev
        st["cls"] = torch.as_tensor(codes, device=coords.device) if _is_torch(coords) else codes
        Y = _dummy_like(yv, coords)
    fm = obj.fm if isinstance(obj, (Lwplsrda, LwplsLda)) else None   # (the _s models search in their score table itself)
    st["eng"] = Lwplsr(coords, Y, fm, obj.metric, obj.h, obj.k, obj.nlv, obj.tol, obj.scal, False)
    obj.__dict__["_lw_engine"] = st
    return st


def _nlv_range(obj, nlv, p):
    a = obj.nlv
    if nlv is None:
        lo = hi = a
    else:
        vals = np.atleast_1d(np.asarray(nlv))
        lo, hi = max(int(vals.min()), 0), min(int(vals.max()), a)
    return lo, min(hi, p)                                         # src/locwlv.jl:14


def _da_predict(obj, coords, X, nlv, ctx, kind, prior, who):
    X = ensure_mat(X)
    try:
        _addr_ld(X)
    except (ValueError, TypeError):
        X = _as_colmajor_copy(X)
    dev = _is_torch(X)
    if dev != _is_torch(coords):
        raise TypeError("training data and queries must both be host arrays or both device tensors")
    n, p = coords.shape
    if X.shape[1] != p:
        raise ValueError(f"DimensionMismatch: X has {X.shape[1]} columns, the model has {p}")
    lo, hi = _nlv_range(obj, nlv, p)
    if hi < lo:
        raise ValueError(f"{who}: empty nlv range {lo} .. {hi}")
    if kind != "rda" and lo < 1:
        raise ValueError(f"{who}: a Gaussian discriminant needs at least one score column (nlv = 0 requested)")   # the reference indexes fm_da[0]
    ctx = ctx or default_context((X.device.index or 0) if dev else 0)
    st = _engine(obj, coords, yv=_labels(obj.y))
    eng, lev, cls = st["eng"], st["lev"], st["cls"]
    nlev = len(lev)
    m, k, le = X.shape[0], min(int(obj.k), n), hi - lo + 1
    hd = _lwplsr_prepared(eng, ctx, dev, nlev)
    code = np.empty((m, le), dtype=np.int32); info = np.empty((m, le), dtype=np.int32); post = np.empty((m, le, nlev))
    ind = np.empty((m, k), dtype=np.int32); dist = np.empty((m, k)); w = np.empty((m, k))
    if hd["device_map"]:
        qa, ldq = None, 0
    else:
        Zq = hd["qmap"](X)
        qa, ldq = _addr_ld(Zq)
    xqa, ldxq = _addr_ld(X)
    if dev:
        torch.cuda.current_stream(X.device).synchronize()
    ctx.check(_lib.load().jch_lwplsda_predict_prepared(ctx._h, hd["handle"], _ptr(cls), nlev, _KIND[kind], _PRIOR[prior], _lib.LOC_DEVICE if dev else _lib.LOC_HOST,
                                                       qa, ldq, xqa, m, ldxq, k, float(obj.h), float(obj.tol), int(obj.scal), lo, hi, code.ctypes.data,
                                                       post.ctypes.data, info.ctypes.data, None, None, _np(ind), _np(dist), _np(w)))
    nbad = int((info == 2).any(axis=1).sum())
    if nbad:
        warnings.warn(f"{who}: {nbad} of {m} neighbourhoods have a covariance that is not positive definite; their labels are the weighted vote", RuntimeWarning,
                      stacklevel=3)
    if getattr(obj, "verbose", False):                            # src/locwlv.jl:19,40
        print("".join(f"{i} " for i in range(1, m + 1)))
    lev = np.asarray(lev)
    preds = [lev[code[:, i]].reshape(-1, 1) for i in range(le)]
    posts = [post[:, i, :].copy() for i in range(le)]
    return LwplsdaPred(preds[0] if le == 1 else preds, ind, dist, w, posts[0] if le == 1 else posts, info[:, 0].copy() if le == 1 else info)


def lwplsrda_predict(obj: Lwplsrda, X, *, nlv=None, ctx: Optional[Context] = None) -> LwplsdaPred:
    """`predict(object::Lwplsrda, X; nlv)` — src/lwplsrda.jl:102-131: `locwlv` with `plsrda`.  posterior: the dummy predictions."""
    return _da_predict(obj, obj.X, X, nlv, ctx, "rda", "unif", "lwplsrda_predict")


def lwplslda_predict(obj: LwplsLda, X, *, nlv=None, ctx: Optional[Context] = None) -> LwplsdaPred:
    """`predict(object::LwplsLda, X; nlv)` — src/lwplslda.jl:105-134: `locwlv` with `plslda`; nlv = 0 raises."""
    return _da_predict(obj, obj.X, X, nlv, ctx, "lda", obj.prior, "lwplslda_predict")


def lwplsqda_predict(obj: LwplsQda, X, *, nlv=None, ctx: Optional[Context] = None) -> LwplsdaPred:
    """`predict(object::LwplsQda, X; nlv)` — src/lwplsqda.jl:110-139: `locwlv` with `plsqda`; nlv = 0 raises."""
    return _da_predict(obj, obj.X, X, nlv, ctx, "qda", obj.prior, "lwplsqda_predict")


def _scores_of(obj, X, ctx):
    X = _colmajor_x(X)
    if _is_torch(X) != _is_torch(obj.T):
        raise TypeError("training data and queries must both be host arrays or both device tensors")
    ctx = ctx or default_context((X.device.index or 0) if _is_torch(X) else 0)
    return _transform(obj.fm, X, ctx), ctx


def lwplsr_s_predict(obj: LwplsrS, X, *, nlv=None, ctx: Optional[Context] = None) -> LwplsrPred:
    """`predict(object::LwplsrS, X; nlv)` — src/lwplsr_s.jl:149-178: the scores of X under the global reduction, then `lwplsr_predict` on the score table."""
    Tq, ctx = _scores_of(obj, X, ctx)
    res = lwplsr_predict(_engine(obj, obj.T, Y=obj.Y)["eng"], Tq, nlv=nlv, ctx=ctx)
    if getattr(obj, "verbose", False):
        print("".join(f"{i} " for i in range(1, Tq.shape[0] + 1)))
    return res


def lwplsrda_s_predict(obj: LwplsrdaS, X, *, nlv=None, ctx: Optional[Context] = None) -> LwplsdaPred:
    """`predict(object::LwplsrdaS, X; nlv)` — src/lwplsrda_s.jl:113-142: as `lwplsrda_predict` on the scores of the global reduction."""
    Tq, ctx = _scores_of(obj, X, ctx)
    return _da_predict(obj, obj.T, Tq, nlv, ctx, "rda", "unif", "lwplsrda_s_predict")
