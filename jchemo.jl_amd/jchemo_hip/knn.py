"""k-nearest-neighbour search, kNN regression and discrimination, and the two kNN members of the one-class family — host-side mirror of the
reference's src/getknn.jl, src/knnr.jl, src/knnda.jl, src/occknndis.jl and src/occlknndis.jl over jch_knn_prepare / jch_knn_search /
jch_knn_wmean / jch_knn_vote / jch_knn_gather_median (include/jchemo_hip.h).

numpy in gives numpy out; a device torch tensor in keeps every m-sized result on the device.  Neighbour lists are int32 and 0-based (Julia: 1-based),
m x k row-major, as `lwplsr_predict` returns them.  The search space of `knnr` / `knnda` is built exactly as lwplsr builds it (`_knn_train_space`,
plsr.py); the device handle of a model is built on its first `predict` and kept for the model's lifetime.

`occlknndis`: the reference runs k further brute-force searches per query, each over a fresh row-removed copy of the training scores.  What those
searches compute — the leave-one-out median kNN distance of a training row — does not depend on the query: it is computed once per training row that
some query needs, by one batched search with `self` set, and cached on the device (`dk_train`).  `predict` is then one search plus a gather."""
from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .occ import OccPred, _check_cut, _colmajor_x, _cutoff, _div, _pred, _pval, _sort
from .pca import pca_transform, pcasvd
from .plsr import _addr_ld, _affine, _as_colmajor_copy, _col_stats, _is_torch, _knn_train_space, colmajor_empty, dummy, ensure_mat, plskern

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


@dataclass
class Knnr:
    """src/knnr.jl:1-11 — same fields."""
    X: object
    Y: object
    fm: object
    nlvdis: int
    metric: str
    h: float
    k: int
    tol: float
    scal: bool


@dataclass
class Knnda:
    """src/knnda.jl:1-13 — same fields (y: the labels as given; lev, ni: `tab(y)`)."""
    X: object
    y: object
    fm: object
    nlvdis: int
    metric: str
    h: float
    k: int
    tol: float
    lev: np.ndarray
    ni: np.ndarray
    scal: bool


@dataclass
class KnnPred:
    """What `predict(::Knnr, X)` / `predict(::Knnda, X)` return (src/knnr.jl:168, src/knnda.jl:137): pred (m x q; Knnda: m x 1 labels, a host
    array), listnn (0-based rows), listd, listw — m x k each."""
    pred: object
    listnn: object
    listd: object
    listw: object


@dataclass
class Occknndis:
    """The reference's `Occknndis` (src/occknndis.jl:1-9): d (the table: d, dstand, pval), fm (the Pca), T (the scaled training scores, where X
    lives), tscales, k, e_cdf (the sorted training d), cutoff."""
    d: dict
    fm: object
    T: object
    tscales: np.ndarray
    k: int
    e_cdf: object
    cutoff: float


@dataclass
class Occlknndis:
    """The reference's `Occlknndis` (src/occlknndis.jl:1-9), same fields as `Occknndis`."""
    d: dict
    fm: object
    T: object
    tscales: np.ndarray
    k: int
    e_cdf: object
    cutoff: float


# ---------------------------------------------------------------------------------- the primitives
def _ctx_for(X, ctx):
    return ctx or default_context((X.device.index or 0) if _is_torch(X) else 0)


def _loc_sync(X):
    if _is_torch(X):
        torch.cuda.current_stream(X.device).synchronize()
        return _lib.LOC_DEVICE
    return _lib.LOC_HOST


def _done(ctx, dev):
    """Behind an entry that only enqueued (device in, device out): the results are read by torch, on its own stream."""
    if dev:
        ctx.synchronize()


def _release_handle(handle):
    try:
        _lib.load().jch_knn_release(None, handle)
    except Exception:  # pragma: no cover  (interpreter shutdown)
        pass


def knn_prepare(Zt, ctx: Context):
    """jch_knn_prepare: the device handle of a search space Zt (n x dd).  Release with `knn_release`."""
    Zt = _colmajor_x(Zt)
    n, dd = Zt.shape
    za, ldz = _addr_ld(Zt)
    h = C.c_void_p()
    ctx.check(_lib.load().jch_knn_prepare(ctx._h, _loc_sync(Zt), za, n, dd, ldz, C.byref(h)))
    return h


def knn_release(handle):
    _release_handle(handle)


def _empty(shape, dtype, like):
    if _is_torch(like):
        return torch.empty(shape, dtype={np.int32: torch.int32, np.float64: torch.float64}[dtype], device=like.device)
    return np.empty(shape, dtype=dtype)


def _ptr(a):
    if a is None:
        return None
    return a.data_ptr() if _is_torch(a) else a.ctypes.data


def knn_search(handle, n: int, Zq, k: int, *, self_rows=None, h: float = float("inf"), tol: float = 0.0, want=("ind", "dist"),
               ctx: Optional[Context] = None) -> dict:
    """jch_knn_search on a prepared handle over n training rows: the wanted ones of ind (m x k int32, 0-based), dist, w (m x k) and dmed (m), where
    Zq lives.  self_rows: None or m row indices (-1: none), removed from the respective query's candidates; k clamps to n (n - 1 with self_rows)."""
    Zq = _colmajor_x(Zq)
    m = Zq.shape[0]
    ctx = _ctx_for(Zq, ctx)
    dev = _is_torch(Zq)
    k = min(int(k), n - 1 if self_rows is not None else n)
    if k < 1 or m < 1:
        raise ValueError(f"getknn: k = {k} and m = {m} must be >= 1")
    sr = None
    if self_rows is not None:
        if dev:
            sr = torch.as_tensor(self_rows, device=Zq.device).to(torch.int64).reshape(-1).contiguous()
        else:
            sr = np.ascontiguousarray(np.asarray(self_rows.cpu() if _is_torch(self_rows) else self_rows), dtype=np.int64).reshape(-1)
        if sr.shape[0] != m:
            raise ValueError(f"DimensionMismatch: {m} queries, {sr.shape[0]} self rows")
    out = {}
    if "ind" in want:
        out["ind"] = _empty((m, k), np.int32, Zq)
    for nm in ("dist", "w"):
        if nm in want:
            out[nm] = _empty((m, k), np.float64, Zq)
    if "dmed" in want:
        out["dmed"] = _empty((m,), np.float64, Zq)
    qa, ldq = _addr_ld(Zq)
    loc = _loc_sync(Zq)
    ctx.check(_lib.load().jch_knn_search(ctx._h, handle, loc, qa, m, ldq, k, _ptr(sr), float(h), float(tol), loc, _ptr(out.get("ind")),
                                         _ptr(out.get("dist")), _ptr(out.get("w")), _ptr(out.get("dmed"))))
    _done(ctx, dev)
    return out


def _lists_like(ind, w, like):
    """ind (int32) and w (float64) as contiguous m x k arrays where `like` lives."""
    if _is_torch(like):
        ind = torch.as_tensor(ind, device=like.device).to(torch.int32).contiguous()
        w = None if w is None else torch.as_tensor(w, device=like.device).to(torch.float64).contiguous()
    else:
        ind = np.ascontiguousarray(ind.cpu().numpy() if _is_torch(ind) else ind, dtype=np.int32)
        w = None if w is None else np.ascontiguousarray(w.cpu().numpy() if _is_torch(w) else w, dtype=np.float64)
    if ind.ndim != 2 or (w is not None and tuple(w.shape) != tuple(ind.shape)):
        raise ValueError("ind and w must be m x k arrays of the same shape")
    return ind, w


def knn_wmean(Y, ind, w, *, ctx: Optional[Context] = None):
    """jch_knn_wmean: pred[i, :] = sum_j (w_ij / sum_j w_ij) Y[ind_ij, :] (m x q, where Y lives); fixed summation order."""
    Y = _colmajor_x(Y)
    n, q = Y.shape
    ind, w = _lists_like(ind, w, Y)
    m, k = ind.shape
    ctx = _ctx_for(Y, ctx)
    pred = colmajor_empty(m, q, Y.device) if _is_torch(Y) else np.empty((m, q), order="F")
    ya, ldy = _addr_ld(Y)
    ctx.check(_lib.load().jch_knn_wmean(ctx._h, _loc_sync(Y), ya, n, q, ldy, _ptr(ind), _ptr(w), m, k, _ptr(pred)))
    _done(ctx, _is_torch(Y))
    return pred


def knn_vote(cls, ncls: int, ind, w, *, score: bool = False, ctx: Optional[Context] = None):
    """jch_knn_vote: pred (m, int32) = the class code with the largest summed weight among the classes present in the neighbourhood (ties: the lowest
    code); with `score=True` also the m x ncls table of the sums.  cls: n int32 codes in [0, ncls), a host array or a device tensor."""
    if _is_torch(cls):
        cls = cls.to(torch.int32).reshape(-1).contiguous()
    else:
        cls = np.ascontiguousarray(cls, dtype=np.int32).reshape(-1)
    n = cls.shape[0]
    ind, w = _lists_like(ind, w, cls)
    m, k = ind.shape
    ctx = _ctx_for(cls, ctx)
    pred = _empty((m,), np.int32, cls)
    sc = None
    if score:
        sc = colmajor_empty(m, int(ncls), cls.device) if _is_torch(cls) else np.empty((m, int(ncls)), order="F")
    ctx.check(_lib.load().jch_knn_vote(ctx._h, _loc_sync(cls), _ptr(cls), n, int(ncls), _ptr(ind), _ptr(w), m, k, _ptr(pred), _ptr(sc)))
    _done(ctx, _is_torch(cls))
    return (pred, sc) if score else pred


def knn_gather_median(v, ind, *, ctx: Optional[Context] = None):
    """jch_knn_gather_median: out[i] = median_j v[ind_ij] (`middle` for even k; NaN last), an m-vector where v lives."""
    if _is_torch(v):
        v = v.to(torch.float64).reshape(-1).contiguous()
    else:
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
    n = v.shape[0]
    ind, _ = _lists_like(ind, None, v)
    m, k = ind.shape
    ctx = _ctx_for(v, ctx)
    out = _empty((m,), np.float64, v)
    ctx.check(_lib.load().jch_knn_gather_median(ctx._h, _loc_sync(v), _ptr(v), n, _ptr(ind), m, k, _ptr(out)))
    _done(ctx, _is_torch(v))
    return out


# ---------------------------------------------------------------------------------- getknn
def _check_metric(metric):
    if metric not in ("eucl", "mahal"):
        raise ValueError(f"metric must be 'eucl' or 'mahal', got {metric!r}")


def getknn(Xtrain, X, *, k: int = 1, metric: str = "eucl", ctx: Optional[Context] = None):
    """`getknn(Xtrain, X; k = 1, metric = "eucl")` — src/getknn.jl:29-57: (ind, d), m x k each, neighbours in (distance, row) order, k clamped to n.
    "mahal": the whitening of `_knn_train_space` (jch_weighted_cov, host Cholesky, the diagonal fallback of :43)."""
    _check_metric(metric)
    Xtrain = _colmajor_x(Xtrain)
    X = _colmajor_x(X)
    if _is_torch(X) != _is_torch(Xtrain):
        raise TypeError("Xtrain and X must both be host arrays or both device tensors")
    if X.shape[1] != Xtrain.shape[1]:
        raise ValueError(f"DimensionMismatch: Xtrain has {Xtrain.shape[1]} columns, X has {X.shape[1]}")
    ctx = _ctx_for(X, ctx)
    Zt, qmap, _ = _knn_train_space(SimpleNamespace(X=Xtrain, Y=None, fm=None, metric=metric, scal=False), ctx)
    handle = knn_prepare(Zt, ctx)
    try:
        res = knn_search(handle, Zt.shape[0], qmap(X), k, ctx=ctx)
    finally:
        knn_release(handle)
    return res["ind"], res["dist"]


# ---------------------------------------------------------------------------------- knnr / knnda
# Prepared device handles live outside the model instances (keyed by id(obj), dropped by a per-object finalizer), as for Lwplsr (plsr.py).
_KNN_PREP = {}


def _drop_prep(oid):
    st = _KNN_PREP.pop(oid, None)
    if st is not None:
        _release_handle(st["handle"])


def _prepared(obj, key, build):
    """The cached state of `obj` — {"key", "handle", ...} — rebuilt by `build()` when `key` changed."""
    oid = id(obj)
    st = _KNN_PREP.get(oid)
    if st is not None and st["key"] == key:
        return st
    if st is not None:
        _drop_prep(oid)
    else:
        weakref.finalize(obj, _drop_prep, oid)
    st = build()
    st["key"] = key
    _KNN_PREP[oid] = st
    return st


def _knn_model_prepared(obj, ynum, ctx, dev: bool):
    """Handle + query map of a Knnr / Knnda (the search space of src/knnr.jl:142-154 built by `_knn_train_space`).  The key covers what the handle was
    built from: re-assigning obj.X, obj.fm, obj.metric or obj.scal after a predict rebuilds it."""
    key = (id(ctx), ctx._h.value, dev, id(obj.X), id(obj.fm), obj.metric, bool(obj.scal))

    def build():
        # (`_knn_train_space` reads Y only for colstd(X) of the unreduced, scaled space: any response matrix of n rows serves)
        Y = ynum() if (obj.fm is None and obj.scal) else None
        Zt, qmap, _ = _knn_train_space(SimpleNamespace(X=obj.X, Y=Y, fm=obj.fm, metric=obj.metric, scal=obj.scal), ctx)
        return {"handle": knn_prepare(Zt, ctx), "qmap": qmap, "n": Zt.shape[0]}
    return _prepared(obj, key, build)


def _check_knn_args(metric, h, k, tol):
    _check_metric(metric)
    if isinstance(k, bool) or int(k) != k or int(k) < 1:
        raise ValueError(f"k = {k} must be an integer >= 1")
    if not float(h) > 0.0:
        raise ValueError(f"h = {h} must be > 0")


def knnr(X, Y, *, nlvdis: int = 0, metric: str = "eucl", h: float = float("inf"), k: int = 1, tol: float = 1e-4, scal: bool = False,
         ctx: Optional[Context] = None) -> Knnr:
    """`knnr(X, Y; nlvdis = 0, metric = "eucl", h = Inf, k = 1, tol = 1e-4, scal = false)` — src/knnr.jl:119-130: stores the data and (nlvdis > 0) a
    global plskern fit whose scores define the neighbourhood space."""
    X = ensure_mat(X); Y = ensure_mat(Y)
    _check_knn_args(metric, h, k, tol)
    fm = None if nlvdis == 0 else plskern(X, Y, nlv=nlvdis, scal=scal, ctx=ctx)
    return Knnr(X, Y, fm, int(nlvdis), metric, h, int(k), tol, bool(scal))


def _labels(y):
    return np.asarray(y.cpu() if _is_torch(y) else y).reshape(-1)


def _dummy_like(y, X):
    Yd, _ = dummy(y)
    Yd = np.asfortranarray(Yd)
    if _is_torch(X):
        Yt = colmajor_empty(Yd.shape[0], Yd.shape[1], X.device); Yt.copy_(torch.from_numpy(Yd)); Yd = Yt
    return Yd


def knnda(X, y, *, nlvdis: int = 0, metric: str = "eucl", h: float = float("inf"), k: int = 1, tol: float = 1e-4, scal: bool = False,
          ctx: Optional[Context] = None) -> Knnda:
    """`knnda(X, y; nlvdis = 0, metric = "eucl", h = Inf, k = 1, tol = 1e-4, scal = false)` — src/knnda.jl:87-100: lev and ni from `tab(y)`; with
    nlvdis > 0 the neighbourhood space is the scores of plskern on `dummy(y)`."""
    X = ensure_mat(X)
    _check_knn_args(metric, h, k, tol)
    yv = _labels(y)
    if yv.shape[0] != X.shape[0]:
        raise ValueError(f"DimensionMismatch: X has {X.shape[0]} rows, y has {yv.shape[0]}")
    lev, ni = np.unique(yv, return_counts=True)
    fm = None if nlvdis == 0 else plskern(X, _dummy_like(yv, X), nlv=nlvdis, scal=scal, ctx=ctx)
    return Knnda(X, y, fm, int(nlvdis), metric, h, int(k), tol, lev, ni, bool(scal))


def _knn_lists(obj, X, ynum, ctx):
    X = _colmajor_x(X)
    dev = _is_torch(X)
    if dev != _is_torch(obj.X):
        raise TypeError("training data and queries must both be host arrays or both device tensors")
    if X.shape[1] != obj.X.shape[1]:
        raise ValueError(f"DimensionMismatch: X has {X.shape[1]} columns, the model has {obj.X.shape[1]}")
    ctx = _ctx_for(X, ctx)
    st = _knn_model_prepared(obj, ynum, ctx, dev)
    res = knn_search(st["handle"], st["n"], st["qmap"](X), obj.k, h=obj.h, tol=obj.tol, want=("ind", "dist", "w"), ctx=ctx)
    return res, st, ctx


def knnr_predict(obj: Knnr, X, *, ctx: Optional[Context] = None) -> KnnPred:
    """`predict(object::Knnr, X)` — src/knnr.jl:137-169: one jch_knn_search (neighbours, distances, `wdist` weights clamped to tol), then the
    weighted means of the neighbours' responses by jch_knn_wmean."""
    res, st, ctx = _knn_lists(obj, X, lambda: obj.Y, ctx)
    Y = obj.Y
    try:
        _addr_ld(Y)
    except (ValueError, TypeError):
        Y = _as_colmajor_copy(Y)
    return KnnPred(knn_wmean(Y, res["ind"], res["w"], ctx=ctx), res["ind"], res["dist"], res["w"])


def knnda_predict(obj: Knnda, X, *, ctx: Optional[Context] = None) -> KnnPred:
    """`predict(object::Knnda, X)` — src/knnda.jl:108-138: the search, then the weighted vote by jch_knn_vote (`findmax_cla`: the first of the sorted
    levels on ties).  pred: an m x 1 host array of labels."""
    yv = _labels(obj.y)
    res, st, ctx = _knn_lists(obj, X, lambda: _dummy_like(yv, obj.X), ctx)
    if "cls" not in st:
        codes = np.searchsorted(obj.lev, yv).astype(np.int32)
        st["cls"] = torch.as_tensor(codes, device=res["ind"].device) if _is_torch(res["ind"]) else codes
    code = knn_vote(st["cls"], len(obj.lev), res["ind"], res["w"], ctx=ctx)
    code = code.cpu().numpy() if _is_torch(code) else code
    return KnnPred(np.asarray(obj.lev)[code].reshape(-1, 1), res["ind"], res["dist"], res["w"])


# ---------------------------------------------------------------------------------- occknndis / occlknndis
def _occ_scores(X, nlv, scal, ctx):
    """pcasvd, then the scores divided by their column stds (src/occknndis.jl:131-134)."""
    fm = pcasvd(X, nlv=nlv, scal=scal, ctx=ctx)
    tscales = _col_stats(fm.T, None, True, ctx)[1]
    return fm, tscales, _affine(fm.T, None, None, np.diag(1.0 / tscales), None, ctx)


def _occ_query(obj, X, ctx):
    """transform(object.fm, X) scaled by tscales (src/occknndis.jl:160-161)."""
    return _affine(pca_transform(obj.fm, X, ctx=ctx), None, None, np.diag(1.0 / obj.tscales), None, ctx)


def _samp_arg(samp, n, nsamp, seed):
    if samp is None:
        samp = np.random.default_rng(seed).choice(n, size=int(nsamp), replace=False)
    samp = np.asarray(samp, dtype=np.int64).reshape(-1)
    if samp.size < 1 or samp.min() < 0 or samp.max() >= n or np.unique(samp).size != samp.size:
        raise ValueError(f"samp must hold distinct rows in [0, {n})")
    return samp


def _occ_table(d, typc, cri, alpha):
    e_cdf = _sort(d)
    cutoff = _cutoff(e_cdf, typc, cri, alpha)
    return dict(d=d, dstand=_div(d, cutoff), pval=_pval(e_cdf, d)), e_cdf, cutoff


def _rows(T, rows):
    """T[rows, :] as a column-major matrix where T lives."""
    if _is_torch(T):
        out = colmajor_empty(len(rows), T.shape[1], T.device)
        out.copy_(T[torch.as_tensor(rows, device=T.device)])
        return out
    return np.asfortranarray(T[rows])


def _occ_handle(obj, ctx):
    """The handle on the scaled training scores of an Occknndis / Occlknndis and, for the latter, the cache `dk_train`: a device n-vector of the
    leave-one-out median kNN distances of the training rows, NaN where not yet computed."""
    key = (id(ctx), ctx._h.value, id(obj.T), int(obj.k))

    def build():
        n = obj.T.shape[0]
        st = {"handle": knn_prepare(obj.T, ctx), "n": n}
        if isinstance(obj, Occlknndis):
            st["dk_train"] = torch.full((n,), float("nan"), dtype=torch.float64, device=torch.device("cuda", ctx.device))
        return st
    return _prepared(obj, key, build)


def occknndis(X, *, nlv, nsamp=None, k, typc: str = "mad", cri=3, alpha=.025, scal: bool = False, samp=None, seed=None,
              ctx: Optional[Context] = None) -> Occknndis:
    """`occknndis(X; nlv, nsamp, k, typc = "mad", cri = 3, alpha = .025, scal = false)` — src/occknndis.jl:125-149.  The sampled rows' k + 1 nearest
    neighbours among all rows; d = the median over places 2:end (:141, literally — no row is removed).  `samp` (0-based rows) may be given, like `P=`
    for `stah`: the reference's `sample` draws from a stream it does not pin; otherwise `nsamp` rows are drawn with `seed`."""
    _check_cut(typc, cri, alpha)
    X = _colmajor_x(X)
    ctx = _ctx_for(X, ctx)
    k = int(k)
    fm, tscales, T = _occ_scores(X, nlv, scal, ctx)
    n = T.shape[0]
    samp = _samp_arg(samp, n, nsamp, seed)
    obj = Occknndis({}, fm, T, tscales, k, None, 0.0)
    st = _occ_handle(obj, ctx)
    dist = knn_search(st["handle"], n, _rows(T, samp), k + 1, ctx=ctx, want=("dist",))["dist"]          # :137-138
    rest = dist[:, 1:]                                                                                    # :141  res.d[i][2:end]
    kk = rest.shape[1]
    d = rest[:, kk // 2] if kk % 2 else rest[:, kk // 2 - 1] / 2 + rest[:, kk // 2] / 2                   # the list is sorted: `median`
    d = d.contiguous() if _is_torch(d) else np.ascontiguousarray(d)
    obj.d, obj.e_cdf, obj.cutoff = _occ_table(d, typc, cri, alpha)                                        # :143-147
    return obj


def _dk_train(st, rows, k, ctx):
    """Fills the cache for the training rows `rows` (a device int64 tensor) that are not in it yet: one search with those rows as queries, `self` set
    to their own index and only dmed asked for — the median of getknn(rmrow(T, j), T[j:j, :]; k).d[1] (src/occlknndis.jl:153-154)."""
    dk = st["dk_train"]
    need = rows[torch.isnan(dk[rows])]
    if need.numel():
        need = torch.unique(need)
        Zq = colmajor_empty(need.numel(), st["T"].shape[1], dk.device)
        Zq.copy_(st["T"][need])
        dk[need] = knn_search(st["handle"], st["n"], Zq, k, self_rows=need, want=("dmed",), ctx=ctx)["dmed"]
    return dk


def _device_scores(st, T):
    """The scaled training scores as a device tensor (the cache fills gather rows from it)."""
    if "T" not in st:
        if _is_torch(T):
            st["T"] = T
        else:
            Td = colmajor_empty(T.shape[0], T.shape[1], st["dk_train"].device); Td.copy_(torch.from_numpy(np.ascontiguousarray(T))); st["T"] = Td
    return st["T"]


def _lk_ratio(obj, st, Zq, self_rows, shift_literal, ctx):
    """d = dmed / zd for the queries Zq (src/occlknndis.jl:148-158, :178-194): one search (with `self_rows` removed when given), the cache fill for the
    unique neighbour rows, then zd = jch_knn_gather_median(dk_train, ind).  shift_literal: the neighbours are numbered as rows of the row-removed
    matrix and used unshifted as rows of T (the reference's second slip)."""
    kin = min(int(obj.k), st["n"] - 1)                     # the neighbours' own searches always remove a row
    k = kin if self_rows is not None else min(int(obj.k), st["n"])
    dev = st["dk_train"].device
    _device_scores(st, obj.T)
    if not _is_torch(Zq):
        Zd = colmajor_empty(Zq.shape[0], Zq.shape[1], dev); Zd.copy_(torch.from_numpy(np.ascontiguousarray(Zq)))
    else:
        Zd = Zq
    sr = None if self_rows is None else torch.as_tensor(np.asarray(self_rows, dtype=np.int64), device=dev)
    res = knn_search(st["handle"], st["n"], Zd, k, self_rows=sr, want=("ind", "dmed"), ctx=ctx)
    ind = res["ind"]
    if shift_literal:
        ind = (ind.to(torch.int64) - (ind.to(torch.int64) > sr[:, None]).to(torch.int64)).to(torch.int32).contiguous()
    dk = _dk_train(st, ind.to(torch.int64).reshape(-1), kin, ctx)
    zd = knn_gather_median(dk, ind, ctx=ctx)
    d = res["dmed"] / zd
    return d if _is_torch(Zq) else d.cpu().numpy()


def occlknndis(X, *, nlv, nsamp=None, k, typc: str = "mad", cri=3, alpha=.025, scal: bool = False, samp=None, seed=None, reading: str = "literal",
               ctx: Optional[Context] = None) -> Occlknndis:
    """`occlknndis(X; nlv, nsamp, k, typc = "mad", cri = 3, alpha = .025, scal = false)` — src/occlknndis.jl:132-165.
    reading = "literal" follows :146-157 line by line, its two slips included: the query is row i of T while the removed row is samp[i], and the
    neighbour indices of the row-removed matrix are used unshifted as rows of T.  reading = "doc" does what the docstring says: the query is row
    samp[i], it is removed, and the indices are mapped back.  `predict` is the same under both."""
    _check_cut(typc, cri, alpha)
    if reading not in ("literal", "doc"):
        raise ValueError(f'reading = {reading!r} must be "literal" or "doc"')
    X = _colmajor_x(X)
    ctx = _ctx_for(X, ctx)
    k = int(k)
    fm, tscales, T = _occ_scores(X, nlv, scal, ctx)
    n = T.shape[0]
    if n < 2:
        raise ValueError("occlknndis needs at least two rows")
    samp = _samp_arg(samp, n, nsamp, seed)
    obj = Occlknndis({}, fm, T, tscales, k, None, 0.0)
    st = _occ_handle(obj, ctx)
    literal = reading == "literal"
    qrows = np.arange(samp.size) if literal else samp                                                     # :148  fm.T[i:i, :]
    d = _lk_ratio(obj, st, _rows(T, qrows), samp, literal, ctx)
    d = d.contiguous() if _is_torch(d) else np.ascontiguousarray(d)
    obj.d, obj.e_cdf, obj.cutoff = _occ_table(d, typc, cri, alpha)                                        # :159-163
    return obj


def occknn_predict(obj, X, *, ctx: Optional[Context] = None) -> OccPred:
    """`predict(object::Occknndis, X)` (src/occknndis.jl:157-171): d = the median of the k nearest distances; `predict(object::Occlknndis, X)`
    (src/occlknndis.jl:173-199): that median over the median of the neighbours' own leave-one-out medians, from the cache."""
    X = _colmajor_x(X)
    if _is_torch(X) != _is_torch(obj.T):
        raise TypeError("the model's scores and X must both be host arrays or both device tensors")
    ctx = _ctx_for(X, ctx)
    st = _occ_handle(obj, ctx)
    Zq = _occ_query(obj, X, ctx)
    if isinstance(obj, Occlknndis):
        d = _lk_ratio(obj, st, Zq, None, False, ctx)
    else:
        d = knn_search(st["handle"], st["n"], Zq, obj.k, want=("dmed",), ctx=ctx)["dmed"]
    tab = dict(d=d, dstand=_div(d, obj.cutoff), pval=_pval(obj.e_cdf, d))
    return OccPred(_pred(tab["dstand"]), tab)
