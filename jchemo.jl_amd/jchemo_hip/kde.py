"""Gaussian kernel density estimation and the discrimination built on it — host-side mirror of the reference's src/dmkern.jl, src/kdeda.jl and
src/plskdeda.jl over jch_kde_dens (include/jchemo_hip.h).

numpy in gives numpy out; a device torch tensor in keeps `dens` / `posterior` (and `pred` of `dmkern_predict`) on the device.  Class labels
(`pred` of the discrimination) are host arrays, as everywhere else.

Every model of the family has a diagonal bandwidth matrix whose inverse separates: model a (the first dims[a] columns), class c, column j has
1 / h = u[j, c] * v[a, c] — default `h`: u = 1 / colstd of the class, v = n_c^(1 / (dims_a + 4)) / a; a real `h`: u = 1 / h, v = 1; a vector `h`
(one model): u = 1 / h_j, v = 1.  So one device pass over the (query, training row) pairs evaluates a `dmkern`, the classes of a `kdeda`, or the
nlv x nlev densities of a `plskdeda` prediction (the squared distance in the first a score columns is a prefix of the one in the first a + 1);
nothing of size m x n is stored.  The density is the reference's plain sum of `exp` terms: a query far from every training row of every class
gets densities of exactly 0, a NaN posterior and the first level as its prediction (Julia's `argmax`, and numpy's, on a NaN row)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .plsr import Plslda, _addr_ld, _as_colmajor_copy, _col_stats, _is_torch, colmajor_empty, dummy, ensure_mat, plskern, transform

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


@dataclass
class Dmkern:
    """src/dmkern.jl:1-6 — same fields: X (the training rows, where they were given), H (p x p diagonal), Hinv, detH."""
    X: object
    H: np.ndarray
    Hinv: np.ndarray
    detH: float


@dataclass
class Kernda:
    """src/kdeda.jl:1-6 — same fields: fm (one Dmkern per level), wprior, lev, ni."""
    fm: list
    wprior: np.ndarray
    lev: np.ndarray
    ni: np.ndarray


# ---------------------------------------------------------------------------------- the primitive
def _ctx_for(X, ctx):
    return ctx or default_context((X.device.index or 0) if _is_torch(X) else 0)


def _colmajor(X):
    X = ensure_mat(X)
    try:
        _addr_ld(X)
    except (ValueError, TypeError):
        X = _as_colmajor_copy(X)
    return X


def kde_dens(Z, Xq, cls_start, u, v2, coef, dims, *, ctx: Optional[Context] = None):
    """jch_kde_dens: out[i, c, a] = coef[a, c] * sum_{r in class c} exp(-0.5 * v2[a, c] * sum_{j < dims[a]} ((Xq[i, j] - Z[r, j]) * u[j, c])^2), an
    (m, ncls, nmod) array where Xq lives (element (i, c, a) at i + m * (c + ncls * a)).  Z (n x d): the training rows grouped by class, class c
    in rows cls_start[c] .. cls_start[c + 1] - 1; u (d x ncls), v2 and coef (nmod x ncls), dims (nmod, non-decreasing within [1, d]): host arrays."""
    Z, Xq = _colmajor(Z), _colmajor(Xq)
    dev = _is_torch(Xq)
    if dev != _is_torch(Z):
        raise TypeError("Z and Xq must both be host arrays or both device tensors")
    n, d = Z.shape
    m = Xq.shape[0]
    if Xq.shape[1] != d:
        raise ValueError(f"DimensionMismatch: Z has {d} columns, Xq has {Xq.shape[1]}")
    cs = np.ascontiguousarray(cls_start, dtype=np.int64).reshape(-1)
    dm = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1)
    ncls, nmod = cs.shape[0] - 1, dm.shape[0]
    u = np.asfortranarray(np.asarray(u, dtype=np.float64).reshape(d, -1))
    v2 = np.asfortranarray(np.asarray(v2, dtype=np.float64).reshape(nmod, -1))
    coef = np.asfortranarray(np.asarray(coef, dtype=np.float64).reshape(nmod, -1))
    if ncls < 1 or nmod < 1 or u.shape[1] != ncls or v2.shape[1] != ncls or coef.shape[1] != ncls:
        raise ValueError(f"kde_dens: {ncls} classes and {nmod} models, but u is {u.shape}, v2 {v2.shape}, coef {coef.shape}")
    ctx = _ctx_for(Xq, ctx)
    if dev:
        out = torch.empty((nmod, ncls, m), dtype=torch.float64, device=Xq.device).permute(2, 1, 0)
        torch.cuda.current_stream(Xq.device).synchronize()
        oa = out.data_ptr()
    else:
        out = np.empty((nmod, ncls, m), dtype=np.float64).transpose(2, 1, 0)
        oa = out.ctypes.data
    za, ldz = _addr_ld(Z)
    qa, ldq = _addr_ld(Xq)
    ctx.check(_lib.load().jch_kde_dens(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, za, n, d, ldz, qa, m, ldq, cs.ctypes.data, ncls,
                                       u.ctypes.data, v2.ctypes.data, coef.ctypes.data, dm.ctypes.data, nmod, oa, max(m, 1)))
    return out


# ---------------------------------------------------------------------------------- dmkern
def _check_h(h, a, p, who):
    """h: None, a real, or a p-vector -> (None | float | np.ndarray); `a` as a float.  Raises before any device work."""
    a = float(a)
    if h is None:
        return None, a
    if np.ndim(h) == 0:
        return float(h), a
    hv = np.asarray(h.cpu() if _is_torch(h) else h, dtype=np.float64).reshape(-1)
    if hv.shape[0] != p:
        raise ValueError(f"DimensionMismatch: {who}: h has {hv.shape[0]} entries, the data has {p} columns")
    return hv, a


def _is_constant_column(X):
    """True where a column of X holds one value only (its colstd is 0: `inv(H)` throws in the reference)."""
    if _is_torch(X):
        return bool((X.amax(dim=0) == X.amin(dim=0)).any().item())
    return bool(np.any(X.max(axis=0) == X.min(axis=0)))


def _scott(n, p, a):
    """a * n^(-1 / (p + 4)) (src/dmkern.jl:134)."""
    return a * n ** (-1 / (p + 4))


def _dm_record(X, hvec):
    """Dmkern from the p bandwidths: H = diagm(h), Hinv = inv(H), detH = det(H) with 0 -> 1e-20 (src/dmkern.jl:135-142)."""
    if np.any(hvec == 0):
        raise ValueError("SingularException: a bandwidth of 0 (constant column, or h = 0): H cannot be inverted")
    detH = 1.0
    for v in hvec:
        detH *= float(v)
    return Dmkern(X, np.diag(hvec), np.diag(1.0 / hvec), 1e-20 if detH == 0 else detH)


def _bandwidths(std, n, p, h, a):
    """The p bandwidths of one dmkern: default a * n^(-1/(p+4)) * colstd, a real h repeated, or the vector as given."""
    if h is None:
        return _scott(n, p, a) * np.asarray(std[:p], dtype=np.float64)
    return np.full(p, h) if np.ndim(h) == 0 else np.array(h, dtype=np.float64)


def _check_default_h(X, n, who):
    if n == 1:
        raise ValueError(f"SingularException: {who}: one training row and h = None: colstd is 0 and H cannot be inverted")
    if _is_constant_column(X):
        raise ValueError(f"SingularException: {who}: a constant column and h = None: colstd is 0 and H cannot be inverted")


def dmkern(X, *, h=None, a=1, ctx: Optional[Context] = None) -> Dmkern:
    """`dmkern(X; h = nothing, a = 1)` — src/dmkern.jl:124-143.  The default bandwidth's colstd (uncorrected, uniform weights) comes from the
    device (jch_col_stats).  A constant column, or one row, with h = None raises ValueError (the reference's `inv(H)` throws)."""
    X = ensure_mat(X)
    n, p = X.shape
    h, a = _check_h(h, a, p, "dmkern")
    std = None
    if h is None:
        _check_default_h(X, n, "dmkern")
        std = _col_stats(X, None, True, ctx)[1]
    return _dm_record(X, _bandwidths(std, n, p, h, a))


def _norm_coef(n, p, detH):
    """1 / n * (2 * pi)^(-p / 2) * (1 / detH), in the reference's order (src/dmkern.jl:160)."""
    return 1 / n * (2 * math.pi) ** (-p / 2) * (1 / detH)


def dmkern_predict(obj: Dmkern, X, *, ctx: Optional[Context] = None):
    """`predict(object::Dmkern, X)` — src/dmkern.jl:151-163: pred (m x 1) where X lives, one jch_kde_dens call."""
    X = ensure_mat(X)
    n, p = obj.X.shape
    if X.shape[1] != p:
        raise ValueError(f"DimensionMismatch: X has {X.shape[1]} columns, the model has {p}")
    out = kde_dens(obj.X, X, [0, n], np.diag(obj.Hinv).reshape(p, 1), [[1.0]], [[_norm_coef(n, p, obj.detH)]], [p], ctx=ctx)
    return out[:, :, 0]


# ---------------------------------------------------------------------------------- kdeda
def _labels(y):
    return np.asarray(y.cpu() if _is_torch(y) else y).reshape(-1)


def _wprior(prior, ni):
    if prior == "unif":
        return np.ones(len(ni)) / len(ni)
    if prior == "prop":
        return ni / ni.sum()
    raise ValueError(f'prior must be "unif" or "prop", got {prior!r}')


def _group_by_class(X, yv, lev):
    """The rows of X grouped by level (a torch `index_select` with the stable order of the labels), column-major where X lives, and the class
    offsets."""
    order = np.argsort(np.searchsorted(lev, yv), kind="stable")
    if _is_torch(X):
        Zg = colmajor_empty(X.shape[0], X.shape[1], X.device)
        Zg.copy_(torch.index_select(X.to(torch.float64), 0, torch.as_tensor(order, device=X.device)))
    else:
        Zg = np.asfortranarray(torch.index_select(torch.from_numpy(np.ascontiguousarray(X, dtype=np.float64)), 0, torch.from_numpy(order)).numpy())
    return Zg


def _class_stds(Zg, cs, ctx):
    """colstd of every class block of the grouped rows (ncls x d), one jch_col_stats call per class."""
    return np.stack([_col_stats(Zg[cs[c]:cs[c + 1]], None, True, ctx)[1] for c in range(len(cs) - 1)])


def _kernda_models(Zg, cs, stds, dims_list, prior, h, a, lev, ni):
    """One Kernda per entry of dims_list (the model on the first dims columns of the grouped rows), as `kdeda` builds it: a dmkern per class."""
    out = []
    for p in dims_list:
        fm = [_dm_record(Zg[cs[c]:cs[c + 1], :p], _bandwidths(None if stds is None else stds[c], int(ni[c]), p, h, a)) for c in range(len(lev))]
        out.append(Kernda(fm, _wprior(prior, ni), lev, ni))
    return out


def _kde_prepare(X, y, h, prior, who):
    """What `kdeda` and `plskdeda` share ahead of any device work: the checks of y, prior and the class sizes; levels, counts, class offsets."""
    yv = _labels(y)
    n = X.shape[0]
    if yv.shape[0] != n:
        raise ValueError(f"DimensionMismatch: X has {n} rows, y has {yv.shape[0]}")
    lev, ni = np.unique(yv, return_counts=True)
    _wprior(prior, ni)
    cs = np.concatenate([[0], np.cumsum(ni)]).astype(np.int64)
    if h is None and np.any(ni == 1):
        raise ValueError(f"SingularException: {who}: a class of one row and h = None: colstd is 0 and H cannot be inverted")
    return yv, lev, ni, cs


def kdeda(X, y, *, prior: str = "unif", h=None, a=1, ctx: Optional[Context] = None) -> Kernda:
    """`kdeda(X, y; prior = "unif", h = nothing, a = 1)` — src/kdeda.jl:62-79: one `dmkern` per class on that class's rows."""
    X = ensure_mat(X)
    n, p = X.shape
    h, a = _check_h(h, a, p, "kdeda")
    yv, lev, ni, cs = _kde_prepare(X, y, h, prior, "kdeda")
    Zg = _group_by_class(X, yv, lev)
    stds = None
    if h is None:
        for c in range(len(lev)):
            _check_default_h(Zg[cs[c]:cs[c + 1]], int(ni[c]), "kdeda")
        stds = _class_stds(Zg, cs, ctx)
    obj = _kernda_models(Zg, cs, stds, [p], prior, h, a, lev, ni)[0]
    obj._Z, obj._cs = Zg, cs                                   # the grouped rows the Dmkern records are views of
    return obj


def _posterior(wprior, dens):
    """src/kdeda.jl:91-95: A = wprior' .* dens, rows divided by their sums; the argmax takes the first level on ties and on a NaN row."""
    if _is_torch(dens):
        A = torch.as_tensor(wprior, device=dens.device)[None, :] * dens
        post = A / A.sum(dim=1, keepdim=True)
        return post, np.argmax(post.cpu().numpy(), axis=1)
    A = wprior[None, :] * dens
    with np.errstate(invalid="ignore", divide="ignore"):
        post = A / A.sum(axis=1, keepdims=True)
    return post, np.argmax(post, axis=1)


def _grouped(obj: Kernda):
    Zg, cs = getattr(obj, "_Z", None), getattr(obj, "_cs", None)
    if Zg is None:                                             # a record put together by hand: the class blocks, one under the other
        blocks = [ensure_mat(f.X) for f in obj.fm]
        Zg = torch.cat(blocks, 0) if _is_torch(blocks[0]) else np.concatenate(blocks, 0)
        cs = np.concatenate([[0], np.cumsum([b.shape[0] for b in blocks])]).astype(np.int64)
    return Zg, cs


def kdeda_predict(obj: Kernda, X, *, ctx: Optional[Context] = None):
    """`predict(object::Kernda, X)` — src/kdeda.jl:81-97: (pred, dens, posterior); pred m x 1 host labels, dens and posterior m x nlev where X
    lives.  One jch_kde_dens call for all classes."""
    X = ensure_mat(X)
    Zg, cs = _grouped(obj)
    p = Zg.shape[1]
    if X.shape[1] != p:
        raise ValueError(f"DimensionMismatch: X has {X.shape[1]} columns, the model has {p}")
    nlev = len(obj.lev)
    u = np.stack([np.diag(f.Hinv) for f in obj.fm], axis=1)
    coef = np.array([[_norm_coef(int(cs[c + 1] - cs[c]), p, obj.fm[c].detH) for c in range(nlev)]])
    dens = kde_dens(Zg, X, cs, u, np.ones((1, nlev)), coef, [p], ctx=ctx)[:, :, 0]
    post, z = _posterior(np.asarray(obj.wprior, dtype=np.float64), dens)
    return np.asarray(obj.lev)[z].reshape(-1, 1), dens, post


# ---------------------------------------------------------------------------------- plskdeda
def plskdeda(X, y, weights=None, *, nlv: int, prior: str = "unif", h=None, a=1, scal: bool = False, ctx: Optional[Context] = None) -> Plslda:
    """`plskdeda(X, y, weights; nlv, prior = "unif", h = nothing, a = 1, scal = false)` — src/plskdeda.jl:52-64: plskern on `dummy(y)`, then
    `kdeda(T[:, 1:i], y)` for i = 1..nlv; returns the `Plslda` record with fm_da a list of `Kernda`.  `h`: None or a real (a vector fits one of
    the nlv models only and is a dimension mismatch for every other one in the reference: ValueError here)."""
    X = ensure_mat(X)
    if h is not None and np.ndim(h) != 0:
        raise ValueError("DimensionMismatch: plskdeda: a vector h fits the model of one nlv only; give None or a real")
    h, a = _check_h(h, a, 0, "plskdeda")
    yv, lev, ni, cs = _kde_prepare(X, y, h, prior, "plskdeda")
    Yd, _ = dummy(yv)
    Yd = np.asfortranarray(Yd)
    if _is_torch(X):
        Yt = colmajor_empty(Yd.shape[0], Yd.shape[1], X.device); Yt.copy_(torch.from_numpy(Yd)); Yd = Yt
    fm = plskern(X, Yd, weights, nlv=nlv, scal=scal, ctx=ctx)
    k = fm.T.shape[1]
    Zg = _group_by_class(fm.T, yv, lev)
    stds = None
    if h is None:
        for c in range(len(lev)):
            _check_default_h(Zg[cs[c]:cs[c + 1]], int(ni[c]), "plskdeda")
        stds = _class_stds(Zg, cs, ctx)
    fm_da = _kernda_models(Zg, cs, stds, list(range(1, k + 1)), prior, h, a, lev, ni)
    obj = Plslda(fm, fm_da, lev, ni)
    # the separable form of the nlv x nlev inverse bandwidths: 1 / h[a, c, j] = u[j, c] * v[a, c]
    if h is None:
        u = (1.0 / stds).T
        v = np.array([[ni[c] ** (1 / (i + 4)) / a for c in range(len(lev))] for i in range(1, k + 1)])
    else:
        u, v = np.full((k, len(lev)), 1.0 / h), np.ones((k, len(lev)))
    obj._kde = dict(Z=Zg, cs=cs, u=np.asfortranarray(u), v2=v * v)
    return obj


def plskdeda_predict(obj: Plslda, X, *, nlv=None, ctx: Optional[Context] = None):
    """`predict(object::Plslda, X; nlv)` on a `plskdeda` model — src/plslda.jl:107-130: (pred, posterior), lists over the clamped nlv range
    (return shape as `plslda_predict`; a range is clamped to 1..nlv of the fit, so 0:7 on a 5-LV model is 1:5, and nlv = 0 alone, like any
    range without a model in it, raises as there).  ONE `transform` at the largest nlv, then ONE jch_kde_dens call with dims = the range."""
    a = obj.fm_pls.P.shape[1]
    if nlv is None:
        rng = [a]
    else:
        vals = np.atleast_1d(np.asarray(nlv))
        rng = list(range(max(int(vals.min()), 1), min(int(vals.max()), a) + 1))   # (src/plslda.jl:114 clamps to 0:a; there is no model 0)
    if not rng:
        raise ValueError("BoundsError: a discriminant model needs nlv >= 1 (src/plslda.jl:120 indexes fm_da[nlv])")
    st = getattr(obj, "_kde", None)
    if st is None or not isinstance(obj.fm_da[0], Kernda):
        raise TypeError("plskdeda_predict needs a model fitted by plskdeda")
    T = transform(obj.fm_pls, X, nlv=rng[-1], ctx=ctx)
    Z = st["Z"]
    if _is_torch(T) != _is_torch(Z):
        raise TypeError("training data and queries must both be host arrays or both device tensors")
    nlev, kmax = len(obj.lev), rng[-1]
    coef = np.array([[_norm_coef(int(obj.ni[c]), k, obj.fm_da[k - 1].fm[c].detH) for c in range(nlev)] for k in rng])
    dens = kde_dens(Z[:, :kmax], T, st["cs"], st["u"][:kmax], st["v2"][[k - 1 for k in rng]], coef, rng, ctx=ctx)
    preds, posts = [], []
    for i, k in enumerate(rng):
        post, z = _posterior(np.asarray(obj.fm_da[k - 1].wprior, dtype=np.float64), dens[:, :, i])
        preds.append(np.asarray(obj.lev)[z].reshape(-1, 1)); posts.append(post)
    return (preds[0], posts[0]) if len(rng) == 1 else (preds, posts)
