"""Model averaging over the number of latent variables: `fweight` (src/fweight.jl), `wshenk` (src/wshenk.jl), `plsravg` with typf = unif / shenk /
cv / stack (src/plsravg.jl, src/plsravg_unif.jl, src/plsravg_shenk.jl, src/plsravg_cv.jl, src/plsrstack.jl) and the voting discrimination models
`plsrdaavg`, `plsldaavg`, `plsqdaavg` (src/plsrdaavg.jl, src/plsldaavg.jl, src/plsqdaavg.jl) — DESIGN.md §27.

Every model is ONE plskern fit at the largest level; the per-level predictions are the existing one-pass range predict (jch_predict), and the
average is a weighted sum over its level blocks in level order.  The Shenk weights need, per row and per level a, the norm of the X-residual after
a latent variables: the reference forms `nlv` m x p `xresid` matrices (src/wshenk.jl:59-62); here it is one `transform` and one
jch_row_resid_ss_lv (csrc/resid_lv.hip), which walks the levels as rank-one updates of one running residual: two reads of X in all.  What is left
on the caller's side is m x nlv element-wise arithmetic (square roots, reciprocals, the row normalisations) where X lives, and p x q host glue.

The local forms `lwplsravg`, `lwplsrdaavg`, `lwplsldaavg`, `lwplsqdaavg` (src/lwplsravg.jl, src/lwplsrdaavg.jl, ...) sit on the existing batched
entries: typf = "unif" is one local-fit call plus the mean of its levels, the discrimination forms one jch_lwplsda_predict_prepared plus the vote;
typf = "shenk" inside the envelope of the p-space local-fit kernel is one jch_lwplsravg_predict_prepared (the kernel returns the Shenk norms of every
local level); cv, stack and shenk outside the envelope run the reference's per-query schedule (src/locw.jl) here in the mirror.

typf = "aic" / "bic" need `dfplsr_cg`, which this library does not have: NotImplementedError."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .lwplsda import locw_pspace_lds_bytes
from .occ import _colmajor_x
from .plsr import (Plsr, Plsrda, _addr_ld, _is_torch, _model_vec, _np, _pred_matrix, coef, colmajor_empty, ensure_mat, gridcvlv, plskern,
                   plskern_, plslda, plslda_predict, plsqda, plsrda, plsrda_predict, rmsep, segmkf, transform)

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

TYPW = ("bisquare", "cauchy", "epan", "fair", "invexp", "invexp2", "gauss", "trian", "tricube")
TYPF = ("unif", "shenk", "cv", "stack")


# ---------------------------------------------------------------------------------- fweight
def fweight(d, typw: str = "bisquare", alpha=0):
    """`fweight(d; typw, alpha)` — src/fweight.jl:71-91, literally: w = f(|d| / q) with q the (1 - alpha) quantile of the non-NaN |d| (Julia's default
    quantile = numpy's "linear"), 0 where |d| / q > 1 and where the weight is NaN.  Host glue on a vector."""
    if typw not in TYPW:
        raise ValueError(f"typw = {typw!r} must be one of {TYPW}")
    d = np.abs(np.asarray(d, dtype=np.float64)).reshape(-1)
    alpha = max(0, min(1, alpha))
    zd = d[~np.isnan(d)]
    q = np.quantile(zd, 1 - alpha)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = d / q
        w = {"bisquare": lambda x: (1 - x ** 2) ** 2, "cauchy": lambda x: 1 / (1 + x ** 2), "epan": lambda x: 1 - x ** 2,
             "fair": lambda x: 1 / (1 + x) ** 2, "invexp": lambda x: np.exp(-x), "invexp2": lambda x: np.exp(-x / 2),
             "gauss": lambda x: np.exp(-x ** 2), "trian": lambda x: 1 - x, "tricube": lambda x: (1 - x ** 3) ** 3}[typw](d)
        w[d > 1] = 0
    w[np.isnan(w)] = 0
    return w


# ---------------------------------------------------------------------------------- the nested residual sums
def row_resid_ss_lv(X, shift, Z, B, a_lo: int, a_hi: int, *, ctx: Optional[Context] = None):
    """jch_row_resid_ss_lv: out[i, a - a_lo] = sum_j (X[i, j] - shift[j] - sum_{l < a} Z[i, l] B[j, l])^2 for a = a_lo .. a_hi, an
    m x (a_hi - a_lo + 1) column-major matrix where X lives, from ONE read of X.  X m x p and Z m x kz (both host arrays or both device tensors);
    shift (p, or None) and B (p x kz) host arrays; 0 <= a_lo <= a_hi <= kz.  a_hi = 0 (Z = B = None allowed): the centred row sums of squares."""
    X = _colmajor_x(X)
    dev = _is_torch(X)
    m, p = X.shape
    kz = 0 if Z is None else ensure_mat(Z).shape[1]
    a_lo, a_hi = int(a_lo), int(a_hi)
    if not 0 <= a_lo <= a_hi <= kz:
        raise ValueError(f"needs 0 <= a_lo <= a_hi <= kz, got a_lo = {a_lo}, a_hi = {a_hi}, kz = {kz}")
    za, ldz, ba = None, 0, None
    if kz:
        Z = _colmajor_x(Z)
        if _is_torch(Z) != dev:
            raise TypeError("X and Z must both be host arrays or both device tensors")
        if Z.shape[0] != m:
            raise ValueError(f"DimensionMismatch: X has {m} rows, Z has {Z.shape[0]}")
        B = np.asfortranarray(B, dtype=np.float64)
        if B.shape != (p, kz):
            raise ValueError(f"DimensionMismatch: B is {B.shape[0]} x {B.shape[1]}, expected {p} x {kz}")
        za, ldz = _addr_ld(Z)
        ba = B.ctypes.data
    sh = None if shift is None else _model_vec(shift)
    if sh is not None and sh.shape[0] != p:
        raise ValueError(f"DimensionMismatch: X has {p} columns, shift has {sh.shape[0]} entries")
    ctx = ctx or default_context((X.device.index or 0) if dev else 0)
    le = a_hi - a_lo + 1
    if dev:
        out = colmajor_empty(m, le, X.device)
        oa = out.data_ptr()
        torch.cuda.current_stream(X.device).synchronize()
    else:
        out = np.empty((m, le), order="F")
        oa = out.ctypes.data
    xa, ldx = _addr_ld(X)
    ctx.check(_lib.load().jch_row_resid_ss_lv(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, xa, m, p, ldx, _np(sh), za, kz, ldz, ba, max(p, 1),
                                              a_lo, a_hi, oa, max(m, 1)))
    return out


# ---------------------------------------------------------------------------------- wshenk
def _rowsum(A):
    return A.sum(dim=1, keepdim=True) if _is_torch(A) else A.sum(axis=1, keepdims=True)


def _shenk_rss(fm, X, nlv, ctx):
    """(rss_r m x nlv where X lives, rss_b (nlv) on the host) of src/wshenk.jl:59-67 for the levels 1 .. nlv."""
    k = fm.T.shape[1] if nlv is None else min(int(nlv), fm.T.shape[1])
    if k < 1:
        raise ValueError("wshenk needs nlv >= 1")
    X = _colmajor_x(X)
    T = transform(fm, X, nlv=k, ctx=ctx)
    Ps = np.asfortranarray(np.asarray(fm.xscales)[:, None] * np.asarray(fm.P)[:, :k])   # the residuals in the original scale (src/xfit.jl:48-51)
    ss = row_resid_ss_lv(X, fm.xmeans, T, Ps, 1, k, ctx=ctx)
    rss_r = ss.sqrt() if _is_torch(ss) else np.sqrt(ss)
    q = fm.C.shape[0]
    rss_b = np.empty(k)
    for j in range(1, k + 1):
        B, intercept = coef(fm, nlv=j)
        rss_b[j - 1] = np.sqrt((np.sum(intercept ** 2) + np.sum(B ** 2)) / q)
    return rss_r, rss_b


def wshenk(fm, X, nlv: Optional[int] = None, *, ctx: Optional[Context] = None):
    """`wshenk(object::Union{Pcr, Plsr}, X; nlv)` — src/wshenk.jl:46-75: (w, wr, wb), the Shenk et al. "LOCAL" weights of the models with
    1 .. nlv LVs for every row of X.  w and wr (m x nlv) live where X lives; wb (nlv) is a host array.  One `transform` and one
    jch_row_resid_ss_lv with shift = xmeans, B = diag(xscales) P; rss_b comes from `coef` on the host."""
    rss_r, rss_b = _shenk_rss(fm, X, nlv, ctx)
    with np.errstate(divide="ignore", invalid="ignore"):
        wb = 1 / rss_b
        wb = wb / wb.sum()
    wr = 1 / rss_r
    wr = wr / _rowsum(wr)
    w = wr * (torch.as_tensor(wb, device=wr.device) if _is_torch(wr) else wb)
    w = w / _rowsum(w)
    return w, wr, wb


# ---------------------------------------------------------------------------------- plsravg
@dataclass
class PlsravgUnif:
    """src/plsravg_unif.jl:1-4."""
    fm: Plsr
    nlv: range


@dataclass
class PlsravgShenk:
    """src/plsravg_shenk.jl:1-4."""
    fm: Plsr
    nlv: range


@dataclass
class PlsravgCri:
    """src/plsravg_aic.jl:1-5 (what plsravg_cv returns)."""
    fm: Plsr
    nlv: range
    w: np.ndarray


@dataclass
class Plsrstack:
    """src/plsrstack.jl: struct Plsrstack (fm, nlv, w, Xstack, ystack, weightsstack)."""
    fm: Plsr
    nlv: range
    w: np.ndarray
    Xstack: np.ndarray
    ystack: np.ndarray
    weightsstack: np.ndarray


@dataclass
class Plsravg:
    """src/plsravg.jl:1-3."""
    fm: object


def parse_nlv(nlv):
    """The reference evaluates the string ("5:20", "10"); here "lo:hi", "k", an int or a range / sequence give (min, max)."""
    if isinstance(nlv, str):
        parts = nlv.split(":")
        if len(parts) not in (1, 2):
            raise ValueError(f"nlv = {nlv!r} must look like '5:20' or '10'")
        try:
            vals = [int(s) for s in parts]
        except ValueError:
            raise ValueError(f"nlv = {nlv!r} must look like '5:20' or '10'") from None
    else:
        vals = [int(v) for v in np.atleast_1d(np.asarray(nlv)).reshape(-1)]
    if not vals or min(vals) < 0 or (len(vals) == 2 and isinstance(nlv, str) and vals[0] > vals[1]):
        raise ValueError(f"nlv = {nlv!r}: needs 0 <= lo <= hi")
    return min(vals), max(vals)


def _clamped(nlv, n, p):
    lo, hi = parse_nlv(nlv)
    return range(min(lo, n, p), min(hi, n, p) + 1)


def _host(a):
    return a.detach().cpu().numpy() if _is_torch(a) else np.asarray(a)


def _rows(A, s):
    """A[s, :] as a column-major matrix where A lives."""
    if _is_torch(A):
        out = colmajor_empty(len(s), A.shape[1], A.device)
        out.copy_(A[torch.as_tensor(np.asarray(s), dtype=torch.int64, device=A.device)])
        return out
    return np.asfortranarray(A[np.asarray(s)])


def _cv_weights(X, Y, rng, typw, alpha, scal, segm, seed, ctx):
    """src/plsravg_cv.jl:17-23.  The reference's `plsravg` does not hand its K to plsravg_cv (src/plsravg.jl:133-135): the folds are 2 whatever K."""
    n = ensure_mat(X).shape[0]
    segm = segmkf(n, 2, rep=1, seed=seed) if segm is None else segm
    res = gridcvlv(X, Y, segm=segm, score=rmsep, fun=plskern, nlv=range(0, rng[-1] + 1), pars=dict(scal=[scal]), ctx=ctx)["res"]
    z = res.mean(axis=1)
    d = (z - z.min())[np.asarray(rng)]
    w = fweight(d, typw=typw, alpha=alpha)
    with np.errstate(divide="ignore", invalid="ignore"):
        return w / w.sum()


def _stack_weights(X, Y, weights, rng, K, rep, scal, segm, seed, ctx):
    """src/plsrstack.jl:12-50: the CV predictions of the levels 0 .. nlvmax, replications and segments stacked, regressed on the observed y
    without intercept.  Each fold is one weight-0 fit on the X that stays where it is (gridcvlv's schedule, the reuse_x path); the held-out rows
    are predicted by the one-pass range predict; the le x le normal equations are solved by Cholesky on the host."""
    n = ensure_mat(X).shape[0]
    if ensure_mat(Y).shape[1] != 1:
        raise ValueError("typf = 'stack' needs a univariate Y (src/plsrstack.jl:49)")
    segm = segmkf(n, K, rep=rep, seed=seed) if segm is None else segm
    wn = np.ones(n) if weights is None else _host(weights).astype(np.float64).reshape(-1)
    wn = wn / wn.sum()
    dev = _is_torch(X)
    nlvmax = rng[-1]
    Xs, ys, ws = [], [], []
    same_x = False
    for listsegm in segm:
        for s in listsegm:
            s = np.asarray(s)
            wcal = wn.copy(); wcal[s] = 0.0
            wfit = torch.as_tensor(wcal, device=X.device) if dev else wcal
            zfm = plskern(X, Y, wfit, nlv=nlvmax, scal=scal, ctx=ctx, reuse_x=same_x)
            same_x = True
            Xs.append(_host(_pred_matrix(zfm, _rows(X, s), list(range(0, nlvmax + 1)), ctx)))
            ys.append(_host(_rows(ensure_mat(Y), s)))
            ws.append(wn[s])
    Xstack, ystack, wstack = np.vstack(Xs), np.vstack(ys), np.concatenate(ws)
    wstack = wstack / wstack.sum()
    Xstack = Xstack[:, np.asarray(rng)]
    XtD = Xstack.T * wstack[None, :]
    L = np.linalg.cholesky(XtD @ Xstack)
    w = np.linalg.solve(L.T, np.linalg.solve(L, XtD @ ystack)).reshape(-1)
    return w, Xstack, ystack, wstack


def _plsravg(fit, X, Y, weights, nlv, typf, typw, alpha, K, rep, scal, segm, seed, ctx):
    if typf in ("aic", "bic"):
        raise NotImplementedError(f"typf = {typf!r} needs dfplsr_cg, which is not in this library")
    if typf not in TYPF:
        raise ValueError(f"typf = {typf!r} must be one of {TYPF + ('aic', 'bic')}")
    if typw not in TYPW:
        raise ValueError(f"typw = {typw!r} must be one of {TYPW}")
    X = ensure_mat(X); Y = ensure_mat(Y)
    n, p = X.shape
    rng = _clamped(nlv, n, p)
    nlvmax = rng[-1]
    if typf == "shenk":
        rng = range(max(rng[0], 1), nlvmax + 1)                      # src/plsravg_shenk.jl:18
        if nlvmax < 1:
            raise ValueError("typf = 'shenk' needs a level >= 1")
    extra = ()
    if typf == "cv":                                                 # (before the fit: the in-place form destroys X)
        extra = (_cv_weights(X, Y, rng, typw, alpha, scal, segm, seed, ctx),)
    elif typf == "stack":
        extra = _stack_weights(X, Y, weights, rng, K, rep, scal, segm, seed, ctx)
    fm = fit(X, Y, weights, nlv=nlvmax, scal=scal, ctx=ctx)
    cls = dict(unif=PlsravgUnif, shenk=PlsravgShenk, cv=PlsravgCri, stack=Plsrstack)[typf]
    return Plsravg(cls(fm, rng, *extra))


def plsravg(X, Y, weights=None, *, nlv, typf: str = "unif", typw: str = "bisquare", alpha=0, K: int = 5, rep: int = 10, scal: bool = False,
            segm=None, seed=None, ctx: Optional[Context] = None) -> Plsravg:
    """`plsravg(X, Y, weights; nlv, typf, typw, alpha, K, rep, scal)` — src/plsravg.jl:109-149.  `nlv` = "lo:hi" or "k" (clamped to min(n, p));
    typf = "unif", "shenk", "cv" (weights fweight(rmsep_cv - min) from `gridcvlv` with 2 folds) or "stack" (K folds x rep).  The segments are an
    argument as everywhere in this package: `segm` (list of replications, each a list of 0-based index vectors), else drawn from `seed`."""
    return _plsravg(plskern, X, Y, weights, nlv, typf, typw, alpha, K, rep, scal, segm, seed, ctx)


def plsravg_(X, Y, weights=None, *, nlv, typf: str = "unif", typw: str = "bisquare", alpha=0, K: int = 5, rep: int = 10, scal: bool = False,
             segm=None, seed=None, ctx: Optional[Context] = None) -> Plsravg:
    """`plsravg!`: the final fit is plskern_ on the caller's X and Y (column-major float64), as the reference's `plskern!`."""
    return _plsravg(plskern_, X, Y, weights, nlv, typf, typw, alpha, K, rep, scal, segm, seed, ctx)


def plsravg_predict(obj: Plsravg, X, *, ctx: Optional[Context] = None):
    """`predict(object::Plsravg, X)` — (pred, predlv), and (pred, predlv, w) for typf = "shenk" (src/plsravg_shenk.jl:24-47; w is None for a single
    level, where the reference leaves it undefined).  predlv is the one-pass range predict (a matrix for one level, else a list); pred is the weighted
    sum over its level blocks in level order, where X lives."""
    sub = obj.fm
    fm, rng = sub.fm, sub.nlv
    le, q = len(rng), fm.C.shape[0]
    X = _colmajor_x(X)
    out = _pred_matrix(fm, X, list(rng), ctx)
    blocks = [out[:, i * q:(i + 1) * q] for i in range(le)]
    shenk = isinstance(sub, PlsravgShenk)
    if le == 1:
        return (blocks[0], blocks[0], None) if shenk else (blocks[0], blocks[0])
    if isinstance(sub, PlsravgUnif):
        acc = blocks[0].clone() if _is_torch(out) else blocks[0].copy()
        for b in blocks[1:]:
            acc += b
        return acc / le, blocks
    if shenk:
        w = wshenk(fm, X, ctx=ctx)[0][:, rng[0] - 1:rng[-1]]
        zw = w / _rowsum(w)
        acc = zw[:, 0:1] * blocks[0]
        for j in range(1, le):
            acc += zw[:, j:j + 1] * blocks[j]
        return acc, blocks, w
    acc = float(sub.w[0]) * blocks[0]
    for j in range(1, le):
        acc += float(sub.w[j]) * blocks[j]
    return acc, blocks


# ---------------------------------------------------------------------------------- plsrdaavg, plsldaavg, plsqdaavg
@dataclass
class Plsdaavg:
    """src/plsrdaavg.jl:1-7 — struct Plsdaavg (fm, nlv, w_mod, lev, ni); fm a Plsrda or a Plslda record."""
    fm: object
    nlv: range
    w_mod: np.ndarray
    lev: np.ndarray
    ni: np.ndarray


def findmax_cla(x, weights=None, lev=None):
    """`findmax_cla(x, weights)` — src/utility.jl:564-570: the label with the largest summed weight; `aggstat` sorts the labels and `argmax` takes
    the first maximum, so a tie goes to the smallest label."""
    x = np.asarray(x).reshape(-1)
    w = np.ones(x.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    lev = np.unique(x) if lev is None else np.asarray(lev)
    tot = np.zeros(len(lev))
    np.add.at(tot, np.searchsorted(lev, x), w)
    return lev[np.argmax(tot)]


def vote(labels, w_mod, lev):
    """Row-wise findmax_cla of an m x le label table over the sorted labels `lev`: (m x 1) labels."""
    labels = np.asarray(labels)
    m, le = labels.shape
    tot = np.zeros((m, len(lev)))
    codes = np.searchsorted(lev, labels)
    for j in range(le):                                              # level order: the sums are formed as aggstat forms them
        np.add.at(tot, (np.arange(m), codes[:, j]), w_mod[j])
    return np.asarray(lev)[np.argmax(tot, axis=1)].reshape(-1, 1)


def _daavg(fit, lowest, X, y, weights, nlv, scal, ctx, **kw):
    X = ensure_mat(X)
    n, p = X.shape
    lo, nlvmax = parse_nlv(nlv)
    rng = range(max(lo, 0), min(nlvmax, n, p) + 1)
    if len(rng) == 0 or rng[0] < lowest:
        raise ValueError(f"nlv = {nlv!r}: a discriminant model on the scores needs levels >= {lowest}")
    w_mod = np.ones(len(rng)) / len(rng)                             # uniform weights for the models
    fm = fit(X, y, weights, nlv=nlvmax, scal=scal, ctx=ctx, **kw)
    return Plsdaavg(fm, rng, w_mod, fm.lev, fm.ni)


def plsrdaavg(X, y, weights=None, *, nlv, scal: bool = False, ctx: Optional[Context] = None) -> Plsdaavg:
    """`plsrdaavg(X, y, weights; nlv, scal)` — src/plsrdaavg.jl:58-71: plsrda at the largest level, uniform vote over the levels lo .. hi (lo = 0
    is allowed here: the level-0 model predicts from the class frequencies)."""
    return _daavg(plsrda, 0, X, y, weights, nlv, scal, ctx)


def plsldaavg(X, y, weights=None, *, nlv, prior: str = "unif", scal: bool = False, ctx: Optional[Context] = None) -> Plsdaavg:
    """`plsldaavg` — src/plsldaavg.jl:60-74, levels >= 1.  `prior` goes to plslda (the reference leaves it at its default "unif")."""
    return _daavg(plslda, 1, X, y, weights, nlv, scal, ctx, prior=prior)


def plsqdaavg(X, y, weights=None, *, nlv, prior: str = "unif", scal: bool = False, ctx: Optional[Context] = None) -> Plsdaavg:
    """`plsqdaavg` — src/plsqdaavg.jl:24-38, levels >= 1."""
    return _daavg(plsqda, 1, X, y, weights, nlv, scal, ctx, prior=prior)


def plsdaavg_predict(obj: Plsdaavg, X, *, ctx: Optional[Context] = None):
    """`predict(object::Plsdaavg, X)` — src/plsrdaavg.jl:80-97: (pred, predlv); the per-level labels are the existing range predict of plsrda /
    plslda / plsqda, pred their row-wise `findmax_cla` under w_mod (m x le labels: host glue)."""
    rng = obj.nlv
    one = plsrda_predict if isinstance(obj.fm, Plsrda) else plslda_predict
    preds = one(obj.fm, X, nlv=list(rng), ctx=ctx)[0]
    if len(rng) == 1:
        return preds, preds
    return vote(np.hstack(preds), obj.w_mod, obj.lev), preds


# ---------------------------------------------------------------------------------- lwplsravg, lwplsrdaavg, lwplsldaavg, lwplsqdaavg
@dataclass
class LwplsrAvg:
    """src/lwplsravg.jl:1-17 — same fields (`nlv` is the range string)."""
    X: object
    Y: object
    fm: Optional[Plsr]
    metric: str
    h: float
    k: int
    nlv: object
    typf: str
    typw: str
    alpha: float
    K: int
    rep: int
    tol: float
    scal: bool
    verbose: bool = False


@dataclass
class LwplsdaAvg:
    """src/lwplsrdaavg.jl:1-14 / lwplsldaavg.jl / lwplsqdaavg.jl — `fm` is the Lwplsrda / LwplsLda / LwplsQda record fitted at the largest level
    (its fields are the reference's X, y, fm, metric, h, k, tol, scal, verbose, lev, ni), `nlv` the range string, `rng` the clamped levels."""
    fm: object
    nlv: object
    rng: range


def _local_range(nlv, k, p, lowest=0):
    """The reference clamps inside the model fitted on a neighbourhood, i.e. with n = k: lo = min(lo, k, p), hi = min(hi, k, p), once, so that
    the levels are distinct."""
    lo, hi = parse_nlv(nlv)
    return range(max(min(lo, k, p), lowest), min(hi, k, p) + 1)


def lwplsravg(X, Y, *, nlvdis: int, metric: str, h: float, k: int, nlv, typf: str = "unif", typw: str = "bisquare", alpha=0, K: int = 5,
              rep: int = 10, tol: float = 1e-4, scal: bool = False, verbose: bool = False, ctx: Optional[Context] = None) -> LwplsrAvg:
    """`lwplsravg(X, Y; nlvdis, metric, h, k, nlv, typf, typw, alpha, K, rep, tol, scal, verbose)` — src/lwplsravg.jl:100-112: kNN-LWPLSR-AVG; stores
    the data and (nlvdis > 0) the global plskern fit whose scores define the neighbourhoods."""
    from .plsr import lwplsr
    if typf in ("aic", "bic"):
        raise NotImplementedError(f"typf = {typf!r} needs dfplsr_cg, which is not in this library")
    if typf not in TYPF:
        raise ValueError(f"typf = {typf!r} must be one of {TYPF + ('aic', 'bic')}")
    if typw not in TYPW:
        raise ValueError(f"typw = {typw!r} must be one of {TYPW}")
    parse_nlv(nlv)
    base = lwplsr(X, Y, nlvdis=nlvdis, metric=metric, h=h, k=k, nlv=0, tol=tol, scal=scal, ctx=ctx)
    return LwplsrAvg(base.X, base.Y, base.fm, metric, h, int(k), nlv, typf, typw, alpha, int(K), int(rep), tol, bool(scal), bool(verbose))


def _avg_engine(obj: LwplsrAvg, hi: int):
    """The `Lwplsr` this model searches and (typf = "unif") fits through, kept with the object so that its prepared handle is reused."""
    from .plsr import Lwplsr
    key = (obj.metric, obj.h, obj.k, obj.tol, obj.scal, hi)
    st = obj.__dict__.get("_lw_engine")
    # (the engine holds the arrays it was built on, so "the same data" is an identity test on live objects, never on a recycled id)
    if st is None or st[0] != key or st[1].X is not obj.X or st[1].Y is not obj.Y or st[1].fm is not obj.fm:
        st = (key, Lwplsr(obj.X, obj.Y, obj.fm, obj.metric, obj.h, obj.k, hi, obj.tol, obj.scal, False))
        obj.__dict__["_lw_engine"] = st
    return st[1]


def lwplsravg_predict(obj: LwplsrAvg, X, *, seed=None, ctx: Optional[Context] = None):
    """`predict(object::LwplsrAvg, X)` — src/lwplsravg.jl:120-150: LwplsrPred(pred, listnn, listd, listw); listnn is 0-based.

    typf = "unif": ONE batched local-fit call for the clamped level range (the kernels of `lwplsr_predict`) and the mean over its levels in level
    order.  typf = "shenk" inside the envelope of the p-space local-fit kernel (p <= 2048, q <= 16, levels <= 48, locw_pspace_lds_bytes <= 150 KiB):
    ONE jch_lwplsravg_predict_prepared — the kernel returns the two Shenk norms per level, the result is an LwplsrAvgPred that also carries pred_lv, wlv,
    rss_r, rss_b and info; one warning when a query has info = 2 (a norm 0 or not finite: NaN, as the reference's arithmetic gives).
    Every other case runs the reference's own schedule (src/locw.jl): one search and one set of weights from the same prepared handle,
    then `plsravg` on the gathered neighbourhood of each query with the weights of that query, a neighbourhood with a constant univariate y
    predicting that value.  Slower, never absent.  The segments of `cv` / `stack` of query i are drawn from (seed, i)."""
    from .plsr import LwplsrPred, lwplsr_predict
    X = ensure_mat(X)
    n, p = obj.X.shape
    k = min(int(obj.k), n)
    rng = _local_range(obj.nlv, k, p, 1 if obj.typf == "shenk" else 0)
    if len(rng) == 0:
        raise ValueError(f"nlv = {obj.nlv!r}: no level left after the clamp to k = {k}, p = {p}")
    eng = _avg_engine(obj, rng[-1])
    if obj.typf == "unif":
        res = lwplsr_predict(eng, X, nlv=rng, ctx=ctx)
        blocks = res.pred if isinstance(res.pred, list) else [res.pred]
        acc = blocks[0].copy()
        for b in blocks[1:]:
            acc += b
        return LwplsrPred(acc / len(blocks) if len(blocks) > 1 else acc, res.listnn, res.listd, res.listw)
    q = ensure_mat(obj.Y).shape[1]
    if obj.typf == "shenk" and p <= 2048 and q <= 16 and rng[-1] <= 48 and locw_pspace_lds_bytes(k, p, q) <= 150 * 1024:
        return _lwplsravg_shenk_batched(obj, eng, X, k, rng, ctx)
    if ctx is not None and getattr(ctx, "nranks", 1) > 1:
        # the loop below fits `plsravg` per query through the collective entries (jch_plskern_fit, jch_col_stats, ...): on a joined ctx those
        # would all-reduce with whatever the other ranks' queries are fitting (include/jchemo_hip.h, the joined ctx contract)
        raise _lib.JchError(_lib.JCH_EINVAL, f"lwplsravg_predict: the per-query schedule is one rank only (communicator of {ctx.nranks})")
    res = lwplsr_predict(eng, X, nlv=0, ctx=ctx)                    # the search and the weights (level 0: the weighted means)
    m = X.shape[0]
    dev = _is_torch(obj.X)
    Xq = X if dev == _is_torch(X) else None
    if Xq is None:
        raise TypeError("training data and queries must both be host arrays or both device tensors")
    pred = np.empty((m, q))
    Yh = _host(ensure_mat(obj.Y))
    for i in range(m):
        if obj.verbose:
            print(i + 1, end=" ")
        s = res.listnn[i].astype(np.int64)
        zY = Yh[s]
        if q == 1 and len(np.unique(zY)) == 1:                      # src/locw.jl:34-36
            pred[i] = zY[0, 0]
            continue
        w = torch.as_tensor(res.listw[i], device=obj.X.device) if dev else np.ascontiguousarray(res.listw[i])
        fm = plsravg(_rows(obj.X, s), _rows(ensure_mat(obj.Y), s), w, nlv=obj.nlv, typf=obj.typf, typw=obj.typw, alpha=obj.alpha, K=obj.K,
                     rep=obj.rep, scal=obj.scal, seed=None if seed is None else [int(seed), i], ctx=ctx)
        pred[i] = _host(plsravg_predict(fm, _rows(Xq, [i]), ctx=ctx)[0])[0]
    if obj.verbose:
        print()
    if obj.typf == "shenk":
        _warn_shenk(int(np.isnan(pred).any(axis=1).sum()), m)
    return LwplsrPred(pred, res.listnn, res.listd, res.listw)


def _warn_shenk(nbad, m):
    if nbad:
        warnings.warn(f"lwplsravg_predict: {nbad} of {m} queries have a Shenk norm that is 0 or not finite; their predictions are NaN, as the "
                      "reference's arithmetic gives", RuntimeWarning, stacklevel=3)


@dataclass
class LwplsrAvgPred:
    """`LwplsrPred` (pred, listnn, listd, listw) with what the batched Shenk call also returns: pred_lv (list of the le level predictions), wlv (m x le),
    rss_r and rss_b (m x hi, the levels 1 .. hi), info (m: 0 fitted, 1 constant neighbourhood, 2 a Shenk norm 0 or not finite) and nlv, the clamped range."""
    pred: object
    listnn: np.ndarray
    listd: np.ndarray
    listw: np.ndarray
    pred_lv: object = None
    wlv: object = None
    rss_r: object = None
    rss_b: object = None
    info: object = None
    nlv: object = None


def lwplsravg_prepared_call(eng, X, k, lo, hi, typf, ctx):
    """jch_lwplsravg_predict_prepared on the engine's prepared handle: (pred, pred_lv (m, le, q), wlv, rss_r, rss_b, info, ind, dist, w), host arrays.
    lo, hi: the level range BEFORE the library's clamp (it clamps with n = k itself; the outputs are sized with the clamped values)."""
    from .plsr import _as_colmajor_copy, _lwplsr_prepared
    X = ensure_mat(X)
    try:
        _addr_ld(X)
    except (ValueError, TypeError):
        X = _as_colmajor_copy(X)
    dev = _is_torch(X)
    if dev != _is_torch(eng.X):
        raise TypeError("training data and queries must both be host arrays or both device tensors")
    ctx = ctx or default_context((X.device.index or 0) if dev else 0)
    n, p = eng.X.shape
    m, q = X.shape[0], ensure_mat(eng.Y).shape[1]
    k = min(int(k), n)
    hic = min(hi, k, p)
    loc_ = max(min(lo, k, p), 1) if typf == 1 else min(lo, k, p)
    le = hic - loc_ + 1
    if le < 1:
        raise ValueError(f"no level left after the clamp (nlv {lo} .. {hi}, k = {k}, p = {p})")
    st = _lwplsr_prepared(eng, ctx, dev, q)
    pred = np.empty((m, q)); pred_lv = np.empty((m, le, q)); wlv = np.empty((m, le)); rr = np.full((m, max(hic, 1)), np.nan); rb = np.full((m, max(hic, 1)), np.nan)
    info = np.zeros(m, dtype=np.int32); ind = np.empty((m, k), dtype=np.int32); dist = np.empty((m, k)); w = np.empty((m, k))
    if st["device_map"]:
        qa, ldq = None, 0
    else:
        Zq = st["qmap"](X)
        qa, ldq = _addr_ld(Zq)
    xqa, ldxq = _addr_ld(X)
    if dev:
        torch.cuda.current_stream(X.device).synchronize()
    ctx.check(_lib.load().jch_lwplsravg_predict_prepared(ctx._h, st["handle"], _lib.LOC_DEVICE if dev else _lib.LOC_HOST, qa, ldq, xqa, m, ldxq, k, float(eng.h),
                                                         float(eng.tol), int(eng.scal), int(lo), int(hi), int(typf), pred.ctypes.data, pred_lv.ctypes.data,
                                                         wlv.ctypes.data, rr.ctypes.data, rb.ctypes.data, info.ctypes.data, ind.ctypes.data, dist.ctypes.data,
                                                         w.ctypes.data))
    return pred, pred_lv, wlv, rr, rb, info, ind, dist, w


def _lwplsravg_shenk_batched(obj, eng, X, k, rng, ctx):
    pred, pred_lv, wlv, rr, rb, info, ind, dist, w = lwplsravg_prepared_call(eng, X, k, rng[0], rng[-1], 1, ctx)
    _warn_shenk(int((info == 2).sum()), pred.shape[0])
    if obj.verbose:
        print("".join(f"{i} " for i in range(1, pred.shape[0] + 1)))
    return LwplsrAvgPred(pred, ind, dist, w, [pred_lv[:, a, :].copy() for a in range(pred_lv.shape[1])], wlv, rr, rb, info, rng)


def _lwdaavg(fit, lowest, X, y, nlv, k, kw):
    n, p = ensure_mat(X).shape
    rng = _local_range(nlv, min(int(k), n), p, 0)
    if len(rng) == 0 or rng[0] < lowest:
        raise ValueError(f"nlv = {nlv!r}: a discriminant model on the scores needs levels >= {lowest}")
    return LwplsdaAvg(fit(X, y, k=k, nlv=rng[-1], **kw), nlv, rng)


def lwplsrdaavg(X, y, *, nlvdis, metric, h, k, nlv, tol: float = 1e-4, scal: bool = False, verbose: bool = False,
                ctx: Optional[Context] = None) -> LwplsdaAvg:
    """`lwplsrdaavg(X, y; nlvdis, metric, h, k, nlv, tol, scal, verbose)` — src/lwplsrdaavg.jl:94-107; level 0 allowed."""
    from .lwplsda import lwplsrda
    return _lwdaavg(lwplsrda, 0, X, y, nlv, k, dict(nlvdis=nlvdis, metric=metric, h=h, tol=tol, scal=scal, verbose=verbose, ctx=ctx))


def lwplsldaavg(X, y, *, nlvdis, metric, h, k, nlv, prior: str = "unif", tol: float = 1e-4, scal: bool = False, verbose: bool = False,
                ctx: Optional[Context] = None) -> LwplsdaAvg:
    """`lwplsldaavg` — src/lwplsldaavg.jl, levels >= 1."""
    from .lwplsda import lwplslda
    return _lwdaavg(lwplslda, 1, X, y, nlv, k, dict(nlvdis=nlvdis, metric=metric, h=h, prior=prior, tol=tol, scal=scal, verbose=verbose, ctx=ctx))


def lwplsqdaavg(X, y, *, nlvdis, metric, h, k, nlv, prior: str = "unif", tol: float = 1e-4, scal: bool = False, verbose: bool = False,
                ctx: Optional[Context] = None) -> LwplsdaAvg:
    """`lwplsqdaavg` — src/lwplsqdaavg.jl, levels >= 1."""
    from .lwplsda import lwplsqda
    return _lwdaavg(lwplsqda, 1, X, y, nlv, k, dict(nlvdis=nlvdis, metric=metric, h=h, prior=prior, tol=tol, scal=scal, verbose=verbose, ctx=ctx))


def lwplsdaavg_predict(obj: LwplsdaAvg, X, *, ctx: Optional[Context] = None):
    """`predict(object::LwplsrdaAvg, X)` and its lda / qda siblings — src/lwplsrdaavg.jl:115-145: ONE jch_lwplsda_predict_prepared over the clamped
    range (the same search, the same weights), then the uniform `findmax_cla` vote over that call's per-level labels on the host.  A unanimous
    neighbourhood gives its class at every level and so as the vote; a level flagged info = 2 contributes the label that call gives it.
    Returns LwplsdaPred(pred, listnn, listd, listw, posterior = None, info (m x le))."""
    from .lwplsda import LwplsdaPred, LwplsQda, LwplsLda, lwplslda_predict, lwplsqda_predict, lwplsrda_predict
    one = lwplsqda_predict if isinstance(obj.fm, LwplsQda) else lwplslda_predict if isinstance(obj.fm, LwplsLda) else lwplsrda_predict
    res = one(obj.fm, X, nlv=obj.rng, ctx=ctx)
    le = len(obj.rng)
    if le == 1:
        return LwplsdaPred(res.pred, res.listnn, res.listd, res.listw, None, np.asarray(res.info).reshape(-1, 1))
    pred = vote(np.hstack(res.pred), np.ones(le) / le, np.asarray(obj.fm.lev))
    return LwplsdaPred(pred, res.listnn, res.listd, res.listw, None, res.info)
