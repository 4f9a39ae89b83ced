"""One-class classification by score distance, orthogonal distance and their compromise — host-side mirror of the reference's src/occsd.jl,
src/occod.jl and src/occsdod.jl over jch_row_resid_ss, jch_transform, jch_affine_gemm and jch_weighted_cov (include/jchemo_hip.h).

numpy in gives numpy out; a device torch tensor in keeps every m-sized result (the columns of the tables, `e_cdf`, `pred`) on the device.  The
nlv-sized results (`Sinv`, `cutoff`) are host values either way.  The tables are dicts of columns (`d`, `dstand`, `pval`, and `gh` for the score
distance), as `summary` returns; `pred` is an int64 m x 1 matrix.

No m x p residual is formed.  The orthogonal distance is the row norm of e_i = (x_i - xmeans) - Ps t_i with Ps = diag(xscales) P_k
(src/xfit.jl:47-51), summed by jch_row_resid_ss straight from X and the scores.  The score distance is t' Sinv t = |Lc' t|^2 with Sinv = Lc Lc':
the same primitive with k = 0 on U = T Lc, and in `predict` Lc is folded into the loadings, so U comes from one pass over X.

Deviations from the reference: `kwargs` are not taken (the reference passes them to a `kde` it never calls here); `occsdod` does not rename the
columns of `fm_sd.d` and `fm_od.d` in place (the reference's `rename!` does, so that its `fm_sd.d` ends up with the `_sd` names).  The cutoffs use
`mad` with StatsBase 0.33 / 0.34's default `normalize = true`."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .plsr import _addr_ld, _affine, _as_colmajor_copy, _cov_uncorrected, _is_torch, _model_vec, _np, _x_out, ensure_mat, kpca_transform, transform

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

MAD_CONSTANT = 1.4826022185056018   # StatsBase 0.33 / 0.34 `mad(x)`: normalize = true multiplies by 1 / quantile(Normal(), 3 / 4)


@dataclass
class Occsd:
    """The reference's `Occsd` (src/occsd.jl:1-8): d (the table: d, dstand, pval, gh), fm, Sinv (nlv x nlv), e_cdf (the sorted training d, where
    T lives), cutoff, nlv.  Then Lc (nlv x nlv, Sinv = Lc Lc'), which `predict` folds into the loadings."""
    d: dict
    fm: object
    Sinv: np.ndarray
    e_cdf: object
    cutoff: float
    nlv: int
    Lc: np.ndarray


@dataclass
class Occod:
    """The reference's `Occod` (src/occod.jl:1-7): d (the table: d, dstand, pval), fm, e_cdf (the sorted training d, where X lives), cutoff, nlv."""
    d: dict
    fm: object
    e_cdf: object
    cutoff: float
    nlv: int


@dataclass
class Occsdod:
    """The reference's `Occsdod` (src/occsdod.jl:1-5): d (the columns of fm_sd.d suffixed _sd, those of fm_od.d suffixed _od, then dstand),
    fm_sd, fm_od."""
    d: dict
    fm_sd: Occsd
    fm_od: Occod


@dataclass
class OccPred:
    """What the reference's `predict` returns for the three models: (pred = int64 m x 1, d = the table)."""
    pred: object
    d: dict


def _kind(fm) -> str:
    return type(fm).__name__


def _colmajor_x(X):
    X = ensure_mat(X)
    if not _is_torch(X):
        X = np.asarray(X)
    try:
        _addr_ld(X)
    except (ValueError, TypeError):
        X = _as_colmajor_copy(X)
    if _is_torch(X) and not X.is_cuda:
        raise TypeError("torch inputs must live on the GPU (host data: pass numpy arrays)")
    return X


def row_resid_ss(X, shift=None, Z=None, B=None, *, ctx: Optional[Context] = None):
    """jch_row_resid_ss: out[i] = sum_j (X[i, j] - shift[j] - sum_l Z[i, l] B[j, l])^2, an m-vector where X lives.  X m x p and Z m x k (both host
    arrays or both device tensors, column-major); shift (p) and B (p x k) host arrays.  Z = B = None (k = 0): the centred row sums of squares."""
    X = _colmajor_x(X)
    dev = _is_torch(X)
    m, p = X.shape
    k = 0 if Z is None else ensure_mat(Z).shape[1]
    za, ldz, ba = None, 0, None
    if k:
        Z = _colmajor_x(Z)
        if _is_torch(Z) != dev:
            raise TypeError("X and Z must both be host arrays or both device tensors")
        if Z.shape[0] != m:
            raise ValueError(f"DimensionMismatch: X has {m} rows, Z has {Z.shape[0]}")
        B = np.asfortranarray(B, dtype=np.float64)
        if B.shape != (p, k):
            raise ValueError(f"DimensionMismatch: B is {B.shape[0]} x {B.shape[1]}, expected {p} x {k}")
        za, ldz = _addr_ld(Z)
        ba = B.ctypes.data
    sh = None if shift is None else _model_vec(shift)
    if sh is not None and sh.shape[0] != p:
        raise ValueError(f"DimensionMismatch: X has {p} columns, shift has {sh.shape[0]} entries")
    ctx = ctx or default_context((X.device.index or 0) if dev else 0)
    if dev:
        out = torch.empty(m, dtype=torch.float64, device=X.device)
        oa = out.data_ptr()
        torch.cuda.current_stream(X.device).synchronize()
    else:
        out = np.empty(m)
        oa = out.ctypes.data
    xa, ldx = _addr_ld(X)
    ctx.check(_lib.load().jch_row_resid_ss(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, xa, m, p, ldx, _np(sh), za, k, ldz, ba, max(p, 1), oa))
    return out


# ---------------------------------------------------------------------------------- cutoffs, on sorted d
def _sort(d):
    return torch.sort(d).values if _is_torch(d) else np.sort(d)


def _median_sorted(s) -> float:
    """The mean of the two middle values for even n (`torch.median` returns the lower one)."""
    n = s.shape[0]
    return (float(s[(n - 1) // 2]) + float(s[n // 2])) / 2 if n % 2 == 0 else float(s[n // 2])


def _quantile_sorted(s, q: float) -> float:
    """Julia's `quantile(v, q)` default (type 7, alpha = beta = 1; Statistics `_quantile`): linear between the order statistics."""
    n = s.shape[0]
    aleph = n * q + (1.0 - q)
    j = int(min(max(np.floor(aleph), 1), max(n - 1, 1)))
    g = min(max(aleph - j, 0.0), 1.0)
    a = float(s[j - 1])
    b = float(s[min(j, n - 1)])
    return a + g * (b - a)


def _mad_sorted(s, med: float) -> float:
    dev = torch.abs(s - med) if _is_torch(s) else np.abs(s - med)
    return MAD_CONSTANT * _median_sorted(_sort(dev))


def _cutoff(s, typc: str, cri, alpha) -> float:
    if typc == "mad":
        med = _median_sorted(s)
        return med + float(cri) * _mad_sorted(s, med)        # src/occsd.jl:138
    if typc == "q":
        return _quantile_sorted(s, 1.0 - float(alpha))         # :139
    raise ValueError(f'typc = {typc!r} must be "mad" or "q"')


def _pval(e_cdf, d):
    """`pval(e_cdf, q)` (src/utility.jl): 1 - ecdf(q), ecdf(q) = #(training d <= q) / n by a right-sided search in the sorted training d."""
    n = e_cdf.shape[0]
    if _is_torch(d):
        cnt = torch.searchsorted(e_cdf, d.contiguous(), right=True).to(torch.float64)
    else:
        cnt = np.searchsorted(e_cdf, d, side="right").astype(np.float64)
    return 1.0 - _div(cnt, n)


def _div(a, b):
    """a / b for a host scalar b, correctly rounded on both sides: torch divides a device tensor by a host scalar as a product with 1 / b, which
    differs from numpy's quotient in the last bit, so the divisor goes to the device first."""
    return a / torch.tensor(float(b), dtype=a.dtype, device=a.device) if _is_torch(a) else a / float(b)


def _sqrt(a):
    return torch.sqrt(a) if _is_torch(a) else np.sqrt(a)


def _pred(dstand):
    if _is_torch(dstand):
        return (dstand > 1).to(torch.int64).reshape(-1, 1)
    return (dstand > 1).astype(np.int64).reshape(-1, 1)


def _check_cut(typc, cri, alpha):
    if typc not in ("mad", "q"):
        raise ValueError(f'typc = {typc!r} must be "mad" or "q"')
    if typc == "q" and not 0.0 <= float(alpha) <= 1.0:
        raise ValueError(f"alpha = {alpha} must lie in [0, 1]")


def _nlv(fm, nlv, lowest):
    a = fm.T.shape[1]
    if nlv is None:
        return a
    if isinstance(nlv, bool) or int(nlv) != nlv or int(nlv) < lowest:
        raise ValueError(f"nlv = {nlv} must be an integer >= {lowest}")
    return min(int(nlv), a)


# ---------------------------------------------------------------------------------- score distance
def _loadings(fm):
    return fm.P if _kind(fm) == "Pca" else fm.R


def occsd(fm, *, nlv: Optional[int] = None, typc: str = "mad", cri=3, alpha=.025, ctx: Optional[Context] = None) -> Occsd:
    """`occsd(object::Union{Pca, Kpca, Plsr}; nlv, typc = "mad", cri = 3, alpha = .025)` — src/occsd.jl:129-145.  S = cov(T[:, 1:nlv], corrected =
    false) through jch_weighted_cov (about the column means, while the distances are measured from zero, as the reference does), Sinv by a host
    Cholesky; with Sinv = Lc Lc', d2 = |Lc' t|^2: U = T Lc by jch_affine_gemm, then jch_row_resid_ss with k = 0.  gh = d2 / nlv.
    Deviation: `kwargs` are not taken (the reference hands them to a `kde` it never calls)."""
    if _kind(fm) not in ("Pca", "Kpca", "Plsr"):
        raise TypeError(f"occsd takes a Pca, Kpca or Plsr model, not a {_kind(fm)}")
    _check_cut(typc, cri, alpha)
    k = _nlv(fm, nlv, 1)
    T = fm.T[:, :k]
    dev = _is_torch(T)
    ctx = ctx or default_context((T.device.index or 0) if dev else 0)
    S = _cov_uncorrected(T, ctx)                                  # :134
    L = np.linalg.cholesky(S)                                     # :135  S = L L'
    Lc = np.linalg.solve(L, np.eye(k)).T                          # inv(L)': Sinv = inv(L)' inv(L) = Lc Lc'
    Lc = np.triu(Lc)
    Sinv = Lc @ Lc.T
    d2 = row_resid_ss(_affine(T, None, None, Lc, None, ctx), ctx=ctx)   # :136
    d = _sqrt(d2)                                                 # :137
    e_cdf = _sort(d)                                              # :140
    cutoff = _cutoff(e_cdf, typc, cri, alpha)                     # :138-139
    tab = dict(d=d, dstand=_div(d, cutoff), pval=_pval(e_cdf, d), gh=_div(d2, k))   # :141-143
    return Occsd(tab, fm, Sinv, e_cdf, cutoff, k, Lc)


def _predict_sd(obj: Occsd, X, ctx):
    """src/occsd.jl:153-164.  Pca / Plsr: one jch_transform with R[:, 1:nlv] Lc.  Kpca: kpca_transform, then the affine step."""
    fm, k = obj.fm, obj.nlv
    if _kind(fm) == "Kpca":
        U = _affine(kpca_transform(fm, X, nlv=k, ctx=ctx), None, None, obj.Lc, None, ctx)
    else:
        Rk = np.asfortranarray(_loadings(fm)[:, :k] @ obj.Lc, dtype=np.float64)
        X, U, ua, ctx, loc = _x_out(X, k, ctx)
        m, p = X.shape
        if Rk.shape[0] != p:
            raise ValueError(f"DimensionMismatch: X has {p} columns, the model has {Rk.shape[0]}")
        xm, xs = _model_vec(fm.xmeans), _model_vec(fm.xscales)
        xa, ldx = _addr_ld(X)
        ctx.check(_lib.load().jch_transform(ctx._h, loc, xa, m, p, ldx, _np(xm), _np(xs), Rk.ctypes.data, k, ua, max(m, 1)))
    d2 = row_resid_ss(U, ctx=ctx)
    d = _sqrt(d2)
    return dict(d=d, dstand=_div(d, obj.cutoff), pval=_pval(obj.e_cdf, d), gh=_div(d2, k))


# ---------------------------------------------------------------------------------- orthogonal distance
def _od2(fm, X, k, ctx):
    """sum(E .* E, dims = 2) of E = xresid(object, X; nlv = k) (src/occod.jl:48-49, src/xfit.jl:41-53) without E."""
    X = _colmajor_x(X)
    if fm.P.shape[0] != X.shape[1]:
        raise ValueError(f"DimensionMismatch: X has {X.shape[1]} columns, the model has {fm.P.shape[0]}")
    if k == 0:
        return row_resid_ss(X, fm.xmeans, ctx=ctx)
    Tq = transform(fm, X, nlv=k, ctx=ctx)
    return row_resid_ss(X, fm.xmeans, Tq, np.asarray(fm.xscales)[:, None] * np.asarray(fm.P)[:, :k], ctx=ctx)


def occod(fm, X, *, nlv: Optional[int] = None, typc: str = "mad", cri=3, alpha=.025, ctx: Optional[Context] = None) -> Occod:
    """`occod(object::Union{Pca, Plsr}, X; nlv, typc = "mad", cri = 3, alpha = .025)` — src/occod.jl:43-57.  T = transform(object, X; nlv), then
    jch_row_resid_ss with shift = xmeans, Z = T, B = diag(xscales) P[:, 1:nlv]: the residuals in the original scale (src/xfit.jl:48-51), two reads of
    X and no m x p matrix.  nlv = 0 gives the distances to the column means.  Deviation: `kwargs` are not taken."""
    if _kind(fm) not in ("Pca", "Plsr"):
        raise TypeError(f"occod takes a Pca or Plsr model, not a {_kind(fm)}")
    _check_cut(typc, cri, alpha)
    k = _nlv(fm, nlv, 0)
    d = _sqrt(_od2(fm, X, k, ctx))                                # :48-50
    e_cdf = _sort(d)                                              # :53
    cutoff = _cutoff(e_cdf, typc, cri, alpha)                     # :51-52
    return Occod(dict(d=d, dstand=_div(d, cutoff), pval=_pval(e_cdf, d)), fm, e_cdf, cutoff, k)


def _predict_od(obj: Occod, X, ctx):
    """src/occod.jl:65-75."""
    d = _sqrt(_od2(obj.fm, X, obj.nlv, ctx))
    return dict(d=d, dstand=_div(d, obj.cutoff), pval=_pval(obj.e_cdf, d))


# ---------------------------------------------------------------------------------- the compromise
def _hcat_sd_od(sd: dict, od: dict) -> dict:
    """src/occsdod.jl:44-50: the columns suffixed _sd / _od, then dstand = sqrt(dstand_sd * dstand_od)."""
    tab = {f"{name}_sd": col for name, col in sd.items()}
    tab.update({f"{name}_od": col for name, col in od.items()})
    tab["dstand"] = _sqrt(sd["dstand"] * od["dstand"])
    return tab


def occsdod(fm, X, *, nlv_sd: Optional[int] = None, nlv_od: Optional[int] = None, typc: str = "mad", cri=3, alpha=.025,
            ctx: Optional[Context] = None) -> Occsdod:
    """`occsdod(object::Union{Pca, Plsr}, X; nlv_sd, nlv_od, typc = "mad", cri = 3, alpha = .025)` — src/occsdod.jl:35-52.  Deviations: `kwargs`
    are not taken; `fm_sd.d` and `fm_od.d` keep their column names (the reference renames them in place)."""
    if _kind(fm) not in ("Pca", "Plsr"):
        raise TypeError(f"occsdod takes a Pca or Plsr model, not a {_kind(fm)}")
    fm_sd = occsd(fm, nlv=nlv_sd, typc=typc, cri=cri, alpha=alpha, ctx=ctx)
    fm_od = occod(fm, X, nlv=nlv_od, typc=typc, cri=cri, alpha=alpha, ctx=ctx)
    if fm_sd.d["d"].shape[0] != fm_od.d["d"].shape[0]:
        raise ValueError(f"DimensionMismatch: the model was fitted on {fm_sd.d['d'].shape[0]} rows, X has {fm_od.d['d'].shape[0]}")
    sd, od = fm_sd.d, fm_od.d
    if _is_torch(sd["d"]) != _is_torch(od["d"]):
        raise TypeError("the model's T and X must both be host arrays or both device tensors")
    return Occsdod(_hcat_sd_od(sd, od), fm_sd, fm_od)


def occ_predict(obj, X, *, ctx: Optional[Context] = None) -> OccPred:
    """`predict(object::Occsd, X)`, `predict(object::Occod, X)`, `predict(object::Occsdod, X)` (src/occsd.jl:153-164, src/occod.jl:65-75,
    src/occsdod.jl:60-74): the table of the new rows and pred = Int64.(dstand .> 1) as an m x 1 matrix.  An Occstah model: src/occstah.jl:55-73
    (stah.py)."""
    kind = _kind(obj)
    if kind == "Occstah":
        from .stah import _predict_stah
        return _predict_stah(obj, X, ctx)
    if kind in ("Occknndis", "Occlknndis"):
        from .knn import occknn_predict
        return occknn_predict(obj, X, ctx=ctx)
    if kind == "Occsd":
        tab = _predict_sd(obj, X, ctx)
    elif kind == "Occod":
        tab = _predict_od(obj, X, ctx)
    elif kind == "Occsdod":
        X = _colmajor_x(X)
        tab = _hcat_sd_od(_predict_sd(obj.fm_sd, X, ctx), _predict_od(obj.fm_od, X, ctx))
    else:
        raise TypeError(f"occ_predict takes an Occsd, Occod, Occsdod or Occstah model, not a {kind}")
    return OccPred(_pred(tab["dstand"]), tab)
