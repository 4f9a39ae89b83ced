"""Exact column medians / MADs and the Stahel-Donoho outlyingness — host-side mirror of the reference's `colmad` (src/utility.jl:162), `stah`
(src/stah.jl:37-58) and `occstah` / `predict(::Occstah, X)` (src/occstah.jl:28-73) over jch_col_median_mad and jch_stah (include/jchemo_hip.h;
DESIGN.md §18).

numpy in gives numpy out; a device torch tensor in gives a device `d` (and with it `e_cdf`, the table's columns and `pred`) out.  What is p- or
a-sized (`mu_scal`, `s_scal`, `mu`, `s`, `P`) is a host array either way.  X is never written: the reference's `cscale!` runs on a copy too.

Deviations from the reference: the directions P are drawn on the host as 0 / 1 from `numpy.random.default_rng(seed)` unless given — the reference
draws them with `sample(0:1, p * a)` from a stream it does not pin, so P is an argument here; `kwargs` are not taken (the reference
passes them to a `kde` it never calls); `mad` uses StatsBase 0.33 / 0.34's default `normalize = true`."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .occ import OccPred, _check_cut, _colmajor_x, _cutoff, _div, _pred, _pval, _sort
from .plsr import _addr_ld, _is_torch, _np

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


@dataclass
class Stah:
    """What the reference's `stah` returns (src/stah.jl:58): (d, P, mu_scal, s_scal, mu, s)."""
    d: object
    P: np.ndarray
    mu_scal: np.ndarray
    s_scal: np.ndarray
    mu: np.ndarray
    s: np.ndarray


@dataclass
class Occstah:
    """The reference's `Occstah` (src/occstah.jl:1-6): d (the table: d, dstand, pval), res_stah, e_cdf (the sorted training d, where X lives), cutoff."""
    d: dict
    res_stah: Stah
    e_cdf: object
    cutoff: float


def _ctx_for(X, ctx):
    return ctx or default_context((X.device.index or 0) if _is_torch(X) else 0)


def col_median_mad(X, *, mad: bool = True, ctx: Optional[Context] = None):
    """jch_col_median_mad: (med, mad) — or med alone with `mad=False` — of the columns of X (n x p, a host array or a column-major device tensor) as host
    p-vectors.  Exact order statistics: odd n the middle value, even n lo / 2 + hi / 2 of the two middle ones; mad = 1.4826022185056018 *
    median(|x - med|).  A column holding a NaN gives NaN for both."""
    X = _colmajor_x(X)
    n, p = X.shape
    if n < 1 or p < 1:
        raise ValueError(f"X is {n} x {p}: at least one row and one column are needed")
    ctx = _ctx_for(X, ctx)
    dev = _is_torch(X)
    if dev:
        torch.cuda.current_stream(X.device).synchronize()
    med = np.empty(p)
    md = np.empty(p) if mad else None
    xa, ldx = _addr_ld(X)
    ctx.check(_lib.load().jch_col_median_mad(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, xa, n, p, ldx, med.ctypes.data, _np(md), _lib.LOC_HOST))
    return (med, md) if mad else med


def colmad(X, *, ctx: Optional[Context] = None):
    """`colmad(X)` — src/utility.jl:162-170: the MAD of each column, a host p-vector."""
    return col_median_mad(X, ctx=ctx)[1]


def _check_a(a):
    if isinstance(a, bool) or int(a) != a or int(a) < 1:
        raise ValueError(f"a = {a} must be an integer >= 1")
    return int(a)


def _directions(p: int, a: int, P, seed):
    if P is None:
        return np.asfortranarray(np.random.default_rng(seed).integers(0, 2, size=(p, a)), dtype=np.float64)   # src/stah.jl:40, on numpy's stream
    P = np.asfortranarray(P, dtype=np.float64)
    if P.shape != (p, a):
        raise ValueError(f"DimensionMismatch: P is {' x '.join(map(str, P.shape))}, expected {p} x {a}")
    return P


def _jch_stah(X, mu_scal, s_scal, P, fit: bool, mu, s, ctx):
    """One jch_stah call; returns d where X lives (mu and s are written in place when fit)."""
    n, p = X.shape
    a = P.shape[1]
    dev = _is_torch(X)
    if dev:
        d = torch.empty(n, dtype=torch.float64, device=X.device)
        da = d.data_ptr()
        torch.cuda.current_stream(X.device).synchronize()
    else:
        d = np.empty(n)
        da = d.ctypes.data
    xa, ldx = _addr_ld(X)
    ctx.check(_lib.load().jch_stah(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, xa, n, p, ldx, _np(mu_scal), _np(s_scal), P.ctypes.data, a, max(p, 1),
                                   int(fit), mu.ctypes.data, s.ctypes.data, da))
    return d


def stah(X, a, *, scal: bool = True, P=None, seed=None, ctx: Optional[Context] = None) -> Stah:
    """`stah(X, a; scal = true)` — src/stah.jl:37-58.  mu_scal, s_scal = the column medians and MADs of X (jch_col_median_mad) when `scal`, zeros and
    ones otherwise (:41-47); then one jch_stah call: T = cscale(X, mu_scal, s_scal) * P in column panels (:48), mu and s = the medians and MADs of
    the columns of T (:49-50), d[i] = max_j |(t_ij - mu_j) / s_j| (:51-57).  P (p x a) is drawn as 0 / 1 from `default_rng(seed)` unless given."""
    a = _check_a(a)
    X = _colmajor_x(X)
    n, p = X.shape
    if n < 1 or p < 1:
        raise ValueError(f"X is {n} x {p}: at least one row and one column are needed")
    P = _directions(p, a, P, seed)
    ctx = _ctx_for(X, ctx)
    if scal:
        mu_scal, s_scal = col_median_mad(X, ctx=ctx)
    else:
        mu_scal, s_scal = np.zeros(p), np.ones(p)
    mu, s = np.empty(a), np.empty(a)
    d = _jch_stah(X, mu_scal if scal else None, s_scal if scal else None, P, True, mu, s, ctx)
    return Stah(d, P, mu_scal, s_scal, mu, s)


def occstah(X, *, a=2000, typc: str = "mad", cri=3, alpha=.025, scal: bool = True, P=None, seed=None, ctx: Optional[Context] = None) -> Occstah:
    """`occstah(X; a = 2000, typc = "mad", cri = 3, alpha = .025, scal = true)` — src/occstah.jl:28-47: d = stah(X, a; scal).d, the cutoff, the ECDF
    and `pval` as for `occsd`.  Deviations: `kwargs` are not taken; P / seed as in `stah`."""
    _check_cut(typc, cri, alpha)
    res = stah(X, a, scal=scal, P=P, seed=seed, ctx=ctx)                   # :30
    d = res.d                                                              # :31
    e_cdf = _sort(d)                                                       # :43
    cutoff = _cutoff(e_cdf, typc, cri, alpha)                              # :41-42
    return Occstah(dict(d=d, dstand=_div(d, cutoff), pval=_pval(e_cdf, d)), res, e_cdf, cutoff)   # :44-46


def _predict_stah(obj: Occstah, X, ctx) -> OccPred:
    """`predict(object::Occstah, X)` — src/occstah.jl:55-73: one jch_stah call with fit = 0."""
    res = obj.res_stah
    X = _colmajor_x(X)
    p = res.P.shape[0]
    if X.shape[1] != p:
        raise ValueError(f"DimensionMismatch: X has {X.shape[1]} columns, the model has {p}")
    ctx = _ctx_for(X, ctx)
    d = _jch_stah(X, np.ascontiguousarray(res.mu_scal, dtype=np.float64), np.ascontiguousarray(res.s_scal, dtype=np.float64),
                  np.asfortranarray(res.P, dtype=np.float64), False, np.ascontiguousarray(res.mu, dtype=np.float64),
                  np.ascontiguousarray(res.s, dtype=np.float64), ctx)
    tab = dict(d=d, dstand=_div(d, obj.cutoff), pval=_pval(obj.e_cdf, d))
    return OccPred(_pred(tab["dstand"]), tab)
