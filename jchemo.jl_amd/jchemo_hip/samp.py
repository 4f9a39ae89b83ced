"""Sampling of the calibration set — host-side mirror of the reference's src/sampling.jl: `sampks` (Kennard-Stone, :40-60) and `sampdp` (Duplex,
:118-148) over jch_farthest_pair and jch_maxmin_select (include/jchemo_hip.h), `sampsys` (:168-182) and `sampcla` (:218-243) on the host.

The reference builds the n x n matrix D = euclsq(X, X) and re-slices it at every step; here nothing n x n exists: the starting pair is a maximum over
the tiles of the Gram, every later row costs one streaming read of X.  X is a host array or a column-major device tensor and is only read.  All indices
are 0-based (as in `covsel`); `train` is in selection order, `test` / `remain` ascending.

Deviations from the reference: `metric = "mahal"` runs the Euclidean path on Z = X * Uinv, Uinv the inverse of the upper Cholesky
factor of the uncorrected covariance S (the reference's own `mahsqchol`) where `mahsq` evaluates (x_i - x_j)' inv(S) (x_i - x_j): equal in exact
arithmetic.  `sampdp` takes its second pair as the farthest pair among the rows outside the first (sampling.jl:133 compares the unmasked D with the masked
maximum; the two readings differ only when a pair touching the first one ties the masked maximum exactly).  A row holding a NaN is never selected.  The
random branch of `sampcla` draws from `numpy.random.default_rng(seed)`: the reference's stream is not pinned."""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .occ import _colmajor_x
from .plsr import _addr_ld, _affine, _is_torch, _np

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


@dataclass
class Samp:
    """What `sampks` and `sampsys` return (src/sampling.jl:59, :181): (train, test)."""
    train: np.ndarray
    test: np.ndarray


@dataclass
class Sampdp:
    """What `sampdp` returns (src/sampling.jl:147): (train, test, remain)."""
    train: np.ndarray
    test: np.ndarray
    remain: np.ndarray


@dataclass
class Sampcla:
    """What `sampcla` returns (src/sampling.jl:242): (train, test, lev, ni, k)."""
    train: np.ndarray
    test: np.ndarray
    lev: np.ndarray
    ni: np.ndarray
    k: np.ndarray


def _ctx_for(X, ctx):
    return ctx or default_context((X.device.index or 0) if _is_torch(X) else 0)


def _loc_sync(X):
    if _is_torch(X):
        torch.cuda.current_stream(X.device).synchronize()
        return _lib.LOC_DEVICE
    return _lib.LOC_HOST


def farthest_pair(X, skip=None, *, ctx: Optional[Context] = None):
    """jch_farthest_pair: (row, col, d2), row > col — the two rows of X (n x p) with the largest squared Euclidean distance among the rows not in `skip`;
    ties go to the smallest col, then the smallest row (the first maximum of a column-major scan of the distance matrix).  d2 is the pair's squared
    distance in direct form."""
    X = _colmajor_x(X)
    n, p = X.shape
    sk = np.ascontiguousarray([] if skip is None else skip, dtype=np.int64).reshape(-1)
    if n < 2 or p < 1:
        raise ValueError(f"X is {n} x {p}: at least two rows and one column are needed")
    ctx = _ctx_for(X, ctx)
    pair, d2 = np.empty(2, dtype=np.int64), np.empty(1)
    xa, ldx = _addr_ld(X)
    ctx.check(_lib.load().jch_farthest_pair(ctx._h, _loc_sync(X), xa, n, p, ldx, sk.ctypes.data if sk.size else None, sk.size, pair.ctypes.data, d2.ctypes.data))
    return int(pair[0]), int(pair[1]), float(d2[0])


def maxmin_select(X, init, k, *, nsets: int = 1, dsel: bool = False, ctx: Optional[Context] = None):
    """jch_maxmin_select: sel (k x nsets, selection order down the columns) — and with `dsel=True` the min-distances at which the rows were taken — from
    the starting pair(s) `init` (2 nsets indices).  nsets = 1: Kennard-Stone; nsets = 2: Duplex."""
    X = _colmajor_x(X)
    n, p = X.shape
    init = np.ascontiguousarray(init, dtype=np.int64).reshape(-1)
    if nsets not in (1, 2) or init.size != 2 * nsets:
        raise ValueError(f"nsets = {nsets} must be 1 or 2 and init must hold 2 nsets indices (got {init.size})")
    k = int(k)
    ctx = _ctx_for(X, ctx)
    sel = np.empty((k if k > 0 else 0, nsets), dtype=np.int64, order="F")
    ds = np.empty(sel.shape, order="F") if dsel else None
    xa, ldx = _addr_ld(X)
    ctx.check(_lib.load().jch_maxmin_select(ctx._h, _loc_sync(X), xa, n, p, ldx, nsets, init.ctypes.data, k, sel.ctypes.data, _np(ds)))
    return (sel, ds) if dsel else sel


def _check_metric(metric):
    if metric not in ("eucl", "mahal"):
        raise ValueError(f'metric = {metric!r} must be "eucl" or "mahal"')


def _check_x_k(X, k, per_row, who):
    k = int(round(k))                                                       # sampling.jl:41, :119 (Julia's `round`: half to even, as Python's)
    X = _colmajor_x(X)
    n, p = X.shape
    if p < 1 or k < 2 or per_row * k > n:
        raise ValueError(f"{who}: k = {k} must be >= 2 and <= n{'' if per_row == 1 else ' / 2'} (X is {n} x {p})")
    return X, k


def _mahal_space(X, ctx):
    """Z = X * Uinv where X lives, S = U'U the uncorrected covariance of X (jch_weighted_cov), Uinv computed on the host; p = 1: 1 / sqrt(S)."""
    n, p = X.shape
    S = np.empty((p, p), order="F")
    xa, ldx = _addr_ld(X)
    ctx.check(_lib.load().jch_weighted_cov(ctx._h, _loc_sync(X), xa, n, p, ldx, None, S.ctypes.data, None))
    S = (S + S.T) / 2
    if not np.all(np.isfinite(S)):
        raise ValueError("metric = \"mahal\": the covariance of X is not finite")
    if p == 1:
        if not S[0, 0] > 0:
            raise ValueError("metric = \"mahal\": the covariance of X is not positive definite")
        Uinv = np.array([[1.0 / np.sqrt(S[0, 0])]])
    else:
        try:
            L = np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            raise ValueError("metric = \"mahal\": the covariance of X is not positive definite") from None
        Uinv = np.linalg.inv(L.T)
    return _affine(X, None, None, np.asfortranarray(Uinv), None, ctx)


def _rest(n, *taken):
    keep = np.ones(n, dtype=bool)
    for t in taken:
        keep[t] = False
    return np.flatnonzero(keep)


def sampks(X, k, metric: str = "eucl", ctx: Optional[Context] = None) -> Samp:
    """`sampks(X; k, metric = "eucl")` — src/sampling.jl:40-60, Kennard-Stone: the start is the farthest pair [row, col] (:49-50, jch_farthest_pair),
    every further row maximises its smallest distance to the rows already taken (:53-58, jch_maxmin_select).  train: the k rows in selection order;
    test: the others, ascending."""
    _check_metric(metric)
    X, k = _check_x_k(X, k, 1, "sampks")
    ctx = _ctx_for(X, ctx)
    Z = X if metric == "eucl" else _mahal_space(X, ctx)
    row, col, _ = farthest_pair(Z, ctx=ctx)
    s = maxmin_select(Z, [row, col], k, nsets=1, ctx=ctx)[:, 0].copy()
    return Samp(s, _rest(X.shape[0], s))


def sampdp(X, k, metric: str = "eucl", ctx: Optional[Context] = None) -> Sampdp:
    """`sampdp(X; k, metric = "eucl")` — src/sampling.jl:118-148, Duplex: two sets of k rows each.  The first pair is the farthest pair (:128-129), the
    second the farthest pair among the other rows (:130-134, the masked reading), then both sets grow by max-min steps, the first set choosing first
    (:137-146), in one read of X per pair of rows.  remain: the rows in neither set, ascending."""
    _check_metric(metric)
    X, k = _check_x_k(X, k, 2, "sampdp")
    if X.shape[0] < 4:
        raise ValueError(f"sampdp: X has {X.shape[0]} rows, two pairs need 4")
    ctx = _ctx_for(X, ctx)
    Z = X if metric == "eucl" else _mahal_space(X, ctx)
    r1, c1, _ = farthest_pair(Z, ctx=ctx)
    r2, c2, _ = farthest_pair(Z, skip=[r1, c1], ctx=ctx)
    sel = maxmin_select(Z, [r1, c1, r2, c2], k, nsets=2, ctx=ctx)
    s1, s2 = sel[:, 0].copy(), sel[:, 1].copy()
    return Sampdp(s1, s2, _rest(X.shape[0], s1, s2))


def _grid(n: int, k: int):
    """`unique(Int64.(round.(collect(1:alpha:n))))`, alpha = (n - 1) / (k - 1) — sampling.jl:172-176, 1-based.  Julia lifts the step of a floating-point
    range to the rational it came from, so the grid points are 1 + i (n - 1) / (k - 1) exactly; `round` is half to even."""
    if k == 1:                                   # alpha = Inf: the range holds its start only
        return [1]
    z, seen = [], set()
    for i in range(k):
        v = int(round(Fraction(k - 1 + i * (n - 1), k - 1)))
        if v not in seen:
            seen.add(v)
            z.append(v)
    return z


def sampsys(y, k) -> Samp:
    """`sampsys(y; k)` — src/sampling.jl:168-182: a regular grid of k ranks over the sorted y; the minimum and the maximum are always taken.  train in
    the order of y's values, test ascending.  Host only."""
    k = int(round(k))
    y = np.asarray(y.cpu() if _is_torch(y) else y).reshape(-1)
    n = y.shape[0]
    if k < 2 or n < 1:
        raise ValueError(f"sampsys: k = {k} must be >= 2 and y must not be empty")
    z = np.asarray(_grid(n, k), dtype=np.int64) - 1
    idx = np.argsort(y, kind="stable")           # sortperm: stable, NaN last
    s = idx[z]
    return Samp(s, _rest(n, s))


def sampcla(x, y=None, k=None, seed=None) -> Sampcla:
    """`sampcla(x, y = nothing; k)` — src/sampling.jl:218-243: k rows (one number, or one per class in the order of the sorted class labels) from every
    class of x, clipped to the class size; random without replacement when y is None (from `default_rng(seed)`), else `sampsys` over the class's y.  A
    class from which a single row is asked gives its smallest y (the range `1:Inf:n` holds 1 only).  Host only."""
    if k is None:
        raise ValueError("sampcla needs k")
    x = np.asarray(x).reshape(-1)
    n = x.shape[0]
    lev, ni = np.unique(x, return_counts=True)   # tab(x): sorted labels and their counts
    nlev = lev.shape[0]
    kk = np.asarray(k).reshape(-1)
    if kk.shape[0] not in (1, nlev):
        raise ValueError(f"k has {kk.shape[0]} entries: one, or one per class ({nlev})")
    kk = np.array([int(round(float(v))) for v in (np.repeat(kk, nlev) if kk.shape[0] == 1 else kk)], dtype=np.int64)
    if np.any(kk < 1):
        raise ValueError("k must be >= 1 in every class")
    if y is not None:
        y = np.asarray(y.cpu() if _is_torch(y) else y).reshape(-1)
        if y.shape[0] != n:
            raise ValueError(f"DimensionMismatch: x has {n} entries, y has {y.shape[0]}")
    rng = np.random.default_rng(seed)
    kk = np.minimum(kk, ni)                      # :229
    s = []
    for i in range(nlev):
        zs = np.flatnonzero(x == lev[i])
        if y is None:
            s.append(rng.choice(zs, size=int(kk[i]), replace=False))
        else:
            u = np.argsort(y[zs], kind="stable")[np.asarray(_grid(zs.shape[0], int(kk[i])), dtype=np.int64) - 1]
            s.append(zs[u])
    s = np.concatenate(s).astype(np.int64)
    return Sampcla(s, _rest(n, s), lev, ni, kk)
