"""Row-wise spectra preprocessing — host-side mirror of the reference's src/preprocessing.jl (snv, detrend, savgol, savgk, mavg,
mavg_runmean, fdif) over jch_rows_standardize / jch_rows_project_out / jch_rows_fir (include/jchemo_hip.h).

numpy in gives numpy out; a device torch tensor in gives a device tensor out (column-major, ready for plskern, kplsr, krr ...).  The
`_` variants work in place on the caller's column-major float64 storage (the reference's `!`) and return it; the plain variants
write a new matrix and leave X untouched.  `interpl` is not provided.

Two readings of ImageFiltering's semantics are not pinned against a run of the reference; each lives in exactly one
function here: `_savgol_taps` (the convolution sign) and `_mavg_window` (where an even window sits)."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .plsr import _addr_ld, _as_colmajor_copy, _as_colmajor_view, _is_torch, colmajor_empty, ensure_mat

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

FIR_SAME, FIR_VALID = 0, 1   # include/jchemo_hip.h JCH_FIR_*
_MAX_K = 8                   # jch_rows_project_out: 1 <= k <= 8


class Savgk(NamedTuple):
    """What the reference's `savgk` returns (src/preprocessing.jl:374)."""
    S: np.ndarray
    G: np.ndarray
    kern: np.ndarray


# ---------------------------------------------------------------------------------- host-side coefficients
def _as_int(v, name):
    if isinstance(v, bool) or int(v) != v:
        raise ValueError(f"{name} = {v} must be an integer")
    return int(v)


def savgk(m, pol, d) -> Savgk:
    """`savgk(m, pol, d)` — src/preprocessing.jl:362-375: S[:, j] = (-m:m)^j, G = S inv(S'S), kern = factorial(d) G[:, d + 1]."""
    m, pol, d = _as_int(m, "m"), _as_int(pol, "pol"), _as_int(d, "d")
    if m < 1:
        raise ValueError(f"savgk: the half-width m = {m} must be at least 1")
    if not (1 <= pol <= 2 * m):
        raise ValueError(f"savgk: pol = {pol} is outside 1 ... 2m = {2 * m}")
    if not (0 <= d <= pol):
        raise ValueError(f"savgk: d = {d} is outside 0 ... pol = {pol}")
    u = np.arange(-m, m + 1, dtype=np.float64)
    S = np.stack([u ** j for j in range(pol + 1)], axis=1)
    G = S @ np.linalg.inv(S.T @ S)
    return Savgk(S, G, math.factorial(d) * G[:, d])


def _savgol_taps(kern):
    """UNPINNED reading: `imfilter` is a correlation and the reference passes `reflect(centered(kern))`
    (src/preprocessing.jl:430-434), so the filter is a true convolution, out[j] = sum_{u=-m}^{m} kern[u] x[j - u]: as a correlation
    window that starts at j + lo, taps[t] = kern[m - t] and lo = -m.  (Dropping the reversal gives the correlation reading.)"""
    kern = np.asarray(kern, dtype=np.float64)
    return np.ascontiguousarray(kern[::-1]), -(len(kern) // 2)


def _mavg_window(f):
    """UNPINNED reading for even f: `centered(ones(f) / f)` (src/preprocessing.jl:250) has the axes
    -((f + 1) >> 1) + 1 : f - ((f + 1) >> 1), i.e. -m:m for odd f and -f/2 + 1 : f/2 for even f; `imfilter` correlates."""
    return np.full(f, 1.0 / f), 1 - ((f + 1) >> 1)


def _detrend_coef(p, pol):
    """vX[:, j] = (1:p)^j and A = pinv(vX'vX, rtol = sqrt(eps)) vX' exactly as src/preprocessing.jl:34-41 (the truncating pinv is part
    of the reference's result: for spectra-sized p the Gram of the monomials keeps rank 2)."""
    z = np.arange(1, p + 1, dtype=np.float64)
    vX = np.stack([z ** j for j in range(pol + 1)], axis=1)
    A = np.linalg.pinv(vX.T @ vX, rcond=math.sqrt(np.finfo(np.float64).eps)) @ vX.T
    return np.asfortranarray(A), np.asfortranarray(vX)


# ---------------------------------------------------------------------------------- plumbing
def _in_out(X, inplace, pout):
    """(X as the entry point reads it, the output matrix, ctx device index): in place the caller's storage is both; otherwise a
    column-major float64 X is read where it is and a new n x pout matrix is written next to it (anything else is converted first)."""
    if inplace:
        X = _as_colmajor_view(X)
        return X, X
    X = ensure_mat(X)
    if not _is_torch(X):
        X = np.asarray(X)
    try:
        _addr_ld(X)
    except (ValueError, TypeError):
        X = _as_colmajor_copy(X)
        if pout == X.shape[1]:
            return X, X
    n = X.shape[0]
    out = colmajor_empty(n, pout, X.device) if _is_torch(X) else np.empty((n, pout), dtype=np.float64, order="F")
    return X, out


def _call(entry, X, out, ctx, *mid):
    dev = _is_torch(X)
    if dev and not (X.is_cuda and out.is_cuda):
        raise TypeError("torch inputs must live on the GPU (host data: pass numpy arrays)")
    n, p = X.shape
    if n < 1 or p < 1:
        raise ValueError(f"X is {n} x {p}: needs at least one row and one column")
    ctx = ctx or default_context((X.device.index or 0) if dev else 0)
    xa, ldx = _addr_ld(X)
    oa, ldo = _addr_ld(out)
    if dev:
        torch.cuda.current_stream(X.device).synchronize()
    ctx.check(getattr(_lib.load(), entry)(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, xa, n, p, ldx, *mid, oa, ldo))
    return out


def _shape(X):
    X = ensure_mat(X)
    return X.shape


# ---------------------------------------------------------------------------------- snv
def _snv(X, cent, scal, ctx, inplace):
    X, out = _in_out(X, inplace, _shape(X)[1])
    return _call("jch_rows_standardize", X, out, ctx, int(bool(cent)), int(bool(scal)))


def snv(X, *, cent: bool = True, scal: bool = True, ctx: Optional[Context] = None):
    """`snv(X; cent = true, scal = true)` — src/preprocessing.jl:467-471: each row minus its mean, over its UNcorrected standard
    deviation (a constant row gives NaN / Inf in that row, as the reference)."""
    return _snv(X, cent, scal, ctx, False)


def snv_(X, *, cent: bool = True, scal: bool = True, ctx: Optional[Context] = None):
    """`snv!(X; cent, scal)` — src/preprocessing.jl:473-481, in place."""
    return _snv(X, cent, scal, ctx, True)


# ---------------------------------------------------------------------------------- detrend
def _detrend(X, pol, ctx, inplace):
    pol = _as_int(pol, "pol")
    if not (0 <= pol <= _MAX_K - 1):
        raise ValueError(f"detrend: pol = {pol} is outside 0 ... {_MAX_K - 1} (jch_rows_project_out takes k = pol + 1 <= {_MAX_K})")
    p = _shape(X)[1]
    X, out = _in_out(X, inplace, p)
    A, V = _detrend_coef(p, pol)
    return _call("jch_rows_project_out", X, out, ctx, A.ctypes.data, V.ctypes.data, pol + 1)


def detrend(X, *, pol: int = 1, ctx: Optional[Context] = None):
    """`detrend(X; pol = 1)` — src/preprocessing.jl:27-31: each row minus vX A row, with the reference's truncating pinv."""
    return _detrend(X, pol, ctx, False)


def detrend_(X, *, pol: int = 1, ctx: Optional[Context] = None):
    """`detrend!(X; pol = 1)` — src/preprocessing.jl:32-47, in place."""
    return _detrend(X, pol, ctx, True)


# ---------------------------------------------------------------------------------- FIR filters
def _fir(X, taps, lo, mode, ctx, inplace):
    n, p = _shape(X)
    f = len(taps)
    pout = p - f + 1 if mode == FIR_VALID else p
    X, out = _in_out(X, inplace, pout)
    taps = np.ascontiguousarray(taps, dtype=np.float64)
    return _call("jch_rows_fir", X, out, ctx, taps.ctypes.data, f, lo, mode)


def _savgol(X, f, pol, d, ctx, inplace):
    f = _as_int(f, "f")
    if not (f % 2 == 1 and f >= 3):
        raise ValueError("f must be odd and >= 3")
    taps, lo = _savgol_taps(savgk((f - 1) // 2, pol, d).kern)
    return _fir(X, taps, lo, FIR_SAME, ctx, inplace)


def savgol(X, *, f, pol, d, ctx: Optional[Context] = None):
    """`savgol(X; f, pol, d)` — src/preprocessing.jl:418-422: Savitzky-Golay filter of each row (f odd and >= 3, 1 <= pol <= f - 1,
    0 <= d <= pol), replicate padding, each point on the centre of the kernel."""
    return _savgol(X, f, pol, d, ctx, False)


def savgol_(X, *, f, pol, d, ctx: Optional[Context] = None):
    """`savgol!(X; f, pol, d)` — src/preprocessing.jl:424-441, in place."""
    return _savgol(X, f, pol, d, ctx, True)


def _mavg(X, f, ctx, inplace):
    f = _as_int(f, "f")
    if f < 1:
        raise ValueError("f must be >= 1")
    taps, lo = _mavg_window(f)
    return _fir(X, taps, lo, FIR_SAME, ctx, inplace)


def mavg(X, *, f, ctx: Optional[Context] = None):
    """`mavg(X; f)` — src/preprocessing.jl:241-245: moving average of each row with the centred kernel ones(f) / f, replicate padding."""
    return _mavg(X, f, ctx, False)


def mavg_(X, *, f, ctx: Optional[Context] = None):
    """`mavg!(X; f)` — src/preprocessing.jl:247-260, in place."""
    return _mavg(X, f, ctx, True)


def _valid_f(X, f, least):
    f = _as_int(f, "f")
    p = _shape(X)[1]
    if not (least <= f <= p):
        raise ValueError(f"f = {f} must agree with: {least} <= f <= p = {p}")
    return f


def mavg_runmean(X, *, f, ctx: Optional[Context] = None):
    """`mavg_runmean(X; f)` — src/preprocessing.jl:299-335: moving average without padding, (n, p) -> (n, p - f + 1), each point on
    the first unit of the kernel.  Every output is its own f-term sum (the reference's running sum carries its rounding along the row)."""
    f = _valid_f(X, f, 1)
    return _fir(X, np.full(f, 1.0 / f), 0, FIR_VALID, ctx, False)


def fdif(X, *, f: int = 2, ctx: Optional[Context] = None):
    """`fdif(X; f = 2)` — src/preprocessing.jl:79-93: M[:, j] = X[:, j + f - 1] - X[:, j], (n, p) -> (n, p - f + 1); one exact
    subtraction per element."""
    f = _valid_f(X, f, 2)
    taps = np.zeros(f)
    taps[0], taps[-1] = -1.0, 1.0
    return _fir(X, taps, 0, FIR_VALID, ctx, False)
