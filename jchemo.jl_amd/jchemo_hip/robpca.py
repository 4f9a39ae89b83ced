"""Spatial median and spherical PCA — host-side mirror of the reference's src/colmedspa.jl and src/pcasph.jl over jch_weiszfeld_step,
jch_spatial_median and jch_pcasph_fit (include/jchemo_hip.h).

numpy in gives numpy out; a column-major device torch tensor in leaves what is n-sized (`T`, `weights`, the distances) on the device.  The p- and
nlv-sized results are host arrays either way, and the two kinds of input give identical bits.

Deviations from the reference: `colmedspa` takes `maxit` (the reference loops for ever on data that never converge) and warns
when it is reached; `pcasph` takes the leading eigenvectors of the Gram of the projected rows instead of a full SVD of the transposed copy; a row
AT the centre (norm 0) gets weight 0 instead of turning the SVD's input into NaN, and is warned about once per fit; `pcasph_` does not leave the
centred X behind."""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Optional

import numpy as np

from . import _lib
from ._lib import Context, default_context
from .pca import Pca, _colmajor, _weights_arg
from .plsr import _addr_ld, _is_torch, colmajor_empty

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

CENT = {"medspa": 0, "mean": 1}   # include/jchemo_hip.h JCH_CENT_*


def _x_in(X, ctx):
    X = _colmajor(X)
    dev = _is_torch(X)
    if dev and not X.is_cuda:
        raise TypeError("torch inputs must live on the GPU (host data: pass numpy arrays)")
    if X.ndim != 2 or X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError("X must be a matrix with at least one row and one column")
    if dev:
        if X.dtype != torch.float64:
            raise TypeError("X must be float64")
        torch.cuda.current_stream(X.device).synchronize()
    else:
        X = np.asfortranarray(X, dtype=np.float64)
    ctx = ctx or default_context((X.device.index or 0) if dev else 0)
    return X, dev, ctx


def weiszfeld_step(X, mu0, *, delta: float = 1e-6, guard: float = -1.0, ctx: Optional[Context] = None):
    """One step of `colmedspa` (src/colmedspa.jl:15-30) from the centre `mu0` through jch_weiszfeld_step: (mu, d, w0, h, nleft).  `guard < 0`: the
    distances first, then the pass with the exact clamp; `guard >= 0`: the rows with d <= guard go through the second stage (it must be >= delta *
    median(d), else the call fails)."""
    if not float(delta) > 0.0:
        raise ValueError(f"delta = {delta} must be > 0")
    mu0 = np.ascontiguousarray(np.asarray(mu0, dtype=np.float64).reshape(-1))
    if getattr(X, "ndim", 0) == 2 and mu0.shape[0] != X.shape[1]:
        raise ValueError(f"DimensionMismatch: mu0 has {mu0.shape[0]} entries, X has {X.shape[1]} columns")
    X, dev, ctx = _x_in(X, ctx)
    n, p = X.shape
    if mu0.shape[0] != p:
        raise ValueError(f"DimensionMismatch: mu0 has {mu0.shape[0]} entries, X has {p} columns")
    mu = np.empty(p)
    d = torch.empty(n, dtype=torch.float64, device=X.device) if dev else np.empty(n)
    w0, h, nl = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
    xa, ldx = _addr_ld(X)
    ctx.check(_lib.load().jch_weiszfeld_step(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, xa, n, p, ldx, mu0.ctypes.data, float(delta), float(guard),
                                             mu.ctypes.data, d.data_ptr() if dev else d.ctypes.data, C.byref(w0), C.byref(h), C.byref(nl)))
    return mu, d, w0.value, h.value, nl.value


def colmedspa(X, *, delta: float = 1e-6, maxit: int = 1000, ctx: Optional[Context] = None) -> np.ndarray:
    """`colmedspa(X; delta = 1e-6)` — src/colmedspa.jl:4-33 through jch_spatial_median: the spatial median of the rows of X as a host p-vector.  X is
    only read.  `maxit` bounds the steps; reaching it warns and returns the last centre."""
    if not float(delta) > 0.0:
        raise ValueError(f"delta = {delta} must be > 0")
    if isinstance(maxit, bool) or int(maxit) != maxit or int(maxit) < 1:
        raise ValueError(f"maxit = {maxit} must be an integer >= 1")
    X, dev, ctx = _x_in(X, ctx)
    n, p = X.shape
    mu = np.empty(p)
    nit, cvg, h = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
    xa, ldx = _addr_ld(X)
    ctx.check(_lib.load().jch_spatial_median(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, xa, n, p, ldx, float(delta), int(maxit), mu.ctypes.data, None,
                                             C.byref(nit), C.byref(h), C.byref(cvg)))
    if not cvg.value:
        warnings.warn(f"colmedspa: no convergence in {nit.value} steps (last step {h.value:.3g}, threshold {float(delta) * np.sqrt(p):.3g})", RuntimeWarning,
                      stacklevel=2)
    return mu


def pcasph(X, weights=None, *, nlv, typc: str = "medspa", delta: float = 1e-3, scal: bool = False, eig_tol: float = 1e-10, eig_maxit: int = 300,
           ctx: Optional[Context] = None) -> Pca:
    """`pcasph(X, weights; nlv, typc = "medspa", delta = .001, scal = false)` — src/pcasph.jl:54-92 through jch_pcasph_fit.  Returns the `Pca` of
    `pcasvd`: `transform`, `summary` and the `occ*` functions take it as they are.  eig = the eigenvalues of the Gram of the projected rows (not
    sv^2: sv holds the MADs of the projected scores), sstot its trace, colvar the weighted column variances of X, niter / conv / resid the eigen
    iteration's report."""
    if isinstance(nlv, bool) or int(nlv) != nlv or int(nlv) < 1:
        raise ValueError(f"nlv = {nlv} must be an integer >= 1")
    if typc not in CENT:
        raise ValueError(f"typc = {typc!r} must be 'medspa' or 'mean'")
    if not float(delta) > 0.0:
        raise ValueError(f"delta = {delta} must be > 0")
    if int(eig_maxit) < 1:
        raise ValueError(f"eig_maxit = {eig_maxit} must be >= 1")
    if not float(eig_tol) > 0.0:
        raise ValueError(f"eig_tol = {eig_tol} must be > 0")
    X, dev, ctx = _x_in(X, ctx)
    n, p = X.shape
    w_arr, w_addr = _weights_arg(weights, n, dev, X.device if dev else None)
    a = min(int(nlv), n, p)                                                  # src/pcasph.jl:63
    if dev:
        T = colmajor_empty(n, a, X.device)
        wn = torch.empty(n, dtype=torch.float64, device=X.device)
        ta, wa = T.data_ptr(), wn.data_ptr()
        torch.cuda.current_stream(X.device).synchronize()
    else:
        T = np.empty((n, a), order="F")
        wn = np.empty(n)
        ta, wa = T.ctypes.data, wn.ctypes.data
    P = np.empty((p, a), order="F")
    sv, eig, res = np.empty(a), np.empty(a), np.empty(a)
    xm, xs, cvar = np.empty(p), np.empty(p), np.empty(p)
    sst = C.c_double(0.0)
    nitm, cvgm, nit, cvg, got = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
    nz = C.c_int64(0)
    xa, ldx = _addr_ld(X)
    ctx.check(_lib.load().jch_pcasph_fit(ctx._h, _lib.LOC_DEVICE if dev else _lib.LOC_HOST, xa, n, p, ldx, w_addr, int(nlv), CENT[typc], float(delta), 1000,
                                         int(bool(scal)), float(eig_tol), int(eig_maxit), ta, P.ctypes.data, sv.ctypes.data, eig.ctypes.data, xm.ctypes.data,
                                         xs.ctypes.data, wa, C.byref(sst), cvar.ctypes.data, C.byref(nitm), C.byref(cvgm), C.byref(nit), res.ctypes.data,
                                         C.byref(cvg), C.byref(got), C.byref(nz)))
    if not cvgm.value:
        warnings.warn(f"pcasph: the spatial median did not converge in {nitm.value} steps", RuntimeWarning, stacklevel=2)
    if nz.value:
        warnings.warn(f"pcasph: {nz.value} row(s) lie at the centre (norm 0): they carry no direction and got weight 0", RuntimeWarning, stacklevel=2)
    conv = bool(cvg.value)
    if not conv:
        warnings.warn(f"pcasph: the subspace iteration did not converge in {nit.value} iterations (max residual {float(res.max()):.3g}, "
                      f"tolerance {float(eig_tol) * float(np.abs(eig).max()):.3g})", RuntimeWarning, stacklevel=2)
    return Pca(T, P, sv, xm, xs, wn, int(nit.value), conv, eig, float(sst.value), cvar, res, conv)


pcasph_ = pcasph   # `pcasph!` (src/pcasph.jl:60) centres X in place; the fit here never writes X
