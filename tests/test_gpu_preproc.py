"""Spectra preprocessing on the GPU (snv, detrend, savgol, mavg, mavg_runmean, fdif over jch_rows_standardize / jch_rows_project_out /
jch_rows_fir) against the literal numpy restatements of src/preprocessing.jl in test_preproc_static.

Tolerances.  eps = 2^-52 (np.finfo(float64).eps) and gamma_k = k eps / (1 - k eps), the constant of the standard bound of a k-term
floating-point sum (Higham, Accuracy and Stability, §3.1: |fl(sum) - sum| <= gamma_{k-1} sum |terms|, products included gamma_k).  The
restatement and the GPU both carry such an error, in different summation orders, hence the factor 2 (4 for standardize, where it
enters through the mean and through the deviations):
  FIR (savgol, mavg)     |out - ref| <= 2 gamma_f sum_t |taps[t]| max_{window} |x|       element-wise, absolute in the inputs
  mavg_runmean           |out - ref| <= 2 gamma_p max_j |x_ij|                           (ref = the reference's running-sum recurrence)
  fdif                   bit-exact (one subtraction)
  project_out (detrend)  |out - ref| <= 2 gamma_p sum_k |V_jk| sum_l |A_kl| |x_il| + eps |ref|
  standardize (snv)      |out - ref| <= (4 gamma_p max_j |x_ij| / s_i + 8 eps) (1 + |out|)  (offset-dominated row, level 1e4, spread 1,
                         p = 500: about 1e-9; such rows are in every grid case)
Nothing here is tuned to what the kernels deliver; every case prints its largest error / bound ratio."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_preproc_static import (np_detrend, np_detrend_coef, np_fdif, np_mavg, np_mavg_runmean, np_savgk, np_savgol,  # noqa: E402
                                 np_snv, spectra)

EPS = float(np.finfo(np.float64).eps)
FIR_SAME, FIR_VALID = 0, 1
NS = [1, 63, 64, 65, 1000, 4097]
PS = [1, 2, 7, 500, 1050, 2500]
SAVGOL = [(3, 1, 1), (21, 3, 2), (9, 2, 0), (71, 3, 1)]     # f = 3; the usual one; f > p for p in {1, 2, 7}; beyond the ring kernel (f > 64)
MAVG = [11, 10]                                                # odd and even


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


@pytest.fixture(scope="module")
def J():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import jchemo_hip
    return jchemo_hip


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    yield c
    c.close()


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _dev(J, A):
    A = np.asarray(A, dtype=np.float64)
    D = J.colmajor_empty(A.shape[0], A.shape[1], "cuda:0")
    D.copy_(torch.from_numpy(A))
    return D


def _run(J, ctx, entry, X, ld, where, inplace, pout, mid):
    """One call of a C entry on X (n x p) stored with leading dimension ld, from the host or the device, in place or not; the rows
    beyond n of both buffers are NaN and must stay so; returns the n x pout result."""
    L = J.load()
    n, p = X.shape
    buf = np.full((ld, p), np.nan, order="F")
    buf[:n] = X
    if where == "host":
        dst = buf if inplace else np.full((ld, pout), np.nan, order="F")
        ctx.check(getattr(L, entry)(ctx._h, 0, buf.ctypes.data, n, p, ld, *mid, dst.ctypes.data, ld))
        res, src = dst, buf
    else:
        sd = torch.from_numpy(np.ascontiguousarray(buf.T)).cuda()          # (p, ld) row-major == ld x p column-major
        dd = sd if inplace else torch.full((pout, ld), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.check(getattr(L, entry)(ctx._h, 1, sd.data_ptr(), n, p, ld, *mid, dd.data_ptr(), ld))
        res, src = dd.cpu().numpy().T, sd.cpu().numpy().T
    assert np.isnan(res[n:]).all(), "rows beyond n were written"
    if not inplace:
        assert np.array_equal(src[:n], X), "the input of a copying call was modified"
    elif pout < p:
        assert np.array_equal(res[:n, pout:], X[:, pout:]), "in place, VALID: the columns from p - f + 1 on keep their input values"
    return np.array(res[:n, :pout])


def _all_routes(J, ctx, entry, X, pout, mid):
    """The eight routes (ld n and n + 3, host and device, copy and in place) must agree bit for bit; returns the common result."""
    n = X.shape[0]
    first = None
    for ld in (n, n + 3):
        for where in ("host", "device"):
            for inplace in (False, True):
                got = _run(J, ctx, entry, X, ld, where, inplace, pout, mid)
                if first is None:
                    first = got
                else:
                    assert np.array_equal(got, first, equal_nan=True), (entry, ld, where, inplace)
    return first


def _check(name, got, ref, bound):
    with np.errstate(all="ignore"):
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]), name
        err = np.abs(got - ref)[fin]
        b = np.broadcast_to(bound, ref.shape)[fin]
    with np.errstate(all="ignore"):
        ratio = float(np.max(np.where(err == 0, 0.0, err / b))) if err.size else 0.0
    print(f"  {name}: max |err| {float(err.max()) if err.size else 0.0:.3e}, max err / bound {ratio:.3f}")
    assert np.all(err <= b), f"{name}: err / bound {ratio:.3f}"


def _window_max(X, f, lo):
    p = X.shape[1]
    cols = np.arange(p)
    W = np.zeros_like(X)
    for t in range(f):
        np.maximum(W, np.abs(X[:, np.clip(cols + lo + t, 0, p - 1)]), out=W)
    return W


def _fir_bound(X, taps, lo, pout):
    return 2 * gamma(len(taps)) * np.abs(taps).sum() * _window_max(X, len(taps), lo)[:, :pout]


def _snv_bound(X, ref):
    with np.errstate(all="ignore"):
        s = X.std(axis=1)
        return (4 * gamma(X.shape[1]) * np.abs(X).max(axis=1) / s + 8 * EPS)[:, None] * (1 + np.abs(ref))


def _detrend_bound(X, ref, pol):
    vX, A = np_detrend_coef(X.shape[1], pol)
    return 2 * gamma(X.shape[1]) * (np.abs(X) @ np.abs(A).T) @ np.abs(vX).T + EPS * np.abs(ref)


def _savgol_taps(f, pol, d):
    kern = np_savgk((f - 1) // 2, pol, d)[2]
    return np.ascontiguousarray(kern[::-1]), -((f - 1) // 2)


# ---------------------------------------------------------------------------------- parity over the grid
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("n", NS)
def test_parity_with_the_restatements(n, p, J, ctx):
    X = spectra(n, p, 1000 * n + p)                  # rows at levels 0, 1, 100, 1e4 with unit spread: offset-dominated rows included
    print(f"n={n} p={p}")
    # snv
    for cent, scal in ((True, True), (True, False), (False, True)):
        got = _all_routes(J, ctx, "jch_rows_standardize", X, p, (int(cent), int(scal)))
        ref = np_snv(X, cent, scal)
        bound = _snv_bound(X, ref) if scal else (4 * gamma(p) * np.abs(X).max(axis=1) + 8 * EPS)[:, None] * (1 + np.abs(ref))
        _check(f"snv cent={cent} scal={scal}", got, ref, bound)
    # detrend
    for pol in (1, 2):
        vX, A = np_detrend_coef(p, pol)
        Af, Vf = np.asfortranarray(A), np.asfortranarray(vX)
        got = _all_routes(J, ctx, "jch_rows_project_out", X, p, (Af.ctypes.data, Vf.ctypes.data, pol + 1))
        ref = np_detrend(X, pol)
        _check(f"detrend pol={pol}", got, ref, _detrend_bound(X, ref, pol))
    # savgol
    for f, pol, d in SAVGOL:
        taps, lo = _savgol_taps(f, pol, d)
        got = _all_routes(J, ctx, "jch_rows_fir", X, p, (taps.ctypes.data, f, lo, FIR_SAME))
        _check(f"savgol f={f} pol={pol} d={d}", got, np_savgol(X, f, pol, d), _fir_bound(X, taps, lo, p))
    # mavg
    for f in MAVG:
        taps, lo = np.full(f, 1.0 / f), 1 - ((f + 1) >> 1)
        got = _all_routes(J, ctx, "jch_rows_fir", X, p, (taps.ctypes.data, f, lo, FIR_SAME))
        _check(f"mavg f={f}", got, np_mavg(X, f), _fir_bound(X, taps, lo, p))
    # mavg_runmean and fdif (VALID: f <= p)
    for f in (1, 2, 7, 70):
        if f <= p:
            taps = np.full(f, 1.0 / f)
            got = _all_routes(J, ctx, "jch_rows_fir", X, p - f + 1, (taps.ctypes.data, f, 0, FIR_VALID))
            _check(f"mavg_runmean f={f}", got, np_mavg_runmean(X, f), (2 * gamma(p) * np.abs(X).max(axis=1))[:, None])
    for f in (2, 5, 66):
        if f <= p:
            taps = np.zeros(f); taps[0], taps[-1] = -1.0, 1.0
            got = _all_routes(J, ctx, "jch_rows_fir", X, p - f + 1, (taps.ctypes.data, f, 0, FIR_VALID))
            assert np.array_equal(got, np_fdif(X, f)), f"fdif f={f} is not bit-exact"


def test_offset_dominated_rows_stay_within_the_snv_bound(J, ctx):
    """Level 1e4, spread 1, p = 500: the bound is about 1e-9 there, and sum x^2 - (sum x)^2 / p would miss it by orders of magnitude."""
    rng = np.random.default_rng(7)
    X = np.asfortranarray(1e4 + rng.standard_normal((300, 500)))
    got = _all_routes(J, ctx, "jch_rows_standardize", X, 500, (1, 1))
    ref = np_snv(X)
    bound = _snv_bound(X, ref)
    print(f"bound on a unit entry: {float(np.median(bound / (1 + np.abs(ref)))):.2e}")
    assert 2e-10 < float(np.median(bound / (1 + np.abs(ref)))) < 5e-9
    _check("snv level 1e4", got, ref, bound)
    xl = X.astype(np.longdouble)
    exact = ((xl - xl.mean(axis=1)[:, None]) / xl.std(axis=1)[:, None]).astype(np.float64)
    print(f"  against longdouble: GPU {np.abs(got - exact).max():.2e}, restatement {np.abs(ref - exact).max():.2e}")


# ---------------------------------------------------------------------------------- the Python interface
@pytest.mark.parametrize("where", ["host", "device"])
def test_python_functions_numpy_in_numpy_out_tensor_in_tensor_out(where, J):
    n, p = 130, 90
    X = spectra(n, p, 11)
    mk = (lambda a: np.array(a, order="F")) if where == "host" else (lambda a: _dev(J, a))
    kind = np.ndarray if where == "host" else torch.Tensor
    cases = [("snv", J.snv, J.snv_, {}, np_snv(X), _snv_bound(X, np_snv(X))),
             ("detrend", J.detrend, J.detrend_, dict(pol=2), np_detrend(X, 2), _detrend_bound(X, np_detrend(X, 2), 2)),
             ("savgol", J.savgol, J.savgol_, dict(f=11, pol=2, d=1), np_savgol(X, 11, 2, 1), _fir_bound(X, *_savgol_taps(11, 2, 1), p)),
             ("mavg", J.mavg, J.mavg_, dict(f=6), np_mavg(X, 6), _fir_bound(X, np.full(6, 1 / 6), -2, p))]
    for name, fun, fun_, kw, ref, bound in cases:
        Xi = mk(X)
        out = fun(Xi, **kw)
        assert isinstance(out, kind) and out.shape == (n, p) and np.array_equal(_host(Xi), X), name
        if where == "device":
            assert out.is_cuda and out.stride() == (1, n) and out.dtype == torch.float64
        _check(name, _host(out), ref, bound)
        same = fun_(Xi, **kw)
        assert same is Xi and np.array_equal(_host(Xi), _host(out)), f"{name}_ differs from {name}"
    Xi = mk(X)
    r = J.mavg_runmean(Xi, f=9)
    assert isinstance(r, kind) and r.shape == (n, p - 8)
    _check("mavg_runmean", _host(r), np_mavg_runmean(X, 9), (2 * gamma(p) * np.abs(X).max(axis=1))[:, None])
    for f in (2, 10):
        d = J.fdif(Xi, f=f) if f != 2 else J.fdif(Xi)
        assert isinstance(d, kind) and np.array_equal(_host(d), np_fdif(X, f))
    assert np.array_equal(_host(Xi), X)
    # layouts the entry points cannot read in place are converted first: row-major, float32, a vector (ensure_mat)
    Xc = np.ascontiguousarray(X) if where == "host" else torch.from_numpy(np.ascontiguousarray(X)).cuda()
    _check("snv of a row-major X", _host(J.snv(Xc)), np_snv(X), _snv_bound(X, np_snv(X)))
    assert np.array_equal(_host(J.fdif(Xc)), np_fdif(X))
    v = X[:, 0].copy() if where == "host" else torch.from_numpy(X[:, 0].copy()).cuda()
    assert J.snv(v, scal=False).shape == (n, 1) and float(np.abs(_host(J.snv(v, scal=False))).max()) == 0.0


# ---------------------------------------------------------------------------------- behaviour
def _battery(J, X):
    """Every function once (ring and wide-window FIR included) on a host or device X."""
    return dict(snv=J.snv(X), snv_nc=J.snv(X, cent=False), detrend=J.detrend(X, pol=2), savgol=J.savgol(X, f=5, pol=2, d=1),
                savgol71=J.savgol(X, f=71, pol=3, d=0), mavg=J.mavg(X, f=4), runmean=J.mavg_runmean(X, f=6), fdif=J.fdif(X, f=5))


@pytest.mark.parametrize("where", ["host", "device"])
def test_a_nan_or_inf_in_one_row_changes_that_row_only_and_runs_repeat_bit_for_bit(where, J):
    n, p, bad = 200, 96, 77
    X = spectra(n, p, 21)
    Xb = X.copy(order="F")
    Xb[bad, 40] = np.nan
    Xb[bad + 1, 41] = np.inf
    mk = (lambda a: a) if where == "host" else (lambda a: _dev(J, a))
    clean, again, dirty = _battery(J, mk(X)), _battery(J, mk(X)), _battery(J, mk(Xb))
    keep = np.ones(n, dtype=bool)
    keep[[bad, bad + 1]] = False
    for k in clean:
        a, b, c = _host(clean[k]), _host(again[k]), _host(dirty[k])
        assert np.array_equal(a, b), f"{k}: two runs differ"
        assert np.array_equal(a[keep], c[keep]), f"{k}: a NaN / Inf leaked into another row"
        assert np.isfinite(a).all() and not np.isfinite(c[bad]).all()
    # zero taps are skipped: fdif(f = 5) of the Inf row is Inf only where an END of the window meets it, never NaN from 0 * Inf
    got = _host(dirty["fdif"])[bad + 1]
    with np.errstate(all="ignore"):
        assert np.array_equal(got, np_fdif(Xb[bad + 1:bad + 2], 5)[0]) and not np.isnan(got).any()


def test_a_constant_row_is_nan_or_inf_in_that_row_only(J):
    X = spectra(70, 50, 31)
    X[13] = 2.5
    X[14] = 0.0
    for where in ("host", "device"):
        Xi = X if where == "host" else _dev(J, X)
        a, b = _host(J.snv(Xi)), _host(J.snv(Xi, cent=False))
        assert np.isnan(a[13]).all() and np.isnan(a[14]).all()                       # 0 / 0
        assert np.isposinf(b[13]).all() and np.isnan(b[14]).all()                    # 2.5 / 0 and 0 / 0
        rest = np.r_[0:13, 15:70]
        assert np.array_equal(a[rest], _host(J.snv(np.asfortranarray(X[rest]) if where == "host" else _dev(J, X[rest]))))
        assert np.isfinite(b[rest]).all()


def test_bad_arguments_of_the_entry_points(J, ctx):
    L = J.load()
    X = np.zeros((8, 6), order="F")
    out = np.zeros((8, 6), order="F")
    t = np.ones(3)
    xa, oa, ta = X.ctypes.data, out.ctypes.data, t.ctypes.data
    EINVAL = -1
    assert L.jch_rows_standardize(ctx._h, 0, xa, 8, 6, 7, 1, 1, oa, 8) == EINVAL                  # ldx < n
    assert L.jch_rows_standardize(ctx._h, 0, xa, 4, 6, 8, 1, 1, xa, 4) == EINVAL                  # in place with another ld
    assert L.jch_rows_standardize(ctx._h, 2, xa, 8, 6, 8, 1, 1, oa, 8) == EINVAL                  # loc
    assert L.jch_rows_project_out(ctx._h, 0, xa, 8, 6, 8, xa, xa, 9, oa, 8) == EINVAL             # k > 8
    assert L.jch_rows_project_out(ctx._h, 0, xa, 8, 6, 8, None, xa, 2, oa, 8) == EINVAL
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 3, 1, FIR_SAME, oa, 8) == EINVAL            # lo > 0
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 3, -3, FIR_SAME, oa, 8) == EINVAL           # lo < -(f - 1)
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 3, -1, FIR_VALID, oa, 8) == EINVAL          # VALID needs lo == 0
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 2, 8, ta, 3, 0, FIR_VALID, oa, 8) == EINVAL           # VALID needs f <= p
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 0, 0, FIR_SAME, oa, 8) == EINVAL
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 3, -1, 2, oa, 8) == EINVAL                  # mode
    assert b"lo" in L.jch_last_error(ctx._h) or b"mode" in L.jch_last_error(ctx._h)
    ctx.check(L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 3, -1, FIR_SAME, oa, 8))                 # the ctx works as usual afterwards


# ---------------------------------------------------------------------------------- pipeline and workspace
def _cmp_fit(O, ref, fm, tol):
    s = O.sign_align(ref.W, _host(fm.W))
    for f in ("T", "P", "R", "W", "C"):
        e = O.rel_fro(getattr(ref, f), _host(getattr(fm, f)) * s)
        assert e < tol, (f, e)


@pytest.mark.parametrize("where", ["device", "host"])
def test_pipeline_snv_savgol_plskern(where, J):
    """plskern(savgol(snv(X)), Y) with everything where X lives, against the oracle on the restatement's output, at the project's
    parity tolerance (1e-6, sign-aligned, as test_gpu_parity)."""
    from oracle import plsr_oracle as O
    n, p, q, nlv = 3000, 400, 2, 6
    X = spectra(n, p, 41)
    Z = np_savgol(np_snv(X), 11, 2, 1)
    rng = np.random.default_rng(42)
    Y = np.asfortranarray(Z @ rng.standard_normal((p, q)) + 0.01 * rng.standard_normal((n, q)))
    ref = O.plskern(Z, Y, nlv=nlv)
    if where == "host":
        fm = J.plskern(J.savgol(J.snv(X), f=11, pol=2, d=1), Y, nlv=nlv)
        assert isinstance(fm.T, np.ndarray)
        _cmp_fit(O, ref, fm, 1e-6)
        return
    Xd, Yd = _dev(J, X), _dev(J, Y)
    Zd = J.savgol(J.snv(Xd), f=11, pol=2, d=1)
    # the preprocessed matrix is a column-major float64 tensor on X's device: the fit reads it where it is (plsr._addr_ld), no host copy
    assert Zd.is_cuda and Zd.device == Xd.device and Zd.dtype == torch.float64 and Zd.stride() == (1, n)
    from jchemo_hip.plsr import _addr_ld
    assert _addr_ld(Zd) == (Zd.data_ptr(), n)
    fm = J.plskern(Zd, Yd, nlv=nlv)
    assert fm.T.is_cuda
    _cmp_fit(O, ref, fm, 1e-6)
    ptr = Zd.data_ptr()
    fm2 = J.plskern_(Zd, Yd, nlv=nlv)                # in place: the fit centres the very storage the preprocessing returned
    assert Zd.data_ptr() == ptr and float(Zd.mean(dim=0).abs().max()) < 1e-12 * float(np.abs(Z).max()) + 1e-13
    _cmp_fit(O, ref, fm2, 1e-6)


@pytest.mark.parametrize("same_x", [True, False])
def test_a_preprocessing_call_ends_the_validity_of_the_previous_fits_copy(same_x, J):
    """A host fit, then a preprocessing call on the same ctx — in place on the fit's own X (same pointer, new contents), or on other
    rows —, then a fit with reuse_x=True: it must equal a fresh fit (the working copy of the first fit is not to be trusted)."""
    from oracle import plsr_oracle as O
    n, p, q, nlv = 5000, 300, 2, 5
    X = spectra(n, p, 51, levels=(0.0, 1.0))
    rng = np.random.default_rng(52)
    Y = np.asfortranarray(X @ rng.standard_normal((p, q)) + 0.1 * rng.standard_normal((n, q)))
    ctx = J.Context(0)
    J.plskern(X, Y, nlv=nlv, ctx=ctx)
    J.plskern(X, Y, nlv=nlv, ctx=ctx, reuse_x=True)
    assert ctx.counter(4) == 1                                     # JCH_COUNTER_XCOPY_REUSED: the copy is in use on this shape
    if same_x:
        J.snv_(X, ctx=ctx)
    else:
        J.savgol(spectra(700, p, 53), f=71, pol=2, d=0, ctx=ctx)
    a = J.plskern(X, Y, nlv=nlv, ctx=ctx, reuse_x=True)
    fresh = J.Context(0)
    b = J.plskern(X, Y, nlv=nlv, ctx=fresh)
    s = O.sign_align(b.W, a.W)
    for f in ("T", "P", "R", "W", "C"):
        assert O.rel_fro(getattr(b, f), getattr(a, f) * s) < 1e-10, f
    assert O.rel_fro(b.xmeans, a.xmeans) < 1e-13
    ctx.close(); fresh.close()


# ---------------------------------------------------------------------------------- the stated size
def test_full_size_in_place_without_a_second_copy(J):
    """n = 1e6, p = 500 (4 GB): snv_ then savgol_(21, 3, 2) in place on the device; a strided sample of 4 096 rows of each step against the
    restatement under the bounds above, and nothing n x p is allocated besides X (device memory before / after; the device route
    stages nothing but the taps)."""
    n, p = 1_000_000, 500
    ctx = J.default_context(0)
    X = J.colmajor_empty(n, p, "cuda:0")
    torch.cuda.synchronize()
    ctx.check(J.load().jch_fill_uniform(ctx._h, X.data_ptr(), n, p, n, 0, n, C.c_uint64(20260101)))
    X.add_((torch.arange(n, device="cuda", dtype=torch.float64) % 7).mul_(50.0).unsqueeze(1))      # per-row offset 0 ... 300, spread 0.29
    idx = torch.arange(0, n, n // 4096, device="cuda")[:4096]
    take = lambda: X.index_select(0, idx).cpu().numpy()           # noqa: E731
    S0 = take()
    W = _dev(J, S0[:64])                                          # (first-call allocations, the taps buffer among them, are not the point)
    J.savgol_(J.snv_(W), f=21, pol=3, d=2)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    J.snv_(X)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    S1 = take()
    free1b = torch.cuda.mem_get_info()[0]
    J.savgol_(X, f=21, pol=3, d=2)
    torch.cuda.synchronize()
    free2 = torch.cuda.mem_get_info()[0]
    S2 = take()
    print(f"device memory taken by snv_: {(free0 - free1) / 2**20:.1f} MiB, by savgol_: {(free1b - free2) / 2**20:.1f} MiB")
    assert free0 - free1 <= 64 << 20 and free1b - free2 <= 64 << 20           # X is 3 815 MiB
    ref1 = np_snv(S0)
    _check("snv_ at n = 1e6", S1, ref1, _snv_bound(S0, ref1))
    taps, lo = _savgol_taps(21, 3, 2)
    _check("savgol_ at n = 1e6", S2, np_savgol(S1, 21, 3, 2), _fir_bound(S1, taps, lo, p))
    del X
    torch.cuda.empty_cache()
