"""Static checks of the spectra-preprocessing surface (snv, detrend, savgol, savgk, mavg, mavg_runmean, fdif): the literal numpy
restatements of src/preprocessing.jl the GPU tests compare against, their self-checks against independent code (scipy), header,
Python package and Julia wrapper.  No GPU needed."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_julia_wrapper import JL, header_protos  # noqa: E402
from test_kplsr_static import _jl_function_kwargs  # noqa: E402

NEW_ENTRIES = {"jch_rows_standardize": 10, "jch_rows_project_out": 11, "jch_rows_fir": 12}
PY_NAMES = ("snv", "snv_", "detrend", "detrend_", "savgol", "savgol_", "savgk", "mavg", "mavg_", "mavg_runmean", "fdif")


# ---------------------------------------------------------------------------------- numpy restatements of src/preprocessing.jl
def np_snv(X, cent=True, scal=True):
    """snv! (:473-481): mu = rowmean or zeros, s = rowstd (uncorrected, src/utility.jl) or ones, X[:, j] = (X[:, j] - mu) / s."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    mu = X.mean(axis=1) if cent else np.zeros(n)
    with np.errstate(all="ignore"):
        s = X.std(axis=1, ddof=0) if scal else np.ones(n)
        return (X - mu[:, None]) / s[:, None]


def np_detrend_coef(p, pol):
    """(:34-41) vX[:, j + 1] = (1:p)^j, A = pinv(vX'vX, rtol = sqrt(eps)) vX'."""
    z = np.arange(1, p + 1, dtype=np.float64)
    vX = np.stack([z ** j for j in range(pol + 1)], axis=1)
    A = np.linalg.pinv(vX.T @ vX, rcond=math.sqrt(np.finfo(np.float64).eps)) @ vX.T
    return vX, A


def np_detrend(X, pol=1):
    """detrend! (:32-47): X[i, :] = y - vX * A * y per row."""
    X = np.asarray(X, dtype=np.float64)
    vX, A = np_detrend_coef(X.shape[1], pol)
    out = np.empty_like(X)
    for i in range(X.shape[0]):
        y = X[i]
        out[i] = y - vX @ (A @ y)
    return out


def np_fdif(X, f=2):
    """fdif! (:87-93): M[:, j] = X[:, j + f - 1] - X[:, j]."""
    X = np.asarray(X, dtype=np.float64)
    zp = X.shape[1] - f + 1
    return X[:, f - 1:f - 1 + zp] - X[:, :zp]


def np_corr_replicate(X, taps, lo):
    """imfilter of every row with a kernel whose axes start at `lo`: a correlation with replicate padding,
    out[j] = sum_t taps[t] x[clamp(j + lo + t)]."""
    X = np.asarray(X, dtype=np.float64)
    p = X.shape[1]
    cols = np.arange(p)
    out = np.zeros_like(X)
    with np.errstate(all="ignore"):
        for t, w in enumerate(taps):
            out += w * X[:, np.clip(cols + lo + t, 0, p - 1)]
    return out


def np_mavg(X, f):
    """mavg! (:247-260): imfilter with centered(ones(f) / f), whose axes are -((f + 1) >> 1) + 1 : f - ((f + 1) >> 1)."""
    return np_corr_replicate(X, np.ones(f) / f, 1 - ((f + 1) >> 1))


def np_mavg_runmean(X, f):
    """mavg_runmean! / runmean! (:307-335): the running-sum recurrence, literally."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    out = np.empty((n, p - f + 1))
    with np.errstate(all="ignore"):
        zsum = np.zeros(n)
        for i in range(f):
            zsum = zsum + X[:, i]
        out[:, 0] = zsum / f
        for i in range(f, p):
            zsum = zsum + (X[:, i] - X[:, i - f])
            out[:, i - f + 1] = zsum / f
    return out


def np_savgk(m, pol, d):
    """savgk (:362-375)."""
    assert m >= 1 and 1 <= pol <= 2 * m and 0 <= d <= pol
    u = np.arange(-m, m + 1, dtype=np.float64)
    S = np.stack([u ** j for j in range(pol + 1)], axis=1)
    G = S @ np.linalg.inv(S.T @ S)
    return S, G, math.factorial(d) * G[:, d]


def np_savgol(X, f, pol, d):
    """savgol! (:424-441): imfilter with reflect(centered(kern)), i.e. the convolution out[j] = sum_{u=-m}^{m} kern[u] x[j - u] with
    replicate padding."""
    assert f % 2 == 1 and f >= 3
    X = np.asarray(X, dtype=np.float64)
    m = (f - 1) // 2
    kern = np_savgk(m, pol, d)[2]
    p = X.shape[1]
    cols = np.arange(p)
    out = np.zeros_like(X)
    with np.errstate(all="ignore"):
        for u in range(-m, m + 1):
            out += kern[u + m] * X[:, np.clip(cols - u, 0, p - 1)]
    return out


def spectra(n, p, seed, levels=(0.0, 1.0, 100.0, 1e4)):
    """Rows with a per-row offset (offset-dominated rows included), a smooth band and unit noise."""
    rng = np.random.default_rng(seed)
    grid = np.linspace(0.0, 1.0, p)
    band = np.exp(-((grid[None, :] - rng.random((n, 1))) / 0.2) ** 2)
    lev = np.asarray(levels)[np.arange(n) % len(levels)]
    return np.asfortranarray(lev[:, None] + 3.0 * band + rng.standard_normal((n, p)))


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---------------------------------------------------------------------------------- the restatements against independent code
@pytest.mark.parametrize("f,pol,d", [(3, 1, 1), (5, 2, 0), (11, 2, 1), (21, 3, 2), (21, 3, 0), (51, 3, 2)])
def test_np_savgol_is_scipy_savgol_with_the_convolution_sign(f, pol, d):
    from scipy.signal import savgol_filter
    X = spectra(40, 300, 1, levels=(0.0, 1.0))
    ref = (-1) ** d * savgol_filter(X, f, pol, deriv=d, axis=1, mode="nearest")
    err = _rel(np_savgol(X, f, pol, d), ref)
    print(f"f={f} pol={pol} d={d}: rel. Frobenius {err:.2e}")
    assert err <= 1e-11


@pytest.mark.parametrize("f", [1, 3, 11, 25])
def test_np_mavg_odd_is_scipy_uniform_filter(f):
    from scipy.ndimage import uniform_filter1d
    X = spectra(30, 200, 2)
    assert _rel(np_mavg(X, f), uniform_filter1d(X, f, axis=1, mode="nearest")) <= 1e-13


def test_np_mavg_even_window_and_runmean_and_fdif():
    X = spectra(5, 40, 3)
    f = 4                                                            # axes -1:2
    j = 10
    assert np.allclose(np_mavg(X, f)[:, j], X[:, j - 1:j + 3].mean(axis=1), rtol=1e-14)
    assert np.allclose(np_mavg(X, f)[:, 0], (2 * X[:, 0] + X[:, 1] + X[:, 2]) / 4, rtol=1e-14)
    r = np_mavg_runmean(X, 7)
    assert r.shape == (5, 34) and np.allclose(r[:, 5], X[:, 5:12].mean(axis=1), rtol=1e-10, atol=1e-10)
    assert np.array_equal(np_fdif(X, 3), X[:, 2:] - X[:, :-2]) and np_fdif(X).shape == (5, 39)


def test_np_detrend_residuals_are_orthogonal_to_the_line():
    X = spectra(20, 300, 4, levels=(0.0, 1.0, 10.0))
    R = np_detrend(X, pol=1)
    vX, A = np_detrend_coef(300, 1)
    assert np.linalg.matrix_rank(vX.T @ vX, tol=math.sqrt(np.finfo(float).eps) * np.linalg.norm(vX.T @ vX, 2)) == 2
    scale = np.abs(X) @ np.abs(vX)
    assert np.max(np.abs(R @ vX) / scale) <= 1e-9


def test_np_snv_rows_have_mean_0_and_std_1():
    X = spectra(50, 500, 5)
    Z = np_snv(X)
    assert np.abs(Z.mean(axis=1)).max() <= 1e-9 and np.abs(Z.std(axis=1) - 1).max() <= 1e-9
    assert np.allclose(np_snv(X, cent=False), X / X.std(axis=1)[:, None], rtol=1e-15)
    assert np.allclose(np_snv(X, scal=False), X - X.mean(axis=1)[:, None], rtol=1e-15)


def test_host_coefficients_equal_the_restatements():
    from jchemo_hip import preproc as P
    for m, pol, d in [(1, 1, 1), (10, 3, 2), (25, 3, 2)]:
        got, ref = P.savgk(m, pol, d), np_savgk(m, pol, d)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b)
        assert got._fields == ("S", "G", "kern")
        taps, lo = P._savgol_taps(got.kern)
        assert lo == -m and np.array_equal(taps, ref[2][::-1])
    for f in (1, 2, 3, 10, 11):
        taps, lo = P._mavg_window(f)
        assert lo == 1 - ((f + 1) >> 1) and np.array_equal(taps, np.ones(f) / f)
    for p, pol in [(1, 1), (7, 2), (500, 1), (2000, 3)]:
        A, V = P._detrend_coef(p, pol)
        vX, Ar = np_detrend_coef(p, pol)
        assert np.array_equal(A, Ar) and np.array_equal(V, vX) and A.flags.f_contiguous and V.flags.f_contiguous


# ---------------------------------------------------------------------------------- interface
def test_header_declares_the_entries():
    protos = header_protos()
    for name, nargs in NEW_ENTRIES.items():
        assert name in protos, name
        assert protos[name][0] == "int32_t"
        assert len(protos[name][1]) == nargs, name
    h = open(os.path.join(ROOT, "include", "jchemo_hip.h")).read()
    assert re.search(r"#define\s+JCH_VERSION\s+108\b", h)
    assert re.search(r"#define\s+JCH_FIR_SAME\s+0\b", h) and re.search(r"#define\s+JCH_FIR_VALID\s+1\b", h)


def test_python_package_exports():
    import inspect
    import jchemo_hip as J
    for name in PY_NAMES:
        assert hasattr(J, name), name
    for s in NEW_ENTRIES:
        assert s in J.SYMBOLS
    kw = lambda fn: [k for k, v in inspect.signature(fn).parameters.items() if v.kind == v.KEYWORD_ONLY and k != "ctx"]  # noqa: E731
    dflt = lambda fn: {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not v.empty and k != "ctx"}  # noqa: E731
    assert kw(J.snv) == kw(J.snv_) == ["cent", "scal"] and dflt(J.snv) == dict(cent=True, scal=True)
    assert kw(J.detrend) == kw(J.detrend_) == ["pol"] and dflt(J.detrend) == dict(pol=1)
    assert kw(J.savgol) == kw(J.savgol_) == ["f", "pol", "d"] and dflt(J.savgol) == {}
    assert kw(J.mavg) == kw(J.mavg_) == kw(J.mavg_runmean) == ["f"]
    assert kw(J.fdif) == ["f"] and dflt(J.fdif) == dict(f=2)
    assert list(inspect.signature(J.savgk).parameters) == ["m", "pol", "d"]


def test_python_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    X = np.zeros((4, 6), order="F")
    for bad in (dict(f=4, pol=1, d=0), dict(f=1, pol=1, d=0), dict(f=5, pol=0, d=0), dict(f=5, pol=5, d=0), dict(f=5, pol=2, d=3),
                dict(f=5, pol=2, d=-1), dict(f=5.5, pol=2, d=0)):
        for fun in (J.savgol, J.savgol_):
            with pytest.raises(ValueError):
                fun(X, **bad)
    for bad in ((0, 1, 0), (2, 0, 0), (2, 5, 0), (2, 2, 3)):
        with pytest.raises(ValueError):
            J.savgk(*bad)
    for fun in (J.mavg, J.mavg_):
        with pytest.raises(ValueError):
            fun(X, f=0)
    for bad in (0, 7):
        with pytest.raises(ValueError):
            J.mavg_runmean(X, f=bad)
    for bad in (1, 7):
        with pytest.raises(ValueError):
            J.fdif(X, f=bad)
    for fun in (J.detrend, J.detrend_):
        for bad in (-1, 8):
            with pytest.raises(ValueError):
                fun(X, pol=bad)
    for fun in (J.snv_, J.detrend_):                                  # the `_` variants need the caller's column-major float64 storage
        with pytest.raises((ValueError, TypeError)):
            fun(np.zeros((4, 6), order="C"))
        with pytest.raises((ValueError, TypeError)):
            fun(np.zeros((4, 6), order="F", dtype=np.float32))


def test_preprocessing_without_a_gpu_raises_enodev():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import jchemo_hip as J
    from jchemo_hip._lib import JCH_ENODEV, JchError
    X = spectra(10, 30, 6)
    calls = [lambda: J.snv(X), lambda: J.snv_(X.copy(order="F")), lambda: J.detrend(X), lambda: J.detrend_(X.copy(order="F"), pol=2),
             lambda: J.savgol(X, f=5, pol=2, d=1), lambda: J.savgol_(X.copy(order="F"), f=5, pol=2, d=1), lambda: J.mavg(X, f=4),
             lambda: J.mavg_(X.copy(order="F"), f=5), lambda: J.mavg_runmean(X, f=5), lambda: J.fdif(X)]
    for call in calls:
        with pytest.raises(JchError) as e:
            call()
        assert e.value.code == JCH_ENODEV


def test_julia_module_exports_and_reference_keywords():
    src = open(JL).read()
    m = re.search(r"\nexport (.*?)\n\n", src, flags=re.S)
    names = {s.strip() for s in m.group(1).replace("\n", " ").split(",")}
    for name in ("snv", "snv!", "detrend", "detrend!", "savgol", "savgol!", "savgk", "mavg", "mavg!", "mavg_runmean", "fdif"):
        assert name in names, name
    want = {"snv": ["cent", "scal", "ctx"], "snv!": ["cent", "scal", "ctx"], "detrend": ["pol", "ctx"], "detrend!": ["pol", "ctx"],
            "savgol": ["f", "pol", "d", "ctx"], "savgol!": ["f", "pol", "d", "ctx"], "mavg": ["f", "ctx"], "mavg!": ["f", "ctx"],
            "mavg_runmean": ["f", "ctx"], "fdif": ["f", "ctx"]}
    for name, kws in want.items():
        found = _jl_function_kwargs(src, name)
        assert kws in found, f"{name}: {found}"
    assert re.search(r"function savgk\(m, pol, d\)", src)
    for entry in NEW_ENTRIES:
        assert re.search(r"ccall\(\(:" + entry + r", LIB\)", src), entry
    assert src.count("UNPINNED") >= 2                                 # the two unpinned readings, one place each
