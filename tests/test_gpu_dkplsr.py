"""Direct kernel PLS on the GPU (dkplsr / krbf / kpol, include/jchemo_hip.h jch_kernel_gram, jch_dkplsr_*) against numpy
restatements of src/kernels.jl and the oracle's plskern / transform / predict on a numpy Gram matrix (src/dkplsr.jl)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "jchemo.jl_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import jchemo_hip as J  # noqa: E402
from jchemo_hip import _lib  # noqa: E402
from oracle import plsr_oracle as O  # noqa: E402

TOL = 1e-6   # the project's parity tolerance (sign-aligned relative Frobenius error)


@pytest.fixture(scope="module")
def ctx():
    return J.default_context(0)


# ---------------------------------------------------------------------------------- numpy restatements
def np_sqdist(Z, X):
    """sum_k (z_ik - x_jk)^2 from the differences (not the norm expansion), in row chunks."""
    out = np.empty((Z.shape[0], X.shape[0]))
    step = max(1, int(2e7 // max(1, X.shape[0] * X.shape[1])))
    for i in range(0, Z.shape[0], step):
        D = Z[i:i + step, None, :] - X[None, :, :]
        out[i:i + step] = np.einsum("ijk,ijk->ij", D, D)
    return out


def np_krbf(Z, X, gamma):
    return np.exp(-gamma * np_sqdist(Z, X))


def np_kpol(Z, X, degree, gamma, coef0):
    K = gamma * Z @ X.T + coef0
    zK = K.copy()
    for _ in range(degree - 1):
        K = K * zK
    return K


def spectra(seed, n, p, base=0.0):
    """Smooth spectra-like rows: a few Gaussian bands with random heights plus a little noise."""
    rng = np.random.default_rng(seed)
    grid = np.linspace(0, 1, p)
    c = np.array([0.2, 0.45, 0.7, 0.85])
    H = rng.random((n, c.size))
    X = H @ np.exp(-((grid[None, :] - c[:, None]) / 0.08) ** 2) + 0.01 * rng.standard_normal((n, p)) + base
    return np.asfortranarray(X), H


def raw_gram(ctx, loc, kind, Z, X, gamma=1.0, coef0=0.0, degree=1, ldpad=3, same=False):
    """jch_kernel_gram through the raw ABI with leading dimensions larger than the row counts."""
    m, p = Z.shape
    n = X.shape[0]
    if loc == _lib.LOC_HOST:
        Zb = np.zeros((m + ldpad, p), order="F"); Zb[:m] = Z
        Xb = Zb if same else np.zeros((n + ldpad, p), order="F")
        if not same:
            Xb[:n] = X
        Kb = np.full((m + ldpad, n), np.nan, order="F")
        st = _lib.load().jch_kernel_gram(ctx._h, loc, kind, Zb.ctypes.data, m, m + ldpad, None, Xb.ctypes.data, n, n + ldpad, None, p,
                                         gamma, coef0, degree, Kb.ctypes.data, m + ldpad)
        ctx.check(st)
        return Kb[:m]
    Zb = J.colmajor_empty(m + ldpad, p); Zb.zero_(); Zb[:m] = torch.as_tensor(Z, device="cuda")
    if same:
        Xb = Zb
    else:
        Xb = J.colmajor_empty(n + ldpad, p); Xb.zero_(); Xb[:n] = torch.as_tensor(X, device="cuda")
    Kb = J.colmajor_empty(m + ldpad, n); Kb.fill_(float("nan"))
    torch.cuda.synchronize()
    st = _lib.load().jch_kernel_gram(ctx._h, loc, kind, Zb.data_ptr(), m, m + ldpad, None, Xb.data_ptr(), n, n + ldpad, None, p,
                                     gamma, coef0, degree, Kb.data_ptr(), m + ldpad)
    ctx.check(st)
    return Kb[:m].cpu().numpy()


# ---------------------------------------------------------------------------------- 1-4: the Gram kernel
SHAPES = [(1, 1, 1), (7, 300, 1), (257, 1000, 37), (1000, 777, 500), (64, 4101, 3)]


@pytest.mark.parametrize("m,n,p", SHAPES)
@pytest.mark.parametrize("loc", [_lib.LOC_HOST, _lib.LOC_DEVICE])
def test_krbf_against_direct_differences(ctx, m, n, p, loc):
    rng = np.random.default_rng(m * 7 + n + p)
    Z = rng.random((m, p)); X = rng.random((n, p))
    gamma = 1.0 / max(1.0, np.median(np_sqdist(Z[:50], X[:50])))
    K = raw_gram(ctx, loc, _lib.KERN_RBF, Z, X, gamma=gamma)
    assert np.max(np.abs(K - np_krbf(Z, X, gamma))) <= 1e-12


@pytest.mark.parametrize("m,n,p", SHAPES)
def test_kpol_against_numpy(ctx, m, n, p):
    rng = np.random.default_rng(m + 3 * n + p)
    Z = rng.random((m, p)); X = rng.random((n, p))
    for degree in (1, 2, 3):
        for coef0 in (0.0, 10.0):
            gamma = 1.0 / p
            ref = np_kpol(Z, X, degree, gamma, coef0)
            for loc in (_lib.LOC_HOST, _lib.LOC_DEVICE):
                K = raw_gram(ctx, loc, _lib.KERN_POL, Z, X, gamma=gamma, coef0=coef0, degree=degree)
                assert np.max(np.abs(K - ref)) <= 1e-12 * np.max(np.abs(ref)), (degree, coef0, loc)


def test_krbf_baseline_offset(ctx):
    Xa, _ = spectra(11, 400, 500, base=100.0)
    Za, _ = spectra(12, 150, 500, base=100.0)
    d = np_sqdist(Za, Xa)
    gamma = 1.0 / np.median(d)
    K = J.krbf(Za, Xa, gamma=gamma, ctx=ctx)
    assert np.max(np.abs(K - np.exp(-gamma * d))) <= 1e-12


def test_symmetric_path(ctx):
    X, _ = spectra(21, 777, 130)
    gamma = 0.5
    for loc in (_lib.LOC_HOST, _lib.LOC_DEVICE):
        Ks = raw_gram(ctx, loc, _lib.KERN_RBF, X, X, gamma=gamma, same=True)
        assert np.array_equal(Ks, Ks.T)
        assert np.all(np.diag(Ks) == 1.0)
        Kr = raw_gram(ctx, loc, _lib.KERN_RBF, X, X.copy(), gamma=gamma)   # other pointer: the rectangular path
        assert np.max(np.abs(Ks - Kr)) <= 1e-13
        Kp = raw_gram(ctx, loc, _lib.KERN_POL, X, X, gamma=0.1, coef0=1.0, degree=2, same=True)
        assert np.array_equal(Kp, Kp.T)
        assert np.max(np.abs(Kp - np_kpol(X, X, 2, 0.1, 1.0))) <= 1e-12 * np.max(np.abs(Kp))


def test_large_index(ctx):
    m, n, p = 65536, 33000, 8
    assert m * n > 2 ** 31
    rng = np.random.default_rng(5)
    Z = rng.random((m, p)); X = rng.random((n, p))
    Zd = J.colmajor_empty(m, p); Zd.copy_(torch.as_tensor(Z, device="cuda"))
    Xd = J.colmajor_empty(n, p); Xd.copy_(torch.as_tensor(X, device="cuda"))
    K = J.krbf(Zd, Xd, gamma=0.3, ctx=ctx)
    rows = np.array([0, 1, 4097, 40000, m - 2, m - 1]); cols = np.array([0, 5, 16385, n - 2, n - 1])
    Kr = K[torch.as_tensor(rows, device="cuda")].cpu().numpy()
    Kc = K[:, torch.as_tensor(cols, device="cuda")].cpu().numpy()
    assert np.max(np.abs(Kr - np_krbf(Z[rows], X, 0.3))) <= 1e-12
    assert np.max(np.abs(Kc - np_krbf(Z, X[cols], 0.3))) <= 1e-12
    del K
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------- 5-7: the fit and its accessors
def _ref_gram(kern, A, B, kw):
    if kern == "krbf":
        return np_krbf(A, B, kw.get("gamma", 1.0))
    return np_kpol(A, B, kw.get("degree", 1), kw.get("gamma", 1.0), kw.get("coef0", 0.0))


def _ref_fit(X, Y, weights, nlv, kern, scal, kw):
    X = np.array(X, dtype=float); Y = np.array(Y, dtype=float).reshape(X.shape[0], -1)
    xs = np.ones(X.shape[1]); ys = np.ones(Y.shape[1])
    if scal:
        w = O.mweight(np.ones(X.shape[0]) if weights is None else weights)
        xs = O.colstd(X, w); ys = O.colstd(Y, w)
        X = X / xs; Y = Y / ys
    K = _ref_gram(kern, X, X, kw)
    return X, O.plskern(K, Y, nlv=nlv), xs, ys


def _check_fit(fm, ref, xs, ys, what):
    s = O.sign_align(ref.W, fm.fm.W)
    errs = {f: O.rel_fro(getattr(ref, f), getattr(fm.fm, f) * s) for f in ("P", "R", "W")}
    T = fm.fm.T.cpu().numpy() if J.plsr._is_torch(fm.fm.T) else fm.fm.T
    errs["T"] = O.rel_fro(ref.T, T * s)
    errs["C"] = O.rel_fro(ref.C, fm.fm.C * s)
    errs["TT"] = O.rel_fro(ref.TT, fm.fm.TT)
    errs["xmeans"] = O.rel_fro(ref.xmeans, fm.fm.xmeans)
    errs["ymeans"] = O.rel_fro(ref.ymeans, fm.fm.ymeans)
    errs["dk_xscales"] = O.rel_fro(xs, fm.xscales)
    errs["dk_yscales"] = O.rel_fro(ys, fm.yscales)
    print(what, "TT[end]/TT[1] = %.2e" % (ref.TT[-1] / ref.TT[0]), {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) < TOL, (what, errs)


FITS = [
    dict(name="rbf", n=300, p=50, q=1, nlv=15, kern="krbf", kw=dict(gamma=0.1), scal=False, w=False),
    dict(name="pol", n=1000, p=200, q=3, nlv=20, kern="kpol", kw=dict(degree=2, coef0=10.0, gamma=0.01), scal=False, w=False),
    dict(name="scal_w", n=400, p=60, q=2, nlv=10, kern="krbf", kw=dict(gamma=0.05), scal=True, w=True),
    dict(name="q20", n=500, p=40, q=20, nlv=12, kern="krbf", kw=dict(gamma=0.1), scal=False, w=False),
    dict(name="wide", n=2500, p=80, q=1, nlv=15, kern="krbf", kw=dict(gamma=0.05), scal=False, w=False),
]


def _fit_data(c):
    X, H = spectra(100 + c["n"], c["n"], c["p"])
    X = X * 3.0
    rng = np.random.default_rng(c["n"] + c["q"])
    if c.get("kern") == "kpol":   # full-rank rows: a degree-2 kernel on a few latent bands has only a few well-determined LVs
        X = np.asfortranarray(rng.random((c["n"], c["p"])))
        H = X[:, :8]
    B = rng.standard_normal((H.shape[1], c["q"]))
    Y = np.asfortranarray(np.sin(2.0 * H) @ B + 0.01 * rng.standard_normal((c["n"], c["q"])))
    w = rng.random(c["n"]) + 0.2 if c["w"] else None
    return X, Y, w


@pytest.mark.parametrize("c", FITS, ids=[c["name"] for c in FITS])
def test_dkplsr_against_oracle(ctx, c):
    X, Y, w = _fit_data(c)
    fm = J.dkplsr(X, Y, w, nlv=c["nlv"], kern=c["kern"], scal=c["scal"], ctx=ctx, keep_gram=True, **c["kw"])
    assert isinstance(fm, J.Dkplsr) and fm.kern == c["kern"] and fm.dots == c["kw"]
    Xs, ref, xs, ys = _ref_fit(X, Y, w, c["nlv"], c["kern"], c["scal"], c["kw"])
    _check_fit(fm, ref, xs, ys, c["name"])
    # the GPU's own centred Gram through the oracle's plskern: fit parity without Gram rounding
    Kc = fm.K.cpu().numpy()
    Ycs = (Y / ys) - (Y / ys).mean(axis=0)
    ref2 = O.plskern(Kc, Ycs, nlv=c["nlv"])
    s = O.sign_align(ref2.W, fm.fm.W)
    for f in ("P", "R", "W"):
        assert O.rel_fro(getattr(ref2, f), getattr(fm.fm, f) * s) < 1e-9, f
    assert O.rel_fro(ref2.C, fm.fm.C * s) < 1e-9
    # new rows: transform / coef / predict
    Xn, _ = spectra(7 + c["n"], 37, c["p"])
    Xn = np.asfortranarray(np.random.default_rng(7).random((37, c["p"]))) if c["kern"] == "kpol" else Xn * 3.0
    Kn = _ref_gram(c["kern"], Xn / xs, Xs, c["kw"])
    Tn = J.transform(fm, Xn, ctx=ctx)
    assert O.rel_fro(O.transform(ref, Kn), Tn * s) < TOL
    pr = J.predict(fm, Xn, ctx=ctx)
    assert O.rel_fro(O.predict(ref, Kn) * ys, pr) < TOL
    B, b0 = J.coef(fm)
    Br, b0r = O.coef(ref)
    assert O.rel_fro(Br, B) < TOL and O.rel_fro(b0r, b0) < TOL


def test_dkplsr_sinc_example(ctx):
    """The reference's own 1-D example (src/dkplsr.jl docstring: sinc after Rosipal & Trejo 2001)."""
    x = np.arange(-10, 10.0001, 0.2)
    x[np.abs(x) < 1e-12] = 1e-5
    y = np.sin(np.abs(x)) / np.abs(x) + 0.2 * np.random.default_rng(3).standard_normal(x.size)
    fm = J.dkplsr(x, y, nlv=2, ctx=ctx)
    Xs, ref, xs, ys = _ref_fit(x.reshape(-1, 1), y, None, 2, "krbf", False, {})
    _check_fit(fm, ref, xs, ys, "sinc")
    pred = J.predict(fm, x, ctx=ctx)
    assert O.rel_fro(O.predict(ref, _ref_gram("krbf", Xs, Xs, {})), pred) < TOL


def test_weights_enter_only_the_scales(ctx):
    X, Y, _ = _fit_data(dict(n=300, p=30, q=2, w=False))
    w = np.random.default_rng(9).random(300) + 0.1
    a = J.dkplsr(X, Y, nlv=8, gamma=0.1, ctx=ctx)
    b = J.dkplsr(X, Y, w, nlv=8, gamma=0.1, ctx=ctx)
    for f in ("T", "P", "R", "W", "C", "TT", "xmeans", "ymeans"):
        assert np.array_equal(getattr(a.fm, f), getattr(b.fm, f)), f
    c1 = J.dkplsr(X, Y, nlv=8, gamma=0.1, scal=True, ctx=ctx)
    c2 = J.dkplsr(X, Y, w, nlv=8, gamma=0.1, scal=True, ctx=ctx)
    wn = O.mweight(w)
    assert O.rel_fro(O.colstd(X, wn), c2.xscales) < 1e-12 and O.rel_fro(O.colstd(Y, wn), c2.yscales) < 1e-12
    assert not np.array_equal(c1.xscales, c2.xscales)
    assert np.allclose(c2.fm.weights, 1.0 / 300)


@pytest.mark.parametrize("m", [1, 777])
def test_predict_new_rows_and_blocks(ctx, monkeypatch, m):
    c = dict(n=600, p=45, q=2, w=True)
    X, Y, w = _fit_data(c)
    fm = J.dkplsr(X, Y, w, nlv=10, gamma=0.2, scal=True, ctx=ctx)
    Xs, ref, xs, ys = _ref_fit(X, Y, w, 10, "krbf", True, dict(gamma=0.2))
    Xn, _ = spectra(77, m, 45)
    Kn = _ref_gram("krbf", Xn / xs, Xs, dict(gamma=0.2))
    s = O.sign_align(ref.W, fm.fm.W)
    one = J.predict(fm, Xn, nlv=6, ctx=ctx)
    assert O.rel_fro(O.predict(ref, Kn, nlv=6) * ys, one) < TOL
    rng_ = J.predict(fm, Xn, nlv=range(0, 11), ctx=ctx)
    refs = O.predict(ref, Kn, nlv=range(0, 11))
    for a, b in zip(refs, rng_):
        assert O.rel_fro(a * ys, b) < TOL
    T1 = J.transform(fm, Xn, nlv=7, ctx=ctx)
    assert O.rel_fro(O.transform(ref, Kn, nlv=7), T1 * s[:7]) < TOL
    Xnd = J.colmajor_empty(m, 45); Xnd.copy_(torch.as_tensor(Xn, device="cuda"))
    monkeypatch.setenv("JCH_DKPLSR_QBLOCK", "64")
    rng_b = J.predict(fm, Xn, nlv=range(0, 11), ctx=ctx)
    T1b = J.transform(fm, Xn, nlv=7, ctx=ctx)
    for a, b in zip(rng_, rng_b):
        assert np.array_equal(a, b)
    assert np.array_equal(T1, T1b)
    monkeypatch.delenv("JCH_DKPLSR_QBLOCK")
    # device-resident model and rows give the same numbers
    fmd = J.dkplsr(torch.as_tensor(X, device="cuda").t().contiguous().t(), torch.as_tensor(Y, device="cuda").t().contiguous().t(),
                   torch.as_tensor(w, device="cuda"), nlv=10, gamma=0.2, scal=True, ctx=ctx)
    pd = J.predict(fmd, Xnd, nlv=6, ctx=ctx)
    assert np.array_equal(pd.cpu().numpy(), one)


def test_copy_semantics(ctx):
    X, Y, w = _fit_data(dict(n=250, p=20, q=2, w=True))
    X0, Y0 = X.copy(), Y.copy()
    a = J.dkplsr(X, Y, w, nlv=6, gamma=0.1, scal=True, ctx=ctx)
    assert np.array_equal(X, X0) and np.array_equal(Y, Y0)
    Xd = J.colmajor_empty(250, 20); Xd.copy_(torch.as_tensor(X, device="cuda"))
    Yd = J.colmajor_empty(250, 2); Yd.copy_(torch.as_tensor(Y, device="cuda"))
    Xd0, Yd0 = Xd.clone(), Yd.clone()
    b = J.dkplsr(Xd, Yd, torch.as_tensor(w, device="cuda"), nlv=6, gamma=0.1, scal=True, ctx=ctx)
    assert torch.equal(Xd, Xd0) and torch.equal(Yd, Yd0)
    for f in ("P", "R", "W", "C", "TT", "xmeans", "ymeans"):
        assert np.array_equal(getattr(a.fm, f), getattr(b.fm, f)), f
    assert np.array_equal(a.fm.T, b.fm.T.cpu().numpy())
    # dkplsr!: X and Y come back scaled (src/dkplsr.jl:117-118); Y also centred, as plskern!(K, Y) leaves it (:122)
    Xi, Yi = X.copy(order="F"), Y.copy(order="F")
    c = J.dkplsr_(Xi, Yi, w, nlv=6, gamma=0.1, scal=True, ctx=ctx)
    assert np.allclose(Xi, X / c.xscales, rtol=0, atol=0)
    Ys = Y / c.yscales
    assert np.max(np.abs(Yi - (Ys - Ys.mean(axis=0)))) < 1e-13
    assert c.X is Xi
    for f in ("P", "R", "C", "TT"):
        assert np.array_equal(getattr(a.fm, f), getattr(c.fm, f)), f


def test_gridscorelv_with_dkplsr(ctx):
    X, Y, _ = _fit_data(dict(n=300, p=25, q=1, w=False))
    Xt, Yt, Xv, Yv = X[:220].copy(order="F"), Y[:220].copy(order="F"), X[220:].copy(order="F"), Y[220:].copy(order="F")
    pars = J.mpar(gamma=[0.01, 0.1, 1.0])
    res = J.gridscorelv(Xt, Yt, Xv, Yv, score=J.rmsep, fun=J.dkplsr, nlv=range(0, 11), pars=pars, ctx=ctx)
    rows = []
    for g in pars["gamma"]:
        fm = J.dkplsr(Xt, Yt, nlv=10, gamma=g, ctx=ctx)
        for pr in J.predict(fm, Xv, nlv=range(0, 11), ctx=ctx):
            rows.append(np.asarray(J.rmsep(pr, Yv)).reshape(1, -1))
    assert np.array_equal(np.vstack(rows), np.asarray(res["res"]))
    assert res["gamma"] == [g for g in pars["gamma"] for _ in range(11)]


def test_errors(ctx):
    L = _lib.load()
    X = np.asfortranarray(np.random.default_rng(0).random((20, 4)))
    Y = np.asfortranarray(np.random.default_rng(1).random((20, 1)))
    out = [np.zeros((20, 5)) for _ in range(4)]

    def fit(dtype=_lib.F64, kind=_lib.KERN_RBF, degree=1):
        d = _lib.PlsDesc(n=20, p=4, q=1, nlv=3, scal=0, dtype=dtype, loc=_lib.LOC_HOST, inplace=0, reserved=0)
        got = C.c_int32(0)
        return L.jch_dkplsr_fit(ctx._h, C.byref(d), kind, 1.0, 0.0, degree, X.ctypes.data, 20, Y.ctypes.data, 20, None, None,
                                None, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, None, None, None, None, None, None, None,
                                None, None, C.byref(got))

    for kw in (dict(dtype=_lib.BF16), dict(kind=7), dict(kind=_lib.KERN_POL, degree=0)):
        assert fit(**kw) == _lib.JCH_EINVAL, kw
        assert L.jch_last_error(ctx._h).decode()
    K = np.zeros((20, 20), order="F")
    st = L.jch_kernel_gram(ctx._h, _lib.LOC_HOST, _lib.KERN_RBF, X.ctypes.data, 20, 20, None, X.ctypes.data, 20, 20, None, 4, 1.0, 0.0, 1,
                           K.ctypes.data, 19)
    assert st == _lib.JCH_EINVAL and b"ldk" in L.jch_last_error(ctx._h)
    assert fit() == _lib.JCH_OK   # the ctx is still usable


def test_full_size_fit(ctx):
    c = dict(n=8192, p=512, q=1, w=False)
    X, Y, _ = _fit_data(c)
    Xd = J.colmajor_empty(8192, 512); Xd.copy_(torch.as_tensor(X, device="cuda"))
    Yd = J.colmajor_empty(8192, 1); Yd.copy_(torch.as_tensor(Y, device="cuda"))
    gamma = 0.02
    fm = J.dkplsr(Xd, Yd, nlv=25, gamma=gamma, ctx=ctx)
    XX = np.einsum("ij,ij->i", X, X)
    K = np.exp(-gamma * np.maximum(XX[:, None] + XX[None, :] - 2.0 * X @ X.T, 0.0))
    ref = O.plskern(K, Y, nlv=25)
    s = O.sign_align(ref.W, fm.fm.W)
    errs = {f: O.rel_fro(getattr(ref, f), getattr(fm.fm, f) * s) for f in ("P", "R", "W")}
    errs["T"] = O.rel_fro(ref.T, fm.fm.T.cpu().numpy() * s)
    errs["C"] = O.rel_fro(ref.C, fm.fm.C * s)
    print("full size TT[end]/TT[1] = %.2e" % (ref.TT[-1] / ref.TT[0]), errs)
    assert max(errs.values()) < TOL, errs


# ---------------------------------------------------------------------------------- the three routes of the C entries (tests/host_routes.py)
@pytest.mark.parametrize("entry", sorted(__import__("host_routes").ROUTES["dkplsr"]))
def test_host_arrays_padded_and_unpadded_give_the_bits_of_the_device_route(entry):
    """Device buffers, host arrays with ld == rows and with ld = rows + 3 between NaN guards: equal bytes, NaN padding kept, inputs unchanged."""
    import host_routes as HR
    HR.three_routes(HR.ROUTES["dkplsr"][entry])
