"""kpca on the GPU against the literal numpy restatement of src/kpca.jl (test_kpca_static.np_kpca), the panel kernel jch_kc_panel
against numpy, the edges of the eigensolver, determinism, and the full-size fit against scipy's eigsh."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_kpca_static import _data, np_kpca, np_kpca_summary, np_kpca_transform  # noqa: E402

TOL = 1e-10


@pytest.fixture(scope="module")
def J():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import jchemo_hip
    return jchemo_hip


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _weights(kind, n, seed=5):
    if kind == "ones":
        return None
    rng = np.random.default_rng(seed)
    w = rng.random(n) + 0.05
    if kind == "zeros":
        w[rng.choice(n, n // 10, replace=False)] = 0.0
    return w


def _gaps(eig, k):
    g = np.empty(k)
    for i in range(k):
        others = np.delete(eig, i)
        g[i] = np.min(np.abs(others - eig[i]))
    return g


def _compare_columns(A, B, eig, nlv, scale, tol=TOL):
    """Columns of A and B (sign-aligned) within 10 tol eig_1 / gap_i (relative to `scale`); a column whose gap is below the
    bound's reach is compared with its cluster as a subspace."""
    gaps = _gaps(eig, nlv)
    for i in range(nlv):
        bound = 10 * tol * eig[0] / gaps[i]
        if bound < 1e-3:
            a, b = A[:, i], B[:, i]
            s = 1.0 if a @ b >= 0 else -1.0
            assert np.linalg.norm(a - s * b) <= max(bound, 1e-11) * scale[i] + 1e-13 * np.linalg.norm(b), (i, bound)
        else:   # cluster: the span of the columns whose eigenvalues are within 1e-3 eig_1 of this one
            idx = [j for j in range(nlv) if abs(eig[j] - eig[i]) < 1e-3 * eig[0]]
            Qa, _ = np.linalg.qr(A[:, idx]); Qb, _ = np.linalg.qr(B[:, idx])
            assert np.linalg.svd(Qa.T @ Qb, compute_uv=False).min() > 1 - 1e-6


CASES = [("krbf", dict(gamma=0.5), False, "ones", 1, 150), ("krbf", dict(gamma=0.2), True, "rand", 3, 400),
         ("krbf", dict(gamma=1.0), False, "zeros", 10, 777), ("kpol", dict(degree=2, gamma=0.5, coef0=1.0), False, "ones", 3, 301),
         ("kpol", dict(degree=3, gamma=0.3, coef0=0.5), True, "zeros", 10, 512), ("krbf", dict(gamma=0.3), True, "rand", 25, 2000),
         ("kpol", dict(degree=1, gamma=1.0, coef0=0.0), False, "rand", 3, 1001)]


@pytest.mark.parametrize("kern,kw,scal,wkind,nlv,n", CASES)
def test_parity_with_the_restatement(J, kern, kw, scal, wkind, nlv, n):
    p = 9
    X = _data(n, p, n)
    X0 = X.copy()
    w = _weights(wkind, n)
    ref = np_kpca(X, w, nlv=nlv, kern=kern, scal=scal, **kw)
    fm = J.kpca(X, w, nlv=nlv, kern=kern, scal=scal, **kw)
    assert np.array_equal(X, X0)
    assert fm.converged and fm.niter >= 1
    e1 = ref["eig"][0]
    assert np.max(np.abs(fm.eig - ref["eig"][:nlv])) <= 1e-10 * e1
    assert np.max(np.abs(fm.sv ** 2 - ref["eig"][:nlv])) <= 1e-10 * e1
    assert np.isclose(fm.sstot, ref["eig"].sum(), rtol=1e-12)
    assert np.allclose(fm.xscales, ref["xscales"], rtol=1e-13)
    sw = np.sqrt(ref["D"])
    P, T = _host(fm.P), _host(fm.T)
    U = np.where(sw[:, None] > 0, P * fm.sv[None, :] / np.where(sw > 0, sw, 1.0)[:, None], 0.0)   # U = P sv / sqrtw (0 on zero weights)
    _compare_columns(U, ref["U"], ref["eig"], nlv, np.ones(nlv))
    _compare_columns(P, ref["P"], ref["eig"], nlv, np.linalg.norm(ref["P"], axis=0))
    _compare_columns(T, ref["T"], ref["eig"], nlv, np.linalg.norm(ref["T"], axis=0))
    # sign rule: the largest-|.| entry of every U column is positive
    for i in range(nlv):
        assert U[np.argmax(np.abs(U[:, i])), i] > 0
    # transform on new rows and summary against the restatement (sign-aligned)
    Xn = _data(50, p, n + 1)
    sg = np.sign(np.sum(U * ref["U"], axis=0))
    Tn = _host(J.kpca_transform(fm, Xn))
    Tr = np_kpca_transform(ref, Xn) * sg
    gaps = _gaps(ref["eig"], nlv)
    for i in range(nlv):
        if 10 * TOL * e1 / gaps[i] < 1e-3:
            assert np.linalg.norm(Tn[:, i] - Tr[:, i]) <= max(1e-9, 100 * TOL * e1 / gaps[i]) * max(np.linalg.norm(Tr[:, i]), 1e-300) + 1e-12
    sm, smr = J.kpca_summary(fm), np_kpca_summary(ref)
    assert np.array_equal(sm["lv"], smr["lv"])
    assert np.allclose(sm["var"], smr["var"], rtol=1e-9, atol=1e-12 * e1)
    assert np.allclose(sm["pvar"], smr["pvar"], rtol=1e-9, atol=1e-12)
    assert np.allclose(sm["cumpvar"], smr["cumpvar"], rtol=1e-9, atol=1e-12)


def test_nlv_clamped_and_the_b_equals_n_path(J):
    n = 150
    X = _data(n, 6, 11)
    fm = J.kpca(X, nlv=n + 20, gamma=0.5)
    ref = np_kpca(X, nlv=n, gamma=0.5)
    assert fm.T.shape == (n, n) and fm.eig.shape == (n,)
    assert fm.niter == 1 and fm.converged   # b == n: one Rayleigh-Ritz step is exact
    assert np.max(np.abs(fm.eig - ref["eig"])) <= 1e-10 * ref["eig"][0]
    k = 10
    _compare_columns(_host(fm.T)[:, :k], ref["T"][:, :k], ref["eig"], k, np.linalg.norm(ref["T"][:, :k], axis=0))


def test_rank_deficient_kd(J):
    n = 300
    X = np.asfortranarray(np.random.default_rng(2).standard_normal((n, 5)))
    fm = J.kpca(X, nlv=10, kern="kpol", degree=1, gamma=1.0, coef0=0.0)   # rank(Kd) <= 5 (the constant term is centred out)
    ref = np_kpca(X, nlv=10, kern="kpol", degree=1, gamma=1.0, coef0=0.0)
    assert np.all(np.isfinite(fm.eig))
    assert np.max(np.abs(fm.eig - ref["eig"][:10])) <= 1e-10 * ref["eig"][0]
    k = 5
    _compare_columns(_host(fm.T)[:, :k], ref["T"][:, :k], ref["eig"], k, np.linalg.norm(ref["T"][:, :k], axis=0))


def test_near_constant_kernel(J):
    n = 200
    X = _data(n, 8, 12)
    fm = J.kpca(X, nlv=3, gamma=1e-6)
    ref = np_kpca(X, nlv=3, gamma=1e-6)
    assert np.all(np.isfinite(fm.eig))
    assert np.max(np.abs(fm.eig - ref["eig"][:3])) <= 1e-10 * ref["eig"][0]
    assert np.isclose(fm.sstot, ref["eig"].sum(), rtol=1e-9)


def test_indefinite_kpol(J):
    n = 250
    X = _data(n, 6, 13)
    kw = dict(kern="kpol", degree=3, gamma=1.0, coef0=-0.5)
    fm = J.kpca(X, nlv=6, **kw)
    ref = np_kpca(X, nlv=6, **kw)
    assert np.max(np.abs(fm.eig - ref["eig"][:6])) <= 1e-10 * ref["eig"][0]   # ordered by |lambda|, as the singular values
    _compare_columns(_host(fm.T), ref["T"], ref["eig"], 6, np.linalg.norm(ref["T"], axis=0))
    assert np.isnan(fm.sstot)
    with pytest.raises(ValueError, match="PSD"):
        J.kpca_summary(fm)
    assert _host(J.kpca_transform(fm, X[:7])).shape == (7, 6)


def test_maxit_one_warns_without_error(J):
    X = _data(500, 8, 14)
    with pytest.warns(RuntimeWarning, match="did not converge"):
        fm = J.kpca(X, nlv=10, gamma=0.3, eig_maxit=1)
    assert fm.niter == 1 and not fm.converged
    assert fm.resid.shape == (10,) and np.all(np.isfinite(fm.resid))


def test_determinism_host_device_and_keep_gram(J):
    n, p = 700, 9
    X = _data(n, p, 15)
    w = _weights("rand", n)
    a = J.kpca(X, w, nlv=8, gamma=0.4, scal=True)
    b = J.kpca(X, w, nlv=8, gamma=0.4, scal=True)
    for f in ("T", "P", "vtot", "sv", "eig", "resid", "xscales"):
        assert np.array_equal(_host(getattr(a, f)), _host(getattr(b, f))), f
    assert a.niter == b.niter and a.sstot == b.sstot
    Xd = J.colmajor_empty(n, p, "cuda:0"); Xd.copy_(torch.as_tensor(X))
    wd = torch.as_tensor(w, device="cuda:0")
    Xd0 = Xd.clone()
    c = J.kpca(Xd, wd, nlv=8, gamma=0.4, scal=True, keep_gram=True)
    assert torch.equal(Xd, Xd0)
    assert isinstance(c.T, torch.Tensor) and c.T.is_cuda
    for f in ("T", "P", "vtot", "sv", "eig", "resid", "xscales"):
        assert np.array_equal(_host(getattr(a, f)), _host(getattr(c, f))), f
    Kt = _host(c.Kt)
    from test_kplsr_static import np_kern
    Kr = np_kern("krbf", X / a.xscales, X / a.xscales, gamma=0.4)
    assert np.max(np.abs(Kt - Kr)) < 1e-12
    assert np.array_equal(_host(J.kpca_transform(a, X[:30])), _host(J.kpca_transform(c, torch.as_tensor(X[:30], device="cuda:0"))))


@pytest.mark.parametrize("n,b", [(1, 16), (7, 16), (129, 32), (1000, 48), (1001, 64), (4099, 80), (517, 5)])
def test_panel_kernel(J, n, b):
    from jchemo_hip import _lib
    rng = np.random.default_rng(n + b)
    Kc = rng.standard_normal((n, n))          # general (non-symmetric) matrix: out = Kc V, not Kc' V
    V = rng.standard_normal((n, b))
    ldv = n + 3
    Kd = J.colmajor_empty(n, n, "cuda:0"); Kd.copy_(torch.as_tensor(Kc))
    Vd = J.colmajor_empty(ldv, b, "cuda:0"); Vd.zero_(); Vd[:n].copy_(torch.as_tensor(V))
    out = J.colmajor_empty(n, b, "cuda:0")
    ctx = J.default_context(0)
    torch.cuda.synchronize()
    ctx.check(_lib.load().jch_kc_panel(ctx._h, Kd.data_ptr(), n, Vd.data_ptr(), ldv, b, out.data_ptr(), n))
    ref = Kc @ V
    err = np.abs(_host(out) - ref).max() / (np.abs(Kc).max() * np.abs(V).max() * n)
    assert err < 1e-15
    out2 = J.colmajor_empty(n, b, "cuda:0")
    ctx.check(_lib.load().jch_kc_panel(ctx._h, Kd.data_ptr(), n, Vd.data_ptr(), ldv, b, out2.data_ptr(), n))
    assert torch.equal(out, out2)


def test_full_size_against_eigsh(J):
    from scipy.sparse.linalg import eigsh
    n, p, nlv = 16384, 512, 25
    g = torch.Generator(device="cpu").manual_seed(1)
    grid = torch.linspace(0, 1, p, dtype=torch.float64)
    cen = torch.tensor([0.15, 0.3, 0.45, 0.6, 0.75, 0.9], dtype=torch.float64)
    H = torch.rand(n, cen.numel(), generator=g, dtype=torch.float64)
    Xh = 3.0 * (H @ torch.exp(-((grid[None, :] - cen[:, None]) / 0.06) ** 2)) + 0.03 * torch.randn(n, p, generator=g, dtype=torch.float64)
    X = J.colmajor_empty(n, p, "cuda:0"); X.copy_(Xh.to("cuda:0"))
    fm = J.kpca(X, nlv=nlv, gamma=1.0 / p, keep_gram=True)
    assert fm.converged
    K = fm.Kt
    w = torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda:0")
    vt = K @ w
    Kd = ((K - vt[:, None] - vt[None, :] + w @ vt) / n).cpu().numpy()   # sqrtD Kc sqrtD with uniform weights
    del K
    fm.Kt = None
    torch.cuda.empty_cache()
    U = _host(fm.P) * fm.sv[None, :] * np.sqrt(n)
    assert np.abs(U.T @ U - np.eye(nlv)).max() < 1e-12
    R = Kd @ U - U * fm.eig[None, :]
    assert np.linalg.norm(R, axis=0).max() <= 10 * TOL * fm.eig[0]
    vals, _ = eigsh(Kd, k=nlv, which="LA", tol=1e-13)
    vals = np.sort(vals)[::-1]
    assert np.max(np.abs(fm.eig - vals)) <= 1e-10 * fm.eig[0]


# ---------------------------------------------------------------------------------- the three routes of the C entries (tests/host_routes.py)
@pytest.mark.parametrize("entry", sorted(__import__("host_routes").ROUTES["kpca"]))
def test_host_arrays_padded_and_unpadded_give_the_bits_of_the_device_route(entry):
    """Device buffers, host arrays with ld == rows and with ld = rows + 3 between NaN guards: equal bytes, NaN padding kept, inputs unchanged."""
    import host_routes as HR
    HR.three_routes(HR.ROUTES["kpca"][entry])
