"""krr on the GPU: the Cholesky primitives (jch_chol_factor / jch_chol_solve / jch_chol_inv_fro2) against scipy, their breakdown
path, krr / krr_coef / krr_predict / gridscorelb / krrda against the literal numpy restatement of src/krr.jl
(test_krr_static.np_krr, full SVD), determinism, and the full-size solve against scipy's Cholesky.

Tolerances of the parity tests: per case, cond = (eig_max + lb^2) / (eig_min + lb^2) from the restatement's own singular values
and the two-route gap g = restatement (SVD) against scipy Cholesky on the CPU; the GPU may differ from the restatement by at most
max(10 g, 50 eps cond) for A and the predictions (relative Frobenius, predictions after subtracting ymeans) and max(10 g, 10 n eps
cond) absolute for df, and never by more than the project's parity tolerance 1e-6 (df: relative to df)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_kpca import CASES, _host, _weights  # noqa: E402
from test_kpca_static import _data  # noqa: E402
from test_krr_static import chol_route, np_krr, np_krr_coef, np_krr_predict  # noqa: E402

EPS = float(np.finfo(np.float64).eps)
CAP = 1e-6


@pytest.fixture(scope="module")
def J():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import jchemo_hip
    return jchemo_hip


def _rel(a, b, scale=None):
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b if scale is None else scale), 1e-300))


def _dev(J, A, ld=None):
    A = np.asarray(A, dtype=np.float64)
    n, m = A.shape
    ld = n if ld is None else ld
    D = J.colmajor_empty(ld, m, "cuda:0")
    D.zero_()
    D[:n].copy_(torch.as_tensor(A))
    return D


def _spd(n, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    return M @ M.T / n + np.eye(n)


def _factor(J, Ad, n, lda):
    from jchemo_hip import _lib
    ctx = J.default_context(0)
    info = C.c_int32(-7)
    torch.cuda.synchronize()
    st = _lib.load().jch_chol_factor(ctx._h, Ad.data_ptr(), n, lda, C.byref(info))
    return ctx, st, info.value


# ---------------------------------------------------------------------------------- the primitives
@pytest.mark.parametrize("n", [1, 17, 127, 128, 129, 257, 1000, 2049])
@pytest.mark.parametrize("pad", [0, 3])
def test_cholesky_primitives_against_scipy(J, n, pad):
    """Bounds: Cholesky and the triangular solves are backward stable with constants gamma_k = k eps / (1 - k eps), k <= n + 1 per
    row (Higham, Accuracy and Stability, thm 10.3 / 8.5), so the forward errors are <= (n + 10) eps cond(A) in norm; the matrices
    M M' / n + I have cond <= 5 + 1."""
    from jchemo_hip import _lib
    from scipy.linalg import cho_solve, cholesky, solve_triangular
    A = _spd(n, n)
    cond = np.linalg.cond(A)
    bound = (n + 10) * EPS * cond
    lda = n + pad
    Aup = A.copy()
    Aup[np.triu_indices(n, 1)] = np.nan            # only the lower triangle may be read
    Ad = _dev(J, Aup, lda)
    ctx, st, info = _factor(J, Ad, n, lda)
    assert st == 0 and info == 0
    Lref = cholesky(A, lower=True)
    Lg = np.tril(_host(Ad)[:n])
    print(f"n={n} lda={lda} factor rel err {_rel(Lg, Lref):.3e} bound {bound:.3e}")
    assert _rel(Lg, Lref) <= bound
    up = _host(Ad)[:n][np.triu_indices(n, 1)]
    assert up.size == 0 or np.all(np.isnan(up))   # the upper triangle is not written either
    L = _lib.load()
    for q in (1, 3, 33, 70):
        B = np.random.default_rng(n + q).standard_normal((n, q))
        ldb = n + (q % 2)
        Bd = _dev(J, B, ldb)
        torch.cuda.synchronize()
        ctx.check(L.jch_chol_solve(ctx._h, Ad.data_ptr(), n, lda, Bd.data_ptr(), q, ldb))
        Xref = cho_solve((Lref, True), B)
        err = _rel(_host(Bd)[:n], Xref)
        print(f"  q={q} solve rel err {err:.3e}")
        assert err <= 2 * bound                      # two substitutions
        Bd2 = _dev(J, B, ldb)
        torch.cuda.synchronize()
        ctx.check(L.jch_chol_solve(ctx._h, Ad.data_ptr(), n, lda, Bd2.data_ptr(), q, ldb))
        assert torch.equal(Bd, Bd2)
    out = C.c_double(0.0)
    ctx.check(L.jch_chol_inv_fro2(ctx._h, Ad.data_ptr(), n, lda, C.byref(out)))
    fref = float(np.sum(solve_triangular(Lref, np.eye(n), lower=True) ** 2))
    print(f"  inv_fro2 rel err {abs(out.value - fref) / fref:.3e}")
    assert abs(out.value - fref) <= 2 * bound * fref
    # a solve against anything but the last factor is refused
    other = _dev(J, A, n)
    torch.cuda.synchronize()
    Bd = _dev(J, np.ones((n, 1)))
    assert L.jch_chol_solve(ctx._h, other.data_ptr(), n, n, Bd.data_ptr(), 1, n) == _lib.JCH_EINVAL
    assert L.jch_chol_solve(ctx._h, Ad.data_ptr(), n, lda + 1, Bd.data_ptr(), 1, n) == _lib.JCH_EINVAL


def test_breakdown_is_reported_not_raised(J):
    """Status check of the info path (chol.hip k_chol_diag: a pivot that is not > 0 stores its 1-based column with one
    compare-and-swap and the workgroup returns; every other kernel returns on a non-zero info word).  Bad numbers only."""
    from jchemo_hip import _lib
    n, j = 300, 200
    rng = np.random.default_rng(1)
    L0 = np.eye(n) + 0.1 * np.tril(rng.standard_normal((n, n)), -1) / np.sqrt(n)
    d = np.ones(n)
    d[j] = -1.0                                          # A = L0 diag(d) L0': the leading minors are positive up to j, then negative
    cases = [(L0 @ (d[:, None] * L0.T), j + 1), (np.zeros((n, n)), 1)]
    A = _spd(n, 2)
    A[150, 150] = np.nan
    cases.append((A, 151))
    lib = _lib.load()
    for A, want in cases:
        Ad = _dev(J, A)
        ctx, st, info = _factor(J, Ad, n, n)
        assert st == 0 and info == want, (st, info, want)
        Bd = _dev(J, np.ones((n, 2)))
        torch.cuda.synchronize()
        assert lib.jch_chol_solve(ctx._h, Ad.data_ptr(), n, n, Bd.data_ptr(), 2, n) == _lib.JCH_EINVAL    # no factor to solve with
        # the next call on the same ctx works
        G = _spd(n, 3)
        Gd = _dev(J, G)
        ctx, st, info = _factor(J, Gd, n, n)
        assert st == 0 and info == 0
        torch.cuda.synchronize()
        ctx.check(lib.jch_chol_solve(ctx._h, Gd.data_ptr(), n, n, Bd.data_ptr(), 2, n))
        assert _rel(_host(Bd), np.linalg.solve(G, np.ones((n, 2)))) < 1e-12


def test_krr_on_an_indefinite_kernel_reports_the_column(J):
    from jchemo_hip._lib import JCH_EINVAL, JchError
    n = 250
    X = _data(n, 6, 13)
    Y = X[:, :2].copy()
    kw = dict(kern="kpol", degree=3, gamma=1.0, coef0=-0.5)
    lb = 1e-4
    ref = np_krr(X, Y, lb=lb, svd=False, **kw)
    assert np.linalg.eigvalsh(ref["Kd"]).min() < -10 * lb ** 2      # not PSD enough for this lb
    fm = J.krr(X, Y, lb=lb, **kw)
    with pytest.raises(JchError, match=r"column \d+") as e:
        J.krr_coef(fm)
    assert e.value.code == JCH_EINVAL
    A, _, df = J.krr_coef(fm, lb=10.0)                              # the same model and ctx, a usable lb
    ref2 = chol_route(ref, 10.0)
    assert _rel(_host(A), ref2["A"]) < 1e-9 and abs(df - ref2["df"]) < 1e-9 * ref2["df"]


# ---------------------------------------------------------------------------------- parity with the restatement
def _lbs(kern, kw, scal):
    cubic = kern == "kpol" and kw.get("degree") == 3 and scal   # leading eigenvalue of Kd 1.07e3 instead of ~0.1
    return [10.0, 1.0, 1e-1] if cubic else [1e-1, 1e-2, 1e-3]


@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("kern,kw,scal,wkind,_nlv,n", CASES)
def test_parity_with_the_restatement(J, kern, kw, scal, wkind, _nlv, n, q):
    p = 9
    X = _data(n, p, n)
    Y = np.asfortranarray(np.random.default_rng(n + q).standard_normal((n, q)) * 0.1 + X[:, :q] ** 2)
    X0, Y0 = X.copy(), Y.copy()
    w = _weights(wkind, n)
    lbs = _lbs(kern, kw, scal)
    ref = np_krr(X, Y, w, lb=lbs[0], kern=kern, scal=scal, **kw)
    fm = J.krr(X, Y, w, lb=lbs[0], kern=kern, scal=scal, **kw)
    assert np.array_equal(X, X0) and np.array_equal(Y, Y0)
    assert np.allclose(fm.xscales, ref["xscales"], rtol=1e-13) and np.allclose(fm.ymeans, ref["ymeans"], rtol=1e-13, atol=1e-15)
    assert _rel(_host(fm.vtot).ravel(), ref["vtot"]) < 1e-12
    assert _rel(_host(fm.Kd), ref["Kd"]) < 1e-12 and _rel(_host(fm.B), ref["DY"]) < 1e-14
    Xn = _data(50, p, n + 1)
    eig = ref["sv"] ** 2
    preds_seq = J.krr_predict(fm, Xn, lb=lbs)
    assert isinstance(preds_seq, list) and len(preds_seq) == len(lbs)
    zero = np.where(ref["weights"] == 0)[0]
    for i, lb in enumerate(lbs):
        cond = (eig.max() + lb ** 2) / (eig.min() + lb ** 2)
        r, c = np_krr_coef(ref, lb), chol_route(ref, lb, Xn)
        rp = np_krr_predict(ref, Xn, lb)
        g_A, g_p, g_df = _rel(c["A"], r["A"]), _rel(c["pred"], rp, rp - ref["ymeans"]), abs(c["df"] - r["df"])
        A, b0, df = J.krr_coef(fm, lb=lb)
        pred = _host(J.krr_predict(fm, Xn, lb=lb))
        e_A, e_p, e_df = _rel(_host(A), r["A"]), _rel(pred, rp, rp - ref["ymeans"]), abs(df - r["df"])
        tol_A, tol_p = min(max(10 * g_A, 50 * EPS * cond), CAP), min(max(10 * g_p, 50 * EPS * cond), CAP)
        tol_df = min(max(10 * g_df, 10 * n * EPS * cond), CAP * r["df"])
        print(f"{kern} scal={scal} w={wkind} n={n} q={q} lb={lb:g} cond={cond:.3e} eps*cond={EPS * cond:.3e} | A gpu {e_A:.3e} gap {g_A:.3e} tol {tol_A:.3e}"
              f" | pred gpu {e_p:.3e} gap {g_p:.3e} tol {tol_p:.3e} | df={r['df']:.6g} gpu {e_df:.3e} gap {g_df:.3e} tol {tol_df:.3e}")
        assert e_A <= tol_A and e_p <= tol_p and e_df <= tol_df
        assert np.array_equal(b0, ref["ymeans"].reshape(1, -1)) or np.allclose(b0, ref["ymeans"].reshape(1, -1), rtol=1e-13, atol=1e-15)
        assert np.array_equal(_host(preds_seq[i]), pred)                # a sequence of lb equals the single-lb calls bit for bit
        if zero.size:
            assert np.abs(_host(A)[zero]).max() == 0.0                  # zero-weight rows: A rows of 0
    # krr_ works in place: X comes back scaled, Y untouched
    X1, Y1 = X0.copy(order="F"), Y0.copy(order="F")
    fm2 = J.krr_(X1, Y1, w, lb=lbs[0], kern=kern, scal=scal, **kw)
    assert np.array_equal(Y1, Y0)
    assert np.allclose(X1, X0 / ref["xscales"], rtol=1e-14) and (scal or np.array_equal(X1, X0))
    assert np.array_equal(_host(J.krr_coef(fm2, df=False)[0]), _host(J.krr_coef(fm, lb=lbs[0], df=False)[0]))


def test_determinism_and_host_equals_device(J):
    n, p, q = 700, 9, 3
    X = _data(n, p, 15)
    Y = np.asfortranarray(np.random.default_rng(16).standard_normal((n, q)))
    w = _weights("rand", n)
    kw = dict(lb=1e-2, gamma=0.4, scal=True)
    a, b = J.krr(X, Y, w, **kw), J.krr(X, Y, w, **kw)
    Xd = J.colmajor_empty(n, p, "cuda:0"); Xd.copy_(torch.as_tensor(X))
    Yd = J.colmajor_empty(n, q, "cuda:0"); Yd.copy_(torch.as_tensor(Y))
    Xd0, Yd0 = Xd.clone(), Yd.clone()
    c = J.krr(Xd, Yd, torch.as_tensor(w, device="cuda:0"), **kw)
    assert torch.equal(Xd, Xd0) and torch.equal(Yd, Yd0)
    assert isinstance(c.B, torch.Tensor) and c.B.is_cuda
    Xn = _data(30, p, 17)
    ra = J.krr_coef(a)
    for other, xn in ((b, Xn), (c, torch.as_tensor(Xn, device="cuda:0"))):
        for f in ("Kd", "B", "vtot", "xscales", "ymeans", "weights"):
            assert np.array_equal(_host(getattr(a, f)), _host(getattr(other, f))), f
        ro = J.krr_coef(other)
        assert np.array_equal(_host(ra[0]), _host(ro[0])) and ra[2] == ro[2]
        assert np.array_equal(_host(J.krr_predict(a, Xn, lb=[1e-1, 1e-2])[0]), _host(J.krr_predict(other, xn, lb=[1e-1, 1e-2])[0]))


# ---------------------------------------------------------------------------------- gridscorelb, krrda
def test_gridscorelb_and_krrda_against_the_restatement(J):
    n, p, q = 400, 9, 2
    X = _data(n, p, 21); Xt = _data(120, p, 22)
    rng = np.random.default_rng(23)
    Y = np.asfortranarray(X[:, :q] ** 2 + 0.05 * rng.standard_normal((n, q))); Yt = np.asfortranarray(Xt[:, :q] ** 2)
    lbs = [1e-1, 1e-3, 1e-2, 1e-1]                                       # mlev: sorted distinct values
    want_lb = [1e-3, 1e-2, 1e-1]

    def ref_rmsep(gamma):
        ref = np_krr(X, Y, lb=max(lbs), gamma=gamma)
        return np.vstack([np.sqrt(np.mean((pr - Yt) ** 2, axis=0)) for pr in np_krr_predict(ref, Xt, want_lb)])

    res = J.gridscorelb(X, Y, Xt, Yt, score=J.rmsep, fun=J.krr, lb=lbs, gamma=0.5)
    assert list(res) == ["lb", "res"] and res["lb"] == want_lb
    assert np.allclose(res["res"], ref_rmsep(0.5), rtol=1e-8)
    pars = J.mpar(gamma=[0.2, 0.5])
    res = J.gridscorelb(X, Y, Xt, Yt, score=J.rmsep, fun=J.krr, lb=lbs, pars=pars)
    assert res["lb"] == want_lb * 2 and res["gamma"] == [0.2] * 3 + [0.5] * 3
    assert np.allclose(res["res"], np.vstack([ref_rmsep(0.2), ref_rmsep(0.5)]), rtol=1e-8)
    custom = J.gridscorelb(X, Y, Xt, Yt, score=lambda pr, y: np.sqrt(np.mean((_host(pr) - y) ** 2, axis=0)), fun=J.krr, lb=lbs, pars=pars)
    assert np.allclose(custom["res"], res["res"], rtol=1e-10)
    # krrda: labels from three clusters of the latent profile
    y = np.array(["a", "b", "c"])[np.argmax(X[:, [1, 4, 7]], axis=1)]
    obj = J.krrda(X, y, lb=1e-2, gamma=0.5)
    assert list(obj.lev) == ["a", "b", "c"] and list(obj.ni) == [int((y == l).sum()) for l in "abc"]
    Yd = (y[:, None] == np.array(["a", "b", "c"])[None, :]).astype(float)
    ref = np_krr(X, Yd, lb=1e-2, gamma=0.5)
    for lb in (None, [1e-1, 1e-2]):
        pred, post = J.krrda_predict(obj, Xt, lb=lb)
        rpost = np_krr_predict(ref, Xt, lb)
        if lb is None:
            pred, post, rpost = [pred], [post], [rpost]
        for pr, po, rp in zip(pred, post, rpost):
            assert np.allclose(_host(po), rp, rtol=1e-7, atol=1e-9)
            assert np.array_equal(pr.ravel(), np.array(["a", "b", "c"])[np.argmax(rp, axis=1)])


# ---------------------------------------------------------------------------------- at size
def test_full_size_against_scipy_cholesky(J):
    """n = 16 384: Kd from the restatement's steps without its SVD, the CPU solve by scipy's Cholesky.  krbf has trace(Kd) = sum_i w_i
    Kc_ii <= 1, so with lb = 1e-2 cond <= 1e4 + 1: A and the predictions within 50 eps cond, df within 10 n eps cond absolute, the
    residual within the backward-error bound 3 n eps |M|_F |A|_F of a Cholesky solve (Higham thm 10.4, gamma_{3n+1})."""
    from scipy.linalg import cho_factor, cho_solve
    from scipy.linalg.lapack import dtrtri
    n, p, q, lb = 16384, 64, 2, 1e-2
    X = _data(n, p, 31)
    Y = np.asfortranarray(X[:, [3, 40]] ** 2 + 0.05 * np.random.default_rng(32).standard_normal((n, q)))
    Xn = _data(1000, p, 33)
    gamma = 1.0 / p
    ref = np_krr(X, Y, lb=lb, svd=False, gamma=gamma)
    fm = J.krr(X, Y, lb=lb, gamma=gamma)
    A, _, df = J.krr_coef(fm)
    A = _host(A)
    pred = _host(J.krr_predict(fm, Xn))
    M = ref["Kd"]
    M[np.diag_indices(n)] += lb ** 2
    cond = 1e4 + 1
    res = M @ A - ref["DY"]
    r_bound = 3 * n * EPS * np.linalg.norm(M) * np.linalg.norm(A)
    print(f"residual {np.linalg.norm(res):.3e} bound {r_bound:.3e}")
    assert np.linalg.norm(res) <= r_bound
    c = cho_factor(M, lower=True, overwrite_a=True)
    Aref = cho_solve(c, ref["DY"])
    from test_krr_static import np_krr_centred_new
    pref = np_krr_centred_new(ref, Xn) @ (ref["sqrtD"][:, None] * Aref)
    Li, info = dtrtri(c[0], lower=1, overwrite_c=1)
    assert info == 0
    dref = 1.0 + n - lb ** 2 * float(np.sum(np.tril(Li) ** 2))
    e_A, e_p, e_df = _rel(A, Aref), _rel(pred - ref["ymeans"], pref), abs(df - dref)
    print(f"A {e_A:.3e} pred {e_p:.3e} (50 eps cond = {50 * EPS * cond:.3e}); df = {dref:.6f}, gpu off by {e_df:.3e} (10 n eps cond = {10 * n * EPS * cond:.3e})")
    assert e_A <= 50 * EPS * cond and e_p <= 50 * EPS * cond and e_df <= 10 * n * EPS * cond


# ---------------------------------------------------------------------------------- the three routes of the C entries (tests/host_routes.py)
@pytest.mark.parametrize("entry", sorted(__import__("host_routes").ROUTES["krr"]))
def test_host_arrays_padded_and_unpadded_give_the_bits_of_the_device_route(entry):
    """Device buffers, host arrays with ld == rows and with ld = rows + 3 between NaN guards: equal bytes, NaN padding kept, inputs unchanged."""
    import host_routes as HR
    HR.three_routes(HR.ROUTES["krr"][entry])
