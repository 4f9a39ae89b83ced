"""jch_xtdx, pcasvd / pcaeigen / pcaeigenk and pcr on the GPU: the Gram kernel through the C ABI against the extended-precision restatement
under the static bound (test_pca_static.gram_bound), the fits against the literal numpy restatements of src/pcasvd.jl and src/pcr.jl."""
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

from test_pca_static import (_data, _weights, gram_bound, gram_longdouble, np_pca_summary, np_pca_transform, np_pcasvd, np_pcr,  # noqa: E402
                             np_pcr_coef, np_pcr_predict)

TOL = 1e-10   # the default eig_tol


@pytest.fixture(scope="module")
def J():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import jchemo_hip
    return jchemo_hip


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


# ---------------------------------------------------------------------------------- jch_xtdx through the C ABI
def _dev_colmajor(X, ldx, offset):
    """A device copy of X with leading dimension ldx whose first element sits `offset` doubles behind an allocation's start."""
    n, p = X.shape
    buf = torch.full((offset + ldx * p,), 7.0, dtype=torch.float64, device="cuda:0")
    V = buf[offset:].view(p, ldx).t()
    V[:n].copy_(torch.as_tensor(np.array(X), device="cuda:0"))
    return buf, V, buf.data_ptr() + 8 * offset


def _xtdx(J, ctx, loc, xaddr, n, p, ldx, waddr, ldg=None):
    """(G, mu) as host arrays: through G_host / mu_host when ldg is None, else read back from a device G with that leading dimension."""
    lib = J.load()
    mu = np.full(p, np.nan)
    if ldg is None:
        G = np.full((p, p), np.nan, order="F")
        ctx.check(lib.jch_xtdx(ctx._h, loc, xaddr, n, p, ldx, waddr, None, 0, None, G.ctypes.data, mu.ctypes.data))
        return G, mu
    Gd = torch.full((p, ldg), -3.0, dtype=torch.float64, device="cuda:0")   # row k of the tensor = column k of G
    mud = torch.empty(p, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.check(lib.jch_xtdx(ctx._h, loc, xaddr, n, p, ldx, waddr, Gd.data_ptr(), ldg, mud.data_ptr(), None, None))
    assert torch.all(Gd[:, p:] == -3.0)                                      # nothing behind the p rows of a column is written
    return _host(Gd[:, :p].t()), _host(mud)


# the smallest shapes at which the kernel can go wrong: one entry; one column; one ragged block; exactly one block; one column into a second
# block; three blocks (off-diagonal tile pairs, ragged last block); n = 4 * 16 + 1 (one row into a chunk); n = 1000 with p = 40 (62 row splits of
# 32 rows leave a last split of 8 rows, shorter than a chunk; (300, 128) ends on a split of 12 rows too)
XT_SHAPES = [(1, 1), (33, 1), (5, 127), (300, 128), (300, 129), (70, 257), (65, 20), (1000, 40)]


@pytest.mark.parametrize("wkind", ["ones", "rand", "zeros"])
@pytest.mark.parametrize("n,p", XT_SHAPES)
def test_xtdx_against_the_longdouble_restatement(J, n, p, wkind):
    ctx = J.Context(0)
    X = _data(n, p, 3 * n + p)
    X0 = X.copy()
    w = _weights(wkind, n)
    Gl, mul = gram_longdouble(X, w)
    bG, bmu = gram_bound(X, w)
    wa = None if w is None else w.ctypes.data
    wd = None if w is None else torch.as_tensor(w, device="cuda:0")
    wda = None if w is None else wd.data_ptr()
    G, mu = _xtdx(J, ctx, 0, X.ctypes.data, n, p, n, wa)                                    # host X
    assert np.array_equal(X, X0)
    errG = np.abs(np.asarray(G - Gl, dtype=np.float64))
    print(f"xtdx n={n} p={p} {wkind}: max err / bound = {float(np.max(errG / bG)):.3g} (mu: {float(np.max(np.abs(mu - np.asarray(mul, dtype=np.float64)) / bmu)):.3g})")
    assert np.all(np.abs(mu - np.asarray(mul, dtype=np.float64)) <= bmu)
    assert np.all(errG <= bG)
    assert np.array_equal(G, G.T)                                                           # G == G' bitwise
    ldx = n + 2 + (n % 2)                                                                   # even and > n: the 16-byte loads
    _, Va, aa = _dev_colmajor(X, ldx, 0)
    _, Vu, au = _dev_colmajor(X, n + 3, 1)                                                  # base one double off: the 8-byte loads
    torch.cuda.synchronize()
    runs = [_xtdx(J, ctx, 0, X.ctypes.data, n, p, n, wa), _xtdx(J, ctx, 1, aa, n, p, ldx, wda), _xtdx(J, ctx, 1, aa, n, p, ldx, wda, ldg=p + 3),
            _xtdx(J, ctx, 1, au, n, p, n + 3, wda), _xtdx(J, ctx, 1, au, n, p, n + 3, wda, ldg=p)]
    for G2, mu2 in runs:                                                                    # a second run, host / device, aligned / unaligned
        assert np.array_equal(G2, G) and np.array_equal(mu2, mu)
    assert np.array_equal(_host(Va[:n]), X0) and np.array_equal(_host(Vu[:n]), X0)          # X is only read
    assert torch.all(Va[n:] == 7.0) and torch.all(Vu[n:] == 7.0)
    ctx.close()


def test_xtdx_one_nan_stays_in_its_row_and_column(J):
    ctx = J.Context(0)
    n, p, j = 70, 257, 130
    X = _data(n, p, 5)
    G0, _ = _xtdx(J, ctx, 0, X.ctypes.data, n, p, n, None)
    X[41, j] = np.nan
    G, mu = _xtdx(J, ctx, 0, X.ctypes.data, n, p, n, None)
    keep = np.ones(p, dtype=bool); keep[j] = False
    assert np.all(np.isnan(G[j, :])) and np.all(np.isnan(G[:, j])) and np.isnan(mu[j])
    assert np.array_equal(G[np.ix_(keep, keep)], G0[np.ix_(keep, keep)]) and np.all(np.isfinite(mu[keep]))
    ctx.close()


# ---------------------------------------------------------------------------------- the fits
def _gaps(eig, k):
    g = np.empty(k)
    for i in range(k):
        others = np.delete(eig, i)
        g[i] = np.min(np.abs(others - eig[i])) if others.size else np.inf   # (p = 1: the one vector is +-1)
    return g


def _col_bounds(eig, nlv, tol=TOL):
    """10 tol eig_1 / gap_i: how far an eigenvector whose residual is tol eig_1 may be from the true one."""
    return 10 * tol * eig[0] / _gaps(eig, nlv)


def _compare_columns(A, B, eig, cols, scale, tol=TOL):
    """Columns `cols` of A and B (sign-aligned) within 10 tol eig_1 / gap_i, relative to `scale`.  Every compared column must take this per-column
    branch (bound < 1e-3): none falls back to a subspace comparison."""
    cb = _col_bounds(eig, max(cols) + 1, tol)
    for i in cols:
        assert cb[i] < 1e-3, (i, cb[i])
        a, b = A[:, i], B[:, i]
        s = 1.0 if a @ b >= 0 else -1.0
        err = np.linalg.norm(a - s * b)
        assert err <= max(cb[i], 1e-11) * scale[i] + 1e-13 * np.linalg.norm(b), (i, err / scale[i], cb[i])


def _new_rows(X, m=50, seed=77):
    rng = np.random.default_rng(seed)
    i, k = rng.integers(0, X.shape[0], m), rng.integers(0, X.shape[0], m)
    return np.asfortranarray(0.5 * (X[i] + X[k]) + 0.01 * rng.standard_normal((m, X.shape[1])))


PCA_CASES = [(150, 40, 3, "ones", False), (400, 129, 10, "rand", True), (777, 257, 25, "zeros", False), (64, 300, 10, "rand", False),
             (2000, 500, 25, "rand", True), (1001, 17, 17, "zeros", False), (33, 1, 1, "ones", False)]
_REF = {}


def _ref(case):
    """The restatement of a case, computed once and shared."""
    if case not in _REF:
        n, p, nlv, wkind, scal = case
        X = _data(n, p, n + p)
        X.setflags(write=False)
        w = _weights(wkind, n)
        _REF[case] = (X, w, np_pcasvd(X, w, nlv=nlv, scal=scal))
    return _REF[case]


@pytest.mark.parametrize("case", PCA_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_pcasvd_parity_with_the_restatement(J, case):
    n, p, nlv, wkind, scal = case
    X, w, ref = _ref(case)
    X0 = X.copy()
    fm = J.pcasvd(X, w, nlv=nlv, scal=scal)
    assert np.array_equal(X, X0)
    assert fm.converged and fm.conv and fm.niter >= 1
    if nlv == p:
        assert fm.niter == 1                                  # b == p: one Rayleigh-Ritz step is exact
    eig = ref["sv"] ** 2
    e1 = eig[0]
    print(f"pcasvd {case}: niter={fm.niter} max|eig err|/eig1={float(np.max(np.abs(fm.eig - eig[:nlv])) / e1):.3g} max resid/eig1={float(fm.resid.max() / e1):.3g}")
    assert fm.eig.shape == (nlv,) and fm.sv.shape == (nlv,)
    assert np.max(np.abs(fm.eig - eig[:nlv])) <= 1e-10 * e1
    assert np.max(np.abs(fm.sv ** 2 - eig[:nlv])) <= 1e-10 * e1
    assert np.isclose(fm.sstot, eig.sum(), rtol=1e-12)
    assert np.allclose(fm.xmeans, ref["xmeans"], rtol=1e-12, atol=0)
    assert np.allclose(fm.xscales, ref["xscales"], rtol=1e-12, atol=0)
    assert np.allclose(_host(fm.weights), ref["weights"], rtol=1e-13, atol=0)
    assert np.allclose(fm.colvar, ref["weights"] @ (X - ref["xmeans"]) ** 2, rtol=1e-12, atol=0)
    P, T = fm.P, _host(fm.T)
    for i in range(nlv):                                      # sign rule: the largest-|.| entry of every P column is positive
        assert P[np.argmax(np.abs(P[:, i])), i] > 0
    eig_pad = np.r_[eig, np.zeros(max(0, p - eig.size))]      # (n < p: the p - n further eigenvalues of G are zero)
    cols = list(range(nlv))
    cb = _col_bounds(eig_pad, nlv)
    print(f"   largest column bound {float(cb.max()):.3g}")
    tn = np.linalg.norm(ref["T"], axis=0)
    _compare_columns(P, ref["P"], eig_pad, cols, np.ones(nlv))
    _compare_columns(T, ref["T"], eig_pad, cols, tn)         # T within the same bound, relative to the reference column's norm
    sg = np.sign(np.sum(P * ref["P"], axis=0))
    sg[sg == 0] = 1.0
    print("   max |dT_i| / (bound_i |T_i|) = %.3g" % max(np.linalg.norm(T[:, i] - sg[i] * ref["T"][:, i]) / (max(cb[i], 1e-11) * tn[i]) for i in cols))
    # transform on 50 new rows: rtol 1e-9, or the column's bound where that is larger, relative to the reference column's norm
    Xn = _new_rows(X)
    Tn, Tr = _host(J.transform(fm, Xn)), np_pca_transform(ref, Xn) * sg
    rat = [np.linalg.norm(Tn[:, i] - Tr[:, i]) / (max(1e-9, cb[i]) * max(np.linalg.norm(Tr[:, i]), 1e-300) + 1e-12) for i in cols]
    print(f"   transform: max |dT_i| / tol_i = {max(rat):.3g}")
    assert max(rat) <= 1.0, rat
    assert _host(J.transform(fm, Xn, nlv=1)).shape == (50, 1)
    # every table of summary against the restatement.  What depends on the eigenvalues only (explvarx): rtol 1e-9, atol 1e-12 in the table's units
    # (eig_1 for var), as the kpca test does.  What is a linear image of P (coord_var = P diag(sv), cor_circle = coord_var ./ colstd) cannot be
    # closer to the restatement than P is: a vector with residual eig_tol eig_1 is determined to eig_tol eig_1 / gap_i.  Those tables are held
    # column by column to max(1e-9, bound_i) relative to the reference column's norm, cor_circle after multiplying both sides by the reference's
    # colstd (a row scaling common to both).  The squared tables (contr_var = P.^2, contr_ind = D T.^2 ./ tt, columns of 1-norm 1) to twice that
    # in the 1-norm: d(x^2) = 2 x dx and Cauchy-Schwarz.  (An elementwise rtol of 1e-9 on these tables is out of reach for any solver stopped at
    # eig_tol = 1e-10: numpy's own subspace iteration on G misses it by factors of 2.7, 1.4, 52 and 86 on the first, second, third and fifth
    # case, in the trailing columns where gap_i / eig_1 is 1e-4, while it meets the column bound with a ratio of 0.006 at the most.)
    sm, smr = J.summary(fm, X), np_pca_summary(ref, X)
    ex, exr = sm["explvarx"], smr["explvarx"]
    assert np.array_equal(ex["lv"], exr["lv"])
    for nm, unit in (("var", e1), ("pvar", 1.0), ("cumpvar", 1.0)):
        assert np.allclose(ex[nm], exr[nm], rtol=1e-9, atol=1e-12 * unit), nm
    std = np.sqrt(ref["weights"] @ ref["Xs"] ** 2)[:, None]
    cbr = np.maximum(1e-9, cb)
    cvn = np.linalg.norm(smr["coord_var"], axis=0)
    rat = dict(coord_var=np.linalg.norm(sm["coord_var"] - smr["coord_var"] * sg, axis=0) / (cbr * cvn),
               cor_circle=np.linalg.norm(std * (sm["cor_circle"] - smr["cor_circle"] * sg), axis=0) / (cbr * cvn),
               contr_var=np.sum(np.abs(sm["contr_var"] - smr["contr_var"]), axis=0) / (2 * cbr),
               contr_ind=np.sum(np.abs(_host(sm["contr_ind"]) - smr["contr_ind"]), axis=0) / (2 * cbr))
    print("   summary, max error / bound: " + ", ".join(f"{k} {float(v.max()):.3g}" for k, v in rat.items()))
    for nm, v in rat.items():
        assert sm[nm].shape == smr[nm].shape and np.all(v <= 1.0), (nm, v)
    with pytest.raises(ValueError):
        J.summary(fm, X[:-1] if n > 1 else np.zeros((2, p)))


def test_aliases_return_the_same_bits_and_nlv_is_clamped(J):
    X, w, _ = _ref(PCA_CASES[1])
    a = J.pcasvd(X, w, nlv=10, scal=True)
    for fn in (J.pcaeigen, J.pcaeigenk, J.pcasvd_, J.pcaeigen_, J.pcaeigenk_):
        b = fn(X, w, nlv=10, scal=True)
        for f in ("T", "P", "sv", "eig", "xmeans", "xscales", "weights", "colvar", "resid"):
            assert np.array_equal(_host(getattr(a, f)), _host(getattr(b, f))), (fn.__name__, f)
        assert (a.sstot, a.niter, a.converged) == (b.sstot, b.niter, b.converged)
    # nlv > min(n, p) clamps; n <= p and nlv = n: the last eigenvalue of the centred data is zero and its vector arbitrary, in the reference too
    n, p = 20, 31
    X = _data(n, p, 4)
    ref = np_pcasvd(X, nlv=n)
    fm = J.pcasvd(X, nlv=n + 50)
    assert fm.T.shape == (n, n) and fm.P.shape == (p, n) and fm.eig.shape == (n,)
    eig = np.r_[ref["sv"] ** 2, np.zeros(p - n)]
    assert np.max(np.abs(fm.eig - eig[:n])) <= 1e-10 * eig[0]
    cols = [i for i in range(n) if eig[i] > 1e-12 * eig[0]]
    assert len(cols) >= n - 1
    _compare_columns(fm.P, ref["P"], eig, cols, np.ones(n))
    fm2 = J.pcasvd(_data(30, 8, 6), nlv=100)                               # p < n: clamps to p, the b == p path
    assert fm2.P.shape == (8, 8) and fm2.niter == 1 and fm2.converged


@pytest.mark.parametrize("q", [1, 3])
def test_pcr_coef_and_predict(J, q):
    n, p, a = 400, 129, 10
    X, w, _ = _ref(PCA_CASES[1])
    rng = np.random.default_rng(21)
    Y = np.asfortranarray((X - X.mean(axis=0))[:, :q] * 2.0 + (X - X.mean(axis=0))[:, 40:40 + q] + 5.0 + 0.05 * rng.standard_normal((n, q)))
    ref = np_pcr(X, Y, w, nlv=a, scal=True)
    X0, Y0 = X.copy(), Y.copy()
    fm = J.pcr(X, Y, w, nlv=a, scal=True)
    assert np.array_equal(X, X0) and np.array_equal(Y, Y0)
    assert fm.fm_pca.converged and fm.R is fm.fm_pca.P and np.array_equal(fm.yscales, np.ones(q))
    assert np.allclose(fm.ymeans, ref["ymeans"], rtol=1e-12)
    eig = ref["fm_pca"]["sv"] ** 2
    cb = _col_bounds(np.r_[eig, np.zeros(max(0, p - eig.size))], a)
    B0, i0 = J.coef(fm, nlv=0)
    assert np.all(B0 == 0) and np.allclose(i0, ref["ymeans"][None, :], rtol=1e-12)          # nlv = 0: intercept only
    beta = np.abs(ref["C"].T)                                                                # a x q
    Xn = _new_rows(X)
    xs = ref["xscales"]
    XnF = np.linalg.norm((Xn - ref["xmeans"]) / xs)                                          # pred = ymeans + ((X - xmeans) / xscales)(xscales o B)
    for k in (1, a):
        B, b0 = J.coef(fm, nlv=k)
        Br, b0r = np_pcr_coef(ref, k)
        # the column bound carried through xscales o B = P beta: sum_i bound_i |beta_i| (|p_i| = 1), floor 1e-9 relative
        tolB = np.maximum((cb[:k, None] * beta[:k]).sum(axis=0), 1e-9 * np.linalg.norm(xs[:, None] * Br, axis=0))
        dB = np.linalg.norm(xs[:, None] * (B - Br), axis=0)
        print(f"pcr q={q} nlv={k}: |xscales o dB| / tol = {(dB / tolB).max():.3g}")
        assert np.all(dB <= tolB)
        assert np.all(np.abs(b0 - b0r) <= tolB * np.linalg.norm(ref["xmeans"] / xs) + 1e-12 * np.abs(b0r))   # int = ymeans - (xmeans / xscales)'(xscales o B)
        pr, prr = _host(J.predict(fm, Xn, nlv=k)), np_pcr_predict(ref, Xn, k)
        assert pr.shape == (50, q)
        assert np.all(np.linalg.norm(pr - prr, axis=0) <= tolB * XnF + 1e-12 * np.linalg.norm(prr, axis=0))
    preds = J.predict(fm, Xn, nlv=range(0, a + 1))
    assert len(preds) == a + 1
    for k, pr in enumerate(preds):
        prr = np_pcr_predict(ref, Xn, k)
        tolB = np.maximum((cb[:k, None] * beta[:k]).sum(axis=0), 1e-9 * np.linalg.norm(xs[:, None] * np_pcr_coef(ref, k)[0], axis=0))
        assert np.all(np.linalg.norm(_host(pr) - prr, axis=0) <= tolB * XnF + 1e-12 * np.linalg.norm(prr, axis=0)), k
    assert np.array_equal(_host(J.transform(fm, Xn)), _host(J.transform(fm.fm_pca, Xn)))   # transform(::Pcr) is the Plsr path with R = P


def test_gridscorelv_with_pcr(J):
    n, p, a, q = 400, 129, 8, 2
    X, w, _ = _ref(PCA_CASES[1])
    rng = np.random.default_rng(22)
    Xc = X - X.mean(axis=0)
    Y = np.asfortranarray(Xc[:, :q] * 2.0 + Xc[:, 60:60 + q] + 0.05 * rng.standard_normal((n, q)))
    Xv = _new_rows(X, 60, 5)
    Yv = np.asfortranarray((Xv - X.mean(axis=0))[:, :q] * 2.0 + (Xv - X.mean(axis=0))[:, 60:60 + q] + 0.05 * rng.standard_normal((60, q)))
    res = J.gridscorelv(X, Y, Xv, Yv, score=J.rmsep, fun=J.pcr, nlv=range(0, a + 1))
    ref = np_pcr(X, Y, nlv=a)
    want = np.vstack([np.sqrt(np.mean((np_pcr_predict(ref, Xv, k) - Yv) ** 2, axis=0)) for k in range(a + 1)])
    got = np.asarray(res["res"])
    assert list(res["nlv"]) == list(range(a + 1)) and got.shape == want.shape
    # rmsep is 1-Lipschitz in pred / sqrt(m): the prediction bound of test_pcr_coef_and_predict carries over
    eig = ref["fm_pca"]["sv"] ** 2
    cb = _col_bounds(np.r_[eig, np.zeros(max(0, p - eig.size))], a)
    beta = np.abs(ref["C"].T)
    for k in range(a + 1):
        tolB = np.maximum((cb[:k, None] * beta[:k]).sum(axis=0), 1e-9 * np.linalg.norm(np_pcr_coef(ref, k)[0], axis=0))
        assert np.all(np.abs(got[k] - want[k]) <= tolB * np.linalg.norm(Xv - ref["xmeans"]) / np.sqrt(60) + 1e-12 * want[k]), k


def test_device_in_device_out(J):
    X, w, ref = _ref(PCA_CASES[0])
    n, p = X.shape
    Xd = J.colmajor_empty(n, p)
    Xd.copy_(torch.as_tensor(np.array(X), device="cuda:0"))
    fm = J.pcasvd(Xd, nlv=3)
    host = J.pcasvd(X, nlv=3)
    assert isinstance(fm.T, torch.Tensor) and fm.T.is_cuda and isinstance(fm.weights, torch.Tensor) and fm.weights.is_cuda
    assert np.array_equal(_host(fm.T), host.T) and np.array_equal(fm.P, host.P)               # host and device X: the same bits
    assert np.array_equal(_host(Xd), X)
    assert isinstance(J.summary(fm, Xd)["contr_ind"], torch.Tensor)
    Tn = J.transform(fm, Xd[:20])
    assert isinstance(Tn, torch.Tensor) and Tn.is_cuda
    rng = np.random.default_rng(1)
    Y = torch.as_tensor(np.asfortranarray(host.T @ rng.standard_normal((3, 2)) + 0.01 * rng.standard_normal((n, 2))), device="cuda:0")
    Yd = J.colmajor_empty(n, 2); Yd.copy_(Y)
    pls = J.plskern(fm.T, Yd, nlv=2)                                                          # straight into a PLS fit, no host trip
    assert isinstance(pls.T, torch.Tensor) and pls.T.is_cuda and pls.T.shape == (n, 2)
    fmr = J.pcr(Xd, Yd, nlv=3)
    pr = J.predict(fmr, Xd[:20])
    assert isinstance(pr, torch.Tensor) and pr.is_cuda and pr.shape == (20, 2)


def test_pure_noise_does_not_converge_and_says_so(J):
    X = np.asfortranarray(np.random.default_rng(3).random((300, 200)))
    with pytest.warns(RuntimeWarning, match="did not converge"):
        fm = J.pcasvd(X, nlv=5, eig_maxit=3)
    assert not fm.converged and fm.niter == 3 and np.all(np.isfinite(fm.eig))


def test_errors(J):
    from jchemo_hip._lib import JCH_EINVAL, JchError
    X = _data(30, 6, 1)
    with pytest.raises(ValueError, match="nlv"):
        J.pcasvd(X, nlv=0)
    with pytest.raises(ValueError, match="eig_tol"):
        J.pcasvd(X, nlv=2, eig_tol=0.0)
    fm = J.pcasvd(X, nlv=2)
    with pytest.raises(ValueError, match="DimensionMismatch"):
        J.transform(fm, X[:, :5])
    lib = J.load()
    ctx = J.Context(0)
    G = np.empty((6, 6), order="F")
    for args, msg in (((0, X.ctypes.data, 30, 6, 29, None, None, 0, None, G.ctypes.data, None), "bad X"),
                      ((0, X.ctypes.data, 30, 40000, 30, None, None, 0, None, G.ctypes.data, None), "beyond 32768")):
        st = lib.jch_xtdx(ctx._h, *args)
        assert st == JCH_EINVAL and msg in lib.jch_last_error(ctx._h).decode()
    st = lib.jch_pca_fit(ctx._h, 0, X.ctypes.data, 30, 6, 30, None, None, 0, 0, 0, 0, 1e-10, 300, *([None] * 11), None, None, None, None)
    assert st == JCH_EINVAL and "nlv" in lib.jch_last_error(ctx._h).decode()
    st = lib.jch_pca_fit(ctx._h, 0, X.ctypes.data, 30, 6, 30, None, None, 0, 0, 2, 0, 0.0, 300, *([None] * 11), None, None, None, None)
    assert st == JCH_EINVAL and "tol" in lib.jch_last_error(ctx._h).decode()
    ctx.close()
    # a communicator of two ranks: one rank only, as for covsel
    grp = C.c_void_p()
    assert lib.jch_loopback_group_create(2, C.byref(grp)) == 0
    c = J.Context(0)
    try:
        c.comm_init_loopback(grp, 0, 2)
        with pytest.raises(JchError, match="one rank only") as ei:
            J.pcasvd(X, nlv=2, ctx=c)
        assert ei.value.code == JCH_EINVAL
        with pytest.raises(JchError, match="one rank only"):
            J.pcr(X, X[:, :1].copy(), nlv=2, ctx=c)
    finally:
        c.close()
        lib.jch_loopback_group_destroy(grp)


# ---------------------------------------------------------------------------------- the three routes of the C entries (tests/host_routes.py)
@pytest.mark.parametrize("entry", sorted(__import__("host_routes").ROUTES["pca"]))
def test_host_arrays_padded_and_unpadded_give_the_bits_of_the_device_route(entry):
    """Device buffers, host arrays with ld == rows and with ld = rows + 3 between NaN guards: equal bytes, NaN padding kept, inputs unchanged."""
    import host_routes as HR
    HR.three_routes(HR.ROUTES["pca"][entry])
