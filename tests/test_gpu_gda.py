"""GPU checks of the Gaussian discrimination family (jch_class_cov, jch_gauss_factor, jch_mahsq_chol; dmnorm, lda, qda, matW, matB, mahsqchol of
jchemo_hip/gda.py) against the longdouble restatements and the error bounds of tests/test_gda_static.py.  Every comparison prints its largest
measured / allowed ratio before it asserts.

Measured on an MI355X, largest measured / allowed: jch_mahsq_chol 0.125, jch_class_cov 0.106 (Wi) / 0.096 (W) / 0.113 (means), jch_gauss_factor 0.011
(Uinv) / 0.007 (diag L) of 50 eps cond2, lda / qda 0.045 (d2) / 0.011 (dens) / 0.004 (posterior), dmnorm 0.059, mahsqchol at (400, 130, 2) 0.00012
(DESIGN.md §24)."""
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

from test_gda_static import (BIG_SHAPE, EPS, LD, MODEL_SHAPES, PRIM_M, PRIM_P, assert_model, chol_uinv, class_cov_reference, cond2,  # noqa: E402
                             factor_tol, gauss_classes, model_case, np_cov, np_dmnorm, np_dmnorm_predict, np_mahsqchol, np_matB, one_row_classes,
                             prim_case, ratio)

SENT = 7.0


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


@pytest.fixture(scope="module")
def used_ctx(J):
    """A ctx that a plskern fit and a krr fit (with its df pass: chol_inv, chol_w) have used."""
    c = J.Context(0)
    rng = np.random.default_rng(5)
    X, Y = np.asfortranarray(rng.normal(size=(200, 30))), np.asfortranarray(rng.normal(size=(200, 2)))
    J.plskern(X, Y, nlv=4, ctx=c)
    J.krr_coef(J.krr(X, Y, lb=0.1, ctx=c), ctx=c)
    yield c
    c.close()


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _dev(a):
    a = np.asarray(a, dtype=np.float64)
    t = torch.empty(a.shape[::-1], dtype=torch.float64, device="cuda:0").t() if a.ndim == 2 else torch.empty(a.shape, dtype=torch.float64, device="cuda:0")
    t.copy_(torch.from_numpy(np.array(a, order="C")))
    return t


def _dev_colmajor(A, ld, offset, tail=0):
    """A device copy of A (column-major, leading dimension ld) whose first element sits `offset` doubles behind an allocation's start; sentinels
    everywhere else.  Returns (buffer, address of A[0, 0])."""
    n, c = A.shape
    buf = torch.full((offset + ld * c + 1 + tail,), SENT, dtype=torch.float64, device="cuda:0")
    V = buf[offset:offset + ld * c].view(c, ld).t()
    V[:n].copy_(torch.as_tensor(np.array(A), device="cuda:0"))
    return buf, buf.data_ptr() + 8 * offset


def _body(buf, ld, cols, offset, rows):
    """(the rows x cols matrix, True if every sentinel around it survived) of a buffer made by _dev_colmajor."""
    O = _host(buf)
    body = O[offset:offset + ld * cols].reshape(cols, ld)
    ok = np.all(O[:offset] == SENT) and np.all(O[offset + ld * cols:] == SENT) and np.all(body[:, rows:] == SENT)
    return body[:, :rows].T.copy(), bool(ok)


# ---------------------------------------------------------------------------------- a. jch_mahsq_chol through the C ABI
def mahsq_device(J, ctx, Xq, Mu, Us, nfac, pad, offset):
    """Device call with ld = rows + pad at `offset` doubles into every allocation; checks the sentinels; returns out (m x ncen)."""
    m, p = Xq.shape
    ncen = Mu.shape[0]
    qb, qa = _dev_colmajor(Xq, m + pad, offset)
    ldu = p + pad
    stride = ldu * p + 3
    ub = torch.full((offset + stride * nfac + 1,), SENT, dtype=torch.float64, device="cuda:0")
    for f in range(nfac):
        ub[offset + f * stride:offset + f * stride + ldu * p].view(p, ldu).t()[:p].copy_(torch.as_tensor(np.array(Us[f]), device="cuda:0"))
    ob, oa = _dev_colmajor(np.full((m, ncen), SENT), m + pad, offset)
    Muf = np.asfortranarray(Mu)
    torch.cuda.synchronize()
    ctx.check(J.load().jch_mahsq_chol(ctx._h, J._lib.LOC_DEVICE, qa, m, p, m + pad, Muf.ctypes.data, ncen, ub.data_ptr() + 8 * offset, ldu, stride, nfac, oa,
                                      m + pad))
    out, ok = _body(ob, m + pad, ncen, offset, m)
    assert ok, "a sentinel around `out` was overwritten"
    assert _body(qb, m + pad, p, offset, m)[1], "Xq was written"
    return out


def mahsq_host(J, ctx, Xq, Mu, Us, nfac):
    m, p = Xq.shape
    ncen = Mu.shape[0]
    Xf, Muf = np.asfortranarray(Xq), np.asfortranarray(Mu)
    Uf = np.ascontiguousarray(np.transpose(np.asarray(Us[:nfac]), (0, 2, 1)))      # slice f column-major
    out = np.full((ncen, m), SENT)
    ctx.check(J.load().jch_mahsq_chol(ctx._h, J._lib.LOC_HOST, Xf.ctypes.data, m, p, m, Muf.ctypes.data, ncen, Uf.ctypes.data, p, p * p, nfac,
                                      out.ctypes.data, m))
    return out.T.copy()


@pytest.mark.parametrize("p", PRIM_P)
@pytest.mark.parametrize("m", PRIM_M)
def test_mahsq_against_longdouble_and_bitwise(J, ctx, m, p):
    worst = 0.0
    for ncen, nfac in ((1, 1), (3, 1), (3, 3)):
        Xq, Mu, Us, d2, bound = prim_case(m, p, ncen, nfac)
        got = mahsq_device(J, ctx, Xq, Mu, Us, nfac, 0, 0)                         # aligned, ld = rows
        r = ratio(got, d2, bound)
        worst = max(worst, r)
        print(f"m={m} p={p} ncen={ncen} nfac={nfac}: device against longdouble, largest measured / allowed = {r:.3f}")
        assert r <= 1.0
        assert np.array_equal(got, mahsq_device(J, ctx, Xq, Mu, Us, nfac, 0, 0)), "two calls differ in their bits"
        assert np.array_equal(got, mahsq_device(J, ctx, Xq, Mu, Us, nfac, 3, 1)), "odd offset / odd ld differs from the aligned call"
        assert np.array_equal(got, mahsq_host(J, ctx, Xq, Mu, Us, nfac)), "loc = host differs from loc = device"
        Un = np.array(Us)
        Un[:, np.tril_indices(p, -1)[0], np.tril_indices(p, -1)[1]] = np.nan
        assert np.array_equal(got, mahsq_device(J, ctx, Xq, Mu, Un, nfac, 3, 1)), "the strictly lower triangle of Uinv reached the result"
    print(f"m={m} p={p}: worst ratio {worst:.3f}")


@pytest.mark.parametrize("m,p", [(129, 17), (257, 260)])
def test_mahsq_nan_stays_in_its_row(J, ctx, m, p):
    Xq, Mu, Us, _, _ = prim_case(m, p, 3, 3)
    Xn = np.array(Xq)
    i, k = m // 2, p // 3
    Xn[i, k] = np.nan
    clean, got = mahsq_device(J, ctx, Xq, Mu, Us, 3, 3, 1), mahsq_device(J, ctx, Xn, Mu, Us, 3, 3, 1)
    assert np.all(np.isnan(got[i])) and not np.any(np.isnan(np.delete(got, i, axis=0)))
    assert np.array_equal(np.delete(got, i, axis=0), np.delete(clean, i, axis=0))


def test_mahsq_bad_arguments(J, ctx):
    Xq, Mu, Us, _, _ = prim_case(129, 17, 3, 3)
    m, p = Xq.shape
    Xf, Muf, Uf = np.asfortranarray(Xq), np.asfortranarray(Mu), np.ascontiguousarray(np.transpose(Us, (0, 2, 1)))
    out = np.full((3, m), SENT)
    L, H = J.load(), J._lib.LOC_HOST

    def call(**kw):
        a = dict(Xq=Xf.ctypes.data, m=m, p=p, ldq=m, Mu=Muf.ctypes.data, ncen=3, U=Uf.ctypes.data, ldu=p, us=p * p, nfac=3, out=out.ctypes.data, ldo=m)
        a.update(kw)
        return L.jch_mahsq_chol(ctx._h, H, a["Xq"], a["m"], a["p"], a["ldq"], a["Mu"], a["ncen"], a["U"], a["ldu"], a["us"], a["nfac"], a["out"], a["ldo"])
    for kw in (dict(Xq=None), dict(Mu=None), dict(U=None), dict(out=None), dict(ldq=m - 1), dict(ldu=p - 1), dict(ldo=m - 1), dict(nfac=2), dict(ncen=65536, nfac=1)):
        assert call(**kw) == J._lib.JCH_EINVAL, kw
        assert np.all(out == SENT)
    assert call() == 0 and not np.any(out == SENT)


# ---------------------------------------------------------------------------------- b. jch_class_cov
def class_cov_abi(J, ctx, Z, cs, where, want_Wi=True, want_W=True, pad=0, offset=0):
    n, p = Z.shape
    ncls = len(cs) - 1
    cs = np.ascontiguousarray(cs, dtype=np.int64)
    ct = np.full((p, ncls), SENT).T                                                # (ncls, p) column-major
    if where == "device":
        zb, za = _dev_colmajor(Z, n + pad, offset)
        Wi = torch.full((ncls * p * p + 1,), SENT, dtype=torch.float64, device="cuda:0")
        W = torch.full((p * p + 1,), SENT, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        wia, wa, ldz, loc = Wi.data_ptr(), W.data_ptr(), n + pad, J._lib.LOC_DEVICE
    else:
        Zf = np.asfortranarray(Z)
        Wi, W = np.full(ncls * p * p + 1, SENT), np.full(p * p + 1, SENT)
        za, wia, wa, ldz, loc = Zf.ctypes.data, Wi.ctypes.data, W.ctypes.data, n, J._lib.LOC_HOST
    ctx.check(J.load().jch_class_cov(ctx._h, loc, za, n, p, ldz, cs.ctypes.data, ncls, wia if want_Wi else None, wa if want_W else None,
                                     ct.ctypes.data))
    Wi, W = _host(Wi), _host(W)
    assert Wi[-1] == SENT and W[-1] == SENT
    if not want_Wi:
        assert np.all(Wi == SENT)
    if not want_W:
        assert np.all(W == SENT)
    if where == "device":
        assert _body(zb, n + pad, p, offset, n)[1], "Z was written"
    return Wi[:-1].reshape(ncls, p, p), W[:-1].reshape(p, p), np.array(ct)


def _class_cases():
    return {
        "n7_p3_1": (gauss_classes(7, 3, 1, 2)[0], np.array([0, 7])),
        "n50_p17_3": (gauss_classes(50, 17, 3, 4)[0], np.array([0, 17, 32, 50])),                # odd class offsets
        "n300_p129_2": (gauss_classes(300, 129, 2, 4)[0], np.array([0, 149, 300])),
        "n40_p5_one_row": one_row_classes(),
    }


@pytest.mark.parametrize("name", ["n7_p3_1", "n50_p17_3", "n300_p129_2", "n40_p5_one_row"])
def test_class_cov_against_longdouble_and_bitwise(J, ctx, name):
    Z, cs = _class_cases()[name]
    rWi, bWi, rct, bct, rW, bW = class_cov_reference(Z, cs)
    Wi, W, ct = class_cov_abi(J, ctx, Z, cs, "device")
    r1, r2 = ratio(Wi, rWi, bWi), ratio(W, rW, bW)
    r3 = ratio(ct, rct, np.maximum(bct, np.finfo(LD).tiny))
    print(f"{name}: Wi {r1:.3f}, W {r2:.3f}, ct {r3:.3f} of the bound")
    assert r1 <= 1.0 and r2 <= 1.0 and r3 <= 1.0
    assert np.array_equal(Wi, np.transpose(Wi, (0, 2, 1))) and np.array_equal(W, W.T), "not bitwise symmetric"
    for c in range(len(cs) - 1):
        if cs[c + 1] - cs[c] == 1:
            assert np.array_equal(ct[c], Z[cs[c]]), "the mean of a class of one row is the row"
    for other in (class_cov_abi(J, ctx, Z, cs, "device"), class_cov_abi(J, ctx, Z, cs, "host"), class_cov_abi(J, ctx, Z, cs, "device", pad=3, offset=1)):
        assert all(np.array_equal(a, b) for a, b in zip((Wi, W, ct), other)), "run / loc / alignment changes the bits"
    _, W2, ct2 = class_cov_abi(J, ctx, Z, cs, "device", want_Wi=False)
    Wi3, _, ct3 = class_cov_abi(J, ctx, Z, cs, "host", want_W=False)
    assert np.array_equal(W2, W) and np.array_equal(Wi3, Wi) and np.array_equal(ct2, ct) and np.array_equal(ct3, ct)


def test_class_cov_bad_arguments(J, ctx):
    Z, cs = _class_cases()["n50_p17_3"]
    Zf = np.asfortranarray(Z)
    n, p = Z.shape
    W = np.full(p * p, SENT)
    L, H = J.load(), J._lib.LOC_HOST

    def call(Zp=Zf.ctypes.data, cs=cs, ldz=n, csnull=False):
        c = np.ascontiguousarray(cs, dtype=np.int64)
        return L.jch_class_cov(ctx._h, H, Zp, n, p, ldz, None if csnull else c.ctypes.data, len(c) - 1, None, W.ctypes.data, None)
    for kw in (dict(Zp=None), dict(csnull=True), dict(ldz=n - 1), dict(cs=[0, 17, 17, 50]), dict(cs=[1, 17, 32, 50]), dict(cs=[0, 17, 32, 49]),
               dict(cs=[0, 32, 17, 50])):
        assert call(**kw) == J._lib.JCH_EINVAL, kw
        assert np.all(W == SENT)
    assert call() == 0


# ---------------------------------------------------------------------------------- c. jch_gauss_factor
def spd_stack(p, nfac, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nfac):
        A = rng.normal(size=(2 * p + 3, p))
        out.append(A.T @ A / (2 * p + 3) + 0.05 * np.eye(p))
    return np.stack(out)


def factor_abi(J, ctx, S, where, pad=0, offset=0):
    nfac, p, _ = S.shape
    diag, info = np.full((nfac, p), SENT), np.full(nfac, -1, dtype=np.int32)
    lds, ldu = p + pad, p + pad
    ss, us = lds * p + 1, ldu * p + 2
    Sb = np.full(offset + ss * nfac + 1, SENT)
    for f in range(nfac):
        Sb[offset + f * ss:offset + f * ss + lds * p].reshape(p, lds)[:, :p] = S[f].T
    if where == "device":
        Sd = torch.as_tensor(Sb, device="cuda:0")
        Ud = torch.full((offset + us * nfac + 1,), SENT, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        sa, ua, loc = Sd.data_ptr() + 8 * offset, Ud.data_ptr() + 8 * offset, J._lib.LOC_DEVICE
    else:
        Sd, Ud = Sb.copy(), np.full(offset + us * nfac + 1, SENT)
        sa, ua, loc = Sd.ctypes.data + 8 * offset, Ud.ctypes.data + 8 * offset, J._lib.LOC_HOST
    ctx.check(J.load().jch_gauss_factor(ctx._h, loc, sa, p, lds, ss, nfac, ua, ldu, us, diag.ctypes.data, info.ctypes.data))
    assert np.array_equal(_host(Sd), Sb), "S was written"
    Uh = _host(Ud)
    Us = []
    for f in range(nfac):
        blk = Uh[offset + f * us:offset + (f + 1) * us]
        M = blk[:ldu * p].reshape(p, ldu)
        assert np.all(M[:, p:] == SENT) and np.all(blk[ldu * p:] == SENT), "Uinv was written outside its p x p"
        Us.append(M[:, :p].T.copy())
    assert np.all(Uh[:offset] == SENT) and Uh[-1] == SENT
    return np.stack(Us), diag, info


@pytest.mark.parametrize("nfac", [1, 3])
@pytest.mark.parametrize("p", [1, 5, 128, 129, 260])
def test_gauss_factor_against_longdouble(J, ctx, p, nfac):
    S = spd_stack(p, nfac, 100 * p + nfac)
    Us, diag, info = factor_abi(J, ctx, S, "device")
    assert np.all(info == 0)
    for f in range(nfac):
        Ul, dl = chol_uinv(S[f], LD)
        tol = factor_tol(S[f])
        e = float(np.linalg.norm(np.asarray(Us[f] - Ul, dtype=np.float64)) / np.linalg.norm(np.asarray(Ul, dtype=np.float64)))
        ed = float(np.linalg.norm(np.asarray(diag[f] - dl, dtype=np.float64)) / np.linalg.norm(np.asarray(dl, dtype=np.float64)))
        print(f"p={p} factor {f}: cond2 {cond2(S[f]):.2e}, |Uinv - ld|_F / |ld|_F = {e:.2e}, diag {ed:.2e}; allowed {tol:.2e}: ratios {e / tol:.4f}, {ed / tol:.4f}")
        assert e <= tol and ed <= tol
        assert np.all(np.tril(Us[f], -1) == 0.0), "not exact zeros below the diagonal"
    for other in (factor_abi(J, ctx, S, "device"), factor_abi(J, ctx, S, "host"), factor_abi(J, ctx, S, "device", pad=1, offset=1)):
        assert np.array_equal(Us, other[0]) and np.array_equal(diag, other[1]), "run / loc / alignment changes the bits"


@pytest.mark.parametrize("p", [5, 129])
def test_gauss_factor_singular_second_factor(J, ctx, p):
    S = spd_stack(p, 3, 7 * p)
    good = factor_abi(J, ctx, S, "device")
    j = p // 2
    bad = np.array(S)
    bad[1, j, :] = 0.0
    bad[1, :, j] = 0.0                                                             # pivot j + 1 is exactly 0
    for where in ("device", "host"):
        Us, diag, info = factor_abi(J, ctx, bad, where)
        assert list(info) == [0, j + 1, 0]
        for f in (0, 2):
            assert np.array_equal(Us[f], good[0][f]) and np.array_equal(diag[f], good[1][f])


def test_gauss_factor_bad_arguments(J, ctx):
    S = np.ascontiguousarray(spd_stack(5, 2, 1))
    Uo, diag, info = np.full(50, SENT), np.zeros(10), np.zeros(2, dtype=np.int32)
    L, H = J.load(), J._lib.LOC_HOST

    def call(**kw):
        a = dict(S=S.ctypes.data, lds=5, ss=25, U=Uo.ctypes.data, ldu=5, us=25, d=diag.ctypes.data, i=info.ctypes.data)
        a.update(kw)
        return L.jch_gauss_factor(ctx._h, H, a["S"], 5, a["lds"], a["ss"], 2, a["U"], a["ldu"], a["us"], a["d"], a["i"])
    for kw in (dict(S=None), dict(U=None), dict(d=None), dict(i=None), dict(lds=4), dict(ldu=4)):
        assert call(**kw) == J._lib.JCH_EINVAL, kw
        assert np.all(Uo == SENT)
    assert call() == 0


# ---------------------------------------------------------------------------------- d. the models
def _put(a, where):
    return _dev(a) if where == "device" else np.asfortranarray(a)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("prior", ["unif", "prop"])
@pytest.mark.parametrize("kind", ["lda", "qda"])
@pytest.mark.parametrize("shape", list(MODEL_SHAPES))
def test_lda_qda_against_longdouble(J, ctx, monkeypatch, shape, kind, prior, where):
    n, p, nlev, m = MODEL_SHAPES[shape]
    X, y, Xq, _ = gauss_classes(n, p, nlev, m)
    ref = model_case(kind, shape, prior)
    fit, predict = (J.lda, J.lda_predict) if kind == "lda" else (J.qda, J.qda_predict)
    obj = fit(_put(X, where), y, prior=prior, ctx=ctx)
    assert isinstance(obj.fm[0].Uinv, torch.Tensor) == (where == "device")
    import jchemo_hip.gda as G
    seen = []
    real = G.mahsq_chol

    def spy(Xa, Mu, Uinv, **kw):
        seen.append(1 if (Uinv.dim() if isinstance(Uinv, torch.Tensor) else np.ndim(Uinv)) == 2 else Uinv.shape[0])
        return real(Xa, Mu, Uinv, **kw)
    monkeypatch.setattr(G, "mahsq_chol", spy)
    pred, dens, post = predict(obj, _put(Xq, where), ctx=ctx)
    assert seen == [1 if kind == "lda" else nlev], "lda_predict issues the kernel with nfac = 1, qda_predict with one factor per class"
    if kind == "lda":
        assert all(f.Uinv is obj.fm[0].Uinv for f in obj.fm)
    assert isinstance(dens, torch.Tensor) == (where == "device") and isinstance(pred, np.ndarray)
    d2 = real(_put(Xq, where), np.stack([f.mu for f in obj.fm]), obj.fm[0].Uinv if kind == "lda" else obj._Uinv, ctx=ctx)   # fitted and evaluated end to end
    assert_model(kind, pred, _host(dens), _host(post), ref, f"{kind} {shape} {prior} {where}", got_d2=_host(d2))
    assert np.array_equal(obj.lev, ref["obj"]["lev"]) and np.array_equal(obj.ni, ref["obj"]["ni"])
    assert np.allclose(obj.wprior, np.asarray(ref["obj"]["wprior"], dtype=np.float64), rtol=1e-15)
    assert np.allclose(obj.ct, np.asarray(ref["obj"]["ct"], dtype=np.float64), rtol=1e-13)


@pytest.mark.parametrize("where", ["host", "device"])
def test_qda_with_a_class_of_one_row(J, ctx, where):
    """Class sizes (1, 59, 60): the one-row class gets S = cov(X; corrected = false) of all rows (src/matW.jl:54-65, src/qda.jl:69-70)."""
    X, _, Xq, _ = gauss_classes(120, 5, 3, 257, sizes=(1, 59, 60))
    y = np.repeat(np.array(["c0", "c1", "c2"]), (1, 59, 60))
    from test_gda_static import model_reference
    ref = model_reference("qda", X, y, Xq, "prop")
    obj = J.qda(_put(X, where), y, prior="prop", ctx=ctx)
    pred, dens, post = J.qda_predict(obj, _put(Xq, where), ctx=ctx)
    assert_model("qda", pred, _host(dens), _host(post), ref, f"qda one-row class {where}")
    assert np.array_equal(_host(obj.Wi)[0], _host(J.matW(_put(X, where), np.zeros(120), ctx=ctx)[1])[0])


@pytest.mark.parametrize("where", ["host", "device"])
def test_dmnorm_against_longdouble(J, ctx, where):
    X, _, Xq, _ = gauss_classes(120, 5, 3, 257)
    for Xa, Xn in ((X, Xq), (X[:, 0], Xq[:, 0])):                                  # a matrix, and a p = 1 vector
        ref = np_dmnorm(Xa, ft=LD)
        rp = np_dmnorm_predict(ref, np.asarray(Xn, dtype=LD), form="diff")
        S = np_cov(np.asarray(Xa, dtype=np.float64).reshape(120, -1), corrected=True)
        p, tol = S.shape[0], factor_tol(S)
        d2 = np_mahsqchol(Xn, ref["mu"].reshape(1, -1), ref["Uinv"], ft=LD, form="diff")
        bound = (LD(0.5) * d2 * tol + p * tol + 8 * LD(EPS)) * rp
        fm = J.dmnorm(_put(Xa, where) if np.ndim(Xa) == 2 else (_dev(Xa) if where == "device" else np.array(Xa)), ctx=ctx)
        got = J.dmnorm_predict(fm, _put(Xn, where) if np.ndim(Xn) == 2 else (_dev(Xn) if where == "device" else np.array(Xn)), ctx=ctx)
        r = ratio(_host(got), rp, bound)
        print(f"dmnorm p={p} {where}: dens {r:.4f} of the bound; detS rel. error {abs(fm.detS - float(ref['detS'])) / float(ref['detS']):.2e}")
        assert r <= 1.0 and got.shape == (257, 1)
        assert abs(fm.detS - float(ref["detS"])) <= 2 * p * tol * float(ref["detS"])
        fm2 = J.dmnorm(mu=fm.mu, S=_put(S, where), ctx=ctx)                         # the mu =, S = form
        got2 = J.dmnorm_predict(fm2, _put(np.asarray(Xn).reshape(257, -1), where), ctx=ctx)
        assert ratio(_host(got2), rp, bound) <= 1.0


@pytest.mark.parametrize("where", ["host", "device"])
def test_matW_matB_and_mahsqchol(J, ctx, where):
    X, y, Xq, _ = gauss_classes(300, 20, 3, 385)
    W, Wi, lev, ni = J.matW(_put(X, where), y, ctx=ctx)
    order = np.argsort(np.searchsorted(lev, y), kind="stable")
    cs = np.concatenate([[0], np.cumsum(ni)])
    rWi, bWi, rct, bct, rW, bW = class_cov_reference(X[order], cs)
    r1, r2 = ratio(_host(Wi), rWi, bWi), ratio(_host(W), rW, bW)
    B, ct, lev2, ni2 = J.matB(_put(X, where), y, ctx=ctx)
    refB = np_matB(X, y, ft=LD)
    r3 = ratio(ct, rct, bct)
    eB = float(np.max(np.abs(np.asarray(B - refB["B"], dtype=np.float64))) / np.max(np.abs(np.asarray(refB["B"], dtype=np.float64))))
    print(f"matW {where}: Wi {r1:.3f}, W {r2:.3f}; matB: ct {r3:.3f} of the bound, B rel. error {eB:.2e}")
    assert r1 <= 1.0 and r2 <= 1.0 and r3 <= 1.0 and eB <= 100 * EPS
    assert isinstance(W, torch.Tensor) == (where == "device") and isinstance(B, np.ndarray)
    assert np.array_equal(lev, lev2) and np.array_equal(ni, ni2)
    # mahsqchol with a given factor: the primitive's bound; without: end to end under 50 eps cond2
    S = np_cov(np.asarray(X), corrected=False)
    Ul, _ = chol_uinv(S, LD)
    U64 = np.asfortranarray(np.asarray(Ul, dtype=np.float64))
    from test_gda_static import ld_mahsq
    d2, bound = ld_mahsq(Xq, X[:3], U64)
    got = J.mahsqchol(_put(Xq, where), _put(X[:3], where), _put(U64, where), ctx=ctx)
    ra = ratio(_host(got), d2, bound)
    dl = np_mahsqchol(X, Xq[:3], ft=LD, form="diff")
    got2 = J.mahsqchol(_put(X, where), _put(Xq[:3], where), ctx=ctx)
    rb = ratio(_host(got2), dl, factor_tol(S) * dl)
    print(f"mahsqchol {where}: with Uinv {ra:.3f} of the primitive's bound, without {rb:.4f} of 50 eps cond2")
    assert ra <= 1.0 and rb <= 1.0 and got.shape == (385, 3) and got2.shape == (300, 3)


def test_mahsqchol_big_case_d2_only(J, ctx):
    n, p, nlev, m = BIG_SHAPE
    X, _, Xq, _ = gauss_classes(n, p, nlev, m)
    S = np_cov(np.asarray(X), corrected=False)
    dl = np_mahsqchol(X, Xq[:2], ft=LD, form="diff")
    got = J.mahsqchol(_dev(X), Xq[:2], ctx=ctx)
    r = ratio(_host(got), dl, factor_tol(S) * dl)
    print(f"(400, 130, 2): cond2 {cond2(S):.3e}, d2 {r:.5f} of 50 eps cond2")
    assert r <= 1.0


def test_posdef_exceptions(J, ctx):
    X, y, _, _ = gauss_classes(120, 5, 3, 257)
    y2 = np.array(y)
    idx = np.flatnonzero(y2 == "c1")
    y2[idx[2:]] = "c2"                                                             # class c1 keeps 2 rows <= p: a covariance of rank 1 ...
    X2 = np.array(X)
    X2[idx[1], 0] = X2[idx[0], 0]                                                  # ... whose first pivot is exactly 0 (rounding cannot rescue it)
    with pytest.raises(ValueError, match=r"PosDefException: qda: class 'c1' \(2 rows\).*failed at column 1"):
        J.qda(np.asfortranarray(X2), y2, ctx=ctx)
    with pytest.raises(ValueError, match="PosDefException: lda"):
        J.lda(np.asfortranarray(X[:3]), ["a", "b", "c"], ctx=ctx)                  # n == nlev
    with pytest.raises(ValueError, match="PosDefException: dmnorm"):
        J.dmnorm(np.asfortranarray(X[:1]), ctx=ctx)                                # one row


# ---------------------------------------------------------------------------------- e. a used ctx
def test_every_entry_on_a_used_ctx(J, ctx, used_ctx):
    """Each entry, and each model, once on a ctx that a plskern fit and a krr fit have used (jch_gauss_factor shares chol_inv and the info word with
    krr): the bits of a fresh ctx."""
    Xq, Mu, Us, _, _ = prim_case(257, 260, 3, 3)
    assert np.array_equal(mahsq_device(J, used_ctx, Xq, Mu, Us, 3, 3, 1), mahsq_device(J, ctx, Xq, Mu, Us, 3, 3, 1))
    assert np.array_equal(mahsq_host(J, used_ctx, Xq, Mu, Us, 1), mahsq_host(J, ctx, Xq, Mu, Us, 1))
    Z, cs = _class_cases()["n300_p129_2"]
    for where in ("device", "host"):
        assert all(np.array_equal(a, b) for a, b in zip(class_cov_abi(J, used_ctx, Z, cs, where), class_cov_abi(J, ctx, Z, cs, where)))
    S = spd_stack(129, 3, 11)
    for where in ("device", "host"):
        a, b = factor_abi(J, used_ctx, S, where), factor_abi(J, ctx, S, where)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    X, y, Xn, _ = gauss_classes(120, 5, 3, 257)
    for fit, predict in ((J.lda, J.lda_predict), (J.qda, J.qda_predict)):
        ra, rb = predict(fit(X, y, ctx=used_ctx), Xn, ctx=used_ctx), predict(fit(X, y, ctx=ctx), Xn, ctx=ctx)
        assert all(np.array_equal(u, v) for u, v in zip(ra, rb))
    assert np.array_equal(J.dmnorm_predict(J.dmnorm(X, ctx=used_ctx), Xn, ctx=used_ctx), J.dmnorm_predict(J.dmnorm(X, ctx=ctx), Xn, ctx=ctx))
    assert np.array_equal(J.mahsqchol(X, Xn[:2], ctx=used_ctx), J.mahsqchol(X, Xn[:2], ctx=ctx))
    for a, b in zip(J.matW(X, y, ctx=used_ctx)[:2] + J.matB(X, y, ctx=used_ctx)[:2], J.matW(X, y, ctx=ctx)[:2] + J.matB(X, y, ctx=ctx)[:2]):
        assert np.array_equal(a, b)
    # and krr still solves on the ctx afterwards (the factor a solve is keyed to was invalidated, not corrupted)
    rng = np.random.default_rng(5)
    Xk, Yk = np.asfortranarray(rng.normal(size=(200, 30))), np.asfortranarray(rng.normal(size=(200, 2)))
    A1, _, df1 = J.krr_coef(J.krr(Xk, Yk, lb=0.1, ctx=used_ctx), ctx=used_ctx)
    A0, _, df0 = J.krr_coef(J.krr(Xk, Yk, lb=0.1, ctx=ctx), ctx=ctx)
    assert np.array_equal(A1, A0) and df1 == df0
