"""Calibration transfer on the GPU: jch_rows_fir in mode JCH_FIR_SAME | JCH_FIR_PER_COLUMN against the longdouble restatement of the header's
formula, the untouched uniform mode on the same shapes, a joined ctx, and calds / calpds / the device route of the mlr family against the
numpy restatements of test_caltransfer_static.

Tolerances (test_caltransfer_static derives them): the FIR mode element-wise under (K + 2) 2^-53 (|c_j| + sum_t |taps[t, j]| |x|); the
models under 50 eps cond_kept |B|_2 for the coefficients, propagated to a prediction as tol_B (1 + sum_j |x_ij|) plus the bound of the
product itself; the PLS-based transfers within 1e-9 relative Frobenius of the C oracle (the project's fixture tolerance); the device
moments route against the host route at 100 eps cond^2 |B|_2, the normal equations' own loss.  Every case prints err / bound."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_caltransfer_static as S  # noqa: E402
from jchemo_hip._lib import JCH_EINVAL as EINVAL  # noqa: E402
from oracle import plsr_oracle as O  # noqa: E402

EPS = S.EPS
LD = np.longdouble
PC = 4            # JCH_FIR_SAME | JCH_FIR_PER_COLUMN


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


def _dev(J, A):
    A = np.asarray(A, dtype=np.float64)
    D = J.colmajor_empty(A.shape[0], A.shape[1], "cuda:0")
    D.copy_(torch.from_numpy(A))
    return D


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _fir(J, ctx, X, taps, f, lo, mode, ld, where, inplace):
    """One jch_rows_fir call on X (n x p) stored with leading dimension ld; the rows beyond n of both buffers are NaN and must stay so."""
    L = J.load()
    n, p = X.shape
    buf = np.full((ld, p), np.nan, order="F")
    buf[:n] = X
    if where == "host":
        dst = buf if inplace else np.full((ld, p), np.nan, order="F")
        ctx.check(L.jch_rows_fir(ctx._h, 0, buf.ctypes.data, n, p, ld, taps.ctypes.data, f, lo, mode, dst.ctypes.data, ld))
        res, src = dst, buf
    else:
        sd = torch.from_numpy(np.ascontiguousarray(buf.T)).cuda()            # (p, ld) row-major == ld x p column-major
        dd = sd if inplace else torch.full((p, ld), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.check(L.jch_rows_fir(ctx._h, 1, sd.data_ptr(), n, p, ld, taps.ctypes.data, f, lo, mode, dd.data_ptr(), ld))
        res, src = dd.cpu().numpy().T, sd.cpu().numpy().T
    assert np.isnan(res[n:]).all(), "rows beyond n were written"
    if not inplace:
        assert np.array_equal(src[:n], X, equal_nan=True), "the input of a copying call was modified"
    return np.array(res[:n])


ROUTES = [(0, "host"), (0, "device"), (3, "device")]      # host arrays, device tensors, an unaligned device view (ldx = n + 3)


def _all_routes(J, ctx, X, taps, f, lo, mode):
    first = None
    for pad, where in ROUTES:
        for inplace in (False, True):
            got = _fir(J, ctx, X, taps, f, lo, mode, X.shape[0] + pad, where, inplace)
            if first is None:
                first = got
            else:
                assert np.array_equal(got, first, equal_nan=True), (pad, where, inplace)
    return first


def _ratio(got, ref, bound):
    err = np.abs((got.astype(LD) - ref).astype(np.float64))
    pos = bound > 0
    assert np.all(err[~pos] == 0.0)
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


# ---------------------------------------------------------------------------------- the per-column mode
@pytest.mark.parametrize("f", S.FIR_FS)
def test_per_column_mode_against_the_longdouble_restatement(J, ctx, f):
    worst = 0.0
    for n in S.FIR_NS:
        for p in S.FIR_PS:
            for lo in S.fir_los(f):
                X, tab = S.fir_case(n, p, f, lo)
                got = _all_routes(J, ctx, X, tab, f, lo, PC)                  # six routes, identical bits
                ref, bound = S.fir_ref(X, tab, lo)
                r = _ratio(got, ref, bound)
                worst = max(worst, r)
                assert r <= 1.0, (n, p, f, lo, r)
    print(f"  per-column f={f}: worst err / bound {worst:.3f}")


def test_per_column_nan_stays_in_its_row_and_zero_taps_hide_inf(J, ctx):
    for f, lo in ((11, -5), (58, -29)):
        X, tab = S.fir_case(130, 33, f, lo)
        clean = _all_routes(J, ctx, X, tab, f, lo, PC)
        Xn = X.copy()
        Xn[64, 7] = np.nan
        Xn[3, 20] = np.inf
        got = _all_routes(J, ctx, Xn, tab, f, lo, PC)
        rows = np.ones(130, dtype=bool)
        rows[[3, 64]] = False
        assert np.array_equal(got[rows], clean[rows]) and np.isnan(got[64]).any() and not np.isfinite(got[3]).all()
        # an Inf under exactly zero taps: the table of a PDS model, whose border windows are zero-padded
        z = np.zeros((f + 1, 33), order="F")
        z[-lo] = 1.0                                                         # identity ...
        z[f] = 0.5                                                           # ... plus a constant
        Xi = X.copy()
        Xi[5, 0] = np.inf
        got = _all_routes(J, ctx, Xi, z, f, lo, PC)
        assert np.isinf(got[5, 0]) and np.isfinite(got[5, 1:]).all() and np.array_equal(got[:, 1:], X[:, 1:] + 0.5)


def test_per_column_bad_arguments(J, ctx):
    L = J.load()
    X, tab = S.fir_case(8, 6, 3, -1)
    out = np.zeros((8, 6), order="F")
    xa, ta, oa = X.ctypes.data, tab.ctypes.data, out.ctypes.data
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 3, 0, 1 | PC, oa, 8) == EINVAL          # VALID | PER_COLUMN
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 3, -1, 8, oa, 8) == EINVAL              # mode 8
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 3, -1, 6, oa, 8) == EINVAL              # 2 | PER_COLUMN: 2 is not a mode
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, None, 3, -1, PC, oa, 8) == EINVAL           # a NULL table
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 3, 1, PC, oa, 8) == EINVAL              # lo > 0
    assert L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 3, -3, PC, oa, 8) == EINVAL             # lo < -(f - 1)
    assert np.all(out == 0.0)
    ctx.check(L.jch_rows_fir(ctx._h, 0, xa, 8, 6, 8, ta, 3, -1, PC, oa, 8))                   # the ctx works as usual afterwards
    ref, bound = S.fir_ref(X, tab, -1)
    assert _ratio(out, ref, bound) <= 1.0


# ---------------------------------------------------------------------------------- the existing mode on the same shapes
@pytest.mark.parametrize("f", S.FIR_FS)
def test_uniform_same_mode_is_untouched(J, ctx, f):
    worst = 0.0
    for n in S.FIR_NS:
        for p in S.FIR_PS:
            for lo in S.fir_los(f):
                X, tab = S.fir_case(n, p, f, lo)
                taps = np.ascontiguousarray(tab[:f, p // 2])                  # one column's taps (exact zeros included), for every output
                got = _all_routes(J, ctx, X, taps, f, lo, 0)
                uni = np.zeros((f + 1, p), order="F")
                uni[:f] = taps[:, None]
                ref, bound = S.fir_ref(X, uni, lo)
                f64 = np.zeros((n, p))                                       # the float64 evaluation in the header's order
                for t in range(f):
                    if taps[t] != 0.0:
                        f64 += taps[t] * X[:, np.clip(np.arange(p) + lo + t, 0, p - 1)]
                err = np.abs(got - f64)
                assert np.all(err <= bound), (n, p, f, lo)
                worst = max(worst, _ratio(got, ref, bound))
                assert worst <= 1.0
    print(f"  uniform SAME f={f}: worst err / bound {worst:.3f}")


# ---------------------------------------------------------------------------------- a joined ctx
def test_per_column_mode_on_a_joined_ctx(J, ctx):
    L = J.load()
    n, p, f, lo = 130, 33, 11, -5
    X, tab = S.fir_case(n, p, f, lo)
    want = _fir(J, ctx, X, tab, f, lo, PC, n, "device", False)
    nr = 2
    grp = C.c_void_p()
    assert L.jch_loopback_group_create(nr, C.byref(grp)) == 0
    ctxs = [J.Context(0) for _ in range(nr)]
    xs = [_dev(J, X) for _ in range(nr)]
    outs = [J.colmajor_empty(n, p, "cuda:0") for _ in range(nr)]
    err = [None] * nr
    torch.cuda.synchronize()

    def work(r):
        try:
            ctxs[r].comm_init_loopback(grp, r, nr)
            ctxs[r].check(L.jch_rows_fir(ctxs[r]._h, 1, xs[r].data_ptr(), n, p, n, tab.ctypes.data, f, lo, PC, outs[r].data_ptr(), n))
        except BaseException as e:  # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(nr)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=30)
    assert not any(t.is_alive() for t in th), "a rank did not come back from a rank-local entry"
    for c in ctxs:
        c.close()
    L.jch_loopback_group_destroy(grp)
    for e in err:
        if e is not None:
            raise e
    for r in range(nr):
        assert _host(outs[r]).tobytes() == want.tobytes()                    # the bytes of the unjoined call
        assert np.array_equal(_host(xs[r]), X)


# ---------------------------------------------------------------------------------- calpds
def _pds_loop(fm_coefs, X, p, m):
    """The reference's per-column loop (src/calpds.jl:94-97) in longdouble with the given coefficients, and the kernel bound."""
    win = S.restate_windows(p, m)
    ref = np.zeros(X.shape, dtype=LD)
    mag = np.zeros(X.shape)
    for i, w in enumerate(win):
        B, c = fm_coefs[i]
        cols = [k - 1 for k in w]
        ref[:, i] = X[:, cols].astype(LD) @ np.asarray(B, dtype=LD).reshape(-1) + LD(float(np.asarray(c).reshape(-1)[0]))
        mag[:, i] = np.abs(X[:, cols]) @ np.abs(np.asarray(B).reshape(-1)) + abs(float(np.asarray(c).reshape(-1)[0]))
    K = np.array([len(w) for w in win])
    return ref, (K + 2)[None, :] * 2.0 ** -53 * mag


@pytest.mark.parametrize("dup", [False, True])
def test_calpds_mlrpinv(J, ctx, dup):
    X, Xt = S.standards()
    Xn = S.library(3, 130)
    if dup:                                                                  # a twin column: every window that holds both is rank deficient
        X, Xn = X.copy(order="F"), Xn.copy(order="F")
        X[:, 11], Xn[:, 11] = X[:, 10], Xn[:, 10]
    fm = J.calpds(X, Xt, fun=J.mlrpinv, m=3)
    for i in (0, 2, 10, 12, 32):
        B, b0, A = S.np_mlr("mlrpinv", X[:, fm.s[i]], Xt[:, i])
        cond = S._ratios_clear(A)
        assert np.abs(fm.fm[i].B - B).max() <= 50 * EPS * cond * np.linalg.norm(B, 2)
        if dup and i in (10, 12):
            a, b = list(fm.s[i]).index(10), list(fm.s[i]).index(11)
            assert abs(fm.fm[i].B[a, 0] - fm.fm[i].B[b, 0]) <= 50 * EPS * cond * np.linalg.norm(B, 2)      # minimum norm
    ref, bound = _pds_loop([J.coef(g) for g in fm.fm], Xn, 33, 3)
    pred = J.predict(fm, Xn, ctx=ctx)
    assert isinstance(pred, np.ndarray) and pred.shape == Xn.shape                                      # host in, host out
    r = _ratio(pred, ref, bound)
    print(f"  calpds mlrpinv dup={dup}: err / bound {r:.3f}")
    assert r <= 1.0
    Xd = _dev(J, Xn)
    pd = J.predict(fm, Xd, ctx=ctx)
    assert torch.is_tensor(pd) and pd.is_cuda and np.array_equal(_host(pd), pred)                       # device in, device out, the same bits
    assert np.array_equal(_host(Xd), Xn)
    same = J.calpds_predict(fm, Xd, ctx=ctx, inplace=True)
    assert same is Xd and np.array_equal(_host(Xd), pred)
    back = J.predict(fm, X, ctx=ctx)                                                                    # and it is a transfer: the standards land on
    assert np.abs(back - Xt).max() < 0.02                                                               # their targets (noise 1e-3, signal of order 1)


def test_calpds_plskern_docstring_example(J, ctx):
    X, Xt = S.standards()
    Xn = S.library(4, 130)
    fm = J.calpds(X, Xt, fun=J.plskern, nlv=1, m=2, ctx=ctx)
    pred = J.predict(fm, Xn, ctx=ctx)
    win = S.restate_windows(33, 2)
    ref = np.empty_like(Xn)
    for i, w in enumerate(win):
        cols = [k - 1 for k in w]
        o = O.plskern(np.ascontiguousarray(X[:, cols]), np.ascontiguousarray(Xt[:, i:i + 1]), nlv=1)
        ref[:, i] = np.asarray(O.predict(o, np.ascontiguousarray(Xn[:, cols]))).reshape(-1)
    r = O.rel_fro(ref, pred)
    print(f"  calpds plskern nlv=1 m=2: rel. Frobenius {r:.2e}")
    assert r <= 1e-9
    assert np.array_equal(J.predict(fm, Xn, nlv=1, ctx=ctx), pred)
    with pytest.raises(ValueError):
        J.predict(fm, Xn, nlv=[0, 1], ctx=ctx)


def test_calpds_loop_route_for_a_model_without_coef(J, ctx):
    X, Xt = S.standards()
    Xn = S.library(5, 64)
    fm = J.calpds(X[:, :9], Xt[:, :9], fun="krr", m=2, lb=1e-2, ctx=ctx)
    assert type(fm.fm[0]).__name__ == "Krr"
    pred = J.predict(fm, Xn[:, :9], ctx=ctx)
    assert isinstance(pred, np.ndarray) and pred.shape == (64, 9)
    for i, s in enumerate(fm.s):
        assert np.array_equal(pred[:, i], np.asarray(J.krr_predict(fm.fm[i], Xn[:, s[0]:s[-1] + 1], ctx=ctx))[:, 0])
    Xd = _dev(J, Xn[:, :9])
    pd = J.predict(fm, Xd, ctx=ctx)
    assert torch.is_tensor(pd) and pd.is_cuda and tuple(pd.shape) == (64, 9)
    for i, s in enumerate(fm.s):
        assert np.array_equal(_host(pd[:, i]), _host(J.krr_predict(fm.fm[i], Xd[:, s[0]:s[-1] + 1], ctx=ctx))[:, 0])


# ---------------------------------------------------------------------------------- calds
COLS = list(range(1, 33, 3))      # eleven columns: sqrtD Xc keeps its singular ratios clear of the threshold


def test_calds_mlrpinv(J, ctx):
    X, Xt = S.standards()
    Xs, Ys, Xn = np.asfortranarray(X[:, COLS]), np.asfortranarray(Xt[:, COLS]), np.asfortranarray(S.library(6, 130)[:, COLS])
    fm = J.calds(Xs, Ys, fun=J.mlrpinv)
    B, b0, A = S.np_mlr("mlrpinv", Xs, Ys)
    cond = S._ratios_clear(A)
    tolB = 50 * EPS * cond * np.linalg.norm(B, 2)
    assert np.abs(fm.fm.B - B).max() <= tolB
    ref = Xn.astype(LD) @ B.astype(LD) + b0.astype(LD)
    mag = np.abs(Xn) @ np.abs(B) + np.abs(b0)
    tol = tolB * (1.0 + np.abs(Xn).sum(axis=1, keepdims=True)) + (len(COLS) + 2) * 2.0 ** -53 * mag
    for Xin in (Xn, _dev(J, Xn)):
        pred = J.predict(fm, Xin, ctx=ctx)
        assert type(pred) is type(Xin)
        err = np.abs((_host(pred).astype(LD) - ref).astype(np.float64))
        print(f"  calds mlrpinv: cond {cond:.3g}, max err / tol {float((err / tol).max()):.3f}")
        assert np.all(err <= tol)


def test_calds_plskern(J, ctx):
    X, Xt = S.standards()
    Xn = S.library(7, 130)
    fm = J.calds(X, Xt, fun="plskern", nlv=5, ctx=ctx)
    o = O.plskern(np.ascontiguousarray(X), np.ascontiguousarray(Xt), nlv=5)
    ref = np.asarray(O.predict(o, np.ascontiguousarray(Xn)))
    for Xin in (Xn, _dev(J, Xn)):
        pred = J.predict(fm, Xin, ctx=ctx)
        assert type(pred) is type(Xin)
        r = O.rel_fro(ref, _host(pred))
        print(f"  calds plskern nlv=5: rel. Frobenius {r:.2e}")
        assert r <= 1e-9


@pytest.mark.parametrize("wkind", ["none", "zeros"])
@pytest.mark.parametrize("kind", ["mlrchol", "mlrpinvn", "mlrvec"])
def test_mlr_device_moments_route(J, ctx, monkeypatch, kind, wkind):
    from jchemo_hip import caltransfer as CT
    X, Xt = S.standards()
    cols = S.FUNS[kind][0]
    Xs, Y = np.asfortranarray(X[:, cols]), np.asfortranarray(Xt[:, 15:18])
    w = S._weights(wkind, 40)
    host = getattr(J, kind)(Xs, Y, w)
    monkeypatch.setattr(CT, "HOST_ROUTE_MAX", 0)                             # every size now takes the device route
    sq = np.sqrt(S.np_mweight(w, 40))[:, None]
    sv = np.linalg.svd(sq * (Xs - S.np_mweight(w, 40) @ Xs), compute_uv=False)
    cond = float(sv[0] / sv[-1])
    tol = 100 * EPS * cond ** 2 * np.linalg.norm(host.B, 2)
    for Xin, Yin in ((_dev(J, Xs), _dev(J, Y)), (Xs, Y)):
        keep = _host(Xin).copy()
        fm = getattr(J, kind + "_")(Xin, Yin, w, ctx=ctx)                    # on this route the `_` form leaves X alone
        assert np.array_equal(_host(Xin), keep)
        err = float(np.abs(fm.B - host.B).max())
        print(f"  {kind} w={wkind}: cond {cond:.3g}, max |dB| {err:.3e}, tol {tol:.3e}")
        assert err <= tol
        assert np.abs(fm.int - host.int).max() <= tol * (1.0 + np.abs(Xs).max() * len(cols)) + 8 * EPS * np.abs(host.int).max()
        assert np.allclose(fm.weights, host.weights, rtol=8 * EPS, atol=0)
    for fn, kw in ((J.mlr, {}), (J.mlrpinv, {}), (J.mlrvec, dict(noint=True))):
        with pytest.raises(NotImplementedError, match="mlrchol / mlrpinvn"):
            fn(_dev(J, X[:, :1]) if fn is J.mlrvec else _dev(J, Xs), _dev(J, Y), **kw)


def test_mlr_predict_and_difmean_on_the_device(J, ctx):
    X, Xt = S.standards()
    fm = J.mlrpinv(X[:, S.WIN], Xt[:, 15:18])
    Xn = np.asfortranarray(S.library(8, 65)[:, S.WIN])
    ref = Xn.astype(LD) @ fm.B.astype(LD) + fm.int.astype(LD)
    bound = (len(S.WIN) + 2) * 2.0 ** -53 * (np.abs(Xn) @ np.abs(fm.B) + np.abs(fm.int))
    ph, pd = J.predict(fm, Xn, ctx=ctx), J.predict(fm, _dev(J, Xn), ctx=ctx)
    assert isinstance(ph, np.ndarray) and torch.is_tensor(pd) and pd.is_cuda
    assert _ratio(ph, ref, bound) <= 1.0 and _ratio(_host(pd), ref, bound) <= 1.0
    small = J.mlrvec(_dev(J, X[:, 16:17]), _dev(J, Xt[:, 15:18]))           # device tensors on the host route are downloaded
    assert np.array_equal(small.B, J.mlrvec(X[:, 16:17], Xt[:, 15:18]).B)
    D, m1, m2 = J.difmean(_dev(J, X), _dev(J, Xt[:17]), normx=True, ctx=ctx)
    Dh, h1, h2 = J.difmean(X, Xt[:17], normx=True)
    assert D.shape == (1, 33) and np.abs(D - Dh).max() <= 40 * EPS and np.abs(m1 - h1).max() <= 40 * EPS and np.abs(m2 - h2).max() <= 40 * EPS
