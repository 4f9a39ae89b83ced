"""One entry through the C ABI by three routes: device buffers, host arrays with ld == rows, host arrays with ld = rows + 3.  One strided copy
serves every entry (jch_copy2d, csrc/util.hip): contiguous when both pitches equal the rows, 2-D otherwise, so both host forms are run.  Every
matrix lives in a NaN-filled allocation between NaN guards (two doubles in front, two behind) with NaN in the rows beyond its own; the two host
routes must give the bytes of the device route, leave padding and guards NaN and the inputs as they were.  Shapes: 65 training rows, 67 queries
(more than one wave), 3 columns (an odd count: a pad column where the entry pads), 5 where an entry needs more.

ROUTES[family][entry] = run(L, ctx, loc, mat, out) -> (input buffers, output arrays); each family's GPU test file parametrises over its own."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "jchemo.jl_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NAN = float("nan")
HN, HM, HP = 65, 67, 3
GUARD = 2


class HostMat:
    """A column-major rows x cols host matrix with leading dimension ld inside a NaN-filled buffer, GUARD doubles in front and behind."""

    def __init__(self, A=None, rows=None, cols=None, ld=None):
        if A is not None:
            A = np.asarray(A, dtype=np.float64)
            A = A.reshape(len(A), -1)
            rows, cols = A.shape
        self.rows, self.cols, self.ld, self.src = rows, cols, (rows if ld is None else ld), A
        self.buf = np.full(GUARD + self.ld * cols + GUARD, NAN)
        self.body = self.buf[GUARD:GUARD + self.ld * cols].reshape(cols, self.ld)      # body[j] = column j
        if A is not None:
            self.body[:, :rows] = A.T
        self.ptr = self.buf.ctypes.data + 8 * GUARD

    def get(self, cols=None):
        cols = self.cols if cols is None else cols
        assert np.isnan(self.buf[:GUARD]).all() and np.isnan(self.buf[GUARD + self.ld * self.cols:]).all(), "written outside the host buffer"
        assert np.isnan(self.body[:, self.rows:]).all(), "the rows beyond the host matrix were written"
        assert np.isnan(self.body[cols:]).all(), "a column beyond the host output was written"
        return np.array(self.body[:cols, :self.rows].T)

    def unchanged(self):
        assert np.array_equal(self.get(), self.src), "a host input was modified"


def vec(v):
    return None if v is None else v.ctypes.data


def three_routes(run):
    """run(L, ctx, loc, mat, out): mat(A, nold=False) an input matrix, out(rows, cols, nold=False) an output; nold: the entry takes no leading
    dimension for it (ld == rows on every route)."""
    import torch
    import jchemo_hip as J
    from test_gpu_accessors import Dev
    L, ctx = J.load(), J.Context(0)
    try:
        def dev(*a, **kw):
            d = Dev(*a, **kw)
            torch.cuda.synchronize()        # (filled on torch's stream, read on the ctx's)
            return d
        ins, ref = run(L, ctx, 1, lambda A, nold=False: dev(A), lambda r, c, nold=False: dev(rows=r, cols=c + 1))
        for x in ins:
            x.unchanged()
        for pad in (0, 3):
            ins, got = run(L, ctx, 0, lambda A, nold=False: HostMat(A, ld=len(A) + (0 if nold else pad)),
                           lambda r, c, nold=False: HostMat(rows=r, cols=c + 1, ld=r + (0 if nold else pad)))
            for x in ins:
                x.unchanged()
            assert len(got) == len(ref)
            for i, (a, b) in enumerate(zip(got, ref)):
                a, b = np.asarray(a), np.asarray(b)
                assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"output {i}: the host route with ld = rows + {pad} differs from the device route"
    finally:
        ctx.close()


def _data(p=HP):
    rng = np.random.default_rng(650367 + p)
    X, Q = rng.standard_normal((HN, p)), rng.standard_normal((HM, p))
    Y = X[:, :2] * 1.5 + 0.1 * rng.standard_normal((HN, 2))
    return dict(X=X, Q=Q, Y=Y, Z=rng.standard_normal((HM, 2)), B=np.asfortranarray(rng.standard_normal((p, 2))), shift=rng.standard_normal(p),
                ind=rng.integers(0, HN, size=(HM, 1)).astype(np.int32), w=np.ones((HM, 1)), P=np.asfortranarray(rng.standard_normal((p, 4))))


def _sync(L, ctx):
    ctx.check(L.jch_ctx_synchronize(ctx._h))


def _i32():
    return C.c_int32(0)


def _desc(loc, n, p, q, nlv):
    from jchemo_hip import _lib
    return _lib.PlsDesc(n, p, q, nlv, 0, 0, loc, 0, 0)


# ---------------------------------------------------------------------------------- occ, stah, samp
def row_resid_ss(L, ctx, loc, mat, out):
    d = _data()
    x, z, o = mat(d["Q"]), mat(d["Z"]), out(HM, 1, True)
    ctx.check(L.jch_row_resid_ss(ctx._h, loc, x.ptr, HM, HP, x.ld, vec(d["shift"]), z.ptr, 2, z.ld, vec(d["B"]), HP, o.ptr))
    return [x, z], [o.get(1)]


def col_median_mad(L, ctx, loc, mat, out):
    x, med, mad = mat(_data()["X"]), np.full(HP, NAN), np.full(HP, NAN)
    ctx.check(L.jch_col_median_mad(ctx._h, loc, x.ptr, HN, HP, x.ld, vec(med), vec(mad), 0))
    return [x], [med, mad]


def stah(L, ctx, loc, mat, out):
    d = _data()
    x, dd, mu, s = mat(d["X"]), out(HN, 1, True), np.full(4, NAN), np.full(4, NAN)
    ctx.check(L.jch_stah(ctx._h, loc, x.ptr, HN, HP, x.ld, None, None, vec(d["P"]), 4, HP, 1, vec(mu), vec(s), dd.ptr))
    return [x], [mu, s, dd.get(1)]


def farthest_pair(L, ctx, loc, mat, out):
    x, pair, d2 = mat(_data()["X"]), np.full(2, -1, dtype=np.int64), np.full(1, NAN)
    ctx.check(L.jch_farthest_pair(ctx._h, loc, x.ptr, HN, HP, x.ld, None, 0, pair.ctypes.data, vec(d2)))
    return [x], [pair, d2]


def maxmin_select(L, ctx, loc, mat, out):
    x, init, sel, dsel = mat(_data()["X"]), np.array([0, 5], dtype=np.int64), np.full(6, -1, dtype=np.int64), np.full(6, NAN)
    ctx.check(L.jch_maxmin_select(ctx._h, loc, x.ptr, HN, HP, x.ld, 1, init.ctypes.data, 6, sel.ctypes.data, vec(dsel)))
    assert np.array_equal(init, [0, 5])
    return [x], [sel, dsel]


# ---------------------------------------------------------------------------------- kde, knn
def kde_dens(L, ctx, loc, mat, out):
    d = _data()
    z, q, o = mat(d["X"]), mat(d["Q"]), out(HM, 2)
    cls, dims = np.array([0, 30, HN], dtype=np.int64), np.array([HP], dtype=np.int32)
    u, v2, coef = np.ones((HP, 2), order="F"), np.ones((1, 2), order="F"), np.ones((1, 2), order="F")
    ctx.check(L.jch_kde_dens(ctx._h, loc, z.ptr, HN, HP, z.ld, q.ptr, HM, q.ld, cls.ctypes.data, 2, vec(u), vec(v2), vec(coef), dims.ctypes.data, 1, o.ptr, o.ld))
    return [z, q], [o.get(2)]


def knn_wmean(L, ctx, loc, mat, out):
    import torch
    d = _data()
    y, o = mat(d["X"]), out(HM, HP, True)
    ic, wc = d["ind"].ravel().copy(), d["w"].ravel().copy()
    if loc == 1:
        it, wt = torch.from_numpy(ic).cuda(), torch.from_numpy(wc).cuda()
        ip, wp = it.data_ptr(), wt.data_ptr()
    else:
        ip, wp = ic.ctypes.data, wc.ctypes.data
    torch.cuda.synchronize()
    ctx.check(L.jch_knn_wmean(ctx._h, loc, y.ptr, HN, HP, y.ld, ip, wp, HM, 1, o.ptr))
    _sync(L, ctx)        # (device in, device out: the entry only enqueues)
    assert np.array_equal(ic, d["ind"].ravel()) and np.array_equal(wc, d["w"].ravel())
    return [y], [o.get(HP)]


def knn_search(L, ctx, loc, mat, out):
    import torch
    d, k = _data(), 4
    z, q = mat(d["X"]), mat(d["Q"])
    model = C.c_void_p()
    ctx.check(L.jch_knn_prepare(ctx._h, loc, z.ptr, HN, HP, z.ld, C.byref(model)))
    try:
        if loc == 1:
            ind, dist, w = (torch.full((HM * k,), -1, dtype=torch.int32, device="cuda"), torch.full((HM * k,), NAN, dtype=torch.float64, device="cuda"),
                            torch.full((HM * k,), NAN, dtype=torch.float64, device="cuda"))
            torch.cuda.synchronize()
            ptrs = [t.data_ptr() for t in (ind, dist, w)]
        else:
            ind, dist, w = np.full(HM * k, -1, dtype=np.int32), np.full(HM * k, NAN), np.full(HM * k, NAN)
            ptrs = [a.ctypes.data for a in (ind, dist, w)]
        ctx.check(L.jch_knn_search(ctx._h, model, loc, q.ptr, HM, q.ld, k, None, 2.0, 1e-4, loc, ptrs[0], ptrs[1], ptrs[2], None))
        _sync(L, ctx)
        outs = [t.cpu().numpy() if loc == 1 else t for t in (ind, dist, w)]
    finally:
        L.jch_knn_release(ctx._h, model)
    return [z, q], outs


# ---------------------------------------------------------------------------------- kernel methods
KNLV = 3


def kernel_gram(L, ctx, loc, mat, out):
    d = _data()
    z, x, k = mat(d["Q"]), mat(d["X"]), out(HM, HN)
    ctx.check(L.jch_kernel_gram(ctx._h, loc, 0, z.ptr, HM, z.ld, None, x.ptr, HN, x.ld, None, HP, 0.5, 0.0, 1, k.ptr, k.ld))
    return [z, x], [k.get(HN)]


def dkplsr(L, ctx, loc, mat, out):
    d, A, n, q = _data(), KNLV, HN, 2
    x, y, xq = mat(d["X"]), mat(d["Y"]), mat(d["Q"])
    T, wn = out(n, A, True), out(n, 1, True)
    P, R, W = (np.full(n * A, NAN) for _ in range(3))
    Cm, TT, xm, xs, ym, ys, dxs, dys = np.full(q * A, NAN), np.full(A, NAN), np.full(n, NAN), np.full(n, NAN), np.full(q, NAN), np.full(q, NAN), np.full(HP, NAN), np.full(q, NAN)
    got, desc = _i32(), _desc(loc, n, HP, q, A)
    ctx.check(L.jch_dkplsr_fit(ctx._h, C.byref(desc), 0, 0.5, 0.0, 1, x.ptr, x.ld, y.ptr, y.ld, None, None, T.ptr, vec(P), vec(R), vec(W), vec(Cm), vec(TT), vec(xm),
                               vec(xs), vec(ym), vec(ys), wn.ptr, vec(dxs), vec(dys), C.byref(got)))
    assert got.value == A
    Tn, pr = out(HM, A), out(HM, (A + 1) * q)
    ctx.check(L.jch_dkplsr_transform(ctx._h, loc, 0, 0.5, 0.0, 1, xq.ptr, HM, HP, xq.ld, None, x.ptr, n, x.ld, vec(xm), vec(xs), vec(R), A, Tn.ptr, Tn.ld))
    ctx.check(L.jch_dkplsr_predict(ctx._h, loc, 0, 0.5, 0.0, 1, xq.ptr, HM, HP, xq.ld, None, x.ptr, n, x.ld, vec(xm), vec(xs), vec(ym), vec(ys), vec(R), vec(Cm), q, 0, A,
                                   vec(dys), pr.ptr, pr.ld))
    return [x, y, xq], [T.get(A), P, R, W, Cm, TT, xm, ym, wn.get(1), Tn.get(A), pr.get((A + 1) * q)]


def kplsr(L, ctx, loc, mat, out):
    d, A, n, q = _data(), KNLV, HN, 2
    x, y, xq = mat(d["X"]), mat(d["Y"]), mat(d["Q"])
    T, U, R, vt, wn = out(n, A, True), out(n, A, True), out(n, A, True), out(n, 1, True), out(n, 1, True)
    Cm, xs, ym, ys = np.full(q * A, NAN), np.full(HP, NAN), np.full(q, NAN), np.full(q, NAN)
    it, got, desc = (C.c_int32 * A)(), _i32(), _desc(loc, n, HP, q, A)
    ctx.check(L.jch_kplsr_fit(ctx._h, C.byref(desc), 0, 0.5, 0.0, 1, 1.5e-8, 100, x.ptr, x.ld, y.ptr, y.ld, None, None, T.ptr, U.ptr, R.ptr, vt.ptr, vec(Cm), vec(xs), vec(ym),
                              vec(ys), wn.ptr, it, C.byref(got)))
    assert got.value == A
    Rh, vth, wnh = np.asfortranarray(R.get(A)), np.ascontiguousarray(vt.get(1)[:, 0]), np.ascontiguousarray(wn.get(1)[:, 0])
    Tn, pr = out(HM, A), out(HM, (A + 1) * q)
    ctx.check(L.jch_kplsr_transform(ctx._h, loc, 0, 0.5, 0.0, 1, xq.ptr, HM, HP, xq.ld, vec(xs), x.ptr, n, x.ld, vec(wnh), vec(vth), vec(Rh), A, Tn.ptr, Tn.ld))
    ctx.check(L.jch_kplsr_predict(ctx._h, loc, 0, 0.5, 0.0, 1, xq.ptr, HM, HP, xq.ld, vec(xs), x.ptr, n, x.ld, vec(wnh), vec(vth), vec(ym), vec(ys), vec(Rh), vec(Cm), q, 0, A,
                                  pr.ptr, pr.ld))
    return [x, y, xq], [T.get(A), U.get(A), Rh, vth, wnh, Cm, ym, np.array(list(it), dtype=np.int32), Tn.get(A), pr.get((A + 1) * q)]


def kpca(L, ctx, loc, mat, out):
    d, A, n = _data(), KNLV, HN
    x = mat(d["X"])
    T, P, vt, wn = out(n, A, True), out(n, A, True), out(n, 1, True), out(n, 1, True)
    xs, sv, eig, ss, res = np.full(HP, NAN), np.full(A, NAN), np.full(A, NAN), np.full(1, NAN), np.full(A, NAN)
    nit, got = _i32(), _i32()
    ctx.check(L.jch_kpca_fit(ctx._h, loc, 0, 0.5, 0.0, 1, x.ptr, n, HP, x.ld, None, A, 0, 1e-9, 200, None, T.ptr, P.ptr, vt.ptr, wn.ptr, vec(xs), vec(sv), vec(eig), vec(ss),
                             C.byref(nit), vec(res), C.byref(got)))
    return [x], [T.get(A), P.get(A), vt.get(1), wn.get(1), sv, eig, ss, np.array([nit.value, got.value])]


def krr(L, ctx, loc, mat, out):
    import torch
    d, n, q = _data(), HN, 2
    x, y = mat(d["X"]), mat(d["Y"])
    B, vt, wn = out(n, q, True), out(n, 1, True), out(n, 1, True)
    Kd = torch.full((n * n,), NAN, dtype=torch.float64, device="cuda")      # (the working Gram is a device matrix on every route)
    torch.cuda.synchronize()
    xs, ym = np.full(HP, NAN), np.full(q, NAN)
    ctx.check(L.jch_krr_fit(ctx._h, loc, 0, 0.5, 0.0, 1, x.ptr, n, HP, x.ld, y.ptr, q, y.ld, None, 0, Kd.data_ptr(), None, B.ptr, vt.ptr, wn.ptr, vec(xs), vec(ym)))
    return [x, y], [B.get(q), vt.get(1), wn.get(1), xs, ym, Kd.cpu().numpy()]


# ---------------------------------------------------------------------------------- lwplsr, xtdx, pca
def _lw_args():
    d = _data(5)
    return d, 5, 1, 2, 20, 2       # data, p, q, dd, k, nlv_hi


def _lw_outs(le, q, k):
    return np.full(HM * le * q, NAN), np.full(HM * k, -1, dtype=np.int32), np.full(HM * k, NAN), np.full(HM * k, NAN)


def lwplsr_predict(L, ctx, loc, mat, out):
    d, p, q, dd, k, hi = _lw_args()
    x, y, zt, zq, xq = mat(d["X"]), mat(d["Y"][:, :q]), mat(d["X"][:, :dd]), mat(d["Q"][:, :dd]), mat(d["Q"])
    pred, ind, dist, w = _lw_outs(hi + 1, q, k)
    ctx.check(L.jch_lwplsr_predict(ctx._h, loc, x.ptr, HN, p, x.ld, y.ptr, q, y.ld, zt.ptr, zt.ld, zq.ptr, zq.ld, dd, xq.ptr, HM, xq.ld, k, 2.0, 1e-4, 0, 0, hi,
                                   vec(pred), ind.ctypes.data, vec(dist), vec(w)))
    return [x, y, zt, zq, xq], [pred, ind, dist, w]


def lwplsr_prepared(L, ctx, loc, mat, out):
    d, p, q, dd, k, hi = _lw_args()
    x, y, zt, zq, xq = mat(d["X"]), mat(d["Y"][:, :q]), mat(d["X"][:, :dd]), mat(d["Q"][:, :dd]), mat(d["Q"])
    pred, ind, dist, w = _lw_outs(hi + 1, q, k)
    model = C.c_void_p()
    ctx.check(L.jch_lwplsr_prepare(ctx._h, loc, x.ptr, HN, p, x.ld, y.ptr, q, y.ld, zt.ptr, zt.ld, dd, C.byref(model)))
    try:
        ctx.check(L.jch_lwplsr_predict_prepared(ctx._h, model, loc, zq.ptr, zq.ld, xq.ptr, HM, xq.ld, k, 2.0, 1e-4, 0, 0, hi, vec(pred), ind.ctypes.data, vec(dist), vec(w)))
    finally:
        L.jch_lwplsr_release(ctx._h, model)
    return [x, y, zt, zq, xq], [pred, ind, dist, w]


def xtdx(L, ctx, loc, mat, out):
    x, G, mu = mat(_data()["X"]), np.full(HP * HP, NAN), np.full(HP, NAN)
    ctx.check(L.jch_xtdx(ctx._h, loc, x.ptr, HN, HP, x.ld, None, None, 0, None, vec(G), vec(mu)))
    return [x], [G, mu]


def pca_fit(L, ctx, loc, mat, out):
    d, A, n, q = _data(), 2, HN, 2
    x, y = mat(d["X"]), mat(d["Y"])
    T, wn = out(n, A, True), out(n, 1, True)
    P, sv, eig, xm, xs, ss, cv, ym, xty, res = (np.full(HP * A, NAN), np.full(A, NAN), np.full(A, NAN), np.full(HP, NAN), np.full(HP, NAN), np.full(1, NAN), np.full(HP, NAN),
                                                np.full(q, NAN), np.full(HP * q, NAN), np.full(A, NAN))
    nit, got, conv = _i32(), _i32(), _i32()
    ctx.check(L.jch_pca_fit(ctx._h, loc, x.ptr, n, HP, x.ld, None, y.ptr, q, y.ld, A, 0, 1e-9, 200, T.ptr, vec(P), vec(sv), vec(eig), vec(xm), vec(xs), wn.ptr, vec(ss), vec(cv),
                            vec(ym), vec(xty), C.byref(nit), vec(res), C.byref(got), C.byref(conv)))
    return [x, y], [T.get(A), P, sv, eig, xm, wn.get(1), ss, cv, ym, xty, np.array([nit.value, got.value, conv.value])]


ROUTES = dict(occ=dict(jch_row_resid_ss=row_resid_ss), stah=dict(jch_col_median_mad=col_median_mad, jch_stah=stah),
              samp=dict(jch_farthest_pair=farthest_pair, jch_maxmin_select=maxmin_select), kde=dict(jch_kde_dens=kde_dens),
              knn=dict(jch_knn_wmean=knn_wmean, jch_knn_search=knn_search), dkplsr=dict(jch_kernel_gram=kernel_gram, jch_dkplsr=dkplsr), kplsr=dict(jch_kplsr=kplsr),
              kpca=dict(jch_kpca_fit=kpca), krr=dict(jch_krr_fit=krr), lwplsr=dict(jch_lwplsr_predict=lwplsr_predict, jch_lwplsr_predict_prepared=lwplsr_prepared),
              pca=dict(jch_xtdx=xtdx, jch_pca_fit=pca_fit))
