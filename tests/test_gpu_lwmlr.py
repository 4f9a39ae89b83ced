"""jch_knn_wls and lwmlr / lwmlr_s / lwmlrda / lwmlrda_s on the GPU, against the longdouble restatement of tests/test_lwmlr_static.py inside the
error bound derived in DESIGN.md §23 (checked there between the float64 and the longdouble restatement first).  Every comparison prints its
largest measured / allowed ratio before it asserts."""
import importlib
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_lwmlr_static import CASES, LD, case, clustered, max_ratio, np_locw_mlrda, np_wdist_clamped, wls_reference  # noqa: E402

SENT, ISENT = 7.25, -77
H, TOL = 2.0, 1e-4


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


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def dev(a):
    """A column-major device copy of a host matrix."""
    a = np.asarray(a)
    t = torch.empty((a.shape[1], a.shape[0]), dtype=torch.float64, device="cuda:0").t()
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def _dev_padded(A, ld, offset):
    """A device copy of A with leading dimension ld > rows that starts `offset` doubles behind an allocation's start: (address, ld)."""
    n, c = A.shape
    buf = torch.full((offset + ld * c,), SENT, dtype=torch.float64, device="cuda:0")
    V = buf[offset:offset + ld * c].view(c, ld).t()
    V[:n].copy_(torch.as_tensor(np.array(A), device="cuda:0"))
    return buf, buf.data_ptr() + 8 * offset, ld


def run_wls(J, ctx, X, Y, Xq, ind, w, mode):
    """(pred, info) as host arrays.  "host": the Python primitive on numpy arrays; "dev": the C ABI on device arrays with ld > rows, an offset
    start, and sentinels in front of and behind pred and info that must survive."""
    if mode == "host":
        pred, info = J.knn_wls(X, Y, Xq, ind, w, info=True, ctx=ctx)
        assert isinstance(pred, np.ndarray) and pred.shape == (Xq.shape[0], Y.shape[1]) and info.dtype == np.int32
        return pred, info
    n, d = X.shape
    q, m, k = Y.shape[1], Xq.shape[0], ind.shape[1]
    keep = [_dev_padded(X, n + 3, 1), _dev_padded(Y, n + 5, 3), _dev_padded(Xq, m + 1, 5)]
    di = torch.as_tensor(np.ascontiguousarray(ind, dtype=np.int32), device="cuda:0")
    dw = torch.as_tensor(np.ascontiguousarray(w), device="cuda:0")
    pbuf = torch.full((m * q + 4,), SENT, dtype=torch.float64, device="cuda:0")
    ibuf = torch.full((m + 4,), ISENT, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ctx.check(J.load().jch_knn_wls(ctx._h, 1, keep[0][1], n, d, keep[0][2], keep[1][1], q, keep[1][2], keep[2][1], m, keep[2][2], di.data_ptr(),
                                   dw.data_ptr(), k, pbuf.data_ptr() + 16, ibuf.data_ptr() + 8))
    ctx.synchronize()
    pb, ib = host(pbuf), host(ibuf)
    assert (pb[:2] == SENT).all() and (pb[-2:] == SENT).all() and (ib[:2] == ISENT).all() and (ib[-2:] == ISENT).all()
    for (buf, _, ld), A in zip(keep, (X, Y, Xq)):                       # the inputs and the padding between their columns are untouched
        full = host(buf)
        assert (full == SENT).sum() >= full.size - A.size
    return pb[2:-2].reshape(q, m).T.copy(), ib[2:-2].copy()


def check_against(J, ctx, X, Y, Xq, ind, w, mode, label, ref=None):
    ref, rinfo, bound = ref if ref is not None else wls_reference(X, Y, Xq, ind, w)
    pred, info = run_wls(J, ctx, X, Y, Xq, ind, w, mode)
    assert np.array_equal(info, rinfo), (label, info, rinfo)
    ratio = max_ratio(pred, ref, bound)
    print(f"{label} [{mode}]: measured / allowed {ratio:.3g} (largest error {np.nanmax(np.abs(pred - ref), initial=0.0):.2e}, info counts {np.bincount(info, minlength=3)})")
    assert ratio <= 1.0, (label, ratio)
    return pred, info


# ---------------------------------------------------------------------------------- a. the primitive
@pytest.mark.parametrize("mode", ["host", "dev"])
@pytest.mark.parametrize("idx", range(len(CASES)))
def test_primitive_at_the_five_shapes(J, ctx, idx, mode):
    c = case(idx)
    check_against(J, ctx, c["X"], c["Y"], c["Xq"], c["ind"], c["w"], mode, f"case {CASES[idx]}", ref=c["ref"])


def lists_for(X, Xq, k):
    """Brute-force neighbour lists in float64 and their clamped weights."""
    d2 = ((Xq[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    ind = np.argsort(d2, axis=1, kind="stable")[:, :k].astype(np.int32)
    dist = np.sqrt(np.take_along_axis(d2, ind, axis=1))
    return ind, np.stack([np_wdist_clamped(r, H, TOL) for r in dist])


# (n, d, q, k, m): k = 1 (q = 1: the shortcut; q = 5: k <= d), k around the wave size and beyond one pass of the workgroup, d = 1, q = 1 and 5,
# m = 1, and more queries than the grid holds workgroups (8 per CU) so that the grid-stride loop runs
BOUNDARY = [(50, 3, 1, 1, 5), (50, 3, 5, 1, 5), (200, 3, 1, 63, 6), (200, 3, 5, 64, 6), (200, 1, 1, 65, 6), (400, 6, 1, 257, 4), (120, 2, 5, 9, 1),
            (300, 2, 1, 6, 2300)]


@pytest.mark.parametrize("shape", BOUNDARY, ids=lambda s: "n%d-d%d-q%d-k%d-m%d" % s)
def test_primitive_at_the_boundary_shapes(J, ctx, shape):
    n, d, q, k, m = shape
    X, Y, _, Xq = clustered(n, d, q, m, 900 + k + q)
    ind, w = lists_for(X, Xq, k)
    _, info = check_against(J, ctx, X, Y, Xq, ind, w, "dev" if m > 1000 else "host", f"boundary {shape}")
    if k == 1:
        assert (info == (2 if q == 1 else 1)).all()
    else:
        assert (info == 0).all()


def test_slabs_beyond_the_lds_and_just_under_the_threshold(J, ctx):
    n, d, q, m = 1000, 24, 2, 3
    lds_max = importlib.import_module("jchemo_hip.lwmlr").WLS_LDS_MAX
    k_under = max(k for k in range(600, 800) if J.knn_wls_lds_bytes(k, d, q) <= lds_max)
    assert J.knn_wls_lds_bytes(900, d, q) > 187000 > lds_max >= J.knn_wls_lds_bytes(k_under, d, q) > lds_max - 8 * (d + q + 3)
    X, Y, _, Xq = clustered(n, d, q, m, 4242)
    for k, mode in ((900, "host"), (900, "dev"), (k_under, "dev"), (k_under + 1, "host")):
        ind, w = lists_for(X, Xq, k)
        _, info = check_against(J, ctx, X, Y, Xq, ind, w, mode, f"k = {k} ({J.knn_wls_lds_bytes(k, d, q)} bytes of slab)")
        assert (info == 0).all()


def test_workspace_instantiation_beside_the_lds_one_at_199_neighbours(J, ctx):
    """The same rows, responses, queries and k = 199, m = 3 at two widths of X: its first 91 columns (d + q = 92: a slab of 152 640 bytes, in LDS)
    and all 96 (d + q = 97: 160 720 bytes, beyond WLS_LDS_MAX = 153 600: one piece of the workspace per workgroup, the <false> instantiation).
    Both sizes are csrc/lwmlr.hip `wls_slab_doubles` x 8 as the Python mirror restates it; the threshold itself lies between 92 and 93 columns.
    Each run against the longdouble restatement inside the bound of DESIGN.md §23, from host arrays and from device arrays."""
    n, q, m, k = 260, 1, 3, 199
    lds_max = importlib.import_module("jchemo_hip.lwmlr").WLS_LDS_MAX
    assert J.knn_wls_lds_bytes(k, 91, q) == 152640 <= lds_max == 153600 < J.knn_wls_lds_bytes(k, 96, q) == 160720
    X, Y, _, Xq = clustered(n, 96, q, m, 5151)
    for d in (91, 96):
        Xd, Qd = np.asfortranarray(X[:, :d]), np.asfortranarray(Xq[:, :d])
        ind, w = lists_for(Xd, Qd, k)
        ref = wls_reference(Xd, Y, Qd, ind, w)
        for mode in ("host", "dev"):
            _, info = check_against(J, ctx, Xd, Y, Qd, ind, w, mode, f"d = {d} ({J.knn_wls_lds_bytes(k, d, q)} bytes of slab)", ref=ref)
            assert (info == 0).all()


def test_special_cases(J, ctx):
    """Disjoint hand-made neighbourhoods (query i owns the rows i k .. (i + 1) k - 1), so that a special case touches one query only."""
    rng = np.random.default_rng(77)
    d, k, m = 3, 10, 6
    n = m * k
    X = np.asfortranarray(rng.standard_normal((n, d)) + 2.0)
    Y1 = np.asfortranarray(1.0 + X @ rng.standard_normal((d, 1)) + 0.1 * rng.standard_normal((n, 1)))
    Y2 = np.asfortranarray(np.hstack([Y1, -Y1 + 0.2 * rng.standard_normal((n, 1))]))
    Xq = np.asfortranarray(rng.standard_normal((m, d)) + 2.0)
    ind = np.arange(n, dtype=np.int32).reshape(m, k)
    w = rng.uniform(0.2, 1.0, (m, k))
    for mode in ("host", "dev"):
        clean1, _ = check_against(J, ctx, X, Y1, Xq, ind, w, mode, "clean q = 1")
        clean2, _ = check_against(J, ctx, X, Y2, Xq, ind, w, mode, "clean q = 2")
        again, _ = run_wls(J, ctx, X, Y2, Xq, ind, w, mode)
        assert np.array_equal(again, clean2)                             # two runs: identical bits
        # the constant response: exact value, info 2; the neighbours of query 1 only
        Yc = Y1.copy(); Yc[ind[1], 0] = 2.5
        pred, info = run_wls(J, ctx, X, Yc, Xq, ind, w, mode)
        assert pred[1, 0] == 2.5 and info[1] == 2 and (np.delete(info, 1) == 0).all()
        assert np.array_equal(np.delete(pred, 1, axis=0), np.delete(clean1, 1, axis=0))
        # ... and for q > 1 there is no shortcut: a constant column is fitted (beta = 0 up to rounding)
        Yc2 = Y2.copy(); Yc2[ind[1], 0] = 2.5
        pred, info = check_against(J, ctx, X, Yc2, Xq, ind, w, mode, "constant column, q = 2")
        assert (info == 0).all() and abs(pred[1, 0] - 2.5) < 1e-13
        # a duplicated column in one neighbourhood: NaN row, info 1, the others untouched
        Xd = X.copy(); Xd[ind[2], 2] = Xd[ind[2], 0]
        pred, info = run_wls(J, ctx, Xd, Y2, Xq, ind, w, mode)
        assert np.isnan(pred[2]).all() and info[2] == 1 and (np.delete(info, 2) == 0).all()
        assert np.array_equal(np.delete(pred, 2, axis=0), np.delete(clean2, 2, axis=0))
        # a NaN in one training row poisons only the query that gathers it
        Xn = X.copy(); Xn[ind[3][4], 1] = np.nan
        pred, info = run_wls(J, ctx, Xn, Y2, Xq, ind, w, mode)
        assert np.isnan(pred[3]).all() and np.array_equal(np.delete(pred, 3, axis=0), np.delete(clean2, 3, axis=0))
        Yn = Y2.copy(); Yn[ind[3][4], 1] = np.nan                        # in Y: that response only
        pred, info = run_wls(J, ctx, X, Yn, Xq, ind, w, mode)
        assert np.isnan(pred[3, 1]) and np.array_equal(pred[:, 0], clean2[:, 0]) and np.array_equal(np.delete(pred, 3, axis=0), np.delete(clean2, 3, axis=0))
        Xqn = Xq.copy(); Xqn[4, 0] = np.nan                              # in a query
        pred, info = run_wls(J, ctx, X, Y2, Xqn, ind, w, mode)
        assert np.isnan(pred[4]).all() and np.array_equal(np.delete(pred, 4, axis=0), np.delete(clean2, 4, axis=0))
        # a row index outside [0, n): a NaN row, nothing read out of bounds
        for bad in (-1, n, 2 ** 31 - 1):
            ib = ind.copy(); ib[5, 7] = bad
            pred, info = run_wls(J, ctx, X, Y2, Xq, ib, w, mode)
            assert np.isnan(pred[5]).all() and np.array_equal(pred[:5], clean2[:5])
    # k <= d: every row NaN, info 1
    pred, info = run_wls(J, ctx, X, Y2, Xq, ind[:, :3], w[:, :3], "host")
    assert np.isnan(pred).all() and (info == 1).all()
    # bad arguments are JCH_EINVAL
    lib = J.load()
    assert lib.jch_knn_wls(ctx._h, 0, X.ctypes.data, n, d, n - 1, Y2.ctypes.data, 2, n, Xq.ctypes.data, m, m, ind.ctypes.data, w.ctypes.data, k,
                           clean2.ctypes.data, None) == J._lib.JCH_EINVAL
    assert lib.jch_knn_wls(ctx._h, 0, X.ctypes.data, n, d, n, Y2.ctypes.data, 2, n, Xq.ctypes.data, m, m, ind.ctypes.data, None, k,
                           clean2.ctypes.data, None) == J._lib.JCH_EINVAL
    assert lib.jch_knn_wls(ctx._h, 2, X.ctypes.data, n, d, n, Y2.ctypes.data, 2, n, Xq.ctypes.data, m, m, ind.ctypes.data, w.ctypes.data, 0,
                           clean2.ctypes.data, None) == J._lib.JCH_EINVAL


# ---------------------------------------------------------------------------------- b. the four models, end to end
MODEL = dict(n=260, d=6, m=40, k=35)


def model_data(classes):
    X, Y, yv, Xq = clustered(MODEL["n"], MODEL["d"], -3 if classes else 2, MODEL["m"], 311 + classes)
    return X, Y, yv, Xq


def put(a, where):
    return dev(a) if where == "device" else np.asfortranarray(a)


def check_lists(J, ctx, coords, Q, res, metric, k):
    """listnn / listd / listw are those of getknn and of jch_knn_search on the same space."""
    ind, dist = J.getknn(coords, Q, k=k, metric=metric, ctx=ctx)
    assert np.array_equal(host(ind), host(res.listnn)) and np.array_equal(host(dist), host(res.listd))
    if metric == "eucl":
        hnd = J.knn_prepare(coords, ctx)
        try:
            r = J.knn_search(hnd, coords.shape[0], Q, k, h=H, tol=TOL, want=("ind", "dist", "w"), ctx=ctx)
        finally:
            J.knn_release(hnd)
        assert np.array_equal(host(r["w"]), host(res.listw)) and np.array_equal(host(r["ind"]), host(res.listnn))
    w = host(res.listw)
    assert w.min() >= TOL and w.max() <= 1.0 and host(res.listnn).dtype == np.int32


def check_regression(J, ctx, coords, Y, Q, res, label):
    ref, rinfo, bound = wls_reference(host(coords), host(Y), host(Q), host(res.listnn), host(res.listw))
    assert (rinfo == 0).all()
    ratio = max_ratio(host(res.pred), ref, bound)
    print(f"{label}: measured / allowed {ratio:.3g}")
    assert ratio <= 1.0, (label, ratio)


def check_labels(J, ctx, coords, Yd, yv, Q, res, label):
    """Against the reference's `mlrda` on the LOCAL levels, in longdouble; queries whose two largest posteriors are closer than the bound are left out."""
    coords, Q, ind, w = host(coords), host(Q), host(res.listnn), host(res.listw)
    lab, gap = np_locw_mlrda(coords, yv, Q, ind, w, LD)
    _, _, bound = wls_reference(coords, Yd, Q, ind, w)
    skip = gap <= 2 * bound.max(axis=1)
    m = Q.shape[0]
    print(f"{label}: smallest top-two gap {gap.min():.2e}, largest bound {bound.max():.2e}, left out {int(skip.sum())} of {m}")
    assert skip.sum() <= 0.01 * m
    pred = np.asarray(res.pred)
    assert pred.shape == (m, 1) and isinstance(res.pred, np.ndarray)
    assert all(lab[i] == pred[i, 0] for i in range(m) if not skip[i] and lab[i] is not None)
    assert sum(l is None for l in lab) == 0


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("metric", ["eucl", "mahal"])
def test_lwmlr_and_lwmlrda(J, ctx, metric, where):
    X, Y, _, Xq = model_data(0)
    Xi, Yi, Qi = put(X, where), put(Y, where), put(Xq, where)
    fm = J.lwmlr(Xi, Yi, metric=metric, h=H, k=MODEL["k"], ctx=ctx)
    res = J.lwmlr_predict(fm, Qi, ctx=ctx)
    assert (where == "device") == torch.is_tensor(res.pred)
    check_lists(J, ctx, Xi, Qi, res, metric, MODEL["k"])
    check_regression(J, ctx, X, Y, Xq, res, f"lwmlr {metric} {where}")
    again = J.lwmlr_predict(fm, Qi, ctx=ctx)                              # the cached handle
    assert np.array_equal(host(again.pred), host(res.pred))
    X, Yd, yv, Xq = model_data(1)
    Xi, Qi = put(X, where), put(Xq, where)
    fd = J.lwmlrda(Xi, yv, metric=metric, h=H, k=MODEL["k"], ctx=ctx)
    rd = J.lwmlrda_predict(fd, Qi, ctx=ctx)
    check_lists(J, ctx, Xi, Qi, rd, metric, MODEL["k"])
    check_labels(J, ctx, X, Yd, yv, Xq, rd, f"lwmlrda {metric} {where}")


@pytest.mark.parametrize("reduc,psamp,samp,where", [("pca", 1, "sys", "host"), ("pls", 1, "sys", "device"), ("dkpls", 1, "sys", "host"),
                                                    ("pls", 0.5, "sys", "host"), ("pca", 0.5, "random", "host")])
def test_lwmlr_s(J, ctx, reduc, psamp, samp, where):
    X, Y, _, Xq = model_data(0)
    Xi, Yi, Qi = put(X, where), put(Y, where), put(Xq, where)
    fm = J.lwmlr_s(Xi, Yi, nlv=3, reduc=reduc, h=H, k=MODEL["k"], gamma=0.05, psamp=psamp, samp=samp, seed=3, ctx=ctx)
    assert tuple(fm.T.shape) == (MODEL["n"], 3)
    nfit = {"pca": lambda f: f.T, "pls": lambda f: f.T, "dkpls": lambda f: f.fm.T}[reduc](fm.fm).shape[0]
    assert nfit == int(round(psamp * MODEL["n"]))                          # psamp = 1: every row
    res = J.lwmlr_s_predict(fm, Qi, ctx=ctx)
    Tq = importlib.import_module("jchemo_hip.lwmlr")._transform(fm.fm, Qi, ctx)
    check_lists(J, ctx, fm.T, Tq, res, "eucl", MODEL["k"])
    check_regression(J, ctx, fm.T, Y, Tq, res, f"lwmlr_s {reduc} psamp = {psamp} {samp} {where}")


@pytest.mark.parametrize("reduc,psamp,samp,metric", [("pca", 1, "cla", "eucl"), ("pls", 1, "cla", "mahal"), ("dkpls", 1, "cla", "eucl"),
                                                     ("pls", 0.5, "cla", "eucl"), ("pca", 0.5, "random", "eucl")])
def test_lwmlrda_s(J, ctx, reduc, psamp, samp, metric):
    X, Yd, yv, Xq = model_data(1)
    fm = J.lwmlrda_s(X, yv, nlv=3, reduc=reduc, metric=metric, h=H, k=MODEL["k"], gamma=0.05, psamp=psamp, samp=samp, seed=3, ctx=ctx)
    assert tuple(fm.T.shape) == (MODEL["n"], 3)
    res = J.lwmlrda_s_predict(fm, Xq, ctx=ctx)
    Tq = importlib.import_module("jchemo_hip.lwmlr")._transform(fm.fm, Xq, ctx)
    check_lists(J, ctx, fm.T, Tq, res, metric, MODEL["k"])
    check_labels(J, ctx, fm.T, Yd, yv, Tq, res, f"lwmlrda_s {reduc} psamp = {psamp} {samp} {metric}")


def test_rank_deficient_neighbourhoods_warn_once_and_fall_back_to_the_vote(J, ctx):
    X, Y, _, Xq = model_data(0)
    fm = J.lwmlr(X, Y, h=H, k=MODEL["d"], ctx=ctx)                         # k <= d: every neighbourhood
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = J.lwmlr_predict(fm, Xq, ctx=ctx)
    assert [str(r.message) for r in rec if r.category is RuntimeWarning] == [f"lwmlr_predict: {MODEL['m']} of {MODEL['m']} neighbourhoods are rank-deficient; their predictions are NaN"]
    assert np.isnan(res.pred).all()
    X, Yd, yv, Xq = model_data(1)
    fd = J.lwmlrda(X, yv, h=H, k=MODEL["d"], ctx=ctx)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        rd = J.lwmlrda_predict(fd, Xq, ctx=ctx)
    assert sum(r.category is RuntimeWarning for r in rec) == 1
    want = J.knnda_predict(J.knnda(X, yv, h=H, k=MODEL["d"], ctx=ctx), Xq, ctx=ctx).pred      # no fit anywhere: the weighted vote of knnda
    assert np.array_equal(rd.pred, want)


# ---------------------------------------------------------------------------------- c. on a used ctx, behind a fit that promised reuse_x
@pytest.fixture(scope="module")
def used_ctx_models(J):
    other = J.Context(0)
    out = {}
    X, Y, _, Xq = model_data(0)
    Xc, Yd, yv, Xqc = model_data(1)
    for where in ("host", "device"):
        Xi, Yi, Qi, Xci, Qci = (put(a, where) for a in (X, Y, Xq, Xc, Xqc))
        ind, w = lists_for(X, Xq, MODEL["k"])
        models = {
            "knn_wls": (lambda c, Xi=Xi, Yi=Yi, Qi=Qi, ind=ind, w=w: J.knn_wls(Xi, Yi, Qi, ind, w, ctx=c)),
            "lwmlr": (lambda c, f=J.lwmlr(Xi, Yi, metric="mahal", h=H, k=MODEL["k"]), Qi=Qi: J.lwmlr_predict(f, Qi, ctx=c).pred),
            "lwmlr_s": (lambda c, f=J.lwmlr_s(Xi, Yi, nlv=3, h=H, k=MODEL["k"], ctx=other), Qi=Qi: J.lwmlr_s_predict(f, Qi, ctx=c).pred),
            "lwmlrda": (lambda c, f=J.lwmlrda(Xci, yv, h=H, k=MODEL["k"]), Qci=Qci: J.lwmlrda_predict(f, Qci, ctx=c).pred),
            "lwmlrda_s": (lambda c, f=J.lwmlrda_s(Xci, yv, nlv=3, reduc="pca", h=H, k=MODEL["k"], ctx=other), Qci=Qci: J.lwmlrda_s_predict(f, Qci, ctx=c).pred),
        }
        for name, call in models.items():
            out[name, where] = (call, host(call(other)))
    yield out
    other.close()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", ["knn_wls", "lwmlr", "lwmlr_s", "lwmlrda", "lwmlrda_s"])
def test_on_a_used_ctx_behind_a_fit_that_promised_reuse_x(name, where, used_ctx_models):
    """plskern(X) / the entry / plskern(X, reuse_x=True) on one ctx (tests/test_gpu_used_ctx.py, Part B): the entry's results equal those on a fresh
    ctx bit for bit, and the third fit equals the same fit on a fresh ctx.  jch_knn_wls reserves the kNN workspace only: behind the primitive alone
    the third fit does take the copy."""
    from test_gpu_used_ctx import reuse_sequence
    call, want = used_ctx_models[name, where]

    def intervener(c, Xi, state):
        if state != "before":
            assert np.array_equal(host(call(c)), want, equal_nan=True)
    taken = reuse_sequence(where, intervener)
    print(f"{name} [{where}]: the third fit took the row-major copy {taken} time(s)")
    if name == "knn_wls":
        assert taken == 1
