"""jch_row_resid_ss and occsd / occod / occsdod on the GPU: the primitive through the C ABI against the extended-precision restatement under the
static bound (test_occ_static.resid_ss_bound), the models against the literal numpy restatements of src/occsd.jl, src/occod.jl, src/occsdod.jl
and src/xfit.jl run on the downloaded model arrays."""
import dataclasses
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_kpca_static import np_kpca_transform  # noqa: E402
from test_occ_static import (OCC_NLV, PRIM_SHAPES, comparable_rows, np_occod, np_occod_predict, np_occsd, np_occsd_predict, np_occsdod,  # noqa: E402
                             np_occsdod_predict, np_transform, np_xfit, np_xresid, occ_data, prim_inputs, resid_ss_bound, resid_ss_longdouble)


@pytest.fixture(scope="module")
def J():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import jchemo_hip
    return jchemo_hip


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


# ---------------------------------------------------------------------------------- jch_row_resid_ss through the C ABI
SENT = 7.0


def _dev_colmajor(A, ld, offset):
    """A device copy of A with leading dimension ld whose first element sits `offset` doubles behind an allocation's start; sentinels elsewhere."""
    n, c = A.shape
    buf = torch.full((offset + ld * max(c, 1),), SENT, dtype=torch.float64, device="cuda:0")
    V = buf[offset:offset + ld * c].view(c, ld).t()
    V[:n].copy_(torch.as_tensor(np.array(A), device="cuda:0"))
    return V, buf.data_ptr() + 8 * offset, ld


def _layouts(A):
    """(aligned with an even ld, one double off with an odd ld)."""
    n = A.shape[0]
    return _dev_colmajor(A, n + 2 + n % 2, 0), _dev_colmajor(A, n + 1 + n % 2, 1)


def _call(J, ctx, loc, xa, m, p, ldx, shift, za, k, ldz, B):
    """out (m) as a host array; the entry behind out[m] must keep its sentinel."""
    lib = J.load()
    sa = None if shift is None else shift.ctypes.data
    ba = B.ctypes.data if k else None
    if loc == 0:
        out = np.full(m + 1, SENT)
        ctx.check(lib.jch_row_resid_ss(ctx._h, 0, xa, m, p, ldx, sa, za if k else None, k, ldz, ba, p, out.ctypes.data))
        assert out[m] == SENT
        return out[:m].copy()
    od = torch.full((m + 2,), SENT, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.check(lib.jch_row_resid_ss(ctx._h, 1, xa, m, p, ldx, sa, za if k else None, k, ldz, ba, p, od.data_ptr() + 8))   # out itself 8-byte aligned only
    o = _host(od)
    assert o[0] == SENT and o[m + 1] == SENT
    return o[1:m + 1].copy()


def _all_runs(J, ctx, X, shift, Z, B):
    """The same call as host data and as device data in every combination of (aligned, even ld) / (one double off, odd ld) for X and for Z.  Checks
    that X and Z come back unchanged and that the sentinels behind row m of every column are untouched; returns the results."""
    m, p = X.shape
    k = Z.shape[1]
    X0, Z0 = X.copy(), Z.copy()
    runs = [_call(J, ctx, 0, X.ctypes.data, m, p, m, shift, Z.ctypes.data, k, m, B)]
    assert np.array_equal(X, X0, equal_nan=True) and np.array_equal(Z, Z0, equal_nan=True)
    xl = _layouts(X)
    zl = _layouts(Z) if k else [(None, None, 0)]
    for xv, xa, ldx in xl:
        for zv, za, ldz in zl:
            runs.append(_call(J, ctx, 1, xa, m, p, ldx, shift, za, k, ldz, B))
    for xv, _, _ in xl:
        assert np.array_equal(_host(xv[:m]), X0, equal_nan=True) and torch.all(xv[m:] == SENT)
    for zv, _, _ in (zl if k else []):
        assert np.array_equal(_host(zv[:m]), Z0, equal_nan=True) and torch.all(zv[m:] == SENT)
    return runs


@pytest.mark.parametrize("m,p,k", PRIM_SHAPES)
def test_row_resid_ss_against_the_longdouble_restatement(J, m, p, k):
    ctx = J.Context(0)
    X, shift, Z, B = prim_inputs(m, p, k)
    ref = resid_ss_longdouble(X, shift, Z, B)
    bound = resid_ss_bound(X, shift, Z, B)
    runs = _all_runs(J, ctx, X, shift, Z, B)
    err = np.abs(np.asarray(runs[0] - ref, dtype=np.float64))
    print(f"row_resid_ss m={m} p={p} k={k}: max err / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(err <= bound)
    for r in runs[1:]:                                                       # host / device, aligned / unaligned X and Z: the same bits
        assert np.array_equal(r, runs[0])
    ctx.close()


def test_row_resid_ss_nan_stays_in_its_row(J):
    ctx = J.Context(0)
    m, p, k = 257, 33, 25
    X, shift, Z, B = prim_inputs(m, p, k)
    base = _all_runs(J, ctx, X, shift, Z, B)[0]
    i, j, i2, l = 70, 20, 201, 13
    X[i, j] = np.nan
    Z[i2, l] = np.nan
    for got in _all_runs(J, ctx, X, shift, Z, B):
        keep = np.ones(m, dtype=bool); keep[[i, i2]] = False
        assert np.isnan(got[i]) and np.isnan(got[i2])
        assert np.array_equal(got[keep], base[keep])                          # every other entry keeps its bits
    ctx.close()


@pytest.mark.parametrize("m,p", [(65, 17), (300, 500)])
def test_row_resid_ss_without_shift_and_scores_is_the_row_sum_of_squares(J, m, p):
    ctx = J.Context(0)
    X, _, _, _ = prim_inputs(m, p, 0)
    Z, B = np.zeros((m, 0), order="F"), np.zeros((p, 0), order="F")
    runs = _all_runs(J, ctx, X, None, Z, B)
    err = np.abs(np.asarray(runs[0] - resid_ss_longdouble(X, None, None, None), dtype=np.float64))
    bound = resid_ss_bound(X, None, None, None)
    print(f"row_resid_ss m={m} p={p} plain: max err / bound = {float(np.max(err / bound)):.3g}")
    assert np.all(err <= bound)
    for r in runs[1:]:
        assert np.array_equal(r, runs[0])
    ctx.close()


# ---------------------------------------------------------------------------------- the models
@pytest.fixture(scope="module")
def fits(J):
    """The models of the issue, fitted once on the GPU from host data, each with its downloaded arrays."""
    X, Y, Xnew, w = occ_data()
    ctx = J.Context(0)
    out = dict(X=X, Xnew=Xnew, ctx=ctx, models={})
    fms = dict(pcasvd=J.pcasvd(X, nlv=OCC_NLV, ctx=ctx), plskern=J.plskern(X, Y, nlv=OCC_NLV, ctx=ctx), plskern_scal=J.plskern(X, Y, nlv=OCC_NLV, scal=True, ctx=ctx),
               plskern_w=J.plskern(X, Y, w, nlv=OCC_NLV, ctx=ctx), kpca=J.kpca(X, nlv=OCC_NLV, kern="krbf", gamma=0.1, ctx=ctx))
    for name, fm in fms.items():
        if name == "kpca":
            arr = dict(T=_host(fm.T), X=_host(fm.X), P=_host(fm.P), D=_host(fm.weights), vtot=_host(fm.vtot).reshape(-1), xscales=fm.xscales, kern=fm.kern, dots=fm.dots)
        else:
            arr = dict(T=_host(fm.T), P=np.asarray(fm.P), R=np.asarray(fm.P if name == "pcasvd" else fm.R), xmeans=np.asarray(fm.xmeans), xscales=np.asarray(fm.xscales))
        out["models"][name] = (fm, arr)
    yield out
    ctx.close()


def _cm(J, a):
    a = np.asarray(a)
    t = J.colmajor_empty(a.shape[0], a.shape[1], "cuda:0")
    t.copy_(torch.as_tensor(a, device="cuda:0"))
    return t


def _dev_model(J, fm):
    """The same model with what is n-sized on the device."""
    kw = dict(T=_cm(J, fm.T), weights=torch.as_tensor(np.asarray(fm.weights), device="cuda:0"))
    if type(fm).__name__ == "Kpca":
        kw.update(X=_cm(J, fm.X), P=_cm(J, fm.P), vtot=torch.as_tensor(np.asarray(fm.vtot), device="cuda:0"), D=kw["weights"])
    return dataclasses.replace(fm, **kw)


def _close(got, ref, tol, what):
    got, ref = _host(got), np.asarray(ref)
    err = float(np.max(np.abs(got - ref) / np.abs(ref)))
    assert err <= tol, (what, err)


def _check_table(got, ref, dtrain, sfx=""):
    """d and gh within 1e-9 relative, dstand within 2e-9; pval on the comparable rows, of which at most 1 % may be missing."""
    _close(got["d" + sfx], ref["d" + sfx], 1e-9, "d" + sfx)
    _close(got["dstand" + sfx], ref["dstand" + sfx], 2e-9, "dstand" + sfx)
    if "gh" + sfx in ref:
        _close(got["gh" + sfx], ref["gh" + sfx], 1e-9, "gh" + sfx)
    keep = comparable_rows(ref["dstand" + sfx], ref["d" + sfx], dtrain)
    assert (~keep).mean() <= 0.01
    assert np.array_equal(_host(got["pval" + sfx])[keep], ref["pval" + sfx][keep])
    return keep


def _check_pred(got, ref_pred, ref_dstand, keep=None):
    p = _host(got)
    assert p.dtype == np.int64 and p.shape == ref_pred.shape
    ok = np.abs(ref_dstand - 1) > 1e-7
    if keep is not None:
        ok &= keep
    assert (~ok).mean() <= 0.01
    assert np.array_equal(p[ok], ref_pred[ok])


def _same_bits_on_device(host_tab, dev_tab):
    assert set(host_tab) == set(dev_tab)
    for name, col in dev_tab.items():
        assert isinstance(col, torch.Tensor) and col.is_cuda, name                     # the device results live on the device
        assert np.array_equal(_host(col), _host(host_tab[name])), name                 # ... and agree with the host run to the bit


MODELS = ["pcasvd", "plskern", "plskern_scal", "plskern_w", "kpca"]


@pytest.mark.parametrize("typc", ["mad", "q"])
@pytest.mark.parametrize("name", MODELS)
def test_occsd_parity_and_predict(J, fits, name, typc):
    fm, arr = fits["models"][name]
    Xnew, ctx = fits["Xnew"], fits["ctx"]
    fmd = _dev_model(J, fm)
    Xd = _cm(J, Xnew)
    for nlv in (None, 1, 3, OCC_NLV + 4):                                              # above the model's: clamps
        ref = np_occsd(arr["T"], nlv, typc)
        got = J.occsd(fm, nlv=nlv, typc=typc, ctx=ctx)
        assert got.nlv == ref["nlv"] and isinstance(got.d["d"], np.ndarray)
        _close(np.array([got.cutoff]), np.array([ref["cutoff"]]), 1e-9, "cutoff")
        assert np.max(np.abs(got.Sinv - ref["Sinv"])) <= 1e-9 * np.abs(ref["Sinv"]).max()
        _check_table(got.d, ref["d"], ref["dtrain"])
        assert np.array_equal(_host(got.e_cdf), np.sort(_host(got.d["d"])))
        k = ref["nlv"]
        Tnew = np_kpca_transform(arr, Xnew, k) if name == "kpca" else np_transform(arr, Xnew, k)
        rp = np_occsd_predict(ref, Tnew)
        gp = J.predict(got, Xnew, ctx=ctx)
        keep = _check_table(gp.d, rp["d"], ref["dtrain"])
        _check_pred(gp.pred, rp["pred"], rp["d"]["dstand"])
        if nlv is None and name != "kpca":
            assert rp["pred"].any() and not rp["pred"].all()                            # both classes occur
        # a device tensor in: every m-sized result on the device, the same bits
        gd = J.occsd(fmd, nlv=nlv, typc=typc, ctx=ctx)
        assert gd.cutoff == got.cutoff and np.array_equal(gd.Sinv, got.Sinv)
        _same_bits_on_device(got.d, gd.d)
        assert gd.e_cdf.is_cuda
        gpd = J.predict(gd, Xd, ctx=ctx)
        _same_bits_on_device(gp.d, gpd.d)
        assert gpd.pred.is_cuda and gpd.pred.dtype == torch.int64 and np.array_equal(_host(gpd.pred), gp.pred)


@pytest.mark.parametrize("typc", ["mad", "q"])
@pytest.mark.parametrize("name", MODELS[:4])
def test_occod_parity_and_predict(J, fits, name, typc):
    fm, arr = fits["models"][name]
    X, Xnew, ctx = fits["X"], fits["Xnew"], fits["ctx"]
    fmd = _dev_model(J, fm)
    Xtd, Xd = _cm(J, X), _cm(J, Xnew)
    for nlv in (None, 0, 1, 3, OCC_NLV + 4):
        ref = np_occod(arr, X, nlv, typc)
        got = J.occod(fm, X, nlv=nlv, typc=typc, ctx=ctx)
        assert got.nlv == ref["nlv"] and isinstance(got.d["d"], np.ndarray)
        _close(np.array([got.cutoff]), np.array([ref["cutoff"]]), 1e-9, "cutoff")
        _check_table(got.d, ref["d"], ref["dtrain"])
        rp = np_occod_predict(ref, Xnew)
        gp = J.predict(got, Xnew, ctx=ctx)
        _check_table(gp.d, rp["d"], ref["dtrain"])
        _check_pred(gp.pred, rp["pred"], rp["d"]["dstand"])
        assert rp["pred"][-10:].all() and not rp["pred"].all()                          # both classes occur
        gd = J.occod(fmd, Xtd, nlv=nlv, typc=typc, ctx=ctx)
        assert gd.cutoff == got.cutoff
        _same_bits_on_device(got.d, gd.d)
        gpd = J.predict(gd, Xd, ctx=ctx)
        _same_bits_on_device(gp.d, gpd.d)
        assert gpd.pred.is_cuda and np.array_equal(_host(gpd.pred), gp.pred)


@pytest.mark.parametrize("typc", ["mad", "q"])
@pytest.mark.parametrize("name", MODELS[:4])
def test_occsdod_parity_and_predict(J, fits, name, typc):
    fm, arr = fits["models"][name]
    X, Xnew, ctx = fits["X"], fits["Xnew"], fits["ctx"]
    fmd = _dev_model(J, fm)
    Xtd, Xd = _cm(J, X), _cm(J, Xnew)
    for nlv_sd, nlv_od in ((None, None), (3, 5), (OCC_NLV + 4, 1)):                       # nlv_sd != nlv_od
        ref = np_occsdod(arr, X, nlv_sd, nlv_od, typc)
        got = J.occsdod(fm, X, nlv_sd=nlv_sd, nlv_od=nlv_od, typc=typc, ctx=ctx)
        assert list(got.d) == ["d_sd", "dstand_sd", "pval_sd", "gh_sd", "d_od", "dstand_od", "pval_od", "dstand"]
        assert (got.fm_sd.nlv, got.fm_od.nlv) == (ref["fm_sd"]["nlv"], ref["fm_od"]["nlv"])
        assert list(got.fm_sd.d) == ["d", "dstand", "pval", "gh"]                       # not renamed in place
        _check_table(got.d, ref["d"], ref["fm_sd"]["dtrain"], "_sd")
        _check_table(got.d, ref["d"], ref["fm_od"]["dtrain"], "_od")
        _close(got.d["dstand"], ref["d"]["dstand"], 2e-9, "dstand")
        rp = np_occsdod_predict(ref, Xnew)
        gp = J.predict(got, Xnew, ctx=ctx)
        _check_table(gp.d, rp["d"], ref["fm_sd"]["dtrain"], "_sd")
        _check_table(gp.d, rp["d"], ref["fm_od"]["dtrain"], "_od")
        _close(gp.d["dstand"], rp["d"]["dstand"], 2e-9, "dstand")
        _check_pred(gp.pred, rp["pred"], rp["d"]["dstand"])
        assert rp["pred"][-10:].all() and not rp["pred"].all()
        gd = J.occsdod(fmd, Xtd, nlv_sd=nlv_sd, nlv_od=nlv_od, typc=typc, ctx=ctx)
        _same_bits_on_device(got.d, gd.d)
        gpd = J.predict(gd, Xd, ctx=ctx)
        _same_bits_on_device(gp.d, gpd.d)
        assert gpd.pred.is_cuda and np.array_equal(_host(gpd.pred), gp.pred)


def test_xfit_and_xresid_take_a_pca_and_a_pcr(J, fits):
    X, Xnew, ctx = fits["X"], fits["Xnew"], fits["ctx"]
    Y = occ_data()[1]
    pca, arr = fits["models"]["pcasvd"]
    pcr = J.pcr(X, Y, nlv=OCC_NLV, scal=True, ctx=ctx)
    arr_pcr = dict(T=_host(pcr.fm_pca.T), P=pcr.fm_pca.P, R=pcr.fm_pca.P, xmeans=pcr.fm_pca.xmeans, xscales=pcr.fm_pca.xscales)
    for fm, a in ((pca, arr), (pcr, arr_pcr)):
        for nlv in (None, 0, 2, OCC_NLV + 4):
            for fn, ref in ((J.xfit, np_xfit(a, Xnew, nlv)), (J.xresid, np_xresid(a, Xnew, nlv))):
                got = fn(fm, Xnew, nlv=nlv, ctx=ctx)
                assert isinstance(got, np.ndarray) and got.shape == ref.shape
                # deliberately relative to the largest entry, not entry by entry: a residual matrix has entries arbitrarily close to zero
                assert np.max(np.abs(got - ref)) <= 1e-9 * np.max(np.abs(ref)), (type(fm).__name__, nlv, fn.__name__)
    gd = J.xresid(pca, _cm(J, Xnew), nlv=3, ctx=ctx)
    assert gd.is_cuda and np.array_equal(_host(gd), J.xresid(pca, Xnew, nlv=3, ctx=ctx))


# ---------------------------------------------------------------------------------- the three routes of the C entries (tests/host_routes.py)
@pytest.mark.parametrize("entry", sorted(__import__("host_routes").ROUTES["occ"]))
def test_host_arrays_padded_and_unpadded_give_the_bits_of_the_device_route(entry):
    """Device buffers, host arrays with ld == rows and with ld = rows + 3 between NaN guards: equal bytes, NaN padding kept, inputs unchanged."""
    import host_routes as HR
    HR.three_routes(HR.ROUTES["occ"][entry])
