"""jch_col_median_mad, jch_stah and stah / occstah / predict on the GPU.  The selection is exact: medians and MADs are compared with `np.array_equal`
against the numpy restatements of the very same matrix (test_stah_static.np_colmed / np_colmad), for a host X and a device X in an aligned and an
unaligned layout, with both output locations.  The row maximum is compared bit for bit too (an identity projection is exact on the matrix cores);
the models against the literal restatements of src/stah.jl and src/occstah.jl within 1e-9 max(1, |ref|)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_occ import SENT, _host, _layouts  # noqa: E402
from test_occ_static import occ_data  # noqa: E402
from test_stah_static import STAH_A, stah_comparable_rows, np_colmad, np_colmed, np_occstah, np_occstah_predict, np_stah, stah_P  # noqa: E402

_CSRC = os.path.join(ROOT, "jchemo.jl_amd", "csrc")
CS_WG_ROWS = int(re.search(r"#define CS_WG_ROWS (\d+)", open(os.path.join(_CSRC, "colselect.hip")).read()).group(1))   # rows of a column one workgroup owns
ST_PANEL_MAXCOLS = int(re.search(r"#define ST_PANEL_MAXCOLS (\d+)", open(os.path.join(_CSRC, "stah.hip")).read()).group(1))   # widest panel of jch_stah


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


# ---------------------------------------------------------------------------------- jch_col_median_mad through the C ABI
def _cmm(J, ctx, loc, xa, n, p, ldx, out_loc, want_mad=True):
    """(med, mad or None) as host arrays; the entries around the p outputs must keep their sentinels."""
    lib = J.load()
    if out_loc == 0:
        med, mad = np.full(p + 2, SENT), np.full(p + 2, SENT)
        ctx.check(lib.jch_col_median_mad(ctx._h, loc, xa, n, p, ldx, med.ctypes.data + 8, mad.ctypes.data + 8 if want_mad else None, 0))
    else:
        md, dd = torch.full((p + 2,), SENT, dtype=torch.float64, device="cuda:0"), torch.full((p + 2,), SENT, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        ctx.check(lib.jch_col_median_mad(ctx._h, loc, xa, n, p, ldx, md.data_ptr() + 8, dd.data_ptr() + 8 if want_mad else None, 1))
        torch.cuda.synchronize()                                              # device to device: the call only enqueues
        med, mad = _host(md), _host(dd)
    assert med[0] == SENT and med[p + 1] == SENT and mad[0] == SENT and mad[p + 1] == SENT
    if not want_mad:
        assert np.all(mad == SENT)
    return med[1:p + 1].copy(), (mad[1:p + 1].copy() if want_mad else None)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _check_all_runs(J, ctx, X):
    """Host X and device X in both layouts, both output locations, the med-only form: every run equals the restatement exactly and all runs carry the
    same bits; X and the sentinels behind row n of every column come back untouched."""
    n, p = X.shape
    X0 = X.copy()
    ref_med, ref_mad = np_colmed(X), np_colmad(X)
    runs = [_cmm(J, ctx, 0, X.ctypes.data, n, p, n, 0), _cmm(J, ctx, 0, X.ctypes.data, n, p, n, 1)]
    layouts = _layouts(X)
    for xv, xa, ldx in layouts:
        runs.append(_cmm(J, ctx, 1, xa, n, p, ldx, 0))
        runs.append(_cmm(J, ctx, 1, xa, n, p, ldx, 1))
    runs.append(_cmm(J, ctx, 1, layouts[1][1], n, p, layouts[1][2], 1))       # once more: two runs give identical bits
    for med, mad in runs:
        assert np.array_equal(med, ref_med, equal_nan=True), (n, p, med, ref_med)
        assert np.array_equal(mad, ref_mad, equal_nan=True), (n, p, mad, ref_mad)
        assert np.array_equal(_bits(med), _bits(runs[0][0])) and np.array_equal(_bits(mad), _bits(runs[0][1]))
    for loc, xa, ldx in ((0, X.ctypes.data, n), (1, layouts[0][1], layouts[0][2])):
        for out_loc in (0, 1):
            med, none = _cmm(J, ctx, loc, xa, n, p, ldx, out_loc, want_mad=False)
            assert none is None and np.array_equal(_bits(med), _bits(runs[0][0]))
    assert np.array_equal(X, X0, equal_nan=True)
    for xv, _, _ in layouts:
        assert np.array_equal(_host(xv[:n]), X0, equal_nan=True) and torch.all(xv[n:] == SENT)


def _contents(n, p, rng):
    """The matrices of one shape, by name."""
    out = {}
    out["normal"] = rng.standard_normal((n, p))
    out["ties"] = np.round(rng.standard_normal((n, p)), 1)                    # ties straddle the median
    A = rng.standard_normal((n, p)); A[:, 0] = 3.25
    out["constant column"] = A                                               # MAD 0
    out["low bits"] = np.stack([1.0 + rng.permutation(n) * 2.0 ** -50 for _ in range(p)], axis=1)   # the keys agree in their top 40 bits
    A = rng.standard_normal((n, p))
    kind = rng.integers(0, 5, size=(n, p))
    A[kind == 0] = 0.0
    A[kind == 1] = -0.0
    sub = rng.integers(-50, 51, size=(n, p)) * 2.0 ** -1070                   # subnormals on a grid whose halves and sums are exact
    A[kind == 2] = sub[kind == 2]
    out["signed zeros and subnormals"] = A
    if n >= 2:
        A = rng.standard_normal((n, p)); A[0, :] = np.inf; A[n - 1, :] = -np.inf
        out["infinities in the tails"] = A
    A = np.abs(rng.standard_normal((n, p))) + 0.5
    A[: n // 2] *= -1                                                        # an even n: the two middle ranks differ in the sign bit
    out["sign change at the median"] = rng.permuted(A, axis=0)
    if p >= 2:
        A = rng.standard_normal((n, p)); A[n // 3, 1] = np.nan                # one NaN in one column: that column alone gives NaN
        out["one NaN"] = A
    return {k: np.asfortranarray(v) for k, v in out.items()}


# (n, p): the smallest; around a wave and the 4-load unrolling of a workgroup; one row below, at and above the CS_WG_ROWS rows one workgroup owns; a column
# that spans many workgroups; many columns per workgroup
CMM_SHAPES = [(1, 1), (2, 1), (3, 2), (63, 3), (64, 3), (65, 3), (1023, 2), (1024, 2), (1025, 2), (CS_WG_ROWS - 1, 2), (CS_WG_ROWS, 2), (CS_WG_ROWS + 1, 2),
              (200001, 3), (5, 300)]


@pytest.mark.parametrize("n,p", CMM_SHAPES)
def test_col_median_mad_is_exact(J, ctx, n, p):
    rng = np.random.default_rng(100 * n + p)
    for name, X in _contents(n, p, rng).items():
        if name == "one NaN":
            ref = np_colmed(X)
            assert np.isnan(ref[1]) and not np.isnan(np.delete(ref, 1)).any()
        _check_all_runs(J, ctx, X)


def test_col_median_mad_mirror(J, ctx):
    X = np.asfortranarray(np.random.default_rng(4).standard_normal((301, 5)))
    med, mad = J.col_median_mad(X, ctx=ctx)
    assert np.array_equal(med, np_colmed(X)) and np.array_equal(mad, np_colmad(X))
    assert np.array_equal(J.col_median_mad(X, mad=False, ctx=ctx), med) and np.array_equal(J.colmad(X, ctx=ctx), mad)
    Xd = J.colmajor_empty(301, 5, "cuda:0"); Xd.copy_(torch.as_tensor(X, device="cuda:0"))
    md, dd = J.col_median_mad(Xd, ctx=ctx)
    assert isinstance(md, np.ndarray) and np.array_equal(md, med) and np.array_equal(dd, mad)
    assert np.array_equal(J.colmad(np.ascontiguousarray(X), ctx=ctx), mad)   # a row-major host array is copied


# ---------------------------------------------------------------------------------- the row-maximum step of jch_stah
def _rowmax(J, ctx, loc, xa, n, a, ldx, mu, s):
    """jch_stah with fit = 0, p = a, P = identity and no scaling: d (n) as a host array, sentinels checked."""
    lib = J.load()
    P = np.asfortranarray(np.eye(a))
    mu0, s0 = mu.copy(), s.copy()
    if loc == 0:
        d = np.full(n + 2, SENT)
        ctx.check(lib.jch_stah(ctx._h, 0, xa, n, a, ldx, None, None, P.ctypes.data, a, a, 0, mu.ctypes.data, s.ctypes.data, d.ctypes.data + 8))
    else:
        dd = torch.full((n + 2,), SENT, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        ctx.check(lib.jch_stah(ctx._h, 1, xa, n, a, ldx, None, None, P.ctypes.data, a, a, 0, mu.ctypes.data, s.ctypes.data, dd.data_ptr() + 8))
        d = _host(dd)
    assert d[0] == SENT and d[n + 1] == SENT
    assert np.array_equal(mu, mu0) and np.array_equal(s, s0)                  # fit = 0: read only
    return d[1:n + 1].copy()


# a = ST_PANEL_MAXCOLS + 3: a second, narrower panel (a = 70 stays within one panel of ST_PANEL_MAXCOLS columns)
ROWMAX_SHAPES = [(n, a) for n in (1, 63, 64, 65, 1025) for a in (1, 3, 70)] + [(1, ST_PANEL_MAXCOLS + 3), (65, ST_PANEL_MAXCOLS + 3)]


@pytest.mark.parametrize("n,a", ROWMAX_SHAPES)
def test_stah_row_maximum_is_exact(J, ctx, n, a):
    rng = np.random.default_rng(10 * n + a)
    X = np.asfortranarray(rng.standard_normal((n, a)))
    mu, s = rng.standard_normal(a), rng.random(a) + 0.5
    ref = np.abs((X - mu) / s).max(1)
    runs = [_rowmax(J, ctx, 0, X.ctypes.data, n, a, n, mu, s)] + [_rowmax(J, ctx, 1, xa, n, a, ldx, mu, s) for _, xa, ldx in _layouts(X)]
    for d in runs:
        assert np.array_equal(d, ref)
    # a NaN at one X[i, j] reaches d[i] only, wherever the column lies
    i, j = n // 2, a - 1
    X[i, j] = np.nan
    for d in [_rowmax(J, ctx, 0, X.ctypes.data, n, a, n, mu, s)] + [_rowmax(J, ctx, 1, xa, n, a, ldx, mu, s) for _, xa, ldx in _layouts(X)]:
        assert np.isnan(d[i]) and np.array_equal(np.delete(d, i), np.delete(ref, i))


def test_stah_row_maximum_with_a_zero_scale_gives_the_ieee_result(J, ctx):
    n, a = 65, 3
    rng = np.random.default_rng(8)
    X = np.asfortranarray(rng.standard_normal((n, a)))
    mu, s = rng.standard_normal(a), np.array([1.5, 0.0, 0.7])
    X[0, 1] = mu[1]                                                          # 0 / 0 in row 0, x / 0 elsewhere
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = np.abs((X - mu) / s).max(1)
    assert np.isnan(ref[0]) and np.all(np.isinf(ref[1:]))
    assert np.array_equal(_rowmax(J, ctx, 0, X.ctypes.data, n, a, n, mu, s), ref, equal_nan=True)


# ---------------------------------------------------------------------------------- stah, occstah and predict against the restatements
def _near(got, ref, what):
    got, ref = _host(got), np.asarray(ref)
    err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
    assert err <= 1e-9, (what, err)


def _cm(J, a):
    t = J.colmajor_empty(a.shape[0], a.shape[1], "cuda:0")
    t.copy_(torch.as_tensor(np.asarray(a), device="cuda:0"))
    return t


@pytest.fixture(scope="module")
def data():
    X, _, Xnew, _ = occ_data()
    return X, Xnew


@pytest.mark.parametrize("scal", [True, False])
@pytest.mark.parametrize("a", STAH_A)
def test_stah_occstah_and_predict_against_the_restatements(J, ctx, data, a, scal):
    X, Xnew = data
    X0 = X.copy()
    P = stah_P(X.shape[1], a)
    ref = np_stah(X, P, scal)
    got = J.stah(X, a, scal=scal, P=P, ctx=ctx)
    assert isinstance(got.d, np.ndarray) and np.array_equal(got.P, P) and np.array_equal(X, X0)
    assert np.array_equal(got.mu_scal, ref["mu_scal"]) and np.array_equal(got.s_scal, ref["s_scal"])      # exact order statistics of X
    _near(got.mu, ref["mu"], "mu"); _near(got.s, ref["s"], "s"); _near(got.d, ref["d"], "d")
    Xd, Xnd = _cm(J, X), _cm(J, Xnew)
    gd = J.stah(Xd, a, scal=scal, P=P, ctx=ctx)
    assert gd.d.is_cuda and np.array_equal(_host(gd.d), got.d) and np.array_equal(gd.mu, got.mu) and np.array_equal(gd.s, got.s)
    assert np.array_equal(_host(Xd), X0)
    for typc in ("mad", "q"):
        robj = np_occstah(X, P, typc, scal=scal)
        obj = J.occstah(X, a=a, typc=typc, scal=scal, P=P, ctx=ctx)
        assert np.array_equal(obj.d["d"], got.d) and np.array_equal(obj.res_stah.mu, got.mu)             # occstah(...).d is stah(...)'s on the same P
        assert list(obj.d) == ["d", "dstand", "pval"] and np.array_equal(obj.e_cdf, np.sort(got.d))
        _near(np.array([obj.cutoff]), np.array([robj["cutoff"]]), "cutoff")
        _near(obj.d["dstand"], robj["d"]["dstand"], "dstand")
        keep = stah_comparable_rows(robj["d"]["dstand"], robj["d"]["d"], robj["dtrain"], True)
        assert (~keep).mean() <= 0.01 and np.array_equal(obj.d["pval"][keep], robj["d"]["pval"][keep])
        rp = np_occstah_predict(robj, Xnew)
        gp = J.predict(obj, Xnew, ctx=ctx)
        _near(gp.d["d"], rp["d"]["d"], "predicted d"); _near(gp.d["dstand"], rp["d"]["dstand"], "predicted dstand")
        keep = stah_comparable_rows(rp["d"]["dstand"], rp["d"]["d"], robj["dtrain"], False)
        assert (~keep).mean() <= 0.01
        assert gp.pred.dtype == np.int64 and gp.pred.shape == rp["pred"].shape
        assert np.array_equal(gp.pred[keep], rp["pred"][keep]) and np.array_equal(gp.d["pval"][keep], rp["d"]["pval"][keep])
        assert rp["pred"].any() and not rp["pred"].all()                                                 # both classes occur
        # device tensors in: d, the table and pred on the device, the same bits
        od = J.occstah(Xd, a=a, typc=typc, scal=scal, P=P, ctx=ctx)
        assert od.cutoff == obj.cutoff and od.e_cdf.is_cuda
        gpd = J.occ_predict(od, Xnd, ctx=ctx)
        for tab_h, tab_d in ((obj.d, od.d), (gp.d, gpd.d)):
            for name, col in tab_d.items():
                assert col.is_cuda and np.array_equal(_host(col), tab_h[name]), name
        assert gpd.pred.is_cuda and gpd.pred.dtype == torch.int64 and np.array_equal(_host(gpd.pred), gp.pred)


def test_seed_gives_the_same_directions_twice(J, ctx, data):
    X, _ = data
    r1, r2 = J.stah(X, 9, seed=3, ctx=ctx), J.stah(X, 9, seed=3, ctx=ctx)
    assert np.array_equal(r1.P, r2.P) and r1.P.shape == (X.shape[1], 9) and set(np.unique(r1.P)) <= {0.0, 1.0}
    assert np.array_equal(r1.d, r2.d) and np.array_equal(r1.mu, r2.mu) and np.array_equal(r1.s, r2.s)
    o = J.occstah(X, a=9, seed=3, ctx=ctx)
    assert np.array_equal(o.res_stah.P, r1.P) and np.array_equal(o.d["d"], r1.d)


# ---------------------------------------------------------------------------------- the three routes of the C entries (tests/host_routes.py)
@pytest.mark.parametrize("entry", sorted(__import__("host_routes").ROUTES["stah"]))
def test_host_arrays_padded_and_unpadded_give_the_bits_of_the_device_route(entry):
    """Device buffers, host arrays with ld == rows and with ld = rows + 3 between NaN guards: equal bytes, NaN padding kept, inputs unchanged."""
    import host_routes as HR
    HR.three_routes(HR.ROUTES["stah"][entry])
