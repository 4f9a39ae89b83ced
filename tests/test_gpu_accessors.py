"""The accessor and statistics primitives on the GPU, straight through the C ABI with raw pointers: jch_affine_gemm, jch_transform,
jch_predict, jch_col_stats, jch_weighted_ss, jch_weighted_cov, jch_score_sums, jch_score_sums_lv against the longdouble restatements and the
per-element bounds of test_accessors_static (its docstring derives every bound; nothing here is tuned to what the kernels deliver).

Common rules: every buffer is padded to its leading dimension with NaN and sits between NaN guards; the rows beyond m, the column after
the last one and the guards of every output must come back NaN, every input bit-identical; every call runs twice and must repeat its
bits; the host route must give the bits of the aligned device route; every case prints max err / bound (`-s` shows them, the last test
prints the worst per primitive)."""
import ctypes as C
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

import test_accessors_static as S  # noqa: E402
from test_accessors_static import LD  # noqa: E402

NAN = float("nan")
WORST = {}                 # primitive -> worst err / bound seen
FOLD = {}                  # (level, width class) -> worst err / centred bound seen (reported in DESIGN.md, never asserted)


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


# ---------------------------------------------------------------------------------------------------- buffers
class Dev:
    """A column-major (rows x cols, leading dimension ld) device matrix inside a NaN-filled allocation: two guard doubles in front (three
    when `mis`: the matrix then starts 8 bytes into a 16-byte aligned allocation), two behind, NaN in the rows beyond `rows`."""

    def __init__(self, A=None, rows=None, cols=None, ld=None, mis=False):
        if A is not None:
            A = np.asarray(A, dtype=np.float64)
            A = A.reshape(len(A), -1)
            rows, cols = A.shape
        self.rows, self.cols, self.ld = rows, cols, (rows if ld is None else ld)
        self.off = 3 if mis else 2
        self.buf = torch.full((self.off + self.ld * cols + 2,), NAN, dtype=torch.float64, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf[self.off:self.off + self.ld * cols].view(cols, self.ld)
        self.src = A
        if A is not None:
            self.view[:, :rows] = torch.from_numpy(np.ascontiguousarray(A.T))
        self.ptr = self.view.data_ptr()
        assert self.ptr % 16 == (8 if mis else 0)

    def get(self, cols=None):
        """The first `cols` columns as rows x cols, after checking that the padding rows, later columns and the guards are still NaN."""
        h = self.buf.cpu().numpy()
        body = h[self.off:self.off + self.ld * self.cols].reshape(self.cols, self.ld)
        cols = self.cols if cols is None else cols
        assert np.isnan(h[:self.off]).all() and np.isnan(h[self.off + self.ld * self.cols:]).all(), "written outside the buffer"
        assert np.isnan(body[:, self.rows:]).all(), "the rows beyond the matrix were written"
        assert np.isnan(body[cols:]).all(), "a column beyond the output was written"
        return np.array(body[:cols, :self.rows].T)

    def unchanged(self):
        assert np.array_equal(self.get(), self.src, equal_nan=True), "an input was modified"


def host_matrix(A, ld):
    """A copy of A (rows x cols) in a column-major host array of leading dimension ld, NaN beyond the rows."""
    A = np.asarray(A, dtype=np.float64)
    b = np.full((ld, A.shape[1]), np.nan, order="F")
    b[:A.shape[0]] = A
    return b


def host_out(rows, cols, ld):
    return np.full((ld, cols + 1), np.nan, order="F")


def take_host_out(b, rows, cols):
    assert np.isnan(b[rows:]).all() and np.isnan(b[:, cols:]).all(), "the host output's padding was written"
    return np.array(b[:rows, :cols])


def vec(v):
    """A host vector argument: its address (kept alive by the caller's reference) or NULL."""
    return None if v is None else v.ctypes.data


def f64(v):
    return None if v is None else np.ascontiguousarray(v, dtype=np.float64)


def _check(prim, name, got, ref, bound):
    got, bound = np.asarray(got), np.asarray(bound, dtype=np.float64)
    assert got.shape == np.shape(ref) == bound.shape, (name, got.shape, np.shape(ref), bound.shape)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all(), f"{name}: not finite"
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    pos = bound > 0.0
    ratio = float(np.max(np.where(pos, err / np.where(pos, bound, 1.0), np.where(err > 0.0, np.inf, 0.0))))
    print(f"  {name}: max |err| {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    WORST[prim] = max(WORST.get(prim, 0.0), ratio)
    assert np.all(err <= bound), f"{name}: err / bound {ratio:.3f}"
    return ratio


# ---------------------------------------------------------------------------------------------------- 1. jch_affine_gemm, device-resident
# (name, ldx - m, ldo - m, X 8 bytes in, out 8 bytes in)
STORAGE = [("aligned", 0, 0, False, False), ("ldo+1", 0, 1, False, False), ("out+8", 0, 0, False, True), ("ldx+1", 1, 0, False, False),
           ("X+8", 0, 0, True, False)]
AFFINE_PARAMS = [(t, c) for t in S.AFFINE_TRIPLES for i, c in enumerate(S.AFFINE_CONFIGS) if i == 0 or t[0] * t[1] <= S.AFFINE_BIG]


def _affine_call(J, ctx, loc, xptr, m, p, ldx, shift, scale, B, k, bias, optr, ldo):
    ctx.check(J.load().jch_affine_gemm(ctx._h, loc, xptr, m, p, ldx, vec(shift), vec(scale), vec(B), k, vec(bias), optr, ldo))


def _affine_reference(X, shift, scale, B, bias):
    ref, factor = S.ref_affine(X, shift, scale, B, bias)
    return ref, S.bound_affine(X, shift, scale, B, bias, factor)


def _report_folding(level, X, shift, scale, B, got, ref):
    cb = S.bound_affine_centred(X, shift, scale, B)
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    r = float(np.max(err[cb > 0.0] / cb[cb > 0.0])) if np.any(cb > 0.0) else 0.0
    key = (level, "p >= 32" if X.shape[1] >= 32 else "p < 32")
    FOLD[key] = max(FOLD.get(key, 0.0), r)
    print(f"  level {level:g}: err / (gamma(p + 3) |X - shift| |Bs|) = {r:.3f}  (reported: what the folding costs)")


@pytest.mark.parametrize("triple,config", AFFINE_PARAMS, ids=["m%d-p%d-k%d-%s-level%g-%s" % (t + (c[0], "all" if c[1] else "NULL")) for t, c in AFFINE_PARAMS])
def test_affine_gemm_device(J, ctx, triple, config):
    m, p, k, _ = triple
    level, present = config
    X, shift, scale, B, bias = S.affine_data(m, p, k, level, present)
    shift, scale, B, bias = f64(shift), f64(scale), np.asfortranarray(B), f64(bias)
    ref, bound = _affine_reference(X, shift, scale, B, bias)
    xs, first = {}, None
    for name, padx, pado, misx, miso in STORAGE:
        kern = S.affine_kernel(m, p, k, (m + padx) % 2 == 0, not misx, (m + pado) % 2 == 0, not miso)
        if (padx, misx) not in xs:                                       # (one copy of X on the device at a time, checked when it leaves)
            for old in xs.values():
                old.unchanged()
            xs.clear()
            xd = None
            xs[(padx, misx)] = Dev(X, ld=m + padx, mis=misx)
        xd = xs[(padx, misx)]
        outs = []
        for rep in range(2):
            od = Dev(rows=m, cols=k + 1, ld=m + pado, mis=miso)
            torch.cuda.synchronize()
            _affine_call(J, ctx, 1, xd.ptr, m, p, xd.ld, shift, scale, B, k, bias, od.ptr, od.ld)
            outs.append(od.get(k))
            del od
        assert np.array_equal(outs[0], outs[1]), f"{name} ({kern}): two runs differ"
        _check("jch_affine_gemm", f"{name} ({kern})", outs[0], ref, bound)
        if first is None:
            first = outs[0]
            if present:
                _report_folding(level, X, shift, scale, B, outs[0], ref)
    xd.unchanged()
    xs.clear()
    del xd
    # the host route: the bits of the aligned device route, from padded host arrays
    xh, oh = host_matrix(X, m + 3), host_out(m, k, m + 2)
    _affine_call(J, ctx, 0, xh.ctypes.data, m, p, m + 3, shift, scale, B, k, bias, oh.ctypes.data, m + 2)
    assert np.array_equal(xh[:m], X) and np.isnan(xh[m:]).all()
    assert np.array_equal(take_host_out(oh, m, k), first), "the host route's bits differ from the aligned device route's"


@pytest.mark.parametrize("level", S.FOLD_LEVELS)
def test_affine_gemm_folding_cost_is_reported(J, ctx, level):
    """The folded form at level 1e2 and 1e4 (the figures of DESIGN.md): asserted against the folded bound, the ratio to the centred bound printed."""
    for m, p, k in S.FOLD_CASES:
        X, shift, scale, B, bias = S.fold_data(m, p, k, level)
        ref, bound = _affine_reference(X, shift, scale, B, bias)
        xd, od = Dev(X), Dev(rows=m, cols=k + 1)
        torch.cuda.synchronize()
        _affine_call(J, ctx, 1, xd.ptr, m, p, m, shift, scale, B, k, bias, od.ptr, m)
        got = od.get(k)
        _check("jch_affine_gemm", f"m{m} p{p} k{k} level {level:g} ({S.affine_kernel(m, p, k)})", got, ref, bound)
        _report_folding(level, X, shift, scale, B, got, ref)


# ---------------------------------------------------------------------------------------------------- 2. jch_transform and jch_predict
def _predict_call(J, ctx, loc, xptr, m, p, ldx, model, q, lo, hi, optr, ldo):
    ctx.check(J.load().jch_predict(ctx._h, loc, xptr, m, p, ldx, vec(model["xmeans"]), vec(model["xscales"]), vec(model["ymeans"]), vec(model["yscales"]),
                                   vec(model["R"]), vec(model["C"]), q, lo, hi, optr, ldo))


@pytest.mark.parametrize("case", S.PREDICT_CASES, ids=lambda c: "m%d-q%d-ldo+%d-%s%s-%s" % (c[0], c[1], c[2], "pred+8-" if c[3] else "", "NULL" if c[4] else "all", c[5]))
def test_transform_and_predict(J, ctx, case):
    m, q, pad, mis, null, _ = case
    p, nlv = S.PREDICT_P, S.PREDICT_NLV
    X, model = S.predict_data(m, q, null)
    model = {key: f64(v) if v is None or v.ndim == 1 else np.asfortranarray(v) for key, v in model.items()}
    L = J.load()
    xd, xh = Dev(X), host_matrix(X, m + 1)
    # transform: the scores, device (twice) and host
    ref, bound = _affine_reference(X, model["xmeans"], model["xscales"], model["R"], None)
    outs = []
    for rep in range(2):
        td = Dev(rows=m, cols=nlv + 1, ld=m + pad, mis=mis)
        torch.cuda.synchronize()
        ctx.check(L.jch_transform(ctx._h, 1, xd.ptr, m, p, m, vec(model["xmeans"]), vec(model["xscales"]), vec(model["R"]), nlv, td.ptr, td.ld))
        outs.append(td.get(nlv))
    th = host_out(m, nlv, m + pad)
    ctx.check(L.jch_transform(ctx._h, 0, xh.ctypes.data, m, p, m + 1, vec(model["xmeans"]), vec(model["xscales"]), vec(model["R"]), nlv, th.ctypes.data, m + pad))
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(take_host_out(th, m, nlv), outs[0]), "transform: runs or routes differ"
    _check("jch_transform", "transform", outs[0], ref, bound)
    for lo, hi in S.PREDICT_RANGES:
        kc = (hi - lo + 1) * q
        path = S.predict_path(m, lo, hi)
        outs = []
        for rep in range(2):
            pd = Dev(rows=m, cols=kc + 1, ld=m + pad, mis=mis)
            torch.cuda.synchronize()
            _predict_call(J, ctx, 1, xd.ptr, m, p, m, model, q, lo, hi, pd.ptr, pd.ld)
            outs.append(pd.get(kc))
        ph = host_out(m, kc, m + pad)
        _predict_call(J, ctx, 0, xh.ctypes.data, m, p, m + 1, model, q, lo, hi, ph.ctypes.data, m + pad)
        assert np.array_equal(outs[0], outs[1]), f"predict {lo}..{hi} ({path}): two runs differ"
        assert np.array_equal(take_host_out(ph, m, kc), outs[0]), f"predict {lo}..{hi} ({path}): the host route's bits differ"
        _check("jch_predict", f"predict {lo}..{hi} ({path})", outs[0], S.ref_predict(X, model, lo, hi), S.bound_predict(X, model, lo, hi))
    xd.unchanged()
    assert np.array_equal(xh[:m], X) and np.isnan(xh[m:]).all()


# ---------------------------------------------------------------------------------------------------- 3. jch_col_stats and jch_weighted_ss
# These two and jch_weighted_cov pick their load path by the layout they are given (k_moments: 16-byte loads of two rows per lane when X,
# the weights and the leading dimension allow, else 8-byte loads with another assignment of rows to lanes; K2: the panel or the tile
# kernel), and the paths sum in different orders.  So the host route, which stages its input with ld = n in an aligned buffer, has the
# bits of the device route ON THAT LAYOUT: that is what is demanded; the case's own layout is run twice and held to the bounds by itself.
def _routes(n, pad, plain, M, w, mis_m=False, mis_w=False):
    """The case's device layout (twice), the layout the host route stages (ld = n, aligned) and the padded host arrays."""
    md, wd = Dev(M, ld=n + pad, mis=mis_m), (None if w is None else Dev(w, mis=mis_w))
    mp, wp = (md, wd) if plain else (Dev(M), None if w is None else Dev(w))
    mh = host_matrix(M, n + pad)
    calls = [("device", 1, md.ptr, wd.ptr if wd else None, n + pad), ("device again", 1, md.ptr, wd.ptr if wd else None, n + pad),
             ("device as staged", 1, mp.ptr, wp.ptr if wp else None, n), ("host", 0, mh.ctypes.data, vec(w), n + pad)]
    return calls, [md, mp] + [v for v in (wd, wp) if v is not None], mh


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("case", S.STATS_CASES, ids=lambda c: "n%d-p%d-level%g-w_%s-ldx+%d%s%s" % (c[:5] + ("-X+8" if c[5] else "", "-w+8" if c[6] else "")))
def test_col_stats_and_weighted_ss(J, ctx, case):
    n, p, level, wkind, pad, misx, misw = case
    L = J.load()
    X, w = S.stats_data(n, p, level, wkind)
    mean, std = S.ref_col_stats(X, w)
    bm, bs = S.bound_means(X, w), S.bound_stds(X, w)
    plain = pad == 0 and not misx and not misw
    calls, inputs, xh = _routes(n, pad, plain, X, w, misx, misw)
    runs = []
    for name, loc, xptr, wptr, ldx in calls:
        mo, so = np.full(p + 1, np.nan), np.full(p + 1, np.nan)
        torch.cuda.synchronize()
        ctx.check(L.jch_col_stats(ctx._h, loc, xptr, n, p, ldx, wptr, mo.ctypes.data, so.ctypes.data))
        assert np.isnan(mo[p]) and np.isnan(so[p])
        runs.append((mo[:p], so[:p]))
        m2 = np.full(p + 1, np.nan)                                         # stds = NULL: the same means
        ctx.check(L.jch_col_stats(ctx._h, loc, xptr, n, p, ldx, wptr, m2.ctypes.data, None))
        assert np.array_equal(m2[:p], mo[:p]) and np.isnan(m2[p])
    assert _same(runs[0], runs[1]), "col_stats: two runs differ"
    assert _same(runs[2], runs[3]), "col_stats: the host route's bits differ from the device route's on the layout it stages"
    for name, r in (("device", runs[0]), ("host", runs[3])):
        _check("jch_col_stats", f"means ({name})", r[0], mean, bm)
        _check("jch_col_stats", f"stds ({name})", r[1], std, bs)
        if p >= 2:
            print(f"  the constant column ({name}): std {r[1][0]:.3e}, bound {bs[0]:.3e}")
    # weighted_ss: the normalised weights as given, about the reference means with column scales, and about nothing
    d = np.ones(n) / n if w is None else w / w.sum()
    calls, inputs2, _ = _routes(n, pad, plain, X, d, misx, misw)
    rng = np.random.default_rng(n + p)
    for shift, scale in ((np.asarray(mean, dtype=np.float64), rng.uniform(0.5, 2.0, p)), (None, None)):
        got = []
        for name, loc, xptr, dptr, ldx in calls:
            ss = np.full(2, np.nan)
            torch.cuda.synchronize()
            ctx.check(L.jch_weighted_ss(ctx._h, loc, xptr, n, p, ldx, dptr, vec(shift), vec(scale), ss.ctypes.data_as(C.POINTER(C.c_double))))
            assert np.isnan(ss[1])
            got.append(ss[0])
        assert got[0] == got[1], "weighted_ss: two runs differ"
        assert got[2] == got[3], "weighted_ss: the host route's bits differ from the device route's on the layout it stages"
        ref, b = np.array([S.ref_weighted_ss(X, d, shift, scale)], dtype=LD), np.array([S.bound_weighted_ss(X, d, shift, scale)])
        for name, v in (("device", got[0]), ("host", got[3])):
            _check("jch_weighted_ss", f"sstot ({name})" + ("" if shift is not None else ", no shift, no scale"), np.array([v]), ref, b)
    for v in inputs + inputs2:
        v.unchanged()
    assert np.array_equal(xh[:n], X) and np.isnan(xh[n:]).all()


# ---------------------------------------------------------------------------------------------------- 4. jch_weighted_cov
@pytest.mark.parametrize("case", S.COV_CASES, ids=lambda c: "n%d-d%d-level%g-w_%s-lda+%d" % c)
def test_weighted_cov(J, ctx, case):
    n, d, level, wkind, pad = case
    L = J.load()
    A, w = S.cov_data(n, d, level, wkind)
    Sref, mu = S.ref_weighted_cov(A, w)
    b, bm = S.bound_weighted_cov(A, w), S.bound_means(A, w)
    calls, inputs, ah = _routes(n, pad, pad == 0, A, w)
    runs = []
    for name, loc, aptr, wptr, lda in calls:
        So, mo = np.full(d * d + 1, np.nan), np.full(d + 1, np.nan)
        torch.cuda.synchronize()
        ctx.check(L.jch_weighted_cov(ctx._h, loc, aptr, n, d, lda, wptr, So.ctypes.data, mo.ctypes.data))
        assert np.isnan(So[d * d]) and np.isnan(mo[d])
        S2 = np.full(d * d + 1, np.nan)                                     # mu = NULL: the same matrix
        ctx.check(L.jch_weighted_cov(ctx._h, loc, aptr, n, d, lda, wptr, S2.ctypes.data, None))
        assert np.array_equal(S2, So, equal_nan=True)
        runs.append((So[:d * d].reshape(d, d).T, mo[:d]))
    assert _same(runs[0], runs[1]), "weighted_cov: two runs differ"
    assert _same(runs[2], runs[3]), "weighted_cov: the host route's bits differ from the device route's on the layout it stages"
    for name, (Sg, mg) in (("device", runs[0]), ("host", runs[3])):
        _check("jch_weighted_cov", f"mu ({name})", mg, mu, bm)
        _check("jch_weighted_cov", f"S ({name})", Sg, Sref, b)
        _check("jch_weighted_cov", f"S - S' ({name})", Sg - Sg.T, np.zeros((d, d), dtype=LD), 2.0 * b)
    for v in inputs:
        v.unchanged()
    assert np.array_equal(ah[:n], A) and np.isnan(ah[n:]).all()


# ---------------------------------------------------------------------------------------------------- 5. jch_score_sums and jch_score_sums_lv
def _m_sel(mask, m):
    return m if mask is None else int(np.count_nonzero(mask))


def _check_sums(prim, name, got, ref, bound, m_sel):
    assert np.all(got[:, 5] == m_sel), f"{name}: the row count is not exact"
    if m_sel == 0:
        assert not np.any(got), f"{name}: an empty selection must give zeros"
    return _check(prim, name, got, ref, bound)


@pytest.mark.parametrize("case", S.SCORE_CASES, ids=lambda c: "m%d-q%d-levels%d-mask_%s-ld+%d" % c)
def test_score_sums(J, ctx, case):
    m, q, levels, mkind, pad = case
    L = J.load()
    Pred, Y, mask = S.score_data(m, q, levels, mkind)
    ncol = levels * q
    ref, A = S.ref_score_sums(Pred, Y, mask)
    pd, yd, md = Dev(Pred, ld=m + pad), Dev(Y, ld=m + 2 * pad), (None if mask is None else Dev(mask))
    ph, yh = host_matrix(Pred, m + pad), host_matrix(Y, m + 2 * pad)
    runs = []
    for loc, pp, yp, mp in ((1, pd.ptr, yd.ptr, md.ptr if md else None), (1, pd.ptr, yd.ptr, md.ptr if md else None), (0, ph.ctypes.data, yh.ctypes.data, vec(mask))):
        out = np.full((ncol + 1, 6), np.nan)
        torch.cuda.synchronize()
        ctx.check(L.jch_score_sums(ctx._h, loc, pp, m, ncol, m + pad, yp, q, m + 2 * pad, mp, out.ctypes.data))
        assert np.isnan(out[ncol]).all()
        runs.append(out[:ncol])
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), "score_sums: runs or routes differ"
    _check_sums("jch_score_sums", "sums", runs[0], ref, S.bound_score_sums(A, _m_sel(mask, m)), _m_sel(mask, m))
    pd.unchanged(); yd.unchanged()
    if md:
        md.unchanged()


@pytest.mark.parametrize("case", S.SCORE_LV_CASES, ids=lambda c: "m%d-q%d-kfit%d-mask_%s-ld+%d-%s" % (c[:5] + ("NULL" if c[5] else "all",)))
def test_score_sums_lv(J, ctx, case):
    m, q, kfit, mkind, pad, null = case
    L = J.load()
    T, Cm, ym, ys, Y, mask = S.score_lv_data(m, q, kfit, mkind, null)
    ym, ys = f64(ym), f64(ys)
    td, yd, md = (Dev(T, ld=m + pad) if kfit else None), Dev(Y, ld=m + 2 * pad), (None if mask is None else Dev(mask))
    th, yh = (host_matrix(T, m + pad) if kfit else None), host_matrix(Y, m + 2 * pad)
    for lo, hi in S.score_lv_ranges(kfit):
        ncol = (hi - lo + 1) * q
        ref, bound = S.ref_score_sums_lv(T, Cm, ym, ys, Y, mask, lo, hi)
        runs = []
        for loc, tp, yp, mp in ((1, td.ptr if td else None, yd.ptr, md.ptr if md else None), (1, td.ptr if td else None, yd.ptr, md.ptr if md else None),
                                (0, th.ctypes.data if kfit else None, yh.ctypes.data, vec(mask))):
            out = np.full((ncol + 1, 6), np.nan)
            torch.cuda.synchronize()
            ctx.check(L.jch_score_sums_lv(ctx._h, loc, tp, m, kfit, m + pad, vec(Cm), vec(ym), vec(ys), yp, q, m + 2 * pad, mp, lo, hi, out.ctypes.data))
            assert np.isnan(out[ncol]).all()
            runs.append(out[:ncol])
        assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2]), f"score_sums_lv {lo}..{hi}: runs or routes differ"
        _check_sums("jch_score_sums_lv", f"levels {lo}..{hi}", runs[0], ref, bound, _m_sel(mask, m))
    yd.unchanged()
    if td:
        td.unchanged()
    if md:
        md.unchanged()


# ---------------------------------------------------------------------------------------------------- 6. the argument table
def _small():
    """Valid host arguments of every entry point (m = 6 rows, p = 3, q = 2, two LVs), by name, and fresh NaN outputs."""
    rng = np.random.default_rng(1)
    a = dict(X=np.asfortranarray(rng.standard_normal((6, 3))), Y=np.asfortranarray(rng.standard_normal((6, 2))), B=np.asfortranarray(rng.standard_normal((3, 2))),
             R=np.asfortranarray(rng.standard_normal((3, 2))), Cm=np.asfortranarray(rng.standard_normal((2, 2))), v3=rng.uniform(1.0, 2.0, 3), v2=rng.uniform(1.0, 2.0, 2),
             w=rng.uniform(1.0, 2.0, 6), Pred=np.asfortranarray(rng.standard_normal((6, 4))), T=np.asfortranarray(rng.standard_normal((6, 2))),
             Xlong=np.asfortranarray(rng.standard_normal((4096, 2))))
    return a


def _table():
    """(entry point, valid argument list after ctx, index of the output arguments, {description: (index, bad value)})."""
    a = _small()
    P = lambda x: x.ctypes.data                                           # noqa: E731
    out = lambda n: np.full(n, np.nan)                                    # noqa: E731
    o = dict(g=out(12), t=out(12), p1=out(36), p3=out(4096 * 6), ss=out(1), mean=out(3), std=out(3), S=out(9), mu=out(3), s1=out(24), s2=out(24))
    ssp = o["ss"].ctypes.data_as(C.POINTER(C.c_double))
    T = [
        ("jch_affine_gemm", [0, P(a["X"]), 6, 3, 6, P(a["v3"]), P(a["v3"]), P(a["B"]), 2, P(a["v2"]), P(o["g"]), 6], ["g"],
         {"X NULL": (1, None), "m < 0": (2, -1), "p < 1": (3, 0), "ldx < m": (4, 5), "B NULL": (7, None), "k < 1": (8, 0), "out NULL": (10, None), "ldo < m": (11, 5),
          "bad loc": (0, 7)}),
        ("jch_transform", [0, P(a["X"]), 6, 3, 6, P(a["v3"]), P(a["v3"]), P(a["R"]), 2, P(o["t"]), 6], ["t"],
         {"R NULL": (7, None), "nlv < 1": (8, 0), "X NULL": (1, None), "ldx < m": (4, 5), "T NULL": (9, None), "ldt < m": (10, 5), "bad loc": (0, 2)}),
        ("jch_predict", [0, P(a["X"]), 6, 3, 6, P(a["v3"]), P(a["v3"]), P(a["v2"]), P(a["v2"]), P(a["R"]), P(a["Cm"]), 2, 0, 2, P(o["p1"]), 6], ["p1"],
         {"R NULL": (9, None), "C NULL": (10, None), "q < 1": (11, 0), "nlv_lo < 0": (12, -1), "nlv_hi < nlv_lo": (13, -1), "X NULL": (1, None), "pred NULL": (14, None),
          "p < 1": (3, 0), "ldx < m": (4, 5), "ldo < m": (15, 5), "bad loc": (0, -1)}),
        # three levels on 4096 rows: the checks of the prefix path
        ("jch_predict", [0, P(a["Xlong"]), 4096, 2, 4096, None, None, None, None, P(a["B"]), P(a["Cm"]), 2, 0, 2, P(o["p3"]), 4096], ["p3"],
         {"prefix: X NULL": (1, None), "prefix: pred NULL": (14, None), "prefix: p < 1": (3, 0), "prefix: ldx < m": (4, 4095), "prefix: ldo < m": (15, 4095),
          "prefix: bad loc": (0, 2)}),
        ("jch_weighted_ss", [0, P(a["X"]), 6, 3, 6, P(a["w"]), P(a["v3"]), P(a["v3"]), ssp], ["ss"],
         {"X NULL": (1, None), "n < 1": (2, 0), "p < 1": (3, 0), "ldx < n": (4, 5), "d NULL": (5, None), "sstot NULL": (8, None), "bad loc": (0, 2)}),
        ("jch_col_stats", [0, P(a["X"]), 6, 3, 6, P(a["w"]), P(o["mean"]), P(o["std"])], ["mean", "std"],
         {"X NULL": (1, None), "n < 1": (2, 0), "p < 1": (3, 0), "ldx < n": (4, 5), "means NULL": (6, None), "bad loc": (0, 2), "p > 2^20": (3, (1 << 20) + 1)}),
        ("jch_weighted_cov", [0, P(a["X"]), 6, 3, 6, P(a["w"]), P(o["S"]), P(o["mu"])], ["S", "mu"],
         {"A NULL": (1, None), "n < 1": (2, 0), "d < 1": (3, 0), "d > 32768": (3, 32769), "lda < n": (4, 5), "S NULL": (6, None), "bad loc": (0, 2)}),
        ("jch_score_sums", [0, P(a["Pred"]), 6, 4, 6, P(a["Y"]), 2, 6, P(a["w"]), P(o["s1"])], ["s1"],
         {"Pred NULL": (1, None), "m < 1": (2, 0), "ncol < 1": (3, 0), "ncol % q != 0": (3, 3), "ldp < m": (4, 5), "Y NULL": (5, None), "q < 1": (6, 0), "ldy < m": (7, 5),
          "sums NULL": (9, None), "bad loc": (0, 2)}),
        ("jch_score_sums_lv", [0, P(a["T"]), 6, 2, 6, P(a["Cm"]), P(a["v2"]), P(a["v2"]), P(a["Y"]), 2, 6, P(a["w"]), 0, 1, P(o["s2"])], ["s2"],
         {"T NULL with kfit > 0": (1, None), "m < 1": (2, 0), "kfit < 0": (3, -1), "ldt < m": (4, 5), "C NULL with kfit > 0": (5, None), "Y NULL": (8, None), "q < 1": (9, 0),
          "ldy < m": (10, 5), "nlv_lo < 0": (12, -1), "nlv_hi < nlv_lo": (13, -1), "sums NULL": (14, None), "bad loc": (0, 2)}),
    ]
    return a, o, T


def test_every_bad_argument_is_refused_and_nothing_is_written(J, ctx):
    L = J.load()
    a, o, table = _table()
    keep = {k: v.copy() for k, v in a.items()}
    for fn, args, outs, bad in table:
        for what, (idx, value) in bad.items():
            call = list(args)
            call[idx] = value
            st = getattr(L, fn)(ctx._h, *call)
            msg = L.jch_last_error(ctx._h)
            assert st == J._lib.JCH_EINVAL, f"{fn}: {what}: returned {st}"
            # (jch_transform and jch_predict hand the checks of X and the output to jch_affine_gemm, whose name the text then carries)
            assert msg and (fn.encode() in msg or (fn in ("jch_transform", "jch_predict") and b"jch_affine_gemm" in msg)), f"{fn}: {what}: jch_last_error says {msg!r}"
            assert all(np.isnan(v).all() for v in o.values()), f"{fn}: {what}: an output was written"
        st = getattr(L, fn)(ctx._h, *args)                                  # and the unmodified call is accepted and writes its outputs
        assert st == 0, (fn, L.jch_last_error(ctx._h))
        assert all(np.isfinite(o[k]).all() for k in outs), fn
        for k in outs:
            o[k][:] = np.nan
        assert getattr(L, fn)(None, *args) == J._lib.JCH_EINVAL, f"{fn}: a NULL context"
        assert all(np.isnan(v).all() for v in o.values())
    assert all(np.array_equal(a[k], keep[k]) for k in a)
    # m = 0 of jch_affine_gemm: accepted, nothing written (host and device)
    g = np.full(12, np.nan)
    assert L.jch_affine_gemm(ctx._h, 0, a["X"].ctypes.data, 0, 3, 6, None, None, a["B"].ctypes.data, 2, None, g.ctypes.data, 6) == 0
    assert np.isnan(g).all()
    xd, od = Dev(a["X"]), Dev(rows=6, cols=2)
    assert L.jch_affine_gemm(ctx._h, 1, xd.ptr, 0, 3, 6, None, None, a["B"].ctypes.data, 2, None, od.ptr, 6) == 0
    torch.cuda.synchronize()
    assert np.isnan(od.buf.cpu().numpy()).all()


def test_zz_report_the_worst_ratios():
    """Not a check of its own: prints what the tests above measured (err / bound per primitive, the folded against the centred bound)."""
    for prim in sorted(WORST):
        print(f"  worst err / bound, {prim}: {WORST[prim]:.3f}")
    for level, width in sorted(FOLD):
        print(f"  level {level:g}, {width}: worst err / (gamma(p + 3) |X - shift| |Bs|) = {FOLD[(level, width)]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())

