"""What the five PLS fits leave in the caller's X and Y on the GPU, element by element, straight through the C ABI with raw pointers:
jch_plskern_fit, jch_plssimp_fit, jch_plsrosa_fit, jch_plsnipals_fit, jch_plswold_fit (and jch_plskern_fit_scaled) with desc->inplace = 1
against the longdouble restatements and the per-element bounds of test_inplace_static (its docstring derives every bound; nothing here is
tuned to what the kernels deliver), evaluated with the model (T, P, C) the library itself returned; and, with inplace = 0, that nothing
the caller owns is written.

Common rules: every X, Y, T and weights_norm buffer is padded to its leading dimension with NaN and sits between NaN guards; the padding and
the guards must come back NaN, the weights bit-identical; an in-place fit runs twice from fresh copies and must repeat its bits; the host
route must give the bits of the aligned device route whenever n is even (it is the same kernel on the staged copy); the model agrees with
the oracle (a consistently wrong model must not satisfy the restatement); every case prints max err / bound (`-s` shows them, the last test
prints the worst per algorithm and route)."""
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

import test_gpu_accessors as G  # noqa: E402
import test_inplace_static as S  # noqa: E402
from test_gpu_accessors import Dev, host_matrix  # noqa: E402
from oracle import plsr_oracle as O  # noqa: E402

TIGHT = 1e-9                # the suite's sign-aligned relative Frobenius gate of a model against the oracle (test_gpu_parity.TIGHT)
SQRT_EPS = float(np.sqrt(np.finfo(float).eps))
WOLD_NAN, ONE_PASS, REUSE_XCOPY = 2, 4, 8      # include/jchemo_hip.h JCH_WOLD_REF_ZERO_WEIGHT_NAN, JCH_NIPALS_ONE_PASS, JCH_REUSE_XCOPY
PREFIX = "in place: "
MODEL = ("P", "R", "W", "C", "TT", "xmeans", "xscales", "ymeans", "yscales")


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


@pytest.fixture(autouse=True)
def _default_deflation(monkeypatch):
    monkeypatch.delenv("JCH_NIPALS_DEFER", raising=False)


def _check(key, name, got, ref, bound):
    return G._check(PREFIX + key, f"{key}, {name}", got, ref, bound)


# ---------------------------------------------------------------------------------------------------- one call
def _call(J, ctx, alg, n, p, q, nlv, scal, loc, xptr, ldx, yptr, ldy, wptr, tptr, wnptr, inplace, reserved=0, xdiv=None, ydiv=None):
    """One fit through the C ABI.  Returns (status, columns computed, the host outputs; NaN where the library wrote nothing)."""
    L = J.load()
    kmax = max(1, min(p, nlv))
    o = dict(P=np.full((p, kmax), np.nan, order="F"), R=np.full((p, kmax), np.nan, order="F"), W=np.full((p, kmax), np.nan, order="F"),
             C=np.full((q, kmax), np.nan, order="F"), TT=np.full(kmax, np.nan), xmeans=np.full(p, np.nan), xscales=np.full(p, np.nan),
             ymeans=np.full(q, np.nan), yscales=np.full(q, np.nan), niter=np.full(kmax, np.nan))
    desc = J._lib.PlsDesc(n=n, p=p, q=q, nlv=nlv, scal=int(scal), dtype=0, loc=loc, inplace=int(inplace), reserved=reserved)
    got = C.c_int32(-1)
    small = [o[k].ctypes.data for k in MODEL]
    if xdiv is not None:
        st = L.jch_plskern_fit_scaled(ctx._h, C.byref(desc), xptr, ldx, yptr, ldy, wptr, xdiv.ctypes.data, G.vec(ydiv), tptr, *small, wnptr, C.byref(got))
    elif alg == "plswold":
        st = L.jch_plswold_fit(ctx._h, C.byref(desc), xptr, ldx, yptr, ldy, wptr, SQRT_EPS, 200, tptr, *small, wnptr, o["niter"].ctypes.data, C.byref(got))
    else:
        st = getattr(L, "jch_%s_fit" % alg)(ctx._h, C.byref(desc), xptr, ldx, yptr, ldy, wptr, tptr, *small, wnptr, C.byref(got))
    return st, got.value, o


def _trim(o, k):
    """The first k columns of the model; the columns the fit did not compute must still be NaN."""
    for f in ("P", "R", "W", "C"):
        assert np.isnan(o[f][:, k:]).all(), f"{f}: a column beyond nlv_out was written"
        o[f] = o[f][:, :k]
    assert np.isnan(o["TT"][k:]).all()
    o["TT"] = o["TT"][:k]
    return o


class DeviceCall:
    """X, Y, weights, T and weights_norm of one device-resident call, each in a NaN-guarded buffer of its own."""

    def __init__(self, X, Y, w, nlv, pad, mis):
        n, p = X.shape
        self.n, self.kmax = n, max(1, min(p, nlv))
        self.xd, self.yd = Dev(X, ld=n + pad, mis=mis), Dev(Y, ld=n + pad, mis=mis)
        self.wd = None if w is None else Dev(w)
        self.td, self.nd = Dev(rows=n, cols=self.kmax), Dev(rows=n, cols=1)

    def run(self, J, ctx, alg, nlv, scal, inplace, reserved=0, xdiv=None, ydiv=None):
        torch.cuda.synchronize()
        return _call(J, ctx, alg, self.n, self.xd.cols, self.yd.cols, nlv, scal, 1, self.xd.ptr, self.xd.ld, self.yd.ptr, self.yd.ld,
                     self.wd.ptr if self.wd else None, self.td.ptr, self.nd.ptr, inplace, reserved, xdiv, ydiv)

    def outputs(self, k):
        """X, Y, T[:, :k], weights_norm after the call (every get() checks the padding, the later columns and the guards); the weights intact."""
        if self.wd:
            self.wd.unchanged()
        return self.xd.get(), self.yd.get(), self.td.get(k), self.nd.get()[:, 0]


def _fit_device(J, ctx, alg, X, Y, w, nlv, scal, pad, mis, reserved=0, xdiv=None, ydiv=None):
    dc = DeviceCall(X, Y, w, nlv, pad, mis)
    st, k, o = dc.run(J, ctx, alg, nlv, scal, True, reserved, xdiv, ydiv)
    assert st == 0, (alg, J.load().jch_last_error(ctx._h))
    Xg, Yg, T, wn = dc.outputs(k)
    return dict(_trim(o, k), X=Xg, Y=Yg, T=T, wn=wn, k=k)


def _fit_host(J, ctx, alg, X, Y, w, nlv, scal, pad, reserved=0, xdiv=None, ydiv=None):
    n, p = X.shape
    q, kmax = Y.shape[1], max(1, min(p, nlv))
    xh, yh = host_matrix(X, n + pad), host_matrix(Y, n + pad)
    th, wn = np.full((n, kmax + 1), np.nan, order="F"), np.full(n + 1, np.nan)
    wh = None if w is None else w.copy()
    st, k, o = _call(J, ctx, alg, n, p, q, nlv, scal, 0, xh.ctypes.data, n + pad, yh.ctypes.data, n + pad, G.vec(wh), th.ctypes.data, wn.ctypes.data,
                     True, reserved, xdiv, ydiv)
    assert st == 0, (alg, J.load().jch_last_error(ctx._h))
    assert np.isnan(xh[n:]).all() and np.isnan(yh[n:]).all(), "the rows beyond the host matrix were written"
    assert np.isnan(th[:, k:]).all() and np.isnan(wn[n]), "a host output was written beyond its end"
    assert w is None or np.array_equal(wh, w), "the host weights were modified"
    return dict(_trim(o, k), X=np.array(xh[:n]), Y=np.array(yh[:n]), T=np.array(th[:, :k]), wn=wn[:n].copy(), k=k)


def _same_bits(a, b, what):
    for f in ("X", "Y", "T", "wn") + MODEL:
        assert np.array_equal(a[f], b[f], equal_nan=True), f"{what}: {f} differs"


def _route_name(alg, case, host, pad, mis):
    n, p, q, _ = case
    kern, back, _ = S.centre_route(n, p, q, n if host else n + pad, True if host else not mis, alg in S.KERN_LIKE)
    if alg in S.KERN_LIKE:
        return f"{kern} kernel, X {back}"
    return "export of the deflated copy, " + ("eager" if S.defer_period(p, q) == 1 else "postponed") + " deflation"


def _check_outputs(alg, route, name, c, r, w, nan_rows=False, rows=slice(None), T=None):
    """X and Y of an in-place result against the restatement with the result's own T, P, C (T: the concatenated scores of a sharded fit)."""
    Xe, bX, Ye, bY = S.expected(alg, c, r["T"] if T is None else T, r["P"], r["C"], rows)
    _check(f"{alg}! X [{route}]", name, r["X"], Xe, bX)
    _check(f"{alg}! Y [{route}]", name, r["Y"], Ye, bY)
    d = np.asarray(c.d[rows], dtype=np.float64)
    _check("weights_norm", name, r["wn"], c.d[rows], S.gamma(c.n + 2) * d)
    if alg == "plswold" and w is not None and np.any(w == 0.0):
        zero = w == 0.0
        assert not np.any(r["X"][zero]) and not np.any(r["Y"][zero]), f"{name}: a row without weight is not exactly 0"
        assert np.isnan(r["T"][zero]).all() if nan_rows else np.isfinite(r["T"]).all(), f"{name}: the scores of the rows without weight"


def _check_model(alg, case, r, ref, w, name, nan_rows=False):
    """T, P, R, W, C, TT against the oracle, sign-aligned, on the latent variables that are well posed."""
    n, p, q, nlv = case
    assert r["k"] == min(n, p, nlv), (name, r["k"])
    deflated = S.well_posed_nlv(case) < min(n, p, nlv)                   # (a fully deflated case: its leading ones, as test_seeded_vs_c_oracle)
    k = max(1, min(n, p) - 2) if deflated else min(n, p, nlv)
    s = O.sign_align(ref.W[:, :k], r["W"][:, :k])
    live = slice(None) if not (alg == "plswold" and w is not None) else w != 0.0
    # (R = W inv(P'W) of plsrosa, plsnipals and plswold takes every column of P, the noise of an ill-posed last one included, in the
    # reference as here: its leading columns are compared where the last latent variable exists)
    for f in ("T", "P", "W", "C") + (("R",) if not (deflated and alg in S.DEFLATES_Y) else ()):
        a, b = getattr(ref, f)[:, :k], r[f][:, :k] * s
        if f == "T":
            a, b = a[live], b[live]
        e = O.rel_fro(a, b)
        assert e < TIGHT, (name, f, e)
    assert O.rel_fro(ref.TT[:k], r["TT"][:k]) < TIGHT, name
    for f in ("xmeans", "xscales", "ymeans", "yscales"):
        assert O.rel_fro(getattr(ref, f), r[f]) < TIGHT, (name, f)


# ---------------------------------------------------------------------------------------------------- a. in place, all five algorithms
@pytest.mark.parametrize("case,scal,wkind", S.PARAMS, ids=["%s-%s-w_%s" % (S.case_id(c), "scal" if s else "noscal", w) for c, s, w in S.PARAMS])
def test_inplace_outputs(J, ctx, case, scal, wkind):
    n, p, q, nlv = case
    X, Y = S.inplace_data(case)
    w = S.inplace_weights(n, wkind)
    c = S.centred(X, Y, w, scal)
    for alg in S.ALGOS:
        ref = S.oracle_inplace(alg, X, Y, w, S.well_posed_nlv(case), scal)[0]
        aligned = None
        for sname, host, pad, mis in S.storage_of(case):
            route = _route_name(alg, case, host, pad, mis)
            name = f"{alg}! {sname}"
            fit = (lambda **kw: _fit_host(J, ctx, alg, X, Y, w, nlv, scal, pad, **kw)) if host else \
                  (lambda **kw: _fit_device(J, ctx, alg, X, Y, w, nlv, scal, pad, mis, **kw))                 # noqa: E731
            r = fit()
            _same_bits(r, fit(), f"{name}: two runs")
            _check_outputs(alg, route, name, c, r, w)
            _check_model(alg, case, r, ref, w, name)
            if sname == "dev-ld+0":
                aligned = r
            if host and n % 2 == 0 and aligned is not None:
                _same_bits(aligned, r, f"{name}: the host route against the aligned device route")
            if alg == "plswold" and wkind == "zeros" and n > 3 and sname in ("dev-ld+0", "dev-ld+1", "host-ld+3"):
                rn = fit(reserved=WOLD_NAN)                                 # the reference's NaN scores: X and Y are the same zeros
                _check_outputs(alg, route, name + ", NaN scores", c, rn, w, nan_rows=True)
                assert np.array_equal(rn["X"], r["X"]) and np.array_equal(rn["Y"], r["Y"]), f"{name}: the NaN-score mode changes X or Y"


# ---------------------------------------------------------------------------------------------------- b. the flush of the postponed deflation
@pytest.mark.parametrize("nlv", S.FLUSH_NLVS)
@pytest.mark.parametrize("alg", ["plsnipals", "plswold"])
def test_flush_of_the_postponed_deflation(J, ctx, monkeypatch, alg, nlv):
    """Every number of corrections pending at the last latent variable (period 6: nlv below, at and one past a multiple) against the
    restatement, and against the eager deflation (JCH_NIPALS_DEFER=1), which leaves through the same export but never postpones."""
    case = S.FLUSH_CASE + (nlv,)
    n, p, q, _ = case
    X, Y = S.inplace_data(case)
    w = S.inplace_weights(n, "zeros")
    c = S.centred(X, Y, w, True)
    ref = S.oracle_inplace(alg, X, Y, w, nlv, True)[0]
    ctx.set_profiling(True)
    try:
        lazy = _fit_device(J, ctx, alg, X, Y, w, nlv, True, 1, False)
        lazy_bytes = ctx.profile().sweep_bytes
        monkeypatch.setenv("JCH_NIPALS_DEFER", "1")
        eager = _fit_device(J, ctx, alg, X, Y, w, nlv, True, 1, False)
        eager_bytes = ctx.profile().sweep_bytes
    finally:
        ctx.set_profiling(False)
    # (the two runs really differ: the eager one rewrites the rows once per latent variable, the postponed one at its flushes only)
    assert eager_bytes > lazy_bytes if nlv > 1 else eager_bytes == lazy_bytes, (lazy_bytes, eager_bytes)
    for how, r in (("postponed", lazy), ("eager", eager)):
        _check_outputs(alg, f"export of the deflated copy, {how} deflation", f"{alg}! nlv {nlv} {how}", c, r, w)
        _check_model(alg, case, r, ref, w, f"{alg}! nlv {nlv} {how}")
    _, bXl, _, bYl = S.expected(alg, c, lazy["T"], lazy["P"], lazy["C"])
    _, bXe, _, bYe = S.expected(alg, c, eager["T"], eager["P"], eager["C"])
    _check(f"{alg}! X [postponed against eager]", f"nlv {nlv}", lazy["X"], eager["X"].astype(G.LD), bXl + bXe)
    _check(f"{alg}! Y [postponed against eager]", f"nlv {nlv}", lazy["Y"], eager["Y"].astype(G.LD), bYl + bYe)


# ---------------------------------------------------------------------------------------------------- c. not in place: nothing is written
NOT_INPLACE = [("plskern", 0), ("plssimp", 0), ("plsrosa", 0), ("plsnipals", 0), ("plswold", 0), ("plskern", 1), ("plsnipals", ONE_PASS),
               ("plswold", ONE_PASS), ("plswold", WOLD_NAN)]


def _untouched(dc, k, name):
    for v, what in ((dc.xd, "X"), (dc.yd, "Y"), (dc.wd, "weights")):
        if v is not None:
            try:
                v.unchanged()
            except AssertionError as e:
                raise AssertionError(f"{name}: {what}: {e}") from None
    dc.td.get(k)                                                            # (columns from k on, the guards)
    dc.nd.get()


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=[S.case_id(c) for c in S.CASES])
def test_not_inplace_leaves_the_inputs_alone(J, ctx, i):
    case = S.CASES[i]
    n, p, q, nlv = case
    scal, wkind = bool(i % 2), S.WKINDS[i % 3]
    X, Y = S.inplace_data(case)
    w = S.inplace_weights(n, wkind)
    for pad, mis in ((0, False), (1, False), (0, True)):
        for alg, reserved in NOT_INPLACE:
            name = f"{alg} reserved {reserved} ld+{pad}{' X+8' if mis else ''}"
            dc = DeviceCall(X, Y, w, nlv, pad, mis)
            st, k, o = dc.run(J, ctx, alg, nlv, scal, False, reserved)
            if reserved in (1, ONE_PASS) and st == J._lib.JCH_EINVAL:       # outside the envelope of the opt-in path: refused, and nothing written
                assert q > 16 or p > S.SWEEP_MAXP or (reserved == ONE_PASS and S.defer_period(p, q) == 1), name
                k = 0
            else:
                assert st == 0, (name, J.load().jch_last_error(ctx._h))
                assert k == min(n, p, nlv) and np.isfinite(dc.nd.get()).all()
            _untouched(dc, k, name)
        # two plskern fits in a row, the second one told that X has not changed
        dc = DeviceCall(X, Y, w, nlv, pad, mis)
        st, k, o1 = dc.run(J, ctx, "plskern", nlv, scal, False, 0)
        assert st == 0
        T1 = dc.td.get(k)
        st, k2, o2 = dc.run(J, ctx, "plskern", nlv, scal, False, REUSE_XCOPY)
        assert st == 0 and k2 == k
        _untouched(dc, k, f"plskern, JCH_REUSE_XCOPY, ld+{pad}")
        s = O.sign_align(o1["W"][:, :k], o2["W"][:, :k])
        kk = max(1, min(n, p) - 2) if min(n, p) <= nlv else nlv
        assert O.rel_fro(T1[:, :kk], dc.td.get(k)[:, :kk] * s[:kk]) < TIGHT


@pytest.mark.parametrize("alg", S.ALGOS)
def test_clamped_fit_leaves_the_unused_score_columns_alone(J, ctx, alg):
    """3 x 5 with nlv = 9: nlv_out = 3 of the 5 columns T was given; the header promises `columns filled`, so the other two stay as they were."""
    n, p, q, _ = S.CASES[1]
    X, Y = S.inplace_data(S.CASES[1])
    for inplace in (False, True):
        dc = DeviceCall(X, Y, None, 9, 1, False)
        assert dc.kmax == 5
        st, k, o = dc.run(J, ctx, alg, 9, False, inplace)
        assert st == 0 and k == 3, (st, k)
        _trim(o, 3)
        T = dc.td.get(3)
        assert T.shape == (3, 3)
        dc.nd.get()
        if not inplace:
            _untouched(dc, 3, alg)


# ---------------------------------------------------------------------------------------------------- d. caller-supplied divisors
def test_scaled_fit_in_place(J, ctx):
    case = S.SCALED_CASE
    n, p, q, nlv = case
    X, Y = S.inplace_data(case)
    w = S.inplace_weights(n, "random")
    rng = np.random.default_rng(5)
    xdiv, ydiv = rng.uniform(0.5, 2.0, p), rng.uniform(0.5, 2.0, q)
    for yd_ in (ydiv, None):
        c = S.centred(X, Y, w, False, xdiv, yd_)
        runs = {}
        for sname, host, pad, mis in S.STORAGE:
            kw = dict(xdiv=xdiv, ydiv=yd_)
            fit = (lambda: _fit_host(J, ctx, "plskern", X, Y, w, nlv, False, pad, **kw)) if host else \
                  (lambda: _fit_device(J, ctx, "plskern", X, Y, w, nlv, False, pad, mis, **kw))               # noqa: E731
            r = runs[sname] = fit()
            _same_bits(r, fit(), f"scaled {sname}: two runs")
            assert np.array_equal(r["xscales"], xdiv) and np.array_equal(r["yscales"], np.ones(q) if yd_ is None else yd_), "the divisors are not echoed"
            kern = S.centre_route(n, p, q, n if host else n + pad, True if host else not mis, True)[0]
            _check_outputs("plskern", f"caller's divisors, {kern} kernel", f"scaled {sname}", c, r, w)
        # (n is odd: the host route stages with ld = n like the device route with ld = n, the tile kernel both)
        _same_bits(runs["dev-ld+0"], runs["host-ld+3"], "scaled: the host route against the device route of the layout it stages")


# ---------------------------------------------------------------------------------------------------- e. row-sharded, in place
def _sharded(J, alg, X, Y, w, cut, nlv, scal):
    """Two ranks on one GPU (a loopback group, one thread and one context each, as test_gpu_parity._run_sharded), device-resident shards."""
    L = J.load()
    n = X.shape[0]
    grp = C.c_void_p()
    assert L.jch_loopback_group_create(2, C.byref(grp)) == 0
    ctxs = [J.Context(0) for _ in range(2)]
    bounds = [(0, cut), (cut, n)]
    dcs = [DeviceCall(np.asfortranarray(X[a:b]), np.asfortranarray(Y[a:b]), None if w is None else w[a:b].copy(), nlv, 1, False) for a, b in bounds]
    torch.cuda.synchronize()
    out, err = [None, None], [None, None]

    def work(r):
        try:
            ctxs[r].comm_init_loopback(grp, r, 2)
            out[r] = dcs[r].run(J, ctxs[r], alg, nlv, scal, True)
        except Exception as e:  # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a rank thread is stuck in a collective"
    assert err == [None, None], err
    res = []
    for r in range(2):
        st, k, o = out[r]
        assert st == 0, L.jch_last_error(ctxs[r]._h)
        Xg, Yg, T, wn = dcs[r].outputs(k)
        res.append(dict(_trim(o, k), X=Xg, Y=Yg, T=T, wn=wn, k=k))
    for cx in ctxs:
        cx.close()
    L.jch_loopback_group_destroy(grp)
    return bounds, res


@pytest.mark.parametrize("alg", ["plskern", "plsnipals", "plswold"])
def test_row_sharded_in_place(J, alg):
    case = S.SHARD_CASE
    n, p, q, nlv = case
    X, Y = S.inplace_data(case)
    w = S.inplace_weights(n, "zeros")
    c = S.centred(X, Y, w, True)                                            # the global means and stds
    bounds, res = _sharded(J, alg, X, Y, w, int(S.SHARD_CUT * n), nlv, True)
    for f in MODEL:
        assert np.array_equal(res[0][f], res[1][f]), f"{f}: the replicated state differs between the ranks"
    T = np.concatenate([r["T"] for r in res], axis=0)
    full = dict(res[0], T=T, k=res[0]["k"])
    _check_model(alg, case, full, S.oracle_inplace(alg, X, Y, w, nlv, True)[0], w, f"{alg}! sharded")
    for (a, b), r in zip(bounds, res):
        _check_outputs(alg, "two ranks, 30 % / 70 %", f"{alg}! rows {a}..{b}", c, r, w[a:b], rows=slice(a, b))


# ---------------------------------------------------------------------------------------------------- f. the report
def test_zz_report_the_worst_ratios():
    """Not a check of its own: prints what the tests above measured (worst err / bound per algorithm, output and route)."""
    mine = {k[len(PREFIX):]: v for k, v in G.WORST.items() if k.startswith(PREFIX)}
    for key in sorted(mine):
        print(f"  worst err / bound, {key}: {mine[key]:.3f}")
    assert all(v <= 1.0 for v in mine.values())
