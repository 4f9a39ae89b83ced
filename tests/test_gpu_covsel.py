"""Covsel on the GPU (jch_covsel_fit and its Python mirror) against the numpy routes of test_covsel_static.

Tolerances (nothing here is tuned to what the kernels deliver; every case prints its error / bound ratio):
  step 1 of C for `cov` is a plain product, K = Xc'Yc:   |K_gpu - K_ref| <= 2 gamma_n sum_i |xc_ij| |yc_ik|,  gamma_n = n eps / (1 - n eps)
      (the standard bound of an n-term sum, once for each summation order).  C holds z_j = sum_k (K_jk / n)^2, so the bound is carried
      through the square: |z_gpu - z_ref| <= sum_k (2 |K_jk| + b_jk) b_jk / n^2, b_jk = that bound + 4 eps |K_jk| (the roundings of the
      means and of the centring), + 8 eps z_j (the squares, the division and the q-term sum);
  everything later, and selcov, cov2, G, QtY, cumpvarx, cumpvary, the in-place X and Y, the predictions of covselr:
      tol = max(10 x the gap between the two CPU routes (literal and postponed) on the same input, 50 eps x the largest magnitude of the
      compared array): the CPU gap measures how ill-conditioned the case is, the factor 10 covers a third summation order.  G and QtY exist
      only in the postponed route; their CPU gap is taken as 0, i.e. the bound is 50 eps x the largest magnitude.
Selections are demanded equal to the literal route's wherever its best-to-second-best gap is > 1e-6 (asserted for the conditioned cases
in test_covsel_static, checked per step for the shape grid)."""
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

from test_covsel_static import (CASES, EPS, GAP, GRID, case_nlv, covselr_from_parts, cpu_gap, excluded, np_covsel_literal,  # noqa: E402
                                np_covsel_postponed, np_covselr, routes, spectra_xy)

TYP = {"cov": 0, "cor": 1}
# (n, p, q, level): every n of {2, 63, 64, 65, 257, 1000, 4097}, p of {1, 2, 7, 130, 513}, q of {1, 3, 17} and both levels; q = 17 is a panel of
# 18 columns (two 16-wide tiles), q = 32 one of 33 (a second chunk that re-reads X); nlv = min(p, 12)
SHAPES = [(2, 1, 1, 1.0), (2, 7, 3, 100.0), (63, 2, 1, 1.0), (64, 130, 3, 100.0), (65, 7, 17, 1.0), (257, 513, 1, 100.0), (257, 1, 17, 1.0),
          (1000, 130, 17, 1.0), (1000, 2, 3, 100.0), (4097, 513, 3, 1.0), (4097, 7, 1, 100.0), (64, 513, 17, 100.0), (257, 130, 32, 1.0)]


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


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


def _run(J, ctx, X, Y, nlv, typ, where="device", pad=0, inplace=False):
    """One jch_covsel_fit on X (n x p) and Y (n x q) stored with leading dimension n + pad, from the host or the device.  The rows beyond n
    of both buffers are NaN and must stay so; without `inplace` both buffers must come back bit-identical.  Returns the results as a dict
    (cut to the completed steps), with the buffers' first n rows as X and Y."""
    L = J.load()
    n, p = X.shape
    q = Y.shape[1]
    a = min(nlv, p)
    ld = n + pad
    xb = np.full((ld, p), np.nan, order="F"); xb[:n] = X
    yb = np.full((ld, q), np.nan, order="F"); yb[:n] = Y
    sel = np.full(a, -1, dtype=np.int32)
    selcov, cpx, cpy, cov2 = np.full(a, np.nan), np.full(a, np.nan), np.full(a, np.nan), np.full(p, np.nan)
    xm, ym, ys = np.full(p, np.nan), np.full(q, np.nan), np.full(q, np.nan)
    Cm, G, QtY = np.full((p, a), np.nan, order="F"), np.full((p, a), np.nan, order="F"), np.full((a, q), np.nan, order="F")
    done = C.c_int32(-1)
    small = [sel, selcov, cov2, Cm, cpx, cpy, xm, ym, ys, G, QtY]
    if where == "host":
        Q = np.full((n, a), np.nan, order="F")
        ctx.check(L.jch_covsel_fit(ctx._h, 0, xb.ctypes.data, n, p, ld, yb.ctypes.data, q, ld, nlv, TYP[typ], int(inplace), *[v.ctypes.data for v in small],
                                   Q.ctypes.data, C.byref(done)))
        xa, ya = xb, yb
    else:
        xd = torch.from_numpy(np.ascontiguousarray(xb.T)).cuda()      # (p, ld) row-major == ld x p column-major
        yd = torch.from_numpy(np.ascontiguousarray(yb.T)).cuda()
        Qd = torch.full((a, n), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.check(L.jch_covsel_fit(ctx._h, 1, xd.data_ptr(), n, p, ld, yd.data_ptr(), q, ld, nlv, TYP[typ], int(inplace), *[v.ctypes.data for v in small],
                                   Qd.data_ptr(), C.byref(done)))
        xa, ya, Q = xd.cpu().numpy().T, yd.cpu().numpy().T, Qd.cpu().numpy().T
    assert np.isnan(xa[n:]).all() and np.isnan(ya[n:]).all(), "rows beyond n were written"
    if not inplace:
        assert np.array_equal(xa[:n], X) and np.array_equal(ya[:n], Y), "X or Y was modified without inplace"
    k = int(done.value)
    assert 0 <= k <= a
    return dict(sel=sel[:k].astype(np.int64), selcov=selcov[:k], cov2=cov2, C=Cm[:, :k], cumpvarx=cpx[:k], cumpvary=cpy[:k], xmeans=xm, ymeans=ym,
                yscales=ys, G=G[:, :k], QtY=QtY[:k], Q=np.array(Q[:, :k]), nlv_out=k, X=np.array(xa[:n]), Y=np.array(ya[:n]), raw=small)


def _same_bits(r1, r2):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(r1["raw"], r2["raw"])) and np.array_equal(r1["Q"], r2["Q"], equal_nan=True)


def _check(name, got, ref, tol):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if got.size == 0:
        return 0.0
    assert np.isfinite(got).all(), name
    err = np.abs(got - ref)
    ratio = float(np.max(err / tol))
    print(f"  {name}: max |err| {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    assert np.all(err <= tol), f"{name}: err / bound {ratio:.3f}"
    return ratio


def _rule(lit_v, post_v, ref):
    """max(10 x the CPU gap, 50 eps x the largest magnitude)."""
    return max(10.0 * cpu_gap(lit_v, post_v), 50.0 * EPS * float(np.max(np.abs(ref))) if np.size(ref) else 0.0)


def _check_first_step_cov(got, X, Y, lit):
    """Step 1 of C for `cov` against the product bound (module docstring)."""
    n = X.shape[0]
    Xc = X - lit["xmeans"]
    Yc = (Y - lit["ymeans"]) / lit["yscales"]
    K = Xc.T @ Yc
    b = 2.0 * gamma(n) * (np.abs(Xc).T @ np.abs(Yc)) + 4.0 * EPS * np.abs(K)      # (+ the roundings of centring and of the mean itself)
    tol = ((2.0 * np.abs(K) + b) * b).sum(1) / n ** 2 + 8.0 * EPS * lit["C"][:, 0]
    _check("C[:, 0] (cov): product bound", got["C"][:, 0], ((K / n) ** 2).sum(1), np.maximum(tol, np.finfo(float).tiny))


def _check_fields(got, lit, post, typ, steps, with_inplace=False):
    """The fields of the first `steps` steps under the rule of the module docstring."""
    p = lit["C"].shape[0]
    for i in range(steps):
        keep = np.ones(p, dtype=bool)
        if typ == "cor":
            keep[excluded(lit, i)] = False
            assert np.all(got["C"][~keep, i] == 0.0)                   # the documented deviation: an exhausted column scores 0
        ref = lit["C"][keep, i]
        _check(f"C[:, {i}]", got["C"][keep, i], ref, _rule(ref, post["C"][keep, i], ref))
    for f in ("selcov", "cumpvarx", "cumpvary"):
        _check(f, got[f][:steps], lit[f][:steps], _rule(lit[f][:steps], post[f][:steps], lit[f][:steps]))
    for f in ("xmeans", "ymeans", "yscales"):
        _check(f, got[f], lit[f], _rule(lit[f], post[f], lit[f]))
    if steps == post["nlv_out"] == got["nlv_out"]:
        full = np.zeros(p); full[lit["sel"][:steps]] = lit["selcov"][:steps]
        _check("cov2", got["cov2"], full, _rule(full, post["cov2"], full))
        _check("G", got["G"], post["G"], _rule(0.0, 0.0, post["G"]))
        _check("QtY", got["QtY"], post["QtY"], _rule(0.0, 0.0, post["QtY"]))
        Qg = got["Q"]
        _check("Q'Q - I", Qg.T @ Qg, np.eye(steps), 50.0 * EPS * max(steps, 1))
        if with_inplace:
            _check("X in place", got["X"], lit["X"], _rule(lit["X"], post["X"], lit["X"]))
            _check("Y in place", got["Y"], lit["Y"], _rule(lit["Y"], post["Y"], lit["Y"]))


# ---------------------------------------------------------------------------------------------------- the pass on its own
@pytest.mark.parametrize("n,p,b,level,pad", [(2, 1, 1, 1.0, 0), (63, 7, 2, 100.0, 3), (64, 130, 17, 1.0, 0), (65, 513, 2, 100.0, 1), (257, 130, 33, 1.0, 3),
                                             (1000, 2, 16, 100.0, 0), (4097, 513, 18, 100.0, 3), (4097, 1050, 2, 1.0, 4)])
def test_pass_is_the_centred_product(J, ctx, n, p, b, level, pad):
    """out = (X - 1 mu')'V within 2 gamma_n sum_i |x_ij - mu_j| |v_ik| (+ eps |x_ij| |v_ik| for the subtraction in registers); V does NOT sum to
    zero, so a pass that dropped the means would be off by n mu_j mean(v_k); rows beyond n are NaN and must not be read; identical bits twice."""
    rng = np.random.default_rng(n + p + b)
    X = level + rng.standard_normal((n, p))
    V = rng.standard_normal((n, b)) + 0.5
    mu = X.mean(0)
    ld = n + pad
    xb = np.full((ld, p), np.nan, order="F"); xb[:n] = X
    vb = np.full((ld, b), np.nan, order="F"); vb[:n] = V
    xd = torch.from_numpy(np.ascontiguousarray(xb.T)).cuda()
    vd = torch.from_numpy(np.ascontiguousarray(vb.T)).cuda()
    md = torch.from_numpy(mu).cuda()
    outs = []
    for rep in range(2):
        od = torch.full((b, p), float("nan"), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        ctx.check(J.load().jch_covsel_pass(ctx._h, xd.data_ptr(), n, p, ld, md.data_ptr(), vd.data_ptr(), b, ld, od.data_ptr()))
        outs.append(od.cpu().numpy().T)
    assert np.array_equal(outs[0], outs[1])
    Xc = X - mu
    bound = 2.0 * gamma(n) * (np.abs(Xc).T @ np.abs(V)) + EPS * (np.abs(X).T @ np.abs(V))
    _check("pass", outs[0], Xc.T @ V, bound)
    od = torch.full((b, p), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.check(J.load().jch_covsel_pass(ctx._h, xd.data_ptr(), n, p, ld, None, vd.data_ptr(), b, ld, od.data_ptr()))
    _check("pass without means", od.cpu().numpy().T, X.T @ V, 2.0 * gamma(n) * (np.abs(X).T @ np.abs(V)))


# ---------------------------------------------------------------------------------------------------- the conditioned cases
@pytest.mark.parametrize("case,typ", GRID)
def test_selection_and_parity(J, ctx, case, typ):
    X, Y, lit, post = routes(case, typ)
    k = case_nlv(case, typ)
    first = None
    for where in ("host", "device"):
        for pad in (0, 3):
            got = _run(J, ctx, X, Y, k, typ, where, pad)
            if first is None:
                first = got
                again = _run(J, ctx, X, Y, k, typ, where, pad)
                assert _same_bits(got, again), "two runs differ"
            else:
                assert _same_bits(got, first), f"{where}, ld = n + {pad}: not the bits of the first route"
    got = first
    assert got["nlv_out"] == k
    assert np.array_equal(got["sel"], lit["sel"]), (got["sel"], lit["sel"])
    if typ == "cov":
        _check_first_step_cov(got, X, Y, lit)
    _check_fields(got, lit, post, typ, k)


@pytest.mark.parametrize("case,typ", GRID)
def test_in_place_leaves_the_deflated_matrices(J, ctx, case, typ):
    X, Y, lit, post = routes(case, typ)
    k = case_nlv(case, typ)
    ref = _run(J, ctx, X, Y, k, typ, "device", 0)
    for where, pad in (("device", 3), ("host", 0)):
        got = _run(J, ctx, X, Y, k, typ, where, pad, inplace=True)
        assert _same_bits(got, ref), "in place changes the results"
        assert np.array_equal(got["sel"], lit["sel"])
        _check_fields(got, lit, post, typ, k, with_inplace=True)


# ---------------------------------------------------------------------------------------------------- the shape grid
@pytest.mark.parametrize("typ", ["cov", "cor"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d-p%d-q%d-level%g" % s)
def test_shapes(J, ctx, shape, typ):
    n, p, q, level = shape
    nlv = min(p, 12)
    X, Y = spectra_xy(n, p, q, level, 7)
    lit = np_covsel_literal(X, Y, nlv, typ, dense_h=n <= 300)
    post = np_covsel_postponed(X, Y, nlv, typ)
    got = _run(J, ctx, X, Y, nlv, typ, "device", 3)
    got_h = _run(J, ctx, X, Y, nlv, typ, "host", 0)
    assert _same_bits(got, got_h)
    want = min(nlv, n - 1)                                            # the centred X has rank min(n - 1, p): the noise makes it full
    assert got["nlv_out"] == want == post["nlv_out"], (got["nlv_out"], post["nlv_out"], want)
    steps = 0                                                         # steps the literal route decides by more than a rounding error
    # (with `cor` the reference itself may land on an already selected column, whose value is rounding noise over rounding noise: the
    # documented deviation, test_covsel_static; the comparison ends there, such a step is not one the literal route decides)
    while steps < want and lit["gap"][steps] > GAP and (typ == "cov" or (sorted(excluded(lit, steps)) == sorted(lit["sel"][:steps])
                                                                          and lit["sel"][steps] not in lit["sel"][:steps])):
        steps += 1
    print(f"  {steps} of {want} steps are conditioned")
    assert steps >= 1 or n == 2        # (n = 2: every column is +-1 after centring, `cor` ties them all)
    assert np.array_equal(got["sel"][:steps], lit["sel"][:steps]), (got["sel"], lit["sel"])
    if typ == "cov":
        _check_first_step_cov(got, X, Y, lit)
    if np.array_equal(post["sel"][:steps], lit["sel"][:steps]):
        _check_fields(got, lit, post, typ, steps)
    assert np.isfinite(got["C"]).all() and np.isfinite(got["G"]).all() and np.isfinite(got["Q"]).all()


# ---------------------------------------------------------------------------------------------------- behaviour
def test_rank_deficient_input_stops_early(J, ctx):
    X, Y = spectra_xy(65, 7, 1, 1.0, 5)
    X = np.array(X, order="F"); X[:, 4] = X[:, 1]
    for typ in ("cov", "cor"):
        got = _run(J, ctx, X, Y, 7, typ, "device", 3)
        k = got["nlv_out"]
        post = np_covsel_postponed(X, Y, 7, typ)
        print(f"  {typ}: nlv_out = {k}, the postponed route: {post['nlv_out']}")
        assert 1 <= k < 7
        for f in ("sel", "selcov", "C", "cumpvarx", "cumpvary", "G", "QtY", "Q"):
            assert np.isfinite(got[f]).all(), f
        assert len(set(got["sel"])) == k and not {1, 4} <= set(got["sel"])          # never both copies
        small = got["raw"]
        assert np.all(small[1][k:] == 0.0) and np.all(small[4][k:] == 0.0) and np.all(small[9][:, k:] == 0.0)   # later steps: zeros, not NaN


def test_python_mirror_records_and_covselr(J, ctx):
    case = CASES[1]
    X, Y, lit, post = routes(case, "cov")
    n, p, q, nlv = case[:4]
    res = J.covsel(X, Y, nlv=nlv, ctx=ctx)
    assert np.array_equal(res.sel["sel"], lit["sel"]) and list(res.sel) == ["sel", "cov2", "cumpvarx", "cumpvary"]
    assert res.C.shape == (p, nlv) and res.cov2.shape == (p,) and res.Q.shape == (n, nlv) and isinstance(res.Q, np.ndarray)
    Xd, Yd = J.colmajor_empty(n, p, "cuda:0"), J.colmajor_empty(n, q, "cuda:0")
    Xd.copy_(torch.from_numpy(np.array(X))); Yd.copy_(torch.from_numpy(np.array(Y)))
    resd = J.covsel(Xd, Yd, nlv=nlv, ctx=ctx)
    assert resd.Q.is_cuda and np.array_equal(resd.C, res.C) and np.array_equal(resd.Q.cpu().numpy(), res.Q)
    assert np.array_equal(Xd.cpu().numpy(), X)
    resi = J.covsel_(Xd, Yd, nlv=nlv, ctx=ctx)                         # in place on the device tensors
    assert np.array_equal(resi.C, res.C)
    _check("covsel_ X", Xd.cpu().numpy(), lit["X"], _rule(lit["X"], post["X"], lit["X"]))
    _check("covsel_ Y", Yd.cpu().numpy(), lit["Y"], _rule(lit["Y"], post["Y"], lit["Y"]))
    # covselr: coefficients and predictions on 100 new rows
    Xn, _ = spectra_xy(100, p, q, case[4], 99)
    Bref, b0ref = np_covselr(X, Y, lit["sel"])
    Bpost, b0post = covselr_from_parts(post)
    for typ in ("cov", "cor"):
        fm = J.covselr(X, Y, nlv, typ, ctx=ctx)
        assert isinstance(fm, J.Covselr)
        if typ == "cov":
            B, b0 = J.coef(fm)
            _check("covselr B", B, Bref, _rule(Bref, Bpost, Bref))
            pref = b0ref + Xn[:, lit["sel"]] @ Bref
            ppost = b0post + Xn[:, lit["sel"]] @ Bpost
            pred = J.predict(fm, Xn, ctx=ctx)
            _check("covselr predictions", pred, pref, _rule(pref, ppost, pref))
            Xnd = J.colmajor_empty(100, p, "cuda:0"); Xnd.copy_(torch.from_numpy(Xn))
            predd = J.predict(fm, Xnd, ctx=ctx)
            assert predd.is_cuda and np.array_equal(predd.cpu().numpy(), pred)


def test_a_communicator_of_two_ranks_is_refused(J):
    L = J.load()
    grp = C.c_void_p()
    assert L.jch_loopback_group_create(2, C.byref(grp)) == 0
    c = J.Context(0)
    try:
        c.comm_init_loopback(grp, 0, 2)
        X, Y = spectra_xy(20, 5, 1, 1.0, 0)
        with pytest.raises(J.JchError) as ei:
            J.covsel(X, Y, nlv=2, ctx=c)
        assert ei.value.code == J._lib.JCH_EINVAL
    finally:
        c.close()
        L.jch_loopback_group_destroy(grp)
