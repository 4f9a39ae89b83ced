"""CPU-side checks of the locally weighted MLR family (jch_knn_wls; lwmlr, lwmlr_s, lwmlrda, lwmlrda_s): numpy restatements of the reference
(src/wdist.jl, src/locw.jl, src/mlr.jl:69-86, src/mlrda.jl) in float64 and in longdouble, the error bound of DESIGN.md §23 checked between the
two before the GPU tests use it, the equivalence of the global-dummy argmax with the reference's local-levels `mlrda`, and the boundary
(header, symbols, exports, fields, defaults, argument checks, no CPU fallback).  No GPU needed; tests/test_gpu_lwmlr.py imports the restatements."""
import dataclasses
import importlib
import inspect
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import plsr_oracle as O  # noqa: E402

U = 2.0 ** -53
LD = np.longdouble

# (n, d, q or -classes, k, m): the shapes of the issue's table
CASES = [(300, 5, 2, 40, 37), (257, 12, 1, 65, 33), (300, 4, -3, 30, 50), (500, 24, 1, 208, 9), (90, 3, -4, 7, 21)]


# ---------------------------------------------------------------------------------- numpy restatements of the reference
def np_wdist_clamped(d, h, tol, dtype=np.float64):
    """src/wdist.jl:58-75 (cri = 4), then `w[w .< tol] .= tol` (src/lwmlr.jl:87-88), in `dtype`."""
    d = np.asarray(d, dtype=dtype)
    zmed = np.median(d)
    zmad = dtype(1.4826) * np.median(np.abs(d - zmed))
    cutoff = zmed + dtype(4) * zmad
    with np.errstate(all="ignore"):
        w = np.where(d <= cutoff, np.exp(-d / (dtype(h) * zmad)), dtype(0))
        w = w / np.max(w)
    w[np.isnan(w)] = dtype(1)
    w[w < dtype(tol)] = dtype(tol)
    return w


def np_householder_ls(A, B):
    """beta = argmin |A beta - B| by Householder QR without pivoting, written out (numpy's lstsq has no longdouble); alpha = -sign(x1) |x|.
    Returns (beta, the diagonal of R)."""
    A = A.copy(); B = B.copy()
    k, d = A.shape
    rd = np.zeros(d, dtype=A.dtype)
    for j in range(d):
        x = A[j:, j]
        sig = x @ x
        nrm = np.sqrt(sig)
        alpha = -nrm if x[0] > 0 else nrm
        rd[j] = alpha
        if sig == 0:
            continue
        v = x.copy()
        v[0] = x[0] - alpha
        bh = 1 / (nrm * (nrm + abs(x[0])))
        if j + 1 < d:
            A[j:, j + 1:] -= np.outer(v, (v @ A[j:, j + 1:]) * bh)
        B[j:] -= np.outer(v, (v @ B[j:]) * bh)
    beta = np.zeros((d, B.shape[1]), dtype=A.dtype)
    with np.errstate(all="ignore"):
        for j in range(d - 1, -1, -1):
            beta[j] = (B[j] - A[j, j + 1:] @ beta[j + 1:]) / rd[j]
    return beta, rd


def np_wls_query(Xs, Ys, w, xq, dtype=np.float64, diag=False):
    """One query of src/locw.jl with fun = mlr (src/mlr.jl:69-86): (pred [q], info) and, with diag, the quantities the bound reads."""
    Xs = np.asarray(Xs, dtype=dtype); Ys = np.asarray(Ys, dtype=dtype); xq = np.asarray(xq, dtype=dtype)
    k, d = Xs.shape
    q = Ys.shape[1]
    nan = np.full(q, np.nan, dtype=dtype)
    if q == 1 and np.all(Ys[:, 0] == Ys[0, 0]):                      # src/locw.jl:33-34
        return (Ys[0].copy(), 2, None) if diag else (Ys[0].copy(), 2)
    wn = np.asarray(w, dtype=dtype) / np.sum(np.asarray(w, dtype=dtype))   # mweight
    xbar = wn @ Xs; ybar = wn @ Ys                                   # colmean(X, weights)
    sw = np.sqrt(wn)[:, None]
    A = sw * (Xs - xbar); B = sw * (Ys - ybar)
    if k <= d:
        return (nan, 1, None) if diag else (nan, 1)
    beta, rd = np_householder_ls(A, B)
    ar = np.abs(rd)
    if np.nanmin(ar) <= min(k, d) * 2.0 ** -52 * np.nanmax(ar):
        return (nan, 1, None) if diag else (nan, 1)
    dx = xq - xbar
    pred = ybar + dx @ beta                                          # int + x B, int = ymeans' - xmeans' B
    if not diag:
        return pred, 0
    return pred, 0, dict(A=A, B=B, beta=beta, rd=rd, xbar=xbar, ybar=ybar, dx=dx, wn=wn, Xs=Xs, Ys=Ys)


def np_knn_wls(X, Y, Xq, ind, w, dtype=np.float64):
    """jch_knn_wls restated: (pred m x q, info m)."""
    m = ind.shape[0]
    pred = np.empty((m, Y.shape[1]), dtype=dtype)
    info = np.empty(m, dtype=np.int32)
    with np.errstate(all="ignore"):
        for i in range(m):
            pred[i], info[i] = np_wls_query(X[ind[i]], Y[ind[i]], w[i], Xq[i], dtype)
    return pred, info


def np_locw_mlrda(X, yv, Xq, ind, w, dtype=np.float64):
    """src/locw.jl with fun = mlrda (src/mlrda.jl:35-54) on the LOCAL levels of every neighbourhood: (labels [m] — None where the local fit is
    rank-deficient —, the gap between the two largest local posteriors [m], inf for a single-class neighbourhood)."""
    m = ind.shape[0]
    lab, gap = [], np.full(m, np.inf)
    for i in range(m):
        zy = yv[ind[i]]
        lev = np.unique(zy)                                           # the local levels
        if lev.shape[0] == 1:                                         # src/locw.jl:33-34
            lab.append(zy[0]); continue
        Yd = (zy[:, None] == lev[None, :]).astype(dtype)             # dummy(y).Y
        post, info = np_wls_query(X[ind[i]], Yd, w[i], Xq[i], dtype)
        if info == 1:
            lab.append(None); continue
        lab.append(lev[int(np.argmax(post))])                         # first maximum in sorted-level order
        top = np.sort(np.asarray(post, dtype=np.float64))[::-1]
        gap[i] = top[0] - top[1]
    return lab, gap


def wls_bound(diag):
    """The per-response bound of DESIGN.md §23 on |pred_computed - pred_exact| of one fitted query, for any float64 evaluation of the algorithm:
        u (k + 4) (sum w~ |y| + sum_j (sum w~ |x_j|) |beta_j|)                        the two weighted means (their error moves pred by dybar - dxbar'beta)
      + u (d + 2) (|ybar| + sum_j |dx_j| |beta_j|)                                    the final inner product
      + |dx| kappa eps / (1 - kappa eps) (2 |beta| + (kappa + 1) |r| / |A|_2)         Householder LS: backward stable with eps = sqrt(d) (10 k d + 4) u,
                                                                                      then Wedin's perturbation bound (Higham, ASNA 2nd ed., Thm 20.1, 20.3)."""
    A = np.asarray(diag["A"], dtype=np.float64); B = np.asarray(diag["B"], dtype=np.float64)
    beta = np.asarray(diag["beta"], dtype=np.float64); dx = np.asarray(diag["dx"], dtype=np.float64)
    wn = np.asarray(diag["wn"], dtype=np.float64)
    k, d = A.shape
    sv = np.linalg.svd(A, compute_uv=False)
    kappa, a2 = sv[0] / sv[-1], sv[0]
    eps = np.sqrt(d) * (10 * k * d + 4) * U
    assert kappa * eps < 0.5, (kappa, eps)
    r = np.linalg.norm(A @ beta - B, axis=0)
    mabs_x = wn @ np.abs(np.asarray(diag["Xs"], dtype=np.float64))
    mabs_y = wn @ np.abs(np.asarray(diag["Ys"], dtype=np.float64))
    means = U * (k + 4) * (mabs_y + mabs_x @ np.abs(beta))
    dot = U * (d + 2) * (np.abs(np.asarray(diag["ybar"], dtype=np.float64)) + np.abs(dx) @ np.abs(beta))
    ls = np.linalg.norm(dx) * kappa * eps / (1 - kappa * eps) * (2 * np.linalg.norm(beta, axis=0) + (kappa + 1) * r / a2)
    return means + dot + ls


def wls_reference(X, Y, Xq, ind, w):
    """The longdouble restatement with the bound of every entry: (pred as float64 m x q, info, bound m x q; 0 where the result is exact or NaN)."""
    m, q = ind.shape[0], Y.shape[1]
    pred = np.empty((m, q)); info = np.empty(m, dtype=np.int32); bound = np.zeros((m, q))
    with np.errstate(all="ignore"):
        for i in range(m):
            p, info[i], dg = np_wls_query(X[ind[i]], Y[ind[i]], w[i], Xq[i], LD, diag=True)
            pred[i] = np.asarray(p, dtype=np.float64)
            if dg is not None:
                bound[i] = wls_bound(dg) + U * np.abs(pred[i])      # (+ the rounding of the reference to float64)
    return pred, info, bound


def max_ratio(got, ref, bound):
    """Largest |got - ref| / bound over the entries with a bound; entries without one (exact results, NaN rows) must agree exactly."""
    got = np.asarray(got, dtype=np.float64)
    has = bound > 0
    exact = ~has
    assert np.array_equal(got[exact], ref[exact], equal_nan=True), "an exact / NaN entry differs"
    return float(np.max(np.abs(got[has] - ref[has]) / bound[has])) if has.any() else 0.0


# ---------------------------------------------------------------------------------- data
def clustered(n, d, qc, m, seed):
    """Three Gaussian clusters in d dimensions; qc > 0: q responses (linear + a smooth term + noise, off-centre); qc < 0: -qc classes that
    overlap inside every cluster.  Returns X, Y (responses or the global dummy table), yv (labels or None), Xq."""
    rng = np.random.default_rng(seed)
    cen = 3.0 * rng.standard_normal((3, d))
    cl = rng.integers(0, 3, n)
    X = np.asfortranarray(cen[cl] + rng.standard_normal((n, d)))
    Xq = np.asfortranarray(cen[rng.integers(0, 3, m)] + rng.standard_normal((m, d)))
    if qc > 0:
        Bc = rng.standard_normal((d, qc))
        Y = np.asfortranarray(4.0 + X @ Bc + np.sin(X[:, :1]) + 0.3 * rng.standard_normal((n, qc)))
        return X, Y, None, Xq
    ncls = -qc
    score = X @ rng.standard_normal(d) + 0.8 * rng.standard_normal(n)
    yv = (np.digitize(score, np.quantile(score, np.linspace(0, 1, 2 * ncls + 1)[1:-1])) % ncls).astype(np.int64) * 10 + 5   # labels 5, 15, 25, ...
    lev = np.unique(yv)
    Y = np.asfortranarray((yv[:, None] == lev[None, :]).astype(np.float64))
    return X, Y, yv, Xq


_CASE_CACHE = {}


def case(idx, h=2.0, tol=1e-4):
    """Case idx of CASES with its neighbour lists (brute force, (distance, row) order), the clamped wdist weights and the longdouble reference."""
    if idx not in _CASE_CACHE:
        n, d, qc, k, m = CASES[idx]
        X, Y, yv, Xq = clustered(n, d, qc, m, 7100 + idx)
        ind, dist = O.getknn(X, Xq, k=k)
        w = np.stack([np_wdist_clamped(dist[i], h, tol) for i in range(m)])
        ref = wls_reference(X, Y, Xq, ind, w)
        _CASE_CACHE[idx] = dict(X=X, Y=Y, yv=yv, Xq=Xq, ind=ind.astype(np.int32), dist=dist, w=w, ref=ref)
    return _CASE_CACHE[idx]


# ---------------------------------------------------------------------------------- tests: the restatements and the bound
@pytest.mark.parametrize("idx", range(len(CASES)))
def test_float64_restatement_sits_inside_half_the_bound(idx):
    c = case(idx)
    ref, info, bound = c["ref"]
    assert (info == 0).all()                                          # every neighbourhood of these cases is of full rank
    got, ginfo = np_knn_wls(c["X"], c["Y"], c["Xq"], c["ind"], c["w"])
    assert np.array_equal(ginfo, info)
    ratio = max_ratio(got, ref, bound)
    err = float(np.max(np.abs(got - ref)))
    print(f"case {CASES[idx]}: float64 vs longdouble error {err:.2e}, prediction scale {np.max(np.abs(ref)):.2g}, measured / allowed {ratio:.3g}")
    assert ratio <= 0.5, ratio
    assert err < 1e-12                                                # (orientation: the issue's table has 5e-16 .. 5e-15 here)


def test_wdist_restatements_agree():
    """float64 against longdouble: w = exp(-x) / max with x = d / (h mad) carrying a relative error of <= 6 u, so |dw| <= (12 x + 8) u w; the clamp
    and the cutoff are decided alike on these distances (none sits within rounding of the cutoff)."""
    for idx in range(len(CASES)):
        c = case(idx)
        for d in c["dist"]:
            w64, wld = np_wdist_clamped(d, 2.0, 1e-4), np_wdist_clamped(d, 2.0, 1e-4, LD)
            mad = 1.4826 * np.median(np.abs(d - np.median(d)))
            x = d / (2.0 * mad)
            assert np.all(np.abs(w64 - np.asarray(wld, dtype=np.float64)) <= (12 * x + 8) * U * w64)
            assert w64.min() >= 1e-4 and w64.max() == 1.0
    w = np_wdist_clamped(np.array([0.0, 1.0, 2.0, 50.0]), 0.5, 1e-4)
    assert w[0] == 1.0 and w[-1] == 1e-4                               # beyond the cutoff: 0, clamped to tol
    assert np.all(np_wdist_clamped(np.full(5, 3.0), 2.0, 1e-4) == 1.0)    # mad = 0: NaN -> 1


@pytest.mark.parametrize("idx", [2, 4])
def test_global_dummy_argmax_equals_mlrda_on_local_levels(idx):
    """The reference fits `mlrda` on the levels present in the neighbourhood; the library fits the global dummy table and takes the row argmax.
    A class absent from the neighbourhood has a zero centred column: posterior exactly 0, while the present ones sum to 1."""
    c = case(idx)
    ref, info, bound = c["ref"]
    lev = np.unique(c["yv"])
    lab_local, gap = np_locw_mlrda(c["X"], c["yv"], c["Xq"], c["ind"], c["w"], LD)
    post, _ = np_knn_wls(c["X"], c["Y"], c["Xq"], c["ind"], c["w"])
    lab_global = lev[np.argmax(post, axis=1)]
    m = post.shape[0]
    skip = gap <= 2 * bound.max(axis=1)
    print(f"case {CASES[idx]}: smallest top-two gap {gap.min():.2e}, largest bound {bound.max():.2e}, left out {int(skip.sum())} of {m}")
    assert skip.sum() <= 0.01 * m
    assert all(lab_local[i] == lab_global[i] for i in range(m) if not skip[i])
    absent = ~np.stack([np.isin(lev, c["yv"][c["ind"][i]]) for i in range(m)])
    assert np.all(post[absent] == 0.0)
    assert np.all(np.abs(post.sum(axis=1) - 1.0) <= 2 * bound.sum(axis=1) + 8 * U)


def test_special_cases_of_the_restatement():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((12, 3)); xq = rng.standard_normal(3); w = rng.uniform(0.5, 1.0, 12)
    p, info = np_wls_query(X, np.full((12, 1), 2.5), w, xq)
    assert info == 2 and p[0] == 2.5                                   # the constant response, exactly
    p, info = np_wls_query(X[:3], rng.standard_normal((3, 1)), w[:3], xq)
    assert info == 1 and np.isnan(p).all()                             # k <= d
    p, info = np_wls_query(X[:3], np.full((3, 1), -1.0), w[:3], xq)
    assert info == 2 and p[0] == -1.0                                  # ... the shortcut comes first (src/locw.jl:33)
    X2 = X.copy(); X2[:, 2] = X2[:, 0]
    p, info = np_wls_query(X2, rng.standard_normal((12, 2)), w, xq)
    assert info == 1 and np.isnan(p).all()                             # a duplicated column
    Y = 1.0 + X @ np.array([[1.0], [-2.0], [0.5]])
    p, info = np_wls_query(X, Y, w, xq)
    assert info == 0 and abs(p[0] - (1.0 + xq @ np.array([1.0, -2.0, 0.5]))) < 1e-13     # an exact linear response is reproduced
    yv = np.array([3] * 12)
    lab, gap = np_locw_mlrda(X, yv, xq[None, :], np.arange(12)[None, :], w[None, :])
    assert lab == [3] and np.isinf(gap[0])


# ---------------------------------------------------------------------------------- tests: the boundary
def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_header_symbol_and_makefile():
    import jchemo_hip as J
    h = re.sub(r"/\*.*?\*/", "", _read("include", "jchemo_hip.h"), flags=re.S)
    m = re.search(r"JCH_API\s+(\w+)\s+jch_knn_wls\s*\(([^;]*?)\)\s*;", h, flags=re.S)
    assert m and m.group(1) == "int32_t"
    assert len(m.group(2).split(",")) == 17
    assert "jch_knn_wls" in J.SYMBOLS and len(J.SYMBOLS) == len(set(J.SYMBOLS))
    assert len(J.load().jch_knn_wls.argtypes) == 17
    srcs = re.search(r"^SRCS := (.*)$", _read("jchemo.jl_amd", "csrc", "Makefile"), flags=re.M).group(1).split()
    assert "lwmlr.hip" in srcs
    src = _read("jchemo.jl_amd", "csrc", "lwmlr.hip")
    assert "asm" not in src and "atomic" not in src.replace("no atomics", "")
    full = _read("include", "jchemo_hip.h")
    assert "minimum-norm" in full and "150 KiB" in full and "info[i] = 2" in full      # the special cases and the threshold are part of the contract
    lds_max = importlib.import_module("jchemo_hip.lwmlr").WLS_LDS_MAX
    assert "WLS_LDS_MAX (150 * 1024)" in src and lds_max == 150 * 1024
    assert J.knn_wls_lds_bytes(900, 24, 2) > lds_max > J.knn_wls_lds_bytes(100, 20, 1)
    assert J.knn_wls_lds_bytes(100, 20, 1) == 8 * (21 * 101 + 200 + 21 + 40 + 50)


def test_python_package_exports_fields_and_defaults():
    import jchemo_hip as J
    for name in ("knn_wls", "Lwmlr", "LwmlrS", "Lwmlrda", "LwmlrdaS", "lwmlr", "lwmlr_s", "lwmlrda", "lwmlrda_s", "lwmlr_predict", "lwmlr_s_predict",
                 "lwmlrda_predict", "lwmlrda_s_predict"):
        assert hasattr(J, name), name
    assert [f.name for f in dataclasses.fields(J.Lwmlr)] == ["X", "Y", "metric", "h", "k", "tol", "verbose"]               # src/lwmlr.jl:1-9
    assert [f.name for f in dataclasses.fields(J.LwmlrS)] == ["T", "Y", "fm", "metric", "h", "k", "tol", "verbose"]        # src/lwmlr_s.jl:1-10
    assert [f.name for f in dataclasses.fields(J.Lwmlrda)] == ["X", "y", "metric", "h", "k", "tol", "verbose"]             # src/lwmlrda.jl:1-9
    assert [f.name for f in dataclasses.fields(J.LwmlrdaS)] == ["T", "y", "fm", "metric", "h", "k", "tol", "verbose"]      # src/lwmlrda_s.jl:1-10

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not v.empty and k not in ("ctx", "seed")}

    def required(fn):
        return [k for k, v in inspect.signature(fn).parameters.items() if v.default is v.empty]
    assert defaults(J.lwmlr) == dict(metric="eucl", tol=1e-4, verbose=False) and required(J.lwmlr) == ["X", "Y", "h", "k"]
    assert defaults(J.lwmlrda) == dict(metric="eucl", tol=1e-4, verbose=False) and required(J.lwmlrda) == ["X", "y", "h", "k"]
    want = dict(reduc="pls", metric="eucl", gamma=1, psamp=1, samp="sys", tol=1e-4, scal=False, verbose=False)
    assert defaults(J.lwmlr_s) == want and required(J.lwmlr_s) == ["X", "Y", "nlv", "h", "k"]
    assert defaults(J.lwmlrda_s) == dict(want, samp="cla") and required(J.lwmlrda_s) == ["X", "y", "nlv", "h", "k"]
    assert list(inspect.signature(J.lwmlr_s).parameters)[:13] == ["X", "Y", "nlv", "reduc", "metric", "h", "k", "gamma", "psamp", "samp", "tol", "scal", "verbose"]
    sig = inspect.signature(J.knn_wls)
    assert list(sig.parameters) == ["X", "Y", "Xq", "ind", "w", "info", "ctx"] and sig.parameters["info"].default is False
    assert [f.name for f in dataclasses.fields(J.KnnPred)] == ["pred", "listnn", "listd", "listw"]


def test_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    X = np.zeros((8, 2), order="F"); Y = np.zeros((8, 1), order="F"); y = np.arange(8) % 2
    for bad in (dict(metric="manhattan", h=2, k=3), dict(h=2, k=0), dict(h=0, k=3), dict(h=-1.0, k=3), dict(h=2, k=2.5)):
        for fn, resp in ((J.lwmlr, Y), (J.lwmlrda, y)):
            with pytest.raises(ValueError):
                fn(X, resp, **bad)
        for fn, resp in ((J.lwmlr_s, Y), (J.lwmlrda_s, y)):
            with pytest.raises(ValueError):
                fn(X, resp, nlv=1, **bad)
    with pytest.raises(ValueError):
        J.lwmlr(X, np.zeros((7, 1)), h=2, k=3)
    with pytest.raises(ValueError):
        J.lwmlrda(X, y[:5], h=2, k=3)
    for kw in (dict(reduc="svd"), dict(samp="cla"), dict(samp="other"), dict(psamp=0), dict(psamp=1.5), dict(nlv=0)):
        with pytest.raises(ValueError):
            J.lwmlr_s(X, Y, **dict(dict(nlv=1, h=2, k=3), **kw))
    for kw in (dict(reduc="svd"), dict(samp="sys"), dict(samp="other"), dict(psamp=0)):
        with pytest.raises(ValueError):
            J.lwmlrda_s(X, y, **dict(dict(nlv=1, h=2, k=3), **kw))
    ind = np.zeros((3, 2), dtype=np.int32); w = np.ones((3, 2))
    with pytest.raises(ValueError):
        J.knn_wls(X, Y, np.zeros((3, 3), order="F"), ind, w)            # mismatched columns
    with pytest.raises(ValueError):
        J.knn_wls(X, Y[:5], np.zeros((3, 2), order="F"), ind, w)        # mismatched rows
    with pytest.raises(ValueError):
        J.knn_wls(X, Y, np.zeros((4, 2), order="F"), ind, w)            # lists for another number of queries
    with pytest.raises(ValueError):
        J.knn_wls(X, Y, np.zeros((3, 2), order="F"), ind, np.ones((3, 3)))
    fm = J.lwmlr(X, Y, h=2, k=3)
    with pytest.raises(ValueError):
        J.lwmlr_predict(fm, np.zeros((2, 3), order="F"))                # mismatched columns
    fm.metric = "manhattan"
    with pytest.raises(ValueError):
        J.lwmlr_predict(fm, np.zeros((2, 2), order="F"))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(TypeError):
            J.lwmlr(torch.zeros(8, 2, dtype=torch.float64), Y, h=2, k=3)   # a host tensor; host / device mix


def test_no_cpu_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import jchemo_hip as J
    c = case(4)
    calls = [lambda: J.knn_wls(c["X"], c["Y"], c["Xq"], c["ind"], c["w"]),
             lambda: J.lwmlr_predict(J.lwmlr(c["X"], c["Y"][:, :1], h=2, k=7), c["Xq"]),
             lambda: J.lwmlrda_predict(J.lwmlrda(c["X"], c["yv"], h=2, k=7), c["Xq"]),
             lambda: J.lwmlr_s(c["X"], c["Y"][:, :1], nlv=2, h=2, k=7),
             lambda: J.lwmlrda_s(c["X"], c["yv"], nlv=2, h=2, k=7)]
    for f in calls:
        with pytest.raises(J.JchError) as ei:
            f()
        assert ei.value.code == J._lib.JCH_ENODEV


def test_julia_module_has_the_names_and_calls_the_entry():
    src = _read("jchemo.jl_amd", "julia", "JchemoHIP.jl")
    exported = set(re.findall(r"[\w!]+", re.search(r"\nexport (.*?)\n\n", src, flags=re.S).group(1)))
    for nm in ("lwmlr", "lwmlr_s", "lwmlrda", "lwmlrda_s", "Lwmlr", "LwmlrS", "Lwmlrda", "LwmlrdaS", "knn_wls"):
        assert nm in exported, nm
        assert re.search(r"(^|\n)\s*(function\s+|struct\s+)" + nm + r"\b", src), nm
    assert "(:jch_knn_wls, LIB)" in src
    for nm in ("Lwmlr", "LwmlrS", "Lwmlrda", "LwmlrdaS"):
        assert re.search(r"function predict\(object::" + nm + r",", src), nm
    assert "NOT EXECUTED" in src


def test_documents_describe_the_entry():
    design = _read("DESIGN.md")
    assert "## 23." in design and "jch_knn_wls" in design and "minimum-norm" in design and "local levels" in design
    assert "jch_knn_wls" in _read("INTEGRATION.md") and "lwmlr" in _read("README.md")
