"""jch_knn_search, jch_knn_wmean, jch_knn_vote, jch_knn_gather_median and getknn / knnr / knnda / occknndis / occlknndis on the GPU.

The primitive is checked through the C ABI on an integer lattice (entries in -8 .. 8, blocks of duplicate rows): every squared distance is then exact
in Float64 whatever the summation order, so neighbours and distances must EQUAL the oracle's, ties included.  The models are checked against the
literal numpy restatements of tests/test_knn_static.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import plsr_oracle as O  # noqa: E402
from test_knn_static import (MAHAL_CASE, MAX_SKIP, U, WMEAN_SHAPES, classes_of, comparable_queries, lattice, lattice_queries, latent,  # noqa: E402
                             mahal_case_reference, np_knnda_predict, np_knnr_predict, np_middle_median, np_occknndis, np_occknndis_predict,
                             np_occlknndis, np_occlknndis_predict, np_weights, np_wmean, wmean_bound, wmean_inputs)

SENT = 7.0
ISENT = -77


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


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _dev_colmajor(A, ld, offset):
    """A device copy of A with leading dimension ld whose first element sits `offset` doubles behind an allocation's start; sentinels elsewhere."""
    n, c = A.shape
    buf = torch.full((offset + ld * max(c, 1),), SENT, dtype=torch.float64, device="cuda:0")
    V = buf[offset:offset + ld * c].view(c, ld).t()
    V[:n].copy_(torch.as_tensor(np.array(A), device="cuda:0"))
    return V, buf.data_ptr() + 8 * offset, ld


# ---------------------------------------------------------------------------------- a. jch_knn_search through the C ABI
H, TOL = 2.0, 1e-4


def prim_data(n, dd, m):
    Zt = lattice(n, dd, seed=n + dd)
    return np.asfortranarray(Zt), np.asfortranarray(lattice_queries(Zt, m, seed=m + dd))


def _ref_with(Zt, Zq, k, sr=None, h=H, tol=TOL):
    """The oracle's lists: getknn over all rows, or over rmrow(Zt, s) with the rows mapped back; wdist weights clamped to tol; the median."""
    n, m = Zt.shape[0], Zq.shape[0]
    kk = min(k, n if sr is None else n - 1)
    ind, d = np.empty((m, kk), dtype=np.int64), np.empty((m, kk))
    for i in range(m):
        if sr is not None and sr[i] >= 0:
            ii, dd_ = O.getknn(O.rmrow(Zt, [sr[i]]), Zq[i:i + 1], k=kk)
            ind[i], d[i] = ii[0] + (ii[0] >= sr[i]), dd_[0]
        else:
            ii, dd_ = O.getknn(Zt, Zq[i:i + 1], k=kk)
            ind[i], d[i] = ii[0], dd_[0]
    w = np.stack([np_weights(d[i], h, tol) for i in range(m)])
    return ind, d, w, np.array([np_middle_median(d[i]) for i in range(m)])


def self_rows(Zt, Zq, kind):
    """None; "own": the training row the query is a copy of (its first copy; -1 for a fresh query); "all": a row for every query, for the
    queries that are no copy a row that is not among their neighbours (the farthest row)."""
    if kind is None:
        return None
    m = Zq.shape[0]
    sr = np.full(m, -1, dtype=np.int64)
    for i in range(m):
        d2 = ((Zt - Zq[i]) ** 2).sum(axis=1)
        hit = np.nonzero(d2 == 0)[0]
        if hit.size:
            sr[i] = hit[-1] if i % 2 else hit[0]                        # the last copy sits behind all the others: often not among the k + 1
        elif kind == "all":
            sr[i] = int(np.argmax(d2))
    return sr


def run_search(J, ctx, Zt, Zq, k, sr=None, mode="host", h=H, tol=TOL, want=(True, True, True, True)):
    """(ind, dist, w, dmed) as host arrays through the C ABI; mode: "host", "dev" (aligned device arrays) or "dev1" (the query block one double
    off an allocation's start with an odd leading dimension).  The entry behind every output must keep its sentinel."""
    lib = J.load()
    n, dd = Zt.shape
    m = Zq.shape[0]
    kk = min(k, n if sr is None else n - 1)
    hnd = C.c_void_p()
    if mode == "host":
        ctx.check(lib.jch_knn_prepare(ctx._h, 0, Zt.ctypes.data, n, dd, n, C.byref(hnd)))
    else:
        Vt, ta, ldt = _dev_colmajor(Zt, n + 3, 0)
        torch.cuda.synchronize()
        ctx.check(lib.jch_knn_prepare(ctx._h, 1, ta, n, dd, ldt, C.byref(hnd)))
    try:
        if mode == "host":
            ind = np.full(m * kk + 1, ISENT, dtype=np.int32); dist = np.full(m * kk + 1, SENT); w = np.full(m * kk + 1, SENT); dmed = np.full(m + 1, SENT)
            ptr = lambda a, on: a.ctypes.data if on else None  # noqa: E731
            ctx.check(lib.jch_knn_search(ctx._h, hnd, 0, Zq.ctypes.data, m, m, k, None if sr is None else sr.ctypes.data, h, tol, 0,
                                         ptr(ind, want[0]), ptr(dist, want[1]), ptr(w, want[2]), ptr(dmed, want[3])))
            outs = [ind, dist, w, dmed]
        else:
            Vq, qa, ldq = _dev_colmajor(Zq, m + 2 + m % 2, 0) if mode == "dev" else _dev_colmajor(Zq, m + 1 + m % 2, 1)
            ind = torch.full((m * kk + 1,), ISENT, dtype=torch.int32, device="cuda:0")
            dist, w = (torch.full((m * kk + 1,), SENT, dtype=torch.float64, device="cuda:0") for _ in range(2))
            dmed = torch.full((m + 1,), SENT, dtype=torch.float64, device="cuda:0")
            srd = None if sr is None else torch.as_tensor(sr, device="cuda:0")
            torch.cuda.synchronize()
            ptr = lambda a, on: a.data_ptr() if on else None  # noqa: E731
            ctx.check(lib.jch_knn_search(ctx._h, hnd, 1, qa, m, ldq, k, None if sr is None else srd.data_ptr(), h, tol, 1,
                                         ptr(ind, want[0]), ptr(dist, want[1]), ptr(w, want[2]), ptr(dmed, want[3])))
            ctx.synchronize()
            assert np.array_equal(_host(Vq[:m]), Zq) and bool((Vq[m:] == SENT).all())     # the queries and the padding behind them are only read
            outs = [_host(a) for a in (ind, dist, w, dmed)]
    finally:
        lib.jch_knn_release(ctx._h, hnd)
    sizes = [m * kk, m * kk, m * kk, m]
    res = []
    for pos, (a, sz, on, sent) in enumerate(zip(outs, sizes, want, [ISENT, SENT, SENT, SENT])):
        assert a[sz] == sent                                              # nothing behind the output was written
        if not on:
            assert np.all(a == sent)
        res.append(a[:sz].reshape(m, kk) if pos < 3 else a[:sz])
    return res


def check_lists(got, ref):
    ind, d, w, dmed = got
    rind, rd, rw, rmed = ref
    assert np.array_equal(ind, rind)
    assert np.array_equal(d, rd)
    assert O.rel_fro(rw, w) < 1e-7
    assert np.all(np.abs(dmed - rmed) <= 4 * U * np.abs(rmed))


# (n, dd, m, k): k and k + 1 at the clamp; two scan segments with 692 copies of one row; the envelope edge into k_knn_generic (k <= 768 scans);
# the screen's edge in dd; a wide space; one query; m no multiple of the scan's 4 queries per workgroup
PRIM_CASES = [(300, 3, 5, 1), (300, 3, 5, 299), (300, 3, 5, 300), (9000, 10, 6, 100), (5000, 7, 9, 767), (5000, 7, 9, 768), (5000, 7, 9, 800),
              (4000, 62, 5, 20), (4000, 63, 5, 20), (3000, 500, 4, 10), (300, 3, 1, 7)]


@pytest.mark.parametrize("n,dd,m,k", PRIM_CASES)
def test_search_equals_the_oracle_on_a_lattice(n, dd, m, k, J, ctx):
    Zt, Zq = prim_data(n, dd, m)
    if (n, k) == (9000, 100):                                             # the ties case of test_lwplsr_knn_ties_and_duplicates: query 0 is the copied row
        Zq[0] = Zt[5]
    ref = _ref_with(Zt, Zq, k)
    if (n, k) == (9000, 100):                                             # ... and its neighbours are the first k copies, in row order
        copies = np.nonzero((Zt == Zt[5]).all(axis=1))[0]
        assert copies.size > 512 and np.array_equal(ref[0][0], copies[:k])
    host = run_search(J, ctx, Zt, Zq, k)
    check_lists(host, ref)
    for mode in ("dev", "dev1"):
        got = run_search(J, ctx, Zt, Zq, k, mode=mode)
        for a, b in zip(got, host):
            assert np.array_equal(a, b), mode                             # host and device inputs, aligned or not: the same bits


def test_outputs_may_be_null_and_h_may_be_infinite(J, ctx):
    Zt, Zq = prim_data(300, 3, 5)
    full = run_search(J, ctx, Zt, Zq, 12)
    for want in [(True, False, False, False), (False, True, False, True), (False, False, True, False), (False, False, False, True)]:
        for mode in ("host", "dev"):
            got = run_search(J, ctx, Zt, Zq, 12, mode=mode, want=want)
            for a, b, on in zip(got, full, want):
                assert not on or np.array_equal(a, b), (want, mode)
    inf = run_search(J, ctx, Zt, Zq, 12, h=float("inf"), tol=1e-4)
    assert np.all(inf[2] == 1.0) and np.array_equal(inf[0], full[0])      # h = Inf: exp(-0) = 1 everywhere


# self removal: k + 1 = n with every query carrying a row; the scan's edge (k + 1 = 768) and the first k + 1 beyond it; a k beyond the
# LDS lists of the finishing kernel (the any-address-space route)
SELF_CASES = [(300, 3, 5, 299, "all"), (300, 3, 5, 4, "own"), (5000, 7, 9, 100, "all"), (5000, 7, 9, 100, "own"), (5000, 7, 9, 767, "all"),
              (5000, 7, 9, 768, "all"), (3000, 4, 3, 1500, "all")]


@pytest.mark.parametrize("n,dd,m,k,kind", SELF_CASES)
def test_self_removal_equals_the_search_over_the_row_removed_matrix(n, dd, m, k, kind, J, ctx):
    Zt, Zq = prim_data(n, dd, m)
    if n == 5000:
        Zq[1] = Zt[5]                                                     # a query on the row with 380 copies: its last copy sits behind all the others
    sr = self_rows(Zt, Zq, kind)
    assert (sr >= 0).any() and (kind == "own" or (sr >= 0).all())
    ref = _ref_with(Zt, Zq, k, sr)
    plain = _ref_with(Zt, Zq, k)[0]
    absent = [i for i in range(m) if sr[i] >= 0 and sr[i] not in plain[i] and sr[i] not in O.getknn(Zt, Zq[i:i + 1], k=min(k + 1, n))[0][0]]
    assert absent or n == 300                                             # some removed row is not among the k + 1: the last entry goes
    host = run_search(J, ctx, Zt, Zq, k, sr)
    check_lists(host, ref)
    dev = run_search(J, ctx, Zt, Zq, k, sr, mode="dev1")
    for a, b in zip(dev, host):
        assert np.array_equal(a, b)


def test_a_nan_query_stays_in_its_query(J, ctx):
    Zt, Zq = prim_data(5000, 7, 9)
    clean = run_search(J, ctx, Zt, Zq, 20)
    Zn = Zq.copy(order="F")
    Zn[4, 2] = np.nan
    for sr in (None, self_rows(Zt, Zq, "all")):
        ref = run_search(J, ctx, Zt, Zq, 20, sr) if sr is not None else clean
        got = run_search(J, ctx, Zt, Zn, 20, sr)
        ind, d, w, dmed = got
        assert np.all(np.isnan(d[4])) and np.isnan(dmed[4]) and np.all(w[4] == 1.0)
        assert np.all((ind[4] >= 0) & (ind[4] < Zt.shape[0]))
        keep = np.arange(9) != 4
        for a, b in zip(got, ref):
            assert np.array_equal(a[keep], b[keep])


_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {pkg!r}); sys.path.insert(0, {tests!r})
import numpy as np
import jchemo_hip as J
import test_gpu_knn as T
ctx = J.Context(0)
Zt, Zq = T.prim_data({n}, {dd}, {m})
sr = T.self_rows(Zt, Zq, "own")
a = T.run_search(J, ctx, Zt, Zq, {k})
b = T.run_search(J, ctx, Zt, Zq, {k}, sr)
np.savez({out!r}, *a, *b)
ctx.close()
"""


@pytest.mark.parametrize("knob", ["JCH_KNN_SCREEN=0", "JCH_KNN_GENERIC=1"])
def test_the_knobs_choose_another_path_and_the_same_result(knob, J, ctx, tmp_path):
    """The knobs are read from the environment by the library: a fresh child process each.  (4000, 62, 5, 20) is inside the screen's envelope."""
    n, dd, m, k = 4000, 62, 5, 20
    Zt, Zq = prim_data(n, dd, m)
    sr = self_rows(Zt, Zq, "own")
    here = run_search(J, ctx, Zt, Zq, k) + run_search(J, ctx, Zt, Zq, k, sr)
    out = str(tmp_path / "child.npz")
    env = dict(os.environ)
    name, val = knob.split("=")
    env[name] = val
    code = _CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "jchemo.jl_amd"), tests=os.path.join(ROOT, "tests"), n=n, dd=dd, m=m, k=k, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    there = np.load(out)
    for i, a in enumerate(here):
        assert np.array_equal(a, there[f"arr_{i}"]), (knob, i)


# ---------------------------------------------------------------------------------- b. the reductions over given lists
def _both(a, dev, colmajor=False):
    if not dev:
        return a
    if colmajor:
        import jchemo_hip as J
        t = J.colmajor_empty(a.shape[0], a.shape[1], "cuda:0"); t.copy_(torch.as_tensor(a)); return t
    return torch.as_tensor(a, device="cuda:0")


@pytest.mark.parametrize("n,q,m,k", WMEAN_SHAPES)
def test_wmean_within_its_bound(n, q, m, k, J, ctx):
    Y, ind, w = wmean_inputs(n, q, m, k, seed=n + k)
    ref = np_wmean(Y, ind, w, np.longdouble).astype(np.float64)
    bound = wmean_bound(Y, ind, w)
    host = J.knn_wmean(Y, ind, w, ctx=ctx)
    assert host.shape == (m, q) and np.all(np.abs(host - ref) <= bound)
    dev = _host(J.knn_wmean(_both(Y, True, True), _both(ind, True), _both(w, True), ctx=ctx))
    assert np.array_equal(dev, host) and np.array_equal(J.knn_wmean(Y, ind, w, ctx=ctx), host)     # fixed order: the same bits every time
    Yn = Y.copy(order="F")
    Yn[ind[1, 0], 0] = np.nan                                             # a NaN response reaches the queries that gather it, and only them
    got = J.knn_wmean(Yn, ind, w, ctx=ctx)
    hit = (ind == ind[1, 0]).any(axis=1)
    assert np.all(np.isnan(got[hit, 0])) and np.array_equal(got[~hit], host[~hit]) and np.array_equal(got[:, 1:], host[:, 1:])


def np_vote(cls, ncls, ind, w):
    m, k = ind.shape
    score = np.zeros((m, ncls))
    pred = np.empty(m, dtype=np.int64)
    for i in range(m):
        present = np.zeros(ncls, dtype=bool)
        for j in range(k):                                                # in neighbour order
            score[i, cls[ind[i, j]]] += w[i, j]
            present[cls[ind[i, j]]] = True
        cand = np.nonzero(present)[0]
        pred[i] = cand[int(np.argmax(score[i, cand]))]                    # the first maximum among the classes present: the lowest code
    return pred, score


@pytest.mark.parametrize("ncls,k", [(2, 5), (7, 64), (7, 300), (300, 65), (3000, 9)])
def test_vote_exact_classes_and_ties(ncls, k, J, ctx):
    rng = np.random.default_rng(ncls + k)
    n, m = 4000, 23
    cls = rng.integers(0, ncls, size=n).astype(np.int32)
    if ncls > 2:
        cls[cls == ncls - 1] = 0                                          # the last class never occurs
    lo, hi = (1, 2) if ncls > 2 else (0, 1)
    cls[:2], cls[2:4] = lo, hi
    ind = rng.integers(0, n, size=(m, k)).astype(np.int32)
    w = rng.integers(1, 9, size=(m, k)) / 8.0                             # dyadic rationals: every sum is exact, ties are exact ties
    # query 0: two classes tie at 0.75, the higher code first in the list; query 1: all weights zero — the lowest PRESENT class wins, not class 0
    if k >= 4:
        ind[0, :4] = [2, 0, 3, 1]; w[0] = 0.0; w[0, :4] = [.5, .25, .25, .5]
    top = np.nonzero(cls == cls.max())[0]
    ind[1] = top[rng.integers(0, top.size, size=k)]; w[1] = 0.0
    rp, rs = np_vote(cls, ncls, ind, w)
    if k >= 4:
        assert rs[0, lo] == rs[0, hi] == 0.75 and rp[0] == lo
    assert rp[1] == cls.max() and cls.max() > 0
    pred, score = J.knn_vote(cls, ncls, ind, w, score=True, ctx=ctx)
    assert np.array_equal(pred, rp)
    assert np.array_equal(score, rs)                                      # exact sums (the bound (k + 2) 2^-53 sum w holds with zero error)
    assert ncls == 2 or (np.all(score[:, ncls - 1] == 0) and ncls - 1 not in pred)
    pd, sd = J.knn_vote(_both(cls, True), ncls, _both(ind, True), _both(w, True), score=True, ctx=ctx)
    assert np.array_equal(_host(pd), pred) and np.array_equal(_host(sd), score)
    # inexact weights: the scores within (k + 2) 2^-53 sum_j w_ij of the sums in neighbour order taken in extended precision
    w2 = np.maximum(np.exp(-rng.uniform(0, 12, size=(m, k))), 1e-4)
    p2, s2 = J.knn_vote(cls, ncls, ind, w2, score=True, ctx=ctx)
    ref2 = np.zeros((m, ncls), dtype=np.longdouble)
    for i in range(m):
        np.add.at(ref2[i], cls[ind[i]], w2[i].astype(np.longdouble))
    assert np.all(np.abs(s2 - ref2.astype(np.float64)) <= (k + 2) * U * w2.sum(axis=1, keepdims=True))
    assert np.array_equal(J.knn_vote(cls, ncls, ind, w2, ctx=ctx), p2)


@pytest.mark.parametrize("k", [1, 2, 7, 8, 1024, 1025, 1500])
def test_gather_median_equals_numpy(k, J, ctx):
    rng = np.random.default_rng(k)
    n, m = 5000, 11
    v = rng.standard_normal(n)
    v[17] = np.nan
    ind = rng.integers(0, n, size=(m, k)).astype(np.int32)
    ind[2, k // 2] = 17                                                   # one NaN: it sorts last
    ind[3, :] = 17 if k < 3 else ind[3, :]                                # (small k: the middle place itself is NaN)
    ind[4, :(k + 1) // 2 + 1] = 17                                        # more than half NaN: the median is NaN
    ref = np.array([np_middle_median(np.sort(v[ind[i]])) for i in range(m)])      # numpy sorts NaN last as well
    got = J.knn_gather_median(v, ind, ctx=ctx)
    assert np.array_equal(got, ref, equal_nan=True) and np.isnan(got[4]) and (k < 3 or not np.isnan(got[2]))
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    dev = _host(J.knn_gather_median(_both(v, True), _both(ind, True), ctx=ctx))
    assert np.array_equal(dev, got, equal_nan=True)


# ---------------------------------------------------------------------------------- c. the models against the restatements
def _dev(A):
    import jchemo_hip as J
    A = np.asarray(A, dtype=np.float64)
    A = A.reshape(-1, 1) if A.ndim == 1 else A
    t = J.colmajor_empty(A.shape[0], A.shape[1], "cuda:0")
    t.copy_(torch.as_tensor(A))
    return t


@pytest.mark.parametrize("metric", ["eucl", "mahal"])
def test_getknn(metric, J, ctx):
    X, Xq, _ = latent(800, 12, 40, 8, seed=3)
    k = 25
    rind, rd = O.getknn(X, Xq, k=k, metric=metric)
    ok = comparable_queries(O.getknn(X, Xq, k=k + 1, metric=metric)[1])
    assert 1.0 - ok.mean() <= MAX_SKIP
    ind, d = J.getknn(X, Xq, k=k, metric=metric, ctx=ctx)
    assert ind.dtype == np.int32 and ind.shape == (40, k)
    assert np.array_equal(ind[ok], rind[ok]) and np.all(np.abs(d[ok] - rd[ok]) <= 1e-9 * rd[ok])
    di, dd = J.getknn(_dev(X), _dev(Xq), k=k, metric=metric, ctx=ctx)
    assert isinstance(di, torch.Tensor) and np.array_equal(_host(di), ind) and np.array_equal(_host(dd), d)
    assert J.getknn(X, Xq, k=5000, metric=metric, ctx=ctx)[0].shape == (40, 800)        # k clamps to n (src/getknn.jl:33)


@pytest.mark.parametrize("scal", [False, True])
@pytest.mark.parametrize("h", [np.inf, 2.0])
def test_knnr_and_knnda_on_a_lattice(scal, h, J, ctx):
    """scal = false: every distance is exact, so lists and distances equal the restatement's.  scal = true: the scaled distances are rounded, but
    copies of a row still tie to the last bit (and are ordered by row), while two DIFFERENT rows at the same scaled distance from a query would need
    the same |difference| in all 12 columns: the neighbour lists stay equal, the distances agree to rounding."""
    n, p, m, k = 1000, 12, 40, 30
    X = lattice(n, p, 8)
    Xq = lattice_queries(X, m, 9)
    rng = np.random.default_rng(10)
    Y = np.column_stack([X[:, :3] @ np.array([1.0, -2.0, 0.5]) + rng.standard_normal(n), rng.standard_normal(n)])
    ycl = classes_of(Y[:, 0], 5)
    kw = dict(nlvdis=0, metric="eucl", h=h, k=k, scal=scal)
    ref = np_knnr_predict(X, Y, Xq, **kw)
    fm = J.knnr(X, Y, ctx=ctx, **kw)
    res = J.predict(fm, Xq, ctx=ctx)
    assert np.array_equal(res.listnn, ref["listnn"])
    assert np.array_equal(res.listd, ref["listd"]) if not scal else O.rel_fro(ref["listd"], res.listd) < 1e-9
    assert O.rel_fro(ref["listw"], res.listw) < 1e-7 and O.rel_fro(ref["pred"], res.pred) < 1e-7
    assert np.array_equal(J.predict(fm, Xq, ctx=ctx).pred, res.pred)      # the cached handle: the same bits
    fd = J.knnr(_dev(X), _dev(Y), ctx=ctx, **kw)
    rd = J.predict(fd, _dev(Xq), ctx=ctx)
    assert isinstance(rd.pred, torch.Tensor)
    assert np.array_equal(_host(rd.listnn), res.listnn) and np.array_equal(_host(rd.listw), res.listw) and np.array_equal(_host(rd.pred), res.pred)
    refc = np_knnda_predict(X, ycl, Xq, **kw)
    fc = J.knnda(X, ycl, ctx=ctx, **kw)
    assert np.array_equal(fc.lev, np.unique(ycl)) and np.array_equal(fc.ni, np.bincount(ycl))
    rc = J.predict(fc, Xq, ctx=ctx)
    assert np.array_equal(rc.listnn, refc["listnn"]) and np.array_equal(rc.pred, refc["pred"])
    rcd = J.predict(J.knnda(_dev(X), ycl, ctx=ctx, **kw), _dev(Xq), ctx=ctx)
    assert np.array_equal(rcd.pred, rc.pred)


@pytest.mark.parametrize("kind", ["knnr", "knnda"])
def test_knnr_and_knnda_in_the_whitened_score_space(kind, J, ctx):
    c = MAHAL_CASE
    X, Xq, y, ok, ref = mahal_case_reference(kind)
    assert 1.0 - ok.mean() <= MAX_SKIP
    kw = dict(nlvdis=c["nlvdis"], metric="mahal", h=c["h"], k=c["k"])
    fm = (J.knnr if kind == "knnr" else J.knnda)(X, y, ctx=ctx, **kw)
    res = J.predict(fm, Xq, ctx=ctx)
    assert np.array_equal(res.listnn[ok], ref["listnn"][ok])
    assert np.all(np.abs(res.listd[ok] - ref["listd"][ok]) <= 1e-9 * ref["listd"][ok])
    assert O.rel_fro(ref["listw"][ok], res.listw[ok]) < 1e-7
    if kind == "knnr":
        assert O.rel_fro(ref["pred"][ok], res.pred[ok]) < 1e-7
    else:
        assert np.array_equal(res.pred[ok], ref["pred"][ok])
    rd = J.predict((J.knnr if kind == "knnr" else J.knnda)(_dev(X), _dev(y) if kind == "knnr" else y, ctx=ctx, **kw), _dev(Xq), ctx=ctx)
    assert np.array_equal(_host(rd.listnn)[ok], res.listnn[ok])
    assert O.rel_fro(_host(res.pred)[ok].astype(float), _host(rd.pred)[ok].astype(float)) < 1e-9


def occ_inputs():
    rng = np.random.default_rng(21)
    n, p, m, a = 800, 20, 34, 6
    L = rng.standard_normal((a, p))
    X = rng.standard_normal((n, a)) * np.array([3.0, 2.5, 2.0, 1.5, 1.2, 1.0]) @ L + 0.1 * rng.standard_normal((n, p))
    Xq = rng.standard_normal((m, a)) * np.array([3.0, 2.5, 2.0, 1.5, 1.2, 1.0]) @ L + 0.1 * rng.standard_normal((m, p))
    Xq[::4] *= 2.5
    samp = rng.choice(n, size=60, replace=False)
    return np.asfortranarray(X), np.asfortranarray(np.vstack([Xq, X[:6]])), samp      # held-out rows, then training rows


def _fm_dict(fm):
    return dict(T=_host(fm.T), P=np.asarray(fm.P), xmeans=np.asarray(fm.xmeans), xscales=np.asarray(fm.xscales))


def check_occ(got_fit, got_pred, ref_fit, ref_pred):
    close = lambda a, b: np.all(np.abs(_host(a) - b) <= 1e-9 * np.abs(b))  # noqa: E731
    assert abs(got_fit.cutoff - ref_fit["cutoff"]) <= 1e-9 * ref_fit["cutoff"]
    for tab, ref in ((got_fit.d, ref_fit["d"]), (got_pred.d, ref_pred["d"])):
        assert close(tab["d"], ref["d"]) and close(tab["dstand"], ref["dstand"])
        clear = np.abs(ref["dstand"] - 1) > 1e-9
        assert np.array_equal(_host(tab["pval"])[clear], ref["pval"][clear])
    clear = np.abs(ref_pred["d"]["dstand"] - 1) > 1e-9
    assert np.array_equal(_host(got_pred.pred)[clear], ref_pred["pred"][clear])
    assert set(np.unique(ref_pred["pred"])) == {0, 1}


@pytest.mark.parametrize("typc", ["mad", "q"])
def test_occknndis(typc, J, ctx):
    X, Xq, samp = occ_inputs()
    obj = J.occknndis(X, nlv=6, k=7, samp=samp, typc=typc, ctx=ctx)
    ref = np_occknndis(X, nlv=6, samp=samp, k=7, typc=typc, fm=_fm_dict(obj.fm))
    assert np.all(np.abs(obj.tscales - ref["tscales"]) <= 1e-12 * ref["tscales"])
    got = J.predict(obj, Xq, ctx=ctx)
    check_occ(obj, got, ref, np_occknndis_predict(ref, Xq))
    od = J.occknndis(_dev(X), nlv=6, k=7, samp=samp, typc=typc, ctx=ctx)
    gd = J.occ_predict(od, _dev(Xq), ctx=ctx)
    assert isinstance(gd.d["d"], torch.Tensor)
    assert O.rel_fro(_host(got.d["d"]), _host(gd.d["d"])) < 1e-12 and np.array_equal(_host(gd.pred), got.pred)


@pytest.mark.parametrize("typc,reading", [("mad", "literal"), ("q", "doc"), ("mad", "doc"), ("q", "literal")])
def test_occlknndis(typc, reading, J, ctx):
    X, Xq, samp = occ_inputs()
    obj = J.occlknndis(X, nlv=6, k=5, samp=samp, typc=typc, reading=reading, ctx=ctx)
    ref = np_occlknndis(X, nlv=6, samp=samp, k=5, typc=typc, reading=reading, fm=_fm_dict(obj.fm))
    got = J.predict(obj, Xq, ctx=ctx)
    check_occ(obj, got, ref, np_occlknndis_predict(ref, Xq))
    warm = J.predict(obj, Xq, ctx=ctx)                                    # from the warm cache: the same bits
    for col in ("d", "dstand", "pval"):
        assert np.array_equal(warm.d[col], got.d[col])
    assert np.array_equal(warm.pred, got.pred)
    od = J.occlknndis(_dev(X), nlv=6, k=5, samp=samp, typc=typc, reading=reading, ctx=ctx)
    gd = J.predict(od, _dev(Xq), ctx=ctx)
    assert isinstance(gd.d["d"], torch.Tensor)
    assert O.rel_fro(_host(got.d["d"]), _host(gd.d["d"])) < 1e-12 and np.array_equal(_host(gd.pred), got.pred)


# ---------------------------------------------------------------------------------- the three routes of the C entries (tests/host_routes.py)
@pytest.mark.parametrize("entry", sorted(__import__("host_routes").ROUTES["knn"]))
def test_host_arrays_padded_and_unpadded_give_the_bits_of_the_device_route(entry):
    """Device buffers, host arrays with ld == rows and with ld = rows + 3 between NaN guards: equal bytes, NaN padding kept, inputs unchanged."""
    import host_routes as HR
    HR.three_routes(HR.ROUTES["knn"][entry])
