"""CPU-side checks of the kNN family: literal numpy restatements of the reference's src/knnr.jl, src/knnda.jl, src/occknndis.jl and src/occlknndis.jl
(shared with tests/test_gpu_knn.py), the argument that lets jch_knn_search remove a training row without a row-removed copy, the cached form of
occlknndis' predict, the error bound of jch_knn_wmean, and the boundary (header, SYMBOLS, exports)."""
import dataclasses
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
from test_occ_static import np_cutoff, np_median, np_pval  # noqa: E402
from test_pca_static import np_pca_transform, np_pcasvd  # noqa: E402

U = 2.0 ** -53


# ---------------------------------------------------------------------------------- numpy restatements of the reference
def np_middle_median(s):
    """`median` of a SORTED vector with Julia's middle(lo, hi) = lo / 2 + hi / 2 for an even length."""
    s = np.asarray(s, dtype=np.float64)
    n = s.shape[0]
    return s[n // 2] if n % 2 else s[n // 2 - 1] / 2 + s[n // 2] / 2


def np_weights(d, h, tol):
    """src/knnr.jl:156-160: w = wdist(d; h), then the clamp from below."""
    with np.errstate(all="ignore"):
        w = O.wdist(d, h=h)
    w[w < tol] = tol
    return w


def np_knn_space(X, Y, Xq, nlvdis, scal):
    """src/knnr.jl:142-154: (training coordinates, query coordinates) ahead of getknn."""
    X, Xq = np.asarray(X, dtype=np.float64), np.asarray(Xq, dtype=np.float64)
    if nlvdis == 0:
        if scal:
            xs = O.colstd(X, np.full(X.shape[0], 1.0 / X.shape[0]))      # :144 colstd(object.X)
            return X / xs, Xq / xs                                      # :145-146
        return X, Xq                                                    # :149
    fm = O.plskern(X, Y, nlv=nlvdis, scal=scal)                          # :126
    return fm.T, O.transform(fm, Xq)                                    # :152


def np_knn_lists(X, Y, Xq, nlvdis, metric, h, k, tol, scal):
    Z1, Z2 = np_knn_space(X, Y, Xq, nlvdis, scal)
    ind, d = O.getknn(Z1, Z2, k=k, metric=metric)                        # :147 / :149 / :152
    w = np.stack([np_weights(d[i], h, tol) for i in range(d.shape[0])])  # :155-160
    return ind, d, w


def np_knnr_predict(X, Y, Xq, *, nlvdis=0, metric="eucl", h=np.inf, k=1, tol=1e-4, scal=False):
    """src/knnr.jl:137-169."""
    Y = O.ensure_mat(np.asarray(Y, dtype=np.float64))
    ind, d, w = np_knn_lists(X, Y, Xq, nlvdis, metric, h, k, tol, scal)
    pred = np.stack([O.colmean(Y[ind[i]], O.mweight(w[i])) for i in range(ind.shape[0])])   # :163-167
    return dict(pred=pred, listnn=ind, listd=d, listw=w)


def np_findmax_cla(x, w):
    """src/utility.jl:564-570: the level of x with the largest summed weight; `argmax` takes the first of the sorted levels on ties."""
    lev = np.unique(x)
    sums = []
    for l in lev:
        s = 0.0
        for v in w[x == l]:                                             # (`aggstat` with fun = sum: in row order)
            s += v
        sums.append(s)
    return lev[int(np.argmax(sums))]


def np_knnda_predict(X, y, Xq, *, nlvdis=0, metric="eucl", h=np.inf, k=1, tol=1e-4, scal=False):
    """src/knnda.jl:108-138 (the scores of plskern on dummy(y), :95)."""
    y = np.asarray(y).reshape(-1)
    Yd = O.dummy(y)[0] if nlvdis else None
    ind, d, w = np_knn_lists(X, Yd, Xq, nlvdis, metric, h, k, tol, scal)
    pred = np.array([np_findmax_cla(y[ind[i]], w[i]) for i in range(ind.shape[0])]).reshape(-1, 1)   # :133-136
    return dict(pred=pred, listnn=ind, listd=d, listw=w)


def _occ_scaled_scores(X, nlv, scal, fm):
    fm = np_pcasvd(X, nlv=nlv, scal=scal) if fm is None else fm          # src/occknndis.jl:131
    T = np.asarray(fm["T"], dtype=np.float64)
    tscales = np.sqrt(np.mean((T - T.mean(axis=0)) ** 2, axis=0))        # :133 colstd(fm.T)
    return fm, tscales, T / tscales                                     # :134


def _occ_table(d, typc, cri, alpha):
    cutoff = np_cutoff(d, typc, cri, alpha)                              # src/occknndis.jl:143-144
    return dict(d=d, dstand=d / cutoff, pval=np_pval(d, d)), cutoff      # :145-147


def np_occknndis(X, *, nlv, samp, k, typc="mad", cri=3, alpha=.025, scal=False, fm=None):
    """src/occknndis.jl:125-149; samp: 0-based rows.  fm: a fitted PCA as a dict (T, P, xmeans, xscales) in place of :131."""
    fm, tscales, T = _occ_scaled_scores(X, nlv, scal, fm)
    _, dd = O.getknn(T, T[np.asarray(samp)], k=k + 1, metric="eucl")    # :137-138
    d = np.array([np_median(dd[i][1:]) for i in range(dd.shape[0])])    # :140-142
    tab, cutoff = _occ_table(d, typc, cri, alpha)
    return dict(d=tab, fm=fm, T=T, tscales=tscales, k=k, e_cdf=np.sort(d), cutoff=cutoff)


def _occ_query(obj, Xq):
    return np_pca_transform(obj["fm"], Xq) / obj["tscales"]              # src/occknndis.jl:160-161


def np_occknndis_predict(obj, Xq):
    """src/occknndis.jl:157-171."""
    _, dd = O.getknn(obj["T"], _occ_query(obj, Xq), k=obj["k"], metric="eucl")      # :162
    d = np.array([np_median(dd[i]) for i in range(dd.shape[0])])         # :164-166
    tab = dict(d=d, dstand=d / obj["cutoff"], pval=np_pval(obj["e_cdf"], d))
    return dict(pred=(tab["dstand"] > 1).astype(np.int64).reshape(-1, 1), d=tab)


def _loo_median(T, j, k):
    """median(getknn(rmrow(T, j), T[j:j, :]; k).d[1]) — src/occlknndis.jl:153-154."""
    return np_median(O.getknn(O.rmrow(T, [j]), T[j:j + 1], k=k, metric="eucl")[1][0])


def np_occlknndis(X, *, nlv, samp, k, typc="mad", cri=3, alpha=.025, scal=False, reading="literal", fm=None):
    """src/occlknndis.jl:132-165.  reading = "literal": :146-157 as written — the query is row i of T while the removed row is samp[i] (:148), and the
    neighbour indices of the row-removed matrix are used unshifted as rows of T (:152-153).  reading = "doc": the query is row samp[i], it is removed,
    and the indices are mapped back to rows of T."""
    fm, tscales, T = _occ_scaled_scores(X, nlv, scal, fm)
    samp = np.asarray(samp)
    d, zd = np.zeros(samp.size), np.zeros(samp.size)
    for i in range(samp.size):                                           # :146
        q = i if reading == "literal" else samp[i]
        ind, dd = O.getknn(O.rmrow(T, [samp[i]]), T[q:q + 1], k=k, metric="eucl")   # :148
        d[i] = np_median(dd[0])                                          # :150
        zind = ind[0] if reading == "literal" else ind[0] + (ind[0] >= samp[i])
        zd[i] = np_median([_loo_median(T, int(j), k) for j in zind])     # :151-156
    d = d / zd                                                           # :158
    tab, cutoff = _occ_table(d, typc, cri, alpha)                        # :159-163
    return dict(d=tab, fm=fm, T=T, tscales=tscales, k=k, e_cdf=np.sort(d), cutoff=cutoff)


def np_occlknndis_predict(obj, Xq, dk_train=None):
    """src/occlknndis.jl:173-199.  dk_train: None — the nested searches as written (:186-191) — or a dict row -> leave-one-out median that is filled
    and looked up instead (the cached form)."""
    T, k = obj["T"], obj["k"]
    ind, dd = O.getknn(T, _occ_query(obj, Xq), k=k, metric="eucl")      # :178
    d, zd = np.zeros(ind.shape[0]), np.zeros(ind.shape[0])
    for i in range(ind.shape[0]):                                        # :183
        d[i] = np_median(dd[i])                                          # :185
        vd = []
        for j in ind[i]:                                                 # :186
            j = int(j)
            if dk_train is None:
                vd.append(_loo_median(T, j, k))                          # :188-190
            else:
                if j not in dk_train:
                    dk_train[j] = _loo_median(T, j, k)
                vd.append(dk_train[j])
        zd[i] = np_median(vd)                                            # :192
    d = d / zd                                                           # :194
    tab = dict(d=d, dstand=d / obj["cutoff"], pval=np_pval(obj["e_cdf"], d))
    return dict(pred=(tab["dstand"] > 1).astype(np.int64).reshape(-1, 1), d=tab)


# ---------------------------------------------------------------------------------- data
def lattice(n, dd, seed, dup_blocks=True):
    """Integer rows with entries in -8 .. 8: every squared distance is exact in Float64 whatever the summation order.  With dup_blocks, rows
    4 i .. 4 i + 3 of the first half are identical and rows 5, 17, 29, ... repeat row 5 (ties at distance 0 and at the k-th place)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-8, 9, size=(n, dd)).astype(np.float64)
    if dup_blocks and n >= 64:
        h = (n // 2) // 4 * 4
        X[:h] = np.repeat(X[:h:4], 4, axis=0)
        dup = np.arange(5, n, 12)[:max(n // 13, 1)]
        X[dup] = X[5]
    return X


def lattice_queries(X, m, seed):
    """m integer queries: every third one a training row itself (distance 0 to its copies), the others fresh lattice points."""
    rng = np.random.default_rng(seed)
    Q = rng.integers(-8, 9, size=(m, X.shape[1])).astype(np.float64)
    rows = rng.integers(0, X.shape[0], size=m)
    Q[::3] = X[rows[::3]]
    return Q


def latent(n, p, m, sources, seed):
    """The latent-structure data of test_lwplsr_predict (tests/test_gpu_parity.py): X, Xq, y."""
    L = O.rand_matrix(seed + 7, sources, p) - 0.5
    X = O.rand_matrix(seed + 5, n, sources) @ L + 0.05 * O.rand_matrix(seed + 1, n, p)
    Xq = O.rand_matrix(seed + 6, m, sources) @ L + 0.05 * O.rand_matrix(seed + 2, m, p)
    y = X[:, :5] @ np.array([1.0, -2.0, 0.5, 3.0, 1.5]) + np.sin(3 * X[:, 5]) + 0.05 * O.rand_matrix(seed + 3, n, 1)[:, 0]
    return X, Xq, y


def classes_of(y, ncls):
    """ncls classes from the quantiles of a response."""
    edges = np.quantile(y, np.linspace(0, 1, ncls + 1)[1:-1])
    return np.searchsorted(edges, y).astype(np.int64)


MAHAL_CASE = dict(n=1500, p=30, m=40, sources=12, seed=40, nlvdis=5, k=30, h=2.0)      # the nlvdis = 5, metric = "mahal" case of the model tests
GAP = 1e-9
MAX_SKIP = 0.02


def comparable_queries(d):
    """d: the reference's distances up to place k + 1 (m x (k + 1)).  A query is comparable when the relative gap between every pair of consecutive
    distances exceeds GAP: below that a rounding of the scores may swap two neighbours, and then lists, weights and predictions legitimately differ."""
    d = np.asarray(d)
    gap = (d[:, 1:] - d[:, :-1]) / np.maximum(d[:, 1:], np.finfo(float).tiny)
    return np.all(gap > GAP, axis=1)


def mahal_case_reference(kind):
    """(X, Xq, y or classes, comparable mask, the restatement's result) for the mahal case; kind: "knnr" or "knnda"."""
    c = MAHAL_CASE
    X, Xq, y = latent(c["n"], c["p"], c["m"], c["sources"], c["seed"])
    kw = dict(nlvdis=c["nlvdis"], metric="mahal", h=c["h"], k=c["k"])
    if kind == "knnda":
        y = classes_of(y, 4)
        Z1, Z2 = np_knn_space(X, O.dummy(y)[0], Xq, c["nlvdis"], False)
        ref = np_knnda_predict(X, y, Xq, **kw)
    else:
        Z1, Z2 = np_knn_space(X, y, Xq, c["nlvdis"], False)
        ref = np_knnr_predict(X, y, Xq, **kw)
    ok = comparable_queries(O.getknn(Z1, Z2, k=c["k"] + 1, metric="mahal")[1])
    return X, Xq, y, ok, ref


def wmean_inputs(n, q, m, k, seed):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((n, q)) * np.exp(rng.uniform(-3, 3, size=(n, 1)))
    ind = rng.integers(0, n, size=(m, k)).astype(np.int32)
    w = np.maximum(np.exp(-rng.uniform(0, 12, size=(m, k))), 1e-4)
    return np.asfortranarray(Y), ind, w


def np_wmean(Y, ind, w, dtype=np.float64):
    """pred[i, :] = sum_j (w_ij / sum_j w_ij) Y[ind_ij, :] — `mweight` + `colmean`, src/knnr.jl:120-124 — in the given precision."""
    Y, w = np.asarray(Y).astype(dtype), np.asarray(w).astype(dtype)
    out = np.zeros((ind.shape[0], Y.shape[1]), dtype=dtype)
    for i in range(ind.shape[0]):
        wn = w[i] / w[i].sum(dtype=dtype)
        out[i] = (wn[:, None] * Y[ind[i]]).sum(axis=0, dtype=dtype)
    return out


def wmean_bound(Y, ind, w):
    """4 (k + 4) 2^-53 sum_j w~_ij |y_ij| per element: k - 1 additions of the weight sum, one division and one product per term, k - 1 additions
    of the terms — (2 k + 1) roundings in any summation order, to first order — with a factor of almost two in hand."""
    k = ind.shape[1]
    wn = w / w.sum(axis=1, keepdims=True)
    return 4 * (k + 4) * U * np.einsum("ik,ikq->iq", wn, np.abs(np.asarray(Y)[ind]))


WMEAN_SHAPES = [(500, 1, 9, 1), (500, 3, 9, 64), (700, 17, 7, 65), (2000, 3, 5, 1500)]   # (n, q, m, k)


# ---------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("n,dd,k", [(60, 3, 4), (200, 2, 7), (300, 3, 299)])
def test_dropping_self_from_a_search_for_k_plus_1_equals_the_search_without_that_row(n, dd, k):
    """jch_knn_search removes training row s from a query's candidates by searching k + 1 over ALL rows and dropping the entry of row s if it is
    there and the last entry otherwise.  The full list is in (distance, index) order; taking row s out of that order leaves the order of the
    others, so the first k of what is left are the k nearest of the row-removed matrix — also when s sits behind k + 1 or more copies of the query
    at lower indices (all at distance 0, all before it): then s is not among the k + 1 and the last one goes."""
    T = lattice(n, dd, 3)
    c = min(k + 2, n - 1)
    T[:c] = T[c]                                                          # k + 2 copies of row k + 2 at lower indices (k = n - 1: all other rows)
    assert np.all(T[:c + 1] == T[c])
    checked_absent = 0
    for s in [0, 5, 17, c, n // 2, n - 1]:
        for q in (T[s], T[(s + 1) % n], lattice_queries(T, 1, s)[0]):
            ind1, d1 = O.getknn(T, q[None, :], k=min(k + 1, n))
            ind1, d1 = ind1[0], d1[0]
            hit = np.nonzero(ind1 == s)[0]
            drop = hit[0] if hit.size else ind1.size - 1
            checked_absent += 0 if hit.size else 1
            keep = np.delete(np.arange(ind1.size), drop)
            indr, dr = O.getknn(O.rmrow(T, [s]), q[None, :], k=k)
            back = indr[0] + (indr[0] >= s)                              # rows of rmrow(T, s) -> rows of T
            assert np.array_equal(ind1[keep], back), (s, ind1, back)
            assert np.array_equal(d1[keep], dr[0])
    assert checked_absent > 0 or k + 1 == n                               # (k + 1 = n lists every row: nothing can be absent)
    # the query is row k + 2 itself, removed: k + 2 copies at lower indices fill all k + 1 places, the row is absent, the last copy goes
    if c == k + 2:
        ind1 = O.getknn(T, T[c][None, :], k=k + 1)[0][0]
        assert c not in ind1 and np.array_equal(ind1, np.arange(k + 1))


def _small_occ_data():
    rng = np.random.default_rng(11)
    n, p, m = 120, 9, 14
    L = rng.standard_normal((4, p))
    X = rng.standard_normal((n, 4)) @ L + 0.1 * rng.standard_normal((n, p))
    Xq = rng.standard_normal((m, 4)) @ L + 0.1 * rng.standard_normal((m, p))
    Xq[::5] *= 3.0
    return X, np.vstack([Xq, X[:6]])


@pytest.mark.parametrize("reading", ["literal", "doc"])
def test_cached_occlknndis_predict_equals_the_nested_searches(reading):
    X, Xq = _small_occ_data()
    samp = np.random.default_rng(5).choice(X.shape[0], size=25, replace=False)
    obj = np_occlknndis(X, nlv=4, samp=samp, k=5, reading=reading)
    nested = np_occlknndis_predict(obj, Xq)
    cache = {}
    cached = np_occlknndis_predict(obj, Xq, dk_train=cache)
    for col in ("d", "dstand", "pval"):
        assert np.array_equal(nested["d"][col], cached["d"][col])
    assert np.array_equal(nested["pred"], cached["pred"]) and 0 < len(cache) <= X.shape[0]
    again = np_occlknndis_predict(obj, Xq, dk_train=cache)               # a warm cache: the same bits
    assert np.array_equal(again["d"]["d"], cached["d"]["d"])
    assert set(np.unique(nested["pred"])) == {0, 1}                       # both classes occur on these inputs


def test_the_two_readings_of_the_occlknndis_fit_differ_and_occknndis_runs():
    X, Xq = _small_occ_data()
    samp = np.random.default_rng(5).choice(X.shape[0], size=25, replace=False)
    lit, doc = np_occlknndis(X, nlv=4, samp=samp, k=5), np_occlknndis(X, nlv=4, samp=samp, k=5, reading="doc")
    assert not np.array_equal(lit["d"]["d"], doc["d"]["d"])
    assert np.all(np.isfinite(lit["d"]["d"])) and np.all(np.isfinite(doc["d"]["d"]))
    for typc in ("mad", "q"):
        obj = np_occknndis(X, nlv=4, samp=samp, k=6, typc=typc)
        res = np_occknndis_predict(obj, Xq)
        assert res["pred"].shape == (Xq.shape[0], 1) and np.all(res["d"]["d"] > 0)
        # place 1 of a training row's own list is the row itself at distance 0: the median over 2:end is over the k others
        dd = O.getknn(obj["T"], obj["T"][samp], k=7)[1]
        assert np.all(dd[:, 0] == 0) and np.array_equal(obj["d"]["d"], [np_median(r[1:]) for r in dd])


@pytest.mark.parametrize("n,q,m,k", WMEAN_SHAPES)
def test_wmean_bound_holds_for_a_float64_evaluation(n, q, m, k):
    Y, ind, w = wmean_inputs(n, q, m, k, seed=n + k)
    ref = np_wmean(Y, ind, w, np.longdouble)
    got = np_wmean(Y, ind, w)
    bound = wmean_bound(Y, ind, w)
    assert np.all(bound > 0)
    assert np.all(np.abs(got - ref.astype(np.float64)) <= bound)
    # ... with room: a float64 evaluation in ANOTHER order (reversed neighbours) also stays inside
    rev = np_wmean(Y, ind[:, ::-1], w[:, ::-1])
    assert np.all(np.abs(rev - ref.astype(np.float64)) <= bound)


@pytest.mark.parametrize("kind", ["knnr", "knnda"])
def test_few_queries_of_the_mahal_case_are_not_comparable(kind):
    X, Xq, y, ok, ref = mahal_case_reference(kind)
    assert ok.shape == (MAHAL_CASE["m"],)
    assert 1.0 - ok.mean() <= MAX_SKIP, (int((~ok).sum()), "queries skipped")
    if kind == "knnda":
        assert len(np.unique(ref["pred"])) >= 3                           # the vote is not trivial on these inputs


def test_restatements_on_a_hand_made_case():
    X = np.array([[0.0], [1.0], [2.0], [10.0]])
    Y = np.array([1.0, 2.0, 4.0, 100.0])
    r = np_knnr_predict(X, Y, np.array([[0.9]]), k=3)                     # h = Inf: equal weights
    assert np.array_equal(r["listnn"], [[1, 0, 2]]) and np.allclose(r["listw"], 1.0) and np.isclose(r["pred"][0, 0], 7.0 / 3.0)
    yc = np.array(["b", "a", "b", "a"])
    assert np_knnda_predict(X, yc, np.array([[0.9]]), k=3)["pred"][0, 0] == "b"
    assert np_knnda_predict(X, yc, np.array([[0.9]]), k=2)["pred"][0, 0] == "a"      # a tie of two equal weights: the first sorted level
    assert np_findmax_cla(np.array([2, 1, 2, 1]), np.array([0.25, 0.5, 0.25, 0.0])) == 1
    assert np_middle_median([1.0, 2.0, 4.0, 8.0]) == 3.0 and np_middle_median([1.0, 5.0, 9.0]) == 5.0


# ---------------------------------------------------------------------------------- the boundary
KNN_ENTRIES = {
    "jch_knn_prepare": 7, "jch_knn_release": 2, "jch_knn_search": 15, "jch_knn_wmean": 11, "jch_knn_vote": 11, "jch_knn_gather_median": 8,
}


def test_header_declares_the_entries_and_the_library_is_built_from_knn_hip():
    h = open(os.path.join(ROOT, "include", "jchemo_hip.h")).read()
    import jchemo_hip as J
    for name, nargs in KNN_ENTRIES.items():
        m = re.search(r"JCH_API\s+int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", h, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
        assert name in J.SYMBOLS
    assert "src/getknn.jl" in h and "src/occlknndis.jl" in h
    mk = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "Makefile")).read()
    assert "knn.hip" in re.search(r"^SRCS := (.*)$", mk, flags=re.M).group(1).split()
    src = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "knn.hip")).read()
    assert "jch_knn_dispatch" in src and "asm" not in src                 # the search is lwplsr's own dispatch; no inline assembly
    lw = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "lwplsr.hip")).read()
    assert lw.count("jch_knn_dispatch(") == 2                             # defined once, called once by lw_run


def test_python_package_exports_fields_and_defaults():
    import jchemo_hip as J
    for name in ("getknn", "knnr", "knnda", "occknndis", "occlknndis", "Knnr", "Knnda", "Occknndis", "Occlknndis", "knn_search", "knn_wmean",
                 "knn_vote", "knn_gather_median"):
        assert hasattr(J, name), name
    assert [f.name for f in dataclasses.fields(J.Knnr)] == ["X", "Y", "fm", "nlvdis", "metric", "h", "k", "tol", "scal"]                     # src/knnr.jl:1-11
    assert [f.name for f in dataclasses.fields(J.Knnda)] == ["X", "y", "fm", "nlvdis", "metric", "h", "k", "tol", "lev", "ni", "scal"]       # src/knnda.jl:1-13
    assert [f.name for f in dataclasses.fields(J.Occknndis)] == ["d", "fm", "T", "tscales", "k", "e_cdf", "cutoff"]                          # src/occknndis.jl:1-9
    assert [f.name for f in dataclasses.fields(J.Occlknndis)] == ["d", "fm", "T", "tscales", "k", "e_cdf", "cutoff"]
    for fn in (J.knnr, J.knnda):
        d = {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not v.empty and k != "ctx"}
        assert d == dict(nlvdis=0, metric="eucl", h=np.inf, k=1, tol=1e-4, scal=False)                                                        # src/knnr.jl:119-120
    sig = inspect.signature(J.occlknndis)
    assert [sig.parameters[k].default for k in ("typc", "cri", "alpha", "scal", "samp", "seed", "reading")] == ["mad", 3, .025, False, None, None, "literal"]
    assert inspect.signature(J.getknn).parameters["k"].default == 1 and inspect.signature(J.getknn).parameters["metric"].default == "eucl"


def test_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    X = np.zeros((6, 2), order="F")
    with pytest.raises(ValueError):
        J.knnr(X, np.zeros(6), metric="manhattan")
    with pytest.raises(ValueError):
        J.knnr(X, np.zeros(6), k=0)
    with pytest.raises(ValueError):
        J.knnda(X, np.zeros(5))
    with pytest.raises(ValueError):
        J.occlknndis(X, nlv=1, nsamp=2, k=1, reading="other")
    with pytest.raises(ValueError):
        J.occknndis(X, nlv=1, nsamp=2, k=1, typc="z")
    with pytest.raises(ValueError):
        J.getknn(X, np.zeros((2, 3)))


def test_julia_module_has_the_names_and_calls_the_entries():
    src = open(os.path.join(ROOT, "jchemo.jl_amd", "julia", "JchemoHIP.jl")).read()
    exported = set(re.findall(r"[\w!]+", re.search(r"\nexport (.*?)\n\n", src, flags=re.S).group(1)))
    for nm in ("getknn", "knnr", "knnda", "occknndis", "occlknndis", "Knnr", "Knnda", "Occknndis", "Occlknndis"):
        assert nm in exported, nm
    for name in KNN_ENTRIES:
        assert f"(:{name}, LIB)" in src, name
