"""sampks / sampdp / sampsys / sampcla without a GPU: literal numpy restatements of src/sampling.jl (an explicit n x n D, scanned column-major for its
first maximum, re-sliced at every step), the streaming max-min form the device runs (one n-vector of running minima per set), the proof that the two
agree on every case of the GPU tests, the exactness facts of the tie cases, the margins of the seeded cases, and the surface of the feature.

tests/test_gpu_samp.py imports the data builders, the case lists and the restatements from here.  All indices are 0-based."""
import inspect
import itertools
import os
import re
from functools import lru_cache

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52

# (n, p): wave (63-65), 128-row tile (127-129, 257: the triangle's second tile row and a third tile), 256-row block (257), T128_KB padding of p
# (1, 3, 15, 16, 17, 200), one launch of several blocks (1000)
MARGIN_CASES = [(2, 1), (3, 2), (3, 3), (63, 15), (64, 16), (65, 1), (127, 17), (128, 3), (129, 17), (257, 3), (300, 200), (1000, 16)]
MAHAL_CASES = [(65, 1), (129, 17), (257, 3), (1000, 16)]
LATTICES = ["lattice128", "lattice130", "lattice_dup"]
BIG = (20000, 64, 200)   # n, p, k of the one larger device run: checked against the streaming form only


# ---- data ---------------------------------------------------------------------------------------------------------------------------------------
def uniform(n, p, seed=None):
    """Seeded uniform data, column-major."""
    return np.asfortranarray(np.random.default_rng(20251019 + 1000 * n + p if seed is None else seed).random((n, p)))


def lattice(name):
    """Integer lattices: every squared distance is an exact integer and ties abound.  lattice128: 16 x 8, one full tile; lattice130: 13 x 10, a partial
    second tile; lattice_dup: the 16 x 8 lattice twice (every row duplicated, 256 rows).  All have dyadic column means."""
    if name == "lattice128":
        pts = list(itertools.product(range(16), range(8)))
    elif name == "lattice130":
        pts = list(itertools.product(range(13), range(10)))
    elif name == "lattice_dup":
        pts = 2 * list(itertools.product(range(16), range(8)))
    else:
        raise KeyError(name)
    return np.asfortranarray(np.array(pts, dtype=np.float64))


@lru_cache(maxsize=None)
def case_data(key):
    X = lattice(key) if isinstance(key, str) else uniform(*key)
    X.setflags(write=False)
    return X


# ---- distances ----------------------------------------------------------------------------------------------------------------------------------
def sqdist(X, dtype=np.float64):
    """D[i, j] = sum_k (x_ik - x_jk)^2, direct form, ascending k."""
    X = np.asarray(X, dtype=dtype)
    D = np.zeros((X.shape[0], X.shape[0]), dtype=dtype)
    for j in range(X.shape[1]):
        d = X[:, j][:, None] - X[:, j][None, :]
        D += d * d
    return D


def mahal_space(X, dtype=np.float64):
    """Z with |z_i - z_j|^2 = (x_i - x_j)' inv(S) (x_i - x_j), S the uncorrected covariance (`mahsq`, src/distances.jl:59-65): Z = X inv(U), S = U'U."""
    X = np.asarray(X, dtype=np.float64)
    S = np.atleast_2d(np.cov(X, rowvar=False, bias=True))
    Uinv = np.linalg.inv(np.linalg.cholesky(S).T)
    return (np.asarray(X, dtype=dtype) @ np.asarray(Uinv, dtype=dtype)).astype(dtype)


def metric_space(X, metric):
    return np.asarray(X) if metric == "eucl" else mahal_space(X)


def first_max(D):
    """`findall(D .== maximum(D))[1]`: the first maximum of a column-major scan, as (row, col)."""
    n = D.shape[0]
    idx = int(np.argmax(D.T.reshape(-1)))
    return idx % n, idx // n


def _setdiff(n, *taken):
    keep = np.ones(n, dtype=bool)
    for t in taken:
        keep[np.asarray(t, dtype=np.int64)] = False
    return np.flatnonzero(keep)


# ---- literal restatements of src/sampling.jl ----------------------------------------------------------------------------------------------------
def np_sampks(X, k, metric="eucl"):
    k = int(round(k))                                            # :41
    D = sqdist(metric_space(X, metric))                          # :42-46
    n = D.shape[0]
    s = list(first_max(D))                                       # :49-50
    cand = _setdiff(n, s)                                        # :52
    for _ in range(k - 2):                                       # :53
        u = D[np.ix_(s, cand)].min(axis=0)                       # :54
        s.append(int(cand[int(np.argmax(u))]))                   # :55-56 (`findall(u .== maximum(u))[1]`)
        cand = _setdiff(n, s)                                    # :57
    return np.array(s, dtype=np.int64), cand                     # :59


def np_sampdp(X, k, metric="eucl"):
    k = int(round(k))                                            # :119
    D = sqdist(metric_space(X, metric))                          # :120-124
    n = D.shape[0]
    s1 = list(first_max(D))                                      # :128-129
    zD = D.copy()                                                # :130
    zD[s1, :] = -np.inf                                          # :131
    zD[:, s1] = -np.inf                                          # :132
    s2 = list(first_max(zD))                                     # :133-134, the masked reading
    cand = _setdiff(n, s1, s2)                                   # :136
    for _ in range(k - 2):                                       # :137
        u = D[np.ix_(s1, cand)].min(axis=0)                      # :138
        s1.append(int(cand[int(np.argmax(u))]))                  # :139-140
        cand = _setdiff(n, s1)                                   # :141
        u = D[np.ix_(s2, cand)].min(axis=0)                      # :142
        s2.append(int(cand[int(np.argmax(u))]))                  # :143-144
        cand = _setdiff(n, s1, s2)                               # :145
    return np.array(s1, dtype=np.int64), np.array(s2, dtype=np.int64), cand   # :147


def _jround(v):
    """Julia's `round` of a Float64: half to even."""
    return int(np.rint(v))


def np_sampsys(y, k):
    k = int(round(k))                                            # :169
    y = np.asarray(y).reshape(-1)                                # :170
    n = y.shape[0]                                               # :171
    alpha = (n - 1) / (k - 1)                                    # :172-173
    z = [1 + i * alpha for i in range(k)]                        # :174 (k points: the test cases have exactly representable steps)
    z = list(dict.fromkeys(_jround(v) for v in z))               # :175-176
    idx = np.argsort(y, kind="stable")                           # :177
    s = idx[np.array(z) - 1]                                     # :178-179
    return s, _setdiff(n, s)                                     # :180-181


def np_sampcla(x, y, k):
    """The systematic branch (:218-243); the random one is checked by its counts."""
    x = np.asarray(x).reshape(-1)
    lev, ni = np.unique(x, return_counts=True)                   # :222-224
    kk = np.minimum(np.repeat(k, lev.shape[0]) if np.ndim(k) == 0 else np.asarray(k), ni)   # :226, :229
    s = []
    for i in range(lev.shape[0]):                                # :228
        zs = np.flatnonzero(x == lev[i])                         # :230
        u = np_sampsys(np.asarray(y)[zs], kk[i])[0] if kk[i] > 1 else np.argsort(np.asarray(y)[zs], kind="stable")[:1]   # :235
        s.append(zs[u])                                          # :236
    s = np.concatenate(s)                                        # :239
    return s, _setdiff(x.shape[0], s), lev, ni, kk               # :240-242


# ---- the streaming form the device runs ---------------------------------------------------------------------------------------------------------
def np_farthest(X, skip=(), dtype=np.float64):
    """(row, col, d2): the first column-major maximum of the direct-form D with the rows of `skip` masked out."""
    D = sqdist(X, dtype)
    sk = list(skip)
    D[sk, :] = -np.inf
    D[:, sk] = -np.inf
    np.fill_diagonal(D, -np.inf)
    r, c = first_max(D)
    return r, c, D[r, c]


def np_stream(X, init, k, nsets=1, dtype=np.float64, gaps=None):
    """jch_maxmin_select restated: mind[s] = the running minimum of d2 to the rows of set s, one update per selected row; the next row of a set is the
    first maximum of mind[s] over the rows no set has taken, set 0 choosing first.  Returns sel (k x nsets) and dsel.  gaps (a list) receives, per
    choice, (winner - runner-up) / winner over the candidates of that choice (inf when there is one candidate)."""
    X = np.asarray(X, dtype=dtype)
    n = X.shape[0]
    init = np.asarray(init, dtype=np.int64).reshape(nsets, 2)
    sel = np.zeros((k, nsets), dtype=np.int64)
    dsel = np.zeros((k, nsets), dtype=dtype)
    taken = np.zeros(n, dtype=bool)
    taken[init.reshape(-1)] = True

    def d2to(r):
        acc = np.zeros(n, dtype=dtype)
        for j in range(X.shape[1]):
            d = X[:, j] - X[r, j]
            acc += d * d
        return acc

    mind = []
    for s in range(nsets):
        a, b = d2to(init[s, 0]), d2to(init[s, 1])
        mind.append(np.minimum(a, b))
        sel[:2, s] = init[s]
        dsel[:2, s] = a[init[s, 1]]
    for t in range(2, k):
        for s in range(nsets):
            m = np.where(taken, -np.inf, mind[s])
            w = int(np.argmax(m))
            if gaps is not None:
                rest = np.delete(m, w)
                rest = rest[rest > -np.inf]
                gaps.append(float((m[w] - rest.max()) / m[w]) if rest.size and m[w] > 0 else np.inf)
            sel[t, s], dsel[t, s] = w, m[w]
            taken[w] = True
        for s in range(nsets):
            mind[s] = np.minimum(mind[s], d2to(sel[t, s]))
    return sel, dsel


def pair_gap(X, skip=()):
    """(largest - second largest) / largest over the pairs i < j of the rows outside `skip`, in extended precision."""
    D = sqdist(X, np.longdouble)
    keep = _setdiff(D.shape[0], list(skip))
    v = np.sort(D[np.ix_(keep, keep)][np.triu_indices(keep.size, 1)])
    return np.inf if v.size < 2 else float((v[-1] - v[-2]) / v[-1])


@lru_cache(maxsize=None)
def reference(key, metric="eucl"):
    """Everything the tests of one case share, computed once: the data in the metric's space, both starting pairs, the full Kennard-Stone order
    (k = n) and the full Duplex orders (k = n // 2) of the literal restatement — a selection with a smaller k is a prefix — and the extended-precision
    dsel of the streaming form."""
    X = case_data(key)
    Z = metric_space(X, metric)
    n = Z.shape[0]
    ks = np_sampks(X, n, metric)[0]
    out = dict(Z=Z, n=n, ks=ks, pair1=np_farthest(Z))
    out["ks_ld"] = np_stream(Z, ks[:2], n, 1, np.longdouble)
    if n >= 4:
        s1, s2, _ = np_sampdp(X, n // 2, metric)
        out.update(dp=(s1, s2), pair2=np_farthest(Z, skip=s1[:2]))
        out["dp_ld"] = np_stream(Z, [s1[0], s1[1], s2[0], s2[1]], n // 2, 2, np.longdouble)
    return out


ALL_KEYS = [(k_, "eucl") for k_ in MARGIN_CASES + LATTICES] + [(k_, "mahal") for k_ in MAHAL_CASES]


# ---- the streaming form equals the literal restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,metric", ALL_KEYS, ids=lambda v: str(v).replace(" ", ""))
def test_streaming_form_equals_the_literal_restatement(key, metric):
    ref = reference(key, metric)
    Z, n = ref["Z"], ref["n"]
    r, c, d2 = ref["pair1"]
    assert r > c and [r, c] == list(ref["ks"][:2])
    sel, dsel = np_stream(Z, [r, c], n, 1)
    assert np.array_equal(sel[:, 0], ref["ks"])
    assert dsel[0, 0] == dsel[1, 0] == d2
    assert sorted(sel[:, 0]) == list(range(n))
    if n >= 4:
        s1, s2 = ref["dp"]
        r2, c2, _ = ref["pair2"]
        assert r2 > c2 and [r2, c2] == list(s2[:2]) and not {r2, c2} & {r, c}
        sel2, _ = np_stream(Z, [r, c, r2, c2], n // 2, 2)
        assert np.array_equal(sel2[:, 0], s1) and np.array_equal(sel2[:, 1], s2)
        assert len(set(s1) | set(s2)) == 2 * (n // 2)


def test_a_smaller_k_is_a_prefix():
    X = case_data((129, 17))
    full = reference((129, 17))
    for k in (2, 3, 43):
        assert np.array_equal(np_sampks(X, k)[0], full["ks"][:k])
        s1, s2, rem = np_sampdp(X, k)
        assert np.array_equal(s1, full["dp"][0][:k]) and np.array_equal(s2, full["dp"][1][:k])
        assert sorted(list(s1) + list(s2) + list(rem)) == list(range(129))


# ---- tie cases: exact arithmetic in both forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LATTICES)
def test_lattice_distances_are_exact_integers_in_both_forms(name):
    X = case_data(name)
    ref = reference(name)
    D = sqdist(X)
    assert np.array_equal(D, np.rint(D)) and np.array_equal(D, sqdist(X, np.longdouble).astype(np.float64))
    # the device centres on the means of the candidate rows: all rows for the first pair, all but the first pair for the second
    for skip in ((), tuple(ref["ks"][:2])):
        keep = _setdiff(X.shape[0], list(skip))
        c = X[keep].sum(axis=0) / keep.size
        assert np.array_equal(2 * c, np.rint(2 * c))                         # dyadic: the shift is exact
        A = X - c
        assert np.array_equal((A + c), X)
        nrm = np.zeros(X.shape[0])
        for j in range(X.shape[1]):
            nrm += A[:, j] * A[:, j]
        E = nrm[:, None] + nrm[None, :] - 2.0 * (A @ A.T)                    # the expanded form of the tile epilogue
        assert np.array_equal(E, D)
    # and there are ties to resolve: the maximum is attained by more than one pair on the duplicated lattice, many steps tie everywhere
    gaps = []
    np_stream(X, ref["ks"][:2], X.shape[0], 1, gaps=gaps)
    assert sum(g == 0.0 for g in gaps) >= 30
    if name == "lattice_dup":
        assert np.count_nonzero(np.triu(D, 1) == D.max()) > 1


# ---- margin cases -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,metric", [(k_, "eucl") for k_ in MARGIN_CASES] + [(k_, "mahal") for k_ in MAHAL_CASES], ids=lambda v: str(v).replace(" ", ""))
def test_seeded_cases_have_margins_and_a_tight_dsel(key, metric):
    ref = reference(key, metric)
    Z, n = ref["Z"], ref["n"]
    gaps = [pair_gap(Z)]
    np_stream(Z, ref["ks"][:2], n, 1, np.longdouble, gaps=gaps)
    if n >= 4:
        s1, s2 = ref["dp"]
        gaps.append(pair_gap(Z, skip=s1[:2]))
        np_stream(Z, [s1[0], s1[1], s2[0], s2[1]], n // 2, 2, np.longdouble, gaps=gaps)
    print(f"{key} {metric}: smallest relative gap {min(gaps):.3g} over {len(gaps)} choices")
    assert min(gaps) >= 1e-9
    _, d64 = np_stream(Z, ref["ks"][:2], n, 1)
    sel_ld, d_ld = ref["ks_ld"]
    assert np.array_equal(sel_ld[:, 0], ref["ks"])
    assert np.all(np.abs(d64 - d_ld) <= 1e-12 * np.abs(d_ld))


# ---- sampsys / sampcla --------------------------------------------------------------------------------------------------------------------------
def test_sampsys_hand_computed_cases():
    import jchemo_hip as J
    y = np.array([5.0, 1.0, 3.0, 2.0, 4.0, 0.0])                   # sorted order: rows 5, 1, 3, 2, 4, 0
    r = J.sampsys(y, 2)                                            # grid 1, 6: the minimum and the maximum
    assert list(r.train) == [5, 0] and list(r.test) == [1, 2, 3, 4]
    r = J.sampsys(y, 6)                                            # k = n: step 1, every row, in the order of y
    assert list(r.train) == [5, 1, 3, 2, 4, 0] and list(r.test) == []
    r = J.sampsys(y, 3)                                            # step 2.5: 1, 3.5, 6 -> 1, 4, 6 (3.5 rounds to the even 4)
    assert list(r.train) == [5, 2, 0] and list(r.test) == [1, 3, 4]
    r = J.sampsys(np.array([3.0, 2.0, 1.0, 0.0]), 3)               # step 1.5: 1, 2.5, 4 -> 1, 2, 4 (2.5 rounds to the even 2, not to 3)
    assert list(r.train) == [3, 2, 0] and list(r.test) == [1]
    r = J.sampsys(np.array([2.0, 0.0, 1.0]), 5)                    # step .5: 1, 1.5, 2, 2.5, 3 -> 1, 2, 2, 2, 3 -> unique
    assert list(r.train) == [1, 2, 0]
    assert list(J.sampsys(y, 2.5).train) == [5, 0] and list(J.sampsys(y, 3.5).train) == list(J.sampsys(y, 4).train)   # k = round(k), half to even
    rng = np.random.default_rng(5)
    for n, k in ((7, 3), (10, 4), (11, 6), (50, 8), (9, 9)):
        yy = rng.random(n)
        got = J.sampsys(yy, k)
        tr, te = np_sampsys(yy, k)
        assert np.array_equal(got.train, tr) and np.array_equal(got.test, te)
        assert got.train[0] == np.argmin(yy) and got.train[-1] == np.argmax(yy)
    with pytest.raises(ValueError):
        J.sampsys(y, 1)


def test_sampcla_counts_clipping_and_systematic_branch():
    import jchemo_hip as J
    x = np.array(list("bbbaacbbac"))                               # a: 3, b: 5, c: 2
    y = np.arange(10.0)[::-1].copy()
    r = J.sampcla(x, k=3, seed=7)
    assert list(r.lev) == ["a", "b", "c"] and list(r.ni) == [3, 5, 2] and list(r.k) == [3, 3, 2]   # min(k, ni)
    assert [list(x[r.train]).count(c) for c in "abc"] == [3, 3, 2]
    assert len(set(r.train)) == 8 and sorted(list(r.train) + list(r.test)) == list(range(10))
    assert list(x[r.train]) == ["a"] * 3 + ["b"] * 3 + ["c"] * 2   # class by class, in the order of the labels
    assert np.array_equal(J.sampcla(x, k=3, seed=7).train, r.train)
    r = J.sampcla(x, k=[1, 4, 5], seed=0)
    assert list(r.k) == [1, 4, 2] and [list(x[r.train]).count(c) for c in "abc"] == [1, 4, 2]
    r = J.sampcla(x, y, k=3)
    tr, te, lev, ni, kk = np_sampcla(x, y, 3)
    assert np.array_equal(r.train, tr) and np.array_equal(r.test, te) and list(r.k) == list(kk)
    zs = np.flatnonzero(x == "b")
    assert r.train[3] == zs[np.argmin(y[zs])] and r.train[5] == zs[np.argmax(y[zs])]
    with pytest.raises(ValueError):
        J.sampcla(x, k=[1, 2])
    with pytest.raises(ValueError):
        J.sampcla(x)


# ---- surface ------------------------------------------------------------------------------------------------------------------------------------
def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_makefile_and_symbols():
    import jchemo_hip as J
    h = re.sub(r"/\*.*?\*/", "", _read("include", "jchemo_hip.h"), flags=re.S)
    want = {"jch_farthest_pair": ["jch_ctx *", "int32_t", "const double *", "int64_t", "int64_t", "int64_t", "const int64_t *", "int32_t", "int64_t *", "double *"],
            "jch_maxmin_select": ["jch_ctx *", "int32_t", "const double *", "int64_t", "int64_t", "int64_t", "int32_t", "const int64_t *", "int64_t", "int64_t *",
                                  "double *"]}
    for name, types in want.items():
        m = re.search(r"JCH_API\s+int32_t\s+" + name + r"\s*\(([^;]*?)\)\s*;", h, flags=re.S)
        assert m, name
        params = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
        assert len(params) == len(types)
        assert [re.sub(r"\s*\b\w+$", "", a) for a in params] == types, params
        assert name in J.SYMBOLS
    assert len(J.SYMBOLS) == len(set(J.SYMBOLS))
    srcs = re.search(r"^SRCS := (.*)$", _read("jchemo.jl_amd", "csrc", "Makefile"), flags=re.M).group(1).split()
    assert "samp.hip" in srcs and os.path.exists(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "samp.hip"))
    L = J.load()
    assert len(L.jch_farthest_pair.argtypes) == 10 and len(L.jch_maxmin_select.argtypes) == 11
    assert L.jch_version() == 108


def test_python_signatures_records_and_argument_checks():
    import dataclasses
    import jchemo_hip as J
    for fn in (J.sampks, J.sampdp):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["X", "k", "metric", "ctx"]
        assert sig.parameters["metric"].default == "eucl" and sig.parameters["ctx"].default is None
        assert sig.parameters["k"].default is inspect.Parameter.empty
    assert list(inspect.signature(J.sampsys).parameters) == ["y", "k"]
    sig = inspect.signature(J.sampcla)
    assert list(sig.parameters) == ["x", "y", "k", "seed"] and sig.parameters["y"].default is None and sig.parameters["seed"].default is None
    assert [f.name for f in dataclasses.fields(J.Samp)] == ["train", "test"]
    assert [f.name for f in dataclasses.fields(J.Sampdp)] == ["train", "test", "remain"]
    assert [f.name for f in dataclasses.fields(J.Sampcla)] == ["train", "test", "lev", "ni", "k"]
    X = uniform(10, 3)
    # the arguments are checked before any device work: these raise ValueError with or without a GPU
    for fn, bad_k in ((J.sampks, (1, 11, 0.4)), (J.sampdp, (1, 6, 5.6))):
        with pytest.raises(ValueError):
            fn(X, 3, metric="manhattan")
        for k in bad_k:
            with pytest.raises(ValueError):
                fn(X, k)
    with pytest.raises(ValueError):
        J.sampdp(X[:3], 2)
    with pytest.raises(ValueError):
        J.maxmin_select(X, [0, 1, 2], 3)


def test_every_device_entry_fails_loudly_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import jchemo_hip as J
    X = uniform(12, 3)
    for call in (lambda: J.sampks(X, 4), lambda: J.sampks(X, 4, metric="mahal"), lambda: J.sampdp(X, 4), lambda: J.sampdp(X, 4, metric="mahal"),
                 lambda: J.farthest_pair(X), lambda: J.maxmin_select(X, [0, 1], 3)):
        with pytest.raises(J.JchError) as ei:
            call()
        assert ei.value.code == J._lib.JCH_ENODEV


def test_julia_exports_and_gc_preserve():
    src = _read("jchemo.jl_amd", "julia", "JchemoHIP.jl")
    exported = set(re.findall(r"[\w!]+", re.search(r"\nexport (.*?)\n\n", src, flags=re.S).group(1)))
    assert {"sampks", "sampdp", "sampsys", "sampcla"} <= exported
    for name in ("jch_farthest_pair", "jch_maxmin_select"):
        i = src.index(f"(:{name}, LIB)")
        k = src.rfind("GC.@preserve", 0, i)
        assert k >= 0 and i - k < 400, name
    for fn in ("sampks", "sampdp", "sampsys", "sampcla"):
        assert re.search(r"(^|\n)function " + fn + r"\(", src), fn
    body = src[src.index("function maxmin_select("):src.index("function _samp_space(")]
    assert "sel .+ 1" in body and ".- 1" in body                              # 1-based indices in and out
