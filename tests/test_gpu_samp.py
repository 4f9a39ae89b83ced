"""jch_farthest_pair, jch_maxmin_select and sampks / sampdp on the GPU, against the numpy restatements of tests/test_samp_static.py.

Selections are compared index for index: on the integer lattices every distance is exact in both forms (ties are resolved by the documented order),
on the seeded data every choice has a relative margin >= 1e-9 (asserted in the static file) against a rounding scale of 1e-13.  d2 / dsel are
compared with the extended-precision values: dsel is a fixed-order direct sum of p non-negative terms (p roundings of the sum, two of each term:
within (p + 2) 2^-53 < 4 p eps), d2 of the farthest pair within the bound of DESIGN.md §19."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_occ import _layouts  # noqa: E402
from test_samp_static import (BIG, EPS, LATTICES, MAHAL_CASES, MARGIN_CASES, case_data, np_sampdp, np_sampks, np_stream, reference, sqdist,  # noqa: E402
                              uniform)

SENT_I = -77
SENT_D = 7.0
IDS = dict(ids=lambda v: str(v).replace(" ", ""))


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


def _sources(X):
    """(loc, address, ldx, keep-alive) of a host X and of two device layouts: ldx > n, and a pointer 8 bytes off a 16-byte boundary."""
    Xh = np.asfortranarray(X)
    out = [(0, Xh.ctypes.data, Xh.shape[0], Xh)]
    for V, xa, ldx in _layouts(Xh):
        out.append((1, xa, ldx, V))
    torch.cuda.synchronize()
    return out


def _pair(J, ctx, src, n, p, skip=()):
    """(row, col, d2) through the ABI; the words around the outputs must keep their sentinels."""
    loc, xa, ldx, _ = src
    pair = np.full(4, SENT_I, dtype=np.int64)
    d2 = np.full(3, SENT_D)
    sk = np.asarray(skip, dtype=np.int64)
    st = J.load().jch_farthest_pair(ctx._h, loc, xa, n, p, ldx, sk.ctypes.data if sk.size else None, sk.size, pair.ctypes.data + 8, d2.ctypes.data + 8)
    ctx.check(st)
    assert pair[0] == SENT_I and pair[3] == SENT_I and d2[0] == SENT_D and d2[2] == SENT_D
    return int(pair[1]), int(pair[2]), float(d2[1])


def _select(J, ctx, src, n, p, nsets, init, k, want_dsel=True):
    """(sel, dsel), k x nsets, through the ABI; sentinels in front of and behind both."""
    loc, xa, ldx, _ = src
    init = np.asarray(init, dtype=np.int64)
    sel = np.full(k * nsets + 2, SENT_I, dtype=np.int64)
    ds = np.full(k * nsets + 2, SENT_D)
    ctx.check(J.load().jch_maxmin_select(ctx._h, loc, xa, n, p, ldx, nsets, init.ctypes.data, k, sel.ctypes.data + 8, ds.ctypes.data + 8 if want_dsel else None))
    assert sel[0] == SENT_I and sel[-1] == SENT_I and ds[0] == SENT_D and ds[-1] == SENT_D
    return sel[1:-1].reshape(nsets, k).T.copy(), ds[1:-1].reshape(nsets, k).T.copy()


def _pair_bound(p):
    """every compared value is within eps_c = 4 (p + 20) u of the largest squared distance D* (u = 2^-53), so the winner's true d2 is
    within 2 eps_c D* of D*; the reported d2 is that pair's direct sum, within (p + 2) u of its true value."""
    return (8 * (p + 20) + p + 2) * 2.0 ** -53


# ---------------------------------------------------------------------------------- jch_farthest_pair through the C ABI
@pytest.mark.parametrize("key", MARGIN_CASES + LATTICES, **IDS)
def test_farthest_pair(J, ctx, key):
    X = case_data(key)
    n, p = X.shape
    ref = reference(key)
    Dld = sqdist(X, np.longdouble)
    got = []
    for src in _sources(X):
        r, c, d2 = _pair(J, ctx, src, n, p)
        assert (r, c) == ref["pair1"][:2], (key, src[0], src[2])
        exact = float(Dld[r, c])
        print(f"{key}: d2 rel. error {abs(d2 - exact) / exact:.3g}, bound {_pair_bound(p):.3g}")
        assert abs(d2 - exact) <= _pair_bound(p) * exact
        got.append(d2)
        if n >= 4:                                                    # skip honoured with 2 indices: the second pair of Duplex
            r2, c2, d22 = _pair(J, ctx, src, n, p, skip=ref["ks"][:2])
            assert (r2, c2) == ref["pair2"][:2]
            assert abs(d22 - float(Dld[r2, c2])) <= _pair_bound(p) * float(Dld[r2, c2])
            assert _pair(J, ctx, src, n, p, skip=[ref["ks"][1], ref["ks"][0], ref["ks"][1]])[:2] == (r2, c2)   # any order, repeats allowed
            got.append(d22)
    assert got[:len(got) // 3] == got[len(got) // 3:2 * len(got) // 3] == got[2 * len(got) // 3:]   # host and device X, any layout: identical bits


def _with_bad_rows(X, rows, value=np.nan):
    """X with extra rows holding `value` in one entry inserted so that they END UP at the positions `rows`; returns it and, per new index, the old one (-1: bad)."""
    n, p = X.shape
    m = n + len(rows)
    old = np.full(m, -1, dtype=np.int64)
    good = np.setdiff1d(np.arange(m), rows)
    old[good] = np.arange(n)
    Y = np.empty((m, p), order="F")
    Y[good] = X
    Y[list(rows)] = X[:len(rows)]
    for a, r in enumerate(rows):
        Y[r, a % p] = value
    return Y, old, good


@pytest.mark.parametrize("key", [(65, 1), (129, 17), "lattice128"], **IDS)
def test_a_nan_row_is_never_returned_or_selected(J, ctx, key):
    X = case_data(key)
    ref = reference(key)
    n, p = X.shape
    Y, old, good = _with_bad_rows(X, [0, 70 if n > 70 else 40, n + 2])        # first row, one in the middle (the second tile for n = 129), the last
    m = Y.shape[0]
    new_of = {int(o): i for i, o in enumerate(old) if o >= 0}
    for src in _sources(Y):
        r, c, _ = _pair(J, ctx, src, m, p)
        assert (old[r], old[c]) == ref["pair1"][:2]
        r2, c2, _ = _pair(J, ctx, src, m, p, skip=[r, c])
        assert (old[r2], old[c2]) == ref["pair2"][:2]
        k = n // 3
        sel, _ = _select(J, ctx, src, m, p, 1, [r, c], k)
        assert np.array_equal(old[sel[:, 0]], ref["ks"][:k])
        sel, _ = _select(J, ctx, src, m, p, 2, [r, c, r2, c2], k)
        assert np.array_equal(old[sel[:, 0]], ref["dp"][0][:k]) and np.array_equal(old[sel[:, 1]], ref["dp"][1][:k])
        sel, _ = _select(J, ctx, src, m, p, 1, [r, c], n)                      # every good row, none of the bad ones
        assert np.array_equal(old[sel[:, 0]], ref["ks"])
    src = _sources(Y)[0]
    with pytest.raises(J.JchError) as ei:                                      # n + 1 rows asked, n can be taken
        _select(J, ctx, src, m, p, 1, [new_of[int(ref["ks"][0])], new_of[int(ref["ks"][1])]], n + 1)
    assert ei.value.code == J._lib.JCH_EINVAL
    # the mirror: the bad rows end in test / remain
    res = J.sampks(Y, n // 3, ctx=ctx)
    assert np.array_equal(old[res.train], ref["ks"][:n // 3]) and set(np.flatnonzero(old < 0)) <= set(res.test)
    res = J.sampdp(Y, n // 3, ctx=ctx)
    assert np.array_equal(old[res.train], ref["dp"][0][:n // 3]) and np.array_equal(old[res.test], ref["dp"][1][:n // 3])
    assert set(np.flatnonzero(old < 0)) <= set(res.remain)


def test_farthest_pair_einval(J, ctx):
    X = uniform(6, 3)
    lib, EINVAL = J.load(), J._lib.JCH_EINVAL
    pair, d2 = np.zeros(2, dtype=np.int64), np.zeros(1)

    def call(n, skip, p=3, ldx=6):
        sk = np.asarray(skip, dtype=np.int64)
        return lib.jch_farthest_pair(ctx._h, 0, X.ctypes.data, n, p, ldx, sk.ctypes.data if sk.size else None, sk.size, pair.ctypes.data, d2.ctypes.data)

    assert call(1, []) == EINVAL                                 # one row
    assert call(6, [0, 1, 2, 3, 4]) == EINVAL                    # fewer than two unskipped rows
    assert call(6, [6]) == EINVAL and call(6, [-1]) == EINVAL    # skip out of range
    assert call(6, [], p=0) == EINVAL and call(6, [], ldx=5) == EINVAL
    Y = X.copy(order="F")
    Y[1:, 0] = np.nan                                            # one row without a NaN
    assert lib.jch_farthest_pair(ctx._h, 0, Y.ctypes.data, 6, 3, 6, None, 0, pair.ctypes.data, d2.ctypes.data) == EINVAL
    assert call(6, [0, 1, 2, 3]) == 0 and sorted(pair) == [4, 5]


# ---------------------------------------------------------------------------------- jch_maxmin_select through the C ABI
def _ks_of(n, full):
    return sorted({k for k in (2, 3, n // 3, full) if 2 <= k <= full})


@pytest.mark.parametrize("key", MARGIN_CASES + LATTICES, **IDS)
def test_maxmin_select(J, ctx, key):
    X = case_data(key)
    n, p = X.shape
    ref = reference(key)
    tol = 4 * p * EPS
    srcs = _sources(X)
    sel_ld, d_ld = ref["ks_ld"]
    worst = 0.0
    for k in _ks_of(n, n):
        runs = [_select(J, ctx, src, n, p, 1, ref["ks"][:2], k) for src in (srcs if k == n else srcs[:1])]
        for sel, ds in runs:
            assert np.array_equal(sel[:, 0], ref["ks"][:k]), (key, k)
            want = d_ld[:k, 0].astype(np.float64)
            assert np.all(np.abs(ds[:, 0] - d_ld[:k, 0]) <= tol * want)
            worst = max(worst, float(np.max(np.abs(ds[:, 0] - d_ld[:k, 0]) / np.where(want > 0, want, 1))))
            assert np.array_equal(ds, runs[0][1])                               # host and device X: identical bits
    if n >= 4:
        s1, s2 = ref["dp"]
        sel_ld, d_ld = ref["dp_ld"]
        init = [s1[0], s1[1], s2[0], s2[1]]
        for k in _ks_of(n, n // 2):
            runs = [_select(J, ctx, src, n, p, 2, init, k) for src in (srcs if k == n // 2 else srcs[:1])]
            for sel, ds in runs:
                assert np.array_equal(sel[:, 0], s1[:k]) and np.array_equal(sel[:, 1], s2[:k]), (key, k)
                want = d_ld[:k].astype(np.float64)
                assert np.all(np.abs(ds - d_ld[:k]) <= tol * want)
                worst = max(worst, float(np.max(np.abs(ds - d_ld[:k]) / np.where(want > 0, want, 1))))
                assert np.array_equal(ds, runs[0][1])
    print(f"{key}: worst dsel rel. error {worst:.3g}, bound {tol:.3g}")
    sel, ds = _select(J, ctx, srcs[0], n, p, 1, ref["ks"][:2], min(n, 3), want_dsel=False)   # dsel = NULL
    assert np.array_equal(sel[:, 0], ref["ks"][:min(n, 3)]) and np.all(ds == SENT_D)
    # the farthest pair's d2 is bitwise the dsel of the starting pair
    loc, xa, ldx, _ = srcs[0]
    pair, d2 = np.zeros(2, dtype=np.int64), np.zeros(1)
    ctx.check(J.load().jch_farthest_pair(ctx._h, loc, xa, n, p, ldx, None, 0, pair.ctypes.data, d2.ctypes.data))
    _, ds = _select(J, ctx, srcs[0], n, p, 1, pair, 2)
    assert ds[0, 0] == ds[1, 0] == d2[0]


def test_maxmin_select_einval(J, ctx):
    X = uniform(9, 2)
    lib, EINVAL = J.load(), J._lib.JCH_EINVAL
    sel = np.zeros(32, dtype=np.int64)

    def call(nsets, init, k, n=9):
        init = np.asarray(init, dtype=np.int64)
        return lib.jch_maxmin_select(ctx._h, 0, X.ctypes.data, n, 2, 9, nsets, init.ctypes.data, k, sel.ctypes.data, None)

    assert call(1, [0, 1], 1) == EINVAL and call(1, [0, 1], 10) == EINVAL          # k < 2, k > n
    assert call(2, [0, 1, 2, 3], 5) == EINVAL and call(2, [0, 1, 2, 3], 1) == EINVAL   # 2 k > n
    assert call(1, [3, 3], 4) == EINVAL and call(2, [0, 1, 2, 0], 3) == EINVAL     # repeated
    assert call(1, [0, 9], 4) == EINVAL and call(1, [-1, 2], 4) == EINVAL          # out of range
    assert call(3, [0, 1], 4) == EINVAL and call(0, [0, 1], 4) == EINVAL
    assert call(1, [0, 1], 9) == 0 and sorted(sel[:9]) == list(range(9))
    assert call(2, [0, 1, 2, 3], 4) == 0 and len(set(sel[:8])) == 8


# ---------------------------------------------------------------------------------- sampks / sampdp
def _check_partition(n, *parts):
    allidx = np.concatenate(parts)
    assert allidx.shape[0] == n and np.array_equal(np.sort(allidx), np.arange(n))


@pytest.mark.parametrize("key,metric", [(k_, "eucl") for k_ in [(3, 2), (65, 1), (129, 17), (300, 200), (1000, 16), "lattice130", "lattice_dup"]]
                         + [(k_, "mahal") for k_ in MAHAL_CASES], **IDS)
def test_sampks_sampdp(J, ctx, key, metric):
    X = case_data(key)
    n, p = X.shape
    ref = reference(key, metric)
    Xd = _layouts(np.asfortranarray(X))[0][0][:n]
    for k in sorted({max(2, n // 3), 2, n}):
        for A in (np.array(X), Xd, np.ascontiguousarray(X)):                    # host, device (column-major view, ldx > n), row-major host (copied)
            res = J.sampks(A, k, metric=metric, ctx=ctx)
            assert np.array_equal(res.train, ref["ks"][:k]), (key, metric, k)
            assert np.array_equal(res.test, np.setdiff1d(np.arange(n), ref["ks"][:k]))
            _check_partition(n, res.train, res.test)
        again = J.sampks(np.array(X), k + 0.4, metric, ctx)                     # k = round(k); positional metric and ctx
        assert np.array_equal(again.train, res.train) and np.array_equal(again.test, res.test)
    if n < 4:
        return
    s1, s2 = ref["dp"]
    for k in sorted({max(2, n // 3), 2, n // 2}):
        out = []
        for A in (np.array(X), Xd):
            res = J.sampdp(A, k, metric=metric, ctx=ctx)
            assert np.array_equal(res.train, s1[:k]) and np.array_equal(res.test, s2[:k]), (key, metric, k)
            assert np.array_equal(res.remain, np.setdiff1d(np.arange(n), np.concatenate([s1[:k], s2[:k]])))
            _check_partition(n, res.train, res.test, res.remain)
            out.append(res)
        res = J.sampdp(np.array(X), k, metric=metric, ctx=ctx)                  # two identical calls, identical output
        assert all(np.array_equal(getattr(res, f), getattr(out[0], f)) for f in ("train", "test", "remain"))
    assert np.array_equal(np.asarray(Xd.cpu()), X)                              # X is only read


def test_mahal_needs_a_positive_definite_covariance(J, ctx):
    X = uniform(20, 3)
    Y = np.asfortranarray(np.column_stack([X, np.ones(20)]))                   # a constant column: its row and column of S are exactly zero
    with pytest.raises(ValueError):
        J.sampks(Y, 5, metric="mahal", ctx=ctx)
    with pytest.raises(ValueError):
        J.sampdp(np.ones((20, 1)), 5, metric="mahal", ctx=ctx)                 # p = 1, S = 0


def test_sampks_on_the_scores_of_a_pca_takes_the_device_tensor(J, ctx):
    """The reference's docstring example (sampling.jl:35-37): fm = pcasvd(X; nlv), sampks(fm.T; k, metric = "mahal"), T left on the device by the fit."""
    rng = np.random.default_rng(31)
    n, p, a, k = 300, 40, 5, 40
    X = np.asfortranarray(rng.random((n, a)) @ rng.random((a, p)) * 3 + 0.05 * rng.random((n, p)))
    fm = J.pcasvd(torch.as_tensor(X.T.copy(), device="cuda:0").t(), nlv=a, ctx=ctx)
    assert isinstance(fm.T, torch.Tensor) and fm.T.is_cuda
    T = np.asfortranarray(fm.T.cpu().numpy())
    want = np_sampks(T, k, "mahal")[0]
    from test_samp_static import mahal_space, pair_gap
    Z = mahal_space(T)
    gaps = [pair_gap(Z)]
    np_stream(Z, want[:2], k, 1, np.longdouble, gaps=gaps)
    assert min(gaps) >= 1e-9                                                   # the comparison below is index for index: its margins
    res = J.sampks(fm.T, k, metric="mahal", ctx=ctx)
    assert np.array_equal(res.train, want)
    _check_partition(n, res.train, res.test)
    s1, s2, rem = np_sampdp(T, k, "mahal")
    rd = J.sampdp(fm.T, k, metric="mahal", ctx=ctx)
    assert np.array_equal(rd.train, s1) and np.array_equal(rd.test, s2) and np.array_equal(rd.remain, rem)


# ---------------------------------------------------------------------------------- one larger run
def _farthest_blocked(X, skip=()):
    """The farthest pair of a large X without an n x n matrix: per block of rows the expanded form on centred data finds the candidates (its error,
    1e-13 relative, is far below any margin that passes), extended precision ranks them.  Returns (row, col, relative gap to the runner-up)."""
    n = X.shape[0]
    keep = np.setdiff1d(np.arange(n), np.asarray(skip, dtype=np.int64))
    A = X[keep] - X[keep].mean(axis=0)
    nrm = (A * A).sum(axis=1)
    cands = []
    for b0 in range(0, keep.size, 2000):
        E = nrm[b0:b0 + 2000, None] + nrm[None, :] - 2.0 * (A[b0:b0 + 2000] @ A.T)
        rows = np.arange(E.shape[0])
        E[rows, b0 + rows] = -np.inf
        a1 = E.argmax(axis=1)
        for i in np.argsort(E[rows, a1])[-8:]:                                 # the block's best rows: their best and second best partner
            cands.append((b0 + i, a1[i]))
            row = E[i].copy()
            row[a1[i]] = -np.inf
            cands.append((b0 + i, int(row.argmax())))
    pairs = sorted({(max(keep[i], keep[j]), min(keep[i], keep[j])) for i, j in cands})
    Xl = X.astype(np.longdouble)
    d = np.array([((Xl[r] - Xl[c]) ** 2).sum() for r, c in pairs])
    order = np.argsort(-d, kind="stable")
    return pairs[order[0]][0], pairs[order[0]][1], float((d[order[0]] - d[order[1]]) / d[order[0]])


def test_one_larger_run_on_a_device_x(J, ctx):
    n, p, k = BIG
    X = uniform(n, p)
    Xd = torch.as_tensor(X.T.copy(), device="cuda:0").t()
    r, c, gap = _farthest_blocked(X)
    assert gap >= 1e-9
    gr, gc, d2 = J.farthest_pair(Xd, ctx=ctx)
    assert (gr, gc) == (r, c)
    exact = float(((X[r].astype(np.longdouble) - X[c].astype(np.longdouble)) ** 2).sum())
    assert abs(d2 - exact) <= (p + 2) * 2.0 ** -53 * exact
    gaps = []
    want, _ = np_stream(X, [r, c], k, 1, gaps=gaps)
    assert min(gaps) >= 1e-9
    res = J.sampks(Xd, k, ctx=ctx)
    assert np.array_equal(res.train, want[:, 0])
    _check_partition(n, res.train, res.test)
    r2, c2, gap2 = _farthest_blocked(X, skip=[r, c])
    assert gap2 >= 1e-9
    gaps = []
    want2, _ = np_stream(X, [r, c, r2, c2], k, 2, gaps=gaps)
    assert min(gaps) >= 1e-9
    rd = J.sampdp(Xd, k, ctx=ctx)
    assert np.array_equal(rd.train, want2[:, 0]) and np.array_equal(rd.test, want2[:, 1])
    _check_partition(n, rd.train, rd.test, rd.remain)


# ---------------------------------------------------------------------------------- the three routes of the C entries (tests/host_routes.py)
@pytest.mark.parametrize("entry", sorted(__import__("host_routes").ROUTES["samp"]))
def test_host_arrays_padded_and_unpadded_give_the_bits_of_the_device_route(entry):
    """Device buffers, host arrays with ld == rows and with ld = rows + 3 between NaN guards: equal bytes, NaN padding kept, inputs unchanged."""
    import host_routes as HR
    HR.three_routes(HR.ROUTES["samp"][entry])
