"""GPU parity tests proper (-m gpu): every call goes through the C ABI (libjchemo_hip.so) and is compared
with the oracle / committed golden vectors on the same seeded inputs.  Tolerance: 1e-6 relative Frobenius
on sign-aligned T, P, C (BASELINE.json north_star); observed values are ~1e-13."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import c_oracle as CO
from oracle import plsr_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-6        # north_star tolerance (sign-aligned relative Frobenius)
TIGHT = 1e-9      # what fp64 arithmetic should actually deliver on these well-conditioned cases
FIELDS = ("T", "P", "R", "W", "C")


@pytest.fixture(scope="module")
def J():
    import jchemo_hip
    return jchemo_hip


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    yield c
    c.close()


def _cmp(ref, fm, tol=TIGHT, T=None):
    s = O.sign_align(ref.W, fm.W)
    for f in FIELDS:
        got = getattr(fm, f) if not (f == "T" and T is not None) else T
        e = O.rel_fro(getattr(ref, f), np.asarray(got) * s)
        assert e < tol, (f, e)
    for f in ("TT", "xmeans", "xscales", "ymeans", "yscales"):
        assert O.rel_fro(getattr(ref, f), getattr(fm, f)) < tol, f
    return s


@pytest.mark.parametrize("name", ["cfg1", "cfg1_scal_w", "q1", "ragged", "wide_q"])
@pytest.mark.parametrize("alg", ["kern", "nipals"])
def test_golden_host_arrays(name, alg, golden_cases, J, ctx):
    g = load_golden(name)
    c = golden_cases.CASES[name]
    X, Y, Xt, w = golden_cases.inputs(c)
    X0, Y0 = X.copy(), Y.copy()
    fn = J.plskern if alg == "kern" else J.plsnipals
    fm = fn(X, Y, w, nlv=c["nlv"], scal=c["scal"], ctx=ctx)
    assert np.array_equal(X, X0) and np.array_equal(Y, Y0)          # non-! variant leaves inputs untouched
    k = fm.T.shape[1]
    assert k == min(c["n"], c["p"], c["nlv"])
    s = O.sign_align(g[f"{alg}_W"], fm.W)
    for f in FIELDS:
        assert O.rel_fro(g[f"{alg}_{f}"], getattr(fm, f) * s) < TIGHT, f
    for f in ("TT", "xmeans", "xscales", "ymeans", "yscales", "weights"):
        assert O.rel_fro(g[f"{alg}_{f}"], getattr(fm, f)) < TIGHT, f
    # accessors (src/plskern.jl:187-260) through the device GEMM
    assert O.rel_fro(g[f"{alg}_transform"], J.transform(fm, Xt, ctx=ctx) * s) < TIGHT
    preds = J.predict(fm, Xt, nlv=range(0, k + 1), ctx=ctx)
    assert len(preds) == k + 1
    assert O.rel_fro(g[f"{alg}_pred"], np.stack(preds)) < TIGHT
    B = np.stack([J.coef(fm, nlv=a)[0] for a in range(k + 1)])
    assert O.rel_fro(g[f"{alg}_B"], B) < TIGHT
    sm = J.summary(fm, X, ctx=ctx)
    assert O.rel_fro(g[f"{alg}_summary"], np.stack([sm["var"], sm["pvar"], sm["cumpvar"]])) < TIGHT


@pytest.mark.parametrize("alg", ["kern", "nipals"])
def test_inplace_variants(alg, golden_cases, J, ctx):
    """`plskern!` / `plsnipals!` overwrite X, Y (src/plskern.jl:122-130, src/plsnipals.jl:86-87)."""
    c = golden_cases.CASES["cfg1_scal_w"]
    X, Y, Xt, w = golden_cases.inputs(c)
    Xo, Yo = np.asfortranarray(X.copy()), np.asfortranarray(Y.copy())
    ref = (O.plskern_ if alg == "kern" else O.plsnipals_)(Xo, Yo, w, nlv=c["nlv"], scal=c["scal"])
    Xg, Yg = np.asfortranarray(X.copy()), np.asfortranarray(Y.copy())
    fm = (J.plskern_ if alg == "kern" else J.plsnipals_)(Xg, Yg, w, nlv=c["nlv"], scal=c["scal"], ctx=ctx)
    _cmp(ref, fm)
    assert O.rel_fro(Xo, Xg) < TIGHT and O.rel_fro(Yo, Yg) < TIGHT
    with pytest.raises((ValueError, TypeError)):
        J.plskern_(np.ascontiguousarray(X), Yg, nlv=2, ctx=ctx)       # row-major array cannot be used in place


def test_device_resident_torch(golden_cases, J, ctx):
    import torch
    c = golden_cases.CASES["wide_q"]
    X, Y, Xt, w = golden_cases.inputs(c)
    ref = O.plskern(X, Y, w, nlv=c["nlv"], scal=c["scal"])
    Xd = J.colmajor_empty(*X.shape); Xd.copy_(torch.from_numpy(X))
    Yd = J.colmajor_empty(*Y.shape); Yd.copy_(torch.from_numpy(Y))
    wd = torch.from_numpy(w).cuda()
    tctx = J.Context(0, stream="torch")
    fm = J.plskern(Xd, Yd, wd, nlv=c["nlv"], scal=c["scal"], ctx=tctx)
    assert fm.T.is_cuda and fm.weights.is_cuda
    s = _cmp(ref, fm, T=fm.T.cpu().numpy())
    assert torch.equal(Xd.cpu(), torch.from_numpy(X))               # untouched
    Td = J.transform(fm, Xd, ctx=tctx)
    assert O.rel_fro(O.transform(ref, X), Td.cpu().numpy() * s) < TIGHT
    pd = J.predict(fm, Xd, nlv=3, ctx=tctx)
    assert O.rel_fro(O.predict(ref, X, nlv=3), pd.cpu().numpy()) < TIGHT
    # in place on the device: the caller's tensor now holds the centred/scaled X
    fm2 = J.plskern_(Xd, Yd, wd, nlv=c["nlv"], scal=c["scal"], ctx=tctx)
    Xs = (X - ref.xmeans) / ref.xscales
    assert O.rel_fro(Xs, Xd.cpu().numpy()) < TIGHT
    _cmp(ref, fm2, T=fm2.T.cpu().numpy())
    tctx.close()


@pytest.mark.parametrize("shape", [(20000, 500, 10, 25), (4099, 129, 3, 9), (3000, 1000, 1, 8), (2500, 2047, 2, 5),
                                   (64, 2, 1, 2), (5, 3, 2, 9), (1000, 31, 17, 6), (600, 2500, 2, 6), (300, 4101, 1, 4)])
@pytest.mark.parametrize("alg", ["kern", "nipals"])
def test_seeded_vs_c_oracle(shape, alg, J, ctx):
    """Medium sizes the C oracle finishes in seconds; covers every sweep specialisation (p <= 128 ... 2048),
    odd p, q == 1, q > 16 (two y groups), n not a multiple of any tile, nlv clamping (5 x 3 -> nlv 3)."""
    n, p, q, nlv = shape
    X = CO.fill_uniform(20250112, n, p); Y = CO.fill_uniform(20250113, n, q)
    w = 0.25 + O.splitmix64_uniform(7, 0, n)
    ref = (CO.plskern if alg == "kern" else CO.plsnipals)(X, Y, w, nlv=nlv, scal=True)
    fm = (J.plskern if alg == "kern" else J.plsnipals)(X, Y, w, nlv=nlv, scal=True, ctx=ctx)
    assert fm.T.shape[1] == min(n, p, nlv)
    if min(n, p) <= nlv:     # last LVs of a fully deflated problem are rounding noise: compare the well-posed part
        k = max(1, min(n, p) - 2)
        s = O.sign_align(ref.W[:, :k], fm.W[:, :k])
        assert O.rel_fro(ref.T[:, :k], fm.T[:, :k] * s) < TOL
        return
    _cmp(ref, fm, tol=TOL)
    # sign-invariant products (F3): B = R C', T P'
    assert O.rel_fro(ref.R @ ref.C.T, fm.R @ fm.C.T) < TOL
    assert O.rel_fro(ref.T @ ref.P.T, fm.T @ fm.P.T) < TOL


def test_invariants_on_gpu_result(J, ctx):
    """Size-independent properties on a GPU fit."""
    n, p, q, nlv = 30000, 300, 4, 12
    X = CO.fill_uniform(1, n, p); Y = CO.fill_uniform(2, n, q)
    fm = J.plskern(X, Y, nlv=nlv, ctx=ctx)
    d = fm.weights
    assert abs(d.sum() - 1) < 1e-12
    G = fm.T.T @ (d[:, None] * fm.T)
    assert np.abs(G - np.diag(fm.TT)).max() < 1e-10 * fm.TT.max()
    assert np.abs(fm.R.T @ fm.P - np.eye(nlv)).max() < 1e-9
    assert np.abs(np.linalg.norm(fm.W, axis=0) - 1).max() < 1e-12
    Xc = X - fm.xmeans
    assert O.rel_fro(fm.T, Xc @ fm.R) < 1e-10
    B0, i0 = J.coef(fm, nlv=0)
    assert np.all(B0 == 0) and np.allclose(i0, fm.ymeans[None, :])
    cum = J.summary(fm, X, ctx=ctx)["cumpvar"]
    assert np.all(np.diff(cum) >= -1e-13) and cum[-1] <= 1 + 1e-12
    f2 = J.plskern(X, Y, np.full(n, 3.7), nlv=nlv, ctx=ctx)          # weight rescaling invariance
    s = O.sign_align(fm.W, f2.W)
    assert O.rel_fro(fm.T, f2.T * s) < 1e-9
    # run-to-run bit reproducibility (deterministic two-stage reductions, no float atomics)
    f3 = J.plskern(X, Y, nlv=nlv, ctx=ctx)
    assert np.array_equal(fm.T, f3.T) and np.array_equal(fm.P, f3.P)


def test_y_vector_and_errors(J, ctx):
    X = O.rand_matrix(1, 40, 9); y = O.rand_matrix(2, 40, 1)[:, 0]
    fm = J.plskern(X, y, nlv=3, ctx=ctx)                              # vector y -> n x 1 (ensure_mat)
    ref = O.plskern(X, y, nlv=3)
    _cmp(ref, fm)
    assert isinstance(J.predict(fm, X[:5], ctx=ctx), np.ndarray)
    assert len(J.predict(fm, X[:5], nlv=[1, 3], ctx=ctx)) == 3
    assert len(J.predict(fm, X[:5], nlv=range(-2, 99), ctx=ctx)) == 4
    assert J.transform(fm, X[:5], nlv=99, ctx=ctx).shape == (5, 3)
    with pytest.raises(ValueError):
        J.plskern(X, y[:-1], nlv=2, ctx=ctx)                          # DimensionMismatch
    with pytest.raises(J.JchError):
        J.plskern(X, y, nlv=0, ctx=ctx)
    with pytest.raises(ValueError):
        J.predict(fm, X[:5, :4], ctx=ctx)


def test_degenerate_rank_propagates_nan(J, ctx):
    """H9: Y exhausted -> tt = 0 -> NaN/Inf propagate like the reference (no guard)."""
    X = O.rand_matrix(1, 30, 6)
    fm = J.plskern(X, np.zeros((30, 1)), nlv=2, ctx=ctx)
    assert not np.all(np.isfinite(fm.C))


def test_generator_matches_oracle(J, ctx):
    import ctypes as C
    import torch
    n, p = 1000, 7
    out = J.colmajor_empty(n, p)
    ctx.check(J.load().jch_fill_uniform(ctx._h, out.data_ptr(), n, p, n, 11, 5000, 42))
    assert np.array_equal(out.cpu().numpy(), O.rand_matrix(42, n, p, row0=11, n_total=5000))


def test_sampled_profiling_of_the_sweeps(J):
    """jch_ctx_set_profiling(ctx, N > 1) (include/jchemo_hip.h): event pairs around every N-th launch of the plskern-shaped sweep only
    — an event record costs the stream ~3 us, and bench.py's timed fits should not pay 50 of them.  The profile then reports the
    sampled launches' mean x the launches made: same fields, same results, a sum that agrees with the fully bracketed fit's."""
    import torch
    from jchemo_hip import _lib
    n, p, q, nlv = 40000, 500, 3, 10
    c = J.Context(0, stream="torch")
    X = J.colmajor_empty(n, p); Y = J.colmajor_empty(n, q)
    c.check(J.load().jch_fill_uniform(c._h, X.data_ptr(), n, p, n, 0, n, 5)); c.check(J.load().jch_fill_uniform(c._h, Y.data_ptr(), n, q, n, 0, n, 6))
    c.set_profiling(True)
    J.plskern(X, Y, nlv=nlv, ctx=c)
    t0 = c.counter(_lib.COUNTER_SWEEPS_TIMED)
    fm_all = J.plskern(X, Y, nlv=nlv, ctx=c); pr_all = c.profile()
    assert c.counter(_lib.COUNTER_SWEEPS_TIMED) - t0 == nlv and pr_all.sweep_launches == nlv
    c.set_profiling(3)
    t0 = c.counter(_lib.COUNTER_SWEEPS_TIMED)
    fm_s = J.plskern(X, Y, nlv=nlv, ctx=c); pr_s = c.profile()
    timed = c.counter(_lib.COUNTER_SWEEPS_TIMED) - t0
    assert 3 <= timed <= 4 and pr_s.sweep_launches == nlv                                  # every third of ten launches
    assert 0.6 * pr_all.sweep_ms < pr_s.sweep_ms < 1.6 * pr_all.sweep_ms                    # (short launches on a shared box: a loose band)
    assert abs(pr_s.fit_ms - pr_s.prologue_ms - pr_s.sweep_ms - pr_s.smallstate_ms) < 1e-9
    assert np.array_equal(fm_all.TT, fm_s.TT) and np.array_equal(fm_all.P, fm_s.P)         # timing never touches results
    c.set_profiling(False)
    J.plskern(X, Y, nlv=nlv, ctx=c)
    assert c.counter(_lib.COUNTER_SWEEPS_TIMED) - t0 == timed
    c.close()


def test_rccl_single_rank_plumbing(J):
    """World size 1: exercises dlopen(librccl), ncclCommInitRank and the all-reduce call sites."""
    c = J.Context(0)
    c.comm_init(J.unique_id(), 0, 1)
    X = O.rand_matrix(1, 500, 40); Y = O.rand_matrix(2, 500, 3)
    fm = J.plskern(X, Y, nlv=5, scal=True, ctx=c)
    _cmp(O.plskern(X, Y, nlv=5, scal=True), fm)
    c.close()


@pytest.mark.parametrize("shape", [(20000, 500, 10, 25, False), (4099, 129, 3, 9, True), (3000, 1000, 1, 8, True)])
def test_bf16_storage_mode(shape, J):
    """BASELINE.json configs[2] (bf16 storage): oracle = the Float64 algorithm on the bf16-ROUNDED inputs
    (SURVEY F6 / §8d).  Budget: 1e-3 on sign-aligned T, P, C; 1e-4 on B = R C' and predictions (measured ~1e-5)."""
    import torch
    n, p, q, nlv, scal = shape
    X = CO.fill_uniform(20250112, n, p); Y = CO.fill_uniform(20250113, n, q)
    w = 0.25 + O.splitmix64_uniform(7, 0, n) if scal else None
    Xb = J.colmajor_empty(n, p, dtype=torch.bfloat16); Xb.copy_(torch.from_numpy(X))
    Yb = J.colmajor_empty(n, q, dtype=torch.bfloat16); Yb.copy_(torch.from_numpy(Y))
    Xq = Xb.to(torch.float64).cpu().numpy(); Yq = Yb.to(torch.float64).cpu().numpy()      # the rounded values
    ref = CO.plskern(Xq, Yq, w, nlv=nlv, scal=scal)
    tctx = J.Context(0, stream="torch")
    fm = J.plskern(Xb, Yb, w, nlv=nlv, scal=scal, ctx=tctx)
    T = fm.T.cpu().numpy()
    s = O.sign_align(ref.W, fm.W)
    errs = {f: O.rel_fro(getattr(ref, f), (T if f == "T" else getattr(fm, f)) * s) for f in ("T", "P", "C", "W", "R")}
    errs["B"] = O.rel_fro(ref.R @ ref.C.T, fm.R @ fm.C.T)
    # fp64 statistics from the exact bf16 values; unit weights without scaling (round 4): the column sums come out of the bf16 matrix
    # pipe's f32 block sums (k_xty_bf16_panel_m32) — 1e-9 relative, five orders below the mode's budget
    assert O.rel_fro(ref.xmeans, fm.xmeans) < (1e-12 if scal else 1e-7) and O.rel_fro(ref.xscales, fm.xscales) < 1e-12
    assert max(errs[f] for f in ("T", "P", "C", "W", "R")) < 1e-3, errs
    assert errs["B"] < 1e-4, errs
    # the other fits on bf16-stored inputs (round 4): the inputs are widened exactly and the Float64 path runs — the mode's contract
    # ("the Float64 algorithm on the rounded inputs") to Float64 accuracy
    for name in ("plsnipals", "plssimp", "plsrosa", "plswold"):
        fo = getattr(J, name)(Xb, Yb, w, nlv=min(nlv, 6), scal=scal, ctx=tctx)
        ro = getattr(O, name)(Xq, Yq, w, nlv=min(nlv, 6), scal=scal)
        so = O.sign_align(ro.R, fo.R)
        for f in ("P", "C", "R"):
            assert O.rel_fro(getattr(ro, f), getattr(fo, f) * so) < 1e-8, (name, f)
        assert O.rel_fro(ro.T, fo.T.cpu().numpy() * so) < 1e-8, name
    tctx.close()


@pytest.mark.parametrize("case", [dict(n=2000, p=60, m=41, k=50, nlvdis=8, nlv=6, metric="mahal", scal=False, h=1.0),
                                  dict(n=1500, p=33, m=10, k=40, nlvdis=5, nlv=9, metric="eucl", scal=True, h=2.0),
                                  dict(n=20000, p=500, m=48, k=200, nlvdis=20, nlv=15, metric="mahal", scal=False, h=1.0),
                                  # the kNN scan in 1 / 2 / 3 row segments, rows not a multiple of 256, k at the capacity (768: one
                                  # segment), a single query, one score dimension, more than 8 (two column batches, the last partial)
                                  dict(n=4097, p=20, m=1, k=30, nlvdis=1, nlv=2, metric="eucl", scal=False, h=1.0),
                                  dict(n=9001, p=25, m=7, k=768, nlvdis=3, nlv=4, metric="mahal", scal=False, h=1.5),
                                  dict(n=13000, p=40, m=130, k=300, nlvdis=11, nlv=5, metric="mahal", scal=True, h=1.0, sources=25),
                                  dict(n=50011, p=30, m=33, k=120, nlvdis=17, nlv=6, metric="eucl", scal=False, h=3.0, sources=28)])
def test_lwplsr_predict(case, J, ctx):
    """BASELINE.json configs[4] shape (last case: cfg5 with fewer rows/queries): kNN in the (whitened) global-score
    space, wdist weights, one weighted local plskern per query, predictions for nlv = 0..nlv (src/lwplsr.jl:134-166)."""
    c = case
    X = CO.fill_uniform(20250112, c["n"], c["p"])
    Xq = CO.fill_uniform(20250115, c["m"], c["p"])
    if c.get("sources"):   # latent structure: on iid columns a PLS1 fit has ~8 meaningful LVs, the later scores are rounding noise
        L = CO.fill_uniform(7, c["sources"], c["p"]) - 0.5
        X = CO.fill_uniform(5, c["n"], c["sources"]) @ L + 0.05 * X
        Xq = CO.fill_uniform(6, c["m"], c["sources"]) @ L + 0.05 * Xq
    y = (X[:, :5] @ np.array([1.0, -2.0, 0.5, 3.0, 1.5]) + np.sin(3 * X[:, 5]) + 0.05 * CO.fill_uniform(20250113, c["n"], 1)[:, 0])
    kw = dict(nlvdis=c["nlvdis"], metric=c["metric"], h=c["h"], k=c["k"], nlv=c["nlv"], scal=c["scal"])
    ref = O.lwplsr_predict(O.lwplsr(X, y, **kw), Xq, nlv=range(0, c["nlv"] + 1))
    fm = J.lwplsr(X, y, ctx=ctx, **kw)
    res = J.predict(fm, Xq, nlv=range(0, c["nlv"] + 1), ctx=ctx)
    # neighbours: identical sets in identical order (ties have measure zero for these inputs); distances / weights
    same = np.mean(res.listnn == ref["listnn"])
    assert same > 0.999, same
    assert O.rel_fro(ref["listd"], res.listd) < 1e-9
    assert O.rel_fro(ref["listw"], res.listw) < 1e-7
    pred = np.stack([p_[:, 0] for p_ in res.pred], axis=1)            # m x le
    assert pred.shape == ref["pred"][:, 0, :].shape
    assert O.rel_fro(ref["pred"][:, 0, :], pred) < 1e-7
    a1 = min(3, c["nlv"])
    one = J.predict(fm, Xq, nlv=a1, ctx=ctx)
    assert isinstance(one.pred, np.ndarray) and O.rel_fro(ref["pred"][:, 0, a1], one.pred[:, 0]) < 1e-7


def test_lwplsr_constant_neighbourhood(J, ctx):
    """q == 1 and all neighbour y equal -> that constant for every nlv (src/locwlv.jl:25-28)."""
    n, p = 300, 12
    X = O.rand_matrix(1, n, p)
    y = np.where(X[:, 0] > 0.5, 2.0, -1.0)
    fm = J.lwplsr(X, y, nlvdis=0, metric="eucl", h=1.0, k=5, nlv=3, ctx=ctx)
    Xq = X[:7] + 1e-9
    ref = O.lwplsr_predict(O.lwplsr(X, y, nlvdis=0, metric="eucl", h=1.0, k=5, nlv=3), Xq, nlv=range(0, 4))
    res = J.predict(fm, Xq, nlv=range(0, 4), ctx=ctx)
    pred = np.stack([p_[:, 0] for p_ in res.pred], axis=1)
    assert np.allclose(pred, ref["pred"][:, 0, :], rtol=1e-8, atol=1e-10)


def test_lwplsr_knn_ties_and_duplicates(J, ctx):
    """Exact ties in the kNN scan (round 3: the candidate buffers are compacted by a SAMPLED bar, not sorted): 700 copies of one
    training row, spread over both row segments, sit at the smallest distance of every query, k = 100 cuts through them — the
    sampled bar then keeps > 512 entries and the compaction must fall back to the exact sort; later copies tie with the bar and
    must lose to the earlier ones (ties are broken by the row index, oracle/plsr_oracle.py getknn).  Groups of 4 duplicates
    among the other rows put ties at the k-th place of the ordinary queries as well.  Only the neighbours and distances are
    compared: a neighbourhood of identical rows has no local model."""
    n, p, m = 9000, 10, 6
    X = CO.fill_uniform(11, n, p)
    X[(np.arange(n) // 4) * 4 != np.arange(n)] = 0.0
    X = X + np.repeat(X[::4], 4, axis=0)[:n] * (X == 0.0)       # rows 4 i .. 4 i + 3 identical
    dup = np.arange(5, n, 12)[:700]
    X[dup] = X[dup[0]]
    y = X[:, :3] @ np.array([1.0, -2.0, 0.5]) + 0.05 * CO.fill_uniform(13, n, 1)[:, 0]
    Xq = np.vstack([X[dup[0]][None, :] + 1e-3 * (CO.fill_uniform(12, 3, p) - 0.5), CO.fill_uniform(14, 3, p)])
    kw = dict(nlvdis=3, metric="mahal", h=1.0, k=100, nlv=2)
    with np.errstate(all="ignore"):
        ref = O.lwplsr_predict(O.lwplsr(X, y, **kw), Xq, nlv=range(0, 3))
    fm = J.lwplsr(X, y, ctx=ctx, **kw)
    res = J.predict(fm, Xq, nlv=range(0, 3), ctx=ctx)
    assert np.array_equal(res.listnn, ref["listnn"])
    copies = np.union1d(dup, [4, 5, 6, 7])                     # (row 5 was one of a group of 4 identical rows already)
    assert np.all(np.isin(res.listnn[:3], copies)) and np.array_equal(res.listnn[0], copies[:100])   # the first 100 copies, in index order
    assert O.rel_fro(ref["listd"], res.listd) < 1e-9
    assert O.rel_fro(ref["listw"][3:], res.listw[3:]) < 1e-7
    pred = np.stack([p_[:, 0] for p_ in res.pred], axis=1)
    assert O.rel_fro(ref["pred"][3:, 0, :], pred[3:]) < 1e-6


@pytest.mark.parametrize("kw", [dict(nlvdis=6, metric="mahal", scal=False), dict(nlvdis=4, metric="eucl", scal=True), dict(nlvdis=0, metric="mahal", scal=True),
                                dict(nlvdis=0, metric="eucl", scal=False)])
def test_lwplsr_device_query_map_is_the_same_arithmetic(kw, J, ctx, monkeypatch):
    """jch_lwplsr_add_query_map (round 3): the prepared handle maps the queries to the neighbour-search space itself (transform,
    then the whitening: the stages of `_knn_train_space`).  Same kernels on the same operands as the two jch_affine_gemm calls
    it replaces, so neighbours, distances, weights and predictions must be IDENTICAL to the last bit; without a map (nlvdis = 0,
    eucl, no scaling: the queries are searched in their own coordinates) the call still takes Zq."""
    n, p, m = 2500, 30, 17
    X = CO.fill_uniform(31, n, p); Xq = CO.fill_uniform(32, m, p)
    y = X[:, :4] @ np.array([1.0, -2.0, 0.5, 3.0]) + 0.05 * CO.fill_uniform(33, n, 1)[:, 0]
    full = dict(h=1.5, k=40, nlv=3, **kw)
    fm = J.lwplsr(X, y, ctx=ctx, **full)
    res = J.predict(fm, Xq, nlv=range(0, 4), ctx=ctx)
    assert J.plsr._LWPLSR_PREP[id(fm)]["device_map"] == (kw["nlvdis"] > 0 or kw["scal"] or kw["metric"] == "mahal")
    monkeypatch.setenv("JCH_LW_DEVICE_QMAP", "0")
    fm2 = J.lwplsr(X, y, ctx=ctx, **full)
    ref = J.predict(fm2, Xq, nlv=range(0, 4), ctx=ctx)
    assert not J.plsr._LWPLSR_PREP[id(fm2)]["device_map"]
    assert np.array_equal(res.listnn, ref.listnn) and np.array_equal(res.listd, ref.listd) and np.array_equal(res.listw, ref.listw)
    for a in range(4):
        assert np.array_equal(res.pred[a], ref.pred[a])
    # Zq = NULL without a map that ends in the model's dd columns is refused
    if not J.plsr._LWPLSR_PREP[id(fm2)]["device_map"]:
        from jchemo_hip import _lib
        h = J.plsr._LWPLSR_PREP[id(fm2)]["handle"]
        out = np.empty((m, 1, 1)); Xf = np.asfortranarray(Xq)
        st = _lib.load().jch_lwplsr_predict_prepared(ctx._h, h, _lib.LOC_HOST, None, 0, Xf.ctypes.data, m, m, 40, 1.5, fm2.tol, 0, 1, 1, out.ctypes.data, None, None, None)
        assert st != 0 and b"query map" in _lib.load().jch_last_error(ctx._h)


@pytest.mark.parametrize("case", [dict(n=20000, k=50, levels=4), dict(n=20000, k=300, levels=3), dict(n=60000, k=200, levels=5), dict(n=3000, k=700, levels=2)])
def test_lwplsr_knn_on_a_lattice(case, J, ctx):
    """Neighbours on a LATTICE: integer coordinates in 6 dimensions, so squared distances are small integers and ties are the rule —
    hundreds of training rows at exactly the k-th distance of every query.  The kNN scan's bar test (`==` admits a row only while
    fewer than k are kept), its sampled-bar compactions (every sample equal; survivors beyond the buffer's mark -> the exact
    sort) and the rank merge of the segments must still deliver the first k rows in (distance, index) order, as the oracle does."""
    c = case
    n, p, m = c["n"], 6, 12
    rng = np.random.default_rng(1234 + c["k"])
    X = rng.integers(0, c["levels"], size=(n, p)).astype(np.float64)
    Xq = rng.integers(0, c["levels"], size=(m, p)).astype(np.float64)
    y = X @ np.arange(1.0, p + 1.0) + rng.standard_normal(n)
    kw = dict(nlvdis=0, metric="eucl", h=2.0, k=c["k"], nlv=2)
    with np.errstate(all="ignore"):
        ref = O.lwplsr_predict(O.lwplsr(X, y, **kw), Xq, nlv=range(0, 2))
    fm = J.lwplsr(X, y, ctx=ctx, **kw)
    res = J.predict(fm, Xq, nlv=range(0, 2), ctx=ctx)
    assert np.array_equal(res.listnn, ref["listnn"])
    assert np.array_equal(res.listd, ref["listd"])                 # (square roots of the same small integers)


@pytest.mark.parametrize("knn_path", ["default", "JCH_KNN_SCREEN=0", "JCH_KNN_GENERIC=1"])
def test_lwplsr_nan_query_row(knn_path, J, ctx, monkeypatch):
    """(Run through the three neighbour searches: the screened one — which hands the NaN query to the exact selection —, the exact
    scan, and the exact selection for all queries; round 4: the latter gathered from the sentinel index.)
    A missing value in ONE query row: its scores, hence all its distances, are NaN and no training row ever beats the
    bar.  The reference's arithmetic gives that query NaN predictions (predict on a NaN row) and leaves the others alone;
    the library must do the same and must not gather from the sentinel index (GPU memory fault)."""
    if knn_path != "default":
        monkeypatch.setenv(*knn_path.split("="))
    n, p, m = 3000, 40, 9
    X = CO.fill_uniform(20250112, n, p)
    Xq = CO.fill_uniform(20250115, m, p)
    y = X[:, :4] @ np.array([1.0, -2.0, 0.5, 3.0]) + 0.05 * CO.fill_uniform(20250113, n, 1)[:, 0]
    kw = dict(nlvdis=6, metric="mahal", h=1.0, k=60, nlv=4)
    fm = J.lwplsr(X, y, ctx=ctx, **kw)
    good = J.predict(fm, Xq, nlv=range(0, 5), ctx=ctx)
    Xbad = Xq.copy(); Xbad[4, 7] = np.nan
    res = J.predict(fm, Xbad, nlv=range(0, 5), ctx=ctx)
    assert res.listnn.min() >= 0 and res.listnn.max() < n            # no sentinel reaches the caller
    assert np.all(np.isnan(res.listd[4]))
    keep = np.arange(m) != 4
    for a in range(5):
        assert np.array_equal(res.pred[a][keep], good.pred[a][keep])    # the other queries: bit-identical
        if a > 0:
            assert np.all(np.isnan(res.pred[a][4]))
    assert np.array_equal(res.listnn[keep], good.listnn[keep])
    # an all-NaN query block and a NaN among the TRAINING scores' rows must not fault either
    res2 = J.predict(fm, np.full((3, p), np.nan), nlv=2, ctx=ctx)
    assert res2.listnn.min() >= 0 and res2.listnn.max() < n


def test_full_size_cfg2_vs_oracle(J):
    """BASELINE.json configs[1] at FULL size (n = 1e6, p = 500, q = 10, nlv = 25, Float64, device-resident): the
    north-star parity statement itself — sign-aligned T, P, C within 1e-6 relative Frobenius of the CPU oracle on
    the same seeded inputs — plus size-independent invariants computed on the device."""
    import torch
    n, p, q, nlv = 1_000_000, 500, 10, 25
    tctx = J.Context(0, stream="torch")
    lib = J.load()
    X = J.colmajor_empty(n, p); Y = J.colmajor_empty(n, q)
    tctx.check(lib.jch_fill_uniform(tctx._h, X.data_ptr(), n, p, n, 0, n, 20250112))
    tctx.check(lib.jch_fill_uniform(tctx._h, Y.data_ptr(), n, q, n, 0, n, 20250113))
    fm = J.plskern(X, Y, nlv=nlv, ctx=tctx)
    T, d = fm.T, fm.weights
    # invariants on the device: T'DT = diag(TT), R'P = I, ||w|| = 1, T = Xc R on a row sample
    G = (T.t() @ (d[:, None] * T)).cpu().numpy()
    assert np.abs(G - np.diag(fm.TT)).max() < 1e-9 * fm.TT.max()
    assert np.abs(fm.R.T @ fm.P - np.eye(nlv)).max() < 1e-8
    assert np.abs(np.linalg.norm(fm.W, axis=0) - 1).max() < 1e-12
    rows = torch.arange(0, n, 997, device="cuda")
    Xs = X[rows].cpu().numpy() - fm.xmeans
    assert O.rel_fro(Xs @ fm.R, T[rows].cpu().numpy()) < 1e-9
    # the oracle on identical inputs (host generator == device generator, tests above)
    Xh = CO.fill_uniform(20250112, n, p); Yh = CO.fill_uniform(20250113, n, q)
    ref = CO.plskern_(Xh, Yh, None, nlv=nlv)
    s = O.sign_align(ref.W, fm.W)
    errs = {"T": O.rel_fro(ref.T, T.cpu().numpy() * s), "P": O.rel_fro(ref.P, fm.P * s), "C": O.rel_fro(ref.C, fm.C * s),
            "R": O.rel_fro(ref.R, fm.R * s), "B": O.rel_fro(ref.R @ ref.C.T, fm.R @ fm.C.T)}
    print("cfg2 full-size parity:", {k_: f"{v:.2e}" for k_, v in errs.items()})
    assert max(errs.values()) < TOL, errs
    tctx.close()


def test_cfg4_shape_plsnipals_structured(J, ctx):
    """BASELINE.json configs[3] shape (plsnipals, p = 2000, q = 1, nlv = 50) at n = 20000 on spectra-like inputs
    (60 latent sources + noise: on iid columns PLS1 runs out of Krylov directions after ~10 LVs and every
    implementation returns rounding noise)."""
    n, p, nlv, r = 20000, 2000, 50, 60
    S = CO.fill_uniform(1, n, r); L = CO.fill_uniform(2, r, p)
    X = np.asfortranarray(S @ L + 0.1 * CO.fill_uniform(3, n, p))
    y = np.asfortranarray((S[:, :8] @ np.arange(1.0, 9.0) + 0.05 * CO.fill_uniform(4, n, 1)[:, 0]).reshape(-1, 1))
    ref = CO.plsnipals(X, y, nlv=nlv)
    fm = J.plsnipals(X, y, nlv=nlv, ctx=ctx)
    s = O.sign_align(ref.W, fm.W)
    errs = {f: O.rel_fro(getattr(ref, f), getattr(fm, f) * s) for f in FIELDS}
    assert ref.TT.min() > 1e-9 * ref.TT.max(), "test data ill-posed"
    assert max(errs.values()) < TOL, errs
    Xg, yg = X.copy(order="F"), y.copy(order="F")
    Xo, yo = X.copy(order="F"), y.copy(order="F")
    CO.plsnipals_(Xo, yo, nlv=nlv); J.plsnipals_(Xg, yg, nlv=nlv, ctx=ctx)      # deflated X, Y (north star: "deflated X")
    assert O.rel_fro(Xo, Xg) < TOL and O.rel_fro(yo, yg) < TOL


@pytest.mark.parametrize("alg", ["plsnipals", "plswold"])
@pytest.mark.parametrize("shape", [(3001, 37, 1, 7), (2500, 130, 2, 9), (1800, 300, 3, 6), (1203, 700, 4, 5), (900, 1100, 2, 10),
                                   (700, 1999, 1, 11), (2500, 130, 7, 9), (1500, 500, 10, 8), (900, 1100, 16, 6), (700, 1999, 3, 7)])
def test_postponed_deflation_matches_the_eager_one(alg, shape, J, ctx, monkeypatch):
    """plsnipals / plswold with q <= 16 rewrite the working copy only every m-th LV and re-apply the pending rank-one
    corrections in registers (k_sweep_lazy + k_kpass_lazy for q <= 4, + k_kpass_tile_lazy above).  Every m — including one that does not divide nlv, the
    capacity limit and the in-place variants whose final X is the flushed copy — must reproduce the eager deflation
    (JCH_NIPALS_DEFER=1) to rounding, and the oracle to the usual bound."""
    n, p, q, nlv = shape
    rng = np.random.default_rng(n + p)
    r = max(2 * nlv, q)
    Lt = rng.standard_normal((n, r))
    X = np.asfortranarray(Lt @ rng.standard_normal((r, p)) + 0.4 * rng.standard_normal((n, p)))
    Y = np.asfortranarray(Lt[:, :q] @ rng.standard_normal((q, q)) + 0.2 * rng.standard_normal((n, q)))
    w = rng.uniform(0.5, 1.5, n)
    fit, fit_ = getattr(J, alg), getattr(J, alg + "_")
    ref = getattr(O, alg)(X, Y, w, nlv=nlv)
    monkeypatch.setenv("JCH_NIPALS_DEFER", "1")
    eager = fit(X, Y, w, nlv=nlv, ctx=ctx)
    Xe, Ye = X.copy(order="F"), Y.copy(order="F")
    fit_(Xe, Ye, w, nlv=nlv, ctx=ctx)
    _cmp(ref, eager)
    for m in ("2", "3", "4", "9", "16"):
        monkeypatch.setenv("JCH_NIPALS_DEFER", m)
        lazy = fit(X, Y, w, nlv=nlv, ctx=ctx)
        for f in FIELDS + ("TT",):
            assert O.rel_fro(getattr(eager, f), getattr(lazy, f)) < 1e-11, (m, f)
        Xl, Yl = X.copy(order="F"), Y.copy(order="F")
        fit_(Xl, Yl, w, nlv=nlv, ctx=ctx)
        assert O.rel_fro(Xe, Xl) < 1e-11 and O.rel_fro(Ye, Yl) < 1e-11, m
    monkeypatch.delenv("JCH_NIPALS_DEFER")
    _cmp(ref, fit(X, Y, w, nlv=nlv, ctx=ctx))           # the default


@pytest.mark.parametrize("shape", [(60000, 100, 3, 6), (300, 40, 2, 5), (25000, 500, 10, 8), (4100, 900, 1, 4)])
def test_slice_sums_inside_the_sweep_are_bit_identical(shape, J, ctx, monkeypatch):
    """JCH_SWEEP_FUSED_REDUCE=1 (measured slower, not the default): the first stage of the fixed-order reduction of the
    sweep's partial rows runs in the sweep's last-arriving blocks.  It must produce the very bits of the stand-alone
    `k_reduce_part`, fit after fit (the ticket counters have to return to zero)."""
    n, p, q, nlv = shape
    rng = np.random.default_rng(p)
    Lt = rng.standard_normal((n, 2 * nlv))
    X = np.asfortranarray(Lt @ rng.standard_normal((2 * nlv, p)) + 0.4 * rng.standard_normal((n, p)))
    Y = np.asfortranarray(Lt[:, :q] @ rng.standard_normal((q, q)) + 0.2 * rng.standard_normal((n, q)))
    monkeypatch.setenv("JCH_LV_SPLIT", "0")        # (the one-kernel small-state path: it consumes the slice sums this test is about)
    ref = J.plskern(X, Y, nlv=nlv, ctx=ctx)
    monkeypatch.setenv("JCH_SWEEP_FUSED_REDUCE", "1")
    for _ in range(3):
        fm = J.plskern(X, Y, nlv=nlv, ctx=ctx)
        for f in FIELDS + ("TT",):
            assert np.array_equal(getattr(ref, f), getattr(fm, f)), f
    _cmp(O.plskern(X, Y, nlv=nlv), fm)


@pytest.mark.parametrize("shape", [dict(n=9001, p=500, q=10, nlv=7), dict(n=3000, p=100, q=1, nlv=6), dict(n=70001, p=300, q=3, nlv=5)])
@pytest.mark.parametrize("mode", ["1", "2"])
def test_sweep_with_cached_loads_and_alternating_direction(shape, mode, J, ctx, monkeypatch):
    """Measurement knob JCH_SWEEP_ALT (round 4; NOT the default — slower): default-policy instead of streaming loads
    in the plskern sweep, the row groups walked in alternating directions launch by launch (=1) or always forward (=2).  The same
    sums in another order: results equal the default's to rounding, and a repeated fit reproduces itself bit for bit (every fit
    starts its walk in the same direction)."""
    n, p, q, nlv = (shape[k] for k in ("n", "p", "q", "nlv"))
    X = CO.fill_uniform(421, n, p) + 1.0
    Y = X @ (CO.fill_uniform(422, p, q) - 0.5) + 0.1 * CO.fill_uniform(423, n, q)
    ref = J.plskern(X, Y, nlv=nlv, ctx=ctx)
    monkeypatch.setenv("JCH_SWEEP_ALT", mode)
    a = J.plskern(X, Y, nlv=nlv, ctx=ctx)
    b = J.plskern(X, Y, nlv=nlv, ctx=ctx)
    s = O.sign_align(ref.W, a.W)
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert O.rel_fro(getattr(ref, f), getattr(a, f) * s) < 1e-9, f


@pytest.mark.parametrize("shape", [(70000, 123, 3, 5), (66002, 500, 10, 25), (65537, 500, 2, 20), (131072, 37, 1, 16)])
def test_long_input_accessors(shape, J, ctx, monkeypatch):
    """`transform` / `predict` on inputs long enough for the persistent accessor kernel (whole coefficient matrix in LDS,
    barrier-free row tiles; m >= 65536, even leading dimension) against the tiled kernel (JCH_GEMM_PERSIST=0) and numpy."""
    m, p, q, nlv = shape
    rng = np.random.default_rng(m)
    Lt = rng.standard_normal((3000, 2 * nlv))
    X = np.asfortranarray(Lt @ rng.standard_normal((2 * nlv, p)) + 0.3 * rng.standard_normal((3000, p)) + 2.0)
    Y = np.asfortranarray(Lt[:, :q] @ rng.standard_normal((q, q)) + 0.2 * rng.standard_normal((3000, q)))
    fm = J.plskern(X, Y, nlv=nlv, scal=True, ctx=ctx)
    Xn = np.asfortranarray(rng.standard_normal((m, p)) + 2.0)
    ref_T = ((Xn - fm.xmeans) / fm.xscales) @ fm.R
    got_T = J.transform(fm, Xn, ctx=ctx)
    assert O.rel_fro(ref_T, got_T) < 1e-12
    B = (fm.R @ fm.C.T) / fm.xscales[:, None] * fm.yscales[None, :]
    ref_p = fm.ymeans + (Xn - fm.xmeans) @ B
    got_p = J.predict(fm, Xn, ctx=ctx)
    got_p = got_p[0] if isinstance(got_p, (list, tuple)) else getattr(got_p, "pred", got_p)
    assert O.rel_fro(ref_p, np.asarray(got_p)) < 1e-11
    monkeypatch.setenv("JCH_GEMM_PERSIST", "0")
    assert O.rel_fro(J.transform(fm, Xn, ctx=ctx), got_T) < 1e-13


@pytest.mark.parametrize("shape", [(70000, 60, 3, 12), (4098, 37, 10, 25), (66002, 200, 2, 20), (5001, 45, 5, 9), (4100, 50, 19, 11)])
@pytest.mark.parametrize("resident", [False, True])
def test_long_input_predict_over_an_nlv_range(shape, resident, J, ctx, monkeypatch):
    """`predict(fm, X; nlv = lo:hi)` on long inputs (src/plskern.jl:226-238): one pass over X for the scores, then the prediction
    blocks as running sums over the score columns (k_predict_prefix, round 4) — against numpy for every level; against the one-GEMM
    path (JCH_PREDICT_PREFIX=0: B_a accumulated on the host, le q output columns) to rounding; plain instead of streaming stores
    (JCH_PREDICT_NT=0) bit for bit.  Even and odd m (two rows / one row per thread), q beyond one response slice (19), ranges that
    start above 0, host and device-resident inputs."""
    m, p, q, nlv = shape
    rng = np.random.default_rng(m + nlv)
    Lt = rng.standard_normal((2000, 2 * nlv))
    X = np.asfortranarray(Lt @ rng.standard_normal((2 * nlv, p)) + 0.3 * rng.standard_normal((2000, p)) + 1.0)
    Y = np.asfortranarray(Lt[:, :min(q, 2 * nlv)] @ rng.standard_normal((min(q, 2 * nlv), q)) + 0.2 * rng.standard_normal((2000, q)))
    fm = J.plskern(X, Y, nlv=nlv, scal=True, ctx=ctx)
    Xn = np.asfortranarray(rng.standard_normal((m, p)) + 1.0)
    Xin = Xn
    if resident:
        import torch
        Xin = J.colmajor_empty(m, p); Xin.copy_(torch.from_numpy(Xn))
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)

    def run(lo, hi):
        got = J.predict(fm, Xin, nlv=range(lo, hi + 1), ctx=ctx)
        got = got if isinstance(got, (list, tuple)) else got.pred
        assert len(got) == hi - lo + 1
        return [host(g) for g in got]

    for lo, hi in ((0, nlv), (3, nlv - 1), (nlv - 2, nlv)):
        got = run(lo, hi)
        for a in range(lo, hi + 1):
            B = (fm.R[:, :a] @ fm.C[:, :a].T) / fm.xscales[:, None] * fm.yscales[None, :]
            ref = fm.ymeans + (Xn - fm.xmeans) @ B
            assert O.rel_fro(ref, got[a - lo]) < 1e-11, (lo, hi, a)
        monkeypatch.setenv("JCH_PREDICT_NT", "0")
        for x, y in zip(run(lo, hi), got):
            assert np.array_equal(x, y), "plain vs streaming stores"
        monkeypatch.delenv("JCH_PREDICT_NT")
        monkeypatch.setenv("JCH_PREDICT_PREFIX", "0")
        for a, (x, y) in enumerate(zip(run(lo, hi), got)):
            assert O.rel_fro(x, y) < 1e-12, ("one-GEMM path", lo + a)
        monkeypatch.delenv("JCH_PREDICT_PREFIX")


@pytest.mark.parametrize("shape", [(70000, 60, 3, 12), (4098, 37, 10, 25)])
def test_long_input_xfit_wide_output_kernel(shape, J, ctx, monkeypatch):
    """`xfit` on long inputs (src/xfit.jl:37-56): its second stage (m x nlv scores -> m x p) runs the wide-output accessor kernel,
    whose tile is computed transposed and stored in 16-byte pairs — against numpy, and against the untransposed tile
    (JCH_GEMM_WIDEOUT_PAIRED=0) and the general kernel (JCH_GEMM_WIDEOUT=0)."""
    m, p, q, nlv = shape
    rng = np.random.default_rng(m + nlv)
    Lt = rng.standard_normal((2000, 2 * nlv))
    X = np.asfortranarray(Lt @ rng.standard_normal((2 * nlv, p)) + 0.3 * rng.standard_normal((2000, p)) + 1.0)
    Y = np.asfortranarray(Lt[:, :q] @ rng.standard_normal((q, q)) + 0.2 * rng.standard_normal((2000, q)))
    fm = J.plskern(X, Y, nlv=nlv, scal=True, ctx=ctx)
    Xn = np.asfortranarray(rng.standard_normal((m, p)) + 1.0)
    got = np.asarray(J.xfit(fm, Xn, nlv=nlv, ctx=ctx))
    ref = (((Xn - fm.xmeans) / fm.xscales) @ fm.R) @ (fm.P.T * fm.xscales[None, :]) + fm.xmeans
    assert O.rel_fro(ref, got) < 1e-11
    for knob in ("JCH_GEMM_WIDEOUT_PAIRED", "JCH_GEMM_WIDEOUT"):
        monkeypatch.setenv(knob, "0")
        assert O.rel_fro(np.asarray(J.xfit(fm, Xn, nlv=nlv, ctx=ctx)), got) < 1e-13, knob
        monkeypatch.delenv(knob)


def test_plsnipals_many_lvs_inverse_outside_lds(J, ctx):
    """`R = W inv(P'W)` (src/plsnipals.jl:95) with nlv = 100 > 90: the Gauss-Jordan runs on global scratch instead of LDS copies."""
    n, p, q, nlv = 600, 130, 2, 100
    rng = np.random.default_rng(3)
    X = np.asfortranarray(rng.standard_normal((n, p)) * np.linspace(3.0, 0.5, p))
    Y = np.asfortranarray(X[:, :q] + 0.5 * rng.standard_normal((n, q)))
    fm = J.plsnipals(X, Y, nlv=nlv, ctx=ctx)
    ref = O.plsnipals(X, Y, nlv=nlv)
    assert np.allclose(fm.R.T @ fm.P, np.eye(nlv), atol=1e-8)
    s = O.sign_align(ref.W, fm.W)
    assert O.rel_fro(ref.R, fm.R * s) < 1e-6 and O.rel_fro(ref.T, fm.T * s) < 1e-6


@pytest.mark.parametrize("case", [dict(m=5000, p=40, q=3, k=12, lo=0, hi=12), dict(m=3001, p=30, q=1, k=5, lo=2, hi=9),
                                  dict(m=2500, p=60, q=11, k=40, lo=0, hi=40), dict(m=4000, p=50, q=2, k=45, lo=7, hi=45)])
@pytest.mark.parametrize("resident", [False, True])
def test_score_sums_from_the_scores_equal_those_of_the_predictions(case, resident, J, ctx):
    """jch_score_sums_lv (round 4): the msep / r2 / ... statistics for nlv = lo..hi from running sums over the rows' score columns
    against jch_score_sums on the prediction matrix itself (src/plskern.jl:226-238, src/gridscore.jl:196-216): with and without a
    row mask, ranges that start above 0, levels beyond the fitted LVs (clamped, :228), more than 32 levels (two launches), one
    response and more than eight, host and device-resident inputs."""
    from jchemo_hip import plsr as PL
    m, p, q, k, lo, hi = (case[x] for x in ("m", "p", "q", "k", "lo", "hi"))
    rng = np.random.default_rng(m + k)
    Lt = rng.standard_normal((1500, k))
    X = np.asfortranarray(Lt @ rng.standard_normal((k, p)) + 0.2 * rng.standard_normal((1500, p)) + 1.0)
    Y = np.asfortranarray(Lt[:, :q] @ rng.standard_normal((q, q)) + 0.3 * rng.standard_normal((1500, q)) + 2.0)
    fm = J.plskern(X, Y, nlv=min(k, p), scal=True, ctx=ctx)
    kf = fm.P.shape[1]
    Xn = np.asfortranarray(rng.standard_normal((m, p)) + 1.0)
    Yn = np.asfortranarray(rng.standard_normal((m, q)) + 2.0)
    mask = (rng.random(m) < 0.3).astype(np.float64)
    levels = list(range(lo, hi + 1))
    preds = J.predict(fm, Xn, nlv=range(lo, min(hi, kf) + 1), ctx=ctx)
    preds = preds if isinstance(preds, list) else [preds]
    preds = preds + [preds[-1]] * (len(levels) - len(preds))            # levels beyond the fit repeat the last one
    Pm = np.asfortranarray(np.hstack([np.asarray(z) for z in preds]))
    Tq = J.transform(fm, Xn, ctx=ctx)
    if resident:
        import torch
        dv = lambda a: (lambda t: (t.copy_(torch.from_numpy(a)), t)[1])(J.colmajor_empty(a.shape[0], a.shape[1]))
        Tq, Yin, Pm_in, msk = dv(np.asfortranarray(Tq)), dv(Yn), dv(Pm), torch.from_numpy(mask).cuda()
    else:
        Yin, Pm_in, msk = Yn, Pm, mask
    for mk in (None, msk):
        ref = PL._score_sums(Pm_in, Yin, mk, ctx)
        got = PL._score_sums_lv(Tq, fm, Yin, mk, levels, ctx)
        assert got.shape == ref.shape == (len(levels), q, 6)
        assert np.allclose(got, ref, rtol=1e-10, atol=1e-9 * np.abs(ref).max()), np.abs(got - ref).max()


@pytest.mark.parametrize("shape", [dict(n=3000, p=500, q=10), dict(n=1501, p=37, q=1), dict(n=2200, p=130, q=3), dict(n=900, p=257, q=11),
                                   dict(n=5000, p=384, q=4), dict(n=700, p=512, q=7)])
@pytest.mark.parametrize("resident", [False, True])
def test_fit_from_the_previous_fits_row_major_copy(shape, resident, J, monkeypatch):
    """JCH_REUSE_XCOPY (`reuse_x=True`; round 4): a fit that is promised the SAME X as the previous fit on its ctx takes X'D[Yc | 1]
    from the row-major copy that fit left in the workspace (prologue.hip k_xty_rows) — other weights, other Y, scaling on or off,
    plskern / plsrosa / plssimp — and equals the fit that goes through the whole prologue (JCH_NO_REUSE_XCOPY=1) to rounding.
    The bit is IGNORED (counter unchanged, results right) when the previous fit was on another X, when a fit in between
    replaced the copy (plsnipals deflates it), after a call that re-used the staging buffers, and for q + 1 > 12."""
    import torch
    from jchemo_hip import _lib
    n, p, q = (shape[k] for k in ("n", "p", "q"))
    nlv = min(6, p)
    ctx = J.Context(0)
    X = CO.fill_uniform(431, n, p) + 2.0
    Y = X @ (CO.fill_uniform(432, p, q) - 0.5) + 0.1 * CO.fill_uniform(433, n, q)
    Y2 = Y[:, ::-1].copy() + 0.05 * CO.fill_uniform(434, n, q)
    w1 = CO.fill_uniform(435, n, 1)[:, 0] + 0.1
    w2 = (CO.fill_uniform(436, n, 1)[:, 0] > 0.2).astype(np.float64)           # a cross-validation fold: 0 / 1 weights
    if resident:
        dv = lambda a: (lambda t: (t.copy_(torch.from_numpy(np.asfortranarray(a))), t)[1])(J.colmajor_empty(a.shape[0], a.shape[1]))
        Xi, Yi, Y2i = dv(X), dv(Y), dv(Y2)
        w1i, w2i = torch.from_numpy(w1).cuda(), torch.from_numpy(w2).cuda()
    else:
        Xi, Yi, Y2i, w1i, w2i = np.asfortranarray(X), np.asfortranarray(Y), np.asfortranarray(Y2), w1, w2
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    reused = lambda: ctx.counter(4)                                             # JCH_COUNTER_XCOPY_REUSED

    def same(a, b, tol=1e-10):
        s = O.sign_align(host(a.W), host(b.W))
        for f in FIELDS:
            assert O.rel_fro(host(getattr(a, f)), host(getattr(b, f)) * s) < tol, f
        assert O.rel_fro(a.xmeans, b.xmeans) < 1e-13 and O.rel_fro(a.ymeans, b.ymeans) < 1e-13

    J.plskern(Xi, Yi, w1i, nlv=nlv, ctx=ctx)                                    # leaves the copy
    c0 = reused()
    for fn, kw in ((J.plskern, dict(scal=False)), (J.plskern, dict(scal=True)), (J.plsrosa, dict(scal=False)), (J.plssimp, dict(scal=True))):
        a = fn(Xi, Y2i, w2i, nlv=nlv, ctx=ctx, reuse_x=True, **kw)
        assert reused() == c0 + 1, "the copy was not used"
        c0 += 1
        monkeypatch.setenv("JCH_NO_REUSE_XCOPY", "1")
        b = fn(Xi, Y2i, w2i, nlv=nlv, ctx=ctx, reuse_x=True, **kw)
        monkeypatch.delenv("JCH_NO_REUSE_XCOPY")
        assert reused() == c0
        same(a, b)
        ref = getattr(O, fn.__name__)(X, Y2, w2, nlv=nlv, **kw)
        s = O.sign_align(ref.W, host(a.W))
        for f in FIELDS:
            assert O.rel_fro(getattr(ref, f), host(getattr(a, f)) * s) < 1e-8, (fn.__name__, f)
    # another X (same shape): the promise is false for the workspace, the bit must be ignored
    X3 = X[::-1].copy()
    X3i = dv(X3) if resident else np.asfortranarray(X3)
    a = J.plskern(X3i, Yi, w1i, nlv=nlv, ctx=ctx, reuse_x=True)
    assert reused() == c0
    same(a, J.plskern(X3i, Yi, w1i, nlv=nlv, ctx=J.Context(0)))
    # a fit that replaces the copy by its deflated rows in between
    J.plskern(Xi, Yi, w1i, nlv=nlv, ctx=ctx)
    J.plsnipals(Xi, Yi, w1i, nlv=nlv, ctx=ctx, reuse_x=True)
    a = J.plskern(Xi, Y2i, w2i, nlv=nlv, ctx=ctx, reuse_x=True)
    assert reused() == c0
    same(a, J.plskern(Xi, Y2i, w2i, nlv=nlv, ctx=J.Context(0)))
    # a call that re-uses the staging buffer of X in between (column statistics of other host rows: jch_col_stats)
    from jchemo_hip import plsr as PL
    J.plskern(Xi, Yi, w1i, nlv=nlv, ctx=ctx)
    J.plskern(Xi, Yi, w1i, nlv=nlv, ctx=ctx, reuse_x=True)
    c0 += 1
    assert reused() == c0
    PL._col_stats(np.asfortranarray(X3), None, True, ctx)
    a = J.plskern(Xi, Y2i, w2i, nlv=nlv, ctx=ctx, reuse_x=True)
    assert reused() == (c0 + 1 if resident else c0)       # (device-resident X has no staging copy to lose)
    same(a, J.plskern(Xi, Y2i, w2i, nlv=nlv, ctx=J.Context(0)))
    ctx.close()


def test_fit_from_the_copy_is_refused_for_many_responses(J):
    """q + 1 > 12: the copy-reading kernel has no instantiation, the whole prologue runs (and the result is right)."""
    n, p, q = 1500, 200, 12
    ctx = J.Context(0)
    X = np.asfortranarray(CO.fill_uniform(441, n, p)); Y = np.asfortranarray(X @ (CO.fill_uniform(442, p, q) - 0.5))
    J.plskern(X, Y, nlv=4, ctx=ctx)
    a = J.plskern(X, Y, nlv=4, ctx=ctx, reuse_x=True)
    assert ctx.counter(4) == 0
    ref = O.plskern(X, Y, nlv=4)
    s = O.sign_align(ref.W, a.W)
    assert O.rel_fro(ref.T, a.T * s) < 1e-8
    ctx.close()


def test_scores_and_gridscorelv(J, ctx):
    """§8f rank 1: scores from device-side sums and gridscorelv == the oracle (src/scores.jl, src/gridscore.jl:167-221)."""
    n, p, q, m = 3000, 40, 3, 700
    X = CO.fill_uniform(1, n, p); Xt = CO.fill_uniform(2, m, p)
    B = CO.fill_uniform(3, p, q) - 0.5
    Y = X @ B + 0.1 * CO.fill_uniform(4, n, q); Yt = Xt @ B + 0.1 * CO.fill_uniform(5, m, q)
    fm = O.plskern(X, Y, nlv=6)
    pred = O.predict(fm, Xt, nlv=4)
    for nm in ("msep", "rmsep", "ssr", "bias", "r2", "cor2"):
        assert np.allclose(getattr(J, nm)(pred, Yt, ctx=ctx), getattr(O, nm)(pred, Yt), rtol=1e-9, atol=1e-12), nm
    rng, ref = O.gridscorelv(X, Y, Xt, Yt, score=O.rmsep, fun=O.plskern, nlv=range(0, 9))
    res = J.gridscorelv(X, Y, Xt, Yt, score=J.rmsep, fun=J.plskern, nlv=range(0, 9), ctx=ctx)
    assert res["nlv"] == rng and np.allclose(res["res"], ref, rtol=1e-8)
    custom = J.gridscorelv(X, Y, Xt, Yt, score=lambda pr, yy: O.msep(pr, yy), fun=J.plskern, nlv=[2, 5], ctx=ctx)   # user score
    assert np.allclose(custom["res"], O.gridscorelv(X, Y, Xt, Yt, score=O.msep, fun=O.plskern, nlv=[2, 5])[1], rtol=1e-8)


@pytest.mark.parametrize("scal", [False, True])
def test_gridcvlv_zero_weight_folds(scal, J, ctx):
    """gridcvlv (src/gridcv.jl:187-228): K-fold CV where each fold is a weighted fit with weight 0 on the held-out
    rows (no rmrow copies) and predictions come from the scores T — must equal the oracle's copy-based CV."""
    n, p, q = 1200, 30, 2
    X = CO.fill_uniform(1, n, p)
    B = CO.fill_uniform(3, p, q) - 0.5
    Y = X @ B + 0.2 * CO.fill_uniform(4, n, q)
    segm = J.segmkf(n, 4, rep=2, seed=7)
    assert sorted(np.concatenate(segm[0]).tolist()) == list(range(n))
    ofun = (lambda a, b, nlv: O.plskern(a, b, nlv=nlv, scal=scal))
    rng, ref, ref_rep = O.gridcvlv(X, Y, segm=segm, score=O.msep, fun=ofun, nlv=range(0, 8))
    res = J.gridcvlv(X, Y, segm=segm, score=J.msep, fun=J.plskern, nlv=range(0, 8), ctx=ctx, scal=scal)
    assert res["nlv"] == rng
    assert np.allclose(res["res_rep"], ref_rep, rtol=1e-7) and np.allclose(res["res"], ref, rtol=1e-7)
    best = int(np.argmin(res["res"][:, 0]))
    assert best >= 2                                         # the signal needs a few LVs; nlv = 0 is the worst
    assert res["res"][0, 0] > res["res"][best, 0]


@pytest.mark.parametrize("case", [dict(q=3, p=25, scal=False, metric="mahal"), dict(q=2, p=140, scal=True, metric="eucl"),
                                  dict(q=8, p=300, scal=False, metric="mahal"), dict(q=10, p=25, scal=False, metric="mahal"),
                                  dict(q=16, p=260, scal=True, metric="mahal"), dict(q=13, p=500, scal=False, metric="eucl"),
                                  dict(q=20, p=25, scal=False, metric="mahal")])
def test_lwplsr_multiresponse(case, J, ctx):
    """q > 1: the batched local-fit kernel (q <= 16: kernel matrix p x q and its q x q eigen-solver inside the query's
    workgroup; src/locwlv.jl:18-39 has no limit on q); q > 16 falls back to one device plskern per query.  Host and
    device-resident inputs."""
    import torch
    q, p = case["q"], case["p"]
    n, m = 800, 6
    X = O.rand_matrix(1, n, p); B = O.rand_matrix(2, p, q) - 0.5
    Y = X @ B + np.sin(2 * X[:, :q]) + 0.05 * O.rand_matrix(3, n, q)
    Xq = O.rand_matrix(4, m, p)
    kw = dict(nlvdis=6, metric=case["metric"], h=1.5, k=60, nlv=5, scal=case["scal"])
    ref = O.lwplsr_predict(O.lwplsr(X, Y, **kw), Xq, nlv=range(0, 6))
    res = J.predict(J.lwplsr(X, Y, ctx=ctx, **kw), Xq, nlv=range(0, 6), ctx=ctx)
    assert np.array_equal(res.listnn, ref["listnn"])
    assert O.rel_fro(ref["pred"], np.stack(res.pred, axis=2)) < 1e-8
    one = J.predict(J.lwplsr(X, Y, ctx=ctx, **kw), Xq, nlv=3, ctx=ctx)              # a single nlv -> one matrix (m x q)
    assert one.pred.shape == (m, q) and O.rel_fro(ref["pred"][:, :, 3], one.pred) < 1e-8
    if q <= 16:
        Xd = J.colmajor_empty(n, p); Xd.copy_(torch.from_numpy(X)); Yd = J.colmajor_empty(n, q); Yd.copy_(torch.from_numpy(Y))
        Xqd = J.colmajor_empty(m, p); Xqd.copy_(torch.from_numpy(Xq))
        rd = J.predict(J.lwplsr(Xd, Yd, ctx=ctx, **kw), Xqd, nlv=range(0, 6), ctx=ctx)
        assert O.rel_fro(ref["pred"], np.stack(rd.pred, axis=2)) < 1e-8


@pytest.mark.parametrize("shape", [(2, 1, 1, 1), (3, 5, 2, 4), (1, 3, 1, 2), (7, 1, 3, 2), (65, 129, 16, 3), (129, 2, 2, 2)])
@pytest.mark.parametrize("alg", ["kern", "nipals"])
def test_tiny_and_boundary_shapes(shape, alg, J, ctx):
    """Smallest shapes and tile-boundary shapes (n, p around 64/128, q = 16 = one full y group): same NaN/Inf
    pattern and same finite values as the oracle.  n = 1: the centred data is all zero -> 0/0 everywhere (H9)."""
    n, p, q, nlv = shape
    X = O.rand_matrix(11, n, p); Y = O.rand_matrix(12, n, q)
    with np.errstate(all="ignore"):
        ref = (O.plskern if alg == "kern" else O.plsnipals)(X, Y, nlv=nlv) if n > 1 else None
    fm = (J.plskern if alg == "kern" else J.plsnipals)(X, Y, nlv=nlv, ctx=ctx)
    assert fm.T.shape == (n, min(n, p, nlv))
    if n == 1:
        assert not np.all(np.isfinite(fm.C))
        return
    k = max(1, min(n - 1, p, nlv))       # with n points the centred data has rank <= n-1: later LVs are 0/0 noise
    s = O.sign_align(ref.W[:, :k], fm.W[:, :k])
    for f in ("T", "P", "C"):
        assert O.rel_fro(getattr(ref, f)[:, :k], getattr(fm, f)[:, :k] * s) < 1e-8, f
    assert np.allclose(ref.xmeans, fm.xmeans) and np.allclose(ref.ymeans, fm.ymeans)


def test_zero_weights_and_constant_column(J, ctx):
    """Zero weights drop rows exactly (what gridcvlv relies on); an all-zero X column with scal = true gives a zero
    scale and NaN/Inf exactly where the oracle has them (the reference has no guard, utility.jl:482-487)."""
    n, p, q = 200, 12, 2
    X = O.rand_matrix(1, n, p); Y = O.rand_matrix(2, n, q)
    w = np.ones(n); w[::3] = 0.0
    keep = w > 0
    a = J.plskern(X, Y, w, nlv=4, scal=True, ctx=ctx)
    b = O.plskern(X[keep], Y[keep], nlv=4, scal=True)
    s = O.sign_align(b.W, a.W)
    assert O.rel_fro(b.P, a.P * s) < 1e-10 and O.rel_fro(b.T, a.T[keep] * s) < 1e-10
    Xc = X.copy(); Xc[:, 5] = 0.0        # an all-zero column: mean and variance are exactly 0 in every summation order
    with np.errstate(all="ignore"):      # q = 1 branch (no SVD: LAPACK would throw on the NaN matrix for q > 1)
        r = O.plskern(Xc, Y[:, :1], nlv=2, scal=True)
    g = J.plskern(Xc, Y[:, :1], nlv=2, scal=True, ctx=ctx)
    assert r.xscales[5] == 0.0 and g.xscales[5] == 0.0
    assert np.array_equal(np.isfinite(r.P), np.isfinite(g.P)) and not np.all(np.isfinite(g.P))


@pytest.mark.parametrize("shape", [(20000, 500, 10, 25, False), (4099, 129, 3, 9, True), (3000, 1000, 1, 8, True), (150, 200, 2, 5, False),
                                   (2500, 2047, 2, 5, False), (70, 130, 16, 4, True)])
def test_opt_in_kernel_algorithm_2(shape, J, ctx):
    """SURVEY §8f rank 2 (opt-in, not the reference's algorithm): X'DX once on MFMA f64, zp = G r, tt = r'G r, T = X R.
    Same model as the oracle's algorithm #1 up to rounding (tolerance 1e-6; typically 1e-11)."""
    n, p, q, nlv, scal = shape
    X = CO.fill_uniform(20250112, n, p); Y = CO.fill_uniform(20250113, n, q)
    w = 0.25 + O.splitmix64_uniform(7, 0, n) if scal else None
    ref = CO.plskern(X, Y, w, nlv=nlv, scal=scal)
    fm = J.plskern(X, Y, w, nlv=nlv, scal=scal, ctx=ctx, variant=1)
    _cmp(ref, fm, tol=TOL)
    assert O.rel_fro(ref.R @ ref.C.T, fm.R @ fm.C.T) < TOL
    with pytest.raises(J.JchError):
        J._fit = None  # (keeps flake quiet)
        J.plsr._fit("jch_plsnipals_fit", np.asfortranarray(X), np.asfortranarray(Y), None, 2, False, False, ctx, 1)


@pytest.mark.parametrize("pad", [2, 3])
def test_device_leading_dimension(pad, J):
    """Device matrices that are column slices of taller parents (ld > n; even ld takes the 16-B load paths, odd ld the
    8-B ones) — the Julia side passes stride(X, 2) as ld."""
    import torch
    n, p, q, nlv = 1001, 37, 3, 6
    X = O.rand_matrix(1, n, p); Y = O.rand_matrix(2, n, q)
    ref = O.plskern(X, Y, nlv=nlv, scal=True)
    Xp = J.colmajor_empty(n + pad, p); Yp = J.colmajor_empty(n + pad, q)
    Xp.fill_(float("nan")); Yp.fill_(float("nan"))
    Xd, Yd = Xp[:n], Yp[:n]
    Xd.copy_(torch.from_numpy(X)); Yd.copy_(torch.from_numpy(Y))
    assert Xd.stride() == (1, n + pad)
    tctx = J.Context(0, stream="torch")
    fm = J.plskern(Xd, Yd, nlv=nlv, scal=True, ctx=tctx)
    _cmp(ref, fm, T=fm.T.cpu().numpy())
    assert O.rel_fro(O.transform(ref, X), J.transform(fm, Xd, ctx=tctx).cpu().numpy() * O.sign_align(ref.W, fm.W)) < TIGHT
    fm2 = J.plskern_(Xd, Yd, nlv=nlv, scal=True, ctx=tctx)           # in place through the strided view
    assert O.rel_fro((X - ref.xmeans) / ref.xscales, Xd.cpu().numpy()) < TIGHT and torch.isnan(Xp[n:]).all()
    tctx.close()


def test_plsrda(J, ctx):
    """§8f rank 4: PLSR-DA = plskern on the class dummy table + argmax (src/plsrda.jl:71-120)."""
    n, p = 900, 20
    X = O.rand_matrix(1, n, p)
    score = X[:, 0] + 0.5 * X[:, 1] - X[:, 2]
    y = np.where(score < 0.1, "a", np.where(score < 0.45, "b", "c"))
    Xq = O.rand_matrix(2, 50, p)
    ref = O.plsrda(X, y, nlv=5)
    rp, rpost = O.plsrda_predict(ref, Xq, nlv=range(1, 6))
    fm = J.plsrda(X, y, nlv=5, ctx=ctx)
    gp, gpost = J.predict(fm, Xq, nlv=range(1, 6), ctx=ctx)
    assert list(fm.lev) == list(ref[1]) and list(fm.ni) == list(ref[2])
    for a in range(5):
        assert O.rel_fro(rpost[a], gpost[a]) < TIGHT
        assert np.array_equal(rp[a], gp[a])
    one_pred, one_post = J.predict(fm, Xq, ctx=ctx)
    assert one_pred.shape == (50, 1) and np.array_equal(one_pred, O.plsrda_predict(ref, Xq)[0])


# ------------------------------------------------------------------ sibling algorithms
def _sib_cmp(ref, fm, tol=TIGHT):
    s = O.sign_align(ref.R, fm.R)
    for f in FIELDS:
        e = O.rel_fro(getattr(ref, f), np.asarray(getattr(fm, f)) * s)
        assert e < tol, (f, e)
    for f in ("TT", "xmeans", "xscales", "ymeans", "yscales", "weights"):
        assert O.rel_fro(getattr(ref, f), getattr(fm, f)) < tol, f


@pytest.mark.parametrize("name", ["cfg1", "cfg1_scal_w", "q1", "ragged", "wide_q"])
@pytest.mark.parametrize("alg", ["simp", "rosa", "wold"])
def test_sibling_golden(name, alg, golden_cases, J, ctx):
    """plssimp / plsrosa / plswold through the C ABI vs the committed fixtures (oracle restatements of
    src/plssimp.jl:28-88, src/plsrosa.jl:32-96, src/plswold.jl:36-111)."""
    g = load_golden(name + "_siblings")
    c = golden_cases.CASES[name]
    X, Y, Xt, w = golden_cases.inputs(c)
    ks = min(c["nlv"], golden_cases.SIB_NLV)
    X0, Y0 = X.copy(), Y.copy()
    fm = getattr(J, "pls" + alg)(X, Y, w, nlv=ks, scal=c["scal"], ctx=ctx)
    assert np.array_equal(X, X0) and np.array_equal(Y, Y0)
    s = O.sign_align(g[f"{alg}_R"], fm.R)
    for f in FIELDS:
        assert O.rel_fro(g[f"{alg}_{f}"], getattr(fm, f) * s) < TIGHT, f
    assert O.rel_fro(g[f"{alg}_TT"], fm.TT) < TIGHT
    if alg == "wold":
        assert np.array_equal(g["wold_niter"], fm.niter)       # same number of inner passes, LV by LV
        assert np.all(s == 1.0)                                # the power iteration fixes the sign: no alignment needed
    else:
        assert fm.niter is None
    if alg == "simp":
        assert np.array_equal(fm.W, fm.R)                      # src/plssimp.jl:85-87
    # `!` variants
    Xi, Yi = np.asfortranarray(X.copy()), np.asfortranarray(Y.copy())
    getattr(J, "pls" + alg + "_")(Xi, Yi, w, nlv=ks, scal=c["scal"], ctx=ctx)
    if alg == "simp":
        ref = O.plskern(X, Y, w, nlv=1, scal=c["scal"])
        assert O.rel_fro((X - ref.xmeans) / ref.xscales, Xi) < TIGHT and O.rel_fro((Y - ref.ymeans) / ref.yscales, Yi) < TIGHT
    elif alg == "rosa":
        ref = O.plskern(X, Y, w, nlv=1, scal=c["scal"])
        assert O.rel_fro((X - ref.xmeans) / ref.xscales, Xi) < TIGHT
        assert O.rel_fro(g["rosa_Yinplace"], Yi) < 1e-8
    else:
        assert O.rel_fro(g["wold_Yinplace"], Yi) < 1e-8
        assert abs(np.linalg.norm(Xi) - g["wold_Xinplace_fro"][0]) < 1e-8 * g["wold_Xinplace_fro"][0]


@pytest.mark.parametrize("shape", [(6000, 500, 10, 12), (4099, 129, 3, 9), (3000, 1000, 1, 8), (2500, 2047, 2, 5), (5000, 300, 16, 6)])
@pytest.mark.parametrize("alg", ["simp", "rosa", "wold"])
def test_sibling_seeded_shapes(shape, alg, J, ctx):
    """Seeded structured data (latent sources + noise) so that every LV is well defined; weighted, scaled."""
    n, p, q, nlv = shape
    rng = np.random.default_rng(n + p)
    L = rng.standard_normal((n, 2 * nlv))
    X = np.asfortranarray(L @ rng.standard_normal((2 * nlv, p)) + 0.5 * rng.standard_normal((n, p)))
    ky = min(max(q, 4), 2 * nlv)
    Y = np.asfortranarray(L[:, :ky] @ rng.standard_normal((ky, q)) + 0.3 * rng.standard_normal((n, q)))
    w = rng.uniform(0.5, 1.5, n)
    scal = (n % 2 == 1)
    ref = getattr(O, "pls" + alg)(X, Y, w, nlv=nlv, scal=scal)
    fm = getattr(J, "pls" + alg)(X, Y, w, nlv=nlv, scal=scal, ctx=ctx)
    _sib_cmp(ref, fm, tol=1e-8)
    if alg == "wold":
        assert np.array_equal(ref.niter, fm.niter)
    # device-resident inputs give the same bits as host inputs
    import torch
    Xd = J.colmajor_empty(n, p); Xd.copy_(torch.from_numpy(X))
    Yd = J.colmajor_empty(n, q); Yd.copy_(torch.from_numpy(Y))
    fd = getattr(J, "pls" + alg)(Xd, Yd, torch.from_numpy(w).cuda(), nlv=nlv, scal=scal, ctx=ctx)
    assert np.array_equal(fd.P, fm.P) and np.array_equal(fd.T.cpu().numpy(), fm.T)


def test_sibling_limits_and_wold_options(J, ctx):
    rng = np.random.default_rng(3)
    X = np.asfortranarray(rng.standard_normal((400, 30))); Y = np.asfortranarray(rng.standard_normal((400, 20)))
    for name in ("plssimp", "plswold", "plsrosa"):          # q = 20 > 16: the generic small-state kernel (K in global memory)
        fm = getattr(J, name)(X, Y, nlv=3, ctx=ctx)
        ref = getattr(O, name)(X, Y, nlv=3)
        _sib_cmp(ref, fm, tol=1e-8)
        if name == "plswold":
            assert np.array_equal(ref.niter, fm.niter)
    Xw = np.asfortranarray(rng.standard_normal((300, 2300))); Yw = np.asfortranarray(Xw[:, :3] @ rng.standard_normal((3, 2)) + 0.1 * rng.standard_normal((300, 2)))
    for name in ("plssimp", "plswold"):                     # p > 2048: two-pass wide sweep + generic small-state kernel
        _sib_cmp(getattr(O, name)(Xw, Yw, nlv=4, scal=True), getattr(J, name)(Xw, Yw, nlv=4, scal=True, ctx=ctx), tol=1e-8)
    Y65 = np.asfortranarray(X[:, :20] @ rng.standard_normal((20, 65)) + 0.2 * rng.standard_normal((400, 65)))
    _sib_cmp(O.plssimp(X, Y65, nlv=2), J.plssimp(X, Y65, nlv=2, ctx=ctx), tol=1e-8)          # q > 64 (round 4): no limit any more
    Y4 = np.asfortranarray(Y[:, :4])
    for maxit in (1, 2, 5):
        ref = O.plswold(X, Y4, nlv=3, maxit=maxit)
        fm = J.plswold(X, Y4, nlv=3, maxit=maxit, ctx=ctx)
        assert np.array_equal(ref.niter, fm.niter) and np.all(fm.niter <= maxit)
        _sib_cmp(ref, fm, tol=1e-8)
    ref = O.plswold(X, Y4, nlv=3, tol=1e-3)
    fm = J.plswold(X, Y4, nlv=3, tol=1e-3, ctx=ctx)
    assert np.array_equal(ref.niter, fm.niter)
    _sib_cmp(ref, fm, tol=1e-8)


def test_named_transform_predict_entry_points(golden_cases, J, ctx):
    """jch_transform / jch_predict (the §8b export list) called directly through ctypes."""
    import ctypes as C
    c = golden_cases.CASES["wide_q"]
    X, Y, Xt, w = golden_cases.inputs(c)
    ref = O.plskern(X, Y, w, nlv=c["nlv"])
    fm = J.plskern(X, Y, w, nlv=c["nlv"], ctx=ctx)
    s = O.sign_align(ref.W, fm.W)
    L = J.load()
    m, p = Xt.shape
    q, k = c["q"], fm.P.shape[1]
    Xf = np.asfortranarray(Xt)
    T = np.empty((m, 5), order="F")
    ctx.check(L.jch_transform(ctx._h, 0, Xf.ctypes.data, m, p, m, fm.xmeans.ctypes.data, fm.xscales.ctypes.data,
                              np.asfortranarray(fm.R).ctypes.data, 5, T.ctypes.data, m))
    assert O.rel_fro(O.transform(ref, Xt, nlv=5), T * s[:5]) < TIGHT
    lo, hi = 2, k
    pred = np.empty((m, q * (hi - lo + 1)), order="F")
    R, Cm = np.asfortranarray(fm.R), np.asfortranarray(fm.C)
    ctx.check(L.jch_predict(ctx._h, 0, Xf.ctypes.data, m, p, m, fm.xmeans.ctypes.data, fm.xscales.ctypes.data,
                            fm.ymeans.ctypes.data, fm.yscales.ctypes.data, R.ctypes.data, Cm.ctypes.data, q, lo, hi,
                            pred.ctypes.data, m))
    want = np.concatenate(O.predict(ref, Xt, nlv=range(lo, hi + 1)), axis=1)
    assert O.rel_fro(want, pred) < TIGHT
    assert L.jch_predict(ctx._h, 0, Xf.ctypes.data, m, p, m, None, None, None, None, R.ctypes.data, Cm.ctypes.data, q, 3, 2,
                         pred.ctypes.data, m) == -1


# ------------------------------------------------------------------ row-sharded path on ONE GPU (loopback communicator)
def _run_sharded(J, fn_name, shards, nlv, scal, post=None, **kw):
    """One thread per rank, each with its own ctx (private stream) joined to a loopback group (include/jchemo_hip.h):
    executes exactly the library code of a multi-GPU fit — global weight sum and row count, all-reduced moments and
    XtY, one all-reduce per LV — with the transport replaced by a host-staged sum."""
    import ctypes as C
    import threading
    nr = len(shards)
    L = J.load()
    grp = C.c_void_p()
    assert L.jch_loopback_group_create(nr, C.byref(grp)) == 0
    ctxs = [J.Context(0) for _ in range(nr)]
    out, err = [None] * nr, [None] * nr

    def work(r):
        try:
            ctxs[r].comm_init_loopback(grp, r, nr)
            Xs, Ys, ws = shards[r]
            out[r] = getattr(J, fn_name)(Xs, Ys, ws, nlv=nlv, scal=scal, ctx=ctxs[r], **kw)
            if post is not None:    # further collective calls of the same rank (every rank makes the same sequence)
                out[r] = (out[r], post(out[r], Xs, Ys, ctxs[r]))
        except Exception as e:  # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(nr)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a rank thread is stuck in a collective"
    assert err == [None] * nr, err
    for c in ctxs:
        c.close()
    L.jch_loopback_group_destroy(grp)
    return out


@pytest.mark.parametrize("alg", ["plskern", "plsnipals", "plssimp", "plsrosa", "plswold", "plskern_v2"])
@pytest.mark.parametrize("cuts", [(0.5,), (0.3, 0.7), (0.002, 0.4, 0.75)])
def test_row_sharded_fit_matches_unsharded(alg, cuts, J):
    """rows sharded over 2-4 ranks (uneven shards, the smallest 12 rows against nlv = 7: a shard below
    min(p, nlv) is test_gpu_joined_ctx.py's small-shard case) must give the unsharded result; every replicated output
    must be bit-identical on all ranks."""
    n, p, q, nlv = 6000, 140, 4, 7
    rng = np.random.default_rng(11)
    Lt = rng.standard_normal((n, 2 * nlv))
    X = Lt @ rng.standard_normal((2 * nlv, p)) + 0.5 * rng.standard_normal((n, p))
    Y = Lt[:, :q] @ rng.standard_normal((q, q)) + 0.3 * rng.standard_normal((n, q))
    w = rng.uniform(0.5, 1.5, n)
    edges = [0] + [int(c * n) for c in cuts] + [n]
    shards = [(np.asfortranarray(X[a:b]), np.asfortranarray(Y[a:b]), w[a:b].copy()) for a, b in zip(edges[:-1], edges[1:])]
    assert min(b - a for a, b in zip(edges[:-1], edges[1:])) >= 1
    scal = len(cuts) == 2
    kw = {"variant": 1} if alg == "plskern_v2" else {}
    name = "plskern" if alg == "plskern_v2" else alg
    ref = getattr(O, name)(X, Y, w, nlv=nlv, scal=scal)
    fms = _run_sharded(J, name, shards, nlv, scal, **kw)
    for f in ("P", "R", "W", "C", "TT", "xmeans", "xscales", "ymeans", "yscales"):
        for fm in fms[1:]:
            assert np.array_equal(getattr(fms[0], f), getattr(fm, f)), f      # replicated state: bit-identical
    T = np.concatenate([fm.T for fm in fms], axis=0)
    wn = np.concatenate([fm.weights for fm in fms])
    s = O.sign_align(ref.R, fms[0].R)
    tol = 1e-8
    assert O.rel_fro(ref.T, T * s) < tol and O.rel_fro(ref.weights, wn) < tol
    for f in ("P", "R", "W", "C"):
        assert O.rel_fro(getattr(ref, f), getattr(fms[0], f) * s) < tol, f
    for f in ("TT", "xmeans", "xscales", "ymeans", "yscales"):
        assert O.rel_fro(getattr(ref, f), getattr(fms[0], f)) < tol, f
    if alg == "plswold":
        assert np.array_equal(ref.niter, fms[0].niter)


def test_pars_grids(J, ctx):
    """`pars` grids of gridscorelv / gridcvlv (src/gridscore.jl:191-216, src/gridcv.jl:206-224) and `mpar`
    (src/mpar.jl:15-24): PLS fits over scal, kNN-LWPLSR over (nlvdis, metric, h, k)."""
    assert J.mpar(scal=[False, True], k=[3, 4, 5]) == O.mpar(scal=[False, True], k=[3, 4, 5])
    rng_ = np.random.default_rng(5)
    n, p, q = 900, 40, 2
    Lt = rng_.standard_normal((n, 6))
    X = Lt @ rng_.standard_normal((6, p)) + 0.3 * rng_.standard_normal((n, p))
    Y = Lt[:, :3] @ rng_.standard_normal((3, q)) + 0.2 * rng_.standard_normal((n, q))
    Xt, Yt, X, Y = X[:100], Y[:100], X[100:], Y[100:]
    pars = J.mpar(scal=[False, True])
    for jf, of in ((J.plskern, O.plskern), (J.plssimp, O.plssimp), (J.plswold, O.plswold)):
        _, ref = O.gridscorelv(X, Y, Xt, Yt, score=O.rmsep, fun=of, nlv=range(0, 6), pars=pars)
        res = J.gridscorelv(X, Y, Xt, Yt, score=J.rmsep, fun=jf, nlv=range(0, 6), pars=pars, ctx=ctx)
        assert res["nlv"] == list(range(6)) * 2 and res["scal"] == [False] * 6 + [True] * 6
        assert np.allclose(res["res"], ref, rtol=1e-7, atol=1e-12)
    segm = J.segmkf(X.shape[0], 3, rep=1, seed=1)
    _, ref, ref_rep = O.gridcvlv(X, Y, segm=segm, score=O.msep, fun=O.plskern, nlv=range(0, 5), pars=pars)
    res = J.gridcvlv(X, Y, segm=segm, score=J.msep, fun=J.plskern, nlv=range(0, 5), pars=pars, ctx=ctx)
    assert np.allclose(res["res"], ref, rtol=1e-6) and np.allclose(res["res_rep"], ref_rep, rtol=1e-6)
    assert res["scal"] == [False] * 5 + [True] * 5
    with pytest.raises(ValueError):
        J.gridscorelv(X, Y, Xt, Yt, score=J.rmsep, fun=J.plskern, nlv=3, pars=dict(nlv=[1]), ctx=ctx)
    # kNN-LWPLSR grid (the reference's own example, src/gridcv.jl:47-57, at a small size); y univariate
    y = Y[:, :1]; yt = Yt[:, :1]
    lp = J.mpar(nlvdis=[4], metric=["mahal"], h=[1.0, 3.0], k=[40, 80])
    _, ref = O.gridscorelv(X, y, Xt, yt, score=O.rmsep, fun=O.lwplsr, nlv=range(0, 4), pars=lp)
    res = J.gridscorelv(X, y, Xt, yt, score=J.rmsep, fun=J.lwplsr, nlv=range(0, 4), pars=lp, ctx=ctx)
    assert res["h"] == [1.0] * 4 + [3.0] * 4 + [1.0] * 4 + [3.0] * 4 and res["k"] == [40] * 8 + [80] * 8
    assert np.allclose(res["res"], ref, rtol=1e-6)


def test_grid_verbose_prints_what_the_reference_prints(J, ctx, capsys):
    """`verbose = true` of gridscorelv / gridcvlv (src/gridscore.jl:178,189,191,217; src/gridcv.jl:197,202,226)."""
    rng_ = np.random.default_rng(6)
    X = rng_.standard_normal((300, 12)); Y = X[:, :2] + 0.1 * rng_.standard_normal((300, 2))
    pars = J.mpar(scal=[False, True])
    quiet = J.gridscorelv(X[50:], Y[50:], X[:50], Y[:50], score=J.rmsep, fun=J.plskern, nlv=range(0, 3), pars=pars, ctx=ctx)
    assert capsys.readouterr().out == ""
    loud = J.gridscorelv(X[50:], Y[50:], X[:50], Y[:50], score=J.rmsep, fun=J.plskern, nlv=range(0, 3), pars=pars, verbose=True, ctx=ctx)
    out = capsys.readouterr().out
    assert out.splitlines() == ["-- Nb. combinations = 2", "scal => False", "scal => True", "-- End."]
    assert np.array_equal(quiet["res"], loud["res"])
    J.gridscorelv(X[50:], Y[50:], X[:50], Y[:50], score=J.rmsep, fun=J.plskern, nlv=2, verbose=True, ctx=ctx)
    assert capsys.readouterr().out.splitlines() == ["-- Nb. combinations = 0.", "-- End."]
    J.gridcvlv(X, Y, segm=J.segmkf(300, 3, rep=2, seed=1), score=J.msep, fun=J.plskern, nlv=range(0, 3), verbose=True, ctx=ctx)
    assert capsys.readouterr().out == "/ repl=1 segm=1 segm=2 segm=3 / repl=2 segm=1 segm=2 segm=3 / End.\n"


def test_row_sharded_bf16_and_reductions(J):
    """BASELINE configs[2] is the bf16 storage mode on 8 GPUs: its sharded path (fp64 statistics and all-reduces from
    bf16 rows) on 3 loopback ranks vs the single-rank bf16 fit; plus the sharded `summary` (jch_weighted_ss) and
    score sums (jch_score_sums), whose results are sums over all ranks' shards."""
    import torch
    n, p, q, nlv = 9000, 200, 3, 6
    X = CO.fill_uniform(20250112, n, p); Y = CO.fill_uniform(20250113, n, q)
    w = 0.25 + O.splitmix64_uniform(7, 0, n)
    edges = [0, 2500, 2600, n]

    def dev_shard(a, b, dtype):
        Xs = J.colmajor_empty(b - a, p, dtype=dtype); Xs.copy_(torch.from_numpy(X[a:b]))
        Ys = J.colmajor_empty(b - a, q, dtype=dtype); Ys.copy_(torch.from_numpy(Y[a:b]))
        return Xs, Ys, torch.from_numpy(w[a:b].copy()).cuda()

    # ---- bf16: sharded == unsharded (same arithmetic up to the order of the fp64 partial sums)
    whole = dev_shard(0, n, torch.bfloat16)
    tctx = J.Context(0)
    one = J.plskern(*whole, nlv=nlv, scal=True, ctx=tctx)
    torch.cuda.synchronize()
    fms = _run_sharded(J, "plskern", [dev_shard(a, b, torch.bfloat16) for a, b in zip(edges[:-1], edges[1:])], nlv, True)
    for f in ("P", "R", "W", "C", "TT", "xmeans", "xscales"):
        assert np.array_equal(getattr(fms[0], f), getattr(fms[2], f)), f
        assert O.rel_fro(getattr(one, f), getattr(fms[0], f)) < 1e-5, f       # fp32 row arithmetic: partial-sum order differs
    T = torch.cat([fm.T for fm in fms], dim=0).cpu().numpy()
    assert O.rel_fro(one.T.cpu().numpy(), T) < 1e-5
    # ---- f64: summary and scores over the shards
    ref = O.plskern(X, Y, w, nlv=nlv)
    sm_ref = O.summary(ref, X)
    pr_ref = np.concatenate(O.predict(ref, X, nlv=range(0, nlv + 1)), axis=1)
    ms_ref = np.stack([O.msep(pr_ref[:, i * q:(i + 1) * q], Y) for i in range(nlv + 1)]).reshape(nlv + 1, q)

    def post(fm, Xs, Ys, ctx):
        sm = J.summary(fm, Xs, ctx=ctx)
        res = J.gridscorelv(Xs, Ys, Xs, Ys, score=J.msep, fun=lambda a, b, nlv, ctx: fm, nlv=range(0, nlv + 1), ctx=ctx)
        return sm["cumpvar"], res["res"]

    outs = _run_sharded(J, "plskern", [dev_shard(a, b, torch.float64) for a, b in zip(edges[:-1], edges[1:])], nlv, False, post=post)
    for fm, (cum, ms) in outs:
        assert O.rel_fro(sm_ref["cumpvar"], cum) < 1e-9
        assert np.allclose(ms, ms_ref, rtol=1e-8)
    tctx.close()


def test_vip_xfit_xresid(golden_cases, J, ctx):
    """§8f rank 4 accessors of a fitted Plsr: vip (src/vip.jl:62-107), xfit / xresid (src/xfit.jl:37-93)."""
    import torch
    for name in ("cfg1_scal_w", "wide_q"):
        c = golden_cases.CASES[name]
        X, Y, Xt, w = golden_cases.inputs(c)
        ref = O.plskern(X, Y, w, nlv=c["nlv"], scal=c["scal"])
        fm = J.plskern(X, Y, w, nlv=c["nlv"], scal=c["scal"], ctx=ctx)
        for k in (None, 0, 1, 3):
            assert O.rel_fro(O.xfit(ref, Xt, nlv=k), J.xfit(fm, Xt, nlv=k, ctx=ctx)) < TIGHT
            assert O.rel_fro(O.xresid(ref, Xt, nlv=k), J.xresid(fm, Xt, nlv=k, ctx=ctx)) < 1e-8
        for k in (None, 2):
            assert O.rel_fro(O.vip(ref, nlv=k)["imp"], J.vip(fm, nlv=k)["imp"]) < TIGHT
            vr, vg = O.vip(ref, Y, nlv=k), J.vip(fm, Y, nlv=k, ctx=ctx)
            assert O.rel_fro(vr["imp"], vg["imp"]) < TIGHT and O.rel_fro(vr["rdd"], vg["rdd"]) < TIGHT
    # device-resident model and data
    Xd = J.colmajor_empty(*X.shape); Xd.copy_(torch.from_numpy(X))
    Yd = J.colmajor_empty(*Y.shape); Yd.copy_(torch.from_numpy(Y))
    fd = J.plskern(Xd, Yd, torch.from_numpy(w).cuda(), nlv=c["nlv"], scal=c["scal"], ctx=ctx)
    assert O.rel_fro(O.vip(ref, Y)["imp"], J.vip(fd, Yd, ctx=ctx)["imp"]) < TIGHT
    assert O.rel_fro(O.xresid(ref, X, nlv=2), J.xresid(fd, Xd, nlv=2, ctx=ctx).cpu().numpy()) < 1e-8


def test_bf16_vector_prologue_tails(J):
    """bf16 storage with a padded leading dimension (ld % 8 == 0, n % 8 != 0): the 16-byte prologue kernels take their
    row-tail branches; result must equal the scalar-prologue result of the same data bit for bit in the fp64 statistics."""
    import torch
    n, ld, p, q, nlv = 1003, 1008, 77, 2, 5
    X = CO.fill_uniform(20250112, n, p); Y = CO.fill_uniform(20250113, n, q)
    w = 0.25 + O.splitmix64_uniform(7, 0, n)
    Xb = J.colmajor_empty(ld, p, dtype=torch.bfloat16)[:n]; Xb.copy_(torch.from_numpy(X))
    Yb = J.colmajor_empty(ld, q, dtype=torch.bfloat16)[:n]; Yb.copy_(torch.from_numpy(Y))
    assert Xb.stride() == (1, ld)
    Xq = Xb.to(torch.float64).cpu().numpy(); Yq = Yb.to(torch.float64).cpu().numpy()
    ref = O.plskern(Xq, Yq, w, nlv=nlv, scal=True)
    tctx = J.Context(0, stream="torch")
    fm = J.plskern(Xb, Yb, w, nlv=nlv, scal=True, ctx=tctx)
    s = O.sign_align(ref.W, fm.W)
    assert O.rel_fro(ref.xmeans, fm.xmeans) < 1e-12 and O.rel_fro(ref.xscales, fm.xscales) < 1e-12
    assert O.rel_fro(ref.ymeans, fm.ymeans) < 1e-12 and O.rel_fro(ref.yscales, fm.yscales) < 1e-12
    for f in ("P", "C", "W", "R"):
        assert O.rel_fro(getattr(ref, f), getattr(fm, f) * s) < 1e-3, f
    assert O.rel_fro(ref.T, fm.T.cpu().numpy() * s) < 1e-3
    tctx.close()


@pytest.mark.parametrize("quad", [False, True])
@pytest.mark.parametrize("prior", ["unif", "prop"])
def test_plslda_plsqda(quad, prior, J, ctx):
    """§8f rank 4: plslda / plsqda (src/plslda.jl:76-130, src/plsqda.jl:23-34; lda.jl, qda.jl, matW.jl, dmnorm.jl)."""
    import torch
    rng = np.random.default_rng(8)
    n, p, nlv = 900, 40, 5
    y = rng.integers(0, 4, n)
    y[0] = 7                                           # a class with ONE observation (src/matW.jl:36-45)
    X = rng.standard_normal((n, p)) + (y % 4)[:, None] * np.linspace(0, 1.5, p)[None, :] + 0.3 * rng.standard_normal((n, 1))
    Xt = rng.standard_normal((60, p)) + rng.integers(0, 4, 60)[:, None] * np.linspace(0, 1.5, p)[None, :]
    w = rng.uniform(0.5, 1.5, n)
    of, jf = (O.plsqda, J.plsqda) if quad else (O.plslda, J.plslda)
    if quad:
        y = np.where(y == 7, 0, y)                     # (QDA of a single point has no Cholesky; the reference fails there too)
    ref = of(X, y, w, nlv=nlv, prior=prior, scal=True)
    mod = jf(X, y, w, nlv=nlv, prior=prior, scal=True, ctx=ctx)
    assert np.array_equal(ref["lev"], mod.lev) and np.array_equal(ref["ni"], mod.ni)
    rp, rpo = O.plslda_predict(ref, Xt, nlv=range(1, nlv + 1))
    gp, gpo = J.predict(mod, Xt, nlv=range(1, nlv + 1), ctx=ctx)
    for k in range(nlv):
        assert np.abs(rpo[k] - gpo[k]).max() < 1e-8, k
        assert np.array_equal(rp[k], gp[k])
    one_p, one_po = J.predict(mod, Xt, ctx=ctx)
    assert np.array_equal(one_p, rp[-1]) and np.abs(one_po - rpo[-1]).max() < 1e-8
    with pytest.raises(ValueError):
        J.predict(mod, Xt, nlv=0, ctx=ctx)
    # device-resident training data and queries
    Xd = J.colmajor_empty(n, p); Xd.copy_(torch.from_numpy(X)); Xtd = J.colmajor_empty(60, p); Xtd.copy_(torch.from_numpy(Xt))
    md = jf(Xd, y, torch.from_numpy(w).cuda(), nlv=nlv, prior=prior, scal=True, ctx=ctx)
    dp, dpo = J.predict(md, Xtd, nlv=3, ctx=ctx)
    assert np.abs(dpo - rpo[2]).max() < 1e-8 and np.array_equal(dp, rp[2])


@pytest.mark.parametrize("bscal", ["none", "frob"])
@pytest.mark.parametrize("scal", [False, True])
def test_mbplsr(bscal, scal, J, ctx):
    """§8f rank 4: multiblock PLSR (src/mbplsr.jl:64-113; transform / predict src/mbplswest.jl:220-254) — raw blocks
    side by side + ONE vector of column divisors through jch_plskern_fit_scaled vs the oracle's materialised blocks."""
    import torch
    rng = np.random.default_rng(2)
    n, nlv = 700, 4
    Lt = rng.standard_normal((n, 5))
    Xbl = [Lt @ rng.standard_normal((5, 30)) * 3 + 1 + 0.2 * rng.standard_normal((n, 30)), Lt[:, :2] @ rng.standard_normal((2, 8)) + 0.1 * rng.standard_normal((n, 8)),
           0.2 * (Lt @ rng.standard_normal((5, 17))) + 0.05 * rng.standard_normal((n, 17))]
    Y = Lt[:, :3] @ rng.standard_normal((3, 2)) + 0.1 * rng.standard_normal((n, 2))
    w = rng.uniform(0.5, 1.5, n)
    Xnew = [b[:40] + 0.01 for b in Xbl]
    ref = O.mbplsr(Xbl, Y, w, nlv=nlv, bscal=bscal, scal=scal)
    fm = J.mbplsr(Xbl, Y, w, nlv=nlv, bscal=bscal, scal=scal, ctx=ctx)
    s = O.sign_align(ref["R"], fm.R)
    assert O.rel_fro(ref["T"], fm.T * s) < TIGHT and O.rel_fro(ref["R"], fm.R * s) < TIGHT and O.rel_fro(ref["C"], fm.C * s) < TIGHT
    assert O.rel_fro(ref["bscales"], fm.bscales) < 1e-12 and O.rel_fro(ref["ymeans"], fm.ymeans) < 1e-12 and O.rel_fro(ref["yscales"], fm.yscales) < 1e-12
    for k in range(3):
        assert O.rel_fro(ref["xmeans"][k], fm.xmeans[k]) < 1e-12 and O.rel_fro(ref["xscales"][k], fm.xscales[k]) < 1e-12
    assert O.rel_fro(ref["fm"].P, fm.fm.P * s) < TIGHT and np.all(fm.fm.xscales == 1.0) and np.all(fm.fm.xmeans == 0.0)
    assert O.rel_fro(O.mbplsr_transform(ref, Xnew, nlv=3), J.mbplsr_transform(fm, Xnew, nlv=3, ctx=ctx) * s[:3]) < TIGHT
    rp = O.mbplsr_predict(ref, Xnew, nlv=range(0, nlv + 1))
    gp = J.predict(fm, Xnew, nlv=range(0, nlv + 1), ctx=ctx)
    assert O.rel_fro(np.stack(rp), np.stack(gp)) < TIGHT
    # device-resident blocks
    Xd = []
    for b in Xbl:
        t = J.colmajor_empty(*b.shape); t.copy_(torch.from_numpy(b)); Xd.append(t)
    fd = J.mbplsr(Xd, Y, w, nlv=nlv, bscal=bscal, scal=scal, ctx=ctx)
    assert O.rel_fro(ref["T"], fd.T.cpu().numpy() * O.sign_align(ref["R"], fd.R)) < TIGHT
    with pytest.raises(ValueError):
        J.mbplsr(Xbl, Y, nlv=2, bscal="mfa", ctx=ctx)


@pytest.mark.parametrize("scal", [False, True])
@pytest.mark.parametrize("offset", [0.0, 1e4])
def test_raw_mode_matches_centred_copy(offset, scal, J, ctx, monkeypatch):
    """plskern without scaling keeps an UNCENTRED row-major copy and folds the centring into the sweeps (fit.hip, raw
    mode); JCH_CENTRED_COPY=1 selects the centred-copy formulation.  Both must agree with the oracle, also when the column
    means dwarf the spread (offset 1e4, spread 0.3: the input itself then carries only ~1e-12 relative precision)."""
    n, p, q, nlv = 5000, 120, 3, 6
    rng = np.random.default_rng(4)
    Lt = rng.standard_normal((n, 8))
    X = np.asfortranarray(0.3 * (Lt @ rng.standard_normal((8, p))) + 0.1 * rng.standard_normal((n, p)) + offset)
    Y = np.asfortranarray(Lt[:, :3] @ rng.standard_normal((3, q)) + 0.1 * rng.standard_normal((n, q)) + offset / 7)
    w = rng.uniform(0.5, 1.5, n)
    X[:, 5] *= 40.0; X[:, 7] *= 0.01                       # very different column spreads (matters when scal = true)
    ref = O.plskern(X, Y, w, nlv=nlv, scal=scal)
    tol = 1e-9 if offset == 0.0 else 1e-7
    raw = J.plskern(X, Y, w, nlv=nlv, scal=scal, ctx=ctx)
    _cmp(ref, raw, tol=tol)
    monkeypatch.setenv("JCH_CENTRED_COPY", "1")
    cen = J.plskern(X, Y, w, nlv=nlv, scal=scal, ctx=ctx)
    _cmp(ref, cen, tol=tol)
    s = O.sign_align(raw.W, cen.W)
    assert O.rel_fro(raw.T, cen.T * s) < tol and O.rel_fro(raw.xmeans, cen.xmeans) < 1e-13


def _offset_design(n, p, q, seed, offset):
    rng = np.random.default_rng(seed)
    Lt = rng.standard_normal((n, 6))
    X = np.asfortranarray(Lt @ rng.standard_normal((6, p)) / np.sqrt(6.0) + 0.2 * rng.standard_normal((n, p)) + offset)
    Y = np.asfortranarray(Lt[:, :3] @ rng.standard_normal((3, q)) + 0.1 * rng.standard_normal((n, q)))
    return X, Y


def test_raw_mode_pivot_unrepresentative_leading_rows(J, ctx, monkeypatch):
    """the raw-mode pivot used to be the mean of the FIRST 64 rows.  Here those rows are blanks
    (zeros) while every other row has mean 1e4 and spread ~1: the strided 256-row sample (prologue.hip k_pivot_rows)
    sees one blank row, lands within ~40 spreads of the means, and the raw fit equals the centred-copy fit to <= 1e-9
    (the old pivot was 1e4 spreads off: error ~1e-8 * 1e8)."""
    n, p, q, nlv = 30000, 150, 3, 6
    X, Y = _offset_design(n, p, q, 11, 1e4)
    X[:64, :] = 0.0
    before = ctx.counter(0)
    raw = J.plskern(X, Y, nlv=nlv, ctx=ctx)
    assert ctx.counter(0) == before                     # the sampled pivot was good enough: no fallback needed
    monkeypatch.setenv("JCH_CENTRED_COPY", "1")
    cen = J.plskern(X, Y, nlv=nlv, ctx=ctx)
    s = O.sign_align(cen.W, raw.W)
    for f in FIELDS:
        assert O.rel_fro(getattr(cen, f), getattr(raw, f) * s) < 1e-9, f
    _cmp(O.plskern(X, Y, nlv=nlv), raw, tol=1e-9)


@pytest.mark.parametrize("pattern", ["periodic_blanks", "row_drift"])
def test_raw_mode_falls_back_to_centred_copy_when_the_pivot_is_poor(pattern, J, ctx, monkeypatch):
    """ADVICE r1 (fit.hip:219): no automatic fallback existed.  periodic_blanks: every row the strided sample looks at
    is a blank while the data sit at 1e4 -> pivot 0, sample spread 0 -> the fit notices |mean - pivot| / spread > 64 when
    it fetches its results and repeats itself on the centred copy (jch_ctx_get_counter counts it); the answer is then the
    centred formulation's, bit for bit.  row_drift: sorted / trending rows, per-column offsets — the strided sample
    spans the drift, so no refit and agreement to 1e-9."""
    n, p, q, nlv = 25600, 96, 2, 5
    X, Y = _offset_design(n, p, q, 12, 0.0)
    if pattern == "periodic_blanks":
        X += 1e4
        X[:: n // 256, :] = 0.0                         # exactly the rows k_pivot_rows samples
    else:
        X += np.linspace(0.0, 300.0, n)[:, None] + np.linspace(-1e3, 1e3, p)[None, :]
    before = ctx.counter(0)
    raw = J.plskern(X, Y, nlv=nlv, ctx=ctx)
    refits = ctx.counter(0) - before
    monkeypatch.setenv("JCH_CENTRED_COPY", "1")
    cen = J.plskern(X, Y, nlv=nlv, ctx=ctx)
    if pattern == "periodic_blanks":
        assert refits == 1
        for f in FIELDS + ("TT", "xmeans"):
            assert np.array_equal(getattr(cen, f), getattr(raw, f)), f
    else:
        assert refits == 0
        s = O.sign_align(cen.W, raw.W)
        for f in FIELDS:
            assert O.rel_fro(getattr(cen, f), getattr(raw, f) * s) < 1e-9, f
    _cmp(O.plskern(X, Y, nlv=nlv), raw, tol=1e-8)


@pytest.mark.parametrize("shape", [(6400, 500, 10, 6, False), (6477, 504, 15, 5, False), (2048 + 9, 40, 16, 4, False), (5000, 130, 3, 5, True),
                                  (3333, 1000, 2, 4, False), (64, 24, 1, 3, False), (4160, 777, 7, 4, True)])
@pytest.mark.parametrize("nh", [2, 4])
def test_bf16_row_panel_prologue_matches_tile_kernel(shape, nh, J):
    """Round 3: the row-panel bf16 prologue (k_center_xty_bf16_panel: complete rows out of an LDS tile, MFMA operands straight
    from the load registers) against the round-1 tile kernel on the same device data: the fp64 statistics, X'DY (seen through
    the first weight vector) and the raw row-major copy (seen through the whole fit) must agree; also vs the oracle on the
    rounded inputs.  Shapes: full tiles only / ragged tail / one piece (NT = 1) / q = 16 (no spare ones column) / scal /
    two 512-column groups / n == one tile / odd piece count."""
    import os
    import torch
    n, p, q, nlv, scal = shape
    ld = (n + 7) // 8 * 8
    X = CO.fill_uniform(20250112, n, p); Y = CO.fill_uniform(20250113, n, q)
    Xb = J.colmajor_empty(ld, p, dtype=torch.bfloat16)[:n]; Xb.copy_(torch.from_numpy(X))
    Yb = J.colmajor_empty(ld, q, dtype=torch.bfloat16)[:n]; Yb.copy_(torch.from_numpy(Y))
    w = 0.25 + O.splitmix64_uniform(7, 0, n) if scal else None
    tctx = J.Context(0, stream="torch")
    keep = {k_: os.environ.get(k_) for k_ in ("JCH_BF16_K2_PANEL", "JCH_BF16_K2_NH", "JCH_BF16_K2_M32")}
    try:
        os.environ["JCH_BF16_K2_M32"] = "0"      # (the f64 products of this kernel; the bf16-pipe variant has its own test below)
        os.environ["JCH_BF16_K2_PANEL"] = "0"
        old = J.plskern(Xb, Yb, w, nlv=nlv, scal=scal, ctx=tctx)
        os.environ["JCH_BF16_K2_PANEL"] = "1"; os.environ["JCH_BF16_K2_NH"] = str(nh)
        new = J.plskern(Xb, Yb, w, nlv=nlv, scal=scal, ctx=tctx)
    finally:
        for k_, v_ in keep.items():
            if v_ is None:
                os.environ.pop(k_, None)
            else:
                os.environ[k_] = v_
    for f in ("xmeans", "ymeans", "xscales", "yscales"):
        assert O.rel_fro(getattr(old, f), getattr(new, f)) < 1e-13, f
    s = O.sign_align(old.W, new.W)
    assert O.rel_fro(old.W[:, 0], new.W[:, 0] * s[0]) < 1e-11                    # w_1 is a function of X'DY alone
    for f in ("P", "C", "W", "R"):
        assert O.rel_fro(getattr(old, f), getattr(new, f) * s) < 1e-5, f          # (fp32 sweeps amplify 1e-16 differences of K)
    assert O.rel_fro(old.T.cpu().numpy(), new.T.cpu().numpy() * s) < 1e-5
    ref = CO.plskern(Xb.to(torch.float64).cpu().numpy(), Yb.to(torch.float64).cpu().numpy(), w, nlv=nlv, scal=scal)
    s = O.sign_align(ref.W, new.W)
    assert O.rel_fro(ref.xmeans, new.xmeans) < 1e-12
    for f in ("P", "C", "W", "R"):
        assert O.rel_fro(getattr(ref, f), getattr(new, f) * s) < 1e-3, f
    assert O.rel_fro(ref.T, new.T.cpu().numpy() * s) < 1e-3
    tctx.close()


@pytest.mark.parametrize("shape", [(4096, 500, 10, 8), (5003, 130, 3, 6), (640, 64, 1, 4), (3000, 700, 15, 5), (64, 40, 2, 3)])
@pytest.mark.parametrize("data", ["uniform", "signal", "magnitudes"])
def test_bf16_prologue_on_the_bf16_matrix_pipe(shape, data, J, monkeypatch):
    """Round 4: unit weights, no scaling — X'[Y | 1] of the bf16 prologue on v_mfma_f32_16x16x32_bf16 (k_xty_bf16_panel_m32: the raw
    bf16 values are the operands, every product exact in f32, 32-term block sums in f32, f64 across blocks, centring afterwards on
    the p x q sums) against the f64-product kernel (JCH_BF16_K2_M32=0) and the oracle on the rounded inputs, inside the mode's
    budget (1e-3 on T / P / C / W, 1e-4 on predictions).  `magnitudes`: columns spanning 2^-20 ... 2^20 (the adversarial case for an
    f32 block sum followed by a centring subtraction); ragged tails, one piece, two column groups, q = 15 (ones column = the last pad)."""
    import torch
    n, p, q, nlv = shape
    ld = (n + 7) // 8 * 8
    X = CO.fill_uniform(20250112, n, p); Y = CO.fill_uniform(20250113, n, q)
    if data == "signal":
        Y = X[:, :q] * 0.7 + 0.3 * Y
    if data == "magnitudes":
        X = X * np.exp2(np.round(np.linspace(-20, 20, p)))[None, :]
        Y = (X[:, :q] / np.exp2(np.round(np.linspace(-20, 20, p)))[None, :q] + 0.2 * Y) * np.exp2(np.round(np.linspace(-10, 10, q)))[None, :]
    Xb = J.colmajor_empty(ld, p, dtype=torch.bfloat16)[:n]; Xb.copy_(torch.from_numpy(X))
    Yb = J.colmajor_empty(ld, q, dtype=torch.bfloat16)[:n]; Yb.copy_(torch.from_numpy(Y))
    tctx = J.Context(0, stream="torch")
    new = J.plskern(Xb, Yb, nlv=nlv, ctx=tctx)
    monkeypatch.setenv("JCH_BF16_K2_M32", "0")
    old = J.plskern(Xb, Yb, nlv=nlv, ctx=tctx)
    assert O.rel_fro(old.xmeans, new.xmeans) < 1e-6 and O.rel_fro(old.ymeans, new.ymeans) < 1e-12
    s = O.sign_align(old.W, new.W)
    assert O.rel_fro(old.W[:, 0], new.W[:, 0] * s[0]) < 2e-5                     # w_1 is a function of X'DY alone: the f32 block sums
    Xr, Yr = Xb.to(torch.float64).cpu().numpy(), Yb.to(torch.float64).cpu().numpy()
    ref = CO.plskern(Xr, Yr, None, nlv=nlv, scal=False)
    s = O.sign_align(ref.W, new.W)
    assert O.rel_fro(ref.xmeans, new.xmeans) < 1e-6
    for f in ("P", "C", "W", "R"):
        assert O.rel_fro(getattr(ref, f), getattr(new, f) * s) < 1e-3, f
    assert O.rel_fro(ref.T, new.T.cpu().numpy() * s) < 1e-3
    Xq = Xb[: min(n, 200)]
    assert O.rel_fro(O.predict(ref, Xr[: min(n, 200)], nlv=nlv), J.predict(new, Xq, nlv=nlv, ctx=tctx).cpu().numpy()) < 1e-4
    tctx.close()


@pytest.mark.parametrize("case", [dict(n=6000, p=500, m=37, k=200, q=1, nlv=15, scal=False), dict(n=5000, p=333, m=19, k=208, q=1, nlv=12, scal=True),
                                  dict(n=4000, p=130, m=9, k=150, q=3, nlv=7, scal=False), dict(n=3000, p=257, m=11, k=129, q=8, nlv=6, scal=True),
                                  dict(n=2500, p=64, m=5, k=31, q=2, nlv=5, scal=False), dict(n=2000, p=40, m=7, k=60, q=1, nlv=48, scal=False),
                                  dict(n=3000, p=1030, m=6, k=200, q=5, nlv=4, scal=False)])
def test_lwplsr_kspace_matches_pspace(case, J, ctx):
    """Round 3: the two local-fit kernels of predict(::Lwplsr) on the same neighbours — the neighbour-space kernel (Gram matrix
    of the gathered rows on the matrix cores, held in registers: lwplsr_kspace.hip, forced with JCH_LOCW_KSPACE=2) against
    the p-space kernel (one sweep of the k x p slab per LV: JCH_LOCW_KSPACE=0), and both against the oracle.  Shapes: the
    cfg5 k and p; k = 208 (all 13 row blocks full) with scal; q = 3 / 8 / 5 (eigen-solver path); k, p not multiples of
    16 / 32; a small k (zero-padded blocks); nlv = 48 > p (clamped local models); p > 1024."""
    import os
    c = case
    Lsrc = CO.fill_uniform(7, 25, c["p"]) - 0.5
    X = CO.fill_uniform(5, c["n"], 25) @ Lsrc + 0.05 * CO.fill_uniform(20250112, c["n"], c["p"])
    Xq = CO.fill_uniform(6, c["m"], 25) @ Lsrc + 0.05 * CO.fill_uniform(20250115, c["m"], c["p"])
    Y = np.column_stack([X[:, (3 * j) % c["p"]] * (1.0 + 0.3 * j) - X[:, (5 * j + 1) % c["p"]] + np.sin(2 * X[:, (j + 2) % c["p"]])
                         + 0.05 * CO.fill_uniform(20250113 + j, c["n"], 1)[:, 0] for j in range(c["q"])])
    kw = dict(nlvdis=6, metric="mahal", h=1.5, k=c["k"], nlv=c["nlv"], scal=c["scal"])
    rng = range(0, c["nlv"] + 1)
    keep = os.environ.get("JCH_LOCW_KSPACE")
    try:
        os.environ["JCH_LOCW_KSPACE"] = "2"
        ks = J.predict(J.lwplsr(X, Y, ctx=ctx, **kw), Xq, nlv=rng, ctx=ctx)
        os.environ["JCH_LOCW_KSPACE"] = "0"
        # (p > 1024 with q > 4: the p-space kernel's LDS bookkeeping does not fit and, with the neighbour-space kernel switched off,
        # the call runs the per-query generic fits — round 4: no shape is refused; the comparison below then is k-space vs generic)
        ps = J.predict(J.lwplsr(X, Y, ctx=ctx, **kw), Xq, nlv=rng, ctx=ctx)
    finally:
        if keep is None:
            os.environ.pop("JCH_LOCW_KSPACE", None)
        else:
            os.environ["JCH_LOCW_KSPACE"] = keep
    assert np.array_equal(ps.listnn, ks.listnn) and np.array_equal(ps.listw, ks.listw)     # same neighbours, same weights
    ref = O.lwplsr_predict(O.lwplsr(X, Y, **kw), Xq, nlv=rng)
    hi = min(c["nlv"], c["p"], c["k"])
    for a in range(len(ps.pred)):
        e_kp = O.rel_fro(ps.pred[a], ks.pred[a])
        e_or = O.rel_fro(ref["pred"][:, :, a], ks.pred[a])
        # the late LVs of a 48-LV local model on 60 neighbours are conditioning noise in ANY fp64 implementation: compare what is defined
        tol_kp, tol_or = (1e-9, 1e-7) if a <= min(hi, 20) else (1e-4, 1e-4)
        assert e_kp < tol_kp, (a, e_kp)
        assert e_or < tol_or, (a, e_or)


def test_plswold_zero_weight_rows_both_modes(J, ctx):
    """src/plswold.jl:107 `Tx .= (1 ./ sqrtw) .* Tx`: the reference returns NaN scores for rows whose weight is 0 (0 * Inf).  Default
    here: finite scores t_i = x_i' r for such rows (what zero-weight cross-validation folds need); `zero_weight_nan = True`
    (desc->reserved |= JCH_WOLD_REF_ZERO_WEIGHT_NAN) reproduces the reference.  Everything else is identical in the two modes."""
    n, p, q, nlv = 400, 30, 3, 5
    X = O.rand_matrix(3, n, p); Y = O.rand_matrix(4, n, q)
    w = 0.5 + O.splitmix64_uniform(11, 0, n)
    zero = np.array([5, 17, 123, 399]); w[zero] = 0.0
    a = J.plswold(X, Y, w, nlv=nlv, ctx=ctx)
    b = J.plswold(X, Y, w, nlv=nlv, zero_weight_nan=True, ctx=ctx)
    keep = np.ones(n, bool); keep[zero] = False
    assert np.all(np.isfinite(a.T))
    assert np.all(np.isnan(b.T[zero])) and np.all(np.isfinite(b.T[keep]))
    assert np.array_equal(a.T[keep], b.T[keep])
    for f in ("P", "R", "W", "C", "TT", "xmeans", "niter"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    # default mode: the scores of the zero-weight rows are their transformed rows
    assert O.rel_fro(J.transform(a, X[zero], ctx=ctx), a.T[zero]) < 1e-10
    # oracle (which mirrors the reference's arithmetic incl. the division by sqrt(w)) on the positive-weight rows
    ref = O.plswold(X[keep], Y[keep], w[keep], nlv=nlv)
    s = O.sign_align(ref.W, b.W)
    assert O.rel_fro(ref.T, b.T[keep] * s) < 1e-8 and O.rel_fro(ref.P, b.P * s) < 1e-8
    # device-resident inputs take the same path
    import torch
    Xd = J.colmajor_empty(n, p); Xd.copy_(torch.from_numpy(X)); Yd = J.colmajor_empty(n, q); Yd.copy_(torch.from_numpy(Y))
    c = J.plswold(Xd, Yd, torch.from_numpy(w).cuda(), nlv=nlv, zero_weight_nan=True, ctx=ctx)
    Tc = c.T.cpu().numpy()
    assert np.all(np.isnan(Tc[zero])) and np.array_equal(Tc[keep], b.T[keep])


@pytest.mark.parametrize("shape", [dict(n=3000, p=500, q=10, nlv=25), dict(n=900, p=37, q=1, nlv=12), dict(n=1200, p=130, q=2, nlv=9),
                                   dict(n=2000, p=257, q=3, nlv=20), dict(n=2500, p=64, q=7, nlv=30), dict(n=1500, p=1000, q=16, nlv=15),
                                   dict(n=700, p=16, q=5, nlv=16), dict(n=400, p=301, q=12, nlv=40)])
@pytest.mark.parametrize("variant", ["raw", "scal_w", "centred", "rosa"])
def test_split_small_state_matches_one_kernel_path(shape, variant, J, ctx, monkeypatch):
    """Round 4: the per-LV small-state step as two kernels (smallstate_split.hip: a p-parallel kernel on (p + 15) / 16 CUs + a
    single-workgroup kernel that starts at the eigenvector) against the one-kernel path (JCH_LV_SPLIT=0) and the oracle: the same
    arithmetic with the sums over p taken block-wise, so agreement to rounding (1e-8 on the leading LVs: a PLS1 fit on uniform columns loses a digit per LV in ANY summation order), every QP instantiation (q = 1 ... 16),
    raw mode / scaling + weights / centred copy, plsrosa, nlv beyond 32 (R rows past the register prefetch)."""
    n, p, q, nlv = (shape[k] for k in ("n", "p", "q", "nlv"))
    X = CO.fill_uniform(401, n, p) + 3.0
    B0 = CO.fill_uniform(402, p, q) - 0.5
    Y = X @ B0 + 0.1 * CO.fill_uniform(403, n, q)
    w = CO.fill_uniform(404, n, 1)[:, 0] + 0.2 if variant == "scal_w" else None
    scal = variant == "scal_w"
    fn, ofn = (J.plsrosa, O.plsrosa) if variant == "rosa" else (J.plskern, O.plskern)
    if variant == "centred":
        monkeypatch.setenv("JCH_CENTRED_COPY", "1")
    fm = fn(X, Y, w, nlv=nlv, scal=scal, ctx=ctx)
    monkeypatch.setenv("JCH_LV_SPLIT", "0")
    fm1 = fn(X, Y, w, nlv=nlv, scal=scal, ctx=ctx)
    ref = ofn(X, Y, w, nlv=nlv, scal=scal)
    k = fm.T.shape[1]
    assert k == fm1.T.shape[1] == min(n, p, nlv)
    # the leading LVs (conditioning of later ones on collinear-ish uniform data is a property of the data, not of the path)
    kk = min(k, 8)
    s1 = O.sign_align(fm1.W[:, :kk], fm.W[:, :kk])
    for f in FIELDS:
        assert O.rel_fro(getattr(fm1, f)[:, :kk], getattr(fm, f)[:, :kk] * s1) < 1e-8, (f, "split vs one kernel")
    assert O.rel_fro(fm1.TT[:kk], fm.TT[:kk]) < 1e-8
    s = O.sign_align(ref.W[:, :kk], fm.W[:, :kk])
    for f in FIELDS:
        assert O.rel_fro(getattr(ref, f)[:, :kk], getattr(fm, f)[:, :kk] * s) < 1e-8, (f, "split vs oracle")
    # invariants on ALL LVs: T'DT = diag(TT), R'P = I
    d = fm.weights
    G = (fm.T * d[:, None]).T @ fm.T
    # Since the end of round 4 the split path carries Z = P'K in its DIRECT form (Z_i = P_i'K_new summed over the blocks): every shape
    # and variant holds this to <= 7e-16 (profiles/r04f_invariant_probe.txt).  With the incremental update Z_i - (P_i.zp) c' the PLS1 shape
    # (n = 900, p = 37, q = 1, nlv = 12: K falls by 1e8 over the fit) sat at 2e-10 ... 1.1e-9 where the oracle holds 2e-15
    # (profiles/r04d_invariant_probe.txt, tools/z_recurrence_drift.py) — the bound below pins the direct form.
    assert np.abs(G - np.diag(fm.TT)).max() < 1e-12 * np.abs(fm.TT).max()
    assert np.abs(fm.R.T @ fm.P - np.eye(k)).max() < 1e-8


@pytest.mark.parametrize("shape", [dict(n=3000, p=500, q=10, nlv=25), dict(n=900, p=37, q=1, nlv=12), dict(n=1200, p=130, q=2, nlv=9),
                                   dict(n=2000, p=257, q=3, nlv=20), dict(n=2500, p=64, q=7, nlv=30), dict(n=1500, p=1000, q=16, nlv=15),
                                   dict(n=700, p=16, q=5, nlv=16), dict(n=400, p=301, q=12, nlv=40), dict(n=5000, p=2048, q=4, nlv=6)])
@pytest.mark.parametrize("variant", ["raw", "scal_w", "centred", "rosa", "bf16"])
def test_merged_small_state_kernel_is_the_two_launch_path_bit_for_bit(shape, variant, J, ctx, monkeypatch):
    """Round 4, second half, OPT-IN (JCH_LV_MERGED=1; measured slower, kept as a knob): ONE launch per LV (k_lv_merged: every block
    runs the p-parallel half, the block that arrives last at the fit's counter goes on as the single-workgroup half —
    smallstate_split.hip) against the default two launches.  The same code on the same data in the same order, so every output is IDENTICAL, bit for bit; and a repeated
    fit reproduces itself (which block arrives last differs from launch to launch — it must not matter).  Every QP instantiation,
    raw mode / scaling + weights / centred copy, plsrosa, the bf16 storage mode, nlv beyond 32, one block (p = 16) and the most
    blocks the LDS-resident path takes (p = 2048)."""
    n, p, q, nlv = (shape[k] for k in ("n", "p", "q", "nlv"))
    X = CO.fill_uniform(411, n, p) + 3.0
    B0 = CO.fill_uniform(412, p, q) - 0.5
    Y = X @ B0 + 0.1 * CO.fill_uniform(413, n, q)
    w = CO.fill_uniform(414, n, 1)[:, 0] + 0.2 if variant == "scal_w" else None
    scal = variant == "scal_w"
    fn = J.plsrosa if variant == "rosa" else J.plskern
    kw = dict(nlv=nlv, scal=scal, ctx=ctx)
    if variant == "bf16":   # device-resident bf16 inputs: the storage mode (results come back as device tensors)
        import torch
        Xb = J.colmajor_empty(n, p, dtype=torch.bfloat16); Xb.copy_(torch.from_numpy(X))
        Yb = J.colmajor_empty(n, q, dtype=torch.bfloat16); Yb.copy_(torch.from_numpy(Y))
        X, Y = Xb, Yb
    if variant == "centred":
        monkeypatch.setenv("JCH_CENTRED_COPY", "1")
    monkeypatch.setenv("JCH_LV_MERGED", "1")
    a = fn(X, Y, w, **kw)
    b = fn(X, Y, w, **kw)
    monkeypatch.delenv("JCH_LV_MERGED")
    c = fn(X, Y, w, **kw)
    host = lambda v: v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    for f in FIELDS + ("TT",):
        assert np.array_equal(host(getattr(a, f)), host(getattr(b, f))), (f, "merged kernel does not reproduce itself")
        assert np.array_equal(host(getattr(a, f)), host(getattr(c, f))), (f, "merged vs two launches")
    assert np.all(np.isfinite(host(a.T)))


@pytest.mark.parametrize("shape", [dict(n=4000, p=500, q=10, nlv=14), dict(n=1500, p=60, q=1, nlv=8), dict(n=2500, p=300, q=4, nlv=13),
                                   dict(n=1200, p=1500, q=3, nlv=9), dict(n=900, p=2000, q=1, nlv=20), dict(n=3000, p=130, q=16, nlv=7)])
@pytest.mark.parametrize("alg", ["nipals", "wold"])
def test_one_pass_nipals_is_the_default_path_to_rounding(shape, alg, J, ctx):
    """Round 4, OPT-IN (JCH_NIPALS_ONE_PASS, `one_pass=True`; never the default): plsnipals / plswold with ONE pass over X per LV —
    K_{a+1} = K_a - zp_raw c_raw' / tt in the small-state kernel instead of the recomputation of X'DY from the deflated matrices
    (src/plsnipals.jl:71), c_raw against the undeflated Y, rows written back every 6th LV.  Gate: <= 1e-9 against the default path
    and <= 1e-6 against the oracle on the leading LVs; every write-back period (nlv not a multiple of it), both small-state
    kernels (LDS-resident; generic at p = 1500 / 2000), q = 1 ... 16; plswold's iteration counts unchanged; the `!` variants and
    shapes outside the postponed write-back refuse the flag."""
    n, p, q, nlv = (shape[k] for k in ("n", "p", "q", "nlv"))
    Lt = CO.fill_uniform(501, n, 16) - 0.5
    X = Lt @ (CO.fill_uniform(502, 16, p) - 0.5) + 0.05 * CO.fill_uniform(503, n, p) + 1.0
    Y = Lt[:, :q] @ (CO.fill_uniform(504, q, q) - 0.5) + (Lt[:, 3:4] ** 2) + 0.05 * CO.fill_uniform(505, n, q)
    w = CO.fill_uniform(506, n, 1)[:, 0] + 0.5
    fn, ofn = (J.plsnipals, O.plsnipals) if alg == "nipals" else (J.plswold, O.plswold)
    one = fn(X, Y, w, nlv=nlv, scal=True, ctx=ctx, one_pass=True)
    dflt = fn(X, Y, w, nlv=nlv, scal=True, ctx=ctx)
    ref = ofn(X, Y, w, nlv=nlv, scal=True)
    kk = min(nlv, 8)
    s = O.sign_align(dflt.W[:, :kk], one.W[:, :kk])
    for f in ("T", "P", "W", "C"):
        assert O.rel_fro(getattr(dflt, f)[:, :kk], getattr(one, f)[:, :kk] * s) < 1e-9, (f, "one pass vs default")
    s = O.sign_align(ref.W[:, :kk], one.W[:, :kk])
    for f in ("T", "P", "W", "C"):
        assert O.rel_fro(getattr(ref, f)[:, :kk], getattr(one, f)[:, :kk] * s) < 1e-6, (f, "one pass vs oracle")
    if alg == "wold":
        assert np.array_equal(dflt.niter[:kk], one.niter[:kk])
    d = one.weights
    G = (one.T * d[:, None]).T @ one.T                               # the scores stay D-orthogonal (the rows ARE deflated, lazily)
    assert np.abs(G - np.diag(np.diag(G))).max() < 1e-9 * np.abs(np.diag(G)).max()
    with pytest.raises(J.JchError):                                  # outside the envelope of the postponed write-back: refused, loudly
        fn(X[:, :20], CO.fill_uniform(507, n, 17), nlv=2, ctx=ctx, one_pass=True)   # q = 17


# ---------------------------------------------------------------------------------- the three routes of the C entries (tests/host_routes.py)
@pytest.mark.parametrize("entry", sorted(__import__("host_routes").ROUTES["lwplsr"]))
def test_host_arrays_padded_and_unpadded_give_the_bits_of_the_device_route(entry):
    """Device buffers, host arrays with ld == rows and with ld = rows + 3 between NaN guards: equal bytes, NaN padding kept, inputs unchanged."""
    import host_routes as HR
    HR.three_routes(HR.ROUTES["lwplsr"][entry])
