"""jch_knn_gda, the score outputs of the local fit and lwplsrda / lwplslda / lwplsqda / lwplsr_s / lwplsrda_s on the GPU, against the longdouble
restatements of tests/test_lwplsda_static.py inside the bounds derived there (checked there between the float64 and the longdouble restatement
first).  Every comparison prints its largest measured / allowed ratio before it asserts."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import plsr_oracle as O  # noqa: E402
from test_lwplsda_static import (reference_with_weights, ABSENT, E2E_SEP, E2E_SHAPE, F64, LD, NLVDIS, PSPACE, SCORE_SHAPES, e2e_case, gda_reference, gen_classes, lists_of, np_plskern_local,  # noqa: E402
                                 prim_case, ratio, undecided)

H, TOL = 2.0, 1e-4


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


def host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def dev(a):
    """A column-major device copy of a host matrix."""
    a = np.asarray(a)
    t = torch.empty((a.shape[1], a.shape[0]), dtype=torch.float64, device="cuda:0").t()
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def put(a, where):
    return dev(a) if where == "device" else np.asfortranarray(a)


# ---------------------------------------------------------------------------------- the primitive
PRIM_SHAPES = [(5, 37, 1, 2), (9, 64, 3, 3), (7, 100, 7, 5), (4, 257, 12, 9), (3, 300, 48, 3), (2, 400, 60, 3)]


def check_prim(J, ctx, shape, kind, prior, where):
    m, k, a, nlev = shape
    case = prim_case(shape)
    T = np.stack([c[0] for c in case]); tq = np.stack([c[1] for c in case]); cls = np.stack([c[2] for c in case])
    args = (T, tq, cls) if where == "host" else tuple(torch.as_tensor(x, device="cuda:0") for x in (T, tq, cls))
    post, code, info = (host(x) for x in J.knn_gda(*args, nlev, kind=kind, prior=prior, nlv=range(1, a + 1), ctx=ctx))
    assert post.shape == (m, a, nlev) and code.shape == info.shape == (m, a)
    worst = 0.0
    for i, (Ti, tqi, ci, _) in enumerate(case):
        ref = gda_reference(Ti, tqi, ci, nlev, kind, prior, 1, a)
        rinfo = ref["info"].copy()
        rpost = np.asarray(ref["post"], dtype=F64)
        if "lev" in ref:                                          # every density of the local levels underflows in float64: 0 / 0, a NaN posterior
            d64 = np.asarray(ref["dens"], dtype=F64)[:, ref["lev"]]
            rpost[(rinfo == 0) & (d64 == 0).all(axis=1)] = np.nan
        assert np.array_equal(info[i], rinfo), (shape, kind, i, info[i], rinfo)
        assert np.array_equal(np.isnan(post[i]), np.isnan(rpost)), (shape, kind, i)
        fit = (rinfo == 0) & np.isfinite(rpost).all(axis=1)
        if fit.any():
            worst = max(worst, ratio(post[i][fit], ref["post"][fit], ref["post_bound"][fit]))
            s = np.sort(rpost[fit], axis=1)
            decided = (s[:, -1] - s[:, -2]) > 100 * np.asarray(ref["post_bound"][fit], dtype=F64).max(axis=1)
            assert np.array_equal(code[i][fit][decided], ref["code"][fit][decided]), (shape, kind, i)
        other = ~fit
        want = np.where(rinfo == 2, -1, ref["code"])
        nanrow = (rinfo != 2) & np.isnan(rpost).any(axis=1)
        want = np.where(nanrow, np.unique(ci)[0], want)           # all densities 0 / a NaN query: the first local level
        assert np.array_equal(code[i][other], want[other]), (shape, kind, i, code[i], want)
        if rinfo[0] == 1:
            assert np.array_equal(post[i], rpost)
    print(f"jch_knn_gda {shape} {kind} {prior} [{where}]: posterior {worst:.3f} of the bound")
    assert worst <= 1.0
    return post, code, info


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("kind", ["lda", "qda"])
@pytest.mark.parametrize("shape", PRIM_SHAPES)
def test_knn_gda_against_longdouble(J, ctx, shape, kind, where):
    """Absent classes and a class of one row (query 0), a class of two rows (query 1: qda gives info 2 from a = 2 on, a = 1 valid), a unanimous list
    (query 2), a NaN in one query's tq (query 3: only that query NaN), a far query (query 4: densities 0); (2, 400, 60, 3) runs in the workspace."""
    if shape == (2, 400, 60, 3):
        assert J.knn_gda_lds_bytes(400, 60, 3) > 150 * 1024
    post, code, info = check_prim(J, ctx, shape, kind, "prop" if shape[2] % 2 else "unif", where)
    if kind == "qda" and shape[2] >= 3:
        assert list(info[1][:3]) == [0, 2, 2]
    if shape[0] > 3:
        assert np.isnan(post[3]).all() and not np.isnan(post[[0, 1, 2]][info[[0, 1, 2]] != 2]).any()


def test_knn_gda_workspace_path_equals_lds_path(J, ctx, monkeypatch):
    shape = (7, 100, 7, 5)
    a = check_prim(J, ctx, shape, "qda", "prop", "host")
    monkeypatch.setenv("JCH_GDA_WS", "1")
    b = check_prim(J, ctx, shape, "qda", "prop", "host")
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


# ---------------------------------------------------------------------------------- score outputs of the local fit
def _engine_call(J, ctx, X, y, Xq, nlev, k, lo, hi, scal, kind=0, prior=0, want_scores=True, Yd=None):
    """jch_lwplsda_predict_prepared through the C ABI on a handle built as the mirror builds it (nlvdis = 0, eucl): dict of the host results.
    Yd: the handle's n x nlev response table when it is not the dummy table of y."""
    from jchemo_hip import _lib
    from jchemo_hip.plsr import Lwplsr, _addr_ld, _lwplsr_prepared
    if Yd is None:
        Yd = np.asfortranarray((y[:, None] == np.arange(nlev)[None, :]).astype(F64))
    eng = Lwplsr(X, Yd, None, "eucl", H, k, hi, TOL, scal, False)
    hd = _lwplsr_prepared(eng, ctx, False, nlev)
    m, le = Xq.shape[0], hi - lo + 1
    out = dict(code=np.empty((m, le), dtype=np.int32), post=np.empty((m, le, nlev)), info=np.empty((m, le), dtype=np.int32), tloc=np.empty((m, k, hi)),
               tq=np.empty((m, hi)), ind=np.empty((m, k), dtype=np.int32), dist=np.empty((m, k)), w=np.empty((m, k)), eng=eng, hd=hd)
    xqa, ldxq = _addr_ld(Xq)
    cls = np.ascontiguousarray(y, dtype=np.int32)
    zqa, ldzq = (None, 0) if hd["device_map"] else _addr_ld(hd["qmap"](Xq))   # (under scal the handle maps the queries into the scaled search space itself)
    st = _lib.load().jch_lwplsda_predict_prepared(ctx._h, hd["handle"], cls.ctypes.data, nlev, kind, prior, 0, zqa, ldzq, xqa, m, ldxq, k, H, TOL, int(scal),
                                                  lo, hi, out["code"].ctypes.data, out["post"].ctypes.data, out["info"].ctypes.data,
                                                  out["tloc"].ctypes.data if want_scores else None, out["tq"].ctypes.data if want_scores else None,
                                                  out["ind"].ctypes.data, out["dist"].ctypes.data, out["w"].ctypes.data)
    out["status"] = st
    return out


GENERIC_SHAPE = (120, 2100, 2, 20, 2, 4)                           # p > 2048: the per-query generic route; so is SCORE_SHAPES[3] (nine classes at p = 1100: beyond the LDS)


@pytest.mark.parametrize("shape,scal", [(s, False) for s in SCORE_SHAPES] + [(SCORE_SHAPES[1], True), (GENERIC_SHAPE, False), (GENERIC_SHAPE, True)])
def test_local_scores_against_the_float64_restatement(J, ctx, shape, scal, monkeypatch):
    """tloc_out / tq_out against the weighted `plskern` on the gathered rows: sign-aligned relative Frobenius error per query <= 1e-7 (the project's
    tolerance for the local fits against the oracle); and `pred` of jch_lwplsr_predict_prepared through the same kernel with the new pointers null
    equals, byte for byte, the dummy predictions delivered with them set."""
    n, p, nlev, k, nlv, m = shape
    batched = shape != GENERIC_SHAPE and PSPACE[SCORE_SHAPES.index(shape)]
    assert (J.locw_pspace_lds_bytes(k, p, nlev) <= 150 * 1024 and p <= 2048) == batched     # the route this case takes (the library decides by the same formula)
    X, y, Xq, _ = gen_classes(n, p, nlev, m)
    r = _engine_call(J, ctx, X, y, Xq, nlev, k, 0, nlv, scal)
    ctx.check(r["status"])
    xs = X.std(axis=0) if scal else 1.0                          # src/lwplsr.jl:141-145: under scal the search runs on the columns divided by colstd(X)
    ind, _, _ = lists_of(X / xs, y, Xq / xs, 0, "eucl", k, nlev=nlev)
    assert np.array_equal(r["ind"], ind)
    Yd = (y[:, None] == np.arange(nlev)[None, :]).astype(F64)
    worst = 0.0
    for i in range(m):
        if r["info"][i, 0] == 1:
            continue
        cn = y[r["ind"][i]]
        lev = np.unique(cn)
        T, tq, pred = np_plskern_local(X[r["ind"][i]], Yd[r["ind"][i]][:, lev], r["w"][i], Xq[i], nlv, scal, F64)
        s = np.sign((T * r["tloc"][i]).sum(axis=0))
        e1 = np.linalg.norm(T - r["tloc"][i] * s) / np.linalg.norm(T)
        e2 = np.linalg.norm(tq - r["tq"][i] * s) / np.linalg.norm(tq)
        e3 = np.linalg.norm(pred[:, :] - r["post"][i][:, lev]) / np.linalg.norm(pred)
        worst = max(worst, e1, e2, e3)
    print(f"local scores {shape} scal={scal}: largest sign-aligned relative Frobenius error {worst:.3e}")
    assert worst <= 1e-7
    r2 = _engine_call(J, ctx, X, y, Xq, nlev, k, 0, nlv, scal, want_scores=False)
    assert np.array_equal(r2["post"], r["post"], equal_nan=True) and np.array_equal(r2["code"], r["code"])
    if not batched:
        return
    # the same kernel without the score outputs (the k-space kernel switched off: it has none)
    from jchemo_hip import _lib
    from jchemo_hip.plsr import _addr_ld
    monkeypatch.setenv("JCH_LOCW_KSPACE", "0")
    pred = np.empty((m, nlv + 1, nlev))
    xqa, ldxq = _addr_ld(Xq)
    zqa, ldzq = (None, 0) if r["hd"]["device_map"] else (xqa, ldxq)
    ctx.check(_lib.load().jch_lwplsr_predict_prepared(ctx._h, r["hd"]["handle"], 0, zqa, ldzq, xqa, m, ldxq, k, H, TOL, int(scal), 0, nlv, pred.ctypes.data, None, None, None))
    fitted = r["info"][:, 0] != 1
    if not scal:                                                  # (under scal the regression kernel divides an absent class's column by its sd 0)
        assert np.array_equal(pred[fitted], r["post"][fitted])


def test_generic_route_equals_the_batched_kernel(J, ctx, monkeypatch):
    """The per-query route forced on a shape the batched kernel takes (JCH_LOCW_GENERIC=1): same labels and flags, posteriors and scores to 1e-9."""
    n, p, nlev, k, nlv, m = SCORE_SHAPES[0]
    X, y, Xq, _ = gen_classes(n, p, nlev, m)
    a = _engine_call(J, ctx, X, y, Xq, nlev, k, 1, nlv, True, kind=2)
    monkeypatch.setenv("JCH_LOCW_GENERIC", "1")
    b = _engine_call(J, ctx, X, y, Xq, nlev, k, 1, nlv, True, kind=2)
    ctx.check(a["status"]); ctx.check(b["status"])
    assert np.array_equal(a["info"], b["info"]) and np.array_equal(a["code"], b["code"]) and np.array_equal(a["ind"], b["ind"])
    s_ = np.sign((a["tloc"] * b["tloc"]).sum(axis=1, keepdims=True))
    assert np.max(np.abs(a["tloc"] - b["tloc"] * s_)) <= 1e-9 * np.max(np.abs(a["tloc"]))
    assert np.nanmax(np.abs(a["post"] - b["post"])) <= 1e-9


# ---------------------------------------------------------------------------------- the label rule
def julia_argmax_present(v, present):
    """Julia's `argmax` of v over the levels that are present, in code order: the first NaN when there is one, else the first maximum."""
    lev = np.flatnonzero(present)
    nan = np.isnan(v[lev])
    return int(lev[np.flatnonzero(nan)[0]] if nan.any() else lev[np.argmax(v[lev])])


def test_label_rule_of_the_rda_route(J, ctx):
    """k_rda_finish on m = 4 queries, nlev = 3, k = 6, the models 0 .. 2.  Every query owns one far cluster of six training rows, so its neighbourhood
    and its class codes are hand-made; the handle's response table is hand-made too (the label rule reads the local predictions whatever they are):
      0. the columns of the two present classes 1 and 2 are equal: a tie in every model, the lower code wins;
      1. a NaN in the column of the last present class (2, beside 0): model 0 — the weighted means — is NaN there only and 2 wins;
      2. a NaN in the column of the first present class;
      3. the absent class 2 holds by far the largest predictions: it is written out and never wins.
    Labels and flags against `julia_argmax_present` on the posteriors the call returned, for equality."""
    nlev, k, m, p, hi = 3, 6, 4, 4, 2
    rng = np.random.default_rng(61)
    cen = 100.0 * np.eye(m, p)
    X = np.asfortranarray(np.repeat(cen, k, axis=0) + rng.standard_normal((m * k, p)))
    Xq = np.asfortranarray(cen + 0.1 * rng.standard_normal((m, p)))
    y = np.array([1, 1, 1, 2, 2, 2] + [0, 0, 0, 2, 2, 2] + [0, 0, 0, 2, 2, 2] + [0, 0, 0, 1, 1, 1], dtype=np.int32)
    Yd = (y[:, None] == np.arange(nlev)[None, :]).astype(F64)
    Yd[0:6, 1] = Yd[0:6, 2] = rng.standard_normal(6)
    Yd[10, 2] = np.nan
    Yd[13, 0] = np.nan
    Yd[18:24, 2] = 10.0 + rng.standard_normal(6)
    r = _engine_call(J, ctx, X, y, Xq, nlev, k, 0, hi, False, kind=0, Yd=np.asfortranarray(Yd))
    ctx.check(r["status"])
    assert np.array_equal(np.sort(r["ind"], axis=1), np.arange(m * k).reshape(m, k))
    post, code, info = r["post"], r["code"], r["info"]
    present = np.stack([np.bincount(y[r["ind"][i]], minlength=nlev) > 0 for i in range(m)])
    # the four cases are what they claim to be
    assert np.array_equal(post[0, :, 1], post[0, :, 2]) and np.isfinite(post[0]).all()
    assert np.isnan(post[1, 0, 2]) and np.isfinite(post[1, 0, :2]).all()
    assert np.isnan(post[2, 0, 0]) and np.isfinite(post[2, 0, 1:]).all()
    assert not present[3, 2] and post[3, 0, 2] > 5.0 > post[3, 0, :2].max()
    want = np.array([[julia_argmax_present(post[i, t], present[i]) for t in range(hi + 1)] for i in range(m)])
    winfo = np.array([[0 if np.isfinite(post[i, t][present[i]]).all() else 3 for t in range(hi + 1)] for i in range(m)])
    print("rda labels", code.tolist(), "flags", info.tolist())
    assert np.array_equal(code, want) and np.array_equal(info, winfo)
    assert code[0].tolist() == [1, 1, 1] and code[1, 0] == 2 and code[2, 0] == 0 and (code[3] != 2).all()


@pytest.mark.parametrize("kind", ["lda", "qda"])
def test_label_rule_of_knn_gda(J, ctx, kind):
    """Step 4 of k_knn_gda on m = 4 queries, nlev = 3, k = 6, a = 2.  A posterior is a density over the sum of the densities, so a NaN in one class is a
    NaN in all of them; the cases this kernel can reach:
      0. the rows of class 2 mirror those of class 1 about the query (class 0 absent): equal densities bit for bit, a tie, the lower code wins;
      1. a query so far away that every density is 0: 0 / 0, NaN in the first and in the last present class, the first one wins;
      2. a NaN in the query's scores: NaN densities, the first present class (1) wins;
      3. class 2 absent, the query inside class 1: its posterior is 0 and it never wins.
    Labels against `julia_argmax_present` on the posteriors the call returned, flags against the longdouble restatement, for equality."""
    nlev, k, a, m = 3, 6, 2, 4
    rng = np.random.default_rng(62)
    A = rng.standard_normal((3, a)) + np.array([1.5, 0.5])
    two = np.vstack([rng.standard_normal((3, a)), rng.standard_normal((3, a)) + 3.0])
    T = np.stack([np.vstack([A, -A]), two, two, two])
    tq = np.array([[0.0, 0.0], [1e6, -1e6], [np.nan, 0.3], [3.1, 2.9]])
    cls = np.array([[1, 1, 1, 2, 2, 2], [0, 0, 0, 2, 2, 2], [1, 1, 1, 2, 2, 2], [0, 0, 0, 1, 1, 1]], dtype=np.int32)
    post, code, info = (host(x) for x in J.knn_gda(T, tq, cls, nlev, kind=kind, prior="unif", nlv=range(1, a + 1), ctx=ctx))
    present = np.stack([np.bincount(c, minlength=nlev) > 0 for c in cls])
    assert np.array_equal(post[0, :, 1], post[0, :, 2]) and (post[0, :, 1] == 0.5).all()
    assert np.isnan(post[1][:, present[1]]).all() and np.isnan(post[2][:, present[2]]).all()
    assert (post[3, :, 2] == 0).all() and np.isfinite(post[3]).all()
    want = np.array([[julia_argmax_present(post[i, t], present[i]) for t in range(a)] for i in range(m)])
    winfo = np.stack([gda_reference(T[i], tq[i], cls[i], nlev, kind, "unif", 1, a)["info"] for i in range(m)])
    print(f"{kind} labels", code.tolist(), "flags", info.tolist())
    assert np.array_equal(code, want) and np.array_equal(info, winfo)
    assert code[0].tolist() == [1, 1] and code[1].tolist() == [0, 0] and code[2].tolist() == [1, 1] and code[3].tolist() == [1, 1]


# ---------------------------------------------------------------------------------- end to end
def _fit(J, kind, X, y, metric, prior, nlv, ctx, **kw):
    f = {"rda": J.lwplsrda, "lda": J.lwplslda, "qda": J.lwplsqda}[kind]
    extra = {} if kind == "rda" else {"prior": prior}
    return f(X, y, nlvdis=NLVDIS, metric=metric, h=H, k=E2E_SHAPE[3], nlv=nlv, tol=TOL, ctx=ctx, **extra, **kw)


def _predict(J, kind):
    return {"rda": J.lwplsrda_predict, "lda": J.lwplslda_predict, "qda": J.lwplsqda_predict}[kind]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("metric", ["eucl", "mahal"])
@pytest.mark.parametrize("kind,prior", [("rda", "unif"), ("lda", "unif"), ("lda", "prop"), ("qda", "unif"), ("qda", "prop")])
def test_models_end_to_end(J, ctx, kind, metric, prior, where):
    c = e2e_case(kind, metric, prior)
    Xi, Qi = put(c["X"], where), put(c["Xq"], where)
    fm = _fit(J, kind, Xi, c["y"], metric, prior, c["hi"], ctx)
    res = _predict(J, kind)(fm, Qi, nlv=range(c["lo"], c["hi"] + 1), ctx=ctx)
    assert np.array_equal(res.listnn, c["ind"])
    post = np.stack(res.posterior, axis=1); code = np.stack([p_[:, 0] for p_ in res.pred], axis=1)
    assert np.array_equal(res.info, c["info"])
    und = undecided(c)
    # the longdouble restatement on the lists the device found (equal to the oracle's) and the weights it handed to its local fits
    rpost, rcode, rinfo = reference_with_weights(c, res.listw)
    r = ratio(post, rpost, np.asarray(c["tol"], dtype=LD))
    r0 = ratio(post, c["post"], np.asarray(c["tol"], dtype=LD))
    dw = float(np.max(np.abs(res.listw - c["w"]) / c["w"]))
    print(f"{kind} {metric} {prior} [{where}]: posterior {r:.3f} of the tolerance (largest {c['tol'].max():.3e}, gap {c['gap']:.3e}); with the oracle's weights "
          f"instead (largest relative difference of a weight {dw:.2e}): {r0:.3f}; undecided {int(und.sum())} of {und.size}")
    assert np.array_equal(rinfo, c["info"]) and np.array_equal(rcode[~und], c["code"][~und])
    assert r <= 1.0
    assert und.mean() <= 0.05 and (c["info"] != 0).mean() <= 0.05
    assert np.array_equal(code[~und], c["code"][~und])
    one = _predict(J, kind)(fm, Qi, nlv=c["hi"], ctx=ctx)         # nlv as an int: the last model of the range, same bits
    assert np.array_equal(one.posterior, res.posterior[-1]) and np.array_equal(one.pred, res.pred[-1]) and one.info.shape == (Qi.shape[0],)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("scal", [False, True])
@pytest.mark.parametrize("kind", ["rda", "lda", "qda"])
def test_models_with_a_class_absent_from_every_neighbourhood(J, ctx, kind, scal, where):
    """Four classes, one of them (code 1) three far rows: every neighbourhood is non-unanimous and lacks it.  Its dummy column is a zero column in
    the local fit — sd 0 under scal —, its posterior is exactly 0 and it never wins; everything else against the local-dummy restatement."""
    c = e2e_case(kind, "eucl", "unif", absent=True, scal=scal)
    Xi, Qi = put(c["X"], where), put(c["Xq"], where)
    f = {"rda": J.lwplsrda, "lda": J.lwplslda, "qda": J.lwplsqda}[kind]
    fm = f(Xi, c["y"], nlvdis=0, metric="eucl", h=H, k=E2E_SHAPE[3], nlv=c["hi"], tol=TOL, scal=scal, ctx=ctx)
    res = _predict(J, kind)(fm, Qi, nlv=range(c["lo"], c["hi"] + 1), ctx=ctx)
    assert np.array_equal(res.listnn, c["ind"]) and not (c["y"][res.listnn] == ABSENT).any()
    post = np.stack(res.posterior, axis=1); code = np.stack([p_[:, 0] for p_ in res.pred], axis=1)
    assert np.array_equal(res.info, c["info"]) and (res.info == 0).all()
    assert (post[:, :, ABSENT] == 0).all() and not (code == ABSENT).any() and np.isfinite(post).all()
    und = undecided(c)
    r = ratio(post, c["post"], np.asarray(c["tol"], dtype=LD))
    print(f"absent class, {kind} scal={scal} [{where}]: posterior {r:.3f} of the tolerance (largest {c['tol'].max():.3e}, gap {c['gap']:.3e}); undecided {int(und.sum())} of {und.size}")
    assert r <= 1.0 and und.mean() <= 0.05
    assert np.array_equal(code[~und], c["code"][~und])


@pytest.mark.parametrize("kind", ["rda", "lda", "qda"])
def test_nan_query_stays_in_its_query(J, ctx, kind):
    """A NaN in one query row: that query gets info 3, a NaN posterior and the first local level of its list (the reference's argmax over NaN) for every
    nlv >= 1, with no warning; the other queries' results do not change by a bit."""
    c = e2e_case(kind, "eucl", "unif")
    fm = _fit(J, kind, c["X"], c["y"], "eucl", "unif", c["hi"], ctx)
    clean = _predict(J, kind)(fm, c["Xq"], nlv=range(1, c["hi"] + 1), ctx=ctx)
    Xq = c["Xq"].copy(order="F"); Xq[1, 3] = np.nan
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = _predict(J, kind)(fm, Xq, nlv=range(1, c["hi"] + 1), ctx=ctx)
    assert not [w_ for w_ in rec if issubclass(w_.category, RuntimeWarning)]
    others = np.arange(Xq.shape[0]) != 1
    assert (res.info[1] == 3).all() and np.array_equal(res.info[others], clean.info[others])
    first = np.unique(c["y"][res.listnn[1]])[0]
    for a in range(c["hi"]):
        assert np.isnan(res.posterior[a][1]).all() and res.pred[a][1, 0] == first
        assert np.array_equal(res.posterior[a][others], clean.posterior[a][others]) and np.array_equal(res.pred[a][others], clean.pred[a][others])


def _clusters(nlev=3, per=40, p=12, seed=3):
    rng = np.random.default_rng(seed)
    cen = 50.0 * rng.standard_normal((nlev, p))
    y = np.repeat(np.arange(nlev), per).astype(np.int32)
    return np.asfortranarray(cen[y] + 0.01 * rng.standard_normal((nlev * per, p))), y, np.asfortranarray(cen + 0.01 * rng.standard_normal((nlev, p)))


@pytest.mark.parametrize("kind", ["rda", "lda", "qda"])
def test_unanimous_neighbourhoods(J, ctx, kind):
    X, y, Xq = _clusters()
    fm = {"rda": J.lwplsrda, "lda": J.lwplslda, "qda": J.lwplsqda}[kind](X, y, nlvdis=0, metric="eucl", h=H, k=15, nlv=2, ctx=ctx)
    res = _predict(J, kind)(fm, Xq, nlv=range(1, 3), ctx=ctx)
    assert (res.info == 1).all()
    for a in range(2):
        assert np.array_equal(res.pred[a][:, 0], np.arange(3)) and np.array_equal(res.posterior[a], np.eye(3))


def test_not_positive_definite_falls_back_to_the_vote_with_one_warning(J, ctx):
    """A class of two rows in every neighbourhood: its qda covariance has rank 1, so a = 1 is fitted and pivot 2 fails; from a = 2 on the label is
    the weighted vote and the posterior NaN, with one warning for the call."""
    rng = np.random.default_rng(5)
    X = np.asfortranarray(np.vstack([rng.standard_normal((60, 10)), 0.1 * rng.standard_normal((2, 10))]))
    y = np.array([0] * 60 + [1] * 2, dtype=np.int32)
    Xq = np.asfortranarray(0.05 * rng.standard_normal((3, 10)))
    fm = J.lwplsqda(X, y, nlvdis=0, metric="eucl", h=H, k=40, nlv=3, ctx=ctx)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        res = J.lwplsqda_predict(fm, Xq, nlv=range(1, 4), ctx=ctx)
    assert len([w_ for w_ in rec if issubclass(w_.category, RuntimeWarning)]) == 1
    assert ((y[res.listnn] == 1).sum(axis=1) == 2).all()
    assert (res.info[:, 0] == 0).all() and (res.info[:, 1:] == 2).all()
    assert np.isfinite(res.posterior[0]).all() and np.isnan(np.stack(res.posterior[1:])).all()
    vote = host(J.knn_vote(y, 2, res.listnn, res.listw, ctx=ctx))
    for a in (1, 2):
        assert np.array_equal(res.pred[a][:, 0], vote)


def test_nlv_zero_raises_for_the_gaussian_models(J, ctx):
    c = e2e_case("lda", "eucl", "unif")
    for kind in ("lda", "qda"):
        fm = _fit(J, kind, c["X"], c["y"], "eucl", "unif", 2, ctx)
        with pytest.raises(ValueError):
            _predict(J, kind)(fm, c["Xq"], nlv=range(0, 3), ctx=ctx)
    fm = _fit(J, "rda", c["X"], c["y"], "eucl", "unif", 2, ctx)
    assert len(J.lwplsrda_predict(fm, c["Xq"], nlv=range(0, 3), ctx=ctx).pred) == 3


@pytest.mark.parametrize("where", ["host", "device"])
def test_lwplsr_s_equals_lwplsr_on_the_score_table(J, ctx, where):
    n, p, nlev, k, nlv, m = E2E_SHAPE
    X, y, Xq, _ = gen_classes(n, p, nlev, m, sep=E2E_SEP)
    Y = np.asfortranarray(X[:, :2] @ np.array([[1.0, 0.5], [-0.5, 2.0]]) + 0.1 * X[:, 2:4])
    Xi, Yi, Qi = put(X, where), put(Y, where), put(Xq, where)
    fm = J.lwplsr_s(Xi, Yi, nlv0=6, metric="mahal", h=H, k=k, nlv=9, ctx=ctx)
    assert fm.nlv == 6 and tuple(fm.T.shape) == (n, 6)
    res = J.lwplsr_s_predict(fm, Qi, nlv=range(0, 4), ctx=ctx)
    by_hand = J.lwplsr_predict(J.lwplsr(fm.T, Yi, nlvdis=0, metric="mahal", h=H, k=k, nlv=6, ctx=ctx), J.transform(fm.fm, Qi, ctx=ctx), nlv=range(0, 4), ctx=ctx)
    assert np.array_equal(res.listnn, by_hand.listnn)
    for a, b in zip(res.pred, by_hand.pred):
        assert np.array_equal(host(a), host(b))
    ref = O.lwplsr_predict(O.lwplsr(host(fm.T), Y, nlvdis=0, metric="mahal", h=H, k=k, nlv=6), host(J.transform(fm.fm, Qi, ctx=ctx)), nlv=range(0, 4))
    for a in range(4):
        assert O.rel_fro(ref["pred"][:, :, a], host(res.pred[a])) <= 1e-7


@pytest.mark.parametrize("reduc", ["pca", "pls", "dkpls"])
def test_lwplsrda_s(J, ctx, reduc):
    n, p, nlev, k, nlv, m = E2E_SHAPE
    X, y, Xq, yq = gen_classes(n, p, nlev, m, sep=E2E_SEP)
    fm = J.lwplsrda_s(X, y, nlv0=5, reduc=reduc, h=H, k=k, nlv=3, gamma=0.01, ctx=ctx)
    res = J.lwplsrda_s_predict(fm, Xq, nlv=range(1, 4), ctx=ctx)
    T, Tq = host(fm.T), host(J.lwplsda._transform(fm.fm, Xq, ctx))
    ind, d, w = lists_of(T, y, Tq, 0, "eucl", k, nlev=nlev)
    assert np.array_equal(res.listnn, ind)
    from test_lwplsda_static import np_locw_da
    ref = np_locw_da(T, y, Tq, ind, w, nlev, "rda", "unif", 1, 3, False, F64)
    post = np.stack(res.posterior, axis=1)
    err = max(float(np.max(np.abs(post[i] - r["post"]))) for i, r in enumerate(ref))
    print(f"lwplsrda_s {reduc}: largest posterior difference from the float64 restatement {err:.3e}")
    assert err <= 1e-7
    code = np.stack([p_[:, 0] for p_ in res.pred], axis=1)
    for i, r in enumerate(ref):
        s = np.sort(r["post"], axis=1)
        dec = (s[:, -1] - s[:, -2]) > 1e-6
        assert np.array_equal(code[i][dec], r["code"][dec])


# ---------------------------------------------------------------------------------- on a used ctx
@pytest.fixture(scope="module")
def used_ctx_models(J):
    other = J.Context(0)
    c = e2e_case("lda", "eucl", "unif")
    out = {}
    case = prim_case((9, 64, 3, 3))
    T = np.stack([x[0] for x in case]); tq = np.stack([x[1] for x in case]); cls = np.stack([x[2] for x in case])
    Y = np.asfortranarray(c["X"][:, :2].copy())
    for where in ("host", "device"):
        Xi, Qi, Yi = put(c["X"], where), put(c["Xq"], where), put(Y, where)
        pa = (T, tq, cls) if where == "host" else tuple(torch.as_tensor(x, device="cuda:0") for x in (T, tq, cls))
        models = {
            "knn_gda": (lambda cc, pa=pa: J.knn_gda(*pa, 3, kind="qda", nlv=range(1, 4), ctx=cc)[0]),
            "lwplsrda": (lambda cc, f=_fit(J, "rda", Xi, c["y"], "eucl", "unif", 3, other), Qi=Qi: J.lwplsrda_predict(f, Qi, ctx=cc).posterior),
            "lwplslda": (lambda cc, f=_fit(J, "lda", Xi, c["y"], "mahal", "unif", 3, other), Qi=Qi: J.lwplslda_predict(f, Qi, ctx=cc).posterior),
            "lwplsqda": (lambda cc, f=_fit(J, "qda", Xi, c["y"], "eucl", "prop", 3, other), Qi=Qi: J.lwplsqda_predict(f, Qi, ctx=cc).posterior),
            "lwplsr_s": (lambda cc, f=J.lwplsr_s(Xi, Yi, nlv0=4, h=H, k=40, nlv=2, ctx=other), Qi=Qi: J.lwplsr_s_predict(f, Qi, ctx=cc).pred),
            "lwplsrda_s": (lambda cc, f=J.lwplsrda_s(Xi, c["y"], nlv0=4, reduc="pca", h=H, k=40, nlv=2, ctx=other), Qi=Qi: J.lwplsrda_s_predict(f, Qi, ctx=cc).posterior),
        }
        for name, call in models.items():
            out[name, where] = (call, host(call(other)))
    yield out
    other.close()


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", ["knn_gda", "lwplsrda", "lwplslda", "lwplsqda", "lwplsr_s", "lwplsrda_s"])
def test_on_a_used_ctx_behind_a_fit_that_promised_reuse_x(name, where, used_ctx_models):
    """plskern(X) / the entry / plskern(X, reuse_x=True) on one ctx (tests/test_gpu_used_ctx.py, Part B): the entry's results equal those on a fresh
    ctx bit for bit, and the third fit equals the same fit on a fresh ctx."""
    from test_gpu_used_ctx import reuse_sequence
    call, want = used_ctx_models[name, where]

    def intervener(c, Xi, state):
        if state != "before":
            assert np.array_equal(host(call(c)), want, equal_nan=True)
    taken = reuse_sequence(where, intervener)
    print(f"{name} [{where}]: the third fit took the row-major copy {taken} time(s)")
