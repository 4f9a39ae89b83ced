"""Permutation importance and interval selection on the GPU (jch_perm_fill, jch_perm_score_sums and the Python mirror) against the
restatements and the bound of tests/viperm_restate.py.

  * jch_perm_fill equals the numpy restatement of the documented generator bit for bit.
  * jch_perm_score_sums stays within the derived per-sum bound of the longdouble restatement, for every shape at which the kernel takes another
    path (m around a wave and around the row slice, q beyond a register group, p beyond the 8 column queues), with the rows that are not listed
    and the padding behind ldx filled with NaN; a host and a device X, an X one double off the allocation, a padded X, an explicit and the
    generated permutation give the same bits.  Every case prints its largest error / bound ratio.
  * `viperm` and `isel` against the literal restatements of src/viperm.jl and src/isel.jl at 1e-9 x the unshuffled score, the project's figure
    for literal restatements (both sides run the same fits; what differs is the weight-0 fit against the fit on gathered rows and the sums
    against the scores of explicit predictions)."""
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

import viperm_restate as V  # noqa: E402
from jchemo_hip.viperm import PERM_QGROUP, PERM_SLICE_ROWS, _splits  # noqa: E402

S = PERM_SLICE_ROWS
M_CASES = (1, 2, 63, 64, 65, S - 1, S, S + 1)
PQ_CASES = ((1, 1), (3, 3), (130, PERM_QGROUP + 1))
# (where, rows, layout of X, permutation)
VARIANTS = (("device", "asc", "plain", "generated"), ("host", "asc", "plain", "explicit"), ("device", "none", "padded", "explicit"),
            ("host", "none", "offset", "generated"), ("device", "shuffled", "offset", "generated"), ("host", "shuffled", "padded", "explicit"))
NAMES = ("ssr", "msep", "rmsep", "bias", "r2", "cor2")


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


def _seed(*parts):
    return int(np.random.SeedSequence([int(v) for v in parts]).generate_state(1)[0])


def _case(m, p, q, seed=0):
    """X (n x p), Pred, Y (n x q), B, and the three row lists; n = m + 37."""
    rng = np.random.default_rng(_seed(m, p, q, seed))
    n = m + 37
    X = rng.normal(size=(n, p)) + 2.0
    B = rng.normal(size=(p, q))
    Y = 1.0 + X @ B + 0.1 * rng.normal(size=(n, q))
    Pred = 1.0 + X @ B
    asc = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64)
    rows = dict(none=None, asc=asc, shuffled=rng.permutation(asc))
    return X, Pred, Y, B, rows


def _x_layout(X, layout):
    """(host view, its flat buffer, ld, offset in doubles) of a column-major copy of X: plain; with 5 NaN rows of padding behind every column;
    one double behind the start of its buffer."""
    n, p = X.shape
    ld, off = (n + 5, 0) if layout == "padded" else (n, 1) if layout == "offset" else (n, 0)
    flat = np.full(ld * p + off, np.nan)
    view = np.ndarray((n, p), dtype=np.float64, buffer=flat, offset=8 * off, strides=(8, 8 * ld))
    view[:] = X
    return view, flat, ld, off


def _dev(a):
    """A column-major device copy of a host matrix."""
    t = torch.empty((a.shape[1], a.shape[0]), dtype=torch.float64, device="cuda:0").t()
    t.copy_(torch.as_tensor(np.ascontiguousarray(a)))
    return t


def _nan_unlisted(r, n, *arrays):
    keep = np.zeros(n, dtype=bool)
    keep[r] = True
    out = []
    for a in arrays:
        a = np.array(a, order="F", copy=True)
        a[~keep] = np.nan
        out.append(a)
    return out


def _run(J, ctx, X, Pred, Y, B, rows, perm, seed, where, layout="plain", m=None):
    r = np.arange(m) if rows is None else rows
    Xn, Pn, Yn = _nan_unlisted(r, X.shape[0], X, Pred, Y)           # rows that are not listed are never read
    Xv, flat, ld, off = _x_layout(Xn, layout)
    if where == "device":
        Xv = torch.as_strided(torch.as_tensor(flat).to("cuda:0"), Xv.shape, (1, ld), off)
        Pn, Yn = _dev(Pn), _dev(Yn)
    return J.perm_score_sums(Xv, Pn, Yn, B, rows=rows, m=m if rows is None else None, perm=perm, seed=seed, ctx=ctx)


# ---------------------------------------------------------------------------------------------------- jch_perm_fill
@pytest.mark.parametrize("m", [mm for mm in V.M_LIST if mm <= 1000] + [2 ** 16 + 1])
def test_perm_fill_equals_the_restated_generator(J, ctx, m):
    seed = _seed(m, 99)
    want = V.perm_matrix(seed, m, 3)
    host = J.perm_fill(m, 3, seed, ctx=ctx)
    dev = J.perm_fill(m, 3, seed, device="cuda:0", ctx=ctx)
    assert host.dtype == np.int32 and dev.dtype == torch.int32
    assert np.array_equal(host, want) and np.array_equal(dev.cpu().numpy(), want)


def test_perm_fill_takes_a_full_64_bit_seed(J, ctx):
    seed = 2 ** 64 - 3
    assert np.array_equal(J.perm_fill(1000, 2, seed, ctx=ctx), V.perm_matrix(seed, 1000, 2))


# ---------------------------------------------------------------------------------------------------- jch_perm_score_sums
@pytest.mark.parametrize("p,q", PQ_CASES)
@pytest.mark.parametrize("m", M_CASES)
def test_sums_within_the_bound_and_the_same_bits_on_every_route(J, ctx, m, p, q):
    X, Pred, Y, B, rows = _case(m, p, q)
    seed = _seed(m, p, q, 7)
    perm = V.perm_matrix(seed, m, p)
    got = {}
    for where, rk, layout, pk in VARIANTS:
        g = _run(J, ctx, X, Pred, Y, B, rows[rk], perm if pk == "explicit" else None, seed, where, layout, m=m)   # rows = None: the rows 0 .. m - 1
        assert g.shape == (p + 1, q, 6)
        if rk in got:
            assert np.array_equal(got[rk], g), (where, rk, layout, pk)      # host / device, layout, explicit / generated: the same bits
        else:
            got[rk] = g
            r = np.arange(m) if rk == "none" else rows[rk]
            ref = V.ref_perm_sums(X, r, Pred, Y, B, perm)
            bound = V.bound_perm_sums(X, r, Pred, Y, B, perm)
            err = np.abs(g.astype(V.LD) - ref).astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = float(np.nanmax(np.where(bound[..., :5] > 0, err[..., :5] / bound[..., :5], 0.0)))
            print(f"m={m} p={p} q={q} rows={rk}: max error / bound = {ratio:.3f}")
            assert np.all(err <= bound)
            assert np.array_equal(g[..., 5], np.full((p + 1, q), float(m)))
    again = _run(J, ctx, X, Pred, Y, B, rows["asc"], None, seed, "device")
    assert np.array_equal(again, got["asc"])                                # two runs: the same bits


def test_a_zero_row_of_B_gives_the_bits_of_the_unshuffled_row(J, ctx):
    X, Pred, Y, B, rows = _case(S + 9, 5, 3, seed=1)
    B[2] = 0.0
    X[:, 4] = 1.25                                                          # a constant column: the difference is exactly 0
    Pred = 1.0 + X @ B
    for where in ("host", "device"):
        g = _run(J, ctx, X, Pred, Y, B, rows["asc"], None, 11, where)
        assert np.array_equal(g[2], g[5]) and np.array_equal(g[4], g[5])
        assert not np.array_equal(g[0], g[5]) and not np.array_equal(g[1], g[5]) and not np.array_equal(g[3], g[5])


def test_a_nan_stays_in_its_column(J, ctx):
    X, Pred, Y, B, rows = _case(300, 6, 2, seed=2)
    clean = _run(J, ctx, X, Pred, Y, B, rows["asc"], None, 12, "device")
    X2 = X.copy()
    X2[rows["asc"][17], 3] = np.nan
    g = _run(J, ctx, X2, Pred, Y, B, rows["asc"], None, 12, "device")
    assert np.all(np.isnan(g[3, :, :3])) and np.array_equal(g[3, :, 3:], clean[3, :, 3:])
    for j in (0, 1, 2, 4, 5, 6):
        assert np.array_equal(g[j], clean[j])


@pytest.mark.parametrize("where", ["host", "device"])
def test_an_index_out_of_range_is_refused_and_never_followed(J, ctx, where):
    X, Pred, Y, B, rows = _case(100, 4, 2, seed=3)
    n = X.shape[0]
    bad_rows = rows["asc"].copy()
    bad_rows[40] = n
    bad_perm = V.perm_matrix(5, 100, 4)
    bad_perm[7, 2] = 100
    neg_rows = rows["asc"].copy()
    neg_rows[0] = -1
    for r, pm in ((bad_rows, None), (neg_rows, None), (rows["asc"], bad_perm)):
        Xv, Pv, Yv = (np.asfortranarray(a) for a in (X, Pred, Y))
        if where == "device":
            Xv, Pv, Yv = _dev(Xv), _dev(Pv), _dev(Yv)
        with pytest.raises(J.JchError) as ei:
            J.perm_score_sums(Xv, Pv, Yv, B, rows=r, perm=pm, seed=1, ctx=ctx)
        assert ei.value.code == J._lib.JCH_EINVAL
    good = _run(J, ctx, X, Pred, Y, B, rows["asc"], None, 1, where)          # the ctx is as usable as before
    assert np.all(np.isfinite(good))


def test_a_call_on_a_used_ctx_gives_the_bits_of_a_fresh_one(J):
    X, Pred, Y, B, rows = _case(S + 100, 20, 2, seed=4)
    fresh = J.Context(0)
    want = _run(J, fresh, X, Pred, Y, B, rows["asc"], None, 13, "device")
    fresh.close()
    used = J.Context(0)
    Xf, Yf = np.asfortranarray(X), np.asfortranarray(Y)
    J.covsel(Xf, Yf, nlv=3, ctx=used)
    J.plskern(Xf, Yf, nlv=3, ctx=used)
    J.perm_fill(5000, 7, 3, ctx=used)                                        # the same workspace buffer, other contents
    _run(J, used, X, Pred, Y, B, None, None, 5, "host", m=300)
    got = _run(J, used, X, Pred, Y, B, rows["asc"], None, 13, "device")
    used.close()
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------- viperm
def _xy(n, p, q, seed, const_col=None):
    rng = np.random.default_rng(seed)
    Z = rng.normal(size=(n, 4))
    X = np.asfortranarray(Z @ rng.normal(size=(4, p)) + 0.3 * rng.normal(size=(n, p)) + 1.0)
    if const_col is not None:
        X[:, const_col] = 0.75
    Y = np.asfortranarray(Z[:, :q] * 2.0 + X[:, :q] + 0.2 * rng.normal(size=(n, q)))
    return X, Y


def _all_scores(pred, Y):
    sc = V.np_scores()
    return np.hstack([sc[nm](pred, Y) for nm in NAMES])


_LITERAL = {}


def _literal(J, ctx, fname, kw, q, nrep=2, seed=31):
    """The literal src/viperm.jl on the library's own fits and predicts, every named score at once: res (p, 6 q, nrep), score0 (6 q, nrep)."""
    key = (fname, q)
    if key not in _LITERAL:
        X, Y = _xy(150, 12, q, 77 + q, const_col=5)
        n, p = X.shape
        splits = _splits(n, 50, nrep, seed, None)
        s = [r for r, _ in splits]
        perms = [V.perm_matrix(ps, 50, p) for _, ps in splits]
        fun = getattr(J, fname)
        _, res, score0 = V.viperm_literal(X, Y, s, perms, _all_scores, lambda Xc, Yc: fun(np.asfortranarray(Xc), np.asfortranarray(Yc), ctx=ctx, **kw),
                                          lambda fm, Xv: np.asarray(J.predict(fm, np.asfortranarray(Xv), ctx=ctx)))
        _LITERAL[key] = (X, Y, s, res, score0)
    return _LITERAL[key]


FUNS = {"plskern": dict(nlv=3), "pcr": dict(nlv=3), "covselr": dict(nlv=4)}


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("fname", sorted(FUNS))
def test_viperm_fast_route_against_the_literal_restatement(J, ctx, fname, q, where):
    X, Y, s, res_lit, score0 = _literal(J, ctx, fname, FUNS[fname], q)
    p = X.shape[1]
    Xv, Yv = (_dev(X), _dev(Y)) if where == "device" else (X, Y)
    for k, name in enumerate(NAMES):
        out = J.viperm(Xv, Yv, perm=2, score=getattr(J, name), fun=getattr(J, fname), seed=31, ctx=ctx, **FUNS[fname])
        assert out.res.shape == (p, q, 2) and out.imp.shape == (p, q) and np.array_equal(out.imp, out.res.mean(axis=2))
        want, s0 = res_lit[:, k * q:(k + 1) * q, :], score0[k * q:(k + 1) * q, :]
        err = np.abs(out.res - want) / np.abs(s0)[None, :, :]
        print(f"{fname} q={q} {where} {name}: max |res - literal| / |score0| = {err.max():.2e}")
        assert np.all(err <= 1e-9)
        assert np.all(out.res[5] == 0.0)                                    # the constant column: exactly 0, as in the reference
        # the pinned rows give the same replications
        if name == "rmsep" and where == "host":
            pinned = J.viperm(Xv, Yv, perm=2, score=J.rmsep, fun=getattr(J, fname), seed=31, s=s, ctx=ctx, **FUNS[fname])
            assert np.array_equal(pinned.res, out.res)


def test_viperm_loop_route_against_the_literal_restatement(J, ctx):
    X, Y, s, res_lit, score0 = _literal(J, ctx, "plskern", FUNS["plskern"], 3)
    k = NAMES.index("rmsep")
    out = J.viperm(X, Y, perm=2, score=J.rmsep, fun=J.plskern, seed=31, route="loop", ctx=ctx, nlv=3)
    err = np.abs(out.res - res_lit[:, 3 * k:3 * k + 3, :]) / np.abs(score0[3 * k:3 * k + 3, :])[None, :, :]
    print(f"loop route: max |res - literal| / |score0| = {err.max():.2e}")
    assert np.all(err <= 1e-9) and np.all(out.res[5] == 0.0)
    fast = J.viperm(X, Y, perm=2, score=J.rmsep, fun=J.plskern, seed=31, route="fast", ctx=ctx, nlv=3)
    assert np.all(np.abs(fast.res - out.res) <= 1e-9 * np.abs(score0[3 * k:3 * k + 3, :])[None, :, :])      # both routes see the same shuffles


def test_a_lambda_score_and_a_non_linear_fun_take_the_loop_route(J, ctx):
    X, Y = _xy(90, 5, 2, 55)
    rm = V.np_scores()["rmsep"]
    score = lambda pred, Yv: rm(np.asarray(pred), np.asarray(Yv))  # noqa: E731
    splits = _splits(90, 30, 1, 8, None)
    s = [r for r, _ in splits]
    perms = [V.perm_matrix(ps, 30, 5) for _, ps in splits]

    def pred_of(fm, Xv):
        pr = J.predict(fm, np.asfortranarray(Xv), ctx=ctx)
        return np.asarray(getattr(pr, "pred", pr))

    for fun, kw in ((J.knnr, dict(k=3)), (J.plskern, dict(nlv=2))):
        out = J.viperm(X, Y, perm=1, score=score, fun=fun, seed=8, ctx=ctx, **kw)
        _, want, score0 = V.viperm_literal(X, Y, s, perms, score, lambda Xc, Yc: fun(np.asfortranarray(Xc), np.asfortranarray(Yc), ctx=ctx, **kw), pred_of)
        assert np.all(np.abs(out.res - want) <= 1e-9 * np.abs(score0)[None, :, :])
        assert np.any(out.res != 0.0)


# ---------------------------------------------------------------------------------------------------- isel
@pytest.mark.parametrize("where", ["host", "device"])
def test_isel_against_the_literal_restatement(J, ctx, where):
    X, Y = _xy(120, 10, 2, 66)
    splits = _splits(120, 40, 2, 9, None)
    s = [r for r, _ in splits]
    sc = V.np_scores()["rmsep"]
    res, res0, res_rep, res0_rep, it = V.isel_literal(X, Y, s, 4, sc, lambda Xc, Yc: J.plskern(np.asfortranarray(Xc), np.asfortranarray(Yc), nlv=2, ctx=ctx),
                                                      lambda fm, Xv: np.asarray(J.predict(fm, np.asfortranarray(Xv), ctx=ctx)))
    Xv, Yv = (_dev(X), _dev(Y)) if where == "device" else (X, Y)
    wl = np.linspace(1100.0, 1118.0, 10)
    out = J.isel(Xv, Yv, wl, rep=2, nint=4, fun=J.plskern, seed=9, ctx=ctx, nlv=2)
    assert np.array_equal(out.int, it - 1) and np.array_equal(it[:, :2], [[1, 3], [4, 5], [6, 7], [8, 10]])
    assert np.array_equal(out.res["lo"], wl[it[:, 0] - 1]) and np.array_equal(out.res["up"], wl[it[:, 1] - 1]) and np.array_equal(out.res["mid"], wl[it[:, 2] - 1])
    assert list(out.res) == ["lo", "up", "mid", "y1", "y2"] and list(out.res0) == ["y1", "y2"]
    assert out.res_rep.shape == (4, 2, 2) and out.res0_rep.shape == (1, 2, 2)
    assert np.all(np.abs(out.res_rep - res_rep) <= 1e-9 * np.abs(res_rep)) and np.all(np.abs(out.res0_rep - res0_rep) <= 1e-9 * np.abs(res0_rep))
    assert np.allclose(np.stack([out.res["y1"], out.res["y2"]], axis=1), res, rtol=1e-9, atol=0) and np.allclose(out.res0["y1"], res0[0, 0], rtol=1e-9, atol=0)
    # a callable score and a fit without weights: gathered rows, the same numbers
    loop = J.isel(X, Y, wl, rep=2, nint=4, fun=J.plskern, seed=9, ctx=ctx, nlv=2, score=lambda pr, yv: sc(np.asarray(pr), np.asarray(yv)))
    assert np.all(np.abs(loop.res_rep - res_rep) <= 1e-9 * np.abs(res_rep))
