"""GPU checks of the kernel density family (jch_kde_dens; dmkern, kdeda, plskdeda of jchemo_hip/kde.py) against the longdouble restatements and the
derived error bound of tests/test_kde_static.py.  Every comparison prints its largest measured / allowed ratio before it asserts.

Measured on an MI355X, largest measured / allowed: the primitive 0.19, dmkern 0.006, kdeda 0.067 (dens) / 0.059 (posterior), plskdeda 0.56 / 0.32
(DESIGN.md §21)."""
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

from oracle import plsr_oracle as O  # noqa: E402
from test_kde_static import (FAR, LD, NLV, PRIM_CASES, assert_gap, clusters, kdeda_reference, ld_kde_dens, np_dmkern,  # noqa: E402
                             plskdeda_reference, prim_case, prim_inputs, ratio)

SENT = 7.0


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


def _dev(a):
    a = np.asarray(a, dtype=np.float64)
    t = torch.empty(a.shape[::-1], dtype=torch.float64, device="cuda:0").t() if a.ndim == 2 else torch.empty(a.shape, dtype=torch.float64, device="cuda:0")
    t.copy_(torch.from_numpy(np.array(a, order="C")))
    return t


def _dev_colmajor(A, ld, offset):
    """A device copy of A with leading dimension ld whose first element sits `offset` doubles behind an allocation's start; sentinels elsewhere."""
    n, c = A.shape
    buf = torch.full((offset + ld * c + 1,), SENT, dtype=torch.float64, device="cuda:0")
    V = buf[offset:offset + ld * c].view(c, ld).t()
    V[:n].copy_(torch.as_tensor(np.array(A), device="cuda:0"))
    return buf, buf.data_ptr() + 8 * offset


def call_abi(J, ctx, inp, loc, *, Z=None, Xq=None, out=None, ldz=None, ldq=None, ldo=None, cs=None, dims=None, n=None, m=None, d=None, nulls=()):
    """jch_kde_dens with the arrays of `inp` (every keyword overrides one argument); returns the status.  Z / Xq / out are raw addresses."""
    cs = np.ascontiguousarray(inp["cs"] if cs is None else cs, dtype=np.int64)
    dm = np.ascontiguousarray(inp["dims"] if dims is None else dims, dtype=np.int32)
    u, v2, coef = (np.asfortranarray(inp[k]) for k in ("u", "v2", "coef"))
    n0, d0 = inp["Z"].shape
    m0 = inp["Xq"].shape[0]
    args = dict(Z=Z, n=n0 if n is None else n, d=d0 if d is None else d, ldz=ldz, Xq=Xq, m=m0 if m is None else m, ldq=ldq, cs=cs.ctypes.data, ncls=len(cs) - 1,
                u=u.ctypes.data, v2=v2.ctypes.data, coef=coef.ctypes.data, dims=dm.ctypes.data, nmod=len(dm), out=out, ldo=ldo)
    for k in nulls:
        args[k] = None
    return J.load().jch_kde_dens(ctx._h, loc, args["Z"], args["n"], args["d"], args["ldz"], args["Xq"], args["m"], args["ldq"], args["cs"], args["ncls"],
                                 args["u"], args["v2"], args["coef"], args["dims"], args["nmod"], args["out"], args["ldo"])


def run_device(J, ctx, inp):
    """Device inputs with ld = rows + 3 at an offset of one double into their allocations; out likewise, sentinels all around it.  Returns the
    (m, ncls, nmod) result after checking that every sentinel survived."""
    (n, d), m = inp["Z"].shape, inp["Xq"].shape[0]
    ncm = (len(inp["cs"]) - 1) * len(inp["dims"])
    zb, za = _dev_colmajor(inp["Z"], n + 3, 1)
    qb, qa = _dev_colmajor(inp["Xq"], m + 3, 1)
    ob, oa = _dev_colmajor(np.full((m, ncm), SENT), m + 3, 1)
    torch.cuda.synchronize()
    ctx.check(call_abi(J, ctx, inp, J._lib.LOC_DEVICE, Z=za, Xq=qa, out=oa, ldz=n + 3, ldq=m + 3, ldo=m + 3))
    ctx.synchronize()
    O = _host(ob)
    body = O[1:1 + (m + 3) * ncm].reshape(ncm, m + 3)
    assert O[0] == SENT and O[-1] == SENT and np.all(body[:, m:] == SENT), "a sentinel around `out` was overwritten"
    for b in (zb, qb):
        hb = _host(b)
        assert hb[0] == SENT and hb[-1] == SENT
    return body[:, :m].T.reshape(m, len(inp["dims"]), len(inp["cs"]) - 1).transpose(0, 2, 1)


def run_host(J, ctx, inp):
    (n, d), m = inp["Z"].shape, inp["Xq"].shape[0]
    ncls, nmod = len(inp["cs"]) - 1, len(inp["dims"])
    Z, Xq = np.asfortranarray(inp["Z"]), np.asfortranarray(inp["Xq"])
    out = np.full((nmod * ncls, m), SENT)
    ctx.check(call_abi(J, ctx, inp, J._lib.LOC_HOST, Z=Z.ctypes.data, Xq=Xq.ctypes.data, out=out.ctypes.data, ldz=n, ldq=m, ldo=m))
    return out.T.reshape(m, nmod, ncls).transpose(0, 2, 1)


# ---------------------------------------------------------------------------------- a. the primitive through the C ABI
@pytest.mark.parametrize("name", list(PRIM_CASES))
def test_primitive_against_longdouble(J, ctx, name):
    inp, ref, bound = prim_case(name)
    got = run_device(J, ctx, inp)
    r = ratio(got, ref, bound)
    print(f"{name}: device against longdouble, largest measured / allowed = {r:.3f}")
    assert r <= 1.0
    again = run_device(J, ctx, inp)
    assert np.array_equal(got, again), "two calls differ in their bits"
    hst = run_host(J, ctx, inp)
    assert np.array_equal(got, hst), "loc = host differs from loc = device"


def test_far_query_is_exactly_zero_in_every_model(J, ctx):
    for name in ("m65_mixed_d7_nested", "m63_mixed_d33_nested", "m65_mixed_d130_nested", "m65_dims_2_2_5"):
        inp = dict(prim_case(name)[0])
        Xq = np.array(inp["Xq"])
        Xq[3] += FAR / inp["u"].min()
        inp["Xq"] = np.asfortranarray(Xq)
        got = run_device(J, ctx, inp)
        assert np.all(got[3] == 0.0), name
        assert np.all(got[2] > 0.0) and np.all(got[4] > 0.0), name


def test_bad_arguments_leave_out_untouched(J, ctx):
    inp = prim_case("m65_dims_2_2_5")[0]
    (n, d), m = inp["Z"].shape, inp["Xq"].shape[0]
    ncm = (len(inp["cs"]) - 1) * len(inp["dims"])
    zb, za = _dev_colmajor(inp["Z"], n, 0)
    qb, qa = _dev_colmajor(inp["Xq"], m, 0)
    ob, oa = _dev_colmajor(np.full((m, ncm), SENT), m, 0)
    good = dict(Z=za, Xq=qa, out=oa, ldz=n, ldq=m, ldo=m)
    cs = np.array(inp["cs"])
    bad = {
        "ldz < n": dict(ldz=n - 1), "ldq < m": dict(ldq=m - 1), "ldo < m": dict(ldo=m - 1),
        "dims decreasing": dict(dims=[2, 1, 5]), "dims above d": dict(dims=[2, 2, d + 1]), "dims below 1": dict(dims=[0, 2, 5]),
        "empty class": dict(cs=[0, cs[1], cs[1], cs[3]]), "cls_start decreasing": dict(cs=[0, cs[2], cs[1], cs[3]]),
        "cls_start short of n": dict(cs=[0, cs[1], cs[2], cs[3] - 1]), "cls_start beyond n": dict(cs=[0, cs[1], cs[2], cs[3] + 1]),
        "cls_start not from 0": dict(cs=[1, cs[1], cs[2], cs[3]]),
        "n = 0": dict(n=0), "m = 0": dict(m=0), "d = 0": dict(d=0), "bad loc": None,
        **{f"NULL {k}": dict(nulls=(k,)) for k in ("Z", "Xq", "cs", "u", "v2", "coef", "dims", "out")},
    }
    for what, kw in bad.items():
        st = call_abi(J, ctx, inp, 7, **good) if kw is None else call_abi(J, ctx, inp, J._lib.LOC_DEVICE, **{**good, **kw})
        assert st == J._lib.JCH_EINVAL, (what, st)
    ctx.synchronize()
    assert np.all(_host(ob) == SENT)
    ctx.check(call_abi(J, ctx, inp, J._lib.LOC_DEVICE, **good))        # (the control: the good call does write)
    assert not np.any(_host(ob)[:m * ncm] == SENT)


# ---------------------------------------------------------------------------------- b. the models against the restatements
def _check(what, got, ref, bound):
    r = ratio(_host(got), ref, bound)
    print(f"{what}: largest measured / allowed = {r:.3f}")
    assert r <= 1.0, what


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("h,a", [(None, 1), (None, 0.5), (0.3, 1), ("vec", 1)])
@pytest.mark.parametrize("p", [1, 4])
def test_dmkern(J, ctx, p, h, a, where):
    cl = clusters()
    hv = np.linspace(0.2, 0.5, p) if h == "vec" else h
    Z, Xq = np.asfortranarray(cl["L"][:, :p]), np.asfortranarray(cl["Lq"][:, :p])
    put = _dev if where == "device" else (lambda x: x)
    fm = J.dmkern(put(Z), h=hv, a=a, ctx=ctx)
    pred = J.dmkern_predict(fm, put(Xq), ctx=ctx)
    assert isinstance(pred, torch.Tensor) == (where == "device") and tuple(pred.shape) == (Xq.shape[0], 1)
    fl = np_dmkern(Z, h=hv, a=a, ft=LD)
    n = Z.shape[0]
    coef = np.array([[1 / LD(n) * (2 * LD(np.pi)) ** (-LD(p) / 2) * (1 / fl["detH"])]], dtype=LD)
    ref, bound = ld_kde_dens(Z, Xq, [0, n], np.diag(fl["Hinv"]).reshape(p, 1), [[1]], coef, [p], model_level=True)
    _check(f"dmkern p={p} h={h} a={a} {where}", _host(pred)[:, 0], ref[:, 0, 0], bound[:, 0, 0])
    assert _host(pred)[-1, 0] == 0.0
    assert abs(fm.detH - float(fl["detH"])) <= (p * (n + 4) + p + 2) * 2.0 ** -52 * float(fl["detH"])


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("prior", ["unif", "prop"])
def test_kdeda(J, ctx, prior, where):
    cl = clusters()
    put = _dev if where == "device" else (lambda x: x)
    obj = J.kdeda(put(cl["L"]), cl["y"], prior=prior, ctx=ctx)
    pred, dens, post = J.kdeda_predict(obj, put(cl["Lq"]), ctx=ctx)
    assert isinstance(dens, torch.Tensor) == (where == "device") and isinstance(post, torch.Tensor) == (where == "device") and isinstance(pred, np.ndarray)
    ref_obj, rd, rb, rp, rpb, rpred = kdeda_reference(cl["L"], cl["Lq"], cl["y"], prior, None, 1)
    assert list(obj.lev) == list(ref_obj["lev"]) and list(obj.ni) == list(ref_obj["ni"]) and np.allclose(obj.wprior, np.asarray(ref_obj["wprior"], dtype=np.float64), rtol=1e-15)
    _check(f"kdeda {prior} {where} dens", dens, rd, rb)
    _check(f"kdeda {prior} {where} posterior", _host(post)[:-1], rp[:-1], rpb[:-1])
    assert_gap(rp, rpb, f"kdeda {prior}")
    assert np.array_equal(pred[:-1], rpred[:-1])                        # every query
    assert np.all(_host(dens)[-1] == 0.0) and np.all(np.isnan(_host(post)[-1])) and pred[-1, 0] == obj.lev[0]   # the far one


PLS_CASES = [(False, False, "unif", None, 1), (True, False, "prop", None, 1), (False, True, "unif", None, 0.5), (True, True, "prop", 0.3, 1)]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("weighted,scal,prior,h,a", PLS_CASES)
def test_plskdeda(J, ctx, weighted, scal, prior, h, a, where):
    """X 197 x 40, nlv = 5.  The restatement runs on the DEVICE fit's scores and the device transform of the queries (plskern and transform have
    tests of their own): what is compared is the density family."""
    cl = clusters()
    put = _dev if where == "device" else (lambda x: np.array(x))
    w = put(cl["w"]) if weighted else None
    obj = J.plskdeda(put(cl["X"]), cl["y"], w, nlv=NLV, prior=prior, h=h, a=a, scal=scal, ctx=ctx)
    assert isinstance(obj, J.Plslda) and len(obj.fm_da) == NLV and all(isinstance(f, J.Kernda) for f in obj.fm_da)
    T, Tq = _host(obj.fm_pls.T), _host(J.transform(obj.fm_pls, put(cl["Xq"]), ctx=ctx))
    rng = list(range(1, NLV + 1))
    ref = plskdeda_reference(T, Tq, cl["y"], prior, h, a, rng)
    preds, posts = J.plskdeda_predict(obj, put(cl["Xq"]), nlv=(0, 7), ctx=ctx)          # 0:7 clamps to 1:5
    assert len(preds) == NLV and len(posts) == NLV
    for k, (rd, rb, rp, rpb, rpred), pred, post in zip(rng, ref, preds, posts):
        assert isinstance(post, torch.Tensor) == (where == "device") and isinstance(pred, np.ndarray)
        _check(f"plskdeda nlv={k} {where} posterior", _host(post)[:-1], rp[:-1], rpb[:-1])
        assert_gap(rp, rpb, f"plskdeda nlv={k}")
        assert np.array_equal(pred[:-1], rpred[:-1]), k
        assert np.all(np.isnan(_host(post)[-1])) and pred[-1, 0] == obj.lev[0], k
        # dens of model k through kdeda_predict on the stored Kernda: the same numbers as the nested call
        p1, d1, po1 = J.kdeda_predict(obj.fm_da[k - 1], put(np.asfortranarray(Tq[:, :k])), ctx=ctx)
        _check(f"plskdeda nlv={k} {where} dens", d1, rd, rb)
        assert np.array_equal(p1, pred)
    p5, po5 = J.plskdeda_predict(obj, put(cl["Xq"]), ctx=ctx)                            # nlv = None: the largest model
    assert np.array_equal(p5, preds[-1]) and np.array_equal(_host(po5), _host(posts[-1]), equal_nan=True)
    p3, po3 = J.plskdeda_predict(obj, put(cl["Xq"]), nlv=3, ctx=ctx)
    assert np.array_equal(p3, preds[2]) and np.array_equal(_host(po3), _host(posts[2]), equal_nan=True)
    with pytest.raises(ValueError):
        J.plskdeda_predict(obj, put(cl["Xq"]), nlv=0, ctx=ctx)
    with pytest.raises(ValueError):
        J.plslda_predict(J.plslda(put(cl["X"]), cl["y"], nlv=2, ctx=ctx), put(cl["Xq"]), nlv=0, ctx=ctx)   # ... as plslda_predict does


# ---------------------------------------------------------------------------------- c. a used ctx
def test_on_a_used_ctx(J):
    """plskern(reuse_x=True) twice, then plskdeda and its predict on the same ctx and the same X, then the same plskern again: the copy the
    fit inside plskdeda left is of the same X and none of the density calls touches it, so the reuse counter advances; the third fit equals the
    first; the density results equal those of a fresh ctx bit for bit.  (Device tensors: a host-array X is staged through the buffer the reuse
    state lives in by every host-array call, jch_col_stats and jch_transform among them, which drops the copy as it must.)"""
    cl = clusters()
    X, Xq, y = _dev(cl["X"]), _dev(cl["Xq"]), cl["y"]
    Yd = _dev((y[:, None] == np.unique(y)[None, :]).astype(np.float64))
    used, fresh = J.Context(0), J.Context(0)
    try:
        a1 = J.plskern(X, Yd, nlv=NLV, ctx=used, reuse_x=True)
        c0 = used.counter(J._lib.COUNTER_XCOPY_REUSED)
        J.plskern(X, Yd, nlv=NLV, ctx=used, reuse_x=True)
        c1 = used.counter(J._lib.COUNTER_XCOPY_REUSED)
        assert c1 == c0 + 1
        obj = J.plskdeda(X, y, nlv=NLV, ctx=used)
        res = J.plskdeda_predict(obj, Xq, nlv=(1, NLV), ctx=used)
        a3 = J.plskern(X, Yd, nlv=NLV, ctx=used, reuse_x=True)
        assert used.counter(J._lib.COUNTER_XCOPY_REUSED) == c1 + 1
        s = O.sign_align(_host(a1.W), _host(a3.W))                      # (the criterion of tests/test_gpu_used_ctx.py for a fit from the copy)
        for f in ("T", "P", "R", "W", "C"):
            assert O.rel_fro(_host(getattr(a1, f)), _host(getattr(a3, f)) * s) < 1e-10, f
        assert O.rel_fro(a1.xmeans, a3.xmeans) < 1e-13
        obj2 = J.plskdeda(X, y, nlv=NLV, ctx=fresh)
        res2 = J.plskdeda_predict(obj2, Xq, nlv=(1, NLV), ctx=fresh)
        for k in range(NLV):
            assert np.array_equal(res[0][k], res2[0][k])
            assert np.array_equal(_host(res[1][k]), _host(res2[1][k]), equal_nan=True), k
        inp = prim_case("m257_mixed_d25_nested")[0]
        assert np.array_equal(run_device(J, used, inp), run_device(J, fresh, inp))
    finally:
        used.close(); fresh.close()


# ---------------------------------------------------------------------------------- d. host arrays and device tensors
def test_host_arrays_and_device_tensors_agree(J, ctx):
    cl = clusters()
    L, Lq, y = np.array(cl["L"]), np.array(cl["Lq"]), cl["y"]
    ph, dh, poh = J.kdeda_predict(J.kdeda(L, y, ctx=ctx), Lq, ctx=ctx)
    pd, dd, pod = J.kdeda_predict(J.kdeda(_dev(L), y, ctx=ctx), _dev(Lq), ctx=ctx)
    assert np.array_equal(ph, pd) and np.array_equal(dh, _host(dd)) and np.array_equal(poh, _host(pod), equal_nan=True)
    gh = J.dmkern_predict(J.dmkern(L[:, :2], ctx=ctx), Lq[:, :2], ctx=ctx)
    gd = J.dmkern_predict(J.dmkern(_dev(L[:, :2]), ctx=ctx), _dev(Lq[:, :2]), ctx=ctx)
    assert np.array_equal(gh, _host(gd))
    inp = prim_inputs(11, 70, (5, 66), 6, (1, 3, 6))
    oh = J.kde_dens(inp["Z"], inp["Xq"], inp["cs"], inp["u"], inp["v2"], inp["coef"], inp["dims"], ctx=ctx)
    od = J.kde_dens(_dev(inp["Z"]), _dev(inp["Xq"]), inp["cs"], inp["u"], inp["v2"], inp["coef"], inp["dims"], ctx=ctx)
    assert oh.shape == (70, 2, 3) and np.array_equal(oh, _host(od))
    ref, bound = ld_kde_dens(inp["Z"], inp["Xq"], inp["cs"], inp["u"], inp["v2"], inp["coef"], inp["dims"])
    assert ratio(oh, ref, bound) <= 1.0


# ---------------------------------------------------------------------------------- the three routes of the C entries (tests/host_routes.py)
@pytest.mark.parametrize("entry", sorted(__import__("host_routes").ROUTES["kde"]))
def test_host_arrays_padded_and_unpadded_give_the_bits_of_the_device_route(entry):
    """Device buffers, host arrays with ld == rows and with ld = rows + 3 between NaN guards: equal bytes, NaN padding kept, inputs unchanged."""
    import host_routes as HR
    HR.three_routes(HR.ROUTES["kde"][entry])
