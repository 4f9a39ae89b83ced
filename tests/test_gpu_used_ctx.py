"""Every entry on a USED ctx.  A jch_ctx is a grow-only workspace (csrc/jch_internal.h) that every entry point carves up for itself;
`jch_reserve` neither shrinks nor clears, so an entry that runs behind a larger call sees that call's bytes in whatever it does not
rewrite itself (pad columns, tails of partial-sum and ticket buffers, shared staging).  Fresh device memory is usually zero, so a
kernel that reads a pad it never wrote passes on a fresh ctx and fails in a session.

Part A: each family runs on a fresh ctx, on a second fresh ctx (the control) and on `dirty_ctx`, a ctx that has run one LARGER call of
every family on finite data of magnitude 2^40.  Whatever the two fresh runs agree on to the byte, the dirty run has to reproduce to the
byte; the fresh run is also held against the family's own CPU reference at the tolerance of the family's own test file, so that "equal
to fresh" cannot mean "equally wrong".  A closing test runs every victim once more on the dirty ctx in reverse order.

Part B: plskern(X) / ONE call of any family / plskern(X, reuse_x=True) on one ctx: the third call must equal the same fit on a fresh
ctx, whatever ran in between (JCH_REUSE_XCOPY: the bit is ignored, with correct results, after any call that touched the staging
buffer or the working copy).

Entries whose two FRESH runs are not byte-equal (the dirty run is then held against the CPU reference instead of the fresh bytes);
at most a quarter of the families may appear here:

    family      cause
    (none: every family below repeats its own bits on two fresh ctxs)
"""
import dataclasses
import os
import sys
import warnings
from functools import lru_cache

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "jchemo.jl_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import jchemo_hip as J  # noqa: E402
from oracle import c_oracle as CO  # noqa: E402
from oracle import plsr_oracle as O  # noqa: E402

import test_gpu_covsel as TCOV  # noqa: E402
import test_gpu_dkplsr as TDK  # noqa: E402
import test_gpu_kpca as TKPCA  # noqa: E402
import test_gpu_krr as TKRR  # noqa: E402
import test_gpu_occ as TOCC  # noqa: E402
import test_gpu_parity as TPAR  # noqa: E402
import test_gpu_pca as TPCA  # noqa: E402
import test_gpu_preproc as TPRE  # noqa: E402
import test_gpu_stah as TSTAH  # noqa: E402
import test_covsel_static as SCOV  # noqa: E402
import test_kplsr_static as SKPL  # noqa: E402
import test_kpca_static as SKPCA  # noqa: E402
import test_krr_static as SKRR  # noqa: E402
import test_occ_static as SOCC  # noqa: E402
import test_pca_static as SPCA  # noqa: E402
import test_preproc_static as SPRE  # noqa: E402
import test_samp_static as SSAMP  # noqa: E402
import test_stah_static as SSTAH  # noqa: E402

# family -> the cause, found in the code, of two fresh runs differing (see the table in the module docstring)
NOT_BYTE_REPRODUCIBLE = {}

S1, S2, S3 = (613, 37, 3), (300, 515, 1), (200, 2049, 2)   # odd p (a pad column), q far from qpad, n no multiple of 64; ldr > 512; p > JCH_SWEEP_MAXP
FIELDS = ("T", "P", "R", "W", "C")
EPS = float(np.finfo(np.float64).eps)


# ---------------------------------------------------------------------------------- plumbing
def host(a):
    if torch.is_tensor(a):
        a = a.detach()
        return (a.to(torch.float64) if a.dtype == torch.bfloat16 else a).cpu().numpy()
    return np.asarray(a)


def put(a, where, dtype=None):
    """A private copy of the master `a` for one call: column-major host array or device tensor."""
    a = np.asarray(a)
    if where == "host":
        return np.array(a, order="F", copy=True)
    if a.ndim == 1:
        return torch.from_numpy(a.copy()).cuda()
    t = J.colmajor_empty(a.shape[0], a.shape[1], "cuda:0", dtype=dtype)
    t.copy_(torch.from_numpy(np.array(a, order="C", copy=True)))
    return t


class Inputs:
    """The caller's arrays of one call: private copies of the masters, compared with them after the call."""

    def __init__(self, where):
        self.where, self.items = where, []

    def __call__(self, master, dtype=None, inplace=False):
        if master is None:
            return None
        a = put(master, self.where, dtype)
        if not inplace:
            self.items.append((a, host(a).copy()))
        return a

    def unchanged(self):
        for a, m in self.items:
            assert np.array_equal(host(a), m), "an input the caller owns was modified"


def flat(obj, pre="", out=None):
    """Every array and scalar a result exposes, by path."""
    out = {} if out is None else out
    if obj is None or isinstance(obj, (str, bytes)):
        return out
    if torch.is_tensor(obj) or isinstance(obj, np.ndarray):
        out[pre] = host(obj).copy()
    elif isinstance(obj, (bool, int, float, np.generic)):
        out[pre] = np.asarray(obj)
    elif dataclasses.is_dataclass(obj) and not isinstance(obj, type):
        for f in dataclasses.fields(obj):
            flat(getattr(obj, f.name), f"{pre}.{f.name}", out)
    elif isinstance(obj, dict):
        for k, v in obj.items():
            flat(v, f"{pre}[{k}]", out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            flat(v, f"{pre}[{i}]", out)
    return out


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def differing(fa, fb):
    assert set(fa) == set(fb), sorted(set(fa) ^ set(fb))
    return sorted(k for k in fa if not same_bytes(fa[k], fb[k]))


class env:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def rel(a, b):
    return O.rel_fro(np.asarray(b), np.asarray(a))


# ---------------------------------------------------------------------------------- the PLS fits
@lru_cache(maxsize=None)
def pls_data(shape, offset=2.0):
    n, p, q = shape
    X = CO.fill_uniform(431 + n, n, p) + offset
    B = CO.fill_uniform(432, p, q) - 0.5
    Y = X @ B + 0.1 * CO.fill_uniform(433, n, q)
    w = CO.fill_uniform(435, n, 1)[:, 0] + 0.1
    Xn = CO.fill_uniform(437, 50, p) + offset
    Yn = Xn @ B + 0.1 * CO.fill_uniform(438, 50, q)
    out = tuple(np.asfortranarray(a) for a in (X, Y, w, Xn, Yn))
    for a in out:
        a.setflags(write=False)
    return out


def bf16_round(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(torch.bfloat16).to(torch.float64).numpy()


PLS_NLV = 5
# name: (mirror function, oracle name, keywords, weights, where, bf16)
PLS = {
    "plskern": ("plskern", dict(), False, "host", False),
    "plskern_scal_w": ("plskern", dict(scal=True), True, "device", False),
    "plskern_variant1": ("plskern", dict(variant=1), True, "host", False),
    "plskern_bf16": ("plskern", dict(), False, "device", True),
    "plsnipals": ("plsnipals", dict(), True, "host", False),
    "plsnipals_dev": ("plsnipals", dict(scal=True), False, "device", False),
    "plssimp": ("plssimp", dict(), True, "device", False),
    "plsrosa": ("plsrosa", dict(scal=True), False, "host", False),
    "plswold": ("plswold", dict(), True, "device", False),
}


@lru_cache(maxsize=None)
def pls_ref(name, shape):
    fn, kw, use_w, _, bf16 = PLS[name]
    X, Y, w, _, _ = pls_data(shape, 0.0 if bf16 else 2.0)
    if bf16:
        X, Y = bf16_round(X), bf16_round(Y)
    kw = {k: v for k, v in kw.items() if k != "variant"}
    return getattr(O, fn)(X, Y, w if use_w else None, nlv=PLS_NLV, **kw)


def pls_victim(name):
    fn, kw, use_w, where, bf16 = PLS[name]

    def run(ctx, shape):
        X, Y, w, _, _ = pls_data(shape, 0.0 if bf16 else 2.0)
        inp = Inputs(where)
        dt = torch.bfloat16 if bf16 else None
        fm = getattr(J, fn)(inp(X, dt), inp(Y, dt), inp(w if use_w else None), nlv=PLS_NLV, ctx=ctx, **kw)
        return fm, inp

    def check(fm, shape):
        ref = pls_ref(name, shape)
        tol = 1e-3 if bf16 else TPAR.TOL    # test_bf16_storage_mode's budget; the parity tolerance of test_gpu_parity.py
        s = O.sign_align(ref.W, fm.W)
        for f in FIELDS:
            assert O.rel_fro(getattr(ref, f), host(getattr(fm, f)) * s) < tol, (name, f)
        assert O.rel_fro(ref.xmeans, fm.xmeans) < (1e-7 if bf16 else tol) and O.rel_fro(ref.ymeans, fm.ymeans) < tol
        if not bf16:
            for f in ("TT", "xscales", "yscales"):
                assert O.rel_fro(getattr(ref, f), getattr(fm, f)) < tol, (name, f)

    return run, check, ((S1, S2) if kw.get("variant") else (S1, S2, S3))    # (algorithm #2 takes p <= 2048 only: JCH_EINVAL beyond)


# ---------------------------------------------------------------------------------- predict / transform / gridscorelv
def _oracle_model(shape):
    X, Y, w, _, _ = pls_data(shape)
    return O.plskern(X, Y, w, nlv=PLS_NLV, scal=True)


def accessor_victim(where):
    def run(ctx, shape):
        ref = _oracle_model(shape)
        fm = J.Plsr(*(np.array(getattr(ref, f), order="F") for f in ("T", "P", "R", "W", "C", "TT", "xmeans", "xscales", "ymeans", "yscales", "weights")))
        inp = Inputs(where)
        Xq = inp(pls_data(shape)[3])
        out = dict(transform=J.transform(fm, Xq, ctx=ctx), transform2=J.transform(fm, Xq, nlv=2, ctx=ctx),
                   predict=J.predict(fm, Xq, nlv=range(0, PLS_NLV + 1), ctx=ctx), predict1=J.predict(fm, Xq, nlv=3, ctx=ctx))
        return out, inp

    def check(out, shape):
        ref, Xn = _oracle_model(shape), pls_data(shape)[3]
        assert rel(host(out["transform"]), O.transform(ref, Xn)) < TPAR.TIGHT and rel(host(out["transform2"]), O.transform(ref, Xn, nlv=2)) < TPAR.TIGHT
        assert rel(np.stack([host(a) for a in out["predict"]]), np.stack(O.predict(ref, Xn, nlv=range(0, PLS_NLV + 1)))) < TPAR.TIGHT
        assert rel(host(out["predict1"]), O.predict(ref, Xn, nlv=3)) < TPAR.TIGHT

    return run, check, (S1, S2)


def gridscorelv_victim():
    def run(ctx, shape):
        X, Y, _, Xn, Yn = pls_data(shape)
        inp = Inputs("host")
        res = J.gridscorelv(inp(X), inp(Y), inp(Xn), inp(Yn), score=J.rmsep, fun=J.plskern, nlv=range(0, PLS_NLV + 1), ctx=ctx)
        return dict(nlv=list(res["nlv"]), res=res["res"]), inp

    def check(out, shape):
        X, Y, _, Xn, Yn = pls_data(shape)
        rng, ref = O.gridscorelv(X, Y, Xn, Yn, score=O.rmsep, fun=O.plskern, nlv=range(0, PLS_NLV + 1))
        assert out["nlv"] == rng and np.allclose(out["res"], ref, rtol=1e-8)    # test_scores_and_gridscorelv

    return run, check, (S1, S2)


# ---------------------------------------------------------------------------------- kNN-LWPLSR
LW = dict(nlvdis=4, metric="mahal", h=1.5, k=40, nlv=5, scal=False)


@lru_cache(maxsize=None)
def lw_data(shape, m=7):
    n, p, q = shape
    Lsrc = CO.fill_uniform(7, 25, p) - 0.5
    X = CO.fill_uniform(5, n, 25) @ Lsrc + 0.05 * CO.fill_uniform(20250112, n, p)
    Xq = CO.fill_uniform(6, m, 25) @ Lsrc + 0.05 * CO.fill_uniform(20250115, m, p)
    Y = np.column_stack([X[:, (3 * j) % p] * (1.0 + 0.3 * j) - X[:, (5 * j + 1) % p] + np.sin(2 * X[:, (j + 2) % p])
                         + 0.05 * CO.fill_uniform(20250113 + j, n, 1)[:, 0] for j in range(q)])
    return tuple(np.asfortranarray(a) for a in (X, Y, Xq))


@lru_cache(maxsize=None)
def lw_ref(shape):
    X, Y, Xq = lw_data(shape)
    return O.lwplsr_predict(O.lwplsr(X, Y, **LW), Xq, nlv=range(0, LW["nlv"] + 1))


def lwplsr_victim(kspace, where):
    def run(ctx, shape):
        X, Y, Xq = lw_data(shape)
        inp = Inputs(where)
        with env(JCH_LOCW_KSPACE=kspace):
            model = J.lwplsr(inp(X), inp(Y), ctx=ctx, **LW)
            one_shot = J.predict(model, inp(Xq), nlv=range(0, LW["nlv"] + 1), ctx=ctx)       # builds the handle, then predicts
            prepared = J.predict(model, inp(Xq[::-1]), nlv=range(0, LW["nlv"] + 1), ctx=ctx)  # through the prepared handle
        return dict(fm=model.fm, one_shot=one_shot, prepared=prepared), inp

    def check(out, shape):
        ref = lw_ref(shape)
        for got, order in ((out["one_shot"], slice(None)), (out["prepared"], slice(None, None, -1))):
            assert np.array_equal(got.listnn, ref["listnn"][order])
            for a in range(len(got.pred)):
                assert O.rel_fro(ref["pred"][order, :, a], got.pred[a]) < 1e-7, a     # test_lwplsr_kspace_matches_pspace

    return run, check, (S1, S2)


# ---------------------------------------------------------------------------------- kernel methods (first shape only)
DK = dict(name="used_ctx", n=S1[0], p=S1[1], q=S1[2], nlv=8, kern="krbf", kw=dict(gamma=0.1), scal=True, w=True)


def dkplsr_victim(where):
    def run(ctx, shape):
        X, Y, w = TDK._fit_data(DK)
        Xn = TDK.spectra(7 + DK["n"], 37, DK["p"])[0] * 3.0
        inp = Inputs(where)
        fm = J.dkplsr(inp(X), inp(Y), inp(w), nlv=DK["nlv"], kern="krbf", scal=True, ctx=ctx, **DK["kw"])
        Xq = inp(Xn)
        return dict(fm=fm, transform=J.transform(fm, Xq, ctx=ctx), predict=J.predict(fm, Xq, ctx=ctx)), inp

    def check(out, shape):
        X, Y, w = TDK._fit_data(DK)
        Xn = TDK.spectra(7 + DK["n"], 37, DK["p"])[0] * 3.0
        Xs, ref, xs, ys = TDK._ref_fit(X, Y, w, DK["nlv"], "krbf", True, DK["kw"])
        TDK._check_fit(out["fm"], ref, xs, ys, "used ctx")
        s = O.sign_align(ref.W, out["fm"].fm.W)
        Kn = TDK._ref_gram("krbf", Xn / xs, Xs, DK["kw"])
        assert O.rel_fro(O.transform(ref, Kn), host(out["transform"]) * s) < TDK.TOL
        assert O.rel_fro(O.predict(ref, Kn) * ys, host(out["predict"])) < TDK.TOL

    return run, check, (S1,)


@lru_cache(maxsize=None)
def kp_data():
    import test_gpu_kplsr as TKPL
    X, Y = TKPL.data(11, S1[0], S1[1], S1[2])
    Xn, _ = TKPL.data(60, 37, S1[1], S1[2])
    return X, Y, TKPL.weights_of("random", S1[0], 5), np.asfortranarray(Xn)


def kplsr_victim(where):
    kw = dict(nlv=6, kern="krbf", scal=True, gamma=0.5)

    def run(ctx, shape):
        X, Y, w, Xn = kp_data()
        inp = Inputs(where)
        fm = J.kplsr(inp(X), inp(Y), inp(w), ctx=ctx, **kw)
        Xq = inp(Xn)
        return dict(fm=fm, transform=J.transform(fm, Xq, ctx=ctx), predict=J.predict(fm, Xq, nlv=range(0, 7), ctx=ctx)), inp

    def check(out, shape):
        X, Y, w, Xn = kp_data()
        ref, fm = SKPL.np_kplsr(X, Y, w, **kw), out["fm"]
        for f in ("T", "U", "C", "R", "vtot"):
            assert SKPL.rel_fro(ref[f], host(getattr(fm, f))) <= 1e-6, f          # test_gpu_kplsr.TOL
        assert SKPL.rel_fro(ref["xscales"], fm.xscales) <= 1e-6 and SKPL.rel_fro(ref["ymeans"], fm.ymeans) <= 1e-6
        assert np.array_equal(np.asarray(fm.iter), ref["iter"])
        assert SKPL.rel_fro(SKPL.np_kplsr_transform(ref, Xn), host(out["transform"])) <= 1e-6
        for a, b in zip(SKPL.np_kplsr_predict(ref, Xn, range(0, 7)), out["predict"]):
            assert SKPL.rel_fro(a, host(b)) <= 1e-6

    return run, check, (S1,)


@lru_cache(maxsize=None)
def kd_data(q=S1[2]):
    n, p = S1[:2]
    X = SKPCA._data(n, p, n)
    Y = np.asfortranarray(np.random.default_rng(n + q).standard_normal((n, q)) * 0.1 + X[:, :q] ** 2)
    return X, Y, TKPCA._weights("rand", n), SKPCA._data(50, p, n + 1)


def kpca_victim(where):
    kw = dict(nlv=3, kern="krbf", scal=True, gamma=0.2)

    def run(ctx, shape):
        X, _, w, Xn = kd_data()
        inp = Inputs(where)
        fm = J.kpca(inp(X), inp(w), ctx=ctx, **kw)
        return dict(fm=fm, transform=J.kpca_transform(fm, inp(Xn), ctx=ctx), summary=J.kpca_summary(fm)), inp

    def check(out, shape):
        X, _, w, Xn = kd_data()
        ref, fm, nlv = SKPCA.np_kpca(X, w, **kw), out["fm"], kw["nlv"]
        e1 = ref["eig"][0]
        assert fm.converged
        assert np.max(np.abs(fm.eig - ref["eig"][:nlv])) <= 1e-10 * e1 and np.isclose(fm.sstot, ref["eig"].sum(), rtol=1e-12)
        assert np.allclose(fm.xscales, ref["xscales"], rtol=1e-13)
        P, T = host(fm.P), host(fm.T)
        TKPCA._compare_columns(P, ref["P"], ref["eig"], nlv, np.linalg.norm(ref["P"], axis=0))
        TKPCA._compare_columns(T, ref["T"], ref["eig"], nlv, np.linalg.norm(ref["T"], axis=0))
        sg = np.sign(np.sum(P * ref["P"], axis=0))
        Tn, Tr = host(out["transform"]), SKPCA.np_kpca_transform(ref, Xn) * sg
        gaps = TKPCA._gaps(ref["eig"], nlv)
        for i in range(nlv):
            if 10 * TKPCA.TOL * e1 / gaps[i] < 1e-3:
                assert np.linalg.norm(Tn[:, i] - Tr[:, i]) <= max(1e-9, 100 * TKPCA.TOL * e1 / gaps[i]) * max(np.linalg.norm(Tr[:, i]), 1e-300) + 1e-12

    return run, check, (S1,)


def krr_victim(where):
    kw, lbs = dict(kern="krbf", scal=True, gamma=0.2), [1e-1, 1e-2]

    def run(ctx, shape):
        X, Y, w, Xn = kd_data()
        inp = Inputs(where)
        fm = J.krr(inp(X), inp(Y), inp(w), lb=lbs[0], ctx=ctx, **kw)
        Xq = inp(Xn)
        coefs = [J.krr_coef(fm, lb=lb, ctx=ctx) for lb in lbs]
        return dict(fm=fm, coefs=coefs, predict=J.krr_predict(fm, Xq, lb=lbs, ctx=ctx)), inp

    def check(out, shape):
        X, Y, w, Xn = kd_data()
        n = X.shape[0]
        ref, fm = SKRR.np_krr(X, Y, w, lb=lbs[0], **kw), out["fm"]
        assert np.allclose(fm.xscales, ref["xscales"], rtol=1e-13) and np.allclose(fm.ymeans, ref["ymeans"], rtol=1e-13, atol=1e-15)
        assert TKRR._rel(host(fm.Kd), ref["Kd"]) < 1e-12 and TKRR._rel(host(fm.B), ref["DY"]) < 1e-14
        eig = ref["sv"] ** 2
        for i, lb in enumerate(lbs):     # the bounds of test_gpu_krr.test_parity_with_the_restatement
            cond = (eig.max() + lb ** 2) / (eig.min() + lb ** 2)
            r, c, rp = SKRR.np_krr_coef(ref, lb), SKRR.chol_route(ref, lb, Xn), SKRR.np_krr_predict(ref, Xn, lb)
            g_A, g_p, g_df = TKRR._rel(c["A"], r["A"]), TKRR._rel(c["pred"], rp, rp - ref["ymeans"]), abs(c["df"] - r["df"])
            A, _, df = out["coefs"][i]
            pred = host(out["predict"][i])
            tol_A, tol_p = min(max(10 * g_A, 50 * EPS * cond), TKRR.CAP), min(max(10 * g_p, 50 * EPS * cond), TKRR.CAP)
            tol_df = min(max(10 * g_df, 10 * n * EPS * cond), TKRR.CAP * r["df"])
            assert TKRR._rel(host(A), r["A"]) <= tol_A and TKRR._rel(pred, rp, rp - ref["ymeans"]) <= tol_p and abs(df - r["df"]) <= tol_df

    return run, check, (S1,)


# ---------------------------------------------------------------------------------- covsel, covselr
def _cov_case(shape):
    return (shape[0], shape[1], shape[2], 8, 1.0, 1)


def covsel_victim(where, regress):
    def run(ctx, shape):
        case = _cov_case(shape)
        X, Y, _, _ = SCOV.routes(case, "cov")
        k = SCOV.case_nlv(case, "cov")
        inp = Inputs(where)
        if not regress:
            return J.covsel(inp(X), inp(Y), nlv=k, ctx=ctx), inp
        fm = J.covselr(inp(X), inp(Y), k, "cov", ctx=ctx)
        Xn = SCOV.spectra_xy(100, shape[1], shape[2], 1.0, 99)[0]
        return dict(fm=fm, predict=J.predict(fm, inp(Xn), ctx=ctx)), inp

    def check(out, shape):
        case = _cov_case(shape)
        X, Y, lit, post = SCOV.routes(case, "cov")
        if not regress:
            assert np.array_equal(out.sel["sel"], lit["sel"]) and out.nlv == SCOV.case_nlv(case, "cov")
            return
        Xn = SCOV.spectra_xy(100, shape[1], shape[2], 1.0, 99)[0]
        Bref, b0ref = SCOV.np_covselr(X, Y, lit["sel"])
        Bpost, b0post = SCOV.covselr_from_parts(post)
        B, _ = J.coef(out["fm"])
        assert np.array_equal(out["fm"].sel["sel"], lit["sel"])
        TCOV._check("covselr B", B, Bref, TCOV._rule(Bref, Bpost, Bref))
        pref, ppost = b0ref + Xn[:, lit["sel"]] @ Bref, b0post + Xn[:, lit["sel"]] @ Bpost
        TCOV._check("covselr predictions", host(out["predict"]), pref, TCOV._rule(pref, ppost, pref))

    return run, check, (S1, S2)


# ---------------------------------------------------------------------------------- pcasvd, pcaeigen, pcr
PCA_NLV = 5


@lru_cache(maxsize=None)
def pca_data(shape):
    n, p, q = shape
    X = SPCA._data(n, p, n + p)
    Xc = X - X.mean(axis=0)
    Y = np.asfortranarray(Xc[:, :q] * 2.0 + Xc[:, 20:20 + q] + 5.0 + 0.05 * np.random.default_rng(21).standard_normal((n, q)))
    return X, Y, SPCA._weights("rand", n), TPCA._new_rows(X)


def pca_victim(fn, where):
    def run(ctx, shape):
        X, _, w, Xn = pca_data(shape)
        inp = Inputs(where)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            fm = getattr(J, fn)(inp(X), inp(w), nlv=PCA_NLV, scal=True, ctx=ctx)
        return dict(fm=fm, transform=J.transform(fm, inp(Xn), ctx=ctx)), inp

    def check(out, shape):
        X, _, w, Xn = pca_data(shape)
        p, fm = shape[1], out["fm"]
        ref = SPCA.np_pcasvd(X, w, nlv=PCA_NLV, scal=True)
        eig = ref["sv"] ** 2
        e1 = eig[0]
        assert fm.converged and np.max(np.abs(fm.eig - eig[:PCA_NLV])) <= 1e-10 * e1 and np.isclose(fm.sstot, eig.sum(), rtol=1e-12)
        assert np.allclose(fm.xmeans, ref["xmeans"], rtol=1e-12, atol=0) and np.allclose(fm.xscales, ref["xscales"], rtol=1e-12, atol=0)
        eig_pad = np.r_[eig, np.zeros(max(0, p - eig.size))]
        cols, cb = list(range(PCA_NLV)), TPCA._col_bounds(eig_pad, PCA_NLV)
        TPCA._compare_columns(fm.P, ref["P"], eig_pad, cols, np.ones(PCA_NLV))
        TPCA._compare_columns(host(fm.T), ref["T"], eig_pad, cols, np.linalg.norm(ref["T"], axis=0))
        sg = np.sign(np.sum(fm.P * ref["P"], axis=0))
        Tn, Tr = host(out["transform"]), SPCA.np_pca_transform(ref, Xn) * sg
        assert max(np.linalg.norm(Tn[:, i] - Tr[:, i]) / (max(1e-9, cb[i]) * max(np.linalg.norm(Tr[:, i]), 1e-300) + 1e-12) for i in cols) <= 1.0

    return run, check, (S1, S2)


def pcr_victim(where):
    def run(ctx, shape):
        X, Y, w, Xn = pca_data(shape)
        inp = Inputs(where)
        fm = J.pcr(inp(X), inp(Y), inp(w), nlv=PCA_NLV, scal=True, ctx=ctx)
        return dict(fm=fm, predict=J.predict(fm, inp(Xn), nlv=PCA_NLV, ctx=ctx)), inp

    def check(out, shape):
        X, Y, w, Xn = pca_data(shape)
        p, a, fm = shape[1], PCA_NLV, out["fm"]
        ref = SPCA.np_pcr(X, Y, w, nlv=a, scal=True)
        assert np.allclose(fm.ymeans, ref["ymeans"], rtol=1e-12)
        eig = ref["fm_pca"]["sv"] ** 2
        cb = TPCA._col_bounds(np.r_[eig, np.zeros(max(0, p - eig.size))], a)
        beta, xs = np.abs(ref["C"].T), ref["xscales"]
        B, _ = J.coef(fm, nlv=a)
        Br, _ = SPCA.np_pcr_coef(ref, a)
        tolB = np.maximum((cb[:a, None] * beta[:a]).sum(axis=0), 1e-9 * np.linalg.norm(xs[:, None] * Br, axis=0))   # test_pcr_coef_and_predict
        assert np.all(np.linalg.norm(xs[:, None] * (B - Br), axis=0) <= tolB)
        prr = SPCA.np_pcr_predict(ref, Xn, a)
        XnF = np.linalg.norm((Xn - ref["xmeans"]) / xs)
        assert np.all(np.linalg.norm(host(out["predict"]) - prr, axis=0) <= tolB * XnF + 1e-12 * np.linalg.norm(prr, axis=0))

    return run, check, (S1, S2)


# ---------------------------------------------------------------------------------- snv, detrend, savgol, mavg, fdif
def preproc_victim(fn, where):
    kw = dict(snv={}, detrend=dict(pol=1), savgol=dict(f=21, pol=3, d=2), mavg=dict(f=11), fdif=dict(f=2))[fn]

    def run(ctx, shape):
        X = SPRE.spectra(shape[0], shape[1], 1000 * shape[0] + shape[1])
        inp = Inputs(where)
        return getattr(J, fn)(inp(X), ctx=ctx, **kw), inp

    def check(out, shape):
        p = shape[1]
        X, got = SPRE.spectra(shape[0], p, 1000 * shape[0] + p), host(out)
        if fn == "snv":
            ref = SPRE.np_snv(X, True, True)
            TPRE._check(fn, got, ref, TPRE._snv_bound(X, ref))
        elif fn == "detrend":
            ref = SPRE.np_detrend(X, 1)
            TPRE._check(fn, got, ref, TPRE._detrend_bound(X, ref, 1))
        elif fn == "savgol":
            taps, lo = TPRE._savgol_taps(21, 3, 2)
            TPRE._check(fn, got, SPRE.np_savgol(X, 21, 3, 2), TPRE._fir_bound(X, taps, lo, p))
        elif fn == "mavg":
            TPRE._check(fn, got, SPRE.np_mavg(X, 11), TPRE._fir_bound(X, np.full(11, 1.0 / 11), 1 - ((11 + 1) >> 1), p))
        else:
            assert np.array_equal(got, SPRE.np_fdif(X, 2))

    return run, check, (S1, S2)


# ---------------------------------------------------------------------------------- occsd, occod, occsdod, stah, occstah, colmad
OCC_NLV = 5


@lru_cache(maxsize=None)
def occ_like(shape):
    """test_occ_static.occ_data at another shape: rank-8 spectra at level 10, 150 new rows, the last 10 shifted by 5 sd."""
    n, p, _ = shape
    rng = np.random.default_rng(SOCC.OCC_SEED + n)
    r = 8
    V = np.linalg.qr(rng.standard_normal((p, r)))[0]
    s = 0.8 ** np.arange(r)
    off = 10.0 + rng.standard_normal(p)

    def rows(m):
        H = rng.standard_normal((m, r)) * s
        sig = H @ V.T
        return sig + 1e-2 * sig.std() * rng.standard_normal((m, p)) + off, H

    X, H = rows(n)
    Xnew, _ = rows(150)
    Xnew[-10:] += 5 * X.std(axis=0)
    Y = H[:, :2] @ np.array([[1.0, 0.3], [-0.5, 1.0]]) + 0.01 * rng.standard_normal((n, 2))
    return np.asfortranarray(X), np.asfortranarray(Y), np.asfortranarray(Xnew)


def occ_victim(kind, where):
    def run(ctx, shape):
        X, Y, Xnew = occ_like(shape)
        inp = Inputs(where)
        Xi, Xq = inp(X), inp(Xnew)
        if kind == "occsd":
            fm = J.pcasvd(Xi, nlv=OCC_NLV, ctx=ctx)
            obj = J.occsd(fm, typc="mad", ctx=ctx)
        elif kind == "occod":
            fm = J.plskern(Xi, inp(Y), nlv=OCC_NLV, ctx=ctx)
            obj = J.occod(fm, Xi, typc="q", ctx=ctx)
        else:
            fm = J.plskern(Xi, inp(Y), nlv=OCC_NLV, scal=True, ctx=ctx)
            obj = J.occsdod(fm, Xi, nlv_sd=3, nlv_od=OCC_NLV, typc="mad", ctx=ctx)
        return dict(obj=obj, pred=J.occ_predict(obj, Xq, ctx=ctx)), inp

    def check(out, shape):
        X, _, Xnew = occ_like(shape)
        obj, gp = out["obj"], out["pred"]
        fm = obj.fm_sd.fm if kind == "occsdod" else obj.fm
        arr = dict(T=host(fm.T), P=np.asarray(fm.P), R=np.asarray(fm.P if kind == "occsd" else fm.R), xmeans=np.asarray(fm.xmeans), xscales=np.asarray(fm.xscales))
        if kind == "occsd":
            ref = SOCC.np_occsd(arr["T"], None, "mad")
            rp = SOCC.np_occsd_predict(ref, SOCC.np_transform(arr, Xnew, ref["nlv"]))
            assert np.max(np.abs(obj.Sinv - ref["Sinv"])) <= 1e-9 * np.abs(ref["Sinv"]).max()
        elif kind == "occod":
            ref = SOCC.np_occod(arr, X, None, "q")
            rp = SOCC.np_occod_predict(ref, Xnew)
        else:
            ref = SOCC.np_occsdod(arr, X, 3, OCC_NLV, "mad")
            rp = SOCC.np_occsdod_predict(ref, Xnew)
            for sfx, sub in (("_sd", "fm_sd"), ("_od", "fm_od")):
                TOCC._check_table(obj.d, ref["d"], ref[sub]["dtrain"], sfx)
                TOCC._check_table(gp.d, rp["d"], ref[sub]["dtrain"], sfx)
            TOCC._close(obj.d["dstand"], ref["d"]["dstand"], 2e-9, "dstand")
            TOCC._close(gp.d["dstand"], rp["d"]["dstand"], 2e-9, "dstand")
            TOCC._check_pred(gp.pred, rp["pred"], rp["d"]["dstand"])
            return
        TOCC._close(np.array([obj.cutoff]), np.array([ref["cutoff"]]), 1e-9, "cutoff")
        TOCC._check_table(obj.d, ref["d"], ref["dtrain"])
        TOCC._check_table(gp.d, rp["d"], ref["dtrain"])
        TOCC._check_pred(gp.pred, rp["pred"], rp["d"]["dstand"])

    return run, check, (S1, S2)


STAH_A = 7


def stah_victim(kind, where):
    def run(ctx, shape):
        X, _, Xnew = occ_like(shape)
        P = SSTAH.stah_P(shape[1], STAH_A)
        inp = Inputs(where)
        if kind == "colmad":
            return J.col_median_mad(inp(X), ctx=ctx), inp
        if kind == "stah":
            return J.stah(inp(X), STAH_A, scal=True, P=P, ctx=ctx), inp
        obj = J.occstah(inp(X), a=STAH_A, typc="mad", scal=True, P=P, ctx=ctx)
        return dict(obj=obj, pred=J.occ_predict(obj, inp(Xnew), ctx=ctx)), inp

    def check(out, shape):
        X, _, Xnew = occ_like(shape)
        P = SSTAH.stah_P(shape[1], STAH_A)
        if kind == "colmad":
            assert np.array_equal(host(out[0]), SSTAH.np_colmed(X)) and np.array_equal(host(out[1]), SSTAH.np_colmad(X))   # exact order statistics
            return
        got = out if kind == "stah" else out["obj"].res_stah
        ref = SSTAH.np_stah(X, P, True)
        assert np.array_equal(got.mu_scal, ref["mu_scal"]) and np.array_equal(got.s_scal, ref["s_scal"])
        TSTAH._near(got.mu, ref["mu"], "mu"); TSTAH._near(got.s, ref["s"], "s"); TSTAH._near(got.d, ref["d"], "d")
        if kind == "occstah":
            robj = SSTAH.np_occstah(X, P, "mad", scal=True)
            obj, gp, rp = out["obj"], out["pred"], SSTAH.np_occstah_predict(robj, Xnew)
            TSTAH._near(np.array([obj.cutoff]), np.array([robj["cutoff"]]), "cutoff")
            TSTAH._near(obj.d["dstand"], robj["d"]["dstand"], "dstand")
            TSTAH._near(gp.d["d"], rp["d"]["d"], "predicted d"); TSTAH._near(gp.d["dstand"], rp["d"]["dstand"], "predicted dstand")
            keep = SSTAH.stah_comparable_rows(rp["d"]["dstand"], rp["d"]["d"], robj["dtrain"], False)
            assert (~keep).mean() <= 0.01 and np.array_equal(host(gp.pred)[keep], rp["pred"][keep])

    return run, check, (S1, S2)


# ---------------------------------------------------------------------------------- sampks, sampdp (first shape only)
def samp_victim(kind, where):
    k = 200 if kind == "sampks" else 100

    def run(ctx, shape):
        inp = Inputs(where)
        return getattr(J, kind)(inp(SSAMP.uniform(shape[0], shape[1])), k, metric="eucl", ctx=ctx), inp

    def check(out, shape):
        X = SSAMP.uniform(shape[0], shape[1])
        if kind == "sampks":
            assert np.array_equal(out.train, SSAMP.np_sampks(X, k, "eucl")[0][:k])
        else:
            s1, s2, _ = SSAMP.np_sampdp(X, k, "eucl")
            assert np.array_equal(out.train, s1[:k]) and np.array_equal(out.test, s2[:k])

    return run, check, (S1,)


# ---------------------------------------------------------------------------------- the victims
FAMILIES = {name: pls_victim(name) for name in PLS}
FAMILIES.update({
    "accessors_host": accessor_victim("host"), "accessors_dev": accessor_victim("device"), "gridscorelv": gridscorelv_victim(),
    "lwplsr_pspace": lwplsr_victim("0", "host"), "lwplsr_kspace": lwplsr_victim("2", "host"), "lwplsr_kspace_dev": lwplsr_victim("2", "device"),
    "dkplsr": dkplsr_victim("host"), "dkplsr_dev": dkplsr_victim("device"), "kplsr": kplsr_victim("host"), "kplsr_dev": kplsr_victim("device"),
    "kpca": kpca_victim("host"), "kpca_dev": kpca_victim("device"), "krr": krr_victim("host"), "krr_dev": krr_victim("device"),
    "covsel": covsel_victim("host", False), "covsel_dev": covsel_victim("device", False), "covselr": covsel_victim("host", True),
    "pcasvd": pca_victim("pcasvd", "host"), "pcaeigen": pca_victim("pcaeigen", "device"), "pcr": pcr_victim("host"), "pcr_dev": pcr_victim("device"),
    "snv": preproc_victim("snv", "host"), "detrend": preproc_victim("detrend", "device"), "savgol": preproc_victim("savgol", "host"),
    "mavg": preproc_victim("mavg", "device"), "fdif": preproc_victim("fdif", "host"),
    "occsd": occ_victim("occsd", "host"), "occod": occ_victim("occod", "device"), "occsdod": occ_victim("occsdod", "host"),
    "stah": stah_victim("stah", "host"), "occstah": stah_victim("occstah", "device"), "colmad": stah_victim("colmad", "host"),
    "sampks": samp_victim("sampks", "host"), "sampdp": samp_victim("sampdp", "device"),
})
VICTIMS = [(name, shape) for name, (_, _, shapes) in FAMILIES.items() for shape in shapes]
VICTIM_IDS = [f"{name}-{shape[0]}x{shape[1]}x{shape[2]}" for name, shape in VICTIMS]
KEPT = {}       # victim -> (flat result of the first fresh run, paths on which the two fresh runs differ)


def run_victim(name, shape, ctx):
    run, _, _ = FAMILIES[name]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out, inp = run(ctx, shape)
    inp.unchanged()
    return out


def fresh_pair(name, shape):
    """Runs (1) and (2): two fresh ctxs; (1) is held against the family's CPU reference.  Computed once and kept."""
    key = (name, shape)
    if key not in KEPT:
        c1, c2 = J.Context(0), J.Context(0)
        try:
            out1 = run_victim(name, shape, c1)
            f1, f2 = flat(out1), flat(run_victim(name, shape, c2))
        finally:
            c1.close(); c2.close()
        FAMILIES[name][1](out1, shape)
        KEPT[key] = (f1, differing(f1, f2))
    return KEPT[key]


def check_on_used_ctx(name, shape, ctx):
    f1, loose = fresh_pair(name, shape)
    if loose:
        print(f"{name} {shape}: two fresh runs differ in {loose}")
        assert name in NOT_BYTE_REPRODUCIBLE, f"two fresh runs of {name} differ in {loose}; the cause belongs in the module's table"
    out3 = run_victim(name, shape, ctx)
    f3 = flat(out3)
    bad = [k for k in differing(f1, f3) if k not in loose]
    assert not bad, f"{name} {shape}: on a used ctx {bad} differ from the fresh run (which two fresh ctxs reproduce to the byte)"
    if loose:
        FAMILIES[name][1](out3, shape)


# ---------------------------------------------------------------------------------- the polluter
PN, PP, PPC, PQ = 1400, 2100, 600, 16     # rows; columns where the entry takes them; columns under JCH_SWEEP_MAXP; responses (= qpad)


def big(seed, n, p):
    """Finite and large: uniform values times 2^40 plus an offset."""
    return np.asfortranarray((CO.fill_uniform(seed, n, p) - 0.25) * 2.0 ** 40 + 2.0 ** 38)


def pollute(ctx):
    """One call of every family on `ctx`, each larger in every dimension than any victim; returns the calls that raised."""
    failed = []
    Xw, Xc = big(901, PN, PP), big(902, PN, PPC)
    Y = np.asfortranarray(Xc[:, :PQ] * 3.0 + big(903, PN, PQ))
    w = CO.fill_uniform(904, PN, 1)[:, 0] + 0.1
    Xq = big(905, 700, PPC)
    dv = lambda a: put(a, "device")
    gam = 2.0 ** -90

    def call(label, fn):
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                return fn()
        except Exception as e:   # noqa: BLE001  (reported by test_the_polluter_ran_every_family)
            failed.append((label, repr(e)))
            return None

    for fn, kw in (("plskern", dict()), ("plskern", dict(scal=True)), ("plskern", dict(variant=1)), ("plsnipals", dict()), ("plssimp", dict()),
                   ("plsrosa", dict()), ("plswold", dict(maxit=5))):
        f = getattr(J, fn)
        if not kw.get("variant"):    # (algorithm #2 takes p <= 2048 only)
            call(fn + " wide host", lambda: f(Xw, Y, w, nlv=6, ctx=ctx, **kw))
        call(fn + " device", lambda: f(dv(Xc), dv(Y), dv(w), nlv=6, ctx=ctx, **kw))
        call(fn + " q4 host", lambda: f(Xc, Y[:, :4], nlv=6, ctx=ctx, **kw))
    call("plskern bf16", lambda: J.plskern(put(Xc, "device", torch.bfloat16), put(Y, "device", torch.bfloat16), nlv=6, ctx=ctx))
    call("plskern bf16 wide", lambda: J.plskern(put(Xw, "device", torch.bfloat16), put(Y, "device", torch.bfloat16), dv(w), nlv=6, ctx=ctx))
    fm = call("model", lambda: J.plskern(Xw, Y, w, nlv=6, scal=True, ctx=ctx))
    if fm is not None:
        Xn = big(906, 900, PP)
        call("transform host", lambda: J.transform(fm, Xn, ctx=ctx))
        call("predict device", lambda: J.predict(fm, dv(Xn), nlv=range(0, 7), ctx=ctx))
        call("gridscorelv", lambda: J.gridscorelv(Xw, Y, Xn, Xn[:, :PQ].copy(order="F"), score=J.rmsep, fun=J.plskern, nlv=range(0, 7), ctx=ctx))
    for ks in ("0", "2"):
        for where in ("host", "device"):
            def lw():
                with env(JCH_LOCW_KSPACE=ks):
                    m = J.lwplsr(put(Xc, where), put(Y, where), nlvdis=6, metric="mahal", h=2.0, k=100, nlv=6, ctx=ctx)
                    J.predict(m, put(Xq, where), nlv=range(0, 7), ctx=ctx)
                    J.predict(m, put(Xq[:300], where), ctx=ctx)
            call(f"lwplsr kspace={ks} {where}", lw)
    kk = dict(kern="krbf", gamma=gam)
    Xk = big(907, 300, PP)
    m = call("dkplsr", lambda: J.dkplsr(Xw, Y, w, nlv=6, scal=True, ctx=ctx, **kk))
    if m is not None:
        call("dkplsr predict", lambda: J.predict(m, dv(Xk) if torch.is_tensor(m.X) else Xk, ctx=ctx))
    m2 = call("kplsr", lambda: J.kplsr(dv(Xw), dv(Y), dv(w), nlv=6, maxit=5, ctx=ctx, **kk))
    if m2 is not None:
        call("kplsr predict", lambda: J.predict(m2, dv(Xk), ctx=ctx))
    m3 = call("kpca", lambda: J.kpca(Xw, w, nlv=6, eig_maxit=5, ctx=ctx, **kk))
    if m3 is not None:
        call("kpca transform", lambda: J.kpca_transform(m3, Xk, ctx=ctx))
    m4 = call("krr", lambda: J.krr(dv(Xw), dv(Y), dv(w), lb=0.1, ctx=ctx, **kk))
    if m4 is not None:
        call("krr predict", lambda: J.krr_predict(m4, dv(Xk), lb=[0.1, 0.01], ctx=ctx))
    call("covsel", lambda: J.covsel(Xw, Y, nlv=10, ctx=ctx))
    call("covselr", lambda: J.covselr(dv(Xw), dv(Y), 10, "cor", ctx=ctx))
    m5 = call("pcasvd", lambda: J.pcasvd(Xw, w, nlv=8, eig_maxit=5, ctx=ctx))
    call("pcaeigen", lambda: J.pcaeigen(dv(Xw), nlv=8, scal=True, eig_maxit=5, ctx=ctx))
    call("pcr", lambda: J.pcr(Xw, Y, w, nlv=8, eig_maxit=5, ctx=ctx))
    for where in ("host", "device"):
        call("snv " + where, lambda: J.snv(put(Xw, where), ctx=ctx))
        call("detrend " + where, lambda: J.detrend(put(Xw, where), pol=2, ctx=ctx))
        call("savgol " + where, lambda: J.savgol(put(Xw, where), f=71, pol=3, d=1, ctx=ctx))
        call("mavg " + where, lambda: J.mavg(put(Xw, where), f=11, ctx=ctx))
        call("fdif " + where, lambda: J.fdif(put(Xw, where), f=5, ctx=ctx))
    if m5 is not None and fm is not None:
        for label, mk in (("occsd", lambda: J.occsd(m5, ctx=ctx)), ("occod", lambda: J.occod(fm, Xw, ctx=ctx)), ("occsdod", lambda: J.occsdod(fm, Xw, ctx=ctx))):
            o = call(label, mk)
            if o is not None:
                call(label + " predict", lambda: J.occ_predict(o, big(906, 900, PP), ctx=ctx))
    call("stah", lambda: J.stah(Xw, 130, seed=3, ctx=ctx))
    o = call("occstah", lambda: J.occstah(dv(Xw), a=130, seed=3, ctx=ctx))
    if o is not None:
        call("occstah predict", lambda: J.occ_predict(o, dv(Xk), ctx=ctx))
    call("colmad", lambda: J.colmad(Xw, ctx=ctx))
    call("sampks", lambda: J.sampks(Xw, 500, ctx=ctx))
    call("sampdp", lambda: J.sampdp(dv(Xw), 300, ctx=ctx))
    return failed


@pytest.fixture(scope="module")
def dirty_ctx():
    ctx = J.Context(0)
    ctx.polluter_failures = pollute(ctx)
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------------- Part A
def test_the_polluter_ran_every_family(dirty_ctx):
    assert not dirty_ctx.polluter_failures, dirty_ctx.polluter_failures


def test_the_table_of_entries_that_do_not_repeat_their_bits_is_short():
    assert set(NOT_BYTE_REPRODUCIBLE) <= set(FAMILIES) and len(NOT_BYTE_REPRODUCIBLE) <= len(FAMILIES) // 4


@pytest.mark.parametrize("name,shape", VICTIMS, ids=VICTIM_IDS)
def test_a_used_ctx_gives_the_bytes_of_a_fresh_one(name, shape, dirty_ctx):
    check_on_used_ctx(name, shape, dirty_ctx)


def test_every_family_behind_every_other_in_reverse_order(dirty_ctx):
    """By now every family has run on `dirty_ctx` at the small shapes; once more, backwards, against the results kept from the fresh runs."""
    for name, shape in reversed(VICTIMS):
        check_on_used_ctx(name, shape, dirty_ctx)


def test_the_two_buffers_of_the_reuse_state_are_reserved_through_their_helpers_only():
    """No writer of `xstage` or `xr` can forget to drop the copy: jch_reserve_xstage / jch_reserve_xr (jch_internal.h) are the only places
    that hand either buffer to jch_reserve."""
    import glob
    import re
    csrc = os.path.join(ROOT, "jchemo.jl_amd", "csrc")
    direct = re.compile(r"jch_reserve\s*\(\s*ctx\s*,\s*ctx->(xstage|xr)\b")
    hits = {os.path.basename(f): len(direct.findall(open(f).read())) for f in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))}
    assert {f: k for f, k in hits.items() if k} == {"jch_internal.h": 2}, hits


# ---------------------------------------------------------------------------------- Part B
NB, PB, QB = S1
NLVB = 6


@lru_cache(maxsize=None)
def reuse_data():
    X = CO.fill_uniform(431, NB, PB) + 2.0
    Y = X @ (CO.fill_uniform(432, PB, QB) - 0.5) + 0.1 * CO.fill_uniform(433, NB, QB)
    Y2 = Y[:, ::-1].copy() + 0.05 * CO.fill_uniform(434, NB, QB)
    w1 = CO.fill_uniform(435, NB, 1)[:, 0] + 0.1
    w2 = (CO.fill_uniform(436, NB, 1)[:, 0] > 0.2).astype(np.float64)
    return X, Y, Y2, w1, w2


THIRD = {"plskern": dict(), "plsrosa": dict(), "plssimp": dict(scal=True)}


@pytest.fixture(scope="module")
def lw_model():
    """A kNN-LWPLSR model per residency, trained on a ctx of its own, with enough queries for the slab scratch of the local fits to
    cover the staging copy of the fit's X (224 doubles per query at the least)."""
    m = max(128, -(-NB * PB // 224))
    X, Y, _ = lw_data((500, PB, 2))
    Xq = lw_data((500, PB, 2), m)[2]
    other = J.Context(0)
    out = {}
    for metric in ("mahal", "eucl"):    # (mahal: the mirror's own whitening runs jch_weighted_cov, which takes the working copy; eucl: nothing but the
        for where in ("host", "device"):    # handle's staging and the local fits touch the workspace)
            out[metric, where] = (J.lwplsr(put(X, where), put(Y, where), ctx=other, **dict(LW, metric=metric)), put(Xq, where))
    yield out
    other.close()


def same(a, b, tol=1e-10):
    """The criterion of test_gpu_parity.test_fit_from_the_previous_fits_row_major_copy."""
    s = O.sign_align(host(a.W), host(b.W))
    for f in FIELDS:
        assert O.rel_fro(host(getattr(a, f)), host(getattr(b, f)) * s) < tol, f
    e = O.rel_fro(a.xmeans, b.xmeans)
    print(f"xmeans: rel. error against the fresh fit {e:.3e}")
    assert e < 1e-13 and O.rel_fro(a.ymeans, b.ymeans) < 1e-13


def reuse_sequence(where, intervener, third="plskern", X=None):
    Xm, Y, Y2, w1, w2 = reuse_data()
    Xm = Xm if X is None else X
    ctx, fresh = J.Context(0), J.Context(0)
    try:
        Xi, Yi, Y2i, w1i, w2i = (put(a, where) for a in (Xm, Y, Y2, w1, w2))
        before = intervener(ctx, Xi, "before")                     # (what an intervener wants in place before the first fit)
        J.plskern(Xi, Yi, w1i, nlv=NLVB, ctx=ctx)
        c0 = ctx.counter(4)
        intervener(ctx, Xi, before)
        fn = getattr(J, third)
        a = fn(Xi, Y2i, w2i, nlv=NLVB, ctx=ctx, reuse_x=True, **THIRD[third])
        b = fn(Xi, Y2i, w2i, nlv=NLVB, ctx=fresh, **THIRD[third])
        same(a, b)
        ref = getattr(O, third)(host(Xi), Y2, w2, nlv=NLVB, **THIRD[third])
        s = O.sign_align(ref.W, host(a.W))
        for f in FIELDS:
            assert O.rel_fro(getattr(ref, f), host(getattr(a, f)) * s) < 1e-8, (third, f)
        return ctx.counter(4) - c0
    finally:
        ctx.close(); fresh.close()


def victim_intervener(name):
    def go(ctx, Xi, state):
        if state != "before":
            run_victim(name, S1, ctx)
    return go


def lw_intervener(kspace, prepared, metric):
    def make(lw_model, where):
        model, Xq = lw_model[metric, where]

        def go(ctx, Xi, state):
            with env(JCH_LOCW_KSPACE=kspace):
                if state == "before":
                    if prepared:
                        J.lwplsr_predict(model, Xq[:3], ctx=ctx)    # builds the handle on this ctx
                    return None
                J.lwplsr_predict(model, Xq, ctx=ctx)                # one-shot: jch_lwplsr_prepare (host: stages Xtrain), then the local fits
        return go
    return make


def snv_in_place(ctx, Xi, state):
    if state != "before":
        J.snv_(Xi, cent=True, scal=False, ctx=ctx)


LW_INTERVENERS = {f"lwplsr_predict-{mt}-kspace{ks}-{'prepared' if pr else 'one_shot'}": lw_intervener(ks, pr, mt)
                  for mt in ("mahal", "eucl") for ks in ("2", "0") for pr in (False, True)}
B_VICTIMS = [name for name, (_, _, shapes) in FAMILIES.items() if S1 in shapes]


@pytest.mark.parametrize("where", ["host", "device"])
def test_without_an_intervener_the_copy_is_used(where):
    """The control: the sequence of Part B does take the third fit from the copy when nothing runs in between."""
    for third in THIRD:
        assert reuse_sequence(where, lambda ctx, Xi, state: None, third) == 1, third


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name", B_VICTIMS)
def test_reuse_x_behind_one_call_of_a_family(name, where):
    reuse_sequence(where, victim_intervener(name))


LW_CASES = [(name, "plskern") for name in LW_INTERVENERS] + [(name, third) for name in LW_INTERVENERS if "kspace2" in name for third in ("plsrosa", "plssimp")]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("name,third", LW_CASES)
def test_reuse_x_behind_an_lwplsr_predict(name, third, where, lw_model):
    """The local fits of predict(::Lwplsr) take their slab scratch from the staging buffer of X, and jch_lwplsr_prepare stages a host
    Xtrain there: a host-array fit with reuse_x=True behind either must not take its pivot from what they left (plsrosa / plssimp as
    the third call: behind the two neighbour-space variants only).  Before both buffers were reserved through jch_reserve_xstage /
    jch_reserve_xr the eight host-array cases behind JCH_LOCW_KSPACE=2 failed with xmeans off by 0.37 ... 99 relative (a `mahal` model
    hid the one-shot case: its whitening goes through jch_weighted_cov, which takes the working copy and so drops it)."""
    reuse_sequence(where, LW_INTERVENERS[name](lw_model, where), third)


@pytest.mark.parametrize("where", ["host", "device"])
def test_reuse_x_behind_an_in_place_call_on_x_itself(where):
    """snv_ rewrites X (same pointer, new contents): the third fit and the fresh one both see the modified X."""
    X = np.array(reuse_data()[0]) * (1.0 + 0.5 * CO.fill_uniform(439, NB, 1))    # rows of different means, so that centring changes the fit
    reuse_sequence(where, snv_in_place, X=np.asfortranarray(X))
