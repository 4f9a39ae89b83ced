"""Every family once from host arrays and once from device tensors, on seeded inputs, every output array into one .npz: the A/B record of a
change to the host plumbing (profiles/hostcall_frame_ab.json was made by running this file on two builds and comparing the two .npz files with
np.array_equal, array by array).  The families, their inputs and their shapes (S1 = 613 x 37 x 3) are those of tests/test_gpu_used_ctx.py; the
kNN, density, local-MLR, local-PLS-discrimination and permutation-importance families, which that file does not have, run here on inputs of the
same size (profiles/lwfamily_refactor_ab.json was made the same way).

    python tools/dump_host_entries.py OUT.npz          # the dump
    python tools/dump_host_entries.py --time           # host-mode timing probe: one JSON line, median of 5 after one warm-up

--time: jch_transform at 100 000 x 500 from a host array and jch_kde_dens at n = 16 384, m = 4 096, d = 8 from host arrays.
"""
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "jchemo.jl_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import jchemo_hip as J  # noqa: E402
from jchemo_hip import _lib  # noqa: E402
import test_gpu_used_ctx as U  # noqa: E402

S1 = U.S1


def knn_family(where):
    def run(ctx, shape):
        n, p, q = shape
        rng = np.random.default_rng(n + p)
        X, Xq = rng.standard_normal((n, p)), rng.standard_normal((67, p))
        Y = X[:, :q] + 0.1 * rng.standard_normal((n, q))
        y = (X[:, 0] > 0).astype(np.int64) + (X[:, 1] > 0.5)
        inp = U.Inputs(where)
        Xi, Qi = inp(X), inp(Xq)
        ind, d = J.getknn(Xi, Qi, k=5, ctx=ctx)
        mah = J.getknn(Xi, Qi, k=5, metric="mahal", ctx=ctx)
        fr = J.knnr(Xi, inp(Y), nlvdis=3, h=2.0, k=7, ctx=ctx)
        fd = J.knnda(Xi, y, h=2.0, k=7, ctx=ctx)
        oc = J.occknndis(Xi, nlv=3, nsamp=50, k=5, seed=1, ctx=ctx)
        ol = J.occlknndis(Xi, nlv=3, nsamp=50, k=5, seed=1, ctx=ctx)
        return dict(ind=ind, d=d, mahal=mah, knnr=J.knnr_predict(fr, Qi, ctx=ctx), knnda=J.knnda_predict(fd, Qi, ctx=ctx),
                    occknndis=J.occknn_predict(oc, Qi, ctx=ctx), occlknndis=J.occknn_predict(ol, Qi, ctx=ctx)), inp
    return run


def kde_family(where):
    def run(ctx, shape):
        n, p, _ = shape
        rng = np.random.default_rng(n + 2 * p)
        X, Xq = rng.standard_normal((n, 5)), rng.standard_normal((67, 5))
        y = (X[:, 0] > 0).astype(np.int64) + (X[:, 1] > 0.5)
        inp = U.Inputs(where)
        Xi, Qi = inp(X), inp(Xq)
        dm = J.dmkern(Xi, ctx=ctx)
        kd = J.kdeda(Xi, y, ctx=ctx)
        pk = J.plskdeda(Xi, y, nlv=3, ctx=ctx)
        return dict(dmkern=J.dmkern_predict(dm, Qi, ctx=ctx), kdeda=J.kdeda_predict(kd, Qi, ctx=ctx), plskdeda=J.plskdeda_predict(pk, Qi, ctx=ctx)), inp
    return run


def _class_data(shape, seed, m=67):
    n, p, _ = shape
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 3, n)
    cen = 2.0 * rng.standard_normal((3, p))
    return cen[y] + rng.standard_normal((n, p)), y.astype(np.int64), cen[rng.integers(0, 3, m)] + rng.standard_normal((m, p)), rng


def lwmlr_family(where):
    def run(ctx, shape):
        n, p, q = shape
        X, y, Xq, rng = _class_data(shape, n + 3 * p)
        X, Xq = X[:, :6], Xq[:, :6]                           # (a local MLR needs k > d)
        Y = X[:, :q] @ rng.standard_normal((q, q)) + 0.1 * rng.standard_normal((n, q))
        inp = U.Inputs(where)
        Xi, Yi, Qi = inp(X), inp(Y), inp(Xq)
        ind, _ = J.getknn(Xi, Qi, k=35, ctx=ctx)
        w = inp(rng.uniform(0.2, 1.0, (Xq.shape[0], 35)))
        pred, info = J.knn_wls(Xi, Yi, Qi, ind, w, info=True, ctx=ctx)
        fm = J.lwmlr(Xi, Yi, metric="mahal", h=2.0, k=35, ctx=ctx)
        fd = J.lwmlrda(Xi, y, h=2.0, k=35, ctx=ctx)
        return dict(knn_wls=pred, knn_wls_info=info, lwmlr=J.lwmlr_predict(fm, Qi, ctx=ctx), lwmlrda=J.lwmlrda_predict(fd, Qi, ctx=ctx)), inp
    return run


def lwplsda_family(where):
    def run(ctx, shape):
        n, p, _ = shape
        X, y, Xq, rng = _class_data(shape, n + 5 * p)
        inp = U.Inputs(where)
        Xi, Qi = inp(X), inp(Xq)
        out = {}
        for name, fit, pred, kw in (("lwplsrda", J.lwplsrda, J.lwplsrda_predict, {}), ("lwplslda", J.lwplslda, J.lwplslda_predict, dict(prior="prop")),
                                    ("lwplsqda", J.lwplsqda, J.lwplsqda_predict, dict(prior="unif"))):
            fm = fit(Xi, y, nlvdis=4, metric="mahal", h=2.0, k=60, nlv=3, ctx=ctx, **kw)
            out[name] = pred(fm, Qi, nlv=range(1, 4), ctx=ctx)
        m, k, a = 9, 40, 3
        T = np.ascontiguousarray(rng.standard_normal((m, k, a)))
        cls = rng.integers(0, 3, (m, k)).astype(np.int32)
        T += cls[:, :, None]
        tq = np.ascontiguousarray(rng.standard_normal((m, a)) + 1.0)
        if where == "device":
            import torch
            T, tq, cls = (torch.as_tensor(x, device="cuda:0") for x in (T, tq, cls))
        for kind in ("lda", "qda"):
            out[f"knn_gda_{kind}"] = J.knn_gda(T, tq, cls, 3, kind=kind, prior="prop", nlv=range(1, a + 1), ctx=ctx)
        return out, inp
    return run


def viperm_family(where):
    def run(ctx, shape):
        n, p, q = shape
        X, _, _, rng = _class_data(shape, n + 7 * p)
        Y = X[:, :q] @ rng.standard_normal((q, q)) + 0.1 * rng.standard_normal((n, q))
        inp = U.Inputs(where)
        return dict(viperm=J.viperm(inp(X), inp(Y), perm=1, score=J.rmsep, fun=J.plskern, seed=31, ctx=ctx, nlv=3)), inp
    return run


def families():
    """name -> run(ctx, shape), every family of the used-ctx test in both modes (its bf16 fit takes device inputs only)."""
    out = {}
    for where in ("host", "device"):
        for name, (fn, kw, use_w, _, bf16) in list(U.PLS.items()):
            if bf16 and where == "host":
                continue
            key = f"{name}@{where}"
            U.PLS[key] = (fn, kw, use_w, where, bf16)      # (pls_victim reads its row once, when it is called: the table is left as found)
            out[key] = U.pls_victim(key)[0]
            del U.PLS[key]
        made = dict(accessors=U.accessor_victim(where), lwplsr_pspace=U.lwplsr_victim("0", where), lwplsr_kspace=U.lwplsr_victim("2", where),
                    dkplsr=U.dkplsr_victim(where), kplsr=U.kplsr_victim(where), kpca=U.kpca_victim(where), krr=U.krr_victim(where),
                    covsel=U.covsel_victim(where, False), covselr=U.covsel_victim(where, True), pcasvd=U.pca_victim("pcasvd", where),
                    pcaeigen=U.pca_victim("pcaeigen", where), pcr=U.pcr_victim(where))
        made.update({fn: U.preproc_victim(fn, where) for fn in ("snv", "detrend", "savgol", "mavg", "fdif")})
        made.update({k: U.occ_victim(k, where) for k in ("occsd", "occod", "occsdod")})
        made.update({k: U.stah_victim(k, where) for k in ("stah", "occstah", "colmad")})
        made.update({k: U.samp_victim(k, where) for k in ("sampks", "sampdp")})
        out.update({f"{k}@{where}": v[0] for k, v in made.items()})
        out[f"knn@{where}"] = knn_family(where)
        out[f"kde@{where}"] = kde_family(where)
        out[f"lwmlr@{where}"] = lwmlr_family(where)
        out[f"lwplsda@{where}"] = lwplsda_family(where)
        out[f"viperm@{where}"] = viperm_family(where)
    out["gridscorelv@host"] = U.gridscorelv_victim()[0]
    return out


def dump(path):
    arrays = {}
    ctx = J.Context(0)
    for name, run in families().items():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res, inp = run(ctx, S1)
        inp.unchanged()
        for k, v in U.flat(res).items():
            arrays[f"{name}:{k}"] = v
        print(name, flush=True)
    ctx.close()
    np.savez(path, **arrays)
    print(f"{len(arrays)} arrays -> {path}")


def timing():
    def med(f):
        f()
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
        return dict(ms=ts, median_ms=float(np.median(ts)))
    ctx, lib = J.Context(0), _lib.load()
    rng = np.random.default_rng(1)
    m, p, k = 100_000, 500, 25
    X = np.asfortranarray(rng.standard_normal((m, p)))
    R = np.asfortranarray(rng.standard_normal((p, k)))
    T = np.empty((m, k), order="F")
    ptr = lambda a: a.ctypes.data if a is not None else None
    out = {}
    out["transform_host_100000x500"] = med(lambda: ctx.check(lib.jch_transform(ctx._h, _lib.LOC_HOST, ptr(X), m, p, m, None, None, ptr(R), k, ptr(T), m)))
    n, mq, d = 16_384, 4_096, 8
    Z, Xq = np.asfortranarray(rng.standard_normal((n, d))), np.asfortranarray(rng.standard_normal((mq, d)))
    cls = np.array([0, n // 2, n], dtype=np.int64)
    u, v2, coef, dims = np.ones((d, 2), order="F"), np.ones((1, 2), order="F"), np.ones((1, 2), order="F"), np.array([d], dtype=np.int32)
    out["kde_dens_host_16384x4096x8"] = med(lambda: J.kde_dens(Z, Xq, cls, u, v2, coef, dims, ctx=ctx))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--time":
        timing()
    elif len(sys.argv) == 2:
        dump(sys.argv[1])
    else:
        sys.exit(__doc__)
