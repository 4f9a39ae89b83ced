"""Literal numpy restatements of the reference's model-averaging sources on top of oracle.plsr_oracle: src/fweight.jl, src/wshenk.jl,
src/plsravg_unif.jl, src/plsravg_shenk.jl, src/plsravg_cv.jl, src/plsrstack.jl, src/plsrdaavg.jl / plsldaavg.jl / plsqdaavg.jl with
`findmax_cla` (src/utility.jl:564-570), and an extended-precision restatement of the nested residual sums of jch_row_resid_ss_lv.  Imported by
test_plsavg_static.py and test_gpu_plsavg.py; nothing here touches the library under test.  Indices and segments are 0-based."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import plsr_oracle as O  # noqa: E402

TYPW = ("bisquare", "cauchy", "epan", "fair", "invexp", "invexp2", "gauss", "trian", "tricube")


# ---------------------------------------------------------------------------------- src/fweight.jl:71-91
def np_fweight(d, typw="bisquare", alpha=0):
    d = np.abs(np.asarray(d, dtype=np.float64)).reshape(-1).copy()
    alpha = max(0, min(1, alpha))
    zd = d[np.isnan(d) == 0]
    q = np.quantile(zd, 1 - alpha)                                   # Julia's default quantile (type 7) = numpy's "linear"
    with np.errstate(divide="ignore", invalid="ignore"):
        d /= q
        if typw == "bisquare":
            w = (1 - d ** 2) ** 2
        if typw == "cauchy":
            w = 1 / (1 + d ** 2)
        if typw == "epan":
            w = 1 - d ** 2
        if typw == "fair":
            w = 1 / (1 + d) ** 2
        if typw == "invexp":
            w = np.exp(-d)
        if typw == "invexp2":
            w = np.exp(-d / 2)
        if typw == "gauss":
            w = np.exp(-d ** 2)
        if typw == "trian":
            w = 1 - d
        if typw == "tricube":
            w = (1 - d ** 3) ** 3
        w[d > 1] = 0
    w[np.isnan(w)] = 0
    return w


# ---------------------------------------------------------------------------------- src/wshenk.jl:46-75
def np_shenk_rss(fm, X, nlv=None):
    """(rss_r m x nlv, rss_b nlv) of :59-67: one `xresid` matrix and one `coef` per level."""
    X = O.ensure_mat(X)
    m, p = X.shape
    q = fm.C.shape[0]
    a = fm.T.shape[1]
    nlv = a if nlv is None else min(nlv, a)
    rss_r = np.empty((m, nlv)); rss_b = np.empty(nlv)
    for j in range(1, nlv + 1):
        E = O.xresid(fm, X, nlv=j)
        rss_r[:, j - 1] = np.sqrt(np.sum(E ** 2, axis=1))
        B, intercept = O.coef(fm, nlv=j)
        Bf = np.vstack([intercept.reshape(1, -1), B])
        rss_b[j - 1] = np.sqrt(np.sum(Bf ** 2) / q)
    return rss_r, rss_b


def np_wshenk(fm, X, nlv=None):
    rss_r, rss_b = np_shenk_rss(fm, X, nlv)
    m, nlv = rss_r.shape
    wb = O.mweight(1 / rss_b)
    w = np.empty((m, nlv)); wr = np.empty((m, nlv))
    for i in range(m):
        wr[i] = O.mweight(1 / rss_r[i])
        w[i] = O.mweight(wr[i] * wb)
    return dict(w=w, wr=wr, wb=wb)


# ---------------------------------------------------------------------------------- src/plsravg_*.jl, src/plsrstack.jl
def _range(nlv, n, p):
    """`eval(Meta.parse(nlv))`, then (min(minimum, n, p):min(maximum, n, p))."""
    parts = [int(s) for s in str(nlv).split(":")]
    lo, hi = parts[0], parts[-1]
    return list(range(min(lo, n, p), min(hi, n, p) + 1))


def _predlv(fm, X, rng):
    z = O.predict(fm, X, nlv=rng)
    return z if isinstance(z, list) else [z]


def np_plsravg_unif(X, Y, weights=None, *, nlv, scal=False):
    n, p = O.ensure_mat(X).shape
    rng = _range(nlv, n, p)
    return dict(fm=O.plskern(X, Y, weights, nlv=max(rng), scal=scal), nlv=rng)


def np_plsravg_unif_predict(obj, X):
    zpred = _predlv(obj["fm"], X, obj["nlv"])
    if len(zpred) == 1:
        return dict(pred=zpred[0], predlv=zpred)
    acc = zpred[0].copy()
    for z in zpred[1:]:
        acc += z
    return dict(pred=acc / len(zpred), predlv=zpred)


def np_plsravg_shenk(X, Y, weights=None, *, nlv, scal=False):
    n, p = O.ensure_mat(X).shape
    rng = _range(nlv, n, p)
    nlvmax = max(rng)
    rng = list(range(max(min(rng), 1), nlvmax + 1))
    return dict(fm=O.plskern(X, Y, weights, nlv=nlvmax, scal=scal), nlv=rng)


def np_plsravg_shenk_predict(obj, X):
    X = O.ensure_mat(X)
    m = X.shape[0]
    q = obj["fm"].C.shape[0]
    rng = obj["nlv"]
    zpred = _predlv(obj["fm"], X, rng)
    if len(rng) == 1:
        return dict(pred=zpred[0], predlv=zpred, w=None)
    pred = np.empty((m, q))
    w = np_wshenk(obj["fm"], X)["w"][:, np.asarray(rng) - 1]
    for i in range(m):
        zw = O.mweight(w[i])
        acc = zw[0] * zpred[0][i]
        for j in range(1, len(rng)):
            acc = acc + zw[j] * zpred[j][i]
        pred[i] = acc
    return dict(pred=pred, predlv=zpred, w=w)


def np_plsravg_cv(X, Y, weights=None, *, nlv, segm, typw="bisquare", alpha=0, scal=False):
    """src/plsravg_cv.jl:10-26 with the segments handed in (the reference draws segmkf(n, 2; rep = 1))."""
    X = O.ensure_mat(X); Y = O.ensure_mat(Y)
    n, p = X.shape
    rng = _range(nlv, n, p)
    nlvmax = max(rng)
    _, res, _ = O.gridcvlv(X, Y, segm=segm, score=O.rmsep, fun=O.plskern, nlv=range(0, nlvmax + 1), pars=O.mpar(scal=scal))
    z = res.mean(axis=1)
    d = (z - z.min())[np.asarray(rng)]
    w = O.mweight(np_fweight(d, typw=typw, alpha=alpha))
    return dict(fm=O.plskern(X, Y, weights, nlv=nlvmax, scal=scal), nlv=rng, w=w)


def np_plsrstack(X, y, weights=None, *, nlv, segm, scal=False):
    """src/plsrstack.jl:7-55 with the segments handed in (the reference draws segmkf(n, K; rep))."""
    X = O.ensure_mat(X); y = O.ensure_mat(y)
    n, p = X.shape
    weights = O.mweight(np.ones(n) if weights is None else weights)
    rng = _range(nlv, n, p)
    nlvmax = max(rng)
    Xs, ys, ws = [], [], []
    for listsegm in segm:
        for s in listsegm:
            s = np.asarray(s)
            zfm = O.plskern(O.rmrow(X, s), O.rmrow(y, s), O.rmrow(weights, s), nlv=nlvmax, scal=scal)
            Xs.append(np.hstack(O.predict(zfm, X[s], nlv=range(0, nlvmax + 1))))
            ys.append(y[s]); ws.append(weights[s])
    Xstack, ystack = np.vstack(Xs), np.vstack(ys)
    wstack = O.mweight(np.concatenate(ws))
    Xstack = Xstack[:, np.asarray(rng)]
    XtD = Xstack.T @ np.diag(wstack)
    L = np.linalg.cholesky(XtD @ Xstack)
    w = np.linalg.solve(L.T, np.linalg.solve(L, XtD @ ystack)).reshape(-1)
    return dict(fm=O.plskern(X, y, weights, nlv=nlvmax, scal=scal), nlv=rng, w=w, Xstack=Xstack, ystack=ystack, weightsstack=wstack)


def np_plsravg_cri_predict(obj, X):
    """src/plsravg_aic.jl:46-60 (PlsravgCri and Plsrstack)."""
    zpred = _predlv(obj["fm"], X, obj["nlv"])
    if len(zpred) == 1:
        return dict(pred=zpred[0], predlv=zpred)
    acc = obj["w"][0] * zpred[0].copy()
    for i in range(1, len(zpred)):
        acc += obj["w"][i] * zpred[i]
    return dict(pred=acc, predlv=zpred)


# ---------------------------------------------------------------------------------- src/plsrdaavg.jl, plsldaavg.jl, plsqdaavg.jl
def np_findmax_cla(x, weights=None):
    """src/utility.jl:564-570: `aggstat` sums the weights per (sorted) label, `argmax` takes the first maximum."""
    x = np.asarray(x).reshape(-1)
    weights = np.ones(len(x)) if weights is None else np.asarray(weights)
    lev = np.unique(x)
    tot = np.array([weights[x == l].sum() for l in lev])
    return lev[np.argmax(tot)], lev, tot


def np_plsdaavg(kind, X, y, weights=None, *, nlv, scal=False):
    n, p = O.ensure_mat(X).shape
    parts = [int(s) for s in str(nlv).split(":")]
    nlvmax = parts[-1]
    rng = list(range(max(parts[0], 0), min(nlvmax, n, p) + 1))
    w_mod = O.mweight(np.ones(nlvmax + 1)[np.asarray(rng)])
    fit = dict(rda=O.plsrda, lda=O.plslda, qda=O.plsqda)[kind]
    return dict(kind=kind, fm=fit(X, y, weights, nlv=nlvmax, scal=scal), nlv=rng, w_mod=w_mod)


def np_plsdaavg_predict(obj, X):
    """src/plsrdaavg.jl:80-97; also returns, per row, the two largest vote totals (what the GPU tests' tie exclusion reads)."""
    one = O.plsrda_predict if obj["kind"] == "rda" else O.plslda_predict
    zpred = one(obj["fm"], X, nlv=obj["nlv"])[0]
    if len(obj["nlv"]) == 1:
        return dict(pred=zpred, predlv=[zpred], top2=None)
    z = np.hstack(zpred)
    m = z.shape[0]
    pred = np.empty((m, 1), dtype=z.dtype); top2 = np.zeros((m, 2))
    for i in range(m):
        pred[i, 0], _, tot = np_findmax_cla(z[i], obj["w_mod"])
        srt = np.sort(tot)[::-1]
        top2[i, :min(2, len(srt))] = srt[:2]
    return dict(pred=pred, predlv=zpred, top2=top2)


# ---------------------------------------------------------------------------------- the nested residual sums
def resid_ss_lv_longdouble(X, shift, Z, B, a_lo, a_hi):
    """out[i, a - a_lo] = sum_j (X[i, j] - shift[j] - sum_{l < a} Z[i, l] B[j, l])^2 in extended precision, each level from scratch."""
    X = np.asarray(X, dtype=np.longdouble)
    E0 = X - (0 if shift is None else np.asarray(shift, dtype=np.longdouble))
    out = np.empty((X.shape[0], a_hi - a_lo + 1), dtype=np.longdouble)
    for a in range(a_lo, a_hi + 1):
        E = E0
        if a:
            E = E0 - np.asarray(Z[:, :a], dtype=np.longdouble) @ np.asarray(B[:, :a], dtype=np.longdouble).T
        out[:, a - a_lo] = np.sum(E * E, axis=1)
    return out


def resid_ss_lv_running_f64(X, shift, Z, B, a_lo, a_hi):
    """The kernel's order in float64: per element e_0 = x - shift, e_a = fma(-z_a, b_a, e_(a-1)) and per level the row sum in column order with
    fused squares.  numpy has no fma: the products are formed exactly in longdouble (64-bit mantissa holds a 53 x 53-bit product's leading
    bits to within one rounding of the fused result's argument), which is inside the bound's own slack; this is an evaluation of the ORDER."""
    X = np.asarray(X, dtype=np.float64)
    m, p = X.shape
    sh = np.zeros(p) if shift is None else np.asarray(shift, dtype=np.float64)
    out = np.zeros((m, a_hi - a_lo + 1))
    for j in range(p):
        e = X[:, j] - sh[j]
        for a in range(0, a_hi + 1):
            if a:
                e = np.asarray(np.asarray(e, dtype=np.longdouble) - np.asarray(Z[:, a - 1], dtype=np.longdouble) * np.longdouble(B[j, a - 1]),
                               dtype=np.float64)
            if a >= a_lo:
                out[:, a - a_lo] = np.asarray(np.asarray(out[:, a - a_lo], dtype=np.longdouble) + np.asarray(e, dtype=np.longdouble) ** 2,
                                              dtype=np.float64)
    return out


# ---------------------------------------------------------------------------------- src/locw.jl driving the local models
def np_local_lists(X, Yspace, Xq, *, nlvdis, metric, h, k, tol=1e-4, scal=False):
    """The search and the weights of src/lwplsravg.jl:124-143 / src/lwplsrdaavg.jl:119-138 (Yspace: Y, or dummy(y) for the DA models)."""
    r = O.lwplsr_predict(O.lwplsr(X, Yspace, nlvdis=nlvdis, metric=metric, h=h, k=k, nlv=0, tol=tol, scal=scal), Xq, nlv=0)
    return r["listnn"], r["listd"], r["listw"]


def np_locw(Xtrain, Ytrain, Xq, listnn, listw, fit_predict):
    """src/locw.jl:21-52: per query the model on its neighbourhood, or the common value of a constant univariate y.  fit_predict(i, Xs, Ys, w, x)
    returns the q predictions (or the label) for the 1 x p query x.  Also returns which rows took the constant shortcut."""
    Xtrain = O.ensure_mat(Xtrain); Ytrain = O.ensure_mat(Ytrain); Xq = O.ensure_mat(Xq)
    m, q = Xq.shape[0], Ytrain.shape[1]
    pred = np.empty((m, q), dtype=Ytrain.dtype)
    const = np.zeros(m, dtype=bool)
    extra = [None] * m
    for i in range(m):
        s = np.asarray(listnn[i])
        zY = Ytrain[s, :]
        if q == 1 and len(np.unique(zY)) == 1:
            pred[i, :] = zY[0, 0]; const[i] = True
            continue
        pred[i, :], extra[i] = fit_predict(i, Xtrain[s, :], zY, listw[i], Xq[i:i + 1, :])
    return pred, const, extra


def np_lwplsravg_predict(X, Y, Xq, *, nlvdis, metric, h, k, nlv, typf="unif", typw="bisquare", alpha=0, tol=1e-4, scal=False, segm_of=None):
    """src/lwplsravg.jl:120-150 with fun = plsravg; segm_of(i): the segments of query i for typf = "cv" / "stack"."""
    listnn, listd, listw = np_local_lists(X, Y, Xq, nlvdis=nlvdis, metric=metric, h=h, k=k, tol=tol, scal=scal)

    def one(i, Xs, Ys, w, x):
        if typf == "unif":
            r = np_plsravg_unif_predict(np_plsravg_unif(Xs, Ys, w, nlv=nlv, scal=scal), x)
        elif typf == "shenk":
            r = np_plsravg_shenk_predict(np_plsravg_shenk(Xs, Ys, w, nlv=nlv, scal=scal), x)
        elif typf == "cv":
            r = np_plsravg_cri_predict(np_plsravg_cv(Xs, Ys, w, nlv=nlv, segm=segm_of(i), typw=typw, alpha=alpha, scal=scal), x)
        else:
            r = np_plsravg_cri_predict(np_plsrstack(Xs, Ys, w, nlv=nlv, segm=segm_of(i), scal=scal), x)
        return r["pred"][0], len(r["predlv"])
    pred, const, nlev = np_locw(X, Y, Xq, listnn, listw, one)
    return dict(pred=pred, listnn=listnn, listd=listd, listw=listw, const=const, nlevels=nlev)


def np_lwplsdaavg_predict(kind, X, y, Xq, *, nlvdis, metric, h, k, nlv, tol=1e-4, scal=False):
    """src/lwplsrdaavg.jl:115-145 (lda / qda alike) with fun = plsrdaavg / plsldaavg / plsqdaavg.  bad[i]: the restatement could not fit query i's
    neighbourhood (a class covariance that is not positive definite); tie[i]: its two largest vote totals are equal."""
    y = np.asarray(y).reshape(-1)
    listnn, listd, listw = np_local_lists(X, O.dummy(y)[0], Xq, nlvdis=nlvdis, metric=metric, h=h, k=k, tol=tol, scal=scal)
    m = O.ensure_mat(Xq).shape[0]
    bad = np.zeros(m, dtype=bool); tie = np.zeros(m, dtype=bool)

    def one(i, Xs, ys, w, x):
        try:
            r = np_plsdaavg_predict(np_plsdaavg(kind, Xs, ys[:, 0], w, nlv=nlv, scal=scal), x)
        except np.linalg.LinAlgError:
            bad[i] = True
            return ys[0, 0], None
        if r["top2"] is not None:
            tie[i] = r["top2"][0, 0] == r["top2"][0, 1]
        return r["pred"][0, 0], None
    pred, const, _ = np_locw(X, y.reshape(-1, 1), Xq, listnn, listw, one)
    return dict(pred=pred, listnn=listnn, const=const, bad=bad, tie=tie)


def np_lwplsravg_shenk_details(X, Y, Xq, *, nlvdis, metric, h, k, nlv, tol=1e-4, scal=False):
    """What a local shenk call is made of, per query, from the literal pieces: the clamped levels lo..hi (n = k), pred_lv (m, le, q), the weights wlv
    (m, le) of src/plsravg_shenk.jl:36-39 (wshenk's w over lo..hi, renormalised), rss_r and rss_b (m, hi) of src/wshenk.jl:59-67 on the local model,
    and pred.  Rows that take the constant-y shortcut are NaN in wlv / rss_r / rss_b."""
    X = O.ensure_mat(X); Y = O.ensure_mat(Y); Xq = O.ensure_mat(Xq)
    listnn, listd, listw = np_local_lists(X, Y, Xq, nlvdis=nlvdis, metric=metric, h=h, k=k, tol=tol, scal=scal)
    m, q = Xq.shape[0], Y.shape[1]
    kk = listnn.shape[1]
    rng = _range(nlv, kk, X.shape[1])
    lo, hi = max(min(rng), 1), max(rng)
    le = hi - lo + 1
    out = dict(pred=np.empty((m, q)), pred_lv=np.empty((m, le, q)), wlv=np.full((m, le), np.nan), rss_r=np.full((m, hi), np.nan),
               rss_b=np.full((m, hi), np.nan), const=np.zeros(m, dtype=bool), lo=lo, hi=hi, listnn=listnn)
    for i in range(m):
        s = listnn[i]
        zY = Y[s]
        if q == 1 and len(np.unique(zY)) == 1:
            out["pred"][i] = zY[0, 0]; out["pred_lv"][i] = zY[0, 0]; out["const"][i] = True
            continue
        obj = np_plsravg_shenk(X[s], zY, listw[i], nlv=nlv, scal=scal)
        r = np_plsravg_shenk_predict(obj, Xq[i:i + 1])
        out["pred"][i] = r["pred"][0]
        out["pred_lv"][i] = np.stack([z[0] for z in r["predlv"]])
        out["wlv"][i] = r["w"][0] / r["w"][0].sum() if le > 1 else 1.0
        rr, rb = np_shenk_rss(obj["fm"], Xq[i:i + 1])
        out["rss_r"][i], out["rss_b"][i] = rr[0], rb
    return out
