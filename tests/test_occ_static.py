"""Static checks of the outlier-distance surface (occsd, occod, occsdod, jch_row_resid_ss): the literal numpy restatements of src/occsd.jl,
src/occod.jl, src/occsdod.jl and src/xfit.jl the GPU tests compare against, the folded forms the device route relies on, the cutoff statistics
against hand-computed values, the error bound of the row-residual kernel, and the header / Python / Julia surface.  No GPU needed."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_julia_wrapper import JL, header_protos  # noqa: E402
from test_pca_static import np_pcasvd  # noqa: E402

U = 2.0 ** -53   # unit roundoff of float64
MAD_CONSTANT = 1.4826022185056018   # StatsBase 0.33 / 0.34: mad(x) = 1.4826... * median(|x - median(x)|) (normalize = true is the default)


# ---------------------------------------------------------------------------------- numpy restatements of the reference
# A model is a dict of arrays as downloaded: T (n x a), P (p x a), R (p x a; a Pca has R = P), xmeans, xscales (p).
def np_transform(fm, X, nlv):
    """src/plskern.jl:187-195 / src/pcasvd.jl:110-115."""
    return (np.asarray(X, dtype=np.float64) - fm["xmeans"]) / fm["xscales"] @ fm["R"][:, :nlv]


def np_xfit(fm, X, nlv=None):
    """src/xfit.jl:37-56."""
    X = np.array(X, dtype=np.float64)
    a = fm["T"].shape[1]
    nlv = a if nlv is None else min(nlv, a)                               # :38-39
    if nlv == 0:
        X[:] = fm["xmeans"]                                               # :41-45
    else:
        X = np_transform(fm, X, nlv) @ fm["P"][:, :nlv].T                 # :47-48
        X = X * fm["xscales"]                                             # :50 scale!(X, 1 ./ xscales)
        X = X + fm["xmeans"]                                              # :52 center!(X, -xmeans)
    return X


def np_xresid(fm, X, nlv=None):
    """src/xfit.jl:93-98."""
    return np.asarray(X, dtype=np.float64) - np_xfit(fm, X, nlv)


def np_median(d):
    s = np.sort(np.asarray(d, dtype=np.float64))
    n = s.shape[0]
    return s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2


def np_mad(d):
    d = np.asarray(d, dtype=np.float64)
    return MAD_CONSTANT * np_median(np.abs(d - np_median(d)))


def np_quantile(d, q):
    """Julia's `quantile(v, q)` (Statistics `_quantile`, alpha = beta = 1: type 7)."""
    s = np.sort(np.asarray(d, dtype=np.float64))
    n = s.shape[0]
    h = (n - 1) * q                                                       # 0-based position n q + (1 - q) - 1
    lo = min(int(np.floor(h)), max(n - 2, 0))
    return s[lo] + (h - lo) * (s[min(lo + 1, n - 1)] - s[lo])


def np_cutoff(d, typc, cri, alpha):
    return np_median(d) + cri * np_mad(d) if typc == "mad" else np_quantile(d, 1 - alpha)   # src/occsd.jl:138-139


def np_pval(dtrain, q):
    """`pval(e_cdf, q)`: 1 - ecdf(dtrain)(q), counted literally."""
    dtrain, q = np.asarray(dtrain, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return 1.0 - (dtrain[None, :] <= q[:, None]).sum(axis=1) / dtrain.shape[0]


def _sd_table(T, Sinv, nlv, dtrain, cutoff):
    d2 = np.einsum("ij,jk,ik->i", T, Sinv, T)                             # mahsq(T, zeros(nlv)', Sinv)
    d = np.sqrt(d2)
    return dict(d=d, dstand=d / cutoff if cutoff is not None else None, pval=np_pval(d if dtrain is None else dtrain, d), gh=d2 / nlv)


def np_occsd(T, nlv=None, typc="mad", cri=3, alpha=.025):
    """src/occsd.jl:129-145 on the scores T."""
    a = T.shape[1]
    nlv = a if nlv is None else min(nlv, a)                               # :131-132
    Tk = T[:, :nlv]                                                       # :133
    S = np.cov(Tk, rowvar=False, bias=True).reshape(nlv, nlv)             # :134
    Linv = np.linalg.inv(np.linalg.cholesky(S))
    Sinv = Linv.T @ Linv                                                  # :135
    tab = _sd_table(Tk, Sinv, nlv, None, None)                            # :136-137
    cutoff = np_cutoff(tab["d"], typc, cri, alpha)                        # :138-139
    tab["dstand"] = tab["d"] / cutoff                                     # :142
    return dict(d=tab, Sinv=Sinv, dtrain=tab["d"], cutoff=cutoff, nlv=nlv)


def np_occsd_predict(obj, Tnew):
    """src/occsd.jl:153-164; Tnew = transform(object.fm, X; nlv)."""
    tab = _sd_table(Tnew[:, :obj["nlv"]], obj["Sinv"], obj["nlv"], obj["dtrain"], obj["cutoff"])
    return dict(pred=(tab["dstand"] > 1).astype(np.int64).reshape(-1, 1), d=tab)


def _od_d(fm, X, nlv):
    E = np_xresid(fm, X, nlv)                                             # src/occod.jl:48
    return np.sqrt(np.sum(E * E, axis=1))                                 # :49-50


def np_occod(fm, X, nlv=None, typc="mad", cri=3, alpha=.025):
    """src/occod.jl:43-57."""
    a = fm["T"].shape[1]
    nlv = a if nlv is None else min(nlv, a)
    d = _od_d(fm, X, nlv)
    cutoff = np_cutoff(d, typc, cri, alpha)
    return dict(d=dict(d=d, dstand=d / cutoff, pval=np_pval(d, d)), fm=fm, dtrain=d, cutoff=cutoff, nlv=nlv)


def np_occod_predict(obj, X):
    """src/occod.jl:65-75."""
    d = _od_d(obj["fm"], X, obj["nlv"])
    tab = dict(d=d, dstand=d / obj["cutoff"], pval=np_pval(obj["dtrain"], d))
    return dict(pred=(tab["dstand"] > 1).astype(np.int64).reshape(-1, 1), d=tab)


def _np_hcat(sd, od):
    tab = {k + "_sd": v for k, v in sd.items()}
    tab.update({k + "_od": v for k, v in od.items()})
    tab["dstand"] = np.sqrt(sd["dstand"] * od["dstand"])
    return tab


def np_occsdod(fm, X, nlv_sd=None, nlv_od=None, typc="mad", cri=3, alpha=.025):
    """src/occsdod.jl:35-52."""
    fm_sd = np_occsd(fm["T"], nlv_sd, typc, cri, alpha)
    fm_od = np_occod(fm, X, nlv_od, typc, cri, alpha)
    return dict(d=_np_hcat(fm_sd["d"], fm_od["d"]), fm_sd=fm_sd, fm_od=fm_od, fm=fm)


def np_occsdod_predict(obj, X):
    """src/occsdod.jl:60-74."""
    sd = np_occsd_predict(obj["fm_sd"], np_transform(obj["fm"], X, obj["fm_sd"]["nlv"]))["d"]
    od = np_occod_predict(obj["fm_od"], X)["d"]
    tab = _np_hcat(sd, od)
    return dict(pred=(tab["dstand"] > 1).astype(np.int64).reshape(-1, 1), d=tab)


def comparable_rows(dstand, d, dtrain):
    """The rows on which `pred` and `pval` are compared: the restated dstand further than 1e-7 from 1 and no OTHER training d within 1e-9 relative
    of the row's d (a row's own training value, an exact match, does not count)."""
    dtrain = np.asarray(dtrain)
    diff = np.abs(dtrain[None, :] - d[:, None])
    close = (diff <= 1e-9 * np.abs(d)[:, None]) & (diff > 0)
    return (np.abs(dstand - 1) > 1e-7) & ~close.any(axis=1)


# ---------------------------------------------------------------------------------- the data of the model tests (shared with test_gpu_occ.py)
OCC_N, OCC_P, OCC_NLV, OCC_M = 400, 60, 6, 150
OCC_SEED = 20240611


def occ_data(seed=OCC_SEED):
    """(X, Y, Xnew, weights): n = 400 rows of rank-8 spectra at level 10 plus noise with sd 1e-2 of the signal, so that the orthogonal distance stays
    above 1e-3 of |xc|; 150 new rows from the same population, the last 10 shifted by 5 sd in every column."""
    rng = np.random.default_rng(seed)
    r = 8
    V = np.linalg.qr(rng.standard_normal((OCC_P, r)))[0]
    s = 0.8 ** np.arange(r)
    off = 10.0 + rng.standard_normal(OCC_P)

    def rows(m):
        H = rng.standard_normal((m, r)) * s
        sig = H @ V.T
        return sig + 1e-2 * sig.std() * rng.standard_normal((m, OCC_P)) + off, H

    X, H = rows(OCC_N)
    Xnew, _ = rows(OCC_M)
    Xnew[-10:] += 5 * X.std(axis=0)
    Y = H[:, :2] @ np.array([[1.0, 0.3], [-0.5, 1.0]]) + 0.01 * rng.standard_normal((OCC_N, 2))
    w = rng.random(OCC_N) + 0.2
    return np.asfortranarray(X), np.asfortranarray(Y), np.asfortranarray(Xnew), w


def _model_from_pca(fm):
    return dict(T=fm["T"], P=fm["P"], R=fm["P"], xmeans=fm["xmeans"], xscales=fm["xscales"])


def _model_from_pls(fm):
    return dict(T=fm.T, P=fm.P, R=fm.R, xmeans=fm.xmeans, xscales=fm.xscales)


def _cpu_models():
    from oracle import plsr_oracle as O
    X, Y, Xnew, w = occ_data()
    return X, Xnew, {
        "pcasvd": _model_from_pca(np_pcasvd(X, None, nlv=OCC_NLV)),
        "plskern": _model_from_pls(O.plskern(X, Y, nlv=OCC_NLV)),
        "plskern_scal": _model_from_pls(O.plskern(X, Y, nlv=OCC_NLV, scal=True)),
        "plskern_w": _model_from_pls(O.plskern(X, Y, w, nlv=OCC_NLV)),
    }


# ---------------------------------------------------------------------------------- the row-residual kernel's reference and error bound
# (m, p, k): one element; around a wave tile (64 rows) and a column tile (16); one row into a second workgroup tile (4 waves x 64 rows); the cfg2
# width; coefficients beyond LDS (k = 5 pads to 16 rows, plus the row of shifts: 17 x 2064 doubles = 281 KB against 150 KB); k one above the
# register-held limit of 64
PRIM_SHAPES = [(1, 1, 0), (1, 1, 1), (63, 15, 3), (64, 16, 4), (65, 17, 5), (257, 33, 25), (300, 500, 25), (70, 2049, 5), (130, 40, 65)]


def prim_inputs(m, p, k, seed=None):
    """X = shift + Z B' + 0.01 noise at level 100 (k = 0: shift + noise), so that the residual is what is left of a cancellation."""
    rng = np.random.default_rng(1000 * m + 10 * p + k if seed is None else seed)
    shift = 100.0 + rng.standard_normal(p)
    Z = np.asfortranarray(rng.standard_normal((m, k)))
    B = np.asfortranarray(rng.standard_normal((p, k)))
    X = np.asfortranarray(shift + Z @ B.T + (0.01 if k else 1.0) * rng.standard_normal((m, p)))
    return X, shift, Z, B


def resid_ss_longdouble(X, shift, Z, B):
    """out[i] = sum_j (X[i, j] - shift[j] - sum_l Z[i, l] B[j, l])^2 in extended precision."""
    X = np.asarray(X, dtype=np.longdouble)
    E = X - (0 if shift is None else np.asarray(shift, dtype=np.longdouble))
    if Z is not None and np.shape(Z)[1]:
        E = E - np.asarray(Z, dtype=np.longdouble) @ np.asarray(B, dtype=np.longdouble).T
    return np.sum(E * E, axis=1)


def _gamma(n):
    return n * U / (1 - n * U)


def resid_ss_bound(X, shift, Z, B):
    """|out_hat[i] - out[i]| for jch_row_resid_ss, u = 2^-53, gamma_n = n u / (1 - n u).

    An element.  fit_hat = sum_l z_l b_l on the matrix cores: the products are exact inside the fused multiply-adds and the k-term sum costs at most
    k roundings on any path, in any order (zero padding adds exact zeros): |fit_hat - fit| <= gamma_k sum |z||b|.  e_hat = fl(fl(x - shift) - fit_hat):
    one rounding for the centring (u (|x| + |shift|)) and one for the subtraction, so with a = |x| + |shift| + sum_l |z_l||b_l|
        de = |e_hat - e| <= gamma_(k+2) a.
    The square.  e_hat^2 - e^2 = 2 e (e_hat - e) + (e_hat - e)^2: at most 2 |e| de + de^2; it is exact inside fma(e_hat, e_hat, s).
    The row sum.  A lane adds its p / 4 squares in column order, then the four lanes of a row are added as (0 + 1) + (2 + 3): every path from a
    square to the result has at most p / 4 + 2 <= p + 1 roundings, gamma_(p+1) on the sum of the computed squares (|e| + de)^2."""
    X = np.asarray(X, dtype=np.longdouble)
    p = X.shape[1]
    sh = np.zeros(p, dtype=np.longdouble) if shift is None else np.asarray(shift, dtype=np.longdouble)
    k = 0 if Z is None else np.shape(Z)[1]
    a = np.abs(X) + np.abs(sh)
    E = X - sh
    if k:
        Zl, Bl = np.asarray(Z, dtype=np.longdouble), np.asarray(B, dtype=np.longdouble)
        a = a + np.abs(Zl) @ np.abs(Bl).T
        E = E - Zl @ Bl.T
    de = _gamma(k + 2) * a
    sq = 2 * np.abs(E) * de + de * de
    return np.asarray(np.sum(sq, axis=1) + _gamma(p + 1) * np.sum((np.abs(E) + de) ** 2, axis=1), dtype=np.float64)


# ---------------------------------------------------------------------------------- tests: the restatements and the algebra
@pytest.mark.parametrize("name", ["pcasvd", "plskern", "plskern_scal", "plskern_w"])
@pytest.mark.parametrize("nlv", [None, 1, 3])
def test_folded_forms_agree_with_the_literal_ones(name, nlv):
    """What the mirror computes — |Lc' t|^2 with Sinv = Lc Lc', and the residual from the scores e = (x - xmeans) - Ps t — against the literal
    t' Sinv t and the row norms of the `xresid` matrix: 1e-12 relative."""
    X, Xnew, models = _cpu_models()
    fm = models[name]
    ref = np_occsd(fm["T"], nlv)
    k = ref["nlv"]
    S = np.cov(fm["T"][:, :k], rowvar=False, bias=True).reshape(k, k)
    Lc = np.linalg.solve(np.linalg.cholesky(S), np.eye(k)).T
    assert np.allclose(Lc @ Lc.T, ref["Sinv"], rtol=1e-12, atol=1e-12 * np.abs(ref["Sinv"]).max())
    d2 = np.sum((fm["T"][:, :k] @ Lc) ** 2, axis=1)
    assert np.max(np.abs(d2 - ref["d"]["d"] ** 2) / ref["d"]["d"] ** 2) < 1e-12
    # predict: Lc folded into the loadings, one pass over X
    Unew = (Xnew - fm["xmeans"]) / fm["xscales"] @ (fm["R"][:, :k] @ Lc)
    pr = np_occsd_predict(ref, np_transform(fm, Xnew, k))
    assert np.max(np.abs(np.sum(Unew ** 2, axis=1) - pr["d"]["d"] ** 2) / pr["d"]["d"] ** 2) < 1e-12
    # the orthogonal distance from the scores
    for Xq in (X, Xnew):
        lit = np.sum(np_xresid(fm, Xq, k) ** 2, axis=1)
        Ps = fm["xscales"][:, None] * fm["P"][:, :k]
        fold = np.sum(((Xq - fm["xmeans"]) - np_transform(fm, Xq, k) @ Ps.T) ** 2, axis=1)
        assert np.max(np.abs(fold - lit) / lit) < 1e-12
    lit0 = np.sum(np_xresid(fm, Xnew, 0) ** 2, axis=1)                       # nlv = 0: the distances to the column means
    assert np.max(np.abs(np.sum((Xnew - fm["xmeans"]) ** 2, axis=1) - lit0) / lit0) < 1e-12


def test_both_classes_occur_and_few_rows_are_excluded():
    """The seeds of the GPU test: on the restatement alone at most 1 % of the rows fall under the exclusion rule of the pred / pval comparison,
    and the 10 shifted rows are flagged while most of the others are not."""
    X, Xnew, models = _cpu_models()
    for name, fm in models.items():
        for typc in ("mad", "q"):
            obj = np_occsdod(fm, X, None, None, typc)
            pr = np_occsdod_predict(obj, Xnew)
            assert pr["pred"][-10:].all() and pr["pred"][:-10].mean() < 0.5, (name, typc)
            for part, tr in ((obj["fm_sd"], obj["fm_sd"]["d"]), (obj["fm_od"], obj["fm_od"]["d"])):
                keep = comparable_rows(tr["dstand"], tr["d"], part["dtrain"])
                assert (~keep).mean() <= 0.01, (name, typc)
            for sfx, part in (("_sd", obj["fm_sd"]), ("_od", obj["fm_od"])):
                keep = comparable_rows(pr["d"]["dstand" + sfx], pr["d"]["d" + sfx], part["dtrain"])
                assert (~keep).mean() <= 0.01, (name, typc)


def test_median_mad_and_quantile_against_hand_computed_values():
    import jchemo_hip.occ as occ
    odd = np.array([5.0, 1.0, 3.0, 3.0, 9.0])                  # sorted 1 3 3 5 9: median 3; |d - 3| = 2 2 0 0 6 -> sorted 0 0 2 2 6: median 2
    even = np.array([4.0, 1.0, 2.0, 2.0, 8.0, 6.0])            # sorted 1 2 2 4 6 8: median (2 + 4) / 2 = 3; |d - 3| = 1 2 1 1 5 3 -> 1 1 1 2 3 5: 1.5
    for d, med, madraw in ((odd, 3.0, 2.0), (even, 3.0, 1.5)):
        s = np.sort(d)
        assert occ._median_sorted(s) == med == np_median(d)
        assert occ._mad_sorted(s, med) == MAD_CONSTANT * madraw == np_mad(d)
        assert occ._cutoff(s, "mad", 3, .025) == med + 3 * MAD_CONSTANT * madraw == np_cutoff(d, "mad", 3, .025)
    # type 7: position (n - 1) q.  odd, q = 0.975: 4 * 0.975 = 3.9 -> 5 + 0.9 (9 - 5) = 8.6; even, q = 0.5: 2.5 -> 2 + 0.5 (4 - 2) = 3; q = 0.3: 1.5 -> 2
    assert occ._quantile_sorted(np.sort(odd), 0.975) == pytest.approx(8.6, rel=1e-15) and np_quantile(odd, 0.975) == pytest.approx(8.6, rel=1e-15)
    assert occ._quantile_sorted(np.sort(even), 0.5) == 3.0 == np_quantile(even, 0.5)
    assert occ._quantile_sorted(np.sort(even), 0.3) == 2.0 == np_quantile(even, 0.3)
    assert occ._quantile_sorted(np.sort(even), 1.0) == 8.0 and occ._quantile_sorted(np.sort(even), 0.0) == 1.0
    assert occ._quantile_sorted(np.array([7.0]), 0.4) == 7.0 and occ._median_sorted(np.array([7.0])) == 7.0
    rng = np.random.default_rng(3)
    for n in (2, 7, 10, 401):
        d = np.round(rng.random(n), 1)                          # ties
        for q in (0.0, 0.025, 0.5, 0.975, 1.0):
            assert occ._quantile_sorted(np.sort(d), q) == pytest.approx(np.quantile(d, q), rel=1e-14, abs=1e-300)
        assert occ._median_sorted(np.sort(d)) == pytest.approx(np.median(d), rel=1e-15)
    assert occ.MAD_CONSTANT == MAD_CONSTANT
    with pytest.raises(ValueError):
        occ._cutoff(np.sort(odd), "kde", 3, .025)


def test_ecdf_and_pval_below_between_equal_and_above():
    import jchemo_hip.occ as occ
    train = np.array([1.0, 2.0, 2.0, 4.0])                      # sorted, one tie
    q = np.array([0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 9.0])
    want = 1.0 - np.array([0, 1, 1, 3, 3, 4, 4]) / 4            # #(train <= q)
    assert np.array_equal(occ._pval(train, q), want)
    assert np.array_equal(np_pval(train, q), want)


@pytest.mark.parametrize("m,p,k", PRIM_SHAPES)
def test_resid_ss_bound_holds_for_a_float64_evaluation(m, p, k):
    X, shift, Z, B = prim_inputs(m, p, k)
    ref = resid_ss_longdouble(X, shift, Z, B)
    bound = resid_ss_bound(X, shift, Z, B)
    got = np.sum(((X - shift) - Z @ B.T) ** 2, axis=1)
    err = np.abs(np.asarray(got - ref, dtype=np.float64))
    assert np.all(err <= bound), float(np.max(err / bound))
    assert np.all(bound <= 1e-9 * np.asarray(ref, dtype=np.float64))        # not vacuous: the bound is far below the result
    # the plain sums of squares (shift = NULL, k = 0)
    r0 = resid_ss_longdouble(X, None, None, None)
    assert np.all(np.abs(np.asarray(np.sum(X * X, axis=1) - r0, dtype=np.float64)) <= resid_ss_bound(X, None, None, None))


@pytest.mark.parametrize("name", ["pcasvd", "plskern_scal"])
def test_xfit_and_xresid_restatements(name):
    X, Xnew, models = _cpu_models()
    fm = models[name]
    for nlv in (None, 0, 2, 99):
        F, E = np_xfit(fm, Xnew, nlv), np_xresid(fm, Xnew, nlv)
        assert np.allclose(F + E, Xnew, rtol=1e-14)
        k = fm["T"].shape[1] if nlv is None else min(nlv, fm["T"].shape[1])
        M = np.eye(OCC_P) - fm["R"][:, :k] @ fm["P"][:, :k].T                # the mirror's one-GEMM form of xresid
        assert np.allclose((Xnew - fm["xmeans"]) / fm["xscales"] @ (M * fm["xscales"][None, :]), E, atol=1e-12 * np.abs(Xnew).max())


# ---------------------------------------------------------------------------------- tests: the surface
def test_header_declares_the_entry():
    protos = header_protos()
    assert protos["jch_row_resid_ss"][0] == "int32_t" and len(protos["jch_row_resid_ss"][1]) == 13
    mk = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "Makefile")).read()
    assert "occ.hip" in re.search(r"SRCS := (.*)", mk).group(1).split()


def test_python_package_exports_and_fields():
    import inspect

    import jchemo_hip as J
    for name in ("Occsd", "Occod", "Occsdod", "occsd", "occod", "occsdod", "occ_predict", "row_resid_ss"):
        assert hasattr(J, name), name
    assert "jch_row_resid_ss" in J.SYMBOLS
    assert [f.name for f in dataclasses.fields(J.Occsd)][:6] == ["d", "fm", "Sinv", "e_cdf", "cutoff", "nlv"]     # src/occsd.jl:1-8
    assert [f.name for f in dataclasses.fields(J.Occod)] == ["d", "fm", "e_cdf", "cutoff", "nlv"]                  # src/occod.jl:1-7
    assert [f.name for f in dataclasses.fields(J.Occsdod)] == ["d", "fm_sd", "fm_od"]                              # src/occsdod.jl:1-5
    sig = inspect.signature(J.occsd)
    assert list(sig.parameters) == ["fm", "nlv", "typc", "cri", "alpha", "ctx"]
    assert (sig.parameters["typc"].default, sig.parameters["cri"].default, sig.parameters["alpha"].default) == ("mad", 3, .025)
    assert list(inspect.signature(J.occod).parameters) == ["fm", "X", "nlv", "typc", "cri", "alpha", "ctx"]
    assert list(inspect.signature(J.occsdod).parameters) == ["fm", "X", "nlv_sd", "nlv_od", "typc", "cri", "alpha", "ctx"]


def test_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    T = np.asfortranarray(np.random.default_rng(1).standard_normal((20, 3)))
    fm = J.Plsr(T, np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((4, 3)), np.zeros((1, 3)), np.ones(3), np.zeros(4), np.ones(4), np.zeros(1), np.ones(1), np.ones(20) / 20)
    X = np.zeros((20, 4), order="F")
    with pytest.raises(ValueError):
        J.occsd(fm, typc="kde")
    with pytest.raises(ValueError):
        J.occsd(fm, nlv=0)
    with pytest.raises(ValueError):
        J.occod(fm, X, nlv=-1)
    with pytest.raises(ValueError):
        J.occod(fm, X, typc="q", alpha=1.5)
    with pytest.raises(TypeError):
        J.occod(object(), X)
    with pytest.raises(TypeError):
        J.occsdod(J.Occod({}, fm, T[:, 0], 1.0, 1), X)
    with pytest.raises(TypeError):
        J.occ_predict(fm, X)
    with pytest.raises(ValueError):
        J.row_resid_ss(X, np.zeros(3))
    with pytest.raises(ValueError):
        J.row_resid_ss(X, None, T, np.zeros((5, 3)))


def test_occ_without_a_gpu_raises_enodev():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import jchemo_hip as J
    from jchemo_hip._lib import JCH_ENODEV, JchError
    with pytest.raises(JchError) as e:
        J.row_resid_ss(np.zeros((4, 2), order="F"))
    assert e.value.code == JCH_ENODEV


def test_julia_module_exports_and_methods():
    src = open(JL).read()
    m = re.search(r"\nexport (.*?)\n\n", src, flags=re.S)
    names = {s.strip() for s in m.group(1).replace("\n", " ").split(",")}
    for name in ("Occsd", "Occod", "Occsdod", "occsd", "occod", "occsdod"):
        assert name in names, name
    # duck-typed like the other accessors of the wrapper, so that the reference's own records are taken too
    assert re.search(r"function occsd\(object; nlv = nothing, typc = \"mad\", cri = 3, alpha = \.025", src)
    assert re.search(r"function occod\(object, X; nlv = nothing, typc = \"mad\", cri = 3, alpha = \.025", src)
    assert re.search(r"function occsdod\(object, X; nlv_sd = nothing, nlv_od = nothing, typc = \"mad\", cri = 3, alpha = \.025", src)
    occ = src[src.index("function occsd(object;"):src.index("function _occ_sd_cols")]
    assert "view(" not in occ and "object.T[:, 1:k]" in occ          # a view of a host Matrix would be taken for device memory by _loc
    for rec in ("Occsd", "Occod", "Occsdod"):
        assert re.search(r"function predict\(object::" + rec + r", X", src), rec
    assert ":jch_row_resid_ss" in src
    assert "1.4826022185056018" in src
