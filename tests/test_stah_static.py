"""Static checks of the column-median / MAD primitive and the Stahel-Donoho surface (jch_col_median_mad, jch_stah, col_median_mad, colmad, stah,
occstah): the literal numpy restatements of src/utility.jl:162-170, src/stah.jl:37-58 and src/occstah.jl:28-73 the GPU tests compare against,
hand-computed medians and MADs, the facts about the model data the GPU tolerances rest on, and the header / Python / Julia surface.  No GPU needed."""
import dataclasses
import inspect
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
from test_occ_static import MAD_CONSTANT, comparable_rows, np_cutoff, np_mad, np_median, np_pval, occ_data  # noqa: E402


# ---------------------------------------------------------------------------------- numpy restatements of the reference
def np_colmed(X):
    """`vec(median(X, dims = 1))` — src/stah.jl:44: Julia's `median` of a column holding a NaN is NaN."""
    X = np.asarray(X, dtype=np.float64)
    with np.errstate(invalid="ignore"):                                  # (-Inf + Inf) / 2 of an even column is NaN, as `middle` gives
        return np.array([np.nan if np.isnan(c).any() else np_median(c) for c in X.T])


def np_colmad(X):
    """`colmad(X)` — src/utility.jl:162-170: `mad` of each column; a NaN in the column, or a NaN deviation (Inf - Inf), gives NaN."""
    X = np.asarray(X, dtype=np.float64)
    out = np.empty(X.shape[1])
    with np.errstate(invalid="ignore"):
        for j, c in enumerate(X.T):
            bad = np.isnan(c).any() or np.isnan(np.abs(c - np_median(c))).any()
            out[j] = np.nan if bad else np_mad(c)
    return out


def _ld_median(v):
    s = np.sort(v)
    n = s.shape[0]
    return s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2


def _ld_colmed(X):
    return np.array([_ld_median(c) for c in X.T], dtype=np.longdouble)


def _ld_colmad(X):
    return np.array([np.longdouble(MAD_CONSTANT) * _ld_median(np.abs(c - _ld_median(c))) for c in X.T], dtype=np.longdouble)


def np_stah(X, P, scal=True, dtype=np.float64):
    """src/stah.jl:37-58 with P given.  dtype = np.longdouble: the same steps in extended precision (NaN-free data only)."""
    colmed, colmad = (np_colmed, np_colmad) if dtype is np.float64 else (_ld_colmed, _ld_colmad)
    zX = np.array(X, dtype=dtype)                                         # :38 copy(ensure_mat(X))
    n, p = zX.shape                                                       # :39
    P = np.asarray(P, dtype=dtype)
    mu_scal = np.zeros(p, dtype=dtype)                                    # :41
    s_scal = np.ones(p, dtype=dtype)                                      # :42
    if scal:                                                              # :43
        mu_scal = colmed(zX)                                              # :44
        s_scal = colmad(zX)                                               # :45
        zX = (zX - mu_scal) / s_scal                                      # :46 cscale!
    T = zX @ P                                                            # :48
    mu = colmed(T)                                                        # :49
    s = colmad(T)                                                         # :50
    T = np.abs((T - mu) / s)                                              # :51-52
    d = T.max(axis=1)                                                     # :53-56 (numpy's max propagates NaN, as Julia's `maximum`)
    return dict(d=d, P=P, mu_scal=mu_scal, s_scal=s_scal, mu=mu, s=s)


def _stah_d(res, X, dtype=np.float64):
    """src/occstah.jl:56-67: the distances of new rows."""
    zX = (np.array(X, dtype=dtype) - res["mu_scal"]) / res["s_scal"]     # :59-60 center!, scale!
    T = zX @ res["P"]                                                     # :61
    return np.abs((T - res["mu"]) / res["s"]).max(axis=1)                 # :62-68


def np_occstah(X, P, typc="mad", cri=3, alpha=.025, scal=True):
    """src/occstah.jl:28-47 with P given."""
    res = np_stah(X, P, scal)                                             # :30
    d = res["d"]                                                          # :31
    cutoff = np_cutoff(d, typc, cri, alpha)                               # :41-42
    return dict(d=dict(d=d, dstand=d / cutoff, pval=np_pval(d, d)), res_stah=res, dtrain=d, cutoff=cutoff)   # :43-46


def np_occstah_predict(obj, X):
    """src/occstah.jl:55-73."""
    d = _stah_d(obj["res_stah"], X)
    tab = dict(d=d, dstand=d / obj["cutoff"], pval=np_pval(obj["dtrain"], d))                               # :69-70
    return dict(pred=(tab["dstand"] > 1).astype(np.int64).reshape(-1, 1), d=tab)                           # :71-72


def stah_comparable_rows(dstand, d, dtrain, training):
    """test_occ_static.comparable_rows, and no OTHER training row with exactly the row's d either.  That rule lets an exact match pass because it
    takes it for the row's own training value; here two different rows do tie exactly: with one direction and an even n the two rows next to the
    median lie at the same distance (lo + hi) / 2 - lo = hi - (lo + hi) / 2 from it, and a last-bit difference in T breaks the tie and moves one
    count of the ECDF.  training: d is dtrain itself (one exact match is the row's own)."""
    same = (np.asarray(dtrain)[None, :] == np.asarray(d)[:, None]).sum(axis=1)
    return comparable_rows(dstand, d, dtrain) & (same <= (1 if training else 0))


# ---------------------------------------------------------------------------------- the data of the model tests (shared with test_gpu_stah.py)
STAH_A = (1, 7, 100, 130)


def stah_P(p, a):
    """0 / 1 directions from default_rng(7 + a), p x a."""
    return np.asfortranarray(np.random.default_rng(7 + a).integers(0, 2, size=(p, a)), dtype=np.float64)


# ---------------------------------------------------------------------------------- tests: hand-computed values and the restatements
def test_median_and_mad_of_an_odd_and_an_even_column_with_ties():
    odd = np.array([5.0, 1.0, 3.0, 3.0, 9.0])                  # sorted 1 3 3 5 9: median 3; |x - 3| = 2 2 0 0 6 -> 0 0 2 2 6: median 2
    even = np.array([4.0, 1.0, 2.0, 2.0, 8.0, 6.0])            # sorted 1 2 2 4 6 8: median (2 + 4) / 2 = 3; |x - 3| = 1 2 1 1 5 3 -> 1 1 1 2 3 5: 1.5
    X = np.zeros((6, 2))
    assert np.array_equal(np_colmed(odd[:, None]), [3.0]) and np.array_equal(np_colmad(odd[:, None]), [MAD_CONSTANT * 2.0])
    assert np.array_equal(np_colmed(even[:, None]), [3.0]) and np.array_equal(np_colmad(even[:, None]), [MAD_CONSTANT * 1.5])
    X[:, 0], X[:, 1] = even, even[::-1] * 2
    assert np.array_equal(np_colmed(X), [3.0, 6.0]) and np.array_equal(np_colmad(X), [MAD_CONSTANT * 1.5, MAD_CONSTANT * 3.0])
    # Julia's middle(lo, hi) = lo / 2 + hi / 2 equals (lo + hi) / 2 bit for bit away from overflow and underflow
    rng = np.random.default_rng(5)
    lo, hi = rng.standard_normal(1000) * 1e3, rng.standard_normal(1000) * 1e-3
    assert np.array_equal(lo / 2 + hi / 2, (lo + hi) / 2)


def test_nan_and_inf_rules_of_the_restatements():
    X = np.array([[1.0, np.nan, -np.inf, -np.inf], [2.0, 0.0, 0.0, np.inf], [4.0, 1.0, 5.0, 1.0], [3.0, 2.0, np.inf, 2.0]])
    med, mad = np_colmed(X), np_colmad(X)
    assert med[0] == 2.5 and mad[0] == MAD_CONSTANT * 1.0      # |x - 2.5| = 1.5 .5 1.5 .5 -> median 1
    assert np.isnan(med[1]) and np.isnan(mad[1])               # a NaN in the column
    assert med[2] == 2.5 and mad[2] == np.inf                  # -Inf 0 5 Inf: the deviations Inf 2.5 2.5 Inf -> (2.5 + Inf) / 2
    assert med[3] == 1.5 and mad[3] == np.inf                  # -Inf 1 2 Inf
    Y = np.array([[-np.inf], [np.inf]])
    assert np.isnan(np_colmed(Y)[0]) and np.isnan(np_colmad(Y)[0])   # middle(-Inf, Inf) = NaN
    Z = np.array([[np.inf], [np.inf], [1.0]])
    assert np_colmed(Z)[0] == np.inf and np.isnan(np_colmad(Z)[0])   # Inf - Inf among the deviations


def test_stah_restatement_on_a_hand_computed_case():
    X = np.array([[0.0, 0.0], [1.0, 2.0], [2.0, 10.0]])
    P = np.array([[1.0, 1.0], [0.0, 1.0]])
    res = np_stah(X, P, scal=False)                                        # T = [0 0; 1 3; 2 12]: medians 1, 3; raw MADs 1, 3
    assert np.array_equal(res["mu"], [1.0, 3.0]) and np.array_equal(res["s"], [MAD_CONSTANT, MAD_CONSTANT * 3.0])
    assert np.allclose(res["d"], np.array([1.0, 0.0, 3.0]) / MAD_CONSTANT, rtol=1e-15)
    res = np_stah(X, P, scal=True)                                         # medians 1, 2; raw MADs 1, 2 -> zX = [-1 -1; 0 0; 1 4] / c
    assert np.array_equal(res["mu_scal"], [1.0, 2.0]) and np.array_equal(res["s_scal"], [MAD_CONSTANT, MAD_CONSTANT * 2.0])
    assert np.allclose(res["d"], np.array([1.0, 0.0, 2.5]) / MAD_CONSTANT, rtol=1e-14)   # T c = [-1 -2; 0 0; 1 5]: |t| / (1, 2)
    X[1, 0] = np.nan
    assert np.isnan(np_stah(X, P, scal=False)["mu"]).all()                # a NaN in X reaches both projections here


@pytest.mark.parametrize("scal", [True, False])
@pytest.mark.parametrize("a", STAH_A)
def test_model_data_facts_the_gpu_tolerances_rest_on(a, scal):
    """On the restatement alone, for the data and the directions of the GPU test: no direction is zero, the float64 restatement is within 1e-11 of
    its extended-precision run for fit and predict (1e-9 on the GPU leaves 100x), at most 1 % of the rows fall under the exclusion rule of the pred /
    pval comparison, and both classes occur.  The gap is absolute for the training rows (d <= 4.9) and in the GPU test's own metric |diff| / max(1, |ref|)
    for the new rows: the 10 shifted ones have d of several hundred, and their absolute gap (3.6e-11 at a = 130 unscaled) is their size times 1e-13."""
    X, _, Xnew, _ = occ_data()
    P = stah_P(X.shape[1], a)
    assert (P.sum(axis=0) > 0).all()
    res, ld = np_stah(X, P, scal), np_stah(X, P, scal, dtype=np.longdouble)
    gap = float(np.max(np.abs(res["d"] - ld["d"])))
    dn, dn_ld = _stah_d(res, Xnew), _stah_d(ld, Xnew, np.longdouble)
    gap_new = float(np.max(np.abs(dn - dn_ld) / np.maximum(1, np.abs(dn_ld))))
    assert float(np.max(np.abs(dn - dn_ld)[:-10])) <= 1e-11               # the unshifted new rows: absolute, like the training rows
    print(f"a={a} scal={scal}: min s = {res['s'].min():.3g}, d in [{res['d'].min():.3g}, {res['d'].max():.3g}], new d up to {dn.max():.3g}, f64 / longdouble gap {gap:.3g} (fit) {gap_new:.3g} (predict)")
    assert gap <= 1e-11 and gap_new <= 1e-11
    assert res["s"].min() > 0.1 and np.isfinite(res["d"]).all()
    for typc in ("mad", "q"):
        obj = np_occstah(X, P, typc, scal=scal)
        pr = np_occstah_predict(obj, Xnew)
        assert not (~comparable_rows(obj["d"]["dstand"], obj["d"]["d"], obj["dtrain"])).any()          # the rule of the occ models excludes no row at all
        assert not (~comparable_rows(pr["d"]["dstand"], pr["d"]["d"], obj["dtrain"])).any()
        out = ~stah_comparable_rows(obj["d"]["dstand"], obj["d"]["d"], obj["dtrain"], True)               # ... with exact ties out: the two median rows at a = 1
        assert out.mean() <= 0.01 and out.sum() == (2 if a == 1 else 0)
        assert not (~stah_comparable_rows(pr["d"]["dstand"], pr["d"]["d"], obj["dtrain"], False)).any()
        assert pr["pred"].any() and not pr["pred"].all()
        if a > 1:
            assert pr["pred"][-10:].all() and pr["pred"][:-10].mean() <= 0.05      # the shifted rows are flagged, few of the others


# ---------------------------------------------------------------------------------- tests: the surface
def test_header_declares_the_entries_and_the_makefile_builds_them():
    protos = header_protos()
    assert protos["jch_col_median_mad"][0] == "int32_t" and len(protos["jch_col_median_mad"][1]) == 9
    assert protos["jch_stah"][0] == "int32_t" and len(protos["jch_stah"][1]) == 15
    mk = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"SRCS := (.*)", mk).group(1).split()
    assert "colselect.hip" in srcs and "stah.hip" in srcs


def test_python_package_exports_fields_and_defaults():
    import jchemo_hip as J
    for name in ("Occstah", "occstah", "stah", "colmad", "col_median_mad", "occ_predict"):
        assert hasattr(J, name), name
    assert "jch_col_median_mad" in J.SYMBOLS and "jch_stah" in J.SYMBOLS
    assert [f.name for f in dataclasses.fields(J.Occstah)] == ["d", "res_stah", "e_cdf", "cutoff"]                 # src/occstah.jl:1-6
    assert [f.name for f in dataclasses.fields(J.Stah)] == ["d", "P", "mu_scal", "s_scal", "mu", "s"]              # src/stah.jl:58
    sig = inspect.signature(J.occstah)
    assert list(sig.parameters) == ["X", "a", "typc", "cri", "alpha", "scal", "P", "seed", "ctx"]
    assert [sig.parameters[k].default for k in ("a", "typc", "cri", "alpha", "scal", "P", "seed")] == [2000, "mad", 3, .025, True, None, None]
    sig = inspect.signature(J.stah)
    assert list(sig.parameters) == ["X", "a", "scal", "P", "seed", "ctx"] and sig.parameters["scal"].default is True
    sig = inspect.signature(J.col_median_mad)
    assert list(sig.parameters) == ["X", "mad", "ctx"] and sig.parameters["mad"].default is True
    assert list(inspect.signature(J.colmad).parameters) == ["X", "ctx"]
    import jchemo_hip.occ as occ
    assert occ.MAD_CONSTANT == MAD_CONSTANT
    src = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "colselect.hip")).read()
    assert "1.4826022185056018" in src


def test_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    X = np.zeros((20, 4), order="F")
    with pytest.raises(ValueError):
        J.occstah(X, typc="kde")
    with pytest.raises(ValueError):
        J.occstah(X, typc="q", alpha=1.5)
    with pytest.raises(ValueError):
        J.occstah(X, a=0)
    with pytest.raises(ValueError):
        J.stah(X, 0)
    with pytest.raises(ValueError):
        J.stah(X, 2.5)
    with pytest.raises(ValueError):
        J.stah(X, 3, P=np.zeros((4, 2)))
    with pytest.raises(ValueError):
        J.stah(X, 3, P=np.zeros((5, 3)))
    with pytest.raises(ValueError):
        J.occstah(X, a=3, P=np.zeros((3, 4)))
    with pytest.raises(ValueError):
        J.col_median_mad(np.zeros((0, 3)))
    res = J.Stah(np.zeros(20), np.zeros((4, 3)), np.zeros(4), np.ones(4), np.zeros(3), np.ones(3))
    with pytest.raises(ValueError):
        J.occ_predict(J.Occstah({}, res, np.zeros(20), 1.0), np.zeros((5, 6)))


def test_without_a_gpu_every_entry_raises_enodev():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import jchemo_hip as J
    from jchemo_hip._lib import JCH_ENODEV, JchError
    X = np.asfortranarray(np.random.default_rng(0).standard_normal((6, 3)))
    res = J.Stah(np.zeros(6), np.ones((3, 2)), np.zeros(3), np.ones(3), np.zeros(2), np.ones(2))
    calls = [lambda: J.col_median_mad(X), lambda: J.col_median_mad(X, mad=False), lambda: J.colmad(X), lambda: J.stah(X, 2, seed=1),
             lambda: J.stah(X, 2, scal=False, seed=1), lambda: J.occstah(X, a=2, seed=1), lambda: J.occ_predict(J.Occstah({}, res, np.zeros(6), 1.0), X),
             lambda: J.predict(J.Occstah({}, res, np.zeros(6), 1.0), X)]
    for call in calls:
        with pytest.raises(JchError) as e:
            call()
        assert e.value.code == JCH_ENODEV


def test_seed_pins_the_directions():
    import jchemo_hip  # noqa: F401
    S = sys.modules["jchemo_hip.stah"]                                    # (the package attribute `stah` is the function)
    P1, P2 = S._directions(5, 4, None, 11), S._directions(5, 4, None, 11)
    assert np.array_equal(P1, P2) and P1.shape == (5, 4) and P1.flags.f_contiguous and set(np.unique(P1)) <= {0.0, 1.0}
    assert not np.array_equal(P1, S._directions(5, 4, None, 12))


def test_julia_module_exports_and_methods():
    src = open(JL).read()
    m = re.search(r"\nexport (.*?)\n\n", src, flags=re.S)
    names = {s.strip() for s in m.group(1).replace("\n", " ").split(",")}
    for name in ("Occstah", "occstah", "stah", "colmad"):
        assert name in names, name
    assert re.search(r"\ncolmad\(X; ctx = default_ctx\(\)\)", src)
    assert re.search(r"function stah\(X, a; scal = true", src)
    assert re.search(r"function occstah\(X; a = 2000, typc = \"mad\", cri = 3, alpha = \.025, scal = true", src)
    assert re.search(r"function predict\(object::Occstah, X", src)
    assert re.search(r"struct Occstah\s[^\n]*\n\s+d\n\s+res_stah\n\s+e_cdf\n\s+cutoff::Float64\nend", src)
    assert ":jch_col_median_mad" in src and ":jch_stah" in src
    # every pointer handed to the two entries is rooted while the call runs
    call = src[src.index("function _stah_call"):src.index('"""`stah(X, a; scal = true)`')]
    assert "GC.@preserve X mu_scal s_scal P mu s d begin" in call
    call = src[src.index("function col_median_mad"):src.index("colmad(X; ctx")]
    assert "GC.@preserve X med md begin" in call
