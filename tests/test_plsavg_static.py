"""Static checks of the model-averaging surface (fweight, wshenk, plsravg, plsrdaavg / plsldaavg / plsqdaavg, jch_row_resid_ss_lv): the algebra the
device route relies on against the literal restatements (tests/plsavg_restate.py), the error bound of the nested residual kernel's summation
order, `fweight` against hand-computed values, and the header / Python / Julia / Makefile boundary.  No GPU needed."""
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

import plsavg_restate as R  # noqa: E402
from oracle import plsr_oracle as O  # noqa: E402
from test_julia_wrapper import JL, header_protos  # noqa: E402
from test_occ_static import prim_inputs, resid_ss_bound  # noqa: E402


def avg_data(n=150, p=40, q=1, m=37, seed=5):
    """Rank-6 structure plus noise, q responses that depend on it."""
    rng = np.random.default_rng(seed)
    S = rng.standard_normal((n + m, 6))
    Xall = 5.0 + S @ rng.standard_normal((6, p)) + 0.05 * rng.standard_normal((n + m, p))
    Yall = S[:, :3] @ rng.standard_normal((3, q)) + 0.1 * rng.standard_normal((n + m, q))
    w = rng.uniform(0.5, 1.5, n)
    return np.asfortranarray(Xall[:n]), np.asfortranarray(Yall[:n]), np.asfortranarray(Xall[n:]), w


# ---------------------------------------------------------------------------------- the algebra
@pytest.mark.parametrize("scal", [False, True])
def test_shenk_weights_are_the_renormalised_reciprocal_products(scal):
    """The three `mweight` calls of src/wshenk.jl:69-73 followed by the one of src/plsravg_shenk.jl:39 cancel: over any level subset the weights are
    1 / (rss_r rss_b) normalised over that subset — what the device route forms — to 1e-12."""
    X, Y, Xnew, w = avg_data()
    fm = O.plskern(X, Y, w, nlv=8, scal=scal)
    ref = R.np_wshenk(fm, Xnew)
    rss_r, rss_b = R.np_shenk_rss(fm, Xnew)
    direct = 1 / (rss_r * rss_b[None, :])
    assert np.max(np.abs(direct / direct.sum(axis=1, keepdims=True) - ref["w"]) / ref["w"]) < 1e-12
    for lo, hi in ((1, 8), (3, 6), (4, 5)):
        sub = ref["w"][:, lo - 1:hi]
        lit = sub / sub.sum(axis=1, keepdims=True)
        d = direct[:, lo - 1:hi]
        assert np.max(np.abs(d / d.sum(axis=1, keepdims=True) - lit) / lit) < 1e-12


@pytest.mark.parametrize("scal", [False, True])
def test_residual_from_the_scores_equals_xresid_per_level(scal):
    """What `wshenk` hands to the kernel — shift = xmeans, Z = transform, B = diag(xscales) P — reproduces the row norms of `xresid` at every
    level, 1e-12 relative (extended-precision sums of the direct form)."""
    X, Y, Xnew, w = avg_data()
    fm = O.plskern(X, Y, w, nlv=8, scal=scal)
    T = O.transform(fm, Xnew)
    Ps = fm.xscales[:, None] * fm.P
    got = np.asarray(R.resid_ss_lv_longdouble(Xnew, fm.xmeans, T, Ps, 1, 8), dtype=np.float64)
    rss_r, _ = R.np_shenk_rss(fm, Xnew)
    assert np.max(np.abs(np.sqrt(got) - rss_r) / rss_r) < 1e-12


@pytest.mark.parametrize("m,p,a_lo,a_hi,kz", [(63, 15, 1, 3, 3), (65, 17, 2, 5, 7), (40, 33, 0, 25, 25), (20, 40, 1, 49, 49)])
def test_running_residual_order_is_within_the_bound_per_level(m, p, a_lo, a_hi, kz):
    """The kernel's order — e_0 = fl(x - shift), e_a = fma(-z_a, b_a, e_(a-1)), the row sum in column order with fused squares — has a + 1 <= a + 2
    roundings per element and p <= p + 1 per row-sum path, so test_occ_static.resid_ss_bound with k = a covers level a unchanged."""
    X, shift, Z, B = prim_inputs(m, p, kz)
    run = R.resid_ss_lv_running_f64(X, shift, Z, B, a_lo, a_hi)
    ref = R.resid_ss_lv_longdouble(X, shift, Z, B, a_lo, a_hi)
    for a in range(a_lo, a_hi + 1):
        bound = resid_ss_bound(X, shift, Z[:, :a], B[:, :a])
        err = np.abs(np.asarray(run[:, a - a_lo] - ref[:, a - a_lo], dtype=np.float64))
        assert np.all(err <= bound), (a, float(np.max(err / bound)))


# ---------------------------------------------------------------------------------- fweight against hand values
D = np.array([0.0, -0.5, 1.0, 2.0, np.nan])    # |d| = 0, .5, 1, 2; the NaN is left out of the quantile and gets weight 0
HAND = {   # f(x) at x = 0, 1/4, 1/2 (alpha = 0: q = max = 2, x = 1 has weight f(1) and is NOT cut: only x > 1 is)
    "bisquare": ([1.0, (15 / 16) ** 2, (3 / 4) ** 2, 0.0], lambda x: (1 - x * x) ** 2),
    "cauchy": ([1.0, 16 / 17, 4 / 5, 1 / 2], lambda x: 1 / (1 + x * x)),
    "epan": ([1.0, 15 / 16, 3 / 4, 0.0], lambda x: 1 - x * x),
    "fair": ([1.0, 16 / 25, 4 / 9, 1 / 4], lambda x: 1 / (1 + x) ** 2),
    "invexp": ([1.0, np.exp(-0.25), np.exp(-0.5), np.exp(-1.0)], lambda x: np.exp(-x)),
    "invexp2": ([1.0, np.exp(-0.125), np.exp(-0.25), np.exp(-0.5)], lambda x: np.exp(-x / 2)),
    "gauss": ([1.0, np.exp(-1 / 16), np.exp(-0.25), np.exp(-1.0)], lambda x: np.exp(-x * x)),
    "trian": ([1.0, 3 / 4, 1 / 2, 0.0], lambda x: 1 - x),
    "tricube": ([1.0, (63 / 64) ** 3, (7 / 8) ** 3, 0.0], lambda x: (1 - x ** 3) ** 3),
}


@pytest.mark.parametrize("typw", R.TYPW)
def test_fweight_against_hand_values(typw):
    import jchemo_hip as J
    hand0, f = HAND[typw]
    for fw in (J.fweight, R.np_fweight):
        w = fw(D.copy(), typw=typw, alpha=0)
        assert np.allclose(w, hand0 + [0.0], rtol=1e-15, atol=0)
        # alpha = 0.1: the 0.9 quantile of (0, .5, 1, 2) is at position 0.9 * 3 = 2.7: 1 + 0.7 * (2 - 1) = 1.7; |d| = 2 is beyond it
        w = fw(D.copy(), typw=typw, alpha=0.1)
        assert np.allclose(w, [f(0.0), f(0.5 / 1.7), f(1 / 1.7), 0.0, 0.0], rtol=1e-14, atol=0)
    assert np.array_equal(D[:4], np.array([0.0, -0.5, 1.0, 2.0]))             # the caller's vector is not rewritten
    with pytest.raises(ValueError):
        J.fweight(D, typw="inv")


def test_findmax_cla_takes_the_smallest_label_on_a_tie():
    import jchemo_hip as J
    from jchemo_hip.plsavg import vote
    assert J.findmax_cla(["b", "a"]) == "a" and R.np_findmax_cla(["b", "a"])[0] == "a"
    assert J.findmax_cla([3, 1, 3, 1, 2]) == 1
    assert J.findmax_cla([3, 1, 2], [0.2, 0.3, 0.5]) == 2
    lab = np.array([[2, 1], [1, 2], [2, 2], [3, 1]])
    assert vote(lab, np.array([0.5, 0.5]), np.array([1, 2, 3])).reshape(-1).tolist() == [1, 1, 2, 1]


# ---------------------------------------------------------------------------------- the boundary
def test_header_makefile_and_symbols_declare_the_entry():
    protos = header_protos()
    ret, args = protos["jch_row_resid_ss_lv"]
    assert ret == "int32_t" and len(args) == 16
    assert len(protos["jch_row_resid_ss"][1]) == 13                            # the existing entry keeps its signature
    hdr = open(os.path.join(ROOT, "include", "jchemo_hip.h")).read()
    assert hdr.index("jch_row_resid_ss(") < hdr.index("jch_row_resid_ss_lv(") < hdr.index("jch_col_median_mad(")   # next to its sibling
    assert re.search(r"#define JCH_VERSION\s+108\b", hdr)
    mk = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "Makefile")).read()
    assert "resid_lv.hip" in re.search(r"SRCS := (.*)", mk).group(1).split()
    import jchemo_hip as J
    assert "jch_row_resid_ss_lv" in J.SYMBOLS and "jch_lwplsravg_predict_prepared" in J.SYMBOLS
    ret, args = protos["jch_lwplsravg_predict_prepared"]
    assert ret == "int32_t" and len(args) == 24
    assert len(protos["jch_lwplsr_predict_prepared"][1]) == 18 and len(protos["jch_lwplsda_predict_prepared"][1]) == 26   # the existing entries keep theirs
    assert "lwplsravg.hip" in re.search(r"SRCS := (.*)", mk).group(1).split()
    dev = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "lwplsr_dev.h")).read()
    for field in ("double *rss_r = nullptr", "double *rss_b = nullptr", "int *shenk_info = nullptr"):
        assert field in dev
    assert "template <int KC, int Q, bool SHENK = false>" in open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "lwplsr.hip")).read()
    assert ":jch_lwplsravg_predict_prepared" in open(JL).read()
    src = open(JL).read()
    assert ":jch_row_resid_ss_lv" in src
    names = {s.strip() for s in re.search(r"\nexport (.*?)\n\n", src, flags=re.S).group(1).replace("\n", " ").split(",")}
    assert "row_resid_ss_lv" in names


def test_python_package_exports_and_fields():
    import jchemo_hip as J
    for name in ("fweight", "wshenk", "row_resid_ss_lv", "plsravg", "plsravg_", "plsravg_predict", "plsrdaavg", "plsldaavg", "plsqdaavg",
                 "plsdaavg_predict", "findmax_cla", "lwplsravg", "lwplsravg_predict", "lwplsrdaavg", "lwplsldaavg", "lwplsqdaavg",
                 "lwplsdaavg_predict", "LwplsrAvg", "LwplsdaAvg", "LwplsrAvgPred", "lwplsravg_prepared_call", "Plsravg", "PlsravgUnif", "PlsravgShenk", "PlsravgCri", "Plsrstack", "Plsdaavg"):
        assert hasattr(J, name), name
    assert [f.name for f in dataclasses.fields(J.Plsravg)] == ["fm"]                                               # src/plsravg.jl:1-3
    assert [f.name for f in dataclasses.fields(J.PlsravgCri)] == ["fm", "nlv", "w"]                                # src/plsravg_aic.jl:1-5
    assert [f.name for f in dataclasses.fields(J.Plsrstack)] == ["fm", "nlv", "w", "Xstack", "ystack", "weightsstack"]
    assert [f.name for f in dataclasses.fields(J.Plsdaavg)] == ["fm", "nlv", "w_mod", "lev", "ni"]                 # src/plsrdaavg.jl:1-7
    sig = inspect.signature(J.plsravg)
    assert list(sig.parameters) == ["X", "Y", "weights", "nlv", "typf", "typw", "alpha", "K", "rep", "scal", "segm", "seed", "ctx"]
    assert [sig.parameters[k].default for k in ("typf", "typw", "alpha", "K", "rep", "scal")] == ["unif", "bisquare", 0, 5, 10, False]
    assert [f.name for f in dataclasses.fields(J.LwplsrAvg)] == ["X", "Y", "fm", "metric", "h", "k", "nlv", "typf", "typw", "alpha", "K", "rep", "tol", "scal",
                                                                 "verbose"]                                      # src/lwplsravg.jl:1-17
    assert list(inspect.signature(J.lwplsravg).parameters) == ["X", "Y", "nlvdis", "metric", "h", "k", "nlv", "typf", "typw", "alpha", "K", "rep", "tol",
                                                               "scal", "verbose", "ctx"]                         # src/lwplsravg.jl:100-102
    assert list(inspect.signature(J.fweight).parameters) == ["d", "typw", "alpha"]
    assert list(inspect.signature(J.wshenk).parameters) == ["fm", "X", "nlv", "ctx"]
    assert list(inspect.signature(J.row_resid_ss_lv).parameters) == ["X", "shift", "Z", "B", "a_lo", "a_hi", "ctx"]


def test_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    X, Y, Xnew, w = avg_data(n=30, p=6, m=4)
    y = np.arange(30) % 3
    for typf in ("aic", "bic"):
        with pytest.raises(NotImplementedError, match="dfplsr_cg"):
            J.plsravg(X, Y, nlv="1:3", typf=typf)
    with pytest.raises(ValueError):
        J.plsravg(X, Y, nlv="1:3", typf="median")
    with pytest.raises(ValueError):
        J.plsravg(X, Y, nlv="1:3", typf="cv", typw="inv")
    with pytest.raises(ValueError):
        J.plsravg(X, Y, nlv="3:1")
    with pytest.raises(ValueError):
        J.plsravg(X, Y, nlv="a:b")
    with pytest.raises(ValueError):
        J.plsravg(X, Y, nlv="0", typf="shenk")
    with pytest.raises(ValueError):
        J.plsravg(X, np.hstack([Y, Y]), nlv="1:3", typf="stack")
    with pytest.raises(ValueError):
        J.plsldaavg(X, y, nlv="0:3")                                           # level 0 is allowed for plsrdaavg only
    with pytest.raises(ValueError):
        J.plsqdaavg(X, y, nlv="0:3")
    lw = dict(nlvdis=0, metric="eucl", h=2.0, k=10)
    with pytest.raises(NotImplementedError, match="dfplsr_cg"):
        J.lwplsravg(X, Y, nlv="1:3", typf="aic", **lw)
    with pytest.raises(ValueError):
        J.lwplsravg(X, Y, nlv="1:3", typf="median", **lw)
    with pytest.raises(ValueError):
        J.lwplsravg(X, Y, nlv="3:1", **lw)
    with pytest.raises(ValueError):
        J.lwplsldaavg(X, y, nlv="0:3", **lw)
    with pytest.raises(ValueError):
        J.lwplsqdaavg(X, y, nlv="0:3", **lw)
    from jchemo_hip.plsavg import _local_range
    assert list(_local_range("5:60", 30, 130)) == list(range(5, 31)) and list(_local_range("0:3", 10, 6, 1)) == [1, 2, 3]
    T = np.asfortranarray(np.zeros((30, 3)))
    with pytest.raises(ValueError):
        J.row_resid_ss_lv(X, None, T, np.zeros((6, 3)), 2, 1)
    with pytest.raises(ValueError):
        J.row_resid_ss_lv(X, None, T, np.zeros((6, 3)), 0, 4)
    with pytest.raises(ValueError):
        J.row_resid_ss_lv(X, None, T, np.zeros((5, 3)), 0, 3)
    with pytest.raises(ValueError):
        J.row_resid_ss_lv(X, np.zeros(5), T, np.zeros((6, 3)), 0, 3)
    from jchemo_hip.plsavg import parse_nlv
    assert parse_nlv("0:6") == (0, 6) and parse_nlv("4") == (4, 4) and parse_nlv(range(2, 5)) == (2, 4) and parse_nlv(3) == (3, 3)


def test_restated_models_hang_together():
    """The restatements the GPU tests compare against: uniform weights reproduce the plain mean, the cv weights sum to one and vanish at the worst
    level, the stacking weights solve their normal equations, and a voting model with one level is that level."""
    X, Y, Xnew, w = avg_data()
    segm = [[np.arange(0, 150, 2), np.arange(1, 150, 2)]]
    un = R.np_plsravg_unif_predict(R.np_plsravg_unif(X, Y, w, nlv="0:6"), Xnew)
    assert np.allclose(un["pred"], np.mean(np.stack(un["predlv"]), axis=0), rtol=1e-13)
    cv = R.np_plsravg_cv(X, Y, w, nlv="0:6", segm=segm)
    assert abs(cv["w"].sum() - 1) < 1e-14 and cv["w"].min() == 0.0 and len(cv["w"]) == 7
    st = R.np_plsrstack(X, Y, w, nlv="3:6", segm=segm)
    G = st["Xstack"].T @ (st["weightsstack"][:, None] * st["Xstack"])
    assert np.allclose(G @ st["w"], st["Xstack"].T @ (st["weightsstack"] * st["ystack"][:, 0]), rtol=1e-9)
    sh = R.np_plsravg_shenk_predict(R.np_plsravg_shenk(X, Y, w, nlv="0:6"), Xnew)
    assert sh["w"].shape == (37, 6) and len(sh["predlv"]) == 6               # level 0 is dropped (src/plsravg_shenk.jl:18)
    y = (np.arange(150) % 3)[np.argsort(X[:, 0])]
    one = R.np_plsdaavg_predict(R.np_plsdaavg("lda", X, y, nlv="4"), Xnew)
    assert np.array_equal(one["pred"], O.plslda_predict(O.plslda(X, y, nlv=4), Xnew, nlv=4)[0])


@pytest.mark.parametrize("scal", [False, True])
@pytest.mark.parametrize("q", [1, 3])
def test_incremental_local_forms_equal_xresid_and_coef(scal, q):
    """The running forms a local-fit kernel would keep per query — e starting at the centred (scaled) row with e -= t_a P_a, Bm starting at 0 with
    Bm[y] += r_a c_a[y] — give, per level, sg e = the `xresid` row and Bo[j, y] = Bm[y][j] ysd[y] / sg[j], int_y = ymean[y] - sum_j mu[j] Bo[j, y] =
    `coef`, hence the two Shenk norms of src/wshenk.jl:59-67, on a weighted local fit: 1e-12."""
    X, Y, Xnew, w = avg_data(n=40, p=25, q=q, m=5)
    a = 8
    fm = O.plskern(X, Y, w, nlv=a, scal=scal)
    sg, mu = fm.xscales, fm.xmeans
    for x in Xnew:
        e = (x - mu) / sg
        xq = e.copy()
        Bm = np.zeros((q, X.shape[1]))
        for l in range(a):
            tq = xq @ fm.R[:, l]
            e = e - tq * fm.P[:, l]
            Bm += np.outer(fm.C[:, l], fm.R[:, l])
            lit = O.xresid(fm, x[None, :], nlv=l + 1)[0]
            assert np.max(np.abs(sg * e - lit)) <= 1e-12 * np.max(np.abs(x - mu))
            B, intercept = O.coef(fm, nlv=l + 1)
            Bo = (Bm * fm.yscales[:, None] / sg[None, :]).T
            assert np.max(np.abs(Bo - B)) <= 1e-12 * np.max(np.abs(B))
            assert np.max(np.abs((fm.ymeans - mu @ Bo) - intercept[0])) <= 1e-12 * max(1.0, np.max(np.abs(intercept)))
            rss_r = np.sqrt(np.sum((sg * e) ** 2))
            rss_b = np.sqrt((np.sum((fm.ymeans - mu @ Bo) ** 2) + np.sum(Bo ** 2)) / q)
            ref_r, ref_b = R.np_shenk_rss(fm, x[None, :], l + 1)
            assert abs(rss_r - ref_r[0, l]) <= 1e-12 * ref_r[0, l] and abs(rss_b - ref_b[l]) <= 1e-12 * ref_b[l]
