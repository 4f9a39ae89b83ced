"""CPU-side checks of permutation importance and interval selection (restatements and bounds: tests/viperm_restate.py, shared with
tests/test_gpu_viperm.py): the documented generator gives permutations and passes the uniformity checks numpy's own generator passes; the
rank-one form of the shuffled predictions equals the reference's loop within the derived bound; a float64 evaluation stays inside that bound in
two summation orders; `isel`'s interval bounds round half to even; and the boundary (header, Makefile, SYMBOLS, exports, defaults, ValueErrors
before any device work).

Uniformity.  For a uniform source the number of fixed points of a permutation has mean 1 and variance 1 (m >= 2), so the mean over N
permutations has standard deviation 1 / sqrt(N); the bound is 6 of them.  Where element 0 lands is uniform over m cells: Pearson's statistic
against N / m per cell is chi-square with m - 1 degrees of freedom, and the bound is its 1 - 1e-6 quantile by the Wilson-Hilferty formula
(z = 4.7534; for 32 degrees of freedom 79.1 against the exact 78.9, for 999 within 0.1 %).  N = 20000 at m = 33 (606 per cell) and N = 6000 at
m = 1000 (6 per cell): the fixed-point bounds are 0.042 and 0.077."""
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

import viperm_restate as V  # noqa: E402

Z_1E6 = 4.7534   # standard normal quantile at 1 - 1e-6


def chi2_quantile_1e6(k):
    """Wilson-Hilferty: the 1 - 1e-6 quantile of chi-square with k degrees of freedom."""
    return k * (1.0 - 2.0 / (9.0 * k) + Z_1E6 * np.sqrt(2.0 / (9.0 * k))) ** 3


# ---------------------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("m", V.M_LIST)
def test_every_column_is_a_permutation(m):
    P = V.perm_matrix(20260101, m, 3)
    assert P.shape == (m, 3) and P.dtype == np.int32
    for c in range(3):
        assert np.array_equal(np.sort(P[:, c]), np.arange(m))


def test_bit_widths_and_rounds_as_documented():
    assert [V.perm_bits(m) for m in (1, 2, 4, 5, 16, 17, 64, 65, 1000, 4096, 4097, 2 ** 16, 2 ** 16 + 1, 2 ** 31 - 1)] == [2, 2, 2, 4, 4, 6, 6, 8, 10, 12, 14, 16, 18, 32]
    assert V.perm_rounds(12) == 24 and V.perm_rounds(14) == 8
    assert np.array_equal(V.perm_matrix(5, 1, 4), np.zeros((1, 4), dtype=np.int32))          # m = 1: the identity


def test_columns_and_seeds_give_different_permutations():
    for m in (33, 1000):
        A, B = V.perm_matrix(7, m, 8), V.perm_matrix(8, m, 8)
        for c in range(8):
            assert not np.array_equal(A[:, c], B[:, c])
            for c2 in range(c):
                assert not np.array_equal(A[:, c], A[:, c2])
    # column j depends on (seed, j) alone: a block of columns started further right is the same columns
    assert np.array_equal(V.perm_matrix(7, 1000, 3, j0=5), V.perm_matrix(7, 1000, 8)[:, 5:])


def _uniformity(P):
    m, N = P.shape
    fixed = float((P == np.arange(m)[:, None]).sum()) / N
    counts = np.bincount(P[0], minlength=m).astype(np.float64)
    return fixed, float(((counts - N / m) ** 2 / (N / m)).sum())


@pytest.mark.parametrize("m,N", [(33, 20000), (1000, 6000)])
@pytest.mark.parametrize("source", ["feistel", "numpy"])
def test_uniformity_of_fixed_points_and_of_where_element_0_lands(m, N, source):
    if source == "feistel":
        P = V.perm_matrix(20260102, m, N)
    else:
        rng = np.random.default_rng(20260102)
        P = np.stack([rng.permutation(m) for _ in range(N)], axis=1)
    fixed, chi2 = _uniformity(P)
    print(f"{source} m={m} N={N}: fixed points per permutation {fixed:.4f} (bound 1 +- {6 / np.sqrt(N):.4f}), chi2 {chi2:.1f} (bound {chi2_quantile_1e6(m - 1):.1f})")
    assert abs(fixed - 1.0) < 6.0 / np.sqrt(N)
    assert chi2 < chi2_quantile_1e6(m - 1)


# ---------------------------------------------------------------------------------------------------- sums, bound, rank-one identity
def _data(n, p, q, m, seed, offset=3.0):
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(rng.normal(size=(n, p)) + offset)
    B = rng.normal(size=(p, q))
    intercept = rng.normal(size=(1, q))
    Y = np.asfortranarray(intercept + X @ B + 0.1 * rng.normal(size=(n, q)))
    rows = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64)
    return X, Y, B, intercept, rows, V.perm_matrix(seed, m, p)


def test_float64_sums_stay_inside_the_bound_in_two_orders():
    X, Y, B, intercept, rows, perm = _data(700, 9, 3, 233, 11)
    Pred = np.asfortranarray(intercept + X @ B)
    ref = V.ref_perm_sums(X, rows, Pred, Y, B, perm)
    bound = V.bound_perm_sums(X, rows, Pred, Y, B, perm)
    worst = 0.0
    for order in (slice(None), slice(None, None, -1)):
        got = V.ref_perm_sums(X, rows, Pred, Y, B, perm, t=np.float64, order=order)
        err = np.abs(got.astype(V.LD) - ref).astype(np.float64)
        assert np.all(err <= bound)
        assert np.array_equal(got[..., 5], np.full(got.shape[:2], 233.0))
        worst = max(worst, float((err[..., :5] / bound[..., :5]).max()))
    print(f"float64 in two orders uses at most {worst:.3f} of the bound")
    assert 0.0 < worst < 0.5   # (the bound is not vacuous either: the reference alone does not sit at zero)


def test_rank_one_sums_equal_the_reference_loop_within_the_bound():
    X, Y, B, intercept, rows, perm = _data(400, 7, 2, 133, 12)
    Pred = (np.asarray(intercept, dtype=V.LD) + np.asarray(X, dtype=V.LD) @ np.asarray(B, dtype=V.LD))
    loop = V.loop_perm_sums(X, rows, Y, B, intercept, perm)
    rank1 = V.ref_perm_sums(X, rows, Pred, Y, B, perm)
    bound = V.bound_perm_sums(X, rows, Pred.astype(np.float64), Y, B, perm)
    err = np.abs(loop - rank1).astype(np.float64)
    print(f"loop vs rank-one (longdouble): at most {float((err[..., :5] / bound[..., :5]).max()):.2e} of the bound")
    assert np.all(err <= bound)
    # ... and in float64 from the rounded predictions, the way the library is called
    got = V.ref_perm_sums(X, rows, np.asfortranarray(Pred.astype(np.float64)), Y, B, perm, t=np.float64)
    # (Pred rounded to float64 moves the exact sums by eps |pred| per element, which the bound's |pred| term covers)
    assert np.all(np.abs(got.astype(V.LD) - loop).astype(np.float64) <= 2.0 * bound)


def test_zero_coefficient_row_and_constant_column_give_the_unshuffled_sums():
    X, Y, B, intercept, rows, perm = _data(300, 5, 2, 100, 13)
    B[2] = 0.0
    X[:, 4] = 1.25
    Pred = np.asfortranarray(intercept + X @ B)
    got = V.ref_perm_sums(X, rows, Pred, Y, B, perm, t=np.float64)
    assert np.array_equal(got[2], got[5]) and np.array_equal(got[4], got[5]) and not np.array_equal(got[0], got[5])


def test_literal_viperm_matches_the_rank_one_scores():
    """The restated src/viperm.jl with a least-squares `fun`: every res[j, :, i] equals the score difference the rank-one sums give."""
    from jchemo_hip.plsr import _score_from_sums
    X, Y, _, _, _, _ = _data(200, 6, 2, 60, 14)
    n, p = X.shape
    rng = np.random.default_rng(15)
    s = [np.sort(rng.choice(n, size=67, replace=False)) for _ in range(2)]
    perms = [V.perm_matrix(100 + i, 67, p) for i in range(2)]

    def fun(Xc, Yc):
        A = np.hstack([np.ones((Xc.shape[0], 1)), Xc])
        return np.linalg.lstsq(A, Yc, rcond=None)[0]

    def predict(coefs, Xv):
        return coefs[0][None, :] + Xv @ coefs[1:]

    for name, score in V.np_scores().items():
        imp, res, score0 = V.viperm_literal(X, Y, s, perms, score, fun, predict)
        assert imp.shape == (p, 2) and res.shape == (p, 2, 2) and np.allclose(imp, res.mean(axis=2))
        for i in range(2):
            coefs = fun(V.rmrow(X, s[i]), V.rmrow(Y, s[i]))
            S = V.ref_perm_sums(X, s[i], predict(coefs, X), Y, coefs[1:], perms[i]).astype(np.float64)
            want = _score_from_sums(name, S[:p]) - _score_from_sums(name, S[p:])
            assert np.allclose(_score_from_sums(name, S[p:])[0], score0[:, i], rtol=1e-9, atol=1e-12), name
            assert np.allclose(res[:, :, i], want, rtol=1e-7, atol=1e-9 * np.abs(score0[:, i]).max()), name


# ---------------------------------------------------------------------------------------------------- isel
def test_isel_interval_bounds_round_half_to_even():
    import jchemo_hip as J
    # p = 10, nint = 4: range(1, 11; length = 5) = 1, 3.5, 6, 8.5, 11 -> 1, 4, 6, 8, 11 (3.5 -> 4, 8.5 -> 8); mids 2, 4.5 -> 4, 6.5 -> 6, 9
    want = np.array([[1, 3, 2], [4, 5, 4], [6, 7, 6], [8, 10, 9]])
    assert np.array_equal(V.isel_intervals(10, 4), want) and np.array_equal(J.isel_intervals(10, 4), want)
    # p = 7, nint = 2: 1, 4.5, 8 -> 1, 4, 8; mids 2, 5.5 -> 6
    want = np.array([[1, 3, 2], [4, 7, 6]])
    assert np.array_equal(V.isel_intervals(7, 2), want) and np.array_equal(J.isel_intervals(7, 2), want)
    for p, nint in ((10, 4), (7, 2), (101, 10), (5, 5)):
        it = V.isel_intervals(p, nint)
        assert it[0, 0] == 1 and it[-1, 1] == p and np.array_equal(it[1:, 0], it[:-1, 1] + 1)      # the intervals tile 1 .. p


def test_literal_isel_shapes():
    X, Y, _, _, _, _ = _data(60, 10, 2, 20, 16)
    s = [np.arange(0, 60, 3), np.arange(1, 60, 3)]
    sc = V.np_scores()["rmsep"]
    res, res0, res_rep, res0_rep, it = V.isel_literal(X, Y, s, 4, sc, lambda A, Yc: np.linalg.lstsq(np.hstack([np.ones((A.shape[0], 1)), A]), Yc, rcond=None)[0],
                                                      lambda c, A: c[0][None, :] + A @ c[1:])
    assert res.shape == (4, 2) and res0.shape == (1, 2) and res_rep.shape == (4, 2, 2) and res0_rep.shape == (1, 2, 2) and it.shape == (4, 3)
    assert np.all(res0 < res)            # all columns predict better than any quarter of them on this linear model


# ---------------------------------------------------------------------------------------------------- the boundary
def test_header_makefile_symbols_and_exports():
    import jchemo_hip as J
    hdr = open(os.path.join(ROOT, "include", "jchemo_hip.h")).read()
    mk = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "viperm.hip")).read()
    jl = open(os.path.join(ROOT, "jchemo.jl_amd", "julia", "JchemoHIP.jl")).read()
    assert " viperm.hip" in mk
    for name in ("jch_perm_fill", "jch_perm_score_sums"):
        assert re.search(r"JCH_API int32_t " + name + r"\(", hdr) and name in J.SYMBOLS and f'extern "C" int32_t {name}(' in src
        assert f"(:{name}, LIB)" in jl
    for word in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "rounds = 24 when b <= 12, else 8", "cycle walking"):
        assert word in hdr, word                                  # the generator's definition is in the header
    assert "atomicAdd" not in src                                 # fixed-order sums
    for name in ("viperm", "isel", "Viperm", "Isel", "perm_fill", "perm_score_sums", "isel_intervals", "PERM_SLICE_ROWS", "PERM_QGROUP"):
        assert hasattr(J, name), name
    from jchemo_hip.viperm import PERM_QGROUP, PERM_SLICE_ROWS
    assert f"#define VP_NT {PERM_SLICE_ROWS // 8}" in src and "#define VP_RPT 8" in src and f"#define VP_QG {PERM_QGROUP}" in src
    exported = re.search(r"\nexport (.*?)\n\n", jl, flags=re.S).group(1)
    assert re.search(r"\bviperm\b", exported) and re.search(r"\bisel\b", exported)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 26." in design and "jch_perm_score_sums" in design and "jch_perm_score_sums" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_viperm.py"))


def test_library_exports_the_two_entries():
    import jchemo_hip as J
    if not os.path.exists(J.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = J.load()
    assert hasattr(lib, "jch_perm_fill") and hasattr(lib, "jch_perm_score_sums")


def test_signatures_and_defaults_follow_the_reference():
    import jchemo_hip as J
    sv = inspect.signature(J.viperm)
    assert list(sv.parameters)[:2] == ["X", "Y"]
    assert {k: v.default for k, v in sv.parameters.items() if v.default is not inspect.Parameter.empty} == dict(
        perm=50, psamp=1 / 3, score=J.rmsep, seed=None, s=None, route="auto", ctx=None)                                   # src/viperm.jl:74-76
    assert sv.parameters["fun"].default is inspect.Parameter.empty and sv.parameters["fun"].kind is inspect.Parameter.KEYWORD_ONLY
    si = inspect.signature(J.isel)
    assert list(si.parameters)[:3] == ["X", "Y", "wl"]
    assert {k: v.default for k, v in si.parameters.items() if v.default is not inspect.Parameter.empty} == dict(
        wl=None, rep=1, nint=5, psamp=1 / 3, score=J.rmsep, seed=None, s=None, ctx=None)                                   # src/isel.jl:76-78
    assert [f.name for f in __import__("dataclasses").fields(J.Viperm)] == ["imp", "res"]
    assert [f.name for f in __import__("dataclasses").fields(J.Isel)] == ["res", "res0", "res_rep", "res0_rep", "int"]


def test_bad_arguments_raise_before_any_device_work():
    import jchemo_hip as J
    X, Y = np.zeros((12, 4)), np.zeros((12, 2))
    bad = [
        (J.viperm, (X, Y), dict(fun=J.plskern, nlv=1, route="quick")),
        (J.viperm, (X, Y), dict(fun=J.plskern, nlv=1, perm=0)),
        (J.viperm, (X, Y), dict(fun=J.plskern, nlv=1, perm=2.5)),
        (J.viperm, (X, Y), dict(fun=J.plskern, nlv=1, psamp=0.01)),          # nval = 0
        (J.viperm, (X, Y), dict(fun=J.plskern, nlv=1, psamp=1.0)),           # nval = n
        (J.viperm, (X, Y[:11]), dict(fun=J.plskern, nlv=1)),
        (J.viperm, (X, Y), dict(fun=J.plskern, nlv=1, perm=2, s=[np.arange(4)])),             # one list for two replications
        (J.viperm, (X, Y), dict(fun=J.plskern, nlv=1, perm=1, s=[np.array([0, 12])])),        # row 12 of 12
        (J.viperm, (X, Y), dict(fun=J.plskern, nlv=1, perm=1, s=[np.array([3, 3])])),         # a row twice
        (J.viperm, (X, Y), dict(fun=J.plskern, nlv=1, route="fast", score=lambda pr, y: 0)),  # not a named score
        (J.viperm, (X, Y), dict(fun=J.knnr, route="fast")),                                   # no coef
        (J.isel, (X, Y), dict(fun=J.plskern, nlv=1, nint=5)),                                  # 5 intervals, 4 columns
        (J.isel, (X, Y), dict(fun=J.plskern, nlv=1, nint=0)),
        (J.isel, (X, Y), dict(fun=J.plskern, nlv=1, rep=0)),
        (J.isel, (X, Y, np.arange(3)), dict(fun=J.plskern, nlv=1, nint=2)),                    # wl of 3 for 4 columns
        (J.perm_fill, (0, 3, 1), dict()),
        (J.perm_fill, (5, 0, 1), dict()),
        (J.perm_fill, (5, 3, -1), dict()),
        (J.perm_score_sums, (X, Y, Y, np.zeros((3, 2))), dict()),                              # B of 3 rows for 4 columns
        (J.perm_score_sums, (X, Y[:11], Y[:11], np.zeros((4, 2))), dict()),
        (J.perm_score_sums, (X, Y, Y, np.zeros((4, 2))), dict(perm=np.zeros((5, 4), dtype=np.int32))),
    ]
    for fn, args, kw in bad:
        with pytest.raises(ValueError):
            fn(*args, **kw)
    with pytest.raises(TypeError):
        J.viperm(X, Y, fun="plskern", nlv=1)
