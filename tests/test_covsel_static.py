"""Covsel without a GPU: the oracles, the identities the device code rests on, and the surface checks.

Oracles
  np_covsel_literal    src/covsel.jl:59-122 line by line, with the n x n projector H (dense_h=False multiplies by the rank-one factors
                       instead, x (x'X) / x'x: the same matrices up to rounding, for the shapes where n x n does not fit a quick test)
  np_covsel_postponed  the formulation of DESIGN.md §15: X is only read, Q and Yd are kept, every deflated quantity comes from Xc'[Yd | q]
  np_covselr           numpy.linalg.lstsq on the centred selected columns (what src/covselr.jl's `mlr` computes)

The literal route also reports, per step, the relative gap between the best and the second-best criterion; wherever the tests demand
equal selections they first assert that this gap is > 1e-6 (a gap at rounding level would make the argmax a coin toss in any arithmetic)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))

EPS = float(np.finfo(np.float64).eps)
EXHAUSTED = 1e-10       # the library's rule: deflated sum of squares <= 1e-10 of the original one
KEPT = 1e-8             # the tests compare `cor` entries only where the LITERAL deflated column keeps more than this share
GAP = 1e-6

# (n, p, q, nlv, level, seed): the conditioned cases; the last one runs nlv = 5 for "cor".  The seeds are the first ones for which the
# literal route meets the gap condition for both typ (with "cor" the reference itself may re-select an exhausted column: see below).
CASES = [(300, 40, 1, 8, 1.0, 3), (300, 40, 3, 8, 1.0, 1), (257, 130, 2, 12, 100.0, 1), (1000, 64, 1, 10, 1.0, 1), (65, 7, 1, 7, 1.0, 1)]


def case_nlv(case, typ):
    n, p, q, nlv, level, seed = case
    return 5 if (typ == "cor" and p == 7) else nlv


def case_id(case):
    return "n%d-p%d-q%d-nlv%d-level%g" % case[:5]


# ---------------------------------------------------------------------------------------------------- inputs
def spectra_xy(n, p, q, level, seed):
    """Six Gaussian bands on a [0, 1] grid (centres uniform in [0, 1], widths in [0.03, 0.3]), n x 6 normal scores,
    X = level + scores bands' + 0.01 noise; Y = the first q scores mixed by a random q x q matrix + 0.05 noise + 3 (for q > 6 the score
    table is continued with columns X knows nothing of)."""
    rng = np.random.default_rng(seed)
    grid = np.linspace(0.0, 1.0, p) if p > 1 else np.array([0.5])
    cen, wid = rng.uniform(0.0, 1.0, 6), rng.uniform(0.03, 0.3, 6)
    bands = np.exp(-0.5 * ((grid[:, None] - cen[None, :]) / wid[None, :]) ** 2)
    S = rng.standard_normal((n, max(6, q)))
    X = level + S[:, :6] @ bands.T + 0.01 * rng.standard_normal((n, p))
    Y = S[:, :q] @ rng.standard_normal((q, q)) + 0.05 * rng.standard_normal((n, q)) + 3.0
    return np.asfortranarray(X), np.asfortranarray(Y)


# ---------------------------------------------------------------------------------------------------- oracles
def _jl_cov(X, Y):
    """cov(X, Y; corrected = false): Statistics centres both arguments itself."""
    return (X - X.mean(0)).T @ (Y - Y.mean(0)) / X.shape[0]


def _jl_cor(X, Y):
    Xc, Yc = X - X.mean(0), Y - Y.mean(0)
    with np.errstate(all="ignore"):
        return (Xc.T @ Yc) / np.sqrt((Xc ** 2).sum(0))[:, None] / np.sqrt((Yc ** 2).sum(0))[None, :]


def _gap(z):
    """Relative gap between the largest and the second largest finite entry of z (inf with fewer than two)."""
    f = np.sort(z[np.isfinite(z)])
    if f.size < 2 or f[-1] <= 0:
        return np.inf if f.size < 2 else 0.0
    return (f[-1] - f[-2]) / f[-1]


def np_covsel_literal(X, Y, nlv=None, typ="cov", dense_h=True):
    """src/covsel.jl:59-122.  Returns a dict: sel (0-based), selcov, cov2, C, cumpvarx, cumpvary, xmeans, ymeans, yscales, the deflated X and
    Y the reference leaves behind, and per step `gap` (see the module docstring) and `kept` (p x nlv: the share of its original sum of
    squares each deflated column holds when step i is judged)."""
    X = np.array(X, dtype=np.float64, copy=True)
    Y = np.array(Y, dtype=np.float64, copy=True).reshape(X.shape[0], -1)
    n, p = X.shape
    q = Y.shape[1]
    nlv = p if nlv is None else nlv                                   # :63
    xmeans, ymeans = X.mean(0), Y.mean(0)                             # :64-65
    X -= xmeans; Y -= ymeans                                          # :66-67
    yscales = np.ones(q)
    if q > 1:                                                         # :68-70
        yscales = np.sqrt((Y ** 2).mean(0))
        Y /= yscales
    css0 = (X ** 2).sum(0)
    xsstot, ysstot = (X ** 2).sum(), (Y ** 2).sum()                   # :71-72
    xss, yss = np.zeros(nlv), np.zeros(nlv)
    selvar = np.zeros(nlv, dtype=np.int64)
    selcov, cov2, Cm = np.zeros(nlv), np.zeros(p), np.zeros((p, nlv))
    gap, kept = np.zeros(nlv), np.zeros((p, nlv))
    with np.errstate(all="ignore"):
        for i in range(nlv):                                          # :81
            zcov = _jl_cov(X, Y) if typ == "cov" else _jl_cor(X, Y)   # :83 / :87
            z = (zcov ** 2).sum(1)                                    # :84 / :88
            kept[:, i] = (X ** 2).sum(0) / css0
            gap[i] = _gap(z)
            Cm[:, i] = z                                              # :105
            zsel = int(np.nanargmax(z)) if np.isfinite(z).any() else 0   # :106 (Julia's argmax would return a NaN's index)
            selvar[i] = zsel; selcov[i] = z[zsel]; cov2[zsel] = z[zsel]   # :107-109
            x = X[:, zsel].copy()                                     # :110
            if dense_h:
                H = np.outer(x, x) / (x @ x)                          # :111
                X -= H @ X; Y -= H @ Y                                # :112-113
            else:
                X -= np.outer(x, (x @ X) / (x @ x)); Y -= np.outer(x, (x @ Y) / (x @ x))
            xss[i], yss[i] = (X ** 2).sum(), (Y ** 2).sum()           # :114-115
    return dict(sel=selvar, selcov=selcov, cov2=cov2, C=Cm, cumpvarx=1 - xss / xsstot, cumpvary=1 - yss / ysstot, xmeans=xmeans, ymeans=ymeans,
                yscales=yscales, X=X, Y=Y, gap=gap, kept=kept)


def np_covsel_postponed(X, Y, nlv=None, typ="cov"):
    """DESIGN.md §15 in numpy: X is never written.  Also returns G = Xc'Q, QtY = Q'Yc (scaled units), Q, nlv_out and the deflated X, Y as
    `covsel!` hands them back (Xc - Q G', Yd)."""
    X = np.asarray(X, dtype=np.float64)
    Y = np.asarray(Y, dtype=np.float64).reshape(X.shape[0], -1)
    n, p = X.shape
    q = Y.shape[1]
    nlv = p if nlv is None else min(nlv, p)
    xmeans, ymeans = X.mean(0), Y.mean(0)
    Xc, Yd = X - xmeans, Y - ymeans
    yscales = np.ones(q)
    if q > 1:
        yscales = np.sqrt((Yd ** 2).mean(0))
        Yd = Yd / yscales
    css0 = (Xc ** 2).sum(0)
    css = css0.copy()
    xsstot, ysstot = css0.sum(), (Yd ** 2).sum()
    Q, G, QtY = np.zeros((n, nlv)), np.zeros((p, nlv)), np.zeros((nlv, q))
    sel, selcov, cov2, Cm = np.zeros(nlv, dtype=np.int64), np.zeros(nlv), np.zeros(p), np.zeros((p, nlv))
    xss, yss = np.zeros(nlv), np.zeros(nlv)
    done = 0
    with np.errstate(all="ignore"):
        for i in range(nlv):
            K = Xc.T @ Yd                                             # = Xd'Yd: Yd is orthogonal to Q
            if typ == "cov":
                z = ((K / n) ** 2).sum(1)
            else:
                z = np.where(css > EXHAUSTED * css0, (K ** 2 / (css[:, None] * (Yd ** 2).sum(0)[None, :])).sum(1), 0.0)
            Cm[:, i] = z
            j = int(np.nanargmax(z)) if np.isfinite(z).any() else 0
            xd = Xc[:, j] - Q[:, :i] @ G[j, :i]
            xd = xd - Q[:, :i] @ (Q[:, :i].T @ xd)                    # the second Gram-Schmidt sweep
            nrm2 = xd @ xd
            if not nrm2 > EXHAUSTED * css0[j]:
                break
            sel[i], selcov[i], cov2[j] = j, z[j], z[j]
            Q[:, i] = xd / np.sqrt(nrm2)
            QtY[i] = Q[:, i] @ Yd
            Yd = Yd - np.outer(Q[:, i], QtY[i])
            G[:, i] = Xc.T @ Q[:, i]
            css = css - G[:, i] ** 2
            xss[i], yss[i] = css.sum(), (Yd ** 2).sum()
            done = i + 1
    return dict(sel=sel[:done], selcov=selcov[:done], cov2=cov2, C=Cm[:, :done], cumpvarx=(1 - xss / xsstot)[:done], cumpvary=(1 - yss / ysstot)[:done],
                xmeans=xmeans, ymeans=ymeans, yscales=yscales, G=G[:, :done], QtY=QtY[:done], Q=Q[:, :done], nlv_out=done,
                X=Xc - Q[:, :done] @ G[:, :done].T, Y=Yd)


def np_covselr(X, Y, sel):
    """`mlr(X[:, sel], Y)`: least squares with an intercept.  Returns (B, int)."""
    Y = np.asarray(Y, dtype=np.float64).reshape(X.shape[0], -1)
    Z = X[:, sel]
    zm, ym = Z.mean(0), Y.mean(0)
    B = np.linalg.lstsq(Z - zm, Y - ym, rcond=None)[0]
    return B, ym[None, :] - zm[None, :] @ B


def covselr_from_parts(res):
    """B and int from what jch_covsel_fit returns: R[k, i] = G[sel_i, k], B = R^-1 Q'Yc rescaled to the raw Y."""
    s = res["sel"]
    R = np.triu(res["G"][s, :].T)
    B = np.linalg.solve(R, res["QtY"]) * res["yscales"][None, :]
    return B, res["ymeans"][None, :] - res["xmeans"][s][None, :] @ B


def excluded(lit, i):
    """Columns of C[:, i] (`cor`) that are not compared: those whose literal deflated column kept <= KEPT of its sum of squares."""
    return np.flatnonzero(~(lit["kept"][:, i] > KEPT))


_memo = {}


def routes(case, typ):
    """(X, Y, literal, postponed) of a conditioned case, computed once per session and never modified."""
    key = (case, typ)
    if key not in _memo:
        n, p, q, nlv, level, seed = case
        X, Y = spectra_xy(n, p, q, level, seed)
        k = case_nlv(case, typ)
        out = (X, Y, np_covsel_literal(X, Y, k, typ), np_covsel_postponed(X, Y, k, typ))
        for a in (X, Y):
            a.setflags(write=False)
        _memo[key] = out
    return _memo[key]


def cpu_gap(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)))) if np.size(a) else 0.0


GRID = [pytest.param(c, t, id=case_id(c) + "-" + t) for c in CASES for t in ("cov", "cor")]


# ---------------------------------------------------------------------------------------------------- the two routes
@pytest.mark.parametrize("case,typ", GRID)
def test_literal_and_postponed_select_the_same_variables(case, typ):
    X, Y, lit, post = routes(case, typ)
    k = case_nlv(case, typ)
    print("gaps", np.array2string(lit["gap"], precision=2))
    assert lit["gap"].min() > GAP                 # the condition under which the GPU test may demand equal selections at every step
    assert post["nlv_out"] == k
    assert np.array_equal(lit["sel"], post["sel"])
    assert len(set(lit["sel"])) == k


@pytest.mark.parametrize("case,typ", GRID)
def test_postponed_reproduces_the_literal_numbers(case, typ):
    X, Y, lit, post = routes(case, typ)
    k = case_nlv(case, typ)
    for i in range(k):
        keep = np.ones(X.shape[1], dtype=bool)
        if typ == "cor":
            ex = excluded(lit, i)
            assert sorted(ex) == sorted(lit["sel"][:i])       # exactly the i previously selected columns: the cap on what is left out
            keep[ex] = False
        ref = lit["C"][keep, i]
        assert np.max(np.abs(post["C"][keep, i] - ref)) <= 1e-9 * np.max(np.abs(ref)), i
    for f in ("selcov", "cumpvarx", "cumpvary"):
        assert np.allclose(post[f], lit[f], rtol=1e-9, atol=1e-13), f
    scale = np.max(np.abs(X - X.mean(0)))
    assert np.max(np.abs(post["X"] - lit["X"])) <= 1e-10 * scale
    assert np.max(np.abs(post["Y"] - lit["Y"])) <= 1e-10 * np.max(np.abs(lit["Y"]) + 1)
    Q = post["Q"]
    assert np.max(np.abs(Q.T @ Q - np.eye(k))) < 50 * EPS * k


def test_the_excluded_cor_entries_are_noise_in_the_reference():
    """The documented deviation: for an already selected column the reference's `cor` is rounding noise over rounding noise.  The literal
    values there are O(1) numbers unrelated to the data (the postponed route sets them to 0), and they can be large enough to matter."""
    worst = 0.0
    for case in CASES:
        X, Y, lit, post = routes(case, "cor")
        for i in range(1, case_nlv(case, "cor")):
            ex = excluded(lit, i)
            assert np.all(post["C"][ex, i] == 0.0)
            with np.errstate(all="ignore"):
                worst = max(worst, float(np.nanmax(np.abs(lit["C"][ex, i] - post["C"][ex, i]) / lit["selcov"][i])))
    print("largest literal `cor` value of an exhausted column / the step's winning value:", worst)
    assert worst > 1e-3      # not a rounding-level difference: noise of the size of the criterion itself


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_covselr_from_the_triangular_factor_equals_lstsq(case):
    X, Y, lit, post = routes(case, "cov")
    B, b0 = covselr_from_parts(post)
    Bref, b0ref = np_covselr(X, Y, post["sel"])
    tol = 1e-8 * max(1.0, np.max(np.abs(Bref)))
    assert np.max(np.abs(B - Bref)) <= tol and np.max(np.abs(b0 - b0ref)) <= tol * max(1.0, np.max(np.abs(X)))
    R = post["G"][post["sel"], :].T
    assert np.max(np.abs(np.tril(R, -1))) <= 1e-10 * np.max(np.abs(R))          # upper triangular up to rounding


def test_rank_deficient_input_stops_early_in_the_postponed_route():
    X, Y = spectra_xy(65, 7, 1, 1.0, 5)
    X = np.array(X); X[:, 4] = X[:, 1]
    post = np_covsel_postponed(X, Y, 7, "cov")
    assert post["nlv_out"] < 7 and np.isfinite(post["C"]).all() and np.isfinite(post["cumpvarx"]).all()


# ---------------------------------------------------------------------------------------------------- surface
def test_header_declares_the_entry_and_the_constants():
    h = open(os.path.join(ROOT, "include", "jchemo_hip.h")).read()
    assert re.search(r"#define JCH_COVSEL_COV 0\b", h) and re.search(r"#define JCH_COVSEL_COR 1\b", h)
    m = re.search(r"JCH_API int32_t jch_covsel_fit\(([^;]*)\);", h)
    assert m
    params = [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in params] == ["ctx", "loc", "X", "n", "p", "ldx", "Y", "q", "ldy", "nlv", "typ", "inplace", "sel", "selcov", "cov2",
                                                           "C", "cumpvarx", "cumpvary", "xmeans", "ymeans", "yscales", "G", "QtY", "Q", "nlv_out"]
    assert "src/covsel.jl:59-122" in h and "src/covselr.jl:48-53" in h          # the header cites the reference lines, like its neighbours
    import jchemo_hip as J
    assert "jch_covsel_fit" in J.SYMBOLS


def test_python_exports_and_signatures():
    import inspect
    import jchemo_hip as J
    for name in ("covsel", "covsel_", "covselr", "Covsel", "Covselr"):
        assert hasattr(J, name), name
    assert list(inspect.signature(J.covsel).parameters) == ["X", "Y", "nlv", "typ", "ctx"]
    assert list(inspect.signature(J.covsel_).parameters) == ["X", "Y", "nlv", "typ", "ctx"]
    assert list(inspect.signature(J.covselr).parameters)[:4] == ["X", "Y", "nlv", "typ"]
    assert inspect.signature(J.covsel).parameters["nlv"].default is None and inspect.signature(J.covsel).parameters["typ"].default == "cov"
    assert inspect.signature(J.covselr).parameters["nlv"].default is inspect.Parameter.empty       # src/covselr.jl:48: nlv has no default
    assert [f for f in J.Covsel.__dataclass_fields__][:3] == ["sel", "cov2", "C"]                 # src/covsel.jl:121
    assert [f for f in J.Covselr.__dataclass_fields__] == ["fm", "sel", "cov2"]                   # src/covselr.jl:1-5


def test_julia_module_exports_the_names_with_the_reference_keywords():
    src = open(os.path.join(ROOT, "jchemo.jl_amd", "julia", "JchemoHIP.jl")).read()
    exported = set(re.findall(r"[\w!]+", re.search(r"\nexport (.*?)\n\n", src, flags=re.S).group(1)))
    assert {"covsel", "covsel!", "covselr", "Covsel", "Covselr"} <= exported
    assert re.search(r"\nfunction covsel\(X, Y; nlv = nothing, typ = \"cov\", ctx", src)            # src/covsel.jl:54
    assert re.search(r"\nfunction covsel!\(X, Y; nlv = nothing, typ = \"cov\", ctx", src)        # :59-60 (any column-major array, device ones included)
    assert re.search(r"\nfunction covselr\(X, Y; nlv, typ = \"cov\", ctx", src)                     # src/covselr.jl:48
    assert re.search(r"\nfunction predict\(object::Covselr, X", src)                               # src/covselr.jl:61
    assert "(:jch_covsel_fit, LIB)" in src
    assert "Int64.(sel)[1:k] .+ 1" in src                                                          # 1-based indices on the Julia side


def test_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    X, Y = np.zeros((10, 4)), np.zeros((10, 2))
    with pytest.raises(ValueError, match="typ"):
        J.covsel(X, Y, nlv=2, typ="aic")
    with pytest.raises(ValueError, match="DimensionMismatch"):
        J.covsel(X, np.zeros((9, 2)), nlv=2)
    with pytest.raises(ValueError, match="nlv"):
        J.covsel(X, Y, nlv=0)
    with pytest.raises(ValueError, match="nlv"):
        J.covsel(X, Y, nlv=1.5)
    with pytest.raises(ValueError, match="nlv"):
        J.covselr(X, Y, None)
    with pytest.raises(TypeError):
        J.covselr(X, Y)
    with pytest.raises((ValueError, TypeError)):
        J.covsel_(np.zeros((10, 4), order="C"), Y, nlv=2)          # in place needs the caller's column-major storage


def test_no_cpu_fallback_without_gpu():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import jchemo_hip as J
    X, Y = spectra_xy(20, 5, 1, 1.0, 0)
    for call in (lambda: J.covsel(X, Y, nlv=2), lambda: J.covselr(X, Y, 2), lambda: J.covsel_(np.array(X, order="F"), np.array(Y, order="F"), nlv=2)):
        with pytest.raises(J.JchError) as ei:
            call()
        assert ei.value.code == J._lib.JCH_ENODEV


def test_design_records_the_deviation_and_labels_its_figures():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    beg = text.index("## 15.")
    part = text[beg:]
    part = part[:part.index("\n## ", 4)]
    assert "1e-10" in part and "unpinned" in part.lower()
    assert "[measured]" in part.splitlines()[0] or "[not measured]" in part.splitlines()[0]      # the heading says which kind of figures follow
