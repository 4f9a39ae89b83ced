"""Calibration transfer without a GPU: the header's new mode flag, `pds_table` against a literal restatement of src/calpds.jl:70-77, the
mlr family on its host route against numpy restatements of src/mlr.jl, `eposvd`, `difmean`, and the per-element bound the GPU tests
hold the per-column FIR mode to.

Tolerances.  eps = 2^-52.
  mlr family   max |B - B_ref| <= 50 eps cond_kept |B|_2, cond_kept = sv_1 / (smallest kept sv) of the matrix the function decomposes
               (sqrtD Xc for mlr / mlrpinv, Xc'D Xc for mlrchol / mlrpinvn): the first-order perturbation bound of a least-squares
               solution whose rank decision is not in doubt.  That last clause is a condition on the INPUTS: no singular ratio of a tested
               matrix lies within a factor 1e3 of the truncation threshold sqrt(eps); `_ratios_clear` asserts it on every matrix used.
  FIR mode     for output (i, j) with K nonzero taps, |err| <= (K + 2) 2^-53 (|c_j| + sum_t |taps[t, j]| |x|): K products, K - 1 additions
               of the running sum and the final addition of the constant, each rounding once (standard model, first order; one spare
               unit).  Evaluating in float64 in the header's order, with or without fused multiply-adds, must stay within HALF of it, so
               that a compiler's choice between the two cannot decide a GPU test."""
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))

import jchemo_hip as J  # noqa: E402
from jchemo_hip import caltransfer as CT  # noqa: E402

EPS = float(np.finfo(np.float64).eps)
THR = float(np.sqrt(EPS))
HEADER = os.path.join(ROOT, "include", "jchemo_hip.h")

# the grid of the GPU tests (tests/test_gpu_caltransfer.py)
FIR_NS = [1, 63, 64, 65, 130]          # the wave edge
FIR_PS = [1, 2, 7, 8, 9, 33]           # the RP_U chunk edges
FIR_FS = [1, 3, 11, 57, 58, 40]        # ... 57 the last ring size, 58 the wide path, 40 > every p


def fir_los(f):
    return sorted({0, -((f - 1) // 2), -(f - 1)})


# ---------------------------------------------------------------------------------- shared data
def standards(seed=20251021, n=40, p=33):
    """(X, Xt): Xt = n standards of three Gaussian bands plus 1e-3 noise; X = Xt shifted by one column, scaled by 1.05, plus 0.02 and noise."""
    rng = np.random.default_rng(seed)
    z = np.arange(float(p))
    amp = rng.uniform(0.5, 1.5, (n, 3))
    bands = np.stack([np.exp(-0.5 * ((z - c) / w) ** 2) for c, w in ((8.0, 3.0), (17.0, 4.0), (26.0, 2.5))])
    Xt = amp @ bands + 1e-3 * rng.standard_normal((n, p))
    X = np.empty_like(Xt)
    X[:, 1:], X[:, 0] = Xt[:, :-1], Xt[:, 0]
    X = 1.05 * X + 0.02 + 1e-3 * rng.standard_normal((n, p))
    return np.asfortranarray(X), np.asfortranarray(Xt)


def library(seed, m, p=33):
    """m spectra of the second instrument to standardise (the same bands, other amplitudes)."""
    rng = np.random.default_rng(seed)
    z = np.arange(float(p))
    bands = np.stack([np.exp(-0.5 * ((z - c) / w) ** 2) for c, w in ((8.0, 3.0), (17.0, 4.0), (26.0, 2.5))])
    return np.asfortranarray(1.05 * (rng.uniform(0.3, 1.7, (m, 3)) @ bands) + 0.02 + 1e-3 * rng.standard_normal((m, p)))


def fir_case(n, p, f, lo, seed=0):
    """(X n x p, table (f + 1) x p): random taps and constants.  Even columns are zero-padded as `pds_table` pads a border window (no tap
    on a column outside 0 .. p - 1), odd columns keep theirs (the clamped reads count), and one tap in ten is an exact zero anywhere."""
    rng = np.random.default_rng([n, p, f, -lo, seed])
    X = np.asfortranarray(rng.standard_normal((n, p)) * 10.0 ** rng.integers(-2, 3, (n, 1)))
    tab = rng.standard_normal((f + 1, p))
    tab[:f][rng.random((f, p)) < 0.1] = 0.0
    for j in range(0, p, 2):
        src = j + lo + np.arange(f)
        tab[:f, j][(src < 0) | (src > p - 1)] = 0.0
    return X, np.asfortranarray(tab)


def fir_ref(X, tab, lo):
    """(reference in longdouble, bound): out[i, j] = sum_t tab[t, j] x[i, clamp(j + lo + t)] + tab[f, j] and (K + 2) 2^-53 (|c_j| + sum |w||x|)."""
    n, p = X.shape
    f = tab.shape[0] - 1
    ref = np.zeros((n, p), dtype=np.longdouble)
    mag = np.zeros((n, p))
    with np.errstate(all="ignore"):
        for j in range(p):
            for t in range(f):
                w = tab[t, j]
                if w != 0.0:
                    x = X[:, min(max(j + lo + t, 0), p - 1)]
                    ref[:, j] += np.longdouble(w) * x.astype(np.longdouble)
                    mag[:, j] += abs(w) * np.abs(x)
            ref[:, j] += np.longdouble(tab[f, j])
            mag[:, j] += abs(tab[f, j])
    K = np.count_nonzero(tab[:f], axis=0)
    return ref, (K + 2)[None, :] * 2.0 ** -53 * mag


def fir_f64(X, tab, lo, fused):
    """The float64 evaluation in the header's order: from 0.0, the taps in the order of t, zero taps skipped, the constant last; `fused` rounds
    w x + acc once (exactly, through rationals), otherwise the product and the sum round separately."""
    n, p = X.shape
    f = tab.shape[0] - 1
    out = np.empty((n, p))
    for i in range(n):
        for j in range(p):
            acc = 0.0
            for t in range(f):
                w = float(tab[t, j])
                if w != 0.0:
                    x = float(X[i, min(max(j + lo + t, 0), p - 1)])
                    acc = float(Fraction(w) * Fraction(x) + Fraction(acc)) if fused else acc + w * x
            out[i, j] = acc + float(tab[f, j])
    return out


# ---------------------------------------------------------------------------------- the header
def test_header_flag_comment_and_exports():
    h = open(HEADER).read()
    assert re.search(r"#define\s+JCH_FIR_PER_COLUMN\s+4\b", h)
    assert re.search(r"#define\s+JCH_FIR_SAME\s+0\b", h) and re.search(r"#define\s+JCH_FIR_VALID\s+1\b", h)
    doc = h[h.index(" * jch_rows_fir"):h.index("#define JCH_FIR_SAME")]
    flat = " ".join(doc.replace("*", " ").split())
    assert "JCH_FIR_PER_COLUMN" in flat
    assert "(f + 1) x p doubles, column-major with ld f + 1" in flat and "followed by its constant c_j" in flat          # the table layout
    assert "summed in the order of t, starting from 0.0, and the constant is added last" in flat                          # the summation order
    assert "exactly 0.0 is skipped" in flat
    assert "JCH_FIR_VALID | JCH_FIR_PER_COLUMN" in flat and "JCH_EINVAL" in flat
    exports = sorted(re.findall(r"JCH_API\s+[\w\s\*]+?\b(jch_\w+)\s*\(", h))
    assert exports == sorted(J.SYMBOLS)
    assert CT.FIR_PER_COLUMN == 4 and (CT.FIR_SAME | CT.FIR_PER_COLUMN) == 4


# ---------------------------------------------------------------------------------- pds_table
def restate_windows(p, m):
    """src/calpds.jl:70-77 with Julia's 1-based ranges written out; returns the 1-based windows."""
    zm = [m] * p
    first = list(range(1, m + 1))                 # zm[1:m] .= collect(1:m) .- 1
    for k, idx in enumerate(first):
        zm[idx - 1] = (k + 1) - 1
    second = list(range(p - m + 1, p + 1))        # zm[(p - m + 1):p] .= collect(m:-1:1) .- 1
    for k, idx in enumerate(second):
        if idx < 1:
            raise IndexError("BoundsError")
        zm[idx - 1] = (m - k) - 1
    s = []
    for i in range(1, p + 1):
        s.append(list(range(i - zm[i - 1], i + zm[i - 1] + 1)))
        if s[-1][0] < 1 or s[-1][-1] > p:
            raise IndexError("BoundsError")
    return s


@pytest.mark.parametrize("p,m", [(1, 0), (3, 2), (7, 3), (33, 3), (9, 0)])
def test_pds_table_against_the_restatement(p, m):
    ref = restate_windows(p, m)
    zm, s = J.pds_windows(p, m)
    assert [list(si + 1) for si in s] == ref
    assert [len(w) for w in ref] == [2 * z + 1 for z in zm]
    rng = np.random.default_rng(p * 100 + m)
    coefs = [(rng.standard_normal((len(si), 1)), rng.standard_normal((1, 1))) for si in s]
    tab, f, lo = J.pds_table(coefs, s, m)
    assert (f, lo) == (2 * m + 1, -m) and tab.shape == (f + 1, p) and tab.flags.f_contiguous
    want = np.zeros((f + 1, p))
    for i, w in enumerate(ref):                   # output i reads the columns w through taps[t] <-> column i + lo + t
        for u, col in enumerate(w):
            want[(col - 1) - (i + lo), i] = coefs[i][0][u, 0]
        want[f, i] = coefs[i][1][0, 0]
    assert np.array_equal(tab, want)
    assert np.count_nonzero(tab[:f]) == sum(len(w) for w in ref)    # exact zeros everywhere else


def test_pds_windows_override_and_errors():
    assert [list(si) for si in J.pds_windows(3, 2)[1]] == [[0], [0, 1, 2], [2]]      # p < 2m: zm = [0, 1, 2] becomes [0, 1, 0], the second assignment overrides the first
    for p, m in [(4, 3), (2, 3), (1, 2)]:
        with pytest.raises(IndexError):
            restate_windows(p, m)
        with pytest.raises(ValueError):
            J.pds_windows(p, m)
    X, Xt = standards()
    with pytest.raises(ValueError):
        J.calpds(X[:, :4], Xt[:, :4], m=3)


# ---------------------------------------------------------------------------------- the mlr family
def np_mweight(w, n):
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    return w / w.sum()


def np_mlr(kind, X, Y, weights=None, noint=False):
    """src/mlr.jl restated: (B, int, the matrix the function decomposes)."""
    X, Y = np.array(X, dtype=np.float64), np.array(Y, dtype=np.float64).reshape(X.shape[0], -1)
    w = np_mweight(weights, X.shape[0])
    if noint:
        xm, ym = np.zeros(X.shape[1]), np.zeros(Y.shape[1])
    else:
        xm, ym = w @ X, w @ Y
    Xc, Yc = X - xm, Y - ym
    sq = np.sqrt(w)[:, None]
    if kind == "mlr":
        A = sq * Xc
        B = np.linalg.lstsq(A, sq * Yc, rcond=None)[0]
    elif kind == "mlrpinv":
        A = sq * Xc
        B = np.linalg.pinv(A, rcond=THR) @ (sq * Yc)
    elif kind == "mlrchol":
        XtD = Xc.T * w
        A = XtD @ Xc
        L = np.linalg.cholesky(A)
        B = np.linalg.solve(L.T, np.linalg.solve(L, XtD @ Yc))
    elif kind == "mlrpinvn":
        XtD = Xc.T * w
        A = XtD @ Xc
        B = np.linalg.pinv(A, rcond=THR) @ (XtD @ Yc)
    else:
        xtD = Xc.T * w
        A = xtD @ Xc
        B = (xtD @ Yc) / A
    return B, ym[None, :] - xm[None, :] @ B, A


def _ratios_clear(A):
    """No singular ratio of A within a factor 1e3 of sqrt(eps); returns cond_kept."""
    sv = np.linalg.svd(A, compute_uv=False)
    r = sv / sv[0]
    assert not np.any((r > THR / 1e3) & (r < THR * 1e3)), f"a singular ratio near the truncation threshold: {r}"
    return float(1.0 / r[r >= THR * 1e3].min())


def _weights(which, n):
    rng = np.random.default_rng(7)
    if which == "none":
        return None
    w = rng.uniform(0.5, 2.0, n)
    if which == "zeros":
        w[::5] = 0.0
    return w


WIN = list(range(10, 17))      # one interior window of m = 3: what calpds fits
SPREAD = [4, 16, 28]           # three well-separated columns: the Gram keeps its ratios clear of the threshold too
FUNS = {"mlr": (WIN, True), "mlrpinv": (WIN, True), "mlrchol": (SPREAD, False), "mlrpinvn": (SPREAD, False), "mlrvec": ([16], True)}


@pytest.mark.parametrize("wkind", ["none", "random", "zeros"])
@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("kind", list(FUNS))
def test_mlr_family_host_route(kind, q, wkind):
    X, Xt = standards()
    cols, has_noint = FUNS[kind]
    Xs, Y = X[:, cols], Xt[:, 15:15 + q]
    w = _weights(wkind, X.shape[0])
    for noint in ([False, True] if has_noint else [False]):
        kw = dict(noint=True) if noint else {}
        fm = getattr(J, kind)(Xs, Y, w, **kw)
        B, b0, A = np_mlr(kind, Xs, Y, w, noint)
        cond = _ratios_clear(A)
        tol = 50 * EPS * cond * np.linalg.norm(B, 2)
        err = float(np.abs(fm.B - B).max())
        print(f"  {kind} q={q} w={wkind} noint={noint}: cond_kept {cond:.3g}, max |dB| {err:.3e}, tol {tol:.3e}")
        assert fm.B.shape == (len(cols), q) and fm.int.shape == (1, q)
        assert err <= tol
        assert np.abs(fm.int - b0).max() <= tol * (1.0 + np.abs(Xs).max() * len(cols))
        assert np.allclose(fm.weights, np_mweight(w, X.shape[0]), rtol=4 * EPS, atol=0) and abs(fm.weights.sum() - 1.0) < 1e-14
        if noint:
            assert np.array_equal(fm.int, np.zeros((1, q)))
        Bc, ic = J.coef(fm)
        assert Bc is fm.B and ic is fm.int


def test_mlr_rank_deficient_duplicated_column():
    X, Xt = standards()
    Xd = np.asfortranarray(X[:, SPREAD + [SPREAD[1]]])
    Y = Xt[:, 15:18]
    for kind in ("mlrpinv", "mlrpinvn"):
        fm = getattr(J, kind)(Xd, Y)
        B, b0, A = np_mlr(kind, Xd, Y)
        sv = np.linalg.svd(A, compute_uv=False)
        assert sv[-1] / sv[0] < THR / 1e3                                    # the dropped ratio is far below the threshold ...
        cond = _ratios_clear(A)                                              # ... and the kept ones far above
        tol = 50 * EPS * cond * np.linalg.norm(B, 2)
        assert np.abs(fm.B - B).max() <= tol
        assert np.abs(fm.B[1] - fm.B[3]).max() <= tol                        # minimum norm: the twins share their coefficient
        full = np_mlr(kind, X[:, SPREAD], Y)[0]
        assert np.abs(fm.B[1] + fm.B[3] - full[1]).max() <= 50 * EPS * cond * np.linalg.norm(full, 2)
    # mlrchol raises as numpy's Cholesky does.  On an exactly singular Gram the last pivot is a rounding residue of either sign, so whether
    # LAPACK refuses depends on the data: here it does (asserted on the restatement), and on every other layout the two must agree.
    with pytest.raises(np.linalg.LinAlgError):
        np_mlr("mlrchol", Xd, Y)
    with pytest.raises(np.linalg.LinAlgError):
        J.mlrchol(Xd, Y)
    for cols in ([4, 16, 28, 4], [4, 4, 16, 28], [4, 16, 28, 28], [4, 16, 16, 28]):
        for wkind in ("none", "random"):
            w = _weights(wkind, X.shape[0])
            try:
                want = np_mlr("mlrchol", X[:, cols], Y, w)[0]
            except np.linalg.LinAlgError:
                want = None
            if want is None:
                with pytest.raises(np.linalg.LinAlgError):
                    J.mlrchol(X[:, cols], Y, w)
            else:
                J.mlrchol(X[:, cols], Y, w)
    with pytest.raises(np.linalg.LinAlgError):
        J.mlr(Xd, Y)                                                         # the unpivoted QR refuses it (use mlrpinv)


def test_mlr_argument_rules_and_inplace_forms():
    X, Xt = standards()
    with pytest.raises(ValueError):
        J.mlrchol(X[:, :1], Xt[:, :1])
    with pytest.raises(ValueError):
        J.mlrvec(X[:, :2], Xt[:, :1])
    with pytest.raises(ValueError):
        J.mlr(X[:5], Xt[:6, :1])
    with pytest.raises(TypeError):
        J.mlrchol(X[:, :3], Xt[:, :1], noint=True)                           # no such keyword in the reference either
    for kind in FUNS:
        cols = FUNS[kind][0]
        Xa, Ya = np.array(X[:, cols], order="F"), np.array(Xt[:, 15:17], order="F")
        Xb, Yb = Xa.copy(order="F"), Ya.copy(order="F")
        f0 = getattr(J, kind)(Xa, Ya)
        assert np.array_equal(Xa, Xb) and np.array_equal(Ya, Yb)             # the plain form only reads
        f1 = getattr(J, kind + "_")(Xb, Yb)
        assert np.array_equal(f0.B, f1.B) and np.array_equal(f0.int, f1.int)
        w = np.full(Xa.shape[0], 1.0 / Xa.shape[0])
        assert np.array_equal(Xb, Xa - (w @ Xa)[None, :]) and np.array_equal(Yb, Ya - (w @ Ya)[None, :])   # centred in place, as the `!`
    Xb, Yb = np.array(X[:, WIN], order="F"), np.array(Xt[:, 15:17], order="F")
    J.mlrpinv_(Xb, Yb, noint=True)
    assert np.array_equal(Xb, X[:, WIN]) and np.array_equal(Yb, Xt[:, 15:17])                              # noint: nothing to centre


def test_mlr_beyond_the_host_route_names_the_normal_equations(monkeypatch):
    X, Xt = standards()
    monkeypatch.setattr(CT, "HOST_ROUTE_MAX", 50)
    for fn, kw in ((J.mlr, {}), (J.mlrpinv, {}), (J.mlrvec, dict(noint=True))):
        with pytest.raises(NotImplementedError, match="mlrchol / mlrpinvn"):
            fn(X[:, :1] if fn is J.mlrvec else X[:, WIN], Xt[:, :1], **kw)


# ---------------------------------------------------------------------------------- calds / calpds records
def test_calds_and_calpds_fits_on_the_host():
    X, Xt = standards()
    ds = J.calds(X[:, SPREAD], Xt[:, SPREAD], fun="mlrpinv")
    assert isinstance(ds, J.CalDs) and np.array_equal(ds.fm.B, J.mlrpinv(X[:, SPREAD], Xt[:, SPREAD]).B)
    with pytest.raises(ValueError):
        J.calds(X, Xt, fun="no_such_function")
    pds = J.calpds(X, Xt, m=3)
    assert isinstance(pds, J.CalPds) and len(pds.fm) == 33 and [list(s + 1) for s in pds.s] == restate_windows(33, 3)
    for i in (0, 2, 16, 31):
        B, b0, A = np_mlr("mlrpinv", X[:, pds.s[i]], Xt[:, i])
        cond = _ratios_clear(A)
        assert np.abs(pds.fm[i].B - B).max() <= 50 * EPS * cond * np.linalg.norm(B, 2)
    with pytest.raises(ValueError):
        J.calpds_predict(pds, X, nlv=[1, 2])
    with pytest.raises(ValueError):
        J.calpds_predict(pds, X[:, :5])


# ---------------------------------------------------------------------------------- eposvd, difmean
def test_eposvd():
    X, Xt = standards()
    D = (X - Xt)[:5]
    M, P = J.eposvd(D, nlv=5)
    assert M.shape == (33, 33) and P.shape == (33, 5)
    assert np.abs(M - M.T).max() <= 4 * EPS and np.abs(M @ M - M).max() <= 64 * EPS          # symmetric, idempotent
    assert np.abs(D @ M).max() <= 64 * EPS * np.linalg.norm(D, 2)                              # nlv = rank: nothing of D is left
    V = np.linalg.svd(D, full_matrices=False)[2].T
    sgn = np.sign(np.sum(V * P, axis=0))
    assert np.abs(P - V * sgn).max() <= 64 * EPS
    M2, P2 = J.eposvd(D, nlv=2)
    assert P2.shape == (33, 2) and np.array_equal(P2, P[:, :2]) and np.linalg.norm(D @ M2, 2) <= np.linalg.svd(D, compute_uv=False)[2] * (1 + 1e-12)
    assert J.eposvd(D[:1], nlv=3)[1].shape == (33, 1)                                         # nlv = min(nlv, n, p)
    assert np.abs(np.abs(J.eposvd(D[:1], nlv=1)[1][:, 0]) - np.abs(D[0]) / np.linalg.norm(D[0])).max() <= 16 * EPS   # n = 1: the normed row (:93-94)
    with pytest.raises(NotImplementedError):
        J.eposvd(np.broadcast_to(np.zeros(1), (1 << 13, (1 << 11) + 1)), nlv=1)


def test_difmean():
    X, Xt = standards()
    D, m1, m2 = J.difmean(X, Xt[:17])
    assert D.shape == (1, 33) and np.array_equal(m1, X.mean(axis=0)) and np.array_equal(m2, Xt[:17].mean(axis=0)) and np.array_equal(D[0], m1 - m2)
    D, m1, m2 = J.difmean(X, Xt[:17], normx=True)
    a, b = X.mean(axis=0), Xt[:17].mean(axis=0)
    assert np.array_equal(m1, a / np.linalg.norm(a)) and np.array_equal(m2, b / np.linalg.norm(b)) and np.array_equal(D[0], m1 - m2)
    assert abs(np.linalg.norm(m1) - 1.0) <= 4 * EPS
    with pytest.raises(ValueError):
        J.difmean(X, Xt[:, :5])


# ---------------------------------------------------------------------------------- the kernel's per-element bound
@pytest.mark.parametrize("f", FIR_FS)
def test_fir_bound_holds_for_both_float64_evaluations(f):
    worst = 0.0
    for p in FIR_PS:
        for lo in fir_los(f):
            X, tab = fir_case(130, p, f, lo)
            X = X[[0, 64, 129]]                                              # three rows of the GPU file's data: the rationals are slow
            ref, bound = fir_ref(X, tab, lo)
            for fused in (False, True):
                got = fir_f64(X, tab, lo, fused)
                err = np.abs((got.astype(np.longdouble) - ref).astype(np.float64))
                ok = bound > 0
                assert np.all(err[~ok] == 0.0)
                worst = max(worst, float((err[ok] / bound[ok]).max()) if ok.any() else 0.0)
                assert np.all(err <= 0.5 * bound), (p, lo, fused)
    print(f"  f={f}: worst err / bound {worst:.3f} (limit 0.5)")


def test_fir_zero_tap_skip_is_part_of_the_definition():
    X, tab = fir_case(3, 9, 3, -1)
    tab[0, 4] = 0.0
    X[1, 3] = np.inf                                                        # under the zero tap of output 4
    ref, _ = fir_ref(X, tab, -1)
    got = fir_f64(X, tab, -1, False)
    assert np.isfinite(got[1, 4]) and np.isfinite(ref[1, 4])
