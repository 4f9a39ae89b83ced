"""The spatial median and spherical PCA without a GPU: literal numpy restatements of src/colmedspa.jl and src/pcasph.jl (float64 and np.longdouble),
the input generators and the cases of tests/test_gpu_medspa.py and tests/test_gpu_pcasph.py, the error bounds those tests hold the device to (derived
here, proved on the restatements alone), and the boundary (header, SYMBOLS, Makefile, exports, Julia signatures).

The step bound.  u = 2^-53.  One Weiszfeld step from a given centre c, any summation order:
  d_i   e_j = fl(x_ij - c_j) carries one rounding, e_j^2 two more (one with an fma), the sum of the p non-negative squares at most p - 1 more whatever
        its order: the sum of squares is within (p + 2) u of exact, its root within (p / 2 + 1) u plus the root's own rounding.
        |d_i - exact| <= (p / 2 + 3) u d_i   (one u of slack).
  w0    a median moves no further than the largest move of an element; Julia's middle(lo, hi) adds two roundings: (p / 2 + 5) u max d.
  mu_j  = sum_i u_i x_ij / sum_i u_i with u_i = 1 / d_i: u_i within (p / 2 + 4) u; a product u_i x_ij one more; the n-term sums at most n - 1 more each,
        relative to sum_i u_i |x_ij| <= max|X| sum_i u_i; the quotient one more (or, normalising first as the reference does, one per term, which the n
        of the sum already covers): |mu_j - exact| <= (p / 2 + 5 + n + p / 2 + 4 + n + 1) u max|X| = (p + 2 n + 10) u max|X| <= (p + 2 n + 16) u max|X|.
        This needs the same rows clamped in both computations: every case keeps every d_i a relative 1e-9 away from ep (and from the loop's guard).
  h     = |mu - c|: a norm moves no further than the norm of the move of its argument, sqrt(p) times the mu bound, plus its own (p / 2 + 3) u h.
The loop bound: max(10 g, the step bound) with g the gap between the float64 and the longdouble restatement at their common step count; the factor
10 covers the device's different summation order."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
HDR = os.path.join(ROOT, "include", "jchemo_hip.h")
JL = os.path.join(ROOT, "jchemo.jl_amd", "julia", "JchemoHIP.jl")
SRC = os.path.join(ROOT, "jchemo.jl_amd", "csrc", "medspa.hip")

U = 2.0 ** -53
MAD_CONSTANT = 1.4826022185056018   # StatsBase `mad`, normalize = true
LD = np.longdouble


# ---------------------------------------------------------------------------------- the kernel's constants
def kernel_constants():
    """rows per tile, waves per workgroup, columns per wave, tiles per workgroup: parsed out of medspa.hip."""
    src = open(SRC).read()
    get = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)\b", src).group(1))   # noqa: E731
    return dict(rows=get("MS_ROWS"), waves=get("MS_WAVES"), cpw=get("MS_CPW"), tiles=get("MS_TILES"))


# ---------------------------------------------------------------------------------- restatements
def julia_median(v):
    """Julia's `median`: NaN if any NaN; the middle element for odd n, middle(lo, hi) = lo / 2 + hi / 2 for even n."""
    v = np.asarray(v)
    if np.any(np.isnan(v)):
        return v.dtype.type(np.nan)
    s = np.sort(v)
    n = s.shape[0]
    return s[n // 2] if n % 2 else s[n // 2 - 1] / 2 + s[n // 2] / 2


def np_step(X, mu0, delta, dt=np.float64):
    """src/colmedspa.jl:15-30, one trip of the loop.  Returns mu, d (the distances before the clamp), w0, h and the mask of the clamped rows."""
    X = np.asarray(X).astype(dt)
    mu0 = np.asarray(mu0).astype(dt)
    delta = dt(delta)
    TT = mu0[None, :] * np.ones(X.shape, dtype=dt)          # :15
    Usq = (X - TT) ** 2                                      # :16
    w = np.sqrt(Usq.sum(axis=1))                             # :17
    d = w.copy()
    w0 = julia_median(w)                                     # :18
    ep = delta * w0                                          # :19
    with np.errstate(invalid="ignore", divide="ignore"):
        s = w <= ep                                          # :20
        clamped = s.copy()
        w[s] = ep                                            # :21
        s = w > ep                                           # :22  (taken after the first assignment: a clamped row keeps ep, not 1 / ep)
        w[s] = 1 / w[s]                                      # :23
        w = w / w.sum()                                      # :24  mweight!
        mu = (w[:, None] * X).sum(axis=0)                    # :25-28
    h = np.sqrt(((mu - mu0) ** 2).sum())                     # :29
    return mu, d, w0, h, clamped


def np_colmedspa(X, delta=1e-6, dt=np.float64, maxit=1000):
    """src/colmedspa.jl:4-33 (with the mirror's maxit).  Returns mu, the number of steps, and per step (mu0, w0, h, d)."""
    X = np.asarray(X).astype(dt)
    n, p = X.shape
    delta1 = dt(delta) * np.sqrt(dt(p))                      # :7
    mu0 = np.array([julia_median(X[:, j]) for j in range(p)], dtype=dt)   # :8
    trace = []
    h = delta1 + 1                                           # :13
    while h > delta1 and len(trace) < maxit:                 # :14
        mu, d, w0, h, _ = np_step(X, mu0, delta, dt)
        trace.append(dict(mu0=mu0, w0=w0, h=h, d=d))
        mu0 = mu.copy()                                      # :30
    return mu0, len(trace), trace


def colmad(A):
    med = np.array([julia_median(A[:, j]) for j in range(A.shape[1])])
    return MAD_CONSTANT * np.array([julia_median(np.abs(A[:, j] - med[j])) for j in range(A.shape[1])])


def np_pcasph(X, weights=None, *, nlv, typc="medspa", delta=1e-3, scal=False, dt=np.float64):
    """src/pcasph.jl:60-92."""
    X = np.asarray(X).astype(dt)
    n, p = X.shape                                           # :62
    nlv = min(nlv, n, p)                                     # :63
    w = np.ones(n, dtype=dt) if weights is None else np.asarray(weights).astype(dt)
    w = w / w.sum()                                          # :64
    wmean = w @ X
    xmeans = np_colmedspa(X, delta, dt)[0] if typc == "medspa" else wmean   # :65-69
    xscales = np.ones(p, dtype=dt)                           # :70
    if scal:
        xscales = np.sqrt(w @ (X - wmean) ** 2)              # :72  colstd(X, weights): about the weighted mean
    Xs = (X - xmeans) / xscales                              # :73 / :75
    sqrtw = np.sqrt(w)                                       # :77
    xnorms = np.sqrt((Xs ** 2).sum(axis=1))                  # :78-79
    zX = Xs / xnorms[:, None]                                # :80-81
    A = (sqrtw[:, None] * zX).astype(np.float64)
    _, s, Vt = np.linalg.svd(A, full_matrices=False)         # :82
    P = Vt.T[:, :nlv].astype(dt)                             # :83
    zT = zX @ P                                              # :84
    sv = colmad(zT)                                          # :85
    T = Xs @ P                                               # :86
    u = np.argsort(-sv, kind="stable")                       # :87
    eig_all = np.r_[s ** 2, np.zeros(max(0, p - s.shape[0]))]
    return dict(T=T[:, u], P=P[:, u], sv=sv[u], xmeans=xmeans, xscales=xscales, weights=w, eig=(s ** 2)[:nlv][u], eig_all=eig_all, order=u, r=xnorms,
                G=A.T @ A, Xs=Xs)


def np_pcasvd_axis(X):
    """First loading of the classical PCA (src/pcasvd.jl:79-97, unit weights)."""
    Xc = X - X.mean(axis=0)
    return np.linalg.svd(Xc, full_matrices=False)[2][0]


# ---------------------------------------------------------------------------------- inputs
def gen(kind, n, p, seed=0):
    """cloud: level 100, spread 1 with decaying column scales, 10 % of the rows shifted by 6 along a fixed direction; level: level 1e4, spread 1;
    rowmu0: rows +-v and one zero row (n odd), so that the column medians ARE a row; dup: 40 % of the rows identical (below half: the median
    distance stays positive); nan: the cloud with one NaN."""
    rng = np.random.default_rng(1000 * n + p + 7 * seed)
    scale = 1.0 / np.sqrt(1.0 + np.arange(p) / 4.0)
    if kind in ("cloud", "nan"):
        X = 100.0 + rng.standard_normal((n, p)) * scale
        k = max(1, n // 10) if n >= 10 else 0
        dirn = rng.standard_normal(p)
        X[:k] += 6.0 * dirn / np.linalg.norm(dirn)
        if kind == "nan":
            X[n // 2, p // 2] = np.nan
    elif kind == "level":
        X = 1e4 + rng.standard_normal((n, p))
    elif kind == "rowmu0":
        assert n % 2 == 1
        V = rng.standard_normal((n // 2, p)) * scale + 0.3
        X = np.vstack([V, -V, np.zeros((1, p))])
    elif kind == "dup":
        X = 100.0 + rng.standard_normal((n, p)) * scale
        k = (2 * n) // 5
        X[:k] = X[0]
    else:
        raise ValueError(kind)
    return np.asfortranarray(X)


def step_cases():
    """(kind, n, p, delta) of tests/test_gpu_medspa.py, named from the kernel's constants: n = 2, 3; one row below, at and above a tile; the same
    around one workgroup's share; p = 1; p below the number of waves; p one below, at and above the widest shape of the register path; a p on the
    second-sweep path (three chunks, the last ragged); several workgroups with a ragged last tile; then the other contents at three of the shapes."""
    k = kernel_constants()
    R, share, wide = k["rows"], k["rows"] * k["tiles"], k["waves"] * k["cpw"]
    shapes = [(2, 5), (3, 5), (R - 1, 7), (R, 7), (R + 1, 7), (share - 1, 6), (share, 6), (share + 1, 6), (R + 1, 1), (200, k["waves"] - 5),
              (70, wide - 1), (70, wide), (70, wide + 1), (130, 2 * wide + 76), (1000, 130)]
    cases = [("cloud", n, p, 1e-3 if i % 2 else 1e-6) for i, (n, p) in enumerate(shapes)]
    for kind in ("level", "rowmu0", "dup"):
        cases += [(kind, R + 1, 3, 1e-6), (kind, share + 1, 7, 1e-3), (kind, 2 * share + 3, k["waves"] * 16 + 2, 1e-6)]
    return cases


NAN_CASE = ("nan", 200, 7, 1e-6)


def step_bound(X, d=None):
    """(per element of mu, per element of d as a factor of d_i, of w0 as a factor of max d, of h as (factor of the mu bound, factor of h))."""
    n, p = X.shape
    amax = float(np.max(np.abs(X)))
    return dict(mu=(p + 2 * n + 16) * U * amax, d_rel=(p / 2 + 3) * U, w0_rel=(p / 2 + 5) * U, h_mu=np.sqrt(p), h_rel=(p / 2 + 3) * U)


def loop_guard(delta, w0_prev, h_prev):
    return delta * (w0_prev + h_prev) * (1.0 + 2.0 ** -40)


_REF = {}


def ref(case):
    """The restatements of a case in both precisions, computed once and shared (read only)."""
    if case not in _REF:
        kind, n, p, delta = case
        X = gen(kind, n, p)
        X.setflags(write=False)
        mu64, it64, tr64 = np_colmedspa(X, delta, np.float64)
        muld, itld, trld = np_colmedspa(X, delta, LD)
        _REF[case] = dict(X=X, mu64=mu64, it64=it64, tr64=tr64, muld=muld, itld=itld, trld=trld)
    return _REF[case]


def loop_bound(case):
    r = ref(case)
    g = float(np.max(np.abs(r["mu64"].astype(LD) - r["muld"])))
    return max(10 * g, step_bound(r["X"])["mu"])


# ---------------------------------------------------------------------------------- pcasph cases
def gen_pca(n, p, seed=0, contaminated=False):
    """A cloud with four separated principal scales over isotropic noise, level 50; `contaminated`: 10 % of the rows shifted by 60 along the THIRD
    axis of the clean cloud."""
    rng = np.random.default_rng(77 * n + p + seed)
    Q = np.linalg.qr(rng.standard_normal((p, p)))[0]
    s = np.full(p, 0.3)
    s[:min(p, 4)] = [9.0, 5.0, 2.5, 1.2][:min(p, 4)]
    X = 50.0 + (rng.standard_normal((n, p)) * s) @ Q.T
    if contaminated:
        X[:n // 10] += 60.0 * Q[:, 2]
    return np.asfortranarray(X), Q


PCA_SHAPES = [(200, 7, 3), (300, 40, 3), (60, 130, 3)]
PCA_CASES = [(n, p, nlv, scal, typc, wk) for (n, p, nlv) in PCA_SHAPES for scal in (False, True) for typc in ("medspa", "mean") for wk in ("ones", "rand")]
EIG_TOL = 1e-10
BEHAVIOUR = dict(n=400, p=12, angle_sph_deg=10.0, angle_svd_deg=60.0)


def pca_weights(kind, n):
    return None if kind == "ones" else 0.5 + np.random.default_rng(n + 3).random(n)


_PREF = {}


def pca_ref(case):
    if case not in _PREF:
        n, p, nlv, scal, typc, wk = case
        X = gen_pca(n, p)[0]
        X.setflags(write=False)
        w = pca_weights(wk, n)
        _PREF[case] = (X, w, np_pcasph(X, w, nlv=nlv, typc=typc, delta=1e-3, scal=scal))
    return _PREF[case]


def gaps(eig_all, idx):
    return np.array([np.min(np.abs(np.delete(eig_all, i) - eig_all[i])) for i in idx])


def pca_bounds(case):
    """Per returned column: cb = 10 eig_tol eig_1 / gap (a vector with residual eig_tol eig_1), and the sv bound from |MAD(a) - MAD(b)| <= 2 * 1.4826
    max|a - b|: a column of zT = zX P moves by no more than |dp_i| (the rows of zX are unit vectors) plus the move dz of a unit row under a centre
    moved by the loop bound (2 sqrt(p) lb / r_min, in scaled units) plus the rounding of the product and the division ((p + 8) u); p_i itself moves
    by cb_i plus 2 dz / gap_i, the perturbation of G (its weights sum to 1) over the gap."""
    n, p, nlv, scal, typc, wk = case
    X, w, rf = pca_ref(case)
    ea = rf["eig_all"]
    gp = gaps(ea, rf["order"])
    cb = 10 * EIG_TOL * ea[0] / gp
    if typc == "medspa":
        r = ref_for_matrix(X, 1e-3)
        lb = max(10 * r[0], step_bound(X)["mu"])
    else:
        lb = (n + 4) * U * float(np.max(np.abs(X)))
    dz = 2 * np.sqrt(p) * lb / float(np.min(rf["xscales"])) / float(np.min(rf["r"]))
    dp = cb + 2 * dz / gp
    svb = 2 * MAD_CONSTANT * (dp + dz + (p + 8) * U)
    return dict(cb=cb, sv=svb, lb=lb, gap=gp)


_GAP = {}


def ref_for_matrix(X, delta):
    key = (X.shape, float(X[0, 0]), delta)
    if key not in _GAP:
        m64, i64, t64 = np_colmedspa(X, delta, np.float64)
        mld, ild, tld = np_colmedspa(X, delta, LD)
        _GAP[key] = (float(np.max(np.abs(m64.astype(LD) - mld))), i64, ild, t64, tld)
    return _GAP[key]


def symmetric_design():
    """rows +-v (integers) and one zero row, with weights whose sum is a power of two: every product w_i x_ij and every partial sum is exact in any
    order, so the weighted mean is exactly 0 and the zero row lies AT the centre."""
    rng = np.random.default_rng(5)
    m, p = 32, 6
    V = rng.integers(-8, 9, (m, p)).astype(np.float64)
    V[V == 0] = 1.0
    X = np.asfortranarray(np.vstack([np.zeros((1, p)), V, -V]))
    w = np.ones(2 * m + 1)
    w[0] = 128 - 2 * m
    return X, w


def angle_deg(a, b):
    c = abs(float(a @ b)) / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.degrees(np.arccos(min(1.0, c))))


# ---------------------------------------------------------------------------------- tests: the loop and the step on the restatements
@pytest.mark.parametrize("case", step_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_both_precisions_take_the_same_steps_away_from_the_threshold(case):
    kind, n, p, delta = case
    r = ref(case)
    assert r["it64"] == r["itld"] and 1 <= r["it64"] < 1000, (r["it64"], r["itld"])
    thr = delta * np.sqrt(p)
    for tr in (r["tr64"], r["trld"]):
        for st in tr:
            assert np.isfinite(float(st["h"])) and np.isfinite(float(st["w0"]))
            assert abs(float(st["h"]) - thr) > 1e-3 * thr, (float(st["h"]), thr)
    # no distance within a relative 1e-9 of the clamp or of the loop's guard, in any step: the same rows are clamped / left out in every precision
    for k_, st in enumerate(r["trld"]):
        d, ep = st["d"].astype(np.float64), float(delta * st["w0"])
        edges = [ep]
        if k_ > 0:
            edges.append(loop_guard(delta, float(r["trld"][k_ - 1]["w0"]), float(r["trld"][k_ - 1]["h"])))
            assert edges[1] >= ep                                   # the triangle inequality's guard IS an upper bound
        for e in edges:
            near = np.abs(d - e) <= 1e-9 * e
            assert not np.any(near & (d != 0.0)), (k_, e)
    assert np.all(np.isfinite(r["mu64"]))


@pytest.mark.parametrize("case", step_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_float64_step_stays_within_the_step_bound_of_the_longdouble_step(case):
    kind, n, p, delta = case
    r = ref(case)
    X = r["X"]
    b = step_bound(X)
    for mu0 in (r["tr64"][0]["mu0"], r["tr64"][-1]["mu0"]):
        m64, d64, w64, h64, c64 = np_step(X, mu0, delta, np.float64)
        mld, dld, wld, hld, cld = np_step(X, mu0, delta, LD)
        assert np.array_equal(c64, cld)
        assert np.all(np.abs(m64.astype(LD) - mld) <= b["mu"])
        assert np.all(np.abs(d64.astype(LD) - dld) <= b["d_rel"] * dld)
        assert abs(LD(w64) - wld) <= b["w0_rel"] * np.max(dld)
        assert abs(LD(h64) - hld) <= b["h_mu"] * b["mu"] + b["h_rel"] * hld
    assert loop_bound(case) >= b["mu"]


def test_constructed_cases_do_clamp_rows_and_stay_finite():
    k = kernel_constants()
    for kind, want in (("rowmu0", 1), ("dup", None)):
        case = (kind, k["rows"] + 1, 3, 1e-6)
        r = ref(case)
        n = case[1]
        clamped = [int(np_step(r["X"], st["mu0"], case[3])[4].sum()) for st in r["tr64"]]
        if kind == "rowmu0":
            assert clamped[0] == 1                                     # the median start IS the zero row
        else:
            assert (2 * n) // 5 < n / 2                                # the coincident rows stay below half: w0 > 0
            assert all(float(st["w0"]) > 0 for st in r["tr64"])
        assert np.all(np.isfinite(r["mu64"]))
    # the shifted cloud never clamps: such rows have to be constructed
    case = next(c for c in step_cases() if c[:3] == ("cloud", 1000, 130))
    r = ref(case)
    assert all(int(np_step(r["X"], st["mu0"], case[3])[4].sum()) == 0 for st in r["tr64"])


def test_a_nan_ends_the_loop_after_one_step_with_nan():
    kind, n, p, delta = NAN_CASE
    mu, it, tr = np_colmedspa(gen(kind, n, p), delta)
    assert it == 1 and np.all(np.isnan(mu)) and np.isnan(tr[0]["h"]) and np.isnan(tr[0]["w0"])
    mu1, it1, _ = np_colmedspa(np.array([[1.0, 2.0]]), 1e-6)
    assert it1 == 1 and np.all(np.isnan(mu1))                        # n = 1: 0 / 0


# ---------------------------------------------------------------------------------- tests: pcasph on the restatements
@pytest.mark.parametrize("case", PCA_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_pcasph_cases_have_separated_spectra_and_a_stable_order(case):
    n, p, nlv, scal, typc, wk = case
    X, w, rf = pca_ref(case)
    b = pca_bounds(case)
    assert np.all(b["gap"] >= 0.05 * rf["eig_all"][0]), b["gap"] / rf["eig_all"][0]
    assert np.all(np.abs(np.diff(rf["sv"])) >= 100 * np.max(b["sv"])), (np.diff(rf["sv"]), b["sv"])
    assert np.all(b["cb"] < 1e-3)
    if typc == "medspa":
        g, i64, ild, t64, tld = ref_for_matrix(X, 1e-3)
        assert i64 == ild
        thr = 1e-3 * np.sqrt(p)
        assert all(abs(float(st["h"]) - thr) > 1e-3 * thr for st in list(t64) + list(tld))
    # the restatement agrees with itself: G P = P diag(eig), unit rows
    assert np.allclose(rf["G"] @ rf["P"], rf["P"] * rf["eig"], atol=1e-12)
    assert np.isclose(np.trace(rf["G"]), 1.0, rtol=1e-12)


def test_symmetric_design_puts_a_row_exactly_at_the_mean():
    X, w = symmetric_design()
    wn = w / w.sum()
    assert np.log2(w.sum()) == int(np.log2(w.sum()))
    for perm in (np.arange(X.shape[0]), np.random.default_rng(1).permutation(X.shape[0])):
        acc = np.zeros(X.shape[1])
        for i in perm:
            acc = acc + wn[i] * X[i]
            assert np.all(acc * w.sum() == np.round(acc * w.sum()))   # every partial sum is exact
        assert np.all(acc == 0.0)
    assert np.all(X[0] == 0.0)


def test_spherical_axis_resists_the_contamination_that_bends_the_classical_one():
    B = BEHAVIOUR
    Xc, Q = gen_pca(B["n"], B["p"], contaminated=True)
    clean = Q[:, 0]
    a_sph = angle_deg(np_pcasph(Xc, nlv=1)["P"][:, 0], clean)
    a_svd = angle_deg(np_pcasvd_axis(Xc), clean)
    assert a_sph <= B["angle_sph_deg"], a_sph
    assert a_svd >= B["angle_svd_deg"], a_svd
    assert angle_deg(np_pcasvd_axis(gen_pca(B["n"], B["p"])[0]), clean) <= B["angle_sph_deg"]   # without the shifted rows both find it


# ---------------------------------------------------------------------------------- tests: the boundary
def header_protos():
    h = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"JCH_API\s+([\w\s\*]+?)\b(jch_\w+)\s*\(([^;]*?)\)\s*;", h, flags=re.S):
        protos[m.group(2)] = (m.group(1).strip(), [re.sub(r"\s+", " ", q.strip()) for q in m.group(3).split(",")])
    return protos


ENTRIES = dict(jch_weiszfeld_step=14, jch_spatial_median=13, jch_pcasph_fit=30)


def test_header_declares_the_entries_with_their_comments():
    protos = header_protos()
    h = open(HDR).read()
    for name, nargs in ENTRIES.items():
        assert protos[name][0] == "int32_t" and len(protos[name][1]) == nargs, name
        assert re.search(r"\* " + name + r" -- ", h), f"{name} has no header comment"
    assert re.search(r"#define\s+JCH_CENT_MEDSPA\s+0\b", h) and re.search(r"#define\s+JCH_CENT_MEAN\s+1\b", h)
    assert [q.split()[-1].lstrip("*") for q in protos["jch_weiszfeld_step"][1]] == ["ctx", "loc", "X", "n", "p", "ldx", "mu0", "delta", "guard", "mu", "d", "w0",
                                                                                    "h", "nleft"]
    assert [q.split()[-1].lstrip("*") for q in protos["jch_spatial_median"][1]] == ["ctx", "loc", "X", "n", "p", "ldx", "delta", "maxit", "mu", "d", "niter",
                                                                                    "h_last", "converged"]
    mk = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "Makefile")).read()
    assert "medspa.hip" in re.search(r"SRCS := (.*)", mk).group(1).split()
    src = open(SRC).read()
    for name in ("jch_weiszfeld_step", "jch_spatial_median"):
        assert f'extern "C" int32_t {name}(' in src
    assert 'extern "C" int32_t jch_pcasph_fit(' in open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "xtdx.hip")).read()
    assert "jch_launch_weiszfeld_dist" in open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "jch_internal.h")).read()
    k = kernel_constants()
    assert k["rows"] == 64 and k["waves"] * k["cpw"] >= 500             # the flagship width stays on the register path
    assert "atomic" not in re.sub(r"//.*", "", src)                     # no atomics in the step


def test_python_package_exports_and_defaults():
    import inspect

    import jchemo_hip as J
    for name in ENTRIES:
        assert name in J.SYMBOLS
    assert len(J.SYMBOLS) == len(set(J.SYMBOLS))
    for name in ("colmedspa", "pcasph", "pcasph_", "weiszfeld_step"):
        assert hasattr(J, name), name
    sig = inspect.signature(J.colmedspa)
    assert list(sig.parameters) == ["X", "delta", "maxit", "ctx"] and sig.parameters["delta"].default == 1e-6 and sig.parameters["maxit"].default == 1000
    sig = inspect.signature(J.pcasph)
    assert list(sig.parameters) == ["X", "weights", "nlv", "typc", "delta", "scal", "eig_tol", "eig_maxit", "ctx"]
    assert sig.parameters["typc"].default == "medspa" and sig.parameters["delta"].default == 1e-3 and sig.parameters["scal"].default is False
    assert sig.parameters["eig_tol"].default == 1e-10 and sig.parameters["eig_maxit"].default == 300
    assert [f.name for f in dataclasses.fields(J.Pca)][:8] == ["T", "P", "sv", "xmeans", "xscales", "weights", "niter", "conv"]


def test_python_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    X = np.zeros((4, 2), order="F")
    for bad in (dict(nlv=0), dict(nlv=1, typc="median"), dict(nlv=1, delta=0.0), dict(nlv=1, eig_tol=0.0), dict(nlv=1, eig_maxit=0)):
        with pytest.raises(ValueError):
            J.pcasph(X, **bad)
    for bad in (dict(delta=0.0), dict(delta=-1.0), dict(maxit=0)):
        with pytest.raises(ValueError):
            J.colmedspa(X, **bad)
    with pytest.raises(ValueError):
        J.weiszfeld_step(X, np.zeros(3))


def test_without_a_gpu_the_mirror_raises_enodev():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import jchemo_hip as J
    from jchemo_hip._lib import JCH_ENODEV, JchError
    for call in (lambda: J.colmedspa(gen("cloud", 10, 3)), lambda: J.pcasph(gen("cloud", 10, 3), nlv=2)):
        with pytest.raises(JchError) as e:
            call()
        assert e.value.code == JCH_ENODEV


def test_julia_module_exports_and_literal_signatures():
    from test_julia_wrapper import _split_top, julia_ccalls
    src = open(JL).read()
    names = {s.strip() for s in re.search(r"\nexport (.*?)\n\n", src, flags=re.S).group(1).replace("\n", " ").split(",")}
    for name in ("colmedspa", "pcasph", "pcasph!"):
        assert name in names, name
    protos = header_protos()
    seen = {}
    for args in julia_ccalls():
        m = re.match(r"\(:(\w+),\s*LIB\)", args[0])
        if m and m.group(1) in ENTRIES:
            seen[m.group(1)] = _split_top(args[2][1:-1])
    for name, nargs in ENTRIES.items():
        if name == "jch_weiszfeld_step":
            continue                                                   # the step is a test entry: the Julia module calls the loop and the fit
        assert name in seen, f"the Julia wrapper never calls {name}"
        assert len(seen[name]) == nargs == len(protos[name][1])
    assert re.search(r"function colmedspa\(X; delta = 1e-6", src) and re.search(r"function pcasph!\(X", src)
