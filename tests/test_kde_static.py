"""CPU-side checks of the kernel density family: literal numpy restatements of the reference's src/dmkern.jl, src/kdeda.jl and src/plskdeda.jl with
their predicts (in float64 and in np.longdouble; shared with tests/test_gpu_kde.py), the error bound of jch_kde_dens as a function, the input
generators of both files, and the boundary (header, SYMBOLS, Makefile, exports, dataclasses, defaults, Julia mirror, ValueErrors).

The error bound (per output element, evaluated in longdouble; eps = 2^-52).  A pair's exponent s = v2 * sum_j ((x_j - z_j) u_j)^2 is a sum of dims_a
non-negative squares of rounded differences: relative error <= (dims_a + 6) eps.  The term exp(-s / 2) then carries (0.5 (dims_a + 6) s + C_EXP) eps,
C_EXP the ulp error of the device `exp` (no ulp table of the device library is installed with the toolchain: 2 is taken, as the issue allows).
The fixed-order sum of the n_c positive terms and the product with coef add n_c eps; terms in the denormal range are covered by the absolute floor
n_c coef 2^-1074.  At the model level a relative error delta_h <= (n_c + 4) eps of a device-computed colstd moves s by 2 delta_h s, the term by
delta_h s.  So
    bound[i, c, a] = coef sum_r exp(-s_r / 2) ((0.5 (dims_a + 6) s_r + C_EXP + n_c [+ (n_c + 4) s_r]) eps) + n_c coef 2^-1074 + 2^-1075.
The last term is not in the issue's list and is the format's own: the product coef * sum is itself rounded to a multiple of 2^-1074 when it lands
in the denormal range, by up to 2^-1075, which n_c coef 2^-1074 does not cover when coef < 1 / (2 n_c).  No float64 result can do without it: the
reference's own arithmetic in float64 (np_dmkern_predict) misses the bound without it by a factor of up to 2.0 on the plskdeda shapes below
(densities of 1e-319 and 5e-323 of the two-row class), which is how it was found; everywhere else the bound is the issue's."""
import dataclasses
import inspect
import os
import re
import sys
from functools import lru_cache

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))

from oracle import plsr_oracle as O  # noqa: E402

EPS = 2.0 ** -52
C_EXP = 2
LD = np.longdouble
# the constants of jchemo.jl_amd/csrc/kde.hip the shapes below straddle
KDE_QT, KDE_DREG, KDE_DLDS, KDE_MG, KDE_CH, KDE_ZL0, KDE_LDS, KDE_SPLIT_ROWS = 64, 32, 80, 8, 256, 5120, 7168, 64
KDE_DR = (4, 8, 16, 32)


def test_longdouble_is_extended_precision():
    assert np.finfo(LD).eps < 1e-18


# ---------------------------------------------------------------------------------- numpy restatements of the reference
def np_colstd(X):
    """`colstd(X)` with uniform weights — src/utility.jl:262,312: sqrt of the uncorrected variance."""
    n = X.shape[0]
    w = np.full(n, 1, dtype=X.dtype) / n
    mu = w @ X
    return np.sqrt(w @ (X - mu) ** 2)


def np_dmkern(X, h=None, a=1, ft=np.float64):
    """src/dmkern.jl:124-143, line by line.  Returns dict(X, H, Hinv, detH)."""
    X = O.ensure_mat(np.asarray(X, dtype=ft))
    n, p = X.shape
    if h is None:
        hv = ft(a) * ft(n) ** (-ft(1) / (p + 4)) * np_colstd(X)       # :134
    else:
        hv = np.full(p, ft(h)) if np.ndim(h) == 0 else np.asarray(h, dtype=ft)   # :137
    H = np.diag(hv)
    if np.any(hv == 0):
        raise np.linalg.LinAlgError("SingularException")            # :139 inv(H)
    Hinv = np.diag(1 / hv)
    detH = np.prod(hv)                                              # :140
    if detH == 0:
        detH = ft(1e-20)                                            # :141
    return dict(X=X, H=H, Hinv=Hinv, detH=detH)


def np_dmkern_predict(fm, X):
    """src/dmkern.jl:151-163: the loop over the m query rows.  (`M * Hinv` with a diagonal Hinv: every entry is one product plus zeros.)"""
    Xt = fm["X"]
    ft = Xt.dtype.type
    X = O.ensure_mat(np.asarray(X, dtype=ft))
    n, p = Xt.shape
    hinv = np.diag(fm["Hinv"])
    pred = np.empty((X.shape[0], 1), dtype=ft)
    for i in range(X.shape[0]):
        M = (X[i:i + 1] - Xt) * hinv                                # :158
        sum2 = np.sum(M ** 2, axis=1)                               # :159
        pred[i, 0] = 1 / ft(n) * (2 * ft(np.pi)) ** (-ft(p) / 2) * (1 / fm["detH"]) * np.sum(np.exp(-ft(.5) * sum2))   # :160
    return pred


def np_kdeda(X, y, prior="unif", h=None, a=1, ft=np.float64):
    """src/kdeda.jl:62-79."""
    X = O.ensure_mat(np.asarray(X, dtype=ft))
    y = np.asarray(y).reshape(-1)
    lev, ni = np.unique(y, return_counts=True)
    nlev = len(lev)
    wprior = np.ones(nlev, dtype=ft) / nlev if prior == "unif" else ni.astype(ft) / ni.sum()
    fm = [np_dmkern(X[y == lev[i]], h=h, a=a, ft=ft) for i in range(nlev)]
    return dict(fm=fm, wprior=wprior, lev=lev, ni=ni)


def np_kdeda_predict(obj, X):
    """src/kdeda.jl:81-97: (pred, dens, posterior)."""
    dens = np.concatenate([np_dmkern_predict(f, X) for f in obj["fm"]], axis=1)
    A = obj["wprior"][None, :] * dens
    with np.errstate(invalid="ignore", divide="ignore"):
        posterior = A / A.sum(axis=1, keepdims=True)
    z = np.argmax(posterior, axis=1)                                # (the first level on ties and on a NaN row, as Julia's)
    return obj["lev"][z].reshape(-1, 1), dens, posterior


def np_plskdeda(T, y, nlv, prior="unif", h=None, a=1, ft=np.float64):
    """src/plskdeda.jl:58-61 on the scores T of the plskern fit of `dummy(y)`: kdeda(T[:, 1:i], y) for i = 1..nlv."""
    return [np_kdeda(np.asarray(T)[:, :i], y, prior=prior, h=h, a=a, ft=ft) for i in range(1, nlv + 1)]


def np_plskdeda_predict(fm_da, Tq, rng):
    """src/plslda.jl:107-130 behind the transform: model fm_da[nlv] on the leading nlv columns of the query scores."""
    return [np_kdeda_predict(fm_da[k - 1], np.asarray(Tq)[:, :k]) for k in rng]


# ---------------------------------------------------------------------------------- the primitive in longdouble, with its bound
def ld_kde_dens(Z, Xq, cs, u, v2, coef, dims, model_level=False):
    """(dens, bound), both (m, ncls, nmod) longdouble: jch_kde_dens' formula and the module docstring's bound."""
    Z, Xq, u, v2, coef = (np.asarray(a, dtype=LD) for a in (Z, Xq, u, v2, coef))
    m, ncls, nmod = Xq.shape[0], len(cs) - 1, len(dims)
    dens, bound = np.zeros((m, ncls, nmod), dtype=LD), np.zeros((m, ncls, nmod), dtype=LD)
    for c in range(ncls):
        Zc = Z[cs[c]:cs[c + 1]]
        nc = Zc.shape[0]
        q = np.zeros((m, nc), dtype=LD)
        j = 0
        for a in range(nmod):
            while j < dims[a]:
                q += ((Xq[:, j][:, None] - Zc[:, j][None, :]) * u[j, c]) ** 2
                j += 1
            s = v2[a, c] * q
            e = np.exp(-s / 2)
            per = 0.5 * (dims[a] + 6) * s + C_EXP + nc + ((nc + 4) * s if model_level else 0)
            dens[:, c, a] = coef[a, c] * e.sum(axis=1)
            bound[:, c, a] = coef[a, c] * (e * per).sum(axis=1) * LD(EPS) + nc * coef[a, c] * LD(2.0) ** -1074 + LD(2.0) ** -1075
    return dens, bound


def posterior_with_bound(wprior, dens, bound):
    """Posterior of (m, nlev) longdouble densities and its bound: post_c = w_c d_c / S, S = sum_k w_k d_k; with |delta d_k| <= B_k, to first
    order |delta post_c| <= w_c B_c / S + post_c sum_k w_k B_k / S; (4 + nlev) eps post_c for the two products with w, the division and the
    nlev roundings of the row sum, and 1e-6 of the whole for the second order (the callers assert that the bound stays below 1e-9).  A density
    or a product w_c d_c in the denormal range is rounded to a multiple of 2^-1074 (2^-1075 each, together at most 2^-1074 in w_c d_c, which
    the division by S magnifies), and so is a denormal quotient: the absolute floor 2^-1074 (1 / S + 1)."""
    w = np.asarray(wprior, dtype=LD)[None, :]
    S = (w * dens).sum(axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        post = w * dens / S
        pb = ((w * bound / S + post * (w * bound).sum(axis=1, keepdims=True) / S) * LD(1 + 1e-6) + (4 + dens.shape[1]) * LD(EPS) * post
              + LD(2.0) ** -1074 * (1 / S + 1))
    return post, pb


def ratio(got, ref, bound):
    """Largest measured / allowed over an array (0 where both the error and the bound are 0)."""
    err = np.abs(np.asarray(got, dtype=LD) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(err == 0, 0, err / bound)
    return float(np.max(r))


# ---------------------------------------------------------------------------------- inputs
def prim_inputs(seed, m, sizes, d, dims):
    """Inputs of one jch_kde_dens call: standard normal rows and queries, u in [0.5, 1.5] / sqrt(d) (so that s stays of order 1 .. 10 in every
    model), v2 in [0.5, 1.5], coef in [0.5, 1.5]."""
    rng = np.random.default_rng(seed)
    n, ncls, nmod = int(sum(sizes)), len(sizes), len(dims)
    cs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    Z = np.asfortranarray(rng.normal(size=(n, d)))
    Xq = np.asfortranarray(rng.normal(size=(m, d)))
    u = np.asfortranarray(rng.uniform(0.5, 1.5, size=(d, ncls)) / np.sqrt(d))
    v2 = np.asfortranarray(rng.uniform(0.5, 1.5, size=(nmod, ncls)))
    coef = np.asfortranarray(rng.uniform(0.5, 1.5, size=(nmod, ncls)))
    return dict(Z=Z, Xq=Xq, cs=cs, u=u, v2=v2, coef=coef, dims=np.asarray(dims, dtype=np.int32))


def _nested(d):
    return tuple(range(1, d + 1))


# (m, class sizes, d, dims): the issue's shapes, then the values that straddle the kernel's own constants
PRIM_CASES = {
    "m1_n1_d1": (1, (1,), 1, (1,)),
    "m63_mixed_d2_nested": (63, (2, 63, 1025), 2, _nested(2)),
    "m64_n64_d7": (64, (64,), 7, (7,)),
    "m65_mixed_d7_nested": (65, (65, 1, 2), 7, _nested(7)),
    "m257_mixed_d25_nested": (257, (1025, 64, 63), 25, _nested(25)),          # 4 model groups of KDE_MG, 17 chunks, 16 slices
    "m65_n65_d33": (65, (65,), 33, (33,)),                                    # the LDS query tile
    "m63_mixed_d33_nested": (63, (2, 63, 65), 33, _nested(33)),               # ... whose first groups walk <= KDE_DREG columns
    "m64_n1025_d130": (64, (1025,), 130, (130,)),                             # beyond KDE_DLDS: global memory
    "m65_mixed_d130_nested": (65, (63, 64, 65), 130, _nested(130)),
    "m65_dims_2_2_5": (65, (65, 2, 1), 7, (2, 2, 5)),                         # not contiguous, two models on the same columns
    "m257_dims_3_3_20_33": (257, (64, 65), 40, (3, 3, 20, 33)),
    **{f"walk_{d}": (65, (3,), d, (d,)) for d in (4, 5, 8, 9, 16, 17, KDE_DREG, KDE_DLDS, KDE_DLDS + 1)},   # the DR ladder and the three modes
    "nmod_8": (65, (5,), 9, _nested(8)), "nmod_9": (65, (5,), 9, _nested(9)),                               # KDE_MG
    "chunk_d32": (3, (KDE_ZL0 // 32, KDE_ZL0 // 32 + 1), 32, (32,)),                                        # rows of a MODE 0 chunk at DR = 32
    "chunk_d3": (3, (KDE_CH, KDE_CH + 1), 3, (3,)),                                                         # KDE_CH
    "chunk_d80": (3, (24, 25, 49), KDE_DLDS, (KDE_DLDS,)),                                                  # rows of a MODE 1 chunk at 80 columns
    "split": (3, (2 * KDE_SPLIT_ROWS - 1, 2 * KDE_SPLIT_ROWS, 2 * KDE_SPLIT_ROWS + 1), 2, (2,)),            # one slice / two slices
}


@lru_cache(maxsize=None)
def prim_case(name):
    """(inputs, longdouble dens, bound) of a case of PRIM_CASES; computed once, shared, not to be written to."""
    m, sizes, d, dims = PRIM_CASES[name]
    inp = prim_inputs(sum(map(ord, name)), m, sizes, d, dims)
    ref, bound = ld_kde_dens(inp["Z"], inp["Xq"], inp["cs"], inp["u"], inp["v2"], inp["coef"], inp["dims"])
    for a in (*inp.values(), ref, bound):
        a.setflags(write=False)
    return inp, ref, bound


def f64_kde_dens(inp):
    """The formula of jch_kde_dens in float64 numpy (column by column, a plain sum)."""
    m, ncls, nmod = inp["Xq"].shape[0], len(inp["cs"]) - 1, len(inp["dims"])
    out = np.zeros((m, ncls, nmod))
    for c in range(ncls):
        Zc = inp["Z"][inp["cs"][c]:inp["cs"][c + 1]]
        q, j = np.zeros((m, Zc.shape[0])), 0
        for a in range(nmod):
            while j < inp["dims"][a]:
                q += ((inp["Xq"][:, j][:, None] - Zc[:, j][None, :]) * inp["u"][j, c]) ** 2
                j += 1
            out[:, c, a] = inp["coef"][a, c] * np.exp(-0.5 * (inp["v2"][a, c] * q)).sum(axis=1)
    return out


SIZES = (2, 65, 130)
NLAT, PX, NLV = 5, 40, 5
SEED = 20250607
FAR = 1e3


@lru_cache(maxsize=None)
def clusters():
    """Three Gaussian clusters (unit covariance, centres 2.5 apart per coordinate on average) in a 5-dimensional latent space, class sizes
    (2, 65, 130), rows shuffled; 40 queries from the same clusters and, last, one query 1e3 standard deviations away.  X = the latent rows through
    a fixed 5 x 40 map plus 2 % noise (197 x 40), Xq likewise."""
    rng = np.random.default_rng(SEED)
    centres = rng.normal(size=(3, NLAT)) * 2.5
    y = np.repeat(np.array(["a", "b", "c"]), SIZES)
    L = centres[np.repeat(np.arange(3), SIZES)] + rng.normal(size=(sum(SIZES), NLAT))
    perm = rng.permutation(sum(SIZES))
    L, y = L[perm], y[perm]
    cq = np.r_[np.repeat(np.arange(3), 13), 0]
    Lq = centres[cq] + rng.normal(size=(40, NLAT))
    Lq = np.vstack([Lq, centres.mean(axis=0) + FAR])
    A = rng.normal(size=(NLAT, PX))
    X = np.asfortranarray(L @ A + 0.02 * rng.normal(size=(L.shape[0], PX)))
    Xq = np.asfortranarray(Lq @ A + 0.02 * rng.normal(size=(Lq.shape[0], PX)))
    w = rng.uniform(0.5, 1.5, size=L.shape[0])
    for a in (L, Lq, X, Xq, w):
        a.setflags(write=False)
    return dict(L=np.asfortranarray(L), Lq=np.asfortranarray(Lq), y=y, X=X, Xq=Xq, w=w)


def model_inputs(fm_list_ld, Z, y):
    """The arguments of ld_kde_dens for a list of restated kdeda models (nested, on the leading columns of Z): grouped rows, offsets, u, v2 = 1,
    coef, dims — all from the longdouble restatement's own H and detH."""
    lev = fm_list_ld[0]["lev"]
    order = np.argsort(np.searchsorted(lev, y), kind="stable")
    ni = fm_list_ld[0]["ni"]
    cs = np.concatenate([[0], np.cumsum(ni)]).astype(np.int64)
    return np.asarray(Z, dtype=LD)[order], cs, lev, ni


def ld_models(fm_list_ld, Z, Xq, y):
    """(dens, bound) (m, nlev, nmod) of restated kdeda models, model k on the first dims_k columns, with the model-level bound.  Every model has
    its own bandwidths (they do not separate exactly in longdouble either), so the primitive's formula runs once per model."""
    Zg, cs, lev, ni = model_inputs(fm_list_ld, Z, y)
    m, nlev, nmod = np.asarray(Xq).shape[0], len(lev), len(fm_list_ld)
    dens, bound = np.zeros((m, nlev, nmod), dtype=LD), np.zeros((m, nlev, nmod), dtype=LD)
    for k, obj in enumerate(fm_list_ld):
        p = obj["fm"][0]["X"].shape[1]
        u = np.stack([np.diag(f["Hinv"]) for f in obj["fm"]], axis=1)
        coef = np.array([[1 / LD(ni[c]) * (2 * LD(np.pi)) ** (-LD(p) / 2) * (1 / obj["fm"][c]["detH"]) for c in range(nlev)]], dtype=LD)
        d1, b1 = ld_kde_dens(Zg[:, :p], np.asarray(Xq)[:, :p], cs, u, np.ones((1, nlev)), coef, [p], model_level=True)
        dens[:, :, k], bound[:, :, k] = d1[:, :, 0], b1[:, :, 0]
    return dens, bound


def top_two_gap(post):
    s = np.sort(np.asarray(post, dtype=np.float64), axis=1)
    return s[:, -1] - s[:, -2]


# ---------------------------------------------------------------------------------- the restatements against each other and the bound
@pytest.mark.parametrize("name", list(PRIM_CASES))
def test_float64_formula_stays_inside_the_bound(name):
    inp, ref, bound = prim_case(name)
    r = ratio(f64_kde_dens(inp), ref, bound)
    print(f"{name}: float64 numpy against longdouble, largest measured / allowed = {r:.3f}")
    assert r <= 1.0


def test_far_query_underflows_to_exactly_zero_in_float64():
    inp = dict(prim_inputs(5, 3, (4, 5), 3, (1, 3)))
    Xq = np.array(inp["Xq"]); Xq[1] += FAR / inp["u"].min()
    inp["Xq"] = Xq
    out = f64_kde_dens(inp)
    assert np.all(out[1] == 0.0) and np.all(out[0] > 0) and np.all(out[2] > 0)


def test_dmkern_density_integrates_to_one():
    """On a 1-D grid the restated density integrates to 1 within the trapezoid rule's error (h^2 / 12 * (b - a) * max |f''|, and the tails)."""
    x = np.random.default_rng(3).normal(size=40)
    fm = np_dmkern(x)
    g = np.linspace(x.min() - 12 * fm["H"][0, 0], x.max() + 12 * fm["H"][0, 0], 4001)
    f = np_dmkern_predict(fm, g)[:, 0]
    step = g[1] - g[0]
    integral = step * (f.sum() - 0.5 * (f[0] + f[-1]))
    fpp_max = 1 / (np.sqrt(2 * np.pi) * fm["H"][0, 0] ** 3)      # |f''| <= max |phi''| / h^3 = phi(0) / h^3
    assert abs(integral - 1) <= step ** 2 / 12 * (g[-1] - g[0]) * fpp_max + 1e-12


@pytest.mark.parametrize("h,a", [(None, 1), (None, 0.5), (0.3, 1), ("vec", 1)])
@pytest.mark.parametrize("p", [1, 4])
def test_dmkern_restatement_float64_against_longdouble(p, h, a):
    cl = clusters()
    hv = np.linspace(0.2, 0.5, p) if h == "vec" else h
    Z, Xq = cl["L"][:, :p], cl["Lq"][:, :p]
    f64 = np_dmkern_predict(np_dmkern(Z, h=hv, a=a), Xq)
    fl = np_dmkern(Z, h=hv, a=a, ft=LD)
    n = Z.shape[0]
    coef = np.array([[1 / LD(n) * (2 * LD(np.pi)) ** (-LD(p) / 2) * (1 / fl["detH"])]], dtype=LD)
    ref, bound = ld_kde_dens(Z, Xq, [0, n], np.diag(fl["Hinv"]).reshape(p, 1), [[1]], coef, [p], model_level=True)
    assert np.max(np.abs(np_dmkern_predict(fl, Xq)[:, 0] - ref[:, 0, 0]) / (bound[:, 0, 0])) < 1e-2   # (the loop and the vectorised form agree)
    r = ratio(f64[:, 0], ref[:, 0, 0], bound[:, 0, 0])
    print(f"dmkern p={p} h={h} a={a}: largest measured / allowed = {r:.3f}")
    assert r <= 1.0 and f64[-1, 0] == 0.0


def kdeda_reference(Z, Xq, y, prior, h, a):
    """Longdouble kdeda on Z: (restated model, dens (m, nlev), its bound, posterior, its bound, pred)."""
    obj = np_kdeda(Z, y, prior=prior, h=h, a=a, ft=LD)
    dens, bound = ld_models([obj], Z, Xq, y)
    post, pb = posterior_with_bound(obj["wprior"], dens[:, :, 0], bound[:, :, 0])
    return obj, dens[:, :, 0], bound[:, :, 0], post, pb, obj["lev"][np.argmax(post, axis=1)].reshape(-1, 1)


@lru_cache(maxsize=None)
def oracle_scores(weighted, scal):
    """float64 scores of the oracle's plskern fit of `dummy(y)` (the static stand-in for the device fit) and of the queries."""
    cl = clusters()
    Yd = (cl["y"][:, None] == np.unique(cl["y"])[None, :]).astype(np.float64)
    fm = O.plskern(np.array(cl["X"]), Yd, np.array(cl["w"]) if weighted else None, nlv=NLV, scal=scal)
    return fm.T, O.transform(fm, np.array(cl["Xq"]))


def plskdeda_reference(T, Tq, y, prior, h, a, rng):
    """Longdouble plskdeda on given scores: per nlv of rng (dens, bound, posterior, its bound, pred)."""
    fm_da = np_plskdeda(T, y, max(rng), prior=prior, h=h, a=a, ft=LD)
    dens, bound = ld_models([fm_da[k - 1] for k in rng], T, Tq, y)
    out = []
    for i, k in enumerate(rng):
        post, pb = posterior_with_bound(fm_da[k - 1]["wprior"], dens[:, :, i], bound[:, :, i])
        out.append((dens[:, :, i], bound[:, :, i], post, pb, fm_da[k - 1]["lev"][np.argmax(post, axis=1)].reshape(-1, 1)))
    return out


def assert_gap(post, pb, what):
    """The top-two gap of the longdouble posterior exceeds twice the posterior bound at every query but the far one (whose row is NaN)."""
    gap = top_two_gap(post[:-1])
    need = 2 * np.max(np.asarray(pb[:-1], dtype=np.float64), axis=1)
    print(f"{what}: smallest top-two gap {gap.min():.3e}, largest 2 x bound {need.max():.3e}")
    assert np.all(gap > need), what
    assert np.max(np.asarray(pb[:-1], dtype=np.float64)) < 1e-9   # (the first-order bound of posterior_with_bound is in its range)


@pytest.mark.parametrize("prior", ["unif", "prop"])
def test_kdeda_restatement_and_the_gap_of_the_seed(prior):
    cl = clusters()
    _, dens, bound, post, pb, pred = kdeda_reference(cl["L"], cl["Lq"], cl["y"], prior, None, 1)
    p64, d64, po64 = np_kdeda_predict(np_kdeda(cl["L"], cl["y"], prior=prior), cl["Lq"])
    r, rp = ratio(d64, dens, bound), ratio(po64[:-1], post[:-1], pb[:-1])
    print(f"kdeda {prior}: dens {r:.3f}, posterior {rp:.3f} of the bound")
    assert r <= 1.0 and rp <= 1.0
    assert_gap(post, pb, f"kdeda {prior}")
    assert np.array_equal(p64[:-1], pred[:-1])
    assert np.all(d64[-1] == 0.0) and np.all(np.isnan(po64[-1])) and p64[-1, 0] == "a"     # the far query: lev[0]


@pytest.mark.parametrize("weighted,scal", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("prior", ["unif", "prop"])
def test_plskdeda_restatement_and_the_gap_of_the_seed(prior, weighted, scal):
    cl = clusters()
    T, Tq = oracle_scores(weighted, scal)
    rng = list(range(1, NLV + 1))
    ref = plskdeda_reference(T, Tq, cl["y"], prior, None, 1, rng)
    got = np_plskdeda_predict(np_plskdeda(T, cl["y"], NLV, prior=prior), Tq, rng)
    for k, (dens, bound, post, pb, pred), (p64, d64, po64) in zip(rng, ref, got):
        assert ratio(d64, dens, bound) <= 1.0 and ratio(po64[:-1], post[:-1], pb[:-1]) <= 1.0, k
        assert_gap(post, pb, f"plskdeda {prior} weighted={weighted} scal={scal} nlv={k}")
        assert np.array_equal(p64[:-1], pred[:-1]) and p64[-1, 0] == "a" and np.all(np.isnan(po64[-1]))


# ---------------------------------------------------------------------------------- the boundary
def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_header_prototype_symbols_and_makefile():
    import jchemo_hip as J
    hdr = _read("include", "jchemo_hip.h")
    m = re.search(r"JCH_API int32_t jch_kde_dens\(([^;]*?)\);", hdr, flags=re.S)
    assert m, "no prototype of jch_kde_dens"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 18, params
    assert [p.split()[-1].lstrip("*") for p in params] == ["ctx", "loc", "Z", "n", "d", "ldz", "Xq", "m", "ldq", "cls_start", "ncls", "u", "v2", "coef",
                                                          "dims", "nmod", "out", "ldo"]
    sec = hdr[:m.start()]
    sec = sec[sec.rindex("/* ----"):]
    for f in ("src/dmkern.jl", "src/kdeda.jl", "src/plskdeda.jl"):
        assert f in sec, f"the header section does not cite {f}"
    assert "jch_kde_dens" in J.SYMBOLS
    assert re.search(r"^SRCS :=.*\bkde\.hip\b", _read("jchemo.jl_amd", "csrc", "Makefile"), flags=re.M)
    assert "kd_ws" in _read("jchemo.jl_amd", "csrc", "jch_internal.h") and "&ctx->kd_ws" in _read("jchemo.jl_amd", "csrc", "ctx.hip")


def test_kernel_source_is_plain_hip():
    src = _read("jchemo.jl_amd", "csrc", "kde.hip")
    assert not re.search(r"\basm\b|__asm", src)
    assert not re.search(r"atomic[A-Z_]", src)
    assert "jch_knob" not in src and "getenv" not in src
    assert "ctx->xr" not in src and "ctx->xstage" not in src and "xcopy" not in src
    assert re.findall(r"jch_reserve\w*\(ctx, ([^,]+),", src) == ["ctx->kd_ws"]
    for name, val in (("KDE_QT", KDE_QT), ("KDE_DREG", KDE_DREG), ("KDE_DLDS", KDE_DLDS), ("KDE_MG", KDE_MG), ("KDE_CH", KDE_CH), ("KDE_ZL0", KDE_ZL0),
                      ("KDE_LDS", KDE_LDS), ("KDE_SPLIT_ROWS", KDE_SPLIT_ROWS)):
        assert re.search(rf"#define {name} {val}\b", src), name


def test_package_names_dataclasses_and_defaults():
    import jchemo_hip as J
    for nm in ("Dmkern", "Kernda", "dmkern", "dmkern_predict", "kdeda", "kdeda_predict", "plskdeda", "plskdeda_predict", "kde_dens"):
        assert hasattr(J, nm), nm
    assert [f.name for f in dataclasses.fields(J.Dmkern)] == ["X", "H", "Hinv", "detH"]          # src/dmkern.jl:1-6
    assert [f.name for f in dataclasses.fields(J.Kernda)] == ["fm", "wprior", "lev", "ni"]        # src/kdeda.jl:1-6

    def sig(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items() if k != "ctx"]
    E = inspect.Parameter.empty
    assert sig(J.dmkern) == [("X", E), ("h", None), ("a", 1)]
    assert sig(J.kdeda) == [("X", E), ("y", E), ("prior", "unif"), ("h", None), ("a", 1)]
    assert sig(J.plskdeda) == [("X", E), ("y", E), ("weights", None), ("nlv", E), ("prior", "unif"), ("h", None), ("a", 1), ("scal", False)]
    assert sig(J.plskdeda_predict) == [("obj", E), ("X", E), ("nlv", None)] == sig(J.plslda_predict)
    assert sig(J.dmkern_predict) == [("obj", E), ("X", E)] == sig(J.kdeda_predict)


def test_julia_mirror():
    src = _read("jchemo.jl_amd", "julia", "JchemoHIP.jl")
    exported = set(re.findall(r"[\w!]+", re.search(r"\nexport (.*?)\n\n", src, flags=re.S).group(1)))
    for nm in ("dmkern", "kdeda", "plskdeda", "Dmkern", "Kernda"):
        assert nm in exported, nm
    assert "(:jch_kde_dens, LIB)" in src
    for pat in (r"struct Dmkern", r"struct Kernda", r"function dmkern\(", r"function kdeda\(", r"function plskdeda\(", r"predict\(object::Dmkern",
                r"predict\(object::Kernda"):
        assert re.search(pat, src), pat


def test_bad_arguments_raise_before_any_device_work():
    """Every one of these is a ValueError on a machine without a GPU too: nothing has touched the device when it is raised."""
    import jchemo_hip as J
    rng = np.random.default_rng(1)
    X, y = rng.normal(size=(20, 3)), np.repeat([0, 1], 10)
    with pytest.raises(ValueError, match="prior"):
        J.kdeda(X, y, prior="flat")
    with pytest.raises(ValueError, match="prior"):
        J.plskdeda(X, y, nlv=2, prior="flat")
    with pytest.raises(ValueError, match="vector h"):
        J.plskdeda(X, y, nlv=2, h=[0.1, 0.2])
    with pytest.raises(ValueError, match="h has 2 entries"):
        J.dmkern(X, h=[0.1, 0.2])
    with pytest.raises(ValueError, match="h has 2 entries"):
        J.kdeda(X, y, h=[0.1, 0.2])
    with pytest.raises(ValueError, match="one row"):
        J.kdeda(X, np.r_[np.zeros(19), 1])
    with pytest.raises(ValueError, match="one row"):
        J.plskdeda(X, np.r_[np.zeros(19), 1], nlv=2)
    with pytest.raises(ValueError, match="one training row"):
        J.dmkern(X[:1])
    with pytest.raises(ValueError, match="constant column"):
        J.dmkern(np.c_[X, np.ones(20)])
    with pytest.raises(ValueError, match="constant column"):
        J.kdeda(np.c_[X, np.r_[np.ones(10), rng.normal(size=10)]], y)
    with pytest.raises(ValueError, match="20 rows, y has 5"):
        J.kdeda(X, y[:5])
    with pytest.raises(ValueError, match="20 rows, y has 5"):
        J.plskdeda(X, y[:5], nlv=2)
    # the restatement throws where the mirror raises
    with pytest.raises(np.linalg.LinAlgError):
        np_dmkern(X[:1])
    with pytest.raises(np.linalg.LinAlgError):
        np_dmkern(np.c_[X, np.zeros(20)])
    # given bandwidths need no device: the record is the reference's
    fm = J.dmkern(X, h=[0.1, 0.2, 0.4])
    ref = np_dmkern(X, h=[0.1, 0.2, 0.4])
    assert np.array_equal(fm.H, ref["H"]) and np.array_equal(fm.Hinv, ref["Hinv"]) and fm.detH == ref["detH"]
    assert J.dmkern(X, h=0.0 + 1e-200).detH == 1e-20               # det(H) underflows to 0 -> 1e-20 (src/dmkern.jl:141)


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import jchemo_hip as J
    X, y = np.random.default_rng(1).normal(size=(20, 3)), np.repeat([0, 1], 10)
    for call in (lambda: J.dmkern(X), lambda: J.dmkern_predict(J.dmkern(X, h=0.3), X), lambda: J.kdeda(X, y),
                 lambda: J.kdeda_predict(J.kdeda(X, y, h=0.3), X), lambda: J.plskdeda(X, y, nlv=2, h=0.3)):
        with pytest.raises(J.JchError) as ei:
            call()
        assert ei.value.code == J._lib.JCH_ENODEV
