"""CPU-side checks of the Gaussian discrimination family: line-by-line numpy restatements of the reference's src/dmnorm.jl, src/lda.jl, src/qda.jl,
src/matW.jl and `mahsqchol` of src/distances.jl with their predicts (in float64 and in np.longdouble, with a longdouble Cholesky and triangular
inverse written out here: numpy's LAPACK does not take longdouble), the input generators and the error bounds as functions (both shared with
tests/test_gpu_gda.py), and the boundary (header, SYMBOLS, Makefile, exports, dataclasses, defaults, Julia mirror, ValueErrors).

The bounds (u = 2^-53, eps = 2^-52, evaluated in longdouble):
  jch_class_cov   `gram_bound` of tests/test_pca_static.py on each class's rows with uniform weights (on all rows for a class of one row); W gets
                  the n_c / n weighted sum of the class bounds plus (ncls + 1) u |W|.
  jch_mahsq_chol  given Uinv: a_j = sum_{k <= j} |x_k - mu_k| |U_kj|, |dz_j| <= (j + 3) 2u a_j (j counted from 1: the terms of z_j),
                  bound[i, c] = sum_j (2 |z_j| dz_j + dz_j^2) + (p + 2) 2u d2.  No constant had to move.
  jch_gauss_factor and the models, norm-wise with the krr tests' constant: tol_f = 50 eps cond2(S_f);
                  |Uinv - Uinv_ld|_F <= tol |Uinv_ld|_F;  |d2 - d2_ld| <= tol d2_ld per element for a model fitted and evaluated end to end;
                  |dens - dens_ld| <= (0.5 d2 tol + p tol + 8 eps) dens_ld;  the posterior: the same relative bound on A pushed through the division
                  (`posterior_with_bound` of tests/test_kde_static.py).
The float64 restatements follow the reference's own arithmetic (x U - mu U, then |x|^2 + |y|^2 - 2 x.y of `Distances.pairwise`); `form="diff"`
switches the distance to the kernel's form (difference first), which is what the bound of jch_mahsq_chol is about."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_kde_static import posterior_with_bound, ratio, top_two_gap  # noqa: E402
from test_pca_static import gram_bound  # noqa: E402

EPS = 2.0 ** -52
U = 2.0 ** -53
LD = np.longdouble
OFFSET = 10.0


def ensure_mat(X, ft):
    X = np.asarray(X, dtype=ft)
    return X.reshape(1, 1) if X.ndim == 0 else X.reshape(-1, 1) if X.ndim == 1 else X


# ---------------------------------------------------------------------------------- longdouble linear algebra
def ld_cholesky(S):
    """Lower Cholesky factor in the dtype of S, column by column; raises LinAlgError at the first pivot that is not > 0."""
    S = np.array(S)
    p = S.shape[0]
    L = np.zeros_like(S)
    for j in range(p):
        d = S[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"PosDefException at column {j + 1}")
        L[j, j] = np.sqrt(d)
        if j + 1 < p:
            L[j + 1:, j] = (S[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def ld_triu_inv(Uu):
    """Inverse of an upper triangular matrix in its dtype, by back substitution column by column."""
    p = Uu.shape[0]
    X = np.zeros_like(Uu)
    for j in range(p):
        X[j, j] = 1 / Uu[j, j]
        for i in range(j - 1, -1, -1):
            X[i, j] = -(Uu[i, i + 1:j + 1] @ X[i + 1:j + 1, j]) / Uu[i, i]
    return X


def chol_uinv(S, ft):
    """(Uinv, diag(U)) of `LinearAlgebra.inv!(cholesky!(Hermitian(S)).U)`: LAPACK in float64, the routines above in longdouble."""
    if ft is LD:
        L = ld_cholesky(np.asarray(S, dtype=LD))
        return ld_triu_inv(L.T.copy()), np.diag(L).copy()
    L = np.linalg.cholesky(np.asarray(S, dtype=np.float64))
    return np.triu(np.linalg.inv(L.T)), np.diag(L).copy()


# ---------------------------------------------------------------------------------- numpy restatements of the reference
def np_cov(X, corrected):
    """`Statistics.cov(X; corrected)`."""
    n = X.shape[0]
    Xc = X - X.sum(axis=0) / n
    return Xc.T @ Xc / (n - 1 if corrected else n)


def np_euclsq(zX, zY):
    """`Distances.pairwise(SqEuclidean(), zX', zY')`: |x|^2 + |y|^2 - 2 x.y, clamped at 0."""
    return np.maximum((zX ** 2).sum(axis=1)[:, None] + (zY ** 2).sum(axis=1)[None, :] - 2 * (zX @ zY.T), 0)


def np_mahsqchol(X, Y, Uinv=None, ft=np.float64, form="ref"):
    """src/distances.jl:104-126."""
    X, Y = ensure_mat(X, ft), ensure_mat(Y, ft)
    if Uinv is None:
        S = np_cov(X, corrected=False)                              # :108
        Uinv = (1 / np.sqrt(S)) if X.shape[1] == 1 else chol_uinv(S, ft)[0]   # :109-113
    Uinv = ensure_mat(Uinv, ft)
    if form == "diff":                                              # the kernel's form
        return np.stack([(((X - Y[c]) @ Uinv) ** 2).sum(axis=1) for c in range(Y.shape[0])], axis=1)
    return np_euclsq(X @ Uinv, Y @ Uinv)                            # :123-125


def np_dmnorm(X=None, mu=None, S=None, ft=np.float64):
    """src/dmnorm.jl:107-128.  Returns dict(mu, Uinv, detS)."""
    if X is not None:
        X = ensure_mat(X, ft)
    if mu is None:
        mu = X.sum(axis=0) / X.shape[0]                             # :114
    if S is None:
        with np.errstate(invalid="ignore", divide="ignore"):
            S = np_cov(X, corrected=True)                           # :117
    S = ensure_mat(S, ft)
    if not np.all(np.isfinite(S)):
        raise np.linalg.LinAlgError("PosDefException")
    Uinv, dg = chol_uinv(S, ft)                                     # :119
    det = ft(1)
    for v in dg:
        det = det * v
    detS = det ** 2                                                 # :120
    if detS == 0:
        detS = ft(1e-20)                                            # :121
    return dict(mu=np.asarray(mu, dtype=ft).reshape(-1), Uinv=Uinv, detS=detS)


def np_dmnorm_predict(fm, X, form="ref"):
    """src/dmnorm.jl:136-143."""
    ft = fm["Uinv"].dtype.type
    X = ensure_mat(X, ft)
    p = X.shape[1]
    d = np_mahsqchol(X, fm["mu"].reshape(1, -1), fm["Uinv"], ft=ft, form=form)
    return (2 * ft(np.pi)) ** (-ft(p) / 2) * (1 / np.sqrt(fm["detS"])) * np.exp(-ft(.5) * d)


def np_matW(X, y, ft=np.float64):
    """src/matW.jl:44-75."""
    X = ensure_mat(X, ft)
    y = np.asarray(y).reshape(-1)
    lev, ni = np.unique(y, return_counts=True)
    if np.any(ni == 1):
        sigma_1obs = np_cov(X, corrected=False)                     # :55
    w = ni.astype(ft) / ni.sum()
    Wi, W = [], None
    for i in range(len(lev)):
        Wi.append(sigma_1obs if ni[i] == 1 else np_cov(X[y == lev[i]], corrected=False))
        W = w[i] * Wi[i] if i == 0 else W + w[i] * Wi[i]            # :69-73
    return dict(W=W, Wi=Wi, lev=lev, ni=ni)


def np_aggmean(X, y, lev):
    return np.stack([X[y == l].sum(axis=0) / np.sum(y == l) for l in lev])


def np_matB(X, y, ft=np.float64):
    """src/matW.jl:23-29 with `covm` of src/utility.jl:439-446."""
    X = ensure_mat(X, ft)
    y = np.asarray(y).reshape(-1)
    lev, ni = np.unique(y, return_counts=True)
    ct = np_aggmean(X, y, lev)
    w = ni.astype(ft) / ni.sum()
    z = np.sqrt(w)[:, None] * (ct - w @ ct)
    return dict(B=z.T @ z, ct=ct, lev=lev, ni=ni)


def _np_prior(prior, ni, ft):
    return np.ones(len(ni), dtype=ft) / len(ni) if prior == "unif" else ni.astype(ft) / ni.sum()


def np_lda(X, y, prior="unif", ft=np.float64):
    """src/lda.jl:56-77."""
    X = ensure_mat(X, ft)
    y = np.asarray(y).reshape(-1)
    n = X.shape[0]
    res = np_matW(X, y, ft)
    lev, ni = res["lev"], res["ni"]
    ct = np_aggmean(X, y, lev)
    with np.errstate(invalid="ignore", divide="ignore"):
        W = res["W"] * ft(n) / ft(n - len(lev))                     # :65
    fm = [np_dmnorm(mu=ct[i], S=W, ft=ft) for i in range(len(lev))]
    return dict(fm=fm, W=W, ct=ct, wprior=_np_prior(prior, ni, ft), lev=lev, ni=ni)


def np_qda(X, y, prior="unif", ft=np.float64):
    """src/qda.jl:55-79."""
    X = ensure_mat(X, ft)
    y = np.asarray(y).reshape(-1)
    res = np_matW(X, y, ft)
    lev, ni = res["lev"], res["ni"]
    ct = np_aggmean(X, y, lev)
    fm = []
    for i in range(len(lev)):
        S = res["Wi"][i] if ni[i] == 1 else res["Wi"][i] * ft(ni[i]) / ft(ni[i] - 1)   # :69-73
        fm.append(np_dmnorm(mu=ct[i], S=S, ft=ft))
    return dict(fm=fm, Wi=res["Wi"], ct=ct, wprior=_np_prior(prior, ni, ft), lev=lev, ni=ni)


def np_da_predict(obj, X, form="ref"):
    """src/lda.jl:85-101 = src/qda.jl:87-104: (pred, dens, posterior)."""
    dens = np.concatenate([np_dmnorm_predict(f, X, form=form) for f in obj["fm"]], axis=1)
    A = obj["wprior"][None, :] * dens
    with np.errstate(invalid="ignore", divide="ignore"):
        posterior = A / A.sum(axis=1, keepdims=True)
    return obj["lev"][np.argmax(posterior, axis=1)].reshape(-1, 1), dens, posterior


# ---------------------------------------------------------------------------------- the bounds
def cond2(S):
    return float(np.linalg.cond(np.asarray(S, dtype=np.float64)))


def factor_tol(S):
    """50 eps cond2(S): the krr tests' constant."""
    return 50 * EPS * cond2(S)


def ld_mahsq(Xq, Mu, Uinv):
    """(d2, bound), both (m, ncen) longdouble: jch_mahsq_chol's formula on the upper triangle of the given factor(s) — Uinv (p, p) or (ncen, p, p) —
    and the module docstring's bound."""
    Xq, Mu, Uinv = np.asarray(Xq, dtype=LD), np.asarray(Mu, dtype=LD), np.asarray(Uinv, dtype=LD)
    m, p = Xq.shape
    ncen = Mu.shape[0]
    d2, bound = np.zeros((m, ncen), dtype=LD), np.zeros((m, ncen), dtype=LD)
    jj = (np.arange(1, p + 1) + 3).astype(LD)
    for c in range(ncen):
        Uf = np.triu(Uinv if Uinv.ndim == 2 else Uinv[c])
        D = Xq - Mu[c]
        z = D @ Uf
        a = np.abs(D) @ np.abs(Uf)
        dz = jj[None, :] * 2 * LD(U) * a
        d2[:, c] = (z ** 2).sum(axis=1)
        bound[:, c] = (2 * np.abs(z) * dz + dz ** 2).sum(axis=1) + (p + 2) * 2 * LD(U) * d2[:, c]
    return d2, bound


def class_cov_reference(Z, cs):
    """Per-class longdouble (Wi, its bound, ct, its bound, W, its bound) of jch_class_cov on grouped rows."""
    Z = np.asarray(Z, dtype=LD)
    n, p = Z.shape
    ncls = len(cs) - 1
    Wi, Bi, ct, Bct = [], [], [], []
    for c in range(ncls):
        Zc = Z[cs[c]:cs[c + 1]]
        ct.append(Zc.sum(axis=0) / Zc.shape[0])
        src = Z if Zc.shape[0] == 1 else Zc                         # the one-row rule (src/matW.jl:54-65)
        Wi.append(np_cov(src, corrected=False))
        gb, mb = gram_bound(src)
        Bi.append(np.asarray(gb, dtype=LD))
        Bct.append(np.zeros(p, dtype=LD) if Zc.shape[0] == 1 else np.asarray(mb, dtype=LD))
    w = [LD(int(cs[c + 1] - cs[c])) / n for c in range(ncls)]
    W = sum(w[c] * Wi[c] for c in range(ncls))
    BW = sum(w[c] * Bi[c] for c in range(ncls)) + (ncls + 1) * LD(U) * np.abs(W)
    return np.stack(Wi), np.stack(Bi), np.stack(ct), np.stack(Bct), W, BW


def dens_bound(d2, dens, tol, p):
    """|dens - dens_ld| <= (0.5 d2 tol + p tol + 8 eps) dens_ld; tol per class (column)."""
    tol = np.asarray(tol, dtype=LD)[None, :]
    return (LD(0.5) * d2 * tol + p * tol + 8 * LD(EPS)) * dens


def model_reference(kind, X, y, Xq, prior):
    """Longdouble lda / qda end to end: dict(obj, tol (per class), d2, dens, dens_bound, post, post_bound, pred)."""
    obj = (np_lda if kind == "lda" else np_qda)(X, y, prior=prior, ft=LD)
    p = np.asarray(X).shape[1]
    Mu = np.stack([f["mu"] for f in obj["fm"]])
    Us = np.stack([f["Uinv"] for f in obj["fm"]])
    d2, _ = ld_mahsq(Xq, Mu, Us)
    _, dens, post = np_da_predict(obj, np.asarray(Xq, dtype=LD), form="diff")
    Ss = [obj["W"]] * len(obj["lev"]) if kind == "lda" else [np.linalg.inv(np.asarray(u @ u.T, dtype=np.float64)) for u in Us]
    tol = np.array([factor_tol(S) for S in Ss])
    db = dens_bound(d2, dens, tol, p)
    post2, pb = posterior_with_bound(obj["wprior"], dens, db)
    return dict(obj=obj, tol=tol, d2=d2, dens=dens, dens_bound=db, post=post2, post_bound=pb, pred=obj["lev"][np.argmax(post2, axis=1)].reshape(-1, 1))


def assert_model(kind, got_pred, got_dens, got_post, ref, what, got_d2=None):
    """dens, posterior and labels of a prediction against `model_reference`, the way the issue sets it; prints the ratios first."""
    r_d = ratio(got_dens, ref["dens"], ref["dens_bound"])
    r_p = ratio(got_post, ref["post"], ref["post_bound"])
    gap = top_two_gap(ref["post"])
    skip = gap < 2 * np.max(np.asarray(ref["post_bound"], dtype=np.float64), axis=1)
    msg = f"{what}: dens {r_d:.3f}, posterior {r_p:.3f} of the bound; smallest top-two gap {gap.min():.3e}; {int(skip.sum())} queries left out of the labels"
    if got_d2 is not None:
        r_2 = ratio(got_d2, ref["d2"], np.asarray(ref["tol"], dtype=LD)[None, :] * ref["d2"])
        msg += f"; d2 {r_2:.3f}"
        assert r_2 <= 1.0, msg
    print(msg)
    assert r_d <= 1.0 and r_p <= 1.0, msg
    assert skip.sum() <= 0.02 * len(skip), msg
    assert np.array_equal(np.asarray(got_pred)[~skip], ref["pred"][~skip]), msg


# ---------------------------------------------------------------------------------- inputs
def prim_inputs(seed, m, p, ncen, nfac):
    """Inputs of one jch_mahsq_chol call: queries and centres at offset 10 with a spread of 0.05 and 0.025 (spectra: a large offset, a small
    spread), upper triangular factors with a diagonal in [0.5, 1.5] / 0.05 and off-diagonal entries of order 1 / (0.05 sqrt(p)) (so that d2
    stays of order p)."""
    rng = np.random.default_rng(seed)
    Xq = np.asfortranarray(OFFSET + 0.05 * rng.normal(size=(m, p)))
    Mu = np.asfortranarray(OFFSET + 0.025 * rng.normal(size=(ncen, p)))
    Us = (np.triu(rng.normal(size=(nfac, p, p)) / np.sqrt(p), 1) + np.stack([np.diag(rng.uniform(0.5, 1.5, size=p)) for _ in range(nfac)])) / 0.05
    return Xq, Mu, Us


PRIM_M = (1, 127, 128, 129, 257)
PRIM_P = (1, 15, 16, 17, 127, 128, 129, 260)


@lru_cache(maxsize=None)
def prim_case(m, p, ncen, nfac):
    """(Xq, Mu, Us, longdouble d2, bound) of one primitive case; computed once, shared, not to be written to."""
    Xq, Mu, Us = prim_inputs(1000 * m + 10 * p + ncen + nfac, m, p, ncen, nfac)
    d2, bound = ld_mahsq(Xq, Mu, Us[0] if nfac == 1 else Us)
    for a in (Xq, Mu, Us, d2, bound):
        a.setflags(write=False)
    return Xq, Mu, Us, d2, bound


MODEL_SHAPES = {"n120_p5": (120, 5, 3, 257), "n300_p20": (300, 20, 3, 385)}
BIG_SHAPE = (400, 130, 2, 64)
SEP = 4.0


@lru_cache(maxsize=None)
def gauss_classes(n, p, nlev, m, seed=20251020, sizes=None):
    """Correlated Gaussian classes, every column offset by 10 (p >= nlev): A_0 = Q diag(s) with singular values s from 0.5 down to 0.05 (cond2 of the
    population covariance 1e2), class k has the covariance A_k A_k' with A_k = A_0 (I + 0.15 G_k / sqrt(p)) and the centre A_0 (SEP e_k): the
    classes are SEP sqrt(2) = 5.7 standard deviations apart in every class's own metric, up to the 15 % (about 99 % accuracy, and squared distances
    to the wrong class of order 20 + p, far from the underflow of `exp`); rows shuffled.  m queries from the same classes."""
    rng = np.random.default_rng(seed + 7 * n + p)
    s = np.geomspace(0.5, 0.05, p)
    A0 = np.linalg.qr(rng.normal(size=(p, p)))[0] * s[None, :]
    As = [A0 @ (np.eye(p) + 0.15 * rng.normal(size=(p, p)) / np.sqrt(p)) for _ in range(nlev)]
    centres = SEP * A0[:, :nlev].T
    grouped = sizes is not None
    sizes = sizes or tuple(n // nlev + (1 if k < n % nlev else 0) for k in range(nlev))
    lab = np.repeat(np.arange(nlev), sizes)
    X = OFFSET + centres[lab] + np.stack([As[k] @ rng.normal(size=p) for k in lab])
    perm = np.arange(n) if grouped else rng.permutation(n)
    X, y = np.asfortranarray(X[perm]), np.array([f"c{k}" for k in lab])[perm]
    lq = rng.integers(0, nlev, size=m)
    Xq = np.asfortranarray(OFFSET + centres[lq] + np.stack([As[k] @ rng.normal(size=p) for k in lq]))
    for a in (X, Xq, y):
        a.setflags(write=False)
    return X, y, Xq, np.array([f"c{k}" for k in lq])


@lru_cache(maxsize=None)
def model_case(kind, shape, prior):
    n, p, nlev, m = MODEL_SHAPES[shape]
    X, y, Xq, _ = gauss_classes(n, p, nlev, m)
    return model_reference(kind, X, y, Xq, prior)


def one_row_classes():
    """(40, 5) in 4 classes of (1, 2, 30, 7) rows, grouped, for the one-row rule."""
    X, _, _, _ = gauss_classes(40, 5, 4, 8, sizes=(1, 2, 30, 7))    # (sizes given: the rows stay grouped)
    return np.asfortranarray(X), np.array([0, 1, 3, 33, 40], dtype=np.int64)


# ---------------------------------------------------------------------------------- the restatements against each other and the bounds
def test_longdouble_is_extended_precision_and_its_factorisation_is_one():
    assert np.finfo(LD).eps < 1e-18
    rng = np.random.default_rng(3)
    A = rng.normal(size=(40, 12))
    S = np.asarray(A.T @ A / 40, dtype=LD)
    L = ld_cholesky(S)
    Ui = ld_triu_inv(L.T.copy())
    assert np.max(np.abs(L @ L.T - S)) < 1e-17 and np.max(np.abs(Ui @ L.T - np.eye(12))) < 1e-16
    assert np.all(np.tril(Ui, -1) == 0)
    with pytest.raises(np.linalg.LinAlgError, match="column 3"):
        ld_cholesky(np.asarray(np.diag([1.0, 2.0, 0.0, 1.0]), dtype=LD))


@pytest.mark.parametrize("p", PRIM_P)
@pytest.mark.parametrize("nfac", [1, 3])
def test_mahsq_float64_kernel_form_stays_inside_the_bound_and_the_reference_form_misses_it(p, nfac):
    Xq, Mu, Us, d2, bound = prim_case(129, p, 3, nfac)
    Uf = Us[0] if nfac == 1 else Us
    got = np.stack([np_mahsqchol(Xq, Mu[c:c + 1], Uf if nfac == 1 else Uf[c], form="diff")[:, 0] for c in range(3)], axis=1)
    ref = np.stack([np_mahsqchol(Xq, Mu[c:c + 1], Uf if nfac == 1 else Uf[c], form="ref")[:, 0] for c in range(3)], axis=1)
    r, rr = ratio(got, d2, bound), ratio(ref, d2, bound)
    print(f"p={p} nfac={nfac}: float64 difference-first {r:.3f} of the bound, the reference's x U - mu U / pairwise form {rr:.1f}")
    assert r <= 1.0
    assert rr > 1.0          # the bound is not vacuous: the offset costs the reference's form its digits


def test_class_cov_float64_restatement_stays_inside_the_bound():
    for Z, cs in [one_row_classes(), (gauss_classes(50, 17, 3, 4)[0], np.array([0, 16, 33, 50]))]:
        Wi, Bi, ct, Bct, W, BW = class_cov_reference(Z, cs)
        n = Z.shape[0]
        Wi64 = [np_cov(Z if cs[c + 1] - cs[c] == 1 else Z[cs[c]:cs[c + 1]], corrected=False) for c in range(len(cs) - 1)]
        W64 = sum((cs[c + 1] - cs[c]) / n * Wi64[c] for c in range(len(cs) - 1))
        r1, r2 = ratio(np.stack(Wi64), Wi, Bi), ratio(W64, W, BW)
        print(f"class_cov n={n}: Wi {r1:.3f}, W {r2:.3f} of the bound")
        assert r1 <= 1.0 and r2 <= 1.0


@pytest.mark.parametrize("shape", list(MODEL_SHAPES))
def test_generators_keep_cond_below_1e6_and_the_labels_decided(shape):
    n, p, nlev, m = MODEL_SHAPES[shape]
    X, y, Xq, yq = gauss_classes(n, p, nlev, m)
    for kind in ("lda", "qda"):
        for prior in ("unif", "prop"):
            ref = model_case(kind, shape, prior)
            c = ref["tol"].max() / (50 * EPS)
            gap = top_two_gap(ref["post"])
            need = 2 * np.max(np.asarray(ref["post_bound"], dtype=np.float64), axis=1)
            acc = np.mean(ref["pred"][:, 0] == yq)
            print(f"{shape} {kind} {prior}: cond2 <= {c:.3e}, accuracy {acc:.3f}, smallest top-two gap {gap.min():.3e}, largest 2 x bound {need.max():.3e}")
            assert c <= 1e6 and acc >= 0.97 and np.all(gap > need)
            assert not np.any(np.isnan(np.asarray(ref["post"], dtype=np.float64)))


@pytest.mark.parametrize("kind", ["lda", "qda"])
@pytest.mark.parametrize("shape", list(MODEL_SHAPES))
def test_float64_restatement_against_longdouble(kind, shape):
    n, p, nlev, m = MODEL_SHAPES[shape]
    X, y, Xq, _ = gauss_classes(n, p, nlev, m)
    ref = model_case(kind, shape, "prop")
    obj = (np_lda if kind == "lda" else np_qda)(X, y, prior="prop")
    pred, dens, post = np_da_predict(obj, Xq, form="diff")
    d2 = np.stack([np_mahsqchol(Xq, f["mu"].reshape(1, -1), f["Uinv"], form="diff")[:, 0] for f in obj["fm"]], axis=1)
    assert_model(kind, pred, dens, post, ref, f"float64 {kind} {shape}", got_d2=d2)
    for f, fl in zip(obj["fm"], ref["obj"]["fm"]):
        assert np.linalg.norm(np.asarray(f["Uinv"] - fl["Uinv"], dtype=np.float64)) <= ref["tol"].max() * np.linalg.norm(np.asarray(fl["Uinv"], dtype=np.float64))
    pr, _, _ = np_da_predict(obj, Xq, form="ref")                   # the reference's own arithmetic decides the same labels
    assert np.array_equal(pr, ref["pred"])


def test_big_case_distances_in_float64_against_longdouble():
    """(400, 130, 2): d2 only, through `mahsqchol` on the covariance of all rows (at this p the reference's densities leave the float64 range on all
    but well-conditioned data; the distances have no such limit)."""
    n, p, nlev, m = BIG_SHAPE
    X, y, Xq, _ = gauss_classes(n, p, nlev, m)
    S = np_cov(np.asarray(X), corrected=False)
    assert cond2(S) <= 1e6
    d64 = np_mahsqchol(X, Xq[:2], form="diff")
    dld = np_mahsqchol(X, Xq[:2], ft=LD, form="diff")
    r = float(np.max(np.abs(d64 - dld) / dld)) / factor_tol(S)
    print(f"big case: cond2 {cond2(S):.3e}, float64 d2 {r:.4f} of 50 eps cond")
    assert r <= 1.0


def test_matB_plus_matW_is_the_total_covariance():
    X, y, _, _ = gauss_classes(120, 5, 3, 257)
    tot = np_matW(X, y)["W"] + np_matB(X, y)["B"]
    assert np.allclose(tot, np_cov(np.asarray(X), corrected=False), rtol=1e-10, atol=1e-13)


def test_dmnorm_density_integrates_to_one():
    x = np.random.default_rng(3).normal(size=40) * 0.7 + 3
    fm = np_dmnorm(x)
    sd = 1 / fm["Uinv"][0, 0]
    g = np.linspace(3 - 12 * sd, 3 + 12 * sd, 4001)
    f = np_dmnorm_predict(fm, g)[:, 0]
    step = g[1] - g[0]
    assert abs(step * (f.sum() - 0.5 * (f[0] + f[-1])) - 1) <= step ** 2 / 12 * (g[-1] - g[0]) / (np.sqrt(2 * np.pi) * sd ** 3) + 1e-12


# ---------------------------------------------------------------------------------- the boundary
def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


PROTOS = {
    "jch_class_cov": ["ctx", "loc", "Z", "n", "p", "ldz", "cls_start", "ncls", "Wi", "W", "ct"],
    "jch_gauss_factor": ["ctx", "loc", "S", "p", "lds", "sstride", "nfac", "Uinv", "ldu", "ustride", "diagU", "info"],
    "jch_mahsq_chol": ["ctx", "loc", "Xq", "m", "p", "ldq", "Mu", "ncen", "Uinv", "ldu", "ustride", "nfac", "out", "ldo"],
}


def test_header_prototypes_symbols_and_makefile():
    import jchemo_hip as J
    hdr = _read("include", "jchemo_hip.h")
    for name, params in PROTOS.items():
        m = re.search(rf"JCH_API int32_t {name}\(([^;]*?)\);", hdr, flags=re.S)
        assert m, f"no prototype of {name}"
        assert [p.strip().split()[-1].lstrip("*") for p in m.group(1).split(",")] == params
        assert name in J.SYMBOLS
    sec = hdr[:hdr.index("JCH_API int32_t jch_class_cov")]
    sec = sec[sec.rindex("/* ----"):]
    for f in ("src/matW.jl", "src/dmnorm.jl", "src/lda.jl", "src/qda.jl", "src/distances.jl"):
        assert f in sec, f"the header section does not cite {f}"
    assert re.search(r"^SRCS :=.*\bgda\.hip\b", _read("jchemo.jl_amd", "csrc", "Makefile"), flags=re.M)
    assert "gd_ws" in _read("jchemo.jl_amd", "csrc", "jch_internal.h") and "&ctx->gd_ws" in _read("jchemo.jl_amd", "csrc", "ctx.hip")
    assert "jch_launch_chol_inv_t" in _read("jchemo.jl_amd", "csrc", "jch_internal.h")


def test_kernel_source_is_plain_hip():
    src = _read("jchemo.jl_amd", "csrc", "gda.hip")
    assert not re.search(r"\basm\b|__asm", src)
    assert not re.search(r"atomic[A-Z_]", src)
    assert "jch_knob" not in src and "getenv" not in src
    assert "ctx->xr" not in src and "ctx->xstage" not in src and "xcopy" not in src
    assert set(re.findall(r"jch_reserve\w*\(ctx, ([^,]+),", src)) == {"ctx->gd_ws"}
    assert "t128_mma" in src and "T128_LDS_BYTES" in src and "no scratch" in src


def test_package_names_dataclasses_and_defaults():
    import jchemo_hip as J
    for nm in ("Dmnorm", "Lda", "Qda", "dmnorm", "dmnorm_predict", "lda", "lda_predict", "qda", "qda_predict", "matW", "matB", "mahsqchol", "class_cov",
               "gauss_factor", "mahsq_chol"):
        assert hasattr(J, nm), nm
    assert [f.name for f in dataclasses.fields(J.Dmnorm)] == ["mu", "Uinv", "detS"]                      # src/dmnorm.jl:1-5
    assert [f.name for f in dataclasses.fields(J.Lda)] == ["fm", "W", "ct", "wprior", "lev", "ni"]      # src/lda.jl:1-8
    assert [f.name for f in dataclasses.fields(J.Qda)] == ["fm", "Wi", "ct", "wprior", "lev", "ni"]     # src/qda.jl:1-8

    def sig(fn):
        return [(k, v.default) for k, v in inspect.signature(fn).parameters.items() if k != "ctx"]
    E = inspect.Parameter.empty
    assert sig(J.dmnorm) == [("X", None), ("mu", None), ("S", None)]
    assert sig(J.lda) == [("X", E), ("y", E), ("prior", "unif")] == sig(J.qda)
    assert sig(J.lda_predict) == [("obj", E), ("X", E)] == sig(J.qda_predict) == sig(J.dmnorm_predict)
    assert sig(J.matW) == [("X", E), ("y", E)] == sig(J.matB)
    assert sig(J.mahsqchol) == [("X", E), ("Y", E), ("Uinv", None)]
    import jchemo_hip.gda as G
    import jchemo_hip.kde as K
    for nm in ("_labels", "_wprior", "_group_by_class", "_posterior"):                                 # reused, not copied
        assert getattr(G, nm) is getattr(K, nm)


def test_julia_mirror():
    src = _read("jchemo.jl_amd", "julia", "JchemoHIP.jl")
    exported = set(re.findall(r"[\w!]+", re.search(r"\nexport (.*?)\n\n", src, flags=re.S).group(1)))
    for nm in ("dmnorm", "lda", "qda", "matW", "matB", "mahsqchol", "Dmnorm", "Lda", "Qda"):
        assert nm in exported, nm
    for sym in PROTOS:
        assert f"(:{sym}, LIB)" in src
    for pat in (r"struct Dmnorm", r"struct Lda", r"struct Qda", r"function dmnorm\(", r"function lda\(", r"function qda\(", r"function matW\(",
                r"function matB\(", r"function mahsqchol\(", r"predict\(object::Dmnorm", r"predict\(object::Lda", r"predict\(object::Qda"):
        assert re.search(pat, src), pat


def test_bad_arguments_raise_before_any_device_work():
    """Every one of these is a ValueError on a machine without a GPU too: nothing has touched the device when it is raised."""
    import jchemo_hip as J
    rng = np.random.default_rng(1)
    X, y = rng.normal(size=(20, 3)), np.repeat([0, 1], 10)
    for fit in (J.lda, J.qda):
        with pytest.raises(ValueError, match="prior"):
            fit(X, y, prior="flat")
        with pytest.raises(ValueError, match="20 rows, y has 5"):
            fit(X, y[:5])
    for fn in (J.matW, J.matB):
        with pytest.raises(ValueError, match="20 rows, y has 5"):
            fn(X, y[:5])
    with pytest.raises(ValueError, match="give X, or both mu and S"):
        J.dmnorm()
    with pytest.raises(ValueError, match="give X, or both mu and S"):
        J.dmnorm(mu=np.zeros(3))
    with pytest.raises(ValueError, match="give X, or both mu and S"):
        J.dmnorm(S=np.eye(3))
    with pytest.raises(ValueError, match="mu has 2 entries"):
        J.dmnorm(mu=np.zeros(2), S=np.eye(3))
    U3 = np.asfortranarray(np.eye(3))
    fm = J.Dmnorm(np.zeros(3), U3, 1.0)
    with pytest.raises(ValueError, match="X has 2 columns, the model has 3"):
        J.dmnorm_predict(fm, X[:, :2])
    ct = np.zeros((2, 3))
    with pytest.raises(ValueError, match="X has 2 columns, the model has 3"):
        J.lda_predict(J.Lda([fm, fm], U3, ct, np.ones(2) / 2, np.array([0, 1]), np.array([10, 10])), X[:, :2])
    with pytest.raises(ValueError, match="X has 2 columns, the model has 3"):
        J.qda_predict(J.Qda([fm, fm], None, ct, np.ones(2) / 2, np.array([0, 1]), np.array([10, 10])), X[:, :2])
    with pytest.raises(ValueError, match="X has 3 columns, Y has 2"):
        J.mahsqchol(X, X[:2, :2])
    # the restatement throws where the mirror raises a PosDefException
    with pytest.raises(np.linalg.LinAlgError):
        np_dmnorm(X[:1])
    with pytest.raises(np.linalg.LinAlgError):
        np_qda(np.r_[X[:19], [[X[18, 0], 0.5, 0.25]]], np.r_[np.zeros(18), np.ones(2)])   # a class with n_c <= p whose first pivot is exactly 0
    with pytest.raises(np.linalg.LinAlgError):
        np_lda(X[:2], [0, 1])                                       # n == nlev


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import jchemo_hip as J
    X, y = np.random.default_rng(1).normal(size=(20, 3)), np.repeat([0, 1], 10)
    for call in (lambda: J.dmnorm(X), lambda: J.dmnorm(mu=np.zeros(3), S=np.eye(3)), lambda: J.lda(X, y), lambda: J.qda(X, y), lambda: J.matW(X, y),
                 lambda: J.matB(X, y), lambda: J.mahsqchol(X, X[:2]), lambda: J.mahsqchol(X, X[:2], np.asfortranarray(np.eye(3)))):
        with pytest.raises(J.JchError) as ei:
            call()
        assert ei.value.code == J._lib.JCH_ENODEV
