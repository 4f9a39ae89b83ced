"""Static checks of the PCA / PCR surface (pcasvd, pcaeigen, pcaeigenk, pcr, jch_xtdx): the literal numpy restatements of
src/pcasvd.jl:79-101,110-146 and src/pcr.jl:82-97 the GPU tests compare against, the algebra the device route relies on (the eigen route,
the summary identities), the elementwise error bound of the Gram kernel, and the header / Python / Julia surface.  No GPU needed."""
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_julia_wrapper import JL, header_protos  # noqa: E402

PCA_FIELDS = ["T", "P", "sv", "xmeans", "xscales", "weights", "niter", "conv", "eig", "sstot", "colvar", "resid", "converged"]
PCR_FIELDS = ["fm_pca", "T", "R", "C", "xmeans", "xscales", "ymeans", "yscales", "weights"]
U = 2.0 ** -53   # unit roundoff of float64


# ---------------------------------------------------------------------------------- numpy restatements of the reference
def _mweight(weights, n):
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    return w / w.sum()


def np_pcasvd(X, weights=None, *, nlv, scal=False):
    """src/pcasvd.jl:79-101 line by line.  A dict with the reference's fields (sv: all min(n, p) values) plus Xs = the centred, scaled X."""
    X = np.array(X, dtype=np.float64)
    n, p = X.shape
    nlv = min(nlv, n, p)                                                  # :82
    w = _mweight(weights, n)                                              # :83
    xmeans = w @ X                                                        # :84 colmean
    xscales = np.ones(p)
    if scal:
        xscales = np.sqrt(w @ (X - xmeans) ** 2)                          # :87 colstd (uncorrected, weighted)
    Xs = (X - xmeans) / xscales                                           # :88 / :90
    sqrtw = np.sqrt(w)                                                    # :94
    Us, S, Vt = np.linalg.svd(sqrtw[:, None] * Xs, full_matrices=False)   # :95
    P = Vt.T[:, :nlv]                                                     # :96
    sv = S.copy()                                                         # :97
    sv[sv < 0] = 0                                                        # :98
    with np.errstate(divide="ignore", invalid="ignore"):
        T = (1.0 / sqrtw)[:, None] * Us[:, :nlv] * sv[:nlv]               # :99
    zero = sqrtw == 0
    if zero.any():                                                        # (1 / 0 on a zero weight: the row's score is Xs P, which :99 equals elsewhere)
        T[zero] = Xs[zero] @ P
    return dict(T=T, P=P, sv=sv, xmeans=xmeans, xscales=xscales, weights=w, Xs=Xs)


def np_pca_transform(fm, Xnew, nlv=None):
    """src/pcasvd.jl:110-115."""
    a = fm["T"].shape[1]
    nlv = a if nlv is None else min(nlv, a)
    return (np.asarray(Xnew, dtype=np.float64) - fm["xmeans"]) / fm["xscales"] @ fm["P"][:, :nlv]


def np_pca_summary(fm, X):
    """src/pcasvd.jl:123-146, reading X as the reference does."""
    w, T = fm["weights"], fm["T"]
    Xs = (np.asarray(X, dtype=np.float64) - fm["xmeans"]) / fm["xscales"]   # :127
    sstot = np.sum(w @ Xs ** 2)                                           # :128
    TT = w[:, None] * T ** 2                                              # :129
    tt = TT.sum(axis=0)                                                   # :130
    pvar = tt / sstot
    explvarx = dict(lv=np.arange(1, T.shape[1] + 1), var=tt, pvar=pvar, cumpvar=np.cumsum(pvar))
    contr_ind = TT / tt                                                   # :138
    xm, tm = w @ Xs, w @ T                                                # :139 corm: weighted correlation of the columns of Xs and T
    cov = (Xs - xm).T @ (w[:, None] * (T - tm))
    cor_circle = cov / np.outer(np.sqrt(w @ (Xs - xm) ** 2), np.sqrt(w @ (T - tm) ** 2))
    Cv = Xs.T @ (w[:, None] * (T / np.sqrt(tt)))                          # :140
    CC = Cv * Cv                                                          # :142
    contr_var = CC / CC.sum(axis=0, keepdims=True)                        # :143-144
    return dict(explvarx=explvarx, contr_ind=contr_ind, contr_var=contr_var, coord_var=Cv, cor_circle=cor_circle)


def np_pcr(X, Y, weights=None, *, nlv, scal=False):
    """src/pcr.jl:82-97."""
    Y = np.asarray(Y, dtype=np.float64).reshape(len(Y), -1)
    fm = np_pcasvd(X, weights, nlv=nlv, scal=scal)                        # :91
    w, T = fm["weights"], fm["T"]
    ymeans = w @ Y                                                        # :86
    beta = np.linalg.solve(T.T @ (w[:, None] * T), T.T @ (w[:, None] * Y))   # :93
    return dict(fm_pca=fm, T=T, R=fm["P"], C=beta.T, xmeans=fm["xmeans"], xscales=fm["xscales"], ymeans=ymeans, yscales=np.ones(Y.shape[1]), weights=w)


def np_pcr_coef(fm, nlv=None):
    """`coef(object::Union{Plsr, Pcr}; nlv)` — src/plskern.jl:207-217."""
    a = fm["R"].shape[1]
    nlv = a if nlv is None else min(nlv, a)
    B = (fm["R"][:, :nlv] / fm["xscales"][:, None]) @ fm["C"][:, :nlv].T * fm["yscales"][None, :]
    return B, fm["ymeans"][None, :] - fm["xmeans"][None, :] @ B


def np_pcr_predict(fm, X, nlv=None):
    B, b0 = np_pcr_coef(fm, nlv)
    return b0 + np.asarray(X, dtype=np.float64) @ B


def _data(n, p, seed):
    """X = U diag(s) V' sqrt(n) + 100 + column offsets: orthonormal U (n x r) and V (p x r), r = min(n - 1, p), s_k = max(0.85^k, 1e-6): spectra
    at level 100 with a decaying spread, an eigenvalue ratio of 0.72 between neighbours of Xc'Xc / n."""
    rng = np.random.default_rng(seed)
    r = min(n - 1, p)
    if r < 1:
        return np.asfortranarray(100.0 + rng.standard_normal((n, p)))
    Uo, _ = np.linalg.qr(rng.standard_normal((n, r)))
    Vo, _ = np.linalg.qr(rng.standard_normal((p, r)))
    s = np.maximum(0.85 ** np.arange(r), 1e-6)
    return np.asfortranarray((Uo * s) @ Vo.T * np.sqrt(n) + 100.0 + rng.standard_normal(p)[None, :])


def _weights(kind, n, seed=5):
    if kind == "ones":
        return None
    rng = np.random.default_rng(seed)
    w = rng.random(n) + 0.05
    if kind == "zeros":
        w[rng.choice(n, max(n // 10, 1 if n > 1 else 0), replace=False)] = 0.0
    return w


# ---------------------------------------------------------------------------------- the Gram kernel's reference and error bound
def gram_longdouble(X, weights=None):
    """(G, mu) = ((X - 1 mu')' D (X - 1 mu'), X'D 1) in extended precision."""
    X = np.asarray(X, dtype=np.longdouble)
    n = X.shape[0]
    w = np.ones(n, dtype=np.longdouble) if weights is None else np.asarray(weights, dtype=np.longdouble)
    d = w / w.sum()
    mu = d @ X
    Xc = X - mu
    return Xc.T @ (d[:, None] * Xc), mu


def gram_bound(X, weights=None):
    """Elementwise bounds (|G - G_hat|, |mu - mu_hat|) for jch_xtdx, u = 2^-53.

    The weights.  d_hat_r = fl(w_r / fl(sum w)): a sum of n terms in any order ((n - 1) u) and a division (u): |d_hat_r - d_r| <= n u d_r.
    The means.  mu_hat_j = sum_r d_hat_r x_rj on the matrix cores: the products are exact inside the fused multiply-adds, the n-term sum costs
    (n - 1) u in ANY order (chunks of 4 rows per instruction, the workgroups' row tiles, then the fixed-order sum of the partials: a tree whose
    every leaf-to-root path has at most n - 1 additions), so with the weights' error
        delta_j = |mu_hat_j - mu_j| <= (2 n + 3) u sum_r d_r |x_rj|.
    The Gram pass.  A term is fl(d_hat_r fl(x_ri - mu_hat_i)) * fl(x_rj - mu_hat_j): one rounding per centring (2 u), one for the product with
    d_hat (u), the weight's own error (n u); the product of the two operands is exact inside the instruction.  The sum runs over 16-row chunks,
    4 rows per instruction, inside a row split, and the splits are added in order by the reduction kernel: again at most n - 1 additions on any
    path, (n - 1) u.  Together (2 n + 2) u, taken as c = 1 with n_terms = 2 n + 4, on the magnitudes |x_ri - mu_hat_i| <= |x_ri - mu_i| + delta_i.
    The rounded means shift the exact result by delta_i delta_j (sum_r d_r (x_ri - mu_i) = 0 kills the first-order terms).  1.01 covers what is
    of second order in u."""
    X = np.asarray(X, dtype=np.longdouble)
    n = X.shape[0]
    w = np.ones(n, dtype=np.longdouble) if weights is None else np.asarray(weights, dtype=np.longdouble)
    d = w / w.sum()
    mu = d @ X
    delta = (2 * n + 3) * U * (d @ np.abs(X))
    A = np.abs(X - mu) + delta
    S = A.T @ (d[:, None] * A)
    return np.asarray(1.01 * ((2 * n + 4) * U * S + np.outer(delta, delta)), dtype=np.float64), np.asarray(1.01 * delta, dtype=np.float64)


def _gram_float64_like_the_kernel(X, weights, chunk=16, nsplit=3):
    """A float64 emulation of the kernel's order: centred in registers, 4 rows per step, chunks inside a row split, the splits added in order."""
    X = np.asarray(X, dtype=np.float64)
    n, p = X.shape
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    d = w / np.sum(w)
    mu = np.zeros(p)
    for r in range(n):
        mu = mu + d[r] * X[r]
    per = -(-(-(-n // nsplit)) // chunk) * chunk
    G = np.zeros((p, p))
    for s0 in range(0, n, per):
        acc = np.zeros((p, p))
        for r0 in range(s0, min(n, s0 + per), 4):
            Xc = X[r0:min(r0 + 4, n, s0 + per)] - mu
            acc = acc + (Xc * d[r0:r0 + Xc.shape[0], None]).T @ Xc
        G = G + acc
    return G, mu


# ---------------------------------------------------------------------------------- tests: the restatements and the algebra
@pytest.mark.parametrize("n,p,nlv,wkind,scal", [(60, 7, 5, "ones", False), (60, 7, 7, "rand", True), (40, 55, 6, "zeros", False), (33, 1, 1, "ones", False)])
def test_restatement_invariants_and_the_eigen_route(n, p, nlv, wkind, scal):
    X = _data(n, p, n + p)
    w = _weights(wkind, n)
    fm = np_pcasvd(X, w, nlv=nlv, scal=scal)
    T, P, sv, D, Xs = fm["T"], fm["P"], fm["sv"], fm["weights"], fm["Xs"]
    a = P.shape[1]
    e1 = sv[0] ** 2
    assert np.allclose(P.T @ P, np.eye(a), atol=1e-12)                                                  # P'P = I
    assert np.allclose(T.T @ (D[:, None] * T), np.diag(sv[:a] ** 2), atol=1e-11 * e1)                   # T'DT = diag(sv^2)
    assert np.allclose(T, Xs @ P, atol=1e-11 * np.abs(T).max())                                         # T = Xc P
    assert np.allclose(np_pca_transform(fm, X), T, atol=1e-11 * np.abs(T).max())                        # transform(Xtrain) == T
    # the eigen route (src/pcaeigen.jl): eigh of Xs'D Xs gives sv^2 and, up to sign, P
    G = Xs.T @ (D[:, None] * Xs)
    lam, V = np.linalg.eigh(G)
    lam, V = lam[::-1], V[:, ::-1]
    assert np.allclose(np.maximum(lam[:a], 0), sv[:a] ** 2, atol=1e-11 * e1)
    for i in range(a):
        if sv[i] ** 2 > 1e-8 * e1:
            s = np.sign(V[:, i] @ P[:, i])
            assert np.linalg.norm(s * V[:, i] - P[:, i]) < 1e-6
    assert np.isclose(np.trace(G), np.sum(sv ** 2), rtol=1e-11)                                         # sstot = trace(G)
    if scal:
        assert np.allclose(np.diag(G), 1.0, rtol=1e-12)
        Gu = ((X - fm["xmeans"]).T * D) @ (X - fm["xmeans"])                                            # scal costs nothing extra:
        assert np.allclose(fm["xscales"], np.sqrt(np.diag(Gu)), rtol=1e-12)                             # xscales = sqrt(diag G)
        assert np.allclose(G, Gu / np.outer(fm["xscales"], fm["xscales"]), atol=1e-12)                  # G_scaled = G ./ (s s')


@pytest.mark.parametrize("n,p,nlv,wkind,scal", [(80, 9, 4, "ones", False), (80, 9, 9, "rand", True), (50, 12, 6, "zeros", True)])
def test_summary_identities_need_no_pass_over_x(n, p, nlv, wkind, scal):
    """What pca_summary computes from the stored quantities against the reference's summary, which reads X: 1e-12 relative."""
    X = _data(n, p, 7 * n + p)
    fm = np_pcasvd(X, _weights(wkind, n), nlv=nlv, scal=scal)
    ref = np_pca_summary(fm, X)
    a = fm["P"].shape[1]
    sv, P, D, T, Xs = fm["sv"][:a], fm["P"], fm["weights"], fm["T"], fm["Xs"]
    colvar = D @ (X - fm["xmeans"]) ** 2
    G = Xs.T @ (D[:, None] * Xs)
    rel = lambda A, B: np.max(np.abs(A - B)) / np.max(np.abs(B))   # noqa: E731
    assert rel(np.array([np.trace(G)]), np.array([np.sum(ref["explvarx"]["var"] / ref["explvarx"]["pvar"]) / a])) < 1e-12   # sstot = trace(G)
    assert rel(sv ** 2, ref["explvarx"]["var"]) < 1e-12                                                                       # tt = sv^2
    coord_var = P * sv
    assert rel(coord_var, ref["coord_var"]) < 1e-12                                                                           # Xs'D T / sqrt(tt) = P sv
    assert rel(coord_var / (np.sqrt(colvar) / fm["xscales"])[:, None], ref["cor_circle"]) < 1e-12
    cc = coord_var ** 2
    assert rel(cc / cc.sum(axis=0), ref["contr_var"]) < 1e-12
    assert rel(D[:, None] * T ** 2 / sv ** 2, ref["contr_ind"]) < 1e-12


@pytest.mark.parametrize("q,wkind,scal", [(1, "ones", False), (3, "rand", True), (2, "zeros", False)])
def test_pcr_restatement_is_the_eigen_route_plus_one_pass(q, wkind, scal):
    n, p, nlv = 70, 11, 6
    X = _data(n, p, 3)
    rng = np.random.default_rng(9)
    Y = X[:, :q] * 0.5 + X[:, 3:3 + q] + 0.01 * rng.standard_normal((n, q))
    fm = np_pcr(X, Y, _weights(wkind, n), nlv=nlv, scal=scal)
    pca = fm["fm_pca"]
    D, Xs = pca["weights"], pca["Xs"]
    K = Xs.T @ (D[:, None] * (Y - fm["ymeans"]))                       # the one pass: Xs'D Yc
    beta = (pca["P"].T @ K) / (pca["sv"][:nlv] ** 2)[:, None]          # diag(1 / sv^2) P' Xs'D Yc
    assert np.allclose(beta, fm["C"].T, rtol=1e-9, atol=1e-12 * np.abs(fm["C"]).max())
    B0, i0 = np_pcr_coef(fm, 0)
    assert np.all(B0 == 0) and np.allclose(i0, fm["ymeans"])           # nlv = 0: intercept only
    assert np.allclose(np_pcr_predict(fm, X), fm["ymeans"] + fm["T"] @ fm["C"].T, atol=1e-9 * np.abs(Y).max())


@pytest.mark.parametrize("n,p,wkind", [(1, 1, "ones"), (33, 1, "rand"), (70, 9, "zeros"), (257, 5, "rand")])
def test_gram_bound_holds_for_a_float64_run_in_the_kernel_order(n, p, wkind):
    X = _data(n, p, n + 11 * p)
    w = _weights(wkind, n)
    Gl, mul = gram_longdouble(X, w)
    bG, bmu = gram_bound(X, w)
    G, mu = _gram_float64_like_the_kernel(X, w)
    assert np.all(np.abs(mu - np.asarray(mul, dtype=np.float64)) <= bmu + 0.0)
    err = np.abs(np.asarray(G - Gl, dtype=np.float64))
    assert np.all(err <= bG), float(np.max(err / bG))
    if n > 1:   # the bound is not vacuous: X'DX - mu mu' in float64, the shortcut the kernel must not take, misses it by far at level 100
        d = _mweight(w, n)
        short = (X.T * d) @ X - np.outer(mu, mu)
        assert np.max(np.abs(np.asarray(short - Gl, dtype=np.float64)) / bG) > np.max(err / bG)


# ---------------------------------------------------------------------------------- tests: the surface
def test_header_declares_the_entries():
    protos = header_protos()
    assert protos["jch_xtdx"][0] == "int32_t" and len(protos["jch_xtdx"][1]) == 12
    assert protos["jch_pca_fit"][0] == "int32_t" and len(protos["jch_pca_fit"][1]) == 29
    h = open(os.path.join(ROOT, "include", "jchemo_hip.h")).read()
    assert re.search(r"#define\s+JCH_VERSION\s+108\b", h)
    mk = open(os.path.join(ROOT, "jchemo.jl_amd", "csrc", "Makefile")).read()
    assert "xtdx.hip" in re.search(r"SRCS := (.*)", mk).group(1).split()


def test_python_package_exports_and_fields():
    import jchemo_hip as J
    for name in ("pcasvd", "pcasvd_", "pcaeigen", "pcaeigen_", "pcaeigenk", "pcaeigenk_", "pcr", "pcr_", "Pca", "Pcr", "pca_transform", "pca_summary"):
        assert hasattr(J, name), name
    for s in ("jch_xtdx", "jch_pca_fit"):
        assert s in J.SYMBOLS
    assert [f.name for f in dataclasses.fields(J.Pca)] == PCA_FIELDS   # src/pcasvd.jl:100, then the eigen route's report
    assert [f.name for f in dataclasses.fields(J.Pcr)] == PCR_FIELDS   # src/pcr.jl:96
    import inspect
    for fn in (J.pcasvd, J.pcasvd_, J.pcaeigen, J.pcaeigen_, J.pcaeigenk, J.pcaeigenk_):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["X", "weights", "nlv", "scal", "eig_tol", "eig_maxit", "ctx"]
        assert sig.parameters["eig_tol"].default == 1e-10 and sig.parameters["eig_maxit"].default == 300
    assert list(inspect.signature(J.pcr).parameters)[:3] == ["X", "Y", "weights"]


def test_python_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    X = np.zeros((4, 2), order="F")
    for bad in (dict(nlv=0), dict(nlv=-1), dict(nlv=1, eig_maxit=0), dict(nlv=1, eig_tol=0.0), dict(nlv=1, eig_tol=-1e-9)):
        with pytest.raises(ValueError):
            J.pcasvd(X, **bad)
        with pytest.raises(ValueError):
            J.pcr(X, np.zeros((4, 1)), **bad)
    with pytest.raises(ValueError):
        J.pcasvd(X, np.ones(3), nlv=1)
    with pytest.raises(ValueError):
        J.pcr(X, np.zeros((3, 1)), nlv=1)


def test_pca_without_a_gpu_raises_enodev():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import jchemo_hip as J
    from jchemo_hip._lib import JCH_ENODEV, JchError
    with pytest.raises(JchError) as e:
        J.pcasvd(_data(10, 3, 1), nlv=2)
    assert e.value.code == JCH_ENODEV


def test_julia_module_exports_and_records():
    src = open(JL).read()
    m = re.search(r"\nexport (.*?)\n\n", src, flags=re.S)
    names = {s.strip() for s in m.group(1).replace("\n", " ").split(",")}
    for name in ("Pca", "Pcr", "pcasvd", "pcasvd!", "pcaeigen", "pcaeigen!", "pcaeigenk", "pcaeigenk!", "pcr", "pcr!"):
        assert name in names, name
    for rec, want in (("Pca", PCA_FIELDS), ("Pcr", PCR_FIELDS)):
        body = re.search(r"struct " + rec + r"[^\n]*\n(.*?)\nend", src, flags=re.S).group(1)
        fields = [re.match(r"\s*(\w+)", ln).group(1) for ln in body.splitlines() if re.match(r"\s*\w+", ln)]
        assert fields == want
    assert re.search(r"function transform\(object::Pca, X; nlv = nothing", src)
    assert re.search(r"function Base\.summary\(object::Pca, X\)", src)
    assert ":jch_pca_fit" in src and ":jch_xtdx" in src
