"""Static checks of the kernel PCA surface (kpca): header, Python package, Julia wrapper, and the literal numpy restatement of
src/kpca.jl:82-147 the GPU tests compare against.  No GPU needed."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_julia_wrapper import JL, header_protos  # noqa: E402
from test_kplsr_static import _colstd, _jl_function_kwargs, np_kern  # noqa: E402

KPCA_FIELDS = ["X", "Kt", "T", "P", "sv", "eig", "D", "DKt", "vtot", "xscales", "weights", "kern", "dots",
               "sstot", "niter", "resid", "converged"]


# ---------------------------------------------------------------------------------- numpy restatement of src/kpca.jl
def np_kpca(X, weights=None, *, nlv, kern="krbf", scal=False, **kw):
    """src/kpca.jl:82-115 line by line (svd of the whole Kd).  Returns a dict with the reference's fields plus U and Kc."""
    X = np.array(X, dtype=np.float64, order="F")
    n, p = X.shape
    nlv = min(nlv, n)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    w = w / w.sum()                                                      # mweight
    xscales = np.ones(p)
    if scal:
        xscales = _colstd(X, w)
        X = X / xscales
    K = np_kern(kern, X, X, **kw)
    DKt = w[:, None] * K.T
    vtot = DKt.sum(axis=0)
    Kc = K - vtot[:, None] - vtot[None, :] + (w[:, None] * DKt.T).sum()
    sqrtw = np.sqrt(w)
    Kd = sqrtw[:, None] * Kc * sqrtw[None, :]
    _, S, Vt = np.linalg.svd(Kd)
    U = Vt.T[:, :nlv]
    eig = S.copy()
    eig[eig < 0] = 0
    sv = np.sqrt(eig)
    P = sqrtw[:, None] * (U / sv[:nlv])
    T = Kc @ P
    return dict(X=X, T=T, P=P, U=U, sv=sv, eig=eig, D=w, vtot=vtot, xscales=xscales, weights=w, kern=kern, dots=kw, Kc=Kc, Kd=Kd)


def np_kpca_transform(fm, Xnew, nlv=None):
    """src/kpca.jl:123-132."""
    a = fm["T"].shape[1]
    nlv = a if nlv is None else min(nlv, a)
    K = np_kern(fm["kern"], np.asarray(Xnew, dtype=np.float64) / fm["xscales"], fm["X"], **fm["dots"])
    DKt = fm["D"][:, None] * K.T
    vnew = DKt.sum(axis=0)
    Kc = K - vnew[:, None] - fm["vtot"][None, :] + fm["D"] @ fm["vtot"]
    return Kc @ fm["P"][:, :nlv]


def np_kpca_summary(fm):
    """src/kpca.jl:138-147."""
    tt = (fm["D"][:, None] * fm["T"] ** 2).sum(axis=0)
    pvar = tt / fm["eig"].sum()
    return dict(lv=np.arange(1, tt.shape[0] + 1), var=tt, pvar=pvar, cumpvar=np.cumsum(pvar))


def _data(n, p, seed):
    rng = np.random.default_rng(seed)
    H = rng.random((n, 3))
    grid = np.linspace(0, 1, p)
    B = np.exp(-((grid[None, :] - np.array([0.2, 0.5, 0.8])[:, None]) / 0.15) ** 2)
    return np.asfortranarray(H @ B + 0.05 * rng.standard_normal((n, p)))


# ---------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("kern,kw,scal,wkind", [("krbf", dict(gamma=0.5), False, "ones"), ("krbf", dict(gamma=0.2), True, "rand"),
                                                 ("kpol", dict(degree=2, gamma=0.5, coef0=1.0), False, "zeros")])
def test_restatement_identities(kern, kw, scal, wkind):
    n, p, nlv = 60, 7, 5
    X = _data(n, p, 3)
    w = {"ones": None, "rand": np.random.default_rng(4).random(n) + 0.1, "zeros": np.r_[np.zeros(5), np.ones(n - 5)]}[wkind]
    fm = np_kpca(X, w, nlv=nlv, kern=kern, scal=scal, **kw)
    T, D = fm["T"], fm["D"]
    assert np.allclose(T.T @ (D[:, None] * T), np.diag(fm["eig"][:nlv]), atol=1e-10 * fm["eig"][0])     # T'DT = diag(eig)
    assert np.allclose(np_kpca_transform(fm, X), T, atol=1e-10 * np.abs(T).max())                       # transform(Xtrain) == T
    assert np.allclose(fm["Kd"] @ fm["U"], fm["U"] * fm["eig"][:nlv], atol=1e-10 * fm["eig"][0])        # PSD: Kd u = eig u
    assert np.isclose(fm["eig"].sum(), np.trace(fm["Kd"]), rtol=1e-10)                                 # sstot = trace for PSD
    sm = np_kpca_summary(fm)
    assert np.allclose(sm["var"], fm["eig"][:nlv], rtol=1e-9)
    if wkind == "zeros":
        assert np.all(np.abs(T[:5]).sum(axis=1) > 0)   # zero-weight rows still get scores


def test_header_declares_the_entries():
    protos = header_protos()
    assert protos["jch_kpca_fit"][0] == "int32_t"
    assert len(protos["jch_kpca_fit"][1]) == 27
    assert len(protos["jch_kc_panel"][1]) == 8
    h = open(os.path.join(ROOT, "include", "jchemo_hip.h")).read()
    assert re.search(r"#define\s+JCH_VERSION\s+108\b", h)


def test_python_package_exports_and_fields():
    import dataclasses
    import jchemo_hip as J
    for name in ("kpca", "kpca_transform", "kpca_summary", "Kpca"):
        assert hasattr(J, name), name
    for s in ("jch_kpca_fit", "jch_kc_panel"):
        assert s in J.SYMBOLS
    assert [f.name for f in dataclasses.fields(J.Kpca)] == KPCA_FIELDS   # src/kpca.jl:1-15, then the solver's report


def test_python_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    X = np.zeros((4, 2), order="F")
    for bad in (dict(nlv=1, kern="ksig"), dict(nlv=1, kern="krbf", degree=2), dict(nlv=0), dict(nlv=1, eig_maxit=0),
                dict(nlv=1, eig_tol=0.0), dict(nlv=1, eig_tol=-1e-9)):
        with pytest.raises(ValueError):
            J.kpca(X, **bad)
    with pytest.raises(ValueError):
        J.kpca(X, np.ones(3), nlv=1)


def test_kpca_without_a_gpu_raises_enodev():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import jchemo_hip as J
    from jchemo_hip._lib import JCH_ENODEV, JchError
    with pytest.raises(JchError) as e:
        J.kpca(_data(10, 3, 1), nlv=2)
    assert e.value.code == JCH_ENODEV


def test_julia_module_exports_and_reference_keywords():
    src = open(JL).read()
    m = re.search(r"\nexport (.*?)\n\n", src, flags=re.S)
    names = {s.strip() for s in m.group(1).replace("\n", " ").split(",")}
    for name in ("kpca", "Kpca"):
        assert name in names, name
    body = re.search(r"struct Kpca[^\n]*\n(.*?)\nend", src, flags=re.S).group(1)
    fields = [re.match(r"\s*(\w+)", ln).group(1) for ln in body.splitlines() if re.match(r"\s*\w+", ln)]
    assert fields == KPCA_FIELDS
    assert ["nlv", "kern", "scal", "ctx", "eig_tol", "eig_maxit", "kwargs..."] in _jl_function_kwargs(src, "kpca")
    assert re.search(r"function transform\(object::Kpca, X; nlv = nothing", src)
    assert re.search(r"function Base\.summary\(object::Kpca", src)
