"""Static checks of the kernel ridge regression surface (krr, krrda, gridscorelb): header, Python package, Julia wrapper, the
literal numpy restatement of src/krr.jl:128-202 the GPU tests compare against, and the identities the Cholesky design rests on
(DESIGN.md §13), checked on the restatement alone.  No GPU needed."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_julia_wrapper import JL, header_protos  # noqa: E402
from test_kpca_static import _data  # noqa: E402
from test_kplsr_static import _colstd, _jl_function_kwargs, np_kern  # noqa: E402

KRR_FIELDS = ["X", "Kd", "B", "vtot", "lb", "xscales", "ymeans", "weights", "kern", "dots"]
NEW_ENTRIES = {"jch_krr_fit": 22, "jch_krr_solve": 13, "jch_chol_factor": 5, "jch_chol_solve": 7, "jch_chol_inv_fro2": 5}


# ---------------------------------------------------------------------------------- numpy restatement of src/krr.jl
def np_krr(X, Y, weights=None, *, lb, kern="krbf", scal=False, svd=True, **kw):
    """src/krr.jl:128-159 line by line (svd of the whole Kd; svd=False stops in front of it: Kd, sqrtD Y and the rest only).
    Returns a dict with the reference's fields plus Kc and Kd."""
    X = np.array(X, dtype=np.float64, order="F")
    Y = np.array(Y, dtype=np.float64, order="F").reshape(X.shape[0], -1)
    n, p = X.shape
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    w = w / w.sum()                                                      # mweight (:135)
    xscales = np.ones(p)
    if scal:
        xscales = _colstd(X, w)
        X = X / xscales
    ymeans = w @ Y
    K = np_kern(kern, X, X, **kw)
    DKt = w[:, None] * K.T
    vtot = DKt.sum(axis=0)
    Kc = K - vtot[:, None] - vtot[None, :] + (w[:, None] * DKt.T).sum()
    sqrtw = np.sqrt(w)
    Kd = sqrtw[:, None] * Kc * sqrtw[None, :]
    fm = dict(X=X, K=K, D=w, sqrtD=sqrtw, vtot=vtot, lb=lb, xscales=xscales, ymeans=ymeans, weights=w, kern=kern, dots=kw, Kc=Kc, Kd=Kd,
              DY=sqrtw[:, None] * Y)
    if svd:
        _, S, Vt = np.linalg.svd(Kd)
        U = Vt.T                                                         # res.V (:153)
        fm.update(U=U, sv=np.sqrt(S), UtDY=U.T @ fm["DY"])
    return fm


def np_krr_coef(fm, lb=None):
    """src/krr.jl:168-177."""
    lb = fm["lb"] if lb is None else lb
    eig = fm["sv"] ** 2
    z = 1.0 / (eig + lb ** 2)
    A = fm["U"] @ (z[:, None] * fm["UtDY"])
    return dict(A=A, int=fm["ymeans"].reshape(1, -1), df=1.0 + np.sum(eig * z))


def np_krr_centred_new(fm, Xnew):
    """The Kc of src/krr.jl:190-193 for new rows."""
    K = np_kern(fm["kern"], np.asarray(Xnew, dtype=np.float64) / fm["xscales"], fm["X"], **fm["dots"])
    DKt = fm["D"][:, None] * K.T
    vnew = DKt.sum(axis=0)
    return K - vnew[:, None] - fm["vtot"][None, :] + fm["D"] @ fm["vtot"]


def np_krr_predict(fm, Xnew, lb=None):
    """src/krr.jl:187-202 (one lb: matrix; a collection: list)."""
    lbs = [fm["lb"]] if lb is None else list(np.atleast_1d(lb))
    Kc = np_krr_centred_new(fm, Xnew)
    pred = []
    for v in lbs:
        z = np_krr_coef(fm, v)
        pred.append(z["int"] + Kc @ (fm["sqrtD"][:, None] * z["A"]))
    return pred[0] if len(pred) == 1 else pred


def chol_route(fm, lb, Xnew=None):
    """The same quantities by the route the library takes: scipy Cholesky of Kd + lb^2 I."""
    from scipy.linalg import cho_factor, cho_solve, solve_triangular
    n = fm["Kd"].shape[0]
    M = fm["Kd"] + lb ** 2 * np.eye(n)
    c = cho_factor(M, lower=True)
    A = cho_solve(c, fm["DY"])
    Linv = solve_triangular(np.tril(c[0]), np.eye(n), lower=True)
    out = dict(A=A, df=1.0 + n - lb ** 2 * np.sum(Linv ** 2))
    if Xnew is not None:
        out["pred"] = fm["ymeans"][None, :] + np_krr_centred_new(fm, Xnew) @ (fm["sqrtD"][:, None] * A)
    return out


# ---------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("kern,kw,scal,wkind", [("krbf", dict(gamma=0.5), False, "ones"), ("krbf", dict(gamma=0.2), True, "rand"),
                                                 ("kpol", dict(degree=2, gamma=0.5, coef0=1.0), False, "zeros")])
@pytest.mark.parametrize("lb", [1e-1, 1e-3])
def test_the_cholesky_route_reproduces_the_svd_route(kern, kw, scal, wkind, lb):
    n, p, q = 300, 7, 3
    X = _data(n, p, 3)
    Y = np.random.default_rng(8).standard_normal((n, q)) + X[:, :q]
    w = {"ones": None, "rand": np.random.default_rng(4).random(n) + 0.1, "zeros": np.r_[np.zeros(5), np.ones(n - 5)]}[wkind]
    fm = np_krr(X, Y, w, lb=lb, kern=kern, scal=scal, **kw)
    eig = fm["sv"] ** 2
    cond = (eig.max() + lb ** 2) / (eig.min() + lb ** 2)
    eps = np.finfo(np.float64).eps
    Xn = _data(40, p, 5)
    a, b = np_krr_coef(fm), chol_route(fm, lb, Xn)
    bound = 50 * eps * cond
    assert np.linalg.norm(a["A"] - b["A"]) <= bound * np.linalg.norm(a["A"])                      # A = (Kd + lb^2 I)^-1 sqrtD Y
    pr = np_krr_predict(fm, Xn)
    assert np.linalg.norm(pr - b["pred"]) <= bound * np.linalg.norm(pr - fm["ymeans"])
    assert abs(a["df"] - b["df"]) <= 10 * n * eps * cond                                         # df = 1 + n - lb^2 |L^-1|_F^2
    # predict(Xtrain) = ymeans + Kc sqrtD A (the Gram is recomputed: its eps-sized differences meet an A that is up to cond larger than the product)
    fit = fm["ymeans"][None, :] + fm["Kc"] @ (fm["sqrtD"][:, None] * a["A"])
    assert np.linalg.norm(np_krr_predict(fm, fm["X"] * fm["xscales"]) - fit) <= bound * np.linalg.norm(fit)
    if wkind == "zeros":   # zero-weight rows: A rows of 0, predictions all the same
        assert np.abs(b["A"][:5]).max() == 0.0 and np.abs(a["A"][:5]).max() <= 1e-9 * np.abs(a["A"]).max()
        assert np.all(np.abs(fit[:5] - fm["ymeans"]).sum(axis=1) > 0)


def test_header_declares_the_entries():
    protos = header_protos()
    for name, nargs in NEW_ENTRIES.items():
        assert name in protos, name
        assert protos[name][0] == "int32_t"
        assert len(protos[name][1]) == nargs, name
    h = open(os.path.join(ROOT, "include", "jchemo_hip.h")).read()
    assert re.search(r"#define\s+JCH_VERSION\s+108\b", h)


def test_python_package_exports_and_fields():
    import dataclasses
    import jchemo_hip as J
    for name in ("krr", "krr_", "krr_coef", "krr_predict", "Krr", "gridscorelb", "krrda", "krrda_predict"):
        assert hasattr(J, name), name
    for s in NEW_ENTRIES:
        assert s in J.SYMBOLS
    names = [f.name for f in dataclasses.fields(J.Krr)]
    assert names[:len(KRR_FIELDS)] == KRR_FIELDS and names[len(KRR_FIELDS):] == ["solved"]      # no U, UtDY, sv: no SVD is taken
    assert not {"U", "UtDY", "sv"} & set(names)


def test_python_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    X = np.zeros((4, 2), order="F"); Y = np.zeros((4, 1), order="F")
    for bad in (dict(lb=0.0), dict(lb=-1e-3), dict(lb=float("nan")), dict(lb=float("inf")), dict(lb=1.0, kern="ksig"),
                dict(lb=1.0, kern="krbf", degree=2)):
        for fun in (J.krr, J.krr_):
            with pytest.raises(ValueError):
                fun(X, Y, **bad)
        with pytest.raises(ValueError):
            J.krrda(X, np.array([0, 1, 0, 1]), **bad)
    with pytest.raises(ValueError):
        J.krr(X, Y, np.ones(3), lb=1.0)
    with pytest.raises(ValueError):
        J.krr(X, np.zeros((3, 1)), lb=1.0)
    with pytest.raises(ValueError, match="must not contain `lb`"):
        J.gridscorelb(X, Y, X, Y, score=J.rmsep, fun=J.krr, lb=[1.0, 0.1], pars=dict(lb=[1.0], gamma=[1.0]))
    with pytest.raises(ValueError):
        J.gridscorelb(X, Y, X, Y, score=J.rmsep, fun=J.krr, lb=[1.0, 0.0])
    fm = J.Krr(X, None, Y, None, 1.0, np.ones(2), np.zeros(1), np.ones(4) / 4, "krbf", {})
    for bad in (0.0, -1.0, float("nan"), [0.1, 0.0]):
        with pytest.raises(ValueError):
            J.krr_predict(fm, X, lb=bad)
    with pytest.raises(ValueError):
        J.krr_coef(fm, lb=0.0)


def test_krr_without_a_gpu_raises_enodev():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import jchemo_hip as J
    from jchemo_hip._lib import JCH_ENODEV, JchError
    with pytest.raises(JchError) as e:
        J.krr(_data(10, 3, 1), np.ones((10, 1)), lb=0.1)
    assert e.value.code == JCH_ENODEV


def test_julia_module_exports_and_reference_keywords():
    src = open(JL).read()
    m = re.search(r"\nexport (.*?)\n\n", src, flags=re.S)
    names = {s.strip() for s in m.group(1).replace("\n", " ").split(",")}
    for name in ("krr", "krr!", "Krr", "gridscorelb", "krrda"):
        assert name in names, name
    body = re.search(r"struct Krr[^\n]*\n(.*?)\nend", src, flags=re.S).group(1)
    fields = [re.match(r"\s*(\w+)", ln).group(1) for ln in body.splitlines() if re.match(r"\s*\w+", ln)]
    assert fields[:len(KRR_FIELDS)] == KRR_FIELDS and not {"U", "UtDY", "sv"} & set(fields)
    want = ["lb", "kern", "scal", "ctx", "kwargs..."]                                     # src/krr.jl:122-123, 128-129 (+ ctx)
    for name in ("krr", "krr!", "krrda"):                                                  # src/krrda.jl:59-60
        found = _jl_function_kwargs(src, name)
        assert want in found, f"{name}: {found}"
    assert ["score", "fun", "lb", "pars", "verbose", "ctx"] in _jl_function_kwargs(src, "gridscorelb")   # src/gridscore.jl:235-236
    assert re.search(r"function coef\(object::Krr; lb = nothing", src)                    # src/krr.jl:168
    assert re.search(r"function predict\(object::Krr, X; lb = nothing", src)              # src/krr.jl:187
    assert re.search(r"function predict\(object::Krrda, X; lb = nothing", src)            # src/rrda.jl:79
