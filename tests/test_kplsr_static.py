"""Static checks of the kernel NIPALS PLS surface (kplsr): header, Python package, Julia wrapper, and the two numpy restatements of
src/kplsr.jl the GPU tests compare against (the literal one with the dense z*K*z' deflation, and the rank-two one for large n).
No GPU needed."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_julia_wrapper import JL, _balanced, _split_top, header_protos  # noqa: E402

NEW_ENTRIES = ("jch_kplsr_fit", "jch_kplsr_transform", "jch_kplsr_predict")
KPLSR_FIELDS = ["X", "Kt", "T", "C", "U", "R", "D", "DKt", "vtot", "xscales", "ymeans", "yscales", "weights", "kern", "dots", "iter"]


# ---------------------------------------------------------------------------------- numpy restatements of src/kplsr.jl
def np_sqdist(Z, X):
    out = np.empty((Z.shape[0], X.shape[0]))
    step = max(1, int(2e7 // max(1, X.shape[0] * X.shape[1])))
    for i in range(0, Z.shape[0], step):
        D = Z[i:i + step, None, :] - X[None, :, :]
        out[i:i + step] = np.einsum("ijk,ijk->ij", D, D)
    return out


def np_kern(kern, Z, X, gamma=1.0, coef0=0.0, degree=1):
    """src/kernels.jl:26-30 (krbf), :59-70 (kpol)."""
    if kern == "krbf":
        return np.exp(-gamma * np_sqdist(Z, X))
    K = gamma * Z @ X.T + coef0
    zK = K.copy()
    for _ in range(degree - 1):
        K = K * zK
    return K


def _colstd(A, w):
    mu = w @ A
    return np.sqrt(w @ (A - mu) ** 2)


def np_kplsr(X, Y, weights=None, *, nlv, kern="krbf", tol=1.5e-8, maxit=100, scal=False, rank2=False, **kw):
    """src/kplsr.jl:119-193 line by line.  rank2=False: the literal `z = I - t*dt'; K .= z*K*z'` (n <= 600); rank2=True: the same
    deflation as K - t a' - a t' + (dt'a) t t' with a = K dt (O(n^2) per LV)."""
    X = np.array(X, dtype=np.float64, order="F")
    Y = np.array(Y, dtype=np.float64, order="F").reshape(X.shape[0], -1)
    n, p = X.shape
    q = Y.shape[1]
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    w = w / w.sum()                                                      # mweight
    ymeans = w @ Y
    xscales, yscales = np.ones(p), np.ones(q)
    if scal:
        xscales, yscales = _colstd(X, w), _colstd(Y, w)
        X /= xscales
        Y = (Y - ymeans) / yscales
    else:
        Y = Y - ymeans
    K = np_kern(kern, X, X, **kw)
    vtot = (w[:, None] * K.T).sum(axis=0)                                # sum(D * Kt, dims = 1)
    s = (w[:, None] * (K * w[None, :])).sum()                            # sum(D * DKt')
    Kc = K - vtot[:, None] - vtot[None, :] + s
    Ka = Kc.copy()
    T = np.zeros((n, nlv)); U = np.zeros((n, nlv)); C = np.zeros((q, nlv)); it = np.zeros(nlv, dtype=np.int64)
    for a in range(nlv):
        if q == 1:
            t = Ka @ (w * Y[:, 0])
            t /= np.sqrt(t @ (w * t))
            dt = w * t
            c = Y.T @ dt
            u = Y @ c
            u /= np.sqrt(u @ u)
        else:
            u = Y[:, 0].copy()
            ztol, ziter = 1.0, 1
            while ztol > tol and ziter <= maxit:
                t = Ka @ (w * u)
                t /= np.sqrt(t @ (w * t))
                dt = w * t
                c = Y.T @ dt
                zu = Y @ c
                zu /= np.sqrt(zu @ zu)
                ztol = np.sqrt(np.sum((u - zu) ** 2))
                u = zu
                ziter += 1
            it[a] = ziter - 1
        if rank2:
            av = Ka @ dt
            Ka = Ka - np.outer(t, av) - np.outer(av, t) + (dt @ av) * np.outer(t, t)
        else:
            z = np.eye(n) - np.outer(t, dt)
            Ka = z @ Ka @ z.T
        Y = Y - np.outer(t, c)
        T[:, a] = t; C[:, a] = c; U[:, a] = u
    DU = w[:, None] * U
    R = DU @ np.linalg.inv(T.T @ (w[:, None] * (Kc @ DU)))
    return dict(X=X, K=K, T=T, C=C, U=U, R=R, vtot=vtot.reshape(1, -1), xscales=xscales, ymeans=ymeans, yscales=yscales, weights=w,
                iter=it, Y=Y, kern=kern, dots=kw)


def np_kplsr_transform(fm, Xnew, nlv=None):
    """src/kplsr.jl:202-212."""
    a = fm["T"].shape[1]
    nlv = a if nlv is None else min(nlv, a)
    K = np_kern(fm["kern"], np.asarray(Xnew, dtype=np.float64) / fm["xscales"], fm["X"], **fm["dots"])
    w = fm["weights"]
    vnew = K @ w
    Kc = K - vnew[:, None] - fm["vtot"] + w @ fm["vtot"].ravel()
    return Kc @ fm["R"][:, :nlv]


def np_kplsr_predict(fm, Xnew, nlv=None):
    """src/kplsr.jl:238-250 (one nlv: matrix; a collection: list over the contiguous range)."""
    a = fm["T"].shape[1]
    rng = [a] if nlv is None else list(range(max(0, min(np.atleast_1d(nlv))), min(a, max(np.atleast_1d(nlv))) + 1))
    T = np_kplsr_transform(fm, Xnew)
    pred = [fm["ymeans"][None, :] + T[:, :k] @ fm["C"][:, :k].T * fm["yscales"][None, :] for k in rng]
    return pred[0] if len(pred) == 1 else pred


def rel_fro(A, B):
    A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    return float(np.linalg.norm(A - B) / max(np.linalg.norm(A), 1e-300))


# ---------------------------------------------------------------------------------- tests
def test_header_declares_the_entries():
    protos = header_protos()
    for name in NEW_ENTRIES:
        assert name in protos, name
        assert protos[name][0] == "int32_t"
    assert len(protos["jch_kplsr_fit"][1]) == 25
    assert len(protos["jch_kplsr_transform"][1]) == 20
    assert len(protos["jch_kplsr_predict"][1]) == 25
    h = open(os.path.join(ROOT, "include", "jchemo_hip.h")).read()
    assert re.search(r"#define\s+JCH_VERSION\s+108\b", h)


def test_python_package_exports_and_fields():
    import dataclasses
    import jchemo_hip as J
    for name in ("kplsr", "kplsr_", "Kplsr"):
        assert hasattr(J, name), name
    for s in NEW_ENTRIES:
        assert s in J.SYMBOLS
    assert [f.name for f in dataclasses.fields(J.Kplsr)] == KPLSR_FIELDS   # src/kplsr.jl:1-18


def test_python_arguments_are_checked_before_any_device_work():
    import jchemo_hip as J
    X = np.zeros((4, 2), order="F"); Y = np.zeros((4, 1), order="F")
    with pytest.raises(ValueError):
        J.kplsr(X, Y, nlv=1, kern="ksig")
    with pytest.raises(ValueError):
        J.kplsr(X, Y, nlv=1, kern="krbf", degree=2)
    with pytest.raises(ValueError):
        J.kplsr(X, Y, nlv=0)
    with pytest.raises(ValueError):
        J.kplsr(X, Y, nlv=1, maxit=0)
    with pytest.raises(ValueError):
        J.kplsr(X, np.zeros((3, 1)), nlv=1)


def _jl_function_kwargs(src, name):
    out = []
    for m in re.finditer(r"(?:^|\n)\s*(?:function\s+)?" + re.escape(name) + r"\(", src):
        end = _balanced(src, m.end() - 1)
        sig = src[m.end():end - 1]
        if ";" not in sig:
            continue
        kw = sig.split(";", 1)[1]
        out.append([a.split("=")[0].strip() for a in _split_top(kw)])
    return out


def test_julia_module_exports_and_reference_keywords():
    src = open(JL).read()
    m = re.search(r"\nexport (.*?)\n\n", src, flags=re.S)
    names = {s.strip() for s in m.group(1).replace("\n", " ").split(",")}
    for name in ("kplsr", "kplsr!", "Kplsr"):
        assert name in names, name
    body = re.search(r"struct Kplsr[^\n]*\n(.*?)\nend", src, flags=re.S).group(1)
    fields = [re.match(r"\s*(\w+)", ln).group(1) for ln in body.splitlines() if re.match(r"\s*\w+", ln)]
    assert fields == KPLSR_FIELDS
    want = ["nlv", "kern", "tol", "maxit", "scal", "ctx", "kwargs..."]
    for name in ("kplsr", "kplsr!"):
        found = _jl_function_kwargs(src, name)
        assert want in found, f"{name}: {found}"


@pytest.mark.parametrize("q,kern,kw,scal", [(1, "krbf", dict(gamma=0.3), False), (3, "krbf", dict(gamma=0.3), True),
                                            (3, "kpol", dict(degree=2, gamma=0.5, coef0=1.0), False)])
def test_rank_two_restatement_matches_the_literal_one(q, kern, kw, scal):
    rng = np.random.default_rng(7 + q)
    n, p = 80, 6
    X = rng.random((n, p)); Y = rng.random((n, q)); w = rng.random(n)
    a = np_kplsr(X, Y, w, nlv=6, kern=kern, scal=scal, **kw)
    b = np_kplsr(X, Y, w, nlv=6, kern=kern, scal=scal, rank2=True, **kw)
    for f in ("T", "U", "C", "R"):
        assert rel_fro(a[f], b[f]) < 1e-9, f
    assert np.array_equal(a["iter"], b["iter"])
    # the scores are D-orthonormal (T'DT = I), which the device's product-form projection relies on only through Z_a
    TT = a["T"].T @ (a["weights"][:, None] * a["T"])
    assert np.abs(TT - np.eye(6)).max() < 1e-8
