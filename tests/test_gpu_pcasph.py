"""pcasph on the GPU against the literal numpy restatement of src/pcasph.jl (tests/test_medspa_static.py), under the bounds derived there; what
the returned `Pca` feeds (transform, summary, occsd / occod / occsdod); and the behaviour the model exists for."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_accessors_static import bound_affine, ref_affine  # noqa: E402
from test_medspa_static import BEHAVIOUR, PCA_CASES, angle_deg, gen_pca, pca_bounds, pca_ref, symmetric_design  # noqa: E402


@pytest.fixture(scope="module")
def J():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import jchemo_hip
    return jchemo_hip


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _dev(X):
    return torch.as_tensor(np.array(X), device="cuda:0").t().contiguous().t()   # column-major on the device


@pytest.mark.parametrize("case", PCA_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_pcasph_parity_with_the_restatement(J, case):
    n, p, nlv, scal, typc, wk = case
    X, w, rf = pca_ref(case)
    b = pca_bounds(case)
    X0 = X.copy()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fm = J.pcasph(X, w, nlv=nlv, typc=typc, scal=scal)
    assert np.array_equal(X, X0)
    assert fm.converged and fm.conv and fm.niter >= 1
    P, T = fm.P, _host(fm.T)
    assert P.shape == (p, nlv) and T.shape == (n, nlv) and fm.sv.shape == (nlv,)
    e_xm = float(np.max(np.abs(fm.xmeans - rf["xmeans"])))
    print(f"pcasph {case}: niter={fm.niter} |dxmeans| / loop bound = {e_xm / b['lb']:.3g}")
    assert e_xm <= b["lb"]
    assert np.allclose(fm.xscales, rf["xscales"], rtol=1e-12, atol=0)
    assert np.allclose(_host(fm.weights), rf["weights"], rtol=1e-13, atol=0)
    assert np.allclose(fm.colvar, rf["weights"] @ (X - rf["weights"] @ X) ** 2, rtol=1e-11, atol=0)
    # sv: within the derived bound, descending, in the restatement's order
    e_sv = np.abs(fm.sv - rf["sv"])
    print(f"   max |dsv| / bound = {float(np.max(e_sv / b['sv'])):.3g}")
    assert np.all(e_sv <= b["sv"]) and np.all(np.diff(fm.sv) <= 0)
    e1 = rf["eig_all"][0]
    assert np.max(np.abs(fm.eig - rf["eig"])) <= 1e-10 * e1 + 4 * b["sv"].max()
    assert np.isclose(fm.sstot, 1.0, rtol=1e-12)                                   # the trace of the Gram of unit rows under weights that sum to 1
    # P column by column, sign-aligned, under 10 eig_tol eig_1 / gap; T = cscale(X) P to the accessor bound
    for i in range(nlv):
        a, r_ = P[:, i], rf["P"][:, i]
        s = 1.0 if a @ r_ >= 0 else -1.0
        err = np.linalg.norm(a - s * r_)
        print(f"   column {i}: |dp| / bound = {err / max(b['cb'][i], 1e-11):.3g}")
        assert err <= max(b["cb"][i], 1e-11) + 1e-13
    Tr, fac = ref_affine(X, fm.xmeans, fm.xscales, P, None)                      # T = cscale(X) P of the RETURNED P, to the accessor bound
    assert np.all(np.abs(T - Tr) <= bound_affine(X, fm.xmeans, fm.xscales, P, None, fac))
    # transform on the training rows reproduces T; device input gives the bits of the host input
    Tt = _host(J.transform(fm, X))
    assert np.array_equal(Tt, T)
    fd = J.pcasph(_dev(X), None if w is None else torch.as_tensor(w, device="cuda:0"), nlv=nlv, typc=typc, scal=scal)
    assert isinstance(fd.T, torch.Tensor) and np.array_equal(_host(fd.T), T) and np.array_equal(fd.P, P) and np.array_equal(fd.sv, fm.sv)
    assert np.array_equal(fd.xmeans, fm.xmeans) and np.array_equal(_host(fd.weights), _host(fm.weights))


def test_a_row_at_the_centre_is_counted_and_warned_about(J):
    X, w = symmetric_design()
    with pytest.warns(RuntimeWarning, match="centre"):
        fm = J.pcasph(X, w, nlv=2, typc="mean")
    assert np.all(fm.xmeans == 0.0)
    assert np.all(np.isfinite(fm.P)) and np.all(np.isfinite(fm.sv)) and np.all(_host(fm.T)[0] == 0.0)
    assert fm.niter >= 1 and np.isclose(fm.sstot, 1.0 - w[0] / w.sum(), rtol=1e-12)  # the zero row's weight is missing from the trace


def test_spherical_axis_resists_the_contamination_that_bends_pcasvd(J):
    B = BEHAVIOUR
    X, Q = gen_pca(B["n"], B["p"], contaminated=True)
    fs = J.pcasph(X, nlv=2)
    fc = J.pcasvd(X, nlv=2)
    a_sph, a_svd = angle_deg(fs.P[:, 0], Q[:, 0]), angle_deg(fc.P[:, 0], Q[:, 0])
    print(f"angle to the clean axis: pcasph {a_sph:.2f} deg, pcasvd {a_svd:.2f} deg")
    assert a_sph <= B["angle_sph_deg"] and a_svd >= B["angle_svd_deg"]
    # the outlier family takes the model as it is, and flags the shifted rows
    k = B["n"] // 10
    sdod = J.occsdod(fs, X, nlv_sd=2, nlv_od=2)
    ds = _host(sdod.d["dstand"])
    assert np.all(ds[:k] > 1.0) and np.mean(ds[k:] > 1.0) < 0.1
    assert _host(J.occsd(fs).d["d"]).shape == (B["n"],) and _host(J.occod(fs, X).d["d"]).shape == (B["n"],)
    sm = J.summary(fs, X)
    assert sm["coord_var"].shape == (B["p"], 2) and np.all(np.isfinite(sm["cor_circle"])) and np.allclose(sm["contr_var"].sum(axis=0), 1.0)
    Xn = np.asfortranarray(X[::7] + 0.01)
    assert np.allclose(_host(J.transform(fs, Xn)), ((Xn - fs.xmeans) / fs.xscales) @ fs.P, rtol=1e-10, atol=1e-10)
    assert J.pcasph_ is J.pcasph


def test_errors_through_the_c_abi(J):
    lib = J.load()
    ctx = J.Context(0)
    X = gen_pca(30, 6)[0]
    a = [ctx._h, 0, X.ctypes.data, 30, 6, 30, None, 2, 0, 1e-3, 100, 0, 1e-10, 300] + [None] * 16
    assert lib.jch_pcasph_fit(*a) == 0                                             # every output may be NULL
    for pos, bad in ((7, 0), (8, 2), (9, 0.0), (10, 0), (12, 0.0), (13, 0), (5, 29), (1, 3)):
        b = list(a)
        b[pos] = bad
        assert lib.jch_pcasph_fit(*b) == -1, pos
    ctx.close()
