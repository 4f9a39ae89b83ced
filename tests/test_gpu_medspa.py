"""jch_weiszfeld_step and jch_spatial_median on the GPU, through the C ABI with sentinels around every output, against the longdouble restatement
of src/colmedspa.jl under the bounds derived in tests/test_medspa_static.py; then the mirror (colmedspa, weiszfeld_step)."""
import ctypes as C
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

from test_medspa_static import (LD, NAN_CASE, gen, kernel_constants, loop_bound, loop_guard, np_step, ref, step_bound, step_cases)  # noqa: E402

SENT = 7.5
EINVAL = -1


@pytest.fixture(scope="module")
def J():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import jchemo_hip
    return jchemo_hip


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    yield c
    c.close()


def _dev_colmajor(X, ldx, offset):
    """A device copy of X with leading dimension ldx whose first element sits `offset` doubles behind an allocation's start; pad rows hold 7."""
    n, p = X.shape
    buf = torch.full((offset + ldx * p,), 7.0, dtype=torch.float64, device="cuda:0")
    V = buf[offset:].view(p, ldx).t()
    V[:n].copy_(torch.as_tensor(np.array(X), device="cuda:0"))
    torch.cuda.synchronize()
    return buf, buf.data_ptr() + 8 * offset


def _step(J, ctx, loc, xaddr, n, p, ldx, mu0, delta, guard):
    """One jch_weiszfeld_step; d lives where X lives.  Returns (status, mu, d, w0, h, nleft) with the sentinels checked."""
    lib = J.load()
    mu = np.full(p + 2, SENT)
    mu0 = np.ascontiguousarray(mu0, dtype=np.float64)
    w0, h, nl = C.c_double(-1.0), C.c_double(-1.0), C.c_int64(-1)
    if loc == 0:
        d = np.full(n + 2, SENT)
        da = d.ctypes.data + 8
    else:
        dd = torch.full((n + 2,), SENT, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        da = dd.data_ptr() + 8
    st = lib.jch_weiszfeld_step(ctx._h, loc, xaddr, n, p, ldx, mu0.ctypes.data, float(delta), float(guard), mu.ctypes.data + 8, da, C.byref(w0), C.byref(h),
                                C.byref(nl))
    if loc != 0:
        d = dd.cpu().numpy()
    assert mu[0] == SENT and mu[-1] == SENT and d[0] == SENT and d[-1] == SENT
    return st, mu[1:-1], d[1:-1], w0.value, h.value, nl.value


def _loop(J, ctx, loc, xaddr, n, p, ldx, delta, maxit=1000):
    lib = J.load()
    mu = np.full(p + 2, SENT)
    nit, cvg, h = C.c_int32(-1), C.c_int32(-1), C.c_double(-1.0)
    if loc == 0:
        d = np.full(n + 2, SENT)
        da = d.ctypes.data + 8
    else:
        dd = torch.full((n + 2,), SENT, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        da = dd.data_ptr() + 8
    ctx.check(lib.jch_spatial_median(ctx._h, loc, xaddr, n, p, ldx, float(delta), int(maxit), mu.ctypes.data + 8, da, C.byref(nit), C.byref(h), C.byref(cvg)))
    if loc != 0:
        d = dd.cpu().numpy()
    assert mu[0] == SENT and mu[-1] == SENT and d[0] == SENT and d[-1] == SENT
    return mu[1:-1], d[1:-1], nit.value, h.value, cvg.value


def _check_step(got, X, mu0, delta, nleft_guard):
    """mu, d, w0, h within the step bound of the longdouble step; nleft = the rows at or below the guard (None: the exact clamp; inf: all)."""
    st, mu, d, w0, h, nl = got
    assert st == 0
    b = step_bound(X)
    mld, dld, wld, hld, cld = np_step(X, mu0, delta, LD)
    e_mu = float(np.max(np.abs(mu.astype(LD) - mld)))
    e_d = float(np.max(np.abs(d.astype(LD) - dld) / np.maximum(dld, LD(1e-300))))
    print(f"   guard {nleft_guard}: |dmu| / bound = {e_mu / b['mu']:.3g}  max |dd| / (d bound) = {e_d / b['d_rel']:.3g}  nleft = {nl}")
    assert e_mu <= b["mu"]
    assert np.all(np.abs(d.astype(LD) - dld) <= b["d_rel"] * dld)
    assert abs(LD(w0) - wld) <= b["w0_rel"] * np.max(dld)
    assert abs(LD(h) - hld) <= b["h_mu"] * b["mu"] + b["h_rel"] * hld
    d64 = dld.astype(np.float64)
    want = int(cld.sum()) if nleft_guard is None else (X.shape[0] if np.isinf(nleft_guard) else int(np.sum(d64 <= nleft_guard)))
    assert nl == want, (nl, want)


@pytest.mark.parametrize("case", step_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_step_on_every_branch_against_the_longdouble_restatement(J, ctx, case):
    kind, n, p, delta = case
    r = ref(case)
    X = r["X"]
    X0 = X.copy()
    tr = r["tr64"]
    print(f"case {case}: {r['it64']} steps")
    # the first step of the loop: no previous median, so the exact route and the all-rows route
    mu0 = np.asarray(tr[0]["mu0"], dtype=np.float64)
    for guard in (-1.0, np.inf):
        _check_step(_step(J, ctx, 0, X.ctypes.data, n, p, n, mu0, delta, guard), X, mu0, delta, None if guard < 0 else guard)
    # the second step (the last one where the loop took one only: its centre is then the first step's): all three routes
    k_ = min(1, len(tr) - 1)
    mu0 = np.asarray(tr[k_]["mu0"], dtype=np.float64)
    prev = tr[max(k_ - 1, 0)]
    lg = loop_guard(delta, float(prev["w0"]), float(prev["h"]))
    for guard in (-1.0, lg, np.inf):
        _check_step(_step(J, ctx, 0, X.ctypes.data, n, p, n, mu0, delta, guard), X, mu0, delta, None if guard < 0 else guard)
    # a guard below ep is refused once the median is known, and nothing is written
    ep = float(delta * np_step(X, mu0, delta)[2])
    if ep > 0:
        st, mu, d, w0, h, nl = _step(J, ctx, 0, X.ctypes.data, n, p, n, mu0, delta, 0.5 * ep)
        assert st == EINVAL and np.all(mu == SENT) and np.all(d == SENT) and nl == -1
        assert "guard" in J.load().jch_last_error(ctx._h).decode()
    assert np.array_equal(X, X0)


@pytest.mark.parametrize("case", step_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_loop_against_the_longdouble_restatement(J, ctx, case):
    kind, n, p, delta = case
    r = ref(case)
    X = r["X"]
    mu, d, nit, h, cvg = _loop(J, ctx, 0, X.ctypes.data, n, p, n, delta)
    lb = loop_bound(case)
    err = float(np.max(np.abs(mu.astype(LD) - r["muld"])))
    print(f"case {case}: niter {nit} (restatement {r['it64']})  |dmu| / loop bound = {err / lb:.3g}")
    assert nit == r["it64"] == r["itld"] and cvg == 1
    assert err <= lb
    last = r["trld"][-1]
    b = step_bound(X)
    assert np.all(np.abs(d.astype(LD) - last["d"]) <= b["d_rel"] * last["d"] + np.sqrt(p) * lb)   # the distances to the LAST centre stepped from
    assert abs(LD(h) - last["h"]) <= 2 * np.sqrt(p) * lb + b["h_rel"] * last["h"]


_K = kernel_constants()
# one row into a second tile; several workgroups; clamped rows over three workgroups; the second-sweep path
BITS = [c for c in step_cases() if c[:3] in (("cloud", _K["rows"] + 1, 7), ("cloud", 1000, 130), ("dup", 2 * _K["rows"] * _K["tiles"] + 3, _K["waves"] * 16 + 2),
                                             ("cloud", 130, 2 * _K["waves"] * _K["cpw"] + 76))]


@pytest.mark.parametrize("case", BITS, ids=lambda c: "-".join(str(v) for v in c))
def test_identical_bits_wherever_x_lives_and_whatever_the_ctx_did_before(J, ctx, case):
    kind, n, p, delta = case
    assert len(BITS) == 4
    r = ref(case)
    X = r["X"]
    tr = r["tr64"]
    k_ = min(1, len(tr) - 1)
    mu0 = np.asarray(tr[k_]["mu0"], dtype=np.float64)
    prev = tr[max(k_ - 1, 0)]
    lg = loop_guard(delta, float(prev["w0"]), float(prev["h"]))
    buf_a, addr_a = _dev_colmajor(X, n, 0)
    buf_u, addr_u = _dev_colmajor(X, n + 3, 1)
    keep_a, keep_u = buf_a.clone(), buf_u.clone()

    def run(c):
        out = []
        for loc, addr, ld in ((0, X.ctypes.data, n), (1, addr_a, n), (1, addr_u, n + 3)):
            for guard in (-1.0, lg):
                out.append(_step(J, c, loc, addr, n, p, ld, mu0, delta, guard))
            out.append(_loop(J, c, loc, addr, n, p, ld, delta))
        return out

    def same(a, b):
        return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))

    first = run(ctx)
    for k in range(3, 9):                       # host, device aligned, device unaligned: route by route the same bits
        assert same(first[k], first[k % 3])
    again = run(ctx)                            # two runs
    assert all(same(a, b) for a, b in zip(first, again))
    fresh = J.Context(0)                        # a fresh ctx against the used one
    try:
        assert all(same(a, b) for a, b in zip(first, run(fresh)))
    finally:
        fresh.close()
    # another entry takes the workspace in between (the selection's counters, the Gram's partials): no stale state
    J.col_median_mad(gen("cloud", 300, 9), ctx=ctx)
    J.pcasvd(gen("cloud", 120, 11), nlv=2, ctx=ctx)
    assert all(same(a, b) for a, b in zip(first, run(ctx)))
    assert torch.equal(buf_a, keep_a) and torch.equal(buf_u, keep_u)   # X and its pad rows untouched


def test_one_nan_makes_everything_nan_and_ends_the_loop(J, ctx):
    kind, n, p, delta = NAN_CASE
    X = gen(kind, n, p)
    mu0 = np.nanmedian(X, axis=0)
    for guard in (-1.0, 1e-3, np.inf):
        st, mu, d, w0, h, nl = _step(J, ctx, 0, X.ctypes.data, n, p, n, mu0, delta, guard)
        assert st == 0 and np.all(np.isnan(mu)) and np.isnan(w0) and np.isnan(h)
        assert np.isnan(d[n // 2]) and np.sum(np.isnan(d)) == 1          # the NaN stays in its row of d
    mu, d, nit, h, cvg = _loop(J, ctx, 0, X.ctypes.data, n, p, n, delta)
    assert nit == 1 and cvg == 1 and np.all(np.isnan(mu)) and np.isnan(h)


def test_one_row_gives_nan_and_maxit_is_reported(J, ctx):
    X = np.asfortranarray(np.array([[1.0, 2.0, 3.0]]))
    mu, d, nit, h, cvg = _loop(J, ctx, 0, X.ctypes.data, 1, 3, 1, 1e-6)
    assert nit == 1 and np.all(np.isnan(mu)) and d[0] == 0.0             # 0 / 0, as in the reference
    case = next(c for c in step_cases() if ref(c)["it64"] >= 3)
    r = ref(case)
    X = r["X"]
    n, p = X.shape
    mu, d, nit, h, cvg = _loop(J, ctx, 0, X.ctypes.data, n, p, n, case[3], maxit=2)
    assert nit == 2 and cvg == 0 and h > case[3] * np.sqrt(p)
    with pytest.warns(RuntimeWarning, match="no convergence"):
        m2 = J.colmedspa(X, delta=case[3], maxit=2, ctx=ctx)
    assert np.array_equal(m2, mu)
    lib = J.load()
    for bad in (dict(n=0), dict(p=0), dict(ldx=n - 1), dict(delta=0.0), dict(maxit=0), dict(loc=2)):
        a = dict(loc=0, n=n, p=p, ldx=n, delta=1e-6, maxit=10)
        a.update(bad)
        assert lib.jch_spatial_median(ctx._h, a["loc"], X.ctypes.data, a["n"], a["p"], a["ldx"], a["delta"], a["maxit"], mu.ctypes.data, None, None, None,
                                      None) == EINVAL
    assert lib.jch_weiszfeld_step(ctx._h, 0, X.ctypes.data, n, p, n, mu.ctypes.data, 1e-6, float("nan"), mu.ctypes.data, None, None, None, None) == EINVAL


def test_mirror_host_and_device_inputs_give_identical_bits(J, ctx):
    case = next(c for c in step_cases() if c[:3] == ("cloud", 1000, 130))
    r = ref(case)
    X = r["X"]
    n, p = X.shape
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mh = J.colmedspa(X, delta=case[3], ctx=ctx)
        Xd = torch.as_tensor(np.array(X), device="cuda:0").t().contiguous().t()      # column-major on the device
        md = J.colmedspa(Xd, delta=case[3], ctx=ctx)
    assert isinstance(md, np.ndarray) and np.array_equal(mh, md)
    assert np.array_equal(mh, _loop(J, ctx, 0, X.ctypes.data, n, p, n, case[3])[0])
    assert float(np.max(np.abs(mh.astype(LD) - r["muld"]))) <= loop_bound(case)
    mu0 = np.asarray(r["tr64"][0]["mu0"], dtype=np.float64)
    sh = J.weiszfeld_step(X, mu0, delta=case[3], ctx=ctx)
    sd = J.weiszfeld_step(Xd, mu0, delta=case[3], ctx=ctx)
    assert np.array_equal(sh[0], sd[0]) and np.array_equal(sh[1], sd[1].cpu().numpy()) and sh[2:] == sd[2:]
    assert np.array_equal(sh[0], _step(J, ctx, 0, X.ctypes.data, n, p, n, mu0, case[3], -1.0)[1])
