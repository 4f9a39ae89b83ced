"""The bf16 storage mode of plskern on the GPU at every row, column and tile boundary: the cases, the data and the proof that the budgets have power
on them are in test_bf16_static (its docstring says why a skipped, duplicated or mis-weighted boundary element cannot hide under them).

Every single-rank case is one jch_plskern_fit through the C ABI on device buffers: X and Y as bf16 inside NaN-guarded allocations, the rows between n
and the leading dimension NaN, T and weights_norm (and the weights) in the guarded Float64 buffers of test_gpu_accessors.  After the fit the
allocations of X and Y are bit-identical to before (the guards and the pad rows with them), the weights unchanged, T written in exactly n x nlv_out,
weights_norm in n, everything returned finite: a NaN that leaks out of a pad row, which the 16-byte kernels load on purpose, shows up here.

Parity is against O.plskern on the rounded inputs under the budgets the mode already has (BUDGET, BUDGET_B and the statistics' 1e-12; 1e-7 for
xmeans from the bf16 matrix pipe; 1e-8 where the inputs are widened to Float64), plus the first weight vector, which is a function of X'DY alone
(TIGHT where the products are f64, W1_PIPE on the matrix pipe), plus the scores in the max norm per latent variable under the same 1e-3.  The
sharded cases run on three loopback ranks through test_gpu_parity._run_sharded: the same checks on the concatenated scores and rank 0's model, the
replicated state bit-identical on all ranks.  Every case prints its figures (`-s`); the last test prints them all."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "jchemo.jl_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import test_bf16_static as S  # noqa: E402
import test_gpu_parity as TP  # noqa: E402
from test_gpu_accessors import Dev  # noqa: E402
from test_gpu_inplace import MODEL, _trim  # noqa: E402
from oracle import plsr_oracle as O  # noqa: E402

GUARD = 8                      # bf16 elements (16 bytes) of NaN in front of and behind every bf16 matrix
FIGURES = {}                   # case -> the errors it showed (recorded, never gated beyond the budgets)
KNOBS = ("JCH_BF16_K2_PANEL", "JCH_BF16_K2_NH", "JCH_BF16_K2_M32", "JCH_CENTRED_COPY", "JCH_LV_SPLIT", "JCH_SWEEP_TSTAGE")


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


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


# ---------------------------------------------------------------------------------------------------- buffers
class BDev:
    """A column-major bf16 matrix (rows x cols, leading dimension ld) inside a NaN-filled allocation: GUARD elements in front (GUARD + shift: the
    matrix then starts 2 * shift bytes past a 16-byte boundary, as a view from row `shift` of an aligned parent does), GUARD behind, NaN in the rows
    beyond `rows`."""

    def __init__(self, A, ld, shift=0):
        self.rows, self.cols = A.shape
        self.ld, self.front = ld, GUARD + shift
        assert ld >= self.rows
        self.buf = torch.full((self.front + ld * self.cols + GUARD,), float("nan"), dtype=torch.bfloat16, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.body = self.buf[self.front:self.front + ld * self.cols].view(self.cols, ld)
        self.body[:, :self.rows] = torch.from_numpy(np.array(A.T, order="C")).to(torch.bfloat16)      # (a copy: the case data are read-only)
        assert np.array_equal(self.view().to(torch.float64).cpu().numpy(), A), "the inputs are not bf16 values"
        self.ptr = self.body.data_ptr()
        assert self.ptr % 16 == (2 * shift) % 16
        torch.cuda.synchronize()
        self.before = self.bits()
        nan = np.isnan(self.buf.to(torch.float32).cpu().numpy())
        assert nan.sum() == self.buf.numel() - self.rows * self.cols, "guards and pad rows must be NaN, the matrix not"

    def bits(self):
        return self.buf.view(torch.int16).cpu().numpy().copy()

    def view(self):
        """rows x cols with strides (1, ld)."""
        return self.body[:, :self.rows].t()

    def unchanged(self, what):
        assert np.array_equal(self.bits(), self.before), f"{what}: the caller's allocation was written (matrix, pad rows or guards)"


# ---------------------------------------------------------------------------------------------------- checks
def _check(c, T, o, wn, rank_note=""):
    """T (n x k, host), the model o, weights_norm against the oracle of the case; returns the figures."""
    ref = S.oracle(c)
    pipe = S.route(c)[1]
    widened = c.p > S.SWEEP_MAXP
    k = min(c.n, c.p, c.nlv)
    assert T.shape == (c.n, k) and o["P"].shape == (c.p, k)
    for f, v in list(o.items()) + [("T", T), ("weights_norm", wn)]:
        assert np.isfinite(v).all(), f"{c.name}{rank_note}: {f} is not finite"
    e = S.errors(ref, T, o["P"], o["C"], o["W"], o["R"])
    for f in ("xmeans", "xscales", "ymeans", "yscales"):
        e[f] = O.rel_fro(getattr(ref, f), o[f])
    e["TT"] = O.rel_fro(ref.TT, o["TT"])
    FIGURES[c.name] = e
    print(f"  {c.name} [{c.branch}]: " + ", ".join(f"{f} {v:.1e}" for f, v in e.items()))
    d = np.ones(c.n) / c.n if not c.weights else S.case_weights(c) / S.case_weights(c).sum()
    assert O.rel_fro(d, wn) < 1e-12, c.name
    for f in ("xscales", "ymeans", "yscales"):
        assert e[f] < 1e-12, (c.name, f, e[f])
    assert e["xmeans"] < (1e-7 if pipe else 1e-12), (c.name, e["xmeans"])
    for f in ("T", "P", "C", "W", "R"):
        assert e[f] < S.BUDGET, (c.name, f, e)
    if widened:
        for f in ("P", "C", "R", "T"):
            assert e[f] < 1e-8, (c.name, f, e)
    assert e["B"] < S.BUDGET_B, (c.name, e)
    assert e["w1"] < (S.W1_PIPE if pipe else S.TIGHT), (c.name, "the first weight vector (X'DY alone)", e["w1"])
    assert e["Tmax"] < S.BUDGET, (c.name, "scores, element by element", e["Tmax"])
    assert e["TT"] < S.BUDGET, (c.name, e)
    return e


# ---------------------------------------------------------------------------------------------------- a. one rank, through the C ABI
@pytest.mark.parametrize("c", [c for c in S.CASES if c.cuts is None], ids=lambda c: c.name)
def test_edges(J, ctx, monkeypatch, c):
    X, Y, w = S.case_data(c)
    for name, value in c.env:
        monkeypatch.setenv(name, value)
    kmax = max(1, min(c.p, c.nlv))
    xd, yd = BDev(X, c.ldx, c.shift), BDev(Y, c.ldx, c.shift)
    wd = None if w is None else Dev(w)
    td, nd = Dev(rows=c.n, cols=kmax), Dev(rows=c.n, cols=1)
    o = dict(P=np.full((c.p, kmax), np.nan, order="F"), R=np.full((c.p, kmax), np.nan, order="F"), W=np.full((c.p, kmax), np.nan, order="F"),
             C=np.full((c.q, kmax), np.nan, order="F"), TT=np.full(kmax, np.nan), xmeans=np.full(c.p, np.nan), xscales=np.full(c.p, np.nan),
             ymeans=np.full(c.q, np.nan), yscales=np.full(c.q, np.nan))
    desc = J._lib.PlsDesc(n=c.n, p=c.p, q=c.q, nlv=c.nlv, scal=int(c.scal), dtype=J._lib.BF16, loc=J._lib.LOC_DEVICE, inplace=0, reserved=0)
    got = C.c_int32(-1)
    torch.cuda.synchronize()
    st = J.load().jch_plskern_fit(ctx._h, C.byref(desc), xd.ptr, xd.ld, yd.ptr, yd.ld, wd.ptr if wd else None, td.ptr,
                                  *[o[f].ctypes.data for f in MODEL], nd.ptr, C.byref(got))
    assert st == 0, (c.name, J.load().jch_last_error(ctx._h))
    torch.cuda.synchronize()
    k = got.value
    assert k == min(c.n, c.p, c.nlv), (c.name, k)
    xd.unchanged(f"{c.name}: X")
    yd.unchanged(f"{c.name}: Y")
    if wd:
        wd.unchanged()
    T = td.get(k)                      # (the columns from k on, the rows beyond n and the guards are still NaN)
    wn = nd.get()[:, 0]
    _check(c, T, _trim(o, k), wn)


# ---------------------------------------------------------------------------------------------------- b. three loopback ranks
@pytest.mark.parametrize("c", [c for c in S.CASES if c.cuts is not None], ids=lambda c: c.name)
def test_sharded_edges(J, c):
    X, Y, w = S.case_data(c)
    bounds = list(zip(c.cuts[:-1], c.cuts[1:]))
    xs = [BDev(np.asfortranarray(X[a:b]), S.roundup(b - a, 8)) for a, b in bounds]
    ys = [BDev(np.asfortranarray(Y[a:b]), S.roundup(b - a, 8)) for a, b in bounds]
    ws = [None if w is None else torch.from_numpy(w[a:b].copy()).cuda() for a, b in bounds]
    for xd, yd in zip(xs, ys):
        assert xd.view().stride() == (1, xd.ld) and yd.view().stride() == (1, yd.ld)
    torch.cuda.synchronize()
    fms = TP._run_sharded(J, "plskern", [(xd.view(), yd.view(), wr) for xd, yd, wr in zip(xs, ys, ws)], c.nlv, c.scal)
    torch.cuda.synchronize()
    for r, (xd, yd) in enumerate(zip(xs, ys)):
        xd.unchanged(f"{c.name}: X of rank {r}")
        yd.unchanged(f"{c.name}: Y of rank {r}")
        assert w is None or np.array_equal(ws[r].cpu().numpy(), w[bounds[r][0]:bounds[r][1]]), "the weights were modified"
    k = min(c.n, c.p, c.nlv)
    for r, fm in enumerate(fms):
        assert fm.T.shape == (bounds[r][1] - bounds[r][0], k), (c.name, r, fm.T.shape)
    for f in ("P", "R", "W", "C", "TT", "xmeans", "xscales"):
        for r, fm in enumerate(fms[1:], 1):
            assert np.array_equal(getattr(fms[0], f), getattr(fm, f)), f"{c.name}: {f} of rank {r} differs from rank 0's"
    T = torch.cat([fm.T for fm in fms], dim=0).cpu().numpy()
    wn = torch.cat([fm.weights for fm in fms]).cpu().numpy()
    _check(c, T, {f: getattr(fms[0], f) for f in MODEL}, wn, " (rank 0)")


# ---------------------------------------------------------------------------------------------------- c. the report
def test_zz_report_the_figures():
    """Not a check of its own: the largest error each case showed (the first per-branch numbers of the mode; no gate is derived from them)."""
    for name in S.IDS:
        if name in FIGURES:
            e = FIGURES[name]
            print(f"  {name:18s} TPCWR {max(e[f] for f in ('T', 'P', 'C', 'W', 'R')):.1e}  B {e['B']:.1e}  w_1 {e['w1']:.1e}  max|dT|/max|T| {e['Tmax']:.1e}"
                  f"  xmeans {e['xmeans']:.1e}")
