"""jch_row_resid_ss_lv, wshenk, plsravg, the voting discrimination models and their local forms on the GPU.

  * The primitive through the C ABI against the extended-precision restatement (plsavg_restate.resid_ss_lv_longdouble) under
    test_occ_static.resid_ss_bound per level, for the shapes of the issue plus one on each side of every limit the kernel has: the 256-row
    workgroup, the 8-column ring of X, the level chunks of 8, 16 and 32 and a third chunk.  NaN-padded ldx / ldz / ldo, an X one double off its
    buffer, host against device: identical bits; padding and rows beyond m untouched; a NaN stays in its row; level a has the same bits whatever
    the range asked for and agrees with jch_row_resid_ss(k = a) within the sum of the two bounds.  Every case prints its largest error / bound.
  * `wshenk`, `plsravg` (unif, shenk, cv, stack) and plsrdaavg / plsldaavg / plsqdaavg against the literal restatements at 1e-9, the project's
    figure for literal restatements; labels wherever the restatement's two largest vote totals differ.
  * The local models against the `locw` restatements at 1e-7; the batched Shenk entry jch_lwplsravg_predict_prepared: pred, wlv, rss_r, rss_b,
    pred_lv bit-identical to the plain p-space call, info 1 and 2, the clamp, the envelope."""
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

import plsavg_restate as R  # noqa: E402
from oracle import plsr_oracle as O  # noqa: E402
from test_occ_static import prim_inputs, resid_ss_bound, resid_ss_longdouble  # noqa: E402
from test_plsavg_static import avg_data  # noqa: E402

# (m, p, a_lo, a_hi, kz): the issue's, then the kernel's own limits — rows 255 / 256 (one workgroup), columns 7 / 8 / 9 (the ring of X), levels
# 8 | 9 and 16 | 17 (the register-held chunk sizes), 32 | 33 (a second chunk that replays the first), 65 (a third chunk; chunk 0 is skipped)
SHAPES = [(1, 1, 0, 1, 1), (63, 15, 1, 3, 3), (64, 16, 0, 4, 4), (65, 17, 2, 5, 7), (257, 33, 1, 25, 25), (300, 500, 1, 25, 25), (70, 2049, 0, 5, 5),
          (130, 40, 1, 49, 49),
          (255, 7, 0, 8, 8), (256, 8, 1, 9, 9), (70, 9, 0, 16, 16), (70, 12, 2, 17, 20), (70, 12, 0, 32, 32), (70, 12, 1, 33, 33), (66, 9, 40, 65, 65)]
NANPAD = float("nan")


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


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _dev_colmajor(A, ld, offset):
    """A device copy of A with leading dimension ld whose first element sits `offset` doubles behind an allocation's start; NaN elsewhere."""
    n, c = A.shape
    buf = torch.full((offset + ld * max(c, 1),), NANPAD, dtype=torch.float64, device="cuda:0")
    V = buf[offset:offset + ld * c].view(c, ld).t()
    V[:n].copy_(torch.as_tensor(np.array(A), device="cuda:0"))
    return V, buf.data_ptr() + 8 * offset, ld


def _layouts(A):
    """(aligned with a padded even ld, one double off with a padded odd ld)."""
    n = A.shape[0]
    return _dev_colmajor(A, n + 2 + n % 2, 0), _dev_colmajor(A, n + 1 + n % 2, 1)


def _call(J, ctx, loc, xa, m, p, ldx, shift, za, kz, ldz, B, a_lo, a_hi, pad):
    """out (m x le) as a host array, written with leading dimension m + pad; what lies behind row m of every column must stay NaN."""
    lib = J.load()
    le = a_hi - a_lo + 1
    ldo = m + pad
    sa = None if shift is None else shift.ctypes.data
    ba = B.ctypes.data if kz else None
    if loc == 0:
        out = np.full((le, ldo), NANPAD)
        ctx.check(lib.jch_row_resid_ss_lv(ctx._h, 0, xa, m, p, ldx, sa, za if kz else None, kz, ldz, ba, p, a_lo, a_hi, out.ctypes.data, ldo))
    else:
        od = torch.full((le * ldo + 1,), NANPAD, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        ctx.check(lib.jch_row_resid_ss_lv(ctx._h, 1, xa, m, p, ldx, sa, za if kz else None, kz, ldz, ba, p, a_lo, a_hi, od.data_ptr() + 8, ldo))
        o = _host(od)
        assert np.isnan(o[0])
        out = o[1:].reshape(le, ldo)
    assert np.all(np.isnan(out[:, m:]))
    return out[:, :m].T.copy()


def _all_runs(J, ctx, X, shift, Z, B, a_lo, a_hi):
    """The same call as host data and as device data in every combination of (aligned, even ld) / (one double off, odd ld) for X and for Z, with
    a tight and a padded out.  X and Z come back unchanged and the NaN behind row m of every column is untouched; returns the results."""
    m, p = X.shape
    kz = Z.shape[1]
    X0, Z0 = X.copy(), Z.copy()
    runs = [_call(J, ctx, 0, X.ctypes.data, m, p, m, shift, Z.ctypes.data, kz, m, B, a_lo, a_hi, 0),
            _call(J, ctx, 0, X.ctypes.data, m, p, m, shift, Z.ctypes.data, kz, m, B, a_lo, a_hi, 3)]
    assert np.array_equal(X, X0, equal_nan=True) and np.array_equal(Z, Z0, equal_nan=True)
    xl = _layouts(X)
    zl = _layouts(Z) if kz else [(None, None, 0)]
    for ix, (xv, xa, ldx) in enumerate(xl):
        for iz, (zv, za, ldz) in enumerate(zl):
            runs.append(_call(J, ctx, 1, xa, m, p, ldx, shift, za, kz, ldz, B, a_lo, a_hi, (ix + 2 * iz) % 3))
    for xv, _, _ in xl:
        assert np.array_equal(_host(xv[:m]), X0, equal_nan=True) and bool(torch.all(torch.isnan(xv[m:])))
    for zv, _, _ in (zl if kz else []):
        assert np.array_equal(_host(zv[:m]), Z0, equal_nan=True) and bool(torch.all(torch.isnan(zv[m:])))
    return runs


# ---------------------------------------------------------------------------------- the primitive
@pytest.mark.parametrize("m,p,a_lo,a_hi,kz", SHAPES)
def test_row_resid_ss_lv_against_the_longdouble_restatement(J, ctx, m, p, a_lo, a_hi, kz):
    X, shift, Z, B = prim_inputs(m, p, kz)
    ref = R.resid_ss_lv_longdouble(X, shift, Z, B, a_lo, a_hi)
    runs = _all_runs(J, ctx, X, shift, Z, B, a_lo, a_hi)
    worst = 0.0
    for a in range(a_lo, a_hi + 1):
        bound = resid_ss_bound(X, shift, Z[:, :a], B[:, :a])
        err = np.abs(np.asarray(runs[0][:, a - a_lo] - ref[:, a - a_lo], dtype=np.float64))
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (a, float(np.max(err / bound)))
    print(f"row_resid_ss_lv m={m} p={p} a={a_lo}:{a_hi} kz={kz}: max err / bound = {worst:.3g}")
    for r in runs[1:]:                                     # host / device, aligned / unaligned X and Z, tight / padded out: the same bits
        assert np.array_equal(r, runs[0])


def test_row_resid_ss_lv_nan_stays_in_its_row(J, ctx):
    m, p, kz = 257, 33, 25
    X, shift, Z, B = prim_inputs(m, p, kz)
    base = _all_runs(J, ctx, X, shift, Z, B, 0, 25)[0]
    i, j, i2, l = 70, 20, 201, 13
    X[i, j] = np.nan
    Z[i2, l] = np.nan
    for got in _all_runs(J, ctx, X, shift, Z, B, 0, 25):
        keep = np.ones(m, dtype=bool); keep[[i, i2]] = False
        assert np.all(np.isnan(got[i]))                                      # every level holds X[i, j]
        assert np.array_equal(got[i2, :l + 1], base[i2, :l + 1]) and np.all(np.isnan(got[i2, l + 1:]))   # Z[i2, l] enters at level l + 1
        assert np.array_equal(got[keep], base[keep])                          # every other row keeps its bits


@pytest.mark.parametrize("m,p,kz", [(65, 17, 7), (257, 33, 25), (66, 9, 65)])
def test_a_level_has_the_same_bits_whatever_the_range_and_agrees_with_the_single_level_entry(J, ctx, m, p, kz):
    X, shift, Z, B = prim_inputs(m, p, kz)
    lib = J.load()
    full = _call(J, ctx, 0, X.ctypes.data, m, p, m, shift, Z.ctypes.data, kz, m, B, 0, kz, 0)
    for a in sorted({0, 1, kz // 2, kz}):                                    # a_lo = a_hi
        one = _call(J, ctx, 0, X.ctypes.data, m, p, m, shift, Z.ctypes.data, kz, m, B, a, a, 0)
        assert np.array_equal(one[:, 0], full[:, a]), a
    lo, hi = max(1, kz // 3), max(1, 2 * kz // 3)
    part = _call(J, ctx, 0, X.ctypes.data, m, p, m, shift, Z.ctypes.data, kz, m, B, lo, hi, 0)
    assert np.array_equal(part, full[:, lo:hi + 1])
    worst = 0.0
    for a in sorted({0, 1, kz // 2, kz}):                                    # against jch_row_resid_ss with k = a: within the sum of the two bounds
        out = np.empty(m)
        ctx.check(lib.jch_row_resid_ss(ctx._h, 0, X.ctypes.data, m, p, m, shift.ctypes.data, Z.ctypes.data if a else None, a, m,
                                       B.ctypes.data if a else None, p, out.ctypes.data))
        bound = resid_ss_bound(X, shift, Z[:, :a], B[:, :a])
        ref = np.asarray(resid_ss_longdouble(X, shift, Z[:, :a], B[:, :a]), dtype=np.float64)
        assert np.all(np.abs(out - ref) <= bound)
        worst = max(worst, float(np.max(np.abs(out - full[:, a]) / (2 * bound))))
        assert np.all(np.abs(out - full[:, a]) <= 2 * bound), a
    print(f"row_resid_ss_lv vs row_resid_ss m={m} p={p} kz={kz}: max |diff| / (2 bound) = {worst:.3g}")


def test_row_resid_ss_lv_without_shift_and_scores(J, ctx):
    m, p = 65, 17
    X, _, _, _ = prim_inputs(m, p, 0)
    lib = J.load()
    out = np.full(m + 1, NANPAD)
    ctx.check(lib.jch_row_resid_ss_lv(ctx._h, 0, X.ctypes.data, m, p, m, None, None, 0, 0, None, p, 0, 0, out.ctypes.data, m))
    ref = resid_ss_longdouble(X, None, None, None)
    assert np.isnan(out[m]) and np.all(np.abs(np.asarray(out[:m] - ref, dtype=np.float64)) <= resid_ss_bound(X, None, None, None))
    with pytest.raises(J.JchError):
        ctx.check(lib.jch_row_resid_ss_lv(ctx._h, 0, X.ctypes.data, m, p, m, None, None, 0, 0, None, p, 0, 1, out.ctypes.data, m))


def test_mirror_wrapper_host_and_device(J, ctx):
    X, shift, Z, B = prim_inputs(65, 17, 7)
    h = J.row_resid_ss_lv(X, shift, Z, B, 2, 5, ctx=ctx)
    d = J.row_resid_ss_lv(torch.as_tensor(X, device="cuda:0").t().contiguous().t(), shift, torch.as_tensor(Z, device="cuda:0").t().contiguous().t(),
                          B, 2, 5, ctx=ctx)
    assert h.shape == (65, 4) and isinstance(d, torch.Tensor) and np.array_equal(_host(d), h)
    assert np.array_equal(h, _call(J, ctx, 0, X.ctypes.data, 65, 17, 65, shift, Z.ctypes.data, 7, 65, B, 2, 5, 0))


# ---------------------------------------------------------------------------------- wshenk
def _rel(ref, got):
    return O.rel_fro(np.asarray(ref, dtype=np.float64), np.asarray(_host(got), dtype=np.float64))


@pytest.fixture(scope="module")
def data1():
    return avg_data(q=1)


@pytest.fixture(scope="module")
def data3():
    return avg_data(q=3)


@pytest.mark.parametrize("name", ["plain", "weighted", "scal", "pcr"])
def test_wshenk_against_the_restatement(J, ctx, data1, name):
    """n = 150, p = 40, nlv = 8, m = 37: both sides are handed the SAME fitted arrays (the GPU fit's, downloaded), so what is compared is wshenk."""
    X, Y, Xnew, w = data1
    if name == "pcr":
        fm = J.pcr(X, Y, nlv=8, ctx=ctx)
        ref_fm = O.Plsr(T=_host(fm.T), P=np.asarray(fm.R), R=np.asarray(fm.R), W=np.asarray(fm.R), C=np.asarray(fm.C), TT=np.ones(8),
                        xmeans=np.asarray(fm.xmeans), xscales=np.asarray(fm.xscales), ymeans=np.asarray(fm.ymeans), yscales=np.asarray(fm.yscales),
                        weights=_host(fm.weights))
    else:
        fm = J.plskern(X, Y, w if name != "plain" else None, nlv=8, scal=name == "scal", ctx=ctx)
        ref_fm = O.Plsr(**{f: _host(getattr(fm, f)) for f in ("T", "P", "R", "W", "C", "TT", "xmeans", "xscales", "ymeans", "yscales", "weights")})
    for nlv in (None, 5):
        ref = R.np_wshenk(ref_fm, Xnew, nlv)
        for Xq in (Xnew, torch.as_tensor(Xnew, device="cuda:0").t().contiguous().t()):
            got_w, got_wr, got_wb = J.wshenk(fm, Xq, nlv, ctx=ctx)
            errs = (_rel(ref["w"], got_w), _rel(ref["wr"], got_wr), _rel(ref["wb"], got_wb))
            print(f"wshenk {name} nlv={nlv} {'device' if isinstance(Xq, torch.Tensor) else 'host'}: rel. errors w, wr, wb = " + ", ".join(f"{e:.2e}" for e in errs))
            assert max(errs) < 1e-9
            assert isinstance(got_w, torch.Tensor) == isinstance(Xq, torch.Tensor) and got_w.shape == ref["w"].shape


# ---------------------------------------------------------------------------------- plsravg
SEGM2 = [[np.arange(0, 150, 2), np.arange(1, 150, 2)]]
SEGM_STACK = [[np.arange(r, 150, 3) for r in range(3)], [np.sort(np.random.default_rng(9).permutation(150)[j::3]) for j in range(3)]]


def _restated(typf, X, Y, w, nlv):
    if typf == "unif":
        obj = R.np_plsravg_unif(X, Y, w, nlv=nlv); return R.np_plsravg_unif_predict, obj
    if typf == "shenk":
        obj = R.np_plsravg_shenk(X, Y, w, nlv=nlv); return R.np_plsravg_shenk_predict, obj
    if typf == "cv":
        obj = R.np_plsravg_cv(X, Y, w, nlv=nlv, segm=SEGM2); return R.np_plsravg_cri_predict, obj
    obj = R.np_plsrstack(X, Y, w, nlv=nlv, segm=SEGM_STACK); return R.np_plsravg_cri_predict, obj


@pytest.mark.parametrize("nlv", ["0:6", "3:6", "4"])
@pytest.mark.parametrize("typf,q", [("unif", 1), ("unif", 3), ("shenk", 1), ("shenk", 3), ("cv", 1), ("cv", 3), ("stack", 1)])
def test_plsravg_predict_against_the_restatement(J, ctx, data1, data3, typf, q, nlv):
    """pred at 1e-9 of |Y|'s scale and predlv per level, host and device X.  typf = "stack" takes a univariate y only (src/plsrstack.jl:49)."""
    X, Y, Xnew, w = data1 if q == 1 else data3
    predict_ref, obj = _restated(typf, X, Y, w, nlv)
    ref = predict_ref(obj, Xnew)
    scale = float(np.max(np.abs(Y)))
    segm = dict(cv=SEGM2, stack=SEGM_STACK).get(typf)
    for dev in (False, True):
        conv = (lambda a: torch.as_tensor(np.asarray(a), device="cuda:0").t().contiguous().t()) if dev else (lambda a: a)
        fm = J.plsravg(conv(X), conv(Y), conv(w.reshape(-1, 1)).reshape(-1) if dev else w, nlv=nlv, typf=typf, segm=segm, ctx=ctx)
        res = J.predict(fm, conv(Xnew), ctx=ctx)
        pred, predlv = res[0], res[1]
        assert list(fm.fm.nlv) == obj["nlv"]
        predlv = predlv if isinstance(predlv, list) else [predlv]
        e_pred = float(np.max(np.abs(_host(pred) - ref["pred"]))) / scale
        e_lv = max(float(np.max(np.abs(_host(a) - b))) for a, b in zip(predlv, ref["predlv"])) / scale
        print(f"plsravg {typf} q={q} nlv={nlv} {'device' if dev else 'host'}: |pred - ref| / |Y| = {e_pred:.2e}, predlv {e_lv:.2e}")
        assert len(predlv) == len(ref["predlv"]) and e_pred < 1e-9 and e_lv < 1e-9
        if typf == "cv":
            assert np.allclose(fm.fm.w, obj["w"], rtol=0, atol=1e-9, equal_nan=True)   # (one level: fweight gives 0 and mweight 0 / 0 on both sides)
        if typf == "shenk" and len(obj["nlv"]) > 1:
            assert _rel(ref["w"], res[2]) < 1e-9
        assert isinstance(pred, torch.Tensor) == dev


def test_plsravg_inplace_form_and_the_not_implemented_criteria(J, ctx, data1):
    X, Y, Xnew, w = data1
    ref = J.predict(J.plsravg(X, Y, w, nlv="2:5", typf="shenk", ctx=ctx), Xnew, ctx=ctx)
    Xc, Yc = X.copy(order="F"), Y.copy(order="F")
    got = J.predict(J.plsravg_(Xc, Yc, w, nlv="2:5", typf="shenk", ctx=ctx), Xnew, ctx=ctx)
    assert np.max(np.abs(got[0] - ref[0])) < 1e-9 * np.max(np.abs(Y))
    with pytest.raises(NotImplementedError):
        J.plsravg(X, Y, nlv="2:5", typf="bic", ctx=ctx)


# ---------------------------------------------------------------------------------- plsrdaavg, plsldaavg, plsqdaavg
@pytest.fixture(scope="module")
def da_data():
    """Three classes cut from a noisy latent direction: neighbouring levels disagree on some rows near the cuts."""
    rng = np.random.default_rng(21)
    n, m, p = 240, 90, 30
    S = rng.standard_normal((n + m, 5))
    Xall = 3.0 + S @ rng.standard_normal((5, p)) + 0.3 * rng.standard_normal((n + m, p))
    lat = S[:, 0] + 0.6 * S[:, 1] + 0.5 * rng.standard_normal(n + m)
    yall = np.digitize(lat, np.quantile(lat, [1 / 3, 2 / 3])) + 1
    return np.asfortranarray(Xall[:n]), yall[:n], np.asfortranarray(Xall[n:])


@pytest.mark.parametrize("kind,nlv", [("rda", "0:6"), ("rda", "1:7"), ("lda", "1:6"), ("qda", "2:6"), ("lda", "3")])
def test_daavg_labels_against_the_restatement(J, ctx, da_data, kind, nlv):
    """Labels equal the restatement's wherever its two largest vote totals differ; at most 5 % of the rows fall under that exclusion (on the
    restatement alone these cases exclude 2, 1, 1, 0 and 0 of the 90 rows; an even number of levels such as "2:7" would exclude 12 %)."""
    X, y, Xnew = da_data
    ref = R.np_plsdaavg_predict(R.np_plsdaavg(kind, X, y, nlv=nlv), Xnew)
    fit = dict(rda=J.plsrdaavg, lda=J.plsldaavg, qda=J.plsqdaavg)[kind]
    obj = fit(X, y, nlv=nlv, ctx=ctx)
    pred, predlv = J.predict(obj, Xnew, ctx=ctx)
    keep = np.ones(Xnew.shape[0], dtype=bool) if ref["top2"] is None else ref["top2"][:, 0] != ref["top2"][:, 1]
    print(f"{kind}avg nlv={nlv}: {int((~keep).sum())} of {len(keep)} rows excluded as ties; {int((pred[keep] != ref['pred'][keep]).sum())} labels differ")
    assert (~keep).mean() <= 0.05
    assert np.array_equal(pred[keep], ref["pred"][keep])
    assert len(np.unique(ref["pred"])) == 3


def test_daavg_tie_of_two_levels_goes_to_the_smaller_label(J, ctx, da_data):
    """Two levels, two labels: the vote totals tie and `findmax_cla` returns the first maximum over the SORTED labels."""
    X, y, Xnew = da_data
    lv = np.hstack(O.plsrda_predict(O.plsrda(X, y, nlv=7), Xnew, nlv=range(0, 8))[0])
    a = next(k for k in range(1, 7) if np.any(lv[:, k] != lv[:, k + 1]))       # (level 0 predicts one class for every row)
    pred, predlv = J.predict(J.plsrdaavg(X, y, nlv=f"{a}:{a + 1}", ctx=ctx), Xnew, ctx=ctx)
    two = np.hstack(predlv)
    tied = two[:, 0] != two[:, 1]
    assert tied.any()
    assert np.array_equal(pred[:, 0], np.minimum(two[:, 0], two[:, 1]))


# ---------------------------------------------------------------------------------- a used ctx
def test_every_entry_on_a_used_ctx(J, data1):
    """A ctx that has run other fits and primitives (grown and reused workspaces) gives the bits of a fresh one."""
    X, Y, Xnew, w = data1
    Xp, shift, Z, B = prim_inputs(257, 33, 25)

    def work(c):
        fm = J.plskern(X, Y, w, nlv=8, ctx=c)
        out = [J.row_resid_ss_lv(Xp, shift, Z, B, 1, 25, ctx=c), *J.wshenk(fm, Xnew, ctx=c)]
        for typf in ("unif", "shenk"):
            out.append(J.predict(J.plsravg(X, Y, w, nlv="1:6", typf=typf, ctx=c), Xnew, ctx=c)[0])
        return out

    fresh = J.Context(0)
    ref = work(fresh)
    fresh.close()
    used = J.Context(0)
    big = prim_inputs(300, 500, 25)
    J.row_resid_ss(big[0], big[1], big[2], big[3], ctx=used)                  # larger staging than anything below
    J.row_resid_ss_lv(big[0], big[1], big[2], big[3], 0, 25, ctx=used)
    J.predict(J.plskern(big[0], big[2][:, :2], nlv=12, ctx=used), big[0], nlv=range(0, 13), ctx=used)
    got = work(used)
    used.close()
    for r, g in zip(ref, got):
        assert np.array_equal(r, g)


# ---------------------------------------------------------------------------------- the local models
def local_data(n, p, q, m=20, seed=3):
    """Rank-5 structure plus 0.05 noise at offset 10."""
    rng = np.random.default_rng(seed + n + p)
    S = rng.standard_normal((n + m, 5))
    Xall = 10.0 + S @ rng.standard_normal((5, p)) + 0.05 * rng.standard_normal((n + m, p))
    Yall = S[:, :3] @ rng.standard_normal((3, q)) + 0.05 * rng.standard_normal((n + m, q))
    return np.asfortranarray(Xall[:n]), np.asfortranarray(Yall[:n]), np.asfortranarray(Xall[n:])


LOCAL = dict(nlvdis=5, metric="mahal", h=2.0)
LOCAL_CASES = [(300, 40, 40, "1:8", False), (300, 40, 40, "1:8", True), (120, 130, 30, "3:12", False)]


def _conditioning(X, Y, Xq, k, nlv, scal):
    """min over queries and levels of rss_r / |x - xmeans| of the local models, from the restatement alone."""
    listnn, _, listw = R.np_local_lists(X, Y, Xq, k=k, scal=scal, **LOCAL)
    worst = np.inf
    for i in range(Xq.shape[0]):
        fm = O.plskern(X[listnn[i]], Y[listnn[i]], listw[i], nlv=int(str(nlv).split(":")[-1]), scal=scal)
        rss_r, _ = R.np_shenk_rss(fm, Xq[i:i + 1])
        worst = min(worst, float(np.min(rss_r) / np.linalg.norm(Xq[i] - fm.xmeans)))
    return worst


@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("n,p,k,nlv,scal", LOCAL_CASES)
def test_lwplsravg_unif_and_shenk_against_the_restatement(J, ctx, n, p, k, nlv, scal, q):
    """20 queries; pred at 1e-7 relative Frobenius, the figure test_lwplsr_predict uses for local fits.  The data must be well posed from the
    restatement alone: min rss_r / |x - xmeans| >= 1e-3.  `unif` is one batched call and equals the mean of lwplsr_predict's levels to 1e-13."""
    X, Y, Xq = local_data(n, p, q)
    cond = _conditioning(X, Y, Xq, k, nlv, scal)
    print(f"lwplsravg n={n} p={p} k={k} nlv={nlv} scal={scal} q={q}: min rss_r / |x - xmeans| = {cond:.3g}")
    assert cond >= 1e-3, "test data ill-posed"
    for typf in ("unif", "shenk"):
        ref = R.np_lwplsravg_predict(X, Y, Xq, k=k, nlv=nlv, typf=typf, scal=scal, **LOCAL)
        fm = J.lwplsravg(X, Y, k=k, nlv=nlv, typf=typf, scal=scal, ctx=ctx, **LOCAL)
        res = J.predict(fm, Xq, ctx=ctx)
        err = O.rel_fro(ref["pred"], res.pred)
        print(f"  {typf}: rel. Frobenius error of pred = {err:.2e}")
        assert np.array_equal(res.listnn, ref["listnn"]) and err < 1e-7
        assert O.rel_fro(ref["listw"], res.listw) < 1e-9
    lo, hi = (int(s) for s in nlv.split(":"))
    lv = J.lwplsr_predict(J.lwplsr(X, Y, k=k, nlv=hi, scal=scal, ctx=ctx, **LOCAL), Xq, nlv=range(lo, hi + 1), ctx=ctx).pred
    un = J.predict(J.lwplsravg(X, Y, k=k, nlv=nlv, scal=scal, ctx=ctx, **LOCAL), Xq, ctx=ctx).pred
    assert np.max(np.abs(un - np.mean(np.stack(lv), axis=0))) <= 1e-13 * np.max(np.abs(Y))


def test_lwplsravg_clamps_the_levels_once_with_n_equal_k(J, ctx):
    """nlv = "5:60" with k = 30 averages the 26 distinct levels 5 .. 30, not 56."""
    from jchemo_hip.plsavg import _local_range
    assert list(_local_range("5:60", 30, 130)) == list(range(5, 31)) and list(_local_range("0:6", 30, 4, 1)) == [1, 2, 3, 4]
    X, Y, Xq = local_data(120, 130, 1)
    un = J.predict(J.lwplsravg(X, Y, k=30, nlv="5:60", ctx=ctx, **LOCAL), Xq, ctx=ctx).pred
    lv = J.lwplsr_predict(J.lwplsr(X, Y, k=30, nlv=30, ctx=ctx, **LOCAL), Xq, nlv=range(5, 31), ctx=ctx).pred
    assert len(lv) == 26
    assert np.allclose(un, np.mean(np.stack(lv), axis=0), rtol=0, atol=1e-13 * np.max(np.abs(Y)), equal_nan=True)


def test_lwplsravg_constant_neighbourhood_and_the_wide_shape_take_the_loop(J, ctx):
    """A neighbourhood with a constant univariate y predicts that value (src/locw.jl:34-36); p = 2100 is beyond the batched p-space kernel and
    meets the same tolerance through the per-query schedule."""
    X, Y, Xq = local_data(300, 40, 1)
    raw = dict(nlvdis=0, metric="eucl", h=2.0)                       # (a search on X itself: it does not move when y is edited)
    listnn, _, _ = R.np_local_lists(X, Y, Xq, k=40, **raw)
    Y = Y.copy(order="F"); Y[listnn[0], 0] = 3.25
    for typf in ("unif", "shenk"):
        ref = R.np_lwplsravg_predict(X, Y, Xq, k=40, nlv="1:8", typf=typf, **raw)
        res = J.predict(J.lwplsravg(X, Y, k=40, nlv="1:8", typf=typf, ctx=ctx, **raw), Xq, ctx=ctx)
        assert ref["const"][0] and abs(res.pred[0, 0] - 3.25) <= (0 if typf == "shenk" else 1e-12)
        assert O.rel_fro(ref["pred"], res.pred) < 1e-7
    X, Y, Xq = local_data(80, 2100, 1, m=3)
    ref = R.np_lwplsravg_predict(X, Y, Xq, k=30, nlv="1:4", typf="shenk", **LOCAL)
    res = J.predict(J.lwplsravg(X, Y, k=30, nlv="1:4", typf="shenk", ctx=ctx, **LOCAL), Xq, ctx=ctx)
    err = O.rel_fro(ref["pred"], res.pred)
    print(f"lwplsravg shenk p=2100: rel. Frobenius error of pred = {err:.2e}")
    assert err < 1e-7


def test_lwplsravg_cv_with_the_same_per_query_segments(J, ctx):
    """typf = "cv" locally: query i's two folds are segmkf(k, 2; rep = 1) drawn from (seed, i); the restatement is handed the same ones."""
    X, Y, Xq = local_data(300, 40, 1, m=4)
    seed = 11
    ref = R.np_lwplsravg_predict(X, Y, Xq, k=40, nlv="1:8", typf="cv", segm_of=lambda i: J.segmkf(40, 2, rep=1, seed=[seed, i]), **LOCAL)
    res = J.lwplsravg_predict(J.lwplsravg(X, Y, k=40, nlv="1:8", typf="cv", ctx=ctx, **LOCAL), Xq, seed=seed, ctx=ctx)
    err = O.rel_fro(ref["pred"], res.pred)
    print(f"lwplsravg cv: rel. Frobenius error of pred = {err:.2e}")
    assert err < 1e-7


@pytest.mark.parametrize("kind,nlv,k", [("rda", "0:4", 80), ("lda", "1:5", 80), ("qda", "1:3", 150)])
def test_local_daavg_labels_against_the_restatement(J, ctx, kind, nlv, k):
    """3 classes, 40 queries.  Labels equal the restatement's except where its two largest vote totals tie or where it cannot fit a
    neighbourhood (a class covariance that is not positive definite); at most 5 % of the rows are excluded."""
    rng = np.random.default_rng(21)
    n, m, p = 300, 40, 30
    S = rng.standard_normal((n + m, 5))
    Xall = 3.0 + S @ rng.standard_normal((5, p)) + 0.3 * rng.standard_normal((n + m, p))
    lat = S[:, 0] + 0.6 * S[:, 1] + 0.5 * rng.standard_normal(n + m)
    yall = np.digitize(lat, np.quantile(lat, [1 / 3, 2 / 3])) + 1
    X, y, Xq = np.asfortranarray(Xall[:n]), yall[:n], np.asfortranarray(Xall[n:])
    kw = dict(nlvdis=4, metric="eucl", h=2.0, k=k, nlv=nlv)
    ref = R.np_lwplsdaavg_predict(kind, X, y, Xq, **kw)
    fit = dict(rda=J.lwplsrdaavg, lda=J.lwplsldaavg, qda=J.lwplsqdaavg)[kind]
    res = J.predict(fit(X, y, ctx=ctx, **kw), Xq, ctx=ctx)
    keep = ~(ref["tie"] | ref["bad"])
    print(f"lw{kind}avg nlv={nlv}: {int((~keep).sum())} of {m} rows excluded; {int((res.pred[keep, 0] != ref['pred'][keep, 0]).sum())} labels differ")
    assert (~keep).mean() <= 0.05
    assert np.array_equal(res.listnn, ref["listnn"]) and np.array_equal(res.pred[keep, 0], ref["pred"][keep, 0])


def test_remaining_entries_on_a_used_ctx(J, data1, da_data):
    """plsravg cv and stack, the three voting models and the local models on a ctx that has run other work: the bits of a fresh one."""
    X, Y, Xnew, w = data1
    Xd, yd, Xdn = da_data
    Xl, Yl, Xlq = local_data(300, 40, 1, m=5)

    def work(c):
        out = []
        for typf, segm in (("cv", SEGM2), ("stack", SEGM_STACK)):
            out.append(J.predict(J.plsravg(X, Y, w, nlv="1:6", typf=typf, segm=segm, ctx=c), Xnew, ctx=c)[0])
        for fit, nlv in ((J.plsrdaavg, "0:6"), (J.plsldaavg, "1:6"), (J.plsqdaavg, "2:6")):
            out.append(J.predict(fit(Xd, yd, nlv=nlv, ctx=c), Xdn, ctx=c)[0])
        for typf in ("unif", "shenk"):
            out.append(J.predict(J.lwplsravg(Xl, Yl, k=40, nlv="1:8", typf=typf, ctx=c, **LOCAL), Xlq, ctx=c).pred)
        for fit, nlv in ((J.lwplsrdaavg, "0:4"), (J.lwplsldaavg, "1:4")):
            out.append(J.predict(fit(Xd, yd, nlvdis=4, metric="eucl", h=2.0, k=80, nlv=nlv, ctx=c), Xdn[:10], ctx=c).pred)
        return out

    fresh = J.Context(0)
    ref = work(fresh)
    fresh.close()
    used = J.Context(0)
    big = prim_inputs(300, 500, 25)
    J.row_resid_ss_lv(big[0], big[1], big[2], big[3], 0, 25, ctx=used)
    J.predict(J.plskern(big[0], big[2][:, :2], nlv=12, ctx=used), big[0], nlv=range(0, 13), ctx=used)
    got = work(used)
    used.close()
    for r, g in zip(ref, got):
        assert np.array_equal(r, g)


# ---------------------------------------------------------------------------------- the batched local Shenk entry
@pytest.mark.parametrize("q", [1, 3])
@pytest.mark.parametrize("n,p,k,nlv,scal", LOCAL_CASES)
def test_local_shenk_outputs_against_the_restatement(J, ctx, monkeypatch, n, p, k, nlv, scal, q):
    """One jch_lwplsravg_predict_prepared: pred, wlv, rss_r, rss_b at 1e-7 relative Frobenius of the literal restatement (the conditioning of the data
    is asserted in test_lwplsravg_unif_and_shenk_against_the_restatement); pred_lv equals jch_lwplsr_predict_prepared's p-space kernel bit for
    bit — the Shenk code must not perturb the fit."""
    X, Y, Xq = local_data(n, p, q)
    ref = R.np_lwplsravg_shenk_details(X, Y, Xq, k=k, nlv=nlv, scal=scal, **LOCAL)
    fm = J.lwplsravg(X, Y, k=k, nlv=nlv, typf="shenk", scal=scal, ctx=ctx, **LOCAL)
    res = J.predict(fm, Xq, ctx=ctx)
    assert isinstance(res, J.LwplsrAvgPred) and list(res.nlv) == list(range(ref["lo"], ref["hi"] + 1)) and not res.info.any()
    errs = {f: O.rel_fro(ref[f], getattr(res, f)) for f in ("pred", "wlv", "rss_r", "rss_b")}
    errs["pred_lv"] = O.rel_fro(ref["pred_lv"], np.stack(res.pred_lv, axis=1))
    print(f"local shenk n={n} p={p} k={k} nlv={nlv} scal={scal} q={q}: " + ", ".join(f"{f} {e:.2e}" for f, e in errs.items()))
    assert max(errs.values()) < 1e-7
    assert np.array_equal(res.listnn, ref["listnn"])
    monkeypatch.setenv("JCH_LOCW_KSPACE", "0")
    hi = ref["hi"]
    lv = J.lwplsr_predict(J.lwplsr(X, Y, k=k, nlv=hi, scal=scal, ctx=ctx, **LOCAL), Xq, nlv=range(ref["lo"], hi + 1), ctx=ctx).pred
    monkeypatch.delenv("JCH_LOCW_KSPACE")
    for a, b in zip(lv if isinstance(lv, list) else [lv], res.pred_lv):
        assert np.array_equal(a, b)


def test_entry_unif_clamp_and_envelope(J, ctx):
    """typf = 0 through the entry: the mean of its own levels in level order, equal to the mirror's unif to 1e-13; "5:60" with k = 30 is 26 levels;
    p = 2100 is outside the envelope: JCH_EINVAL naming the shape."""
    from jchemo_hip.plsavg import _avg_engine
    X, Y, Xq = local_data(120, 130, 3)
    obj = J.lwplsravg(X, Y, k=30, nlv="3:12", ctx=ctx, **LOCAL)
    pred, pred_lv, wlv, rr, rb, info, ind, dist, w = J.lwplsravg_prepared_call(_avg_engine(obj, 12), Xq, 30, 3, 12, 0, ctx)
    acc = pred_lv[:, 0, :].copy()
    for a in range(1, 10):
        acc += pred_lv[:, a, :]
    assert pred_lv.shape == (20, 10, 3) and np.array_equal(pred, acc / 10) and np.allclose(wlv, 0.1, rtol=1e-15) and not info.any()
    assert np.max(np.abs(pred - J.predict(obj, Xq, ctx=ctx).pred)) <= 1e-13 * np.max(np.abs(Y))
    X1, Y1, Xq1 = local_data(120, 130, 1)
    out = J.lwplsravg_prepared_call(_avg_engine(J.lwplsravg(X1, Y1, k=30, nlv="5:60", typf="shenk", ctx=ctx, **LOCAL), 30), Xq1, 30, 5, 60, 1, ctx)
    assert out[1].shape == (20, 26, 1) and out[2].shape == (20, 26) and out[3].shape == (20, 30)
    Xw, Yw, Xqw = local_data(80, 2100, 1, m=3)
    with pytest.raises(J.JchError, match="k = 30, p = 2100, q = 1, nlv = 4"):
        J.lwplsravg_prepared_call(_avg_engine(J.lwplsravg(Xw, Yw, k=30, nlv="1:4", typf="shenk", ctx=ctx, **LOCAL), 4), Xqw, 30, 1, 4, 1, ctx)


def test_local_shenk_info_flags(J, ctx):
    """info = 1: a constant univariate y in the neighbourhood — pred is that value, the wlv and rss rows are NaN.  info = 2: a query equal to the
    (weighted) mean of a neighbourhood of duplicates — the local X is constant, a Shenk norm is not finite, pred is NaN as the reference's arithmetic
    gives, and the mirror raises ONE warning."""
    X, Y, Xq = local_data(300, 40, 1)
    raw = dict(nlvdis=0, metric="eucl", h=2.0)
    listnn, _, _ = R.np_local_lists(X, Y, Xq, k=40, **raw)
    Y = Y.copy(order="F"); Y[listnn[0], 0] = 3.25
    res = J.predict(J.lwplsravg(X, Y, k=40, nlv="1:8", typf="shenk", ctx=ctx, **raw), Xq, ctx=ctx)
    assert res.info[0] == 1 and res.pred[0, 0] == 3.25 and np.all(np.isnan(res.wlv[0])) and np.all(np.isnan(res.rss_r[0])) and np.all(np.isnan(res.rss_b[0]))
    assert not res.info[1:].any() and np.all(np.isfinite(res.pred[1:]))
    rng = np.random.default_rng(4)
    X2 = np.asfortranarray(rng.standard_normal((100, 10)))
    X2[:20] = 50.0 + np.arange(10)                                           # 20 identical rows far from the rest
    Y2 = np.asfortranarray(rng.standard_normal((100, 1)))
    Xq2 = np.asfortranarray(np.vstack([X2[0], rng.standard_normal((2, 10))]))
    with pytest.warns(RuntimeWarning) as rec:
        res2 = J.predict(J.lwplsravg(X2, Y2, k=20, nlv="1:3", typf="shenk", ctx=ctx, **raw), Xq2, ctx=ctx)
    assert len([r for r in rec if "Shenk norm" in str(r.message)]) == 1
    assert sorted(res2.listnn[0].tolist()) == list(range(20))
    assert res2.info.tolist() == [2, 0, 0] and np.all(np.isnan(res2.pred[0])) and np.all(np.isfinite(res2.pred[1:]))
