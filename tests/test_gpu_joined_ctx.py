"""Every entry on a ctx JOINED to a communicator (include/jchemo_hip.h, "joined ctx contract").  From jch_ctx_comm_init (here: the loopback
group, ranks = threads of this process, one ctx each) on, ctx->nranks > 1 and everything that reaches jch_allreduce_f64 is a collective.  The table below puts
every exported entry in one class; tests/test_joined_ctx_static.py holds it against the header.

  C  collective   three loopback ranks make the same call on their own rows: per-row outputs per shard, everything else byte-equal on all ranks and equal to
                  the result on the concatenated rows -- the fits against the oracle at the project's sharded gate (rel. Frobenius < 1e-8 after sign_align:
                  DESIGN.md, test_row_sharded_fit_matches_unsharded), the primitives inside the per-element bounds of test_accessors_static.
  L  rank-local   two ranks with DIFFERENT data of equal shape: the bytes of the same call on a fresh ctx without a communicator, which is also held to the
                  family's own reference; then one jch_col_stats on the same ctxs gives the class-C answer (the communicator is still there).
  R  refused      two ranks, valid small arguments (the same call returns 0 on an unjoined ctx): JCH_EINVAL, "one rank only" in jch_last_error, outputs
                  untouched, inputs unchanged, and a following jch_col_stats gives the class-C answer.
  M  management   exempt.

Every rank makes the same sequence of calls with the same shapes, so a stray collective in a class-L entry shows as wrong numbers, never as ranks waiting
for each other: q = 2 (no constant-y shortcut), two classes present in every neighbourhood (no unanimous one).  A rank thread that is still alive after 30 s
fails its test and every later test of this file is skipped with that reason.

Where the table departs from what one might expect:
  jch_lwplsravg_predict_prepared   has no per-query loop in the library (outside the p-space envelope it is JCH_EINVAL); the loop is the Python mirror's
                                   (plsavg.lwplsravg_predict), which calls class-C entries per query and therefore refuses a joined ctx.
  plskern variant 1, q = 17        JCH_EINVAL on every rank (algorithm #2 needs q <= 16): asserted as such in the generic-q case.
  R of plsnipals / plsrosa / plswold in the global-clamp case: no reference (test_joined_ctx_static.R_HAS_NO_REFERENCE); T, P, W, C, TT are compared.
"""
import ctypes as C
import os
import sys
import threading
from functools import lru_cache

import numpy as np
import pytest

CLASSES = {
    "C": ["jch_plskern_fit", "jch_plsnipals_fit", "jch_plssimp_fit", "jch_plsrosa_fit", "jch_plswold_fit", "jch_plskern_fit_scaled", "jch_col_stats",
          "jch_weighted_ss", "jch_weighted_cov", "jch_score_sums", "jch_score_sums_lv", "jch_ctx_allreduce_probe"],
    "L": ["jch_affine_gemm", "jch_transform", "jch_predict", "jch_rows_standardize", "jch_rows_project_out", "jch_rows_fir", "jch_row_resid_ss",
          "jch_row_resid_ss_lv", "jch_fill_uniform", "jch_chol_factor", "jch_chol_solve", "jch_chol_inv_fro2", "jch_kc_panel", "jch_covsel_pass",
          "jch_lwplsr_predict", "jch_lwplsr_prepare", "jch_lwplsr_predict_prepared", "jch_lwplsr_release", "jch_lwplsr_add_query_map", "jch_knn_prepare",
          "jch_knn_release", "jch_knn_search", "jch_knn_wmean", "jch_knn_vote", "jch_knn_gather_median", "jch_knn_wls", "jch_knn_gda",
          "jch_lwplsda_predict_prepared", "jch_lwplsravg_predict_prepared", "jch_kde_dens"],
    "R": ["jch_kernel_gram", "jch_dkplsr_fit", "jch_dkplsr_transform", "jch_dkplsr_predict", "jch_kplsr_fit", "jch_kplsr_transform", "jch_kplsr_predict",
          "jch_kpca_fit", "jch_krr_fit", "jch_krr_solve", "jch_covsel_fit", "jch_xtdx", "jch_pca_fit", "jch_pcasph_fit", "jch_col_median_mad", "jch_stah",
          "jch_weiszfeld_step", "jch_spatial_median", "jch_farthest_pair", "jch_maxmin_select", "jch_class_cov", "jch_gauss_factor", "jch_mahsq_chol",
          "jch_perm_fill", "jch_perm_score_sums"],
    "M": ["jch_version", "jch_ctx_create", "jch_ctx_destroy", "jch_last_error", "jch_comm_unique_id", "jch_ctx_comm_init", "jch_ctx_comm_info",
          "jch_ctx_p2p_export", "jch_ctx_p2p_import", "jch_ctx_p2p_enable", "jch_loopback_group_create", "jch_loopback_group_destroy",
          "jch_ctx_comm_init_loopback", "jch_ctx_set_profiling", "jch_ctx_get_profile", "jch_ctx_synchronize", "jch_ctx_get_counter"],
}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "jchemo.jl_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import jchemo_hip as J  # noqa: E402
from jchemo_hip import _lib  # noqa: E402
from oracle import plsr_oracle as O  # noqa: E402

import plsavg_restate as RAVG  # noqa: E402
import test_accessors_static as S  # noqa: E402
import test_gpu_preproc as TPRE  # noqa: E402
import test_joined_ctx_static as SJ  # noqa: E402
import test_kde_static as SKDE  # noqa: E402
import test_knn_static as SKNN  # noqa: E402
import test_lwmlr_static as SMLR  # noqa: E402
import test_lwplsda_static as SDA  # noqa: E402
import test_occ_static as SOCC  # noqa: E402
import test_preproc_static as SPRE  # noqa: E402
from host_routes import HM, HN, HostMat  # noqa: E402
from test_accessors_static import LD  # noqa: E402
from test_gpu_accessors import Dev  # noqa: E402

NAN = float("nan")
EPS = float(np.finfo(np.float64).eps)
EINVAL = _lib.JCH_EINVAL
TOL = 1e-8                       # the project's sharded gate (test_row_sharded_fit_matches_unsharded)
WORST = {}                       # class-C primitive -> worst err / bound seen (reported in DESIGN.md 29, asserted only against 1)
STUCK = []                       # the reason, once a rank thread did not come back


@pytest.fixture(autouse=True)
def _nothing_runs_behind_a_stuck_rank():
    if STUCK:
        pytest.skip(STUCK[0])
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ---------------------------------------------------------------------------------------------------- the runner
def run_ranks(nr, fn):
    """One thread and one J.Context(0) per rank, joined to a loopback group of nr; fn(rank, ctx) makes the calls (the same sequence on every rank) and
    its return values come back in rank order.  Buffers are made by the caller beforehand: the threads only call the library."""
    L = J.load()
    grp = C.c_void_p()
    assert L.jch_loopback_group_create(nr, C.byref(grp)) == 0
    ctxs = [J.Context(0) for _ in range(nr)]
    out, err = [None] * nr, [None] * nr
    torch.cuda.synchronize()

    def work(r):
        try:
            ctxs[r].comm_init_loopback(grp, r, nr)
            out[r] = fn(r, ctxs[r])
        except BaseException as e:  # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(nr)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=30)
    if any(t.is_alive() for t in th):
        STUCK.append("a rank thread of an earlier test is still inside a collective: the ctxs and the GPU queue behind it cannot be trusted (errors so far: %r)" % (err,))
        pytest.fail(STUCK[0])
    for c in ctxs:
        c.close()
    L.jch_loopback_group_destroy(grp)
    for e in err:
        if e is not None:
            raise e
    return out


def nanv(n):
    """A host output of n doubles with one more behind it that must stay NaN."""
    return np.full(n + 1, NAN)


def body(v):
    assert np.isnan(v[-1]), "the double behind a host output was written"
    return v[:-1]


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def vptr(v):
    return None if v is None else (v.ptr if hasattr(v, "ptr") else v.ctypes.data)


def mat(loc, A=None, **kw):
    return Dev(A, **kw) if loc else HostMat(A, **kw)


def unchanged(m_):
    """Dev / HostMat input: padding and guards still NaN, the matrix as it was (NaN entries of an unselected row included)."""
    assert np.array_equal(m_.get(), m_.src, equal_nan=True), "an input was modified"


def check_bound(prim, name, got, ref, bound):
    got, bound = np.asarray(got), np.asarray(bound, dtype=np.float64)
    assert got.shape == np.shape(ref) == bound.shape, (name, got.shape, np.shape(ref), bound.shape)
    assert np.isfinite(got).all(), f"{name}: not finite"
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    pos = bound > 0.0
    ratio = float(np.max(np.where(pos, err / np.where(pos, bound, 1.0), np.where(err > 0.0, np.inf, 0.0)))) if err.size else 0.0
    print(f"  {name}: max err / bound {ratio:.3f}")
    WORST[prim] = max(WORST.get(prim, 0.0), ratio)
    assert np.all(err <= bound), f"{name}: err / bound {ratio:.3f}"


# ==================================================================================================== class C: the fits
ENTRY = dict(plskern="jch_plskern_fit", plskern_v1="jch_plskern_fit", plsnipals="jch_plsnipals_fit", plssimp="jch_plssimp_fit", plsrosa="jch_plsrosa_fit",
             plswold="jch_plswold_fit")
ONE_PASS, REUSE_XCOPY, WOLD_NAN = 4, 8, 2
SQRT_EPS = float(np.sqrt(np.finfo(float).eps))


class FitRank:
    """The buffers of one rank's fit, every one NaN-prefilled with padding and guards (Dev / HostMat), and the call through the C ABI."""

    def __init__(self, loc, X, Y, w, nlv):
        n, p = X.shape
        q = Y.shape[1]
        self.loc, self.n, self.p, self.q, self.kmax = loc, n, p, q, max(1, min(p, nlv))
        pad = 1 if loc else 3
        self.X, self.Y = mat(loc, X, ld=n + pad), mat(loc, Y, ld=n + 2 * pad)
        self.w = None if w is None else (Dev(w) if loc else np.array(w, dtype=np.float64))
        self.w0 = None if w is None else np.array(w, dtype=np.float64)
        self.T, self.wn = mat(loc, rows=n, cols=self.kmax + 1), mat(loc, rows=n, cols=2)
        k = self.kmax
        self.h = {f: nanv(sz) for f, sz in dict(P=p * k, R=p * k, W=p * k, C=q * k, TT=k, xm=p, xs=p, ym=q, ys=q, niter=k).items()}
        self.got, self.status, self.msg = C.c_int32(-1), None, b""

    def call(self, L, ctx, alg, nlv, reserved=0, scaled=None, scal=0):
        h = self.h
        desc = _lib.PlsDesc(self.n, self.p, self.q, nlv, int(scal), _lib.F64, self.loc, 0, reserved | (1 if alg == "plskern_v1" else 0))
        head = [ctx._h, C.byref(desc), self.X.ptr, self.X.ld, self.Y.ptr, self.Y.ld, vptr(self.w)]
        outs = [self.T.ptr] + [h[f].ctypes.data for f in ("P", "R", "W", "C", "TT", "xm", "xs", "ym", "ys")] + [self.wn.ptr]
        if scaled is not None:
            st = L.jch_plskern_fit_scaled(*head, scaled[0].ctypes.data, scaled[1].ctypes.data, *outs, C.byref(self.got))
        elif alg == "plswold":
            st = L.jch_plswold_fit(*head, SQRT_EPS, 200, *outs, h["niter"].ctypes.data, C.byref(self.got))
        else:
            st = getattr(L, ENTRY[alg])(*head, *outs, C.byref(self.got))
        self.status, self.msg = st, (L.jch_last_error(ctx._h) or b"")
        return st

    def result(self):
        """The outputs, after checking that everything beyond them is still NaN and that X, Y and the weights are as they were."""
        k, kmax, p, q, h = self.got.value, self.kmax, self.p, self.q, self.h
        assert 0 <= k <= kmax
        T = self.T.get(kmax)
        assert np.isnan(T[:, k:]).all(), "a score column beyond nlv_out was written"
        out = dict(k=k, T=T[:, :k], weights=self.wn.get(1)[:, 0])
        for f, rows in (("P", p), ("R", p), ("W", p), ("C", q), ("TT", 1), ("niter", 1)):
            a = body(h[f])
            assert np.isnan(a[rows * k:]).all(), f"{f}: written beyond nlv_out columns"
            out[f] = a[:rows * k].reshape(k, rows).T.copy() if rows > 1 or f in ("P", "R", "W", "C") else a[:k].copy()
        for f, g in (("xm", "xmeans"), ("xs", "xscales"), ("ym", "ymeans"), ("ys", "yscales")):
            out[g] = body(h[f]).copy()
        unchanged(self.X); unchanged(self.Y)
        if self.w is not None:
            assert np.array_equal(self.w.get()[:, 0] if self.loc else self.w, self.w0), "the weights were modified"
        return out


def sharded_fit(case, alg, loc=0, reserved=0, calls=1, scaled=None, Y=None, w=None, scal=0):
    """The fit of one case on its loopback ranks; calls > 1 repeats it on the same joined ctxs with fresh outputs: [call][rank] FitRank."""
    X, Y0, w0, edges = SJ.fit_data(case)
    Y, w = (Y0 if Y is None else Y), (w0 if w is None else w)
    rows, p, q, nlv, _ = SJ.FIT_CASES[case]
    reserved = reserved if isinstance(reserved, (list, tuple)) else [reserved] * calls
    first = [FitRank(loc, X[a:b], Y[a:b], w[a:b], nlv) for a, b in zip(edges[:-1], edges[1:])]
    runs = [first]
    for _ in range(1, calls):                               # the same X, Y and weights (the same pointers: JCH_REUSE_XCOPY's promise), new outputs
        nxt = [FitRank(loc, X[a:b][:1], Y[a:b][:1], None, nlv) for a, b in zip(edges[:-1], edges[1:])]
        for f, g in zip(first, nxt):
            g.n, g.X, g.Y, g.w, g.w0 = f.n, f.X, f.Y, f.w, f.w0
            g.T, g.wn = mat(loc, rows=f.n, cols=f.kmax + 1), mat(loc, rows=f.n, cols=2)
        runs.append(nxt)
    L = J.load()

    def fn(r, ctx):
        cnt = []
        for i, ranks in enumerate(runs):
            ranks[r].call(L, ctx, alg, nlv, reserved[i], scaled, scal)
            cnt.append(ctx.counter(_lib.COUNTER_XCOPY_REUSED))
        return cnt

    counters = run_ranks(len(rows), fn)
    return runs, counters


def check_replicated(res):
    for f in ("P", "R", "W", "C", "TT", "xmeans", "xscales", "ymeans", "yscales", "niter", "k"):
        for r in res[1:]:
            assert same_bytes(res[0][f], r[f]), f"{f} differs between the ranks"


def check_against(ref, res, X, w, alg, kc, skip_R=False, tol=TOL, what=""):
    """Sign-aligned relative Frobenius errors of the concatenated scores and rank 0's model against `ref` on the first kc LVs."""
    T = np.concatenate([r["T"] for r in res], axis=0)[:, :kc]
    wn = np.concatenate([r["weights"] for r in res])
    key = "W" if skip_R else "R"
    s = O.sign_align(getattr(ref, key)[:, :kc], res[0][key][:, :kc])
    Tref = np.array(ref.T[:, :kc])
    zero = np.asarray(w) == 0.0
    if alg == "plswold" and zero.any():                      # the reference divides by sqrt(w) = 0 there; the library's default is t_i = x_i' r (header)
        Tref[zero] = (((X - ref.xmeans) / ref.xscales) @ ref.R[:, :kc])[zero]
    errs = {"T": O.rel_fro(Tref, T * s), "weights": O.rel_fro(ref.weights, wn)}
    for f in ("P", "R", "W", "C"):
        if not (f == "R" and skip_R):
            errs[f] = O.rel_fro(getattr(ref, f)[:, :kc], res[0][f][:, :kc] * s)
    errs["TT"] = O.rel_fro(ref.TT[:kc], res[0]["TT"][:kc])
    for f in ("xmeans", "xscales", "ymeans", "yscales"):
        errs[f] = O.rel_fro(getattr(ref, f), res[0][f])
    print(f"  {what}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if not v < tol}
    assert not bad, (what, bad)


FIT_PARAMS = [(case, alg, loc) for case, (_, _, _, _, algs) in SJ.FIT_CASES.items() for alg in algs for loc in ((0, 1) if case == "small-shard" else (0,))]


@pytest.mark.parametrize("case,alg,loc", FIT_PARAMS, ids=["%s-%s-%s" % (c, a, "device" if l else "host") for c, a, l in FIT_PARAMS])
def test_fit_on_three_ranks_equals_the_oracle_on_the_concatenated_rows(case, alg, loc):
    rows, p, q, nlv, _ = SJ.FIT_CASES[case]
    X, Y, w, edges = SJ.fit_data(case)
    scal = loc == 1 or case == "generic-q"                   # the column scales (a second all-reduced moment pass, or the raw mode's own) on two of the cases
    (ranks,), _ = sharded_fit(case, alg, loc, scal=scal)
    if alg == "plskern_v1" and (q > 16 or p > 2048):         # algorithm #2 does not take this shape: the same refusal on every rank
        assert all(r.status == EINVAL and b"variant 2" in r.msg for r in ranks), [(r.status, r.msg) for r in ranks]
        return
    assert all(r.status == 0 for r in ranks), [(r.status, r.msg) for r in ranks]
    res = [r.result() for r in ranks]
    k = min(sum(rows), p, nlv)
    assert all(r["k"] == k for r in res), ("nlv_out", [r["k"] for r in res], k)
    check_replicated(res)
    assert all(np.isfinite(r["T"]).all() for r in res), "scores not finite"
    ref = SJ.oracle_fit(alg, X, Y, w, nlv, scal)
    kc = SJ.CLAMP_COMPARED if case == "global-clamp" else k
    check_against(ref, res, X, w, alg, kc, skip_R=(case, alg) in SJ.R_HAS_NO_REFERENCE, what=f"{case} {alg} loc {loc}")
    if alg == "plswold":
        assert np.array_equal(ref.niter[:kc], res[0]["niter"][:kc]), (ref.niter, res[0]["niter"])
    if alg == "plssimp":
        assert same_bytes(res[0]["W"], res[0]["R"])


def test_plswold_zero_weight_shard_gives_nan_scores_only_under_the_reference_bit():
    """JCH_WOLD_REF_ZERO_WEIGHT_NAN on the zero-weight-shard case: every score of rank 1 is NaN, the other ranks' scores and the model are the oracle's."""
    case, alg = "zero-weight-shard", "plswold"
    rows, p, q, nlv, _ = SJ.FIT_CASES[case]
    X, Y, w, edges = SJ.fit_data(case)
    (ranks,), _ = sharded_fit(case, alg, 0, reserved=WOLD_NAN)
    assert all(r.status == 0 for r in ranks), [(r.status, r.msg) for r in ranks]
    res = [r.result() for r in ranks]
    check_replicated(res)
    assert np.isnan(res[1]["T"]).all() and np.isfinite(res[0]["T"]).all() and np.isfinite(res[2]["T"]).all()
    ref = SJ.oracle_fit(alg, X, Y, w, nlv)
    assert np.array_equal(np.isnan(ref.T).all(axis=1), w == 0.0)
    keep = w > 0.0
    T = np.concatenate([r["T"] for r in res], axis=0)
    s = O.sign_align(ref.R, res[0]["R"])
    assert O.rel_fro(ref.T[keep], T[keep] * s) < TOL
    for f in ("P", "R", "W", "C"):
        assert O.rel_fro(getattr(ref, f), res[0][f] * s) < TOL, f


def test_plskern_fit_scaled_on_three_ranks():
    """Caller-supplied divisors on the small-shard case: the oracle's plskern on X ./ xdiv, Y ./ ydiv (centring commutes with the division)."""
    case = "small-shard"
    rows, p, q, nlv, _ = SJ.FIT_CASES[case]
    X, Y, w, edges = SJ.fit_data(case)
    rng = np.random.default_rng(3)
    xdiv, ydiv = rng.uniform(0.5, 2.0, p), rng.uniform(0.5, 2.0, q)
    (ranks,), _ = sharded_fit(case, "plskern", 0, scaled=(xdiv, ydiv))
    assert all(r.status == 0 for r in ranks), [(r.status, r.msg) for r in ranks]
    res = [r.result() for r in ranks]
    check_replicated(res)
    ref = O.plskern(X / xdiv, Y / ydiv, w, nlv=nlv)
    assert same_bytes(res[0]["xscales"], xdiv) and same_bytes(res[0]["yscales"], ydiv)
    ref.xmeans, ref.ymeans, ref.xscales, ref.yscales = ref.xmeans * xdiv, ref.ymeans * ydiv, xdiv, ydiv
    check_against(ref, res, X, w, "plskern", nlv, what="plskern_fit_scaled")


@pytest.mark.parametrize("alg", ["plsnipals", "plswold"])
def test_one_pass_on_three_ranks_equals_the_sharded_default_path(alg):
    """JCH_NIPALS_ONE_PASS on the small-shard case at its documented 1e-9 against the default path, both sharded; and against the oracle at the gate."""
    case = "small-shard"
    rows, p, q, nlv, _ = SJ.FIT_CASES[case]
    X, Y, w, edges = SJ.fit_data(case)
    (a,), _ = sharded_fit(case, alg, 0)
    (b,), _ = sharded_fit(case, alg, 0, reserved=ONE_PASS)
    assert all(r.status == 0 for r in a + b), [(r.status, r.msg) for r in a + b]
    ra, rb = [r.result() for r in a], [r.result() for r in b]
    check_replicated(rb)
    s = O.sign_align(ra[0]["W"], rb[0]["W"])
    errs = {f: O.rel_fro(ra[0][f], rb[0][f] * s) for f in ("P", "R", "W", "C")}
    errs["T"] = O.rel_fro(np.concatenate([r["T"] for r in ra]), np.concatenate([r["T"] for r in rb]) * s)
    errs["TT"] = O.rel_fro(ra[0]["TT"], rb[0]["TT"])
    print(f"  one pass against the default path ({alg}): " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert all(v < 1e-9 for v in errs.values()), errs
    check_against(SJ.oracle_fit(alg, X, Y, w, nlv), rb, X, w, alg, nlv, what=f"one pass {alg}")


@pytest.mark.parametrize("loc", [0, 1], ids=["host", "device"])
def test_a_second_fit_with_reuse_xcopy_on_the_same_joined_ctx(loc):
    """plskern twice on the same joined ctxs, the second time with JCH_REUSE_XCOPY (the same X, Y and weights pointers): the bit is honoured (the counter
    says on which ranks) and the result is the oracle's; both fits byte-equal across the ranks."""
    case = "small-shard"
    rows, p, q, nlv, _ = SJ.FIT_CASES[case]
    X, Y, w, edges = SJ.fit_data(case)
    (a, b), counters = sharded_fit(case, "plskern", loc, reserved=[0, REUSE_XCOPY], calls=2)
    assert all(r.status == 0 for r in a + b), [(r.status, r.msg) for r in a + b]
    print(f"  JCH_COUNTER_XCOPY_REUSED after the two fits, per rank: {counters}")
    assert all(c[0] == 0 for c in counters) and max(c[1] for c in counters) == 1, counters
    ref = SJ.oracle_fit("plskern", X, Y, w, nlv)
    for ranks, what in ((a, "first fit"), (b, "second fit, reuse")):
        res = [r.result() for r in ranks]
        check_replicated(res)
        check_against(ref, res, X, w, "plskern", nlv, what=what)


# ==================================================================================================== class C: the primitives
def _vec(loc, v):
    return None if v is None else (Dev(v) if loc else np.array(v, dtype=np.float64))


def _prim_ranks(arrays, vectors):
    """Per rank and route (loc 0: host, ld = rows + 3; loc 1: device, ld = rows + 1) the shard of every matrix and vector."""
    out = []
    for r in range(len(SJ.SPLIT)):
        a, b = SJ.EDGES[r], SJ.EDGES[r + 1]
        out.append([dict(mats=[None if A is None else mat(loc, A[a:b], ld=(b - a) + (1 if loc else 3)) for A in arrays],
                         vecs=[_vec(loc, None if v is None else v[a:b]) for v in vectors], n=int(b - a)) for loc in (0, 1)])
    return out


def _prim_unchanged(ranks, arrays, vectors):
    for r, per_loc in enumerate(ranks):
        a, b = SJ.EDGES[r], SJ.EDGES[r + 1]
        for loc, bufs in enumerate(per_loc):
            for m_ in bufs["mats"]:
                if m_ is not None:
                    unchanged(m_)
            for v, src in zip(bufs["vecs"], vectors):
                if v is not None:
                    assert np.array_equal(v.get()[:, 0] if loc else v, src[a:b], equal_nan=True), "a vector input was modified"


def _all_ranks_equal(outs):
    """outs[rank] = list of output arrays (status first): every status 0, every array byte-equal to rank 0's; returns rank 0's arrays."""
    for o in outs:
        assert o[0] == [0] * len(o[0]), ("status", o[0])
    for o in outs[1:]:
        for i, (x, y) in enumerate(zip(outs[0][1:], o[1:])):
            assert same_bytes(x, y), f"output {i} differs between the ranks"
    return outs[0][1:]


@pytest.mark.parametrize("case", SJ.STATS_CASES, ids=lambda c: "p%d-level%g-w_%s" % c)
def test_col_stats_and_weighted_ss_on_three_ranks(case):
    p, level, wkind = case
    X, w = S.stats_data(SJ.N, p, level, wkind)
    d = np.ones(SJ.N) / SJ.N if w is None else w / w.sum()
    mean, std = S.ref_col_stats(X, w)
    shift, scale = np.asarray(mean, dtype=np.float64), np.random.default_rng(SJ.N + p).uniform(0.5, 2.0, p)
    ranks = _prim_ranks([X], [w, d])
    L = J.load()

    def fn(r, ctx):
        st, res = [], []
        for loc in (0, 1):
            b = ranks[r][loc]
            x, wv, dv, n = b["mats"][0], b["vecs"][0], b["vecs"][1], b["n"]
            mo, so, m2, s1, s2 = nanv(p), nanv(p), nanv(p), nanv(1), nanv(1)
            st.append(L.jch_col_stats(ctx._h, loc, x.ptr, n, p, x.ld, vptr(wv), mo.ctypes.data, so.ctypes.data))
            st.append(L.jch_col_stats(ctx._h, loc, x.ptr, n, p, x.ld, vptr(wv), m2.ctypes.data, None))
            st.append(L.jch_weighted_ss(ctx._h, loc, x.ptr, n, p, x.ld, vptr(dv), shift.ctypes.data, scale.ctypes.data, s1.ctypes.data_as(C.POINTER(C.c_double))))
            st.append(L.jch_weighted_ss(ctx._h, loc, x.ptr, n, p, x.ld, vptr(dv), None, None, s2.ctypes.data_as(C.POINTER(C.c_double))))
            res += [mo, so, m2, s1, s2]
        return [st] + res

    got = _all_ranks_equal(run_ranks(3, fn))
    _prim_unchanged(ranks, [X], [w, d])
    bm, bs = S.bound_means(X, w), S.bound_stds(X, w)
    for loc, name in ((0, "host"), (1, "device")):
        mo, so, m2, s1, s2 = (body(v) for v in got[5 * loc:5 * loc + 5])
        assert same_bytes(mo, m2), "stds = NULL changes the means"
        check_bound("jch_col_stats", f"means ({name})", mo, mean, bm)
        check_bound("jch_col_stats", f"stds ({name})", so, std, bs)
        for v, sh, sc in ((s1, shift, scale), (s2, None, None)):
            check_bound("jch_weighted_ss", f"sstot ({name})", v, np.array([S.ref_weighted_ss(X, d, sh, sc)], dtype=LD), np.array([S.bound_weighted_ss(X, d, sh, sc)]))


@pytest.mark.parametrize("case", SJ.COV_CASES, ids=lambda c: "d%d-level%g-w_%s" % c)
def test_weighted_cov_on_three_ranks(case):
    d_, level, wkind = case
    A, w = S.cov_data(SJ.N, d_, level, wkind)
    ranks = _prim_ranks([A], [w])
    L = J.load()

    def fn(r, ctx):
        st, res = [], []
        for loc in (0, 1):
            b = ranks[r][loc]
            a, wv, n = b["mats"][0], b["vecs"][0], b["n"]
            So, mo, S2 = nanv(d_ * d_), nanv(d_), nanv(d_ * d_)
            st.append(L.jch_weighted_cov(ctx._h, loc, a.ptr, n, d_, a.ld, vptr(wv), So.ctypes.data, mo.ctypes.data))
            st.append(L.jch_weighted_cov(ctx._h, loc, a.ptr, n, d_, a.ld, vptr(wv), S2.ctypes.data, None))
            res += [So, mo, S2]
        return [st] + res

    got = _all_ranks_equal(run_ranks(3, fn))
    _prim_unchanged(ranks, [A], [w])
    Sref, mu = S.ref_weighted_cov(A, w)
    b, bm = S.bound_weighted_cov(A, w), S.bound_means(A, w)
    for loc, name in ((0, "host"), (1, "device")):
        So, mo, S2 = (body(v) for v in got[3 * loc:3 * loc + 3])
        assert same_bytes(So, S2), "mu = NULL changes S"
        Sg = So.reshape(d_, d_).T
        check_bound("jch_weighted_cov", f"mu ({name})", mo, mu, bm)
        check_bound("jch_weighted_cov", f"S ({name})", Sg, Sref, b)
        check_bound("jch_weighted_cov", f"S - S' ({name})", Sg - Sg.T, np.zeros((d_, d_), dtype=LD), 2.0 * b)


def _check_sums(prim, name, got, ref, bound, m_sel):
    assert np.all(got[:, 5] == m_sel), f"{name}: the row count is not exact"
    check_bound(prim, name, got, ref, bound)


@pytest.mark.parametrize("case", SJ.SCORE_CASES, ids=lambda c: "q%d-levels%d-mask_%s" % c)
def test_score_sums_on_three_ranks(case):
    q, levels, mkind = case
    Pred, Y, mask = SJ.score_case(q, levels, mkind)
    ncol = levels * q
    ranks = _prim_ranks([Pred, Y], [mask])
    L = J.load()

    def fn(r, ctx):
        st, res = [], []
        for loc in (0, 1):
            b = ranks[r][loc]
            pr, y, mk, n = b["mats"][0], b["mats"][1], b["vecs"][0], b["n"]
            out = nanv(ncol * 6)
            st.append(L.jch_score_sums(ctx._h, loc, pr.ptr, n, ncol, pr.ld, y.ptr, q, y.ld, vptr(mk), out.ctypes.data))
            res.append(out)
        return [st] + res

    got = _all_ranks_equal(run_ranks(3, fn))
    _prim_unchanged(ranks, [Pred, Y], [mask])
    ref, A = S.ref_score_sums(Pred, Y, mask)
    m_sel = SJ.N if mask is None else int(np.count_nonzero(mask))
    if mask is not None:
        assert not np.any(mask[:SJ.SPLIT[0]]) and m_sel > 0            # rank 0 selects nothing
    for loc, name in ((0, "host"), (1, "device")):
        _check_sums("jch_score_sums", f"sums ({name})", body(got[loc]).reshape(ncol, 6), ref, S.bound_score_sums(A, m_sel), m_sel)


@pytest.mark.parametrize("case", SJ.SCORE_LV_CASES, ids=lambda c: "q%d-kfit%d-mask_%s" % c)
def test_score_sums_lv_on_three_ranks(case):
    q, kfit, mkind = case
    T, Cm, ym, ys, Y, mask = SJ.score_lv_case(q, kfit, mkind)
    ym, ys, Cm = np.ascontiguousarray(ym), np.ascontiguousarray(ys), np.asfortranarray(Cm)
    ranges = [(0, kfit), (kfit, kfit + 2)]
    ranks = _prim_ranks([T, Y], [mask])
    L = J.load()

    def fn(r, ctx):
        st, res = [], []
        for loc in (0, 1):
            b = ranks[r][loc]
            t, y, mk, n = b["mats"][0], b["mats"][1], b["vecs"][0], b["n"]
            for lo, hi in ranges:
                out = nanv((hi - lo + 1) * q * 6)
                st.append(L.jch_score_sums_lv(ctx._h, loc, t.ptr, n, kfit, t.ld, Cm.ctypes.data, ym.ctypes.data, ys.ctypes.data, y.ptr, q, y.ld, vptr(mk), lo, hi,
                                              out.ctypes.data))
                res.append(out)
        return [st] + res

    got = _all_ranks_equal(run_ranks(3, fn))
    _prim_unchanged(ranks, [T, Y], [mask])
    m_sel = SJ.N if mask is None else int(np.count_nonzero(mask))
    for loc, name in ((0, "host"), (1, "device")):
        for i, (lo, hi) in enumerate(ranges):
            ref, bound = S.ref_score_sums_lv(T, Cm, ym, ys, Y, mask, lo, hi)
            _check_sums("jch_score_sums_lv", f"levels {lo}..{hi} ({name})", body(got[2 * loc + i]).reshape(-1, 6), ref, bound, m_sel)


def test_allreduce_probe_counts_the_ranks():
    L = J.load()

    def fn(r, ctx):
        v, us = np.ones(5), C.c_double(-1.0)
        st = L.jch_ctx_allreduce_probe(ctx._h, _lib.TRANSPORT_LOOPBACK, v.ctypes.data, 5, 3, C.byref(us))
        return st, v, us.value

    for st, v, us in run_ranks(3, fn):
        assert st == 0 and np.array_equal(v, np.full(5, 3.0)) and us >= 0.0


# ---------------------------------------------------------------------------------------------------- the closing class-C call of the L and R tests
def _stats_after(nr=2):
    """The jch_col_stats call every rank makes after its class-L / class-R calls: (per-rank buffers, the call, the check of what came back)."""
    p = 37
    X, w = S.stats_data(100, p, 1e4, "random")
    edges = [0, 3, 100]
    bufs = [(HostMat(X[a:b], ld=(b - a) + 3), np.array(w[a:b])) for a, b in zip(edges[:-1], edges[1:])]

    def call(L, ctx, r):
        x, wv = bufs[r]
        mo, so = nanv(p), nanv(p)
        st = L.jch_col_stats(ctx._h, 0, x.ptr, x.rows, p, x.ld, wv.ctypes.data, mo.ctypes.data, so.ctypes.data)
        return st, mo, so

    def check(res):
        mean, std = S.ref_col_stats(X, w)
        assert all(r[0] == 0 for r in res), [r[0] for r in res]
        assert same_bytes(res[0][1], res[1][1]) and same_bytes(res[0][2], res[1][2]), "the closing jch_col_stats differs between the ranks"
        check_bound("jch_col_stats", "closing means", body(res[0][1]), mean, S.bound_means(X, w))
        check_bound("jch_col_stats", "closing stds", body(res[0][2]), std, S.bound_stds(X, w))

    return call, check


# ==================================================================================================== class L
K_NB, NLV_HI, H_W, TOL_W = 20, 2, 2.0, 1e-4


@lru_cache(maxsize=None)
def ldata(rank):
    """The data of one rank: 65 training rows, 67 queries, p = 5 (p = 3 where an entry needs fewer), q = 2, two classes that both occur in every
    neighbourhood of K_NB rows (the seed is advanced until they do: a unanimous neighbourhood is not fitted, and the ranks' call counts would differ)."""
    seed = 650367 + 1000 * rank
    while True:
        rng = np.random.default_rng(seed)
        X, Q = rng.standard_normal((HN, 5)), rng.standard_normal((HM, 5))
        Y = X[:, :2] * 1.5 + 0.3 * X[:, 2:4] ** 2 + 0.1 * rng.standard_normal((HN, 2))
        cls = (0.6 * X[:, 0] + 0.8 * rng.standard_normal(HN) > 0).astype(np.int32)
        ind, _ = O.getknn(X, Q, k=K_NB)
        cnt = cls[ind].sum(axis=1)
        if cnt.min() >= 3 and cnt.max() <= K_NB - 3:
            break
        seed += 1
    d = dict(X=X, Q=Q, Y=Y, cls=cls, X3=X[:, :3].copy(), Q3=Q[:, :3].copy(), Z2=rng.standard_normal((HM, 2)), B=np.asfortranarray(rng.standard_normal((3, 2))),
             shift=rng.standard_normal(3), scale=rng.uniform(0.5, 2.0, 3), bias=rng.standard_normal(2), Cm=np.asfortranarray(rng.standard_normal((2, 2))),
             ym=rng.standard_normal(2), ys=rng.uniform(0.5, 2.0, 2), seed=seed)
    M = rng.standard_normal((HN, HN))
    d["SPD"] = M @ M.T / HN + np.eye(HN)
    d["V"] = rng.standard_normal((HN, 3))
    T = rng.standard_normal((HM, K_NB, NLV_HI)) + (np.arange(K_NB) % 2)[None, :, None] * 1.5
    d["gdaT"], d["gdatq"], d["gdacls"] = T, rng.standard_normal((HM, NLV_HI)) + 0.7, np.tile((np.arange(K_NB) % 2).astype(np.int32), (HM, 1))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


class Route:
    """One rank's call sequence: `ins` collects the HostMat inputs (checked unchanged), `out` the named results, `st` every status."""

    def __init__(self, L, ctx, d):
        self.L, self.ctx, self.d, self.ins, self.out, self.st = L, ctx, d, [], {}, []

    def inp(self, A, ld_pad=3):
        m_ = HostMat(A, ld=len(A) + ld_pad)
        self.ins.append(m_)
        return m_

    def call(self, name, *args):
        st = getattr(self.L, name)(self.ctx._h, *args)
        self.st.append((name, st, (self.L.jch_last_error(self.ctx._h) or b"") if st else b""))
        return st


def r_accessors(t):
    d, L = t.d, t.L
    x = t.inp(d["Q3"])
    o1, o2, o3 = HostMat(rows=HM, cols=3, ld=HM + 3), HostMat(rows=HM, cols=3, ld=HM + 3), HostMat(rows=HM, cols=7, ld=HM + 3)
    sh, sc, bi, ym, ys = (np.array(d[k]) for k in ("shift", "scale", "bias", "ym", "ys"))
    t.call("jch_affine_gemm", 0, x.ptr, HM, 3, x.ld, sh.ctypes.data, sc.ctypes.data, d["B"].ctypes.data, 2, bi.ctypes.data, o1.ptr, o1.ld)
    t.call("jch_transform", 0, x.ptr, HM, 3, x.ld, sh.ctypes.data, sc.ctypes.data, d["B"].ctypes.data, 2, o2.ptr, o2.ld)
    t.call("jch_predict", 0, x.ptr, HM, 3, x.ld, sh.ctypes.data, sc.ctypes.data, ym.ctypes.data, ys.ctypes.data, d["B"].ctypes.data, d["Cm"].ctypes.data, 2, 0, 2,
           o3.ptr, o3.ld)
    t.out.update(affine=o1.get(2), transform=o2.get(2), predict=o3.get(6))


def c_accessors(d, o):
    X, sh, sc = d["Q3"], d["shift"], d["scale"]
    ref, f = S.ref_affine(X, sh, sc, d["B"], d["bias"])
    check_bound("L", "jch_affine_gemm", o["affine"], ref, S.bound_affine(X, sh, sc, d["B"], d["bias"], f))
    ref, f = S.ref_affine(X, sh, sc, d["B"], None)
    check_bound("L", "jch_transform", o["transform"], ref, S.bound_affine(X, sh, sc, d["B"], None, f))
    model = dict(xmeans=sh, xscales=sc, ymeans=d["ym"], yscales=d["ys"], R=d["B"], C=d["Cm"])
    check_bound("L", "jch_predict", o["predict"], S.ref_predict(X, model, 0, 2), S.bound_predict(X, model, 0, 2))


def r_rows(t):
    d = t.d
    x = t.inp(d["Q"])
    p = 5
    vX, A = SPRE.np_detrend_coef(p, 1)
    Af, Vf, taps = np.asfortranarray(A), np.asfortranarray(vX), np.full(3, 1.0 / 3)
    o = [HostMat(rows=HM, cols=p + 1, ld=HM + 3) for _ in range(3)]
    t.call("jch_rows_standardize", 0, x.ptr, HM, p, x.ld, 1, 1, o[0].ptr, o[0].ld)
    t.call("jch_rows_project_out", 0, x.ptr, HM, p, x.ld, Af.ctypes.data, Vf.ctypes.data, 2, o[1].ptr, o[1].ld)
    t.call("jch_rows_fir", 0, x.ptr, HM, p, x.ld, taps.ctypes.data, 3, -1, 0, o[2].ptr, o[2].ld)
    t.out.update(snv=o[0].get(p), detrend=o[1].get(p), mavg=o[2].get(p))


def c_rows(d, o):
    X = np.asfortranarray(d["Q"])
    ref = SPRE.np_snv(X, True, True)
    TPRE._check("snv", o["snv"], ref, TPRE._snv_bound(X, ref))
    ref = SPRE.np_detrend(X, 1)
    TPRE._check("detrend", o["detrend"], ref, TPRE._detrend_bound(X, ref, 1))
    TPRE._check("mavg", o["mavg"], SPRE.np_mavg(X, 3), TPRE._fir_bound(X, np.full(3, 1.0 / 3), -1, 5))


def r_resid(t):
    d = t.d
    x, z = t.inp(d["Q3"]), t.inp(d["Z2"])
    o1, o2 = HostMat(rows=HM, cols=2), HostMat(rows=HM, cols=4, ld=HM + 3)
    sh = np.array(d["shift"])
    t.call("jch_row_resid_ss", 0, x.ptr, HM, 3, x.ld, sh.ctypes.data, z.ptr, 2, z.ld, d["B"].ctypes.data, 3, o1.ptr)
    t.call("jch_row_resid_ss_lv", 0, x.ptr, HM, 3, x.ld, sh.ctypes.data, z.ptr, 2, z.ld, d["B"].ctypes.data, 3, 0, 2, o2.ptr, o2.ld)
    t.out.update(resid=o1.get(1), resid_lv=o2.get(3))


def c_resid(d, o):
    X, sh, Z, B = d["Q3"], d["shift"], d["Z2"], d["B"]
    check_bound("L", "jch_row_resid_ss", o["resid"][:, 0], SOCC.resid_ss_longdouble(X, sh, Z, B), np.asarray(SOCC.resid_ss_bound(X, sh, Z, B), dtype=np.float64))
    ref = RAVG.resid_ss_lv_longdouble(X, sh, Z, B, 0, 2)
    for a in range(3):
        check_bound("L", f"jch_row_resid_ss_lv level {a}", o["resid_lv"][:, a], ref[:, a], np.asarray(SOCC.resid_ss_bound(X, sh, Z[:, :a], B[:, :a]), dtype=np.float64))


KDE = dict(cs=np.array([0, 30, HN], dtype=np.int64), dims=np.array([2, 3], dtype=np.int32), u=np.asfortranarray(np.full((3, 2), 0.7)),
           v2=np.asfortranarray(np.array([[1.0, 0.8], [1.2, 0.9]])), coef=np.asfortranarray(np.array([[0.5, 0.4], [0.3, 0.2]])))


def r_kde(t):
    d = t.d
    z, q = t.inp(d["X3"]), t.inp(d["Q3"])
    o = HostMat(rows=HM, cols=5, ld=HM + 3)
    k = {key: np.array(v, order="F") for key, v in KDE.items()}
    t.call("jch_kde_dens", 0, z.ptr, HN, 3, z.ld, q.ptr, HM, q.ld, k["cs"].ctypes.data, 2, k["u"].ctypes.data, k["v2"].ctypes.data, k["coef"].ctypes.data,
           k["dims"].ctypes.data, 2, o.ptr, o.ld)
    t.out.update(kde=o.get(4))


def c_kde(d, o):
    dens, bound = SKDE.ld_kde_dens(d["X3"], d["Q3"], KDE["cs"], KDE["u"], KDE["v2"], KDE["coef"], KDE["dims"])
    got = o["kde"].reshape(HM, 2, 2).transpose(0, 2, 1)          # element (i, c, a) sits in column c + ncls a
    r = SKDE.ratio(got, dens, bound)
    print(f"  jch_kde_dens: {r:.3f} of the bound")
    assert r <= 1.0


def r_knn(t):
    d, L = t.d, t.L
    z, q, y = t.inp(d["X"]), t.inp(d["Q"]), t.inp(d["Y"])
    model = C.c_void_p()
    t.call("jch_knn_prepare", 0, z.ptr, HN, 5, z.ld, C.byref(model))
    k = K_NB
    ind, dist, w, dmed = np.full(HM * k + 1, -1, dtype=np.int32), nanv(HM * k), nanv(HM * k), nanv(HM)
    t.call("jch_knn_search", model, 0, q.ptr, HM, q.ld, k, None, H_W, TOL_W, 0, ind.ctypes.data, dist.ctypes.data, w.ctypes.data, dmed.ctypes.data)
    t.call("jch_knn_release", model)
    assert ind[-1] == -1
    pm = HostMat(rows=HM, cols=3)
    t.call("jch_knn_wmean", 0, y.ptr, HN, 2, y.ld, ind.ctypes.data, w.ctypes.data, HM, k, pm.ptr)
    cls, vp, vs = np.array(d["cls"]), np.full(HM + 1, -1, dtype=np.int32), HostMat(rows=HM, cols=3)
    t.call("jch_knn_vote", 0, cls.ctypes.data, HN, 2, ind.ctypes.data, w.ctypes.data, HM, k, vp.ctypes.data, vs.ptr)
    v, gm = np.array(d["X"][:, 0]), nanv(HM)
    t.call("jch_knn_gather_median", 0, v.ctypes.data, HN, ind.ctypes.data, HM, k, gm.ctypes.data)
    pw, info = HostMat(rows=HM, cols=3), np.full(HM + 1, -1, dtype=np.int32)
    t.call("jch_knn_wls", 0, z.ptr, HN, 5, z.ld, y.ptr, 2, y.ld, q.ptr, HM, q.ld, ind.ctypes.data, w.ctypes.data, k, pw.ptr, info.ctypes.data)
    assert vp[-1] == -1 and info[-1] == -1
    t.out.update(ind=ind[:-1].reshape(HM, k).copy(), dist=body(dist).reshape(HM, k).copy(), w=body(w).reshape(HM, k).copy(), dmed=body(dmed).copy(), wmean=pm.get(2),
                 vote=vp[:-1].copy(), score=vs.get(2), gmed=body(gm).copy(), wls=pw.get(2), wls_info=info[:-1].copy())


def c_knn(d, o):
    ind, dist = O.getknn(d["X"], d["Q"], k=K_NB)
    assert np.array_equal(o["ind"], ind), "jch_knn_search: other neighbours than the brute-force search"
    assert np.all(np.abs(o["dist"] - dist) <= 1e-9 * dist)                                  # test_gpu_knn.test_getknn
    w = np.stack([SKNN.np_weights(o["dist"][i], H_W, TOL_W) for i in range(HM)])
    assert O.rel_fro(w, o["w"]) < 1e-7                                                       # test_gpu_knn
    med = np.array([SKNN.np_middle_median(np.sort(o["dist"][i])) for i in range(HM)])
    assert np.all(np.abs(o["dmed"] - med) <= 4 * 2.0 ** -53 * np.abs(med))
    ref = SKNN.np_wmean(d["Y"], o["ind"], o["w"], LD)
    assert np.all(np.abs(o["wmean"].astype(LD) - ref) <= SKNN.wmean_bound(d["Y"], o["ind"], o["w"]))
    score = np.zeros((HM, 2))
    for i in range(HM):
        for j in range(K_NB):
            score[i, d["cls"][o["ind"][i, j]]] += o["w"][i, j]
    assert np.array_equal(o["score"], score) and np.array_equal(o["vote"], np.argmax(score, axis=1))
    gm = np.array([SKNN.np_middle_median(np.sort(d["X"][o["ind"][i], 0])) for i in range(HM)])
    assert np.array_equal(o["gmed"], gm)
    pred, info, bound = SMLR.wls_reference(d["X"], d["Y"], d["Q"], o["ind"], o["w"])
    assert np.array_equal(o["wls_info"], info) and not info.any()
    r = SMLR.max_ratio(o["wls"], pred, bound)
    print(f"  jch_knn_wls: {r:.3f} of the bound")
    assert r <= 1.0


def r_gda(t):
    d = t.d
    T, tq, cn = (np.ascontiguousarray(d[k]) for k in ("gdaT", "gdatq", "gdacls"))
    le = NLV_HI
    post, code, info = nanv(HM * le * 2), np.full(HM * le + 1, -7, dtype=np.int32), np.full(HM * le + 1, -7, dtype=np.int32)
    t.call("jch_knn_gda", 0, T.ctypes.data, HM, K_NB, NLV_HI, tq.ctypes.data, cn.ctypes.data, 2, 2, 1, 1, NLV_HI, post.ctypes.data, code.ctypes.data, info.ctypes.data)
    assert code[-1] == -7 and info[-1] == -7
    t.out.update(gda_post=body(post).reshape(HM, le, 2).copy(), gda_code=code[:-1].reshape(HM, le).copy(), gda_info=info[:-1].reshape(HM, le).copy())


def c_gda(d, o):
    worst = 0.0
    for i in range(HM):
        ref = SDA.gda_reference(d["gdaT"][i], d["gdatq"][i], d["gdacls"][i], 2, "qda", "prop", 1, NLV_HI)
        assert np.array_equal(o["gda_info"][i], ref["info"]) and not ref["info"].any()
        worst = max(worst, SKDE.ratio(o["gda_post"][i], ref["post"], ref["post_bound"]))
    print(f"  jch_knn_gda: {worst:.3f} of the bound")
    assert worst <= 1.0


def r_lwplsr(t):
    d = t.d
    x, y, xq = t.inp(d["X"]), t.inp(d["Y"]), t.inp(d["Q"])
    le, q, k, m = NLV_HI + 1, 2, K_NB, HM

    def outs():
        return nanv(m * le * q), np.full(m * k + 1, -1, dtype=np.int32), nanv(m * k), nanv(m * k)

    pred, ind, dist, w = outs()
    t.call("jch_lwplsr_predict", 0, x.ptr, HN, 5, x.ld, y.ptr, q, y.ld, x.ptr, x.ld, xq.ptr, xq.ld, 5, xq.ptr, m, xq.ld, k, H_W, TOL_W, 0, 0, NLV_HI,
           pred.ctypes.data, ind.ctypes.data, dist.ctypes.data, w.ctypes.data)
    model = C.c_void_p()
    t.call("jch_lwplsr_prepare", 0, x.ptr, HN, 5, x.ld, y.ptr, q, y.ld, x.ptr, x.ld, 5, C.byref(model))
    p2, i2, d2, w2 = outs()
    t.call("jch_lwplsr_predict_prepared", model, 0, xq.ptr, xq.ld, xq.ptr, m, xq.ld, k, H_W, TOL_W, 0, 0, NLV_HI, p2.ctypes.data, i2.ctypes.data, d2.ctypes.data,
           w2.ctypes.data)
    eye = np.asfortranarray(np.eye(5))
    t.call("jch_lwplsr_add_query_map", model, None, None, eye.ctypes.data, 5, 5, None)
    p3, i3, d3, w3 = outs()
    t.call("jch_lwplsr_predict_prepared", model, 0, None, 0, xq.ptr, m, xq.ld, k, H_W, TOL_W, 0, 0, NLV_HI, p3.ctypes.data, i3.ctypes.data, d3.ctypes.data, w3.ctypes.data)
    # the discrimination and the averaging entries on a handle of their own kind
    t.call("jch_lwplsr_release", model)
    assert ind[-1] == i2[-1] == i3[-1] == -1
    t.out.update(lw_pred=body(pred).reshape(m, le, q).copy(), lw_ind=ind[:-1].reshape(m, k).copy(), lw_dist=body(dist).copy(), lw_w=body(w).reshape(m, k).copy(),
                 lw_pred2=body(p2).copy(), lw_ind2=i2[:-1].copy(), lw_w2=body(w2).copy(), lw_pred3=body(p3).copy(), lw_ind3=i3[:-1].copy(), lw_w3=body(w3).copy())


def c_lwplsr(d, o):
    ref = O.lwplsr_predict(O.lwplsr(d["X"], d["Y"], nlvdis=0, metric="eucl", h=H_W, k=K_NB, nlv=NLV_HI, tol=TOL_W), d["Q"], nlv=range(0, NLV_HI + 1))
    assert np.array_equal(o["lw_ind"], ref["listnn"]) and O.rel_fro(ref["listw"], o["lw_w"]) < 1e-7
    err = O.rel_fro(ref["pred"], o["lw_pred"].transpose(0, 2, 1))
    print(f"  jch_lwplsr_predict: rel. Frobenius error of pred {err:.2e}")
    assert err < 1e-7                                                                     # test_gpu_envelope._cmp_lw
    assert np.array_equal(o["lw_ind2"], o["lw_ind"].ravel()) and np.array_equal(o["lw_ind3"], o["lw_ind"].ravel())
    for key in ("lw_pred2", "lw_pred3"):
        assert O.rel_fro(o["lw_pred"].ravel(), o[key]) < 1e-10                            # (the prepared forms: the same kernels behind another front end)


def r_lwplsda(t):
    d = t.d
    x, xq = t.inp(d["X"]), t.inp(d["Q"])
    cls = np.array(d["cls"])
    yd = t.inp((cls[:, None] == np.arange(2)[None, :]).astype(np.float64))
    m, k, lo, hi, nlev = HM, K_NB, 1, NLV_HI, 2
    le = hi - lo + 1
    model = C.c_void_p()
    t.call("jch_lwplsr_prepare", 0, x.ptr, HN, 5, x.ld, yd.ptr, nlev, yd.ld, x.ptr, x.ld, 5, C.byref(model))
    for kind in (0, 1):
        code, post, info = np.full(m * le + 1, -7, dtype=np.int32), nanv(m * le * nlev), np.full(m * le + 1, -7, dtype=np.int32)
        tloc, tq, ind, dist, w = nanv(m * k * hi), nanv(m * hi), np.full(m * k + 1, -1, dtype=np.int32), nanv(m * k), nanv(m * k)
        t.call("jch_lwplsda_predict_prepared", model, cls.ctypes.data, nlev, kind, 0, 0, xq.ptr, xq.ld, xq.ptr, m, xq.ld, k, H_W, TOL_W, 0, lo, hi, code.ctypes.data,
               post.ctypes.data, info.ctypes.data, tloc.ctypes.data, tq.ctypes.data, ind.ctypes.data, dist.ctypes.data, w.ctypes.data)
        assert code[-1] == -7 and info[-1] == -7 and ind[-1] == -1
        t.out.update({f"da{kind}_code": code[:-1].reshape(m, le).copy(), f"da{kind}_post": body(post).reshape(m, le, nlev).copy(),
                      f"da{kind}_info": info[:-1].reshape(m, le).copy(), f"da{kind}_tloc": body(tloc).copy(), f"da{kind}_tq": body(tq).copy(),
                      f"da{kind}_ind": ind[:-1].reshape(m, k).copy(), f"da{kind}_w": body(w).reshape(m, k).copy()})
    t.call("jch_lwplsr_release", model)


def c_lwplsda(d, o):
    for kind, name in ((0, "rda"), (1, "lda")):
        ind, w = o[f"da{kind}_ind"], o[f"da{kind}_w"]
        assert not o[f"da{kind}_info"].any(), "a neighbourhood was not fitted: the ranks' call counts may differ"
        ref = SDA.np_locw_da(d["X"], d["cls"], d["Q"], ind, w, 2, name, "unif", 1, NLV_HI, False, np.float64)
        post = np.stack([r["post"] for r in ref])
        if kind == 0:
            err = O.rel_fro(post, o["da0_post"])
            print(f"  jch_lwplsda_predict_prepared (rda): rel. Frobenius error of the dummy predictions {err:.2e}")
            assert err < 1e-7                                                             # test_gpu_lwplsda: the local fits against the restatement
        # the labels wherever the reference's two posteriors are further apart than the local scores' 1e-7 can move them (d2 <= 100: 1e-5; 1e-4 taken)
        code = np.stack([r["code"] for r in ref])
        decided = np.abs(post[:, :, 0] - post[:, :, 1]) > 1e-4
        assert decided.mean() > 0.9 and np.array_equal(o[f"da{kind}_code"][decided], code[decided])


def r_lwplsravg(t):
    d = t.d
    x, y, xq = t.inp(d["X"]), t.inp(d["Y"]), t.inp(d["Q"])
    m, k, q = HM, K_NB, 2
    model = C.c_void_p()
    t.call("jch_lwplsr_prepare", 0, x.ptr, HN, 5, x.ld, y.ptr, q, y.ld, x.ptr, x.ld, 5, C.byref(model))
    for typf in (0, 1):
        lo, hi = 1, NLV_HI
        le = hi - lo + 1
        pred, plv, wlv, rr, rb = nanv(m * q), nanv(m * le * q), nanv(m * le), nanv(m * hi), nanv(m * hi)
        info, ind, dist, w = np.full(m + 1, -7, dtype=np.int32), np.full(m * k + 1, -1, dtype=np.int32), nanv(m * k), nanv(m * k)
        t.call("jch_lwplsravg_predict_prepared", model, 0, xq.ptr, xq.ld, xq.ptr, m, xq.ld, k, H_W, TOL_W, 0, lo, hi, typf, pred.ctypes.data, plv.ctypes.data,
               wlv.ctypes.data, rr.ctypes.data, rb.ctypes.data, info.ctypes.data, ind.ctypes.data, dist.ctypes.data, w.ctypes.data)
        assert info[-1] == -7 and ind[-1] == -1
        t.out.update({f"avg{typf}_pred": body(pred).reshape(m, q).copy(), f"avg{typf}_plv": body(plv).copy(), f"avg{typf}_wlv": body(wlv).copy(),
                      f"avg{typf}_ind": ind[:-1].reshape(m, k).copy(), f"avg{typf}_info": info[:-1].copy()})
        if typf == 1:
            t.out.update(avg1_rr=body(rr).copy(), avg1_rb=body(rb).copy())
        else:
            assert np.isnan(rr).all() and np.isnan(rb).all(), "typf = 0 writes no Shenk norms"
    t.call("jch_lwplsr_release", model)


def c_lwplsravg(d, o):
    for typf, name in ((0, "unif"), (1, "shenk")):
        ref = RAVG.np_lwplsravg_predict(d["X"], d["Y"], d["Q"], nlvdis=0, metric="eucl", h=H_W, k=K_NB, nlv=f"1:{NLV_HI}", typf=name, tol=TOL_W)
        err = O.rel_fro(ref["pred"], o[f"avg{typf}_pred"])
        print(f"  jch_lwplsravg_predict_prepared ({name}): rel. Frobenius error of pred {err:.2e}")
        assert np.array_equal(o[f"avg{typf}_ind"], ref["listnn"]) and err < 1e-7          # test_gpu_plsavg
        assert not o[f"avg{typf}_info"].any()


LOCAL_ROUTES = [(r_knn, c_knn), (r_lwplsr, c_lwplsr), (r_lwplsda, c_lwplsda), (r_lwplsravg, c_lwplsravg)]
PLAIN_ROUTES = [(r_accessors, c_accessors), (r_rows, c_rows), (r_resid, c_resid), (r_kde, c_kde), (r_gda, c_gda)]


def _joined_against_unjoined(routes):
    """The routes on two joined ranks (each with its own data), then the closing jch_col_stats; the same routes on a fresh unjoined ctx per rank: the same
    bytes; the unjoined results against the families' references."""
    L = J.load()
    closing, closing_check = _stats_after()

    def sequence(ctx, r, errors):
        outs = {}
        for run, _ in routes:
            t = Route(L, ctx, ldata(r))
            try:                                             # (a failing route must not keep this rank from the calls behind it)
                run(t)
                for x in t.ins:
                    unchanged(x)
            except BaseException as e:  # noqa: BLE001
                errors.append((run.__name__, repr(e)))
            errors.extend((run.__name__, name, st, msg) for name, st, msg in t.st if st != 0)
            outs.update(t.out)
        return outs

    def fn(r, ctx):
        errors = []
        outs = sequence(ctx, r, errors)
        return outs, errors, closing(L, ctx, r)

    joined = run_ranks(2, fn)
    for r, (outs, errors, _) in enumerate(joined):
        assert not errors, (r, errors)
    closing_check([j[2] for j in joined])
    for r in range(2):
        ctx, errors = J.Context(0), []
        try:
            plain = sequence(ctx, r, errors)
        finally:
            ctx.close()
        assert not errors, ("unjoined", r, errors)
        assert set(plain) == set(joined[r][0])
        diff = sorted(k for k in plain if not same_bytes(plain[k], joined[r][0][k]))
        assert not diff, f"rank {r}: on the joined ctx these outputs are not the bytes of the unjoined call: {diff}"
        for _, check in routes:
            check(ldata(r), plain)


def test_the_two_ranks_hold_different_data_of_equal_shape():
    a, b = ldata(0), ldata(1)
    assert all(np.shape(a[k]) == np.shape(b[k]) for k in a) and not np.array_equal(a["X"], b["X"]) and not np.array_equal(a["Q"], b["Q"])


def test_rank_local_accessors_rows_residuals_kde_and_gda():
    _joined_against_unjoined(PLAIN_ROUTES)


@pytest.mark.parametrize("knobs", [{}, {"JCH_KNN_GENERIC": "1"}, {"JCH_LOCW_GENERIC": "1"}, {"JCH_LOCW_KSPACE": "0"}],
                         ids=["default", "generic-knn", "generic-per-query-fits", "p-space-kernel"])
def test_rank_local_models(knobs, monkeypatch):
    """The local-model family by its routes: the batched kernels, the generic kNN selection (JCH_KNN_GENERIC=1), the per-query jch_plskern_fit + jch_predict
    (+ jch_transform) of jch_lwplsr_predict* and jch_lwplsda_predict_prepared (JCH_LOCW_GENERIC=1: on a joined ctx these fits were collectives before
    jch_comm_off) and the p-space kernel with the neighbour-space one switched off.  The knobs are read at call time, by both ranks alike."""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    _joined_against_unjoined(LOCAL_ROUTES)


def test_rank_local_device_entries():
    """jch_fill_uniform, jch_chol_*, jch_kc_panel and jch_covsel_pass take device pointers only: the buffers are made here, the rank threads only call."""
    L = J.load()
    closing, closing_check = _stats_after()
    n = HN

    def buffers(r):
        d = ldata(r)
        return dict(fill=Dev(rows=7, cols=4, ld=8), A=Dev(d["SPD"], ld=n + 1), B=Dev(d["V"], ld=n + 1), K=Dev(d["SPD"]), V=Dev(d["V"], ld=n + 1), KV=Dev(rows=n, cols=4, ld=n + 1),
                    X=Dev(d["X"], ld=n + 1), mu=Dev(d["X"].mean(axis=0)), XV=Dev(rows=5, cols=4), info=C.c_int32(-7), fro=C.c_double(NAN))

    def sequence(ctx, r, b):
        st = [L.jch_fill_uniform(ctx._h, b["fill"].ptr, 7, 3, 8, 5 + r, 40, 99 + r),
              L.jch_chol_factor(ctx._h, b["A"].ptr, n, n + 1, C.byref(b["info"])),
              L.jch_chol_solve(ctx._h, b["A"].ptr, n, n + 1, b["B"].ptr, 3, n + 1),
              L.jch_chol_inv_fro2(ctx._h, b["A"].ptr, n, n + 1, C.byref(b["fro"])),
              L.jch_kc_panel(ctx._h, b["K"].ptr, n, b["V"].ptr, n + 1, 3, b["KV"].ptr, n + 1),
              L.jch_covsel_pass(ctx._h, b["X"].ptr, n, 5, n + 1, b["mu"].ptr, b["V"].ptr, 3, n + 1, b["XV"].ptr),
              L.jch_ctx_synchronize(ctx._h)]
        return st

    def collect(b):
        return dict(fill=b["fill"].get(3), L=np.tril(b["A"].get()), solve=b["B"].get(), fro=np.array([b["fro"].value]), info=np.array([b["info"].value]), KV=b["KV"].get(3),
                    XV=b["XV"].get(3))

    jb = [buffers(0), buffers(1)]
    res = run_ranks(2, lambda r, ctx: (sequence(ctx, r, jb[r]), closing(L, ctx, r)))
    closing_check([x[1] for x in res])
    for r in range(2):
        assert res[r][0] == [0] * 7, res[r][0]
        pb, ctx = buffers(r), J.Context(0)
        torch.cuda.synchronize()
        try:
            assert sequence(ctx, r, pb) == [0] * 7
        finally:
            ctx.close()
        plain, joined, d = collect(pb), collect(jb[r]), ldata(r)
        diff = sorted(k for k in plain if not same_bytes(plain[k], joined[k]))
        assert not diff, f"rank {r}: not the bytes of the unjoined call: {diff}"
        for x in (pb["K"], pb["V"], pb["X"], pb["mu"]):
            x.unchanged()
        assert np.array_equal(plain["fill"], O.rand_matrix(99 + r, 7, 3, row0=5 + r, n_total=40)) and plain["info"][0] == 0
        A, V = d["SPD"], d["V"]
        bound = (n + 10) * EPS * np.linalg.cond(A)                                       # test_gpu_krr.test_cholesky_primitives_against_scipy
        Lref = np.linalg.cholesky(A)
        assert O.rel_fro(Lref, plain["L"]) <= bound and O.rel_fro(np.linalg.solve(A, V), plain["solve"]) <= 2 * bound
        fref = float(np.sum(np.linalg.inv(Lref) ** 2))
        assert abs(plain["fro"][0] - fref) <= 2 * bound * fref
        # a fixed-order n-term dot product per element: gamma(n) on the sum of the absolute terms, twice for an order of their own; the centring of
        # jch_covsel_pass adds one rounding per term (n + 4)
        check_bound("L", "jch_kc_panel", plain["KV"], A.astype(LD) @ V.astype(LD), 2 * S.gamma(n + 2) * (np.abs(A) @ np.abs(V)))
        Xc = d["X"].astype(LD) - d["X"].mean(axis=0).astype(LD)
        check_bound("L", "jch_covsel_pass", plain["XV"], Xc.T @ V.astype(LD), 2 * S.gamma(n + 4) * (np.abs(np.asarray(Xc, dtype=np.float64)).T @ np.abs(V)))


def test_the_mirror_refuses_its_per_query_loop_on_a_joined_ctx():
    """plsavg.lwplsravg_predict outside the batched call's envelope (p = 2100) fits `plsravg` per query through class-C entries: on a joined ctx it raises
    before any device work instead of all-reducing with the other ranks' queries; the batched shape goes through as a class-L call."""
    rng = np.random.default_rng(9)
    X, Y, Xq = np.asfortranarray(rng.standard_normal((40, 2100))), np.asfortranarray(rng.standard_normal((40, 2))), np.asfortranarray(rng.standard_normal((3, 2100)))

    def fn(r, ctx):
        fm = J.lwplsravg(X, Y, nlvdis=0, metric="eucl", h=2.0, k=20, nlv="1:2", typf="shenk", ctx=ctx)
        try:
            J.predict(fm, Xq, ctx=ctx)
        except _lib.JchError as e:
            return e.code, str(e)
        return 0, ""

    for code, msg in run_ranks(2, fn):
        assert code == EINVAL and "one rank only" in msg, (code, msg)


# ==================================================================================================== class R
class Refusals:
    """Valid small arguments (65 x 3, q = 2) of every class-R entry on host arrays; `outs` registers every output (NaN, or -1 for integers), `ins` every
    input with a copy.  calls() -> [(name, args after ctx)]."""

    def __init__(self, rank):
        d = ldata(rank)
        self.ins, self.outs, self.keep = [], [], []
        n, m, p, q, A = HN, HM, 3, 2, 2
        f = lambda a: self.i(np.asfortranarray(a))                                     # noqa: E731
        X, Q, Y = f(d["X3"]), f(d["Q3"]), f(d["Y"])
        o, oi, P = self.o, self.oi, (lambda a: None if a is None else a.ctypes.data)
        i32, f64, i64 = (lambda: self.ref(C.c_int32(-1))), (lambda: self.ref(C.c_double(NAN))), (lambda: self.ref(C.c_int64(-1)))
        desc = self.ref(_lib.PlsDesc(n, p, q, A, 0, 0, 0, 0, 0))
        rng = np.random.default_rng(5 + rank)
        vn, vp, vq = (f(rng.uniform(0.5, 1.5, k)) for k in (n, p, q))
        Rn, Cq = f(rng.standard_normal((n, A))), f(rng.standard_normal((q, A)))
        wn = f(np.full(n, 1.0 / n))
        Kd = Dev(d["SPD"])                                                               # (the working Gram of krr is a device matrix on every route)
        self.keep.append(Kd)
        cs, init, rows_ = f(np.array([0, 30, n], dtype=np.int64)), f(np.array([0, 5], dtype=np.int64)), f(np.arange(0, 40, dtype=np.int64))
        Sm, Mu, Bpq = f(np.stack([np.cov(d["X3"].T) + np.eye(p)] * 2).reshape(2 * p, p).T.copy()), f(rng.standard_normal((2, p))), f(rng.standard_normal((p, q)))
        Uinv = f(np.stack([np.triu(rng.standard_normal((p, p))) + 3 * np.eye(p)] * 2).reshape(2 * p, p).T.copy())
        mu0 = f(d["X3"].mean(axis=0))
        g = (0, 0.5, 0.0, 1)                                                             # krbf, gamma, coef0, degree
        self.calls = [
            ("jch_kernel_gram", [0, g[0], P(Q), m, m, None, P(X), n, n, None, p, g[1], g[2], g[3], P(o(m * n)), m]),
            ("jch_dkplsr_fit", [desc, *g, P(X), n, P(Y), n, None, None, P(o(n * A)), P(o(n * A)), P(o(n * A)), P(o(n * A)), P(o(q * A)), P(o(A)), P(o(n)), P(o(n)), P(o(q)), P(o(q)),
                                P(o(n)), P(o(p)), P(o(q)), i32()]),
            ("jch_dkplsr_transform", [0, *g, P(Q), m, p, m, None, P(X), n, n, P(vn), P(vn), P(Rn), A, P(o(m * A)), m]),
            ("jch_dkplsr_predict", [0, *g, P(Q), m, p, m, None, P(X), n, n, P(vn), P(vn), P(vq), P(vq), P(Rn), P(Cq), q, 0, A, None, P(o(m * (A + 1) * q)), m]),
            ("jch_kplsr_fit", [desc, *g, 1.5e-8, 100, P(X), n, P(Y), n, None, None, P(o(n * A)), P(o(n * A)), P(o(n * A)), P(o(n)), P(o(q * A)), P(o(p)), P(o(q)), P(o(q)), P(o(n)),
                               self.ref((C.c_int32 * A)(-1, -1)), i32()]),
            ("jch_kplsr_transform", [0, *g, P(Q), m, p, m, None, P(X), n, n, P(wn), P(vn), P(Rn), A, P(o(m * A)), m]),
            ("jch_kplsr_predict", [0, *g, P(Q), m, p, m, None, P(X), n, n, P(wn), P(vn), P(vq), P(vq), P(Rn), P(Cq), q, 0, A, P(o(m * (A + 1) * q)), m]),
            ("jch_kpca_fit", [0, *g, P(X), n, p, n, None, A, 0, 1e-9, 200, None, P(o(n * A)), P(o(n * A)), P(o(n)), P(o(n)), P(o(p)), P(o(A)), P(o(A)), P(o(1)), i32(), P(o(A)), i32()]),
            ("jch_krr_fit", [0, *g, P(X), n, p, n, P(Y), q, n, None, 0, Kd.ptr, None, P(o(n * q)), P(o(n)), P(o(n)), P(o(p)), P(o(q))]),
            ("jch_krr_solve", [0, Kd.ptr, n, P(Y), q, P(wn), 0.1, 1, P(o(n * q)), P(o(n * q)), P(o(1)), i32()]),
            ("jch_covsel_fit", [0, P(X), n, p, n, P(Y), q, n, 2, 0, 0, P(oi(2)), P(o(2)), P(o(p)), P(o(p * 2)), P(o(2)), P(o(2)), P(o(p)), P(o(q)), P(o(q)), P(o(p * 2)), P(o(2 * q)),
                                P(o(n * 2)), i32()]),
            ("jch_xtdx", [0, P(X), n, p, n, None, None, 0, None, P(o(p * p)), P(o(p))]),
            ("jch_pca_fit", [0, P(X), n, p, n, None, P(Y), q, n, A, 0, 1e-9, 200, P(o(n * A)), P(o(p * A)), P(o(A)), P(o(A)), P(o(p)), P(o(p)), P(o(n)), P(o(1)), P(o(p)), P(o(q)),
                             P(o(p * q)), i32(), P(o(A)), i32(), i32()]),
            ("jch_pcasph_fit", [0, P(X), n, p, n, None, A, 0, 1e-3, 50, 0, 1e-9, 200, P(o(n * A)), P(o(p * A)), P(o(A)), P(o(A)), P(o(p)), P(o(p)), P(o(n)), f64(), P(o(p)), i32(), i32(),
                                i32(), P(o(A)), i32(), i32(), i64()]),
            ("jch_col_median_mad", [0, P(X), n, p, n, P(o(p)), P(o(p)), 0]),
            ("jch_stah", [0, P(X), n, p, n, None, None, P(Bpq), q, p, 1, P(o(q)), P(o(q)), P(o(n))]),
            ("jch_weiszfeld_step", [0, P(X), n, p, n, P(mu0), 1e-3, -1.0, P(o(p)), P(o(n)), f64(), f64(), i64()]),
            ("jch_spatial_median", [0, P(X), n, p, n, 1e-3, 50, P(o(p)), P(o(n)), i32(), f64(), i32()]),
            ("jch_farthest_pair", [0, P(X), n, p, n, None, 0, P(oi(2, np.int64)), P(o(1))]),
            ("jch_maxmin_select", [0, P(X), n, p, n, 1, P(init), 6, P(oi(6, np.int64)), P(o(6))]),
            ("jch_class_cov", [0, P(X), n, p, n, P(cs), 2, P(o(p * p * 2)), P(o(p * p)), P(o(2 * p))]),
            ("jch_gauss_factor", [0, P(Sm), p, p, p * p, 2, P(o(p * p * 2)), p, p * p, P(o(p * 2)), P(oi(2))]),
            ("jch_mahsq_chol", [0, P(Q), m, p, m, P(Mu), 2, P(Uinv), p, p * p, 2, P(o(m * 2)), m]),
            ("jch_perm_fill", [0, P(oi(40 * 3)), 40, 3, 40, 7]),
            ("jch_perm_score_sums", [0, P(X), n, p, n, P(rows_), 40, P(Y), n, P(Y), q, n, P(Bpq), p, None, 0, 7, P(o((p + 1) * q * 6))]),
        ]

    def i(self, a):
        self.ins.append((a, a.copy()))
        return a

    def o(self, n):
        a = np.full(n, NAN)
        self.outs.append(a)
        return a

    def oi(self, n, dtype=np.int32):
        a = np.full(n, -1, dtype=dtype)
        self.outs.append(a)
        return a

    def ref(self, c):
        """A ctypes scalar / array output, passed by reference."""
        self.keep.append(c)
        self.outs.append(c)
        return c if isinstance(c, C.Array) else C.byref(c)

    def untouched(self):
        for a in self.outs:
            if isinstance(a, np.ndarray):
                if not (np.isnan(a).all() if a.dtype == np.float64 else np.all(a == -1)):
                    return False
            elif isinstance(a, C.c_double):
                if not np.isnan(a.value):
                    return False
            elif isinstance(a, (C.c_int32, C.c_int64)):
                if a.value != -1:
                    return False
            elif isinstance(a, C.Array):
                if any(v != -1 for v in a):
                    return False
        return True

    def reset(self):
        for a in self.outs:
            if isinstance(a, np.ndarray):
                a[...] = NAN if a.dtype == np.float64 else -1
            elif isinstance(a, C.c_double):
                a.value = NAN
            elif isinstance(a, (C.c_int32, C.c_int64)):
                a.value = -1
            elif isinstance(a, C.Array):
                for j in range(len(a)):
                    a[j] = -1

    def unchanged(self):
        return all(np.array_equal(a, b) for a, b in self.ins) and all(k.unchanged() is None for k in self.keep if isinstance(k, Dev))


def test_the_refusal_table_names_class_r():
    assert [name for name, _ in Refusals(0).calls] == CLASSES["R"]


def test_every_refused_entry_refuses_on_two_ranks_and_accepts_the_same_call_unjoined():
    L = J.load()
    closing, closing_check = _stats_after()
    tabs = [Refusals(0), Refusals(1)]

    def fn(r, ctx):
        seen = []
        for name, args in tabs[r].calls:
            st = getattr(L, name)(ctx._h, *args)
            seen.append((name, st, L.jch_last_error(ctx._h) or b"", tabs[r].untouched(), tabs[r].unchanged()))
        return seen, closing(L, ctx, r)

    res = run_ranks(2, fn)
    for r, (seen, _) in enumerate(res):
        for name, st, msg, untouched, unchanged in seen:
            assert st == EINVAL, f"rank {r}: {name} returned {st} on a joined ctx ({msg!r})"
            assert b"one rank only" in msg and name.encode() in msg, f"rank {r}: {name}: jch_last_error says {msg!r}"
            assert untouched, f"rank {r}: {name} wrote an output before it refused"
            assert unchanged, f"rank {r}: {name} changed an input"
    closing_check([x[1] for x in res])
    # the same calls on a ctx without a communicator are accepted: the refusal above was the only reason to fail
    ctx = J.Context(0)
    try:
        for name, args in tabs[0].calls:
            tabs[0].reset()
            st = getattr(L, name)(ctx._h, *args)
            assert st == 0, f"{name}: the table's arguments are not valid: {st} {L.jch_last_error(ctx._h)!r}"
            assert not tabs[0].untouched(), f"{name}: accepted, but wrote nothing"
    finally:
        ctx.close()


def test_zz_report_the_worst_ratios_of_the_class_c_primitives():
    """Not a check of its own: prints what the tests above measured (DESIGN.md 29 reports these figures)."""
    for prim in sorted(WORST):
        print(f"  worst err / bound on a joined ctx, {prim}: {WORST[prim]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
