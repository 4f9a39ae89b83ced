"""The joined ctx contract without a GPU (include/jchemo_hip.h, "joined ctx contract").

1. Every exported entry of the header is in exactly one class -- C collective, L rank-local, R refused, M management -- in the table of
   tests/test_gpu_joined_ctx.py (read with `ast`, so that this file needs no GPU and no library), and the header's contract block lists the same
   names per class: a new export cannot arrive unclassified.
2. The shapes and data of the class-C cases, shared with the GPU file, and the check the issue asks for before anything runs on the GPU: the
   longdouble references of the primitives, rounded to Float64, and a Float64 evaluation that adds per-shard partial sums in rank order (what a
   row-sharded call does) stay inside the per-element bounds of tests/test_accessors_static.py at these shapes.
3. The oracle facts the fit cases rely on (see `test_the_oracle_on_the_fit_cases`)."""
import ast
import os
import re
import sys
from functools import lru_cache

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_accessors_static as S  # noqa: E402
from oracle import plsr_oracle as O  # noqa: E402
from test_accessors_static import LD  # noqa: E402

HEADER = os.path.join(ROOT, "include", "jchemo_hip.h")
GPU_FILE = os.path.join(ROOT, "tests", "test_gpu_joined_ctx.py")


# ---------------------------------------------------------------------------------------------------- 1. the classes
def header_exports():
    """Every `JCH_API <type> jch_name(` of the header, in order."""
    with open(HEADER) as f:
        return re.findall(r"^JCH_API\s+[\w\s\*]*?\**\s*(jch_\w+)\s*\(", f.read(), flags=re.M)


def header_contract():
    """{class: [names]} of the header's contract block: its lines ` *   C: jch_a jch_b ...`."""
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r"---- joined ctx contract:(.*?)---- end of the joined ctx contract", text, flags=re.S)
    assert m, "include/jchemo_hip.h has no joined ctx contract block"
    out = {}
    for cls, names in re.findall(r"^ \*\s+([CLRM]):\s+(.*)$", m.group(1), flags=re.M):
        out.setdefault(cls, []).extend(names.split())
    return out


def gpu_table():
    """The literal `CLASSES = {...}` of tests/test_gpu_joined_ctx.py."""
    with open(GPU_FILE) as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "CLASSES" for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError("tests/test_gpu_joined_ctx.py has no CLASSES table")


def is_management(name):
    """Class M as the issue names it: ctx, communicator, p2p, profiling and counter management (the all-reduce probe is a collective)."""
    if name == "jch_ctx_allreduce_probe":
        return False
    return name in ("jch_version", "jch_last_error") or name.startswith(("jch_ctx_", "jch_comm_", "jch_loopback_"))


def test_the_header_parser_sees_the_exports():
    names = header_exports()
    assert len(names) == len(set(names)) and len(names) >= 84
    assert {"jch_last_error", "jch_plskern_fit", "jch_ctx_get_counter", "jch_lwplsravg_predict_prepared", "jch_pcasph_fit"} <= set(names)
    with open(HEADER) as f:
        assert len(re.findall(r"^JCH_API\s", f.read(), flags=re.M)) == len(names)          # no prototype the pattern above does not read


def test_every_export_is_in_exactly_one_class_of_the_gpu_table():
    table, names = gpu_table(), header_exports()
    assert set(table) == {"C", "L", "R", "M"}
    listed = [n for cls in "CLRM" for n in table[cls]]
    assert len(listed) == len(set(listed)), sorted(n for n in set(listed) if listed.count(n) > 1)
    assert set(listed) == set(names), ("unclassified: %s; not exported: %s" % (sorted(set(names) - set(listed)), sorted(set(listed) - set(names))))


def test_the_header_block_lists_the_same_names_per_class():
    table, block = gpu_table(), header_contract()
    assert set(block) == {"C", "L", "R", "M"}
    for cls in "CLRM":
        assert len(block[cls]) == len(set(block[cls])), cls
        assert set(block[cls]) == set(table[cls]), (cls, sorted(set(block[cls]) ^ set(table[cls])))


def test_class_m_holds_the_management_entries_only():
    table = gpu_table()
    assert set(table["M"]) == {n for n in header_exports() if is_management(n)}
    assert "jch_ctx_allreduce_probe" in table["C"]


def test_the_classes_the_issue_names():
    table = gpu_table()
    assert set(table["C"]) == {"jch_plskern_fit", "jch_plsnipals_fit", "jch_plssimp_fit", "jch_plsrosa_fit", "jch_plswold_fit", "jch_plskern_fit_scaled", "jch_col_stats",
                               "jch_weighted_ss", "jch_weighted_cov", "jch_score_sums", "jch_score_sums_lv", "jch_ctx_allreduce_probe"}
    for n in ("jch_affine_gemm", "jch_transform", "jch_predict", "jch_row_resid_ss", "jch_row_resid_ss_lv", "jch_fill_uniform", "jch_kc_panel", "jch_covsel_pass",
              "jch_knn_wls", "jch_knn_gda", "jch_lwplsda_predict_prepared", "jch_lwplsravg_predict_prepared", "jch_kde_dens"):
        assert n in table["L"], n
    assert {n for n in header_exports() if n.startswith(("jch_rows_", "jch_chol_", "jch_lwplsr_", "jch_knn_"))} <= set(table["L"])
    for n in ("jch_col_median_mad", "jch_stah", "jch_xtdx", "jch_farthest_pair", "jch_pca_fit", "jch_covsel_fit"):
        assert n in table["R"], n


def test_the_wording_of_the_header_agrees_with_the_classes():
    """No class-L or class-C entry is still called "One rank only", and jch_col_median_mad now is."""
    with open(HEADER) as f:
        text = f.read()
    table = gpu_table()
    docs = {}
    for m in re.finditer(r"/\*(.*?)\*/\s*((?:typedef[^;]*;\s*)?(?:JCH_API[^;]*;\s*)+)", text, flags=re.S):   # a comment and the prototypes it heads
        for name in re.findall(r"(jch_\w+)\s*\(", m.group(2)):
            docs[name] = m.group(1)
    for name in ("jch_row_resid_ss", "jch_row_resid_ss_lv", "jch_knn_search", "jch_knn_wls", "jch_lwplsravg_predict_prepared", "jch_col_stats", "jch_weighted_cov"):
        assert name in docs and not re.search(r"one rank only", docs[name], flags=re.I), name
        assert (name in table["L"] and "ank-local" in docs[name]) or (name in table["C"] and "ollective" in docs[name]), name
    assert re.search(r"One rank only", docs["jch_col_median_mad"])


# ---------------------------------------------------------------------------------------------------- 2. the class-C primitives: cases and data
SPLIT = (3, 97, 97)                                    # rows per loopback rank: one shard of three rows, two of 97 (no multiple of anything)
N = sum(SPLIT)
EDGES = np.concatenate([[0], np.cumsum(SPLIT)])


def shards(a):
    return [None if a is None else a[EDGES[r]:EDGES[r + 1]] for r in range(len(SPLIT))]


# jch_col_stats / jch_weighted_ss: (p, level, weights); stds and NULL stds are both called.  jch_weighted_cov: (d, level, weights): d = 5 takes the X'DY
# kernels, d = 70 the centred copy and the tiled SYRK.
STATS_CASES = [(37, 1e4, None), (37, 1e4, "zeros"), (130, 0.0, "random")]
COV_CASES = [(5, 100.0, "random"), (70, 100.0, None), (70, 0.0, "zeros")]
SCORE_CASES = [(3, 2, None), (3, 2, "random"), (17, 33, "random")]          # (q, levels, mask); with a mask rank 0 selects nothing
SCORE_LV_CASES = [(3, 7, "random"), (1, 12, None)]                          # (q, kfit, mask)


def score_case(q, levels, mkind):
    Pred, Y, mask = S.score_data(N, q, levels, mkind)
    if mask is not None:                                                    # the three rows of rank 0: unselected, and NaN like every unselected row
        mask = mask.copy(); mask[:SPLIT[0]] = 0.0
        Pred, Y = Pred.copy(order="F"), Y.copy(order="F")
        Pred[:SPLIT[0]] = np.nan; Y[:SPLIT[0]] = np.nan
    return Pred, Y, mask


def score_lv_case(q, kfit, mkind):
    T, Cm, ym, ys, Y, mask = S.score_lv_data(N, q, kfit, mkind, False)
    if mask is not None:
        mask = mask.copy(); mask[:SPLIT[0]] = 0.0
        T, Y = T.copy(order="F"), Y.copy(order="F")
        T[:SPLIT[0]] = np.nan; Y[:SPLIT[0]] = np.nan
    return T, Cm, ym, ys, Y, mask


def _inside(name, got, ref, bound, share=1.0):
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    assert np.isfinite(err).all() and np.all(bound >= 0.0), name
    assert np.all(err <= share * bound), f"{name}: err / bound {float(np.max(err / np.where(bound > 0, bound, 1.0))):.3f}"


def _rank_order_sum(parts):
    acc = parts[0].copy()
    for x in parts[1:]:
        acc = acc + x
    return acc


@pytest.mark.parametrize("case", STATS_CASES, ids=lambda c: "p%d-level%g-w_%s" % c)
def test_col_stats_and_weighted_ss_references_fit_the_bounds_when_sharded(case):
    p, level, wkind = case
    X, w = S.stats_data(N, p, level, wkind)
    mean, std = S.ref_col_stats(X, w)
    bm, bs = S.bound_means(X, w), S.bound_stds(X, w)
    _inside("means rounded", np.asarray(mean, dtype=np.float64), mean, bm)
    _inside("stds rounded", np.asarray(std, dtype=np.float64), std, bs)
    w64 = np.ones(N) if w is None else w
    tot = _rank_order_sum([np.array([ws.sum()]) for ws in shards(w64)])[0]
    m64 = _rank_order_sum([(ws / tot) @ xs for xs, ws in zip(shards(X), shards(w64))])
    v64 = _rank_order_sum([(ws / tot) @ (xs - m64) ** 2 for xs, ws in zip(shards(X), shards(w64))])
    _inside("means sharded", m64, mean, bm, 0.5)
    _inside("stds sharded", np.sqrt(v64), std, bs, 0.5)
    d = w64 / w64.sum()
    for shift, scale in ((np.asarray(mean, dtype=np.float64), np.random.default_rng(N + p).uniform(0.5, 2.0, p)), (None, None)):
        ref, b = S.ref_weighted_ss(X, d, shift, scale), S.bound_weighted_ss(X, d, shift, scale)
        sh, sc = S._or(shift, 0.0, p), S._or(scale, 1.0, p)
        got = _rank_order_sum([((ds @ (xs - sh) ** 2) / sc ** 2).sum(keepdims=True) for xs, ds in zip(shards(X), shards(d))])
        _inside("ss rounded", np.array([float(ref)]), np.array([ref], dtype=LD), np.array([b]))
        _inside("ss sharded", got, np.array([ref], dtype=LD), np.array([b]), 0.5)


@pytest.mark.parametrize("case", COV_CASES, ids=lambda c: "d%d-level%g-w_%s" % c)
def test_weighted_cov_reference_fits_the_bounds_when_sharded(case):
    d_, level, wkind = case
    A, w = S.cov_data(N, d_, level, wkind)
    Sref, mu = S.ref_weighted_cov(A, w)
    b, bm = S.bound_weighted_cov(A, w), S.bound_means(A, w)
    _inside("S rounded", np.asarray(Sref, dtype=np.float64), Sref, b)
    _inside("mu rounded", np.asarray(mu, dtype=np.float64), mu, bm)
    w64 = np.ones(N) if w is None else w
    dd = w64 / w64.sum()
    m64 = _rank_order_sum([ds @ a for a, ds in zip(shards(A), shards(dd))])
    S64 = _rank_order_sum([(a - m64).T @ ((a - m64) * ds[:, None]) for a, ds in zip(shards(A), shards(dd))])
    _inside("mu sharded", m64, mu, bm, 0.5)
    _inside("S sharded", S64, Sref, b, 0.5)


@pytest.mark.parametrize("case", SCORE_CASES, ids=lambda c: "q%d-levels%d-mask_%s" % c)
def test_score_sums_reference_fits_the_bounds_when_sharded(case):
    Pred, Y, mask = score_case(*case)
    ref, A = S.ref_score_sums(Pred, Y, mask)
    m_sel = N if mask is None else int(np.count_nonzero(mask))
    b = S.bound_score_sums(A, m_sel)
    _inside("rounded", np.asarray(ref, dtype=np.float64), ref, b)
    parts = [S.ref_score_sums(pr, y, mk, t=np.float64)[0] for pr, y, mk in zip(shards(Pred), shards(Y), shards(mask) if mask is not None else [None] * 3)]
    if mask is not None:
        assert not np.any(parts[0]), "rank 0 selects nothing: its contribution is zero"
    _inside("sharded", _rank_order_sum(parts), ref, b, 0.5)


@pytest.mark.parametrize("case", SCORE_LV_CASES, ids=lambda c: "q%d-kfit%d-mask_%s" % c)
def test_score_sums_lv_reference_fits_the_bounds_when_sharded(case):
    T, Cm, ym, ys, Y, mask = score_lv_case(*case)
    kfit = case[1]
    for lo, hi in ((0, kfit), (kfit, kfit + 2)):
        ref, b = S.ref_score_sums_lv(T, Cm, ym, ys, Y, mask, lo, hi)
        _inside("rounded", np.asarray(ref, dtype=np.float64), ref, b)
        parts = [S.ref_score_sums_lv(t, Cm, ym, ys, y, mk, lo, hi, t=np.float64)[0]
                 for t, y, mk in zip(shards(T), shards(Y), shards(mask) if mask is not None else [None] * 3)]
        _inside("sharded", _rank_order_sum(parts), ref, b, 0.5)


# ---------------------------------------------------------------------------------------------------- 3. the class-C fits: cases and data
# name: (rows per rank, p, q, nlv, algorithms)
ALGS = ("plskern", "plsnipals", "plssimp", "plsrosa", "plswold", "plskern_v1")
FIT_CASES = {
    "small-shard": ((3, 97, 97), 37, 3, 5, ALGS),               # a shard below min(p, nlv): it fetches the global row count (fit.hip)
    "global-clamp": ((1, 2, 3), 9, 1, 8, ALGS),                 # nlv clamps to the GLOBAL row count, 6
    "zero-weight-shard": ((40, 60, 50), 37, 3, 4, ALGS),        # rank 1's weights are all zero
    "generic-q": ((64, 65, 21), 37, 17, 4, ALGS),               # q > 16: the generic small-state kernels (all-reduces of deflate.hip)
    "generic-p": ((64, 65, 21), 2049, 2, 3, ("plskern", "plssimp", "plswold")),   # p > 2048
}
CLAMP_COMPARED = 4                                              # LVs of the global-clamp case that are compared
# R = W inv(P'W) of plsnipals / plsrosa / plswold involves ALL computed LVs.  In the global-clamp case LV 6 is 0 / 0 (six weighted-centred rows have
# rank 5): the oracle's own leading columns of R then differ from those of its 4-LV fit by O(1) (asserted below), so there is no reference for R of
# these three there; T, P, W, C, TT are per-LV quantities and are compared.  plskern and plssimp build R column by column from earlier LVs only.
R_HAS_NO_REFERENCE = {("global-clamp", "plsnipals"), ("global-clamp", "plsrosa"), ("global-clamp", "plswold")}


@lru_cache(maxsize=None)
def fit_data(name):
    """X, Y, weights of a fit case (concatenated rows) and the rank edges.  Latent structure plus noise, so that the compared LVs are well separated."""
    rows, p, q, nlv, _ = FIT_CASES[name]
    n = sum(rows)
    rng = np.random.default_rng(2029 + n + p + q)
    k = 2 * nlv
    Lt = rng.standard_normal((n, k))
    X = Lt @ rng.standard_normal((k, p)) + 0.5 * rng.standard_normal((n, p)) + 2.0
    Y = Lt @ rng.standard_normal((k, q)) + 0.3 * rng.standard_normal((n, q))
    w = rng.uniform(0.5, 1.5, n)
    edges = np.concatenate([[0], np.cumsum(rows)])
    if name == "zero-weight-shard":
        w[edges[1]:edges[2]] = 0.0
    out = (np.asfortranarray(X), np.asfortranarray(Y), w, edges)
    for a in out:
        a.setflags(write=False)
    return out


def oracle_fit(alg, X, Y, w, nlv, scal=False):
    with np.errstate(all="ignore"):                              # (a zero LV, a zero weight under plswold: 0 / 0 in the reference, on purpose)
        return getattr(O, "plskern" if alg == "plskern_v1" else alg)(X, Y, w, nlv=nlv, scal=bool(scal))


def test_the_oracle_on_the_fit_cases():
    """The global clamp gives 6 LVs of which the first four are those of a 4-LV fit; R of the three W inv(P'W) algorithms is not (see above)."""
    X, Y, w, edges = fit_data("global-clamp")
    assert edges[-1] == 6
    for alg in ALGS:
        a, b = oracle_fit(alg, X, Y, w, 8), oracle_fit(alg, X, Y, w, CLAMP_COMPARED)
        assert a.T.shape[1] == 6
        for f in ("T", "P", "W", "C"):
            assert O.rel_fro(getattr(b, f), getattr(a, f)[:, :CLAMP_COMPARED]) < 1e-12, (alg, f)
        r = O.rel_fro(b.R, a.R[:, :CLAMP_COMPARED])
        assert (r > 1e-6) == (("global-clamp", alg) in R_HAS_NO_REFERENCE), (alg, r)
    for name, (rows, p, q, nlv, algs) in FIT_CASES.items():
        X, Y, w, edges = fit_data(name)
        assert X.shape == (sum(rows), p) and Y.shape[1] == q and list(np.diff(edges)) == list(rows)
    rows, p, q, nlv, _ = FIT_CASES["small-shard"]
    assert min(rows) < min(p, nlv) <= sorted(rows)[1]
    X, Y, w, edges = fit_data("zero-weight-shard")
    assert not np.any(w[edges[1]:edges[2]]) and np.all(w[:edges[1]] > 0)
