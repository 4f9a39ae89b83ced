"""What the in-place PLS fits (`desc->inplace = 1`: the reference's plskern!, plssimp!, plsrosa!, plsnipals!, plswold!) leave in the caller's
X and Y, without a GPU: plain restatements in np.longdouble, the per-element bounds the GPU tests hold the kernels to
(tests/test_gpu_inplace.py imports everything from here), the check that the float64 oracle alone does not use the bounds up, and the check
that the case lists reach every route of the library that writes X or Y.

Restatements.  d = w / sum w, mu = d'X and, with scal, s_j = sqrt(sum_i d_i (x_ij - mu_j)^2) (else s = 1; jch_plskern_fit_scaled: s = the
caller's divisors) are taken in longdouble from the raw inputs; Xc = (X - mu) / s and Yc likewise.  Given a fitted model (T, P, C):

    plskern!, plssimp!   X = Xc                         Y = Yc                          (oracle/plsr_oracle.py plskern_, plssimp_)
    plsrosa!             X = Xc                         Y = Yc - T C'                   (plsrosa_)
    plsnipals!           X = Xc - T P'                  Y = Yc - T C'                   (plsnipals_)
    plswold!             X_i = sqrt(d_i) (Xc - T P')_i  Y_i = sqrt(d_i) (Yc - T C')_i   (plswold_; a row with d_i = 0 is exactly 0 whatever T
                                                                                         holds there: the oracle's score of such a row is NaN)

Bounds, per element; gamma(k) = k eps / (1 - k eps) as in test_accessors_static, whose bound_means and bound_stds are the bounds dm_j and ds_j
of the mean and the std the library subtracts and divides by.  Nothing is tuned to what the kernels deliver.

  centring   the kernel forms fl(fl(x - m) / v) with |m - mu| <= dm, |v - s| <= ds.  Exactly, (x - m) / v - (x - mu) / s = (mu - m) / v +
             (x - mu) (1 / v - 1 / s), which is at most dm / (s - ds) + |x - mu| ds / (s (s - ds)); the subtraction rounds once, the division
             once, or twice when it is a product with a rounded reciprocal: gamma(3) |x - m| / v (gamma(1) without a division).  So
                 bc = (dm + |x - mu| ds / (s - ds)) / (s - ds) + gamma(3 | 1) (|x - mu| + dm) / (s - ds),
             with ds = 0 for caller-supplied divisors and without scal.
  deflation  every rank-one step x <- x - t_a p_a multiplies once and subtracts once: 2 nlv roundings in either order of the steps, with or
             without FMA, in one flush of several pending steps or one at a time, and likewise for a sum over a of t_a c_a subtracted once
             (k_ydeflate_all); each intermediate is at most |Xc| + |T||P|' in magnitude.  Four more roundings for what surrounds the steps
             (the oracle's plswold divides its scores by sqrt(d) before they are compared with sqrt(d) T): the centring error passes through
             unchanged, so   bd = bc + gamma(2 nlv + 4) (|Xc| + |T||P|'),   and the same with C for Y.
  plswold!   the factor sqrt(d_i): d_i = w_i / sum w carries gamma(n + 1) (an n-term sum of non-negative weights and a division), the root
             halves that and rounds once, the product rounds once:   bw = sqrt(d_i) (bd + (gamma(n + 2) / 2 + gamma(2)) (|Xc| + |T||P|' + bd)).

The float64 oracle's own in-place outputs, taken with the oracle's own T, P, C, stay within half of these bounds on every case below
(test_oracle_uses_half_the_bound_at_most; measured: 0.12 at most).  One case asks for a latent variable that does not exist (3 x 5, nlv = 3:
centred data of 3 rows has rank 2); there the oracle, like the reference, returns NaN or noise, and it runs with the two that exist
(well_posed_nlv), while the library runs the case as listed.
"""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_accessors_static as A  # noqa: E402
from test_accessors_static import LD, gamma, ld  # noqa: E402
from oracle import plsr_oracle as O  # noqa: E402

CUS = 256                          # compute units of an MI355X: the launch rules below restate prologue.hip's for it
SWEEP_MAXP = 2048                  # jch_internal.h JCH_SWEEP_MAXP
NIPALS_DEFER_DEFAULT = 6           # jch_internal.h JCH_NIPALS_DEFER_DEFAULT
ALGOS = ("plskern", "plssimp", "plsrosa", "plsnipals", "plswold")
KERN_LIKE = ("plskern", "plssimp", "plsrosa")      # X goes back from the centring kernel; the others export the deflated working copy
DEFLATES_Y = ("plsrosa", "plsnipals", "plswold")

# ==================================================================================================== shapes (shared with the GPU file)
# (n, p, q, nlv): each the smallest shape at which an edge of a kernel still exists
CASES = [
    (2, 1, 1, 1), (3, 5, 2, 3), (33, 7, 1, 3),     # less than one 64 x 64 tile, less than one 32-row unit
    (65, 129, 16, 5),                              # one past a tile both ways; q = 16: the last width with the fused write-back
    (97, 40, 17, 6),                               # q > 16: two Y groups, X back through the export kernel, eager deflation; nlv = the flush period
    (131, 513, 3, 7),                              # p crosses the panel kernel's 512-column group; nlv = 6 + 1: one correction pending at the last flush
    (257, 130, 9, 12),                             # nlv = 2 x 6; q = 9: a second group of 8 in k_ydeflate_all
    (200, 2049, 2, 4),                             # p > JCH_SWEEP_MAXP: generic path, eager deflation, odd p with an even working pitch, nlv < 6
]
# more row chunks than blocks launched, so that the grid-stride loops run: (case, the one storage variant it runs with, the loop meant)
BIG_CASES = [
    ((4131, 513, 3, 7), "dev-ld+1", "panel-units"),    # more 32-row units than blocks: the launcher's clamp of the grid no longer binds
    ((8258, 513, 3, 7), "dev-ld+0", "panel"),          # more 64-row tiles than blocks: the panel kernel's row loop takes a second trip
    ((8225, 513, 3, 5), "dev-ld+0", "tile"),           # odd ld: the tile kernel, more chunks than row slots
    ((2113, 2049, 2, 3), "dev-ld+1", "export"),        # the export of the deflated copy, more chunks than row slots
]
SCALS = (False, True)
WKINDS = (None, "random", "zeros")                   # no weights, random in [0.3, 1.7], the same with every 7th exactly 0
# storage variants of the in-place test: (name, host, ld - n, matrix starts 8 bytes into a 16-byte aligned allocation)
STORAGE = [("dev-ld+0", False, 0, False), ("dev-ld+1", False, 1, False), ("dev-ld+3", False, 3, False), ("dev-mis", False, 0, True),
           ("host-ld+0", True, 0, False), ("host-ld+3", True, 3, False)]
FLUSH_CASE, FLUSH_NLVS = (257, 130, 3), (1, 5, 6, 7, 11, 12, 13)
SCALED_CASE = (131, 513, 3, 4)
SHARD_CASE, SHARD_CUT = (257, 130, 3, 7), 0.3


def case_id(c):
    return "n%d-p%d-q%d-a%d" % tuple(c)


def storage_of(case):
    """The storage variants a case runs with: all six, or the one of a big case."""
    for c, name, _ in BIG_CASES:
        if c == tuple(case):
            return [s for s in STORAGE if s[0] == name]
    return STORAGE


# ==================================================================================================== the routes (restated launch rules)
def _cdiv(a, b):
    return -(-a // b)


def lazy_pitch(ldr):
    return 128 * (1 if ldr <= 128 else 2 if ldr <= 256 else 4 if ldr <= 512 else 8 if ldr <= 1024 else 16)


def lazy_capacity(ldr, q):
    """sweep.hip jch_nipals_lazy_capacity: the postponed deflations the lazy kernels hold (0: outside their envelope, eager deflation)."""
    if ldr < 2 or ldr > 2048 or q < 1 or q > 16:
        return 0
    lds_cap = min((144 * 1024) // (8 * lazy_pitch(ldr)), 16)
    if q <= 4 and not (ldr > 1024 and q > 2):
        return lds_cap
    if ldr > 1024:
        return min(lds_cap, 8)
    return 6 if ldr <= 512 else 3


def defer_period(p, q, knob=NIPALS_DEFER_DEFAULT):
    """fit.hip: the rows are rewritten every defer_m-th latent variable (1: eager)."""
    return max(1, min(knob, lazy_capacity((p + 1) & ~1, q)))


def centre_route(n, p, q, ld, aligned, writeback):
    """prologue.hip jch_launch_center_xty for 256 CUs: (kernel, how X goes back, whether a block takes more than one row tile)."""
    ldr, qpad = (p + 1) & ~1, _cdiv(q, 16) * 16
    tiles = _cdiv(n, 64)
    if qpad == 16 and ld % 2 == 0 and aligned:
        groups = _cdiv(ldr, 512)
        nbx = min(max(1, CUS // groups), _cdiv(n, 32))
        return "panel", ("fused" if writeback else None), tiles > nbx
    ptiles, ygroups = _cdiv(ldr, 64), qpad // 16
    nbx = max(1, min(_cdiv(CUS * 3, ptiles * ygroups), tiles))
    return "tile", (None if not writeback else "fused" if ygroups == 1 else "export"), tiles > nbx


def export_loops(n, p, with_x):
    """prologue.hip jch_launch_export_colmajor: whether a block takes more than one 64-row chunk."""
    ptiles = _cdiv(p, 64) if with_x else 1
    return _cdiv(n, 64) > _cdiv(CUS * 4, ptiles)


def routes(alg, case, scal, host, pad, mis):
    """The names of the X- and Y-writing routes one in-place fit takes (the host route stages with ld = n in an aligned buffer)."""
    n, p, q, nlv = case
    nlv = min(n, p, nlv)
    ld_, al = (n, True) if host else (n + pad, not mis)
    kern, back, loops = centre_route(n, p, q, ld_, al, alg in KERN_LIKE)
    sc = "scal" if scal else "noscal"
    out = set()
    if alg in KERN_LIKE:
        out.add(f"{kern}-{back}-{sc}")
        if loops:
            out.add(f"{kern}-{back}-row-loop")
        if kern == "panel" and _cdiv(n, 32) > max(1, CUS // _cdiv((p + 1) & ~1, 512)):
            out.add("panel-grid-not-clamped")
        if back == "export" and export_loops(n, p, True):
            out.add("export-row-loop")
        if alg == "plsrosa":
            out.add("ydeflate_all-%d-groups" % _cdiv(q, 8))
    else:
        m = defer_period(p, q)
        how = "eager" if m == 1 else "lazy-%d-pending-at-the-end" % ((nlv - 1) % m + 1)
        out.add("export-%s%s" % (how, "-sqrtd" if alg == "plswold" else ""))
        out.add("export-" + ("eager" if m == 1 else "lazy") + ("-sqrtd" if alg == "plswold" else ""))
        out.add(f"{kern}-no-writeback")
        if export_loops(n, p, True):
            out.add("export-row-loop")
    return out


def all_routes():
    got = set()
    for case in CASES + [c for c, _, _ in BIG_CASES]:
        for _, host, pad, mis in storage_of(case):
            for alg in ALGOS:
                for scal in SCALS:
                    got |= routes(alg, case, scal, host, pad, mis)
    return got


# ==================================================================================================== inputs
@functools.lru_cache(maxsize=2)
def inplace_data(case):
    """Latent structure plus noise, column offsets in [-3, 3] (as tests/test_gpu_fuzz.py): every latent variable is well defined.  The arrays
    are shared between the tests: every user copies them."""
    n, p, q, nlv = case
    rng = np.random.default_rng(A._seed(n, p, q, nlv, 23))
    k = max(nlv + 2, 4)
    Lt = rng.standard_normal((n, k))
    X = np.asfortranarray(Lt @ rng.standard_normal((k, p)) * rng.uniform(0.5, 2.0, p) + 0.3 * rng.standard_normal((n, p)) + rng.uniform(-3, 3, p))
    ky = min(k, max(q, 2))
    Y = np.asfortranarray(Lt[:, :ky] @ rng.standard_normal((ky, q)) + 0.2 * rng.standard_normal((n, q)) + 1.0)
    return X, Y


def inplace_weights(n, wkind):
    if wkind is None:
        return None
    w = np.random.default_rng(A._seed(n, 29)).uniform(0.3, 1.7, n)
    if wkind == "zeros":
        w[3::7] = 0.0
    return w


# ==================================================================================================== references and bounds
class Centred:
    """Xc, Yc (longdouble), their bounds bX, bY (float64), the normalised weights d (longdouble) and the number of rows behind sum w."""


def _centre_one(M, w, scal, div, rows):
    mean, std = A.ref_col_stats(M, w)
    dm = A.bound_means(M, w)
    dev = ld(M[rows]) - mean
    a = np.abs(np.asarray(dev, dtype=np.float64))
    if div is not None:
        s, ds, k = ld(div), 0.0, 3
    elif scal:
        s, ds, k = std, A.bound_stds(M, w), 3
    else:
        s, ds, k = np.ones(M.shape[1], dtype=LD), 0.0, 1
    s_lo = np.asarray(s, dtype=np.float64) - ds
    assert np.all(s_lo > 0.0), "a column's std is not separated from 0: the bound does not exist"
    return dev / s, (dm + a * ds / s_lo) / s_lo + gamma(k) * (a + dm) / s_lo


def centred(X, Y, w, scal, xdiv=None, ydiv=None, rows=slice(None)):
    """`rows`: keep these rows only (the statistics are those of all the rows)."""
    c = Centred()
    c.Xc, c.bX = _centre_one(X, w, scal, xdiv, rows)
    c.Yc, c.bY = _centre_one(Y, w, scal, (None if xdiv is None else np.ones(Y.shape[1]) if ydiv is None else ydiv), rows)
    c.d, c.n = A._norm_weights(w, X.shape[0])[rows], X.shape[0]
    return c


def _deflate(Mc, b, T, L, nlv):
    Ta, La = np.abs(np.asarray(T, dtype=np.float64)), np.abs(np.asarray(L, dtype=np.float64))
    mag = np.abs(np.asarray(Mc, dtype=np.float64)) + Ta @ La.T
    return Mc - ld(T) @ ld(L).T, b + gamma(2 * nlv + 4) * mag, mag


def expected(alg, c, T, P, Cm, rows=slice(None)):
    """What `alg`! leaves in X and Y for the model (T, P, C) and the bounds: (X, bX, Y, bY), X and Y in longdouble.  `rows`: the rows of the
    centred data T belongs to (a rank's shard)."""
    Xc, Yc, bX, bY, d = c.Xc[rows], c.Yc[rows], c.bX[rows], c.bY[rows], c.d[rows]
    nlv = T.shape[1]
    if alg == "plswold":                                                    # a row without weight is 0 whatever its score holds
        T = np.where((np.asarray(d, dtype=np.float64) == 0.0)[:, None], 0.0, T)
    magX = magY = None
    if alg not in KERN_LIKE:
        Xc, bX, magX = _deflate(Xc, bX, T, P, nlv)
    if alg in DEFLATES_Y:
        Yc, bY, magY = _deflate(Yc, bY, T, Cm, nlv)
    if alg == "plswold":
        r = np.sqrt(d)
        r64, frel = np.asarray(r, dtype=np.float64)[:, None], 0.5 * gamma(c.n + 2) + gamma(2)
        Xc, Yc = r[:, None] * Xc, r[:, None] * Yc
        bX, bY = r64 * (bX + frel * (magX + bX)), r64 * (bY + frel * (magY + bY))
    return Xc, bX, Yc, bY


def well_posed_nlv(case):
    """The latent variables of a case that exist: centred data of n rows has rank n - 1 at most.  Beyond that (3 x 5 with nlv = 3) a score is
    rounding noise or exactly 0, and the reference and the oracle return NaN (plsrosa, plssimp: 0 / 0) or noise: the oracle runs with this many,
    the library with the case's own nlv and is compared with the oracle on these leading ones."""
    n, p, q, nlv = case
    return max(1, min(nlv, n - 1, p))


def oracle_inplace(alg, X, Y, w, nlv, scal):
    """The float64 oracle's `!` form on copies: (model, X after, Y after)."""
    Xo, Yo = np.array(X, order="F"), np.array(Y, order="F")
    with np.errstate(invalid="ignore", divide="ignore"):                    # (plswold: 0 / 0 in the scores of the rows without weight)
        fm = getattr(O, alg + "_")(Xo, Yo, w, nlv=nlv, scal=scal)
    return fm, Xo, Yo


# ==================================================================================================== the static checks
def test_longdouble_is_extended_precision():
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is not wider than float64 here: the references would be no reference"


def test_the_case_lists_reach_every_route():
    got = all_routes()
    need = {
        # the panel kernel with the fused write-back, the tile kernel with it (odd ld, misaligned X), the unfused q > 16 route
        "panel-fused-scal", "panel-fused-noscal", "tile-fused-scal", "tile-fused-noscal", "tile-export-scal", "tile-export-noscal",
        # the export of the deflated copy, lazy and eager, with and without sqrt(d); the pending counts of the last flush
        "export-lazy", "export-eager", "export-lazy-sqrtd", "export-eager-sqrtd",
        "export-lazy-1-pending-at-the-end", "export-lazy-6-pending-at-the-end",
        "panel-no-writeback", "tile-no-writeback",
        "ydeflate_all-1-groups", "ydeflate_all-2-groups", "ydeflate_all-3-groups",
        # the grid-stride loops
        "panel-fused-row-loop", "tile-fused-row-loop", "export-row-loop", "panel-grid-not-clamped",
    }
    assert need <= got, sorted(need - got)
    # which case is meant for which route
    r = lambda alg, case, name: routes(alg, case, True, *[s for s in STORAGE if s[0] == name][0][1:])   # noqa: E731
    assert "panel-fused-scal" in r("plskern", (65, 129, 16, 5), "dev-ld+1") and "tile-fused-scal" in r("plskern", (65, 129, 16, 5), "dev-ld+0")
    assert "tile-fused-scal" in r("plssimp", (200, 2049, 2, 4), "dev-mis") and "panel-fused-scal" in r("plssimp", (200, 2049, 2, 4), "host-ld+3")
    assert "tile-export-scal" in r("plsrosa", (97, 40, 17, 6), "dev-ld+1") and "export-eager" in r("plsnipals", (97, 40, 17, 6), "dev-ld+0")
    assert "export-lazy-1-pending-at-the-end" in r("plsnipals", (131, 513, 3, 7), "dev-ld+0")
    assert "export-lazy-6-pending-at-the-end-sqrtd" in r("plswold", (257, 130, 9, 12), "dev-ld+0") and defer_period(130, 9) == 6
    assert "export-eager-sqrtd" in r("plswold", (200, 2049, 2, 4), "dev-ld+0") and defer_period(2049, 2) == 1 and defer_period(40, 17) == 1
    for (case, name, loop), alg, want in zip(BIG_CASES, ("plskern", "plskern", "plsrosa", "plswold"),
                                             ("panel-grid-not-clamped", "panel-fused-row-loop", "tile-fused-row-loop", "export-row-loop")):
        assert want in r(alg, case, name), (case, name, want)
    assert "panel-fused-row-loop" not in r("plskern", (4131, 513, 3, 7), "dev-ld+1")   # (its 65 tiles fit the 128 blocks: why 8258 is there too)
    # the flush arithmetic cases: every number of corrections pending at the last flush of a period of 6, one to six
    assert defer_period(FLUSH_CASE[1], FLUSH_CASE[2]) == 6 and {(a - 1) % 6 + 1 for a in FLUSH_NLVS} == {1, 5, 6}
    assert {a // 6 for a in FLUSH_NLVS} == {0, 1, 2}
    assert all(c[3] <= min(c[0], c[1]) for c in CASES) and SHARD_CASE[3] % 6 == 1


def _half_rows(name, got, ref, bound):
    return A._half(name, got, ref, bound)


PARAMS = [(c, s, w) for c in CASES + [b[0] for b in BIG_CASES] for s in SCALS for w in WKINDS]


@pytest.mark.parametrize("case,scal,wkind", PARAMS, ids=["%s-%s-w_%s" % (case_id(c), "scal" if s else "noscal", w) for c, s, w in PARAMS])
def test_oracle_uses_half_the_bound_at_most(case, scal, wkind):
    n, p, q, nlv = case
    X, Y = inplace_data(case)
    w = inplace_weights(n, wkind)
    rows = A._rows_subset(n)                                                # (a long case: its first, middle and last 64 rows)
    c = centred(X, Y, w, scal, rows=rows)
    for alg in ALGOS:
        fm, Xo, Yo = oracle_inplace(alg, X, Y, w, well_posed_nlv(case), scal)
        assert fm.T.shape[1] == well_posed_nlv(case)
        Xe, bX, Ye, bY = expected(alg, c, fm.T[rows], fm.P, fm.C)
        if alg == "plswold" and wkind == "zeros" and n > 3:
            zero = w[rows] == 0.0
            assert zero.any() and np.isnan(fm.T[rows][zero]).all() and not np.any(Xo[rows][zero]) and not np.any(Yo[rows][zero])
            assert not np.any(np.asarray(Xe[zero], dtype=np.float64)) and not np.any(bX[zero]) and not np.any(bY[zero])
        _half_rows(f"{alg}! X", Xo[rows], Xe, bX)
        _half_rows(f"{alg}! Y", Yo[rows], Ye, bY)


def test_the_scaled_and_the_sharded_references():
    """Caller-supplied divisors: the centring bound without its std term; a shard: the rows of the restatement on all the rows."""
    n, p, q, nlv = SCALED_CASE
    X, Y = inplace_data(SCALED_CASE)
    rng = np.random.default_rng(5)
    xdiv, ydiv = rng.uniform(0.5, 2.0, p), rng.uniform(0.5, 2.0, q)
    w = inplace_weights(n, "random")
    c = centred(X, Y, w, False, xdiv, ydiv)
    d = w / w.sum()
    _half_rows("scaled X", (X - d @ X) / xdiv, c.Xc, c.bX)
    _half_rows("scaled Y", (Y - d @ Y) / ydiv, c.Yc, c.bY)
    c1 = centred(X, Y, w, False, xdiv, None)                                # yscales_in = NULL: ones
    _half_rows("scaled Y, no divisors", Y - d @ Y, c1.Yc, c1.bY)
    n, p, q, nlv = SHARD_CASE
    X, Y = inplace_data(SHARD_CASE)
    w = inplace_weights(n, "zeros")
    c = centred(X, Y, w, True)
    cut = int(SHARD_CUT * n)
    assert 0 < cut < n - cut
    for alg in ("plskern", "plsnipals", "plswold"):
        fm, Xo, Yo = oracle_inplace(alg, X, Y, w, nlv, True)
        for rows in (slice(0, cut), slice(cut, n)):
            Xe, bX, Ye, bY = expected(alg, c, fm.T[rows], fm.P, fm.C, rows)
            _half_rows(f"{alg}! X shard", Xo[rows], Xe, bX)
            _half_rows(f"{alg}! Y shard", Yo[rows], Ye, bY)
