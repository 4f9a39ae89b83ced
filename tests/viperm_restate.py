"""Restatements for the permutation-importance tests (tests/test_viperm_static.py, tests/test_gpu_viperm.py), none of which needs a GPU:

  * the permutation generator of jch_perm_fill as include/jchemo_hip.h defines it, in numpy uint64 arithmetic;
  * src/viperm.jl:74-110 and src/isel.jl:76-129 taken literally, on given held-out rows and given permutations;
  * the six sums of jch_perm_score_sums in np.longdouble, and the per-sum bound the kernel is held to.

Bound.  eps = 2^-52, gamma(k) = k eps / (1 - k eps).  Per element the kernel forms d = x_b - x_a, t = d B, s = pred + t, e = y - s: four
operations (three with a fused multiply-add) on intermediates none of which exceeds
    M_ik = |y_ik| + |pred_ik| + (|x_a| + |x_b|)_i |B_jk|
in magnitude, so the computed residual is within be = gamma(4) M of the exact one WHATEVER e itself is (a bound from |e| cannot hold: a
row whose residual is small against its prediction has an error of eps |pred|).  A sum of m terms in ANY order is within gamma(m) of the
sum of the terms' magnitudes.  Hence, with one gamma per summation and a factor 2 as in tests/test_accessors_static.py:
    sum e     2 gamma(m + 4) sum M                                  (the terms |e^| <= M (1 + gamma(4)), plus sum be)
    sum e^2   (2 gamma(m + 4) + 3 gamma(4)) sum M^2                 (|e^2 - e^^2| <= (2 M + be) be, the square's own rounding)
    sum y e   (2 gamma(m + 4) + 2 gamma(4)) sum |y| M               (|y| be, the product's own rounding)
    sum y     2 gamma(m + 1) sum |y|;    sum y^2   2 gamma(m + 2) sum y^2;    count   exact.
The magnitudes are taken in float64 (the bound's own rounding is far below its slack)."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
C1, C2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
M_LIST = (1, 2, 3, 7, 33, 64, 65, 1000, 2 ** 16, 2 ** 16 + 1)


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


# ---------------------------------------------------------------------------------------------------- the generator
def mix64(z):
    """The splitmix64 finaliser on a uint64 array (arithmetic modulo 2^64)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(C1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(C2)
    return z ^ (z >> np.uint64(31))


def perm_bits(m):
    b = 2
    while (1 << b) < m:
        b += 2
    return b


def perm_rounds(b):
    return 24 if b <= 12 else 8


def perm_keys(seed, cols):
    """key_j = mix64(seed + (j + 1) G) for the column numbers `cols`."""
    j = np.asarray(cols, dtype=np.uint64)
    return mix64(np.uint64(seed & M64) + (j + np.uint64(1)) * np.uint64(GOLDEN))


def perm_matrix(seed, m, ncols, j0=0):
    """m x ncols int32: column c = pi_{j0 + c}(0 .. m - 1) for `seed`, as jch_perm_fill defines it."""
    b = perm_bits(m)
    h, rounds = b // 2, perm_rounds(b)
    mask = np.uint64((1 << h) - 1)
    keys = perm_keys(seed, np.arange(j0, j0 + ncols))
    v = np.repeat(np.arange(m, dtype=np.uint64)[:, None], ncols, axis=1).reshape(-1)     # row-major (i, c)
    kk = np.tile(keys, m)
    todo = np.arange(v.size)
    with np.errstate(over="ignore"):
        while todo.size:
            x, key = v[todo], kk[todo]
            L, R = x >> np.uint64(h), x & mask
            rk = key.copy()
            for _ in range(rounds):
                rk = rk + np.uint64(GOLDEN)
                f = mix64(rk ^ R) >> np.uint64(64 - h)
                L, R = R, L ^ f
            x = (L << np.uint64(h)) | R
            v[todo] = x
            todo = todo[x >= np.uint64(m)]                                               # cycle walking: these go round again
    return v.reshape(m, ncols).astype(np.int32)


# ---------------------------------------------------------------------------------------------------- literal restatements
def rmrow(A, s):
    return np.delete(A, s, axis=0)


def np_scores():
    """src/scores.jl, per column of (pred, Y): 1 x q each."""
    def ssr(pred, Y):
        return ((pred - Y) ** 2).sum(axis=0, keepdims=True)

    def msep(pred, Y):
        return ((pred - Y) ** 2).mean(axis=0, keepdims=True)

    def rmsep(pred, Y):
        return np.sqrt(msep(pred, Y))

    def bias(pred, Y):
        return (pred - Y).mean(axis=0, keepdims=True)

    def r2(pred, Y):
        return 1.0 - msep(pred, Y) / ((Y - Y.mean(axis=0)) ** 2).mean(axis=0, keepdims=True)

    def cor2(pred, Y):
        pc, yc = pred - pred.mean(axis=0), Y - Y.mean(axis=0)
        return ((pc * yc).sum(axis=0) ** 2 / ((pc ** 2).sum(axis=0) * (yc ** 2).sum(axis=0)))[None, :]

    return dict(ssr=ssr, msep=msep, rmsep=rmsep, bias=bias, r2=r2, cor2=cor2)


def viperm_literal(X, Y, s, perms, score, fun, predict):
    """src/viperm.jl:89-109 with the held-out rows s[i] and the shuffles perms[i][:, j] given (0-based).  (imp, res, score0 (q x perm)); a
    `score` that returns several scores side by side (1 x k q) gives k q columns."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    p, nrep = X.shape[1], len(s)
    res = score0s = None
    for i in range(nrep):
        Xcal, Ycal = rmrow(X, s[i]), rmrow(Y, s[i])
        Xval, Yval = X[s[i], :], Y[s[i], :]
        fm = fun(Xcal, Ycal)
        score0 = np.asarray(score(np.asarray(predict(fm, Xval)), Yval)).reshape(-1)
        if res is None:
            res, score0s = np.empty((p, score0.size, nrep)), np.empty((score0.size, nrep))
        score0s[:, i] = score0
        for j in range(p):
            zXval = Xval.copy()
            zs = perms[i][:, j]
            zXval[:, j] = zXval[zs, j]
            res[j, :, i] = np.asarray(score(np.asarray(predict(fm, zXval)), Yval)).reshape(-1) - score0
    return res.mean(axis=2), res, score0s


def isel_intervals(p, nint):
    """src/isel.jl:84-87, 1-based: [lo up mid]; Julia's `round` is half to even (np.rint)."""
    z = np.rint(np.linspace(1, p + 1, nint + 1))
    it = np.stack([z[:nint], z[1:] - 1], axis=1)
    return np.concatenate([it, np.rint(it.mean(axis=1, keepdims=True))], axis=1).astype(np.int64)


def isel_literal(X, Y, s, nint, score, fun, predict):
    """src/isel.jl:98-128 with the held-out rows given.  (res (nint x q), res0 (1 x q), res_rep, res0_rep, int 1-based)."""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    p, q, nrep = X.shape[1], Y.shape[1], len(s)
    it = isel_intervals(p, nint)
    res_rep, res0_rep = np.zeros((nint, q, nrep)), np.zeros((1, q, nrep))
    for i in range(nrep):
        Xcal, Ycal = rmrow(X, s[i]), rmrow(Y, s[i])
        Xval, Yval = X[s[i], :], Y[s[i], :]
        fm = fun(Xcal, Ycal)
        res0_rep[:, :, i] = score(np.asarray(predict(fm, Xval)), Yval)
        for j in range(nint):
            u = slice(it[j, 0] - 1, it[j, 1])
            fm = fun(np.asfortranarray(Xcal[:, u]), Ycal)
            res_rep[j, :, i] = np.asarray(score(np.asarray(predict(fm, np.asfortranarray(Xval[:, u]))), Yval)).reshape(-1)
    return res_rep.mean(axis=2), res0_rep.mean(axis=2), res_rep, res0_rep, it


# ---------------------------------------------------------------------------------------------------- the six sums and their bound
def six(y, e, t=LD, order=slice(None)):
    """{sum e, sum e^2, sum y e, sum y, sum y^2, count} over the rows, per column; type t, rows taken in `order`, added one after the other
    (a cumulative sum: numpy's own `sum` is pairwise)."""
    y, e = np.asarray(y, dtype=t)[order], np.asarray(e, dtype=t)[order]
    terms = np.stack([e, e * e, y * e, y, y * y, np.ones_like(y)], axis=-1)               # (m, q, 6)
    return np.cumsum(terms, axis=0, dtype=t)[-1]


def _rows(rows, n, m=None):
    return np.arange(n if m is None else m) if rows is None else np.asarray(rows, dtype=np.int64)


def ref_perm_sums(X, rows, Pred, Y, B, perm, t=LD, order=slice(None)):
    """jch_perm_score_sums in type t, direct form: (p + 1, q, 6); row p with the difference taken as 0."""
    n, p = X.shape
    r = _rows(rows, n)
    Xt, Bt = np.asarray(X, dtype=t), np.asarray(B, dtype=t)
    y, pr = np.asarray(Y, dtype=t)[r], np.asarray(Pred, dtype=t)[r]
    out = np.empty((p + 1, Y.shape[1], 6), dtype=t)
    for j in range(p):
        xa = Xt[r, j]
        d = xa[perm[:, j]] - xa
        out[j] = six(y, y - (pr + d[:, None] * Bt[j][None, :]), t, order)
    out[p] = six(y, y - pr, t, order)
    return out


def bound_perm_sums(X, rows, Pred, Y, B, perm):
    """The bound of the module docstring, (p + 1, q, 6) float64."""
    n, p = X.shape
    r = _rows(rows, n)
    m = r.shape[0]
    ay, ap, aB = np.abs(np.asarray(Y, dtype=np.float64)[r]), np.abs(np.asarray(Pred, dtype=np.float64)[r]), np.abs(np.asarray(B, dtype=np.float64))
    g, g4 = 2.0 * gamma(m + 4), gamma(4)
    out = np.zeros((p + 1, Y.shape[1], 6))
    for j in range(p + 1):
        if j < p:
            xa = np.abs(np.asarray(X, dtype=np.float64)[r, j])
            M = ay + ap + (xa + xa[perm[:, j]])[:, None] * aB[j][None, :]
        else:
            M = ay + ap
        out[j, :, 0] = g * M.sum(axis=0)
        out[j, :, 1] = (g + 3.0 * g4) * (M * M).sum(axis=0)
        out[j, :, 2] = (g + 2.0 * g4) * (ay * M).sum(axis=0)
        out[j, :, 3] = 2.0 * gamma(m + 1) * ay.sum(axis=0)
        out[j, :, 4] = 2.0 * gamma(m + 2) * (ay * ay).sum(axis=0)
    return out


def loop_perm_sums(X, rows, Y, B, intercept, perm, t=LD):
    """The same sums the way the reference gets there: copy the held-out block, shuffle one column, predict as int + X B, take the
    residuals.  (p + 1, q, 6) in type t; row p from the unshuffled block."""
    n, p = X.shape
    r = _rows(rows, n)
    Xval, Yval = np.asarray(X, dtype=t)[r], np.asarray(Y, dtype=t)[r]
    Bt, it = np.asarray(B, dtype=t), np.asarray(intercept, dtype=t).reshape(1, -1)
    out = np.empty((p + 1, Y.shape[1], 6), dtype=t)
    for j in range(p + 1):
        z = Xval.copy()
        if j < p:
            z[:, j] = z[perm[:, j], j]
        out[j] = six(Yval, Yval - (it + z @ Bt), t)
    return out
