"""The accessor and statistics primitives without a GPU: plain restatements in np.longdouble, the per-element bounds the GPU tests hold
the kernels to (tests/test_gpu_accessors.py imports everything from here), and the check that the references alone do not use the bounds up.

    jch_affine_gemm / jch_transform   ref_affine        jch_col_stats      ref_col_stats       jch_score_sums      ref_score_sums
    jch_predict                       ref_predict       jch_weighted_ss    ref_weighted_ss     jch_score_sums_lv   ref_score_sums_lv
                                                        jch_weighted_cov   ref_weighted_cov

Bounds.  gamma(k) = k eps / (1 - k eps), eps = 2^-52: the standard bound of a k-term sum; one gamma per summation, a factor 2 where the
reference and the kernel may each use an order of their own.  Nothing is tuned to what the kernels deliver.

  affine   The library folds the centring into Bs = B ./ scale and bias' = bias - shift'Bs and evaluates X Bs + bias' (gemm.hip), so
           |err_ic| <= gamma(p + 3) (|X| |Bs| + |shift|'|Bs| + |bias|)_ic: a p-term sum plus the division, the folded bias and the final
           addition.  The bound of the FOLDED form grows with |x|, not with |x - shift|.  A product too large for a longdouble matmul
           (m p k > LD_LIMIT) takes float64 BLAS on the CENTRED form as its reference, and the bound the factor 2.
  predict  one GEMM (at most two levels, or m < 4096): the bound above with the stacked coefficient matrices B_a = diag(1 / xscales) R_a
           C_a' diag(yscales), shift = xmeans, bias = ymeans.  Prefix path (three levels or more and m >= 4096): the scores' bound
           bt = gamma(p + 3) (|X| |Rs| + |xmeans|'|Rs|) carried through the running sum, sum_{l <= a} bt_il |Cs_lk| + gamma(a + 2) (|ymeans_k| +
           sum_{l <= a} |t_il| |Cs_lk|), Cs = C' .* yscales.
  means    2 gamma(n + 2) d'|X|, d = w / sum w: the sum of the weights and the weighted sum, n terms each, the division and the product.
  variance v_j = sum_i d_i (x_ij - m_j)^2:  2 gamma(n + 4) v_j  (as the means, plus the square and its product)
           + 2 dm_j d'|x_j - m_j| + dm_j^2  (the mean the kernel subtracts is off by at most dm_j, the means' bound)
           + 2 eps d'(|x_j| |x_j - m_j|)    (the subtraction in registers).
           Through the root: |s - sqrt(v)| <= max(sqrt(v) - sqrt(max(v - bv, 0)), sqrt(v + bv) - sqrt(v)) + eps sqrt(v + bv);
           a constant column (v = 0) may return at most sqrt(bv) (+ its rounding).
  ss       the variance bound with the given shift (dm = 0) and the given d, divided by scale^2 and summed over p, + gamma(p + 2) times the
           p-term host sum itself.
  cov      2 gamma(n + 4) sum_i d_i |ac_ij| |ac_ik| + the mean-error terms sum_i d_i (|ac_ij| dm_k + |ac_ik| dm_j) + dm_j dm_k + the subtraction
           eps sum_i d_i (|a_ij| |ac_ik| + |ac_ij| |a_ik|);  S - S' within twice that;  mu within the means' bound.
  scores   per statistic 2 gamma(m_sel + 3) times the sum of the absolute values of the summands over the selected rows; the row count exact.
           For jch_score_sums_lv the prediction is not an input but a running sum the kernel forms itself, whose rounding bp_i = gamma(a + 2)
           (|ymeans_k| + sum_{l <= a} |t_il| |Cs_lk|) (the prefix term of `predict`, a clamped to kfit) reaches e = y - pred: the three
           statistics of e get sum w bp, sum w (2 |e| + bp) bp and sum w |y| bp on top.  (Without it the bound cannot hold: one selected
           row whose residual is small against its prediction has an error of a eps |pred| against a bound of 4 eps |e|.)
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
LD_LIMIT = 1.0e8            # multiply-adds up to which a product is taken in longdouble (about half a second)
CUS = 256                   # compute units of an MI355X: the dispatch rules below restate gemm.hip's for it


def gamma(k):
    return k * EPS / (1.0 - k * EPS)


def ld(a):
    return None if a is None else np.asarray(a, dtype=LD)


# ==================================================================================================== shapes (shared with the GPU file)
# ---- jch_affine_gemm: (m, p, k, kernel the aligned layout is meant for).  Dispatch (gemm.hip, cus = 256), kpad = k rounded up to 16:
#   k <= 32:  gemm32p<1,4> (kpad 16) / <2,8> (kpad 32) when m >= 65536, m even and the coefficients fit in 150 KiB of LDS (kpad 32: p <= 576);
#             gemm32s when m <= 8192 and p >= 64; gemm32 otherwise
#   k  > 32:  wideout<4|8|16> (p <= 16 | 32 | 64) when m >= 4096 and m even; the general kernel otherwise (grid.y = ceil(kpad / 128))
# (ldx odd or a misaligned X send gemm32p to gemm32 and wideout to the general kernel; ldo odd or a misaligned out select the unpaired
# instantiations of gemm32p and wideout: the storage variants of the GPU file)
AFFINE_TRIPLES = [
    (1, 1, 1, "gemm32"), (31, 3, 15, "gemm32"), (33, 5, 16, "gemm32"), (127, 63, 17, "gemm32"), (129, 16, 32, "gemm32"),
    (4097, 33, 1, "gemm32"), (4098, 4, 17, "gemm32"), (8194, 64, 32, "gemm32-m-above-32cus"), (8194, 130, 16, "gemm32-m-above-32cus"),
    (65537, 17, 16, "gemm32-odd-m"), (65538, 580, 32, "gemm32-lds-too-small"),
    (1, 64, 1, "gemm32s"), (32, 64, 16, "gemm32s"), (33, 65, 17, "gemm32s"), (127, 130, 32, "gemm32s"), (4096, 64, 15, "gemm32s"),
    (8192, 64, 32, "gemm32s-m-at-32cus"), (8192, 130, 1, "gemm32s-m-at-32cus"), (129, 576, 32, "gemm32s"),
    (65536, 1, 1, "gemm32p<1,4>"), (65536, 17, 16, "gemm32p<1,4>"), (65538, 33, 15, "gemm32p<1,4>"), (65538, 64, 16, "gemm32p<1,4>"),
    (65536, 4, 17, "gemm32p<2,8>"), (65536, 65, 32, "gemm32p<2,8>"), (65538, 130, 32, "gemm32p<2,8>"), (65538, 576, 32, "gemm32p<2,8>-lds-limit"),
    (4096, 16, 33, "wideout<4>"), (4098, 1, 128, "wideout<4>"), (8192, 5, 260, "wideout<4>"),
    (4096, 17, 33, "wideout<8>"), (4098, 32, 129, "wideout<8>"),
    (4096, 33, 128, "wideout<16>"), (8194, 64, 260, "wideout<16>"), (65536, 63, 33, "wideout<16>"),
    (1, 1, 33, "general"), (32, 3, 128, "general"), (33, 130, 129, "general-grid.y2"), (127, 65, 260, "general-grid.y3"),
    (129, 17, 260, "general-grid.y3"), (4097, 16, 33, "general-odd-m"), (4096, 65, 33, "general-p-above-64"),
]
AFFINE_BIG = 65538 * 500        # m p above which a triple runs one configuration only (the 300 MB cases)
# (level, shift / scale / bias present): the two configurations of every triple
AFFINE_CONFIGS = [(100.0, True), (0.0, False)]


def affine_kernel(m, p, k, ldx_even=True, x_aligned=True, ldo_even=True, out_aligned=True):
    """The kernel gemm.hip launches for a device-resident call (restated for the ids and the report; no test depends on it)."""
    kpad = (k + 15) // 16 * 16
    fast_x = m % 2 == 0 and ldx_even and x_aligned
    paired = "paired" if (ldo_even and out_aligned) else "unpaired"
    if kpad <= 32:
        ldsp = 8 * (((p + 3) // 4 + 15) // 16 * 64) * (kpad + 1)
        if ldsp <= 150 * 1024 and m >= 65536 and fast_x:
            return ("gemm32p<1,4," if kpad == 16 else "gemm32p<2,8,") + paired + ">"
        if m <= 32 * CUS and p >= 64:
            return "gemm32s"
        return "gemm32"
    if p <= 64 and m >= 4096 and fast_x:
        ks = (p + 3) // 4
        return "wideout<%d,%s>" % (4 if ks <= 4 else 8 if ks <= 8 else 16, paired)
    return "general"


# ---- the cost of the folding, reported at two levels on three kernels of jch_affine_gemm: (m, p, k)
FOLD_CASES = [(4096, 64, 16), (4098, 33, 17), (65536, 65, 32)]
FOLD_LEVELS = [1e2, 1e4]

# ---- jch_transform / jch_predict: (m, q, ldo - m, pred misaligned, means and scales NULL, what the prefix path runs); p and nlv below
PREDICT_P, PREDICT_NLV = 20, 12
PREDICT_RANGES = [(0, 0), (0, 1), (0, 2), (3, 9), (PREDICT_NLV - 2, PREDICT_NLV)]
PREDICT_CASES = [
    (4095, 1, 0, False, False, "one-gemm-only"), (4096, 1, 0, False, False, "prefix<4,V2>"), (4096, 4, 1, False, True, "prefix<4,V1>-odd-ldo"),
    (4096, 5, 0, True, False, "prefix<8,V1>-misaligned"), (4098, 8, 2, False, True, "prefix<8,V2>"), (4097, 9, 0, False, False, "prefix<16,V1>-odd-m"),
    (4098, 17, 0, False, False, "prefix<16,V2>-grid.y2"), (4096, 17, 2, False, True, "prefix<16,V2>-grid.y2"), (4097, 17, 1, False, False, "prefix<16,V1>-odd-m"),
    (4095, 17, 2, True, True, "one-gemm-only"),
]


def predict_path(m, lo, hi):
    return "prefix" if (hi - lo + 1 > 2 and m >= 4096) else "gemm"


# ---- jch_col_stats / jch_weighted_ss: (n, p, level, weights, ldx - n, X misaligned, weights misaligned); column 0 is constant when p >= 2
STATS_CASES = [
    (1, 1, 0.0, None, 0, False, False), (2, 2, 1e4, "random", 1, False, False), (255, 130, 0.0, "zeros", 2, False, False),
    (256, 1, 1e4, None, 0, True, False), (257, 2, 0.0, "random", 0, False, True), (511, 130, 1e4, "zeros", 1, False, False),
    (513, 1, 0.0, "random", 2, True, True), (2047, 2, 1e4, None, 0, False, False), (2048, 130, 0.0, "random", 0, False, False),
    (2048, 2, 1e4, "zeros", 0, False, True), (2049, 2100, 1e4, "zeros", 0, False, False), (2049, 130, 0.0, None, 1, False, False),
    (70001, 2, 1e4, "random", 1, False, False), (70001, 130, 0.0, "zeros", 0, False, False), (70001, 1, 1e4, None, 1, True, False),
]
# ---- jch_weighted_cov: (n, d, level, weights, lda - n)
COV_CASES = [
    (1, 1, 0.0, None, 0), (1, 17, 100.0, "random", 1), (2, 2, 100.0, "random", 0), (2, 65, 100.0, None, 0), (63, 15, 0.0, "zeros", 1),
    (64, 16, 100.0, None, 0), (64, 16, 0.0, "random", 1), (65, 17, 100.0, "zeros", 2), (65, 130, 0.0, None, 0), (257, 63, 0.0, "random", 0),
    (257, 64, 100.0, None, 1), (4097, 16, 100.0, "random", 1), (4097, 65, 0.0, "random", 1), (4097, 130, 100.0, "zeros", 0),
]
# ---- jch_score_sums: (m, q, levels, mask, padding of ldp and ldy)
SCORE_CASES = [
    (1, 1, 1, None, 0), (1, 3, 2, "last", 1), (255, 11, 32, "random", 2), (256, 17, 33, "ones", 0), (257, 1, 64, "zeros", 1),
    (257, 3, 65, "random", 0), (255, 1, 65, "last", 0), (256, 3, 1, "zeros", 0), (70001, 3, 2, "random", 1), (70001, 1, 33, None, 0),
    (70001, 17, 1, "last", 2), (70001, 11, 2, "ones", 0),
]
# ---- jch_score_sums_lv: (m, q, kfit, mask, padding of ldt and ldy, ymeans and yscales NULL)
SCORE_LV_CASES = [
    (1, 1, 0, None, 0, False), (1, 3, 7, "last", 1, False), (255, 11, 12, "random", 2, False), (256, 17, 7, "ones", 0, True),
    (257, 1, 33, "zeros", 1, False), (257, 3, 12, "random", 0, True), (256, 1, 40, "random", 1, False), (70001, 3, 12, "random", 1, False),
    (70001, 1, 0, None, 0, True), (70001, 17, 7, "last", 2, False),
]


def score_lv_ranges(kfit):
    return [(0, 0), (0, kfit), (kfit, kfit + 5), (kfit + 2, kfit + 40), (5, 5 + 32)]


# ==================================================================================================== inputs
def _seed(*parts):
    return int(sum((i + 1) * 7919 * int(v) for i, v in enumerate(parts)) % (2 ** 31))


def affine_data(m, p, k, level, present):
    rng = np.random.default_rng(_seed(m, p, k, level, present))
    X = np.asfortranarray(level + rng.standard_normal((p, m)).T)
    B = np.asfortranarray(rng.standard_normal((p, k)) / np.sqrt(p))
    if not present:
        return X, None, None, B, None
    return X, level + 0.1 * rng.standard_normal(p), rng.uniform(0.5, 2.0, p), B, rng.standard_normal(k)


def fold_data(m, p, k, level):
    rng = np.random.default_rng(m + p)
    X = np.asfortranarray(level + rng.standard_normal((p, m)).T)
    return (X, level + 0.1 * rng.standard_normal(p), rng.uniform(0.5, 2.0, p), np.asfortranarray(rng.standard_normal((p, k)) / np.sqrt(p)),
            rng.standard_normal(k))


def predict_data(m, q, null):
    p, nlv = PREDICT_P, PREDICT_NLV
    rng = np.random.default_rng(_seed(m, q, null, 5))
    X = np.asfortranarray(100.0 + rng.standard_normal((p, m)).T)
    model = dict(R=np.asfortranarray(rng.standard_normal((p, nlv)) / np.sqrt(p)), C=np.asfortranarray(rng.standard_normal((q, nlv))),
                 xmeans=None, xscales=None, ymeans=None, yscales=None)
    if not null:
        model.update(xmeans=100.0 + 0.1 * rng.standard_normal(p), xscales=rng.uniform(0.5, 2.0, p), ymeans=3.0 + rng.standard_normal(q),
                     yscales=rng.uniform(0.5, 2.0, q))
    return X, model


def weights_of(kind, n, rng):
    """NULL, random and unnormalised, or random with a quarter of them zero (at least one stays positive)."""
    if kind is None:
        return None
    w = rng.uniform(0.5, 3.0, n)
    if kind == "zeros":
        w[rng.permutation(n)[: n // 4]] = 0.0
    return w


def stats_data(n, p, level, wkind):
    rng = np.random.default_rng(_seed(n, p, level, 11))
    X = np.asfortranarray(level + rng.standard_normal((p, n)).T)
    if p >= 2:
        X[:, 0] = level + 1.5
    return X, weights_of(wkind, n, rng)


def cov_data(n, d, level, wkind):
    rng = np.random.default_rng(_seed(n, d, level, 13))
    A = np.asfortranarray(level + rng.standard_normal((d, n)).T @ (np.eye(d) + 0.3 * rng.standard_normal((d, d))))
    return A, weights_of(wkind, n, rng)


def mask_of(kind, m, rng):
    if kind is None:
        return None
    if kind == "ones":
        return np.ones(m)
    mask = np.zeros(m)
    if kind == "random":
        mask[rng.random(m) < 0.5] = 1.0
    elif kind == "last":
        mask[m - 1] = 1.0
    return mask


def _nan_unselected(mask, *arrays):
    if mask is not None:
        for a in arrays:
            a[mask == 0.0] = np.nan


def score_data(m, q, levels, mkind):
    """Y, a prediction matrix whose residuals shrink with the level, the mask; NaN in every unselected row."""
    rng = np.random.default_rng(_seed(m, q, levels, 17))
    Y = np.asfortranarray(3.0 + rng.standard_normal((q, m)).T)
    Pred = np.asfortranarray(np.tile(Y, (1, levels)) + rng.standard_normal((levels * q, m)).T / (1.0 + np.repeat(np.arange(levels), q)))
    mask = mask_of(mkind, m, rng)
    _nan_unselected(mask, Y, Pred)
    return Pred, Y, mask


def score_lv_data(m, q, kfit, mkind, null):
    rng = np.random.default_rng(_seed(m, q, kfit, 19))
    T = np.asfortranarray(rng.standard_normal((kfit, m)).T * (1.0 + np.arange(kfit))) if kfit > 0 else None
    Cm = np.asfortranarray(rng.standard_normal((q, kfit)) / (1.0 + np.arange(kfit))) if kfit > 0 else None
    ym = None if null else 3.0 + rng.standard_normal(q)
    ys = None if null else rng.uniform(0.5, 2.0, q)
    Y = (0.0 if null else ym) + 0.3 * rng.standard_normal((m, q))
    if kfit > 0:
        Y = Y + T @ (Cm * (1.0 if null else ys[:, None])).T
    Y = np.asfortranarray(Y)
    mask = mask_of(mkind, m, rng)
    _nan_unselected(mask, Y, *([T] if kfit > 0 else []))
    return T, Cm, ym, ys, Y, mask


# ==================================================================================================== references and bounds
def _or(v, fill, n):
    return np.full(n, fill) if v is None else np.asarray(v)


def folded(p, k, shift, scale, B):
    """|Bs| and |shift|'|Bs| of the folded form (float64: the bound's own rounding is far below its slack)."""
    aBs = np.abs(np.asarray(B) / _or(scale, 1.0, p)[:, None])
    return aBs, np.abs(_or(shift, 0.0, p)) @ aBs


def ref_affine(X, shift, scale, B, bias, exact=None):
    """((X - 1 shift') diag(1 / scale)) B + 1 bias', as the header states it.  Returns (reference, factor): longdouble and 1, or, for a
    product above LD_LIMIT (exact=False), float64 BLAS on the same centred form and 2."""
    m, p = X.shape
    k = B.shape[1]
    if exact is None:
        exact = float(m) * p * k <= LD_LIMIT
    t = LD if exact else np.float64
    Z = (np.asarray(X, dtype=t) - _or(shift, 0.0, p).astype(t)) / _or(scale, 1.0, p).astype(t)
    return Z @ np.asarray(B, dtype=t) + _or(bias, 0.0, k).astype(t), (1.0 if exact else 2.0)


def bound_affine(X, shift, scale, B, bias, factor=1.0):
    m, p = X.shape
    k = B.shape[1]
    aBs, sB = folded(p, k, shift, scale, B)
    return factor * gamma(p + 3) * (np.abs(X) @ aBs + sB + np.abs(_or(bias, 0.0, k)))


def bound_affine_centred(X, shift, scale, B):
    """gamma(p + 3) |X - shift| |Bs|: what the unfolded evaluation would be held to (reported, never asserted)."""
    p = X.shape[1]
    aBs, _ = folded(p, B.shape[1], shift, scale, B)
    return gamma(p + 3) * (np.abs(X - _or(shift, 0.0, p)) @ aBs)


def _model_parts(model, p, q):
    return (_or(model["xmeans"], 0.0, p), _or(model["xscales"], 1.0, p), _or(model["ymeans"], 0.0, q), _or(model["yscales"], 1.0, q))


def ref_scores(X, model, nlv):
    p = X.shape[1]
    xm, xs, _, _ = _model_parts(model, p, model["C"].shape[0])
    return ((ld(X) - ld(xm)) / ld(xs)) @ ld(model["R"][:, :nlv])


def ref_predict(X, model, lo, hi):
    """pred_a = ymeans + T_a (C_a .* yscales)' for a = lo..hi, T = cscale(X, xmeans, xscales) R: the blocks side by side (longdouble)."""
    p, q = X.shape[1], model["C"].shape[0]
    _, _, ym, ys = _model_parts(model, p, q)
    T = ref_scores(X, model, max(hi, 1))
    Cs = (ld(model["C"]) * ld(ys)[:, None]).T                               # (nlv, q)
    return np.concatenate([ld(ym) + T[:, :a] @ Cs[:a] for a in range(lo, hi + 1)], axis=1)


def bound_predict(X, model, lo, hi, path=None):
    """The bound of the path jch_predict takes for this m and range (module docstring); `path` overrides the choice (static test)."""
    m, p = X.shape
    q = model["C"].shape[0]
    xm, xs, ym, ys = _model_parts(model, p, q)
    Rs, Cs = model["R"] / xs[:, None], (model["C"] * ys[:, None]).T       # (p, nlv), (nlv, q)
    out = []
    if (path or predict_path(m, lo, hi)) == "gemm":
        for a in range(lo, hi + 1):
            aB = np.abs(Rs[:, :a] @ Cs[:a])                                 # |B_a| (p, q)
            out.append(gamma(p + 3) * (np.abs(X) @ aB + np.abs(xm) @ aB + np.abs(ym)))
        return np.concatenate(out, axis=1)
    T = np.asarray(ref_scores(X, model, hi), dtype=np.float64)
    bt = gamma(p + 3) * (np.abs(X) @ np.abs(Rs[:, :hi]) + np.abs(xm) @ np.abs(Rs[:, :hi]))
    for a in range(lo, hi + 1):
        out.append(bt[:, :a] @ np.abs(Cs[:a]) + gamma(a + 2) * (np.abs(ym) + np.abs(T[:, :a]) @ np.abs(Cs[:a])))
    return np.concatenate(out, axis=1)


def _norm_weights(w, n):
    w = np.ones(n, dtype=LD) if w is None else ld(w)
    return w / w.sum()


def ref_col_stats(X, w):
    """Weighted column means and uncorrected standard deviations, d = w / sum w (longdouble)."""
    d = _norm_weights(w, X.shape[0])
    Xl = ld(X)
    mean = d @ Xl
    return mean, np.sqrt(d @ (Xl - mean) ** 2)


def bound_means(X, w):
    n = X.shape[0]
    return 2.0 * gamma(n + 2) * (np.asarray(_norm_weights(w, n), dtype=np.float64) @ np.abs(X))


def bound_variance(X, d, mean, dm):
    """The variance bound of the module docstring for weights d (as used: normalised or given), centre `mean` known within dm."""
    n = X.shape[0]
    Xc = np.abs(X - mean)
    return 2.0 * gamma(n + 4) * (d @ Xc ** 2) + 2.0 * dm * (d @ Xc) + dm ** 2 + 2.0 * EPS * (d @ (np.abs(X) * Xc))


def bound_stds(X, w):
    n = X.shape[0]
    d = np.asarray(_norm_weights(w, n), dtype=np.float64)
    mean, std = (np.asarray(v, dtype=np.float64) for v in ref_col_stats(X, w))
    bv = bound_variance(X, d, mean, bound_means(X, w))
    v = std ** 2
    return np.maximum(std - np.sqrt(np.maximum(v - bv, 0.0)), np.sqrt(v + bv) - std) + EPS * np.sqrt(v + bv)


def ref_weighted_ss(X, d, shift, scale):
    """sum_j (1 / scale_j^2) sum_i d_i (x_ij - shift_j)^2 with d as given (longdouble)."""
    p = X.shape[1]
    return float((((ld(d) @ (ld(X) - ld(_or(shift, 0.0, p))) ** 2)) / ld(_or(scale, 1.0, p)) ** 2).sum())


def bound_weighted_ss(X, d, shift, scale):
    p = X.shape[1]
    sh, sc = _or(shift, 0.0, p), _or(scale, 1.0, p)
    v = (d @ (X - sh) ** 2) / sc ** 2
    return float((bound_variance(X, d, sh, 0.0) / sc ** 2).sum() + gamma(p + 2) * v.sum())


def ref_weighted_cov(A, w):
    """S = (A - 1 mu')' diag(d) (A - 1 mu'), d = w / sum w, and mu = d'A (longdouble)."""
    d = _norm_weights(w, A.shape[0])
    Al = ld(A)
    mu = d @ Al
    Ac = Al - mu
    return Ac.T @ (Ac * d[:, None]), mu


def bound_weighted_cov(A, w):
    n = A.shape[0]
    d = np.asarray(_norm_weights(w, n), dtype=np.float64)
    mu = np.asarray(d @ A, dtype=np.float64)
    dm = bound_means(A, w)
    Ac, Aa = np.abs(A - mu), np.abs(A)
    M = Ac.T @ (Ac * d[:, None])
    s1 = d @ Ac                                                             # sum_i d_i |ac_ij|
    cross = Aa.T @ (Ac * d[:, None])
    b = 2.0 * gamma(n + 4) * M + np.outer(s1, dm) + np.outer(dm, s1) + np.outer(dm, dm) + EPS * (cross + cross.T)
    return np.maximum(b, b.T)                                               # (symmetric but for the rounding of the products above)


def _six(w, y, e, t=LD):
    """The six sums of one prediction column over already selected rows, and the sums of the summands' absolute values."""
    terms = [w * e, w * e * e, w * y * e, w * y, w * y * y, w]
    return np.array([x.sum(dtype=t) for x in terms], dtype=t), np.array([float(np.abs(x).sum()) for x in terms])


def ref_score_sums(Pred, Y, mask, t=LD, order=slice(None)):
    """sums[c] = (sum e, sum e^2, sum y e, sum y, sum y^2, count) over the rows with mask != 0, e = y - pred, c = level q + k.  Returns the
    sums (ncol x 6) and, per entry, the sum of the summands' absolute values.  `t` and `order` serve the float64 routes of the static test."""
    m, ncol = Pred.shape
    q = Y.shape[1]
    sel = np.arange(m) if mask is None else np.flatnonzero(mask)
    sel = sel[order]
    w = np.ones(len(sel), dtype=t) if mask is None else np.asarray(mask[sel], dtype=t)
    S, A = np.zeros((ncol, 6), dtype=t), np.zeros((ncol, 6))
    for c in range(ncol):
        y = np.asarray(Y[sel, c % q], dtype=t)
        S[c], A[c] = _six(w, y, y - np.asarray(Pred[sel, c], dtype=t), t)
    return S, A


def bound_score_sums(A, m_sel):
    b = 2.0 * gamma(m_sel + 3) * A
    b[:, 5] = 0.0
    return b


def lv_predictions(T, Cm, ymeans, yscales, q, sel, lo, hi, t=LD):
    """The predictions of levels lo..hi on the rows `sel` (levels beyond kfit repeat level kfit) and the rounding bound bp of each."""
    kfit = 0 if T is None else T.shape[1]
    ym, ys = _or(ymeans, 0.0, q), _or(yscales, 1.0, q)
    Cs = np.zeros((0, q), dtype=t) if kfit == 0 else (np.asarray(Cm, dtype=t) * ys.astype(t)[:, None]).T
    Ts = np.zeros((len(sel), 0), dtype=t) if kfit == 0 else np.asarray(T[sel], dtype=t)
    P, BP = [], []
    for a in range(lo, hi + 1):
        a = min(a, kfit)
        P.append(ym.astype(t) + Ts[:, :a] @ Cs[:a])
        BP.append(gamma(a + 2) * (np.abs(ym) + np.abs(Ts[:, :a]).astype(np.float64) @ np.abs(Cs[:a]).astype(np.float64)))
    return np.concatenate(P, axis=1), np.concatenate(BP, axis=1)


def ref_score_sums_lv(T, Cm, ymeans, yscales, Y, mask, lo, hi, t=LD, order=slice(None)):
    """jch_score_sums on pred_a = ymeans + sum_{l <= min(a, kfit)} t_l (c_l .* yscales)', a = lo..hi.  Returns the sums and their bound."""
    m, q = Y.shape
    sel = (np.arange(m) if mask is None else np.flatnonzero(mask))[order]
    w = np.ones(len(sel), dtype=t) if mask is None else np.asarray(mask[sel], dtype=t)
    P, BP = lv_predictions(T, Cm, ymeans, yscales, q, sel, lo, hi, t)
    ncol = P.shape[1]
    S, B = np.zeros((ncol, 6), dtype=t), np.zeros((ncol, 6))
    wf = np.asarray(w, dtype=np.float64)
    kfit, done = (0 if T is None else T.shape[1]), {}
    for c in range(ncol):
        key = (min(lo + c // q, kfit), c % q)                               # (the levels beyond kfit repeat level kfit: computed once)
        if key in done:
            S[c], B[c] = S[done[key]], B[done[key]]
            continue
        done[key] = c
        y = np.asarray(Y[sel, c % q], dtype=t)
        e = y - P[:, c]
        S[c], A = _six(w, y, e, t)
        B[c] = 2.0 * gamma(len(sel) + 3) * A
        ea, ya, bp = np.abs(e).astype(np.float64), np.abs(y).astype(np.float64), BP[:, c]
        B[c, 0] += (wf * bp).sum(); B[c, 1] += (wf * (2.0 * ea + bp) * bp).sum(); B[c, 2] += (wf * ya * bp).sum()
        B[c, 5] = 0.0
    return S, B


# ==================================================================================================== the static checks
def _half(name, got, ref, bound):
    """A float64 route stays within half of the bound against the longdouble route."""
    err = np.abs(np.asarray(got, dtype=LD) - ref).astype(np.float64)
    bound = np.asarray(bound, dtype=np.float64)
    assert np.isfinite(err).all() and np.all(bound >= 0.0), name
    ok = err <= 0.5 * bound
    ratio = float(np.max(np.where(bound > 0.0, err / np.where(bound > 0.0, bound, 1.0), np.where(err > 0.0, np.inf, 0.0)))) if err.size else 0.0
    print(f"  {name}: max err / bound {ratio:.3f}")
    assert ok.all(), f"{name}: the float64 route uses {ratio:.3f} of the bound"
    return ratio


def _rows_subset(m, cap=192):
    """Every row, or for a long input the first, middle and last 64: the affine map is row by row."""
    if m <= cap:
        return np.arange(m)
    return np.concatenate([np.arange(64), np.arange(m // 2 - 32, m // 2 + 32), np.arange(m - 64, m)])


def test_longdouble_is_extended_precision():
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is not wider than float64 here: the references would be no reference"


def test_the_shape_lists_cover_what_the_issue_names():
    kern = {affine_kernel(m, p, k) for m, p, k, _ in AFFINE_TRIPLES}
    unp = {affine_kernel(m, p, k, ldo_even=False) for m, p, k, _ in AFFINE_TRIPLES}
    for need in ("general", "gemm32", "gemm32s", "gemm32p<1,4,paired>", "gemm32p<2,8,paired>", "wideout<4,paired>", "wideout<8,paired>", "wideout<16,paired>"):
        assert sum(affine_kernel(m, p, k) == need for m, p, k, _ in AFFINE_TRIPLES) >= 2, need
    assert {"gemm32p<1,4,unpaired>", "gemm32p<2,8,unpaired>", "wideout<4,unpaired>", "wideout<8,unpaired>", "wideout<16,unpaired>"} <= unp
    for m, p, k, name in AFFINE_TRIPLES:                     # the id says what runs
        assert affine_kernel(m, p, k).split(",")[0].split("<")[0] == name.split("<")[0].split("-")[0], (m, p, k, name)
    assert {m for m, _, _, _ in AFFINE_TRIPLES} == {1, 31, 32, 33, 127, 129, 4096, 4097, 4098, 8192, 8194, 65536, 65538, 65537}
    assert {p for _, p, _, _ in AFFINE_TRIPLES} == {1, 3, 4, 5, 16, 17, 32, 33, 63, 64, 65, 130, 576, 580}
    assert {k for _, _, k, _ in AFFINE_TRIPLES} == {1, 15, 16, 17, 32, 33, 128, 129, 260}
    assert sum(m * p > AFFINE_BIG for m, p, _, _ in AFFINE_TRIPLES) == 2
    assert {c[0] for c in PREDICT_CASES} == {4095, 4096, 4097, 4098} and {c[1] for c in PREDICT_CASES} == {1, 4, 5, 8, 9, 17}
    assert {c[2] for c in PREDICT_CASES} == {0, 1, 2}
    assert {c[0] for c in STATS_CASES} == {1, 2, 255, 256, 257, 511, 513, 2047, 2048, 2049, 70001} and {c[1] for c in STATS_CASES} == {1, 2, 130, 2100}
    assert {c[0] for c in COV_CASES} == {1, 2, 63, 64, 65, 257, 4097} and {c[1] for c in COV_CASES} == {1, 2, 15, 16, 17, 63, 64, 65, 130}
    assert {c[0] for c in SCORE_CASES} == {1, 255, 256, 257, 70001} and {c[1] for c in SCORE_CASES} == {1, 3, 11, 17}
    assert {c[2] for c in SCORE_CASES} == {1, 2, 32, 33, 64, 65} and {c[3] for c in SCORE_CASES} == {None, "random", "ones", "zeros", "last"}
    assert {c[0] for c in SCORE_LV_CASES} == {1, 255, 256, 257, 70001} and {c[1] for c in SCORE_LV_CASES} == {1, 3, 11, 17}


def _affine_id(t):
    return "m%d-p%d-k%d-%s" % t


@pytest.mark.parametrize("triple", AFFINE_TRIPLES + [c + ("folding-cost",) for c in FOLD_CASES], ids=_affine_id)
def test_affine_reference_uses_half_the_bound_at_most(triple):
    m, p, k, name = triple
    fold = name == "folding-cost"
    for level, present in ([(v, True) for v in FOLD_LEVELS] if fold else AFFINE_CONFIGS[: 1 if m * p > AFFINE_BIG else 2]):
        X, shift, scale, B, bias = fold_data(m, p, k, level) if fold else affine_data(m, p, k, level, present)
        rows = _rows_subset(m)
        Xs = X[rows]
        ref, _ = ref_affine(Xs, shift, scale, B, bias, exact=True)
        bound = bound_affine(Xs, shift, scale, B, bias)
        sh, sc, bi = _or(shift, 0.0, p), _or(scale, 1.0, p), _or(bias, 0.0, k)
        fwd = ((Xs - sh) / sc) @ B + bi
        rev = ((Xs - sh) / sc)[:, ::-1] @ B[::-1] + bi
        Bs = B / sc[:, None]                                              # and the folded form itself, term by term in both orders
        fold_f, fold_r = np.tile(bi - sh @ Bs, (len(rows), 1)), np.tile(bi - sh[::-1] @ Bs[::-1], (len(rows), 1))
        for j in range(p):
            fold_f += np.outer(Xs[:, j], Bs[j]); fold_r += np.outer(Xs[:, p - 1 - j], Bs[p - 1 - j])
        for name, got in (("centred forward", fwd), ("centred reversed", rev), ("folded forward", fold_f), ("folded reversed", fold_r)):
            _half(f"level {level:g}: {name}", got, ref, bound)


@pytest.mark.parametrize("case", PREDICT_CASES, ids=lambda c: "m%d-q%d" % c[:2])
def test_predict_reference_uses_half_the_bound_at_most(case):
    m, q, _, _, null, _ = case
    X, model = predict_data(m, q, null)
    X = X[_rows_subset(m)]
    p = X.shape[1]
    xm, xs, ym, ys = _model_parts(model, p, q)
    Cs = (model["C"] * ys[:, None]).T
    for lo, hi in PREDICT_RANGES:
        ref = ref_predict(X, model, lo, hi)
        T = ((X - xm) / xs) @ model["R"]
        Tr = ((X - xm) / xs)[:, ::-1] @ model["R"][::-1]
        fwd = np.concatenate([ym + T[:, :a] @ Cs[:a] for a in range(lo, hi + 1)], axis=1)
        rev = np.concatenate([ym + Tr[:, :a][:, ::-1] @ Cs[:a][::-1] for a in range(lo, hi + 1)], axis=1)   # (from the last score column down)
        for path in ("gemm", "prefix"):                                     # both paths' bounds (the subset has fewer rows than either needs)
            bound = bound_predict(X, model, lo, hi, path)
            _half(f"range {lo}..{hi}, {path} bound, forward", fwd, ref, bound)
            _half(f"range {lo}..{hi}, {path} bound, reversed", rev, ref, bound)


@pytest.mark.parametrize("case", STATS_CASES, ids=lambda c: "n%d-p%d-level%g-%s" % c[:4])
def test_col_stats_and_weighted_ss_references_use_half_the_bound_at_most(case):
    n, p, level, wkind = case[:4]
    X, w = stats_data(n, p, level, wkind)
    mean, std = ref_col_stats(X, w)
    bm, bs = bound_means(X, w), bound_stds(X, w)
    w64 = np.ones(n) if w is None else w
    for name, o in (("forward", slice(None)), ("reversed", slice(None, None, -1))):
        d64 = w64[o] / w64[o].sum()
        m64 = d64 @ X[o]
        s64 = np.sqrt(d64 @ (X[o] - m64) ** 2)
        _half(f"means, {name}", m64, mean, bm)
        _half(f"stds, {name}", s64, std, bs)
    if p >= 2:
        assert float(std[0]) < 1e-3 * bs[0]                               # the constant column: the reference is exact, the bound is not zero
    d = w64 / w64.sum()
    rng = np.random.default_rng(n + p)
    for shift, scale in ((np.asarray(mean, dtype=np.float64), rng.uniform(0.5, 2.0, p)), (None, None)):
        ref, b = ref_weighted_ss(X, d, shift, scale), bound_weighted_ss(X, d, shift, scale)
        sh, sc = _or(shift, 0.0, p), _or(scale, 1.0, p)
        for name, o in (("forward", slice(None)), ("reversed", slice(None, None, -1))):
            got = ((d[o] @ (X[o] - sh) ** 2) / sc ** 2)[o if p > 1 else slice(None)].sum()
            _half(f"ss, {name}", np.array([got]), np.array([ref], dtype=LD), np.array([b]))


@pytest.mark.parametrize("case", COV_CASES, ids=lambda c: "n%d-d%d-level%g-%s" % c[:4])
def test_weighted_cov_reference_uses_half_the_bound_at_most(case):
    n, d, level, wkind = case[:4]
    A, w = cov_data(n, d, level, wkind)
    S, mu = ref_weighted_cov(A, w)
    b, bm = bound_weighted_cov(A, w), bound_means(A, w)
    assert np.array_equal(b, b.T)
    w64 = np.ones(n) if w is None else w
    for name, o in (("forward", slice(None)), ("reversed", slice(None, None, -1))):
        dd = w64[o] / w64[o].sum()
        m64 = dd @ A[o]
        Ac = A[o] - m64
        _half(f"mu, {name}", m64, mu, bm)
        _half(f"S, {name}", Ac.T @ (Ac * dd[:, None]), S, b)
    if n == 1:
        assert not np.any(np.asarray(S, dtype=np.float64)) and np.all(b > 0.0)


@pytest.mark.parametrize("case", SCORE_CASES, ids=lambda c: "m%d-q%d-levels%d-%s" % c[:4])
def test_score_sums_reference_uses_half_the_bound_at_most(case):
    m, q, levels, mkind, _ = case
    Pred, Y, mask = score_data(m, q, levels, mkind)
    S, A = ref_score_sums(Pred, Y, mask)
    m_sel = m if mask is None else int(np.count_nonzero(mask))
    assert np.all(np.asarray(S[:, 5], dtype=np.float64) == m_sel) and np.isfinite(np.asarray(S, dtype=np.float64)).all()
    if m_sel == 0:
        assert not np.any(np.asarray(S, dtype=np.float64))
    b = bound_score_sums(A, m_sel)
    for name, o in (("forward", slice(None)), ("reversed", slice(None, None, -1))):
        got, _ = ref_score_sums(Pred, Y, mask, t=np.float64, order=o)
        _half(name, got, S, b)


@pytest.mark.parametrize("case", SCORE_LV_CASES, ids=lambda c: "m%d-q%d-kfit%d-%s" % c[:4])
def test_score_sums_lv_reference_uses_half_the_bound_at_most(case):
    m, q, kfit, mkind, _, null = case
    T, Cm, ym, ys, Y, mask = score_lv_data(m, q, kfit, mkind, null)
    for lo, hi in score_lv_ranges(kfit):
        S, b = ref_score_sums_lv(T, Cm, ym, ys, Y, mask, lo, hi)
        assert np.isfinite(np.asarray(S, dtype=np.float64)).all()
        if lo >= kfit:                                                      # levels beyond the fit repeat level kfit
            assert all(np.array_equal(S[:q], S[i * q:(i + 1) * q]) for i in range(hi - lo + 1))
        for name, o in (("forward", slice(None)), ("reversed", slice(None, None, -1))):
            got, _ = ref_score_sums_lv(T, Cm, ym, ys, Y, mask, lo, hi, t=np.float64, order=o)
            _half(f"{lo}..{hi} {name}", got, S, b)
        if lo == 0 and hi == kfit and mask is not None and np.count_nonzero(mask):   # the two references agree with each other
            sel = np.flatnonzero(mask)
            P = np.full((m, (hi - lo + 1) * q), np.nan, dtype=LD)
            P[sel], _ = lv_predictions(T, Cm, ym, ys, q, sel, lo, hi)
            S2, _ = ref_score_sums(P, Y, mask)
            assert np.allclose(np.asarray(S2, dtype=np.float64), np.asarray(S, dtype=np.float64), rtol=1e-12, atol=1e-12)
