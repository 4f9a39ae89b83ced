// The Gaussian discriminants of a neighbourhood, for the whole range of nested score spaces at once (src/lwplslda.jl, src/lwplsqda.jl through
// src/locwlv.jl, src/plslda.jl:84-86, src/plsqda.jl; the fits restate src/lda.jl:56-77, src/qda.jl:55-79, src/matW.jl:47-77 and
// src/dmnorm.jl:112-143) — jch_knn_gda, include/jchemo_hip.h; DESIGN.md §25.
//
// The reference refits lda / qda on T[:, 1:a] for every a.  The Cholesky factor of a leading block is the leading block of the Cholesky factor, so
// the squared Mahalanobis distance in the first a score columns is a prefix sum of the squares of ONE forward substitution and the determinant a
// prefix product of the diagonal: one factorisation and one substitution per class give all the nested models of a query.
//
//   k_knn_gda<LDS>   one 256-thread workgroup per query.  The slab — the k x a scores, the a x a covariance / factor (row-major, leading dimension
//                    a | 1: the lanes that walk down a column of the factor then fall on different banks of the 8-byte reads), the class means, the
//                    substitution vectors of the four waves, the class codes and counts — lives in dynamic LDS (LDS = true) or, beyond
//                    GDA_LDS_MAX bytes, in a per-workgroup piece of the workspace (LDS = false): the same code, the slab pointer apart (and a
//                    __threadfence_block in front of the barriers).  Steps, with the workgroup barriers between them:
//                      1. codes, scores and the query's scores into the slab; class counts; the local levels.  A unanimous list: info 1, one-hot.
//                      2. class means (unweighted), and the mean of all k rows when a class of one row needs it (src/matW.jl:55-65).
//                      3. per factor (LDA: one, QDA: one per local level): the covariance — differences t - mu before any product, one thread
//                         per entry of the lower triangle, rows in order —, the left-looking Cholesky with the pivot rule of the header, then per
//                         class one wave: forward substitution column by column; lane 0 carries the prefix sums d2_a and the prefix products of
//                         the diagonal and writes prior x density of every requested model.
//                      4. per model one thread: the sum over the local levels in code order, the posterior, the first maximum.
//                    Every sum has a fixed order and there are no atomics: two runs give identical bits.
// jch_lwplsda_predict_prepared (at the end of this file) is jch_lwplsr_predict_prepared on a handle whose Ytrain is the dummy table: search and
// weights (jch_knn_dispatch), the neighbours' class codes (k_da_gather_cls), the local fits with their score outputs (k_locw_plskern of lwplsr.hip,
// or one fit per query outside its envelope: jch_lw_generic_fits_da), then k_rda_finish (plsrda) or k_knn_gda + jch_knn_vote + k_da_vote_fill.
// gfx950, hipcc -O3; plain HIP C++.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "jch_internal.h"
#include "lwplsr_dev.h"

#define GDA_LDS_MAX (150 * 1024)   // largest slab that lives in LDS; beyond: the workspace

// doubles of one workgroup's slab: scores k x a, factor a x (a | 1), the covariance's diagonal and the factor's (a each), the means (nlev + 1) x a,
// the substitution vectors 4 x a, the query's scores a, then the ints: counts nlev, codes k
size_t jch_knn_gda_slab_doubles(int64_t k, int64_t a, int64_t nlev)
{
    const size_t ld = (size_t)a | 1;
    return (size_t)k * a + (size_t)a * ld + 2 * (size_t)a + ((size_t)nlev + 1) * a + 4 * (size_t)a + (size_t)a + ((size_t)nlev + (size_t)k + 1) / 2 + 2;
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_knn_gda(gda_args g)
{
    extern __shared__ __attribute__((aligned(16))) double gda_dyn[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k = g.k, a = g.a, nlev = g.nlev, ld = a | 1, le = g.nlv_hi - g.nlv_lo + 1;
    double *Tl = LDS ? gda_dyn : g.scratch + (size_t)blockIdx.x * g.per_block;   // [k][a]
    double *Lm = Tl + (size_t)k * a;               // [a][ld]
    double *sd = Lm + (size_t)a * ld;              // [a] diagonal of the covariance
    double *dg = sd + a;                           // [a] diagonal of the factor
    double *mu = dg + a;                           // [nlev + 1][a]: class means, then the mean of all rows
    double *zb = mu + ((size_t)nlev + 1) * a;      // [4][a]
    double *tqv = zb + 4 * (size_t)a;              // [a]
    int *cnt = reinterpret_cast<int *>(tqv + a);   // [nlev]
    int *cl = cnt + nlev;                          // [k]
    const double nan = __builtin_nan("");
    for (int qi = blockIdx.x; qi < g.m; qi += gridDim.x) {
        double *post = g.post + (size_t)qi * le * nlev;
        int *code = g.code + (size_t)qi * le, *info = g.info + (size_t)qi * le;
        slab_bsync<LDS>();                                      // (the previous query is done with the slab)
        // ---- 1. the slab
        for (int e = tid; e < k; e += 256) { const int c = g.cls[(size_t)qi * k + e]; cl[e] = (c >= 0 && c < nlev) ? c : -1; }
        {
            const double *Tq = g.T + (size_t)qi * g.tstride;
            int row = 0, col = tid;
            while (col >= a) { col -= a; ++row; }
            for (; row < k;) {
                Tl[(size_t)row * a + col] = Tq[(size_t)row * g.ldt + col];
                col += 256;
                while (col >= a) { col -= a; ++row; }
            }
        }
        for (int j = tid; j < a; j += 256) tqv[j] = g.tq[(size_t)qi * g.ldq + j];
        slab_bsync<LDS>();
        knn_class_counts(cl, k, nlev, cnt);
        slab_bsync<LDS>();
        int nloc = 0, n1 = 0, first = -1, nvalid = 0;          // (every thread the same walk: block-uniform)
        for (int c = 0; c < nlev; ++c) {
            const int n = cnt[c];
            nvalid += n;
            if (n > 0) { ++nloc; if (first < 0) first = c; }
            if (n == 1) ++n1;
        }
        if (nvalid != k || nloc == 1) {
            // a code outside [0, nlev): no model (info 3, NaN); one local level: the reference's shortcut (src/locwlv.jl:25-28), info 1 and a one-hot posterior
            const bool una = nvalid == k;
            for (int e = tid; e < le * nlev; e += 256) post[e] = una ? ((e % nlev) == first ? 1.0 : 0.0) : nan;
            for (int t = tid; t < le; t += 256) { code[t] = una ? first : -1; info[t] = una ? 1 : 3; }
            continue;
        }
        // ---- 2. the means
        for (int it = tid; it < (nlev + 1) * a; it += 256) {
            const int c = it / a, j = it - c * a;
            const bool all = c == nlev;
            double s = 0.0;
            int cn = all ? (n1 > 0 ? k : 0) : cnt[c];
            if (cn > 0)
                for (int e = 0; e < k; ++e)
                    if (all || cl[e] == c) s += Tl[(size_t)e * a + j];
            mu[it] = cn > 0 ? s / (double)cn : 0.0;
        }
        slab_bsync<LDS>();
        // ---- 3. the factors
        const double *mug = mu + (size_t)nlev * a;
        int jfmin = a;                                         // the first pivot (0-based) that was not positive, over the factors
        int jnan = a;                                          // the first pivot that was a NaN (a NaN among the neighbours' scores)
        const int nfac = g.kind == 1 ? 1 : nlev;
        for (int f = 0; f < nfac; ++f) {
            const int fc = g.kind == 1 ? -1 : f;               // QDA: the class of this factor
            if (fc >= 0 && cnt[fc] == 0) continue;             // (block-uniform)
            const int nf = fc >= 0 ? cnt[fc] : 0;
            for (int it = tid; it < a * a; it += 256) {
                const int i = it / a, j = it - i * a;
                if (j > i) continue;
                double s1 = 0.0, s2 = 0.0;
                if (fc < 0) {
                    for (int e = 0; e < k; ++e) {
                        const int c = cl[e];
                        if (cnt[c] >= 2) s1 += (Tl[(size_t)e * a + i] - mu[(size_t)c * a + i]) * (Tl[(size_t)e * a + j] - mu[(size_t)c * a + j]);
                    }
                } else if (nf >= 2) {
                    for (int e = 0; e < k; ++e)
                        if (cl[e] == fc) s1 += (Tl[(size_t)e * a + i] - mu[(size_t)fc * a + i]) * (Tl[(size_t)e * a + j] - mu[(size_t)fc * a + j]);
                }
                if (fc < 0 ? n1 > 0 : nf == 1)
                    for (int e = 0; e < k; ++e) s2 += (Tl[(size_t)e * a + i] - mug[i]) * (Tl[(size_t)e * a + j] - mug[j]);
                double s;
                if (fc < 0) {
                    // W = sum_c (n_c / k) W_c with W_c the uncorrected covariance (a class of one row: that of all rows), S = W k / (k - nlev_loc)
                    const double w = (s1 + (double)n1 * (s2 / (double)k)) / (double)k;
                    s = w * (double)k / (double)(k - nloc);
                } else {
                    s = nf >= 2 ? (s1 / (double)nf) * (double)nf / (double)(nf - 1) : s2 / (double)k;
                }
                Lm[(size_t)i * ld + j] = s;
                if (i == j) sd[i] = s;
            }
            slab_bsync<LDS>();
            int jfail = a;
            for (int j = 0; j < a; ++j) {
                for (int i = j + tid; i < a; i += 256) {
                    double s = Lm[(size_t)i * ld + j];
                    for (int l = 0; l < j; ++l) s -= Lm[(size_t)i * ld + l] * Lm[(size_t)j * ld + l];
                    if (i == j) {
                        // pivot j (1-based j + 1) is not positive when it is <= (k + 4 j) 2^-52 S_jj: the error the covariance sum and the
                        // factorisation leave on the diagonal (a NaN is not positive either)
                        const bool ok = s > ((double)k + 4.0 * (double)(j + 1)) * 0x1p-52 * sd[j];
                        dg[j] = ok ? sqrt(s) : (s != s ? s : 0.0);   // (a NaN pivot stays a NaN: non-finite scores, not a rank deficiency)
                    } else Lm[(size_t)i * ld + j] = s;
                }
                slab_bsync<LDS>();
                const double r = dg[j];
                if (!(r > 0.0)) { jfail = j; if (r != r) jnan = min(jnan, j); break; }   // (block-uniform: every thread reads the same dg[j])
                for (int i = j + 1 + tid; i < a; i += 256) Lm[(size_t)i * ld + j] /= r;
                slab_bsync<LDS>();
            }
            jfmin = min(jfmin, jfail);
            // per class under this factor one wave: z = L^-1 (tq - mu_c), then prefix sums of z^2 and prefix products of the diagonal
            for (int c = (fc < 0 ? wv : fc); c < (fc < 0 ? nlev : (wv == 0 ? fc + 1 : 0)); c += 4) {
                if (cnt[c] == 0) continue;                     // (wave-uniform)
                double *z = zb + (size_t)wv * a;
                for (int j = lane; j < a; j += 64) z[j] = tqv[j] - mu[(size_t)c * a + j];
                slab_wsync<LDS>();
                const double wprior = g.prior == 0 ? 1.0 / (double)nloc : (double)cnt[c] / (double)k;
                double d2 = 0.0, pd = 1.0;
                for (int j = 0; j < jfail; ++j) {
                    const double zj = z[j] / dg[j];
                    for (int i = j + 1 + lane; i < jfail; i += 64) z[i] -= Lm[(size_t)i * ld + j] * zj;
                    slab_wsync<LDS>();
                    d2 += zj * zj;
                    pd *= dg[j];
                    const int am = j + 1;                      // the model on the first am score columns; requests beyond a clamp to a
                    const int k0 = max(am, g.nlv_lo), k1 = am == a ? g.nlv_hi : min(am, g.nlv_hi);
                    if (lane == 0 && k0 <= k1) {
                        double det = pd * pd;
                        if (det == 0.0) det = 1e-20;               // src/dmnorm.jl:122
                        const double dens = pow(2.0 * 3.14159265358979323846, -0.5 * (double)am) * (1.0 / sqrt(det)) * exp(-0.5 * d2);
                        for (int kk = k0; kk <= k1; ++kk) post[(size_t)(kk - g.nlv_lo) * nlev + c] = wprior * dens;
                    }
                }
            }
            __threadfence_block();
            __syncthreads();                                   // (the factor is done with; prior x density of its classes is in post)
        }
        // ---- 4. posteriors and labels, one thread per model
        for (int t = tid; t < le; t += 256) {
            const int am = min(g.nlv_lo + t, a);
            double *pt = post + (size_t)t * nlev;
            if (am > jfmin) {                                  // the covariance is not positive definite in these score columns
                for (int c = 0; c < nlev; ++c) pt[c] = nan;
                const bool nonfinite = jnan == jfmin;          // the pivot that stopped the models was a NaN: info 3 and the first local level
                code[t] = nonfinite ? first : -1; info[t] = nonfinite ? 3 : 2;
                continue;
            }
            double s = 0.0;
            int bad = 0;
            for (int c = 0; c < nlev; ++c)
                if (cnt[c] > 0) { const double v = pt[c]; s += v; bad |= (v - v == 0.0) ? 0 : 1; }
            int best = -1;                                     // (two local levels at least: one is taken)
            double bv = 0.0;
            for (int c = 0; c < nlev; ++c) {
                if (cnt[c] == 0) { pt[c] = 0.0; continue; }
                const double v = pt[c] / s;
                pt[c] = v;
                if (best < 0 || knn_vote_better(v, bv)) { best = c; bv = v; }   // the label rule (lwplsr_dev.h)
            }
            code[t] = best; info[t] = bad ? 3 : 0;
        }
    }
}

// *slab: the doubles of this shape's slab; where it lives and the workgroups of the launch: jch_slab_plan (JCH_GDA_WS=1: the workspace path at any shape — tests)
jch_slab_where jch_knn_gda_plan(jch_ctx *ctx, int64_t m, int64_t k, int64_t a, int64_t nlev, size_t *slab)
{
    *slab = (jch_knn_gda_slab_doubles(k, a, nlev) + 31) & ~(size_t)31;
    return jch_slab_plan(ctx, m, *slab, GDA_LDS_MAX, jch_knob("JCH_GDA_WS", 0) == 1);
}

// g: all pointers on the device; g.scratch: null (LDS) or nb slabs of g.per_block doubles, as jch_knn_gda_plan said
int32_t jch_launch_knn_gda(jch_ctx *ctx, const gda_args &g, int64_t nb)
{
    return jch_launch_slab<k_knn_gda<true>, k_knn_gda<false>>(ctx, {g.scratch != nullptr, nb}, g.per_block, GDA_LDS_MAX, g);
}


extern "C" int32_t jch_knn_gda(jch_ctx *ctx, int32_t loc, const double *T, int64_t m, int32_t k, int32_t a_hi, const double *tq, const int32_t *cls_nb,
                               int32_t nlev, int32_t kind, int32_t prior, int32_t nlv_lo, int32_t nlv_hi, double *post, int32_t *code, int32_t *info)
{
    if (!ctx) return JCH_EINVAL;
    if (!T || !tq || !cls_nb || !post || !code || !info || m < 1 || k < 1 || a_hi < 1 || nlev < 1 || m >= ((int64_t)1 << 31) - 1 || k >= (1 << 24) ||
        a_hi > (1 << 12) || nlev > (1 << 20) || (size_t)m * (size_t)k * (size_t)a_hi >= ((size_t)1 << 40))
        return jch_fail(ctx, JCH_EINVAL, "jch_knn_gda: bad arguments");
    if (kind != 1 && kind != 2) return jch_fail(ctx, JCH_EINVAL, "jch_knn_gda: kind must be 1 (lda) or 2 (qda), not %d", kind);
    if (prior != 0 && prior != 1) return jch_fail(ctx, JCH_EINVAL, "jch_knn_gda: prior must be 0 (unif) or 1 (prop), not %d", prior);
    if (nlv_lo < 1 || nlv_hi < nlv_lo || nlv_hi > a_hi)
        return jch_fail(ctx, JCH_EINVAL, "jch_knn_gda: the models nlv_lo .. nlv_hi = %d .. %d must lie in 1 .. a_hi = %d", nlv_lo, nlv_hi, a_hi);
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "jch_knn_gda: bad loc");
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST;
    const size_t le = (size_t)(nlv_hi - nlv_lo + 1), nt = (size_t)m * k * a_hi, nq = (size_t)m * a_hi, nc = (size_t)m * k, np = (size_t)m * le * nlev, ni = (size_t)m * le;
    size_t slab = 0;
    const jch_slab_where at = jch_knn_gda_plan(ctx, m, k, nlv_hi, nlev, &slab);
    jch_carve cv;
    const size_t o_t = host ? cv.take(nt) : 0, o_q = host ? cv.take(nq) : 0, o_c = host ? cv.take(jch_ints_as_doubles(nc)) : 0, o_p = host ? cv.take(np) : 0;
    const size_t o_k = host ? cv.take(jch_ints_as_doubles(ni)) : 0, o_f = host ? cv.take(jch_ints_as_doubles(ni)) : 0, o_sc = at.glob ? cv.take((size_t)at.nb * slab) : 0;
    JCH_TRY(jch_reserve(ctx, ctx->kn_ws, sizeof(double) * cv.off + 256));
    double *ws = (double *)ctx->kn_ws.ptr;
    return jch_synced(ctx, host, [&]() -> int32_t {
        gda_args g;
        g.T = T; g.tq = tq; g.cls = cls_nb; g.post = post; g.code = code; g.info = info;
        if (host) {
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_t, T, sizeof(double) * nt, hipMemcpyHostToDevice, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_q, tq, sizeof(double) * nq, hipMemcpyHostToDevice, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_c, cls_nb, sizeof(int) * nc, hipMemcpyHostToDevice, ctx->stream));
            g.T = ws + o_t; g.tq = ws + o_q; g.cls = (const int *)(ws + o_c); g.post = ws + o_p; g.code = (int *)(ws + o_k); g.info = (int *)(ws + o_f);
        }
        // the factor spans the first nlv_hi score columns: the columns behind them are never read
        g.tstride = (int64_t)k * a_hi; g.ldt = a_hi; g.ldq = a_hi; g.m = (int)m; g.k = k; g.a = nlv_hi; g.nlev = nlev; g.kind = kind; g.prior = prior;
        g.nlv_lo = nlv_lo; g.nlv_hi = nlv_hi; g.scratch = at.glob ? ws + o_sc : nullptr; g.per_block = slab;
        JCH_TRY(jch_launch_knn_gda(ctx, g, at.nb));
        if (host) {
            JCH_HIP(ctx, hipMemcpyAsync(post, g.post, sizeof(double) * np, hipMemcpyDeviceToHost, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(code, g.code, sizeof(int) * ni, hipMemcpyDeviceToHost, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(info, g.info, sizeof(int) * ni, hipMemcpyDeviceToHost, ctx->stream));
        }
        return JCH_OK;
    });
}

// ---------------------------------------------------------------- local PLS discrimination (src/lwplsrda.jl, src/lwplslda.jl, src/lwplsqda.jl)
// cls_nb[i][e] = cls[ind[i][e]]
__global__ __launch_bounds__(256) void k_da_gather_cls(const int *__restrict__ cls, const int *__restrict__ ind, size_t mk, int *__restrict__ out)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < mk; e += (size_t)gridDim.x * 256) out[e] = cls[ind[e]];
}

// PLSR-DA (src/plsrda.jl:106-114) per query: post = the dummy predictions, the label = the first maximum over the LOCAL levels (absent classes are masked,
// a NaN counts as the largest value: Julia's argmax); a unanimous neighbourhood (info1 = 1): that class, a one-hot posterior.  One workgroup per query.
__global__ __launch_bounds__(256) void k_rda_finish(const double *__restrict__ pred, const int *__restrict__ info1, const int *__restrict__ cls_nb, int m, int k,
                                                    int nlev, int le, double *__restrict__ post, int *__restrict__ code, int *__restrict__ info)
{
    extern __shared__ int rda_cnt[];   // [nlev]
    const int tid = threadIdx.x;
    for (int qi = blockIdx.x; qi < m; qi += gridDim.x) {
        __syncthreads();
        const int *cn = cls_nb + (size_t)qi * k;
        knn_class_counts(cn, k, nlev, rda_cnt);
        __syncthreads();
        const double *pq = pred + (size_t)qi * le * nlev;
        double *po = post + (size_t)qi * le * nlev;
        if (info1[qi] == 1) {
            const int c0 = cn[0];
            for (int e = tid; e < le * nlev; e += 256) po[e] = (e % nlev) == c0 ? 1.0 : 0.0;
            for (int t = tid; t < le; t += 256) { code[(size_t)qi * le + t] = c0; info[(size_t)qi * le + t] = 1; }
            continue;
        }
        for (int t = tid; t < le; t += 256) {
            int best = -1, bad = 0;
            double bv = 0.0;
            for (int c = 0; c < nlev; ++c) {
                const double v = pq[(size_t)t * nlev + c];
                po[(size_t)t * nlev + c] = v;
                if (rda_cnt[c] == 0) continue;
                bad |= (v - v == 0.0) ? 0 : 1;
                if (best < 0 || knn_vote_better(v, bv)) { best = c; bv = v; }
            }
            code[(size_t)qi * le + t] = best;
            info[(size_t)qi * le + t] = bad ? 3 : 0;
        }
    }
}

// info 2 (the covariance is not positive definite in these score columns): the label is the weighted vote of the neighbourhood
__global__ __launch_bounds__(256) void k_da_vote_fill(const int *__restrict__ info, const int *__restrict__ vote, int m, int le, int *__restrict__ code)
{
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)m * le; e += (size_t)gridDim.x * 256)
        if (info[e] == 2) code[e] = vote[e / le];
}


extern "C" int32_t jch_lwplsda_predict_prepared(jch_ctx *ctx, const jch_lwplsr_model *model, const int32_t *cls_train, int32_t nlev, int32_t kind, int32_t prior,
                                                int32_t loc, const double *Zq, int64_t ldzq, const double *Xq, int64_t m, int64_t ldxq, int32_t k, double h,
                                                double tol, int32_t scal, int32_t nlv_lo, int32_t nlv_hi, int32_t *code, double *post, int32_t *info,
                                                double *tloc_out, double *tq_out, int32_t *ind_out, double *dist_out, double *w_out)
{
    if (!ctx) return JCH_EINVAL;
    const char *who = "jch_lwplsda_predict_prepared";
    if (!model || !cls_train || !Xq || !code || !post || !info || ldxq < m || (Zq && ldzq < m)) return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments", who);
    if (kind < 0 || kind > 2) return jch_fail(ctx, JCH_EINVAL, "%s: kind must be 0 (rda), 1 (lda) or 2 (qda), not %d", who, kind);
    if (prior != 0 && prior != 1) return jch_fail(ctx, JCH_EINVAL, "%s: prior must be 0 (unif) or 1 (prop), not %d", who, prior);
    if (nlev < 1 || nlev != model->q) return jch_fail(ctx, JCH_EINVAL, "%s: the model's Ytrain must be the n x nlev dummy table (it has %lld columns, nlev = %d)", who, (long long)model->q, nlev);
    JCH_TRY(jch_lw_front_check(ctx, who, model, Zq));
    if (m < 1 || k < 1 || nlv_lo < 0 || nlv_hi < nlv_lo || m >= ((int64_t)1 << 31) - 1) return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments", who);
    if (k > model->n) k = (int32_t)model->n;                      // src/getknn.jl:33
    if (kind != 0 && nlv_lo < 1) return jch_fail(ctx, JCH_EINVAL, "%s: a Gaussian discriminant needs at least one score column (nlv_lo = %d)", who, nlv_lo);
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc", who);
    const int64_t n = model->n, p = model->p, dd = model->dd;
    const int le = nlv_hi - nlv_lo + 1;
    if (loc == JCH_LOC_HOST)
        for (int64_t i = 0; i < n; ++i)
            if (cls_train[i] < 0 || cls_train[i] >= nlev) return jch_fail(ctx, JCH_EINVAL, "%s: cls_train[%lld] = %d is no code in 0 .. %d", who, (long long)i, cls_train[i], nlev - 1);
    locw_args g;
    g.Xrm = model->Xrm; g.ldr = model->ldr; g.p = (int)p; g.Y = model->Y; g.ldy = n; g.q = nlev; g.m = (int)m; g.k = k; g.scal = scal;
    g.nlv_lo = nlv_lo; g.nlv_hi = nlv_hi; g.scratch = nullptr; g.slab = 0; g.flags = nullptr; g.dbg = 0; g.da = 1;
    // outside the envelope of the p-space kernel (the batched kernel that hands out its scores): one fit per query (lwplsr_generic.hip); JCH_LOCW_GENERIC=1 forces it (tests)
    const bool generic = !jch_locw_pspace_fits(g) || jch_knob("JCH_LOCW_GENERIC", 0) == 1;
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST;
    const size_t mk = (size_t)m * k, ntl = mk * (size_t)std::max(nlv_hi, 1), ntq = (size_t)m * std::max(nlv_hi, 1), np = (size_t)m * le * nlev, nm = (size_t)m * le;
    // the local model's LVs: what k_locw_plskern fits, and what jch_plskern_fit reports back on the per-query route (min(k, p, nlv) there too), so
    // the score columns beyond a_fit are the zeros of both routes and the models beyond a_fit clamp to it
    const int a_fit = std::min(std::min((int)k, (int)p), (int)nlv_hi);
    size_t slab = 0;
    const jch_slab_where at = kind != 0 ? jch_knn_gda_plan(ctx, m, k, a_fit, nlev, &slab) : jch_slab_where{false, 0};
    jch_carve cv;
    const size_t o_tl = cv.take(ntl), o_tq = cv.take(ntq), o_cn = cv.take(jch_ints_as_doubles(mk)), o_po = cv.take(np), o_co = cv.take(jch_ints_as_doubles(nm));
    const size_t o_in = cv.take(jch_ints_as_doubles(nm)), o_i1 = cv.take(jch_ints_as_doubles((size_t)m)), o_vo = cv.take(jch_ints_as_doubles((size_t)m));
    const size_t o_cl = host ? cv.take(jch_ints_as_doubles((size_t)n)) : 0, o_sc = at.glob ? cv.take((size_t)at.nb * slab) : 0;
    JCH_TRY(jch_reserve(ctx, ctx->gd_ws, sizeof(double) * cv.off + 256));
    JCH_TRY(jch_reserve(ctx, ctx->gemm_out, sizeof(double) * (mk * 2 + np) + sizeof(int) * mk + 256));
    return jch_synced(ctx, true, [&]() -> int32_t {
        double *ws = (double *)ctx->gd_ws.ptr;
        double *dtl = ws + o_tl, *dtq = ws + o_tq, *dpost = ws + o_po;
        int *dcn = (int *)(ws + o_cn), *dcode = (int *)(ws + o_co), *dinfo = (int *)(ws + o_in), *dinfo1 = (int *)(ws + o_i1), *dvote = (int *)(ws + o_vo);
        double *ddist = (double *)ctx->gemm_out.ptr, *dw = ddist + mk, *dpred = dw + mk;
        int *dind = (int *)(dpred + np);
        const int *dcls = cls_train;
        lw_queries qs{Zq, ldzq, Xq, ldxq};
        JCH_TRY(jch_lw_front_stage(ctx, model, host, m, &qs));
        if (host) {
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_cl, cls_train, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
            dcls = (const int *)(ws + o_cl);
        }
        if (!Zq) JCH_TRY(jch_lw_front_map(ctx, model, m, &qs));
        int *sflags = nullptr;
        JCH_TRY(jch_knn_dispatch(ctx, jch_knn_make_args(model->Zt, n, dd, qs.Zq, qs.ldzq, m, k, h, tol, dind, ddist, dw), model->has_screen ? &model->screen : nullptr,
                                 &model->screen_off, &sflags));
        const unsigned gb = (unsigned)std::max<size_t>(1, std::min<size_t>((mk + 255) / 256, (size_t)ctx->cus * 8));
        hipLaunchKernelGGL(k_da_gather_cls, dim3(gb), dim3(256), 0, ctx->stream, dcls, dind, mk, dcn);
        // (a unanimous neighbourhood is not fitted: its scores and predictions stay the zeros written here)
        JCH_HIP(ctx, hipMemsetAsync(dtl, 0, sizeof(double) * ntl, ctx->stream));
        JCH_HIP(ctx, hipMemsetAsync(dtq, 0, sizeof(double) * ntq, ctx->stream));
        JCH_HIP(ctx, hipMemsetAsync(dpred, 0, sizeof(double) * np, ctx->stream));
        g.Xq = qs.Xq; g.ldxq = qs.ldxq; g.ind = dind; g.w = dw; g.pred = dpred; g.tloc = dtl; g.tqv = dtq; g.cls = dcls; g.info = dinfo1;
        if (generic) {
            std::vector<int> hcn(mk);
            JCH_HIP(ctx, hipMemcpyAsync(hcn.data(), dcn, sizeof(int) * mk, hipMemcpyDeviceToHost, ctx->stream));
            JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
            JCH_TRY(jch_lw_generic_fits_da(ctx, g, hcn.data()));
        } else JCH_TRY(jch_launch_locw_pspace(ctx, g));
        if (kind == 0) {
            hipLaunchKernelGGL(k_rda_finish, dim3((unsigned)std::min<int64_t>(m, (int64_t)ctx->cus * 8)), dim3(256), sizeof(int) * (size_t)nlev, ctx->stream, dpred, dinfo1, dcn,
                               (int)m, (int)k, (int)nlev, le, dpost, dcode, dinfo);
        } else {
            gda_args a;
            a.T = dtl; a.tstride = (int64_t)k * nlv_hi; a.ldt = nlv_hi; a.tq = dtq; a.ldq = nlv_hi; a.cls = dcn; a.m = (int)m; a.k = k; a.a = a_fit; a.nlev = nlev;
            a.kind = kind; a.prior = prior; a.nlv_lo = nlv_lo; a.nlv_hi = nlv_hi; a.post = dpost; a.code = dcode; a.info = dinfo;
            a.scratch = at.glob ? ws + o_sc : nullptr; a.per_block = slab;
            JCH_TRY(jch_launch_knn_gda(ctx, a, at.nb));
            JCH_TRY(jch_knn_vote(ctx, JCH_LOC_DEVICE, dcls, n, nlev, dind, dw, m, k, dvote, nullptr));
            hipLaunchKernelGGL(k_da_vote_fill, dim3((unsigned)std::max<size_t>(1, std::min<size_t>((nm + 255) / 256, (size_t)ctx->cus * 8))), dim3(256), 0, ctx->stream,
                               dinfo, dvote, (int)m, le, dcode);
        }
        JCH_HIP(ctx, hipGetLastError());
        JCH_HIP(ctx, hipMemcpyAsync(code, dcode, sizeof(int) * nm, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(post, dpost, sizeof(double) * np, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(info, dinfo, sizeof(int) * nm, hipMemcpyDeviceToHost, ctx->stream));
        if (tloc_out && nlv_hi > 0) JCH_HIP(ctx, hipMemcpyAsync(tloc_out, dtl, sizeof(double) * mk * (size_t)nlv_hi, hipMemcpyDeviceToHost, ctx->stream));
        if (tq_out && nlv_hi > 0) JCH_HIP(ctx, hipMemcpyAsync(tq_out, dtq, sizeof(double) * (size_t)m * nlv_hi, hipMemcpyDeviceToHost, ctx->stream));
        if (ind_out) JCH_HIP(ctx, hipMemcpyAsync(ind_out, dind, sizeof(int) * mk, hipMemcpyDeviceToHost, ctx->stream));
        if (dist_out) JCH_HIP(ctx, hipMemcpyAsync(dist_out, ddist, sizeof(double) * mk, hipMemcpyDeviceToHost, ctx->stream));
        if (w_out) JCH_HIP(ctx, hipMemcpyAsync(w_out, dw, sizeof(double) * mk, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    });
}
