// Direct kernel PLS (src/dkplsr.jl): jch_kernel_gram, jch_dkplsr_fit, jch_dkplsr_transform, jch_dkplsr_predict
// (include/jchemo_hip.h).  The Gram comes from kgram.hip; the fit on it is jch_plskern_fit's device path, the accessors are
// jch_transform / jch_predict on Gram blocks of the new rows.
#include <stdlib.h>

#include <algorithm>

#include "jch_internal.h"

namespace {

// transform (pred == false) or predict over the new rows, block by block
struct dk_model {
    const double *xmeans, *xscales, *ymeans, *yscales, *R, *C;
    int64_t q; int32_t lo, hi, nlv;
};

int32_t dk_apply(jch_ctx *ctx, const char *who, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X, int64_t m,
                 int64_t p, int64_t ldx, const double *xscale, const double *Xt, int64_t n, int64_t ldxt, const dk_model &md, bool pred,
                 int64_t ncols, double *out, int64_t ldo)
{
    int64_t mb = 0;
    JCH_TRY(jch_kblocks_begin(ctx, who, loc, kind, degree, X && Xt && out, m, n, p, ldx, ldxt, ldo, jch_knob("JCH_DKPLSR_QBLOCK", 0), &mb));
    if (mb == 0) return JCH_OK;
    return jch_kblocks_run(ctx, loc, kind, gamma, coef0, degree, X, m, p, ldx, xscale, Xt, n, ldxt, mb, ncols, out, ldo,
                           [&](double *Kb, int64_t rows, double *ob, int64_t ldob) {
        if (pred)
            return jch_predict(ctx, JCH_LOC_DEVICE, Kb, rows, n, rows, md.xmeans, md.xscales, md.ymeans, md.yscales, md.R, md.C, md.q, md.lo, md.hi, ob, ldob);
        return jch_transform(ctx, JCH_LOC_DEVICE, Kb, rows, n, rows, md.xmeans, md.xscales, md.R, md.nlv, ob, ldob);
    });
}

}  // namespace

extern "C" int32_t jch_kernel_gram(jch_ctx *ctx, int32_t loc, int32_t kind, const double *Z, int64_t m, int64_t ldz, const double *zscale,
                                   const double *X, int64_t n, int64_t ldx, const double *xscale, int64_t p, double gamma, double coef0,
                                   int32_t degree, double *K, int64_t ldk)
{
    static const char *who = "jch_kernel_gram";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(jch_check_kernel(ctx, who, kind, degree));
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (!Z || !X || !K || m < 1 || n < 1 || p < 1 || ldz < m || ldx < n || ldk < m)
        return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments (m=%lld n=%lld p=%lld ldz=%lld ldx=%lld ldk=%lld)", who, (long long)m, (long long)n,
                        (long long)p, (long long)ldz, (long long)ldx, (long long)ldk);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool same_scales = zscale == xscale || (zscale && xscale && memcmp(zscale, xscale, sizeof(double) * (size_t)p) == 0);
    const bool sym = Z == X && ldz == ldx && m == n && same_scales;
    const bool host = loc == JCH_LOC_HOST;
    if (host) {
        JCH_TRY(jch_reserve(ctx, ctx->dk_x, sizeof(double) * (size_t)n * p));
        if (!sym) JCH_TRY(jch_reserve(ctx, ctx->dk_q, sizeof(double) * (size_t)m * p));
        JCH_TRY(jch_reserve(ctx, ctx->dk_k, sizeof(double) * (size_t)m * n));
    }
    return jch_synced(ctx, true, [&]() -> int32_t {
        const double *dZ = Z, *dX = X;
        int64_t ldzd = ldz, ldxd = ldx;
        JCH_TRY(jch_stage_in(ctx, host, (double *)ctx->dk_x.ptr, n, p, &dX, &ldxd));
        if (host && sym) { dZ = dX; ldzd = ldxd; }
        else JCH_TRY(jch_stage_in(ctx, host, (double *)ctx->dk_q.ptr, m, p, &dZ, &ldzd));
        double *dK = host ? (double *)ctx->dk_k.ptr : K;
        const int64_t ldkd = host ? m : ldk;
        JCH_TRY(jch_launch_kgram(ctx, kind, dZ, m, ldzd, zscale, dX, n, ldxd, xscale, p, gamma, coef0, degree, sym, dK, ldkd));
        if (host) JCH_TRY(jch_copy2d(ctx, K, ldk, dK, ldkd, m, n, hipMemcpyDeviceToHost));
        return JCH_OK;
    });
}

extern "C" int32_t jch_dkplsr_fit(jch_ctx *ctx, const jch_pls_desc *desc, int32_t kind, double gamma, double coef0, int32_t degree,
                                  void *X, int64_t ldx, void *Y, int64_t ldy, const double *weights, double *K_out, double *T, double *P,
                                  double *R, double *W, double *C, double *TT, double *xmeans, double *xscales, double *ymeans,
                                  double *yscales, double *weights_norm, double *dk_xscales, double *dk_yscales, int32_t *nlv_out)
{
    static const char *who = "jch_dkplsr_fit";
    if (!ctx) return JCH_EINVAL;
    if (!desc) return jch_fail(ctx, JCH_EINVAL, "%s: desc is NULL", who);
    if (desc->dtype != JCH_F64) return jch_fail(ctx, JCH_EINVAL, "%s: Float64 only (dtype %d)", who, desc->dtype);
    JCH_TRY(jch_check_kernel(ctx, who, kind, degree));
    const jch_pls_desc &d = *desc;
    if (d.n < 1 || d.p < 1 || d.q < 1 || d.nlv < 1) return jch_fail(ctx, JCH_EINVAL, "%s: empty input or nlv < 1", who);
    if (d.n > (1 << 20) || d.q > (1 << 12)) return jch_fail(ctx, JCH_EINVAL, "%s: n=%lld or q=%lld too large", who, (long long)d.n, (long long)d.q);
    if (d.loc != JCH_LOC_HOST && d.loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, d.loc);
    if (!X || !Y) return jch_fail(ctx, JCH_EINVAL, "%s: X or Y is NULL", who);
    if (ldx < d.n || ldy < d.n) return jch_fail(ctx, JCH_EINVAL, "%s: ldx/ldy smaller than n", who);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t n = d.n, p = d.p, q = d.q;
    const bool host = d.loc == JCH_LOC_HOST, inplace = d.inplace != 0, scal = d.scal != 0;
    const int64_t kcap = std::min<int64_t>(n, d.nlv);
    std::vector<double> xs((size_t)p, 1.0), ys((size_t)q, 1.0), mtmp((size_t)std::max(p, q));
    int32_t got = 0;
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        // ---- device views: X (read; scaled in place only for dkplsr!), Y (the inner plskern! centres it: a working copy unless dkplsr!)
        double *dX = (double *)X, *dY = (double *)Y;
        const double *dw = weights;
        int64_t ldxd = ldx, ldyd = ldy;
        if (host) {
            JCH_TRY(jch_reserve(ctx, ctx->dk_x, sizeof(double) * (size_t)n * p));
            JCH_TRY(jch_copy2d(ctx, (double *)ctx->dk_x.ptr, n, (const double *)X, ldx, n, p, hipMemcpyHostToDevice));
            dX = (double *)ctx->dk_x.ptr; ldxd = n;
        }
        if (host || !inplace) {
            JCH_TRY(jch_reserve(ctx, ctx->dk_y, sizeof(double) * (size_t)n * q));
            JCH_TRY(jch_copy2d(ctx, (double *)ctx->dk_y.ptr, n, (const double *)Y, ldy, n, q, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
            dY = (double *)ctx->dk_y.ptr; ldyd = n;
        }
        // ---- outer scales (src/dkplsr.jl:112-119): the only use of the weights
        JCH_TRY(jch_reserve(ctx, ctx->dk_s, sizeof(double) * ((size_t)p + q + (size_t)n)));
        double *xs_dev = (double *)ctx->dk_s.ptr, *ys_dev = xs_dev + p, *w_dev = ys_dev + q;
        if (scal) {
            if (host && weights) {
                JCH_HIP(ctx, hipMemcpyAsync(w_dev, weights, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
                dw = w_dev;
            }
            JCH_TRY(jch_col_stats(ctx, JCH_LOC_DEVICE, dX, n, p, ldxd, dw, mtmp.data(), xs.data()));
            JCH_TRY(jch_col_stats(ctx, JCH_LOC_DEVICE, dY, n, q, ldyd, dw, mtmp.data(), ys.data()));
            JCH_HIP(ctx, hipMemcpyAsync(xs_dev, xs.data(), sizeof(double) * (size_t)p, hipMemcpyHostToDevice, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(ys_dev, ys.data(), sizeof(double) * (size_t)q, hipMemcpyHostToDevice, ctx->stream));
            JCH_TRY(jch_launch_divcols(ctx, dY, ldyd, n, q, ys_dev));
            if (inplace) JCH_TRY(jch_launch_divcols(ctx, dX, ldxd, n, p, xs_dev));   // dkplsr! hands X back scaled; otherwise the Gram divides on the fly
        }
        // ---- K = kern(X, X) (src/dkplsr.jl:121), the symmetric path
        double *Kd = K_out;
        if (!Kd) {
            JCH_TRY(jch_reserve(ctx, ctx->dk_k, sizeof(double) * (size_t)n * n));
            Kd = (double *)ctx->dk_k.ptr;
        }
        const double *gdiv = scal && !inplace ? xs.data() : nullptr;
        JCH_TRY(jch_launch_kgram(ctx, kind, dX, n, ldxd, gdiv, dX, n, ldxd, gdiv, p, gamma, coef0, degree, true, Kd, n));
        // ---- plskern!(K, Y; nlv) (:122): no weights, in place on K and on the (scaled) Y
        double *Tdev = T, *wn = weights_norm;
        if (host) {
            JCH_TRY(jch_reserve(ctx, ctx->dk_o, sizeof(double) * (size_t)n * (kcap + 1)));
            Tdev = T ? (double *)ctx->dk_o.ptr : nullptr;
            wn = weights_norm ? (double *)ctx->dk_o.ptr + (size_t)n * kcap : nullptr;
        }
        jch_pls_desc di{};
        di.n = n; di.p = n; di.q = q; di.nlv = d.nlv; di.scal = 0; di.dtype = JCH_F64; di.loc = JCH_LOC_DEVICE; di.inplace = 1; di.reserved = 0;
        JCH_TRY(jch_plskern_fit(ctx, &di, Kd, n, dY, ldyd, nullptr, Tdev, P, R, W, C, TT, xmeans, xscales, ymeans, yscales, wn, &got));
        if (host) {
            if (T) JCH_TRY(jch_copy2d(ctx, T, n, Tdev, n, n, got, hipMemcpyDeviceToHost));
            if (weights_norm) JCH_HIP(ctx, hipMemcpyAsync(weights_norm, wn, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
            if (inplace) {
                JCH_TRY(jch_copy2d(ctx, (double *)X, ldx, dX, ldxd, n, p, hipMemcpyDeviceToHost));
                JCH_TRY(jch_copy2d(ctx, (double *)Y, ldy, dY, ldyd, n, q, hipMemcpyDeviceToHost));
            }
        }
        return JCH_OK;
    }));
    if (dk_xscales) std::copy(xs.begin(), xs.end(), dk_xscales);
    if (dk_yscales) std::copy(ys.begin(), ys.end(), dk_yscales);
    if (nlv_out) *nlv_out = got;
    return JCH_OK;
}

extern "C" int32_t jch_dkplsr_transform(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X,
                                        int64_t m, int64_t p, int64_t ldx, const double *xscale, const double *Xtrain, int64_t n,
                                        int64_t ldxt, const double *xmeans, const double *xscales, const double *R, int32_t nlv, double *T,
                                        int64_t ldt)
{
    if (ctx && (!R || nlv < 1)) return jch_fail(ctx, JCH_EINVAL, "jch_dkplsr_transform: R is NULL or nlv < 1");
    const dk_model md{xmeans, xscales, nullptr, nullptr, R, nullptr, 0, 0, 0, nlv};
    return dk_apply(ctx, "jch_dkplsr_transform", loc, kind, gamma, coef0, degree, X, m, p, ldx, xscale, Xtrain, n, ldxt, md, false, nlv, T, ldt);
}

extern "C" int32_t jch_dkplsr_predict(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X,
                                      int64_t m, int64_t p, int64_t ldx, const double *xscale, const double *Xtrain, int64_t n, int64_t ldxt,
                                      const double *xmeans, const double *xscales, const double *ymeans, const double *yscales,
                                      const double *R, const double *C, int64_t q, int32_t nlv_lo, int32_t nlv_hi, const double *dk_yscales,
                                      double *pred, int64_t ldo)
{
    if (ctx && (!R || !C || q < 1 || nlv_lo < 0 || nlv_hi < nlv_lo)) return jch_fail(ctx, JCH_EINVAL, "jch_dkplsr_predict: bad model arguments");
    // pred * Diagonal(dk_yscales) (src/dkplsr.jl:161): folded into the inner model's ymeans / yscales
    std::vector<double> ym((size_t)std::max<int64_t>(q, 1)), ys((size_t)std::max<int64_t>(q, 1));
    for (int64_t k = 0; k < q; ++k) {
        const double s = dk_yscales ? dk_yscales[k] : 1.0;
        ym[k] = (ymeans ? ymeans[k] : 0.0) * s;
        ys[k] = (yscales ? yscales[k] : 1.0) * s;
    }
    const dk_model md{xmeans, xscales, ym.data(), ys.data(), R, C, q, nlv_lo, nlv_hi, 0};
    return dk_apply(ctx, "jch_dkplsr_predict", loc, kind, gamma, coef0, degree, X, m, p, ldx, xscale, Xtrain, n, ldxt, md, true,
                    ((int64_t)nlv_hi - nlv_lo + 1) * q, pred, ldo);
}
