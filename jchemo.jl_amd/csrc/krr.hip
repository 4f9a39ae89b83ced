// Kernel ridge regression (src/krr.jl:128-202): jch_krr_fit and jch_krr_solve (include/jchemo_hip.h).
//
// The reference takes svd(Kd) of Kd = sqrtD Kc sqrtD and keeps U (n x n); its outputs only need
//   coef(lb).A = U diag(1 / (eig + lb^2)) U' sqrtD Y = (Kd + lb^2 I)^-1 sqrtD Y          (:170-172)
//   coef(lb).df = 1 + sum eig / (eig + lb^2) = 1 + n - lb^2 trace((Kd + lb^2 I)^-1)       (:175-176)
// and Kd + lb^2 I is symmetric positive definite for a PSD kernel and lb > 0: jch_krr_fit builds Kd and B = sqrtD Y with the
// launches of kplsr / kpca, jch_krr_solve factors a copy of Kd + lb^2 I (chol.hip), solves for A and takes the trace as
// |L^-1|_F^2.  predict (:187-202) is jch_kplsr_transform with R = sqrtD A.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "jch_internal.h"

#define KR_NT 256

// out[i, j] = r_i in[i, j] c_j (c = null: 1); out may be in (element-wise)
__global__ __launch_bounds__(KR_NT) void k_kr_scale(const double *in, int64_t ldi, double *out, int64_t ldo, int64_t n, int64_t m,
                                                    const double *__restrict__ r, const double *__restrict__ c)
{
    const int64_t tot = n * m;
    for (int64_t e = (int64_t)blockIdx.x * KR_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * KR_NT) {
        const int64_t j = e / n, i = e - j * n;
        const double v = r[i] * in[(size_t)i + (size_t)j * (size_t)ldi];
        out[(size_t)i + (size_t)j * (size_t)ldo] = c ? v * c[j] : v;
    }
}
__global__ __launch_bounds__(KR_NT) void k_kr_adddiag(double *A, int64_t n, double v)
{
    const int64_t i = (int64_t)blockIdx.x * KR_NT + threadIdx.x;
    if (i < n) A[(size_t)i * (size_t)(n + 1)] += v;
}

extern "C" int32_t jch_krr_fit(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, double *X, int64_t n, int64_t p,
                               int64_t ldx, const double *Y, int64_t q, int64_t ldy, const double *weights, int32_t scal, double *Kd, double *K_out,
                               double *B, double *vtot, double *weights_norm, double *xscales, double *ymeans)
{
    static const char *who = "jch_krr_fit";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(jch_check_kernel(ctx, who, kind, degree));
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (!X || n < 1 || p < 1 || ldx < n) return jch_fail(ctx, JCH_EINVAL, "%s: bad X (n=%lld p=%lld ldx=%lld)", who, (long long)n, (long long)p, (long long)ldx);
    if (!Y || q < 1 || ldy < n) return jch_fail(ctx, JCH_EINVAL, "%s: bad Y (q=%lld ldy=%lld)", who, (long long)q, (long long)ldy);
    if (!Kd) return jch_fail(ctx, JCH_EINVAL, "%s: Kd is NULL", who);
    if (n > (1 << 20)) return jch_fail(ctx, JCH_EINVAL, "%s: n=%lld too large", who, (long long)n);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST;
    const size_t nn = (size_t)n;
    std::vector<double> xs((size_t)p, 1.0), xm((size_t)p), ym((size_t)q);
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        // ---- device views of X, Y and the raw weights
        double *dX = X;
        int64_t ldxd = ldx;
        if (host) {
            JCH_TRY(jch_reserve(ctx, ctx->dk_x, sizeof(double) * nn * p));
            JCH_TRY(jch_copy2d(ctx, (double *)ctx->dk_x.ptr, n, X, ldx, n, p, hipMemcpyHostToDevice));
            dX = (double *)ctx->dk_x.ptr; ldxd = n;
        }
        jch_carve cv;
        const size_t oY = cv.take(nn * q), oB = cv.take(nn * q), owr = cv.take(nn), ow = cv.take(nn), osw = cv.take(nn), ovt = cv.take(nn), ohdr = cv.take(8), os = cv.take(8),
                     oxs = cv.take((size_t)p);
        JCH_TRY(jch_reserve(ctx, ctx->kr_ws, sizeof(double) * cv.off));
        double *ws = (double *)ctx->kr_ws.ptr;
        double *Yd = ws + oY, *Bd = ws + oB, *wraw = ws + owr, *wn = ws + ow, *sw = ws + osw, *vt = ws + ovt, *hdr = ws + ohdr, *sdev = ws + os,
               *xs_dev = ws + oxs;
        const double *dY = Y;
        int64_t ldyd = ldy;
        JCH_TRY(jch_stage_in(ctx, host, Yd, n, q, &dY, &ldyd));
        const double *dw = weights;
        if (host && weights) {
            JCH_HIP(ctx, hipMemcpyAsync(wraw, weights, sizeof(double) * nn, hipMemcpyHostToDevice, ctx->stream));
            dw = wraw;
        }
        JCH_TRY(jch_launch_weights(ctx, dw, n, wn, hdr));   // `mweight` (src/krr.jl:135)
        JCH_TRY(jch_launch_sqrt(ctx, wn, n, sw));
        // ---- scal: xscales = colstd(X, w), X divided by them in place (:136-140; X is not centred); ymeans = colmean(Y, w) (:141)
        if (scal) {
            JCH_TRY(jch_col_stats(ctx, JCH_LOC_DEVICE, dX, n, p, ldxd, dw, xm.data(), xs.data()));
            JCH_HIP(ctx, hipMemcpyAsync(xs_dev, xs.data(), sizeof(double) * (size_t)p, hipMemcpyHostToDevice, ctx->stream));
            JCH_TRY(jch_launch_divcols(ctx, dX, ldxd, n, p, xs_dev));
            if (host) JCH_TRY(jch_copy2d(ctx, X, ldx, dX, n, n, p, hipMemcpyDeviceToHost));
        }
        JCH_TRY(jch_col_stats(ctx, JCH_LOC_DEVICE, dY, n, q, ldyd, dw, ym.data(), nullptr));
        // ---- K = kern(X, X), vtot = K w, Kc = K - vtot' - vtot + w'vtot (:143-147) in the caller's buffer, then Kd = sqrtD Kc sqrtD (:150-151)
        JCH_TRY(jch_launch_kp_centred_gram(ctx, kind, gamma, coef0, degree, dX, n, ldxd, nullptr, p, wn, K_out ? K_out : Kd, Kd, vt, sdev));
        hipLaunchKernelGGL(k_kr_scale, dim3(jch_grid1(ctx, n * n)), dim3(KR_NT), 0, ctx->stream, Kd, n, Kd, n, n, n, sw, sw);
        JCH_HIP(ctx, hipGetLastError());
        // ---- B = sqrtD Y (Y raw, as `U' * sqrtD * Y` :156)
        hipLaunchKernelGGL(k_kr_scale, dim3(jch_grid1(ctx, n * q)), dim3(KR_NT), 0, ctx->stream, dY, ldyd, Bd, n, n, q, sw, nullptr);
        JCH_HIP(ctx, hipGetLastError());
        const hipMemcpyKind dir = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (B) JCH_HIP(ctx, hipMemcpyAsync(B, Bd, sizeof(double) * nn * q, dir, ctx->stream));
        if (vtot) JCH_HIP(ctx, hipMemcpyAsync(vtot, vt, sizeof(double) * nn, dir, ctx->stream));
        if (weights_norm) JCH_HIP(ctx, hipMemcpyAsync(weights_norm, wn, sizeof(double) * nn, dir, ctx->stream));
        return JCH_OK;
    }));
    if (xscales) std::copy(xs.begin(), xs.end(), xscales);
    if (ymeans) std::copy(ym.begin(), ym.end(), ymeans);
    return JCH_OK;
}

extern "C" int32_t jch_krr_solve(jch_ctx *ctx, int32_t loc, const double *Kd, int64_t n, const double *B, int64_t q, const double *weights_norm,
                                 double lb, int32_t want_df, double *A, double *alpha, double *df, int32_t *info)
{
    static const char *who = "jch_krr_solve";
    if (!ctx) return JCH_EINVAL;
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (!Kd || !B || !weights_norm || n < 1 || q < 1 || n > (1 << 20))
        return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments (n=%lld q=%lld)", who, (long long)n, (long long)q);
    if (!(lb > 0.0) || !std::isfinite(lb))
        return jch_fail(ctx, JCH_EINVAL, "%s: lb = %g must be finite and > 0 (Kd is singular by construction: Kd sqrt(w) = 0)", who, lb);
    if (want_df && !df) return jch_fail(ctx, JCH_EINVAL, "%s: want_df without df", who);
    if (ctx->nranks > 1) return jch_fail(ctx, JCH_EINVAL, "%s: one rank only (communicator of %d)", who, ctx->nranks);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST;
    const size_t nn = (size_t)n;
    JCH_TRY(jch_reserve(ctx, ctx->chol_a, sizeof(double) * nn * nn));
    jch_carve cv;
    const size_t oA = cv.take(nn * q), oal = cv.take(nn * q), ow = cv.take(nn), osw = cv.take(nn), odf = cv.take(8);
    JCH_TRY(jch_reserve(ctx, ctx->kr_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->kr_ws.ptr;
    double *Ad = ws + oA, *ald = ws + oal, *wn = ws + ow, *sw = ws + osw, *fro = ws + odf, *M = (double *)ctx->chol_a.ptr;
    int *idev = nullptr;
    JCH_TRY(jch_chol_info_word(ctx, &idev));
    int hinfo = 0;
    double hfro = 0.0;
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        const hipMemcpyKind in = host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, out = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        JCH_HIP(ctx, hipMemcpyAsync(Ad, B, sizeof(double) * nn * q, in, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(wn, weights_norm, sizeof(double) * nn, in, ctx->stream));
        JCH_TRY(jch_launch_sqrt(ctx, wn, n, sw));
        // ---- M = Kd + lb^2 I = L L'; A = M^-1 B (:170-172); alpha = sqrtD A (what predict multiplies with, :198)
        JCH_HIP(ctx, hipMemcpyAsync(M, Kd, sizeof(double) * nn * nn, hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(k_kr_adddiag, dim3((unsigned)((n + KR_NT - 1) / KR_NT)), dim3(KR_NT), 0, ctx->stream, M, n, lb * lb);
        JCH_HIP(ctx, hipGetLastError());
        JCH_TRY(jch_launch_chol_factor(ctx, M, n, n, idev));
        JCH_TRY(jch_launch_chol_solve(ctx, M, n, n, Ad, q, n, idev));
        hipLaunchKernelGGL(k_kr_scale, dim3(jch_grid1(ctx, n * q)), dim3(KR_NT), 0, ctx->stream, Ad, n, ald, n, n, q, sw, nullptr);
        JCH_HIP(ctx, hipGetLastError());
        // ---- df = 1 + n - lb^2 trace(M^-1), trace(M^-1) = |L^-1|_F^2 (:175-176)
        if (want_df) JCH_TRY(jch_launch_chol_inv_fro2(ctx, M, n, n, fro, idev));
        JCH_HIP(ctx, hipMemcpyAsync(&hinfo, idev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        if (want_df) JCH_HIP(ctx, hipMemcpyAsync(&hfro, fro, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (info) *info = hinfo;
        if (hinfo != 0) {
            ctx->chol_L = nullptr;
            return jch_fail(ctx, JCH_EINVAL, "%s: Kd + lb^2 I is not positive definite (lb = %g): the pivot of column %d is not > 0; the kernel / its "
                            "parameters are not PSD enough for this lb", who, lb, hinfo);
        }
        if (A) JCH_HIP(ctx, hipMemcpyAsync(A, Ad, sizeof(double) * nn * q, out, ctx->stream));
        if (alpha) JCH_HIP(ctx, hipMemcpyAsync(alpha, ald, sizeof(double) * nn * q, out, ctx->stream));
        return JCH_OK;
    }));
    if (want_df) *df = 1.0 + (double)n - lb * lb * hfro;
    return JCH_OK;
}
