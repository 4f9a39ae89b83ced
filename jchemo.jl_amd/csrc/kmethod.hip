// What the kernel-method entry points share (dkplsr.hip, kplsr.hip, kpca.hip, krr.hip): the kernel / rank check,
// the column divide and sqrt kernels, and transform / predict over Gram blocks of new rows.
#include <math.h>

#include <algorithm>

#include "jch_internal.h"

// A[:, k] /= s[k]  (`scale!`, src/utility.jl: X ./ xscales')
__global__ __launch_bounds__(256) void k_km_divcols(double *__restrict__ A, int64_t lda, int64_t n, int64_t cols, const double *__restrict__ s)
{
    const int64_t tot = n * cols;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) {
        const int64_t k = e / n, i = e - k * n;
        A[(size_t)i + (size_t)k * (size_t)lda] /= s[k];
    }
}
// sw = sqrt(w)
__global__ __launch_bounds__(256) void k_km_sqrt(const double *__restrict__ w, int64_t n, double *__restrict__ sw)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) sw[i] = sqrt(w[i]);
}

int32_t jch_check_kernel(jch_ctx *ctx, const char *who, int32_t kind, int32_t degree)
{
    if (kind != JCH_KERN_RBF && kind != JCH_KERN_POL) return jch_fail(ctx, JCH_EINVAL, "%s: unknown kernel kind %d", who, kind);
    if (kind == JCH_KERN_POL && degree < 1) return jch_fail(ctx, JCH_EINVAL, "%s: degree = %d must be >= 1", who, degree);
    if (ctx->nranks > 1) return jch_fail(ctx, JCH_EINVAL, "%s: the Gram matrix is not sharded: one rank only (communicator of %d)", who, ctx->nranks);
    return JCH_OK;
}

int32_t jch_launch_divcols(jch_ctx *ctx, double *A, int64_t lda, int64_t n, int64_t cols, const double *s_dev)
{
    hipLaunchKernelGGL(k_km_divcols, dim3(jch_grid1(ctx, n * cols)), dim3(256), 0, ctx->stream, A, lda, n, cols, s_dev);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

int32_t jch_launch_sqrt(jch_ctx *ctx, const double *w, int64_t n, double *sw)
{
    hipLaunchKernelGGL(k_km_sqrt, dim3(jch_grid1(ctx, n)), dim3(256), 0, ctx->stream, w, n, sw);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

int64_t jch_qblock(int knob, int64_t n)
{
    if (knob >= 1) return knob;
    return std::max<int64_t>(1, ((int64_t)1 << 27) / n);
}

int32_t jch_kblocks_begin(jch_ctx *ctx, const char *who, int32_t loc, int32_t kind, int32_t degree, bool ptrs_ok, int64_t m, int64_t n, int64_t p,
                          int64_t ldx, int64_t ldxt, int64_t ldo, int qblock_knob, int64_t *mb)
{
    *mb = 0;
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(jch_check_kernel(ctx, who, kind, degree));
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (!ptrs_ok || m < 0 || n < 1 || p < 1 || ldx < m || ldxt < n || ldo < m)
        return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments (m=%lld n=%lld p=%lld ldx=%lld ldxt=%lld ldo=%lld)", who, (long long)m, (long long)n,
                        (long long)p, (long long)ldx, (long long)ldxt, (long long)ldo);
    if (m == 0) return JCH_OK;
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    *mb = std::min<int64_t>(m, jch_qblock(qblock_knob, n));
    return JCH_OK;
}

int32_t jch_kblocks_run(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X, int64_t m, int64_t p,
                        int64_t ldx, const double *xscale, const double *Xt, int64_t n, int64_t ldxt, int64_t mb, int64_t ncols, double *out,
                        int64_t ldo, const jch_kblock_step &step)
{
    const bool host = loc == JCH_LOC_HOST;
    return jch_synced(ctx, true, [&]() -> int32_t {   // (from the top: the caller may have queued uploads of its model's host vectors)
        if (host) {
            JCH_TRY(jch_reserve(ctx, ctx->dk_x, sizeof(double) * (size_t)n * p));
            JCH_TRY(jch_reserve(ctx, ctx->dk_q, sizeof(double) * (size_t)mb * p));
            JCH_TRY(jch_reserve(ctx, ctx->dk_o, sizeof(double) * (size_t)mb * ncols));
        }
        JCH_TRY(jch_reserve(ctx, ctx->dk_k, sizeof(double) * (size_t)mb * n));
        const double *dXt = Xt;
        int64_t ldxtd = ldxt;
        JCH_TRY(jch_stage_in(ctx, host, (double *)ctx->dk_x.ptr, n, p, &dXt, &ldxtd));
        double *Kb = (double *)ctx->dk_k.ptr;
        for (int64_t r0 = 0; r0 < m; r0 += mb) {
            const int64_t rows = std::min(mb, m - r0);
            const double *Zb = X + r0;
            int64_t ldz = ldx;
            JCH_TRY(jch_stage_in(ctx, host, (double *)ctx->dk_q.ptr, rows, p, &Zb, &ldz));
            double *ob = host ? (double *)ctx->dk_o.ptr : out + r0;
            const int64_t ldob = host ? rows : ldo;
            JCH_TRY(jch_launch_kgram(ctx, kind, Zb, rows, ldz, xscale, dXt, n, ldxtd, nullptr, p, gamma, coef0, degree, false, Kb, rows));
            JCH_TRY(step(Kb, rows, ob, ldob));
            if (host) JCH_TRY(jch_copy2d(ctx, out + r0, ldo, ob, ldob, rows, ncols, hipMemcpyDeviceToHost));
        }
        return JCH_OK;
    });
}
