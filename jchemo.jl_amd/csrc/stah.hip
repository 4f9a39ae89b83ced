// Stahel-Donoho outlyingness (src/stah.jl:37-58, src/occstah.jl:55-73) — jch_stah, include/jchemo_hip.h; DESIGN.md §18.
//
//   d[i] = max_j | (t_ij - mu_j) / s_j |,   T = ((X - 1 mu_scal') diag(1 / s_scal)) P,   mu_j = median(T[:, j]), s_j = mad(T[:, j])
//
// The n x a matrix T (16 GB at n = 1e6, a = 2000) never exists: P is walked in column panels of at most ST_PANEL_BYTES of T and ST_PANEL_MAXCOLS
// columns.  Per panel: (i) the projection by jch_launch_affine_gemm (gemm.hip) with the centring and scaling folded into the coefficients as
// jch_affine_gemm folds them; (ii) when fitting, the panel's medians and MADs by jch_launch_col_median_mad (colselect.hip), device to device;
// (iii) k_st_rowmax.  All folded coefficients go up in one copy ahead of the loop, which is enqueued without a host synchronisation.
//
//   k_st_rowmax   one lane per row, the panel's columns in order, four loads in flight: one coalesced read of the panel.  d[i] = max(d[i],
//                 |fl(fl(t - mu_j) / s_j)|) with a true division (`cscale!`); a NaN term takes the row's maximum and keeps it (Julia's `maximum`),
//                 and stays in its row.  Nothing guards s_j = 0: a constant direction gives Inf or NaN (0 / 0) as in the reference.
// gfx950, hipcc -O3, no scratch: k_st_rowmax 50 VGPRs.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "jch_internal.h"

#define ST_PANEL_BYTES ((size_t)1 << 30)   // of T per panel: 128 columns at n = 1e6
#define ST_PANEL_MAXCOLS 512                // the selection's counters are 32 KB per column

__global__ __launch_bounds__(256) void k_st_rowmax(const double *__restrict__ T, int64_t n, int64_t ldt, int bw, const double *__restrict__ mu,
                                                   const double *__restrict__ s, double *__restrict__ d, int first)
{
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        double m = first ? 0.0 : d[i];
        auto take = [&](double t, int j) {
            const double v = fabs((t - mu[j]) / s[j]);
            m = (v > m || v != v) ? v : m;     // once m is NaN both tests fail for every later v: it stays
        };
        const double *t = T + i;
        int j = 0;
        for (; j + 3 < bw; j += 4) {
            const double t0 = t[(size_t)j * ldt], t1 = t[(size_t)(j + 1) * ldt], t2 = t[(size_t)(j + 2) * ldt], t3 = t[(size_t)(j + 3) * ldt];
            take(t0, j); take(t1, j + 1); take(t2, j + 2); take(t3, j + 3);
        }
        for (; j < bw; ++j) take(t[(size_t)j * ldt], j);
        d[i] = m;
    }
}

extern "C" int32_t jch_stah(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *mu_scal, const double *s_scal,
                            const double *P, int64_t a, int64_t ldp, int32_t fit, double *mu, double *s, double *d)
{
    if (!ctx) return JCH_EINVAL;
    if (!X || !P || !mu || !s || !d || n < 1 || p < 1 || p > (1 << 30) || a < 1 || ldx < n || ldp < p) return jch_fail(ctx, JCH_EINVAL, "jch_stah: bad arguments");
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "jch_stah: bad loc");
    if (ctx->nranks > 1) return jch_fail(ctx, JCH_EINVAL, "jch_stah: one rank only (communicator of %d)", ctx->nranks);
    // panel width: within the budget, a multiple of 16 (the GEMM pads its coefficients to 16 columns) unless fewer fit
    int64_t b = std::min<int64_t>(std::min<int64_t>(a, ST_PANEL_MAXCOLS), std::max<int64_t>(1, (int64_t)(ST_PANEL_BYTES / (sizeof(double) * (size_t)n))));
    if (b >= 16 && b < a) b -= b % 16;
    const int64_t npanel = (a + b - 1) / b;
    auto kpad_of = [&](int64_t k) { return (int)((std::min<int64_t>(b, a - k * b) + 15) / 16 * 16); };   // a narrower last panel pads to its own width
    const size_t blk = (size_t)(p + 1) * kpad_of(0);   // per panel: Bs [p][kpad] = diag(1 / s_scal) P_b, then the bias - mu_scal' Bs
    std::vector<double> hb(blk * (size_t)npanel, 0.0);
    for (int64_t c = 0; c < a; ++c) {
        const int kpad = kpad_of(c / b);
        double *Bs = hb.data() + blk * (size_t)(c / b), *b2 = Bs + (size_t)p * kpad;
        const int64_t cc = c % b;
        double acc = 0.0;
        for (int64_t j = 0; j < p; ++j) {
            const double v = P[j + c * ldp] / (s_scal ? s_scal[j] : 1.0);
            Bs[j * kpad + cc] = v;
            if (mu_scal) acc -= mu_scal[j] * v;
        }
        b2[cc] = acc;
    }
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    JCH_TRY(jch_reserve(ctx, ctx->gemm_b, sizeof(double) * hb.size()));
    JCH_TRY(jch_reserve(ctx, ctx->st_t, sizeof(double) * (size_t)n * (size_t)b));
    JCH_TRY(jch_reserve(ctx, ctx->st_ms, sizeof(double) * (2 * (size_t)a + (loc == JCH_LOC_HOST ? (size_t)n : 0))));
    if (fit) JCH_TRY(jch_colselect_reserve(ctx, b));
    if (loc == JCH_LOC_HOST) JCH_TRY(jch_reserve(ctx, ctx->xq, sizeof(double) * (size_t)n * (size_t)p));
    double *dB = (double *)ctx->gemm_b.ptr, *dT = (double *)ctx->st_t.ptr, *dmu = (double *)ctx->st_ms.ptr, *ds = dmu + a;
    return jch_synced(ctx, true, [&]() -> int32_t {
        JCH_HIP(ctx, hipMemcpyAsync(dB, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice, ctx->stream));
        const double *dX = X;
        double *dd = d;
        int64_t ldxd = ldx;
        JCH_TRY(jch_stage_in(ctx, loc == JCH_LOC_HOST, (double *)ctx->xq.ptr, n, p, &dX, &ldxd));   // staged once for all panels
        if (loc == JCH_LOC_HOST) dd = ds + a;
        if (!fit) {
            JCH_HIP(ctx, hipMemcpyAsync(dmu, mu, sizeof(double) * (size_t)a, hipMemcpyHostToDevice, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(ds, s, sizeof(double) * (size_t)a, hipMemcpyHostToDevice, ctx->stream));
        }
        for (int64_t k = 0; k < npanel; ++k) {
            const int64_t c0 = k * b;
            const int bw = (int)std::min<int64_t>(b, a - c0);
            const double *Bk = dB + blk * (size_t)k;
            const int kpad = kpad_of(k);
            JCH_TRY(jch_launch_affine_gemm(ctx, dX, n, (int)p, ldxd, Bk, bw, kpad, Bk + (size_t)p * kpad, dT, n));
            if (fit) JCH_TRY(jch_launch_col_median_mad(ctx, dT, n, bw, n, dmu + c0, ds + c0));
            hipLaunchKernelGGL(k_st_rowmax, dim3(jch_grid1(ctx, n)), dim3(256), 0, ctx->stream, dT, n, n, bw, dmu + c0, ds + c0, dd, k == 0 ? 1 : 0);
            JCH_HIP(ctx, hipGetLastError());
        }
        if (loc == JCH_LOC_HOST) JCH_HIP(ctx, hipMemcpyAsync(d, dd, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        if (fit) {
            JCH_HIP(ctx, hipMemcpyAsync(mu, dmu, sizeof(double) * (size_t)a, hipMemcpyDeviceToHost, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(s, ds, sizeof(double) * (size_t)a, hipMemcpyDeviceToHost, ctx->stream));
        }
        return JCH_OK;
    });
}
