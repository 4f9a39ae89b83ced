// The local fit of the MLR branch of the locally weighted family (src/lwmlr.jl, src/lwmlr_s.jl, src/lwmlrda.jl, src/lwmlrda_s.jl through src/locw.jl
// and src/mlr.jl:69-86) — jch_knn_wls, include/jchemo_hip.h; DESIGN.md §23.
//
// Per query: a weighted least-squares regression of the k neighbours' responses on their d coordinates by Householder QR, then the prediction of the
// query's own row.  m independent small factorisations: one 256-thread workgroup per query, one launch for all of them.
//   k_wls_rowmajor   the row-major copy [X | Y] (n x (d + q)) of the column-major training data, through a 64 x 32 LDS tile: a neighbour is then one
//                    contiguous row of d + q doubles instead of d + q cache lines.
//   k_knn_wls<LDS>   the slab [A | B] (k x (d + q), column-major, leading dimension L = k | 1: odd, so that the d + q lanes that write one gathered
//                    row into d + q columns fall on different banks) lives in dynamic LDS (LDS = true) or, for slabs beyond WLS_LDS_MAX bytes, in a
//                    per-workgroup piece of ctx->kn_ws (LDS = false): the same code, the slab pointer apart (and a __threadfence_block in front of
//                    the barriers).  Steps, with the workgroup barriers between them:
//                      1. sum of the weights (every wave the same lane-strided sum + jch_wave_sum: identical bits, no exchange), w~ and sqrt(w~);
//                      2. the gather of the k rows (an index outside [0, n) gathers NaN);
//                      3. q == 1: are the k responses all == ?  (a vote per wave, the four votes through LDS: block-uniform)  Then k <= d.
//                      4. the columns dealt round-robin to the four waves: weighted mean (lane-strided sum + butterfly), centring, scaling by sqrt(w~);
//                      5. per Householder column j: every wave takes |x|^2 of the column itself (the same bits in all four: no barrier, and no
//                         thread writes v — the one entry in which v differs from x, v_1 = x_1 - alpha, is substituted on reading); the remaining
//                         d - j - 1 + q columns are dealt round-robin to the waves, each takes v'a and applies the update; ONE barrier per column.
//                         alpha = -sign(x_1) |x| (no cancellation in v_1).  r_jj = alpha goes to rd[j]; min and max |r_jj| stay in registers.
//                      6. the rank test (block-uniform, from registers), then per response one wave: back substitution column by column and
//                         pred = ybar + (xq - xbar)'beta, accumulated in the order j = d-1 .. 0.
//                    Every sum has a fixed order and there are no atomics: two runs give identical bits.
// gfx950, hipcc -O3; plain HIP C++.
#include <stdint.h>

#include <algorithm>

#include "jch_internal.h"
#include "lwplsr_dev.h"

#define WLS_LDS_MAX (150 * 1024)   // largest slab (with its vectors) that lives in LDS; beyond: ctx->kn_ws

struct wls_args {
    const double *XY;        // [n][ldr] row-major [X | Y]
    int64_t n;
    int ldr;
    const double *Xq;        // m x d column-major
    int64_t ldq;
    const int *ind;          // [m][k]
    const double *w;         // [m][k]
    int m, k, d, q, L, gshift;
    double *pred;            // m x q column-major, ld m
    int *info;               // [m] or null
    double *scratch;         // null (LDS) or [blocks][per_block]
    size_t per_block;
};

// doubles of one workgroup's slab and vectors: [A | B] (d + q) x L, w~ and sqrt(w~) (k each), the means (d + q), xq - xbar and r_jj (d each), the rows (k ints)
static size_t wls_slab_doubles(int64_t k, int64_t d, int64_t q)
{
    const size_t L = (size_t)k | 1;
    return (size_t)(d + q) * L + 2 * (size_t)k + (size_t)(d + q) + 2 * (size_t)d + ((size_t)k + 1) / 2;
}

__global__ __launch_bounds__(256) void k_wls_rowmajor(const double *__restrict__ X, int64_t ldx, const double *__restrict__ Y, int64_t ldy, int64_t n, int d,
                                                      int q, double *__restrict__ XY)
{
    __shared__ double tile[32][65];
    const int tid = threadIdx.x, nc = d + q;
    const int64_t nchunks = (n + 63) / 64;
    for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        const int64_t r0 = ch * 64;
        for (int ct = 0; ct < nc; ct += 32) {
            __syncthreads();
            {
                const int r = tid & 63;
                for (int c = tid >> 6; c < 32; c += 4) {
                    const int cc = ct + c;
                    if (cc < nc && r0 + r < n) tile[c][r] = cc < d ? X[(size_t)(r0 + r) + (size_t)cc * (size_t)ldx] : Y[(size_t)(r0 + r) + (size_t)(cc - d) * (size_t)ldy];
                }
            }
            __syncthreads();
            {
                const int c = tid & 31, cc = ct + c;
                for (int r = tid >> 5; r < 64; r += 8)
                    if (cc < nc && r0 + r < n) XY[(size_t)(r0 + r) * (size_t)nc + cc] = tile[c][r];
            }
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(256) void k_knn_wls(wls_args g)
{
    extern __shared__ __attribute__((aligned(16))) double wls_dyn[];
    __shared__ int s_any[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int k = g.k, d = g.d, q = g.q, nc = d + q, L = g.L;
    double *S = LDS ? wls_dyn : g.scratch + (size_t)blockIdx.x * g.per_block;   // [nc][L]
    double *wt = S + (size_t)nc * L, *sq = wt + k, *mean = sq + k, *dx = mean + nc, *rd = dx + d;
    int *rows = reinterpret_cast<int *>(rd + d);
    const double nan = __builtin_nan("");
    const int gs = g.gshift, G = 1 << gs, per = 64 >> gs, sub = lane >> gs, c0 = lane & (G - 1);   // G lanes per gathered row
    auto fail_row = [&](int qi, int code) {
        for (int c = tid; c < q; c += 256) g.pred[(size_t)qi + (size_t)c * (size_t)g.m] = nan;
        if (tid == 0 && g.info) g.info[qi] = code;
    };
    for (int qi = blockIdx.x; qi < g.m; qi += gridDim.x) {
        const int *ii = g.ind + (size_t)qi * k;
        const double *ww = g.w + (size_t)qi * k;
        slab_bsync<LDS>();                                      // (the previous query is done with the slab)
        // ---- 1. the weights
        double s = 0.0;
        for (int e = lane; e < k; e += 64) s += ww[e];
        const double sw = jch_wave_sum(s);                     // (the same bits in every wave)
        for (int e = tid; e < k; e += 256) {
            const int r = ii[e];
            rows[e] = (r >= 0 && (int64_t)r < g.n) ? r : -1;
            const double wn = ww[e] / sw;
            wt[e] = wn;
            sq[e] = sqrt(wn);
        }
        slab_bsync<LDS>();
        // ---- 2. the gather: G lanes per row, 4 * per rows at a time
        for (int j = wv * per + sub; j < k; j += 4 * per) {
            const int r = rows[j];
            const double *src = g.XY + (size_t)(r < 0 ? 0 : r) * (size_t)g.ldr;
            for (int c = c0; c < nc; c += G) S[(size_t)c * L + j] = r >= 0 ? src[c] : nan;
        }
        slab_bsync<LDS>();
        // ---- 3. the shortcuts (block-uniform)
        if (q == 1) {                                          // src/locw.jl:33-34
            const double *yc = S + (size_t)d * L;
            const double y0 = yc[0];
            int differs = 0;
            for (int e = tid; e < k; e += 256) differs |= (yc[e] != y0) ? 1 : 0;   // (a NaN differs from itself: no shortcut)
            const int wave_differs = __any(differs);
            if (lane == 0) s_any[wv] = wave_differs;
            __syncthreads();
            if (!(s_any[0] | s_any[1] | s_any[2] | s_any[3])) {
                if (tid == 0) { g.pred[qi] = y0; if (g.info) g.info[qi] = 2; }
                continue;
            }
        }
        if (k <= d) { fail_row(qi, 1); continue; }             // a centred k-row slab has rank <= k - 1 < d
        // ---- 4. weighted means, centring, sqrt(w~): the columns round-robin over the waves
        for (int c = wv; c < nc; c += 4) {
            double *col = S + (size_t)c * L;
            double a = 0.0;
            for (int i = lane; i < k; i += 64) a += wt[i] * col[i];
            const double mu = jch_wave_sum(a);
            for (int i = lane; i < k; i += 64) col[i] = sq[i] * (col[i] - mu);
            if (lane == 0) {
                mean[c] = mu;
                if (c < d) dx[c] = g.Xq[(size_t)qi + (size_t)c * (size_t)g.ldq] - mu;
            }
        }
        slab_bsync<LDS>();
        // ---- 5. Householder QR of A, applied to the columns behind it and to B
        double rmax = 0.0, rmin = __builtin_inf();
        for (int j = 0; j < d; ++j) {
            const double *vj = S + (size_t)j * L;
            double a = 0.0;
            for (int i = j + lane; i < k; i += 64) { const double x = vj[i]; a += x * x; }
            const double sig = jch_wave_sum(a);                // (the same bits in every wave)
            const double x1 = vj[j], nrm = sqrt(sig);
            const double alpha = x1 > 0.0 ? -nrm : nrm;
            const double v1 = x1 - alpha;
            rmax = fmax(rmax, nrm); rmin = fmin(rmin, nrm);    // (a NaN is neither: it is no rank deficiency, it reaches pred by the arithmetic)
            if (tid == 0) rd[j] = alpha;
            if (!(sig == 0.0)) {                               // (a zero column: H = I, r_jj = 0 and the rank test below fails the query)
                const double bh = 1.0 / (nrm * (nrm + fabs(x1)));   // 2 / v'v
                for (int c = j + 1 + wv; c < nc; c += 4) {
                    double *col = S + (size_t)c * L;
                    double t = 0.0;
                    for (int i = j + lane; i < k; i += 64) t += (i == j ? v1 : vj[i]) * col[i];
                    const double f = jch_wave_sum(t) * bh;
                    for (int i = j + lane; i < k; i += 64) col[i] -= f * (i == j ? v1 : vj[i]);
                }
            }
            slab_bsync<LDS>();
        }
        // ---- 6. the rank test, then per response one wave: back substitution and the prediction
        if (rmin <= (double)min(k, d) * 0x1p-52 * rmax) { fail_row(qi, 1); continue; }
        for (int c = wv; c < q; c += 4) {
            double *b = S + (size_t)(d + c) * L;
            double acc = 0.0;
            for (int j = d - 1; j >= 0; --j) {
                const double bj = b[j] / rd[j];
                acc += dx[j] * bj;
                const double *rj = S + (size_t)j * L;
                for (int i = lane; i < j; i += 64) b[i] -= rj[i] * bj;
                slab_wsync<LDS>();
            }
            if (lane == 0) g.pred[(size_t)qi + (size_t)c * (size_t)g.m] = mean[d + c] + acc;
        }
        if (tid == 0 && g.info) g.info[qi] = 0;
    }
}


extern "C" int32_t jch_knn_wls(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t d, int64_t ldx, const double *Y, int64_t q, int64_t ldy,
                               const double *Xq, int64_t m, int64_t ldq, const int32_t *ind, const double *w, int32_t k, double *pred, int32_t *info)
{
    if (!ctx) return JCH_EINVAL;
    if (!X || !Y || !Xq || !ind || !w || !pred || n < 1 || m < 1 || k < 1 || d < 1 || q < 1 || n >= ((int64_t)1 << 31) - 1 || m >= ((int64_t)1 << 31) - 1 ||
        k >= ((int32_t)1 << 30) || d > (1 << 20) || q > (1 << 20) || (size_t)m * (size_t)k >= ((size_t)1 << 40) || ldx < n || ldy < n || ldq < m)
        return jch_fail(ctx, JCH_EINVAL, "jch_knn_wls: bad arguments");
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "jch_knn_wls: bad loc");
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t mk = (size_t)m * k, nc = (size_t)(d + q);
    const bool host = loc == JCH_LOC_HOST;
    const size_t slab = wls_slab_doubles(k, d, q);
    const jch_slab_where at = jch_slab_plan(ctx, m, slab, WLS_LDS_MAX, false);
    jch_carve cv;
    const size_t o_x = host ? cv.take((size_t)n * d) : 0, o_y = host ? cv.take((size_t)n * q) : 0, o_q = host ? cv.take((size_t)m * d) : 0;
    const size_t o_i = host ? cv.take(jch_ints_as_doubles(mk)) : 0, o_w = host ? cv.take(mk) : 0, o_p = host ? cv.take((size_t)m * q) : 0;
    const size_t o_f = (host && info) ? cv.take(jch_ints_as_doubles((size_t)m)) : 0;
    const size_t o_xy = cv.take((size_t)n * nc), o_sc = at.glob ? cv.take((size_t)at.nb * slab) : 0;
    JCH_TRY(jch_reserve(ctx, ctx->kn_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->kn_ws.ptr;
    return jch_synced(ctx, host, [&]() -> int32_t {
        const double *dX = X, *dY = Y, *dQ = Xq, *dw = w;
        const int *di = ind;
        double *dp = pred;
        int *df = info;
        int64_t ldxd = ldx, ldyd = ldy, ldqd = ldq;
        JCH_TRY(jch_stage_in(ctx, host, ws + o_x, n, d, &dX, &ldxd));
        JCH_TRY(jch_stage_in(ctx, host, ws + o_y, n, q, &dY, &ldyd));
        JCH_TRY(jch_stage_in(ctx, host, ws + o_q, m, d, &dQ, &ldqd));
        if (host) {
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_i, ind, sizeof(int) * mk, hipMemcpyHostToDevice, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_w, w, sizeof(double) * mk, hipMemcpyHostToDevice, ctx->stream));
            di = (const int *)(ws + o_i); dw = ws + o_w; dp = ws + o_p; df = info ? (int *)(ws + o_f) : nullptr;
        }
        const unsigned tb = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 63) / 64, (int64_t)ctx->cus * 8));
        hipLaunchKernelGGL(k_wls_rowmajor, dim3(tb), dim3(256), 0, ctx->stream, dX, ldxd, dY, ldyd, n, (int)d, (int)q, ws + o_xy);
        JCH_HIP(ctx, hipGetLastError());
        wls_args a;
        a.XY = ws + o_xy; a.n = n; a.ldr = (int)nc; a.Xq = dQ; a.ldq = ldqd; a.ind = di; a.w = dw;
        a.m = (int)m; a.k = k; a.d = (int)d; a.q = (int)q; a.L = k | 1;
        a.gshift = 0;
        while (a.gshift < 6 && ((size_t)1 << a.gshift) < nc) ++a.gshift;
        a.pred = dp; a.info = df;
        a.scratch = at.glob ? ws + o_sc : nullptr; a.per_block = slab;
        JCH_TRY((jch_launch_slab<k_knn_wls<true>, k_knn_wls<false>>(ctx, at, slab, WLS_LDS_MAX, a)));
        if (host) {
            JCH_HIP(ctx, hipMemcpyAsync(pred, dp, sizeof(double) * (size_t)m * q, hipMemcpyDeviceToHost, ctx->stream));
            if (info) JCH_HIP(ctx, hipMemcpyAsync(info, df, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        }
        return JCH_OK;
    });
}
