// Spatial median of the rows of a column-major matrix (src/colmedspa.jl:4-33): jch_weiszfeld_step, jch_spatial_median — include/jchemo_hip.h;
// DESIGN.md §28.  jch_pcasph_fit (xtdx.hip) centres on it and takes its distances-only mode for the row norms.
//
// One Weiszfeld step from the centre c (:15-30):  d_i = |x_i - c|,  w0 = median(d),  ep = delta w0,  u_i = ep when d_i <= ep, else 1 / d_i,
// mu = sum_i u_i x_i / sum_i u_i,  h = |mu - c|.  The reference reads X three times per step through three n x p temporaries; the route over
// jch_row_resid_ss and jch_covsel_pass reads it twice.  k_ms_pass reads it ONCE:
//
//   k_ms_pass    A workgroup of MS_WAVES waves owns consecutive tiles of MS_ROWS = 64 rows, one lane per row, so that every column access of a wave
//                is one 512-byte run.  The waves split the columns: wave w holds columns [MS_CPW w, MS_CPW (w + 1)) of the tile in registers, forms
//                its part of sum_j (x_ij - c_j)^2 (the difference first, then the square: never an expanded form), and the parts meet in LDS at one
//                barrier per tile, added in wave order.  Every wave then scales its held values by u_i = 1 / d_i and folds them over the 64 rows with
//                a transposing butterfly (MS_CPW - 1 cross-lane exchanges for MS_CPW columns, a fixed tree): lane l ends with the tile's sum of
//                column l of the wave, which goes into ONE accumulator per lane that lives across all tiles of the workgroup.  After the last tile:
//                one partial row per workgroup, and the workgroup's sum of u.  No atomics.
//                p > MS_WAVES MS_CPW (WIDE): the columns are walked in chunks of MS_WAVES MS_CPW; the distance sweep keeps the last chunk, a second
//                sweep over the same tile (out of the caches, ordinary loads) folds the chunks one by one into the workgroup's own partial row in
//                global memory.  Slower, any p.
//   the clamp    u_i = ep needs the median of ALL distances.  The pass takes an upper bound tau >= ep instead, leaves every row with d_i <= tau out
//                of its sums (and counts them per workgroup), and writes d.  After the median, k_ms_finish walks the workgroups that left rows out in
//                ascending row order and adds u_i x_i with the true u_i: nothing is subtracted back.  In the loop tau = delta (w0_prev + h_prev)
//                (1 + 2^-40) (the triangle inequality: median(d_new) <= median(d_prev) + h_prev); the first step has no previous median and runs
//                the distances alone first (one more read), then the pass with tau = ep.
//   k_ms_finish  one workgroup: partial rows added in workgroup order, the left-out rows, mu = S / sum u, h, the next tau.
// Rows >= n and columns >= p are never read, X is never written, row numbers are 64-bit.  Every sum has a fixed order that does not depend on where
// X lives or how it is aligned (8-byte loads only): two runs give identical bits.  A NaN in X makes its row's distance NaN, hence the median, hence
// mu and h (:18; the loop then ends after that step, as in the reference).
// gfx950, hipcc -O3, scratch 0 throughout: k_ms_pass 170 VGPRs (step) and 148 (distances only), the wide instances 168 and 149, 8 KB of LDS: one
// workgroup of 8 waves per CU at 2 waves per SIMD; k_ms_finish 28 VGPRs.
#include <math.h>

#include <algorithm>

#include "jch_internal.h"

#define MS_ROWS 64     // rows per tile: one lane per row
#define MS_WAVES 8     // waves per workgroup: they split the columns of a chunk
#define MS_CPW 64      // columns a wave holds in registers
#define MS_TILES 4     // tiles per workgroup, at least (more when the grid would exceed one workgroup per CU)
#define MS_NT (64 * MS_WAVES)
#define MS_CHUNK (MS_WAVES * MS_CPW)   // widest shape of the register path
#define MS_FNT 256

static_assert(MS_ROWS == 64 && MS_CPW == 64, "the butterfly folds 64 columns over the 64 lanes of a wave");

// STEP: false = distances only.  part [grid][ldp], su [2 grid]: sum of u, rows left out.
template <bool STEP, bool WIDE>
__global__ __launch_bounds__(MS_NT) void k_ms_pass(const double *__restrict__ X, int64_t n, int p, int64_t ldx, const double *__restrict__ c,
                                                   const double *__restrict__ sdiv, const double *__restrict__ tau_dev, int64_t tpw,
                                                   double *__restrict__ d, double *__restrict__ part, int ldp, double *__restrict__ su)
{
    __shared__ double ssp[2][MS_WAVES][MS_ROWS];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nchunk = WIDE ? (p + MS_CHUNK - 1) / MS_CHUNK : 1;
    const int64_t ntile = (n + MS_ROWS - 1) / MS_ROWS;
    const int64_t t0 = (int64_t)blockIdx.x * tpw, t1 = std::min<int64_t>(ntile, t0 + tpw);
    const double tau = STEP ? *tau_dev : 0.0;
    double v[MS_CPW];
    double acc = 0.0, usum = 0.0, left = 0.0;
    double *mypart = STEP ? part + (size_t)blockIdx.x * (size_t)ldp : nullptr;
    int buf = 0;
    for (int64_t t = t0; t < t1; ++t, buf ^= 1) {
        const int64_t r = t * MS_ROWS + lane;
        const bool live = r < n;
        auto fetch = [&](int c0) {
            const double *x = X + (size_t)c0 * (size_t)ldx + (size_t)(live ? r : 0);
#pragma unroll
            for (int k = 0; k < MS_CPW; ++k) {
                v[k] = 0.0;
                if (c0 + k < p && live) v[k] = WIDE ? x[(size_t)k * (size_t)ldx] : __builtin_nontemporal_load(x + (size_t)k * (size_t)ldx);
            }
        };
        double ss = 0.0;
        for (int ch = 0; ch < nchunk; ++ch) {
            const int c0 = ch * MS_CHUNK + wv * MS_CPW;
            fetch(c0);
#pragma unroll
            for (int k = 0; k < MS_CPW; ++k)
                if (c0 + k < p) {
                    double e = v[k] - c[c0 + k];
                    if (sdiv) e /= sdiv[c0 + k];
                    ss = fma(e, e, ss);
                }
        }
        ssp[buf][wv][lane] = ss;
        __syncthreads();   // (the one barrier of a tile: the other buffer's last readers passed it one tile ago)
        double dsq = 0.0;
#pragma unroll
        for (int w = 0; w < MS_WAVES; ++w) dsq += ssp[buf][w][lane];
        const double di = sqrt(dsq);
        if (wv == 0 && live) d[r] = di;
        if (!STEP) continue;
        const bool out = di <= tau;
        const double u = live ? (out ? 0.0 : 1.0 / di) : 0.0;
        usum += u;
        left += (live && out) ? 1.0 : 0.0;
        for (int ch = nchunk - 1; ch >= 0; --ch) {
            const int c0 = ch * MS_CHUNK + wv * MS_CPW;
            if (ch != nchunk - 1) fetch(c0);
#pragma unroll
            for (int k = 0; k < MS_CPW; ++k) v[k] *= u;
            // fold the 64 rows: after the step with offset o lane l holds the sums over its pair of the columns whose bit o equals l's
#pragma unroll
            for (int m = MS_CPW; m > 1; m >>= 1) {
                const int o = m >> 1;
                const bool up = (lane & o) != 0;
#pragma unroll
                for (int i = 0; i < o; ++i) {
                    const double a = v[i], b = v[i + o];
                    const double send = up ? a : b, keep = up ? b : a;
                    v[i] = keep + __shfl_xor(send, o, 64);
                }
            }
            if (WIDE) {
                double *dst = mypart + ch * MS_CHUNK + wv * MS_CPW + lane;
                *dst = (t == t0 ? 0.0 : *dst) + v[0];
            } else {
                acc += v[0];
            }
        }
    }
    if (!STEP) return;
    if (!WIDE) mypart[wv * MS_CPW + lane] = acc;
    if (wv == 0) {
        usum = jch_wave_sum(usum);
        left = jch_wave_sum(left);
        if (lane == 0) { su[2 * blockIdx.x] = usum; su[2 * blockIdx.x + 1] = left; }
    }
}

// *tau = v (w0 null) or delta * *w0
__global__ void k_ms_settau(double *tau, double v, double delta, const double *w0)
{
    *tau = w0 ? delta * *w0 : v;
}

// out: [0] w0, [1] h, [2] rows left out, [3] 1 when tau < ep (nothing else is written then), [4] the next step's tau.  tau lives in out[4].
__global__ __launch_bounds__(MS_FNT) void k_ms_finish(const double *__restrict__ X, int64_t n, int p, int64_t ldx, const double *__restrict__ c,
                                                      const double *__restrict__ d, const double *__restrict__ part, int ldp,
                                                      const double *__restrict__ su, int nwg, int64_t tpw, const double *__restrict__ w0_dev, double delta,
                                                      double *__restrict__ mu, double *__restrict__ out)
{
    __shared__ double scr[MS_FNT / 64];
    const double w0 = *w0_dev, ep = delta * w0, tau = out[4];
    if (tau < ep) {   // (uniform) the guard was no upper bound of ep
        if (threadIdx.x == 0) { out[0] = w0; out[3] = 1.0; }
        return;
    }
    double hh = 0.0, nleft = 0.0;
    for (int j0 = 0; j0 < p; j0 += MS_FNT) {   // (uniform trip count: the barriers below are reached by all)
        const int j = j0 + threadIdx.x;
        const bool col = j < p;
        double S = 0.0, us = 0.0, nl = 0.0;
        for (int g = 0; g < nwg; ++g) {
            if (col) S += part[(size_t)g * (size_t)ldp + j];
            us += su[2 * g];
        }
        for (int g = 0; g < nwg; ++g) {
            if (su[2 * g + 1] == 0.0) continue;
            const int64_t r0 = (int64_t)g * tpw * MS_ROWS, r1 = std::min<int64_t>(n, r0 + tpw * MS_ROWS);
            for (int64_t r = r0; r < r1; ++r) {
                const double di = d[r];
                if (!(di <= tau)) continue;
                const double u = di <= ep ? ep : 1.0 / di;
                if (col) S += u * X[(size_t)r + (size_t)j * (size_t)ldx];
                us += u;
                nl += 1.0;
            }
        }
        if (col) {
            const double m = S / us;
            mu[j] = m;
            const double e = m - c[j];
            hh = fma(e, e, hh);
        }
        nleft = nl;
    }
    hh = jch_block_sum<MS_FNT>(hh, scr);
    if (threadIdx.x == 0) {
        const double h = sqrt(hh);
        out[0] = w0; out[1] = h; out[2] = nleft; out[3] = 0.0;
        out[4] = delta * (w0 + h) * (1.0 + 0x1p-40);
    }
}

namespace {

struct ms_plan {
    int nwg = 1, ldp = MS_CHUNK;
    int64_t tpw = MS_TILES;
    bool wide = false;
};

ms_plan ms_make_plan(const jch_ctx *ctx, int64_t n, int64_t p)
{
    ms_plan pl;
    const int64_t ntile = (n + MS_ROWS - 1) / MS_ROWS;
    pl.tpw = std::max<int64_t>(MS_TILES, (ntile + ctx->cus - 1) / ctx->cus);
    pl.nwg = (int)((ntile + pl.tpw - 1) / pl.tpw);
    pl.wide = p > MS_CHUNK;
    pl.ldp = (int)((p + MS_CHUNK - 1) / MS_CHUNK) * MS_CHUNK;
    return pl;
}

// the device state of a call: everything lives in ctx->ms_ws
struct ms_state {
    ms_plan pl;
    double *d = nullptr, *mua = nullptr, *mub = nullptr, *part = nullptr, *su = nullptr, *out = nullptr, *w0 = nullptr, *xs = nullptr;
};

int32_t ms_reserve(jch_ctx *ctx, int64_t n, int64_t p, bool stage_x, ms_state *st)
{
    st->pl = ms_make_plan(ctx, n, p);
    jch_carve cv;
    const size_t od = cv.take((size_t)n), oa = cv.take((size_t)p), ob = cv.take((size_t)p), op = cv.take((size_t)st->pl.nwg * st->pl.ldp),
                 os = cv.take(2 * (size_t)st->pl.nwg), oo = cv.take(8), ow = cv.take(8), ox = cv.take(stage_x ? (size_t)n * (size_t)p : 0);
    JCH_TRY(jch_reserve(ctx, ctx->ms_ws, sizeof(double) * cv.off));
    JCH_TRY(jch_colselect_reserve(ctx, p));
    double *ws = (double *)ctx->ms_ws.ptr;
    st->d = ws + od; st->mua = ws + oa; st->mub = ws + ob; st->part = ws + op; st->su = ws + os; st->out = ws + oo; st->w0 = ws + ow; st->xs = ws + ox;
    return JCH_OK;
}

template <bool STEP>
void ms_launch_pass(jch_ctx *ctx, const ms_plan &pl, const double *X, int64_t n, int p, int64_t ldx, const double *c, const double *sdiv, const double *tau,
                    double *d, double *part, double *su)
{
    if (pl.wide) hipLaunchKernelGGL((k_ms_pass<STEP, true>), dim3(pl.nwg), dim3(MS_NT), 0, ctx->stream, X, n, p, ldx, c, sdiv, tau, pl.tpw, d, part, pl.ldp, su);
    else hipLaunchKernelGGL((k_ms_pass<STEP, false>), dim3(pl.nwg), dim3(MS_NT), 0, ctx->stream, X, n, p, ldx, c, sdiv, tau, pl.tpw, d, part, pl.ldp, su);
}

// One step from the device centre c into the device centre mu, enqueued only.  guard < 0: the distances first, then the pass with tau = ep.
// known_w0: st->w0 and d already belong to c (a guarded step that has to be redone exactly).
int32_t ms_step(jch_ctx *ctx, const ms_state &st, const double *X, int64_t n, int p, int64_t ldx, const double *c, double delta, bool exact, double guard,
                bool guard_on_dev, bool known_w0, double *d, double *mu)
{
    double *tau = st.out + 4;
    if (exact) {
        if (!known_w0) {
            ms_launch_pass<false>(ctx, st.pl, X, n, p, ldx, c, nullptr, nullptr, d, nullptr, nullptr);
            JCH_TRY(jch_launch_col_median_mad(ctx, d, n, 1, n, st.w0, nullptr));
        }
        hipLaunchKernelGGL(k_ms_settau, dim3(1), dim3(1), 0, ctx->stream, tau, 0.0, delta, (const double *)st.w0);
        ms_launch_pass<true>(ctx, st.pl, X, n, p, ldx, c, nullptr, tau, d, st.part, st.su);
    } else {
        if (!guard_on_dev) hipLaunchKernelGGL(k_ms_settau, dim3(1), dim3(1), 0, ctx->stream, tau, guard, 0.0, (const double *)nullptr);
        ms_launch_pass<true>(ctx, st.pl, X, n, p, ldx, c, nullptr, tau, d, st.part, st.su);
        JCH_TRY(jch_launch_col_median_mad(ctx, d, n, 1, n, st.w0, nullptr));
    }
    hipLaunchKernelGGL(k_ms_finish, dim3(1), dim3(MS_FNT), 0, ctx->stream, X, n, p, ldx, c, (const double *)d, (const double *)st.part, st.pl.ldp,
                       (const double *)st.su, st.pl.nwg, st.pl.tpw, (const double *)st.w0, delta, mu, st.out);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

int32_t ms_check(jch_ctx *ctx, const char *who, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, double delta)
{
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (!X || n < 1 || p < 1 || p > (1 << 30) || ldx < n) return jch_fail(ctx, JCH_EINVAL, "%s: bad X (n=%lld p=%lld ldx=%lld)", who, (long long)n, (long long)p, (long long)ldx);
    if (!(delta > 0.0)) return jch_fail(ctx, JCH_EINVAL, "%s: delta must be > 0", who);
    if (ctx->nranks > 1) return jch_fail(ctx, JCH_EINVAL, "%s: one rank only (communicator of %d)", who, ctx->nranks);
    return JCH_OK;
}

}  // namespace

int32_t jch_launch_weiszfeld_dist(jch_ctx *ctx, const double *X, int64_t n, int p, int64_t ldx, const double *c, const double *sdiv, double *d)
{
    const ms_plan pl = ms_make_plan(ctx, n, p);
    ms_launch_pass<false>(ctx, pl, X, n, p, ldx, c, sdiv, nullptr, d, nullptr, nullptr);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

// The whole loop on a device X (src/colmedspa.jl:8-32).  mu_dev: the result (device, p).  d_dev (device, n) or null.  Reads one scalar record per step.
int32_t jch_spatial_median_dev(jch_ctx *ctx, const double *X, int64_t n, int p, int64_t ldx, double delta, int maxit, double *mu_dev, double *d_dev, int32_t *niter,
                               double *h_last, int32_t *converged)
{
    ms_state st;
    JCH_TRY(ms_reserve(ctx, n, p, false, &st));
    double *d = d_dev ? d_dev : st.d;
    const double delta1 = delta * sqrt((double)p);   // :7
    JCH_TRY(jch_launch_col_median_mad(ctx, X, n, p, ldx, st.mua, nullptr));   // :8
    double *cur = st.mua, *nxt = st.mub;
    double rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int it = 0;
    bool conv = false;
    while (it < maxit) {
        JCH_TRY(ms_step(ctx, st, X, n, p, ldx, cur, delta, it == 0, 0.0, true, false, d, nxt));
        JCH_HIP(ctx, hipMemcpyAsync(rec, st.out, sizeof(double) * 5, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (rec[3] != 0.0) {   // the guard fell below ep (rounding at the edge of the triangle inequality): the same step with the exact clamp
            JCH_TRY(ms_step(ctx, st, X, n, p, ldx, cur, delta, true, 0.0, true, true, d, nxt));
            JCH_HIP(ctx, hipMemcpyAsync(rec, st.out, sizeof(double) * 5, hipMemcpyDeviceToHost, ctx->stream));
            JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        ++it;
        std::swap(cur, nxt);
        if (!(rec[1] > delta1)) { conv = true; break; }   // :14 (a NaN h ends the loop)
    }
    JCH_HIP(ctx, hipMemcpyAsync(mu_dev, cur, sizeof(double) * (size_t)p, hipMemcpyDeviceToDevice, ctx->stream));
    if (niter) *niter = it;
    if (h_last) *h_last = rec[1];
    if (converged) *converged = conv ? 1 : 0;
    return JCH_OK;
}

extern "C" int32_t jch_weiszfeld_step(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *mu0, double delta,
                                      double guard, double *mu, double *d, double *w0, double *h, int64_t *nleft)
{
    static const char *who = "jch_weiszfeld_step";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(ms_check(ctx, who, loc, X, n, p, ldx, delta));
    if (!mu0 || !mu) return jch_fail(ctx, JCH_EINVAL, "%s: mu0 and mu are required", who);
    if (guard != guard) return jch_fail(ctx, JCH_EINVAL, "%s: guard is NaN", who);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST;
    ms_state st;
    JCH_TRY(ms_reserve(ctx, n, p, host, &st));
    double rec[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        const double *dX = X;
        int64_t ldxd = ldx;
        JCH_TRY(jch_stage_in(ctx, host, st.xs, n, p, &dX, &ldxd));
        JCH_HIP(ctx, hipMemcpyAsync(st.mua, mu0, sizeof(double) * (size_t)p, hipMemcpyHostToDevice, ctx->stream));
        double *dd = (host || !d) ? st.d : d;
        JCH_TRY(ms_step(ctx, st, dX, n, (int)p, ldxd, st.mua, delta, guard < 0.0, guard, false, false, dd, st.mub));
        JCH_HIP(ctx, hipMemcpyAsync(rec, st.out, sizeof(double) * 5, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (rec[3] != 0.0) return JCH_OK;   // (reported below, nothing else is copied out)
        JCH_HIP(ctx, hipMemcpyAsync(mu, st.mub, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, ctx->stream));
        if (host && d) JCH_HIP(ctx, hipMemcpyAsync(d, dd, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    }));
    if (rec[3] != 0.0) return jch_fail(ctx, JCH_EINVAL, "%s: guard = %g is below this step's ep = delta * w0 = %g", who, guard, delta * rec[0]);
    if (w0) *w0 = rec[0];
    if (h) *h = rec[1];
    if (nleft) *nleft = (int64_t)rec[2];
    return JCH_OK;
}

extern "C" int32_t jch_spatial_median(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, double delta, int32_t maxit, double *mu,
                                      double *d, int32_t *niter, double *h_last, int32_t *converged)
{
    static const char *who = "jch_spatial_median";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(ms_check(ctx, who, loc, X, n, p, ldx, delta));
    if (!mu) return jch_fail(ctx, JCH_EINVAL, "%s: mu is required", who);
    if (maxit < 1) return jch_fail(ctx, JCH_EINVAL, "%s: maxit = %d must be >= 1", who, maxit);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST;
    ms_state st;
    JCH_TRY(ms_reserve(ctx, n, p, host, &st));
    JCH_TRY(jch_reserve(ctx, ctx->sel_out, sizeof(double) * (size_t)p));
    double *mud = (double *)ctx->sel_out.ptr;
    return jch_synced(ctx, true, [&]() -> int32_t {
        const double *dX = X;
        int64_t ldxd = ldx;
        JCH_TRY(jch_stage_in(ctx, host, st.xs, n, p, &dX, &ldxd));
        double *dd = (host || !d) ? st.d : d;
        JCH_TRY(jch_spatial_median_dev(ctx, dX, n, (int)p, ldxd, delta, maxit, mud, dd, niter, h_last, converged));
        JCH_HIP(ctx, hipMemcpyAsync(mu, mud, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, ctx->stream));
        if (host && d) JCH_HIP(ctx, hipMemcpyAsync(d, dd, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    });
}
