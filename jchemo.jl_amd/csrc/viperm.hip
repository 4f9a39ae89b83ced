// Permutation importance (src/viperm.jl:89-107): jch_perm_fill, jch_perm_score_sums — include/jchemo_hip.h; DESIGN.md §26.
//
// The reference copies the held-out block, shuffles one column, predicts and scores, p times per replication.  For a model that predicts as
// int + X B, shuffling column j changes the prediction of row i by (x[pi_j(i), j] - x[i, j]) B[j, :], so the six score sums of all p shuffled
// predictions come from one read of the held-out rows of X, given the unshuffled predictions.  The residual is formed per element
// (e = y - (pred + d B[j, k]), never expanded into cross-products) and the row of sums behind the last column is the same code with d = 0.
//
// The permutations are counter-based: pi_j(i) is a balanced Feistel network over b bits (b = the smallest even number with 2^b >= m), walked
// until it lands in [0, m).  Nothing of size m x p is stored unless the caller hands its own permutations in.
#include <algorithm>
#include <vector>

#include "jch_internal.h"

#define VP_NT 256
#define VP_RPT 8                      // rows per thread, VP_NT apart: a wave reads 64 consecutive entries of `rows`
#define VP_SLICE (VP_NT * VP_RPT)     // rows per work item (jchemo_hip.viperm.PERM_SLICE_ROWS)
#define VP_QG 4                       // response columns whose 6 sums a thread holds in registers at a time
#define VP_XCDS 8                     // workgroups go to the XCDs round-robin by their linear index

// ---- the generator (the definition is in include/jchemo_hip.h) ----------------------------------------------------------------------
#define VP_GOLDEN 0x9E3779B97F4A7C15ULL
__host__ __device__ __forceinline__ uint64_t vp_mix64(uint64_t z)   // the splitmix64 finaliser (util.hip)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t vp_key(uint64_t seed, uint64_t j) { return vp_mix64(seed + (j + 1) * VP_GOLDEN); }
static int vp_bits(int64_t m)
{
    int b = 2;
    while (((int64_t)1 << b) < m) b += 2;
    return b;
}
static int vp_rounds(int b) { return b <= 12 ? 24 : 8; }
__host__ __device__ __forceinline__ uint32_t vp_perm(uint64_t key, int half, int rounds, uint32_t m, uint32_t i)
{
    const uint32_t mask = (1u << half) - 1u;
    uint32_t v = i;
    do {   // (a permutation of [0, 2^b) walked from a point of [0, m) comes back into [0, m))
        uint32_t L = v >> half, R = v & mask;
        uint64_t rk = key;
        for (int r = 0; r < rounds; ++r) {
            rk += VP_GOLDEN;
            const uint32_t f = (uint32_t)(vp_mix64(rk ^ (uint64_t)R) >> (64 - half));
            const uint32_t t = L ^ f;
            L = R;
            R = t;
        }
        v = (L << half) | R;
    } while (v >= m);
    return v;
}

__global__ __launch_bounds__(VP_NT) void k_vp_fill(int32_t *__restrict__ perm, int64_t m, int64_t ncols, int64_t ldperm, uint64_t seed, int half, int rounds)
{
    const int64_t total = m * ncols;
    for (int64_t e = (int64_t)blockIdx.x * VP_NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * VP_NT) {
        const int64_t j = e / m, i = e - j * m;
        perm[(size_t)i + (size_t)j * (size_t)ldperm] = (int32_t)vp_perm(vp_key(seed, (uint64_t)j), half, rounds, (uint32_t)m, (uint32_t)i);
    }
}

// ---- the pass -------------------------------------------------------------------------------------------------------------------------
// Work item = (column j <= p, slice s of VP_SLICE held-out rows); j == p is the unshuffled row of sums (d = 0, B = 0).  Linear workgroup index
// w: XCD x = w % 8 runs the columns j = x, x + 8, ... one after the other and the slices of a column back to back, so a column is gathered by
// one XCD within a short stretch of time and sits in that XCD's L2 (or, beyond 4 MiB, in the Infinity Cache) while it is.
// The lane for held-out row i reads x[r_i, j] (ascending `rows`: near-coalesced) and x[r_pi(i), j] (the gather).  An index outside its range
// is never followed: the lane reads row 0 (or takes pi = i) instead and raises *flag, which the host turns into JCH_EINVAL.
// part [(j nslice + s) q + k][6]: the block's sums, each a fixed tree over fixed per-thread chains.
template <bool GEN>
__global__ __launch_bounds__(VP_NT) void k_vp_pass(const double *__restrict__ X, int64_t n, int p, int64_t ldx, const int64_t *__restrict__ rows, int64_t m,
                                                   const double *__restrict__ Pred, int64_t ldp, const double *__restrict__ Y, int64_t ldy, int q,
                                                   const double *__restrict__ B, const int32_t *__restrict__ perm, int64_t ldperm, uint64_t seed, int half,
                                                   int rounds, int nslice, double *__restrict__ part, int *__restrict__ flag)
{
    __shared__ double red[VP_NT / 64];
    const int xcd = blockIdx.x % VP_XCDS;
    const int64_t w = blockIdx.x / VP_XCDS;
    const int64_t jw = w / nslice * VP_XCDS + xcd;
    const int s = (int)(w % nslice);
    if (jw > p) return;   // (block-uniform)
    const int j = (int)jw;
    const bool ref = j == p;
    const int64_t i0 = (int64_t)s * VP_SLICE + threadIdx.x;
    const double *xj = X + (size_t)(ref ? 0 : j) * (size_t)ldx;
    const uint64_t key = vp_key(seed, (uint64_t)j);
    double d[VP_RPT];
    int64_t r[VP_RPT];
    bool bad = false;
#pragma unroll
    for (int u = 0; u < VP_RPT; ++u) {
        const int64_t i = i0 + (int64_t)VP_NT * u;
        d[u] = 0.0;
        r[u] = 0;
        if (i < m) {
            int64_t ri = rows ? rows[i] : i;
            if ((uint64_t)ri >= (uint64_t)n) { bad = true; ri = 0; }
            r[u] = ri;
            if (!ref) {
                int64_t pi = GEN ? (int64_t)vp_perm(key, half, rounds, (uint32_t)m, (uint32_t)i) : (int64_t)perm[(size_t)i + (size_t)j * (size_t)ldperm];
                if ((uint64_t)pi >= (uint64_t)m) { bad = true; pi = i; }
                int64_t rp = rows ? rows[pi] : pi;
                if ((uint64_t)rp >= (uint64_t)n) { bad = true; rp = 0; }
                d[u] = xj[rp] - xj[ri];
            }
        }
    }
    if (bad) *flag = 1;
    for (int k0 = 0; k0 < q; k0 += VP_QG) {
        double acc[VP_QG][6], b[VP_QG];
#pragma unroll
        for (int g = 0; g < VP_QG; ++g) {
            b[g] = (!ref && k0 + g < q) ? B[(size_t)j + (size_t)(k0 + g) * (size_t)p] : 0.0;
#pragma unroll
            for (int t = 0; t < 6; ++t) acc[g][t] = 0.0;
        }
#pragma unroll
        for (int u = 0; u < VP_RPT; ++u) {
            if (i0 + (int64_t)VP_NT * u < m) {
#pragma unroll
                for (int g = 0; g < VP_QG; ++g) {
                    if (k0 + g < q) {
                        const double y = Y[(size_t)r[u] + (size_t)(k0 + g) * (size_t)ldy];
                        const double pr = Pred[(size_t)r[u] + (size_t)(k0 + g) * (size_t)ldp];
                        const double e = y - (pr + d[u] * b[g]);
                        acc[g][0] += e; acc[g][1] += e * e; acc[g][2] += y * e; acc[g][3] += y; acc[g][4] += y * y; acc[g][5] += 1.0;
                    }
                }
            }
        }
#pragma unroll
        for (int g = 0; g < VP_QG; ++g) {
            if (k0 + g < q) {   // (block-uniform)
                double *out = part + (((size_t)j * (size_t)nslice + (size_t)s) * (size_t)q + (size_t)(k0 + g)) * 6;
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    const double v = jch_block_sum<VP_NT>(acc[g][t], red);
                    if (threadIdx.x == 0) out[t] = v;
                }
            }
        }
    }
}

// out[j][k][t] = the slices' partials added in slice order
__global__ __launch_bounds__(VP_NT) void k_vp_reduce(const double *__restrict__ part, int64_t ncol /*p + 1*/, int nslice, int q6, double *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * VP_NT + threadIdx.x;
    if (e >= ncol * q6) return;
    const int64_t j = e / q6, c = e - j * q6;
    const double *src = part + (size_t)j * (size_t)nslice * (size_t)q6 + (size_t)c;
    double sum = 0.0;
    for (int s = 0; s < nslice; ++s) sum += src[(size_t)s * (size_t)q6];
    out[e] = sum;
}

// ---- entries ------------------------------------------------------------------------------------------------------------------------
extern "C" int32_t jch_perm_fill(jch_ctx *ctx, int32_t loc, int32_t *perm, int64_t m, int64_t ncols, int64_t ldperm, uint64_t seed)
{
    static const char *who = "jch_perm_fill";
    if (!ctx) return JCH_EINVAL;
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (!perm || m < 1 || m >= ((int64_t)1 << 31) || ncols < 1 || ldperm < m)
        return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments (m=%lld ncols=%lld ldperm=%lld; 1 <= m < 2^31)", who, (long long)m, (long long)ncols, (long long)ldperm);
    if (ctx->nranks > 1) return jch_fail(ctx, JCH_EINVAL, "%s: one rank only (communicator of %d)", who, ctx->nranks);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST;
    const int b = vp_bits(m);
    int32_t *dperm = perm;
    int64_t ldd = ldperm;
    if (host) {
        JCH_TRY(jch_reserve(ctx, ctx->vp_ws, sizeof(int32_t) * (size_t)m * (size_t)ncols));
        dperm = (int32_t *)ctx->vp_ws.ptr;
        ldd = m;
    }
    return jch_synced(ctx, true, [&]() -> int32_t {
        hipLaunchKernelGGL(k_vp_fill, dim3(jch_grid1(ctx, m * ncols)), dim3(VP_NT), 0, ctx->stream, dperm, m, ncols, ldd, seed, b / 2, vp_rounds(b));
        JCH_HIP(ctx, hipGetLastError());
        if (host)
            JCH_HIP(ctx, hipMemcpy2DAsync(perm, sizeof(int32_t) * (size_t)ldperm, dperm, sizeof(int32_t) * (size_t)m, sizeof(int32_t) * (size_t)m, (size_t)ncols,
                                          hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    });
}

extern "C" int32_t jch_perm_score_sums(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const int64_t *rows, int64_t m,
                                       const double *Pred, int64_t ldp, const double *Y, int64_t q, int64_t ldy, const double *B, int64_t ldb,
                                       const int32_t *perm, int64_t ldperm, uint64_t seed, double *sums)
{
    static const char *who = "jch_perm_score_sums";
    if (!ctx) return JCH_EINVAL;
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (!X || n < 1 || p < 1 || ldx < n) return jch_fail(ctx, JCH_EINVAL, "%s: bad X (n=%lld p=%lld ldx=%lld)", who, (long long)n, (long long)p, (long long)ldx);
    if (!Pred || !Y || q < 1 || ldp < n || ldy < n)
        return jch_fail(ctx, JCH_EINVAL, "%s: bad Pred / Y (q=%lld ldp=%lld ldy=%lld)", who, (long long)q, (long long)ldp, (long long)ldy);
    if (!B || ldb < p || !sums) return jch_fail(ctx, JCH_EINVAL, "%s: bad B (ldb=%lld) or sums", who, (long long)ldb);
    if (m < 1 || m >= ((int64_t)1 << 31) || (!rows && m > n)) return jch_fail(ctx, JCH_EINVAL, "%s: m=%lld (1 <= m < 2^31; m <= n without rows)", who, (long long)m);
    if (perm && ldperm < m) return jch_fail(ctx, JCH_EINVAL, "%s: ldperm=%lld < m", who, (long long)ldperm);
    const int64_t nslice = (m + VP_SLICE - 1) / VP_SLICE, ncolg = (p + 1 + VP_XCDS - 1) / VP_XCDS;
    if (q > (1 << 20) || (p + 1) * q > ((int64_t)1 << 27) || ncolg * VP_XCDS * nslice > (int64_t)INT32_MAX)
        return jch_fail(ctx, JCH_EINVAL, "%s: (p + 1) q = %lld x %lld beyond 2^27, or more than 2^31 work items", who, (long long)(p + 1), (long long)q);
    if (ctx->nranks > 1) return jch_fail(ctx, JCH_EINVAL, "%s: one rank only (communicator of %d)", who, ctx->nranks);
    const bool host = loc == JCH_LOC_HOST;
    if (host) {   // the index lists are here: an entry outside its range is refused before any device work
        if (rows)
            for (int64_t i = 0; i < m; ++i)
                if (rows[i] < 0 || rows[i] >= n) return jch_fail(ctx, JCH_EINVAL, "%s: rows[%lld] = %lld outside 0 .. n - 1", who, (long long)i, (long long)rows[i]);
        if (perm)
            for (int64_t j = 0; j < p; ++j)
                for (int64_t i = 0; i < m; ++i) {
                    const int32_t v = perm[(size_t)i + (size_t)j * (size_t)ldperm];
                    if (v < 0 || v >= m) return jch_fail(ctx, JCH_EINVAL, "%s: perm[%lld, %lld] = %d outside 0 .. m - 1", who, (long long)i, (long long)j, v);
                }
    }
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const int pi = (int)p, qi = (int)q, q6 = qi * 6;
    const size_t nout = (size_t)(p + 1) * (size_t)q6;
    jch_carve cv;
    const size_t oB = cv.take((size_t)p * qi), opart = cv.take(nout * (size_t)nslice), oout = cv.take(nout + 1 /*the range flag behind the sums*/),
                 oX = cv.take(host ? (size_t)n * (size_t)p : 0), oP = cv.take(host ? (size_t)n * qi : 0), oY = cv.take(host ? (size_t)n * qi : 0),
                 orows = cv.take(host && rows ? (size_t)m : 0), operm = cv.take(host && perm ? jch_ints_as_doubles((size_t)m * (size_t)p) : 0);
    JCH_TRY(jch_reserve(ctx, ctx->vp_ws, sizeof(double) * cv.off));
    JCH_TRY(jch_reserve_host(ctx, sizeof(double) * (nout + 1)));
    double *ws = (double *)ctx->vp_ws.ptr, *dB = ws + oB, *part = ws + opart, *out = ws + oout, *hs = (double *)ctx->hstage;
    int *flag = (int *)(out + nout);
    std::vector<double> hB((size_t)p * qi);
    for (int k = 0; k < qi; ++k) memcpy(hB.data() + (size_t)k * (size_t)p, B + (size_t)k * (size_t)ldb, sizeof(double) * (size_t)p);
    const int b = vp_bits(m);
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        const double *dX = X, *dP = Pred, *dY = Y;
        const int64_t *drows = rows;
        const int32_t *dperm = perm;
        int64_t ldxd = ldx, ldpd = ldp, ldyd = ldy, ldpermd = ldperm;
        JCH_TRY(jch_stage_in(ctx, host, ws + oX, n, p, &dX, &ldxd));
        JCH_TRY(jch_stage_in(ctx, host, ws + oP, n, q, &dP, &ldpd));
        JCH_TRY(jch_stage_in(ctx, host, ws + oY, n, q, &dY, &ldyd));
        if (host && rows) {
            JCH_HIP(ctx, hipMemcpyAsync(ws + orows, rows, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
            drows = (const int64_t *)(ws + orows);
        }
        if (host && perm) {
            JCH_HIP(ctx, hipMemcpy2DAsync(ws + operm, sizeof(int32_t) * (size_t)m, perm, sizeof(int32_t) * (size_t)ldperm, sizeof(int32_t) * (size_t)m, (size_t)p,
                                          hipMemcpyHostToDevice, ctx->stream));
            dperm = (const int32_t *)(ws + operm);
            ldpermd = m;
        }
        JCH_HIP(ctx, hipMemcpyAsync(dB, hB.data(), sizeof(double) * hB.size(), hipMemcpyHostToDevice, ctx->stream));
        JCH_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(double), ctx->stream));
        const dim3 grid((unsigned)(ncolg * VP_XCDS * nslice));
        if (dperm)
            hipLaunchKernelGGL((k_vp_pass<false>), grid, dim3(VP_NT), 0, ctx->stream, dX, n, pi, ldxd, drows, m, dP, ldpd, dY, ldyd, qi, dB, dperm, ldpermd, seed, b / 2,
                               vp_rounds(b), (int)nslice, part, flag);
        else
            hipLaunchKernelGGL((k_vp_pass<true>), grid, dim3(VP_NT), 0, ctx->stream, dX, n, pi, ldxd, drows, m, dP, ldpd, dY, ldyd, qi, dB, dperm, ldpermd, seed, b / 2,
                               vp_rounds(b), (int)nslice, part, flag);
        hipLaunchKernelGGL(k_vp_reduce, dim3((unsigned)((nout + VP_NT - 1) / VP_NT)), dim3(VP_NT), 0, ctx->stream, part, p + 1, (int)nslice, q6, out);
        JCH_HIP(ctx, hipGetLastError());
        JCH_HIP(ctx, hipMemcpyAsync(hs, out, sizeof(double) * (nout + 1), hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    }));
    if (*(const int *)(hs + nout)) return jch_fail(ctx, JCH_EINVAL, "%s: an entry of rows outside 0 .. n - 1 or of perm outside 0 .. m - 1", who);
    memcpy(sums, hs, sizeof(double) * nout);
    return JCH_OK;
}
