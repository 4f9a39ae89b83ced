// Exact column medians and MADs of a column-major device matrix: the order statistic the robust members of the reference need (`median(X, dims = 1)`,
// `colmad`, src/utility.jl:162; src/stah.jl:44-52) — jch_col_median_mad, include/jchemo_hip.h; DESIGN.md §18.
//
// A most-significant-digit radix select on the order-preserving 64-bit image of the doubles (key = bits ^ (sign ? all ones : the sign bit): the
// unsigned order of the keys is the order of the values, -0.0 just below +0.0, -Inf lowest, +Inf highest).  CS_PASSES passes of CS_BITS bits (the
// last one takes the 9 bits left); a pass is two kernels:
//
//   k_cs_hist    grid (row segments, column groups).  A workgroup owns CS_WG_ROWS rows of a column (more only when n > 65535 CS_WG_ROWS) and, when a
//                column is shorter than that, up to CS_MAXCPW columns one after the other.  It counts the digit of every element whose higher digits
//                equal the column's prefix into an LDS histogram with integer atomics and adds the non-zero bins to the column's global histogram
//                with 64-bit integer atomics: integer adds commute, two runs give identical bits.  8-byte loads only, so that an unaligned X and
//                an odd ldx run the same instructions.  Rows >= n are never read; row indices and counts are 64-bit.
//   k_cs_narrow  one workgroup per column: finds the digit that holds the sought rank, extends the prefix, reduces the rank to the rank within
//                that digit and zeroes the histogram for the next pass.  Behind the last pass the prefix IS the key of the order statistic.
//
// An even n follows both middle ranks in the same passes: while their prefixes agree (`same`) one histogram serves both; from the digit where they
// part, elements are tested against both prefixes and counted in two histograms.  median = lo for odd n, Julia's middle(lo, hi) = lo / 2 + hi / 2
// for even n.  The MAD is a second selection of the same kind over fl(|fl(x - med)|), recomputed from X in every pass: no n x p workspace.  The
// workspace is 2 CS_BINS counters and one state record per column of a chunk of CS_COLCHUNK columns; wider matrices are walked chunk by chunk.
// NaN: the first pass of a selection raises the column's flag, the result is NaN whatever the counts say (Julia's `median`); a NaN median makes every
// deviation NaN and so the MAD.  No early exit: 12 reads of X for both results, 6 for the medians alone.
// gfx950, hipcc -O3, no scratch: k_cs_hist 30 VGPRs in both instances (8 waves per SIMD), k_cs_narrow 52, k_cs_init 8; LDS 16 388 B (hist: 8 workgroups per CU), 4 144 B (narrow).
#include <stdint.h>

#include <algorithm>

#include "jch_internal.h"

#define CS_BITS 11
#define CS_BINS (1 << CS_BITS)
#define CS_PASSES 6                 // 5 x 11 + 9 bits
#define CS_NT 256
#define CS_WG_ROWS 8192             // rows of one column a workgroup counts per pass
#define CS_MAXCPW 64                // columns a workgroup serves when a column is shorter than CS_WG_ROWS
#define CS_COLCHUNK 1024            // columns selected by one sequence of launches: 32 MB of counters
#define CS_MAD_CONSTANT 1.4826022185056018   // StatsBase 0.33 / 0.34 `mad(x)`, normalize = true

typedef unsigned long long cs_u64;

struct cs_state {        // per column
    cs_u64 prefix[2];    // the digits decided so far of the two sought keys (lower bits zero)
    long long rank[2];   // 0-based rank of each among the elements that share its prefix
    int same;            // the two prefixes agree so far: histogram 0 serves both
    unsigned nan;        // a NaN was seen by the first pass
};

__device__ __forceinline__ cs_u64 cs_key(double v)
{
    const cs_u64 u = (cs_u64)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double cs_unkey(cs_u64 k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__global__ __launch_bounds__(64) void k_cs_init(cs_state *st, int pc, long long klo, long long khi)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c < pc) { st[c].prefix[0] = st[c].prefix[1] = 0; st[c].rank[0] = klo; st[c].rank[1] = khi; st[c].same = 1; st[c].nan = 0; }
}

// DEV: the values are fl(|fl(x - med[c])|)
template <bool DEV>
__global__ __launch_bounds__(CS_NT) void k_cs_hist(const double *__restrict__ X, int64_t n, int64_t ldx, int pc, int64_t rpw, int cpw, int pass, cs_state *st,
                                                   cs_u64 *hist, const double *__restrict__ med)
{
    __shared__ unsigned h[2 * CS_BINS];
    __shared__ unsigned sawnan;
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rpw, r1 = std::min<int64_t>(n, r0 + rpw);
    const int hib = 64 - CS_BITS * pass;              // bits not decided before this pass
    const int w = hib < CS_BITS ? hib : CS_BITS, sh = hib - w;
    const unsigned mask = (1u << w) - 1u;
    const int c1 = min(pc, ((int)blockIdx.y + 1) * cpw);
    for (int c = (int)blockIdx.y * cpw; c < c1; ++c) {
        for (int e = tid; e < 2 * CS_BINS; e += CS_NT) h[e] = 0;
        if (tid == 0) sawnan = 0;
        __syncthreads();
        const cs_u64 p0 = st[c].prefix[0], p1 = st[c].prefix[1];
        const bool two = st[c].same == 0;
        const double m = DEV ? med[c] : 0.0;
        const double *x = X + (size_t)c * (size_t)ldx;
        auto count = [&](double v) {
            if (DEV) v = fabs(v - m);
            if (pass == 0 && v != v) sawnan = 1;
            const cs_u64 key = cs_key(v);
            const unsigned dg = (unsigned)(key >> sh) & mask;
            if (pass == 0 || ((key ^ p0) >> hib) == 0) atomicAdd(&h[dg], 1u);
            if (two && ((key ^ p1) >> hib) == 0) atomicAdd(&h[CS_BINS + dg], 1u);
        };
        int64_t i = r0 + tid;
        for (; i + 3 * CS_NT < r1; i += 4 * CS_NT) {   // four loads in flight per lane
            const double v0 = x[i], v1 = x[i + CS_NT], v2 = x[i + 2 * CS_NT], v3 = x[i + 3 * CS_NT];
            count(v0); count(v1); count(v2); count(v3);
        }
        for (; i < r1; i += CS_NT) count(x[i]);
        __syncthreads();
        cs_u64 *g = hist + (size_t)c * (2 * CS_BINS);
        for (int e = tid; e < 2 * CS_BINS; e += CS_NT) {
            const unsigned v = h[e];
            if (v) atomicAdd(&g[e], (cs_u64)v);
        }
        if (tid == 0 && sawnan) atomicOr(&st[c].nan, 1u);
        __syncthreads();
    }
}

// stage 0: behind the last pass med_out[c] = the median and the state is set up for the selection of the deviations; stage 1: mad_out[c]
__global__ __launch_bounds__(CS_NT) void k_cs_narrow(cs_state *st, cs_u64 *hist, int pass, int64_t n, int stage, double *med_out, double *mad_out)
{
    constexpr int PER = CS_BINS / CS_NT;
    __shared__ cs_u64 part[2][CS_NT];
    __shared__ int chunk[2];
    __shared__ cs_u64 base[2];
    __shared__ unsigned digit[2];
    __shared__ long long nrank[2];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int hib = 64 - CS_BITS * pass;
    const int sh = hib - (hib < CS_BITS ? hib : CS_BITS);
    const int same = st[c].same;
    const long long rank[2] = {st[c].rank[0], st[c].rank[1]};
    cs_u64 *g = hist + (size_t)c * (2 * CS_BINS);
    cs_u64 cnt[2][PER];
#pragma unroll
    for (int b = 0; b < PER; ++b) {
        cnt[0][b] = g[tid * PER + b];
        cnt[1][b] = same ? cnt[0][b] : g[CS_BINS + tid * PER + b];
        g[tid * PER + b] = 0;
        g[CS_BINS + tid * PER + b] = 0;
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        cs_u64 s = 0;
#pragma unroll
        for (int b = 0; b < PER; ++b) s += cnt[r][b];
        part[r][tid] = s;
    }
    if (tid < 2) { chunk[tid] = CS_NT - 1; base[tid] = 0; }
    __syncthreads();
    if (tid < 2) {   // the thread whose bins hold the rank (the counts of a prefix sum to more than its rank: the last chunk is never needed as a default)
        cs_u64 acc = 0;
        for (int t = 0; t < CS_NT; ++t) {
            if (acc + part[tid][t] > (cs_u64)rank[tid]) { chunk[tid] = t; base[tid] = acc; break; }
            acc += part[tid][t];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r)
        if (chunk[r] == tid) {
            cs_u64 acc = base[r];
            int b = 0;
            for (; b < PER - 1; ++b) {
                if (acc + cnt[r][b] > (cs_u64)rank[r]) break;
                acc += cnt[r][b];
            }
            digit[r] = (unsigned)(tid * PER + b);
            nrank[r] = rank[r] - (long long)acc;
        }
    __syncthreads();
    if (tid == 0) {
        const cs_u64 k0 = st[c].prefix[0] | ((cs_u64)digit[0] << sh), k1 = st[c].prefix[1] | ((cs_u64)digit[1] << sh);
        if (pass + 1 < CS_PASSES) {
            st[c].prefix[0] = k0; st[c].prefix[1] = k1;
            st[c].rank[0] = nrank[0]; st[c].rank[1] = nrank[1];
            st[c].same = same && digit[0] == digit[1];
        } else {
            const double lo = cs_unkey(k0), hi = cs_unkey(k1);
            double v = (n & 1) ? lo : __dadd_rn(__dmul_rn(lo, 0.5), __dmul_rn(hi, 0.5));   // Julia's middle(lo, hi)
            if (st[c].nan) v = __longlong_as_double(0x7ff8000000000000ll);
            if (stage == 0) med_out[c] = v; else mad_out[c] = __dmul_rn(CS_MAD_CONSTANT, v);
            st[c].prefix[0] = st[c].prefix[1] = 0;
            st[c].rank[0] = (long long)((n - 1) / 2); st[c].rank[1] = (long long)(n / 2);
            st[c].same = 1; st[c].nan = 0;
        }
    }
}

static size_t cs_ws_bytes(int64_t p)
{
    const size_t pc = (size_t)std::min<int64_t>(p, CS_COLCHUNK);
    return pc * (2 * CS_BINS * sizeof(cs_u64) + sizeof(cs_state));
}

int32_t jch_colselect_reserve(jch_ctx *ctx, int64_t p) { return jch_reserve(ctx, ctx->sel_ws, cs_ws_bytes(p)); }

// X, med, mad: device; med is always written (the deviations need it), mad may be null.  Needs jch_colselect_reserve(ctx, p); enqueues only.
int32_t jch_launch_col_median_mad(jch_ctx *ctx, const double *X, int64_t n, int64_t p, int64_t ldx, double *med, double *mad)
{
    const int64_t rpw = std::max<int64_t>(CS_WG_ROWS, (n + 65534) / 65535);
    const int64_t segs = (n + rpw - 1) / rpw;
    const int cpw = segs > 1 ? 1 : (int)std::max<int64_t>(1, std::min<int64_t>(CS_MAXCPW, CS_WG_ROWS / n));
    for (int64_t c0 = 0; c0 < p; c0 += CS_COLCHUNK) {
        const int pc = (int)std::min<int64_t>(CS_COLCHUNK, p - c0);
        cs_u64 *hist = (cs_u64 *)ctx->sel_ws.ptr;
        cs_state *st = (cs_state *)(hist + (size_t)std::min<int64_t>(p, CS_COLCHUNK) * (2 * CS_BINS));
        JCH_HIP(ctx, hipMemsetAsync(hist, 0, (size_t)pc * 2 * CS_BINS * sizeof(cs_u64), ctx->stream));
        hipLaunchKernelGGL(k_cs_init, dim3((unsigned)((pc + 63) / 64)), dim3(64), 0, ctx->stream, st, pc, (long long)((n - 1) / 2), (long long)(n / 2));
        const double *Xc = X + (size_t)c0 * (size_t)ldx;
        const dim3 grid((unsigned)segs, (unsigned)((pc + cpw - 1) / cpw));
        for (int stage = 0; stage < (mad ? 2 : 1); ++stage)
            for (int pass = 0; pass < CS_PASSES; ++pass) {
                if (stage == 0) hipLaunchKernelGGL(k_cs_hist<false>, grid, dim3(CS_NT), 0, ctx->stream, Xc, n, ldx, pc, rpw, cpw, pass, st, hist, (const double *)nullptr);
                else hipLaunchKernelGGL(k_cs_hist<true>, grid, dim3(CS_NT), 0, ctx->stream, Xc, n, ldx, pc, rpw, cpw, pass, st, hist, (const double *)(med + c0));
                hipLaunchKernelGGL(k_cs_narrow, dim3((unsigned)pc), dim3(CS_NT), 0, ctx->stream, st, hist, pass, n, stage, med + c0, mad ? mad + c0 : nullptr);
            }
        JCH_HIP(ctx, hipGetLastError());
    }
    return JCH_OK;
}

extern "C" int32_t jch_col_median_mad(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, double *med, double *mad, int32_t out_loc)
{
    if (!ctx) return JCH_EINVAL;
    if (!X || !med || n < 1 || p < 1 || ldx < n) return jch_fail(ctx, JCH_EINVAL, "jch_col_median_mad: bad arguments");
    if ((loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) || (out_loc != JCH_LOC_HOST && out_loc != JCH_LOC_DEVICE))
        return jch_fail(ctx, JCH_EINVAL, "jch_col_median_mad: bad loc");
    if (ctx->nranks > 1) return jch_fail(ctx, JCH_EINVAL, "jch_col_median_mad: one rank only (communicator of %d)", ctx->nranks);   // a median needs every row
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    JCH_TRY(jch_colselect_reserve(ctx, p));
    if (loc == JCH_LOC_HOST) JCH_TRY(jch_reserve(ctx, ctx->xq, sizeof(double) * (size_t)n * (size_t)p));
    if (out_loc == JCH_LOC_HOST) JCH_TRY(jch_reserve(ctx, ctx->sel_out, sizeof(double) * 2 * (size_t)p));
    return jch_synced(ctx, loc == JCH_LOC_HOST || out_loc == JCH_LOC_HOST, [&]() -> int32_t {
        const double *dX = X;
        int64_t ldxd = ldx;
        JCH_TRY(jch_stage_in(ctx, loc == JCH_LOC_HOST, (double *)ctx->xq.ptr, n, p, &dX, &ldxd));
        double *dmed = med, *dmad = mad;
        if (out_loc == JCH_LOC_HOST) { dmed = (double *)ctx->sel_out.ptr; dmad = mad ? dmed + p : nullptr; }
        JCH_TRY(jch_launch_col_median_mad(ctx, dX, n, p, ldxd, dmed, dmad));
        if (out_loc == JCH_LOC_HOST) {
            JCH_HIP(ctx, hipMemcpyAsync(med, dmed, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, ctx->stream));
            if (mad) JCH_HIP(ctx, hipMemcpyAsync(mad, dmad, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, ctx->stream));
        }
        return JCH_OK;
    });
}
