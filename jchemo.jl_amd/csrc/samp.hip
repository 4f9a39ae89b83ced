// Kennard-Stone and Duplex sampling (src/sampling.jl:40-148) without the n x n distance matrix — jch_farthest_pair and jch_maxmin_select,
// include/jchemo_hip.h; DESIGN.md §19.
//
// The reference builds D = euclsq(X, X) and, per selected row, takes a minimum over D[s, cand]: 8 n^2 bytes and O(k^2 n) work.  Both algorithms are
// max-min selections: the start is the farthest pair, every later row is argmax_i min_{s selected} d2(i, s).
//
// jch_farthest_pair: the maximum over the tiles of the symmetric Gram of k_gram (kgram.hip), with the stores removed.
//   k_sp_rowflag    one lane per row: 1 when every entry of the row is finite and the row is not in `skip` (the candidates)
//   k_sp_colmean    c = the column means over the candidates: some candidate j has (x_i - c).(x_j - c) <= 0, so the largest d2 is at least the largest
//                   centred squared norm and the cancellation of |a_i|^2 + |a_j|^2 - 2 a_i.a_j is bounded by the result
//   (kgram.hip)     the zero-padded copy of X - 1 c' and its squared row norms: jch_launch_kgram_prep
//   k_sp_masknorms  the norm of every row that is no candidate (and of the padding rows) becomes NaN: its d2 are NaN and lose every comparison
//   k_sp_pair       t128_mma on the tiles ti <= tj of the triangle; epilogue in registers: each workgroup keeps one (d2, row, col), row > col,
//                   by the total order (d2 descending, col ascending, row ascending) — the first maximum of a column-major scan of the
//                   symmetric D (`findall(D .== maximum(D))[1]`); registers -> wave shuffles -> LDS -> one triple per workgroup
//   k_sp_pair_final one workgroup reduces the triples by the same order (the result does not depend on the order of the tiles) and recomputes the
//                   winner's d2 in direct form, sum_j (x_rj - x_cj)^2 in ascending j: bitwise what k_mm_step computes for that pair
// jch_maxmin_select: one n-vector of running minima per set, one streaming read of the column-major X per selected row (per pair of rows for Duplex).
//   k_mm_gather     the starting rows as p-vectors
//   k_mm_step       one lane per row (every column access of a wave is one contiguous 512-byte run, RP_U-style unrolling keeps 8 loads in flight);
//                   the targets are read wave-uniformly; d2 in direct form, ascending j; mind = min(mind, d2); the rows that are this pass's
//                   targets become taken (-1), a row with a non-finite d2 becomes invalid for good (-2); then the block's argmax of
//                   (mind descending, index ascending) over the rows with mind >= 0 — for the second set of Duplex its top two
//   k_mm_finish     one workgroup: the partials in the same order; Duplex: the second set takes its runner-up when its best is the row the first set
//                   takes in this step (sampling.jl:141-143); appends to sel / dsel, gathers the new rows for the next pass
// No atomics; every output is a fixed-order sum or the extremum of a total order: two runs give identical bits, and so do a host and a device X.
// gfx950, hipcc -O3, no scratch: k_sp_pair 199 VGPRs (two workgroups per CU, as k_gram), k_mm_step<1, 1> 26, k_mm_step<2, 1> 31, k_mm_step<2, 2> 52.
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "jch_internal.h"
#include "tile128_dev.h"

#define SP_NT 256          // rows per workgroup of the row-per-lane kernels
#define SP_U 8             // columns loaded ahead per lane (RP_U of rowprep.hip)
#define SP_FINAL_NT 1024   // threads of k_sp_pair_final
#define SP_NONE INT64_MAX  // index of "no candidate"

// ---- (d2 descending, col ascending, row ascending); a NaN d2 compares false both ways and never replaces anything ---------------------------
__device__ __forceinline__ bool sp_better(double d, int64_t r, int64_t c, double bd, int64_t br, int64_t bc)
{
    return d > bd || (d == bd && (c < bc || (c == bc && r < br)));
}

__device__ __forceinline__ void sp_wave_best(double &d, int64_t &r, int64_t &c)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(d, o, 64);
        const int64_t orow = __shfl_xor((long long)r, o, 64), oc = __shfl_xor((long long)c, o, 64);
        if (sp_better(od, orow, oc, d, r, c)) { d = od; r = orow; c = oc; }
    }
}

__global__ __launch_bounds__(SP_NT) void k_sp_rowflag(const double *__restrict__ X, int64_t n, int64_t p, int64_t ldx, const int64_t *__restrict__ skip,
                                                      int nskip, unsigned char *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * SP_NT + threadIdx.x;
    if (i >= n) return;
    const double *x = X + i;
    bool ok = true;
#pragma unroll SP_U
    for (int64_t j = 0; j < p; ++j) ok &= fabs(x[j * ldx]) <= DBL_MAX;
    for (int s = 0; s < nskip; ++s) ok &= skip[s] != i;
    flag[i] = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_sp_colmean(const double *__restrict__ X, int64_t n, int64_t ldx, const unsigned char *__restrict__ flag,
                                                    double *__restrict__ c)
{
    __shared__ double scr[4];
    const int64_t k = blockIdx.x;
    double s = 0.0, cnt = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256)
        if (flag[i]) { s += X[(size_t)i + (size_t)k * (size_t)ldx]; cnt += 1.0; }
    s = jch_block_sum<256>(s, scr);
    cnt = jch_block_sum<256>(cnt, scr);
    if (threadIdx.x == 0) c[k] = cnt > 0.0 ? s / cnt : 0.0;
}

__global__ __launch_bounds__(256) void k_sp_masknorms(double *__restrict__ nrm, int64_t ldc, int64_t n, const unsigned char *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < ldc && (i >= n || !flag[i])) nrm[i] = __longlong_as_double(0x7ff8000000000000ll);
}

__global__ __launch_bounds__(256, 2) void k_sp_pair(const double *__restrict__ Xc, int64_t ldc, int pp, const double *__restrict__ nrm, double *__restrict__ pd,
                                                    int64_t *__restrict__ prow, int64_t *__restrict__ pcol)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t ti, tj;
    t128_tri(blockIdx.x, ti, tj);   // ti <= tj
    const int64_t i0 = ti * T128_T, j0 = tj * T128_T;
    const int qj = wv >> 1, qi = wv & 1;
    t128_v4d acc[4][4];
    t128_mma(
        lds, pp / T128_KB,
        [&](int k, int c) { return __builtin_nontemporal_load(reinterpret_cast<const t128_v2d *>(Xc + (size_t)k * (size_t)ldc + (size_t)j0 + c)); },
        [&](int k, int c) { return __builtin_nontemporal_load(reinterpret_cast<const t128_v2d *>(Xc + (size_t)k * (size_t)ldc + (size_t)i0 + c)); },
        acc);
    // acc[mj][ni][reg] = a_j.a_i, j = j0 + 64 qj + 16 mj + (lane >> 4) + 4 reg, i = i0 + 64 qi + 16 ni + (lane & 15); the pair is (row j, col i), j > i
    double bd = -1.0;
    int64_t br = SP_NONE, bc = SP_NONE;
    double zn[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) zn[ni] = nrm[i0 + 64 * qi + 16 * ni + (lane & 15)];
#pragma unroll
    for (int mj = 0; mj < 4; ++mj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t j = j0 + 64 * qj + 16 * mj + (lane >> 4) + 4 * reg;
            const double xn = nrm[j];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int64_t i = i0 + 64 * qi + 16 * ni + (lane & 15);
                double d = zn[ni] + xn - 2.0 * acc[mj][ni][reg];
                d = d < 0.0 ? 0.0 : d;   // euclsq's clamp; a NaN stays a NaN
                if (j > i && sp_better(d, j, i, bd, br, bc)) { bd = d; br = j; bc = i; }
            }
        }
    sp_wave_best(bd, br, bc);
    int64_t *li = reinterpret_cast<int64_t *>(lds + 4);   // t128_mma ended behind a barrier: lds is free
    if (lane == 0) { lds[wv] = bd; li[wv] = br; li[4 + wv] = bc; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (sp_better(lds[w], li[w], li[4 + w], bd, br, bc)) { bd = lds[w]; br = li[w]; bc = li[4 + w]; }
        pd[blockIdx.x] = bd; prow[blockIdx.x] = br; pcol[blockIdx.x] = bc;
    }
}

// res_d[0] = the winner's d2 in direct form, res_i[0 .. 1] = (row, col); no pair at all: res_i[0] = -1
__global__ __launch_bounds__(SP_FINAL_NT) void k_sp_pair_final(const double *__restrict__ pd, const int64_t *__restrict__ prow, const int64_t *__restrict__ pcol,
                                                               int64_t nb, const double *__restrict__ X, int64_t p, int64_t ldx, double *__restrict__ res_d,
                                                               int64_t *__restrict__ res_i)
{
    __shared__ double sd[SP_FINAL_NT];
    __shared__ int64_t sr[SP_FINAL_NT / 64], sc[SP_FINAL_NT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double bd = -1.0;
    int64_t br = SP_NONE, bc = SP_NONE;
    for (int64_t b = tid; b < nb; b += SP_FINAL_NT)
        if (sp_better(pd[b], prow[b], pcol[b], bd, br, bc)) { bd = pd[b]; br = prow[b]; bc = pcol[b]; }
    sp_wave_best(bd, br, bc);
    if (lane == 0) { sd[wv] = bd; sr[wv] = br; sc[wv] = bc; }
    __syncthreads();
    bd = sd[0]; br = sr[0]; bc = sc[0];
    for (int w = 1; w < SP_FINAL_NT / 64; ++w)
        if (sp_better(sd[w], sr[w], sc[w], bd, br, bc)) { bd = sd[w]; br = sr[w]; bc = sc[w]; }
    __syncthreads();
    if (br == SP_NONE) {
        if (tid == 0) { res_d[0] = 0.0; res_i[0] = -1; res_i[1] = -1; }
        return;
    }
    double acc = 0.0;
    for (int64_t j0 = 0; j0 < p; j0 += SP_FINAL_NT) {
        const int64_t j = j0 + tid;
        if (j < p) sd[tid] = X[(size_t)br + (size_t)j * (size_t)ldx] - X[(size_t)bc + (size_t)j * (size_t)ldx];
        __syncthreads();
        if (tid == 0) {
            const int m = (int)std::min<int64_t>(SP_FINAL_NT, p - j0);
            for (int t = 0; t < m; ++t) acc = fma(sd[t], sd[t], acc);
        }
        __syncthreads();
    }
    if (tid == 0) { res_d[0] = acc; res_i[0] = br; res_i[1] = bc; }
}

static int32_t sp_check_x(jch_ctx *ctx, const char *who, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx)
{
    if (!X || n < 1 || p < 1 || p > (1 << 30) || ldx < n) return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments", who);
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc", who);
    if (ctx->nranks > 1) return jch_fail(ctx, JCH_EINVAL, "%s: one rank only (communicator of %d)", who, ctx->nranks);
    return JCH_OK;
}

extern "C" int32_t jch_farthest_pair(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const int64_t *skip, int32_t nskip,
                                     int64_t *pair, double *d2)
{
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(sp_check_x(ctx, "jch_farthest_pair", loc, X, n, p, ldx));
    if (!pair || !d2 || nskip < 0 || (nskip > 0 && !skip)) return jch_fail(ctx, JCH_EINVAL, "jch_farthest_pair: bad arguments");
    std::vector<int64_t> sk(skip, skip + nskip);
    std::sort(sk.begin(), sk.end());
    sk.erase(std::unique(sk.begin(), sk.end()), sk.end());
    if (!sk.empty() && (sk.front() < 0 || sk.back() >= n)) return jch_fail(ctx, JCH_EINVAL, "jch_farthest_pair: skip index out of range");
    if (n - (int64_t)sk.size() < 2) return jch_fail(ctx, JCH_EINVAL, "jch_farthest_pair: fewer than two unskipped rows (n=%lld)", (long long)n);
    const int ns = (int)sk.size();
    const int64_t pp = (p + T128_KB - 1) / T128_KB * T128_KB;
    const int64_t tiles = (n + T128_T - 1) / T128_T, ldc = tiles * T128_T;
    const int64_t nblocks = tiles * (tiles + 1) / 2;
    if (nblocks > 0x7fffffffLL) return jch_fail(ctx, JCH_EINVAL, "jch_farthest_pair: shape too large (n=%lld: more than 2^31 tiles)", (long long)n);
    jch_carve cv;
    const size_t o_flag = cv.take((size_t)(n + 7) / 8), o_skip = cv.take((size_t)std::max(ns, 1)), o_c = cv.take((size_t)pp), o_nrm = cv.take((size_t)ldc);
    const size_t o_pd = cv.take((size_t)nblocks), o_pr = cv.take((size_t)nblocks), o_pc = cv.take((size_t)nblocks), o_res = cv.take(4);
    const size_t o_cp = cv.take((size_t)ldc * (size_t)pp);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    JCH_TRY(jch_reserve(ctx, ctx->sp_ws, sizeof(double) * cv.off));
    JCH_TRY(jch_reserve_host(ctx, 64));
    if (loc == JCH_LOC_HOST) JCH_TRY(jch_reserve(ctx, ctx->xq, sizeof(double) * (size_t)n * (size_t)p));
    double *ws = (double *)ctx->sp_ws.ptr;
    unsigned char *flag = (unsigned char *)(ws + o_flag);
    int64_t *dskip = (int64_t *)(ws + o_skip), *prow = (int64_t *)(ws + o_pr), *pcol = (int64_t *)(ws + o_pc), *res_i = (int64_t *)(ws + o_res) + 1;
    double *c = ws + o_c, *nrm = ws + o_nrm, *pd = ws + o_pd, *res_d = ws + o_res, *cp = ws + o_cp;
    static jch_per_device_once attr;
    if (!attr.done(ctx->device)) {
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_sp_pair, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr.mark(ctx->device);
    }
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        const double *dX = X;
        int64_t ldxd = ldx;
        JCH_TRY(jch_stage_in(ctx, loc == JCH_LOC_HOST, (double *)ctx->xq.ptr, n, p, &dX, &ldxd));
        if (ns) JCH_HIP(ctx, hipMemcpyAsync(dskip, sk.data(), sizeof(int64_t) * (size_t)ns, hipMemcpyHostToDevice, ctx->stream));
        const unsigned nbr = (unsigned)((n + SP_NT - 1) / SP_NT);
        hipLaunchKernelGGL(k_sp_rowflag, dim3(nbr), dim3(SP_NT), 0, ctx->stream, dX, n, p, ldxd, (const int64_t *)dskip, ns, flag);
        hipLaunchKernelGGL(k_sp_colmean, dim3((unsigned)p), dim3(256), 0, ctx->stream, dX, n, ldxd, (const unsigned char *)flag, c);
        JCH_TRY(jch_launch_kgram_prep(ctx, dX, n, ldxd, p, c, cp, ldc, pp, nrm));
        hipLaunchKernelGGL(k_sp_masknorms, dim3((unsigned)((ldc + 255) / 256)), dim3(256), 0, ctx->stream, nrm, ldc, n, (const unsigned char *)flag);
        hipLaunchKernelGGL(k_sp_pair, dim3((unsigned)nblocks), dim3(256), T128_LDS_BYTES, ctx->stream, (const double *)cp, ldc, (int)pp, (const double *)nrm, pd,
                           prow, pcol);
        hipLaunchKernelGGL(k_sp_pair_final, dim3(1), dim3(SP_FINAL_NT), 0, ctx->stream, (const double *)pd, (const int64_t *)prow, (const int64_t *)pcol, nblocks,
                           dX, p, ldxd, res_d, res_i);
        JCH_HIP(ctx, hipGetLastError());
        JCH_HIP(ctx, hipMemcpyAsync(ctx->hstage, res_d, 32, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    }));
    const int64_t *hi = (const int64_t *)ctx->hstage + 1;
    if (hi[0] < 0) return jch_fail(ctx, JCH_EINVAL, "jch_farthest_pair: fewer than two unskipped rows without a non-finite entry");
    pair[0] = hi[0]; pair[1] = hi[1];
    *d2 = *(const double *)ctx->hstage;
    return JCH_OK;
}

// ---- max-min selection ----------------------------------------------------------------------------------------------------------------------
// (mind descending, index ascending) over the candidates (mind >= 0); anything else enters as (-1, SP_NONE) and loses to every candidate
__device__ __forceinline__ bool mm_better(double m, int64_t i, double bm, int64_t bi) { return m > bm || (m == bm && i < bi); }

// block argmax, valid in every thread; scr_m / scr_i: SP_NT / 64 entries of LDS each, free again on return
__device__ __forceinline__ void mm_block_best(double &m, int64_t &i, double *scr_m, int64_t *scr_i)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double om = __shfl_xor(m, o, 64);
        const int64_t oi = __shfl_xor((long long)i, o, 64);
        if (mm_better(om, oi, m, i)) { m = om; i = oi; }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { scr_m[wv] = m; scr_i[wv] = i; }
    __syncthreads();
    m = scr_m[0]; i = scr_i[0];
#pragma unroll
    for (int w = 1; w < SP_NT / 64; ++w)
        if (mm_better(scr_m[w], scr_i[w], m, i)) { m = scr_m[w]; i = scr_i[w]; }
    __syncthreads();
}

__global__ __launch_bounds__(SP_NT) void k_mm_gather(const double *__restrict__ X, int64_t p, int64_t ldx, const int64_t *__restrict__ cur, double *__restrict__ tgt,
                                                     int64_t pstride)
{
    const int64_t w = cur[blockIdx.x];
    for (int64_t j = threadIdx.x; j < p; j += SP_NT) tgt[(size_t)blockIdx.x * pstride + j] = X[(size_t)w + (size_t)j * (size_t)ldx];
}

// NS sets, NT targets per set (2: the first pass, which folds the starting pairs; 1: every later pass).  cur[s * NT + t] / tgt[(s * NT + t) * pstride ..]:
// the targets' indices and rows.  mind[s * n + i].  part_m / part_i[slot * nb + block]: slot 0 the best of set 0, slot 1 / 2 the best two of set 1.
template <int NS, int NT>
__global__ __launch_bounds__(SP_NT) void k_mm_step(const double *__restrict__ X, int64_t n, int64_t p, int64_t ldx, const double *__restrict__ tgt, int64_t pstride,
                                                   const int64_t *__restrict__ cur, double *__restrict__ mind, int first, double *__restrict__ part_m,
                                                   int64_t *__restrict__ part_i, int64_t *__restrict__ sel, double *__restrict__ dsel, int64_t k)
{
    __shared__ double scr_m[SP_NT / 64];
    __shared__ int64_t scr_i[SP_NT / 64];
    const int64_t i = (int64_t)blockIdx.x * SP_NT + threadIdx.x;
    const bool live = i < n;
    const double *x = X + (live ? i : n - 1);
    double acc[NS][NT];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[s][t] = 0.0;
#pragma unroll SP_U
    for (int64_t j = 0; j < p; ++j) {
        const double v = x[j * ldx];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double d = v - tgt[(s * NT + t) * pstride + j];
                acc[s][t] = fma(d, d, acc[s][t]);
            }
    }
    bool fin = true, istgt = false;
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            fin &= acc[s][t] <= DBL_MAX;
            istgt |= cur[s * NT + t] == i;
        }
    double m[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        double d = acc[s][0];
        if (NT == 2) d = acc[s][1] < d ? acc[s][1] : d;
        double mm = (first || !live) ? INFINITY : mind[(size_t)s * (size_t)n + (size_t)i];
        if (mm >= 0.0) mm = d < mm ? d : mm;
        if (!fin) mm = -2.0;
        if (istgt) mm = -1.0;
        if (live) mind[(size_t)s * (size_t)n + (size_t)i] = mm;
        m[s] = live ? mm : -1.0;
        if (NT == 2 && first && live) {   // the starting pair of the set: its place in sel, its mutual d2 in dsel
            if (i == cur[s * 2]) { sel[s * k] = i; dsel[s * k] = acc[s][1]; dsel[s * k + 1] = acc[s][1]; }
            if (i == cur[s * 2 + 1]) sel[s * k + 1] = i;
        }
    }
    const size_t nb = gridDim.x, b = blockIdx.x;
    {
        double bm = m[0] >= 0.0 ? m[0] : -1.0;
        int64_t bi = m[0] >= 0.0 ? i : SP_NONE;
        mm_block_best(bm, bi, scr_m, scr_i);
        if (threadIdx.x == 0) { part_m[b] = bm; part_i[b] = bi; }
    }
    if (NS == 2) {
        const bool cand = m[NS - 1] >= 0.0;
        double bm = cand ? m[NS - 1] : -1.0;
        int64_t bi = cand ? i : SP_NONE;
        mm_block_best(bm, bi, scr_m, scr_i);
        double cm = (cand && i != bi) ? m[NS - 1] : -1.0;
        int64_t ci = (cand && i != bi) ? i : SP_NONE;
        mm_block_best(cm, ci, scr_m, scr_i);
        if (threadIdx.x == 0) { part_m[nb + b] = bm; part_i[nb + b] = bi; part_m[2 * nb + b] = cm; part_i[2 * nb + b] = ci; }
    }
}

// the t-th row of every set (0-based position t >= 2) from the partials of the pass before; sel gets -1 when no candidate is left
template <int NS>
__global__ __launch_bounds__(SP_NT) void k_mm_finish(const double *__restrict__ part_m, const int64_t *__restrict__ part_i, int64_t nb, const double *__restrict__ X,
                                                     int64_t p, int64_t ldx, double *__restrict__ tgt, int64_t pstride, int64_t *__restrict__ cur,
                                                     int64_t *__restrict__ sel, double *__restrict__ dsel, int64_t k, int64_t t)
{
    __shared__ double scr_m[SP_NT / 64];
    __shared__ int64_t scr_i[SP_NT / 64];
    double wm[NS];
    int64_t wi[NS];
    {
        double bm = -1.0;
        int64_t bi = SP_NONE;
        for (int64_t b = threadIdx.x; b < nb; b += SP_NT)
            if (mm_better(part_m[b], part_i[b], bm, bi)) { bm = part_m[b]; bi = part_i[b]; }
        mm_block_best(bm, bi, scr_m, scr_i);
        wm[0] = bm; wi[0] = bi;
    }
    if (NS == 2) {
        // the best entry of set 1 that is not the row set 0 takes in this step: its best, or its runner-up
        double bm = -1.0;
        int64_t bi = SP_NONE;
        for (int64_t b = threadIdx.x; b < 2 * nb; b += SP_NT) {
            const double pm = part_m[nb + b];
            const int64_t pi = part_i[nb + b];
            if (pi != wi[0] && mm_better(pm, pi, bm, bi)) { bm = pm; bi = pi; }
        }
        mm_block_best(bm, bi, scr_m, scr_i);
        wm[NS - 1] = bm; wi[NS - 1] = bi;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int64_t w = wi[s] == SP_NONE ? -1 : wi[s];
        if (threadIdx.x == 0) { sel[s * k + t] = w; dsel[s * k + t] = wm[s]; cur[s] = w; }
        if (w >= 0)
            for (int64_t j = threadIdx.x; j < p; j += SP_NT) tgt[(size_t)s * pstride + j] = X[(size_t)w + (size_t)j * (size_t)ldx];
    }
}

template <int NS>
static void mm_enqueue(jch_ctx *ctx, const double *X, int64_t n, int64_t p, int64_t ldx, int64_t k, double *tgt, int64_t pstride, int64_t *cur, double *mind,
                       double *part_m, int64_t *part_i, int64_t *sel, double *dsel)
{
    const int64_t nb = (n + SP_NT - 1) / SP_NT;
    hipLaunchKernelGGL(k_mm_gather, dim3(2 * NS), dim3(SP_NT), 0, ctx->stream, X, p, ldx, (const int64_t *)cur, tgt, pstride);
    hipLaunchKernelGGL((k_mm_step<NS, 2>), dim3((unsigned)nb), dim3(SP_NT), 0, ctx->stream, X, n, p, ldx, (const double *)tgt, pstride, (const int64_t *)cur, mind, 1,
                       part_m, part_i, sel, dsel, k);
    for (int64_t t = 2; t < k; ++t) {
        hipLaunchKernelGGL((k_mm_finish<NS>), dim3(1), dim3(SP_NT), 0, ctx->stream, (const double *)part_m, (const int64_t *)part_i, nb, X, p, ldx, tgt, pstride, cur,
                           sel, dsel, k, t);
        if (t + 1 < k)
            hipLaunchKernelGGL((k_mm_step<NS, 1>), dim3((unsigned)nb), dim3(SP_NT), 0, ctx->stream, X, n, p, ldx, (const double *)tgt, pstride, (const int64_t *)cur,
                               mind, 0, part_m, part_i, sel, dsel, k);
    }
}

extern "C" int32_t jch_maxmin_select(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, int32_t nsets, const int64_t *init, int64_t k,
                                     int64_t *sel, double *dsel)
{
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(sp_check_x(ctx, "jch_maxmin_select", loc, X, n, p, ldx));
    if (!init || !sel || (nsets != 1 && nsets != 2)) return jch_fail(ctx, JCH_EINVAL, "jch_maxmin_select: bad arguments");
    if (k < 2 || (nsets == 1 && k > n) || (nsets == 2 && k > n / 2))
        return jch_fail(ctx, JCH_EINVAL, "jch_maxmin_select: k = %lld rows per set do not fit %d set(s) of n = %lld rows", (long long)k, nsets, (long long)n);
    if ((n + SP_NT - 1) / SP_NT > 0x7fffffffLL) return jch_fail(ctx, JCH_EINVAL, "jch_maxmin_select: shape too large (n=%lld)", (long long)n);
    int64_t hinit[4];
    for (int a = 0; a < 2 * nsets; ++a) {
        hinit[a] = init[a];
        if (init[a] < 0 || init[a] >= n) return jch_fail(ctx, JCH_EINVAL, "jch_maxmin_select: init[%d] = %lld out of range", a, (long long)init[a]);
        for (int b = 0; b < a; ++b)
            if (init[b] == init[a]) return jch_fail(ctx, JCH_EINVAL, "jch_maxmin_select: init holds row %lld twice", (long long)init[a]);
    }
    const int64_t nb = (n + SP_NT - 1) / SP_NT, pstride = (p + 31) / 32 * 32;
    const size_t nk = (size_t)k * (size_t)nsets;
    jch_carve cv;
    const size_t o_cur = cv.take(4), o_tgt = cv.take((size_t)(4 * pstride)), o_pm = cv.take((size_t)(3 * nb)), o_pi = cv.take((size_t)(3 * nb));
    const size_t o_sel = cv.take(nk), o_dsel = cv.take(nk), o_mind = cv.take((size_t)n * (size_t)nsets);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    JCH_TRY(jch_reserve(ctx, ctx->sp_ws, sizeof(double) * cv.off));
    if (loc == JCH_LOC_HOST) JCH_TRY(jch_reserve(ctx, ctx->xq, sizeof(double) * (size_t)n * (size_t)p));
    double *ws = (double *)ctx->sp_ws.ptr;
    int64_t *cur = (int64_t *)(ws + o_cur), *part_i = (int64_t *)(ws + o_pi), *dsel_i = (int64_t *)(ws + o_sel);
    double *tgt = ws + o_tgt, *part_m = ws + o_pm, *ddsel = ws + o_dsel, *mind = ws + o_mind;
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        const double *dX = X;
        int64_t ldxd = ldx;
        JCH_TRY(jch_stage_in(ctx, loc == JCH_LOC_HOST, (double *)ctx->xq.ptr, n, p, &dX, &ldxd));   // staged once for all steps
        JCH_HIP(ctx, hipMemcpyAsync(cur, hinit, sizeof(int64_t) * 2 * (size_t)nsets, hipMemcpyHostToDevice, ctx->stream));
        if (nsets == 1) mm_enqueue<1>(ctx, dX, n, p, ldxd, k, tgt, pstride, cur, mind, part_m, part_i, dsel_i, ddsel);
        else mm_enqueue<2>(ctx, dX, n, p, ldxd, k, tgt, pstride, cur, mind, part_m, part_i, dsel_i, ddsel);
        JCH_HIP(ctx, hipGetLastError());
        JCH_HIP(ctx, hipMemcpyAsync(sel, dsel_i, sizeof(int64_t) * nk, hipMemcpyDeviceToHost, ctx->stream));
        if (dsel) JCH_HIP(ctx, hipMemcpyAsync(dsel, ddsel, sizeof(double) * nk, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    }));
    for (size_t a = 0; a < nk; ++a)
        if (sel[a] < 0) return jch_fail(ctx, JCH_EINVAL, "jch_maxmin_select: fewer than %lld rows per set without a non-finite entry", (long long)k);
    return JCH_OK;
}
