// Row sums of squared rank-k residuals: the device primitive behind the outlier distances `occsd`, `occod`, `occsdod`
// (src/occsd.jl, src/occod.jl, src/occsdod.jl) — jch_row_resid_ss, include/jchemo_hip.h; DESIGN.md §17.
//
//   out[i] = sum_j ( X[i, j] - shift[j] - sum_{l < k} Z[i, l] B[j, l] )^2
//
// The reference forms E = xresid(object, X) (m x p) and sums its squares by row (src/occod.jl:48-49).  E has rank-k structure,
// e_i = (x_i - xmeans) - Ps t_i with Ps = diag(xscales) P_k, so from the scores it costs 2 m p k flops and no output beyond one number per row.
//
//   k_row_resid_ss  k_affine_gemm_wideout's tile (gemm.hip), reading X where that kernel stores.  A persistent grid; a wave owns 64-row tiles
//                   (two row tiles of 32).  Its Z rows sit in registers as the B operand of v_mfma_f64_16x16x4_f64, the coefficients Bt[l][j] =
//                   B[j, l] in LDS as the A operand, so lane (kq, cl) holds the fitted values of rows 2 cl and 2 cl + 1 of columns kq + 4 reg of
//                   a 16-column tile: the matching X values are ONE 16-byte load per (reg, row tile) and sixteen lanes read one 256-byte run of a
//                   column.  Per column tile the lane forms e = (x - shift) - fit, and adds e^2 into its two row sums per row tile; after the last
//                   column tile the four kq groups are added as (kq0 + kq1) + (kq2 + kq3) and lane kq = 0 stores the row pair.  No atomics: the
//                   order is fixed, two runs give identical bits.
//   loads           every X load is issued unconditionally with clamped indices (rows past m re-read the last row or pair, columns past p re-read
//                   column p - 1) and what must not count is replaced by an exact zero AFTER the load (a select, not a branch: gemm.hip records
//                   a 2.3x loss from a branch around a load).  The next column tile's X — the first one of the wave's next row tile behind the
//                   last — is in flight while the current one is multiplied.
//   VEC = false     odd m, odd ldx or an X that is only 8-byte aligned: two 8-byte loads per pair, the same values in the same registers, hence the
//                   same bits.  Z (k / p of the traffic) is always read with 8-byte loads.
//   BLDS = false    the coefficients do not fit in LDS ((rows + 1) x ppad doubles: p = 2000 with k = 25 is 528 KB): the operand reads go to the
//                   same array in global memory (L2) instead.  Same products, same order.
//   k > 64          Z no longer fits in registers: the wave walks it in chunks of 64 columns inside every column tile, re-reading the chunk (L2)
//                   per tile.  Slower, never absent.  k = 0 (KS = 0) runs no MFMA at all: the centred row sums of squares.
//   Rows >= m and columns >= p are never read past the allocation; padding enters as exact zeros.  A NaN at X[i, j] or Z[i, l] stays in the
//   lane's sums of row i (the B operand's column cl carries row 2 cl or 2 cl + 1 only) and reaches out[i] alone.
// gfx950, hipcc -O3, no scratch in any of the 16 instances (KS x VEC x BLDS).  VGPRs and waves per SIMD by registers: KS = 0 (k = 0): 82-132, 3-5;
// KS = 4 (k <= 16): 183-198, 2; KS = 8 (k <= 32): 226-240, 2; KS = 16 (k > 32, workgroups of 4 waves): 256 + 74-88 accumulator registers, 1.  KS <= 8
// is launched as one workgroup of 8 waves per CU sharing the one LDS copy of the coefficients (131 KB + 4 KB of shifts at p = 500, k = 25): the 2 waves
// per SIMD the registers allow, so that one wave's MFMAs cover the other's wait for its loads.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "jch_internal.h"

typedef double oc_v2 __attribute__((ext_vector_type(2)));
typedef double oc_v4 __attribute__((ext_vector_type(4)));

#define OC_RT 2                     // row tiles of 32 per wave tile
#define OC_TR (32 * OC_RT)          // rows per wave tile
#define OC_LDS_MAX (150 * 1024)     // bytes of coefficients a workgroup may stage

struct oc_rows {   // where a lane's row pairs of one wave tile start: VEC reads [r0, r0 + 1] as one piece (r0 even, r0 + 1 < m)
    int64_t r0[OC_RT], r1[OC_RT];
};

template <int KS, bool VEC, bool BLDS, int NW>   // KS k-steps of 4 score columns per chunk (k <= 4 KS: one chunk, held in registers)
__global__ __launch_bounds__(64 * NW) void k_row_resid_ss(const double *__restrict__ X, int64_t m, int p, int64_t ldx, const double *__restrict__ Z, int k,
                                                           int64_t ldz, const double *__restrict__ Bt, int PB, int lrows, double *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double oc_lds[];   // BLDS: [lrows + 1][PB], row lrows = the shifts; zero beyond k and p
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double *bsrc = Bt;
    if constexpr (BLDS) {
        for (int e = tid; e < (lrows + 1) * PB; e += 64 * NW) oc_lds[e] = Bt[e];
        __syncthreads();
        bsrc = oc_lds;
    }
    const int kq = lane >> 4, cl = lane & 15;
    const int nct = (p + 15) / 16;
    const int64_t ntile = (m + OC_TR - 1) / OC_TR, tstep = (int64_t)gridDim.x * NW;
    int64_t tile = (int64_t)blockIdx.x * NW + wv;
    if (tile >= ntile) return;
    auto rows_of = [&](int64_t t) {
        oc_rows r;
#pragma unroll
        for (int rt = 0; rt < OC_RT; ++rt) {
            const int64_t i = t * OC_TR + 32 * rt + 2 * cl;
            if (VEC) { r.r0[rt] = std::min<int64_t>(i, m - 2); r.r1[rt] = r.r0[rt] + 1; }      // (m even: re-read the last pair)
            else { r.r0[rt] = std::min<int64_t>(i, m - 1); r.r1[rt] = std::min<int64_t>(i + 1, m - 1); }
        }
        return r;
    };
    // the lane's X values of column tile ct: rows (r0, r1) of columns 16 ct + kq + 4 reg, clamped to column p - 1
    auto loadx = [&](const oc_rows &r, int ct, oc_v2 (&x)[4][OC_RT]) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const size_t col = (size_t)min(16 * ct + kq + 4 * reg, p - 1) * (size_t)ldx;
#pragma unroll
            for (int rt = 0; rt < OC_RT; ++rt) {
                if (VEC) x[reg][rt] = __builtin_nontemporal_load(reinterpret_cast<const oc_v2 *>(X + col + r.r0[rt]));
                else x[reg][rt] = oc_v2{__builtin_nontemporal_load(X + col + r.r0[rt]), __builtin_nontemporal_load(X + col + r.r1[rt])};
            }
        }
    };
    // chunk kc of the lane's Z values: rows (r0, r1) of columns 4 KS kc + 4 ks + kq, clamped to column k - 1 (zero coefficients beyond k)
    auto loadz = [&](const oc_rows &r, int kc, oc_v2 (&z)[KS > 0 ? KS : 1][OC_RT]) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const size_t col = (size_t)min(4 * KS * kc + 4 * ks + kq, k - 1) * (size_t)ldz;
#pragma unroll
            for (int rt = 0; rt < OC_RT; ++rt) z[ks][rt] = oc_v2{Z[col + r.r0[rt]], Z[col + r.r1[rt]]};
        }
    };
    const int nchunk = KS > 0 ? lrows / (KS > 0 ? 4 * KS : 1) : 0;
    oc_rows cur = rows_of(tile);
    oc_v2 xa[4][OC_RT], xb[4][OC_RT];
    loadx(cur, 0, xa);
    for (; tile < ntile; tile += tstep) {
        const oc_rows nxt = rows_of(std::min<int64_t>(tile + tstep, ntile - 1));
        oc_v2 z[KS > 0 ? KS : 1][OC_RT];
        if (KS > 0 && nchunk == 1) loadz(cur, 0, z);
        double s[OC_RT][2];
#pragma unroll
        for (int rt = 0; rt < OC_RT; ++rt) s[rt][0] = s[rt][1] = 0.0;
        for (int ct = 0; ct < nct; ++ct) {
            const bool last = ct + 1 == nct;
            oc_rows pre;
#pragma unroll
            for (int rt = 0; rt < OC_RT; ++rt) { pre.r0[rt] = last ? nxt.r0[rt] : cur.r0[rt]; pre.r1[rt] = last ? nxt.r1[rt] : cur.r1[rt]; }
            loadx(pre, last ? 0 : ct + 1, xb);
            oc_v4 acc[OC_RT][2];
#pragma unroll
            for (int rt = 0; rt < OC_RT; ++rt) { acc[rt][0] = oc_v4{0.0, 0.0, 0.0, 0.0}; acc[rt][1] = oc_v4{0.0, 0.0, 0.0, 0.0}; }
            if constexpr (KS > 0) {
                for (int kc = 0; kc < nchunk; ++kc) {
                    if (nchunk > 1) loadz(cur, kc, z);
                    const double *bp = bsrc + (size_t)(4 * KS * kc + kq) * PB + 16 * ct + cl;
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        const double b = bp[(size_t)(4 * ks) * PB];
#pragma unroll
                        for (int rt = 0; rt < OC_RT; ++rt) {
                            acc[rt][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b, z[ks][rt].x, acc[rt][0], 0, 0, 0);
                            acc[rt][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(b, z[ks][rt].y, acc[rt][1], 0, 0, 0);
                        }
                    }
                }
            }
            // acc[rt][par][reg] of lane (kq, cl) = fit[row 32 rt + 2 cl + par][column 16 ct + kq + 4 reg]   (f64 16x16x4: D[kq + 4 reg][cl])
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int j = 16 * ct + kq + 4 * reg;
                const double sh = bsrc[(size_t)lrows * PB + j];
                const bool live = j < p;
#pragma unroll
                for (int rt = 0; rt < OC_RT; ++rt) {
                    const double e0 = (xa[reg][rt].x - sh) - acc[rt][0][reg], e1 = (xa[reg][rt].y - sh) - acc[rt][1][reg];
                    const double f0 = live ? e0 : 0.0, f1 = live ? e1 : 0.0;
                    s[rt][0] = __builtin_fma(f0, f0, s[rt][0]);
                    s[rt][1] = __builtin_fma(f1, f1, s[rt][1]);
                }
            }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
#pragma unroll
                for (int rt = 0; rt < OC_RT; ++rt) xa[reg][rt] = xb[reg][rt];
        }
#pragma unroll
        for (int rt = 0; rt < OC_RT; ++rt)
#pragma unroll
            for (int par = 0; par < 2; ++par) {
                const double v = s[rt][par];
                const double t = (__shfl(v, cl, 64) + __shfl(v, 16 + cl, 64)) + (__shfl(v, 32 + cl, 64) + __shfl(v, 48 + cl, 64));
                const int64_t i = tile * OC_TR + 32 * rt + 2 * cl + par;
                if (kq == 0 && i < m) out[i] = t;
            }
        cur = nxt;
    }
}

// Bt: device [lrows + 1][PB] (row l < k: B[., l]; rows k .. lrows - 1 zero; row lrows: the shifts; columns >= p zero), PB = p rounded up to 16
static int32_t oc_launch(jch_ctx *ctx, const double *X, int64_t m, int p, int64_t ldx, const double *Z, int k, int64_t ldz, const double *Bt, int ks,
                         int lrows, int PB, double *out)
{
    const bool vec = m % 2 == 0 && ldx % 2 == 0 && (((uintptr_t)X) & 15) == 0;
    const size_t lds = sizeof(double) * (size_t)(lrows + 1) * (size_t)PB;
    const bool blds = lds <= OC_LDS_MAX;
    const int nw = ks <= 8 ? 8 : 4;
    // two waves per SIMD, so that one wave's MFMAs cover the other's wait for its loads (gemm.hip, k_affine_gemm32p)
    const int wpc = 8;
    const int bpc = std::max(1, blds ? std::min((int)((158 * 1024) / lds), wpc / nw) : wpc / nw);
    const int64_t ntile = (m + OC_TR - 1) / OC_TR;
    const unsigned nb = (unsigned)std::min<int64_t>((ntile + nw - 1) / nw, (int64_t)ctx->cus * bpc);
#define JCH_OC(KS, VEC, BLDS, NW) do { \
        static jch_per_device_once once_; \
        if (BLDS && !once_.done(ctx->device)) { JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_row_resid_ss<KS, VEC, BLDS, NW>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); once_.mark(ctx->device); } \
        hipLaunchKernelGGL((k_row_resid_ss<KS, VEC, BLDS, NW>), dim3(nb), dim3(64 * NW), BLDS ? lds : 0, ctx->stream, X, m, p, ldx, Z, k, ldz, Bt, PB, lrows, out); } while (0)
#define JCH_OC2(KS, NW) do { if (vec) { if (blds) JCH_OC(KS, true, true, NW); else JCH_OC(KS, true, false, NW); } \
                             else { if (blds) JCH_OC(KS, false, true, NW); else JCH_OC(KS, false, false, NW); } } while (0)
    if (ks == 0) JCH_OC2(0, 8); else if (ks == 4) JCH_OC2(4, 8); else if (ks == 8) JCH_OC2(8, 8); else JCH_OC2(16, 4);
#undef JCH_OC2
#undef JCH_OC
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

extern "C" int32_t jch_row_resid_ss(jch_ctx *ctx, int32_t loc, const double *X, int64_t m, int64_t p, int64_t ldx, const double *shift, const double *Z,
                                    int64_t k, int64_t ldz, const double *B, int64_t ldb, double *out)
{
    if (!ctx) return JCH_EINVAL;
    if (!X || !out || m < 0 || p < 1 || p > (1 << 30) || k < 0 || k > (1 << 20) || ldx < m) return jch_fail(ctx, JCH_EINVAL, "jch_row_resid_ss: bad arguments");
    if (k > 0 && (!Z || !B || ldz < m || ldb < p)) return jch_fail(ctx, JCH_EINVAL, "jch_row_resid_ss: k > 0 needs Z (ldz >= m) and B (ldb >= p)");
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "jch_row_resid_ss: bad loc");
    if (m == 0) return JCH_OK;
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const int ks = k == 0 ? 0 : k <= 16 ? 4 : k <= 32 ? 8 : 16;
    const int lrows = ks == 0 ? 0 : (int)((k + 4 * ks - 1) / (4 * ks)) * 4 * ks;
    const int PB = (int)((p + 15) / 16 * 16);
    std::vector<double> hb((size_t)(lrows + 1) * PB, 0.0);
    for (int64_t l = 0; l < k; ++l)
        for (int64_t j = 0; j < p; ++j) hb[(size_t)l * PB + j] = B[j + l * ldb];
    if (shift) for (int64_t j = 0; j < p; ++j) hb[(size_t)lrows * PB + j] = shift[j];
    JCH_TRY(jch_reserve(ctx, ctx->gemm_b, sizeof(double) * hb.size()));
    if (loc == JCH_LOC_HOST) {   // jch_transform's staging: X into xq, then Z and the result side by side in gemm_out
        JCH_TRY(jch_reserve(ctx, ctx->xq, sizeof(double) * (size_t)m * p));
        JCH_TRY(jch_reserve(ctx, ctx->gemm_out, sizeof(double) * (size_t)m * (size_t)(k + 1)));
    }
    double *dB = (double *)ctx->gemm_b.ptr;
    return jch_synced(ctx, true, [&]() -> int32_t {
        JCH_HIP(ctx, hipMemcpyAsync(dB, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice, ctx->stream));
        const double *dX = X, *dZ = Z;
        double *dO = out;
        int64_t ldxd = ldx, ldzd = ldz;
        if (loc == JCH_LOC_HOST) {
            JCH_TRY(jch_stage_in(ctx, true, (double *)ctx->xq.ptr, m, p, &dX, &ldxd));
            if (k > 0) JCH_TRY(jch_stage_in(ctx, true, (double *)ctx->gemm_out.ptr, m, k, &dZ, &ldzd));
            else { dZ = (const double *)ctx->gemm_out.ptr; ldzd = m; }
            dO = (double *)ctx->gemm_out.ptr + (size_t)m * k;
        }
        JCH_TRY(oc_launch(ctx, dX, m, (int)p, ldxd, dZ, (int)k, ldzd, dB, ks, lrows, PB, dO));
        if (loc == JCH_LOC_HOST) JCH_HIP(ctx, hipMemcpyAsync(out, dO, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    });
}
