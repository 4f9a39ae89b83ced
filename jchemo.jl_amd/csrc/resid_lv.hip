// Nested row sums of squared residuals: every level a_lo..a_hi of a rank-a model in ONE read of X (a_hi <= 32; see `chunks`) — the device primitive behind the Shenk
// weights of `wshenk` / `plsravg` (src/wshenk.jl, src/plsravg_shenk.jl) — jch_row_resid_ss_lv, include/jchemo_hip.h; DESIGN.md §27.
//
//   out[i + (a - a_lo) ldo] = sum_j ( X[i, j] - shift[j] - sum_{l < a} Z[i, l] B[j, l] )^2,   a = a_lo .. a_hi
//
// The residual after a latent variables is the residual after a - 1 minus ONE rank-one term, so a lane that walks the levels in order gets all of
// them from one value of X: e_0 = x - shift, e_a = fma(-z_a, b_a, e_(a-1)), s_a = fma(e_a, e_a, s_a).  The direct form (subtract, then square) is
// kept: the expanded |x|^2 - 2 t'g + t'G t loses exactly the digits the weights 1 / rss are made of (occ.hip says the same of x U - mu U).
//
//   k_row_resid_lv  rowprep.hip's layout: one lane owns one row, so a wave reads one 512-byte run of a column, holds its row's scores z and the
//                   running sums s of a chunk of LC levels in registers, and owns every sum from its first term to its last: no cross-lane
//                   reduction, no atomics, one fixed order (columns ascending), and a NaN at X[i, j] or Z[i, l] never leaves lane i.  The levels
//                   run on the vector pipe (MFMA could add only 4 levels at a time and the f64 peaks are equal).  Per column the coefficients
//                   Bt[j][0] = shift[j], Bt[j][1 + l] = B[j, l] are wave-uniform: plain const __restrict__ loads at a uniform address, which the
//                   compiler keeps in scalar registers and hands to v_fma_f64 directly.  They are taken in stages of RL_G levels, the next
//                   stage's fetched while this one is worked on; more than two stages' worth does not fit in the scalar file.  RL_U columns
//                   of X are in flight per lane: a register ring refilled one column per step, the column loop unrolled by RL_U.
//   chunks          levels beyond the LC a lane holds are walked by further launches, each of which reads X again: chunk c covers levels c LC + 1 .. (c + 1) LC and first replays
//                   the c LC rank-one terms before it, in the same order, with z re-read from memory per column.  The fma chain of a level is the
//                   same whatever the chunking, hence the same bits.  Slower, never absent.
//   Rows >= m shadow row m - 1 and store nothing; columns >= p and score columns >= a_hi are never read (Bt is zero padded to whole chunks).
//   Every load is 8 bytes wide: alignment and leading dimensions cannot change a bit.
// gfx950, hipcc -O3, no scratch in any of the four instances.  VGPRs / waves per SIMD: LC = 8: 60 / 8; LC = 16: 92 / 5; LC = 32: 157 / 3;
// LC = 32 behind the first chunk (REPLAY): 247 / 2.  LC = 32 parks 48 scalar values in VGPR lanes, all outside the column loop (the z / store
// predicates); the REPLAY instance parks 578, some inside it: that is the slower path of a_hi > 32.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "jch_internal.h"

#define RL_NT 256   // rows per workgroup
#define RL_U 8      // columns of X loaded ahead per lane
#define RL_G 8    // levels per stage: the coefficients of two stages fit in the scalar registers

template <int LC, bool REPLAY>   // REPLAY: a chunk behind the first (l0 > 0)
__global__ __launch_bounds__(RL_NT) void k_row_resid_lv(const double *__restrict__ X, int64_t m, int p, int64_t ldx, const double *__restrict__ Z, int64_t ldz,
                                                        const double *__restrict__ Bt, int LD, int l0arg, int a_lo, int a_hi, double *__restrict__ out,
                                                        int64_t ldo)
{
    constexpr int G = LC < RL_G ? LC : RL_G, H = LC / G;   // a column's LC levels go in H stages of G
    const int l0 = REPLAY ? l0arg : 0;
    int64_t i = (int64_t)blockIdx.x * RL_NT + threadIdx.x;
    const bool live = i < m;
    if (!live) i = m - 1;                       // (idle lanes of the last workgroup shadow the last row and store nothing)
    const double *x = X + i;
    const double *zr = Z + i;                   // (never dereferenced when a_hi == 0)
    double z[LC], s[LC];
#pragma unroll
    for (int l = 0; l < LC; ++l) {
        z[l] = l0 + l < a_hi ? zr[(size_t)(l0 + l) * (size_t)ldz] : 0.0;
        s[l] = 0.0;
    }
    double s0 = 0.0;
    // RL_U columns of the lane's row are in flight: xr[u] holds column j with j % RL_U == u and is refilled with column j + RL_U as soon as it has
    // been taken (columns past p - 1 re-read column p - 1, unused).  The column loop is unrolled by RL_U so that u is a constant.
    double xr[RL_U];
#pragma unroll
    for (int u = 0; u < RL_U; ++u) xr[u] = __builtin_nontemporal_load(x + (size_t)min(u, p - 1) * (size_t)ldx);
    // the coefficients are wave-uniform and live in scalar registers: stage (j, h) computes with bc while bn is fetched for the stage after it
    const double *bj = Bt + 1 + l0;
    double bc[G], bn[G], shc = Bt[0], shn;
#pragma unroll
    for (int g = 0; g < G; ++g) bc[g] = bj[g];
    auto column = [&](double xv, int j) {
        const double *bnext = Bt + (size_t)min(j + 1, p - 1) * (size_t)LD + 1 + l0;
        double e = xv - shc;
        s0 = __builtin_fma(e, e, s0);
        if constexpr (REPLAY)
            for (int l = 0; l < l0; ++l) e = __builtin_fma(-zr[(size_t)l * (size_t)ldz], bj[l - l0], e);   // (the chunks before this one, replayed)
#pragma unroll
        for (int h = 0; h < H; ++h) {
            const double *bsrc = h + 1 < H ? bj + (h + 1) * G : bnext;
#pragma unroll
            for (int g = 0; g < G; ++g) bn[g] = bsrc[g];
            if (h + 1 == H) shn = bnext[-1 - l0];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                e = __builtin_fma(-z[h * G + g], bc[g], e);
                s[h * G + g] = __builtin_fma(e, e, s[h * G + g]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < G; ++g) bc[g] = bn[g];
        }
        shc = shn;
        bj = bnext;
    };
    int j0 = 0;
    for (; j0 + RL_U <= p; j0 += RL_U) {
#pragma unroll
        for (int u = 0; u < RL_U; ++u) {
            const double xv = xr[u];
            xr[u] = __builtin_nontemporal_load(x + (size_t)min(j0 + u + RL_U, p - 1) * (size_t)ldx);
            column(xv, j0 + u);
        }
    }
#pragma unroll
    for (int u = 0; u < RL_U; ++u)
        if (j0 + u < p) column(xr[u], j0 + u);
    if (!live) return;
    if (l0 == 0 && a_lo == 0) out[i] = s0;
#pragma unroll
    for (int l = 0; l < LC; ++l) {
        const int a = l0 + l + 1;
        if (a >= a_lo && a <= a_hi) out[i + (size_t)(a - a_lo) * (size_t)ldo] = s[l];
    }
}

// Bt: device [p][LD], LD = 1 + nchunk lc.  One launch per chunk of lc levels (a_hi = 0: one launch, level 0 alone).
static int32_t rl_launch(jch_ctx *ctx, const double *X, int64_t m, int p, int64_t ldx, const double *Z, int64_t ldz, const double *Bt, int LD, int lc,
                         int a_lo, int a_hi, double *out, int64_t ldo)
{
    const unsigned nb = (unsigned)((m + RL_NT - 1) / RL_NT);
    for (int l0 = 0; l0 == 0 || l0 < a_hi; l0 += lc) {
        if (l0 + lc < a_lo) continue;           // (no level of this chunk is asked for)
#define JCH_RL(LC, REPLAY) hipLaunchKernelGGL((k_row_resid_lv<LC, REPLAY>), dim3(nb), dim3(RL_NT), 0, ctx->stream, X, m, p, ldx, Z, ldz, Bt, LD, l0, a_lo, a_hi, out, ldo)
        if (lc == 8) JCH_RL(8, false);          // (8 and 16 levels are one chunk by construction)
        else if (lc == 16) JCH_RL(16, false);
        else if (l0 == 0) JCH_RL(32, false);
        else JCH_RL(32, true);
#undef JCH_RL
        JCH_HIP(ctx, hipGetLastError());
    }
    return JCH_OK;
}

extern "C" int32_t jch_row_resid_ss_lv(jch_ctx *ctx, int32_t loc, const double *X, int64_t m, int64_t p, int64_t ldx, const double *shift, const double *Z,
                                       int64_t kz, int64_t ldz, const double *B, int64_t ldb, int32_t a_lo, int32_t a_hi, double *out, int64_t ldo)
{
    if (!ctx) return JCH_EINVAL;
    if (!X || !out || m < 0 || p < 1 || p > (1 << 30) || kz < 0 || kz > (1 << 20) || ldx < m || ldo < m)
        return jch_fail(ctx, JCH_EINVAL, "jch_row_resid_ss_lv: bad arguments");
    if (a_lo < 0 || a_lo > a_hi || a_hi > kz) return jch_fail(ctx, JCH_EINVAL, "jch_row_resid_ss_lv: needs 0 <= a_lo <= a_hi <= kz");
    if (a_hi > 0 && (!Z || !B || ldz < m || ldb < p)) return jch_fail(ctx, JCH_EINVAL, "jch_row_resid_ss_lv: a_hi > 0 needs Z (ldz >= m) and B (ldb >= p)");
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "jch_row_resid_ss_lv: bad loc");
    if (m == 0) return JCH_OK;
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const int lc = a_hi <= 8 ? 8 : a_hi <= 16 ? 16 : 32;
    const int LD = 1 + std::max(1, (a_hi + lc - 1) / lc) * lc;
    const int64_t le = (int64_t)a_hi - a_lo + 1;
    std::vector<double> hb((size_t)p * LD, 0.0);
    for (int64_t j = 0; j < p; ++j) {
        if (shift) hb[(size_t)j * LD] = shift[j];
        for (int64_t l = 0; l < a_hi; ++l) hb[(size_t)j * LD + 1 + l] = B[j + l * ldb];
    }
    JCH_TRY(jch_reserve(ctx, ctx->gemm_b, sizeof(double) * hb.size()));
    if (loc == JCH_LOC_HOST) {   // jch_row_resid_ss's staging: X into xq, then the a_hi score columns and the result side by side in gemm_out
        JCH_TRY(jch_reserve(ctx, ctx->xq, sizeof(double) * (size_t)m * p));
        JCH_TRY(jch_reserve(ctx, ctx->gemm_out, sizeof(double) * (size_t)m * (size_t)(a_hi + le)));
    }
    double *dB = (double *)ctx->gemm_b.ptr;
    return jch_synced(ctx, true, [&]() -> int32_t {
        JCH_HIP(ctx, hipMemcpyAsync(dB, hb.data(), sizeof(double) * hb.size(), hipMemcpyHostToDevice, ctx->stream));
        const double *dX = X, *dZ = Z;
        double *dO = out;
        int64_t ldxd = ldx, ldzd = ldz, ldod = ldo;
        if (loc == JCH_LOC_HOST) {
            JCH_TRY(jch_stage_in(ctx, true, (double *)ctx->xq.ptr, m, p, &dX, &ldxd));
            if (a_hi > 0) JCH_TRY(jch_stage_in(ctx, true, (double *)ctx->gemm_out.ptr, m, a_hi, &dZ, &ldzd));
            dO = (double *)ctx->gemm_out.ptr + (size_t)m * a_hi;
            ldod = m;
        }
        if (a_hi == 0) { dZ = dX; ldzd = ldxd; }   // (a valid address for the kernel's row pointer; never read)
        JCH_TRY(rl_launch(ctx, dX, m, (int)p, ldxd, dZ, ldzd, dB, LD, lc, a_lo, a_hi, dO, ldod));
        if (loc == JCH_LOC_HOST) JCH_TRY(jch_copy2d(ctx, out, ldo, dO, m, m, le, hipMemcpyDeviceToHost));
        return JCH_OK;
    });
}
