// Blocked Cholesky factorisation of a symmetric positive definite matrix on the f64 matrix cores, the two triangular solves with the
// factor and |L^-1|_F^2: the dense direct solver under jch_krr_solve (krr.hip).  jch_chol_factor / jch_chol_solve /
// jch_chol_inv_fro2 of include/jchemo_hip.h.
//
// A = L L' (lower triangle, column-major, in place, right-looking, block width CH_NB = 128).  Per block column k:
//   k_chol_diag       one workgroup: the NB x NB diagonal block factored in LDS (128 KB), L_kk written back, inv(L_kk) computed in
//                     place in LDS and kept in ctx->chol_inv (n x NB doubles, zero above the diagonal and in the padding)
//   k_chol_tile<0>    the panel below: L_ik = A_ik inv(L_kk)' as a product (in place: a workgroup owns whole rows of the panel)
//   k_chol_tile<1>    the trailing update A_ij -= L_ik L_jk' for the 128 x 128 tiles on or below the diagonal (~all of the n^3/3 flop)
// k_chol_tile is k_gram's tile scheme (kgram.hip): 128 x 128 output tile per workgroup of 4 waves, 4 x 4 v_mfma_f64_16x16x4_f64 tiles
// per wave, 16-column chunks of both operands through LDS, double-buffered, two workgroups per CU; the operands are read where they
// lie (a k-column of a tile is contiguous in a column-major panel), with scalar loads and zero fill at the edges, so any n and lda.
// Only the lower triangle of A is read or written.  A pivot that is not > 0 (negative, zero, NaN) writes its 1-based column into
// the device info word once; every later kernel of the call returns on seeing it.  No host round trip, no kernel waits on another,
// no floating-point atomics: every output element is one thread's fixed-order sum.
//
// Solves (B n x q in place), block column by block column with the kept inverses: forward Y_k = inv(L_kk) B_k, rows below
// -= L_ik Y_k; backward B_k -= L_ik' X_i (column dots, one workgroup per column of L, fixed tree), X_k = inv(L_kk)' B_k.  L is
// read once per direction and per 8 columns of B.
// |L^-1|_F^2: W = L^-T (upper triangle of an n x n workspace) from X L' = I by the same forward substitution on block rows of the
// identity: W[:, k] = W[:, k] inv(L_kk)' (k_chol_tile<0>), W[:, i] -= W[:, k] L_ik' for i > k (k_chol_tile<2>); the rows below block k
// are known zeros and are never touched, so the cost is n^3/3 flop in products of inner dimension NB.  jch_launch_chol_inv_t writes W
// into any n x n buffer (ld ldw): ctx->chol_w here, the caller's Uinv for jch_gauss_factor (gda.hip).  Of jch_chol_inv_fro2 only the sum
// of squares leaves the device (block partials, then one workgroup, fixed order).
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "jch_internal.h"
#include "tile128_dev.h"

#define CH_NB T128_T // block width of the factorisation = tile edge
#define CH_QC 8      // columns of B per workgroup of the solve kernels
#define CH_SUMSQ_WG 1024

// two consecutive rows r, r + 1 of column k of a column-major panel; zero beyond nvalid rows / kdim columns
__device__ __forceinline__ t128_v2d ch_ld2(const double *P, int64_t ld, int64_t r, int64_t nvalid, int k, int kdim, bool vec)
{
    t128_v2d v{0.0, 0.0};
    if (k >= kdim) return v;
    const double *c = P + (size_t)k * (size_t)ld;
    if (vec && r + 1 < nvalid) return *reinterpret_cast<const t128_v2d *>(c + r);
    if (r < nvalid) v.x = c[r];
    if (r + 1 < nvalid) v.y = c[r + 1];
    return v;
}

// C[i, j] (i < nrow, j < ncol) op sum_{t < kdim} R[i, t] Q[j, t]   (R, Q, C column-major).
// MODE 0: C = (C may be R when ncol <= 128: every load of a workgroup's rows is done before its first store);
// MODE 1: C -=, symmetric (R == Q): tiles ti >= tj only, and i >= j only on the diagonal tiles; MODE 2: C -=, all tiles.
template <int MODE>
__global__ __launch_bounds__(256, 2) void k_chol_tile(const double *R, int64_t ldr, int64_t nrow, bool vr, const double *Q, int64_t ldq, int64_t ncol,
                                                      bool vq, int kdim, double *C, int64_t ldc, int tiles_i, const int *__restrict__ info)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    if (*info != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t ti, tj;
    if (MODE == 1) {
        t128_tri(blockIdx.x, tj, ti);   // tj <= ti
    } else {
        ti = blockIdx.x % tiles_i; tj = blockIdx.x / tiles_i;
    }
    const int64_t i0 = ti * CH_NB, j0 = tj * CH_NB;
    const int qj = wv >> 1, qi = wv & 1;
    t128_v4d acc[4][4];   // A = Q tile (output columns j: the MFMA's rows), B = R tile (output rows i: the MFMA's columns, the contiguous direction)
    t128_mma(
        lds, (kdim + T128_KB - 1) / T128_KB,
        [&](int k, int c) { return ch_ld2(Q, ldq, j0 + c, ncol, k, kdim, vq); },
        [&](int k, int c) { return ch_ld2(R, ldr, i0 + c, nrow, k, kdim, vr); },
        acc);
    // acc[mj][ni][reg] = sum_t Q[j, t] R[i, t], j = j0 + 64 qj + 16 mj + (lane >> 4) + 4 reg, i = i0 + 64 qi + 16 ni + (lane & 15):
    // every load / store instruction touches 128-byte pieces of columns of C
#pragma unroll
    for (int mj = 0; mj < 4; ++mj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t j = j0 + 64 * qj + 16 * mj + (lane >> 4) + 4 * reg;
            if (j >= ncol) continue;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int64_t i = i0 + 64 * qi + 16 * ni + (lane & 15);
                if (i >= nrow || (MODE == 1 && ti == tj && i < j)) continue;
                double *c = C + (size_t)i + (size_t)j * (size_t)ldc;
                if (MODE == 0) *c = acc[mj][ni][reg];
                else *c = *c - acc[mj][ni][reg];
            }
        }
}

// The diagonal block: Akk (nb x nb, nb <= 128, lower triangle) -> L_kk in place, inv(L_kk) to inv (128 x 128, ld 128, zero elsewhere).
// S lives in LDS column-major with ld 128 (thread = row: conflict-free); the Cholesky is the right-looking column sweep, the
// inverse the in-place column recurrence X[r, j] = -(sum_{j < k <= r} X[r, k] L[k, j]) / L[j, j] from the last column to the first.
__global__ __launch_bounds__(256) void k_chol_diag(double *Akk, int64_t lda, int nb, int64_t k0, double *__restrict__ inv, int *info)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *S = lds, *tmp = lds + CH_NB * CH_NB, *red = tmp + CH_NB;
    if (*info != 0) return;
    const int tid = threadIdx.x, r = tid & (CH_NB - 1), half = tid >> 7;
    for (int e = tid; e < nb * CH_NB; e += 256) {
        const int rr = e & (CH_NB - 1), c = e >> 7;
        if (rr < nb) S[e] = rr >= c ? Akk[(size_t)rr + (size_t)c * (size_t)lda] : 0.0;
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j) {
        const double d = S[j + CH_NB * j];
        if (!(d > 0.0)) {   // the same value in every thread: the whole workgroup leaves
            if (tid == 0) atomicCAS(info, 0, (int)(k0 + j + 1));
            return;
        }
        const double sd = sqrt(d);
        if (tid > j && tid < nb) S[tid + CH_NB * j] /= sd;
        __syncthreads();
        if (tid == j) S[j + CH_NB * j] = sd;
        if (r > j && r < nb) {
            const double lr = S[r + CH_NB * j];
            for (int c = j + 1 + half; c <= r; c += 2) S[r + CH_NB * c] = fma(-lr, S[c + CH_NB * j], S[r + CH_NB * c]);
        }
        __syncthreads();
    }
    for (int e = tid; e < nb * CH_NB; e += 256) {
        const int rr = e & (CH_NB - 1), c = e >> 7;
        if (rr < nb && rr >= c) Akk[(size_t)rr + (size_t)c * (size_t)lda] = S[e];
    }
    for (int j = nb - 1; j >= 0; --j) {
        const double djj = S[j + CH_NB * j];
        if (tid > j && tid < nb) tmp[tid] = S[tid + CH_NB * j];
        __syncthreads();
        double s = 0.0;
        if (r > j && r < nb)
            for (int k = j + 1 + half; k <= r; k += 2) s = fma(S[r + CH_NB * k], tmp[k], s);
        red[tid] = s;
        __syncthreads();
        if (half == 0) {
            if (r > j && r < nb) S[r + CH_NB * j] = -(red[r] + red[r + CH_NB]) / djj;
            else if (r == j) S[j + CH_NB * j] = 1.0 / djj;
        }
        __syncthreads();
    }
    for (int e = tid; e < CH_NB * CH_NB; e += 256) {
        const int rr = e & (CH_NB - 1), c = e >> 7;
        inv[e] = (rr < nb && c < nb && rr >= c) ? S[e] : 0.0;
    }
}

// ---- the solves.  Bk: the kb rows of B of block column k; inv: inv(L_kk) (128 x 128, zero-padded)
// Bk = inv Bk (TRANS: inv' Bk); workgroup = 8 columns of B, thread = row
template <bool TRANS>
__global__ __launch_bounds__(CH_NB) void k_chol_sdiag(const double *__restrict__ inv, int kb, double *Bk, int64_t ldb, int64_t q, const int *__restrict__ info)
{
    __shared__ double Ys[CH_NB * CH_QC];
    if (*info != 0) return;
    const int r = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * CH_QC;
#pragma unroll
    for (int c = 0; c < CH_QC; ++c) Ys[r * CH_QC + c] = (r < kb && c0 + c < q) ? Bk[(size_t)r + (size_t)(c0 + c) * (size_t)ldb] : 0.0;
    __syncthreads();
    double acc[CH_QC];
#pragma unroll
    for (int c = 0; c < CH_QC; ++c) acc[c] = 0.0;
    if (!TRANS) {
        for (int t = 0; t <= r; ++t) {
            const double v = inv[r + CH_NB * t];
#pragma unroll
            for (int c = 0; c < CH_QC; ++c) acc[c] = fma(v, Ys[t * CH_QC + c], acc[c]);
        }
    } else {
        for (int t = r; t < kb; ++t) {
            const double v = inv[t + CH_NB * r];
#pragma unroll
            for (int c = 0; c < CH_QC; ++c) acc[c] = fma(v, Ys[t * CH_QC + c], acc[c]);
        }
    }
    if (r < kb)
#pragma unroll
        for (int c = 0; c < CH_QC; ++c)
            if (c0 + c < q) Bk[(size_t)r + (size_t)(c0 + c) * (size_t)ldb] = acc[c];
}

// forward: B[i, :] -= sum_t Lp[i, t] Yk[t, :] for the `rows` rows below block column k (Lp = L[k0 + 128.., k0..], Yk = B[k0.., :], Bp = B[k0 + 128.., :])
__global__ __launch_bounds__(256) void k_chol_fwd(const double *__restrict__ Lp, int64_t ldl, int64_t rows, const double *Yk, double *Bp, int64_t ldb,
                                                  int64_t q, const int *__restrict__ info)
{
    __shared__ double Ys[CH_NB * CH_QC];
    if (*info != 0) return;
    const int64_t c0 = (int64_t)blockIdx.y * CH_QC;
    for (int e = threadIdx.x; e < CH_NB * CH_QC; e += 256) {
        const int t = e / CH_QC, c = e - t * CH_QC;
        Ys[e] = c0 + c < q ? Yk[(size_t)t + (size_t)(c0 + c) * (size_t)ldb] : 0.0;
    }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    double acc[CH_QC];
#pragma unroll
    for (int c = 0; c < CH_QC; ++c) acc[c] = 0.0;
#pragma unroll 4
    for (int t = 0; t < CH_NB; ++t) {
        const double l = Lp[(size_t)i + (size_t)t * (size_t)ldl];
#pragma unroll
        for (int c = 0; c < CH_QC; ++c) acc[c] = fma(l, Ys[t * CH_QC + c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < CH_QC; ++c)
        if (c0 + c < q) Bp[(size_t)i + (size_t)(c0 + c) * (size_t)ldb] -= acc[c];
}

// backward: Bk[t, :] -= sum_i Lp[i, t] Bp[i, :] over the `rows` rows below; workgroup (column t of L, 8 columns of B)
__global__ __launch_bounds__(256) void k_chol_bwd(const double *__restrict__ Lp, int64_t ldl, int64_t rows, double *Bk, const double *Bp, int64_t ldb,
                                                  int64_t q, const int *__restrict__ info)
{
    __shared__ double scr[4];
    if (*info != 0) return;
    const int t = blockIdx.x;
    const int64_t c0 = (int64_t)blockIdx.y * CH_QC;
    const double *col = Lp + (size_t)t * (size_t)ldl;
    double acc[CH_QC];
#pragma unroll
    for (int c = 0; c < CH_QC; ++c) acc[c] = 0.0;
    for (int64_t i = threadIdx.x; i < rows; i += 256) {
        const double l = col[i];
#pragma unroll
        for (int c = 0; c < CH_QC; ++c)
            if (c0 + c < q) acc[c] = fma(l, Bp[(size_t)i + (size_t)(c0 + c) * (size_t)ldb], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < CH_QC; ++c) {
        const double s = jch_block_sum<256>(acc[c], scr);
        if (threadIdx.x == 0 && c0 + c < q) Bk[(size_t)t + (size_t)(c0 + c) * (size_t)ldb] -= s;
    }
}

// ---- |L^-1|_F^2
__global__ __launch_bounds__(256) void k_chol_eye(double *W, int64_t n, int64_t ldw)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) W[(size_t)i * (size_t)(ldw + 1)] = 1.0;
}
__global__ __launch_bounds__(256) void k_chol_sumsq(const double *__restrict__ W, int64_t tot, double *__restrict__ part, const int *__restrict__ info)
{
    __shared__ double scr[4];
    if (*info != 0) return;
    double s = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) s = fma(W[e], W[e], s);
    s = jch_block_sum<256>(s, scr);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void k_chol_sum1(const double *__restrict__ part, int np, double *__restrict__ out, const int *__restrict__ info)
{
    __shared__ double scr[4];
    if (*info != 0) return;
    double s = 0.0;
    for (int e = threadIdx.x; e < np; e += 256) s += part[e];
    s = jch_block_sum<256>(s, scr);
    if (threadIdx.x == 0) *out = s;
}

namespace {

constexpr size_t CH_DIAG_LDS = sizeof(double) * (CH_NB * CH_NB + CH_NB + 256);      // 134 144 B

bool ch_vec(const double *P, int64_t ld) { return ((uintptr_t)P % 16) == 0 && (ld % 2) == 0; }

int32_t ch_attrs(jch_ctx *ctx)
{
    static jch_per_device_once attr;
    if (!attr.done(ctx->device)) {
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_chol_tile<0>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_chol_tile<1>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_chol_tile<2>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_chol_diag, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr.mark(ctx->device);
    }
    return JCH_OK;
}

template <int MODE>
int32_t launch_tile(jch_ctx *ctx, const double *R, int64_t ldr, int64_t nrow, const double *Q, int64_t ldq, int64_t ncol, int kdim, double *C,
                    int64_t ldc, const int *info)
{
    if (nrow < 1 || ncol < 1 || kdim < 1) return JCH_OK;
    const int64_t ti = (nrow + CH_NB - 1) / CH_NB, tj = (ncol + CH_NB - 1) / CH_NB;
    const int64_t nblocks = MODE == 1 ? ti * (ti + 1) / 2 : ti * tj;
    if (nblocks > 0x7fffffffLL) return jch_fail(ctx, JCH_EINVAL, "cholesky: shape too large (%lld x %lld tiles)", (long long)ti, (long long)tj);
    hipLaunchKernelGGL(k_chol_tile<MODE>, dim3((unsigned)nblocks), dim3(256), T128_LDS_BYTES, ctx->stream, R, ldr, nrow, ch_vec(R, ldr), Q, ldq, ncol,
                       ch_vec(Q, ldq), kdim, C, ldc, (int)ti, info);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

}  // namespace

int32_t jch_chol_info_word(jch_ctx *ctx, int **info_dev)
{
    JCH_TRY(jch_reserve(ctx, ctx->chol_s, 256 + sizeof(double) * (CH_SUMSQ_WG + 8)));
    *info_dev = (int *)ctx->chol_s.ptr;
    return JCH_OK;
}

int32_t jch_launch_chol_factor(jch_ctx *ctx, double *A, int64_t n, int64_t lda, int *info)
{
    ctx->chol_L = nullptr;
    const int64_t nblk = (n + CH_NB - 1) / CH_NB;
    JCH_TRY(jch_reserve(ctx, ctx->chol_inv, sizeof(double) * (size_t)nblk * CH_NB * CH_NB));
    JCH_TRY(ch_attrs(ctx));
    double *inv = (double *)ctx->chol_inv.ptr;
    JCH_HIP(ctx, hipMemsetAsync(info, 0, sizeof(int), ctx->stream));
    for (int64_t k = 0; k < nblk; ++k) {
        const int64_t k0 = k * CH_NB, below = n - k0 - CH_NB;
        const int kb = (int)std::min<int64_t>(CH_NB, n - k0);
        double *Akk = A + (size_t)k0 + (size_t)k0 * (size_t)lda, *ik = inv + (size_t)k * CH_NB * CH_NB;
        hipLaunchKernelGGL(k_chol_diag, dim3(1), dim3(256), CH_DIAG_LDS, ctx->stream, Akk, lda, kb, k0, ik, info);
        JCH_HIP(ctx, hipGetLastError());
        if (below < 1) break;
        double *P = Akk + CH_NB;   // the panel below the diagonal block
        JCH_TRY(launch_tile<0>(ctx, P, lda, below, ik, CH_NB, CH_NB, CH_NB, P, lda, info));
        JCH_TRY(launch_tile<1>(ctx, P, lda, below, P, lda, below, CH_NB, P + (size_t)CH_NB * (size_t)lda, lda, info));
    }
    ctx->chol_L = A; ctx->chol_n = n; ctx->chol_ld = lda;
    return JCH_OK;
}

int32_t jch_launch_chol_solve(jch_ctx *ctx, const double *L, int64_t n, int64_t ldl, double *B, int64_t q, int64_t ldb, const int *info)
{
    if (ctx->chol_L != L || ctx->chol_n != n || ctx->chol_ld != ldl)
        return jch_fail(ctx, JCH_EINVAL, "jch_chol_solve: L is not the factor the last jch_chol_factor of this ctx produced");
    const int64_t nblk = (n + CH_NB - 1) / CH_NB;
    const double *inv = (const double *)ctx->chol_inv.ptr;
    const unsigned qg = (unsigned)((q + CH_QC - 1) / CH_QC);
    for (int64_t k = 0; k < nblk; ++k) {   // L Y = B
        const int64_t k0 = k * CH_NB, below = n - k0 - CH_NB;
        const int kb = (int)std::min<int64_t>(CH_NB, n - k0);
        hipLaunchKernelGGL(k_chol_sdiag<false>, dim3(qg), dim3(CH_NB), 0, ctx->stream, inv + (size_t)k * CH_NB * CH_NB, kb, B + k0, ldb, q, info);
        if (below > 0)
            hipLaunchKernelGGL(k_chol_fwd, dim3((unsigned)((below + 255) / 256), qg), dim3(256), 0, ctx->stream,
                               L + (size_t)(k0 + CH_NB) + (size_t)k0 * (size_t)ldl, ldl, below, B + k0, B + k0 + CH_NB, ldb, q, info);
    }
    JCH_HIP(ctx, hipGetLastError());
    for (int64_t k = nblk - 1; k >= 0; --k) {   // L' X = Y
        const int64_t k0 = k * CH_NB, below = n - k0 - CH_NB;
        const int kb = (int)std::min<int64_t>(CH_NB, n - k0);
        if (below > 0)
            hipLaunchKernelGGL(k_chol_bwd, dim3(CH_NB, qg), dim3(256), 0, ctx->stream, L + (size_t)(k0 + CH_NB) + (size_t)k0 * (size_t)ldl, ldl, below,
                               B + k0, B + k0 + CH_NB, ldb, q, info);
        hipLaunchKernelGGL(k_chol_sdiag<true>, dim3(qg), dim3(CH_NB), 0, ctx->stream, inv + (size_t)k * CH_NB * CH_NB, kb, B + k0, ldb, q, info);
    }
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

int32_t jch_launch_chol_inv_t(jch_ctx *ctx, const double *L, int64_t n, int64_t ldl, double *W, int64_t ldw, const int *info)
{
    if (ctx->chol_L != L || ctx->chol_n != n || ctx->chol_ld != ldl)
        return jch_fail(ctx, JCH_EINVAL, "the inverse factor: L is not the factor the last jch_chol_factor of this ctx produced");
    const size_t nn = (size_t)n, lw = (size_t)ldw;
    JCH_TRY(ch_attrs(ctx));
    const double *inv = (const double *)ctx->chol_inv.ptr;
    if (lw == nn) JCH_HIP(ctx, hipMemsetAsync(W, 0, sizeof(double) * nn * nn, ctx->stream));
    else JCH_HIP(ctx, hipMemset2DAsync(W, sizeof(double) * lw, 0, sizeof(double) * nn, nn, ctx->stream));
    hipLaunchKernelGGL(k_chol_eye, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, W, n, ldw);
    JCH_HIP(ctx, hipGetLastError());
    const int64_t nblk = (n + CH_NB - 1) / CH_NB;
    for (int64_t k = 0; k < nblk; ++k) {
        const int64_t k0 = k * CH_NB, below = n - k0 - CH_NB;
        const int kb = (int)std::min<int64_t>(CH_NB, n - k0);
        double *Wk = W + (size_t)k0 * lw;   // block column k of W: rows [0, k0 + kb) are live
        JCH_TRY(launch_tile<0>(ctx, Wk, ldw, k0 + kb, inv + (size_t)k * CH_NB * CH_NB, CH_NB, kb, kb, Wk, ldw, info));
        if (below > 0)
            JCH_TRY(launch_tile<2>(ctx, Wk, ldw, k0 + CH_NB, L + (size_t)(k0 + CH_NB) + (size_t)k0 * (size_t)ldl, ldl, below, CH_NB,
                                   W + (size_t)(k0 + CH_NB) * lw, ldw, info));
    }
    return JCH_OK;
}

int32_t jch_launch_chol_inv_fro2(jch_ctx *ctx, const double *L, int64_t n, int64_t ldl, double *out, const int *info)
{
    if (ctx->chol_L != L || ctx->chol_n != n || ctx->chol_ld != ldl)
        return jch_fail(ctx, JCH_EINVAL, "jch_chol_inv_fro2: L is not the factor the last jch_chol_factor of this ctx produced");
    const size_t nn = (size_t)n;
    if (jch_reserve(ctx, ctx->chol_w, sizeof(double) * nn * nn) != JCH_OK)
        return jch_fail(ctx, JCH_ENOMEM, "jch_chol_inv_fro2: no room for the n x n workspace of inv(L) (%.1f GiB) that df needs; ask without df",
                        (double)(sizeof(double) * nn * nn) / (1024.0 * 1024.0 * 1024.0));
    JCH_TRY(jch_reserve(ctx, ctx->chol_s, 256 + sizeof(double) * (CH_SUMSQ_WG + 8)));
    double *W = (double *)ctx->chol_w.ptr, *part = (double *)((char *)ctx->chol_s.ptr + 256);
    JCH_TRY(jch_launch_chol_inv_t(ctx, L, n, ldl, W, n, info));
    const int64_t tot = n * n;
    const int np = (int)std::max<int64_t>(1, std::min<int64_t>(CH_SUMSQ_WG, (tot + 255) / 256));
    hipLaunchKernelGGL(k_chol_sumsq, dim3((unsigned)np), dim3(256), 0, ctx->stream, W, tot, part, info);
    hipLaunchKernelGGL(k_chol_sum1, dim3(1), dim3(256), 0, ctx->stream, part, np, out, info);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

// ---- the exported primitives (DEVICE pointers; include/jchemo_hip.h)
namespace {
int32_t ch_check(jch_ctx *ctx, const char *who, const void *A, int64_t n, int64_t lda)
{
    if (!A || n < 1 || lda < n || n > (1 << 20)) return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments (n=%lld ld=%lld)", who, (long long)n, (long long)lda);
    return JCH_OK;
}
}  // namespace

extern "C" int32_t jch_chol_factor(jch_ctx *ctx, double *A, int64_t n, int64_t lda, int32_t *info)
{
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(ch_check(ctx, "jch_chol_factor", A, n, lda));
    if (!info) return jch_fail(ctx, JCH_EINVAL, "jch_chol_factor: info is NULL");
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    int *idev = nullptr;
    JCH_TRY(jch_chol_info_word(ctx, &idev));
    JCH_TRY(jch_launch_chol_factor(ctx, A, n, lda, idev));
    int h = 0;
    JCH_HIP(ctx, hipMemcpyAsync(&h, idev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *info = h;
    if (h != 0) ctx->chol_L = nullptr;   // no factor to solve with
    return JCH_OK;
}

extern "C" int32_t jch_chol_solve(jch_ctx *ctx, const double *L, int64_t n, int64_t ldl, double *B, int64_t q, int64_t ldb)
{
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(ch_check(ctx, "jch_chol_solve", L, n, ldl));
    if (!B || q < 1 || ldb < n) return jch_fail(ctx, JCH_EINVAL, "jch_chol_solve: bad B (q=%lld ldb=%lld)", (long long)q, (long long)ldb);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    int *idev = nullptr;
    JCH_TRY(jch_chol_info_word(ctx, &idev));   // 0 since the factor this solve is keyed to succeeded
    JCH_TRY(jch_launch_chol_solve(ctx, L, n, ldl, B, q, ldb, idev));
    JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JCH_OK;
}

extern "C" int32_t jch_chol_inv_fro2(jch_ctx *ctx, const double *L, int64_t n, int64_t ldl, double *out)
{
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(ch_check(ctx, "jch_chol_inv_fro2", L, n, ldl));
    if (!out) return jch_fail(ctx, JCH_EINVAL, "jch_chol_inv_fro2: out is NULL");
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    int *idev = nullptr;
    JCH_TRY(jch_chol_info_word(ctx, &idev));
    double *odev = (double *)((char *)idev + 128);
    JCH_TRY(jch_launch_chol_inv_fro2(ctx, L, n, ldl, odev, idev));
    JCH_HIP(ctx, hipMemcpyAsync(out, odev, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JCH_OK;
}
