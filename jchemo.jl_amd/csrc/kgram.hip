// Kernel Gram matrices of dkplsr (src/dkplsr.jl:102-122 through src/kernels.jl:26-30, 59-70):
//   K (m x n, column-major, ld ldk) = kern(Z diag(1/zdiv), X diag(1/xdiv))
//   krbf: K_ij = exp(-gamma max(0, |z_i|^2 + |x_j|^2 - 2 z_i.x_j))   (euclsq, src/distances.jl:24-28: expanded norms, clamped at 0)
//   kpol: K_ij = (gamma z_i.x_j + coef0)^degree, the power by degree - 1 successive multiplications (src/kernels.jl:62-67)
// krbf runs on rows shifted by one common vector c = the column means of the (scaled) X argument: the distances do not change,
// the cancellation of the norm expansion on spectra with a large baseline goes away (the reference does not shift; our values
// are closer to the exact distances than its own, never further).
//
//   k_gram_colmean  c (krbf only)
//   k_gram_copy     scaled, shifted, zero-padded column-major copies of Z and X (rows padded to 128, columns to T128_KB)
//   k_gram_norms    |z_i|^2, |x_j|^2 of those copies: O((m + n) p)
//   k_gram          128 x 128 output tile per workgroup of 4 waves (64 x 64 per wave, 4 x 4 v_mfma_f64_16x16x4_f64 tiles);
//                   a k-column of a tile is one contiguous 1 KB read of the copy; operands staged through LDS, double-buffered
//                   (the next chunk is loaded into registers while the current one is multiplied, one barrier per chunk);
//                   A = X tile, B = Z tile so that the accumulator's lane index (f64 C/D: col = lane & 15, row = (lane >> 4) +
//                   4 reg) runs along i, the contiguous direction of K: every store instruction writes 128-byte column pieces.
//                   Symmetric case (the train Gram: Z == X): the tiles with ti <= tj only; each is stored at (i, j) directly and
//                   at (j, i) through LDS (512-byte column pieces); K is bitwise symmetric and, for krbf, d_ii = 0 (diagonal 1).
// Bound: 2 m n p flop (n^2 p symmetric) at the f64 matrix peak (78.6 TF) against 8 m n bytes written.
// Every index into K and into the copies is 64-bit: m * ldk > 2^31 is legal.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "jch_internal.h"
#include "tile128_dev.h"

#define KG_WLD 66    // LDS row stride of the transposing store (64 + 2)

__global__ __launch_bounds__(256) void k_gram_colmean(const double *__restrict__ X, int64_t n, int64_t ldx, const double *__restrict__ xdiv,
                                                      double *__restrict__ c)
{
    __shared__ double scr[4];
    const int64_t k = blockIdx.x;
    const double dv = xdiv ? xdiv[k] : 1.0;
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < n; j += 256) s += X[(size_t)j + (size_t)k * (size_t)ldx] / dv;
    s = jch_block_sum<256>(s, scr);
    if (threadIdx.x == 0) c[k] = s / (double)n;
}

// out[k * ldc + i] = src[i, k] / div[k] - c[k] for i < rows, k < p; 0 in the padding (i < ldc, k < pp)
__global__ __launch_bounds__(256) void k_gram_copy(const double *__restrict__ src, int64_t rows, int64_t lds, int64_t p, const double *__restrict__ div,
                                                   const double *__restrict__ c, double *__restrict__ out, int64_t ldc, int64_t pp)
{
    const int64_t tot = ldc * pp;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) {
        const int64_t k = e / ldc, i = e - k * ldc;
        double v = 0.0;
        if (i < rows && k < p) {
            v = src[(size_t)i + (size_t)k * (size_t)lds];
            if (div) v /= div[k];
            if (c) v -= c[k];
        }
        out[e] = v;
    }
}

__global__ __launch_bounds__(256) void k_gram_norms(const double *__restrict__ cp, int64_t ldc, int64_t pp, double *__restrict__ nrm)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= ldc) return;
    double s = 0.0;
    for (int64_t k = 0; k < pp; ++k) {
        const double v = cp[(size_t)i + (size_t)k * (size_t)ldc];
        s += v * v;
    }
    nrm[i] = s;
}

template <bool SYM>
__global__ __launch_bounds__(256, 2) void k_gram(const double *__restrict__ Zc, int64_t ldcz, const double *__restrict__ Xc, int64_t ldcx, int pp,
                                                 const double *__restrict__ nz, const double *__restrict__ nx, int64_t m, int64_t n, int tiles_i,
                                                 int kind, double gamma, double coef0, int degree, double *__restrict__ K, int64_t ldk)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t ti, tj;
    if (SYM) {
        t128_tri(blockIdx.x, ti, tj);   // ti <= tj
    } else {
        ti = blockIdx.x % tiles_i; tj = blockIdx.x / tiles_i;
    }
    const int64_t i0 = ti * T128_T, j0 = tj * T128_T;
    const int qj = wv >> 1, qi = wv & 1;
    t128_v4d acc[4][4];   // A = X tile (output rows j of the MFMA), B = Z tile (output columns i)
    t128_mma(
        lds, pp / T128_KB,
        [&](int k, int c) { return __builtin_nontemporal_load(reinterpret_cast<const t128_v2d *>(Xc + (size_t)k * (size_t)ldcx + (size_t)j0 + c)); },
        [&](int k, int c) { return __builtin_nontemporal_load(reinterpret_cast<const t128_v2d *>(Zc + (size_t)k * (size_t)ldcz + (size_t)i0 + c)); },
        acc);
    // epilogue in registers: acc[mj][ni][reg] = dot(x_j, z_i), j = j0 + 64 qj + 16 mj + (lane >> 4) + 4 reg, i = i0 + 64 qi + 16 ni + (lane & 15)
    double zn[4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) zn[ni] = kind == JCH_KERN_RBF ? nz[i0 + 64 * qi + 16 * ni + (lane & 15)] : 0.0;
#pragma unroll
    for (int mj = 0; mj < 4; ++mj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t j = j0 + 64 * qj + 16 * mj + (lane >> 4) + 4 * reg;
            const double xn = kind == JCH_KERN_RBF ? nx[j] : 0.0;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const double dot = acc[mj][ni][reg];
                double v;
                if (kind == JCH_KERN_RBF) {
                    const int64_t i = i0 + 64 * qi + 16 * ni + (lane & 15);
                    double d = zn[ni] + xn - 2.0 * dot;
                    if (SYM && i == j) d = 0.0;
                    v = exp(-gamma * fmax(d, 0.0));
                } else {
                    const double t = gamma * dot + coef0;
                    v = t;
                    for (int r = 1; r < degree; ++r) v *= t;
                }
                acc[mj][ni][reg] = v;
            }
        }
    // direct store K[i + j ldk] (symmetric diagonal tile: j >= i only, the rest comes from the mirrored store)
#pragma unroll
    for (int mj = 0; mj < 4; ++mj)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t j = j0 + 64 * qj + 16 * mj + (lane >> 4) + 4 * reg;
            if (j >= n) continue;
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int64_t i = i0 + 64 * qi + 16 * ni + (lane & 15);
                if (i < m && (!SYM || ti != tj || j >= i)) K[(size_t)i + (size_t)j * (size_t)ldk] = acc[mj][ni][reg];
            }
        }
    if (!SYM) return;
    // mirrored store K[j + i ldk] (j > i on the diagonal tile): per 16-column slice ni, the wave's 64 j x 16 i values go through LDS
    // [i][j] so that lane = j and every store instruction writes a 512-byte piece of one column of K
    double *Wt = lds + wv * 16 * KG_WLD;
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
        for (int mj = 0; mj < 4; ++mj)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) Wt[(lane & 15) * KG_WLD + 16 * mj + (lane >> 4) + 4 * reg] = acc[mj][ni][reg];
        __syncthreads();
        const int64_t j = j0 + 64 * qj + lane;
        if (j < n) {
#pragma unroll 4
            for (int il = 0; il < 16; ++il) {
                const int64_t i = i0 + 64 * qi + 16 * ni + il;
                if (i < m && (ti != tj || j > i)) K[(size_t)j + (size_t)i * (size_t)ldk] = Wt[il * KG_WLD + lane];
            }
        }
        __syncthreads();
    }
}

int32_t jch_launch_kgram_prep(jch_ctx *ctx, const double *X, int64_t n, int64_t ldx, int64_t p, const double *c, double *cp, int64_t ldc, int64_t pp, double *nrm)
{
    const unsigned nb = (unsigned)std::min<int64_t>((ldc * pp + 255) / 256, (int64_t)ctx->cus * 16);
    hipLaunchKernelGGL(k_gram_copy, dim3(nb), dim3(256), 0, ctx->stream, X, n, ldx, p, (const double *)nullptr, c, cp, ldc, pp);
    hipLaunchKernelGGL(k_gram_norms, dim3((unsigned)((ldc + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)cp, ldc, pp, nrm);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

int32_t jch_launch_kgram(jch_ctx *ctx, int kind, const double *Z, int64_t m, int64_t ldz, const double *zdiv, const double *X, int64_t n,
                         int64_t ldx, const double *xdiv, int64_t p, double gamma, double coef0, int degree, bool sym, double *K, int64_t ldk)
{
    if (m < 1 || n < 1) return JCH_OK;
    const int64_t pp = (p + T128_KB - 1) / T128_KB * T128_KB;
    const int64_t tiles_i = (m + T128_T - 1) / T128_T, tiles_j = (n + T128_T - 1) / T128_T;
    const int64_t ldcz = tiles_i * T128_T, ldcx = tiles_j * T128_T;
    const int64_t nblocks = sym ? tiles_j * (tiles_j + 1) / 2 : tiles_i * tiles_j;
    if (nblocks > 0x7fffffffLL || pp > 0x7fffffffLL) return jch_fail(ctx, JCH_EINVAL, "jch_kernel_gram: shape too large (m=%lld n=%lld p=%lld)", (long long)m, (long long)n, (long long)p);
    const bool rbf = kind == JCH_KERN_RBF;
    const size_t need = 256 * 8 + sizeof(double) * (3 * (size_t)pp + (size_t)ldcz + (size_t)ldcx + (size_t)ldcz * pp + (sym ? 0 : (size_t)ldcx * pp));
    JCH_TRY(jch_reserve(ctx, ctx->kg_ws, need));
    jch_carve cv;
    double *ws = (double *)ctx->kg_ws.ptr;
    double *c = ws + cv.take(pp), *dz = ws + cv.take(pp), *dx = ws + cv.take(pp);
    double *nzv = ws + cv.take(ldcz), *nxv = sym ? nzv : ws + cv.take(ldcx);
    double *Zcp = ws + cv.take((size_t)ldcz * pp), *Xcp = sym ? Zcp : ws + cv.take((size_t)ldcx * pp);
    if (zdiv) JCH_HIP(ctx, hipMemcpyAsync(dz, zdiv, sizeof(double) * (size_t)p, hipMemcpyHostToDevice, ctx->stream));
    if (xdiv) JCH_HIP(ctx, hipMemcpyAsync(dx, xdiv, sizeof(double) * (size_t)p, hipMemcpyHostToDevice, ctx->stream));
    if (rbf) hipLaunchKernelGGL(k_gram_colmean, dim3((unsigned)p), dim3(256), 0, ctx->stream, X, n, ldx, xdiv ? dx : nullptr, c);
    auto copy = [&](const double *src, int64_t rows, int64_t ld, const double *div, double *out, int64_t ldc, double *nrm) {
        const unsigned nb = (unsigned)std::min<int64_t>((ldc * pp + 255) / 256, (int64_t)ctx->cus * 16);
        hipLaunchKernelGGL(k_gram_copy, dim3(nb), dim3(256), 0, ctx->stream, src, rows, ld, p, div, rbf ? c : nullptr, out, ldc, pp);
        if (rbf) hipLaunchKernelGGL(k_gram_norms, dim3((unsigned)((ldc + 255) / 256)), dim3(256), 0, ctx->stream, out, ldc, pp, nrm);
    };
    copy(Z, m, ldz, zdiv ? dz : nullptr, Zcp, ldcz, nzv);
    if (!sym) copy(X, n, ldx, xdiv ? dx : nullptr, Xcp, ldcx, nxv);
    JCH_HIP(ctx, hipGetLastError());
    static jch_per_device_once attr;
    if (!attr.done(ctx->device)) {
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_gram<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_gram<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr.mark(ctx->device);
    }
    if (sym)
        hipLaunchKernelGGL(k_gram<true>, dim3((unsigned)nblocks), dim3(256), T128_LDS_BYTES, ctx->stream, Zcp, ldcz, Xcp, ldcx, (int)pp, nzv, nxv, m, n,
                           (int)tiles_i, kind, gamma, coef0, degree, K, ldk);
    else
        hipLaunchKernelGGL(k_gram<false>, dim3((unsigned)nblocks), dim3(256), T128_LDS_BYTES, ctx->stream, Zcp, ldcz, Xcp, ldcx, (int)pp, nzv, nxv, m, n,
                           (int)tiles_i, kind, gamma, coef0, degree, K, ldk);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}
