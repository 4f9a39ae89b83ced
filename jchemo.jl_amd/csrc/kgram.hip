// Kernel Gram matrices of dkplsr (src/dkplsr.jl:102-122 through src/kernels.jl:26-30, 59-70):
//   K (m x n, column-major, ld ldk) = kern(Z diag(1/zdiv), X diag(1/xdiv))
//   krbf: K_ij = exp(-gamma max(0, |z_i|^2 + |x_j|^2 - 2 z_i.x_j))   (euclsq, src/distances.jl:24-28: expanded norms, clamped at 0)
//   kpol: K_ij = (gamma z_i.x_j + coef0)^degree, the power by degree - 1 successive multiplications (src/kernels.jl:62-67)
// krbf runs on rows shifted by one common vector c = the column means of the (scaled) X argument: the distances do not change,
// the cancellation of the norm expansion on spectra with a large baseline goes away (the reference does not shift; our values
// are closer to the exact distances than its own, never further).
//
//   k_gram_colmean  c (krbf only)
//   k_gram_copy     scaled, shifted, zero-padded column-major copies of Z and X (rows padded to 128, columns to KG_KB)
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

typedef double v2f64 __attribute__((ext_vector_type(2)));
typedef double v4f64 __attribute__((ext_vector_type(4)));

#define KG_T 128     // output tile edge
#define KG_KB 16     // k-columns per staged chunk
#define KG_LD 144    // LDS row stride (doubles): 128 + 16 (consecutive k-rows 32 banks apart, as k_syrk)
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
    double *As = lds;                            // [2][KG_KB][KG_LD]  X tile (output rows j of the MFMA)
    double *Bs = lds + 2 * KG_KB * KG_LD;        // [2][KG_KB][KG_LD]  Z tile (output columns i of the MFMA)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int64_t ti, tj;
    if (SYM) {   // linear index -> (ti <= tj): tj (tj + 1) / 2 <= b < (tj + 1)(tj + 2) / 2
        const int64_t b = blockIdx.x;
        int64_t t = (int64_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
        while (t * (t + 1) / 2 > b) --t;
        while ((t + 1) * (t + 2) / 2 <= b) ++t;
        tj = t; ti = b - t * (t + 1) / 2;
    } else {
        ti = blockIdx.x % tiles_i; tj = blockIdx.x / tiles_i;
    }
    const int64_t i0 = ti * KG_T, j0 = tj * KG_T;
    const int qj = wv >> 1, qi = wv & 1;
    v4f64 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = v4f64{0.0, 0.0, 0.0, 0.0};
    v2f64 va[4], vb[4];
    auto load = [&](int k0) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int64_t k = k0 + wv * 4 + it;
            va[it] = __builtin_nontemporal_load(reinterpret_cast<const v2f64 *>(Xc + (size_t)k * (size_t)ldcx + (size_t)j0 + 2 * lane));
            vb[it] = __builtin_nontemporal_load(reinterpret_cast<const v2f64 *>(Zc + (size_t)k * (size_t)ldcz + (size_t)i0 + 2 * lane));
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = wv * 4 + it;
            *reinterpret_cast<v2f64 *>(As + (buf * KG_KB + row) * KG_LD + 2 * lane) = va[it];
            *reinterpret_cast<v2f64 *>(Bs + (buf * KG_KB + row) * KG_LD + 2 * lane) = vb[it];
        }
    };
    const int nch = pp / KG_KB;
    load(0);
    stage(0);
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nch) load((ch + 1) * KG_KB);
        const double *A = As + buf * KG_KB * KG_LD, *B = Bs + buf * KG_KB * KG_LD;
#pragma unroll
        for (int kk = 0; kk < KG_KB / 4; ++kk) {
            const int krow = 4 * kk + (lane >> 4);
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] = A[krow * KG_LD + 64 * qj + 16 * u + (lane & 15)];
                b[u] = B[krow * KG_LD + 64 * qi + 16 * u + (lane & 15)];
            }
#pragma unroll
            for (int mj = 0; mj < 4; ++mj)
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) acc[mj][ni] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mj], b[ni], acc[mj][ni], 0, 0, 0);
        }
        if (ch + 1 < nch) stage(buf ^ 1);
        __syncthreads();
    }
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

namespace {
struct kg_carve {
    char *base; size_t off;
    double *take(size_t count) { double *p = (double *)(base + off); off += ((count * sizeof(double)) + 255) & ~(size_t)255; return p; }
};
}  // namespace

int32_t jch_launch_kgram(jch_ctx *ctx, int kind, const double *Z, int64_t m, int64_t ldz, const double *zdiv, const double *X, int64_t n,
                         int64_t ldx, const double *xdiv, int64_t p, double gamma, double coef0, int degree, bool sym, double *K, int64_t ldk)
{
    if (m < 1 || n < 1) return JCH_OK;
    const int64_t pp = (p + KG_KB - 1) / KG_KB * KG_KB;
    const int64_t tiles_i = (m + KG_T - 1) / KG_T, tiles_j = (n + KG_T - 1) / KG_T;
    const int64_t ldcz = tiles_i * KG_T, ldcx = tiles_j * KG_T;
    const int64_t nblocks = sym ? tiles_j * (tiles_j + 1) / 2 : tiles_i * tiles_j;
    if (nblocks > 0x7fffffffLL || pp > 0x7fffffffLL) return jch_fail(ctx, JCH_EINVAL, "jch_kernel_gram: shape too large (m=%lld n=%lld p=%lld)", (long long)m, (long long)n, (long long)p);
    const bool rbf = kind == JCH_KERN_RBF;
    const size_t need = 256 * 8 + sizeof(double) * (3 * (size_t)pp + (size_t)ldcz + (size_t)ldcx + (size_t)ldcz * pp + (sym ? 0 : (size_t)ldcx * pp));
    JCH_TRY(jch_reserve(ctx, ctx->kg_ws, need));
    kg_carve cv{(char *)ctx->kg_ws.ptr, 0};
    double *c = cv.take(pp), *dz = cv.take(pp), *dx = cv.take(pp);
    double *nzv = cv.take(ldcz), *nxv = sym ? nzv : cv.take(ldcx);
    double *Zcp = cv.take((size_t)ldcz * pp), *Xcp = sym ? Zcp : cv.take((size_t)ldcx * pp);
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
    const size_t ldsb = sizeof(double) * 4 * KG_KB * KG_LD;   // 73 728 B: two workgroups per CU
    static jch_per_device_once attr;
    if (!attr.done(ctx->device)) {
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_gram<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_gram<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr.mark(ctx->device);
    }
    if (sym)
        hipLaunchKernelGGL(k_gram<true>, dim3((unsigned)nblocks), dim3(256), ldsb, ctx->stream, Zcp, ldcz, Xcp, ldcx, (int)pp, nzv, nxv, m, n,
                           (int)tiles_i, kind, gamma, coef0, degree, K, ldk);
    else
        hipLaunchKernelGGL(k_gram<false>, dim3((unsigned)nblocks), dim3(256), ldsb, ctx->stream, Zcp, ldcz, Xcp, ldcx, (int)pp, nzv, nxv, m, n,
                           (int)tiles_i, kind, gamma, coef0, degree, K, ldk);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}
