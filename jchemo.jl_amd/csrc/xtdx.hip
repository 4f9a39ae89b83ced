// Weighted centred Gram of a column-major matrix, and PCA / PCR on it (src/pcasvd.jl:79-146, src/pcr.jl:82-97): jch_xtdx, jch_pca_fit —
// include/jchemo_hip.h; DESIGN.md §16.
//
//   G = (X - 1 mu')' D (X - 1 mu'),  D = diag(w / sum w),  p x p from ONE read-only pass over the n x p column-major X per tile pair, with no
//   n x p workspace: the means and the weights are applied in registers on the way into LDS.  Nothing is computed as X'DX - mu mu' (spectra
//   at level 100 with spread 1 would lose the digits the fit needs; k_cs_pass of covsel.hip makes the same argument).
//
//   k_xtdx         partial tiles on v_mfma_f64_16x16x4_f64, k_syrk's scheme (kern2.hip): one 128 x 128 output tile per workgroup, upper tile
//                  pairs only, the rows split over workgroups, operands staged through LDS while the next chunk is in flight in registers.
//                  A chunk is 16 rows; a lane loads two consecutive rows of four columns of each operand (16-byte loads when X and ldx allow,
//                  two 8-byte loads otherwise: the same values in the same places, hence the same bits).  Two stages alternate, so a chunk costs
//                  one barrier.  (k_syrk's 32-row chunk with one stage needs 64 load registers beside the 128 accumulators and spills; 16 rows
//                  need 32.)  A stage is column-major, At[col][XT_LD]: XT_LD = 18 doubles puts the 16 columns x 2 k-rows that one 32-lane half
//                  reads with ds_read_b64 on the 32 distinct 8-byte slots of the 256-byte bank row (18 l mod 32 runs through the 16 even
//                  numbers), so the operand reads are conflict-free.
//   k_xtdx_reduce  sums the partial tiles in split order and writes G[i, j] and G[j, i] from the same value (of a diagonal tile only the
//                  entries on or above the diagonal are used): G == G' bitwise, no atomics, two runs give identical bits.
//   Rows >= n are never read; padding rows and columns enter the stage as exact zeros.  A NaN at X[r, j] reaches column j of both operands
//   only, that is row j and column j of G.
// gfx950, hipcc -O3: k_xtdx<true> and k_xtdx<false> 240 VGPRs each, no scratch: 2 waves per SIMD, that is 2 workgroups per CU, which the 74 KB of
// LDS per workgroup allow too.
//
// PCA (jch_pca_fit): the reference takes svd(sqrtD Xc).  Here P and sv^2 are the leading eigenpairs of G (the reference's own `pcaeigen` route)
// from the block subspace iteration kpca uses (jch_eig_lead, kpca.hip), which only ever touches the p x p matrix G; T = cscale(X) P is one
// jch_transform.  scal = true rescales G by xscales = sqrt(diag G) instead of touching X; sstot = trace(G).
//
// Spherical PCA (jch_pcasph_fit, src/pcasph.jl:60-92): the same pass with mu = the spatial median (medspa.hip) and the row weights
// w_i / r_i^2, r_i the norm of the centred (scaled) row, is the Gram of the rows projected on the unit sphere; P from the same iteration, T by
// jch_transform, sv = the MADs of T / r (colselect.hip), everything reordered by sv.
#include <math.h>

#include <algorithm>

#include "jch_internal.h"

typedef double xt_v2 __attribute__((ext_vector_type(2)));
typedef double xt_v4 __attribute__((ext_vector_type(4)));

#define XT_NT 256
#define XT_KB 16    // rows per staged chunk
#define XT_LD 18    // doubles per staged column: XT_KB + 2 (see the header)
#define XT_STAGE (2 * 128 * XT_LD)   // doubles of one stage: both operands
#define XT_MAXP 32768

template <bool VEC>
__global__ __launch_bounds__(XT_NT, 2) void k_xtdx(const double *__restrict__ X, int64_t n, int p, int64_t ldx, const double *__restrict__ mu,
                                                   const double *__restrict__ dw, double *__restrict__ Gpart, int nsplit, int nblk)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    // stage s (of two): At = lds + s * XT_STAGE, [128][XT_LD] d_r (X[r, i-block] - mu); Bt = At + 128 * XT_LD, X[r, j-block] - mu
    double *mus = lds + 2 * XT_STAGE;       // [2][128] the means of the two column blocks (0 for padding columns)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // upper-triangular tile pair from the linear pair index
    int pr = blockIdx.y, bi = 0;
    while (pr >= nblk - bi) { pr -= nblk - bi; ++bi; }
    const int bj = bi + pr;
    const bool diag = bi == bj;
    const int64_t per = ((n + nsplit - 1) / nsplit + XT_KB - 1) / XT_KB * XT_KB;
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = std::min<int64_t>(n, r0 + per);
    {
        const int c = 128 * (tid < 128 ? bi : bj) + (tid & 127);
        mus[tid] = c < p ? mu[c] : 0.0;
    }
    // loader: row pair rp of the chunk, columns c0 + 32 it of each block
    const int rp = tid & 7, c0 = tid >> 3;
    xt_v4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = xt_v4{0.0, 0.0, 0.0, 0.0};
    xt_v2 va[4], vb[4], dv;
    const double *xa = X + (size_t)(128 * bi + c0) * (size_t)ldx, *xb = X + (size_t)(128 * bj + c0) * (size_t)ldx;   // (only dereferenced for columns < p)
    const size_t cstep = (size_t)32 * (size_t)ldx;
    auto load2 = [&](const double *ptr, bool col, int64_t r) -> xt_v2 {
        xt_v2 v = xt_v2{0.0, 0.0};
        if (col && r < r1) {
            if (VEC && r + 1 < r1) {
                v = __builtin_nontemporal_load(reinterpret_cast<const xt_v2 *>(ptr + r));
            } else {
                v.x = __builtin_nontemporal_load(ptr + r);
                if (r + 1 < r1) v.y = __builtin_nontemporal_load(ptr + r + 1);
            }
        }
        return v;
    };
    auto prefetch = [&](int64_t rb) {
        const int64_t r = rb + 2 * rp;
        dv = xt_v2{r < r1 ? dw[r] : 0.0, r + 1 < r1 ? dw[r + 1] : 0.0};
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            va[it] = load2(xa + it * cstep, 128 * bi + c0 + 32 * it < p, r);
            if (!diag) vb[it] = load2(xb + it * cstep, 128 * bj + c0 + 32 * it < p, r);
        }
    };
    // what prefetch(rb) fetched goes, centred and weighted, into stage s
    auto stage = [&](int64_t rb, int s) {
        double *At = lds + s * XT_STAGE, *Bt = At + 128 * XT_LD;
        const int64_t r = rb + 2 * rp;
        const bool l0 = r < r1, l1 = r + 1 < r1;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int c = c0 + 32 * it;
            const double ma = mus[c];
            const xt_v2 ca = xt_v2{l0 ? va[it].x - ma : 0.0, l1 ? va[it].y - ma : 0.0};   // (a padding column holds 0 - 0)
            xt_v2 cb = ca;
            if (!diag) {
                const double mb = mus[128 + c];
                cb = xt_v2{l0 ? vb[it].x - mb : 0.0, l1 ? vb[it].y - mb : 0.0};
            }
            *reinterpret_cast<xt_v2 *>(At + c * XT_LD + 2 * rp) = xt_v2{ca.x * dv.x, ca.y * dv.y};
            *reinterpret_cast<xt_v2 *>(Bt + c * XT_LD + 2 * rp) = cb;
        }
    };
    const int qi = wv >> 1, qj = wv & 1;
    if (r0 < r1) prefetch(r0);
    __syncthreads();   // (mus)
    if (r0 < r1) stage(r0, 0);
    __syncthreads();
    int s = 0;
    for (int64_t rb = r0; rb < r1; rb += XT_KB, s ^= 1) {
        const bool more = rb + XT_KB < r1;   // (uniform over the workgroup)
        if (more) prefetch(rb + XT_KB);     // in flight while this chunk is multiplied
        const double *At = lds + s * XT_STAGE, *Bt = At + 128 * XT_LD;
#pragma unroll
        for (int kk = 0; kk < XT_KB / 4; ++kk) {
            const int krow = 4 * kk + (lane >> 4);
            double a[4], b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                a[m] = At[(64 * qi + 16 * m + (lane & 15)) * XT_LD + krow];
                b[m] = Bt[(64 * qj + 16 * m + (lane & 15)) * XT_LD + krow];
            }
#pragma unroll
            for (int mi = 0; mi < 4; ++mi)
#pragma unroll
                for (int nj = 0; nj < 4; ++nj) acc[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[nj], acc[mi][nj], 0, 0, 0);
        }
        if (more) stage(rb + XT_KB, s ^ 1);   // (the other stage: its last readers passed the barrier below one trip ago)
        __syncthreads();
    }
    // D[m][n]: n = lane & 15, m = (lane >> 4) + 4 reg
    double *gp = Gpart + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * (128 * 128);
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int nj = 0; nj < 4; ++nj)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int m = 64 * qi + 16 * mi + (lane >> 4) + 4 * reg, nn = 64 * qj + 16 * nj + (lane & 15);
                gp[m * 128 + nn] = acc[mi][nj][reg];
            }
}

// G[i, j] = G[j, i] = sum over the splits, in split order
__global__ __launch_bounds__(XT_NT) void k_xtdx_reduce(const double *__restrict__ Gpart, int nsplit, int npairs, int nblk, int p, double *__restrict__ G,
                                                       int64_t ldg)
{
    int pr = blockIdx.y, bi = 0;
    while (pr >= nblk - bi) { pr -= nblk - bi; ++bi; }
    const int bj = bi + pr;
    const int e = blockIdx.x * XT_NT + threadIdx.x;   // element of the 128 x 128 tile
    const int m = e >> 7, nn = e & 127;
    const int i = 128 * bi + m, j = 128 * bj + nn;
    if (i >= p || j >= p || (bi == bj && m > nn)) return;
    double s = 0.0;
    for (int sp = 0; sp < nsplit; ++sp) s += Gpart[((size_t)sp * npairs + blockIdx.y) * (128 * 128) + e];
    G[(size_t)i + (size_t)j * (size_t)ldg] = s;
    G[(size_t)j + (size_t)i * (size_t)ldg] = s;
}

// colvar = diag(G); scal: xs = sqrt(colvar) (what `colstd` is: the uncorrected weighted standard deviation, no rule of its own for a constant
// column, as in the plskern prologue), else xs = 1
__global__ __launch_bounds__(XT_NT) void k_xt_diag(const double *__restrict__ G, int64_t ldg, int p, int scal, double *__restrict__ colvar, double *__restrict__ xs)
{
    const int j = blockIdx.x * XT_NT + threadIdx.x;
    if (j >= p) return;
    const double v = G[(size_t)j * (size_t)(ldg + 1)];
    colvar[j] = v;
    xs[j] = scal ? sqrt(v) : 1.0;
}

// G[i, j] /= xs[i] xs[j] (the product commutes: the two triangles stay bitwise equal)
__global__ __launch_bounds__(XT_NT) void k_xt_rescale(double *__restrict__ G, int64_t ldg, int p, const double *__restrict__ xs)
{
    const int64_t tot = (int64_t)p * p;
    for (int64_t e = (int64_t)blockIdx.x * XT_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * XT_NT) {
        const int64_t j = e / p, i = e - j * p;
        G[(size_t)i + (size_t)j * (size_t)ldg] /= xs[i] * xs[j];
    }
}

// *out = trace(G): thread-strided chains, then the block tree (one workgroup, fixed order)
__global__ __launch_bounds__(XT_NT) void k_xt_trace(const double *__restrict__ G, int64_t ldg, int p, double *out)
{
    __shared__ double scr[XT_NT / 64];
    double a = 0.0;
    for (int j = threadIdx.x; j < p; j += XT_NT) a += G[(size_t)j * (size_t)(ldg + 1)];
    a = jch_block_sum<XT_NT>(a, scr);
    if (threadIdx.x == 0) *out = a;
}

// V[i, k] = d[i] (Y[i, k] - ym[k]): the panel of Xc'D Yc
__global__ __launch_bounds__(XT_NT) void k_xt_dyc(const double *__restrict__ Y, int64_t n, int q, int64_t ldy, const double *__restrict__ ym,
                                                  const double *__restrict__ d, double *__restrict__ V)
{
    const int64_t tot = n * q;
    for (int64_t e = (int64_t)blockIdx.x * XT_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * XT_NT) {
        const int64_t k = e / n, i = e - k * n;
        V[e] = d[i] * (Y[(size_t)i + (size_t)k * (size_t)ldy] - ym[k]);
    }
}

int32_t jch_launch_xtdx(jch_ctx *ctx, const double *X, int64_t n, int p, int64_t ldx, const double *mu, const double *d, double *G, int64_t ldg)
{
    const int nblk = (p + 127) / 128, npairs = nblk * (nblk + 1) / 2;
    int nsplit = std::max(1, (ctx->cus * 2) / npairs);
    if ((int64_t)nsplit * XT_KB > n) nsplit = (int)std::max<int64_t>(1, n / XT_KB);
    JCH_TRY(jch_reserve(ctx, ctx->xt_part, sizeof(double) * (size_t)nsplit * npairs * 128 * 128));
    double *Gpart = (double *)ctx->xt_part.ptr;
    const size_t lds = sizeof(double) * (2 * XT_STAGE + 256);
    static jch_per_device_once attr;
    if (!attr.done(ctx->device)) {
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_xtdx<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_xtdx<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr.mark(ctx->device);
    }
    const bool vec = ((uintptr_t)X % 16 == 0) && (ldx % 2 == 0);   // (a split starts on a multiple of XT_KB rows, a lane on an even row of it)
    if (vec) hipLaunchKernelGGL(k_xtdx<true>, dim3(nsplit, npairs), dim3(XT_NT), lds, ctx->stream, X, n, p, ldx, mu, d, Gpart, nsplit, nblk);
    else hipLaunchKernelGGL(k_xtdx<false>, dim3(nsplit, npairs), dim3(XT_NT), lds, ctx->stream, X, n, p, ldx, mu, d, Gpart, nsplit, nblk);
    hipLaunchKernelGGL(k_xtdx_reduce, dim3(64, npairs), dim3(XT_NT), 0, ctx->stream, Gpart, nsplit, npairs, nblk, p, G, ldg);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

namespace {

// device views of a [loc] matrix and of the raw weights; the normalised weights; mu = X'd by the covsel pass against the one-column panel d (a
// fixed-order sum on the matrix cores whose bits do not depend on where X lives or how it is aligned)
struct xt_in {
    const double *dX = nullptr, *dw = nullptr;
    int64_t ldxd = 0;
};

int32_t xt_stage(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *weights, double *wraw, xt_in *in)
{
    in->dX = X; in->ldxd = ldx; in->dw = weights;
    if (loc == JCH_LOC_HOST) {
        const int64_t ld = (n + 1) & ~(int64_t)1;
        JCH_TRY(jch_reserve(ctx, ctx->dk_x, sizeof(double) * (size_t)ld * (size_t)p));
        JCH_TRY(jch_copy2d(ctx, (double *)ctx->dk_x.ptr, ld, X, ldx, n, p, hipMemcpyHostToDevice));
        in->dX = (const double *)ctx->dk_x.ptr; in->ldxd = ld;
        if (weights) {
            JCH_HIP(ctx, hipMemcpyAsync(wraw, weights, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
            in->dw = wraw;
        }
    }
    return JCH_OK;
}

int32_t xt_check(jch_ctx *ctx, const char *who, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx)
{
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (!X || n < 1 || p < 1 || ldx < n) return jch_fail(ctx, JCH_EINVAL, "%s: bad X (n=%lld p=%lld ldx=%lld)", who, (long long)n, (long long)p, (long long)ldx);
    if (p > XT_MAXP) return jch_fail(ctx, JCH_EINVAL, "%s: p=%lld beyond %d", who, (long long)p, XT_MAXP);
    if (ctx->nranks > 1) return jch_fail(ctx, JCH_EINVAL, "%s: one rank only (communicator of %d)", who, ctx->nranks);
    return JCH_OK;
}

}  // namespace

extern "C" int32_t jch_xtdx(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *weights, double *G_dev, int64_t ldg,
                            double *mu_dev, double *G_host, double *mu_host)
{
    static const char *who = "jch_xtdx";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(xt_check(ctx, who, loc, X, n, p, ldx));
    if (G_dev && ldg < p) return jch_fail(ctx, JCH_EINVAL, "%s: ldg=%lld < p=%lld", who, (long long)ldg, (long long)p);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    jch_carve cv;
    const size_t ow = cv.take((size_t)n), owr = cv.take((size_t)n), omu = cv.take((size_t)p), ohdr = cv.take(8), oG = cv.take(G_dev ? 0 : (size_t)p * p);
    JCH_TRY(jch_reserve(ctx, ctx->xt_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->xt_ws.ptr;
    double *wn = ws + ow, *mu = mu_dev ? mu_dev : ws + omu, *G = G_dev ? G_dev : ws + oG;
    const int64_t ld = G_dev ? ldg : p;
    return jch_synced(ctx, true, [&]() -> int32_t {
        xt_in in;
        JCH_TRY(xt_stage(ctx, loc, X, n, p, ldx, weights, ws + owr, &in));
        JCH_TRY(jch_launch_weights(ctx, in.dw, n, wn, ws + ohdr));
        JCH_TRY(jch_covsel_pass(ctx, in.dX, n, p, in.ldxd, nullptr, wn, 1, n, mu));
        JCH_TRY(jch_launch_xtdx(ctx, in.dX, n, (int)p, in.ldxd, mu, wn, G, ld));
        if (G_host) JCH_TRY(jch_copy2d(ctx, G_host, p, G, ld, p, p, hipMemcpyDeviceToHost));
        if (mu_host) JCH_HIP(ctx, hipMemcpyAsync(mu_host, mu, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    });
}

extern "C" int32_t jch_pca_fit(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *weights, const double *Y, int64_t q,
                               int64_t ldy, int32_t nlv, int32_t scal, double tol, int32_t maxit, double *T, double *P, double *sv, double *eig, double *xmeans,
                               double *xscales, double *weights_norm, double *sstot, double *colvar, double *ymeans, double *xtdy, int32_t *niter,
                               double *resid, int32_t *nlv_out, int32_t *converged)
{
    static const char *who = "jch_pca_fit";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(xt_check(ctx, who, loc, X, n, p, ldx));
    if (nlv < 1) return jch_fail(ctx, JCH_EINVAL, "%s: nlv = %d must be >= 1", who, nlv);
    if (maxit < 1) return jch_fail(ctx, JCH_EINVAL, "%s: maxit = %d must be >= 1", who, maxit);
    if (!(tol > 0.0)) return jch_fail(ctx, JCH_EINVAL, "%s: tol must be > 0", who);
    if (q < 0 || q > (1 << 15) || (q > 0 && (!Y || ldy < n))) return jch_fail(ctx, JCH_EINVAL, "%s: bad Y (q=%lld ldy=%lld)", who, (long long)q, (long long)ldy);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST;
    const int pi = (int)p, qi = (int)q;
    const int A = (int)std::min<int64_t>(nlv, std::min(n, p));   // src/pcasvd.jl:82
    const size_t nn = (size_t)n;
    jch_carve cv;
    const size_t oG = cv.take((size_t)p * p), ow = cv.take(nn), owr = cv.take(nn), omu = cv.take(pi), ocv = cv.take(pi), oxs = cv.take(pi), ohdr = cv.take(8),
                 otr = cv.take(8), oT = cv.take(host && T ? nn * A : 0), oY = cv.take(host ? nn * qi : 0), oV = cv.take(nn * qi), oym = cv.take(qi),
                 oK = cv.take((size_t)pi * qi);
    JCH_TRY(jch_reserve(ctx, ctx->xt_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->xt_ws.ptr;
    double *G = ws + oG, *wn = ws + ow, *mu = ws + omu, *cvd = ws + ocv, *xsd = ws + oxs, *trd = ws + otr;
    std::vector<double> xm((size_t)pi), xs((size_t)pi), cvh((size_t)pi);
    double trh = 0.0;
    jch_eig_lead_out eg;
    std::vector<double> Ph((size_t)pi * A), ym((size_t)qi), K((size_t)pi * qi);
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        xt_in in;
        JCH_TRY(xt_stage(ctx, loc, X, n, p, ldx, weights, ws + owr, &in));
        // ---- weights -> mu -> G (:83-91 without touching X)
        JCH_TRY(jch_launch_weights(ctx, in.dw, n, wn, ws + ohdr));
        JCH_TRY(jch_covsel_pass(ctx, in.dX, n, p, in.ldxd, nullptr, wn, 1, n, mu));
        JCH_TRY(jch_launch_xtdx(ctx, in.dX, n, pi, in.ldxd, mu, wn, G, p));
        hipLaunchKernelGGL(k_xt_diag, dim3((pi + XT_NT - 1) / XT_NT), dim3(XT_NT), 0, ctx->stream, G, p, pi, (int)(scal != 0), cvd, xsd);
        if (scal) hipLaunchKernelGGL(k_xt_rescale, dim3(jch_grid1(ctx, p * p)), dim3(XT_NT), 0, ctx->stream, G, p, pi, xsd);
        hipLaunchKernelGGL(k_xt_trace, dim3(1), dim3(XT_NT), 0, ctx->stream, G, p, pi, trd);
        JCH_HIP(ctx, hipGetLastError());
        JCH_HIP(ctx, hipMemcpyAsync(xm.data(), mu, sizeof(double) * (size_t)pi, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(xs.data(), xsd, sizeof(double) * (size_t)pi, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(cvh.data(), cvd, sizeof(double) * (size_t)pi, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(&trh, trd, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        // ---- the A leading eigenpairs of G: P and sv^2 (:95-98 by the eigen route)
        JCH_TRY(jch_eig_lead(ctx, G, p, p, nullptr, A, tol, maxit, &eg));
        JCH_HIP(ctx, hipMemcpyAsync(Ph.data(), eg.X, sizeof(double) * Ph.size(), hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        // ---- T = cscale(X, xmeans, xscales) P (:99 is the same matrix: sqrtD^-1 U S = Xc V)
        if (T) {
            double *Td = host ? ws + oT : T;
            JCH_TRY(jch_transform(ctx, JCH_LOC_DEVICE, in.dX, n, p, in.ldxd, xm.data(), xs.data(), Ph.data(), A, Td, n));
            if (host) JCH_HIP(ctx, hipMemcpyAsync(T, Td, sizeof(double) * nn * A, hipMemcpyDeviceToHost, ctx->stream));
        }
        // ---- pcr (src/pcr.jl:86-93): ymeans and Xs'D Yc, from which beta = diag(1 / sv^2) P' Xs'D Yc is host work (Xs = cscale(X))
        if (qi > 0) {
            const double *dY = Y;
            int64_t ldyd = ldy;
            JCH_TRY(jch_stage_in(ctx, host, ws + oY, n, q, &dY, &ldyd));
            JCH_TRY(jch_col_stats(ctx, JCH_LOC_DEVICE, dY, n, q, ldyd, in.dw, ym.data(), nullptr));
            JCH_HIP(ctx, hipMemcpyAsync(ws + oym, ym.data(), sizeof(double) * (size_t)qi, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_xt_dyc, dim3(jch_grid1(ctx, n * q)), dim3(XT_NT), 0, ctx->stream, dY, n, qi, ldyd, ws + oym, wn, ws + oV);
            JCH_HIP(ctx, hipGetLastError());
            JCH_TRY(jch_covsel_pass(ctx, in.dX, n, p, in.ldxd, mu, ws + oV, q, n, ws + oK));
            JCH_HIP(ctx, hipMemcpyAsync(K.data(), ws + oK, sizeof(double) * K.size(), hipMemcpyDeviceToHost, ctx->stream));
            JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if (ymeans) std::copy(ym.begin(), ym.end(), ymeans);
            if (xtdy)
                for (int k = 0; k < qi; ++k)
                    for (int j = 0; j < pi; ++j) xtdy[(size_t)j + (size_t)k * pi] = K[(size_t)j + (size_t)k * pi] / xs[j];
        }
        if (weights_norm) JCH_HIP(ctx, hipMemcpyAsync(weights_norm, wn, sizeof(double) * nn, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
        return JCH_OK;
    }));
    for (int e = 0; e < A; ++e) {
        const double ev = std::max(eg.theta[e], 0.0);   // `sv[sv .< 0] .= 0` (:98)
        if (eig) eig[e] = ev;
        if (sv) sv[e] = sqrt(ev);
        if (resid) resid[e] = eg.resid[e];
    }
    if (P) std::copy(Ph.begin(), Ph.end(), P);
    if (xmeans) std::copy(xm.begin(), xm.end(), xmeans);
    if (xscales) std::copy(xs.begin(), xs.end(), xscales);
    if (colvar) std::copy(cvh.begin(), cvh.end(), colvar);
    if (sstot) *sstot = trh;
    if (niter) *niter = eg.niter;
    if (nlv_out) *nlv_out = A;
    if (converged) *converged = eg.converged ? 1 : 0;   // the iteration's own decision (on |theta_1|)
    return JCH_OK;
}

// ---- spherical PCA (src/pcasph.jl:60-92) ----------------------------------------------------------------------------------------
// dw[i] = wn[i] / r[i]^2: the row weight of the Gram of the rows projected on the unit sphere; a row AT the centre (r = 0) gets 0
__global__ __launch_bounds__(XT_NT) void k_ph_rowweight(const double *__restrict__ r, const double *__restrict__ wn, int64_t n, double *__restrict__ dw)
{
    for (int64_t i = (int64_t)blockIdx.x * XT_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * XT_NT) {
        const double ri = r[i];
        dw[i] = ri == 0.0 ? 0.0 : wn[i] / (ri * ri);
    }
}

// *out = the number of rows with r = 0 (one workgroup, integer counts)
__global__ __launch_bounds__(XT_NT) void k_ph_nzero(const double *__restrict__ r, int64_t n, long long *out)
{
    __shared__ long long scr[XT_NT];
    long long c = 0;
    for (int64_t i = threadIdx.x; i < n; i += XT_NT) c += r[i] == 0.0 ? 1 : 0;
    scr[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long s = 0;
        for (int t = 0; t < XT_NT; ++t) s += scr[t];
        *out = s;
    }
}

// zT[i, k] = T[i, k] / r[i] (`zX * P`, :84), a zero row where r = 0
__global__ __launch_bounds__(XT_NT) void k_ph_divrows(const double *__restrict__ T, const double *__restrict__ r, int64_t n, int a, double *__restrict__ zT)
{
    const int64_t tot = n * a;
    for (int64_t e = (int64_t)blockIdx.x * XT_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * XT_NT) {
        const double ri = r[e % n];
        zT[e] = ri == 0.0 ? 0.0 : T[e] / ri;
    }
}

extern "C" int32_t jch_pcasph_fit(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *weights, int32_t nlv, int32_t typc,
                                  double delta, int32_t maxit_med, int32_t scal, double tol, int32_t maxit, double *T, double *P, double *sv, double *eig,
                                  double *xmeans, double *xscales, double *weights_norm, double *sstot, double *colvar, int32_t *niter_med,
                                  int32_t *converged_med, int32_t *niter, double *resid, int32_t *converged, int32_t *nlv_out, int64_t *nzero)
{
    static const char *who = "jch_pcasph_fit";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(xt_check(ctx, who, loc, X, n, p, ldx));
    if (nlv < 1) return jch_fail(ctx, JCH_EINVAL, "%s: nlv = %d must be >= 1", who, nlv);
    if (maxit < 1 || maxit_med < 1) return jch_fail(ctx, JCH_EINVAL, "%s: maxit = %d and maxit_med = %d must be >= 1", who, maxit, maxit_med);
    if (!(tol > 0.0) || !(delta > 0.0)) return jch_fail(ctx, JCH_EINVAL, "%s: tol and delta must be > 0", who);
    if (typc != JCH_CENT_MEDSPA && typc != JCH_CENT_MEAN) return jch_fail(ctx, JCH_EINVAL, "%s: bad typc %d", who, typc);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST;
    const int pi = (int)p;
    const int A = (int)std::min<int64_t>(nlv, std::min(n, p));   // src/pcasph.jl:63
    const size_t nn = (size_t)n;
    jch_carve cv;
    const size_t oG = cv.take((size_t)p * p), ow = cv.take(nn), owr = cv.take(nn), omean = cv.take(pi), omu = cv.take(pi), ostd = cv.take(pi), ohdr = cv.take(8),
                 otr = cv.take(8), ocnt = cv.take(8), orr = cv.take(nn), odw = cv.take(nn), oT = cv.take(nn * A), oz = cv.take(nn * A), omed = cv.take(A),
                 omad = cv.take(A);
    JCH_TRY(jch_reserve(ctx, ctx->xt_ws, sizeof(double) * cv.off));
    JCH_TRY(jch_colselect_reserve(ctx, p));
    double *ws = (double *)ctx->xt_ws.ptr;
    double *G = ws + oG, *wn = ws + ow, *mean = ws + omean, *mu = ws + omu, *sd = ws + ostd, *trd = ws + otr, *rr = ws + orr, *dw = ws + odw, *Tw = ws + oT,
           *zT = ws + oz;
    long long *cntd = (long long *)(ws + ocnt);
    std::vector<double> xm((size_t)pi), xs((size_t)pi, 1.0), sdh((size_t)pi), Ph((size_t)pi * A), madh((size_t)A);
    std::vector<int> perm((size_t)A);
    double trh = 0.0;
    long long cnth = 0;
    int32_t nit_med = 0, conv_med = 1;
    jch_eig_lead_out eg;
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        xt_in in;
        JCH_TRY(xt_stage(ctx, loc, X, n, p, ldx, weights, ws + owr, &in));
        // ---- weights, the weighted mean and colstd about it (:64, :68, :72)
        JCH_TRY(jch_launch_weights(ctx, in.dw, n, wn, ws + ohdr));
        JCH_TRY(jch_covsel_pass(ctx, in.dX, n, p, in.ldxd, nullptr, wn, 1, n, mean));
        JCH_TRY(jch_launch_moments(ctx, in.dX, in.ldxd, nullptr, 0, wn, n, pi, 0, mean, sd));
        // ---- xmeans (:65-69)
        if (typc == JCH_CENT_MEDSPA) JCH_TRY(jch_spatial_median_dev(ctx, in.dX, n, pi, in.ldxd, delta, maxit_med, mu, nullptr, &nit_med, nullptr, &conv_med));
        else JCH_HIP(ctx, hipMemcpyAsync(mu, mean, sizeof(double) * (size_t)pi, hipMemcpyDeviceToDevice, ctx->stream));
        // ---- r = the row norms of Xs (:79), G = Xs' diag(w / r^2) Xs (:80-82 is the SVD of sqrtw .* zX)
        JCH_TRY(jch_launch_weiszfeld_dist(ctx, in.dX, n, pi, in.ldxd, mu, scal ? sd : nullptr, rr));
        hipLaunchKernelGGL(k_ph_rowweight, dim3(jch_grid1(ctx, n)), dim3(XT_NT), 0, ctx->stream, (const double *)rr, (const double *)wn, n, dw);
        hipLaunchKernelGGL(k_ph_nzero, dim3(1), dim3(XT_NT), 0, ctx->stream, (const double *)rr, n, cntd);
        JCH_TRY(jch_launch_xtdx(ctx, in.dX, n, pi, in.ldxd, mu, dw, G, p));
        if (scal) hipLaunchKernelGGL(k_xt_rescale, dim3(jch_grid1(ctx, p * p)), dim3(XT_NT), 0, ctx->stream, G, p, pi, (const double *)sd);
        hipLaunchKernelGGL(k_xt_trace, dim3(1), dim3(XT_NT), 0, ctx->stream, (const double *)G, p, pi, trd);
        JCH_HIP(ctx, hipGetLastError());
        JCH_HIP(ctx, hipMemcpyAsync(xm.data(), mu, sizeof(double) * (size_t)pi, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(sdh.data(), sd, sizeof(double) * (size_t)pi, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(&trh, trd, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(&cnth, cntd, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        // ---- P (:83)
        JCH_TRY(jch_eig_lead(ctx, G, p, p, nullptr, A, tol, maxit, &eg));
        JCH_HIP(ctx, hipMemcpyAsync(Ph.data(), eg.X, sizeof(double) * Ph.size(), hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (scal) xs = sdh;
        // ---- T = Xs P (:86), zT = T / r (:84), sv = colmad(zT) (:85)
        JCH_TRY(jch_transform(ctx, JCH_LOC_DEVICE, in.dX, n, p, in.ldxd, xm.data(), xs.data(), Ph.data(), A, Tw, n));
        hipLaunchKernelGGL(k_ph_divrows, dim3(jch_grid1(ctx, n * A)), dim3(XT_NT), 0, ctx->stream, (const double *)Tw, (const double *)rr, n, A, zT);
        JCH_HIP(ctx, hipGetLastError());
        JCH_TRY(jch_launch_col_median_mad(ctx, zT, n, A, n, ws + omed, ws + omad));
        JCH_HIP(ctx, hipMemcpyAsync(madh.data(), ws + omad, sizeof(double) * (size_t)A, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        // ---- the order of sv, descending, ties in eigen order (:87-90)
        for (int e = 0; e < A; ++e) perm[e] = e;
        std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return madh[a] > madh[b]; });
        if (T)
            for (int e = 0; e < A; ++e)
                JCH_HIP(ctx, hipMemcpyAsync(T + (size_t)e * nn, Tw + (size_t)perm[e] * nn, sizeof(double) * nn, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                            ctx->stream));
        if (weights_norm) JCH_HIP(ctx, hipMemcpyAsync(weights_norm, wn, sizeof(double) * nn, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, ctx->stream));
        return JCH_OK;
    }));
    for (int e = 0; e < A; ++e) {
        const int s = perm[e];
        if (sv) sv[e] = madh[s];
        if (eig) eig[e] = eg.theta[s];
        if (resid) resid[e] = eg.resid[s];
        if (P) std::copy(Ph.begin() + (size_t)s * pi, Ph.begin() + (size_t)(s + 1) * pi, P + (size_t)e * pi);
    }
    if (xmeans) std::copy(xm.begin(), xm.end(), xmeans);
    if (xscales) std::copy(xs.begin(), xs.end(), xscales);
    if (colvar)
        for (int j = 0; j < pi; ++j) colvar[j] = sdh[j] * sdh[j];
    if (sstot) *sstot = trh;
    if (niter_med) *niter_med = nit_med;
    if (converged_med) *converged_med = conv_med;
    if (niter) *niter = eg.niter;
    if (nlv_out) *nlv_out = A;
    if (converged) *converged = eg.converged ? 1 : 0;
    if (nzero) *nzero = (int64_t)cnth;
    return JCH_OK;
}
