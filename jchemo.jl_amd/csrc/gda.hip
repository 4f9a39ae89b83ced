// Gaussian discrimination on raw X: class means and within-class covariances, the Cholesky factors of one or several covariances with their
// inverse factors, and squared Mahalanobis distances under such factors (src/matW.jl, src/dmnorm.jl:107-143, src/lda.jl, src/qda.jl, `mahsqchol`
// of src/distances.jl:104-126).  jch_class_cov, jch_gauss_factor, jch_mahsq_chol of include/jchemo_hip.h; DESIGN.md §24.
//
// jch_class_cov and jch_gauss_factor are orchestration of what exists: per class jch_launch_weights, jch_covsel_pass (the mean) and
// jch_launch_xtdx (the centred Gram of a row range of the grouped Z, centring in registers), then k_gd_combine for W; per factor
// jch_launch_chol_factor on a working copy and jch_launch_chol_inv_t (chol.hip) for L^-T.
//
// jch_mahsq_chol is the new kernel:   out[i, c] = sum_j z_j^2,  z_j = sum_{k <= j} (Xq[i, k] - Mu[c, k]) Uinv_f[k, j],  f = (nfac == 1 ? 0 : c)
//   k_gd_ut     once per call: Ut_f[j, k] = Uinv_f[k, j] for k <= j < p, exact zeros elsewhere, j padded to a multiple of 128 and k to a multiple of
//               16.  The strictly lower triangle of Uinv_f is never read, so whatever a caller left there (garbage, NaN) cannot reach a result;
//               and a k-column of Ut is contiguous in j, so the operand loads of the main kernel are aligned 16-byte loads with no edge cases.
//   k_gd_mahsq  one workgroup of 4 waves per (128 query rows, centre), t128_mma of tile128_dev.h (4 x 4 v_mfma_f64_16x16x4_f64 tiles per wave,
//               16-column chunks of both operands through LDS, double-buffered).  The operand along the contiguous direction is the centred query
//               rows: the loader subtracts Mu[c, k] — the difference is taken BEFORE the product, never x U - mu U: spectra sit at a large offset
//               from a small within-class spread, and that is where the digits would go — and replaces rows >= m and columns >= p by exact zeros
//               AFTER an unconditional load with clamped indices (a select, not a branch around a load: occ.hip records why).  The other operand
//               is the z-columns of Ut.  The workgroup walks the column tiles jt of 128 z-columns; tile jt multiplies only the
//               ceil(min(p, 128 (jt + 1)) / 16) chunks on or above its diagonal: the triangle halves the flops.  There is no m x p intermediate.
//   epilogue    a lane squares its 64 accumulators and adds them by query row (4 rows, 16 terms each, fixed order), the four lane >> 4 groups are
//               added as (g0 + g1) + (g2 + g3), the two waves that share a row as w0 + w1 through LDS, the column tiles in order.  No atomics:
//               two runs give identical bits, and so do host and device inputs and aligned and unaligned ones (VEC = false reads the same
//               values into the same registers with 8-byte loads).
//   A NaN at Xq[i, k] reaches row i of out only; rows >= m of Xq and of out are never read or written.  ncen is meant to be small (classes, not
//   observations: every centre re-reads the query rows), <= 65535.  Row tiles are not split over column tiles: m / 128 x ncen workgroups fill
//   the card from m of a few thousand on; below that the call is microseconds anyway.
// gfx950, hipcc -O3: k_gd_mahsq<true> 251 VGPRs, k_gd_mahsq<false> 253 VGPRs, no scratch; 75 776 B of LDS (T128_LDS_BYTES + the row sums): two
// workgroups per CU (2 waves per SIMD), as __launch_bounds__(256, 2) asks.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "jch_internal.h"
#include "tile128_dev.h"

#define GD_MAXP 32768
#define GD_MAXC 65535
constexpr size_t GD_LDS_BYTES = T128_LDS_BYTES + sizeof(double) * 2 * T128_T;

// W = w G (first) or W + w G: the reference's `W = W + w[i] * Wi[i]` (src/matW.jl:69-73), product and sum rounded separately
__global__ __launch_bounds__(256) void k_gd_combine(double *__restrict__ W, int64_t ldw, const double *__restrict__ G, int p, double w, int first)
{
    const int64_t tot = (int64_t)p * p;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < tot; e += (int64_t)gridDim.x * 256) {
        const int64_t j = e / p, i = e - j * p;
        const double t = __dmul_rn(w, G[e]);
        double *o = W + (size_t)i + (size_t)j * (size_t)ldw;
        *o = first ? t : __dadd_rn(*o, t);
    }
}

// d[i] = A[i, i]
__global__ __launch_bounds__(256) void k_gd_diag(const double *__restrict__ A, int64_t lda, int p, double *__restrict__ d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < p) d[i] = A[(size_t)i * (size_t)(lda + 1)];
}

// Ut_f (pp x pk, ld pp) = the zero-padded transpose of the upper triangle of Uinv_f (p x p, ld ldu); grid (pp / 32, ceil(pk / 32), nfac), block 32 x 8
__global__ __launch_bounds__(256) void k_gd_ut(const double *__restrict__ U, int64_t ldu, int64_t ustride, int p, double *__restrict__ Ut, int64_t pp, int pk)
{
    __shared__ double tile[32][33];
    const double *Uf = U + (size_t)blockIdx.z * (size_t)ustride;
    double *Utf = Ut + (size_t)blockIdx.z * (size_t)pp * (size_t)pk;
    const int jb = blockIdx.x * 32, kb = blockIdx.y * 32, tx = threadIdx.x, ty = threadIdx.y;
    for (int r = ty; r < 32; r += 8) {   // tile[j - jb][k - kb], read along k
        const int j = jb + r, k = kb + tx;
        tile[r][tx] = (k <= j && j < p) ? Uf[(size_t)k + (size_t)j * (size_t)ldu] : 0.0;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {   // written along j
        const int k = kb + r, j = jb + tx;
        if (k < pk) Utf[(size_t)j + (size_t)k * (size_t)pp] = tile[tx][r];
    }
}

template <bool VEC>
__global__ __launch_bounds__(256, 2) void k_gd_mahsq(const double *__restrict__ Xq, int64_t m, int p, int64_t ldq, const double *__restrict__ mu, int pk,
                                                     const double *__restrict__ Ut, int64_t pp, size_t fstride, double *__restrict__ out, int64_t ldo)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double *rs = lds + 4 * T128_KB * T128_LD;   // [2][128]: the row sums of the two waves that share a row
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int qj = wv >> 1, qi = wv & 1;
    const int64_t i0 = (int64_t)blockIdx.x * T128_T;
    const double *muc = mu + (size_t)blockIdx.y * (size_t)pk;
    const double *U = Ut + (size_t)blockIdx.y * fstride;
    const int ntile = (p + T128_T - 1) / T128_T;
    double tot = 0.0;
    for (int jt = 0; jt < ntile; ++jt) {
        const int j0 = jt * T128_T;
        const int nch = (std::min(p, j0 + T128_T) + T128_KB - 1) / T128_KB;   // k < 16 nch <= pk
        t128_v4d acc[4][4];   // acc[mj][ni][reg]: z-column j0 + 64 qj + 16 mj + (lane >> 4) + 4 reg of query row i0 + 64 qi + 16 ni + (lane & 15)
        t128_mma(
            lds, nch,
            [&](int k, int c) { return *reinterpret_cast<const t128_v2d *>(U + (size_t)k * (size_t)pp + (size_t)(j0 + c)); },
            [&](int k, int c) {
                const int kc = std::min(k, p - 1);
                const double muv = muc[kc];
                const double *col = Xq + (size_t)kc * (size_t)ldq;
                const int64_t r = i0 + c;
                t128_v2d v;
                if (VEC) {   // m even: the last pair starts at m - 2
                    v = *reinterpret_cast<const t128_v2d *>(col + std::min<int64_t>(r, m - 2));
                } else {
                    v.x = col[std::min<int64_t>(r, m - 1)];
                    v.y = col[std::min<int64_t>(r + 1, m - 1)];
                }
                const bool kin = k < p;
                v.x = (kin && r < m) ? v.x - muv : 0.0;
                v.y = (kin && r + 1 < m) ? v.y - muv : 0.0;
                return v;
            },
            acc);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            double s = 0.0;
#pragma unroll
            for (int mj = 0; mj < 4; ++mj)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) s = fma(acc[mj][ni][reg], acc[mj][ni][reg], s);
            s += __shfl_xor(s, 16);   // g0 + g1 | g2 + g3
            s += __shfl_xor(s, 32);   // (g0 + g1) + (g2 + g3) in every group (the sum of two doubles does not depend on their order)
            if (lane < 16) rs[qj * T128_T + 64 * qi + 16 * ni + lane] = s;
        }
        __syncthreads();
        if (tid < T128_T) tot += rs[tid] + rs[T128_T + tid];
        // (rs is written again only behind the barriers of the next tile's t128_mma)
    }
    if (tid < T128_T && i0 + tid < m) out[(size_t)(i0 + tid) + (size_t)blockIdx.y * (size_t)ldo] = tot;
}

namespace {

int32_t gd_common(jch_ctx *ctx, const char *who, int32_t loc)
{
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (ctx->nranks > 1) return jch_fail(ctx, JCH_EINVAL, "%s: one rank only (communicator of %d)", who, ctx->nranks);
    return JCH_OK;
}

}  // namespace

// ---------------------------------------------------------------- C ABI
extern "C" int32_t jch_class_cov(jch_ctx *ctx, int32_t loc, const double *Z, int64_t n, int64_t p, int64_t ldz, const int64_t *cls_start, int32_t ncls,
                                 double *Wi, double *W, double *ct)
{
    static const char *who = "jch_class_cov";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(gd_common(ctx, who, loc));
    if (!Z || !cls_start) return jch_fail(ctx, JCH_EINVAL, "%s: NULL argument", who);
    if (n < 1 || p < 1 || ncls < 1 || ldz < n)
        return jch_fail(ctx, JCH_EINVAL, "%s: bad shape (n=%lld p=%lld ncls=%d ldz=%lld)", who, (long long)n, (long long)p, ncls, (long long)ldz);
    if (p > GD_MAXP || ncls > GD_MAXC || n >= ((int64_t)1 << 40)) return jch_fail(ctx, JCH_EINVAL, "%s: shape too large (p <= %d, ncls <= %d)", who, GD_MAXP, GD_MAXC);
    if (cls_start[0] != 0 || cls_start[ncls] != n) return jch_fail(ctx, JCH_EINVAL, "%s: cls_start must run from 0 to n", who);
    bool one_row = false;
    for (int c = 0; c < ncls; ++c) {
        const int64_t nc = cls_start[c + 1] - cls_start[c];
        if (nc < 1) return jch_fail(ctx, JCH_EINVAL, "%s: class %d is empty (or cls_start decreases)", who, c);
        one_row = one_row || nc == 1;
    }
    const bool host = loc == JCH_LOC_HOST, need_g = Wi || W;
    const bool own_g = need_g && (host || !Wi);   // the class covariance goes through the workspace
    const size_t pp = (size_t)p * (size_t)p;
    const int64_t ldzs = (n + 1) & ~(int64_t)1;
    jch_carve cv;
    const size_t o_wn = cv.take((size_t)n), o_hdr = cv.take(8), o_mu = cv.take((size_t)ncls * (size_t)p), o_mua = cv.take(one_row && need_g ? (size_t)p : 0),
                 o_g = cv.take(own_g ? pp : 0), o_ga = cv.take(one_row && need_g ? pp : 0), o_w = cv.take(W && host ? pp : 0),
                 o_z = cv.take(host ? (size_t)ldzs * (size_t)p : 0);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    JCH_TRY(jch_reserve(ctx, ctx->gd_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->gd_ws.ptr;
    std::vector<double> hmu(ct ? (size_t)ncls * (size_t)p : 0);
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        const double *Zd = Z;
        int64_t ldzd = ldz;
        if (host) {
            JCH_TRY(jch_copy2d(ctx, ws + o_z, ldzs, Z, ldz, n, p, hipMemcpyHostToDevice));
            Zd = ws + o_z; ldzd = ldzs;
        }
        double *wn = ws + o_wn, *hdr = ws + o_hdr, *Wd = W ? (host ? ws + o_w : W) : nullptr;
        const unsigned gp = jch_grid1(ctx, (int64_t)pp);
        if (one_row && need_g) {   // cov(X; corrected = false) of all the rows, for the classes of one row (src/matW.jl:54-56)
            JCH_TRY(jch_launch_weights(ctx, nullptr, n, wn, hdr));
            JCH_TRY(jch_covsel_pass(ctx, Zd, n, p, ldzd, nullptr, wn, 1, n, ws + o_mua));
            JCH_TRY(jch_launch_xtdx(ctx, Zd, n, (int)p, ldzd, ws + o_mua, wn, ws + o_ga, p));
        }
        for (int c = 0; c < ncls; ++c) {
            const int64_t r0 = cls_start[c], nc = cls_start[c + 1] - r0;
            const double *Zc = Zd + r0;
            double *muc = ws + o_mu + (size_t)c * (size_t)p;
            double *Gc = own_g ? ws + o_g : (Wi ? Wi + (size_t)c * pp : nullptr);
            if (nc == 1) {   // the mean of one row is the row
                JCH_TRY(jch_copy2d(ctx, muc, 1, Zc, ldzd, 1, p, hipMemcpyDeviceToDevice));
                if (need_g) {
                    if (Wi) JCH_TRY(jch_copy2d(ctx, Wi + (size_t)c * pp, p, ws + o_ga, p, p, p, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
                    Gc = ws + o_ga;
                }
            } else {
                JCH_TRY(jch_launch_weights(ctx, nullptr, nc, wn, hdr));
                JCH_TRY(jch_covsel_pass(ctx, Zc, nc, p, ldzd, nullptr, wn, 1, nc, muc));
                if (need_g) {
                    JCH_TRY(jch_launch_xtdx(ctx, Zc, nc, (int)p, ldzd, muc, wn, Gc, p));
                    if (Wi && host) JCH_TRY(jch_copy2d(ctx, Wi + (size_t)c * pp, p, Gc, p, p, p, hipMemcpyDeviceToHost));
                }
            }
            if (Wd) {
                hipLaunchKernelGGL(k_gd_combine, dim3(gp), dim3(256), 0, ctx->stream, Wd, (int64_t)p, (const double *)Gc, (int)p, (double)nc / (double)n,
                                   c == 0 ? 1 : 0);
                JCH_HIP(ctx, hipGetLastError());
            }
        }
        if (W && host) JCH_TRY(jch_copy2d(ctx, W, p, Wd, p, p, p, hipMemcpyDeviceToHost));
        if (ct) JCH_HIP(ctx, hipMemcpyAsync(hmu.data(), ws + o_mu, sizeof(double) * hmu.size(), hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    }));
    if (ct)
        for (int c = 0; c < ncls; ++c)
            for (int64_t j = 0; j < p; ++j) ct[(size_t)c + (size_t)j * (size_t)ncls] = hmu[(size_t)c * (size_t)p + (size_t)j];
    return JCH_OK;
}

extern "C" int32_t jch_gauss_factor(jch_ctx *ctx, int32_t loc, const double *S, int64_t p, int64_t lds, int64_t sstride, int32_t nfac, double *Uinv,
                                    int64_t ldu, int64_t ustride, double *diagU, int32_t *info)
{
    static const char *who = "jch_gauss_factor";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(gd_common(ctx, who, loc));
    if (!S || !Uinv || !diagU || !info) return jch_fail(ctx, JCH_EINVAL, "%s: NULL argument", who);
    if (p < 1 || nfac < 1 || lds < p || ldu < p)
        return jch_fail(ctx, JCH_EINVAL, "%s: bad shape (p=%lld nfac=%d lds=%lld ldu=%lld)", who, (long long)p, nfac, (long long)lds, (long long)ldu);
    if (p > GD_MAXP || nfac > GD_MAXC) return jch_fail(ctx, JCH_EINVAL, "%s: shape too large (p <= %d, nfac <= %d)", who, GD_MAXP, GD_MAXC);
    if (nfac > 1 && (sstride < lds * (p - 1) + p || ustride < ldu * (p - 1) + p))
        return jch_fail(ctx, JCH_EINVAL, "%s: a stride shorter than one matrix (sstride=%lld ustride=%lld)", who, (long long)sstride, (long long)ustride);
    const bool host = loc == JCH_LOC_HOST;
    const size_t pp = (size_t)p * (size_t)p;
    jch_carve cv;
    const size_t o_a = cv.take(pp), o_w = cv.take(host ? pp : 0), o_d = cv.take((size_t)p * (size_t)nfac), o_i = cv.take(jch_ints_as_doubles((size_t)nfac));
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    JCH_TRY(jch_reserve(ctx, ctx->gd_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->gd_ws.ptr;
    int *idev = nullptr;
    JCH_TRY(jch_chol_info_word(ctx, &idev));
    std::vector<int32_t> hinfo((size_t)nfac, 0);
    const int32_t st = jch_synced(ctx, true, [&]() -> int32_t {
        double *A = ws + o_a, *dd = ws + o_d;
        int *infos = (int *)(ws + o_i);
        for (int f = 0; f < nfac; ++f) {
            JCH_TRY(jch_copy2d(ctx, A, p, S + (size_t)f * (size_t)sstride, lds, p, p, host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice));
            JCH_TRY(jch_launch_chol_factor(ctx, A, p, p, idev));
            double *Uf = Uinv + (size_t)f * (size_t)ustride;
            double *Wd = host ? ws + o_w : Uf;
            JCH_TRY(jch_launch_chol_inv_t(ctx, A, p, p, Wd, host ? p : ldu, idev));
            hipLaunchKernelGGL(k_gd_diag, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)A, p, (int)p, dd + (size_t)f * (size_t)p);
            JCH_HIP(ctx, hipGetLastError());
            JCH_HIP(ctx, hipMemcpyAsync(infos + f, idev, sizeof(int), hipMemcpyDeviceToDevice, ctx->stream));
            if (host) JCH_TRY(jch_copy2d(ctx, Uf, ldu, Wd, p, p, p, hipMemcpyDeviceToHost));
        }
        JCH_HIP(ctx, hipMemcpyAsync(diagU, dd, sizeof(double) * (size_t)p * (size_t)nfac, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(hinfo.data(), infos, sizeof(int) * (size_t)nfac, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    });
    ctx->chol_L = nullptr;   // the working copy is this call's own: no later solve is keyed to it
    JCH_TRY(st);
    memcpy(info, hinfo.data(), sizeof(int32_t) * (size_t)nfac);
    return JCH_OK;
}

extern "C" int32_t jch_mahsq_chol(jch_ctx *ctx, int32_t loc, const double *Xq, int64_t m, int64_t p, int64_t ldq, const double *Mu, int32_t ncen,
                                  const double *Uinv, int64_t ldu, int64_t ustride, int32_t nfac, double *out, int64_t ldo)
{
    static const char *who = "jch_mahsq_chol";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(gd_common(ctx, who, loc));
    if (!Xq || !Mu || !Uinv || !out) return jch_fail(ctx, JCH_EINVAL, "%s: NULL argument", who);
    if (m < 1 || p < 1 || ncen < 1 || ldq < m || ldu < p || ldo < m)
        return jch_fail(ctx, JCH_EINVAL, "%s: bad shape (m=%lld p=%lld ncen=%d ldq=%lld ldu=%lld ldo=%lld)", who, (long long)m, (long long)p, ncen, (long long)ldq,
                        (long long)ldu, (long long)ldo);
    if (nfac != 1 && nfac != ncen) return jch_fail(ctx, JCH_EINVAL, "%s: nfac=%d is neither 1 nor ncen=%d", who, nfac, ncen);
    if (p > GD_MAXP || ncen > GD_MAXC || m >= ((int64_t)1 << 36)) return jch_fail(ctx, JCH_EINVAL, "%s: shape too large (p <= %d, ncen <= %d)", who, GD_MAXP, GD_MAXC);
    if (nfac > 1 && ustride < ldu * (p - 1) + p) return jch_fail(ctx, JCH_EINVAL, "%s: ustride=%lld shorter than one factor", who, (long long)ustride);
    const bool host = loc == JCH_LOC_HOST;
    const int pi = (int)p, pk = (pi + T128_KB - 1) / T128_KB * T128_KB;
    const int64_t ppad = (p + T128_T - 1) / T128_T * T128_T, mq = (m + 1) & ~(int64_t)1;
    const size_t utsz = (size_t)ppad * (size_t)pk, pp = (size_t)p * (size_t)p;
    jch_carve cv;
    const size_t o_ut = cv.take(utsz * (size_t)nfac), o_mu = cv.take((size_t)ncen * (size_t)pk), o_q = cv.take(host ? (size_t)mq * (size_t)p : 0),
                 o_u = cv.take(host ? pp * (size_t)nfac : 0), o_o = cv.take(host ? (size_t)m * (size_t)ncen : 0);
    std::vector<double> hmu((size_t)ncen * (size_t)pk, 0.0);   // centre by centre, zero-padded to pk
    for (int c = 0; c < ncen; ++c)
        for (int k = 0; k < pi; ++k) hmu[(size_t)c * pk + k] = Mu[(size_t)c + (size_t)k * (size_t)ncen];
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    JCH_TRY(jch_reserve(ctx, ctx->gd_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->gd_ws.ptr;
    static jch_per_device_once attr;
    if (!attr.done(ctx->device)) {
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_gd_mahsq<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_gd_mahsq<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr.mark(ctx->device);
    }
    return jch_synced(ctx, true, [&]() -> int32_t {
        JCH_HIP(ctx, hipMemcpyAsync(ws + o_mu, hmu.data(), sizeof(double) * hmu.size(), hipMemcpyHostToDevice, ctx->stream));
        const double *Xd = Xq, *Ud = Uinv;
        int64_t ldqd = ldq, ldud = ldu, usd = ustride;
        double *od = out;
        int64_t ldod = ldo;
        if (host) {
            JCH_TRY(jch_copy2d(ctx, ws + o_q, mq, Xq, ldq, m, p, hipMemcpyHostToDevice));
            for (int f = 0; f < nfac; ++f)
                JCH_TRY(jch_copy2d(ctx, ws + o_u + (size_t)f * pp, p, Uinv + (size_t)f * (size_t)ustride, ldu, p, p, hipMemcpyHostToDevice));
            Xd = ws + o_q; ldqd = mq; Ud = ws + o_u; ldud = p; usd = (int64_t)pp; od = ws + o_o; ldod = m;
        }
        hipLaunchKernelGGL(k_gd_ut, dim3((unsigned)(ppad / 32), (unsigned)((pk + 31) / 32), (unsigned)nfac), dim3(32, 8), 0, ctx->stream, Ud, ldud, usd, pi,
                           ws + o_ut, ppad, pk);
        JCH_HIP(ctx, hipGetLastError());
        const dim3 grid((unsigned)((m + T128_T - 1) / T128_T), (unsigned)ncen);
        const size_t fstride = nfac == 1 ? 0 : utsz;
        const bool vec = ((uintptr_t)Xd % 16 == 0) && (ldqd % 2 == 0) && (m % 2 == 0);
        if (vec)
            hipLaunchKernelGGL(k_gd_mahsq<true>, grid, dim3(256), GD_LDS_BYTES, ctx->stream, Xd, m, pi, ldqd, (const double *)(ws + o_mu), pk,
                               (const double *)(ws + o_ut), ppad, fstride, od, ldod);
        else
            hipLaunchKernelGGL(k_gd_mahsq<false>, grid, dim3(256), GD_LDS_BYTES, ctx->stream, Xd, m, pi, ldqd, (const double *)(ws + o_mu), pk,
                               (const double *)(ws + o_ut), ppad, fstride, od, ldod);
        JCH_HIP(ctx, hipGetLastError());
        if (host) JCH_TRY(jch_copy2d(ctx, out, ldo, od, m, m, ncen, hipMemcpyDeviceToHost));
        return JCH_OK;
    });
}
