// Kernel PCA (src/kpca.jl:82-147): jch_kpca_fit and the panel utility jch_kc_panel (include/jchemo_hip.h).
//
// The reference takes svd(Kd) of the whole n x n matrix Kd = sqrtD Kc sqrtD and keeps its nlv leading triplets.  Here the
// leading eigenpairs of Kd come from block subspace iteration with Rayleigh-Ritz on the operator A(V) = sqrtw o (Kc (sqrtw o V)),
// one read of Kc per iteration:
//
//   k_kc_vt / k_kc_panel   W = Kc (sqrtw o Q): the n x b panel product on v_mfma_f64_16x16x4_f64 (below)
//   k_pc_part              block partials of Q' D^1/2 W (b x b) and of Z'Z, summed in block order by the one-workgroup kernels
//   k_pc_rr                H = sym(Q'AQ), Jacobi, Ritz pairs ordered by |theta| descending
//   k_pc_rot               X = Q S (Ritz vectors), W S (= Kc (sqrtw o X)), Z = A X and the residual partials |A x - theta x|^2
//   k_pc_svqb / k_pc_orth  SVQB orthonormalisation of the next block Z (twice), dependent directions refilled from a fixed
//                          pseudo-random reservoir
// Convergence is decided on the host from the residuals of the first nlv pairs; every reduction has a fixed order, so two fits
// are bitwise equal.  The iteration itself is jch_eig_lead (jch_internal.h): "a symmetric device matrix times a panel", with or without
// the row metric sqrtw.  jch_kpca_fit runs it on Kc with sqrtw, jch_pca_fit (xtdx.hip) on the p x p Gram without.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "jacobi_dev.h"

typedef double pc_v2d __attribute__((ext_vector_type(2)));
typedef double pc_v4d __attribute__((ext_vector_type(4)));

#define PC_NT 256
#define KC_TM 64          // rows of Kc (and of the output) per workgroup of the panel kernel
#define PC_RED_NB 64      // row blocks of the b x b partials
#define PC_LDS_B 64       // largest b whose Jacobi matrices live in LDS; beyond: global workspace

// ---- the hot path: out[i, l] = sum_j Kc[i, j] Vt[j, l] for i < n, l < bc (Kc n x n, ld ldk; Vt row-major jpad x 16 NB, zero rows
// from n on).  A workgroup owns KC_TM = 64 rows of the output: each of its 4 waves runs over its own quarter of every chunk of
// 16 U columns and keeps the 64 x 16 NB accumulators in registers; the four partial sums are added in wave order at the end, so
// every output is one workgroup's fixed-order sum.  MFMA operand A = Kc (rows i, k = j): lane (m = lane & 15, kq = lane >> 4) holds
// rows i0 + 2m + {0, 1} and i0 + 32 + 2m + {0, 1} of column j = jb + kq, i.e. two 16-byte loads per lane, 256 contiguous bytes
// per 16 lanes: the four row tiles u of the MFMA are the row sets {i0 + 32 (u >> 1) + 2m + (u & 1)}, which the epilogue undoes.
// Operand B = Vt (k = j, columns l): lane reads Vt[j, 16 g + m], 128 contiguous bytes per 16 lanes.  No LDS staging is needed for
// the operands: the loads of the next chunk are in flight in registers while the current one is multiplied.
// VEC: n even, ldk even and Kc 16-byte aligned (pair loads); otherwise one 8-byte load per row.
template <int NB, int U, bool VEC, bool CL>
__device__ __forceinline__ void kc_load(const double *__restrict__ K, int64_t n, int64_t ldk, const int64_t (&r)[4], const double *__restrict__ Vt,
                                        int bp, int64_t jb, int kq, int m, double (&A)[U][4], double (&B)[U][NB])
{
#pragma unroll
    for (int t = 0; t < U; ++t) {
        const int64_t j = jb + 4 * t + kq;
        const int64_t jk = CL ? std::min<int64_t>(j, n - 1) : j;   // tail chunk only: columns >= n meet zero rows of Vt
        const double *col = K + (size_t)jk * (size_t)ldk;
        if (VEC) {
            const pc_v2d x = __builtin_nontemporal_load(reinterpret_cast<const pc_v2d *>(col + r[0]));
            const pc_v2d y = __builtin_nontemporal_load(reinterpret_cast<const pc_v2d *>(col + r[2]));
            A[t][0] = x.x; A[t][1] = x.y; A[t][2] = y.x; A[t][3] = y.y;
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) A[t][u] = __builtin_nontemporal_load(col + r[u]);
        }
#pragma unroll
        for (int g = 0; g < NB; ++g) B[t][g] = Vt[(size_t)j * (size_t)bp + 16 * g + m];
    }
}

template <int NB, int U>
__device__ __forceinline__ void kc_mma(pc_v4d (&acc)[4][NB], const double (&A)[U][4], const double (&B)[U][NB])
{
#pragma unroll
    for (int t = 0; t < U; ++t)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int g = 0; g < NB; ++g) acc[u][g] = __builtin_amdgcn_mfma_f64_16x16x4f64(A[t][u], B[t][g], acc[u][g], 0, 0, 0);
}

template <int NB, int U, bool VEC>
__global__ __launch_bounds__(PC_NT) void k_kc_panel(const double *__restrict__ K, int64_t n, int64_t ldk, const double *__restrict__ Vt,
                                                    int64_t nfull, int64_t nsc, int bc, double *__restrict__ out, int64_t ldo)
{
    __shared__ double red[3][16][64];
    constexpr int bp = 16 * NB;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = lane & 15, kq = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * KC_TM;
    // the lane's rows, clamped into [0, n) so that the last workgroup's loads stay inside Kc (those outputs are not stored)
    int64_t r[4];
    if (VEC) {
        const int64_t a = std::min<int64_t>(i0 + 2 * m, n - 2), b = std::min<int64_t>(i0 + 32 + 2 * m, n - 2);
        r[0] = a; r[1] = a + 1; r[2] = b; r[3] = b + 1;
    } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = std::min<int64_t>(i0 + 32 * (u >> 1) + 2 * m + (u & 1), n - 1);
    }
    pc_v4d acc[4][NB];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int g = 0; g < NB; ++g) acc[u][g] = pc_v4d{0.0, 0.0, 0.0, 0.0};
    double ca[U][4], cb[U][NB], na[U][4], nb[U][NB];
    const int64_t sc = 16 * U, wo = 4 * U * wv;   // columns per chunk; the wave's offset inside a chunk
    if (nsc > 0) {
        if (nfull > 0) kc_load<NB, U, VEC, false>(K, n, ldk, r, Vt, bp, wo, kq, m, ca, cb);
        else kc_load<NB, U, VEC, true>(K, n, ldk, r, Vt, bp, wo, kq, m, ca, cb);
    }
    int64_t c = 0;
    for (; c + 1 < nfull; ++c) {   // main loop: chunk c + 1 (whole, no clamping) in flight while chunk c is multiplied
        kc_load<NB, U, VEC, false>(K, n, ldk, r, Vt, bp, (c + 1) * sc + wo, kq, m, na, nb);
        kc_mma<NB, U>(acc, ca, cb);
#pragma unroll
        for (int t = 0; t < U; ++t) {
#pragma unroll
            for (int u = 0; u < 4; ++u) ca[t][u] = na[t][u];
#pragma unroll
            for (int g = 0; g < NB; ++g) cb[t][g] = nb[t][g];
        }
    }
    for (; c + 1 < nsc; ++c) {     // the tail chunk (at most one)
        kc_load<NB, U, VEC, true>(K, n, ldk, r, Vt, bp, (c + 1) * sc + wo, kq, m, na, nb);
        kc_mma<NB, U>(acc, ca, cb);
#pragma unroll
        for (int t = 0; t < U; ++t) {
#pragma unroll
            for (int u = 0; u < 4; ++u) ca[t][u] = na[t][u];
#pragma unroll
            for (int g = 0; g < NB; ++g) cb[t][g] = nb[t][g];
        }
    }
    if (nsc > 0) kc_mma<NB, U>(acc, ca, cb);
    // waves 1..3 hand their sums to wave 0 through LDS, one 16-column group at a time; wave 0 adds them in wave order and stores.
    // acc[u][g][reg] at lane (m, kq) = out[i0 + 32 (u >> 1) + 2 (kq + 4 reg) + (u & 1), 16 g + m]  (f64 C/D: col = lane & 15,
    // row = (lane >> 4) + 4 reg)
#pragma unroll
    for (int g = 0; g < NB; ++g) {
        if (wv > 0)
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) red[wv - 1][u * 4 + reg][lane] = acc[u][g][reg];
        __syncthreads();
        if (wv == 0) {
            const int l = 16 * g + m;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const double s = ((acc[u][g][reg] + red[0][u * 4 + reg][lane]) + red[1][u * 4 + reg][lane]) + red[2][u * 4 + reg][lane];
                    const int64_t i = i0 + 32 * (u >> 1) + 2 * (kq + 4 * reg) + (u & 1);
                    if (i < n && l < bc) out[(size_t)i + (size_t)l * (size_t)ldo] = s;
                }
        }
        __syncthreads();
    }
}

// Vt[j, l] (row-major, jpad x bp) = d[j] V[j, l] for j < n, l < bc; zero elsewhere (d = null: 1)
__global__ __launch_bounds__(PC_NT) void k_kc_vt(const double *__restrict__ V, int64_t ldv, int64_t n, int bc, const double *__restrict__ d,
                                                 double *__restrict__ Vt, int bp, int64_t jpad)
{
    const int64_t tot = jpad * bp;
    for (int64_t e = (int64_t)blockIdx.x * PC_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * PC_NT) {
        const int64_t l = e / jpad, j = e - l * jpad;
        double v = 0.0;
        if (j < n && l < bc) v = d ? d[j] * V[(size_t)j + (size_t)l * (size_t)ldv] : V[(size_t)j + (size_t)l * (size_t)ldv];
        Vt[(size_t)j * bp + l] = v;
    }
}

namespace {

template <int NB>
int32_t launch_panel_nb(jch_ctx *ctx, const double *K, int64_t n, int64_t ldk, const double *Vt, int bc, double *out, int64_t ldo, bool vec)
{
    constexpr int U = NB <= 2 ? 8 : 4;
    const int64_t sc = 16 * U, nsc = (n + sc - 1) / sc, nfull = n / sc;
    const unsigned grid = (unsigned)((n + KC_TM - 1) / KC_TM);
    if (vec)
        hipLaunchKernelGGL((k_kc_panel<NB, U, true>), dim3(grid), dim3(PC_NT), 0, ctx->stream, K, n, ldk, Vt, nfull, nsc, bc, out, ldo);
    else
        hipLaunchKernelGGL((k_kc_panel<NB, U, false>), dim3(grid), dim3(PC_NT), 0, ctx->stream, K, n, ldk, Vt, nfull, nsc, bc, out, ldo);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

}  // namespace

int32_t jch_launch_kc_panel(jch_ctx *ctx, const double *Kc, int64_t n, int64_t ldk, const double *V, int64_t ldv, int b, const double *d,
                            double *out, int64_t ldo)
{
    if (n < 1 || b < 1) return JCH_OK;
    const int64_t jpad = (n + 127) / 128 * 128;   // a whole number of chunks for every U (16 U <= 128)
    JCH_TRY(jch_reserve(ctx, ctx->kc_vt, sizeof(double) * (size_t)jpad * 64));
    double *Vt = (double *)ctx->kc_vt.ptr;
    const bool vec = n >= 2 && (n % 2) == 0 && (ldk % 2) == 0 && ((uintptr_t)Kc % 16) == 0;
    for (int c0 = 0; c0 < b; c0 += 64) {
        const int bc = std::min(64, b - c0), NB = (bc + 15) / 16;
        hipLaunchKernelGGL(k_kc_vt, dim3(jch_grid1(ctx, jpad * 16 * NB)), dim3(PC_NT), 0, ctx->stream, V + (size_t)c0 * (size_t)ldv, ldv, n, bc, d, Vt,
                           16 * NB, jpad);
        JCH_HIP(ctx, hipGetLastError());
        double *oc = out + (size_t)c0 * (size_t)ldo;
        switch (NB) {
        case 1: JCH_TRY(launch_panel_nb<1>(ctx, Kc, n, ldk, Vt, bc, oc, ldo, vec)); break;
        case 2: JCH_TRY(launch_panel_nb<2>(ctx, Kc, n, ldk, Vt, bc, oc, ldo, vec)); break;
        case 3: JCH_TRY(launch_panel_nb<3>(ctx, Kc, n, ldk, Vt, bc, oc, ldo, vec)); break;
        default: JCH_TRY(launch_panel_nb<4>(ctx, Kc, n, ldk, Vt, bc, oc, ldo, vec)); break;
        }
    }
    return JCH_OK;
}

extern "C" int32_t jch_kc_panel(jch_ctx *ctx, const double *Kc, int64_t n, const double *V, int64_t ldv, int32_t b, double *out, int64_t ldo)
{
    if (!ctx) return JCH_EINVAL;
    if (!Kc || !V || !out || n < 1 || b < 1 || ldv < n || ldo < n)
        return jch_fail(ctx, JCH_EINVAL, "jch_kc_panel: bad arguments (n=%lld b=%d ldv=%lld ldo=%lld)", (long long)n, b, (long long)ldv, (long long)ldo);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    JCH_TRY(jch_launch_kc_panel(ctx, Kc, n, n, V, ldv, b, nullptr, out, ldo));
    JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JCH_OK;
}

// ---- the small algebra around the pass

// part[blk][k b + l] = sum over the rows of block blk of A[i, k] d_i B[i, l] (d = null: 1).  Workgroup (tile of 16 x 16 entries,
// row block); 64-row slices of A and B staged through LDS, each thread one entry, rows in ascending order.
__global__ __launch_bounds__(PC_NT) void k_pc_part(const double *__restrict__ A, const double *__restrict__ B, const double *__restrict__ d,
                                                   int64_t n, int64_t ld, int b, int nt, int64_t chunk, double *__restrict__ part)
{
    __shared__ double As[64][17], Bs[64][17];
    const int tid = threadIdx.x, tk = tid >> 4, tl = tid & 15;
    const int kt = blockIdx.x / nt, lt = blockIdx.x - kt * nt;
    const int64_t r0 = (int64_t)blockIdx.y * chunk, r1 = std::min<int64_t>(n, r0 + chunk);
    double s = 0.0;
    for (int64_t s0 = r0; s0 < r1; s0 += 64) {
        for (int e = tid; e < 64 * 16; e += PC_NT) {
            const int row = e & 63, c = e >> 6;
            const int64_t i = s0 + row;
            const int ka = 16 * kt + c, la = 16 * lt + c;
            As[row][c] = (i < r1 && ka < b) ? A[(size_t)i + (size_t)ka * (size_t)ld] : 0.0;
            double bv = (i < r1 && la < b) ? B[(size_t)i + (size_t)la * (size_t)ld] : 0.0;
            if (d && i < r1) bv *= d[i];
            Bs[row][c] = bv;
        }
        __syncthreads();
#pragma unroll 8
        for (int row = 0; row < 64; ++row) s = fma(As[row][tk], Bs[row][tl], s);
        __syncthreads();
    }
    const int k = 16 * kt + tk, l = 16 * lt + tl;
    if (k < b && l < b) part[(size_t)blockIdx.y * b * b + (size_t)k * b + l] = s;
}

// the Jacobi workspace of the one-workgroup kernels: A0, A1, V0, V1 (b x (b + 1)), cs, lam, cvec (SVQB column scales), partner / flag
__host__ __device__ inline size_t pc_eig_doubles(int b) { return 4 * (size_t)b * (b + 1) + 2 * (size_t)(b + 2) + 2 * (size_t)b + (size_t)(b + 4); }

struct pc_eig_ws {
    double *A0, *A1, *V0, *V1, *cs, *lam, *cvec;
    int *partner, *flag;
};
__device__ inline pc_eig_ws pc_carve(double *base, int b)
{
    pc_eig_ws w;
    const int lda = b + 1;
    w.A0 = base; w.A1 = w.A0 + (size_t)b * lda; w.V0 = w.A1 + (size_t)b * lda; w.V1 = w.V0 + (size_t)b * lda;
    w.cs = w.V1 + (size_t)b * lda;
    w.lam = w.cs + 2 * (b + 2);
    w.cvec = w.lam + b;
    w.partner = reinterpret_cast<int *>(w.cvec + b);
    w.flag = w.partner + (b + 2);
    return w;
}

// A0 = sym(sum over the nrb blocks of part) (fixed order), then Jacobi: eigenvalues w.lam, eigenvectors the columns of w.V0
__device__ void pc_sym_eig(const double *__restrict__ part, int nrb, int b, pc_eig_ws &w, const double *scale)
{
    const int lda = b + 1;
    for (int e = threadIdx.x; e < b * b; e += PC_NT) {
        const int k = e / b, l = e - k * b;
        double hkl = 0.0, hlk = 0.0;
        for (int r = 0; r < nrb; ++r) {
            hkl += part[(size_t)r * b * b + (size_t)k * b + l];
            hlk += part[(size_t)r * b * b + (size_t)l * b + k];
        }
        double h = 0.5 * (hkl + hlk);
        if (scale) h *= scale[k] * scale[l];
        w.A0[k * lda + l] = h;
    }
    __syncthreads();
    jacobi_eig<PC_NT>(b, lda, w.A0, w.A1, w.V0, w.V1, w.cs, w.partner, w.flag);
    for (int k = threadIdx.x; k < b; k += PC_NT) w.lam[k] = w.A0[k * lda + k];
    __syncthreads();
}

// Rayleigh-Ritz: H = sym(Q'AQ) from the partials, H = S diag(theta) S' with the pairs ordered by |theta| descending (ties by index).
// S (b x b, column-major) and theta go to global memory.
__global__ __launch_bounds__(PC_NT) void k_pc_rr(const double *__restrict__ part, int nrb, int b, double *gws, double *__restrict__ S,
                                                 double *__restrict__ theta)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    pc_eig_ws w = pc_carve(b <= PC_LDS_B ? lds : gws, b);
    pc_sym_eig(part, nrb, b, w, nullptr);
    const int lda = b + 1;
    for (int k = threadIdx.x; k < b; k += PC_NT) {
        const double ak = fabs(w.lam[k]);
        int rank = 0;
        for (int j = 0; j < b; ++j) {
            const double aj = fabs(w.lam[j]);
            rank += (aj > ak || (aj == ak && j < k)) ? 1 : 0;
        }
        theta[rank] = w.lam[k];
        for (int i = 0; i < b; ++i) S[(size_t)i + (size_t)rank * b] = w.V0[i * lda + k];
    }
}

// SVQB: G = sym(Z'Z), c = diag(G)^-1/2 (0 for a zero column), c G c = U diag(lam) U'; M[:, e] = c o U[:, e] / sqrt(lam_e) when
// lam_e > 1e-14 max lam, else the direction is numerically dependent: M[:, e] = 0 and refill[e] = 1 (k_pc_orth fills that column
// from the reservoir; the second SVQB pass orthonormalises it against the rest)
__global__ __launch_bounds__(PC_NT) void k_pc_svqb(const double *__restrict__ part, int nrb, int b, double *gws, double *__restrict__ M,
                                                   double *__restrict__ refill)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    pc_eig_ws w = pc_carve(b <= PC_LDS_B ? lds : gws, b);
    double *cvec = w.cvec;
    for (int k = threadIdx.x; k < b; k += PC_NT) {
        double g = 0.0;
        for (int r = 0; r < nrb; ++r) g += part[(size_t)r * b * b + (size_t)k * b + k];
        cvec[k] = g > 1e-300 ? 1.0 / sqrt(g) : 0.0;
    }
    __syncthreads();
    pc_sym_eig(part, nrb, b, w, cvec);
    double lmax = 0.0;
    for (int k = 0; k < b; ++k) lmax = fmax(lmax, w.lam[k]);
    const int lda = b + 1;
    for (int e = threadIdx.x; e < b * b; e += PC_NT) {
        const int col = e / b, k = e - col * b;
        const double le = w.lam[col];
        const bool ok = le > 1e-14 * lmax && le > 0.0;
        M[(size_t)k + (size_t)col * b] = ok ? cvec[k] * w.V0[k * lda + col] / sqrt(le) : 0.0;
        if (k == 0) refill[col] = ok ? 0.0 : 1.0;
    }
}

// out[i, e] = refill[e] ? Res[i, e] : sum_k Z[i, k] M[k, e]; workgroup (256 rows, 16 columns e)
__global__ __launch_bounds__(PC_NT) void k_pc_orth(const double *__restrict__ Z, int64_t n, int b, const double *__restrict__ M,
                                                   const double *__restrict__ refill, const double *__restrict__ Res, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * PC_NT + threadIdx.x;
    const int e0 = 16 * blockIdx.y;
    if (i >= n) return;
    double acc[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) acc[jj] = 0.0;
    for (int k = 0; k < b; ++k) {
        const double z = Z[(size_t)i + (size_t)k * n];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj)
            if (e0 + jj < b) acc[jj] = fma(z, M[(size_t)k + (size_t)(e0 + jj) * b], acc[jj]);
    }
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
        const int e = e0 + jj;
        if (e < b) out[(size_t)i + (size_t)e * n] = refill[e] != 0.0 ? Res[(size_t)i + (size_t)e * n] : acc[jj];
    }
}

// After the pass W = Kc (sqrtw o Q) and the Ritz step (S, theta):  X = Q S, WS = W S, Z = sqrtw o WS (= A X) and the residual
// partials rpart[blk][e] = sum over the block's rows of (Z - theta_e X)[i, e]^2; workgroup (256 rows, 16 columns e)
__global__ __launch_bounds__(PC_NT) void k_pc_rot(const double *__restrict__ Q, const double *__restrict__ W, int64_t n, int b,
                                                  const double *__restrict__ S, const double *__restrict__ theta, const double *__restrict__ sw,
                                                  double *__restrict__ X, double *__restrict__ WS, double *__restrict__ Z, double *__restrict__ rpart)
{
    __shared__ double scr[PC_NT / 64];
    const int64_t i = (int64_t)blockIdx.x * PC_NT + threadIdx.x;
    const int e0 = 16 * blockIdx.y;
    const bool row = i < n;
    double xa[16], wa[16];
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) xa[jj] = wa[jj] = 0.0;
    if (row)
        for (int k = 0; k < b; ++k) {
            const double q = Q[(size_t)i + (size_t)k * n], wk = W[(size_t)i + (size_t)k * n];
#pragma unroll
            for (int jj = 0; jj < 16; ++jj)
                if (e0 + jj < b) {
                    const double s = S[(size_t)k + (size_t)(e0 + jj) * b];
                    xa[jj] = fma(q, s, xa[jj]);
                    wa[jj] = fma(wk, s, wa[jj]);
                }
        }
    const double swi = row ? (sw ? sw[i] : 1.0) : 0.0;   // (sw = null: no row metric; a product with 1.0 is exact)
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) {
        const int e = e0 + jj;
        if (e >= b) break;   // uniform over the workgroup
        const double z = swi * wa[jj], res = z - theta[e] * xa[jj];
        if (row) {
            X[(size_t)i + (size_t)e * n] = xa[jj];
            WS[(size_t)i + (size_t)e * n] = wa[jj];
            Z[(size_t)i + (size_t)e * n] = z;
        }
        const double s = jch_block_sum<PC_NT>(row ? res * res : 0.0, scr);
        if (threadIdx.x == 0) rpart[(size_t)blockIdx.x * b + e] = s;
    }
}

// sign rule of the outputs: sg[e] = +1 when the largest-|.| entry of X[:, e] (first index on ties) is >= 0, else -1; one workgroup
// per column
__global__ __launch_bounds__(PC_NT) void k_pc_sign(const double *__restrict__ X, int64_t n, double *__restrict__ sg)
{
    __shared__ double sv[PC_NT];
    __shared__ int64_t si[PC_NT];
    const double *x = X + (size_t)blockIdx.x * n;
    double best = -1.0;
    int64_t bi = n;
    for (int64_t i = threadIdx.x; i < n; i += PC_NT) {
        const double a = fabs(x[i]);
        if (a > best) { best = a; bi = i; }
    }
    sv[threadIdx.x] = best; si[threadIdx.x] = bi;
    __syncthreads();
    for (int s = PC_NT / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            const double o = sv[threadIdx.x + s];
            const int64_t oi = si[threadIdx.x + s];
            if (o > sv[threadIdx.x] || (o == sv[threadIdx.x] && oi < si[threadIdx.x])) { sv[threadIdx.x] = o; si[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) sg[blockIdx.x] = (si[0] < n && x[si[0]] < 0.0) ? -1.0 : 1.0;
}

// In place: the first A columns of X and of WS times sg (a product with +-1 is exact)
__global__ __launch_bounds__(PC_NT) void k_pc_apply_sign(double *__restrict__ X, double *__restrict__ WS, int64_t n, int A, const double *__restrict__ sg)
{
    const int64_t tot = n * A;
    for (int64_t e = (int64_t)blockIdx.x * PC_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * PC_NT) {
        const double s = sg[e / n];
        X[e] = s * X[e];
        WS[e] = s * WS[e];
    }
}

// From the sign-fixed Ritz vectors U and WS = Kc (sqrtw o U): P = sqrtw o U / sv (src/kpca.jl:113 `sqrtD * scale(U, sv)`),
// T = Kc P = WS / sv (:114), first A columns.  T may alias WS (element-wise).
__global__ __launch_bounds__(PC_NT) void k_pc_out(const double *__restrict__ U, const double *WS, int64_t n, int A, const double *__restrict__ theta,
                                                  const double *__restrict__ sw, double *__restrict__ P, double *T)
{
    const int64_t tot = n * A;
    for (int64_t e = (int64_t)blockIdx.x * PC_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * PC_NT) {
        const int64_t j = e / n, i = e - j * n;
        const double sv = sqrt(fabs(theta[j]));
        P[e] = sw[i] * U[e] / sv;
        T[e] = WS[e] / sv;
    }
}

// sstot = sum_i w_i Kc[i, i] (one workgroup)
__global__ __launch_bounds__(PC_NT) void k_pc_trace(const double *__restrict__ Kc, int64_t n, const double *__restrict__ w, double *out)
{
    __shared__ double scr[PC_NT / 64];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += PC_NT) a = fma(w[i], Kc[(size_t)i * (size_t)(n + 1)], a);
    a = jch_block_sum<PC_NT>(a, scr);
    if (threadIdx.x == 0) *out = a;
}

namespace {

struct pc_state {
    int64_t n; int b, nrb;
    int64_t chunk;
    double *part, *gws, *S, *theta, *M, *refill, *res;
    size_t lds;
};

int32_t launch_part(jch_ctx *ctx, const pc_state &s, const double *A, const double *B, const double *d)
{
    const int nt = (s.b + 15) / 16;
    hipLaunchKernelGGL(k_pc_part, dim3((unsigned)(nt * nt), (unsigned)s.nrb), dim3(PC_NT), 0, ctx->stream, A, B, d, s.n, s.n, s.b, nt, s.chunk, s.part);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

dim3 rows_grid(const pc_state &s) { return dim3((unsigned)((s.n + PC_NT - 1) / PC_NT), (unsigned)((s.b + 15) / 16)); }

// one SVQB pass: out = orthonormal basis of span(Z), dependent directions replaced by reservoir columns
int32_t svqb(jch_ctx *ctx, const pc_state &s, const double *Z, double *out)
{
    JCH_TRY(launch_part(ctx, s, Z, Z, nullptr));
    hipLaunchKernelGGL(k_pc_svqb, dim3(1), dim3(PC_NT), s.lds, ctx->stream, s.part, s.nrb, s.b, s.gws, s.M, s.refill);
    JCH_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pc_orth, rows_grid(s), dim3(PC_NT), 0, ctx->stream, Z, s.n, s.b, s.M, s.refill, s.res, out);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

// default oversampling of the block (b = min(n, roundup16(nlv + oversample))); JCH_KPCA_OVERSAMPLE overrides it (measurement knob)
int oversample()
{
    const int v = jch_knob("JCH_KPCA_OVERSAMPLE", 7);
    return v >= 0 && v <= 4096 ? v : 7;
}

}  // namespace

// The leading eigenpairs of the symmetric device matrix A (dim x dim, ld lda), or of sqrtw o A o sqrtw' when sqrtw is given, by block subspace
// iteration with Rayleigh-Ritz (jch_internal.h).  One read of A per iteration; convergence is decided on the host from the
// residuals of the first nlv pairs; every reduction has a fixed order.
int32_t jch_eig_lead(jch_ctx *ctx, const double *A, int64_t dim, int64_t lda, const double *sqrtw, int nlv, double tol, int maxit, jch_eig_lead_out *out)
{
    const int64_t n = dim;
    const size_t nn = (size_t)n;
    const int b = (int)std::min<int64_t>(n, ((int64_t)nlv + oversample() + 15) / 16 * 16);
    // ---- workspace (doubles, ld n): Q | W | Z | X | WS | reservoir (n x b each), partials and the small state
    pc_state st{};
    st.n = n; st.b = b;
    st.nrb = (int)std::max<int64_t>(1, std::min<int64_t>(PC_RED_NB, (n + 255) / 256));
    st.chunk = (n + st.nrb - 1) / st.nrb;
    const int64_t rblk = (n + PC_NT - 1) / PC_NT;
    jch_carve cv;
    const size_t nb = nn * b;
    const size_t oQ = cv.take(nb), oW = cv.take(nb), oZ = cv.take(nb), oX = cv.take(nb), oWS = cv.take(nb), oR = cv.take(nb),
                 opart = cv.take((size_t)st.nrb * b * b), ogws = cv.take(b > PC_LDS_B ? pc_eig_doubles(b) : 0), oS = cv.take((size_t)b * b), oth = cv.take(b),
                 oM = cv.take((size_t)b * b), orf = cv.take(b), orp = cv.take((size_t)rblk * b), osg = cv.take(nlv);
    JCH_TRY(jch_reserve(ctx, ctx->pc_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->pc_ws.ptr;
    double *Qd = ws + oQ, *Wd = ws + oW, *Zd = ws + oZ, *Xd = ws + oX, *WSd = ws + oWS, *rpart = ws + orp, *sg = ws + osg;
    st.part = ws + opart; st.gws = ws + ogws; st.S = ws + oS; st.theta = ws + oth; st.M = ws + oM; st.refill = ws + orf; st.res = ws + oR;
    st.lds = b <= PC_LDS_B ? sizeof(double) * pc_eig_doubles(b) : 0;
    static jch_per_device_once attr;
    if (!attr.done(ctx->device)) {
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_pc_rr, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        JCH_HIP(ctx, hipFuncSetAttribute((const void *)k_pc_svqb, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        attr.mark(ctx->device);
    }
    // ---- start block: uniform numbers from a fixed seed, orthonormalised (SVQB twice); the reservoir of refill columns
    JCH_TRY(jch_launch_fill(ctx, st.res, n, b, n, 0, n, 0x6b706361ULL));
    JCH_TRY(jch_launch_fill(ctx, Zd, n, b, n, 0, n, 0x6b706360ULL));
    JCH_TRY(svqb(ctx, st, Zd, Xd));
    JCH_TRY(svqb(ctx, st, Xd, Qd));
    std::vector<double> &th = out->theta;
    std::vector<double> &res = out->resid;
    th.assign((size_t)b, 0.0);
    res.assign((size_t)nlv, 0.0);
    std::vector<double> rp((size_t)rblk * b);
    int it = 0;
    bool conv = false;
    for (;;) {
        ++it;
        JCH_TRY(jch_launch_kc_panel(ctx, A, n, lda, Qd, n, b, sqrtw, Wd, n));          // W = A (sqrtw o Q)
        JCH_TRY(launch_part(ctx, st, Qd, Wd, sqrtw));                                    // Q' (sqrtw o W) partials
        hipLaunchKernelGGL(k_pc_rr, dim3(1), dim3(PC_NT), st.lds, ctx->stream, st.part, st.nrb, b, st.gws, st.S, st.theta);
        JCH_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_pc_rot, rows_grid(st), dim3(PC_NT), 0, ctx->stream, Qd, Wd, n, b, st.S, st.theta, sqrtw, Xd, WSd, Zd, rpart);
        JCH_HIP(ctx, hipGetLastError());
        JCH_HIP(ctx, hipMemcpyAsync(th.data(), st.theta, sizeof(double) * b, hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(rp.data(), rpart, sizeof(double) * rp.size(), hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
        conv = true;
        for (int e = 0; e < nlv; ++e) {
            double s = 0.0;
            for (int64_t r = 0; r < rblk; ++r) s += rp[(size_t)r * b + e];
            res[e] = sqrt(s);
            if (!(res[e] <= tol * fabs(th[0]))) conv = false;
        }
        if (conv || it >= maxit) break;
        JCH_TRY(svqb(ctx, st, Zd, Wd));   // next block: orth(A X), W is free until the next pass
        JCH_TRY(svqb(ctx, st, Wd, Qd));
    }
    // ---- the sign rule of the outputs, applied to the Ritz vectors and to W S alike
    hipLaunchKernelGGL(k_pc_sign, dim3((unsigned)nlv), dim3(PC_NT), 0, ctx->stream, Xd, n, sg);
    hipLaunchKernelGGL(k_pc_apply_sign, dim3(jch_grid1(ctx, n * nlv)), dim3(PC_NT), 0, ctx->stream, Xd, WSd, n, nlv, sg);
    JCH_HIP(ctx, hipGetLastError());
    out->b = b; out->niter = it; out->converged = conv;
    out->X = Xd; out->AX = WSd; out->theta_dev = st.theta; out->scratch = Qd;
    return JCH_OK;
}

namespace {

bool psd_kernel(int kind, double gamma, double coef0, int degree)
{
    if (kind == JCH_KERN_RBF) return gamma >= 0.0;
    return gamma >= 0.0 && (degree == 1 || coef0 >= 0.0);
}

}  // namespace

extern "C" int32_t jch_kpca_fit(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, double *X, int64_t n, int64_t p,
                                int64_t ldx, const double *weights, int32_t nlv, int32_t scal, double tol, int32_t maxit, double *K_out, double *T,
                                double *P, double *vtot, double *weights_norm, double *xscales, double *sv, double *eig, double *sstot,
                                int32_t *niter, double *resid, int32_t *nlv_out)
{
    static const char *who = "jch_kpca_fit";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(jch_check_kernel(ctx, who, kind, degree));
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (!X || n < 1 || p < 1 || ldx < n) return jch_fail(ctx, JCH_EINVAL, "%s: bad X (n=%lld p=%lld ldx=%lld)", who, (long long)n, (long long)p, (long long)ldx);
    if (nlv < 1) return jch_fail(ctx, JCH_EINVAL, "%s: nlv = %d must be >= 1", who, nlv);
    if (maxit < 1) return jch_fail(ctx, JCH_EINVAL, "%s: maxit = %d must be >= 1", who, maxit);
    if (!(tol > 0.0)) return jch_fail(ctx, JCH_EINVAL, "%s: tol must be > 0", who);
    if (n > (1 << 20)) return jch_fail(ctx, JCH_EINVAL, "%s: n=%lld too large", who, (long long)n);
    const int A = (int)std::min<int64_t>(n, nlv);   // src/kpca.jl:100 `nlv = min(nlv, n)`
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST;
    const size_t nn = (size_t)n;
    std::vector<double> xs((size_t)p, 1.0), xm((size_t)p);
    jch_eig_lead_out eg;
    double trh = NAN;
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        // ---- device views of X and the raw weights
        double *dX = X;
        int64_t ldxd = ldx;
        if (host) {
            JCH_TRY(jch_reserve(ctx, ctx->dk_x, sizeof(double) * nn * p));
            JCH_TRY(jch_copy2d(ctx, (double *)ctx->dk_x.ptr, n, X, ldx, n, p, hipMemcpyHostToDevice));
            dX = (double *)ctx->dk_x.ptr; ldxd = n;
        }
        // ---- the fit's own vectors (the eigensolver's panels live in ctx->pc_ws)
        jch_carve cv;
        const size_t ow = cv.take(nn), osw = cv.take(nn), ovt = cv.take(nn), owr = cv.take(nn), ohdr = cv.take(8), os = cv.take(8), oxs = cv.take((size_t)p),
                     otr = cv.take(8);
        JCH_TRY(jch_reserve(ctx, ctx->pc_vec, sizeof(double) * cv.off));
        double *ws = (double *)ctx->pc_vec.ptr;
        double *wn = ws + ow, *sw = ws + osw, *vt = ws + ovt, *wraw = ws + owr, *hdr = ws + ohdr, *sdev = ws + os, *xs_dev = ws + oxs, *trd = ws + otr;
        const double *dw = weights;
        if (host && weights) {
            JCH_HIP(ctx, hipMemcpyAsync(wraw, weights, sizeof(double) * nn, hipMemcpyHostToDevice, ctx->stream));
            dw = wraw;
        }
        JCH_TRY(jch_launch_weights(ctx, dw, n, wn, hdr));   // `mweight` (src/kpca.jl:93)
        JCH_TRY(jch_launch_sqrt(ctx, wn, n, sw));
        // ---- scal: xscales = colstd(X, w), X divided by them in place (:94-98)
        if (scal) {
            JCH_TRY(jch_col_stats(ctx, JCH_LOC_DEVICE, dX, n, p, ldxd, dw, xm.data(), xs.data()));
            JCH_HIP(ctx, hipMemcpyAsync(xs_dev, xs.data(), sizeof(double) * (size_t)p, hipMemcpyHostToDevice, ctx->stream));
            JCH_TRY(jch_launch_divcols(ctx, dX, ldxd, n, p, xs_dev));
            if (host) JCH_TRY(jch_copy2d(ctx, X, ldx, dX, n, n, p, hipMemcpyDeviceToHost));
        }
        // ---- K = kern(X, X), vtot = K w, Kc = K - vtot' - vtot + w'vtot (:99-103)
        JCH_TRY(jch_reserve(ctx, ctx->dk_k, sizeof(double) * nn * nn));
        double *Kc = (double *)ctx->dk_k.ptr;
        JCH_TRY(jch_launch_kp_centred_gram(ctx, kind, gamma, coef0, degree, dX, n, ldxd, nullptr, p, wn, K_out ? K_out : Kc, Kc, vt, sdev));
        // ---- the nlv leading eigenpairs of Kd = sqrtD Kc sqrtD
        JCH_TRY(jch_eig_lead(ctx, Kc, n, n, sw, A, tol, maxit, &eg));
        // ---- outputs (:104-114): U = sign-fixed Ritz vectors, P = sqrtD U / sv, T = Kc P; eig = |theta|, sv = sqrt(eig)
        double *Pd = eg.scratch, *WSd = eg.AX;
        hipLaunchKernelGGL(k_pc_out, dim3(jch_grid1(ctx, n * A)), dim3(PC_NT), 0, ctx->stream, eg.X, WSd, n, A, eg.theta_dev, sw, Pd, WSd);
        JCH_HIP(ctx, hipGetLastError());
        const bool psd = psd_kernel(kind, gamma, coef0, degree);
        if (psd) {
            hipLaunchKernelGGL(k_pc_trace, dim3(1), dim3(PC_NT), 0, ctx->stream, Kc, n, wn, trd);
            JCH_HIP(ctx, hipGetLastError());
        }
        const hipMemcpyKind dir = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (T) JCH_HIP(ctx, hipMemcpyAsync(T, WSd, sizeof(double) * nn * A, dir, ctx->stream));
        if (P) JCH_HIP(ctx, hipMemcpyAsync(P, Pd, sizeof(double) * nn * A, dir, ctx->stream));
        if (vtot) JCH_HIP(ctx, hipMemcpyAsync(vtot, vt, sizeof(double) * nn, dir, ctx->stream));
        if (weights_norm) JCH_HIP(ctx, hipMemcpyAsync(weights_norm, wn, sizeof(double) * nn, dir, ctx->stream));
        if (psd) JCH_HIP(ctx, hipMemcpyAsync(&trh, trd, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    }));
    const std::vector<double> &th = eg.theta, &res = eg.resid;
    const int it = eg.niter;
    for (int e = 0; e < A; ++e) {
        const double ev = fabs(th[e]);
        if (eig) eig[e] = ev;
        if (sv) sv[e] = sqrt(ev);
        if (resid) resid[e] = res[e];
    }
    if (sstot) *sstot = trh;
    if (xscales) std::copy(xs.begin(), xs.end(), xscales);
    if (niter) *niter = it;
    if (nlv_out) *nlv_out = A;
    return JCH_OK;
}
