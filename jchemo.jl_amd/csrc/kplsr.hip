// Kernel NIPALS PLS (src/kplsr.jl, Rosipal & Trejo 2001): jch_kplsr_fit, jch_kplsr_transform, jch_kplsr_predict
// (include/jchemo_hip.h).  The Gram comes from kgram.hip (symmetric path); this file centres it in the metric D and runs the LV loop
// with the deflation postponed: K_a = Z_a Kc Z_a', Z_a = z_{a-1} ... z_0, z_i = I - t_i dt_i', so that every LV reads Kc once
// (k_kp_pass) and the z_i are applied to n x q panels before and after that pass.
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "jch_internal.h"

#define KP_NT 256
#define KP_RED_NB 64        // row blocks of the skinny reductions (their partials are summed in block order by the consumer)
#define KP_MAXQ 1024        // q of the single-workgroup q x q iteration (vectors in LDS)

typedef double kp_v2d __attribute__((ext_vector_type(2)));

// ---- the hot path: out[j, l] = sum_i K[i, j] V[i, l] for l < rr  (K symmetric n x n, ld n: = (K V)[j, l]).  One block owns CB
// whole columns of K at a time, so every output is one block's fixed-order sum (no cross-block reduction, no atomics).  K is
// streamed with non-temporal loads; V (n x R, ld ldv; columns rr..R-1 are padding that is read but never written out) comes from
// the caches.  VEC: n even and 16-byte aligned columns, two rows per load.
template <int R, int CB, bool VEC>
__global__ __launch_bounds__(KP_NT) void k_kp_pass(const double *__restrict__ K, int64_t n, const double *__restrict__ V, int64_t ldv, int rr,
                                                   double *__restrict__ out, int64_t ldo, int64_t ngroups)
{
    __shared__ double red[KP_NT / 64][CB * R];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int64_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const int64_t j0 = g * CB;
        const double *col[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) col[c] = K + (size_t)std::min<int64_t>(j0 + c, n - 1) * (size_t)n;
        double acc[CB][R];
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
            for (int l = 0; l < R; ++l) acc[c][l] = 0.0;
        if (VEC) {
            const int64_t np = n >> 1;
            constexpr int U = CB * R <= 8 ? 2 : 1;
            int64_t ip = tid;
            for (; ip + (U - 1) * KP_NT < np; ip += U * KP_NT) {
                kp_v2d kv[U][CB];
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int c = 0; c < CB; ++c) kv[u][c] = __builtin_nontemporal_load(reinterpret_cast<const kp_v2d *>(col[c]) + ip + u * KP_NT);
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int l = 0; l < R; ++l) {
                        const kp_v2d v = *(reinterpret_cast<const kp_v2d *>(V + (size_t)l * (size_t)ldv) + ip + u * KP_NT);
#pragma unroll
                        for (int c = 0; c < CB; ++c) acc[c][l] = fma(kv[u][c].y, v.y, fma(kv[u][c].x, v.x, acc[c][l]));
                    }
            }
            for (; ip < np; ip += KP_NT) {
#pragma unroll
                for (int l = 0; l < R; ++l) {
                    const kp_v2d v = *(reinterpret_cast<const kp_v2d *>(V + (size_t)l * (size_t)ldv) + ip);
#pragma unroll
                    for (int c = 0; c < CB; ++c) {
                        const kp_v2d kv = __builtin_nontemporal_load(reinterpret_cast<const kp_v2d *>(col[c]) + ip);
                        acc[c][l] = fma(kv.y, v.y, fma(kv.x, v.x, acc[c][l]));
                    }
                }
            }
        } else {
            for (int64_t i = tid; i < n; i += KP_NT) {
                double kv[CB];
#pragma unroll
                for (int c = 0; c < CB; ++c) kv[c] = __builtin_nontemporal_load(col[c] + i);
#pragma unroll
                for (int l = 0; l < R; ++l) {
                    const double v = V[(size_t)i + (size_t)l * (size_t)ldv];
#pragma unroll
                    for (int c = 0; c < CB; ++c) acc[c][l] = fma(kv[c], v, acc[c][l]);
                }
            }
        }
#pragma unroll
        for (int c = 0; c < CB; ++c)
#pragma unroll
            for (int l = 0; l < R; ++l) {
                const double s = jch_wave_sum(acc[c][l]);
                if (lane == 0) red[wv][c * R + l] = s;
            }
        __syncthreads();
        for (int e = tid; e < CB * R; e += KP_NT) {
            const int c = e / R, l = e - c * R;
            double s = red[0][e];
#pragma unroll
            for (int w = 1; w < KP_NT / 64; ++w) s += red[w][e];
            if (j0 + c < n && l < rr) out[(size_t)(j0 + c) + (size_t)l * (size_t)ldo] = s;
        }
        __syncthreads();
    }
}

// Kc[i, j] = ((K[i, j] - vr[i]) - vc[j]) + s   (src/kplsr.jl:142 `K .- vtot' .- vtot .+ sum(D * DKt')`, same order; :209 for new rows).
// m x n, in place allowed.  s: *sdev when sdev is set, else shost.
__global__ __launch_bounds__(KP_NT) void k_kp_center(const double *__restrict__ K, int64_t ldk, double *Kc, int64_t ldc, int64_t m, int64_t n,
                                                     const double *__restrict__ vr, const double *__restrict__ vc, const double *sdev, double shost)
{
    const double s = sdev ? *sdev : shost;
    for (int64_t j = blockIdx.y; j < n; j += gridDim.y) {
        const double vj = vc[j];
        const double *src = K + (size_t)j * (size_t)ldk;
        double *dst = Kc + (size_t)j * (size_t)ldc;
        for (int64_t i = (int64_t)blockIdx.x * KP_NT + threadIdx.x; i < m; i += (int64_t)gridDim.x * KP_NT) dst[i] = ((src[i] - vr[i]) - vj) + s;
    }
}

// s = w' v, one workgroup (fixed order)
__global__ __launch_bounds__(KP_NT) void k_kp_wdot(const double *__restrict__ w, const double *__restrict__ v, int64_t n, double *s)
{
    __shared__ double scr[KP_NT / 64];
    double a = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += KP_NT) a = fma(w[i], v[i], a);
    a = jch_block_sum<KP_NT>(a, scr);
    if (threadIdx.x == 0) *s = a;
}

// Y[:, k] = (Ysrc[:, k] - m[k]) / s[k]  (`cscale!` / `center!` / `scale!` with m = NULL, src/kplsr.jl:128-135); in place allowed
__global__ __launch_bounds__(KP_NT) void k_kp_cscale(const double *Ys, int64_t lds, double *Y, int64_t ldy, int64_t n, int64_t q,
                                                     const double *__restrict__ mu, const double *__restrict__ sc)
{
    const int64_t tot = n * q;
    for (int64_t e = (int64_t)blockIdx.x * KP_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * KP_NT) {
        const int64_t k = e / n, i = e - k * n;
        Y[(size_t)i + (size_t)k * (size_t)ldy] = (Ys[(size_t)i + (size_t)k * (size_t)lds] - (mu ? mu[k] : 0.0)) / sc[k];
    }
}

// out[i, l] = d_i * (A[i, l] - sum_{k < ka} T[i, k] coef[k q + l])  for l < q (d = null: 1); in place allowed
__global__ __launch_bounds__(KP_NT) void k_kp_apply(double *out, int64_t ldo, const double *A, int64_t lda, const double *__restrict__ T,
                                                    int64_t ldt, int ka, const double *__restrict__ coef, const double *__restrict__ d,
                                                    int64_t n, int q)
{
    const int64_t tot = n * q;
    for (int64_t e = (int64_t)blockIdx.x * KP_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * KP_NT) {
        const int64_t l = e / n, i = e - l * n;
        double v = A[(size_t)i + (size_t)l * (size_t)lda];
        for (int k = 0; k < ka; ++k) v -= T[(size_t)i + (size_t)k * (size_t)ldt] * coef[(size_t)k * q + l];
        out[(size_t)i + (size_t)l * (size_t)ldo] = d ? d[i] * v : v;
    }
}

// part[b][k kb + l] = sum over the rows of block b of d_i A[i, k] B[i, l] (d = null: 1); one wave per entry, lanes over rows
__global__ __launch_bounds__(KP_NT) void k_kp_red(const double *__restrict__ A, int64_t lda, int ka, const double *__restrict__ B, int64_t ldb,
                                                  int kb, const double *__restrict__ d, int64_t n, int64_t chunk, double *__restrict__ part, int ldp)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * chunk, i1 = std::min<int64_t>(n, i0 + chunk);
    for (int e = wv; e < ka * kb; e += KP_NT / 64) {
        const int k = e / kb, l = e - k * kb;
        const double *a = A + (size_t)k * (size_t)lda, *b = B + (size_t)l * (size_t)ldb;
        double s = 0.0;
        for (int64_t i = i0 + lane; i < i1; i += 64) s = fma(d ? d[i] * a[i] : a[i], b[i], s);
        s = jch_wave_sum(s);
        if (lane == 0) part[(size_t)blockIdx.x * ldp + e] = s;
    }
}

__device__ __forceinline__ double kp_fin(const double *part, int nb, int ldp, int e)
{
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += part[(size_t)b * ldp + e];
    return s;
}

// Before the pass of LV a (>= 1): S row a-1 (S = T'DT, from the previous LV's partials), b = T'(D Y_a) (a x q) and the product-form
// coefficients of Z_a' = z_0' ... z_{a-1}' on D Y_a: alpha_i = b_i - sum_{j > i} S_ij alpha_j, i = a-1 .. 0 (z_{a-1}' acts first).
// after == true (behind the pass): c = T'(D W), beta_i = c_i - sum_{j < i} S_ij beta_j, i = 0 .. a-1 (Z_a W, z_0 acts first).
struct kp_small_args {
    const double *spart, *part;
    double *S, *coef;
    int a, q, nlv, nb, ldsp, ldp;
};
__global__ __launch_bounds__(KP_NT) void k_kp_proj(kp_small_args g, bool after)
{
    const int a = g.a, q = g.q, A = g.nlv;
    if (!after) {
        for (int j = threadIdx.x; j < a; j += KP_NT) {
            const double s = kp_fin(g.spart, g.nb, g.ldsp, j);
            g.S[(size_t)(a - 1) * A + j] = s;
            g.S[(size_t)j * A + (a - 1)] = s;
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < a * q; e += KP_NT) g.coef[e] = kp_fin(g.part, g.nb, g.ldp, e);   // [k][l] = entry k * q + l
    __syncthreads();
    for (int l = threadIdx.x; l < q; l += KP_NT) {
        if (!after) {
            for (int i = a - 1; i >= 0; --i) {
                double v = g.coef[(size_t)i * q + l];
                for (int j = i + 1; j < a; ++j) v -= g.S[(size_t)i * A + j] * g.coef[(size_t)j * q + l];
                g.coef[(size_t)i * q + l] = v;
            }
        } else {
            for (int i = 0; i < a; ++i) {
                double v = g.coef[(size_t)i * q + l];
                for (int j = 0; j < i; ++j) v -= g.S[(size_t)i * A + j] * g.coef[(size_t)j * q + l];
                g.coef[(size_t)i * q + l] = v;
            }
        }
    }
}

// The q x q form of the reference's inner loop (src/kplsr.jl:158-181) with u = Y_a g, M = K_a D Y_a:
//   t ~ M g, t'Dt = g'Bg, c = A g / sqrt(g'Bg), g' = c / sqrt(c'Gc), ztol^2 = (g - g')'G(g - g')
// with A = Y_a'DM, B = M'DM (both from the partials of [Y_a | M]' D M) and G = Y_a'Y_a.  Writes st[0] = 1/sqrt(g_t'Bg_t),
// st[1 .. q] = g_t (the g of the last t), st[q+1 ..] = c, st[2q+1 ..] = g_u (the new u), C[:, a] and iter[a].
struct kp_iter_args {
    const double *part, *gpart;
    double *mat;   // [3][q][q] A, B, G
    double *st, *C, *iter;
    int a, q, nb, ldp, ldg, maxit;
    double tol;
};
__global__ __launch_bounds__(KP_NT) void k_kp_iter(kp_iter_args g)
{
    __shared__ double gv[KP_MAXQ], gn[KP_MAXQ], cv[KP_MAXQ], hv[KP_MAXQ];
    __shared__ double scr[KP_NT / 64];
    const int q = g.q, tid = threadIdx.x;
    double *Am = g.mat, *Bm = g.mat + (size_t)q * q, *Gm = Bm + (size_t)q * q;
    for (int e = tid; e < q * q; e += KP_NT) {
        const int k = e / q, l = e - k * q;   // A[k][l] = Y_k' D M_l; B[k][l] = M_k' D M_l
        Am[e] = kp_fin(g.part, g.nb, g.ldp, k * q + l);
        Bm[e] = kp_fin(g.part, g.nb, g.ldp, (q + k) * q + l);
        Gm[e] = kp_fin(g.gpart, g.nb, g.ldg, e);
    }
    for (int k = tid; k < q; k += KP_NT) gv[k] = k == 0 ? 1.0 : 0.0;   // u = Y[:, 1]
    __syncthreads();
    int it = 0;
    double st = 0.0;
    for (;;) {
        double part = 0.0;
        for (int k = tid; k < q; k += KP_NT) {
            double h = 0.0;
            for (int l = 0; l < q; ++l) h += Bm[(size_t)k * q + l] * gv[l];
            part += gv[k] * h;
        }
        st = 1.0 / sqrt(jch_block_sum<KP_NT>(part, scr));
        for (int k = tid; k < q; k += KP_NT) {
            double h = 0.0;
            for (int l = 0; l < q; ++l) h += Am[(size_t)k * q + l] * gv[l];
            cv[k] = h * st;
        }
        __syncthreads();
        part = 0.0;
        for (int k = tid; k < q; k += KP_NT) {
            double h = 0.0;
            for (int l = 0; l < q; ++l) h += Gm[(size_t)k * q + l] * cv[l];
            part += cv[k] * h;
        }
        const double nc = 1.0 / sqrt(jch_block_sum<KP_NT>(part, scr));
        for (int k = tid; k < q; k += KP_NT) gn[k] = cv[k] * nc;
        __syncthreads();
        if (q == 1) break;   // src/kplsr.jl:158-164: no iteration, iter[a] = 0
        ++it;
        for (int k = tid; k < q; k += KP_NT) hv[k] = gv[k] - gn[k];
        __syncthreads();
        part = 0.0;
        for (int k = tid; k < q; k += KP_NT) {
            double h = 0.0;
            for (int l = 0; l < q; ++l) h += Gm[(size_t)k * q + l] * hv[l];
            part += hv[k] * h;
        }
        const double ztol = sqrt(fmax(jch_block_sum<KP_NT>(part, scr), 0.0));
        if (!(ztol > g.tol) || it >= g.maxit) break;
        for (int k = tid; k < q; k += KP_NT) gv[k] = gn[k];
        __syncthreads();
    }
    if (tid == 0) {
        g.st[0] = st;
        g.iter[g.a] = it;
    }
    for (int k = tid; k < q; k += KP_NT) {
        g.st[1 + k] = gv[k];
        g.st[1 + q + k] = cv[k];
        g.st[1 + 2 * q + k] = gn[k];
        g.C[(size_t)g.a * q + k] = cv[k];
    }
}

// Row step of LV a: t = st M g_t -> T[:, a], u = Y_a g_u -> U[:, a], Y_{a+1} = Y_a - t c' (src/kplsr.jl:182-188, the deflation of K postponed)
__global__ __launch_bounds__(KP_NT) void k_kp_rows(const double *__restrict__ M, double *Y, int64_t n, int q, const double *__restrict__ st,
                                                   double *__restrict__ t, double *__restrict__ u)
{
    const double s = st[0];
    const double *gt = st + 1, *c = st + 1 + q, *gu = st + 1 + 2 * q;
    for (int64_t i = (int64_t)blockIdx.x * KP_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * KP_NT) {
        double tv = 0.0, uv = 0.0;
        for (int l = 0; l < q; ++l) {
            tv += M[(size_t)i + (size_t)l * n] * gt[l];
            uv += Y[(size_t)i + (size_t)l * n] * gu[l];
        }
        tv *= s;
        t[i] = tv;
        u[i] = uv;
        for (int l = 0; l < q; ++l) Y[(size_t)i + (size_t)l * n] -= tv * c[l];
    }
}

namespace {

template <int R>
int32_t launch_pass_r(jch_ctx *ctx, const double *K, int64_t n, const double *V, int64_t ldv, int rr, double *out, int64_t ldo)
{
    constexpr int CB = R <= 2 ? 8 : R <= 4 ? 4 : R <= 8 ? 2 : 1;
    const int64_t ngroups = (n + CB - 1) / CB;
    const int64_t nb = std::min<int64_t>(ngroups, (int64_t)ctx->cus * 8);
    const bool vec = (n % 2) == 0 && (ldv % 2) == 0 && ((uintptr_t)K % 16) == 0 && ((uintptr_t)V % 16) == 0;
    if (vec)
        hipLaunchKernelGGL((k_kp_pass<R, CB, true>), dim3((unsigned)nb), dim3(KP_NT), 0, ctx->stream, K, n, V, ldv, rr, out, ldo, ngroups);
    else
        hipLaunchKernelGGL((k_kp_pass<R, CB, false>), dim3((unsigned)nb), dim3(KP_NT), 0, ctx->stream, K, n, V, ldv, rr, out, ldo, ngroups);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

// out (n x r, ld ldo) = K V for symmetric K; V (n x >= roundup(r), ld ldv) may be read past column r up to the instantiated width:
// the caller's buffer holds kp_padcols(r) columns
int kp_padcols(int r) { return r <= 8 ? r : r <= 16 ? 16 : ((r + 31) / 32) * 32; }
int32_t launch_pass(jch_ctx *ctx, const double *K, int64_t n, const double *V, int64_t ldv, int r, double *out, int64_t ldo)
{
    for (int c0 = 0; c0 < r; c0 += 32) {
        const int rr = std::min(32, r - c0);
        const double *Vc = V + (size_t)c0 * ldv;
        double *oc = out + (size_t)c0 * ldo;
        switch (rr) {
        case 1: JCH_TRY(launch_pass_r<1>(ctx, K, n, Vc, ldv, rr, oc, ldo)); break;
        case 2: JCH_TRY(launch_pass_r<2>(ctx, K, n, Vc, ldv, rr, oc, ldo)); break;
        case 3: JCH_TRY(launch_pass_r<3>(ctx, K, n, Vc, ldv, rr, oc, ldo)); break;
        case 4: JCH_TRY(launch_pass_r<4>(ctx, K, n, Vc, ldv, rr, oc, ldo)); break;
        case 5: JCH_TRY(launch_pass_r<5>(ctx, K, n, Vc, ldv, rr, oc, ldo)); break;
        case 6: JCH_TRY(launch_pass_r<6>(ctx, K, n, Vc, ldv, rr, oc, ldo)); break;
        case 7: JCH_TRY(launch_pass_r<7>(ctx, K, n, Vc, ldv, rr, oc, ldo)); break;
        case 8: JCH_TRY(launch_pass_r<8>(ctx, K, n, Vc, ldv, rr, oc, ldo)); break;
        default:
            if (rr <= 16) JCH_TRY(launch_pass_r<16>(ctx, K, n, Vc, ldv, rr, oc, ldo));
            else JCH_TRY(launch_pass_r<32>(ctx, K, n, Vc, ldv, rr, oc, ldo));
        }
    }
    return JCH_OK;
}

int32_t launch_red(jch_ctx *ctx, const double *A, int64_t lda, int ka, const double *B, int64_t ldb, int kb, const double *d, int64_t n,
                   int nb, double *part, int ldp)
{
    const int64_t chunk = (n + nb - 1) / nb;
    hipLaunchKernelGGL(k_kp_red, dim3(nb), dim3(KP_NT), 0, ctx->stream, A, lda, ka, B, ldb, kb, d, n, chunk, part, ldp);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

int32_t launch_apply(jch_ctx *ctx, double *out, int64_t ldo, const double *A, int64_t lda, const double *T, int64_t ldt, int ka,
                     const double *coef, const double *d, int64_t n, int q)
{
    hipLaunchKernelGGL(k_kp_apply, dim3(jch_grid1(ctx, n * q)), dim3(KP_NT), 0, ctx->stream, out, ldo, A, lda, T, ldt, ka, coef, d, n, q);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

int32_t launch_center(jch_ctx *ctx, const double *K, int64_t ldk, double *Kc, int64_t ldc, int64_t m, int64_t n, const double *vr,
                      const double *vc, const double *sdev, double shost)
{
    const unsigned gx = (unsigned)std::min<int64_t>((m + KP_NT - 1) / KP_NT, 64);
    const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)ctx->cus * 16 / gx));
    hipLaunchKernelGGL(k_kp_center, dim3(gx, gy), dim3(KP_NT), 0, ctx->stream, K, ldk, Kc, ldc, m, n, vr, vc, sdev, shost);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

struct kp_model {
    const double *weights, *vtot, *ymeans, *yscales, *R, *C;
    int64_t q; int32_t lo, hi, nlv;
};

// transform (pred == false) or predict over the new rows, block by block: Knew, vnew = Knew w, Kc_new = Knew - vnew 1' - 1 vtot' + s
// (src/kplsr.jl:202-212, predict :238-250), then the Plsr GEMMs on Kc_new with no shift / scale (T = Kc_new R; pred = ymeans + T C' diag(yscales))
int32_t kp_apply(jch_ctx *ctx, const char *who, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X, int64_t m,
                 int64_t p, int64_t ldx, const double *xscales, const double *Xt, int64_t n, int64_t ldxt, const kp_model &md, bool pred,
                 int64_t ncols, double *out, int64_t ldo)
{
    int64_t mb = 0;
    JCH_TRY(jch_kblocks_begin(ctx, who, loc, kind, degree, X && Xt && out && md.weights && md.vtot, m, n, p, ldx, ldxt, ldo,
                              jch_knob("JCH_KPLSR_QBLOCK", 0), &mb));
    if (mb == 0) return JCH_OK;
    double s = 0.0;   // sum(D * DKt') = w' K w = weights . vtot
    for (int64_t j = 0; j < n; ++j) s += md.weights[j] * md.vtot[j];
    JCH_TRY(jch_reserve(ctx, ctx->dk_s, sizeof(double) * (size_t)(n + mb)));
    double *vt_dev = (double *)ctx->dk_s.ptr, *vnew = vt_dev + n;
    JCH_HIP(ctx, hipMemcpyAsync(vt_dev, md.vtot, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    return jch_kblocks_run(ctx, loc, kind, gamma, coef0, degree, X, m, p, ldx, xscales, Xt, n, ldxt, mb, ncols, out, ldo,
                           [&](double *Kb, int64_t rows, double *ob, int64_t ldob) {
        JCH_TRY(jch_transform(ctx, JCH_LOC_DEVICE, Kb, rows, n, rows, nullptr, nullptr, md.weights, 1, vnew, rows));
        JCH_TRY(launch_center(ctx, Kb, rows, Kb, rows, rows, n, vnew, vt_dev, nullptr, s));
        if (pred)
            return jch_predict(ctx, JCH_LOC_DEVICE, Kb, rows, n, rows, nullptr, nullptr, md.ymeans, md.yscales, md.R, md.C, md.q, md.lo, md.hi, ob, ldob);
        return jch_transform(ctx, JCH_LOC_DEVICE, Kb, rows, n, rows, nullptr, nullptr, md.R, md.nlv, ob, ldob);
    });
}

}  // namespace

// K = kern(X, X) (symmetric path) into Kraw, vtot = K w, s = w'vtot and Kc = K - vtot 1' - 1 vtot' + s into Kc (Kc == Kraw allowed):
// for jch_kplsr_fit below, kpca.hip and krr.hip
int32_t jch_launch_kp_centred_gram(jch_ctx *ctx, int kind, double gamma, double coef0, int degree, const double *X, int64_t n, int64_t ldx,
                                   const double *xdiv, int64_t p, const double *wn, double *Kraw, double *Kc, double *vt, double *sdev)
{
    JCH_TRY(jch_launch_kgram(ctx, kind, X, n, ldx, xdiv, X, n, ldx, xdiv, p, gamma, coef0, degree, true, Kraw, n));
    JCH_TRY(launch_pass(ctx, Kraw, n, wn, n, 1, vt, n));   // vtot = K w (columns of the symmetric K against w)
    hipLaunchKernelGGL(k_kp_wdot, dim3(1), dim3(KP_NT), 0, ctx->stream, wn, vt, n, sdev);
    JCH_HIP(ctx, hipGetLastError());
    return launch_center(ctx, Kraw, n, Kc, n, n, n, vt, vt, sdev, 0.0);
}

extern "C" int32_t jch_kplsr_fit(jch_ctx *ctx, const jch_pls_desc *desc, int32_t kind, double gamma, double coef0, int32_t degree, double tol,
                                 int32_t maxit, void *X, int64_t ldx, void *Y, int64_t ldy, const double *weights, double *K_out, double *T,
                                 double *U, double *R, double *vtot, double *C, double *xscales, double *ymeans, double *yscales,
                                 double *weights_norm, int32_t *iter, int32_t *nlv_out)
{
    static const char *who = "jch_kplsr_fit";
    if (!ctx) return JCH_EINVAL;
    if (!desc) return jch_fail(ctx, JCH_EINVAL, "%s: desc is NULL", who);
    if (desc->dtype != JCH_F64) return jch_fail(ctx, JCH_EINVAL, "%s: Float64 only (dtype %d)", who, desc->dtype);
    JCH_TRY(jch_check_kernel(ctx, who, kind, degree));
    const jch_pls_desc &d = *desc;
    if (d.n < 1 || d.p < 1 || d.q < 1 || d.nlv < 1) return jch_fail(ctx, JCH_EINVAL, "%s: empty input or nlv < 1", who);
    if (maxit < 1) return jch_fail(ctx, JCH_EINVAL, "%s: maxit = %d must be >= 1", who, maxit);
    if (!(tol >= 0.0)) return jch_fail(ctx, JCH_EINVAL, "%s: tol must be >= 0", who);
    if (d.n > (1 << 20) || d.q > KP_MAXQ) return jch_fail(ctx, JCH_EINVAL, "%s: n=%lld or q=%lld too large (q <= %d)", who, (long long)d.n, (long long)d.q, KP_MAXQ);
    if (d.loc != JCH_LOC_HOST && d.loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, d.loc);
    if (!X || !Y) return jch_fail(ctx, JCH_EINVAL, "%s: X or Y is NULL", who);
    if (ldx < d.n || ldy < d.n) return jch_fail(ctx, JCH_EINVAL, "%s: ldx/ldy smaller than n", who);
    const int64_t n = d.n, p = d.p, q = d.q;
    const int A = (int)std::min<int64_t>(n, d.nlv);   // the reference does not clamp (src/kplsr.jl:145-146 allocate n x nlv)
    if ((int64_t)A * n >= ((int64_t)1 << 31)) return jch_fail(ctx, JCH_EINVAL, "%s: n * nlv too large", who);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = d.loc == JCH_LOC_HOST, inplace = d.inplace != 0, scal = d.scal != 0;
    std::vector<double> xs((size_t)p, 1.0), ym((size_t)q), ys((size_t)q, 1.0), xm((size_t)p);
    std::vector<double> Ch((size_t)A * q), ith((size_t)A);
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        // ---- device views of X and the raw weights
        double *dX = (double *)X;
        int64_t ldxd = ldx;
        const double *dw = weights;
        if (host) {
            JCH_TRY(jch_reserve(ctx, ctx->dk_x, sizeof(double) * (size_t)n * p));
            JCH_TRY(jch_copy2d(ctx, (double *)ctx->dk_x.ptr, n, (const double *)X, ldx, n, p, hipMemcpyHostToDevice));
            dX = (double *)ctx->dk_x.ptr; ldxd = n;
        }
        // ---- workspace (doubles, ld n): Ya | Wb (adjacent: one reduction gives Y_a'DM and M'DM) | Vb | T | U | DU, then the vectors and
        // the small state
        const int pc = kp_padcols(std::max<int>((int)q, A));
        const int ldp = (int)std::max<int64_t>({(int64_t)A * q, 2 * q * q, (int64_t)A + 1});
        const size_t nn = (size_t)n;
        jch_carve cv;
        const size_t oY = cv.take(nn * (q + pc)), oV = cv.take(nn * pc), oT = cv.take(nn * A), oU = cv.take(nn * A), oDU = cv.take(nn * A);
        const size_t ow = cv.take(nn), ovt = cv.take(nn), ohdr = cv.take(8), os = cv.take(8), oms = cv.take(2 * q + (size_t)p), oS = cv.take((size_t)A * A),
                     ocoef = cv.take((size_t)A * q), ost = cv.take(3 * (size_t)q + 1), omat = cv.take(3 * (size_t)q * q), oC = cv.take((size_t)A * q),
                     oit = cv.take(A), op1 = cv.take((size_t)KP_RED_NB * ldp), op2 = cv.take((size_t)KP_RED_NB * ldp), op3 = cv.take((size_t)KP_RED_NB * ldp),
                     op4 = cv.take((size_t)KP_RED_NB * ldp), op5 = cv.take((size_t)KP_RED_NB * ldp);
        JCH_TRY(jch_reserve(ctx, ctx->kp_ws, sizeof(double) * cv.off));
        double *ws = (double *)ctx->kp_ws.ptr;
        double *Ya = ws + oY, *Wb = ws + oY + nn * q, *Vb = ws + oV, *Td = ws + oT, *Ud = ws + oU, *DU = ws + oDU, *wn = ws + ow, *vt = ws + ovt,
               *hdr = ws + ohdr, *sdev = ws + os, *ms = ws + oms, *Sd = ws + oS, *coef = ws + ocoef, *st = ws + ost, *mat = ws + omat,
               *Cd = ws + oC, *itd = ws + oit, *part1 = ws + op1, *part2 = ws + op2, *part3 = ws + op3, *part4 = ws + op4, *part5 = ws + op5;
        if (host && weights) {
            JCH_HIP(ctx, hipMemcpyAsync(Vb, weights, sizeof(double) * nn, hipMemcpyHostToDevice, ctx->stream));   // (Vb: free until the LV loop)
            dw = Vb;
        }
        JCH_TRY(jch_launch_weights(ctx, dw, n, wn, hdr));   // `mweight` (src/kplsr.jl:124)
        // ---- Y: ymeans = colmean(Y, w); with scal, xscales = colstd(X, w), yscales = colstd(Y, w) (:125-135)
        if (host) JCH_TRY(jch_copy2d(ctx, Ya, n, (const double *)Y, ldy, n, q, hipMemcpyHostToDevice));
        const double *ysrc = host ? Ya : (const double *)Y;
        const int64_t ldys = host ? n : ldy;
        JCH_TRY(jch_col_stats(ctx, JCH_LOC_DEVICE, ysrc, n, q, ldys, dw, ym.data(), scal ? ys.data() : nullptr));
        if (scal) JCH_TRY(jch_col_stats(ctx, JCH_LOC_DEVICE, dX, n, p, ldxd, dw, xm.data(), xs.data()));
        double *ym_dev = ms, *ys_dev = ms + q, *xs_dev = ms + 2 * q;
        JCH_HIP(ctx, hipMemcpyAsync(ym_dev, ym.data(), sizeof(double) * (size_t)q, hipMemcpyHostToDevice, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(ys_dev, ys.data(), sizeof(double) * (size_t)q, hipMemcpyHostToDevice, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(xs_dev, xs.data(), sizeof(double) * (size_t)p, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_kp_cscale, dim3(jch_grid1(ctx, n * q)), dim3(KP_NT), 0, ctx->stream, ysrc, ldys, Ya, n, n, q, ym_dev, ys_dev);
        JCH_HIP(ctx, hipGetLastError());
        if (scal && inplace) {   // kplsr! hands X back divided by xscales (`scale!`, :131); otherwise the Gram divides on the fly
            hipLaunchKernelGGL(k_kp_cscale, dim3(jch_grid1(ctx, n * p)), dim3(KP_NT), 0, ctx->stream, dX, ldxd, dX, ldxd, n, p, nullptr, xs_dev);
            JCH_HIP(ctx, hipGetLastError());
        }
        // ---- K = kern(X, X) (:137), symmetric path; Kc = K - vtot 1' - 1 vtot' + w'Kw (:138-142) formed in the workspace Gram
        JCH_TRY(jch_reserve(ctx, ctx->dk_k, sizeof(double) * nn * nn));
        double *Kc = (double *)ctx->dk_k.ptr;
        double *Kraw = K_out ? K_out : Kc;
        const double *gdiv = scal && !inplace ? xs.data() : nullptr;
        JCH_TRY(jch_launch_kp_centred_gram(ctx, kind, gamma, coef0, degree, dX, n, ldxd, gdiv, p, wn, Kraw, Kc, vt, sdev));
        // ---- LV loop (:157-188): one pass over Kc per LV
        const int nbr = (int)std::max<int64_t>(1, std::min<int64_t>(KP_RED_NB, (n + 255) / 256));
        for (int a = 0; a < A; ++a) {
            if (a > 0) {
                JCH_TRY(launch_red(ctx, Td, n, a, Ya, n, (int)q, wn, n, nbr, part1, ldp));     // b = T'(D Y_a)
                kp_small_args g{part5, part1, Sd, coef, a, (int)q, A, nbr, ldp, ldp};
                hipLaunchKernelGGL(k_kp_proj, dim3(1), dim3(KP_NT), 0, ctx->stream, g, false);
                JCH_HIP(ctx, hipGetLastError());
            }
            JCH_TRY(launch_apply(ctx, Vb, n, Ya, n, Td, n, a, coef, wn, n, (int)q));        // V = D (Y_a - T alpha) = Z_a' D Y_a
            JCH_TRY(launch_pass(ctx, Kc, n, Vb, n, (int)q, Wb, n));                          // W = Kc V
            if (a > 0) {
                JCH_TRY(launch_red(ctx, Td, n, a, Wb, n, (int)q, wn, n, nbr, part2, ldp));     // c = T'(D W)
                kp_small_args g{part5, part2, Sd, coef, a, (int)q, A, nbr, ldp, ldp};
                hipLaunchKernelGGL(k_kp_proj, dim3(1), dim3(KP_NT), 0, ctx->stream, g, true);
                JCH_HIP(ctx, hipGetLastError());
                JCH_TRY(launch_apply(ctx, Wb, n, Wb, n, Td, n, a, coef, nullptr, n, (int)q)); // M = W - T beta = Z_a W
            }
            JCH_TRY(launch_red(ctx, Ya, n, 2 * (int)q, Wb, n, (int)q, wn, n, nbr, part3, ldp)); // [Y_a | M]' D M
            JCH_TRY(launch_red(ctx, Ya, n, (int)q, Ya, n, (int)q, nullptr, n, nbr, part4, ldp)); // Y_a'Y_a
            kp_iter_args gi{part3, part4, mat, st, Cd, itd, a, (int)q, nbr, ldp, ldp, maxit, tol};
            hipLaunchKernelGGL(k_kp_iter, dim3(1), dim3(KP_NT), 0, ctx->stream, gi);
            JCH_HIP(ctx, hipGetLastError());
            hipLaunchKernelGGL(k_kp_rows, dim3(jch_grid1(ctx, n)), dim3(KP_NT), 0, ctx->stream, Wb, Ya, n, (int)q, st, Td + nn * a, Ud + nn * a);
            JCH_HIP(ctx, hipGetLastError());
            if (a + 1 < A) JCH_TRY(launch_red(ctx, Td, n, a + 1, Td + nn * a, n, 1, wn, n, nbr, part5, ldp));   // S row a = t_a' D T
        }
        // ---- R = DU inv(T' D Kc DU) (:189-190): P = Kc (D T) in one pass, then plsnipals' M = P'W, Gauss-Jordan, R = W Mi with W = DU
        JCH_TRY(launch_apply(ctx, Vb, n, Td, n, nullptr, n, 0, nullptr, wn, n, A));
        JCH_TRY(launch_apply(ctx, DU, n, Ud, n, nullptr, n, 0, nullptr, wn, n, A));
        JCH_TRY(launch_pass(ctx, Kc, n, Vb, n, A, Wb, n));
        double *Rd = Vb;   // (D T is consumed by the pass)
        jch_small sm{};
        sm.P = Wb; sm.W = DU; sm.R = Rd;
        JCH_TRY(jch_launch_nipals_R(ctx, sm, (int)n, A));
        // ---- outputs
        const hipMemcpyKind dir = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
        if (T) JCH_TRY(jch_copy2d(ctx, T, n, Td, n, n, A, dir));
        if (U) JCH_TRY(jch_copy2d(ctx, U, n, Ud, n, n, A, dir));
        if (R) JCH_TRY(jch_copy2d(ctx, R, n, Rd, n, n, A, dir));
        if (vtot) JCH_HIP(ctx, hipMemcpyAsync(vtot, vt, sizeof(double) * nn, dir, ctx->stream));
        if (weights_norm) JCH_HIP(ctx, hipMemcpyAsync(weights_norm, wn, sizeof(double) * nn, dir, ctx->stream));
        if (inplace) {   // kplsr! hands X (scaled; already in place on the device) and Y (centred, scaled) back
            if (host) JCH_TRY(jch_copy2d(ctx, (double *)X, ldx, dX, ldxd, n, p, dir));
            JCH_TRY(jch_copy2d(ctx, (double *)Y, ldy, Ya, n, n, q, dir));
        }
        JCH_HIP(ctx, hipMemcpyAsync(Ch.data(), Cd, sizeof(double) * Ch.size(), hipMemcpyDeviceToHost, ctx->stream));
        JCH_HIP(ctx, hipMemcpyAsync(ith.data(), itd, sizeof(double) * ith.size(), hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    }));
    if (C) std::copy(Ch.begin(), Ch.end(), C);
    if (iter)
        for (int a = 0; a < A; ++a) iter[a] = (int32_t)ith[a];
    if (xscales) std::copy(xs.begin(), xs.end(), xscales);
    if (ymeans) std::copy(ym.begin(), ym.end(), ymeans);
    if (yscales) std::copy(ys.begin(), ys.end(), yscales);
    if (nlv_out) *nlv_out = A;
    return JCH_OK;
}

extern "C" int32_t jch_kplsr_transform(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X,
                                       int64_t m, int64_t p, int64_t ldx, const double *xscales, const double *Xtrain, int64_t n, int64_t ldxt,
                                       const double *weights, const double *vtot, const double *R, int32_t nlv, double *T, int64_t ldt)
{
    if (ctx && (!R || nlv < 1)) return jch_fail(ctx, JCH_EINVAL, "jch_kplsr_transform: R is NULL or nlv < 1");
    const kp_model md{weights, vtot, nullptr, nullptr, R, nullptr, 0, 0, 0, nlv};
    return kp_apply(ctx, "jch_kplsr_transform", loc, kind, gamma, coef0, degree, X, m, p, ldx, xscales, Xtrain, n, ldxt, md, false, nlv, T, ldt);
}

extern "C" int32_t jch_kplsr_predict(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X,
                                     int64_t m, int64_t p, int64_t ldx, const double *xscales, const double *Xtrain, int64_t n, int64_t ldxt,
                                     const double *weights, const double *vtot, const double *ymeans, const double *yscales, const double *R,
                                     const double *C, int64_t q, int32_t nlv_lo, int32_t nlv_hi, double *pred, int64_t ldo)
{
    if (ctx && (!R || !C || q < 1 || nlv_lo < 0 || nlv_hi < nlv_lo)) return jch_fail(ctx, JCH_EINVAL, "jch_kplsr_predict: bad model arguments");
    const kp_model md{weights, vtot, ymeans, yscales, R, C, q, nlv_lo, nlv_hi, 0};
    return kp_apply(ctx, "jch_kplsr_predict", loc, kind, gamma, coef0, degree, X, m, p, ldx, xscales, Xtrain, n, ldxt, md, true,
                    ((int64_t)nlv_hi - nlv_lo + 1) * q, pred, ldo);
}
