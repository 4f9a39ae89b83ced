// Covsel variable selection (src/covsel.jl:59-122, src/covselr.jl:48-53): jch_covsel_fit — include/jchemo_hip.h; DESIGN.md §15.
//
// The reference deflates X and Y with an n x n projector per selected variable.  Here X is never written (unless `inplace`) and never
// copied: with Q (n x i) an orthonormal basis of the deflated selected columns and Yd = (I - QQ')Yc,
//   Xd'Yd = Xc'Yd,   css_j(deflated) = css_j - sum_k G[j,k]^2 with G = Xc'Q,   x_d = Xc[:, j] - Q G[j, :]',
// so one step is ONE read-only pass over the column-major X against the panel [Yd | q_i] (k_cs_pass) plus O(n (i + q)) work on Q and
// Yd.  The whole loop is enqueued on the ctx stream; the selected index, the stop flag and every scalar live in device memory.
#include <math.h>

#include <algorithm>

#include "jch_internal.h"

#define CS_NT 256
#define CS_ROWS 1024         // rows per workgroup of the n-sized step kernels (4 per thread, 256 apart: coalesced)
#define CS_TILES 8           // 16-column tiles of X per wave and pass: a workgroup covers 4 * 8 * 16 = 512 columns
#define CS_PANEL 32          // panel columns one pass serves (two 16-wide MFMA tiles); wider panels re-read X per chunk of 32
#define CS_EXHAUSTED 1e-10   // a column whose deflated sum of squares is <= this share of its original one is exhausted

typedef double cs_v4 __attribute__((ext_vector_type(4)));

// device scalars of one fit: flag[0] stopped, flag[1] completed steps, flag[2] candidate column of the running step;
// sc[0] its criterion, sc[1] the norm of its deflated column, sc[2] xsstot, sc[3] ysstot
enum { CS_STOP = 0, CS_DONE = 1, CS_CAND = 2 };
enum { CS_CANDZ = 0, CS_NRM = 1, CS_XSSTOT = 2, CS_YSSTOT = 3 };

// ---- the pass: part[blk][k][j] = sum over the row tiles of the workgroup of (X[i, j] - mu_j) V[i, k] ---------------------------------
// v_mfma_f64_16x16x4: A[m = lane & 15][k = lane >> 4] is X' (m: 16 columns of X), B[k][n = lane & 15] the panel, D[(lane >> 4) + 4 reg][lane & 15].
// The sum index k of the instruction need not be consecutive rows: lane group kg = lane >> 4 owns the rows r0 + 4 kg ... + 3 of a
// 16-row tile and feeds them through four instructions, so one load instruction of a wave reads 16 columns x 128 contiguous bytes.
// Wave wv owns the column tiles 4 t + wv (t < CS_TILES) of the workgroup's 512 columns; the workgroups of a column group walk the row
// tiles interleaved (tile blockIdx.x, + gridDim.x, ...): at any moment they read one contiguous run of every column.
// Panel column k < nb0 is V0 + k ldv, the others V1 + (k - nb0) ldv; both null: the panel is one column of ones (column sums).  The
// panel's rows beyond n up to the next multiple of 16 exist and are zero (the caller's workspace); rows of X beyond n are never read.
// CSS: one more output column b, sum_i (X[i, j] - mu_j)^2.
template <int NB, bool CSS, bool ALIGNED>
__global__ __launch_bounds__(CS_NT) void k_cs_pass(const double *__restrict__ X, int64_t n, int p, int64_t ldx, const double *__restrict__ mu,
                                                   const double *__restrict__ V0, int nb0, const double *__restrict__ V1, int b, int64_t ldv,
                                                   double *__restrict__ part, int ldp, const int *__restrict__ flag)
{
    if (flag && flag[CS_STOP]) return;
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cl = lane & 15, kg = lane >> 4;
    const int ct0 = blockIdx.y * (4 * CS_TILES) + wv;              // first 16-column tile of this wave; the others follow 4 tiles apart
    const int ntw = std::min(CS_TILES, ((p + 15) / 16 - ct0 + 3) / 4);   // tiles of this wave that hold columns (<= 0: none)
    const int c0 = ct0 * 16 + cl;
    const double *xb = X + (size_t)c0 * (size_t)ldx;
    const size_t xstep = (size_t)64 * (size_t)ldx;
    double muc[CS_TILES];
#pragma unroll
    for (int t = 0; t < CS_TILES; ++t) muc[t] = (mu && c0 + 64 * t < p) ? mu[c0 + 64 * t] : 0.0;
    const bool ones = !V0 && !V1;
    const double *vb[NB];
#pragma unroll
    for (int h = 0; h < NB; ++h) {
        const int k = 16 * h + cl;
        vb[h] = (ones || k >= b) ? nullptr : (k < nb0 ? V0 + (size_t)k * (size_t)ldv : V1 + (size_t)(k - nb0) * (size_t)ldv);
    }
    cs_v4 acc[CS_TILES][NB];
    double sq[CS_TILES];
#pragma unroll
    for (int t = 0; t < CS_TILES; ++t) {
        sq[t] = 0.0;
#pragma unroll
        for (int h = 0; h < NB; ++h) acc[t][h] = cs_v4{0.0, 0.0, 0.0, 0.0};
    }
    const int64_t ntile = (n + 15) / 16;
    for (int64_t tau = blockIdx.x; tau < ntile; tau += gridDim.x) {
        const int64_t r = tau * 16 + 4 * kg;
        const bool whole = tau * 16 + 16 <= n;   // (wave-uniform)
        cs_v4 bv[NB];
#pragma unroll
        for (int h = 0; h < NB; ++h) {
            const double one = (ones && h == 0 && cl == 0) ? 1.0 : 0.0;
            bv[h] = vb[h] ? *reinterpret_cast<const cs_v4 *>(vb[h] + r) : cs_v4{one, one, one, one};
        }
        cs_v4 xv[CS_TILES];
#pragma unroll
        for (int t = 0; t < CS_TILES; ++t) {
            const double m = muc[t];
            xv[t] = cs_v4{m, m, m, m};   // (what is not loaded contributes x - mu = 0)
            if (t < ntw && c0 + 64 * t < p) {
                const double *ptr = xb + t * xstep + r;
                if (ALIGNED && whole) {
                    xv[t] = *reinterpret_cast<const cs_v4 *>(ptr);
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (r + s < n) xv[t][s] = ptr[s];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < CS_TILES; ++t) {
            if (t < ntw) {   // (scalar branch: every lane of the wave takes it, the matrix instructions run with all lanes on)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const double a = xv[t][s] - muc[t];
                    if (CSS) sq[t] += a * a;
#pragma unroll
                    for (int h = 0; h < NB; ++h) acc[t][h] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv[h][s], acc[t][h], 0, 0, 0);
                }
            }
        }
    }
    const int bout = b + (CSS ? 1 : 0);
    double *pp = part + (size_t)blockIdx.x * (size_t)bout * (size_t)ldp;
#pragma unroll
    for (int t = 0; t < CS_TILES; ++t) {
        if (t < ntw) {
            const int jb = (ct0 + 4 * t) * 16;
#pragma unroll
            for (int h = 0; h < NB; ++h) {
                const int k = 16 * h + cl;
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int j = jb + kg + 4 * reg;
                    if (j < p && k < b) pp[(size_t)k * ldp + j] = acc[t][h][reg];
                }
            }
            if (CSS) {
                double v = sq[t];
                v += __shfl_xor(v, 16, 64);
                v += __shfl_xor(v, 32, 64);
                if (kg == 0 && jb + cl < p) pp[(size_t)b * ldp + jb + cl] = v;
            }
        }
    }
}

// ---- small helpers of the step kernels ---------------------------------------------------------------------------------------------
// out[e] = sum over the blocks of part[blk][e], e < m: wave w of the workgroup takes the entries w, w + waves, ...; its lanes take the
// blocks lane, lane + 64, ... in order and the 64 lane sums meet in jch_wave_sum's fixed butterfly.
__device__ __forceinline__ void cs_sum_part(const double *__restrict__ part, int64_t nblk, int ld, int m, double *out)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int e = wv; e < m; e += nw) {
        double s = 0.0;
        for (int64_t bk = lane; bk < nblk; bk += 64) s += part[(size_t)bk * ld + e];
        s = jch_wave_sum(s);
        if (lane == 0) out[e] = s;
    }
}

// Sum over the p entries of v in a fixed order (thread-strided chains, then the block tree).
__device__ __forceinline__ double cs_vec_sum(const double *v, int p, double *scratch)
{
    double s = 0.0;
    for (int j = threadIdx.x; j < p; j += CS_NT) s += v[j];
    return jch_block_sum<CS_NT>(s, scratch);
}

__global__ __launch_bounds__(CS_NT) void k_cs_zero_pad(double *W, int64_t n, int64_t ldw, int cols)
{
    const int64_t pad = ldw - n, tot = pad * cols;
    for (int64_t e = (int64_t)blockIdx.x * CS_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * CS_NT) {
        const int64_t c = e / pad, i = e - c * pad;
        W[(size_t)(n + i) + (size_t)c * (size_t)ldw] = 0.0;
    }
}

// mu = colsum / n
__global__ __launch_bounds__(CS_NT) void k_cs_means(const double *__restrict__ colsum, int p, double n, double *__restrict__ mu)
{
    const int j = blockIdx.x * CS_NT + threadIdx.x;
    if (j < p) mu[j] = colsum[j] / n;
}

// One workgroup per Y column (src/covsel.jl:65-70): ymeans, yscales (the uncorrected std when q > 1, else 1), Yd = (Y - ymeans) / yscales
// and ycs = sum Yd^2; three reads of the column in a fixed order.
__global__ __launch_bounds__(1024) void k_cs_ystats(const double *__restrict__ Y, int64_t n, int q, int64_t ldy, double *__restrict__ Yd, int64_t ldw,
                                                    double *__restrict__ ymeans, double *__restrict__ yscales, double *__restrict__ ycs)
{
    __shared__ double red[16];
    const int k = blockIdx.x;
    const double *y = Y + (size_t)k * (size_t)ldy;
    double *yd = Yd + (size_t)k * (size_t)ldw;
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) s += y[i];
    const double m = jch_block_sum<1024>(s, red) / (double)n;
    double ss = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) { const double d = y[i] - m; ss += d * d; }
    ss = jch_block_sum<1024>(ss, red);
    const double sd = q > 1 ? sqrt(ss / (double)n) : 1.0;
    double s2 = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) { const double d = (y[i] - m) / sd; yd[i] = d; s2 += d * d; }
    s2 = jch_block_sum<1024>(s2, red);
    if (threadIdx.x == 0) { ymeans[k] = m; yscales[k] = sd; ycs[k] = s2; }
}

// ---- step i, first kernel (one workgroup): close step i - 1, then the criterion and its argmax ---------------------------------------
// KG [q + 1][ldp] is what the last pass delivered: K = Xc'Yd in the columns k < q; column q is css (first pass) or g = Xc'q_{i-1}.
// i == 0: css0 = css = KG[q], xsstot.  i > 0: G[:, i-1] = g, css -= g^2, xss[i-1] = sum css; ycs (per column of Yd) from the partials of
// the last update, yss[i-1].  select == 0 (after the last step): only that.
// typ 0 (cov, src/covsel.jl:83-84): z_j = sum_k (K_jk / n)^2.  typ 1 (cor, :87-88): z_j = sum_k K_jk^2 / (css_j ycs_k), and z_j = 0 for an
// exhausted column.  C[:, i] = z; argmax with ties to the lowest index; a NaN never wins.
__global__ __launch_bounds__(CS_NT) void k_cs_select(int i, int p, int q, double n, int typ, int select, const double *__restrict__ KG, int ldp,
                                                     double *__restrict__ css0, double *__restrict__ css, double *__restrict__ G, double *__restrict__ C,
                                                     double *__restrict__ xss, double *__restrict__ yss, double *__restrict__ ycs,
                                                     const double *__restrict__ ypart, int64_t nblk, int ldpart, int *flag, double *sc)
{
    __shared__ double red[CS_NT / 64];
    __shared__ double bz[CS_NT];
    __shared__ int bi[CS_NT];
    if (flag[CS_STOP]) return;
    const double *g = KG + (size_t)q * ldp;
    if (i == 0) {
        for (int j = threadIdx.x; j < p; j += CS_NT) css0[j] = css[j] = g[j];
    } else {
        for (int j = threadIdx.x; j < p; j += CS_NT) {
            const double v = g[j];
            G[(size_t)j + (size_t)(i - 1) * p] = v;
            css[j] -= v * v;
        }
        cs_sum_part(ypart, nblk, ldpart, q, ycs);
    }
    __syncthreads();
    const double xs = cs_vec_sum(css, p, red);
    const double ys = cs_vec_sum(ycs, q, red);
    if (threadIdx.x == 0) {
        if (i == 0) { sc[CS_XSSTOT] = xs; sc[CS_YSSTOT] = ys; }
        else { xss[i - 1] = xs; yss[i - 1] = ys; }
    }
    if (!select) return;
    double best = -1.0;
    int bj = INT32_MAX;
    for (int j = threadIdx.x; j < p; j += CS_NT) {
        double z = 0.0;
        if (typ == 0) {
            for (int k = 0; k < q; ++k) { const double c = KG[(size_t)k * ldp + j] / n; z += c * c; }
        } else if (css[j] > CS_EXHAUSTED * css0[j]) {
            const double cj = css[j];
            for (int k = 0; k < q; ++k) { const double c = KG[(size_t)k * ldp + j]; z += (c * c) / (cj * ycs[k]); }
        }
        C[(size_t)j + (size_t)i * p] = z;
        if (z > best) { best = z; bj = j; }   // (ascending j: the first of equal values stays; a NaN compares false)
    }
    bz[threadIdx.x] = best;
    bi[threadIdx.x] = bj;
    __syncthreads();
    for (int o = CS_NT / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const double z2 = bz[threadIdx.x + o];
            const int j2 = bi[threadIdx.x + o];
            if (z2 > bz[threadIdx.x] || (z2 == bz[threadIdx.x] && j2 < bi[threadIdx.x])) { bz[threadIdx.x] = z2; bi[threadIdx.x] = j2; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int j = bi[0] == INT32_MAX ? 0 : bi[0];   // (every z a NaN: column 0, with its NaN)
        flag[CS_CAND] = j;
        sc[CS_CANDZ] = C[(size_t)j + (size_t)i * p];
    }
}

// ---- step i, n-sized kernels: rows blockIdx.x * CS_ROWS + threadIdx.x + 256 s, s < 4; W = [Yd (q columns) | Q], leading dimension ldw -----
// x_d = X[:, j] - mu_j - Q G[j, :]' into Q[:, i] (j = the candidate, read from device memory), and the partial dots Q[:, k]'x_d, k < i
__global__ __launch_bounds__(CS_NT) void k_cs_xd(const double *__restrict__ X, int64_t n, int64_t ldx, const double *__restrict__ mu,
                                                 const double *__restrict__ G, int p, double *__restrict__ Q, int64_t ldw, int i,
                                                 const int *__restrict__ flag, double *__restrict__ part, int ldpart)
{
    __shared__ double red[CS_NT / 64];
    if (flag[CS_STOP]) return;
    const int j = flag[CS_CAND];
    const double muj = mu[j];
    const int64_t base = (int64_t)blockIdx.x * CS_ROWS + threadIdx.x;
    const double *xj = X + (size_t)j * (size_t)ldx;
    double x[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) x[s] = base + 256 * s < n ? xj[base + 256 * s] - muj : 0.0;
    for (int k = 0; k < i; ++k) {
        const double g = G[(size_t)j + (size_t)k * p];
        const double *qk = Q + (size_t)k * (size_t)ldw;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (base + 256 * s < n) x[s] -= qk[base + 256 * s] * g;
    }
    double *qi = Q + (size_t)i * (size_t)ldw;
#pragma unroll
    for (int s = 0; s < 4; ++s)
        if (base + 256 * s < n) qi[base + 256 * s] = x[s];
    for (int k = 0; k < i; ++k) {
        const double *qk = Q + (size_t)k * (size_t)ldw;
        double d = 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (base + 256 * s < n) d += qk[base + 256 * s] * x[s];
        d = jch_block_sum<CS_NT>(d, red);
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * ldpart + k] = d;
    }
}

__global__ __launch_bounds__(1024) void k_cs_sum_part(const double *__restrict__ part, int64_t nblk, int ld, int m, double *__restrict__ out,
                                                      const int *__restrict__ flag)
{
    if (flag[CS_STOP]) return;
    cs_sum_part(part, nblk, ld, m, out);
}

// the second Gram-Schmidt sweep: x_d -= Q h; partials of |x_d|^2 (entry 0) and of x_d'Yd[:, k] (entries 1 + k)
__global__ __launch_bounds__(CS_NT) void k_cs_reorth(double *__restrict__ W, int64_t n, int64_t ldw, int i, int q, const double *__restrict__ h,
                                                     const int *__restrict__ flag, double *__restrict__ part, int ldpart)
{
    __shared__ double red[CS_NT / 64];
    if (flag[CS_STOP]) return;
    const int64_t base = (int64_t)blockIdx.x * CS_ROWS + threadIdx.x;
    double *Q = W + (size_t)q * (size_t)ldw;
    double *qi = Q + (size_t)i * (size_t)ldw;
    double x[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) x[s] = base + 256 * s < n ? qi[base + 256 * s] : 0.0;
    for (int k = 0; k < i; ++k) {
        const double hk = h[k];
        const double *qk = Q + (size_t)k * (size_t)ldw;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (base + 256 * s < n) x[s] -= qk[base + 256 * s] * hk;
    }
    double d = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        if (base + 256 * s < n) qi[base + 256 * s] = x[s];
        d += x[s] * x[s];
    }
    d = jch_block_sum<CS_NT>(d, red);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * ldpart] = d;
    for (int k = 0; k < q; ++k) {
        const double *yk = W + (size_t)k * (size_t)ldw;
        double u = 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (base + 256 * s < n) u += x[s] * yk[base + 256 * s];
        u = jch_block_sum<CS_NT>(u, red);
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * ldpart + 1 + k] = u;
    }
}

// One workgroup: |x_d|^2 and x_d'Yd from the partials.  An exhausted column (|x_d|^2 not > CS_EXHAUSTED css0_j; a NaN too) stops the loop;
// otherwise the step is recorded: sel, selcov, cov2[sel], row i of QtY = q_i'Yd = x_d'Yd / |x_d|.
__global__ __launch_bounds__(1024) void k_cs_commit(const double *__restrict__ part, int64_t nblk, int ldpart, int q, int i, int nlv,
                                                    const double *__restrict__ css0, int *flag, double *sc, double *__restrict__ vals /*[q + 1]*/,
                                                    double *__restrict__ tq, double *__restrict__ QtY, int *__restrict__ sel, double *__restrict__ selcov,
                                                    double *__restrict__ cov2)
{
    if (flag[CS_STOP]) return;
    cs_sum_part(part, nblk, ldpart, q + 1, vals);
    __threadfence_block();
    __syncthreads();
    const int j = flag[CS_CAND];
    const double nrm2 = vals[0];
    if (!(nrm2 > CS_EXHAUSTED * css0[j])) {
        __syncthreads();
        if (threadIdx.x == 0) flag[CS_STOP] = 1;
        return;
    }
    const double nrm = sqrt(nrm2);
    for (int k = threadIdx.x; k < q; k += 1024) {
        const double t = vals[1 + k] / nrm;
        tq[k] = t;
        QtY[(size_t)i + (size_t)k * nlv] = t;
    }
    if (threadIdx.x == 0) {
        sc[CS_NRM] = nrm;
        sel[i] = j;
        selcov[i] = sc[CS_CANDZ];
        cov2[j] = sc[CS_CANDZ];
        flag[CS_DONE] = i + 1;
    }
}

// q_i = x_d / |x_d|; Yd -= q_i t with t = x_d'Yd / |x_d|; partials of what is left of q_i'Yd.  |x_d|^2 is an n-term sum, so q_i'q_i is 1 only up
// to sqrt(n) eps and t (q_i'q_i - 1) stays behind in Yd; it would come back in every later K as G[j, i] times that.  Hence a second sweep for Yd
// too (k_cs_update2), as for x_d.
__global__ __launch_bounds__(CS_NT) void k_cs_update(double *__restrict__ W, int64_t n, int64_t ldw, int i, int q, const double *__restrict__ sc,
                                                     const double *__restrict__ tq, const int *__restrict__ flag, double *__restrict__ part, int ldpart)
{
    __shared__ double red[CS_NT / 64];
    if (flag[CS_STOP]) return;
    const int64_t base = (int64_t)blockIdx.x * CS_ROWS + threadIdx.x;
    double *qi = W + (size_t)(q + i) * (size_t)ldw;
    const double nrm = sc[CS_NRM];
    double x[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        x[s] = 0.0;
        if (base + 256 * s < n) { x[s] = qi[base + 256 * s] / nrm; qi[base + 256 * s] = x[s]; }
    }
    for (int k = 0; k < q; ++k) {
        double *yk = W + (size_t)k * (size_t)ldw;
        const double t = tq[k];
        double u = 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (base + 256 * s < n) {
                const double y = yk[base + 256 * s] - x[s] * t;
                yk[base + 256 * s] = y;
                u += x[s] * y;
            }
        u = jch_block_sum<CS_NT>(u, red);
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * ldpart + k] = u;
    }
}

// One workgroup: t2 = what was left of q_i'Yd, from the partials; row i of QtY += t2
__global__ __launch_bounds__(1024) void k_cs_qty2(const double *__restrict__ part, int64_t nblk, int ldpart, int q, int i, int nlv, const int *__restrict__ flag,
                                                  double *__restrict__ tq, double *__restrict__ QtY)
{
    if (flag[CS_STOP]) return;
    cs_sum_part(part, nblk, ldpart, q, tq);
    __syncthreads();
    for (int k = threadIdx.x; k < q; k += 1024) QtY[(size_t)i + (size_t)k * nlv] += tq[k];
}

// Yd -= q_i t2; partials of the column sums of squares of the new Yd
__global__ __launch_bounds__(CS_NT) void k_cs_update2(double *__restrict__ W, int64_t n, int64_t ldw, int i, int q, const double *__restrict__ tq,
                                                      const int *__restrict__ flag, double *__restrict__ part, int ldpart)
{
    __shared__ double red[CS_NT / 64];
    if (flag[CS_STOP]) return;
    const int64_t base = (int64_t)blockIdx.x * CS_ROWS + threadIdx.x;
    const double *qi = W + (size_t)(q + i) * (size_t)ldw;
    double x[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) x[s] = base + 256 * s < n ? qi[base + 256 * s] : 0.0;
    for (int k = 0; k < q; ++k) {
        double *yk = W + (size_t)k * (size_t)ldw;
        const double t = tq[k];
        double u = 0.0;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (base + 256 * s < n) {
                const double y = yk[base + 256 * s] - x[s] * t;
                yk[base + 256 * s] = y;
                u += y * y;
            }
        u = jch_block_sum<CS_NT>(u, red);
        if (threadIdx.x == 0) part[(size_t)blockIdx.x * ldpart + k] = u;
    }
}

// ---- covsel!: X <- Xc - Q G' over the completed steps (what src/covsel.jl:112 leaves in X); one thread per row and 4 columns -------
__global__ __launch_bounds__(CS_NT) void k_cs_deflate_x(double *__restrict__ X, int64_t n, int p, int64_t ldx, const double *__restrict__ mu,
                                                        const double *__restrict__ Q, int64_t ldw, const double *__restrict__ G, const int *__restrict__ flag)
{
    const int64_t r = (int64_t)blockIdx.x * CS_NT + threadIdx.x;
    if (r >= n) return;
    const int nd = flag[CS_DONE];
    for (int j0 = 4 * blockIdx.y; j0 < p; j0 += 4 * gridDim.y) {
        double a[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c] = j0 + c < p ? X[(size_t)r + (size_t)(j0 + c) * (size_t)ldx] - mu[j0 + c] : 0.0;
        for (int k = 0; k < nd; ++k) {
            const double qv = Q[(size_t)r + (size_t)k * (size_t)ldw];
            const double *gk = G + (size_t)k * p + j0;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (j0 + c < p) a[c] -= qv * gk[c];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (j0 + c < p) X[(size_t)r + (size_t)(j0 + c) * (size_t)ldx] = a[c];
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
template <int NB, bool CSS>
static void cs_launch_pass(jch_ctx *ctx, bool aligned, dim3 grid, const double *X, int64_t n, int p, int64_t ldx, const double *mu, const double *V0,
                           int nb0, const double *V1, int b, int64_t ldv, double *part, int ldp, const int *flag)
{
    if (aligned)
        hipLaunchKernelGGL((k_cs_pass<NB, CSS, true>), grid, dim3(CS_NT), 0, ctx->stream, X, n, p, ldx, mu, V0, nb0, V1, b, ldv, part, ldp, flag);
    else
        hipLaunchKernelGGL((k_cs_pass<NB, CSS, false>), grid, dim3(CS_NT), 0, ctx->stream, X, n, p, ldx, mu, V0, nb0, V1, b, ldv, part, ldp, flag);
}

// KG [b (+ 1 with css)][ldp] = (X - 1 mu')'[V0 (nb0 columns) | V1 (b - nb0 columns)] (and the centred column sums of squares behind it):
// the pass per chunk of CS_PANEL panel columns, then the fixed-order sum of the per-workgroup partials.
static int32_t cs_pass(jch_ctx *ctx, const double *X, int64_t n, int p, int64_t ldx, const double *mu, const double *V0, int nb0, const double *V1, int b,
                       int64_t ldv, bool css, double *KG, int ldp, const int *flag)
{
    const int64_t ntile = (n + 15) / 16;
    const unsigned gx = (unsigned)std::min<int64_t>(ntile, 2 * (int64_t)ctx->cus);
    const dim3 grid(gx, (unsigned)((p + 64 * CS_TILES - 1) / (64 * CS_TILES)));
    const bool aligned = ((uintptr_t)X % 32 == 0) && (ldx % 4 == 0);
    const bool ones = !V0 && !V1;
    for (int k0 = 0; k0 < b; k0 += CS_PANEL) {
        const int bc = std::min(CS_PANEL, b - k0);
        const bool docss = css && k0 + bc == b;
        const int bout = bc + (docss ? 1 : 0);
        const int n0 = std::max(0, std::min(nb0, k0 + bc) - k0);   // panel columns of this chunk that come from V0
        const double *v0 = ones ? nullptr : (n0 > 0 ? V0 + (size_t)k0 * (size_t)ldv : nullptr);
        const double *v1 = ones ? nullptr : V1 + (size_t)(std::max(k0, nb0) - nb0) * (size_t)ldv;
        JCH_TRY(jch_reserve(ctx, ctx->cs_part, sizeof(double) * (size_t)gx * (size_t)bout * (size_t)ldp));
        double *part = (double *)ctx->cs_part.ptr;
        if (bc > 16) {
            if (docss) cs_launch_pass<2, true>(ctx, aligned, grid, X, n, p, ldx, mu, v0, n0, v1, bc, ldv, part, ldp, flag);
            else cs_launch_pass<2, false>(ctx, aligned, grid, X, n, p, ldx, mu, v0, n0, v1, bc, ldv, part, ldp, flag);
        } else {
            if (docss) cs_launch_pass<1, true>(ctx, aligned, grid, X, n, p, ldx, mu, v0, n0, v1, bc, ldv, part, ldp, flag);
            else cs_launch_pass<1, false>(ctx, aligned, grid, X, n, p, ldx, mu, v0, n0, v1, bc, ldv, part, ldp, flag);
        }
        JCH_HIP(ctx, hipGetLastError());
        JCH_TRY(jch_launch_reduce_rows(ctx, part, (int)gx, bout * ldp, bout * ldp, KG + (size_t)k0 * ldp));
    }
    return JCH_OK;
}

extern "C" int32_t jch_covsel_fit(jch_ctx *ctx, int32_t loc, double *X, int64_t n, int64_t p, int64_t ldx, double *Y, int64_t q, int64_t ldy, int32_t nlv,
                                  int32_t typ, int32_t inplace, int32_t *sel, double *selcov, double *cov2, double *C, double *cumpvarx, double *cumpvary,
                                  double *xmeans, double *ymeans, double *yscales, double *G, double *QtY, double *Q, int32_t *nlv_out)
{
    static const char *who = "jch_covsel_fit";
    if (!ctx) return JCH_EINVAL;
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (!X || n < 1 || p < 1 || ldx < n) return jch_fail(ctx, JCH_EINVAL, "%s: bad X (n=%lld p=%lld ldx=%lld)", who, (long long)n, (long long)p, (long long)ldx);
    if (!Y || q < 1 || ldy < n) return jch_fail(ctx, JCH_EINVAL, "%s: bad Y (q=%lld ldy=%lld)", who, (long long)q, (long long)ldy);
    if (nlv < 1) return jch_fail(ctx, JCH_EINVAL, "%s: nlv=%d must be at least 1", who, nlv);
    if (typ != JCH_COVSEL_COV && typ != JCH_COVSEL_COR) return jch_fail(ctx, JCH_EINVAL, "%s: bad typ %d", who, typ);
    if (q > (1 << 20) || p > (int64_t)(1 << 30) / (q + 2))
        return jch_fail(ctx, JCH_EINVAL, "%s: p (q + 2) = %lld x %lld beyond 2^30", who, (long long)p, (long long)(q + 2));
    if (ctx->nranks > 1) return jch_fail(ctx, JCH_EINVAL, "%s: one rank only (communicator of %d)", who, ctx->nranks);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST;
    const int a = (int)std::min<int64_t>(nlv, p);   // nlv is clamped to p
    const int pi = (int)p, qi = (int)q;
    const int ldp = (pi + 7) & ~7;
    const int64_t ldw = (n + 15) & ~(int64_t)15;
    const int64_t nblk = (n + CS_ROWS - 1) / CS_ROWS;
    const int ldpart = std::max(a, qi + 1);
    if (nblk > INT32_MAX) return jch_fail(ctx, JCH_EINVAL, "%s: n=%lld too large", who, (long long)n);
    if (inplace) ctx->xcopy_valid = false;   // X is about to be rewritten: a working copy a fit left of it is stale (JCH_REUSE_XCOPY)
    jch_carve cv;
    const size_t oW = cv.take((size_t)ldw * (size_t)(qi + a)), oY = cv.take(host ? (size_t)n * qi : 0), omu = cv.take(pi), ocss0 = cv.take(pi), ocss = cv.take(pi),
                 oKG = cv.take((size_t)(qi + 2) * ldp), oG = cv.take((size_t)pi * a), oC = cv.take((size_t)pi * a), ocov2 = cv.take(pi), oselcov = cv.take(a),
                 oxss = cv.take(a), oyss = cv.take(a), oycs = cv.take(qi), otq = cv.take(qi), oh = cv.take(a), ovals = cv.take(qi + 1),
                 oQtY = cv.take((size_t)a * qi), oym = cv.take(qi), oys = cv.take(qi), osc = cv.take(8), oflag = cv.take(8), osel = cv.take(a),
                 opart = cv.take((size_t)nblk * ldpart);
    JCH_TRY(jch_reserve(ctx, ctx->cs_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->cs_ws.ptr;
    double *W = ws + oW, *Qd = W + (size_t)qi * (size_t)ldw, *Ystage = ws + oY, *mu = ws + omu, *css0 = ws + ocss0, *css = ws + ocss, *KG = ws + oKG, *Gd = ws + oG,
           *Cd = ws + oC, *cov2d = ws + ocov2, *selcovd = ws + oselcov, *xss = ws + oxss, *yss = ws + oyss, *ycs = ws + oycs, *tq = ws + otq, *hd = ws + oh,
           *vals = ws + ovals, *QtYd = ws + oQtY, *ymd = ws + oym, *ysd = ws + oys, *sc = ws + osc, *part = ws + opart;
    int *flag = (int *)(ws + oflag), *seld = (int *)(ws + osel);
    std::vector<double> small(opart - oG);
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        // ---- device views of X and Y
        double *dX = X;
        int64_t ldxd = ldx;
        if (host) {
            JCH_TRY(jch_reserve(ctx, ctx->dk_x, sizeof(double) * (size_t)ldw * (size_t)p));
            JCH_TRY(jch_copy2d(ctx, (double *)ctx->dk_x.ptr, ldw, X, ldx, n, p, hipMemcpyHostToDevice));
            dX = (double *)ctx->dk_x.ptr; ldxd = ldw;
        }
        const double *dY = Y;
        int64_t ldyd = ldy;
        JCH_TRY(jch_stage_in(ctx, host, Ystage, n, q, &dY, &ldyd));
        // ---- everything from oG up to the partials starts as zero (G, C, cov2, the tables, the scalars and the flags)
        JCH_HIP(ctx, hipMemsetAsync(ws + oG, 0, sizeof(double) * (opart - oG), ctx->stream));
        if (ldw > n) {
            hipLaunchKernelGGL(k_cs_zero_pad, dim3(jch_grid1(ctx, (ldw - n) * (qi + a))), dim3(CS_NT), 0, ctx->stream, W, n, ldw, qi + a);
            JCH_HIP(ctx, hipGetLastError());
        }
        // ---- xmeans (a pass against a column of ones), ymeans / yscales / Yd, then K = Xc'Yd with the centred column sums of squares (:64-72)
        JCH_TRY(cs_pass(ctx, dX, n, pi, ldxd, nullptr, nullptr, 0, nullptr, 1, ldw, false, KG, ldp, nullptr));
        hipLaunchKernelGGL(k_cs_means, dim3((pi + CS_NT - 1) / CS_NT), dim3(CS_NT), 0, ctx->stream, KG, pi, (double)n, mu);
        hipLaunchKernelGGL(k_cs_ystats, dim3(qi), dim3(1024), 0, ctx->stream, dY, n, qi, ldyd, W, ldw, ymd, ysd, ycs);
        JCH_HIP(ctx, hipGetLastError());
        JCH_TRY(cs_pass(ctx, dX, n, pi, ldxd, mu, W, qi, nullptr, qi, ldw, true, KG, ldp, flag));
        const dim3 gn((unsigned)nblk);
        for (int i = 0; i < a; ++i) {
            hipLaunchKernelGGL(k_cs_select, dim3(1), dim3(CS_NT), 0, ctx->stream, i, pi, qi, (double)n, (int)typ, 1, KG, ldp, css0, css, Gd, Cd, xss, yss, ycs, part,
                               nblk, ldpart, flag, sc);
            hipLaunchKernelGGL(k_cs_xd, gn, dim3(CS_NT), 0, ctx->stream, dX, n, ldxd, mu, Gd, pi, Qd, ldw, i, flag, part, ldpart);
            if (i > 0) hipLaunchKernelGGL(k_cs_sum_part, dim3(1), dim3(1024), 0, ctx->stream, part, nblk, ldpart, i, hd, flag);
            hipLaunchKernelGGL(k_cs_reorth, gn, dim3(CS_NT), 0, ctx->stream, W, n, ldw, i, qi, hd, flag, part, ldpart);
            hipLaunchKernelGGL(k_cs_commit, dim3(1), dim3(1024), 0, ctx->stream, part, nblk, ldpart, qi, i, a, css0, flag, sc, vals, tq, QtYd, seld, selcovd, cov2d);
            hipLaunchKernelGGL(k_cs_update, gn, dim3(CS_NT), 0, ctx->stream, W, n, ldw, i, qi, sc, tq, flag, part, ldpart);
            hipLaunchKernelGGL(k_cs_qty2, dim3(1), dim3(1024), 0, ctx->stream, part, nblk, ldpart, qi, i, a, flag, tq, QtYd);
            hipLaunchKernelGGL(k_cs_update2, gn, dim3(CS_NT), 0, ctx->stream, W, n, ldw, i, qi, tq, flag, part, ldpart);
            JCH_HIP(ctx, hipGetLastError());
            // the next K = Xc'Yd and G[:, i] = Xc'q_i in one read of X; after the last step only G[:, a - 1] is left to fetch
            if (i + 1 < a) JCH_TRY(cs_pass(ctx, dX, n, pi, ldxd, mu, W, qi, Qd + (size_t)i * (size_t)ldw, qi + 1, ldw, false, KG, ldp, flag));
            else JCH_TRY(cs_pass(ctx, dX, n, pi, ldxd, mu, nullptr, 0, Qd + (size_t)i * (size_t)ldw, 1, ldw, false, KG + (size_t)qi * ldp, ldp, flag));
        }
        hipLaunchKernelGGL(k_cs_select, dim3(1), dim3(CS_NT), 0, ctx->stream, a, pi, qi, (double)n, (int)typ, 0, KG, ldp, css0, css, Gd, Cd, xss, yss, ycs, part, nblk,
                           ldpart, flag, sc);
        JCH_HIP(ctx, hipGetLastError());
        if (inplace) {   // X <- Xc - Q G', Y <- Yd (:112-113)
            const dim3 gd((unsigned)((n + CS_NT - 1) / CS_NT), (unsigned)std::min(1024, (pi + 3) / 4));
            hipLaunchKernelGGL(k_cs_deflate_x, gd, dim3(CS_NT), 0, ctx->stream, dX, n, pi, ldxd, mu, Qd, ldw, Gd, flag);
            JCH_HIP(ctx, hipGetLastError());
            if (host) JCH_TRY(jch_copy2d(ctx, X, ldx, dX, ldxd, n, p, hipMemcpyDeviceToHost));
            JCH_TRY(jch_copy2d(ctx, Y, ldy, W, ldw, n, q, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
        }
        if (Q) JCH_TRY(jch_copy2d(ctx, Q, n, Qd, ldw, n, a, host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice));
        // ---- the small results: one copy of the zero-initialised region, then the host picks them apart
        JCH_HIP(ctx, hipMemcpyAsync(small.data(), ws + oG, sizeof(double) * small.size(), hipMemcpyDeviceToHost, ctx->stream));
        if (xmeans) JCH_HIP(ctx, hipMemcpyAsync(xmeans, mu, sizeof(double) * (size_t)pi, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    }));
    auto at = [&](size_t off) { return small.data() + (off - oG); };
    const int *hflag = (const int *)at(oflag);
    const int done = hflag[CS_DONE];
    const double xsstot = at(osc)[CS_XSSTOT], ysstot = at(osc)[CS_YSSTOT];
    if (nlv_out) *nlv_out = done;
    if (sel) memcpy(sel, at(osel), sizeof(int32_t) * (size_t)a);
    if (selcov) memcpy(selcov, at(oselcov), sizeof(double) * (size_t)a);
    if (cov2) memcpy(cov2, at(ocov2), sizeof(double) * (size_t)pi);
    if (C) memcpy(C, at(oC), sizeof(double) * (size_t)pi * a);
    if (G) memcpy(G, at(oG), sizeof(double) * (size_t)pi * a);
    if (QtY) memcpy(QtY, at(oQtY), sizeof(double) * (size_t)a * qi);
    if (ymeans) memcpy(ymeans, at(oym), sizeof(double) * (size_t)qi);
    if (yscales) memcpy(yscales, at(oys), sizeof(double) * (size_t)qi);
    for (int i = 0; i < a; ++i) {   // (:117-118; the steps that were not completed stay 0)
        if (cumpvarx) cumpvarx[i] = i < done ? 1.0 - at(oxss)[i] / xsstot : 0.0;
        if (cumpvary) cumpvary[i] = i < done ? 1.0 - at(oyss)[i] / ysstot : 0.0;
    }
    return JCH_OK;
}

// The pass on its own (tools/bench_covsel.py, tests): out (p x b, ld p) = (X - 1 mu')'V, everything on the device.  V is copied into the
// ctx workspace first, where its columns are padded with zero rows up to a multiple of 16.
extern "C" int32_t jch_covsel_pass(jch_ctx *ctx, const double *X, int64_t n, int64_t p, int64_t ldx, const double *mu, const double *V, int64_t b, int64_t ldv,
                                   double *out)
{
    static const char *who = "jch_covsel_pass";
    if (!ctx) return JCH_EINVAL;
    if (!X || !V || !out || n < 1 || p < 1 || b < 1 || ldx < n || ldv < n)
        return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments (n=%lld p=%lld b=%lld ldx=%lld ldv=%lld)", who, (long long)n, (long long)p, (long long)b, (long long)ldx,
                        (long long)ldv);
    if (b > (1 << 20) || p > (int64_t)(1 << 30) / (b + 1)) return jch_fail(ctx, JCH_EINVAL, "%s: p (b + 1) = %lld x %lld beyond 2^30", who, (long long)p, (long long)(b + 1));
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const int pi = (int)p, bi = (int)b, ldp = (pi + 7) & ~7;
    const int64_t ldw = (n + 15) & ~(int64_t)15;
    jch_carve cv;
    const size_t oW = cv.take((size_t)ldw * (size_t)bi), oKG = cv.take((size_t)bi * ldp);
    JCH_TRY(jch_reserve(ctx, ctx->cs_ws, sizeof(double) * cv.off));
    double *W = (double *)ctx->cs_ws.ptr + oW, *KG = (double *)ctx->cs_ws.ptr + oKG;
    JCH_TRY(jch_copy2d(ctx, W, ldw, V, ldv, n, b, hipMemcpyDeviceToDevice));
    if (ldw > n) {
        hipLaunchKernelGGL(k_cs_zero_pad, dim3(jch_grid1(ctx, (ldw - n) * bi)), dim3(CS_NT), 0, ctx->stream, W, n, ldw, bi);
        JCH_HIP(ctx, hipGetLastError());
    }
    JCH_TRY(cs_pass(ctx, X, n, pi, ldx, mu, W, bi, nullptr, bi, ldw, false, KG, ldp, nullptr));
    JCH_TRY(jch_copy2d(ctx, out, p, KG, ldp, p, b, hipMemcpyDeviceToDevice));
    JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return JCH_OK;
}
