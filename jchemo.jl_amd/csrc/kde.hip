// Gaussian kernel density estimates: what the reference's `dmkern`, `kdeda` and `plskdeda` evaluate at prediction time (src/dmkern.jl:151-163,
// src/kdeda.jl:81-97, src/plskdeda.jl:52-64 through src/plslda.jl:107-130) — jch_kde_dens, include/jchemo_hip.h; DESIGN.md §21.
//
//   out[i, c, a] = coef[a, c] * sum_{r in class c} exp(-0.5 * v2[a, c] * sum_{j < dims[a]} ((Xq[i, j] - Z[r, j]) * u[j, c])^2)
//
//   k_kde_pairs<MODE, DR>   one workgroup = KDE_QT queries (one per lane; its 4 waves share them) x one class x one slice of that class's rows x
//                       one group of KDE_MG models.  A pair's scaled squared distance is accumulated column by column as a running prefix; model a
//                       is read off when the walk reaches column dims[a], so one walk serves the whole group.  The term is (x - z) * u: the
//                       difference is taken first, on the unscaled values (the Gram expansion, or x * u - z * u on pre-scaled rows, would put a
//                       cancellation error of order eps |x u|^2 into the exponent).  A chunk of the slice's rows sits in LDS, row-major; wave w
//                       takes the rows w, w + 4, ... of it and every lane of a wave reads the same address (a broadcast, no bank conflict).
//                         MODE 0  walks of <= KDE_DREG columns: the query's coordinates and the class's u live in registers, the column loop is
//                                 unrolled over DR = 4, 8, 16 or 32 columns (the first that holds the walk; the padding columns are zeros); the
//                                 prefix at a model's last column goes through a per-thread LDS slot (the model index is a run-time value, the
//                                 column index a compile-time one);
//                         MODE 1  <= KDE_DLDS columns: the coordinates come from a transposed query tile in LDS (lane stride 1), u from LDS;
//                         MODE 2  beyond: queries and rows are read from global memory as they stand (column-major: lane stride 1, and one
//                                 address per wave).
//                       The library `exp` is where the time goes (gfx950 has no f64 exp instruction); it is skipped when the argument of EVERY lane
//                       of the wave is below KDE_EXP_ZERO, where the f64 result is exactly 0 (a NaN argument is not below it and reaches `exp`).
//                       The 4 waves' sums meet in LDS in wave order; the workgroup writes one partial per (query, class, model, slice).
//   k_kde_reduce        out = coef * (the slices' partials added in slice order).  No atomics anywhere: two runs give identical bits.
// Every index that reaches memory is below the extent checked in jch_kde_dens: query rows are clamped to m - 1 (the surplus lanes compute a copy
// and store nothing), rows run inside [cls_start[c], cls_start[c + 1]), columns below dims[nmod - 1] <= d.  gfx950, hipcc -O3, no inline assembly.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "jch_internal.h"

#define KDE_QT 64           // queries per workgroup: one per lane
#define KDE_NT 256          // threads per workgroup: 4 waves on the same queries, each with a quarter of a chunk's rows
#define KDE_DREG 32         // widest walk whose query coordinates stay in registers (64 VGPRs, and 64 for u)
#define KDE_DLDS 80         // widest walk whose query tile (KDE_QT x d), u and a chunk of >= 24 rows fit KDE_LDS
#define KDE_MG 8            // models per workgroup: their prefixes and sums stay in registers
#define KDE_LDS 7168        // doubles of LDS per workgroup (56 KB); afterwards the 4 x KDE_MG x KDE_QT sums of the waves
#define KDE_ZL0 5120        // MODE 0: doubles of the row chunk; the KDE_MG x KDE_NT prefix slots follow it
#define KDE_CH 256          // most rows of a chunk
#define KDE_SPLIT_ROWS 64   // fewest rows of a class a slice is worth
#define KDE_SPLIT_MAX 64    // most slices per class
#define KDE_EXP_ZERO -746.0 // exp(x) == 0.0 in f64 for every x below (2^-1075 = exp(-745.13...))
static_assert(KDE_ZL0 + KDE_MG * KDE_NT <= KDE_LDS && 4 * KDE_MG * KDE_QT <= KDE_LDS && (KDE_QT + 1) * KDE_DLDS + 24 * KDE_DLDS <= KDE_LDS, "LDS layout");

struct kde_args {
    const double *Xq; int64_t ldq, m;
    const double *Z; int64_t ldz;
    const int64_t *cls_start;   // [ncls + 1]
    const double *u, *v2;       // [d x ncls], [nmod x ncls]
    const int *dims;            // [nmod]
    int d, ncls, nmod, nsplit, ngroup;
    double *part;               // [nsplit][ncls * nmod][m]: model a of class c in column c + ncls * a
};

// the models of a group read off the prefixes of one pair: acc[k] += exp(gv[k] * sg[k]), gv = -0.5 v2
__device__ __forceinline__ void kde_emit(const double (&sg)[KDE_MG], const double (&gv)[KDE_MG], int ng, double (&acc)[KDE_MG])
{
#pragma unroll
    for (int k = 0; k < KDE_MG; ++k) {
        if (k < ng) {                                          // (uniform)
            const double arg = gv[k] * sg[k];
            if (__any(!(arg < KDE_EXP_ZERO))) acc[k] += exp(arg);   // (wave-uniform skip: every lane's term would be exactly 0)
        }
    }
}

// one pair with the column index a run-time value: xg(j) / zg(j) / ug(j) are the query's, the row's and the class's value in column j
template <class XG, class ZG, class UG>
__device__ __forceinline__ void kde_walk(XG xg, ZG zg, UG ug, const int (&gd)[KDE_MG], const double (&gv)[KDE_MG], int ng, double (&acc)[KDE_MG])
{
    double s = 0.0, sg[KDE_MG];
    int j = 0;
#pragma unroll
    for (int k = 0; k < KDE_MG; ++k) {
        sg[k] = 0.0;
        if (k < ng) {                                          // (uniform)
#pragma unroll 4
            for (; j < gd[k]; ++j) {
                const double t = (xg(j) - zg(j)) * ug(j);
                s = fma(t, t, s);
            }
            sg[k] = s;
        }
    }
    kde_emit(sg, gv, ng, acc);
}

template <int MODE, int DR>
__global__ __launch_bounds__(KDE_NT) void k_kde_pairs(kde_args g)
{
    __shared__ double lds[KDE_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c = blockIdx.y, sp = (int)blockIdx.z / g.ngroup, grp = (int)blockIdx.z % g.ngroup;
    const int a0 = grp * KDE_MG, ng = min(KDE_MG, g.nmod - a0);
    const int64_t q0 = (int64_t)blockIdx.x * KDE_QT;
    const int64_t iq = min(q0 + lane, g.m - 1);                // (surplus lanes of the last tile redo the last query and store nothing)
    const int64_t cs = g.cls_start[c], nc = g.cls_start[c + 1] - cs;
    const int64_t r0 = cs + nc * sp / g.nsplit, r1 = cs + nc * (sp + 1) / g.nsplit;   // (a slice of a small class may be empty: its partial is 0)
    const double *__restrict__ uc = g.u + (size_t)c * (size_t)g.d;
    int gd[KDE_MG];
    double gv[KDE_MG], acc[KDE_MG];
#pragma unroll
    for (int k = 0; k < KDE_MG; ++k) {
        gd[k] = k < ng ? g.dims[a0 + k] : 0;
        gv[k] = k < ng ? -0.5 * g.v2[(size_t)(a0 + k) + (size_t)g.nmod * (size_t)c] : 0.0;
        acc[k] = 0.0;
    }
    const int dw = g.dims[a0 + ng - 1];                        // columns this group walks (<= d; MODE 0: <= DR)

    if constexpr (MODE == 0) {
        double x[DR], uu[DR];
#pragma unroll
        for (int j = 0; j < DR; ++j) {
            x[j] = j < dw ? g.Xq[iq + (int64_t)j * g.ldq] : 0.0;
            uu[j] = j < dw ? uc[j] : 0.0;
        }
        unsigned emask = 0;                                    // bit j set: some model of the group ends at column j + 1
#pragma unroll
        for (int k = 0; k < KDE_MG; ++k) if (k < ng) emask |= 1u << (gd[k] - 1);
        int ek[KDE_MG];                                        // the slot of model k: the ends in front of its own
#pragma unroll
        for (int k = 0; k < KDE_MG; ++k) ek[k] = k < ng ? __popc(emask & ((1u << (gd[k] - 1)) - 1u)) : 0;
        double *esl = lds + KDE_ZL0 + tid;                     // this thread's slots, KDE_NT apart
        const int ch = min(KDE_CH, KDE_ZL0 / DR);
        for (int64_t rc = r0; rc < r1; rc += ch) {
            const int nr = (int)min((int64_t)ch, r1 - rc);
            __syncthreads();                                   // (the previous chunk is done with)
            for (int j = 0; j < DR; ++j)                       // global reads run down a column; row r of the chunk at [r * DR, r * DR + DR)
                for (int r = tid; r < nr; r += KDE_NT) lds[r * DR + j] = j < dw ? g.Z[rc + r + (int64_t)j * g.ldz] : 0.0;
            __syncthreads();
            for (int r = wv; r < nr; r += 4) {                 // (wave-uniform)
                const double *z = lds + r * DR;
                double s = 0.0, sg[KDE_MG], tt[DR];
                int cnt = 0;
#pragma unroll
                for (int j = 0; j < DR; ++j) {                 // (no branch in here: the LDS reads of a row go out together)
                    const double t = (x[j] - z[j]) * uu[j];
                    tt[j] = t * t;
                }
#pragma unroll
                for (int j = 0; j < DR; ++j) {
                    s += tt[j];
                    if ((emask >> j) & 1u) { esl[cnt * KDE_NT] = s; ++cnt; }   // (uniform)
                }
#pragma unroll
                for (int k = 0; k < KDE_MG; ++k) sg[k] = esl[ek[k] * KDE_NT];  // (a thread reads what it wrote itself)
                kde_emit(sg, gv, ng, acc);
            }
        }
    } else if constexpr (MODE == 1) {
        for (int e = tid; e < KDE_QT * dw; e += KDE_NT) {      // the transposed query tile: element (lane l, column j) at [j * 64 + l]
            const int j = e >> 6, l = e & 63;
            lds[e] = g.Xq[min(q0 + l, g.m - 1) + (int64_t)j * g.ldq];
        }
        double *ul = lds + KDE_QT * dw, *zl = ul + dw;
        for (int j = tid; j < dw; j += KDE_NT) ul[j] = uc[j];
        const int ch = ((KDE_LDS - (KDE_QT + 1) * dw) / dw) & ~3;
        const double *xl = lds + lane;
        for (int64_t rc = r0; rc < r1; rc += ch) {
            const int nr = (int)min((int64_t)ch, r1 - rc);
            __syncthreads();
            for (int e = tid; e < nr * dw; e += KDE_NT) {
                const int j = e / nr, r = e - j * nr;
                zl[r * dw + j] = g.Z[rc + r + (int64_t)j * g.ldz];
            }
            __syncthreads();
            for (int r = wv; r < nr; r += 4) {                 // (wave-uniform)
                const double *z = zl + r * dw;
                kde_walk([&](int j) { return xl[j * KDE_QT]; }, [&](int j) { return z[j]; }, [&](int j) { return ul[j]; }, gd, gv, ng, acc);
            }
        }
    } else {
        const double *__restrict__ xp = g.Xq + iq;
        for (int64_t r = r0 + wv; r < r1; r += 4) {            // (wave-uniform)
            const double *__restrict__ zp = g.Z + r;
            kde_walk([&](int j) { return xp[(int64_t)j * g.ldq]; }, [&](int j) { return zp[(int64_t)j * g.ldz]; }, [&](int j) { return uc[j]; }, gd, gv,
                     ng, acc);
        }
    }
    // the waves' sums, added in wave order
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KDE_MG; ++k) lds[(wv * KDE_MG + k) * KDE_QT + lane] = acc[k];
    __syncthreads();
    if (wv == 0 && q0 + lane < g.m) {
        for (int k = 0; k < ng; ++k) {
            double s = lds[k * KDE_QT + lane];
            for (int w = 1; w < 4; ++w) s += lds[(w * KDE_MG + k) * KDE_QT + lane];
            const size_t col = (size_t)c + (size_t)g.ncls * (size_t)(a0 + k);
            g.part[((size_t)sp * (size_t)g.ncls * (size_t)g.nmod + col) * (size_t)g.m + (size_t)(q0 + lane)] = s;
        }
    }
}

// out[i, col] = coef[col] * (part[0][col][i] + part[1][col][i] + ...), col = c + ncls * a; coefd is laid out by col
__global__ __launch_bounds__(256) void k_kde_reduce(const double *__restrict__ part, int nsplit, int64_t m, int64_t ncm, const double *__restrict__ coefd,
                                                    double *__restrict__ out, int64_t ldo)
{
    const int64_t total = m * ncm;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t col = e / m, i = e - col * m;
        double s = part[e];
        for (int sp = 1; sp < nsplit; ++sp) s += part[(size_t)sp * (size_t)total + (size_t)e];
        out[i + col * ldo] = coefd[col] * s;
    }
}

// ---------------------------------------------------------------- C ABI
extern "C" int32_t jch_kde_dens(jch_ctx *ctx, int32_t loc, const double *Z, int64_t n, int64_t d, int64_t ldz, const double *Xq, int64_t m, int64_t ldq,
                                const int64_t *cls_start, int32_t ncls, const double *u, const double *v2, const double *coef, const int32_t *dims,
                                int32_t nmod, double *out, int64_t ldo)
{
    if (!ctx) return JCH_EINVAL;
    if (!Z || !Xq || !cls_start || !u || !v2 || !coef || !dims || !out) return jch_fail(ctx, JCH_EINVAL, "jch_kde_dens: NULL argument");
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "jch_kde_dens: bad loc");
    if (n < 1 || m < 1 || d < 1 || ncls < 1 || nmod < 1 || ldz < n || ldq < m || ldo < m)
        return jch_fail(ctx, JCH_EINVAL, "jch_kde_dens: bad shape (n=%lld m=%lld d=%lld ncls=%d nmod=%d ldz=%lld ldq=%lld ldo=%lld)", (long long)n, (long long)m,
                        (long long)d, ncls, nmod, (long long)ldz, (long long)ldq, (long long)ldo);
    if (n >= ((int64_t)1 << 40) || m >= ((int64_t)1 << 36) || d > (1 << 20) || ncls > 65535 || nmod > (1 << 20))
        return jch_fail(ctx, JCH_EINVAL, "jch_kde_dens: shape too large");
    if (cls_start[0] != 0 || cls_start[ncls] != n) return jch_fail(ctx, JCH_EINVAL, "jch_kde_dens: cls_start must run from 0 to n");
    int64_t ncmax = 0;
    for (int c = 0; c < ncls; ++c) {
        const int64_t nc = cls_start[c + 1] - cls_start[c];
        if (nc < 1) return jch_fail(ctx, JCH_EINVAL, "jch_kde_dens: class %d is empty (or cls_start decreases)", c);
        ncmax = std::max(ncmax, nc);
    }
    for (int a = 0; a < nmod; ++a)
        if (dims[a] < 1 || dims[a] > d || (a > 0 && dims[a] < dims[a - 1]))
            return jch_fail(ctx, JCH_EINVAL, "jch_kde_dens: dims must be non-decreasing within [1, d] (dims[%d] = %d)", a, dims[a]);
    const int64_t ncm = (int64_t)ncls * nmod;
    const int dw = dims[nmod - 1];                             // the widest walk (the groups in front of the last walk fewer columns)
    const int64_t qtiles = (m + KDE_QT - 1) / KDE_QT;
    const int ngroup = (nmod + KDE_MG - 1) / KDE_MG;
    // slices per class: enough workgroups for 4 per CU, none with fewer than KDE_SPLIT_ROWS rows of the largest class
    const int64_t base = qtiles * ncls * ngroup, want = ((int64_t)ctx->cus * 4 + base - 1) / base;
    int nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, KDE_SPLIT_MAX), ncmax / KDE_SPLIT_ROWS));
    if ((int64_t)nsplit * ngroup > 65535) nsplit = std::max(1, 65535 / ngroup);
    if ((int64_t)ngroup > 65535 || (double)m * (double)ncm * (double)nsplit >= (double)((int64_t)1 << 40))
        return jch_fail(ctx, JCH_EINVAL, "jch_kde_dens: m x ncls x nmod too large");
    const bool host = loc == JCH_LOC_HOST;
    // ---- one reservation: class offsets | dims | u | v2 | coef by output column | partials | the staging of a host call
    jch_carve cv;
    const size_t o_cs = cv.take((size_t)ncls + 1), o_dm = cv.take(jch_ints_as_doubles((size_t)nmod)), o_u = cv.take((size_t)d * ncls), o_v = cv.take((size_t)ncm),
                 o_cf = cv.take((size_t)ncm);
    const size_t n_small = cv.off;
    const size_t o_pt = cv.take((size_t)m * (size_t)ncm * (size_t)nsplit);
    const size_t o_z = host ? cv.take((size_t)n * (size_t)d) : 0, o_q = host ? cv.take((size_t)m * (size_t)d) : 0, o_o = host ? cv.take((size_t)m * (size_t)ncm) : 0;
    std::vector<double> small(n_small, 0.0);                   // host image of the first five pieces
    memcpy(small.data() + o_cs, cls_start, sizeof(int64_t) * ((size_t)ncls + 1));
    memcpy(small.data() + o_dm, dims, sizeof(int32_t) * (size_t)nmod);
    memcpy(small.data() + o_u, u, sizeof(double) * (size_t)d * ncls);
    memcpy(small.data() + o_v, v2, sizeof(double) * (size_t)ncm);
    for (int a = 0; a < nmod; ++a)
        for (int c = 0; c < ncls; ++c) small[o_cf + (size_t)c + (size_t)ncls * a] = coef[(size_t)a + (size_t)nmod * c];
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    JCH_TRY(jch_reserve(ctx, ctx->kd_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->kd_ws.ptr;
    return jch_synced(ctx, true, [&]() -> int32_t {
        JCH_HIP(ctx, hipMemcpyAsync(ws, small.data(), sizeof(double) * n_small, hipMemcpyHostToDevice, ctx->stream));
        kde_args g;
        g.Xq = Xq; g.ldq = ldq; g.m = m; g.Z = Z; g.ldz = ldz;
        double *dout = out;
        int64_t ldod = ldo;
        if (host) {
            JCH_TRY(jch_copy2d(ctx, ws + o_z, n, Z, ldz, n, d, hipMemcpyHostToDevice));
            JCH_TRY(jch_copy2d(ctx, ws + o_q, m, Xq, ldq, m, d, hipMemcpyHostToDevice));
            g.Z = ws + o_z; g.ldz = n; g.Xq = ws + o_q; g.ldq = m; dout = ws + o_o; ldod = m;
        }
        g.cls_start = (const int64_t *)(ws + o_cs); g.dims = (const int *)(ws + o_dm); g.u = ws + o_u; g.v2 = ws + o_v;
        g.d = (int)d; g.ncls = ncls; g.nmod = nmod; g.nsplit = nsplit; g.ngroup = ngroup; g.part = ws + o_pt;
        const dim3 grid((unsigned)qtiles, (unsigned)ncls, (unsigned)(nsplit * ngroup)), block(KDE_NT);
        if (dw <= 4) hipLaunchKernelGGL((k_kde_pairs<0, 4>), grid, block, 0, ctx->stream, g);
        else if (dw <= 8) hipLaunchKernelGGL((k_kde_pairs<0, 8>), grid, block, 0, ctx->stream, g);
        else if (dw <= 16) hipLaunchKernelGGL((k_kde_pairs<0, 16>), grid, block, 0, ctx->stream, g);
        else if (dw <= KDE_DREG) hipLaunchKernelGGL((k_kde_pairs<0, KDE_DREG>), grid, block, 0, ctx->stream, g);
        else if (dw <= KDE_DLDS) hipLaunchKernelGGL((k_kde_pairs<1, 0>), grid, block, 0, ctx->stream, g);
        else hipLaunchKernelGGL((k_kde_pairs<2, 0>), grid, block, 0, ctx->stream, g);
        JCH_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_kde_reduce, dim3(jch_grid1(ctx, m * ncm)), dim3(256), 0, ctx->stream, (const double *)(ws + o_pt), nsplit, m, ncm,
                           (const double *)(ws + o_cf), dout, ldod);
        JCH_HIP(ctx, hipGetLastError());
        if (host) JCH_TRY(jch_copy2d(ctx, out, ldo, dout, m, m, ncm, hipMemcpyDeviceToHost));
        return JCH_OK;
    });
}
