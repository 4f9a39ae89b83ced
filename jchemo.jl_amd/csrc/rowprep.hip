// Row-wise spectra preprocessing (src/preprocessing.jl): jch_rows_standardize (snv!), jch_rows_project_out (detrend!) and
// jch_rows_fir (savgol!, mavg!, mavg_runmean!, fdif!; with per-column taps: predict(::CalPds, X)) — include/jchemo_hip.h; DESIGN.md §14.
//
// One thread owns one row of the column-major X from its first load to its last store, so neighbouring lanes hold neighbouring
// rows: every column access of a wave is one contiguous 512-byte run, every output element is one thread's fixed-order sum, a
// NaN stays in its row, and `out == X` needs no second n x p buffer.  The kernels keep several columns of loads in flight per
// wave (RP_U independent loads issued ahead of their first use) because one row-thread has no other parallelism.
#include <math.h>

#include <algorithm>

#include "jch_internal.h"

#define RP_NT 256           // threads (rows) per workgroup of the standardize / project_out kernels
#define RP_U 8              // columns loaded ahead per thread
#define RP_FIR_NT 64        // rows per workgroup of the ring FIR kernel: one wave, its ring is [slots][64] doubles of LDS
#define RP_FIR_MAXF 57      // widest window of the ring kernel (64 slots = 32 KiB of LDS per wave); beyond: the row-block copy path
#define RP_STAGE_BYTES ((size_t)64 << 20)   // bound of the row-block staging (host data; windows beyond RP_FIR_MAXF)

// ---- standardize: out[i, :] = (x_i - mu_i) / s_i -----------------------------------------------------------------------------
// Two passes for the statistics (the mean, then the squared deviations from it: Statistics.std), a third for the output; the
// second and third read of a row come from L2 / the Infinity Cache where the rows of the waves in flight fit.
__global__ __launch_bounds__(RP_NT) void k_rp_standardize(const double *X, int64_t n, int64_t p, int64_t ldx, int cent, int scal, double *out,
                                                          int64_t ldo)
{
    const int64_t i = (int64_t)blockIdx.x * RP_NT + threadIdx.x;
    if (i >= n) return;
    const double *x = X + i;
    double *o = out + i;
    double s = 0.0;
    if (cent || scal) {
#pragma unroll RP_U
        for (int64_t j = 0; j < p; ++j) s += x[j * ldx];
    }
    const double mean = s / (double)p;
    double sd = 1.0;
    if (scal) {
        double ss = 0.0;
#pragma unroll RP_U
        for (int64_t j = 0; j < p; ++j) {
            const double d = x[j * ldx] - mean;
            ss += d * d;
        }
        sd = sqrt(ss / (double)p);   // uncorrected (src/utility.jl rowstd)
    }
    const double mu = cent ? mean : 0.0;
#pragma unroll RP_U
    for (int64_t j = 0; j < p; ++j) o[j * ldo] = (x[j * ldx] - mu) / sd;
}

// ---- project_out: out[i, :] = x_i - V (A x_i) -----------------------------------------------------------------------------------
// AV [p][2K]: per column j the K entries A[:, j] then the K entries V[j, :] (wave-uniform reads).
template <int K>
__global__ __launch_bounds__(RP_NT) void k_rp_project_out(const double *X, int64_t n, int64_t p, int64_t ldx, const double *__restrict__ AV,
                                                          double *out, int64_t ldo)
{
    const int64_t i = (int64_t)blockIdx.x * RP_NT + threadIdx.x;
    if (i >= n) return;
    const double *x = X + i;
    double *o = out + i;
    double c[K];
#pragma unroll
    for (int k = 0; k < K; ++k) c[k] = 0.0;
#pragma unroll RP_U
    for (int64_t j = 0; j < p; ++j) {
        const double v = x[j * ldx];
        const double *a = AV + j * (2 * K);
#pragma unroll
        for (int k = 0; k < K; ++k) c[k] += a[k] * v;
    }
#pragma unroll RP_U
    for (int64_t j = 0; j < p; ++j) {
        const double *a = AV + j * (2 * K) + K;
        double fit = 0.0;
#pragma unroll
        for (int k = 0; k < K; ++k) fit += a[k] * c[k];
        o[j * ldo] = x[j * ldx] - fit;
    }
}

// ---- FIR, windows up to RP_FIR_MAXF: the not-yet-overwritten originals of a row live in a ring --------------------------------
// out[i, j] = sum_t taps[t] x[i, clamp(j + lo + t, 0, p - 1)], j < pout, with -(f - 1) <= lo <= 0; the host hands over the nonzero
// taps only, as (weight, t) pairs in the order of t.  The outputs go in chunks of RP_U.  Chunk j0 needs the columns from j0 + lo
// up to j0 + RP_U - 1 + D, D = lo + f - 1 >= 0: f + RP_U - 1 of them, so a ring of R >= f + RP_U - 1 slots (R a power of two, slot =
// column & (R - 1)) that has received every column up to j0 + RP_U - 1 + D holds them all, and the chunk's own columns j0 ... are
// stored only after they went into the ring (D >= 0), which is what makes out == X safe.  The ring is LDS, [slot][lane]: a lane
// only ever touches its own words (no barrier) and all slot arithmetic is wave-uniform.  The columns of the NEXT chunk are loaded
// into registers before this chunk is computed; the taps are the outer loop, so that one tap feeds RP_U independent sums.
template <bool CLAMP>
__device__ __forceinline__ void rp_fir_chunk(const double *rg, const double *__restrict__ wts, const int *__restrict__ offs, int nnz, int64_t base0,
                                             int64_t p, int ringmask, double (&acc)[RP_U])
{
#pragma unroll 4
    for (int k = 0; k < nnz; ++k) {   // (unrolled so that the wave-uniform tap loads of a group go out together)
        const double w = wts[k];
        const int64_t base = base0 + offs[k];
#pragma unroll
        for (int u = 0; u < RP_U; ++u) {
            const int64_t c = CLAMP ? std::min<int64_t>(std::max<int64_t>(base + u, 0), p - 1) : base + u;
            acc[u] += w * rg[(size_t)(c & ringmask) * RP_FIR_NT];
        }
    }
}

__global__ __launch_bounds__(RP_FIR_NT) void k_rp_fir_ring(const double *X, int64_t n, int64_t p, int64_t ldx, const double *__restrict__ wts,
                                                           const int *__restrict__ offs, int nnz, int f, int lo, int64_t pout, int ringmask, double *out,
                                                           int64_t ldo)
{
    extern __shared__ double ring[];   // [ringmask + 1][RP_FIR_NT]
    const int lane = threadIdx.x;
    int64_t i = (int64_t)blockIdx.x * RP_FIR_NT + lane;
    const bool live = i < n;
    if (!live) i = n - 1;              // (idle lanes of the last wave shadow the last row and store nothing)
    const double *x = X + i;
    double *o = out + i;
    double *rg = ring + lane;
    const int64_t D = (int64_t)lo + f - 1;
    const int64_t npro = std::min<int64_t>(D, p);   // columns [0, npro) go in before the first chunk
    for (int64_t c0 = 0; c0 < npro; c0 += RP_U) {
        double r[RP_U];
#pragma unroll
        for (int u = 0; u < RP_U; ++u) r[u] = x[std::min<int64_t>(c0 + u, p - 1) * ldx];
#pragma unroll
        for (int u = 0; u < RP_U; ++u)
            if (c0 + u < npro) rg[(size_t)((c0 + u) & ringmask) * RP_FIR_NT] = r[u];
    }
    double nxt[RP_U];
#pragma unroll
    for (int u = 0; u < RP_U; ++u) nxt[u] = x[std::min<int64_t>(D + u, p - 1) * ldx];
    for (int64_t j0 = 0; j0 < pout; j0 += RP_U) {
        double cur[RP_U], acc[RP_U];
#pragma unroll
        for (int u = 0; u < RP_U; ++u) cur[u] = nxt[u];
#pragma unroll
        for (int u = 0; u < RP_U; ++u) nxt[u] = x[std::min<int64_t>(j0 + RP_U + D + u, p - 1) * ldx];
#pragma unroll
        for (int u = 0; u < RP_U; ++u) {
            if (j0 + D + u < p) rg[(size_t)((j0 + D + u) & ringmask) * RP_FIR_NT] = cur[u];
            acc[u] = 0.0;
        }
        if (j0 + lo >= 0 && j0 + RP_U - 1 + D <= p - 1)
            rp_fir_chunk<false>(rg, wts, offs, nnz, j0 + lo, p, ringmask, acc);
        else   // a border chunk, or the tail of the row (its surplus sums read clamped columns and are dropped)
            rp_fir_chunk<true>(rg, wts, offs, nnz, j0 + lo, p, ringmask, acc);
#pragma unroll
        for (int u = 0; u < RP_U; ++u)
            if (live && j0 + u < pout) o[(j0 + u) * ldo] = acc[u];
    }
}

// ---- FIR with per-column taps (JCH_FIR_PER_COLUMN), windows up to RP_FIR_MAXF ---------------------------------------------------
// out[i, j] = (sum_t tab[t, j] x[i, clamp(j + lo + t, 0, p - 1)]) + tab[f, j]; tab is (f + 1) x p, ld f + 1.  The ring, the chunks and
// the run-ahead loads are those of k_rp_fir_ring (same invariants, same proof that out == X is safe); only the taps differ: those of
// output j0 + u come from column j0 + u of the table.  The RP_U columns of a chunk are one contiguous slab of RP_U (f + 1) doubles.  The
// wave fetches the slab of the NEXT chunk with one coalesced vector load per lane (next to the run-ahead loads of X, on the same
// counter) and parks it behind the ring at the start of that chunk; the sums then read their taps from LDS, every lane the same word
// (a broadcast).  Measured: read through the scalar path instead, the table (48 KB at f = 11, p = 500) streams through
// the 16 KiB scalar cache of waves that sit at different columns, and the wave waits for one such miss per tap.
// Per t the RP_U ring words are read unconditionally (every window column of a chunk is in the ring, clamped ones included), so that
// the LDS reads overlap; where all RP_U taps are nonzero (every interior column of a PDS table) the sums take them without a test,
// otherwise each zero tap is skipped on its own.  The workgroup is ONE wave: slab writes and reads are LDS operations of the same
// wave, which the hardware keeps in order; the fences only keep the compiler from moving them across each other.
#define RP_PC_K ((RP_U * (RP_FIR_MAXF + 1) + RP_FIR_NT - 1) / RP_FIR_NT)   // slab words per lane at the widest window

__device__ __forceinline__ void rp_wave_sync_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the slab of the chunk at column j0, lane's words lane, lane + 64, ...; 0.0 beyond the table (the surplus sums of the tail are dropped)
__device__ __forceinline__ void rp_pc_fetch(const double *tab, int64_t j0, int64_t tabn, int slab, int lane, double (&tn)[RP_PC_K])
{
#pragma unroll
    for (int k = 0; k < RP_PC_K; ++k) {
        tn[k] = 0.0;
        if (k * RP_FIR_NT < slab) {   // (wave-uniform)
            const int64_t g = j0 * (slab / RP_U) + k * RP_FIR_NT + lane;
            if (k * RP_FIR_NT + lane < slab && g < tabn) tn[k] = tab[g];
        }
    }
}

template <bool CLAMP>
__device__ __forceinline__ void rp_fir_chunk_pc(const double *rg, const double *tp, int f, int64_t j0, int lo, int64_t p, int ringmask,
                                                double (&acc)[RP_U])
{
    const int ldt = f + 1;
    for (int t = 0; t < f; ++t) {
        double w[RP_U], v[RP_U];
        bool dense = true;
#pragma unroll
        for (int u = 0; u < RP_U; ++u) {
            w[u] = tp[u * ldt + t];
            dense = dense && w[u] != 0.0;
            const int64_t c = CLAMP ? std::min<int64_t>(std::max<int64_t>(j0 + lo + t + u, 0), p - 1) : j0 + lo + t + u;
            v[u] = rg[(size_t)(c & ringmask) * RP_FIR_NT];
        }
        if (__builtin_amdgcn_readfirstlane((int)dense)) {   // (every lane holds the same taps)
#pragma unroll
            for (int u = 0; u < RP_U; ++u) acc[u] += w[u] * v[u];
        } else {
#pragma unroll
            for (int u = 0; u < RP_U; ++u)
                if (w[u] != 0.0) acc[u] += w[u] * v[u];
        }
    }
#pragma unroll
    for (int u = 0; u < RP_U; ++u) acc[u] += tp[u * ldt + f];
}

__global__ __launch_bounds__(RP_FIR_NT) void k_rp_fir_ring_pc(const double *X, int64_t n, int64_t p, int64_t ldx, const double *tab, int f, int lo,
                                                              int ringmask, double *out, int64_t ldo)
{
    extern __shared__ double ring[];   // [ringmask + 1][RP_FIR_NT], then the slab of the current chunk [RP_U * (f + 1)]
    const int lane = threadIdx.x;
    int64_t i = (int64_t)blockIdx.x * RP_FIR_NT + lane;
    const bool live = i < n;
    if (!live) i = n - 1;              // (idle lanes of the last wave shadow the last row and store nothing)
    const double *x = X + i;
    double *o = out + i;
    double *rg = ring + lane;
    double *tp = ring + (size_t)(ringmask + 1) * RP_FIR_NT;
    const int slab = RP_U * (f + 1);
    const int64_t tabn = p * ((int64_t)f + 1);
    const int64_t D = (int64_t)lo + f - 1;
    const int64_t npro = std::min<int64_t>(D, p);   // columns [0, npro) go in before the first chunk
    double tn[RP_PC_K];
    rp_pc_fetch(tab, 0, tabn, slab, lane, tn);
    for (int64_t c0 = 0; c0 < npro; c0 += RP_U) {
        double r[RP_U];
#pragma unroll
        for (int u = 0; u < RP_U; ++u) r[u] = x[std::min<int64_t>(c0 + u, p - 1) * ldx];
#pragma unroll
        for (int u = 0; u < RP_U; ++u)
            if (c0 + u < npro) rg[(size_t)((c0 + u) & ringmask) * RP_FIR_NT] = r[u];
    }
    double nxt[RP_U];
#pragma unroll
    for (int u = 0; u < RP_U; ++u) nxt[u] = x[std::min<int64_t>(D + u, p - 1) * ldx];
    for (int64_t j0 = 0; j0 < p; j0 += RP_U) {
        double cur[RP_U], acc[RP_U];
        rp_wave_sync_lds();            // the sums of the previous chunk have read their taps
#pragma unroll
        for (int k = 0; k < RP_PC_K; ++k)
            if (k * RP_FIR_NT + lane < slab) tp[k * RP_FIR_NT + lane] = tn[k];
#pragma unroll
        for (int u = 0; u < RP_U; ++u) cur[u] = nxt[u];
        rp_pc_fetch(tab, j0 + RP_U, tabn, slab, lane, tn);
#pragma unroll
        for (int u = 0; u < RP_U; ++u) nxt[u] = x[std::min<int64_t>(j0 + RP_U + D + u, p - 1) * ldx];
#pragma unroll
        for (int u = 0; u < RP_U; ++u) {
            if (j0 + D + u < p) rg[(size_t)((j0 + D + u) & ringmask) * RP_FIR_NT] = cur[u];
            acc[u] = 0.0;
        }
        rp_wave_sync_lds();            // the slab is in place
        if (j0 + lo >= 0 && j0 + RP_U - 1 + D <= p - 1)
            rp_fir_chunk_pc<false>(rg, tp, f, j0, lo, p, ringmask, acc);
        else   // a border chunk, or the tail of the row
            rp_fir_chunk_pc<true>(rg, tp, f, j0, lo, p, ringmask, acc);
#pragma unroll
        for (int u = 0; u < RP_U; ++u)
            if (live && j0 + u < p) o[(j0 + u) * ldo] = acc[u];
    }
}

// per-column taps, any window (the route of k_rp_fir_copy below, W as there): tab (f + 1) x p as above
__global__ __launch_bounds__(RP_NT) void k_rp_fir_copy_pc(const double *W, int64_t rows, int64_t p, int64_t ldw, const double *__restrict__ tab, int64_t f,
                                                          int64_t lo, double *out, int64_t ldo)
{
    const int64_t tot = rows * p;
    for (int64_t e = (int64_t)blockIdx.x * RP_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * RP_NT) {
        const int64_t j = e / rows, i = e - j * rows;
        const double *__restrict__ col = tab + (size_t)j * (size_t)(f + 1);
        double acc = 0.0;
        for (int64_t t = 0; t < f; ++t) {
            const double w = col[t];
            if (w != 0.0) {
                const int64_t c = std::min<int64_t>(std::max<int64_t>(j + lo + t, 0), p - 1);
                acc += w * W[(size_t)i + (size_t)c * (size_t)ldw];
            }
        }
        out[(size_t)i + (size_t)j * (size_t)ldo] = acc + col[f];
    }
}

// ---- FIR, any window: W is the input itself (out != X) or a copy of a block of its rows, so every output reads its taps from it ---------------------------
__global__ __launch_bounds__(RP_NT) void k_rp_fir_copy(const double *W, int64_t rows, int64_t p, int64_t ldw, const double *__restrict__ wts,
                                                       const int *__restrict__ offs, int nnz, int64_t lo, int64_t pout, double *out, int64_t ldo)
{
    const int64_t tot = rows * pout;
    for (int64_t e = (int64_t)blockIdx.x * RP_NT + threadIdx.x; e < tot; e += (int64_t)gridDim.x * RP_NT) {
        const int64_t j = e / rows, i = e - j * rows;
        double acc = 0.0;
        for (int k = 0; k < nnz; ++k) {
            const int64_t c = std::min<int64_t>(std::max<int64_t>(j + lo + offs[k], 0), p - 1);
            acc += wts[k] * W[(size_t)i + (size_t)c * (size_t)ldw];
        }
        out[(size_t)i + (size_t)j * (size_t)ldo] = acc;
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
static int64_t rp_block_rows(int64_t n, int64_t cols)
{
    int64_t rb = (int64_t)(RP_STAGE_BYTES / (sizeof(double) * (size_t)cols));
    if (rb >= 256) rb &= ~(int64_t)255;
    return std::max<int64_t>(1, std::min(rb, n));
}

static int32_t rp_check(jch_ctx *ctx, const char *who, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *out, int64_t ldo)
{
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc %d", who, loc);
    if (!X || !out || n < 1 || p < 1 || ldx < n || ldo < n)
        return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments (n=%lld p=%lld ldx=%lld ldo=%lld)", who, (long long)n, (long long)p, (long long)ldx, (long long)ldo);
    if (out == X && ldo != ldx) return jch_fail(ctx, JCH_EINVAL, "%s: in place (out == X) needs ldo == ldx", who);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    // A preprocessing call may rewrite, in place, the very X a plskern-shaped fit left its working copy of: that copy is not to be
    // trusted afterwards, whatever the next fit promises (JCH_REUSE_XCOPY).
    ctx->xcopy_valid = false;
    return JCH_OK;
}

// Device rows in place or not: fn(X, rows, ldx, out, ldo).  Host rows: blocks of at most RP_STAGE_BYTES go through ctx->rp_stage,
// are processed there in place and the first pout columns come back.
template <class F>
static int32_t rp_run(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, double *out, int64_t ldo, int64_t pout, F fn)
{
    return jch_synced(ctx, true, [&]() -> int32_t {
        if (loc == JCH_LOC_DEVICE) return fn(X, n, ldx, out, ldo);
        const int64_t rb = rp_block_rows(n, p);
        JCH_TRY(jch_reserve(ctx, ctx->rp_stage, sizeof(double) * (size_t)rb * (size_t)p));
        double *S = (double *)ctx->rp_stage.ptr;
        for (int64_t r0 = 0; r0 < n; r0 += rb) {
            const int64_t rows = std::min(rb, n - r0);
            JCH_TRY(jch_copy2d(ctx, S, rb, X + r0, ldx, rows, p, hipMemcpyHostToDevice));
            JCH_TRY(fn(S, rows, rb, S, rb));
            JCH_TRY(jch_copy2d(ctx, out + r0, ldo, S, rb, rows, pout, hipMemcpyDeviceToHost));
        }
        return JCH_OK;
    });
}

static int32_t rp_coef(jch_ctx *ctx, const double *host, size_t count, const double **dev)
{
    JCH_TRY(jch_reserve(ctx, ctx->rp_coef, sizeof(double) * count));
    JCH_HIP(ctx, hipMemcpyAsync(ctx->rp_coef.ptr, host, sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
    JCH_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the host array may be a temporary of the caller's)
    *dev = (const double *)ctx->rp_coef.ptr;
    return JCH_OK;
}

static unsigned rp_grid(int64_t n, int nt) { return (unsigned)((n + nt - 1) / nt); }

extern "C" int32_t jch_rows_standardize(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, int32_t cent, int32_t scal,
                                        double *out, int64_t ldo)
{
    static const char *who = "jch_rows_standardize";
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(rp_check(ctx, who, loc, X, n, p, ldx, out, ldo));
    return rp_run(ctx, loc, X, n, p, ldx, out, ldo, p, [&](const double *x, int64_t rows, int64_t ld, double *o, int64_t ldout) -> int32_t {
        hipLaunchKernelGGL(k_rp_standardize, dim3(rp_grid(rows, RP_NT)), dim3(RP_NT), 0, ctx->stream, x, rows, p, ld, (int)(cent != 0), (int)(scal != 0), o,
                           ldout);
        JCH_HIP(ctx, hipGetLastError());
        return JCH_OK;
    });
}

template <int K>
static int32_t rp_launch_project(jch_ctx *ctx, int k, const double *x, int64_t rows, int64_t p, int64_t ld, const double *AV, double *o, int64_t ldout)
{
    if constexpr (K > 1) {
        if (k < K) return rp_launch_project<K - 1>(ctx, k, x, rows, p, ld, AV, o, ldout);
    }
    hipLaunchKernelGGL(k_rp_project_out<K>, dim3(rp_grid(rows, RP_NT)), dim3(RP_NT), 0, ctx->stream, x, rows, p, ld, AV, o, ldout);
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

extern "C" int32_t jch_rows_project_out(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *A, const double *V,
                                        int32_t k, double *out, int64_t ldo)
{
    static const char *who = "jch_rows_project_out";
    if (!ctx) return JCH_EINVAL;
    if (!A || !V || k < 1 || k > 8) return jch_fail(ctx, JCH_EINVAL, "%s: A (k x p), V (p x k) with 1 <= k <= 8 (k=%d)", who, k);
    JCH_TRY(rp_check(ctx, who, loc, X, n, p, ldx, out, ldo));
    std::vector<double> av((size_t)p * 2 * k);   // per column: A[:, j] (k x p, ld k), then V[j, :] (p x k, ld p)
    for (int64_t j = 0; j < p; ++j)
        for (int r = 0; r < k; ++r) {
            av[(size_t)j * 2 * k + r] = A[(size_t)r + (size_t)j * k];
            av[(size_t)j * 2 * k + k + r] = V[(size_t)j + (size_t)r * p];
        }
    const double *AV = nullptr;
    JCH_TRY(rp_coef(ctx, av.data(), av.size(), &AV));
    return rp_run(ctx, loc, X, n, p, ldx, out, ldo, p, [&](const double *x, int64_t rows, int64_t ld, double *o, int64_t ldout) -> int32_t {
        return rp_launch_project<8>(ctx, k, x, rows, p, ld, AV, o, ldout);
    });
}

// JCH_FIR_SAME | JCH_FIR_PER_COLUMN: the (f + 1) x p table goes to the device as it is; the routes are those of the uniform modes.
static int32_t rp_fir_per_column(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *tab, int64_t f, int64_t lo,
                                 double *out, int64_t ldo)
{
    const double *tdev = nullptr;
    JCH_TRY(rp_coef(ctx, tab, (size_t)(f + 1) * (size_t)p, &tdev));
    return rp_run(ctx, loc, X, n, p, ldx, out, ldo, p, [&](const double *x, int64_t rows, int64_t ld, double *o, int64_t ldout) -> int32_t {
        if (f <= RP_FIR_MAXF) {
            int slots = 1;
            while (slots < f + RP_U - 1) slots <<= 1;
            hipLaunchKernelGGL(k_rp_fir_ring_pc, dim3(rp_grid(rows, RP_FIR_NT)), dim3(RP_FIR_NT),
                               sizeof(double) * ((size_t)slots * RP_FIR_NT + (size_t)RP_U * (size_t)(f + 1)), ctx->stream, x, rows, p, ld, tdev, (int)f, (int)lo,
                               slots - 1, o, ldout);
            JCH_HIP(ctx, hipGetLastError());
            return JCH_OK;
        }
        if (o != x) {
            hipLaunchKernelGGL(k_rp_fir_copy_pc, dim3(jch_grid1(ctx, rows * p)), dim3(RP_NT), 0, ctx->stream, x, rows, p, ld, tdev, f, lo, o, ldout);
            JCH_HIP(ctx, hipGetLastError());
            return JCH_OK;
        }
        const int64_t rb = rp_block_rows(rows, p);
        JCH_TRY(jch_reserve(ctx, ctx->rp_rows, sizeof(double) * (size_t)rb * (size_t)p));
        double *W = (double *)ctx->rp_rows.ptr;
        for (int64_t r0 = 0; r0 < rows; r0 += rb) {
            const int64_t m = std::min(rb, rows - r0);
            JCH_TRY(jch_copy2d(ctx, W, rb, x + r0, ld, m, p, hipMemcpyDeviceToDevice));
            hipLaunchKernelGGL(k_rp_fir_copy_pc, dim3(jch_grid1(ctx, m * p)), dim3(RP_NT), 0, ctx->stream, W, m, p, rb, tdev, f, lo, o + r0, ldout);
            JCH_HIP(ctx, hipGetLastError());
        }
        return JCH_OK;
    });
}

extern "C" int32_t jch_rows_fir(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *taps, int64_t f, int64_t lo,
                                int32_t mode, double *out, int64_t ldo)
{
    static const char *who = "jch_rows_fir";
    if (!ctx) return JCH_EINVAL;
    if (!taps || f < 1) return jch_fail(ctx, JCH_EINVAL, "%s: taps with f >= 1 (f=%lld)", who, (long long)f);
    if (mode != JCH_FIR_SAME && mode != JCH_FIR_VALID && mode != (JCH_FIR_SAME | JCH_FIR_PER_COLUMN))
        return jch_fail(ctx, JCH_EINVAL, "%s: bad mode %d", who, mode);
    if (mode == JCH_FIR_VALID && (lo != 0 || f > p))
        return jch_fail(ctx, JCH_EINVAL, "%s: VALID needs lo == 0 and f <= p (f=%lld p=%lld lo=%lld)", who, (long long)f, (long long)p, (long long)lo);
    if (lo > 0 || lo < -(f - 1))
        return jch_fail(ctx, JCH_EINVAL, "%s: the window must contain its output, -(f - 1) <= lo <= 0 (f=%lld lo=%lld)", who, (long long)f, (long long)lo);
    JCH_TRY(rp_check(ctx, who, loc, X, n, p, ldx, out, ldo));
    const int64_t pout = mode == JCH_FIR_VALID ? p - f + 1 : p;
    if (f > INT32_MAX) return jch_fail(ctx, JCH_EINVAL, "%s: f=%lld too large", who, (long long)f);
    if (mode & JCH_FIR_PER_COLUMN) return rp_fir_per_column(ctx, loc, X, n, p, ldx, taps, f, lo, out, ldo);
    // the nonzero taps as (weight, t) pairs, in the order of t: [nnz doubles][nnz ints] in one buffer (at least one slot each)
    std::vector<double> wv;
    std::vector<int> ov;
    for (int64_t t = 0; t < f; ++t)
        if (taps[t] != 0.0) { wv.push_back(taps[t]); ov.push_back((int)t); }
    const int nnz = (int)wv.size();
    std::vector<double> packed((size_t)std::max(nnz, 1) + ((size_t)std::max(nnz, 1) + 1) / 2, 0.0);
    if (nnz) {
        memcpy(packed.data(), wv.data(), sizeof(double) * (size_t)nnz);
        memcpy(packed.data() + nnz, ov.data(), sizeof(int) * (size_t)nnz);
    }
    const double *wdev = nullptr;
    JCH_TRY(rp_coef(ctx, packed.data(), packed.size(), &wdev));
    const int *odev = (const int *)(wdev + nnz);
    return rp_run(ctx, loc, X, n, p, ldx, out, ldo, pout, [&](const double *x, int64_t rows, int64_t ld, double *o, int64_t ldout) -> int32_t {
        if (f <= RP_FIR_MAXF) {
            int slots = 1;
            while (slots < f + RP_U - 1) slots <<= 1;
            hipLaunchKernelGGL(k_rp_fir_ring, dim3(rp_grid(rows, RP_FIR_NT)), dim3(RP_FIR_NT), sizeof(double) * (size_t)slots * RP_FIR_NT, ctx->stream, x, rows,
                               p, ld, wdev, odev, nnz, (int)f, (int)lo, pout, slots - 1, o, ldout);
            JCH_HIP(ctx, hipGetLastError());
            return JCH_OK;
        }
        // wider windows: every output reads its taps straight from the input; in place, a bounded block of rows is copied aside first
        if (o != x) {
            hipLaunchKernelGGL(k_rp_fir_copy, dim3(jch_grid1(ctx, rows * pout)), dim3(RP_NT), 0, ctx->stream, x, rows, p, ld, wdev, odev, nnz, lo, pout, o, ldout);
            JCH_HIP(ctx, hipGetLastError());
            return JCH_OK;
        }
        const int64_t rb = rp_block_rows(rows, p);
        JCH_TRY(jch_reserve(ctx, ctx->rp_rows, sizeof(double) * (size_t)rb * (size_t)p));
        double *W = (double *)ctx->rp_rows.ptr;
        for (int64_t r0 = 0; r0 < rows; r0 += rb) {
            const int64_t m = std::min(rb, rows - r0);
            JCH_TRY(jch_copy2d(ctx, W, rb, x + r0, ld, m, p, hipMemcpyDeviceToDevice));
            hipLaunchKernelGGL(k_rp_fir_copy, dim3(jch_grid1(ctx, m * pout)), dim3(RP_NT), 0, ctx->stream, W, m, p, rb, wdev, odev, nnz, lo, pout, o + r0, ldout);
            JCH_HIP(ctx, hipGetLastError());
        }
        return JCH_OK;
    });
}
