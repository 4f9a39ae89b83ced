// Arguments shared by the batched local-fit kernels of the kNN-LWPLSR prediction path (lwplsr.hip: k_locw_plskern, the
// p-space kernel; lwplsr_kspace.hip: k_locw_kspace, the Gram / k-space kernel) — src/locwlv.jl:9-48.
#pragma once
#include <algorithm>
#include <vector>

#include "jch_internal.h"

struct locw_args {
    const double *Xrm; int ldr; int p;      // row-major training X (uncentred)
    const double *Y; int64_t ldy; int q;    // training Y (column-major n x q)
    const double *Xq; int64_t ldxq; int m;  // queries, column-major m x p
    const int *ind; const double *w; int k; // neighbours / weights [m][k]
    int scal, nlv_lo, nlv_hi;
    double *scratch; size_t slab;           // per-block global scratch (p-space kernel: Xg [k][ldr], P [nlv][ldr], R [nlv][ldr]; k-space kernel: [ldr] column stds)
    double *pred;                           // [m][le][q], le = nlv_hi - nlv_lo + 1
    int dbg;                                // measurement switches (JCH_LOCW_DBG; results then wrong by design): 1 = every query gathers rows 0 .. k-1
    int *flags;                             // [m] or null.  k-space kernel: flags[i] = 1 when query i lies too far from its neighbours for the
                                            // Gram matrix about the query row (pivot check, lwplsr_kspace.hip): the caller refits those queries
    // p-space kernel only, all optional (null / 0: nothing changes) — the local scores for the discriminants of lwplsda.hip
    double *tloc = nullptr;                 // [m][k][nlv_hi]: the score of neighbour e on LV a at ((i k + e) nlv_hi + a); columns beyond the local model's LVs are 0
    double *tqv = nullptr;                  // [m][nlv_hi]: the query's own scores
    const int *cls = nullptr;               // [n] training class codes, read with da
    int da = 0;                             // discrimination: Y is a dummy table.  A neighbourhood of one class is not fitted (info = 1, src/locwlv.jl:25-28
                                            // on the label column); a response whose local weighted sd is 0 (a class absent from the neighbourhood) is a zero column
    int *info = nullptr;                    // [m], written with da: 1 = unanimous neighbourhood (nothing else written for the query), 0 otherwise
    // p-space kernel only, optional, all three or none (null: the kernel without them) — the Shenk norms of the local models (lwplsravg.hip)
    double *rss_r = nullptr;                // [m][nlv_hi]: |xresid| of the query after a + 1 local LVs at (i nlv_hi + a), in the original scale
    double *rss_b = nullptr;                // [m][nlv_hi]: sqrt((|int|^2 + |B|^2) / q) of the local model with a + 1 LVs
    int *shenk_info = nullptr;              // [m]: 1 = constant univariate y in the neighbourhood (nothing fitted, the norms not written), 0 otherwise
};

// lwplsr_kspace.hip: _feasible: the k-space kernel can take this shape (k <= 208, q <= 8, nlv <= 48, p <= 2048);
// _supported: ... and is expected to beat the p-space kernel there
bool jch_locw_kspace_feasible(const locw_args &g);
bool jch_locw_kspace_supported(const locw_args &g);
int32_t jch_launch_locw_kspace(jch_ctx *ctx, locw_args &g);

// Arguments of the kNN + weights stage (lwplsr.hip: k_knn_scan / k_knn_finish; lwplsr_generic.hip: k_knn_generic) — src/getknn.jl:29-57,
// src/wdist.jl:64-75.
struct knn_args {
    const double *Zt; int64_t ldzt; int64_t n;   // train scores, column-major n x dd
    const double *Zq; int64_t ldzq; int m;       // query scores, column-major m x dd
    int dd, k;
    double h, cri, tol;
    int *ind;      // [m][k]
    double *dist;  // [m][k]
    double *w;     // [m][k]
    int nseg;      // the training rows are scanned in nseg segments by different workgroups (block b: segment b % nseg, query group b / nseg)
    double *ckey;  // [m][nseg][k] squared distances of every segment's k best (ascending; +inf beyond the segment's rows)
    int *cidx;     // [m][nseg][k]
    const int *only_flags = nullptr;   // null, or [m] device flags — only the queries with a non-zero flag are done (k_knn_scan: only their groups of qb)
};
// the search of m queries (Zq, ld ldzq) among the n rows of Zt (ld n; a caller with another pitch sets ldzt), cri = 4 (src/wdist.jl:64); nseg, ckey, cidx: the scan's own
inline knn_args jch_knn_make_args(const double *Zt, int64_t n, int64_t dd, const double *Zq, int64_t ldzq, int64_t m, int k, double h, double tol, int *ind,
                                  double *dist, double *w)
{
    knn_args a{};
    a.Zt = Zt; a.ldzt = n; a.n = n; a.Zq = Zq; a.ldzq = ldzq; a.m = (int)m; a.dd = (int)dd; a.k = k;
    a.h = h; a.cri = 4.0; a.tol = tol; a.ind = ind; a.dist = dist; a.w = w;
    return a;
}

// lwplsr_screen.hip: the screened kNN (round 4).  Squared distances of ALL (row, query) pairs on the matrix cores
// (v_mfma_f32_32x32x16_bf16 on two-piece bf16, norm-augmented operands), an error-bounded bar per query from the k-th smallest GROUP minimum, exact
// f64 distances only for the survivors (k .. ~1.2 k rows per query); queries the screen cannot settle (non-finite scores, more
// survivors than the candidate list holds) are flagged and done by k_knn_generic.  Results identical to k_knn_scan's.
struct knn_screen {          // the model-constant part: built once per prepared model, or per call in the ctx workspace
    uint4 *Zs = nullptr;     // [ntiles][KS][64 lanes] operand-ordered two-piece bf16 copy of the centred training scores (+ the |z|^2 and 1 slots)
    double *Zr = nullptr;    // [n][ldzr] row-major f64 copy of the scores (uncentred, the caller's values): one 8 dd-byte read per exact distance
    int ldzr = 0;
    double *mu = nullptr;    // [dd] column means the copy is centred on (distances do not depend on them)
    unsigned *hdr = nullptr; // [0] bits of max |z|^2 (f32) over the rows, [1] non-zero: a training score is not finite
    int KS = 0;              // k-steps of 16 operand slots: 16 KS >= 3 dd + 4
    int64_t ntiles = 0;      // 32-row tiles
};
bool jch_knn_screen_shape_ok(int64_t n, int dd, int k);
size_t jch_knn_screen_model_bytes(int64_t n, int dd);
// mem: jch_knn_screen_model_bytes(n, dd) bytes of device memory (256-B aligned) that `out` is carved from
int32_t jch_knn_screen_build(jch_ctx *ctx, const double *dZt, int64_t ldzt, int64_t n, int dd, void *mem, knn_screen *out);
// flags: [m] device ints, set to 1 for the queries handed to the exact selection (0 otherwise)
int32_t jch_launch_knn_screen(jch_ctx *ctx, const knn_args &a, const knn_screen &sc, int *flags);

// lwplsr.hip: row-major copy Xrm [n][ldr] of a column-major n x p matrix (columns p .. ldr - 1 zero), on the ctx stream
void jch_lw_to_rowmajor(jch_ctx *ctx, const double *dX, int64_t ldxd, int64_t n, int p, double *Xrm, int ldr);
// lwplsr.hip: the exact scan (k <= 768, LDS for the score space: jch_knn_scan_lds <= 150 KB)
size_t jch_knn_scan_lds(int dd);
int32_t jch_launch_knn_scan(jch_ctx *ctx, knn_args a, jch_buf &cbuf);
// lwplsr.hip: the search of one call — screen, scan or generic selection by shape and knobs (lw_run; jch_knn_search, knn.hip)
int32_t jch_knn_dispatch(jch_ctx *ctx, knn_args a, const knn_screen *scr, const bool *screen_off, int **sflags_out);

// lwplsr_generic.hip: the paths WITHOUT shape limits (any k <= n, any p, q, nlv) behind the batched kernels' envelope.
// kNN + weights of all m queries: exact selection of the k smallest distances per query, (distance, index) order, wdist weights
int32_t jch_launch_knn_generic(jch_ctx *ctx, const knn_args &a);
// local fits one query at a time: gather the neighbour rows, jch_plskern_fit on them, jch_predict on the query row (the
// reference's own schedule, src/locwlv.jl:18-39); dpred [m][le][q] device
int32_t jch_lw_generic_fits(jch_ctx *ctx, const locw_args &g, int64_t n, const int *only = nullptr /*host: query indices to fit (null: all)*/, int n_only = 0);

// The model-constant part of a prediction (jch_lwplsr_prepare, lwplsr.hip): the handle of include/jchemo_hip.h
struct jch_lwplsr_model {
    int device = 0;
    int64_t n = 0, p = 0, q = 0, dd = 0;
    int ldr = 0;
    double *Xrm = nullptr;   // [n][ldr]
    double *Y = nullptr;     // n x q, column-major, ld n
    double *Zt = nullptr;    // n x dd, column-major, ld n
    // optional: the map that takes a query block to the neighbour-search space, as a chain of affine maps (the reference's
    // transform(fm, X) followed by the whitening of getknn: two stages) kept on the device — jch_lwplsr_add_query_map
    struct qmap { int p_in = 0, k_out = 0, kpad = 0; double *dB = nullptr; };   // dB: [p_in][kpad] folded B, then kpad folded biases
    std::vector<qmap> qmaps;
    // the operand-ordered f32 copy of the scores for the screened kNN (lwplsr_screen.hip); absent when the score space is too wide
    bool has_screen = false;
    mutable bool screen_off = false;   // set when a call had a quarter of its queries redone by the exact scan
    knn_screen screen;
    void *screen_mem = nullptr;
};
// lwplsr.hip: the shape fits the p-space local-fit kernel (the one that can hand out its local scores), and its launch
bool jch_locw_pspace_fits(const locw_args &g);
int32_t jch_launch_locw_pspace(jch_ctx *ctx, locw_args &g);
// lwplsr.hip: the front end of a prediction on a prepared model, for jch_lwplsr_predict_prepared and jch_lwplsda_predict_prepared (lwplsda.hip); who: the
// entry's name in the messages.  _check: Zq or a query map that ends in the model's dd columns, and the model on the ctx's device — called among the
// entry's own argument checks, so that every bad call keeps its message.  Then, inside the entry's jch_synced frame, _stage: the ctx->xq reservation and
// the upload of a host call's Zq / Xq (q: the caller's pointers and pitches in, the device's out), the profile reset; _map (Zq null): Xq -> the
// neighbour-search space, stage by stage in the two halves of ctx->qz.
struct lw_queries { const double *Zq; int64_t ldzq; const double *Xq; int64_t ldxq; };
int32_t jch_lw_front_check(jch_ctx *ctx, const char *who, const jch_lwplsr_model *model, const double *Zq);
int32_t jch_lw_front_stage(jch_ctx *ctx, const jch_lwplsr_model *model, bool host, int64_t m, lw_queries *q);
int32_t jch_lw_front_map(jch_ctx *ctx, const jch_lwplsr_model *model, int64_t m, lw_queries *q);

// A per-query slab of slab_doubles doubles (k_knn_wls, lwmlr.hip; k_knn_gda, lwplsda.hip) lives in dynamic LDS or, beyond lds_max_bytes or with
// force_workspace, in one piece per workgroup of a workspace (glob).  nb, the workgroups of the launch: what the LDS lets a CU hold (at most 8 of 256
// threads); beyond the LDS four per CU, their slabs within 1 GiB
struct jch_slab_where { bool glob; int64_t nb; };
inline jch_slab_where jch_slab_plan(const jch_ctx *ctx, int64_t m, size_t slab_doubles, size_t lds_max_bytes, bool force_workspace)
{
    const size_t bytes = slab_doubles * sizeof(double);
    if (bytes > lds_max_bytes || force_workspace)
        return {true, std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(m, (int64_t)ctx->cus * 4), (int64_t)(((size_t)1 << 30) / bytes)))};
    return {false, std::min<int64_t>(m, (int64_t)ctx->cus * std::max<int64_t>(1, std::min<int64_t>(8, (160 * 1024) / (int64_t)bytes)))};
}

// lwplsda.hip: the nested Gaussian discriminants of a neighbourhood (k_knn_gda); all pointers on the device
struct gda_args {
    const double *T; int64_t tstride; int ldt;   // scores: neighbour e of query i on LV j at T[i tstride + e ldt + j]
    const double *tq; int ldq;                   // the queries' scores [m][ldq]
    const int *cls;                              // [m][k] class codes of the neighbours
    int m, k, a, nlev, kind, prior;              // a: the score columns that are factorised (models beyond a clamp to a); kind 1 lda, 2 qda; prior 0 unif, 1 prop
    int nlv_lo, nlv_hi;                          // the models, 1 <= nlv_lo <= nlv_hi
    double *post; int *code; int *info;          // [m][le][nlev], [m][le], [m][le]
    double *scratch; size_t per_block;           // null (LDS) or one slab of per_block doubles per workgroup
};
size_t jch_knn_gda_slab_doubles(int64_t k, int64_t a, int64_t nlev);
jch_slab_where jch_knn_gda_plan(jch_ctx *ctx, int64_t m, int64_t k, int64_t a, int64_t nlev, size_t *slab);
int32_t jch_launch_knn_gda(jch_ctx *ctx, const gda_args &g, int64_t nb);

// lwplsr_generic.hip: the discrimination fits outside the p-space kernel's envelope, one query at a time (hcn: HOST [m][k] neighbour class codes)
int32_t jch_lw_generic_fits_da(jch_ctx *ctx, const locw_args &g, const int *hcn);

#ifdef __HIPCC__
// The launch of a slab kernel pair as jch_slab_plan placed it: KWS (the workspace instantiation, K<false>) without dynamic LDS, or KLDS (K<true>) with the
// slab in it, after the once-per-device rise of its dynamic LDS limit to lds_max_bytes; 256 threads
template <auto KLDS, auto KWS, class A>
static int32_t jch_launch_slab(jch_ctx *ctx, jch_slab_where at, size_t slab_doubles, int lds_max_bytes, const A &a)
{
    if (at.glob) hipLaunchKernelGGL(KWS, dim3((unsigned)at.nb), dim3(256), 0, ctx->stream, a);
    else {
        static jch_per_device_once attr;
        if (!attr.done(ctx->device)) {
            JCH_HIP(ctx, hipFuncSetAttribute((const void *)KLDS, hipFuncAttributeMaxDynamicSharedMemorySize, lds_max_bytes));
            attr.mark(ctx->device);
        }
        hipLaunchKernelGGL(KLDS, dim3((unsigned)at.nb), dim3(256), slab_doubles * sizeof(double), ctx->stream, a);
    }
    JCH_HIP(ctx, hipGetLastError());
    return JCH_OK;
}

#define KNN_CAP 1024   // candidate buffer per query (LDS) of the scan; the finishing kernels order at most this many (distance, index) pairs

// bitonic sort of `cap` (a power of two <= KNN_CAP) (key, idx) pairs in LDS, ascending by (key, idx); NT threads
template <int NT>
__device__ static void bitonic_sort_n(double *key, int *idx, int cap)
{
    const int tid = threadIdx.x;
    for (int size = 2; size <= cap; size <<= 1) {
        for (int stride = size >> 1, ls = 31 - __builtin_clz(size >> 1); stride > 0; stride >>= 1, --ls) {
            __syncthreads();
            for (int t = tid; t < cap / 2; t += NT) {
                // (shifts, not t / stride and t % stride: a runtime integer division is ~40 instructions on this ISA and was
                // 3/4 of the sort's time)
                const int lo = ((t >> ls) << (ls + 1)) | (t & (stride - 1)), hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const double a = key[lo], b = key[hi];
                const int ia = idx[lo], ib = idx[hi];
                const bool gt = (a > b) || (a == b && ia > ib) || (a != a && b == b);   // NaN sorts last
                if (gt == up) { key[lo] = b; key[hi] = a; idx[lo] = ib; idx[hi] = ia; }
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void knn_wavesync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// the barriers of a slab kernel (jch_slab_plan): a slab in the workspace (LDS = false) needs its stores fenced in front of them
template <bool LDS> __device__ __forceinline__ void slab_bsync() { if (!LDS) __threadfence_block(); __syncthreads(); }
template <bool LDS> __device__ __forceinline__ void slab_wsync() { if (!LDS) __threadfence_block(); knn_wavesync(); }

// The label rule of the family: the first maximum over the classes PRESENT in the neighbourhood, in code order, a NaN counting as the largest value
// (Julia's `argmax`) — `if (present && (best < 0 || knn_vote_better(v, bv))) { best = c; bv = v; }` over c ascending.
// a beats b as a class score: a NaN beats a number, else the larger one
__device__ __forceinline__ bool knn_vote_better(double a, double b) { return (a != a && b == b) || a > b; }
__device__ __forceinline__ bool knn_vote_same(double a, double b) { return a == b || (a != a && b != b); }
// cnt[c] = how many of the k neighbour class codes cl are c, for c < nlev: one class per thread of 256; every thread calls, a barrier follows
__device__ __forceinline__ void knn_class_counts(const int *cl, int k, int nlev, int *cnt)
{
    for (int c = threadIdx.x; c < nlev; c += 256) {
        int n = 0;
        for (int e = 0; e < k; ++e) n += cl[e] == c ? 1 : 0;
        cnt[c] = n;
    }
}
// The same network run by ONE wave (no workgroup barrier between the passes: a wave's LDS operations complete in order): the four
// waves of a scan workgroup sort the four queries' buffers side by side — 7 us per 1024 entries against 14 us x 4 queries with
// the workgroup-wide sort, which was half of the scan's time.
template <int PP>   // PP = pairs per lane and pass = cap / 128 (1 for cap <= 128): all of a pass's loads go out together
__device__ __forceinline__ void bitonic_sort_wave_pp(double *key, int *idx, int cap)
{
    const int lane = threadIdx.x & 63;
    for (int size = 2; size <= cap; size <<= 1) {
        for (int stride = size >> 1, ls = 31 - __builtin_clz(size >> 1); stride > 0; stride >>= 1, --ls) {
            knn_wavesync();
            double a[PP], b[PP];
            int ia[PP], ib[PP], lo[PP];
#pragma unroll
            for (int u = 0; u < PP; ++u) {
                const int t = lane + 64 * u;
                lo[u] = ((t >> ls) << (ls + 1)) | (t & (stride - 1));
                const int l = t < cap / 2 ? lo[u] : 0;
                a[u] = key[l]; b[u] = key[l + stride]; ia[u] = idx[l]; ib[u] = idx[l + stride];
            }
#pragma unroll
            for (int u = 0; u < PP; ++u) {
                const bool up = ((lo[u] & size) == 0);
                const bool gt = (a[u] > b[u]) || (a[u] == b[u] && ia[u] > ib[u]) || (a[u] != a[u] && b[u] == b[u]);   // NaN sorts last
                if (lane + 64 * u < cap / 2 && gt == up) { key[lo[u]] = b[u]; key[lo[u] + stride] = a[u]; idx[lo[u]] = ib[u]; idx[lo[u] + stride] = ia[u]; }
            }
        }
    }
    knn_wavesync();
}
__device__ static void bitonic_sort_wave(double *key, int *idx, int cap)
{
    if (cap <= 128) bitonic_sort_wave_pp<1>(key, idx, cap);
    else if (cap == 256) bitonic_sort_wave_pp<2>(key, idx, cap);
    else if (cap == 512) bitonic_sort_wave_pp<4>(key, idx, cap);
    else bitonic_sort_wave_pp<8>(key, idx, cap);
}

// 64 (key, idx) pairs, one per lane, into ascending (key, idx) order across the lanes of a wave: the bitonic network on registers
// (21 exchange steps through the lanes, no LDS, no barrier)
__device__ __forceinline__ void knn_sort64_lanes(double &kv, int &iv)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1)
#pragma unroll
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const double pk = __shfl_xor(kv, stride, 64);
            const int pi = __shfl_xor(iv, stride, 64);
            const bool keepmin = ((lane & stride) == 0) == ((lane & size) == 0);
            const bool p_first = (pk < kv) || (pk == kv && pi < iv);      // the partner's pair comes before mine
            const bool m_first = (kv < pk) || (kv == pk && iv < pi);
            const bool take = keepmin ? p_first : m_first;
            kv = take ? pk : kv;
            iv = take ? pi : iv;
        }
}

// The tail shared by the finishing kernels (k_knn_finish, k_knn_finish_screen), in two parts the callers run back to back.  okey / oidx [kk] hold the
// query's nearest squared distances and rows in (distance, index) order (sentinels +inf / 0x7fffffff where fewer than kk were found).
// Part 1, knn_tail_holes: writes the neighbour list and the distances, and leaves the distances (square-rooted) in okey.  256 threads; every thread calls.
__device__ static void knn_tail_holes(const knn_args &g, int qi, int kk, double *okey, const int *oidx)
{
    const int tid = threadIdx.x;
    const int k = g.k;
    int *oi = g.ind + (size_t)qi * k;
    double *od = g.dist + (size_t)qi * k;
    // fewer than k candidates with a finite distance (NaN / Inf in the query's or the training scores: no comparison
    // against the bar ever holds): the empty places keep the sentinel index.  They are given the in-range row `e` and a
    // NaN distance — wdist then yields weights 1 for the query exactly as the reference's arithmetic does (every
    // comparison with NaN is false, 0 / 0 -> NaN -> 1, src/wdist.jl:64-75) and nothing downstream reads out of bounds.
    for (int e = tid; e < kk; e += 256) {
        const bool hole = oidx[e] < 0 || (int64_t)oidx[e] >= g.n;
        oi[e] = hole ? e : oidx[e];
        const double dv = hole ? __builtin_nan("") : sqrt(okey[e]);
        okey[e] = dv;
        od[e] = dv;
    }
}
// Part 2, knn_tail_wdist: the wdist weights (src/wdist.jl:64-75) of the kk distances okey (not squared, ascending, NaN last; any address space) into
// ow [kk].  key: scratch of >= kk doubles; sred [8], smed [2], snn [4]: LDS.  256 threads; every thread calls, behind a barrier after okey was written.
__device__ static void knn_tail_wdist(double h, double cri, double tol, int kk, double *key, const double *okey, double *ow, double *sred, double *smed, int *snn)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // wdist (src/wdist.jl:64-75): median, MAD, cutoff, exp weights, / max, NaN -> 1, then the tol clamp
    const double med = (kk & 1) ? okey[kk / 2] : 0.5 * (okey[kk / 2 - 1] + okey[kk / 2]);
    // the median of |d - med|: the values at the places t0, t1 of the kk deviations in ascending order, NaN last.
    const int t1 = kk / 2, t0 = (kk & 1) ? -1 : kk / 2 - 1;
    const double dlast = okey[kk - 1];
    if (med == med && fabs(med) < __builtin_inf() && dlast == dlast && fabs(dlast) < __builtin_inf()) {   // (block-uniform)
        // All distances finite (they ascend; holes, NaN, would be last).  The deviations are then two monotone runs — descending up
        // to the first distance >= med, ascending from there — and an entry's place in their merged order is its place in its own
        // run plus a binary search of the other (round 4; was a count over all kk entries per entry: kk^2 steps, 10 of the
        // finishing kernel's 55 us at cfg5).  Ties: the descending run's entries first — any order of equal values puts the same
        // VALUE at a place.
        for (int e = tid; e < kk; e += 256) key[e] = fabs(okey[e] - med);
        if (tid == 0) snn[0] = kk;
        if (tid < 2) smed[tid] = __builtin_nan("");
        __syncthreads();
        for (int e = tid; e < kk; e += 256)
            if (okey[e] >= med && (e == 0 || okey[e - 1] < med)) snn[0] = e;
        __syncthreads();
        const int p = snn[0];
        for (int e = tid; e < kk; e += 256) {
            const double v = key[e];
            int r;
            if (e < p) {            // descending run, read backwards: ascending; entries of the other run strictly below v come first
                int lo = 0, hi = kk - p;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (key[p + mid] < v) lo = mid + 1; else hi = mid; }
                r = (p - 1 - e) + lo;
            } else {                // ascending run; entries of the other run at or below v come first
                int lo = 0, hi = p;
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (key[p - 1 - mid] <= v) lo = mid + 1; else hi = mid; }
                r = (e - p) + lo;
            }
            if (r == t1) smed[1] = v;
            if (r == t0) smed[0] = v;
        }
    } else {
        // (non-finite distances) by RANK COUNTING: entry e's place — by value, then by position, NaN last — is the number of entries
        // that come before it
        int nn = 0;
        for (int e = tid; e < kk; e += 256) { const double v = fabs(okey[e] - med); key[e] = v; nn += v == v ? 1 : 0; }
        for (int o = 32; o > 0; o >>= 1) nn += __shfl_xor(nn, o, 64);
        if (lane == 0) snn[wv] = nn;
        if (tid < 2) smed[tid] = __builtin_nan("");                // (a target place among the NaNs stays NaN)
        __syncthreads();
        nn = snn[0] + snn[1] + snn[2] + snn[3];
        for (int e = tid; e < kk; e += 256) {
            const double v = key[e];
            if (v != v) continue;
            int r = 0;
            for (int f = 0; f < kk; ++f) { const double u = key[f]; r += (u < v || (u == v && f < e)) ? 1 : 0; }
            if (r == t1) smed[1] = v;
            if (r == t0) smed[0] = v;
        }
    }
    __syncthreads();
    const double zmad = 1.4826 * ((kk & 1) ? smed[1] : 0.5 * (smed[0] + smed[1]));
    const double cutoff = med + cri * zmad;
    // weights; max with NaN propagation (Julia's `maximum` returns NaN if any NaN is present)
    double wmax = -__builtin_inf();
    int anynan = 0;
    __syncthreads();                                           // (key: the deviations are done with, the weights go there)
    for (int e = tid; e < kk; e += 256) {
        const double dv = okey[e];
        const double wv_ = dv <= cutoff ? exp(-dv / (h * zmad)) : 0.0;
        key[e] = wv_;
        if (wv_ != wv_) anynan = 1;
        else if (wv_ > wmax) wmax = wv_;
    }
    for (int o = 32; o > 0; o >>= 1) { wmax = fmax(wmax, __shfl_xor(wmax, o, 64)); anynan |= __shfl_xor(anynan, o, 64); }
    if (lane == 0) { sred[wv] = wmax; sred[4 + wv] = (double)anynan; }
    __syncthreads();
    wmax = fmax(fmax(sred[0], sred[1]), fmax(sred[2], sred[3]));
    if (sred[4] + sred[5] + sred[6] + sred[7] > 0.0) wmax = __builtin_nan("");
    for (int e = tid; e < kk; e += 256) {
        double wv_ = key[e] / wmax;
        if (wv_ != wv_) wv_ = 1.0;
        if (wv_ < tol) wv_ = tol;
        ow[e] = wv_;
    }
}
__device__ static void knn_finish_tail(const knn_args &g, int qi, int kk, double *key, double *okey, int *oidx, double *sred, double *smed, int *snn)
{
    knn_tail_holes(g, qi, kk, okey, oidx);
    __syncthreads();
    knn_tail_wdist(g.h, g.cri, g.tol, kk, key, okey, g.w + (size_t)qi * g.k, sred, smed, snn);
}

// ascending bitonic sort of cap (power of two) (key, idx) pairs by (key, idx), NaN last; any address space; 256 threads
__device__ static void kg_bitonic(double *key, int *idx, int cap)
{
    const int tid = threadIdx.x;
    for (int size = 2; size <= cap; size <<= 1) {
        for (int stride = size >> 1, ls = 31 - __builtin_clz(size >> 1); stride > 0; stride >>= 1, --ls) {
            __syncthreads();
            for (int t = tid; t < cap / 2; t += 256) {
                const int lo = ((t >> ls) << (ls + 1)) | (t & (stride - 1)), hi = lo + stride;
                const bool up = ((lo & size) == 0);
                const double a = key[lo], b = key[hi];
                const int ia = idx[lo], ib = idx[hi];
                const bool gt = (a > b) || (a == b && ia > ib) || (a != a && b == b);
                if (gt == up) { key[lo] = b; key[hi] = a; idx[lo] = ib; idx[hi] = ia; }
            }
        }
    }
    __syncthreads();
}
#endif
