// The k-nearest-neighbour search on its own, and what the reference builds on it besides lwplsr (src/getknn.jl:29-57, src/knnr.jl:119-169,
// src/knnda.jl:87-138, src/occknndis.jl:125-171, src/occlknndis.jl:132-199) — jch_knn_*, include/jchemo_hip.h; DESIGN.md §20.
//
// The search itself is lwplsr's (jch_knn_dispatch, lwplsr.hip: the screened search, the exact scan or the generic selection — the same kernels in the
// same order), run on a handle that keeps the search space and the screen's operand copy.  New here:
//   k_knn_post            one workgroup per query, behind a search for k + 1: drops the entry whose row is self[i] (else the last one), which is the
//                         search over the training rows without row self[i] — the list is in (distance, index) order, so the k kept entries are the
//                         first k of that order with the row taken out, duplicates at distance 0 included (tests/test_knn_static.py).  Then the wdist
//                         weights over the k KEPT distances (knn_tail_wdist, lwplsr_dev.h) and their median (the list is sorted: the middle place(s)).
//   k_knn_wmean           one wave per query: pred[i, :] = sum_j (w_ij / sum_j w_ij) Y[ind_ij, :] (`mweight` + `colmean`, src/knnr.jl:120-124).  Fixed
//                         order: lane l adds the terms l, l + 64, ... in that order, the 64 partial sums combine in the xor butterfly of jch_wave_sum
//                         (strides 32, 16, ..., 1); the same for sum_j w_ij.  No atomics: two runs give identical bits.
//   k_knn_vote            one workgroup per query: score[i, c] = sum of w_ij over the neighbours of class c, added in neighbour order by the one thread
//                         that owns class c (c mod 256), so no atomics; the (class, weight) pairs of 256 neighbours at a time are staged in LDS.  The
//                         accumulators live in LDS up to KNN_VOTE_LDS classes and in global memory beyond.  pred[i] = the best class PRESENT in the
//                         neighbourhood, ties to the lowest code (`findmax_cla`, src/utility.jl:564-570: `argmax` over the sorted levels; a NaN sum wins,
//                         the first one, as Julia's `argmax` has it).
//   k_knn_gather_median   one workgroup per query: the median of v[ind_ij] by a bitonic sort of the k gathered values, NaN last (LDS for k <= KNN_CAP,
//                         global memory beyond), `middle(lo, hi) = lo / 2 + hi / 2` for even k.
// Every kernel reads at most k gathered values per query and checks every gathered index against n (a bad index contributes NaN, never a read out of
// bounds).  gfx950, hipcc -O3.
#include <stdint.h>

#include <algorithm>
#include <new>
#include <vector>

#include "jch_internal.h"
#include "lwplsr_dev.h"

#define KNN_VOTE_LDS 2048   // classes whose accumulators fit the workgroup's LDS (24 KB)

struct jch_knn_model {
    int device = 0;
    int64_t n = 0, dd = 0;
    double *Zt = nullptr;    // n x dd, column-major, ld n
    bool has_screen = false;
    mutable bool screen_off = false;   // set when a host-output call had a quarter of its queries redone by the exact scan
    knn_screen screen;
    void *screen_mem = nullptr;
};

struct knn_post_args {
    const int *sind; const double *sdist;   // [m][k1] the search's lists
    int k1, k, m;
    const int64_t *self;                    // [m] or null
    double h, cri, tol;
    int *ind; double *dist; double *w; double *dmed;   // [m][k] x 3, [m]; each may be null
    double *scratch;                        // null (k <= KNN_CAP: LDS) or [blocks][2 k]
};

__global__ __launch_bounds__(256) void k_knn_post(knn_post_args g)
{
    __shared__ double s_okey[KNN_CAP], s_key[KNN_CAP];
    __shared__ double sred[8], smed[2];
    __shared__ int snn[4];
    __shared__ int spos;
    const int tid = threadIdx.x, k = g.k, k1 = g.k1;
    double *okey = g.scratch ? g.scratch + (size_t)blockIdx.x * 2 * (size_t)k : s_okey;
    double *key = g.scratch ? okey + k : s_key;
    for (int qi = blockIdx.x; qi < g.m; qi += gridDim.x) {
        const int *si = g.sind + (size_t)qi * k1;
        const double *sd = g.sdist + (size_t)qi * k1;
        __syncthreads();
        if (tid == 0) spos = k1 - 1;                         // (k1 == k: nothing is dropped, see `src` below)
        __syncthreads();
        const int64_t s = (g.self && k1 > k) ? g.self[qi] : -1;
        if (s >= 0)   // at most one entry matches: the rows of the entries with a distance are distinct (holes carry NaN and a made-up row)
            for (int e = tid; e < k1; e += 256)
                if ((int64_t)si[e] == s && sd[e] == sd[e]) spos = e;
        __syncthreads();
        const int pos = k1 > k ? spos : k1;
        for (int e = tid; e < k; e += 256) {
            const int src = e + (e >= pos ? 1 : 0);
            const double dv = sd[src];
            okey[e] = dv;
            if (g.ind) g.ind[(size_t)qi * k + e] = si[src];
            if (g.dist) g.dist[(size_t)qi * k + e] = dv;
        }
        __syncthreads();
        if (g.dmed && tid == 0) g.dmed[qi] = (k & 1) ? okey[k / 2] : okey[k / 2 - 1] / 2 + okey[k / 2] / 2;
        if (g.w) knn_tail_wdist(g.h, g.cri, g.tol, k, key, okey, g.w + (size_t)qi * k, sred, smed, snn);   // (block-uniform)
    }
}

__global__ __launch_bounds__(256) void k_knn_wmean(const double *__restrict__ Y, int64_t n, int q, int64_t ldy, const int *__restrict__ ind,
                                                   const double *__restrict__ w, int m, int k, double *__restrict__ pred)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int qi = blockIdx.x * 4 + wv; qi < m; qi += (int)gridDim.x * 4) {      // (wave-uniform)
        const int *ii = ind + (size_t)qi * k;
        const double *ww = w + (size_t)qi * k;
        double s = 0.0;
        for (int e = lane; e < k; e += 64) s += ww[e];
        const double sw = jch_wave_sum(s);
        for (int c = 0; c < q; ++c) {
            const double *yc = Y + (size_t)c * (size_t)ldy;
            double acc = 0.0;
            for (int e = lane; e < k; e += 64) {
                const int r = ii[e];
                const double y = (r >= 0 && (int64_t)r < n) ? yc[r] : __builtin_nan("");
                acc += (ww[e] / sw) * y;
            }
            acc = jch_wave_sum(acc);
            if (lane == 0) pred[(size_t)qi + (size_t)c * (size_t)m] = acc;
        }
    }
}

__global__ __launch_bounds__(256) void k_knn_vote(const int *__restrict__ cls, int64_t n, int ncls, const int *__restrict__ ind, const double *__restrict__ w,
                                                  int m, int k, int *__restrict__ pred, double *__restrict__ score, double *gacc, int *gcnt)
{
    __shared__ double s_acc[KNN_VOTE_LDS];
    __shared__ int s_cnt[KNN_VOTE_LDS];
    __shared__ double cw[256];
    __shared__ int cc[256];
    __shared__ double bv[4];
    __shared__ int bc[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double *acc = gacc ? gacc + (size_t)blockIdx.x * (size_t)ncls : s_acc;
    int *cnt = gacc ? gcnt + (size_t)blockIdx.x * (size_t)ncls : s_cnt;
    for (int qi = blockIdx.x; qi < m; qi += gridDim.x) {
        const int *ii = ind + (size_t)qi * k;
        const double *ww = w + (size_t)qi * k;
        for (int c = tid; c < ncls; c += 256) { acc[c] = 0.0; cnt[c] = 0; }   // (a thread touches the classes c = tid mod 256 only, here and below)
        for (int e0 = 0; e0 < k; e0 += 256) {
            __syncthreads();                                   // (the previous chunk, or the previous query's last one, is done with)
            const int e = e0 + tid;
            int c = -1;
            double wv_ = 0.0;
            if (e < k) {
                const int r = ii[e];
                if (r >= 0 && (int64_t)r < n) c = cls[r];
                wv_ = ww[e];
            }
            cc[tid] = (c >= 0 && c < ncls) ? c : -1;
            cw[tid] = wv_;
            __syncthreads();
            const int ne = min(256, k - e0);
            for (int f = 0; f < ne; ++f) {
                const int c2 = cc[f];
                if (c2 >= 0 && (c2 & 255) == tid) { acc[c2] += cw[f]; cnt[c2] += 1; }
            }
        }
        int best = -1;
        double bval = 0.0;
        for (int c = tid; c < ncls; c += 256) {                // ascending codes: a tie keeps the lower one
            const bool present = cnt[c] > 0;
            const double v = acc[c];
            if (score) score[(size_t)qi + (size_t)c * (size_t)m] = present ? v : 0.0;
            if (present && (best < 0 || knn_vote_better(v, bval))) { best = c; bval = v; }
        }
        auto merge = [&](int oc, double ov) {
            if (oc >= 0 && (best < 0 || knn_vote_better(ov, bval) || (knn_vote_same(ov, bval) && oc < best))) { best = oc; bval = ov; }
        };
        for (int o = 32; o > 0; o >>= 1) {
            const int oc = __shfl_xor(best, o, 64);
            const double ov = __shfl_xor(bval, o, 64);
            merge(oc, ov);
        }
        if (lane == 0) { bv[wv] = bval; bc[wv] = best; }
        __syncthreads();
        if (tid == 0) {
            for (int u = 1; u < 4; ++u) merge(bc[u], bv[u]);
            pred[qi] = best;
        }
    }
}

__global__ __launch_bounds__(256) void k_knn_gather_median(const double *__restrict__ v, int64_t n, const int *__restrict__ ind, int m, int k, int cap,
                                                           double *__restrict__ out, double *gkey, int *gidx)
{
    __shared__ double s_key[KNN_CAP];
    __shared__ int s_idx[KNN_CAP];
    const int tid = threadIdx.x;
    double *key = gkey ? gkey + (size_t)blockIdx.x * (size_t)cap : s_key;
    int *idx = gkey ? gidx + (size_t)blockIdx.x * (size_t)cap : s_idx;
    for (int qi = blockIdx.x; qi < m; qi += gridDim.x) {
        const int *ii = ind + (size_t)qi * k;
        __syncthreads();
        for (int e = tid; e < cap; e += 256) {                 // the padding is NaN too: it sorts last with the gathered NaNs
            double x = __builtin_nan("");
            if (e < k) { const int r = ii[e]; if (r >= 0 && (int64_t)r < n) x = v[r]; }
            key[e] = x;
            idx[e] = e;
        }
        __syncthreads();
        if (gkey) kg_bitonic(key, idx, cap); else bitonic_sort_n<256>(key, idx, cap);
        if (tid == 0) out[qi] = (k & 1) ? key[k / 2] : key[k / 2 - 1] / 2 + key[k / 2] / 2;
    }
}

// ---------------------------------------------------------------- C ABI
extern "C" int32_t jch_knn_prepare(jch_ctx *ctx, int32_t loc, const double *Ztrain, int64_t n, int64_t dd, int64_t ldzt, jch_knn_model **model_out)
{
    if (!ctx) return JCH_EINVAL;
    if (!model_out) return jch_fail(ctx, JCH_EINVAL, "jch_knn_prepare: model_out is NULL");
    *model_out = nullptr;
    if (!Ztrain || n < 1 || dd < 1 || ldzt < n || n >= ((int64_t)1 << 31) - 1 || dd > (1 << 20)) return jch_fail(ctx, JCH_EINVAL, "jch_knn_prepare: bad arguments");
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "jch_knn_prepare: bad loc");
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    jch_knn_model *mo = new (std::nothrow) jch_knn_model();
    if (!mo) return jch_fail(ctx, JCH_ENOMEM, "jch_knn_prepare: host allocation failed");
    mo->device = ctx->device; mo->n = n; mo->dd = dd;
    auto fail = [&](int32_t st) { (void)hipFree(mo->Zt); (void)hipFree(mo->screen_mem); delete mo; return st; };
    if (hipMalloc((void **)&mo->Zt, sizeof(double) * (size_t)n * (size_t)dd) != hipSuccess)
        return fail(jch_fail(ctx, JCH_ENOMEM, "jch_knn_prepare: device allocation failed (%lld x %lld search space)", (long long)n, (long long)dd));
    if (jch_copy2d(ctx, mo->Zt, n, Ztrain, ldzt, n, dd, loc == JCH_LOC_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice) != JCH_OK)
        return fail(jch_fail(ctx, JCH_EHIP, "jch_knn_prepare: copy of the search space failed"));
    if (dd <= 62 && n < ((int64_t)1 << 26)) {   // (whether a call is screened also depends on its k: jch_knn_screen_shape_ok)
        // (no memory for the operand copy: the handle works without it — every screened call then builds it in the ctx workspace)
        if (hipMalloc(&mo->screen_mem, jch_knn_screen_model_bytes(n, (int)dd)) != hipSuccess) { mo->screen_mem = nullptr; (void)hipGetLastError(); }
        else {
            const int32_t st = jch_knn_screen_build(ctx, mo->Zt, n, n, (int)dd, mo->screen_mem, &mo->screen);
            if (st != JCH_OK) return fail(st);
            mo->has_screen = true;
        }
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
        return fail(jch_fail(ctx, JCH_EHIP, "jch_knn_prepare: building the handle failed"));
    *model_out = mo;
    return JCH_OK;
}

extern "C" int32_t jch_knn_release(jch_ctx *ctx, jch_knn_model *model)
{
    if (!model) return JCH_OK;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
    }
    (void)hipFree(model->Zt); (void)hipFree(model->screen_mem);
    delete model;
    return JCH_OK;
}

extern "C" int32_t jch_knn_search(jch_ctx *ctx, const jch_knn_model *model, int32_t loc, const double *Zq, int64_t m, int64_t ldzq, int32_t k,
                                  const int64_t *self, double h, double tol, int32_t out_loc, int32_t *ind, double *dist, double *w, double *dmed)
{
    if (!ctx) return JCH_EINVAL;
    if (!model || !Zq || m < 1 || ldzq < m || k < 1 || m >= ((int64_t)1 << 31) - 1) return jch_fail(ctx, JCH_EINVAL, "jch_knn_search: bad arguments");
    if ((loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) || (out_loc != JCH_LOC_HOST && out_loc != JCH_LOC_DEVICE)) return jch_fail(ctx, JCH_EINVAL, "jch_knn_search: bad loc / out_loc");
    if (model->device != ctx->device) return jch_fail(ctx, JCH_EINVAL, "jch_knn_search: the handle lives on device %d, the ctx on %d", model->device, ctx->device);
    const int64_t n = model->n, dd = model->dd;
    const int64_t kmax = self ? n - 1 : n;                     // src/getknn.jl:33 on the rows that are left
    if (kmax < 1) return jch_fail(ctx, JCH_EINVAL, "jch_knn_search: no candidate is left when the only training row is removed");
    if (k > kmax) k = (int32_t)kmax;
    const int k1 = self ? k + 1 : k;                           // (<= n)
    if ((size_t)m * (size_t)k1 >= ((size_t)1 << 40)) return jch_fail(ctx, JCH_EINVAL, "jch_knn_search: m x k too large");
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool post = self != nullptr || dmed != nullptr;
    const bool hin = loc == JCH_LOC_HOST, hout = out_loc == JCH_LOC_HOST;
    const size_t mk1 = (size_t)m * k1, mk = (size_t)m * k;
    const int post_blocks = (int)std::min<int64_t>(m, (int64_t)ctx->cus * 8);
    // ---- one reservation: staged inputs | the search's lists | the results of a host call | sort scratch beyond the LDS
    jch_carve cv;
    const size_t o_zq = hin ? cv.take((size_t)m * dd) : 0, o_self = (hin && self) ? cv.take((size_t)m) : 0;
    const size_t o_ad = cv.take(mk1), o_aw = cv.take(mk1), o_ai = cv.take(jch_ints_as_doubles(mk1));
    const bool bres = post && hout;
    const size_t o_bd = bres ? cv.take(mk) : 0, o_bw = bres ? cv.take(mk) : 0, o_bi = bres ? cv.take(jch_ints_as_doubles(mk)) : 0, o_bm = bres ? cv.take((size_t)m) : 0;
    const bool big = post && k > KNN_CAP;
    const size_t o_sc = big ? cv.take((size_t)post_blocks * 2 * (size_t)k) : 0;
    JCH_TRY(jch_reserve(ctx, ctx->kn_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->kn_ws.ptr;
    std::vector<int> hsf;   // the screen's per-query flags, fetched by a host-output call that was screened
    JCH_TRY(jch_synced(ctx, hin || hout, [&]() -> int32_t {
        const double *dZq = Zq;
        const int64_t *dself = self;
        int64_t ldq = ldzq;
        JCH_TRY(jch_stage_in(ctx, hin, ws + o_zq, m, dd, &dZq, &ldq));
        if (hin && self) {
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_self, self, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, ctx->stream));
            dself = (const int64_t *)(ws + o_self);
        }
        int *sflags = nullptr;
        knn_args a = jch_knn_make_args(model->Zt, n, dd, dZq, ldq, m, k1, h, tol, (int *)(ws + o_ai), ws + o_ad, ws + o_aw);
        if (!self && !hout) {   // no removal behind the search: it writes the caller's device arrays itself
            if (ind) a.ind = ind;
            if (dist) a.dist = dist;
            if (w) a.w = w;
        }
        JCH_TRY(jch_knn_dispatch(ctx, a, model->has_screen ? &model->screen : nullptr, &model->screen_off, &sflags));
        const int *rind = a.ind;
        const double *rdist = a.dist, *rw = a.w, *rmed = nullptr;
        if (post) {
            knn_post_args g;
            g.sind = a.ind; g.sdist = a.dist; g.k1 = k1; g.k = k; g.m = (int)m; g.self = dself; g.h = h; g.cri = 4.0; g.tol = tol;
            if (hout) {
                g.ind = ind ? (int *)(ws + o_bi) : nullptr; g.dist = dist ? ws + o_bd : nullptr;
                g.w = w ? ws + o_bw : nullptr; g.dmed = dmed ? ws + o_bm : nullptr;
            } else { g.ind = ind; g.dist = dist; g.w = w; g.dmed = dmed; }
            if (!self) { g.ind = nullptr; g.dist = nullptr; g.w = nullptr; }   // (k1 == k: the search's own lists and weights stand)
            g.scratch = big ? ws + o_sc : nullptr;
            hipLaunchKernelGGL(k_knn_post, dim3(post_blocks), dim3(256), 0, ctx->stream, g);
            JCH_HIP(ctx, hipGetLastError());
            if (self) { rind = g.ind; rdist = g.dist; rw = g.w; }
            rmed = g.dmed;
        }
        if (hout) {
            if (ind) JCH_HIP(ctx, hipMemcpyAsync(ind, rind, sizeof(int) * mk, hipMemcpyDeviceToHost, ctx->stream));
            if (dist) JCH_HIP(ctx, hipMemcpyAsync(dist, rdist, sizeof(double) * mk, hipMemcpyDeviceToHost, ctx->stream));
            if (w) JCH_HIP(ctx, hipMemcpyAsync(w, rw, sizeof(double) * mk, hipMemcpyDeviceToHost, ctx->stream));
            if (dmed) JCH_HIP(ctx, hipMemcpyAsync(dmed, rmed, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (sflags && hout) {
            hsf.resize((size_t)m);
            JCH_HIP(ctx, hipMemcpyAsync(hsf.data(), sflags, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        }
        return JCH_OK;
    }));
    if (!hsf.empty()) {
        long long redone = 0;
        for (int64_t i = 0; i < m; ++i) redone += hsf[(size_t)i] ? 1 : 0;
        ctx->knn_screened += (long long)m;
        ctx->knn_screen_redone += redone;
        // a search space whose geometry defeats the screen's error bound (lwplsr_screen.hip): the handle stops screening
        if (m >= 8 && redone * 4 > (long long)m) model->screen_off = true;
    }
    return JCH_OK;
}

// inputs of the three gather entries: ind [m][k] and one more array, staged into ctx->kn_ws for a host call
static int32_t knn_check_lists(jch_ctx *ctx, const char *who, int32_t loc, const void *a, const void *ind, const void *out, int64_t n, int64_t m, int64_t k)
{
    if (!a || !ind || !out || n < 1 || m < 1 || k < 1 || n >= ((int64_t)1 << 31) - 1 || m >= ((int64_t)1 << 31) - 1 || k >= ((int64_t)1 << 30) ||
        (size_t)m * (size_t)k >= ((size_t)1 << 40))
        return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments", who);
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc", who);
    return JCH_OK;
}

extern "C" int32_t jch_knn_wmean(jch_ctx *ctx, int32_t loc, const double *Y, int64_t n, int64_t q, int64_t ldy, const int32_t *ind, const double *w,
                                 int64_t m, int32_t k, double *pred)
{
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(knn_check_lists(ctx, "jch_knn_wmean", loc, Y, ind, pred, n, m, k));
    if (!w || q < 1 || q > (1 << 20) || ldy < n) return jch_fail(ctx, JCH_EINVAL, "jch_knn_wmean: bad arguments");
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t mk = (size_t)m * k;
    const bool host = loc == JCH_LOC_HOST;
    jch_carve cv;
    const size_t o_y = host ? cv.take((size_t)n * q) : 0, o_i = host ? cv.take(jch_ints_as_doubles(mk)) : 0, o_w = host ? cv.take(mk) : 0, o_p = host ? cv.take((size_t)m * q) : 0;
    if (host) JCH_TRY(jch_reserve(ctx, ctx->kn_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->kn_ws.ptr;
    return jch_synced(ctx, host, [&]() -> int32_t {
        const double *dY = Y, *dw = w;
        const int *di = ind;
        double *dp = pred;
        int64_t ldyd = ldy;
        JCH_TRY(jch_stage_in(ctx, host, ws + o_y, n, q, &dY, &ldyd));
        if (host) {
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_i, ind, sizeof(int) * mk, hipMemcpyHostToDevice, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_w, w, sizeof(double) * mk, hipMemcpyHostToDevice, ctx->stream));
            di = (const int *)(ws + o_i); dw = ws + o_w; dp = ws + o_p;
        }
        const unsigned nb = (unsigned)std::min<int64_t>((m + 3) / 4, (int64_t)ctx->cus * 8);
        hipLaunchKernelGGL(k_knn_wmean, dim3(nb), dim3(256), 0, ctx->stream, dY, n, (int)q, ldyd, di, dw, (int)m, (int)k, dp);
        JCH_HIP(ctx, hipGetLastError());
        if (host) JCH_HIP(ctx, hipMemcpyAsync(pred, dp, sizeof(double) * (size_t)m * q, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    });
}

extern "C" int32_t jch_knn_vote(jch_ctx *ctx, int32_t loc, const int32_t *cls, int64_t n, int32_t ncls, const int32_t *ind, const double *w, int64_t m,
                                int32_t k, int32_t *pred, double *score)
{
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(knn_check_lists(ctx, "jch_knn_vote", loc, cls, ind, pred, n, m, k));
    if (!w || ncls < 1) return jch_fail(ctx, JCH_EINVAL, "jch_knn_vote: bad arguments");
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t mk = (size_t)m * k;
    const bool host = loc == JCH_LOC_HOST, glob = ncls > KNN_VOTE_LDS;
    // beyond the LDS: one accumulator row per workgroup, within 1 GiB
    const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(m, (int64_t)ctx->cus * 8), glob ? ((int64_t)1 << 30) / (12 * (int64_t)ncls) : m));
    jch_carve cv;
    const size_t o_c = host ? cv.take(jch_ints_as_doubles((size_t)n)) : 0, o_i = host ? cv.take(jch_ints_as_doubles(mk)) : 0, o_w = host ? cv.take(mk) : 0;
    const size_t o_p = host ? cv.take(jch_ints_as_doubles((size_t)m)) : 0, o_s = (host && score) ? cv.take((size_t)m * ncls) : 0;
    const size_t o_ga = glob ? cv.take((size_t)nb * ncls) : 0, o_gc = glob ? cv.take(jch_ints_as_doubles((size_t)nb * ncls)) : 0;
    if (cv.off) JCH_TRY(jch_reserve(ctx, ctx->kn_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->kn_ws.ptr;
    return jch_synced(ctx, host, [&]() -> int32_t {
        const int *dc = cls, *di = ind;
        const double *dw = w;
        int *dp = pred;
        double *ds = score;
        if (host) {
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_c, cls, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_i, ind, sizeof(int) * mk, hipMemcpyHostToDevice, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_w, w, sizeof(double) * mk, hipMemcpyHostToDevice, ctx->stream));
            dc = (const int *)(ws + o_c); di = (const int *)(ws + o_i); dw = ws + o_w; dp = (int *)(ws + o_p); ds = score ? ws + o_s : nullptr;
        }
        hipLaunchKernelGGL(k_knn_vote, dim3((unsigned)nb), dim3(256), 0, ctx->stream, dc, n, (int)ncls, di, dw, (int)m, (int)k, dp, ds,
                           glob ? ws + o_ga : nullptr, glob ? (int *)(ws + o_gc) : nullptr);
        JCH_HIP(ctx, hipGetLastError());
        if (host) {
            JCH_HIP(ctx, hipMemcpyAsync(pred, dp, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
            if (score) JCH_HIP(ctx, hipMemcpyAsync(score, ds, sizeof(double) * (size_t)m * ncls, hipMemcpyDeviceToHost, ctx->stream));
        }
        return JCH_OK;
    });
}

extern "C" int32_t jch_knn_gather_median(jch_ctx *ctx, int32_t loc, const double *v, int64_t n, const int32_t *ind, int64_t m, int32_t k, double *out)
{
    if (!ctx) return JCH_EINVAL;
    JCH_TRY(knn_check_lists(ctx, "jch_knn_gather_median", loc, v, ind, out, n, m, k));
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const size_t mk = (size_t)m * k;
    const bool host = loc == JCH_LOC_HOST, glob = k > KNN_CAP;
    int cap = 64;
    while (cap < k) cap <<= 1;
    const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(m, (int64_t)ctx->cus * 8), glob ? ((int64_t)1 << 30) / (12 * (int64_t)cap) : m));
    jch_carve cv;
    const size_t o_v = host ? cv.take((size_t)n) : 0, o_i = host ? cv.take(jch_ints_as_doubles(mk)) : 0, o_o = host ? cv.take((size_t)m) : 0;
    const size_t o_gk = glob ? cv.take((size_t)nb * cap) : 0, o_gi = glob ? cv.take(jch_ints_as_doubles((size_t)nb * cap)) : 0;
    if (cv.off) JCH_TRY(jch_reserve(ctx, ctx->kn_ws, sizeof(double) * cv.off));
    double *ws = (double *)ctx->kn_ws.ptr;
    return jch_synced(ctx, host, [&]() -> int32_t {
        const double *dv = v;
        const int *di = ind;
        double *dout = out;
        if (host) {
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_v, v, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(ws + o_i, ind, sizeof(int) * mk, hipMemcpyHostToDevice, ctx->stream));
            dv = ws + o_v; di = (const int *)(ws + o_i); dout = ws + o_o;
        }
        hipLaunchKernelGGL(k_knn_gather_median, dim3((unsigned)nb), dim3(256), 0, ctx->stream, dv, n, di, (int)m, (int)k, cap, dout,
                           glob ? ws + o_gk : nullptr, glob ? (int *)(ws + o_gi) : nullptr);
        JCH_HIP(ctx, hipGetLastError());
        if (host) JCH_HIP(ctx, hipMemcpyAsync(out, dout, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    });
}
