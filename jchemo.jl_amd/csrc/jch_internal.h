// Internal declarations of libjchemo_hip.so (gfx950 only).  Public ABI: include/jchemo_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "jchemo_hip.h"

#define JCH_MAXQ 64       // largest q whose Jacobi workspace (q x q matrices) lives in LDS; beyond: global memory (smallstate.hip)
#define JCH_ZT_SLICES 8      // max second-stage partial slices of the sweep reduction
#define JCH_SWEEP_MAXP 2048  // widest row the register-resident fused sweep holds (16 column chunks of 128)

struct xcopy_key {
    const void *X; int64_t n, ldx; int p, host;
    bool operator==(const xcopy_key &o) const { return X == o.X && n == o.n && ldx == o.ldx && p == o.p && host == o.host; }
};
struct jch_buf {  // grow-only device buffer
    void *ptr = nullptr;
    size_t bytes = 0;
};

struct jch_uid {
    char internal[128];
};
struct jch_rccl {  // RCCL entry points, dlopen'ed on first use (single-GPU users never need RCCL)
    void *handle = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, jch_uid, int) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};

#define JCH_P2P_MAXR 16
struct jch_p2p {   // P2P inbox transport (p2p.hip)
    bool ready = false, tested = false;
    int nranks = 0, rank = 0;
    void *local = nullptr;                     // own inbox (fine-grained device memory)
    void *peer[JCH_P2P_MAXR] = {};             // every rank's inbox as mapped here
    bool opened[JCH_P2P_MAXR] = {};
    unsigned long long *host_status = nullptr, *host_status_dev = nullptr;   // pinned, device-visible sticky error word
    unsigned long long epoch = 0;
    long long timeout_ticks = 0;
    size_t cap = 0;                            // doubles per (parity, rank) slot
    unsigned long long *stats = nullptr;       // device [2 phases][4]: ticks in the exchange, ticks polling flags, calls, -
};

// The memory-side Infinity Cache of the MI355X (not a queryable attribute; the library runs on gfx950 only), and the slice of a
// working copy the plskern sweep keeps in it by default: the best point of the scan in DESIGN.md §4 (the cache also carries the
// T column, the weights and the small state between two sweeps).
constexpr int JCH_INFINITY_CACHE_MIB = 256;
constexpr int JCH_RESIDENT_DEFAULT_MIB = 128;
// Where the plskern sweeps stage the T column in LDS when JCH_SWEEP_TSTAGE is unset (k_sweep_v2 / k_sweep_bf16_v2): per kernel and
// shard size, wherever the A/B against the direct store met the bar of DESIGN.md §4 (sweeps of a fit down by more than 3 x the parent's
// run-to-run spread).  500-column Float64 rows from 3900 rows per CU on (1e6 rows on one MI355X: 14.21 -> 13.89 ms per 25 sweeps); 500 k
// rows and less showed nothing, the bf16 sweep gained 0.26 ms of 4.19 at 1e6 rows beside a parent spread of 0.14 ms: direct stores.
inline bool jch_sweep_tstage_default(int kc, int64_t n, int cus) { return kc == 4 && n >= (int64_t)3900 * cus; }
inline bool jch_sweep_bf16_tstage_default(int64_t n, int cus) { (void)n; (void)cus; return false; }

struct jch_ctx {
    int device = 0;
    int cus = 256;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // communicator
    void *comm = nullptr;
    int rank = 0, nranks = 1;
    void *loop = nullptr;            // loopback group (tests; ctx.hip)
    jch_p2p p2p;
    std::vector<double> loop_sum;
    // workspace (grow-only)
    void *hstage = nullptr;          // pinned host staging for the small outputs (grow-only)
    size_t hstage_bytes = 0;
    // the raw row-major working copy a plskern-shaped fit left in `xr` (JCH_REUSE_XCOPY): which X it is a copy of
    xcopy_key xcopy{};
    bool xcopy_valid = false;
    long long xcopy_reused = 0;   // fits that took their kernel matrix from it
    unsigned sweep_seq = 0;   // launches of the plskern-shaped sweep so far (JCH_SWEEP_ALT: alternating walk direction)
    int sweep_alt = 0;                 // JCH_SWEEP_ALT and JCH_SWEEP_FUSED_REDUCE=1 as read when the current fit started
    bool sweep_fused_reduce = false;
    int sweep_resident_mb = -1;        // JCH_SWEEP_RESIDENT_MB, read with them: MiB of the working copy the sweep keeps in the Infinity Cache (< 0: by shape)
    int sweep_tstage = -1;             // JCH_SWEEP_TSTAGE, read with them: row groups per wave of the T column's LDS ring (0: direct stores; < 0: by shape)
    jch_buf gram, xr, yr, xstage, ystage, wstage, tbuf, dnorm, part, kpart, small, colpart, gemm_b, gemm_out, xq, tickets, qz, lw_work, lw_xrm, lvws, lw_flags, lw_screen;
    jch_buf kg_ws, dk_x, dk_y, dk_k, dk_q, dk_o, dk_s;   // Gram kernel workspace (kgram.hip), dkplsr staging (dkplsr.hip)
    jch_buf kp_ws;   // kplsr panels and small state (kplsr.hip)
    jch_buf kc_vt, pc_ws, pc_vec;   // panel operand of the panel pass, the eigensolver's panels and small state, kpca's n-vectors (kpca.hip)
    jch_buf chol_inv, chol_a, chol_w, chol_s, kr_ws;   // inv(L_kk) blocks of the last factor, krr's working copy of Kd, the L^-T workspace of df, info / partial sums (chol.hip); krr staging (krr.hip)
    jch_buf rp_stage, rp_rows, rp_coef;   // row preprocessing (rowprep.hip): bounded row-block staging of host data, the row-block copy of the wide-window FIR, taps / A and V
    jch_buf cs_ws, cs_part;   // covsel (covsel.hip): [Yd | Q] and the small state of a selection; per-workgroup partials of the pass
    jch_buf xt_part, xt_ws;   // xtdx.hip: per-split partial tiles of the Gram pass; G, the vectors and the staging of a PCA fit
    jch_buf sel_ws, sel_out;   // colselect.hip: digit counters and per-column state of a chunk of columns; medians and MADs on their way to the host
    jch_buf st_t, st_ms;   // stah.hip: one panel of projections; [mu | s | d of a host call]
    jch_buf sp_ws;   // samp.hip: row flags, per-workgroup triples and the result of a farthest-pair search; running minima, partials and targets of a max-min selection
    jch_buf kn_ws;   // knn.hip: the search's lists ahead of the drop of `self`, the results of a host call, the sort buffers and class accumulators of shapes beyond the LDS
    jch_buf kd_ws;   // kde.hip: the bandwidth factors, class offsets and model dimensions of a call, the per-split partial sums, the staging of a host call
    jch_buf gd_ws;   // gda.hip: per entry, the vectors, one or two p x p matrices, the padded transposed factors and the staging of a host call
    jch_buf ms_ws;   // medspa.hip: the distances, two centres, the per-workgroup partial rows and sums of a Weiszfeld step, its scalar record; the staging of a host call
    jch_buf vp_ws;   // viperm.hip: B, the slice partials, the sums and the range flag of a permutation pass; the staging of a host call
    const void *chol_L = nullptr;   // the factor the blocks in chol_inv belong to (null: none); a solve against another one is JCH_EINVAL
    int64_t chol_n = 0, chol_ld = 0;
    // profiling
    bool profiling = false;
    int prof_stride = 1;        // jch_ctx_set_profiling(ctx, N > 1): event pairs around every N-th launch of the sampled dominant kernels only
    unsigned prof_seq = 0;
    int64_t sweeps_timed = 0;   // JCH_COUNTER_SWEEPS_TIMED
    jch_profile prof{};
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    size_t ev_mark = 0;
    // collective timing (profiling only): event pairs around the all-reduces that are calls of their own, tagged with the
    // phase of the fit (0 prologue, 1 LV loop); the fused inbox exchange is timed inside its kernel (p2p.stats)
    std::vector<hipEvent_t> cev_pool;
    std::vector<int> cev_phase;      // one entry per PAIR
    size_t cev_used = 0;             // events handed out (2 per pair)
    int coll_phase = 0;
    bool coll_in_fit = false;        // between jch_coll_reset (start of a fit) and jch_coll_collect
    int coll_transport = 0;          // JCH_TRANSPORT_* of the last LV-loop all-reduce
    // second stream + event (created on first use): result copies that may run beside the last kernel of a call (lwplsr.hip)
    hipStream_t aux_stream = nullptr;
    hipEvent_t aux_event = nullptr;
    // diagnostics
    long long pivot_refits = 0;      // raw-mode fits repeated on the centred copy because the sampled pivot was poor
    long long knn_screened = 0, knn_screen_redone = 0;   // kNN-LWPLSR queries done by the screened search / redone by the exact selection behind it
    long long locw_refits = 0;       // kNN-LWPLSR queries refitted by the per-query path after the neighbour-space kernel's pivot check
};

// One-time initialisation per (call site, device): hipFuncSetAttribute and occupancy queries are per device, and a
// process may hold ctxs on several GPUs.  The flag is raised AFTER the initialisation (two threads may both run it: benign).
struct jch_per_device_once {
    unsigned long long mask = 0;
    bool done(int dev) const { return (mask >> (dev & 63)) & 1ull; }
    void mark(int dev) { mask |= 1ull << (dev & 63); }
};

// Consecutive pieces of one workspace buffer, counted in doubles, each rounded up to 256 bytes: take() returns the offset of the next
// piece; `off` is the doubles taken so far (what to reserve).
struct jch_carve {
    size_t off = 0;
    size_t take(size_t count) { const size_t o = off; off += (count + 31) & ~(size_t)31; return o; }
};
inline size_t jch_ints_as_doubles(size_t count) { return (count + 1) / 2; }   // doubles that hold `count` ints: what an int array takes of a carve

// ---- error plumbing --------------------------------------------------------------------------------
int32_t jch_fail(jch_ctx *ctx, int32_t code, const char *fmt, ...);
#define JCH_HIP(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return jch_fail(ctx, e__ == hipErrorOutOfMemory ? JCH_ENOMEM : JCH_EHIP, "%s: %s (%s:%d)", #expr, \
                            hipGetErrorString(e__), __FILE__, __LINE__);                           \
    } while (0)
#define JCH_TRY(expr)                 \
    do {                              \
        int32_t s__ = (expr);         \
        if (s__ != JCH_OK) return s__; \
    } while (0)

// environment switches (ctx.hip: the only place of the library that reads the environment): presence, and integer value or dflt when unset
bool jch_knob_set(const char *name);
int jch_knob(const char *name, int dflt);

int32_t jch_reserve(jch_ctx *ctx, jch_buf &b, size_t bytes);
// The two buffers the JCH_REUSE_XCOPY state lives in are reserved through these two and nowhere else: `xstage` holds the staged X of
// a host-array fit (the reuse path takes the pivot from it and never uploads X again), `xr` the raw row-major copy itself.  Whoever
// takes either of them for something else thereby drops the copy; only the fit that is itself reusing it passes keep_copy.
inline int32_t jch_reserve_xstage(jch_ctx *ctx, size_t bytes, bool keep_copy = false) {
    if (!keep_copy && ctx->xcopy.host) ctx->xcopy_valid = false;   // (a device-resident X has no staging copy to lose)
    return jch_reserve(ctx, ctx->xstage, bytes);
}
inline int32_t jch_reserve_xr(jch_ctx *ctx, size_t bytes, bool keep_copy = false) {
    if (!keep_copy) ctx->xcopy_valid = false;
    return jch_reserve(ctx, ctx->xr, bytes);
}
int32_t jch_reserve_host(jch_ctx *ctx, size_t bytes);   // ctx->hstage (pinned)
int32_t jch_allreduce_f64(jch_ctx *ctx, double *dev_buf, size_t count);  // no-op when nranks == 1
// The communicator out of reach for a scope: a rank-local entry (include/jchemo_hip.h, "what an entry does on a joined ctx") that goes
// through code which is a collective on a joined ctx — the per-query jch_plskern_fit of the local models: the other ranks are fitting
// OTHER queries, or none — runs it as the one-rank code it is.  Everything jch_allreduce_f64, jch_allreduce_slices, the fits' shard
// logic and the inbox fusion of the small-state kernels look at is taken away and put back on every way out.
struct jch_comm_off {
    jch_ctx *ctx;
    void *comm, *loop;
    int nranks, rank;
    bool p2p_ready;
    explicit jch_comm_off(jch_ctx *c) : ctx(c), comm(c->comm), loop(c->loop), nranks(c->nranks), rank(c->rank), p2p_ready(c->p2p.ready)
    {
        c->comm = nullptr; c->loop = nullptr; c->nranks = 1; c->rank = 0; c->p2p.ready = false;
    }
    ~jch_comm_off()
    {
        ctx->comm = comm; ctx->loop = loop; ctx->nranks = nranks; ctx->rank = rank;
        ctx->p2p.ready = p2p_ready && !(ctx->p2p.host_status && *ctx->p2p.host_status != 0ull);   // (a timed-out inbox stays disabled: jch_p2p_check)
    }
    jch_comm_off(const jch_comm_off &) = delete;
    jch_comm_off &operator=(const jch_comm_off &) = delete;
};
// all-reduce of the per-LV sweep output zt [nslice][ldz] (first m entries of every slice); *nslice_out = slices the
// consumer has to add afterwards (1 when the transport summed them)
int32_t jch_allreduce_slices(jch_ctx *ctx, double *zt, int m, int nslice, int ldz, int *nslice_out);
// p2p.hip
int32_t jch_p2p_allreduce(jch_ctx *ctx, const double *src, size_t count, int nslice, int ldz, double *dst);
int32_t jch_p2p_check(jch_ctx *ctx);
void jch_p2p_destroy(jch_ctx *ctx);

// profiling helpers: record an event on the stream when profiling is on
struct jch_span {
    hipEvent_t a = nullptr, b = nullptr;
};
hipEvent_t jch_ev(jch_ctx *ctx);  // nullptr when profiling is off
bool jch_prof_sample(jch_ctx *ctx);   // profiling on and this launch of a sampled dominant kernel is one to bracket with events
void jch_coll_begin(jch_ctx *ctx);   // profiling: event in front of / behind an all-reduce call (ctx.hip)
void jch_coll_end(jch_ctx *ctx);
void jch_coll_reset(jch_ctx *ctx);   // start of a fit: forget the pairs, zero the inbox tick counters
void jch_coll_collect(jch_ctx *ctx, jch_profile &pr);   // after the fit's final sync: fill the collective fields

// sweep output as the per-block partial rows (the launcher skipped its k_reduce_part): part [nb][ldpart]
struct jch_part_view {
    const double *part = nullptr;
    int nb = 0, ldpart = 0;
};

// ---- kernel launchers (each enqueues on ctx->stream; no host sync) --------------------------------
// prologue.hip
int32_t jch_launch_weights(jch_ctx *ctx, const double *w_dev /*may be null*/, int64_t n, double *dnorm,
                           double *hdr /*[4] device: sum w, n_total*/, double *zero0 = nullptr, int nzero0 = 0,
                           double *zero1 = nullptr, int nzero1 = 0 /*two small regions zeroed by the same launch*/);
int32_t jch_launch_moments(jch_ctx *ctx, const double *Xc, int64_t ldx, const double *Yc, int64_t ldy,
                           const double *d, int64_t n, int p, int q, const double *means /*null: first moment*/,
                           double *out /*[p+q] device*/, bool do_sqrt = true);
int32_t jch_launch_center_xty(jch_ctx *ctx, double *Xc, int64_t ldx, double *Yc, int64_t ldy, const double *d,
                              int64_t n, int p, int q, const double *mom, const double *scl, bool writeback,
                              double *Xr, int ldr, double *Yr, int qpad, double *K /*[p][qpad] device*/, bool scal,
                              double *means_out = nullptr /*raw mode: X is copied minus the pivot mom[0..p), its weighted means land here*/,
                              double *mshift_out = nullptr /*means - pivot*/,
                              const double *spread2 = nullptr /*[p] sample variances from jch_launch_pivot*/,
                              double *qual = nullptr /*[1] max_j |means - pivot| / spread (atomicMax; zeroed by the caller)*/,
                              double *ones_out = nullptr /*raw mode: == mom's storage; [0, p + q) becomes 1.0 and means_out[p..p+q) = mom[p..p+q)*/);
int32_t jch_launch_pivot(jch_ctx *ctx, const double *Xc, int64_t ldx, int64_t n, int p, const double *hdr /*[1] = n_total*/,
                         double *pivot /*[p] device, same on all ranks*/, double *spread2 /*[p]*/);
int32_t jch_launch_export_colmajor(jch_ctx *ctx, const double *Xr, int ldr, const double *Yr, int qpad, int64_t n,
                                   int p, int q, double *Xc, int64_t ldx, double *Yc, int64_t ldy,
                                   const double *sqrt_rowscale = nullptr /*rows scaled by sqrt(d_i): plswold! row metric*/);
// sweep.hip
int32_t jch_launch_sweep(jch_ctx *ctx, const double *Xr, int64_t n, int p, int ldr, const double *d, const double *rvec,
                         const double *Yr, int qpad, int q_extra /*0: plskern; q: also c_raw (plsnipals)*/,
                         double *tcol, double *zt /*[nslice][ldz] device, reduced over blocks*/, int ldz, int max_slices,
                         int *nslice_out, const double *mu = nullptr /*raw mode: Xr is uncentred; t = x.r - mu.r, st at [ldr+1]*/,
                         jch_part_view *pv = nullptr /*non-null: the launcher MAY leave the block partials unreduced and describe them here (pv->part stays null when it reduced into zt as usual)*/);
int32_t jch_launch_reduce_rows(jch_ctx *ctx, const double *part, int nb, int ldpart, int m, double *out);
int32_t jch_launch_xty_rows(jch_ctx *ctx, const double *Xr, int ldr, const double *Yc, int64_t ldy, const double *d, int64_t n, int p, int q,
                            const double *mom, double *Yr, int qpad, double *K, double *means_out, double *mshift_out,
                            const double *spread2, double *qual, double *ones_out, bool *done);
int32_t jch_launch_raw_scales(jch_ctx *ctx, const double *Xr, int64_t n, int p, int ldr, const double *d, const double *mshift,
                              const double *Yr, int qpad, int q, double *tmp, double *scl, double *K);
int32_t jch_launch_reduce_part8(jch_ctx *ctx, const double *part, int nb, int ldpart, int m, double *zt, int ldz, int *nslice_out);
int32_t jch_launch_sweep_wide(jch_ctx *ctx, const double *Xr, int64_t n, int ldr, const double *d, const double *rvec,
                              const double *Yr, int qpad, bool nipals, double *tcol, double *zt);
int32_t jch_launch_ytdt(jch_ctx *ctx, const double *Yr, int64_t n, int qpad, const double *d, const double *tcol, double *out /*[qpad]*/);   // sweep_wide.hip
// plsnipals with postponed write-back (sweep.hip, deflate.hip): the working copy holds the rows of `npend` LVs ago; pending
// loadings pend_p[k][jch_nipals_lazy_pitch(ldr)] (pad columns zero), pending scores tpend + k * tstride, oldest first
#define JCH_NIPALS_DEFER_DEFAULT 6   // rows rewritten every 6th LV (cfg4, ms per LV: eager 8.5-8.9; m = 2: 6.6, 4: 5.76, 5-7: 5.3-5.55, 8-9: 5.45-5.5 — up to 4 pending corrections hide behind the loads, each further one costs ~0.17 ms per pass in LDS reads)
static inline int jch_nipals_lazy_pitch(int ldr) { return 128 * (ldr <= 128 ? 1 : ldr <= 256 ? 2 : ldr <= 512 ? 4 : ldr <= 1024 ? 8 : 16); }
int32_t jch_sweep_tickets(jch_ctx *ctx, int **out);   // sweep.hip: counters of the fused slice sums
int jch_nipals_lazy_capacity(int ldr, int q);   // 0: shape outside the lazy kernels' envelope
int32_t jch_launch_sweep_lazy(jch_ctx *ctx, const double *Xr, int64_t n, int ldr, const double *d, const double *wvec,
                              const double *Yr, int qpad, double *tcol, double *zt, int ldz, int max_slices, int *nslice_out,
                              const double *pend_p, int npend, int npend_max, const double *tpend, int64_t tstride);
// next K = X'DY from the rows with all `npend` corrections applied (the newest is this LV's; its Y step uses cvec); the rows
// are written back only when `flush`
int32_t jch_launch_kpass_lazy(jch_ctx *ctx, double *Xr, int64_t n, int p, int ldr, double *Yr, int qpad, int q, const double *d,
                              const double *pend_p, int npend, int npend_max, const double *tpend, int64_t tstride,
                              const double *cvec, bool flush, double *Knext);
int32_t jch_launch_deflate(jch_ctx *ctx, double *Xr, int64_t n, int p, int ldr, double *Yr, int qpad, int q,
                           const double *d, const double *tcol, const double *zpc /*[ldr + qpad]: zp then c*/,
                           double *Knext /*[p][qpad] or null*/);
// smallstate.hip
struct jch_small {  // device-resident replicated small state of one fit
    double *K;      // [p][qpad]
    double *w, *r;  // [ldr]
    double *P, *R, *W;  // [nlv][p]   (== Julia's p x nlv column-major)
    double *C;          // [nlv][q]
    double *TT;         // [nlv]
    double *Z;          // [nlv][q]   Z = P'K of the finished LVs (fast small-state path)
    double *zt;         // [JCH_ZT_SLICES][ldz]  reduced sweep output slices: zp, tt, (c_raw); ldz = ldr + 1 + qpad (+pad)
    double *zpc;        // [ldr + qpad]      plsnipals: zp/tt, c/tt
    double *mom, *scl;  // [p+q]
    double *mshift;     // [ldr] raw mode: means - pivot (the stored rows are x - pivot); null otherwise
    double *rs;         // [ldr] raw mode with scaling: r / xscales, the vector the sweep multiplies the unscaled rows with; null otherwise
    double *hdr;        // [4]
    int variant;        // 0: algorithm #1 (zt holds [zp, tt] from the sweep); 1: algorithm #2 (zt = G r, tt = r'zp computed here);
                        // 2: algorithm #1 in raw mode (uncentred row copy: zt holds [zp_raw, tt, st], zp = zp_raw - mom * st)
    double *dbg;        // [nlv + 1] diagnostics (JCH_LV_DEBUG): Jacobi sweeps per LV; may be null
    double *niter;      // [nlv] plswold: inner iterations per LV (src/plswold.jl:93); null otherwise
    double *kr;         // [16] split small-state path (smallstate_split.hip): K' r of the current LV; null otherwise
    double *gpart;      // [blocks][gld] split path: per-block partials of K_new'K_new, zp'K_new and P_i'K_new; null otherwise
    unsigned *lvctr;    // split path: arrival counter of the fit's blocks, non-null iff the fit runs the merged kernel (JCH_LV_MERGED=1, decided and zeroed in jch_lv_split_begin_fit)
};

int32_t jch_launch_lv_update(jch_ctx *ctx, const jch_small &s, int p, int q, int qpad, int ldr, int a /*-1: init*/,
                             int nlv, int algo /*0 plskern, 1 plsnipals*/, int nslice, int ldz, bool fast, bool fuse_p2p = false,
                             const double *bf_src = nullptr, int bf_ld = 0, int bf_ldr = 0, double tol = 0.0, int maxit = 0);
size_t jch_lv_fast_lds_bytes(int p, int q, int qpad, int ldr, int nlv);
int32_t jch_launch_lv_update_fast(jch_ctx *ctx, const jch_small &s, int p, int q, int qpad, int ldr, int a, int nlv, int algo,
                                  int do_a, int do_b, int nslice, int ldz, bool fuse_p2p = false, const double *bf_src = nullptr,
                                  int bf_ld = 0, int bf_ldr = 0);
// smallstate_split.hip: the per-LV step of the plskern-shaped loop as a p-parallel kernel + a single-workgroup kernel
int jch_lv_split_blocks(int p);
int jch_lv_split_gld(int nlv);
size_t jch_lv_split_doubles(int p, int nlv);
int32_t jch_lv_split_begin_fit(jch_ctx *ctx, jch_small &s, double *gbuf, int p, int nlv);
size_t jch_lv_solve_lds_bytes(int p, int q, int ldr, int nlv);
int32_t jch_launch_lv_split(jch_ctx *ctx, const jch_small &s, int p, int q, int ldr, int a, int nlv, const double *part, int nb,
                            int ldpart, int itt, int ist /*< 0: none*/, int mode /*0 centred copy, 1 f64 raw mode, 2 bf16*/, bool solve,
                            bool fuse_p2p = false /*the inbox all-reduce of the LOCAL partial rows inside the p-parallel kernel, block by block*/);
bool jch_lv_split_p2p_ok(const jch_ctx *ctx, int p);
struct p2p_dev;
void jch_p2p_next(jch_ctx *ctx, p2p_dev *out);   // p2p.hip: device view of the inbox transport for the next epoch
int32_t jch_launch_nipals_R(jch_ctx *ctx, const jch_small &s, int p, int nlv);
// siblings.hip (plssimp / plsrosa / plswold small-state kernels)
bool jch_sibling_supported(int p, int q, int ldr, int nlv);
int32_t jch_launch_lv_update_simp(jch_ctx *ctx, const jch_small &s, int p, int q, int ldr, int a /*-1: init*/, int nlv, int nslice, int ldz);
int32_t jch_launch_wold_b(jch_ctx *ctx, const jch_small &s, int p, int q, int ldr, int a, int nlv, double tol, int maxit);
int32_t jch_launch_rosa_orthw(jch_ctx *ctx, double *W, int p, int nlv);
int32_t jch_launch_ydeflate_all(jch_ctx *ctx, double *Yc, int64_t ldy, const double *T, int64_t n, const double *C, int q, int nlv);
// gemm.hip
int32_t jch_launch_affine_gemm(jch_ctx *ctx, const double *Xc, int64_t m, int p, int64_t ldx, const double *Bs /*[p][kpad] scaled*/,
                               int k, int kpad, const double *bias /*[kpad]*/, double *out, int64_t ldo);
int32_t jch_launch_weighted_ss(jch_ctx *ctx, const double *Xc, int64_t n, int p, int64_t ldx, const double *d,
                               const double *shift, const double *iscale, double *out1);
// bf16.hip
int32_t jch_fit_plskern_bf16(jch_ctx *ctx, const jch_pls_desc &d, const void *Xv, int64_t ldx, const void *Yv, int64_t ldy,
                             const double *wdev, double *dn, double *Tdev, jch_small &s, int ldr_small, int qpad, int ldz,
                             bool fast, int *nlv_out);
// kern2.hip (opt-in kernel algorithm #2)
int32_t jch_launch_syrk(jch_ctx *ctx, const double *Xr, int64_t n, int p, int ldr, const double *d, double *G, int ldg);
int32_t jch_launch_gmatvec(jch_ctx *ctx, const double *G, int ldg, int p, int ldr, const double *r, double *out);
int32_t jch_launch_scores(jch_ctx *ctx, const double *Xr, int64_t n, int p, int ldr, const double *Rm, int nlv, double *T);
// kgram.hip: K (m x n, ld ldk) = kern(Z diag(1/zdiv), X diag(1/xdiv)); zdiv / xdiv HOST p-vectors or null; sym: Z == X (same
// pointer, ld and divisors), only the tiles on or below the diagonal are computed and each is stored twice
int32_t jch_launch_kgram(jch_ctx *ctx, int kind, const double *Z, int64_t m, int64_t ldz, const double *zdiv, const double *X, int64_t n,
                         int64_t ldx, const double *xdiv, int64_t p, double gamma, double coef0, int degree, bool sym, double *K, int64_t ldk);
// kgram.hip: the preparation of the symmetric krbf Gram on its own (samp.hip): cp (ldc x pp, ldc and pp the padded sizes of jch_launch_kgram) = the
// zero-padded copy of X - 1 c' (c: device p-vector, given), nrm (ldc) = the squared norms of its rows
int32_t jch_launch_kgram_prep(jch_ctx *ctx, const double *X, int64_t n, int64_t ldx, int64_t p, const double *c, double *cp, int64_t ldc, int64_t pp, double *nrm);
// kplsr.hip: K = kern(X, X) into Kraw, vtot = K w, *sdev = w'vtot, Kc = K - vtot 1' - 1 vtot' + *sdev (Kc == Kraw allowed)
int32_t jch_launch_kp_centred_gram(jch_ctx *ctx, int kind, double gamma, double coef0, int degree, const double *X, int64_t n, int64_t ldx,
                                   const double *xdiv, int64_t p, const double *wn, double *Kraw, double *Kc, double *vt, double *sdev);
// kpca.hip: out (n x b, ld ldo) = Kc (diag(d) V) on the f64 matrix cores (d: device n-vector or null); any b, chunks of 64 columns
int32_t jch_launch_kc_panel(jch_ctx *ctx, const double *Kc, int64_t n, int64_t ldk, const double *V, int64_t ldv, int b, const double *d,
                            double *out, int64_t ldo);
// kpca.hip: the nlv leading eigenpairs (by |.|) of the symmetric device matrix A (dim x dim, ld lda) -- of diag(sqrtw) A diag(sqrtw) when sqrtw (a
// device dim-vector) is given -- by block subspace iteration with Rayleigh-Ritz, block b = min(dim, roundup16(nlv + oversample)); 1 <= nlv <= dim.
// Stops when the residuals |A x_e - theta_e x_e| of the first nlv pairs are all <= tol |theta_0|, or after maxit iterations.  The device pointers
// point into ctx->pc_ws and hold until the next call; the call ends synchronised with ctx->stream up to the sign kernels it enqueued last.
struct jch_eig_lead_out {
    int b = 0, niter = 0;
    bool converged = false;
    std::vector<double> theta, resid;   // host: the b Ritz values ordered by |.| descending; the residual norms of the first nlv pairs
    double *X = nullptr;                // dim x b (ld dim): Ritz vectors, the first nlv signed so that their largest-|.| entry (first index on ties) is positive
    double *AX = nullptr;               // dim x b: A (sqrtw o X), signed alike
    const double *theta_dev = nullptr;  // the Ritz values on the device
    double *scratch = nullptr;          // dim x b the caller may use (the last iterate)
};
int32_t jch_eig_lead(jch_ctx *ctx, const double *A, int64_t dim, int64_t lda, const double *sqrtw, int nlv, double tol, int maxit, jch_eig_lead_out *out);
// xtdx.hip: G (p x p, ld ldg) = (X - 1 mu')' diag(d) (X - 1 mu'), everything on the device; X n x p column-major (ld ldx), read only.  Both
// triangles are written from the same value; fixed-order sums, no atomics.
int32_t jch_launch_xtdx(jch_ctx *ctx, const double *X, int64_t n, int p, int64_t ldx, const double *mu, const double *d, double *G, int64_t ldg);
// colselect.hip: exact medians (and, mad non-null, MADs) of the p columns of the device matrix X (n x p, ld ldx) into the device vectors med and mad.
// jch_colselect_reserve(ctx, p) first: the launcher itself reserves nothing and only enqueues.
int32_t jch_colselect_reserve(jch_ctx *ctx, int64_t p);
int32_t jch_launch_col_median_mad(jch_ctx *ctx, const double *X, int64_t n, int64_t p, int64_t ldx, double *med, double *mad);
// medspa.hip: d[i] = |(x_i - c) / s| (c, s device p-vectors, s may be null: no division), the distances-only mode of the Weiszfeld pass: one read of X,
// enqueued only, no workspace.  jch_spatial_median_dev: the whole loop of `colmedspa` on a device X into the device vector mu_dev (d_dev: the distances
// to the last centre the loop stepped from, or null); reserves ctx->ms_ws and the selection's workspace, synchronises once per step.
int32_t jch_launch_weiszfeld_dist(jch_ctx *ctx, const double *X, int64_t n, int p, int64_t ldx, const double *c, const double *sdiv, double *d);
int32_t jch_spatial_median_dev(jch_ctx *ctx, const double *X, int64_t n, int p, int64_t ldx, double delta, int maxit, double *mu_dev, double *d_dev, int32_t *niter,
                               double *h_last, int32_t *converged);
// kmethod.hip: what the kernel-method entry points (dkplsr.hip, kplsr.hip, kpca.hip, krr.hip) share
int32_t jch_check_kernel(jch_ctx *ctx, const char *who, int32_t kind, int32_t degree);   // kernel kind / degree, one rank only
int32_t jch_launch_divcols(jch_ctx *ctx, double *A, int64_t lda, int64_t n, int64_t cols, const double *s_dev);   // A[:, k] /= s[k]
int32_t jch_launch_sqrt(jch_ctx *ctx, const double *w, int64_t n, double *sw);                                    // sw = sqrt(w)
// rows of new data per Gram block of a transform / predict over n training rows: knob (the caller's JCH_*_QBLOCK) when >= 1, else 1 GiB of Gram
int64_t jch_qblock(int knob, int64_t n);
// Transform / predict over m new rows X against the n training rows Xt, in blocks of at most qblock rows.  jch_kblocks_begin: the
// argument checks (ptrs_ok: every pointer the entry point needs is set), then *mb = rows per block (0: m == 0, nothing to do).
// jch_kblocks_run: per block, Kb (rows x n, ld rows, device) = kern(X_block / xscale, Xt), then step(Kb, rows, out_block, ld_out) fills the
// block's rows x ncols of the output on the device; host data is staged in and out; ends with a stream sync.
typedef std::function<int32_t(double *Kb, int64_t rows, double *out_block, int64_t ld_out)> jch_kblock_step;
int32_t jch_kblocks_begin(jch_ctx *ctx, const char *who, int32_t loc, int32_t kind, int32_t degree, bool ptrs_ok, int64_t m, int64_t n, int64_t p,
                          int64_t ldx, int64_t ldxt, int64_t ldo, int qblock_knob, int64_t *mb);
int32_t jch_kblocks_run(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X, int64_t m, int64_t p,
                        int64_t ldx, const double *xscale, const double *Xt, int64_t n, int64_t ldxt, int64_t mb, int64_t ncols, double *out,
                        int64_t ldo, const jch_kblock_step &step);
// chol.hip: blocked Cholesky of the lower triangle of A (n x n, ld lda, in place), everything on ctx->stream, no host sync.  info_dev: a device
// int that ends up 0 or the 1-based index of the first pivot that is not > 0.  The solves and jch_launch_chol_inv_fro2 need the factor the
// last jch_launch_chol_factor produced (its inv(L_kk) blocks live in ctx->chol_inv).  jch_launch_chol_inv_t writes W = L^-T (upper triangle,
// exact zeros below the diagonal) into the caller's n x n device buffer (ld ldw >= n; rows >= n of a column are not touched);
// jch_launch_chol_inv_fro2 is that into ctx->chol_w followed by the sum of squares.
int32_t jch_launch_chol_factor(jch_ctx *ctx, double *A, int64_t n, int64_t lda, int *info_dev);
int32_t jch_launch_chol_solve(jch_ctx *ctx, const double *L, int64_t n, int64_t ldl, double *B, int64_t q, int64_t ldb, const int *info_dev);
int32_t jch_launch_chol_inv_t(jch_ctx *ctx, const double *L, int64_t n, int64_t ldl, double *W, int64_t ldw, const int *info_dev);
int32_t jch_launch_chol_inv_fro2(jch_ctx *ctx, const double *L, int64_t n, int64_t ldl, double *out_dev, const int *info_dev);
int32_t jch_chol_info_word(jch_ctx *ctx, int **info_dev);   // the ctx's own device info word
// util.hip
unsigned jch_grid1(const jch_ctx *ctx, int64_t work);   // workgroups of 256 threads of a grid-stride element-wise launch
// The only strided matrix copy of the library: column-major rows x cols from src (ld lds) to dst (ld ldd) on ctx->stream; one
// contiguous copy when both pitches equal rows.
int32_t jch_copy2d(jch_ctx *ctx, double *dst, int64_t ldd, const double *src, int64_t lds, int64_t rows, int64_t cols, hipMemcpyKind kind);
// A matrix operand (rows x cols) of an entry with a `loc`: a host call uploads *src (ld *ld) into dst (ld rows) and leaves *src = dst,
// *ld = rows; a device call leaves both as they are.  Vectors and index lists stay plain hipMemcpyAsync lines.
int32_t jch_stage_in(jch_ctx *ctx, bool host, double *dst, int64_t rows, int64_t cols, const double **src, int64_t *ld);
// The frame of a host-array call.  Such a call queues asynchronous copies on the caller's pageable arrays and on its own local host
// images, and none of that memory may be released before the stream has drained, on the failure paths too.  So: between the first copy
// queued on host memory and this synchronisation, nothing returns except through the frame.  Runs body(); with `sync`, synchronises
// ctx->stream whatever body returned; returns body's failure if there was one, else the synchronisation's status.  sync == false (device
// in, device out: enqueued only) returns body's status unchanged.
template <class F> int32_t jch_synced(jch_ctx *ctx, bool sync, F &&body)
{
    const int32_t st = body();
    if (!sync) return st;
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (st != JCH_OK) return st;
    JCH_HIP(ctx, es);
    return JCH_OK;
}
// The same frame around a body that ends synchronised on every success path of its own (fit_impl, lw_run): the success path does exactly
// the stream operations of the body; the stream is drained here only when body failed (and `sync`: host memory may have copies queued).
template <class F> int32_t jch_synced_on_failure(jch_ctx *ctx, bool sync, F &&body)
{
    const int32_t st = body();
    if (st != JCH_OK && sync) (void)hipStreamSynchronize(ctx->stream);
    return st;
}
int32_t jch_launch_fill(jch_ctx *ctx, double *out, int64_t n, int64_t p, int64_t ld, int64_t row0, int64_t n_total,
                        uint64_t seed);

// ---- device helpers ---------------------------------------------------------------------------------
#ifdef __HIPCC__
__device__ __forceinline__ double jch_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// Sum over a block of NT threads (NT multiple of 64, <= 1024); result valid in every thread.
// scratch: >= NT/64 doubles of LDS.  Deterministic (fixed tree).
template <int NT>
__device__ __forceinline__ double jch_block_sum(double v, double *scratch)
{
    v = jch_wave_sum(v);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) scratch[wv] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) s += scratch[i];
    return s;
}
#endif
