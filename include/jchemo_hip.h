/*
 * jchemo_hip.h — C ABI of libjchemo_hip.so: the MI355X (gfx950) PLS regression engine behind
 * Jchemo.jl's plskern / plsnipals hot path.
 *
 * The reference (/root/reference, Jchemo.jl v0.1.23) has NO FFI boundary: its "operator API" is the
 * Julia call shape  fun(X, Y[, weights]; nlv, scal=false) -> ::Plsr  plus the generics
 * transform / coef / predict / summary.  Each entry point below names the reference lines it
 * replaces; INTEGRATION.md shows the Julia `ccall` stubs (and the ctypes stubs used by the tests).
 *
 * Conventions
 *   - every function returns an int32 status: 0 = OK, <0 = error (codes below); the message is
 *     available from jch_last_error().  Nothing throws or aborts across the boundary.
 *   - matrices are COLUMN-MAJOR float64 exactly as Julia stores them (element (i,j) at
 *     base[i + j*ld]); `ld` is in elements.
 *   - the caller owns every buffer it passes; the library keeps no host pointer after return and
 *     owns only device workspace inside the ctx (re-used across calls).
 *   - a ctx is bound to ONE GPU and one HIP stream and is not thread-safe.  All calls are blocking
 *     (they return after the ctx stream has drained).
 *   - multi-GPU = one process (one ctx) per GPU, rows of X/Y/weights/T sharded by rows; the ctx is
 *     joined to an RCCL communicator with jch_ctx_comm_init and every rank makes the same call with
 *     its own shard.  All p x q-and-smaller results are replicated (bit-identical) on every rank.
 */
#ifndef JCHEMO_HIP_H
#define JCHEMO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JCH_VERSION 108 /* 0.1.8 (jch_covsel_fit, like the krr and row preprocessing entries, joined without a new number): jch_ctx_set_profiling(ctx, N > 1) samples the sweeps, JCH_COUNTER_SWEEPS_TIMED; 0.1.7: JCH_REUSE_XCOPY, JCH_COUNTER_XCOPY_REUSED; 0.1.6: + jch_score_sums_lv, jch_predict over an nlv range as running sums over the scores; 0.1.5: screened kNN (JCH_COUNTER_KNN_SCREENED / _REDONE); 0.1.4: no shape limits (generic lwplsr / small-state paths), JCH_NIPALS_ONE_PASS, JCH_COUNTER_LOCW_REFITS; 0.1.3: + jch_lwplsr_add_query_map (0.1.2: collective fields of jch_profile, jch_ctx_allreduce_probe, jch_lwplsr_prepare / _release) */

#if defined(JCH_BUILD)
#define JCH_API __attribute__((visibility("default")))
#else
#define JCH_API
#endif

/* status codes */
#define JCH_OK 0
#define JCH_EINVAL (-1) /* bad argument / unsupported shape */
#define JCH_EHIP (-2)   /* HIP runtime error (message has the HIP string) */
#define JCH_ERCCL (-3)  /* RCCL error or RCCL not loadable */
#define JCH_ENOMEM (-4) /* device or host allocation failed */
#define JCH_ENODEV (-5) /* no usable gfx950 device */

/* where the n-sized arrays (X, Y, weights, T, weights_norm) of a call live */
#define JCH_LOC_HOST 0   /* host pointers: the library stages them through the device */
#define JCH_LOC_DEVICE 1 /* device pointers on the ctx's GPU (e.g. an AMDGPU.jl ROCArray / torch tensor) */

/* storage type of X / Y handed to a fit */
#define JCH_F64 0
#define JCH_BF16 1 /* bf16 storage (BASELINE config 3); device-resident only.  jch_plskern_fit (p <= 2048): bf16-resident kernels, fp32 row
                      arithmetic, fp64 small state; every other fit: the inputs are widened exactly to Float64 on the device and the
                      Float64 path runs (same contract — the Float64 algorithm on the bf16-rounded inputs —, no bandwidth saving) */

typedef struct jch_ctx jch_ctx; /* opaque: device, stream, RCCL communicator, workspace pool */

JCH_API int32_t jch_version(void);

/* Create a context on HIP device `device_id`.  `stream` is a hipStream_t to launch on (e.g.
 * torch.cuda.current_stream().cuda_stream) or NULL to let the ctx create its own. */
JCH_API int32_t jch_ctx_create(jch_ctx **out, int32_t device_id, void *stream, uint32_t flags);
JCH_API int32_t jch_ctx_destroy(jch_ctx *ctx);
/* Message of the last failing call on ctx (ctx == NULL: last jch_ctx_create failure).  Valid until
 * the next call on the same ctx. */
JCH_API const char *jch_last_error(const jch_ctx *ctx);

/* ---- row-sharded multi-GPU (RCCL over xGMI) ------------------------------------
 * Rank 0 fills a 128-byte id with jch_comm_unique_id, the host side broadcasts it (the Python mirror
 * uses torch.distributed, the Julia wrapper MPI/Distributed), every rank calls jch_ctx_comm_init. */
JCH_API int32_t jch_comm_unique_id(void *uid128);
JCH_API int32_t jch_ctx_comm_init(jch_ctx *ctx, const void *uid128, int32_t rank, int32_t nranks);
JCH_API int32_t jch_ctx_comm_info(const jch_ctx *ctx, int32_t *rank, int32_t *nranks);

/* ---- P2P inbox transport for the latency-bound all-reduces (the per-LV [zp, tt] message is 4 KB) -----------------
 * Each rank owns an inbox in fine-grained device memory; the other ranks' processes map it through a HIP IPC handle
 * and store their contribution + an epoch flag straight into it over xGMI; one single-workgroup kernel per rank and
 * all-reduce, sums in rank order (bit-identical on every rank), bounded waits (a lost peer yields JCH_ERCCL, never a
 * hang).  Set-up, driven by the host side that already exchanged the RCCL id:
 *   1. every rank: jch_ctx_p2p_export(ctx, nranks, handle64)             -> 64-byte IPC handle of its inbox
 *   2. all-gather the handles (torch.distributed / MPI), every rank: jch_ctx_p2p_import(ctx, handles, rank, nranks, 0)
 *      — maps the peers and runs a collective self-test; returns JCH_ERCCL on the ranks where it failed
 *   3. agree (min over ranks of "import succeeded") and call jch_ctx_p2p_enable(ctx, 1) everywhere, or leave it off:
 *      RCCL (jch_ctx_comm_init) remains the transport for large messages and the fallback.
 * `flags` is reserved (0).  nranks <= 16. */
JCH_API int32_t jch_ctx_p2p_export(jch_ctx *ctx, int32_t nranks, void *handle64);
JCH_API int32_t jch_ctx_p2p_import(jch_ctx *ctx, const void *handles, int32_t rank, int32_t nranks, uint32_t flags);
JCH_API int32_t jch_ctx_p2p_enable(jch_ctx *ctx, int32_t on);

/* Loopback communicator — TEST HARNESS for the row-sharded path on a one-GPU box (RCCL refuses two ranks on one device):
 * the "ranks" are host threads of ONE process, each with its own ctx on the same GPU; all-reduces are staged through
 * host memory in rank order (bit-identical sums on every rank, like the RCCL path).  Every rank thread must make the
 * same sequence of library calls.  Not a production transport. */
JCH_API int32_t jch_loopback_group_create(int32_t nranks, void **group_out);
JCH_API int32_t jch_loopback_group_destroy(void *group);
JCH_API int32_t jch_ctx_comm_init_loopback(jch_ctx *ctx, void *group, int32_t rank);

/* ---- joined ctx contract: what every entry does on a ctx that was joined to a communicator of N > 1 ranks -----------------------
 * (jch_ctx_comm_init, jch_ctx_p2p_import, jch_ctx_comm_init_loopback).  Every exported entry is in exactly one class; the lists below
 * are read by tests/test_joined_ctx_static.py (a new export cannot arrive unclassified) and held by tests/test_gpu_joined_ctx.py.
 *
 * Class C -- collective.  Every rank makes the same call, with the same shapes but for the row count, on its own rows.  Outputs with one
 *   entry per row (T, weights_norm) are per shard; everything else is replicated bit-identically on every rank and equals the result on
 *   the concatenated rows up to the summation order.  A rank that does not call leaves the others waiting.
 *   C: jch_plskern_fit jch_plsnipals_fit jch_plssimp_fit jch_plsrosa_fit jch_plswold_fit jch_plskern_fit_scaled
 *   C: jch_col_stats jch_weighted_ss jch_weighted_cov jch_score_sums jch_score_sums_lv jch_ctx_allreduce_probe
 *
 * Class L -- rank-local.  The ranks are replicas or hold independent rows; the call enters no collective, may be made by any subset of the
 *   ranks with any shapes, and returns exactly the bytes the same call returns on a ctx without a communicator.  This is what the replica
 *   scheme of kNN-LWPLSR needs (the global model fitted row-sharded, the queries split over the ranks, every rank holding
 *   all of Xtrain): the per-query jch_plskern_fit / jch_predict / jch_transform of the generic paths run with the communicator out of
 *   reach (csrc/jch_internal.h jch_comm_off) and the ctx is handed back joined.
 *   L: jch_affine_gemm jch_transform jch_predict jch_rows_standardize jch_rows_project_out jch_rows_fir
 *   L: jch_row_resid_ss jch_row_resid_ss_lv jch_fill_uniform jch_chol_factor jch_chol_solve jch_chol_inv_fro2 jch_kc_panel jch_covsel_pass
 *   L: jch_lwplsr_predict jch_lwplsr_prepare jch_lwplsr_predict_prepared jch_lwplsr_release jch_lwplsr_add_query_map
 *   L: jch_knn_prepare jch_knn_release jch_knn_search jch_knn_wmean jch_knn_vote jch_knn_gather_median jch_knn_wls jch_knn_gda
 *   L: jch_lwplsda_predict_prepared jch_lwplsravg_predict_prepared jch_kde_dens
 *
 * Class R -- refused.  The algorithm needs every row at once (a median, a Gram matrix, a selection over all rows) and has no replica
 *   use: the call returns JCH_EINVAL with "one rank only (communicator of N)" in jch_last_error before any device work, writes no output
 *   and enters no collective.  The argument checks that come first are those of the unjoined call.
 *   R: jch_kernel_gram jch_dkplsr_fit jch_dkplsr_transform jch_dkplsr_predict jch_kplsr_fit jch_kplsr_transform jch_kplsr_predict
 *   R: jch_kpca_fit jch_krr_fit jch_krr_solve jch_covsel_fit jch_xtdx jch_pca_fit jch_pcasph_fit jch_col_median_mad jch_stah
 *   R: jch_weiszfeld_step jch_spatial_median jch_farthest_pair jch_maxmin_select jch_class_cov jch_gauss_factor jch_mahsq_chol
 *   R: jch_perm_fill jch_perm_score_sums
 *
 * Class M -- ctx, communicator, p2p, profiling and counter management: what joins, inspects and frees a ctx.  Not covered by the above.
 *   M: jch_version jch_ctx_create jch_ctx_destroy jch_last_error jch_comm_unique_id jch_ctx_comm_init jch_ctx_comm_info
 *   M: jch_ctx_p2p_export jch_ctx_p2p_import jch_ctx_p2p_enable jch_loopback_group_create jch_loopback_group_destroy
 *   M: jch_ctx_comm_init_loopback jch_ctx_set_profiling jch_ctx_get_profile jch_ctx_synchronize jch_ctx_get_counter
 * ---- end of the joined ctx contract */

typedef struct jch_pls_desc {
    int64_t n;       /* rows held by THIS rank (all rows when single-GPU) */
    int64_t p;       /* columns of X */
    int64_t q;       /* columns of Y (>= 1; q <= 16 runs the LDS-resident small-state kernels, larger q a generic one) */
    int32_t nlv;     /* requested LVs; clamped to min(n_total, p, nlv) like plskern.jl:116 */
    int32_t scal;    /* 0/1: scale columns by their weighted uncorrected std (plskern.jl:123-126) */
    int32_t dtype;   /* JCH_F64 | JCH_BF16 */
    int32_t loc;     /* JCH_LOC_HOST | JCH_LOC_DEVICE for X, Y, weights, T, weights_norm */
    int32_t inplace; /* 1 = `plskern!` / `plsnipals!` semantics: X and Y are overwritten with their
                        centred/scaled (plsnipals: and deflated) versions; 0 = `plskern` (inputs untouched,
                        the reference's copy at plskern.jl:108 never materialises) */
    int32_t reserved; /* option bits.  0 = the reference's algorithm (improved kernel #1, one sweep over X per LV);
                         bit 0 (1) = OPT-IN kernel algorithm #2 (X'DX once, no pass over X and no collective in the LV
                         loop; plskern, q <= 16, p <= 2048): same results up to rounding;
                         JCH_WOLD_REF_ZERO_WEIGHT_NAN (jch_plswold_fit only): see below;
                         JCH_NIPALS_ONE_PASS (jch_plsnipals_fit / jch_plswold_fit): see below;
                         JCH_REUSE_XCOPY (any fit): X is unchanged since the previous fit on this ctx, see below */
} jch_pls_desc;
/* jch_plswold_fit: give the rows with weight 0 NaN scores, as the reference does (src/plswold.jl:107 divides by sqrt(w) = 0).
 * Default (bit clear): finite scores t_i = x_i' r for those rows — what a cross-validation fold with zero weights on its
 * held-out rows needs (gridcvlv). */
#define JCH_WOLD_REF_ZERO_WEIGHT_NAN 2
/* jch_plsnipals_fit / jch_plswold_fit, OPT-IN (never the default: it is not what the reference computes, src/plsnipals.jl:71 recomputes
 * X'DY from the deflated matrices every LV): ONE pass over X per LV.  The next kernel matrix follows from the exact identity
 * K_{a+1} = (X - t p')'D(Y - t c') = K_a - zp_raw c_raw' / tt (t is D-orthogonal to its own residuals), c_raw = Y'Dt is taken
 * against the UNdeflated Y (equal for the same reason), and the second read of X per LV disappears; the deflated rows are still
 * written back every few LVs (the postponed write-back needs q <= 16, p <= 2048, inplace = 0, Float64: JCH_EINVAL otherwise).
 * Same results up to rounding (gate of the tests: 1e-9 against the default path on well-conditioned LVs). */
#define JCH_NIPALS_ONE_PASS 4
/* Any fit: the caller PROMISES that X (pointer, shape, leading dimension and contents) is what the previous fit on this ctx was
 * given — the folds of a cross-validation (`gridcvlv`, src/gridcv.jl:200-208: the same X with other rows held out), the combinations
 * of a parameter grid.  A Float64 plskern-shaped fit whose predecessor left its row-major working copy in the workspace then skips
 * the staging of X (host arrays) and the transposing copy, and takes X'D[Yc | 1] from one streaming read of that copy (q <= 11,
 * p <= 512; same results up to the summation order of X'DY).  In every other situation the bit is ignored.  Y and the weights may
 * change freely; if X changed, the results are those of the OLD X.
 * The promise is about X only, never about the ctx: a result does not depend on what ran on the ctx before.  Any call in between
 * that touched the staging buffer or the working copy (another fit, a prediction, a kernel method, a preprocessing call, ...) makes
 * the library ignore the bit and run the whole prologue, with correct results. */
#define JCH_REUSE_XCOPY 8

/*
 * jch_plskern_fit — replaces `plskern!` / `plskern` (src/plskern.jl:106-178): weight normalisation
 * (utility.jl:715-723), weighted column means / stds (utility.jl:195,264,314-323), centring/scaling
 * (utility.jl:76-81,482-487), XtY = X'DY (plskern.jl:131-132) and the per-LV loop (plskern.jl:149-175).
 *   X  n x p (ldx >= n), Y  n x q (ldy >= n), weights n or NULL (= ones)          [desc->loc]
 *   T  n x nlv (ld n), weights_norm n                                              [desc->loc]
 *   P, R, W  p x nlv (ld p); C  q x nlv (ld q); TT nlv; xmeans, xscales p; ymeans, yscales q   [HOST]
 *   nlv_out: the clamped number of LVs actually computed (columns filled in T/P/R/W/C/TT).
 * Any output pointer may be NULL to skip it.  Sign of each LV (w, r, t, P, C columns flip together,
 * SURVEY F3) is fixed by: the largest-|.| component of the dominant right singular vector is positive.
 */
JCH_API int32_t jch_plskern_fit(jch_ctx *ctx, const jch_pls_desc *desc, void *X, int64_t ldx, void *Y, int64_t ldy,
                        const double *weights, double *T, double *P, double *R, double *W, double *C,
                        double *TT, double *xmeans, double *xscales, double *ymeans, double *yscales,
                        double *weights_norm, int32_t *nlv_out);

/* jch_plsnipals_fit — replaces `plsnipals!` / `plsnipals` (src/plsnipals.jl:31-97); same signature.
 * With inplace = 1, X and Y return centred AND deflated (plsnipals.jl:86-87). */
JCH_API int32_t jch_plsnipals_fit(jch_ctx *ctx, const jch_pls_desc *desc, void *X, int64_t ldx, void *Y, int64_t ldy,
                          const double *weights, double *T, double *P, double *R, double *W, double *C,
                          double *TT, double *xmeans, double *xscales, double *ymeans, double *yscales,
                          double *weights_norm, int32_t *nlv_out);

/* jch_plskern_fit_scaled — jch_plskern_fit with CALLER-SUPPLIED column divisors instead of `scal`: X is centred by its
 * weighted means and divided by xscales_in (p, HOST), Y by yscales_in (q, HOST; NULL = ones); desc->scal is ignored and
 * the divisors are echoed in xscales / yscales.  This is what multiblock PLSR needs (src/mbplsr.jl:77-113: per-block
 * column scales times one scalar per block, then plskern with scal = false on the concatenated blocks).  Float64. */
JCH_API int32_t jch_plskern_fit_scaled(jch_ctx *ctx, const jch_pls_desc *desc, void *X, int64_t ldx, void *Y, int64_t ldy,
                        const double *weights, const double *xscales_in, const double *yscales_in, double *T, double *P,
                        double *R, double *W, double *C, double *TT, double *xmeans, double *xscales, double *ymeans,
                        double *yscales, double *weights_norm, int32_t *nlv_out);

/* jch_col_stats — weighted column means and (stds != NULL) uncorrected standard deviations: `colmean`, `colstd`
 * (src/utility.jl:193-195,312-323) on their own.  X n x p [loc], weights n or NULL [loc]; means, stds (p) HOST.
 * Collective on a joined ctx (the prologue kernels of the fits: the weight sum and the moments are all-reduced): every rank calls with its
 * own rows and weights and gets the statistics of the concatenated rows, the same bits on every rank. */
JCH_API int32_t jch_col_stats(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *weights,
                      double *means, double *stds);

/* ---- sibling algorithms: same row kernels, different small state --------------------------------
 * jch_plssimp_fit — `plssimp!` / `plssimp` (src/plssimp.jl:22-88, SIMPLS with un-normed scores); W is returned equal to R
 *   (src/plssimp.jl:85-87).  One fused sweep over X per LV, like plskern.
 * jch_plsrosa_fit — `plsrosa!` / `plsrosa` (src/plsrosa.jl:26-96): X never deflated, Y deflated (inplace = 1 hands back
 *   the centred X and the deflated Y, :87), W re-orthonormalised (:77-79), R = W inv(P'W) (:94).  One fused sweep per LV:
 *   the score orthogonalisation of :75-76 is applied to the weight vector before the sweep (t = X r), which is the same
 *   vector in exact arithmetic.
 * jch_plswold_fit — `plswold!` / `plswold` (src/plswold.jl:30-111): NIPALS with the inner power iteration; `tol` and
 *   `maxit` as the reference's keywords (defaults sqrt(eps), 200); niter (nlv, HOST, as Float64 like :71) receives the
 *   number of inner passes per LV.  The reference seeds each LV's first convergence check with `rand(p)` (:78), which
 *   can never pass; that check is skipped here.  Rows with zero weight get finite scores by default (the reference divides
 *   by sqrt(w) = 0 at :107 and returns NaN for them; desc->reserved |= JCH_WOLD_REF_ZERO_WEIGHT_NAN reproduces that).
 *   inplace = 1 hands back X, Y deflated AND carrying the row metric sqrt(w) (:57-58).
 * plssimp / plswold run their LDS-resident small-state kernels when q <= 16, p <= 2048 and the p x q state fits in LDS,
 * and a generic kernel (state in global memory; any p, q and nlv — for q > 64 its q x q eigen-solver matrices live in
 * global memory too) otherwise; Float64 only. */
JCH_API int32_t jch_plssimp_fit(jch_ctx *ctx, const jch_pls_desc *desc, void *X, int64_t ldx, void *Y, int64_t ldy,
                        const double *weights, double *T, double *P, double *R, double *W, double *C,
                        double *TT, double *xmeans, double *xscales, double *ymeans, double *yscales,
                        double *weights_norm, int32_t *nlv_out);
JCH_API int32_t jch_plsrosa_fit(jch_ctx *ctx, const jch_pls_desc *desc, void *X, int64_t ldx, void *Y, int64_t ldy,
                        const double *weights, double *T, double *P, double *R, double *W, double *C,
                        double *TT, double *xmeans, double *xscales, double *ymeans, double *yscales,
                        double *weights_norm, int32_t *nlv_out);
JCH_API int32_t jch_plswold_fit(jch_ctx *ctx, const jch_pls_desc *desc, void *X, int64_t ldx, void *Y, int64_t ldy,
                        const double *weights, double tol, int32_t maxit, double *T, double *P, double *R, double *W,
                        double *C, double *TT, double *xmeans, double *xscales, double *ymeans, double *yscales,
                        double *weights_norm, double *niter, int32_t *nlv_out);

/*
 * jch_affine_gemm — out (m x k, ld ldo) = ((X - 1*shift') * diag(1/scale)) * B + 1*bias'
 * the single device primitive behind `transform` (src/plskern.jl:187-195: shift = xmeans, scale =
 * xscales, B = R[:,1:k], bias = 0) and `predict` (src/plskern.jl:226-238 via coef :207-217:
 * shift = 0, scale = 1, B = [B_k0 | B_k1 | ...], bias = [int_k0 | ...]; one pass over X for the whole
 * nlv range instead of one GEMM per value).
 *   X m x p (ldx) and out [loc]; shift, scale (p, may be NULL), B (p x k, ld p), bias (k, may be NULL) HOST.
 */
JCH_API int32_t jch_affine_gemm(jch_ctx *ctx, int32_t loc, const double *X, int64_t m, int64_t p, int64_t ldx,
                        const double *shift, const double *scale, const double *B, int64_t k,
                        const double *bias, double *out, int64_t ldo);

/* jch_transform — `transform(object::Plsr, X; nlv)` (src/plskern.jl:187-195): T (m x nlv, ld ldt) [loc] =
 * cscale(X, xmeans, xscales) * R[:, 1:nlv].  X m x p [loc]; xmeans, xscales (p), R (p x >= nlv, ld p) HOST. */
JCH_API int32_t jch_transform(jch_ctx *ctx, int32_t loc, const double *X, int64_t m, int64_t p, int64_t ldx,
                      const double *xmeans, const double *xscales, const double *R, int32_t nlv, double *T, int64_t ldt);

/* jch_predict — `predict(object::Plsr, X; nlv)` (src/plskern.jl:226-238 through coef, :207-217) for every nlv in
 * [nlv_lo, nlv_hi] (0 = intercept only) in ONE pass over X: pred (m x q*(nlv_hi-nlv_lo+1), ld ldo) [loc]; block b =
 * columns b*q .. b*q+q-1 = prediction with nlv_lo + b LVs.  Model pieces (xmeans, xscales p; ymeans, yscales q;
 * R p x nlv_fit ld p; C q x nlv_fit ld q) HOST, nlv_hi <= nlv_fit is the caller's responsibility (the reference
 * clamps at :228).  One or two levels: one GEMM with the levels' coefficient matrices side by side.  Three or more on a long input
 * (m >= 4096): the scores X_c R once (m x nlv_hi), then the blocks as running sums over the score columns,
 * pred_a = pred_{a-1} + t_a (c_a .* yscales)' — X_c B_a = T_a C_a' — written in one streaming pass (cfg2 size, nlv = 0..25: 1.15 ms). */
JCH_API int32_t jch_predict(jch_ctx *ctx, int32_t loc, const double *X, int64_t m, int64_t p, int64_t ldx, const double *xmeans,
                    const double *xscales, const double *ymeans, const double *yscales, const double *R, const double *C,
                    int64_t q, int32_t nlv_lo, int32_t nlv_hi, double *pred, int64_t ldo);

/* jch_weighted_ss — sum_i d_i * || (x_i - shift) / scale ||^2 : the `sstot` of `summary`
 * (src/plskern.jl:250-251).  X n x p and d (n) [loc]; shift/scale HOST; result HOST.  With a
 * communicator the result is the sum over all ranks' shards. */
JCH_API int32_t jch_weighted_ss(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx,
                        const double *d, const double *shift, const double *scale, double *sstot);

/*
 * jch_lwplsr_predict — the prediction path of kNN-LWPLSR, batched over the m queries: replaces getknn
 * (src/getknn.jl:29-57), the wdist weight loop (src/lwplsr.jl:152-159, src/wdist.jl:64-75) and locwlv
 * (src/locwlv.jl:9-48, `Threads.@threads` over queries: one weighted plskern + 1-row predict per query).
 *   Xtrain n x p, Ytrain n x q, Xq m x p                                   [loc], column-major
 *   Ztrain n x dd, Zq m x dd: the space the neighbours are searched in (global PLS scores, already whitened by
 *     the host side for metric = "mahal": scores * inv(chol(cov).U), src/getknn.jl:37-49)      [loc]
 *   k neighbours (clamped to n), h / tol: weight shape and floor; scal; nlv range nlv_lo..nlv_hi (contiguous)
 *   pred  m x le x q (le = nlv_hi - nlv_lo + 1), query-major: pred[(i*le + a)*q + y]              [HOST]
 *   ind_out (m x k, 0-based, row-major), dist_out, w_out (m x k): optional                       [HOST]
 * No shape limits (the reference has none: src/getknn.jl:29-57, src/locwlv.jl:9-48).  Inside the batched kernels' envelope —
 * k <= 768 for the kNN scan; p <= 2048, q <= 16, nlv <= 48 and 150 KB of LDS for the local fits — one launch serves all m
 * queries: for k <= 208, q <= 8 and wide rows the fit runs in NEIGHBOUR space (the k x k Gram matrix of the gathered rows, built
 * on the matrix cores in one pass and held in registers: lwplsr_kspace.hip; same T, C and predictions up to rounding), otherwise
 * one workgroup per query sweeps the k x p slab once per LV.  Outside it the generic paths of lwplsr_generic.hip run: an exact
 * per-query selection of the k smallest distances (radix select + sort in global memory, the same distance expression: the
 * same neighbours, order and distance bits), and one jch_plskern_fit + jch_predict per query on the gathered rows — the
 * reference's own schedule (src/locwlv.jl:18-39); slower, never absent.
 * The constant-y shortcut of src/locwlv.jl:25-28 applies to q == 1 only, as in the reference.
 * Neighbours at equal distance are ordered by their row index.
 * Rank-local on a joined ctx (class L of the joined ctx contract; so are the prepared forms and the discrimination and averaging entries
 * built on them): the per-query fits of the generic path are one rank's own and never meet another rank's.
 */
JCH_API int32_t jch_lwplsr_predict(jch_ctx *ctx, int32_t loc, const double *Xtrain, int64_t n, int64_t p, int64_t ldx,
                                   const double *Ytrain, int64_t q, int64_t ldy, const double *Ztrain, int64_t ldzt,
                                   const double *Zq, int64_t ldzq, int64_t dd, const double *Xq, int64_t m, int64_t ldxq,
                                   int32_t k, double h, double tol, int32_t scal, int32_t nlv_lo, int32_t nlv_hi,
                                   double *pred, int32_t *ind_out, double *dist_out, double *w_out);

/* ---- persistent model state of kNN-LWPLSR: the reference's `Lwplsr` object (src/lwplsr.jl:1-12) is fitted once
 * (`lwplsr`, :114-131) and predicted from many times (`predict`, :134-166).  jch_lwplsr_prepare keeps the model-constant
 * device data — the row-major copy of Xtrain the neighbour gathers read, Ytrain, the (whitened) training scores Ztrain — in
 * a handle; jch_lwplsr_predict_prepared is jch_lwplsr_predict without those three arguments and without their per-call
 * copies; jch_lwplsr_release frees the handle.  The handle belongs to the ctx's device; the inputs of prepare are not
 * referenced after it returns.  Same paths and errors as jch_lwplsr_predict. */
typedef struct jch_lwplsr_model jch_lwplsr_model;
JCH_API int32_t jch_lwplsr_prepare(jch_ctx *ctx, int32_t loc, const double *Xtrain, int64_t n, int64_t p, int64_t ldx,
                                   const double *Ytrain, int64_t q, int64_t ldy, const double *Ztrain, int64_t ldzt, int64_t dd,
                                   jch_lwplsr_model **model_out);
JCH_API int32_t jch_lwplsr_predict_prepared(jch_ctx *ctx, const jch_lwplsr_model *model, int32_t loc, const double *Zq, int64_t ldzq,
                                            const double *Xq, int64_t m, int64_t ldxq, int32_t k, double h, double tol, int32_t scal,
                                            int32_t nlv_lo, int32_t nlv_hi, double *pred, int32_t *ind_out, double *dist_out,
                                            double *w_out);
JCH_API int32_t jch_lwplsr_release(jch_ctx *ctx, jch_lwplsr_model *model);
/* The map that takes a query block to the neighbour-search space — the reference's `transform(object.fm, X)`
 * (src/lwplsr.jl:139-151) followed by getknn's whitening (src/getknn.jl:37-49) — as a chain of affine stages
 * Z <- ((Z - shift) ./ scale) B + bias (the arithmetic of jch_affine_gemm; shift, scale, bias may be NULL; B is p_in x k_out,
 * column-major, all on the HOST), kept on the device with the model.  Stage 1 takes the model's p columns, every later stage
 * the previous one's k_out, the last one must deliver dd columns; at most 4 stages.  With a map in place
 * jch_lwplsr_predict_prepared accepts Zq = NULL and computes the query scores itself: same numbers as two jch_affine_gemm
 * calls, without their uploads and synchronisations. */
JCH_API int32_t jch_lwplsr_add_query_map(jch_ctx *ctx, jch_lwplsr_model *model, const double *shift, const double *scale,
                                         const double *B, int64_t p_in, int64_t k_out, const double *bias);

/* jch_weighted_cov — S = (A - 1 mu')' D (A - 1 mu') (d x d), D = diag(weights / sum); weights NULL = ones:
 * `Statistics.cov(Xtrain, corrected = false)` of getknn's Mahalanobis branch (src/getknn.jl:38; with nlvdis = 0 the
 * reference whitens the raw X, src/lwplsr.jl:21: d = p).  d <= 64: the X'DY kernels of the fit with Y = A; wider: the centred
 * row-major copy + the tiled MFMA SYRK of the opt-in algorithm #2.  A n x d [loc]; S (column-major d x d) and mu (d, may be
 * NULL) HOST.  Collective on a joined ctx, on both paths (weight sum, means and the d x d sums are all-reduced): every rank calls with
 * its own rows and gets S and mu of the concatenated rows, the same bits on every rank. */
JCH_API int32_t jch_weighted_cov(jch_ctx *ctx, int32_t loc, const double *A, int64_t n, int64_t d, int64_t lda,
                                 const double *weights, double *S, double *mu);

/* jch_score_sums — sufficient statistics of prediction scores over the rows selected by `mask` (NULL = all rows), per
 * prediction column c = level * q + k:  sums[c*6 + 0..5] = { sum e, sum e^2, sum y e, sum y, sum y^2, row count },
 * e = y - pred.  msep / rmsep / ssr / bias / r2 / cor2 (src/scores.jl:25-32,54-62,155-158,190-196,268,426-429) follow on
 * the host; this is what gridscorelv / gridcvlv (src/gridscore.jl:167-221, src/gridcv.jl:187-228) evaluate per nlv.
 *   Pred m x ncol (ncol multiple of q), Y m x q, mask m [loc]; sums ncol x 6 HOST. */
JCH_API int32_t jch_score_sums(jch_ctx *ctx, int32_t loc, const double *Pred, int64_t m, int64_t ncol, int64_t ldp,
                               const double *Y, int64_t q, int64_t ldy, const double *mask, double *sums);

/* jch_score_sums_lv — the statistics of jch_score_sums for the predictions with nlv = nlv_lo..nlv_hi latent variables, straight
 * from the rows' scores: pred_a = ymeans + sum_{l <= a} t_l (c_l .* yscales)' (src/plskern.jl:207-217, 226-238 applied to
 * `transform(object, X)`), accumulated level by level in registers — the m x (levels q) prediction matrix that gridscorelv /
 * gridcvlv (src/gridscore.jl:196-216, src/gridcv.jl:206-224) would score never exists.  Levels beyond kfit repeat level kfit (the
 * reference clamps, src/plskern.jl:228).
 *   T m x kfit (scores of the rows, ld ldt), Y m x q, mask m (may be NULL) [loc]; C q x kfit (ld q), ymeans, yscales (q; NULL = 0 / 1)
 *   HOST; sums (nlv_hi - nlv_lo + 1) q x 6 HOST, laid out like jch_score_sums on the level-major prediction matrix. */
JCH_API int32_t jch_score_sums_lv(jch_ctx *ctx, int32_t loc, const double *T, int64_t m, int64_t kfit, int64_t ldt, const double *C,
                                  const double *ymeans, const double *yscales, const double *Y, int64_t q, int64_t ldy, const double *mask,
                                  int32_t nlv_lo, int32_t nlv_hi, double *sums);

/* ---- permutation importance: what the reference's `viperm` evaluates per replication (src/viperm.jl:89-107) -- DESIGN.md §26.  Both entries
 * serve one rank only (a communicator of more ranks: JCH_EINVAL), Float64 only, and end synchronised with the ctx stream.
 * jch_perm_fill -- perm (m x ncols int32, column-major, ld ldperm >= m, [loc]): column j = pi_j(0 .. m - 1), the permutation of 0 .. m - 1 for
 *   (seed, j).  Counter-based: pi_j(i) is a function of (seed, j, m, i) alone.  1 <= m < 2^31; m = 1 gives 0.  With all arithmetic modulo 2^64,
 *     mix64(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31)   (the splitmix64 finaliser
 *       of jch_fill_uniform); G = 0x9E3779B97F4A7C15; key_j = mix64(seed + (j + 1) G);
 *     b = the smallest even number >= 2 with 2^b >= m, h = b / 2; rounds = 24 when b <= 12, else 8;
 *     one walk of v < 2^b: L = v >> h, R = v & (2^h - 1); for r = 1 .. rounds: (L, R) <- (R, L ^ (mix64((key_j + r G) ^ R) >> (64 - h)));
 *       v <- (L << h) | R;
 *     pi_j(i) = the first of walk(i), walk(walk(i)), ... that is < m (cycle walking: a balanced Feistel network is a permutation of [0, 2^b)).
 * jch_perm_score_sums -- for a model that predicts as int + X B: the six sums of jch_score_sums for the p predictions in which ONE column of the
 *   held-out block was shuffled, from one read of the held-out rows of X and the unshuffled predictions.  With r = rows (m entries, int64,
 *   0-based, [loc]; NULL = the rows 0 .. m - 1, m <= n) and pi_j = column j of perm (m x p int32, ld ldperm, [loc]; NULL = generated from `seed`
 *   exactly as jch_perm_fill would), for j < p:
 *       e[i, k] = y[r_i, k] - (pred[r_i, k] + (x[r_pi_j(i), j] - x[r_i, j]) * B[j, k]),
 *   sums[(j q + k) 6 + 0..5] = { sum e, sum e^2, sum y e, sum y, sum y^2, m } over i < m; row j = p holds the unshuffled sums (the difference taken
 *   as 0), from the same code in the same summation order: a column whose row of B is zero gives that row's bits, and an importance of exactly 0.
 *   X n x p (ld ldx), Pred and Y n x q (ld ldp, ldy; indexed by the same row numbers as X) [loc], read only; B p x q (ld ldb) HOST, in the
 *   units of the raw X (`coef(fm).B`); sums (p + 1) x q x 6 HOST.  Any n, m, p, q >= 1 (m < 2^31, (p + 1) q <= 2^27).  Rows not listed are
 *   never read.  The residual is formed per element; fixed-order sums, no floating-point atomics: the same call gives the same bits, and so do a
 *   host and a device X, an aligned and an unaligned X, and an explicit perm equal to the generated one.  No guards beyond IEEE: a non-finite
 *   value in column j makes the sums of row j non-finite and touches no other row.  An entry of rows outside 0 .. n - 1 or of perm outside
 *   0 .. m - 1 is JCH_EINVAL: host lists are checked before any device work, device lists inside the pass (the index is not followed, `sums` is
 *   left untouched).  That a column of perm IS a permutation is the caller's promise.  loc JCH_LOC_DEVICE: the call enqueues on the ctx stream
 *   and synchronises once, for the download of the sums.  The workspace is the ctx's own (the X copy a fit left for JCH_REUSE_XCOPY is not
 *   touched). */
JCH_API int32_t jch_perm_fill(jch_ctx *ctx, int32_t loc, int32_t *perm, int64_t m, int64_t ncols, int64_t ldperm, uint64_t seed);
JCH_API int32_t jch_perm_score_sums(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const int64_t *rows, int64_t m,
                                    const double *Pred, int64_t ldp, const double *Y, int64_t q, int64_t ldy, const double *B, int64_t ldb,
                                    const int32_t *perm, int64_t ldperm, uint64_t seed, double *sums);

/* ---- direct kernel PLS (src/dkplsr.jl:1-163): plskern on a Gram matrix built on the device -------------------------------
 * Kernel kinds: JCH_KERN_RBF = `krbf(X, Y; gamma)` = exp(-gamma * euclsq(X, Y)) (src/kernels.jl:26-30, euclsq src/distances.jl:24-28:
 * expanded norms clamped at 0; here on rows shifted by the column means of the second argument, which leaves the distances unchanged
 * and removes the cancellation of the expansion); JCH_KERN_POL = `kpol(X, Y; degree, gamma, coef0)` = (gamma X Y' + coef0) raised to
 * `degree` by degree - 1 successive multiplications (src/kernels.jl:59-70).  Float64 only; one GPU (a ctx with a communicator of
 * more than one rank gets JCH_EINVAL). */
#define JCH_KERN_RBF 0
#define JCH_KERN_POL 1

/* jch_kernel_gram — `krbf` / `kpol` on their own: K (m x n, ld ldk >= m) [loc] = kern(Z diag(1/zscale), X diag(1/xscale)).
 *   Z m x p (ldz), X n x p (ldx) [loc]; zscale, xscale (p) HOST or NULL (= ones).  The train Gram (Z == X, same ld, m == n and the
 *   same scales) computes only the tiles on or below the diagonal and stores each twice: K is bitwise symmetric and krbf's diagonal
 *   is exactly 1.  Dot products on the f64 matrix cores; all indices 64-bit. */
JCH_API int32_t jch_kernel_gram(jch_ctx *ctx, int32_t loc, int32_t kind, const double *Z, int64_t m, int64_t ldz, const double *zscale,
                                const double *X, int64_t n, int64_t ldx, const double *xscale, int64_t p, double gamma, double coef0,
                                int32_t degree, double *K, int64_t ldk);

/* jch_dkplsr_fit — `dkplsr!` / `dkplsr` (src/dkplsr.jl:102-123): with desc->scal, dk_xscales = colstd(X, weights) and dk_yscales =
 * colstd(Y, weights) (:113-116; the weights enter nowhere else), X and Y divided by them (:117-118); K = kern(X, X) (:121); then
 * `plskern!(K, Y; nlv)` (:122) — the jch_plskern_fit path on the device, in place, WITHOUT weights (the reference passes none).
 *   desc: n, p (columns of X), q, nlv, scal, loc, inplace (1 = `dkplsr!`: X returns scaled, Y scaled and centred, as plskern! leaves
 *   it); dtype must be JCH_F64.  X n x p, Y n x q, weights n or NULL [loc].
 *   Outputs of the inner fit exactly as jch_plskern_fit's with p replaced by n: T n x nlv, weights_norm n [loc]; P, R, W n x nlv,
 *   C q x nlv, TT, xmeans, xscales (n), ymeans, yscales (q) HOST.  dk_xscales (p), dk_yscales (q) HOST: the outer scales (ones
 *   unless scal).  K_out: a DEVICE n x n buffer (ld n) that receives the centred Gram the reference leaves in Dkplsr.K, or NULL (ctx
 *   workspace). */
JCH_API int32_t jch_dkplsr_fit(jch_ctx *ctx, const jch_pls_desc *desc, int32_t kind, double gamma, double coef0, int32_t degree,
                               void *X, int64_t ldx, void *Y, int64_t ldy, const double *weights, double *K_out, double *T, double *P,
                               double *R, double *W, double *C, double *TT, double *xmeans, double *xscales, double *ymeans,
                               double *yscales, double *weights_norm, double *dk_xscales, double *dk_yscales, int32_t *nlv_out);

/* jch_dkplsr_transform — `transform(object::Dkplsr, X; nlv)` (src/dkplsr.jl:133-137) = jch_transform on kern(scale(X, xscale),
 * Xtrain).  jch_dkplsr_predict — `predict(object::Dkplsr, X; nlv)` (:158-163) = jch_predict on the same Gram, every block times
 * Diagonal(dk_yscales) (NULL = ones).  X m x p (ldx), Xtrain n x p (ldxt, the model's X: already scaled), T / pred [loc]; xscale (p,
 * the divisors of the NEW rows only; NULL = ones) and the inner model's pieces (xmeans, xscales n; R n x nlv; ymeans, yscales q;
 * C q x nlv) HOST.  The new rows are processed in blocks so that the m x n Gram workspace stays bounded: 1 GiB per block by default,
 * JCH_DKPLSR_QBLOCK=<rows> in the environment (read at call time) sets the block; the results do not depend on it. */
JCH_API int32_t jch_dkplsr_transform(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X,
                                     int64_t m, int64_t p, int64_t ldx, const double *xscale, const double *Xtrain, int64_t n,
                                     int64_t ldxt, const double *xmeans, const double *xscales, const double *R, int32_t nlv, double *T,
                                     int64_t ldt);
JCH_API int32_t jch_dkplsr_predict(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X,
                                   int64_t m, int64_t p, int64_t ldx, const double *xscale, const double *Xtrain, int64_t n, int64_t ldxt,
                                   const double *xmeans, const double *xscales, const double *ymeans, const double *yscales,
                                   const double *R, const double *C, int64_t q, int32_t nlv_lo, int32_t nlv_hi, const double *dk_yscales,
                                   double *pred, int64_t ldo);

/* ---- kernel NIPALS PLS (src/kplsr.jl:1-250, Rosipal & Trejo 2001) on a Gram matrix built on the device ----------------------
 * jch_kplsr_fit — `kplsr!` / `kplsr` (src/kplsr.jl:119-193): w = mweight(weights) (:124); ymeans = colmean(Y, w); with desc->scal
 * xscales = colstd(X, w) and yscales = colstd(Y, w), X DIVIDED only and Y centred and scaled, else Y centred (:125-135);
 * K = kern(X, X) (:137); Kc = K - vtot 1' - 1 vtot' + w'Kw with vtot = K w (:138-142); the NIPALS LV loop (:157-188) with tol and
 * maxit (q > 1 only; iter[a] = 0 when q == 1); R = DU inv(T' D Kc DU) (:189-190).  The deflation K .= z*K*z' (:182-183) is
 * postponed: every LV reads Kc once against an n x q panel projected with the previous LVs' z_i.
 *   desc: n, p (columns of X), q (<= 1024), nlv, scal, loc, inplace (1 = `kplsr!`: X returns scaled when scal, Y centred / scaled
 *   AND deflated, as the reference leaves it); dtype must be JCH_F64.  X n x p, Y n x q, weights n or NULL [loc].
 *   nlv is clamped to n (the reference does not clamp: it allocates n x nlv and runs every LV); *nlv_out = min(n, nlv).
 *   Outputs: T, U, R n x nlv (ld n), vtot n, weights_norm n [loc]; C q x nlv, xscales p, ymeans q, yscales q, iter nlv HOST; any may be
 *   NULL.  K_out: a DEVICE n x n buffer (ld n) that receives the UNcentred Gram (the reference's Kplsr.Kt), or NULL.  The centred
 *   Gram lives in ctx workspace (n^2 doubles); a Gram that does not fit returns JCH_ENOMEM.  Float64 only; one GPU. */
JCH_API int32_t jch_kplsr_fit(jch_ctx *ctx, const jch_pls_desc *desc, int32_t kind, double gamma, double coef0, int32_t degree, double tol,
                              int32_t maxit, void *X, int64_t ldx, void *Y, int64_t ldy, const double *weights, double *K_out, double *T,
                              double *U, double *R, double *vtot, double *C, double *xscales, double *ymeans, double *yscales,
                              double *weights_norm, int32_t *iter, int32_t *nlv_out);

/* jch_kplsr_transform — `transform(object::Kplsr, X; nlv)` (src/kplsr.jl:202-212): Knew = kern(scale(X, xscales), Xtrain),
 * Kc_new = Knew - vnew 1' - 1 vtot' + weights . vtot with vnew = Knew weights, T = Kc_new R[:, 1:nlv].  jch_kplsr_predict —
 * `predict(object::Kplsr, X; nlv)` (:238-250 through coef :221-228) for every nlv in [nlv_lo, nlv_hi], laid out as jch_predict's:
 * ymeans + Kc_new R[:, 1:a] C[:, 1:a]' diag(yscales).  X m x p (ldx), Xtrain n x p (ldxt, the model's X: already scaled), T / pred
 * [loc]; xscales (p, NULL = ones), weights (the normalised weights, n), vtot (n), R (n x nlv, ld n), ymeans, yscales (q), C (q x nlv)
 * HOST.  The new rows are processed in Gram blocks of 1 GiB by default; JCH_KPLSR_QBLOCK=<rows> in the environment (read at call
 * time) sets the block; the results do not depend on it. */
JCH_API int32_t jch_kplsr_transform(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X,
                                    int64_t m, int64_t p, int64_t ldx, const double *xscales, const double *Xtrain, int64_t n, int64_t ldxt,
                                    const double *weights, const double *vtot, const double *R, int32_t nlv, double *T, int64_t ldt);
JCH_API int32_t jch_kplsr_predict(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, const double *X,
                                  int64_t m, int64_t p, int64_t ldx, const double *xscales, const double *Xtrain, int64_t n, int64_t ldxt,
                                  const double *weights, const double *vtot, const double *ymeans, const double *yscales, const double *R,
                                  const double *C, int64_t q, int32_t nlv_lo, int32_t nlv_hi, double *pred, int64_t ldo);

/* ---- kernel PCA (src/kpca.jl:1-147) on a Gram matrix built on the device ---------------------------------------------------
 * jch_kpca_fit — `kpca(X, weights; nlv, kern, scal, kwargs...)` (src/kpca.jl:82-115): w = mweight(weights) (:93); with scal
 * xscales = colstd(X, w) and X DIVIDED by them in place (:94-98; X is not centred); K = kern(X, X), vtot = K w,
 * Kc = K - vtot' - vtot + w'vtot (:99-103); the leading nlv eigenpairs of Kd = sqrtD Kc sqrtD, ordered by |lambda| (the singular
 * triplets of svd(Kd), :104-108), from block subspace iteration with Rayleigh-Ritz on the device (one read of Kc per iteration,
 * DESIGN.md §12); eig = |lambda|, sv = sqrt(eig) (:109-110), P = sqrtD U diag(1/sv) (:113), T = Kc P (:114).  Sign rule: the
 * largest-|.| entry of every U column is positive.  An eigenvalue that is exactly 0 gives Inf / NaN in P, as in the reference.
 *   X n x p (ldx), weights n or NULL [loc]; kind / gamma / coef0 / degree as jch_kernel_gram.  nlv is clamped to n (:100);
 *   *nlv_out = min(n, nlv).  tol > 0, maxit >= 1: the iteration stops when every one of the first nlv residual norms
 *   |Kd u_i - lambda_i u_i| is <= tol * eig[0], or after maxit iterations; it never fails for lack of convergence.
 *   Outputs: T, P n x nlv (ld n), vtot n, weights_norm n [loc]; xscales p (ones without scal), sv, eig, resid nlv, sstot 1,
 *   niter 1 HOST; any may be NULL.  sv / eig hold the nlv leading values only (the reference keeps all n).  The fit converged iff
 *   every resid[i] <= tol * eig[0].  sstot = sum of all n singular values of Kd (summary's denominator, :138-147): computed as
 *   trace(Kd) = sum_i w_i Kc_ii for the kernels that are PSD by construction (krbf with gamma >= 0; kpol with gamma >= 0 and
 *   degree == 1 or coef0 >= 0); NaN for any other parameter set.  K_out: a DEVICE n x n buffer (ld n) that receives the
 *   UNcentred Gram (the reference's Kpca.Kt), or NULL.  The centred Gram lives in ctx workspace (n^2 doubles); a Gram that does
 *   not fit returns JCH_ENOMEM.  Float64 only; one GPU (a communicator of more than one rank: JCH_EINVAL).
 *   `transform(object::Kpca, X; nlv)` (:123-129) is jch_kplsr_transform with R = P (the model's X, weights_norm, vtot and xscales).
 *   The block size is min(n, roundup16(nlv + 7)); JCH_KPCA_OVERSAMPLE=<k> in the environment replaces the 7 (measurement only). */
JCH_API int32_t jch_kpca_fit(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, double *X, int64_t n, int64_t p,
                             int64_t ldx, const double *weights, int32_t nlv, int32_t scal, double tol, int32_t maxit, double *K_out, double *T,
                             double *P, double *vtot, double *weights_norm, double *xscales, double *sv, double *eig, double *sstot,
                             int32_t *niter, double *resid, int32_t *nlv_out);

/* ---- kernel ridge regression (src/krr.jl:1-202, LS-SVM) by a device Cholesky of the Gram -------------------------------------
 * The reference takes svd(Kd) of Kd = sqrtD Kc sqrtD (src/krr.jl:152) and keeps U (n x n), UtDY and sv.  Its outputs do not need
 * them: coef(lb).A = U diag(1 / (eig + lb^2)) U' sqrtD Y = (Kd + lb^2 I)^-1 sqrtD Y (:170-172) and coef(lb).df = 1 + sum eig /
 * (eig + lb^2) = 1 + n - lb^2 trace((Kd + lb^2 I)^-1) (:175-176).  Kd + lb^2 I is symmetric positive definite for a PSD kernel
 * and lb > 0, so the fit keeps Kd and every lb is one blocked Cholesky factorisation on the f64 matrix cores.
 * Deviation: there are no U, UtDY and sv outputs.
 *
 * jch_krr_fit — `krr!` / `krr` (src/krr.jl:128-159) up to the SVD: w = mweight(weights) (:135); with scal xscales = colstd(X, w) and
 * X DIVIDED by them in place (:136-140; X is not centred, Y is not touched); ymeans = colmean(Y, w) (:141); K = kern(X, X) (:143),
 * vtot = K w (:145-146), Kc = K - vtot' - vtot + w'vtot (:147) by the launches of jch_kplsr_fit / jch_kpca_fit (same bits);
 * Kd = sqrtD Kc sqrtD (:150-151); B = sqrtD Y (Y raw, as `U' * sqrtD * Y` :156).
 *   X n x p (ldx), Y n x q (ldy), weights n or NULL [loc]; kind / gamma / coef0 / degree as jch_kernel_gram.
 *   Outputs: Kd a caller-owned DEVICE n x n buffer (ld n; required); K_out a DEVICE n x n buffer that receives the UNcentred Gram
 *   (the reference's Krr.K), or NULL; B n x q (ld n), vtot n, weights_norm n [loc]; xscales p (ones without scal), ymeans q HOST;
 *   any of the last five may be NULL.  Float64 only; one GPU (a communicator of more than one rank: JCH_EINVAL). */
JCH_API int32_t jch_krr_fit(jch_ctx *ctx, int32_t loc, int32_t kind, double gamma, double coef0, int32_t degree, double *X, int64_t n, int64_t p,
                            int64_t ldx, const double *Y, int64_t q, int64_t ldy, const double *weights, int32_t scal, double *Kd, double *K_out,
                            double *B, double *vtot, double *weights_norm, double *xscales, double *ymeans);

/* jch_krr_solve — `coef(object::Krr; lb)` (src/krr.jl:168-177): a copy of Kd in ctx workspace gets lb^2 added to its diagonal, is
 * factored (jch_chol_factor's kernels) and A = (Kd + lb^2 I)^-1 B is solved for (:170-172); alpha = sqrtD A is what `predict`
 * multiplies the centred Gram of the new rows with (:198): `predict(object::Krr, X; lb)` (:187-202) is jch_kplsr_transform with
 * R = the alphas of all requested lb side by side (n x (q le_lb)), plus ymeans.  With want_df, df = 1 + n - lb^2 |L^-1|_F^2
 * (:175-176; jch_chol_inv_fro2's kernels, one more n x n workspace: JCH_ENOMEM with a message that names df when it cannot be had).
 *   Kd DEVICE n x n (ld n, from jch_krr_fit; not modified); B n x q (ld n), weights_norm n [loc]; lb finite and > 0 (lb = 0 is
 *   singular by construction, Kd sqrt(w) = 0, and gives Inf / NaN in the reference): JCH_EINVAL otherwise.
 *   Outputs: A, alpha n x q (ld n) [loc]; df 1 HOST (required with want_df); info 1 HOST: 0, or the 1-based column whose pivot was not
 *   > 0 — then the kernel / parameter set is not PSD enough for this lb, the call returns JCH_EINVAL with that column in the message
 *   and A, alpha, df are not written.  The next call on the ctx works as usual. */
JCH_API int32_t jch_krr_solve(jch_ctx *ctx, int32_t loc, const double *Kd, int64_t n, const double *B, int64_t q, const double *weights_norm,
                              double lb, int32_t want_df, double *A, double *alpha, double *df, int32_t *info);

/* ---- row-wise spectra preprocessing (src/preprocessing.jl) -------------------------------------------------------
 * Three primitives the reference's snv!, detrend!, savgol!, mavg!, mavg_runmean! and fdif! reduce to.  Float64; X n x p column-major
 * (ldx >= n), out column-major (ldo >= n), both [loc]; rows are independent (a communicator of any size: every rank preprocesses its own
 * shard, no collective).  One thread owns a row from its first load to its last store, so
 *   - out == X (with ldo == ldx) works for every entry and mode and needs no second n x p buffer (any other overlap of out and X is
 *     undefined); host data is staged in row blocks of at most 64 MiB;
 *   - every output element is one thread's fixed-order sum (two runs give identical bits) and a NaN / Inf in row i changes row i only.
 * A call ends the validity of the working copy a fit may have left for JCH_REUSE_XCOPY (X may just have been rewritten in place).
 *
 * jch_rows_standardize — `snv!` (src/preprocessing.jl:473-481): out[i, :] = (x_i - mu_i) / s_i, mu_i = the row mean (0 without cent),
 *   s_i = the UNcorrected row standard deviation around the row mean (src/utility.jl rowstd; 1 without scal), two-pass (the mean, then the
 *   squared deviations).  A constant row divides by s_i = 0 as the reference does: NaN / Inf in that row.
 * jch_rows_project_out — `detrend!` (:32-47): out[i, :] = x_i - V (A x_i); A (k x p, column-major ld k) and V (p x k, column-major ld p)
 *   HOST matrices, 1 <= k <= 8.  For detrend V = vX and A = pinv(vX'vX, rtol = sqrt(eps)) vX' are built by the caller on the host.
 * jch_rows_fir — `savgol!` (:424-441), `mavg!` (:247-260), `mavg_runmean!` (:307-335), `fdif!` (:87-93): taps f HOST doubles, f >= 1.
 *   mode JCH_FIR_SAME: p outputs, out[i, j] = sum_{t < f} taps[t] x[i, clamp(j + lo + t, 0, p - 1)] (replicate border), -(f - 1) <= lo <= 0
 *   (the window contains its output); any f, f > p included.  mode JCH_FIR_VALID: p - f + 1 outputs, lo == 0, f <= p, no clamping; in place
 *   the columns from p - f + 1 on keep their input values.  Taps that are exactly 0.0 are skipped (no 0 * Inf; fdif is one subtraction).
 *   Windows up to 57 run from a ring of the row's originals; wider ones from a copy of a bounded block of rows.
 *   mode JCH_FIR_SAME | JCH_FIR_PER_COLUMN (`predict(::CalPds, X)`, src/calpds.jl:89-99, as one banded map): every output
 *   column has taps and a constant of its own.  Table layout: taps is a HOST table of (f + 1) x p doubles, column-major with ld f + 1;
 *   column j holds the f taps of output j followed by its constant c_j.  p outputs,
 *     out[i, j] = (sum_{t < f} taps[t, j] x[i, clamp(j + lo + t, 0, p - 1)]) + c_j,   -(f - 1) <= lo <= 0, any f >= 1 (f > p included).
 *   Summation order: the taps are summed in the order of t, starting from 0.0, and the constant is added last; a tap that is exactly 0.0 is
 *   skipped (a zero-padded border window never multiplies a clamped column and never forms 0 * Inf).  JCH_FIR_PER_COLUMN is a flag ORed
 *   into the mode: JCH_FIR_VALID | JCH_FIR_PER_COLUMN and every other value (2 and 3 are not modes) are JCH_EINVAL.  out == X, host
 *   staging, the ring up to 57 taps and the row-block copy beyond are those of the uniform modes, whose code path and bits are unchanged. */
#define JCH_FIR_SAME 0
#define JCH_FIR_VALID 1
#define JCH_FIR_PER_COLUMN 4   /* a flag, ORed into the mode; 2 and 3 are not modes */
JCH_API int32_t jch_rows_standardize(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, int32_t cent, int32_t scal,
                                     double *out, int64_t ldo);
JCH_API int32_t jch_rows_project_out(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *A, const double *V,
                                     int32_t k, double *out, int64_t ldo);
JCH_API int32_t jch_rows_fir(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *taps, int64_t f, int64_t lo,
                             int32_t mode, double *out, int64_t ldo);

/* ---- Covsel: variable selection by repeated argmax and deflation (src/covsel.jl, src/covselr.jl) ----------------------
 * jch_covsel_fit — `covsel!` / `covsel` (src/covsel.jl:59-122).  Float64; X n x p (ldx >= n) and Y n x q (ldy >= n) column-major [loc];
 * one GPU only (a communicator of more than one rank is JCH_EINVAL).  xmeans, ymeans (:64-67); for q > 1 Y is divided by its uncorrected
 * column stds (:68-70; yscales is ones when q == 1).  Per step (:81-116): the criterion z over the columns (typ JCH_COVSEL_COV:
 * z_j = sum_k (Xd'Yd / n)_jk^2, :83-84; JCH_COVSEL_COR: the squared correlations, :87-88; "aic", :92-103, is not provided), C[:, i] = z,
 * its argmax (ties: the lowest index; a NaN never wins), then X and Y orthogonalised to that column.  The reference does that with an
 * n x n projector (:78, :111-113); here X is only READ, once per step: an orthonormal basis Q of the deflated selected columns and
 * Yd = (I - QQ')Yc are kept, Xd'Yd = Xc'Yd, the deflated column sums of squares are css_j - sum_k G[j,k]^2 with G = Xc'Q, and the deflated
 * selected column is Xc[:, j] - Q G[j, :]' (orthogonalised against Q a second time before it is normalised).
 *   nlv >= 1 is clamped to p.  Deviations: a column whose deflated sum of squares is <= 1e-10 of its original one is
 *   exhausted — `cor` gives it z = 0 (the reference divides rounding noise by rounding noise there), and when the argmax lands on one the
 *   loop stops: *nlv_out = the completed steps (< nlv on a rank-deficient X), and what belongs to later steps is 0 (column nlv_out of C
 *   holds the criterion of the abandoned step).
 *   inplace != 0: X <- Xc - Q G' and Y <- Yd, what the reference leaves in its arguments (:112-113); the working copy a fit left for
 *   JCH_REUSE_XCOPY is then no longer valid.  inplace == 0: X and Y are not written.
 * Outputs, each may be NULL; HOST unless noted.  sel int32 [nlv], 0-based; selcov [nlv] (:108); cov2 [p] (:109); C p x nlv (ld p);
 * cumpvarx, cumpvary [nlv] (:117-118); xmeans [p]; ymeans, yscales [q]; G p x nlv (ld p) = Xc'Q; QtY nlv x q (ld nlv) = Q'Yc in the units of
 * the SCALED Y (multiply column k by yscales[k] for raw units); Q n x nlv (ld n) [loc]; nlv_out.  With Xc[:, sel] = Q R and
 * R[k, i] = G[sel_i, k] (upper triangular), `covselr` (src/covselr.jl:48-53) is B = R^-1 QtY on the host.
 * Every sum is taken in a fixed order: two runs give identical bits. */
#define JCH_COVSEL_COV 0
#define JCH_COVSEL_COR 1
JCH_API int32_t jch_covsel_fit(jch_ctx *ctx, int32_t loc, double *X, int64_t n, int64_t p, int64_t ldx, double *Y, int64_t q, int64_t ldy, int32_t nlv,
                               int32_t typ, int32_t inplace, int32_t *sel, double *selcov, double *cov2, double *C, double *cumpvarx, double *cumpvary,
                               double *xmeans, double *ymeans, double *yscales, double *G, double *QtY, double *Q, int32_t *nlv_out);
/* jch_covsel_pass — the one kernel a Covsel step spends its time in, on its own: out (p x b, ld p) = (X - 1 mu')' V, all DEVICE pointers; X n x p
 * (ldx >= n, read only), mu p means or NULL (no centring), V n x b (ldv >= n), any b >= 1: up to 32 panel columns are served by one read of X,
 * wider panels by one read per 32 columns.  mu is subtracted in registers (nothing relies on sum(V) = 0).  Per-workgroup partials are summed in
 * a fixed order: two runs give identical bits. */
JCH_API int32_t jch_covsel_pass(jch_ctx *ctx, const double *X, int64_t n, int64_t p, int64_t ldx, const double *mu, const double *V, int64_t b, int64_t ldv,
                                double *out);

/* ---- weighted centred Gram, PCA and PCR (src/pcasvd.jl, src/pcaeigen.jl, src/pcr.jl) ----------------------------------------
 * jch_xtdx -- G = (X - 1 mu')' D (X - 1 mu') (p x p), D = diag(weights / sum weights) (weights NULL = ones), mu = X'D 1, in one pass over the
 * column-major X on the f64 matrix cores with no n x p workspace: the means and the weights are applied in registers (nothing is computed as
 * X'DX - mu mu').  X n x p (ldx >= n) and weights (n) [loc], read only; p <= 32768; row indices are 64-bit.  G_dev (ld ldg >= p) and mu_dev (p): DEVICE
 * pointers, each may be NULL (ctx workspace); G_host (p x p, ld p) and mu_host (p): HOST copies, each may be NULL.  Rows >= n are never read.  Every
 * sum has a fixed order and both triangles are written from one value: G == G' bitwise, two runs give identical bits, and so do a host and a
 * device X and an aligned and an unaligned X.  A NaN at X[r, j] reaches only row j and column j of G.  One rank only. */
JCH_API int32_t jch_xtdx(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *weights, double *G_dev, int64_t ldg,
                         double *mu_dev, double *G_host, double *mu_host);
/* jch_pca_fit -- `pcasvd!` / `pcaeigen!` / `pcaeigenk!` (src/pcasvd.jl:79-101) and what `pcr!` (src/pcr.jl:82-97) adds to it.  P and sv^2 are the nlv
 * leading eigenpairs of G = Xs'D Xs (Xs = cscale(X, xmeans, xscales); jch_xtdx, rescaled by xscales = sqrt(diag G) when scal) from the block
 * subspace iteration of jch_kpca_fit (tol, maxit: its stopping rule on the residuals |G p_i - eig_i p_i| <= tol eig_1); T = Xs P.  X is never
 * written (the reference's `!` forms leave the centred X in their argument; here they do not).  nlv is clamped to min(n, p).
 *   X n x p, weights n or NULL, Y n x q or NULL (q = 0) [loc].
 *   Outputs, each may be NULL: T n x nlv (ld n) and weights_norm n [loc]; HOST: P p x nlv (ld p), each column signed so that its largest-|.| entry
 *   (first index on ties) is positive; sv, eig, resid (nlv values: the reference keeps min(n, p)); xmeans, xscales, colvar = diag(G) before the
 *   rescaling (p); sstot = trace(G); niter; nlv_out; converged (1 / 0: the iteration's own decision).  With Y: ymeans (q) and xtdy = Xs'D (Y - 1 ymeans') (p x q, ld p, through jch_covsel_pass),
 *   from which beta = diag(1 / eig) P' xtdy (src/pcr.jl:93).  One rank only.  Every sum has a fixed order: two fits give identical bits. */
JCH_API int32_t jch_pca_fit(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *weights, const double *Y, int64_t q,
                            int64_t ldy, int32_t nlv, int32_t scal, double tol, int32_t maxit, double *T, double *P, double *sv, double *eig, double *xmeans,
                            double *xscales, double *weights_norm, double *sstot, double *colvar, double *ymeans, double *xtdy, int32_t *niter,
                            double *resid, int32_t *nlv_out, int32_t *converged);

/* ---- outlier distances (src/occsd.jl, src/occod.jl, src/occsdod.jl) ------------------------------------------------------------
 * jch_row_resid_ss -- out[i] = sum_j ( X[i, j] - shift[j] - sum_{l < k} Z[i, l] B[j, l] )^2: the row sums of squares of the rank-k residual
 * E = (X - 1 shift') - Z B' without forming E (the reference's `sum(E .* E, dims = 2)` over `xresid`, src/occod.jl:48-49, with shift = xmeans, Z = the
 * scores and B = diag(xscales) P[:, 1:k]).  X m x p (ldx >= m), Z m x k (ldz >= m) and out (m) [loc], X and Z read only; shift (p, NULL = zeros) and
 * B (p x k, ldb >= p) HOST.  k = 0 is valid (Z and B may then be NULL): the centred row sums of squares.  Any m, p, k: coefficients that do not fit in
 * LDS are read from L2, more than 64 score columns are walked in chunks.  Rows >= m and columns >= p are never read.  Every sum has a fixed order and
 * no atomics: two runs give identical bits, and so do a host and a device X or Z and an aligned and an unaligned one.  A NaN at X[i, j] or Z[i, l]
 * reaches out[i] only.  Rank-local on a joined ctx: the rows are independent, no collective (class L of the joined ctx contract). */
JCH_API int32_t jch_row_resid_ss(jch_ctx *ctx, int32_t loc, const double *X, int64_t m, int64_t p, int64_t ldx, const double *shift, const double *Z,
                                 int64_t k, int64_t ldz, const double *B, int64_t ldb, double *out);
/* jch_row_resid_ss_lv -- the nested form, every level a_lo .. a_hi in ONE read of X (src/wshenk.jl:59-62 forms nlv `xresid` matrices):
 * out[i + (a - a_lo) ldo] = sum_j ( X[i, j] - shift[j] - sum_{l < a} Z[i, l] B[j, l] )^2 for 0 <= a_lo <= a_hi <= kz.  X m x p (ldx >= m), Z m x kz
 * (ldz >= m) and out m x (a_hi - a_lo + 1) (ldo >= m) [loc], X and Z read only; shift (p, NULL = zeros) and B (p x kz, ldb >= p) HOST.  a_hi = 0 is
 * valid (Z and B may then be NULL).  The residual of level a is the residual of level a - 1 minus one rank-one term, subtracted and then squared (no
 * expanded form).  Any m, p, kz: one read of X holds for a_hi <= 32; beyond, every further 32 levels are one more launch that reads X again and replays the terms before its chunk.  Rows >= m, columns >= p and score columns >= a_hi
 * are never read; out beyond row m of a column is never written.  Every sum has a fixed order and no atomics: two runs give identical bits, and so do
 * a host and a device X or Z and an aligned and an unaligned one, and level a has the same bits whatever a_lo and a_hi.  A NaN at X[i, j] or Z[i, l]
 * reaches row i only.  Rank-local on a joined ctx, like jch_row_resid_ss. */
JCH_API int32_t jch_row_resid_ss_lv(jch_ctx *ctx, int32_t loc, const double *X, int64_t m, int64_t p, int64_t ldx, const double *shift, const double *Z,
                                    int64_t kz, int64_t ldz, const double *B, int64_t ldb, int32_t a_lo, int32_t a_hi, double *out, int64_t ldo);

/* ---- exact column medians and MADs, Stahel-Donoho outlyingness (src/utility.jl:162, src/stah.jl, src/occstah.jl) ---------------
 * jch_col_median_mad -- med[j] = median(X[:, j]), mad[j] = 1.4826022185056018 * median(|X[:, j] - med[j]|) (StatsBase's `mad`), by an
 * exact radix select on the device: no sampling, no sort, no n x p workspace (the deviations fl(|fl(x - med)|) are recomputed from X in every pass).
 * X n x p (ldx >= n) [loc], read only; med and mad (p values each; mad may be NULL) on the host or the device as out_loc says.  With loc and
 * out_loc both JCH_LOC_DEVICE the call only enqueues on the ctx stream and returns without a host synchronisation.  Odd n: the order statistic of
 * rank (n - 1) / 2; even n: Julia's middle(lo, hi) = lo / 2 + hi / 2 of ranks n / 2 - 1 and n / 2.  Any n >= 1 and p >= 1; rows >= n are never read; row
 * indices and counts are 64-bit.  Integer counters only: two runs give identical bits, and so do a host and a device X and an aligned and an
 * unaligned one.  A column holding a NaN gets med = mad = NaN and no other column is touched; +-Inf are ordinary ordered values (a NaN deviation
 * Inf - Inf makes that column's MAD NaN); the sign of a zero result is not specified.  One rank only (a median needs every row: a
 * communicator of more ranks is JCH_EINVAL before any device work, like jch_stah). */
JCH_API int32_t jch_col_median_mad(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, double *med, double *mad, int32_t out_loc);
/* jch_stah -- `stah` (src/stah.jl:37-58, fit != 0) and the distances of `predict(::Occstah, X)` (src/occstah.jl:55-73, fit = 0) in one entry:
 * d[i] = max_j |(t_ij - mu_j) / s_j| with T = ((X - 1 mu_scal') diag(1 / s_scal)) P.  X n x p (ldx >= n) and d (n) [loc], X read only; mu_scal and
 * s_scal (p, NULL = zeros / ones) and P (p x a, ldp >= p) HOST; mu and s (a) HOST: written when fit (the medians and MADs of the columns of T,
 * jch_col_median_mad), read otherwise.  P is walked in column panels within a fixed workspace budget: T never exists beyond one panel, a host X is
 * staged once, the whole loop is enqueued without a host synchronisation.  The projection is jch_affine_gemm's (centring and scaling folded into
 * the coefficients); the division by s_j is a true division and nothing guards s_j = 0 (a constant direction gives the IEEE result).  A NaN term
 * makes d[i] NaN and stays in its row.  Any n, a >= 1.  One rank only. */
JCH_API int32_t jch_stah(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *mu_scal, const double *s_scal,
                         const double *P, int64_t a, int64_t ldp, int32_t fit, double *mu, double *s, double *d);

/* ---- spatial median and spherical PCA (src/colmedspa.jl, src/pcasph.jl) ----------------------------------------------------------
 * X n x p (ldx >= n) [loc], read only, never written; any n, p >= 1; rows >= n and columns >= p are never read; row numbers are 64-bit.  No atomics,
 * every sum in a fixed order: two runs give identical bits, and so do a host and a device X and an aligned and an unaligned one.  One rank only.
 * jch_weiszfeld_step -- ONE step of `colmedspa` (src/colmedspa.jl:15-30) from the centre mu0 in one read of X: d_i = |x_i - mu0|, w0 = median(d)
 *   (Julia's: lo / 2 + hi / 2 for even n), ep = delta w0, u_i = ep when d_i <= ep and 1 / d_i otherwise (the literal reading of :20-23), mu =
 *   sum u_i x_i / sum u_i, h = |mu - mu0|.  The pass cannot know ep before it has every distance: it leaves the rows with d_i <= guard out of its
 *   sums and they are added afterwards, in ascending row order, with their true weight.  guard >= 0 must be >= ep, else JCH_EINVAL once the median
 *   is known (mu, d, h and nleft are then not written); guard = +Inf sends every row through the second stage; guard < 0: the distances are taken
 *   first (one more read of X) and the pass runs with guard = ep.  mu0 and mu (p) HOST; d (n) [loc], may be NULL; HOST scalars, each may be NULL:
 *   w0, h, nleft = the rows the pass left out.  A NaN in X makes w0, h and every entry of mu NaN.
 * jch_spatial_median -- `colmedspa(X; delta)` (:4-33): the column medians (jch_col_median_mad), then steps while h > delta sqrt(p), the first with
 *   guard < 0, every later one with guard = delta (w0_prev + h_prev) (1 + 2^-40), an upper bound of its ep by the triangle inequality (a step whose
 *   guard rounding has put below ep is redone with the exact clamp).  The host reads one scalar record per step.  maxit >= 1 bounds the steps (the
 *   reference loops for ever on data that never converge): converged = 0 reports it.  mu (p) HOST; d (n) [loc], may be NULL: the distances to the
 *   LAST centre stepped from, as the loop left them; niter, h_last, converged HOST, each may be NULL.  NaN in X: one step, mu = NaN, converged = 1
 *   (the reference's `while h > delta1` ends on a NaN h too); n = 1 gives NaN through 0 / 0, as in the reference. */
JCH_API int32_t jch_weiszfeld_step(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *mu0, double delta,
                                   double guard, double *mu, double *d, double *w0, double *h, int64_t *nleft);
JCH_API int32_t jch_spatial_median(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, double delta, int32_t maxit, double *mu,
                                   double *d, int32_t *niter, double *h_last, int32_t *converged);
/* jch_pcasph_fit -- `pcasph!` (src/pcasph.jl:60-92) without a copy of X, a transpose or an SVD.  xmeans = the spatial median (typc = JCH_CENT_MEDSPA;
 *   delta, maxit_med as above) or the weighted column mean (JCH_CENT_MEAN); xscales = ones or, scal != 0, colstd(X, weights) about the weighted mean
 *   whatever typc (:72); r_i = |(x_i - xmeans) / xscales|; G = Xs' diag(w_i / r_i^2) Xs (jch_xtdx's pass with mu = xmeans, rescaled by xscales when scal:
 *   the Gram of the rows projected on the unit sphere); P = its nlv leading eigenvectors (jch_pca_fit's iteration, tol, maxit, sign rule); T = Xs P;
 *   sv = the MADs of the columns of T / r (jch_col_median_mad on the device); T, P, sv, eig and resid are returned ordered by sv descending, ties in
 *   eigen order (:87-90).  A row with r_i = 0 makes the reference's SVD fail on NaN; here it gets weight 0 in G and a zero row in T / r, and is
 *   counted in nzero.  nlv is clamped to min(n, p); p <= 32768.
 *   weights n or NULL [loc].  Outputs, each may be NULL: T n x nlv (ld n) and weights_norm n [loc]; HOST: P p x nlv (ld p); sv, eig (the eigenvalues
 *   of G), resid (nlv); xmeans, xscales, colvar = the weighted variances of the columns of X about the weighted mean (p); sstot = trace(G);
 *   niter_med, converged_med (0, 1 when typc = JCH_CENT_MEAN); niter, converged (the eigen iteration); nlv_out; nzero. */
#define JCH_CENT_MEDSPA 0
#define JCH_CENT_MEAN 1
JCH_API int32_t jch_pcasph_fit(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const double *weights, int32_t nlv, int32_t typc,
                               double delta, int32_t maxit_med, int32_t scal, double tol, int32_t maxit, double *T, double *P, double *sv, double *eig,
                               double *xmeans, double *xscales, double *weights_norm, double *sstot, double *colvar, int32_t *niter_med,
                               int32_t *converged_med, int32_t *niter, double *resid, int32_t *converged, int32_t *nlv_out, int64_t *nzero);

/* ---- Kennard-Stone and Duplex sampling without an n x n distance matrix (src/sampling.jl:40-148) ---------------------------------
 * Row indices are 0-based int64_t.  X n x p (ldx >= n) [loc], read only; a host X is staged once per call.  No atomics: two runs give identical
 * bits, and so do a host and a device X and an aligned and an unaligned one.  One rank only.
 * jch_farthest_pair -- pair[0] > pair[1] (HOST): the two rows with the largest squared Euclidean distance among the rows that are not listed in
 * skip (nskip indices, HOST; may be NULL when nskip = 0) and hold no non-finite entry; ties go to the smallest pair[1], then the smallest pair[0]:
 * the first maximum of a column-major scan of the symmetric distance matrix (`findall(D .== maximum(D))[1]`).  The search compares
 * |a_i|^2 + |a_j|^2 - 2 a_i.a_j of the rows a = x - c centred on the column means of the candidates, 128 x 128 tiles of the triangle on the f64
 * matrix cores, n^2 p flop, nothing n x n stored (one triple per tile); every compared value is within 4 (p + 20) 2^-53 of the largest squared
 * distance.  *d2 (HOST) = the pair's squared distance in direct form, sum_j (x_rj - x_cj)^2 in ascending j.  JCH_EINVAL: fewer than
 * two candidate rows, a skip index out of range, more than 2^31 - 1 tiles.
 * jch_maxmin_select -- nsets = 1: Kennard-Stone; nsets = 2: Duplex.  init (HOST, 2 nsets indices): the starting pair of each set; k >= 2: rows per
 * set, the starting pair included (k <= n, 2 k <= n for Duplex).  Every further row of a set is argmax_i min_{s in the set} d2(i, s) over the rows
 * no set has taken, ties to the smallest index; in a Duplex step the first set chooses first.  d2 in direct form, ascending j.  One read of X per
 * selected row (per pair of rows for Duplex), no host synchronisation inside the loop.  sel (HOST, k x nsets column-major): the rows in the order
 * they were taken; dsel (HOST, same shape, may be NULL): the min-distance at which each row was taken, the starting pairs their mutual d2.  A
 * row with a non-finite distance to a selected row is never taken and changes nothing for the others.  JCH_EINVAL: k out of range, init out of
 * range or repeated, fewer than k nsets rows that can be taken. */
JCH_API int32_t jch_farthest_pair(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, const int64_t *skip, int32_t nskip,
                                  int64_t *pair, double *d2);
JCH_API int32_t jch_maxmin_select(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t p, int64_t ldx, int32_t nsets, const int64_t *init,
                                  int64_t k, int64_t *sel, double *dsel);

/* ---- harness utilities (bench / tests) ---------------------------------------------------------- */
/* Fill device matrix out (n x p, column-major ld) with rows [row0,row0+n) of the n_total x p matrix
 * whose element (i,j) is splitmix64-uniform(seed, i + j*n_total) — the README's `rand(n,p)` stand-in
 * (README.md:79-94), identical to oracle/plsr_oracle.py:splitmix64_uniform. */
JCH_API int32_t jch_fill_uniform(jch_ctx *ctx, double *dev_out, int64_t n, int64_t p, int64_t ld, int64_t row0,
                         int64_t n_total, uint64_t seed);

/* out (n x b, ld ldo) = Kc V, Kc n x n (ld n), V n x b (ld ldv), all DEVICE pointers: the panel product of jch_kpca_fit on the
 * f64 matrix cores (any b >= 1, in chunks of 64 columns).  Every output is one workgroup's fixed-order sum. */
JCH_API int32_t jch_kc_panel(jch_ctx *ctx, const double *Kc, int64_t n, const double *V, int64_t ldv, int32_t b, double *out, int64_t ldo);

/* The dense direct solver under jch_krr_solve on its own, DEVICE pointers, column-major.
 * jch_chol_factor: A (n x n, ld lda >= n, any n >= 1) = L L' in place on the f64 matrix cores; only the lower triangle of A is read
 *   and written.  *info (HOST) = 0, or the 1-based index of the first column whose pivot was not > 0 (negative, zero, NaN): a
 *   result, not an error — the call returns JCH_OK, A is then partly overwritten and there is no factor to solve with.  The
 *   inverses of the 128 x 128 diagonal blocks stay in ctx workspace, keyed to (A, n, lda).
 * jch_chol_solve: B (n x q, ld ldb, any q >= 1) = (L L')^-1 B in place with the factor the LAST jch_chol_factor of this ctx left in
 *   L; any other L, n or ldl is JCH_EINVAL, not a wrong answer.
 * jch_chol_inv_fro2: *out (HOST) = |L^-1|_F^2 = trace((L L')^-1) for that same factor; n^3/3 flop and an n x n workspace in the ctx
 *   (JCH_ENOMEM when it cannot be had).
 * Every output element is a fixed-order sum: two runs give identical bits. */
JCH_API int32_t jch_chol_factor(jch_ctx *ctx, double *A, int64_t n, int64_t lda, int32_t *info);
JCH_API int32_t jch_chol_solve(jch_ctx *ctx, const double *L, int64_t n, int64_t ldl, double *B, int64_t q, int64_t ldb);
JCH_API int32_t jch_chol_inv_fro2(jch_ctx *ctx, const double *L, int64_t n, int64_t ldl, double *out);

/* ---- the k-nearest-neighbour search on its own, and the reductions over a neighbourhood (src/getknn.jl, src/knnr.jl, src/knnda.jl,
 * src/occknndis.jl, src/occlknndis.jl) -------------------------------------------------------------------------------------------
 * jch_knn_prepare -- a handle on a search space Ztrain (n x dd, ldzt >= n) [loc]: the device copy of it and, where the screened search can apply
 *   (dd <= 62, n < 2^26), the screen's operand copy, built once.  jch_knn_release frees it (NULL is allowed).
 * jch_knn_search -- the k nearest rows of the search space for each of the m rows of Zq (m x dd, ldzq >= m) [loc], in (distance, row index) order:
 *   exactly the search of jch_lwplsr_predict (the screened search on the bf16 matrix cores with exact Float64 distances for the survivors, the exact
 *   scan, or the generic selection outside their envelopes: any n, dd, k; JCH_KNN_SCREEN=0 / JCH_KNN_GENERIC=1 choose as they do there), without
 *   the local fits.  Outputs [out_loc], each may be NULL: ind (int32, 0-based, [m][k] row-major), dist and w ([m][k]: Euclidean distances, not
 *   squared, and the `wdist` weights exp(-d / (h MAD)) / max with the 4-MAD cutoff, NaN -> 1, then clamped from below to tol, src/wdist.jl:64-75;
 *   h = Inf is valid: all weights 1 before the clamp), dmed ([m]: the median of the query's k distances, Julia's middle(lo, hi) = lo / 2 + hi / 2
 *   for even k).  k is clamped to the number of candidates: n, or n - 1 when `self` is given (the caller sizes the outputs with the clamped k).
 *   self: NULL, or [m] int64 [loc]; self[i] >= 0 removes training row self[i] from query i's candidates -- the reference's
 *   getknn(rmrow(T, s), ...) without the copy, rows reported in the ORIGINAL numbering.  Done as a search for k + 1 followed by the drop of the
 *   entry of row self[i] if it is among them and of the last entry otherwise (also for self[i] < 0); weights and dmed are computed after the drop,
 *   over the k kept distances.  A query holding a NaN gets NaN distances, the in-range rows 0 .. k-1 and weights 1, and disturbs no other query.
 *   With loc and out_loc both JCH_LOC_DEVICE the call only enqueues on the ctx stream; otherwise it returns synchronised.  The screen counters
 *   (JCH_COUNTER_KNN_SCREENED / _REDONE) and the handle's "stop screening" rule follow host-output calls only.  All jch_knn_* entries are
 *   rank-local on a joined ctx (class L of the joined ctx contract): every rank searches its own handle for its own queries, no collective.
 * jch_knn_wmean -- pred[i, c] = sum_j (w_ij / sum_j w_ij) Y[ind_ij, c] (`mweight` + `colmean`, src/knnr.jl:120-124).  Y n x q (ldy >= n), ind and w
 *   [m][k], pred m x q column-major (ld m), all [loc].  Fixed summation order (per query one wave: lane l adds the terms l, l + 64, ... in order, the
 *   64 partial sums combine in a fixed butterfly), no atomics: two runs give identical bits.  Error per element <= 4 (k + 4) 2^-53 sum_j w~_ij |y_ij|.
 *   A NaN stays in its query.  A row index outside [0, n) contributes NaN.
 * jch_knn_vote -- score[i, c] = sum of w_ij over the neighbours j with cls[ind_ij] = c, in neighbour order (m x ncls column-major, ld m; may be NULL;
 *   0 for an absent class); pred[i] (int32) = the class with the largest score among those PRESENT in the neighbourhood, ties to the lowest code
 *   (`findmax_cla`, src/utility.jl:564-570).  cls: [n] int32 class codes, 0-based in sorted-level order; codes outside [0, ncls) are ignored.  Any
 *   ncls >= 1.  All arrays [loc].
 * jch_knn_gather_median -- out[i] = median_j v[ind_ij], middle(lo, hi) for even k; NaN sorts last and the median is NaN if a middle place is.
 *   v (n), ind [m][k], out (m), all [loc].  Any k.
 * The last three only enqueue on the ctx stream when loc is JCH_LOC_DEVICE. */
typedef struct jch_knn_model jch_knn_model;
JCH_API int32_t jch_knn_prepare(jch_ctx *ctx, int32_t loc, const double *Ztrain, int64_t n, int64_t dd, int64_t ldzt, jch_knn_model **model_out);
JCH_API int32_t jch_knn_release(jch_ctx *ctx, jch_knn_model *model);
JCH_API int32_t jch_knn_search(jch_ctx *ctx, const jch_knn_model *model, int32_t loc, const double *Zq, int64_t m, int64_t ldzq, int32_t k,
                               const int64_t *self, double h, double tol, int32_t out_loc, int32_t *ind, double *dist, double *w, double *dmed);
JCH_API int32_t jch_knn_wmean(jch_ctx *ctx, int32_t loc, const double *Y, int64_t n, int64_t q, int64_t ldy, const int32_t *ind, const double *w,
                              int64_t m, int32_t k, double *pred);
JCH_API int32_t jch_knn_vote(jch_ctx *ctx, int32_t loc, const int32_t *cls, int64_t n, int32_t ncls, const int32_t *ind, const double *w, int64_t m,
                             int32_t k, int32_t *pred, double *score);
JCH_API int32_t jch_knn_gather_median(jch_ctx *ctx, int32_t loc, const double *v, int64_t n, const int32_t *ind, int64_t m, int32_t k, double *out);

/* ---- the local fit of the locally weighted MLR models (src/lwmlr.jl, src/lwmlr_s.jl, src/lwmlrda.jl, src/lwmlrda_s.jl through src/locw.jl and
 * src/mlr.jl:69-86) ----------------------------------------------------------------------------------------------------------------
 * jch_knn_wls -- for each of the m queries a weighted least-squares regression of its k neighbours' responses on their d coordinates, and the
 *   prediction of the query's own row.  X n x d (ldx >= n), Y n x q (ldy >= n), Xq m x d (ldq >= m), column-major; ind (int32, 0-based) and w [m][k]
 *   row-major, as jch_knn_search writes them; pred m x q column-major (ld m); info [m] int32, may be NULL.  All arrays [loc].  Any n, m, d, q, k >= 1
 *   (d, q <= 2^20).  Per query i, with the rows r_j = ind[i][j]:
 *       w~_j = w_ij / sum_j w_ij (`mweight`);  xbar = sum_j w~_j X[r_j, :], ybar = sum_j w~_j Y[r_j, :];
 *       A = diag(sqrt(w~)) (X[r, :] - 1 xbar'), B = diag(sqrt(w~)) (Y[r, :] - 1 ybar');
 *       beta = argmin |A beta - B| by Householder QR of A (no pivoting, no normal equations: the reference's `mlr` is the QR one);
 *       pred[i, :] = ybar + (Xq[i, :] - xbar)' beta -- the reference's `int + x B` in centred form;  info[i] = 0.
 *   Special cases:
 *   - q == 1 and the k gathered responses all == (src/locw.jl:33-34): pred[i] is that value exactly and info[i] = 2, whatever k and d are.  For
 *     q > 1 there is no shortcut.
 *   - rank deficiency -- k <= d (a centred k-row slab has rank <= k - 1), or some |r_jj| <= min(k, d) 2^-52 max_i |r_ii|: the whole row pred[i, :]
 *     is NaN and info[i] = 1.  A DEPARTURE from the reference, whose `\` returns LAPACK's minimum-norm solution on such a slab.
 *   - a NaN in a neighbourhood or in a query stays in that query's row (info[i] = 0: it is no rank deficiency); a row index outside [0, n) gathers
 *     NaN, so the whole row pred[i, :] is NaN, and is never read out of bounds.  The weights are expected > 0 (jch_knn_search clamps them to tol).
 *   Fixed summation order, no atomics: the same call gives the same bits.  One 256-thread workgroup per query, one launch; the k x (d + q) slab
 *   lives in LDS while 8 ((d + q) (k | 1) + 2 k + 3 d + q + ceil(k / 2)) bytes <= 150 KiB, beyond that in the ctx workspace (the same device code,
 *   slower, never absent).  The entry first writes a row-major copy [X | Y] (n (d + q) doubles) into the ctx workspace.  It reserves the kNN
 *   workspace only: the X copy a fit left for JCH_REUSE_XCOPY survives.  With loc JCH_LOC_DEVICE the call only enqueues on the ctx stream;
 *   otherwise it returns synchronised.  Rank-local on a joined ctx (class L): one QR per query, no collective. */
JCH_API int32_t jch_knn_wls(jch_ctx *ctx, int32_t loc, const double *X, int64_t n, int64_t d, int64_t ldx, const double *Y, int64_t q, int64_t ldy,
                            const double *Xq, int64_t m, int64_t ldq, const int32_t *ind, const double *w, int32_t k, double *pred, int32_t *info);

/* ---- local PLS discrimination (src/lwplsrda.jl, src/lwplslda.jl, src/lwplsqda.jl through src/locwlv.jl) ---------------------------------
 * jch_knn_gda -- for each of the m queries the Gaussian discriminants (kind 1: `lda`, src/lda.jl:56-77; kind 2: `qda`, src/qda.jl:55-79) of its k
 *   neighbours' scores, for ALL the nested score spaces T[:, 1:a], a = nlv_lo .. nlv_hi, from one Cholesky factorisation and one forward substitution
 *   per covariance: the factor of a leading block is the leading block of the factor, so the squared Mahalanobis distance on the first a columns is a
 *   prefix sum of z_j^2, z = L^-1 (tq - mu), and det S_a a prefix product of L_jj^2 (the reference refits per a, src/plslda.jl:84-86).
 *   T [m][k][a_hi] (the score of neighbour e of query i on column j at (i k + e) a_hi + j), tq [m][a_hi] the queries' own scores, cls_nb [m][k] int32
 *   the neighbours' class codes in 0 .. nlev - 1, post [m][le][nlev], code and info [m][le] int32, le = nlv_hi - nlv_lo + 1; all [loc].
 *   1 <= nlv_lo <= nlv_hi <= a_hi; prior 0 = "unif", 1 = "prop".  Per query:
 *     the local levels are the codes present, with counts ni; wprior = 1 / nlev_loc or ni / k; class means of the scores, unweighted;
 *     Wi = the uncorrected covariance of the class's rows, for a class of ONE row that of all k rows (src/matW.jl:55-65);
 *     lda: S = (sum_i ni / k Wi) k / (k - nlev_loc), shared; qda: S_i = Wi ni / (ni - 1), Wi itself when ni = 1;
 *     dens_a = (2 pi)^(-a / 2) detS_a^(-1/2) exp(-d2_a / 2) (a detS of 0 is replaced by 1e-20, src/dmnorm.jl:122); post = wprior .* dens, normalised;
 *     an absent class has posterior 0; code = the first maximum over the local levels (a NaN counts as the largest value: Julia's argmax).
 *   info: 0 = fitted (all densities 0: a NaN posterior and the first local level); 1 = one local level: code is that class, post one-hot;
 *     2 = pivot j of a covariance was <= (k + 4 j) 2^-52 S_jj (the error the covariance sum and the factorisation leave on the diagonal): the
 *     models a >= j of that query get post NaN and code -1, the models a < j are valid; 3 = non-finite: a non-finite density (a NaN in the
 *     query's scores) or a NaN pivot (a NaN among the neighbours' scores in the first a columns): post NaN, code the first local level; also for
 *     a code outside 0 .. nlev - 1 in the list (code -1).
 *   Differences t - mu are taken before any product; fixed summation order, no atomics: the same call gives the same bits; a NaN stays in its
 *   query.  One 256-thread workgroup per query; scores, covariance and factor live in LDS while they fit in 150 KiB, beyond that in the kNN
 *   workspace (the same device code).  Any k, nlev, a_hi <= 4096.  loc JCH_LOC_DEVICE only enqueues on the ctx stream; otherwise synchronised.
 * jch_lwplsda_predict_prepared -- jch_lwplsr_predict_prepared on a handle whose Ytrain is the n x nlev dummy table of the class codes cls_train
 *   ([n] int32 in 0 .. nlev - 1, [loc] like Zq and Xq): search, `wdist` weights, one weighted `plskern` per query on the dummy columns, then
 *   kind 0 (`plsrda`, src/plsrda.jl:106-114): post = the dummy predictions, code = their first maximum over the LOCAL levels;
 *   kind 1 / 2 (`plslda` / `plsqda`): jch_knn_gda on the local scores, which the local-fit kernel hands out (nlv_lo = 0: JCH_EINVAL).
 *   A class absent from a neighbourhood is a zero response column, also under scal (the reference builds `dummy` on the local levels: the same
 *   fit).  info as above, per (query, nlv); 1 = unanimous neighbourhood (src/locwlv.jl:25-28; not fitted, scores 0); with info 2 code is the
 *   weighted vote of jch_knn_vote.  Requested nlv beyond the local model's clamp.  Results on the HOST: code, info [m][le], post [m][le][nlev],
 *   tloc_out [m][k][nlv_hi] and tq_out [m][nlv_hi] (local scores, may be NULL), ind_out, dist_out, w_out [m][k] (may be NULL).
 *   Outside the envelope of the p-space local-fit kernel (p <= 2048, nlev <= 16, nlv_hi <= 48, its LDS) the fits run one query at a time
 *   (jch_plskern_fit on the local levels' dummy columns, jch_predict, one jch_transform row): slower, never absent. */
JCH_API int32_t jch_knn_gda(jch_ctx *ctx, int32_t loc, const double *T, int64_t m, int32_t k, int32_t a_hi, const double *tq, const int32_t *cls_nb,
                            int32_t nlev, int32_t kind, int32_t prior, int32_t nlv_lo, int32_t nlv_hi, double *post, int32_t *code, int32_t *info);
JCH_API int32_t jch_lwplsda_predict_prepared(jch_ctx *ctx, const jch_lwplsr_model *model, const int32_t *cls_train, int32_t nlev, int32_t kind,
                                             int32_t prior, int32_t loc, const double *Zq, int64_t ldzq, const double *Xq, int64_t m, int64_t ldxq,
                                             int32_t k, double h, double tol, int32_t scal, int32_t nlv_lo, int32_t nlv_hi, int32_t *code,
                                             double *post, int32_t *info, double *tloc_out, double *tq_out, int32_t *ind_out, double *dist_out,
                                             double *w_out);
/* jch_lwplsravg_predict_prepared -- kNN-LWPLSR-AVG (src/lwplsravg.jl, typf = "unif" / "shenk") on a prepared handle: the search and the
 * weights of jch_lwplsr_predict_prepared (the same front end), ONE launch of the p-space local-fit kernel over the level range, the average on the host.
 * The levels are clamped once, as the reference does inside the model of a neighbourhood (n = k): lo = min(nlv_lo, k, p), hi = min(nlv_hi, k, p), for
 * typf = 1 lo = max(lo, 1); le = hi - lo + 1 distinct levels, and every array below is sized with these clamped lo, hi, le.  typf = 0: pred = the mean of
 * the le level predictions in level order.  typf = 1: wlv[a] proportional to 1 / (rss_r[a] rss_b[a]), normalised over lo..hi (what the reference's three
 * `mweight` calls cancel to), pred = sum_a wlv[a] pred_a in level order; rss_r[a - 1] = |xresid| of the query after a local LVs (original scale),
 * rss_b[a - 1] = sqrt((|int|^2 + |B|^2) / q) of the local model with a LVs (src/wshenk.jl:59-67), a = 1..hi.
 *   Zq m x dd or NULL (the handle's query map), Xq m x p [loc].  Results on the HOST: pred [m][q]; each may be NULL: pred_lv [m][le][q], wlv [m][le],
 *   rss_r and rss_b [m][hi] (typf = 1 only), info [m], ind_out / dist_out / w_out [m][k].
 *   info[i] (typf = 1; 0 throughout for typf = 0): 0 = fitted; 1 = a constant univariate y in the neighbourhood (src/locw.jl:34-36): pred = that value, the
 *   wlv and rss rows NaN; 2 = a Shenk norm of lo..hi is 0 or not finite: the reference's arithmetic gives NaN there and so do pred[i] and wlv.
 * Outside the envelope of the p-space kernel (jch_lwplsda_predict_prepared's): JCH_EINVAL with a message naming k, p, q, nlv.  Rank-local on a
 * joined ctx (class L): the ranks are replicas that hold the same handle and split the queries; no collective. */
JCH_API int32_t jch_lwplsravg_predict_prepared(jch_ctx *ctx, const jch_lwplsr_model *model, int32_t loc, const double *Zq, int64_t ldzq, const double *Xq,
                                               int64_t m, int64_t ldxq, int32_t k, double h, double tol, int32_t scal, int32_t nlv_lo, int32_t nlv_hi,
                                               int32_t typf, double *pred, double *pred_lv, double *wlv, double *rss_r, double *rss_b, int32_t *info,
                                               int32_t *ind_out, double *dist_out, double *w_out);

/* ---- Gaussian kernel density estimates: what the reference's `dmkern`, `kdeda` and `plskdeda` evaluate (src/dmkern.jl:151-163,
 * src/kdeda.jl:81-97, src/plskdeda.jl:52-64 with the prediction of src/plslda.jl:107-130) -- DESIGN.md §21.
 * jch_kde_dens -- for the m queries Xq (m x d) against the n training rows Z (n x d) GROUPED BY CLASS (class c owns the rows
 * cls_start[c] .. cls_start[c + 1] - 1; cls_start[0] = 0, cls_start[ncls] = n, no class empty) and nmod nested models:
 *     out[i, c, a] = coef[a, c] * sum_{r in class c} exp(-0.5 * v2[a, c] * sum_{j < dims[a]} ((Xq[i, j] - Z[r, j]) * u[j, c])^2)
 *   The inverse bandwidth of model a, class c, column j is u[j, c] * sqrt(v2[a, c]); dims[a] is the number of leading columns model a
 *   reads, 1 <= dims[0] <= ... <= dims[nmod - 1] <= d (equal values allowed).  One pass over the (query, row) pairs serves every model:
 *   the squared distance over the first dims[a] columns is a running prefix of the one over dims[a + 1]; nothing of size m x n is stored.
 *   Differences are taken before scaling ((x - z) * u, never x * u - z * u) and the sum is a plain sum of `exp` terms, as in the reference:
 *   a query far from every row of a class gives exactly 0.  Fixed summation order, no atomics: the same call gives the same bits.
 *   Z, Xq, out [loc], column-major, ld >= rows; out is m x (ncls * nmod), element (i, c, a) at out[i + ldo * (c + ncls * a)].
 *   cls_start (ncls + 1), u (d x ncls), v2 and coef (nmod x ncls, both column-major: element (a, c) at [a + nmod * c]) and dims (nmod) are
 *   HOST arrays whatever loc is.  Any m, n, d, ncls, nmod >= 1 (ncls <= 65535).  JCH_EINVAL before any device work for a NULL pointer,
 *   ld < rows, dims decreasing or outside [1, d], an empty class, or cls_start not running from 0 to n.  The workspace is the ctx's own
 *   (the X copy a fit left for JCH_REUSE_XCOPY is not touched); the call ends synchronised with the ctx stream. */
JCH_API int32_t jch_kde_dens(jch_ctx *ctx, int32_t loc, const double *Z, int64_t n, int64_t d, int64_t ldz, const double *Xq, int64_t m, int64_t ldq,
                             const int64_t *cls_start, int32_t ncls, const double *u, const double *v2, const double *coef, const int32_t *dims,
                             int32_t nmod, double *out, int64_t ldo);

/* ---- Gaussian discrimination on raw X: what the reference's `matW`, `dmnorm`, `lda`, `qda` and `mahsqchol` compute (src/matW.jl,
 * src/dmnorm.jl:107-143, src/lda.jl:56-77, src/qda.jl:55-79, src/distances.jl:104-126) -- DESIGN.md §24.  All matrices column-major; [loc]: where
 * `loc` says.  Each of the three entries serves one rank only, ends synchronised with the ctx stream, uses the ctx's own workspace (the X copy a
 * fit left for JCH_REUSE_XCOPY is not touched) and returns JCH_EINVAL with a message before any device work for a NULL pointer, a leading
 * dimension smaller than the row count, an empty class, or a cls_start that does not run from 0 to n.  Every output element is a fixed-order sum
 * with no floating-point atomics: the same call gives the same bits, and so do a host and a device input, and an aligned and an unaligned one.
 * jch_class_cov -- class means and within-class covariances of the n x p matrix Z [loc] GROUPED BY CLASS exactly as in jch_kde_dens (cls_start,
 *   ncls + 1 entries, HOST).  ct (ncls x p, ld ncls, HOST, may be NULL): the class means.  Wi ([loc], p x p x ncls, ld p, stride p * p, may be
 *   NULL): cov(Z_c; corrected = false) of every class, from one read-only pass over the rows of the class with the centring in registers; for a
 *   class of ONE row the uncorrected covariance of all n rows (src/matW.jl:54-65; one more pass over Z, made only in that case).  W ([loc], p x p,
 *   ld p, may be NULL) = sum_c (n_c / n) Wi[c], added in class order as src/matW.jl:69-73 does.  With Wi NULL one p x p workspace is reused per
 *   class.  Both triangles of every output are bitwise symmetric.  p <= 32768, ncls <= 65535.
 * jch_gauss_factor -- for f < nfac: S_f = S + f * sstride ([loc], p x p, ld lds; only its lower triangle is read, it is copied to the workspace and
 *   never written) = L L' by the blocked Cholesky of jch_chol_factor; Uinv_f = Uinv + f * ustride ([loc], ld ldu) = L^-T, upper triangular with
 *   exact zeros strictly below the diagonal (the reference's `LinearAlgebra.inv!(cholesky!(Hermitian(S)).U)`, src/dmnorm.jl:120-123); diagU
 *   (p x nfac, HOST) = diag(L): det(S_f) = prod(diagU[:, f])^2; info[f] (HOST) as jch_chol_factor's: 0, or the 1-based column of the first pivot
 *   that is not > 0 -- then Uinv_f and diagU[:, f] are unspecified; it is a result, not an error, and the other factors are not affected.  The call
 *   invalidates the factor a jch_chol_solve of this ctx would be keyed to.  p <= 32768, nfac <= 65535.
 * jch_mahsq_chol -- out[i, c] = sum_j z_j^2,  z_j = sum_{k <= j} (Xq[i, k] - Mu[c, k]) * Uinv_f[k, j],  f = (nfac == 1 ? 0 : c): the squared
 *   Mahalanobis distances of the m rows of Xq ([loc], m x p, ld ldq) to the ncen centres Mu (ncen x p, ld ncen, HOST) under one shared factor
 *   (nfac == 1) or one per centre (nfac == ncen); Uinv as jch_gauss_factor writes it ([loc]); out m x ncen ([loc], ldo >= m).  On the f64 matrix
 *   cores, without an m x p intermediate.  The difference is taken before the product, never x U - mu U.  The strictly lower triangle of Uinv_f is
 *   never read.  A NaN at Xq[i, k] reaches row i of out only; rows >= m of Xq and of out are never read or written.  ncen is meant to be small
 *   (classes, not observations: every centre reads the query rows again): ncen <= 65535, p <= 32768. */
JCH_API int32_t jch_class_cov(jch_ctx *ctx, int32_t loc, const double *Z, int64_t n, int64_t p, int64_t ldz, const int64_t *cls_start, int32_t ncls,
                              double *Wi, double *W, double *ct);
JCH_API int32_t jch_gauss_factor(jch_ctx *ctx, int32_t loc, const double *S, int64_t p, int64_t lds, int64_t sstride, int32_t nfac, double *Uinv,
                                 int64_t ldu, int64_t ustride, double *diagU, int32_t *info);
JCH_API int32_t jch_mahsq_chol(jch_ctx *ctx, int32_t loc, const double *Xq, int64_t m, int64_t p, int64_t ldq, const double *Mu, int32_t ncen,
                               const double *Uinv, int64_t ldu, int64_t ustride, int32_t nfac, double *out, int64_t ldo);

typedef struct jch_profile {
    double fit_ms;        /* device time of the last fit, first kernel -> last kernel (HIP events)   */
    double prologue_ms;   /* weights + means (+ var) + centre/transpose/XtY                           */
    double sweep_ms;      /* sum over LVs of the dominant kernel (fused sweep; plsnipals: sweep+deflate) */
    double smallstate_ms; /* sum over LVs of partial reduce + lv_update (+ all-reduce)                */
    int32_t sweep_launches;
    int32_t nlv;
    double sweep_bytes;   /* algorithmic bytes of ONE dominant-kernel launch          */
    /* ---- cross-GPU all-reduces of the last fit (all zero on one GPU).  RCCL / loopback / stand-alone inbox kernel: HIP
     * events around each call on the ctx stream (so the time includes waiting for the slowest rank); inbox fused into
     * the small-state kernel: wall_clock64 stamps inside that kernel, first peer store -> rank-ordered sum done.  The
     * fused time is part of smallstate_ms, the others sit between the kernels smallstate_ms spans: either way
     * smallstate_ms - collective_ms is the small-state kernels + launch gaps alone. */
    double collective_ms;          /* sum over the LV loop's all-reduces ([zp, tt] per LV; plsnipals: + K)      */
    double prologue_collective_ms; /* sum over the prologue's all-reduces (weights, moments / pivot, XtY)        */
    double collective_wait_ms;     /* inbox only: the part of collective_ms spent polling the peers' flags      */
    int32_t collective_calls;      /* all-reduces inside the LV loop                                            */
    int32_t collective_transport;  /* JCH_TRANSPORT_* of the LV loop's all-reduce                               */
} jch_profile;
#define JCH_TRANSPORT_NONE 0
#define JCH_TRANSPORT_RCCL 1
#define JCH_TRANSPORT_INBOX 2       /* stand-alone single-workgroup inbox kernel (p2p.hip)                       */
#define JCH_TRANSPORT_INBOX_FUSED 3 /* inbox exchange inside the small-state kernel (no launch of its own)       */
#define JCH_TRANSPORT_LOOPBACK 4    /* test harness                                                              */
/* Enable (1) / disable (0) per-kernel HIP-event timing of subsequent fits (adds event records on the
 * ctx stream, no host syncs inside the fit).  enable = N > 1: the plskern-shaped sweeps (Float64 p <= 1024 and bf16) are SAMPLED —
 * an event pair around every N-th launch only, counted across fits (an event record costs the stream about 3 us: 50 of them are
 * 1 % of a cfg2 fit and 6 % of a 125 k-row share); jch_profile then reports sweep_ms = the sampled launches' mean x the launches
 * made, sweep_launches = the launches made; JCH_COUNTER_SWEEPS_TIMED counts the launches actually bracketed. */
JCH_API int32_t jch_ctx_set_profiling(jch_ctx *ctx, int32_t enable);
JCH_API int32_t jch_ctx_get_profile(const jch_ctx *ctx, jch_profile *out);
/* Waits for everything queued on the ctx stream: what a caller of an entry that "only enqueues" (jch_col_median_mad and jch_knn_* with device
 * inputs and outputs) does before it reads the results on another stream or on the host. */
JCH_API int32_t jch_ctx_synchronize(jch_ctx *ctx);

/* jch_ctx_allreduce_probe — diagnostic: all-reduce (sum) the `count` doubles of `vec` (HOST, in/out) `iters` times
 * back to back through ONE named transport and report the average time per all-reduce in microseconds (HIP events on
 * the ctx stream; iteration 0 is a warm-up and excluded when iters > 1).  Every iteration starts from the caller's
 * values, so on return vec = the sum over ranks: a vector of ones comes back as the number of ranks the transport
 * actually reached.  Collective: every rank calls it with the same count / iters / transport.
 *   transport: JCH_TRANSPORT_RCCL (needs jch_ctx_comm_init), JCH_TRANSPORT_INBOX (needs a self-tested inbox; it need
 *   not be enabled), JCH_TRANSPORT_LOOPBACK, or JCH_TRANSPORT_NONE = whatever a fit would use for this message size.
 * This is how bench.py compares RCCL and the inbox on the per-LV message of the fit it times. */
JCH_API int32_t jch_ctx_allreduce_probe(jch_ctx *ctx, int32_t transport, double *vec, int64_t count, int32_t iters,
                                        double *avg_us);

/* Diagnostic counters of a ctx (cumulative since jch_ctx_create).  which = JCH_COUNTER_PIVOT_REFITS: fits whose one-pass
 * ("raw") prologue was repeated on the centred working copy because the sampled pivot turned out to be further than 64
 * sample standard deviations from a column mean (results are those of the centred formulation). */
#define JCH_COUNTER_PIVOT_REFITS 0
/* which = JCH_COUNTER_LOCW_REFITS: queries of jch_lwplsr_predict* that the neighbour-space local-fit kernel flagged as lying more
 * than 64 local standard deviations (along the offset) from the mean of their neighbours — possible because the neighbours are
 * chosen in the score space, not in p-space — and that were refitted by the per-query path (explicit centring). */
#define JCH_COUNTER_LOCW_REFITS 1
/* which = JCH_COUNTER_KNN_SCREENED: queries of jch_lwplsr_predict* whose neighbours were found by the screened search (all (row, query)
 * pairs on the bf16 matrix cores from two-piece operands, an error-bounded bar per query, exact Float64 distances for the survivors;
 * score spaces of <= 62 dimensions, k <= 768, n < 2^26 and enough rows for the bar to be tight — otherwise, and with
 * JCH_KNN_SCREEN=0 in the environment, the exact scan);
 * which = JCH_COUNTER_KNN_SCREEN_REDONE: those of them the screen could not settle (non-finite scores, or more rows within its
 * error bound of the k-th distance than a candidate list holds: ties on a lattice, neighbour distances far below the scores' norms)
 * and the exact scan redid.  Neighbours, their order, distances and weights do not depend on which search ran.  A prepared model
 * (jch_lwplsr_prepare) that sees more than a quarter of a call's queries redone stops screening. */
#define JCH_COUNTER_KNN_SCREENED 2
#define JCH_COUNTER_KNN_SCREEN_REDONE 3
/* which = JCH_COUNTER_XCOPY_REUSED: fits that honoured JCH_REUSE_XCOPY, i.e. took X'D[Yc | 1] from the previous fit's row-major copy */
#define JCH_COUNTER_XCOPY_REUSED 4
/* which = JCH_COUNTER_SWEEPS_TIMED: launches of the plskern-shaped sweep that were bracketed by HIP events (jch_ctx_set_profiling) */
#define JCH_COUNTER_SWEEPS_TIMED 5
JCH_API int32_t jch_ctx_get_counter(const jch_ctx *ctx, int32_t which, int64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* JCHEMO_HIP_H */
