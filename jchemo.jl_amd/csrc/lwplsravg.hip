// kNN-LWPLSR-AVG (src/lwplsravg.jl with typf = "unif" / "shenk"): jch_lwplsravg_predict_prepared, include/jchemo_hip.h; DESIGN.md §27.
//
// The call goes through the shared query front end (jch_lw_front_check / _stage / _map: the same search, the same weights as every local model), then ONE
// launch of the p-space local-fit kernel k_locw_plskern (lwplsr.hip) over the clamped level range.  typf = 1 takes its SHENK instantiation, which also
// returns, per query and level, the two Shenk norms of src/wshenk.jl:59-67 on the local model; the weights and the average are m x le host arithmetic:
//   wlv[a] = (1 / (rss_r[a] rss_b[a])) / sum over lo..hi     (the reference's three `mweight` calls cancel to this),   pred = sum_a wlv[a] pred_a
// in level order.  typf = 0 is the same kernel without the norms and the mean over the levels.
// The levels are clamped ONCE, here, as the reference does inside the model it fits on a neighbourhood (n = k): lo = min(nlv_lo, k, p),
// hi = min(nlv_hi, k, p), for Shenk lo = max(lo, 1) (src/plsravg_shenk.jl:15-18); le = hi - lo + 1 distinct levels.
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "jch_internal.h"
#include "lwplsr_dev.h"

extern "C" int32_t jch_lwplsravg_predict_prepared(jch_ctx *ctx, const jch_lwplsr_model *model, int32_t loc, const double *Zq, int64_t ldzq, const double *Xq,
                                                  int64_t m, int64_t ldxq, int32_t k, double h, double tol, int32_t scal, int32_t nlv_lo, int32_t nlv_hi,
                                                  int32_t typf, double *pred, double *pred_lv, double *wlv, double *rss_r, double *rss_b, int32_t *info,
                                                  int32_t *ind_out, double *dist_out, double *w_out)
{
    if (!ctx) return JCH_EINVAL;
    const char *who = "jch_lwplsravg_predict_prepared";
    if (!model || !Xq || !pred || ldxq < m || (Zq && ldzq < m)) return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments", who);
    if (typf != 0 && typf != 1) return jch_fail(ctx, JCH_EINVAL, "%s: typf must be 0 (unif) or 1 (shenk), not %d", who, typf);
    JCH_TRY(jch_lw_front_check(ctx, who, model, Zq));
    if (m < 1 || k < 1 || nlv_lo < 0 || nlv_hi < nlv_lo || m >= ((int64_t)1 << 31) - 1) return jch_fail(ctx, JCH_EINVAL, "%s: bad arguments", who);
    if (loc != JCH_LOC_HOST && loc != JCH_LOC_DEVICE) return jch_fail(ctx, JCH_EINVAL, "%s: bad loc", who);
    if (k > model->n) k = (int32_t)model->n;                      // src/getknn.jl:33
    const int64_t n = model->n, p = model->p, dd = model->dd, q = model->q;
    const int kp = (int)std::min<int64_t>(k, p);
    const int hi = std::min(nlv_hi, kp);
    const int lo = typf == 1 ? std::max(std::min(nlv_lo, kp), 1) : std::min(nlv_lo, kp);
    if (hi < lo) return jch_fail(ctx, JCH_EINVAL, "%s: no level left after the clamp (nlv %d .. %d, k = %d, p = %lld)", who, nlv_lo, nlv_hi, k, (long long)p);
    const int le = hi - lo + 1;
    locw_args g;
    g.Xrm = model->Xrm; g.ldr = model->ldr; g.p = (int)p; g.Y = model->Y; g.ldy = n; g.q = (int)q; g.m = (int)m; g.k = k; g.scal = scal;
    g.nlv_lo = lo; g.nlv_hi = hi; g.scratch = nullptr; g.slab = 0; g.flags = nullptr; g.dbg = 0;
    if (!jch_locw_pspace_fits(g))
        return jch_fail(ctx, JCH_EINVAL, "%s: outside the envelope of the p-space local-fit kernel (k = %d, p = %lld, q = %lld, nlv = %d)", who, k, (long long)p,
                        (long long)q, hi);
    JCH_HIP(ctx, hipSetDevice(ctx->device));
    const bool host = loc == JCH_LOC_HOST, shenk = typf == 1;
    const size_t mk = (size_t)m * k, np = (size_t)m * le * (size_t)q, nr = (size_t)m * hi;
    jch_carve cv;
    const size_t o_rr = cv.take(nr), o_rb = cv.take(nr), o_in = cv.take(jch_ints_as_doubles((size_t)m));
    JCH_TRY(jch_reserve(ctx, ctx->gd_ws, sizeof(double) * cv.off + 256));
    JCH_TRY(jch_reserve(ctx, ctx->gemm_out, sizeof(double) * (mk * 2 + np) + sizeof(int) * mk + 256));
    std::vector<double> hp(np), hr(shenk ? nr : 0), hb(shenk ? nr : 0);
    std::vector<int> hin(shenk ? (size_t)m : 0);
    JCH_TRY(jch_synced(ctx, true, [&]() -> int32_t {
        double *ws = (double *)ctx->gd_ws.ptr;
        double *ddist = (double *)ctx->gemm_out.ptr, *dw = ddist + mk, *dpred = dw + mk;
        int *dind = (int *)(dpred + np);
        lw_queries qs{Zq, ldzq, Xq, ldxq};
        JCH_TRY(jch_lw_front_stage(ctx, model, host, m, &qs));
        if (!Zq) JCH_TRY(jch_lw_front_map(ctx, model, m, &qs));
        int *sflags = nullptr;
        JCH_TRY(jch_knn_dispatch(ctx, jch_knn_make_args(model->Zt, n, dd, qs.Zq, qs.ldzq, m, k, h, tol, dind, ddist, dw), model->has_screen ? &model->screen : nullptr,
                                 &model->screen_off, &sflags));
        g.Xq = qs.Xq; g.ldxq = qs.ldxq; g.ind = dind; g.w = dw; g.pred = dpred;
        if (shenk) { g.rss_r = ws + o_rr; g.rss_b = ws + o_rb; g.shenk_info = (int *)(ws + o_in); }
        JCH_TRY(jch_launch_locw_pspace(ctx, g));
        JCH_HIP(ctx, hipGetLastError());
        JCH_HIP(ctx, hipMemcpyAsync(hp.data(), dpred, sizeof(double) * np, hipMemcpyDeviceToHost, ctx->stream));
        if (shenk) {
            JCH_HIP(ctx, hipMemcpyAsync(hr.data(), g.rss_r, sizeof(double) * nr, hipMemcpyDeviceToHost, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(hb.data(), g.rss_b, sizeof(double) * nr, hipMemcpyDeviceToHost, ctx->stream));
            JCH_HIP(ctx, hipMemcpyAsync(hin.data(), g.shenk_info, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        }
        if (ind_out) JCH_HIP(ctx, hipMemcpyAsync(ind_out, dind, sizeof(int) * mk, hipMemcpyDeviceToHost, ctx->stream));
        if (dist_out) JCH_HIP(ctx, hipMemcpyAsync(dist_out, ddist, sizeof(double) * mk, hipMemcpyDeviceToHost, ctx->stream));
        if (w_out) JCH_HIP(ctx, hipMemcpyAsync(w_out, dw, sizeof(double) * mk, hipMemcpyDeviceToHost, ctx->stream));
        return JCH_OK;
    }));
    // the weights and the average: m x le host arithmetic, sums in level order
    const double qnan = __builtin_nan("");
    std::vector<double> wl((size_t)le);
    for (int64_t i = 0; i < m; ++i) {
        const double *pl = hp.data() + (size_t)i * le * q;
        int inf = 0;
        if (!shenk) {
            for (int a = 0; a < le; ++a) wl[(size_t)a] = 1.0 / le;
        } else if (hin[(size_t)i] == 1) {      // constant neighbourhood: every level predicts that value; no model, no norms
            inf = 1;
            for (int a = 0; a < hi; ++a) hr[(size_t)i * hi + a] = hb[(size_t)i * hi + a] = qnan;
        } else {
            double tot = 0.0;
            for (int a = 0; a < le; ++a) {
                const double rr = hr[(size_t)i * hi + (lo - 1 + a)], rb = hb[(size_t)i * hi + (lo - 1 + a)];
                if (!(rr > 0.0) || !(rb > 0.0) || !std::isfinite(rr) || !std::isfinite(rb)) inf = 2;   // the reference's arithmetic gives NaN there
                wl[(size_t)a] = 1.0 / (rr * rb);
                tot += wl[(size_t)a];
            }
            for (int a = 0; a < le; ++a) wl[(size_t)a] = inf == 2 ? qnan : wl[(size_t)a] / tot;
        }
        for (int64_t y = 0; y < q; ++y) {
            double acc;
            if (inf == 1) acc = pl[y];
            else if (!shenk) {
                acc = pl[y];
                for (int a = 1; a < le; ++a) acc += pl[(size_t)a * q + y];
                if (le > 1) acc /= le;
            } else {
                acc = wl[0] * pl[y];
                for (int a = 1; a < le; ++a) acc += wl[(size_t)a] * pl[(size_t)a * q + y];
            }
            pred[(size_t)i * q + y] = acc;
        }
        if (wlv) for (int a = 0; a < le; ++a) wlv[(size_t)i * le + a] = inf == 1 ? qnan : wl[(size_t)a];
        if (info) info[i] = inf;
    }
    if (pred_lv) std::copy(hp.begin(), hp.end(), pred_lv);
    if (shenk && rss_r) std::copy(hr.begin(), hr.end(), rss_r);
    if (shenk && rss_b) std::copy(hb.begin(), hb.end(), rss_b);
    return JCH_OK;
}
