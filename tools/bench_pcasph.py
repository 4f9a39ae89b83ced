"""The Weiszfeld step, colmedspa and pcasph with X on the device (a cloud at level 100, spread 1, 10 % of the rows shifted by 6 along one direction).
One JSON line with HIP-event times, medians of --reps runs after one warm-up; competing routes alternate inside one loop:
  * the fused step: jch_weiszfeld_step with the loop's own guard (one read of X), whole call, and the same minus the median of the n distances
    (timed on its own: jch_col_median_mad on one column), DERIVED; the exact-mode step (guard < 0: one more read);
  * the two-launch route the library offered before: jch_row_resid_ss with k = 0 and shift = mu0, then jch_covsel_pass with the one-column panel u
    (no median in either);
  * the one-read yardstick: jch_transform with one score column;
  * colmedspa at delta 1e-3 and 1e-6 (whole calls, with their step counts) and pcasph at --nlv;
  * the stages that can be timed on their own: the column medians, the Gram pass (jch_xtdx), the transform at --nlv, the MADs of n x nlv scores; the
    distances pass as exact step - guarded step (DERIVED), what is left of pcasph as eigen iteration and the rest (DERIVED).
Run it under a `timeout` of its own, as every GPU step.  Whoever runs it writes the numbers into DESIGN.md §28, the README and
profiles/pcasph_bench.json.

    python tools/bench_pcasph.py [--n N] [--p P] [--nlv A] [--reps R] [--hbm-peak GBS] [--out FILE]
"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--p", type=int, default=500)
ap.add_argument("--nlv", type=int, default=25)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--hbm-peak", type=float, default=8000.0, help="GB/s (MI355X: 8 TB/s)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")
L = J.load()
n, p, nlv = a.n, a.p, a.nlv


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def alt_median_ms(fns, reps):
    """Medians of `reps` timings of every function, the functions taking turns inside one loop (after one warm-up each)."""
    for f in fns:
        f()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            t[k].append(event_ms(f))
    return [float(np.median(v)) for v in t]


g = torch.Generator(device=dev); g.manual_seed(7)
X = J.colmajor_empty(n, p, dev)
k10 = n // 10
dirn = torch.randn(p, dtype=torch.float64, device=dev, generator=g)
dirn = 6.0 * dirn / dirn.norm()
for c0 in range(0, p, 125):               # (in column blocks: no second n x p temporary)
    c1 = min(p, c0 + 125)
    X[:, c0:c1] = torch.randn((n, c1 - c0), dtype=torch.float64, device=dev, generator=g) + 100.0
    X[:k10, c0:c1] += dirn[c0:c1]
torch.cuda.synchronize()
gb = n * p * 8 / 1e9
xa = X.data_ptr()

# ---- the centre of the second step of the loop, and its guard
med = np.empty(p)
ctx.check(L.jch_col_median_mad(ctx._h, 1, xa, n, p, n, med.ctypes.data, None, 0))
mu1, d1, w0_1, h_1, _ = J.weiszfeld_step(X, med, delta=1e-6, ctx=ctx)
guard = 1e-6 * (w0_1 + h_1) * (1.0 + 2.0 ** -40)
mu2 = np.empty(p)
dd = torch.empty(n, dtype=torch.float64, device=dev)
w0, hh, nl = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
torch.cuda.synchronize()


def fused(gd):
    ctx.check(L.jch_weiszfeld_step(ctx._h, 1, xa, n, p, n, mu1.ctypes.data, 1e-6, gd, mu2.ctypes.data, dd.data_ptr(), C.byref(w0), C.byref(hh), C.byref(nl)))


u = torch.empty(n, dtype=torch.float64, device=dev)
outp = torch.empty(p, dtype=torch.float64, device=dev)
wmed = np.empty(1)


def two_launch():
    ctx.check(L.jch_row_resid_ss(ctx._h, 1, xa, n, p, n, mu1.ctypes.data, None, 0, n, None, p, dd.data_ptr()))
    ctx.check(L.jch_covsel_pass(ctx._h, xa, n, p, n, None, u.data_ptr(), 1, n, outp.data_ptr()))
    ctx.check(L.jch_ctx_synchronize(ctx._h))


fused(guard)
u.copy_(1.0 / dd)
torch.cuda.synchronize()
nleft_guarded = nl.value
r1 = np.ones((p, 1), order="F")
T1 = J.colmajor_empty(n, 1, dev)
ones = np.ones(p)
torch.cuda.synchronize()
yard = lambda: ctx.check(L.jch_transform(ctx._h, 1, xa, n, p, n, mu1.ctypes.data, ones.ctypes.data, r1.ctypes.data, 1, T1.data_ptr(), n))   # noqa: E731
dmedian = lambda: ctx.check(L.jch_col_median_mad(ctx._h, 1, dd.data_ptr(), n, 1, n, wmed.ctypes.data, None, 0))                                # noqa: E731
t_fused, t_two, t_yard, t_dmed, t_exact = alt_median_ms([lambda: fused(guard), two_launch, yard, dmedian, lambda: fused(-1.0)], a.reps)

# ---- whole calls
lib_loop = {}
for delta in (1e-3, 1e-6):
    mu = np.empty(p); nit, cvg, hl = C.c_int32(0), C.c_int32(0), C.c_double(0.0)
    call = lambda: ctx.check(L.jch_spatial_median(ctx._h, 1, xa, n, p, n, delta, 1000, mu.ctypes.data, None, C.byref(nit), C.byref(hl), C.byref(cvg)))   # noqa: E731
    lib_loop[delta] = (alt_median_ms([call], a.reps)[0], nit.value, cvg.value)
medians = lambda: ctx.check(L.jch_col_median_mad(ctx._h, 1, xa, n, p, n, med.ctypes.data, None, 0))   # noqa: E731
t_medians = alt_median_ms([medians], a.reps)[0]
fm = J.pcasph(X, nlv=nlv, ctx=ctx)
t_pcasph = alt_median_ms([lambda: J.pcasph(X, nlv=nlv, ctx=ctx)], a.reps)[0]
t_pcasph_mean = alt_median_ms([lambda: J.pcasph(X, nlv=nlv, typc="mean", ctx=ctx)], a.reps)[0]
gram = lambda: ctx.check(L.jch_xtdx(ctx._h, 1, xa, n, p, n, None, None, 0, None, None, med.ctypes.data))   # noqa: E731
Pn = np.asfortranarray(fm.P)
Tn = J.colmajor_empty(n, fm.P.shape[1], dev)
madv, medv = np.empty(fm.P.shape[1]), np.empty(fm.P.shape[1])
torch.cuda.synchronize()
trans = lambda: ctx.check(L.jch_transform(ctx._h, 1, xa, n, p, n, fm.xmeans.ctypes.data, ones.ctypes.data, Pn.ctypes.data, Pn.shape[1], Tn.data_ptr(), n))   # noqa: E731
mads = lambda: ctx.check(L.jch_col_median_mad(ctx._h, 1, Tn.data_ptr(), n, Pn.shape[1], n, medv.ctypes.data, madv.ctypes.data, 0))                          # noqa: E731
t_gram, t_trans, t_mads = alt_median_ms([gram, trans, mads], a.reps)
t_dist = t_exact - t_fused
nit3 = lib_loop[1e-3][1]
t_rest = t_pcasph - (lib_loop[1e-3][0] + t_dist + t_gram + t_trans + t_mads)

res = dict(metric="pcasph", device=torch.cuda.get_device_name(0), n=n, p=p, nlv=nlv, reps=a.reps, x_gb=round(gb, 3), hbm_peak_gbs=a.hbm_peak,
           second_sweep_path=bool(p > 512),
           fused_step_call_ms=round(t_fused, 3), median_of_distances_ms=round(t_dmed, 3),
           fused_step_without_median_ms_derived=round(t_fused - t_dmed, 3),
           fused_step_gbs_derived=round(gb / ((t_fused - t_dmed) * 1e-3), 1), rows_left_out_by_the_guard=nleft_guarded,
           two_launch_route_ms=round(t_two, 3), fused_over_two_launch_derived=round((t_fused - t_dmed) / t_two, 3),
           one_read_yardstick_transform_1col_ms=round(t_yard, 3), exact_step_call_ms=round(t_exact, 3),
           distances_pass_ms_derived_exact_minus_guarded=round(t_dist, 3),
           colmedspa_delta_1e3_ms=round(lib_loop[1e-3][0], 3), colmedspa_delta_1e3_steps=nit3, colmedspa_delta_1e6_ms=round(lib_loop[1e-6][0], 3),
           colmedspa_delta_1e6_steps=lib_loop[1e-6][1], colmedspa_converged=bool(lib_loop[1e-3][2] and lib_loop[1e-6][2]),
           column_medians_ms=round(t_medians, 3), steps_ms_derived_colmedspa_1e3_minus_medians=round(lib_loop[1e-3][0] - t_medians, 3),
           pcasph_ms=round(t_pcasph, 3), pcasph_typc_mean_ms=round(t_pcasph_mean, 3), pcasph_eig_niter=fm.niter, pcasph_converged=bool(fm.converged),
           gram_xtdx_ms=round(t_gram, 3), transform_nlv_ms=round(t_trans, 3), mad_of_scores_ms=round(t_mads, 3),
           eigen_and_rest_ms_derived=round(t_rest, 3))
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
