"""Outlier distances at n = 1e6, p = 500, nlv = 25 with X on the device: X = H B + 100 + noise with a decaying spectrum (32 factors, 0.85^k), a
pcasvd model fitted on it.  One JSON line with HIP-event times of whole calls, medians of --reps runs after one warm-up, of
  * jch_row_resid_ss alone (scores given), in ms and GB/s of X read, with k = nlv and with k = 0;
  * jch_transform alone on the same X: the yardstick for a one-read pass (k_affine_gemm32p), in the same units;
  * the squared orthogonal distances by the new route (transform, then jch_row_resid_ss: two reads of X) and, in runs that ALTERNATE with it in
    the same process, by the parent commit's route (`xresid`, an m x p matrix from a p x p device GEMM, then `(E * E).sum(1)`), their ratio and
    the largest relative difference between the two results;
  * occod and occsdod, fit and predict.
Run it under a `timeout` of its own, as every GPU step.  Whoever runs it writes the numbers into DESIGN.md §17, the README and
profiles/occ_bench.json.

    python tools/bench_occ.py [--n N] [--p P] [--nlv A] [--reps R] [--out FILE]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--p", type=int, default=500)
ap.add_argument("--nlv", type=int, default=25)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")
L = J.load()
n, p, nlv = a.n, a.p, min(a.nlv, a.p)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, reps):
    fn()                                  # warm-up: workspace growth, first-launch costs
    return float(np.median([event_ms(fn) for _ in range(reps)]))


g = torch.Generator(device=dev); g.manual_seed(7)
r = 32
X = J.colmajor_empty(n, p, dev)
H = torch.randn((n, r), dtype=torch.float64, device=dev, generator=g) * (0.85 ** torch.arange(r, dtype=torch.float64, device=dev))
B = torch.linalg.qr(torch.randn((p, r), dtype=torch.float64, device=dev, generator=g))[0].t().contiguous()
for c0 in range(0, p, 125):               # (in column blocks: no second n x p temporary)
    c1 = min(p, c0 + 125)
    X[:, c0:c1] = H @ B[:, c0:c1] + 100.0 + 1e-3 * torch.randn((n, c1 - c0), dtype=torch.float64, device=dev, generator=g)
del H
torch.cuda.synchronize()
fm = J.pcasvd(X, nlv=nlv, ctx=ctx)
k = fm.P.shape[1]
gb = n * p * 8 / 1e9

# the primitive alone, through the C ABI, and the one-read yardstick
T = J.transform(fm, X, ctx=ctx)
Ps = np.asfortranarray(fm.xscales[:, None] * fm.P)
xm, xs, R = np.ascontiguousarray(fm.xmeans), np.ascontiguousarray(fm.xscales), np.asfortranarray(fm.P)
out = torch.empty(n, dtype=torch.float64, device=dev)
Tq = J.colmajor_empty(n, k, dev)
torch.cuda.synchronize()
prim = lambda: ctx.check(L.jch_row_resid_ss(ctx._h, 1, X.data_ptr(), n, p, n, xm.ctypes.data, T.data_ptr(), k, n, Ps.ctypes.data, p, out.data_ptr()))   # noqa: E731
prim0 = lambda: ctx.check(L.jch_row_resid_ss(ctx._h, 1, X.data_ptr(), n, p, n, xm.ctypes.data, None, 0, 0, None, p, out.data_ptr()))                      # noqa: E731
trans = lambda: ctx.check(L.jch_transform(ctx._h, 1, X.data_ptr(), n, p, n, xm.ctypes.data, xs.ctypes.data, R.ctypes.data, k, Tq.data_ptr(), n))          # noqa: E731
prim(); trans()
tp, tt = [], []
for _ in range(a.reps):                    # alternating runs on one box
    tp.append(event_ms(prim)); tt.append(event_ms(trans))
t_prim, t_trans = float(np.median(tp)), float(np.median(tt))
t_prim0 = median_ms(prim0, a.reps)

# the squared orthogonal distances: the new route against the parent commit's, alternating
new_route = lambda: J.row_resid_ss(X, fm.xmeans, J.transform(fm, X, ctx=ctx), Ps, ctx=ctx)                       # noqa: E731


def parent_route():
    E = J.xresid(fm, X, ctx=ctx)
    return (E * E).sum(1)


d_new, d_par = new_route(), parent_route()
agree = float(torch.max(torch.abs(d_new - d_par) / d_par))
del d_new, d_par
tn, to = [], []
for _ in range(a.reps):
    tn.append(event_ms(new_route)); to.append(event_ms(parent_route))
t_new, t_par = float(np.median(tn)), float(np.median(to))
torch.cuda.empty_cache()

reps2 = max(1, a.reps // 2 + 1)
t_od_fit = median_ms(lambda: J.occod(fm, X, ctx=ctx), reps2)
od = J.occod(fm, X, ctx=ctx)
t_od_pred = median_ms(lambda: J.predict(od, X, ctx=ctx), reps2)
t_sd_fit = median_ms(lambda: J.occsd(fm, ctx=ctx), reps2)
t_sdod_fit = median_ms(lambda: J.occsdod(fm, X, ctx=ctx), reps2)
sdod = J.occsdod(fm, X, ctx=ctx)
t_sdod_pred = median_ms(lambda: J.predict(sdod, X, ctx=ctx), reps2)

res = dict(metric="occ", device=torch.cuda.get_device_name(0), n=n, p=p, nlv=k, reps=a.reps, x_gb=round(gb, 3),
           row_resid_ss_ms=round(t_prim, 3), row_resid_ss_gbs=round(gb / (t_prim * 1e-3), 1),
           row_resid_ss_k0_ms=round(t_prim0, 3), row_resid_ss_k0_gbs=round(gb / (t_prim0 * 1e-3), 1),
           transform_ms=round(t_trans, 3), transform_gbs=round(gb / (t_trans * 1e-3), 1), read_rate_over_transform=round(t_trans / t_prim, 3),
           od2_new_route_ms=round(t_new, 3), od2_parent_route_ms=round(t_par, 3), parent_over_new=round(t_par / t_new, 2),
           parent_route="xresid (p x p device GEMM, m x p output), then (E * E).sum(1)", max_rel_diff_new_vs_parent=agree,
           occod_fit_ms=round(t_od_fit, 3), occod_predict_ms=round(t_od_pred, 3), occsd_fit_ms=round(t_sd_fit, 3),
           occsdod_fit_ms=round(t_sdod_fit, 3), occsdod_predict_ms=round(t_sdod_pred, 3))
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
