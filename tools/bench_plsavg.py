"""Model averaging at n = 1e6, p = 500, levels 1..25 with X on the device: X = H B + 100 + noise with a decaying spectrum (32 factors, 0.85^k), a
univariate y on the first factors, a plskern model fitted on them.  One JSON line with HIP-event times of whole calls, medians of --reps runs
after one warm-up, of
  (a) jch_row_resid_ss_lv for the levels 1..nlv in ms and GB/s of X read, and, in runs that ALTERNATE with it in the same process, the parent
      commit's only route to the same numbers (nlv calls of jch_row_resid_ss with k = 1..nlv) and jch_transform with nlv columns, the one-read
      yardstick; the largest relative difference between the two routes' results; the vector-pipe work 4 n p nlv flop over the kernel's time;
  (b) a whole `wshenk` and a whole `plsravg` shenk predict ("1:nlv");
  (c) `lwplsravg` unif and shenk predict at n = 1e5, k = 200, nlv "5:15", 1000 queries against `lwplsr_predict` over the same levels with
      JCH_LOCW_KSPACE=0 (and with the default kernel), host clock around whole calls.
Run it under a `timeout` of its own, as every GPU step.  Whoever runs it writes the numbers into DESIGN.md §27, the README and
profiles/plsavg_bench.json.

    python tools/bench_plsavg.py [--n N] [--p P] [--nlv A] [--reps R] [--out FILE]
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
ap.add_argument("--local-n", dest="local_n", type=int, default=100000)
ap.add_argument("--queries", type=int, default=1000)
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


g = torch.Generator(device=dev); g.manual_seed(7)
r = 32
X = J.colmajor_empty(n, p, dev)
H = torch.randn((n, r), dtype=torch.float64, device=dev, generator=g) * (0.85 ** torch.arange(r, dtype=torch.float64, device=dev))
B = torch.linalg.qr(torch.randn((p, r), dtype=torch.float64, device=dev, generator=g))[0].t().contiguous()
for c0 in range(0, p, 125):               # (in column blocks: no second n x p temporary)
    c1 = min(p, c0 + 125)
    X[:, c0:c1] = H @ B[:, c0:c1] + 100.0 + 1e-3 * torch.randn((n, c1 - c0), dtype=torch.float64, device=dev, generator=g)
y = J.colmajor_empty(n, 1, dev)
y[:, 0] = H[:, :8] @ torch.linspace(1.0, 0.3, 8, dtype=torch.float64, device=dev) + 0.01 * torch.randn(n, dtype=torch.float64, device=dev, generator=g)
del H
torch.cuda.synchronize()
fm = J.plskern(X, y, nlv=nlv, ctx=ctx)
k = fm.P.shape[1]
gb = n * p * 8 / 1e9

# (a) the primitive through the C ABI, the parent's route and the one-read yardstick, alternating
T = J.transform(fm, X, ctx=ctx)
Ps = np.asfortranarray(fm.xscales[:, None] * fm.P)
xm, xs, R = np.ascontiguousarray(fm.xmeans), np.ascontiguousarray(fm.xscales), np.asfortranarray(fm.R)
out_lv = J.colmajor_empty(n, k, dev)
out_25 = J.colmajor_empty(n, k, dev)
Tq = J.colmajor_empty(n, k, dev)
torch.cuda.synchronize()
nested = lambda: ctx.check(L.jch_row_resid_ss_lv(ctx._h, 1, X.data_ptr(), n, p, n, xm.ctypes.data, T.data_ptr(), k, n, Ps.ctypes.data, p, 1, k,   # noqa: E731
                                                 out_lv.data_ptr(), n))


def calls_25():
    for lv in range(1, k + 1):
        ctx.check(L.jch_row_resid_ss(ctx._h, 1, X.data_ptr(), n, p, n, xm.ctypes.data, T.data_ptr(), lv, n, Ps.ctypes.data, p,
                                     out_25.data_ptr() + 8 * n * (lv - 1)))


trans = lambda: ctx.check(L.jch_transform(ctx._h, 1, X.data_ptr(), n, p, n, xm.ctypes.data, xs.ctypes.data, R.ctypes.data, k, Tq.data_ptr(), n))   # noqa: E731
nested(); calls_25(); trans()
agree = float(torch.max(torch.abs(out_lv - out_25) / out_25))
tn, tc, tt = [], [], []
for _ in range(a.reps):
    tn.append(event_ms(nested)); tc.append(event_ms(calls_25)); tt.append(event_ms(trans))
t_nested, t_calls, t_trans = (float(np.median(v)) for v in (tn, tc, tt))
del out_lv, out_25, Tq, T
torch.cuda.empty_cache()

# (b) the whole calls of the mirror
w_fn = lambda: J.wshenk(fm, X, ctx=ctx)                                                                        # noqa: E731
avg = J.Plsravg(J.PlsravgShenk(fm, range(1, k + 1)))
p_fn = lambda: J.predict(avg, X, ctx=ctx)                                                                      # noqa: E731
w_fn(); p_fn()
tw, tp = [], []
for _ in range(a.reps):
    tw.append(event_ms(w_fn)); tp.append(event_ms(p_fn))
t_wshenk, t_pred = float(np.median(tw)), float(np.median(tp))

# (c) the local models: `lwplsravg` unif (one batched local-fit call, then the mean of the levels) and shenk (one
# jch_lwplsravg_predict_prepared: the p-space kernel with its Shenk outputs) against `lwplsr_predict` over the same levels with JCH_LOCW_KSPACE=0, whole
# calls with host results, host clock around a call that ends synchronised
import time
del X, y
torch.cuda.empty_cache()
nl, ml, kl, lv = a.local_n, a.queries, 200, "5:15"
rl = 30
Sl = torch.randn((nl + ml, rl), dtype=torch.float64, device=dev, generator=g)
Xa = J.colmajor_empty(nl + ml, p, dev)
Xa.copy_(Sl @ torch.randn((rl, p), dtype=torch.float64, device=dev, generator=g) + 0.1 * torch.randn((nl + ml, p), dtype=torch.float64, device=dev, generator=g))
ya = J.colmajor_empty(nl + ml, 1, dev)
ya[:, 0] = Sl[:, :5] @ torch.tensor([1.0, -2.0, 0.5, 3.0, 1.5], dtype=torch.float64, device=dev) + torch.sin(Sl[:, 5]) + 0.05 * torch.randn(nl + ml, dtype=torch.float64, device=dev, generator=g)
Xl = J.colmajor_empty(nl, p, dev); Xl.copy_(Xa[:nl]); yl = J.colmajor_empty(nl, 1, dev); yl.copy_(ya[:nl]); Xlq = J.colmajor_empty(ml, p, dev); Xlq.copy_(Xa[nl:])
del Xa, ya, Sl
lkw = dict(nlvdis=20, metric="mahal", h=1.0, k=kl)
f_lw = J.lwplsr(Xl, yl, nlv=15, ctx=ctx, **lkw)
f_un = J.lwplsravg(Xl, yl, nlv=lv, typf="unif", ctx=ctx, **lkw)
f_sh = J.lwplsravg(Xl, yl, nlv=lv, typf="shenk", ctx=ctx, **lkw)


def wall_ms(fn, reps):
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), [round(v, 2) for v in out]


def lw_pspace():
    os.environ["JCH_LOCW_KSPACE"] = "0"
    try:
        return J.predict(f_lw, Xlq, nlv=range(5, 16), ctx=ctx)
    finally:
        del os.environ["JCH_LOCW_KSPACE"]


t_lw_p, all_lw_p = wall_ms(lw_pspace, a.reps)
t_lw, all_lw = wall_ms(lambda: J.predict(f_lw, Xlq, nlv=range(5, 16), ctx=ctx), a.reps)
t_un, all_un = wall_ms(lambda: J.predict(f_un, Xlq, ctx=ctx), a.reps)
t_sh, all_sh = wall_ms(lambda: J.predict(f_sh, Xlq, ctx=ctx), 3)

flop = 4.0 * n * p * k
res = dict(metric="plsavg", device=torch.cuda.get_device_name(0), n=n, p=p, nlv=k, reps=a.reps, x_gb=round(gb, 3),
           resid_lv_ms=round(t_nested, 3), resid_lv_gbs=round(gb / (t_nested * 1e-3), 1), resid_lv_tflops=round(flop / (t_nested * 1e-3) / 1e12, 2),
           resid_lv_ms_all=[round(v, 3) for v in tn],
           resid_ss_calls=k, resid_ss_calls_ms=round(t_calls, 3), resid_ss_calls_ms_all=[round(v, 3) for v in tc],
           calls_over_nested=round(t_calls / t_nested, 2), max_rel_diff_nested_vs_calls=agree,
           transform_ms=round(t_trans, 3), transform_gbs=round(gb / (t_trans * 1e-3), 1), nested_over_transform=round(t_nested / t_trans, 2),
           wshenk_ms=round(t_wshenk, 3), plsravg_shenk_predict_ms=round(t_pred, 3),
           local=dict(n=nl, p=p, k=kl, nlv=lv, queries=ml, timing="host clock around whole calls, host results, median",
                      lwplsr_predict_pspace_ms=round(t_lw_p, 2), lwplsr_predict_pspace_ms_all=all_lw_p,
                      lwplsr_predict_default_ms=round(t_lw, 2), lwplsr_predict_default_ms_all=all_lw,
                      lwplsravg_unif_ms=round(t_un, 2), lwplsravg_unif_ms_all=all_un,
                      lwplsravg_shenk_ms=round(t_sh, 2), lwplsravg_shenk_ms_all=all_sh, lwplsravg_shenk_reps=3,
                      shenk_route="one jch_lwplsravg_predict_prepared: the p-space local-fit kernel with its Shenk outputs",
                      pspace_regression="tools/bench_lwplsr.py with JCH_LOCW_KSPACE=0, this build and the parent commit's alternating: profiles/README.md"))
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
