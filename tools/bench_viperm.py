"""Permutation importance at n in {1e5, 1e6}, p = 500, q = 1, psamp = 1/3 (device-resident, filled by jch_fill_uniform): one JSON line with,
per n,
  * jch_perm_score_sums with generated and with explicit permutations (HIP events, medians of --reps runs after one warm-up): ms, the bytes of
    X the pass has to fetch (m p 8: every held-out value once, however often the gather asks for it) over time in TB/s, that rate over the 8 TB/s
    HBM peak;
  * the one-read yardstick in the same run: jch_transform with one score column on the first m rows of the same X (the same m p 8 bytes, streamed,
    no gather), its ms and rate, and the ratio pass / yardstick;
  * one whole `viperm` replication (plskern, nlv = 15, rmsep) by the fast route and by route = "loop" (wall clock around the synchronised calls:
    both hold host work).  The loop is the reference's route on this GPU through the library's own `predict`; it is timed on --loop-cols columns
    and scaled to p, as tools/bench_knn.py does for its yardstick.
Run it under a `timeout` of its own, as every GPU step.  Whoever runs it writes the numbers into DESIGN.md §26 and profiles/viperm_bench.json.

    python tools/bench_viperm.py [--n N ...] [--p P] [--q Q] [--nlv A] [--reps R] [--loop-cols C] [--out FILE]
"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J

HBM_TBS = 8.0      # HBM peak, TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[100000, 1000000])
ap.add_argument("--p", type=int, default=500)
ap.add_argument("--q", type=int, default=1)
ap.add_argument("--nlv", type=int, default=15)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-cols", type=int, default=8)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")
L = J.load()
VPM = sys.modules["jchemo_hip.viperm"]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, reps):
    fn()                                  # warm-up: workspace growth, first-launch costs
    return float(np.median([event_ms(fn) for _ in range(reps)]))


def wall_ms(fn, reps):
    out = []
    for _ in range(reps + 1):
        torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out[1:]))


runs = []
p, q = a.p, a.q
for n in a.n:
    X = J.colmajor_empty(n, p, dev)
    ctx.check(L.jch_fill_uniform(ctx._h, X.data_ptr(), n, p, n, 0, n, C.c_uint64(7)))
    E = J.colmajor_empty(n, q, dev)
    ctx.check(L.jch_fill_uniform(ctx._h, E.data_ptr(), n, q, n, 0, n, C.c_uint64(11)))
    Y = J.colmajor_empty(n, q, dev)
    Y.copy_(X[:, :: max(1, p // (4 * q))][:, :q] * 2.0 + X[:, 3:3 + q] + 0.1 * E)        # Y depends on some columns of X
    m = int(round(n / 3))
    rows, pseed = VPM._splits(n, m, 1, 20260103, None)[0]
    rows_d = torch.as_tensor(rows).to(dev)
    w = torch.ones(n, dtype=torch.float64, device=dev); w[rows_d] = 0.0
    fm = J.plskern(X, Y, w, nlv=a.nlv, ctx=ctx)
    pred = J.predict(fm, X, ctx=ctx)
    B = np.asfortranarray(J.coef(fm)[0])
    perm_d = J.perm_fill(m, p, pseed, device=dev, ctx=ctx)
    sums = np.empty((p + 1, q, 6))
    torch.cuda.synchronize()

    def pass_(pm):
        ctx.check(L.jch_perm_score_sums(ctx._h, J._lib.LOC_DEVICE, X.data_ptr(), n, p, n, rows_d.data_ptr(), m, pred.data_ptr(), n, Y.data_ptr(), q, n,
                                        B.ctypes.data, p, pm, m, C.c_uint64(pseed), sums.ctypes.data))

    t_gen = median_ms(lambda: pass_(None), a.reps)
    s_gen = sums.copy()
    t_exp = median_ms(lambda: pass_(perm_d.data_ptr()), a.reps)
    same = bool(np.array_equal(s_gen, sums))
    out1 = J.colmajor_empty(m, 1, dev)
    R1 = np.asfortranarray(fm.R[:, :1]); xm = np.ascontiguousarray(fm.xmeans); xs = np.ascontiguousarray(fm.xscales)
    t_tr = median_ms(lambda: ctx.check(L.jch_transform(ctx._h, J._lib.LOC_DEVICE, X.data_ptr(), m, p, n, xm.ctypes.data, xs.ctypes.data, R1.ctypes.data, 1,
                                                       out1.data_ptr(), m)), a.reps)
    nbytes = 8.0 * m * p
    tbs = lambda ms: nbytes / (ms * 1e-3) / 1e12  # noqa: E731
    kw = dict(nlv=a.nlv)
    t_fast = wall_ms(lambda: VPM._fast_replication(X, Y, rows, pseed, "rmsep", J.plskern, ctx, kw, True), a.reps)
    nc = min(a.loop_cols, p)
    t_loop0 = wall_ms(lambda: VPM._loop_replication(X, Y, rows, pseed, J.rmsep, J.plskern, ctx, kw, cols=[]), 2)
    t_loopc = wall_ms(lambda: VPM._loop_replication(X, Y, rows, pseed, J.rmsep, J.plskern, ctx, kw, cols=list(range(nc))), 2)
    per_col = (t_loopc - t_loop0) / nc
    res = dict(n=n, p=p, q=q, m=m, column_bytes=8 * n, pass_generated_ms=round(t_gen, 4), pass_explicit_ms=round(t_exp, 4), explicit_equals_generated=same,
               pass_generated_tbs=round(tbs(t_gen), 3), pass_explicit_tbs=round(tbs(t_exp), 3), explicit_share_of_hbm_peak=round(tbs(t_exp) / HBM_TBS, 3),
               generated_share_of_hbm_peak=round(tbs(t_gen) / HBM_TBS, 3), transform_ms=round(t_tr, 4), transform_tbs=round(tbs(t_tr), 3),
               transform_share_of_hbm_peak=round(tbs(t_tr) / HBM_TBS, 3), explicit_over_transform=round(t_exp / t_tr, 2), generated_over_transform=round(t_gen / t_tr, 2),
               replication_fast_ms=round(t_fast, 2), loop_fixed_ms=round(t_loop0, 2), loop_cols_timed=nc, loop_ms_per_column=round(per_col, 3),
               replication_loop_ms_scaled=round(t_loop0 + per_col * p, 1), loop_over_fast=round((t_loop0 + per_col * p) / t_fast, 1), nlv=a.nlv)
    print(json.dumps(res), flush=True)
    runs.append(res)
    del X, Y, E, pred, perm_d, w, out1
    torch.cuda.empty_cache()
line = json.dumps(dict(metric="viperm", device=torch.cuda.get_device_name(0), hbm_peak_tbs=HBM_TBS, reps=a.reps, runs=runs))
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
