"""Covsel at n = 1e6, p = 500, q in {1, 10} (device-resident, filled by jch_fill_uniform plus a column offset of 100): one JSON line with
HIP-event times (medians of --reps runs after one warm-up) of
  * the pass on its own, jch_covsel_pass with the panel of a step ([Yd | q_i]: q + 1 columns): ms, algorithmic bytes (n p 8 for X plus
    n (q + 1) 8 for the panel) over time in TB/s, that rate over the 8 TB/s HBM peak and over the fused plskern sweep's 6.9 TB/s
    (DESIGN.md §4).  The interval also holds the entry's copy of the panel into its padded workspace (2 n (q + 1) 8 bytes) and the sum of
    the partials;
  * a whole selection, jch_covsel_fit with nlv = 25 and typ = "cov": ms, ms per step, and the share of it that nlv + 3 passes explain.
The split by kernel comes from a `rocprofv3 --kernel-trace --stats` run of this script (profiles/covsel_kernel_stats.csv).  Run it under
a `timeout` of its own, as every GPU step.  Whoever runs it writes the numbers into DESIGN.md §15 and profiles/covsel_bench.json.

    python tools/bench_covsel.py [--n N] [--p P] [--q Q ...] [--nlv A] [--reps R] [--out FILE]
"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J

HBM_TBS = 8.0      # HBM peak, TB/s
SWEEP_TBS = 6.9    # the fused plskern sweep

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--p", type=int, default=500)
ap.add_argument("--q", type=int, nargs="+", default=[1, 10])
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


X = J.colmajor_empty(n, p, dev)
ctx.check(L.jch_fill_uniform(ctx._h, X.data_ptr(), n, p, n, 0, n, C.c_uint64(7)))
X.add_(100.0)
mu = X.mean(0).contiguous()
runs = []
for q in a.q:
    b = q + 1
    V = J.colmajor_empty(n, b, dev)
    ctx.check(L.jch_fill_uniform(ctx._h, V.data_ptr(), n, b, n, 0, n, C.c_uint64(11)))
    Y = J.colmajor_empty(n, q, dev)
    Y.copy_(X[:, :: max(1, p // q)][:, :q] * 0.5 + V[:, :q])          # Y depends on some columns of X
    out = torch.empty((b, p), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    t_pass = median_ms(lambda: ctx.check(L.jch_covsel_pass(ctx._h, X.data_ptr(), n, p, n, mu.data_ptr(), V.data_ptr(), b, n, out.data_ptr())), a.reps)
    nbytes = 8.0 * n * (p + b)
    rate = nbytes / (t_pass * 1e-3) / 1e12
    sel = np.zeros(nlv, dtype=np.int32)
    done = C.c_int32(0)
    nul = [None] * 11

    def fit():
        ctx.check(L.jch_covsel_fit(ctx._h, J._lib.LOC_DEVICE, X.data_ptr(), n, p, n, Y.data_ptr(), q, n, nlv, 0, 0, sel.ctypes.data, *nul, C.byref(done)))

    t_fit = median_ms(fit, max(1, a.reps // 2))
    res = dict(q=q, panel=b, pass_ms=round(t_pass, 4), pass_tbs=round(rate, 3), share_of_hbm_peak=round(rate / HBM_TBS, 3),
               rate_over_fused_sweep=round(rate / SWEEP_TBS, 3), fit_ms=round(t_fit, 3), nlv=nlv, nlv_out=int(done.value), ms_per_step=round(t_fit / nlv, 4),
               share_explained_by_passes=round((nlv + 3) * t_pass / t_fit, 3), sel=[int(v) for v in sel[:int(done.value)]])
    print(json.dumps(res), flush=True)
    runs.append(res)
    del V, Y, out
line = json.dumps(dict(metric="covsel", device=torch.cuda.get_device_name(0), n=n, p=p, hbm_peak_tbs=HBM_TBS, fused_sweep_tbs=SWEEP_TBS, reps=a.reps, runs=runs))
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
