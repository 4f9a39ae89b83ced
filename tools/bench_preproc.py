"""Spectra preprocessing at n = 1e6 x p = 500 and n = 2.5e5 x p = 2000 (device-resident, filled by jch_fill_uniform plus a per-row offset):
one JSON line with HIP-event times (medians of --reps runs after one warm-up) of snv_, detrend_, savgol_(21, 3, 2), mavg_(11) and
fdif(2), each next to a same-size device-to-device hipMemcpyAsync timed in the same process in alternation — the yardstick: independent
of the code under test, one read and one write of the matrix.  The events bracket the C entry (jch_rows_*) with the host-side
coefficients built beforehand, so the interval holds the entry's own small upload and its launch but neither numpy's pinv / inv nor
the Python plumbing.  Per function: ms, algorithmic bytes (2 n p 8; fdif n (2 p - 1) 8) over time in TB/s, that rate over the 8 TB/s
HBM peak and over the copy's rate.  --host-rows N also times the numpy restatements (tests/test_preproc_static.py) on N rows on the
host, scaled to n (context only).  The split by kernel comes from a `rocprofv3 --kernel-trace --stats` run of this script
(profiles/preproc_kernel_stats.csv).  Run it under a `timeout` of its own, as every GPU step.

    python tools/bench_preproc.py [--shapes N,P ...] [--reps R] [--host-rows N] [--only NAME ...] [--out FILE]
"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd"), os.path.join(ROOT, "tests")]
import numpy as np, torch
import jchemo_hip as J

HBM_TBS = 8.0     # HBM peak, TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", nargs="+", default=["1000000,500", "250000,2000"])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--host-rows", type=int, default=0)
ap.add_argument("--only", nargs="+", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")
L = J.load()


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


rows = []
for shape in a.shapes:
    n, p = (int(v) for v in shape.split(","))
    X = J.colmajor_empty(n, p, dev)
    B = J.colmajor_empty(n, p, dev)      # the copy's destination

    def refill():
        ctx.check(L.jch_fill_uniform(ctx._h, X.data_ptr(), n, p, n, 0, n, C.c_uint64(7)))
        X.add_((torch.arange(n, device=dev, dtype=torch.float64) % 7).mul_(50.0).unsqueeze(1))
        torch.cuda.synchronize()

    def copy():
        B.t().copy_(X.t())               # both contiguous as p x n: one hipMemcpyAsync device to device

    nb = 2.0 * n * p * 8
    # the C entries themselves, with the host-side coefficients built beforehand (what preproc.py hands over): the interval holds the
    # entry's small upload of them and its launch, not numpy's pinv / inv nor the Python plumbing
    from jchemo_hip import preproc as P
    A, V = P._detrend_coef(p, 1)
    sg, sg_lo = P._savgol_taps(P.savgk(10, 3, 2).kern)
    ma, ma_lo = P._mavg_window(11)
    fd = np.array([-1.0, 1.0])
    xp, bp, DEV = X.data_ptr(), B.data_ptr(), J._lib.LOC_DEVICE

    def fir(taps, lo, mode, out):
        return lambda: ctx.check(L.jch_rows_fir(ctx._h, DEV, xp, n, p, n, taps.ctypes.data, len(taps), lo, mode, out, n))

    funs = dict(snv_=(lambda: ctx.check(L.jch_rows_standardize(ctx._h, DEV, xp, n, p, n, 1, 1, xp, n)), nb),
                detrend_=(lambda: ctx.check(L.jch_rows_project_out(ctx._h, DEV, xp, n, p, n, A.ctypes.data, V.ctypes.data, 2, xp, n)), nb),
                savgol_=(fir(sg, sg_lo, P.FIR_SAME, xp), nb), mavg_=(fir(ma, ma_lo, P.FIR_SAME, xp), nb),
                fdif=(fir(fd, 0, P.FIR_VALID, bp), (2.0 * p - 1) * n * 8))   # (its n x (p - 1) output goes into the copy's destination)
    res = dict(n=n, p=p, reps=a.reps)
    samples = {}
    for name, (fn, nbytes) in funs.items():
        if a.only and name not in a.only:
            continue
        tf, tc = [], []
        for it in range(a.reps + 1):     # the first round is the warm-up (workspace growth, first-launch costs)
            refill()
            t_copy = event_ms(copy)
            t_fun = event_ms(fn)
            if it:
                tc.append(t_copy); tf.append(t_fun)
        mf, mc = float(np.median(tf)), float(np.median(tc))
        rate, crate = nbytes / (mf * 1e-3) / 1e12, nb / (mc * 1e-3) / 1e12
        res[name] = dict(ms=round(mf, 4), tbs=round(rate, 3), share_of_hbm_peak=round(rate / HBM_TBS, 3), copy_ms=round(mc, 4), copy_tbs=round(crate, 3),
                         rate_over_copy=round(rate / crate, 3))
        samples[name] = dict(fun=[round(t, 4) for t in tf], copy=[round(t, 4) for t in tc])
        print(name, json.dumps(res[name]), flush=True)
    res["samples"] = samples
    if a.host_rows:
        from test_preproc_static import np_detrend, np_fdif, np_mavg, np_savgol, np_snv
        m = min(a.host_rows, n)
        refill()
        H = np.asfortranarray(X[:m].cpu().numpy())
        host = {}
        for name, fn in (("snv_", lambda: np_snv(H)), ("detrend_", lambda: np_detrend(H)), ("savgol_", lambda: np_savgol(H, 21, 3, 2)),
                         ("mavg_", lambda: np_mavg(H, 11)), ("fdif", lambda: np_fdif(H))):
            t0 = time.perf_counter(); fn(); host[name] = round((time.perf_counter() - t0) * n / m, 2)
        res["numpy_restatement_s_scaled_to_n"] = dict(rows_timed=m, **host)
    rows.append(res)
    del X, B
    torch.cuda.empty_cache()
line = json.dumps(dict(metric="preproc_rows", device=torch.cuda.get_device_name(0), hbm_peak_tbs=HBM_TBS, runs=rows))
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
