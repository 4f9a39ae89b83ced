"""The PDS transform (`predict(::CalPds, X)` as one jch_rows_fir call in mode JCH_FIR_SAME | JCH_FIR_PER_COLUMN) at n = 1e6 x p = 500,
device-resident, for the half-windows m in {2, 5, 10}: one JSON line with HIP-event times (medians of --reps runs after one warm-up
round; every variant in this one process, the order reversed every other round) of

    pass_out / pass_in   the per-column pass out of place and in place (the C entry with the table built beforehand);
    same_out / same_in   yardstick (a): jch_rows_fir in JCH_FIR_SAME with ONE window of the same f = 2m + 1 at the same shape — the
                         one-read-one-write floor of this access pattern;
    gemm_loop            yardstick (b): the route without the mode, one jch_affine_gemm per output column on its column window, timed
                         on the first --loop-rows rows (default 1e5) of the same matrix and scaled to n (said so in the output);

and the wall-clock time of a whole `calpds` fit at 64 standards with `mlrpinv` and with `plskern, nlv = 1` (host arrays, median of 3).
Reported: pass / (a) and (b) / pass per m.  `not_measured` lists what this script does not establish.  Run it under a `timeout` of its
own, as every GPU step.

    python tools/bench_caltransfer.py [--n N] [--p P] [--ms 2 5 10] [--reps R] [--loop-rows N] [--out FILE]   (default: profiles/caltransfer_bench.json)
"""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J
from jchemo_hip import caltransfer as CT

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--p", type=int, default=500)
ap.add_argument("--ms", type=int, nargs="+", default=[2, 5, 10])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--loop-rows", type=int, default=100000)
ap.add_argument("--standards", type=int, default=64)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "caltransfer_bench.json"))
a = ap.parse_args()
n, p = a.n, a.p
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")
L = J.load()
DEV = J._lib.LOC_DEVICE
X, B = J.colmajor_empty(n, p, dev), J.colmajor_empty(n, p, dev)
ctx.check(L.jch_fill_uniform(ctx._h, X.data_ptr(), n, p, n, 0, n, C.c_uint64(7)))
torch.cuda.synchronize()
xp, bp = X.data_ptr(), B.data_ptr()


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def pds_like(m, rng):
    """A table with the zero pattern of a PDS model: positive taps summing to one per column (a repeated in-place pass stays bounded)."""
    _, s = CT.pds_windows(p, m)
    coefs = []
    for si in s:
        b = rng.uniform(0.5, 1.0, len(si))
        coefs.append((b / b.sum(), np.array([0.01])))
    return CT.pds_table(coefs, s, m) + (s, coefs)


res = dict(n=n, p=p, reps=a.reps, loop_rows=min(a.loop_rows, n))
rng = np.random.default_rng(11)
for m in a.ms:
    tab, f, lo, s, coefs = pds_like(m, rng)
    uni = np.ascontiguousarray(tab[:f, p // 2])
    rows = res["loop_rows"]

    def fir(taps, mode, out):
        return lambda: ctx.check(L.jch_rows_fir(ctx._h, DEV, xp, n, p, n, taps.ctypes.data, f, lo, mode, out, n))

    gemm_args = [(xp + 8 * n * int(si[0]), len(si), np.asfortranarray(b.reshape(-1, 1)), c, bp + 8 * n * i) for i, (si, (b, c)) in enumerate(zip(s, coefs))]

    def gemm_loop():
        for xa, k, b, c, oa in gemm_args:
            ctx.check(L.jch_affine_gemm(ctx._h, DEV, xa, rows, k, n, None, None, b.ctypes.data, 1, c.ctypes.data, oa, n))

    variants = dict(pass_out=fir(tab, CT.FIR_SAME | CT.FIR_PER_COLUMN, bp), pass_in=fir(tab, CT.FIR_SAME | CT.FIR_PER_COLUMN, xp),
                    same_out=fir(uni, CT.FIR_SAME, bp), same_in=fir(uni, CT.FIR_SAME, xp), gemm_loop=gemm_loop)
    t = {k: [] for k in variants}
    for it in range(a.reps + 1):                 # the first round is the warm-up
        order = list(variants) if it % 2 == 0 else list(variants)[::-1]
        for k in order:
            ms_ = event_ms(variants[k])
            if it:
                t[k].append(ms_)
    med = {k: float(np.median(v)) for k, v in t.items()}
    loop_scaled = med["gemm_loop"] * n / rows
    nb = 2.0 * n * p * 8
    res[f"m={m}"] = dict(f=f, table_bytes=int(tab.nbytes), ms={k: round(v, 4) for k, v in med.items()}, gemm_loop_ms_scaled_to_n=round(loop_scaled, 2),
                         pass_tbs=round(nb / (med["pass_out"] * 1e-3) / 1e12, 3), same_tbs=round(nb / (med["same_out"] * 1e-3) / 1e12, 3),
                         pass_over_a=dict(out=round(med["pass_out"] / med["same_out"], 3), inplace=round(med["pass_in"] / med["same_in"], 3)),
                         b_over_pass=round(loop_scaled / med["pass_out"], 1), samples={k: [round(x, 4) for x in v] for k, v in t.items()})
    print(f"m={m}", json.dumps({k: res[f'm={m}'][k] for k in ("ms", "gemm_loop_ms_scaled_to_n", "pass_over_a", "b_over_pass")}), flush=True)

# a whole calpds fit at 64 standards (host arrays: the fits are host work, plskern's 500 small fits go through the library)
k = a.standards
z = np.arange(float(p))
St = np.asfortranarray(rng.uniform(0.5, 1.5, (k, 6)) @ np.stack([np.exp(-0.5 * ((z - c) / 12.0) ** 2) for c in np.linspace(30, p - 30, 6)])
                       + 1e-3 * rng.standard_normal((k, p)))
Sx = np.asfortranarray(1.05 * np.roll(St, 1, axis=1) + 0.02 + 1e-3 * rng.standard_normal((k, p)))
fit = {}
for name, kw in (("mlrpinv", dict(fun=J.mlrpinv)), ("plskern_nlv1", dict(fun=J.plskern, nlv=1, ctx=ctx))):
    ts = []
    for it in range(4):
        t0 = time.perf_counter(); fm = J.calpds(Sx, St, m=5, **kw); dt = time.perf_counter() - t0
        if it:
            ts.append(dt * 1e3)
    t0 = time.perf_counter(); J.predict(fm, Sx, ctx=ctx); tp = (time.perf_counter() - t0) * 1e3
    fit[name] = dict(fit_ms=round(float(np.median(ts)), 2), predict_standards_ms=round(tp, 2))
    print("calpds fit", name, json.dumps(fit[name]), flush=True)
res["calpds_fit_64_standards_m5"] = fit
res["not_measured"] = ["p = 2000 and windows beyond f = 21 (the 0.9 MB table of f = 57)", "host-array inputs (staged in row blocks)",
                       "the wide path beyond f = 57", "hardware counters (a run of their own)", "the gemm loop at the full n (scaled from loop_rows)",
                       "a two-rows-per-lane variant of the kernel (not built)"]
line = json.dumps(dict(metric="caltransfer_pds_pass", device=torch.cuda.get_device_name(0), **res))
print(line)
if a.out:
    with open(a.out, "w") as f_:
        f_.write(line + "\n")
