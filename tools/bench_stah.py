"""Exact column medians / MADs and the Stahel-Donoho outlyingness at n = 1e6, p = 500, a = 2000 with X on the device (standard normal X + 10, 0 / 1
directions from default_rng(7)).  One JSON line with HIP-event times, medians of --reps runs after one warm-up, of
  * jch_col_median_mad on the device-resident X with host results (whole calls), medians and MADs and the medians alone; the bytes it
    reads (X once per pass: 6 passes per selection) over that time, in GB/s and as a share of --hbm-peak;
  * the same medians from `torch.sort` along the columns of the same tensor (what a user has without the primitive), and the ratio;
  * `stah` at a directions, fit (jch_stah with fit = 1) and predict (fit = 0: projection and row maximum only), whole calls; the projection alone
    as one jch_affine_gemm call per panel of the width jch_stah uses (measured, each with its own upload and synchronisation); the selection as
    fit - predict and the row maximum as predict - projection (both DERIVED, marked so in the keys).
Run it under a `timeout` of its own, as every GPU step.  Whoever runs it writes the numbers into DESIGN.md §18, the README and
profiles/stah_bench.json.

    python tools/bench_stah.py [--n N] [--p P] [--a A] [--reps R] [--hbm-peak GBS] [--out FILE]
"""
import argparse, json, os, re, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--p", type=int, default=500)
ap.add_argument("--a", type=int, default=2000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--hbm-peak", type=float, default=8000.0, help="GB/s (MI355X: 8 TB/s)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")
L = J.load()
n, p, na = a.n, a.p, a.a
csrc = os.path.join(ROOT, "jchemo.jl_amd", "csrc")
passes = int(re.search(r"#define CS_PASSES (\d+)", open(os.path.join(csrc, "colselect.hip")).read()).group(1))
st_src = open(os.path.join(csrc, "stah.hip")).read()
budget = 1 << int(re.search(r"#define ST_PANEL_BYTES \(\(size_t\)1 << (\d+)\)", st_src).group(1))
b = min(na, int(re.search(r"#define ST_PANEL_MAXCOLS (\d+)", st_src).group(1)), max(1, budget // (8 * n)))
if 16 <= b < na:
    b -= b % 16


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, reps):
    fn()                                  # warm-up: workspace growth, first-launch costs
    return float(np.median([event_ms(fn) for _ in range(reps)]))


g = torch.Generator(device=dev); g.manual_seed(7)
X = J.colmajor_empty(n, p, dev)
for c0 in range(0, p, 125):               # (in column blocks: no second n x p temporary)
    c1 = min(p, c0 + 125)
    X[:, c0:c1] = torch.randn((n, c1 - c0), dtype=torch.float64, device=dev, generator=g) + 10.0
torch.cuda.synchronize()
gb = n * p * 8 / 1e9

# host outputs: the call then ends with a synchronisation, so the events on torch's stream bracket all of its kernels whichever stream the ctx owns
# (device outputs only enqueue); the price is one 4 KB copy per result
med, mad = np.empty(p), np.empty(p)
both = lambda: ctx.check(L.jch_col_median_mad(ctx._h, 1, X.data_ptr(), n, p, n, med.ctypes.data, mad.ctypes.data, 0))   # noqa: E731
only = lambda: ctx.check(L.jch_col_median_mad(ctx._h, 1, X.data_ptr(), n, p, n, med.ctypes.data, None, 0))             # noqa: E731
t_both, t_only = median_ms(both, a.reps), median_ms(only, a.reps)


def sort_medians():
    s = torch.sort(X.t(), dim=1).values       # X.t() is the contiguous p x n view of the column-major X
    return s[:, (n - 1) // 2] / 2 + s[:, n // 2] / 2


agree = bool(np.array_equal(sort_medians().cpu().numpy(), med))
t_sort = median_ms(sort_medians, a.reps)
torch.cuda.empty_cache()

P = np.asfortranarray(np.random.default_rng(7).integers(0, 2, size=(p, na)), dtype=np.float64)
reps2 = max(1, a.reps // 2 + 1)
t_fit = median_ms(lambda: J.stah(X, na, scal=False, P=P, ctx=ctx), reps2)
obj = J.occstah(X, a=na, scal=False, P=P, ctx=ctx)
t_pred = median_ms(lambda: sys.modules["jchemo_hip.stah"]._jch_stah(X, None, None, P, False, obj.res_stah.mu, obj.res_stah.s, ctx), reps2)
t_occ_fit = median_ms(lambda: J.occstah(X, a=na, scal=False, P=P, ctx=ctx), reps2)
t_occ_pred = median_ms(lambda: J.predict(obj, X, ctx=ctx), reps2)
npanel = -(-na // b)
Tb = J.colmajor_empty(n, b, dev)
Pb = np.asfortranarray(P[:, :b])
torch.cuda.synchronize()
t_gemm_panel = median_ms(lambda: ctx.check(L.jch_affine_gemm(ctx._h, 1, X.data_ptr(), n, p, n, None, None, Pb.ctypes.data, b, None, Tb.data_ptr(), n)), a.reps)
t_gemm = t_gemm_panel * na / b

res = dict(metric="stah", device=torch.cuda.get_device_name(0), n=n, p=p, a=na, reps=a.reps, x_gb=round(gb, 3), passes_per_selection=passes,
           col_median_mad_ms=round(t_both, 3), col_median_mad_read_gb=round(2 * passes * gb, 1), col_median_mad_gbs=round(2 * passes * gb / (t_both * 1e-3), 1),
           col_median_mad_share_of_hbm_peak=round(2 * passes * gb / (t_both * 1e-3) / a.hbm_peak, 3),
           col_median_ms=round(t_only, 3), col_median_gbs=round(passes * gb / (t_only * 1e-3), 1), hbm_peak_gbs=a.hbm_peak,
           torch_sort_medians_ms=round(t_sort, 3), torch_sort_over_col_median=round(t_sort / t_only, 2), medians_equal_torch_sort=agree,
           panel_cols=b, panels=npanel, stah_fit_ms=round(t_fit, 3), stah_predict_ms=round(t_pred, 3),
           projection_ms=round(t_gemm, 3), projection_one_panel_ms=round(t_gemm_panel, 3),
           selection_ms_derived_fit_minus_predict=round(t_fit - t_pred, 3), rowmax_ms_derived_predict_minus_projection=round(t_pred - t_gemm, 3),
           occstah_fit_ms=round(t_occ_fit, 3), occstah_predict_ms=round(t_occ_pred, 3))
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
