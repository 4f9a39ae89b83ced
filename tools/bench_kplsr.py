"""kplsr at n = 16 384 (and 4 096), p = 512, nlv = 25, q = 1 and 4, krbf (seeded spectra-like data, device-resident): one JSON line
with HIP-event times of the symmetric Gram (jch_kernel_gram), the whole kplsr fit at nlv = 1 and nlv = 25 (their difference over 24
is the cost of one LV: the pass over Kc plus the panel projections and the small state), predict of 1 000 new rows over nlv = 0:25,
and dkplsr on the same data.  The split of the fit by kernel (centring, the per-LV pass, the R pass) comes from a
`rocprofv3 --kernel-trace --stats` run of this script (profiles/kplsr_kernel_stats.csv).

    python tools/bench_kplsr.py [--n N ...] [--p P] [--reps R] [--out FILE]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J
from jchemo_hip import _lib

HBM_TBS = 8.0     # HBM peak, TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[16384, 4096])
ap.add_argument("--p", type=int, default=512)
ap.add_argument("--q", type=int, nargs="+", default=[1, 4])
ap.add_argument("--nlv", type=int, default=25)
ap.add_argument("--m", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-dkplsr", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
p, nlv, m = a.p, a.nlv, a.m
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")
L = J.load()


def spectra(rows, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    grid = torch.linspace(0, 1, p, dtype=torch.float64)
    c = torch.tensor([0.15, 0.3, 0.45, 0.6, 0.75, 0.9], dtype=torch.float64)
    H = torch.rand(rows, c.numel(), generator=g, dtype=torch.float64)
    X = 3.0 * (H @ torch.exp(-((grid[None, :] - c[:, None]) / 0.06) ** 2)) + 0.03 * torch.randn(rows, p, generator=g, dtype=torch.float64)
    out = J.colmajor_empty(rows, p, dev); out.copy_(X.to(dev))
    return out, H


def timed(fn, reps):
    fn()   # warm-up (workspace growth, first-launch costs)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), [round(t, 4) for t in ts]


gamma = 0.05
rows = []
for n in a.n:
    X, H = spectra(n, 1)
    Xn, _ = spectra(m, 2)
    K = J.colmajor_empty(n, n, dev)
    torch.cuda.synchronize()

    def gram():
        ctx.check(L.jch_kernel_gram(ctx._h, _lib.LOC_DEVICE, _lib.KERN_RBF, X.data_ptr(), n, n, None, X.data_ptr(), n, n, None, p, gamma,
                                    0.0, 1, K.data_ptr(), n))

    t_gram, s_gram = timed(gram, a.reps)
    del K
    for q in a.q:
        Y = J.colmajor_empty(n, q, dev)
        Y.copy_(torch.stack([torch.sin((k + 2.0) * H).sum(1) for k in range(q)], 1).to(dev))
        box = {}

        def fit(k):
            box["fm"] = J.kplsr(X, Y, nlv=k, gamma=gamma, ctx=ctx)

        t1, s1 = timed(lambda: fit(1), a.reps)
        t25, s25 = timed(lambda: fit(nlv), a.reps)
        fm = box["fm"]
        t_pred, s_pred = timed(lambda: J.predict(fm, Xn, nlv=range(0, nlv + 1), ctx=ctx), a.reps)
        per_lv = (t25 - t1) / (nlv - 1)
        kc_bytes = 8.0 * n * n
        res = dict(n=n, p=p, q=q, nlv=nlv, gram_ms=round(t_gram, 4), fit_nlv1_ms=round(t1, 4), fit_ms=round(t25, 4),
                   per_lv_ms=round(per_lv, 4), per_lv_hbm_share=round(kc_bytes / (per_lv * 1e-3) / (HBM_TBS * 1e12), 3),
                   kc_read_at_peak_ms=round(kc_bytes / (HBM_TBS * 1e12) * 1e3, 4), predict_rows=m, predict_nlv="0:%d" % nlv,
                   predict_ms=round(t_pred, 4), iter_max=int(np.max(fm.iter)), iter_sum=int(np.sum(fm.iter)),
                   samples=dict(gram=s_gram, fit_nlv1=s1, fit=s25, predict=s_pred))
        if not a.no_dkplsr and q == 1:
            t_dk, s_dk = timed(lambda: J.dkplsr(X, Y, nlv=nlv, gamma=gamma, ctx=ctx), max(2, a.reps // 2))
            res.update(dkplsr_ms=round(t_dk, 4), samples=dict(res["samples"], dkplsr=s_dk))
        rows.append(res)
        print(json.dumps(res), flush=True)
line = json.dumps(dict(metric="kplsr_krbf", gamma=gamma, device=torch.cuda.get_device_name(0), runs=rows))
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
