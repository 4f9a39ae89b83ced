"""kpca at n = 16 384 (and 4 096), p = 512, nlv = 25, krbf with gamma = 1/p (seeded spectra-like data, device-resident): one JSON line
with HIP-event times of the symmetric Gram (jch_kernel_gram), the panel product Kc V (jch_kc_panel) at b = 16 / 32 / 64, the whole
kpca fit with its iteration count at the default block and at the blocks the oversampling knob JCH_KPCA_OVERSAMPLE selects
(b = 32 / 48 / 64), and transform of 1 000 new rows.  The split of the fit by kernel (Gram, centring, pass, small kernels) comes from
a `rocprofv3 --kernel-trace --stats` run of this script (profiles/kpca_kernel_stats.csv).

    python tools/bench_kpca.py [--n N ...] [--p P] [--reps R] [--out FILE]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J
from jchemo_hip import _lib

HBM_TBS = 8.0     # HBM peak, TB/s
F64_MFMA_TF = 78.6

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, nargs="+", default=[16384, 4096])
ap.add_argument("--p", type=int, default=512)
ap.add_argument("--nlv", type=int, default=25)
ap.add_argument("--m", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--oversample", type=int, nargs="*", default=[7, 23, 39])
ap.add_argument("--out", default=None)
a = ap.parse_args()
p, nlv, m = a.p, a.nlv, a.m
gamma = 1.0 / p
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
    return out


def timed(fn, reps):
    fn()   # warm-up (workspace growth, first-launch costs)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), [round(t, 4) for t in ts]


rows = []
for n in a.n:
    X = spectra(n, 1)
    Xn = spectra(m, 2)
    K = J.colmajor_empty(n, n, dev)
    torch.cuda.synchronize()

    def gram():
        ctx.check(L.jch_kernel_gram(ctx._h, _lib.LOC_DEVICE, _lib.KERN_RBF, X.data_ptr(), n, n, None, X.data_ptr(), n, n, None, p, gamma,
                                    0.0, 1, K.data_ptr(), n))

    t_gram, s_gram = timed(gram, a.reps)
    res = dict(n=n, p=p, nlv=nlv, gamma=gamma, gram_ms=round(t_gram, 4), kc_read_at_peak_ms=round(8.0 * n * n / (HBM_TBS * 1e12) * 1e3, 4))
    samples = dict(gram=s_gram)
    for b in (16, 32, 64):
        V = J.colmajor_empty(n, b, dev); V.copy_(torch.rand(n, b, dtype=torch.float64, device=dev))
        out = J.colmajor_empty(n, b, dev)
        torch.cuda.synchronize()
        reps = 20

        def panel():
            for _ in range(reps):
                ctx.check(L.jch_kc_panel(ctx._h, K.data_ptr(), n, V.data_ptr(), n, b, out.data_ptr(), n))

        t, s = timed(panel, a.reps)
        ms = t / reps
        res[f"panel_b{b}_ms"] = round(ms, 4)
        res[f"panel_b{b}_hbm_share"] = round(8.0 * n * n / (ms * 1e-3) / (HBM_TBS * 1e12), 3)
        res[f"panel_b{b}_tflops"] = round(2.0 * n * n * b / (ms * 1e-3) / 1e12, 2)
        samples[f"panel_b{b}"] = s
    del K, V, out
    torch.cuda.empty_cache()
    box = {}

    def fit():
        box["fm"] = J.kpca(X, nlv=nlv, gamma=gamma, ctx=ctx)

    t_fit, s_fit = timed(fit, a.reps)
    fm = box["fm"]
    res.update(fit_ms=round(t_fit, 4), niter=fm.niter, converged=fm.converged, max_resid_rel=float(fm.resid.max() / fm.eig[0]),
               eig_head=[float(v) for v in fm.eig[:3]])
    samples["fit"] = s_fit
    sweep = {}
    for os_ in a.oversample:
        os.environ["JCH_KPCA_OVERSAMPLE"] = str(os_)
        t, s = timed(fit, max(2, a.reps // 2))
        sweep[str(os_)] = dict(b=min(n, (nlv + os_ + 15) // 16 * 16), fit_ms=round(t, 4), niter=box["fm"].niter, converged=box["fm"].converged)
    os.environ.pop("JCH_KPCA_OVERSAMPLE", None)
    res["oversample_sweep"] = sweep
    t_tr, s_tr = timed(lambda: J.kpca_transform(fm, Xn, ctx=ctx), a.reps)
    res.update(transform_rows=m, transform_ms=round(t_tr, 4))
    samples["transform"] = s_tr
    res["samples"] = samples
    rows.append(res)
    print(json.dumps(res), flush=True)
line = json.dumps(dict(metric="kpca_krbf", device=torch.cuda.get_device_name(0), f64_mfma_peak_tf=F64_MFMA_TF, hbm_peak_tbs=HBM_TBS, runs=rows))
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
