"""dkplsr at n = 16 384, p = 512, q = 1, nlv = 25, krbf (seeded spectra-like data, device-resident): one JSON line with HIP-event
times of the symmetric Gram (jch_kernel_gram), the inner fit on K (plskern on the 16 384-column Gram: the two-pass wide sweep),
the whole dkplsr, and predict of 1 000 new rows over nlv = 0:25; Gram TF/s against the f64 matrix peak and the bytes bound.

    python tools/bench_dkplsr.py [--n N] [--p P] [--reps R] [--out FILE]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J
from jchemo_hip import _lib

PEAK_TF = 78.6    # f64 matrix peak (MI355X)
HBM_TBS = 8.0     # HBM peak, TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16384)
ap.add_argument("--p", type=int, default=512)
ap.add_argument("--nlv", type=int, default=25)
ap.add_argument("--m", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, p, nlv, m = a.n, a.p, a.nlv, a.m
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


X, H = spectra(n, 1)
Y = J.colmajor_empty(n, 1, dev); Y.copy_(torch.sin(2.0 * H).sum(1, keepdim=True).to(dev))
Xn, _ = spectra(m, 2)
gamma = 0.05


def timed(fn, reps):
    fn()   # warm-up (workspace growth, first-launch costs)
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), [round(t, 4) for t in ts]


K = J.colmajor_empty(n, n, dev)
torch.cuda.synchronize()


def gram():
    ctx.check(L.jch_kernel_gram(ctx._h, _lib.LOC_DEVICE, _lib.KERN_RBF, X.data_ptr(), n, n, None, X.data_ptr(), n, n, None, p, gamma, 0.0, 1,
                                K.data_ptr(), n))


t_gram, s_gram = timed(gram, a.reps)
t_fit, s_fit = timed(lambda: J.plskern(K, Y, nlv=nlv, ctx=ctx), max(2, a.reps // 2))
fm = None


def whole():
    global fm
    fm = J.dkplsr(X, Y, nlv=nlv, gamma=gamma, ctx=ctx)


t_dk, s_dk = timed(whole, max(2, a.reps // 2))
t_pred, s_pred = timed(lambda: J.predict(fm, Xn, nlv=range(0, nlv + 1), ctx=ctx), a.reps)
flop = float(n) * n * p            # symmetric: half of the 2 n^2 p of the full product
tf = flop / (t_gram * 1e-3) / 1e12
bytes_out = 8.0 * n * n
res = dict(
    metric="dkplsr_krbf", n=n, p=p, q=1, nlv=nlv, gamma=gamma, device=torch.cuda.get_device_name(0),
    gram_ms=round(t_gram, 4), gram_tflops=round(tf, 2), gram_share_of_f64_peak=round(tf / PEAK_TF, 3),
    gram_flop_bound_ms=round(flop / (PEAK_TF * 1e12) * 1e3, 4), gram_bytes_bound_ms=round(bytes_out / (HBM_TBS * 1e12) * 1e3, 4),
    fit_on_K_ms=round(t_fit, 4), dkplsr_ms=round(t_dk, 4), predict_rows=m, predict_nlv="0:%d" % nlv, predict_ms=round(t_pred, 4),
    samples=dict(gram=s_gram, fit_on_K=s_fit, dkplsr=s_dk, predict=s_pred),
    nlv_fitted=int(fm.fm.P.shape[1]), tt_ratio=float(fm.fm.TT[-1] / fm.fm.TT[0]),
)
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
