"""krr at n = 16 384 (and 4 096), p = 512, q = 1 and 4, krbf with gamma = 1/p, lb = 1e-2 (seeded spectra-like data, device-resident): one
JSON line with HIP-event times of the Cholesky factorisation (jch_chol_factor) next to the symmetric Gram (jch_kernel_gram) of the
same call — the yardstick: same instruction, same tile scheme —, the two solves (jch_chol_solve), the df pass (jch_chol_inv_fro2),
the whole krr + krr_coef and krr_predict of 1 000 rows for 1 and for 8 values of lb.  Flops and bytes come from the shapes.  The split
of the factorisation by kernel (diagonal step x count, panel, trailing update) comes from a `rocprofv3 --kernel-trace --stats` run of
this script (profiles/krr_kernel_stats.csv).  --svd-n N also times the numpy restatement's full SVD on the host (a CPU stand-in for
the reference's route, context only).

    python tools/bench_krr.py [--n N ...] [--p P] [--reps R] [--svd-n N] [--out FILE]
"""
import argparse, ctypes as C, json, os, sys, time
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
ap.add_argument("--q", type=int, nargs="+", default=[1, 4])
ap.add_argument("--m", type=int, default=1000)
ap.add_argument("--lb", type=float, default=1e-2)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--svd-n", type=int, default=0)
ap.add_argument("--out", default=None)
a = ap.parse_args()
p, m, lb = a.p, a.m, a.lb
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
    return out, H


def timed(fn, reps, setup=None):
    ts = []
    for it in range(reps + 1):   # the first one is the warm-up (workspace growth, first-launch costs)
        if setup:
            setup()
            torch.cuda.synchronize()   # the setup runs on torch's stream, the library on the ctx's own
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        if it:
            ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), [round(t, 4) for t in ts]


rows = []
for n in a.n:
    X, H = spectra(n, 1)
    Xn, _ = spectra(m, 2)
    qmax = max(a.q)
    Y = J.colmajor_empty(n, qmax, dev); Y.copy_((H[:, :qmax] ** 2 + 0.05 * torch.randn(n, qmax, dtype=torch.float64)).to(dev))
    K = J.colmajor_empty(n, n, dev)
    torch.cuda.synchronize()

    def gram():
        ctx.check(L.jch_kernel_gram(ctx._h, _lib.LOC_DEVICE, _lib.KERN_RBF, X.data_ptr(), n, n, None, X.data_ptr(), n, n, None, p, gamma,
                                    0.0, 1, K.data_ptr(), n))

    t_gram, s_gram = timed(gram, a.reps)
    res = dict(n=n, p=p, gamma=gamma, lb=lb, gram_ms=round(t_gram, 4), gram_tflops=round(float(n) * n * p / (t_gram * 1e-3) / 1e12, 2))
    samples = dict(gram=s_gram)
    del K
    torch.cuda.empty_cache()
    fm = J.krr(X, Y, lb=lb, gamma=gamma, ctx=ctx)
    M = J.colmajor_empty(n, n, dev)
    info = C.c_int32(0)

    def fresh():
        M.copy_(fm.Kd); M.diagonal().add_(lb * lb)

    def factor():
        ctx.check(L.jch_chol_factor(ctx._h, M.data_ptr(), n, n, C.byref(info)))

    t_f, s_f = timed(factor, a.reps, setup=fresh)
    assert info.value == 0
    tf = float(n) ** 3 / 3 / (t_f * 1e-3) / 1e12
    res.update(factor_ms=round(t_f, 4), factor_tflops=round(tf, 2), factor_share_of_f64_peak=round(tf / F64_MFMA_TF, 3),
               factor_over_gram_rate=round(tf / res["gram_tflops"], 3), factor_floor_at_peak_ms=round(float(n) ** 3 / 3 / (F64_MFMA_TF * 1e12) * 1e3, 3))
    samples["factor"] = s_f
    for q in a.q:
        B = J.colmajor_empty(n, q, dev)

        def solve():
            ctx.check(L.jch_chol_solve(ctx._h, M.data_ptr(), n, n, B.data_ptr(), q, n))

        t, s = timed(solve, a.reps, setup=lambda: B.copy_(fm.B[:, :q]))
        passes = (q + 7) // 8                                # L is read once per direction and per 8 columns of B
        res[f"solve_q{q}_ms"] = round(t, 4)
        res[f"solve_q{q}_hbm_share"] = round(2 * passes * 4.0 * n * n / (t * 1e-3) / (HBM_TBS * 1e12), 3)   # the triangle: n^2 / 2 doubles per direction
        samples[f"solve_q{q}"] = s
    fro = C.c_double(0.0)
    t, s = timed(lambda: ctx.check(L.jch_chol_inv_fro2(ctx._h, M.data_ptr(), n, n, C.byref(fro))), a.reps)
    res.update(df_pass_ms=round(t, 4), df_pass_tflops=round(float(n) ** 3 / 3 / (t * 1e-3) / 1e12, 2), df=1.0 + n - lb * lb * fro.value)
    samples["df_pass"] = s
    del M
    torch.cuda.empty_cache()
    for q in a.q:
        box = {}

        def whole():
            box["fm"] = J.krr(X, Y[:, :q], lb=lb, gamma=gamma, ctx=ctx)
            box["coef"] = J.krr_coef(box["fm"], ctx=ctx)

        t, s = timed(whole, max(2, a.reps // 2))
        res[f"krr_coef_q{q}_ms"] = round(t, 4)
        samples[f"krr_coef_q{q}"] = s
        if q == a.q[0]:
            res["krr_coef_df"] = box["coef"][2]
    fmq = box["fm"]
    lbs8 = [lb * f for f in (0.25, 0.5, 1, 2, 4, 8, 16, 32)]
    for v in lbs8:
        J.krr_coef(fmq, lb=v, df=False, ctx=ctx)              # the solves are cached: predict is timed alone
    t1, s1 = timed(lambda: J.krr_predict(fmq, Xn, ctx=ctx), a.reps)
    t8, s8 = timed(lambda: J.krr_predict(fmq, Xn, lb=lbs8, ctx=ctx), a.reps)
    res.update(predict_rows=m, predict_q=fmq.B.shape[1], predict_1lb_ms=round(t1, 4), predict_8lb_ms=round(t8, 4))
    samples.update(predict_1lb=s1, predict_8lb=s8)
    res["samples"] = samples
    rows.append(res)
    print(json.dumps(res), flush=True)
    del fm, fmq, box
    torch.cuda.empty_cache()
cpu = None
if a.svd_n:
    n = a.svd_n
    rng = np.random.default_rng(0)
    G = rng.standard_normal((n, 64))
    Kd = G @ G.T / n
    t0 = time.perf_counter(); np.linalg.svd(Kd); t1 = time.perf_counter()
    cpu = dict(n=n, full_svd_s=round(t1 - t0, 2), note="numpy full SVD of an n x n PSD matrix on the host: a CPU stand-in for the reference's svd(Kd), context only")
line = json.dumps(dict(metric="krr_krbf", device=torch.cuda.get_device_name(0), f64_mfma_peak_tf=F64_MFMA_TF, hbm_peak_tbs=HBM_TBS, runs=rows,
                       cpu_stand_in=cpu))
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
