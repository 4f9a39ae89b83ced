"""PCA / PCR at n = 1e6, p = 500 (and --p 2000): device-resident X = H B + 100 + noise with a decaying spectrum (32 factors, 0.85^k; on pure
noise the subspace iteration has no gap to converge on).  One JSON line with HIP-event times, medians of --reps runs after one warm-up, of
  * jch_xtdx alone (weights, means, the Gram pass, its reduction) and the mean pass alone (jch_covsel_pass against the weight panel); the Gram
    kernels' time is taken as their difference.  Two rates: the useful one, n p^2 flop over that time, and the executed one, 2 n 128^2 flop per
    upper tile pair (padding and the unused half of the diagonal tiles included), which is how k_syrk's 44 TF = 0.56 of the 78.6 TF f64 matrix
    peak is counted (kern2.hip);
  * the parent route to the same matrix, jch_weighted_cov on the device X with d = p (moments, a centred row-major copy of X, k_syrk, and a
    host download of the d x d result), timed in runs that ALTERNATE with jch_xtdx's;
  * the whole pcasvd at nlv = 25 with its niter, jch_transform alone, and the iteration as what is left (fit - xtdx - transform);
  * pcr at q = 1 and q = 10.
Run it under a `timeout` of its own, as every GPU step.  Whoever runs it writes the numbers into DESIGN.md §16 and profiles/pca_bench.json.

    python tools/bench_pca.py [--n N] [--p P] [--nlv A] [--q Q ...] [--reps R] [--out FILE]
"""
import argparse, ctypes as C, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J

F64_MATRIX_TF = 78.6

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--p", type=int, default=500)
ap.add_argument("--nlv", type=int, default=25)
ap.add_argument("--q", type=int, nargs="+", default=[1, 10])
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


g = torch.Generator(device=dev); g.manual_seed(7)
r = 32
X = J.colmajor_empty(n, p, dev)
H = torch.randn((n, r), dtype=torch.float64, device=dev, generator=g) * (0.85 ** torch.arange(r, dtype=torch.float64, device=dev))
B = torch.linalg.qr(torch.randn((p, r), dtype=torch.float64, device=dev, generator=g))[0].t().contiguous()
for c0 in range(0, p, 125):               # (in column blocks: no second n x p temporary)
    c1 = min(p, c0 + 125)
    X[:, c0:c1] = H @ B[:, c0:c1] + 100.0 + 1e-3 * torch.randn((n, c1 - c0), dtype=torch.float64, device=dev, generator=g)
wn = torch.full((n,), 1.0 / n, dtype=torch.float64, device=dev)
Gd = torch.empty((p, p), dtype=torch.float64, device=dev)
mud = torch.empty(p, dtype=torch.float64, device=dev)
S = np.empty((p, p), order="F")
torch.cuda.synchronize()

xtdx = lambda: ctx.check(L.jch_xtdx(ctx._h, 1, X.data_ptr(), n, p, n, None, Gd.data_ptr(), p, mud.data_ptr(), None, None))          # noqa: E731
mean = lambda: ctx.check(L.jch_covsel_pass(ctx._h, X.data_ptr(), n, p, n, None, wn.data_ptr(), 1, n, mud.data_ptr()))               # noqa: E731
wcov = lambda: ctx.check(L.jch_weighted_cov(ctx._h, 1, X.data_ptr(), n, p, n, None, S.ctypes.data, None))                            # noqa: E731
xtdx(); wcov()
tx, tw = [], []
for _ in range(a.reps):                    # alternating runs on one box
    tx.append(event_ms(xtdx)); tw.append(event_ms(wcov))
t_xtdx, t_wcov = float(np.median(tx)), float(np.median(tw))
t_mean = median_ms(mean, a.reps)
Gh = Gd.cpu().numpy()
agree = float(np.max(np.abs(Gh - S)) / np.max(np.abs(S)))
t_gram = t_xtdx - t_mean
tf = n * float(p) * p / (t_gram * 1e-3) / 1e12
nblk = (p + 127) // 128
tf_exec = 2.0 * n * 128 * 128 * (nblk * (nblk + 1) // 2) / (t_gram * 1e-3) / 1e12

fm = J.pcasvd(X, nlv=nlv, ctx=ctx)
t_fit = median_ms(lambda: J.pcasvd(X, nlv=nlv, ctx=ctx), max(1, a.reps // 2 + 1))
t_tr = median_ms(lambda: J.transform(fm, X, ctx=ctx), a.reps)
res = dict(metric="pca", device=torch.cuda.get_device_name(0), n=n, p=p, nlv=nlv, reps=a.reps, xtdx_ms=round(t_xtdx, 3), mean_pass_ms=round(t_mean, 3),
           gram_ms=round(t_gram, 3), gram_tf=round(tf, 2), gram_share_of_f64_matrix_peak=round(tf / F64_MATRIX_TF, 3),
           gram_tf_executed=round(tf_exec, 2), gram_executed_share_of_f64_matrix_peak=round(tf_exec / F64_MATRIX_TF, 3),
           weighted_cov_ms=round(t_wcov, 3), weighted_cov_includes="moments, centred row-major copy, k_syrk, host download of G",
           xtdx_over_weighted_cov=round(t_xtdx / t_wcov, 3), max_rel_diff_to_weighted_cov=agree,
           pcasvd_ms=round(t_fit, 3), niter=fm.niter, converged=bool(fm.converged), transform_ms=round(t_tr, 3),
           iteration_ms=round(t_fit - t_xtdx - t_tr, 3), iteration_ms_per_iter=round((t_fit - t_xtdx - t_tr) / max(fm.niter, 1), 3), pcr=[])
for q in a.q:
    Y = J.colmajor_empty(n, q, dev)
    Y.copy_(X[:, :: max(1, p // q)][:, :q] * 0.5 + torch.randn((n, q), dtype=torch.float64, device=dev, generator=g))
    torch.cuda.synchronize()
    t_pcr = median_ms(lambda: J.pcr(X, Y, nlv=nlv, ctx=ctx), max(1, a.reps // 2 + 1))
    res["pcr"].append(dict(q=q, pcr_ms=round(t_pcr, 3), over_pcasvd_ms=round(t_pcr - t_fit, 3)))
    del Y
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
