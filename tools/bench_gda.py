"""The three entries of the Gaussian discrimination family on the device, HIP-event times, medians of --reps runs after one warm-up, everything on
device tensors.  One JSON line (and --out FILE, by default profiles/gda_bench.json) with
  * `class_cov` at n = 100 000, p = 500, 10 classes: the one-pass jch_class_cov (Wi, W and the means) against ten jch_weighted_cov calls with
    indicator weights, which is what `_class_score_stats` of plsr.py would cost on that block;
  * `gauss_factor` of the 10 class covariances (p = 500) in one call, beside `torch.linalg.cholesky` + `torch.linalg.solve_triangular` of the same;
  * `mahsq_chol` for m = 100 000 queries against 10 centres with nfac = 1 and nfac = 10: time and the achieved f64 flop rate (m ncen p (p + 1)
    flops: the multiply-adds on and above the diagonal), beside the yardstick in the same run — z = (X - mu) Uinv by `torch.matmul` and the row
    sums of z^2 per centre — and the largest relative difference between the two.
Nothing here is a gate; the numbers are recorded.  Run it under a `timeout` of its own, as every GPU step.

    python tools/bench_gda.py [--n N] [--m M] [--p P] [--ncls C] [--reps R] [--out FILE]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J
from jchemo_hip import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--m", type=int, default=100000)
ap.add_argument("--p", type=int, default=500)
ap.add_argument("--ncls", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gda_bench.json"))
a = ap.parse_args()
n, m, p, ncls = a.n, a.m, a.p, a.ncls
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, reps=a.reps):
    fn()                                  # warm-up: workspace growth, first-launch costs
    return float(np.median([event_ms(fn) for _ in range(reps)]))


g = torch.Generator(device=dev); g.manual_seed(20251020)
mix = torch.randn((p, p), generator=g, dtype=torch.float64, device=dev) / np.sqrt(p) + torch.eye(p, dtype=torch.float64, device=dev)
centres = 10 + torch.randn((ncls, p), generator=g, dtype=torch.float64, device=dev)
sizes = [n // ncls + (1 if c < n % ncls else 0) for c in range(ncls)]
cs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
lab = torch.as_tensor(np.repeat(np.arange(ncls), sizes), device=dev)
Z = J.colmajor_empty(n, p, dev); Z.copy_(centres[lab] + torch.randn((n, p), generator=g, dtype=torch.float64, device=dev) @ mix)
Xq = J.colmajor_empty(m, p, dev); Xq.copy_(centres[torch.as_tensor(np.arange(m) % ncls, device=dev)] + torch.randn((m, p), generator=g, dtype=torch.float64, device=dev) @ mix)
res = dict(metric="gda", device=torch.cuda.get_device_name(0), n=n, m=m, p=p, ncls=ncls, reps=a.reps)

# ---- 1. class_cov against ncls jch_weighted_cov calls with indicator weights
Wi, W, ct = J.class_cov(Z, cs, ctx=ctx)
res["class_cov_ms"] = median_ms(lambda: J.class_cov(Z, cs, ctx=ctx))
ind = [torch.zeros(n, dtype=torch.float64, device=dev) for _ in range(ncls)]
for c in range(ncls):
    ind[c][cs[c]:cs[c + 1]] = 1.0
S = np.empty((p, p), order="F")


def ten_calls():
    for c in range(ncls):
        ctx.check(_lib.load().jch_weighted_cov(ctx._h, _lib.LOC_DEVICE, Z.data_ptr(), n, p, n, ind[c].data_ptr(), S.ctypes.data, None))


res["weighted_cov_x_ncls_ms"] = median_ms(ten_calls)
res["class_cov_last_class_max_rel_diff"] = float(np.max(np.abs(S - Wi[ncls - 1].cpu().numpy())) / np.max(np.abs(S)))

# ---- 2. gauss_factor of the class covariances (corrected)
f = torch.as_tensor(np.array([k / (k - 1) for k in sizes]), device=dev)[:, None, None]
Sc = (Wi * f).contiguous()
Uinv, diagU, info = J.gauss_factor(Sc, ctx=ctx)
assert not info.any()
res["gauss_factor_ms"] = median_ms(lambda: J.gauss_factor(Sc, ctx=ctx))
eye = torch.eye(p, dtype=torch.float64, device=dev).expand(ncls, p, p).contiguous()


def torch_factor():
    L = torch.linalg.cholesky(Sc)
    return torch.linalg.solve_triangular(L.transpose(1, 2), eye, upper=True)


res["torch_cholesky_solve_triangular_ms"] = median_ms(torch_factor)
Ut = torch_factor()
res["gauss_factor_max_rel_diff"] = float(((Uinv - Ut).abs().amax() / Ut.abs().amax()).item())

# ---- 3. mahsq_chol, one shared factor and one per class
flops = float(m) * ncls * p * (p + 1)


def torch_mahsq(U3):
    out = torch.empty((m, ncls), dtype=torch.float64, device=dev)
    for c in range(ncls):
        z = (Xq - centres[c]) @ U3[c if U3.shape[0] > 1 else 0]
        out[:, c] = (z * z).sum(dim=1)
    return out


mu = centres.cpu().numpy()
for name, U in (("nfac1", Uinv[0]), (f"nfac{ncls}", Uinv)):
    d = J.mahsq_chol(Xq, mu, U, ctx=ctx)
    ms = median_ms(lambda: J.mahsq_chol(Xq, mu, U, ctx=ctx))
    U3 = U[None] if U.dim() == 2 else U
    ref = torch_mahsq(U3)
    res[f"mahsq_chol_{name}_ms"] = ms
    res[f"mahsq_chol_{name}_f64_tflops"] = flops / ms / 1e9
    res[f"torch_matmul_rowsum_{name}_ms"] = median_ms(lambda: torch_mahsq(U3))
    res[f"mahsq_chol_{name}_max_rel_diff"] = float(((d - ref).abs() / ref).amax().item())

line = json.dumps(res)
print(line)
with open(a.out, "w") as fh:
    fh.write(line + "\n")
ctx.close()
