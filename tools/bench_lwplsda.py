"""Local PLS discrimination on the device: n = 1e5 training rows, p = 500, 4 classes, nlvdis = 20, mahal, k = 200, nlv = 1:15, 1000 queries, device
tensors.  HIP events on the stream the ctx shares with torch, medians of --reps after a warm-up.  Every stage is printed as it finishes, then
one JSON line (and --out FILE) with
  * the whole `predict` of `lwplsrda`, `lwplslda`, `lwplsqda` for the nlv range;
  * `jch_knn_gda` alone on the local scores the engine hands out (lda and qda), i.e. the share of `k_knn_gda`; the whole predict of `lwplsrda` minus
    nothing else is the search + `k_locw_plskern` with score stores (its share is read from a kernel trace, which this tool does not take);
  * the only other device route to the same discriminants: torch's batched `cholesky` + `solve_triangular` ONCE PER a on the same scores (lda's
    pooled covariance), with the largest posterior difference to the library's.
Not done by this tool: `lwplsrda` against `lwplsr_predict` on the dummy table through the p-space kernel of the parent commit.  The regression
guard of the p-space kernel with null score outputs at k = 300, q = 1, p = 500 is tools/bench_locw_guard.py, run alternately on two builds.
No figure here is a pass condition.  Run it under a `timeout` of its own, as every GPU step.

    python tools/bench_lwplsda.py [--n N] [--p P] [--m M] [--k K] [--nlv A] [--reps R] [--skip-torch] [--out FILE]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--p", type=int, default=500)
ap.add_argument("--m", type=int, default=1000)
ap.add_argument("--k", type=int, default=200)
ap.add_argument("--nlv", type=int, default=15)
ap.add_argument("--nlvdis", type=int, default=20)
ap.add_argument("--nlev", type=int, default=4)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--skip-torch", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, p, m, k, nlv, nlev = a.n, a.p, a.m, a.k, a.nlv, a.nlev
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")
out = {"shape": dict(n=n, p=p, m=m, k=k, nlv=[1, nlv], nlvdis=a.nlvdis, nlev=nlev, metric="mahal", device=torch.cuda.get_device_name(0))}


def stage(key, value):
    out[key] = value
    print(key, json.dumps(value), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f)


def timed(fn, reps=a.reps):
    fn(); ctx.synchronize(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); ctx.synchronize(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps)


def colmajor(t):
    o = torch.empty((t.shape[1], t.shape[0]), dtype=torch.float64, device=dev).t()
    o.copy_(t)
    return o


g = torch.Generator(device=dev); g.manual_seed(20251021)
cen = 0.4 * torch.randn((nlev, p), generator=g, device=dev, dtype=torch.float64)
B = torch.randn((6, p), generator=g, device=dev, dtype=torch.float64)


def draw(r):
    y = torch.arange(r, device=dev) % nlev
    return colmajor(cen[y] + torch.randn((r, 6), generator=g, device=dev, dtype=torch.float64) @ B + 0.3 * torch.randn((r, p), generator=g, device=dev, dtype=torch.float64)), y.cpu().numpy().astype(np.int32)


X, y = draw(n)
Xq, _ = draw(m)
rng = range(1, nlv + 1)
common = dict(nlvdis=a.nlvdis, metric="mahal", h=2.0, k=k, nlv=nlv, ctx=ctx)
models = {"lwplsrda": (J.lwplsrda(X, y, **common), J.lwplsrda_predict), "lwplslda": (J.lwplslda(X, y, **common), J.lwplslda_predict),
          "lwplsqda": (J.lwplsqda(X, y, **common), J.lwplsqda_predict)}
res = {}
for name, (fm, pr) in models.items():
    res[name] = pr(fm, Xq, nlv=rng, ctx=ctx)
    info = np.asarray(res[name].info)
    stage(name + "_predict", dict(timed(lambda fm=fm, pr=pr: pr(fm, Xq, nlv=rng, ctx=ctx)), info_counts={int(v): int((info == v).sum()) for v in np.unique(info)}))

# the local scores of the same call, through the C ABI (the mirror does not ask for them)
from jchemo_hip import _lib
from jchemo_hip.plsr import _addr_ld, _lwplsr_prepared
st = models["lwplslda"][0].__dict__["_lw_engine"]
hd = _lwplsr_prepared(st["eng"], ctx, True, nlev)
tl = np.empty((m, k, nlv)); tq = np.empty((m, nlv)); code = np.empty((m, nlv), dtype=np.int32); info = np.empty((m, nlv), dtype=np.int32); post = np.empty((m, nlv, nlev))
ind = np.empty((m, k), dtype=np.int32)
xqa, ldxq = _addr_ld(Xq)
ctx.check(_lib.load().jch_lwplsda_predict_prepared(ctx._h, hd["handle"], st["cls"].data_ptr(), nlev, 1, 0, 1, None, 0, xqa, m, ldxq, k, 2.0, 1e-4, 0, 1, nlv, code.ctypes.data,
                                                   post.ctypes.data, info.ctypes.data, tl.ctypes.data, tq.ctypes.data, ind.ctypes.data, None, None))
T = torch.as_tensor(tl, device=dev); Tq = torch.as_tensor(tq, device=dev); cn = torch.as_tensor(y[ind], device=dev)
stage("knn_gda_lds_bytes", J.knn_gda_lds_bytes(k, nlv, nlev))
for kind in ("lda", "qda"):
    stage("jch_knn_gda_" + kind, timed(lambda kind=kind: J.knn_gda(T, Tq, cn, nlev, kind=kind, nlv=rng, ctx=ctx)))

if not a.skip_torch:
    oh = torch.nn.functional.one_hot(cn.long(), nlev).double()                 # m x k x nlev
    ni = oh.sum(dim=1)                                                         # m x nlev

    def torch_lda():
        mu = torch.einsum("mkc,mka->mca", oh, T) / ni.clamp(min=1)[:, :, None]                 # (an absent class: mean 0, masked below; its rows do not exist)
        D = T - torch.einsum("mkc,mca->mka", oh, mu)
        S = torch.einsum("mka,mkb->mab", D, D) / (k - (ni > 0).sum(dim=1)).double()[:, None, None]
        posts = []
        for a_ in rng:                                                         # once per a: the only other route on the device
            Lc = torch.linalg.cholesky_ex(S[:, :a_, :a_]).L                     # (no raise on a unanimous neighbourhood's zero matrix: those are not compared)
            z = torch.linalg.solve_triangular(Lc[:, None], (Tq[:, None, :a_] - mu[:, :, :a_])[..., None], upper=False)[..., 0]
            ld = -0.5 * (z ** 2).sum(dim=2) - torch.log(torch.diagonal(Lc, dim1=1, dim2=2)).sum(dim=1)[:, None]
            A = torch.exp(ld - ld.max(dim=1, keepdim=True).values) * (ni > 0)
            posts.append(A / A.sum(dim=1, keepdim=True))
        return torch.stack(posts, dim=1)
    pt = torch_lda().cpu().numpy()
    # compared where the yardstick's formula is the model: every class of the neighbourhood has two rows or more (it has no one-row rule) and was fitted
    full = (ni.cpu().numpy() != 1).all(axis=1)[:, None]
    ok = (info == 0) & np.isfinite(post).all(axis=2) & full & np.isfinite(pt).all(axis=2)
    stage("torch_lda_per_a", dict(timed(torch_lda), max_abs_posterior_difference=float(np.nanmax(np.abs(pt[ok] - post[ok]))), compared=int(ok.sum())))
stage("not_measured", ["k_locw_plskern share (kernel trace)", "lwplsrda against lwplsr_predict on the parent commit"])
print(json.dumps(out))
