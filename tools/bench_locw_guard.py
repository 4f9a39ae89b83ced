"""Regression guard of the p-space local-fit kernel (`k_locw_plskern`) with null score outputs: the device time of the batched local fits of
`lwplsr_predict` (profile field sweep_ms: HIP events around that one launch) at n = 1e5, p = 500, q = 1, k = 300, nlv = 15, 1000 queries, with
the neighbour-space kernel switched off (JCH_LOCW_KSPACE=0), for the library of the tree given by --tree.  Run it alternately for a build of the
parent commit and of this one ON ONE BOX and compare the medians with the run-to-run spread; prints one JSON line.

    JCH_LOCW_KSPACE=0 python tools/bench_locw_guard.py --tree TREE [--reps R] [--label NAME]
"""
import argparse, json, os, sys
ap = argparse.ArgumentParser()
ap.add_argument("--tree", required=True, help="root of the tree whose jchemo.jl_amd (mirror and built library) is measured")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--label", default="")
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--p", type=int, default=500)
ap.add_argument("--k", type=int, default=300)
ap.add_argument("--m", type=int, default=1000)
ap.add_argument("--nlv", type=int, default=15)
a = ap.parse_args()
os.environ["JCH_LOCW_KSPACE"] = "0"
sys.path[:0] = [os.path.join(os.path.abspath(a.tree), "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J

dev = torch.device("cuda", 0)
ctx = J.Context(0)
g = torch.Generator(device=dev); g.manual_seed(7)


def colmajor(t):
    o = torch.empty((t.shape[1], t.shape[0]), dtype=torch.float64, device=dev).t()
    o.copy_(t)
    return o


B = torch.randn((6, a.p), generator=g, device=dev, dtype=torch.float64)
X = colmajor(torch.randn((a.n, 6), generator=g, device=dev, dtype=torch.float64) @ B + 0.3 * torch.randn((a.n, a.p), generator=g, device=dev, dtype=torch.float64))
Y = colmajor(X[:, :3].sum(dim=1, keepdim=True) + 0.1 * torch.randn((a.n, 1), generator=g, device=dev, dtype=torch.float64))
Xq = colmajor(torch.randn((a.m, 6), generator=g, device=dev, dtype=torch.float64) @ B + 0.3 * torch.randn((a.m, a.p), generator=g, device=dev, dtype=torch.float64))
fm = J.lwplsr(X, Y, nlvdis=20, metric="mahal", h=2.0, k=a.k, nlv=a.nlv, ctx=ctx)
ctx.set_profiling(True)
J.lwplsr_predict(fm, Xq, nlv=range(0, a.nlv + 1), ctx=ctx)
ts = []
for _ in range(a.reps):
    J.lwplsr_predict(fm, Xq, nlv=range(0, a.nlv + 1), ctx=ctx)
    ts.append(ctx.profile().sweep_ms)
print(json.dumps(dict(label=a.label, lib=J.LIB_PATH, shape=dict(n=a.n, p=a.p, q=1, k=a.k, m=a.m, nlv=a.nlv), local_fits_ms=dict(median=float(np.median(ts)), min=float(min(ts)),
                                                                                                                         max=float(max(ts)), reps=a.reps))))
