"""jch_knn_wls and `lwmlr_predict` on the device: n = 16 384 training rows in d = 20 coordinates, q = 1 response, k = 100 neighbours, m = 4 096
queries, everything device-resident.  Host-clock times of windows of --inner back-to-back calls that end in a device synchronise, --reps windows after a warm-up: median, minimum
and maximum per call.  Every stage is printed as it finishes, then one JSON line (and --out FILE) with
  * jch_knn_wls alone (the row-major copy of [X | Y] and the local-fit kernel; device in, device out: the calls only enqueue);
  * the whole `lwmlr_predict` (search on the cached handle, weights, jch_knn_wls, the Python around them);
  * the comparison: `torch.linalg.lstsq` on the same GPU over the gathered, centred, sqrt(w)-scaled batch (m x k x d), timed alone and with the
    gather, centring, scaling and prediction around it; the largest difference between its predictions and the library's is reported;
  * the LDS bytes of one workgroup's slab and the workgroups per CU that leaves room for (of at most 8 of 256 threads).
No figure here is a pass condition.  Run it under a `timeout` of its own, as every GPU step.  Whoever runs it writes the numbers into DESIGN.md §23,
the README and profiles/lwmlr_bench.json.

    python tools/bench_lwmlr.py [--n N] [--m M] [--d D] [--k K] [--reps R] [--inner I] [--skip-torch] [--out FILE]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16384)
ap.add_argument("--m", type=int, default=4096)
ap.add_argument("--d", type=int, default=20)
ap.add_argument("--k", type=int, default=100)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--skip-torch", action="store_true", help="leave the torch.linalg.lstsq comparison out (it takes minutes: over a minute per call at the default shape)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, m, d, k, q = a.n, a.m, a.d, a.k, 1
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")
L = J.load()


def drain():
    ctx.synchronize(); torch.cuda.synchronize()         # (the ctx may own a stream of its own: an event on torch's stream would not see its kernels)


def window_ms(fn, inner):
    drain()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    drain()
    return 1e3 * (time.perf_counter() - t0) / inner


def stats(fn, inner=a.inner, reps=a.reps):
    fn(); drain()                                       # warm-up: workspace growth, first-launch costs
    ts = [window_ms(fn, inner) for _ in range(reps)]
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)), reps=reps, calls_per_window=inner)


out = {}


def stage(key, value):
    """Every finished stage is printed and written at once: a run that is cut short leaves what it had."""
    out[key] = value
    print(f"{key}: {json.dumps(value)}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


def colmajor(t):
    out = J.colmajor_empty(t.shape[0], t.shape[1], dev); out.copy_(t); return out


g = torch.Generator(device=dev); g.manual_seed(20240611)
cen = 3.0 * torch.randn(3, d, generator=g, device=dev, dtype=torch.float64)
X = colmajor(cen[torch.randint(0, 3, (n,), generator=g, device=dev)] + torch.randn(n, d, generator=g, device=dev, dtype=torch.float64))
Xq = colmajor(cen[torch.randint(0, 3, (m,), generator=g, device=dev)] + torch.randn(m, d, generator=g, device=dev, dtype=torch.float64))
Y = colmajor(4.0 + X @ torch.randn(d, q, generator=g, device=dev, dtype=torch.float64) + torch.sin(X[:, :1])
             + 0.3 * torch.randn(n, q, generator=g, device=dev, dtype=torch.float64))

fm = J.lwmlr(X, Y, h=2.0, k=k)
res = J.lwmlr_predict(fm, Xq, ctx=ctx)
ind, w = res.listnn, res.listw
pred = J.colmajor_empty(m, q, dev)
info = torch.empty(m, dtype=torch.int32, device=dev)
torch.cuda.synchronize()


def wls():
    ctx.check(L.jch_knn_wls(ctx._h, 1, X.data_ptr(), n, d, n, Y.data_ptr(), q, n, Xq.data_ptr(), m, m, ind.data_ptr(), w.data_ptr(), k, pred.data_ptr(),
                            info.data_ptr()))


stage("shape", dict(n=n, d=d, q=q, k=k, m=m, device=torch.cuda.get_device_name(0)))
lds = J.knn_wls_lds_bytes(k, d, q)
stage("lds", dict(bytes_per_workgroup=lds, workgroups_per_cu_by_lds=max(1, min(8, (160 * 1024) // lds))))
stage("jch_knn_wls", stats(wls))
ctx.synchronize()
assert bool((info == 0).all()) and bool(torch.equal(pred, res.pred))
stage("lwmlr_predict", stats(lambda: J.lwmlr_predict(fm, Xq, ctx=ctx), inner=max(1, a.inner // 4)))


# ---- the comparison: the same fits through torch.linalg.lstsq on the gathered, centred, scaled batch
def batch():
    idx = ind.long()
    wn = w / w.sum(dim=1, keepdim=True)
    Xs, Ys = X[idx], Y[idx]                              # m x k x d, m x k x q
    xbar = (wn[:, :, None] * Xs).sum(dim=1); ybar = (wn[:, :, None] * Ys).sum(dim=1)
    sw = wn.sqrt()[:, :, None]
    return sw * (Xs - xbar[:, None, :]), sw * (Ys - ybar[:, None, :]), xbar, ybar


def torch_route():
    A, B, xbar, ybar = batch()
    beta = torch.linalg.lstsq(A, B).solution
    return ybar + torch.einsum("md,mdq->mq", Xq - xbar, beta)


try:
    if a.skip_torch:
        raise RuntimeError("skipped (--skip-torch)")
    A, B, _, _ = batch()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    ref = torch_route()                                  # the first call on its own clock: torch's batched lstsq may loop over the m matrices on the host
    torch.cuda.synchronize(); first_s = time.perf_counter() - t0
    stage("torch_first_call_s", first_s)
    stage("max_abs_difference_to_torch", dict(diff=float((ref - res.pred).abs().max()), prediction_scale=float(res.pred.abs().max())))
    few = dict(inner=1, reps=3) if first_s > 0.25 else dict(inner=max(1, a.inner // 4))   # (windows of one call where a call is long in itself:
    # 74 s per call were measured at the default shape, where torch's batched lstsq walks the 4 096 matrices one at a time)
    stage("torch_lstsq_alone", stats(lambda: torch.linalg.lstsq(A, B), **few))
    stage("torch_gather_centre_lstsq_predict", stats(torch_route, **few))
except Exception as e:                                   # (a driver torch.linalg.lstsq lacks on this build is recorded, not hidden)
    stage("torch_lstsq_error", f"{type(e).__name__}: {e}")

print(json.dumps(out))
