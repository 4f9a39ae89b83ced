"""The kNN family on the device at the cfg5 shapes (BASELINE.json configs[4]: n = 1e5, p = 500, 20 global LVs, k = 200, 1000 queries), X on the device,
HIP-event times, medians of --reps runs after one warm-up.  One JSON line (and --out FILE) with
  * jch_knn_search on the cfg5 search space (the whitened scores of the lwplsr model) with device outputs, beside the kNN stage of
    jch_lwplsr_predict_prepared in the same run — from its profile, prologue_ms - smallstate_ms — measured twice, so that the spread between two
    repeats of the yardstick is on record; the same search on the raw spectra (nlvdis = 0: 500 columns, the exact vector scan);
  * `occlknndis` predict at m = 1000, n = 1e5, nlv = 30 for k = 5 and k = 100 with a cold and a warm cache, beside the reference's route restated in
    torch on the device (k + 1 brute-force searches per query, each over a row-removed copy of the scores), which is timed on a SAMPLE of the
    queries and scaled to m (the key says so);
  * jch_knn_wmean (q = 1 and q = 10) and jch_knn_vote at m = 1000, k = 200 against the bytes they gather.
Run it under a `timeout` of its own, as every GPU step.  Whoever runs it writes the numbers into DESIGN.md §20, the README and
profiles/knn_bench.json.

    python tools/bench_knn.py [--n N] [--m M] [--reps R] [--out FILE]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J
from jchemo_hip import knn as K
from jchemo_hip.plsr import _knn_train_space

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100000)
ap.add_argument("--m", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()
n, m, p, k, nlvdis = a.n, a.m, 500, 200, 20
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")
L = J.load()


def event_ms(fn):
    # the ctx may own a stream of its own: every timed call ends synchronised with it (the wrappers do that themselves, the raw entries through
    # `synced`), so the events on torch's stream bracket all of its kernels; the price is one host round trip per call, inside the time
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def synced(status):
    ctx.check(status)
    ctx.synchronize()


def median_ms(fn, reps=a.reps, before=None):
    fn()                                  # warm-up: workspace growth, first-launch costs
    ts = []
    for _ in range(reps):
        if before:
            before()
        ts.append(event_ms(fn))
    return float(np.median(ts))


def gen(rows, seed, r=30):                # the inputs of tools/bench_lwplsr.py: 30 latent sources + noise
    S = J.colmajor_empty(rows, r, dev); E = J.colmajor_empty(rows, p, dev)
    ctx.check(L.jch_fill_uniform(ctx._h, S.data_ptr(), rows, r, rows, 0, rows, seed))
    ctx.check(L.jch_fill_uniform(ctx._h, E.data_ptr(), rows, p, rows, 0, rows, seed + 100))
    Lm = J.colmajor_empty(r, p, dev); ctx.check(L.jch_fill_uniform(ctx._h, Lm.data_ptr(), r, p, r, 0, r, 777))
    out = J.colmajor_empty(rows, p, dev); out.copy_(S @ Lm + 0.1 * E)
    return out


X, Xq = gen(n, 20250112), gen(m, 20250115)
beta = torch.zeros(p, dtype=torch.float64, device=dev); beta[:5] = torch.tensor([1.0, -2.0, 0.5, 3.0, 1.5], dtype=torch.float64)
y = J.colmajor_empty(n, 1, dev); y.copy_((X @ beta + torch.sin(3 * X[:, 5])).reshape(-1, 1))
res = dict(metric="knn", device=torch.cuda.get_device_name(0), n=n, m=m, p=p, reps=a.reps)

# ---- 1. the search at the cfg5 shape, beside the kNN stage of the prepared lwplsr predict
fm = J.lwplsr(X, y, nlvdis=nlvdis, metric="mahal", h=1.0, k=k, nlv=15, ctx=ctx)
J.predict(fm, Xq, ctx=ctx)
ctx.set_profiling(True)


def knn_stage_ms():
    ts = []
    for _ in range(a.reps):
        J.predict(fm, Xq, ctx=ctx)
        pr = ctx.profile()
        ts.append(pr.prologue_ms - pr.smallstate_ms)
    return float(np.median(ts))


y1, y2 = knn_stage_ms(), knn_stage_ms()
ctx.set_profiling(False)
Zt, qmap, _ = _knn_train_space(fm, ctx)
Zq = qmap(Xq)
hnd = K.knn_prepare(Zt, ctx)
ind = torch.empty((m, k), dtype=torch.int32, device=dev); dist = torch.empty((m, k), dtype=torch.float64, device=dev); w = torch.empty_like(dist)
torch.cuda.synchronize()
search = lambda: synced(L.jch_knn_search(ctx._h, hnd, 1, Zq.data_ptr(), m, m, k, None, 1.0, 1e-4, 1, ind.data_ptr(), dist.data_ptr(), w.data_ptr(), None))  # noqa: E731
s1, s2 = median_ms(search), median_ms(search)
sr = torch.arange(m, device=dev, dtype=torch.int64)
torch.cuda.synchronize()
search_self = lambda: synced(L.jch_knn_search(ctx._h, hnd, 1, Zq.data_ptr(), m, m, k, sr.data_ptr(), 1.0, 1e-4, 1, ind.data_ptr(), dist.data_ptr(), w.data_ptr(), None))  # noqa: E731
s_self = median_ms(search_self)
K.knn_release(hnd)
res.update(search_shape=f"n={n} dd={Zt.shape[1]} k={k} m={m}", lwplsr_knn_stage_ms=[round(y1, 4), round(y2, 4)], knn_search_ms=[round(s1, 4), round(s2, 4)],
           knn_search_with_self_ms=round(s_self, 4), yardstick_spread_ms=round(abs(y1 - y2), 4), search_minus_yardstick_ms=round(min(s1, s2) - min(y1, y2), 4))
hraw = K.knn_prepare(X, ctx)
torch.cuda.synchronize()
raw = lambda: synced(L.jch_knn_search(ctx._h, hraw, 1, Xq.data_ptr(), m, m, k, None, 1.0, 1e-4, 1, ind.data_ptr(), dist.data_ptr(), w.data_ptr(), None))  # noqa: E731
res.update(raw_spectra_search_ms=round(median_ms(raw, reps=3), 3), raw_spectra_shape=f"n={n} dd={p} k={k} m={m} (exact vector scan)")
K.knn_release(hraw)
del fm, Zt, Zq

# ---- 2. wmean / vote against the bytes they gather
gi = torch.randint(0, n, (m, k), dtype=torch.int32, device=dev)
gw = torch.rand((m, k), dtype=torch.float64, device=dev) + 1e-4
for q in (1, 10):
    Yq = J.colmajor_empty(n, q, dev); Yq.copy_(torch.rand((n, q), dtype=torch.float64, device=dev))
    pred = J.colmajor_empty(m, q, dev)
    torch.cuda.synchronize()
    t = median_ms(lambda: synced(L.jch_knn_wmean(ctx._h, 1, Yq.data_ptr(), n, q, n, gi.data_ptr(), gw.data_ptr(), m, k, pred.data_ptr())))
    gb = m * k * (8 * q + 12) / 1e9
    res[f"wmean_q{q}_ms"] = round(t, 4); res[f"wmean_q{q}_gathered_gbs"] = round(gb / (t * 1e-3), 1)
cls = torch.randint(0, 10, (n,), dtype=torch.int32, device=dev)
vp = torch.empty(m, dtype=torch.int32, device=dev)
torch.cuda.synchronize()
t = median_ms(lambda: synced(L.jch_knn_vote(ctx._h, 1, cls.data_ptr(), n, 10, gi.data_ptr(), gw.data_ptr(), m, k, vp.data_ptr(), None)))
res.update(vote_ncls10_ms=round(t, 4), vote_gathered_gbs=round(m * k * 16 / 1e9 / (t * 1e-3), 1))

# ---- 3. occlknndis predict, cold and warm, beside the reference's route in torch
nlv = 30
samp = np.random.default_rng(1).choice(n, size=50, replace=False)


def mid(v):
    """Julia's `median`: `middle` of the two central values for an even count (`torch.median` returns the lower one)."""
    s_ = torch.sort(v).values
    c = s_.shape[0]
    return s_[c // 2] if c % 2 else s_[c // 2 - 1] / 2 + s_[c // 2] / 2


def torch_reference_route(T, Tq, kk, rows):
    """src/occlknndis.jl:178-194 on the device for the queries `rows`: per query one search over T, then kk searches, each over rmrow(T, zind)."""
    nT = T.shape[0]
    out = []
    for i in rows:
        d = torch.sqrt(((T - Tq[i]) ** 2).sum(dim=1))
        dd, ii = torch.topk(d, kk, largest=False, sorted=True)
        vd = []
        for j in ii.tolist():
            keep = torch.ones(nT, dtype=torch.bool, device=T.device); keep[j] = False
            Tr = T[keep]                                                  # rmrow: a fresh copy
            dj = torch.sqrt(((Tr - T[j]) ** 2).sum(dim=1))
            vd.append(mid(torch.topk(dj, kk, largest=False).values))
        out.append(mid(dd) / mid(torch.stack(vd)))
    return torch.stack(out)


for kk, nsample in ((5, 20), (100, 3)):
    obj = J.occlknndis(X, nlv=nlv, k=kk, samp=samp, ctx=ctx)
    st = K._occ_handle(obj, ctx)
    cold = median_ms(lambda: J.predict(obj, Xq, ctx=ctx), before=lambda: st["dk_train"].fill_(float("nan")))
    warm = median_ms(lambda: J.predict(obj, Xq, ctx=ctx))
    Tq = K._occ_query(obj, Xq, ctx)
    Tc, Tqc = obj.T.contiguous(), Tq.contiguous()
    rows = list(range(nsample))
    t_ref = median_ms(lambda: torch_reference_route(Tc, Tqc, kk, rows), reps=2)
    got = J.predict(obj, Xq, ctx=ctx).d["d"][:nsample]
    ref = torch_reference_route(Tc, Tqc, kk, rows)
    res[f"occlknndis_k{kk}"] = dict(predict_cold_ms=round(cold, 3), predict_warm_ms=round(warm, 3),
                                    torch_reference_route_ms_scaled_from_sample=round(t_ref * m / nsample, 1), sample_queries=nsample,
                                    ratio_reference_over_cold=round(t_ref * m / nsample / cold, 1), ratio_reference_over_warm=round(t_ref * m / nsample / warm, 1),
                                    max_rel_diff_on_sample=float(((got - ref).abs() / ref.abs()).max()))
    del obj, st

line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
ctx.close()
