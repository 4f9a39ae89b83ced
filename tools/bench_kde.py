"""The kernel density family on the device, HIP-event times, medians of --reps runs after one warm-up, everything on device tensors.  One JSON line
(and --out FILE, by default profiles/kde_bench.json) with
  * `plskdeda_predict` at n = 16 384 training rows in 4 classes, nlv = 25, m = 4 096 queries, all 25 models (nlv = 1:25): the whole call
    (one transform, one jch_kde_dens, the posteriors) and the jch_kde_dens call alone, pair-models per second (m x n x 25 `exp` terms), and the
    share of the f64 vector rate that the `exp` count implies (EXP_FLOPS flops per `exp`, counted from the compiled kernel's instructions —
    see DESIGN.md §21 — over 78.6 TFLOP/s, the MI355X's f64 vector peak);
  * `dmkern_predict` at n = 16 384, m = 4 096 for p = 2 and p = 25;
  * the yardstick, in the same run: the same computation written in torch on the same GPU in float64 — per model and class
    `torch.cdist(...) ** 2`, `exp`, `sum`, over query chunks that fit memory — and the largest relative difference between the two.
Run it under a `timeout` of its own, as every GPU step.

    python tools/bench_kde.py [--n N] [--m M] [--nlv K] [--reps R] [--out FILE]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J
from jchemo_hip import kde as K

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=16384)
ap.add_argument("--m", type=int, default=4096)
ap.add_argument("--nlv", type=int, default=25)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kde_bench.json"))
a = ap.parse_args()
n, m, nlv, p, ncls = a.n, a.m, a.nlv, 200, 4
EXP_FLOPS = 30          # f64 flops of one library `exp` as compiled into k_kde_pairs: 1 mul, 13 fma (2 each), rndne, cvt, ldexp
F64_VECTOR_PEAK = 78.6e12
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, reps=a.reps):
    fn()                                  # warm-up: workspace growth, first-launch costs
    return float(np.median([event_ms(fn) for _ in range(reps)]))


def colmajor(t):
    out = J.colmajor_empty(t.shape[0], t.shape[1], dev); out.copy_(t)
    return out


def torch_dens(Z, cs, Xq, u, v2, coef, dims, chunk=1024):
    """The yardstick: out[i, c, a] by cdist ** 2, exp, sum per model and class, in query chunks."""
    out = torch.empty((Xq.shape[0], len(cs) - 1, len(dims)), dtype=torch.float64, device=dev)
    for c in range(len(cs) - 1):
        Zc = Z[cs[c]:cs[c + 1]] * u[:, c]
        Xc = Xq * u[:, c]
        for ia, d in enumerate(dims):
            Zd = Zc[:, :d].contiguous()
            for i0 in range(0, Xq.shape[0], chunk):
                D2 = torch.cdist(Xc[i0:i0 + chunk, :d].contiguous(), Zd) ** 2
                out[i0:i0 + chunk, c, ia] = coef[ia, c] * torch.exp(-0.5 * v2[ia, c] * D2).sum(dim=1)
    return out


g = torch.Generator(device=dev); g.manual_seed(20250607)
centres = torch.randn((ncls, nlv), generator=g, dtype=torch.float64, device=dev) * 1.5
yv = np.repeat(np.arange(ncls), n // ncls)
lat = centres[torch.as_tensor(yv, device=dev)] + torch.randn((n, nlv), generator=g, dtype=torch.float64, device=dev)
latq = centres[torch.as_tensor(np.arange(m) % ncls, device=dev)] + torch.randn((m, nlv), generator=g, dtype=torch.float64, device=dev)
A = torch.randn((nlv, p), generator=g, dtype=torch.float64, device=dev)
X = colmajor(lat @ A + 0.05 * torch.randn((n, p), generator=g, dtype=torch.float64, device=dev))
Xq = colmajor(latq @ A + 0.05 * torch.randn((m, p), generator=g, dtype=torch.float64, device=dev))
res = dict(metric="kde", device=torch.cuda.get_device_name(0), n=n, m=m, nlv=nlv, ncls=ncls, reps=a.reps, exp_flops=EXP_FLOPS)

# ---- 1. plskdeda_predict, all nlv models
obj = J.plskdeda(X, yv, nlv=nlv, ctx=ctx)
st = obj._kde
rng = list(range(1, nlv + 1))
T = J.transform(obj.fm_pls, Xq, nlv=nlv, ctx=ctx)
coef = np.array([[K._norm_coef(int(obj.ni[c]), k, obj.fm_da[k - 1].fm[c].detH) for c in range(ncls)] for k in rng])
t_call = median_ms(lambda: J.plskdeda_predict(obj, Xq, nlv=(1, nlv), ctx=ctx))
t_dens = median_ms(lambda: J.kde_dens(st["Z"], T, st["cs"], st["u"], st["v2"], coef, rng, ctx=ctx))
ut, vt, ct = (torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in (st["u"], st["v2"], coef))
Zc_, Tc_ = st["Z"].contiguous(), T.contiguous()
t_torch = median_ms(lambda: torch_dens(Zc_, st["cs"], Tc_, ut, vt, ct, rng), reps=max(2, a.reps // 2))
got = J.kde_dens(st["Z"], T, st["cs"], st["u"], st["v2"], coef, rng, ctx=ctx)
ref = torch_dens(Zc_, st["cs"], Tc_, ut, vt, ct, rng)
big = ref > 1e-280
pair_models = float(m) * n * nlv
res["plskdeda_predict"] = dict(
    whole_call_ms=round(t_call, 3), kde_dens_ms=round(t_dens, 3), torch_cdist_exp_sum_ms=round(t_torch, 3),
    ratio_torch_over_kde_dens=round(t_torch / t_dens, 2), pair_models_per_s=round(pair_models / (t_dens * 1e-3), 0),
    share_of_f64_vector_peak_from_exp_count=round(pair_models * EXP_FLOPS / (t_dens * 1e-3) / F64_VECTOR_PEAK, 4),
    max_rel_diff_to_torch=float(((got - ref).abs() / ref.abs())[big].max()))

# ---- 2. dmkern_predict
for pp in (2, 25):
    Z, Q = colmajor(lat[:, :pp]), colmajor(latq[:, :pp])
    fm = J.dmkern(Z, ctx=ctx)
    t = median_ms(lambda: J.dmkern_predict(fm, Q, ctx=ctx))
    hinv = torch.as_tensor(np.diag(fm.Hinv).reshape(pp, 1).copy(), device=dev)
    c1 = torch.as_tensor(np.array([[K._norm_coef(n, pp, fm.detH)]]), device=dev)
    one = torch.ones((1, 1), dtype=torch.float64, device=dev)
    Zc2, Qc2 = Z.contiguous(), Q.contiguous()
    tt = median_ms(lambda: torch_dens(Zc2, [0, n], Qc2, hinv, one, c1, [pp]), reps=max(2, a.reps // 2))
    res[f"dmkern_predict_p{pp}"] = dict(ms=round(t, 3), torch_cdist_exp_sum_ms=round(tt, 3), ratio_torch_over_ours=round(tt / t, 2),
                                        pairs_per_s=round(float(m) * n / (t * 1e-3), 0))

line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
ctx.close()
