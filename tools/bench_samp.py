"""Kennard-Stone / Duplex sampling on a device-resident X (uniform data from a seeded device generator).  One JSON line with HIP-event times around
whole calls, medians of --reps runs after one warm-up:
  * the max-min step of jch_maxmin_select at n = --n, p = --p and at p = --pscore (the score-space case), Kennard-Stone and Duplex: whole calls at
    two values of k and the time per step DERIVED from their difference (the calls share the staging-free start, the first pass and the result
    copy); the bytes of one read of X over that time; jch_transform with one score column on the same X in the same run as the one-read yardstick;
  * jch_farthest_pair at n = --npair (two sizes), p = --ppair: whole calls, n^2 p flop over that time; jch_kernel_gram (symmetric krbf: the same
    tile loop plus the n x n stores) at the smaller size in the same run;
  * `sampks` with k = --k at the smaller size against a literal device restatement of the reference's route — a torch n x n squared-distance matrix,
    then its loop over D[s][:, cand] — with the two selections compared.
Run it under a `timeout` of its own, as every GPU step.  Whoever runs it writes the numbers into DESIGN.md §19, the README and profiles/samp_bench.json.

    python tools/bench_samp.py [--n N] [--p P] [--pscore P] [--npair N1 N2] [--ppair P] [--k K] [--reps R] [--hbm-peak GBS] [--out FILE]
"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "jchemo.jl_amd")]
import numpy as np, torch
import jchemo_hip as J

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1000000)
ap.add_argument("--p", type=int, default=500)
ap.add_argument("--pscore", type=int, default=16)
ap.add_argument("--npair", type=int, nargs=2, default=[16384, 131072])
ap.add_argument("--ppair", type=int, default=512)
ap.add_argument("--k", type=int, default=1000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--hbm-peak", type=float, default=8000.0, help="GB/s (MI355X: 8 TB/s)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
dev = torch.device("cuda", 0)
ctx = J.Context(0, stream="torch")
L = J.load()


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1)


def median_ms(fn, reps):
    fn()                                  # warm-up: workspace growth, first-launch costs
    return float(np.median([event_ms(fn) for _ in range(reps)]))


def filled(n, p, seed):
    g = torch.Generator(device=dev); g.manual_seed(seed)
    X = J.colmajor_empty(n, p, dev)
    for c0 in range(0, p, 125):           # (in column blocks: no second n x p temporary)
        c1 = min(p, c0 + 125)
        X[:, c0:c1] = torch.rand((n, c1 - c0), dtype=torch.float64, device=dev, generator=g)
    torch.cuda.synchronize()
    return X


res = dict(metric="samp", device=torch.cuda.get_device_name(0), reps=a.reps, hbm_peak_gbs=a.hbm_peak)

# ---- the max-min step -------------------------------------------------------------------------------------------------------------------------
K1, K2 = 12, 52
for tag, p in (("wide", a.p), ("score", a.pscore)):
    n = a.n
    X = filled(n, p, 7)
    gb = n * p * 8 / 1e9
    xm, xs, R = np.zeros(p), np.ones(p), np.asfortranarray(np.random.default_rng(7).random((p, 1)))
    T = J.colmajor_empty(n, 1, dev)
    torch.cuda.synchronize()
    t_read = median_ms(lambda: ctx.check(L.jch_transform(ctx._h, 1, X.data_ptr(), n, p, n, xm.ctypes.data, xs.ctypes.data, R.ctypes.data, 1, T.data_ptr(), n)), a.reps)
    out = {f"{tag}_n": n, f"{tag}_p": p, f"{tag}_x_gb": round(gb, 3), f"{tag}_transform_one_column_ms": round(t_read, 3),
           f"{tag}_transform_gbs": round(gb / (t_read * 1e-3), 1)}
    init = np.array([0, 1, 2, 3], dtype=np.int64)
    for name, nsets in (("ks", 1), ("dp", 2)):
        t = {}
        for k in (K1, K2):
            sel = np.empty(k * nsets, dtype=np.int64)
            t[k] = median_ms(lambda: ctx.check(L.jch_maxmin_select(ctx._h, 1, X.data_ptr(), n, p, n, nsets, init.ctypes.data, k, sel.ctypes.data, None)), a.reps)
        step = (t[K2] - t[K1]) / (K2 - K1)
        out.update({f"{tag}_{name}_k{K1}_ms": round(t[K1], 3), f"{tag}_{name}_k{K2}_ms": round(t[K2], 3),
                    f"{tag}_{name}_step_ms_derived": round(step, 4), f"{tag}_{name}_step_gbs": round(gb / (step * 1e-3), 1),
                    f"{tag}_{name}_step_share_of_hbm_peak": round(gb / (step * 1e-3) / a.hbm_peak, 3),
                    f"{tag}_{name}_step_over_transform": round(step / t_read, 3)})
    res.update(out)
    del X, T
    torch.cuda.empty_cache()

# ---- the farthest pair ------------------------------------------------------------------------------------------------------------------------
p = a.ppair
pair, d2 = np.empty(2, dtype=np.int64), np.empty(1)
for n in a.npair:
    X = filled(n, p, 11)
    t_pair = median_ms(lambda: ctx.check(L.jch_farthest_pair(ctx._h, 1, X.data_ptr(), n, p, n, None, 0, pair.ctypes.data, d2.ctypes.data)), a.reps)
    res.update({f"pair_n{n}_p": p, f"pair_n{n}_ms": round(t_pair, 3), f"pair_n{n}_tflops": round(n * n * p / (t_pair * 1e-3) / 1e12, 2)})
    if n == min(a.npair):
        Kd = J.colmajor_empty(n, n, dev)
        torch.cuda.synchronize()
        t_gram = median_ms(lambda: ctx.check(L.jch_kernel_gram(ctx._h, 1, J._lib.KERN_RBF, X.data_ptr(), n, n, None, X.data_ptr(), n, n, None, p, 1.0 / p, 0.0, 1,
                                                                 Kd.data_ptr(), n)), a.reps)
        res.update({f"gram_krbf_sym_n{n}_ms": round(t_gram, 3), f"gram_krbf_sym_n{n}_tflops": round(n * n * p / (t_gram * 1e-3) / 1e12, 2),
                    f"pair_over_gram_n{n}": round(t_pair / t_gram, 3)})
        del Kd

        # ---- sampks against the reference's route restated on the device ----------------------------------------------------------------------
        k = a.k

        def torch_route():
            nrm = (X * X).sum(dim=1)
            D = (nrm[:, None] + nrm[None, :] - 2.0 * (X @ X.t())).clamp_(min=0)           # euclsq: the n x n matrix
            D = torch.triu(D, 1)                                                       # one triangle mirrored, as Distances.pairwise does for
            D = D + D.t()                                                              # (X, X): D == D' bitwise, which a GEMM does not give
            idx = int(torch.argmax(D.t().reshape(-1)))                                 # the first maximum of a column-major scan
            s = [idx % n, idx // n]
            mask = torch.ones(n, dtype=torch.bool, device=dev)
            mask[s] = False
            for _ in range(k - 2):
                cand = torch.nonzero(mask).reshape(-1)
                u = D[torch.as_tensor(s, device=dev)][:, cand].min(dim=0).values       # minimum(D[s, cand], dims = 1)
                zs = int(cand[int(torch.argmax(u))])
                s.append(zs)
                mask[zs] = False
            return np.array(s)

        t_ks = median_ms(lambda: J.sampks(X, k, ctx=ctx), max(1, a.reps // 2 + 1))
        t_ref = median_ms(torch_route, 1)
        same = bool(np.array_equal(J.sampks(X, k, ctx=ctx).train, torch_route()))
        res.update({f"sampks_n{n}_k": k, f"sampks_n{n}_ms": round(t_ks, 3), f"torch_nxn_route_n{n}_ms": round(t_ref, 3),
                    f"torch_route_over_sampks_n{n}": round(t_ref / t_ks, 2), f"sampks_equals_torch_route_n{n}": same})
    del X
    torch.cuda.empty_cache()

line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
