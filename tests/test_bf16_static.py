"""The bf16 storage mode of plskern at its row, column and tile boundaries, without a GPU: the case table and the data builder of
tests/test_gpu_bf16_edges.py, a restatement of the dispatch of jch_fit_plskern_bf16 (csrc/bf16.hip) that says which kernels a case enters,
and the two conditions that give the mode's existing budget (1e-3 on T, P, C, W, R; 1e-4 on B = R C') power on these data.

The data.  The seeded uniform base of the other bf16 tests, plus sentinels: a sentinel COLUMN j is multiplied by 4 and half of it is added to (or
taken from) one response; a sentinel ROW r is multiplied by 8 with a sign per column and gets +-2 in every response.  Everything is rounded to bf16
through torch.bfloat16 and the rounded values, as Float64, are what the oracle sees.  The sentinels sit where the kernels change what they do: the
first and last row of a 64- or 128-row tile, of an 8-row group, of a shard; the first and last column of a 64-column piece, of a 512-column
group, of the 8-column pad.

Power (test_power).  The oracle fit WITHOUT one sentinel row (the row deleted, its weight with it), or with one sentinel column replaced by fresh
uniform noise, must differ from the full oracle fit by at least 100 times the gate of the GPU test: 1e-2 on B (gate 1e-4), and on the sign-aligned
first weight vector 2e-3 where its gate is 2e-5 (the bf16 matrix pipe), 1e-7 where it is 1e-9.  Deletion and replacement stand in for "this element
never reached the sums": a kernel that skips, duplicates or mis-weights a boundary row, or that maps a lane to the wrong column, moves the result
at least as much as leaving the element out moves it, by construction of the amplitudes.  Only the oracle enters this proof.

Benign data (test_benign).  A CPU model of the mode's arithmetic (f64 statistics and X'DY; scores from f32 dot products of the raw bf16 rows with
f32(r / scale); X'Dt from f32 running sums per wave over interleaved row groups; the centring fix-up in f64) stays within 3e-5 of the oracle on T,
P, C, W, R, on B and on max_i |dT|_ia / max_i |T|_ia: 30 times under the loosest budget, so a failure on the device cannot be blamed on the
conditioning of the case.  This is a condition on the inputs, never a gate on the device.

If a case misses a condition its amplitudes or its nlv change; the budgets do not."""
import os
import re
from functools import lru_cache
from typing import NamedTuple, Optional, Tuple

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import c_oracle as CO  # noqa: E402
from oracle import plsr_oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16_HIP = os.path.join(ROOT, "jchemo.jl_amd", "csrc", "bf16.hip")

# ---- the gates of tests/test_gpu_bf16_edges.py (the budgets the mode already has) and what the power condition asks of the data
BUDGET, BUDGET_B = 1e-3, 1e-4          # sign-aligned relative Frobenius error on T, P, C, W, R; on B = R C'
TIGHT, W1_PIPE = 1e-9, 2e-5            # first weight vector: f64 products; the bf16 matrix pipe (test_bf16_prologue_on_the_bf16_matrix_pipe)
POWER = 100.0
BENIGN = 3e-5
SWEEP_MAXP = 2048                      # jch_internal.h JCH_SWEEP_MAXP: wider inputs are widened to Float64 (fit.hip)
COL_AMP, COL_SHARE, ROW_AMP, ROW_Y = 4.0, 0.5, 8.0, 2.0


def roundup(v, m):
    return (v + m - 1) // m * m


class Case(NamedTuple):
    name: str
    n: int
    p: int
    q: int
    nlv: int
    weights: bool
    scal: bool
    rows: Tuple[int, ...]
    cols: Tuple[int, ...]
    branch: str                        # what route() must say
    decided_by: Tuple[str, ...]        # the expressions of jch_fit_plskern_bf16 (fit.hip where marked) that send the case there
    env: Tuple[Tuple[str, str], ...] = ()
    ld: Optional[int] = None           # leading dimension of X and Y (default: n rounded up to 8)
    shift: int = 0                     # elements between a 16-byte boundary and the first element (1: a view from row 1 of an aligned parent)
    cuts: Optional[Tuple[int, ...]] = None     # row-sharded over len(cuts) - 1 loopback ranks

    @property
    def ldx(self):
        return roundup(self.n + self.shift, 8) if self.ld is None else self.ld


# Line numbers: csrc/bf16.hip as of this change (n_total 1184, raw_b 1194, v8 1213, the knobs 1216-1217, panel_ok / panel 1219-1220, m32 1225,
# the tails 1234 / 1259, the sweeps 1321-1323, fast / generic 1327 / 1337-1341); fit.hip 195 (widening), 336 (fastb).
# test_decisions_are_still_in_the_source keeps the expressions honest when the numbers drift.
RAW = "const bool raw_b = !d.scal && q <= 15 && ldx % 8 == 0 && ((uintptr_t)Xc) % 16 == 0"
V8 = "const bool v8 = ldx % 8 == 0 && ((uintptr_t)Xc) % 16 == 0;"
PANEL = "const bool panel_ok = k2panel && v8 && qpad == 16 && ldy % 8 == 0"
NFULL = "const bool panel = panel_ok && nfull > 0;"
M32 = "m32 = panel_ok && raw_b && !wdev && jch_knob(\"JCH_BF16_K2_M32\", 1) != 0 && NHv == 2 && (nfull > 0 || ctx->nranks > 1);"
NH = "jch_knob(\"JCH_BF16_K2_NH\", 2) == 4 ? 4 : 2"
K2P = "jch_knob(\"JCH_BF16_K2_PANEL\", 1)"
TAIL = "const bool tail = nfull < n;"
SW1, SW2, SW4 = "if (ldr_b <= 512) JCH_TRY((launch_sweep_bf16_v2_t<1, 8>", "else if (ldr_b <= 1024) JCH_TRY((launch_sweep_bf16_v2_t<2, 8>", \
    "else JCH_TRY((launch_sweep_bf16_t<4, 2>"
GENERIC = "hipLaunchKernelGGL(k_bf16_fix_zt"
NTOTAL = "if (ctx->nranks > 1 && n < std::min<int64_t>(p, d.nlv))"
RANKS = "ctx->nranks > 1"
ROWS_A = (0, 63, 64, 191, 192, 196)
COLS_A = (0, 7, 8, 76)
ROWS_B = (0, 127, 128, 255, 256, 260)

CASES = [
    Case("pipe", 197, 77, 2, 3, False, False, ROWS_A, COLS_A, "raw; matrix-pipe panel + its tail kernel; sweep <1,8>; fast",
         (RAW, PANEL, M32, TAIL, SW1)),
    Case("panel-nh2", 197, 520, 3, 3, True, False, (0, 191, 192, 196), (0, 511, 512, 519), "raw; f64 panel NH=2 + 16-byte tile tail; sweep <2,8>; fast",
         (RAW, PANEL, M32, NFULL, SW2)),
    Case("panel-nh4", 197, 520, 3, 3, True, False, (0, 191, 192, 196), (0, 511, 512, 519), "raw; f64 panel NH=4 + 16-byte tile tail; sweep <2,8>; fast",
         (NH, NFULL, PANEL), env=(("JCH_BF16_K2_NH", "4"),)),
    Case("pipe-off", 197, 77, 2, 3, False, False, ROWS_A, COLS_A, "raw; f64 panel NH=2 + 16-byte tile tail; sweep <1,8>; fast",
         (M32, PANEL), env=(("JCH_BF16_K2_M32", "0"),)),
    Case("panel-off", 197, 77, 2, 3, False, False, ROWS_A, COLS_A, "raw; 16-byte tile kernel; sweep <1,8>; fast",
         (K2P, PANEL, V8), env=(("JCH_BF16_K2_PANEL", "0"),)),
    Case("q16-scal", 261, 130, 16, 3, True, True, ROWS_B, (0, 129), "centred; f64 panel NH=2 + 16-byte tile tail; sweep <1,8>; fast",
         (RAW, PANEL, NFULL, SW1)),
    Case("q15-ones-last", 261, 130, 15, 3, False, False, ROWS_B, (0, 129), "raw; matrix-pipe panel + its tail kernel; sweep <1,8>; fast",
         (RAW, PANEL, M32, TAIL)),
    Case("no-full-tile", 37, 77, 2, 3, False, True, (0, 7, 8, 36), (0, 76), "centred; 16-byte tile kernel; sweep <1,8>; fast",
         (NFULL, PANEL, V8)),
    Case("q17-wide", 133, 1030, 17, 3, True, False, (0, 132), (1023, 1024, 1029), "centred; 16-byte tile kernel; sweep <4,2>; generic",
         (RAW, PANEL, SW4, GENERIC, "const bool fastb = q <= 16 && p <= JCH_SWEEP_MAXP  [fit.hip]")),
    Case("p2048", 133, 2048, 2, 3, False, False, (0, 132), (1023, 1024, 2047), "raw; matrix-pipe panel + its tail kernel; sweep <4,2>; fast",
         (M32, SW4)),
    Case("p2050-widened", 133, 2050, 2, 3, False, False, (0, 132), (0, 2049), "widened to Float64",
         ("io.d->dtype == JCH_BF16 && (algo != ALGO_KERN || io.d->p > JCH_SWEEP_MAXP)  [fit.hip]",)),
    Case("n9", 9, 24, 1, 2, False, False, (7, 8), (0, 23), "raw; 16-byte tile kernel; sweep <1,8>; fast", (NFULL, PANEL, V8, SW1)),
    Case("n8", 8, 24, 1, 2, False, False, (7,), (0, 23), "raw; 16-byte tile kernel; sweep <1,8>; fast", (NFULL, PANEL, V8, SW1)),
    Case("n7", 7, 24, 1, 2, False, False, (6,), (0, 23), "raw; 16-byte tile kernel; sweep <1,8>; fast", (NFULL, PANEL, V8, SW1)),
    Case("odd-ld", 197, 77, 2, 3, False, False, ROWS_A, COLS_A, "centred; scalar tile kernel; sweep <1,8>; fast", (RAW, V8), ld=197),
    Case("row1-view", 197, 77, 2, 3, False, False, ROWS_A, COLS_A, "centred; scalar tile kernel; sweep <1,8>; fast", (RAW, V8), shift=1),
    Case("shards-64-5-128", 197, 77, 2, 3, False, False, (63, 64, 68, 69), (),
         "3 ranks: raw; matrix-pipe panel | raw; matrix-pipe tail kernel alone | raw; matrix-pipe panel; sweep <1,8>; fast",
         (M32, RANKS, NFULL), cuts=(0, 64, 69, 197)),
    Case("shards-64-5-128-w", 197, 77, 2, 3, True, False, (63, 64, 68, 69), (),
         "3 ranks: raw; f64 panel NH=2 | raw; 16-byte tile kernel | raw; f64 panel NH=2; sweep <1,8>; fast",
         (M32, PANEL, NFULL), cuts=(0, 64, 69, 197)),
    Case("shards-3-97-97", 197, 77, 2, 5, False, False, (0, 2, 3), (),
         "3 ranks: raw; matrix-pipe tail kernel alone | raw; matrix-pipe panel + its tail kernel | raw; matrix-pipe panel + its tail kernel; "
         "sweep <1,8>; fast", (NTOTAL, M32, RANKS), cuts=(0, 3, 100, 197)),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]


# ---- the dispatch, restated ---------------------------------------------------------------------------------------------------------------------
def _prologue(c, n, ld, aligned, nranks):
    """The X'DY kernels of one rank with n rows (jch_fit_plskern_bf16, `---- prologue`).  weights_norm, T and Y are 16-byte aligned in these tests and
    Y has X's leading dimension."""
    env = dict(c.env)
    qpad = roundup(c.q, 16)
    v8 = ld % 8 == 0 and aligned
    raw = not c.scal and c.q <= 15 and v8
    nh = 4 if env.get("JCH_BF16_K2_NH") == "4" else 2
    nfull = n // (32 * nh) * (32 * nh)
    panel_ok = env.get("JCH_BF16_K2_PANEL", "1") != "0" and v8 and qpad == 16
    pipe = panel_ok and raw and not c.weights and env.get("JCH_BF16_K2_M32", "1") != "0" and nh == 2 and (nfull > 0 or nranks > 1)
    head = "raw; " if raw else "centred; "
    if pipe:
        return head + ("matrix-pipe tail kernel alone" if nfull == 0 else "matrix-pipe panel" + (" + its tail kernel" if nfull < n else "")), True
    if panel_ok and nfull > 0:
        return head + f"f64 panel NH={nh}" + (" + 16-byte tile tail" if nfull < n else ""), False
    return head + ("16-byte tile kernel" if v8 else "scalar tile kernel"), False


def route(c):
    """(the branch of the case in words, whether X'DY comes from the bf16 matrix pipe)."""
    if c.p > SWEEP_MAXP:
        return "widened to Float64", False
    ldr_b = roundup(c.p, 8)
    sweep = "<1,8>" if ldr_b <= 512 else "<2,8>" if ldr_b <= 1024 else "<4,2>"
    state = "fast" if c.q <= 16 else "generic"
    if c.cuts is None:
        pro, pipe = _prologue(c, c.n, c.ldx, c.shift == 0, 1)
        return f"{pro}; sweep {sweep}; {state}", pipe
    parts = [_prologue(c, b - a, roundup(b - a, 8), True, len(c.cuts) - 1) for a, b in zip(c.cuts[:-1], c.cuts[1:])]
    assert len({pp for _, pp in parts}) == 1, "the ranks of a sharded fit must all sum the same quantity into X'DY"
    return f"{len(parts)} ranks: " + " | ".join(t for t, _ in parts) + f"; sweep {sweep}; {state}", parts[0][1]


def sweep_rows(c):
    """Rows per wave iteration of the sweep the case takes (k_sweep_bf16_v2: 8, the round-1 k_sweep_bf16<4, 2>: 2)."""
    return 8 if roundup(c.p, 8) <= 1024 else 2


# ---- data ---------------------------------------------------------------------------------------------------------------------------------------
def bf16_round(A):
    """Round to nearest even to bf16, back as Float64 (exact)."""
    return torch.from_numpy(np.ascontiguousarray(A, dtype=np.float64)).to(torch.bfloat16).to(torch.float64).numpy()


@lru_cache(maxsize=None)
def _data(n, p, q, rows, cols):
    X = CO.fill_uniform(20250112, n, p)
    Y = CO.fill_uniform(20250113, n, q)
    rng = np.random.default_rng(1000003 * n + 1009 * p + q)
    for i, j in enumerate(cols):                     # sentinel column j, served by response i mod q
        X[:, j] *= COL_AMP
        Y[:, i % q] += rng.choice([-1.0, 1.0]) * COL_SHARE * X[:, j]
    for r in rows:                                   # sentinel row r
        X[r, :] = ROW_AMP * rng.choice([-1.0, 1.0], p) * X[r, :]
        Y[r, :] = ROW_Y * rng.choice([-1.0, 1.0], q)
    X, Y = np.asfortranarray(bf16_round(X)), np.asfortranarray(bf16_round(Y))
    fresh = np.asfortranarray(bf16_round(rng.random((n, max(1, len(cols))))))    # what replaces a sentinel column in the power condition
    for a in (X, Y, fresh):
        a.setflags(write=False)
    return X, Y, fresh


def case_data(c):
    """(X, Y, weights or None): the bf16-rounded inputs as Float64, read-only and shared between the tests."""
    X, Y, _ = _data(c.n, c.p, c.q, c.rows, c.cols)
    return X, Y, case_weights(c)


def case_weights(c):
    return 0.25 + O.splitmix64_uniform(7, 0, c.n) if c.weights else None


@lru_cache(maxsize=None)
def _oracle(n, p, q, rows, cols, nlv, weights, scal):
    c = Case("", n, p, q, nlv, weights, scal, rows, cols, "", ())
    X, Y, w = case_data(c)
    return O.plskern(X, Y, w, nlv=nlv, scal=scal)


def oracle(c):
    """The Float64 fit of the rounded inputs, computed once per data set and shared (do not modify)."""
    return _oracle(c.n, c.p, c.q, c.rows, c.cols, c.nlv, c.weights, c.scal)


# ---- comparisons --------------------------------------------------------------------------------------------------------------------------------
def coef(fm):
    return fm.R @ fm.C.T


def errors(ref, T, P, C, W, R):
    """The figures of the GPU test: sign-aligned relative Frobenius errors, B, the first weight vector, the scores in the max norm per LV."""
    s = O.sign_align(ref.W, W)
    e = {f: O.rel_fro(getattr(ref, f), g * s) for f, g in (("T", T), ("P", P), ("C", C), ("W", W), ("R", R))}
    e["B"] = O.rel_fro(coef(ref), R @ C.T)
    e["w1"] = O.rel_fro(ref.W[:, 0], W[:, 0] * s[0])
    e["Tmax"] = float(np.max(np.max(np.abs(ref.T - T * s), axis=0) / np.max(np.abs(ref.T), axis=0)))
    return e


# ---- the CPU model of the mode ------------------------------------------------------------------------------------------------------------------
def model_fit(X, Y, w, nlv, scal, R):
    """plskern as the bf16 mode computes it (csrc/bf16.hip, header): f64 statistics and X'DY from the exact bf16 values; per LV t_i = f32 dot
    product of the raw row with rt = f32(r / scale), minus f32(sum_j mean_j rt_j); X'Dt as f32 running sums, one per wave, over the wave's row
    groups (R rows each, group g with wave g mod (4 blocks)), added in f64; zp = (sum - mean * sum_i d_i t_i) / scale in f64."""
    f32 = np.float32
    n, p = X.shape
    d = O.mweight(np.ones(n) if w is None else w)
    xm, ym = d @ X, d @ Y
    xs = np.sqrt(d @ (X - xm) ** 2) if scal else np.ones(p)
    ys = np.sqrt(d @ (Y - ym) ** 2) if scal else np.ones(Y.shape[1])
    K = ((X - xm) / xs).T @ (d[:, None] * ((Y - ym) / ys))
    nlv = min(n, p, nlv)
    X32 = X.astype(f32)                                                 # exact
    ngroups = (n + R - 1) // R
    nwaves = 4 * max(1, (ngroups + 3) // 4)
    T, W, P, Rm, C = np.empty((n, nlv)), np.empty((p, nlv)), np.empty((p, nlv)), np.empty((p, nlv)), np.empty((Y.shape[1], nlv))
    d32 = d.astype(f32)
    for a in range(nlv):
        wv = O.dominant_left_sv(K)
        r = wv.copy()
        for j in range(a):
            r -= np.dot(wv, P[:, j]) * Rm[:, j]
        rt = (r / xs).astype(f32)
        off = f32(np.dot(xm, rt.astype(np.float64)))
        t = np.array([np.dot(X32[i], rt) for i in range(n)], dtype=f32) - off
        dt = d32 * t
        zp, tt, st = np.zeros(p), 0.0, 0.0
        for wave in range(min(nwaves, ngroups)):
            acc = np.zeros(p, dtype=f32)
            for g in range(wave, ngroups, nwaves):
                ttg, stg = f32(0), f32(0)
                for i in range(g * R, min(n, (g + 1) * R)):
                    acc += dt[i] * X32[i]
                    ttg += dt[i] * t[i]
                    stg += dt[i]
                tt += float(ttg)
                st += float(stg)
            zp += acc.astype(np.float64)
        zp = (zp - xm * st) / xs
        c = (K.T @ r) / tt
        K = K - np.outer(zp, c)
        P[:, a], T[:, a], W[:, a], Rm[:, a], C[:, a] = zp / tt, t.astype(np.float64), wv, r, c
    return T, P, C, W, Rm


# ---- tests --------------------------------------------------------------------------------------------------------------------------------------
def test_the_table_is_the_issue_s():
    assert len(CASES) == len(set(IDS)) == 19
    for c in CASES:
        assert all(0 <= r < c.n for r in c.rows) and all(0 <= j < c.p for j in c.cols) and (c.rows or c.cols), c.name
        assert c.ldx >= c.n + c.shift and (c.cuts is None or (c.cuts[0] == 0 and c.cuts[-1] == c.n and not c.cols)), c.name
    assert BY_NAME["odd-ld"].ldx % 8 != 0 and BY_NAME["row1-view"].ldx % 8 == 0 and BY_NAME["pipe"].ldx == 200
    sh = BY_NAME["shards-3-97-97"]
    assert sh.cuts[1] - sh.cuts[0] < min(sh.p, sh.nlv), "the first shard must be smaller than nlv (the n_total read-back)"


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_route(c):
    """Every case enters the branch the table says, by the restated dispatch."""
    assert route(c)[0] == c.branch


def test_the_table_enters_every_branch():
    said = " ".join(c.branch for c in CASES)
    for what in ("matrix-pipe panel + its tail kernel", "matrix-pipe tail kernel alone", "f64 panel NH=2 + 16-byte tile tail", "f64 panel NH=4",
                 "16-byte tile kernel; sweep", "scalar tile kernel", "sweep <1,8>", "sweep <2,8>", "sweep <4,2>", "generic", "widened", "centred; f64 panel"):
        assert what in said, what


def test_decisions_are_still_in_the_source():
    """The expressions the table cites are in bf16.hip (fit.hip where marked) as written."""
    flat = {}
    for name in ("bf16.hip", "fit.hip"):
        with open(os.path.join(os.path.dirname(BF16_HIP), name)) as f:
            flat[name] = re.sub(r"\s+", " ", f.read())
    for c in CASES:
        assert c.decided_by, c.name
        for expr in c.decided_by:
            name = "fit.hip" if expr.endswith("[fit.hip]") else "bf16.hip"
            assert re.sub(r"\s+", " ", expr.replace("[fit.hip]", "")).strip() in flat[name], (c.name, expr)


def _power(c, what, ref, fm, pipe):
    dB = O.rel_fro(coef(ref), coef(fm))
    s = np.sign(np.dot(ref.W[:, 0], fm.W[:, 0])) or 1.0
    dw = O.rel_fro(ref.W[:, 0], fm.W[:, 0] * s)
    print(f"  {c.name}: without {what}: B moves {dB:.3e}, w_1 {dw:.3e}")
    assert dB >= POWER * BUDGET_B, (c.name, what, dB)
    assert dw >= POWER * (W1_PIPE if pipe else TIGHT), (c.name, what, dw)
    return dB, dw


@pytest.mark.parametrize("c", [c for c in CASES if not c.env and c.ld is None and not c.shift], ids=lambda c: c.name)
def test_power(c):
    """Every sentinel carries at least 100 gates of the result (the cases that only change a knob or the storage share the data of `pipe`)."""
    X, Y, w = case_data(c)
    fresh = _data(c.n, c.p, c.q, c.rows, c.cols)[2]
    ref, pipe = oracle(c), route(c)[1]
    for r in c.rows:
        keep = np.arange(c.n) != r
        _power(c, f"row {r}", ref, O.plskern(X[keep], Y[keep], None if w is None else w[keep], nlv=c.nlv, scal=c.scal), pipe)
    for i, j in enumerate(c.cols):
        Xn = np.array(X)
        Xn[:, j] = fresh[:, i]
        _power(c, f"column {j}", ref, O.plskern(Xn, Y, w, nlv=c.nlv, scal=c.scal), pipe)


def test_the_variants_share_their_data():
    for c in CASES:
        if c.env or c.ld is not None or c.shift:
            base = next(b for b in CASES if not b.env and b.ld is None and not b.shift and b.cuts is None and (b.n, b.p, b.q) == (c.n, c.p, c.q))
            assert (base.rows, base.cols, base.nlv, base.weights, base.scal) == (c.rows, c.cols, c.nlv, c.weights, c.scal), c.name
            assert oracle(base) is oracle(c)


@pytest.mark.parametrize("c", [c for c in CASES if not c.env and c.ld is None and not c.shift], ids=lambda c: c.name)
def test_benign(c):
    """The CPU model of the mode stays 30 times under the loosest budget: the data are well conditioned for f32 row arithmetic."""
    X, Y, w = case_data(c)
    e = errors(oracle(c), *model_fit(X, Y, w, c.nlv, c.scal, sweep_rows(c)))
    print(f"  {c.name}: model against the oracle: " + ", ".join(f"{k} {v:.1e}" for k, v in e.items()))
    assert max(e.values()) <= BENIGN, (c.name, e)


def test_the_model_is_not_the_oracle():
    """(the model really rounds: on the first case it differs from the oracle, by more than Float64 noise)"""
    c = CASES[0]
    X, Y, w = case_data(c)
    e = errors(oracle(c), *model_fit(X, Y, w, c.nlv, c.scal, 8))
    assert e["w1"] < 1e-13 and 1e-9 < e["T"] <= BENIGN
