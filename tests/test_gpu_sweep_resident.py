"""JCH_SWEEP_RESIDENT_MB (-m gpu): a fixed set of the plskern sweep's waves reads its row groups with default-policy loads, so that
slice of the working copy stays in the Infinity Cache from sweep to sweep; every other wave streams with non-temporal loads
(DESIGN.md §4).  Only the load instruction of a row changes — not the wave that reads it, nor any order of summation — so every
output must be the very bits of the all-streaming kernel (`=0`), whatever the size of the slice."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FIELDS = ("T", "P", "R", "W", "C", "TT", "xmeans", "xscales", "ymeans", "yscales")
# 0: the all-streaming kernel; None: the library's default for the shape; 1: a single resident wave on the long shapes (a few on
# the short ones); 64: a part of the grid; 256: the cap (the whole cache; every wave where the copy is smaller than that)
SETTINGS = ("0", None, "1", "64", "256")


@pytest.fixture(scope="module")
def J():
    import jchemo_hip
    return jchemo_hip


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    yield c
    c.close()


def _data(n, p, q, seed, zeros=False):
    rng = np.random.default_rng(seed)
    Lt = rng.standard_normal((n, 12))
    X = np.asfortranarray(Lt @ rng.standard_normal((12, p)) + 0.4 * rng.standard_normal((n, p)) + 1.0)
    Y = np.asfortranarray(Lt[:, :q] @ rng.standard_normal((q, q)) + 0.2 * rng.standard_normal((n, q)))
    w = rng.uniform(0.5, 1.5, n)
    if zeros:
        w[rng.random(n) < 0.3] = 0.0
    return X, Y, w


def _set(monkeypatch, mb):
    if mb is None:
        monkeypatch.delenv("JCH_SWEEP_RESIDENT_MB", raising=False)
    else:
        monkeypatch.setenv("JCH_SWEEP_RESIDENT_MB", mb)


def _same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)


# the two sweep instantiations (p = 500: four 128-column chunks, 8 rows per group; p = 1000: eight chunks, 4 rows per group);
# n not a multiple of the group; fewer row groups than waves; q = 1 and q = 10; zero weights; scal
SHAPES = [
    dict(n=9001, p=500, q=10, nlv=7),
    dict(n=9001, p=500, q=10, nlv=6, zeros=True, scal=True),
    dict(n=4101, p=1000, q=1, nlv=5),
    dict(n=4102, p=1000, q=10, nlv=4, zeros=True),
    dict(n=300, p=500, q=1, nlv=5),
    dict(n=37, p=1000, q=10, nlv=4, scal=True),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
def test_resident_slice_leaves_every_bit_alone(shape, J, ctx, monkeypatch):
    n, p, q, nlv = (shape[k] for k in ("n", "p", "q", "nlv"))
    X, Y, w = _data(n, p, q, seed=n + p, zeros=shape.get("zeros", False))
    scal = shape.get("scal", False)
    _set(monkeypatch, "0")
    ref = J.plskern(X, Y, w, nlv=nlv, scal=scal, ctx=ctx)
    for mb in SETTINGS[1:]:
        _set(monkeypatch, mb)
        a = J.plskern(X, Y, w, nlv=nlv, scal=scal, ctx=ctx)
        b = J.plskern(X, Y, w, nlv=nlv, scal=scal, ctx=ctx)
        _same(ref, a, mb)
        _same(a, b, (mb, "repeated fit"))


@pytest.mark.parametrize("n", [300001, 340003])
def test_resident_slice_either_side_of_the_short_shard_grid(n, J, ctx, monkeypatch):
    """The sweep takes a larger grid below 1280 rows per CU (327 680 rows on 256 CUs): one shard on either side of the switch,
    long enough that `=1` is a single resident wave and `=64` / `=256` a part of the grid."""
    p, q, nlv = 258, 3, 3                      # 258 columns: still the four-chunk instantiation, half the bytes
    X, Y, w = _data(n, p, q, seed=n)
    _set(monkeypatch, "0")
    ref = J.plskern(X, Y, w, nlv=nlv, ctx=ctx)
    for mb in SETTINGS[1:]:
        _set(monkeypatch, mb)
        a = J.plskern(X, Y, w, nlv=nlv, ctx=ctx)
        _same(ref, a, mb)
    _same(a, J.plskern(X, Y, w, nlv=nlv, ctx=ctx), "repeated fit")


@pytest.mark.parametrize("alg", ["plssimp", "plsrosa"])
def test_resident_slice_siblings_of_plskern(alg, J, ctx, monkeypatch):
    """plssimp and plsrosa run the same sweep."""
    X, Y, w = _data(9001, 500, 4, seed=77)
    fit = getattr(J, alg)
    _set(monkeypatch, "0")
    ref = fit(X, Y, w, nlv=6, ctx=ctx)
    for mb in ("1", "256"):
        _set(monkeypatch, mb)
        _same(ref, fit(X, Y, w, nlv=6, ctx=ctx), mb)


def _run_sharded(J, shards, nlv):
    """One thread per rank, each with its own ctx joined to a loopback group: the library code of a multi-GPU fit on one GPU."""
    nr = len(shards)
    L = J.load()
    grp = C.c_void_p()
    assert L.jch_loopback_group_create(nr, C.byref(grp)) == 0
    ctxs = [J.Context(0) for _ in range(nr)]
    out, err = [None] * nr, [None] * nr

    def work(r):
        try:
            ctxs[r].comm_init_loopback(grp, r, nr)
            Xs, Ys, ws = shards[r]
            out[r] = J.plskern(Xs, Ys, ws, nlv=nlv, ctx=ctxs[r])
        except Exception as e:  # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(nr)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in th), "a rank thread is stuck in a collective"
    assert err == [None] * nr, err
    for c in ctxs:
        c.close()
    L.jch_loopback_group_destroy(grp)
    return out


def test_resident_slice_row_sharded(J, monkeypatch):
    """Uneven shards on three loopback ranks: every rank derives its resident waves from its own shard, the replicated state stays
    bit-identical across the ranks, and the whole fit equals the all-streaming one bit for bit."""
    n, p, q, nlv = 12000, 500, 4, 6
    X, Y, w = _data(n, p, q, seed=5)
    edges = [0, 40, 5000, n]
    shards = [(np.asfortranarray(X[a:b]), np.asfortranarray(Y[a:b]), w[a:b].copy()) for a, b in zip(edges[:-1], edges[1:])]
    _set(monkeypatch, "0")
    ref = _run_sharded(J, shards, nlv)
    for mb in ("1", "256"):
        _set(monkeypatch, mb)
        fms = _run_sharded(J, shards, nlv)
        for f in FIELDS[1:]:
            for fm in fms[1:]:
                assert np.array_equal(getattr(fms[0], f), getattr(fm, f)), (mb, f)
        for r0, r1 in zip(ref, fms):
            _same(r0, r1, mb)
