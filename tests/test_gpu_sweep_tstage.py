"""JCH_SWEEP_TSTAGE (-m gpu): the plskern sweeps keep the score column of a launch in per-wave LDS rings and write a ring out with
all 64 lanes when it is full and once behind the wave's last row group, instead of one 64-byte store per row group between the
loads.  The staged values are the registers the direct store writes and go to the same addresses — nothing else
changes, not the wave that computes a row nor any order of summation — so every output must be the very bits of the direct-store
kernel (`=0`) for every ring length, and nothing may be written beyond row n or into another column.  The ring length is a runtime
argument: rings of 1-3 row groups run the code of the long default ring (fill, wrap, flush when full, flush of a partly filled
ring) at small n; `4096` is more than any wave holds and more than the 64 KB of LDS allow: the launcher's cap."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_gpu_sweep_resident import FIELDS, _data, _run_sharded  # noqa: E402

# 0: direct stores (the reference of every comparison); None: the library's default for the shape
SETTINGS = ("0", None, "1", "2", "3", "4096")


@pytest.fixture(scope="module")
def J():
    import jchemo_hip
    return jchemo_hip


@pytest.fixture(scope="module")
def ctx(J):
    c = J.Context(0)
    yield c
    c.close()


def _env(monkeypatch, name, v):
    if v is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, v)


def _set(monkeypatch, ring, resident=None):
    _env(monkeypatch, "JCH_SWEEP_TSTAGE", ring)
    _env(monkeypatch, "JCH_SWEEP_RESIDENT_MB", resident)


def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else a


def _same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(_host(getattr(a, f)), _host(getattr(b, f))), (what, f)


# p = 500: k_sweep_v2<4, 4, 3> (all these n are short shards: 4 rows per group, 224 blocks = 896 waves);
# p = 1000: k_sweep_v2<8, 4, 2> (4 rows per group, 208 blocks = 832 waves).
#   n = 37: fewer groups than waves — most waves flush an empty ring;  n = 9001: n not a multiple of the group, waves hold 2 or 3
#   groups;  n = 33283 = 8 * 832 * 5 + 3: 9 or 10 groups per wave, so rings 1, 2 and 3 wrap a different number of times and end
#   partly filled, and the last group is partial;  zero weights;  scal;  nlv >= 3: the first sweep of a fit walks backwards (the
#   flush addresses of the `rev` walk), the later ones forwards
SHAPES = [
    dict(n=37, p=500, q=10, nlv=4),
    dict(n=300, p=500, q=1, nlv=5),
    dict(n=9001, p=500, q=10, nlv=5),
    dict(n=33283, p=500, q=10, nlv=4),
    dict(n=4101, p=1000, q=1, nlv=4),
    dict(n=16645, p=1000, q=10, nlv=3),
    dict(n=9001, p=500, q=10, nlv=4, zeros=True),
    dict(n=9001, p=500, q=3, nlv=4, scal=True),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(f"{k}{v}" for k, v in s.items()))
def test_score_ring_leaves_every_bit_alone(shape, J, ctx, monkeypatch):
    n, p, q, nlv = (shape[k] for k in ("n", "p", "q", "nlv"))
    X, Y, w = _data(n, p, q, seed=n + p, zeros=shape.get("zeros", False))
    scal = shape.get("scal", False)
    _set(monkeypatch, "0")
    ref = J.plskern(X, Y, w, nlv=nlv, scal=scal, ctx=ctx)
    _same(ref, J.plskern(X, Y, w, nlv=nlv, scal=scal, ctx=ctx), ("0", "repeated fit"))
    for ring in SETTINGS[1:]:
        _set(monkeypatch, ring)
        a = J.plskern(X, Y, w, nlv=nlv, scal=scal, ctx=ctx)
        b = J.plskern(X, Y, w, nlv=nlv, scal=scal, ctx=ctx)
        _same(ref, a, ring)
        _same(a, b, (ring, "repeated fit"))


@pytest.mark.parametrize("p", [500, 1000])
def test_score_ring_beside_a_resident_slice(p, J, ctx, monkeypatch):
    """Both copies of the row loop (streaming and default-policy loads, JCH_SWEEP_RESIDENT_MB) stage and flush."""
    n, q, nlv = 33283, 4, 3
    X, Y, w = _data(n, p, q, seed=11 + p)
    _set(monkeypatch, "0", "0")
    ref = J.plskern(X, Y, w, nlv=nlv, ctx=ctx)
    for resident in ("0", "64"):
        for ring in ("0", "2"):
            _set(monkeypatch, ring, resident)
            a = J.plskern(X, Y, w, nlv=nlv, ctx=ctx)
            _same(ref, a, (resident, ring))
            _same(a, J.plskern(X, Y, w, nlv=nlv, ctx=ctx), (resident, ring, "repeated fit"))


def test_score_ring_long_shard_kernel(J, ctx, monkeypatch):
    """k_sweep_v2<4, 8, 2> (8 rows per group, 208 blocks) runs from 1280 rows per CU on: one shard just above that, narrow rows
    (258 columns are still the four-chunk instantiation), 49 or 50 groups per wave: ring 3 wraps 16 times, `4096` never (the ring
    then holds every group of a wave and is written out once: what the library does by default at the headline size)."""
    n, p, q, nlv = 331779, 258, 3, 3
    X, Y, w = _data(n, p, q, seed=n)
    _set(monkeypatch, "0")
    ref = J.plskern(X, Y, w, nlv=nlv, ctx=ctx)
    for ring in (None, "3", "4096"):
        _set(monkeypatch, ring)
        a = J.plskern(X, Y, w, nlv=nlv, ctx=ctx)
        _same(ref, a, ring)
    _same(a, J.plskern(X, Y, w, nlv=nlv, ctx=ctx), "repeated fit")


def test_score_ring_row_sharded(J, monkeypatch):
    """Three uneven shards on loopback ranks (40 / 4960 / 7000 rows): every rank sizes its ring from its own shard."""
    n, p, q, nlv = 12000, 500, 4, 6
    X, Y, w = _data(n, p, q, seed=5)
    edges = [0, 40, 5000, n]
    shards = [(np.asfortranarray(X[a:b]), np.asfortranarray(Y[a:b]), w[a:b].copy()) for a, b in zip(edges[:-1], edges[1:])]
    _set(monkeypatch, "0")
    ref = _run_sharded(J, shards, nlv)
    _set(monkeypatch, "2")
    fms = _run_sharded(J, shards, nlv)
    for f in FIELDS[1:]:
        for fm in fms[1:]:
            assert np.array_equal(getattr(fms[0], f), getattr(fm, f)), f
    for r0, r1 in zip(ref, fms):
        _same(r0, r1, "2")


@pytest.mark.parametrize("n", [37, 9001, 33283])
def test_score_ring_bf16_storage(n, J, monkeypatch):
    """k_sweep_bf16_v2: the fit on bf16-stored device tensors (as tests/test_gpu_parity.py::test_bf16_storage_mode calls it)."""
    p, q, nlv = 500, 3, 4
    X, Y, w = _data(n, p, q, seed=n + 1)
    Xb = J.colmajor_empty(n, p, dtype=torch.bfloat16); Xb.copy_(torch.from_numpy(X))
    Yb = J.colmajor_empty(n, q, dtype=torch.bfloat16); Yb.copy_(torch.from_numpy(Y))
    tctx = J.Context(0, stream="torch")
    _set(monkeypatch, "0")
    ref = J.plskern(Xb, Yb, w, nlv=nlv, ctx=tctx)
    for ring in (None, "1", "3"):
        _set(monkeypatch, ring)
        a = J.plskern(Xb, Yb, w, nlv=nlv, ctx=tctx)
        _same(ref, a, ring)
        _same(a, J.plskern(Xb, Yb, w, nlv=nlv, ctx=tctx), (ring, "repeated fit"))
    tctx.close()


@pytest.mark.parametrize("case", [dict(n=9001, p=500), dict(n=33283, p=500), dict(n=4101, p=1000)], ids=lambda c: f"n{c['n']}-p{c['p']}")
def test_score_ring_writes_nothing_beyond_its_column(case, J, ctx, monkeypatch):
    """T in a NaN-filled allocation as tests/test_gpu_inplace.py pads its buffers: guards in front and behind, two columns more
    than the fit computes.  A flush that wrote past row n would land in the next column (overwritten later, except behind the last
    one: the spare columns and the rear guard catch it); the columns themselves must equal the direct store's."""
    import test_gpu_inplace as IP
    n, p, q, nlv = case["n"], case["p"], 2, 3
    X, Y, w = _data(n, p, q, seed=3 * n)
    got = {}
    for ring in ("0", "1", "2", "3", "4096"):
        _set(monkeypatch, ring)
        dc = IP.DeviceCall(X, Y, w, nlv + 2, pad=0, mis=False)
        st, k, o = dc.run(J, ctx, "plskern", nlv, False, False)
        assert st == 0 and k == nlv, (ring, J.load().jch_last_error(ctx._h))
        got[ring] = dc.td.get(k)          # (checks the guards, the spare columns)
        assert np.isfinite(got[ring]).all(), ring
        assert np.array_equal(got[ring], got["0"]), ring
