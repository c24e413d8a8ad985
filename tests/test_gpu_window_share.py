"""The fast scan's shared window search against the oracle (real MI355X).

When the query window is m = 1..64 whole steps, the fast kernel searches only
each window's END row and hands the start row over from the lane that
searched the same offset as window w-m's end (scan_fast.hip's window phase,
window_bounds.h's fdb_bound_s_from_e); any other window/step pair keeps the
two-searches-per-window path. The shapes below take both: ratios 1, 2, 20,
63, 64 share; 65 and 300 fall back on the ratio, window 70 000 / step 15 000
because the step does not divide the window. Window counts 1, 64, 65, 256,
257 and 600 at m = 20 and m = 63 run the slot -1 seed (lanes below m take
their start row from the windows before the tile) and the carry from one
256-window tile to the next.

Stores, sizes and tolerances are those of tests/test_gpu_window_bounds.py:
single-chunk series of 1..400 rows, at most 64 per store, one store per
timestamp law; count_over_time (= e-s+1) and timestamp (= ts[e]) are compared
exactly, rate and avg_over_time at rtol 1e-9 / atol 1e-12. As there, every
window edge is = 0 (mod 10) relative to T0 and the duplicate class keeps its
rows at 5 (mod 10): on an edge that falls on a run of equal timestamps the
oracle and the engine legitimately differ (that file's docstring), so that
case is checked on the host only (tests/test_window_share_host.py). Edges
that hit a single row exactly are covered by the "grid" store."""
import numpy as np
import pytest

from conftest import build_store

pytestmark = pytest.mark.gpu

T0 = 10_000_000
STEP = 15000
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 240, 400]
CLASSES = ["bench", "grid", "drop30", "clusters", "dupruns"]
FN_RATE, FN_COUNT, FN_AVG, FN_TIMESTAMP = 0, 4, 5, 14
COUNTS = [1, 64, 65, 256, 257, 600]


def _scrape(rng, n, drop, jitter=300):
    grid = np.arange(int(n / (1 - drop)) + 64)
    if drop > 0:
        grid = grid[rng.random(grid.size) >= drop]
    grid = grid[:n]
    assert grid.size == n
    return grid * STEP + rng.integers(-jitter, jitter + 1, n)


def _timestamps(cls, rng, n):
    if cls == "bench":
        t = _scrape(rng, n, 0.0)
    elif cls == "grid":                     # rows exactly on wEnd and wStart
        t = np.arange(n) * STEP
    elif cls == "drop30":
        t = _scrape(rng, n, 0.30)
    elif cls == "clusters":                 # two dense clusters, one 2^30 gap
        gaps = rng.integers(900, 1101, n)
        if n >= 2:
            gaps[n // 2 - 1] = 1 << 30
        t = np.concatenate([[0], np.cumsum(gaps)[:-1]])
    else:                                   # dupruns: runs of 1..5 equal rows
        runs = rng.integers(1, 6, n)
        base = np.cumsum(STEP + rng.integers(-300, 301, n))
        t = np.repeat(base, runs)[:n]
    t = np.maximum.accumulate(np.asarray(t, dtype=np.int64))
    t = T0 + t - t[0]
    if cls == "dupruns":
        t = t // 10 * 10 + 5      # off every window edge (module docstring)
    return t


class Case:
    def __init__(self, fdb, engine, cls):
        rng = np.random.default_rng(2000 + CLASSES.index(cls))
        series, groups = [], []
        for n in SIZES:
            for resets in (False, True):    # rate path with and without drops
                ts = _timestamps(cls, rng, n)
                vals = np.cumsum(rng.poisson(10.0, n).astype(np.float64))
                if resets:
                    for i in np.nonzero(rng.random(n) < 0.05)[0]:
                        vals[i:] -= vals[i]
                series.append([[(int(t), float(v)) for t, v in zip(ts, vals)]])
                groups.append(len(series) % 3)
        self.max_ts = max(ch[0][-1][0] for ch in series)
        self.store = build_store(fdb, series, kind=fdb.COL_COUNTER, groups=groups)
        self.ds = engine.upload(self.store)


@pytest.fixture(scope="module")
def engine(fdb):
    return fdb.Engine(0)


@pytest.fixture(scope="module")
def cases(fdb, engine):
    cache = {}

    def get(cls):
        if cls not in cache:
            cache[cls] = Case(fdb, engine, cls)
        return cache[cls]
    return get


def _shape(name, case):
    """(start, step, num_windows, window) of a named query shape."""
    span = case.max_ts - T0
    if name == "nodiv":          # step does not divide the window: fallback
        return T0, STEP, 241, 70_000
    if name == "before":         # starts 3 windows before the first row
        return T0 - 900_000, STEP, 241, 300_000
    if name == "after":          # every window starts after the last row
        return (case.max_ts + 400_000) // 10 * 10, STEP, 100, 300_000
    if name == "wide20":         # m = 20 swept across the store's whole span
        st = max(span // 400 * 10, 10)
        return T0 - 5 * st, st, 50, 20 * st
    if name.startswith("m"):     # window = m steps, optionally "_nw<count>"
        m, _, nw = name[1:].partition("_nw")
        nw = int(nw) if nw else 241
        step = 10_000 if nw == 600 else STEP      # 600 windows span the chunk
        return T0, step, nw, int(m) * step
    raise KeyError(name)


SHAPES = (["m1", "m2", "m20", "m63", "m64", "m65", "m300", "nodiv", "before",
           "after", "wide20"] +
          [f"m{m}_nw{nw}" for m in (20, 63) for nw in COUNTS])


def _run(fdb, oracle, engine, case, q):
    ns, nw = case.store.num_series, q.num_windows
    out_len = (q.num_groups if q.agg_id else ns) * nw
    want = oracle.query_exec(case.store.view(), q, ns, nw, nthreads=4)
    got = np.empty(out_len, dtype=np.float64)
    engine.query(case.ds, q, out=got)
    return got, want


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cls", CLASSES)
def test_shared_bounds_vs_oracle(fdb, oracle, engine, cases, cls, shape):
    case = cases(cls)
    start, step, nw, window = _shape(shape, case)
    end = start + (nw - 1) * step
    for func in (FN_COUNT, FN_TIMESTAMP):       # the bounds themselves: exact
        q = fdb.make_query(start, step, end, window, func)
        assert q.num_windows == nw
        got, want = _run(fdb, oracle, engine, case, q)
        np.testing.assert_array_equal(got, want)
    for func in (FN_RATE, FN_AVG):
        q = fdb.make_query(start, step, end, window, func)
        got, want = _run(fdb, oracle, engine, case, q)
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12,
                                   equal_nan=True)


def test_fused_group_sum_shared(fdb, oracle, engine, cases, monkeypatch):
    """sum by (group) through the fused-group emit (W <= 256) at m = 20."""
    monkeypatch.setenv("FDB_FUSED_GROUP", "1")
    case = cases("bench")
    for func in (FN_RATE, FN_COUNT):
        q = fdb.make_query(T0, STEP, T0 + 240 * STEP, 300_000, func,
                           fdb.AGG_SUM, 3)
        got, want = _run(fdb, oracle, engine, case, q)
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12,
                                   equal_nan=True)
