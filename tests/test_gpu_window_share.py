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
import pytest

import window_cases as wc

pytestmark = pytest.mark.gpu

T0 = 10_000_000
STEP = 15000
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 240, 400]
CLASSES = ["bench", "grid", "drop30", "clusters", "dupruns"]
FN_RATE, FN_COUNT, FN_AVG, FN_TIMESTAMP = 0, 4, 5, 14
COUNTS = [1, 64, 65, 256, 257, 600]


def _timestamps(cls, rng, n):
    # the duplicate class sits off every window edge (module docstring)
    return wc.scrape_ts(cls, rng, n, T0, STEP, off_edges=cls == "dupruns")


@pytest.fixture(scope="module")
def engine(fdb):
    return fdb.Engine(0)


@pytest.fixture(scope="module")
def cases(fdb, engine):
    return wc.case_cache(lambda cls: wc.Case(
        fdb, engine, cls, SIZES, 2000 + CLASSES.index(cls), _timestamps))


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


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cls", CLASSES)
def test_shared_bounds_vs_oracle(fdb, oracle, engine, cases, cls, shape):
    case = cases(cls)
    start, step, nw, window = _shape(shape, case)
    end = start + (nw - 1) * step
    for func in (FN_COUNT, FN_TIMESTAMP):       # the bounds themselves: exact
        q = fdb.make_query(start, step, end, window, func)
        assert q.num_windows == nw
        got, want = wc.run_both(oracle, engine, case, q)
        wc.assert_exact(got, want)
    for func in (FN_RATE, FN_AVG):
        q = fdb.make_query(start, step, end, window, func)
        got, want = wc.run_both(oracle, engine, case, q)
        wc.assert_close(got, want)


def test_fused_group_sum_shared(fdb, oracle, engine, cases, monkeypatch):
    """sum by (group) through the fused-group emit (W <= 256) at m = 20."""
    monkeypatch.setenv("FDB_FUSED_GROUP", "1")
    case = cases("bench")
    for func in (FN_RATE, FN_COUNT):
        q = fdb.make_query(T0, STEP, T0 + 240 * STEP, 300_000, func,
                           fdb.AGG_SUM, 3)
        got, want = wc.run_both(oracle, engine, case, q)
        wc.assert_close(got, want)
