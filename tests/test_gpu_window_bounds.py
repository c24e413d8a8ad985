"""Window row bounds of the fast scan kernel against the oracle (real MI355X).

The fast kernel finds each window's [startRow, endRow] with a linear guess, a
four-row probe and a binary-search fallback (filodb_amd/csrc/window_bounds.h).
count_over_time (= e-s+1) and timestamp (= ts[e]) expose the two bounds
directly and are compared exactly, NaN positions included; rate and
avg_over_time ride on the same bounds and keep test_gpu_parity's tolerance.
Stores are single-chunk (the fast path), at most 64 series each, one per
timestamp law; every query shape runs against every store.

Duplicate timestamps: the engine resolves a window edge that falls exactly on
a run of equal timestamps to the run's last row (end) or first row (start);
tools/verify_window_bounds.cpp checks that convention against a linear scan.
The oracle restates the reference's delta-delta search, which returns
whichever row of the run its slope guess walks to, so on such an edge the two
legitimately differ (a series never holds two samples of one timestamp in
practice). Every window edge here is = 0 or 2 (mod 10) relative to T0, and
the two duplicate classes place their rows at 5 (mod 10), so no edge lands on
a run and the comparison stays exact; edges that hit a row exactly are
covered by the duplicate-free "grid" and "bench" (row 0) stores."""
import pytest

import window_cases as wc

pytestmark = pytest.mark.gpu

T0 = 10_000_000
STEP = 15000
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 240, 400]
CLASSES = ["bench", "grid", "drop2", "drop10", "drop30", "geometric",
           "clusters", "allequal", "dupruns"]
DUP_CLASSES = ("allequal", "dupruns")
FN_RATE, FN_COUNT, FN_AVG, FN_TIMESTAMP = 0, 4, 5, 14


def _timestamps(cls, rng, n):
    # the duplicate classes sit off every window edge (module docstring)
    return wc.scrape_ts(cls, rng, n, T0, STEP, off_edges=cls in DUP_CLASSES)


@pytest.fixture(scope="module")
def engine(fdb):
    return fdb.Engine(0)


@pytest.fixture(scope="module")
def cases(fdb, engine):
    return wc.case_cache(lambda cls: wc.Case(
        fdb, engine, cls, SIZES, 1000 + CLASSES.index(cls), _timestamps))


def _shape(name, case):
    """(start, step, num_windows, window) of a named query shape."""
    span = case.max_ts - T0
    if name == "div":            # step divides the window
        return T0, STEP, 241, 300_000
    if name == "nodiv":          # step does not divide the window
        return T0, STEP, 241, 70_000
    if name == "sparse":         # step larger than the window
        return T0, 60_000, 100, 20_000
    if name == "longwin":        # window longer than a 400-row scrape chunk
        return T0, STEP, 241, 10_000_000
    if name == "win2p31":        # i64 epilogue path (window >= 2^31 ms)
        return T0 + 200_000, STEP, 64, 1 << 31
    if name == "wide":           # windows swept across the store's whole span
        st = max(span // 400 * 10, 10)
        return T0 - 5 * st, st, 50, max(span // 30 * 10, 10)
    if name == "before":         # every window ends before the first row
        return T0 - 3_000_000, STEP, 161, 300_000
    if name == "after":          # every window starts after the last row
        return (case.max_ts + 400_000) // 10 * 10, STEP, 100, 300_000
    if name.startswith("nw"):    # window-count edges of the 4x64 lane layout
        nw = int(name[2:])
        return T0, (10_000 if nw == 600 else STEP), nw, 300_000
    raise KeyError(name)


SHAPES = ["div", "nodiv", "sparse", "longwin", "win2p31", "wide", "before",
          "after", "nw1", "nw64", "nw65", "nw256", "nw257", "nw600"]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("cls", CLASSES)
def test_bounds_vs_oracle(fdb, oracle, engine, cases, cls, shape):
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


@pytest.mark.parametrize("cls", ["bench", "drop30", "clusters"])
def test_fused_group_sum(fdb, oracle, engine, cases, cls, monkeypatch):
    """sum by (group) through the fused-group emit (W <= 256)."""
    monkeypatch.setenv("FDB_FUSED_GROUP", "1")
    case = cases(cls)
    for func in (FN_RATE, FN_COUNT):
        q = fdb.make_query(T0, STEP, T0 + 240 * STEP, 300_000, func,
                           fdb.AGG_SUM, 3)
        got, want = wc.run_both(oracle, engine, case, q)
        wc.assert_close(got, want)
