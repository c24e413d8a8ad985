"""Direct window rows of the fast scan kernel (real MI355X).

Where the query step matches a series' scrape grid, the kernel takes each
window's [startRow, endRow] from one comparison per bound instead of the
search (filodb_amd/csrc/window_bounds.h, fdb_aligned_*); the series is chosen
per wave from its upload-time descriptor, in a kernel build the launcher picks
when at least a quarter of a host-side descriptor sample qualifies under the
query. FDB_ALIGNED=0, read at launch, keeps the search-only build; the
launcher's test hook (fdb_debug_last_fast_aligned) says which build ran and
how many sampled series qualified, and is asserted on both sides. Both paths feed the same s, e, t1, t2
into the same arithmetic, so for every function the grid with the direct path
on must equal the grid with it off bit for bit, NaN positions included; and
the result must agree with the oracle to tests/test_gpu_window_bounds.py's
tolerances (count and timestamp exact, the others 1e-9 relative).

Stores are single-chunk, 32 series each, one per timestamp law. Every store
mixes series that take the direct path (the law itself, with and without
counter resets) with series that must not: a scrape grid with a row dropped,
a 10 s scrape interval under the 15 s step, and the one- and two-row series,
whose timestamp vectors the builder stores raw.

Duplicate timestamps ("dups": a late row and the next, early one share a
timestamp 0.55 step after a grid point, which still satisfies the condition):
the oracle resolves a window edge that falls on a run of equal timestamps
differently (tests/test_gpu_window_bounds.py's docstring), so those rows sit
8250 ms after the grid, which no query phase used here (0, 1, 7500, 14999,
-1) puts an edge on. tools/verify_aligned_bounds.cpp checks edges on runs
against a linear scan.

"constjit" is a +-100 ms jitter, which the builder stores as a const vector
(every row rounded onto a line): such series take the direct path too, and
direct against searched is checked bit for bit. The oracle comparison is left
out for this one class: the stored last row then precedes the chunk's recorded
end time, and engine and oracle disagree on timestamp() for a window that
starts in between, on the search path as much as on the direct one."""
import pytest

import window_cases as wc

pytestmark = pytest.mark.gpu

STEP = 15000
T0 = 10_005_000                 # a multiple of STEP: the scrape grid's origin
SIZES = [1, 2, 3, 5, 64, 65, 240, 400]
CLASSES = ["bench", "zerojitter", "driftm1", "driftp1", "driftm5", "driftp5",
           "dups", "constjit"]
NO_ORACLE = ("constjit",)
NUM_WINDOWS = [1, 49, 65, 241, 257]
# (window in steps, query phase relative to the scrape grid)
QUERIES = [(1, 0), (1, STEP // 2), (20, 0), (20, 1), (20, STEP // 2),
           (20, STEP - 1), (20, -1), (64, -1), (64, STEP - 1)]
FUNCS = ["FN_RATE", "FN_INCREASE", "FN_DELTA", "FN_AVG_OVER_TIME",
         "FN_COUNT_OVER_TIME", "FN_TIMESTAMP", "FN_LAST", "FN_CHANGES"]
EXACT = ("FN_COUNT_OVER_TIME", "FN_TIMESTAMP")


def _timestamps(law, rng, n):
    return wc.aligned_ts(law, rng, n, T0, STEP)


@pytest.fixture(scope="module")
def engine(fdb):
    return fdb.Engine(0)


@pytest.fixture(scope="module")
def cases(fdb, engine):
    # four series per size: the class with and without counter resets, and
    # two that must not take the direct path
    return wc.case_cache(lambda cls: wc.Case(
        fdb, engine, cls, SIZES, 7000 + CLASSES.index(cls), _timestamps,
        plan=((cls, False), (cls, True), ("drop", True), ("10s", False))))


def _query(fdb, nw, m, phase, func, agg=0, groups=0):
    start = T0 - 10 * STEP + phase          # the first windows precede row 0
    q = fdb.make_query(start, STEP, start + (nw - 1) * STEP, m * STEP, func,
                       agg, groups)
    assert q.num_windows == nw
    return q


def _engine(engine, case, q, monkeypatch, aligned):
    if aligned:
        monkeypatch.delenv("FDB_ALIGNED", raising=False)
    else:
        monkeypatch.setenv("FDB_ALIGNED", "0")
    return wc.run_engine(engine, case, q)


@pytest.mark.parametrize("nw", NUM_WINDOWS)
@pytest.mark.parametrize("cls", CLASSES)
def test_direct_rows_equal_search_and_oracle(fdb, oracle, engine, cases, cls, nw,
                                             monkeypatch):
    case = cases(cls)
    for m, phase in QUERIES:
        for name in FUNCS:
            q = _query(fdb, nw, m, phase, getattr(fdb, name))
            what = f"{name} m={m} phase={phase}"
            on = _engine(engine, case, q, monkeypatch, True)
            # the build with the direct rows ran: at least a quarter of the
            # store's 32 series passed the launcher's test
            assert fdb.lib().fdb_debug_last_fast_aligned() >= 8, what
            off = _engine(engine, case, q, monkeypatch, False)
            assert fdb.lib().fdb_debug_last_fast_aligned() == 0, what
            assert on.tobytes() == off.tobytes(), what
            if cls in NO_ORACLE:
                continue
            want = wc.run_oracle(oracle, case, q)
            if name in EXACT:
                wc.assert_exact(on, want, what)
            else:
                wc.assert_close(on, want, what)


@pytest.mark.parametrize("fused", ["0", "1"])
def test_sum_by_group(fdb, oracle, engine, cases, fused, monkeypatch):
    """sum by (group)(rate[5m]) through the two-phase reduce and the
    fused-group emit, direct path on and off."""
    monkeypatch.setenv("FDB_FUSED_GROUP", fused)
    case = cases("bench")
    for m, phase in ((20, 0), (20, STEP - 1), (64, -1)):
        q = _query(fdb, 241, m, phase, fdb.FN_RATE, fdb.AGG_SUM, 3)
        want = wc.run_oracle(oracle, case, q)
        for aligned in (True, False):
            got = _engine(engine, case, q, monkeypatch, aligned)
            wc.assert_close(got, want)
