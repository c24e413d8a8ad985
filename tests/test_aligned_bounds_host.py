"""The fast scan's direct window rows as plain host C++:
tools/verify_aligned_bounds.cpp runs window_bounds.h's eligibility test
(fdb_aligned_guess / fdb_aligned_test) and the two direct bounds
(fdb_aligned_bounds) on descriptors built by fast_desc.h from real
stores, and compares every window in [-64, nw+64) with a linear scan: the
bench law, an exact grid (every row a tie), query phases 0, 1, q/2, q-1, -1,
slow drift, duplicate timestamps inside the condition, row counts 1..8,
63..65, 240, 400 and windows of 1, 20, 40, 64 steps; dropped rows, irregular
series and a scrape interval that is not the step check that the test never
accepts a series the condition does not hold for. No GPU, nothing loaded into
Python (hipcc only supplies the include path of the store's source file)."""
import re

import pytest

from verifier_run import STORE_SRC, run_verifier

CLASSES = ["bench", "zerojitter", "driftm1", "driftp1", "driftm5", "driftp5",
           "dups", "widejitter", "drop", "irregular", "interval10s", "benchlaw"]
FIELDS = ("cases", "eligible", "c_holds", "rejected_c", "windows", "mismatches")
# classes whose every series of three rows or more must take the direct path
# (one- and two-row vectors are stored raw and never qualify)
ALIGNED = ["bench", "zerojitter", "driftm1", "driftp1", "driftm5", "driftp5"]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    rc, out, rows = run_verifier("verify_aligned_bounds", tmp_path_factory.mktemp("ab"),
                                 flags=["-fopenmp"], sources=[STORE_SRC])
    bench = re.search(r"bench-law series eligible: (\d+) of (\d+)", out)
    return rc, rows, bench


def test_direct_bounds_match_linear_scan(report):
    rc, rows, _ = report
    assert sorted(rows) == sorted(CLASSES)
    for cls, r in rows.items():
        assert tuple(r) == FIELDS, cls
        assert r["mismatches"] == 0, cls
        assert r["eligible"] <= r["c_holds"], cls     # never accepted without C
    for cls in ALIGNED:
        r = rows[cls]
        assert r["eligible"] == r["cases"] * 11 // 13, cls
        assert r["windows"] > 100000, cls
    for cls in ("dups", "widejitter", "drop", "irregular", "interval10s"):
        assert 0 < rows[cls]["eligible"] < rows[cls]["cases"], cls
    assert rc == 0


def test_bench_law_is_fully_eligible(report):
    """Every one of 20,000 series built with bench.py's generator parameters
    takes the direct path under bench.py's query, and the eligibility test
    rejects none of them although the condition holds."""
    _, rows, bench = report
    assert bench and bench.group(1) == bench.group(2) == "20000"
    assert rows["benchlaw"]["rejected_c"] == 0
    assert rows["benchlaw"]["windows"] == 2000 * (241 + 128)
