"""The fast scan's shared window search as plain host C++:
tools/verify_window_share.cpp checks window_bounds.h's fdb_bound_s_from_e (a
window's start row derived from the end search at the same offset) and a
lane-by-lane model of the kernel's exchange (64 lanes x 4 slots x tiles, the
slot -1 seed, the tile carry) against a brute-force linear scan, for
window/step ratios 1, 2, 20, 40, 63, 64, window counts 1..600 and queries
that start before, inside and after the chunk. Window edges are placed
exactly on rows and on runs of equal timestamps, the case the oracle cannot
judge (tests/test_gpu_window_bounds.py's docstring), so it is checked only
here. No GPU, nothing loaded into Python."""
import pytest

from verifier_run import run_verifier

CLASSES = ["bench", "drop2", "drop10", "drop30", "grid", "geometric",
           "clusters", "allequal", "dupruns", "dupgrid"]
FIELDS = ("offsets", "ties", "dupties", "windows", "wties", "wdupties",
          "mismatches")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    rc, _, rows = run_verifier("verify_window_share", tmp_path_factory.mktemp("ws"))
    return rc, rows


def test_share_matches_linear_scan(report):
    rc, rows = report
    assert sorted(rows) == sorted(CLASSES)
    for cls, row in rows.items():
        assert tuple(row) == FIELDS, cls
        assert row["offsets"] > 20000, cls
        # 11 sizes x 2 steps x 6 ratios x 6 window counts x >= 4 query starts
        assert row["windows"] > 500000, cls
        assert row["mismatches"] == 0, cls
    assert rc == 0


def test_edges_on_rows_and_duplicate_runs_are_exercised(report):
    """The tie branch (an edge exactly on a row) and its fallback (the row is
    inside a run of equal timestamps) both ran, in the derivation check and
    in the exchange model."""
    _, rows = report
    for cls in CLASSES:
        assert rows[cls]["ties"] > 500 and rows[cls]["wties"] > 1000, cls
    for cls in ("allequal", "dupruns", "dupgrid"):
        assert rows[cls]["dupties"] > 500 and rows[cls]["wdupties"] > 1000, cls
    assert rows["grid"]["wties"] > 30000
    assert rows["dupgrid"]["wdupties"] > 10000
