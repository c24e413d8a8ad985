"""The fast rate kernel's lean epilogue and seed early-out as plain host C++:
tools/verify_rate_epilogue.cpp compiles rate_core.h and window_bounds.h (the
text the kernels include) and checks the reciprocal-table quotient against
`/`, d_extrapolate_core<true> against d_extrapolate_core<false> bit for bit,
and fdb_windows_before_chunk against the seed search it replaces. This runs
its reduced domain ("quick": ms <= 2^16, 2e6 core inputs, under a second);
the full domain (1.7e10 table cases, 1.2e9 core inputs) is the tool's own
documented run. No GPU, nothing loaded into Python."""
import re

import pytest

from verifier_run import run_verifier



@pytest.fixture(scope="module")
def report(tmp_path_factory):
    rc, out, _ = run_verifier("verify_rate_epilogue", tmp_path_factory.mktemp("re"),
                              flags=["-ffp-contract=off"], args=["quick"])
    return rc, out


def test_lean_epilogue_matches_plain(report):
    rc, out = report
    m = re.search(r"table bad=(\d+) of (\d+)", out)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) == 65536 * 255
    m = re.search(r"core bad=(\d+) of (\d+) \(skip taken on (\d+), table on (\d+)\)", out)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) >= 2_000_000
    # both shortcuts ran, and so did the paths they replace
    n, skip, table = int(m.group(2)), int(m.group(3)), int(m.group(4))
    assert n // 10 < skip < n - n // 10 and n // 10 < table < n - n // 10
    assert rc == 0


def test_seed_early_out_matches_search(report):
    rc, out = report
    m = re.search(r"seed bad=(\d+) of (\d+) early lanes \((\d+) searched, (\d+) of them "
                  r"nonzero\)", out)
    assert m and int(m.group(1)) == 0
    assert int(m.group(2)) > 100_000 and int(m.group(4)) > 100_000
    assert rc == 0
