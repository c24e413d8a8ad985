"""CPU-only checks of the instant-function model (tests/instant_model.py):
it reproduces the reference's own test literals (tests/golden/
instant_fixtures.json, transcribed from RateFunctionsSpec.scala), it agrees
with the per-window closed forms the kernels implement, and the public ids are
the ones the header defines."""
import json
import math
import os
import re

import numpy as np
import pytest

import instant_model as im

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(HERE, "golden", "instant_fixtures.json")) as f:
        return json.load(f)


def _cols(rows):
    return ([int(t) for t, _ in rows], [float(v) for _, v in rows])


def _one_window(ts, vals, start_ts, end_ts, func):
    return im.sliding(ts, vals, end_ts, 1, end_ts, end_ts - start_ts, func)[0]


def test_irate_golden(fx):
    c = fx["irate"]
    ts, vals = _cols(fx[c["samples"]]["rows"])
    expected = (vals[-1] - vals[-2]) / (ts[-1] - ts[-2]) * 1000
    got = _one_window(ts, vals, c["start_ts"], c["end_ts"], im.IRATE)
    assert got == expected


def test_idelta_golden(fx):
    c = fx["idelta"]
    ts, vals = _cols(fx[c["samples"]]["rows"])
    got = _one_window(ts, vals, c["start_ts"], c["end_ts"], im.IDELTA)
    assert got == vals[-1] - vals[-2] == 3099.0


def test_resets_golden_add_remove(fx):
    """The spec's own sequence: add every row, evict five, evict the rest."""
    c = fx["resets"]
    ts, vals = _cols(fx[c["samples"]]["rows"])
    fn = im.ResetsFunction()
    w = im.Window()
    assert math.isnan(fn.apply(c["start_ts"], c["end_ts"], w))
    for t, v in zip(ts, vals):
        r = im.Row(t, v)
        w.q.append(r)
        fn.added(r, w)
    assert fn.apply(c["start_ts"], c["end_ts"], w) == c["expected_full"] == 4.0
    for _ in range(c["evict_first"]):
        fn.removed(w.q.popleft(), w)
    assert fn.apply(c["start_ts"], c["end_ts"], w) == c["expected_after_evict"] == 1.0
    while w.size:
        fn.removed(w.q.popleft(), w)
    assert c["expected_empty"] is None
    assert math.isnan(fn.apply(c["start_ts"], c["end_ts"], w))


def test_resets_golden_sliding(fx):
    """The same three results through the sliding iterator."""
    c = fx["resets"]
    ts, vals = _cols(fx[c["samples"]]["rows"])
    end = c["end_ts"]
    assert _one_window(ts, vals, c["start_ts"], end, im.RESETS) == 4.0
    assert _one_window(ts, vals, ts[c["evict_first"]], end, im.RESETS) == 1.0
    assert math.isnan(_one_window(ts, vals, ts[0] - 1000, ts[0] - 1, im.RESETS))


def test_deriv_golden_bit_exact(fx):
    c = fx["deriv"]
    ts, vals = _cols(c["rows"])
    k = c["window_rows"]
    assert len(c["expected"]) == len(ts) - k + 1 == 8
    for i, (end_ts, want) in enumerate(c["expected"]):
        assert end_ts == ts[i + k - 1]
        got = _one_window(ts, vals, ts[i], end_ts, im.DERIV)
        assert got == want, (i, got, want)       # bit-for-bit


def _int_counter(rng, n, nan_p):
    ts = 100000 + np.cumsum(rng.integers(1, 30000, n))
    vals = np.cumsum(rng.integers(0, 1 << 20, n)).astype(np.float64)
    for i in np.nonzero(rng.random(n) < 0.08)[0]:
        vals[i:] -= vals[i] - float(rng.integers(0, 50))   # restart near 0
    vals[rng.random(n) < nan_p] = np.nan
    return ts.astype(np.int64), vals


def _gauge(rng, n, nan_p):
    ts = 100000 + np.cumsum(rng.integers(1, 30000, n))
    vals = np.cumsum(rng.normal(0, 1, n)) + rng.random(n)
    vals[rng.random(n) < nan_p] = np.nan
    return ts.astype(np.int64), vals


@pytest.mark.parametrize("nan_p", [0.0, 0.1])
@pytest.mark.parametrize("window,step", [(300000, 75000), (100000, 33000),
                                         (20000, 60000)])
def test_model_equals_closed_forms(nan_p, window, step):
    rng = np.random.default_rng(1234 + int(nan_p * 10) + window)
    for _ in range(6):
        cts, cvals = _int_counter(rng, 300, nan_p)
        assert np.all(np.diff(cts) > 0) and np.nanmax(np.abs(cvals)) < 2 ** 40
        assert np.nanmin(cvals) >= 0
        gts, gvals = _gauge(rng, 300, nan_p)
        start, end = int(cts[0]) - 5000, int(cts[-1]) + 2 * window
        # irate: integral counters with resets and NaNs (corrected sums exact)
        np.testing.assert_array_equal(
            im.sliding(cts, cvals, start, step, end, window, im.IRATE),
            im.closed_form(cts, cvals, start, step, end, window, im.IRATE))
        start, end = int(gts[0]) - 5000, int(gts[-1]) + 2 * window
        for f in (im.IDELTA, im.RESETS, im.DERIV):
            np.testing.assert_array_equal(
                im.sliding(gts, gvals, start, step, end, window, f),
                im.closed_form(gts, gvals, start, step, end, window, f),
                err_msg=f)
        # resets on the counter too (real drops, not just gauge noise)
        np.testing.assert_array_equal(
            im.sliding(cts, cvals, start, step, end, window, im.RESETS),
            im.closed_form(cts, cvals, start, step, end, window, im.RESETS))


def test_window_edges_inclusive():
    ts = [1000, 2000, 3000, 4000]
    vals = [1.0, 5.0, 2.0, 9.0]
    # wStart and wEnd exactly on sample timestamps: both rows belong
    assert im.sliding(ts, vals, 3000, 1, 3000, 1000, im.IDELTA)[0] == -3.0
    assert im.sliding(ts, vals, 3000, 1, 3000, 999, im.RESETS)[0] == 0.0
    assert im.sliding(ts, vals, 3000, 1, 3000, 1000, im.RESETS)[0] == 1.0
    assert math.isnan(im.sliding(ts, vals, 3000, 1, 3000, 999, im.IDELTA)[0])
    assert math.isnan(im.sliding(ts, vals, 2999, 1, 2999, 998, im.RESETS)[0])


def test_python_ids(fdb):
    assert (fdb.FN_IRATE, fdb.FN_IDELTA, fdb.FN_RESETS, fdb.FN_DERIV) == \
        (21, 22, 23, 24)


def test_header_ids():
    with open(os.path.join(REPO, "include", "filodb_amd.h")) as f:
        text = f.read()
    for name, val in (("IRATE", 21), ("IDELTA", 22), ("RESETS", 23),
                      ("DERIV", 24)):
        m = re.search(r"#define\s+FDB_FN_%s\s+(\d+)" % name, text)
        assert m, "FDB_FN_%s missing from include/filodb_amd.h" % name
        assert int(m.group(1)) == val
