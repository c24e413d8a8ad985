"""The engine stays usable after a query fails.

Each case makes one call fail with an ordinary argument or capacity error the
engine already reports, then runs a plain query on the SAME engine and dataset
and compares it with the oracle: the overflow flag the failing call raised must
have been cleared, and what the failing call allocated must not be in the way.
"""
import numpy as np
import pytest

from conftest import build_store, synth_gauge_series
from test_hist import make_hist_store, synth_hist

pytestmark = pytest.mark.gpu

T0, STEP = 100000, 15000


@pytest.fixture(scope="module")
def engine(fdb):
    return fdb.Engine(0)


def check(got, want):
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12, equal_nan=True)


def sample_overflow_case(fdb):
    """One gauge series of 3 chunks x 400 rows without NaN; a window over all
    1200 rows (more than the sample kernel's 1024-sample buffer) and a 5-minute
    query over the same rows."""
    rng = np.random.default_rng(11)
    ts, vs = synth_gauge_series(rng, 1200, start_ts=T0, step=STEP)
    rows = [(int(t), float(v)) for t, v in zip(ts, vs)]
    st = build_store(fdb, [[rows[0:400], rows[400:800], rows[800:1200]]],
                     kind=fdb.COL_GAUGE)
    end = int(ts[-1]) + STEP
    q_over = fdb.make_query(end, STEP, end, end - T0 + STEP,
                            fdb.FN_QUANTILE_OVER_TIME, param=0.5)
    q_ok = fdb.make_query(T0 + 380 * STEP, STEP, T0 + 440 * STEP, 300000,
                          fdb.FN_QUANTILE_OVER_TIME, param=0.5)
    return st, q_over, q_ok


def count_values_case(fdb):
    """10 series with distinct constant values in one group."""
    series = [[[(T0 + i * STEP, float(s + 1)) for i in range(8)]]
              for s in range(10)]
    st = build_store(fdb, series, kind=fdb.COL_GAUGE)
    q = fdb.make_query(T0 + 2 * STEP, STEP, T0 + 6 * STEP, 2 * STEP,
                       fdb.FN_LAST, fdb.AGG_COUNT_VALUES, 1)
    return st, q


def hist_case(fdb):
    """8 series x 40 rows, nb=8, no max/min companion columns; windows
    straddling before/inside/after the data."""
    rng = np.random.default_rng(4)
    series = [synth_hist(rng, 40, nb=8) for _ in range(8)]
    st = make_hist_store(fdb, series, nb=8, groups=[i % 2 for i in range(8)])
    start = int(series[0][0][0]) - 100000
    q = fdb.make_query(start, 60000, start + 30 * 60000, 300000,
                       fdb.FN_HIST_RATE, fdb.AGG_SUM, 2, param=0.5)
    return st, q


def test_query_after_window_sample_overflow(fdb, oracle, engine):
    st, q_over, q_ok = sample_overflow_case(fdb)
    ds = engine.upload(st)
    with pytest.raises(RuntimeError):
        engine.query(ds, q_over, out=np.empty(q_over.num_windows))
    got = np.empty(q_ok.num_windows)
    engine.query(ds, q_ok, out=got)
    want = oracle.query_exec(st.view(), q_ok, 1, q_ok.num_windows)
    assert np.isfinite(want).all()
    check(got, want)


def check_count_values(oracle, engine, st, ds, q):
    gv, gc, gn = engine.count_values(ds, q, k_cap=16)
    wv, wc, wn = oracle.count_values(st.view(), q, k_cap=16)
    assert wn.tolist() == [10] * q.num_windows
    np.testing.assert_array_equal(gn, wn)
    for i in range(len(wn)):
        check(gv[i][:wn[i]], wv[i][:wn[i]])
        np.testing.assert_array_equal(gc[i][:wn[i]], wc[i][:wn[i]])


def test_count_values_after_overflow(fdb, oracle, engine):
    st, q = count_values_case(fdb)
    ds = engine.upload(st)
    with pytest.raises(RuntimeError):
        engine.count_values(ds, q, k_cap=4)
    check_count_values(oracle, engine, st, ds, q)


def test_count_values_over_sample_overflow(fdb, oracle, engine):
    """count_values over quantile_over_time whose window overflows the sample
    buffer: the error is the scan's, not the presenter's distinct-value limit,
    and the flag the two kernels share is clear afterwards"""
    st, q_over, _ = sample_overflow_case(fdb)
    q_over.agg_id, q_over.num_groups = fdb.AGG_COUNT_VALUES, 1
    ds = engine.upload(st)
    with pytest.raises(RuntimeError) as ei:
        engine.count_values(ds, q_over, k_cap=16)
    assert "sample buffer" in str(ei.value)
    assert "distinct values" not in str(ei.value)
    st2, q = count_values_case(fdb)
    check_count_values(oracle, engine, st2, engine.upload(st2), q)


def test_hist_query_after_argument_error(fdb, oracle, engine):
    st, q = hist_case(fdb)
    nb, cells = 8, q.num_groups * q.num_windows
    ds = engine.upload(st)
    with pytest.raises(RuntimeError):
        engine.query_hist_mm(ds, q, nb, out_bucket_sums=np.zeros(cells * nb),
                             out_counts=np.zeros(cells),
                             out_max=np.zeros(cells), out_min=np.zeros(cells))
    got_s, got_c, got_q = np.zeros(cells * nb), np.zeros(cells), np.zeros(cells)
    engine.query_hist(ds, q, nb, out_bucket_sums=got_s, out_counts=got_c,
                      out_quantile=got_q)
    want_s, want_c, want_q = oracle.query_exec_hist(st.view(), q, nb)
    assert want_c.max() > 0
    np.testing.assert_array_equal(got_c, want_c)
    check(got_s, want_s)
    check(got_q, want_q)
