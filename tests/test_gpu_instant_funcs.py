"""irate / idelta / resets / deriv on the GPU against the independent model in
tests/instant_model.py (a literal restatement of the reference's sliding path;
the CPU oracle does not know these functions). The engine is never compared
with itself except where two of its paths must agree bit for bit.

irate, idelta and resets are bit-exact; deriv sums in tree order on the device,
so it gets the project's existing tolerance (test_gpu_parity.check).
"""
import contextlib
import json
import os

import numpy as np
import pytest

import instant_model as im
from conftest import build_store, synth_gauge_series
from test_gpu_parity import check

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
T0, STEP = 100000, 15000
MODEL = {21: im.IRATE, 22: im.IDELTA, 23: im.RESETS, 24: im.DERIV}


@pytest.fixture(scope="module")
def engine(fdb):
    return fdb.Engine(0)


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


# ---------------------------------------------------------------------------
# builders (strictly increasing timestamps, asserted)
# ---------------------------------------------------------------------------
def mk_ts(rng, n, jitter=400):
    ts = T0 + np.arange(n, dtype=np.int64) * STEP
    if jitter:
        ts = ts + rng.integers(-jitter, jitter + 1, n)
    assert np.all(np.diff(ts) > 0)
    return ts.astype(np.int64)


def mk_counter(rng, n, nan_p=0.0, resets_at=(), nan_at=(), jitter=400):
    """Integral counter <= 2^40 with random and forced resets."""
    vals = np.cumsum(rng.integers(1, 1 << 20, n)).astype(np.float64)
    forced = [i for i in resets_at if 0 < i < n]
    for i in sorted(set(np.nonzero(rng.random(n) < 0.04)[0].tolist() + forced)):
        if i > 0:
            # restarts at n - i: small, and still a drop right after a drop
            vals[i:] -= vals[i] - float(n - i)
    for i in forced:
        assert vals[i] < vals[i - 1]
    assert vals.max() <= 2.0 ** 40 and vals.min() >= 0
    if nan_p:
        vals[rng.random(n) < nan_p] = np.nan
    for i in nan_at:
        if i < n:
            vals[i] = np.nan
    return mk_ts(rng, n, jitter), vals


def mk_gauge(rng, n, nan_p=0.0, resets_at=(), nan_at=(), jitter=400):
    """Raw (non-integral) random walk with forced drops."""
    vals = np.cumsum(rng.normal(0, 1, n)) + rng.random(n)
    for i in resets_at:
        if 0 < i < n:
            vals[i] = vals[i - 1] - 0.37
    if nan_p:
        vals[rng.random(n) < nan_p] = np.nan
    for i in nan_at:
        if i < n:
            vals[i] = np.nan
    return mk_ts(rng, n, jitter), vals


def chunked(ts, vals, sizes):
    assert sum(sizes) == len(ts)
    out, i = [], 0
    for c in sizes:
        out.append([(int(t), float(v)) for t, v in zip(ts[i:i + c], vals[i:i + c])])
        i += c
    return out


class Case:
    """A sealed store, its series AS THE STORE HOLDS THEM, and datasets
    uploaded for the default dispatch and with the general path forced
    (FDB_FAST=0).

    The model must see the rows the engine sees: like the reference
    (DeltaDeltaVector.scala:46,77, approxConst), the encoder stores a chunk
    whose timestamps all lie within 250 ms of the line through its first and
    last row as that line, so short or low-jitter chunks come back with
    slightly different timestamps than were appended. The series are therefore
    read back from the sealed chunks with the CPU oracle's vector decoders."""

    def __init__(self, fdb, oracle, engine, series, sizes, kind, groups=None):
        self.store = build_store(
            fdb, [chunked(t, v, s) for (t, v), s in zip(series, sizes)],
            kind=kind, groups=groups)
        self.series = []
        for sid, ((ts_in, vals_in), sz) in enumerate(zip(series, sizes)):
            assert self.store.num_chunks(sid) == len(sz)
            ts, vals = [], []
            for c, rows in enumerate(sz):
                tsb, vab, n, _, _ = self.store.chunk(sid, c)
                assert n == rows
                ts.append(oracle.decode_longs(tsb)[:n])
                vals.append(oracle.decode_doubles(vab)[:n])
            ts, vals = np.concatenate(ts), np.concatenate(vals)
            assert np.all(np.diff(ts) > 0)            # strictly increasing
            assert np.max(np.abs(ts - ts_in)) <= 250
            np.testing.assert_array_equal(vals, vals_in)
            self.series.append((ts, vals))
        self.ds = engine.upload(self.store)
        with env("FDB_FAST", "0"):
            self.ds_general = engine.upload(self.store)


def run(fdb, engine, ds, ns, start, step, nw, window, func, agg=0, ng=0):
    q = fdb.make_query(start, step, start + (nw - 1) * step, window, func, agg, ng)
    assert q.num_windows == nw
    out = np.empty((ng if agg else ns) * nw, dtype=np.float64)
    engine.query(ds, q, out=out)
    return out


def run_general(fdb, engine, case, *a, **kw):
    with env("FDB_FAST", "0"):
        return run(fdb, engine, case.ds_general, len(case.series), *a, **kw)


def model(case, start, step, nw, window, func):
    return im.grid(case.series, start, step, start + (nw - 1) * step, window,
                   MODEL[func])


# ---------------------------------------------------------------------------
# fast path: one chunk per series
# ---------------------------------------------------------------------------
FAST_ROWS = (1, 2, 3, 64, 65, 400)


def _fast_series(mk, seed):
    rng = np.random.default_rng(seed)
    series = []
    for nan_p in (0.0, 0.1):
        for n in FAST_ROWS:
            series.append(mk(rng, n, nan_p=nan_p))
    # a drop and a NaN on rows 63/64: the indicator pair straddles the
    # 64-lane scan carry
    series.append(mk(rng, 65, resets_at=(64,)))
    series.append(mk(rng, 130, resets_at=(64,)))
    series.append(mk(rng, 130, resets_at=(63, 65), nan_at=(64,)))
    series.append(mk(rng, 130, resets_at=(64,), nan_at=(63,)))
    # exact 15 s grid: window edges land exactly on sample timestamps
    series.append(mk(rng, 130, resets_at=(64, 100), jitter=0))
    series.append(mk(rng, 130, nan_p=0.1, jitter=0))
    return series


@pytest.fixture(scope="module")
def fast_counter(fdb, oracle, engine):
    s = _fast_series(mk_counter, 11)
    return Case(fdb, oracle, engine, s, [(len(t),) for t, _ in s], fdb.COL_COUNTER)


@pytest.fixture(scope="module")
def fast_gauge(fdb, oracle, engine):
    s = _fast_series(mk_gauge, 12)
    return Case(fdb, oracle, engine, s, [(len(t),) for t, _ in s], fdb.COL_GAUGE)


# (start, step, num_windows, window): windows slide in from before the data,
# so they are empty, then hold 1, 2 and many rows; starts on the 15 s grid hit
# the jitter-free series' timestamps exactly at both edges
FAST_QUERIES = {
    "shared_4x_257w": (T0 - 3 * STEP, STEP, 257, 4 * STEP),
    "shared_20x_257w": (T0 - 3 * STEP, STEP, 257, 20 * STEP),
    "unshared_257w": (T0 - 3 * STEP, STEP, 257, 50000),
    "unshared_fine_step": (T0 - 20000, 7000, 300, 45000),
    "one_window": (T0 + 100 * STEP, STEP, 1, 20 * STEP),
    "one_window_unshared": (T0 + STEP, 7000, 1, STEP),
}


@pytest.mark.parametrize("qname", sorted(FAST_QUERIES))
@pytest.mark.parametrize("func,data", [(21, "counter"), (22, "gauge"),
                                       (23, "gauge"), (23, "counter")])
def test_fast_path(fdb, engine, fast_counter, fast_gauge, func, data, qname):
    case = fast_counter if data == "counter" else fast_gauge
    qargs = FAST_QUERIES[qname]
    want = model(case, *qargs, func)
    got = run(fdb, engine, case.ds, len(case.series), *qargs, func)
    np.testing.assert_array_equal(got, want)
    # path agreement: the general (summary + walk) path on the same store
    general = run_general(fdb, engine, case, *qargs, func)
    np.testing.assert_array_equal(general, want)
    np.testing.assert_array_equal(general, got)
    if qargs[2] > 1:
        assert np.isnan(want).any() and np.isfinite(want).any()


# ---------------------------------------------------------------------------
# stream path: multi-chunk series
# ---------------------------------------------------------------------------
CHUNKINGS = ((400, 400), (399, 1, 400), (1, 1, 398, 400))


def _stream_series(mk, seed):
    rng = np.random.default_rng(seed)
    series, sizes = [], []
    for nan_p, nan_at in ((0.0, ()), (0.1, (400,))):
        for sz in CHUNKINGS:
            # drops exactly on chunk boundaries (rows 1, 2, 399, 400) and inside
            series.append(mk(rng, 800, nan_p=nan_p, nan_at=nan_at,
                             resets_at=(1, 2, 200, 399, 400, 401, 600)))
            sizes.append(sz)
    return series, sizes


@pytest.fixture(scope="module")
def stream_counter(fdb, oracle, engine):
    s, sz = _stream_series(mk_counter, 21)
    return Case(fdb, oracle, engine, s, sz, fdb.COL_COUNTER)


@pytest.fixture(scope="module")
def stream_gauge(fdb, oracle, engine):
    s, sz = _stream_series(mk_gauge, 22)
    return Case(fdb, oracle, engine, s, sz, fdb.COL_GAUGE)


STREAM_QUERIES = {
    # the 1-row chunks at the head of the series
    "head": (T0 - 2 * STEP, STEP, 30, 3 * STEP),
    # window ends sweep rows 385..425: the last two rows straddle a boundary
    "boundary_short": (T0 + 385 * STEP, STEP, 40, 3 * STEP),
    # 105 min lookback: the 398-row and 1-row middle chunks come whole from
    # their summaries (resets_in)
    "boundary_long": (T0 + 385 * STEP + 5000, STEP, 40, 420 * STEP),
    # every chunk whole, then windows running off the end of the data
    "all_rows": (T0 + 700 * STEP, 4 * STEP + 1000, 40, 800 * STEP),
}


@pytest.mark.parametrize("qname", sorted(STREAM_QUERIES))
@pytest.mark.parametrize("func,data", [(21, "counter"), (22, "gauge"),
                                       (23, "gauge"), (23, "counter")])
def test_stream_path(fdb, engine, stream_counter, stream_gauge, func, data, qname):
    case = stream_counter if data == "counter" else stream_gauge
    qargs = STREAM_QUERIES[qname]
    want = model(case, *qargs, func)
    got = run(fdb, engine, case.ds, len(case.series), *qargs, func)
    np.testing.assert_array_equal(got, want)
    assert np.isfinite(want).any()


# ---------------------------------------------------------------------------
# deriv
# ---------------------------------------------------------------------------
def _deriv_series(seed, n, n_series, nan_p=0.0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_series):
        ts, vals = synth_gauge_series(rng, n, start_ts=T0, step=STEP, nan_p=nan_p)
        assert np.all(np.diff(ts) > 0)
        out.append((ts, vals))
    return out


@pytest.fixture(scope="module")
def deriv_single(fdb, oracle, engine):
    s = _deriv_series(31, 240, 3) + _deriv_series(32, 240, 2, nan_p=0.03)
    return Case(fdb, oracle, engine, s, [(240,)] * len(s), fdb.COL_GAUGE)


@pytest.fixture(scope="module")
def deriv_multi(fdb, oracle, engine):
    s = _deriv_series(33, 800, 2) + _deriv_series(34, 800, 1, nan_p=0.01)
    return Case(fdb, oracle, engine, s, [(400, 400)] * len(s), fdb.COL_GAUGE)


def _check_deriv(fdb, engine, case, qargs):
    want = model(case, *qargs, 24)
    # the device sums in tree order: bound what reordering alone may change
    # on this very data before comparing (sequential vs pairwise summation)
    pair = np.concatenate([
        im.closed_form(t, v, qargs[0], qargs[1],
                       qargs[0] + (qargs[2] - 1) * qargs[1], qargs[3],
                       im.DERIV, pairwise=True) for t, v in case.series])
    np.testing.assert_array_equal(np.isnan(pair), np.isnan(want))
    fin = np.isfinite(want)
    if fin.any():
        gap = np.max(np.abs(pair[fin] - want[fin]) / np.abs(want[fin]))
        print("deriv sequential-vs-pairwise gap %.3g" % gap)
        assert gap < 1e-10
    got = run(fdb, engine, case.ds, len(case.series), *qargs, 24)
    check(got, want)
    return want


@pytest.mark.parametrize("k", [0, 1, 2, 3, 64, 65, 130])
def test_deriv_sample_counts(fdb, engine, deriv_single, k):
    """One window holding exactly k samples of series 0 (edges on its
    timestamps; the other series see k or k +- 1)."""
    ts = deriv_single.series[0][0]
    j = 200
    if k == 0:
        end, window = int(ts[0]) - 1000, 500
    elif k == 1:
        end, window = int(ts[j]), 1000
    else:
        end, window = int(ts[j]), int(ts[j] - ts[j - k + 1])
    s = int(np.searchsorted(ts, end - window, side="left"))
    e = int(np.searchsorted(ts, end, side="right")) - 1
    assert e - s + 1 == k
    want = _check_deriv(fdb, engine, deriv_single, (end, STEP, 1, window))
    assert np.isfinite(want[0]) == (k >= 2)


def test_deriv_sweep_and_nan(fdb, engine, deriv_single):
    qargs = (T0 - 2 * STEP, STEP, 257, 20 * STEP)
    want = _check_deriv(fdb, engine, deriv_single, qargs).reshape(5, 257)
    # a NaN sample anywhere in the window gives NaN (not skipped)
    ts, vals = deriv_single.series[3]
    assert np.isnan(vals).any()
    for w in range(30, 220):
        end = qargs[0] + w * STEP
        inside = (ts >= end - qargs[3]) & (ts <= end)
        if np.isnan(vals[inside]).any():
            assert np.isnan(want[3, w])
    assert np.isnan(want[3, 30:220]).any() and np.isfinite(want[3, 30:220]).any()


def test_deriv_multichunk(fdb, engine, deriv_multi):
    # windows crossing the 400/400 boundary, short and spanning both chunks
    _check_deriv(fdb, engine, deriv_multi, (T0 + 385 * STEP, STEP, 40, 20 * STEP))
    _check_deriv(fdb, engine, deriv_multi, (T0 + 500 * STEP, 7 * STEP, 20, 130 * STEP))


# ---------------------------------------------------------------------------
# the reference's own literals, on the device
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    with open(os.path.join(HERE, "golden", "instant_fixtures.json")) as f:
        return json.load(f)


def _golden_case(fdb, oracle, engine, rows, kind):
    """The fixture rows as one chunk, behind one guard row 67 s earlier that
    no tested window reaches. Without it the ten ~10.1 s-spaced timestamps lie
    within 250 ms of a line and the chunk would hold that line instead (see
    Case), and the spec's expressions are over the literal timestamps."""
    ts = np.array([rows[0][0] - 67000] + [t for t, _ in rows], dtype=np.int64)
    vals = np.array([rows[0][1] - 19.0] + [v for _, v in rows], dtype=np.float64)
    assert np.all(np.diff(ts) > 0)
    case = Case(fdb, oracle, engine, [(ts, vals)], [(len(ts),)], kind)
    np.testing.assert_array_equal(case.series[0][0], ts)     # stored exactly
    return case


def _one(fdb, engine, case, start_ts, end_ts, func):
    return run(fdb, engine, case.ds, 1, end_ts, 1, 1, end_ts - start_ts, func)[0]


def test_golden_irate_idelta(fdb, oracle, engine, fx):
    c = fx["irate"]
    rows = fx[c["samples"]]["rows"]
    case = _golden_case(fdb, oracle, engine, rows, fdb.COL_COUNTER)
    (t1, v1), (t2, v2) = rows[-2], rows[-1]
    assert _one(fdb, engine, case, c["start_ts"], c["end_ts"], 21) == \
        (v2 - v1) / (t2 - t1) * 1000
    c = fx["idelta"]
    rows = fx[c["samples"]]["rows"]
    case = _golden_case(fdb, oracle, engine, rows, fdb.COL_GAUGE)
    assert _one(fdb, engine, case, c["start_ts"], c["end_ts"], 22) == \
        rows[-1][1] - rows[-2][1]


def test_golden_resets(fdb, oracle, engine, fx):
    c = fx["resets"]
    rows = fx[c["samples"]]["rows"]
    case = _golden_case(fdb, oracle, engine, rows, fdb.COL_GAUGE)
    end = c["end_ts"]
    assert _one(fdb, engine, case, c["start_ts"], end, 23) == c["expected_full"] == 4.0
    # the first five rows evicted: the window starts on row 5's timestamp
    assert _one(fdb, engine, case, rows[c["evict_first"]][0], end, 23) == \
        c["expected_after_evict"] == 1.0
    assert c["expected_empty"] is None
    assert np.isnan(_one(fdb, engine, case, rows[0][0] - 1000, rows[0][0] - 1, 23))


def test_golden_deriv(fdb, oracle, engine, fx):
    c = fx["deriv"]
    rows = c["rows"]
    case = _golden_case(fdb, oracle, engine, rows, fdb.COL_GAUGE)
    k = c["window_rows"]
    got = [_one(fdb, engine, case, rows[i][0], rows[i + k - 1][0], 24)
           for i in range(len(c["expected"]))]
    check(np.array(got), np.array([v for _, v in c["expected"]]))


# ---------------------------------------------------------------------------
# aggregation
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def agg_case(fdb, oracle, engine):
    rng = np.random.default_rng(41)
    s = [mk_counter(rng, 240, nan_p=0.05 if i % 4 == 0 else 0.0)
         for i in range(30)]
    return Case(fdb, oracle, engine, s, [(240,)] * 30, fdb.COL_COUNTER,
                groups=[i % 3 for i in range(30)])


AGG_Q = (T0 - 2 * STEP, STEP, 200, 20 * STEP)


def _fold(grid, groups, ng, how):
    """NaN-skipping group fold of an [S x W] grid; all-NaN cells stay NaN."""
    out = np.full((ng, grid.shape[1]), np.nan)
    for g in range(ng):
        rows = grid[[i for i, x in enumerate(groups) if x == g]]
        some = ~np.isnan(rows).all(axis=0)
        with np.errstate(all="ignore"):
            if how == "sum":
                v = np.nansum(rows, axis=0)
            elif how == "max":
                v = np.fmax.reduce(rows, axis=0)
            else:
                v = np.nansum(rows, axis=0) / np.sum(~np.isnan(rows), axis=0)
        out[g, some] = v[some]
    return out.ravel()


@pytest.mark.parametrize("agg,how", [(1, "sum"), (4, "max")])
def test_irate_aggregated(fdb, engine, agg_case, agg, how):
    groups = [i % 3 for i in range(30)]
    want = _fold(model(agg_case, *AGG_Q, 21).reshape(30, -1), groups, 3, how)
    assert np.isnan(want).any() and np.isfinite(want).any()
    two_phase = run(fdb, engine, agg_case.ds, 30, *AGG_Q, 21, agg=agg, ng=3)
    if how == "max":
        np.testing.assert_array_equal(two_phase, want)
    else:
        # <= 10 non-negative terms per cell: reordering the sum moves it by at
        # most 9 roundings (1e-15 relative); the project's 1e-9 bar is ample
        check(two_phase, want)
    with env("FDB_FUSED_GROUP", "1"):
        fused = run(fdb, engine, agg_case.ds, 30, *AGG_Q, 21, agg=agg, ng=3)
    check(fused, two_phase)
    check(fused, want)


def test_deriv_avg_two_phase(fdb, engine, deriv_single):
    """avg(deriv): deriv has no fused emit, so FDB_FUSED_GROUP=1 must leave it
    on the two-phase route with the same answer."""
    qargs = (T0 + 10 * STEP, STEP, 100, 20 * STEP)
    want = _fold(model(deriv_single, *qargs, 24).reshape(5, -1), [0] * 5, 1, "avg")
    got = run(fdb, engine, deriv_single.ds, 5, *qargs, 24, agg=5, ng=1)
    check(got, want)
    with env("FDB_FUSED_GROUP", "1"):
        again = run(fdb, engine, deriv_single.ds, 5, *qargs, 24, agg=5, ng=1)
    np.testing.assert_array_equal(again, got)


# ---------------------------------------------------------------------------
# histogram datasets keep rejecting scalar range functions
# ---------------------------------------------------------------------------
def test_histogram_dataset_still_rejected(fdb, engine):
    st = fdb.ChunkStore()
    sid = st.add_series(0, fdb.COL_HIST)
    ts = T0 + np.arange(20, dtype=np.int64) * STEP
    bv = np.cumsum(np.ones((20, 8), dtype=np.uint64), axis=0)
    bv = np.cumsum(bv, axis=1).astype(np.uint64)
    st.append_hist(sid, ts, bv, first=2.0, mult=2.0)
    st.seal()
    ds = engine.upload(st)
    for func in (21, 22, 23, 24):
        with pytest.raises(RuntimeError, match="histogram dataset"):
            run(fdb, engine, ds, 1, T0 + 10 * STEP, STEP, 4, 5 * STEP, func)
