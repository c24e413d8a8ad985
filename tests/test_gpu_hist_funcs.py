"""increase() and the last sample on histogram datasets (hist2 kernel) against
the numpy model of tests/hist_funcs_model.py — the CPU oracle knows neither.

Every case is at most 8 series × 120 rows of synth_hist data. Sums of integer
bucket counts below 2^53 are exact in any atomic order, so the last-sample
grids compare with assert_array_equal; increase compares at the histogram
tests' rtol=1e-9, atol=1e-12. The one CPU test checks, with the model alone,
that the chosen inputs really reach the edges the cases are named for."""
import numpy as np
import pytest

import hist_funcs_model as model
from test_hist import _multichunk_cases, make_hist_store, synth_hist
from test_hist_mm import synth_mm

STEP = 15000


@pytest.fixture(scope="module")
def engine(fdb):
    return fdb.Engine(0)


def decoded_chunks(oracle, st, sid, with_corr=False):
    """[(stored ts, raw rows[, in-chunk corrections])] of one series."""
    out = []
    for ci in range(st.num_chunks(sid)):
        tsb, vab, n, _, _ = st.chunk(sid, ci)
        ts = np.asarray(oracle.decode_longs(tsb))[:n].astype(np.int64)
        raw = oracle.hist_decode(vab).astype(np.float64)
        assert raw.shape[0] == n
        if with_corr:
            out.append((ts, raw, oracle.hist_corrections(vab).astype(np.float64)))
        else:
            out.append((ts, raw))
    return out


def stored_ts(oracle, st, sid, ci=0):
    tsb, _, n, _, _ = st.chunk(sid, ci)
    return np.asarray(oracle.decode_longs(tsb))[:n].astype(np.int64)


class Case:
    def __init__(self, st, q, nb, groups):
        self.st, self.q, self.nb, self.groups = st, q, nb, groups
        self.ng = max(groups) + 1

    def expect_last(self, oracle):
        """(sums [G,W,nb], counts [G,W], {(sid, w): (chunk, row)})"""
        q, nw = self.q, self.q.num_windows
        sums = np.zeros((self.ng, nw, self.nb))
        cnts = np.zeros((self.ng, nw))
        hits = {}
        for sid, g in enumerate(self.groups):
            chunks = decoded_chunks(oracle, self.st, sid)
            for w in range(nw):
                w_end = q.start + w * q.step
                hit = model.last_sample_window(chunks, w_end - q.window, w_end)
                if hit is None:
                    continue
                sums[g, w] += chunks[hit[0]][1][hit[1]]
                cnts[g, w] += 1
                hits[(sid, w)] = hit
        return sums, cnts, hits

    def expect_increase(self, oracle):
        q, nw = self.q, self.q.num_windows
        sums = np.zeros((self.ng, nw, self.nb))
        cnts = np.zeros((self.ng, nw))
        for sid, g in enumerate(self.groups):
            chunks = decoded_chunks(oracle, self.st, sid, with_corr=True)
            for w in range(nw):
                w_end = q.start + w * q.step
                r = model.increase_window(oracle, chunks, w_end - q.window,
                                          w_end, self.nb)
                if r is not None:
                    sums[g, w] += r
                    cnts[g, w] += 1
        return sums, cnts


def last_query(fdb, start, step, nw, window, ng):
    return fdb.make_query(int(start), step, int(start) + (nw - 1) * step,
                          window, fdb.FN_LAST, fdb.AGG_SUM, ng)


def build_last_cases(fdb, oracle):
    cases = {}

    # windows that end before the first sample; three series share group 0,
    # each with its own first sample
    rng = np.random.default_rng(101)
    series = [synth_hist(rng, 40, start_ts=s)
              for s in (100000, 130000, 190000, 100000, 160000)]
    groups = [0, 0, 0, 1, 1]
    st = make_hist_store(fdb, series, groups=groups)
    cases["before_first"] = Case(
        st, last_query(fdb, 100000 - 6 * STEP, STEP, 30, 300000, 2), 8, groups)

    # lookback (9 s) shorter than the scrape gap (15 s): empty windows fall
    # between samples; window 0 starts exactly on sample 5; step < window
    rng = np.random.default_rng(102)
    st = make_hist_store(fdb, [synth_hist(rng, 40)])
    ts = stored_ts(oracle, st, 0)
    cases["short_lookback"] = Case(
        st, last_query(fdb, ts[5] + 9000, 3000, 100, 9000, 1), 8, [0])

    # window 0 ends exactly on sample 7; step (45 s) > window (20 s): E hops
    # three elements a window, over section bases it does not stop on; the
    # second series has TypeDrop sections
    rng = np.random.default_rng(103)
    series = [synth_hist(rng, 60), synth_hist(rng, 60, reset_p=0.08)]
    st = make_hist_store(fdb, series, groups=[0, 1])
    ts = stored_ts(oracle, st, 0)
    cases["exact_end_hops"] = Case(
        st, last_query(fdb, ts[7], 45000, 15, 20000, 2), 8, [0, 1])

    # windows past the last sample, inside the lookback and beyond it
    rng = np.random.default_rng(104)
    series = [synth_hist(rng, 30), synth_hist(rng, 30)]
    st = make_hist_store(fdb, series, groups=[0, 1])
    ts = stored_ts(oracle, st, 0)
    cases["past_last"] = Case(
        st, last_query(fdb, ts[-10], STEP, 18, 60000, 2), 8, [0, 1])

    # E stops on every element in turn: section bases (16, 32), section ends
    # (15, 31) and the first element of each TypeDrop section
    rng = np.random.default_rng(105)
    series = [synth_hist(rng, 60), synth_hist(rng, 60, reset_p=0.08)]
    st = make_hist_store(fdb, series, groups=[0, 1])
    cases["sections"] = Case(
        st, last_query(fdb, 100000 + 1000, STEP, 60, 20000, 2), 8, [0, 1])

    # chunk seams: series 0 restarts near zero after a 100 s gap (next chunk
    # starts beyond wEnd for the windows in the gap; the seam is a counter
    # drop, which the last sample ignores); series 1 continues seamlessly
    rng = np.random.default_rng(106)
    a_ts, a = synth_hist(rng, 20)
    b_ts, b = synth_hist(rng, 20, start_ts=int(a_ts[-1]) + 100000)
    c_ts, c = synth_hist(rng, 20)
    d_ts, d = synth_hist(rng, 20, start_ts=int(c_ts[-1]) + STEP)
    st = make_hist_store(fdb, [[(a_ts, a), (b_ts, b)],
                               [(c_ts, c), (d_ts, d + c[-1])]], groups=[0, 1])
    ts = stored_ts(oracle, st, 0)
    cases["seam"] = Case(
        st, last_query(fdb, ts[5] + 1000, STEP, 45, 60000, 2), 8, [0, 1])

    # bucket counts around the 8-value NibblePack group and the wave width
    for nb in (1, 8, 9, 64):
        rng = np.random.default_rng(200 + nb)
        groups = [0, 0, 0, 1, 1, 2, 2, 2]
        series = [synth_hist(rng, 50, nb=nb, reset_p=0.03) for _ in groups]
        st = make_hist_store(fdb, series, nb=nb, groups=groups)
        cases[f"nb{nb}"] = Case(
            st, last_query(fdb, 100000 + 10 * STEP + 500, STEP, 50, 300000, 3),
            nb, groups)
    return cases


def build_increase_cases(fdb, oracle):
    rng = np.random.default_rng(47)
    nb = 8
    shapes = _multichunk_cases(rng, nb) + [[synth_hist(rng, 60, nb=nb)]]
    names = ["three_chunks", "seam_drop", "resets_and_gap", "equal_seam",
             "clean_single"]
    cases = {}
    for name, shape in zip(names, shapes):
        st = make_hist_store(fdb, [shape], nb=nb)
        start = int(stored_ts(oracle, st, 0)[10])
        end = int(stored_ts(oracle, st, 0, len(shape) - 1)[-1]) + 30000
        q = fdb.make_query(start, 30000, end, 300000, fdb.FN_INCREASE,
                           fdb.AGG_SUM, 1)
        cases[name] = Case(st, q, nb, [0])
    return cases


LAST_NAMES = ["before_first", "short_lookback", "exact_end_hops", "past_last",
              "sections", "seam", "nb1", "nb8", "nb9", "nb64"]
INCREASE_NAMES = ["three_chunks", "seam_drop", "resets_and_gap", "equal_seam",
                  "clean_single"]


@pytest.fixture(scope="module")
def last_cases(fdb, oracle):
    """name -> (case, expected sums, counts, hits): computed once, shared"""
    out = {}
    for name, case in build_last_cases(fdb, oracle).items():
        out[name] = (case,) + case.expect_last(oracle)
    assert sorted(out) == sorted(LAST_NAMES)
    return out


@pytest.fixture(scope="module")
def increase_cases(fdb, oracle):
    out = {}
    for name, case in build_increase_cases(fdb, oracle).items():
        out[name] = (case,) + case.expect_increase(oracle)
    assert sorted(out) == sorted(INCREASE_NAMES)
    return out


def drop_rows(oracle, st, sid):
    """first rows of the TypeDrop sections of a single-chunk series"""
    _, vab, _, _, _ = st.chunk(sid, 0)
    corr = oracle.hist_corrections(vab)
    return [i for i in range(1, len(corr)) if (corr[i] != corr[i - 1]).any()]


def test_case_inputs_cover_the_edges(fdb, oracle, last_cases, increase_cases):
    """CPU, model only: every case has at least half of its windows non-empty
    and at least one empty one where it is about emptiness, and the edges in
    the case names are really reached."""
    for name, (case, _, cnts, _) in list(last_cases.items()) + \
            [(n, v + (None,)) for n, v in increase_cases.items()]:
        assert (cnts > 0).mean() >= 0.5, name
        assert case.st.num_series <= 8, name
        for sid in range(case.st.num_series):
            rows = sum(case.st.chunk(sid, ci)[2]
                       for ci in range(case.st.num_chunks(sid)))
            assert rows <= 120, name
    rows_of = lambda hits, sid: {h for (s, _), h in hits.items() if s == sid}

    case, _, cnts, hits = last_cases["before_first"]
    first = [stored_ts(oracle, case.st, sid)[0] for sid in range(5)]
    assert case.q.start < min(first) and (cnts[0, :6] == 0).all()
    assert sorted(set(cnts[0])) == [0, 1, 2, 3]     # the group fills up

    case, _, cnts, hits = last_cases["short_lookback"]
    ts = stored_ts(oracle, case.st, 0)
    assert case.q.start - case.q.window == ts[5] and hits[(0, 0)] == (0, 5)
    assert case.q.start < ts[6]                     # ... and it is alone there
    assert case.q.step < case.q.window < int(np.diff(ts).min())
    assert 0.2 < (cnts == 0).mean() <= 0.5

    case, _, cnts, hits = last_cases["exact_end_hops"]
    ts = stored_ts(oracle, case.st, 0)
    assert case.q.start == ts[7] and hits[(0, 0)] == (0, 7)
    assert case.q.step > case.q.window
    stops = sorted(r for _, r in rows_of(hits, 0))
    assert min(np.diff(stops)) >= 2 and max(stops) > 48
    assert {16, 32, 48} - set(stops)     # a section base is hopped over
    assert drop_rows(oracle, case.st, 1)

    case, _, cnts, hits = last_cases["past_last"]
    ts = stored_ts(oracle, case.st, 0)
    w_end = case.q.start + np.arange(case.q.num_windows) * case.q.step
    past = w_end > ts[-1]
    inside = past & (w_end - case.q.window <= ts[-1])
    assert inside.sum() >= 3 and (cnts[0][inside] == 1).all()
    assert (past & ~inside).sum() >= 3 and (cnts[0][past & ~inside] == 0).all()
    assert all(hits[(0, w)] == (0, 29) for w in np.nonzero(inside)[0])

    case, _, cnts, hits = last_cases["sections"]
    assert {15, 16, 31, 32} <= {r for _, r in rows_of(hits, 0)}
    drops = drop_rows(oracle, case.st, 1)
    assert drops and set(drops) <= {r for _, r in rows_of(hits, 1)}
    assert case.q.step < case.q.window

    case, _, cnts, hits = last_cases["seam"]
    a, b = stored_ts(oracle, case.st, 0, 0), stored_ts(oracle, case.st, 0, 1)
    w_end = case.q.start + np.arange(case.q.num_windows) * case.q.step
    gap = (w_end > a[-1]) & (w_end < b[0])
    held = [w for w in np.nonzero(gap)[0] if (0, w) in hits]
    assert held and all(hits[(0, w)] == (0, 19) for w in held)
    assert any((0, w) not in hits for w in np.nonzero(gap)[0])
    assert (1, 0) in rows_of(hits, 0) and (1, 0) in rows_of(hits, 1)
    assert a[-1] < b[0]                  # strictly increasing across the seam
    raws = decoded_chunks(oracle, case.st, 0)
    assert model._lex_less(raws[1][1][0], raws[0][1][-1])   # the seam drops

    for nb in (1, 8, 9, 64):
        case, sums, cnts, _ = last_cases[f"nb{nb}"]
        assert sums.shape[2] == nb and cnts.max() == 3
        assert sums.max() < 2.0 ** 53


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAST_NAMES)
def test_last_sample(fdb, engine, last_cases, name):
    case, want_s, want_c, _ = last_cases[name]
    nw = case.q.num_windows
    gs = np.full(case.ng * nw * case.nb, -1.0)
    gc = np.full(case.ng * nw, -1.0)
    engine.query_hist(engine.upload(case.st), case.q, case.nb,
                      out_bucket_sums=gs, out_counts=gc)
    assert (want_c > 0).mean() >= 0.5
    # exact, empty cells included: count 0 and zero sums where the model says so
    np.testing.assert_array_equal(gc, want_c.ravel())
    np.testing.assert_array_equal(gs, want_s.ravel())


@pytest.mark.gpu
def test_last_sample_companion_columns(fdb, oracle, engine):
    """max/min are the companion values at the E row, merged across series —
    not the window fold FDB_FN_SUM_OVER_TIME reports on the same data."""
    rng = np.random.default_rng(77)
    nb, groups = 8, [0, 1, 2, 0, 1, 2]
    series = [synth_mm(rng, 60, nb=nb, reset_p=0.03) for _ in groups]
    st = fdb.ChunkStore()
    st.set_max_rows(25)                  # three chunks a series
    for g, (ts, bv, mx, mn) in zip(groups, series):
        st.append_hist_mm(st.add_series(g, fdb.COL_HIST), ts, bv, mx, mn)
    st.seal()
    q = last_query(fdb, 100000 + 5 * STEP + 700, STEP, 60, 60000, 3)
    case = Case(st, q, nb, groups)
    want_s, want_c, hits = case.expect_last(oracle)
    nw = q.num_windows
    want_mx = np.full((3, nw), np.nan)
    want_mn = np.full((3, nw), np.nan)
    for (sid, w), (ci, row) in hits.items():
        g = groups[sid]
        grow = sum(st.chunk(sid, c)[2] for c in range(ci)) + row
        x, n = series[sid][2][grow], series[sid][3][grow]
        if not np.isnan(x) and not x <= want_mx[g, w]:
            want_mx[g, w] = x
        if not np.isnan(n) and not n >= want_mn[g, w]:
            want_mn[g, w] = n
    assert (want_c > 0).mean() >= 0.5 and (want_c == 0).any()
    assert {ci for ci, _ in hits.values()} == {0, 1, 2}

    ds = engine.upload(st)

    def run(func):
        q.func_id = func
        gs, gc = np.zeros(3 * nw * nb), np.zeros(3 * nw)
        gmx, gmn = np.zeros(3 * nw), np.zeros(3 * nw)
        engine.query_hist_mm(ds, q, nb, out_bucket_sums=gs, out_counts=gc,
                             out_max=gmx, out_min=gmn)
        return gs, gc, gmx, gmn

    gs, gc, gmx, gmn = run(fdb.FN_LAST)
    np.testing.assert_array_equal(gc, want_c.ravel())
    np.testing.assert_array_equal(gs, want_s.ravel())
    np.testing.assert_array_equal(gmx, want_mx.ravel())
    np.testing.assert_array_equal(gmn, want_mn.ravel())
    _, _, fmx, fmn = run(fdb.FN_SUM_OVER_TIME)
    both = ~np.isnan(gmx) & ~np.isnan(fmx)
    assert (fmx[both] >= gmx[both]).all() and (fmx[both] > gmx[both]).any()
    both = ~np.isnan(gmn) & ~np.isnan(fmn)
    assert (fmn[both] <= gmn[both]).all() and (fmn[both] < gmn[both]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", INCREASE_NAMES)
def test_increase(fdb, engine, increase_cases, name):
    case, want_s, want_c = increase_cases[name]
    nw = case.q.num_windows
    gs = np.full(case.ng * nw * case.nb, -1.0)
    gc = np.full(case.ng * nw, -1.0)
    engine.query_hist(engine.upload(case.st), case.q, case.nb,
                      out_bucket_sums=gs, out_counts=gc)
    assert (want_c > 0).mean() >= 0.5
    np.testing.assert_array_equal(gc, want_c.ravel())
    empty = np.repeat(want_c.ravel() == 0, case.nb)
    assert (gs[empty] == 0).all()
    np.testing.assert_allclose(gs, want_s.ravel(), rtol=1e-9, atol=1e-12)


@pytest.mark.gpu
def test_increase_scales_rate(fdb, engine, increase_cases):
    """rate × window seconds is the model's increase up to rounding (one
    divide and two multiplies): the same walk, only the scaling differs"""
    case, want_s, _ = increase_cases["resets_and_gap"]
    nw = case.q.num_windows
    q = fdb.make_query(case.q.start, case.q.step, case.q.end, case.q.window,
                       fdb.FN_HIST_RATE, fdb.AGG_SUM, 1)
    gs = np.zeros(nw * case.nb)
    engine.query_hist(engine.upload(case.st), q, case.nb, out_bucket_sums=gs)
    np.testing.assert_allclose(gs * (q.window / 1000.0), want_s.ravel(),
                               rtol=1e-9, atol=1e-12)


@pytest.mark.gpu
def test_increase_with_max_min_raises(fdb, engine):
    rng = np.random.default_rng(5)
    st = fdb.ChunkStore()
    ts, bv, mx, mn = synth_mm(rng, 30)
    st.append_hist_mm(st.add_series(0, fdb.COL_HIST), ts, bv, mx, mn)
    st.seal()
    ds = engine.upload(st)
    q = fdb.make_query(int(ts[5]), STEP, int(ts[20]), 60000, fdb.FN_INCREASE,
                       fdb.AGG_SUM, 1)
    nw = q.num_windows
    gs, gc = np.zeros(nw * 8), np.zeros(nw)
    engine.query_hist_mm(ds, q, 8, out_bucket_sums=gs, out_counts=gc)
    assert gc.sum() > 0
    with pytest.raises(RuntimeError, match="max/min"):
        engine.query_hist_mm(ds, q, 8, out_bucket_sums=gs, out_counts=gc,
                             out_max=np.zeros(nw), out_min=np.zeros(nw))
    q.func_id = fdb.FN_DELTA                       # still rejected
    with pytest.raises(RuntimeError, match="FDB_FN_LAST"):
        engine.query_hist(ds, q, 8, out_bucket_sums=gs, out_counts=gc)
