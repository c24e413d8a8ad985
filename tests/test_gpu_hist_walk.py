"""hist2 walk branches vs the CPU oracle: unstaged (> 242 B) and staged
elements, stage-window straddles, bucket counts off the 8-value group size,
TypeDrop sections against the 16-element section size, chunk-seam drops, many
tiny chunks under one window with max/min companions, a series without
chunks, SumOverTime across many chunks and the FDB_HIST_WAVES=4 build.

Every series has a group of its own, so each output cell has one addend.
Windows step 15 s over a 15 s scrape grid; each store runs with a 300 s, a
15 s (= step) and a 5 s window, from two steps before the first grid point to
four steps after the last. A rate needs two samples, so a 5 s window over a
15 s grid alone would leave every rate cell empty: each series therefore has
a few row pairs 2.5 s apart, placed to end on a window's end.
"""
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T0, STEP = 100000, 15000
WINDOWS = [300000, 15000, 5000]
UNSTAGED_OVER = 242          # elen + 14 + shift <= 256 is the staged parse


def parse_sections(vab):
    """[(type byte, [element payload lengths])] of a sect-delta hist vector:
    def at 11, its size as u16 at 9, sections of u16 bytes / u8 n / u8 type,
    elements of u16 len + payload."""
    end = 4 + struct.unpack_from("<I", vab, 0)[0]
    pos = 11 + struct.unpack_from("<H", vab, 9)[0]
    sections = []
    while pos < end:
        sbytes, n, stype = struct.unpack_from("<HBB", vab, pos)
        p, lens = pos + 4, []
        for _ in range(n):
            elen = struct.unpack_from("<H", vab, p)[0]
            lens.append(elen)
            p += 2 + elen
        assert p == pos + 4 + sbytes
        sections.append((stype, lens))
        pos = p
    return sections


def store_sections(st, sid):
    return [s for c in range(st.num_chunks(sid))
            for s in parse_sections(st.chunk(sid, c)[1])]


def elem_lens(st, sid=0):
    return np.array([l for _, lens in store_sections(st, sid) for l in lens])


def grid_ts(rng, n, pairs):
    """15 s grid with +-250 ms jitter (row 0 exact, so a window ends on it);
    rows r-1, r of each pair sit 4 s and 1.5 s before grid point r."""
    ts = T0 + np.arange(n) * STEP + rng.integers(-250, 251, n)
    ts[0] = T0
    for r in pairs:
        ts[r - 1] = T0 + r * STEP - 4000
        ts[r] = T0 + r * STEP - 1500
    assert np.all(np.diff(ts) > 0)
    return ts.astype(np.int64)


def counters(rng, n, nb, hi, resets=(), big_rows=(), big_hi=0):
    """Cumulative-LE rows: per-bucket counters grow by [1, hi) a row
    ([1, big_hi) on big_rows); a reset row restarts every counter."""
    cur = np.zeros(nb, dtype=np.uint64)
    rows = np.zeros((n, nb), dtype=np.uint64)
    for i in range(n):
        if i in resets:
            cur = np.zeros(nb, dtype=np.uint64)
        top = big_hi if i in big_rows else hi
        cur = cur + rng.integers(1, top, nb).astype(np.uint64)
        rows[i] = cur
    return np.cumsum(rows, axis=1)


def plain_store(fdb, series):
    """series: (ts, cum) or a list of them (explicit chunk cuts); group = sid."""
    st = fdb.ChunkStore()
    for i, entry in enumerate(series):
        sid = st.add_series(i, fdb.COL_HIST)
        for ci, (ts, cum) in enumerate(entry if isinstance(entry, list) else [entry]):
            if ci > 0:
                st.cut_chunk(sid)
            st.append_hist(sid, ts, cum)
    st.seal()
    return st


def build_mixed(fdb):
    """Case 1: elements on both sides of the staged-parse line in one chunk."""
    rng = np.random.default_rng(101)
    n, nb = 48, 64
    series = [(grid_ts(rng, n, (8, 25, 31)),
               counters(rng, n, nb, 16, resets=(30,), big_rows=range(20, 30),
                        big_hi=2**31)) for _ in range(5)]
    st = plain_store(fdb, series)
    lens = elem_lens(st)
    assert (lens > UNSTAGED_OVER).any() and (lens <= UNSTAGED_OVER).any(), lens
    return st, nb, n


def build_large(fdb):
    """Case 2: every element straddles a 256-B stage window."""
    rng = np.random.default_rng(102)
    n, nb = 40, 64
    series = [(grid_ts(rng, n, (8, 25)), counters(rng, n, nb, 2**31))
              for _ in range(3)]
    st = plain_store(fdb, series)
    assert (elem_lens(st) > 256).all()
    return st, nb, n


def build_mid(fdb):
    """Case 3: two to three elements per stage window."""
    rng = np.random.default_rng(103)
    n, nb = 40, 64
    series = [(grid_ts(rng, n, (8, 25)), counters(rng, n, nb, 2**12))
              for _ in range(3)]
    st = plain_store(fdb, series)
    lens = elem_lens(st)
    assert lens.min() > 256 // 3 and lens.max() < 256 * 3 // 4, lens
    return st, nb, n


def build_nb(nb):
    """Case 4: a partly live last group; one bucket."""
    def build(fdb):
        rng = np.random.default_rng(104 + nb)
        n = 40
        hi = 2**40 if nb == 13 else 16
        series = [(grid_ts(rng, n, (8, 25)),
                   counters(rng, n, nb, hi, resets=(20,))) for _ in range(3)]
        return plain_store(fdb, series), nb, n
    return build


def build_resets(fdb):
    """Case 5: TypeDrop sections next to, on and after the 16-element section
    boundary, consecutive, and on a chunk's last element; a second series
    whose drops sit on chunk seams (chunk-boundary compare, not TypeDrop)."""
    rng = np.random.default_rng(105)
    n, nb = 48, 8
    drops = (1, 15, 16, 17, n - 1)
    a = (grid_ts(rng, n, (1, 16, n - 1)), counters(rng, n, nb, 16, resets=drops))
    ts = grid_ts(rng, n, (16, 33))
    cum = counters(rng, n, nb, 16, resets=(16, 32))
    b = [(ts[i:i + 16], cum[i:i + 16]) for i in (0, 16, 32)]
    st = plain_store(fdb, [a, b])
    # element index of each section start, by type
    starts, at = {0: [], 1: []}, 0
    for stype, lens in store_sections(st, 0):
        starts[stype].append(at)
        at += len(lens)
    assert starts[1] == list(drops), starts
    assert starts[0] == [0, 33], starts     # 16 elements after the drop at 17
    assert st.num_chunks(1) == 3
    assert all(stype == 0 for stype, _ in store_sections(st, 1))
    return st, nb, n


def build_tiny_mm(fdb):
    """Case 6: 5-row chunks with companions, and a series with no rows."""
    rng = np.random.default_rng(106)
    n, nb = 23, 13
    st = fdb.ChunkStore()
    st.set_max_rows(5)
    for g in range(3):
        sid = st.add_series(g, fdb.COL_HIST)
        if g == 1:
            continue                        # no chunks at all
        mx = rng.random(n) * 50
        mn = rng.random(n) * 5
        mx[rng.random(n) < 0.3] = np.nan
        mn[5:10] = np.nan                   # a whole chunk of NaN
        st.append_hist_mm(sid, grid_ts(rng, n, (5, 12)),
                          counters(rng, n, nb, 16, resets=(11,)), mx, mn)
    st.seal()
    assert [st.num_chunks(s) for s in range(3)] == [5, 0, 5]
    return st, nb, n


BUILDERS = {"mixed": build_mixed, "large": build_large, "mid": build_mid,
            "nb1": build_nb(1), "nb3": build_nb(3), "nb13": build_nb(13),
            "resets": build_resets, "tiny_mm": build_tiny_mm}


class Walk:
    """Stores, uploads and oracle results, each made once."""

    def __init__(self, fdb, oracle):
        self.fdb, self.oracle = fdb, oracle
        self.engine = fdb.Engine(0)
        self.stores, self.wants = {}, {}

    def store(self, case):
        if case not in self.stores:
            st, nb, n = BUILDERS[case](self.fdb)
            self.stores[case] = (st, self.engine.upload(st), nb, n)
        return self.stores[case]

    def query(self, case, window, fid):
        st, _, nb, n = self.store(case)
        return self.fdb.make_query(T0 - 2 * STEP, STEP, T0 + (n - 1 + 4) * STEP,
                                   window, fid, self.fdb.AGG_SUM,
                                   st.num_series, param=0.9)

    def want(self, case, window, fid):
        key = (case, window, fid)
        if key not in self.wants:
            st, _, nb, _ = self.store(case)
            q = self.query(case, window, fid)
            if case == "tiny_mm":
                w = self.oracle.query_exec_hist_mm(st.view(), q, nb)
            else:
                s, c, qu = self.oracle.query_exec_hist(st.view(), q, nb)
                w = (s, c, None, None, qu)
            assert (w[1] == 0).any() and (w[1] != 0).any(), key
            self.wants[key] = w
        return self.wants[key]

    def check(self, case, window, fid):
        ws, wc, wmx, wmn, wq = self.want(case, window, fid)
        _, ds, nb, _ = self.store(case)
        q = self.query(case, window, fid)
        cells = q.num_groups * q.num_windows
        gs, gc, gq = np.zeros(cells * nb), np.zeros(cells), np.zeros(cells)
        if wmx is None:
            self.engine.query_hist(ds, q, nb, out_bucket_sums=gs, out_counts=gc,
                                   out_quantile=gq)
        else:
            gmx, gmn = np.zeros(cells), np.zeros(cells)
            self.engine.query_hist_mm(ds, q, nb, out_bucket_sums=gs,
                                      out_counts=gc, out_max=gmx, out_min=gmn,
                                      out_quantile=gq)
            np.testing.assert_allclose(gmx, wmx, rtol=1e-12, equal_nan=True)
            np.testing.assert_allclose(gmn, wmn, rtol=1e-12, equal_nan=True)
        np.testing.assert_array_equal(gc, wc)
        np.testing.assert_allclose(gs, ws, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(gq, wq, rtol=1e-9, atol=1e-12, equal_nan=True)


@pytest.fixture(scope="module")
def walk(fdb, oracle):
    return Walk(fdb, oracle)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("case", ["mixed", "large", "mid", "nb1", "nb3", "nb13",
                                  "resets"])
def test_hist_rate_walk(walk, case, window):
    walk.check(case, window, walk.fdb.FN_HIST_RATE)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("func", ["rate", "sum"])
def test_tiny_chunks_companions_empty_series(walk, func, window):
    fid = walk.fdb.FN_HIST_RATE if func == "rate" else walk.fdb.FN_SUM_OVER_TIME
    _, wc, wmx, _, _ = walk.want("tiny_mm", window, fid)
    nw = wc.size // 3
    assert not wc[nw:2 * nw].any() and np.isnan(wmx[nw:2 * nw]).all()
    if window == 300000:    # non-empty windows per group, checked on the CPU
        filled = [int((wc[g * nw:(g + 1) * nw] != 0).sum()) for g in range(3)]
        assert filled == ([25, 0, 26] if func == "rate" else [27, 0, 27])
    walk.check("tiny_mm", window, fid)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("case", ["mixed", "resets"])
def test_hist_rate_walk_4_waves(walk, monkeypatch, case, window):
    monkeypatch.setenv("FDB_HIST_WAVES", "4")   # read per launch
    walk.check(case, window, walk.fdb.FN_HIST_RATE)
