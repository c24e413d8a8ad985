"""The fast scan's upload-time decode descriptors and four-rows-per-lane
decode against the oracle (real MI355X).

fdb_dataset_upload parses every series' two vector headers once into a 64-byte
descriptor (csrc/fast_desc.h); fast_scan_kernel loads it with one scalar load
and decodes packed 8/16-bit delta-delta vectors four rows per lane with
128-bit LDS stores, values through an exact i32 path when the descriptor's
val_exact32 flag allows it (csrc/scan_common.h). One store per vector
encoding, single-chunk series of 1..400 rows (the 4-row lane groups and the
256-row pass boundary), at most 64 series per store.

Every store is asked last_over_time, count_over_time and timestamp() on a
grid whose window equals its step and is shorter than the smallest gap
between two rows, so every row is alone in some window: each decoded value
and each decoded timestamp is compared with the oracle bit for bit. rate and
avg_over_time run at the suite's rtol 1e-9 / atol 1e-12.

What the encoder (csrc/chunk_builder.cpp) decides, and what that means here:
 * chunks of one or two rows are always raw 64-bit, whatever the store's law;
   the expected encoding is asserted from three rows up;
 * a timestamp vector whose deltas all lie within +-250 ms of the line is
   const; one that fits signed 8 bits always does, so the builder's only
   packed 8-bit timestamps are UNSIGNED (an outlier of 251..255 ms, "t8u").
   The signed 8-bit case (step 100 ms, jitter +-100, one +-120 outlier) and
   raw i64 timestamps of three or more rows are legal frozen vectors the
   builder never emits: those two stores are encoded here and enter through
   add_encoded_chunk;
 * window edges are = 0 (mod 10) relative to T0. Only the signed 8-bit store
   has runs of equal timestamps; its rows sit at 5 (mod 10), off every edge
   (tests/test_gpu_window_bounds.py explains why). The other stores' rows are
   strictly increasing."""
import struct

import numpy as np
import pytest

import window_cases as wc
from conftest import build_store

pytestmark = pytest.mark.gpu

T0 = 10_000_000
SIZES = [1, 2, 3, 4, 5, 63, 64, 65, 240, 255, 256, 257, 399, 400]
FN_RATE, FN_COUNT, FN_AVG, FN_LAST, FN_TIMESTAMP = 0, 4, 5, 12, 14

WF_DDV, WF_CONST, WF_RAW = 0x0808, 0x0608, 0x0506


def _deltas(rng, n, lo, hi, hit):
    """n offsets from a line in [lo, hi], first and last 0 (the encoder's
    slope is then the line's), `hit` present so the width is the one meant."""
    d = rng.integers(lo, hi + 1, n)
    d[0] = 0
    d[-1] = 0
    if n >= 3:
        d[1] = hit
    return d.astype(np.int64)


# timestamp laws: name -> (scrape step, lo, hi, hit, expected (wf, nbits, sign))
TS_LAWS = {
    "tconst": (15000, 0, 0, 0, (WF_CONST, 0, 0)),
    "t8u": (1000, 0, 255, 255, (WF_DDV, 8, 0)),
    "t16s": (15000, -300, 300, -300, (WF_DDV, 16, 1)),      # the bench law
    "t16u": (100_000, 0, 65535, 65535, (WF_DDV, 16, 0)),
}
# value laws: name -> (init, slope, lo, hi, hit, expected)
VAL_LAWS = {
    "v2u": (1000, 7, 0, 3, 3, (WF_DDV, 2, 0)),
    "v4u": (1000, 40, 0, 15, 15, (WF_DDV, 4, 0)),
    "v8s": (5000, 300, -128, 127, -128, (WF_DDV, 8, 1)),
    "v8u": (5000, 300, 0, 255, 255, (WF_DDV, 8, 0)),
    "v16s": (10**6, 70000, -32768, 32767, -32768, (WF_DDV, 16, 1)),
    "v16u": (10**6, 70000, 0, 65535, 65535, (WF_DDV, 16, 0)),
    "v32": (10**10, 3, -(1 << 30), 1 << 30, 1 << 30, (WF_DDV, 32, 1)),
    "vconst": (123456, 11, 0, 0, 0, (WF_CONST, 0, 0)),
    "vneg": (-10**9, -1000, -128, 127, 127, (WF_DDV, 8, 1)),
    # 2^52 + 1: must miss val_exact32 (|init| >= 2^52) and still be exact
    "vbig": ((1 << 52) + 1, 300, -128, 127, -128, (WF_DDV, 8, 1)),
}
TS_STORES = ["tconst", "t8u", "t8s", "t16s", "t16u", "t32", "traw"]
VAL_STORES = list(VAL_LAWS) + ["vraw", "vresets"]


def _vec_info(b):
    """(wire format, nbits, sign) of a frozen vector."""
    wf = struct.unpack_from("<H", b, 4)[0]
    if wf == WF_DDV:
        return wf, b[26] & 0x7f, b[26] >> 7
    return wf, 0, 0


def _enc_raw_i64(ts):
    n = len(ts)
    return (struct.pack("<IHH", 4 + 8 * n, WF_RAW, 64 | 0x80) +
            np.asarray(ts, dtype="<i8").tobytes())


def _enc_ddv_s8(ts):
    """Packed delta-delta, signed 8-bit inner vector."""
    n = len(ts)
    slope = int(ts[-1] - ts[0]) // (n - 1)
    d = np.asarray(ts, dtype=np.int64) - (int(ts[0]) + slope * np.arange(n))
    assert d.min() >= -128 and d.max() <= 127
    inner = struct.pack("<IHBB", 4 + n, 0x0806, 8 | 0x80, 0) + d.astype("<i1").tobytes()
    body = struct.pack("<Iqi", WF_DDV, int(ts[0]), slope) + inner
    return struct.pack("<I", len(body)) + body


def _bench_ts(rng, n):
    return T0 + 15000 * np.arange(n) + _deltas(rng, n, -300, 300, -300)


def _bench_vals(rng, n):
    return np.cumsum(rng.poisson(10.0, n).astype(np.float64))


class Case:
    """One store; .ranges are the (start, step, num_windows) grids on which
    every row is alone in a window of one step."""

    def __init__(self, fdb, engine, name):
        rng = np.random.default_rng(5000 + (TS_STORES + VAL_STORES).index(name))
        self.fdb = fdb
        kind = fdb.COL_COUNTER if name in TS_STORES + ["vresets"] else fdb.COL_GAUGE
        encoded = name in ("t8s", "traw")
        rows, self.qstep, self.scrape = [], 10000, 15000
        for n in SIZES:
            if name in TS_LAWS:
                step, lo, hi, hit, _ = TS_LAWS[name]
                ts = T0 + step * np.arange(n) + _deltas(rng, n, lo, hi, hit)
                self.scrape = step
                self.qstep = {1000: 700, 100_000: 30000}.get(step, 10000)
            elif name == "t8s":
                j = rng.integers(-10, 11, n) * 10
                j[0] = j[-1] = 0          # the line's slope is the step
                if n >= 3:
                    j[n // 2] = 120 if n % 2 else -120
                ts = T0 + 5 + np.maximum.accumulate(100 * np.arange(n) + j)
                self.scrape, self.qstep = 100, 10
            elif name == "t32":                # two clusters, one 2^30 gap
                gaps = rng.integers(900, 1101, n)
                if n >= 2:
                    gaps[n // 2 - 1] = 1 << 30
                ts = T0 + np.concatenate([[0], np.cumsum(gaps)[:-1]])
                self.scrape, self.qstep = 1000, 800
            else:
                ts = _bench_ts(rng, n)
            if name in VAL_LAWS:
                init, slope, lo, hi, hit, _ = VAL_LAWS[name]
                vals = (init + slope * np.arange(n) +
                        _deltas(rng, n, lo, hi, hit)).astype(np.float64)
                assert np.all(vals == np.rint(vals)) and abs(vals).max() < 2.0**53
            elif name == "vraw":
                vals = np.cumsum(rng.normal(0, 1, n)) + rng.random(n) + 0.3
            else:
                vals = _bench_vals(rng, n)
                if name == "vresets":
                    for i in np.nonzero(rng.random(n) < 0.05)[0]:
                        vals[i:] -= vals[i]
                    if n >= 3:
                        vals[n // 2:] -= vals[n // 2]       # at least one reset
            rows.append((np.asarray(ts, dtype=np.int64), vals))
        series = [[[(int(t), float(v)) for t, v in zip(ts, vals)]]
                  for ts, vals in rows]
        groups = [i % 3 for i in range(len(rows))]
        built = build_store(fdb, series, kind=kind, groups=groups)
        if encoded:       # same value bytes, timestamps encoded here
            st = fdb.ChunkStore()
            for i, (ts, _) in enumerate(rows):
                sid = st.add_series(groups[i], kind)
                _, vab, nr, t_lo, t_hi = built.chunk(i, 0)
                tsb = (_enc_raw_i64(ts) if name == "traw" or len(ts) < 3
                       else _enc_ddv_s8(ts))
                fdb.add_encoded_chunk(st, sid, tsb, vab, nr, t_lo, t_hi)
            st.seal()
            built = st
        self.store = built
        want_ts = (TS_LAWS[name][4] if name in TS_LAWS else
                   {"t8s": (WF_DDV, 8, 1), "t32": (WF_DDV, 32, 1),
                    "traw": (WF_RAW, 0, 0)}.get(name, TS_LAWS["t16s"][4]))
        want_val = (VAL_LAWS[name][5] if name in VAL_LAWS else
                    (WF_RAW, 0, 0) if name == "vraw" else None)
        for i, n in enumerate(SIZES):
            tsb, vab, nr, _, _ = built.chunk(i, 0)
            assert nr == n
            if n >= 3:
                assert _vec_info(tsb) == want_ts, (name, n)
                if want_val:
                    assert _vec_info(vab) == want_val, (name, n)
            if name == "vresets" and n >= 3:
                assert struct.unpack_from("<H", vab, 6)[0] & 0x8000   # dropped
        # grids: one per cluster of rows (t32 has two), two windows of margin
        allts = np.unique(np.concatenate([ts for ts, _ in rows]))
        cuts = np.nonzero(np.diff(allts) > 1000 * self.qstep)[0] + 1
        self.ranges = []
        for seg in np.split(allts, cuts):
            lo = (int(seg[0]) - T0) // self.qstep * self.qstep + T0 - 2 * self.qstep
            nw = (int(seg[-1]) - lo) // self.qstep + 3
            self.ranges.append((lo, self.qstep, nw))
        assert sum(r[2] for r in self.ranges) < 10_000
        self.ds = engine.upload(self.store)


@pytest.fixture(scope="module")
def engine(fdb):
    return fdb.Engine(0)


@pytest.fixture(scope="module")
def cases(fdb, engine):
    return wc.case_cache(lambda name: Case(fdb, engine, name))


@pytest.mark.parametrize("name", TS_STORES + VAL_STORES)
def test_every_row_vs_oracle(fdb, oracle, engine, cases, name):
    case = cases(name)
    seen = 0
    for start, step, nw in case.ranges:
        end = start + (nw - 1) * step
        for func in (FN_LAST, FN_COUNT, FN_TIMESTAMP):
            q = fdb.make_query(start, step, end, step, func)
            assert q.num_windows == nw
            got, want = wc.run_both(oracle, engine, case, q)
            wc.assert_exact(got, want)
            if func == FN_COUNT:
                seen += int(np.nansum(want))
                if name != "t8s":       # strictly increasing rows: one per window
                    assert np.nanmax(want) == 1
    # the grids put every row of every series into some window (a row on an
    # edge is in two)
    assert seen >= sum(SIZES)
    # a lookback of 20 scrape intervals over the first cluster of rows
    start, step, nw = case.ranges[0]
    step = max(case.scrape // 10 * 10, 10)
    nw = min(nw * case.qstep // step + 1, 700)
    for func in (FN_RATE, FN_AVG):
        q = fdb.make_query(start, step, start + (nw - 1) * step, 20 * step, func)
        got, want = wc.run_both(oracle, engine, case, q)
        assert np.isfinite(want).any()
        wc.assert_close(got, want)


def test_avg_sc_second_table(fdb, oracle, engine):
    """avg over sum+count columns: the count column (integral, packed
    delta-delta) is scanned through the dataset's second descriptor table."""
    rng = np.random.default_rng(77)
    st = fdb.ChunkStore()
    for n in SIZES:
        ts = _bench_ts(rng, n)
        sums = rng.normal(50, 20, n) * rng.integers(1, 30, n)
        counts = rng.integers(1, 30, n).astype(np.float64)
        sid = st.add_series(0, fdb.COL_GAUGE)
        st.append_sc(sid, ts, sums, counts)
    st.seal()
    ds = engine.upload(st)
    q = fdb.make_query(T0, 15000, T0 + 410 * 15000, 300_000, FN_AVG)
    want = oracle.query_exec_avg_sc(st.view(), q, st.num_series, q.num_windows)
    got = engine.query_avg_sc(ds, q)
    assert np.isfinite(want).any()
    wc.assert_close(got, want)


def test_fused_group_sum(fdb, oracle, engine, cases, monkeypatch):
    """sum by (group) through the fused-group emit: the descriptor table is
    indexed through the group-sorted series order."""
    monkeypatch.setenv("FDB_FUSED_GROUP", "1")
    case = cases("t16s")
    for func in (FN_RATE, FN_COUNT):
        q = fdb.make_query(T0, 15000, T0 + 240 * 15000, 300_000, func,
                           fdb.AGG_SUM, 3)
        got, want = wc.run_both(oracle, engine, case, q)
        wc.assert_close(got, want)
