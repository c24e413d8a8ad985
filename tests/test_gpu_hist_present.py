"""GPU histogram present steps (hist_present_kernel): fdb_hist_present on the
reference's literals and against the numpy model, the argument checks, and
fdb_query_exec_hist_present against scan-then-present."""
import json
import os

import numpy as np
import pytest

import hist_funcs_model as model
from test_hist import make_hist_store, synth_hist
from test_hist_mm import make_mm_store, synth_mm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "hist_present.json")
NAN = float("nan")
INF = float("inf")


@pytest.fixture(scope="module")
def engine(fdb):
    return fdb.Engine(0)


def present(fdb, engine, pid, sums, cnts, nb, first, mult, p0=0.0, p1=0.0,
            maxs=None, mins=None):
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    return fdb.hist_present(engine, pid, f64(sums).ravel(), f64(cnts), nb,
                            first, mult, p0=p0, p1=p1, maxs=f64(maxs),
                            mins=f64(mins))


def test_geometric_goldens(fdb, engine):
    """within the reference's own ± tolerance; its exact literals within the
    project's double-parity bound (pow is the only source of difference)"""
    g = json.load(open(GOLDEN))
    qm = g["quantile_minmax"]
    for c in qm["cases"]:
        v = np.array([c["values"]], dtype=np.float64)
        one = np.ones(1)
        mx, mn = np.array([float(c["max"])]), np.array([float(c["min"])])
        got = present(fdb, engine, fdb.HP_QUANTILE_MINMAX, v, one, 8,
                      qm["first"], qm["mult"], p0=c["q"], maxs=mx, mins=mn)[0]
        assert abs(got - c["expected"]) <= c["tol"], (c, got)
        if c["min"] == 0:     # HistogramMaxQuantileImpl: quantile(q, 0, max)
            got = present(fdb, engine, fdb.HP_MAX_QUANTILE, v, one, 8,
                          qm["first"], qm["mult"], p0=c["q"], maxs=mx,
                          mins=np.array([NAN]))[0]
            assert abs(got - c["expected"]) <= c["tol"], (c, got)
    q50 = g["quantile50"]
    v = np.array([c["values"] for c in q50["cases"]], dtype=np.float64)
    want = np.array([c["expected"] for c in q50["cases"]])
    got = present(fdb, engine, fdb.HP_QUANTILE, v, np.ones(4), 8,
                  q50["first"], q50["mult"], p0=q50["q"])
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)


def random_cells(rng, cells, nb):
    """cumulative-LE cells of rate-like (non-integral) sums, a few empty"""
    v = np.cumsum(rng.random((cells, nb)) * rng.integers(0, 3, (cells, nb)), axis=1)
    cnt = rng.integers(0, 4, cells).astype(np.float64)
    cnt[:3] = 0
    v[3] = 0.0                                   # top == 0 with a count
    return v, cnt


@pytest.mark.parametrize("nb", [2, 8, 64])
def test_matches_model_on_random_cells(fdb, engine, nb):
    rng = np.random.default_rng(300 + nb)
    cells = 200
    first, mult = (0.5, 1.5) if nb == 64 else (2.0, 2.0)
    tops = model.geometric_tops(first, mult, nb)
    v, cnt = random_cells(rng, cells, nb)
    # companion values around the interesting buckets, some NaN
    mx = np.array([tops[int(rng.integers(0, nb))] * (0.3 + rng.random())
                   for _ in range(cells)])
    mn = mx * rng.random(cells)
    mx[rng.random(cells) < 0.1] = NAN
    mn[rng.random(cells) < 0.1] = NAN
    le = tops[nb // 2]
    lo, up = tops[0] * 0.7, tops[nb - 1] * 0.6
    runs = [(fdb.HP_QUANTILE, 0.9, 0.0), (fdb.HP_QUANTILE, 0.0, 0.0),
            (fdb.HP_QUANTILE, 1.0, 0.0), (fdb.HP_QUANTILE, -0.5, 0.0),
            (fdb.HP_QUANTILE, 1.5, 0.0),
            (fdb.HP_QUANTILE_MINMAX, 0.95, 0.0), (fdb.HP_QUANTILE_MINMAX, 0.05, 0.0),
            (fdb.HP_MAX_QUANTILE, 0.99, 0.0),
            (fdb.HP_BUCKET, le, 0.0), (fdb.HP_BUCKET, le + 5e-11, 0.0),
            (fdb.HP_BUCKET, le * 1.01, 0.0),
            (fdb.HP_FRACTION, lo, up), (fdb.HP_FRACTION, 0.0, 0.0),
            (fdb.HP_FRACTION, up, lo), (fdb.HP_FRACTION, tops[0], tops[nb - 1]),
            (fdb.HP_FRACTION, 0.0, tops[nb - 1] * 4),
            (fdb.HP_FRACTION_MINMAX, lo, up),
            (fdb.HP_FRACTION_MINMAX, tops[nb // 2] * 0.8, tops[nb // 2] * 0.9)]
    for pid, p0, p1 in runs:
        want = np.array([
            model.present(pid, tops, v[i], p0, p1, mx=mx[i], mn=mn[i])
            if cnt[i] > 0 else NAN for i in range(cells)])
        got = present(fdb, engine, pid, v, cnt, nb, first, mult, p0=p0, p1=p1,
                      maxs=mx, mins=mn)
        assert np.isnan(got[:3]).all()
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=0,
                                   equal_nan=True, err_msg=str((pid, p0, p1)))
    # nb == 2 has an nb < 2 neighbour: one bucket gives NaN quantiles
    if nb == 2:
        got = present(fdb, engine, fdb.HP_QUANTILE, v[:, :1], cnt, 1, first, mult, p0=0.5)
        assert np.isnan(got).all()


def test_nan_sum_stays_inside_the_cell(fdb, engine):
    """a NaN bucket sum (NaN rank) must not walk past the cell's buckets"""
    v = np.array([[1.0, NAN, NAN, NAN], [1.0, 2.0, 3.0, 4.0]])
    got = present(fdb, engine, fdb.HP_QUANTILE, v, np.ones(2), 4, 2.0, 2.0, p0=0.5)
    assert np.isnan(got[0])
    assert got[1] == model.quantile(model.geometric_tops(2.0, 2.0, 4), v[1], 0.5)


def test_badarg(fdb, engine):
    v, one = np.ones((1, 8)), np.ones(1)
    mm = dict(maxs=np.ones(1), mins=np.ones(1))

    def bad(match, pid, nb=8, **kw):
        with pytest.raises(RuntimeError, match=match) as ei:
            present(fdb, engine, pid, np.ones((1, max(nb, 1))), one, nb,
                    2.0, 2.0, **kw)
        assert "rc=-3" in str(ei.value)

    for pid, extra in ((fdb.HP_FRACTION, {}), (fdb.HP_FRACTION_MINMAX, mm)):
        bad("should be >= 0", pid, p0=-1.0, p1=2.0, **extra)
        bad("should be >= 0", pid, p0=1.0, p1=-2.0, **extra)
        bad("should be >= 0", pid, p0=NAN, p1=2.0, **extra)
        bad("should be >= 0", pid, p0=1.0, p1=NAN, **extra)
    bad(r"\+Inf bucket", fdb.HP_BUCKET, p0=INF)
    for pid in (fdb.HP_QUANTILE_MINMAX, fdb.HP_MAX_QUANTILE, fdb.HP_FRACTION_MINMAX):
        bad("needs max and min", pid, p0=0.5, p1=0.6)
        bad("needs max and min", pid, p0=0.5, p1=0.6, maxs=np.ones(1))
    bad("unknown histogram present id", 6, p0=0.5)
    bad("unknown histogram present id", -1, p0=0.5)
    bad("num_buckets", fdb.HP_QUANTILE, nb=0, p0=0.5)
    bad("num_buckets", fdb.HP_QUANTILE, nb=65, p0=0.5)
    # -Inf is an ordinary le that matches no bucket
    assert np.isnan(present(fdb, engine, fdb.HP_BUCKET, v, one, 8, 2.0, 2.0, p0=-INF)[0])


def test_query_badarg(fdb, engine):
    """the scan-plus-present entry point checks before it scans"""
    rng = np.random.default_rng(8)
    ts, cum = synth_hist(rng, 30)
    ds = engine.upload(make_hist_store(fdb, [(ts, cum)]))
    q = fdb.make_query(int(ts[5]), 15000, int(ts[20]), 60000, fdb.FN_LAST,
                       fdb.AGG_SUM, 1, param=-1.0, param2=2.0)
    for pid, match in ((fdb.HP_FRACTION, "should be >= 0"),
                       (fdb.HP_QUANTILE_MINMAX, "needs max and min"),
                       (9, "unknown histogram present id")):
        with pytest.raises(RuntimeError, match=match) as ei:
            engine.query_hist_present(ds, q, 8, pid)
        assert "rc=-3" in str(ei.value)
    q.param = INF
    with pytest.raises(RuntimeError, match=r"\+Inf bucket"):
        engine.query_hist_present(ds, q, 8, fdb.HP_BUCKET)


@pytest.fixture(scope="module")
def mm_dataset(fdb, engine):
    """one series a group: a cell's rate sum has one addend, so two scans
    give the same bits whatever the atomic order"""
    rng = np.random.default_rng(91)
    series = [synth_mm(rng, 80, reset_p=0.03) for _ in range(4)]
    st = make_mm_store(fdb, series, groups=[0, 1, 2, 3])
    start = int(series[0][0][0]) - 45000       # the first windows are empty
    return engine.upload(st), start


@pytest.mark.parametrize("func", ["rate", "last"])
def test_query_is_scan_then_present(fdb, engine, mm_dataset, func):
    ds, start = mm_dataset
    nb, ng = 8, 4
    fid = fdb.FN_HIST_RATE if func == "rate" else fdb.FN_LAST
    tops = model.geometric_tops(2.0, 2.0, nb)
    for pid, p0, p1 in ((fdb.HP_QUANTILE, 0.9, 0.0),
                        (fdb.HP_QUANTILE_MINMAX, 0.99, 0.0),
                        (fdb.HP_MAX_QUANTILE, 0.99, 0.0),
                        (fdb.HP_BUCKET, tops[3], 0.0),
                        (fdb.HP_FRACTION, 3.0, 40.0),
                        (fdb.HP_FRACTION_MINMAX, 3.0, 40.0)):
        q = fdb.make_query(start, 15000, start + 70 * 15000, 120000, fid,
                           fdb.AGG_SUM, ng, param=p0, param2=p1)
        n = ng * q.num_windows
        s1, c1, x1, n1 = np.zeros(n * nb), np.zeros(n), np.zeros(n), np.zeros(n)
        got = engine.query_hist_present(ds, q, nb, pid, out_bucket_sums=s1,
                                        out_counts=c1, out_max=x1, out_min=n1)
        s2, c2, x2, n2 = np.zeros(n * nb), np.zeros(n), np.zeros(n), np.zeros(n)
        engine.query_hist_mm(ds, q, nb, out_bucket_sums=s2, out_counts=c2,
                             out_max=x2, out_min=n2)
        want = present(fdb, engine, pid, s2, c2, nb, 2.0, 2.0, p0=p0, p1=p1,
                       maxs=x2, mins=n2)
        for a, b in ((s1, s2), (c1, c2), (x1, x2), (n1, n2), (got, want)):
            assert a.tobytes() == b.tobytes(), (func, pid)
        assert (c1 == 0).any() and np.isnan(got[c1 == 0]).all()
        assert np.isfinite(got[c1 > 0]).mean() > 0.5
        # the grids are optional
        alone = engine.query_hist_present(ds, q, nb, pid)
        assert alone.tobytes() == got.tobytes(), (func, pid)


def test_quantile_mode_is_out_quantile(fdb, engine, mm_dataset):
    ds, start = mm_dataset
    nb, ng = 8, 4
    for q0 in (0.5, 0.99, 0.0, 1.0, -0.1, 1.1):
        q = fdb.make_query(start, 15000, start + 70 * 15000, 120000,
                           fdb.FN_HIST_RATE, fdb.AGG_SUM, ng, param=q0)
        n = ng * q.num_windows
        s, c, quant = np.zeros(n * nb), np.zeros(n), np.zeros(n)
        engine.query_hist(ds, q, nb, out_bucket_sums=s, out_counts=c,
                          out_quantile=quant)
        got = present(fdb, engine, fdb.HP_QUANTILE, s, c, nb, 2.0, 2.0, p0=q0)
        assert got.tobytes() == quant.tobytes(), q0
        assert (c > 0).any() and (c == 0).any()


@pytest.mark.parametrize("func", ["rate", "last"])
def test_max_and_min_outputs_are_independent(fdb, engine, mm_dataset, func):
    """out_min alone, out_max alone and both give the same grids"""
    ds, start = mm_dataset
    nb, ng = 8, 4
    fid = fdb.FN_HIST_RATE if func == "rate" else fdb.FN_LAST
    q = fdb.make_query(start, 15000, start + 70 * 15000, 120000, fid,
                       fdb.AGG_SUM, ng)
    n = ng * q.num_windows

    def run(want_max, want_min):
        s, c = np.zeros(n * nb), np.zeros(n)
        mx = np.zeros(n) if want_max else None
        mn = np.zeros(n) if want_min else None
        engine.query_hist_mm(ds, q, nb, out_bucket_sums=s, out_counts=c,
                             out_max=mx, out_min=mn)
        return s, c, mx, mn

    s0, c0, mx0, mn0 = run(True, True)
    assert np.isfinite(mx0).any() and np.isfinite(mn0).any()
    assert np.isnan(mx0).any() and np.isnan(mn0).any()    # the empty windows
    s1, c1, _, mn1 = run(False, True)
    s2, c2, mx2, _ = run(True, False)
    assert mn1.tobytes() == mn0.tobytes()
    assert mx2.tobytes() == mx0.tobytes()
    for s, c in ((s1, c1), (s2, c2)):
        assert s.tobytes() == s0.tobytes() and c.tobytes() == c0.tobytes()


def test_scheme_comes_from_the_dataset(fdb, engine):
    """a 0.5/1.5 scheme: out_quantile presents over the uploaded store's own
    bucket tops (every other store here is 2.0/2.0)"""
    rng = np.random.default_rng(17)
    nb, first, mult = 8, 0.5, 1.5
    st = fdb.ChunkStore()
    t0 = None
    for g in range(2):
        ts, cum = synth_hist(rng, 30, nb=nb)
        t0 = int(ts[0]) if t0 is None else t0
        st.append_hist(st.add_series(g, fdb.COL_HIST), ts, cum, first=first,
                       mult=mult)
    st.seal()
    ds = engine.upload(st)
    start = t0 - 45000                       # the first windows are empty
    q = fdb.make_query(start, 15000, start + 25 * 15000, 120000,
                       fdb.FN_HIST_RATE, fdb.AGG_SUM, 2, param=0.9)
    n = 2 * q.num_windows
    s, c, quant = np.zeros(n * nb), np.zeros(n), np.zeros(n)
    engine.query_hist(ds, q, nb, out_bucket_sums=s, out_counts=c,
                      out_quantile=quant)
    want = present(fdb, engine, fdb.HP_QUANTILE, s, c, nb, first, mult, p0=0.9)
    assert quant.tobytes() == want.tobytes()
    assert (c == 0).any() and np.isnan(quant[c == 0]).all()
    assert np.isfinite(quant[c > 0]).mean() > 0.5
    other = present(fdb, engine, fdb.HP_QUANTILE, s, c, nb, 2.0, 2.0, p0=0.9)
    assert other.tobytes() != quant.tobytes()
