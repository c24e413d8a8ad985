"""What the GPU tests of the fast scan's window rows share
(test_gpu_window_bounds.py, test_gpu_window_share.py,
test_gpu_aligned_bounds.py; test_gpu_rate_epilogue.py and
test_gpu_fast_desc.py take the cache and the run helpers): the counter value
law, the two families of timestamp laws, the store-per-class Case, and the
engine / oracle run and comparison helpers. Each test file keeps its class
list, seeds, shapes and test bodies. The order of draws from the generator is
part of every law: the stores must not change."""
import numpy as np

from conftest import build_store


def counter_values(rng, n, resets):
    """Cumulative Poisson(10) counter; `resets`: 5 % of the rows restart it."""
    vals = np.cumsum(rng.poisson(10.0, n).astype(np.float64))
    if resets:
        for i in np.nonzero(rng.random(n) < 0.05)[0]:
            vals[i:] -= vals[i]
    return vals


# ---- family one: scrape laws, rebased so that row 0 is at `origin` ---------
def scrape(rng, n, step, drop, jitter=300):
    grid = np.arange(int(n / (1 - drop)) + 64)
    if drop > 0:
        grid = grid[rng.random(grid.size) >= drop]
    grid = grid[:n]
    assert grid.size == n
    return grid * step + rng.integers(-jitter, jitter + 1, n)


def scrape_ts(cls, rng, n, origin, step, off_edges=False):
    """off_edges puts every row at 5 (mod 10) from the origin: off every
    window edge of queries whose edges are = 0 or 2 (mod 10)."""
    if cls == "bench":
        t = scrape(rng, n, step, 0.0)
    elif cls == "grid":                     # rows exactly on wEnd and wStart
        t = np.arange(n) * step
    elif cls.startswith("drop"):
        t = scrape(rng, n, step, int(cls[4:]) / 100.0)
    elif cls == "geometric":                # gaps double, restart every 21 rows
        gaps = 1 << (np.arange(n) % 21)
        t = np.concatenate([[0], np.cumsum(gaps)[:-1]])
    elif cls == "clusters":                 # two dense clusters, one 2^30 gap
        gaps = rng.integers(900, 1101, n)
        if n >= 2:
            gaps[n // 2 - 1] = 1 << 30
        t = np.concatenate([[0], np.cumsum(gaps)[:-1]])
    elif cls == "allequal":
        t = np.zeros(n, dtype=np.int64)
    elif cls == "dupruns":                  # runs of 1..5 equal rows
        runs = rng.integers(1, 6, n)
        base = np.cumsum(step + rng.integers(-300, 301, n))
        t = np.repeat(base, runs)[:n]
    else:
        raise KeyError(cls)
    t = np.maximum.accumulate(np.asarray(t, dtype=np.int64))
    t = origin + t - t[0]
    if off_edges:
        t = t // 10 * 10 + 5
    return t


# ---- family two: laws around a scrape grid whose point 0 is `origin` -------
def pinned_jitter(rng, n, amp):
    """+-amp ms, with row 0 and the last row on the line and row 1 a full amp
    off it: the builder stores a vector whose rows all lie within 250 ms of
    that line as a const one, rounding every row onto the line, and the
    engine and the oracle do not agree on such a chunk's last millisecond."""
    j = rng.integers(-amp, amp + 1, n)
    j[0] = j[-1] = 0
    if n >= 3:
        j[1] = amp
    return j


def aligned_ts(cls, rng, n, origin, step):
    i = np.arange(n, dtype=np.int64)
    if cls == "bench":
        t = i * step + pinned_jitter(rng, n, 300)
    elif cls == "constjit":                 # stored as a const vector
        t = i * step + rng.integers(-100, 101, n)
    elif cls == "zerojitter":               # every row exactly on a window edge
        t = i * step
    elif cls.startswith("drift"):           # scrape interval q-1, q+1, q-5, q+5
        d = {"m1": -1, "p1": 1, "m5": -5, "p5": 5}[cls[5:]]
        t = i * (step + d) + (pinned_jitter(rng, n, 300) if abs(d) == 1 else 0)
    elif cls == "dups":
        t = i * step + rng.integers(-50, 51, n)
        for k in range(1, n - 2, 3):        # rows 0 and n-1 stay on the grid
            t[k] = k * step + step * 11 // 20
            t[k + 1] = t[k]
    elif cls == "drop":                     # one scrape missing in the middle
        t = (i + (i > n // 2)) * step + pinned_jitter(rng, n, 300)
    elif cls == "10s":                      # interval is not the step
        t = i * 10_000 + pinned_jitter(rng, n, 300)
    else:
        raise KeyError(cls)
    return origin + np.maximum.accumulate(t)


# ---- stores ----------------------------------------------------------------
class Case:
    """One single-chunk counter store, uploaded: for every size, one series
    per (law, resets) of `plan`, timestamps from ts_law(law, rng, n), groups
    0..2 in turn. The default plan is the class with and without resets (the
    rate path with and without drops)."""

    def __init__(self, fdb, engine, cls, sizes, seed, ts_law, plan=None):
        rng = np.random.default_rng(seed)
        series, groups = [], []
        for n in sizes:
            for law, resets in plan or ((cls, False), (cls, True)):
                ts = ts_law(law, rng, n)
                vals = counter_values(rng, n, resets)
                series.append([[(int(t), float(v)) for t, v in zip(ts, vals)]])
                groups.append(len(series) % 3)
        self.max_ts = max(ch[0][-1][0] for ch in series)
        self.store = build_store(fdb, series, kind=fdb.COL_COUNTER, groups=groups)
        self.ds = engine.upload(self.store)


def case_cache(make):
    """get(name) -> make(name), made once."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = make(name)
        return cache[name]
    return get


# ---- running and comparing ---------------------------------------------------
# a case is anything with .store (sealed) and .ds (its upload)
def run_oracle(oracle, case, q):
    return oracle.query_exec(case.store.view(), q, case.store.num_series,
                             q.num_windows, nthreads=4)


def run_engine(engine, case, q):
    rows = q.num_groups if q.agg_id else case.store.num_series
    got = np.empty(rows * q.num_windows, dtype=np.float64)
    engine.query(case.ds, q, out=got)
    return got


def run_both(oracle, engine, case, q):
    want = run_oracle(oracle, case, q)
    return run_engine(engine, case, q), want


def assert_exact(got, want, what=""):
    np.testing.assert_array_equal(got, want, err_msg=what)


def assert_close(got, want, what=""):
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12, equal_nan=True,
                               err_msg=what)
