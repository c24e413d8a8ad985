"""The counter-reset table and its overflow ("dense") path, in both kernels.

One scan step (csrc/window_funcs.h: d_reset_scan_step) fills the sparse
(position, cumulative correction) table of the fast kernel (capacity 32, one
400-row chunk per series) and of the chunk summaries behind the stream walk
(capacity 8 per chunk); a chunk with more resets than its table holds is
"dense" and every lookup recomputes serially (d_corr_at). Random data at
reset_p <= 0.05 essentially never overflows a table, so the series here place
resets at chosen rows, and the host asserts each chunk's reset count before
anything runs.

rate and increase against the CPU oracle at the project's bar
(test_gpu_parity.run_both / check); irate, which ignores the table, is the
control, bit-exact against tests/instant_model.py.
"""
import numpy as np
import pytest

import instant_model as im
from test_gpu_instant_funcs import Case, STEP, T0, env, mk_ts, run, run_general
from test_gpu_parity import check, run_both

pytestmark = pytest.mark.gpu

RATE, INCREASE, IRATE = 0, 1, 21
WINDOW_STEPS = (5, 20)


@pytest.fixture(scope="module")
def engine(fdb):
    return fdb.Engine(0)


def mk_series(rng, n, resets_at, nan_at=()):
    """Integral counter that drops exactly at rows `resets_at`: increments are
    >= 1000 and a reset halves the previous value, so runs of consecutive
    resets still drop (up to ten in a row)."""
    vals = np.empty(n)
    vals[0] = float(rng.integers(1000, 2000))
    resets = set(resets_at)
    for i in range(1, n):
        if i in resets:
            vals[i] = float(int(vals[i - 1]) // 2)
        else:
            vals[i] = vals[i - 1] + float(rng.integers(1000, 2000))
    for i in nan_at:
        vals[i] = np.nan
    return mk_ts(rng, n), vals


def resets_per_chunk(vals, sizes):
    """What the device scan counts: per chunk, rows below their predecessor
    with NaN read as 0 (a chunk's first row has no predecessor)."""
    x = np.nan_to_num(vals, nan=0.0)
    out, i = [], 0
    for c in sizes:
        out.append(int(np.sum(x[i + 1:i + c] < x[i:i + c - 1])))
        i += c
    return tuple(out)


def pick(rng, lo, hi, k):
    return sorted(rng.choice(np.arange(lo, hi), k, replace=False).tolist())


def build(fdb, oracle, engine, specs):
    """specs: (sizes, resets_at, nan_at, claimed per-chunk reset counts)."""
    rng = np.random.default_rng(77)
    series, sizes = [], []
    for sz, resets_at, nan_at, claim in specs:
        ts, vals = mk_series(rng, sum(sz), resets_at, nan_at)
        assert resets_per_chunk(vals, sz) == claim, (resets_per_chunk(vals, sz), claim)
        series.append((ts, vals))
        sizes.append(sz)
    return Case(fdb, oracle, engine, series, sizes, fdb.COL_COUNTER)


@pytest.fixture(scope="module")
def single(fdb, oracle, engine):
    """One 400-row chunk per series: the fast kernel, table capacity 32."""
    rng = np.random.default_rng(5)
    edge = (63, 64, 65, 127, 128)       # both sides of the 64-row scan passes
    return build(fdb, oracle, engine, [
        ((400,), (), (), (0,)),
        ((400,), pick(rng, 1, 400, 32), (), (32,)),      # a full table
        ((400,), pick(rng, 1, 400, 33), (), (33,)),      # the first dense chunk
        ((400,), pick(rng, 1, 400, 120), (), (120,)),
        ((400,), edge, (), (5,)),
        # NaN at row 64 reads as 0: still a reset there, none possible at 65
        ((400,), edge, (64,), (4,)),
    ])


@pytest.fixture(scope="module")
def multi(fdb, oracle, engine):
    """Three 130-row chunks per series: summaries + walk, table capacity 8."""
    rng = np.random.default_rng(6)
    sz = (130, 130, 130)
    mid8 = [5, 50] + pick(rng, 131, 260, 8) + [300]
    mid9 = [5, 50] + pick(rng, 131, 260, 9) + [300]
    # a dense FIRST chunk: windows that start in chunk 2 carry its chunk_corr
    # through meta_corr
    first9 = pick(rng, 1, 130, 9) + [200, 300]
    # drops exactly on each later chunk's first row: cross-chunk, in no table
    heads = [130, 260]
    return build(fdb, oracle, engine, [
        (sz, mid8, (), (2, 8, 1)),
        (sz, mid9, (), (2, 9, 1)),
        (sz, first9, (), (9, 1, 1)),
        (sz, heads, (), (0, 0, 0)),
    ])


def query_args(case, wsteps):
    """Windows slide in from before the data and run off its end."""
    rows = max(len(ts) for ts, _ in case.series)
    return T0 - 3 * STEP, STEP, rows + wsteps + 6, wsteps * STEP


def against_oracle(fdb, oracle, engine, case, func, wsteps):
    start, step, nw, window = query_args(case, wsteps)
    q = fdb.make_query(start, step, start + (nw - 1) * step, window, func)
    assert q.num_windows == nw
    got, want = run_both(fdb, oracle, engine, case.store, q)
    assert np.isfinite(want).any() and np.isnan(want).any()
    check(got, want)


def irate_model(case, wsteps):
    start, step, nw, window = query_args(case, wsteps)
    return im.grid(case.series, start, step, start + (nw - 1) * step, window,
                   im.IRATE)


@pytest.mark.parametrize("wsteps", WINDOW_STEPS)
@pytest.mark.parametrize("func", [RATE, INCREASE])
def test_single_chunk_fast(fdb, oracle, engine, single, func, wsteps):
    against_oracle(fdb, oracle, engine, single, func, wsteps)


@pytest.mark.parametrize("wsteps", WINDOW_STEPS)
@pytest.mark.parametrize("func", [RATE, INCREASE])
def test_single_chunk_walk(fdb, oracle, engine, single, func, wsteps):
    """The same store through summaries + walk (capacity 8: the chunks with
    32, 33 and 120 resets are all dense there)."""
    with env("FDB_FAST", "0"):
        against_oracle(fdb, oracle, engine, single, func, wsteps)


@pytest.mark.parametrize("wsteps", WINDOW_STEPS)
@pytest.mark.parametrize("func", [RATE, INCREASE])
def test_multi_chunk_walk(fdb, oracle, engine, multi, func, wsteps):
    against_oracle(fdb, oracle, engine, multi, func, wsteps)


@pytest.mark.parametrize("wsteps", WINDOW_STEPS)
def test_irate_control(fdb, engine, single, multi, wsteps):
    for case in (single, multi):
        want = irate_model(case, wsteps)
        args = query_args(case, wsteps)
        np.testing.assert_array_equal(
            run(fdb, engine, case.ds, len(case.series), *args, IRATE), want)
        np.testing.assert_array_equal(
            run_general(fdb, engine, case, *args, IRATE), want)
