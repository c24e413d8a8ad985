"""The fast scan's lean rate epilogue and seed early-out against the oracle
(real MI355X).

The fast kernel's extrapolatedRate epilogue (rate_core.h, LEAN) takes avgDur
through a reciprocal table when numSamples-1 < 256 and the window is at most
2^26 ms, and branches around the v1/delta division when v1 >= delta and
durationToStart <= sampledInterval; the shared window search skips its seed
search for a series that begins after window -1 ends. Each is meant to leave
every output bit as it was, so wherever the build before this change equalled
the oracle exactly (==, NaN positions included) this file asserts exactly
that: every AGG_NONE case below, for rate, increase and delta, and `sum by
group` where the sum's order cannot matter or is fixed (EXACT_SUM). Elsewhere
`sum by group` adds a group's series in another order than the oracle does —
a reduction tree in the two-phase path, atomicAdd arrival order (not
reproducible from run to run with three or more series in a group) in the
FDB_FUSED_GROUP=1 path; there the build before the change was only within
tests/test_gpu_parity.py's tolerance of the oracle, and that tolerance (rtol
1e-9, atol 1e-12) is kept. Recorded from this file run on that build: all 42
AGG_NONE comparisons equal; two-phase sums equal on linear, pairs, dense1s and
span27 (at most three series per group) and not on poisson0, poisson1e9,
resets and seed; fused sums equal on linear (at most two series per group: a
commutative sum) and, for delta on dense1s[0] and span27[0], equal in one run
and not in the next, so those are arrival-order coincidences and stay on the
tolerance.

Stores are single-chunk, at most 64 series each:
  poisson0    counters from 0, Poisson(10), 240 rows at 15 s +- 300 ms, [5m]
              step 15 s from the first sample: lanes that skip the division
              and lanes that do not share a wave (v1 < delta early on)
  poisson1e9  the same plus 1e9: every lane skips
  linear      v = 10(i+1) on an exact 15 s grid: v1 == delta at s+1 == e-s,
              and its neighbours on both sides
  pairs       two samples 1 s apart every 290 s: durationToStart >
              sampledInterval, the skip's other condition fails
  dense1s     400 rows at 1 s, windows of 300 s and 400 s at steps that put
              numSamples-1 above and below 256 within one wave
  span27      400 rows over about 2^27 ms, windows of exactly 2^26 ms (table)
              and 2^26 + 15 000 ms (plain division)
  resets      5 % resets and 5 % NaN rows
  seed        first samples at qstart - qstep + {-1, 0, +1}, at qstart and
              mid-range, interleaved: the waves of one block take both seed
              branches
"""
from types import SimpleNamespace

import numpy as np
import pytest

import window_cases as wc
from conftest import build_store

pytestmark = pytest.mark.gpu

T0 = 10_000_000
STEP = 15000
FUNCS = {"rate": 0, "increase": 1, "delta": 2}
NGROUPS = 3
# sum-by-group cases (store, FDB_FUSED_GROUP) that equalled the oracle on the
# build before this change, reproducibly (module docstring): asserted with ==;
# every other sum-by-group case keeps test_gpu_parity's tolerance
EXACT_SUM = {("linear", "0"), ("linear", "1"), ("pairs", "0"), ("dense1s", "0"),
             ("span27", "0")}


def _jitter_grid(rng, n, start=T0):
    ts = start + np.arange(n) * STEP + rng.integers(-300, 301, n)
    ts[0] = start
    return np.maximum.accumulate(ts)


def _series(name):
    """list of (ts, vals) per series of store `name`"""
    rng = np.random.default_rng(600 + sorted(SHAPES).index(name))
    out = []
    if name in ("poisson0", "poisson1e9"):
        for _ in range(24):
            ts = _jitter_grid(rng, 240)
            vals = np.cumsum(rng.poisson(10.0, 240).astype(np.float64))
            vals -= vals[0]                              # counters start at 0
            out.append((ts, vals + (1e9 if name == "poisson1e9" else 0.0)))
    elif name == "linear":
        for n in (240, 239, 64, 22):
            out.append((T0 + np.arange(n) * STEP, 10.0 * (np.arange(n) + 1)))
    elif name == "pairs":
        for _ in range(8):
            base = T0 + np.repeat(np.arange(60) * 290_000, 2)
            base[1::2] += 1000
            vals = np.cumsum(rng.poisson(10.0, 120).astype(np.float64))
            out.append((base, vals))
    elif name == "dense1s":
        for k in range(8):
            ts = T0 + np.arange(400) * 1000
            vals = np.cumsum(rng.poisson(10.0, 400).astype(np.float64))
            out.append((ts, vals + (0.0 if k % 2 else 1e6)))
    elif name == "span27":
        gap = (1 << 27) // 400
        for k in range(8):
            ts = T0 + np.arange(400) * gap + rng.integers(-300, 301, 400)
            ts[0] = T0
            vals = np.cumsum(rng.poisson(10.0, 400).astype(np.float64))
            out.append((np.maximum.accumulate(ts), vals + (0.0 if k % 2 else 1e6)))
    elif name == "resets":
        for _ in range(24):
            ts = _jitter_grid(rng, 240)
            vals = np.cumsum(rng.poisson(10.0, 240).astype(np.float64))
            for i in np.nonzero(rng.random(240) < 0.05)[0]:
                vals[i:] -= vals[i]
            vals[rng.random(240) < 0.05] = np.nan
            out.append((ts, vals))
    elif name == "seed":
        firsts = [T0 - STEP - 1, T0 - STEP, T0 - STEP + 1, T0, T0 + 100 * STEP + 7,
                  T0 - 30 * STEP]
        for i in range(36):
            n = 240 - 7 * (i % 5)
            ts = _jitter_grid(rng, n, start=firsts[i % len(firsts)])
            out.append((ts, np.cumsum(rng.poisson(10.0, n).astype(np.float64))))
    return out


# store -> list of (start offset from T0, step, num_windows, window)
SHAPES = {
    "poisson0": [(0, STEP, 241, 300_000)],
    "poisson1e9": [(0, STEP, 241, 300_000)],
    "linear": [(0, STEP, 241, 300_000), (0, STEP, 241, 70_000)],
    "pairs": [(0, STEP, 241, 300_000), (0, 290_000, 60, 300_000)],
    # k = numSamples-1 grows by step/1 s per window up to the window length:
    # 400 s / 8 s shares (m = 50), k crosses 256 at window 32 (slot 0);
    # 400 s / 3 s does not share, crosses at window 86 (slot 1); 300 s / 5 s
    # shares (m = 60), crosses at window 52 and stays at 300 from window 60
    "dense1s": [(0, 8000, 60, 400_000), (0, 3000, 150, 400_000),
                (0, 5000, 90, 300_000)],
    "span27": [(0, 1 << 21, 70, 1 << 26), (0, 1 << 21, 70, (1 << 26) + 15000)],
    "resets": [(0, STEP, 241, 300_000)],
    "seed": [(0, STEP, 241, 300_000), (0, STEP, 300, 900_000)],
}
CASES = [(name, i) for name in SHAPES for i in range(len(SHAPES[name]))]


@pytest.fixture(scope="module")
def engine(fdb):
    return fdb.Engine(0)


@pytest.fixture(scope="module")
def stores(fdb, engine):
    def make(name):
        series = _series(name)
        assert 0 < len(series) <= 64
        st = build_store(
            fdb, [[[(int(t), float(v)) for t, v in zip(ts, vals)]]
                  for ts, vals in series],
            kind=fdb.COL_COUNTER, groups=[i % NGROUPS for i in range(len(series))])
        return SimpleNamespace(store=st, ds=engine.upload(st))
    return wc.case_cache(make)


@pytest.mark.parametrize("name,shape", CASES)
def test_rate_epilogue_vs_oracle(fdb, oracle, engine, stores, monkeypatch, name, shape):
    case = stores(name)
    off, step, nw, window = SHAPES[name][shape]
    start = T0 + off
    end = start + (nw - 1) * step
    for fname, func in FUNCS.items():
        q = fdb.make_query(start, step, end, window, func)
        assert q.num_windows == nw
        got, want = wc.run_both(oracle, engine, case, q)
        assert np.isfinite(want).sum() > 0, "the case computes nothing"
        print(f"{name}[{shape}] {fname} none: equal={np.array_equal(got, want, equal_nan=True)}")
        wc.assert_exact(got, want)

        qs = fdb.make_query(start, step, end, window, func, fdb.AGG_SUM, NGROUPS)
        want = wc.run_oracle(oracle, case, qs)
        for fused in ("0", "1"):
            monkeypatch.setenv("FDB_FUSED_GROUP", fused)
            got = wc.run_engine(engine, case, qs)
            print(f"{name}[{shape}] {fname} sum fused={fused}: "
                  f"equal={np.array_equal(got, want, equal_nan=True)}")
            if (name, fused) in EXACT_SUM:
                wc.assert_exact(got, want)
            else:
                wc.assert_close(got, want)
