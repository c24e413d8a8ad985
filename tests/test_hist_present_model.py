"""The histogram present model (tests/hist_funcs_model.py) against the
reference's own literals (tests/golden/hist_present.json, transcribed from
HistogramTest.scala) and the edge rules of Histogram.scala:65-197 and
InstantFunction.scala:433-453. CPU only: the GPU presenter is then held to the
model in tests/test_gpu_hist_present.py."""
import json
import math
import os

import pytest

import hist_funcs_model as model

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "hist_present.json")
INF = float("inf")
NAN = float("nan")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def num(x):
    """golden number: "inf" stands for +Infinity"""
    return float(x)


def within(got, expected, tol):
    return got == expected if tol == 0 else abs(got - expected) <= tol


def test_fraction_custom_goldens():
    g = load_golden()["fraction_custom"]
    tops = [num(t) for t in g["tops"]]
    vals = [float(v) for v in g["values"]]
    assert len(g["cases"]) == 6
    for c in g["cases"]:
        lo, up = num(c["lower"]), num(c["upper"])
        if c["min"] is None:
            got = model.fraction(tops, vals, lo, up)
        else:
            got = model.fraction(tops, vals, lo, up, num(c["min"]), num(c["max"]))
        assert within(got, c["expected"], c["tol"]), (c, got)


def test_quantile_minmax_goldens():
    g = load_golden()["quantile_minmax"]
    assert len(g["cases"]) == 4
    for c in g["cases"]:
        tops = model.geometric_tops(g["first"], g["mult"], len(c["values"]))
        got = model.quantile(tops, [float(v) for v in c["values"]], c["q"],
                             num(c["min"]), num(c["max"]))
        assert within(got, c["expected"], c["tol"]), (c, got)
        # the clip matters: the unclipped quantile misses the literal
        plain = model.quantile(tops, [float(v) for v in c["values"]], c["q"])
        assert not within(plain, c["expected"], c["tol"]), (c, plain)


def test_quantile50_goldens():
    g = load_golden()["quantile50"]
    assert len(g["cases"]) == 4
    for c in g["cases"]:
        tops = model.geometric_tops(g["first"], g["mult"], len(c["values"]))
        got = model.quantile(tops, [float(v) for v in c["values"]], g["q"])
        assert got == c["expected"], (c, got)


def test_quantile_matches_oracle(oracle):
    """the model's plain quantile is the oracle's hist_quantile"""
    import numpy as np
    rng = np.random.default_rng(12)
    for _ in range(50):
        nb = int(rng.integers(2, 20))
        v = np.cumsum(rng.integers(0, 9, nb)).astype(np.float64)
        q = float(rng.random())
        want = oracle.hist_quantile(q, v, 2.0, 2.0)
        got = model.quantile(model.geometric_tops(2.0, 2.0, nb), v, q)
        assert got == pytest.approx(want, rel=1e-12, nan_ok=True)


TOPS8 = model.geometric_tops(1.0, 2.0, 8)
VALS8 = [10.0, 15, 17, 20, 25, 34, 76, 82]


def test_fraction_edges():
    assert model.fraction(TOPS8, VALS8, 5.0, 5.0) == 0.0          # lower >= upper
    assert model.fraction(TOPS8, VALS8, 9.0, 3.0) == 0.0
    assert model.fraction(TOPS8, VALS8, 0.0, 0.0) == VALS8[0] / VALS8[-1]
    assert math.isnan(model.fraction(TOPS8, [0.0] * 8, 1.0, 4.0))  # top == 0
    assert math.isnan(model.fraction(TOPS8, [0.0] * 8, 0.0, 0.0))
    # bucket boundaries need no interpolation
    assert model.fraction(TOPS8, VALS8, 2.0, 16.0) == (25 - 15) / 82
    # beyond the last top both ranks clamp to the count
    assert model.fraction(TOPS8, VALS8, 200.0, 300.0) == 0.0
    for lo, up in ((-1.0, 2.0), (1.0, -2.0), (NAN, 2.0), (1.0, NAN)):
        with pytest.raises(ValueError):
            model.fraction(TOPS8, VALS8, lo, up)
    # Math.max/min propagate a NaN companion value into the interpolation
    assert math.isnan(model.fraction(TOPS8, VALS8, 3.0, 5.0, NAN, NAN))
    # ... but not when both ends sit on bucket boundaries
    assert model.fraction(TOPS8, VALS8, 2.0, 16.0, NAN, NAN) == (25 - 15) / 82


def test_quantile_edges():
    assert model.quantile(TOPS8, VALS8, -0.1) == -INF
    assert model.quantile(TOPS8, VALS8, 1.1) == INF
    assert math.isnan(model.quantile(TOPS8, [0.0] * 8, 0.5))       # top <= 0
    assert math.isnan(model.quantile(TOPS8[:1], VALS8[:1], 0.5))   # < 2 buckets
    # a NaN max/min compares false and clips nothing
    plain = model.quantile(TOPS8, VALS8, 0.95)
    assert model.quantile(TOPS8, VALS8, 0.95, NAN, NAN) == plain
    assert model.quantile(TOPS8, VALS8, 0.95, 0.0, NAN) == plain
    # max outside (bucketStart, bucketEnd] clips nothing either
    assert model.quantile(TOPS8, VALS8, 0.95, 0.0, 64.0) == plain
    assert model.quantile(TOPS8, VALS8, 0.95, 0.0, 500.0) == plain
    assert model.quantile(TOPS8, VALS8, 0.95, 0.0, 90.0) < plain


def test_bucket_edges():
    assert model.bucket(TOPS8, VALS8, 4.0) == 17.0
    assert model.bucket(TOPS8, VALS8, 4.0 + 5e-11) == 17.0
    assert math.isnan(model.bucket(TOPS8, VALS8, 3.0))             # not a bucket
    assert math.isnan(model.bucket(TOPS8, VALS8, 4.0 + 1e-9))
    with pytest.raises(ValueError):
        model.bucket(TOPS8, VALS8, INF)
    assert model.bucket(TOPS8[:7] + [INF], VALS8, INF) == 82.0


def test_present_dispatch():
    assert model.present(0, TOPS8, VALS8, 0.95) == model.quantile(TOPS8, VALS8, 0.95)
    assert model.present(1, TOPS8, VALS8, 0.95, mx=100.0, mn=10.0) == \
        model.quantile(TOPS8, VALS8, 0.95, 10.0, 100.0)
    assert model.present(2, TOPS8, VALS8, 0.95, mx=90.0, mn=70.0) == \
        model.quantile(TOPS8, VALS8, 0.95, 0.0, 90.0)
    assert model.present(3, TOPS8, VALS8, 8.0) == 20.0
    assert model.present(4, TOPS8, VALS8, 3.0, 5.0) == model.fraction(TOPS8, VALS8, 3.0, 5.0)
    assert model.present(5, TOPS8, VALS8, 3.0, 5.0, mx=4.5, mn=3.5) == \
        model.fraction(TOPS8, VALS8, 3.0, 5.0, 3.5, 4.5)
