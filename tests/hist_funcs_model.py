"""Independent numpy model of the histogram functions the CPU oracle does not
know — a plain helper module, not a conftest.

Window functions, over decoded chunks (a list of (ts, raw[, corr]) per series,
in time order; ts the STORED timestamps, raw the decoded bucket rows):

  * last_sample_window   LastSampleChunkedFunctionH / ...HMax.addChunks
                         (RangeFunction.scala:595-682), chunk by chunk: the
                         latest row with ts <= wEnd wins when ts >= wStart
  * increase_window      HistIncreaseFunction (RateFunctions.scala:415-418):
                         the per-window correction walk of
                         tests/test_hist.py's naive_hist_rate_window, ending in
                         extrapolatedRate with isRate = false

Present rules, over an ARBITRARY array of bucket tops (so the reference's
custom-bucket literals pin them too), linear interpolation only:

  * quantile             Histogram.quantile(q, min, max)   Histogram.scala:65-108
  * fraction             Histogram.histogramFraction       Histogram.scala:119-197
  * bucket               HistogramBucketImpl               InstantFunction.scala:433-453

An empty histogram (no contributing series) is the caller's rule: NaN.
"""
import math

import numpy as np

NAN = float("nan")
INF = float("inf")


# ---------------------------------------------------------------------------
# window functions
# ---------------------------------------------------------------------------
def last_sample_window(chunks, w_start, w_end):
    """Returns (chunk index, row) of the last sample in [w_start, w_end], or
    None. chunks[i][0] is the chunk's timestamp array."""
    timestamp = -1
    hit = None
    for ci, ch in enumerate(chunks):
        ts = ch[0]
        # ceilingIndex(endTime): last row with ts <= endTime, -1 when none
        end_row = min(int(np.searchsorted(ts, w_end, side="right")) - 1,
                      len(ts) - 1)
        if end_row >= 0:
            t = int(ts[end_row])
            if t >= w_start and t > timestamp:
                timestamp = t
                hit = (ci, end_row)
    return hit


def _lex_less(a, b):
    """Histogram.compare with equal schemes (Histogram.scala:204-214): top
    bucket down, first difference."""
    for i in range(len(a) - 1, -1, -1):
        if a[i] != b[i]:
            return a[i] < b[i]
    return False


def increase_window(oracle, chunks, w_start, w_end, nb):
    """chunks: list of (ts, raw [n×nb], corr [n×nb]) with corr the in-chunk
    TypeDrop corrections. Returns the per-bucket increase or None for a window
    without two samples at distinct times."""
    carry = np.zeros(nb)
    lastv = None
    samples = 0
    low_t = hi_t = None
    lo = hi = None
    for ts, raw, corr in chunks:
        if int(ts[-1]) < w_start:
            continue
        s = int(np.searchsorted(ts, w_start, side="left"))
        e = min(int(np.searchsorted(ts, w_end, side="right")) - 1, len(ts) - 1)
        if lastv is not None and _lex_less(raw[0], lastv):
            carry = carry + lastv          # drop across the chunk seam
        if s <= e:
            if low_t is None or ts[s] < low_t or ts[e] > hi_t:
                samples += e - s + 1
                if low_t is None or ts[s] < low_t:
                    low_t = int(ts[s])
                    lo = raw[s] + corr[s] + carry
                if hi_t is None or ts[e] > hi_t:
                    hi_t = int(ts[e])
                    hi = raw[e] + corr[e] + carry
        carry = carry + corr[-1]
        lastv = raw[-1]
        if int(ts[-1]) >= w_end:
            break
    if low_t is None or hi_t is None or not hi_t > low_t:
        return None
    return np.array([oracle.extrapolated_rate(int(w_start), int(w_end), samples,
                                              low_t, float(lo[b]),
                                              hi_t, float(hi[b]), True, False)
                     for b in range(nb)])


# ---------------------------------------------------------------------------
# present rules
# ---------------------------------------------------------------------------
def _jmax(a, b):
    """java.lang.Math.max: NaN if either argument is NaN."""
    return NAN if (math.isnan(a) or math.isnan(b)) else max(a, b)


def _jmin(a, b):
    return NAN if (math.isnan(a) or math.isnan(b)) else min(a, b)


def _div(a, b):
    """IEEE double division (numpy scalars: x/0 is inf or NaN, no exception)."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def geometric_tops(first, mult, nb):
    return [first * mult ** b for b in range(nb)]


def quantile(tops, v, q, mn=0.0, mx=INF):
    nb = len(tops)
    top = float(v[nb - 1]) if nb > 0 else NAN
    if q < 0:
        return -INF
    if q > 1:
        return INF
    if nb < 2 or top <= 0:
        return NAN
    rank = q * top
    bucket = 0
    while v[bucket] < rank:       # firstBucketGTE; rank <= top ends it
        bucket += 1
    start = 0.0 if bucket == 0 else tops[bucket - 1]
    end = tops[bucket]
    if mn > start and mn <= end:
        start = mn
    if mx > start and mx <= end:
        end = mx
    if bucket == nb - 1 and end == INF:
        return tops[nb - 2]
    if bucket == 0 and tops[0] <= 0:
        return tops[0]
    count = v[0] if bucket == 0 else v[bucket] - v[bucket - 1]
    rank -= 0 if bucket == 0 else v[bucket - 1]
    return start + (end - start) * _div(rank, count)


def fraction(tops, v, lower, upper, mn=-INF, mx=INF):
    if not (lower >= 0 and upper >= 0):
        raise ValueError(f"lower & upper params should be >= 0: "
                         f"lower={lower}, upper={upper}")
    nb = len(tops)
    if nb == 0 or v[nb - 1] == 0:
        return NAN
    count = float(v[nb - 1])
    if lower == 0 and upper == 0:
        return _div(v[0], count)
    if lower >= upper:
        return 0.0
    lower_rank = upper_rank = 0.0
    lower_set = upper_set = False
    for b in range(nb):
        if lower_set and upper_set:
            break
        b_upper = tops[b]
        b_lower = 0.0 if b == 0 else tops[b - 1]
        val = float(v[b])
        prev = 0.0 if b == 0 else float(v[b - 1])

        def interpolate(x):
            low = _jmax(b_lower, mn)
            high = _jmin(b_upper, mx)
            return prev + (val - prev) * _div(x - low, high - low)

        if not lower_set and b_lower == lower:
            lower_rank, lower_set = prev, True
        if not upper_set and b_upper == upper:
            upper_rank, upper_set = val, True
        if not lower_set and b_lower < lower and b_upper > lower:
            lower_rank, lower_set = interpolate(lower), True
        if not upper_set and b_lower < upper and b_upper > upper:
            upper_rank, upper_set = interpolate(upper), True
    if not lower_set or lower_rank > count:
        lower_rank = count
    if not upper_set or upper_rank > count:
        upper_rank = count
    return _div(upper_rank - lower_rank, count)


def bucket(tops, v, le):
    if le == INF:
        if tops[-1] == INF:
            return float(v[len(tops) - 1])
        raise ValueError("+Inf bucket not in the last position!")
    for b in range(len(tops)):
        if abs(tops[b] - le) <= 1e-10:
            return float(v[b])
    return NAN


# FDB_HP_* ids -> the rule over one cell (v, max, min)
def present(present_id, tops, v, p0, p1=0.0, mx=NAN, mn=NAN):
    if present_id == 0:
        return quantile(tops, v, p0)
    if present_id == 1:
        return quantile(tops, v, p0, mn, mx)
    if present_id == 2:
        return quantile(tops, v, p0, 0.0, mx)
    if present_id == 3:
        return bucket(tops, v, p0)
    if present_id == 4:
        return fraction(tops, v, p0, p1)
    if present_id == 5:
        return fraction(tops, v, p0, p1, mn, mx)
    raise ValueError(present_id)
