"""Independent CPU model of the reference's four instant range functions
(irate, idelta, resets, deriv) — a plain helper module, not a conftest.

The CPU oracle under oracle/ does not know these functions, so parity for them
rests on this file. It is a LITERAL restatement of the reference's sliding
path, deliberately not the closed forms the kernels use:

  * SlidingWindowIterator.next            PeriodicSamplesMapper.scala:404-455
    (inclusive-range=true: a row joins when ts >= wStart, the head leaves
    when ts < wStart), driving add/remove callbacks on a queue
  * BufferableCounterCorrectionIterator   PeriodicSamplesMapper.scala:551-574
  * instantValue(isRate)                  RangeInstantFunctions.scala:68-95
  * ResetsFunction (add/remove state)     RangeInstantFunctions.scala:352-384
  * derivFunction / linearRegression      RangeInstantFunctions.scala:10-18,45-66
    (sequential summation order)

closed_form() restates the issue's per-window definitions (what the kernels
compute); tests/test_instant_model.py proves the two agree on the data domain
the GPU tests use.
"""
import math
from collections import deque

import numpy as np

IRATE, IDELTA, RESETS, DERIV = "irate", "idelta", "resets", "deriv"
NAN = float("nan")


class Row:
    __slots__ = ("timestamp", "value")

    def __init__(self, timestamp, value):
        self.timestamp = int(timestamp)
        self.value = float(value)


class Window:
    """QueueBasedWindow over the iterator's queue."""

    def __init__(self):
        self.q = deque()

    @property
    def size(self):
        return len(self.q)

    def __call__(self, i):
        return self.q[i]

    @property
    def head(self):
        return self.q[0]

    @property
    def last(self):
        return self.q[-1]


def raw_rows(ts, vals):
    for t, v in zip(ts, vals):
        yield Row(t, v)


def counter_corrected_rows(ts, vals):
    """BufferableCounterCorrectionIterator: NaN -> 0 (explicit reset); a drop
    adds the previous value to a running correction."""
    correction = 0.0
    prev_val = 0.0
    for t, v in zip(ts, vals):
        next_val = float(v)
        if math.isnan(next_val):
            next_val = 0.0
        if next_val < prev_val:
            correction += prev_val
        yield Row(t, next_val + correction)
        prev_val = next_val


def instant_value(start_ts, end_ts, window, is_rate):
    if window.size < 2:
        return NAN
    assert window.head.timestamp >= start_ts
    assert window.last.timestamp <= end_ts
    last_sample = window.last.value
    prev_row = window(window.size - 2)
    result = last_sample - prev_row.value
    if is_rate and last_sample < prev_row.value:
        result = last_sample
    if is_rate:
        sampled_interval = float(window.last.timestamp - prev_row.timestamp)
        if sampled_interval == 0:
            return NAN
        result = result / sampled_interval * 1000
    return result


def linear_regression_slope(window, intercept_time):
    n = 0.0
    sum_x = sum_y = sum_xy = sum_x2 = 0.0
    for i in range(window.size):
        sample = window(i)
        x = float(sample.timestamp - intercept_time) / 1000.0
        n += 1.0
        sum_y += sample.value
        sum_x += x
        sum_xy += x * sample.value
        sum_x2 += x * x
    cov_xy = sum_xy - sum_x * sum_y / n
    var_x = sum_x2 - sum_x * sum_x / n
    # JVM double division: x/0 is +-inf or NaN, never an exception
    return float(np.float64(cov_xy) / np.float64(var_x))


class IRateFunction:
    needs_counter_correction = True

    def added(self, row, window):
        pass

    def removed(self, row, window):
        pass

    def apply(self, start_ts, end_ts, window):
        return instant_value(start_ts, end_ts, window, True)


class IDeltaFunction:
    needs_counter_correction = False

    def added(self, row, window):
        pass

    def removed(self, row, window):
        pass

    def apply(self, start_ts, end_ts, window):
        return instant_value(start_ts, end_ts, window, False)


class ResetsFunction:
    needs_counter_correction = False

    def __init__(self):
        self.resets = NAN  # NaN for windows that do not have data

    def added(self, row, window):
        size = window.size
        if math.isnan(self.resets) and size > 0:
            self.resets = 0.0
        if size > 1:
            prev_value = window(size - 2).value
            curr_value = row.value
            if (not math.isnan(curr_value) and not math.isnan(prev_value)
                    and curr_value < prev_value):
                self.resets += 1

    def removed(self, row, window):
        if window.size > 0:
            removed_value = row.value
            next_value = window.head.value
            if (not math.isnan(removed_value) and not math.isnan(next_value)
                    and removed_value > next_value):
                self.resets -= 1
        else:
            self.resets = NAN

    def apply(self, start_ts, end_ts, window):
        return self.resets


class DerivFunction:
    needs_counter_correction = False

    def added(self, row, window):
        pass

    def removed(self, row, window):
        pass

    def apply(self, start_ts, end_ts, window):
        if window.size < 2:
            return NAN
        return linear_regression_slope(window, window(0).timestamp)


FUNCTIONS = {IRATE: IRateFunction, IDELTA: IDeltaFunction,
             RESETS: ResetsFunction, DERIV: DerivFunction}


def sliding(ts, vals, start, step, end, window_ms, func):
    """One series through SlidingWindowIterator with range function `func`
    (a name from FUNCTIONS). Returns one value per window end in
    start, start+step, ..., <= end."""
    fn = FUNCTIONS[func]()
    src = counter_corrected_rows if fn.needs_counter_correction else raw_rows
    rows = src(ts, vals)
    nxt = next(rows, None)               # the buffered iterator's head
    window = Window()
    out = []
    cur_end = start
    with np.errstate(all="ignore"):
        while cur_end <= end:
            cur_start = cur_end - window_ms
            while nxt is not None and nxt.timestamp <= cur_end:
                cur = nxt
                nxt = next(rows, None)
                if cur.timestamp >= cur_start:        # shouldAddCurToWindow
                    window.q.append(cur)
                    fn.added(cur, window)
            while window.size and window.head.timestamp < cur_start:
                removed = window.q.popleft()          # shouldRemoveWindowHead
                fn.removed(removed, window)
            out.append(fn.apply(cur_start, cur_end, window))
            cur_end += step
    return np.array(out, dtype=np.float64)


def grid(series, start, step, end, window_ms, func):
    """series: list of (ts, vals). Returns the flat [S x W] grid."""
    return np.concatenate([sliding(t, v, start, step, end, window_ms, func)
                           for t, v in series])


# ---------------------------------------------------------------------------
# the per-window definitions the kernels implement, for the model-vs-closed-
# form check (and the pairwise-summation variant of deriv, to bound what a
# tree-order sum may differ from the sequential reference)
# ---------------------------------------------------------------------------
def _pairwise(a):
    a = list(a)
    if not a:
        return 0.0
    while len(a) > 1:
        a = [a[i] + a[i + 1] if i + 1 < len(a) else a[i]
             for i in range(0, len(a), 2)]
    return a[0]


def closed_form(ts, vals, start, step, end, window_ms, func, pairwise=False):
    ts = np.asarray(ts, dtype=np.int64)
    vals = np.asarray(vals, dtype=np.float64)
    out = []
    w_end = start
    with np.errstate(all="ignore"):
        while w_end <= end:
            s = int(np.searchsorted(ts, w_end - window_ms, side="left"))
            e = int(np.searchsorted(ts, w_end, side="right")) - 1
            n = e - s + 1
            res = NAN
            if func == IRATE:
                if n >= 2:
                    last = 0.0 if math.isnan(vals[e]) else float(vals[e])
                    prev = 0.0 if math.isnan(vals[e - 1]) else float(vals[e - 1])
                    d = last if last < prev else last - prev
                    dt = float(ts[e] - ts[e - 1])
                    res = NAN if dt == 0 else d / dt * 1000
            elif func == IDELTA:
                if n >= 2:
                    res = float(vals[e]) - float(vals[e - 1])
            elif func == RESETS:
                if n > 0:
                    v = vals[s:e + 1]
                    a, b = v[:-1], v[1:]
                    res = float(np.sum(~np.isnan(a) & ~np.isnan(b) & (b < a)))
            else:
                if n >= 2:
                    x = [float(t - ts[s]) / 1000.0 for t in ts[s:e + 1]]
                    y = [float(q) for q in vals[s:e + 1]]
                    add = _pairwise if pairwise else _seq
                    sx, sy = add(x), add(y)
                    sxy = add([p * q for p, q in zip(x, y)])
                    sx2 = add([p * p for p in x])
                    cov = sxy - sx * sy / n
                    var = sx2 - sx * sx / n
                    res = float(np.float64(cov) / np.float64(var))
            out.append(res)
            w_end += step
    return np.array(out, dtype=np.float64)


def _seq(a):
    s = 0.0
    for x in a:
        s += x
    return s
