// extrapolatedRate's floating-point core, written once for every kernel that
// applies it (window_funcs.h wraps it for the i64 and i32 timestamp forms).
//
// Compiles as device code under hipcc and as plain host C++ (no HIP runtime
// needed) — tools/verify_rate_epilogue.cpp checks the lean form against the
// plain one bit for bit. Build host users with -ffp-contract=off, like the
// library: the rule's products and sums are rounded one by one.
#ifndef FDB_RATE_CORE_H
#define FDB_RATE_CORE_H

#ifdef __HIPCC__
#define FDB_RC_FN __host__ __device__ __forceinline__
#else
#define FDB_RC_FN inline
#endif

// Correctly-rounded x/1000 in 3 ops (mul + 2 fma, Markstein fixup) instead of
// the ~10-instruction v_div_scale/v_div_fmas/v_div_fixup sequence. EXACTLY
// equal to RN(x/1000) for every integer |x| <= 2^33 — verified exhaustively
// (8.59e9 cases, 0 mismatches; the naive q0 = x*(1/1000) alone differs on 13%
// of them). Callers pass integer millisecond DIFFERENCES bounded by the
// window length; the engine rejects windows > 2^33 ms (~99 days) up front.
FDB_RC_FN double d_div1000(double x) {
  constexpr double r = 1.0 / 1000.0;                // RN reciprocal
  double q0 = x * r;
  double e = __builtin_fma(-1000.0, q0, x);         // exact residual
  return __builtin_fma(e, r, q0);
}

// The lean core's reciprocal table: rk[k] = RN(1/k) for k < FDB_RATE_RTAB
// ([0] = +inf, never a divisor: a window has at least two samples). 256
// entries are what the fast rate kernel's LDS budget allows at 7 blocks/CU
// (scan_fast.hip); a 5-minute window at a 15 s scrape needs k <= 20.
#define FDB_RATE_RTAB 256
// largest window (ms) whose gaps the table quotient is verified for
#define FDB_RATE_RTAB_MAX_MS ((long long)1 << 26)

// si/k by the same construction as d_div1000, rk = RN(1/k). EXACTLY equal to
// RN(si/k) for every si = d_div1000(ms), integer ms in 1..2^26, and every
// integer k in 1..255 — verified exhaustively by tools/verify_rate_epilogue
// (1.7e10 cases, 0 mismatches). Outside that domain callers divide.
FDB_RC_FN double d_div_small_int(double si, double k, double rk) {
  double q0 = si * rk;
  double e = __builtin_fma(-k, q0, si);
  return __builtin_fma(e, rk, q0);
}

// extrapolatedRate (RateFunctions.scala:72-111) from the three durations in
// seconds to scaledDelta — the oracle's EXACT operation sequence. Do not
// reassociate or replace the divisions: the durationToZero/threshold
// comparisons are discontinuous and integer counter data makes exact rational
// ties (v1/delta == 1.1/(numSamples-1)) common, so the branch taken must
// follow the reference's own FP rounding.
//
// LEAN (the fast rate kernel's i32 path) returns the same bits with two of the
// four divisions gone where they can be proved away; it is this one rule with
// two shortcuts, not a second rule:
//  * avgDur through rk[] when numSamples-1 < rk_lim (d_div_small_int; the
//    caller passes rk_lim = 0 unless the window is <= FDB_RATE_RTAB_MAX_MS,
//    and sampledInterval = d_div1000 of an integer ms gap)
//  * durationToZero = sampledInterval * (v1/delta) only matters when it is
//    smaller than durationToStart. With v1 >= delta > 0 the exact quotient is
//    >= 1, so RN(v1/delta) >= RN(1) = 1 (round-to-nearest is monotone; +inf
//    for a subnormal delta included), and then RN(sampledInterval * q) >=
//    RN(sampledInterval * 1) = sampledInterval >= durationToStart: the
//    comparison is false whatever the quotient is, and the divide, the
//    multiply and the compare are skipped. NaN cannot reach the test: delta >
//    0 && v1 >= 0 gates it. A counter at least as large as its increase over
//    the window is the normal case for long-lived counters, so whole waves
//    branch around the divide.
template <bool LEAN = false>
FDB_RC_FN double d_extrapolate_core(
    double durationToStart, double durationToEnd, double sampledInterval,
    int numSamples, double v1, double v2, bool isCounter,
    const double* rk = nullptr, int rk_lim = 0) {
  const double k = (double)numSamples - 1;
  double avgDur;
  if (LEAN && numSamples - 1 < rk_lim)
    avgDur = d_div_small_int(sampledInterval, k, rk[numSamples - 1]);
  else
    avgDur = sampledInterval / k;
  double delta = v2 - v1;
  if (isCounter && delta > 0 && v1 >= 0) {
    if (!(LEAN && v1 >= delta && durationToStart <= sampledInterval)) {
      double durationToZero = sampledInterval * (v1 / delta);
      if (durationToZero < durationToStart) durationToStart = durationToZero;
    }
  }
  double thresh = avgDur * 1.1;
  double ext = sampledInterval;
  ext += (durationToStart < thresh) ? durationToStart : avgDur / 2;
  ext += (durationToEnd < thresh) ? durationToEnd : avgDur / 2;
  return delta * (ext / sampledInterval);
}

#endif  // FDB_RATE_CORE_H
