// Per-window rules of the range functions, each written once for every kernel
// that applies it (scan_fast, scan_stream, window_sample, hist2). Only rules
// with the same floating-point operation sequence at every site live here.
// Deliberately NOT shared: the fast kernel's AVG/STDDEV/STDVAR through its
// reciprocal table (<= 2 ulp) against the walk's plain divisions, and K_PFX's
// prefix differences.
#ifndef FDB_WINDOW_FUNCS_H
#define FDB_WINDOW_FUNCS_H

#include "scan_common.h"
#include "rate_core.h"   // d_div1000, d_extrapolate_core

// i64 timestamps (the walk, hist2). The /1000 sites use d_div1000 —
// bit-identical on the engine's ms-difference domain.
__device__ inline double d_extrapolated_rate(
    int64_t windowStart, int64_t windowEnd, int numSamples, int64_t t1, double v1,
    int64_t t2, double v2, bool isCounter, bool isRate) {
  double scaledDelta = d_extrapolate_core(
      d_div1000((double)(t1 - windowStart)), d_div1000((double)(windowEnd - t2)),
      d_div1000((double)(t2 - t1)), numSamples, v1, v2, isCounter);
  return isRate ? (scaledDelta / (double)(windowEnd - windowStart) * 1000.0) : scaledDelta;
}

// i32-difference variant for the fast path: all three millisecond gaps fit
// i32 when the window does (caller checks), so each i64 subtract +
// 4-instruction i64→f64 convert becomes a truncate + single v_cvt_f64_i32; the
// window duration is wave-uniform and passed pre-converted. Same values into
// the same core, so results are bit-identical to d_extrapolated_rate. LEAN
// selects the core's lean form (rate_core.h: same bits, two divisions fewer
// where provable) with the reciprocal table rk[0..rk_lim).
template <bool LEAN = false>
__device__ inline double d_extrapolated_rate_i32(
    int32_t toStart_ms, int32_t toEnd_ms, int numSamples, int32_t sampled_ms,
    double dur_ms, double v1, double v2, bool isCounter, bool isRate,
    const double* rk = nullptr, int rk_lim = 0) {
  double scaledDelta = d_extrapolate_core<LEAN>(
      d_div1000((double)toStart_ms), d_div1000((double)toEnd_ms),
      d_div1000((double)sampled_ms), numSamples, v1, v2, isCounter, rk, rk_lim);
  return isRate ? (scaledDelta / dur_ms * 1000.0) : scaledDelta;
}

// --- counter correction (CorrectingDoubleVectorReader :305-392) -------------
// One chunk's resets become a sparse table of (position, cumulative
// correction); a chunk with more than CAP resets is "dense": its table is
// void and lookups recompute serially.
struct ResetScan {
  int count = 0;            // table entries (meaningless once dense)
  bool dense = false;
  double carry_corr = 0;    // correction total of the rows scanned so far
  double carry_x = -1.7976931348623157e308;   // previous pass's last value
};

// one 64-row pass of the reset scan (:325-342): x is lane's row i with NaN→0
// like the reference (0 when !live); every lane of the wave calls this
template <int CAP>
__device__ __forceinline__ void d_reset_scan_step(
    ResetScan& st, int i, bool live, double x, int lane, int16_t* dpos, double* dcum) {
  double px = __shfl_up(x, 1);
  if (lane == 0) px = st.carry_x;
  double ci = (live && x < px) ? px : 0;
  double scan = wave_incl_scan(ci, lane);
  uint64_t mask = __ballot(ci != 0);
  int here = __popcll(mask);
  if (here) {
    if (st.count + here > CAP) {
      st.dense = true;
    } else if (ci != 0) {
      int slot = st.count + __popcll(mask & ((1ULL << lane) - 1));
      dpos[slot] = (int16_t)i;
      dcum[slot] = st.carry_corr + scan;
    }
    if (!st.dense) st.count += here;
  }
  st.carry_corr += __shfl(scan, 63);
  st.carry_x = __shfl(x, 63);
}

// in-chunk correction at row i (the step function the reference materializes
// as corrected[]): the table walk, or for a dense chunk the serial recompute
// over row_at(j), the chunk's raw rows
template <typename RowAt>
__device__ __forceinline__ double d_corr_at(
    const int16_t* dpos, const double* dcum, int count, bool dense, int i, RowAt row_at) {
  if (dense) {      // rare
    double corr = 0, last = -1.7976931348623157e308;
    for (int j = 0; j <= i; j++) {
      double x = row_at(j);
      if (isnan(x)) x = 0;
      if (x < last) corr += last;
      last = x;
    }
    return corr;
  }
  double c = 0;
  for (int j = 0; j < count; j++) {
    if (dpos[j] <= i) c = dcum[j]; else break;
  }
  return c;
}

// --- folds and predicates ---------------------------------------------------
// adjacent pair (px, x) counts for changes (x != px) or resets (x < px,
// ResetsFunction RangeInstantFunctions.scala:352-375; DoubleVectorDataReader64
// .changes :283-302); a NaN on either side never counts
template <bool IS_RESETS>
__device__ __forceinline__ bool d_pair_counts(double x, double px) {
  return !isnan(x) && !isnan(px) && (IS_RESETS ? x < px : x != px);
}

// NaN-ignoring min/max fold (acc stays NaN until a non-NaN x arrives)
template <bool IS_MIN>
__device__ __forceinline__ void d_fold_mm(double& acc, double x) {
  if (!isnan(x) && (isnan(acc) || (IS_MIN ? x < acc : x > acc))) acc = x;
}

// NaN-skipping sum / sum of squares / count of rows s..e; the sums stay NaN
// until the first non-NaN row, like the reference's per-range accumulators
template <typename RowAt>
__device__ __forceinline__ void d_range_moments(RowAt row_at, int s, int e,
                                                double& sum, double& sq, int& cnt) {
  sum = NAN; sq = NAN; cnt = 0;
  for (int i = s; i <= e; i++) {
    double x = row_at(i);
    if (isnan(x)) continue;
    if (isnan(sum)) { sum = 0; sq = 0; }
    sum += x; sq += x * x; cnt++;
  }
}

// acc += x across ranges: the first non-NaN addend starts a NaN acc at 0, a
// NaN addend (a range without samples) poisons it — the reference's quirk
__device__ __forceinline__ void d_poison_add(double& acc, double x) {
  if (!isnan(x) && isnan(acc)) acc = 0;
  acc += x;
}

// --- finishers ---------------------------------------------------------------
// stdvar/stddev from NaN-zeroed totals (VarOverTimeChunkedFunctionD
// AggrOverTimeFunctions.scala:1082-1115); not the fast kernel's, which
// multiply by its reciprocal table instead
__device__ __forceinline__ double d_var_finish(double sum, double sqsum, int n,
                                               bool is_stddev) {
  if (n <= 0) return isnan(sum) ? sum : 0;
  double avg = sum / n;
  double r = sqsum / n - avg * avg;
  return is_stddev ? sqrt(r) : r;
}

// z_score_over_time (AggrOverTimeFunctions.scala:1592-1603); last = the
// window's last row when it is not NaN
__device__ __forceinline__ double d_zscore_finish(double sum, double sqsum, int n,
                                                  double last) {
  if (n <= 0) return isnan(sum) ? sum : 0;
  return (last - sum / n) / d_var_finish(sum, sqsum, n, true);
}

// irate: instantValue(isRate=true), RangeInstantFunctions.scala:68-95, over
// counter-corrected rows (BufferableCounterCorrectionIterator: NaN -> 0, a
// drop adds the previous value to a running correction); the correction
// common to both rows cancels, leaving last on a drop and last - prev
// otherwise. One divide, then one multiply.
__device__ __forceinline__ double d_irate_finish(double last, double prev,
                                                 double dt_ms) {
  if (isnan(last)) last = 0;
  if (isnan(prev)) prev = 0;
  const double d = (last < prev) ? last : last - prev;
  return (dt_ms == 0) ? NAN : d / dt_ms * 1000.0;
}

// present_over_time's sample at a range's end row e with raw value v
// (LastSampleChunkedFunction, RangeFunction.scala:599-614): a NaN looks back
// one row inside its chunk. False when the row decides nothing (NaN at row 0).
template <typename RowAt>
__device__ __forceinline__ bool d_present_at(double v, int e, RowAt row_at,
                                             double* out) {
  if (!isnan(v)) { *out = 1.0; return true; }
  if (e > 0) { *out = isnan(row_at(e - 1)) ? NAN : 1.0; return true; }
  return false;
}

// --- per-chunk walk preamble (WindowedChunkIterator, ChunkSetInfo.scala:445-529)
// drop rule: a chunk that ends before the window starts is skipped
__device__ __forceinline__ bool d_chunk_before_window(int64_t cend, int64_t wStart) {
  return cend < wStart;
}
// add-while rule: the chunk that reaches the window's end is the last one
__device__ __forceinline__ bool d_chunk_ends_walk(int64_t cend, int64_t wEnd) {
  return cend >= wEnd;
}

struct ChunkRows { DVec tv, vv; int64_t ts0; int n, startRow, endRow; };

// opens both vectors of `chunk` and finds window [wStart, wEnd]'s row range
// (startRow > endRow: none). The chunk's first timestamp is *ts0_known, or
// parsed from the timestamp vector's header when that is null. inv_slope(n,
// ts0) is d_search_ge's guess slope, evaluated per search: a window usually
// needs neither search or only one.
template <typename Slope>
__device__ __forceinline__ ChunkRows d_chunk_rows(
    const uint8_t* blob, const DirSoA& dir, int chunk, int64_t wStart,
    int64_t wEnd, const int64_t* ts0_known, int64_t ts_last, Slope inv_slope) {
  ChunkRows r;
  d_vec_open_wide(blob + dir.ts_off[chunk], &r.tv, ts0_known ? nullptr : &r.ts0);
  d_vec_open_wide(blob + dir.val_off[chunk], &r.vv, nullptr);
  if (ts0_known) r.ts0 = *ts0_known;
  r.n = dir.num_rows[chunk];
  r.startRow = (wStart <= r.ts0) ? 0
      : d_search_ge(r.tv, r.n, wStart, r.ts0, inv_slope(r.n, r.ts0));
  r.endRow = (wEnd >= ts_last) ? r.n - 1
      : d_search_ge(r.tv, r.n, wEnd + 1, r.ts0, inv_slope(r.n, r.ts0)) - 1;
  return r;
}

#endif  // FDB_WINDOW_FUNCS_H
