// Streaming general path: multi-chunk series with NO capacity caps.
//
// Round 1 kept whole series LDS-resident (two tiers, capped at 1600 rows /
// 16 chunks — a 24h@15s lookback could not run). Round 2 replaces both tiers:
//
//  * summary_kernel (once per dataset upload, one wave per chunk): decodes
//    each chunk into LDS and reduces it to a 192-B ChunkSum — totals
//    (sum/sumsq/count/min/max/interior-changes/interior-resets), boundary values, the
//    counter-correction pieces (in-chunk correction total, sparse reset
//    table, updateCorrection operand), and the interpolation-search slope.
//    Query-independent, amortized across queries.
//  * stream_walk_kernel (per query): one wave per series, lanes split the
//    windows; each window walks its overlapping chunks exactly like the
//    reference's WindowedChunkIterator + addChunks chain
//    (ChunkSetInfo.scala:445-529, RangeFunction.scala:131-198), taking FULL
//    middle chunks from their summaries in O(1) and decoding only the two
//    boundary ranges directly from the packed vectors in global memory
//    (L1/L2-served — the walk revisits the same small chunks across windows).
//
// Per-window semantics are the round-1 general path's (parity-green against
// the oracle): the NaN-poison sum quirk, the single-row-NaN chunk skip for
// counters, the correction meta chain, LastSample/present/timestamp rules.
// Unbounded: rows per series, chunks per series, window/step ratio and
// num_windows. Per-chunk rows stay <= 400 (the reference's own chunk cap,
// filodb-defaults.conf:835).

#include <cstring>
#include <cmath>

#include "engine_internal.h"

#define SUM_DROPS 8          // sparse per-chunk counter-reset table capacity

struct ChunkSum {            // 192 B per chunk, in a device-resident array
  int64_t ts0, ts_last;      // decoded first/last timestamps
  double sum, sqsum;         // NaN-zeroed totals
  double first_val, last_val;   // RAW val[0], val[n-1]
  double vmin, vmax;         // NaN-ignoring (NaN when all-NaN)
  double chunk_corr;         // CorrectingDoubleVectorReader total correction
  double last_for_update;    // updateCorrection operand (DoubleVector.scala:375-391)
  double dcum[SUM_DROPS];    // cumulative correction at/after dpos[j]
  int16_t dpos[SUM_DROPS];   // reset positions (ascending)
  int32_t cnt;               // non-NaN count
  int32_t changes_in;        // interior value changes (NaN-aware)
  float   inv_slope;         // (n-1)/(ts_last-ts0); 0 when degenerate
  uint8_t v0_nan, dropped, dense, ndrops;
  int32_t resets_in;         // interior resets: x < px, both non-NaN
  int32_t _pad[2];
};
static_assert(sizeof(ChunkSum) == 192, "ChunkSum layout");

// ---------------------------------------------------------------------------
// summary kernel: one wave per chunk
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256)
void summary_kernel(const uint8_t* __restrict__ blob, DirSoA dir,
                    int64_t num_chunks, ChunkSum* __restrict__ out) {
  __shared__ int64_t ts_all[4][FDB_DEFAULT_MAX_ROWS];
  __shared__ double val_all[4][FDB_DEFAULT_MAX_ROWS];
  __shared__ int16_t dpos_all[4][SUM_DROPS];
  __shared__ double dcum_all[4][SUM_DROPS];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  int64_t* ts = ts_all[wave];
  double* val = val_all[wave];

  for (int64_t c = blockIdx.x * 4 + wave; c < num_chunks; c += gridDim.x * 4) {
    DVec tv, vv;
    d_vec_open_wide(blob + dir.ts_off[c], &tv, nullptr);
    d_vec_open_wide(blob + dir.val_off[c], &vv, nullptr);
    int n = dir.num_rows[c];
    if (n > FDB_DEFAULT_MAX_ROWS || n > tv.n) n = 0;
    if (n > 0) {
      d_decode_chunk<false>(tv, n, ts, nullptr, lane);
      d_decode_chunk<true>(vv, n, nullptr, val, lane);
    }
    d_lds_fence();

    ChunkSum s;
    memset(&s, 0, sizeof(s));
    s.vmin = NAN; s.vmax = NAN; s.first_val = NAN; s.last_val = NAN;
    if (n > 0) {
      double sum = 0, sq = 0, mn = NAN, mx = NAN;
      int cnt = 0, changes = 0, resets = 0;
      double carry_raw = NAN;                 // previous row's raw value
      ResetScan rs;
      const bool dropped = vv.dropped != 0;
      double last_nonnan = 0;                 // last_for_update when dropped
      int last_nonnan_idx = -1;
      for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool live = i < n;
        double raw = live ? val[i] : NAN;
        bool ok = live && !isnan(raw);
        double x = ok ? raw : 0;
        sum += x;                              // lane partials; reduced below
        sq += x * x;
        cnt += ok ? 1 : 0;
        d_fold_mm<true>(mn, raw);              // raw is NaN past the chunk
        d_fold_mm<false>(mx, raw);
        // interior changes and resets (raw is NaN past the chunk)
        double px = __shfl_up(raw, 1);
        if (lane == 0) px = carry_raw;
        changes += (i > 0 && d_pair_counts<false>(raw, px)) ? 1 : 0;
        resets += (i > 0 && d_pair_counts<true>(raw, px)) ? 1 : 0;
        carry_raw = __shfl(raw, 63);
        // counter-reset scan; table slots published through LDS so lane 0
        // can emit them
        if (dropped) {
          d_reset_scan_step<SUM_DROPS>(rs, i, live, x, lane,
                                       dpos_all[wave], dcum_all[wave]);
          if (ok) { last_nonnan_idx = i; last_nonnan = raw; }
        }
      }
      for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off);
        sq += __shfl_down(sq, off);
        cnt += __shfl_down(cnt, off);
        changes += __shfl_down(changes, off);
        resets += __shfl_down(resets, off);
        d_fold_mm<true>(mn, __shfl_down(mn, off));
        d_fold_mm<false>(mx, __shfl_down(mx, off));
        int oi = __shfl_down(last_nonnan_idx, off);
        double ov = __shfl_down(last_nonnan, off);
        if (oi > last_nonnan_idx) { last_nonnan_idx = oi; last_nonnan = ov; }
      }
      d_lds_fence();
      s.ts0 = ts[0];
      s.ts_last = ts[n - 1];
      s.sum = sum; s.sqsum = sq; s.cnt = cnt; s.changes_in = changes;
      s.resets_in = resets;
      s.vmin = mn; s.vmax = mx;
      s.first_val = val[0];
      s.last_val = val[n - 1];
      s.v0_nan = isnan(val[0]) ? 1 : 0;
      s.dropped = dropped ? 1 : 0;
      s.dense = rs.dense ? 1 : 0;
      s.ndrops = (uint8_t)(rs.dense ? 0 : rs.count);
      s.chunk_corr = rs.carry_corr;
      s.last_for_update = dropped ? (last_nonnan_idx >= 0 ? last_nonnan : 0)
                                  : val[n - 1];
      s.inv_slope = (s.ts_last > s.ts0)
                        ? (float)(n - 1) / (float)(s.ts_last - s.ts0) : 0.0f;
      if (!rs.dense) {
        for (int j = 0; j < rs.count; j++) {
          s.dpos[j] = dpos_all[wave][j];
          s.dcum[j] = dcum_all[wave][j];
        }
      }
    }
    if (lane == 0) out[c] = s;
    d_lds_fence();
  }
}

// ---------------------------------------------------------------------------
// global-memory row access for the walk kernel's boundary ranges
// ---------------------------------------------------------------------------
// in-chunk corrected value at row: raw NaN→0 plus the chunk's correction
__device__ double g_corrected(const DVec& vv, const ChunkSum& cs, int row) {
  double x = d_dv_at(&vv, row);
  if (!cs.dropped) return x;
  if (isnan(x)) x = 0;
  return x + d_corr_at(cs.dpos, cs.dcum, cs.ndrops, cs.dense, row,
                       [&](int j) { return d_dv_at(&vv, j); });
}

// one chunk's row range for a window, searched with its summary's endpoints
__device__ __forceinline__ ChunkRows walk_rows(const uint8_t* blob, const DirSoA& dir,
                                               const ChunkSum& cs, int chunk,
                                               int64_t wStart, int64_t wEnd) {
  return d_chunk_rows(blob, dir, chunk, wStart, wEnd, &cs.ts0, cs.ts_last,
                      [&](int, int64_t) { return cs.inv_slope; });
}

// ---------------------------------------------------------------------------
// the walk kernel: one wave per series, lanes split windows; per (window,
// chunk): summaries for full chunks, direct decode for boundary ranges
// ---------------------------------------------------------------------------
template <int FUNC>
__global__ __launch_bounds__(256)
void stream_walk_kernel(const uint8_t* __restrict__ blob, DirSoA dir,
                        const ChunkSum* __restrict__ sums,
                        const int32_t* __restrict__ series_first,
                        const int32_t* __restrict__ series_nchunks,
                        int num_series,
                        int64_t qstart, int64_t qstep, int64_t qend,
                        int64_t qwindow, int num_windows,
                        double* __restrict__ out) {
  constexpr bool RATE_FAMILY = (FUNC <= FN_DELTA);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;

  for (int sid = blockIdx.x * 4 + wave; sid < num_series;
       sid += gridDim.x * 4) {
    const int first = series_first[sid];
    const int nchunks = series_nchunks[sid];

    for (int w = lane; w < num_windows; w += 64) {
      const int64_t wEnd = qstart + (int64_t)w * qstep;
      const int64_t wStart = wEnd - qwindow;
      double result = NAN;

      if constexpr (RATE_FAMILY) {
        bool meta_has = false;
        double meta_last = 0, meta_corr = 0;
        int numSamples = 0;
        int64_t lowestTime = INT64_MAX, highestTime = 0;
        double lowestValue = NAN, highestValue = NAN;
        constexpr bool isCounter = (FUNC != FN_DELTA);
        for (int c = 0; c < nchunks; c++) {
          const int64_t cend = dir.end_time[first + c];
          if (d_chunk_before_window(cend, wStart)) continue;
          const ChunkSum& cs = sums[first + c];
          const ChunkRows r = walk_rows(blob, dir, cs, first + c, wStart, wEnd);
          const DVec &tv = r.tv, &vv = r.vv;
          const int n = r.n, startRow = r.startRow, endRow = r.endRow;
          if (isCounter && meta_has) {        // detectDropAndCorrection
            double firstv = cs.first_val;
            if (isnan(firstv) || firstv < meta_last) meta_corr += meta_last;
          }
          if (startRow <= endRow && endRow < n) {
            bool skip = isCounter && startRow == 0 && endRow == 0 && cs.v0_nan;
            if (!skip) {
              int64_t st = (startRow == 0) ? cs.ts0 : d_lv_at(&tv, startRow);
              int64_t en = (endRow == n - 1) ? cs.ts_last : d_lv_at(&tv, endRow);
              if (st < lowestTime || en > highestTime) {
                numSamples += endRow - startRow + 1;
                if (st < lowestTime) {
                  lowestTime = st;
                  lowestValue = isCounter
                      ? g_corrected(vv, cs, startRow) + meta_corr
                      : d_dv_at(&vv, startRow);
                }
                if (en > highestTime) {
                  highestTime = en;
                  highestValue = isCounter
                      ? g_corrected(vv, cs, endRow) + meta_corr
                      : d_dv_at(&vv, endRow);
                }
              }
            }
          }
          if (isCounter) {                    // updateCorrection
            if (cs.dropped) meta_corr += cs.chunk_corr;
            meta_last = cs.last_for_update;
            meta_has = true;
          }
          if (d_chunk_ends_walk(cend, wEnd)) break;
        }
        if (highestTime > lowestTime)
          result = d_extrapolated_rate(wStart, wEnd, numSamples,
                                       lowestTime, lowestValue,
                                       highestTime, highestValue,
                                       isCounter, FUNC == FN_RATE);
      } else {
        double sum = NAN, sqsum = NAN, mm = NAN;
        double changes = NAN, prev = NAN;
        double last_val = NAN, last_sample = NAN;
        int64_t last_ts = -1, prev_ts = -1;
        int icount = 0;
        for (int c = 0; c < nchunks; c++) {
          const int64_t cend = dir.end_time[first + c];
          if (d_chunk_before_window(cend, wStart)) continue;
          const ChunkSum& cs = sums[first + c];
          const ChunkRows r = walk_rows(blob, dir, cs, first + c, wStart, wEnd);
          const DVec &tv = r.tv, &vv = r.vv;
          const int n = r.n, startRow = r.startRow, endRow = r.endRow;

          if constexpr (FUNC == FN_LAST || FUNC == FN_PRESENT) {
            // LastSampleChunkedFunction.addChunks (RangeFunction.scala:599-614)
            if (endRow >= 0 && endRow < n) {
              int64_t t = (endRow == n - 1) ? cs.ts_last : d_lv_at(&tv, endRow);
              if (t >= wStart && t > last_ts) {
                double v = d_dv_at(&vv, endRow);
                if (FUNC == FN_LAST) { last_ts = t; last_val = v; }
                else if (d_present_at(v, endRow, [&](int j) { return d_dv_at(&vv, j); },
                                      &last_val))
                  last_ts = t;
              }
            }
          } else if constexpr (FUNC == FN_TIMESTAMP) {
            if (endRow >= 0 && endRow < n) {
              int64_t t = (endRow == n - 1) ? cs.ts_last : d_lv_at(&tv, endRow);
              if (t > last_ts) { last_ts = t; last_val = (double)t / 1000.0; }
            }
          } else if (startRow <= endRow && endRow < n) {
            const bool full = (startRow == 0 && endRow == n - 1);
            constexpr bool VAR_FAMILY =
                (FUNC == FN_STDDEV || FUNC == FN_STDVAR || FUNC == FN_ZSCORE);
            if constexpr (FUNC == FN_SUM || FUNC == FN_AVG || FUNC == FN_COUNT ||
                          FUNC == FN_RATE_OVER_DELTA || VAR_FAMILY) {
              // the range's NaN-skipping moments: a whole chunk's from its summary
              double csm = NAN, csq = NAN; int cc = 0;
              if (!full)
                d_range_moments([&](int j) { return d_dv_at(&vv, j); },
                                startRow, endRow, csm, csq, cc);
              else if (cs.cnt > 0) { csm = cs.sum; csq = cs.sqsum; cc = cs.cnt; }
              if constexpr (FUNC == FN_COUNT) {
                if (isnan(sum)) sum = 0;     // CountOverTime: any range starts 0
                sum += (double)cc;
              } else {
                d_poison_add(sum, csm);       // NaN-poison quirk preserved
                icount += cc;
              }
              if constexpr (VAR_FAMILY) {
                // VarOverTimeChunkedFunctionD :1082-1115; last_sample set only
                // from a non-NaN range end (:1103)
                d_poison_add(sqsum, csq);
                const double end_raw = full ? cs.last_val : d_dv_at(&vv, endRow);
                if (!isnan(end_raw)) last_sample = end_raw;
              }
            } else if constexpr (FUNC == FN_MIN || FUNC == FN_MAX) {
              constexpr bool IS_MIN = (FUNC == FN_MIN);
              if (full) d_fold_mm<IS_MIN>(mm, IS_MIN ? cs.vmin : cs.vmax);
              else for (int i = startRow; i <= endRow; i++)
                d_fold_mm<IS_MIN>(mm, d_dv_at(&vv, i));
            } else if constexpr (FUNC == FN_IRATE || FUNC == FN_IDELTA) {
              // the window's last two rows: a range of >= 2 rows supplies
              // both, a 1-row range shifts last -> prev (the previous sample
              // is then the last row of the preceding visited range)
              const int rn = endRow - startRow + 1;
              if (rn >= 2) {
                prev_ts = d_lv_at(&tv, endRow - 1);
                prev = d_dv_at(&vv, endRow - 1);
              } else {
                prev_ts = last_ts; prev = last_val;
              }
              last_ts = (endRow == n - 1) ? cs.ts_last : d_lv_at(&tv, endRow);
              last_val = (endRow == n - 1) ? cs.last_val : d_dv_at(&vv, endRow);
              icount += rn;
            } else {  // FN_CHANGES / FN_RESETS
              constexpr bool IS_RESETS = (FUNC == FN_RESETS);
              if (isnan(changes)) changes = 0;
              double first_raw, last_raw;
              double ch;
              if (full) {
                ch = (double)(IS_RESETS ? cs.resets_in : cs.changes_in);
                first_raw = cs.first_val; last_raw = cs.last_val;
              } else {
                ch = 0;
                double p = NAN;
                for (int i = startRow; i <= endRow; i++) {
                  double x = d_dv_at(&vv, i);
                  if (i > startRow && d_pair_counts<IS_RESETS>(x, p)) ch += 1;
                  p = x;
                }
                first_raw = d_dv_at(&vv, startRow);
                last_raw = p;
              }
              if (d_pair_counts<IS_RESETS>(first_raw, prev))
                ch += 1;                      // cross-chunk boundary pair
              changes += ch;
              prev = last_raw;
            }
          }
          if (d_chunk_ends_walk(cend, wEnd)) break;
        }
        switch (FUNC) {
          case FN_SUM: result = sum; break;
          case FN_RATE_OVER_DELTA:
            // RateOverDeltaChunkedFunctionD (RateFunctions.scala:424-445)
            result = sum / (double)(wEnd - wStart) * 1000;
            break;
          case FN_COUNT: result = sum; break;
          case FN_AVG:
            result = icount > 0 ? sum / icount : (isnan(sum) ? sum : 0);
            break;
          case FN_MIN: case FN_MAX: result = mm; break;
          case FN_STDDEV: case FN_STDVAR:
            result = d_var_finish(sum, sqsum, icount, FUNC == FN_STDDEV);
            break;
          case FN_CHANGES: case FN_RESETS: result = changes; break;
          case FN_IDELTA:
            // instantValue(isRate=false), RangeInstantFunctions.scala:68-95
            if (icount >= 2) result = last_val - prev;
            break;
          case FN_IRATE:
            if (icount >= 2)
              result = d_irate_finish(last_val, prev, (double)(last_ts - prev_ts));
            break;
          case FN_LAST: case FN_PRESENT: case FN_TIMESTAMP:
            result = last_val; break;
          case FN_ZSCORE:
            result = d_zscore_finish(sum, sqsum, icount, last_sample);
            break;
        }
      }
      out[(size_t)sid * num_windows + w] = result;
    }
  }
}

// ---------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------
int32_t fdb_launch_summaries(hipStream_t stream, const uint8_t* blob, DirSoA dir,
                             int64_t num_chunks, void* sums) {
  int grid = (int)((num_chunks + 3) / 4);
  if (grid > 8192) grid = 8192;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(summary_kernel, dim3(grid), dim3(256), 0, stream,
                     blob, dir, num_chunks, (ChunkSum*)sums);
  return fdb_launched("summary_kernel");
}

int64_t fdb_chunksum_bytes(int64_t num_chunks) {
  return num_chunks * (int64_t)sizeof(ChunkSum);
}

int32_t fdb_launch_stream_walk(hipStream_t stream, const DatasetView& v,
                               const void* sums, const WindowGrid& w,
                               int func_id, double* out) {
  int grid = (v.num_series + 3) / 4;
  if (grid > 8192) grid = 8192;
  if (grid < 1) grid = 1;
  #define SARGS v.blob, v.dir, (const ChunkSum*)sums, v.series_first, \
      v.series_nchunks, v.num_series, w.start, w.step, w.end, w.window, w.n, out
  #define SCASE(F) case F: \
    hipLaunchKernelGGL((stream_walk_kernel<F>), dim3(grid), dim3(256), 0, \
                       stream, SARGS); break
  switch (func_id) {
    SCASE(FN_RATE); SCASE(FN_INCREASE); SCASE(FN_DELTA); SCASE(FN_SUM);
    SCASE(FN_COUNT); SCASE(FN_AVG); SCASE(FN_RATE_OVER_DELTA);
    SCASE(FN_MIN); SCASE(FN_MAX); SCASE(FN_STDDEV); SCASE(FN_STDVAR);
    SCASE(FN_CHANGES); SCASE(FN_LAST); SCASE(FN_PRESENT); SCASE(FN_TIMESTAMP);
    SCASE(FN_ZSCORE);
    SCASE(FN_IRATE); SCASE(FN_IDELTA); SCASE(FN_RESETS);
    default:
      fdb_set_error("stream walk: unsupported func_id %d", func_id);
      return FDB_ERR_BADARG;
  }
  #undef SCASE
  #undef SARGS
  return fdb_launched("stream_walk_kernel");
}
