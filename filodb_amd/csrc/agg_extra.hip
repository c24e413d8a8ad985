// Presenter kernels: everything that runs after a scan, over the per-series
// [S×W] grid or the aggregated [G×W] grids (group reduce, top/bottom-k, the
// aggregate presentation fixup, histogram quantile, avg division), and the
// cross-series quantile (t-digest) and count_values aggregators.
//
// The last two run as presenters over the per-series [S×W] grid the scan writes
// (the two-phase reduce of DESIGN.md §4): one THREAD per (group, window)
// cell walks its group's members in ascending series order — the exact
// insertion order of the oracle's fold, and the reference's fastReduce
// accumulator order (AggrOverRangeVectors.scala:320-377), so the t-digest
// (shared implementation, tdigest_impl.h) produces bit-identical centroids
// to the oracle.
//
//   quantile:     QuantileRowAggregator.scala:21-76 (t-digest per cell,
//                 present step = digest.quantile(q))
//   count_values: CountValuesRowAggregator.scala:26-100 (value→frequency map
//                 per cell; > limit distinct values is an error — the
//                 reference throws at 1000)

#include <cstring>
#include <cmath>

#include "engine_internal.h"
#include "tdigest_impl.h"

__global__ __launch_bounds__(64)
void quantile_cell_kernel(const double* __restrict__ grid,
                          const int32_t* __restrict__ sbg,
                          const int32_t* __restrict__ goff,
                          int ng, int nw, double q,
                          double* __restrict__ out) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)ng * nw) return;
  int g = (int)(idx / nw), w = (int)(idx % nw);
  tdigest_t td;
  td_init(&td);
  for (int i = goff[g]; i < goff[g + 1]; i++)
    td_add(&td, grid[(size_t)sbg[i] * nw + w]);
  out[idx] = td_quantile(&td, q);
}

#define CV_CAP 1000      // the reference's hard distinct-value limit

__global__ __launch_bounds__(64)
void count_values_kernel(const double* __restrict__ grid,
                         const int32_t* __restrict__ sbg,
                         const int32_t* __restrict__ goff,
                         int ng, int nw, int k_cap,
                         double* __restrict__ out_vals,
                         double* __restrict__ out_cnts,
                         int32_t* __restrict__ out_n,
                         int32_t* __restrict__ overflow) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)ng * nw) return;
  int g = (int)(idx / nw), w = (int)(idx % nw);
  double cv[CV_CAP], cc[CV_CAP];
  int n = 0;
  for (int i = goff[g]; i < goff[g + 1]; i++) {
    double x = grid[(size_t)sbg[i] * nw + w];
    if (isnan(x)) continue;
    int lo = 0, hi = n;
    while (lo < hi) { int mid = (lo + hi) / 2;
      if (cv[mid] < x) lo = mid + 1; else hi = mid; }
    if (lo < n && cv[lo] == x) { cc[lo] += 1; }
    else {
      if (n >= k_cap) { atomicExch(overflow, 1); n = -1; break; }
      for (int j = n; j > lo; j--) { cv[j] = cv[j - 1]; cc[j] = cc[j - 1]; }
      cv[lo] = x; cc[lo] = 1;
      n++;
    }
  }
  out_n[idx] = n < 0 ? 0 : n;
  for (int j = 0; j < n; j++) {
    out_vals[idx * (size_t)k_cap + j] = cv[j];
    out_cnts[idx * (size_t)k_cap + j] = cc[j];
  }
}

// cross-series group reduction from a per-series [S×W] grid. Replaces the
// contended-atomic accumulation path: the scan writes plain per-series window
// results (identical to AGG_NONE) and this kernel folds each group's
// contiguous members from the group-sorted index — one coalesced read of the
// grid instead of 2-3 f64 RMWs per (series, window) on a hot [G×W] grid.
// Semantics: RangeVectorAggregator.fastReduce (AggrOverRangeVectors.scala:
// 320-377) with the RowAggregator map/reduce rules (NaN rows skipped; MIN/MAX
// stay NaN until a value arrives). Raw sums+counts out — agg_present_kernel
// applies the presentation step, as the atomic path did.
__global__ void group_reduce_kernel(const double* __restrict__ grid,
                                    const int32_t* __restrict__ sbg,
                                    const int32_t* __restrict__ goff,
                                    int ng, int nw, int agg_id,
                                    double* __restrict__ out,
                                    double* __restrict__ cnt,
                                    double* __restrict__ sq) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)ng * nw) return;
  int g = (int)(idx / nw), w = (int)(idx % nw);
  // consecutive threads share g and walk consecutive w, so each member's row
  // grid[s*nw + w..] is read coalesced across the wave
  const int i0 = goff[g], i1 = goff[g + 1];
  if (agg_id == AGG_MIN || agg_id == AGG_MAX) {
    const bool is_min = agg_id == AGG_MIN;
    double acc = NAN, c = 0.0;
    for (int i = i0; i < i1; i++) {
      double x = grid[(size_t)sbg[i] * nw + w];
      if (isnan(x)) continue;
      c += 1.0;
      acc = isnan(acc) || (is_min ? x < acc : x > acc) ? x : acc;
    }
    out[idx] = acc;
    cnt[idx] = c;
    if (sq) sq[idx] = 0.0;
    return;
  }
  // sum-shaped reductions: 4 independent accumulator chains keep 4 loads in
  // flight (a single chain leaves the loop latency-bound far below the HBM
  // rate). Reordering the member sum is fine: the atomic path this replaced
  // already accumulated in nondeterministic order.
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  double c0 = 0, c1 = 0, q0 = 0, q1 = 0;
  int i = i0;
  for (; i + 3 < i1; i += 4) {
    double x0 = grid[(size_t)sbg[i] * nw + w];
    double x1 = grid[(size_t)sbg[i + 1] * nw + w];
    double x2 = grid[(size_t)sbg[i + 2] * nw + w];
    double x3 = grid[(size_t)sbg[i + 3] * nw + w];
    bool n0 = !isnan(x0), n1 = !isnan(x1), n2 = !isnan(x2), n3 = !isnan(x3);
    a0 += n0 ? x0 : 0.0; a1 += n1 ? x1 : 0.0;
    a2 += n2 ? x2 : 0.0; a3 += n3 ? x3 : 0.0;
    c0 += (double)n0 + (double)n2; c1 += (double)n1 + (double)n3;
    q0 += n0 ? x0 * x0 : 0.0; q1 += n1 ? x1 * x1 : 0.0;
    q0 += n2 ? x2 * x2 : 0.0; q1 += n3 ? x3 * x3 : 0.0;
  }
  for (; i < i1; i++) {
    double x = grid[(size_t)sbg[i] * nw + w];
    if (isnan(x)) continue;
    a0 += x; c0 += 1.0; q0 += x * x;
  }
  double c = c0 + c1;
  out[idx] = (agg_id == AGG_COUNT || agg_id == AGG_GROUP)
                 ? c : (a0 + a1) + (a2 + a3);
  cnt[idx] = c;
  if (sq) sq[idx] = q0 + q1;
}

// top/bottom-k presenter (TopBottomKRowAggregator.scala:29-100): one thread
// per (group, window) walks its group's series in ascending id order over the
// [S×W] grid, maintaining a sorted k-list — identical insertion order to the
// oracle's fold, so results (including ties) match exactly.
__global__ void topk_kernel(const double* __restrict__ grid,
                            const int32_t* __restrict__ sbg,
                            const int32_t* __restrict__ goff,
                            int ng, int nw, int k, int top,
                            double* __restrict__ out, double* __restrict__ ids) {
  size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)ng * nw) return;
  int g = (int)(idx / nw), w = (int)(idx % nw);
  double best[16], bid[16];
  for (int j = 0; j < 16; j++) { best[j] = NAN; bid[j] = -1; }
  for (int i = goff[g]; i < goff[g + 1]; i++) {
    int s = sbg[i];
    double x = grid[(size_t)s * nw + w];
    if (isnan(x)) continue;
    int pos = -1;
    for (int j = 0; j < k; j++)
      if (isnan(best[j]) || (top ? x > best[j] : x < best[j])) { pos = j; break; }
    if (pos >= 0) {
      for (int j = k - 1; j > pos; j--) { best[j] = best[j - 1]; bid[j] = bid[j - 1]; }
      best[pos] = x; bid[pos] = (double)s;
    }
  }
  for (int j = 0; j < k; j++) {
    out[idx * k + j] = best[j];
    if (ids) ids[idx * k + j] = bid[j];
  }
}

// presentation fixup for aggregated grids (NaN where no contributions; mean for avg)
__global__ void agg_present_kernel(double* out, const double* cnt, const double* sq,
                                   size_t n, int agg_id, int partial) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (partial) return;                      // partial mode: leave raw sums + counts
  if (cnt[i] <= 0) { out[i] = NAN; return; }
  if (agg_id == AGG_GROUP) out[i] = 1.0;   // GroupRowAggregator.scala:12-31
  else if (agg_id == AGG_AVG) out[i] = out[i] / cnt[i];
  else if (agg_id == AGG_STDDEV || agg_id == AGG_STDVAR) {
    double mean = out[i] / cnt[i];
    double var = sq[i] / cnt[i] - mean * mean;   // StddevRowAggregator.scala:49-52
    out[i] = agg_id == AGG_STDDEV ? sqrt(var) : var;
  }
}

// --- histogram present step, every mode (FDB_HP_*) ---------------------------
// One thread per cell over a geometric scheme: top(b) = first * pow(mult, b).
// A geometric scheme is never Base2ExpHistogramBuckets: interpolation is
// linear and no top is +Inf.

// Histogram.quantile(q, min, max) (Histogram.scala:65-108). clip = false is
// the plain Histogram.quantile(q) (no min/max step): the one implementation
// behind out_quantile and FDB_HP_QUANTILE, so the two return the same bits.
// The firstBucketGTE walk stops at nb - 1, so a NaN sum cannot leave the
// cell; the reference's unbounded walk ends there too for valid input
// (passing bucket nb - 1 needs top < q * top with 0 <= q <= 1 and top > 0).
__device__ double hp_quantile(const double* __restrict__ v, int nb, double q,
                              double first, double mult, bool clip,
                              double mn, double mx) {
  double top = v[nb - 1];
  if (q < 0) return -INFINITY;
  if (q > 1) return INFINITY;
  if (nb < 2 || !(top > 0)) return NAN;
  double rank = q * top;
  int bucket = 0;
  while (bucket < nb - 1 && v[bucket] < rank) bucket++;
  double bucketStart = bucket == 0 ? 0 : first * pow(mult, bucket - 1);
  double bucketEnd = first * pow(mult, bucket);
  if (clip) {   // a NaN min/max compares false and clips nothing
    if (mn > bucketStart && mn <= bucketEnd) bucketStart = mn;
    if (mx > bucketStart && mx <= bucketEnd) bucketEnd = mx;
  }
  if (bucket == nb - 1 && isinf(bucketEnd)) return first * pow(mult, nb - 2);
  if (bucket == 0 && first <= 0) return first;
  double count = bucket == 0 ? v[0] : v[bucket] - v[bucket - 1];
  rank -= bucket == 0 ? 0 : v[bucket - 1];
  return bucketStart + (bucketEnd - bucketStart) * (rank / count);
}

// java.lang.Math.max/min: NaN if either argument is NaN
__device__ __forceinline__ double hp_jmax(double a, double b) {
  return (isnan(a) || isnan(b)) ? NAN : (a > b ? a : b);
}
__device__ __forceinline__ double hp_jmin(double a, double b) {
  return (isnan(a) || isnan(b)) ? NAN : (a < b ? a : b);
}

// Histogram.histogramFraction(lower, upper, min, max) (Histogram.scala:119-197),
// linear branch. The host has checked lower >= 0 && upper >= 0.
__device__ double hp_fraction(const double* __restrict__ v, int nb,
                              double lower, double upper,
                              double first, double mult, double mn, double mx) {
  const double count = v[nb - 1];
  if (count == 0) return NAN;
  if (lower == 0 && upper == 0) return v[0] / count;
  if (lower >= upper) return 0.0;
  double lowerRank = 0.0, upperRank = 0.0;
  bool lowerSet = false, upperSet = false;
  double bucketLower = 0.0, prevVal = 0.0;
  for (int b = 0; b < nb && (!lowerSet || !upperSet); b++) {
    const double bucketUpper = first * pow(mult, b);
    const double val = v[b];
    const double low = hp_jmax(bucketLower, mn);
    const double high = hp_jmin(bucketUpper, mx);
    if (!lowerSet && bucketLower == lower) { lowerRank = prevVal; lowerSet = true; }
    if (!upperSet && bucketUpper == upper) { upperRank = val; upperSet = true; }
    if (!lowerSet && bucketLower < lower && bucketUpper > lower) {
      lowerRank = prevVal + (val - prevVal) * ((lower - low) / (high - low));
      lowerSet = true;
    }
    if (!upperSet && bucketLower < upper && bucketUpper > upper) {
      upperRank = prevVal + (val - prevVal) * ((upper - low) / (high - low));
      upperSet = true;
    }
    bucketLower = bucketUpper;
    prevVal = val;
  }
  if (!lowerSet || lowerRank > count) lowerRank = count;
  if (!upperSet || upperRank > count) upperRank = count;
  return (upperRank - lowerRank) / count;
}

// HistogramBucketImpl (InstantFunction.scala:433-453): the first bucket whose
// top is within 1e-10 of le, else NaN
__device__ double hp_bucket(const double* __restrict__ v, int nb, double le,
                            double first, double mult) {
  for (int b = 0; b < nb; b++)
    if (fabs(first * pow(mult, b) - le) <= 1e-10) return v[b];
  return NAN;
}

// maxs/mins are null unless the mode reads them (the host checks). cnt == 0 is
// the reference's empty histogram: NaN in every mode.
__global__ void hist_present_kernel(const double* __restrict__ sums,
                                    const double* __restrict__ cnt,
                                    const double* __restrict__ maxs,
                                    const double* __restrict__ mins,
                                    double* __restrict__ out,
                                    size_t cells, int nb, int present_id,
                                    double p0, double p1,
                                    double first, double mult) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cells) return;
  if (!(cnt[i] > 0)) { out[i] = NAN; return; }
  const double* v = sums + i * nb;
  double r = NAN;
  switch (present_id) {
    case FDB_HP_QUANTILE:
      r = hp_quantile(v, nb, p0, first, mult, false, 0, 0); break;
    case FDB_HP_QUANTILE_MINMAX:
      r = hp_quantile(v, nb, p0, first, mult, true, mins[i], maxs[i]); break;
    case FDB_HP_MAX_QUANTILE:
      r = hp_quantile(v, nb, p0, first, mult, true, 0, maxs[i]); break;
    case FDB_HP_BUCKET:
      r = hp_bucket(v, nb, p0, first, mult); break;
    case FDB_HP_FRACTION:
      r = hp_fraction(v, nb, p0, p1, first, mult, -INFINITY, INFINITY); break;
    case FDB_HP_FRACTION_MINMAX:
      r = hp_fraction(v, nb, p0, p1, first, mult, mins[i], maxs[i]); break;
  }
  out[i] = r;
}

__global__ void avg_div_kernel(double* __restrict__ out,
                               const double* __restrict__ a,
                               const double* __restrict__ b, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a[i] / b[i];
}

// ---------------------------------------------------------------------------
// host-side launchers (prototypes in engine_internal.h)
// ---------------------------------------------------------------------------
// one thread per element, 256-thread blocks
static dim3 blocks256(size_t n) { return dim3((uint32_t)((n + 255) / 256)); }

int32_t fdb_launch_group_reduce(hipStream_t stream, const double* grid,
                                const DatasetView& v, const WindowGrid& w,
                                int ng, int agg_id,
                                double* out, double* cnt, double* sq) {
  hipLaunchKernelGGL(group_reduce_kernel, blocks256((size_t)ng * w.n), dim3(256),
                     0, stream, grid, v.sbg, v.goff, ng, w.n, agg_id, out, cnt, sq);
  return fdb_launched("group_reduce_kernel");
}

int32_t fdb_launch_topk(hipStream_t stream, const double* grid,
                        const DatasetView& v, const WindowGrid& w,
                        int ng, int k, int top, double* out, double* ids) {
  hipLaunchKernelGGL(topk_kernel, blocks256((size_t)ng * w.n), dim3(256), 0,
                     stream, grid, v.sbg, v.goff, ng, w.n, k, top, out, ids);
  return fdb_launched("topk_kernel");
}

int32_t fdb_launch_agg_present(hipStream_t stream, double* out,
                               const double* cnt, const double* sq,
                               size_t n, int agg_id, int partial) {
  hipLaunchKernelGGL(agg_present_kernel, blocks256(n), dim3(256), 0, stream,
                     out, cnt, sq, n, agg_id, partial);
  return fdb_launched("agg_present_kernel");
}

bool fdb_hist_present_needs_mm(int present_id) {
  return present_id == FDB_HP_QUANTILE_MINMAX ||
         present_id == FDB_HP_MAX_QUANTILE ||
         present_id == FDB_HP_FRACTION_MINMAX;
}

// the argument rules of a present step, checked before anything is launched
int32_t fdb_hist_present_check(int present_id, double p0, double p1,
                               bool have_mm, int nb) {
  if (present_id < FDB_HP_QUANTILE || present_id > FDB_HP_FRACTION_MINMAX) {
    fdb_set_error("unknown histogram present id %d (FDB_HP_*)", present_id);
    return FDB_ERR_BADARG;
  }
  if (nb < 1 || nb > 64) { fdb_set_error("num_buckets must be 1..64"); return FDB_ERR_BADARG; }
  const bool fraction = present_id == FDB_HP_FRACTION ||
                        present_id == FDB_HP_FRACTION_MINMAX;
  if (fraction && !(p0 >= 0 && p1 >= 0)) {   // the reference's require; NaN fails it
    fdb_set_error("lower & upper params should be >= 0: lower=%g, upper=%g", p0, p1);
    return FDB_ERR_BADARG;
  }
  if (present_id == FDB_HP_BUCKET && std::isinf(p0) && p0 > 0) {
    fdb_set_error("+Inf bucket not in the last position (a geometric scheme "
                  "has no +Inf top)");
    return FDB_ERR_BADARG;
  }
  if (fdb_hist_present_needs_mm(present_id) && !have_mm) {
    fdb_set_error("histogram present id %d needs max and min inputs", present_id);
    return FDB_ERR_BADARG;
  }
  return FDB_OK;
}

int32_t fdb_launch_hist_present(hipStream_t stream, const double* sums,
                                const double* cnt, const double* maxs,
                                const double* mins, double* out, size_t cells,
                                int nb, int present_id, double p0, double p1,
                                double first, double mult) {
  if (int32_t rc = fdb_hist_present_check(present_id, p0, p1, maxs && mins, nb))
    return rc;
  hipLaunchKernelGGL(hist_present_kernel, blocks256(cells), dim3(256), 0,
                     stream, sums, cnt, maxs, mins, out, cells, nb, present_id,
                     p0, p1, first, mult);
  return fdb_launched("hist_present_kernel");
}

int32_t fdb_launch_avg_div(hipStream_t stream, double* out, const double* a,
                           const double* b, size_t n) {
  hipLaunchKernelGGL(avg_div_kernel, blocks256(n), dim3(256), 0, stream,
                     out, a, b, n);
  return fdb_launched("avg_div_kernel");
}

int32_t fdb_launch_quantile_cells(hipStream_t stream, const double* grid,
                                  const DatasetView& v, const WindowGrid& w,
                                  int ng, double q, double* out) {
  size_t cells = (size_t)ng * w.n;
  hipLaunchKernelGGL(quantile_cell_kernel,
                     dim3((uint32_t)((cells + 63) / 64)), dim3(64), 0, stream,
                     grid, v.sbg, v.goff, ng, w.n, q, out);
  return fdb_launched("quantile_cell_kernel");
}

int32_t fdb_launch_count_values(hipStream_t stream, const double* grid,
                                const DatasetView& v, const WindowGrid& w,
                                int ng, int k_cap,
                                double* out_vals, double* out_cnts,
                                int32_t* out_n, int32_t* overflow) {
  if (k_cap < 1 || k_cap > CV_CAP) {
    fdb_set_error("count_values k_cap %d out of range 1..%d", k_cap, CV_CAP);
    return FDB_ERR_BADARG;
  }
  size_t cells = (size_t)ng * w.n;
  hipLaunchKernelGGL(count_values_kernel,
                     dim3((uint32_t)((cells + 63) / 64)), dim3(64), 0, stream,
                     grid, v.sbg, v.goff, ng, w.n, k_cap, out_vals, out_cnts,
                     out_n, overflow);
  return fdb_launched("count_values_kernel");
}
