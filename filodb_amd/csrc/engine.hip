// MI355X (gfx950) engine, host side: engine and dataset lifecycle, upload,
// launch dispatch and the C-ABI entry points. The kernels live beside it
// (scan_fast.hip, scan_stream.hip, window_sample.hip, hist2.hip and the
// presenters in agg_extra.hip) behind the launchers of engine_internal.h.
//
// Replaces, as one batched GPU launch per (shard, query), the per-window virtual
// dispatch of the reference execution engine:
//   ChunkedWindowIterator.doNext        query/.../exec/PeriodicSamplesMapper.scala:293-330
//   WindowedChunkIterator               core/.../store/ChunkSetInfo.scala:445-529
//   ChunkedRangeFunction.addChunks      query/.../rangefn/RangeFunction.scala:101-198
//   ChunkedRateFunctionBase/extrapolatedRate  rangefn/RateFunctions.scala:72-111,230-289
//   gauge over-time functions           rangefn/AggrOverTimeFunctions.scala
//   RangeVectorAggregator.fastReduce    query/.../exec/AggrOverRangeVectors.scala:320-377
//
// Execution model: one 64-lane wavefront per series; 256-thread
// blocks = 4 series; chunks decoded into LDS once per series; windows parallel
// across lanes reading LDS (the ~97% window overlap is served on-chip). Counter
// correction is a wave-wide prefix scan; the chunk→chunk carry is sequential in
// time order exactly like the reference's CorrectionMeta carry.
//
// There is NO CPU fallback: engine creation fails without a HIP device.

#include <cstring>
#include <cstdio>
#include <cmath>
#include <vector>
#include <cstdlib>
#include <memory>

#include "engine_internal.h"
#include "fast_desc.h"

// ---------------------------------------------------------------------------
// host engine
// ---------------------------------------------------------------------------
struct fdb_engine {
  int device;
  hipStream_t stream;
  int32_t* dev_flag;        // sample-kernel overflow flag (device)
};

// every device table is owned: `delete d` frees them all
struct fdb_dataset {
  DevPtr<uint8_t> blob;
  DevPtr<uint64_t> ts_off, val_off;
  DevPtr<int64_t> start_time, end_time;
  DevPtr<int32_t> num_rows;
  DevPtr<int32_t> series_first, series_nchunks, group_ids;
  DevPtr<int32_t> series_by_group, group_offsets;   // group-sorted series index (topk)
  DevPtr<uint64_t> max_off, min_off;  // hist companion column offsets (0 = absent)
  DevPtr<uint8_t> sums;     // ChunkSum[num_chunks] for the streaming walk
  // fast scan decode descriptors, one per series (fast_desc.h), built at
  // upload when fast_ok; fast_desc_sc describes the count column riding
  // max_off (has_sc) so avg_sc's second scan takes the same kernel
  DevPtr<FdbFastDesc> fast_desc, fast_desc_sc;
  int32_t num_series = 0;
  int64_t num_chunks = 0;
  int64_t payload_bytes = 0;  // sum of vector bytes (algorithmic HBM footprint)
  int64_t total_samples = 0;
  int max_group = 0;        // max group id seen (for validation)
  int has_hist = 0;         // dataset holds sect-delta histogram vectors
  int fast_ok = 0;          // single-chunk series, chunk spans fit i32 ms
  int has_mm = 0;           // every hist chunk carries max/min columns
  int has_sc = 0;           // every scalar chunk carries a count column
  // bucket scheme (first, mult) of a histogram dataset, from its first vector
  double hist_scheme[2] = {0, 0};
  // host copies of up to FDB_FAST_SAMPLE evenly spaced descriptors per table:
  // the launcher runs the aligned-rows test on them with the query at hand
  // and picks the kernel build by the share that passes (scan_fast.hip)
  FdbFastDesc fast_sample[2][FDB_FAST_SAMPLE] = {};
  int fast_nsample = 0;
};

// the dataset as the kernels take it; count_col swaps the value column for
// the count column riding max_off (avg_sc)
static DatasetView view_of(const fdb_dataset_t* d, bool count_col = false) {
  return DatasetView{
      d->blob.get(),
      DirSoA{d->ts_off.get(), count_col ? d->max_off.get() : d->val_off.get(),
             d->start_time.get(), d->end_time.get(), d->num_rows.get()},
      d->max_off.get(), d->min_off.get(), d->series_first.get(),
      d->series_nchunks.get(), d->group_ids.get(), d->series_by_group.get(),
      d->group_offsets.get(), d->num_series};
}

// FDB_FAST=0 (perf/parity experiments): queries take the general path, and an
// upload keeps the chunk summaries that path needs
static bool fast_disabled() { return fdb_env_int("FDB_FAST", 1) == 0; }

extern "C" fdb_engine_t* fdb_engine_create(int32_t device) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) {
    fdb_set_error("no HIP device present (hipGetDeviceCount: %s) — "
                  "filodb_amd has no CPU fallback", hipGetErrorString(e));
    return nullptr;
  }
  if (device < 0 || device >= count) { fdb_set_error("bad device %d", device); return nullptr; }
  HIP_CHECK_NULL(hipSetDevice(device));
  auto* eng = new fdb_engine();
  eng->device = device;
  if (hipStreamCreate(&eng->stream) != hipSuccess) {
    fdb_set_error("hipStreamCreate failed");
    delete eng;
    return nullptr;
  }
  if (hipMalloc(&eng->dev_flag, 4) != hipSuccess ||
      hipMemset(eng->dev_flag, 0, 4) != hipSuccess) {
    fdb_set_error("engine flag allocation failed");
    (void)hipStreamDestroy(eng->stream);
    delete eng;
    return nullptr;
  }
  return eng;
}

extern "C" void fdb_engine_destroy(fdb_engine_t* e) {
  if (!e) return;
  (void)hipFree(e->dev_flag);
  (void)hipStreamDestroy(e->stream);
  delete e;
}

hipStream_t fdb_engine_stream(fdb_engine_t* e) { return e->stream; }

extern "C" int32_t fdb_engine_synchronize(fdb_engine_t* e) {
  HIP_CHECK(hipStreamSynchronize(e->stream));
  return FDB_OK;
}

extern "C" void fdb_dataset_destroy(fdb_dataset_t* d) { delete d; }

extern "C" int64_t fdb_dataset_bytes(const fdb_dataset_t* d) { return d->payload_bytes; }
extern "C" int64_t fdb_dataset_samples(const fdb_dataset_t* d) { return d->total_samples; }

// --- upload, in steps ---------------------------------------------------------

// what one pass over the chunk directory finds
struct DirScan {
  std::vector<uint64_t> ts_off, val_off, max_off, min_off;   // SoA columns
  std::vector<int64_t> start, end;
  std::vector<int32_t> rows;
  int64_t payload = 0, samples = 0;
  int has_hist = 0, has_scalar = 0, max_chunk_rows = 0, spans_fit_i32 = 1;
  int any_mm = 0, all_mm = 1;
};

static DirScan scan_directory(const fdb_view_t& view) {
  const fdb_dir_entry_t* dir = (const fdb_dir_entry_t*)view.dir;
  const size_t nc = (size_t)view.num_chunks;
  DirScan s;
  s.ts_off.resize(nc); s.val_off.resize(nc); s.max_off.resize(nc); s.min_off.resize(nc);
  s.start.resize(nc); s.end.resize(nc); s.rows.resize(nc);
  auto vec_bytes = [&](uint64_t off) {   // a vector's length word plus what it counts
    uint32_t len;
    memcpy(&len, view.blob + off, 4);
    return (int64_t)len + 4;
  };
  for (size_t i = 0; i < nc; i++) {
    const fdb_dir_entry_t& c = dir[i];
    s.ts_off[i] = c.ts_off; s.val_off[i] = c.val_off;
    s.max_off[i] = c.max_off; s.min_off[i] = c.min_off;
    s.start[i] = c.start_time; s.end[i] = c.end_time; s.rows[i] = c.num_rows;
    s.payload += vec_bytes(c.ts_off) + vec_bytes(c.val_off);
    if (c.max_off) {
      s.any_mm = 1;
      s.payload += vec_bytes(c.max_off) + vec_bytes(c.min_off);
    } else {
      s.all_mm = 0;
    }
    s.samples += c.num_rows;
    uint16_t wf;
    memcpy(&wf, view.blob + c.val_off + 4, 2);
    if (wf == FDB_WF_HIST_SECTDELTA) s.has_hist = 1; else s.has_scalar = 1;
    if (c.num_rows > s.max_chunk_rows) s.max_chunk_rows = c.num_rows;
    if (c.end_time - c.start_time >= (int64_t)1 << 31) s.spans_fit_i32 = 0;
  }
  return s;
}

// group-sorted series index for the top/bottom-k presenter: stable ascending
// series order per group (ties then resolve identically to the oracle's fold)
static void group_index(const fdb_view_t& view, int max_group,
                        std::vector<int32_t>* sbg, std::vector<int32_t>* goff) {
  goff->assign((size_t)max_group + 2, 0);
  for (int32_t s = 0; s < view.num_series; s++) (*goff)[(size_t)view.group_ids[s] + 1]++;
  for (size_t g = 1; g < goff->size(); g++) (*goff)[g] += (*goff)[g - 1];
  sbg->resize((size_t)view.num_series);
  std::vector<int32_t> cur(goff->begin(), goff->end() - 1);
  for (int32_t s = 0; s < view.num_series; s++)
    (*sbg)[(size_t)cur[(size_t)view.group_ids[s]]++] = s;
}

// fast scan descriptors of one column (0: values, 1: the count column): every
// per-series fact the kernel needs before it touches the payload, parsed once
// from the host blob (fast_desc.h). A vector the record cannot address (not
// 64-B aligned, or past 2^38 B) clears fast_ok and sends the dataset down the
// general path instead. False only when the device upload fails.
static bool upload_fast_descs(fdb_dataset_t* d, const fdb_view_t& view,
                              const DirScan& s, int col) {
  const int32_t ns = view.num_series;
  const std::vector<uint64_t>& voff = col ? s.max_off : s.val_off;
  std::vector<FdbFastDesc> desc((size_t)ns);
  int addressable = 1;
  #pragma omp parallel for schedule(static) reduction(&:addressable)
  for (int32_t sid = 0; sid < ns; sid++) {
    const int32_t c = view.series_first[sid];
    const bool has = view.series_nchunks[sid] >= 1;
    if (has && (((s.ts_off[c] | voff[c]) & 63) != 0 ||
                ((s.ts_off[c] | voff[c]) >> 38) != 0)) {
      addressable = 0;
      continue;
    }
    fdb_build_fast_desc(view.blob, has ? s.ts_off[c] : 0, has ? voff[c] : 0,
                        has ? s.rows[c] : 0, &desc[(size_t)sid]);
  }
  if (!addressable) { d->fast_ok = 0; return true; }
  d->fast_nsample = ns < FDB_FAST_SAMPLE ? ns : FDB_FAST_SAMPLE;
  for (int k = 0; k < d->fast_nsample; k++)
    d->fast_sample[col][k] = desc[(size_t)((int64_t)k * ns / d->fast_nsample)];
  return (col ? d->fast_desc_sc : d->fast_desc).upload(desc.data(), desc.size());
}

// chunk summaries for the streaming walk (query-independent)
static int32_t build_summaries(fdb_engine_t* e, fdb_dataset_t* d) {
  if (!d->sums.alloc((size_t)fdb_chunksum_bytes(d->num_chunks))) {
    fdb_set_error("summary allocation failed (out of HBM?)");
    return FDB_ERR;
  }
  return fdb_launch_summaries(e->stream, d->blob.get(), view_of(d).dir,
                              d->num_chunks, d->sums.get());
}

extern "C" fdb_dataset_t* fdb_dataset_upload(fdb_engine_t* e, const fdb_store_t* s) {
  fdb_view_t view;
  if (fdb_store_view(s, &view) != FDB_OK) return nullptr;
  HIP_CHECK_NULL(hipSetDevice(e->device));

  const DirScan ds = scan_directory(view);
  const size_t nc = (size_t)view.num_chunks, ns = (size_t)view.num_series;
  if (ds.has_hist && ds.has_scalar) {
    fdb_set_error("mixed histogram and scalar series in one store are not "
                  "supported — upload them as separate datasets");
    return nullptr;
  }
  int max_group = 0, max_chunks = 0;
  for (int32_t sid = 0; sid < view.num_series; sid++) {
    if (view.group_ids[sid] > max_group) max_group = view.group_ids[sid];
    if (view.series_nchunks[sid] > max_chunks) max_chunks = view.series_nchunks[sid];
  }
  if (ds.max_chunk_rows > FDB_DEFAULT_MAX_ROWS) {
    fdb_set_error("chunk has %d rows; the reference's chunk cap is %d "
                  "(filodb-defaults.conf:835)", ds.max_chunk_rows,
                  FDB_DEFAULT_MAX_ROWS);
    return nullptr;
  }

  std::unique_ptr<fdb_dataset> d(new fdb_dataset());
  d->num_series = view.num_series;
  d->num_chunks = view.num_chunks;
  d->payload_bytes = ds.payload;
  d->total_samples = ds.samples;
  d->max_group = max_group;
  d->has_hist = ds.has_hist;
  d->fast_ok = !ds.has_hist && max_chunks <= 1 && ds.spans_fit_i32;
  d->has_mm = ds.has_hist && ds.any_mm && ds.all_mm;
  d->has_sc = ds.has_scalar && ds.any_mm && ds.all_mm;   // count column rides max_off
  if (ds.has_hist)
    memcpy(d->hist_scheme, view.blob + ds.val_off[0] + FDB_HIST_OFF_DEF + 2, 16);

  std::vector<int32_t> sbg, goff;
  group_index(view, max_group, &sbg, &goff);
  // +512 B tail pad on the blob: the hist walk's wave-staged element reads may
  // extend up to 256 B past the last element's start, and its linear stage
  // PREFETCH one further 256-B window beyond that
  bool ok = d->blob.upload(view.blob, (size_t)view.blob_len, 512)
    && d->ts_off.upload(ds.ts_off.data(), nc)
    && d->val_off.upload(ds.val_off.data(), nc)
    && d->start_time.upload(ds.start.data(), nc)
    && d->end_time.upload(ds.end.data(), nc)
    && d->num_rows.upload(ds.rows.data(), nc)
    && d->series_first.upload(view.series_first, ns)
    && d->series_nchunks.upload(view.series_nchunks, ns)
    && d->group_ids.upload(view.group_ids, ns)
    && d->series_by_group.upload(sbg.data(), sbg.size())
    && d->group_offsets.upload(goff.data(), goff.size())
    && d->max_off.upload(ds.max_off.data(), nc)
    && d->min_off.upload(ds.min_off.data(), nc);
  for (int col = 0; col < (d->has_sc ? 2 : 1) && ok && d->fast_ok; col++)
    ok = upload_fast_descs(d.get(), view, ds, col);
  if (!ok) {
    fdb_set_error("device upload failed (out of HBM?)");
    return nullptr;
  }
  // summaries are skipped when every series takes the single-chunk fast path;
  // FDB_FAST=0 at upload keeps them, so the same dataset can be walked by the
  // general path for A/B runs
  if (ds.has_scalar && (!d->fast_ok || fast_disabled()) &&
      build_summaries(e, d.get()) != FDB_OK)
    return nullptr;
  return d.release();
}

// the fast single-chunk kernel handles this (dataset, query) pair?
static bool fast_eligible(const fdb_dataset_t* d, const fdb_query_t* q) {
  return !fast_disabled() && d->fast_ok && fdb_scan_supported(q->func_id) &&
         q->step > 0 && q->step < ((int64_t)1 << 31) && q->window >= 0;
}

static int32_t launch_fast(fdb_engine_t* e, const fdb_dataset_t* d, const fdb_query_t* q,
                           const WindowGrid& w, int agg_id, bool emit_group,
                           double* out, double* cnt, double* sq, bool count_col = false) {
  return fdb_launch_fast_scan(e->stream, view_of(d, count_col),
                              (count_col ? d->fast_desc_sc : d->fast_desc).get(),
                              d->fast_sample[count_col ? 1 : 0], d->fast_nsample,
                              w, q->func_id, agg_id, emit_group, out, cnt, sq, q->_pad);
}

// the scan of q's range function into the per-series [S×W] grid dev_out
static int32_t launch_scan(fdb_engine_t* e, const fdb_dataset_t* d, const fdb_query_t* q,
                           const WindowGrid& w, double* dev_out, double* dev_cnt,
                           bool count_col = false) {
  if (fast_eligible(d, q))
    return launch_fast(e, d, q, w, AGG_NONE, false, dev_out, dev_cnt, nullptr, count_col);
  const DatasetView v = view_of(d, count_col);
  // sample-buffer functions (quantile/MAD/predict_linear) have their own
  // per-(series,window) kernel, on any dataset shape
  if (fdb_window_sample_supported(q->func_id))
    return fdb_launch_window_sample(e->stream, v, w, q->func_id, q->param,
                                    q->param2, dev_out, e->dev_flag);
  // everything else: the unbounded summary+walk general path. It writes the
  // per-series [S×W] grid only (aggregation is the two-phase reduce outside).
  if (!fdb_scan_supported(q->func_id)) {
    fdb_set_error("bad func_id %d", q->func_id);
    return FDB_ERR_BADARG;
  }
  if (!d->sums) {
    fdb_set_error("dataset has no chunk summaries (internal)");
    return FDB_ERR;
  }
  return fdb_launch_stream_walk(e->stream, v, d->sums.get(), w, q->func_id, dev_out);
}

// window-grid checks every query entry point shares; bad_nw is the entry
// point's own message for an empty or inverted window grid
static int32_t check_windows(const fdb_query_t* q, const char* bad_nw, WindowGrid* w) {
  *w = WindowGrid{q->start, q->step, q->end, q->window, fdb_num_windows(q)};
  if (w->n <= 0) { fdb_set_error("%s", bad_nw); return FDB_ERR_BADARG; }
  if (q->window > ((int64_t)1 << 33)) {   // d_div1000 exactness domain
    fdb_set_error("window length > 2^33 ms (~99 days) unsupported");
    return FDB_ERR_BADARG;
  }
  return FDB_OK;
}

static int32_t alloc_failed(const char* who) {
  fdb_set_error("%s: device allocation failed (out of HBM?)", who);
  return FDB_ERR;
}

// Waits for the stream, then reads the engine's overflow flag and clears it
// if it was raised. The window-sample kernels and count_values_kernel share
// the flag, so each is asked about right after it ran.
static int32_t take_overflow(fdb_engine_t* e, bool* raised) {
  int32_t flag = 0;
  HIP_CHECK(hipStreamSynchronize(e->stream));
  HIP_CHECK(hipMemcpy(&flag, e->dev_flag, 4, hipMemcpyDeviceToHost));
  if (flag) HIP_CHECK(hipMemset(e->dev_flag, 0, 4));
  *raised = flag != 0;
  return FDB_OK;
}

static int32_t sample_overflow_error() {
  fdb_set_error("a window exceeded the %d-sample buffer of the "
                "quantile/MAD kernel", 1024);
  return FDB_ERR;
}

// what run_query decides before it allocates anything
struct QueryPlan {
  WindowGrid w;
  int k;                   // top/bottom-k's k, else 0
  size_t out_len, buf_len; // cells of the result grid; doubles in the caller's `out`
  bool is_topk, is_quant, needs_sq, partial, fused;
};

static int32_t plan_query(const fdb_dataset_t* d, const fdb_query_t* q,
                          bool has_counts, QueryPlan* p) {
  if (d->has_hist) {
    fdb_set_error("histogram dataset: use fdb_query_exec_hist");
    return FDB_ERR_BADARG;
  }
  if (int32_t rc = check_windows(q, "bad window params", &p->w)) return rc;
  if (q->func_id == FDB_FN_HOLT_WINTERS &&
      !(q->param >= 0 && q->param <= 1 && q->param2 >= 0 && q->param2 <= 1)) {
    // parseParameters (AggrOverTimeFunctions.scala:1373-1382)
    fdb_set_error("holt_winters sf/tf must be in [0, 1]");
    return FDB_ERR_BADARG;
  }
  const bool agg = q->agg_id != AGG_NONE;
  p->is_topk = q->agg_id == AGG_TOPK || q->agg_id == AGG_BOTTOMK;
  p->k = p->is_topk ? (int)q->param : 0;
  if (p->is_topk && (p->k < 1 || p->k > 16)) {
    fdb_set_error("topk k=%d out of range 1..16 (q.param)", p->k);
    return FDB_ERR_BADARG;
  }
  if (agg && (q->num_groups <= 0 || d->max_group >= q->num_groups)) {
    fdb_set_error("num_groups %d inconsistent with dataset max group %d",
                  q->num_groups, d->max_group);
    return FDB_ERR_BADARG;
  }
  p->out_len = !agg ? (size_t)d->num_series * p->w.n
             : (size_t)q->num_groups * p->w.n * (p->is_topk ? p->k : 1);
  p->needs_sq = q->agg_id == AGG_STDDEV || q->agg_id == AGG_STDVAR;
  p->partial = agg && !p->is_topk && has_counts;
  // stddev/stdvar partials ship (raw sums, raw sumsq) stacked: the caller's
  // `out` is [2 × G × W]; shards merge both halves + counts by addition —
  // algebraically StddevRowAggregator.scala:36-52's reduction
  p->buf_len = (p->needs_sq && p->partial) ? p->out_len * 2 : p->out_len;
  p->is_quant = q->agg_id == AGG_QUANTILE;
  if (p->is_quant && has_counts) {
    fdb_set_error("quantile aggregation has no partial (multi-shard) mode — "
                  "digest shipping is not implemented");
    return FDB_ERR_BADARG;
  }
  // aggregated queries: the fused-group fast path folds fastReduce into the
  // scan (per-lane register partials + one atomic burst per group change) and
  // never materializes the [S×W] grid; other shapes run two-phase — the scan
  // fills an internal per-series grid with plain stores, then a presenter
  // (topk_kernel / group_reduce_kernel) folds it along the group-sorted index.
  // The fused-group emit measured ~6% SLOWER than the two-phase reduce at
  // current scan cost (3.20 vs 3.02 ms on configs[5]; the scan is
  // compute-bound, so skipping the grid re-read does not pay yet) — two-phase
  // is the default, FDB_FUSED_GROUP=1 opts in
  p->fused = fdb_env_int("FDB_FUSED_GROUP", 0) == 1 && !p->is_quant && agg &&
             !p->is_topk && p->w.n <= 256 && fast_eligible(d, q);
  return FDB_OK;
}

static int32_t run_query(fdb_engine_t* e, const fdb_dataset_t* d, const fdb_query_t* q,
                         double* out, double* out_counts, int32_t out_on_device,
                         int32_t warmup, int32_t iters, double* avg_ms) {
  HIP_CHECK(hipSetDevice(e->device));
  QueryPlan p;
  if (int32_t rc = plan_query(d, q, out_counts != nullptr, &p)) return rc;
  const bool agg = q->agg_id != AGG_NONE;
  const DatasetView v = view_of(d);

  // every exit (including the HIP_CHECK early returns) releases what this call
  // owns — device buffers and events must not leak on a failed launch
  OutBuf dev_out(out, out_on_device, p.buf_len), dev_cnt(out_counts, out_on_device, p.out_len);
  DevBuf dev_sq, per_grid;
  DevEvent ev0, ev1;
  if (!dev_out.alloc() || (agg && !dev_cnt.alloc())) return alloc_failed("query");
  if (p.needs_sq) {
    if (p.partial) dev_sq.wrap(dev_out.get() + p.out_len);   // second half of the caller grid
    else if (!dev_sq.alloc(p.out_len * 8)) return alloc_failed("query");
  }
  HIP_CHECK(ev0.create());
  HIP_CHECK(ev1.create());
  fdb_query_t qscan = *q;
  if (agg && !p.fused) {
    if (!per_grid.alloc((size_t)d->num_series * p.w.n * 8)) return alloc_failed("query");
    qscan.agg_id = AGG_NONE;
  }

  // one run of the query's launches: the fused scan, or scan + presenter
  auto run_once = [&]() -> int32_t {
    if (p.fused) {
      // atomically-accumulated grids: reset per launch. MIN/MAX start the
      // value grid at NaN (atomic_min_max_f64's empty-cell marker).
      const bool mm = q->agg_id == AGG_MIN || q->agg_id == AGG_MAX;
      HIP_CHECK(hipMemsetAsync(dev_out.get(), mm ? 0xFF : 0, p.buf_len * 8, e->stream));
      HIP_CHECK(hipMemsetAsync(dev_cnt.get(), 0, p.out_len * 8, e->stream));
      if (dev_sq && !(p.needs_sq && p.partial))
        HIP_CHECK(hipMemsetAsync(dev_sq.get(), 0, p.out_len * 8, e->stream));
      return launch_fast(e, d, q, p.w, q->agg_id, true, dev_out.get(),
                         dev_cnt.get(), dev_sq.get());
    }
    int32_t rc = launch_scan(e, d, &qscan, p.w, per_grid ? per_grid.get() : dev_out.get(),
                             per_grid ? nullptr : dev_cnt.get());
    if (rc != FDB_OK) return rc;
    if (p.is_topk)
      return fdb_launch_topk(e->stream, per_grid.get(), v, p.w, q->num_groups, p.k,
                             q->agg_id == AGG_TOPK ? 1 : 0, dev_out.get(), dev_cnt.get());
    if (p.is_quant)
      return fdb_launch_quantile_cells(e->stream, per_grid.get(), v, p.w,
                                       q->num_groups, q->param, dev_out.get());
    if (agg)
      return fdb_launch_group_reduce(e->stream, per_grid.get(), v, p.w, q->num_groups,
                                     q->agg_id, dev_out.get(), dev_cnt.get(), dev_sq.get());
    return FDB_OK;
  };

  int total_runs = warmup + iters;
  float ms_sum = 0;
  for (int it = 0; it < total_runs; it++) {
    bool timed = it >= warmup;
    if (timed) HIP_CHECK(hipEventRecord(ev0.get(), e->stream));
    if (int32_t rc = run_once()) return rc;
    if (timed) {
      HIP_CHECK(hipEventRecord(ev1.get(), e->stream));
      HIP_CHECK(hipEventSynchronize(ev1.get()));
      float ms;
      HIP_CHECK(hipEventElapsedTime(&ms, ev0.get(), ev1.get()));
      ms_sum += ms;
    }
  }
  if (agg && !p.is_topk && !p.is_quant) {
    int32_t rc = fdb_launch_agg_present(e->stream, dev_out.get(), dev_cnt.get(),
                                        dev_sq.get(), p.out_len, q->agg_id, p.partial);
    if (rc != FDB_OK) return rc;
  }
  bool overflow = false;
  if (fdb_window_sample_supported(q->func_id)) {
    if (int32_t rc = take_overflow(e, &overflow)) return rc;
  } else {
    HIP_CHECK(hipStreamSynchronize(e->stream));
  }
  if (overflow) return sample_overflow_error();
  HIP_CHECK(dev_out.fetch());
  HIP_CHECK(dev_cnt.fetch());
  if (avg_ms) *avg_ms = iters > 0 ? (double)ms_sum / iters : 0.0;
  return FDB_OK;
}

// a histogram query's caller outputs, each optional: [G × W × nb] bucket sums,
// [G × W] counts, max, min and the present grid of step present_id (FDB_HP_*)
struct HistOut {
  double *sums, *counts, *max, *min, *present;
  int32_t present_id;
};

static int32_t run_hist(fdb_engine_t* e, const fdb_dataset_t* d,
                        const fdb_query_t* q, int32_t nb, const HistOut& o,
                        int32_t out_on_device) {
  HIP_CHECK(hipSetDevice(e->device));
  WindowGrid w;
  if (int32_t rc = check_windows(q, "bad hist query params", &w)) return rc;
  if (q->num_groups <= 0) { fdb_set_error("bad hist query params"); return FDB_ERR_BADARG; }
  if (nb < 1 || nb > 64) { fdb_set_error("num_buckets must be 1..64"); return FDB_ERR_BADARG; }
  if (!d->has_hist) {
    fdb_set_error("not a histogram dataset");
    return FDB_ERR_BADARG;
  }
  int hfunc;
  switch (q->func_id) {
    case FDB_FN_HIST_RATE:     hfunc = H2_RATE; break;
    case FDB_FN_SUM_OVER_TIME: hfunc = H2_SUM; break;
    case FDB_FN_INCREASE:      hfunc = H2_INCREASE; break;
    case FDB_FN_LAST:          hfunc = H2_LAST; break;
    default:
      fdb_set_error("histogram queries support FDB_FN_HIST_RATE, "
                    "FDB_FN_INCREASE, FDB_FN_SUM_OVER_TIME and FDB_FN_LAST "
                    "(got %d)", q->func_id);
      return FDB_ERR_BADARG;
  }
  if (hfunc == H2_INCREASE && (o.max || o.min)) {
    // only Rate maps to RateAndMinMaxOverTime (RangeFunction.scala:383-385)
    fdb_set_error("FDB_FN_INCREASE on a histogram has no max/min outputs");
    return FDB_ERR_BADARG;
  }
  // a present step's arguments are checked before the scan runs; a mode that
  // reads max/min scans the companion columns whether or not the caller asked
  // for those grids
  const bool present = o.present != nullptr;
  const bool need_mm = present && fdb_hist_present_needs_mm(o.present_id);
  if (present)
    if (int32_t rc = fdb_hist_present_check(o.present_id, q->param, q->param2,
                                            d->has_mm != 0, nb))
      return rc;
  if (need_mm && hfunc == H2_INCREASE) {
    fdb_set_error("FDB_FN_INCREASE on a histogram has no max/min for present "
                  "id %d", o.present_id);
    return FDB_ERR_BADARG;
  }
  // the max and min grids come as a pair (the kernel takes both or neither),
  // whichever of the two the caller asked for
  const bool scan_mm = o.max || o.min || need_mm;
  if (scan_mm && !d->has_mm) {
    fdb_set_error("dataset has no max/min companion columns "
                  "(fdb_series_append_hist_mm)");
    return FDB_ERR_BADARG;
  }
  if (d->max_group >= q->num_groups) { fdb_set_error("num_groups too small"); return FDB_ERR_BADARG; }
  const size_t cells = (size_t)q->num_groups * w.n;

  OutBuf dev_sums(o.sums, out_on_device, cells * nb), dev_cnt(o.counts, out_on_device, cells),
      dev_max(o.max, out_on_device, cells), dev_min(o.min, out_on_device, cells),
      dev_present(o.present, out_on_device, cells);
  if (!dev_sums.alloc() || !dev_cnt.alloc() || (present && !dev_present.alloc()) ||
      (scan_mm && (!dev_max.alloc() || !dev_min.alloc())))
    return alloc_failed("hist query");
  HIP_CHECK(hipMemsetAsync(dev_sums.get(), 0, cells * nb * 8, e->stream));
  HIP_CHECK(hipMemsetAsync(dev_cnt.get(), 0, cells * 8, e->stream));
  if (scan_mm) {    // NaN start for the maxIgnoreNaN/minIgnoreNaN merges
    HIP_CHECK(hipMemsetAsync(dev_max.get(), 0xFF, cells * 8, e->stream));
    HIP_CHECK(hipMemsetAsync(dev_min.get(), 0xFF, cells * 8, e->stream));
  }

  int32_t rc = fdb_launch_hist2(e->stream, view_of(d), w, nb, hfunc, dev_sums.get(),
                                dev_cnt.get(), dev_max.get(), dev_min.get());
  if (rc != FDB_OK) return rc;
  if (present) {
    rc = fdb_launch_hist_present(e->stream, dev_sums.get(), dev_cnt.get(),
                                 need_mm ? dev_max.get() : nullptr,
                                 need_mm ? dev_min.get() : nullptr,
                                 dev_present.get(), cells, nb, o.present_id,
                                 q->param, q->param2, d->hist_scheme[0],
                                 d->hist_scheme[1]);
    if (rc != FDB_OK) return rc;
  }
  HIP_CHECK(hipStreamSynchronize(e->stream));
  for (const OutBuf* g : {&dev_sums, &dev_cnt, &dev_max, &dev_min, &dev_present})
    HIP_CHECK(g->fetch());
  return FDB_OK;
}

// out_quantile is the plain-quantile present step with p0 = q->param
extern "C" int32_t fdb_query_exec_hist(fdb_engine_t* e, const fdb_dataset_t* d,
                                       const fdb_query_t* q, int32_t nb,
                                       double* out_bucket_sums, double* out_counts,
                                       double* out_quantile, int32_t out_on_device) {
  return run_hist(e, d, q, nb, HistOut{out_bucket_sums, out_counts, nullptr, nullptr,
                                       out_quantile, FDB_HP_QUANTILE}, out_on_device);
}

// histogram query with otel max/min companion outputs [G × W]
// (SumAndMaxOverTimeFuncHD / CumulativeHistRateAndMinMaxFunction,
//  AggrOverTimeFunctions.scala:612-813; HistMaxMinSumAggregator merges)
extern "C" int32_t fdb_query_exec_hist_mm(fdb_engine_t* e, const fdb_dataset_t* d,
                                          const fdb_query_t* q, int32_t nb,
                                          double* out_bucket_sums, double* out_counts,
                                          double* out_max, double* out_min,
                                          double* out_quantile, int32_t out_on_device) {
  return run_hist(e, d, q, nb, HistOut{out_bucket_sums, out_counts, out_max, out_min,
                                       out_quantile, FDB_HP_QUANTILE}, out_on_device);
}

// scan plus present step (FDB_HP_*) in one call: p0 = q->param, p1 = q->param2,
// the scheme the dataset's own
extern "C" int32_t fdb_query_exec_hist_present(
    fdb_engine_t* e, const fdb_dataset_t* d, const fdb_query_t* q, int32_t nb,
    int32_t present_id, double* out_bucket_sums, double* out_counts,
    double* out_max, double* out_min, double* out_present,
    int32_t out_on_device) {
  if (!out_present) {
    fdb_set_error("fdb_query_exec_hist_present: out_present is NULL");
    return FDB_ERR_BADARG;
  }
  return run_hist(e, d, q, nb, HistOut{out_bucket_sums, out_counts, out_max, out_min,
                                       out_present, present_id}, out_on_device);
}

// standalone presenter over caller grids (host or device pointers): what a
// multi-GPU caller runs after all-reducing the bucket sums
extern "C" int32_t fdb_hist_present(
    fdb_engine_t* e, int32_t present_id, double p0, double p1,
    const double* bucket_sums, const double* counts, const double* maxs,
    const double* mins, int64_t cells, int32_t nb, double bucket_first,
    double bucket_mult, double* out, int32_t on_device) {
  HIP_CHECK(hipSetDevice(e->device));
  if (!bucket_sums || !counts || !out || cells < 1) {
    fdb_set_error("fdb_hist_present: bucket_sums, counts and out are "
                  "required and cells must be >= 1");
    return FDB_ERR_BADARG;
  }
  if (int32_t rc = fdb_hist_present_check(present_id, p0, p1, maxs && mins, nb))
    return rc;
  const bool need_mm = fdb_hist_present_needs_mm(present_id);
  const size_t n = (size_t)cells;
  DevBuf dsum, dcnt, dmax, dmin;
  OutBuf dout(out, on_device, n);
  if (on_device) {
    dsum.wrap(const_cast<double*>(bucket_sums));
    dcnt.wrap(const_cast<double*>(counts));
    if (need_mm) { dmax.wrap(const_cast<double*>(maxs)); dmin.wrap(const_cast<double*>(mins)); }
  } else {
    if (!dsum.alloc(n * nb * 8) || !dcnt.alloc(n * 8) || !dout.alloc() ||
        (need_mm && (!dmax.alloc(n * 8) || !dmin.alloc(n * 8))))
      return alloc_failed("hist present");
    HIP_CHECK(hipMemcpyAsync(dsum.get(), bucket_sums, n * nb * 8, hipMemcpyHostToDevice, e->stream));
    HIP_CHECK(hipMemcpyAsync(dcnt.get(), counts, n * 8, hipMemcpyHostToDevice, e->stream));
    if (need_mm) {
      HIP_CHECK(hipMemcpyAsync(dmax.get(), maxs, n * 8, hipMemcpyHostToDevice, e->stream));
      HIP_CHECK(hipMemcpyAsync(dmin.get(), mins, n * 8, hipMemcpyHostToDevice, e->stream));
    }
  }
  int32_t rc = fdb_launch_hist_present(e->stream, dsum.get(), dcnt.get(),
                                       dmax.get(), dmin.get(), dout.get(), n,
                                       nb, present_id, p0, p1, bucket_first,
                                       bucket_mult);
  if (rc != FDB_OK) return rc;
  HIP_CHECK(hipStreamSynchronize(e->stream));
  HIP_CHECK(dout.fetch());
  return FDB_OK;
}

extern "C" int32_t fdb_query_exec(fdb_engine_t* e, const fdb_dataset_t* d, const fdb_query_t* q,
                                  double* out, double* out_counts, int32_t out_on_device) {
  return run_query(e, d, q, out, out_counts, out_on_device, 0, 1, nullptr);
}

// Downsample avg: AvgWithSumAndCountOverTimeFuncD (AggrOverTimeFunctions.
// scala:820-860) — per window, SumOverTime of the sum column divided by
// SumOverTime of the count column (plain IEEE division, each column with the
// NaN-poison sum semantics). The count column rides the dataset's max_off
// slots, so the second pass is the SAME fast scan with the directory's value
// offsets swapped — no new scan code.
extern "C" int32_t fdb_query_exec_avg_sc(fdb_engine_t* e, const fdb_dataset_t* d,
                                         const fdb_query_t* q, double* out,
                                         int32_t out_on_device) {
  HIP_CHECK(hipSetDevice(e->device));
  if (!d->has_sc) {
    fdb_set_error("dataset has no count columns (fdb_series_append_sc)");
    return FDB_ERR_BADARG;
  }
  WindowGrid w;
  if (int32_t rc = check_windows(q, "bad window params", &w)) return rc;
  if (q->agg_id != AGG_NONE) {
    fdb_set_error("avg_sc emits the [series x windows] grid only");
    return FDB_ERR_BADARG;
  }
  fdb_query_t q2 = *q;
  q2.func_id = FDB_FN_SUM_OVER_TIME;
  if (!fast_eligible(d, &q2)) {
    fdb_set_error("avg_sc needs a fast-eligible dataset (single-chunk "
                  "series, spans inside i32 ms)");
    return FDB_ERR_BADARG;
  }
  const size_t cells = (size_t)d->num_series * (size_t)w.n;
  DevBuf dsum, dcnt;
  OutBuf dout(out, out_on_device, cells);
  if (!dsum.alloc(cells * 8) || !dcnt.alloc(cells * 8) || !dout.alloc())
    return alloc_failed("avg_sc");
  int32_t rc = launch_scan(e, d, &q2, w, dsum.get(), nullptr);
  if (rc != FDB_OK) return rc;
  rc = launch_scan(e, d, &q2, w, dcnt.get(), nullptr, /*count_col=*/true);
  if (rc != FDB_OK) return rc;
  rc = fdb_launch_avg_div(e->stream, dout.get(), dsum.get(), dcnt.get(), cells);
  if (rc != FDB_OK) return rc;
  HIP_CHECK(hipStreamSynchronize(e->stream));
  HIP_CHECK(dout.fetch());
  return FDB_OK;
}

// count_values cross-series aggregation (CountValuesRowAggregator.scala):
// per (group, window) the distinct non-NaN values with frequencies, sorted
// ascending; more than k_cap distinct values in any cell is an error (the
// reference throws at its 1000-value limit). Host-memory outputs:
//   out_vals/out_cnts: [num_groups × num_windows × k_cap]
//   out_n:             [num_groups × num_windows]
extern "C" int32_t fdb_query_exec_count_values(
    fdb_engine_t* e, const fdb_dataset_t* d, const fdb_query_t* q,
    int32_t k_cap, double* out_vals, double* out_cnts, int32_t* out_n) {
  HIP_CHECK(hipSetDevice(e->device));
  if (d->has_hist) { fdb_set_error("histogram dataset"); return FDB_ERR_BADARG; }
  WindowGrid w;
  if (int32_t rc = check_windows(q, "bad count_values query params", &w)) return rc;
  if (q->num_groups <= 0 || d->max_group >= q->num_groups) {
    fdb_set_error("bad count_values query params");
    return FDB_ERR_BADARG;
  }
  const size_t cells = (size_t)q->num_groups * w.n;
  DevBuf per_grid;
  OutBuf dv(out_vals, false, cells * (size_t)k_cap), dc(out_cnts, false, cells * (size_t)k_cap);
  OutGrid<int32_t> dn(out_n, false, cells);
  fdb_query_t qscan = *q;
  qscan.agg_id = AGG_NONE;
  if (!per_grid.alloc((size_t)d->num_series * w.n * 8) ||
      !dv.alloc() || !dc.alloc() || !dn.alloc())
    return alloc_failed("count_values");
  int32_t rc = launch_scan(e, d, &qscan, w, per_grid.get(), nullptr);
  if (rc != FDB_OK) return rc;
  // the sample kernels raise the same flag as the presenter below: ask now
  bool overflow = false;
  if (fdb_window_sample_supported(q->func_id))
    if ((rc = take_overflow(e, &overflow)) != FDB_OK) return rc;
  if (overflow) return sample_overflow_error();
  rc = fdb_launch_count_values(e->stream, per_grid.get(), view_of(d), w, q->num_groups,
                               k_cap, dv.get(), dc.get(), dn.get(), e->dev_flag);
  if (rc != FDB_OK) return rc;
  if ((rc = take_overflow(e, &overflow)) != FDB_OK) return rc;
  if (overflow) {
    fdb_set_error("count_values: a cell exceeded %d distinct values "
                  "(the reference throws at its 1000-value limit)", k_cap);
    return FDB_ERR;
  }
  HIP_CHECK(dv.fetch());
  HIP_CHECK(dc.fetch());
  HIP_CHECK(dn.fetch());
  return FDB_OK;
}

extern "C" int32_t fdb_query_bench(fdb_engine_t* e, const fdb_dataset_t* d, const fdb_query_t* q,
                                   double* out, double* out_counts, int32_t out_on_device,
                                   int32_t warmup, int32_t iters, double* avg_kernel_ms) {
  return run_query(e, d, q, out, out_counts, out_on_device, warmup, iters, avg_kernel_ms);
}
