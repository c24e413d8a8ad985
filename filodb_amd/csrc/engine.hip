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

struct fdb_dataset {
  uint8_t* blob;
  uint64_t *ts_off, *val_off;
  int64_t *start_time, *end_time;
  int32_t *num_rows;
  int32_t *series_first, *series_nchunks, *group_ids;
  int32_t *series_by_group, *group_offsets;   // group-sorted series index (topk)
  int32_t num_series;
  int64_t num_chunks;
  int64_t payload_bytes;    // sum of vector bytes (algorithmic HBM footprint)
  int64_t total_samples;
  int max_group;            // max group id seen (for validation)
  int has_hist;             // dataset holds sect-delta histogram vectors
  int fast_ok;              // single-chunk series, chunk spans fit i32 ms
  void* sums;               // ChunkSum[num_chunks] for the streaming walk
  uint64_t *max_off, *min_off;  // hist companion column offsets (0 = absent)
  int has_mm;               // every hist chunk carries max/min columns
  int has_sc;               // every scalar chunk carries a count column
  // fast scan decode descriptors, one per series (fast_desc.h), built at
  // upload when fast_ok; fast_desc_sc describes the count column riding
  // max_off (has_sc) so avg_sc's second scan takes the same kernel
  FdbFastDesc *fast_desc, *fast_desc_sc;
  // host copies of up to FDB_FAST_SAMPLE evenly spaced descriptors per table:
  // the launcher runs the aligned-rows test on them with the query at hand
  // and picks the kernel build by the share that passes (scan_fast.hip)
  FdbFastDesc fast_sample[2][FDB_FAST_SAMPLE];
  int fast_nsample;
};

// the dataset's chunk directory as the kernels take it; count_col swaps the
// value column for the count column riding max_off (avg_sc)
static DirSoA dir_of(const fdb_dataset_t* d, bool count_col = false) {
  return DirSoA{d->ts_off, count_col ? d->max_off : d->val_off,
                d->start_time, d->end_time, d->num_rows};
}

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

extern "C" void fdb_dataset_destroy(fdb_dataset_t* d) {
  if (!d) return;
  (void)hipFree(d->blob); (void)hipFree(d->ts_off); (void)hipFree(d->val_off);
  (void)hipFree(d->start_time); (void)hipFree(d->end_time); (void)hipFree(d->num_rows);
  (void)hipFree(d->series_first); (void)hipFree(d->series_nchunks); (void)hipFree(d->group_ids);
  (void)hipFree(d->series_by_group); (void)hipFree(d->group_offsets);
  (void)hipFree(d->sums);
  (void)hipFree(d->max_off); (void)hipFree(d->min_off);
  (void)hipFree(d->fast_desc); (void)hipFree(d->fast_desc_sc);
  delete d;
}

extern "C" int64_t fdb_dataset_bytes(const fdb_dataset_t* d) { return d->payload_bytes; }
extern "C" int64_t fdb_dataset_samples(const fdb_dataset_t* d) { return d->total_samples; }

extern "C" fdb_dataset_t* fdb_dataset_upload(fdb_engine_t* e, const fdb_store_t* s) {
  fdb_view_t view;
  if (fdb_store_view(s, &view) != FDB_OK) return nullptr;
  HIP_CHECK_NULL(hipSetDevice(e->device));

  const fdb_dir_entry_t* dir = (const fdb_dir_entry_t*)view.dir;
  int64_t nc = view.num_chunks;

  // SoA host staging
  std::vector<uint64_t> ts_off(nc), val_off(nc), mx_off(nc), mn_off(nc);
  std::vector<int64_t> st(nc), en(nc);
  std::vector<int32_t> nr(nc);
  int64_t payload = 0, samples = 0;
  int all_mm = 1, any_mm = 0;
  for (int64_t i = 0; i < nc; i++) {
    ts_off[i] = dir[i].ts_off; val_off[i] = dir[i].val_off;
    mx_off[i] = dir[i].max_off; mn_off[i] = dir[i].min_off;
    if (dir[i].max_off) any_mm = 1; else all_mm = 0;
    st[i] = dir[i].start_time; en[i] = dir[i].end_time; nr[i] = dir[i].num_rows;
    uint32_t tl, vl;
    memcpy(&tl, view.blob + dir[i].ts_off, 4);
    memcpy(&vl, view.blob + dir[i].val_off, 4);
    payload += (int64_t)tl + 4 + (int64_t)vl + 4;
    if (dir[i].max_off) {
      uint32_t xl, nl;
      memcpy(&xl, view.blob + dir[i].max_off, 4);
      memcpy(&nl, view.blob + dir[i].min_off, 4);
      payload += (int64_t)xl + 4 + (int64_t)nl + 4;
    }
    samples += dir[i].num_rows;
  }
  int max_group = 0, max_chunks = 0, max_chunk_rows = 0;
  int has_hist = 0, has_scalar = 0, spans_fit_i32 = 1;
  for (int64_t i2 = 0; i2 < nc; i2++) {
    uint16_t wf;
    memcpy(&wf, view.blob + dir[i2].val_off + 4, 2);
    if (wf == FDB_WF_HIST_SECTDELTA) has_hist = 1; else has_scalar = 1;
    if (dir[i2].num_rows > max_chunk_rows) max_chunk_rows = dir[i2].num_rows;
    if (dir[i2].end_time - dir[i2].start_time >= (int64_t)1 << 31) spans_fit_i32 = 0;
  }
  if (has_hist && has_scalar) {
    fdb_set_error("mixed histogram and scalar series in one store are not "
                  "supported — upload them as separate datasets");
    return nullptr;
  }
  for (int32_t sid = 0; sid < view.num_series; sid++) {
    if (view.group_ids[sid] > max_group) max_group = view.group_ids[sid];
    if (view.series_nchunks[sid] > max_chunks) max_chunks = view.series_nchunks[sid];
  }
  if (max_chunk_rows > FDB_DEFAULT_MAX_ROWS) {
    fdb_set_error("chunk has %d rows; the reference's chunk cap is %d "
                  "(filodb-defaults.conf:835)", max_chunk_rows,
                  FDB_DEFAULT_MAX_ROWS);
    return nullptr;
  }

  auto* d = new fdb_dataset();
  memset(d, 0, sizeof(*d));
  d->num_series = view.num_series;
  d->num_chunks = nc;
  d->payload_bytes = payload;
  d->total_samples = samples;
  d->max_group = max_group;
  d->has_hist = has_hist;
  d->fast_ok = !has_hist && max_chunks <= 1 &&
               max_chunk_rows <= FDB_DEFAULT_MAX_ROWS && spans_fit_i32;
  d->has_mm = has_hist && any_mm && all_mm;
  d->has_sc = has_scalar && any_mm && all_mm;   // count column rides max_off

  auto upload = [&](void** dst, const void* src, size_t bytes) -> bool {
    if (hipMalloc(dst, bytes ? bytes : 8) != hipSuccess) return false;
    return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  // group-sorted series index for the top/bottom-k presenter: stable ascending
  // series order per group (ties then resolve identically to the oracle's fold)
  std::vector<int32_t> goff((size_t)max_group + 2, 0);
  for (int32_t s2 = 0; s2 < view.num_series; s2++) goff[(size_t)view.group_ids[s2] + 1]++;
  for (size_t g = 1; g < goff.size(); g++) goff[g] += goff[g - 1];
  std::vector<int32_t> sbg((size_t)view.num_series);
  {
    std::vector<int32_t> cur(goff.begin(), goff.end() - 1);
    for (int32_t s2 = 0; s2 < view.num_series; s2++)
      sbg[(size_t)cur[(size_t)view.group_ids[s2]]++] = s2;
  }

  // +512 B tail pad: the hist walk's wave-staged element reads may extend up
  // to 256 B past the last element's start, and its linear stage PREFETCH one
  // further 256-B window beyond that
  auto upload_pad = [&](void** dst, const void* src, size_t bytes) -> bool {
    if (hipMalloc(dst, bytes + 512) != hipSuccess) return false;
    if (hipMemset((char*)*dst + bytes, 0, 512) != hipSuccess) return false;
    return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  bool ok = upload_pad((void**)&d->blob, view.blob, (size_t)view.blob_len)
    && upload((void**)&d->ts_off, ts_off.data(), nc * 8)
    && upload((void**)&d->val_off, val_off.data(), nc * 8)
    && upload((void**)&d->start_time, st.data(), nc * 8)
    && upload((void**)&d->end_time, en.data(), nc * 8)
    && upload((void**)&d->num_rows, nr.data(), nc * 4)
    && upload((void**)&d->series_first, view.series_first, (size_t)view.num_series * 4)
    && upload((void**)&d->series_nchunks, view.series_nchunks, (size_t)view.num_series * 4)
    && upload((void**)&d->group_ids, view.group_ids, (size_t)view.num_series * 4)
    && upload((void**)&d->series_by_group, sbg.data(), sbg.size() * 4)
    && upload((void**)&d->group_offsets, goff.data(), goff.size() * 4)
    && upload((void**)&d->max_off, mx_off.data(), nc * 8)
    && upload((void**)&d->min_off, mn_off.data(), nc * 8);
  // fast scan descriptors: every per-series fact the kernel needs before it
  // touches the payload, parsed once from the host blob (fast_desc.h). A
  // vector the record cannot address (not 64-B aligned, or past 2^38 B)
  // sends the dataset down the general path instead.
  if (ok && d->fast_ok) {
    const int32_t ns = view.num_series;
    for (int col = 0; col < (d->has_sc ? 2 : 1) && d->fast_ok; col++) {
      const std::vector<uint64_t>& voff = col ? mx_off : val_off;
      std::vector<FdbFastDesc> desc((size_t)ns);
      int addressable = 1;
      #pragma omp parallel for schedule(static) reduction(&:addressable)
      for (int32_t sid = 0; sid < ns; sid++) {
        const int32_t c = view.series_first[sid];
        const bool has = view.series_nchunks[sid] >= 1;
        if (has && (((ts_off[c] | voff[c]) & 63) != 0 ||
                    ((ts_off[c] | voff[c]) >> 38) != 0)) {
          addressable = 0;
          continue;
        }
        fdb_build_fast_desc(view.blob, has ? ts_off[c] : 0, has ? voff[c] : 0,
                            has ? nr[c] : 0, &desc[(size_t)sid]);
      }
      if (!addressable) { d->fast_ok = 0; break; }
      d->fast_nsample = ns < FDB_FAST_SAMPLE ? ns : FDB_FAST_SAMPLE;
      for (int k = 0; k < d->fast_nsample; k++)
        d->fast_sample[col][k] = desc[(size_t)((int64_t)k * ns / d->fast_nsample)];
      ok = upload((void**)(col ? &d->fast_desc_sc : &d->fast_desc), desc.data(),
                  desc.size() * sizeof(FdbFastDesc));
      if (!ok) break;
    }
  }
  if (!ok) {
    fdb_set_error("device upload failed (out of HBM?)");
    fdb_dataset_destroy(d);
    return nullptr;
  }
  // chunk summaries for the streaming walk (query-independent; skipped when
  // every series takes the single-chunk fast path; FDB_FAST=0 at upload keeps
  // them, so the same dataset can be walked by the general path for A/B runs)
  const char* fenv = getenv("FDB_FAST");
  const bool fast_off = fenv && atoi(fenv) == 0;
  if (has_scalar && (!d->fast_ok || fast_off)) {
    if (hipMalloc(&d->sums, (size_t)fdb_chunksum_bytes(nc)) != hipSuccess) {
      fdb_set_error("summary allocation failed (out of HBM?)");
      fdb_dataset_destroy(d);
      return nullptr;
    }
    if (fdb_launch_summaries(e->stream, d->blob, dir_of(d), nc, d->sums) != FDB_OK) {
      fdb_dataset_destroy(d);
      return nullptr;
    }
  }
  return d;
}

// the fast single-chunk kernel handles this (dataset, query) pair?
static bool fast_eligible(const fdb_dataset_t* d, const fdb_query_t* q) {
  const char* v = getenv("FDB_FAST");             // perf/parity experiments
  if (v && atoi(v) == 0) return false;
  return d->fast_ok && fdb_scan_supported(q->func_id) &&
         q->step > 0 && q->step < ((int64_t)1 << 31) && q->window >= 0;
}

static int32_t launch_scan(fdb_engine_t* e, const fdb_dataset_t* d, const fdb_query_t* q,
                           double* dev_out, double* dev_cnt, double* dev_sq,
                           bool count_col = false) {
  DirSoA dir = dir_of(d, count_col);
  int nw = fdb_num_windows(q);
  if (fast_eligible(d, q) && q->agg_id == AGG_NONE) {
    return fdb_launch_fast_scan(e->stream, d->blob,
                                count_col ? d->fast_desc_sc : d->fast_desc,
                                d->fast_sample[count_col ? 1 : 0], d->fast_nsample,
                                d->group_ids,
                                d->series_by_group, d->num_series,
                                q->start, q->step, q->window, nw,
                                q->func_id, AGG_NONE, /*emit_group=*/0,
                                dev_out, dev_cnt, dev_sq, q->_pad);
  }
  // sample-buffer functions (quantile/MAD/predict_linear) have their own
  // per-(series,window) kernel, on any dataset shape
  if (fdb_window_sample_supported(q->func_id)) {
    return fdb_launch_window_sample(e->stream, d->blob, dir, d->series_first,
                                    d->series_nchunks, d->num_series,
                                    q->start, q->step, q->window, nw,
                                    q->func_id, q->param, q->param2,
                                    dev_out, e->dev_flag);
  }
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
  (void)dev_cnt; (void)dev_sq;
  return fdb_launch_stream_walk(e->stream, d->blob, dir, d->sums,
                                d->series_first, d->series_nchunks,
                                d->num_series, q->start, q->step, q->end,
                                q->window, nw, q->func_id, dev_out);
}

// window-grid checks every query entry point shares; bad_nw is the entry
// point's own message for an empty or inverted window grid
static int32_t check_windows(const fdb_query_t* q, const char* bad_nw, int* nw) {
  *nw = fdb_num_windows(q);
  if (*nw <= 0) { fdb_set_error("%s", bad_nw); return FDB_ERR_BADARG; }
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

static int32_t run_query(fdb_engine_t* e, const fdb_dataset_t* d, const fdb_query_t* q,
                         double* out, double* out_counts, int32_t out_on_device,
                         int32_t warmup, int32_t iters, double* avg_ms) {
  HIP_CHECK(hipSetDevice(e->device));
  if (d->has_hist) {
    fdb_set_error("histogram dataset: use fdb_query_exec_hist");
    return FDB_ERR_BADARG;
  }
  int nw;
  if (int32_t rc = check_windows(q, "bad window params", &nw)) return rc;
  if (q->func_id == FDB_FN_HOLT_WINTERS &&
      !(q->param >= 0 && q->param <= 1 && q->param2 >= 0 && q->param2 <= 1)) {
    // parseParameters (AggrOverTimeFunctions.scala:1373-1382)
    fdb_set_error("holt_winters sf/tf must be in [0, 1]");
    return FDB_ERR_BADARG;
  }
  const bool is_topk = q->agg_id == AGG_TOPK || q->agg_id == AGG_BOTTOMK;
  const int kk = is_topk ? (int)q->param : 0;
  if (is_topk && (kk < 1 || kk > 16)) {
    fdb_set_error("topk k=%d out of range 1..16 (q.param)", kk);
    return FDB_ERR_BADARG;
  }
  size_t out_len = (q->agg_id == AGG_NONE) ? (size_t)d->num_series * nw
                 : is_topk ? (size_t)q->num_groups * nw * kk
                           : (size_t)q->num_groups * nw;
  if (q->agg_id != AGG_NONE) {
    if (q->num_groups <= 0 || d->max_group >= q->num_groups) {
      fdb_set_error("num_groups %d inconsistent with dataset max group %d",
                    q->num_groups, d->max_group);
      return FDB_ERR_BADARG;
    }
  }

  const bool needs_sq = q->agg_id == AGG_STDDEV || q->agg_id == AGG_STDVAR;
  int partial = (q->agg_id != AGG_NONE && !is_topk && out_counts != nullptr) ? 1 : 0;
  // stddev/stdvar partials ship (raw sums, raw sumsq) stacked: the caller's
  // `out` is [2 × G × W]; shards merge both halves + counts by addition —
  // algebraically StddevRowAggregator.scala:36-52's reduction
  size_t buf_len = (needs_sq && partial) ? out_len * 2 : out_len;

  // every exit (including the HIP_CHECK early returns) releases what this call
  // owns — device buffers and events must not leak on a failed launch
  DevBuf dev_out, dev_cnt, dev_sq, per_grid;
  DevEvent ev0, ev1;
  if (out_on_device) { dev_out.wrap(out); dev_cnt.wrap(out_counts); }
  if (!dev_out && !dev_out.alloc(buf_len * 8)) return alloc_failed("query");
  if (q->agg_id != AGG_NONE && !dev_cnt && !dev_cnt.alloc(out_len * 8))
    return alloc_failed("query");
  if (needs_sq) {
    if (partial) dev_sq.wrap(dev_out.get() + out_len);   // second half of the caller grid
    else if (!dev_sq.alloc(out_len * 8)) return alloc_failed("query");
  }
  HIP_CHECK(ev0.create());
  HIP_CHECK(ev1.create());

  // aggregated queries: the fused-group fast path folds fastReduce into the
  // scan (per-lane register partials + one atomic burst per group change) and
  // never materializes the [S×W] grid; other shapes run two-phase — the scan
  // fills an internal per-series grid with plain stores, then a presenter
  // (topk_kernel / group_reduce_kernel) folds it along the group-sorted index
  const bool is_quant = q->agg_id == AGG_QUANTILE;
  if (is_quant && out_counts) {
    fdb_set_error("quantile aggregation has no partial (multi-shard) mode — "
                  "digest shipping is not implemented");
    return FDB_ERR_BADARG;
  }
  // the fused-group emit (no [S×W] intermediate) measured ~6% SLOWER than
  // the two-phase reduce at current scan cost (3.20 vs 3.02 ms on configs[5];
  // the scan is compute-bound, so skipping the grid re-read does not pay
  // yet) — two-phase is the default, FDB_FUSED_GROUP=1 opts in
  const char* fe = getenv("FDB_FUSED_GROUP");
  const bool fused = (fe && atoi(fe) == 1) && !is_quant &&
                     q->agg_id != AGG_NONE && !is_topk &&
                     nw <= 256 && fast_eligible(d, q);
  fdb_query_t qscan = *q;
  if (q->agg_id != AGG_NONE && !fused) {
    if (!per_grid.alloc((size_t)d->num_series * nw * 8)) return alloc_failed("query");
    qscan.agg_id = AGG_NONE;
  }

  // one run of the query's launches: the fused scan, or scan + presenter
  auto run_once = [&]() -> int32_t {
    if (fused) {
      // atomically-accumulated grids: reset per launch. MIN/MAX start the
      // value grid at NaN (atomic_min_max_f64's empty-cell marker).
      const bool mm = q->agg_id == AGG_MIN || q->agg_id == AGG_MAX;
      HIP_CHECK(hipMemsetAsync(dev_out.get(), mm ? 0xFF : 0, buf_len * 8, e->stream));
      HIP_CHECK(hipMemsetAsync(dev_cnt.get(), 0, out_len * 8, e->stream));
      if (dev_sq && !(needs_sq && partial))
        HIP_CHECK(hipMemsetAsync(dev_sq.get(), 0, out_len * 8, e->stream));
      return fdb_launch_fast_scan(
          e->stream, d->blob, d->fast_desc, d->fast_sample[0], d->fast_nsample,
          d->group_ids, d->series_by_group, d->num_series,
          q->start, q->step, q->window, nw, q->func_id, q->agg_id,
          /*emit_group=*/1, dev_out.get(), dev_cnt.get(), dev_sq.get(), q->_pad);
    }
    int32_t rc = launch_scan(e, d, &qscan, per_grid ? per_grid.get() : dev_out.get(),
                             per_grid ? nullptr : dev_cnt.get(), nullptr);
    if (rc != FDB_OK) return rc;
    if (is_topk)
      return fdb_launch_topk(e->stream, per_grid.get(), d->series_by_group,
                             d->group_offsets, q->num_groups, nw, kk,
                             q->agg_id == AGG_TOPK ? 1 : 0,
                             dev_out.get(), dev_cnt.get());
    if (is_quant)
      return fdb_launch_quantile_cells(e->stream, per_grid.get(),
                                       d->series_by_group, d->group_offsets,
                                       q->num_groups, nw, q->param, dev_out.get());
    if (q->agg_id != AGG_NONE)
      return fdb_launch_group_reduce(e->stream, per_grid.get(),
                                     d->series_by_group, d->group_offsets,
                                     q->num_groups, nw, q->agg_id,
                                     dev_out.get(), dev_cnt.get(), dev_sq.get());
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
  if (q->agg_id != AGG_NONE && !is_topk && !is_quant) {
    int32_t rc = fdb_launch_agg_present(e->stream, dev_out.get(), dev_cnt.get(),
                                        dev_sq.get(), out_len, q->agg_id, partial);
    if (rc != FDB_OK) return rc;
  }
  HIP_CHECK(hipStreamSynchronize(e->stream));
  if (fdb_window_sample_supported(q->func_id)) {
    int32_t flag = 0;
    HIP_CHECK(hipMemcpy(&flag, e->dev_flag, 4, hipMemcpyDeviceToHost));
    if (flag) {
      (void)hipMemset(e->dev_flag, 0, 4);
      fdb_set_error("a window exceeded the %d-sample buffer of the "
                    "quantile/MAD kernel", 1024);
      return FDB_ERR;
    }
  }

  if (!out_on_device) {
    HIP_CHECK(hipMemcpy(out, dev_out.get(), buf_len * 8, hipMemcpyDeviceToHost));
    if (q->agg_id != AGG_NONE && out_counts)
      HIP_CHECK(hipMemcpy(out_counts, dev_cnt.get(), out_len * 8, hipMemcpyDeviceToHost));
  }
  if (avg_ms) *avg_ms = iters > 0 ? (double)ms_sum / iters : 0.0;
  return FDB_OK;
}

static int32_t run_hist(fdb_engine_t* e, const fdb_dataset_t* d,
                        const fdb_query_t* q, int32_t nb,
                        double* out_bucket_sums, double* out_counts,
                        double* out_max, double* out_min,
                        double* out_quantile, int32_t out_on_device,
                        int32_t present_id = -1, double* out_present = nullptr) {
  HIP_CHECK(hipSetDevice(e->device));
  int nw;
  if (int32_t rc = check_windows(q, "bad hist query params", &nw)) return rc;
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
  if (hfunc == H2_INCREASE && (out_max || out_min)) {
    // only Rate maps to RateAndMinMaxOverTime (RangeFunction.scala:383-385)
    fdb_set_error("FDB_FN_INCREASE on a histogram has no max/min outputs");
    return FDB_ERR_BADARG;
  }
  // a present step's arguments are checked before the scan runs; a mode that
  // reads max/min scans the companion columns whether or not the caller asked
  // for those grids
  const bool present = out_present != nullptr;
  const bool need_mm = present && fdb_hist_present_needs_mm(present_id);
  if (present)
    if (int32_t rc = fdb_hist_present_check(present_id, q->param, q->param2,
                                            d->has_mm != 0, nb))
      return rc;
  if (need_mm && hfunc == H2_INCREASE) {
    fdb_set_error("FDB_FN_INCREASE on a histogram has no max/min for present "
                  "id %d", present_id);
    return FDB_ERR_BADARG;
  }
  if ((out_max || out_min || need_mm) && !d->has_mm) {
    fdb_set_error("dataset has no max/min companion columns "
                  "(fdb_series_append_hist_mm)");
    return FDB_ERR_BADARG;
  }
  if (d->max_group >= q->num_groups) { fdb_set_error("num_groups too small"); return FDB_ERR_BADARG; }
  size_t cells = (size_t)q->num_groups * nw;

  // caller-provided device outputs are wrapped, everything else is owned and
  // released on every exit
  DevBuf dev_sums, dev_cnt, dev_quant, dev_max, dev_min, dev_present;
  if (out_on_device) {
    dev_sums.wrap(out_bucket_sums);
    dev_cnt.wrap(out_counts);
    dev_quant.wrap(out_quantile);
    dev_max.wrap(out_max); dev_min.wrap(out_min);
    dev_present.wrap(out_present);
  }
  if (!dev_sums && !dev_sums.alloc(cells * nb * 8)) return alloc_failed("hist query");
  if (!dev_cnt && !dev_cnt.alloc(cells * 8)) return alloc_failed("hist query");
  if (out_quantile && !dev_quant && !dev_quant.alloc(cells * 8))
    return alloc_failed("hist query");
  if (present && !dev_present && !dev_present.alloc(cells * 8))
    return alloc_failed("hist query");
  if (out_max && !dev_max &&
      (!dev_max.alloc(cells * 8) || !dev_min.alloc(cells * 8)))
    return alloc_failed("hist query");
  if (need_mm && ((!dev_max && !dev_max.alloc(cells * 8)) ||
                  (!dev_min && !dev_min.alloc(cells * 8))))
    return alloc_failed("hist query");
  HIP_CHECK(hipMemsetAsync(dev_sums.get(), 0, cells * nb * 8, e->stream));
  HIP_CHECK(hipMemsetAsync(dev_cnt.get(), 0, cells * 8, e->stream));
  if (dev_max) {    // NaN start for the maxIgnoreNaN/minIgnoreNaN merges
    HIP_CHECK(hipMemsetAsync(dev_max.get(), 0xFF, cells * 8, e->stream));
    HIP_CHECK(hipMemsetAsync(dev_min.get(), 0xFF, cells * 8, e->stream));
  }

  int32_t rc = fdb_launch_hist2(e->stream, d->blob, dir_of(d), d->max_off,
                                d->min_off, d->series_first,
                                d->series_nchunks, d->group_ids,
                                d->num_series, q->start, q->step, q->window,
                                nw, nb, hfunc, dev_sums.get(), dev_cnt.get(),
                                dev_max.get(), dev_min.get());
  if (rc != FDB_OK) return rc;

  if (out_quantile || present) {
    // bucket scheme (first, mult) from the first hist vector in the blob
    uint64_t voff0;
    HIP_CHECK(hipMemcpy(&voff0, d->val_off, 8, hipMemcpyDeviceToHost));
    double fm[2];
    HIP_CHECK(hipMemcpy(fm, d->blob + voff0 + FDB_HIST_OFF_DEF + 2, 16,
                        hipMemcpyDeviceToHost));
    if (out_quantile) {
      rc = fdb_launch_hist_quantile(e->stream, dev_sums.get(), dev_cnt.get(),
                                    dev_quant.get(), cells, nb, q->param,
                                    fm[0], fm[1]);
      if (rc != FDB_OK) return rc;
    }
    if (present) {
      rc = fdb_launch_hist_present(e->stream, dev_sums.get(), dev_cnt.get(),
                                   need_mm ? dev_max.get() : nullptr,
                                   need_mm ? dev_min.get() : nullptr,
                                   dev_present.get(), cells, nb, present_id,
                                   q->param, q->param2, fm[0], fm[1]);
      if (rc != FDB_OK) return rc;
    }
  }
  HIP_CHECK(hipStreamSynchronize(e->stream));
  if (!out_on_device) {
    if (out_bucket_sums)
      HIP_CHECK(hipMemcpy(out_bucket_sums, dev_sums.get(), cells * nb * 8, hipMemcpyDeviceToHost));
    if (out_counts)
      HIP_CHECK(hipMemcpy(out_counts, dev_cnt.get(), cells * 8, hipMemcpyDeviceToHost));
    if (out_quantile)
      HIP_CHECK(hipMemcpy(out_quantile, dev_quant.get(), cells * 8, hipMemcpyDeviceToHost));
    if (present)
      HIP_CHECK(hipMemcpy(out_present, dev_present.get(), cells * 8, hipMemcpyDeviceToHost));
    if (out_max && dev_max)
      HIP_CHECK(hipMemcpy(out_max, dev_max.get(), cells * 8, hipMemcpyDeviceToHost));
    if (out_min && dev_min)
      HIP_CHECK(hipMemcpy(out_min, dev_min.get(), cells * 8, hipMemcpyDeviceToHost));
  }
  return FDB_OK;
}

extern "C" int32_t fdb_query_exec_hist(fdb_engine_t* e, const fdb_dataset_t* d,
                                       const fdb_query_t* q, int32_t nb,
                                       double* out_bucket_sums, double* out_counts,
                                       double* out_quantile, int32_t out_on_device) {
  return run_hist(e, d, q, nb, out_bucket_sums, out_counts, nullptr, nullptr,
                  out_quantile, out_on_device);
}

// histogram query with otel max/min companion outputs [G × W]
// (SumAndMaxOverTimeFuncHD / CumulativeHistRateAndMinMaxFunction,
//  AggrOverTimeFunctions.scala:612-813; HistMaxMinSumAggregator merges)
extern "C" int32_t fdb_query_exec_hist_mm(fdb_engine_t* e, const fdb_dataset_t* d,
                                          const fdb_query_t* q, int32_t nb,
                                          double* out_bucket_sums, double* out_counts,
                                          double* out_max, double* out_min,
                                          double* out_quantile, int32_t out_on_device) {
  return run_hist(e, d, q, nb, out_bucket_sums, out_counts, out_max, out_min,
                  out_quantile, out_on_device);
}

// scan plus present step (FDB_HP_*) in one call: p0 = q->param, p1 = q->param2,
// the scheme read from the dataset
extern "C" int32_t fdb_query_exec_hist_present(
    fdb_engine_t* e, const fdb_dataset_t* d, const fdb_query_t* q, int32_t nb,
    int32_t present_id, double* out_bucket_sums, double* out_counts,
    double* out_max, double* out_min, double* out_present,
    int32_t out_on_device) {
  if (!out_present) {
    fdb_set_error("fdb_query_exec_hist_present: out_present is NULL");
    return FDB_ERR_BADARG;
  }
  return run_hist(e, d, q, nb, out_bucket_sums, out_counts, out_max, out_min,
                  nullptr, out_on_device, present_id, out_present);
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
  DevBuf dsum, dcnt, dmax, dmin, dout;
  if (on_device) {
    dsum.wrap(const_cast<double*>(bucket_sums));
    dcnt.wrap(const_cast<double*>(counts));
    if (need_mm) { dmax.wrap(const_cast<double*>(maxs)); dmin.wrap(const_cast<double*>(mins)); }
    dout.wrap(out);
  } else {
    if (!dsum.alloc(n * nb * 8) || !dcnt.alloc(n * 8) || !dout.alloc(n * 8) ||
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
  if (!on_device)
    HIP_CHECK(hipMemcpy(out, dout.get(), n * 8, hipMemcpyDeviceToHost));
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
  int nw;
  if (int32_t rc = check_windows(q, "bad window params", &nw)) return rc;
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
  const size_t cells = (size_t)d->num_series * (size_t)nw;
  DevBuf dsum, dcnt, dout;
  if (out_on_device) dout.wrap(out);
  if (!dsum.alloc(cells * 8) || !dcnt.alloc(cells * 8) ||
      (!out_on_device && !dout.alloc(cells * 8)))
    return alloc_failed("avg_sc");
  int32_t rc = launch_scan(e, d, &q2, dsum.get(), nullptr, nullptr);
  if (rc != FDB_OK) return rc;
  rc = launch_scan(e, d, &q2, dcnt.get(), nullptr, nullptr, /*count_col=*/true);
  if (rc != FDB_OK) return rc;
  rc = fdb_launch_avg_div(e->stream, dout.get(), dsum.get(), dcnt.get(), cells);
  if (rc != FDB_OK) return rc;
  HIP_CHECK(hipStreamSynchronize(e->stream));
  if (!out_on_device)
    HIP_CHECK(hipMemcpy(out, dout.get(), cells * 8, hipMemcpyDeviceToHost));
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
  int nw;
  if (int32_t rc = check_windows(q, "bad count_values query params", &nw)) return rc;
  if (q->num_groups <= 0 || d->max_group >= q->num_groups) {
    fdb_set_error("bad count_values query params");
    return FDB_ERR_BADARG;
  }
  size_t cells = (size_t)q->num_groups * nw;
  DevBuf per_grid, dv, dc;
  DevPtr<int32_t> dn;
  fdb_query_t qscan = *q;
  qscan.agg_id = AGG_NONE;
  if (!per_grid.alloc((size_t)d->num_series * nw * 8) ||
      !dv.alloc(cells * (size_t)k_cap * 8) ||
      !dc.alloc(cells * (size_t)k_cap * 8) || !dn.alloc(cells * 4))
    return alloc_failed("count_values");
  int32_t rc = launch_scan(e, d, &qscan, per_grid.get(), nullptr, nullptr);
  if (rc != FDB_OK) return rc;
  rc = fdb_launch_count_values(e->stream, per_grid.get(), d->series_by_group,
                               d->group_offsets, q->num_groups, nw, k_cap,
                               dv.get(), dc.get(), dn.get(), e->dev_flag);
  if (rc != FDB_OK) return rc;
  HIP_CHECK(hipStreamSynchronize(e->stream));
  int32_t flag = 0;
  (void)hipMemcpy(&flag, e->dev_flag, 4, hipMemcpyDeviceToHost);
  if (flag) {
    (void)hipMemset(e->dev_flag, 0, 4);
    fdb_set_error("count_values: a cell exceeded %d distinct values "
                  "(the reference throws at its 1000-value limit)", k_cap);
    return FDB_ERR;
  }
  HIP_CHECK(hipMemcpy(out_vals, dv.get(), cells * (size_t)k_cap * 8, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(out_cnts, dc.get(), cells * (size_t)k_cap * 8, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(out_n, dn.get(), cells * 4, hipMemcpyDeviceToHost));
  return FDB_OK;
}

extern "C" int32_t fdb_query_bench(fdb_engine_t* e, const fdb_dataset_t* d, const fdb_query_t* q,
                                   double* out, double* out_counts, int32_t out_on_device,
                                   int32_t warmup, int32_t iters, double* avg_kernel_ms) {
  return run_query(e, d, q, out, out_counts, out_on_device, warmup, iters, avg_kernel_ms);
}
