// Declarations shared by the library's translation units and by nothing
// outside csrc/: the error sink, the engine's stream accessor, the HIP error
// macros, owning wrappers for device memory, output grids and events, the
// dataset view and window grid, and every kernel launcher's prototype. Each defining file includes this header, so a
// signature that drifts from its declaration is a compile error.
#ifndef FDB_ENGINE_INTERNAL_H
#define FDB_ENGINE_INTERNAL_H

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>

#include "chunk_format.h"
#include "scan_common.h"
#include "window_funcs.h"
#include "../../include/filodb_amd.h"

void fdb_set_error(const char* fmt, ...);         // chunk_builder.cpp
hipStream_t fdb_engine_stream(fdb_engine_t* e);   // engine.hip

#define HIP_CHECK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
  fdb_set_error("%s failed: %s", #expr, hipGetErrorString(_e)); return FDB_ERR; } } while (0)
#define HIP_CHECK_NULL(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { \
  fdb_set_error("%s failed: %s", #expr, hipGetErrorString(_e)); return nullptr; } } while (0)

// after a kernel launch: the launch error, if any, named after the kernel
inline int32_t fdb_launched(const char* kernel) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fdb_set_error("%s launch failed: %s", kernel, hipGetErrorString(e));
    return FDB_ERR;
  }
  return FDB_OK;
}

// integer knob from the environment, read afresh at every call: the tests flip
// these between two queries of one process
inline int fdb_env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

// Device buffer that is freed on every exit of the scope that holds it. It
// either owns an allocation (alloc) or wraps memory that belongs to someone
// else (wrap: a caller's device output, or a slice of another buffer) and then
// frees nothing.
template <typename T>
class DevPtr {
 public:
  DevPtr() = default;
  DevPtr(const DevPtr&) = delete;
  DevPtr& operator=(const DevPtr&) = delete;
  DevPtr(DevPtr&& o) noexcept : p_(o.p_), owned_(o.owned_) { o.p_ = nullptr; o.owned_ = false; }
  DevPtr& operator=(DevPtr&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; owned_ = o.owned_; o.p_ = nullptr; o.owned_ = false; }
    return *this;
  }
  ~DevPtr() { reset(); }

  bool alloc(size_t bytes) {
    reset();
    if (hipMalloc((void**)&p_, bytes) != hipSuccess) { p_ = nullptr; return false; }
    owned_ = true;
    return true;
  }
  // allocates count elements plus tail_pad_bytes zeroed bytes and copies src
  // in; zero bytes still allocates 8, so an empty table has a real address
  bool upload(const T* src, size_t count, size_t tail_pad_bytes = 0) {
    const size_t bytes = count * sizeof(T), total = bytes + tail_pad_bytes;
    if (!alloc(total ? total : 8)) return false;
    if (tail_pad_bytes &&
        hipMemset((char*)p_ + bytes, 0, tail_pad_bytes) != hipSuccess) return false;
    return hipMemcpy(p_, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
  }
  void wrap(T* p) { reset(); p_ = p; }
  void reset() {
    if (owned_) (void)hipFree(p_);
    p_ = nullptr; owned_ = false;
  }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
  bool owned_ = false;
};
using DevBuf = DevPtr<double>;

// One output grid of n elements that a caller passed as `user`: the caller's
// own device memory when on_device, else a device buffer of ours that fetch()
// copies back to the host pointer. A null `user` is a grid the call needs but
// the caller did not ask for. alloc() is separate so that an optional grid
// costs nothing until the entry point decides it exists.
template <typename T>
class OutGrid {
 public:
  OutGrid(T* user, bool on_device, size_t n)
      : user_(on_device ? nullptr : user), n_(n) { if (on_device) dev_.wrap(user); }
  bool alloc() { return dev_ || dev_.alloc(n_ * sizeof(T)); }
  T* get() const { return dev_.get(); }
  explicit operator bool() const { return (bool)dev_; }
  hipError_t fetch() const {
    if (!user_ || !dev_) return hipSuccess;
    return hipMemcpy(user_, dev_.get(), n_ * sizeof(T), hipMemcpyDeviceToHost);
  }

 private:
  DevPtr<T> dev_;
  T* user_;      // host destination of fetch(), null when there is none
  size_t n_;
};
using OutBuf = OutGrid<double>;

// hipEvent_t destroyed on scope exit
class DevEvent {
 public:
  DevEvent() = default;
  DevEvent(const DevEvent&) = delete;
  DevEvent& operator=(const DevEvent&) = delete;
  ~DevEvent() { if (ev_) (void)hipEventDestroy(ev_); }
  hipError_t create() { return hipEventCreate(&ev_); }
  hipEvent_t get() const { return ev_; }

 private:
  hipEvent_t ev_ = nullptr;
};

// range functions the two scan kernels (scan_fast.hip's single-chunk fast path
// and scan_stream.hip's summary walk) both implement; each launcher rejects
// anything else itself
inline bool fdb_scan_supported(int func_id) {
  switch (func_id) {
    case FN_RATE: case FN_INCREASE: case FN_DELTA:
    case FN_SUM: case FN_COUNT: case FN_AVG: case FN_RATE_OVER_DELTA:
    case FN_MIN: case FN_MAX: case FN_STDDEV: case FN_STDVAR:
    case FN_CHANGES: case FN_LAST: case FN_PRESENT: case FN_TIMESTAMP:
    case FN_ZSCORE:
    case FN_IRATE: case FN_IDELTA: case FN_RESETS:
      return true;
    default:
      return false;
  }
}

// What the kernels read of an uploaded dataset (device pointers) and a query's
// window grid. Host-side only: every launcher unpacks them into its kernel's
// own arguments.
struct DatasetView {
  const uint8_t* blob;
  DirSoA dir;
  const uint64_t *max_off, *min_off;   // hist companion columns (0 = absent)
  const int32_t *series_first, *series_nchunks, *group_ids;
  const int32_t *sbg, *goff;           // group-sorted series index
  int num_series;
};
struct WindowGrid { int64_t start, step, end, window; int n; };

// scan_fast.hip: single-chunk-per-series fast path
struct FdbFastDesc;   // fast_desc.h: one decode descriptor per series
#define FDB_FAST_SAMPLE 256   // host-side descriptor sample kept per dataset
int32_t fdb_launch_fast_scan(hipStream_t stream, const DatasetView& v,
                             const FdbFastDesc* desc,
                             const FdbFastDesc* sample, int nsample,   // host
                             const WindowGrid& w, int func_id, int agg_id,
                             int emit_group, double* out, double* out_cnt,
                             double* out_sq, int phase_mask);

// scan_stream.hip: unbounded multi-chunk general path (chunk summaries +
// per-window walk)
int32_t fdb_launch_summaries(hipStream_t stream, const uint8_t* blob, DirSoA dir,
                             int64_t num_chunks, void* sums);
int64_t fdb_chunksum_bytes(int64_t num_chunks);
int32_t fdb_launch_stream_walk(hipStream_t stream, const DatasetView& v,
                               const void* sums, const WindowGrid& w,
                               int func_id, double* out);

// window_sample.hip: per-(series,window) sample-buffer functions (FN 16-18,
// holt_winters, deriv)
bool fdb_window_sample_supported(int func_id);
int32_t fdb_launch_window_sample(hipStream_t stream, const DatasetView& v,
                                 const WindowGrid& w, int func_id, double param,
                                 double param2, double* out, int32_t* overflow);

// hist2.hip: two-cursor histogram walk (unbounded chunks / window ratio).
// hfunc is the walk's window function.
enum { H2_RATE = 0, H2_SUM = 1, H2_INCREASE = 2, H2_LAST = 3 };
int32_t fdb_launch_hist2(hipStream_t stream, const DatasetView& v,
                         const WindowGrid& w, int nb, int hfunc,
                         double* out_sums, double* out_cnt,
                         double* out_max, double* out_min);

// agg_extra.hip: presenters over the per-series [S×W] grid (folded along the
// view's group-sorted index into ng groups) or the [G×W] aggregate grids
int32_t fdb_launch_group_reduce(hipStream_t stream, const double* grid,
                                const DatasetView& v, const WindowGrid& w,
                                int ng, int agg_id,
                                double* out, double* cnt, double* sq);
int32_t fdb_launch_topk(hipStream_t stream, const double* grid,
                        const DatasetView& v, const WindowGrid& w,
                        int ng, int k, int top, double* out, double* ids);
int32_t fdb_launch_agg_present(hipStream_t stream, double* out,
                               const double* cnt, const double* sq,
                               size_t n, int agg_id, int partial);
// histogram present step over [cells × nb] sums (FDB_HP_*; maxs/mins nullable).
// The launcher runs fdb_hist_present_check itself; an entry point that scans
// first calls it before the scan.
bool fdb_hist_present_needs_mm(int present_id);
int32_t fdb_hist_present_check(int present_id, double p0, double p1,
                               bool have_mm, int nb);
int32_t fdb_launch_hist_present(hipStream_t stream, const double* sums,
                                const double* cnt, const double* maxs,
                                const double* mins, double* out, size_t cells,
                                int nb, int present_id, double p0, double p1,
                                double first, double mult);
int32_t fdb_launch_avg_div(hipStream_t stream, double* out, const double* a,
                           const double* b, size_t n);
int32_t fdb_launch_quantile_cells(hipStream_t stream, const double* grid,
                                  const DatasetView& v, const WindowGrid& w,
                                  int ng, double q, double* out);
int32_t fdb_launch_count_values(hipStream_t stream, const double* grid,
                                const DatasetView& v, const WindowGrid& w,
                                int ng, int k_cap,
                                double* out_vals, double* out_cnts,
                                int32_t* out_n, int32_t* overflow);

#endif  // FDB_ENGINE_INTERNAL_H
