// Shared device-side pieces of the MI355X scan engine: frozen-vector readers,
// chunk decoders, wave scans and launch plumbing types (window_funcs.h has
// the range functions' per-window rules).
// Layouts: DESIGN.md §2 (bit-faithful to the reference's off-heap vectors).
#ifndef FDB_SCAN_COMMON_H
#define FDB_SCAN_COMMON_H

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <cmath>

#include "chunk_format.h"

// function / aggregation ids (include/filodb_amd.h; dispatch table
// RangeFunction.scala:294-410, aggregator/RowAggregator.scala)
enum { FN_RATE=0, FN_INCREASE=1, FN_DELTA=2, FN_SUM=3, FN_COUNT=4, FN_AVG=5,
       FN_MIN=6, FN_MAX=7, FN_STDDEV=8, FN_STDVAR=9, FN_CHANGES=10, FN_LAST=12,
       FN_PRESENT=13, FN_TIMESTAMP=14, FN_ZSCORE=15,
       FN_QUANTILE=16, FN_MAD=17, FN_PREDICT_LINEAR=18, FN_RATE_OVER_DELTA=19,
       FN_HOLT_WINTERS=20,
       // instant range functions (RangeFunction.scala:489-494,
       // RangeInstantFunctions.scala)
       FN_IRATE=21, FN_IDELTA=22, FN_RESETS=23, FN_DERIV=24 };
enum { AGG_NONE=0, AGG_SUM=1, AGG_COUNT=2, AGG_MIN=3, AGG_MAX=4, AGG_AVG=5,
       AGG_TOPK=6, AGG_BOTTOMK=7, AGG_STDDEV=8, AGG_STDVAR=9, AGG_GROUP=10,
       AGG_QUANTILE=11, AGG_COUNT_VALUES=12 };

struct DirSoA {
  const uint64_t* ts_off;
  const uint64_t* val_off;
  const int64_t*  start_time;
  const int64_t*  end_time;
  const int32_t*  num_rows;
};

__device__ __forceinline__ uint16_t d_u16(const uint8_t* p) { uint16_t v; memcpy(&v, p, 2); return v; }
__device__ __forceinline__ uint32_t d_u32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
__device__ __forceinline__ int32_t  d_i32(const uint8_t* p) { int32_t v; memcpy(&v, p, 4); return v; }
__device__ __forceinline__ int64_t  d_i64(const uint8_t* p) { int64_t v; memcpy(&v, p, 8); return v; }
__device__ __forceinline__ double   d_f64(const uint8_t* p) { double v; memcpy(&v, p, 8); return v; }

struct DVec {           // opened vector header
  const uint8_t* idata;
  int64_t init;
  int32_t slope;
  int n;
  uint16_t wf;
  uint8_t nbits, sign, dropped;
};

__device__ __forceinline__ int64_t d_inner_at(const DVec* v, int i) {
  switch (v->nbits) {
    case 32: return d_i32(v->idata + 4 * (size_t)i);
    case 16: { int32_t x = (int16_t)d_u16(v->idata + 2 * (size_t)i);
               return v->sign ? x : (x & 0xffff); }
    case 8:  { int32_t x = (int8_t)v->idata[i];
               return v->sign ? x : (x & 0xff); }
    case 4:  return (v->idata[i >> 1] >> ((i & 1) * 4)) & 0x0f;
    case 2:  return (v->idata[i >> 2] >> ((i & 3) * 2)) & 0x03;
  }
  return 0;
}

// wave-local LDS ordering only: s_waitcnt lgkmcnt(0) — unlike s_waitcnt(0)
// this does NOT drain vmcnt, so outstanding global loads/stores/atomics keep
// flying across the fence
__device__ __forceinline__ void d_wait_lds() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// the wave's LDS writes so far are visible to all of its lanes
__device__ __forceinline__ void d_lds_fence() {
  d_wait_lds();
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int64_t d_lv_at(const DVec* v, int i) {
  if (v->wf == FDB_WF_DDV) return v->init + (int64_t)v->slope * i + d_inner_at(v, i);
  if (v->wf == FDB_WF_DDV_CONST) return v->init + (int64_t)v->slope * i;
  return d_i64(v->idata + 8 * (size_t)i);
}

__device__ __forceinline__ double d_dv_at(const DVec* v, int i) {
  if (v->wf == FDB_WF_PRIM64) return d_f64(v->idata + 8 * (size_t)i);
  return (double)d_lv_at(v, i);
}

// first index in [0,n) with ts[i] >= item; n when none — interpolation guess
// + exact walk over the encoded vector (DeltaDeltaDataReader.binarySearch
// semantics for our lower-bound convention)
__device__ __forceinline__ int d_search_ge(const DVec& tv, int n, int64_t item,
                                           int64_t ts0, float inv_slope) {
  if (n <= 0) return 0;
  int g = (int)((float)(item - ts0) * inv_slope);
  if (g < 0) g = 0;
  if (g > n - 1) g = n - 1;
  while (g > 0 && d_lv_at(&tv, g - 1) >= item) g--;
  while (g < n && d_lv_at(&tv, g) < item) g++;
  return g;
}

// one-load header open: vectors are 64-B aligned in the device blob (padded
// tail), so a single 32-byte read covers every header field of all three
// scalar layouts — one round trip instead of the ~6 dependent global loads a
// field-by-field open costs. first_val (optional) returns element 0 (ts0 for a timestamp
// vector) parsed from the same 32 bytes.
__device__ __forceinline__ void d_vec_open_wide(const uint8_t* p, DVec* v,
                                                int64_t* first_val) {
  uint32_t h[8];
  memcpy(h, p, 32);
  const uint16_t wf = (uint16_t)(h[1] & 0xffff);
  v->wf = wf;
  v->dropped = ((h[1] >> 16) & FDB_DROP_MASK) != 0;
  if (wf == FDB_WF_DDV) {
    v->init = (int64_t)(((uint64_t)h[3] << 32) | h[2]);
    v->slope = (int32_t)h[4];
    const uint32_t w6 = h[6];                  // inner bytes 4..7
    v->nbits = (uint8_t)((w6 >> 16) & FDB_NBITS_MASK);
    v->sign = ((w6 >> 16) & FDB_SIGN_MASK) != 0;
    const int bitShift = (int)(w6 >> 24) & 0x3f;
    v->idata = p + FDB_DDV_OFF_INNER + FDB_PRIM_OFF_DATA;
    const int numBytes = (int)h[5];            // inner length word
    v->n = ((numBytes - 4) * 8 + (bitShift != 0 ? bitShift - 8 : 0)) / v->nbits;
    if (first_val) {
      int64_t in0;                             // inner element 0 is in h[7]
      switch (v->nbits) {
        case 32: in0 = (int32_t)h[7]; break;
        case 16: { int32_t x = (int16_t)(h[7] & 0xffff);
                   in0 = v->sign ? x : (x & 0xffff); } break;
        case 8:  { int32_t x = (int8_t)(h[7] & 0xff);
                   in0 = v->sign ? x : (x & 0xff); } break;
        case 4:  in0 = h[7] & 0x0f; break;
        default: in0 = h[7] & 0x03; break;
      }
      *first_val = v->init + in0;
    }
  } else if (wf == FDB_WF_DDV_CONST) {
    v->n = (int32_t)h[2];
    v->init = (int64_t)(((uint64_t)h[4] << 32) | h[3]);
    v->slope = (int32_t)h[5];
    v->idata = nullptr; v->nbits = 0; v->sign = 0;
    if (first_val) *first_val = v->init;
  } else {
    v->n = ((int)h[0] - 4) / 8;
    v->idata = p + FDB_PRIM_OFF_DATA;
    v->init = 0; v->slope = 0; v->nbits = 64; v->sign = 1;
    if (first_val) *first_val = (int64_t)(((uint64_t)h[3] << 32) | h[2]);
  }
}

// wave-wide inclusive prefix sums (64 lanes)
__device__ __forceinline__ double wave_incl_scan(double x, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    double t = __shfl_up(x, off);
    if (lane >= off) x += t;
  }
  return x;
}
__device__ __forceinline__ int wave_incl_scan_i(int x, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    int t = __shfl_up(x, off);
    if (lane >= off) x += t;
  }
  return x;
}

// vectorized decode: whole chunk into LDS, wide loads, high ILP.
// (element semantics identical to d_lv_at/d_dv_at, which remain the
//  reference implementations / fallback)
template <bool AS_DOUBLE>
__device__ inline void d_decode_chunk(const DVec& v, int n, int64_t* tout,
                                      double* dout, int lane) {
  if (v.wf == FDB_WF_DDV_CONST) {
    for (int i = lane; i < n; i += 64) {
      int64_t x = v.init + (int64_t)v.slope * i;
      if (AS_DOUBLE) dout[i] = (double)x; else tout[i] = x;
    }
    return;
  }
  if (v.wf == FDB_WF_PRIM64) {
    // raw 64-bit payload, 8-byte aligned (+8 from a 64B-aligned base)
    for (int i = lane; i < n; i += 64) {
      if (AS_DOUBLE) dout[i] = d_f64(v.idata + 8 * (size_t)i);
      else           tout[i] = d_i64(v.idata + 8 * (size_t)i);
    }
    return;
  }
  // packed DDV inner data starts at +28 (4-byte aligned only)
  if (v.nbits == 16) {
    for (int i0 = 4 * lane; i0 < n; i0 += 256) {
      uint32_t lo = d_u32(v.idata + 2 * (size_t)i0);
      uint32_t hi = d_u32(v.idata + 2 * (size_t)i0 + 4);
      uint64_t w = ((uint64_t)hi << 32) | lo;
      #pragma unroll
      for (int k = 0; k < 4; k++) {
        if (i0 + k < n) {
          int32_t d = (int32_t)(int16_t)(uint16_t)(w >> (16 * k));
          if (!v.sign) d &= 0xffff;
          int64_t x = v.init + (int64_t)v.slope * (i0 + k) + d;
          if (AS_DOUBLE) dout[i0 + k] = (double)x; else tout[i0 + k] = x;
        }
      }
    }
    return;
  }
  if (v.nbits == 8) {
    for (int i0 = 8 * lane; i0 < n; i0 += 512) {
      uint32_t lo = d_u32(v.idata + (size_t)i0);
      uint32_t hi = d_u32(v.idata + (size_t)i0 + 4);
      uint64_t w = ((uint64_t)hi << 32) | lo;
      #pragma unroll
      for (int k = 0; k < 8; k++) {
        if (i0 + k < n) {
          int32_t d = (int32_t)(int8_t)(uint8_t)(w >> (8 * k));
          if (!v.sign) d &= 0xff;
          int64_t x = v.init + (int64_t)v.slope * (i0 + k) + d;
          if (AS_DOUBLE) dout[i0 + k] = (double)x; else tout[i0 + k] = x;
        }
      }
    }
    return;
  }
  if (v.nbits == 32) {
    for (int i0 = 2 * lane; i0 < n; i0 += 128) {
      #pragma unroll
      for (int k = 0; k < 2; k++) {
        if (i0 + k < n) {
          int64_t x = v.init + (int64_t)v.slope * (i0 + k)
                    + d_i32(v.idata + 4 * (size_t)(i0 + k));
          if (AS_DOUBLE) dout[i0 + k] = (double)x; else tout[i0 + k] = x;
        }
      }
    }
    return;
  }
  // nbits 2/4 fallback (rare)
  for (int i = lane; i < n; i += 64) {
    int64_t x = v.init + (int64_t)v.slope * i + d_inner_at(&v, i);
    if (AS_DOUBLE) dout[i] = (double)x; else tout[i] = x;
  }
}

// --- four rows per lane: the fast scan's packed-DDV decode (8/16-bit) -------
// Lane l owns rows 4l..4l+3 of each 256-row pass (400 rows: two passes): one
// 4- or 8-byte payload load, four results, 128-bit LDS stores. The only guard
// is the lane's (first row < n), so:
//  * the output array must be 16-byte aligned and hold 4*ceil(n/4) entries;
//    rows n..4*ceil(n/4)-1 are written with garbage that nothing interprets
//    (scan_fast.hip's decode section lists the readers);
//  * the last active lane reads up to 3 elements, <= 6 bytes, past the
//    vector's end. Vectors are padded to 64 B inside the blob and the blob
//    carries a 512-B tail pad, so the bytes exist; they only feed those
//    garbage rows.
// Inner data starts at vector + 28: 4-byte aligned, like each lane's slice.
template <int NBITS>
__device__ __forceinline__ void d_load_rows4(const uint8_t* idata, int i0,
                                             bool sign, int32_t d[4]) {
  static_assert(NBITS == 8 || NBITS == 16, "packed widths with a 4-row slice");
  if (NBITS == 16) {
    // unsigned 32-bit byte offsets: a uniform base plus a zero-extended lane
    // offset addresses through the SGPR-base form, no 64-bit VGPR pair
    const uint32_t lo = d_u32(idata + 2u * (uint32_t)i0);
    const uint32_t hi = d_u32(idata + (2u * (uint32_t)i0 + 4u));
    const int32_t m = sign ? -1 : 0xffff;      // unsigned: drop the extension
    d[0] = (int32_t)(int16_t)(lo & 0xffff) & m;
    d[1] = ((int32_t)lo >> 16) & m;
    d[2] = (int32_t)(int16_t)(hi & 0xffff) & m;
    d[3] = ((int32_t)hi >> 16) & m;
  } else {
    const uint32_t w = d_u32(idata + (uint32_t)i0);
    const int32_t m = sign ? -1 : 0xff;
    d[0] = (int32_t)(int8_t)(w & 0xff) & m;
    d[1] = (int32_t)(int8_t)((w >> 8) & 0xff) & m;
    d[2] = (int32_t)(int8_t)((w >> 16) & 0xff) & m;
    d[3] = ((int32_t)w >> 24) & m;
  }
}

// values: v[i] = (double)(init + slope*i + inner[i]). exact32 (upload-time
// flag, fast_desc.h): |init| < 2^52 and off = slope*i + inner[i] fits i32 for
// every row, so (double)init + (double)off adds two integers whose sum stays
// below 2^53 — the f64 add is exact and equals the i64 sum's conversion bit
// for bit, at one v_cvt_f64_i32 and one add per row instead of an i64
// multiply-add and a four-instruction i64 -> f64 convert.
template <int NBITS>
__device__ __forceinline__ void d_decode_val4(const uint8_t* idata, bool sign,
                                              int64_t init, int32_t slope,
                                              bool exact32, int n, double* dout,
                                              int lane) {
  if (exact32) {
    const double init_f = (double)init;          // wave-uniform, once per series
    for (int i0 = 4 * lane; i0 < n; i0 += 256) {
      int32_t d[4];
      d_load_rows4<NBITS>(idata, i0, sign, d);
      const uint32_t b = (uint32_t)slope * (uint32_t)i0;
      double2 a, c;
      a.x = init_f + (double)(int32_t)(b + (uint32_t)d[0]);
      a.y = init_f + (double)(int32_t)(b + (uint32_t)slope + (uint32_t)d[1]);
      c.x = init_f + (double)(int32_t)(b + 2u * (uint32_t)slope + (uint32_t)d[2]);
      c.y = init_f + (double)(int32_t)(b + 3u * (uint32_t)slope + (uint32_t)d[3]);
      *reinterpret_cast<double2*>(dout + i0) = a;
      *reinterpret_cast<double2*>(dout + i0 + 2) = c;
    }
    return;
  }
  for (int i0 = 4 * lane; i0 < n; i0 += 256) {
    int32_t d[4];
    d_load_rows4<NBITS>(idata, i0, sign, d);
    const int64_t b = init + (int64_t)slope * i0;
    double2 a, c;
    a.x = (double)(b + d[0]);
    a.y = (double)(b + slope + d[1]);
    c.x = (double)(b + 2 * (int64_t)slope + d[2]);
    c.y = (double)(b + 3 * (int64_t)slope + d[3]);
    *reinterpret_cast<double2*>(dout + i0) = a;
    *reinterpret_cast<double2*>(dout + i0 + 2) = c;
  }
}

// i32-offset decode variant: timestamps relative to the chunk's first ts.
// Caller guarantees the chunk's time span fits i32 (upload-time check). The
// packed 8/16-bit arms use the four-rows-per-lane layout above: tout must be
// 16-byte aligned with 4*ceil(n/4) writable entries.
__device__ inline void d_decode_ts_offsets(const DVec& v, int n, int64_t ts0,
                                           int32_t* tout, int lane) {
  // all arithmetic in i32: the upload guard pins the chunk's span (and so
  // base + slope*i + inner, = ts_i - ts0) inside i32, and i32 wrap-around
  // equals the i64-then-truncate result whenever the true value fits
  if (v.wf == FDB_WF_DDV_CONST) {
    const int32_t cbase = (int32_t)(v.init - ts0);
    for (int i = lane; i < n; i += 64)
      tout[i] = (int32_t)((uint32_t)v.slope * (uint32_t)i + (uint32_t)cbase);
    return;
  }
  if (v.wf == FDB_WF_PRIM64) {
    for (int i = lane; i < n; i += 64)
      tout[i] = (int32_t)(d_i64(v.idata + 8 * (size_t)i) - ts0);
    return;
  }
  const int32_t base = (int32_t)(v.init - ts0);
  if (v.nbits == 16 || v.nbits == 8) {
    const uint32_t sl = (uint32_t)v.slope;
    for (int i0 = 4 * lane; i0 < n; i0 += 256) {
      int32_t d[4];
      if (v.nbits == 16) d_load_rows4<16>(v.idata, i0, v.sign, d);
      else               d_load_rows4<8>(v.idata, i0, v.sign, d);
      const uint32_t b = (uint32_t)base + sl * (uint32_t)i0;
      int4 r;
      r.x = (int32_t)(b + (uint32_t)d[0]);
      r.y = (int32_t)(b + sl + (uint32_t)d[1]);
      r.z = (int32_t)(b + 2u * sl + (uint32_t)d[2]);
      r.w = (int32_t)(b + 3u * sl + (uint32_t)d[3]);
      *reinterpret_cast<int4*>(tout + i0) = r;
    }
    return;
  }
  if (v.nbits == 32) {
    for (int i0 = 2 * lane; i0 < n; i0 += 128) {
      #pragma unroll
      for (int k = 0; k < 2; k++)
        if (i0 + k < n)
          tout[i0 + k] = (int32_t)((uint32_t)base
              + (uint32_t)v.slope * (uint32_t)(i0 + k)
              + (uint32_t)d_i32(v.idata + 4 * (size_t)(i0 + k)));
    }
    return;
  }
  for (int i = lane; i < n; i += 64)
    tout[i] = (int32_t)((uint32_t)base + (uint32_t)v.slope * (uint32_t)i
                        + (uint32_t)d_inner_at(&v, i));
}

// NaN-aware f64 atomic min/max via CAS (group aggregation; RowAggregator semantics)
__device__ inline void atomic_min_max_f64(double* addr, double val, bool is_min) {
  unsigned long long* a = (unsigned long long*)addr;
  unsigned long long old = *a, assumed;
  do {
    assumed = old;
    double cur = __longlong_as_double((long long)assumed);
    double nw = isnan(cur) ? val : (is_min ? fmin(cur, val) : fmax(cur, val));
    if (!isnan(cur) && nw == cur) return;
    old = atomicCAS(a, assumed, (unsigned long long)__double_as_longlong(nw));
  } while (old != assumed);
}

#endif  // FDB_SCAN_COMMON_H
