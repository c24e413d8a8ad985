// Per-series decode descriptors of the fast scan (scan_fast.hip), built once
// at upload from the sealed, immutable blob.
//
// Everything the kernel used to re-derive per series and per query before its
// first decode instruction — series_first[sid] / series_nchunks[sid], the
// directory row (ts_off / val_off / num_rows) and both 32-byte vector headers
// (wire format, nbits / sign / bitShift arithmetic, init, slope, element 0) —
// is a function of the dataset alone. One 64-byte, 64-byte-aligned record per
// series holds the parsed result, so the kernel fetches it with one scalar
// load through a wave-uniform address and goes straight to the payload.
//
// ts_rmin / ts_rmax bound the timestamp vector's residuals: inner[i] of a
// packed vector over the series' rows, 0 for a const one. With them the
// kernel decides, in scalar arithmetic and without touching a row, whether
// every row sits within one query step of "its" window edge, and then takes
// each window's rows directly (window_bounds.h, fdb_aligned_*). ts_rmin >
// ts_rmax marks a series that never qualifies: raw 64-bit timestamps, no
// rows, residuals outside i16, or offsets that leave i32.
//
// Host-only, plain C++ (no HIP): engine.hip builds the table,
// tools/verify_fast_desc.cpp checks the builder against a restatement of the
// device header parser and a lane-by-lane model of the decode.
#ifndef FDB_FAST_DESC_H
#define FDB_FAST_DESC_H

#include <cstdint>
#include <cstring>

#include "chunk_format.h"

enum { FDB_FD_CONST = 0,     // const DDV: init + slope*i, no payload
       FDB_FD_PACKED = 1,    // packed DDV: init + slope*i + inner[i]
       FDB_FD_RAW64 = 2 };   // raw 64-bit elements (i64 timestamps, f64 values)
enum { FDB_FD_SIGN = 1,      // packed inner elements are signed
       FDB_FD_DROPPED = 2,   // value vector's counter-reset (drop) bit
       FDB_FD_EXACT32 = 4 }; // value vector: |init| < 2^52 and slope*i + inner[i]
                             // fits i32 for every row (checked row by row)

struct FdbFastDesc {
  uint32_t ts_unit;      // timestamp vector's blob offset / 64 (vectors are
  uint32_t val_unit;     // 64-B aligned); payload = vector + 28 (packed) / 8 (raw)
  uint16_t n;            // rows; 0 = empty series (no chunk, or a guard tripped)
  uint8_t  ts_cls, ts_nbits;
  uint8_t  ts_flags, val_cls, val_nbits, val_flags;
  int64_t  ts0;          // first timestamp
  int32_t  ts_base;      // (int32)(init - ts0): tso[i] = ts_base + ts_slope*i + inner[i]
  int32_t  ts_slope;
  int64_t  val_init;
  int32_t  val_slope;
  int16_t  ts_rmin, ts_rmax;   // min / max timestamp residual; rmin > rmax: none
  uint32_t _pad[4];
};
static_assert(sizeof(FdbFastDesc) == 64, "one 64-byte scalar load per series");

// a vector header as the device's d_vec_open_wide parses it
struct FdbFdVec {
  int64_t init, first;
  int32_t slope, n;
  uint32_t payload;      // byte offset of element data from the vector start
  uint8_t cls, nbits, flags;
};

inline FdbFdVec fdb_fd_open(const uint8_t* p) {
  uint32_t h[8];
  memcpy(h, p, 32);
  FdbFdVec v;
  memset(&v, 0, sizeof(v));
  const uint16_t wf = (uint16_t)(h[1] & 0xffff);
  if (((h[1] >> 16) & FDB_DROP_MASK) != 0) v.flags |= FDB_FD_DROPPED;
  if (wf == FDB_WF_DDV) {
    v.cls = FDB_FD_PACKED;
    v.init = (int64_t)(((uint64_t)h[3] << 32) | h[2]);
    v.slope = (int32_t)h[4];
    const uint32_t w6 = h[6];
    v.nbits = (uint8_t)((w6 >> 16) & FDB_NBITS_MASK);
    if (((w6 >> 16) & FDB_SIGN_MASK) != 0) v.flags |= FDB_FD_SIGN;
    const int bitShift = (int)(w6 >> 24) & 0x3f;
    const int numBytes = (int)h[5];
    v.n = v.nbits
        ? ((numBytes - 4) * 8 + (bitShift != 0 ? bitShift - 8 : 0)) / v.nbits : 0;
    v.payload = FDB_DDV_OFF_INNER + FDB_PRIM_OFF_DATA;
    const bool sg = (v.flags & FDB_FD_SIGN) != 0;
    int64_t in0;
    switch (v.nbits) {
      case 32: in0 = (int32_t)h[7]; break;
      case 16: { int32_t x = (int16_t)(h[7] & 0xffff); in0 = sg ? x : (x & 0xffff); } break;
      case 8:  { int32_t x = (int8_t)(h[7] & 0xff); in0 = sg ? x : (x & 0xff); } break;
      case 4:  in0 = h[7] & 0x0f; break;
      default: in0 = h[7] & 0x03; break;
    }
    v.first = v.init + in0;
  } else if (wf == FDB_WF_DDV_CONST) {
    v.cls = FDB_FD_CONST;
    v.n = (int32_t)h[2];
    v.init = (int64_t)(((uint64_t)h[4] << 32) | h[3]);
    v.slope = (int32_t)h[5];
    v.first = v.init;
  } else {
    v.cls = FDB_FD_RAW64;
    v.n = ((int)h[0] - 4) / 8;
    v.nbits = 64;
    v.flags |= FDB_FD_SIGN;
    v.payload = FDB_PRIM_OFF_DATA;
    v.first = (int64_t)(((uint64_t)h[3] << 32) | h[2]);
  }
  return v;
}

// packed-DDV inner element i (d_inner_at's semantics)
inline int64_t fdb_fd_inner(const uint8_t* idata, int nbits, bool sign, int i) {
  switch (nbits) {
    case 32: { int32_t x; memcpy(&x, idata + 4 * (size_t)i, 4); return x; }
    case 16: { uint16_t u; memcpy(&u, idata + 2 * (size_t)i, 2);
               int32_t x = (int16_t)u; return sign ? x : (x & 0xffff); }
    case 8:  { int32_t x = (int8_t)idata[i]; return sign ? x : (x & 0xff); }
    case 4:  return (idata[i >> 1] >> ((i & 1) * 4)) & 0x0f;
    case 2:  return (idata[i >> 2] >> ((i & 3) * 2)) & 0x03;
  }
  return 0;
}

// One series' descriptor from its single chunk: the two vectors' blob offsets
// and the directory's row count. num_rows <= 0 (a series without a chunk)
// gives the empty record. Both offsets must be multiples of 64 below 2^38
// (the caller checks; the builder's vectors always are).
inline void fdb_build_fast_desc(const uint8_t* blob, uint64_t ts_off,
                                uint64_t val_off, int32_t num_rows,
                                FdbFastDesc* out) {
  FdbFastDesc d;
  memset(&d, 0, sizeof(d));
  d.ts_rmin = 1;             // rmin > rmax: not eligible for direct window rows
  if (num_rows > 0) {
    const FdbFdVec tv = fdb_fd_open(blob + ts_off);
    const FdbFdVec vv = fdb_fd_open(blob + val_off);
    d.ts_unit = (uint32_t)(ts_off >> 6);
    d.val_unit = (uint32_t)(val_off >> 6);
    d.ts_cls = tv.cls; d.ts_nbits = tv.nbits; d.ts_flags = tv.flags;
    d.val_cls = vv.cls; d.val_nbits = vv.nbits; d.val_flags = vv.flags;
    d.ts_slope = tv.slope;
    d.val_init = vv.init; d.val_slope = vv.slope;
    // the kernel's guards, decided here: an over-long chunk or a directory
    // row count the timestamp vector does not hold is an empty series
    if (num_rows <= FDB_DEFAULT_MAX_ROWS && num_rows <= tv.n) {
      d.n = (uint16_t)num_rows;
      d.ts0 = tv.first;
      d.ts_base = (int32_t)(tv.init - tv.first);
      // residual range of the timestamp vector: tso[i] = ts_base + ts_slope*i
      // + inner[i] must hold in plain integers (no i32 wrap) for the
      // aligned-window test to stand on it
      if (tv.cls != FDB_FD_RAW64 &&
          tv.init - tv.first >= INT32_MIN && tv.init - tv.first <= INT32_MAX) {
        const uint8_t* idata = blob + ts_off + tv.payload;
        const bool sg = (tv.flags & FDB_FD_SIGN) != 0;
        int64_t rmin = 0, rmax = 0;
        bool fits = true;
        for (int i = 0; i < num_rows && fits; i++) {
          const int64_t in = tv.cls == FDB_FD_PACKED
                                 ? fdb_fd_inner(idata, tv.nbits, sg, i) : 0;
          const int64_t off = (tv.init - tv.first) + (int64_t)tv.slope * i + in;
          if (i == 0 || in < rmin) rmin = in;
          if (i == 0 || in > rmax) rmax = in;
          fits = off >= 0 && off <= INT32_MAX;
        }
        if (fits && rmin >= INT16_MIN && rmax <= INT16_MAX) {
          d.ts_rmin = (int16_t)rmin;
          d.ts_rmax = (int16_t)rmax;
        }
      }
      if (vv.cls == FDB_FD_PACKED && vv.n >= num_rows &&
          vv.init > -((int64_t)1 << 52) && vv.init < ((int64_t)1 << 52)) {
        const uint8_t* idata = blob + val_off + vv.payload;
        const bool sg = (vv.flags & FDB_FD_SIGN) != 0;
        bool fits = true;
        for (int i = 0; i < num_rows && fits; i++) {
          const int64_t off = (int64_t)vv.slope * i +
                              fdb_fd_inner(idata, vv.nbits, sg, i);
          fits = off >= INT32_MIN && off <= INT32_MAX;
        }
        if (fits) d.val_flags |= FDB_FD_EXACT32;
      }
    }
  }
  *out = d;
}

#endif  // FDB_FAST_DESC_H
