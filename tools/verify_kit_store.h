// The part of the verifiers' kit that needs the store: series in through the C
// API, the sealed store's view, and each series' descriptor and timestamps as
// the fast scan kernel holds them. A verifier that includes this links
// filodb_amd/csrc/chunk_builder.cpp; the others include verify_kit.h alone.
#pragma once
#include <cstring>

#include "../filodb_amd/csrc/fast_desc.h"
#include "../include/filodb_amd.h"
#include "verify_kit.h"

namespace kit {

inline void add_series(fdb_store_t* st, int kind, const std::vector<int64_t>& ts,
                       const std::vector<double>& v) {
  const int32_t sid = fdb_store_add_series(st, 0, kind);
  fdb_series_append(st, sid, ts.data(), v.data(), (int32_t)ts.size());
}

// seals the store and takes its view; false, with a line on stderr, if none
inline bool sealed_view(const char* name, fdb_store_t* st, fdb_view_t* view) {
  fdb_store_seal(st);
  if (fdb_store_view(st, view) == FDB_OK) return true;
  fprintf(stderr, "%s: no view\n", name);
  return false;
}

// a series' first chunk (nullptr: it has none) and the descriptor the upload
// builds for it
inline const fdb_dir_entry_t* series_desc(const fdb_view_t& view, int32_t sid,
                                          FdbFastDesc* d) {
  const fdb_dir_entry_t* e =
      view.series_nchunks[sid] >= 1
          ? &((const fdb_dir_entry_t*)view.dir)[view.series_first[sid]] : nullptr;
  fdb_build_fast_desc(view.blob, e ? e->ts_off : 0, e ? e->val_off : 0,
                      e ? e->num_rows : 0, d);
  return e;
}

// one series' timestamps as the kernel holds them, from the descriptor alone:
// offsets from row 0 in buf[1 .. n], with exactly one cell before row 0 and
// one after row n-1, both garbage, so a wider read is an address-sanitizer
// error. false: an offset does not fit a non-negative i32.
inline bool decode_tso(const uint8_t* blob, const fdb_dir_entry_t& e, const FdbFastDesc& d,
                       std::vector<int32_t>& buf) {
  const int n = d.n;
  buf.assign((size_t)n + 2, 0x5a5a5a5a);
  buf[0] = INT32_MIN + 7;                                  // tso[-1]: garbage
  buf[(size_t)n + 1] = 12345;                              // tso[n]: garbage
  const FdbFdVec tv = fdb_fd_open(blob + e.ts_off);
  const uint8_t* idata = blob + e.ts_off + tv.payload;
  for (int i = 0; i < n; i++) {
    int64_t t;
    if (tv.cls == FDB_FD_RAW64) { memcpy(&t, idata + 8 * (size_t)i, 8); t -= d.ts0; }
    else t = (int64_t)d.ts_base + (int64_t)d.ts_slope * i +
             (tv.cls == FDB_FD_PACKED
                  ? fdb_fd_inner(idata, tv.nbits, (tv.flags & FDB_FD_SIGN) != 0, i) : 0);
    if (t < 0 || t > INT32_MAX) return false;
    buf[(size_t)i + 1] = (int32_t)t;
  }
  return true;
}

}  // namespace kit
