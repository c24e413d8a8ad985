// Host verification of the fast scan's upload-time decode descriptors
// (filodb_amd/csrc/fast_desc.h) and of the four-rows-per-lane decode that
// consumes them (scan_common.h: d_load_rows4 / d_decode_val4 /
// d_decode_ts_offsets; scan_fast.hip's decode section).
//
//   hipcc -O2 -std=c++17 -fopenmp -o verify_fast_desc
//       tools/verify_fast_desc.cpp filodb_amd/csrc/chunk_builder.cpp
//   ./verify_fast_desc              # exit 0 = no mismatch
// (hipcc only for the HIP include path chunk_builder.cpp's header wants: both
// files are host C++, no GPU is touched. Add -fsanitize=address,undefined for
// the sanitized build; the program is stand-alone.)
//
// Stores are built through the C API: one per vector encoding x the row
// counts 1..400 that cross the 4-row lane groups and the 256-row pass, plus
// random vectors and a bench-law sample (fdb_synth_generate, the law of
// bench.py's rate_1m). For every series:
//  * "fields": fdb_build_fast_desc against open_ref below, a literal
//    restatement of the device's d_vec_open_wide, field for field, and the
//    timestamp residual range (ts_rmin / ts_rmax) against the element reader;
//  * "rows": a lane-by-lane replay of the kernel's decode (64 lanes, 256-row
//    passes, whole 4-row groups stored with no per-row guard) into sentinel-
//    filled tso[404] / val[400]; every row < n must equal the element
//    readers' value, init + slope*i + inner then (double), bit for bit; rows
//    >= 4*ceil(n/4) must still hold the sentinel; the bytes a lane loads past
//    its vector's end ("overread", max over all lanes) must stay <= 6 and
//    inside the blob plus its 512-B upload pad.
// One line per store: "store=<name> series=<n> fields=<n> rows=<n>
// exact32=<n> resid=<n> overread=<bytes> mismatches=<n>" (resid: series with a
// valid timestamp residual range, ts_rmin <= ts_rmax).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "verify_kit_store.h"

namespace {

using kit::Rng;

const int kSizes[] = {1, 2, 3, 4, 5, 63, 64, 65, 240, 255, 256, 257, 399, 400};
const int64_t kT0 = 10000000;

// ---- literal restatement of d_vec_open_wide (scan_common.h) ---------------
struct RefVec {
  const uint8_t* idata;
  int64_t init, first;
  int32_t slope;
  int n;
  uint16_t wf;
  uint8_t nbits, sign, dropped;
};

RefVec open_ref(const uint8_t* p) {
  RefVec v;
  memset(&v, 0, sizeof(v));
  uint32_t h[8];
  memcpy(h, p, 32);
  const uint16_t wf = (uint16_t)(h[1] & 0xffff);
  v.wf = wf;
  v.dropped = ((h[1] >> 16) & FDB_DROP_MASK) != 0;
  if (wf == FDB_WF_DDV) {
    v.init = (int64_t)(((uint64_t)h[3] << 32) | h[2]);
    v.slope = (int32_t)h[4];
    const uint32_t w6 = h[6];
    v.nbits = (uint8_t)((w6 >> 16) & FDB_NBITS_MASK);
    v.sign = ((w6 >> 16) & FDB_SIGN_MASK) != 0;
    const int bitShift = (int)(w6 >> 24) & 0x3f;
    v.idata = p + FDB_DDV_OFF_INNER + FDB_PRIM_OFF_DATA;
    const int numBytes = (int)h[5];
    v.n = ((numBytes - 4) * 8 + (bitShift != 0 ? bitShift - 8 : 0)) / v.nbits;
    int64_t in0;
    switch (v.nbits) {
      case 32: in0 = (int32_t)h[7]; break;
      case 16: { int32_t x = (int16_t)(h[7] & 0xffff);
                 in0 = v.sign ? x : (x & 0xffff); } break;
      case 8:  { int32_t x = (int8_t)(h[7] & 0xff);
                 in0 = v.sign ? x : (x & 0xff); } break;
      case 4:  in0 = h[7] & 0x0f; break;
      default: in0 = h[7] & 0x03; break;
    }
    v.first = v.init + in0;
  } else if (wf == FDB_WF_DDV_CONST) {
    v.n = (int32_t)h[2];
    v.init = (int64_t)(((uint64_t)h[4] << 32) | h[3]);
    v.slope = (int32_t)h[5];
    v.first = v.init;
  } else {
    v.n = ((int)h[0] - 4) / 8;
    v.idata = p + FDB_PRIM_OFF_DATA;
    v.nbits = 64; v.sign = 1;
    v.first = (int64_t)(((uint64_t)h[3] << 32) | h[2]);
  }
  return v;
}

// element readers (d_inner_at / d_lv_at / d_dv_at)
int64_t inner_at(const RefVec& v, int i) {
  switch (v.nbits) {
    case 32: { int32_t x; memcpy(&x, v.idata + 4 * (size_t)i, 4); return x; }
    case 16: { uint16_t u; memcpy(&u, v.idata + 2 * (size_t)i, 2);
               int32_t x = (int16_t)u; return v.sign ? x : (x & 0xffff); }
    case 8:  { int32_t x = (int8_t)v.idata[i]; return v.sign ? x : (x & 0xff); }
    case 4:  return (v.idata[i >> 1] >> ((i & 1) * 4)) & 0x0f;
    case 2:  return (v.idata[i >> 2] >> ((i & 3) * 2)) & 0x03;
  }
  return 0;
}
int64_t lv_at(const RefVec& v, int i) {
  if (v.wf == FDB_WF_DDV) return v.init + (int64_t)v.slope * i + inner_at(v, i);
  if (v.wf == FDB_WF_DDV_CONST) return v.init + (int64_t)v.slope * i;
  int64_t x; memcpy(&x, v.idata + 8 * (size_t)i, 8); return x;
}
double dv_at(const RefVec& v, int i) {
  if (v.wf == FDB_WF_PRIM64) { double x; memcpy(&x, v.idata + 8 * (size_t)i, 8); return x; }
  return (double)lv_at(v, i);
}

// ---- the kernel's decode, lane by lane ------------------------------------
struct Span { const uint8_t* blob; size_t blob_len; size_t vec_end; int over; };

uint32_t load_u32(Span& sp, const uint8_t* p) {
  const size_t off = (size_t)(p - sp.blob);
  if (off + 4 > sp.vec_end) {
    const int o = (int)(off + 4 - sp.vec_end);
    if (o > sp.over) sp.over = o;
  }
  if (off + 4 > sp.blob_len + 512) { sp.over = 1 << 20; return 0; }   // outside pad
  uint32_t v = 0;                    // the pad is zero-filled at upload
  for (int k = 0; k < 4; k++)
    if (off + k < sp.blob_len) v |= (uint32_t)sp.blob[off + k] << (8 * k);
  return v;
}

template <int NBITS>
void load_rows4(Span& sp, const uint8_t* idata, int i0, bool sign, int32_t d[4]) {
  if (NBITS == 16) {
    const uint32_t lo = load_u32(sp, idata + 2u * (uint32_t)i0);
    const uint32_t hi = load_u32(sp, idata + (2u * (uint32_t)i0 + 4u));
    const int32_t m = sign ? -1 : 0xffff;
    d[0] = (int32_t)(int16_t)(lo & 0xffff) & m;
    d[1] = ((int32_t)lo >> 16) & m;
    d[2] = (int32_t)(int16_t)(hi & 0xffff) & m;
    d[3] = ((int32_t)hi >> 16) & m;
  } else {
    const uint32_t w = load_u32(sp, idata + (uint32_t)i0);
    const int32_t m = sign ? -1 : 0xff;
    d[0] = (int32_t)(int8_t)(w & 0xff) & m;
    d[1] = (int32_t)(int8_t)((w >> 8) & 0xff) & m;
    d[2] = (int32_t)(int8_t)((w >> 16) & 0xff) & m;
    d[3] = ((int32_t)w >> 24) & m;
  }
}

template <int NBITS>
void decode_ts4(Span& sp, const uint8_t* idata, bool sign, int32_t base,
                int32_t slope, int n, int32_t* tout) {
  const uint32_t sl = (uint32_t)slope;
  for (int lane = 0; lane < 64; lane++)
    for (int i0 = 4 * lane; i0 < n; i0 += 256) {
      int32_t d[4];
      load_rows4<NBITS>(sp, idata, i0, sign, d);
      const uint32_t b = (uint32_t)base + sl * (uint32_t)i0;
      tout[i0 + 0] = (int32_t)(b + (uint32_t)d[0]);
      tout[i0 + 1] = (int32_t)(b + sl + (uint32_t)d[1]);
      tout[i0 + 2] = (int32_t)(b + 2u * sl + (uint32_t)d[2]);
      tout[i0 + 3] = (int32_t)(b + 3u * sl + (uint32_t)d[3]);
    }
}

template <int NBITS>
void decode_val4(Span& sp, const uint8_t* idata, bool sign, int64_t init,
                 int32_t slope, bool exact32, int n, double* dout) {
  const double init_f = (double)init;
  for (int lane = 0; lane < 64; lane++)
    for (int i0 = 4 * lane; i0 < n; i0 += 256) {
      int32_t d[4];
      load_rows4<NBITS>(sp, idata, i0, sign, d);
      for (int k = 0; k < 4; k++) {
        if (exact32) {
          const uint32_t off = (uint32_t)slope * (uint32_t)i0 +
                               (uint32_t)k * (uint32_t)slope + (uint32_t)d[k];
          dout[i0 + k] = init_f + (double)(int32_t)off;
        } else {
          // garbage rows may overflow i64 on the device (wrap); keep it defined
          const uint64_t x = (uint64_t)init + (uint64_t)((int64_t)slope * i0) +
                             (uint64_t)((int64_t)k * slope) + (uint64_t)(int64_t)d[k];
          dout[i0 + k] = (double)(int64_t)x;
        }
      }
    }
}

struct Totals { long series = 0, fields = 0, rows = 0, exact32 = 0, resid = 0, mism = 0; int over = 0; };

const int32_t kSentT = 0x5a5a5a5a;
const double kSentV = -7.25e300;

void check_series(const fdb_view_t& view, int32_t sid, Totals& t) {
  const uint8_t* blob = view.blob;
  FdbFastDesc d;
  const fdb_dir_entry_t* e = kit::series_desc(view, sid, &d);
  t.series++;
  auto bad = [&](const char* what) {
    kit::mismatch(t.mism, "series %d: %s\n", sid, what);
  };
  if (!e) {
    if (d.n != 0) bad("n of an empty series");
    if (d.ts_rmin <= d.ts_rmax) bad("ts_rmin/ts_rmax of an empty series");
    return;
  }
  const RefVec tv = open_ref(blob + e->ts_off), vv = open_ref(blob + e->val_off);
  // ---- fields ----
  int n = e->num_rows;
  if (n > FDB_DEFAULT_MAX_ROWS || n > tv.n) n = 0;
  auto cls_of = [](const RefVec& v) {
    return v.wf == FDB_WF_DDV ? FDB_FD_PACKED : v.wf == FDB_WF_DDV_CONST ? FDB_FD_CONST
                                                                          : FDB_FD_RAW64; };
#define FIELD(cond, what) do { t.fields++; if (!(cond)) bad(what); } while (0)
  FIELD(((uint64_t)d.ts_unit << 6) == e->ts_off, "ts_unit");
  FIELD(((uint64_t)d.val_unit << 6) == e->val_off, "val_unit");
  FIELD(d.n == n, "n");
  FIELD(d.ts_cls == cls_of(tv) && d.val_cls == cls_of(vv), "class");
  FIELD(d.ts_nbits == tv.nbits && d.val_nbits == vv.nbits, "nbits");
  FIELD(((d.ts_flags & FDB_FD_SIGN) != 0) == (tv.sign != 0) &&
        ((d.val_flags & FDB_FD_SIGN) != 0) == (vv.sign != 0), "sign");
  FIELD(((d.val_flags & FDB_FD_DROPPED) != 0) == (vv.dropped != 0), "dropped");
  FIELD(d.ts_slope == tv.slope && d.val_slope == vv.slope && d.val_init == vv.init, "init/slope");
  if (n > 0) {
    FIELD(d.ts0 == tv.first, "ts0");
    FIELD(d.ts_base == (int32_t)(tv.init - tv.first), "ts_base");
    const uint8_t* tdata = blob + e->ts_off + (d.ts_cls == FDB_FD_PACKED ? 28 : 8);
    const uint8_t* vdata = blob + e->val_off + (d.val_cls == FDB_FD_PACKED ? 28 : 8);
    FIELD(d.ts_cls == FDB_FD_CONST || tdata == tv.idata, "ts payload");
    FIELD(d.val_cls == FDB_FD_CONST || vdata == vv.idata, "val payload");
    // val_exact32 restated: row by row in i64
    bool ex = vv.wf == FDB_WF_DDV && vv.n >= n && std::llabs(vv.init) < ((int64_t)1 << 52);
    for (int i = 0; ex && i < n; i++) {
      const int64_t off = (int64_t)vv.slope * i + inner_at(vv, i);
      ex = off >= INT32_MIN && off <= INT32_MAX;
    }
    FIELD(((d.val_flags & FDB_FD_EXACT32) != 0) == ex, "val_exact32");
    // ts_rmin / ts_rmax restated from the element reader: the residuals
    // lv_at(i) - (init + slope*i) over the rows, valid only where every
    // offset from the first timestamp is a non-negative i32 and both bounds
    // fit i16; never for a raw vector
    bool rok = tv.wf != FDB_WF_PRIM64 &&
               tv.init - tv.first >= INT32_MIN && tv.init - tv.first <= INT32_MAX;
    int64_t rmin = 0, rmax = 0;
    for (int i = 0; rok && i < n; i++) {
      const int64_t off = lv_at(tv, i) - tv.first;
      const int64_t res = lv_at(tv, i) - (tv.init + (int64_t)tv.slope * i);
      if (i == 0 || res < rmin) rmin = res;
      if (i == 0 || res > rmax) rmax = res;
      rok = off >= 0 && off <= INT32_MAX;
    }
    rok = rok && rmin >= INT16_MIN && rmax <= INT16_MAX;
    FIELD(rok ? (d.ts_rmin == rmin && d.ts_rmax == rmax) : d.ts_rmin > d.ts_rmax,
          "ts_rmin/ts_rmax");
    if (rok) t.resid++;
  } else {
    FIELD(d.ts_rmin > d.ts_rmax, "ts_rmin/ts_rmax of an empty series");
  }
#undef FIELD
  if (d.val_flags & FDB_FD_EXACT32) t.exact32++;
  if (n == 0) return;
  // ---- rows: replay the decode as scan_fast.hip dispatches it ----
  static int32_t tso[FDB_DEFAULT_MAX_ROWS + 4];
  static double val[FDB_DEFAULT_MAX_ROWS];
  for (int i = 0; i < FDB_DEFAULT_MAX_ROWS + 4; i++) tso[i] = kSentT;
  for (int i = 0; i < FDB_DEFAULT_MAX_ROWS; i++) val[i] = kSentV;
  auto vec_end = [&](uint64_t off) {
    uint32_t lw; memcpy(&lw, blob + off, 4); return (size_t)off + 4 + lw; };
  Span ts_sp{blob, (size_t)view.blob_len, vec_end(e->ts_off), 0};
  Span v_sp{blob, (size_t)view.blob_len, vec_end(e->val_off), 0};
  bool ts4 = false, val4 = false;
  if (d.ts_cls == FDB_FD_PACKED && (d.ts_nbits == 8 || d.ts_nbits == 16)) {
    ts4 = true;
    const uint8_t* idata = blob + ((size_t)d.ts_unit << 6) + 28;
    if (d.ts_nbits == 16)
      decode_ts4<16>(ts_sp, idata, d.ts_flags & FDB_FD_SIGN, d.ts_base, d.ts_slope, n, tso);
    else
      decode_ts4<8>(ts_sp, idata, d.ts_flags & FDB_FD_SIGN, d.ts_base, d.ts_slope, n, tso);
  } else {                   // the per-element loops: init = ts0 + ts_base
    RefVec r = tv;
    r.init = d.ts0 + d.ts_base; r.slope = d.ts_slope;
    for (int i = 0; i < n; i++) tso[i] = (int32_t)(lv_at(r, i) - d.ts0);
  }
  if (d.val_cls == FDB_FD_PACKED && (d.val_nbits == 8 || d.val_nbits == 16)) {
    val4 = true;
    const uint8_t* idata = blob + ((size_t)d.val_unit << 6) + 28;
    const bool ex = (d.val_flags & FDB_FD_EXACT32) != 0;
    if (d.val_nbits == 16)
      decode_val4<16>(v_sp, idata, d.val_flags & FDB_FD_SIGN, d.val_init, d.val_slope, ex, n, val);
    else
      decode_val4<8>(v_sp, idata, d.val_flags & FDB_FD_SIGN, d.val_init, d.val_slope, ex, n, val);
  } else {
    RefVec r = vv;
    r.init = d.val_init; r.slope = d.val_slope;
    for (int i = 0; i < n; i++) val[i] = dv_at(r, i);
  }
  if (ts_sp.over > t.over) t.over = ts_sp.over;
  if (v_sp.over > t.over) t.over = v_sp.over;
  for (int i = 0; i < n; i++) {
    t.rows++;
    const int32_t wt = (int32_t)(lv_at(tv, i) - tv.first);
    const double wv = dv_at(vv, i);
    if (tso[i] != wt) bad("timestamp row");
    if (memcmp(&val[i], &wv, 8) != 0) bad("value row");
  }
  const int n4 = (n + 3) / 4 * 4;
  for (int i = ts4 ? n4 : n; i < FDB_DEFAULT_MAX_ROWS + 4; i++)
    if (tso[i] != kSentT) bad("tso[] written past the last 4-row group");
  for (int i = val4 ? n4 : n; i < FDB_DEFAULT_MAX_ROWS; i++)
    if (memcmp(&val[i], &kSentV, 8) != 0) bad("val[] written past the last 4-row group");
}

// ---- stores ---------------------------------------------------------------
struct Law { const char* name; int64_t step; int64_t lo, hi; };   // offsets from a line

std::vector<int64_t> line(Rng& r, int n, int64_t init, int64_t step, int64_t lo, int64_t hi) {
  std::vector<int64_t> v((size_t)n);
  for (int i = 0; i < n; i++) {
    int64_t d = (i == 0 || i == n - 1) ? 0 : (i == 1 ? (lo < 0 ? lo : hi) : r.range(lo, hi));
    v[(size_t)i] = init + step * i + d;
  }
  return v;
}

std::vector<uint8_t> enc_raw_i64(const std::vector<int64_t>& ts) {
  std::vector<uint8_t> b(8 + 8 * ts.size());
  const uint32_t lw = (uint32_t)(4 + 8 * ts.size());
  const uint16_t wf = FDB_WF_PRIM64, nb = 64 | FDB_SIGN_MASK;
  memcpy(&b[0], &lw, 4); memcpy(&b[4], &wf, 2); memcpy(&b[6], &nb, 2);
  memcpy(&b[8], ts.data(), 8 * ts.size());
  return b;
}
std::vector<uint8_t> enc_ddv_s8(const std::vector<int64_t>& ts) {   // signed 8-bit inner
  const int n = (int)ts.size();
  const int32_t slope = (int32_t)((ts[(size_t)n - 1] - ts[0]) / (n - 1));
  std::vector<uint8_t> b(28 + (size_t)n, 0);
  const uint32_t lw = (uint32_t)(b.size() - 4), wf = FDB_WF_DDV, ilw = (uint32_t)(4 + n);
  const uint16_t iwf = FDB_WF_INT_NOMASK;
  memcpy(&b[0], &lw, 4); memcpy(&b[4], &wf, 4); memcpy(&b[8], &ts[0], 8);
  memcpy(&b[16], &slope, 4); memcpy(&b[20], &ilw, 4); memcpy(&b[24], &iwf, 2);
  b[26] = 8 | FDB_SIGN_MASK; b[27] = 0;
  for (int i = 0; i < n; i++) b[28 + (size_t)i] = (uint8_t)(int8_t)(ts[(size_t)i] - (ts[0] + (int64_t)slope * i));
  return b;
}

int report(const char* name, fdb_store_t* st, long* exact_out = nullptr) {
  fdb_view_t view;
  if (!kit::sealed_view(name, st, &view)) return 1;
  Totals t;
  for (int32_t sid = 0; sid < view.num_series; sid++) check_series(view, sid, t);
  kit::report_line("store", name,
                   {{"series", t.series}, {"fields", t.fields}, {"rows", t.rows},
                    {"exact32", t.exact32}, {"resid", t.resid}, {"overread", t.over},
                    {"mismatches", t.mism}});
  if (exact_out) *exact_out = t.exact32;
  fdb_store_destroy(st);
  return (t.mism != 0 || t.over > 6) ? 1 : 0;
}

using kit::add_series;

std::vector<double> counter(Rng& r, int n) {
  std::vector<double> v((size_t)n);
  double c = 0;
  for (int i = 0; i < n; i++) { c += (double)r.range(0, 20); v[(size_t)i] = c; }
  return v;
}

}  // namespace

int main() {
  int rc = 0;
  Rng r{20240};
  // timestamp encodings (values: counters)
  const Law tlaws[] = {{"tconst", 15000, 0, 0}, {"t8u", 1000, 0, 255},
                       {"t16s", 15000, -300, 300}, {"t16u", 100000, 0, 65535},
                       {"t32", 3000000, -(1 << 30) / 1024, (int64_t)1 << 20}};
  for (const Law& l : tlaws) {
    fdb_store_t* st = fdb_store_create(0);
    for (int n : kSizes) add_series(st, FDB_COL_COUNTER, line(r, n, kT0, l.step, l.lo, l.hi), counter(r, n));
    rc |= report(l.name, st);
  }
  for (int enc = 0; enc < 2; enc++) {            // hand-encoded: signed 8-bit, raw i64
    fdb_store_t* tmp = fdb_store_create(0);
    std::vector<std::vector<int64_t>> tss;
    for (int n : kSizes) {
      tss.push_back(enc ? line(r, n, kT0, 15000, -300, 300) : line(r, n, kT0, 1000, -120, 100));
      add_series(tmp, FDB_COL_COUNTER, tss.back(), counter(r, n));
    }
    fdb_view_t tv;
    if (!kit::sealed_view("tmp", tmp, &tv)) return 1;
    const fdb_dir_entry_t* dir = (const fdb_dir_entry_t*)tv.dir;
    fdb_store_t* st = fdb_store_create(0);
    for (size_t i = 0; i < tss.size(); i++) {
      const fdb_dir_entry_t& e = dir[tv.series_first[i]];
      uint32_t vl; memcpy(&vl, tv.blob + e.val_off, 4);
      const std::vector<uint8_t> tb = (enc || tss[i].size() < 3) ? enc_raw_i64(tss[i]) : enc_ddv_s8(tss[i]);
      const int32_t sid = fdb_store_add_series(st, 0, FDB_COL_COUNTER);
      if (fdb_store_add_encoded_chunk(st, sid, tb.data(), (int32_t)tb.size(), tv.blob + e.val_off,
                                      (int32_t)vl + 4, e.num_rows, e.start_time, e.end_time) != FDB_OK) {
        fprintf(stderr, "add_encoded_chunk: %s\n", fdb_last_error());
        return 1;
      }
    }
    rc |= report(enc ? "traw" : "t8s", st);
    fdb_store_destroy(tmp);
  }
  // value encodings (timestamps: the bench law)
  struct VLaw { const char* name; int64_t init, slope, lo, hi; };
  const VLaw vlaws[] = {{"v2u", 1000, 7, 0, 3}, {"v4u", 1000, 40, 0, 15},
                        {"v8s", 5000, 300, -128, 127}, {"v8u", 5000, 300, 0, 255},
                        {"v16s", 1000000, 70000, -32768, 32767}, {"v16u", 1000000, 70000, 0, 65535},
                        {"v32", 10000000000LL, 3, -(1 << 30), 1 << 30}, {"vconst", 123456, 11, 0, 0},
                        {"vneg", -1000000000, -1000, -128, 127},
                        {"vbig", ((int64_t)1 << 52) + 1, 300, -128, 127},
                        // slope*i alone leaves i32 after row 107: misses val_exact32
                        {"vsteep", 0, 20000000, -128, 127}};
  for (const VLaw& l : vlaws) {
    fdb_store_t* st = fdb_store_create(0);
    for (int n : kSizes) {
      const std::vector<int64_t> lv = line(r, n, l.init, l.slope, l.lo, l.hi);
      add_series(st, FDB_COL_GAUGE, line(r, n, kT0, 15000, -300, 300), std::vector<double>(lv.begin(), lv.end()));
    }
    long ex = 0;
    rc |= report(l.name, st, &ex);
    // vbig must miss the flag on |init| in every series, vsteep on the offset
    // from 240 rows up (check_series restates the flag per series; this pins
    // the two cases the flag exists for)
    if ((!strcmp(l.name, "vbig") && ex != 0) || (!strcmp(l.name, "vsteep") && ex > 9)) {
      fprintf(stderr, "%s: val_exact32 set on %ld series\n", l.name, ex);
      rc = 1;
    }
  }
  {                                                     // raw f64 and counters with resets
    fdb_store_t* st = fdb_store_create(0);
    for (int n : kSizes) {
      std::vector<double> v((size_t)n);
      for (double& x : v) x = r.unit() * 100 + 0.25;
      add_series(st, FDB_COL_GAUGE, line(r, n, kT0, 15000, -300, 300), v);
    }
    rc |= report("vraw", st);
    st = fdb_store_create(0);
    for (int n : kSizes) {
      std::vector<double> v = counter(r, n);
      if (n >= 3) for (int i = n / 2; i < n; i++) v[(size_t)i] -= v[(size_t)n / 2];
      add_series(st, FDB_COL_COUNTER, line(r, n, kT0, 15000, -300, 300), v);
    }
    rc |= report("vresets", st);
  }
  {                                                     // random vectors
    fdb_store_t* st = fdb_store_create(0);
    for (int k = 0; k < 4000; k++) {
      const int n = (int)r.range(1, 400);
      const int tb = (int)r.range(0, 3), vb = (int)r.range(0, 5);
      const int64_t trange[] = {0, 255, 32767, 65535}, vrange[] = {0, 3, 15, 127, 32767, 1 << 30};
      const int64_t tstep = 70000 + r.range(0, 100000);
      const int64_t vinit = r.range(-((int64_t)1 << 53), (int64_t)1 << 53) >> r.range(0, 40);
      const int64_t vslope = r.range(-3000000, 3000000);
      const bool sg = r.range(0, 1);
      std::vector<int64_t> lv = line(r, n, vinit, vslope, sg ? -vrange[vb] : 0, vrange[vb]);
      bool fits = true;                                  // stay exactly representable
      for (int64_t x : lv) fits = fits && std::llabs(x) < ((int64_t)1 << 53);
      if (!fits) continue;
      add_series(st, r.range(0, 1) ? FDB_COL_COUNTER : FDB_COL_GAUGE,
          line(r, n, kT0, tstep, (tb == 2) ? -trange[tb] : 0, trange[tb]),
          std::vector<double>(lv.begin(), lv.end()));
    }
    rc |= report("random", st);
  }
  {                                                     // the bench law (rate_1m's generator)
    fdb_store_t* st = fdb_store_create(0);
    fdb_synth_generate(st, FDB_COL_COUNTER, 20000, 240, 100000, 15000, 300, 10.0, 0.001, 1000, 42);
    long ex = 0;
    rc |= report("bench", st, &ex);
    printf("bench-law series with val_exact32: %ld of 20000\n", ex);
  }
  return kit::exit_status(rc, true);
}
