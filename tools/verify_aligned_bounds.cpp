// Host verification of the fast scan's direct window rows
// (filodb_amd/csrc/window_bounds.h: fdb_aligned_guess / fdb_aligned_test /
// fdb_aligned_bounds) together with the descriptor fields they
// stand on (fast_desc.h: ts_base, ts_slope, ts_rmin, ts_rmax).
//
//   hipcc -O2 -std=c++17 -fopenmp -o verify_aligned_bounds
//       tools/verify_aligned_bounds.cpp filodb_amd/csrc/chunk_builder.cpp
//   ./verify_aligned_bounds         # exit 0 = no mismatch, bench law eligible
// (hipcc only for the HIP include path chunk_builder.cpp's header wants: both
// files are host C++, no GPU is touched. Add -fsanitize=address,undefined for
// the sanitized build; the program is stand-alone.)
//
// Every series goes through the store and the descriptor builder, so the
// rows and the residual range are the ones the kernel will see (the builder
// stores a near-linear timestamp vector as a const one; verify_fast_desc.cpp
// checks the decode itself). For each series, each query
// phase relative to the scrape grid (0, 1, q/2, q-1, -1) and each window
// length m = 1, 20, 40, 64 steps:
//  * the eligibility test is run as the kernel runs it; condition C is also
//    decided by brute force over the rows. Accepted without C = a mismatch
//    ("unsound"); rejected although C holds is counted and printed;
//  * for an accepted series, every window w in [-64, nw+64) is compared with
//    a linear scan: e, s, and t2 / t1 where the bound is a row. tso[] has
//    exactly one cell before row 0 and one after row n-1, both garbage: a
//    wider read is an address-sanitizer error.
// One line per class: "class=<name> cases=<n> eligible=<n> c_holds=<n>
// rejected_c=<n> windows=<n> mismatches=<n>"; then the bench law through
// fdb_synth_generate with bench.py's parameters and query: all 20,000 series
// must be eligible.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../filodb_amd/csrc/window_bounds.h"
#include "verify_kit_store.h"

namespace {

using kit::Rng;

const int kSizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 240, 400};
const int kM[] = {1, 20, 40, 64};
const int64_t kQ = 15000;
const int64_t kT0 = 10000000;      // a multiple of kQ: the scrape grid's origin
const int64_t kPhases[] = {0, 1, kQ / 2, kQ - 1, -1};

struct Totals {
  long cases = 0, eligible = 0, c_holds = 0, rejected_c = 0, windows = 0, mism = 0;
};

// the kernel's sequence for one (series, query); returns eligibility
bool check_query(const char* cls, const FdbFastDesc& d, const int32_t* tso,
                 int64_t qstart, int64_t q,
                 int m, int nw, bool compare, Totals& t) {
  const int n = d.n;
  const int64_t A = d.ts0 - qstart;
  const int32_t k0 = fdb_aligned_guess(d.ts_base, d.ts_rmin, d.ts_rmax, A,
                                       1.0f / (float)q);
  const FdbAligned al = fdb_aligned_test(n, d.ts_base, d.ts_slope, d.ts_rmin,
                                         d.ts_rmax, A, q, m, nw, k0);
  t.cases++;
  bool c = n >= 1 && k0 != INT32_MIN;                      // condition C(k0), by rows
  for (int i = 0; c && i < n; i++) {
    const int64_t u = (int64_t)tso[i] + A - ((int64_t)i + k0) * q;
    c = u > -q && u < q;
  }
  if (c) t.c_holds++;
  if (al.ok) t.eligible++;
  if (c && !al.ok) t.rejected_c++;
  if (al.ok && !c) {
    kit::mismatch(t.mism, "UNSOUND class=%s n=%d k0=%d\n", cls, n, k0);
    return true;
  }
  if (!al.ok || !compare) return al.ok;
  for (int w = -64; w < nw + 64; w++) {
    const int32_t x = (int32_t)((uint32_t)al.x0 + (uint32_t)w * (uint32_t)q);
    const int32_t y = (int32_t)((uint32_t)x - (uint32_t)(m * q));
    int32_t t1 = 0, t2 = 0;
    int e, s;
    fdb_aligned_bounds(tso, n, al.k0, w, m, x, y, &e, &s, &t1, &t2);
    const int64_t xw = (int64_t)w * q - A, yw = xw - (int64_t)m * q;
    const int we = kit::brute_e(tso, n, xw), wsr = kit::brute_s(tso, n, yw);
    t.windows++;
    const bool ok = e == we && s == wsr && (e < 0 || t2 == tso[e]) &&
                    (s >= n || t1 == tso[s]);
    if (!ok)
      kit::mismatch(t.mism, "MISMATCH class=%s n=%d m=%d w=%d: e=%d want %d, s=%d want %d "
                    "(t2=%d t1=%d)\n", cls, n, m, w, e, we, s, wsr, t2, t1);
  }
  return true;
}

void report(const char* cls, const Totals& t) {
  kit::report_line("class", cls,
                   {{"cases", t.cases}, {"eligible", t.eligible}, {"c_holds", t.c_holds},
                    {"rejected_c", t.rejected_c}, {"windows", t.windows},
                    {"mismatches", t.mism}});
}

}  // namespace

int main() {
  const char* classes[] = {"bench", "zerojitter", "driftm1", "driftp1", "driftm5",
                           "driftp5", "dups", "widejitter", "drop", "irregular",
                           "interval10s"};
  long total_bad = 0;
  std::vector<int32_t> buf;
  for (const char* cls : classes) {
    Rng r{0xa11ULL * 1000003ULL + strlen(cls) * 7919ULL + (uint64_t)cls[0]};
    // this tool's "drop" keeps row 0; the scrape family's drop laws do not
    const char* law = strcmp(cls, "drop") ? cls : "drop5keep0";
    fdb_store_t* st = fdb_store_create(0);
    std::vector<int> sizes;
    for (int n : kSizes)
      for (int rep = 0; rep < 3; rep++) {
        kit::add_series(st, FDB_COL_GAUGE, kit::make_ts(law, r, n, kT0, kQ, false),
                        std::vector<double>((size_t)n, 1.0));
        sizes.push_back(n);
      }
    fdb_view_t view;
    if (!kit::sealed_view(cls, st, &view)) return 1;
    Totals t;
    for (int32_t sid = 0; sid < view.num_series; sid++) {
      FdbFastDesc d;
      const fdb_dir_entry_t* e = kit::series_desc(view, sid, &d);
      if (view.series_nchunks[sid] != 1 || d.n != sizes[(size_t)sid] ||
          !kit::decode_tso(view.blob, *e, d, buf)) {
        t.mism++;
        continue;
      }
      const int nw = d.n + 40;
      for (int64_t ph : kPhases)
        for (int m : kM)
          check_query(cls, d, buf.data() + 1, kT0 - 10 * kQ + ph,
                      kQ, m, nw, true, t);
    }
    report(cls, t);
    total_bad += t.mism;
    fdb_store_destroy(st);
  }
  {
    // bench.py's store (synth_generate: start 100000, 15 s, +-300 ms, lambda
    // 10, reset_p 0.001, seed 42) and query (start = the store's origin, step
    // 15 s, 241 windows of 5 m); windows compared for the first 2,000 series
    fdb_store_t* st = fdb_store_create(0);
    fdb_synth_generate(st, FDB_COL_COUNTER, 20000, 240, 100000, 15000, 300, 10.0, 0.001,
                       1000, 42);
    fdb_view_t view;
    if (!kit::sealed_view("bench", st, &view)) return 1;
    Totals t;
    long eligible = 0;
    for (int32_t sid = 0; sid < view.num_series; sid++) {
      FdbFastDesc d;
      const fdb_dir_entry_t* e = kit::series_desc(view, sid, &d);
      if (!e || !kit::decode_tso(view.blob, *e, d, buf)) { t.mism++; continue; }
      if (check_query("benchlaw", d, buf.data() + 1, 100000, 15000, 20, 241,
                      sid < 2000, t))
        eligible++;
    }
    report("benchlaw", t);
    printf("bench-law series eligible: %ld of %d\n", eligible, view.num_series);
    total_bad += t.mism;
    if (eligible != view.num_series) total_bad++;
    fdb_store_destroy(st);
  }
  return kit::exit_status(total_bad, true);
}
