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
#include <string>
#include <vector>

#include "../filodb_amd/csrc/fast_desc.h"
#include "../filodb_amd/csrc/window_bounds.h"
#include "../include/filodb_amd.h"

namespace {

struct Rng {                       // splitmix64: deterministic everywhere
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
  }
  int64_t range(int64_t lo, int64_t hi) {      // inclusive
    return lo + (int64_t)(next() % (uint64_t)(hi - lo + 1));
  }
  double unit() { return (double)(next() >> 11) / 9007199254740992.0; }
};

const int kSizes[] = {1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 240, 400};
const int kM[] = {1, 20, 40, 64};
const int64_t kQ = 15000;
const int64_t kT0 = 10000000;      // a multiple of kQ: the scrape grid's origin
const int64_t kPhases[] = {0, 1, kQ / 2, kQ - 1, -1};

std::vector<int64_t> grid(Rng& r, int n, int64_t interval, int64_t jitter) {
  std::vector<int64_t> t((size_t)n);
  for (int i = 0; i < n; i++)
    t[(size_t)i] = kT0 + interval * i + (jitter ? r.range(-jitter, jitter) : 0);
  return t;
}

std::vector<int64_t> make(const std::string& cls, Rng& r, int n) {
  std::vector<int64_t> t;
  if (cls == "bench") t = grid(r, n, kQ, 300);
  else if (cls == "zerojitter") t = grid(r, n, kQ, 0);       // every row a tie
  else if (cls == "driftm1") t = grid(r, n, kQ - 1, 100);
  else if (cls == "driftp1") t = grid(r, n, kQ + 1, 100);
  else if (cls == "driftm5") t = grid(r, n, kQ - 5, 0);
  else if (cls == "driftp5") t = grid(r, n, kQ + 5, 0);
  else if (cls == "dups") {
    // a late row and the next, early one share a timestamp: 0.55 q after one
    // grid point is 0.45 q before the next, and both stay inside C
    t = grid(r, n, kQ, 50);
    for (int i = 0; i + 1 < n; i += (int)r.range(2, 5)) {
      t[(size_t)i] = kT0 + kQ * i + (kQ * 11) / 20;
      t[(size_t)i + 1] = t[(size_t)i];
    }
  } else if (cls == "drop") {                  // a scrape grid with rows missing
    for (int64_t j = 0; (int)t.size() < n; j++) {
      if (j > 0 && r.unit() < 0.05) continue;
      t.push_back(kT0 + j * kQ + r.range(-300, 300));
    }
  } else if (cls == "irregular") {
    int64_t x = kT0;
    for (int i = 0; i < n; i++) { t.push_back(x); x += r.range(1, 40000); }
  } else if (cls == "interval10s") {
    t = grid(r, n, 10000, 300);
  } else if (cls == "widejitter") {            // residuals around +-0.6 q
    t = grid(r, n, kQ, 9000);
  }
  for (size_t i = 1; i < t.size(); i++)        // nondecreasing, like the store
    if (t[i] < t[i - 1]) t[i] = t[i - 1];
  return t;
}

struct Totals {
  long cases = 0, eligible = 0, c_holds = 0, rejected_c = 0, windows = 0, mism = 0;
};

// one series' timestamps as the kernel holds them, from the descriptor alone
bool decode_tso(const uint8_t* blob, const fdb_dir_entry_t& e, const FdbFastDesc& d,
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

int brute_e(const int32_t* tso, int n, int64_t x) {
  for (int i = n - 1; i >= 0; i--) if (tso[i] <= x) return i;
  return -1;
}
int brute_s(const int32_t* tso, int n, int64_t y) {
  for (int i = 0; i < n; i++) if (tso[i] >= y) return i;
  return n;
}

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
    if (t.mism < 10) fprintf(stderr, "UNSOUND class=%s n=%d k0=%d\n", cls, n, k0);
    t.mism++;
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
    const int we = brute_e(tso, n, xw), wsr = brute_s(tso, n, yw);
    t.windows++;
    const bool ok = e == we && s == wsr && (e < 0 || t2 == tso[e]) &&
                    (s >= n || t1 == tso[s]);
    if (!ok) {
      if (t.mism < 10)
        fprintf(stderr, "MISMATCH class=%s n=%d m=%d w=%d: e=%d want %d, s=%d want %d "
                "(t2=%d t1=%d)\n", cls, n, m, w, e, we, s, wsr, t2, t1);
      t.mism++;
    }
  }
  return true;
}

}  // namespace

int main() {
  const char* classes[] = {"bench", "zerojitter", "driftm1", "driftp1", "driftm5",
                           "driftp5", "dups", "widejitter", "drop", "irregular",
                           "interval10s"};
  long total_bad = 0;
  for (const char* cls : classes) {
    Rng r{0xa11ULL * 1000003ULL + strlen(cls) * 7919ULL + (uint64_t)cls[0]};
    fdb_store_t* st = fdb_store_create(0);
    std::vector<std::vector<int64_t>> tss;
    for (int n : kSizes)
      for (int rep = 0; rep < 3; rep++) {
        tss.push_back(make(cls, r, n));
        const std::vector<double> v((size_t)n, 1.0);
        const int32_t sid = fdb_store_add_series(st, 0, FDB_COL_GAUGE);
        fdb_series_append(st, sid, tss.back().data(), v.data(), n);
      }
    fdb_store_seal(st);
    fdb_view_t view;
    if (fdb_store_view(st, &view) != FDB_OK) { fprintf(stderr, "%s: no view\n", cls); return 1; }
    const fdb_dir_entry_t* dir = (const fdb_dir_entry_t*)view.dir;
    Totals t;
    std::vector<int32_t> buf;
    for (int32_t sid = 0; sid < view.num_series; sid++) {
      if (view.series_nchunks[sid] != 1) { t.mism++; continue; }
      const fdb_dir_entry_t& e = dir[view.series_first[sid]];
      FdbFastDesc d;
      fdb_build_fast_desc(view.blob, e.ts_off, e.val_off, e.num_rows, &d);
      if (d.n != (int)tss[(size_t)sid].size() || !decode_tso(view.blob, e, d, buf)) {
        t.mism++;
        continue;
      }
      const int nw = d.n + 40;
      for (int64_t ph : kPhases)
        for (int m : kM)
          check_query(cls, d, buf.data() + 1, kT0 - 10 * kQ + ph,
                      kQ, m, nw, true, t);
    }
    printf("class=%s cases=%ld eligible=%ld c_holds=%ld rejected_c=%ld windows=%ld "
           "mismatches=%ld\n", cls, t.cases, t.eligible, t.c_holds, t.rejected_c,
           t.windows, t.mism);
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
    fdb_store_seal(st);
    fdb_view_t view;
    if (fdb_store_view(st, &view) != FDB_OK) { fprintf(stderr, "bench: no view\n"); return 1; }
    const fdb_dir_entry_t* dir = (const fdb_dir_entry_t*)view.dir;
    Totals t;
    long eligible = 0;
    std::vector<int32_t> buf;
    for (int32_t sid = 0; sid < view.num_series; sid++) {
      const fdb_dir_entry_t& e = dir[view.series_first[sid]];
      FdbFastDesc d;
      fdb_build_fast_desc(view.blob, e.ts_off, e.val_off, e.num_rows, &d);
      if (!decode_tso(view.blob, e, d, buf)) { t.mism++; continue; }
      if (check_query("benchlaw", d, buf.data() + 1, 100000, 15000, 20, 241,
                      sid < 2000, t))
        eligible++;
    }
    printf("class=benchlaw cases=%ld eligible=%ld c_holds=%ld rejected_c=%ld windows=%ld "
           "mismatches=%ld\n", t.cases, t.eligible, t.c_holds, t.rejected_c, t.windows,
           t.mism);
    printf("bench-law series eligible: %ld of %d\n", eligible, view.num_series);
    total_bad += t.mism;
    if (eligible != view.num_series) total_bad++;
    fdb_store_destroy(st);
  }
  printf(total_bad ? "FAILED\n" : "OK\n");
  return total_bad == 0 ? 0 : 1;
}
