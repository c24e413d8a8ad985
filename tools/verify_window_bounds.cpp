// Host verification of filodb_amd/csrc/window_bounds.h: both bounds against a
// brute-force linear scan over every input class the fast scan kernel can
// meet, plus the count of bounds that needed the binary-search residue path.
//
//   c++ -O2 -std=c++17 -o verify_window_bounds tools/verify_window_bounds.cpp
//   ./verify_window_bounds          # exit 0 = no mismatch
//
// One line per input class: "class=<name> bounds=<checked> residue=<count>
// mismatches=<count>". tests/test_window_bounds_host.py builds and runs this.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../filodb_amd/csrc/window_bounds.h"
#include "verify_kit.h"

using kit::Rng;

const int kSizes[] = {0, 1, 2, 63, 64, 65, 240, 400};

int main() {
  const char* classes[] = {"bench", "drop2", "drop10", "drop30", "geometric",
                           "clusters", "allequal", "dupruns"};
  long total_bad = 0;
  for (const char* cls : classes) {
    long bounds = 0, bad = 0;
    int residue = 0;
    for (int n : kSizes) {
      Rng r{0x5eedULL * 1000003ULL + (uint64_t)n * 7919ULL + strlen(cls)};
      // scrape grid 15 s from 0, as offsets from row 0; exactly max(n, 4)
      // elements, so an over-read is an address-sanitizer error
      const std::vector<int32_t> tso =
          kit::tso_exact(kit::make_ts(cls, r, n, 0, 15000, true), r);
      const int64_t span = n > 0 ? tso[n - 1] : 0;

      std::vector<int64_t> xs;
      for (int i = 0; i < n; i++)
        for (int d = -1; d <= 1; d++) xs.push_back((int64_t)tso[i] + d);
      for (int k = 0; k < 3000; k++) xs.push_back(r.range(-20000, span + 20000));
      // the kernel's own query law: window ends on a 15 s grid, starts 5 m back
      for (int64_t w = -25; w <= span / 15000 + 25; w++) {
        xs.push_back(w * 15000);
        xs.push_back(w * 15000 - 300000);
      }
      for (int sh = 20; sh <= 40; sh++)              // far outside the chunk
        for (int d = -1; d <= 1; d++) {
          xs.push_back(((int64_t)1 << sh) + d);
          xs.push_back(-((int64_t)1 << sh) + d);
          xs.push_back(span + ((int64_t)1 << sh) + d);
        }

      const FdbLin lin = fdb_bounds_prepare(tso.data(), n);
      for (int64_t x : xs) {
        int32_t te = 0, ts = 0;
        const int e = fdb_bound_e(tso.data(), n, lin, x, &te, &residue);
        const int s = fdb_bound_s(tso.data(), n, lin, x, &ts, &residue);
        const int we = kit::brute_e(tso.data(), n, x), wsr = kit::brute_s(tso.data(), n, x);
        bounds += 2;
        const bool ok = e == we && s == wsr && (e < 0 || te == tso[e]) &&
                        (s >= n || ts == tso[s]);
        if (!ok)
          kit::mismatch(bad, "MISMATCH class=%s n=%d x=%lld: e=%d want %d, "
                        "s=%d want %d (t_e=%d t_s=%d)\n", cls, n, (long long)x,
                        e, we, s, wsr, te, ts);
      }
    }
    kit::report_line("class", cls, {{"bounds", bounds}, {"residue", residue},
                                    {"mismatches", bad}});
    total_bad += bad;
  }
  return kit::exit_status(total_bad);
}
