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
#include <string>
#include <vector>

#include "../filodb_amd/csrc/window_bounds.h"

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

const int kSizes[] = {0, 1, 2, 63, 64, 65, 240, 400};

// scrape grid 15 s +- 300 ms with a fraction `drop` of the rows deleted
std::vector<int64_t> scrape(Rng& r, int n, double drop) {
  std::vector<int64_t> t;
  for (int64_t j = 0; (int)t.size() < n; j++) {
    if (drop > 0 && r.unit() < drop) continue;
    t.push_back(j * 15000 + r.range(-300, 300));
  }
  return t;
}

std::vector<int64_t> make(const std::string& cls, Rng& r, int n) {
  std::vector<int64_t> t;
  if (cls == "bench") t = scrape(r, n, 0.0);
  else if (cls == "drop2") t = scrape(r, n, 0.02);
  else if (cls == "drop10") t = scrape(r, n, 0.10);
  else if (cls == "drop30") t = scrape(r, n, 0.30);
  else if (cls == "geometric") {         // gaps double, restarting every 21 rows
    int64_t x = 0;
    for (int i = 0; i < n; i++) { t.push_back(x); x += (int64_t)1 << (i % 21); }
  } else if (cls == "clusters") {        // two dense clusters, one 2^30 ms gap
    int64_t x = 0;
    for (int i = 0; i < n; i++) {
      t.push_back(x);
      x += (i == n / 2 - 1) ? ((int64_t)1 << 30) : r.range(900, 1100);
    }
  } else if (cls == "allequal") {
    t.assign(n, 0);
  } else if (cls == "dupruns") {         // runs of 1..5 equal timestamps
    int64_t x = 0;
    while ((int)t.size() < n) {
      int run = (int)r.range(1, 5);
      for (int k = 0; k < run && (int)t.size() < n; k++) t.push_back(x);
      x += 15000 + r.range(-300, 300);
    }
  }
  for (size_t i = 1; i < t.size(); i++)      // nondecreasing, like the store
    if (t[i] < t[i - 1]) t[i] = t[i - 1];
  for (size_t i = t.size(); i-- > 0;) t[i] -= t[0];   // offsets from row 0
  return t;
}

int brute_e(const std::vector<int32_t>& tso, int n, int64_t x) {
  for (int i = n - 1; i >= 0; i--) if (tso[i] <= x) return i;
  return -1;
}
int brute_s(const std::vector<int32_t>& tso, int n, int64_t y) {
  for (int i = 0; i < n; i++) if (tso[i] >= y) return i;
  return n;
}

}  // namespace

int main() {
  const char* classes[] = {"bench", "drop2", "drop10", "drop30", "geometric",
                           "clusters", "allequal", "dupruns"};
  long total_bad = 0;
  for (const char* cls : classes) {
    long bounds = 0, bad = 0;
    int residue = 0;
    for (int n : kSizes) {
      Rng r{0x5eedULL * 1000003ULL + (uint64_t)n * 7919ULL + strlen(cls)};
      const std::vector<int64_t> t = make(cls, r, n);
      // exactly max(n, 4) elements (the header's contract): an over-read is
      // an address-sanitizer error; cells past n hold garbage on purpose
      std::vector<int32_t> tso((size_t)(n > 4 ? n : 4));
      for (size_t i = 0; i < tso.size(); i++)
        tso[i] = i < (size_t)n ? (int32_t)t[i]
                               : (int32_t)(r.next() & 1 ? INT32_MIN : 12345);
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
        const int we = brute_e(tso, n, x), wsr = brute_s(tso, n, x);
        bounds += 2;
        const bool ok = e == we && s == wsr && (e < 0 || te == tso[e]) &&
                        (s >= n || ts == tso[s]);
        if (!ok) {
          if (bad < 10)
            fprintf(stderr, "MISMATCH class=%s n=%d x=%lld: e=%d want %d, "
                    "s=%d want %d (t_e=%d t_s=%d)\n", cls, n, (long long)x,
                    e, we, s, wsr, te, ts);
          bad++;
        }
      }
    }
    printf("class=%s bounds=%ld residue=%d mismatches=%ld\n", cls, bounds,
           residue, bad);
    total_bad += bad;
  }
  return total_bad == 0 ? 0 : 1;
}
