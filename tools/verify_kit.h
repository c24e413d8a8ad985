// What the host verifiers (tools/verify_*.cpp) share: the generator, the
// linear-scan reference every row bound is judged against, the timestamp
// laws, and the report / mismatch / exit-status conventions. Header only, host
// C++17, no HIP and nothing of the store: verify_kit_store.h adds the part
// that needs the store's sources. Each verifier keeps its own main, case
// lists, seeds and checks.
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

namespace kit {

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

// ---- the reference: last row <= x (-1: none), first row >= y (n: none) ----
inline int brute_e(const int32_t* tso, int n, int64_t x) {
  for (int i = n - 1; i >= 0; i--) if (tso[i] <= x) return i;
  return -1;
}
inline int brute_s(const int32_t* tso, int n, int64_t y) {
  for (int i = 0; i < n; i++) if (tso[i] >= y) return i;
  return n;
}

// ---- timestamp laws ---------------------------------------------------------
// rows on a grid of `interval` ms from `origin`, each +- `jitter` ms
inline std::vector<int64_t> grid(Rng& r, int n, int64_t origin, int64_t interval,
                                 int64_t jitter) {
  std::vector<int64_t> t((size_t)n);
  for (int i = 0; i < n; i++)
    t[(size_t)i] = origin + interval * i + (jitter ? r.range(-jitter, jitter) : 0);
  return t;
}

// scrape grid q +- 300 ms with a fraction `drop` of the rows deleted, row 0
// like any other
inline std::vector<int64_t> scrape(Rng& r, int n, int64_t origin, int64_t q,
                                   double drop) {
  std::vector<int64_t> t;
  for (int64_t j = 0; (int)t.size() < n; j++) {
    if (drop > 0 && r.unit() < drop) continue;
    t.push_back(origin + j * q + r.range(-300, 300));
  }
  return t;
}

// n nondecreasing timestamps of law `law`: grid point 0 at `origin`, scrape
// interval q; from_row0 hands back offsets from row 0 instead. An unknown
// name gives no rows.
inline std::vector<int64_t> make_ts(const std::string& law, Rng& r, int n,
                                    int64_t origin, int64_t q, bool from_row0) {
  std::vector<int64_t> t;
  if (law == "bench") t = grid(r, n, origin, q, 300);
  else if (law == "grid" || law == "zerojitter")          // every row a tie
    t = grid(r, n, origin, q, 0);
  else if (law == "drop2") t = scrape(r, n, origin, q, 0.02);
  else if (law == "drop10") t = scrape(r, n, origin, q, 0.10);
  else if (law == "drop30") t = scrape(r, n, origin, q, 0.30);
  else if (law == "drop5keep0") {          // rows missing, never row 0 (and
    for (int64_t j = 0; (int)t.size() < n; j++) {       // no draw for it)
      if (j > 0 && r.unit() < 0.05) continue;
      t.push_back(origin + j * q + r.range(-300, 300));
    }
  } else if (law == "geometric") {         // gaps double, restarting every 21 rows
    int64_t x = origin;
    for (int i = 0; i < n; i++) { t.push_back(x); x += (int64_t)1 << (i % 21); }
  } else if (law == "clusters") {          // two dense clusters, one 2^30 ms gap
    int64_t x = origin;
    for (int i = 0; i < n; i++) {
      t.push_back(x);
      x += (i == n / 2 - 1) ? ((int64_t)1 << 30) : r.range(900, 1100);
    }
  } else if (law == "allequal") {
    t.assign((size_t)n, origin);
  } else if (law == "dupruns" || law == "dupgrid") {   // runs of 1..5 equal rows,
    int64_t x = origin;                                // dupgrid: on grid points
    while ((int)t.size() < n) {
      int run = (int)r.range(1, 5);
      for (int k = 0; k < run && (int)t.size() < n; k++) t.push_back(x);
      x += q + (law == "dupgrid" ? 0 : r.range(-300, 300));
    }
  } else if (law == "driftm1") t = grid(r, n, origin, q - 1, 100);
  else if (law == "driftp1") t = grid(r, n, origin, q + 1, 100);
  else if (law == "driftm5") t = grid(r, n, origin, q - 5, 0);
  else if (law == "driftp5") t = grid(r, n, origin, q + 5, 0);
  else if (law == "dups") {
    // a late row and the next, early one share a timestamp: 0.55 q after one
    // grid point is 0.45 q before the next
    t = grid(r, n, origin, q, 50);
    for (int i = 0; i + 1 < n; i += (int)r.range(2, 5)) {
      t[(size_t)i] = origin + q * i + (q * 11) / 20;
      t[(size_t)i + 1] = t[(size_t)i];
    }
  } else if (law == "irregular") {
    int64_t x = origin;
    for (int i = 0; i < n; i++) { t.push_back(x); x += r.range(1, 40000); }
  } else if (law == "interval10s") {
    t = grid(r, n, origin, 10000, 300);
  } else if (law == "widejitter") {        // residuals around +-0.6 q
    t = grid(r, n, origin, q, 9000);
  }
  for (size_t i = 1; i < t.size(); i++)        // nondecreasing, like the store
    if (t[i] < t[i - 1]) t[i] = t[i - 1];
  if (from_row0)
    for (size_t i = t.size(); i-- > 0;) t[i] -= t[0];
  return t;
}

// offsets as window_bounds.h takes them: exactly max(n, 4) elements (the
// header's contract), so an over-read is an address-sanitizer error; cells
// past n hold garbage on purpose
inline std::vector<int32_t> tso_exact(const std::vector<int64_t>& t, Rng& r) {
  const size_t n = t.size();
  std::vector<int32_t> tso(n > 4 ? n : 4);
  for (size_t i = 0; i < tso.size(); i++)
    tso[i] = i < n ? (int32_t)t[i] : (int32_t)(r.next() & 1 ? INT32_MIN : 12345);
  return tso;
}

// ---- reporting --------------------------------------------------------------
// "<key>=<name> k=v k=v ..." on stdout: the line the host tests parse
struct KV { const char* k; long long v; };
inline void report_line(const char* key, const char* name, std::initializer_list<KV> kvs) {
  printf("%s=%s", key, name);
  for (const KV& kv : kvs) printf(" %s=%lld", kv.k, kv.v);
  printf("\n");
}

// counts a mismatch; the first ten of a tally go to stderr
template <class Count>
#if defined(__GNUC__)
__attribute__((format(printf, 2, 3)))
#endif
inline void mismatch(Count& bad, const char* fmt, ...) {
  if (bad < 10) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
  }
  bad++;
}

// exit status 0 = no mismatch; `verdict` also prints OK / FAILED
inline int exit_status(long long bad, bool verdict = false) {
  if (verdict) printf(bad ? "FAILED\n" : "OK\n");
  return bad == 0 ? 0 : 1;
}

}  // namespace kit
