// Host verification of the fast rate kernel's lean epilogue and seed early-out
// (filodb_amd/csrc/rate_core.h, window_bounds.h; scan_fast.hip uses both).
// It compiles the shipped rule text itself — the headers below are the ones
// the kernels include — and checks three things; zero mismatches is the
// condition:
//
//  1. table:  d_div_small_int(si, k, RN(1/k)) == si / k for EVERY si =
//     d_div1000(ms), ms = 1..FDB_RATE_RTAB_MAX_MS (2^26), and every k =
//     1..FDB_RATE_RTAB-1 (255): 1.7e10 cases, the whole domain on which the
//     kernel takes the table path.
//  2. core:   d_extrapolate_core<true> == d_extrapolate_core<false> bit for
//     bit (NaN payloads included) on >= 1e9 inputs: random ones, and the
//     edges of the skipped division — v1 == delta, v1 one ulp and one unit
//     either side of delta, durationToStart == sampledInterval and one ms
//     either side, subnormal and huge delta, NaN/inf/negative values,
//     numSamples 2..400 (both sides of the table limit), isCounter both ways,
//     table limit on and off.
//  3. seed:   wherever fdb_windows_before_chunk(-1, qstep, Ae) holds, the
//     search it replaces returns e = -1 and start row 0 for each of windows
//     -64..-1, over the timestamp laws of verify_window_share.cpp with Ae
//     stepped across -qstep.
//
//   c++ -O3 -std=c++17 -ffp-contract=off -march=native -fopenmp
//       -o verify_rate_epilogue tools/verify_rate_epilogue.cpp   (one line)
//   ./verify_rate_epilogue          # full domain, under a minute on 8 cores
//   ./verify_rate_epilogue quick    # ms <= 2^16, 2e6 core inputs: for a
//                                   # -fsanitize=address,undefined build
// -ffp-contract=off is required: the rule rounds every product and sum.
// Last full run (2026-10-21): table bad=0 of 17112760320, core bad=0 of
// 1207959552 (skip taken on 26%, table on 70%), seed bad=0 of 266112 early
// lanes (542592 searched, 262791 of them with a nonzero start row).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../filodb_amd/csrc/rate_core.h"
#include "../filodb_amd/csrc/window_bounds.h"
#include "verify_kit.h"

namespace {

using kit::Rng;

uint64_t bits(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }

// ---- 1. the table quotient ---------------------------------------------------
long long check_table(int64_t max_ms, long long* cases) {
  double rk[FDB_RATE_RTAB];
  for (int k = 0; k < FDB_RATE_RTAB; k++) rk[k] = 1.0 / (double)k;
  long long bad = 0, n = 0;
#pragma omp parallel for reduction(+ : bad, n) schedule(static)
  for (int64_t ms = 1; ms <= max_ms; ms++) {
    const double si = d_div1000((double)ms);
    for (int k = 1; k < FDB_RATE_RTAB; k++) {
      const double q = d_div_small_int(si, (double)k, rk[k]);
      if (bits(q) != bits(si / (double)k)) bad++;
      n++;
    }
  }
  *cases = n;
  return bad;
}

// ---- 2. lean core against plain core ------------------------------------------
struct CoreIn {
  double dts, dte, si;
  int ns;
  double v1, v2;
  bool counter;
  int lim;
};

struct CoreTally { long long n = 0, bad = 0, skip = 0, table = 0; };

void check_core(const CoreIn& c, const double* rk, CoreTally& ty) {
  const double a = d_extrapolate_core<false>(c.dts, c.dte, c.si, c.ns, c.v1, c.v2,
                                             c.counter);
  const double b = d_extrapolate_core<true>(c.dts, c.dte, c.si, c.ns, c.v1, c.v2,
                                            c.counter, rk, c.lim);
  ty.n++;
  const double delta = c.v2 - c.v1;
  if (c.counter && delta > 0 && c.v1 >= delta && c.dts <= c.si) ty.skip++;
  if (c.ns - 1 < c.lim) ty.table++;
  if (bits(a) != bits(b)) {
#pragma omp critical
    kit::mismatch(ty.bad, "CORE MISMATCH dts=%a dte=%a si=%a ns=%d v1=%a v2=%a "
                  "counter=%d lim=%d: plain %a lean %a\n", c.dts, c.dte, c.si, c.ns,
                  c.v1, c.v2, (int)c.counter, c.lim, a, b);
  }
}

// a value pair of class `cls`: the classes walk the skip condition's edges
void make_values(Rng& r, int cls, double* v1, double* v2) {
  const double dmin = std::numeric_limits<double>::denorm_min();
  const double inf = std::numeric_limits<double>::infinity();
  switch (cls) {
    case 0: {            // integer counter, any relation of v1 to delta
      const double a = (double)r.range(0, 1 << 20), d = (double)r.range(0, 4000);
      *v1 = a; *v2 = a + d; break;
    }
    case 1: {            // v1 == delta exactly, and one unit either side
      const double a = (double)r.range(1, (int64_t)1 << 40);
      *v1 = a; *v2 = 2 * a + (double)r.range(-1, 1); break;
    }
    case 2: {            // v1 one ulp either side of delta (any binade)
      const double d = std::ldexp(1.0 + r.unit(), (int)r.range(-1000, 1000));
      const int side = (int)r.range(-1, 1);
      *v1 = side < 0 ? std::nextafter(d, 0.0) : side > 0 ? std::nextafter(d, inf) : d;
      *v2 = *v1 + d; break;
    }
    case 3: {            // subnormal v1 and delta, exact to the last bit
      const int64_t a = r.range(0, 1 << 12), d = r.range(0, 1 << 12);
      const int64_t dd = r.next() & 1 ? a + r.range(-1, 1) : d;
      *v1 = (double)a * dmin; *v2 = (double)(a + (dd < 0 ? 0 : dd)) * dmin; break;
    }
    case 4: {            // huge values: delta up to the overflow edge
      *v1 = std::ldexp(1.0 + r.unit(), (int)r.range(900, 1023));
      *v2 = std::ldexp(1.0 + r.unit(), (int)r.range(900, 1023)); break;
    }
    case 5: {            // non-integral gauge-like values, both signs
      *v1 = (r.unit() - 0.3) * std::ldexp(1.0, (int)r.range(-30, 60));
      *v2 = *v1 + (r.unit() - 0.3) * std::ldexp(1.0, (int)r.range(-30, 60)); break;
    }
    case 6: {            // subnormal delta under a normal v1 cannot exist
                         // (v2 - v1 is 0 or >= ulp(v1)): the smallest deltas
      *v1 = std::ldexp(1.0 + r.unit(), (int)r.range(-1022, 100));
      *v2 = std::nextafter(*v1, r.next() & 1 ? inf : -inf); break;
    }
    default: {           // specials
      const double sp[] = {0.0, -0.0, NAN, inf, -inf, dmin, 1.0,
                           std::numeric_limits<double>::max(),
                           std::numeric_limits<double>::min()};
      *v1 = sp[r.range(0, 8)]; *v2 = sp[r.range(0, 8)]; break;
    }
  }
}

CoreTally check_cores(long long rounds, int64_t max_ms) {
  double rk[FDB_RATE_RTAB];
  for (int k = 0; k < FDB_RATE_RTAB; k++) rk[k] = 1.0 / (double)k;
  CoreTally total;
  long long n = 0, bad = 0, skip = 0, table = 0;
#pragma omp parallel for reduction(+ : n, bad, skip, table) schedule(dynamic, 16)
  for (long long blk = 0; blk < rounds; blk++) {
    Rng r{0xc0ffeeULL + (uint64_t)blk * 0x1000193ULL};
    CoreTally ty;
    for (int it = 0; it < 4096; it++) {
      CoreIn c;
      // the kernel's domain: three integer ms gaps of one window
      const int64_t sampled = r.next() & 3 ? r.range(1, 600000) : r.range(1, max_ms);
      int64_t to_start;
      switch (r.next() & 7) {
        case 0: to_start = sampled; break;               // durationToStart == si
        case 1: to_start = sampled + 1; break;
        case 2: to_start = sampled > 1 ? sampled - 1 : 0; break;
        case 3: to_start = r.range(0, max_ms); break;    // often > sampled
        default: to_start = r.range(0, 20000); break;
      }
      const int64_t to_end = r.next() & 1 ? r.range(0, 20000) : r.range(0, max_ms);
      c.si = d_div1000((double)sampled);
      c.dts = d_div1000((double)to_start);
      c.dte = d_div1000((double)to_end);
      c.ns = (int)(r.next() & 1 ? r.range(2, 400) : r.range(2, 24));
      if ((r.next() & 15) == 0) c.ns = (int)r.range(FDB_RATE_RTAB - 1, FDB_RATE_RTAB + 2);
      c.lim = r.next() & 7 ? FDB_RATE_RTAB : 0;
      c.counter = (r.next() & 3) != 0;
      make_values(r, (int)(r.next() & 7), &c.v1, &c.v2);
      check_core(c, rk, ty);
    }
    n += ty.n; bad += ty.bad; skip += ty.skip; table += ty.table;
  }
  total.n = n; total.bad = bad; total.skip = skip; total.table = table;
  return total;
}

// ---- 3. the seed early-out -----------------------------------------------------
// six of verify_window_share.cpp's timestamp laws, offsets from row 0
const char* const kSeedLaws[] = {"bench", "grid", "drop30", "clusters", "allequal",
                                 "dupruns"};

struct SeedTally { long long early = 0, searched = 0, nonzero = 0, bad = 0; };

SeedTally check_seed() {
  SeedTally ty;
  const int sizes[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 240, 400};
  const int64_t steps[] = {1, 10, 1000, 15000, 60000, 3600000};
  for (int law = 0; law < 6; law++)
    for (int n : sizes) {
      Rng r{0x5eedULL + (uint64_t)law * 7919ULL + (uint64_t)n};
      const std::vector<int32_t> tso =      // max(n, 4) cells: the header's contract
          kit::tso_exact(kit::make_ts(kSeedLaws[law], r, n, 0, 15000, true), r);
      const FdbLin lin = fdb_bounds_prepare(tso.data(), n);
      for (int64_t qstep : steps) {
        std::vector<int64_t> aes;
        for (int64_t d = -3; d <= 3; d++) aes.push_back(-qstep + d);   // the edge
        for (int64_t d = -3; d <= 3; d++) aes.push_back(d);
        for (int m : {2, 20, 63, 64, 65})
          for (int64_t d = -1; d <= 1; d++) aes.push_back(-(int64_t)m * qstep + d);
        aes.push_back((int64_t)1 << 40);
        aes.push_back(-((int64_t)1 << 40));
        if (n > 0) aes.push_back(-(int64_t)tso[n - 1] - qstep);
        for (int64_t Ae : aes) {
          const bool early = fdb_windows_before_chunk(-1, qstep, Ae);
          for (int lane = 0; lane < 64; lane++) {
            // FastBounds::end_search at w = lane - 64
            const int64_t x = (int64_t)(lane - 64) * qstep - Ae;
            int32_t t2 = 0, t_next = 0, unused = 0;
            const int e = fdb_bound_core(tso.data(), n, lin, x, &t2, &t_next, nullptr);
            const int s = fdb_bound_s_from_e(tso.data(), n, lin, x, e, t2, t_next,
                                             &unused);
            if (early) {
              ty.early++;
              if (e != -1 || s != 0)
                kit::mismatch(ty.bad, "SEED MISMATCH law=%d n=%d qstep=%lld Ae=%lld "
                              "lane=%d: e=%d s=%d\n", law, n, (long long)qstep,
                              (long long)Ae, lane, e, s);
            } else {
              ty.searched++;
              if (s != 0) ty.nonzero++;
            }
          }
        }
      }
    }
  return ty;
}

}  // namespace

int main(int argc, char** argv) {
  const bool quick = argc > 1 && strcmp(argv[1], "quick") == 0;
  const int64_t max_ms = FDB_RATE_RTAB_MAX_MS;

  long long tcases = 0;
  const long long tbad = check_table(quick ? (int64_t)1 << 16 : max_ms, &tcases);
  printf("table bad=%lld of %lld (ms <= %lld, k < %d)\n", tbad, tcases,
         (long long)(quick ? (int64_t)1 << 16 : max_ms), FDB_RATE_RTAB);

  const CoreTally ct = check_cores(quick ? 512 : 294912, max_ms);
  printf("core bad=%lld of %lld (skip taken on %lld, table on %lld)\n", ct.bad,
         ct.n, ct.skip, ct.table);

  const SeedTally st = check_seed();
  printf("seed bad=%lld of %lld early lanes (%lld searched, %lld of them "
         "nonzero)\n", st.bad, st.early, st.searched, st.nonzero);
  // a check that never takes the path it guards proves nothing
  const bool vacuous = ct.skip == 0 || ct.table == 0 || st.early == 0 ||
                       st.nonzero == 0;
  if (vacuous) fprintf(stderr, "a guarded path was never taken\n");
  return kit::exit_status(tbad || ct.bad || st.bad || vacuous);
}
