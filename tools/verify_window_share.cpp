// Host verification of the fast scan kernel's SHARED window search
// (filodb_amd/csrc/window_bounds.h: fdb_bound_s_from_e; scan_fast.hip's
// window phase): when the query window is m whole steps, window w starts at
// the offset where window w-m ends, so only window ENDS are searched and each
// start row is handed over from the lane that searched that offset.
//
//   c++ -O2 -std=c++17 -o verify_window_share tools/verify_window_share.cpp
//   ./verify_window_share           # exit 0 = no mismatch
//
// Two checks per timestamp class, both against a brute-force linear scan:
//  * the derivation alone: s(y) from the end search at y, over row-adjacent,
//    random, grid and far-outside offsets ("offsets=", with the number of
//    exact ties and of ties inside a run of equal timestamps);
//  * the kernel's exchange, as a plain loop over 64 lanes x 4 slots x tiles
//    with the same seed, sender select and source lane ("windows="): m in
//    {1, 2, 20, 40, 63, 64}, 1..600 windows, query starts before, inside
//    (window edges placed exactly on rows and on duplicate runs) and after
//    the chunk.
// One line per class: "class=<name> offsets=<n> ties=<n> dupties=<n>
// windows=<n> wties=<n> wdupties=<n> mismatches=<n>" (wties/wdupties: windows
// whose start edge fell exactly on a row / on a run of equal rows).
// tests/test_window_share_host.py builds and runs this.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../filodb_amd/csrc/window_bounds.h"
#include "verify_kit.h"

namespace {

using kit::Rng;
using kit::brute_e;
using kit::brute_s;

const int kSizes[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 240, 400};
const int kRatios[] = {1, 2, 20, 40, 63, 64};
const int kWindows[] = {1, 64, 65, 256, 257, 600};

struct Tally {
  long offsets = 0, ties = 0, dupties = 0;        // derivation check
  long windows = 0, wties = 0, wdupties = 0;      // exchange check
  long bad = 0;
};

void report(const char* cls, int n, const char* what, long long a, long long b,
            int got, int want, Tally& ty) {
  kit::mismatch(ty.bad, "MISMATCH class=%s n=%d %s (%lld, %lld): got %d want %d\n",
                cls, n, what, a, b, got, want);
}

// what a lane keeps from the end search at offset x: e(x), tso[e], and the
// start row AT x (s(x), with its timestamp) for the window that starts there
struct EndSearch { int e; int32_t t2; int s_at_end; int32_t t_at_end; };

EndSearch end_search(const std::vector<int32_t>& tso, int n, FdbLin lin,
                     int64_t x) {
  EndSearch r;
  int32_t t_next = 0;
  r.t2 = 0;
  r.t_at_end = 0;
  r.e = fdb_bound_core(tso.data(), n, lin, x, &r.t2, &t_next, nullptr);
  r.s_at_end = fdb_bound_s_from_e(tso.data(), n, lin, x, r.e, r.t2, t_next,
                                  &r.t_at_end);
  return r;
}

// the derivation alone, over a list of offsets
void check_offsets(const char* cls, const std::vector<int32_t>& tso, int n,
                   FdbLin lin, const std::vector<int64_t>& ys, Tally& ty) {
  for (int64_t y : ys) {
    const EndSearch r = end_search(tso, n, lin, y);
    const int want = brute_s(tso.data(), n, y);
    ty.offsets++;
    if (r.e >= 0 && tso[r.e] == y) {
      ty.ties++;
      if (r.e > 0 && tso[r.e - 1] == tso[r.e]) ty.dupties++;
    }
    if (r.e != brute_e(tso.data(), n, y)) report(cls, n, "e(y)", y, 0, r.e, brute_e(tso.data(), n, y), ty);
    else if (r.s_at_end != want) report(cls, n, "s(y)", y, 0, r.s_at_end, want, ty);
    else if (want < n && r.t_at_end != tso[want])
      report(cls, n, "tso[s(y)]", y, 0, r.t_at_end, tso[want], ty);
  }
}

// the kernel's window phase: lanes own windows lane + 64k of a 256-window
// tile, slots run in order, the start row of window w comes from the lane
// that searched the end of window w-m
void check_exchange(const char* cls, const std::vector<int32_t>& tso, int n,
                    FdbLin lin, int64_t Ae, int64_t qstep, int m,
                    int num_windows, Tally& ty) {
  const int64_t qwindow = (int64_t)m * qstep;
  int s_prev[64], s_cur[64], e_cur[64];
  int32_t t2_cur[64];
  for (int lane = 0; lane < 64; lane++)          // slot -1: windows -64..-1
    s_prev[lane] = end_search(tso, n, lin, (int64_t)(lane - 64) * qstep - Ae).s_at_end;
  for (int tb = 0; tb < num_windows; tb += 256) {
    const int tn = num_windows - tb < 256 ? num_windows - tb : 256;
    for (int k = 0; k < 4; k++) {
      if (64 * k >= tn) continue;                // wave-uniform skip
      for (int lane = 0; lane < 64; lane++) {    // every lane searches
        const int w = tb + lane + 64 * k;
        const EndSearch r = end_search(tso, n, lin, (int64_t)w * qstep - Ae);
        e_cur[lane] = r.e; t2_cur[lane] = r.t2; s_cur[lane] = r.s_at_end;
      }
      int send[64];
      for (int lane = 0; lane < 64; lane++)
        send[lane] = lane < 64 - m ? s_cur[lane] : s_prev[lane];
      for (int lane = 0; lane < 64; lane++) {
        const int wi = lane + 64 * k;
        if (wi >= tn) continue;
        const int w = tb + wi;
        const int64_t x = (int64_t)w * qstep - Ae;
        const int s = send[(lane - m) & 63];
        const int e = e_cur[lane];
        const int we = brute_e(tso.data(), n, x), wsr = brute_s(tso.data(), n, x - qwindow);
        ty.windows++;
        if (wsr < n && tso[wsr] == x - qwindow) {      // start edge on a row
          ty.wties++;
          if (wsr + 1 < n && tso[wsr + 1] == tso[wsr]) ty.wdupties++;
        }
        if (s != wsr) report(cls, n, "window start (w, m)", w, m, s, wsr, ty);
        else if (e != we) report(cls, n, "window end (w, m)", w, m, e, we, ty);
        else if (e >= 0 && t2_cur[lane] != tso[e])
          report(cls, n, "tso[e] (w, m)", w, m, t2_cur[lane], tso[e], ty);
        else if (s < 0 || s > n)       // the kernel reads tso[s]: 0 <= s <= n
          report(cls, n, "start row range (w, m)", w, m, s, n, ty);
      }
      memcpy(s_prev, s_cur, sizeof s_prev);
    }
  }
}

}  // namespace

int main() {
  const char* classes[] = {"bench", "drop2", "drop10", "drop30", "grid",
                           "geometric", "clusters", "allequal", "dupruns",
                           "dupgrid"};
  long total_bad = 0;
  for (const char* cls : classes) {
    Tally ty;
    for (int n : kSizes) {
      Rng r{0x5eedULL * 1000003ULL + (uint64_t)n * 7919ULL + strlen(cls)};
      // scrape grid 15 s from 0, as offsets from row 0; exactly max(n, 4)
      // elements, so an over-read is an address-sanitizer error
      const std::vector<int32_t> tso =
          kit::tso_exact(kit::make_ts(cls, r, n, 0, 15000, true), r);
      const int64_t span = n > 0 ? tso[n - 1] : 0;
      const FdbLin lin = fdb_bounds_prepare(tso.data(), n);

      std::vector<int64_t> ys;
      for (int i = 0; i < n; i++)
        for (int d = -1; d <= 1; d++) ys.push_back((int64_t)tso[i] + d);
      for (int k = 0; k < 2000; k++) ys.push_back(r.range(-20000, span + 20000));
      for (int64_t w = -25; w <= (span / 15000 < 400 ? span / 15000 : 400) + 25; w++)
        ys.push_back(w * 15000);
      for (int sh = 20; sh <= 40; sh++)              // far outside the chunk
        for (int d = -1; d <= 1; d++) {
          ys.push_back(((int64_t)1 << sh) + d);
          ys.push_back(-((int64_t)1 << sh) + d);
          ys.push_back(span + ((int64_t)1 << sh) + d);
        }
      check_offsets(cls, tso, n, lin, ys, ty);

      // query steps: the scrape interval, and one that sweeps the whole span
      // in ~200 windows (the only one that reaches far rows of "clusters")
      const int64_t steps[] = {15000, span / 200 + 1};
      for (int64_t qstep : steps)
        for (int m : kRatios)
          for (int nw : kWindows) {
            const int64_t qwindow = (int64_t)m * qstep;
            // Ae = ts0 - qstart. Before: the query starts 3 windows ahead of
            // row 0 (and once 2^40 ms ahead). Inside: window 0 ends exactly
            // on a row (first, middle — inside a run for the duplicate
            // classes — and last), so window m starts exactly on it. After:
            // every window starts past the last row.
            std::vector<int64_t> aes = {3 * qwindow, (int64_t)1 << 40,
                                        -(span + qwindow + 1), -(span + qwindow)};
            if (n > 0) {
              aes.push_back(-(int64_t)tso[0]);
              aes.push_back(-(int64_t)tso[n / 2]);
              aes.push_back(-(int64_t)tso[n - 1]);
              aes.push_back(-(int64_t)tso[n / 2] + 7 * qstep);   // edge on a row mid-query
              aes.push_back(-(int64_t)tso[n / 2] - 1);
            }
            for (int64_t Ae : aes)
              check_exchange(cls, tso, n, lin, Ae, qstep, m, nw, ty);
          }
    }
    kit::report_line("class", cls,
                     {{"offsets", ty.offsets}, {"ties", ty.ties}, {"dupties", ty.dupties},
                      {"windows", ty.windows}, {"wties", ty.wties},
                      {"wdupties", ty.wdupties}, {"mismatches", ty.bad}});
    total_bad += ty.bad;
  }
  return kit::exit_status(total_bad);
}
