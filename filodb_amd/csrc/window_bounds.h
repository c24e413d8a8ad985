// Window row bounds over one chunk's sorted timestamp offsets: for a time
// offset x (relative to the chunk's first timestamp, like tso[])
//
//   fdb_bound_e(x) = largest  row i with tso[i] <= x, or -1 if there is none
//   fdb_bound_s(y) = smallest row i with tso[i] >= y, or  n if there is none
//
// (WindowedChunkIterator's endRow/startRow, ChunkSetInfo.scala:467-511; rows
// with equal timestamps resolve to the largest index for e and the smallest
// for s.) For integer timestamps s(y) = e(y - 1) + 1, so one search serves both.
// And s(y) follows from the end search at the SAME offset, e(y), with at most
// one extra read (fdb_bound_s_from_e): where the query window is a whole
// number of steps, a window's start offset is an earlier window's end offset,
// and the start search is not repeated at all.
//
// Scrape timestamps are close to linear in the row index, so a bound is found
// by a linear guess, one secant correction from the guessed row's own
// timestamp, and a four-row probe around the corrected guess: a short fixed
// number of independent reads instead of a dependent binary-search chain. The
// floating-point arithmetic only steers the guess; the result is accepted on
// an exact integer predicate over the probed rows, and a bound the probe does
// not bracket falls back to a plain binary search (the "residue" path), so
// the answer is exact for ANY sorted tso[].
//
// Where the query step matches the series' scrape grid no search is needed
// at all: the second half of this header (fdb_aligned_*) decides that per
// series from the chunk descriptor's residual range and gives both bounds by
// one comparison each.
//
// Compiles as device code under hipcc and as plain host C++ (no HIP runtime
// needed) — tools/verify_window_bounds.cpp checks it against a linear scan,
// tools/verify_aligned_bounds.cpp the aligned half.
//
// Contract: tso[0..n) sorted ascending with tso[0] >= 0, and the array has at
// least 4 readable elements whatever n is (the probe reads a clamped 4-row
// span; elements at index >= n are read but never interpreted).
#ifndef FDB_WINDOW_BOUNDS_H
#define FDB_WINDOW_BOUNDS_H

#include <cstdint>

#ifdef __HIPCC__
#define FDB_HD __host__ __device__
#else
#define FDB_HD
#endif

// per-series constants of the linear guess, computed once per series
// (wave-uniform on the device): the last timestamp and the rows-per-unit-time
// slope. The slope is 0 for a degenerate span — every guess is then row 0 and
// the probe/residue path does the work.
struct FdbLin {
  int32_t last;     // tso[n-1], 0 when n == 0
  float inv_h;      // (n-1) / tso[n-1], 0 when n < 2 or tso[n-1] == 0
};

FDB_HD inline FdbLin fdb_bounds_prepare(const int32_t* tso, int n) {
  FdbLin lin;
  lin.last = n > 0 ? tso[n - 1] : 0;
  lin.inv_h = (n >= 2 && lin.last > 0) ? (float)(n - 1) / (float)lin.last : 0.0f;
  return lin;
}

// residue path: largest i in [-1, n) with tso[i] <= x (<= 9 steps at n <= 400)
FDB_HD inline int fdb_bound_search(const int32_t* tso, int n, int32_t x) {
  int lo = 0, hi = n;            // invariant: tso[<lo] <= x < tso[>=hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tso[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// e(x) plus the timestamps the probe already holds: *t_e = tso[e] when e >= 0,
// *t_next = tso[e+1] when e+1 < n (unspecified otherwise). `residue`, when
// non-null, is incremented if the binary-search fallback ran.
FDB_HD inline int fdb_bound_core(const int32_t* tso, int n, FdbLin lin,
                                 int64_t x, int32_t* t_e, int32_t* t_next,
                                 int* residue) {
  // clamp in i64 before narrowing: x may lie far outside the chunk. e(x) is
  // constant below -1 and above the last timestamp, so the clamp is exact.
  const float inv_h = lin.inv_h;
  int64_t xl = x < -1 ? -1 : x;
  if (xl > lin.last) xl = lin.last;
  const int32_t xc = (int32_t)xl;
  const int top = n > 0 ? n - 1 : 0;

  // linear guess, then one secant step from the guessed row's timestamp
  // (differences via unsigned wrap: they only steer, never decide)
  int g = (int)((float)xc * inv_h);
  g = g < 0 ? 0 : (g > top ? top : g);
  const int32_t d = (int32_t)((uint32_t)xc - (uint32_t)tso[g]);
  g += (int)__builtin_floorf((float)d * inv_h);
  g = g < 0 ? 0 : (g > top ? top : g);

  // probe rows b0..b0+3 (covers g-1..g+2 away from the ends); le_k says
  // "row b0+k exists and is <= x", non-increasing in k for sorted input
  const int bmax = n > 4 ? n - 4 : 0;
  int b0 = g - 1;
  b0 = b0 < 0 ? 0 : (b0 > bmax ? bmax : b0);
  const int32_t v0 = tso[b0], v1 = tso[b0 + 1], v2 = tso[b0 + 2], v3 = tso[b0 + 3];
  const bool le0 = b0 < n && v0 <= xc;
  const bool le1 = b0 + 1 < n && v1 <= xc;
  const bool le2 = b0 + 2 < n && v2 <= xc;
  const bool le3 = b0 + 3 < n && v3 <= xc;
  const int c = (int)le0 + (int)le1 + (int)le2 + (int)le3;
  int e = b0 - 1 + c;
  // exact acceptance: the row below the span is <= x (or there is none), and
  // the row above e is > x (or e is the last row)
  const bool ok = (le0 || b0 == 0) && (!le3 || b0 + 3 >= n - 1);
  *t_e = c == 1 ? v0 : (c == 2 ? v1 : (c == 3 ? v2 : v3));
  *t_next = c == 0 ? v0 : (c == 1 ? v1 : (c == 2 ? v2 : v3));
  if (!ok) {
    e = fdb_bound_search(tso, n, xc);
    if (e >= 0) *t_e = tso[e];
    if (e + 1 < n) *t_next = tso[e + 1];
    if (residue) ++*residue;
  }
  return e;
}

// endRow: largest i with tso[i] <= x (-1 = none); *t = tso[e] when e >= 0
FDB_HD inline int fdb_bound_e(const int32_t* tso, int n, FdbLin lin, int64_t x,
                              int32_t* t, int* residue = nullptr) {
  int32_t unused;
  return fdb_bound_core(tso, n, lin, x, t, &unused, residue);
}

// startRow: smallest i with tso[i] >= y (n = none); *t = tso[s] when s < n
FDB_HD inline int fdb_bound_s(const int32_t* tso, int n, FdbLin lin, int64_t y,
                              int32_t* t, int* residue = nullptr) {
  int32_t unused;
  return fdb_bound_core(tso, n, lin, y - 1, &unused, t, residue) + 1;
}

// startRow at offset y from the END search at the same offset: E = e(y),
// t_e = tso[E] (valid when E >= 0), t_next = tso[E+1] (valid when E+1 < n),
// exactly as fdb_bound_core hands them back. Returns s(y), the smallest row
// with tso >= y (n = none); *t1 = tso[s] when s < n.
//
//   no row sits exactly on y (E < 0 or t_e != y): every row up to E is < y,
//     so s = E + 1 and tso[s] = t_next — no memory access at all
//   t_e == y, and row E-1 is smaller (or E == 0): s = E — one read
//   t_e == y inside a run of equal timestamps: the run's first row, by the
//     full search (fdb_bound_s)
//
// The fast scan kernel uses this to share searches between windows: when the
// window length is m query steps, window w starts where window w-m ends, so
// w's start row follows from the end search w-m already did.
FDB_HD inline int fdb_bound_s_from_e(const int32_t* tso, int n, FdbLin lin,
                                     int64_t y, int E, int32_t t_e,
                                     int32_t t_next, int32_t* t1,
                                     int* residue = nullptr) {
  int s = E + 1;
  *t1 = t_next;
  if (E >= 0 && (int64_t)t_e == y) {
    if (E == 0 || tso[E - 1] < t_e) {
      s = E;
      *t1 = t_e;
    } else {
      s = fdb_bound_s(tso, n, lin, y, t1, residue);
    }
  }
  return s;
}

// True when every window up to index w_last (wEnd(w) = qstart + w*qstep,
// qstep > 0, Ae = ts0 - qstart) ends before the chunk's first row: its end
// offset w_last*qstep - Ae is negative and tso[0] >= 0, so for each of them
// e = -1 and the start row at that offset is 0, with no search. The fast scan
// kernel's shared search asks this for its seed slot (w_last = -1).
FDB_HD inline bool fdb_windows_before_chunk(int64_t w_last, int64_t qstep,
                                            int64_t Ae) {
  return w_last * qstep - Ae < 0;
}

// ---- direct window rows: the query step matches the scrape grid -------------
//
// Window w ends at offset x_w = w*q - A (q = query step, A = ts0 - qstart)
// and, the window being m whole steps, starts at y = x_(w-m). Write
//
//   u_i = tso[i] + A - (i + k0)*q        for one integer k0 per series.
//
// Condition C(k0): -q < u_i < q for every row i < n — row i lies strictly
// within one step of window edge i + k0. Under C, with j = w - k0:
//
//   rows <= j-1 have u < q:   tso[i] < (i+k0+1)*q - A <= x_w
//   rows >= j+1 have u > -q:  tso[i] > (i+k0-1)*q - A >= x_w
//
// so only row j can sit on either side of (or exactly on) the edge:
//
//   e(x_w) = j - [tso[j] > x_w]     largest row with tso <= x_w
//   s(x_w) = j + [tso[j] < x_w]     smallest row with tso >= x_w
//
// both with j clamped into [0, n-1], which stays exact: for j < 0, row 0 has
// tso[0] > (k0-1)*q - A >= x_w, so e = -1 and s = 0; for j > n-1, row n-1
// has tso[n-1] < (n+k0)*q - A <= x_w, so e = n-1 and s = n. Equal timestamps
// and rows exactly on an edge need no special case (the two formulas are
// independent, neither is derived from the other), and nothing here needs
// tso[] to be sorted. The timestamp at the bound is one of two neighbouring
// cells, fetched together: tso[j-1], tso[j] for the end (tso[-1] must be
// readable; its value is never used: it is handed back only with e = -1) and
// tso[j], tso[j+1] for the start (tso[n] must be readable, as above).
//
// C is decided per series without touching a row. The chunk's descriptor
// gives tso[i] = ts_base + ts_slope*i + inner[i] with rmin <= inner[i] <=
// rmax (fast_desc.h), hence u_i = C0 + d*i + inner[i] with C0 = ts_base + A -
// k0*q and d = ts_slope - q, and over 0 <= i <= n-1
//
//   lo = C0 + rmin + min(0, (n-1)*d) <= u_i <= C0 + rmax + max(0, (n-1)*d) = hi.
//
// lo > -q and hi < q imply C: sufficient, not necessary (tight when d == 0).
// k0 is steered by a float estimate; correctness rests on the integer test.
// The query must also keep every window offset of the launch inside i32, so
// that the per-window arithmetic is i32: x_w for w in [0, nw) and the
// earliest start x_(-m).
struct FdbAligned {
  bool ok;          // take the direct path
  int32_t k0;       // row i belongs to window edge i + k0
  int32_t x0;       // x_0 = -A
};

// k0 ~ round((ts_base + A + (rmin+rmax)/2) / q); inv_q = 1/q. INT32_MIN when
// the estimate is out of range (the test then rejects).
FDB_HD inline int32_t fdb_aligned_guess(int32_t ts_base, int32_t rmin, int32_t rmax,
                                        int64_t A, float inv_q) {
  const float k = __builtin_rintf(
      ((float)(A + ts_base) + 0.5f * (float)(rmin + rmax)) * inv_q);
  return (k > -1.0e9f && k < 1.0e9f) ? (int32_t)k : INT32_MIN;
}

// The exact test: integers only. m = window / q (whole), nw = windows of the
// launch. |A| < 2^40 and q < 2^30 keep every product below inside i64.
FDB_HD inline FdbAligned fdb_aligned_test(int n, int32_t ts_base, int32_t ts_slope,
                                          int32_t rmin, int32_t rmax, int64_t A,
                                          int64_t q, int64_t m, int64_t nw,
                                          int32_t k0) {
  FdbAligned al{false, k0, (int32_t)(uint32_t)(0 - (uint64_t)A)};
  const int64_t lim = (int64_t)1 << 40;
  if (n < 1 || rmin > rmax || k0 == INT32_MIN || q < 1 || q >= ((int64_t)1 << 30) ||
      m < 1 || m > 64 || nw < 1 || nw >= ((int64_t)1 << 30) || A <= -lim || A >= lim)
    return al;
  const int64_t x_first = -m * q - A, x_last = (nw - 1) * q - A;
  if (x_first < INT32_MIN || x_last > INT32_MAX) return al;
  const int64_t d = (int64_t)ts_slope - q, dn = (int64_t)(n - 1) * d;
  const int64_t C0 = (int64_t)ts_base + A - (int64_t)k0 * q;
  const int64_t lo = C0 + rmin + (dn < 0 ? dn : 0);
  const int64_t hi = C0 + rmax + (dn > 0 ? dn : 0);
  al.ok = lo > -q && hi < q;
  return al;
}

// Row j of edge index w, clamped into [0, n-1] (n >= 1)
FDB_HD inline int fdb_aligned_row(int n, int32_t k0, int w) {
  const int j = w - k0;
  return j < 0 ? 0 : (j > n - 1 ? n - 1 : j);
}

// endRow from row j = fdb_aligned_row(w) and the cells below = tso[j-1],
// at = tso[j] (x = x_w as i32): largest row with tso <= x, -1 = none;
// *t2 = tso[e] when e >= 0
FDB_HD inline int fdb_aligned_e_pick(int j, int32_t below, int32_t at, int32_t x,
                                     int32_t* t2) {
  const bool gt = at > x;
  *t2 = gt ? below : at;
  return j - (int)gt;
}

// startRow from row j = fdb_aligned_row(w - m) and the cells at = tso[j],
// above = tso[j+1] (y = x_(w-m) as i32): smallest row with tso >= y,
// n = none; *t1 = tso[s] when s < n
FDB_HD inline int fdb_aligned_s_pick(int j, int32_t at, int32_t above, int32_t y,
                                     int32_t* t1) {
  const bool lt = at < y;
  *t1 = lt ? above : at;
  return j + (int)lt;
}

// Both bounds of window w (m steps long; x = x_w, y = x_(w-m) as i32). The
// four cells are loaded before either comparison, so the two reads are in
// flight together. tso[-1] and tso[n] must be readable (never interpreted).
FDB_HD inline void fdb_aligned_bounds(const int32_t* tso, int n, int32_t k0, int w,
                                      int m, int32_t x, int32_t y, int* e, int* s,
                                      int32_t* t1, int32_t* t2) {
  const int je = fdb_aligned_row(n, k0, w), js = fdb_aligned_row(n, k0, w - m);
  const int32_t e_below = tso[je - 1], e_at = tso[je];
  const int32_t s_at = tso[js], s_above = tso[js + 1];
  *e = fdb_aligned_e_pick(je, e_below, e_at, x, t2);
  *s = fdb_aligned_s_pick(js, s_at, s_above, y, t1);
}

#endif  // FDB_WINDOW_BOUNDS_H
