// Fast scan kernel: the single-chunk-per-series shape (BASELINE configs[1-3]).
//
// One wave per series: decode the chunk into LDS, build the kind's per-row
// structures (meta), then evaluate 4 windows per lane.
//
//  * per-series bookkeeping comes from a descriptor table built once at
//    upload (fast_desc.h): sealed chunks never change, so the directory row
//    and both vector headers are parsed on the host into one 64-byte record
//    per series — payload offsets, row count (row guards already decided),
//    wire-format class / nbits / sign, drop bit, ts0, timestamp base and
//    slope and residual range, value init and slope, val_exact32. The kernel
//    loads desc[sid] through a wave-uniform address and goes straight to the
//    payload: two dependent memory trips per series instead of the four of
//    series_first -> directory row -> 32-B headers -> payload
//  * packed 8/16-bit delta-delta vectors decode four rows per lane (one
//    payload load, 128-bit LDS stores, no per-row guard; scan_common.h), the
//    values in exact i32 + f64 arithmetic where val_exact32 holds
//  * each window's row range [startRow, endRow] is computed directly in the
//    window phase (window_bounds.h): a linear guess from the series' mean
//    scrape interval, one secant correction, a four-row LDS probe and an
//    exact integer acceptance test, with a binary search for the rare bound
//    the probe does not bracket — a short fixed number of independent LDS
//    reads per bound, exact for arbitrary sorted timestamps (replaces
//    DeltaDeltaDataReader.binarySearch/ceilingIndex on the device; semantics:
//    WindowedChunkIterator, ChunkSetInfo.scala:467-511). Earlier designs: a
//    per-window binary search (~9 dependent LDS reads per bound, round 1) and
//    a rows→windows inversion scan through per-window LDS arrays (round 2);
//    profiles/README.md has the measurements.
//  * when the query window is m = 1..64 whole steps (rate()[5m] at step 15 s:
//    m = 20), window w starts at the offset where window w-m ends, so the
//    SHARE instantiations search only each window's END: the start row at
//    that same offset follows from what the probe already holds
//    (fdb_bound_s_from_e: no read, or one read when a row sits exactly on
//    the edge) and travels to the lane that owns window w+m through one
//    ds_bpermute — five searches per lane and tile instead of eight, no LDS
//    array. Any other window/step pair keeps two searches per window.
//  * where, in a SHARE build, the step also matches the series' scrape grid —
//    every row within one step of "its" window edge (window_bounds.h,
//    condition C; the commonest dashboard shape and the benchmark's) — there
//    is nothing to search: window w's end row is row w-k0 or the one before,
//    its start row is row w-m-k0 or the one after, one comparison each on two
//    neighbouring cells read together. The series is chosen per wave, in
//    scalar arithmetic, from the residual range the descriptor carries
//    (ts_rmin / ts_rmax, fast_desc.h), without touching a row; an aligned
//    series skips the last-row read, the slope divide, the seed search and
//    the exchange. Everything else — raw timestamp vectors, dropped scrapes,
//    another interval — keeps the search, series by series within one
//    launch. Holding both paths costs the searched series registers, so the
//    ALIGNED build is a template parameter picked per launch, where a host-
//    side sample of the descriptors says at least a quarter of the series
//    qualify under the query at hand; every other launch, and FDB_ALIGNED=0
//    (read at launch), takes the search-only build.
//  * timestamps live in LDS as i32 offsets from the chunk's first ts (halves
//    the LDS footprint and read traffic; chunk span is checked at upload)
//  * the extrapolatedRate epilogue keeps the oracle's exact operation
//    sequence (its threshold comparisons are discontinuous — see
//    fast_window_value), in the core's lean form: bit-identical, with the
//    avgDur division through a per-block reciprocal table and the v1/delta
//    division branched around where it provably decides nothing
//    (rate_core.h); AVG/STDDEV use a per-block reciprocal table of their own
//    (continuous, ≤2 ulp)
//  * window results are branch-lean selects; one store per window
//
// Per-window semantics are IDENTICAL to the round-1 kernel's single-chunk
// stage C (parity-green against the oracle): RateFunctions.scala:72-111,
// 230-289; AggrOverTimeFunctions.scala:553-605,924-1028,1082-1224;
// RangeFunction.scala:595-745. Rules the walk applies too are in
// window_funcs.h.
//
// EMIT=1 ("fused group" emit) folds fastReduce into the scan: each lane keeps
// its windows' group-partials in registers while the wave walks a contiguous
// slab of the group-sorted series index, flushing one atomicAdd burst per
// group change — the [S×W] intermediate grid of the two-phase reduce is never
// materialized (AggrOverRangeVectors.scala:320-377 semantics; raw sums +
// counts out, agg_present_kernel applies the presentation step).

#include <cstddef>
#include <cstring>
#include <cmath>

#include "engine_internal.h"
#include "fast_desc.h"
#include "window_bounds.h"

#define FAST_TILE 256        // windows per pass: 4 per lane, unrolled
#define FAST_WAVES 4
#define FAST_DROPS 32        // sparse counter-reset table capacity

// kinds (which auxiliary LDS arrays a function family needs)
#define K_RATE    0
#define K_PFX     1
#define K_PFX_SQ  2
#define K_MINMAX  3
#define K_CHANGES 4
#define K_LAST    5

template <int FUNC> struct FKind { static constexpr int v =
    (FUNC <= FN_DELTA) ? K_RATE :
    (FUNC == FN_SUM || FUNC == FN_AVG || FUNC == FN_COUNT ||
     FUNC == FN_RATE_OVER_DELTA) ? K_PFX :
    (FUNC == FN_STDDEV || FUNC == FN_STDVAR) ? K_PFX_SQ :
    (FUNC == FN_MIN || FUNC == FN_MAX) ? K_MINMAX :
    (FUNC == FN_CHANGES || FUNC == FN_RESETS) ? K_CHANGES :
    K_LAST; };   // incl. FN_IRATE / FN_IDELTA: the window's last two raw rows

template <int KIND>
struct alignas(16) FWs {            // per-wave LDS workspace; tso[] and val[]
                                    // start 16-B aligned and hold a multiple of
                                    // four rows (128-bit decode stores)
  // ts - ts0 (i32 offsets) in one array: four cells of front pad keep
  // tso()[-1] readable (the aligned end bound reads tso[j-1], tso[j] at j >= 0;
  // the value is never used) and tso() 16-B aligned; the back pad keeps
  // tso()[startRow] readable at startRow == n
  int32_t tsbuf[4 + FDB_DEFAULT_MAX_ROWS + 4];
  __device__ __forceinline__ int32_t* tso() { return tsbuf + 4; }
  __device__ __forceinline__ const int32_t* tso() const { return tsbuf + 4; }
  double  val[FDB_DEFAULT_MAX_ROWS];       // raw values, or prefix sums (PFX kinds)
  uint16_t cnt[(KIND == K_PFX || KIND == K_PFX_SQ || KIND == K_CHANGES)
                   ? FDB_DEFAULT_MAX_ROWS : 1];
  double  sq[KIND == K_PFX_SQ ? FDB_DEFAULT_MAX_ROWS : 1];
  double  grp[KIND == K_MINMAX ? (FDB_DEFAULT_MAX_ROWS + 7) / 8 : 1];
  int16_t dpos[KIND == K_RATE ? FAST_DROPS : 1];
  double  dcum[KIND == K_RATE ? FAST_DROPS : 1];
};

// A descriptor as the kernel holds it: the record's first twelve dwords,
// loaded as whole dwords through a wave-uniform address (scalar loads have
// no sub-dword form; a u16/u8 field read would fall back to vector loads and
// drag everything derived from it into VGPRs). Little-endian field views.
struct FDesc {
  uint32_t w[12];
  __device__ __forceinline__ int n() const { return (int)(w[2] & 0xffff); }
  __device__ __forceinline__ int ts_cls() const { return (int)((w[2] >> 16) & 0xff); }
  __device__ __forceinline__ int ts_nbits() const { return (int)(w[2] >> 24); }
  __device__ __forceinline__ int ts_flags() const { return (int)(w[3] & 0xff); }
  __device__ __forceinline__ int val_cls() const { return (int)((w[3] >> 8) & 0xff); }
  __device__ __forceinline__ int val_nbits() const { return (int)((w[3] >> 16) & 0xff); }
  __device__ __forceinline__ int val_flags() const { return (int)(w[3] >> 24); }
  __device__ __forceinline__ int64_t ts0() const {
    return (int64_t)(((uint64_t)w[5] << 32) | w[4]); }
  __device__ __forceinline__ int32_t ts_base() const { return (int32_t)w[6]; }
  __device__ __forceinline__ int32_t ts_slope() const { return (int32_t)w[7]; }
  __device__ __forceinline__ int64_t val_init() const {
    return (int64_t)(((uint64_t)w[9] << 32) | w[8]); }
  __device__ __forceinline__ int32_t val_slope() const { return (int32_t)w[10]; }
  __device__ __forceinline__ int32_t ts_rmin() const { return (int32_t)(int16_t)(w[11] & 0xffff); }
  __device__ __forceinline__ int32_t ts_rmax() const { return (int32_t)w[11] >> 16; }
};
static_assert(offsetof(FdbFastDesc, n) == 8 && offsetof(FdbFastDesc, ts_flags) == 12 &&
              offsetof(FdbFastDesc, ts0) == 16 && offsetof(FdbFastDesc, ts_base) == 24 &&
              offsetof(FdbFastDesc, val_init) == 32 && offsetof(FdbFastDesc, val_slope) == 40 &&
              offsetof(FdbFastDesc, ts_rmin) == 44 && offsetof(FdbFastDesc, ts_rmax) == 46,
              "FDesc's dword views follow FdbFastDesc's layout");

// series bookkeeping: one 64-B descriptor per series (fast_desc.h), parsed
// from the vector headers once at upload, fetched here with one scalar load
// through a wave-uniform address — the payload is the only dependent trip
// behind it. (Requesting desc[next sid] a series early, held in SGPRs, in
// VGPRs, or only touched into cache, measured 0.01-0.02 ms SLOWER on
// rate_1m than this plain load: at 7 waves/SIMD the second trip is hidden
// already. profiles/README.md, round 5.)
__device__ __forceinline__ FDesc fast_load_desc(const FdbFastDesc* desc, int s) {
  const uint4* p = reinterpret_cast<const uint4*>(desc + s);
  const uint4 a = p[0], b = p[1], c = p[2];
  return FDesc{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w}};
}

// reciprocal table users: AVG/STDDEV/STDVAR index it by a sample count up to
// the row cap; the rate epilogue's lean core by numSamples-1 below
// FDB_RATE_RTAB, exactly (rate_core.h). 256 entries put the K_RATE block at
// 22,784 B of LDS, inside the 23,405 B that 7 blocks/CU leave each.
template <int KIND> constexpr bool needs_inv = KIND == K_PFX || KIND == K_PFX_SQ;
template <int KIND> constexpr int inv_entries =
    needs_inv<KIND> ? FDB_DEFAULT_MAX_ROWS + 2 : KIND == K_RATE ? FDB_RATE_RTAB : 0;

// wave-uniform constants of the query
struct FastQuery {
  int64_t qstep, qwindow;
  double rate_scale, dur_ms;     // 1000/qwindow, (double)qwindow
  bool qw32;                     // the window fits i32: i32 rate epilogue
  int rk_lim;                    // lean rate core: table entries usable at this
                                 // window length (0: it divides)
  float inv_qstep;               // steers the aligned path's k0 estimate
};

// TIMED: the s_memtime phase split (perf ablation: tools/perf_sweep.py sets
// q._pad = 8; result stores are suppressed and out[0..nwaves*4) receives each
// wave's cycles per phase). Untimed, every method is empty.
enum { PH_DECODE = 0, PH_META = 1, PH_BOUNDS = 2, PH_WINDOWS = 3 };
template <bool TIMED> struct FastTimer {
  uint64_t t[4] = {0, 0, 0, 0}, tt = 0;
  __device__ __forceinline__ void start() {
    if constexpr (TIMED) tt = __builtin_amdgcn_s_memtime();
  }
  __device__ __forceinline__ void lap(int phase) {
    if constexpr (TIMED) {
      const uint64_t now = __builtin_amdgcn_s_memtime();
      t[phase] += now - tt;
      tt = now;
    }
  }
  __device__ __forceinline__ void store(double* out, size_t gw, int lane) const {
    if constexpr (TIMED) {
      #pragma unroll
      for (int p = 0; p < 4; p++) if (lane == 0) out[gw * 4 + p] = (double)t[p];
    }
  }
};

// ---- decode: the single chunk into LDS (i32 ts offsets + f64 values) -------
// n == 0 is an empty series: no chunk, or a guard that upload decided (rows
// above the chunk cap, or more rows than the timestamp vector has). The
// packed 8/16-bit arms write whole 4-row groups (scan_common.h), so rows
// n..4*ceil(n/4)-1 of tso[] and val[] hold garbage. Nothing interprets them:
// the meta loops guard i < n, the bound search accepts rows < n only
// (window_bounds.h reads past n but never interprets it), every window row
// range keeps s <= e < n, and the one tso[s] read at s == n (shared_bounds;
// the aligned start bound's tso[j+1] at j == n-1) is readable and never used,
// like tso[-1] (FWs::tsbuf's front pad, the aligned end bound at j == 0).
struct FastChunk { int n; int64_t ts0; bool dropped; };

template <typename WS>
__device__ __forceinline__ FastChunk fast_decode(const FDesc& cd, const uint8_t* blob,
                                                 WS& ws, int lane) {
  const int n = cd.n();
  const int64_t ts0 = cd.ts0();
  const bool dropped = n > 0 && (cd.val_flags() & FDB_FD_DROPPED) != 0;
  if (n > 0) {
    // the decoders see the lane id through an opaque copy made here, per
    // series: otherwise every arm's lane-scaled blob address (blob + 8*lane,
    // + 4*lane, ...) is hoisted out of the series loop as a 64-bit VGPR pair
    // that stays live, or spilled, across the window phase
    int dl = lane;
    asm volatile("" : "+v"(dl));
    const uint8_t* tp = blob + ((size_t)cd.w[0] << 6);
    const uint8_t* vp = blob + ((size_t)cd.w[1] << 6);
    DVec tv;
    tv.wf = cd.ts_cls() == FDB_FD_PACKED ? FDB_WF_DDV
          : cd.ts_cls() == FDB_FD_CONST ? FDB_WF_DDV_CONST : FDB_WF_PRIM64;
    tv.idata = tp + (cd.ts_cls() == FDB_FD_PACKED
                         ? FDB_DDV_OFF_INNER + FDB_PRIM_OFF_DATA : FDB_PRIM_OFF_DATA);
    tv.init = ts0 + cd.ts_base();     // d_decode_ts_offsets takes init - ts0
    tv.slope = cd.ts_slope();
    tv.n = n; tv.nbits = (uint8_t)cd.ts_nbits();
    tv.sign = (cd.ts_flags() & FDB_FD_SIGN) != 0; tv.dropped = 0;
    d_decode_ts_offsets(tv, n, ts0, ws.tso(), dl);
    const int vcls = cd.val_cls(), vbits = cd.val_nbits();
    const bool vsign = (cd.val_flags() & FDB_FD_SIGN) != 0;
    const bool exact32 = (cd.val_flags() & FDB_FD_EXACT32) != 0;
    const uint8_t* vdata = vp + FDB_DDV_OFF_INNER + FDB_PRIM_OFF_DATA;
    if (vcls == FDB_FD_PACKED && vbits == 8) {
      d_decode_val4<8>(vdata, vsign, cd.val_init(), cd.val_slope(), exact32,
                       n, ws.val, dl);
    } else if (vcls == FDB_FD_PACKED && vbits == 16) {
      d_decode_val4<16>(vdata, vsign, cd.val_init(), cd.val_slope(), exact32,
                        n, ws.val, dl);
    } else {        // const DDV, raw f64, packed 2/4/32-bit: the common decoder
      DVec vv;
      vv.wf = vcls == FDB_FD_PACKED ? FDB_WF_DDV
            : vcls == FDB_FD_CONST ? FDB_WF_DDV_CONST : FDB_WF_PRIM64;
      vv.idata = vcls == FDB_FD_PACKED ? vdata : vp + FDB_PRIM_OFF_DATA;
      vv.init = cd.val_init(); vv.slope = cd.val_slope();
      vv.n = n; vv.nbits = (uint8_t)vbits; vv.sign = vsign; vv.dropped = dropped;
      d_decode_chunk<true>(vv, n, nullptr, ws.val, dl);
    }
  }
  return FastChunk{n, ts0, dropped};
}

// ---- meta: kind-specific per-row structures; K_RATE returns the reset table's
// entry count (0 when dense) and dense flag, the other kinds an empty scan
template <int KIND, int FUNC, typename WS>
__device__ __forceinline__ ResetScan fast_meta(WS& ws, int n, bool dropped, int lane) {
  ResetScan rs;
  if constexpr (KIND == K_RATE) {
    if (dropped && n > 0) {
      for (int base = 0; base < n; base += 64) {
        int i = base + lane;
        double raw = (i < n) ? ws.val[i] : 0;
        double x = (i < n && !isnan(raw)) ? raw : 0;
        d_reset_scan_step<FAST_DROPS>(rs, i, i < n, x, lane, ws.dpos, ws.dcum);
      }
      if (rs.dense) rs.count = 0;
    }
  }
  if constexpr (KIND == K_PFX || KIND == K_PFX_SQ) {
    double carry = 0, carry_sq = 0;
    int ccarry = 0;
    for (int base = 0; base < n; base += 64) {
      int i = base + lane;
      double raw = (i < n) ? ws.val[i] : NAN;
      bool ok = (i < n) && !isnan(raw);
      double x = ok ? raw : 0;
      double s = wave_incl_scan(x, lane);
      int cs = wave_incl_scan_i(ok ? 1 : 0, lane);
      double sqs = 0;
      if constexpr (KIND == K_PFX_SQ) sqs = wave_incl_scan(x * x, lane);
      __builtin_amdgcn_wave_barrier();        // all raw reads precede writes
      if (i < n) {
        ws.val[i] = carry + s;                // val[] becomes the prefix
        ws.cnt[i] = (uint16_t)(ccarry + cs);
        if constexpr (KIND == K_PFX_SQ) ws.sq[i] = carry_sq + sqs;
      }
      carry += __shfl(s, 63);
      ccarry += __shfl(cs, 63);
      if constexpr (KIND == K_PFX_SQ) carry_sq += __shfl(sqs, 63);
    }
  }
  if constexpr (KIND == K_MINMAX) {           // min/max of each 8-row group
    for (int base = 0; base < n; base += 64) {
      int i = base + lane;
      double x = (i < n) ? ws.val[i] : NAN;
      #pragma unroll
      for (int off = 1; off < 8; off <<= 1)
        d_fold_mm<FUNC == FN_MIN>(x, __shfl_xor(x, off));
      if ((lane & 7) == 0 && i < n) ws.grp[i >> 3] = x;
    }
  }
  if constexpr (KIND == K_CHANGES) {          // adjacent-pair indicator prefix
    int ccarry = 0;
    double carry_x = NAN;
    for (int base = 0; base < n; base += 64) {
      int i = base + lane;
      double x = (i < n) ? ws.val[i] : NAN;
      double px = __shfl_up(x, 1);
      if (lane == 0) px = carry_x;
      int ind = (i > 0 && i < n && d_pair_counts<FUNC == FN_RESETS>(x, px)) ? 1 : 0;
      int s = wave_incl_scan_i(ind, lane);
      if (i < n) ws.cnt[i] = (uint16_t)(ccarry + s);
      ccarry += __shfl(s, 63);
      carry_x = __shfl(x, 63);
    }
  }
  return rs;
}

// ---- bounds: window w's row range [s, e] -------------------------------------
// e = last row with ts <= wEnd, s = first row with ts >= wStart (sentinels
// e = -1 / s = n when there is none); t1/t2 are tso[s]/tso[e] as the probe
// loaded them (valid iff in range)
struct WB { int s, e; int32_t t1, t2; };

// One series' bound search (window_bounds.h). Window time base: wEnd(w) =
// qstart + w*qstep; offsets are vs ts0.
//
// Shared search (SHARE; wshare = m, window = m steps): window w starts at the
// offset where window w-m ends, so each lane searches only its windows' ENDS,
// derives the start row AT that same offset from what the probe already holds
// (fdb_bound_s_from_e) and hands it to the lane that owns window w+m. Windows
// sit at lane + 64k, so w-m is lane (lane-m)&63 of this slot when lane >= m
// and of the previous slot otherwise: the sender picks by lane < 64-m, one
// ds_bpermute delivers, and only the previous slot's start row stays live.
// Five searches per lane instead of eight: four ends plus the seed for the
// windows before the first tile.
//
// ALIGNED (a SHARE build that also holds the direct rows; chosen per launch,
// fdb_launch_fast_scan): each series is tested against condition C and takes
// the direct rows or the search. The plain SHARE build holds the search
// alone, so a launch the direct rows would not serve keeps that build's
// registers and instruction text.
template <bool SHARE, bool ALIGNED>
struct FastBounds {
  const int32_t* tso;
  int n, lane, wshare;
  FastQuery q;
  FdbLin lin;         // the last timestamp and the rows-per-ms slope, wave-uniform
  int64_t Ae;         // ts0 - qstart: wEnd >= ts  ⟺ w*qstep >= o+Ae
  int share_src;      // bpermute address
  int s_prev;         // start row at the end of this lane's window in the
                      // previous slot; slot -1 = windows -64..-1

  FdbAligned al;      // ALIGNED: the series takes the direct rows (wave-uniform)

  // nw: windows of the launch
  __device__ __forceinline__ FastBounds(const int32_t* tso_, int n_, int64_t Ae_,
                                        const FastQuery& q_, int wshare_, int lane_,
                                        const FDesc& cd, int nw)
      : tso(tso_), n(n_), lane(lane_), wshare(wshare_), q(q_), lin{0, 0.0f}, Ae(Ae_),
        share_src(((lane_ - wshare_) & 63) << 2), s_prev(0), al{false, 0, 0} {
    // the step matches this series' scrape grid (window_bounds.h, condition
    // C, decided from the descriptor in scalar arithmetic): each window's rows
    // come from one comparison, and the last-row read, the divide, the seed
    // search and the exchange below are all skipped
    if constexpr (ALIGNED) {
      const int32_t k0 = __builtin_amdgcn_readfirstlane(fdb_aligned_guess(
          cd.ts_base(), cd.ts_rmin(), cd.ts_rmax(), Ae, q.inv_qstep));
      al = fdb_aligned_test(n, cd.ts_base(), cd.ts_slope(), cd.ts_rmin(),
                            cd.ts_rmax(), Ae, q.qstep, wshare, nw, k0);
      if (al.ok) return;
    }
    const int32_t tlast = n > 0 ? tso[n - 1] : 0;
    lin.last = __builtin_amdgcn_readfirstlane(tlast);
    lin.inv_h = (n >= 2 && lin.last > 0) ? (float)(n - 1) / (float)lin.last : 0.0f;
    // the seed: slot -1's start rows. Where the series begins after window
    // -1 ends (wave-uniform; any series or chunk that starts inside the
    // queried range) every one of those searches finds no row, e = -1 and
    // s = 0: s_prev stays 0 and the fifth search is not run.
    if constexpr (SHARE) {
      if (!fdb_windows_before_chunk(-1, q.qstep, Ae)) {
        int32_t unused;
        end_search(lane - 64, &unused, &s_prev);
      }
    }
  }
  __device__ __forceinline__ WB window_bounds(int w) const {
    WB b;
    const int64_t wEndOff = (int64_t)w * q.qstep - Ae;     // wEnd - ts0
    b.e = fdb_bound_e(tso, n, lin, wEndOff, &b.t2);
    b.s = fdb_bound_s(tso, n, lin, wEndOff - q.qwindow, &b.t1);
    return b;
  }
  __device__ __forceinline__ int end_search(int w, int32_t* t2, int* s_at_end) const {
    const int64_t x = (int64_t)w * q.qstep - Ae;         // wEnd - ts0
    int32_t t_next, unused;
    const int e = fdb_bound_core(tso, n, lin, x, t2, &t_next, nullptr);
    *s_at_end = fdb_bound_s_from_e(tso, n, lin, x, e, *t2, t_next, &unused);
    return e;
  }
  // every lane of the wave calls this (the exchange needs its senders)
  __device__ __forceinline__ WB shared_bounds(int w) {
    WB b;
    int s_cur;
    b.e = end_search(w, &b.t2, &s_cur);
    b.s = __builtin_amdgcn_ds_bpermute(share_src, lane < 64 - wshare ? s_cur : s_prev);
    s_prev = s_cur;
    b.t1 = tso[b.s];     // 0 <= s <= n; tso[n] is readable, never used
    return b;
  }
  // the direct rows of an aligned series: i32 throughout (fdb_aligned_test
  // checked the launch's offsets), no state, no other lane involved
  __device__ __forceinline__ WB aligned_bounds(int w) const {
    WB b;
    const int32_t x = (int32_t)((uint32_t)al.x0 + (uint32_t)w * (uint32_t)q.qstep);
    const int32_t y = (int32_t)((uint32_t)x - (uint32_t)q.qwindow);
    fdb_aligned_bounds(tso, n, al.k0, w, wshare, x, y, &b.e, &b.s, &b.t1, &b.t2);
    return b;
  }
  // slot k's bounds in a tile of tn windows; slots run in order k = 0..3 (the
  // shared search hands slot k-1 on to slot k, and slot 3 on to the next
  // tile's slot 0). A window that is not there (!wok) gets the empty range
  // {1, -1}: every arm of fast_window_value rejects it by its own range test
  // and returns NaN, so no caller guards on wok again.
  __device__ __forceinline__ WB calc_bounds(int k, int w, bool wok, int tn) {
    WB b = WB{1, -1, 0, 0};
    if constexpr (SHARE) {
      if (64 * k < tn) {             // wave-uniform: the slot has windows
        WB sb;
        if (ALIGNED && al.ok) sb = aligned_bounds(w);
        else sb = shared_bounds(w);
        if (wok) b = sb;
      }
    } else if (wok) {
      b = window_bounds(w);
    }
    return b;
  }
};

// ---- value: one window's result from its row range ----------------------------
template <int FUNC, typename WS>
__device__ __forceinline__ double fast_window_value(const WS& ws, const WB& wb, int w,
                                                    const FastChunk& ch,
                                                    const ResetScan& rs, int64_t Ae,
                                                    const FastQuery& q,
                                                    const double* inv_tab) {
  constexpr int KIND = FKind<FUNC>::v;
  const int s = wb.s, e = wb.e, n = ch.n;
  double res = NAN;
  if constexpr (KIND == K_RATE) {
    // ChunkedRateFunctionBase + extrapolatedRate; e>s implies s valid,
    // covers empty and single-sample windows (highestTime>lowestTime).
    // The epilogue keeps the oracle's EXACT operation sequence
    // (d_extrapolate_core says why). All inputs are ts0-relative;
    // extrapolatedRate uses differences only, so offset-domain i64s give
    // bit-identical results. (An explicitly staged variant — all 4 windows'
    // loads before any math — measured SLOWER: 2.84 -> 3.26 ms, register
    // pressure.)
    constexpr bool IS_COUNTER = (FUNC == FN_RATE || FUNC == FN_INCREASE);
    if (e > s) {
      const int t1 = wb.t1, t2 = wb.t2;   // tso[s], tso[e] from the probe
      if (t2 > t1) {
        double v1 = ws.val[s], v2 = ws.val[e];
        if (IS_COUNTER && ch.dropped) {
          if (isnan(v1)) v1 = 0;
          if (isnan(v2)) v2 = 0;
          auto row_at = [&](int j) { return ws.val[j]; };
          v1 += d_corr_at(ws.dpos, ws.dcum, rs.count, rs.dense, s, row_at);
          v2 += d_corr_at(ws.dpos, ws.dcum, rs.count, rs.dense, e, row_at);
        }
        const int64_t wEndOff = (int64_t)w * q.qstep - Ae;   // wEnd - ts0
        if (q.qw32)    // uniform: window fits i32 ⇒ so do all three gaps
          res = d_extrapolated_rate_i32<true>(
              (int32_t)(t1 - (wEndOff - q.qwindow)), (int32_t)(wEndOff - t2),
              e - s + 1, t2 - t1, q.dur_ms, v1, v2, IS_COUNTER, FUNC == FN_RATE,
              inv_tab, q.rk_lim);
        else
          res = d_extrapolated_rate(wEndOff - q.qwindow, wEndOff, e - s + 1,
                                    t1, v1, t2, v2, IS_COUNTER, FUNC == FN_RATE);
      }
    }
  } else if constexpr (KIND == K_PFX || KIND == K_PFX_SQ) {
    // prefix differences; AVG/STDDEV/STDVAR through the reciprocal table
    // (the walk divides — deliberately different, ≤2 ulp apart)
    if (e >= s && e >= 0) {
      double ps = ws.val[e] - (s ? ws.val[s - 1] : 0.0);
      int pc = (int)ws.cnt[e] - (s ? (int)ws.cnt[s - 1] : 0);
      if constexpr (FUNC == FN_SUM) res = pc > 0 ? ps : NAN;
      else if constexpr (FUNC == FN_COUNT) res = (double)pc;
      else if constexpr (FUNC == FN_AVG) res = pc > 0 ? ps * inv_tab[pc] : NAN;
      else if constexpr (FUNC == FN_RATE_OVER_DELTA)   // RateFunctions.scala:424-445
        res = (pc > 0 ? ps : NAN) * q.rate_scale;
      else if (pc > 0) {                               // FN_STDDEV / FN_STDVAR
        double qs = ws.sq[e] - (s ? ws.sq[s - 1] : 0.0);
        double inv = inv_tab[pc];
        double avg = ps * inv;
        double r = qs * inv - avg * avg;
        res = (FUNC == FN_STDDEV) ? sqrt(r) : r;
      }
    }
  } else if constexpr (KIND == K_MINMAX) {
    if (e >= s && e >= 0) {
      constexpr bool IS_MIN = (FUNC == FN_MIN);
      int ga = (s + 7) >> 3, gb = (e + 1) >> 3;
      if (ga < gb) {
        for (int i = s; i < ga * 8; i++) d_fold_mm<IS_MIN>(res, ws.val[i]);
        for (int g = ga; g < gb; g++) d_fold_mm<IS_MIN>(res, ws.grp[g]);
        for (int i = gb * 8; i <= e; i++) d_fold_mm<IS_MIN>(res, ws.val[i]);
      } else {
        for (int i = s; i <= e; i++) d_fold_mm<IS_MIN>(res, ws.val[i]);
      }
    }
  } else if constexpr (KIND == K_CHANGES) {
    // single chunk: indicator prefix over (s, e]; prev starts NaN.
    // resets: same shape, an empty window stays NaN
    if (e >= s && e >= 0) res = (double)((int)ws.cnt[e] - (int)ws.cnt[s]);
  } else if constexpr (FUNC == FN_TIMESTAMP) {
    // TimestampChunkedFunction: no window-start bound on the row, but
    // WindowedChunkIterator drops a chunk that ends before wStart
    // (s == n), so such a window has no sample at all; seconds
    if (e >= 0 && s < n) res = (double)(ch.ts0 + wb.t2) / 1000.0;
  } else if constexpr (FUNC == FN_PRESENT) {
    if (e >= s && e >= 0)
      d_present_at(ws.val[e], e, [&](int j) { return ws.val[j]; }, &res);
  } else if constexpr (FUNC == FN_LAST) {
    // ts[e] >= ts[s] >= wStart holds whenever the range is nonempty
    if (e >= s && e >= 0) res = ws.val[e];
  } else if constexpr (FUNC == FN_IRATE || FUNC == FN_IDELTA) {
    // instantValue (RangeInstantFunctions.scala:68-95) on the window's last
    // two raw rows; e > s means at least two rows, e >= 1
    if (e > s) {
      const double last = ws.val[e], prev = ws.val[e - 1];
      if constexpr (FUNC == FN_IDELTA) res = last - prev;
      else res = d_irate_finish(last, prev, (double)(wb.t2 - ws.tso()[e - 1]));
    }
  } else {  // FN_ZSCORE
    if (e >= s && e >= 0) {
      double sm, sq;
      int pc;
      d_range_moments([&](int j) { return ws.val[j]; }, s, e, sm, sq, pc);
      res = d_zscore_finish(sm, sq, pc, ws.val[e]);   // a NaN last row: NaN
    }
  }
  return res;
}

// ---- EMIT=1: per-lane group accumulators (windows lane+64k, k<4; W <= 256) ----
struct FastGroupAcc {
  double accS[4] = {NAN, NAN, NAN, NAN}, accQ[4] = {}, accC[4] = {};
  int cur_grp = -1;
  __device__ __forceinline__ void clear() {
    #pragma unroll
    for (int k = 0; k < 4; k++) { accS[k] = NAN; accQ[k] = 0; accC[k] = 0; }
  }
  // fastReduce register-accumulate (NaN rows skipped, RowAggregator semantics)
  __device__ __forceinline__ void accumulate(int k, int agg_id, double res) {
    if (isnan(res)) return;
    accC[k] += 1.0;
    switch (agg_id) {
      case AGG_MIN: d_fold_mm<true>(accS[k], res); break;
      case AGG_MAX: d_fold_mm<false>(accS[k], res); break;
      case AGG_COUNT: case AGG_GROUP: break;
      case AGG_STDDEV: case AGG_STDVAR: accQ[k] += res * res; [[fallthrough]];
      default:   // the sum: AGG_SUM / AGG_AVG, and the two above
        accS[k] = isnan(accS[k]) ? res : accS[k] + res;
    }
  }
  // one atomic burst into the open group's cells (if any), then start over
  __device__ __forceinline__ void flush(int lane, int num_windows, int agg_id,
                                        double* out, double* out_cnt, double* out_sq) {
    if (cur_grp < 0) return;
    #pragma unroll
    for (int k = 0; k < 4; k++) {
      int w = lane + 64 * k;
      if (w < num_windows && accC[k] > 0) {
        size_t cell = (size_t)cur_grp * num_windows + w;
        if (agg_id == AGG_MIN || agg_id == AGG_MAX)
          atomic_min_max_f64(&out[cell], accS[k], agg_id == AGG_MIN);
        else
          atomicAdd(&out[cell],
                    (agg_id == AGG_COUNT || agg_id == AGG_GROUP) ? accC[k] : accS[k]);
        atomicAdd(&out_cnt[cell], accC[k]);
        if (out_sq) atomicAdd(&out_sq[cell], accQ[k]);
      }
    }
    clear();
  }
};

// MINW = min waves/SIMD the register allocator must meet. PFX_SQ is
// LDS-bound at 4 blocks/CU; the group-emit variant carries 12 accumulator
// registers (4 waves); K_RATE (a 256-entry reciprocal table: 22,784 B of LDS
// per block, which still fits 7 blocks/CU) is
// built at 7 as measured on hardware (profiles/README.md, rounds 3 and 4);
// the gauge kinds are built at 6. Since round 5 the bounds no longer bind:
// with the decoders' lane-scaled blob addresses kept out of the series loop's
// live set (see fast_decode) every plain-grid instantiation sits at 36-53
// VGPRs with no scratch (FN_RATE 53, FN_AVG 44), and occupancy is set by LDS
// alone. SHARE selects the shared window search (window = 1..64 whole steps;
// wshare carries that ratio): a template parameter, not a runtime branch.
template <int FUNC, int EMIT, int MINW, bool TIMED = false, bool SHARE = false,
          bool ALIGNED = false>
__global__ __launch_bounds__(FAST_WAVES * 64, MINW)
void fast_scan_kernel(const uint8_t* __restrict__ blob,
                      const FdbFastDesc* __restrict__ desc,
                      const int32_t* __restrict__ group_ids,
                      const int32_t* __restrict__ sbg,   // EMIT=1: group-sorted order
                      int num_series,
                      int64_t qstart, int64_t qstep, int64_t qwindow,
                      int num_windows, int agg_id,
                      double* __restrict__ out,
                      double* __restrict__ out_cnt,
                      double* __restrict__ out_sq,
                      int wshare)   // SHARE: m = qwindow/qstep, 1..64
{
  constexpr int KIND = FKind<FUNC>::v;
  __shared__ FWs<KIND> ws_all[FAST_WAVES];
  __shared__ double inv_tab[inv_entries<KIND> ? inv_entries<KIND> : 1];

  // readfirstlane pins the wave id (and everything derived from it — series
  // ids, descriptor addresses) as wave-uniform for the compiler: the whole
  // per-series bookkeeping chain then lives in SGPRs with scalar loads
  // instead of occupying VGPRs
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  FWs<KIND>& ws = ws_all[wave];

  if (inv_entries<KIND>) {
    for (int i = threadIdx.x; i < inv_entries<KIND>; i += FAST_WAVES * 64)
      inv_tab[i] = 1.0 / (double)i;          // [0] = +inf (never a divisor)
    __syncthreads();
  }

  const FastQuery q{qstep, qwindow, 1000.0 / (double)qwindow, (double)qwindow,
                    qwindow < ((int64_t)1 << 31),
                    qwindow <= (int64_t)FDB_RATE_RTAB_MAX_MS ? FDB_RATE_RTAB : 0,
                    1.0f / (float)qstep};
  FastTimer<TIMED> timer;

  // series iteration: grid-stride for the plain grid emit; a contiguous slab
  // of the group-sorted index for the fused-group emit (so one wave sees each
  // group as a run and flushes once per group change)
  int pos0, pos1, pos_step;
  if (EMIT == 1) {
    const int gw = blockIdx.x * FAST_WAVES + wave;
    const int nwaves = gridDim.x * FAST_WAVES;
    const int slab = (num_series + nwaves - 1) / nwaves;
    pos0 = gw * slab;
    pos1 = min(num_series, pos0 + slab);
    pos_step = 1;
  } else {
    pos0 = blockIdx.x * FAST_WAVES + wave;
    pos1 = num_series;
    pos_step = gridDim.x * FAST_WAVES;
  }
  FastGroupAcc acc;

  for (int pos = pos0; pos < pos1; pos += pos_step) {
    timer.start();
    const int sid = __builtin_amdgcn_readfirstlane((EMIT == 1) ? sbg[pos] : pos);
    const FDesc cd = fast_load_desc(desc, sid);

    const FastChunk ch = fast_decode(cd, blob, ws, lane);
    d_lds_fence();
    timer.lap(PH_DECODE);

    const ResetScan rs = fast_meta<KIND, FUNC>(ws, ch.n, ch.dropped, lane);
    d_lds_fence();
    timer.lap(PH_META);

    if (EMIT == 1 && group_ids[sid] != acc.cur_grp) {     // group change
      acc.flush(lane, num_windows, agg_id, out, out_cnt, out_sq);
      acc.cur_grp = group_ids[sid];
    }

    FastBounds<SHARE, ALIGNED> bnd(ws.tso(), ch.n, ch.ts0 - qstart, q, wshare, lane,
                                   cd, num_windows);
    for (int tb = 0; tb < num_windows; tb += FAST_TILE) {
      const int tn = min(FAST_TILE, num_windows - tb);
      // the timed variant computes all four windows' bounds ahead of the
      // window phase so the split can charge them to PH_BOUNDS; the sinks
      // keep them, and each window's result, alive although its result
      // stores are suppressed
      WB tbnd[TIMED ? 4 : 1];
      if constexpr (TIMED) {
        #pragma unroll
        for (int k = 0; k < 4; k++) {
          const int wi = lane + 64 * k;
          tbnd[k] = bnd.calc_bounds(k, tb + wi, wi < tn, tn);
          asm volatile("" :: "v"(tbnd[k].s ^ tbnd[k].e ^ tbnd[k].t1 ^ tbnd[k].t2));
        }
        timer.lap(PH_BOUNDS);
      }

      // window phase: 4 windows per lane; plain grid store, or the group
      // accumulators
      #pragma unroll
      for (int k = 0; k < 4; k++) {
        const int wi = lane + 64 * k;
        const int w = tb + wi;
        const bool wok = wi < tn;
        WB wb;
        if constexpr (TIMED) wb = tbnd[k];
        else wb = bnd.calc_bounds(k, w, wok, tn);
        const double res = fast_window_value<FUNC>(ws, wb, w, ch, rs, bnd.Ae, q, inv_tab);
        if constexpr (TIMED) asm volatile("" :: "v"(res));
        if (EMIT == 1) acc.accumulate(k, agg_id, res);
        else if (wok && !TIMED) out[(size_t)sid * num_windows + w] = res;
      }
      d_lds_fence();
      timer.lap(PH_WINDOWS);
    }  // tiles
  }  // series
  if (EMIT == 1) acc.flush(lane, num_windows, agg_id, out, out_cnt, out_sq);
  if (EMIT == 0) timer.store(out, (size_t)blockIdx.x * FAST_WAVES + wave, lane);
}

// ---------------------------------------------------------------------------
// host-side launcher (called from engine.hip's launch dispatch)
// ---------------------------------------------------------------------------
struct FastLaunch {   // grid, stream, the kernel's arguments, the build selectors
  int grid; hipStream_t stream;
  const DatasetView& v; const FdbFastDesc* desc; const WindowGrid& w; int agg_id;
  double *out, *out_cnt, *out_sq;
  int wshare;         // 0: two searches per window
  bool aligned;       // shared search only: the build that holds the direct rows
  bool emit_group, timed;
};

// Launches FUNC F's build: the group emit at 4 waves/SIMD or the plain grid at
// MINW, the shared search when wshare is set. The timed build (phase_mask bit
// 3) exists for FN_RATE and FN_AVG, the shipped builds of the two bench
// shapes; elsewhere the bit changes nothing.
template <int F, int EMIT, int MINW, bool TIMED>
static void launch_fast_as(const FastLaunch& a) {
  const auto kernel =
      !a.wshare ? fast_scan_kernel<F, EMIT, MINW, TIMED, false, false>
      : a.aligned ? fast_scan_kernel<F, EMIT, MINW, TIMED, true, true>
                  : fast_scan_kernel<F, EMIT, MINW, TIMED, true, false>;
  hipLaunchKernelGGL(kernel, dim3(a.grid), dim3(FAST_WAVES * 64), 0, a.stream,
                     a.v.blob, a.desc, a.v.group_ids, a.v.sbg, a.v.num_series,
                     a.w.start, a.w.step, a.w.window, a.w.n, a.agg_id, a.out,
                     a.out_cnt, a.out_sq, a.wshare);
}
template <int F, int MINW>
static void launch_fast(const FastLaunch& a) {
  if (a.emit_group) return launch_fast_as<F, 1, 4, false>(a);
  if constexpr (F == FN_RATE || F == FN_AVG)
    if (a.timed) return launch_fast_as<F, 0, MINW, true>(a);
  launch_fast_as<F, 0, MINW, false>(a);
}

// test hook: how many descriptors of the sample passed the aligned-rows test
// at the last launch if that launch took the ALIGNED build, else 0
static int32_t g_last_aligned = 0;
extern "C" int32_t fdb_debug_last_fast_aligned(void) { return g_last_aligned; }

int32_t fdb_launch_fast_scan(hipStream_t stream, const DatasetView& v,
                             const FdbFastDesc* desc,
                             const FdbFastDesc* sample, int nsample,
                             const WindowGrid& w, int func_id, int agg_id,
                             int emit_group, double* out, double* out_cnt,
                             double* out_sq, int phase_mask) {
  const int64_t qstart = w.start, qstep = w.step, qwindow = w.window;
  const int num_windows = w.n;
  int grid = (v.num_series + FAST_WAVES - 1) / FAST_WAVES;
  // measured best of {1536, 3072, 8192, 16384}; FDB_GRID: perf experiments
  const int cap = fdb_env_int("FDB_GRID", 16384);
  if (cap > 0 && grid > cap) grid = cap;
  // windows share end searches when the window is m = 1..64 whole steps
  // (FDB_WINDOW_SHARE=0: the two-searches-per-window path, for A/B runs)
  int wshare = 0;
  if (qstep > 0 && qwindow % qstep == 0 && qwindow / qstep >= 1 &&
      qwindow / qstep <= 64)
    wshare = (int)(qwindow / qstep);
  if (fdb_env_int("FDB_WINDOW_SHARE", 1) == 0) wshare = 0;
  // The build that also holds the direct rows (ALIGNED) costs a series that
  // does not qualify about 2 % (registers, SGPR spills: profiles/README.md,
  // round 7) and saves one that does about 9 %, so it is launched only where
  // at least a quarter of the dataset qualifies under THIS query: the
  // kernel's own test, run here on the host-side descriptor sample kept at
  // upload. Any other launch keeps the search-only build.
  // (FDB_ALIGNED=0: always the search-only build, for A/B runs)
  int sampled = 0, eligible = 0;
  if (wshare) {
    const float inv_q = 1.0f / (float)qstep;
    for (int i = 0; i < nsample; i++) {
      const FdbFastDesc& d = sample[i];
      if (d.n == 0) continue;
      sampled++;
      const int64_t A = d.ts0 - qstart;
      const int32_t k0 = fdb_aligned_guess(d.ts_base, d.ts_rmin, d.ts_rmax, A, inv_q);
      if (fdb_aligned_test(d.n, d.ts_base, d.ts_slope, d.ts_rmin, d.ts_rmax, A, qstep,
                           wshare, num_windows, k0).ok)
        eligible++;
    }
  }
  bool aligned = eligible > 0 && 4 * eligible >= sampled;
  if (fdb_env_int("FDB_ALIGNED", 1) == 0) aligned = false;
  g_last_aligned = aligned ? eligible : 0;
  const FastLaunch a{grid, stream, v, desc, w, agg_id,
                     out, out_cnt, out_sq, wshare, aligned, emit_group != 0,
                     (phase_mask & 8) != 0};   // bit 3: s_memtime phase ablation
  switch (func_id) {     // <function, plain-grid MINW>
    case FN_RATE:            launch_fast<FN_RATE, 7>(a); break;   // LDS: 7 blocks/CU
    case FN_INCREASE:        launch_fast<FN_INCREASE, 6>(a); break;
    case FN_DELTA:           launch_fast<FN_DELTA, 6>(a); break;
    case FN_SUM:             launch_fast<FN_SUM, 6>(a); break;
    case FN_COUNT:           launch_fast<FN_COUNT, 6>(a); break;
    case FN_AVG:             launch_fast<FN_AVG, 6>(a); break;
    case FN_RATE_OVER_DELTA: launch_fast<FN_RATE_OVER_DELTA, 6>(a); break;
    case FN_MIN:             launch_fast<FN_MIN, 6>(a); break;
    case FN_MAX:             launch_fast<FN_MAX, 6>(a); break;
    case FN_STDDEV:          launch_fast<FN_STDDEV, 3>(a); break;
    case FN_STDVAR:          launch_fast<FN_STDVAR, 3>(a); break;
    case FN_CHANGES:         launch_fast<FN_CHANGES, 6>(a); break;
    case FN_LAST:            launch_fast<FN_LAST, 6>(a); break;
    case FN_PRESENT:         launch_fast<FN_PRESENT, 6>(a); break;
    case FN_TIMESTAMP:       launch_fast<FN_TIMESTAMP, 6>(a); break;
    case FN_ZSCORE:          launch_fast<FN_ZSCORE, 6>(a); break;
    case FN_IRATE:           launch_fast<FN_IRATE, 6>(a); break;
    case FN_IDELTA:          launch_fast<FN_IDELTA, 6>(a); break;
    case FN_RESETS:          launch_fast<FN_RESETS, 6>(a); break;
    default:
      fdb_set_error("fast scan: unsupported func_id %d", func_id);
      return FDB_ERR_BADARG;
  }
  return fdb_launched("fast_scan_kernel");
}
