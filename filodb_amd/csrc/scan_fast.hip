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
//    slope, value init and slope, val_exact32. The kernel loads desc[sid]
//    through a wave-uniform address and goes straight to the payload: two
//    dependent memory trips per series instead of the four of
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
//  * timestamps live in LDS as i32 offsets from the chunk's first ts (halves
//    the LDS footprint and read traffic; chunk span is checked at upload)
//  * the extrapolatedRate epilogue keeps the oracle's exact operation
//    sequence (its threshold comparisons are discontinuous — see the window
//    phase); AVG/STDDEV use a per-block reciprocal table (continuous, ≤2 ulp)
//  * window results are branch-lean selects; one store per window
//
// Per-window semantics are IDENTICAL to the round-1 kernel's single-chunk
// stage C (parity-green against the oracle): RateFunctions.scala:72-111,
// 230-289; AggrOverTimeFunctions.scala:553-605,924-1028,1082-1224;
// RangeFunction.scala:595-745.
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
  int32_t tso[FDB_DEFAULT_MAX_ROWS + 4];   // ts - ts0 (i32 offsets); the pad keeps
                                           // tso[startRow] readable at startRow == n
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
};
static_assert(offsetof(FdbFastDesc, n) == 8 && offsetof(FdbFastDesc, ts_flags) == 12 &&
              offsetof(FdbFastDesc, ts0) == 16 && offsetof(FdbFastDesc, ts_base) == 24 &&
              offsetof(FdbFastDesc, val_init) == 32 && offsetof(FdbFastDesc, val_slope) == 40,
              "FDesc's dword views follow FdbFastDesc's layout");

template <int KIND> struct NeedsInv {   // reciprocal table users (AVG/STDDEV;
  // the rate epilogue keeps the oracle's exact divisions — its threshold
  // comparisons are discontinuous and must round identically, see below)
  static constexpr bool v = KIND == K_PFX || KIND == K_PFX_SQ;
};

// in-chunk correction at row i from the sparse drop table (the step function
// CorrectingDoubleVectorReader :325-342 materializes as corrected[])
template <typename WS>
__device__ __forceinline__ double f_corr_at(const WS& ws, int dcount, bool dense,
                                            int n, int i) {
  if (dense) {      // >FAST_DROPS resets in the chunk: serial recompute (rare)
    double corr = 0, last = -1.7976931348623157e308;
    for (int j = 0; j <= i; j++) {
      double x = ws.val[j];
      if (isnan(x)) x = 0;
      if (x < last) corr += last;
      last = x;
    }
    return corr;
  }
  double c = 0;
  for (int j = 0; j < dcount; j++) {
    if (ws.dpos[j] <= i) c = ws.dcum[j]; else break;
  }
  return c;
}

// MINW = min waves/SIMD the register allocator must meet. PFX_SQ is
// LDS-bound at 4 blocks/CU; the group-emit variant carries 12 accumulator
// registers (4 waves); K_RATE (no reciprocal table, LDS fits 7 blocks/CU) is
// built at 5, 6 and 7 — the launcher picks via FDB_RATE_WAVES, default 7 as
// measured on hardware (profiles/README.md, rounds 3 and 4); the gauge kinds
// are built at 6. Since round 5 the bounds no longer bind: with the decoders'
// lane-scaled blob addresses kept out of the series loop's live set (see the
// decode section) every plain-grid instantiation sits at 36-53 VGPRs with no
// scratch (FN_RATE 53, FN_AVG 44), and occupancy is set by LDS alone.
// SHARE selects the shared window search (window = 1..64 whole steps; wshare
// carries that ratio): a template parameter, not a runtime branch.
template <int FUNC, int EMIT, int MINW, bool TIMED = false, bool SHARE = false>
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
                      int pm,    // bit 3: s_memtime phase split into out[]
                      int wshare)   // SHARE: m = qwindow/qstep, 1..64
{
  constexpr int KIND = FKind<FUNC>::v;
  constexpr bool IS_COUNTER = (FUNC == FN_RATE || FUNC == FN_INCREASE);
  __shared__ FWs<KIND> ws_all[FAST_WAVES];
  __shared__ double inv_tab[NeedsInv<KIND>::v ? FDB_DEFAULT_MAX_ROWS + 2 : 1];

  // readfirstlane pins the wave id (and everything derived from it — series
  // ids, directory offsets, header pointers) as wave-uniform for the
  // compiler: the whole per-series bookkeeping chain then lives in SGPRs
  // with scalar loads instead of occupying VGPRs
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  FWs<KIND>& ws = ws_all[wave];

  if (NeedsInv<KIND>::v) {
    for (int i = threadIdx.x; i < FDB_DEFAULT_MAX_ROWS + 2; i += FAST_WAVES * 64)
      inv_tab[i] = 1.0 / (double)i;          // [0] = +inf (never a divisor)
    __syncthreads();
  }

  const double rate_scale = 1000.0 / (double)qwindow;
  const bool qw32 = qwindow < ((int64_t)1 << 31);   // i32 epilogue eligibility
  const double dur_ms = (double)qwindow;
  (void)pm;
  constexpr bool timing = TIMED;        // perf ablation (clobbers out[])
  uint64_t tD = 0, tM = 0, tI = 0, tW = 0, tt = 0;

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

  // EMIT=1 per-lane group accumulators (windows lane+64k, k<4; W <= 256)
  double accS[4], accQ[4], accC[4];
  int cur_grp = -1;
  if (EMIT == 1) {
    #pragma unroll
    for (int k = 0; k < 4; k++) { accS[k] = NAN; accQ[k] = 0; accC[k] = 0; }
  }
  auto flush_group = [&](int g) {
    #pragma unroll
    for (int k = 0; k < 4; k++) {
      int w = lane + 64 * k;
      if (w < num_windows && accC[k] > 0) {
        size_t cell = (size_t)g * num_windows + w;
        if (agg_id == AGG_MIN || agg_id == AGG_MAX)
          atomic_min_max_f64(&out[cell], accS[k], agg_id == AGG_MIN);
        else
          atomicAdd(&out[cell],
                    (agg_id == AGG_COUNT || agg_id == AGG_GROUP) ? accC[k] : accS[k]);
        atomicAdd(&out_cnt[cell], accC[k]);
        if (out_sq) atomicAdd(&out_sq[cell], accQ[k]);
      }
      accS[k] = NAN; accQ[k] = 0; accC[k] = 0;
    }
  };

  // series bookkeeping: one 64-B descriptor per series (fast_desc.h), parsed
  // from the vector headers once at upload, fetched here with one scalar load
  // through a wave-uniform address — the payload is the only dependent trip
  // behind it. (Requesting desc[next sid] a series early, held in SGPRs, in
  // VGPRs, or only touched into cache, measured 0.01-0.02 ms SLOWER on
  // rate_1m than this plain load: at 7 waves/SIMD the second trip is hidden
  // already. profiles/README.md, round 5.)
  auto load_desc = [&](int s) {
    const uint4* p = reinterpret_cast<const uint4*>(desc + s);
    const uint4 a = p[0], b = p[1], c = p[2];
    return FDesc{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w}};
  };
  for (int pos = pos0; pos < pos1; pos += pos_step) {
    if (timing) tt = __builtin_amdgcn_s_memtime();
    const int sid = __builtin_amdgcn_readfirstlane((EMIT == 1) ? sbg[pos] : pos);
    const FDesc cd = load_desc(sid);

    // ---- decode: the single chunk into LDS (i32 ts offsets + f64 values) ---
    // n == 0 is an empty series: no chunk, or a guard that upload decided
    // (rows above the chunk cap, or more rows than the timestamp vector has).
    // The packed 8/16-bit arms write whole 4-row groups (scan_common.h), so
    // rows n..4*ceil(n/4)-1 of tso[] and val[] hold garbage. Nothing
    // interprets them: the meta loops guard i < n, the bound search accepts
    // rows < n only (window_bounds.h reads past n but never interprets it),
    // every window row range keeps s <= e < n, and the one tso[s] read at
    // s == n (shared_bounds) is readable and never used.
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
      d_decode_ts_offsets(tv, n, ts0, ws.tso, dl);
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
    d_wait_lds();
    __builtin_amdgcn_wave_barrier();
    if (timing) { uint64_t t = __builtin_amdgcn_s_memtime(); tD += t - tt; tt = t; }

    // ---- meta: kind-specific per-row structures ----------------------------
    int dcount = 0;
    bool dense = false;
    if constexpr (KIND == K_RATE) {
      // counter-reset scan → sparse (position, cumulative correction) table
      // (CorrectingDoubleVectorReader :325-342; NaN→0 like the reference)
      if (dropped && n > 0) {
        double carry_corr = 0;
        double carry_x = -1.7976931348623157e308;
        for (int base = 0; base < n; base += 64) {
          int i = base + lane;
          double raw = (i < n) ? ws.val[i] : 0;
          double x = (i < n && !isnan(raw)) ? raw : 0;
          double px = __shfl_up(x, 1);
          if (lane == 0) px = carry_x;
          double ci = (i < n && x < px) ? px : 0;
          double scan = wave_incl_scan(ci, lane);
          uint64_t mask = __ballot(ci != 0);
          int here = __popcll(mask);
          if (here) {
            if (dcount + here > FAST_DROPS) {
              dense = true;
            } else if (ci != 0) {
              int slot = dcount + __popcll(mask & ((1ULL << lane) - 1));
              ws.dpos[slot] = (int16_t)i;
              ws.dcum[slot] = carry_corr + scan;
            }
            if (!dense) dcount += here;
          }
          carry_corr += __shfl(scan, 63);
          carry_x = __shfl(x, 63);
        }
        if (dense) dcount = 0;
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
    if constexpr (KIND == K_MINMAX) {
      constexpr bool IS_MIN = (FUNC == FN_MIN);
      for (int base = 0; base < n; base += 64) {
        int i = base + lane;
        double x = (i < n) ? ws.val[i] : NAN;
        #pragma unroll
        for (int off = 1; off < 8; off <<= 1) {
          double o = __shfl_xor(x, off);
          if (!isnan(o) && (isnan(x) || (IS_MIN ? o < x : o > x))) x = o;
        }
        if ((lane & 7) == 0 && i < n) ws.grp[i >> 3] = x;
      }
    }
    if constexpr (KIND == K_CHANGES) {
      // adjacent-pair indicator prefix: x != px (changes) or x < px (resets,
      // ResetsFunction RangeInstantFunctions.scala:352-375); a NaN on either
      // side never counts
      constexpr bool IS_RESETS = (FUNC == FN_RESETS);
      int ccarry = 0;
      double carry_x = NAN;
      for (int base = 0; base < n; base += 64) {
        int i = base + lane;
        double x = (i < n) ? ws.val[i] : NAN;
        double px = __shfl_up(x, 1);
        if (lane == 0) px = carry_x;
        int ind = (i > 0 && i < n && !isnan(x) && !isnan(px) &&
                   (IS_RESETS ? x < px : x != px)) ? 1 : 0;
        int s = wave_incl_scan_i(ind, lane);
        if (i < n) ws.cnt[i] = (uint16_t)(ccarry + s);
        ccarry += __shfl(s, 63);
        carry_x = __shfl(x, 63);
      }
    }
    d_wait_lds();
    __builtin_amdgcn_wave_barrier();
    if (timing) { uint64_t t = __builtin_amdgcn_s_memtime(); tM += t - tt; tt = t; }

    // window time base: wEnd(w) = qstart + w*qstep; offsets are vs ts0
    const int64_t Ae = ts0 - qstart;            // wEnd >= ts  ⟺ w*qstep >= o+Ae
    if (EMIT == 1) {
      const int grp_id = group_ids[sid];
      if (grp_id != cur_grp) {
        if (cur_grp >= 0) flush_group(cur_grp);
        cur_grp = grp_id;
      }
    }

    // per-series constants of the bound search (window_bounds.h): the last
    // timestamp and the rows-per-ms slope, pinned wave-uniform
    FdbLin lin;
    {
      const int32_t tlast = n > 0 ? ws.tso[n - 1] : 0;
      lin.last = __builtin_amdgcn_readfirstlane(tlast);
      lin.inv_h = (n >= 2 && lin.last > 0)
                      ? (float)(n - 1) / (float)lin.last : 0.0f;
    }
    // window w's row range [s, e]: e = last row with ts <= wEnd, s = first
    // row with ts >= wStart (sentinels e = -1 / s = n when there is none);
    // t1/t2 are tso[s]/tso[e] as the probe loaded them (valid iff in range)
    struct WB { int s, e; int32_t t1, t2; };
    auto window_bounds = [&](int w) {
      WB b;
      const int64_t wEndOff = (int64_t)w * qstep - Ae;     // wEnd - ts0
      b.e = fdb_bound_e(ws.tso, n, lin, wEndOff, &b.t2);
      b.s = fdb_bound_s(ws.tso, n, lin, wEndOff - qwindow, &b.t1);
      return b;
    };
    // shared search (wshare = m, window = m steps): window w starts at the
    // offset where window w-m ends, so each lane searches only its windows'
    // ENDS, derives the start row AT that same offset from what the probe
    // already holds (fdb_bound_s_from_e) and hands it to the lane that owns
    // window w+m. Windows sit at lane + 64k, so w-m is lane (lane-m)&63 of
    // this slot when lane >= m and of the previous slot otherwise: the sender
    // picks by lane < 64-m, one ds_bpermute delivers, and only the previous
    // slot's start row stays live. Five searches per lane instead of eight:
    // four ends plus the seed for the windows before the first tile.
    auto end_search = [&](int w, int32_t* t2, int* s_at_end) {
      const int64_t x = (int64_t)w * qstep - Ae;           // wEnd - ts0
      int32_t t_next, unused;
      const int e = fdb_bound_core(ws.tso, n, lin, x, t2, &t_next, nullptr);
      *s_at_end = fdb_bound_s_from_e(ws.tso, n, lin, x, e, *t2, t_next, &unused);
      return e;
    };
    const int share_src = ((lane - wshare) & 63) << 2;     // bpermute address
    int s_prev = 0;         // start row at the end of this lane's window in
                            // the previous slot; slot -1 = windows -64..-1
    if constexpr (SHARE) {
      int32_t unused;
      end_search(lane - 64, &unused, &s_prev);
    }
    // every lane of the wave calls this (the exchange needs its senders)
    auto shared_bounds = [&](int w) {
      WB b;
      int s_cur;
      b.e = end_search(w, &b.t2, &s_cur);
      b.s = __builtin_amdgcn_ds_bpermute(share_src,
                                         lane < 64 - wshare ? s_cur : s_prev);
      s_prev = s_cur;
      b.t1 = ws.tso[b.s];     // 0 <= s <= n; tso[n] is readable, never used
      return b;
    };

    for (int tb = 0; tb < num_windows; tb += FAST_TILE) {
      const int tn = min(FAST_TILE, num_windows - tb);
      // slot k's bounds; slots run in order k = 0..3 (the shared search hands
      // slot k-1 on to slot k, and slot 3 on to the next tile's slot 0)
      auto calc_bounds = [&](int k, int w, bool wok) {
        WB b = WB{1, -1, 0, 0};
        if constexpr (SHARE) {
          if (64 * k < tn) {             // wave-uniform: the slot has windows
            const WB sb = shared_bounds(w);
            if (wok) b = sb;
          }
        } else if (wok) {
          b = window_bounds(w);
        }
        return b;
      };
      // the timed variant computes all four windows' bounds ahead of the
      // window phase so the split can charge them to tI; the sink keeps them
      // alive although its result stores are suppressed
      WB tbnd[timing ? 4 : 1];
      if constexpr (timing) {
        #pragma unroll
        for (int k = 0; k < 4; k++) {
          const int wi = lane + 64 * k;
          tbnd[k] = calc_bounds(k, tb + wi, wi < tn);
          asm volatile("" :: "v"(tbnd[k].s ^ tbnd[k].e ^ tbnd[k].t1 ^ tbnd[k].t2));
        }
        uint64_t t = __builtin_amdgcn_s_memtime(); tI += t - tt; tt = t;
      }
      auto bounds_of = [&](int k, int w, bool wok) {
        if constexpr (timing) { (void)w; (void)wok; return tbnd[k]; }
        else return calc_bounds(k, w, wok);
      };

      // ---- window phase: 4 windows per lane --------------------------------
      // results land through emit_res: plain grid store or fastReduce
      // register-accumulate (NaN rows skipped, RowAggregator semantics)
      auto emit_res = [&](int k, int w, bool wok, double res) {
        if (EMIT == 0) {
          // timing mode suppresses result stores so the per-wave cycle
          // records at out[0..nwaves*4) survive (perf ablation only)
          if (wok && w < num_windows && !timing)
            out[(size_t)sid * num_windows + w] = res;
        } else if (!isnan(res)) {
          switch (agg_id) {
            case AGG_MIN:
              accS[k] = (isnan(accS[k]) || res < accS[k]) ? res : accS[k];
              accC[k] += 1.0; break;
            case AGG_MAX:
              accS[k] = (isnan(accS[k]) || res > accS[k]) ? res : accS[k];
              accC[k] += 1.0; break;
            case AGG_STDDEV: case AGG_STDVAR:
              accQ[k] += res * res;
              accS[k] = isnan(accS[k]) ? res : accS[k] + res;
              accC[k] += 1.0; break;
            case AGG_COUNT: case AGG_GROUP:
              accC[k] += 1.0; break;
            default:   // AGG_SUM / AGG_AVG
              accS[k] = isnan(accS[k]) ? res : accS[k] + res;
              accC[k] += 1.0; break;
          }
        }
      };

      if constexpr (KIND == K_RATE) {
        // ChunkedRateFunctionBase + extrapolatedRate; e>s implies s valid,
        // covers empty and single-sample windows (highestTime>lowestTime).
        // The epilogue keeps the oracle's EXACT operation sequence
        // (RateFunctions.scala:72-111): its durationToZero/threshold
        // comparisons are discontinuous — counters make exact rational ties
        // like v1/delta == 1.1/(numSamples-1) common, and the branch taken
        // then depends on the reference's own FP rounding. All inputs are
        // ts0-relative; extrapolatedRate uses differences only, so
        // offset-domain i64s give bit-identical results.
        // (an explicitly staged variant — all 4 windows' loads before any
        // math — measured SLOWER: 2.84 -> 3.26 ms, register pressure)
        #pragma unroll
        for (int k = 0; k < 4; k++) {
          const int wi = lane + 64 * k;
          const int w = tb + wi;
          const bool wok = wi < tn;
          const WB wb = bounds_of(k, w, wok);
          const int s = wb.s, e = wb.e;
          double res = NAN;
          if (e > s) {
            const int t1 = wb.t1, t2 = wb.t2;   // tso[s], tso[e] from the probe
            if (t2 > t1) {
              double v1 = ws.val[s], v2 = ws.val[e];
              if (IS_COUNTER && dropped) {
                if (isnan(v1)) v1 = 0;
                if (isnan(v2)) v2 = 0;
                v1 += f_corr_at(ws, dcount, dense, n, s);
                v2 += f_corr_at(ws, dcount, dense, n, e);
              }
              const int64_t wEndOff = (int64_t)w * qstep - Ae;   // wEnd - ts0
              if (qw32)      // uniform: window fits i32 ⇒ so do all three gaps
                res = d_extrapolated_rate_i32(
                    (int32_t)(t1 - (wEndOff - qwindow)), (int32_t)(wEndOff - t2),
                    e - s + 1, t2 - t1, dur_ms, v1, v2,
                    IS_COUNTER, FUNC == FN_RATE);
              else
                res = d_extrapolated_rate(wEndOff - qwindow, wEndOff, e - s + 1,
                                          t1, v1, t2, v2,
                                          IS_COUNTER, FUNC == FN_RATE);
            }
          }
          emit_res(k, w, wok, res);
        }
      } else if constexpr (KIND == K_PFX) {
        #pragma unroll
        for (int k = 0; k < 4; k++) {
          const int wi = lane + 64 * k;
          const bool wok = wi < tn;
          const WB wb = bounds_of(k, tb + wi, wok);
          const int s = wb.s, e = wb.e;
          double res = NAN;
          if (e >= s && e >= 0) {
            double ps = ws.val[e] - (s ? ws.val[s - 1] : 0.0);
            int pc = (int)ws.cnt[e] - (s ? (int)ws.cnt[s - 1] : 0);
            if constexpr (FUNC == FN_SUM) res = pc > 0 ? ps : NAN;
            else if constexpr (FUNC == FN_COUNT) res = (double)pc;
            else if constexpr (FUNC == FN_AVG)
              res = pc > 0 ? ps * inv_tab[pc] : NAN;
            else   // FN_RATE_OVER_DELTA (RateFunctions.scala:424-445)
              res = (pc > 0 ? ps : NAN) * rate_scale;
          }
          emit_res(k, tb + wi, wok, res);
        }
      } else {
      #pragma unroll
      for (int k = 0; k < 4; k++) {
        const int wi = lane + 64 * k;
        const int w = tb + wi;
        const bool wok = wi < tn;
        const WB wb = bounds_of(k, w, wok);
        const int s = wb.s, e = wb.e;
        double res = NAN;

        if constexpr (KIND == K_PFX_SQ) {
          if (wok && e >= s && e >= 0) {
            double ps = ws.val[e] - (s ? ws.val[s - 1] : 0.0);
            int pc = (int)ws.cnt[e] - (s ? (int)ws.cnt[s - 1] : 0);
            if (pc > 0) {
              double qs = ws.sq[e] - (s ? ws.sq[s - 1] : 0.0);
              double inv = inv_tab[pc];
              double avg = ps * inv;
              double r = qs * inv - avg * avg;
              res = (FUNC == FN_STDDEV) ? sqrt(r) : r;
            }
          }
        } else if constexpr (KIND == K_MINMAX) {
          if (wok && e >= s && e >= 0) {
            constexpr bool IS_MIN = (FUNC == FN_MIN);
            double mm = NAN;
            auto acc = [&](double x) {
              if (!isnan(x) && (isnan(mm) || (IS_MIN ? x < mm : x > mm))) mm = x;
            };
            int ga = (s + 7) >> 3, gb = (e + 1) >> 3;
            if (ga < gb) {
              for (int i = s; i < ga * 8; i++) acc(ws.val[i]);
              for (int g = ga; g < gb; g++) acc(ws.grp[g]);
              for (int i = gb * 8; i <= e; i++) acc(ws.val[i]);
            } else {
              for (int i = s; i <= e; i++) acc(ws.val[i]);
            }
            res = mm;
          }
        } else if constexpr (KIND == K_CHANGES) {
          // single chunk: indicator prefix over (s, e]; prev starts NaN.
          // resets: same shape, an empty window stays NaN
          if (wok && e >= s && e >= 0)
            res = (double)((int)ws.cnt[e] - (int)ws.cnt[s]);
        } else {  // K_LAST family
          if constexpr (FUNC == FN_TIMESTAMP) {
            // TimestampChunkedFunction: no window-start bound on the row, but
            // WindowedChunkIterator drops a chunk that ends before wStart
            // (s == n), so such a window has no sample at all; seconds
            if (wok && e >= 0 && s < n) res = (double)(ts0 + wb.t2) / 1000.0;
          } else if constexpr (FUNC == FN_PRESENT) {
            if (wok && e >= s && e >= 0) {
              double v = ws.val[e];
              if (!isnan(v)) res = 1.0;
              else if (e > 0) res = isnan(ws.val[e - 1]) ? NAN : 1.0;
            }
          } else if constexpr (FUNC == FN_LAST) {
            // ts[e] >= ts[s] >= wStart holds whenever the range is nonempty
            if (wok && e >= s && e >= 0) res = ws.val[e];
          } else if constexpr (FUNC == FN_IRATE || FUNC == FN_IDELTA) {
            // instantValue (RangeInstantFunctions.scala:68-95) on the
            // window's last two rows; e > s means at least two rows, e >= 1.
            // irate: IRateFunction reads counter-corrected rows
            // (BufferableCounterCorrectionIterator: NaN -> 0, a drop adds the
            // previous value to a running correction); the correction common
            // to both rows cancels, leaving last on a drop and last - prev
            // otherwise. One divide, then one multiply.
            if (wok && e > s) {
              double last = ws.val[e], prev = ws.val[e - 1];
              if constexpr (FUNC == FN_IDELTA) {
                res = last - prev;
              } else {
                if (isnan(last)) last = 0;
                if (isnan(prev)) prev = 0;
                const double d = (last < prev) ? last : last - prev;
                const double dt = (double)(wb.t2 - ws.tso[e - 1]);
                res = (dt == 0) ? NAN : d / dt * 1000.0;
              }
            }
          } else {  // FN_ZSCORE (AggrOverTimeFunctions.scala:1592-1603)
            if (wok && e >= s && e >= 0) {
              double sm = NAN, sq = NAN, lastv = NAN;
              int pc = 0;
              for (int i = s; i <= e; i++) {
                double x = ws.val[i];
                if (isnan(x)) continue;
                if (isnan(sm)) { sm = 0; sq = 0; }
                if (i == e) lastv = x;
                sm += x; sq += x * x; pc++;
              }
              if (pc > 0) {
                double avg = sm / pc;
                double sd = sqrt(sq / pc - avg * avg);
                res = (lastv - avg) / sd;
              } else res = isnan(sm) ? sm : 0;
            }
          }
        }

        emit_res(k, w, wok, res);
      }
      }  // generic-kind loop
      d_wait_lds();
      __builtin_amdgcn_wave_barrier();
      if (timing) { uint64_t t = __builtin_amdgcn_s_memtime(); tW += t - tt; tt = t; }
    }  // tiles
  }  // series
  if (EMIT == 1 && cur_grp >= 0) flush_group(cur_grp);
  if (timing && EMIT == 0 && lane == 0) {
    size_t gw = (size_t)blockIdx.x * FAST_WAVES + wave;
    out[gw * 4 + 0] = (double)tD;
    out[gw * 4 + 1] = (double)tM;
    out[gw * 4 + 2] = (double)tI;
    out[gw * 4 + 3] = (double)tW;
  }
}

// ---------------------------------------------------------------------------
// host-side launcher (called from engine.hip's launch dispatch)
// ---------------------------------------------------------------------------
int32_t fdb_launch_fast_scan(hipStream_t stream, const uint8_t* blob,
                             const FdbFastDesc* desc,
                             const int32_t* group_ids, const int32_t* series_by_group,
                             int num_series,
                             int64_t qstart, int64_t qstep, int64_t qwindow,
                             int num_windows, int func_id, int agg_id, int emit_group,
                             double* out, double* out_cnt, double* out_sq,
                             int phase_mask) {
  (void)phase_mask;
  int grid = (num_series + FAST_WAVES - 1) / FAST_WAVES;
  int cap = 16384;      // measured best of {1536, 3072, 8192, 16384}
  if (const char* g = getenv("FDB_GRID")) cap = atoi(g);   // perf experiments
  if (cap > 0 && grid > cap) grid = cap;
  const char* rw = getenv("FDB_RATE_WAVES");   // occupancy experiment knob
  const int rate_w = rw ? atoi(rw) : 7;   // 7 measured best (rounds 3 and 4)
  // windows share end searches when the window is m = 1..64 whole steps
  // (FDB_WINDOW_SHARE=0: the two-searches-per-window path, for A/B runs)
  int wshare = 0;
  if (qstep > 0 && qwindow % qstep == 0 && qwindow / qstep >= 1 &&
      qwindow / qstep <= 64)
    wshare = (int)(qwindow / qstep);
  if (const char* s = getenv("FDB_WINDOW_SHARE")) { if (atoi(s) == 0) wshare = 0; }
  // one launch of <F, EMIT, MINW, TIMED>, SHARE picked by wshare
  #define LAUNCH4(F, E, W, T) do { \
    if (wshare) hipLaunchKernelGGL((fast_scan_kernel<F, E, W, T, true>), \
        dim3(grid), dim3(FAST_WAVES * 64), 0, stream, FARGS); \
    else hipLaunchKernelGGL((fast_scan_kernel<F, E, W, T, false>), \
        dim3(grid), dim3(FAST_WAVES * 64), 0, stream, FARGS); } while (0)
  #define FARGS blob, desc, group_ids, \
      series_by_group, num_series, qstart, qstep, qwindow, num_windows, \
      agg_id, out, out_cnt, out_sq, phase_mask, wshare
  #define LAUNCH(F, E, W) LAUNCH4(F, E, W, false)
  #define FCASE(F, W) case F: \
    if (emit_group) LAUNCH(F, 1, 4); else LAUNCH(F, 0, W); break
  const bool timed = (phase_mask & 8) != 0;   // s_memtime phase ablation
  switch (func_id) {
    case FN_RATE:
      if (emit_group) LAUNCH(FN_RATE, 1, 4);
      else if (timed) LAUNCH4(FN_RATE, 0, 7, true);   // the shipped default, timed
      else if (rate_w == 6) LAUNCH(FN_RATE, 0, 6);
      else if (rate_w == 7)   // LDS fits 7 blocks/CU; needs <= 72 VGPRs
        LAUNCH(FN_RATE, 0, 7);
      else LAUNCH(FN_RATE, 0, 5);
      break;
    case FN_AVG:
      if (emit_group) LAUNCH(FN_AVG, 1, 4);
      else if (timed) LAUNCH4(FN_AVG, 0, 6, true);
      else LAUNCH(FN_AVG, 0, 6);
      break;
    FCASE(FN_INCREASE, 6); FCASE(FN_DELTA, 6); FCASE(FN_SUM, 6);
    FCASE(FN_COUNT, 6); FCASE(FN_RATE_OVER_DELTA, 6);
    FCASE(FN_MIN, 6); FCASE(FN_MAX, 6); FCASE(FN_STDDEV, 3); FCASE(FN_STDVAR, 3);
    FCASE(FN_CHANGES, 6); FCASE(FN_LAST, 6); FCASE(FN_PRESENT, 6);
    FCASE(FN_TIMESTAMP, 6); FCASE(FN_ZSCORE, 6);
    FCASE(FN_IRATE, 6); FCASE(FN_IDELTA, 6); FCASE(FN_RESETS, 6);
    default:
      fdb_set_error("fast scan: unsupported func_id %d", func_id);
      return FDB_ERR_BADARG;
  }
  #undef FCASE
  #undef LAUNCH
  #undef LAUNCH4
  #undef FARGS
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fdb_set_error("fast_scan_kernel launch failed: %s", hipGetErrorString(e));
    return FDB_ERR;
  }
  return FDB_OK;
}
