// Histogram scan: two-cursor monotonic walk over sect-delta histogram vectors.
//
// One wave per series, lane l = bucket l (nb <= 64). rate(hist[w]) needs only
// the FIRST element >= wStart and the LAST element <= wEnd of each window
// (HistogramRateFunctionBase, RateFunctions.scala:330-400), and windows come in
// time order, so two cursors only move forward: S tracks the window-start
// element, E the window-end element. Each holds its chunk's timestamps in LDS
// and hops elements by their u16 length prefix. Chunks per series, window/step
// and num_windows are unbounded; rows per chunk <= FDB_DEFAULT_MAX_ROWS (the
// LDS timestamp buffers; upload enforces it).
//
// Stage. A cursor reads its stream (section headers, length prefixes,
// NibblePack groups) from a 256-B register window (nibble_stream.h) and keeps
// the load of the NEXT 256 B in flight: the stream is consumed forward, so the
// usual restage is a register swap whose wait overlapped the last two or three
// elements' work. A cold load happens at a chunk open and when the bytes wanted
// straddle the window's end. An element > 242 B parses from global memory.
//
// Decode. An element's value is the bucket-wise prefix sum of its deltas, plus
// its section's first element unless it is that element (HistogramVector.scala:
// 491-545). A cursor decodes section bases as it passes them, the element it
// stops on once a window needs it (both cursors' together), and the elements
// the corrections read. SumOverTime (SumOverTimeChunkedFunctionH: raw bucket
// sums, no corrections) decodes every element and carries a running prefix.
//
// Corrections (rate). A TypeDrop section (Section.scala:17-24 type byte) adds
// the value of the element before it, apply(e-1). At a chunk seam the previous
// chunk's last value is added when the new chunk's first value is lower in
// Histogram.compare's top-bucket-down order (Histogram.scala:204-214). A window
// counts corrections from the entry of its start element's chunk: the
// reference's per-window CorrectionMeta starts NoCorrection there.
//
// Increase (HistIncreaseFunction, RateFunctions.scala:415-418) is the rate walk
// with the extrapolated delta left unscaled (isRate = false).
//
// Last sample (LastSampleChunkedFunctionH, RangeFunction.scala:630-641): the raw
// buckets of the last element with ts in [wEnd - window, wEnd], no corrections.
// Only the E cursor exists; it decodes section bases and the element a window
// stops on, nothing else. With companion columns the cell's max/min are the
// companion values at that row (LastSampleChunkedFunctionHMax, :643-682), not a
// fold over the window. Divergence: where two chunks meet on an equal
// timestamp the reference keeps the earlier chunk's row (ts > timestamp,
// strictly) and this cursor lands on the later one — the documented
// duplicate-timestamp boundary index choice (README).

#include <cstring>
#include <cmath>

#include "engine_internal.h"
#include "nibble_stream.h"

#define H2_WAVES 4

// wave-wide inclusive prefix sum over i64 (bucket-cumulative reconstruction)
__device__ __forceinline__ int64_t wave_incl_scan_i64(int64_t x, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    int64_t t = __shfl_up(x, off);
    if (lane >= off) x += t;
  }
  return x;
}

// parse one element's per-lane bucket delta from its NibblePack stream.
// ep = element start (at the u16 length); wave-uniform. All lanes must be
// active (estream shuffles). Returns the lane's (<<trailing-zeroes) delta.
// The _buf form takes a pre-staged 256-B register window so two elements'
// stage loads can be issued together and their parse chains interleaved.
template <bool EST>
__device__ __forceinline__ int64_t h2_parse_est(const uint8_t* ep, int nb, int b,
                                                bool live, uint32_t ebuf,
                                                int eshift) {
  // 8-value group headers, walked serially (wave-uniform). EST is a
  // compile-time constant: with it true the walk is pure readlane + scalar
  // arithmetic (SGPR chain, no exec-mask churn); the runtime est ? : form
  // made every access an if-converted dual path whose global-load arm
  // poisoned the uniformity analysis and kept the whole walk on the VALU.
  const int my_group = b >> 3;
  int off = 0, gOff = 0, gBits = 0, gTrail = 0;
  uint32_t gMask = 0;
  for (int g = 0; g * 8 < nb; g++) {
    uint32_t mask = estream_byte_uni(EST, ebuf, eshift, ep, 2 + off);
    const NibbleGroup grp = nibble_group(
        mask, mask ? estream_byte_uni(EST, ebuf, eshift, ep, 2 + off + 1) : 0);
    if (g == my_group) { gOff = off; gBits = grp.numBits; gTrail = grp.trail; gMask = mask; }
    off += grp.glen;
  }
  const int k = b & 7;
  const int bit = nibble_slot_bit(gMask, gBits, k);
  const int koff = 2 + gOff + 2 + (bit >> 3);
  const uint64_t w64 = estream_w64(EST, ebuf, eshift, ep, koff);
  const uint32_t b8 = estream_byte(EST, ebuf, eshift, ep, koff + 8);
  int64_t delta = 0;
  if (live) delta = (int64_t)nibble_slot_value(gMask, gBits, gTrail, k, bit, w64, b8);
  return delta;
}

// uniform-branch dispatcher: big elements (stage window overrun) take the
// unstaged global-load path; everything else stays on the scalarized walk
__device__ __forceinline__ int64_t h2_parse_buf(const uint8_t* ep, int elen,
                                                int nb, int b, bool live,
                                                uint32_t ebuf, int eshift) {
  if (elen + 14 + eshift <= 256)
    return h2_parse_est<true>(ep, nb, b, live, ebuf, eshift);
  return h2_parse_est<false>(ep, nb, b, live, ebuf, eshift);
}

struct H2Cursor {
  const uint8_t* ep;     // current element start (u16 len prefix)
  const uint8_t* sp;     // NEXT section header
  const uint8_t* sb;     // 4-aligned base of the 256-B register stage (null = none)
  uint32_t sbuf;         // this lane's dword of the stage
  uint32_t sbuf2;        // prefetched next 256-B window (load in flight)
  int elen;              // current element's payload length
  int sect_left;         // elements left in section AFTER the current one
  int c;                 // chunk index within the series
  int e_local, e_global; // element indices (current)
  int nrows;             // rows in current chunk
  bool decoded;          // val_b holds the current element
  bool sect_first;       // current element is its section's base
  double base_b;         // per-lane section base value
  double val_b;          // per-lane raw value of current element (if decoded)
  double C_b;            // per-lane correction total at current position
  double Centry_b;       // C at current chunk entry (after boundary drop)
  double prevlast_b;     // raw value of the previous chunk's last element
  double psum_b;         // per-lane running value prefix (HFUNC==1)
};

// value = section base + the deltas' bucket-wise prefix sum (scan); a section
// base element's value is the scan of its own deltas
__device__ __forceinline__ void h2_set_value(H2Cursor& cu, int64_t scan) {
  if (cu.sect_first) { cu.val_b = (double)scan; cu.base_b = cu.val_b; }
  else cu.val_b = cu.base_b + (double)scan;
  cu.decoded = true;
}

// HFUNC H2_RATE = counter-corrected rate (HistRateFunction); H2_SUM =
// SumOverTime of the histograms (raw bucket sums — SumOverTimeChunkedFunctionH,
// no corrections; both cursors then decode every element they pass and carry a
// per-bucket running prefix); H2_INCREASE = the rate walk unscaled; H2_LAST =
// the window's last raw sample, E cursor only. out_max/out_min (nullable) add
// the otel companion-column max/min per window (H2_LAST: at the E row), merged
// across series with maxIgnoreNaN/minIgnoreNaN (HistMaxMinSumAggregator).
template <int MINW, int HFUNC>
__global__ __launch_bounds__(H2_WAVES * 64, MINW)
void hist2_kernel(const uint8_t* __restrict__ blob, DirSoA dir,
                  const uint64_t* __restrict__ max_off,
                  const uint64_t* __restrict__ min_off,
                  const int32_t* __restrict__ series_first,
                  const int32_t* __restrict__ series_nchunks,
                  const int32_t* __restrict__ group_ids,
                  int num_series,
                  int64_t qstart, int64_t qstep, int64_t qwindow,
                  int num_windows, int nb,
                  double* __restrict__ out_sums,   // [G × W × nb]
                  double* __restrict__ out_cnt,    // [G × W]
                  double* __restrict__ out_max,    // [G × W] or null
                  double* __restrict__ out_min,    // [G × W] or null
                  int abl) {   // perf ablation: 1=skip emits, 2=skip decodes
  __shared__ int64_t tsS_all[H2_WAVES][FDB_DEFAULT_MAX_ROWS];
  __shared__ int64_t tsE_all[H2_WAVES][FDB_DEFAULT_MAX_ROWS];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int b = lane;
  const bool live = b < nb;
  constexpr bool IS_RATE = HFUNC == H2_RATE || HFUNC == H2_INCREASE;
  constexpr bool IS_LAST = HFUNC == H2_LAST;
  const bool tmg = (abl & 8) != 0;   // s_memtime phase split into out_cnt[0..3]
  uint64_t tAdv = 0, tDec = 0, tEmit = 0, tc = 0;

  for (int sid = blockIdx.x * H2_WAVES + wave; sid < num_series;
       sid += gridDim.x * H2_WAVES) {
    const int first = series_first[sid];
    const int nchunks = series_nchunks[sid];
    if (nchunks < 1) continue;
    const int grp = group_ids[sid];

    // per-cursor persistent 256-B register stage: one coalesced global load
    // serves the element hops, section headers and parses of the next ~4-8
    // elements (the raw dependent d_u16 hop loads were the serial chain —
    // ~16k cycles per element of wall, sweep ablate data). Returns the byte
    // offset of ptr within the stage, restaging when [ptr, ptr+need) leaves it.
    // dual-buffer linear streaming: sbuf2 always holds an ISSUED load of the
    // NEXT 256-B window (the stream is consumed forward), so the common
    // restage is a register swap whose vmcnt wait overlapped the previous
    // ~2-3 elements of parse work instead of a cold ~600-cycle stall. A cold
    // (re-anchoring) restage only happens at chunk opens and when an element
    // straddles the window boundary. The +512 blob tail pad covers the
    // prefetch past the last vector.
    auto ensure_stage = [&](H2Cursor& cu, const uint8_t* ptr, int need) -> int {
      int off = (int)(ptr - cu.sb);
      if (cu.sb == nullptr || off < 0 || off + need > 256) {
        if (cu.sb != nullptr && off >= 256 && off + need <= 512) {
          cu.sb += 256;                        // swap in the prefetched window
          cu.sbuf = cu.sbuf2;
        } else {
          // cold anchor at ptr (chunk open, straddling element, or jump)
          cu.sb = (const uint8_t*)((uintptr_t)ptr & ~(uintptr_t)3);
          cu.sbuf = estream_stage(cu.sb, lane);
        }
        cu.sbuf2 = estream_stage(cu.sb + 256, lane);   // issue next prefetch
        off = (int)(ptr - cu.sb);
      }
      return off;
    };
    auto staged_byte = [&](H2Cursor& cu, const uint8_t* ptr) -> uint32_t {
      int off = ensure_stage(cu, ptr, 1);
      return estream_byte_uni(true, cu.sbuf, 0, ptr, off);
    };
    auto staged_u16 = [&](H2Cursor& cu, const uint8_t* ptr) -> uint32_t {
      int off = ensure_stage(cu, ptr, 2);
      return estream_byte_uni(true, cu.sbuf, 0, ptr, off) |
             (estream_byte_uni(true, cu.sbuf, 0, ptr, off + 1) << 8);
    };

    // open a chunk for a cursor: decode its timestamps into the cursor's LDS
    // buffer and position at element 0 (section base, decoded)
    auto open_chunk = [&](H2Cursor& cu, int c, int64_t* tsbuf) {
      const uint8_t* hv = blob + dir.val_off[first + c];
      DVec tv;
      d_vec_open_wide(blob + dir.ts_off[first + c], &tv, nullptr);
      cu.nrows = dir.num_rows[first + c];
      if (cu.nrows > FDB_DEFAULT_MAX_ROWS || cu.nrows > tv.n) cu.nrows = 0;
      d_decode_chunk<false>(tv, cu.nrows, tsbuf, nullptr, lane);
      d_wait_lds();
      __builtin_amdgcn_wave_barrier();
      const int defsz = d_u16(hv + FDB_HIST_OFF_DEFSIZE);
      cu.sp = hv + FDB_HIST_OFF_DEF + defsz;
      cu.c = c;
      cu.e_local = -1;
      cu.sect_left = 0;
      cu.decoded = false;
      cu.sb = nullptr;
    };

    // decode the current element (value = section base + scanned deltas;
    // a section base element's value is the scan of its own deltas)
    auto decode_cur = [&](H2Cursor& cu) {
      if (cu.decoded) return;
      if (abl & 2) { cu.decoded = true; cu.val_b = 0; cu.base_b = 0; return; }
      const int off = ensure_stage(cu, cu.ep, min(cu.elen + 14, 256));
      int64_t delta = h2_parse_buf(cu.ep, cu.elen, nb, b, live,
                                   cu.sbuf, off);
      int64_t scan = wave_incl_scan_i64(live ? delta : 0, lane);
      h2_set_value(cu, scan);
      if (HFUNC == H2_SUM) cu.psum_b += cu.val_b;   // value prefix through current
    };

    // step to the next element; returns false when the series is exhausted.
    // tsbuf is the cursor's chunk-timestamp LDS buffer.
    auto step = [&](H2Cursor& cu, int64_t* tsbuf) -> bool {
      if (cu.e_local + 1 >= cu.nrows) {
        if (cu.c + 1 >= nchunks) return false;
        // leaving a chunk: its last element's raw value feeds the boundary
        // drop detection (and TypeDrop at the next chunk's head)
        if (!IS_LAST) {
          decode_cur(cu);
          cu.prevlast_b = cu.val_b;
        }
        open_chunk(cu, cu.c + 1, tsbuf);
      }
      bool new_sect = false;
      if (cu.sect_left == 0) {
        // entering a section; TypeDrop adds apply(e-1) (the element we just
        // ensured is decoded below / at the chunk seam above)
        int stype = (int)staged_byte(cu, cu.sp + 3);
        cu.sect_left = (int)staged_byte(cu, cu.sp + 2);
        int slen = (int)staged_u16(cu, cu.sp);
        cu.ep = cu.sp + 4;
        cu.sp += 4 + slen;
        new_sect = true;
        if (!IS_LAST && stype == 1 && cu.e_local >= 0) cu.C_b += cu.val_b;
      } else {
        cu.ep += 2 + cu.elen;
      }
      cu.elen = (int)staged_u16(cu, cu.ep);
      cu.sect_left--;
      cu.e_local++;
      cu.e_global++;
      cu.sect_first = new_sect;
      cu.decoded = false;
      if (HFUNC == H2_SUM) decode_cur(cu);    // sum mode: full prefix
      else if (new_sect) decode_cur(cu);      // section base always decoded
      else if (!IS_LAST && cu.sect_left == 0 && cu.e_local + 1 < cu.nrows &&
               staged_byte(cu, cu.sp + 3) == 1)
        decode_cur(cu);   // section last feeds the NEXT section's TypeDrop
                          // correction — peek its type byte and decode only
                          // then (drops are rare; the chunk seam decodes its
                          // own last element unconditionally in step())
      if (!IS_LAST && cu.e_local == 0) {
        // first element of a chunk: boundary drop detection
        // (Histogram.compare top-bucket-down, Histogram.scala:204-214)
        if (cu.c > 0) {
          unsigned long long diff = __ballot(live && cu.val_b != cu.prevlast_b);
          if (diff) {
            int L = 63 - __clzll(diff);
            int lt = __shfl((int)(cu.val_b < cu.prevlast_b), L);
            if (lt) cu.C_b += cu.prevlast_b;
          }
        }
        cu.Centry_b = cu.C_b;
      }
      return true;
    };

    // initialize both cursors at element 0
    H2Cursor S, E;
    memset(&S, 0, sizeof(S)); memset(&E, 0, sizeof(E));
    S.e_global = -1; E.e_global = -1;
    S.C_b = 0; E.C_b = 0;
    S.psum_b = 0; E.psum_b = 0;
    if (IS_LAST) {        // E alone: S is never opened or stepped
      open_chunk(E, 0, tsE_all[wave]);
      if (E.nrows == 0) continue;
      if (!step(E, tsE_all[wave])) continue;
    } else {
      open_chunk(S, 0, tsS_all[wave]);
      if (S.nrows == 0) continue;
      if (!step(S, tsS_all[wave])) continue;
      open_chunk(E, 0, tsE_all[wave]);
      step(E, tsE_all[wave]);
    }
    bool s_more = true;

    for (int w = 0; w < num_windows; w++) {
      if (tmg) tc = __builtin_amdgcn_s_memtime();
      const int64_t wEnd = qstart + (int64_t)w * qstep;
      const int64_t wStart = wEnd - qwindow;
      // E → last element with ts <= wEnd
      for (;;) {
        int64_t nxt;
        if (E.e_local + 1 < E.nrows) nxt = tsE_all[wave][E.e_local + 1];
        else if (E.c + 1 < nchunks) nxt = dir.start_time[first + E.c + 1];
        else break;
        if (nxt > wEnd) break;
        if (!step(E, tsE_all[wave])) break;
      }
      if (IS_LAST) {
        // E sits on element 0 with ts > wEnd until the first sample is reached
        const int64_t t2 = tsE_all[wave][E.e_local];
        if (t2 > wEnd || t2 < wStart) continue; // empty window
        decode_cur(E);
        const size_t cell = (size_t)grp * num_windows + w;
        if ((out_max || out_min) && lane == 0 && max_off[first + E.c] != 0) {
          // companion values at the E row only
          DVec xv, nv;
          d_vec_open_wide(blob + max_off[first + E.c], &xv, nullptr);
          d_vec_open_wide(blob + min_off[first + E.c], &nv, nullptr);
          const double emax = d_dv_at(&xv, E.e_local);
          const double emin = d_dv_at(&nv, E.e_local);
          if (out_max && !isnan(emax)) atomic_min_max_f64(&out_max[cell], emax, false);
          if (out_min && !isnan(emin)) atomic_min_max_f64(&out_min[cell], emin, true);
        }
        if (abl & 1) continue;
        if (live) atomicAdd(&out_sums[cell * nb + b], E.val_b);
        if (lane == 0) atomicAdd(&out_cnt[cell], 1.0);
        continue;
      }
      // S → first element with ts >= wStart
      while (s_more && tsS_all[wave][S.e_local] < wStart) {
        if (!step(S, tsS_all[wave])) { s_more = false; break; }
      }
      if (tmg) { uint64_t t2m = __builtin_amdgcn_s_memtime(); tAdv += t2m - tc; tc = t2m; }
      if (!s_more) break;                     // no element >= wStart: done
      const int64_t t1 = tsS_all[wave][S.e_local];
      const int64_t t2 = tsE_all[wave][E.e_local];
      if (t1 > wEnd || t2 < wStart) continue; // empty window
      if (t2 < t1) continue;
      const size_t cell = (size_t)grp * num_windows + w;
      // otel companion columns: NaN-ignoring max/min over the window's rows
      // [S..E], read straight from the raw double vectors chunk by chunk
      if (out_max || out_min) {
        double wmax = NAN, wmin = NAN;
        for (int c2 = S.c; c2 <= E.c; c2++) {
          if (max_off[first + c2] == 0) continue;
          DVec xv, nv;
          d_vec_open_wide(blob + max_off[first + c2], &xv, nullptr);
          d_vec_open_wide(blob + min_off[first + c2], &nv, nullptr);
          const int lo = (c2 == S.c) ? S.e_local : 0;
          const int hi = (c2 == E.c) ? E.e_local : dir.num_rows[first + c2] - 1;
          for (int i = lo + lane; i <= hi; i += 64) {
            d_fold_mm<false>(wmax, d_dv_at(&xv, i));
            d_fold_mm<true>(wmin, d_dv_at(&nv, i));
          }
        }
        for (int off = 32; off > 0; off >>= 1) {
          d_fold_mm<false>(wmax, __shfl_down(wmax, off));
          d_fold_mm<true>(wmin, __shfl_down(wmin, off));
        }
        if (lane == 0) {
          if (out_max && !isnan(wmax)) atomic_min_max_f64(&out_max[cell], wmax, false);
          if (out_min && !isnan(wmin)) atomic_min_max_f64(&out_min[cell], wmin, true);
        }
      }
      if (IS_RATE) {
        if (!(t2 > t1)) continue;             // highestTime > lowestTime rule
        // paired decode: issue both cursors' stage loads together and let the
        // two (independent) header-parse chains interleave — the per-element
        // parse latency was 19 of the 36 ms on config #4 (sweep ablate=3)
        if (!S.decoded && !E.decoded && !(abl & 2)) {
          const int offS = ensure_stage(S, S.ep, min(S.elen + 14, 256));
          const int offE = ensure_stage(E, E.ep, min(E.elen + 14, 256));
          int64_t dS = h2_parse_buf(S.ep, S.elen, nb, b, live, S.sbuf,
                                    offS);
          int64_t dE = h2_parse_buf(E.ep, E.elen, nb, b, live, E.sbuf,
                                    offE);
          int64_t sS = wave_incl_scan_i64(live ? dS : 0, lane);
          int64_t sE = wave_incl_scan_i64(live ? dE : 0, lane);
          h2_set_value(S, sS);
          h2_set_value(E, sE);
        }
        decode_cur(S);
        decode_cur(E);
        if (tmg) { uint64_t t2m = __builtin_amdgcn_s_memtime(); tDec += t2m - tc; tc = t2m; }
        const int numSamples = E.e_global - S.e_global + 1;
        if (abl & 1) continue;
        if (live) {
          // corrections relative to the window's first chunk: the reference's
          // per-window CorrectionMeta starts NoCorrection there
          double v1 = S.val_b + (S.C_b - S.Centry_b);
          double v2 = E.val_b + (E.C_b - S.Centry_b);
          // increase is d_extrapolated_rate(..., isRate = false), spelled as
          // its core: a second caller with another isRate keeps the compiler
          // from folding the constant into the shared wrapper, and the rate
          // instantiations then schedule differently than before
          double r = HFUNC == H2_RATE
              ? d_extrapolated_rate(wStart, wEnd, numSamples,
                                    t1, v1, t2, v2, true, true)
              : d_extrapolate_core(d_div1000((double)(t1 - wStart)),
                                   d_div1000((double)(wEnd - t2)),
                                   d_div1000((double)(t2 - t1)),
                                   numSamples, v1, v2, true);
          atomicAdd(&out_sums[cell * nb + b], r);
        }
        if (lane == 0) atomicAdd(&out_cnt[cell], 1.0);
        if (tmg) { uint64_t t2m = __builtin_amdgcn_s_memtime(); tEmit += t2m - tc; tc = t2m; }
      } else {
        // SumOverTime: prefix difference over [S..E] inclusive
        if (live) {
          double sum_b = E.psum_b - S.psum_b + S.val_b;
          atomicAdd(&out_sums[cell * nb + b], sum_b);
        }
        if (lane == 0) atomicAdd(&out_cnt[cell], 1.0);
      }
    }
    d_wait_lds();
    __builtin_amdgcn_wave_barrier();
  }
  if (tmg && lane == 0) {
    atomicAdd(&out_cnt[0], (double)tAdv);
    atomicAdd(&out_cnt[1], (double)tDec);
    atomicAdd(&out_cnt[2], (double)tEmit);
  }
}

int32_t fdb_launch_hist2(hipStream_t stream, const DatasetView& v,
                         const WindowGrid& w, int nb, int hfunc,
                         double* out_sums, double* out_cnt,
                         double* out_max, double* out_min) {
  int grid = (v.num_series + H2_WAVES - 1) / H2_WAVES;
  const int cap = fdb_env_int("FDB_HIST_GRID", 8192);
  if (cap > 0 && grid > cap) grid = cap;
  // occupancy experiment knob; 5 waves/SIMD measured best
  const bool w4 = fdb_env_int("FDB_HIST_WAVES", 0) == 4;
  // 1=skip emits, 2=skip decodes, 8=phase split
  const int abl = fdb_env_int("FDB_HIST_ABLATE", 0);
  const auto kernel = hfunc == H2_SUM        ? hist2_kernel<4, H2_SUM>
                      : hfunc == H2_INCREASE ? hist2_kernel<5, H2_INCREASE>
                      : hfunc == H2_LAST     ? hist2_kernel<4, H2_LAST>
                      : w4                   ? hist2_kernel<4, H2_RATE>
                                             : hist2_kernel<5, H2_RATE>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(H2_WAVES * 64), 0, stream,
                     v.blob, v.dir, v.max_off, v.min_off, v.series_first,
                     v.series_nchunks, v.group_ids, v.num_series, w.start,
                     w.step, w.window, w.n, nb, out_sums, out_cnt, out_max,
                     out_min, abl);
  return fdb_launched("hist2_kernel");
}
