// NibblePack streams read by one wave (NibblePack.scala:304-394): the
// register-staged byte window and the 8-value group decode. Included by
// hist2.hip (sect-delta histogram elements) and npxor.hip (XOR double
// streams) and by nothing else.
#ifndef FDB_NIBBLE_STREAM_H
#define FDB_NIBBLE_STREAM_H

#include "scan_common.h"

// --- wave-staged stream ---------------------------------------------------
// One coalesced dword-per-lane load stages the 256 B at p (rounded down to 4)
// into the wave's registers; byte/u64 reads of the window are then register
// shuffles instead of dependent global loads. `shift` is p & 3. A reader whose
// bytes leave the window passes staged = false and reads global memory.
// The load takes all 256 B whatever the stream's length, so the allocation
// carries a zeroed tail pad: dataset upload pads the blob 512 B (hist2 also
// prefetches the window after the current one), the npxor wrapper 256 B.
__device__ __forceinline__ uint32_t estream_stage(const uint8_t* p, int lane) {
  const uint8_t* base = (const uint8_t*)((uintptr_t)p & ~(uintptr_t)3);
  uint32_t d;
  memcpy(&d, base + lane * 4, 4);
  return d;
}
// `staged` must be WAVE-UNIFORM and every call site must have the full wave
// active: __shfl is ds_bpermute, and a source lane that is inactive (or a
// divergent caller) yields undefined data.
__device__ __forceinline__ uint32_t estream_byte(bool staged, uint32_t buf,
                                                 int shift, const uint8_t* g,
                                                 int k) {
  if (staged) {
    int kk = k + shift;
    uint32_t d = __shfl(buf, kk >> 2);
    return (d >> ((kk & 3) * 8)) & 0xff;
  }
  return g[k];
}
// wave-UNIFORM byte read from the staged window: kk>>2 is the same for every
// lane, so v_readlane (scalar result, no LDS pipe) replaces ds_bpermute —
// the header walks of the NibblePack parsers are built from these
__device__ __forceinline__ uint32_t estream_byte_uni(bool staged, uint32_t buf,
                                                     int shift, const uint8_t* g,
                                                     int k) {
  if (staged) {
    int kk = k + shift;
    uint32_t d = __builtin_amdgcn_readlane(buf, kk >> 2);
    return (d >> ((kk & 3) * 8)) & 0xff;
  }
  return g[k];
}

// little-endian 8-byte window at offset k (per-lane k; bpermute shuffles)
__device__ __forceinline__ uint64_t estream_w64(bool staged, uint32_t buf,
                                                int shift, const uint8_t* g,
                                                int k) {
  if (staged) {
    int kk = k + shift;
    int dw = kk >> 2;
    uint64_t a = __shfl(buf, dw);
    uint64_t b = __shfl(buf, dw + 1);
    uint64_t c = __shfl(buf, dw + 2);
    int sh = (kk & 3) * 8;
    uint64_t w = (a | (b << 32)) >> sh;
    if (sh) w |= c << (64 - sh);
    return w;
  }
  uint64_t w;
  memcpy(&w, g + k, 8);
  return w;
}

// --- 8-value group ----------------------------------------------------------
// A group is a mask byte (bit k set: value k is non-zero), then, unless the
// mask is 0, a widths byte (high nibble: nibbles per value - 1; low nibble:
// trailing zero nibbles dropped) and the set values packed numBits each.
struct NibbleGroup {
  uint32_t mask;
  int numBits, trail, glen;   // glen: bytes of the whole group, header included
};
// widths is read only when mask != 0 (pass 0 otherwise)
__device__ __forceinline__ NibbleGroup nibble_group(uint32_t mask, uint32_t widths) {
  if (mask == 0) return NibbleGroup{0, 0, 0, 1};
  const uint32_t numBits = ((widths >> 4) + 1) * 4;
  return NibbleGroup{mask, (int)numBits, (int)(widths & 0x0f) * 4,
                     (int)(2 + (numBits * __popc(mask) + 7) / 8)};
}
// bit offset of value k inside the group's packed values (which start 2 bytes
// into the group): the caller fetches w64 = the 8 bytes at (bit >> 3) and
// b8 = the byte after them, then extracts with nibble_slot_value
__device__ __forceinline__ int nibble_slot_bit(uint32_t mask, int numBits, int k) {
  return __popc(mask & ((1u << k) - 1)) * numBits;
}
// value k of the group, whose bits start at `bit`; 0 when the mask has no bit k
__device__ __forceinline__ uint64_t nibble_slot_value(uint32_t mask, int numBits,
                                                      int trail, int k, int bit,
                                                      uint64_t w64, uint32_t b8) {
  const int sh = bit & 7;
  uint64_t v = w64 >> sh;
  if (numBits > 64 - sh) v |= (uint64_t)b8 << (64 - sh);   // spills into byte 9
  const uint64_t m = numBits >= 64 ? ~0ULL : ((1ULL << numBits) - 1);
  return (mask & (1u << k)) ? (v & m) << trail : 0;
}

#endif  // FDB_NIBBLE_STREAM_H
