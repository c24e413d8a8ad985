// Gorilla-XOR double bitstream decode on the GPU (NibblePack.unpackDoubleXOR,
// NibblePack.scala:360-394) — the wavefront ballot/prefix design the
// north_star names: one wave per stream; each iteration the lanes
//
//  1. walk 8 group headers on uniform staged bytes (bitmask byte → ballot of
//     present values; nibble-width byte → group length), producing the 8
//     group offsets,
//  2. extract 64 packed XOR deltas in parallel (lane = one value: 8 groups ×
//     8 slots), and
//  3. reconstruct the chain with a wave-wide inclusive PREFIX-XOR (XOR is
//     associative — value[i] = first ^ delta[1] ^ … ^ delta[i]), carrying
//     lane 63's word into the next iteration.
//
// The streams decode bit-exactly against the host/oracle decoder (and
// roundtrip against packDoubles); 64 doubles retire per prefix pass.

#include <cstring>

#include "engine_internal.h"
#include "nibble_stream.h"

__device__ __forceinline__ uint64_t wave_incl_xor(uint64_t x, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    uint64_t t = __shfl_up(x, off);
    if (lane >= off) x ^= t;
  }
  return x;
}

// streams: concatenated packed bytes; offs[i]/lens[i] describe stream i,
// counts[i] its decoded length; outs land at out + out_offs[i]
__global__ __launch_bounds__(256)
void xor_unpack_kernel(const uint8_t* __restrict__ blob,
                       const int64_t* __restrict__ offs,
                       const int32_t* __restrict__ counts,
                       const int64_t* __restrict__ out_offs,
                       int num_streams,
                       double* __restrict__ out) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;

  for (int s = blockIdx.x * 4 + wave; s < num_streams; s += gridDim.x * 4) {
    const uint8_t* p = blob + offs[s];
    const int n = counts[s];
    double* o = out + out_offs[s];
    if (n < 1) continue;
    uint64_t carry = d_i64(p);               // first double stored raw
    if (lane == 0) memcpy(&o[0], &carry, 8);
    int pos = 8, i = 1;
    while (i < n) {
      // header walk for up to 8 groups (wave-uniform; staged 256 B). Whatever
      // the two header bytes hold, the widths nibble caps numBits at 64 and popc
      // caps the count at 8, so a group is at most 2 + 64 B: the first one
      // always fits under the 244-B limit and ngroups >= 1, corrupt input too.
      const uint8_t* gp = p + pos;
      uint32_t stg = estream_stage(gp, lane);
      const int shift = (int)((uintptr_t)gp & 3);
      // lane = (group, slot): each lane keeps its own group's header; a lane
      // whose group the walk did not reach keeps mask 0 and extracts 0
      NibbleGroup mine{0, 0, 0, 0};
      int mine_off = 0, off = 0, ngroups = 0;
      for (int g = 0; g < 8; g++) {
        const uint32_t mask = estream_byte_uni(true, stg, shift, gp, off);
        const NibbleGroup grp = nibble_group(
            mask, mask ? estream_byte_uni(true, stg, shift, gp, off + 1) : 0);
        if (off + grp.glen > 244) break;   // k+8+shift stays under the 64-dword stage
        if (g == lane >> 3) { mine = grp; mine_off = off; }
        off += grp.glen;
        ngroups++;
        if (i + ngroups * 8 >= n) break;      // enough values decoded
      }
      // The estream reads are SHUFFLES, so every lane must execute them
      // (inactive source lanes yield undefined data): only the value is
      // predicated, on the mask bit.
      const int k = lane & 7;
      const int bit = nibble_slot_bit(mine.mask, mine.numBits, k);
      const int koff = mine_off + 2 + (bit >> 3);
      const uint64_t w = estream_w64(true, stg, shift, gp, koff);
      const uint32_t b8 = estream_byte(true, stg, shift, gp, koff + 8);
      const uint64_t delta = nibble_slot_value(mine.mask, mine.numBits, mine.trail,
                                               k, bit, w, b8);
      // prefix-XOR reconstructs up to 64 chain values at once
      uint64_t chain = wave_incl_xor(delta, lane) ^ carry;
      const int avail = ngroups * 8;
      const int take = (n - i) < avail ? (n - i) : avail;
      if (lane < take) memcpy(&o[i + lane], &chain, 8);
      carry = __shfl(chain, take - 1);
      i += take;
      pos += off;
    }
    d_lds_fence();
  }
}

// host entry: decodes num_streams packed streams (host memory) on the GPU.
// offs/counts/out_offs are host arrays; out is a host buffer.
extern "C" int32_t fdb_gpu_unpack_doubles_xor(fdb_engine_t* e,
                                              const uint8_t* blob, int64_t blob_len,
                                              const int64_t* offs,
                                              const int32_t* counts,
                                              const int64_t* out_offs,
                                              int32_t num_streams,
                                              double* out, int64_t out_len) {
  hipStream_t stream = fdb_engine_stream(e);
  DevPtr<uint8_t> db;
  DevPtr<int64_t> doffs, dooffs;
  DevPtr<int32_t> dcounts;
  DevBuf dout;
  // +256 B tail pad so the wave staging never reads past the blob
  if (!db.alloc((size_t)blob_len + 256) || !doffs.alloc((size_t)num_streams * 8) ||
      !dcounts.alloc((size_t)num_streams * 4) ||
      !dooffs.alloc((size_t)num_streams * 8) || !dout.alloc((size_t)out_len * 8)) {
    fdb_set_error("xor decode: device allocation failed (out of HBM?)");
    return FDB_ERR;
  }
  HIP_CHECK(hipMemset(db.get() + blob_len, 0, 256));
  HIP_CHECK(hipMemcpy(db.get(), blob, (size_t)blob_len, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(doffs.get(), offs, (size_t)num_streams * 8, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dcounts.get(), counts, (size_t)num_streams * 4, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(dooffs.get(), out_offs, (size_t)num_streams * 8, hipMemcpyHostToDevice));
  int grid = (num_streams + 3) / 4;
  if (grid > 8192) grid = 8192;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(xor_unpack_kernel, dim3(grid), dim3(256), 0, stream,
                     db.get(), doffs.get(), dcounts.get(), dooffs.get(),
                     num_streams, dout.get());
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(stream));
  HIP_CHECK(hipMemcpy(out, dout.get(), (size_t)out_len * 8, hipMemcpyDeviceToHost));
  return FDB_OK;
}
