// k2hash_amd -- what the two RALLEDATA producers share (k2h_ralledata.hip: records as CSR
// streams; k2h_ralledata_recs.hip: records as ranges into a scanned file): the LDS-only
// barrier, the 8-lane copy of the group / direct form, and the packed segment table entry.
#pragma once
#include "k2h_endwalk.h"

namespace k2h {
namespace {

// Workgroup barrier over LDS only (see its use in the gather kernels).
__device__ __forceinline__ void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Group form (oversize tiles): G lanes per record, 64/G records per wave.  Lane q of a group
// writes header piece q (5 x 16 B) and copies bytes [16q + 16Gj, +16) of each segment,
// so a group's loads and stores are consecutive 16-byte pieces instead of one lane
// streaming a whole record.  A segment's last partial piece is the 16 bytes ENDING at
// its last byte (they overlap the previous piece with the same bytes, so the order of
// the two stores does not matter); only segments shorter than 16 bytes are copied byte
// by byte.  G = 8 keeps most lanes busy on BASELINE-like records (keys 8-64 B, values
// 0-256 B).
template <int G>
__device__ __forceinline__ void group_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t len,
                                           uint32_t q) {
  uint64_t full = len & ~15ull;
  for (uint64_t j = 16ull * q; j < full; j += 16ull * G)
    *reinterpret_cast<u32x4_ua*>(dst + j) = *reinterpret_cast<const u32x4_ua*>(src + j);
  if (full == len) return;
  if (len >= 16) {
    if (q == G - 1)
      *reinterpret_cast<u32x4_ua*>(dst + len - 16) = *reinterpret_cast<const u32x4_ua*>(src + len - 16);
    return;
  }
  for (uint64_t t = full + q; t < len; t += G) dst[t] = src[t];  // the <= 15 tail bytes
}

// Segment table entry: span byte y of the segment sits at img[y + adj]; end = where the
// segment ends in the span.  Both fit 16 bits once the block's bytes fit the LDS image.
__device__ __forceinline__ uint32_t seg_pack(int32_t adj, int32_t end) {
  return (uint32_t)(uint16_t)(int16_t)adj | ((uint32_t)end << 16);
}
__device__ __forceinline__ int2 seg_unpack(uint32_t v) { return int2{(int32_t)(int16_t)(v & 0xffffu), (int32_t)(v >> 16)}; }

}  // namespace
}  // namespace k2h
