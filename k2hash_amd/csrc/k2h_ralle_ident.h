// k2hash_amd -- a blob's identity as the kernels that sort blobs by their stored hash hold and
// compare it (k2h_ralledata_dedup.hip, k2h_ralledata_diff.hip): the side record a gather leaves
// per participant, the end-aligned 16-byte compare of two byte ranges of one length, and the
// number of hash bits the pairs are sorted by.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "k2h_endwalk.h"

namespace k2h {

constexpr uint32_t kNone = 0xFFFFFFFFu;  // the index of a pair that stands for a non-participant

// What resolve needs of a participant; 32 bytes, so one aligned sector per record.
struct __attribute__((aligned(16))) Side {
  uint64_t sub;    // stored subhash
  uint64_t koff;   // the key's first byte, from `blobs`
  uint64_t klen;   // >= 1
  uint64_t attrs;  // 1: attrs_length != 0
};
static_assert(sizeof(Side) == 32, "two 16-byte loads");

__device__ __forceinline__ bool differ(uint4 x, uint4 y) {
  return ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0;
}

// Two keys of the same length kl >= 1, as ceil(kl / 16) chunks that end at each key's last
// byte; the lead bytes of chunk 0 (bytes before the keys) are masked off.
__device__ __forceinline__ bool same_key(const uint8_t* a, const uint8_t* b, uint64_t kl) {
  const uint64_t k = (kl + 15) >> 4;
  const uint32_t lead = (uint32_t)(16 * k - kl);
  const uint8_t* ca = a + kl - 16 * k;
  const uint8_t* cb = b + kl - 16 * k;
  if (differ(mask_lead(ld16(ca), lead), mask_lead(ld16(cb), lead))) return false;
  for (uint64_t q = 1; q < k; ++q)
    if (differ(ld16(ca + 16 * q), ld16(cb + 16 * q))) return false;
  return true;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The low hash bits the pairs are sorted by: 8 more than the blobs' number has, in whole
// bytes (the library sorts a byte per pass), at least 16.  Equal hashes are neighbours under
// any number of bits, and the sort stays stable; with 8 spare bits about one pair of neighbours
// in 256 shares the sorted bits without sharing the hash, and the walk steps over those.  At
// 8 Mi blobs this is 32 bits, half the passes of a 64-bit sort.
inline int sort_bits_for(uint64_t n) {
  int bits = 0;
  while (bits < 64 && (n - 1) >> bits) ++bits;
  bits = (bits + 8 + 7) / 8 * 8;
  return bits < 16 ? 16 : bits > 64 ? 64 : bits;
}

}  // namespace k2h
