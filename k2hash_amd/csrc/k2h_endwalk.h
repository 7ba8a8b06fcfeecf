// k2hash_amd -- the end-aligned key walk shared by every kernel whose lanes hash keys of
// their own length (k2h_csr.hip, k2h_ralledata.hip, k2h_archive_dev.hip, k2h_import_dev.hip).
//
// A key of len >= 1 bytes is hashed as k = ceil(len / 16) whole 16-byte chunks that END at
// its last byte.  Chunk 0 starts p = 16 k - len bytes before the key; its p lead bytes are
// zeroed and the state starts at S_p = seed * P^-p (SpadTable, make_spad): a zero byte is a
// bare multiply, so the p lead steps land exactly on the seed.  No byte tail, and the second
// hash (the state before the key's final byte, lib/k2hashfunc.cc:83-85) is always the
// snapshot before byte 15 of the last chunk.
//
// A caller keeps what is its own: how a chunk is fetched (pointer, checked file view, LDS),
// where its buffer starts (chunk 0 may begin before it: chunk0_from_bytes), and what the
// result means (empty key -> 0, one byte -> h2 = h1, a C string's h1 = raw * P, h2 = raw).
#pragma once
#include "k2h_fnv_device.h"

namespace k2h {

// 16 bytes at any alignment.
__device__ __forceinline__ uint4 ld16(const uint8_t* p) {
  u32x4_ua v = *reinterpret_cast<const u32x4_ua*>(p);
  return make_uint4(v.x, v.y, v.z, v.w);
}

// Zero the first p (0..15) bytes of a chunk.
__device__ __forceinline__ uint4 mask_lead(uint4 c, uint32_t p) {
  // word mask = low half of (~0 << clamp(8p - base, 0, 32)): sub, med3, 64-bit shift
  // (a 32-bit shift cannot produce the all-zero mask), no compares or selects
  int32_t sh = (int32_t)(8u * p);
  auto m = [sh](int32_t base) -> uint32_t {
    int32_t t = sh - base;
    t = t < 0 ? 0 : (t > 32 ? 32 : t);
    return (uint32_t)(~0ull << t);
  };
  return make_uint4(c.x & m(0), c.y & m(32), c.z & m(64), c.w & m(96));
}

// The same mask by compares and selects, the form the import and archive walkers had.  Their
// callers keep it so that their kernels' code stays the parent's.  The timing evidence for it
// is mixed: in two same-process A/B runs and a kernel trace the TSV scan's
// pass A (tsv_a_kernel, whose only code difference was this mask) ran 1.3 % longer with the
// shift form; in a third run both forms and the parent timed the same.
__device__ __forceinline__ uint4 mask_lead_sel(uint4 c, uint32_t p) {
  const uint32_t m0 = p >= 4 ? 0u : ~0u << (8 * p), m1 = p >= 8 ? 0u : p <= 4 ? ~0u : ~0u << (8 * (p - 4));
  const uint32_t m2 = p >= 12 ? 0u : p <= 8 ? ~0u : ~0u << (8 * (p - 8)), m3 = p <= 12 ? ~0u : ~0u << (8 * (p - 12));
  return make_uint4(c.x & m0, c.y & m1, c.z & m2, c.w & m3);
}

// Chunk 0 of a key that starts fewer than p bytes into its buffer, so that a 16-byte load
// would touch bytes below the buffer: only the key's own first 16 - p bytes are read, one
// at a time through byte(i) (i = 0 is the key's first byte), and the lead bytes are zero.
// (The loop the import walker had: with it the import kernels' code is the parent's.)
template <class ByteAt>
__device__ __forceinline__ uint4 chunk0_from_bytes(uint32_t p, ByteAt byte) {
  uint32_t w[4] = {0, 0, 0, 0};
  for (uint32_t j = p; j < 16; ++j) w[j >> 2] |= byte(j - p) << (8 * (j & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// The walk: k >= 1 chunks, chunk 0 already fetched and its p lead bytes zeroed (mask_lead),
// chunk q >= 1 from fetch(q), loaded one ahead of the chunk being hashed (AHEAD) or after it
// (the RALLEDATA kernel, at its 64-VGPR cap, has no room for a second chunk in flight).  spad is
// the S_p table.  Returns the hash of the whole key in h and, with SNAP, the state before the
// key's final byte in pre; without SNAP (C-string callers, whose NUL is a bare multiply on top
// of h) pre is not written.
template <bool SNAP = true, bool AHEAD = true, class K, class Fetch>
__device__ __forceinline__ void end_aligned_walk(K k, uint32_t p, uint4 c0, const uint64_t* spad, Fetch fetch,
                                                 uint64_t& h, uint64_t& pre) {
  const uint64_t st = spad[p];
  uint32_t lo = (uint32_t)st, hi = (uint32_t)(st >> 32);
  uint4 c = c0;
  for (K q = 1; q < k; ++q) {
    uint4 nx;
    if constexpr (AHEAD) nx = fetch(q);
    fnv_chunk16(lo, hi, c);
    if constexpr (!AHEAD) nx = fetch(q);
    c = nx;
  }
  if constexpr (SNAP) {
    uint32_t lo2, hi2;
    fnv_chunk16_last(lo, hi, lo2, hi2, c);
    pre = pack2(lo2, hi2);
  } else {
    fnv_chunk16(lo, hi, c);
  }
  h = pack2(lo, hi);
}

// The same over a plain pointer: chunk q at c0p + 16 q, c0p = key end - 16 k; bytes below
// `low` (the buffer's start) are never read.
template <bool SNAP = true, bool AHEAD = true, class K>
__device__ __forceinline__ void end_aligned_walk_ptr(K k, uint32_t p, const uint8_t* c0p, const uint8_t* low,
                                                     const uint64_t* spad, uint64_t& h, uint64_t& pre) {
  const uint4 c0 = c0p >= low ? ld16(c0p) : chunk0_from_bytes(p, [=](uint32_t i) { return (uint32_t)c0p[p + i]; });
  end_aligned_walk<SNAP, AHEAD>(k, p, mask_lead(c0, p), spad, [=](K q) { return ld16(c0p + 16 * q); }, h, pre);
}

}  // namespace k2h
