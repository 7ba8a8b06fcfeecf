// k2hash_amd -- the two builtin times of a serialized K2HAttrs segment, read on the device
// (k2h_ralledata_times.hip, k2h_ralledata_dedup.hip): what K2hAttrBuiltin::GetTime answers for
// "mtime" and "expire" (lib/k2hattrbuiltin.cc:864-883) after K2HAttrs::Serialize(const unsigned
// char*, size_t) has parsed the segment (lib/k2hattrs.cc:121-166).
//
// The segment A[0, AL): a u64 count, then entries of u64 kl, u64 vl, kl key bytes, vl value
// bytes.  Serialize stops at the first entry that does not fit and keeps the ones before it;
// insert refuses kl == 0 and lets an entry replace an earlier one of the same key (:356-363).
// find(const char*) looks a name up with its NUL, so the keys are "mtime\0" (kl 6) and
// "expire\0" (kl 7), and a time is present exactly when the LAST accepted entry of that key
// has vl == 16 (a struct timespec: int64 tv_sec, int64 tv_nsec); a later entry with another vl
// hides an earlier good one.
//
// One departure from the reference: it forms 16 + kl + vl in size_t and, where that sum
// wraps, goes on to read out of bounds.  Here the sum is never formed: an entry with
// kl > rest - 16 or vl > rest - 16 - kl ends the walk.
//
// One lane walks one segment, a serial chain: the next entry's place depends on this entry's
// two lengths, one 16-byte load per step.  Off that chain a step reads the 8 bytes that end
// with the key's last byte, only when kl is 6 or 7 (they begin inside the entry's own length
// fields, so at most 7 of them are key bytes), and the 16 value bytes only of a key that
// matched.  Every load lies wholly inside [A, A + AL) -- the end-aligned technique of
// k2h_endwalk.h, which here needs no masking -- at any alignment of A.
#pragma once
#include "k2h_endwalk.h"

namespace k2h {

constexpr uint32_t kAttrMtime = 0x1u;   // K2H_AMD_TIMES_MTIME
constexpr uint32_t kAttrExpire = 0x2u;  // K2H_AMD_TIMES_EXPIRE
constexpr uint32_t kAttrCut = 0x4u;     // K2H_AMD_TIMES_CUT: the walk ended before `count` entries

struct AttrTimes {
  int64_t msec, mnsec;  // 0, 0 without kAttrMtime
  int64_t esec, ensec;  // 0, 0 without kAttrExpire
  uint32_t flags;
};

// Dynamic LDS a kernel that walks attrs is launched with and never touches: 64 KiB per
// 256-thread block leave two blocks resident on a CU, two waves per SIMD instead of eight.  The
// lanes in flight then hold a quarter of the lines between them; supposedly a chain's later
// steps then find the line its first step fetched still in L2.  Measured on 10.5 M blobs: the
// times call takes 1.05 ms where it takes 1.53 ms at full occupancy, and 6, 5 and 3 resident
// blocks lie in between in that order.
constexpr size_t kWalkLdsBytes = 64 << 10;

typedef uint64_t u64_ua __attribute__((aligned(1)));  // 8 bytes at any alignment

__device__ __forceinline__ uint64_t ld8(const uint8_t* p) { return *reinterpret_cast<const u64_ua*>(p); }

// "mtime\0" and "expire\0" as little-endian integers of 6 and 7 bytes.
constexpr uint64_t kKeyMtime = 0x0000656D69746Dull;
constexpr uint64_t kKeyExpire = 0x00657269707865ull;

// sec first, signed, nsec as stored (no normalisation): lib/k2hattrbuiltin.cc:854-860,
// lib/k2hshmdirect.cc:180-188, :402, :416.
__device__ __forceinline__ bool time_less(int64_t as, int64_t an, int64_t bs, int64_t bn) {
  return as < bs || (as == bs && an < bn);
}

__device__ __forceinline__ AttrTimes walk_attrs(const uint8_t* A, uint64_t AL) {
  AttrTimes t = {0, 0, 0, 0, 0};
  if (AL < 8) {
    if (AL) t.flags = kAttrCut;
    return t;
  }
  uint64_t count = ld8(A);
  uint64_t pos = 8, rest = AL - 8;
  for (; count; --count) {
    if (rest < 16) break;
    const uint4 v = ld16(A + pos);
    const uint64_t kl = pack2(v.x, v.y), vl = pack2(v.z, v.w);
    if (kl > rest - 16 || vl > rest - 16 - kl) break;
    if (kl == 6 || kl == 7) {
      const uint64_t key = ld8(A + pos + 8 + kl) >> (8 * (8 - kl));
      const bool m = kl == 6 && key == kKeyMtime, x = kl == 7 && key == kKeyExpire;
      if (m | x) {
        const uint32_t bit = m ? kAttrMtime : kAttrExpire;
        int64_t sec = 0, nsec = 0;
        if (vl == 16) {
          const uint4 w = ld16(A + pos + 16 + kl);
          sec = (int64_t)pack2(w.x, w.y);
          nsec = (int64_t)pack2(w.z, w.w);
          t.flags |= bit;
        } else {
          t.flags &= ~bit;
        }
        if (m) {
          t.msec = sec;
          t.mnsec = nsec;
        } else {
          t.esec = sec;
          t.ensec = nsec;
        }
      }
    }
    pos += 16 + kl + vl;
    rest -= 16 + kl + vl;
  }
  if (count) t.flags |= kAttrCut;
  return t;
}

}  // namespace k2h
