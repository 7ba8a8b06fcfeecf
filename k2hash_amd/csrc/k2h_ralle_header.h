// k2hash_amd -- a RALLEDATA blob's header as the consumer-side kernels judge it
// (k2h_ralledata_check.hip, k2h_ralledata_dedup.hip): the ten fields and the header tests of
// K2HShm::SetElementByBinArray, in its order (lib/k2hshmdirect.cc:351, 355, 361-364).
#pragma once
#include "k2h_endwalk.h"
#include "k2h_kernels.h"

namespace k2h {

constexpr int kHdr = K2H_AMD_RALLEDATA_HEADER;

// The header's own tests, in SetElementByBinArray's order; L is the blob's length.
// f: hash, subhash, key / val / skey / attrs length, key / val / skey / attrs pos.
__device__ __forceinline__ uint32_t classify(const uint64_t (&f)[10], uint64_t L) {
  if (!(f[2] | f[3] | f[4] | f[5])) return K2H_AMD_RALLE_EMPTY;  // :351
  if (!f[2]) return K2H_AMD_RALLE_NO_KEY;                        // :355
  bool bad = false;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const uint64_t len = f[2 + s], pos = f[6 + s];
    // pos is an off_t; pos + len as an integer must not pass the blob's end (a 64-bit
    // wrap of the sum is such a pass).  A length-0 segment's pos is ignored (:362-364).
    bad |= len && ((int64_t)pos < kHdr || len > L || pos > L - len);
  }
  return bad ? K2H_AMD_RALLE_BAD_RANGE : K2H_AMD_RALLE_OK;
}

__device__ __forceinline__ void load_fields(const uint8_t* p, uint64_t (&f)[10]) {
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    const uint4 v = ld16(p + 16 * c);
    f[2 * c] = pack2(v.x, v.y);
    f[2 * c + 1] = pack2(v.z, v.w);
  }
}

}  // namespace k2h
