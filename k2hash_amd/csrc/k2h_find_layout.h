// k2hash_amd -- the index a held stream is looked up through (include/k2hash_amd.h section 4e):
// its header and how the caller's buffer is cut into its columns.  Plain C++ without any device
// include, like k2h_layout.h: k2h_amd_ralledata_index_size is this layout over a null base, the launchers
// place the columns with the same function, and a host compiler alone builds and tests it
// (tests/test_find_layout.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "k2h_layout.h"

namespace k2h {

constexpr uint64_t kIndexMagic = 0x3158444932484B52ull;  // "RKH2IDX1"
constexpr size_t kIndexHeaderBytes = 256;
constexpr size_t kIndexSideBytes = 32;  // sizeof(Side), k2h_ralle_ident.h

// Written last, by a kernel: an index whose build has not finished on its stream has no magic.
struct IndexHeader {
  uint64_t magic;
  uint64_t n;      // the stream's blobs
  uint64_t size;   // the stream's bytes
  uint64_t bits;   // sort_bits_for(n): the hash column is monotone in hash & mask
  uint64_t mask;   // sort_mask(bits)
  uint64_t parts;  // P: the participants are the sorted positions [0, P)
};
static_assert(sizeof(IndexHeader) <= kIndexHeaderBytes, "the header column");

struct IndexCols {
  IndexHeader* head;
  uint64_t* hash;  // n, sorted on the low `bits` bits, stable: a hash's blobs in stream order
  uint32_t* idx;   // n, the blob of each sorted position; kNone behind the participants
  void* side;      // n side records by blob index; a non-participant's is never written
  size_t total;
};

inline IndexCols index_layout(void* base, uint64_t n) {
  Carver c(base);
  IndexCols k;
  k.head = (IndexHeader*)c.bytes(kIndexHeaderBytes);
  k.hash = c.take<uint64_t>(n);
  k.idx = c.take<uint32_t>(n);
  k.side = c.bytes(n * kIndexSideBytes);
  k.total = c.total();
  return k;
}

}  // namespace k2h
