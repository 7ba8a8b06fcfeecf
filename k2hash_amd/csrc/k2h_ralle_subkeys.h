// k2hash_amd -- a serialized K2HSubKeys segment walked on the device
// (k2h_ralledata_subkeys.hip): what K2HSubKeys::Serialize(const unsigned char*, size_t) parses
// (lib/k2hsubkeys.cc:113-156) and K2HPage::GetSubKeys then keeps (lib/k2hpage.cc:274-299).
//
// The segment S[0, L): a u64 count, then `count` entries of u64 length + length bytes.  A
// zero-length entry is refused by insert (:302-305) and skipped, parsing goes on; a length field
// or a name that does not fit makes Serialize return false, and GetSubKeys then throws the whole
// list away: a rejected segment means NO subkeys, not the entries read so far.  Bytes after the
// last entry are ignored, count == 0 is an accepted empty list.
//
// One departure from the reference, the counterpart of the attrs walk's (k2h_ralle_attrs.h).
// The reference starts rest_length at the whole segment length although its read position is
// already past the count, so on a malformed segment it accepts an entry that runs up to 8 bytes
// past the segment's end, and it reads the count itself out of bounds when L is 1..7.  The
// rule here is the strict one, which never reads outside the segment:
//   L == 0: no list.  L < 8: BAD.  Else pos = 8 and `count` times: BAD if L - pos < 8;
//   len = the u64 at pos, pos += 8; BAD if L - pos < len; an edge when len > 0; pos += len.
// Every segment the reference's own writer produces is judged the same by both rules; they
// differ only where the reference reads out of bounds (tests/golden/gen_ralle_subkeys.cc hands
// the reference no such segment).
//
// One lane walks one segment, a serial chain: the next entry's place depends on this entry's
// length, one 8-byte load per entry, each wholly inside [S, S + L) at any alignment of S.  No
// name byte is read.  A count field larger than the segment can hold ends in BAD after at most
// L / 8 steps.
#pragma once
#include "k2h_ralle_attrs.h"

namespace k2h {

// Walks S[0, L), L >= 1.  emit(k, pos, len) for the k-th edge: the name S[pos, pos + len).
// Returns false for a BAD segment (what was emitted before is then void), else true with the
// number of edges in `edges`.
template <class Emit>
__device__ __forceinline__ bool walk_subkeys(const uint8_t* S, uint64_t L, uint64_t& edges, Emit emit) {
  edges = 0;
  if (L < 8) return false;
  uint64_t pos = 8;
  for (uint64_t count = ld8(S); count; --count) {
    if (L - pos < 8) return false;
    const uint64_t len = ld8(S + pos);
    pos += 8;
    if (L - pos < len) return false;
    if (len) {
      emit(edges, pos, len);
      ++edges;
    }
    pos += len;
  }
  return true;
}

}  // namespace k2h
