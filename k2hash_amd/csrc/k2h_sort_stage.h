// k2hash_amd -- the host side of the two library sequences the stream and log launchers share
// ("Scratch policy").  No kernel is defined here.  Both types are class templates
// so that a translation unit instantiates the library kernels of the calls it makes and no others.
//
// SortStage: "order N (hash, index) pairs by the low bits of the hash".  A launcher's gather
// leaves each participant's hash by index (hashes()) and each tile's participant count; then
//   scan_tiles  an exclusive sum over the tiles + 1 counts;
//   compact     the launcher's kernel (ralle_compact_kernel of k2h_ralle_ident.h, or fold's own)
//               lays the pairs out in keys_in / idx_in: participants first, in index order, every
//               other slot behind them as (~0, kNone);
//   sort        hipcub::DeviceRadixSort::SortPairs into keys_out / idx_out on the hash's low
//               sort_bits_for(pairs) bits only (k2h_layout.h): stable, so entries of one hash are
//               neighbours in index order, now and then with an entry of another hash among them;
//               the resolve kernels compare under mask() and step over those;
//   max_scan    (diff, subkeys) an inclusive max-scan over a mark column: for every sorted
//               position the nearest marked position at or before it.
// PlaceRank: the two in-place exclusive sums that turn per-slot output sizes and emitted flags
// into places and ranks (unlink, apply, delta).
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "k2h_scratch.h"

namespace k2h {

struct RalleMaxU32 {
  __host__ __device__ __forceinline__ uint32_t operator()(uint32_t x, uint32_t y) const { return x > y ? x : y; }
};

// Every call is gated on tr.ok(): after a first error nothing more is enqueued.  The library's
// storage (`tmp`, at least tmp_bytes()) stays the launcher's column: apply shares it with its
// PlaceRank.  measure_max_scan follows measure in a launcher that calls max_scan.
template <class Key = uint64_t>
struct SortStage {
  static_assert(sizeof(Key) == 2 * sizeof(uint32_t), "a key column holds two 32-bit columns");
  uint64_t pairs = 0, tiles = 0;
  int bits = 0;
  size_t tile_bytes = 0, sort_bytes = 0, max_bytes = 0;
  Key *keys_in = nullptr, *keys_out = nullptr;
  uint32_t *idx_in = nullptr, *idx_out = nullptr;
  uint64_t *tile_count = nullptr, *tile_base = nullptr;  // tiles + 1 entries each

  void measure(FirstError& tr, uint64_t pairs_, uint64_t tiles_, hipStream_t stream) {
    pairs = pairs_;
    tiles = tiles_;
    bits = sort_bits_for(pairs);
    tr(hipcub::DeviceScan::ExclusiveSum(nullptr, tile_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, tiles + 1, stream));
    tr(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const Key*)nullptr, (Key*)nullptr,
                                          (const uint32_t*)nullptr, (uint32_t*)nullptr, pairs, 0, bits, stream));
  }
  void measure_max_scan(FirstError& tr, hipStream_t stream) {
    tr(hipcub::DeviceScan::InclusiveScan(nullptr, max_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                         RalleMaxU32(), pairs, stream));
  }
  size_t tmp_bytes() const { return std::max({tile_bytes, sort_bytes, max_bytes}); }
  SortStage take(Carver& c) const {  // the measured stage with its six columns placed
    SortStage s = *this;
    s.keys_in = c.take<Key>(pairs);
    s.keys_out = c.take<Key>(pairs);
    s.idx_in = c.take<uint32_t>(pairs);
    s.idx_out = c.take<uint32_t>(pairs);
    s.tile_count = c.take<uint64_t>(tiles + 1);
    s.tile_base = c.take<uint64_t>(tiles + 1);
    return s;
  }
  // Entry `tiles` of the counts is 0, so entry `tiles` of their exclusive scan is the total.
  void clear(FirstError& tr, hipStream_t stream) const { tr(hipMemsetAsync(tile_count + tiles, 0, 8, stream)); }
  void scan_tiles(FirstError& tr, void* tmp, hipStream_t stream) const {
    size_t bytes = tile_bytes;
    if (tr.ok()) tr(hipcub::DeviceScan::ExclusiveSum(tmp, bytes, tile_count, tile_base, tiles + 1, stream));
  }
  void sort(FirstError& tr, void* tmp, hipStream_t stream) const {
    size_t bytes = sort_bytes;
    if (tr.ok())
      tr(hipcub::DeviceRadixSort::SortPairs(tmp, bytes, (const Key*)keys_in, keys_out, (const uint32_t*)idx_in, idx_out,
                                            pairs, 0, bits, stream));
  }
  uint64_t mask() const { return sort_mask(bits); }
  void max_scan(FirstError& tr, void* tmp, const uint32_t* in, uint32_t* out, hipStream_t stream) const {
    size_t bytes = max_bytes;
    if (tr.ok()) tr(hipcub::DeviceScan::InclusiveScan(tmp, bytes, in, out, RalleMaxU32(), pairs, stream));
  }
  // Until the sort has written it, keys_out holds the gather's hashes by index.
  Key* hashes() const { return keys_out; }
  // Free once the sort has read them, its input columns: a mark column takes the index column's
  // place, the max-scan's output and one more 32-bit column the two halves of the key column's.
  uint32_t* mark() const { return idx_in; }
  uint32_t* scanned() const { return (uint32_t*)keys_in; }
  uint32_t* second() const { return (uint32_t*)keys_in + pairs; }
};

// `count` slots' sizes and emitted flags, entry `count` of each 0, summed in place: the last
// entries are the totals.  The columns are the launcher's (delta's place may be the caller's).
template <class Place = uint64_t>
struct PlaceRank {
  uint64_t entries = 0;  // count + 1
  size_t place_bytes = 0, rank_bytes = 0;

  void measure(FirstError& tr, uint64_t count, hipStream_t stream) {
    entries = count + 1;
    tr(hipcub::DeviceScan::ExclusiveSum(nullptr, place_bytes, (Place*)nullptr, (Place*)nullptr, entries, stream));
    tr(hipcub::DeviceScan::ExclusiveSum(nullptr, rank_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, entries, stream));
  }
  size_t tmp_bytes() const { return std::max(place_bytes, rank_bytes); }
  void scan(FirstError& tr, void* tmp, Place* place, uint32_t* rank, hipStream_t stream) const {
    size_t b8 = place_bytes, b4 = rank_bytes;
    if (tr.ok()) tr(hipcub::DeviceScan::ExclusiveSum(tmp, b8, place, place, entries, stream));
    if (tr.ok()) tr(hipcub::DeviceScan::ExclusiveSum(tmp, b4, rank, rank, entries, stream));
  }
};

}  // namespace k2h
