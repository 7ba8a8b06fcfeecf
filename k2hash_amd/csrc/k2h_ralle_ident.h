// k2hash_amd -- a blob's identity as the kernels that sort blobs by their stored hash hold and
// compare it (dedup, diff, subkeys, apply): the side record a gather leaves per participant and the
// end-aligned 16-byte compare of two byte ranges of one length.  Below those, the kernels on either
// side of the sort stage (k2h_sort_stage.h has the stage's order and the library calls) with the
// host helpers that launch them from a SortStage: the compact kernel that lays the pairs out for
// the sort, the mark kernel that feeds the max-scan (diff, subkeys), and the backward walk to the
// last held entry of an identity.  k2h_archive_fold.hip has a side record and a compact kernel of
// its own and does not include this header.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stddef.h>
#include <stdint.h>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_scratch.h"
#include "k2h_sort_stage.h"

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

__device__ __forceinline__ uint64_t ralle_shfl_u64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
  return pack2(lo, hi);
}

constexpr int kIdentBlobs = 256;  // gather / compact: blobs per 256-thread block, one per thread

// The sort's input: participant g at its rank among the participants, every other blob behind
// all m of them and behind `extra` more places that the caller fills itself, as (~0, kNone) --
// so a non-participant sorts behind every participant of any hash and ends every walk that
// reaches it (tile_base = the scanned tile counts, entry ntiles = m).
// (A template only so that every file that launches it holds its own copy.)
template <int BLOBS = kIdentBlobs>
__global__ __launch_bounds__(BLOBS) void ralle_compact_kernel(const uint8_t* __restrict__ part,
                                                              const uint64_t* __restrict__ hash, uint64_t n,
                                                              const uint64_t* __restrict__ tile_base, uint64_t ntiles,
                                                              uint64_t extra, uint64_t* __restrict__ keys,
                                                              uint32_t* __restrict__ idx) {
  typedef hipcub::BlockScan<uint32_t, BLOBS> Scan;
  __shared__ typename Scan::TempStorage tmp;
  const uint64_t g = (uint64_t)blockIdx.x * BLOBS + threadIdx.x;
  const uint32_t p = g < n && part[g] ? 1u : 0u;
  uint32_t rank;
  Scan(tmp).ExclusiveSum(p, rank);
  if (g >= n) return;
  const uint64_t before = tile_base[blockIdx.x] + rank;  // participants before blob g
  const uint64_t pos = p ? before : tile_base[ntiles] + extra + (g - before);
  keys[pos] = p ? hash[g] : ~0ull;
  idx[pos] = p ? (uint32_t)g : kNone;
}

// mark[p] = p + 1 for a sorted entry with an index below nb (a held blob), else 0: the
// max-scan's input.
template <int BLOCK = 256>
__global__ __launch_bounds__(BLOCK) void ralle_mark_kernel(const uint32_t* __restrict__ idx, uint64_t n, uint64_t nb,
                                                           uint32_t* __restrict__ mark) {
  const uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (p < n) mark[p] = idx[p] < nb ? (uint32_t)(p + 1) : 0u;
}

// The two launched from a stage: the pairs of the n slots with participant bytes `part` into the
// sort's input; the sorted entries below `held` marked in the stage's mark column.
template <int BLOBS>
void ralle_compact(FirstError& tr, const SortStage<>& st, const uint8_t* part, uint64_t n, uint64_t extra,
                   hipStream_t stream) {
  if (!tr.ok()) return;
  ralle_compact_kernel<BLOBS><<<(unsigned)st.tiles, BLOBS, 0, stream>>>(part, st.hashes(), n, st.tile_base, st.tiles,
                                                                      extra, st.keys_in, st.idx_in);
  tr(hipGetLastError());
}
template <int BLOCK>
void ralle_mark(FirstError& tr, const SortStage<>& st, uint64_t held, hipStream_t stream) {
  if (!tr.ok()) return;
  ralle_mark_kernel<BLOCK><<<(unsigned)((st.pairs + BLOCK - 1) / BLOCK), BLOCK, 0, stream>>>(st.idx_out, st.pairs, held,
                                                                                           st.mark());
  tr(hipGetLastError());
}

// The last held entry (index below nb) with the identity of `sa` and hash h: backward from
// sorted position q0 (1 + a position, 0: none) over the run's held entries while the sorted
// bits agree.  Returns its index, kNone when there is none.  x: the buffer sa's key offset counts
// from, y: the held entries'.  The walk hands out the index only: a caller that needs the held
// entry's side record reads side[index] behind the walk.  A record carried out of the loop was
// seen to keep the caller's initial value for keys of more than 16 bytes in one build of
// k2h_ralledata_diff.hip, and the index alone also leaves the loop fewer
// registers to keep.
__device__ __forceinline__ uint32_t last_held(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
                                              const Side* __restrict__ side, uint64_t q0, uint64_t h, uint64_t mask,
                                              uint64_t nb, const Side& sa, const uint8_t* x, const uint8_t* y) {
  for (uint64_t q = q0; q > 0; --q) {
    const uint64_t hq = keys[q - 1];
    if ((hq ^ h) & mask) break;
    if (hq != h) continue;  // another hash with the same sorted bits
    const uint32_t c = idx[q - 1];
    if (c >= nb) break;  // (never: in a run every entry before a held entry is held)
    const Side sc = side[c];
    if (sc.sub != sa.sub || sc.klen != sa.klen || !same_key(x + sa.koff, y + sc.koff, sa.klen)) continue;
    return c;
  }
  return kNone;
}

}  // namespace k2h
