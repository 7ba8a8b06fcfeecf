// k2hash_amd -- RALLEDATA consumer side: drop the superseded duplicates of a blob stream in
// device memory (include/k2hash_amd.h section 4b').
//
// K2HShm::SetElementByBinArray (lib/k2hshmdirect.cc:343-478) finds the element a blob
// addresses by the blob's STORED hash (GetCKIndex, :373), its stored hash and subhash
// (GetElementList, :377) and its key bytes (GetElement, :378): those four -- hash, subhash,
// key_length, key -- are the blob's identity.  Blob i is superseded when the nearest later
// blob j of the same identity exists and neither i nor j carries attrs: whatever the table
// held for that key, i either is overwritten by j unconditionally (an element without an attrs
// page: GetAttrs gives NULL, lib/k2hshm.cc:2059-2073, so :382 is skipped) or returns early
// exactly as j does (:402-405, :421-427).  A blob with attrs is never dropped and never
// causes a drop.
//
// k2h_amd_ralledata_dedup_mtime (section 4b'''') runs the same three stages with another drop
// rule, for streams whose blobs carry the builtin mtime: its gather also walks the attrs of
// the participants that have some (k2h_ralle_attrs.h) and leaves each mtime for resolve, where
// i is superseded by j when i has no mtime, or both have one and m_i < m_j and m_i < pts.
// The kernels are templates on that bool; the plain rule's instantiations are the code they
// were.
//
// Three stages, all on the caller's stream (the scan, compact and sort between gather and resolve
// are the sort stage of k2h_sort_stage.h):
//   gather   one lane per blob: span, header and classify (k2h_ralle_header.h, shared with
//            the check kernel); a participant leaves its stored hash and a 32-byte side
//            record (subhash, absolute key offset, key length, attrs bit), a tile its count.
//   sort     the (hash, index) pairs on the hash's low bits: blobs of one stored hash are
//            neighbours in stream order, now and then with a blob of another hash among them.
//   resolve  one lane per sorted position p.  Other sorted bits at p + 1: the blob is kept
//            and nothing more is read.  Else the lane walks forward from p + 1 to the first
//            entry with its hash, subhash, key length and key bytes -- `by` -- and applies
//            the attrs rule.
//            A run of r equal keys costs O(1) per lane (the match is at p + 1).  A run of r
//            DISTINCT keys under one stored hash costs O(r) per lane, O(r^2) in all: only a
//            crafted stream (or one with wrong hash fields, which k2h_amd_ralledata_check
//            finds) has such runs.
//
// Blob i = blobs[off[i], off[i+1]).  No byte outside [0, size) is read: a key is compared in
// 16-byte chunks that END at its last byte, and it starts at or after byte 80 of its blob,
// so chunk 0 never begins below the buffer and no chunk passes the key's end.  Nothing of a
// non-participant is read beyond its header, and nothing of a blob whose span is bad or
// whose `consider` byte is 0.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <mutex>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_ralle_attrs.h"
#include "k2h_ralle_header.h"
#include "k2h_ralle_ident.h"

namespace k2h {
namespace {

constexpr int kDedupBlobs = 256;         // gather / compact: blobs per 256-thread block, one per thread
constexpr int kResolveBlock = 256;       // resolve: sorted positions per block, one per thread

// The mtime rule (k2h_amd_ralledata_dedup_mtime) keeps a participant's mtime next to its side
// record, in an array of its own so that the side record and the plain rule's kernels stay what
// they are.  A blob without attrs, or whose attrs give no mtime (GetMTime fails), has none.
struct __attribute__((aligned(16))) Mtime {
  int64_t sec, nsec;
};
struct MtimeRule {
  Mtime* mt;          // n entries; entry i is written only for a blob with kHasMtime
  int64_t sec, nsec;  // pts
};
constexpr uint64_t kHasMtime = 2;  // Side::attrs bit 1, set by the gather of the mtime rule only

// keep[i] = 1 for a participant (resolve clears the superseded ones), by[i] = ~0; the
// participant's stored hash to hash[i] and its side record to side[i]; the tile's count.
// MT: a participant with attrs also has them walked (k2h_ralle_attrs.h) and leaves its mtime.
template <bool MT>
__global__ __launch_bounds__(256) void ralledata_dedup_gather_kernel(
    const uint8_t* __restrict__ blobs, uint64_t size, const uint64_t* __restrict__ off, uint64_t n,
    const uint8_t* __restrict__ consider, uint8_t* __restrict__ keep, uint64_t* __restrict__ by,
    uint64_t* __restrict__ hash, Side* __restrict__ side, uint64_t* __restrict__ tile_count,
    Mtime* __restrict__ mt) {
  typedef hipcub::BlockReduce<uint32_t, kDedupBlobs> Reduce;
  __shared__ typename Reduce::TempStorage tmp;
  const uint64_t i = (uint64_t)blockIdx.x * kDedupBlobs + threadIdx.x;
  uint32_t part = 0;
  if (i < n && (!consider || consider[i])) {
    const uint64_t b = off[i], e = off[i + 1];
    if (e >= b && e <= size && e - b >= (uint64_t)kHdr) {
      uint64_t f[10];
      load_fields(blobs + b, f);
      if (classify(f, e - b) == K2H_AMD_RALLE_OK) {
        part = 1;
        hash[i] = f[0];
        if constexpr (MT) {
          uint64_t attrs = f[5] ? 1ull : 0ull;
          if (f[5]) {
            const AttrTimes t = walk_attrs(blobs + b + f[9], f[5]);
            if (t.flags & kAttrMtime) {
              attrs |= kHasMtime;
              mt[i] = Mtime{t.msec, t.mnsec};
            }
          }
          side[i] = Side{f[1], b + f[6], f[2], attrs};
        } else {
          side[i] = Side{f[1], b + f[6], f[2], f[5] ? 1ull : 0ull};
        }
      }
    }
  }
  if (i < n) {
    keep[i] = (uint8_t)part;
    if (by) by[i] = ~0ull;
  }
  const uint32_t count = Reduce(tmp).Sum(part);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = count;
}

// keys / idx: the pairs, sorted by the hash bits under `mask` (sort_bits_for).  Writes
// keep[i] = 0 for a superseded blob and by[i] for every blob that has a later one of its
// identity; counts the superseded into the counter lines of `dropped`, word 0 (their sum is the
// count).  MT: the mtime rule in place of the attrs rule -- i is superseded by j when i has
// no mtime, or both have one and m_i < m_j and m_i < pts (both strict).
template <bool MT>
__global__ __launch_bounds__(kResolveBlock) void ralledata_dedup_resolve_kernel(
    const uint8_t* __restrict__ blobs, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
    uint64_t n, uint64_t mask, const Side* __restrict__ side, uint8_t* __restrict__ keep,
    uint64_t* __restrict__ by, unsigned long long* __restrict__ dropped, MtimeRule rule) {
  const uint64_t p = (uint64_t)blockIdx.x * kResolveBlock + threadIdx.x;
  bool drop = false;
  if (p + 1 < n) {  // the last position has nothing behind it
    const uint32_t i = idx[p];
    const uint64_t h = keys[p];
    if (i != kNone && !((keys[p + 1] ^ h) & mask) && idx[p + 1] != kNone) {
      const Side a = side[i];
      for (uint64_t q = p + 1; q < n; ++q) {
        const uint64_t hq = keys[q];
        if ((hq ^ h) & mask) break;
        const uint32_t j = idx[q];
        if (j == kNone) break;  // (sorted bits all ones: the non-participants follow the participants)
        if (hq != h) continue;  // another hash with the same sorted bits
        const Side b = side[j];
        if (b.sub != a.sub || b.klen != a.klen || !same_key(blobs + a.koff, blobs + b.koff, a.klen)) continue;
        if (by) by[i] = j;
        if constexpr (MT) {
          if (!(a.attrs & kHasMtime)) {
            drop = true;
          } else if (b.attrs & kHasMtime) {
            const Mtime mi = rule.mt[i], mj = rule.mt[j];
            drop = time_less(mi.sec, mi.nsec, mj.sec, mj.nsec) && time_less(mi.sec, mi.nsec, rule.sec, rule.nsec);
          }
        } else {
          drop = !(a.attrs | b.attrs);
        }
        break;
      }
      if (drop) keep[i] = 0;
    }
  }
  // one atomic per wave, neighbouring waves on different lines: with every wave adding to one
  // word the adds queue up behind each other and set the kernel's time
  const unsigned long long m = __ballot(drop);
  if ((threadIdx.x & 63u) == 0 && m) {
    const uint32_t wave = blockIdx.x * (kResolveBlock / 64) + (threadIdx.x >> 6);
    atomicAdd(dropped + 8 * (wave % kCounterLines), (unsigned long long)__popcll(m));
  }
}

// The call's temporaries (k2h_scratch.h) -- 56 bytes per blob (the stage's two key and two index
// columns, the side records), the tile counts and their scan, the counters, and the library's own
// storage; the mtime rule adds 16 bytes per blob behind them.
PerDevice<> g_dedup;

struct DedupCols {
  SortStage<> st;
  Side* side;
  unsigned long long* counter;
  void* tmp;
  Mtime* mt;  // the mtime rule only, behind everything else: the plain rule's layout stays
  size_t total;
};

// Both entry points; pts == NULL: the attrs rule.
int dedup_stages(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n, const uint8_t* consider,
                 uint8_t* keep, uint64_t* by, uint64_t* dropped, const k2h_amd_timespec* pts, hipStream_t stream,
                 hipError_t* herr) {
  *herr = hipSuccess;
  const uint64_t nt = (n + kDedupBlobs - 1) / kDedupBlobs;
  FirstError tr;
  DeviceScratch* const sc = g_dedup.current(tr);
  SortStage<> st;
  st.measure(tr, n, nt, stream);
  if (!tr.ok()) {
    *herr = tr.e;
    return K2H_AMD_EHIP;
  }
  auto layout = [&](void* base) {
    Carver c(base);
    DedupCols k;
    k.st = st.take(c);
    k.side = c.take<Side>(n);
    k.counter = (unsigned long long*)c.bytes(kCounterBytes);
    k.tmp = c.bytes(st.tmp_bytes());
    k.mt = pts ? c.take<Mtime>(n) : nullptr;
    k.total = c.total();
    return k;
  };
  std::lock_guard<std::mutex> lk(sc->mu);
  if (const int rc = sc->reserve(layout(nullptr).total, stream, herr)) return rc;
  const DedupCols k = layout(sc->p);
  k.st.clear(tr, stream);
  tr(hipMemsetAsync(k.counter, 0, kCounterBytes, stream));
  if (tr.ok()) {
    if (pts)
      ralledata_dedup_gather_kernel<true><<<(unsigned)nt, kDedupBlobs, kWalkLdsBytes, stream>>>(
          (const uint8_t*)blobs, size, blob_off, n, consider, keep, by, k.st.hashes(), k.side, k.st.tile_count, k.mt);
    else
      ralledata_dedup_gather_kernel<false><<<(unsigned)nt, kDedupBlobs, 0, stream>>>(
          (const uint8_t*)blobs, size, blob_off, n, consider, keep, by, k.st.hashes(), k.side, k.st.tile_count, nullptr);
    tr(hipGetLastError());
  }
  k.st.scan_tiles(tr, k.tmp, stream);
  ralle_compact<kDedupBlobs>(tr, k.st, keep, n, 0, stream);
  k.st.sort(tr, k.tmp, stream);
  if (tr.ok()) {
    const uint64_t grid = (n + kResolveBlock - 1) / kResolveBlock;
    const uint64_t mask = k.st.mask();
    if (pts)
      ralledata_dedup_resolve_kernel<true><<<(unsigned)grid, kResolveBlock, 0, stream>>>(
          (const uint8_t*)blobs, k.st.keys_out, k.st.idx_out, n, mask, k.side, keep, by, k.counter,
          MtimeRule{k.mt, pts->sec, pts->nsec});
    else
      ralledata_dedup_resolve_kernel<false><<<(unsigned)grid, kResolveBlock, 0, stream>>>(
          (const uint8_t*)blobs, k.st.keys_out, k.st.idx_out, n, mask, k.side, keep, by, k.counter,
          MtimeRule{nullptr, 0, 0});
    tr(hipGetLastError());
  }
  unsigned long long counts[kCounterBytes / 8];
  if (tr.ok() && dropped) tr(hipMemcpyAsync(counts, k.counter, kCounterBytes, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(sc->mark_done(stream));
  if (tr.ok() && dropped) {
    tr(hipStreamSynchronize(stream));
    if (tr.ok()) *dropped = counter_sum(counts, 0);
  }
  *herr = tr.e;
  return !tr.ok() ? K2H_AMD_EHIP : K2H_AMD_OK;
}

}  // namespace

// Returns a K2H_AMD_* code (the HIP error, if any, in *herr); synchronises the stream once
// when dropped != NULL, else not at all.  1 <= n <= 2^32 - 2.
int launch_ralledata_dedup(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                           const uint8_t* consider, uint8_t* keep, uint64_t* by, uint64_t* dropped, hipStream_t stream,
                           hipError_t* herr) {
  return dedup_stages(blobs, size, blob_off, n, consider, keep, by, dropped, nullptr, stream, herr);
}

// The same with the mtime rule; pts is a host pointer, read before the call returns.
int launch_ralledata_dedup_mtime(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                                 const uint8_t* consider, const k2h_amd_timespec* pts, uint8_t* keep, uint64_t* by,
                                 uint64_t* dropped, hipStream_t stream, hipError_t* herr) {
  return dedup_stages(blobs, size, blob_off, n, consider, keep, by, dropped, pts, stream, herr);
}

}  // namespace k2h
