// k2hash_amd -- log compaction of a k2hash transaction archive in device memory by the rule of
// K2HArchive::Load (include/k2hash_amd.h section 5b: k2h_amd_archive_fold).
//
// Load's switch (lib/k2harchive.cc:328-363) replays SET_ALL through K2HShm::ReplaceAll
// (lib/k2hshm.cc:2948-2950: the value always, subkeys and attrs only when the record's own are
// non-empty), REPLACE_VAL / _SKEY / _ATTRS through K2HShm::Replace (:2973-3036) and ReplacePage
// (:3168-3225), DEL_KEY through Remove(key, false) (:2544-2560, RemoveEx :2789-2820), so every
// record writes a set W of the element's fields {V, S, A}.  A record whose W is covered by the
// union of the W of the later records of its key -- up to the first OW_VAL or RENAME of that key,
// and not across any RENAME of the log -- changes nothing in the table the log leaves.
//
// Stages, all on the caller's stream:
//   gather   one lane per record: participant or not, its W bits and barrier bit, a 32-byte
//            side record (key offset, key length, bits), the first cover summary (nothing
//            behind it), and the tile's packed count: participants in the low half, RENAME
//            participants in the high half.
//   sort     the sort stage of k2h_sort_stage.h over (h1, index), with this file's own compact
//            kernel, which also gives every participant its seg -- the RENAMEs before it -- from
//            the high half of the scanned counts.  Stable, so records of one hash are neighbours
//            in record order.
//   link     one lane per sorted position: forward to the nearest later entry of the same full
//            h1, key length and key bytes -- `by` -- and from it the lane's first summary
//            (U, nxt): U = W(by), nxt = by; or nothing when by is absent, a barrier or in
//            another seg.  h1 is only a grouping key: wrong values make the walks longer, the
//            identity is key length and key bytes.
//   cover    pointer doubling over the summaries: U[i] |= U[nxt[i]], nxt[i] = nxt[nxt[i]],
//            from one buffer into the other, so every pair read is the summary of a whole range
//            of i's chain.  A lane is finished when W(i) is inside U(i) (dropped) or nxt(i) is
//            none (kept); lanes that are finished but still have a nxt go on doubling, because
//            the unfinished ones jump over them.  A round reports whether any lane is still
//            unfinished; the host reads that word and stops.  A plain forward walk instead
//            would chase, for the one SET_ALL(v, s, a) at the head of a key that a million
//            REPLACE_VALs follow, a million dependent scattered loads in one lane.
//   finish   keep[i] = 0 for the covered, and their count.
//
// Synchronisations of the stream per call: one after link, one after each cover round (none
// when link already left no lane unfinished), one more when the count is wanted.  Rounds: a
// lane needs about log2 of the number of records of its key between it and the record that
// completes its cover (or its chain's end): six on the measured 8 Mi-record log with a quarter
// rewrites, 17 for a head before 65,536 REPLACE_VALs; at most 32, since nxt
// always points to a later record.
//
// No byte outside [0, size) is read: a key is compared in 16-byte chunks that END at its last
// byte; chunk 0 of a key that begins fewer bytes into the file than its chunk leads it is put
// together from the key's own bytes (hand-made recs may have key_off < 16).  Nothing of a
// record is read but its key, and nothing of a record that does not take part.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <mutex>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_sort_stage.h"

// Dynamic LDS, never touched, that a build can give to the link and cover kernels so that fewer
// blocks fit a CU: 64 KiB leaves two 256-thread blocks per CU, two waves per SIMD; 0 leaves
// eight.  Both kernels were measured both ways: unlike the attrs walk of 5.4f
// they are faster at eight, link by a tenth of the call and cover by a twelfth, so 0 is built.
#ifndef K2H_FOLD_LINK_LDS
#define K2H_FOLD_LINK_LDS 0
#endif
#ifndef K2H_FOLD_COVER_LDS
#define K2H_FOLD_COVER_LDS 0
#endif

namespace k2h {
namespace {

constexpr int kFoldRecs = 256;           // every kernel: records (or sorted positions) per block, one per thread
constexpr uint32_t kNone = 0xFFFFFFFFu;  // no record: a pair's index, a summary's nxt
constexpr int kMaxRounds = 32;           // nxt points to a later record, n < 2^32: a chain has fewer than 2^32 links
constexpr size_t kLinkLds = K2H_FOLD_LINK_LDS, kCoverLds = K2H_FOLD_COVER_LDS;

// A participant's bits.
constexpr uint32_t kV = 1, kS = 2, kA = 4;  // W: the fields the record writes
constexpr uint32_t kBarrier = 8;            // OW_VAL, RENAME: always kept, ends the chains that reach it
constexpr uint32_t kRename = 16;            // RENAME: a new seg starts behind it

// What link needs of a participant; 32 bytes, so one aligned sector per record.
struct __attribute__((aligned(16))) Side {
  uint64_t koff;  // the key's first byte, from `file`
  uint64_t klen;  // >= 1, the key lies inside the file
  uint32_t bits;  // kV .. kRename
  uint32_t seg;   // RENAME participants before this record
  uint64_t pad;
};
static_assert(sizeof(Side) == 32, "two 16-byte loads");

// A cover summary in one word, so that a load gives a consistent (U, nxt): nxt in bits 0-31, U
// in bits 32-34, the lane's own W in bits 35-37.  A record that can never be dropped (a
// barrier, a non-participant) carries W = 7 and never gets a nxt.
constexpr int kUShift = 32, kWShift = 35;
__host__ __device__ constexpr uint64_t summary(uint32_t w, uint32_t u, uint32_t nxt) {
  return (uint64_t)nxt | (uint64_t)u << kUShift | (uint64_t)w << kWShift;
}
__device__ __forceinline__ uint32_t nxt_of(uint64_t s) { return (uint32_t)s; }
__device__ __forceinline__ bool covered(uint64_t s) { return (((s >> kWShift) & ~(s >> kUShift)) & 7u) == 0; }
__device__ __forceinline__ bool unfinished(uint64_t s) { return nxt_of(s) != kNone && !covered(s); }

// SET_ALL: V always, S and A when the record's own are non-empty (lib/k2hshm.cc:2948-2950);
// REPLACE_VAL / _SKEY / _ATTRS: the one field; DEL_KEY: all three; OW_VAL and RENAME: barriers.
__device__ __forceinline__ uint32_t bits_of(int64_t type, uint64_t slen, uint64_t alen) {
  switch (type) {
    case 0: return kV | (slen ? kS : 0u) | (alen ? kA : 0u);
    case 1: return kV;
    case 2: return kS;
    case 3: return kV | kS | kA;
    case 4: return kBarrier;
    case 5: return kA;
    default: return kBarrier | kRename;  // 6
  }
}

// keep[i] = 1 for a participant (finish clears the dropped ones), by[i] = ~0, the first summary
// and, for a participant, the side record; the tile's participants (low half) and RENAME
// participants (high half).
__global__ __launch_bounds__(kFoldRecs) void archive_fold_gather_kernel(
    const k2h_amd_archive_rec* __restrict__ recs, uint64_t size, uint64_t n, uint8_t* __restrict__ keep,
    uint64_t* __restrict__ by, Side* __restrict__ side, uint64_t* __restrict__ sum0,
    uint64_t* __restrict__ tile_count) {
  typedef hipcub::BlockReduce<uint64_t, kFoldRecs> Reduce;
  __shared__ typename Reduce::TempStorage tmp;
  const uint64_t i = (uint64_t)blockIdx.x * kFoldRecs + threadIdx.x;
  uint64_t cnt = 0;
  if (i < n) {
    const k2h_amd_archive_rec& r = recs[i];
    const int64_t type = r.type;
    const uint64_t koff = r.key_off, klen = r.key_len;
    uint32_t w = 7;
    if (r.status == 0 && type >= 0 && type <= 6 && klen >= 1 && koff <= size && klen <= size - koff) {
      const uint32_t bits = bits_of(type, r.skey_len, r.attrs_len);
      side[i] = Side{koff, klen, bits, 0u, 0ull};
      cnt = 1ull | (uint64_t)((bits & kRename) != 0) << 32;
      if (!(bits & kBarrier)) w = bits & 7u;
    }
    keep[i] = (uint8_t)(cnt & 1u);
    if (by) by[i] = ~0ull;
    sum0[i] = summary(w, 0u, kNone);
  }
  const uint64_t total = Reduce(tmp).Sum(cnt);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// The sort's input, n pairs: participant i at its rank among the participants, every other
// record behind all m of them (tile_base = the scanned tile counts, entry ntiles = the
// totals); and every participant's seg.
__global__ __launch_bounds__(kFoldRecs) void archive_fold_compact_kernel(
    const uint8_t* __restrict__ keep, const uint64_t* __restrict__ hash, uint64_t n,
    const uint64_t* __restrict__ tile_base, uint64_t ntiles, Side* __restrict__ side, uint64_t* __restrict__ keys,
    uint32_t* __restrict__ idx) {
  typedef hipcub::BlockScan<uint64_t, kFoldRecs> Scan;
  __shared__ typename Scan::TempStorage tmp;
  const uint64_t i = (uint64_t)blockIdx.x * kFoldRecs + threadIdx.x;
  const bool part = i < n && keep[i];
  const uint64_t cnt = part ? 1ull | (uint64_t)((side[i].bits & kRename) != 0) << 32 : 0ull;
  uint64_t rank;
  Scan(tmp).ExclusiveSum(cnt, rank);
  if (i >= n) return;
  const uint64_t at = tile_base[blockIdx.x] + rank;  // (neither half carries: both counts are below 2^32)
  const uint64_t before = at & 0xFFFFFFFFull;        // participants before record i
  if (part) side[i].seg = (uint32_t)(at >> 32);
  const uint64_t pos = part ? before : (tile_base[ntiles] & 0xFFFFFFFFull) + (i - before);
  keys[pos] = part ? hash[i] : ~0ull;
  idx[pos] = part ? (uint32_t)i : kNone;
}

__device__ __forceinline__ bool differ(uint4 x, uint4 y) {
  return ((x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w)) != 0;
}

// Chunk 0 of the key at file offset a whose chunks end at its last byte: the 16 bytes from
// a - lead with the lead bytes zeroed; only the key's own bytes where that would begin below
// the file.
__device__ __forceinline__ uint4 chunk0(const uint8_t* f, uint64_t a, uint32_t lead) {
  if (a >= lead) return mask_lead(ld16(f + (a - lead)), lead);
  return chunk0_from_bytes(lead, [=](uint32_t j) { return (uint32_t)f[a + j]; });
}

// Two keys of the same length kl >= 1 at file offsets a and b, as ceil(kl / 16) chunks that
// end at each key's last byte.
__device__ __forceinline__ bool same_key(const uint8_t* f, uint64_t a, uint64_t b, uint64_t kl) {
  const uint64_t k = (kl + 15) >> 4;
  const uint32_t lead = (uint32_t)(16 * k - kl);
  if (differ(chunk0(f, a, lead), chunk0(f, b, lead))) return false;
  for (uint64_t q = 1; q < k; ++q)  // (a - lead may wrap; a - lead + 16 q >= a does not)
    if (differ(ld16(f + (a - lead + 16 * q)), ld16(f + (b - lead + 16 * q)))) return false;
  return true;
}

// keys / idx: the pairs, sorted by the hash bits under `mask`.  Writes by[i] and the first
// summary of every participant that has a later one of its identity, and *flag = 1 when some
// lane is left unfinished.
__global__ __launch_bounds__(kFoldRecs) void archive_fold_link_kernel(
    const uint8_t* __restrict__ file, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, uint64_t n,
    uint64_t mask, const Side* __restrict__ side, uint64_t* __restrict__ by, uint64_t* __restrict__ sum0,
    uint32_t* __restrict__ flag) {
  const uint64_t p = (uint64_t)blockIdx.x * kFoldRecs + threadIdx.x;
  bool open = false;
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
        if (b.klen != a.klen || !same_key(file, a.koff, b.koff, a.klen)) continue;
        if (by) by[i] = j;
        if (!((a.bits | b.bits) & kBarrier) && a.seg == b.seg) {
          const uint64_t s = summary(a.bits & 7u, b.bits & 7u, j);
          sum0[i] = s;
          open = unfinished(s);
        }
        break;
      }
    }
  }
  if (__ballot(open) && (threadIdx.x & 63u) == 0) *flag = 1u;
}

// One round of pointer doubling, `in` to `out`.
__global__ __launch_bounds__(kFoldRecs) void archive_fold_cover_kernel(const uint64_t* __restrict__ in,
                                                                      uint64_t* __restrict__ out, uint64_t n,
                                                                      uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * kFoldRecs + threadIdx.x;
  bool open = false;
  if (i < n) {
    uint64_t s = in[i];
    const uint32_t nx = nxt_of(s);
    if (nx != kNone) {
      const uint64_t t = in[nx];
      s = (s & ~0xFFFFFFFFull) | (t & (7ull << kUShift)) | nxt_of(t);
      open = unfinished(s);
    }
    out[i] = s;
  }
  if (__ballot(open) && (threadIdx.x & 63u) == 0) *flag = 1u;
}

// keep[i] = 0 for the covered records; their number into word 0 of the counter lines of `dropped`.
__global__ __launch_bounds__(kFoldRecs) void archive_fold_finish_kernel(const uint64_t* __restrict__ sum, uint64_t n,
                                                                       uint8_t* __restrict__ keep,
                                                                       unsigned long long* __restrict__ dropped) {
  const uint64_t i = (uint64_t)blockIdx.x * kFoldRecs + threadIdx.x;
  const bool drop = i < n && covered(sum[i]);
  if (drop) keep[i] = 0;
  // one atomic per wave, neighbouring waves on different lines (k2h_ralledata_dedup.hip)
  const unsigned long long m = __ballot(drop);
  if ((threadIdx.x & 63u) == 0 && m) {
    const uint32_t wave = blockIdx.x * (kFoldRecs / 64) + (threadIdx.x >> 6);
    atomicAdd(dropped + 8 * (wave % kCounterLines), (unsigned long long)__popcll(m));
  }
}

// The call's temporaries (k2h_scratch.h) -- 72 bytes per record (two key and two index columns,
// the side records, two summary columns), the tile counts and their scan, the round flags, the
// counters, and the library's own storage.
PerDevice<> g_fold;

constexpr size_t kFlagBytes = 256;  // kMaxRounds + 1 words

struct FoldCols {
  SortStage<> st;  // hashes(): the records' own hashes when h1 == NULL
  uint64_t *sum_a, *sum_b;
  Side* side;
  uint32_t* flags;
  unsigned long long* counter;  // right behind the flags: one memset clears both
  void* tmp;
  size_t total;
};

}  // namespace

// Returns a K2H_AMD_* code (the HIP error, if any, in *herr).  1 <= n <= 2^32 - 2.
int launch_archive_fold(const void* file, uint64_t size, const k2h_amd_archive_rec* recs, uint64_t n,
                        const uint64_t* h1, uint64_t seed, uint8_t* keep, uint64_t* by, uint64_t* dropped,
                        hipStream_t stream, hipError_t* herr) {
  *herr = hipSuccess;
  const uint64_t nt = (n + kFoldRecs - 1) / kFoldRecs;
  FirstError tr;
  DeviceScratch* const sc = g_fold.current(tr);
  SortStage<> st;
  st.measure(tr, n, nt, stream);
  if (!tr.ok()) {
    *herr = tr.e;
    return K2H_AMD_EHIP;
  }
  auto layout = [&](void* base) {
    Carver c(base);
    FoldCols k;
    k.st = st.take(c);
    k.sum_a = c.take<uint64_t>(n);
    k.sum_b = c.take<uint64_t>(n);
    k.side = c.take<Side>(n);
    k.flags = (uint32_t*)c.bytes(kFlagBytes);
    k.counter = (unsigned long long*)c.bytes(kCounterBytes);
    k.tmp = c.bytes(st.tmp_bytes());
    k.total = c.total();
    return k;
  };
  std::lock_guard<std::mutex> lk(sc->mu);
  if (const int rc = sc->reserve(layout(nullptr).total, stream, herr)) return rc;
  const FoldCols k = layout(sc->p);
  const unsigned grid = (unsigned)nt;
  k.st.clear(tr, stream);
  tr(hipMemsetAsync(k.flags, 0, kFlagBytes + kCounterBytes, stream));
  if (tr.ok() && !h1) {
    ArchiveHashOut ho;
    ho.h1 = k.st.hashes();
    tr(launch_archive_prehash(file, size, recs, n, seed, ho, stream));
  }
  if (tr.ok()) {
    archive_fold_gather_kernel<<<grid, kFoldRecs, 0, stream>>>(recs, size, n, keep, by, k.side, k.sum_a, k.st.tile_count);
    tr(hipGetLastError());
  }
  k.st.scan_tiles(tr, k.tmp, stream);
  if (tr.ok()) {
    archive_fold_compact_kernel<<<grid, kFoldRecs, 0, stream>>>(keep, h1 ? h1 : k.st.hashes(), n, k.st.tile_base, nt,
                                                               k.side, k.st.keys_in, k.st.idx_in);
    tr(hipGetLastError());
  }
  k.st.sort(tr, k.tmp, stream);
  if (tr.ok()) {
    archive_fold_link_kernel<<<grid, kFoldRecs, kLinkLds, stream>>>((const uint8_t*)file, k.st.keys_out, k.st.idx_out, n,
                                                                    k.st.mask(), k.side, by, k.sum_a, k.flags);
    tr(hipGetLastError());
  }
  // the rounds: flags[r] says whether the kernel before round r left a lane unfinished
  uint64_t *cur = k.sum_a, *other = k.sum_b;
  for (int r = 0; tr.ok(); ++r) {
    uint32_t open = 0;
    tr(hipMemcpyAsync(&open, k.flags + r, 4, hipMemcpyDeviceToHost, stream));
    tr(hipStreamSynchronize(stream));
    if (!tr.ok() || !open) break;
    if (r == kMaxRounds) {  // (cannot happen: every nxt is a later record)
      tr.e = hipErrorUnknown;
      break;
    }
    archive_fold_cover_kernel<<<grid, kFoldRecs, kCoverLds, stream>>>(cur, other, n, k.flags + r + 1);
    tr(hipGetLastError());
    uint64_t* t = cur;
    cur = other;
    other = t;
  }
  if (tr.ok()) {
    archive_fold_finish_kernel<<<grid, kFoldRecs, 0, stream>>>(cur, n, keep, k.counter);
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

}  // namespace k2h
