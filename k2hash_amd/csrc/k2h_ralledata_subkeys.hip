// k2hash_amd -- RALLEDATA consumer side: the subkeys of a blob stream in device memory as edges
// between its blobs, and what a set of root blobs reaches over them
// (include/k2hash_amd.h section 4b'''''').
//
// k2h_amd_ralledata_subkeys.  A blob's subkeys segment is a serialized K2HSubKeys list
// (k2h_ralle_subkeys.h: the strict walk).  Every name in it is an edge from the blob to the
// element the table would find under that name: K2HShm::Remove(key, true) and RemoveSubkeys
// (lib/k2hshm.cc:2544-2560, :2866-2898) hash the name with K2H_HASH_FUNC / K2H_2ND_HASH_FUNC
// and look the element up by hash, subhash and key bytes.  So an edge carries the name's
// COMPUTED hashes, its length and its bytes, a blob its STORED hash, stored subhash, key_length
// and key bytes, and the two are joined as k2h_ralledata_diff.hip joins two streams: a blob
// whose stored hashes are wrong is not found by name, as in the table.  All on the caller's
// stream:
//   count    one lane per blob: span, header and classify (k2h_ralle_header.h, the participants
//            of _dedup), then the walk of a participant's segment: a flag byte and the number
//            of edges.  An exclusive scan gives edge_off[n + 1]; E = edge_off[n] and three
//            counters come back to the host (first synchronisation).  The walk is a per-lane
//            chain of dependent loads like the attrs walk's, and starts from that walk's launch
//            shape (kWalkLdsBytes, two waves per SIMD).
//   emit     one lane per blob again: a participant leaves its stored hash and side record
//            (k2h_ralle_ident.h) and its tile's count, a blob with edges walks its segment
//            once more and leaves, per edge, the name's absolute 64-bit position and length.
//   hash     one lane per edge: the name's two hashes over the end-aligned chunks of
//            k2h_endwalk.h, as k2h_hash / k2h_second_hash compute them on the raw name bytes
//            (no NUL is added: the name carries whatever NUL it was stored with); the lane
//            lays the pair (hash, n + e) out for the sort behind the m participating blobs.
//   sort     blobs at [0, n) and edges at [n, n + E) in one index space, through the sort stage
//            of k2h_sort_stage.h (tiles of the n blobs, n + E pairs); stable, so within a run of
//            equal sorted bits the blobs come first, in stream order, then the edges.
//   resolve  two mark kernels and two inclusive max-scans give every sorted position the
//            nearest blob entry at or before it, and (scanned over the mirrored positions) the
//            first position behind it that is no blob entry or starts another run.  One lane
//            per sorted entry walks BACKWARD from the last blob entry of its run to the first
//            one of its identity (last_held): for an edge that is child[e], for a blob rep[i].
//
// Cost of the resolve: r copies of one key cost O(1) steps per lane, r DISTINCT identities that
// share all sorted bits O(r) per lane among them -- the crafted-stream case of
// k2h_ralledata_dedup.hip.  Cost of the walk: one lane per segment, so a blob with a very long
// list holds its wave for the length of that list (DESIGN.md 5.4i has what it costs).
//
// k2h_amd_ralledata_reach.  A level-synchronous frontier traversal over child, from the start
// set {rep[i] : roots[i] != 0, rep[i] != ~0}.  Only blobs that are their own rep are ever in a
// frontier: earlier copies of a key are not in the table and their lists do not exist.  A blob
// enters a frontier once (an atomic OR on a bitmap decides), so the work is O(n + E) in all; a
// frontier blob with more than kReachWaveEdges edges has them followed by its whole wave.  One
// 8-byte read-back through pinned memory per level says how large the next frontier is.  A
// chain-shaped stream costs one level, one kernel and one synchronisation per link: the crafted
// case, which max_levels bounds.
//
// Reads.  No byte of `blobs` outside [0, size): every load of the walk lies wholly inside the
// segment, which classify keeps inside the blob; a name is hashed and compared in 16-byte
// chunks that END at its last byte, and it starts at least 96 bytes into its blob, so chunk 0
// never begins below the buffer and its lead bytes are masked off.  Nothing of a
// non-participant beyond its header, nothing of a blob whose span is bad or whose consider byte
// is 0, and nothing outside a blob's own subkeys segment is ever interpreted.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <mutex>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_ralle_header.h"
#include "k2h_ralle_ident.h"
#include "k2h_ralle_subkeys.h"

namespace k2h {
namespace {

constexpr int kSkBlobs = 256;         // count / emit: blobs per 256-thread block, one per thread
constexpr int kSkBlock = 256;         // every other kernel: items per block, one per thread
constexpr int kReachWaveEdges = 32;   // a frontier blob with more edges than this is followed by its wave
constexpr size_t kSkPinnedBytes = kCounterBytes + 64;  // the counters, then one word

struct SkStream {
  const uint8_t* blobs;
  uint64_t size;
  const uint64_t* off;
  const uint8_t* consider;
};

// Blob i takes part: its first byte to o and its header fields to f.
__device__ __forceinline__ bool sk_participant(const SkStream& s, uint64_t i, uint64_t& o, uint64_t (&f)[10]) {
  if (s.consider && !s.consider[i]) return false;
  o = s.off[i];
  const uint64_t e = s.off[i + 1];
  if (!(e >= o && e <= s.size && e - o >= (uint64_t)kHdr)) return false;
  load_fields(s.blobs + o, f);
  return classify(f, e - o) == K2H_AMD_RALLE_OK;
}

// One add per wave and word, neighbouring waves on different lines (as the dedup's resolve counts).
__device__ __forceinline__ void sk_count(unsigned long long* counter, int word, bool x) {
  const unsigned long long m = __ballot(x);
  if ((threadIdx.x & 63u) == 0 && m) {
    const uint32_t wave = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    atomicAdd(counter + 8 * (wave % kCounterLines) + word, (unsigned long long)__popcll(m));
  }
}

// sk_flags[i] and cnt[i], the number of blob i's edges; counts {participants, blobs with an
// edge, BAD segments} into the counter lines.
__global__ __launch_bounds__(kSkBlobs) void subkeys_count_kernel(SkStream s, uint64_t n, uint8_t* __restrict__ sk_flags,
                                                                 uint64_t* __restrict__ cnt,
                                                                 unsigned long long* __restrict__ counter) {
  const uint64_t i = (uint64_t)blockIdx.x * kSkBlobs + threadIdx.x;
  uint32_t fl = 0;
  uint64_t edges = 0;
  if (i < n) {
    uint64_t o, f[10];
    if (sk_participant(s, i, o, f)) {
      fl = K2H_AMD_SKEY_PART;
      if (f[4]) {
        fl |= K2H_AMD_SKEY_HAS;
        if (!walk_subkeys(s.blobs + o + f[8], f[4], edges, [](uint64_t, uint64_t, uint64_t) {})) {
          fl |= K2H_AMD_SKEY_BAD;
          edges = 0;
        }
      }
    }
    sk_flags[i] = (uint8_t)fl;
    cnt[i] = edges;
  }
  sk_count(counter, 0, fl != 0);
  sk_count(counter, 1, edges != 0);
  sk_count(counter, 2, (fl & K2H_AMD_SKEY_BAD) != 0);
}

// part[i] = 1 for a participant, its stored hash to hash[i], its side record to side[i]; the
// tile's count; rep[i] = ~0 for every other blob.  A blob with edges walks its segment again
// and leaves the name of edge e = edge_off[i] + k in side[n + e] (position from `blobs`, length,
// and the blob it belongs to; the hash kernel adds the second hash).
__global__ __launch_bounds__(kSkBlobs) void subkeys_emit_kernel(SkStream s, uint64_t n,
                                                                const uint64_t* __restrict__ edge_off, uint64_t E,
                                                                uint8_t* __restrict__ part,
                                                                uint64_t* __restrict__ hash, Side* __restrict__ side,
                                                                uint64_t* __restrict__ tile_count,
                                                                uint64_t* __restrict__ rep) {
  typedef hipcub::BlockReduce<uint32_t, kSkBlobs> Reduce;
  __shared__ typename Reduce::TempStorage tmp;
  const uint64_t i = (uint64_t)blockIdx.x * kSkBlobs + threadIdx.x;
  uint32_t p = 0;
  if (i < n) {
    uint64_t o, f[10];
    if (sk_participant(s, i, o, f)) {
      p = 1;
      hash[i] = f[0];
      side[i] = Side{f[1], o + f[6], f[2], 0};
      const uint64_t e0 = edge_off[i], e1 = edge_off[i + 1];
      if (f[4] && e1 > e0) {  // (a BAD segment has no edges)
        const uint64_t base = o + f[8];
        Side* const edge = side + n;
        uint64_t edges;
        walk_subkeys(s.blobs + base, f[4], edges, [=](uint64_t k, uint64_t pos, uint64_t len) {
          const uint64_t e = e0 + k;
          if (e < e1 && e < E) edge[e] = Side{0, base + pos, len, i};
        });
      }
    }
    part[i] = (uint8_t)p;
    if (rep && !p) rep[i] = ~0ull;
  }
  const uint32_t count = Reduce(tmp).Sum(p);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = count;
}

// One lane per edge: the name's hashes; the pair (hash, n + e) to place m + e of the sort's
// input, m = tile_base[ntiles] the participating blobs' number.
__global__ __launch_bounds__(kSkBlock) void subkeys_hash_kernel(const uint8_t* __restrict__ blobs, uint64_t n, uint64_t E,
                                                                Side* __restrict__ side,
                                                                const uint64_t* __restrict__ tile_base, uint64_t ntiles,
                                                                uint64_t* __restrict__ keys, uint32_t* __restrict__ idx,
                                                                SpadTable spad_tab) {
  __shared__ uint64_t spad[16];
  if (threadIdx.x < 16) spad[threadIdx.x] = spad_tab.v[threadIdx.x];
  __syncthreads();
  const uint64_t e = (uint64_t)blockIdx.x * kSkBlock + threadIdx.x;
  if (e >= E) return;
  const Side sd = side[n + e];
  const uint64_t len = sd.klen, k = (len + 15) >> 4;  // len >= 1
  uint64_t h1, h2;
  end_aligned_walk_ptr<true, false>(k, (uint32_t)(16 * k - len), blobs + sd.koff + len - 16 * k, blobs, spad, h1, h2);
  if (len == 1) h2 = h1;  // lib/k2hashfunc.cc:83
  side[n + e].sub = h2;
  const uint64_t at = tile_base[ntiles] + e;
  keys[at] = h1;
  idx[at] = (uint32_t)(n + e);
}

// The second mark, over the mirrored positions u = N - 1 - p: u + 1 where the entry at p is no
// blob entry or is the first of its run of equal sorted bits, else 0.  Its inclusive max-scan
// S gives a blob entry at p the first such position behind it: N - S[N - 2 - p] (N when that is
// 0 or p is the last position), which is 1 + the position of the last blob entry of p's run.
__global__ __launch_bounds__(kSkBlock) void subkeys_bound_kernel(const uint64_t* __restrict__ keys,
                                                                 const uint32_t* __restrict__ idx, uint64_t N, uint64_t n,
                                                                 uint64_t mask, uint32_t* __restrict__ mark_r) {
  const uint64_t p = (uint64_t)blockIdx.x * kSkBlock + threadIdx.x;
  if (p >= N) return;
  const bool bound = idx[p] >= n || (p > 0 && ((keys[p] ^ keys[p - 1]) & mask));
  const uint64_t u = N - 1 - p;
  mark_r[u] = bound ? (uint32_t)(u + 1) : 0u;
}

// keys / idx: the N pairs, sorted by the hash bits under `mask`.  child[e] for every edge,
// rep[i] for every participating blob (rep may be NULL); counts the dangling edges.
__global__ __launch_bounds__(kSkBlock) void subkeys_resolve_kernel(
    const uint8_t* __restrict__ blobs, uint64_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
    uint64_t N, uint64_t mask, const uint32_t* __restrict__ last_b, const uint32_t* __restrict__ bound_s,
    const Side* __restrict__ side, uint64_t* __restrict__ rep, uint64_t* __restrict__ child,
    unsigned long long* __restrict__ counter) {
  const uint64_t p = (uint64_t)blockIdx.x * kSkBlock + threadIdx.x;
  bool dangling = false;
  if (p < N) {
    const uint32_t g = idx[p];
    if (g != kNone && (g >= n || rep)) {
      const Side sa = side[g];
      uint64_t q0;
      if (g >= n) {
        q0 = last_b[p];
      } else {
        const uint32_t sc = p + 1 < N ? bound_s[N - 2 - p] : 0u;
        q0 = sc ? N - sc : N;
      }
      const uint32_t j = last_held(keys, idx, side, q0, keys[p], mask, n, sa, blobs, blobs);
      if (g >= n) {
        child[g - n] = j == kNone ? ~0ull : (uint64_t)j;
        dangling = j == kNone;
      } else {
        rep[g] = j == kNone ? (uint64_t)g : (uint64_t)j;  // (never kNone: the walk meets g itself)
      }
    }
  }
  sk_count(counter, 3, dangling);
}

// ------------------------------------------------------------------------------------ reach
// Blob c enters the next frontier unless it has been in one; c >= n (~0, a dangling name) is no blob.
__device__ __forceinline__ void reach_visit(uint64_t c, uint64_t n, uint32_t* __restrict__ bits,
                                            uint32_t* __restrict__ next, unsigned long long* __restrict__ next_count) {
  if (c >= n) return;
  const uint32_t bit = 1u << (c & 31u);
  if (!(atomicOr(bits + (c >> 5), bit) & bit)) next[atomicAdd(next_count, 1ull)] = (uint32_t)c;
}

__global__ __launch_bounds__(kSkBlock) void reach_start_kernel(const uint64_t* __restrict__ rep,
                                                               const uint8_t* __restrict__ roots, uint64_t n,
                                                               uint32_t* __restrict__ bits, uint32_t* __restrict__ next,
                                                               unsigned long long* __restrict__ next_count) {
  const uint64_t i = (uint64_t)blockIdx.x * kSkBlock + threadIdx.x;
  if (i < n && roots[i]) reach_visit(rep[i], n, bits, next, next_count);
}

// One lane per blob of the frontier: its edges' children; more than kReachWaveEdges of them
// are taken 64 at a time by the whole wave.
__global__ __launch_bounds__(kSkBlock) void reach_level_kernel(const uint32_t* __restrict__ cur, uint64_t fc,
                                                               const uint64_t* __restrict__ edge_off,
                                                               const uint64_t* __restrict__ child, uint64_t n,
                                                               uint32_t* __restrict__ bits, uint32_t* __restrict__ next,
                                                               unsigned long long* __restrict__ next_count) {
  const uint64_t t = (uint64_t)blockIdx.x * kSkBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t lo = 0, hi = 0;
  if (t < fc) {
    const uint32_t b = cur[t];
    lo = edge_off[b];
    hi = edge_off[b + 1];
    if (hi < lo) hi = lo;
  }
  const bool wide = hi - lo > (uint64_t)kReachWaveEdges;
  if (!wide)
    for (uint64_t e = lo; e < hi; ++e) reach_visit(child[e], n, bits, next, next_count);
  for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1) {
    const int src = __ffsll((long long)todo) - 1;
    const uint64_t l = ralle_shfl_u64(lo, src), h = ralle_shfl_u64(hi, src);
    for (uint64_t e = l + lane; e < h; e += 64) reach_visit(child[e], n, bits, next, next_count);
  }
}

// reach[i] = blob i has a rep and the rep was in a frontier; counts them.
__global__ __launch_bounds__(kSkBlock) void reach_final_kernel(const uint64_t* __restrict__ rep, uint64_t n,
                                                               const uint32_t* __restrict__ bits,
                                                               uint8_t* __restrict__ reach,
                                                               unsigned long long* __restrict__ counter) {
  const uint64_t i = (uint64_t)blockIdx.x * kSkBlock + threadIdx.x;
  bool r = false;
  if (i < n) {
    const uint64_t c = rep[i];
    r = c < n && ((bits[c >> 5] >> (c & 31u)) & 1u);
    reach[i] = r ? 1 : 0;
  }
  sk_count(counter, 0, r);
}

// Both calls' temporaries (k2h_scratch.h) and the pinned words their read-backs land in.
struct SkScratch : DeviceScratch {
  void* pinned = nullptr;
};
PerDevice<SkScratch> g_sk;

struct CountCols {  // the count pass: a column of n + 1 counts, the counters, the scan's storage
  uint64_t* cnt;
  unsigned long long* counter;
  void* tmp;
  size_t total;
};
struct JoinCols {  // the join, over N = n + E entries
  SortStage<> st;
  uint32_t* bound_s;
  Side* side;
  uint8_t* part;
  unsigned long long* counter;
  void* tmp;
  size_t total;
};
struct ReachCols {
  uint32_t *bits, *cur, *next;
  unsigned long long* counter;  // the counter lines, then the frontier's size, one word per parity of the level
  size_t total;
};

}  // namespace

// Returns a K2H_AMD_* code (the HIP error, if any, in *herr).  1 <= n <= 2^32 - 2.  Synchronises
// the stream once after the count pass and, when child != NULL, once more at the end.
// K2H_AMD_EINVAL with *why = 1: child != NULL and cap < E; *why = 2: n + E > 2^32 - 2; in both
// counts and edge_off are filled, counts[3] = E, and child is not written.
int launch_ralledata_subkeys(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                             const uint8_t* consider, uint64_t seed, uint8_t* sk_flags, uint64_t* edge_off,
                             uint64_t* rep, uint64_t* child, uint64_t cap, uint64_t* counts, int* why,
                             hipStream_t stream, hipError_t* herr) {
  *herr = hipSuccess;
  *why = 0;
  const uint64_t nt = (n + kSkBlobs - 1) / kSkBlobs;
  FirstError tr;
  auto done = [&]() {
    *herr = tr.e;
    return !tr.ok() ? K2H_AMD_EHIP : K2H_AMD_OK;
  };
  SkScratch* const scp = g_sk.current(tr);
  size_t scan_bytes = 0;
  tr(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, n + 1, stream));
  if (!tr.ok()) return done();
  SkScratch& sc = *scp;
  std::lock_guard<std::mutex> lk(sc.mu);
  if (!sc.pinned) tr(hipHostMalloc(&sc.pinned, kSkPinnedBytes, hipHostMallocDefault));
  if (!tr.ok()) return done();
  unsigned long long* const host = (unsigned long long*)sc.pinned;
  unsigned long long* const host_word = host + kCounterBytes / 8;
  const SkStream s{(const uint8_t*)blobs, size, blob_off, consider};

  {
    auto layout = [&](void* base) {
      Carver c(base);
      CountCols k;
      k.cnt = c.take<uint64_t>(n + 1);
      k.counter = (unsigned long long*)c.bytes(kCounterBytes);
      k.tmp = c.bytes(scan_bytes);
      k.total = c.total();
      return k;
    };
    if (const int rc = sc.reserve(layout(nullptr).total, stream, herr)) return rc;
    const CountCols k = layout(sc.p);
    tr(hipMemsetAsync(k.cnt + n, 0, 8, stream));
    tr(hipMemsetAsync(k.counter, 0, kCounterBytes, stream));
    if (tr.ok()) {
      subkeys_count_kernel<<<(unsigned)nt, kSkBlobs, kWalkLdsBytes, stream>>>(s, n, sk_flags, k.cnt, k.counter);
      tr(hipGetLastError());
    }
    if (tr.ok()) tr(hipcub::DeviceScan::ExclusiveSum(k.tmp, scan_bytes, k.cnt, edge_off, n + 1, stream));
    if (tr.ok()) tr(hipMemcpyAsync(host, k.counter, kCounterBytes, hipMemcpyDeviceToHost, stream));
    if (tr.ok()) tr(hipMemcpyAsync(host_word, edge_off + n, 8, hipMemcpyDeviceToHost, stream));
    if (tr.ok()) tr(sc.mark_done(stream));
    if (tr.ok()) tr(hipStreamSynchronize(stream));
    if (!tr.ok()) return done();
  }
  const uint64_t E = *host_word;
  counts[0] = counter_sum(host, 0);
  counts[1] = counter_sum(host, 1);
  counts[2] = counter_sum(host, 2);
  counts[3] = E;
  counts[4] = 0;
  if (!child) return done();
  if (cap < E) {
    *why = 1;
    return K2H_AMD_EINVAL;
  }
  if (E > 0xFFFFFFFEull || n + E > 0xFFFFFFFEull) {
    *why = 2;
    return K2H_AMD_EINVAL;
  }

  // the join, over N = n + E entries
  const uint64_t N = n + E;
  SortStage<> st;
  st.measure(tr, N, nt, stream);
  st.measure_max_scan(tr, stream);
  if (!tr.ok()) return done();
  auto layout = [&](void* base) {
    Carver c(base);
    JoinCols k;
    k.st = st.take(c);
    k.bound_s = c.take<uint32_t>(N);
    k.side = c.take<Side>(N);
    k.part = c.take<uint8_t>(n);
    k.counter = (unsigned long long*)c.bytes(kCounterBytes);
    k.tmp = c.bytes(st.tmp_bytes());
    k.total = c.total();
    return k;
  };
  if (const int rc = sc.reserve(layout(nullptr).total, stream, herr)) return rc;
  const JoinCols k = layout(sc.p);
  // the first mark column's scan and the second mark column stand in the stage's input columns
  uint32_t* const last_b = k.st.scanned();
  uint32_t* const mark_r = k.st.second();

  k.st.clear(tr, stream);
  tr(hipMemsetAsync(k.counter, 0, kCounterBytes, stream));
  if (tr.ok()) {
    subkeys_emit_kernel<<<(unsigned)nt, kSkBlobs, kWalkLdsBytes, stream>>>(s, n, edge_off, E, k.part, k.st.hashes(),
                                                                           k.side, k.st.tile_count, rep);
    tr(hipGetLastError());
  }
  k.st.scan_tiles(tr, k.tmp, stream);
  ralle_compact<kSkBlobs>(tr, k.st, k.part, n, E, stream);
  if (tr.ok() && E) {
    subkeys_hash_kernel<<<(unsigned)((E + kSkBlock - 1) / kSkBlock), kSkBlock, 0, stream>>>(
        s.blobs, n, E, k.side, k.st.tile_base, nt, k.st.keys_in, k.st.idx_in, make_spad(seed));
    tr(hipGetLastError());
  }
  k.st.sort(tr, k.tmp, stream);
  const unsigned grid = (unsigned)((N + kSkBlock - 1) / kSkBlock);
  const uint64_t mask = k.st.mask();
  ralle_mark<kSkBlock>(tr, k.st, n, stream);
  if (tr.ok()) {
    subkeys_bound_kernel<<<grid, kSkBlock, 0, stream>>>(k.st.keys_out, k.st.idx_out, N, n, mask, mark_r);
    tr(hipGetLastError());
  }
  k.st.max_scan(tr, k.tmp, k.st.mark(), last_b, stream);
  k.st.max_scan(tr, k.tmp, mark_r, k.bound_s, stream);
  if (tr.ok()) {
    subkeys_resolve_kernel<<<grid, kSkBlock, 0, stream>>>(s.blobs, n, k.st.keys_out, k.st.idx_out, N, mask, last_b,
                                                         k.bound_s, k.side, rep, child, k.counter);
    tr(hipGetLastError());
  }
  if (tr.ok()) tr(hipMemcpyAsync(host, k.counter, kCounterBytes, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(sc.mark_done(stream));
  if (tr.ok()) tr(hipStreamSynchronize(stream));
  if (tr.ok()) counts[4] = counter_sum(host, 3);
  return done();
}

// Returns a K2H_AMD_* code (the HIP error, if any, in *herr).  1 <= n <= 2^32 - 2.  Synchronises
// the stream once for the start set, once per level run and once at the end.
int launch_ralledata_reach(const uint64_t* edge_off, const uint64_t* child, const uint64_t* rep, uint64_t n,
                           const uint8_t* roots, uint64_t max_levels, uint8_t* reach, uint64_t* counts,
                           hipStream_t stream, hipError_t* herr) {
  *herr = hipSuccess;
  FirstError tr;
  auto done = [&]() {
    *herr = tr.e;
    return !tr.ok() ? K2H_AMD_EHIP : K2H_AMD_OK;
  };
  SkScratch* const scp = g_sk.current(tr);
  if (!tr.ok()) return done();
  SkScratch& sc = *scp;
  std::lock_guard<std::mutex> lk(sc.mu);
  if (!sc.pinned) tr(hipHostMalloc(&sc.pinned, kSkPinnedBytes, hipHostMallocDefault));
  if (!tr.ok()) return done();
  unsigned long long* const host = (unsigned long long*)sc.pinned;
  unsigned long long* const host_word = host + kCounterBytes / 8;
  const size_t nbits = (n + 31) / 32;  // bitmap words
  auto layout = [&](void* base) {
    Carver c(base);
    ReachCols k;
    k.bits = c.take<uint32_t>(nbits);
    k.cur = c.take<uint32_t>(n);
    k.next = c.take<uint32_t>(n);
    k.counter = (unsigned long long*)c.bytes(kCounterBytes + 256);
    k.total = c.total();
    return k;
  };
  if (const int rc = sc.reserve(layout(nullptr).total, stream, herr)) return rc;
  const ReachCols k = layout(sc.p);
  uint32_t *const bits = k.bits, *cur = k.cur, *next = k.next;
  unsigned long long* const counter = k.counter;
  unsigned long long* fcount = counter + kCounterBytes / 8;
  const unsigned grid = (unsigned)((n + kSkBlock - 1) / kSkBlock);
  tr(hipMemsetAsync(bits, 0, align256(nbits * 4), stream));
  tr(hipMemsetAsync(counter, 0, kCounterBytes + 256, stream));
  if (tr.ok()) {
    reach_start_kernel<<<grid, kSkBlock, 0, stream>>>(rep, roots, n, bits, cur, fcount);
    tr(hipGetLastError());
  }
  if (tr.ok()) tr(hipMemcpyAsync(host_word, fcount, 8, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(hipStreamSynchronize(stream));
  uint64_t fc = tr.ok() ? *host_word : 0, levels = 0;
  int w = 0;
  while (tr.ok() && fc && (!max_levels || levels < max_levels)) {
    w ^= 1;
    tr(hipMemsetAsync(fcount + w, 0, 8, stream));
    if (tr.ok()) {
      reach_level_kernel<<<(unsigned)((fc + kSkBlock - 1) / kSkBlock), kSkBlock, 0, stream>>>(cur, fc, edge_off, child, n,
                                                                                             bits, next, fcount + w);
      tr(hipGetLastError());
    }
    if (tr.ok()) tr(hipMemcpyAsync(host_word, fcount + w, 8, hipMemcpyDeviceToHost, stream));
    if (tr.ok()) tr(hipStreamSynchronize(stream));
    if (tr.ok()) fc = *host_word;
    uint32_t* t = cur;
    cur = next;
    next = t;
    ++levels;
  }
  if (tr.ok()) {
    reach_final_kernel<<<grid, kSkBlock, 0, stream>>>(rep, n, bits, reach, counter);
    tr(hipGetLastError());
  }
  if (tr.ok()) tr(hipMemcpyAsync(host, counter, kCounterBytes, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(sc.mark_done(stream));
  if (tr.ok()) tr(hipStreamSynchronize(stream));
  if (tr.ok()) {
    counts[0] = counter_sum(host, 0);
    counts[1] = levels;
    counts[2] = fc == 0 ? 1 : 0;
  }
  return done();
}

}  // namespace k2h
