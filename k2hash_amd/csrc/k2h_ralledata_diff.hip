// k2hash_amd -- RALLEDATA consumer side: two blob streams in device memory joined by identity
// (include/k2hash_amd.h section 4b''''').
//
// A is an incoming stream, B a dump of what the table holds.  For every participant i of A the
// call finds the last participant of B with i's identity -- stored hash, stored subhash, key
// length, key bytes, the identity of K2HShm::SetElementByBinArray (lib/k2hshmdirect.cc:373-378)
// and of k2h_ralledata_dedup.hip -- and compares the value, subkeys and attrs segments of the
// pair byte for byte.  With the caller's pts and clock it also restates :380-431 with the
// matched blob's attrs as the existing element's: whether the call would go on to write.
//
// Both streams share one index space, B at [0, nb) and A at [nb, nb + na).  Four stages, all
// on the caller's stream (the scan, compact and sort behind the gather and the max-scan are the
// sort stage of k2h_sort_stage.h):
//   gather   one lane per blob of B, then of A: span, header and classify (k2h_ralle_header.h);
//            a participant leaves its stored hash and a side record (k2h_ralle_ident.h) whose
//            last word holds its flags; with times it also has its attrs walked
//            (k2h_ralle_attrs.h) and leaves its mtime, and a blob of B whether it is expired
//            at `now`.
//   sort     stable, so within a run of equal sorted bits all of B's entries come first, in
//            stream order, followed by A's in stream order.
//   resolve  a mark kernel and one inclusive max-scan give every sorted position the nearest
//            B entry at or before it.  One lane per sorted A entry starts there and walks
//            BACKWARD over B's entries while the sorted bits agree, to the first one of its
//            identity: the last such blob of B.  REPEAT looks for an equal 64-bit hash among
//            the A entries of the run, forward first and then backward, to the first hit.
//            The lane writes match, seen and every bit of rel but the byte compares' (unequal
//            segment lengths set their bit here, with no payload byte read), and leaves the
//            matched index as a work item when some segment has equal non-zero lengths.
//   compare  one lane per blob of A.  A pair with at most kDiffWaveBytes to compare is compared
//            by its lane, each segment in 16-byte chunks that END at the segment's last byte,
//            the lead bytes of chunk 0 masked (same_key's technique: the two segments sit at
//            unrelated alignments).  A pair with more is compared by its whole wave, 64 chunks
//            of each side per step and a ballot.  The kernel also counts.
//
// Cost.  r copies of one key in A, matched or not, cost O(1) steps per lane: the walk over B
// starts at the run's last B entry and meets only B's entries, and a copy's neighbour in the
// run stores its hash.  r DISTINCT identities that share the sorted bits, in A or in B, cost
// O(r) steps per lane, O(r^2) in all: a crafted stream, or one whose hash fields
// k2h_amd_ralledata_check would have refused (the case k2h_ralledata_dedup.hip documents).
//
// Reads.  No byte outside [0, size) of either stream: every compared range starts at or after
// byte 80 of its blob, so chunk 0 never begins below the buffer, and no chunk passes the
// range's end.  Nothing of a non-participant beyond its header, nothing of a blob whose span
// is bad or whose consider byte is 0, and no payload byte of a pair whose segment lengths
// differ.
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

constexpr int kDiffBlobs = 256;         // gather / compact / compare: blobs per 256-thread block
constexpr int kDiffResolveBlock = 256;  // resolve: sorted positions per block, one per thread
constexpr int kDiffWaveBytes = 128;     // a pair with more bytes to compare than this is compared by its wave

// Side::attrs of this file's gather.
constexpr uint64_t kFlagAttrs = 1;    // attrs_length != 0
constexpr uint64_t kFlagMtime = 2;    // with times: the attrs give an mtime
constexpr uint64_t kFlagExpired = 4;  // with times, B only: expired at `now`
constexpr uint64_t kFlagData = 8;     // a value, subkeys or attrs (lib/k2hshmdirect.cc:438)

struct __attribute__((aligned(16))) DiffMtime {
  int64_t sec, nsec;
};

struct DiffStream {
  const uint8_t* blobs;
  uint64_t size;
  const uint64_t* off;
  const uint8_t* consider;
};

struct DiffTimes {
  DiffMtime* mt;  // nb + na entries; written only for a blob with kFlagMtime
  int64_t pts_sec, pts_nsec, now_sec, now_nsec;
};

// part[g] = 1 for a participant, its stored hash to hash[g], its side record to side[g]; the
// tile's count.  A blob of A that does not take part gets rel 0 and match ~0 here.  TM: the
// attrs of a participant that has some are walked.
template <bool TM>
__global__ __launch_bounds__(256) void ralledata_diff_gather_kernel(DiffStream a, uint64_t na, DiffStream b,
                                                                    uint64_t nb, uint8_t* __restrict__ part,
                                                                    uint64_t* __restrict__ hash,
                                                                    Side* __restrict__ side,
                                                                    uint64_t* __restrict__ tile_count,
                                                                    uint8_t* __restrict__ rel,
                                                                    uint64_t* __restrict__ match, DiffTimes tm) {
  typedef hipcub::BlockReduce<uint32_t, kDiffBlobs> Reduce;
  __shared__ typename Reduce::TempStorage tmp;
  const uint64_t g = (uint64_t)blockIdx.x * kDiffBlobs + threadIdx.x;
  const bool in_a = g >= nb;
  const DiffStream s = in_a ? a : b;
  const uint64_t i = in_a ? g - nb : g;
  uint32_t p = 0;
  if (g < nb + na && (!s.consider || s.consider[i])) {
    const uint64_t o = s.off[i], e = s.off[i + 1];
    if (e >= o && e <= s.size && e - o >= (uint64_t)kHdr) {
      uint64_t f[10];
      load_fields(s.blobs + o, f);
      if (classify(f, e - o) == K2H_AMD_RALLE_OK) {
        p = 1;
        hash[g] = f[0];
        uint64_t flags = (f[5] ? kFlagAttrs : 0) | ((f[3] | f[4] | f[5]) ? kFlagData : 0);
        if constexpr (TM) {
          if (f[5]) {
            const AttrTimes t = walk_attrs(s.blobs + o + f[9], f[5]);
            if (t.flags & kAttrMtime) {
              flags |= kFlagMtime;
              tm.mt[g] = DiffMtime{t.msec, t.mnsec};
            }
            if (!in_a && (t.flags & kAttrExpire) && time_less(t.esec, t.ensec, tm.now_sec, tm.now_nsec))
              flags |= kFlagExpired;
          }
        }
        side[g] = Side{f[1], o + f[6], f[2], flags};
      }
    }
  }
  if (g < nb + na) {
    part[g] = (uint8_t)p;
    if (in_a && !p) {
      rel[i] = 0;
      if (match) match[i] = ~0ull;
    }
  }
  const uint32_t count = Reduce(tmp).Sum(p);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = count;
}

struct Lens {
  uint64_t v, s, a;  // val, skey, attrs length
};
__device__ __forceinline__ Lens load_lens(const uint8_t* blob) {
  const uint4 x = ld16(blob + 16), y = ld16(blob + 32);
  return Lens{pack2(x.z, x.w), pack2(y.x, y.y), pack2(y.z, y.w)};
}

// keys / idx: the pairs, sorted by the hash bits under `mask`; last_b[p]: 1 + the nearest
// position at or before p that holds an entry of B, 0 when there is none.
template <bool TM>
__global__ __launch_bounds__(kDiffResolveBlock) void ralledata_diff_resolve_kernel(
    DiffStream a, DiffStream b, uint64_t nb, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx,
    uint64_t n, uint64_t mask, const uint32_t* __restrict__ last_b, const Side* __restrict__ side,
    uint8_t* __restrict__ rel, uint64_t* __restrict__ match, uint8_t* __restrict__ seen,
    uint32_t* __restrict__ work, DiffTimes tm) {
  const uint64_t p = (uint64_t)blockIdx.x * kDiffResolveBlock + threadIdx.x;
  if (p >= n) return;
  const uint32_t g = idx[p];
  if (g == kNone || g < nb) return;  // a non-participant, or an entry of B
  const uint64_t i = g - nb;
  const uint64_t h = keys[p];
  const Side sa = side[g];
  uint32_t r = K2H_AMD_DIFF_PART | ((sa.attrs & kFlagData) ? K2H_AMD_DIFF_DATA : 0u);

  // the last blob of B with i's identity: backward over the run's B entries
  const uint32_t j = last_held(keys, idx, side, last_b[p], h, mask, nb, sa, a.blobs, b.blobs);

  // another participant of A with i's stored hash: forward, then backward, over the run's A entries
  bool repeat = false;
  for (uint64_t q = p + 1; q < n; ++q) {
    const uint64_t hq = keys[q];
    if (((hq ^ h) & mask) || idx[q] == kNone) break;
    if (hq == h) {
      repeat = true;
      break;
    }
  }
  for (uint64_t q = p; !repeat && q > 0; --q) {
    const uint64_t hq = keys[q - 1];
    if (((hq ^ h) & mask) || idx[q - 1] < nb) break;
    repeat = hq == h;
  }
  if (repeat) r |= K2H_AMD_DIFF_REPEAT;

  bool apply = true;  // not FOUND: the path falls through at :377-378
  if (j != kNone) {
    r |= K2H_AMD_DIFF_FOUND;
    const Lens la = load_lens(a.blobs + a.off[i]), lb = load_lens(b.blobs + b.off[j]);
    if (la.v != lb.v) r |= K2H_AMD_DIFF_VAL;
    if (la.s != lb.s) r |= K2H_AMD_DIFF_SKEY;
    if (la.a != lb.a) r |= K2H_AMD_DIFF_ATTRS;
    const bool bytes = (la.v == lb.v && la.v) || (la.s == lb.s && la.s) || (la.a == lb.a && la.a);
    work[i] = bytes ? j : kNone;
    if (seen) seen[j] = 1;
    if constexpr (TM) {
      const uint64_t fb = side[j].attrs;  // the matched blob's flags, read behind the walk (last_held)
      if (!(fb & kFlagAttrs) || (fb & kFlagExpired) || !(fb & kFlagMtime)) {
        apply = true;  // no attrs page, :390, :395
      } else {
        const DiffMtime mb = tm.mt[j];
        if (!time_less(mb.sec, mb.nsec, tm.pts_sec, tm.pts_nsec)) {
          apply = false;  // :402
        } else if (sa.attrs & kFlagMtime) {
          const DiffMtime mi = tm.mt[g];
          apply = time_less(mb.sec, mb.nsec, mi.sec, mi.nsec);  // :416
        } else {
          apply = false;  // :426
        }
      }
    }
  }
  if constexpr (TM) {
    if (apply) r |= K2H_AMD_DIFF_APPLY;
  }
  rel[i] = (uint8_t)r;
  if (match) match[i] = j == kNone ? ~0ull : (uint64_t)j;
}

// Two byte ranges of one length len >= 1 compared by a whole wave: chunk q of each side, the
// chunks ending at the ranges' last bytes, goes to lane q % 64.  The answer is the wave's.
__device__ __forceinline__ bool wave_ranges_differ(const uint8_t* x, const uint8_t* y, uint64_t len, uint32_t lane) {
  const uint64_t k = (len + 15) >> 4;
  const uint32_t lead = (uint32_t)(16 * k - len);
  const uint8_t* cx = x + len - 16 * k;
  const uint8_t* cy = y + len - 16 * k;
  for (uint64_t base = 0; base < k; base += 64) {
    const uint64_t q = base + lane;
    bool d = false;
    if (q < k) {
      uint4 u = ld16(cx + 16 * q), v = ld16(cy + 16 * q);
      if (q == 0) {
        u = mask_lead(u, lead);
        v = mask_lead(v, lead);
      }
      d = differ(u, v);
    }
    if (__ballot(d)) return true;
  }
  return false;
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
  return pack2(lo, hi);
}

// One lane per blob of A; work[i], written for every FOUND blob: the matched blob of B when
// some segment of the pair has equal non-zero lengths, else kNone.  ORs the differ bits of those segments into rel[i], and
// counts {PART, FOUND, FOUND without a differ bit, APPLY} into the counter lines (four words in each).
__global__ __launch_bounds__(kDiffBlobs) void ralledata_diff_compare_kernel(DiffStream a, uint64_t na, DiffStream b,
                                                                            const uint32_t* __restrict__ work,
                                                                            uint8_t* __restrict__ rel,
                                                                            unsigned long long* __restrict__ counter) {
  const uint64_t i = (uint64_t)blockIdx.x * kDiffBlobs + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t r = i < na ? rel[i] : 0u;
  const uint32_t j = (r & K2H_AMD_DIFF_FOUND) ? work[i] : kNone;
  const uint8_t* x[3] = {nullptr, nullptr, nullptr};
  const uint8_t* y[3] = {nullptr, nullptr, nullptr};
  uint64_t len[3] = {0, 0, 0};  // 0: nothing to compare
  uint32_t found = 0;
  bool wide = false;
  if (j != kNone) {
    const uint8_t* pa = a.blobs + a.off[i];
    const uint8_t* pb = b.blobs + b.off[j];
    uint64_t fa[10], fb[10];
    load_fields(pa, fa);
    load_fields(pb, fb);
    uint64_t total = 0;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      if (fa[3 + s] == fb[3 + s] && fa[3 + s]) {
        len[s] = fa[3 + s];
        x[s] = pa + fa[7 + s];
        y[s] = pb + fb[7 + s];
        total += len[s];  // each is at most its blob's length: no wrap
      }
    }
    wide = total > (uint64_t)kDiffWaveBytes;
    if (!wide) {
#pragma unroll
      for (int s = 0; s < 3; ++s)
        if (len[s] && !same_key(x[s], y[s], len[s])) found |= K2H_AMD_DIFF_VAL << s;
    }
  }
  for (unsigned long long todo = __ballot(wide); todo; todo &= todo - 1) {
    const int src = __ffsll((long long)todo) - 1;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const uint64_t l = shfl_u64(len[s], src);
      const uint8_t* px = (const uint8_t*)shfl_u64((uint64_t)x[s], src);
      const uint8_t* py = (const uint8_t*)shfl_u64((uint64_t)y[s], src);
      if (l && wave_ranges_differ(px, py, l, lane) && lane == (uint32_t)src) found |= K2H_AMD_DIFF_VAL << s;
    }
  }
  if (found) {
    r |= found;
    rel[i] = (uint8_t)r;
  }
  const bool hit = (r & K2H_AMD_DIFF_FOUND) != 0;
  const unsigned long long m0 = __ballot((r & K2H_AMD_DIFF_PART) != 0), m1 = __ballot(hit);
  const unsigned long long m2 =
      __ballot(hit && !(r & (K2H_AMD_DIFF_VAL | K2H_AMD_DIFF_SKEY | K2H_AMD_DIFF_ATTRS)));
  const unsigned long long m3 = __ballot((r & K2H_AMD_DIFF_APPLY) != 0);
  if (lane == 0 && m0) {
    // one line per wave, neighbouring waves on different lines (as the dedup's resolve counts)
    const uint32_t wave = blockIdx.x * (kDiffBlobs / 64) + (threadIdx.x >> 6);
    unsigned long long* c = counter + 8 * (wave % kCounterLines);
    atomicAdd(c, (unsigned long long)__popcll(m0));
    if (m1) atomicAdd(c + 1, (unsigned long long)__popcll(m1));
    if (m2) atomicAdd(c + 2, (unsigned long long)__popcll(m2));
    if (m3) atomicAdd(c + 3, (unsigned long long)__popcll(m3));
  }
}
static_assert(K2H_AMD_DIFF_SKEY == K2H_AMD_DIFF_VAL << 1 && K2H_AMD_DIFF_ATTRS == K2H_AMD_DIFF_VAL << 2,
              "the three differ bits in segment order");

// The call's temporaries (k2h_scratch.h).  With n = na + nb: the stage's two key and two index
// columns and the side records (56 n bytes), a participant byte per blob, the tile counts and
// their scan, the counters and the library's own storage; with times 16 n more for the mtimes.
// The scan column and the na work items need none of their own: they stand in the stage's input
// columns (SortStage::scanned, ::second; n * 4 >= na * 4 bytes).
PerDevice<> g_diff;

struct DiffCols {
  SortStage<> st;
  Side* side;
  uint8_t* part;
  unsigned long long* counter;
  void* tmp;
  DiffMtime* mt;  // with times only, behind everything else
  size_t total;
};

}  // namespace

// Returns a K2H_AMD_* code (the HIP error, if any, in *herr); synchronises the stream once when
// counts != NULL, else not at all.  na >= 1, na + nb <= 2^32 - 2; times is a host pointer.
int launch_ralledata_diff(const void* a_blobs, uint64_t a_size, const uint64_t* a_off, uint64_t na,
                          const uint8_t* a_consider, const void* b_blobs, uint64_t b_size, const uint64_t* b_off,
                          uint64_t nb, const uint8_t* b_consider, const k2h_amd_diff_times* times, uint8_t* rel,
                          uint64_t* match, uint8_t* seen, uint64_t* counts, hipStream_t stream, hipError_t* herr) {
  *herr = hipSuccess;
  const uint64_t n = na + nb;
  const uint64_t nt = (n + kDiffBlobs - 1) / kDiffBlobs;
  FirstError tr;
  DeviceScratch* const sc = g_diff.current(tr);
  SortStage<> st;
  st.measure(tr, n, nt, stream);
  st.measure_max_scan(tr, stream);
  if (!tr.ok()) {
    *herr = tr.e;
    return K2H_AMD_EHIP;
  }
  auto layout = [&](void* base) {
    Carver c(base);
    DiffCols k;
    k.st = st.take(c);
    k.side = c.take<Side>(n);
    k.part = c.take<uint8_t>(n);
    k.counter = (unsigned long long*)c.bytes(kCounterBytes);
    k.tmp = c.bytes(st.tmp_bytes());
    k.mt = c.take<DiffMtime>(times ? n : 0);
    k.total = c.total();
    return k;
  };
  std::lock_guard<std::mutex> lk(sc->mu);
  if (const int rc = sc->reserve(layout(nullptr).total, stream, herr)) return rc;
  const DiffCols k = layout(sc->p);
  uint32_t* const last_b = k.st.scanned();
  uint32_t* const work = k.st.second();

  const DiffStream sa{(const uint8_t*)a_blobs, a_size, a_off, a_consider};
  const DiffStream sb{(const uint8_t*)b_blobs, b_size, b_off, b_consider};
  DiffTimes tm{k.mt, 0, 0, 0, 0};
  if (times) tm = DiffTimes{k.mt, times->pts.sec, times->pts.nsec, times->now.sec, times->now.nsec};
  k.st.clear(tr, stream);
  tr(hipMemsetAsync(k.counter, 0, kCounterBytes, stream));
  if (seen && nb) tr(hipMemsetAsync(seen, 0, nb, stream));
  if (tr.ok()) {
    if (times)
      ralledata_diff_gather_kernel<true><<<(unsigned)nt, kDiffBlobs, kWalkLdsBytes, stream>>>(
          sa, na, sb, nb, k.part, k.st.hashes(), k.side, k.st.tile_count, rel, match, tm);
    else
      ralledata_diff_gather_kernel<false><<<(unsigned)nt, kDiffBlobs, 0, stream>>>(
          sa, na, sb, nb, k.part, k.st.hashes(), k.side, k.st.tile_count, rel, match, tm);
    tr(hipGetLastError());
  }
  k.st.scan_tiles(tr, k.tmp, stream);
  ralle_compact<kDiffBlobs>(tr, k.st, k.part, n, 0, stream);
  k.st.sort(tr, k.tmp, stream);
  ralle_mark<256>(tr, k.st, nb, stream);
  k.st.max_scan(tr, k.tmp, k.st.mark(), last_b, stream);
  if (tr.ok()) {
    const uint64_t grid = (n + kDiffResolveBlock - 1) / kDiffResolveBlock;
    const uint64_t mask = k.st.mask();
    if (times)
      ralledata_diff_resolve_kernel<true><<<(unsigned)grid, kDiffResolveBlock, 0, stream>>>(
          sa, sb, nb, k.st.keys_out, k.st.idx_out, n, mask, last_b, k.side, rel, match, seen, work, tm);
    else
      ralledata_diff_resolve_kernel<false><<<(unsigned)grid, kDiffResolveBlock, 0, stream>>>(
          sa, sb, nb, k.st.keys_out, k.st.idx_out, n, mask, last_b, k.side, rel, match, seen, work, tm);
    tr(hipGetLastError());
  }
  if (tr.ok()) {
    ralledata_diff_compare_kernel<<<(unsigned)((na + kDiffBlobs - 1) / kDiffBlobs), kDiffBlobs, 0, stream>>>(
        sa, na, sb, work, rel, k.counter);
    tr(hipGetLastError());
  }
  unsigned long long host[kCounterBytes / 8];
  if (tr.ok() && counts) tr(hipMemcpyAsync(host, k.counter, kCounterBytes, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(sc->mark_done(stream));
  if (tr.ok() && counts) {
    tr(hipStreamSynchronize(stream));
    if (tr.ok())
      for (int w = 0; w < 4; ++w) counts[w] = counter_sum(host, w);
  }
  *herr = tr.e;
  return !tr.ok() ? K2H_AMD_EHIP : K2H_AMD_OK;
}

}  // namespace k2h
