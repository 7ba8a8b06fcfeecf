// k2hash_amd -- keys looked up in a held RALLEDATA stream (include/k2hash_amd.h section 4e):
// index, find and fetch.
//
// K2HShm::Get(const unsigned char*, size_t, unsigned char**, bool checkattr, ...)
// (lib/k2hshm.cc:1857-1938) reaches its element as SetElementByBinArray does
// (lib/k2hshmdirect.cc:373-378): K2H_HASH_FUNC / K2H_2ND_HASH_FUNC of the key, then hash,
// subhash, key length, key bytes -- the identity dedup, diff, subkeys and apply share
// (k2h_ralle_ident.h).  Those calls sort the held side on every call; a lookup wants it sorted
// once and probed many times:
//
//   index  dedup's first two stages, kept: the gather (one lane per blob: span, header and
//          classify; a participant leaves its stored hash and its side record), the stage's
//          scan, compact and sort (k2h_sort_stage.h).  The sort's outputs and the side column
//          lie in the caller's buffer (k2h_find_layout.h), its inputs and the library's storage
//          in the launcher's scratch.  A 256-byte header is written last.
//   find   one lane per query.  A binary search of the sorted hash column over the participants
//          [0, P) for the end of the run of the query's sorted bits, then the walk of
//          last_held (k2h_ralle_ident.h) BACKWARD through the run: the first entry that agrees
//          in hash, subhash, key length and key bytes is the last blob of the identity.  The
//          attrs of a matched blob that has some are walked for its expire (k2h_ralle_attrs.h),
//          those of no other blob.  Hashes the caller does not pass are computed by a kernel of
//          this file, one lane per query, and not by the CSR tile kernel: that one reads the
//          offsets as one trusted CSR, while here every query is judged alone and nothing of a
//          query that takes no part may be read.
//   fetch  one segment of a list of blobs as a packed CSR column: a sizes kernel (one lane per
//          slot), one in-place exclusive sum, and a copy kernel in which 16 lanes move a slot
//          in 16-byte pieces and a whole block moves a slot of 4 KiB or more.
//
// Memory rule.  No byte outside [0, size) of the stream or [0, key_bytes) of the keys is read.  A
// held key is compared in 16-byte chunks that END at its last byte and starts at or after byte 80
// of its blob, so chunk 0 never begins below the stream; a query may start fewer than 16 bytes
// into its buffer, and then chunk 0 is put together from the query's own bytes
// (chunk0_from_bytes).  fetch reads the bytes of the segment alone and writes [0, total) of out.
// All absolute offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <mutex>

#include "k2h_endwalk.h"
#include "k2h_find_layout.h"
#include "k2h_kernels.h"
#include "k2h_ralle_attrs.h"
#include "k2h_ralle_header.h"
#include "k2h_ralle_ident.h"

namespace k2h {
namespace {

static_assert(sizeof(Side) == kIndexSideBytes, "the index's side column");
constexpr int kFindBlock = 256;    // find, hash: queries per block, one per thread
constexpr int kFetchGroup = 16;    // copy: lanes per slot
constexpr int kFetchSlots = 256 / kFetchGroup;
static_assert(kFetchGroup >= 16 && 256 % kFetchGroup == 0, "fetch_move: the up to 15 tail bytes go a byte per lane");
constexpr uint64_t kFetchBig = 4096;  // copy: a slot of this many bytes or more is moved by the whole block

// ------------------------------------------------------------------------------- index
// part[i] = 1 for a participant; its stored hash to hash[i], its side record to side[i]; the
// tile's count.  (dedup's gather without keep / by and without the mtime rule.)
__global__ __launch_bounds__(kIdentBlobs) void ralledata_index_gather_kernel(
    const uint8_t* __restrict__ blobs, uint64_t size, const uint64_t* __restrict__ off, uint64_t n,
    const uint8_t* __restrict__ consider, uint8_t* __restrict__ part_out, uint64_t* __restrict__ hash,
    Side* __restrict__ side, uint64_t* __restrict__ tile_count) {
  typedef hipcub::BlockReduce<uint32_t, kIdentBlobs> Reduce;
  __shared__ typename Reduce::TempStorage tmp;
  const uint64_t i = (uint64_t)blockIdx.x * kIdentBlobs + threadIdx.x;
  uint32_t part = 0;
  if (i < n && (!consider || consider[i])) {
    const uint64_t b = off[i], e = off[i + 1];
    if (e >= b && e <= size && e - b >= (uint64_t)kHdr) {
      uint64_t f[10];
      load_fields(blobs + b, f);
      if (classify(f, e - b) == K2H_AMD_RALLE_OK) {
        part = 1;
        hash[i] = f[0];
        side[i] = Side{f[1], b + f[6], f[2], f[5] ? 1ull : 0ull};
      }
    }
  }
  if (i < n) part_out[i] = (uint8_t)part;
  const uint32_t count = Reduce(tmp).Sum(part);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = count;
}

// The header, behind everything else of the build; parts == NULL: no participant.
__global__ void ralledata_index_head_kernel(IndexHeader* __restrict__ head, uint64_t n, uint64_t size, uint64_t bits,
                                            uint64_t mask, const uint64_t* __restrict__ parts) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    head->n = n;
    head->size = size;
    head->bits = bits;
    head->mask = mask;
    head->parts = parts ? *parts : 0;
    head->magic = kIndexMagic;
  }
}

// -------------------------------------------------------------------------------- find
// Whether query i takes part, and its bytes [b, e).
__device__ __forceinline__ bool query_span(const uint64_t* __restrict__ key_off, uint64_t i, uint64_t key_bytes,
                                           bool cstr, uint64_t& b, uint64_t& e) {
  b = key_off[i];
  e = key_off[i + 1];
  return b <= e && e <= key_bytes && (cstr || e > b);
}

// K2H_HASH_FUNC / K2H_2ND_HASH_FUNC of every query that takes part; CSTR: of the bytes and a NUL
// (a zero byte is a bare multiply: h1 = state * P, h2 = state; the empty string is "\0").
template <bool CSTR>
__global__ __launch_bounds__(kFindBlock) void ralledata_find_hash_kernel(
    const uint8_t* __restrict__ keys, uint64_t key_bytes, const uint64_t* __restrict__ key_off, uint64_t m,
    SpadTable sp, uint64_t* __restrict__ h1, uint64_t* __restrict__ h2) {
  __shared__ uint64_t spad[16];
  if (threadIdx.x < 16) spad[threadIdx.x] = sp.v[threadIdx.x];
  __syncthreads();
  const uint64_t i = (uint64_t)blockIdx.x * kFindBlock + threadIdx.x;
  if (i >= m) return;
  uint64_t b, e, r1 = 0, r2 = 0;
  if (query_span(key_off, i, key_bytes, CSTR, b, e)) {
    const uint64_t len = e - b, k = (len + 15) >> 4;
    if constexpr (CSTR) {
      uint64_t raw = spad[0];
      if (len) end_aligned_walk_ptr<false>(k, (uint32_t)(16 * k - len), keys + e - 16 * k, keys, spad, raw, r2);
      r1 = raw * kPrime;
      r2 = len ? raw : r1;
    } else {
      end_aligned_walk_ptr(k, (uint32_t)(16 * k - len), keys + e - 16 * k, keys, spad, r1, r2);
      if (len == 1) r2 = r1;  // length 1: second hash not shortened (lib/k2hashfunc.cc:83)
    }
  }
  h1[i] = r1;
  h2[i] = r2;
}

// The query's cl >= 1 bytes at q against a held key's first cl bytes at h: same_key, but chunk 0
// of the query is not loaded whole where it would begin below `low`, the query buffer's start.
__device__ __forceinline__ bool same_query(const uint8_t* q, const uint8_t* low, const uint8_t* h, uint64_t cl) {
  const uint64_t k = (cl + 15) >> 4;
  const uint32_t lead = (uint32_t)(16 * k - cl);
  const uint8_t* cq = q + cl - 16 * k;
  const uint8_t* ch = h + cl - 16 * k;
  const uint4 q0 = cq >= low ? ld16(cq) : chunk0_from_bytes(lead, [=](uint32_t i) { return (uint32_t)cq[lead + i]; });
  if (differ(mask_lead(q0, lead), mask_lead(ld16(ch), lead))) return false;
  for (uint64_t c = 1; c < k; ++c)
    if (differ(ld16(cq + 16 * c), ld16(ch + 16 * c))) return false;
  return true;
}

struct FindNow {
  int on;
  int64_t sec, nsec;
};

// One lane per query.  counter: words 0, 1, 2 of the counter lines take the queries that take
// part, found and expired.
template <bool CSTR>
__global__ __launch_bounds__(kFindBlock) void ralledata_find_kernel(
    const uint8_t* __restrict__ blobs, uint64_t size, const uint64_t* __restrict__ blob_off, uint64_t n,
    const IndexHeader* __restrict__ head, const uint64_t* __restrict__ skeys, const uint32_t* __restrict__ sidx,
    const Side* __restrict__ side, const uint8_t* __restrict__ keys, uint64_t key_bytes,
    const uint64_t* __restrict__ key_off, uint64_t m, const uint64_t* __restrict__ h1, const uint64_t* __restrict__ h2,
    FindNow now, uint64_t* __restrict__ match, uint8_t* __restrict__ status, uint8_t* __restrict__ hit,
    unsigned long long* __restrict__ counter) {
  const uint64_t i = (uint64_t)blockIdx.x * kFindBlock + threadIdx.x;
  if (head->magic != kIndexMagic || head->n != n || head->size != size) {  // (uniform)
    if (i < m) {
      status[i] = K2H_AMD_FIND_BAD_INDEX;
      if (match) match[i] = ~0ull;
    }
    return;
  }
  uint32_t st = 0;
  uint32_t found = kNone;
  uint64_t b, e;
  if (i < m && query_span(key_off, i, key_bytes, CSTR, b, e)) {
    st = K2H_AMD_FIND_PART;
    const uint64_t h = h1[i], sub = h2[i], len = e - b, L = len + (CSTR ? 1 : 0);
    const uint64_t mask = head->mask, hm = h & mask;
    uint64_t lo = 0, hi = head->parts;
    while (lo < hi) {  // the first position whose sorted bits lie above the query's
      const uint64_t mid = lo + ((hi - lo) >> 1);
      if ((skeys[mid] & mask) <= hm) lo = mid + 1;
      else hi = mid;
    }
    for (uint64_t q = lo; q > 0; --q) {
      const uint64_t hq = skeys[q - 1];
      if ((hq ^ h) & mask) break;
      if (hq != h) continue;  // another hash with the same sorted bits
      const uint32_t c = sidx[q - 1];
      const Side sc = side[c];
      if (sc.sub != sub || sc.klen != L) continue;
      if (CSTR && blobs[sc.koff + len] != 0) continue;  // the held key's last byte
      if (len && !same_query(keys + b, keys, blobs + sc.koff, len)) continue;
      found = c;
      st |= K2H_AMD_FIND_FOUND | (sc.attrs ? K2H_AMD_FIND_ATTRS : 0u);
      break;
    }
    if ((st & K2H_AMD_FIND_ATTRS) && now.on) {  // a participant: its header passed classify
      const uint8_t* p = blobs + blob_off[found];
      const AttrTimes t = walk_attrs(p + ld8(p + 72), ld8(p + 40));
      if ((t.flags & kAttrExpire) && time_less(t.esec, t.ensec, now.sec, now.nsec)) st |= K2H_AMD_FIND_EXPIRED;
    }
    if (hit && found != kNone) hit[found] = 1;
  }
  if (i < m) {
    status[i] = (uint8_t)st;
    if (match) match[i] = found == kNone ? ~0ull : (uint64_t)found;
  }
  // one atomic per wave and word, neighbouring waves on different lines (k2h_layout.h)
  const unsigned long long mp = __ballot(st & K2H_AMD_FIND_PART), mf = __ballot(st & K2H_AMD_FIND_FOUND),
                           mx = __ballot(st & K2H_AMD_FIND_EXPIRED);
  if ((threadIdx.x & 63u) == 0 && mp) {
    const uint32_t wave = blockIdx.x * (kFindBlock / 64) + (threadIdx.x >> 6);
    unsigned long long* line = counter + kCounterLineWords * (wave % kCounterLines);
    atomicAdd(line, (unsigned long long)__popcll(mp));
    if (mf) atomicAdd(line + 1, (unsigned long long)__popcll(mf));
    if (mx) atomicAdd(line + 2, (unsigned long long)__popcll(mx));
  }
}

// ------------------------------------------------------------------------------- fetch
// place[i] = the bytes slot i yields, place[m] = 0; src[i] = where they start, from `blobs`.
__global__ __launch_bounds__(256) void ralledata_fetch_sizes_kernel(
    const uint8_t* __restrict__ blobs, uint64_t size, const uint64_t* __restrict__ off, uint64_t n,
    const uint64_t* __restrict__ which, uint64_t m, const uint8_t* __restrict__ take, uint32_t segment,
    uint64_t* __restrict__ place, uint64_t* __restrict__ src, uint8_t* __restrict__ bad) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i > m) return;
  uint64_t len = 0, from = 0;
  uint32_t isbad = 0;
  if (i < m && (!take || take[i])) {
    const uint64_t w = which[i];
    if (w != ~0ull) {
      isbad = 1;
      if (w < n) {
        const uint64_t b = off[w], e = off[w + 1];
        if (e >= b && e <= size && e - b >= (uint64_t)kHdr) {
          const uint64_t L = e - b, sl = ld8(blobs + b + 16 + 8 * segment), sp = ld8(blobs + b + 48 + 8 * segment);
          // a length-0 segment's pos is ignored, as classify ignores it; pos + len is never formed
          if (!sl || (sp <= L && sl <= L - sp)) {
            isbad = 0;
            len = sl;
            from = b + sp;
          }
        }
      }
    }
  }
  place[i] = len;
  if (i < m) {
    src[i] = from;
    if (bad) bad[i] = (uint8_t)isbad;
  }
}

// `len` bytes from s to d by `lanes` lanes, this one lane q: whole 16-byte pieces at any
// alignment of either side, then the tail a byte per lane.  Only [s, s + len) is read and only
// [d, d + len) written.
__device__ __forceinline__ void fetch_move(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, uint64_t len,
                                           uint32_t q, uint32_t lanes) {
  const uint64_t full = len & ~15ull;
  for (uint64_t j = 16ull * q; j < full; j += 16ull * lanes)
    *reinterpret_cast<u32x4_ua*>(d + j) = *reinterpret_cast<const u32x4_ua*>(s + j);
  const uint64_t t = full + q;
  if (t < len) d[t] = s[t];
}

// place: the scanned sizes.  A group of 16 lanes per slot; then the block's slots of kFetchBig
// bytes or more, each by all 256 threads.
__global__ __launch_bounds__(256) void ralledata_fetch_copy_kernel(const uint8_t* __restrict__ blobs,
                                                                   const uint64_t* __restrict__ place,
                                                                   const uint64_t* __restrict__ src, uint64_t m,
                                                                   uint8_t* __restrict__ out) {
  const uint64_t first = (uint64_t)blockIdx.x * kFetchSlots;
  const uint64_t slot = first + threadIdx.x / kFetchGroup;
  if (slot < m) {
    const uint64_t d = place[slot], len = place[slot + 1] - d;
    if (len && len < kFetchBig) fetch_move(blobs + src[slot], out + d, len, threadIdx.x % kFetchGroup, kFetchGroup);
  }
  for (uint64_t s = first; s < first + kFetchSlots && s < m; ++s) {  // (uniform)
    const uint64_t d = place[s], len = place[s + 1] - d;
    if (len >= kFetchBig) fetch_move(blobs + src[s], out + d, len, threadIdx.x, 256);
  }
}

// The calls' temporaries (k2h_scratch.h), one family per entry point.
PerDevice<> g_index, g_find, g_fetch;

struct IndexTmp {
  SortStage<> st;
  uint8_t* part;
  void* tmp;
  size_t total;
};

struct FindTmp {
  uint64_t *h1, *h2;
  unsigned long long* counter;
  size_t total;
};

struct FetchTmp {
  uint64_t *place, *src;
  void* tmp;
  size_t total;
};

}  // namespace

uint64_t ralledata_index_bytes(uint64_t n) { return index_layout(nullptr, n).total; }

// Returns a K2H_AMD_* code (the HIP error, if any, in *herr); synchronises the stream once when
// participants != NULL, else not at all.  n <= 2^32 - 2, `index` at least ralledata_index_bytes(n).
int launch_ralledata_index(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                           const uint8_t* consider, void* index, uint64_t* participants, hipStream_t stream,
                           hipError_t* herr) {
  *herr = hipSuccess;
  const IndexCols ix = index_layout(index, n);
  const int bits = sort_bits_for(n ? n : 1);
  FirstError tr;
  if (n == 0) {
    ralledata_index_head_kernel<<<1, 64, 0, stream>>>(ix.head, 0, size, (uint64_t)bits, sort_mask(bits), nullptr);
    tr(hipGetLastError());
    if (participants) {
      tr(hipStreamSynchronize(stream));
      *participants = 0;
    }
    *herr = tr.e;
    return tr.ok() ? K2H_AMD_OK : K2H_AMD_EHIP;
  }
  const uint64_t nt = (n + kIdentBlobs - 1) / kIdentBlobs;
  DeviceScratch* const sc = g_index.current(tr);
  SortStage<> st;
  st.measure(tr, n, nt, stream);
  if (!tr.ok()) {
    *herr = tr.e;
    return K2H_AMD_EHIP;
  }
  // the sort's outputs are the index's columns; its inputs, the tiles and the library's storage
  // are the scratch's
  auto layout = [&](void* base) {
    Carver c(base);
    IndexTmp k;
    k.st = st;
    k.st.keys_out = ix.hash;
    k.st.idx_out = ix.idx;
    k.st.keys_in = c.take<uint64_t>(n);
    k.st.idx_in = c.take<uint32_t>(n);
    k.st.tile_count = c.take<uint64_t>(nt + 1);
    k.st.tile_base = c.take<uint64_t>(nt + 1);
    k.part = c.take<uint8_t>(n);
    k.tmp = c.bytes(st.tmp_bytes());
    k.total = c.total();
    return k;
  };
  std::lock_guard<std::mutex> lk(sc->mu);
  if (const int rc = sc->reserve(layout(nullptr).total, stream, herr)) return rc;
  const IndexTmp k = layout(sc->p);
  k.st.clear(tr, stream);
  if (tr.ok()) {
    ralledata_index_gather_kernel<<<(unsigned)nt, kIdentBlobs, 0, stream>>>(
        (const uint8_t*)blobs, size, blob_off, n, consider, k.part, k.st.hashes(), (Side*)ix.side, k.st.tile_count);
    tr(hipGetLastError());
  }
  k.st.scan_tiles(tr, k.tmp, stream);
  ralle_compact<kIdentBlobs>(tr, k.st, k.part, n, 0, stream);
  k.st.sort(tr, k.tmp, stream);
  if (tr.ok()) {
    ralledata_index_head_kernel<<<1, 64, 0, stream>>>(ix.head, n, size, (uint64_t)k.st.bits, k.st.mask(),
                                                      k.st.tile_base + nt);
    tr(hipGetLastError());
  }
  uint64_t parts = 0;
  if (tr.ok() && participants) tr(hipMemcpyAsync(&parts, k.st.tile_base + nt, 8, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(sc->mark_done(stream));
  if (tr.ok() && participants) {
    tr(hipStreamSynchronize(stream));
    if (tr.ok()) *participants = parts;
  }
  *herr = tr.e;
  return !tr.ok() ? K2H_AMD_EHIP : K2H_AMD_OK;
}

// Returns a K2H_AMD_* code (the HIP error in *herr); synchronises the stream once when
// counts != NULL, else not at all.  m >= 1, n <= 2^32 - 2; h1 and h2 both given or both NULL
// (then hashed with `seed`); now is a host pointer, read before the call returns.
int launch_ralledata_find(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n, const void* index,
                          const void* keys, uint64_t key_bytes, const uint64_t* key_off, uint64_t m,
                          const uint64_t* h1, const uint64_t* h2, uint64_t seed, bool cstr,
                          const k2h_amd_timespec* now, uint64_t* match, uint8_t* status, uint8_t* hit,
                          uint64_t* counts, hipStream_t stream, hipError_t* herr) {
  *herr = hipSuccess;
  const IndexCols ix = index_layout(const_cast<void*>(index), n);
  const FindNow fn = now ? FindNow{1, now->sec, now->nsec} : FindNow{0, 0, 0};
  const bool hashed = !h1;
  FirstError tr;
  DeviceScratch* const sc = g_find.current(tr);
  if (!tr.ok()) {
    *herr = tr.e;
    return K2H_AMD_EHIP;
  }
  auto layout = [&](void* base) {
    Carver c(base);
    FindTmp k;
    k.counter = (unsigned long long*)c.bytes(kCounterBytes);
    k.h1 = c.take<uint64_t>(hashed ? m : 0);
    k.h2 = c.take<uint64_t>(hashed ? m : 0);
    k.total = c.total();
    return k;
  };
  std::lock_guard<std::mutex> lk(sc->mu);
  if (const int rc = sc->reserve(layout(nullptr).total, stream, herr)) return rc;
  const FindTmp k = layout(sc->p);
  const unsigned grid = (unsigned)((m + kFindBlock - 1) / kFindBlock);
  tr(hipMemsetAsync(k.counter, 0, kCounterBytes, stream));
  if (tr.ok() && hit && n) tr(hipMemsetAsync(hit, 0, n, stream));
  if (tr.ok() && hashed) {
    const SpadTable sp = make_spad(seed);
    if (cstr)
      ralledata_find_hash_kernel<true><<<grid, kFindBlock, 0, stream>>>((const uint8_t*)keys, key_bytes, key_off, m, sp,
                                                                       k.h1, k.h2);
    else
      ralledata_find_hash_kernel<false><<<grid, kFindBlock, 0, stream>>>((const uint8_t*)keys, key_bytes, key_off, m, sp,
                                                                        k.h1, k.h2);
    tr(hipGetLastError());
  }
  if (tr.ok()) {
    const uint64_t *q1 = hashed ? k.h1 : h1, *q2 = hashed ? k.h2 : h2;
    if (cstr)
      ralledata_find_kernel<true><<<grid, kFindBlock, 0, stream>>>(
          (const uint8_t*)blobs, size, blob_off, n, ix.head, ix.hash, ix.idx, (const Side*)ix.side, (const uint8_t*)keys,
          key_bytes, key_off, m, q1, q2, fn, match, status, hit, k.counter);
    else
      ralledata_find_kernel<false><<<grid, kFindBlock, 0, stream>>>(
          (const uint8_t*)blobs, size, blob_off, n, ix.head, ix.hash, ix.idx, (const Side*)ix.side, (const uint8_t*)keys,
          key_bytes, key_off, m, q1, q2, fn, match, status, hit, k.counter);
    tr(hipGetLastError());
  }
  unsigned long long lines[kCounterBytes / 8];
  if (tr.ok() && counts) tr(hipMemcpyAsync(lines, k.counter, kCounterBytes, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(sc->mark_done(stream));
  if (tr.ok() && counts) {
    tr(hipStreamSynchronize(stream));
    if (tr.ok())
      for (int w = 0; w < 3; ++w) counts[w] = counter_sum(lines, w);
  }
  *herr = tr.e;
  return !tr.ok() ? K2H_AMD_EHIP : K2H_AMD_OK;
}

// Returns a K2H_AMD_* code (the HIP error in *herr) and synchronises the stream once to return
// *total.  m >= 1; out == NULL: sizes only; *total > out_cap: K2H_AMD_EINVAL with nothing written
// to out.
int launch_ralledata_fetch(const void* blobs, uint64_t size, const uint64_t* blob_off, uint64_t n,
                           const uint64_t* which, uint64_t m, const uint8_t* take, uint32_t segment, void* out,
                           uint64_t out_cap, uint64_t* out_off, uint8_t* bad, uint64_t* total, hipStream_t stream,
                           hipError_t* herr) {
  *herr = hipSuccess;
  FirstError tr;
  DeviceScratch* const sc = g_fetch.current(tr);
  size_t scan_bytes = 0;
  tr(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, m + 1, stream));
  if (!tr.ok()) {
    *herr = tr.e;
    return K2H_AMD_EHIP;
  }
  auto layout = [&](void* base) {
    Carver c(base);
    FetchTmp k;
    k.place = c.take<uint64_t>(m + 1);
    k.src = c.take<uint64_t>(m);
    k.tmp = c.bytes(scan_bytes);
    k.total = c.total();
    return k;
  };
  std::lock_guard<std::mutex> lk(sc->mu);
  if (const int rc = sc->reserve(layout(nullptr).total, stream, herr)) return rc;
  const FetchTmp k = layout(sc->p);
  ralledata_fetch_sizes_kernel<<<(unsigned)((m + 1 + 255) / 256), 256, 0, stream>>>(
      (const uint8_t*)blobs, size, blob_off, n, which, m, take, segment, k.place, k.src, bad);
  tr(hipGetLastError());
  if (tr.ok()) tr(hipcub::DeviceScan::ExclusiveSum(k.tmp, scan_bytes, k.place, k.place, m + 1, stream));
  if (tr.ok() && out_off) tr(hipMemcpyAsync(out_off, k.place, (m + 1) * 8, hipMemcpyDeviceToDevice, stream));
  uint64_t tot = 0;
  if (tr.ok()) tr(hipMemcpyAsync(&tot, k.place + m, 8, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(hipStreamSynchronize(stream));
  int rc = K2H_AMD_OK;
  if (tr.ok()) {
    *total = tot;
    if (out && tot > out_cap) {
      rc = K2H_AMD_EINVAL;
    } else if (out && tot) {
      ralledata_fetch_copy_kernel<<<(unsigned)((m + kFetchSlots - 1) / kFetchSlots), 256, 0, stream>>>(
          (const uint8_t*)blobs, k.place, k.src, m, (uint8_t*)out);
      tr(hipGetLastError());
    }
  }
  if (tr.ok()) tr(sc->mark_done(stream));
  *herr = tr.e;
  return !tr.ok() ? K2H_AMD_EHIP : rc;
}

}  // namespace k2h
