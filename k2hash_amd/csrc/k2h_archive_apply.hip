// k2hash_amd -- a transaction log applied to a held RALLEDATA stream, both in device memory
// (include/k2hash_amd.h section 5c: k2h_amd_archive_apply).
//
// The held stream is a dump of what a peer's table holds, the log what K2HTransaction wrote
// since.  Per identity -- hash, subhash, key length, key bytes -- the call finds what Load's
// switch (lib/k2harchive.cc:328-341) leaves of the element after the identity's records, the
// prior element being the LAST held blob of that identity, and writes it as one blob in
// GetElementToBinary's layout (lib/k2hshmdirect.cc:59-89).  Held blobs no record touches are
// copied through.  OW_VAL and RENAME are not executed: the first of them ends the log (stop).
//
// Held blobs and records share one index space, blob j at j and record i at na + i.  All on the
// caller's stream:
//   gather   one lane per slot.  A held blob: keep byte, span, header and classify
//            (k2h_ralle_header.h); it leaves its default output size (its span, or 0 when it is
//            left out) and, as a participant, its stored hash and a side record
//            (k2h_ralle_ident.h).  A record: fold's participant test and the consider byte; it
//            leaves its W bits and a DEL_KEY bit in the side record's last word.  A considered
//            OW_VAL or RENAME with status 0 raises the stop word by an atomic max of n - i.
//   count    participants per tile, the records at or behind the stop taken out: only now is
//            the stop known.
//   sort     the sort stage of k2h_sort_stage.h: stable, so in a run of equal sorted bits the held
//            entries come first in stream order, then the records in log order.
//   plan     one lane per sorted position.  Forward to the next entry of the lane's identity.
//            A held blob that has one is superseded (the next is a held blob) or touched (a
//            record) and gives up its output bytes.  A record that has none is its
//            identity's anchor: unless it is a DEL_KEY it walks backward over the run and
//            takes, for every field of {V, S, A} still open, the entry that wrote it last --
//            until the three are covered, at a DEL_KEY (the open fields are empty), at the
//            deciding held blob (it supplies them) or at the run's start.  An entry that writes
//            no open field is passed without a key compare; one that shares only the sorted
//            bits is stepped over on the hash, one that shares the hash on subhash, length and
//            key bytes.  The anchor leaves the three sources and the blob's size.
//   place    two exclusive sums over the slots in index order (PlaceRank), sizes into places and
//            emitted flags into ranks; the counts and the stop come back to the host (the one
//            synchronisation of the call).
//   copy     part 1, the held blobs that are emitted unchanged: ralle_place_copy_kernel
//            (k2h_ralle_copy.h) over the places of the first na slots; place[na] is where
//            part 1 ends.
//   build    part 2, launched only when it is not empty: 8 lanes per anchor.  The header is
//            built in registers, the key and the three fields go through group_copy
//            (k2h_ralle_pieces.h) from wherever their source puts them -- a record's file
//            ranges, a held blob's segments in any order; a field of kApLong bytes or more is
//            moved by the anchor's whole wave.
//
// Cost.  A key with r applied records costs its anchor a backward walk of up to r entries in
// one lane (two dependent loads each, a key compare only for the entries that write an open
// field): the case of a head record before a long run of REPLACE_VALs.  A consider mask from
// k2h_amd_archive_fold over the same prefix shortens every walk to the records that matter.  r
// DISTINCT identities that share the sorted bits cost O(r) steps per lane, as in
// k2h_ralledata_dedup.hip.
//
// Reads.  No byte outside [0, held_size) of the held stream or [0, size) of the file, except
// within the aligned 16 bytes that hold a valid byte: a key is compared in 16-byte chunks that
// END at its last byte, chunk 0 of a key that begins fewer bytes into its buffer than its chunk
// leads it is put together from the key's own bytes; the copies load exact source bytes.  A
// record's data segment whose range is not inside the file is taken as empty.  Nothing of a
// record is read that takes no part, nothing of a held blob that is left out.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include <mutex>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_ralle_copy.h"
#include "k2h_ralle_header.h"
#include "k2h_ralle_ident.h"
#include "k2h_ralle_pieces.h"

// Dynamic LDS, never touched, that a build can give to the plan kernel so that fewer blocks fit
// a CU (k2h_archive_fold.hip): 0 leaves eight waves per SIMD, 64 KiB two.
#ifndef K2H_APPLY_PLAN_LDS
#define K2H_APPLY_PLAN_LDS 0
#endif

namespace k2h {
namespace {

constexpr int kApBlock = 256;         // every kernel but build: slots (or sorted positions) per block, one per thread
constexpr int kApGroup = 8;           // build: lanes per blob
constexpr int kApTabPieces = 4096;    // copy: as kSelTabPieces of the select copy
constexpr uint64_t kApLong = 4096;    // build: a field of at least this many bytes is moved by the whole wave
constexpr size_t kPlanLds = K2H_APPLY_PLAN_LDS;

// Side::attrs of a record: the fields it writes, and whether it is a DEL_KEY.
constexpr uint64_t kV = 1, kS = 2, kA = 4, kDel = 8;

typedef uint32_t u32x2_ua __attribute__((ext_vector_type(2), aligned(1)));

struct ApIn {
  const uint8_t* held;
  uint64_t held_size;
  const uint64_t* held_off;
  uint64_t na;
  const uint8_t* held_keep;
  const uint8_t* file;
  uint64_t size;
  const k2h_amd_archive_rec* recs;
  uint64_t n;
  const uint8_t* consider;
  const uint64_t *h1, *h2;  // the records' hashes: the caller's, or the prehash's
};

struct Seg {
  uint64_t off, len;
};

__device__ __forceinline__ uint64_t ld8(const uint8_t* p) {
  const u32x2_ua v = *reinterpret_cast<const u32x2_ua*>(p);
  return pack2(v.x, v.y);
}

// Field f (0: value, 1: subkeys, 2: attrs) of record i as its own ranges give it; empty when
// the range is not inside the file.
__device__ __forceinline__ Seg rec_seg(const ApIn& s, uint64_t i, int f) {
  const uint64_t* w = reinterpret_cast<const uint64_t*>(s.recs + i) + 4 + 2 * f;
  const uint64_t off = w[0], len = w[1];
  return off <= s.size && len <= s.size - off ? Seg{off, len} : Seg{0, 0};
}

// Field f of entry c of the shared index space: where it lies and how long it is.  kNone: empty.
__device__ __forceinline__ const uint8_t* field_of(const ApIn& s, uint32_t c, int f, uint64_t& len) {
  len = 0;
  if (c == kNone) return nullptr;
  if (c < s.na) {
    const uint8_t* b = s.held + s.held_off[c];
    len = ld8(b + 24 + 8 * f);
    return b + ld8(b + 56 + 8 * f);
  }
  const Seg g = rec_seg(s, c - s.na, f);
  len = g.len;
  return s.file + g.off;
}

// SET_ALL: V always, S and A when the record's own are non-empty (lib/k2hshm.cc:2948-2950);
// REPLACE_VAL / _SKEY / _ATTRS: the one field; DEL_KEY: all three.
__device__ __forceinline__ uint64_t bits_of(const ApIn& s, uint64_t i, int64_t type) {
  switch (type) {
    case 0: return kV | (rec_seg(s, i, 1).len ? kS : 0u) | (rec_seg(s, i, 2).len ? kA : 0u);
    case 1: return kV;
    case 2: return kS;
    case 3: return kV | kS | kA | kDel;
    default: return kA;  // 5
  }
}

__device__ __forceinline__ void ap_count(unsigned long long* counter, int word, bool v) {
  const unsigned long long m = __ballot(v);
  if ((threadIdx.x & 63u) == 0 && m) {
    const uint32_t wave = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
    atomicAdd(counter + 8 * (wave % kCounterLines) + word, (unsigned long long)__popcll(m));
  }
}

// Slot g of the na + n: part[g], and for a participant hash[g] and side[g]; the slot's default
// output -- a held blob that is emitted: its span and flag 1, every other slot nothing -- with
// entry na + n of sizes and flags 0; touched[j] 0 or K2H_AMD_APPLY_LEFT_OUT.  *stopw becomes
// n - stop.
__global__ __launch_bounds__(kApBlock) void apply_gather_kernel(ApIn s, uint8_t* __restrict__ part,
                                                                uint64_t* __restrict__ hash, Side* __restrict__ side,
                                                                uint64_t* __restrict__ sizes, uint32_t* __restrict__ flags,
                                                                uint8_t* __restrict__ touched,
                                                                unsigned long long* __restrict__ stopw) {
  const uint64_t g = (uint64_t)blockIdx.x * kApBlock + threadIdx.x;
  const uint64_t N = s.na + s.n;
  if (g > N) return;
  uint64_t v = 0;
  uint32_t k = 0, p = 0;
  if (g < s.na) {
    uint32_t st = K2H_AMD_APPLY_LEFT_OUT;
    if (!s.held_keep || s.held_keep[g]) {
      const uint64_t o = s.held_off[g], e = s.held_off[g + 1];
      if (e >= o && e <= s.held_size && e - o >= (uint64_t)kHdr) {
        st = 0;
        k = 1;
        v = e - o;
        uint64_t f[10];
        load_fields(s.held + o, f);
        if (classify(f, v) == K2H_AMD_RALLE_OK) {
          p = 1;
          hash[g] = f[0];
          side[g] = Side{f[1], o + f[6], f[2], 0ull};
        }
      }
    }
    if (touched) touched[g] = (uint8_t)st;
  } else if (g < N) {
    const uint64_t i = g - s.na;
    const k2h_amd_archive_rec& r = s.recs[i];
    const int64_t type = r.type;
    if (r.status == 0 && type >= 0 && type <= 6 && (!s.consider || s.consider[i])) {
      if (type == 4 || type == 6) {
        // a barrier: the first one is the stop.  Blocks start roughly in index order, so the
        // word soon holds a value no later barrier can raise, and those skip the atomic.
        const unsigned long long mine = s.n - i;
        if (mine > *(volatile unsigned long long*)stopw) atomicMax(stopw, mine);
      } else {
        const uint64_t koff = r.key_off, klen = r.key_len;
        if (klen >= 1 && koff <= s.size && klen <= s.size - koff) {
          p = 1;
          hash[g] = s.h1[i];
          side[g] = Side{s.h2[i], koff, klen, bits_of(s, i, type)};
        }
      }
    }
  }
  sizes[g] = v;
  flags[g] = k;
  if (g < N) part[g] = (uint8_t)p;
}

// The tile's participants, a record at or behind the stop no longer one of them.
__global__ __launch_bounds__(kApBlock) void apply_count_kernel(uint8_t* __restrict__ part, uint64_t na, uint64_t n,
                                                               const unsigned long long* __restrict__ stopw,
                                                               uint64_t* __restrict__ tile_count) {
  typedef hipcub::BlockReduce<uint32_t, kApBlock> Reduce;
  __shared__ typename Reduce::TempStorage tmp;
  const uint64_t g = (uint64_t)blockIdx.x * kApBlock + threadIdx.x;
  const uint64_t stop = n - *stopw;
  uint32_t p = 0;
  if (g < na + n) {
    p = part[g];
    if (p && g >= na && g - na >= stop) {
      p = 0;
      part[g] = 0;
    }
  }
  const uint32_t count = Reduce(tmp).Sum(p);
  if (threadIdx.x == 0) tile_count[blockIdx.x] = count;
}

// Chunk 0 of the key at offset a of buffer f whose chunks end at its last byte: the 16 bytes
// from a - lead with the lead bytes zeroed; only the key's own bytes where that would begin
// below the buffer (k2h_archive_fold.hip).
__device__ __forceinline__ uint4 ap_chunk0(const uint8_t* f, uint64_t a, uint32_t lead) {
  if (a >= lead) return mask_lead(ld16(f + (a - lead)), lead);
  return chunk0_from_bytes(lead, [=](uint32_t j) { return (uint32_t)f[a + j]; });
}

// Two keys of one length kl >= 1, at offset a of buffer x and offset b of buffer y.
__device__ __forceinline__ bool ap_same_key(const uint8_t* x, uint64_t a, const uint8_t* y, uint64_t b, uint64_t kl) {
  const uint64_t k = (kl + 15) >> 4;
  const uint32_t lead = (uint32_t)(16 * k - kl);
  if (differ(ap_chunk0(x, a, lead), ap_chunk0(y, b, lead))) return false;
  for (uint64_t q = 1; q < k; ++q)  // (a - lead may wrap; a - lead + 16 q >= a does not)
    if (differ(ld16(x + (a - lead + 16 * q)), ld16(y + (b - lead + 16 * q)))) return false;
  return true;
}

// keys / idx: the pairs, sorted by the hash bits under `mask`.  A held blob with a later entry
// of its identity loses its output and gets its touched byte; a record anchor that is no
// DEL_KEY gets its plan (the entries that supply V, S and A; kNone: empty), its size and its
// flag.  Counts {touched, superseded, left absent, applied} into the counter lines.
__global__ __launch_bounds__(kApBlock) void apply_plan_kernel(ApIn s, const uint64_t* __restrict__ keys,
                                                              const uint32_t* __restrict__ idx, uint64_t mask,
                                                              const Side* __restrict__ side, uint64_t* __restrict__ sizes,
                                                              uint32_t* __restrict__ flags, uint4* __restrict__ plan,
                                                              uint8_t* __restrict__ touched,
                                                              unsigned long long* __restrict__ counter) {
  const uint64_t p = (uint64_t)blockIdx.x * kApBlock + threadIdx.x;
  const uint64_t N = s.na + s.n;
  const uint32_t g = p < N ? idx[p] : kNone;
  bool is_touched = false, is_super = false, is_absent = false, is_applied = false;
  if (g != kNone) {
    const uint64_t h = keys[p];
    const Side a = side[g];
    const uint8_t* const xa = g < s.na ? s.held : s.file;
    uint32_t nx = kNone;  // the next entry of this identity
    for (uint64_t q = p + 1; q < N; ++q) {
      const uint64_t hq = keys[q];
      if ((hq ^ h) & mask) break;
      const uint32_t j = idx[q];
      if (j == kNone) break;  // (sorted bits all ones: the non-participants follow the participants)
      if (hq != h) continue;  // another hash with the same sorted bits
      const Side b = side[j];
      if (b.sub != a.sub || b.klen != a.klen ||
          !ap_same_key(xa, a.koff, j < s.na ? s.held : s.file, b.koff, a.klen))
        continue;
      nx = j;
      break;
    }
    if (g < s.na) {
      if (nx != kNone) {
        is_super = nx < s.na;
        is_touched = !is_super;
        sizes[g] = 0;
        flags[g] = 0;
        if (touched) touched[g] = (uint8_t)(is_super ? K2H_AMD_APPLY_SUPERSEDED : K2H_AMD_APPLY_TOUCHED);
      }
    } else {
      is_applied = true;
      if (nx == kNone) {
        if (a.attrs & kDel) {
          is_absent = true;
        } else {
          uint32_t sv = kNone, ss = kNone, sa = kNone;
          uint64_t open = kV | kS | kA;
          auto take = [&](uint64_t w, uint32_t c) {
            if (w & kV) sv = c;
            if (w & kS) ss = c;
            if (w & kA) sa = c;
            open &= ~w;
          };
          take(a.attrs & 7u, g);
          for (uint64_t q = p; q > 0 && open; --q) {
            const uint64_t hq = keys[q - 1];
            if ((hq ^ h) & mask) break;
            if (hq != h) continue;
            const uint32_t c = idx[q - 1];
            const Side b = side[c];
            const bool rec = c >= s.na;
            if (rec && !(b.attrs & (open | kDel))) continue;  // writes no open field, whatever its identity
            if (b.sub != a.sub || b.klen != a.klen ||
                !ap_same_key(s.file, a.koff, rec ? s.file : s.held, b.koff, a.klen))
              continue;
            if (!rec) {
              take(open, c);  // the deciding held blob: the prior element
            } else if (b.attrs & kDel) {
              break;  // the open fields are empty
            } else {
              take(b.attrs & open, c);
            }
          }
          uint64_t lv, ls, la;
          field_of(s, sv, 0, lv);
          field_of(s, ss, 1, ls);
          field_of(s, sa, 2, la);
          plan[g - s.na] = make_uint4(sv, ss, sa, 0u);
          sizes[g] = (uint64_t)kHdr + a.klen + lv + ls + la;
          flags[g] = 1;
        }
      }
    }
  }
  ap_count(counter, 0, is_touched);
  ap_count(counter, 1, is_super);
  ap_count(counter, 2, is_absent);
  ap_count(counter, 3, is_applied);
}

// Part 2: one blob per anchor with a plan, by a group of kApGroup lanes, in GetElementToBinary's
// layout.  A field of kApLong bytes or more is left to the wave: its 64 lanes move one such field
// after the other.  8 waves per SIMD: at most 64 VGPRs, no scratch.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void apply_build_kernel(
    ApIn s, const uint64_t* __restrict__ place, const uint32_t* __restrict__ rank, const uint4* __restrict__ plan,
    uint8_t* __restrict__ out, uint64_t* __restrict__ out_off, uint64_t* __restrict__ origin) {
  const uint64_t i = (uint64_t)blockIdx.x * (256 / kApGroup) + threadIdx.x / kApGroup;
  const uint32_t q = threadIdx.x % kApGroup, lane = threadIdx.x & 63u;
  const uint64_t g = s.na + i;
  if (blockIdx.x == 0 && threadIdx.x == 0) out_off[rank[s.na + s.n]] = place[s.na + s.n];
  const uint8_t* src[3] = {nullptr, nullptr, nullptr};
  uint64_t len[3] = {0, 0, 0};
  uint8_t* to = nullptr;
  bool active = false;
  if (i < s.n) {
    const uint32_t rk = rank[g];
    active = rank[g + 1] != rk;
    if (active) {
      const uint64_t at = place[g];
      const uint4 pl = plan[i];
      const uint64_t koff = s.recs[i].key_off, klen = s.recs[i].key_len;
      src[0] = field_of(s, pl.x, 0, len[0]);
      src[1] = field_of(s, pl.y, 1, len[1]);
      src[2] = field_of(s, pl.z, 2, len[2]);
      uint8_t* const r = out + at;
      if (q == 0) {
        out_off[rk] = at;
        if (origin) origin[rk] = g;
      }
      if (q < 5) {
        const uint64_t vp = (uint64_t)kHdr + klen, sp = vp + len[0], ap = sp + len[1];
        uint64_t w0, w1;
        switch (q) {
          case 0: w0 = s.h1[i], w1 = s.h2[i]; break;
          case 1: w0 = klen, w1 = len[0]; break;
          case 2: w0 = len[1], w1 = len[2]; break;
          case 3: w0 = kHdr, w1 = vp; break;
          default: w0 = sp, w1 = ap; break;
        }
        *reinterpret_cast<u32x4_ua*>(r + 16 * q) =
            u32x4_ua{(uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32)};
      }
      group_copy<kApGroup>(r + kHdr, s.file + koff, klen, q);
      to = r + kHdr + klen;
    }
  }
#pragma unroll
  for (int f = 0; f < 3; ++f) {
    const bool wide = active && len[f] >= kApLong;
    if (active && len[f] && !wide) group_copy<kApGroup>(to, src[f], len[f], q);
    for (unsigned long long todo = __ballot(wide && q == 0); todo; todo &= todo - 1) {
      const int from = __ffsll((long long)todo) - 1;
      uint8_t* const d = (uint8_t*)ralle_shfl_u64((uint64_t)to, from);
      const uint8_t* const c = (const uint8_t*)ralle_shfl_u64((uint64_t)src[f], from);
      group_copy<64>(d, c, ralle_shfl_u64(len[f], from), lane);
    }
    to += len[f];
  }
}

// The call's temporaries (k2h_scratch.h) and the pinned words the results land in.  With
// N = na + n: two key and two index columns, the side records, a participant byte, a place and a
// rank (69 N bytes); per record a plan (16 bytes) and, when the call hashes the keys itself, two
// hashes; the tile counts and their scan, the counters with the stop word behind them, and the
// library's own storage.
struct ApScratch : DeviceScratch {
  void* pinned = nullptr;
};
PerDevice<ApScratch> g_apply;

constexpr size_t kApPinned = kCounterBytes + 64;  // the counter lines, the stop word, bytes, part-1 blobs, blobs

struct ApCols {
  SortStage<> st;
  Side* side;
  uint8_t* part;
  uint64_t* place;
  uint32_t* rank;
  uint4* plan;
  uint64_t *h1, *h2;
  unsigned long long* counter;  // the stop word right behind the lines: one memset clears both
  void* tmp;
  size_t total;
};

}  // namespace

// Returns a K2H_AMD_* code (the HIP error, if any, in *herr).  1 <= na + n <= 2^32 - 2; h1 and h2
// both given or both NULL (then hashed with `seed`).  Synchronises the stream once, to return
// counts and stop.  K2H_AMD_EINVAL: out != NULL and counts[1] > out_cap (counts, stop and touched
// are filled; out, out_off and origin are not written).
int launch_archive_apply(const void* held, uint64_t held_size, const uint64_t* held_off, uint64_t na,
                         const uint8_t* held_keep, const void* file, uint64_t size, const k2h_amd_archive_rec* recs,
                         uint64_t n, const uint8_t* consider, const uint64_t* h1, const uint64_t* h2, uint64_t seed,
                         void* out, uint64_t out_cap, uint64_t* out_off, uint64_t* origin, uint8_t* touched,
                         uint64_t* counts, uint64_t* stop, hipStream_t stream, hipError_t* herr) {
  *herr = hipSuccess;
  FirstError tr;
  auto done = [&](int rc) {
    *herr = tr.e;
    return !tr.ok() ? K2H_AMD_EHIP : rc;
  };
  const uint64_t N = na + n;
  const uint64_t nt = (N + kApBlock - 1) / kApBlock;
  ApScratch* const scp = g_apply.current(tr);
  SortStage<> st;
  PlaceRank<> pr;
  pr.measure(tr, N, stream);
  st.measure(tr, N, nt, stream);
  if (!tr.ok()) return done(K2H_AMD_OK);
  const size_t tmp_bytes = std::max(st.tmp_bytes(), pr.tmp_bytes());
  ApScratch& sc = *scp;
  std::lock_guard<std::mutex> lk(sc.mu);
  if (!sc.pinned) tr(hipHostMalloc(&sc.pinned, kApPinned, hipHostMallocDefault));
  if (!tr.ok()) return done(K2H_AMD_OK);
  unsigned long long* const host = (unsigned long long*)sc.pinned;
  auto layout = [&](void* base) {
    Carver c(base);
    ApCols k;
    k.st = st.take(c);
    k.side = c.take<Side>(N);
    k.part = c.take<uint8_t>(N);
    k.place = c.take<uint64_t>(N + 1);
    k.rank = c.take<uint32_t>(N + 1);
    k.plan = c.take<uint4>(n);
    k.h1 = c.take<uint64_t>(h1 ? 0 : n);
    k.h2 = c.take<uint64_t>(h1 ? 0 : n);
    k.counter = (unsigned long long*)c.bytes(kCounterBytes + 8);
    k.tmp = c.bytes(tmp_bytes);
    k.total = c.total();
    return k;
  };
  if (const int rc = sc.reserve(layout(nullptr).total, stream, herr)) return rc;
  const ApCols k = layout(sc.p);
  unsigned long long* const stopw = k.counter + kCounterBytes / 8;
  const unsigned grid = (unsigned)nt;

  k.st.clear(tr, stream);
  tr(hipMemsetAsync(k.counter, 0, kCounterBytes + 8, stream));
  if (tr.ok() && !h1 && n) {
    ArchiveHashOut ho;
    ho.h1 = k.h1, ho.h2 = k.h2;
    tr(launch_archive_prehash(file, size, recs, n, seed, ho, stream));
  }
  const ApIn s{(const uint8_t*)held, held_size, held_off, na,          held_keep,        (const uint8_t*)file,
               size,                 recs,      n,        consider,    h1 ? h1 : k.h1,   h1 ? h2 : k.h2};
  if (tr.ok()) {
    apply_gather_kernel<<<(unsigned)(N / kApBlock + 1), kApBlock, 0, stream>>>(s, k.part, k.st.hashes(), k.side, k.place,
                                                                               k.rank, touched, stopw);
    tr(hipGetLastError());
  }
  if (tr.ok()) {
    apply_count_kernel<<<grid, kApBlock, 0, stream>>>(k.part, na, n, stopw, k.st.tile_count);
    tr(hipGetLastError());
  }
  k.st.scan_tiles(tr, k.tmp, stream);
  ralle_compact<kApBlock>(tr, k.st, k.part, N, 0, stream);
  k.st.sort(tr, k.tmp, stream);
  if (tr.ok()) {
    apply_plan_kernel<<<grid, kApBlock, kPlanLds, stream>>>(s, k.st.keys_out, k.st.idx_out, k.st.mask(), k.side, k.place,
                                                            k.rank, k.plan, touched, k.counter);
    tr(hipGetLastError());
  }
  pr.scan(tr, k.tmp, k.place, k.rank, stream);
  unsigned long long* const tail = host + kCounterBytes / 8;  // stop word, bytes, part-1 blobs | blobs
  if (tr.ok()) tr(hipMemcpyAsync(host, k.counter, kCounterBytes + 8, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(hipMemcpyAsync(tail + 1, k.place + N, 8, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(hipMemcpyAsync(tail + 2, k.rank + na, 4, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(hipMemcpyAsync(tail + 3, k.rank + N, 4, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(sc.mark_done(stream));
  if (tr.ok()) tr(hipStreamSynchronize(stream));
  if (!tr.ok()) return done(K2H_AMD_OK);
  const uint64_t part1 = (uint32_t)tail[2], blobs = (uint32_t)tail[3];
  counts[0] = blobs;
  counts[1] = tail[1];
  counts[2] = part1;
  for (int w = 0; w < 4; ++w) counts[3 + w] = counter_sum(host, w);
  *stop = n - tail[0];
  if (!out) return done(K2H_AMD_OK);
  if (counts[1] > out_cap) return done(K2H_AMD_EINVAL);
  if (na) {
    ralle_place_copy_kernel<false, kApBlock, kApTabPieces>
        <<<(unsigned)((na + kApBlock - 1) / kApBlock), kApBlock, 0, stream>>>(
        s.held, held_off, na, k.place, k.rank, nullptr, (uint8_t*)out, out_off, origin);
    tr(hipGetLastError());
  }
  if (tr.ok() && blobs > part1) {
    const uint64_t per = 256 / kApGroup;
    apply_build_kernel<<<(unsigned)((n + per - 1) / per), 256, 0, stream>>>(s, k.place, k.rank, k.plan, (uint8_t*)out,
                                                                            out_off, origin);
    tr(hipGetLastError());
  }
  if (tr.ok() && !na && blobs == part1) tr(hipMemsetAsync(out_off, 0, 8, stream));
  if (tr.ok()) tr(sc.mark_done(stream));
  return done(K2H_AMD_OK);
}

}  // namespace k2h
