// k2hash_amd -- the barrier records of a transaction log, OW_VAL and RENAME, executed on a held
// RALLEDATA stream in place (include/k2hash_amd.h section 5d: k2h_amd_archive_barrier).
//
// k2h_amd_archive_apply (k2h_archive_apply.hip) stops at the first OW_VAL or RENAME.  This call
// executes that record -- for OW_VAL the whole run of chunks on the one key that follows it, up
// to K2H_AMD_BARRIER_MAX_RUN records -- by Load's arms (lib/k2harchive.cc:343-362): the held
// stream is an arena with room behind its last blob, the call clears the keep byte of every
// participant copy of the addressed identity and appends the one blob that holds the new
// element, in GetElementToBinary's layout.  Nothing of the arena is moved: the next apply
// compacts the dead copies away.
//
// All on the caller's stream:
//   judge    one wave.  Record b and its exdata: the outcome so far.  For OW_VAL the run: 64
//            records per trip, a ballot of the lanes whose record continues the run; the lanes
//            before the first that does not leave their write in the patch table (offset,
//            length, file offset), in log order.
//   locate   one lane per held blob, launched when a blob is held: keep byte, span, header and
//            classify (k2h_ralle_header.h), the stored hash, subhash and key length against the
//            old identity (and the new one of a RENAME), then the key bytes.  An atomic max of
//            j + 1 per identity, skipped when the word already holds more; the indices of the
//            old identity's copies go to a list, one atomic per wave.  Nothing of a blob is read
//            but its offsets, its header and, when those agree, its key.
//   size     one wave.  The outcome, the deciding blob's segments, the final value length (the
//            maximum of the old length and every patch's end) and whether a byte of the value is
//            left uncovered: a leftmost uncovered byte lies at the old length or at a patch's
//            end, so each such place is tested against every patch.  The plan of the build and
//            the eight result words; the host reads the words after the call's one
//            synchronisation and judges the capacity.
//   build    the appended blob as the 16-byte pieces of its destination, a grid-stride loop over
//            them.  A whole piece that lies in one segment with one source -- the key, the
//            subkeys, the attrs, one patch, the old value under no patch, or the gap -- is one
//            unaligned load and one aligned store; every other piece (the header, a segment
//            boundary, a patch boundary, the two ends) is resolved byte by byte, each byte from
//            the last patch that holds it.  Overlapping patches are never copied one over the
//            other.  The same launch clears the listed keep bytes and writes held_off[na + 1]
//            and held_keep[na].
//
// Reads.  No byte outside [0, held_size) of the held stream or [0, size) of the file, except
// within the aligned 16 bytes that hold a valid byte (the key compares, as in
// k2h_archive_apply.hip); the build loads exact source bytes.  Writes.  held[held_size,
// held_size + result[2]), held_off[na + 1], held_keep[na] and the listed keep bytes, all by the
// build kernel, which is launched only for an EXECUTED outcome that fits held_cap.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"
#include "k2h_ralle_header.h"
#include "k2h_ralle_ident.h"

namespace k2h {
namespace {

constexpr int kBrBlock = 256;                      // locate and build: threads per block
constexpr int kBrRun = K2H_AMD_BARRIER_MAX_RUN;    // the patch table's entries
constexpr unsigned kBrBuildBlocks = 4096;          // build: at most this many blocks stride over the pieces
static_assert(kBrRun % 64 == 0, "the judge walks the run 64 records per trip");

struct BrIn {
  const uint8_t* held;
  uint64_t held_size;
  const uint64_t* held_off;
  uint64_t na;
  const uint8_t* held_keep;
  const uint8_t* file;
  uint64_t size;
  const k2h_amd_archive_rec* recs;
  uint64_t n, b;
  const uint8_t* consider;
  const uint64_t* hash;  // h1, h2, new_h1, new_h2 of record b
};

// One OW_VAL of the run: `len` bytes from file offset `foff` written at `off` of the value.
struct Patch {
  uint64_t off, len, foff;
};

// What the judge leaves for locate and size.
struct BrState {
  uint32_t outcome;    // so far: EXECUTED, BAD_RECORD or NOT_A_BARRIER
  uint32_t type;       // 4 or 6
  uint32_t np;         // OW_VAL: the run's records
  uint32_t check_new;  // RENAME: the new key's bytes are not the old key's
  uint64_t koff, klen;    // the record's key in the file
  uint64_t nkoff, nklen;  // RENAME: the new key
  uint64_t aoff, alen;    // RENAME: the record's attrs; length 0: the old blob's
  unsigned long long decide[2];  // 1 + the last participant of the old / the new identity
  unsigned long long nlist;      // the old identity's participants
};

// What size leaves for build.  The value is the old value's bytes [0, oldlen) under the patches.
struct BrPlan {
  uint64_t hdr[10];
  const uint8_t* src[4];  // key, old value, subkeys, attrs
  uint64_t len[4];        // key, final value, subkeys, attrs
  uint64_t oldlen;
  uint64_t total;
  uint64_t nclear;
  uint64_t np;
};
static_assert(sizeof(BrPlan) % 8 == 0 && sizeof(Patch) == 24, "copied to LDS as 8-byte words");

__device__ __forceinline__ bool in_file(const BrIn& s, uint64_t off, uint64_t len) {
  return off <= s.size && len <= s.size - off;
}

// Chunk 0 of the key at offset a of buffer f whose chunks end at its last byte; only the key's
// own bytes where the 16 bytes would begin below the buffer (k2h_archive_apply.hip).
__device__ __forceinline__ uint4 br_chunk0(const uint8_t* f, uint64_t a, uint32_t lead) {
  if (a >= lead) return mask_lead(ld16(f + (a - lead)), lead);
  return chunk0_from_bytes(lead, [=](uint32_t j) { return (uint32_t)f[a + j]; });
}

// Two keys of one length kl >= 1, at offset a of buffer x and offset b of buffer y.
__device__ __forceinline__ bool br_same_key(const uint8_t* x, uint64_t a, const uint8_t* y, uint64_t b, uint64_t kl) {
  const uint64_t k = (kl + 15) >> 4;
  const uint32_t lead = (uint32_t)(16 * k - kl);
  if (differ(br_chunk0(x, a, lead), br_chunk0(y, b, lead))) return false;
  for (uint64_t q = 1; q < k; ++q)
    if (differ(ld16(x + (a - lead + 16 * q)), ld16(y + (b - lead + 16 * q)))) return false;
  return true;
}

// An OW_VAL that Load fails (lib/k2harchive.cc:344, lib/k2hdaccess.cc:266, :394) or whose exdata
// would overflow OWVAL_EXDATA.  off: the exdata bytes over a zeroed off_t.
__device__ __forceinline__ bool ow_bad(const BrIn& s, const k2h_amd_archive_rec& r, uint64_t& off) {
  off = 0;
  const uint64_t xl = r.exdata_len, xo = r.exdata_off;
  if (xl < 1 || xl > 8 || !in_file(s, xo, xl) || r.val_len == 0 || !in_file(s, r.val_off, r.val_len)) return true;
  for (uint32_t k = 0; k < (uint32_t)xl; ++k) off |= (uint64_t)s.file[xo + k] << (8 * k);
  return (int64_t)off < 0;
}

__global__ __launch_bounds__(64) void barrier_judge_kernel(BrIn s, BrState* __restrict__ st, Patch* __restrict__ patch) {
  const uint32_t lane = threadIdx.x;
  const k2h_amd_archive_rec& r = s.recs[s.b];
  const int64_t type = r.type;
  const uint64_t koff = r.key_off, klen = r.key_len;
  uint32_t outcome = K2H_AMD_BARRIER_NOT_A_BARRIER, np = 0, check_new = 0;
  uint64_t aoff = 0, alen = 0;
  if (r.status == 0 && (!s.consider || s.consider[s.b]) && (type == 4 || type == 6) && klen >= 1 &&
      in_file(s, koff, klen)) {
    outcome = K2H_AMD_BARRIER_EXECUTED;
    if (type == 6) {
      const uint64_t xo = r.exdata_off, xl = r.exdata_len;
      if (xl == 0 || !in_file(s, xo, xl)) {
        outcome = K2H_AMD_BARRIER_BAD_RECORD;
      } else {
        check_new = !(xl == klen && br_same_key(s.file, koff, s.file, xo, klen));
        if (r.attrs_len && in_file(s, r.attrs_off, r.attrs_len)) aoff = r.attrs_off, alen = r.attrs_len;
      }
    } else {
      uint64_t off;
      if (ow_bad(s, r, off)) outcome = K2H_AMD_BARRIER_BAD_RECORD;
    }
  }
  if (outcome == K2H_AMD_BARRIER_EXECUTED && type == 4) {
    bool open = true;
    for (uint32_t t = 0; t < kBrRun / 64 && open; ++t) {
      const uint64_t at = 64ull * t + lane;  // (b < n <= 2^63: no wrap below)
      bool ok = false;
      uint64_t off = 0, vlen = 0, voff = 0;
      if (at < s.n - s.b) {
        const k2h_amd_archive_rec& c = s.recs[s.b + at];
        if (c.status == 0 && (!s.consider || s.consider[s.b + at]) && c.type == 4 && c.key_len == klen &&
            in_file(s, c.key_off, klen) && !ow_bad(s, c, off) && br_same_key(s.file, koff, s.file, c.key_off, klen)) {
          ok = true;
          vlen = c.val_len, voff = c.val_off;
        }
      }
      const unsigned long long m = __ballot(ok);
      const uint32_t run = ~m ? (uint32_t)__ffsll((long long)~m) - 1 : 64u;
      if (lane < run) patch[at] = Patch{off, vlen, voff};
      np += run;
      open = run == 64;
    }
  }
  if (lane == 0) {
    st->outcome = outcome;
    st->type = (uint32_t)type;
    st->np = np;
    st->check_new = check_new;
    st->koff = koff, st->klen = klen;
    st->nkoff = r.exdata_off, st->nklen = r.exdata_len;
    st->aoff = aoff, st->alen = alen;
    st->decide[0] = st->decide[1] = 0;
    st->nlist = 0;
  }
}

__global__ __launch_bounds__(kBrBlock) void barrier_locate_kernel(BrIn s, BrState* __restrict__ st,
                                                                  uint32_t* __restrict__ list) {
  if (st->outcome != K2H_AMD_BARRIER_EXECUTED) return;
  const uint64_t j = (uint64_t)blockIdx.x * kBrBlock + threadIdx.x;
  bool old_hit = false, new_hit = false;
  if (j < s.na && s.held_keep[j]) {
    const uint64_t o = s.held_off[j], e = s.held_off[j + 1];
    if (e >= o && e <= s.held_size && e - o >= (uint64_t)kHdr) {
      uint64_t f[10];
      load_fields(s.held + o, f);
      if (classify(f, e - o) == K2H_AMD_RALLE_OK) {
        if (f[0] == s.hash[0] && f[1] == s.hash[1] && f[2] == st->klen)
          old_hit = br_same_key(s.held, o + f[6], s.file, st->koff, f[2]);
        if (st->check_new && f[0] == s.hash[2] && f[1] == s.hash[3] && f[2] == st->nklen)
          new_hit = br_same_key(s.held, o + f[6], s.file, st->nkoff, f[2]);
      }
    }
  }
  // Blocks start roughly in index order: the words soon hold what few later copies can raise.
  if (old_hit && j + 1 > *(volatile unsigned long long*)&st->decide[0]) atomicMax(&st->decide[0], j + 1);
  if (new_hit && j + 1 > *(volatile unsigned long long*)&st->decide[1]) atomicMax(&st->decide[1], j + 1);
  const unsigned long long m = __ballot(old_hit);
  if (m) {
    const uint32_t lane = threadIdx.x & 63u, first = (uint32_t)__ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == first) base = atomicAdd(&st->nlist, (unsigned long long)__popcll(m));
    base = ralle_shfl_u64(base, (int)first);
    if (old_hit) list[base + __popcll(m & ((1ull << lane) - 1))] = (uint32_t)j;
  }
}

__global__ __launch_bounds__(64) void barrier_size_kernel(BrIn s, const BrState* __restrict__ st,
                                                          const Patch* __restrict__ patch, BrPlan* __restrict__ plan,
                                                          uint64_t* __restrict__ result) {
  __shared__ uint64_t t_off[kBrRun], t_end[kBrRun], lane_max[64];
  const uint32_t lane = threadIdx.x;
  const uint32_t np = st->np, type = st->type;
  const uint64_t d = st->decide[0];
  uint32_t outcome = st->outcome;
  if (outcome == K2H_AMD_BARRIER_EXECUTED && type == 6) {
    if (!d) outcome = K2H_AMD_BARRIER_NOT_FOUND;
    else if (st->check_new && st->decide[1]) outcome = K2H_AMD_BARRIER_NEW_EXISTS;
  }
  if (outcome != K2H_AMD_BARRIER_EXECUTED) {
    if (lane < 8) result[lane] = lane == 0 ? outcome : lane == 5 ? ~0ull : 0ull;
    return;
  }
  // the deciding blob's segments (none: an OW_VAL on a key that is not held)
  uint64_t f[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  const uint8_t* blob = s.held;
  if (d) {
    blob = s.held + s.held_off[d - 1];
    load_fields(blob, f);
  }
  uint64_t mx = 0;
  for (uint32_t k = lane; k < np; k += 64) {
    const Patch p = patch[k];
    t_off[k] = p.off;
    t_end[k] = p.off + p.len;
    mx = mx > p.off + p.len ? mx : p.off + p.len;
  }
  lane_max[lane] = mx;
  __syncthreads();
  const uint64_t oldlen = f[3];
  uint64_t vlen = oldlen;
  for (uint32_t k = 0; k < 64; ++k) vlen = vlen > lane_max[k] ? vlen : lane_max[k];
  // place c = the old length (k == np) or a patch's end: a gap begins there when it lies inside
  // the value, at or behind the old value's end, and inside no patch
  bool gap = false;
  for (uint32_t k = lane; k <= np; k += 64) {
    const uint64_t c = k == np ? oldlen : t_end[k];
    if (c < oldlen || c >= vlen) continue;
    bool covered = false;
    for (uint32_t q = 0; q < np && !covered; ++q) covered = t_off[q] <= c && c < t_end[q];
    gap |= !covered;
  }
  const bool any_gap = __ballot(gap) != 0;
  if (lane) return;
  const bool ren = type == 6;
  BrPlan p;
  p.src[0] = s.file + (ren ? st->nkoff : st->koff);
  p.len[0] = ren ? st->nklen : st->klen;
  p.src[1] = blob + f[7];
  p.len[1] = vlen;
  p.src[2] = blob + f[8];
  p.len[2] = f[4];
  p.src[3] = ren && st->alen ? s.file + st->aoff : blob + f[9];
  p.len[3] = ren && st->alen ? st->alen : f[5];
  p.oldlen = oldlen;
  p.total = (uint64_t)kHdr + p.len[0] + p.len[1] + p.len[2] + p.len[3];
  p.nclear = st->nlist;
  p.np = np;
  p.hdr[0] = s.hash[ren ? 2 : 0];
  p.hdr[1] = s.hash[ren ? 3 : 1];
  uint64_t pos = kHdr;
  for (int g = 0; g < 4; ++g) {
    p.hdr[2 + g] = p.len[g];
    p.hdr[6 + g] = pos;
    pos += p.len[g];
  }
  *plan = p;
  result[0] = K2H_AMD_BARRIER_EXECUTED;
  result[1] = ren ? 1 : np;
  result[2] = p.total;
  result[3] = (d ? 0u : K2H_AMD_BARRIER_CREATED) | (any_gap ? K2H_AMD_BARRIER_GAP : 0u);
  result[4] = p.nclear;
  result[5] = d ? d - 1 : ~0ull;
  result[6] = vlen;
  result[7] = 0;
}

// Byte v of the value: from the last patch that holds it, else the old value's, else a gap's zero.
__device__ __forceinline__ uint32_t value_byte(const BrPlan& P, const Patch* tab, const uint8_t* file, uint64_t v) {
  for (uint32_t q = (uint32_t)P.np; q-- > 0;) {
    const uint64_t po = tab[q].off;
    if (po <= v && v - po < tab[q].len) return file[tab[q].foff + (v - po)];
  }
  return v < P.oldlen ? P.src[1][v] : 0u;
}

// Byte x of the appended blob.
__device__ __forceinline__ uint32_t blob_byte(const BrPlan& P, const Patch* tab, const uint8_t* file, uint64_t x) {
  if (x < (uint64_t)kHdr) return (uint32_t)(P.hdr[x >> 3] >> (8 * (x & 7))) & 0xFFu;
  x -= kHdr;
  if (x < P.len[0]) return P.src[0][x];
  x -= P.len[0];
  if (x < P.len[1]) return value_byte(P, tab, file, x);
  x -= P.len[1];
  if (x < P.len[2]) return P.src[2][x];
  return P.src[3][x - P.len[2]];
}

// The 16 source bytes of the whole piece at byte x of the blob, when one source has them all;
// zero: the piece lies in a gap; neither: the piece is mixed.
__device__ __forceinline__ const uint8_t* piece_source(const BrPlan& P, const Patch* tab, const uint8_t* file,
                                                       uint64_t x, bool& zero) {
  zero = false;
  if (x < (uint64_t)kHdr) return nullptr;
  x -= kHdr;
  if (x < P.len[0]) return P.len[0] - x >= 16 ? P.src[0] + x : nullptr;
  x -= P.len[0];
  if (x < P.len[1]) {
    if (P.len[1] - x < 16) return nullptr;
    for (uint32_t q = (uint32_t)P.np; q-- > 0;) {
      const uint64_t po = tab[q].off, pe = po + tab[q].len;
      if (po < x + 16 && pe > x) return po <= x && pe >= x + 16 ? file + tab[q].foff + (x - po) : nullptr;
    }
    if (x + 16 <= P.oldlen) return P.src[1] + x;
    zero = x >= P.oldlen;
    return nullptr;
  }
  x -= P.len[1];
  if (x < P.len[2]) return P.len[2] - x >= 16 ? P.src[2] + x : nullptr;
  x -= P.len[2];
  return P.len[3] - x >= 16 ? P.src[3] + x : nullptr;
}

__global__ __launch_bounds__(kBrBlock) void barrier_build_kernel(uint8_t* __restrict__ held, uint64_t held_size,
                                                                 uint64_t* __restrict__ held_off,
                                                                 uint8_t* __restrict__ held_keep, uint64_t na,
                                                                 const uint8_t* __restrict__ file,
                                                                 const BrPlan* __restrict__ plan,
                                                                 const Patch* __restrict__ patch,
                                                                 const uint32_t* __restrict__ list) {
  __shared__ BrPlan P;
  __shared__ Patch tab[kBrRun];
  const uint32_t words = (uint32_t)(sizeof(BrPlan) / 8);
  if (threadIdx.x < words) reinterpret_cast<uint64_t*>(&P)[threadIdx.x] = reinterpret_cast<const uint64_t*>(plan)[threadIdx.x];
  const uint32_t np = (uint32_t)plan->np;
  for (uint32_t k = threadIdx.x; k < 3 * np; k += kBrBlock)
    reinterpret_cast<uint64_t*>(tab)[k] = reinterpret_cast<const uint64_t*>(patch)[k];
  __syncthreads();
  const uint64_t g = (uint64_t)blockIdx.x * kBrBlock + threadIdx.x, stride = (uint64_t)gridDim.x * kBrBlock;
  for (uint64_t k = g; k < P.nclear; k += stride) held_keep[list[k]] = 0;
  if (g == 0) {
    held_off[na + 1] = held_size + P.total;
    held_keep[na] = 1;
  }
  uint8_t* const out = held + held_size;
  const uint64_t lead = (uint64_t)(uintptr_t)out & 15u, total = P.total;
  const uint64_t pieces = (lead + total + 15) >> 4;
  for (uint64_t p = g; p < pieces; p += stride) {
    const uint64_t lo = p ? 16 * p - lead : 0, hi = 16 * p - lead + 16 < total ? 16 * p - lead + 16 : total;
    if (hi - lo == 16) {
      bool zero;
      const uint8_t* const src = piece_source(P, tab, file, lo, zero);
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (src) {
        v = ld16(src);
      } else if (!zero) {
        uint64_t w0 = 0, w1 = 0;
        for (uint32_t k = 0; k < 8; ++k) {
          w0 |= (uint64_t)blob_byte(P, tab, file, lo + k) << (8 * k);
          w1 |= (uint64_t)blob_byte(P, tab, file, lo + 8 + k) << (8 * k);
        }
        v = make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
      }
      *reinterpret_cast<uint4*>(out + lo) = v;
    } else {
      for (uint64_t x = lo; x < hi; ++x) out[x] = (uint8_t)blob_byte(P, tab, file, x);
    }
  }
}

// The call's temporaries (k2h_scratch.h) and the pinned words the result lands in: the state, the
// plan, the result, record b's four hashes, the patch table and 4 bytes per held blob for the list.
struct BrScratch : DeviceScratch {
  void* pinned = nullptr;
};
PerDevice<BrScratch> g_barrier;

struct BrCols {
  BrState* st;
  BrPlan* plan;
  uint64_t* result;
  uint64_t* hash;
  Patch* patch;
  uint32_t* list;
  size_t total;
};

}  // namespace

int launch_archive_barrier(void* held, uint64_t held_size, uint64_t held_cap, uint64_t* held_off, uint64_t na,
                           uint8_t* held_keep, const void* file, uint64_t size, const k2h_amd_archive_rec* recs,
                           uint64_t n, uint64_t b, const uint8_t* consider, const uint64_t* h1, const uint64_t* h2,
                           const uint64_t* new_h1, const uint64_t* new_h2, uint64_t seed, bool count_only,
                           uint64_t* result, hipStream_t stream, hipError_t* herr) {
  *herr = hipSuccess;
  FirstError tr;
  auto done = [&](int rc) {
    *herr = tr.e;
    return !tr.ok() ? K2H_AMD_EHIP : rc;
  };
  BrScratch* const scp = g_barrier.current(tr);
  if (!tr.ok()) return done(K2H_AMD_OK);
  BrScratch& sc = *scp;
  std::lock_guard<std::mutex> lk(sc.mu);
  if (!sc.pinned) tr(hipHostMalloc(&sc.pinned, 64, hipHostMallocDefault));
  if (!tr.ok()) return done(K2H_AMD_OK);
  auto layout = [&](void* base) {
    Carver c(base);
    BrCols k;
    k.st = c.take<BrState>(1);
    k.plan = c.take<BrPlan>(1);
    k.result = c.take<uint64_t>(8);
    k.hash = c.take<uint64_t>(4);
    k.patch = c.take<Patch>(kBrRun);
    k.list = c.take<uint32_t>(na);
    k.total = c.total();
    return k;
  };
  if (const int rc = sc.reserve(layout(nullptr).total, stream, herr)) return rc;
  const BrCols k = layout(sc.p);
  if (h1) {
    const uint64_t* const from[4] = {h1 + b, h2 + b, new_h1 + b, new_h2 + b};
    for (int w = 0; w < 4 && tr.ok(); ++w)
      tr(hipMemcpyAsync(k.hash + w, from[w], 8, hipMemcpyDeviceToDevice, stream));
  } else {
    ArchiveHashOut ho;
    ho.h1 = k.hash, ho.h2 = k.hash + 1, ho.new_h1 = k.hash + 2, ho.new_h2 = k.hash + 3;
    tr(launch_archive_prehash(file, size, recs + b, 1, seed, ho, stream));
  }
  const BrIn s{(const uint8_t*)held, held_size, held_off, na, held_keep, (const uint8_t*)file, size, recs, n, b, consider,
               k.hash};
  if (tr.ok()) {
    barrier_judge_kernel<<<1, 64, 0, stream>>>(s, k.st, k.patch);
    tr(hipGetLastError());
  }
  if (tr.ok() && na) {
    barrier_locate_kernel<<<(unsigned)((na + kBrBlock - 1) / kBrBlock), kBrBlock, 0, stream>>>(s, k.st, k.list);
    tr(hipGetLastError());
  }
  if (tr.ok()) {
    barrier_size_kernel<<<1, 64, 0, stream>>>(s, k.st, k.patch, k.plan, k.result);
    tr(hipGetLastError());
  }
  if (tr.ok()) tr(hipMemcpyAsync(sc.pinned, k.result, 64, hipMemcpyDeviceToHost, stream));
  if (tr.ok()) tr(sc.mark_done(stream));
  if (tr.ok()) tr(hipStreamSynchronize(stream));
  if (!tr.ok()) return done(K2H_AMD_OK);
  for (int w = 0; w < 8; ++w) result[w] = ((const uint64_t*)sc.pinned)[w];
  if (count_only || result[0] != K2H_AMD_BARRIER_EXECUTED) return done(K2H_AMD_OK);
  if (result[2] > held_cap - held_size) return done(K2H_AMD_EINVAL);
  const uint64_t pieces = (result[2] + 15) / 16 + 1;
  const uint64_t blocks = (pieces + kBrBlock - 1) / kBrBlock;
  barrier_build_kernel<<<(unsigned)(blocks < kBrBuildBlocks ? blocks : kBrBuildBlocks), kBrBlock, 0, stream>>>(
      (uint8_t*)held, held_size, held_off, held_keep, na, (const uint8_t*)file, k.plan, k.patch, k.list);
  tr(hipGetLastError());
  if (tr.ok()) tr(sc.mark_done(stream));
  return done(K2H_AMD_OK);
}

}  // namespace k2h
